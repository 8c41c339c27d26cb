#!/usr/bin/env python
"""PD-WGAN against its two halves in microseconds per training batch: 784-400-20, bs = 512, whole epochs on the graph
path, one process.

    python tools/pdwgan_bench.py [--n-train 50000] [--reps 5] [--out profiles/pdwgan_bench.json]

A PD-WGAN batch does about the work of one plain autoencoder batch (ae.py) plus one WGAN-GP iteration with D_steps = 1
(w_gp_gan.py); the goal is its time <= (their sum) * 1.10.  The autoencoder and PD-WGAN are timed like
tools/aae_bench.py (HIP events around the engine's training pass, validation excluded); the WGAN-GP iteration with HIP
events around train(1, D_steps=1) (its epoch-end read-back included: one copy per 98 iterations).  Median over the
repetitions after one warm-up epoch that captures the graphs.  Synthetic binary images."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdwgan_bench.json"))
    a = ap.parse_args()
    import torch
    import ae
    import pdw_gan
    import w_gp_gan
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    xv, yv = x[:512], y[:512]
    dl = lambda *t: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(*t), batch_size=512, shuffle=True)
    steps = (a.n_train + 511) // 512
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": steps, "reps": a.reps}}

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps

    def report(name, us):
        out[name] = {"us_per_batch_median": statistics.median(us), "us_per_batch": us}
        print(name, "%.2f us / batch (median of %d epochs)" % (statistics.median(us), a.reps), flush=True)

    for name, mk in (("ae", lambda: ae.AutoencoderTrainer(ae.Autoencoder(784, 400), dl(x, y), dl(xv, yv), dl(xv, yv))),
                     ("pdwgan", lambda: pdw_gan.PDWGANTrainer(pdw_gan.PDWGAN(), dl(x, y), dl(xv, yv), dl(xv, yv)))):
        torch.manual_seed(1234)
        tr = mk()
        tr.train(1, quiet=True)                          # warm-up: graphs captured
        eng, data = tr._engine, tr._device_data(tr.train_iter)
        assert eng is not None, name
        report(name, [timed(lambda: eng.run_pass(data, trainers._epoch_order(tr.train_iter), True, 0))
                      for _ in range(a.reps)])
    torch.manual_seed(1234)
    tr = w_gp_gan.WGPGANTrainer(w_gp_gan.WGPGAN(784, 400, 20), dl(x, y), dl(xv, yv), dl(xv, yv))

    def wgp_epoch():
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(1, D_steps=1)
    wgp_epoch()
    assert tr._engine is not None
    report("wgan_gp", [timed(wgp_epoch) for _ in range(a.reps)])
    parts = out["ae"]["us_per_batch_median"] + out["wgan_gp"]["us_per_batch_median"]
    out["sum_ae_wgan_gp_us"] = parts
    out["ratio_pdwgan_over_sum"] = out["pdwgan"]["us_per_batch_median"] / parts
    out["goal"] = "pdwgan <= 1.10 * (ae + wgan_gp)"
    out["goal_met"] = bool(out["ratio_pdwgan_over_sum"] <= 1.10)
    print("PD-WGAN / (AE + WGAN-GP) = %.3f, goal (<= 1.10) %s" % (out["ratio_pdwgan_over_sum"],
                                                                "met" if out["goal_met"] else "missed"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
