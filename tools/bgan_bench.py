#!/usr/bin/env python
"""NSGAN against the Bayesian GAN in microseconds per iteration: 784-400-20, bs = 256, whole epochs on the graph path,
plus gm_sghmc_step alone against its bandwidth floor.

    python tools/bgan_bench.py [--n-train 50000] [--reps 5] [--only NAME] [--out profiles/bgan_bench.json]

Each repetition times one train(1) call of each trainer (host sampler replay, graph launches and the epoch's loss
read-back included, the same for both) with a synchronize on each side; the median over repetitions is reported, after
one warm-up epoch that captures the graphs.  The SGHMC launch is timed with HIP events over 200 back-to-back launches on
the (4, 2) model's generator and critic buffers; its floor is 5 x 4 B x parameters (read g, theta, v; write theta, v)
at 6.3 TB/s.  Synthetic binary images."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))

B = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="nsgan, bgan11 or bgan42 (the profile runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgan_bench.json"))
    a = ap.parse_args()
    import torch
    import bayes_gan
    import ns_gan

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=B,
                                               shuffle=True)
    steps = (a.n_train + B - 1) // B
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "batch": B, "n_train": a.n_train,
                      "iterations_per_epoch": steps, "reps": a.reps, "D_steps": 1}}
    runs = (("nsgan", lambda: ns_gan.NSGANTrainer(ns_gan.NSGAN(784, 400, 20), dl(a.n_train), dl(B), dl(B))),
            ("bgan11", lambda: bayes_gan.BayesGANTrainer(bayes_gan.BayesGAN(num_gen=1, num_disc=1), dl(a.n_train),
                                                         dl(B), dl(B))),
            ("bgan42", lambda: bayes_gan.BayesGANTrainer(bayes_gan.BayesGAN(num_gen=4, num_disc=2), dl(a.n_train),
                                                         dl(B), dl(B))))
    last = None
    for name, mk in runs:
        if a.only and name != a.only:
            continue
        torch.manual_seed(1234)
        tr = mk()
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(1)                                  # warm-up: graphs captured
            us = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train(1)
                torch.cuda.synchronize()
                us.append((time.perf_counter() - t0) * 1e6 / steps)
        out[name] = {"us_per_iteration_median": statistics.median(us), "us_per_iteration": us}
        print(name, "%.2f us / iteration (median of %d epochs)" % (statistics.median(us), a.reps), flush=True)
        last = tr
    if a.only:
        return 0
    for n in ("bgan11", "bgan42"):
        out["ratio_%s_over_nsgan" % n] = out[n]["us_per_iteration_median"] / out["nsgan"]["us_per_iteration_median"]
        print("%s / NSGAN = %.3f" % (n, out["ratio_%s_over_nsgan" % n]))
    from generative_models_amd import ops_fused
    eng = last._engine
    sg = {}
    for side, f, segs, lr in (("generators", eng.fG, eng.segG, eng.lr[1:2]), ("critics", eng.fD, eng.segD,
                                                                               eng.lr[0:1])):
        params = sum(p.numel() for p in f.params)
        launch = lambda: ops_fused.sghmc_step(f.flat, f.grad, f.v, segs, lr, 0.0, 0.0, 0.0, 0, t=0)
        for _ in range(10):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / 200
        floor = 5 * 4 * params / 6.3e12 * 1e6
        sg[side] = {"parameters": params, "us_per_launch": us, "bandwidth_floor_us": floor,
                    "ratio_to_floor": us / floor}
        print("sghmc %s: %d parameters, %.2f us / launch, floor %.2f us" % (side, params, us, floor))
    out["sghmc_step"] = sg
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
