#!/usr/bin/env python
"""IWAE against the VAE in microseconds per training batch: 784-400-20, bs = 512, whole epochs on the graph path.

    python tools/iwae_bench.py [--n-train 50176] [--reps 5] [--general-batches 20] [--out profiles/iwae_bench.json]

Rows: the VAE at bs 512; the VAE at bs 2560 (the decoder rows of k = 5); the fused IWAE at k = 1, 5, 50; the IWAE's
general path (autograd over the fused linear kernels) at k = 5.  tools/dvae_bench.py's protocol: each repetition times
one training pass of each fused model in turn (the models alternate, so drift hits all alike) with HIP events
(validation excluded: the engine's run_pass for the training set); the median over repetitions is reported, after one
warm-up epoch per model that captures the graphs.  The general path has no engine: its row is the median over
repetitions of --general-batches training batches (zero_grad, compute_batch, backward, optimizer step) between HIP
events, after as many warm-up batches.  Synthetic binary images (the bit-packed dataset, as get_data() gives);
50176 = 98 batches of 512."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--general-batches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iwae_bench.json"))
    a = ap.parse_args()
    import torch
    import iwae
    import vae
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda bs, n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=bs,
                                                        shuffle=True)
    its = lambda bs: (dl(bs), dl(bs, bs), dl(bs, bs))
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": (a.n_train + 511) // 512, "reps": a.reps,
                      "general_batches": a.general_batches}}
    models = {"vae_b512": (512, lambda: vae.VAETrainer(vae.VAE(), *its(512))),
              "vae_b2560": (2560, lambda: vae.VAETrainer(vae.VAE(), *its(2560)))}
    for k in (1, 5, 50):
        models["iwae_k%d" % k] = (512, lambda k=k: iwae.IWAETrainer(iwae.IWAE(), *its(512), k=k, seed=0))
    runs = {}
    for name, (bs, mk) in models.items():
        torch.manual_seed(1234)
        tr = mk()
        tr.train(1, quiet=True)                          # warm-up: graphs captured
        assert type(tr._engine).__name__ == ("VAEEngine" if name.startswith("vae") else "IWAEEngine")
        runs[name] = (tr, tr._engine, tr._device_data(tr.train_iter), (a.n_train + bs - 1) // bs, [])
    for _ in range(a.reps):
        for name, (tr, eng, data, steps, us) in runs.items():
            perm = trainers._epoch_order(tr.train_iter)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.run_pass(data, perm, True, 0)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / steps)
    for name, (_, _, _, _, us) in runs.items():
        out[name] = {"us_per_batch_median": statistics.median(us), "us_per_batch": us}
        print(name, "%.2f us / batch (median of %d epochs)" % (statistics.median(us), a.reps), flush=True)

    # the general path at k = 5: a trainer whose compute_batch is overridden
    class General(iwae.IWAETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    torch.manual_seed(1234)
    tr = General(iwae.IWAE(), *its(512), k=5, seed=0)
    assert not tr._stock()
    opt = trainers.FlatAdam(tr.model.parameters(), 1e-3, weight_decay=1e-5)
    tr.model.train()
    batches = [(x[i * 512:(i + 1) * 512], y[i * 512:(i + 1) * 512]) for i in range(a.general_batches)]

    def step(batch):
        opt.zero_grad()
        loss, _ = tr.compute_batch(batch)
        loss.backward()
        opt.step()
    for b in batches:
        step(b)                                          # warm-up
    us = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for b in batches:
            step(b)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / len(batches))
    out["iwae_k5_general"] = {"us_per_batch_median": statistics.median(us), "us_per_batch": us}
    print("iwae_k5_general %.2f us / batch (median of %d x %d batches)" % (statistics.median(us), a.reps, len(batches)))
    med = lambda n: out[n]["us_per_batch_median"]
    out["ratio_iwae_k1_over_vae_b512"] = med("iwae_k1") / med("vae_b512")
    out["ratio_iwae_k5_over_vae_b2560"] = med("iwae_k5") / med("vae_b2560")
    out["ratio_general_over_fused_k5"] = med("iwae_k5_general") / med("iwae_k5")
    for n in ("ratio_iwae_k1_over_vae_b512", "ratio_iwae_k5_over_vae_b2560", "ratio_general_over_fused_k5"):
        print("%s = %.3f" % (n, out[n]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0 if med("iwae_k5") < med("iwae_k5_general") else 1


if __name__ == "__main__":
    sys.exit(main())
