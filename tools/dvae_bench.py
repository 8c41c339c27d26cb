#!/usr/bin/env python
"""VAE against DVAE (salt-and-pepper and gaussian) in microseconds per training batch: 784-400-20, bs = 512, whole
epochs on the graph path.

    python tools/dvae_bench.py [--n-train 50000] [--reps 5] [--out profiles/dvae_bench.json]

Each repetition times one training pass of each model in turn (the models alternate, so drift hits all three alike)
with HIP events (validation excluded: the engine's run_pass for the training set); the median over repetitions is
reported, after one warm-up epoch per model that captures the graphs.  Synthetic binary images (the bit-packed
dataset, as get_data() gives)."""
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
    ap.add_argument("--n-train", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvae_bench.json"))
    a = ap.parse_args()
    import torch
    import dvae
    import vae
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    xv, yv = x[:512], y[:512]
    dl = lambda *t: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(*t), batch_size=512, shuffle=True)
    steps = (a.n_train + 511) // 512
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": steps, "reps": a.reps, "salt_pepper_level": 0.25, "gaussian_level": 0.3}}
    models = {
        "vae": lambda: vae.VAETrainer(vae.VAE(), dl(x, y), dl(xv, yv), dl(xv, yv)),
        "dvae_salt_pepper": lambda: dvae.DVAETrainer(dvae.DVAE(), dl(x, y), dl(xv, yv), dl(xv, yv),
                                                     noise="salt_pepper", level=0.25, seed=0),
        "dvae_gaussian": lambda: dvae.DVAETrainer(dvae.DVAE(), dl(x, y), dl(xv, yv), dl(xv, yv),
                                                  noise="gaussian", level=0.3, seed=0),
    }
    runs = {}
    for name, mk in models.items():
        torch.manual_seed(1234)
        tr = mk()
        tr.train(1, quiet=True)                          # warm-up: graphs captured
        runs[name] = (tr, tr._engine, tr._device_data(tr.train_iter), [])
    for _ in range(a.reps):
        for name, (tr, eng, data, us) in runs.items():
            perm = trainers._epoch_order(tr.train_iter)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.run_pass(data, perm, True, 0)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / steps)
    for name, (_, eng, _, us) in runs.items():
        assert type(eng).__name__ == ("VAEEngine" if name == "vae" else "DVAEEngine")
        out[name] = {"us_per_batch_median": statistics.median(us), "us_per_batch": us}
        print(name, "%.2f us / batch (median of %d epochs)" % (statistics.median(us), a.reps), flush=True)
    for name in ("dvae_salt_pepper", "dvae_gaussian"):
        out["ratio_%s_over_vae" % name] = out[name]["us_per_batch_median"] / out["vae"]["us_per_batch_median"]
        print("%s / VAE = %.3f" % (name, out["ratio_%s_over_vae" % name]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
