#!/usr/bin/env python
"""The DDPM against the plain autoencoder in microseconds per training batch, and its sampler in microseconds per step:
784-400-32, bs = 512, T = 1000, whole epochs on the graph path.

    python tools/ddpm_bench.py [--n-train 50176] [--reps 5] [--general-batches 20] [--sampler-steps 200]
                               [--out profiles/ddpm_bench.json]

Rows: the autoencoder (784-32, the engine's closest relative: 5 launches per batch) and the fused DDPM (10 launches),
alternating in one process, tools/dvae_bench.py's protocol -- each repetition times one training pass of each model in
turn with HIP events (validation excluded), the median over repetitions is reported, after one warm-up epoch per model
that captures the graphs; the DDPM's general path (autograd over the fused linear kernels) as the median over repetitions
of --general-batches training batches, after as many warm-up batches; the sampler at n = 10 000 and n = 64 rows as the
median over repetitions of one sample(n, steps=--sampler-steps) call divided by its steps, after one warm-up call that
captures the graph (the call's synchronises, table upload and final clamp are inside the figure).  Synthetic binary
images (the bit-packed dataset, as get_data() gives); 50176 = 98 batches of 512."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--general-batches", type=int, default=20)
    ap.add_argument("--sampler-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpm_bench.json"))
    a = ap.parse_args()
    import torch
    import ae
    import ddpm
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    out = {"config": {"image_size": 784, "hidden_dim": 400, "time_dim": 32, "T": 1000, "batch": 512,
                      "n_train": a.n_train, "batches_per_epoch": steps, "reps": a.reps,
                      "general_batches": a.general_batches, "sampler_steps": a.sampler_steps}}
    models = {"ae": lambda: ae.AutoencoderTrainer(ae.Autoencoder(), *its()),
              "ddpm": lambda: ddpm.DDPMTrainer(ddpm.DDPM(), *its(), seed=0)}
    runs = {}
    for name, mk in models.items():
        torch.manual_seed(1234)
        tr = mk()
        with open(os.devnull, "w") as null:
            stdout, sys.stdout = sys.stdout, null
            try:
                tr.train(1)                                  # warm-up: graphs captured
            finally:
                sys.stdout = stdout
        assert type(tr._engine).__name__ == ("AEEngine" if name == "ae" else "DDPMEngine")
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
    for name, (_, _, _, us) in runs.items():
        out[name] = {"us_per_batch_median": statistics.median(us), "us_per_batch": us}
        print(name, "%.2f us / batch (median of %d epochs)" % (statistics.median(us), a.reps), flush=True)

    # the sampler: one hipGraph of G steps replayed steps / G times
    tr = runs["ddpm"][0]
    for n in (10000, 64):
        tr.sample(n, seed=0, steps=a.sampler_steps)          # warm-up: graph captured
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.sample(n, seed=0, steps=a.sampler_steps)      # ends with a synchronise
            us.append((time.perf_counter() - t0) * 1e6 / a.sampler_steps)
        out["sampler_n%d" % n] = {"us_per_step_median": statistics.median(us), "us_per_step": us}
        print("sampler n=%d %.2f us / step (median of %d calls of %d steps)" % (n, statistics.median(us), a.reps,
                                                                                a.sampler_steps), flush=True)

    # the general path: a trainer whose compute_batch is overridden
    class General(ddpm.DDPMTrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    torch.manual_seed(1234)
    tr = General(ddpm.DDPM(), *its(), seed=0)
    assert not tr._stock()
    opt = trainers.FlatAdam(tr.model.parameters(), 2e-4)
    tr.model.train()
    batches = [(x[i * 512:(i + 1) * 512], y[i * 512:(i + 1) * 512]) for i in range(a.general_batches)]

    def step(batch):
        opt.zero_grad()
        loss = tr.compute_batch(batch)
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
    out["ddpm_general"] = {"us_per_batch_median": statistics.median(us), "us_per_batch": us}
    print("ddpm_general %.2f us / batch (median of %d x %d batches)" % (statistics.median(us), a.reps, len(batches)))
    med = lambda n: out[n]["us_per_batch_median"]
    out["ratio_ddpm_over_ae"] = med("ddpm") / med("ae")
    out["ratio_general_over_fused"] = med("ddpm_general") / med("ddpm")
    for n in ("ratio_ddpm_over_ae", "ratio_general_over_fused"):
        print("%s = %.3f" % (n, out[n]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
