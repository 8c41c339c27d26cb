#!/usr/bin/env python
"""NSGAN against the AC-GAN in microseconds per iteration: 784-400-20, C = 10, bs = 256, whole epochs on the graph
path, plus the two head kernels alone.

    python tools/acgan_bench.py [--n-train 50000] [--reps 5] [--out profiles/acgan_bench.json]

tools/bgan_bench.py's protocol: each repetition times one train(1) call of each trainer (host sampler replay, graph
launches and the epoch's loss read-back included, the same for both) with a synchronize on each side, the trainers
alternating; the median over repetitions is reported, after one warm-up epoch that captures the graphs.  The head
kernels are timed with HIP events over 200 back-to-back launches on the engine's own buffers (critic mode on 2B rows
without the Adam step's schedule, generator mode on B rows); their floor is one read of H (forward) or one read of H
and one write of dPre (backward) at 6.3 TB/s.  Synthetic binary images, classes arange(n) % 10."""
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

B, C, H = 256, 10, 400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acgan_bench.json"))
    a = ap.parse_args()
    import torch
    import ac_gan
    import ns_gan
    from generative_models_amd import ops, ops_fused

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.arange(a.n_train) % C
    dl = lambda n: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=B,
                                               shuffle=True)
    steps = (a.n_train + B - 1) // B
    out = {"config": {"image_size": 784, "hidden_dim": H, "z_dim": 20, "num_classes": C, "batch": B,
                      "n_train": a.n_train, "iterations_per_epoch": steps, "reps": a.reps, "D_steps": 1}}
    trainers = {}
    for name, mk in (("nsgan", lambda: ns_gan.NSGANTrainer(ns_gan.NSGAN(784, H, 20), dl(a.n_train), dl(B), dl(B))),
                     ("acgan", lambda: ac_gan.ACGANTrainer(ac_gan.ACGAN(784, H, 20, C), dl(a.n_train), dl(B), dl(B)))):
        torch.manual_seed(1234)
        trainers[name] = mk()
        with contextlib.redirect_stdout(io.StringIO()):
            trainers[name].train(1)                      # warm-up: graphs captured
    assert type(trainers["acgan"]._engine).__name__ == "ACGANEngine"
    us = {n: [] for n in trainers}
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(a.reps):
            for name, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train(1)
                torch.cuda.synchronize()
                us[name].append((time.perf_counter() - t0) * 1e6 / steps)
    for name in trainers:
        out[name] = {"us_per_iteration_median": statistics.median(us[name]), "us_per_iteration": us[name]}
        print(name, "%.2f us / iteration (median of %d epochs)" % (statistics.median(us[name]), a.reps), flush=True)
    out["ratio_acgan_over_nsgan"] = out["acgan"]["us_per_iteration_median"] / out["nsgan"]["us_per_iteration_median"]
    eng = trainers["acgan"]._engine
    out["launches_per_iteration"] = eng.launches_per_iteration(1)
    print("AC-GAN / NSGAN = %.3f, %d launches per iteration" % (out["ratio_acgan_over_nsgan"],
                                                                out["launches_per_iteration"]))
    lab = ops.label_src(eng.labels, eng.idx[0])
    heads = eng._heads()
    D2, Dc = eng.D2, eng.Dc
    loss = torch.zeros(3, device=eng.dev)

    def fwd(gen):
        rows = eng.Hd[:B] if gen else eng.Hd
        ops_fused.acgan_heads_fwd(rows, *heads, lab, B, gen, 1.0, eng.da2, eng.dq, eng.ws, loss_out=loss)

    def bwd(gen):
        rows, dPre = (eng.Hd[:B], eng.dPre[:B]) if gen else (eng.Hd, eng.dPre)
        ops_fused.acgan_heads_bwd(rows, *heads, B, gen, eng.da2, eng.dq, dPre, eng.ws,
                                  grads=None if gen else (D2.gW, D2.gb, Dc.gW, Dc.gb))
    kern = {}
    for name, fn, gen, traffic in (("heads_fwd_D", fwd, False, 2 * B * H * 4), ("heads_fwd_G", fwd, True, B * H * 4),
                                   ("heads_bwd_D", bwd, False, 2 * 2 * B * H * 4), ("heads_bwd_G", bwd, True, 2 * B * H * 4)):
        for _ in range(10):
            fn(gen)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn(gen)
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1000.0 / 200
        kern[name] = {"us_per_call": t, "bandwidth_floor_us": traffic / 6.3e12 * 1e6}
        print("%s: %.2f us / call (floor %.3f us)" % (name, t, kern[name]["bandwidth_floor_us"]))
    out["kernels"] = kern
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
