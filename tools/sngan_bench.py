#!/usr/bin/env python
"""NSGAN against the SN-GAN in microseconds per iteration: 784-400-20, bs = 256, whole epochs on the graph path, plus
the new kernels alone.

    python tools/sngan_bench.py [--n-train 50000] [--reps 5] [--out profiles/sngan_bench.json]

tools/acgan_bench.py's protocol: each repetition times one train(1) call of each trainer (host sampler replay, graph
launches and the epoch's loss read-back included, the same for both) with a synchronize on each side, the trainers
alternating; the median over repetitions is reported, after one warm-up epoch that captures the graphs.  The kernels
are timed with HIP events over 200 back-to-back calls on the engine's own buffers.  Each floor is the bytes the call's
shapes require over 6.3 TB/s (the achievable HBM rate): the power stage reads W three times and writes Wbar once,
gm_sn_grad reads G twice, Wbar once and writes gW, the head reads H (and writes dPre in the backward).  W's 1.25 MB is
L2-resident between the launches, so the real floor is lower.  Synthetic binary images."""
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

B, H, I = 256, 400, 784
HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sngan_bench.json"))
    a = ap.parse_args()
    import torch
    import ns_gan
    import sn_gan
    from generative_models_amd import ops_fused

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=B,
                                               shuffle=True)
    steps = (a.n_train + B - 1) // B
    out = {"config": {"image_size": I, "hidden_dim": H, "z_dim": 20, "batch": B, "n_train": a.n_train,
                      "iterations_per_epoch": steps, "reps": a.reps, "D_steps": 1}}
    trainers = {}
    for name, mk in (("nsgan", lambda: ns_gan.NSGANTrainer(ns_gan.NSGAN(I, H, 20), dl(a.n_train), dl(B), dl(B))),
                     ("sngan", lambda: sn_gan.SNGANTrainer(sn_gan.SNGAN(I, H, 20), dl(a.n_train), dl(B), dl(B)))):
        torch.manual_seed(1234)
        trainers[name] = mk()
        with contextlib.redirect_stdout(io.StringIO()):
            trainers[name].train(1)                      # warm-up: graphs captured
    assert type(trainers["sngan"]._engine).__name__ == "SNGANEngine"
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
    out["ratio_sngan_over_nsgan"] = out["sngan"]["us_per_iteration_median"] / out["nsgan"]["us_per_iteration_median"]
    eng = trainers["sngan"]._engine
    out["launches_per_iteration"] = eng.launches_per_iteration(1)
    print("SN-GAN / NSGAN = %.3f, %d launches per iteration" % (out["ratio_sngan_over_nsgan"],
                                                                out["launches_per_iteration"]))
    D1, D2 = eng.D1, eng.D2
    loss = torch.zeros(1, device=eng.dev)
    u = eng.u.clone()                                    # (the timed power iterations run on a copy of u)

    def power():
        ops_fused.sn_power_iter(D1.W, u, eng.v, eng.Wbar, D2.W, eng.w2bar, eng.stats, eng.ws_p)

    def grad():
        ops_fused.sn_grad(eng.Gw, eng.Wbar, u, eng.v, eng.stats, D1.gW, eng.ws_g)

    def fwd(gen):
        rows = eng.Hd[:B] if gen else eng.Hd
        ops_fused.sn_head_fwd(rows, eng.w2bar, D2.b, B, gen, eng.s, eng.ds, eng.ws_h, loss_out=loss)

    def bwd(gen):
        rows, dPre = (eng.Hd[:B], eng.dPre[:B]) if gen else (eng.Hd, eng.dPre)
        ops_fused.sn_head_bwd(rows, eng.w2bar, B, gen, eng.ds, dPre, eng.ws_h, stats=eng.stats,
                              grads=None if gen else (D2.gW, D2.gb))
    W4 = H * I * 4
    kern = {}
    for name, fn, traffic in (("power_iter_3_launches", power, 4 * W4), ("sn_grad_2_launches", grad, 4 * W4),
                              ("head_fwd_D", lambda: fwd(False), 2 * B * H * 4), ("head_fwd_G", lambda: fwd(True), B * H * 4),
                              ("head_bwd_D", lambda: bwd(False), 2 * 2 * B * H * 4),
                              ("head_bwd_G", lambda: bwd(True), 2 * B * H * 4)):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1000.0 / 200
        kern[name] = {"us_per_call": t, "bandwidth_floor_us": traffic / HBM * 1e6}
        print("%s: %.2f us / call (floor %.3f us)" % (name, t, kern[name]["bandwidth_floor_us"]))
    out["kernels"] = kern
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
