#!/usr/bin/env python
"""The GMMN in microseconds per training batch against an NSGAN iteration and the autoencoder's batch, its MMD launches
against a torch composition of the same contract, metrics.mmd at 10 000 x 10 000 x 784 against torch, and the share of a
batch spent writing and re-reading the coefficient array C.  784-400-20.

    python tools/gmmn_bench.py [--n-train 50176] [--reps 5] [--iters 50] [--out profiles/gmmn_bench.json]

train: GMMN at bs 512 and bs 1000 (the paper's), NSGAN and the autoencoder at the same batch sizes.  Each repetition
times each model in turn (the models alternate, so drift hits all alike), after one warm-up epoch per model that captures
the graphs.  Two figures, never mixed in a ratio: `us_per_batch_epoch`, every model's train(1) on the host clock around
a device synchronise, over the training batches (the one validation batch and the epoch's host work are in it for all
three alike) -- what the ratios against the NSGAN and the autoencoder are formed from; and `us_per_batch`, the GMMN's and
the autoencoder's training pass alone (the engine's run_pass between HIP events), what the shares of a batch refer to.

mmd: at N = M = 512 and 1000 rows of 784 in [0, 1], the paper's six bandwidths: gm_mmd_pairs + gm_mmd_finalize without C
(forward) and pairs + finalize + C R + gm_mmd_grad (forward + backward), against torch on the same rows -- the Gram form
through torch.mm, exp per bandwidth, the loss, and autograd back to X.  pairs_with_C - pairs_without_C, C R and the grad
launch are listed one by one: c_share_of_batch = ((pairs with C - pairs without C) + C R) / the training batch's time is
the upper bound of what a kernel that never writes C could save.

metric: metrics.mmd (unbiased) on 10 000 x 10 000 rows against the same torch composition in blocks of 2 000 rows.

Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic binary images (the bit-packed dataset, as get_data() gives)."""
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


def record(us, key):
    med = statistics.median(us)
    return {key + "_median": med, key: us, key + "_spread": (max(us) - min(us)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--metric-rows", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmmn_bench.json"))
    a = ap.parse_args()
    import torch
    import ae
    import gmmn
    import ns_gan
    from generative_models_amd import metrics, ops, ops_fused, trainers

    if not torch.cuda.is_available():
        raise SystemExit("gmmn_bench measures on the MI355X: no GPU is visible")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "n_train": a.n_train, "reps": a.reps,
                      "iters": a.iters, "sigmas": list(metrics.MMD_SIGMAS)}, "train": {}, "mmd": {}, "metric": {}}

    def timed(fn, iters=a.iters):
        fn()                                             # warm-up
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / iters)
        return record(us, "us_per_call")

    for B in (512, 1000):
        dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=B,
                                                        shuffle=True)
        steps = (a.n_train + B - 1) // B
        models = {"gmmn": lambda: gmmn.GMMNTrainer(gmmn.GMMN(), dl(), dl(B), dl(B), seed=0),
                  "autoencoder": lambda: ae.AutoencoderTrainer(ae.Autoencoder(), dl(), dl(B), dl(B)),
                  "nsgan": lambda: ns_gan.NSGANTrainer(ns_gan.NSGAN(784, 400, 20), dl(), dl(B), dl(B))}
        runs = {}
        for name, mk in models.items():
            torch.manual_seed(1234)
            tr = mk()
            with contextlib.redirect_stdout(io.StringIO()):
                tr.train(1)                              # warm-up: graphs captured
            runs[name] = (tr, [])
        assert type(runs["gmmn"][0]._engine).__name__ == "GMMNEngine"
        epoch_us = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, (tr, us) in runs.items():
                torch.cuda.synchronize()
                with contextlib.redirect_stdout(io.StringIO()):
                    t0 = time.perf_counter()
                    tr.train(1)
                    torch.cuda.synchronize()
                    epoch_us[name].append((time.perf_counter() - t0) * 1e6 / steps)
                if name == "nsgan":
                    continue
                eng, data = tr._engine, tr._device_data(tr.train_iter)
                perm = trainers._epoch_order(tr.train_iter)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.run_pass(data, perm, True, 0)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1000.0 / steps)
        T = out["train"]["bs%d" % B] = {"batches_per_epoch": steps}
        for name, (_, us) in runs.items():
            T[name] = record(epoch_us[name], "us_per_batch_epoch")
            if us:
                T[name].update(record(us, "us_per_batch"))
            print("bs %d %s %.2f us / batch over train(1)%s (median of %d epochs)" % (
                B, name, T[name]["us_per_batch_epoch_median"],
                ", %.2f for the training pass alone" % T[name]["us_per_batch_median"] if us else "", a.reps), flush=True)
        ep = lambda n: T[n]["us_per_batch_epoch_median"]
        T["ratio_gmmn_over_nsgan"] = ep("gmmn") / ep("nsgan")
        T["ratio_gmmn_over_autoencoder"] = ep("gmmn") / ep("autoencoder")
        runs.clear()

        # the MMD launches alone against torch on the same rows
        gen = torch.Generator().manual_seed(B)
        X, Y = torch.rand(B, 784, generator=gen).to(dev), torch.rand(B, 784, generator=gen).to(dev)
        R = torch.cat([X, Y], 0).contiguous()
        Xr, Yr = R[:B], R[B:]
        sig = ops_fused.mmd_sigmas(metrics.MMD_SIGMAS, dev)
        ws = ops_fused.mmd_workspace(B, B, True, dev)
        C = torch.zeros(B, 2 * B, device=dev)
        stats = torch.zeros(10, dtype=torch.float64, device=dev)
        r, P, dA = torch.zeros(B, device=dev), torch.zeros(B, 784, device=dev), torch.zeros(B, 784, device=dev)
        s2 = torch.tensor(metrics.MMD_SIGMAS, device=dev) ** 2

        def kern(a_, b_):
            d2 = ((a_ * a_).sum(1)[:, None] + (b_ * b_).sum(1)[None, :] - 2.0 * (a_ @ b_.T)).clamp_min(0.0)
            return torch.exp(-d2[..., None] / (2.0 * s2)).sum()

        def t_loss(xx):
            n, m = xx.shape[0], Y.shape[0]
            return torch.sqrt(kern(xx, xx) / (n * n) - 2.0 * kern(xx, Y) / (n * m) + kern(Y, Y) / (m * m) + 1e-8)

        def t_fwd():
            with torch.no_grad():
                t_loss(X)
        Xg = X.clone().requires_grad_()
        t_both = lambda: torch.autograd.grad(t_loss(Xg), Xg)
        Rc = torch.zeros_like(R)
        pairs0 = lambda: ops_fused.mmd_pairs(Xr, Yr, sig, ws, Rc=Rc)
        pairsC = lambda: ops_fused.mmd_pairs(Xr, Yr, sig, ws, C=C, Rc=Rc)
        fin0 = lambda: ops_fused.mmd_finalize(B, B, sig.numel(), True, ws, stats)
        finC = lambda: ops_fused.mmd_finalize(B, B, sig.numel(), True, ws, stats, r=r)
        gemm = lambda: ops.linear_bwd_dx(C, Rc, P, M=B)
        grad = lambda: ops_fused.mmd_grad(Xr, P, r, stats, dA, mu=Xr[:1])
        M = out["mmd"]["bs%d" % B] = {
            "pairs_without_C": timed(pairs0), "pairs_with_C": timed(pairsC), "finalize_without_r": timed(fin0),
            "finalize_with_r": timed(finC), "C_R_gemm": timed(gemm), "grad": timed(grad),
            "fused_forward": timed(lambda: (pairs0(), fin0())),
            "fused_forward_backward": timed(lambda: (pairsC(), finC(), gemm(), grad())),
            "torch_forward": timed(t_fwd), "torch_forward_backward": timed(t_both)}
        m = lambda k: M[k]["us_per_call_median"]
        M["ratio_torch_over_fused_forward"] = m("torch_forward") / m("fused_forward")
        M["ratio_torch_over_fused_forward_backward"] = m("torch_forward_backward") / m("fused_forward_backward")
        M["c_write_and_reread_us"] = (m("pairs_with_C") - m("pairs_without_C")) + m("C_R_gemm")
        M["c_share_of_batch"] = M["c_write_and_reread_us"] / T["gmmn"]["us_per_batch_median"]
        M["mmd_share_of_batch"] = m("fused_forward_backward") / T["gmmn"]["us_per_batch_median"]
        M["pairs_share_of_batch"] = m("pairs_with_C") / T["gmmn"]["us_per_batch_median"]
        M["planner_C_R"] = {k: v for k, v in ops.linear_plan("dx", ops._dx_args(C, Rc, P, M=B)).items()}
        print("mmd bs %d: fused forward %.1f, forward + backward %.1f (pairs %.1f -> %.1f with C, C R %.1f, grad %.1f); "
              "torch %.1f / %.1f us; C share of the batch %.3f" % (
                  B, m("fused_forward"), m("fused_forward_backward"), m("pairs_without_C"), m("pairs_with_C"),
                  m("C_R_gemm"), m("grad"), m("torch_forward"), m("torch_forward_backward"), M["c_share_of_batch"]),
              flush=True)

    # the score at evaluation size
    n = a.metric_rows
    gen = torch.Generator().manual_seed(7)
    S, D = torch.rand(n, 784, generator=gen).to(dev), torch.rand(n, 784, generator=gen).to(dev)
    s2 = torch.tensor(metrics.MMD_SIGMAS, device=dev) ** 2

    def t_metric():
        with torch.no_grad():
            def ksum(a_, b_, off):
                tot = torch.zeros((), dtype=torch.float64, device=dev)
                nb = (b_ * b_).sum(1)
                for lo in range(0, a_.shape[0], 2000):
                    blk = a_[lo:lo + 2000]
                    d2 = ((blk * blk).sum(1)[:, None] + nb[None, :] - 2.0 * (blk @ b_.T)).clamp_min(0.0)
                    if off:
                        d2[torch.arange(blk.shape[0]), torch.arange(lo, lo + blk.shape[0])] = 0.0
                    for s in s2:
                        tot += torch.exp(-d2 / (2.0 * s)).sum(dtype=torch.float64)
                return tot - (a_.shape[0] * len(s2) if off else 0)
            v = ksum(S, S, True) / (n * (n - 1.0)) - 2.0 * ksum(S, D, False) / (float(n) * n) + \
                ksum(D, D, True) / (n * (n - 1.0))
            return float(v)
    fused = metrics.mmd(S, D)
    ref = t_metric()
    Q = out["metric"] = {"rows": n, "mmd2_fused": fused.mmd2, "mmd2_torch": ref,
                         "metrics_mmd": timed(lambda: metrics.mmd(S, D), iters=3),
                         "torch_blocks": timed(t_metric, iters=3)}
    Q["ratio_torch_over_fused"] = Q["torch_blocks"]["us_per_call_median"] / Q["metrics_mmd"]["us_per_call_median"]
    Q["pair_kernel_evaluations"] = 3 * n * n * len(metrics.MMD_SIGMAS)
    Q["gram_flops"] = 2.0 * 784 * 3 * n * n                     # the three blocks the kernel forms (xy once)
    Q["gram_tflops_achieved"] = Q["gram_flops"] / (Q["metrics_mmd"]["us_per_call_median"] * 1e-6) / 1e12
    print("metric %d x %d: metrics.mmd %.1f ms, torch %.1f ms (mmd2 %.3e / %.3e)" % (
        n, n, Q["metrics_mmd"]["us_per_call_median"] / 1e3, Q["torch_blocks"]["us_per_call_median"] / 1e3, fused.mmd2,
        ref), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
