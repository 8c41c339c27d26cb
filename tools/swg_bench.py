#!/usr/bin/env python
"""The SWG in microseconds per training batch against the GMMN, an NSGAN iteration and the autoencoder's batch, its sort
launch against a torch composition of the same contract, and metrics.sliced_wasserstein at 10 000 x 10 000 x 784 against
torch.  784-400-20.

    python tools/swg_bench.py [--n-train 50176] [--reps 5] [--iters 50] [--out profiles/swg_bench.json]

train: the SWG at P = 256 and P = 1024 directions, the GMMN, NSGAN and the autoencoder, at bs 512 and bs 1000, timed the
way tools/gmmn_bench.py times them.  Each repetition times each model in turn (the models alternate, so drift hits all
alike), after one warm-up epoch per model that captures the graphs.  Two figures, never mixed in a ratio:
`us_per_batch_epoch`, every model's train(1) on the host clock around a device synchronise, over the training batches
(the one validation batch and the epoch's host work are in it for all alike) -- what the ratios are formed from; and
`us_per_batch`, the engine's training pass alone (run_pass between HIP events), what the shares of a batch refer to.

sort: at N = M = 512 and 1000 rows and P = 256 and 1024 projections (random normals): gm_sw_sort without Ct + finalize
(forward) and with Ct + finalize (the backward's coefficients come out of the same launch), against torch on the same
projections -- two `sort`s, `gather` of nothing (N = M: the ranks match one to one), the elementwise tail and the mean,
and autograd back to the projections.  The directions launch, the projection GEMM and the product Ct^T Theta are listed
one by one with their share of the training pass.

metric: metrics.sliced_wasserstein (1024 directions) on 10 000 x 10 000 rows against torch: `randn` directions
normalised, one matmul per block of 256 directions, two sorts, the mean.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swg_bench.json"))
    a = ap.parse_args()
    import torch
    import ae
    import gmmn
    import ns_gan
    import swg
    from generative_models_amd import metrics, ops, ops_fused, trainers
    from generative_models_amd import swg as gswg

    if not torch.cuda.is_available():
        raise SystemExit("swg_bench measures on the MI355X: no GPU is visible")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "n_train": a.n_train, "reps": a.reps,
                      "iters": a.iters}, "train": {}, "sort": {}, "metric": {}}

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
        models = {"swg_p256": lambda: swg.SWGTrainer(swg.SWG(), dl(), dl(B), dl(B), num_projections=256, seed=0),
                  "swg_p1024": lambda: swg.SWGTrainer(swg.SWG(), dl(), dl(B), dl(B), num_projections=1024, seed=0),
                  "gmmn": lambda: gmmn.GMMNTrainer(gmmn.GMMN(), dl(), dl(B), dl(B), seed=0),
                  "autoencoder": lambda: ae.AutoencoderTrainer(ae.Autoencoder(), dl(), dl(B), dl(B)),
                  "nsgan": lambda: ns_gan.NSGANTrainer(ns_gan.NSGAN(784, 400, 20), dl(), dl(B), dl(B))}
        runs = {}
        for name, mk in models.items():
            torch.manual_seed(1234)
            tr = mk()
            with contextlib.redirect_stdout(io.StringIO()):
                tr.train(1)                              # warm-up: graphs captured
            runs[name] = (tr, [])
        assert type(runs["swg_p256"][0]._engine).__name__ == "SWGEngine"
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
        for s in ("swg_p256", "swg_p1024"):
            for other in ("gmmn", "nsgan", "autoencoder"):
                T["ratio_%s_over_%s" % (s, other)] = ep(s) / ep(other)
        runs.clear()

        # the sort launch alone against torch on the same projections, and the launches around it
        for P in (256, 1024):
            gen = torch.Generator().manual_seed(B + P)
            Pr = torch.randn(P, 2 * B, generator=gen).to(dev)
            Pr2 = torch.empty_like(Pr)
            R = torch.rand(2 * B, 784, generator=gen).to(dev)
            th = torch.empty(P, 784, device=dev)
            noise = ops_fused.sw_noise(0, gswg.TAG_DT)
            ws = ops_fused.sw_workspace(P, dev)
            Ct = torch.zeros(P, B, device=dev)
            dX = torch.zeros(B, 784, device=dev)
            stats = torch.zeros(2, dtype=torch.float64, device=dev)

            def t_loss(pr):
                sa, sb = torch.sort(pr[:, :B], dim=1)[0], torch.sort(pr[:, B:], dim=1)[0]
                return ((sa - sb) ** 2).mean()

            def t_fwd():
                with torch.no_grad():
                    t_loss(Pr)
            Pg = Pr.clone().requires_grad_()
            t_both = lambda: torch.autograd.grad(t_loss(Pg), Pg)
            sort0 = lambda: ops_fused.sw_sort(Pr, B, B, ws)
            sortC = lambda: ops_fused.sw_sort(Pr, B, B, ws, Ct=Ct)
            fin = lambda: ops_fused.sw_finalize(P, B, B, ws, stats)
            S = out["sort"]["bs%d_p%d" % (B, P)] = {
                "sort_without_Ct": timed(sort0), "sort_with_Ct": timed(sortC), "finalize": timed(fin),
                "directions": timed(lambda: ops_fused.sw_directions(th, noise)),
                "projection_gemm": timed(lambda: ops.linear_fwd(th, R, None, Pr2, "id")),
                "Ct_T_Theta_gemm": timed(lambda: ops.linear_bwd_dw(Ct, th, dX, None)),
                "fused_forward": timed(lambda: (sort0(), fin())),
                "fused_forward_backward": timed(lambda: (sortC(), fin())),
                "torch_forward": timed(t_fwd), "torch_forward_backward": timed(t_both)}
            m = lambda k: S[k]["us_per_call_median"]
            S["ratio_torch_over_fused_forward"] = m("torch_forward") / m("fused_forward")
            S["ratio_torch_over_fused_forward_backward"] = m("torch_forward_backward") / m("fused_forward_backward")
            batch = T["swg_p%d" % P]["us_per_batch_median"]
            for k in ("sort_with_Ct", "directions", "projection_gemm", "Ct_T_Theta_gemm"):
                S[k + "_share_of_batch"] = m(k) / batch
            print("sort bs %d P %d: %.1f us without Ct, %.1f with; finalize %.1f, directions %.1f, projection GEMM %.1f, "
                  "Ct^T Theta %.1f; torch %.1f forward / %.1f forward + backward; sort share of the batch %.3f" % (
                      B, P, m("sort_without_Ct"), m("sort_with_Ct"), m("finalize"), m("directions"), m("projection_gemm"),
                      m("Ct_T_Theta_gemm"), m("torch_forward"), m("torch_forward_backward"),
                      S["sort_with_Ct_share_of_batch"]), flush=True)

    # the score at evaluation size
    n, P = a.metric_rows, 1024
    gen = torch.Generator().manual_seed(7)
    Sx, D = torch.rand(n, 784, generator=gen).to(dev), (0.9 * torch.rand(n, 784, generator=gen) + 0.05).to(dev)

    def t_metric():
        with torch.no_grad():
            tot = torch.zeros((), dtype=torch.float64, device=dev)
            tg = torch.Generator(device=dev).manual_seed(0)
            for p0 in range(0, P, 256):
                th = torch.randn(256, 784, generator=tg, device=dev)
                th = th / th.norm(dim=1, keepdim=True)
                sa, sb = torch.sort(th @ Sx.T, dim=1)[0], torch.sort(th @ D.T, dim=1)[0]
                tot += ((sa - sb) ** 2).sum(dtype=torch.float64)
            return float(tot / (float(P) * n))
    fused = metrics.sliced_wasserstein(Sx, D, P)
    ref = t_metric()
    Q = out["metric"] = {"rows": n, "n_projections": P, "swd2_fused": fused.swd2, "swd2_torch_other_directions": ref,
                         "metrics_sliced_wasserstein": timed(lambda: metrics.sliced_wasserstein(Sx, D, P), iters=3),
                         "torch_blocks": timed(t_metric, iters=3)}
    Q["ratio_torch_over_fused"] = Q["torch_blocks"]["us_per_call_median"] / \
        Q["metrics_sliced_wasserstein"]["us_per_call_median"]
    print("metric %d x %d, %d directions: metrics.sliced_wasserstein %.1f ms, torch %.1f ms (swd2 %.4e / %.4e on other "
          "directions)" % (n, n, P, Q["metrics_sliced_wasserstein"]["us_per_call_median"] / 1e3,
                           Q["torch_blocks"]["us_per_call_median"] / 1e3, fused.swd2, ref), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
