#!/usr/bin/env python
"""The beta-TCVAE against the VAE and the IWAE at k = 1 in microseconds per training batch, and its two pair kernels
against the torch composition of the general path: 784-400-20, bs = 512, whole epochs on the graph path.

    python tools/tcvae_bench.py [--n-train 50176] [--reps 5] [--out profiles/tcvae_bench.json]

train: the VAE, the IWAE at k = 1 and the TCVAE (alpha, beta, gamma = 1, 6, 1).  Each repetition times one training pass
of each model in turn (the models alternate, so drift hits all alike) with HIP events (validation excluded: the engine's
run_pass for the training set), after one warm-up epoch per model that captures the graphs.  The yardstick of "the
decomposition is cheap" is the IWAE at k = 1 taken in the same run: ratio_tcvae_over_iwae_k1.

pairs: 512 rows, Z = 20, in the two input regimes of tests/test_gpu_tcvae.py: gm_tc_sample alone and gm_tc_reduce alone,
against the forward (tcvae.decomposition_terms: the [B, B, Z] tensor, its two logsumexps) and the forward + backward
(autograd of sum(dzdec . z - lp) back to [mu | lv]) in torch on the same rows: --iters launches between HIP events.

Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic binary images (the bit-packed dataset, as get_data() gives); 50176 = 98 batches of 512."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))


def record(us, key):
    med = statistics.median(us)
    return {key + "_median": med, key: us, "spread": (max(us) - min(us)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tcvae_bench.json"))
    a = ap.parse_args()
    import torch
    import iwae
    import tc_vae
    import vae
    from generative_models_amd import ops_fused, trainers
    from generative_models_amd import tcvae as gtc

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    coef = (1.0, 6.0, 1.0)
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": steps, "reps": a.reps, "iters": a.iters, "alpha_beta_gamma": coef},
           "train": {}, "pairs": {}}
    models = {"vae": ("VAEEngine", lambda: vae.VAETrainer(vae.VAE(), *its())),
              "iwae_k1": ("IWAEEngine", lambda: iwae.IWAETrainer(iwae.IWAE(), *its(), k=1, seed=0)),
              "tcvae": ("TCVAEEngine", lambda: tc_vae.TCVAETrainer(tc_vae.TCVAE(), *its(), seed=0))}
    runs = {}
    for name, (engine, mk) in models.items():
        torch.manual_seed(1234)
        tr = mk()
        tr.train(1, quiet=True)                          # warm-up: graphs captured
        assert type(tr._engine).__name__ == engine
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
    T = out["train"]
    for name, (_, _, _, us) in runs.items():
        T[name] = record(us, "us_per_batch")
        print(name, "%.2f us / batch (median of %d epochs)" % (T[name]["us_per_batch_median"], a.reps), flush=True)
    med = lambda n: T[n]["us_per_batch_median"]
    T["ratio_iwae_k1_over_vae"] = med("iwae_k1") / med("vae")
    T["ratio_tcvae_over_iwae_k1"] = med("tcvae") / med("iwae_k1")
    T["ratio_tcvae_over_vae"] = med("tcvae") / med("vae")
    print("tcvae / iwae k=1 = %.3f, tcvae / vae = %.3f" % (T["ratio_tcvae_over_iwae_k1"], T["ratio_tcvae_over_vae"]),
          flush=True)
    runs.clear()

    # the two pair kernels alone against the torch composition
    def timed(fn):
        fn()                                             # warm-up
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / a.iters)
        return record(us, "us_per_call")
    B, Z, dev = 512, 20, "cuda"
    L = math.log(a.n_train * B)
    C = out["pairs"]
    for regime in ("isolated", "overlapping"):
        gen = torch.Generator().manual_seed(1000 * Z + B)
        n = torch.randn(B, 2 * Z, generator=gen)
        ml = (0.3 * n if regime == "overlapping" else torch.cat([n[:, :Z], 0.5 * n[:, Z:] - 1.0], 1)).to(dev).contiguous()
        dzdec = torch.randn(B, Z, generator=gen).to(dev)
        wn = torch.ones(B, device=dev)
        z, lp, dml = torch.empty(B, Z, device=dev), torch.empty(B, device=dev), torch.empty(B, 2 * Z, device=dev)
        lsej, lsed, tcr = ops_fused.tc_records(B, Z, device=dev)
        noise = ops_fused.iwae_noise(0, 1, 1)
        sample = lambda: ops_fused.tc_sample(ml, z, lp, lsej, lsed, tcr, noise, *coef, L, B, Z)
        reduce = lambda: ops_fused.tc_reduce(ml, z, lsej, lsed, wn, dzdec, dml, noise, *coef, B, Z)
        eps = ops_fused.iwae_normals(B, 1, Z, 0, 0, 1, device=dev)
        pml = ml.clone().requires_grad_()

        def torch_lp(m):
            mu, lv = m[:, :Z], m[:, Z:]
            zz = mu + eps * torch.exp(lv / 2)
            mi, tc, dw = gtc.decomposition_terms(zz, mu, lv, L)
            return zz, -(coef[0] * mi + coef[1] * tc + coef[2] * dw)

        def t_fwd():
            with torch.no_grad():
                torch_lp(ml)

        def t_both():
            zz, lpt = torch_lp(pml)
            torch.autograd.grad((dzdec * zz).sum() - lpt.sum(), pml)
        C[regime] = {"tc_sample": timed(sample), "tc_reduce": timed(reduce), "torch_forward": timed(t_fwd),
                     "torch_forward_backward": timed(t_both)}
        m = lambda k: C[regime][k]["us_per_call_median"]
        C[regime]["ratio_torch_forward_over_tc_sample"] = m("torch_forward") / m("tc_sample")
        C[regime]["ratio_torch_over_fused_both_ways"] = m("torch_forward_backward") / (m("tc_sample") + m("tc_reduce"))
        print("pairs %s: sample %.2f, reduce %.2f, torch forward %.2f, torch forward + backward %.2f us"
              % (regime, m("tc_sample"), m("tc_reduce"), m("torch_forward"), m("torch_forward_backward")), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
