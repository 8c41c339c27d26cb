#!/usr/bin/env python
"""The VQ-VAE against the VAE, the IWAE (k = 1) and the categorical VAE in microseconds per training batch, its three
quantisation launches against the torch composition of the same maths, and sample(10 000) with the MADE prior: 784-400,
N = 16 variables of D = 16 floats, K = 128 codes, bs = 512, whole epochs on the graph path.

    python tools/vqvae_bench.py [--n-train 50176] [--reps 5] [--out profiles/vqvae_bench.json]

train: the VAE, the IWAE at k = 1, the categorical VAE (relaxed) and the VQ-VAE.  Each repetition times one training pass
of each model in turn (the models alternate, so drift hits all alike) with HIP events (validation excluded: the engine's
run_pass for the training set), after one warm-up epoch per model that captures the graphs.

quantise: on 512 rows, gm_vq_quantise, gm_vq_reduce and gm_vq_step alone and together, against torch's cdist + argmin +
embedding forward and the same plus the commitment gradient and index_add_ for (n_k, s_k) and the codebook gradient (no
Adam step on the torch side, one on the fused side): --iters launches between HIP events.

sample: VQVAETrainer.sample(10 000) with a MADE prior fitted for one epoch (prior.sample -> bits_code -> decode), wall
clock around the call with a device synchronise.

Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic binary images (the bit-packed dataset, as get_data() gives); 50176 = 98 batches of 512."""
import argparse
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
    return {key + "_median": med, key: us, "spread": (max(us) - min(us)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vqvae_bench.json"))
    a = ap.parse_args()
    import torch
    import cat_vae
    import iwae
    import vae
    import vq_vae
    from generative_models_amd import ops, ops_fused, trainers

    N, D, K = 16, 16, 128
    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    out = {"config": {"image_size": 784, "hidden_dim": 400, "num_vars": N, "code_dim": D, "num_codes": K, "batch": 512,
                      "n_train": a.n_train, "batches_per_epoch": steps, "reps": a.reps, "iters": a.iters},
           "train": {}, "quantise": {}, "sample": {}}
    models = {"vae": ("VAEEngine", lambda: vae.VAETrainer(vae.VAE(), *its())),
              "iwae_k1": ("IWAEEngine", lambda: iwae.IWAETrainer(iwae.IWAE(), *its(), k=1, seed=0)),
              "catvae": ("CatVAEEngine", lambda: cat_vae.CatVAETrainer(cat_vae.CatVAE(784, 400, 20, 10), *its(), seed=0)),
              "vqvae": ("VQVAEEngine", lambda: vq_vae.VQVAETrainer(vq_vae.VQVAE(784, 400, N, D, K), *its()))}
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
    for base in ("vae", "iwae_k1", "catvae"):
        n = "ratio_vqvae_over_%s" % base
        T[n] = med("vqvae") / med(base)
        print("%s = %.3f" % (n, T[n]), flush=True)
    vq = runs["vqvae"][0]
    runs.clear()

    # the three launches alone against the torch composition
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
    B, W, dev, beta = 512, N * D, "cuda", 0.25
    gen = torch.Generator().manual_seed(3)
    ze = torch.randn(B, W, generator=gen).to(dev)
    E = torch.randn(K, D, generator=gen).to(dev)
    dz = torch.randn(B, W, generator=gen).to(dev)
    wn = torch.ones(B, device=dev)
    zq, qerr, lp, dml = torch.empty(B, W, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), \
        torch.empty(B, W, device=dev)
    codes = torch.empty(B, N, dtype=torch.int32, device=dev)
    Es, m, v, gE = E.clone(), torch.zeros(K, D, device=dev), torch.zeros(K, D, device=dev), torch.empty(K, D, device=dev)
    nk = torch.empty(K, dtype=torch.int32, device=dev)
    sched = torch.from_numpy(ops.adam_schedule(0.0, 1)).to(dev)      # lr = 0: the timed step leaves the codebook in place

    def f_quantise():
        ops_fused.vq_quantise(ze, E, zq, codes, qerr, lp, beta, B, N, D)

    def f_reduce():
        ops_fused.vq_reduce(ze, E, codes, dz, wn, dml, beta, B, N, D)

    def f_step():
        ops_fused.vq_step(ze, codes, Es, B, N, D, moments=(m, v), sched=sched, grad=gE, nk=nk)

    def f_all():
        f_quantise(), f_reduce(), f_step()

    def t_fwd():
        z = ze.view(B * N, D)
        c = torch.cdist(z, E).argmin(1)
        q = torch.nn.functional.embedding(c, E)
        e = ((z - q) ** 2).view(B, N * D).sum(1)
        return z, c, q, e, -(1.0 + beta) * e

    def t_both():
        z, c, q, _, _ = t_fwd()
        d = dz + 2.0 * beta * (z - q).view(B, W)
        n = torch.bincount(c, minlength=K)
        s = torch.zeros(K, D, device=dev).index_add_(0, c, z)
        return d, 2.0 * (n[:, None] * E - s)
    Q = out["quantise"]
    f_quantise()
    for name, fn in (("vq_quantise", f_quantise), ("vq_reduce", f_reduce), ("vq_step", f_step), ("fused_all", f_all),
                     ("torch_forward", t_fwd), ("torch_forward_backward", t_both)):
        Q[name] = timed(fn)
    mq = lambda n: Q[n]["us_per_call_median"]
    Q["ratio_torch_forward_over_vq_quantise"] = mq("torch_forward") / mq("vq_quantise")
    Q["ratio_torch_over_fused_all"] = mq("torch_forward_backward") / mq("fused_all")
    print("quantise: quantise %.2f, reduce %.2f, step %.2f, the three %.2f, torch forward %.2f, torch both ways %.2f us"
          % tuple(mq(n) for n in ("vq_quantise", "vq_reduce", "vq_step", "fused_all", "torch_forward",
                                  "torch_forward_backward")), flush=True)

    # sample(10 000) through the MADE prior
    vq.fit_prior(1)
    vq.sample(10000, seed=0)                             # warm-up
    ms = []
    for r in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = vq.sample(10000, seed=r)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert tuple(s.shape) == (10000, 784)
    out["sample"]["sample_10000_with_prior"] = record(ms, "ms_per_call")
    print("sample(10000) with the MADE prior: %.2f ms" % out["sample"]["sample_10000_with_prior"]["ms_per_call_median"],
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
