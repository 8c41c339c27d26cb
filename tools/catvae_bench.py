#!/usr/bin/env python
"""The categorical VAE against the VAE and the IWAE (k = 1) in microseconds per training batch, and its two Gumbel-Softmax
launches against the torch composition of the same math: 784-400, N = 20 variables of C = 10 classes, bs = 512, whole
epochs on the graph path.

    python tools/catvae_bench.py [--n-train 50176] [--reps 5] [--out profiles/catvae_bench.json]

train: the VAE, the IWAE at k = 1, the categorical VAE relaxed and with hard=True.  Each repetition times one training
pass of each model in turn (the models alternate, so drift hits all alike) with HIP events (validation excluded: the
engine's run_pass for the training set), after one warm-up epoch per model that captures the graphs.  The baselines are
the VAE's and the IWAE's batches of the same run: ratio_catvae_*_over_vae / _over_iwae_k1.

relax: on 512 rows, gm_cat_sample alone (RELAXED and ST) and gm_cat_reduce alone, against the forward and the forward +
backward of catvae.gumbel_softmax / categorical_kl in torch on the same logits and noise (the gradient of sum(dy . y) + sum
KL taken by autograd): --iters launches between HIP events.

Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic binary images (the bit-packed dataset, as get_data() gives); 50176 = 98 batches of 512."""
import argparse
import json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catvae_bench.json"))
    a = ap.parse_args()
    import torch
    import cat_vae
    import iwae
    import vae
    from generative_models_amd import _lib, ops_fused, trainers
    from generative_models_amd import catvae as gcat

    N, C = 20, 10
    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "num_vars": N, "num_classes": C, "batch": 512,
                      "n_train": a.n_train, "batches_per_epoch": steps, "reps": a.reps, "iters": a.iters},
           "train": {}, "relax": {}}
    models = {"vae": ("VAEEngine", lambda: vae.VAETrainer(vae.VAE(), *its())),
              "iwae_k1": ("IWAEEngine", lambda: iwae.IWAETrainer(iwae.IWAE(), *its(), k=1, seed=0)),
              "catvae_relaxed": ("CatVAEEngine", lambda: cat_vae.CatVAETrainer(cat_vae.CatVAE(784, 400, N, C), *its(),
                                                                               seed=0)),
              "catvae_hard": ("CatVAEEngine", lambda: cat_vae.CatVAETrainer(cat_vae.CatVAE(784, 400, N, C), *its(), seed=0,
                                                                            hard=True))}
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
    for name in ("catvae_relaxed", "catvae_hard"):
        for base in ("vae", "iwae_k1"):
            n = "ratio_%s_over_%s" % (name, base)
            T[n] = med(name) / med(base)
            print("%s = %.3f" % (n, T[n]), flush=True)
    runs.clear()

    # the two launches alone against the torch composition
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
    B, W, dev, tau = 512, N * C, "cuda", 0.7
    gen = torch.Generator().manual_seed(3)
    l = (torch.randn(B, W, generator=gen) * 1.5).to(dev)
    dy = torch.randn(B, W, generator=gen).to(dev)
    wn = torch.ones(B, device=dev)
    yo, lp, kl, dlg = torch.empty(B, W, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), \
        torch.empty(B, W, device=dev)
    noise = ops_fused.iwae_noise(0, gcat.TAG_TRAIN, 1)
    gn = ops_fused.catvae_gumbels(B, 1, N, C, 0, 0, gcat.TAG_TRAIN)
    pl = l.clone().requires_grad_()

    def t_fwd(hard=False):
        with torch.no_grad():
            gcat.gumbel_softmax(l, gn, tau, N, C, hard=hard)
            gcat.categorical_kl(l, N, C)

    def t_both():
        z = gcat.gumbel_softmax(pl, gn, tau, N, C)
        torch.autograd.grad((dy * z).sum() + gcat.categorical_kl(pl, N, C).sum(), (pl,))
    Rl = out["relax"]
    Rl["cat_sample_relaxed"] = timed(lambda: ops_fused.cat_sample(l, yo, lp, noise, B, 1, N, C, _lib.CAT_RELAXED, tau=tau,
                                                                  kl=kl))
    Rl["cat_sample_st"] = timed(lambda: ops_fused.cat_sample(l, yo, lp, noise, B, 1, N, C, _lib.CAT_ST, kl=kl))
    Rl["cat_reduce"] = timed(lambda: ops_fused.cat_reduce(l, dy, wn, dlg, noise, B, N, C, tau=tau))
    Rl["torch_forward"] = timed(t_fwd)
    Rl["torch_forward_hard"] = timed(lambda: t_fwd(True))
    Rl["torch_forward_backward"] = timed(t_both)
    m = lambda n: Rl[n]["us_per_call_median"]
    Rl["ratio_torch_forward_over_cat_sample"] = m("torch_forward") / m("cat_sample_relaxed")
    Rl["ratio_torch_over_fused_both_ways"] = m("torch_forward_backward") / (m("cat_sample_relaxed") + m("cat_reduce"))
    print("relax: sample %.2f (ST %.2f), reduce %.2f, torch forward %.2f (hard %.2f), torch forward + backward %.2f us"
          % (m("cat_sample_relaxed"), m("cat_sample_st"), m("cat_reduce"), m("torch_forward"), m("torch_forward_hard"),
             m("torch_forward_backward")), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
