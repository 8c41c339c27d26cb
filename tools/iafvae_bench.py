#!/usr/bin/env python
"""The IAF-VAE against the VAE, the IWAE and the planar NF-VAE in microseconds per training batch, and its three flow
launches against the torch chain of the general path: 784-400-20, F = 64, C = 20, bs = 512, whole epochs on the graph path.
tools/nfvae_bench.py's protocol.

    python tools/iafvae_bench.py [--n-train 50176] [--reps 5] [--out profiles/iafvae_bench.json]

train: the VAE, the IWAE at k = 1 and 5, the NF-VAE at K = 4 and the IAF-VAE at K in {2, 4, 8}, both x k in {1, 5}.  Each
repetition times one training pass of each model in turn (the models alternate, so drift hits all alike) with HIP events
(validation excluded: the engine's run_pass for the training set), after one warm-up epoch per model that captures the
graphs.  The yardstick of what the flow costs is the IWAE at the same k taken in the same run:
ratio_iafvae_K*_k*_over_iwae_k*.  No ratio is fixed in advance.

chain: at K in {2, 4, 8}, k in {1, 5}, 512 images: gm_iaf_sample alone and gm_iaf_reduce + gm_iaf_step alone, against the
forward and the forward + backward of iafvae.iaf_chain in torch on the same rows (z_0 and h given, the gradient of
sum(dzdec . z_K - wn lp) taken by autograd): --iters launches between HIP events.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iafvae_bench.json"))
    a = ap.parse_args()
    import torch
    import iwae
    import iaf_vae
    import nf_vae
    import vae
    from generative_models_amd import iafvae as giaf
    from generative_models_amd import ops, ops_fused, trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    out = {"config": {"image_size": 784, "hidden_dim": 400, "z_dim": 20, "batch": 512, "n_train": a.n_train,
                      "flow_hidden": 64, "context_dim": 20,
                      "batches_per_epoch": steps, "reps": a.reps, "iters": a.iters}, "train": {}, "chain": {}}
    KS, ks = (2, 4, 8), (1, 5)
    models = {"vae": ("VAEEngine", lambda: vae.VAETrainer(vae.VAE(), *its()))}
    for k in ks:
        models["iwae_k%d" % k] = ("IWAEEngine", lambda k=k: iwae.IWAETrainer(iwae.IWAE(), *its(), k=k, seed=0))
    for k in ks:
        models["nfvae_K4_k%d" % k] = ("NFVAEEngine", lambda k=k: nf_vae.NFVAETrainer(
            nf_vae.NFVAE(num_flows=4), *its(), k=k, seed=0))
    for K in KS:
        for k in ks:
            models["iafvae_K%d_k%d" % (K, k)] = ("IAFVAEEngine", lambda K=K, k=k: iaf_vae.IAFVAETrainer(
                iaf_vae.IAFVAE(num_flows=K, flow_hidden=64, context_dim=20), *its(), k=k, seed=0))
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
    for k in ks:
        T["ratio_nfvae_K4_k%d_over_iwae_k%d" % (k, k)] = med("nfvae_K4_k%d" % k) / med("iwae_k%d" % k)
    for K in KS:
        for k in ks:
            n = "ratio_iafvae_K%d_k%d_over_iwae_k%d" % (K, k, k)
            T[n] = med("iafvae_K%d_k%d" % (K, k)) / med("iwae_k%d" % k)
            print("%s = %.3f" % (n, T[n]), flush=True)
    runs.clear()

    # the two flow kernels alone against the torch chain
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
    B, Z, F, Cx, dev = 512, 20, 64, 20, "cuda"
    C = out["chain"]
    for K in KS:
        for k in ks:
            gen = torch.Generator().manual_seed(K * 10 + k)
            ml = torch.randn(B, 2 * Z + Cx, generator=gen)
            ml[:, Z:2 * Z] = ml[:, Z:2 * Z] * 0.5 - 1.0
            ml = ml.to(dev)
            torch.manual_seed(K * 10 + k)
            fl = giaf.IAFFlow(K, Z, F, Cx)
            with torch.no_grad():                            # a fresh flow's W2 is zero: give it work to do
                fl.W2.copy_(torch.randn(K, 2 * Z, F, generator=gen) / 8.0)
                fl.apply_masks()
            fl = fl.to(dev)
            params = tuple(p.detach().contiguous() for p in fl.tensors())
            wn = torch.softmax(torch.randn(B, k, generator=gen), 1).reshape(-1).to(dev)
            dzdec = torch.randn(B * k, Z, generator=gen).to(dev)
            z, lp = torch.empty(B * k, Z, device=dev), torch.empty(B * k, device=dev)
            dml = torch.empty(B, 2 * Z + Cx, device=dev)
            part = ops_fused.iaf_parts(B, k, K, Z, F, Cx, device=dev)
            mom = [(torch.zeros(p.numel(), device=dev), torch.zeros(p.numel(), device=dev)) for p in params]
            sched = torch.from_numpy(ops.adam_schedule(0.0, 1)).to(dev)          # lr 0: the parameters stay
            noise, blk = ops_fused.iwae_noise(0, 1, k), ops_fused.iaf_params(*params)
            m_in = fl.m_in.contiguous()

            def bwd():
                ops_fused.iaf_reduce(ml, wn, dzdec, dml, part, noise, blk, B, k, Z)
                ops_fused.iaf_step(part, B, k, params, m_in, mom, sched)
            z0 = (ml[:, None, :Z] + torch.randn(B, k, Z, device=dev) * torch.exp(ml[:, None, Z:2 * Z] / 2)).reshape(B * k, Z)
            h = ml[:, None, 2 * Z:].expand(B, k, Cx).reshape(B * k, Cx).contiguous()
            pz, ph = z0.clone().requires_grad_(), h.clone().requires_grad_()

            def t_fwd():
                with torch.no_grad():
                    giaf.iaf_chain(z0, h, fl)

            def t_both():
                zk, ld = giaf.iaf_chain(pz, ph, fl)
                loss = (dzdec * zk).sum() - (wn * (ld - 0.5 * (zk * zk).sum(1))).sum()
                torch.autograd.grad(loss, (pz, ph) + tuple(fl.parameters()))
            tag = "K%d_k%d" % (K, k)
            C[tag] = {"iaf_sample": timed(lambda: ops_fused.iaf_sample(ml, z, lp, noise, blk, B, k, Z)),
                      "iaf_reduce_step": timed(bwd), "torch_forward": timed(t_fwd),
                      "torch_forward_backward": timed(t_both)}
            m = lambda n: C[tag][n]["us_per_call_median"]
            C[tag]["ratio_torch_forward_over_iaf_sample"] = m("torch_forward") / m("iaf_sample")
            C[tag]["ratio_torch_over_fused_both_ways"] = m("torch_forward_backward") / (m("iaf_sample")
                                                                                       + m("iaf_reduce_step"))
            print("chain %s: sample %.2f, reduce + step %.2f, torch forward %.2f, torch forward + backward %.2f us"
                  % (tag, m("iaf_sample"), m("iaf_reduce_step"), m("torch_forward"), m("torch_forward_backward")),
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
