#!/usr/bin/env python
"""RealNVP against the autoencoder and the VAE in microseconds per training batch, its row kernels against the torch
composition of the same arithmetic, and its sampler against MADE's one-launch sampler: 784-400, bs = 512.

    python tools/realnvp_bench.py [--n-train 50176] [--reps 5] [--limit 240] [--out profiles/realnvp_bench.json]

Every section runs in a child process of its own under its own time limit (--limit seconds); a section that fails or runs
out of time ends the tool, and nothing more is started on the GPU.

train:   the autoencoder, the VAE and the fused RealNVP at K = 2, 4, 8 couplings, alternating in one process,
         tools/made_bench.py's protocol -- each repetition times one training pass of each model in turn with HIP events
         (validation excluded), after one warm-up epoch per model that captures the graphs.
kernels: the five row kernels of one K = 4 coupling stack at b = 512 (gm_nvp_pre, 4 x gm_nvp_couple, gm_nvp_loss with dz,
         4 x gm_nvp_couple_bwd, and the sampler's gm_nvp_post) between two HIP events, against realnvp.preprocess / the
         coupling arithmetic / nll_rows / their autograd backward / postprocess in torch on the same ST and noise (the
         torch side reads u from memory, keeps its leaves and output buffer across calls and splits / merges the halves
         by index); and each kernel alone, 20 launches back to back (gm_nvp_couple in its inverse mode).
sampler: sample(64) and sample(10 000) of a stock RealNVP (3 K + 2 launches, K = 4) and of a stock MADE (one launch), wall
         clock, each call's synchronises included.
Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic binary images (the bit-packed dataset, as get_data() gives); 50176 = 98 batches of 512."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))

KS = (2, 4, 8)


def summary(us, key):
    med = statistics.median(us)
    return {key + "_median": med, key: us, "spread": (max(us) - min(us)) / med}


def quiet(fn):
    with open(os.devnull, "w") as null:
        stdout, sys.stdout = sys.stdout, null
        try:
            return fn()
        finally:
            sys.stdout = stdout


def section_train(a):
    import torch
    import ae
    import real_nvp
    import vae
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    models = {"ae": ("AEEngine", lambda: ae.AutoencoderTrainer(ae.Autoencoder(784, 400), *its())),
              "vae": ("VAEEngine", lambda: vae.VAETrainer(vae.VAE(), *its()))}
    for K in KS:
        models["realnvp_k%d" % K] = ("RealNVPEngine",
                                     lambda K=K: real_nvp.RealNVPTrainer(real_nvp.RealNVP(784, 400, K), *its()))
    runs, out = {}, {}
    for name, (engine, mk) in models.items():
        torch.manual_seed(1234)
        tr = mk()
        quiet(lambda: tr.train(1))                          # warm-up: graphs captured
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
    for name, (_, _, _, us) in runs.items():
        out[name] = summary(us, "us_per_batch")
        print(name, "%.2f us / batch (median of %d epochs)" % (out[name]["us_per_batch_median"], a.reps), flush=True)
    for K in KS:
        for base in ("ae", "vae"):
            key = "ratio_realnvp_k%d_over_%s" % (K, base)
            out[key] = out["realnvp_k%d" % K]["us_per_batch_median"] / out[base]["us_per_batch_median"]
            print("%s = %.3f" % (key, out[key]))
    return out


def section_kernels(a):
    import numpy as np
    import torch
    from generative_models_amd import ops_fused as of_
    from generative_models_amd import realnvp as gnvp

    dev, b, D, K, cap, alpha, levels = "cuda", 512, 784, 4, 2.0, 0.05, 256
    Dh = D // 2
    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((b, D), 0.1307), generator=g).to(dev)
    st = [((torch.rand(b, 2 * Dh, generator=g) * 2 - 1) * 1.5).to(dev) for _ in range(K)]
    ya, yb, ld, part = (torch.empty(b, Dh, device=dev), torch.empty(b, Dh, device=dev), torch.empty(b, device=dev),
                        torch.empty(b, device=dev))
    Y = [torch.empty(b, Dh, device=dev) for _ in range(K)]
    dza, dzb = torch.empty(b, Dh, device=dev), torch.empty(b, Dh, device=dev)
    dST, dX = torch.empty(b, 2 * Dh, device=dev), torch.empty(b, Dh, device=dev)
    xo = torch.empty(b, D, device=dev)
    cst, scale = float(np.float32(gnvp.nll_constant(D, levels))), float(np.float32(1.0 / b))
    u = of_.nvp_uniforms(b, D, 0, gnvp.TAG_TRAIN, device=dev)
    ia, ib = (torch.from_numpy(i).to(dev) for i in gnvp.split_indices(D, "checker"))

    def chain():
        cur = [ya, yb]
        for k in range(K):
            t = 1 - (k & 1)
            yield k, t, cur[t]
            cur[t] = Y[k]

    def fused():
        of_.nvp_pre(x, ya, yb, ld, b, 0, gnvp.TAG_TRAIN, alpha, levels, "checker")
        for k, t, xt in chain():
            of_.nvp_couple(st[k], xt, Y[k], b, Dh, cap, logdet=ld)
        of_.nvp_loss(Y[K - 1], Y[K - 2], ld, part, b, cst, scale=scale, dza=dza, dzb=dzb)
        for k, t, xt in reversed(list(chain())):
            of_.nvp_couple_bwd(st[k], xt, dza if t == 0 else dzb, dST, b, Dh, cap, -scale, dx=dX)
        of_.nvp_post(Y[K - 1], Y[K - 2], xo, b, alpha, "checker")

    sts = [s.clone().requires_grad_(True) for s in st]      # the torch side's leaves and output, made once
    xt_out = torch.empty(b, D, device=dev)

    def composed():
        for s in sts:
            s.grad = None
        y, ld0 = gnvp.preprocess(x, u, alpha, levels)
        h = [y[:, ia], y[:, ib]]
        logdet = torch.zeros(b, device=dev)
        for k in range(K):
            t = 1 - (k & 1)
            s = cap * torch.tanh(sts[k][:, :Dh])
            h[t] = h[t] * torch.exp(s) + sts[k][:, Dh:]
            logdet = logdet + s.sum(1)
        z = torch.cat(h, 1)
        (gnvp.nll_rows(z, ld0, logdet, D, levels).sum() / b).backward()
        with torch.no_grad():
            xt_out[:, ia], xt_out[:, ib] = gnvp.postprocess(h[0], alpha), gnvp.postprocess(h[1], alpha)
        return xt_out

    out = {"launches_fused": 2 * K + 3}
    for name, fn in (("fused", fused), ("torch", composed)):
        fn()
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0)
        out[name] = summary(us, "us_per_stack")
        print("%s row work of one K = %d stack: %.1f us (median of %d)" % (name, K, statistics.median(us), a.reps), flush=True)
    out["ratio_torch_over_fused"] = out["torch"]["us_per_stack_median"] / out["fused"]["us_per_stack_median"]
    print("ratio_torch_over_fused = %.2f" % out["ratio_torch_over_fused"])
    # each kernel alone, 20 launches between two events
    single = {"gm_nvp_pre": lambda: of_.nvp_pre(x, ya, yb, ld, b, 0, gnvp.TAG_TRAIN, alpha, levels, "checker"),
              "gm_nvp_couple": lambda: of_.nvp_couple(st[0], yb, Y[0], b, Dh, cap, inverse=True),
              "gm_nvp_loss": lambda: of_.nvp_loss(Y[K - 1], Y[K - 2], ld, part, b, cst, scale=scale, dza=dza, dzb=dzb),
              "gm_nvp_couple_bwd": lambda: of_.nvp_couple_bwd(st[0], yb, dzb, dST, b, Dh, cap, -scale, dx=dX),
              "gm_nvp_post": lambda: of_.nvp_post(Y[K - 1], Y[K - 2], xo, b, alpha, "checker")}
    for name, fn in single.items():
        fn()
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / 20)
        out[name] = summary(us, "us_per_launch")
        print("%s %.2f us / launch back to back (median of %d)" % (name, statistics.median(us), a.reps), flush=True)
    return out


def section_sampler(a):
    import torch
    import made
    import real_nvp

    x = torch.bernoulli(torch.full((64, 1, 28, 28), 0.1307), generator=torch.Generator().manual_seed(0))
    dl = lambda: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(64, dtype=torch.int64)),
                                             batch_size=64, shuffle=True)
    torch.manual_seed(1234)
    trainers = {"realnvp_k4": real_nvp.RealNVPTrainer(real_nvp.RealNVP(784, 400, 4), dl(), dl(), dl()),
                "made": made.MADETrainer(made.MADE(784, 400), dl(), dl(), dl())}
    out = {}
    for n in (64, 10000):
        for name, tr in trainers.items():
            tr.sample(n, seed=0)                             # warm-up
            us = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.sample(n, seed=0)                         # ends with a synchronise
                us.append((time.perf_counter() - t0) * 1e6)
            out["%s_n%d" % (name, n)] = summary(us, "us_per_call")
            print("%s sample(%d) %.1f us / call (median of %d)" % (name, n, statistics.median(us), a.reps), flush=True)
        out["ratio_made_over_realnvp_n%d" % n] = (out["made_n%d" % n]["us_per_call_median"]
                                                  / out["realnvp_k4_n%d" % n]["us_per_call_median"])
        print("ratio_made_over_realnvp_n%d = %.2f" % (n, out["ratio_made_over_realnvp_n%d" % n]))
    return out


SECTIONS = {"train": section_train, "kernels": section_kernels, "sampler": section_sampler}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds each section may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realnvp_bench.json"))
    ap.add_argument("--section", choices=sorted(SECTIONS), help=argparse.SUPPRESS)     # a child's job
    a = ap.parse_args()
    if a.section:
        print("RESULT " + json.dumps(SECTIONS[a.section](a)))
        return 0
    out = {"config": {"image_size": 784, "hidden_dim": 400, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": (a.n_train + 511) // 512, "couplings": list(KS), "reps": a.reps,
                      "limit_s": a.limit}}
    for name in ("train", "kernels", "sampler"):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--n-train", str(a.n_train), "--reps",
               str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print("section %s ran past its limit of %.0f s: stopping" % (name, a.limit))
            return 2
        sys.stdout.write("".join(l + "\n" for l in r.stdout.splitlines() if not l.startswith("RESULT ")))
        if r.returncode != 0:
            sys.stdout.write(r.stderr)
            print("section %s failed (exit status %d): stopping" % (name, r.returncode))
            return 1
        out[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
