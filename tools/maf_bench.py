#!/usr/bin/env python
"""The masked autoregressive flow against the autoencoder, MADE and RealNVP in microseconds per training batch, and its
one-launch inverse against the general D-pass sampler: 784-400, bs = 512, whole epochs on the graph path.

    python tools/maf_bench.py [--n-train 50176] [--reps 5] [--limit 240] [--out profiles/maf_bench.json]

Every section runs in a child process of its own under its own time limit (--limit seconds); a section that fails or runs
out of time ends the tool, and nothing more is started on the GPU.

train:   the autoencoder, MADE, RealNVP at K = 2 and the MAF at K = 2 and K = 5, alternating in one process,
         tools/ddpm_bench.py's protocol -- each repetition times one training pass of each model in turn with HIP events
         (validation excluded), after one warm-up epoch per model that captures the graphs.
sampler: at n = 64 and n = 10 000 and K = 2, sample(n) of a stock model (the prior normals, K x gm_maf_invert, gm_nvp_post;
         the call's synchronises, the transposed copies of linear.weight and the orders' uploads are inside the figure) and
         of the same weights in a user subclass (the general sampler: D passes per layer, built from the existing GEMM
         launches -- the baseline, not the code under test), wall clock; and gm_maf_invert alone between two HIP events,
         divided by n: microseconds per row.
Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic grey-level images (256 levels, fp32 resident); 50176 = 98 batches of 512."""
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


def summary(us, key):
    med = statistics.median(us)
    return {key + "_median": med, key: us, "spread": (max(us) - min(us)) / med}


def section_train(a):
    import torch
    import ae
    import made
    import maf
    import real_nvp
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.floor(torch.rand(a.n_train, 1, 28, 28, generator=g) * 256.0) / 255.0
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    models = {"ae": (lambda: ae.AutoencoderTrainer(ae.Autoencoder(784, 400), *its()), "AEEngine"),
              "made": (lambda: made.MADETrainer(made.MADE(784, 400), *its()), "MADEEngine"),
              "realnvp_k2": (lambda: real_nvp.RealNVPTrainer(real_nvp.RealNVP(784, 400, 2), *its()), "RealNVPEngine"),
              "maf_k2": (lambda: maf.MAFTrainer(maf.MAF(784, 400, 2), *its()), "MAFEngine"),
              "maf_k5": (lambda: maf.MAFTrainer(maf.MAF(784, 400, 5), *its()), "MAFEngine")}
    runs, out = {}, {}
    for name, (mk, engine) in models.items():
        torch.manual_seed(1234)
        tr = mk()
        with open(os.devnull, "w") as null:
            stdout, sys.stdout = sys.stdout, null
            try:
                tr.train(1)                                  # warm-up: graphs captured
            finally:
                sys.stdout = stdout
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
    for name in ("maf_k2", "maf_k5"):
        for base in ("ae", "made", "realnvp_k2"):
            out["ratio_%s_over_%s" % (name, base)] = out[name]["us_per_batch_median"] / out[base]["us_per_batch_median"]
    return out


def section_sampler(a):
    import torch
    import maf
    from generative_models_amd import maf as gmaf
    from generative_models_amd import ops_fused as of_

    class Edited(maf.MAF):
        """The same network as a user subclass: the general path."""

    K = 2
    x = torch.floor(torch.rand(64, 1, 28, 28, generator=torch.Generator().manual_seed(0)) * 256.0) / 255.0
    dl = lambda: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(64, dtype=torch.int64)),
                                             batch_size=64, shuffle=True)
    torch.manual_seed(1234)
    fused = maf.MAFTrainer(maf.MAF(784, 400, K), dl(), dl(), dl())
    edited = Edited(784, 400, K)
    edited.load_state_dict(fused.model.state_dict())
    general = maf.MAFTrainer(edited, dl(), dl(), dl())
    assert gmaf.maf_fused_ok(fused.model) and not gmaf.maf_fused_ok(general.model)
    out = {"num_layers": K}
    for n in (64, 10000):
        for name, tr in (("fused", fused), ("general", general)):
            tr.sample(n, seed=0)                             # warm-up
            us = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.sample(n, seed=0)                         # ends with a synchronise
                us.append((time.perf_counter() - t0) * 1e6)
            out["%s_n%d" % (name, n)] = summary(us, "us_per_call")
            print("%s sampler n=%d %.1f us / call (median of %d)" % (name, n, statistics.median(us), a.reps), flush=True)
        out["ratio_general_over_fused_n%d" % n] = (out["general_n%d" % n]["us_per_call_median"]
                                                   / out["fused_n%d" % n]["us_per_call_median"])
        print("ratio_general_over_fused_n%d = %.1f" % (n, out["ratio_general_over_fused_n%d" % n]))
        # the kernel alone: one layer's inverse
        c = fused.model.layers[0]
        dev = next(c.parameters()).device
        W1T = c.linear.weight.detach().t().contiguous()
        inv = torch.from_numpy(gmaf.inverse_order(c.m_in)).to(dev)
        u = torch.randn(n, 784, generator=torch.Generator().manual_seed(1)).to(dev)
        ys = torch.empty(n, 784, device=dev)
        args = (u, c.out.weight.detach(), c.out.bias.detach(), W1T, c.linear.bias.detach(), c.m_h, inv, fused.s_cap)
        of_.maf_invert(*args, y=ys)
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            of_.maf_invert(*args, y=ys)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / n)
        out["kernel_n%d" % n] = summary(us, "us_per_row")
        print("gm_maf_invert n=%d %.3f us / row (median of %d)" % (n, statistics.median(us), a.reps), flush=True)
    return out


SECTIONS = {"train": section_train, "sampler": section_sampler}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds each section may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maf_bench.json"))
    ap.add_argument("--section", choices=sorted(SECTIONS), help=argparse.SUPPRESS)     # a child's job
    a = ap.parse_args()
    if a.section:
        print("RESULT " + json.dumps(SECTIONS[a.section](a)))
        return 0
    out = {"config": {"image_size": 784, "hidden_dim": 400, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": (a.n_train + 511) // 512, "reps": a.reps, "limit_s": a.limit}}
    for name in ("train", "sampler"):
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
