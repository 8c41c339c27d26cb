#!/usr/bin/env python
"""The restricted Boltzmann machine in microseconds: a training batch against the plain autoencoder's, a Gibbs step of the
one-launch chain against the torch composition of the same step, a whole sample and an AIS run: 784-400, bs = 512.

    python tools/rbm_bench.py [--n-train 50176] [--reps 5] [--limit 240] [--out profiles/rbm_bench.json]

Every section runs in a child process of its own under its own time limit (--limit seconds); a section that fails or runs
out of time ends the tool, and nothing more is started on the GPU.

train:  the autoencoder (784-400, 5 launches per batch) and the RBM under CD-1 (8 launches), CD-10 (8) and PCD-1 (10),
        alternating in one process, tools/made_bench.py's protocol -- each repetition times one training pass of each
        model in turn with HIP events (validation excluded), after one warm-up epoch per model that captures the graphs.
chain:  at n = 64, 512 and 10 000 chains, gm_rbm_chain alone between two HIP events for --chain-steps Gibbs steps,
        divided by the steps: microseconds per Gibbs step; and the torch composition of the same steps on the same
        uniforms (gm_rbm_uniform, two matmuls, two sigmoids, two compares per step), timed the same way over
        --torch-steps steps.  The crossover is read off the two columns.
sample: sample(10 000, steps=1000) of a stock model, wall clock (the call's synchronises and the transpose inside).
ais:    log-weights of 512 chains x 1000 uniformly spaced betas (RBMTrainer.ais), wall clock.
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
    import rbm
    from generative_models_amd import trainers

    g = torch.Generator().manual_seed(0)
    x = torch.bernoulli(torch.full((a.n_train, 1, 28, 28), 0.1307), generator=g)
    y = torch.zeros(a.n_train, dtype=torch.int64)
    dl = lambda n=None: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x[:n], y[:n]), batch_size=512,
                                                    shuffle=True)
    its = lambda: (dl(), dl(512), dl(512))
    steps = (a.n_train + 511) // 512
    mk_rbm = lambda k, mode: (lambda: rbm.RBMTrainer(rbm.RBM(784, 400), *its(), k=k, mode=mode))
    models = {"ae": lambda: ae.AutoencoderTrainer(ae.Autoencoder(784, 400), *its()),
              "cd1": mk_rbm(1, "cd"), "cd10": mk_rbm(10, "cd"), "pcd1": mk_rbm(1, "pcd")}
    runs, out = {}, {}
    for name, mk in models.items():
        torch.manual_seed(1234)
        tr = mk()
        quiet(lambda: tr.train(1))                           # warm-up: graphs captured
        assert type(tr._engine).__name__ == ("AEEngine" if name == "ae" else "RBMEngine")
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
    for name in ("cd1", "cd10", "pcd1"):
        out["ratio_%s_over_ae" % name] = out[name]["us_per_batch_median"] / out["ae"]["us_per_batch_median"]
    return out


def _trained(n_train=4096):
    """A stock trainer after one epoch on synthetic digits-like rows: weights away from their initial values."""
    import torch
    import rbm
    x = torch.bernoulli(torch.full((n_train, 1, 28, 28), 0.1307), generator=torch.Generator().manual_seed(0))
    dl = lambda: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(n_train, dtype=torch.int64)),
                                             batch_size=512, shuffle=True)
    torch.manual_seed(1234)
    tr = rbm.RBMTrainer(rbm.RBM(784, 400), dl(), dl(), dl())
    quiet(lambda: tr.train(1))
    return tr


def section_chain(a):
    import torch
    from generative_models_amd import ops_fused as of_
    from generative_models_amd._lib import RBM_TAG_H, RBM_TAG_V

    tr = _trained()
    W, WT, c, b = tr._weights()
    dev = W.device
    out = {}

    def timed(fn, per):
        fn()                                                 # warm-up
        us = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / per)
        return summary(us, "us_per_step")

    for n in (64, 512, 10000):
        x = torch.full((n, 784), 0.5, device=dev)
        v = torch.empty(n, 784, device=dev)
        out["kernel_n%d" % n] = timed(lambda: of_.rbm_chain(W, WT, c, b, x, a.chain_steps, 0, v_out=v), a.chain_steps)

        def composed():
            cur = (of_.rbm_uniform(n, 784, 0, 0x52424D44, device=dev) < x).float()
            for s in range(a.torch_steps):
                ph = torch.sigmoid(torch.addmm(c, cur, WT))
                h = (of_.rbm_uniform(n, 400, 0, RBM_TAG_H, step=s, device=dev) < ph).float()
                pv = torch.sigmoid(torch.addmm(b, h, W))
                cur = (of_.rbm_uniform(n, 784, 0, RBM_TAG_V, step=s, device=dev) < pv).float()
            return cur
        out["torch_n%d" % n] = timed(composed, a.torch_steps)
        out["ratio_torch_over_kernel_n%d" % n] = (out["torch_n%d" % n]["us_per_step_median"]
                                                  / out["kernel_n%d" % n]["us_per_step_median"])
        print("n=%d: gm_rbm_chain %.2f us / Gibbs step, torch composition %.2f, ratio %.2f"
              % (n, out["kernel_n%d" % n]["us_per_step_median"], out["torch_n%d" % n]["us_per_step_median"],
                 out["ratio_torch_over_kernel_n%d" % n]), flush=True)
    return out


def _wall(fn, reps):
    import torch
    fn()                                                     # warm-up
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                                 # ends with a synchronise
        ms.append((time.perf_counter() - t0) * 1e3)
    return summary(ms, "ms_per_call")


def section_sample(a):
    tr = _trained()
    out = {"sample_n10000_steps1000": _wall(lambda: tr.sample(10000, seed=0, steps=1000), a.reps)}
    print("sample(10 000, steps=1000) %.2f ms" % out["sample_n10000_steps1000"]["ms_per_call_median"], flush=True)
    return out


def section_ais(a):
    tr = _trained()
    out = {"ais_512x1000": _wall(lambda: tr.ais(chains=512, betas=1000, seed=0), a.reps)}
    print("AIS 512 chains x 1000 betas %.2f ms" % out["ais_512x1000"]["ms_per_call_median"], flush=True)
    return out


SECTIONS = {"train": section_train, "chain": section_chain, "sample": section_sample, "ais": section_ais}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=50176)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain-steps", type=int, default=200)
    ap.add_argument("--torch-steps", type=int, default=20)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds each section may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbm_bench.json"))
    ap.add_argument("--section", choices=sorted(SECTIONS), help=argparse.SUPPRESS)     # a child's job
    a = ap.parse_args()
    if a.section:
        print("RESULT " + json.dumps(SECTIONS[a.section](a)))
        return 0
    out = {"config": {"image_size": 784, "hidden_dim": 400, "batch": 512, "n_train": a.n_train,
                      "batches_per_epoch": (a.n_train + 511) // 512, "reps": a.reps, "chain_steps": a.chain_steps,
                      "torch_steps": a.torch_steps, "limit_s": a.limit}}
    for name in ("train", "chain", "sample", "ais"):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", name, "--n-train", str(a.n_train), "--reps",
               str(a.reps), "--chain-steps", str(a.chain_steps), "--torch-steps", str(a.torch_steps)]
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
