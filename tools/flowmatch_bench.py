#!/usr/bin/env python
"""Flow matching in microseconds: a training batch against the DDPM's and RealNVP's, a field evaluation of the solver with
and without the divergence, gm_fm_div against the composition it replaces, the samplers against the DDPM's, and the
likelihood of 10 000 rows.  784-400-32.

    python tools/flowmatch_bench.py [--n-train 50176] [--reps 5] [--iters 50] [--out profiles/flowmatch_bench.json]

train: FlowMatching, DDPM and RealNVP (K = 4) at bs 512.  Each repetition times each model's train(1) in turn on the
host clock around a device synchronise (the models alternate, so drift hits all alike), after one warm-up epoch per
model that captures the graphs; us_per_batch_epoch = the epoch over its training batches (the validation pass and the
epoch's host work are in it for all three alike).

field: us per field evaluation inside the solver at n = 10 000 rows -- heun, 50 steps = 100 evaluations -- sampling (three
forwards + gm_fm_stage) and under the likelihood (+ gm_fm_div); the whole call on the host clock over its evaluations:
the copies of the start rows, the table's upload and, under the likelihood, forming Q are in it (the graph is captured by
the warm-up call and replayed), so the difference of the two figures is an upper bound of the divergence launches' share.

div: gm_fm_div (both launches) at (B, H) = (512, 400) and (10 000, 400) against a mask written by torch, ops.linear_fwd
and a torch row dot on the same operands, between device events over --iters launches.

sample: sample(10 000, steps = 50) per solver against DDPMTrainer.sample(10 000, steps = 50); log_likelihood_rows over
10 000 rows (rk4, 100 steps).

Every timing: the median of --reps repetitions after one warm-up, with all repetitions listed and the spread (max - min)
/ median.  Synthetic grey-level images; the weights are random (`out` included), so no ReLU pattern is degenerate."""
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
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowmatch_bench.json"))
    a = ap.parse_args()
    import torch
    import ddpm
    import flow_matching
    import real_nvp
    from generative_models_amd import ops, ops_fused

    if not torch.cuda.is_available():
        raise SystemExit("flowmatch_bench measures on the MI355X: no GPU is visible")
    dev = "cuda"
    I, H, E, T, bs = 784, 400, 32, 1000, 512
    g = torch.Generator().manual_seed(0)

    def loader(n):
        x = (torch.randint(0, 256, (n, 1, 28, 28), generator=g).float() / 255.0)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=True)
    its = loader(a.n_train), loader(bs), loader(bs)
    n_batches = len(its[0])

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, out

    def quiet(fn):
        with contextlib.redirect_stdout(io.StringIO()):
            return fn()

    torch.manual_seed(1)
    fm = flow_matching.FlowMatching(I, H, E, T)
    with torch.no_grad():
        torch.nn.init.normal_(fm.field.out.weight, std=0.5 / H ** 0.5)
    trainers_ = {
        "flowmatch": flow_matching.FlowMatchingTrainer(fm, *its),
        "ddpm": ddpm.DDPMTrainer(ddpm.DDPM(I, H, E, T), *its),
        "realnvp_k4": real_nvp.RealNVPTrainer(real_nvp.RealNVP(I, H, 4), *its),
    }
    res = {"shape": {"I": I, "H": H, "E": E, "T": T, "batch": bs, "n_train": a.n_train, "batches": n_batches},
           "reps": a.reps, "iters": a.iters, "train": {}, "field": {}, "div": {}, "sample": {}}
    for tr in trainers_.values():
        quiet(lambda: tr.train(1))                              # warm-up: graphs captured
    times = {k: [] for k in trainers_}
    for _ in range(a.reps):
        for k, tr in trainers_.items():
            times[k].append(sync_time(lambda: quiet(lambda: tr.train(1)))[0] / n_batches)
    for k, us in times.items():
        res["train"][k] = record(us, "us_per_batch_epoch")
    ref = res["train"]["flowmatch"]["us_per_batch_epoch_median"]
    res["train"]["flowmatch_over_ddpm"] = ref / res["train"]["ddpm"]["us_per_batch_epoch_median"]
    res["train"]["flowmatch_over_realnvp_k4"] = ref / res["train"]["realnvp_k4"]["us_per_batch_epoch_median"]

    # the solver: a field evaluation with and without the divergence
    tr = trainers_["flowmatch"]
    n = a.rows
    y = torch.randn(n, I, device=dev)
    for name, div in (("sampling", False), ("likelihood", True)):
        tr._solve(y, -1, 50, "heun", with_div=div)
        us = [sync_time(lambda: tr._solve(y, -1, 50, "heun", with_div=div))[0] / 100 for _ in range(a.reps)]
        res["field"][name] = dict(record(us, "us_per_evaluation"), rows=n, evaluations=100,
                                  launches_per_evaluation=5 if div else 4)
    res["field"]["divergence_share"] = 1.0 - (res["field"]["sampling"]["us_per_evaluation_median"]
                                              / res["field"]["likelihood"]["us_per_evaluation_median"])

    # gm_fm_div against the composition it replaces
    def events(fn):
        fn()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        return out

    Q = tr.divergence_matrix()
    zero = torch.zeros(H, device=dev)
    for B in (512, n):
        H1, H2 = torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)
        part, out = torch.empty(ops_fused.fm_div_tiles(H), B, device=dev), torch.empty(B, device=dev)
        mask, prod = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)

        def composed():                                         # prod[b, i] = sum_j m1[b, j] Q[i, j]: W = Q as it stands
            mask.copy_(H1 > 0)
            ops.linear_fwd(mask, Q, zero, prod, "id")
            return (prod * (H2 > 0)).sum(1)

        kern = events(lambda: ops_fused.fm_div(H1, H2, Q, part=part, div=out))
        comp = events(composed)
        d = (out - composed()).abs().max().item()
        res["div"]["B%d_H%d" % (B, H)] = dict(record(kern, "kernel_us"), **record(comp, "composition_us"),
                                              composition_over_kernel=statistics.median(comp) / statistics.median(kern),
                                              max_abs_difference=d)

    # the samplers and the likelihood
    for solver in ("euler", "heun", "rk4"):
        tr.sample(n, steps=50, solver=solver)
        us = [sync_time(lambda: tr.sample(n, seed=r, steps=50, solver=solver))[0] for r in range(a.reps)]
        res["sample"][solver] = dict(record(us, "us"), rows=n, steps=50)
    dt = trainers_["ddpm"]
    dt.sample(n, steps=50)
    us = [sync_time(lambda: dt.sample(n, seed=r, steps=50))[0] for r in range(a.reps)]
    res["sample"]["ddpm"] = dict(record(us, "us"), rows=n, steps=50)
    x = torch.rand(n, I, generator=g)
    tr.log_likelihood_rows(x)
    us = [sync_time(lambda: tr.log_likelihood_rows(x))[0] for _ in range(a.reps)]
    res["log_likelihood"] = dict(record(us, "us"), rows=n, steps=100, solver="rk4", evaluations=400, batch=1024)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("train", "field", "div")}, indent=1, sort_keys=True)[:3000])


if __name__ == "__main__":
    main()
