#!/usr/bin/env python
"""Parzen-window log-likelihood: the fused kernel (gm_parzen_ll) against a chunked torch composition, same process.

    python tools/parzen_bench.py [--reps 10] [--out results/parzen_bench.json]

Shapes: 10 000 queries x 10 000 samples x 784 with 10 sigmas (the evaluation's sigma search), and 2 000 x 10 000 x 784
with one sigma.  The kernel is timed with HIP events around `reps` back-to-back calls after warm-up, workspace and
output allocated once.  The torch composition is mm + row norms + logsumexp per sigma over 1 000-query chunks (it
never holds the full distance matrix either).  FLOP = 2 nq ns d (the distance dot products); the share is of the
FP32-input MFMA peak of an MI355X (157.3 TFLOP/s)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from generative_models_amd import _lib, metrics  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_parzen(s, q, sig, chunk=1000):
    n, d = s.shape
    sn = (s * s).sum(1)
    out = torch.empty(len(sig), q.shape[0], device=q.device)
    for i in range(0, q.shape[0], chunk):
        qc = q[i:i + chunk]
        a = torch.addmm((qc * qc).sum(1)[:, None] + sn[None, :], qc, s.t(), beta=-0.5)
        for k, sg in enumerate(sig):
            out[k, i:i + chunk] = torch.logsumexp(a / (sg * sg), 1) - math.log(n) - d * math.log(sg * math.sqrt(2 * math.pi))
    return out


def run(nq, ns, d, n_sigma, warmup, reps):
    g = torch.Generator().manual_seed(0)
    q = (torch.rand(nq, d, generator=g) < 0.13).float().cuda()
    s = torch.rand(ns, d, generator=g).cuda()
    sig = list(np.logspace(-1, 0, 10)) if n_sigma == 10 else [0.2]
    sig_d = torch.tensor(np.asarray(sig, dtype=np.float32)).cuda()
    ws = torch.empty(metrics.workspace_bytes(nq, ns, n_sigma), dtype=torch.uint8, device="cuda")
    out = torch.empty(n_sigma, nq, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        _lib.call("gm_parzen_ll", stream, q.data_ptr(), q.stride(0), nq, s.data_ptr(), s.stride(0), ns, d,
                  sig_d.data_ptr(), n_sigma, ws.data_ptr(), ws.numel(), out.data_ptr(), out.stride(0))

    ms = timed(kernel, warmup, reps)
    t_ms = timed(lambda: torch_parzen(s, q, sig), 1, max(1, reps // 5))
    dev = (out - torch_parzen(s, q, sig)).abs().max().item()
    flop = 2.0 * nq * ns * d
    tf = flop / (ms * 1e-3) / 1e12
    return {"shape": [nq, ns, d], "n_sigma": n_sigma, "kernel_ms": round(ms, 4), "tflops": round(tf, 2),
            "share_of_fp32_mfma_peak": round(tf / PEAK_TFLOPS, 3), "torch_ms": round(t_ms, 4),
            "speedup_vs_torch": round(t_ms / ms, 2), "max_abs_diff_vs_torch": dev, "gflop": round(flop / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run(10000, 10000, 784, 10, a.warmup, a.reps), run(2000, 10000, 784, 1, a.warmup, a.reps)]
    for r in rows:
        print("%-18s S=%-2d kernel %8.3f ms  %6.1f TFLOP/s  %.3f of peak | torch %8.3f ms  x%.1f" % (
            "x".join(map(str, r["shape"])), r["n_sigma"], r["kernel_ms"], r["tflops"], r["share_of_fp32_mfma_peak"],
            r["torch_ms"], r["speedup_vs_torch"]))
    res = {"device": torch.cuda.get_device_name(), "peak_fp32_mfma_tflops": PEAK_TFLOPS, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
