"""Gaussian Parzen-window log-likelihood: the MNIST number of the GAN paper the reference's GAN headers link
(arXiv 1406.2661, table 1; ns_gan.py:1-5), for comparing trained generators by a distribution-level score.

For query rows x, generator samples s_1..s_N and bandwidth sigma (d = row length):

    ll_sigma(x) = logsumexp_i(-|x - s_i|^2 / (2 sigma^2)) - log N - d log(sigma sqrt(2 pi))

The values come from one fused HIP kernel (gm_parzen_ll, csrc/gm_eval.hip); there is no CPU fallback.
parzen_evaluate picks sigma on validation rows (argmax of the mean, ties to the smaller sigma) and reports the mean
over the test rows with its standard error std / sqrt(n_test) (population std, as numpy's default).
Under data parallelism every rank computes the same value locally: nothing here communicates."""
import collections

import numpy as np
import torch

from . import _lib
from ._lib import GMError

MAX_SIGMAS = 16                      # also the kernel MMD's (GM_MMD_MAX_SIGMAS)

ParzenResult = collections.namedtuple("ParzenResult", "sigma ll_mean ll_stderr val_means")
# VAETrainer.log_likelihood (iwae.py): the importance-weighted estimate of log p(x) over n rows from k samples each
IWAEResult = collections.namedtuple("IWAEResult", "ll_mean ll_stderr k n")
# the exact log-likelihood of a model with a tractable one (made.MADETrainer.log_likelihood), nats per image
NLLResult = collections.namedtuple("NLLResult", "ll_mean ll_stderr n")
# rbm.RBMTrainer.log_likelihood: log p(v) = -F(v) - log Z with log Z by annealed importance sampling (chains x n_betas)
AISResult = collections.namedtuple("AISResult", "ll_mean ll_stderr log_z log_z_stderr chains n_betas n")
# vqvae.VQVAETrainer.log_likelihood: the lower bound log p(x | z) + log p(z) at z = the image's codes, the prior a MADE over
# the codes' bits; ll_mean = recon_mean + prior_mean
VQResult = collections.namedtuple("VQResult", "ll_mean ll_stderr recon_mean prior_mean n")

# tcvae.TCVAETrainer.decomposition: the KL's three terms (index-code mutual information, total correlation, dimension-wise
# KL) and the reconstruction error, per image, over n rows
TCResult = collections.namedtuple("TCResult", "mi tc dw_kl recon n")


def default_sigmas():
    """numpy.logspace(-1, 0, 10): the sigma grid of the evaluation."""
    return np.logspace(-1, 0, 10)


def workspace_bytes(nq, ns, n_sigma):
    """Bytes of device workspace gm_parzen_ll needs (include/gm_hip.h gives the formula)."""
    n = _lib.load().gm_parzen_workspace_bytes(int(nq), int(ns), int(n_sigma))
    if n < 0:
        _lib.check(int(n), "gm_parzen_workspace_bytes")
    return int(n)


def _rows(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        raise GMError("parzen: %s must be a float32 tensor on the MI355X (got %s); there is no CPU fallback"
                      % (what, x.device if isinstance(x, torch.Tensor) else type(x).__name__))
    x = x.reshape(x.shape[0], -1)
    return x if x.stride(1) == 1 else x.contiguous()


def parzen_log_likelihood(samples, data, sigmas):
    """ll[k, j] = ll_{sigmas[k]}(data[j]) under the Parzen window of `samples` -> float32 [len(sigmas), n_data]."""
    s, q = _rows(samples, "samples"), _rows(data, "data")
    if s.shape[1] != q.shape[1]:
        raise GMError("parzen: samples have %d values per row, data %d" % (s.shape[1], q.shape[1]))
    sig = torch.as_tensor(np.asarray(sigmas, dtype=np.float32).reshape(-1)).to(q.device)
    ns, nq, d, k = s.shape[0], q.shape[0], q.shape[1], sig.numel()
    if not 1 <= k <= MAX_SIGMAS:
        raise GMError("parzen: 1 to %d bandwidths per call, got %d" % (MAX_SIGMAS, k))
    if not bool(torch.all(sig > 0)):
        raise GMError("parzen: every sigma must be > 0")
    with torch.cuda.device(q.device):
        ws = torch.empty(workspace_bytes(nq, ns, k), dtype=torch.uint8, device=q.device)
        out = torch.empty(k, nq, dtype=torch.float32, device=q.device)
        _lib.call("gm_parzen_ll", torch.cuda.current_stream().cuda_stream, q.data_ptr(), q.stride(0), nq,
                  s.data_ptr(), s.stride(0), ns, d, sig.data_ptr(), k, ws.data_ptr(), ws.numel(), out.data_ptr(),
                  out.stride(0))
    return out


def select_sigma(sigmas, val_means):
    """Index of the sigma with the largest validation mean; ties go to the smaller sigma."""
    sigmas, val_means = np.asarray(sigmas, dtype=np.float64), np.asarray(val_means, dtype=np.float64)
    if not np.all(np.isfinite(val_means)):
        raise GMError("parzen: non-finite validation mean %s" % val_means)
    best = np.flatnonzero(val_means == val_means.max())
    return int(best[np.argmin(sigmas[best])])


def parzen_evaluate(samples, val, test, sigmas=None):
    """sigma* = argmax over `sigmas` of the mean validation ll; mean and standard error of ll_sigma* on `test`."""
    sig = default_sigmas() if sigmas is None else np.asarray(sigmas, dtype=np.float64).reshape(-1)
    val_means = parzen_log_likelihood(samples, val, sig).double().mean(1).cpu().numpy()
    k = select_sigma(sig, val_means)
    ll = parzen_log_likelihood(samples, test, sig[k:k + 1])[0].double()
    return ParzenResult(float(sig[k]), float(ll.mean()), float(ll.std(unbiased=False)) / np.sqrt(ll.numel()),
                        val_means)


# ---- kernel maximum mean discrepancy (gm_mmd_pairs / gm_mmd_finalize, csrc/gm_gmmn.hip; gmmn.py holds the contract) ------
# mmd2 of n_samples generated rows against n_data data rows under k(a, b) = sum_s exp(-|a - b|^2 / (2 sigma_s^2));
# mmd = sqrt(max(mmd2, 0)).  A two-sample statistic: no bandwidth is picked on validation rows.
MMDResult = collections.namedtuple("MMDResult", "mmd2 mmd n_samples n_data")
MMD_SIGMAS = (2.0, 5.0, 10.0, 20.0, 40.0, 80.0)      # the GMMN paper's data-space bandwidths (arXiv 1502.02761)


def mmd(samples, data, sigmas=None, unbiased=True):
    """The kernel MMD between `samples` [N, ...] and `data` [M, ...] (float32 tensors on the MI355X) -> MMDResult.
    unbiased (needs N, M >= 2): the U-statistic -- the xx and yy sums without their diagonals over N (N - 1) and
    M (M - 1); else the V-statistic of gmmn.py's loss, diagonals in.  Nothing of size N x M is stored."""
    from . import ops_fused as of_
    s, q = _rows(samples, "samples"), _rows(data, "data")
    if s.shape[1] != q.shape[1]:
        raise GMError("mmd: samples have %d values per row, data %d" % (s.shape[1], q.shape[1]))
    n, m = s.shape[0], q.shape[0]
    if min(n, m) < (2 if unbiased else 1):
        raise GMError("mmd: %d samples and %d data rows; the %s statistic needs at least %d of each"
                      % (n, m, "unbiased" if unbiased else "biased", 2 if unbiased else 1))
    with torch.cuda.device(q.device):
        sig = of_.mmd_sigmas(MMD_SIGMAS if sigmas is None else sigmas, q.device, "mmd")
        st = of_.mmd_stats(s, q, sig).cpu().tolist()             # the one sync
    if unbiased:
        mmd2 = st[6] / (n * (n - 1.0)) - 2.0 * st[4] / (float(n) * m) + st[7] / (m * (m - 1.0))
    else:
        mmd2 = st[0]
    return MMDResult(mmd2, float(np.sqrt(max(mmd2, 0.0))), n, m)


# ---- sliced Wasserstein distance (gm_sw_directions / gm_sw_sort / gm_sw_finalize, csrc/gm_sw.hip; swg.py holds the
# contract) ----  swd2 = the mean over n_projections random unit directions of the squared 2-Wasserstein distance between
# the projected samples and the projected data; swd = sqrt(swd2).
SWDResult = collections.namedtuple("SWDResult", "swd2 swd n_projections n_samples n_data")
SWD_BLOCK = 256                      # projections per launch: nothing larger than [256, N + M] is stored
SWD_GROUP = 64                       # gm_sw_finalize adds ws in groups of 64 consecutive projections, in ascending order
assert SWD_BLOCK % SWD_GROUP == 0    # so a block is whole groups, and the block sums close in block order


def sliced_wasserstein(samples, data, n_projections=1024, seed=0):
    """The sliced Wasserstein distance between `samples` [N, ...] and `data` [M, ...] (float32 tensors on the MI355X) ->
    SWDResult.  Any 1 <= N, M <= GM_SW_MAX_ROWS (16384), N != M included; the directions are rows 0 .. n_projections - 1
    of the stream (seed, step 0, "SWDM").  Projections run in blocks of at most SWD_BLOCK; every projection's sum lands in
    one fp64 array and one launch closes it in a fixed order (groups of 64 in ascending order, so block after block)."""
    from . import ops, ops_fused as of_
    s, q = _rows(samples, "samples"), _rows(data, "data")
    if s.shape[1] != q.shape[1] or not 1 <= s.shape[1] <= _lib.MMD_MAX_I:
        raise GMError("sliced_wasserstein: samples have %d values per row, data %d (1 to %d, equal)"
                      % (s.shape[1], q.shape[1], _lib.MMD_MAX_I))
    n, m, I = s.shape[0], q.shape[0], s.shape[1]
    if not (1 <= n <= _lib.SW_MAX_ROWS and 1 <= m <= _lib.SW_MAX_ROWS):
        raise GMError("sliced_wasserstein: %d samples and %d data rows; each projection is sorted in LDS, which holds 1 to "
                      "%d rows a side (a radix sort for more is not implemented)" % (n, m, _lib.SW_MAX_ROWS))
    P = _lib.check_int(n_projections, "n_projections")
    if not 1 <= P <= _lib.SW_MAX_P:
        raise GMError("sliced_wasserstein: n_projections must lie in [1, %d], got %d" % (_lib.SW_MAX_P, P))
    seed = _lib.check_seed(seed)
    with torch.cuda.device(q.device):
        R = torch.cat([s, q], 0).contiguous()
        pb = min(P, SWD_BLOCK)
        theta, Pr = torch.empty(pb, I, device=q.device), torch.empty(pb, n + m, device=q.device)
        ws = of_.sw_workspace(P, q.device)
        stats = torch.zeros(2, dtype=torch.float64, device=q.device)
        for p0 in range(0, P, SWD_BLOCK):
            k = min(SWD_BLOCK, P - p0)
            of_.sw_directions(theta, of_.sw_noise(seed, _lib.SWG_TAG_DM, row0=p0), P=k)
            ops.linear_fwd(theta[:k], R, None, Pr[:k], "id")
            of_.sw_sort(Pr, n, m, ws[p0:p0 + k], P=k)
        of_.sw_finalize(P, n, m, ws, stats)
        st = stats.cpu().tolist()                                    # the one sync
    return SWDResult(st[0], st[1], P, n, m)
