"""Parzen-window log-likelihood on the MI355X (gm_parzen_ll, metrics.py, the trainers' sample() / parzen()).

Kernel bound.  The fp64 reference is the direct-difference formula (|x - s|^2 summed term by term in float64).  The
kernel evaluates the norm expansion -(|x|^2 + |s|^2) / 2 + x.s in fp32, so its error is that of an fp32 dot product
chain against the row norms, divided by sigma^2.  The same expansion computed in fp32 by torch on the CPU (its own
summation order) carries an error of the same kind; as in test_gpu_ops.close64 the kernel must stay within TWICE the
CPU's largest error over the queries (measured in units of 1 + |ll|) plus a floor of 1e-5 (1 + |ll|) for what the
CPU expansion does not round: the kernel's fp32 exponent scale log2(e) / sigma^2, its fp32 partial sums and its fp32
output."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

from generative_models_amd import metrics  # noqa: E402

DEV = "cuda"
LOG_2PI = float(np.log(2 * np.pi))
SIGMAS = {1: [0.2], 3: [0.1, 0.3, 1.0], 10: list(np.logspace(-1, 0, 10))}
SIGMAS[3] = [SIGMAS[10][0], 0.3, SIGMAS[10][-1]]
REF_SIGMAS = SIGMAS[10] + [0.2, 0.3]                    # one fp64 reference per data set serves every S


def _sig(s):
    return torch.tensor(np.asarray(s, dtype=np.float32)).double()     # what the kernel sees


def ll_from_neg_half_d2(a, n, d, sig64):
    """a [nq, ns] = -|x - s|^2 / 2 (float64) -> ll [S, nq] float64."""
    return torch.stack([torch.logsumexp(a / (s * s), dim=1) - np.log(n) - d * (torch.log(s) + 0.5 * LOG_2PI)
                        for s in sig64])


def refs(q, s, sig):
    """(fp64 direct-difference ll, fp32 norm-expansion ll) on the CPU."""
    sig64 = _sig(sig)
    d2 = torch.cdist(q.double(), s.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2
    ll64 = ll_from_neg_half_d2(-0.5 * d2, s.shape[0], q.shape[1], sig64)
    a32 = -0.5 * ((q * q).sum(1)[:, None] + (s * s).sum(1)[None, :]) + q @ s.t()
    ll32 = ll_from_neg_half_d2(a32.double(), s.shape[0], q.shape[1], sig64)
    return ll64, ll32


def check_bound(got, ll64, ll32, what):
    got = got.detach().cpu().double()
    unit = 1.0 + ll64.abs()
    e_cpu = ((ll32 - ll64).abs() / unit).amax(dim=1, keepdim=True)       # per sigma, worst query
    err = (got - ll64).abs() / unit
    assert torch.isfinite(got).all(), what
    bad = err > 2.0 * e_cpu + 1e-5
    assert not bad.any(), "%s: %d values out of bound; worst %.3e vs cpu %.3e" % (
        what, int(bad.sum()), float(err.max()), float(e_cpu.max()))


def data(nq, ns, d, kind, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.rand(nq, d, generator=g)
    if kind == "binary":
        q = (q < 0.13).float()
    s = torch.rand(ns, d, generator=g)                                  # generator outputs: continuous in (0, 1)
    return q, s


_REF = {}


@pytest.mark.parametrize("kind", ["binary", "continuous"])
@pytest.mark.parametrize("nq,ns,d", [(1, 1, 1), (7, 5, 3), (33, 65, 13), (100, 257, 64), (513, 1029, 784),
                                     (2048, 4096, 784)])
@pytest.mark.parametrize("S", [1, 3, 10])
def test_parzen_kernel_against_fp64(nq, ns, d, kind, S):
    q, s = data(nq, ns, d, kind, nq + 7 * ns + d)
    key = (nq, ns, d, kind)
    if key not in _REF:
        _REF.clear()
        _REF[key] = refs(q, s, REF_SIGMAS)
    ll64, ll32 = _REF[key]
    idx = [REF_SIGMAS.index(x) for x in SIGMAS[S]]
    got = metrics.parzen_log_likelihood(s.to(DEV), q.to(DEV), SIGMAS[S])
    assert got.shape == (S, nq)
    check_bound(got, ll64[idx], ll32[idx], "%s %s S=%d" % (key, kind, S))


@pytest.mark.parametrize("kind", ["binary", "continuous"])
def test_parzen_small_sigma_stays_finite(kind):
    q, s = data(300, 700, 784, kind, 11)
    ll64, ll32 = refs(q, s, [0.01])
    got = metrics.parzen_log_likelihood(s.to(DEV), q.to(DEV), [0.01])
    check_bound(got, ll64, ll32, "sigma 0.01 " + kind)


def test_parzen_strided_operands():
    """Row pitch above d on both operands (ld arguments), d not a multiple of the k tile."""
    q, s = data(70, 300, 50, "binary", 5)
    qb, sb = torch.zeros(70, 64), torch.zeros(300, 61)
    qb[:, :50], sb[:, :50] = q, s
    ll64, ll32 = refs(q, s, SIGMAS[3])
    got = metrics.parzen_log_likelihood(sb.to(DEV)[:, :50], qb.to(DEV)[:, :50], SIGMAS[3])
    check_bound(got, ll64, ll32, "strided")


def test_parzen_full_size_against_fp64_on_the_gpu():
    n, d = 10000, 784
    g = torch.Generator().manual_seed(2024)
    q = (torch.rand(n, d, generator=g) < 0.13).float().to(DEV)
    s = torch.rand(n, d, generator=g).to(DEV)
    sig = SIGMAS[10]
    got = metrics.parzen_log_likelihood(s, q, sig)
    sig64 = _sig(sig).to(DEV)
    ll64, ll32 = [], []
    s64, sn32 = s.double(), (s * s).sum(1)
    for i in range(0, n, 1000):
        qc = q[i:i + 1000]
        d2 = torch.cdist(qc.double(), s64, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        ll64.append(ll_from_neg_half_d2(-0.5 * d2, n, d, sig64).cpu())
        a32 = -0.5 * ((qc * qc).sum(1)[:, None] + sn32[None, :]) + qc @ s.t()
        ll32.append(ll_from_neg_half_d2(a32.double(), n, d, sig64).cpu())
    check_bound(got, torch.cat(ll64, 1), torch.cat(ll32, 1), "10k x 10k x 784")


def test_parzen_deterministic_and_independent_of_the_other_queries():
    q, s = data(1000, 3000, 784, "binary", 9)
    q, s = q.to(DEV), s.to(DEV)
    a = metrics.parzen_log_likelihood(s, q, SIGMAS[10])
    b = metrics.parzen_log_likelihood(s, q, SIGMAS[10])
    assert torch.equal(a, b)
    idx = torch.tensor([3, 700, 999] + list(range(100, 165)) + [0], device=DEV)
    sub = metrics.parzen_log_likelihood(s, q[idx].contiguous(), SIGMAS[10])
    assert torch.equal(sub, a[:, idx])
    one = metrics.parzen_log_likelihood(s, q[511:512], SIGMAS[10][4:5])
    assert torch.equal(one[0], a[4, 511:512])


def test_parzen_evaluate_selection_rule():
    q, s = data(400, 900, 784, "binary", 13)
    v = (torch.rand(300, 784, generator=torch.Generator().manual_seed(1)) < 0.13).float()
    r = metrics.parzen_evaluate(s.to(DEV), v.to(DEV), q.to(DEV))
    full = metrics.parzen_log_likelihood(s.to(DEV), v.to(DEV), metrics.default_sigmas()).double().mean(1).cpu()
    assert np.array_equal(r.val_means, full.numpy())
    k = metrics.select_sigma(metrics.default_sigmas(), r.val_means)
    assert r.sigma == metrics.default_sigmas()[k]
    t = metrics.parzen_log_likelihood(s.to(DEV), q.to(DEV), [r.sigma])[0].double().cpu().numpy()
    assert r.ll_mean == pytest.approx(t.mean(), rel=1e-12)
    assert r.ll_stderr == pytest.approx(t.std() / np.sqrt(t.size), rel=1e-9)


# ---- trainers --------------------------------------------------------------------------------------------------

def fwd64(net, z):
    """fp64 CPU forward of a stock two-layer net: relu(first) -> out_act(second)."""
    l1, l2 = getattr(net, net._names[0]), getattr(net, net._names[1])
    h = torch.relu(z @ l1.weight.detach().cpu().double().t() + l1.bias.detach().cpu().double())
    y = h @ l2.weight.detach().cpu().double().t() + l2.bias.detach().cpu().double()
    return torch.sigmoid(y) if net._out_act == "sigmoid" else torch.relu(y) if net._out_act == "relu" else y


def check_samples(got, net, z):
    """got against the fp64 forward, within twice the fp32 CPU forward's error plus one fp32 ulp (close64's bound)."""
    torch.cuda.synchronize()
    ref64 = fwd64(net, z.double())
    l1, l2 = getattr(net, net._names[0]), getattr(net, net._names[1])
    h = torch.relu(z @ l1.weight.detach().cpu().t() + l1.bias.detach().cpu())
    y = h @ l2.weight.detach().cpu().t() + l2.bias.detach().cpu()
    ref32 = torch.sigmoid(y) if net._out_act == "sigmoid" else y
    got = got.detach().cpu().double()
    e_hip = (got - ref64).abs().max().item()
    e_cpu = (ref32.double() - ref64).abs().max().item()
    assert e_hip <= 2.0 * e_cpu + 2.0 ** -23, (e_hip, e_cpu)


def _nsgan(seed=1234):
    import ns_gan
    loaders = ns_gan.get_data(BATCH_SIZE=100, n_train=2000, n_val=1000, n_test=1000)
    torch.manual_seed(seed)
    return ns_gan.NSGANTrainer(ns_gan.NSGAN(image_size=784, hidden_dim=400, z_dim=20), *loaders)


def _train(tr, n=1):
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(num_epochs=n)


def _params(m):
    torch.cuda.synchronize()
    return [p.detach().clone() for p in m.parameters()]


def test_nsgan_parzen_leaves_rng_parameters_and_mode_alone():
    tr = _nsgan()
    _train(tr)
    cpu, gpu, p0, mode = torch.get_rng_state(), torch.cuda.get_rng_state(), _params(tr.model), tr.model.training
    r = tr.parzen(n_samples=2000)
    assert np.isfinite([r.sigma, r.ll_mean, r.ll_stderr]).all() and len(r.val_means) == 10
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), gpu)
    assert all(torch.equal(a, b) for a, b in zip(p0, _params(tr.model)))
    assert tr.model.training == mode


def test_nsgan_sample_matches_fp64_forward_and_parzen_is_repeatable():
    tr = _nsgan()
    _train(tr)
    got = tr.sample(3000, seed=5)
    z = torch.randn(3000, 20, generator=torch.Generator().manual_seed(5))
    check_samples(got, tr.model.G, z)
    a, b = tr.parzen(n_samples=2000, seed=3), tr.parzen(n_samples=2000, seed=3)
    assert (a.sigma, a.ll_mean, a.ll_stderr) == (b.sigma, b.ll_mean, b.ll_stderr)
    assert np.array_equal(a.val_means, b.val_means)


def test_nsgan_parzen_between_epochs_changes_no_training():
    a = _nsgan()                    # each trainer is built right before its run: training draws from the global
    _train(a)                       # generator, which _nsgan() re-seeds
    a.parzen(n_samples=2000)
    _train(a)
    b = _nsgan()
    _train(b)
    _train(b)
    assert a.Glosses == b.Glosses and a.Dlosses == b.Dlosses
    assert all(torch.equal(x, y) for x, y in zip(_params(a.model), _params(b.model)))


def _small_loaders():
    from oracle import port
    return port.synthetic_loaders(16, n_train=64, n_val=48, n_test=48, image_shape=(1, 8, 8))


def test_infogan_samples_follow_the_noise_layout():
    import info_gan
    loaders = _small_loaders()
    torch.manual_seed(5)
    model = info_gan.InfoGAN(image_size=64, hidden_dim=32, z_dim=6, disc_dim=4, cont_dim=3)
    tr = info_gan.InfoGANTrainer(model, *loaders)
    _train(tr)
    got = tr.sample(200, seed=8)
    g = torch.Generator().manual_seed(8)
    z = torch.randn(200, 6, generator=g)
    cat = torch.randint(0, 4, (200,), dtype=torch.long, generator=g)
    noise = torch.cat((z, torch.nn.functional.one_hot(cat, 4).float(), torch.randn(200, 3, generator=g)), dim=1)
    check_samples(got, model.G, noise)
    r = tr.parzen(n_samples=500, n_val=48)
    assert np.isfinite(r.ll_mean)


@pytest.mark.parametrize("which", ["vae", "bir"])
def test_vae_samples_come_through_the_decoder(which):
    import bir_vae
    import vae
    loaders = _small_loaders()
    torch.manual_seed(6)
    if which == "vae":
        model = vae.VAE(image_size=64, hidden_dim=32, z_dim=5)
        tr = vae.VAETrainer(model, *loaders)
    else:
        model = bir_vae.BIRVAE(image_size=64, hidden_dim=32, z_dim=5)
        tr = bir_vae.BIRVAETrainer(model, *loaders)
    _train(tr)
    got = tr.sample(300, seed=2)
    check_samples(got, model.decoder, torch.randn(300, 5, generator=torch.Generator().manual_seed(2)))
    r = tr.parzen(n_samples=400)
    assert np.isfinite(r.ll_mean) and r.sigma in metrics.default_sigmas()
