"""Parzen-window evaluation, the parts that need no GPU: gm_parzen_ll rejects bad arguments before any launch, the
workspace size follows the formula in include/gm_hip.h, sigma selection, and the trainers that cannot be scored."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

from generative_models_amd import _lib, metrics, trainers  # noqa: E402

FAKE = 1 << 20          # a non-null, 8-byte aligned "device pointer": every call below must fail before using it


def _ws(nq, ns, k):
    return 8 * k * nq * -(-ns // 128) + 4 * (nq + ns)


def test_workspace_bytes_formula_and_monotone():
    lib = _lib.load()
    prev = {}
    for nq in (1, 2, 7, 255, 256, 257, 10000):
        for ns in (1, 127, 128, 129, 255, 256, 257, 10000):
            for k in (1, 3, 10, 16):
                n = lib.gm_parzen_workspace_bytes(nq, ns, k)
                assert n == _ws(nq, ns, k) == metrics.workspace_bytes(nq, ns, k), (nq, ns, k, n)
                for key, p in ((("ns", nq, k), ns), (("nq", ns, k), nq), (("k", nq, ns), k)):
                    if key in prev:
                        assert n >= prev[key][1], (key, p, n, prev[key])
                    prev[key] = (p, n)


@pytest.mark.parametrize("nq,ns,k", [(0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 17), (-1, 5, 1)])
def test_workspace_bytes_rejects_bad_sizes(nq, ns, k):
    lib = _lib.load()
    assert lib.gm_parzen_workspace_bytes(nq, ns, k) == _lib.GM_EINVAL
    assert b"bad argument" in lib.gm_last_error()
    with pytest.raises(_lib.GMError):
        metrics.workspace_bytes(nq, ns, k)


def _good(nq=10, ns=20, d=8, k=3):
    return dict(stream=None, q=FAKE, ldq=d, nq=nq, s=FAKE, lds=d, ns=ns, d=d, sig=FAKE, k=k, ws=FAKE,
                ws_bytes=_ws(nq, ns, k), out=FAKE, ldo=nq)


BAD = [("nq", 0), ("ns", 0), ("d", 0), ("k", 0), ("k", 17), ("ldq", 7), ("lds", 7), ("ldo", 9),
       ("ws_bytes", _ws(10, 20, 3) - 1), ("ws_bytes", 0), ("q", None), ("s", None), ("sig", None), ("ws", None),
       ("out", None), ("ws", FAKE + 4)]


@pytest.mark.parametrize("field,value", BAD)
def test_parzen_ll_rejects_bad_arguments_without_a_gpu(field, value):
    a = _good()
    a[field] = value
    lib = _lib.load()
    rc = lib.gm_parzen_ll(a["stream"], a["q"], a["ldq"], a["nq"], a["s"], a["lds"], a["ns"], a["d"], a["sig"], a["k"],
                          a["ws"], a["ws_bytes"], a["out"], a["ldo"])
    assert rc == _lib.GM_EINVAL, (field, value, rc)
    assert b"bad argument" in lib.gm_last_error()


def test_select_sigma_argmax_and_ties_to_the_smaller_sigma():
    sig = np.logspace(-1, 0, 10)
    assert metrics.select_sigma(sig, [-5, -4, -3, -2, -1.5, -2, -3, -4, -5, -6]) == 4
    assert metrics.select_sigma(sig, [-1.0] * 10) == 0
    assert metrics.select_sigma(sig, [-3, -1, -2, -1, -5, -6, -7, -8, -9, -10]) == 1
    # the tie rule is about sigma, not position
    assert metrics.select_sigma([0.5, 0.2, 0.3], [7.0, 7.0, 1.0]) == 1
    with pytest.raises(trainers.GMError):
        metrics.select_sigma([0.1, 0.2], [float("nan"), 1.0])


def test_default_sigma_grid():
    assert np.array_equal(metrics.default_sigmas(), np.logspace(-1, 0, 10))


def test_parzen_needs_device_tensors():
    x = torch.rand(4, 6)
    with pytest.raises(trainers.GMError, match="no CPU fallback"):
        metrics.parzen_log_likelihood(x, x, [0.2])


def test_autoencoder_trainer_parzen_raises():
    import ae
    mk = lambda n: torch.utils.data.DataLoader(
        torch.utils.data.TensorDataset(torch.rand(n, 1, 4, 4), torch.zeros(n, dtype=torch.int64)), batch_size=4)
    torch.manual_seed(0)
    tr = ae.AutoencoderTrainer(ae.Autoencoder(image_size=16, hidden_dim=3), mk(8), mk(8), mk(8))
    with pytest.raises(trainers.GMError, match="no prior"):
        tr.parzen()
    with pytest.raises(trainers.GMError, match="no prior"):
        tr.sample(4)
