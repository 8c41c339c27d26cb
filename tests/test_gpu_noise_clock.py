"""The step clock (csrc/gm_philox.h PhClock: step = *step_ctr + *step_base + step_add, taken mod 2^32) through the entry
points that no other test drives with the device words: gm_flow_sample, gm_cat_sample's NOISE mode, gm_cat_reduce,
gm_nvp_pre's NOISE mode and gm_rbm_uniform.  For each, at one seed: step 77 given as a number and as 3 + [70] + [4]
on the device give the same bits, so does 77 + 2^32, and step 76 does not (an ignored clock would pass the first two).
The DVAE, IWAE, DDPM, RealNVP-step and RBM-chain clocks have such tests beside their kernels' tests.

Shapes: 3 images of k = 2 samples, Z = 5, 2 flow layers, N = 3 variables of C = 5 classes, 7 uniforms per row and the
smallest RealNVP row that is not a multiple of 4 -- each reaches a partial quad and a second row."""
import ctypes

import pytest
import torch

from generative_models_amd import _lib
from generative_models_amd import ops_fused as of_
from generative_models_amd._lib import GMError

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 0x5EED0123456789AB
B, K_S, Z, K_F, N, C, W_U = 3, 2, 5, 2, 3, 5, 7
D_NVP = next(d for d in range(_lib.NVP_MIN_D, _lib.NVP_MIN_D + 4) if d % 4)


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _flow_sample(**clock):
    ml, b = _rand(B, 2 * Z, seed=1), 0.3 * _rand(K_F, seed=4)
    u, w = 0.3 * _rand(K_F, Z, seed=2), 0.3 * _rand(K_F, Z, seed=3)
    z, lp = torch.zeros(B * K_S, Z, device=DEV), torch.zeros(B * K_S, device=DEV)
    noise = of_.iwae_noise(SEED, _lib.IWAE_TAG_TRAIN, K_S, **clock)
    of_.flow_sample(ml, z, lp, noise, of_.flow_params(u, w, b), B, K_S, Z)
    return torch.cat([z.flatten(), lp])


def _cat_noise(**clock):
    y = torch.zeros(B * K_S, N * C, device=DEV)
    of_.cat_sample(None, y, None, of_.iwae_noise(SEED, _lib.CAT_TAG_TRAIN, K_S, **clock), B, K_S, N, C, _lib.CAT_NOISE)
    return y


def _cat_reduce(**clock):
    logits, dz, wn = _rand(B, N * C, seed=5), _rand(B, N * C, seed=6), _rand(B, seed=7).abs()
    dl = torch.zeros(B, N * C, device=DEV)
    of_.cat_reduce(logits, dz, wn, dl, of_.iwae_noise(SEED, _lib.CAT_TAG_TRAIN, 1, **clock), B, N, C, tau=0.7)
    return dl


def _nvp_noise(step=0, step_ctr=None, step_base=None):
    u = torch.zeros(B, D_NVP, device=DEV)
    a = of_.NvpPreArgs()
    a.u, a.ldu, a.mode, a.B, a.D = u.data_ptr(), u.stride(0), _lib.NVP_NOISE, B, D_NVP
    of_._nvp_noise(a, SEED, _lib.NVP_TAG_TRAIN, step, step_ctr, step_base, 0)
    _lib.call("gm_nvp_pre", of_.stream_ptr(), ctypes.byref(a))
    return u


def _rbm_uniform(**clock):
    return of_.rbm_uniform(B, W_U, SEED, _lib.RBM_TAG_H, **clock)


ENTRIES = {"flow_sample": _flow_sample, "cat_sample_noise": _cat_noise, "cat_reduce": _cat_reduce,
           "nvp_pre_noise": _nvp_noise, "rbm_uniform": _rbm_uniform}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_step_is_ctr_plus_base_plus_add_mod_2_32(name):
    run = ENTRIES[name]
    ctr = torch.tensor([70], dtype=torch.int64, device=DEV)
    base = torch.tensor([4], dtype=torch.int64, device=DEV)
    at77 = run(step=77)
    split = run(step=3, step_ctr=ctr, step_base=base)
    wrapped = run(step=77 + 2 ** 32)
    at76 = run(step=76)
    torch.cuda.synchronize()
    assert torch.isfinite(at77).all()
    assert torch.equal(at77, split)
    assert torch.equal(at77, wrapped)
    assert not torch.equal(at77, at76)


def test_int32_device_tensor_is_refused():
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    for name in sorted(ENTRIES):
        for which in ("step_ctr", "step_base"):
            with pytest.raises(GMError, match=which):
                ENTRIES[name](**{which: bad})
