"""The noise builders' shared clock and seed checks (ops_fused._clock / _seed64), without a GPU:
what the blocks hold when no tensor is given, the seed's range, and that a step tensor which is not an int64 device
tensor is refused before anything reaches the library -- the kernels would read it as raw memory."""
import pytest
import torch

from generative_models_amd import _lib
from generative_models_amd import ops_fused as of_
from generative_models_amd._lib import GMError

SEED = 0x0123456789ABCDEF
BUILDERS = {
    "corrupt_args": lambda seed=SEED, **kw: of_.corrupt_args("gaussian", 0.25, seed, row0=11, **kw),
    "iwae_noise": lambda seed=SEED, **kw: of_.iwae_noise(seed, _lib.IWAE_TAG_TRAIN, 9, j0=2, q0=5, **kw),
    "ddpm_noise": lambda seed=SEED, **kw: of_.ddpm_noise(seed, True, row0=11, **kw),
}


def _nvp_block(seed=SEED, step=0, step_ctr=None, step_base=None):
    a = of_.NvpPreArgs()
    of_._nvp_noise(a, seed, _lib.NVP_TAG_TRAIN, step, step_ctr, step_base, 11)
    return a


def _rbm_chain(step_ctr=None, step_base=None):
    W = torch.zeros(3, 5)
    of_.rbm_chain(W, W.t().contiguous(), torch.zeros(3), torch.zeros(5), torch.zeros(2, 5), 1, SEED,
                  step_ctr=step_ctr, step_base=step_base)


def _rbm_uniform(step_ctr=None, step_base=None):
    of_.rbm_uniform(2, 7, SEED, _lib.RBM_TAG_H, step=3, step_ctr=step_ctr, step_base=step_base)


CLOCKED = dict(BUILDERS, nvp_pre=lambda **kw: _nvp_block(**kw), rbm_chain=_rbm_chain, rbm_uniform=_rbm_uniform)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_block_without_tensors_holds_the_arguments(name):
    a = BUILDERS[name](step=77)
    assert (a.seed, a.step_add, a.step_ctr, a.step_base) == (SEED, 77, None, None)
    if name == "iwae_noise":
        assert (a.tag, a.k_total, a.j0, a.q0) == (_lib.IWAE_TAG_TRAIN, 9, 2, 5)
    else:
        assert a.row0 == 11
    if name == "ddpm_noise":
        assert (a.tag_t, a.tag_e) == (_lib.DDPM_TAG_T, _lib.DDPM_TAG_E)


def test_nvp_block_without_tensors_holds_the_arguments():
    a = _nvp_block(step=77)
    assert (a.seed, a.tag, a.step_add, a.row0) == (SEED, _lib.NVP_TAG_TRAIN, 77, 11)
    assert (a.step_ctr, a.step_base) == (None, None)


@pytest.mark.parametrize("name", sorted(BUILDERS) + ["nvp_pre"])
def test_seed_range(name):
    build = CLOCKED[name]
    assert build(seed=2 ** 64 - 1).seed == 2 ** 64 - 1
    for bad in (-1, 2 ** 64):
        with pytest.raises(GMError, match="seed"):
            build(seed=bad)


@pytest.mark.parametrize("which", ["step_ctr", "step_base"])
@pytest.mark.parametrize("bad", ["cpu_int64", "int32", "not_a_tensor"])
@pytest.mark.parametrize("name", sorted(CLOCKED))
def test_wrong_step_tensor_is_refused_before_the_library(name, bad, which):
    t = {"cpu_int64": torch.zeros(1, dtype=torch.int64), "int32": torch.zeros(1, dtype=torch.int32),
         "not_a_tensor": 5}[bad]
    with pytest.raises(GMError, match=which):
        CLOCKED[name](**{which: t})
