"""The order of work of the eight one-network engines (MADE, MAF, RealNVP, DDPM, RBM, GMMN, flow matching, SWG): the
entry points one train(1) calls through _lib.call, eager and under graphs, against sequences recorded before the engines
were given a shared base.  10 training and 6 validation rows at batch 4: two full training batches and a ragged one of
2 rows, then a full validation batch and a ragged one.  Under graphs the same launches are issued once per captured
graph and replayed, so the two modes pin both what a batch launches and which graphs an epoch captures."""
import contextlib
import io
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from generative_models_amd import _lib, ddpm, flowmatch, gmmn, made, maf, realnvp, rbm, swg  # noqa: E402

I, H = 16, 8
CASES = {
    "MADE": (made.MADETrainer, lambda: made.MADE(I, H), {}),
    "MAF": (maf.MAFTrainer, lambda: maf.MAF(I, H, 2), {}),
    "RealNVP": (realnvp.RealNVPTrainer, lambda: realnvp.RealNVP(I, H, 2), {}),
    "DDPM": (ddpm.DDPMTrainer, lambda: ddpm.DDPM(I, H, 4, 10), {}),
    "RBM": (rbm.RBMTrainer, lambda: rbm.RBM(I, H), {}),
    "GMMN": (gmmn.GMMNTrainer, lambda: gmmn.GMMN(I, H, 2), {}),
    "FlowMatch": (flowmatch.FlowMatchTrainer, lambda: flowmatch.FlowMatching(I, H, 4, 10), {}),
    "SWG": (swg.SWGTrainer, lambda: swg.SWG(I, H, 2), {"num_projections": 5}),
}


def _loaders():
    g = torch.Generator().manual_seed(7)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True)
    return mk(10), mk(6), mk(6)


def _train_once(name, use_graph):
    cls, model, kw = CASES[name]
    torch.manual_seed(1234)
    tr = cls(model(), *_loaders(), **kw)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    return tr


def record(name, use_graph):
    """The entry-point names of one train(1) of a fresh trainer, after another fresh trainer of the same kind has
    trained once so that whatever the process does a single time (self-checks, workspaces) is behind it."""
    _train_once(name, use_graph)
    names, orig = [], _lib.call

    def call(entry, *args):
        names.append(entry)
        return orig(entry, *args)
    _lib.call = call
    try:
        tr = _train_once(name, use_graph)
    finally:
        _lib.call = orig
    assert type(tr._engine).__name__ == name + "Engine" and len(tr.losses) == 3
    return names


# ---- the recorded sequences ------------------------------------------------------------------------------------------
# Per engine: what configure() calls before the first batch, one training batch and one validation batch of an eager
# run, name by name as recorded.  A training batch follows the launch list of the engine's docstring; where a call
# issues two kernels the list is one name shorter than the docstring's count: the paired weight gradients
# (ops.linear_bwd_dw_adam_pair) are ONE gm_linear_bwd_dw_ex, and gm_mmd_pairs is the row-norm launch and the tile launch.
_F, _DX, _DW, _SUM = "gm_linear_fwd", "gm_linear_bwd_dx", "gm_linear_bwd_dw_ex", "gm_sum_finalize"
_G = "gm_gather_rows_bits"
RECORDED = {
    # 8 launches: gather, two forwards, the loss, dH, the pair, the masks, the sum
    "MADE": (["gm_made_mask"],
             [_G, _F, _F, "gm_made_bce", _DX, _DW, "gm_made_mask", _SUM],
             [_G, _F, _F, "gm_made_bce", _SUM]),
    # gather, pre, 2 x (two forwards, couple), loss, then layer 1 (couple_bwd, dH, the input's cotangent, pair, mask)
    # and layer 0 (couple_bwd, dH, pair, mask), the sum
    "MAF": (["gm_maf_mask", "gm_maf_mask"],
            [_G, "gm_nvp_pre", _F, _F, "gm_maf_couple", _F, _F, "gm_maf_couple", "gm_nvp_loss",
             "gm_maf_couple_bwd", _DX, "gm_linear_bwd_dx_ex", _DW, "gm_maf_mask",
             "gm_maf_couple_bwd", _DX, _DW, "gm_maf_mask", _SUM],
            [_G, "gm_nvp_pre", _F, _F, "gm_maf_couple", _F, _F, "gm_maf_couple", "gm_nvp_loss", _SUM]),
    "RealNVP": ([],
                [_G, "gm_nvp_pre", _F, _F, "gm_nvp_couple", _F, _F, "gm_nvp_couple", "gm_nvp_loss",
                 "gm_nvp_couple_bwd", _DX, "gm_linear_bwd_dx_ex", _DW, "gm_nvp_couple_bwd", _DX, _DW, _SUM],
                [_G, "gm_nvp_pre", _F, _F, "gm_nvp_couple", _F, _F, "gm_nvp_couple", "gm_nvp_loss", _SUM]),
    # 10 launches: gather + q-sample, three forwards, the loss, two dX, the pair, the first layer's dW, the sum
    "DDPM": ([],
             [_G + "_qsample", _F, _F, _F, "gm_ddpm_loss", _DX, _DX, _DW, _DW, _SUM],
             [_G + "_qsample", _F, _F, _F, "gm_ddpm_loss", _SUM]),
    # 8 launches (CD-k): gather, chain, the stacked forward, grad, dW + Adam, vbias, transpose, the sum
    "RBM": (["gm_rbm_transpose"],
            [_G, "gm_rbm_chain", _F, "gm_rbm_grad", _DW, "gm_rbm_vbias", "gm_rbm_transpose", _SUM],
            [_G, "gm_rbm_chain", "gm_made_bce", _SUM]),
    # 12 launches in 11 calls: gather, prior, two forwards, gm_mmd_pairs (2 kernels), finalize, C (R - mu), grad, dH,
    # the pair, the record
    "GMMN": ([],
             [_G, "gm_gmmn_prior", _F, _F, "gm_mmd_pairs", "gm_mmd_finalize", _DX, "gm_mmd_grad", _DX, _DW, _SUM],
             [_G, "gm_gmmn_prior", _F, _F, "gm_mmd_pairs", "gm_mmd_finalize", _SUM]),
    # the DDPM's 10 with the path sample in front
    "FlowMatch": ([],
                  [_G + "_fm_qsample", _F, _F, _F, "gm_ddpm_loss", _DX, _DX, _DW, _DW, _SUM],
                  [_G + "_fm_qsample", _F, _F, _F, "gm_ddpm_loss", _SUM]),
    # 13 launches: gather, prior, two forwards, directions, the projections, sort, finalize, dX, the sigmoid's
    # backward, dH, the pair, the record
    "SWG": ([],
            [_G, "gm_gmmn_prior", _F, _F, "gm_sw_directions", _F, "gm_sw_sort", "gm_sw_finalize", "gm_linear_bwd_dw",
             "gm_act_bwd", _DX, _DW, _SUM],
            [_G, "gm_gmmn_prior", _F, _F, "gm_sw_directions", _F, "gm_sw_sort", "gm_sw_finalize", _SUM]),
}
LADDER = (1, 2, 4, 8, 16, 32)                    # batches per captured graph: every power of two up to graph_iters


def expected(name, use_graph):
    """The whole train(1) as recorded.  Eager: configure, three training batches, two validation batches.  Under
    graphs a batch's last call carries the counter tick; a pass captures, at its first full batch, the graphs of 1 to
    32 batches of that size and launches the one that covers its full batches (two when training, one when
    validating), then captures and launches the ragged batch's own graph."""
    pre, train, val = RECORDED[name]
    if not use_graph:
        return pre + 3 * train + 2 * val
    out = list(pre)
    for seg in (train, val):
        seg = seg[:-1] + [_SUM + "_tick"]
        for k in LADDER:
            out += ["gm_graph_begin"] + k * seg + ["gm_graph_end"]
        out += ["gm_graph_launch", "gm_graph_begin"] + seg + ["gm_graph_end", "gm_graph_launch"]
    return out


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_train_issues_the_recorded_launches_in_order(name, use_graph):
    got, want = record(name, use_graph), expected(name, use_graph)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, "%d calls against %d recorded; first difference at call %d: %s" % (
        len(got), len(want), first, (got[first:first + 3], want[first:first + 3]))
