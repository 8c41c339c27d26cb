"""The bookkeeping of tests/kernel_path_cases.py: the non-GEMM kernels have no plan query, so a case only CLAIMS the arm
it reaches.  Held here against the predicates the table quotes: every clause of every predicate has a case that fails
that clause alone, every predicate has a case that satisfies all of them, a case's claim is what its own shape and
placement imply, ids are unique and the counts are the ones the module's docstring states.  Also the assertions on the
INPUTS that the GPU test relies on (no undefined ReLU mask, row norms away from k)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kernel_path_cases as kp  # noqa: E402


def test_ids_are_unique_and_counts_match_the_docstring():
    assert len({c.id for c in kp.CASES}) == len(kp.CASES)
    counts = {k: len(kp.cases(k)) for k in kp.KERNELS}
    assert counts == kp.docstring_counts(), counts


@pytest.mark.parametrize("kernel", list(kp.PREDICATES))
def test_every_clause_fails_alone_in_some_case_and_one_case_satisfies_all(kernel):
    alone = {}
    for c in kp.cases(kernel):
        f = kp.failed(c)
        # the claim is what the placement implies: one clause, the named one -- or none on the vector arm
        assert f == ([c.clause] if c.clause else []), (c.id, f, c.clause)
        assert c.arm == ("elem" if f else "vec"), (c.id, c.arm, f)
        if f:
            alone.setdefault(f[0], []).append(c.id)
    missing = [cl for cl in kp.clauses(kernel) if cl not in alone]
    assert not missing, "%s: no case fails %s alone" % (kernel, missing)
    assert any(c.arm == "vec" for c in kp.cases(kernel)), kernel


def test_cases_without_a_predicate_claim_no_arm():
    for c in kp.CASES:
        if c.kernel not in kp.PREDICATES:
            assert c.arm == "loop" and c.clause is None, c.id
        assert set(c.off) | set(c.ld) | set(c.absent) <= _arrays(c.kernel), c.id


def _arrays(kernel):
    known = {"gp_dw2": "s h t gw2", "dragan_head_bwd": "H T da2 w2 gw2 gb2 dA1", "adam": "p g m v", "gp_u": "s h w2 u",
             "bir_reparam": "mu eps z", "pdw_couple": "x xr t n share dA xhat xcopy", "bir_mmd": "z prior dz partial"}
    if kernel in kp.LD_KERNELS:
        return set(kp.LD_KERNELS[kernel][1])
    names = set(known.get(kernel, "").split())
    if kernel in kp.PREDICATES:
        names |= {n for n, _ in kp.PREDICATES[kernel]["arrays"]}
    return names


def test_the_shapes_the_issue_names_are_all_there():
    have = lambda k: {(c.B, c.W) for c in kp.cases(k)}
    for k in ("gp_norm", "pdw_dir", "pdw_couple"):
        assert {(B, W) for B in (1, 5) for W in kp.ROW_WIDTHS} <= have(k), k
    assert {(B, W) for B in (1, 5) for W in kp.HEAD_WIDTHS} <= have("head_gp")
    assert {(B, 33) for B in kp.DW2_B} | {(129, H) for H in kp.DW2_H} <= have("gp_dw2")
    assert {(B, 17) for B in kp.HB_B} | {(65, H) for H in kp.HB_H} <= have("dragan_head_bwd")
    for scaled in (False, True):
        ns = {c.W for c in kp.cases("adam") if c.flags["scaled"] == scaled and not c.flags.get("refused")}
        assert ns == set(kp.ADAM_SMALL + kp.ADAM_LARGE)
        assert {c.off for c in kp.cases("adam") if c.flags["scaled"] == scaled and c.flags.get("refused")} == \
            {("p",), ("g",), ("m",), ("v",)}
    assert min(kp.ADAM_LARGE) > 4 * 256 * 1024                       # the float4 loop's second trip
    for form in ("plain", "tick", "fin2"):
        assert {c.W for c in kp.cases("sum_finalize") if c.flags["form"] == form} == set(kp.SUM_N)
    assert have("gp_u") == {(1030, 512), (1, 1)} and 1030 * 512 > 2048 * 256
    assert have("bir_reparam") == {(1100, 60)} and 1100 * 60 > 256 * 256
    assert {c.W for c in kp.cases("act_bwd")} == {2048 * 256 + 5} and {c.W for c in kp.cases("copy_slot")} == {1024 * 256 + 5}
    # pdw_couple: every optional array absent in turn, t through a ring slot
    assert {c.absent for c in kp.cases("pdw_couple")} >= {("n",), ("dA",), ("xhat", "t"), ("xcopy",)}
    assert any(c.flags.get("ring") for c in kp.cases("pdw_couple"))
    assert {c.flags["k"] for c in kp.cases("gp_norm")} == {1.0, 0.75}


def test_head_gp_inputs_leave_no_row_within_rounding_of_the_relu_kink():
    """A row whose fp64 pre-activation is within rounding of 0 has no defined mask: an assertion on the inputs."""
    for B, W in sorted({(c.B, c.W) for c in kp.cases("head_gp")}):
        a2 = kp.ref_head_gp(kp.row_inputs("head_gp", B, W), torch.float64)["a2"]
        assert a2.abs().min().item() > 1e-3, (B, W, a2)
        if B == 5 and W >= 37:                                       # rows the output ReLU kills and rows it does not
            assert bool((a2 < 0).any()) and bool((a2 > 0).any()), (B, W, a2)
        h = kp.row_inputs("head_gp", B, W)["h"]
        assert W < 37 or bool((h == 0).any())


def test_row_norms_sit_where_the_issue_wants_them():
    for B, W in sorted({(c.B, c.W) for c in kp.cases("gp_norm")}):
        n = kp.row_inputs("gp_norm", B, W)["g"].double().norm(2, dim=1)
        assert torch.allclose(n, torch.tensor(kp.NORMS[:B], dtype=torch.float64), rtol=1e-6)
        assert B == 1 or n[1].item() == 0.0                          # the all-zero row
    for k in ("pdw_dir", "pdw_couple"):
        for B, W in sorted({(c.B, c.W) for c in kp.cases(k)}):
            t = kp.row_inputs(k, B, W)
            assert B == 1 or (torch.equal(t["x"][1], t["xr"][1]) and t["n"][1].item() == 0.0)


def test_column_inputs_carry_both_signs_and_exact_zeros():
    for k, names in (("gp_dw2", ("s", "h")), ("dragan_head_bwd", ("da2", "H"))):
        t = kp.column_inputs(k, 129 if k == "gp_dw2" else 65, 33)
        for n in names:
            assert bool((t[n] > 0).any()) and bool((t[n] < 0).any()) and bool((t[n] == 0).any()), (k, n)
        assert bool((t["gw2"] != 0).all())                           # the accumulating forms start from non-zero sums
