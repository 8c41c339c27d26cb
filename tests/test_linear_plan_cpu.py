"""Which kernel every case of tests/linear_path_cases.py reaches, pinned against the library's own dispatch
(gm_linear_plan: the launch plan that decide<MODE> makes of the call, read instead of issued -- no GPU, no HIP call).
Two things are asserted:
every case resolves to the plan written next to it, and the plans of the table are EXACTLY the plans a plain launch can
reach -- listed here family by family, and checked against a sweep of the query over shapes, alignments and ring slots.
A retuned threshold moves cases onto other plans and fails the first test by name; a new instantiation the dispatch can
reach fails the second until a case reaches it."""
import itertools
import os

import pytest

from generative_models_amd import _lib, ops

import linear_path_cases as lp

pytestmark = pytest.mark.skipif(not os.path.isfile(_lib.LIB_PATH), reason="libgm_hip.so not built")


def resolve(c):
    mode, d = lp.descriptor(c, lp.placeholder_pointers(c))
    p = ops.linear_plan(mode, d)
    assert p["launches"] == 1 and p["block"] == {"lds": 512, "k32": 256, "split": 1024}[p["family"]], (c.id, p)
    return lp.plan_key(p)


def test_every_case_reaches_the_plan_written_next_to_it():
    moved = ["%s: meant for [%s], the dispatch takes [%s]" % (c.id, c.plan, got)
             for c, got in ((c, resolve(c)) for c in lp.CASES) if got != c.plan]
    assert not moved, "%d case(s) moved to another launch plan:\n%s" % (len(moved), "\n".join(moved))


B = (0, 1)
# Every plan a plain (rider-free) launch can reach: family x tile x vec, xv, vec_epi x dma x loop instantiation x slot.
REACHABLE = set(
    # forward, split reduction: five tiles; 16-byte X / W rows or not; either epilogue; with and without a ring slot
    [lp.split("fwd", t, v, 0, e, 0, s) for t in ("32x32", "16x32", "32x64", "64x32", "48x32") for v in B for e in B for s in B] +
    # forward over K <= 32 (16-byte rows only)
    [lp.k32(e, s) for e in B for s in B] +
    # LDS macro tiles, forward and input gradient: 64x64 / 32x64; runtime loop, 13 and 25 unrolled stages
    [lp.lds(m, cfg, ns, e) for m in ("fwd", "dx") for cfg in (1, 2) for ns in (0, 13, 25) for e in B] +
    # input gradient, split reduction: four tiles, dA (vec) and W (xv) each on either path
    [lp.split("dx", t, v, x, e) for t in ("32x32", "16x32", "32x64", "64x32") for v in B for x in B for e in B] +
    # weight gradient: six tiles, operands by 16-byte loads or scalar; LDS-DMA on the two 48-wide tiles
    [lp.split("dw", t, 0, x, e, 0, s) for t in ("32x32", "16x32", "32x64", "64x32", "32x48", "48x32")
     for x in B for e in B for s in B] +
    [lp.split("dw", t, 0, 1, e, 1, s) for t in ("32x48", "48x32") for e in B for s in B])

# Instantiations the library compiles (on_tile expands every tile for every mode) that NO plain call reaches, and
# why; the sweep below backs each line -- none of these plans may ever come out of the query.
UNREACHABLE = {
    "fwd split 32x48": "pick_tile turns 32x64 into 32x48 for weight gradients only",
    "dx split 32x48": "pick_tile turns 32x64 into 32x48 for weight gradients only",
    "dx split 48x32": "pick_tile turns 64x32 into 48x32 for forwards and weight gradients only",
}


def test_the_table_covers_exactly_the_reachable_plans():
    table = {c.plan for c in lp.CASES}
    assert len(REACHABLE) == 156
    missing, stray = sorted(REACHABLE - table), sorted(table - REACHABLE)
    assert not missing, "reachable launch plans without a case:\n" + "\n".join(missing)
    assert not stray, "cases on plans that are not listed as reachable:\n" + "\n".join(stray)


def _sweep_cases():
    """Shapes on a coarse grid up to 2100 (every threshold of the dispatch from both sides), each with the operands on
    and off the 16-byte paths, the output on and off the float4 epilogue, with and without a ring slot."""
    grid = (1, 4, 16, 17, 32, 33, 36, 64, 68, 100, 400, 416, 497, 500, 767, 768, 784, 800, 1023, 1024, 1025, 1300, 2100)
    for M, K, N in itertools.product(grid, repeat=3):
        if 2.0 * M * K * N > 4e9:            # (nothing in the dispatch looks at a product of all three)
            continue
        for opnd, outp, s in itertools.product(B, B, B):
            yield lp.Case("", "fwd", M, K, N, ("X", "W") * opnd + ("Y",) * outp, {}, dict(slot=s), None)
            yield lp.Case("", "dw", M, K, N, ("dA", "X") * opnd + ("dW",) * outp, {}, dict(slot=s), None)
            yield lp.Case("", "dx", M, K, N, ("dA",) * opnd + ("W",) * s + ("dX",) * outp, {}, {}, None)


def test_a_sweep_of_the_query_finds_no_plan_outside_the_list():
    seen = {}
    for c in _sweep_cases():
        seen.setdefault(resolve(c), (c.op, c.M, c.K, c.N, c.off, c.flags))
    new = {k: v for k, v in seen.items() if k not in REACHABLE}
    assert not new, "the dispatch reaches plans that tests/linear_path_cases.py does not list:\n" + \
        "\n".join("%s at %r" % kv for kv in sorted(new.items()))
    for prefix, why in UNREACHABLE.items():
        assert not [k for k in seen if k.startswith(prefix)], (prefix, why)
    # ... and the sweep itself finds most of the list (the rest needs the leading dimensions / K % 4 of the table)
    assert len(seen) >= 100, len(seen)


def test_riders_and_refusals_answer_without_a_plan():
    c = lp.CASES[0]
    mode, d = lp.descriptor(c, lp.placeholder_pointers(c))
    d.hd_w2 = 4096
    with pytest.raises(_lib.GMError, match="plain launches only"):
        ops.linear_plan(mode, d)
    mode, d = lp.descriptor(c, lp.placeholder_pointers(c))
    d.ldx = c.K - 1
    with pytest.raises(_lib.GMError, match="bad argument"):
        ops.linear_plan(mode, d)
    # the query leaves the launch path as it was: the next real call on this thread still reaches the argument checks
    assert _lib.load().gm_linear_fwd_ex(None, None) == _lib.GM_EINVAL
