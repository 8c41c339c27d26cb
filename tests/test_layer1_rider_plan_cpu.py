"""Launch plan of the generator's first layer (CPU): where it rides (GANEngine._l1_rides), a graph -- or an eager run --
of k iterations issues the standalone first-layer launch (and its batch gather) once, at its first iteration; every
later iteration starts from what the previous one's launches formed, in the other HG buffer; the last forms nothing
ahead.  Where it does not ride, every iteration keeps today's plan."""
from types import SimpleNamespace

import pytest

from generative_models_amd.engine import GANEngine


def _plan(k, rides):
    seen = []
    eng = SimpleNamespace(_l1_rides=lambda: rides, _HG_pp=["HG0", "HG1"], Bl=2, HG=None)
    eng._use_hg = lambda b: GANEngine._use_hg(eng, b)
    eng._segments = lambda: [(lambda st, it: seen.append((eng._l1_in, eng._l1_out, eng.HG,
                                                          getattr(eng, "_l1_next", None) if eng._l1_out else None)),
                              None)]
    eng._allreduce = lambda *a: None
    for i in range(k):
        GANEngine._issue_iteration(eng, None, 0, i, k)
        assert not eng._l1_in and not eng._l1_out            # reset behind every iteration
    return seen


@pytest.mark.parametrize("k", [1, 2, 3, 128])
def test_first_layer_launch_once_per_graph_where_it_rides(k):
    seen = _plan(k, True)
    standalone = [i for i, (lin, _, _, _) in enumerate(seen) if not lin]
    assert standalone == [0]                                  # one k32 launch per graph, none inside it
    assert [out for _, out, _, _ in seen] == [True] * (k - 1) + [False]
    for i, (_, out, hg, nxt) in enumerate(seen):
        assert hg == "HG%d" % (i & 1)                         # HG by parity from the graph's start
        if out:
            assert nxt == (i + 1) & 1                         # ... and the next iteration's into the other one


@pytest.mark.parametrize("k", [1, 4])
def test_todays_plan_where_it_does_not_ride(k):
    assert _plan(k, False) == [(False, False, None, None)] * k
