"""The seeded walks of tests/map_walks.py through the oracle alone: every fixed seed must be a walk worth running on
the GPU (tests/test_map_walks_gpu.py).  A seed that is not fails here; it is not skipped."""
import pytest

from tests import map_walks as W


def test_six_seeds_and_two_of_them_dense():
    assert len(set(W.SEEDS)) == 6 and len(W.DENSE_SEEDS) == 2 and set(W.DENSE_SEEDS) <= set(W.SEEDS)


@pytest.mark.parametrize("seed", W.SEEDS)
def test_walk_is_worth_running(oracle, seed):
    w = W.walk(seed)
    assert w["cap"] in (1, 3, 20) and 28 <= len(w["steps"]) <= 34
    assert len(W.case()["xyz"]) <= 6000
    for step in w["steps"]:
        if step[0] in ("add", "add_nowait"):
            assert 500 <= len(step[1]) <= 3000
    assert sum(1 for s in w["steps"] if s[0] == "clear") <= 1
    assert any(s[0] == "align_cleanup" and s[2] is None for s in w["steps"])
    assert any(s[0] == "align_cleanup" and s[2] is not None for s in w["steps"])
    s = W.survey(w, oracle)
    print(seed, w["cap"], s)
    assert len(s["erasing"]) >= 3, "at least three cleanups erase voxels"
    assert any(f < 0.25 for f in s["erasing"]), "one erases fewer than a quarter of the voxels it meets"
    assert any(f > 0.25 for f in s["erasing"]), "one erases more than a quarter"
    assert s["small_then_big"], "empty slabs pile up and are closed later"
    assert s["recreated"] >= 1, "a later insert re-creates erased voxels"
    assert s["cap_lowered"] >= 1, "the cap is lowered below what some voxel holds"
    assert s["final_size"] > 0


def test_walks_are_a_function_of_the_seed():
    a, b = W.walk(W.SEEDS[0]), W.walk(W.SEEDS[0])
    assert a["cap"] == b["cap"] and len(a["steps"]) == len(b["steps"])
    for x, y in zip(a["steps"], b["steps"]):
        assert x[0] == y[0] and all((p == q).all() if hasattr(p, "all") else p == q for p, q in zip(x[1:], y[1:]))
