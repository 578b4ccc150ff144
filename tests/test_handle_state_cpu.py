"""What tests/test_gpu_handle_state.py rests on, shown with the CPU oracle alone: every poison instance of the scripted life does produce
non-finite values (so the handle's workspaces hold NaN / inf afterwards), every other instance of the script is finite in all outputs (so a
non-finite word in a later result is the handle's past, not the problem), and the sentinel the caller-owned buffers are prefilled with occurs
in no expected output (so "no payload word still holds the sentinel" can be asserted)."""
import numpy as np
import pytest

import handle_state_cases as hs


@pytest.mark.parametrize("mlp,math", hs.ARITH)
def test_poison_instances_diverge_and_all_others_stay_finite(mlp, math):
    ref = hs.life_reference(mlp, math, full=(mlp, math) == ("f32", "exact"))
    sampled = hs.life_reference(mlp, math)
    assert len(ref) == len(hs.LIFE) >= 14
    for (kind, B, _, seed, _), (idx, out), (sidx, _) in zip(hs.LIFE, ref, sampled):
        assert {0, B - 1} <= set(sidx) and len(sidx) >= min(B, 5)
        if kind == "poison":
            uopt, xevol, info = out
            for k in range(len(idx)):
                assert not np.isfinite(info[k, [3, 5, 6]]).all(), (kind, seed, idx[k], info[k])     # gradient norm, initial cost or final cost
            assert not np.isfinite(xevol).all()
        else:
            for a in out:
                assert np.isfinite(np.asarray(a, np.float64)).all(), (kind, seed)
            if kind != "closed_loop":
                assert hs.holds_sentinel(*out) == 0
            if kind in ("solve", "solve_keys"):
                assert (out[2][:, 2] >= 1).all()                    # iterations ran


def test_poison_inputs_are_finite_and_distinct():
    cfg = hs.cfg_for(hs.LIFE_P)
    x0 = hs.poison_problem(cfg, 40, 103)[0]
    assert np.isfinite(x0).all() and len({r.tobytes() for r in x0}) == 40 and np.abs(x0[:, 10:13]).min() >= 5e29


@pytest.mark.parametrize("P", [1, 33, 70])
def test_sentinel_occurs_in_no_expected_output(P):
    _, _, prob, ref = hs.small_reference(P)
    for kind, out in ref.items():
        assert hs.holds_sentinel(*out) == 0, kind
        assert all(np.isfinite(np.asarray(a, np.float64)).all() for a in out), kind
    assert hs.holds_sentinel(*prob) == 0
    assert np.isfinite(np.array([hs.SENTINEL], np.uint32).view(np.float32)[0])
