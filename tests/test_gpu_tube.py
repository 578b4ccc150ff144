"""The predicted tube (SPEC.md §12) on the GPU: every plane against tests/tube_ref.py applied to the ORACLE's particle x horizon tensor — mean, var and outside bit
for bit, min and max by value — on the cases of tests/tube_cases.py, in every arithmetic and rollout layout, through every entry point, on a poisoned handle,
between guard words, with a non-finite instance in the batch and with several workgroups per launch."""
import numpy as np
import pytest

import orc
import tube_cases as TC
import tube_ref as TR
from cases import bits_differ
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import SdempcError, SdeMpcSolver

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A          # prefill of caller-owned buffers: no float32 result and no count of these cases has this pattern
GUARD = 64


def _same(got, want, what):
    """got: a solver.Tube or a dict of planes; want: tube_ref's dict"""
    for k in TR.PLANES:
        g, w = np.asarray(getattr(got, k) if hasattr(got, k) else got[k]), want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, g.dtype)
        if k == "outside":
            bad = np.argwhere(g != w)
        elif k in TR.BITS_PLANES:
            bad = np.argwhere((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w)))
        else:
            bad = np.argwhere((g != w) & ~(np.isnan(g) & np.isnan(w)))
        if len(bad):
            i = tuple(bad[0])
            raise AssertionError(f"{what}: plane {k}: {len(bad)} words differ, first at {list(i)}: got {g[i]!r}, want {w[i]!r}")


def _check_case(name, mlp="f32", math="exact", options=None):
    R = TC.reference(name, mlp, math)
    want = TR.tube(R["traj"], R["lo"], R["hi"])
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=TC.B, options=options or {})
    try:
        got = S.tube(R["x0"], R["u"], R["xref"], R["noise"], lo=R["lo"], hi=R["hi"])
        cost, _, xmean = S.rollout(R["x0"], R["u"], R["xref"], R["noise"], False, True)
    finally:
        S.close()
    what = (name, mlp, math, options)
    _same(got, want, what)
    assert got.mean.tobytes() == xmean.tobytes(), (what, "mean is not the rollout's xmean")
    assert got.cost.tobytes() == cost.tobytes() and bits_differ(cost, R["cost"]) == 0, (what, "cost")
    assert got.P == R["cfg"].num_particles and got.std.dtype == np.float32
    assert np.array_equal(got.p_outside, want["outside"] / got.P)
    return got


@pytest.mark.parametrize("name", TC.NAMES)
def test_tube_f32_exact(name):
    _check_case(name)


@pytest.mark.parametrize("mlp", ["f32x3", "f16"])
@pytest.mark.parametrize("name", TC.BIG)
def test_tube_matrix_pipe_fast(name, mlp):
    _check_case(name, mlp, "fast")


def test_tube_single_particle_in_both_layouts():
    a = _check_case("h6_p1", options={"lane": 1})
    b = _check_case("h6_p1", options={"lane": 0})
    assert (a.var == 0).all() and (a.min == a.max).all() and (a.min == a.mean).all()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("duo", [0, 1])
def test_tube_does_not_depend_on_the_rollouts_layout(duo):
    _check_case("h6_p70", options={"duo": duo})


def test_tube_keys_equals_tube_on_the_drawn_noise():
    R = TC.reference("h6_p33")
    keys = np.stack([prng.split(np.array([0, 77 + b], np.uint32), 2)[1] for b in range(TC.B)]).astype(np.uint32)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=TC.B)
    noise = S.noise_from_keys(keys)
    a = S.tube_keys(R["x0"], R["u"], R["xref"], keys, lo=R["lo"], hi=R["hi"])
    b = S.tube(R["x0"], R["u"], R["xref"], noise, lo=R["lo"], hi=R["hi"])
    S.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert (a.var[:, 1:, 3:6] > 0).all()
    assert bits_differ(noise[0], orc.noise_from_key(keys[0], R["cfg"].num_particles, R["cfg"].horizon)) == 0


# ---- device pointers: guard | payload | guard ------------------------------------------------------------------------------------------
class Guarded:
    def __init__(self, shape):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.t = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * GUARD
        torch.cuda.current_stream().synchronize()

    def result(self, what, dtype=np.float32):
        w = self.t.cpu().numpy().view(np.uint32)
        lo, pay, hi = w[:GUARD], w[GUARD:GUARD + self.n], w[GUARD + self.n:]
        assert (lo == SENTINEL).all(), (what, "write in front of the buffer")
        assert (hi == SENTINEL).all(), (what, "write behind the buffer")
        assert not (pay == SENTINEL).any(), (what, "words never written", np.flatnonzero(pay == SENTINEL)[:4])
        return pay.view(dtype).reshape(self.shape).copy()


def _rollout_dev(S, R, B, store_traj=True, x0=None):
    """stages the first B instances and runs rollout_dev on the current torch stream; returns what must stay alive"""
    import torch
    x0 = R["x0"] if x0 is None else x0
    dev = [torch.from_numpy(np.array(a[:B])).cuda() for a in (x0, R["u"], R["xref"], S.noise_to_device_layout(R["noise"][:B]))]
    cost = torch.zeros(B, dtype=torch.float32, device="cuda")
    xmean = torch.zeros((B, S.H + 1, 13), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    S.rollout_dev(B, *[d.data_ptr() for d in dev], cost.data_ptr(), xmean.data_ptr(), store_traj, st)
    return dev, cost, xmean, st


def _tube_dev_guarded(S, R, B, what, outside=True):
    import torch
    shape = (B, S.H + 1, 13)
    planes = [Guarded(shape) for _ in range(5)]
    st = torch.cuda.current_stream().cuda_stream
    S.tube_dev(B, *[p.ptr for p in planes[:4]], planes[4].ptr if outside else None, lo=R["lo"] if outside else None, hi=R["hi"] if outside else None, stream=st)
    torch.cuda.synchronize()
    out = {k: p.result((what, k), np.uint32 if k == "outside" else np.float32) for k, p in zip(TR.PLANES, planes) if outside or k != "outside"}
    return out


@pytest.mark.parametrize("name", ["h6_p33", "h6_p130"])
def test_tube_dev_after_a_rollout_between_guard_words(name):
    import torch
    R = TC.reference(name)
    want = TR.tube(R["traj"], R["lo"], R["hi"])
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=TC.B)
    keep = _rollout_dev(S, R, TC.B)
    got = _tube_dev_guarded(S, R, TC.B, name)
    _same(got, want, name)
    assert keep[2].cpu().numpy().tobytes() == got["mean"].tobytes()
    # fewer instances than the workspace holds: fine; some planes only: the others are not touched
    part = _tube_dev_guarded(S, R, 2, (name, "first two"))
    _same(part, {k: v[:2] for k, v in want.items()}, (name, "first two"))
    only = Guarded((TC.B, S.H + 1, 13))
    S.tube_dev(TC.B, None, only.ptr, None, None, stream=keep[3])
    torch.cuda.synchronize()
    assert only.result((name, "var alone")).tobytes() == want["var"].tobytes()
    S.close()


def test_tube_dev_is_refused_when_the_workspace_holds_no_such_rollout():
    import torch
    R = TC.reference("h6_p33")
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=TC.B)
    buf = torch.zeros((TC.B, S.H + 1, 13), dtype=torch.float32, device="cuda")
    with pytest.raises(SdempcError, match="holds no rollout"):
        S.tube_dev(TC.B, buf.data_ptr(), None, None, None)
    keep = _rollout_dev(S, R, TC.B, store_traj=False)
    with pytest.raises(SdempcError, match="holds no rollout"):
        S.tube_dev(TC.B, buf.data_ptr(), None, None, None)
    keep = _rollout_dev(S, R, 2)
    torch.cuda.synchronize()
    with pytest.raises(SdempcError, match="holds fewer instances"):
        S.tube_dev(TC.B, buf.data_ptr(), None, None, None)
    S.tube_dev(2, buf.data_ptr(), None, None, None, stream=keep[3])
    torch.cuda.synchronize()
    S.grad(R["x0"], R["u"], R["xref"], R["noise"])
    with pytest.raises(SdempcError, match="holds no rollout"):
        S.tube_dev(2, buf.data_ptr(), None, None, None)
    keep = _rollout_dev(S, R, TC.B)
    torch.cuda.synchronize()
    u0 = np.tile(np.asarray(R["cfg"].uref, np.float32), (TC.B, S.H, 1))
    S.solve(R["x0"], R["xref"], R["noise"], u0, np.full(TC.B, 0.01, np.float32))
    with pytest.raises(SdempcError, match="holds no rollout"):
        S.tube_dev(TC.B, buf.data_ptr(), None, None, None)
    S.close()


@pytest.mark.parametrize("name", ["h6_p1", "h6_p33", "h6_p70", "h6_p130"])         # (h6_p130: five groups, the path that loads twice)
def test_tube_on_a_poisoned_handle(name):
    """SDEMPC_OPT_TEST_WS_FILL = 255: every float-valued device word the handle allocates starts as a NaN pattern — the padded lanes of the tensor among them (the
    rollout does not write them) and the tube's staging planes. Same bits: the padded lanes are masked and no unwritten word is read."""
    _check_case(name, options={"test_ws_fill": 255})


def test_one_non_finite_instance_stays_alone():
    R = TC.reference("h6_p33")
    P = R["cfg"].num_particles
    x0, u, xref, noise = TC.nonfinite_variant("h6_p33", b=1)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=TC.B)
    bad = S.tube(x0, u, xref, noise, lo=R["lo"], hi=R["hi"])
    good = S.tube(R["x0"], u, xref, noise, lo=R["lo"], hi=R["hi"])
    S.close()
    _, traj, _ = TC.oracle_rollout(R["cfg"], R["model"], x0, u, xref, noise)
    _same(bad, TR.tube(traj, R["lo"], R["hi"]), "non-finite instance")
    assert np.isnan(traj[1]).all()                                 # every particle of instance 1 is NaN in every column
    assert (bad.outside[1] == P).all() and np.isnan(bad.mean[1]).all() and np.isnan(bad.var[1]).all()      # a NaN counts, bounded component or not
    assert (bad.min[1] == np.inf).all() and (bad.max[1] == -np.inf).all()
    for b in (0, 2):
        assert all(np.asarray(x)[b].tobytes() == np.asarray(y)[b].tobytes() for x, y in zip(bad, good)), b


def test_several_workgroups_per_launch():
    """B = 300 at P = 1, H = 6: 900 workgroups, instance indices far past one workgroup's"""
    R = TC.reference("h6_p1")
    cfg, model = R["cfg"], R["model"]
    Bn = 300
    rng = np.random.default_rng(5)
    x0 = np.tile(R["x0"], (Bn // TC.B, 1))
    x0[:, :6] += rng.normal(0, 0.2, (Bn, 6)).astype(np.float32)
    u, xref, noise = (np.tile(R[k], (Bn // TC.B,) + (1,) * (R[k].ndim - 1)) for k in ("u", "xref", "noise"))
    S = SdeMpcSolver(cfg, model, max_batch=Bn)
    got = S.tube(x0, u, xref, noise, lo=R["lo"], hi=R["hi"])
    _, traj, xmean = S.rollout(x0, u, xref, noise, True, True)
    S.close()
    _same(got, TR.tube(traj, R["lo"], R["hi"]), "B = 300")
    assert got.mean.tobytes() == xmean.tobytes()
    O = orc.Oracle(cfg, model)
    for b in (0, 149, 299):
        _, t, xm = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        assert bits_differ(traj[b], t) == 0 and bits_differ(got.mean[b], xm) == 0, b


@pytest.mark.parametrize("enu", [False, True])
def test_m_tube_mean_is_m_mpcs_xevol(enu):
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    R = TC.reference("h6_p33")
    prob = MpcProblem(R["cfg"].replace(max_iter=4, max_no_improvement_iter=4), R["model"], convert_to_enu=enu)
    x = R["x0"][0]
    rng = np.array([0, 42], np.uint32)
    st = prob.m_reset(x, rng, x)
    uopt, st2, new_rng, xevol = prob.m_mpc(x, rng, st, curr_t=0.0, xdes=x)
    t = prob.m_tube(x, rng, np.asarray(uopt), curr_t=0.0, xdes=x, lo=R["lo"], hi=R["hi"])
    prob.solver().close()
    assert t.mean.shape == (prob.cfg.horizon + 1, 13) and t.outside.dtype == np.uint32 and t.P == 33
    mean = enu2ned(t.mean, np) if enu else t.mean
    assert np.asarray(xevol).tobytes() == np.asarray(mean, np.float32).tobytes()
    assert (t.var[1:, 3:6] > 0).all() and float(st2.num_steps) >= 1
