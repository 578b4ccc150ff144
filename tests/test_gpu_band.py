"""Predicted bands (SPEC.md §12b) on the GPU: every output against tests/band_ref.py applied to the ORACLE's particle x horizon tensor, bit for bit — q by bits
with a NaN as 0x7FC00000, below / at exactly — on the cases of tests/band_cases.py, in every arithmetic and rollout layout, through every entry point, on a poisoned
handle, between guard words, with special values in the tensor and with several workgroups per launch."""
import numpy as np
import pytest

import band_cases as BC
import band_ref as BR
from cases import bits_differ
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import Bands, SdempcError, SdeMpcSolver

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A          # prefill of caller-owned buffers: no float32 result and no count of these cases has this pattern
GUARD = 64


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


def _rollout_dev(S, R, B, store_traj=True):
    """stages the first B instances and runs rollout_dev on the current torch stream; returns what must stay alive"""
    import torch
    dev = [torch.from_numpy(np.array(a[:B])).cuda() for a in (R["x0"], R["u"], R["xref"], S.noise_to_device_layout(R["noise"][:B]))]
    cost = torch.zeros(B, dtype=torch.float32, device="cuda")
    xmean = torch.zeros((B, S.H + 1, 13), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    S.rollout_dev(B, *[d.data_ptr() for d in dev], cost.data_ptr(), xmean.data_ptr(), store_traj, st)
    return dev, cost, xmean, st


def _same(got, want, what):
    """got: a solver.Bands or a dict; want: band_ref's dict. q by bits, below / at by value."""
    for k in ("q", "below", "at"):
        g, w = (getattr(got, k) if hasattr(got, k) else got[k]), want[k]
        if w is None:
            assert g is None, (what, k)
            continue
        g = np.asarray(g)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, g.dtype, w.shape, w.dtype)
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        if len(bad):
            i = tuple(bad[0])
            raise AssertionError(f"{what}: {k}: {len(bad)} words differ, first at {list(i)}: got {g[i]!r}, want {w[i]!r}")


def _check_case(name, mlp="f32", math="exact", options=None):
    R = BC.reference(name, mlp, math)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B, options=options or {})
    try:
        got = S.bands(R["x0"], R["u"], R["xref"], R["noise"], quantiles=None, ranks=R["ranks"], observed=R["obs"])
    finally:
        S.close()
    what = (name, mlp, math, options)
    _same(got, R["want"], what)
    assert bits_differ(got.cost, R["cost"]) == 0, (what, "cost")
    assert got.P == R["cfg"].num_particles and got.ranks == R["ranks"]
    # t = 0: every rank returns x0, and obs = x0 has nothing below it and every particle at it
    P = got.P
    assert (got.q[:, :, 0, :].view(np.uint32) == R["x0"].view(np.uint32)[:, None, :]).all()
    assert (got.below[:, 0] == 0).all() and (got.at[:, 0] == P).all()
    return got


@pytest.mark.parametrize("name", BC.NAMES)
def test_bands_f32_exact(name):
    _check_case(name)


@pytest.mark.parametrize("mlp", ["f32x3", "f16"])
@pytest.mark.parametrize("name", BC.BIG)
def test_bands_matrix_pipe_fast(name, mlp):
    _check_case(name, mlp, "fast")


def test_bands_single_particle_in_both_layouts():
    a = _check_case("h6_p1", options={"lane": 1})
    b = _check_case("h6_p1", options={"lane": 0})
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("duo", [0, 1])
def test_bands_do_not_depend_on_the_rollouts_layout(duo):
    _check_case("h6_p70", options={"duo": duo})


@pytest.mark.parametrize("name", ["h6_p33", "h6_p70", "h6_p128", "h6_p130"])
def test_bands_special_values(name):
    """Ties, NaN particles, an all-NaN instance and both zeros. The reference here is band_ref of the tensor the SAME handle returns through
    rollout(want_traj=True) on identical inputs, not the oracle's: how a rollout propagates a NaN (which words of a particle become NaN, and from which step) is
    the rollout's business and is tested elsewhere; here the REDUCER is judged, on whatever tensor the rollout left."""
    R = BC.reference(name)
    x0, u, xref, noise = BC.special_problem(name)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)
    try:
        _, traj, _ = S.rollout(x0, u, xref, noise, True, True)
        obs = BC.special_observations(traj, x0)
        got = S.bands(x0, u, xref, noise, quantiles=None, ranks=R["ranks"], observed=obs)
    finally:
        S.close()
    P = got.P
    _same(got, BR.bands(traj, R["ranks"], obs), (name, "special values"))
    assert (np.isnan(traj).any(axis=1) & ~np.isnan(traj).all(axis=1)).any(), "no partly-NaN column in the tensor"
    assert (traj[0, 0] == traj[0, 1]).all() and (traj[2, 0] == traj[2, 1]).all()              # exact ties at every step
    assert (got.q[1].view(np.uint32) == 0x7FC00000).all()                          # the all-NaN instance: every selected value is THE quiet NaN
    zc = BC.ZERO_COMPONENT
    assert (got.q[0, :, 0, zc].view(np.uint32) == 0x80000000).all() and (got.q[2, :, 0, zc].view(np.uint32) == 0x80000000).all()
    assert got.below[0, 0, zc] == P and got.at[0, 0, zc] == 0                      # obs +0.0 above P particles at -0.0
    assert got.below[2, 0, zc] == 0 and got.at[2, 0, zc] == P                      # obs -0.0 at them
    nan_obs = np.isnan(obs)
    assert nan_obs.any() and (got.below[nan_obs] + got.at[nan_obs] == P).all()
    assert np.isnan(got.pit[nan_obs]).all() and not got.inside(0, 0)[nan_obs].any()


def test_bands_keys_equals_bands_on_the_drawn_noise():
    R = BC.reference("h6_p33")
    keys = np.stack([prng.split(np.array([0, 91 + b], np.uint32), 2)[1] for b in range(BC.B)]).astype(np.uint32)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)
    noise = S.noise_from_keys(keys)
    a = S.bands_keys(R["x0"], R["u"], R["xref"], keys, quantiles=(0.05, 0.5, 0.95), observed=R["obs"])
    b = S.bands(R["x0"], R["u"], R["xref"], noise, quantiles=(0.05, 0.5, 0.95), observed=R["obs"])
    S.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a.ranks == tuple(BR.quantile_ranks((0.05, 0.5, 0.95), 33)) and a.median.tobytes() == a.band(1).tobytes()
    assert (BR.keys(a.band(0)) <= BR.keys(a.band(1))).all() and (BR.keys(a.band(1)) <= BR.keys(a.band(2))).all()


def _bands_dev_guarded(S, R, B, what, ranks, obs=True):
    import torch
    T = S.H + 1
    q = Guarded((B, len(ranks), T, 13)) if ranks else None
    below, at = (Guarded((B, T, 13)), Guarded((B, T, 13))) if obs else (None, None)
    o = torch.from_numpy(np.array(R["obs"][:B])).cuda() if obs else None
    st = torch.cuda.current_stream().cuda_stream
    S.bands_dev(B, ranks=ranks or None, observed=o.data_ptr() if obs else None, q=q.ptr if q else None, below=below.ptr if obs else None,
                at=at.ptr if obs else None, stream=st)
    torch.cuda.synchronize()
    return {"q": q.result((what, "q")) if q else None, "below": below.result((what, "below"), np.uint32) if obs else None,
            "at": at.result((what, "at"), np.uint32) if obs else None}


@pytest.mark.parametrize("name", ["h6_p33", "h6_p70", "h6_p130"])
def test_bands_dev_after_a_rollout_between_guard_words(name):
    R = BC.reference(name)
    want = R["want"]
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)
    keep = _rollout_dev(S, R, BC.B)
    _same(_bands_dev_guarded(S, R, BC.B, name, list(R["ranks"])), want, name)
    # fewer instances than the workspace holds: fine; some outputs only: the others are not touched
    part = _bands_dev_guarded(S, R, 2, (name, "first two"), list(R["ranks"]))
    _same(part, {k: v[:2] for k, v in want.items()}, (name, "first two"))
    _same(_bands_dev_guarded(S, R, BC.B, (name, "q alone"), list(R["ranks"]), obs=False), {"q": want["q"], "below": None, "at": None}, (name, "q alone"))
    _same(_bands_dev_guarded(S, R, BC.B, (name, "ranks alone"), [], obs=True), {"q": None, "below": want["below"], "at": want["at"]}, (name, "ranks alone"))
    S.close()
    assert keep is not None


def test_bands_dev_is_refused_when_the_workspace_holds_no_such_rollout():
    import torch
    R = BC.reference("h6_p33")
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)
    buf = torch.zeros((BC.B, 1, S.H + 1, 13), dtype=torch.float32, device="cuda")
    call = lambda B, st=0: S.bands_dev(B, ranks=[0], q=buf.data_ptr(), stream=st)
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(BC.B)
    keep = _rollout_dev(S, R, BC.B, store_traj=False)
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(BC.B)
    keep = _rollout_dev(S, R, 2)
    torch.cuda.synchronize()
    with pytest.raises(SdempcError, match="holds fewer instances"):
        call(BC.B)
    call(2, keep[3])
    torch.cuda.synchronize()
    keep = _rollout_dev(S, R, BC.B)
    torch.cuda.synchronize()
    u0 = np.tile(np.asarray(R["cfg"].uref, np.float32), (BC.B, S.H, 1))
    S.solve(R["x0"], R["xref"], R["noise"], u0, np.full(BC.B, 0.01, np.float32))
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(BC.B)
    S.close()


@pytest.mark.parametrize("name", ["h6_p1", "h6_p33", "h6_p70", "h6_p130"])
def test_bands_on_a_poisoned_handle(name):
    """SDEMPC_OPT_TEST_WS_FILL = 255: every float-valued device word the handle allocates starts as a NaN pattern — the padded lanes of the tensor among them.
    Same bits: the padded lanes are masked and no unwritten word is read."""
    _check_case(name, options={"test_ws_fill": 255})


@pytest.mark.parametrize("name", ["h6_p70", "h6_p130"])
def test_permuted_particles_give_identical_words(name):
    R = BC.reference(name)
    perm = np.random.default_rng(8).permutation(R["cfg"].num_particles)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)
    a = S.bands(R["x0"], R["u"], R["xref"], R["noise"], quantiles=None, ranks=R["ranks"], observed=R["obs"])
    b = S.bands(R["x0"], R["u"], R["xref"], R["noise"][:, perm], quantiles=None, ranks=R["ranks"], observed=R["obs"])
    S.close()
    for k in ("q", "below", "at"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (name, k)


@pytest.mark.parametrize("name", ["h6_p33", "h6_p128", "h6_p300"])
def test_extreme_ranks_are_the_tubes_min_and_max(name):
    R = BC.reference(name)
    P = R["cfg"].num_particles
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)
    bd = S.bands(R["x0"], R["u"], R["xref"], R["noise"], quantiles=(0.0, 1.0))
    tb = S.tube(R["x0"], R["u"], R["xref"], R["noise"])
    S.close()
    assert bd.ranks == (0, P - 1) and bd.below is None and bd.at is None
    assert not np.isnan(bd.q).any()
    assert (bd.band(0) == tb.min).all() and (bd.band(1) == tb.max).all()           # by value: the tube's extrema do not tell -0 from +0


def test_several_workgroups_per_launch():
    """B = 300 at P = 33, H = 6: 900 workgroups, instance indices far past one workgroup's"""
    R = BC.reference("h6_p33")
    Bn = 300
    rng = np.random.default_rng(6)
    x0 = np.tile(R["x0"], (Bn // BC.B, 1))
    x0[:, :6] += rng.normal(0, 0.2, (Bn, 6)).astype(np.float32)
    u, xref, noise, obs = (np.tile(R[k], (Bn // BC.B,) + (1,) * (R[k].ndim - 1)) for k in ("u", "xref", "noise", "obs"))
    rk = [32, 0, 16, 5]
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=Bn)
    got = S.bands(x0, u, xref, noise, quantiles=None, ranks=rk, observed=obs)
    _, traj, _ = S.rollout(x0, u, xref, noise, True, True)
    S.close()
    _same(got, BR.bands(traj, rk, obs), "B = 300")


def test_m_bands_extremes_are_m_tubes():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    R = BC.reference("h6_p33")
    prob = MpcProblem(R["cfg"].replace(max_iter=4, max_no_improvement_iter=4), R["model"], convert_to_enu=True)
    x = R["x0"][0]
    rng = np.array([0, 42], np.uint32)
    st = prob.m_reset(x, rng, x)
    uopt, _, _, _ = prob.m_mpc(x, rng, st, curr_t=0.0, xdes=x)
    t = prob.m_tube(x, rng, np.asarray(uopt), curr_t=0.0, xdes=x)
    bd = prob.m_bands(x, rng, np.asarray(uopt), curr_t=0.0, xdes=x, quantiles=(0, 1), observed=t.mean)
    prob.solver().close()
    assert isinstance(bd, Bands) and bd.q.shape == (2, prob.cfg.horizon + 1, 13) and bd.P == 33 and bd.below.dtype == np.uint32
    assert (bd.band(0) == t.min).all() and (bd.band(1) == t.max).all()
    # (the rounded mean may lie a rounding outside [min, max]) obs >= min iff something is below or at it, obs <= max iff not everything is below it
    assert np.array_equal(bd.inside(0, 1), (bd.below + bd.at >= 1) & (bd.below < bd.P)) and ((bd.pit >= 0) & (bd.pit <= 1)).all()
    assert bd.inside(0, 1)[1:, 3:6].all()
    assert bd.cost.tobytes() == t.cost.tobytes()


def test_other_modes_of_the_hosting_kernel_are_unchanged_by_a_bands_call():
    """tube, risk and noise outputs of one handle before and after a bands call"""
    R = BC.reference("h6_p70")
    keys = np.stack([prng.split(np.array([0, 5 + b], np.uint32), 2)[1] for b in range(BC.B)]).astype(np.uint32)
    lo, hi = np.full(13, -0.5, np.float32), np.full(13, 0.5, np.float32)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=BC.B)

    def others():
        t = S.tube(R["x0"], R["u"], R["xref"], R["noise"], lo=lo, hi=hi)
        r = S.risk(R["x0"], R["u"], R["xref"], R["noise"], lo=lo, hi=hi, centre="xref", tail=0.1, quantiles=(0.5, 0.9), want_particles=True)
        return [np.asarray(a).tobytes() for a in t] + [np.asarray(a).tobytes() for a in r if a is not None] + [S.noise_from_keys(keys).tobytes()]
    before = others()
    _same(S.bands(R["x0"], R["u"], R["xref"], R["noise"], quantiles=None, ranks=R["ranks"], observed=R["obs"]), R["want"], "between")
    after = others()
    S.close()
    assert before == after
