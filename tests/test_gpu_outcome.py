"""Predicted outcome (SPEC.md §12c) on the GPU: every output against tests/outcome_ref.py applied to the ORACLE's particle x horizon tensor, bit for bit — integer
words exactly, float words by bit pattern with NaNs as a class, the min / max columns by value — on the cases of tests/outcome_cases.py, in every arithmetic,
through every entry point, each output alone, with special values in the tensor, with every target shape, on a poisoned handle and on a handle with a past."""
import numpy as np
import pytest

import band_ref as BR
import outcome_cases as OC
import outcome_ref as OR
import tube_ref as TR
from cases import bits_differ
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import Outcome, SdempcError, SdeMpcSolver

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A          # prefill of caller-owned buffers: no float32 result and no count of these cases has this pattern
GUARD = 64


class Guarded:
    """device words: guard | payload | guard"""

    def __init__(self, shape):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.t = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * GUARD
        torch.cuda.current_stream().synchronize()

    def result(self, what, dtype):
        w = self.t.cpu().numpy().view(np.uint32)
        lo, pay, hi = w[:GUARD], w[GUARD:GUARD + self.n], w[GUARD + self.n:]
        assert (lo == SENTINEL).all(), (what, "write in front of the buffer")
        assert (hi == SENTINEL).all(), (what, "write behind the buffer")
        assert not (pay == SENTINEL).any(), (what, "words never written", np.flatnonzero(pay == SENTINEL)[:4])
        return pay.view(dtype).reshape(self.shape).copy()


def _same(got, want, what):
    n = OR.differs(got, want)
    if n:
        for k in OR.OUTPUTS:
            g, w = (getattr(got, k) if not isinstance(got, dict) else got[k]), want[k]
            if g is not None and w is not None and OR.differs({q: (g if q == k else None) for q in OR.OUTPUTS}, {q: (w if q == k else None) for q in OR.OUTPUTS}):
                bad = np.argwhere(np.asarray(g).view(np.uint32) != np.asarray(w).view(np.uint32))
                i = tuple(bad[0])
                raise AssertionError(f"{what}: {k}: {n} words differ in all, first of {k} at {list(i)}: got {np.asarray(g)[i]!r}, want {np.asarray(w)[i]!r}")
    assert n == 0, what


def _check_case(name, mlp="f32", math="exact", options=None):
    R = OC.reference(name, mlp, math)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B, options=options or {})
    try:
        got = S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], ranks=R["ranks"], quantiles=None, want_particles=True)
    finally:
        S.close()
    what = (name, mlp, math, options)
    _same(got, R["want"], what)
    assert bits_differ(got.cost, R["cost"]) == 0, (what, "cost")
    assert got.P == R["cfg"].num_particles and got.ranks == R["ranks"]
    assert (got.first_fail.sum(axis=1) == got.P).all()
    return got


@pytest.mark.parametrize("name", OC.NAMES)
def test_outcome_f32_exact(name):
    _check_case(name)


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("mlp", ["f32", "f16", "f32x3"])
@pytest.mark.parametrize("name", OC.BIG)
def test_outcome_in_every_arithmetic(name, mlp, math):
    _check_case(name, mlp, math)


@pytest.mark.parametrize("name", ["h6_p1", "h6_p33", "h6_p70", "h6_p130"])
def test_outcome_on_a_poisoned_handle(name):
    """SDEMPC_OPT_TEST_WS_FILL = 255: every float-valued device word the handle allocates starts as a NaN pattern — the padded lanes of the tensor among them.
    Same bits: the padded lanes are masked and no unwritten word is read."""
    _check_case(name, options={"test_ws_fill": 255})


@pytest.mark.parametrize("name", ["h6_p33", "h6_p130"])
@pytest.mark.parametrize("per_step,per_instance", OC.TARGET_SHAPES)
def test_every_target_shape(name, per_step, per_instance):
    R = OC.reference(name)
    tg = OC.targets(R["xref"], per_step, per_instance)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    got = S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], target=tg, ranks=R["ranks"], quantiles=None, want_particles=True)
    S.close()
    want = OR.outcome(R["traj"], R["thresholds"], target=tg, ranks=R["ranks"])
    _same(got, want, (name, tg.shape))
    assert OR.differs(want, R["want"]) > 0                                  # the rows are not the xref window


@pytest.mark.parametrize("name", ["h6_p33", "h6_p70", "h6_p128", "h6_p130"])
def test_outcome_special_values(name):
    """Ties, NaN particles, an all-NaN instance and a +inf position. The reference here is outcome_ref of the tensor the SAME handle returns through
    rollout(want_traj=True) on identical inputs, not the oracle's: how a rollout propagates a NaN is the rollout's business and is tested elsewhere; here the
    REDUCER is judged, on whatever tensor the rollout left."""
    R = OC.reference(name)
    x0, u, xref, noise = OC.special_problem(name)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    try:
        _, traj, _ = S.rollout(x0, u, xref, noise, True, True)
        got = S.outcome(x0, u, xref, noise, score=R["score"], ranks=R["ranks"], quantiles=None, want_particles=True)
    finally:
        S.close()
    P = got.P
    _same(got, OR.outcome(traj, R["thresholds"], xref=xref, ranks=R["ranks"]), (name, "special values"))
    w = got.words
    assert (w[0, 0] == w[0, 1]).all() and (w[2, 0] == w[2, 1]).all()                       # exact ties
    assert ((w[:, 2:5, 9] & 8) == 8).all() and (w[0, 5:, 9] & 8 == 0).all()                # the NaN particles carry bit 8, their neighbours do not
    assert (got.cause_ever[1] == P).all() and got.first_fail[1, 0] == P                    # the all-NaN instance
    assert np.isposinf(got.chan_stat[1, :, :, 1]).all() and np.isneginf(got.chan_stat[1, :, :, 2]).all()
    assert got.cause_ever[2, 0] == P and got.cause_ever[2, 3] == P                         # the +inf position: radius and non-finite in every particle
    if got.chan_q is not None:
        assert (got.chan_q[1].view(np.uint32) == 0x7FC00000).all()                         # every selected value of the all-NaN instance is THE quiet NaN


def _rollout_dev(S, R, B, store_traj=True):
    """stages the first B instances and runs rollout_dev on the current torch stream; returns what must stay alive"""
    import torch
    dev = [torch.from_numpy(np.array(a[:B])).cuda() for a in (R["x0"], R["u"], R["xref"], S.noise_to_device_layout(R["noise"][:B]))]
    cost = torch.zeros(B, dtype=torch.float32, device="cuda")
    xmean = torch.zeros((B, S.H + 1, 13), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    S.rollout_dev(B, *[d.data_ptr() for d in dev], cost.data_ptr(), xmean.data_ptr(), store_traj, st)
    return dev, cost, xmean, st


def _shapes(S, B, K):
    H, P = S.H, S.P
    return {"words": ((B, P, 11), np.uint32), "fail_step": ((B, H, 5), np.uint32), "first_fail": ((B, H + 1), np.uint32), "cause_ever": ((B, 4), np.uint32),
            "chan_stat": ((B, H, 4, 3), np.float32), "chan_q": ((B, H, 4, K), np.float32), "agg_stat": ((B, 4, 3), np.float32), "agg_q": ((B, 4, K), np.float32)}


def _outcome_dev_guarded(S, R, B, keep, what, outputs, target=None):
    """outcome_dev with exactly `outputs` given, each between guard words -> dict (None for the others)"""
    import torch
    ranks = list(R["ranks"]) if R["ranks"] else None
    shapes = _shapes(S, B, len(ranks) if ranks else 0)
    bufs = {k: Guarded(shapes[k][0]) for k in outputs}
    tg = torch.from_numpy(np.array(target)).cuda() if target is not None else None
    want_q = "chan_q" in outputs or "agg_q" in outputs
    S.outcome_dev(B, score=R["score"], target=tg.data_ptr() if tg is not None else None, tgt_steps=target.shape[1] if target is not None else None,
                  tgt_batch=target.shape[0] if target is not None else None, xref=keep[0][2].data_ptr(), ranks=ranks if want_q else None,
                  stream=keep[3], **{k: b.ptr for k, b in bufs.items()})
    torch.cuda.synchronize()
    return {k: (bufs[k].result((what, k), shapes[k][1]) if k in bufs else None) for k in OR.OUTPUTS}


@pytest.mark.parametrize("name", ["h6_p33", "h6_p70", "h6_p130"])
def test_outcome_dev_between_guard_words_and_each_output_alone(name):
    R = OC.reference(name)
    want = R["want"]
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    keep = _rollout_dev(S, R, OC.B)
    have = [k for k in OR.OUTPUTS if want[k] is not None]
    _same(_outcome_dev_guarded(S, R, OC.B, keep, name, have), want, name)
    for k in have:                                                           # the others NULL: the same words, nothing else touched
        alone = _outcome_dev_guarded(S, R, OC.B, keep, (name, k, "alone"), [k])
        _same(alone, {q: (want[q] if q == k else None) for q in OR.OUTPUTS}, (name, k, "alone"))
    # fewer instances than the workspace holds; caller's rows through device pointers
    part = _outcome_dev_guarded(S, R, 2, keep, (name, "first two"), have)
    _same(part, {k: (None if v is None else v[:2]) for k, v in want.items()}, (name, "first two"))
    tg = OC.targets(R["xref"], True, False)
    _same(_outcome_dev_guarded(S, R, OC.B, keep, (name, "rows"), have, target=tg), OR.outcome(R["traj"], R["thresholds"], target=tg, ranks=R["ranks"]), (name, "rows"))
    S.close()
    assert keep is not None


def test_the_three_entry_points_agree():
    R = OC.reference("h6_p33")
    keys = np.stack([prng.split(np.array([0, 17 + b], np.uint32), 2)[1] for b in range(OC.B)]).astype(np.uint32)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    noise = S.noise_from_keys(keys)
    kw = dict(score=R["score"], quantiles=(0.05, 0.5, 0.95), want_particles=True)
    a = S.outcome_keys(R["x0"], R["u"], R["xref"], keys, **kw)
    b = S.outcome(R["x0"], R["u"], R["xref"], noise, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a.ranks == tuple(BR.quantile_ranks((0.05, 0.5, 0.95), 33)) and a.quantiles == (0.05, 0.5, 0.95)
    R2 = dict(R, noise=noise, ranks=a.ranks)
    keep = _rollout_dev(S, R2, OC.B)
    c = _outcome_dev_guarded(S, R2, OC.B, keep, "dev", list(OR.OUTPUTS))
    S.close()
    assert OR.differs(c, {k: getattr(a, k) for k in OR.OUTPUTS}) == 0
    for k in OR.OUTPUTS:
        assert c[k].tobytes() == getattr(a, k).tobytes(), k
    # the order statistics are ordered, and the conveniences read them
    assert (BR.keys(a.chan_q[..., 0]) <= BR.keys(a.chan_q[..., 1])).all() and (BR.keys(a.chan_q[..., 1]) <= BR.keys(a.chan_q[..., 2])).all()
    assert (a.pos_err(0) <= a.pos_err(2)).all() and (a.tilt_deg(0) >= a.tilt_deg(2)).all() and ((a.p_fail >= 0) & (a.p_fail <= 1)).all()


def test_want_particles_and_no_ranks():
    R = OC.reference("h6_p70")
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    a = S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], ranks=R["ranks"], quantiles=None, want_particles=False)
    b = S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], ranks=None, quantiles=None)
    S.close()
    assert a.words is None and b.words is None and b.chan_q is None and b.agg_q is None and b.ranks is None
    _same(a, dict(R["want"], words=None), "no particles")
    _same(b, dict(R["want"], words=None, chan_q=None, agg_q=None), "no ranks")


def test_outcome_refusals_on_the_device():
    import torch
    R = OC.reference("h6_p33")
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    buf = torch.zeros((OC.B, S.H + 1), dtype=torch.int32, device="cuda")
    xr = torch.from_numpy(np.array(R["xref"])).cuda()
    call = lambda B, st=0: S.outcome_dev(B, score=R["score"], xref=xr.data_ptr(), first_fail=buf.data_ptr(), stream=st)
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(OC.B)
    keep = _rollout_dev(S, R, OC.B, store_traj=False)
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(OC.B)
    keep = _rollout_dev(S, R, 2)
    torch.cuda.synchronize()
    with pytest.raises(SdempcError, match="holds fewer instances"):
        call(OC.B)
    call(2, keep[3])
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy()[:2].view(np.uint32), R["want"]["first_fail"][:2])
    with pytest.raises(SdempcError, match="NaN"):
        S.outcome_dev(2, score=type("S", (), {"thresholds": lambda self: (np.float32(np.nan), np.float32(0), np.float32(1))})(), xref=xr.data_ptr(),
                      first_fail=buf.data_ptr(), stream=keep[3])
    with pytest.raises(SdempcError, match="no output"):
        S.outcome_dev(2, score=R["score"], xref=xr.data_ptr(), stream=keep[3])
    with pytest.raises(SdempcError, match="rank"):
        S.outcome_dev(2, score=R["score"], xref=xr.data_ptr(), ranks=[33], agg_q=buf.data_ptr(), stream=keep[3])
    with pytest.raises(SdempcError, match="tgt_steps"):
        S.outcome_dev(2, score=R["score"], target=xr.data_ptr(), tgt_steps=3, first_fail=buf.data_ptr(), stream=keep[3])
    u0 = np.tile(np.asarray(R["cfg"].uref, np.float32), (OC.B, S.H, 1))
    S.solve(R["x0"], R["xref"], R["noise"], u0, np.full(OC.B, 0.01, np.float32))
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(2)
    S.close()
    # the particle limit of the order statistics, through the host form
    R = OC.reference("h6_p130")
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)
    with pytest.raises(SdempcError, match="128 particles"):
        S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], quantiles=(0.5,))
    S.close()


def test_a_handle_with_a_past():
    """noise, tube, risk and bands of one handle, then an outcome call, then the four again: the same bytes, and the tube's and the bands' still their own
    references' of the oracle's tensor — the new mode disturbs none."""
    R = OC.reference("h6_p70")
    keys = np.stack([prng.split(np.array([0, 5 + b], np.uint32), 2)[1] for b in range(OC.B)]).astype(np.uint32)
    lo, hi = np.full(13, -0.5, np.float32), np.full(13, 0.5, np.float32)
    rk = [69, 0, 35]
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=OC.B)

    def others():
        t = S.tube(R["x0"], R["u"], R["xref"], R["noise"], lo=lo, hi=hi)
        r = S.risk(R["x0"], R["u"], R["xref"], R["noise"], lo=lo, hi=hi, centre="xref", tail=0.1, quantiles=(0.5, 0.9), want_particles=True)
        q = S.bands(R["x0"], R["u"], R["xref"], R["noise"], quantiles=None, ranks=rk, observed=R["xref"])
        return t, q, [np.asarray(a).tobytes() for a in t] + [np.asarray(a).tobytes() for a in r if a is not None] + [np.asarray(a).tobytes() for a in q] + \
            [S.noise_from_keys(keys).tobytes()]
    _, _, before = others()
    _same(S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], ranks=R["ranks"], quantiles=None, want_particles=True), R["want"], "between")
    t, q, after = others()
    _same(S.outcome(R["x0"], R["u"], R["xref"], R["noise"], score=R["score"], ranks=R["ranks"], quantiles=None, want_particles=True), R["want"], "behind")
    S.close()
    assert before == after
    tw = TR.tube(R["traj"], lo, hi)
    assert TR.planes_differ({k: getattr(t, k) for k in TR.PLANES}, tw) == 0
    bw = BR.bands(R["traj"], rk, R["xref"])
    assert all(getattr(q, k).tobytes() == bw[k].tobytes() for k in ("q", "below", "at"))


def test_several_workgroups_per_launch():
    """B = 300 at P = 33, H = 6: instance indices far past the first workgroups'"""
    R = OC.reference("h6_p33")
    Bn = 300
    rng = np.random.default_rng(6)
    x0 = np.tile(R["x0"], (Bn // OC.B, 1))
    x0[:, :6] += rng.normal(0, 0.2, (Bn, 6)).astype(np.float32)
    u, xref, noise = (np.tile(R[k], (Bn // OC.B,) + (1,) * (R[k].ndim - 1)) for k in ("u", "xref", "noise"))
    rk = [32, 0, 16, 5]
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=Bn)
    got = S.outcome(x0, u, xref, noise, score=R["score"], ranks=rk, quantiles=None, want_particles=True)
    _, traj, _ = S.rollout(x0, u, xref, noise, True, True)
    S.close()
    _same(got, OR.outcome(traj, R["thresholds"], xref=xref, ranks=rk), "B = 300")


def test_m_outcome_is_outcome_keys_on_the_solves_noise():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.solver import Score
    R = OC.reference("h6_p33")
    prob = MpcProblem(R["cfg"].replace(max_iter=4, max_no_improvement_iter=4), R["model"], convert_to_enu=True)
    x = R["x0"][0]
    rng = np.array([0, 42], np.uint32)
    st = prob.m_reset(x, rng, x)
    uopt, _, _, _ = prob.m_mpc(x, rng, st, curr_t=0.0, xdes=x)
    sc = Score(pos_radius=0.05, tilt_max=np.radians(3.0), rate_max=0.5)
    o = prob.m_outcome(x, rng, np.asarray(uopt), curr_t=0.0, xdes=x, score=sc, quantiles=(0.0, 0.5, 1.0))
    t = prob.m_tube(x, rng, np.asarray(uopt), curr_t=0.0, xdes=x)
    prob.solver().close()
    H = prob.cfg.horizon
    assert isinstance(o, Outcome) and o.P == 33 and o.first_fail.shape == (H + 1,) and o.fail_step.shape == (H, 5) and o.chan_q.shape == (H, 4, 3)
    assert o.first_fail.sum() == 33 and o.cost.tobytes() == t.cost.tobytes() and o.words is None
    # the body-rate channel against the tube of the same tensor: max w2 per row is bounded by the squared extrema of the three rate components
    bound = np.maximum(t.min[1:, 10:] ** 2, t.max[1:, 10:] ** 2).sum(axis=1)
    assert (o.chan_stat[:, 3, 2] <= bound * (1 + 1e-6)).all() and (o.chan_q[:, 3, 2] == o.chan_stat[:, 3, 2]).all()
