"""Predicted risk (SPEC.md §12a) on the GPU: every output against tests/risk_ref.py applied to the ORACLE's particle x horizon tensor — bit for bit, min and max
by value — on the cases of tests/risk_cases.py, in every arithmetic and rollout layout, with every centre mode, through every entry point, on a poisoned handle,
between guard words, with a non-finite instance in the batch, with several workgroups per launch and with more particle groups than a workgroup has halves."""
import numpy as np
import pytest

import orc
import risk_cases as RC
import risk_ref as RR
import tube_cases as TC
from cases import bits_differ
from sde4mbrl_px4_amd import prng
from sde4mbrl_px4_amd.solver import SdempcError, SdeMpcSolver

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A          # prefill of caller-owned buffers: no float32 result and no count of these cases has this pattern
GUARD = 64


def _same(got, want, what):
    """got: a solver.Risk or a dict; want: risk_ref's dict"""
    for k in RR.OUTPUTS:
        g, w = (getattr(got, k) if hasattr(got, k) else got[k]), want[k]
        assert (g is None) == (w is None), (what, k)
        if w is None:
            continue
        g = np.asarray(g)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, g.dtype, w.shape, w.dtype)
    n = RR.outputs_differ({k: (getattr(got, k) if hasattr(got, k) else got[k]) for k in RR.OUTPUTS}, want)
    if n:
        for k in RR.OUTPUTS:
            g = np.asarray(getattr(got, k) if hasattr(got, k) else got[k])
            if want[k] is not None and g.tobytes() != want[k].tobytes():
                bad = np.argwhere(~((g == want[k]) | (np.isnan(g.astype(np.float64)) & np.isnan(want[k].astype(np.float64)))))
                i = tuple(bad[0]) if len(bad) else None
                raise AssertionError(f"{what}: {n} words differ; {k}: first at {i}: got {g[i] if i else g!r}, want {want[k][i] if i else want[k]!r}")
        raise AssertionError(f"{what}: {n} words differ")


def _kw(R, centre="rows"):
    return dict(lo=R["lo"], hi=R["hi"], centre=R.get("centre", R["xmean"]) if isinstance(centre, str) and centre == "rows" else centre, tail=R["tail_k"],
                quantiles=RC.QUANTILES, want_particles=True)


def _check_case(R, what, options=None, centre="rows", want=None):
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=RC.B, options=options or {})
    try:
        got = S.risk(R["x0"], R["u"], R["xref"], R["noise"], **_kw(R, centre))
        cost = S.rollout(R["x0"], R["u"], R["xref"], R["noise"], False, False)[0]
    finally:
        S.close()
    _same(got, R["want"] if want is None else want, what)
    assert got.cost.tobytes() == cost.tobytes() and bits_differ(cost, R["cost"]) == 0, (what, "cost")
    assert got.P == R["cfg"].num_particles
    assert np.array_equal(got.p_ever, 1.0 - got.first_exit[:, -1] / got.P) and got.survival.shape == (RC.B, R["cfg"].horizon + 1)
    return got


@pytest.mark.parametrize("name", RC.NAMES)
def test_risk_f32_exact(name):
    _check_case(RC.reference(name), name)


@pytest.mark.parametrize("mlp", ["f32x3", "f16"])
@pytest.mark.parametrize("name", RC.BIG)
def test_risk_matrix_pipe_fast(name, mlp):
    _check_case(RC.reference(name, mlp, "fast"), (name, mlp))


def test_risk_single_particle_in_both_layouts():
    R = RC.reference("h6_p1")
    a = _check_case(R, "lane", options={"lane": 1})
    b = _check_case(R, "tile", options={"lane": 0})
    assert (a.jstat[:, 1] == 0).all() and (a.jq == a.jx).all() and (a.jtail == a.jx[:, 0]).all()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("duo", [0, 1])
def test_risk_does_not_depend_on_the_rollouts_layout(duo):
    _check_case(RC.reference("h6_p70"), ("duo", duo), options={"duo": duo})


@pytest.mark.parametrize("which", ["ties", "state_constr"])
def test_risk_special_cases(which):
    R = {"ties": RC.tie_case, "state_constr": RC.state_constr_case}[which]()
    got = _check_case(R, which)
    if which == "state_constr":
        assert (got.jx >= RC.reference("h6_p33")["want"]["jx"]).all() and (got.jx > RC.reference("h6_p33")["want"]["jx"]).any()


def test_risk_more_groups_than_halves():
    """P = 290: ten groups, so two halves of the workgroup walk two groups each, the slots take three group totals and the last group has two valid lanes"""
    T = TC.reference("h6_p33")
    cfg = T["cfg"].replace(num_particles=290)
    x0, xref, noise, u = __import__("cases").asymmetric_problem(cfg, RC.B, seed=11)
    R = RC._finish(RC._rolled(cfg, T["model"], x0, u, xref, noise))
    _check_case(R, "P = 290")


@pytest.mark.parametrize("name", ["h6_p33", "h6_p130"])
def test_all_four_centre_modes(name):
    R = RC.reference(name)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=RC.B)
    args = (R["x0"], R["u"], R["xref"], R["noise"])
    try:
        none = S.risk(*args, **_kw(R, None))
        rows = S.risk(*args, **_kw(R, "rows"))
        xref = S.risk(*args, **_kw(R, "xref"))
        mean = S.risk(*args, **_kw(R, "mean"))
        tube_mean = S.tube(*args).mean
        via_tube = S.risk(*args, **_kw(R, tube_mean))
        unbounded = S.risk(*args, tail=R["tail_k"], quantiles=RC.QUANTILES, want_particles=True)
    finally:
        S.close()
    _same(none, RC.want(R, None), (name, "mode 0"))
    _same(rows, R["want"], (name, "mode 1"))
    _same(xref, RC.want(R, R["xref"]), (name, "mode 2"))
    _same(mean, R["want"], (name, "mode 3"))                   # the tensor's own mean is the oracle's mean trajectory (SPEC.md §12)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(mean, via_tube))
    assert (none.first_exit[:, 0] == R["cfg"].num_particles).all() and not np.array_equal(xref.first_exit, rows.first_exit)
    assert unbounded.exit is None and unbounded.first_exit is None and unbounded.outside_any is None
    _same(unbounded, RC.want(R, None, None, None), (name, "no bounds"))


def test_risk_keys_equals_risk_on_the_drawn_noise():
    R = RC.reference("h6_p33")
    keys = np.stack([prng.split(np.array([0, 77 + b], np.uint32), 2)[1] for b in range(RC.B)]).astype(np.uint32)
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=RC.B)
    noise = S.noise_from_keys(keys)
    kw = _kw(R, "mean")
    a = S.risk_keys(R["x0"], R["u"], R["xref"], keys, **kw)
    b = S.risk(R["x0"], R["u"], R["xref"], noise, **kw)
    S.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert (a.jstat[:, 1] > 0).all() and not np.array_equal(a.jx, R["want"]["jx"])
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


def _rollout_dev(S, R, B, store_traj=True):
    """stages the first B instances and runs rollout_dev on the current torch stream; returns what must stay alive"""
    import torch
    dev = [torch.from_numpy(np.array(a[:B])).cuda() for a in (R["x0"], R["u"], R["xref"], S.noise_to_device_layout(R["noise"][:B]))]
    cost = torch.zeros(B, dtype=torch.float32, device="cuda")
    xmean = torch.zeros((B, S.H + 1, 13), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    S.rollout_dev(B, *[d.data_ptr() for d in dev], cost.data_ptr(), xmean.data_ptr(), store_traj, st)
    return dev, cost, xmean, st


_SHAPES = lambda B, P, H, Q: {"exit": ((B, P), np.uint32), "jx": ((B, P), np.float32), "first_exit": ((B, H + 2), np.uint32), "outside_any": ((B, H + 1), np.uint32),
                              "jstat": ((B, 4), np.float32), "jq": ((B, Q), np.float32), "jtail": ((B,), np.float32)}


def _risk_dev_guarded(S, R, B, keep, what, only=RR.OUTPUTS, centre="rows"):
    import torch
    dev, _, _, st = keep
    shapes = _SHAPES(B, S.P, S.H, len(RC.QUANTILES))
    bufs = {k: Guarded(shapes[k][0]) for k in only}
    lo, hi = (torch.from_numpy(np.array(R[k][:B])).cuda() for k in ("lo", "hi"))
    rows = torch.from_numpy(np.array(R["xmean"][:B])).cuda()
    torch.cuda.current_stream().synchronize()
    S.risk_dev(B, xref=dev[2].data_ptr(), lo=lo.data_ptr(), hi=hi.data_ptr(), centre=rows.data_ptr() if centre == "rows" else centre, tail=R["tail_k"],
               quantiles=RC.QUANTILES, stream=st, **{k: b.ptr for k, b in bufs.items()})
    torch.cuda.synchronize()
    return {k: (bufs[k].result((what, k), shapes[k][1]) if k in bufs else None) for k in RR.OUTPUTS}


@pytest.mark.parametrize("name", ["h6_p33", "h6_p130"])
def test_risk_dev_after_a_rollout_between_guard_words(name):
    R = RC.reference(name)
    want = R["want"]
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=RC.B)
    keep = _rollout_dev(S, R, RC.B)
    _same(_risk_dev_guarded(S, R, RC.B, keep, name), want, name)
    _same(_risk_dev_guarded(S, R, RC.B, keep, (name, "mean"), centre="mean"), want, (name, "mean"))
    # fewer instances than the workspace holds: fine; some outputs only: the others are not computed and nothing else is touched
    part = _risk_dev_guarded(S, R, 2, keep, (name, "first two"))
    _same(part, {k: v[:2] for k, v in want.items()}, (name, "first two"))
    for only in (("first_exit",), ("jtail",), ("jq", "outside_any"), ("exit", "jstat")):
        got = _risk_dev_guarded(S, R, RC.B, keep, (name, only), only=only)
        for k in only:
            assert RR.outputs_differ({o: got[o] if o == k else None for o in RR.OUTPUTS}, {o: want[o] if o == k else None for o in RR.OUTPUTS}) == 0, (only, k)
    S.close()


def test_risk_dev_is_refused_when_the_workspace_holds_no_such_rollout():
    import torch
    R = RC.reference("h6_p33")
    S = SdeMpcSolver(R["cfg"], R["model"], max_batch=RC.B)
    buf = torch.zeros((RC.B, 4), dtype=torch.float32, device="cuda")
    xr = torch.from_numpy(np.array(R["xref"])).cuda()
    call = lambda B, st=0: S.risk_dev(B, xref=xr.data_ptr(), jstat=buf.data_ptr(), stream=st)
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(RC.B)
    keep = _rollout_dev(S, R, RC.B, store_traj=False)
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(RC.B)
    keep = _rollout_dev(S, R, 2)
    torch.cuda.synchronize()
    with pytest.raises(SdempcError, match="holds fewer instances"):
        call(RC.B)
    call(2, keep[3])
    torch.cuda.synchronize()
    assert bits_differ(buf.cpu().numpy()[:2], R["want"]["jstat"][:2]) == 0
    S.grad(R["x0"], R["u"], R["xref"], R["noise"])
    with pytest.raises(SdempcError, match="holds no rollout"):
        call(2)
    with pytest.raises(SdempcError, match="need bounds"):
        S.risk_dev(2, xref=xr.data_ptr(), first_exit=buf.data_ptr())
    S.close()


@pytest.mark.parametrize("name", ["h6_p1", "h6_p33", "h6_p70", "h6_p130"])
def test_risk_on_a_poisoned_handle(name):
    """SDEMPC_OPT_TEST_WS_FILL = 255: every float-valued device word the handle allocates starts as a NaN pattern — the padded lanes of the tensor among them (the
    rollout does not write them) and the risk staging rows. Same bits: the padded lanes are masked and no unwritten word is read."""
    R = RC.reference(name)
    _check_case(R, (name, "poisoned"), options={"test_ws_fill": 255})
    _check_case(R, (name, "poisoned", "mean"), options={"test_ws_fill": 255}, centre="mean")


def test_one_non_finite_instance_stays_alone():
    N, R = RC.nonfinite_case(), RC.reference("h6_p33")
    P = 33
    got = _check_case(N, "non-finite instance")
    assert got.first_exit[1, 0] == P and (got.outside_any[1] == P).all() and np.isnan(got.jq[1]).all() and np.isnan(got.jtail[1])
    for b in (0, 2):
        assert all(np.asarray(getattr(got, k))[b].tobytes() == R["want"][k][b].tobytes() for k in RR.OUTPUTS), b


def test_several_workgroups_per_launch():
    """B = 300 at P = 1, H = 6: 300 workgroups, instance indices far past one workgroup's; against risk_ref of the call's own tensor and, for three instances, of
    the oracle's"""
    R = RC.reference("h6_p1")
    cfg, model = R["cfg"], R["model"]
    Bn = 300
    rng = np.random.default_rng(5)
    x0 = np.tile(R["x0"], (Bn // RC.B, 1))
    x0[:, :6] += rng.normal(0, 0.2, (Bn, 6)).astype(np.float32)
    u, xref, noise = (np.tile(R[k], (Bn // RC.B,) + (1,) * (R[k].ndim - 1)) for k in ("u", "xref", "noise"))
    centre = np.repeat(x0[:, None, :], cfg.horizon + 1, axis=1)                   # the box sits on the deviation from the initial state ...
    w = (0.002 * 1.03 ** np.arange(Bn)).astype(np.float32)                       # ... and is another one per instance: every exit step occurs
    lo = np.full((Bn, 13), -np.inf, np.float32)
    lo[:, :6] = -w[:, None]
    hi = -lo
    S = SdeMpcSolver(cfg, model, max_batch=Bn)
    got = S.risk(x0, u, xref, noise, lo=lo, hi=hi, centre=centre, tail=1, quantiles=RC.QUANTILES, want_particles=True)
    _, traj, _ = S.rollout(x0, u, xref, noise, True, True)
    S.close()
    _same(got, RR.risk(traj, cfg, model, xref, lo, hi, centre, R["ranks"], 1), "B = 300")
    assert len(np.unique(got.exit)) >= 6 and (got.first_exit.sum(axis=1) == 1).all()
    O = orc.Oracle(cfg, model)
    for b in (0, 149, 299):
        _, t, _ = O.rollout(x0[b], u[b], xref[b], noise[b], True, True)
        assert bits_differ(traj[b], t) == 0, b


@pytest.mark.parametrize("name", ["h6_p33", "h6_p130", "h7_m6_p33"])
def test_anchor_against_the_rollouts_own_cost(name):
    """With every cost term but the tracking cost switched off, the mean of Jx IS the rollout's cost: the restated stage cost against the rollout kernels' own"""
    R = RC.anchor_case(name)
    got = _check_case(R, (name, "anchor"))
    assert got.jstat[:, 0].tobytes() == got.cost.tobytes()


def _m_inputs(prob, x, rng, uopt):
    """what m_risk hands the solver: the state in the solver's frame, the plan, the reference window, the noise drawn from the solve's key"""
    from sde4mbrl_px4_amd.sde_mpc_design import _next_key
    from sde4mbrl_px4_amd.utils import enu2ned
    x = np.asarray(x, np.float32)
    xs = enu2ned(x, np) if prob.convert_to_enu else x
    _, sub = _next_key(rng)
    u = np.asarray(uopt, np.float32).reshape(prob.cfg.horizon, prob.cfg.num_motors)
    noise = prob.solver().noise_from_keys(np.asarray(sub, np.uint32)[None])[0]
    return xs, u, prob.xref(0.0, x), noise


@pytest.mark.parametrize("enu", [False, True])
def test_m_risk_is_the_risk_of_m_mpcs_plan(enu):
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    R = RC.reference("h6_p33")
    prob = MpcProblem(R["cfg"].replace(max_iter=4, max_no_improvement_iter=4), R["model"], convert_to_enu=enu)
    x = R["x0"][0]
    rng = np.array([0, 42], np.uint32)
    st = prob.m_reset(x, rng, x)
    uopt, st2, new_rng, xevol = prob.m_mpc(x, rng, st, curr_t=0.0, xdes=x)
    lo, hi = np.full(13, -np.inf, np.float32), np.full(13, np.inf, np.float32)
    lo[[0, 1, 2]], hi[[0, 1, 2]] = -0.02, 0.02
    r = prob.m_risk(x, rng, np.asarray(uopt), curr_t=0.0, xdes=x, lo=lo, hi=hi, centre="mean", tail=0.1, quantiles=(0.5, 0.9), want_particles=True)
    xs, u, xref, noise = _m_inputs(prob, x, rng, uopt)
    _, tensor, xmean = prob.solver().rollout(xs[None], u[None], xref[None], noise[None], True, True)
    prob.solver().close()
    mean = enu2ned(xmean[0], np) if enu else xmean[0]
    assert np.asarray(xevol).tobytes() == np.asarray(mean, np.float32).tobytes()           # the plan m_mpc returned, on the noise it was solved on
    want = RR.risk(tensor, prob.cfg, R["model"], xref[None], lo[None], hi[None], xmean, (16, 29), 4)
    _same({k: getattr(r, k)[None] for k in RR.OUTPUTS}, want, ("m_risk", enu))
    assert r.P == 33 and r.exit.shape == (33,) and r.first_exit.shape == (prob.cfg.horizon + 2,) and r.cost.shape == ()
    assert r.first_exit.sum() == 33 and float(r.p_ever) == 1.0 - r.first_exit[-1] / 33 and float(st2.num_steps) >= 1
