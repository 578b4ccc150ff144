"""A handle's results depend on the call alone, not on the handle's past (include/sdempc.h: layout, batch position and options "never change a
bit of any result"). Every other GPU parity file runs a fresh handle whose buffers come zeroed from their first hipMalloc and fit the batch
exactly; here one handle lives through a script of calls — batches that vary, options changed on the live handle, diverged instances that leave
NaN / inf in the rows the next call reuses — with SDEMPC_OPT_TEST_WS_FILL = 0xFF (every float-valued device buffer starts as NaN patterns) and
without; caller-owned device buffers sit between guard words and start as a sentinel; first calls arrive on non-blocking streams and two
handles run at once. Every comparison is bit for bit against the CPU oracle (tests/handle_state_cases.py holds the inputs and the oracle
results, tests/test_handle_state_cpu.py the conditions: the poison diverges, everything else is finite, the sentinel is no result)."""
import functools

import numpy as np
import pytest

import handle_state_cases as hs
import kernel_census as kc
import orc
from cases import bits_differ
from sde4mbrl_px4_amd import prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu

FILLS = [255, -1]


def _same(got, want, what):
    assert len(got) >= len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if np.asarray(w).dtype == np.uint32:
            assert np.array_equal(g, w), (what, k)
            continue
        d = bits_differ(g, w)
        if d:
            ga, wa = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(w, np.float32)
            bad = np.argwhere((ga.view(np.uint32) != wa.view(np.uint32)) & ~(np.isnan(ga) & np.isnan(wa)))
            raise AssertionError(f"{what}: output {k}: {d} words differ, first at index {bad[0].tolist()}: got {ga[tuple(bad[0])]!r}, want {wa[tuple(bad[0])]!r}")


# ---- A. one handle, a scripted life ---------------------------------------------------------------------------------------------------------
def _life_call(S, kind, inputs):
    x0, xref, nz, u, s = inputs
    if kind in ("solve", "poison"):
        return S.solve(x0, xref, nz, u, s)
    if kind == "solve_keys":
        return S.solve_keys(x0, xref, nz, u, s)
    if kind == "rollout":
        return S.rollout(x0, u, xref, nz, True, True)
    if kind == "grad":
        return S.grad(x0, u, xref, nz)
    return S.closed_loop(x0, xref[None], nz, hs.LOOP_T, u_init=u, stepsize_in=s)


@functools.lru_cache(maxsize=None)
def _fresh_handle_results(mlp, math):
    """The calls of the script with more than 8 instances, each on a handle of its own with that call's options and nothing before it."""
    cfg, model = hs.cfg_for(hs.LIFE_P, mlp, math), synthetic_iris()
    out, opts = {}, {}
    for i, (kind, B, o, _, _) in enumerate(hs.LIFE):
        opts.update(o)
        if B > 8:
            S = SdeMpcSolver(cfg, model, max_batch=B, options=opts)
            out[i] = _life_call(S, kind, hs.life_inputs(cfg, i))
            S.close()
    return out


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("mlp,math", hs.ARITH)
def test_scripted_life_of_one_handle(mlp, math, fill):
    cfg, model = hs.cfg_for(hs.LIFE_P, mlp, math), synthetic_iris()
    ref = hs.life_reference(mlp, math)
    fresh = _fresh_handle_results(mlp, math)
    S = SdeMpcSolver(cfg, model, max_batch=hs.LIFE_MAX_BATCH, options={"test_ws_fill": fill})
    assert S.get_option("test_ws_fill") == fill and not S.device_ready()
    for i, (kind, B, opts, seed, marker) in enumerate(hs.LIFE):
        for k, v in opts.items():
            S.set_option(k, v)                                  # on the live handle
        got = _life_call(S, kind, hs.life_inputs(cfg, i))
        what = (i, kind, B)
        if mlp == "f32" and marker is not None:
            assert kc.normalise(S.last_kernel_name()) == (_kernel(marker, B, hs.LIFE_P, S), math), (what, S.last_kernel_name())
        S.solve_status()
        idx, want = ref[i]
        _same(tuple(np.asarray(g)[idx] for g in got), want, what)
        if B > 8:
            _same(got, fresh[i], (what, "against a fresh handle"))
        if kind == "poison":
            assert not np.isfinite(got[2][:, [3, 5, 6]]).all(axis=1).any(), what       # every instance did diverge
        else:
            assert all(np.isfinite(np.asarray(g, np.float64)).all() for g in got), what
    assert S.layout_fallbacks() == 0
    S.close()


# ---- B. caller-owned device buffers: guard | payload | guard, all prefilled with the sentinel ---------------------------------------------
class Guarded:
    """An output of n float32 words inside one torch allocation; ptr points at the payload. The prefill runs on torch's current stream: sync
    waits for it, because a call that is given stream 0 runs on the handle's own non-blocking stream; callers that launch on the very stream
    the buffer was made on pass sync=False."""

    def __init__(self, shape, sync=True):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.t = torch.full((self.n + 2 * hs.GUARD,), hs.SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * hs.GUARD
        if sync:
            torch.cuda.current_stream().synchronize()

    def result(self, what, may_keep_sentinel=False):
        """After synchronisation: guards untouched, no payload word still the sentinel; the payload as float32."""
        w = self.t.cpu().numpy().view(np.uint32)
        lo, pay, hi = w[:hs.GUARD], w[hs.GUARD:hs.GUARD + self.n], w[hs.GUARD + self.n:]
        assert (lo == hs.SENTINEL).all(), (what, "write in front of the buffer", np.flatnonzero(lo != hs.SENTINEL)[:4] - hs.GUARD)
        assert (hi == hs.SENTINEL).all(), (what, "write behind the buffer", np.flatnonzero(hi != hs.SENTINEL)[:4])
        if not may_keep_sentinel:
            assert not (pay == hs.SENTINEL).any(), (what, "words never written", np.flatnonzero(pay == hs.SENTINEL)[:4])
        return pay.view(np.float32).reshape(self.shape).copy()


class Inputs:
    """Device copies of the inputs of a call; unchanged() compares them with what was uploaded, bit for bit."""

    def __init__(self, **arrays):
        import torch
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in self.host.items()}

    def __getitem__(self, k):
        return self.dev[k].data_ptr()

    def unchanged(self, what):
        for k, v in self.host.items():
            assert self.dev[k].cpu().numpy().tobytes() == v.tobytes(), (what, "input written in place", k)


def _sync():
    import torch
    torch.cuda.synchronize()


def _stream0():
    import torch
    return torch.cuda.current_stream().cuda_stream


# name -> (P, handle options, the normalised kernel name)
DEV_LAYOUTS = {
    "lane": (1, dict(coop=0), "sdempc_solve_kernel<TeamWave, 4, 0, false, 1, false>"),
    "spec": (33, dict(), hs.SPEC),
    "coop": (33, dict(spec=0), hs.COOP),
    "tile": (33, dict(lane=0, coop=0), "sdempc_solve_kernel<TeamBlock, 4, 0, false, 0, false>"),
    "duo": (70, dict(coop=0, pk=0, duo=1), "sdempc_solve_kernel<TeamPairT<2>, 4, 0, false, 3, false>"),
}


def _kernel(marker, B, P, S):
    """{pk} of a cooperative kernel's name: launch_coop_m's choice for this batch on this device"""
    return marker.format(pk="true" if B * ((P + 3) // 4) <= S.get_option("device_cus") else "false")


def _solve_dev_guarded(S, B, prob, noise_dev_host, stream=None, what=None):
    x0, xref, _, u, s = prob
    H, m = S.H, S.m
    inp = Inputs(x0=x0[:B], xref=xref[:B], noise=noise_dev_host[:B], u=u[:B], s=s[:B])
    uopt, xevol, info = Guarded((B, H, m)), Guarded((B, H + 1, 13)), Guarded((B, 8))
    S.solve_dev(B, inp["x0"], inp["xref"], inp["noise"], inp["u"], inp["s"], uopt.ptr, xevol.ptr, info.ptr, _stream0() if stream is None else stream)
    _sync()
    S.solve_status()
    out = uopt.result((what, "uopt")), xevol.result((what, "xevol")), info.result((what, "info"))
    inp.unchanged(what)
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("layout", list(DEV_LAYOUTS))
def test_solve_dev_stays_inside_its_buffers(layout, B):
    P, opts, marker = DEV_LAYOUTS[layout]
    cfg, model, prob, ref = hs.small_reference(P)
    S = SdeMpcSolver(cfg, model, max_batch=8, options={"test_ws_fill": 255, **opts})
    got = _solve_dev_guarded(S, B, prob, S.noise_to_device_layout(prob[2]), what=(layout, B))
    assert kc.normalise(S.last_kernel_name()) == (_kernel(marker, B, P, S), "exact"), S.last_kernel_name()
    _same(got, tuple(a[:B] for a in ref["solve"]), (layout, B))
    S.close()


def test_solve_dev_at_the_ticketed_batch_size():
    """B = 4,700 at P = 40, two iterations: a persistent launch that hands its instances out by ticket. Every instance equals two striped
    launches of the same handle; the first, the last and three drawn ones equal the oracle; nothing outside [B] is written, nothing inside is left."""
    cfg = hs.cfg_for(40, max_iter=2, max_no_improvement_iter=2, num_short_dt=10)
    model = synthetic_iris()
    B, P = 4700, 40
    x0 = W.random_initial_states(B, 70)
    xref = np.stack([W.reference_window(0.05 * (b % 160), cfg.time_steps) for b in range(B)]).astype(np.float32)
    keys = prng.split(prng.PRNGKey(11), B)
    S = SdeMpcSolver(cfg, model, max_batch=B, options={"test_ws_fill": 255})
    yk, i0 = S.reset()
    u = np.tile(yk[None], (B, 1, 1))
    s = np.full(B, i0["stepsize"], np.float32)
    nz = Guarded((B, S.lib.sdempc_noise_dev_floats(S._h, 1)))
    S.noise_from_keys_dev(keys, nz.ptr, _stream0())
    _sync()
    noise_dev = nz.result("noise_from_keys_dev")
    got = _solve_dev_guarded(S, B, (x0, xref, None, u, s), noise_dev, what="ticketed")
    assert ", false, 3, " in S.last_kernel_name() and 3 * 6 * S.get_option("device_cus") <= B          # persistent, ticketed
    half = B // 2
    assert half < 3 * 6 * S.get_option("device_cus")                                                    # striped
    for sl in (slice(0, half), slice(half, B)):
        part = _solve_dev_guarded(S, half, (x0[sl], xref[sl], None, u[sl], s[sl]), noise_dev[sl], what=("striped", sl.start))
        _same(tuple(g[sl] for g in got), part, ("ticketed against striped", sl.start))
    O = orc.Oracle(cfg, model)
    for b in hs.sample_of(B, 5):
        _same(tuple(g[b] for g in got), O.solve(x0[b], xref[b], orc.noise_from_key(keys[b], P, hs.H), u[b], float(s[b]))[:3], ("ticketed against the oracle", b))
    S.close()


@pytest.mark.parametrize("P", [33, 70])
def test_rollout_dev_and_grad_dev_stay_inside_their_buffers(P):
    cfg, model, prob, ref = hs.small_reference(P)
    x0, xref, noise, u, _ = prob
    B, H, m = 3, cfg.horizon, cfg.num_motors
    S = SdeMpcSolver(cfg, model, max_batch=8, options={"test_ws_fill": 255})
    inp = Inputs(x0=x0, xref=xref, noise=S.noise_to_device_layout(noise), u=u)
    c_ref, _, xm_ref = ref["rollout"]
    for with_mean in (True, False):
        cost, xmean = Guarded((B,)), Guarded((B, H + 1, 13))
        S.rollout_dev(B, inp["x0"], inp["u"], inp["xref"], inp["noise"], cost.ptr, xmean.ptr if with_mean else None, False, _stream0())
        _sync()
        _same((cost.result(("rollout", with_mean)),), (c_ref,), ("rollout cost", P, with_mean))
        if with_mean:
            _same((xmean.result("xmean"),), (xm_ref,), ("rollout xmean", P))
        else:
            assert hs.holds_sentinel(xmean.result("xmean not asked for", may_keep_sentinel=True)) == xmean.n      # untouched
    cost, grad = Guarded((B,)), Guarded((B, H, m))
    S.grad_dev(B, inp["x0"], inp["u"], inp["xref"], inp["noise"], cost.ptr, grad.ptr, _stream0())
    _sync()
    _same((cost.result("grad cost"), grad.result("grad")), ref["grad"], ("grad", P))
    inp.unchanged(("rollout / grad", P))
    S.close()


@pytest.mark.parametrize("P", [1, 31, 33, 70])
def test_noise_conversions_write_every_word_and_zero_the_padded_lanes(P):
    cfg, model = hs.cfg_for(P), synthetic_iris()
    B, G = 3, (P + 31) // 32
    keys = np.stack([prng.PRNGKey(40 + b) for b in range(B)])
    canon = np.stack([orc.noise_from_key(k, P, hs.H) for k in keys])
    S = SdeMpcSolver(cfg, model, max_batch=8, options={"test_ws_fill": 255})
    want = S.noise_to_device_layout(canon)                      # host conversion: padded lanes are zeros
    assert want.shape == (B, G, hs.H, 6, 32) and not any(want[:, g, :, :, max(0, P - 32 * g):].any() for g in range(G))
    a = Guarded(want.shape)
    S.noise_from_keys_dev(keys, a.ptr, _stream0())
    inp = Inputs(canon=canon)
    b = Guarded(want.shape)
    S.noise_to_device_layout_dev(B, inp["canon"], b.ptr, _stream0())
    _sync()
    _same((a.result(("noise_from_keys_dev", P)), b.result(("noise_to_device_layout_dev", P))), (want, want), ("noise", P))
    inp.unchanged(("noise_to_device_layout_dev", P))
    # a smaller batch than max_batch, on a handle whose staging buffers have seen the larger one
    got = S.noise_from_keys(keys[:2])
    _same((got,), (canon[:2],), ("noise_from_keys", P))
    S.close()


@pytest.mark.parametrize("fill", FILLS)
def test_traj_to_canonical_dev_after_a_diverged_solve_of_a_larger_batch(fill):
    """The trajectory workspace is zeroed when it is allocated; nothing may need that. The handle's previous call left NaN / inf in all eight
    rows; the rollout then stores three."""
    P = 70
    cfg, model, prob, ref = hs.small_reference(P)
    x0, xref, noise, u, _ = prob
    B, H = 3, cfg.horizon
    S = SdeMpcSolver(cfg, model, max_batch=8, options={"test_ws_fill": fill, "coop": 0})
    px0, pxref, pnoise, pu, ps = hs.poison_problem(cfg, 8, 300)
    bad = S.solve(px0, pxref, pnoise, pu, ps)
    assert not np.isfinite(bad[2][:, [3, 5, 6]]).all(axis=1).any()
    inp = Inputs(x0=x0, xref=xref, noise=S.noise_to_device_layout(noise), u=u)
    cost, traj = Guarded((B,)), Guarded((B, P, H + 1, 13))
    S.rollout_dev(B, inp["x0"], inp["u"], inp["xref"], inp["noise"], cost.ptr, None, True, _stream0())
    S.traj_to_canonical_dev(B, traj.ptr, _stream0())
    _sync()
    c_ref, t_ref, _ = ref["rollout"]
    _same((cost.result("cost"), traj.result("traj")), (c_ref, t_ref), "rollout with store_traj after a diverged solve")
    inp.unchanged("traj")
    S.close()


# ---- C. streams ---------------------------------------------------------------------------------------------------------------------------
def _pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


@pytest.mark.parametrize("fill", FILLS)
def test_first_device_call_on_a_non_blocking_stream(fill):
    """The handle's first device call is solve_dev on a caller's non-blocking stream, inputs uploaded on that stream, no host synchronisation
    before the launch; grad_dev at a larger batch follows on the same stream without one either (the workspaces are reallocated under it)."""
    import torch
    P = 33
    cfg, model, prob, ref = hs.small_reference(P)
    cfg8, _, prob8, ref8 = hs.small_reference(P, seed=17, B=8)
    S = SdeMpcSolver(cfg, model, max_batch=8, options={"test_ws_fill": fill, "coop": 0})
    nd3, nd8 = S.noise_to_device_layout(prob[2]), S.noise_to_device_layout(prob8[2])         # host-only conversions
    assert not S.device_ready()
    H, m = cfg.horizon, cfg.num_motors
    host = [_pinned(a) for a in (prob[0], prob[1], nd3, prob[3], prob[4], prob8[0], prob8[1], nd8, prob8[3])]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dev = [h.to("cuda", non_blocking=True) for h in host]
        uopt, xevol, info = Guarded((3, H, m), False), Guarded((3, H + 1, 13), False), Guarded((3, 8), False)
        cost, grad = Guarded((8,), False), Guarded((8, H, m), False)
        x0, xref, nz, u, s, x0b, xrefb, nzb, ub = [d.data_ptr() for d in dev]
        S.solve_dev(3, x0, xref, nz, u, s, uopt.ptr, xevol.ptr, info.ptr, st.cuda_stream)
        S.grad_dev(8, x0b, ub, xrefb, nzb, cost.ptr, grad.ptr, st.cuda_stream)
    st.synchronize()
    S.solve_status()
    _same((uopt.result("uopt"), xevol.result("xevol"), info.result("info")), ref["solve"], "first call on a stream")
    _same((cost.result("cost"), grad.result("grad")), ref8["grad"], "grad_dev behind it, larger batch")
    for d, h in zip(dev, host):
        assert d.cpu().numpy().tobytes() == h.numpy().tobytes()
    S.close()


def _solve_on(S, st, prob, nd):
    """Enqueue one solve of prob on stream st; returns the guarded outputs (and keeps the inputs alive)."""
    import torch
    x0, xref, _, u, s = prob
    B, H, m = x0.shape[0], S.H, S.m
    with torch.cuda.stream(st):
        dev = [_pinned(a).to("cuda", non_blocking=True) for a in (x0, xref, nd, u, s)]
        out = Guarded((B, H, m), False), Guarded((B, H + 1, 13), False), Guarded((B, 8), False)
        S.solve_dev(B, *[d.data_ptr() for d in dev], out[0].ptr, out[1].ptr, out[2].ptr, st.cuda_stream)
    return out, dev


def test_work_counters_reset_between_solves_on_a_stream():
    import torch
    P = 33
    cfg, model, prob, ref = hs.small_reference(P)
    _, _, prob2, ref2 = hs.small_reference(P, seed=27)
    st = torch.cuda.Stream()
    counters = []
    for fresh in (False, True):
        S = SdeMpcSolver(cfg, model, max_batch=3, options={"coop": 0})          # (the tile layouts count their work)
        if not fresh:
            o1, keep1 = _solve_on(S, st, prob, S.noise_to_device_layout(prob[2]))
            st.synchronize()
            _same(tuple(o.result("first") for o in o1), ref["solve"], "first solve")
            first = S.work_counters(reset=True)
            assert first[0] == 3 and first[2] == int(ref["solve"][2][:, 7].sum()) + 2 * 3
        o2, keep2 = _solve_on(S, st, prob2, S.noise_to_device_layout(prob2[2]))
        st.synchronize()
        S.solve_status()
        info = o2[2].result("info")
        _same((o2[0].result("uopt"), o2[1].result("xevol"), info), ref2["solve"], ("second solve", fresh))
        solves, grads, fwd = S.work_counters()
        assert solves == 3 and fwd == int(info[:, 7].sum()) + 2 * 3 and 3 <= grads <= int(info[:, 2].sum())
        counters.append((solves, grads, fwd))
        S.close()
    assert counters[0] == counters[1]


def test_two_handles_in_flight_on_their_own_streams():
    """P = 33 and P = 70, cooperative layouts off (they assume an otherwise idle device): three solves each, enqueued alternately without a host
    synchronisation; all six equal the oracle."""
    import torch
    cases = [[hs.small_reference(P, seed=sd) for sd in (7, 17, 27)] for P in (33, 70)]
    handles = [SdeMpcSolver(c[0][0], c[0][1], max_batch=3, options={"coop": 0}) for c in cases]
    nds = [[S.noise_to_device_layout(r[2][2]) for r in c] for S, c in zip(handles, cases)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = []
    for k in range(3):
        for j in range(2):
            pending.append((j, k, _solve_on(handles[j], streams[j], cases[j][k][2], nds[j][k])))
    for st in streams:
        st.synchronize()
    for j, k, (out, _) in pending:
        _same(tuple(o.result((j, k)) for o in out), cases[j][k][3]["solve"], ("handle", j, "solve", k))
    for S in handles:
        S.solve_status()
        assert S.work_counters()[0] == 9
        S.close()
