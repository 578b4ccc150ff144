"""Closed loop with a scenario (SPEC.md §11c) without a GPU: the CPU reference of tests/scenario_loop_ref.py against timed_loop_ref with both
schedules absent, the one-row schedule, the key schedule, the statement about zero rows, every refusal of sdempc_closed_loop_batch_scenario (no
HIP call may happen before them), the Python surface's own checks, header / binding / option 14, simulate's frame conversion, and the
discrimination of three wrong loops on the inputs the GPU tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cases import ROOT, bits_differ
from scenario_cases import ALPHA, B5, S3, SCHEDULE, T7, disturbance, episodes, motor_state, perturbed_plants, small_cfg
from scenario_loop_ref import MUTANTS, gust, scenario_loop_ref
from sde4mbrl_px4_amd import _abi, prng, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdempcError, SdeMpcSolver
from timed_loop_ref import num_solves, timed_loop_ref


def test_abi_surface_of_the_scenario_entry_point_and_option_14():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_scenario_cfg \{[^}]*struct_size;[^}]*\*\s*dist;[^}]*dist_ticks;[^}]*dist_batch;[^}]*plant_ticks;[^}]*\}", hdr)
    assert C.sizeof(_abi.SdempcScenarioCfg) == 32 and _abi.SdempcScenarioCfg.dist.offset == 8 and _abi.SdempcScenarioCfg.plant_ticks.offset == 24
    assert "sdempc_closed_loop_batch_scenario" in _abi.EXPORTED_SYMBOLS
    lib = _abi.load_library()
    fn = _abi.scenario_entry(lib)
    assert len(fn.argtypes) == len(_abi.timed_entry(lib).argtypes) + 1 and fn.restype is C.c_int
    # option 14: header, binding, default, validation; host-only
    assert int(re.search(r"#define SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES (\d+)", hdr).group(1)) == _abi.OPTIONS["test_loop_chunk_bytes"] == 14
    assert "SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES" in hdr.split("#define SDEMPC_OPT_LANE")[0]             # documented in the table
    S = SdeMpcSolver(small_cfg(), synthetic_iris(), max_batch=1)
    assert S.get_option("test_loop_chunk_bytes") == -1
    for v in (0, 1, 4096, 2**31 - 1, -1):
        S.set_option("test_loop_chunk_bytes", v)
        assert S.get_option("test_loop_chunk_bytes") == v
    with pytest.raises(SdempcError):
        S.set_option("test_loop_chunk_bytes", -2)
    assert not S.device_ready()
    S.close()


@pytest.mark.parametrize("n", [1, 3])
def test_reference_without_schedules_is_the_timed_loop(n):
    cfg = small_cfg()
    model = synthetic_iris()
    B, T = 2, 5
    x0, xref, keys = episodes(cfg, B, 20)
    pl = perturbed_plants(model, 2)
    kw = dict(S=2, D=n + 1, alpha=ALPHA, substeps=n, u_act_in=motor_state(B, 4))
    want = timed_loop_ref(cfg, model, pl, x0, xref, keys, T, **kw)
    got = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T, **kw)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    # a 2-D plant_of with one row is the 1-D plant_of
    of = np.array([1, 0], np.int32)
    a = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T, plant_of=of, **kw)
    b = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T, plant_of=of[None], **kw)
    c = timed_loop_ref(cfg, model, pl, x0, xref, keys, T, plant_of=of, **kw)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    # either schedule changes the states and leaves the key schedule alone
    w = disturbance(T, B)
    sched = np.array([[0, 1], [0, 1], [1, 1], [1, 0], [0, 0]], np.int32)
    for extra in (dict(disturbance=w), dict(plant_of=sched), dict(disturbance=w, plant_of=sched)):
        r = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T, **{**kw, **extra})
        assert bits_differ(r[0], got[0]) > 0 and np.array_equal(r[5], got[5]) and r[2].shape == (B, num_solves(T, 2), 8)


def test_zero_rows_change_nothing_but_the_sign_of_a_zero():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((200, 13)).astype(np.float32)
    x[0, 3], x[0, 11], x[1, 5] = -0.0, -0.0, 0.0
    for zero in (np.zeros(6, np.float32), -np.zeros(6, np.float32)):
        for row in x:
            y = gust(row, zero, np.float32(0.0033333))
            assert bits_differ(y[[0, 1, 2, 6, 7, 8, 9]], row[[0, 1, 2, 6, 7, 8, 9]]) == 0                 # position and attitude: untouched, always
            moved = [i for i in (3, 4, 5, 10, 11, 12) if y[i].tobytes() != row[i].tobytes()]
            assert all(row[i] == 0 and np.signbit(row[i]) and not np.signbit(y[i]) for i in moved)       # only -0 -> +0
    # a loop with an all-zero schedule is the loop without one wherever no velocity component is a negative zero
    cfg = small_cfg(num_particles=1, max_iter=1, max_no_improvement_iter=1)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, 1, 7)
    a = scenario_loop_ref(cfg, model, None, x0, xref, keys, 3, S=2, substeps=2)
    b = scenario_loop_ref(cfg, model, None, x0, xref, keys, 3, S=2, substeps=2, disturbance=np.zeros(6, np.float32))
    for p, q in zip(a, b):
        assert p.tobytes() == q.tobytes()


def test_gust_is_one_fma_per_component():
    rng = np.random.default_rng(3)
    x = rng.uniform(-2.0, 2.0, (3000, 13)).astype(np.float32)
    w = rng.uniform(-4.0, 4.0, (3000, 6)).astype(np.float32)
    dt = np.float32(np.float32(0.01) / np.float32(3))
    got = np.stack([gust(a, b, dt) for a, b in zip(x, w)])
    idx = [3, 4, 5, 10, 11, 12]
    p = w.astype(np.float64) * np.float64(dt)                              # exact in float64
    s = p + x[:, idx].astype(np.float64)
    t = s - p
    exact = ((p - (s - t)) + (x[:, idx].astype(np.float64) - t)) == 0.0   # two-sum: where the float64 addition is exact, one rounding of s is the fma
    assert exact.sum() > 100
    assert got[:, idx][exact].tobytes() == s[exact].astype(np.float32).tobytes()
    two = (p.astype(np.float32) + x[:, idx]).astype(np.float32)
    assert (got[:, idx] != two).any()                                     # an fma, not a rounded product and a rounded sum


@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_loops_differ_on_the_gpu_tests_inputs(mutant):
    """The inputs of test_both_schedules_in_every_arithmetic (n = 3, so dt_p != dt_0; plants whose sigma differ): each wrong loop leaves the
    right one's bits, so the GPU's bit-for-bit agreement with the right one says which of the two the kernel is."""
    cfg = small_cfg()
    model = synthetic_iris()
    n = 3
    x0, xref, keys = episodes(cfg, B5, 44)
    pl = perturbed_plants(model, 3)
    assert all(bits_differ(pl[0].sigma, p.sigma) == 6 for p in pl[1:])
    kw = dict(S=S3, D=n + 1, alpha=ALPHA, substeps=n, plant_of=SCHEDULE, disturbance=disturbance(T7, B5), u_act_in=motor_state(B5, 4), episodes=[1, 3])
    right = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T7, **kw)
    wrong = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T7, mutant=mutant, **kw)
    for b in (1, 3):                 # episode 1 switches on every tick, episode 3 once, at a period start
        assert bits_differ(right[0][b], wrong[0][b]) > 0, (mutant, b)
    assert np.array_equal(right[5], wrong[5])


class _Call:
    """ctypes buffers of one sdempc_closed_loop_batch_scenario call; every field can be overridden."""

    def __init__(self, cfg, B=4, T=7):
        self.B, self.T, self.H, self.m = B, T, cfg.horizon, cfg.num_motors

    def __call__(self, lib, h, blobs, S=3, D=0, alpha=0.0, s_size=None, null_scenario=False, dist=None, dist_ticks=1, dist_batch=1, plant_ticks=1,
                 t_size=None, substeps=2, num_plants=None, xref_solves=1, plant_of=None, B=None, T=None):
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        B = self.B if B is None else B
        T = self.T if T is None else T
        Tb = max(T, 1)
        Ns = num_solves(Tb, max(S, 1))
        x0 = np.zeros((B, 13), np.float32); x0[:, 6] = 1.0
        xref = np.zeros((max(xref_solves, 1), 1, self.H + 1, 13), np.float32); xref[..., 6] = 1.0
        keys = np.zeros((B, 2), np.uint32)
        xs = np.zeros((B, Tb + 1, 13), np.float32)
        us = np.zeros((B, Tb, self.m), np.float32)
        info = np.zeros((B, Ns, 8), np.float32)
        d = None if dist is None else np.ascontiguousarray(dist, np.float32)
        sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg) if s_size is None else s_size, None if d is None else d.ctypes.data_as(fp),
                                    dist_ticks, dist_batch, plant_ticks)
        tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg) if t_size is None else t_size, S, D, alpha)
        Np = len(blobs) if num_plants is None else num_plants
        pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), Np, substeps, 0.0, -1, -1)
        bufs = (C.c_char_p * max(len(blobs), 1))(*blobs)
        sz = (C.c_size_t * max(len(blobs), 1))(*[len(b) for b in blobs])
        of = None if plant_of is None else np.ascontiguousarray(plant_of, np.int32)
        return _abi.scenario_entry(lib)(
            h, None if null_scenario else C.byref(sc), C.byref(tc), C.byref(pc), C.cast(bufs, C.POINTER(C.c_void_p)), sz,
            None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)), B, T, x0.ctypes.data_as(fp), xref.ctypes.data_as(fp), xref_solves, 1,
            keys.ctypes.data_as(u32p), None, None, None, xs.ctypes.data_as(fp), us.ctypes.data_as(fp), info.ctypes.data_as(C.POINTER(_abi.SdempcInfo)),
            None, None, None, None)


def test_scenario_argument_checks_make_no_hip_call():
    import torch
    lib = _abi.load_library()
    cfg = small_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    hexa = synthetic_hexa().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EBLOB, EDEVICE, ECAPACITY = -1, -2, -3, -5
    B, T = 4, 7
    ok_w = np.zeros((T, B, 6), np.float32)
    bad = {name: ok_w.copy() for name in ("nan", "inf", "ninf")}
    bad["nan"][6, 3, 5], bad["inf"][0, 0, 0], bad["ninf"][3, 1, 2] = np.nan, np.inf, -np.inf
    sched = np.zeros((T, B), np.int32)
    try:
        call = _Call(cfg, B, T)               # S = 3 (Ns = 3), n = 2
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(s_size=24), EINVAL, "struct_size"),
            (dict(null_scenario=True), EINVAL, "struct_size"),
            (dict(dist=ok_w, dist_ticks=3, dist_batch=B), EINVAL, "dist_ticks"),          # Ns, not T
            (dict(dist=ok_w, dist_ticks=0, dist_batch=B), EINVAL, "dist_ticks"),
            (dict(dist=ok_w, dist_ticks=T, dist_batch=2), EINVAL, "dist_batch"),
            (dict(dist=ok_w, dist_ticks=T, dist_batch=0), EINVAL, "dist_batch"),
            (dict(dist=bad["nan"], dist_ticks=T, dist_batch=B), EINVAL, "non-finite"),
            (dict(dist=bad["inf"], dist_ticks=T, dist_batch=B), EINVAL, "non-finite"),
            (dict(dist=bad["ninf"], dist_ticks=T, dist_batch=B), EINVAL, "non-finite"),
            (dict(plant_ticks=3, plant_of=sched), EINVAL, "plant_ticks"),                  # Ns, not T
            (dict(plant_ticks=0, plant_of=sched), EINVAL, "plant_ticks"),
            (dict(plant_ticks=T), EINVAL, "plant_of"),                                     # a schedule needs its indices
            (dict(plant_ticks=T, plant_of=np.where(np.arange(T * B).reshape(T, B) == 27, 1, 0), blobs=[blob]), EINVAL, "index"),      # last row, last episode
            (dict(plant_ticks=T, plant_of=sched - (np.arange(T * B).reshape(T, B) == 9), blobs=[blob, blob]), EINVAL, "index"),
            (dict(plant_ticks=T, plant_of=sched, blobs=[blob] * 2, num_plants=T * B + 1), EINVAL, "num_plants"),
            (dict(blobs=[blob] * 2, num_plants=B + 1, plant_of=np.zeros(B, np.int32)), EINVAL, "num_plants"),                          # Tp = 1: today's bound
            (dict(num_plants=0), EINVAL, "num_plants"),
            (dict(blobs=[blob, blob]), EINVAL, "plant_of"),                                # where §11a refuses a NULL plant_of
            # ... and everything the timed entry point refuses
            (dict(t_size=12), EINVAL, "struct_size"),
            (dict(S=0), EINVAL, "solve_period"),
            (dict(D=7), EINVAL, "solve_delay"),
            (dict(alpha=float("nan")), EINVAL, "lag_alpha"),
            (dict(xref_solves=7), EINVAL, "xref_solves"),
            (dict(T=0), EINVAL, "T must"),
            (dict(B=5), ECAPACITY, "max_batch"),
            (dict(substeps=0), EINVAL, "substeps"),
            (dict(blobs=[blob[:-4]]), EBLOB, "too small"),
            (dict(blobs=[hexa]), EINVAL, "num_motors"),
        ]
        for kw, want, word in cases:
            kw = {"blobs": [blob], **kw}
            rc = call(lib, h, **kw)
            msg = lib.sdempc_last_error(h).decode()
            assert rc == want, (sorted(kw), rc, msg)
            assert word in msg, (word, msg)
            assert lib.sdempc_device_ready(h) == 0
        # valid arguments reach the device: every shape of either schedule, more plants than episodes, NULL schedules
        ok = 0 if torch.cuda.is_available() else EDEVICE
        many = np.arange(T * B, dtype=np.int32).reshape(T, B) % 6
        for kw in (dict(), dict(dist=ok_w[:1, :1]), dict(dist=ok_w, dist_ticks=T, dist_batch=B), dict(dist=ok_w[:, :1], dist_ticks=T),
                   dict(plant_ticks=T, plant_of=many, blobs=[blob] * 6), dict(plant_ticks=T, plant_of=sched, dist=ok_w[:1], dist_batch=B, D=6, alpha=1.0)):
            rc = call(lib, h, **{"blobs": [blob], **kw})
            assert rc == ok, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


class _Recording:
    """A view of the loaded library that records which attributes are looked up."""

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, name):
        self.seen.append(name)
        return getattr(self._lib, name)


def test_only_a_scenario_resolves_the_scenario_symbol():
    cfg = small_cfg(max_iter=1, max_no_improvement_iter=1, num_particles=1)
    model = synthetic_iris()
    S = SdeMpcSolver(cfg, model, max_batch=2)
    S.lib = _Recording(S.lib)
    x0, xref, keys = episodes(cfg, 2, 3)
    for kw, n_out in ((dict(), 6), (dict(plant=[model, model], plant_of=np.array([1, 0])), 6), (dict(solve_period=2, plant=model, disturbance=None), 7)):
        try:
            assert len(S.closed_loop(x0, xref, keys, 2, **kw)) == n_out
        except SdempcError:
            pass                                                   # (no GPU: the call itself is refused by the device, after the dispatch)
    assert "sdempc_closed_loop_batch_scenario" not in S.lib.seen
    for kw in (dict(disturbance=np.zeros(6, np.float32)), dict(plant=[model, model], plant_of=np.array([[1, 0], [0, 0]]))):
        S.lib.seen.clear()
        try:
            out = S.closed_loop(x0, xref, keys, 2, **kw)
            assert len(out) == 7 and out[2].shape == (2, 2, 8)
        except SdempcError:
            pass
        assert "sdempc_closed_loop_batch_scenario" in S.lib.seen
    S.lib = S.lib._lib
    S.close()


def test_python_surface_checks_the_scenario_keywords():
    cfg = small_cfg()
    model = synthetic_iris()
    B, T = 3, 4
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), np.float32)
    xref = np.zeros((cfg.horizon + 1, 13), np.float32)
    k = np.zeros((B, 2), np.uint32)
    nan = np.zeros((T, 6), np.float32); nan[2, 1] = np.nan
    for kw in (dict(disturbance=np.zeros((B, 6), np.float32)),                       # [B][6] is not accepted: it cannot be told from [T][6]
               dict(disturbance=np.zeros(5, np.float32)), dict(disturbance=np.zeros((T, B, 5), np.float32)), dict(disturbance=np.zeros((2, B, 6), np.float32)),
               dict(disturbance=np.zeros((T, 2, 6), np.float32)), dict(disturbance=np.zeros((1, T, B, 6), np.float32)), dict(disturbance=nan),
               dict(disturbance=np.full(6, np.inf, np.float32)),
               dict(plant=[model] * 2, plant_of=np.zeros((2, B), np.int32)), dict(plant=[model] * 2, plant_of=np.zeros((T, 2), np.int32)),
               dict(plant_of=np.zeros((T, B), np.int32)),                             # a schedule names members of a plant set
               dict(disturbance=np.zeros(6, np.float32), solve_period=2, solve_delay=3)):       # the timing checks still apply
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    assert not S.device_ready()
    S.close()


def test_simulate_takes_the_disturbance_in_the_frame_of_x():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.utils import enu2ned
    cfg = small_cfg(num_particles=1)
    model = synthetic_iris()
    T = 5
    w = disturbance(T, 1)[:, 0]
    of = np.array([0, 0, 1, 1, 0], np.int32)

    class Spy:
        def closed_loop(self, x0, xref, keys, T, **kw):
            self.kw = kw
            B = x0.shape[0]
            return (np.zeros((B, T + 1, 13), np.float32), np.zeros((B, T, 4), np.float32), np.zeros((B, 3, 8), np.float32), np.zeros((B, 4, 4), np.float32),
                    np.zeros(B, np.float32), np.zeros((B, 2), np.uint32), np.zeros((B, 4), np.float32))

    x = W.random_initial_states(1, 80)[0]
    for enu in (True, False):
        prob = MpcProblem(cfg=cfg, model=model, convert_to_enu=enu)
        spy = Spy()
        prob.solver = lambda spy=spy: spy
        prob.simulate(x, prng.PRNGKey(1), T, plant=[model, model], solve_period=2, disturbance=w, plant_of=of)
        got = spy.kw["disturbance"]
        assert got.shape == (T, 6) and got.dtype == np.float32 and spy.kw["plant_of"].shape == (T, 1) and np.array_equal(spy.kw["plant_of"][:, 0], of)
        if not enu:
            assert got.tobytes() == w.tobytes()
            continue
        # the vector rules of enu2ned, exact in float32: what enu2ned itself does to a velocity and a body rate
        probe = np.zeros((T, 13), np.float32); probe[:, 6] = 1.0
        probe[:, 3:6], probe[:, 10:13] = w[:, :3], w[:, 3:]
        flipped = enu2ned(probe, np)
        assert got[:, :3].tobytes() == flipped[:, 3:6].tobytes() and got[:, 3:].tobytes() == flipped[:, 10:13].tobytes()
        assert got[:, 0].tobytes() == w[:, 1].tobytes() and got[:, 2].tobytes() == (-w[:, 2]).tobytes() and got[:, 4].tobytes() == (-w[:, 4]).tobytes()
        # a constant row converts the same way
        prob.simulate(x, prng.PRNGKey(1), T, disturbance=w[0])
        assert spy.kw["disturbance"].tobytes() == got[0].tobytes() and spy.kw["plant_of"] is None
    with pytest.raises(ValueError):
        MpcProblem(cfg=cfg, model=model).simulate(x, prng.PRNGKey(1), T, disturbance=np.zeros((T + 1, 6), np.float32))
    with pytest.raises(ValueError):
        MpcProblem(cfg=cfg, model=model).simulate(x, prng.PRNGKey(1), T, plant=[model, model], plant_of=np.zeros((T, 1), np.int32))
