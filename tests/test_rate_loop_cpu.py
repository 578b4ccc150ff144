"""Closed loop through the rate-setpoint interface (SPEC.md §11d) without a GPU: header / binding / library agree on the new symbol at ABI version 3, every
refusal of sdempc_closed_loop_batch_rate (no HIP call may happen before them) and of the Python surface, the routing of closed_loop (rate_loop=None never
touches the new symbol; rate_loop=... hands it the expected struct), the reference of tests/rate_loop_ref.py against scenario_loop_ref with the rate loop
absent, the discrimination of six wrong loops, the census of the shared cases, the tie to the node's post-processing (tests/worker.py), the
sign of RotorSDEModel.rate_mixer() and a closed-loop check that the rate loop does reject a disturbance between solves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
from cases import CDIR, ROOT, asymmetric_cfg, asymmetric_model, bits_differ
from closed_loop_ref import oracle_for
from rate_loop_cases import ALPHA, B5, S3, T7, disturbance, episodes, motor_state, perturbed_plants, rate_loop, ref_cases, small_cfg
from rate_loop_ref import MUTANTS, rate_loop_ref, thrust_setpoint
from scenario_loop_ref import scenario_loop_ref
from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import RateLoop, SdempcError, SdeMpcSolver
from timed_loop_ref import num_solves

F = np.float32


def test_abi_surface_of_the_rate_entry_point():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_rate_cfg \{[^}]*struct_size;[^}]*kp\[3\];[^}]*ki_dt\[3\];[^}]*integ_limit\[3\];[^}]*"
                     r"mixer\[SDEMPC_MAX_MOTORS\]\[3\];[^}]*motor_weight;[^}]*inv_m;[^}]*\}", hdr)
    R = _abi.SdempcRateCfg
    assert C.sizeof(R) == 4 * (1 + 9 + 24 + 2) and R.kp.offset == 4 and R.ki_dt.offset == 16 and R.integ_limit.offset == 28 and R.mixer.offset == 40
    assert R.motor_weight.offset == 136 and R.inv_m.offset == 140
    assert "sdempc_closed_loop_batch_rate" in _abi.EXPORTED_SYMBOLS and "int sdempc_closed_loop_batch_rate(" in hdr
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, "sdempc_closed_loop_batch_rate")
    fn = _abi.rate_entry(lib)
    assert len(fn.argtypes) == len(_abi.scenario_entry(lib).argtypes) + 6 and fn.restype is C.c_int
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint sdempc_closed_loop_batch_rate\([^{]*\{\n\s*return guarded\(", src)


class _Call:
    """ctypes buffers of one sdempc_closed_loop_batch_rate call; every field can be overridden."""

    def __init__(self, cfg, B=4, T=7):
        self.B, self.T, self.H, self.m = B, T, cfg.horizon, cfg.num_motors

    def __call__(self, lib, h, blobs, S=3, D=0, alpha=0.0, r_size=None, null_rate=False, kp=(0.1, 0.1, 0.1), ki_dt=(0.0, 0.0, 0.0), limit=(0.1, 0.1, 0.1),
                 mixer=None, weight=0.0, inv_m=0.0, null_ws=False, null_xs=False, scenario=None, s_size=None, dist=None, dist_ticks=1, dist_batch=1,
                 plant_ticks=1, t_size=None, substeps=2, num_plants=None, xref_solves=1, plant_of=None, B=None, T=None, tail=True):
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        B = self.B if B is None else B
        T = self.T if T is None else T
        Tb = max(T, 1)
        Ns = num_solves(Tb, max(S, 1))
        x0 = np.zeros((B, 13), F); x0[:, 6] = 1.0
        xref = np.zeros((max(xref_solves, 1), 1, self.H + 1, 13), F); xref[..., 6] = 1.0
        keys = np.zeros((B, 2), np.uint32)
        xs, us, info = np.zeros((B, Tb + 1, 13), F), np.zeros((B, Tb, self.m), F), np.zeros((B, Ns, 8), F)
        ws, gn, tn = np.zeros((B, Tb, 4), F), np.zeros((B, 3), F), np.zeros((B, self.H, 3), F)
        rc = _abi.SdempcRateCfg()
        rc.struct_size = C.sizeof(rc) if r_size is None else r_size
        mx = np.zeros((_abi.MAX_MOTORS, 3), F) if mixer is None else np.asarray(mixer, F)
        for a in range(3):
            rc.kp[a], rc.ki_dt[a], rc.integ_limit[a] = kp[a], ki_dt[a], limit[a]
            for l in range(_abi.MAX_MOTORS):
                rc.mixer[l][a] = mx[l, a]
        rc.motor_weight, rc.inv_m = weight, inv_m
        d = None if dist is None else np.ascontiguousarray(dist, F)
        use_sc = scenario if scenario is not None else (d is not None or plant_ticks != 1 or s_size is not None)
        sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg) if s_size is None else s_size, None if d is None else d.ctypes.data_as(fp),
                                    dist_ticks, dist_batch, plant_ticks)
        tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg) if t_size is None else t_size, S, D, alpha)
        Np = len(blobs) if num_plants is None else num_plants
        pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), Np, substeps, 0.0, -1, -1)
        bufs = (C.c_char_p * max(len(blobs), 1))(*blobs)
        sz = (C.c_size_t * max(len(blobs), 1))(*[len(b) for b in blobs])
        of = None if plant_of is None else np.ascontiguousarray(plant_of, np.int32)
        return _abi.rate_entry(lib)(
            h, None if null_rate else C.byref(rc), C.byref(sc) if use_sc else None, C.byref(tc), C.byref(pc), C.cast(bufs, C.POINTER(C.c_void_p)), sz,
            None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)), B, T, x0.ctypes.data_as(fp), xref.ctypes.data_as(fp), xref_solves, 1,
            keys.ctypes.data_as(u32p), None, None, None, None if null_xs else xs.ctypes.data_as(fp), us.ctypes.data_as(fp),
            info.ctypes.data_as(C.POINTER(_abi.SdempcInfo)), None, None, None, None, None, None,
            None if null_ws else ws.ctypes.data_as(fp), gn.ctypes.data_as(fp) if tail else None, tn.ctypes.data_as(fp) if tail else None)


def test_rate_argument_checks_make_no_hip_call():
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
    nan, inf = float("nan"), float("inf")
    ok_m = np.zeros((8, 3), F)
    bad_m = ok_m.copy(); bad_m[3, 2] = np.nan
    far_m = ok_m.copy(); far_m[4, 0] = np.nan                 # a row beyond the handle's four motors is not looked at
    ok_w = np.zeros((T, B, 6), F)
    bad_w = ok_w.copy(); bad_w[2, 1, 3] = np.inf
    sched = np.zeros((T, B), np.int32)
    try:
        call = _Call(cfg, B, T)               # S = 3 (Ns = 3), n = 2
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(r_size=140), EINVAL, "struct_size"),
            (dict(null_rate=True), EINVAL, "struct_size"),
            (dict(kp=(0.1, nan, 0.1)), EINVAL, "non-finite gain"),
            (dict(kp=(inf, 0.1, 0.1)), EINVAL, "non-finite gain"),
            (dict(ki_dt=(0.0, 0.0, -inf)), EINVAL, "non-finite gain"),
            (dict(limit=(0.1, 0.1, nan)), EINVAL, "non-finite limit"),
            (dict(limit=(inf, 0.1, 0.1)), EINVAL, "non-finite limit"),
            (dict(limit=(0.1, -1e-6, 0.1)), EINVAL, "integ_limit must be >= 0"),
            (dict(mixer=bad_m), EINVAL, "mixer"),
            (dict(weight=-0.01), EINVAL, "motor_weight"),
            (dict(weight=1.01), EINVAL, "motor_weight"),
            (dict(weight=nan), EINVAL, "motor_weight"),
            (dict(inv_m=0.2), EINVAL, "inv_m"),
            (dict(null_ws=True), EINVAL, "ws is NULL"),
            (dict(null_xs=True), EINVAL, "NULL host pointer"),
            # ... and everything the scenario entry point refuses
            (dict(s_size=24), EINVAL, "struct_size"),
            (dict(dist=ok_w, dist_ticks=3, dist_batch=B), EINVAL, "dist_ticks"),
            (dict(dist=ok_w, dist_ticks=T, dist_batch=2), EINVAL, "dist_batch"),
            (dict(dist=bad_w, dist_ticks=T, dist_batch=B), EINVAL, "non-finite"),
            (dict(plant_ticks=3, plant_of=sched), EINVAL, "plant_ticks"),
            (dict(plant_ticks=T), EINVAL, "plant_of"),
            (dict(plant_ticks=T, plant_of=np.where(np.arange(T * B).reshape(T, B) == 27, 1, 0), blobs=[blob]), EINVAL, "index"),
            (dict(num_plants=0), EINVAL, "num_plants"),
            (dict(blobs=[blob, blob]), EINVAL, "plant_of"),
            (dict(t_size=12), EINVAL, "struct_size"),
            (dict(S=0), EINVAL, "solve_period"),
            (dict(D=7), EINVAL, "solve_delay"),
            (dict(alpha=nan), EINVAL, "lag_alpha"),
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
        # valid arguments reach the device: no scenario at all, either schedule, zero limits, both ends of the blend, inv_m as the binding forms it, no *_next
        ok = 0 if torch.cuda.is_available() else EDEVICE
        for kw in (dict(), dict(scenario=True), dict(dist=ok_w, dist_ticks=T, dist_batch=B), dict(plant_ticks=T, plant_of=sched), dict(limit=(0.0, 0.0, 0.0)),
                   dict(weight=1.0, kp=(0.0, 0.0, 0.0)), dict(inv_m=float(F(1.0) / F(4.0)), mixer=far_m, D=6, alpha=1.0), dict(tail=False)):
            rc = call(lib, h, **{"blobs": [blob], **kw})
            assert rc == ok, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_checks_the_rate_keywords():
    cfg = small_cfg()
    model = synthetic_iris()
    B, T = 3, 4
    for bad in (dict(kp=[0.1, 0.1]), dict(kp=np.nan), dict(kp=0.1, ki=np.inf), dict(kp=0.1, integ_limit=-0.1), dict(kp=0.1, integ_limit=[0.1, np.nan, 0.1]),
                dict(kp=0.1, motor_weight=1.5), dict(kp=0.1, motor_weight=-0.1), dict(kp=0.1, motor_weight=np.nan), dict(kp=0.1, mixer=np.zeros((4, 2))),
                dict(kp=0.1, mixer=np.zeros((9, 3))), dict(kp=0.1, mixer=np.full((4, 3), np.inf))):
        with pytest.raises(ValueError):
            RateLoop(**bad)
    rl = RateLoop(kp=0.5, ki=2.0, integ_limit=0.1)
    assert rl.kp.tolist() == [0.5] * 3 and rl.ki.dtype == np.float32 and rl.integ_limit.shape == (3,) and rl.mixer is None and rl.motor_weight == 0.0
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    for kw in (dict(rate_integ_in=np.zeros((B, 3), F)), dict(rate_tail_in=np.zeros((B, cfg.horizon, 3), F)),       # ... need rate_loop
               dict(rate_loop=dict(kp=0.1)),                                                                       # not a RateLoop
               dict(rate_loop=rl, rate_integ_in=np.zeros((B, 2), F)), dict(rate_loop=rl, rate_tail_in=np.zeros((B, cfg.horizon + 1, 3), F)),
               dict(rate_loop=RateLoop(kp=0.1, mixer=np.zeros((6, 3), F))),                                         # a hexa's mixer on four motors
               dict(rate_loop=rl, solve_period=2, solve_delay=3),                                                   # the timing checks still apply
               dict(rate_loop=rl, disturbance=np.zeros((B, 6), F)), dict(rate_loop=rl, plant_of=np.zeros((T, B), np.int32))):
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    assert not S.device_ready()
    S.close()


class _Recording:
    """A view of the loaded library that records which attributes are looked up and captures the arguments of the rate entry point."""

    def __init__(self, lib):
        self._lib, self.seen, self.args = lib, [], None

    def __getattr__(self, name):
        self.seen.append(name)
        fn = getattr(self._lib, name)
        if name != "sdempc_closed_loop_batch_rate":
            return fn
        _abi.rate_entry(self._lib)                              # (prototype set on the real symbol)

        class Stub:
            argtypes, restype = fn.argtypes, fn.restype

            def __call__(stub, *a):
                rc = C.cast(a[1], C.POINTER(_abi.SdempcRateCfg)).contents
                self.args = (a, _abi.SdempcRateCfg.from_buffer_copy(rc))
                return fn(*a)
        return Stub()


def test_routing_and_struct_contents():
    cfg = small_cfg(max_iter=1, max_no_improvement_iter=1, num_particles=1)
    model = synthetic_iris()
    S = SdeMpcSolver(cfg, model, max_batch=2)
    S.lib = _Recording(S.lib)
    x0, xref, keys = episodes(cfg, 2, 3)
    # rate_loop=None: every existing route, and none of them looks the new symbol up
    for kw, n_out in ((dict(), 6), (dict(plant=[model, model], plant_of=np.array([1, 0])), 6), (dict(solve_period=2, plant=model), 7),
                      (dict(disturbance=np.zeros(6, F)), 7), (dict(plant=[model, model], plant_of=np.array([[1, 0], [0, 0]])), 7)):
        try:
            assert len(S.closed_loop(x0, xref, keys, 2, rate_loop=None, **kw)) == n_out
        except SdempcError:
            pass                                                   # (no GPU: the call itself is refused by the device, after the dispatch)
    assert "sdempc_closed_loop_batch_rate" not in S.lib.seen
    # rate_loop=...: the new symbol, whatever else is given, with the struct the SPEC names
    n, dt = 3, 0.004
    mx = np.arange(12, dtype=F).reshape(4, 3) / F(7)
    for rl, kw, dtp in ((RateLoop(kp=[0.1, 0.2, 0.3], ki=[1.5, 2.5, 3.5], integ_limit=[0.01, 0.02, 0.03], motor_weight=0.35), dict(plant_substeps=n),
                         F(F(cfg.time_steps[0]) / F(n))),
                        (RateLoop(kp=0.7, ki=0.3, integ_limit=0.5, mixer=mx, motor_weight=1.0), dict(plant=model, plant_dt=dt, disturbance=np.zeros(6, F)), F(dt))):
        S.lib.seen.clear()
        S.lib.args = None
        try:
            out = S.closed_loop(x0, xref, keys, 2, rate_loop=rl, **kw)
            assert len(out) == 10 and out[2].shape == (2, 2, 8) and out[7].shape == (2, 2, 4) and out[8].shape == (2, 3) and out[9].shape == (2, cfg.horizon, 3)
        except SdempcError:
            pass
        assert "sdempc_closed_loop_batch_rate" in S.lib.seen and "sdempc_closed_loop_batch_scenario" not in S.lib.seen
        a, rc = S.lib.args
        assert rc.struct_size == C.sizeof(_abi.SdempcRateCfg) == 144
        assert np.array(rc.kp[:], F).tobytes() == rl.kp.tobytes() and np.array(rc.integ_limit[:], F).tobytes() == rl.integ_limit.tobytes()
        assert np.array(rc.ki_dt[:], F).tobytes() == (rl.ki * dtp).astype(F).tobytes()          # float32(ki) * float32(dt_plant)
        assert F(rc.inv_m).tobytes() == F(F(1.0) / F(4.0)).tobytes() and F(rc.motor_weight).tobytes() == F(rl.motor_weight).tobytes()
        want_m = model.rate_mixer() if rl.mixer is None else rl.mixer
        got_m = np.array([[rc.mixer[l][k] for k in range(3)] for l in range(8)], F)
        assert got_m[:4].tobytes() == want_m.tobytes() and not got_m[4:].any()
        assert (a[2] is None) == ("disturbance" not in kw)                                     # no scenario: a NULL scenario cfg
    S.lib = S.lib._lib
    S.close()


def test_reference_without_a_rate_loop_is_the_scenario_loop():
    cfg = small_cfg()
    model = synthetic_iris()
    B, T, n = 2, 5, 3
    x0, xref, keys = episodes(cfg, B, 20)
    pl = perturbed_plants(model, 2)
    kw = dict(S=2, D=n + 1, alpha=ALPHA, substeps=n, u_act_in=motor_state(B, 4), disturbance=disturbance(T, B),
              plant_of=np.array([[0, 1], [0, 1], [1, 1], [1, 0], [0, 0]], np.int32))
    want = scenario_loop_ref(cfg, model, pl, x0, xref, keys, T, **kw)
    got = rate_loop_ref(cfg, model, pl, x0, xref, keys, T, rate_loop=None, **kw)
    assert len(got) == 7
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    # motor_weight = 1 with zero gains flies the motor rows: the scenario loop's seven outputs again, through the rate loop's own code path
    thru = rate_loop_ref(cfg, model, pl, x0, xref, keys, T, rate_loop=RateLoop(kp=0.0, motor_weight=1.0), **kw)
    assert len(thru) == 10
    for g, w in zip(thru[:7], want):
        assert g.tobytes() == w.tobytes()
    # ... and a rate loop that acts changes the states and leaves the key schedule alone
    act = rate_loop_ref(cfg, model, pl, x0, xref, keys, T, rate_loop=rate_loop("soft"), **kw)
    assert bits_differ(act[0], want[0]) > 0 and np.array_equal(act[5], want[5])


@pytest.fixture(scope="module")
def shared():
    """The right loop on the shared cases, computed once: {name: (outputs, census)}."""
    cfg = small_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 61)
    return cfg, model, x0, xref, keys, {name: rate_loop_ref(cfg, model, pl, x0, xref, keys, T7, census=True, **kw) for name, pl, kw in ref_cases()}


def test_census_of_the_shared_cases_reaches_every_class(shared):
    """In the reference alone: substeps with an input-bound clamp active, with an integrator clamp active and with neither all occur, so no parity case
    on these inputs can pass by never reaching a clamp (or by never leaving one)."""
    total = {k: sum(c[k] for _, c in shared[5].values()) for k in ("input", "integ", "free")}
    assert all(v > 0 for v in total.values()), total
    n_sub = B5 * T7 * 3                                  # every substep is counted: free, or in at least one of the two clamp classes
    for name, (_, c) in shared[5].items():
        assert c["free"] <= n_sub <= c["free"] + c["input"] + c["integ"] <= 2 * n_sub - c["free"], (name, c)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_loops_differ_on_the_shared_cases(shared, mutant):
    cfg, model, x0, xref, keys, right = shared
    eps = [1, 3]
    differ = 0
    for name, pl, kw in ref_cases():
        wrong = rate_loop_ref(cfg, model, pl, x0, xref, keys, T7, mutant=mutant, episodes=eps, **kw)
        differ += sum(bits_differ(r[eps], w[eps]) for r, w in zip(right[name][0], wrong))
        assert np.array_equal(right[name][0][5][eps], wrong[5][eps])           # the key schedule is S and T only
    assert differ > 0, mutant


def test_ws_rows_are_the_nodes_wopt_rows():
    """SURVEY row A8 for m = 4: what the node's worker makes of a solution (tests/worker.py, the statements marked :431 and :432) is, row r, the setpoint
    this loop flies in row r — bit for bit, the thrust included (a division by 4 and a multiplication by 0.25 are the same float32 operation)."""
    import inspect
    import worker
    src = inspect.getsource(worker.MpcWorker.step)
    lines = [ln.split("#")[0].strip() for ln in src.splitlines() if re.search(r"#\s*:43[12]\b", ln)]
    assert len(lines) == 2 and lines[0].startswith("thrust =") and lines[1].startswith("wopt =")
    cfg = small_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, 1, 62)
    T = S3 + 1                                       # tick S3 starts period 1: its row 0 is solve 1's
    out = rate_loop_ref(cfg, model, None, x0, xref, keys, T, rate_loop=rate_loop("soft"), S=S3, D=0, substeps=2)
    O = oracle_for(cfg, model)
    r1, sub = orc.split(keys[0], 2)
    uopt, evol, _, _ = O.solve(x0[0], xref[0, 0], orc.noise_from_key(sub, cfg.num_particles, cfg.horizon), np.tile(np.asarray(cfg.uref, F), (cfg.horizon, 1)),
                               F(cfg.ls_init_stepsize if cfg.ls_maxls > 0 else cfg.stepsize))
    env = dict(np=np, uopt=np.array(uopt), evol=np.asarray(evol))
    for ln in lines:
        exec(ln, env)
    wopt = env["wopt"]
    assert wopt.dtype == np.float32 and wopt.shape == (cfg.horizon, 4)
    for i in range(S3):                              # ticks 0 .. S - 1 fly rows 0 .. S - 1 of solve 0 (D = 0)
        assert out[7][0, i].tobytes() == wopt[min(i, cfg.horizon - 1)].tobytes(), i
    assert out[7][0, S3].tobytes() != wopt[0].tobytes()
    # the thrust of an odd motor count may differ from the division by one ulp, never more (stated in SPEC.md §11d)
    rng = np.random.default_rng(5)
    for m in (3, 5, 6, 7):
        u = rng.uniform(0.0, 1.0, (2000, m)).astype(F)
        mine = np.array([thrust_setpoint(r, F(F(1.0) / F(m))) for r in u])
        node = (np.sum(u, axis=1) / m).astype(F)
        ulp = np.abs(mine.view(np.int32).astype(np.int64) - node.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (m, ulp.max())


def _asym3():
    return asymmetric_cfg(3, horizon=4, num_short_dt=4, num_particles=1, max_iter=1, max_no_improvement_iter=1), asymmetric_model(3)


@pytest.mark.parametrize("vehicle", ["iris", "hexa", "asymmetric"])
def test_rate_mixer_sign(vehicle):
    """From hover with zero plant noise, one Oracle.step under hover + mixer . tau: a positive tau[a] must leave omega[a] ABOVE what the same step leaves
    under the hover command alone (tau = 0), for every axis. If this fails the helper's sign is wrong, not the test."""
    if vehicle == "iris":
        cfg, model = small_cfg(), synthetic_iris()
    elif vehicle == "hexa":
        cfg = load_mpc_config(os.path.join(CDIR, "c3_hexa_traj_h50_p256.yaml")).replace(horizon=4, num_short_dt=4, num_particles=1, max_iter=1, max_no_improvement_iter=1)
        model = synthetic_hexa()
    else:
        cfg, model = _asym3()
    m = cfg.num_motors
    M = model.rate_mixer()
    assert M.shape == (m, 3) and M.dtype == np.float32
    E = np.stack([model.rotor_y, -model.rotor_x, model.rotor_dir]).astype(np.float64)
    if m >= 4:
        assert np.allclose(E @ M.astype(np.float64), np.eye(3), atol=1e-5)          # a right inverse wherever the geometry has rank 3
    O = oracle_for(cfg, model)
    u0 = np.asarray(cfg.uref, F)[:m]
    base, _ = O.step(W.HOVER.copy(), u0, np.zeros(6, F), t=0)
    for a in range(3):
        tau = np.zeros(3, F); tau[a] = 0.05
        x, _ = O.step(W.HOVER.copy(), (u0 + M @ tau).astype(F), np.zeros(6, F), t=0)
        assert x[10 + a] > base[10 + a], (vehicle, a, x[10:13], base[10:13])


def test_the_rate_loop_closes_the_loop_between_solves():
    """A shared plant, zero plant noise (sigma = 0), S = 3, a constant angular-acceleration disturbance: with kp > 0 the body rates end closer to the
    setpoint in force than with kp = 0, where the vehicle flies the mean thrust open loop. Both sides come from the reference loop; strict inequality."""
    import dataclasses
    cfg = small_cfg()
    model = synthetic_iris()
    quiet = dataclasses.replace(model, sigma=np.zeros(6, F))
    x0, xref, keys = episodes(cfg, 1, 63)
    n, T = 3, 6
    w = np.array([0, 0, 0, 3.0, -2.0, 1.5], F)
    err = {}
    for kp in (0.0, 0.08):
        out = rate_loop_ref(cfg, model, quiet, x0, xref, keys, T, rate_loop=RateLoop(kp=kp), S=S3, D=0, substeps=n, disturbance=w)
        # the setpoint in force when the last tick started, against the rates the episode ended with
        err[kp] = float(np.abs(out[0][0, T, 10:13] - out[7][0, T - 1, 1:4]).max())
    assert err[0.08] < err[0.0], err
