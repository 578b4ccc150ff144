"""Closed loop with per-motor actuator faults and substep-resolution states (SPEC.md §11e) without a GPU: header / binding / library agree on the new symbol
at ABI version 3, every refusal of sdempc_closed_loop_batch_fault (no HIP call may happen before them) and of the Python surface, the routing of closed_loop
(fault=None with substep_states=False never touches the new symbol; every other combination calls only it), the reference of tests/fault_loop_ref.py against
rate_loop_ref with both additions absent, a census of the shared cases of tests/fault_cases.py (every state finite, the healthy episode untouched, every
faulted episode and its solves changed, a neutral schedule bit-identical to no schedule), the discrimination of four wrong loops, the tie between xsub and
xs, and the frame rule of MpcProblem.simulate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cases import ROOT, bits_differ
from fault_cases import B5, LOOPS, N3, S3, T7, episodes, faults, perturbed_plants, ref_kwargs, small_cfg
from fault_loop_ref import MUTANTS, fault_loop_ref
from rate_loop_cases import rate_loop
from rate_loop_ref import rate_loop_ref
from sde4mbrl_px4_amd import _abi, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import RateLoop, SdempcError, SdeMpcSolver, fault_schedule
from sde4mbrl_px4_amd.utils import enu2ned
from timed_loop_ref import num_solves

F = np.float32
NEW = "sdempc_closed_loop_batch_fault"


def test_abi_surface_of_the_fault_entry_point():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_fault_cfg \{[^}]*struct_size;[^}]*const float\* fault;[^}]*fault_ticks;[^}]*fault_batch;[^}]*\}", hdr)
    R = _abi.SdempcFaultCfg
    assert C.sizeof(R) == 24 and R.fault.offset == 8 and R.fault_ticks.offset == 16 and R.fault_batch.offset == 20
    assert NEW in _abi.EXPORTED_SYMBOLS and f"int {NEW}(" in hdr
    proto = re.search(r"int " + NEW + r"\((.*?)\);", hdr, re.S).group(1)
    assert re.search(r"sdempc_fault_cfg\* fault_cfg[^,]*,\s*const sdempc_rate_cfg\* rate[^,]*,\s*const sdempc_scenario_cfg\* scenario", proto)
    assert re.search(r"float\* rate_tail_next[^,]*,\s*float\* xsub[^,]*$", proto.strip())
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, NEW)
    fn = _abi.fault_entry(lib)
    assert len(fn.argtypes) == len(_abi.rate_entry(lib).argtypes) + 2 and fn.restype is C.c_int
    assert fn.argtypes[1]._type_ is _abi.SdempcFaultCfg and fn.argtypes[2]._type_ is _abi.SdempcRateCfg
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint " + NEW + r"\([^{]*\{\n\s*return guarded\(", src)


class _Call:
    """ctypes buffers of one sdempc_closed_loop_batch_fault call; every field can be overridden."""

    def __init__(self, cfg, B=4, T=7):
        self.B, self.T, self.H, self.m = B, T, cfg.horizon, cfg.num_motors

    def __call__(self, lib, h, blobs, fault="ok", f_size=None, fault_ticks=None, fault_batch=None, null_fc=False, xsub=True, rate=True, ws=None, gn=None, tn=None,
                 g_in=False, t_in=False, S=3, D=0, alpha=0.0, r_size=None, kp=(0.1, 0.1, 0.1), limit=(0.1, 0.1, 0.1), weight=0.0, inv_m=0.0, null_xs=False,
                 scenario=None, s_size=None, dist=None, dist_ticks=1, dist_batch=1, plant_ticks=1, t_size=None, substeps=2, num_plants=None, xref_solves=1,
                 plant_of=None, B=None, T=None):
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        B = self.B if B is None else B
        T = self.T if T is None else T
        Tb = max(T, 1)
        Ns = num_solves(Tb, max(S, 1))
        x0 = np.zeros((B, 13), F); x0[:, 6] = 1.0
        xref = np.zeros((max(xref_solves, 1), 1, self.H + 1, 13), F); xref[..., 6] = 1.0
        keys = np.zeros((B, 2), np.uint32)
        xs, us, info = np.zeros((B, Tb + 1, 13), F), np.zeros((B, Tb, self.m), F), np.zeros((B, Ns, 8), F)
        b_ws, b_gn, b_tn = np.zeros((B, Tb, 4), F), np.zeros((B, 3), F), np.zeros((B, self.H, 3), F)
        b_gi, b_ti = np.zeros((B, 3), F), np.zeros((B, self.H, 3), F)
        b_xsub = np.zeros((B, Tb * max(substeps, 1), 13), F)
        ws = rate if ws is None else ws                         # (the rate-only outputs follow `rate` unless stated)
        gn = rate if gn is None else gn
        tn = rate if tn is None else tn
        rc = _abi.SdempcRateCfg()
        rc.struct_size = C.sizeof(rc) if r_size is None else r_size
        for a in range(3):
            rc.kp[a], rc.ki_dt[a], rc.integ_limit[a] = kp[a], 0.0, limit[a]
        rc.motor_weight, rc.inv_m = weight, inv_m
        f = fault_schedule(Tb, B, self.m) if isinstance(fault, str) else (None if fault is None else np.ascontiguousarray(fault, F))
        fc = _abi.SdempcFaultCfg(C.sizeof(_abi.SdempcFaultCfg) if f_size is None else f_size, None if f is None else f.ctypes.data_as(fp),
                                 (1 if f is None else f.shape[0]) if fault_ticks is None else fault_ticks,
                                 (1 if f is None else f.shape[1]) if fault_batch is None else fault_batch)
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
        return _abi.fault_entry(lib)(
            h, None if null_fc else C.byref(fc), C.byref(rc) if rate else None, C.byref(sc) if use_sc else None, C.byref(tc), C.byref(pc),
            C.cast(bufs, C.POINTER(C.c_void_p)), sz, None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)), B, T, x0.ctypes.data_as(fp),
            xref.ctypes.data_as(fp), xref_solves, 1, keys.ctypes.data_as(u32p), None, None, None, None if null_xs else xs.ctypes.data_as(fp),
            us.ctypes.data_as(fp), info.ctypes.data_as(C.POINTER(_abi.SdempcInfo)), None, None, None, None,
            b_gi.ctypes.data_as(fp) if g_in else None, b_ti.ctypes.data_as(fp) if t_in else None, b_ws.ctypes.data_as(fp) if ws else None,
            b_gn.ctypes.data_as(fp) if gn else None, b_tn.ctypes.data_as(fp) if tn else None, b_xsub.ctypes.data_as(fp) if xsub else None)


def test_fault_argument_checks_make_no_hip_call():
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
    ok_f = fault_schedule(T, B, 4)
    nan_f = ok_f.copy(); nan_f[5, 2, 3, 0] = np.nan
    inf_f = ok_f.copy(); inf_f[6, 3, 3, 1] = -np.inf            # the very last entry
    ok_w = np.zeros((T, B, 6), F)
    bad_w = ok_w.copy(); bad_w[2, 1, 3] = np.inf
    sched = np.zeros((T, B), np.int32)
    try:
        call = _Call(cfg, B, T)               # S = 3 (Ns = 3), n = 2
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(f_size=20), EINVAL, "fault: struct_size"),
            (dict(f_size=20, fault=None), EINVAL, "fault: struct_size"),
            (dict(fault=ok_f[:3]), EINVAL, "fault_ticks"),
            (dict(fault=ok_f, fault_ticks=0), EINVAL, "fault_ticks"),
            (dict(fault=ok_f[:, :2]), EINVAL, "fault_batch"),
            (dict(fault=ok_f, fault_batch=B + 1), EINVAL, "fault_batch"),
            (dict(fault=nan_f), EINVAL, "non-finite"),
            (dict(fault=inf_f), EINVAL, "non-finite"),
            (dict(fault=inf_f[6:, 3:]), EINVAL, "non-finite"),
            # rate-only pointers without a rate cfg, one at a time
            (dict(rate=False, ws=True), EINVAL, "without a rate cfg"),
            (dict(rate=False, gn=True), EINVAL, "without a rate cfg"),
            (dict(rate=False, tn=True), EINVAL, "without a rate cfg"),
            (dict(rate=False, g_in=True), EINVAL, "without a rate cfg"),
            (dict(rate=False, t_in=True), EINVAL, "without a rate cfg"),
            # ... and everything the rate entry point refuses
            (dict(r_size=140), EINVAL, "struct_size"),
            (dict(kp=(0.1, nan, 0.1)), EINVAL, "non-finite gain"),
            (dict(limit=(inf, 0.1, 0.1)), EINVAL, "non-finite limit"),
            (dict(limit=(0.1, -1e-6, 0.1)), EINVAL, "integ_limit must be >= 0"),
            (dict(weight=1.01), EINVAL, "motor_weight"),
            (dict(inv_m=0.2), EINVAL, "inv_m"),
            (dict(ws=False), EINVAL, "ws is NULL"),
            (dict(null_xs=True), EINVAL, "NULL host pointer"),
            (dict(s_size=24), EINVAL, "struct_size"),
            (dict(rate=False, s_size=24), EINVAL, "struct_size"),
            (dict(dist=ok_w, dist_ticks=3, dist_batch=B), EINVAL, "dist_ticks"),
            (dict(dist=ok_w, dist_ticks=T, dist_batch=2), EINVAL, "dist_batch"),
            (dict(dist=bad_w, dist_ticks=T, dist_batch=B), EINVAL, "non-finite"),
            (dict(rate=False, dist=bad_w, dist_ticks=T, dist_batch=B), EINVAL, "non-finite"),
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
        # valid arguments reach the device: with and without rate / scenario / fault cfg / fault pointer / xsub, broadcast schedules, extreme but finite rows
        ok = 0 if torch.cuda.is_available() else EDEVICE
        big = ok_f.copy(); big[..., 0] = -3.0e38
        for kw in (dict(), dict(rate=False), dict(rate=False, scenario=True), dict(null_fc=True), dict(fault=None, fault_ticks=99, fault_batch=-1),
                   dict(xsub=False), dict(null_fc=True, xsub=False, rate=False), dict(fault=ok_f[:1]), dict(fault=ok_f[:, :1]), dict(fault=ok_f[:1, :1]),
                   dict(fault=big), dict(dist=ok_w, dist_ticks=T, dist_batch=B, plant_ticks=T, plant_of=sched, D=6, alpha=1.0)):
            rc = call(lib, h, **{"blobs": [blob], **kw})
            assert rc == ok, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_checks_the_fault_keywords():
    f = fault_schedule(7, 5, 4)
    assert f.shape == (7, 5, 4, 2) and f.dtype == np.float32 and (f[..., 0] == 1).all() and not f[..., 1].any()
    for word in ("dead", "effectiveness", "stuck", "bias"):
        assert word in fault_schedule.__doc__
    cfg = small_cfg()
    model = synthetic_iris()
    B, T = 3, 4
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    bad = fault_schedule(T, B, 4); bad[1, 2, 3, 1] = np.nan
    for kw in (dict(fault=fault_schedule(T, B, 6)), dict(fault=fault_schedule(T + 1, B, 4)), dict(fault=fault_schedule(T, 2, 4)), dict(fault=np.ones((B, 4, 2), F)),
               dict(fault=np.ones((4,), F)), dict(fault=np.ones((T, B, 4, 3), F)), dict(fault=bad),
               dict(fault=fault_schedule(T, B, 4), solve_period=2, solve_delay=3),                                   # the timing checks still apply
               dict(substep_states=True, rate_integ_in=np.zeros((B, 3), F)),                                         # ... and the rate loop's
               dict(substep_states=True, plant_dt=0.01)):                                                            # plant_* need plant=...
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    assert not S.device_ready()
    S.close()


class _Recording:
    """A view of the loaded library that records which closed-loop entry points are CALLED and captures the arguments of the new one."""

    def __init__(self, lib):
        self._lib, self.seen, self.called, self.args = lib, [], [], None

    def __getattr__(self, name):
        self.seen.append(name)
        fn = getattr(self._lib, name)
        if not name.startswith("sdempc_closed_loop_batch"):
            return fn
        note = self

        class Entry:
            def __call__(self, *a):
                note.called.append(name)
                if name == NEW:
                    fc = None if not a[1] else _abi.SdempcFaultCfg.from_buffer_copy(C.cast(a[1], C.POINTER(_abi.SdempcFaultCfg)).contents)
                    note.args = (a, fc)
                return fn(*a)

            def __getattr__(self, key):
                return getattr(fn, key)

            def __setattr__(self, key, value):
                setattr(fn, key, value)

        return Entry()


def test_routing_and_arguments():
    cfg = small_cfg(max_iter=1, max_no_improvement_iter=1, num_particles=1)
    model = synthetic_iris()
    S = SdeMpcSolver(cfg, model, max_batch=2)
    S.lib = _Recording(S.lib)
    x0, xref, keys = episodes(cfg, 2, 3)
    rl = RateLoop(kp=0.1)
    # fault=None, substep_states=False: every existing route, and none of them looks the new symbol up
    for kw, n_out in ((dict(), 6), (dict(plant=[model, model], plant_of=np.array([1, 0])), 6), (dict(solve_period=2, plant=model), 7),
                      (dict(disturbance=np.zeros(6, F)), 7), (dict(plant=[model, model], plant_of=np.array([[1, 0], [0, 0]])), 7), (dict(rate_loop=rl), 10)):
        try:
            assert len(S.closed_loop(x0, xref, keys, 2, fault=None, substep_states=False, **kw)) == n_out
        except SdempcError:
            pass                                                   # (no GPU: the call itself is refused by the device, after the dispatch)
    assert NEW not in S.lib.seen and len(S.lib.called) == 6
    # every other combination calls the new symbol and only it
    n = 3
    f4 = fault_schedule(2, 2, 4); f4[1, 0, 2] = (0.0, 0.0)
    for kw, n_out, f_shape, has_rate, has_sc in (
            (dict(fault=f4), 7, (2, 2), False, False),
            (dict(substep_states=True, plant_substeps=n), 8, None, False, False),
            (dict(fault=f4[1, 0], substep_states=True, plant_substeps=n, disturbance=np.zeros(6, F)), 8, (1, 1), False, True),
            (dict(fault=f4[:, 0], rate_loop=rl), 10, (2, 1), True, False),
            (dict(fault=f4[:1], substep_states=True, rate_loop=rl, plant=[model, model], plant_of=np.array([[1, 0], [0, 0]]), plant_substeps=n), 11, (1, 2), True, True)):
        S.lib.seen.clear(); S.lib.called.clear()
        S.lib.args = None
        try:
            out = S.closed_loop(x0, xref, keys, 2, **kw)
            assert len(out) == n_out
            if kw.get("substep_states"):
                assert out[-1].shape == (2, 2 * n, 13) and out[-1].dtype == np.float32
        except SdempcError:
            pass
        assert S.lib.called == [NEW], (sorted(kw), S.lib.called)
        a, fc = S.lib.args
        assert len(a) == 32
        assert (fc is None) == (f_shape is None)
        if fc is not None:
            assert fc.struct_size == C.sizeof(_abi.SdempcFaultCfg) == 24 and (fc.fault_ticks, fc.fault_batch) == f_shape
            got = np.ctypeslib.as_array(fc.fault, shape=f_shape + (4, 2))
            assert got.tobytes() == np.asarray(kw["fault"], F).tobytes()
        assert bool(a[2]) == has_rate and bool(a[3]) == has_sc
        assert all(bool(p) == has_rate for p in a[28:31])                                  # ws and the two rate outputs come with the rate cfg only
        assert not a[26] and not a[27]
        assert bool(a[31]) == bool(kw.get("substep_states"))
    S.lib = S.lib._lib
    S.close()


def test_reference_with_both_additions_absent_is_the_rate_loop_reference():
    cfg = small_cfg()
    model = synthetic_iris()
    B, T = 2, 4
    x0, xref, keys = episodes(cfg, B, 20)
    pl = perturbed_plants(model, 2)
    for name in (None, "soft"):
        kw = {k: (v[:T, :B] if k in ("plant_of", "disturbance") else v[:B] if k in ("u_act_in", "rate_tail_in") else v) for k, v in ref_kwargs(name).items()}
        kw["plant_of"] = kw["plant_of"] % 2
        want = rate_loop_ref(cfg, model, pl, x0, xref, keys, T, **kw)
        got = fault_loop_ref(cfg, model, pl, x0, xref, keys, T, fault=None, substep_states=False, **kw)
        assert len(got) == len(want) == (7 if name is None else 10)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        # ... and its own loop, asked for the substep states only, gives the same values and the record
        own = fault_loop_ref(cfg, model, pl, x0, xref, keys, T, substep_states=True, **kw)
        assert len(own) == len(want) + 1 and own[-1].shape == (B, T * N3, 13)
        for g, w in zip(own, want):
            assert g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def shared():
    """The right loop on the shared cases, computed once: {rate loop name: (healthy, faulted, neutral)}, each with the substep states."""
    cfg = small_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 81)
    pl = perturbed_plants(model, 3)
    runs = {}
    for name in LOOPS:
        kw = ref_kwargs(name)
        runs[name] = tuple(fault_loop_ref(cfg, model, pl, x0, xref, keys, T7, fault=f, substep_states=True, **kw)
                           for f in (None, faults(), fault_schedule(1, 1, 4)))
    return cfg, model, pl, x0, xref, keys, runs


@pytest.mark.parametrize("name", LOOPS, ids=[str(n) for n in LOOPS])
def test_census_of_the_shared_cases(shared, name):
    healthy, hit, neutral = shared[6][name]
    assert all(np.isfinite(v).all() for v in hit) and np.abs(hit[0]).max() < 10.0          # (the largest magnitude is a body rate of 6.45, without a rate loop)
    words = [bits_differ(hit[0][b], healthy[0][b]) for b in range(B5)]
    print("xs words that differ from the fault-free run, per episode:", name, words, "max |x|", float(np.abs(hit[0]).max()))
    assert words == [0, 65, 52, 78, 91], words                                              # every word of every row after the tick at which the fault sets in
    if name is None:
        assert 6.4 < np.abs(hit[0]).max() < 6.5 and np.abs(hit[0]).max() == np.abs(hit[0][1, :, 10:13]).max()        # a body rate of episode 1
    for v_h, v_f in zip(healthy, hit):                                                     # the healthy episode: every output, every bit
        assert v_h[0].tobytes() == v_f[0].tobytes()
    assert all(bits_differ(hit[2][b], healthy[2][b]) > 0 for b in range(1, B5))            # info: the solves react, through the state
    assert np.array_equal(hit[5], healthy[5])                                              # the key schedule is S and T only
    for v_h, v_n in zip(healthy, neutral):                                                 # a neutral schedule [1][1][m][2]: every bit
        assert v_h.tobytes() == v_n.tobytes()
    for run in (healthy, hit):                                                             # the last substep of a tick is the tick's state
        assert run[-1].shape == (B5, T7 * N3, 13) and run[-1][:, N3 - 1::N3].tobytes() == run[0][:, 1:].tobytes()
    assert bits_differ(hit[-1][:, 0::N3], hit[0][:, 1:]) > 0                               # ... and the first one is not
    # the fault leaves the motor state alone: episode 3's motor 1 is stuck at 0.9 on ticks 1 - 4, and us never shows 0.9
    assert not (hit[1][3, :, 1] == F(0.9)).any()


@pytest.mark.parametrize("name", LOOPS, ids=[str(n) for n in LOOPS])
@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_loops_differ_on_the_shared_cases(shared, mutant, name):
    cfg, model, pl, x0, xref, keys, runs = shared
    eps = [3, 4]                              # a stuck motor that is released; a dead motor beside a biased one
    right = runs[name][1]
    wrong = fault_loop_ref(cfg, model, pl, x0, xref, keys, T7, fault=faults(), mutant=mutant, episodes=eps, **ref_kwargs(name))
    assert bits_differ(right[0][eps], wrong[0][eps]) + bits_differ(right[1][eps], wrong[1][eps]) > 0, (mutant, name)
    assert np.array_equal(right[5][eps], wrong[5][eps])


class _FakeSolver:
    """Stands in for the handle of an MpcProblem: records closed_loop's keywords and returns recognisable arrays."""

    def __init__(self, m, H, n):
        self.m, self.H, self.n, self.kw = m, H, n, None

    def closed_loop(self, x0, xref, keys, T, **kw):
        self.kw = kw
        rng = np.random.default_rng(2)
        Ns = -(-T // kw["solve_period"])
        out = (rng.normal(size=(1, T + 1, 13)).astype(F), rng.normal(size=(1, T, self.m)).astype(F), rng.normal(size=(1, Ns, 8)).astype(F),
               rng.normal(size=(1, self.H, self.m)).astype(F), np.ones(1, F), np.zeros((1, 2), np.uint32), np.zeros((1, self.m), F))
        self.xsub = rng.normal(size=(1, T * self.n, 13)).astype(F)
        return out + (self.xsub,) if kw.get("substep_states") else out


@pytest.mark.parametrize("to_enu", [True, False])
def test_simulate_frame_rule(to_enu):
    """xsub comes back in the frame of x, row by row like xs[1:]; the fault schedule has no frame and goes through as f32[T or 1][1][m][2]."""
    cfg = small_cfg()
    T, n, m = 4, 3, 4
    prob = MpcProblem(cfg=cfg, model=synthetic_iris(), convert_to_enu=to_enu)
    fake = _FakeSolver(m, cfg.horizon, n)
    prob._solver, prob._pid = fake, os.getpid()
    x = np.zeros(13, F); x[6] = 1.0
    f = fault_schedule(T, 1, m)[:, 0]; f[2:, 1] = (0.0, 0.3)
    out = prob.simulate(x, np.zeros(2, np.uint32), T, plant_substeps=n, solve_period=2, fault=f, substep_states=True)
    assert len(out) == 6 and out[5].shape == (T * n, 13)
    want = np.stack([enu2ned(r, np) for r in fake.xsub[0]]) if to_enu else fake.xsub[0]
    assert out[5].tobytes() == np.ascontiguousarray(want, F).tobytes()
    assert fake.kw["fault"].shape == (T, 1, m, 2) and fake.kw["fault"].tobytes() == f.tobytes() and fake.kw["substep_states"] is True
    out = prob.simulate(x, np.zeros(2, np.uint32), T, plant_substeps=n, solve_period=2, fault=f[2])          # one row for every tick; five values as before
    assert len(out) == 5 and fake.kw["fault"].shape == (1, 1, m, 2) and "substep_states" not in fake.kw
    out = prob.simulate(x, np.zeros(2, np.uint32), T, plant_substeps=n, solve_period=2)
    assert len(out) == 5 and "fault" not in fake.kw and "substep_states" not in fake.kw
    for bad in (np.ones((T, 1, m, 2), F), np.ones((T + 1, m, 2), F), np.ones((m,), F)):
        with pytest.raises(ValueError):
            prob.simulate(x, np.zeros(2, np.uint32), T, fault=bad)
