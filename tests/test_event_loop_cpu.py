"""Motor faults and estimator dropouts drawn on the device (SPEC.md §11k) without a GPU: header / binding / library agree on the new symbol at ABI version 3 and
no kernel was added, every refusal of sdempc_closed_loop_batch_events in its documented order (no HIP call may happen before them) and of the Python surface, the
unchanged routing without the new keywords, the positions of the new values in the returned tuples, what the committed cases show on the reference generator alone
(tests/event_cases.py), the ten wrong generators of tests/event_loop_ref.py, faulted against unfaulted episodes through the loop reference, the chains' statistics
over 50,000 steps, the threshold endpoints and the host helpers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_census
from cases import ROOT, bits_differ
from event_cases import CASES, S2, case_events, for_ref, happenings, score_cfg, scored_episodes
from event_loop_ref import DROP_MUTANTS, FAULT_MUTANTS, MUTANTS, drop_rows, event_loop_ref, fault_rows
from loop_cases import REF_NAME
from sde4mbrl_px4_amd import _abi, prng, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, Dropouts, FaultProcess, Score, SdeMpcSolver, event_summary, score_init
from timed_loop_ref import num_solves

F = np.float32
U32 = np.uint32
NEW, OLD = "sdempc_closed_loop_batch_events", "sdempc_closed_loop_batch_tracked"
NEW_OUTS = ["fault_rows", "fault_keys_next", "fault_state_next", "valid_rows", "valid_keys_next", "valid_state_next"]


def test_abi_surface_of_the_events_entry_point_and_no_new_kernel():
    """FAILS before SPEC.md §11k: the library then has no such symbol."""
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    fields = lambda name: [ln.split(";")[0].split()[-1].lstrip("*") for ln in                                      # noqa: E731
                           re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1).strip().splitlines()]
    ff = ["struct_size", "n_modes", "batch", "onset", "clear", "modes", "keys", "state_in", "tick0"]
    df = ["struct_size", "batch", "drop", "recover", "keys", "state_in"]
    assert fields("sdempc_fault_process_cfg") == ff and fields("sdempc_dropout_process_cfg") == df
    R, D = _abi.SdempcFaultProcessCfg, _abi.SdempcDropoutProcessCfg
    assert [f[0] for f in R._fields_] == ff and C.sizeof(R) == 64 and (R.n_modes.offset, R.batch.offset, R.onset.offset, R.state_in.offset, R.tick0.offset) == (4, 8, 16, 48, 56)
    assert [f[0] for f in D._fields_] == df and C.sizeof(D) == 40 and (D.batch.offset, D.drop.offset, D.state_in.offset) == (4, 8, 32)
    names = lambda p: [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", p, flags=re.S).split(",")]      # noqa: E731
    proto = re.search(r"int " + NEW + r"\((.*?)\);", hdr, re.S).group(1)
    tproto = re.search(r"int " + OLD + r"\((.*?)\);", hdr, re.S).group(1)
    assert names(proto) == ["h", "fault_proc", "drop_proc"] + names(tproto)[1:] + NEW_OUTS          # every argument of the tracked entry point after h, in its order
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, NEW) and NEW in _abi.EXPORTED_SYMBOLS
    fn, ta = _abi.events_entry(lib), _abi.tracked_entry(lib).argtypes
    fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    assert list(fn.argtypes[3:-6]) == list(ta[1:]) and fn.argtypes[0] is ta[0] and fn.argtypes[1]._type_ is R and fn.argtypes[2]._type_ is D and fn.restype is C.c_int
    assert list(fn.argtypes[-6:]) == [fp, u32p, i32p, i32p, u32p, i32p]
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint " + NEW + r"\([^{]*\{\n\s*return guarded\(", src)
    # the chains are an argument of an existing kernel: the built kernel set is the census table, in both directions
    built = kernel_census.built_kernels()
    assert built is not None and built == kernel_census.table_names()
    assert ("sdempc_loop_keys_period_kernel", "") in built


def _call(lib, h, cfg, blob, B=4, T=5, S=2, n=2, fault=True, drop=True, fsize=None, dsize=None, K=2, fbatch=None, dbatch=None, onset="ok", clear="ok", modes="ok",
          fkeys=True, fstate=None, tick0=0, dthr=True, drecover=True, dkeys=True, dstate=None, obs=None, obs_keys=None, outs=None, score=False, null=(), D=0, track_size=None):
    """One sdempc_closed_loop_batch_events call on small neutral inputs; every field of the two event cfgs can be overridden. `outs` names the new outputs passed
    (default: those of the cfgs given); `null` the per-row outputs passed as NULL; track_size: a track cfg of that struct_size (wrong on purpose)."""
    fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    H, m = cfg.horizon, cfg.num_motors
    Tb, Bb = max(T, 1), max(B, 1)
    Ns = num_solves(Tb, max(S, 1))
    x0 = np.zeros((Bb, 13), F); x0[:, 6] = 1.0
    xref = np.zeros((1, 1, H + 1, 13), F); xref[..., 6] = 1.0
    k0, qk, fk, dk = (np.zeros((Bb, 2), U32) for _ in range(4))
    bufs_ = dict(xs=np.zeros((Bb, Tb + 1, 13), F), us=np.zeros((Bb, Tb, m), F), info=np.zeros((Bb, Ns, 8), F))
    p = {k: (None if k in null else v.ctypes.data_as(fp)) for k, v in bufs_.items()}
    obs = drop if obs is None else obs
    obs_keys = obs if obs_keys is None else obs_keys
    oc = _abi.SdempcObsCfg(C.sizeof(_abi.SdempcObsCfg), None, None, 1, 1, None, 1, 1)          # (no sigma, beta or valid: legal with a dropout chain)
    b_xm, b_qn, b_xn = np.zeros((Bb, Ns, 13), F), np.zeros((Bb, 2), U32), np.zeros((Bb, 13), F)
    g = np.zeros((1, 1, 13), F)
    zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg), 0, 1.0, 0.5, 4.0, g.ctypes.data_as(fp), 1, 1)
    zo = np.zeros((Bb, 16), U32)
    Kb = min(max(K, 1), 4)
    rows = B if fbatch is None else fbatch
    on = np.tile(np.arange(1, Kb + 1, dtype=U32) * U32(1 << 28), (max(rows, 1), m, 1)) if isinstance(onset, str) else (None if onset is None else np.ascontiguousarray(onset, U32))
    cl = np.full((max(rows, 1), m, Kb), 1 << 30, U32) if isinstance(clear, str) else (None if clear is None else np.ascontiguousarray(clear, U32))
    md = np.full((max(rows, 1), m, Kb, 2), 0.5, F) if isinstance(modes, str) else (None if modes is None else np.ascontiguousarray(modes, F))
    fs = None if fstate is None else np.ascontiguousarray(fstate, np.int32)
    ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)                  # noqa: E731
    fpc = _abi.SdempcFaultProcessCfg(C.sizeof(_abi.SdempcFaultProcessCfg) if fsize is None else fsize, K, rows, ptr(on, u32p), ptr(cl, u32p), ptr(md, fp),
                                     fk.ctypes.data_as(u32p) if fkeys else None, ptr(fs, i32p), tick0)
    drows = B if dbatch is None else dbatch
    dr, re_ = np.full(max(drows, 1), 1 << 30, U32), np.full(max(drows, 1), 1 << 31, U32)
    ds = None if dstate is None else np.ascontiguousarray(dstate, np.int32)
    dpc = _abi.SdempcDropoutProcessCfg(C.sizeof(_abi.SdempcDropoutProcessCfg) if dsize is None else dsize, drows, dr.ctypes.data_as(u32p) if dthr else None,
                                       re_.ctypes.data_as(u32p) if drecover else None, dk.ctypes.data_as(u32p) if dkeys else None, ptr(ds, i32p))
    o_f = (np.zeros((Bb, Tb, m, 2), F), np.zeros((Bb, 2), U32), np.zeros((Bb, m, 2), np.int32))
    o_d = (np.zeros((Bb, Ns), np.int32), np.zeros((Bb, 2), U32), np.zeros((Bb, 2), np.int32))
    want_f = fault if outs is None else "fault" in outs
    want_d = drop if outs is None else "drop" in outs
    new = ([o_f[0].ctypes.data_as(fp), o_f[1].ctypes.data_as(u32p), o_f[2].ctypes.data_as(i32p)] if want_f else [None] * 3) + \
          ([o_d[0].ctypes.data_as(i32p), o_d[1].ctypes.data_as(u32p), o_d[2].ctypes.data_as(i32p)] if want_d else [None] * 3)
    tk = None if track_size is None else _abi.SdempcTrackCfg(track_size, *([0, None, None, None, None, None, None, None, None, 0, 0, 0]))
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S, D, 0.0)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 1, n, 0.0, -1, -1)
    bufs = (C.c_char_p * 1)(blob)
    sz = (C.c_size_t * 1)(len(blob))
    return _abi.events_entry(lib)(
        h, C.byref(fpc) if fault else None, C.byref(dpc) if drop else None, None if tk is None else C.byref(tk), None, None, C.byref(zc) if score else None, None, None, None,
        C.byref(oc) if obs else None, qk.ctypes.data_as(u32p) if obs_keys else None, None, None, None, None, C.byref(tc), C.byref(pc),
        C.cast(bufs, C.POINTER(C.c_void_p)), sz, None, B, T, x0.ctypes.data_as(fp), xref.ctypes.data_as(fp), 1, 1, k0.ctypes.data_as(u32p), None, None, None,
        p["xs"], p["us"], None if p["info"] is None else C.cast(p["info"], C.POINTER(_abi.SdempcInfo)), None, None, None, None,
        None, None, None, None, None, None,
        b_xm.ctypes.data_as(fp) if obs and "xs" not in null else None, b_qn.ctypes.data_as(u32p) if obs else None, b_xn.ctypes.data_as(fp) if obs else None, None,
        zo.ctypes.data_as(u32p) if score else None, None, None, None, None, None, None, *new)


def test_events_argument_checks_make_no_hip_call_and_come_in_the_documented_order():
    import torch
    lib = _abi.load_library()
    cfg = score_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EDEVICE, ECAPACITY = -1, -3, -5
    B, m = 4, 4
    nan, inf = float("nan"), float("inf")
    dec = np.tile(np.array([1 << 29, 1 << 28], U32), (B, m, 1)); dec[:B - 1] = dec[:B - 1, :, ::-1]       # the LAST episode's rows decrease
    bad_modes = np.full((B, m, 2, 2), 0.5, F); bad_modes[B - 1, m - 1, 1, 1] = nan

    def state(b, l, s, first):
        a = np.tile(np.array([0, -1], np.int32), (B, m, 1))
        a[b, l] = (s, first)
        return a
    try:
        cases = [  # (keyword arguments, expected code, a word of the message), in the documented order
            (dict(fault=False, outs=("fault", "drop")), EINVAL, "without fault_proc"),
            (dict(drop=False, outs=("fault", "drop")), EINVAL, "without drop_proc"),
            (dict(fault=False, drop=False, outs=("drop",), obs=False), EINVAL, "without drop_proc"),
            (dict(fsize=56), EINVAL, "fault_proc struct_size"),
            (dict(fsize=0, T=0), EINVAL, "fault_proc struct_size"),                    # the structs are looked at first
            (dict(K=0), EINVAL, "n_modes"),
            (dict(K=5), EINVAL, "n_modes"),
            (dict(fbatch=0), EINVAL, "fault_proc batch"),
            (dict(fbatch=2), EINVAL, "fault_proc batch"),
            (dict(onset=None), EINVAL, "is NULL"),
            (dict(clear=None), EINVAL, "is NULL"),
            (dict(modes=None), EINVAL, "is NULL"),
            (dict(fkeys=False), EINVAL, "is NULL"),
            (dict(onset=dec), EINVAL, "onset row decreases"),
            (dict(modes=bad_modes), EINVAL, "modes holds"),
            (dict(modes=np.where(np.isnan(bad_modes), -inf, bad_modes)), EINVAL, "modes holds"),
            (dict(fstate=state(3, 3, 3, -1)), EINVAL, "fault_proc state_in"),          # s > K = 2
            (dict(fstate=state(0, 1, -1, -1)), EINVAL, "fault_proc state_in"),
            (dict(fstate=state(2, 0, 1, -2)), EINVAL, "fault_proc state_in"),
            (dict(tick0=-1), EINVAL, "tick0"),
            (dict(tick0=(1 << 24) - 5), EINVAL, "tick0"),
            (dict(dsize=32), EINVAL, "drop_proc struct_size"),
            (dict(dbatch=3), EINVAL, "drop_proc batch"),
            (dict(dthr=False), EINVAL, "drop, recover or keys"),
            (dict(drecover=False), EINVAL, "drop, recover or keys"),
            (dict(dkeys=False), EINVAL, "drop, recover or keys"),
            (dict(dstate=np.array([[0, 0], [2, 0], [0, 0], [0, 0]])), EINVAL, "drop_proc state_in"),
            (dict(dstate=np.array([[0, 0], [1, 0], [0, 0], [0, -1]])), EINVAL, "drop_proc state_in"),
            (dict(obs_keys=False, obs=True), EINVAL, "drop_proc needs"),
            (dict(obs=False), EINVAL, "drop_proc needs"),
            # a call wrong in two ways is refused for the earlier reason
            (dict(fault=False, outs=("fault", "drop"), dsize=0), EINVAL, "without fault_proc"),
            (dict(fsize=0, K=9), EINVAL, "fault_proc struct_size"),
            (dict(K=0, fbatch=2), EINVAL, "n_modes"),
            (dict(fbatch=2, onset=None), EINVAL, "fault_proc batch"),
            (dict(fkeys=False, onset=dec), EINVAL, "is NULL"),
            (dict(onset=dec, modes=bad_modes), EINVAL, "onset row decreases"),
            (dict(modes=bad_modes, fstate=state(0, 0, 3, -1)), EINVAL, "modes holds"),
            (dict(fstate=state(0, 0, 3, -1), tick0=-1), EINVAL, "fault_proc state_in"),
            (dict(tick0=-1, dsize=0), EINVAL, "tick0"),
            (dict(dbatch=3, obs=False), EINVAL, "drop_proc batch"),
            (dict(obs=False, track_size=8), EINVAL, "drop_proc needs"),                 # the event checks stand in FRONT of the track checks
            (dict(tick0=-1, S=0), EINVAL, "tick0"),
            # everything the tracked entry point refuses, behind valid event cfgs
            (dict(track_size=8), EINVAL, "track: struct_size"),
            (dict(null=("xs",)), EINVAL, "NULL host pointer"),
            (dict(D=5), EINVAL, "solve_delay"),
            (dict(T=0), EINVAL, "T must"),
            (dict(B=5, fbatch=1, dbatch=1), ECAPACITY, "max_batch"),
            (dict(n=0), EINVAL, "substeps"),
            (dict(S=0), EINVAL, "solve_period"),
        ]
        for kw, want, word in cases:
            rc = _call(lib, h, cfg, blob, **kw)
            msg = lib.sdempc_last_error(h).decode()
            assert rc == want, (sorted(kw), rc, msg)
            assert word in msg, (word, msg)
            assert lib.sdempc_device_ready(h) == 0
        # valid arguments reach the device: each chain alone, shared thresholds, one and four modes, equal cumulative thresholds, a state, the largest tick0, no new
        # outputs, NULL rows under a score, both cfgs NULL (the tracked call)
        good = 0 if torch.cuda.is_available() else EDEVICE
        flat = np.full((B, m, 2), 1 << 28, U32)
        for kw in (dict(), dict(drop=False), dict(fault=False), dict(fbatch=1, dbatch=1), dict(K=1), dict(K=4), dict(onset=flat), dict(onset=np.zeros((B, m, 2), U32)),
                   dict(fstate=state(1, 2, 2, 0), dstate=np.array([[1, 3]] * B)), dict(tick0=(1 << 24) - 6), dict(outs=()), dict(score=True, null=("xs", "us", "info")),
                   dict(fault=False, drop=False), dict(fault=False, drop=False, score=True), dict(T=1)):
            rc = _call(lib, h, cfg, blob, **kw)
            assert rc == good, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def _fake_entries(monkeypatch, seen):
    def fake(name):
        def entry(lib):
            def call(h, *args):
                seen["name"], seen["args"] = name, args
                return 0
            return call
        return entry
    for e in ("events", "tracked", "drawn", "scored", "aged", "observed", "fault", "rate", "scenario", "timed"):
        monkeypatch.setattr(_abi, e + "_entry", fake(e))


def test_python_surface_checks_the_event_keywords():
    cfg = score_cfg()
    model = synthetic_iris()
    B, T, m = 3, 5, 4
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), U32)
    fpr = FaultProcess(np.full((m, 2), 0.1), 0.3, np.zeros((m, 2, 2), F))
    dp = Dropouts(0.3, 0.4)
    for kw in (dict(fault_keys=k), dict(fault_state_in=np.zeros((B, m, 2), np.int32)), dict(fault_tick0=3)):      # each needs its process
        with pytest.raises(ValueError, match="need fault_process"):
            S.closed_loop(x0, xref, k, T, **kw)
    for kw in (dict(drop_keys=k), dict(drop_state_in=np.zeros((B, 2), np.int32))):
        with pytest.raises(ValueError, match="need drop_process"):
            S.closed_loop(x0, xref, k, T, **kw)
    for kw in (dict(fault_process=fpr), dict(drop_process=dp, meas_keys=k)):                                       # a process needs its keys
        with pytest.raises(ValueError, match="_keys .* is required"):
            S.closed_loop(x0, xref, k, T, **kw)
    with pytest.raises(ValueError, match="meas_keys"):
        S.closed_loop(x0, xref, k, T, drop_process=dp, drop_keys=k)
    st = np.tile(np.array([0, -1], np.int32), (B, m, 1))
    for kw in (dict(fault_process=(0.1, 0.3), fault_keys=k), dict(fault_process=fpr, fault_keys=k[:2]), dict(fault_process=fpr, fault_keys=k, fault_state_in=st[:, :3]),
               dict(fault_process=fpr, fault_keys=k, fault_state_in=st + np.array([3, 0], np.int32)), dict(fault_process=fpr, fault_keys=k, fault_state_in=st - np.array([0, 1], np.int32)),
               dict(fault_process=fpr, fault_keys=k, fault_tick0=-1), dict(fault_process=fpr, fault_keys=k, fault_tick0=(1 << 24) - 5),
               dict(fault_process=FaultProcess(np.full((6, 2), 0.1), 0.3, np.zeros((6, 2, 2), F)), fault_keys=k),                 # six motors on a four-motor handle
               dict(fault_process=FaultProcess(np.full((2, m, 1), 0.1), 0.3, np.zeros((2, m, 1, 2), F)), fault_keys=k),           # two rows for three episodes
               dict(drop_process=0.3, drop_keys=k, meas_keys=k), dict(drop_process=Dropouts(np.full(2, 0.3), 0.4), drop_keys=k, meas_keys=k),
               dict(drop_process=dp, drop_keys=k, meas_keys=k, drop_state_in=np.array([[2, 0]] * B)), dict(drop_process=dp, drop_keys=k, meas_keys=k, drop_state_in=np.array([[0, -1]] * B)),
               dict(fault_process=fpr, fault_keys=k, outputs=False)):
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    for bad in (dict(p_onset=np.full((m, 3), 0.4), p_clear=0.3, modes=np.zeros((m, 3, 2))),                         # a row sums to 1.2
                dict(p_onset=np.full((m, 2), -0.1), p_clear=0.3, modes=np.zeros((m, 2, 2))), dict(p_onset=np.full((m, 2), 0.1), p_clear=1.5, modes=np.zeros((m, 2, 2))),
                dict(p_onset=np.full((m, 5), 0.1), p_clear=0.3, modes=np.zeros((m, 5, 2))), dict(p_onset=np.full((m, 2), 0.1), p_clear=0.3, modes=np.zeros((m, 3, 2))),
                dict(p_onset=np.full((m, 2), 0.1), p_clear=0.3, modes=np.full((m, 2, 2), np.inf)), dict(p_onset=np.full(m, 0.1), p_clear=0.3, modes=np.zeros((m, 1, 2)))):
        with pytest.raises(ValueError):
            FaultProcess(**bad)
    with pytest.raises(ValueError, match="decreases"):
        FaultProcess.from_thresholds(np.array([[5, 4]] * m), np.zeros((m, 2), np.int64), np.zeros((m, 2, 2)))
    for bad in ((1.5, 0.1), (-0.1, 0.1), (0.5, np.nan)):
        with pytest.raises(ValueError):
            Dropouts(*bad)
    with pytest.raises(ValueError):
        Dropouts.from_thresholds(1 << 32, 0)
    assert not S.device_ready()
    S.close()
    prob = MpcProblem(cfg=cfg, model=model)
    z2 = np.zeros(2, U32)
    with pytest.raises(ValueError, match="need fault_process"):
        prob.simulate(np.zeros(13, F), z2, T, fault_rng=z2)
    with pytest.raises(ValueError, match="need drop_process"):
        prob.simulate(np.zeros(13, F), z2, T, drop_state=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="fault_rng .* is required"):
        prob.simulate(np.zeros(13, F), z2, T, fault_process=fpr)
    with pytest.raises(ValueError, match="meas_rng"):
        prob.simulate(np.zeros(13, F), z2, T, drop_process=dp, drop_rng=z2)


def test_routing_without_the_new_keywords_is_unchanged_and_tuple_positions(monkeypatch):
    """Without one of the seven keywords every call looks up the entry point it looked up before and returns the tuple it returned before; with them the new values sit
    behind the bias process's values and in front of xsub, faults first; outputs=False returns None for the rows."""
    from sde4mbrl_px4_amd.solver import GaussMarkov, Trajectory
    cfg = score_cfg()
    B, T, n, m = 3, 5, 2, 4
    Ns = num_solves(T, 2)
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=B)
    seen = {}
    _fake_entries(monkeypatch, seen)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), U32)
    g = np.zeros((T, 1, 13), F)
    tm = dict(solve_period=2, plant_substeps=n)
    gd = GaussMarkov(np.arange(1.0, 7.0), 0.5, 0.05)
    tr = Trajectory(np.array([0.0, 1.0], F), np.tile(np.eye(13, dtype=F)[6], (2, 1)))
    unchanged = ((dict(tm), "timed", 7), (dict(tm, disturbance=np.zeros(6, F)), "scenario", 7), (dict(tm, substep_states=True), "fault", 8),
                 (dict(tm, meas_valid=np.ones(Ns, int), meas_keys=k), "observed", 10), (dict(tm, meas_valid=np.ones(Ns, int), meas_keys=k, meas_renorm=True), "aged", 10),
                 (dict(tm, score=Score(), score_ref=g), "scored", 8), (dict(tm, dist_process=gd, dist_keys=k), "drawn", 10), (dict(tm, track=tr), "tracked", 7))
    for kw, name, count in unchanged:
        out = S.closed_loop(x0, None if "track" in kw else xref, k, T, **kw)
        assert seen["name"] == name and len(out) == count, (name, seen["name"], len(out))
    n_tracked = len(seen["args"])
    fpr = FaultProcess(np.full((m, 3), 0.1), 0.3, np.arange(m * 3 * 2, dtype=F).reshape(m, 3, 2))
    dp = Dropouts(np.full(B, 0.3), 0.4)
    # the fault chain alone: no observation, no score, no track — NULL in every cfg position but the first
    out = S.closed_loop(x0, xref, k, T, **tm, fault_process=fpr, fault_keys=k, fault_tick0=11)
    a = seen["args"]
    assert seen["name"] == "events" and len(a) == n_tracked + 8 and len(out) == 10
    assert [v.shape for v in out[7:]] == [(B, T, m, 2), (B, 2), (B, m, 2)] and out[8].dtype == U32 and out[9].dtype == np.int32
    assert a[0] is not None and all(v is None for v in a[1:12]) and all(v is not None for v in a[-6:-3]) and all(v is None for v in a[-3:])
    pc = a[0]._obj
    assert (pc.struct_size, pc.n_modes, pc.batch, pc.tick0) == (64, 3, 1, 11) and not pc.state_in
    on, cl, md = fpr.arrays(B, m)
    assert np.ctypeslib.as_array(pc.onset, (m, 3)).tobytes() == on.tobytes() and np.ctypeslib.as_array(pc.modes, (m, 3, 2)).tobytes() == md.tobytes()
    # the dropout chain alone makes the call an observed one with an empty obs cfg
    out = S.closed_loop(x0, xref, k, T, **tm, drop_process=dp, drop_keys=k, meas_keys=k, drop_state_in=np.array([[1, 2]] * B))
    a = seen["args"]
    assert seen["name"] == "events" and len(out) == 13 and [v.shape for v in out[7:]] == [(B, Ns, 13), (B, 2), (B, 13), (B, Ns), (B, 2), (B, 2)]
    assert out[10].dtype == np.int32 and a[0] is None and a[1] is not None and a[1]._obj.batch == B and a[9] is not None and a[10] is not None
    oc = a[9]._obj
    assert not oc.sigma and not oc.beta and not oc.valid
    assert all(v is None for v in a[-6:-3]) and all(v is not None for v in a[-3:])
    # both, with a Gauss-Markov process, a score and xsub: score, dist values, fault values, dropout values, xsub
    both = dict(tm, fault_process=fpr, fault_keys=k, drop_process=dp, drop_keys=k, meas_keys=k, dist_process=gd, dist_keys=k, score=Score(), score_ref=g, substep_states=True)
    out = S.closed_loop(x0, xref, k, T, **both)
    assert len(out) == 21 and out[10].dtype == SCORE_DTYPE
    assert [v.shape for v in out[11:]] == [(B, T, 6), (B, 2), (B, 6), (B, T, m, 2), (B, 2), (B, m, 2), (B, Ns), (B, 2), (B, 2), (B, T * n, 13)]
    out = S.closed_loop(x0, xref, k, T, **both, outputs=False)
    names = ("xs", "us", "info", "u_next", "stepsize_next", "keys_next", "u_act_next", "xmeas", "meas_keys_next", "xmeas_next", "score", "dist_rows", "dist_keys_next",
             "dist_state_next", "fault_rows", "fault_keys_next", "fault_state_next", "valid_rows", "valid_keys_next", "valid_state_next", "xsub")
    assert len(out) == len(names)
    for nm, v in zip(names, out):
        assert (v is None) == (nm in ("xs", "us", "info", "xmeas", "dist_rows", "fault_rows", "valid_rows", "xsub")), nm
    a = seen["args"]
    assert a[-6] is None and a[-5] is not None and a[-4] is not None and a[-3] is None and a[-2] is not None and a[-1] is not None
    # with a track the track cfg keeps its place behind the two event cfgs
    out = S.closed_loop(x0, None, k, T, **tm, track=tr, fault_process=fpr, fault_keys=k)
    assert seen["name"] == "events" and seen["args"][2] is not None and len(out) == 10
    assert not S.device_ready()
    S.close()


def test_the_cases_show_what_they_were_chosen_to_show():
    """The conditions of tests/event_cases.py, on the reference generator alone."""
    h = {name: happenings(name) for name in CASES}
    assert set().union(*(v["modes"] for v in h.values())) == {0, 1, 2, 3}
    assert h["iris_k4_per_episode"]["modes"] == {0, 1, 2, 3} and h["iris_k3_shared"]["modes"] == {0, 1, 2}
    for cond in ("clear", "never_fails", "two_in_one_tick", "onset_at_tick0", "onset_inside_period", "drop_at_solve0", "recovery", "never_dropped"):
        assert any(v[cond] for v in h.values()), cond
    assert all(v["first_matches"] for v in h.values())          # `first` is the tick of the first onset, -1 without one
    assert {c["m"] for c in CASES.values()} == {3, 4, 6} and {c["K"] for c in CASES.values()} == {1, 3, 4}
    assert {c["per_episode"] for c in CASES.values()} == {False, True}
    # thresholds distinct per motor
    for name, c in CASES.items():
        on = case_events(name)["fault_process"].onset
        assert len({on[0, l].tobytes() for l in range(c["m"])}) == c["m"], name


def _generated(name, mutant=None, scheduled=True, states=False):
    """(fault part, drop part) of the generator on a case: scheduled rows of both kinds, start states on request."""
    from event_cases import VALID
    from fault_cases import faults_any
    c = CASES[name]
    B, m, K, T = c["B"], c["m"], c["K"], c["T"]
    Ns = num_solves(T, S2)
    kw = for_ref(case_events(name, states=states), B, m)
    fsched = faults_any(T, B, m) if scheduled else None
    vsched = np.ascontiguousarray(VALID[:Ns, :B]) if scheduled else None
    f = fault_rows(kw["fault_keys"], *kw["fault_process"], kw["fault_state_in"], T, kw.get("fault_tick0", 0), fsched, S2, mutant if mutant in FAULT_MUTANTS else None)
    d = drop_rows(kw["drop_keys"], *kw["drop_process"], kw["drop_state_in"], Ns, vsched, mutant if mutant in DROP_MUTANTS else None)
    return f, d


def _differs(a, b):
    return any(not np.array_equal(np.asarray(x).view(U32) if np.asarray(x).dtype == F else x, np.asarray(y).view(U32) if np.asarray(y).dtype == F else y)
               for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_wrong_generator_differs_from_the_reference_on_the_cases(mutant):
    """Ten wrong generators; each changes the rows, the chain or the state of the chain it touches on at least one committed case — and on the case named for the
    mutants that need a particular one."""
    assert len(MUTANTS) == 10
    hit_f = hit_d = 0
    for name in CASES:
        for states in (False, True):
            right, wrong = _generated(name, states=states), _generated(name, mutant, states=states)
            hit_f += _differs(right[0], wrong[0])
            hit_d += _differs(right[1], wrong[1])
    if mutant in FAULT_MUTANTS:
        assert hit_f > 0, mutant
    if mutant in DROP_MUTANTS:
        assert hit_d > 0, mutant
    if mutant == "le_for_lt":                           # thresholds ON a drawn word: the one case that can tell <= from <
        right, wrong = _generated("tri_k3_boundary"), _generated("tri_k3_boundary", mutant)
        assert right[0][3][0, 0, 1] != 1 and wrong[0][3][0, 0, 1] == 1 and right[1][3][0, 0] == 0 and wrong[1][3][0, 0] == 1
    if mutant == "words_reversed":                      # the odd lane count alone shows it
        assert _differs(_generated("tri_k3_shared")[0], _generated("tri_k3_shared", mutant)[0])
    if mutant == "mode_off_by_one":
        assert not _differs(_generated("hexa_k1_per_episode")[0][:1], _generated("hexa_k1_per_episode", mutant)[0][:1])       # (one mode: nothing to be off by)
        assert _differs(_generated("iris_k4_per_episode")[0], _generated("iris_k4_per_episode", mutant)[0])


def test_generator_passes_schedules_through_and_continues():
    """State 0 passes the scheduled row through bit for bit (-0 included) and the neutral row otherwise; a failed motor reads its mode row whatever the schedule;
    the dropout flag is the AND of chain and schedule; both chains continue bit for bit through keys_next / state_next and tick0 + T."""
    from fault_cases import faults_any
    name = "iris_k4_per_episode"
    c = CASES[name]
    B, m, T = c["B"], c["m"], c["T"]
    kw = for_ref(case_events(name), B, m)
    sched = faults_any(T, B, m)
    sched[0, 0, 0] = (-0.0, -0.0)
    rows, kn, sn, s = fault_rows(kw["fault_keys"], *kw["fault_process"], None, T, scheduled=sched)
    plain = fault_rows(kw["fault_keys"], *kw["fault_process"], None, T)[0]
    md = kw["fault_process"][2]
    for b in range(B):
        for k in range(T):
            for l in range(m):
                want = md[b, l, s[b, k, l] - 1] if s[b, k, l] > 0 else sched[k, b, l]
                assert rows[b, k, l].tobytes() == want.tobytes()
                assert plain[b, k, l].tobytes() == (want if s[b, k, l] > 0 else np.array([1, 0], F)).tobytes()
    for cut in (1, 3, 4):
        a = fault_rows(kw["fault_keys"], *kw["fault_process"], None, cut, tick0=5, scheduled=sched[:cut])
        b_ = fault_rows(a[1], *kw["fault_process"], a[2], T - cut, tick0=5 + cut, scheduled=sched[cut:])
        whole = fault_rows(kw["fault_keys"], *kw["fault_process"], None, T, tick0=5, scheduled=sched)
        assert np.concatenate([a[0], b_[0]], axis=1).tobytes() == whole[0].tobytes() and np.array_equal(b_[1], whole[1]) and np.array_equal(b_[2], whole[2])
    Ns = 3
    valid = np.array([[1, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1]])
    flags, dk, dn, d = drop_rows(kw["drop_keys"], *kw["drop_process"], None, Ns, valid)
    assert np.array_equal(flags, ((d == 0) & (valid.T != 0)).astype(np.int32)) and np.array_equal(dn[:, 1], (d == 1).sum(axis=1))
    free = drop_rows(kw["drop_keys"], *kw["drop_process"], None, Ns)
    assert np.array_equal(free[3], d) and np.array_equal(free[1], dk)            # the chain does not see the schedule
    a = drop_rows(kw["drop_keys"], *kw["drop_process"], None, 1, valid[:1])
    b_ = drop_rows(a[1], *kw["drop_process"], a[2], 2, valid[1:])
    assert np.array_equal(np.concatenate([a[0], b_[0]], axis=1), flags) and np.array_equal(b_[1], dk) and np.array_equal(b_[2], dn)


def _ref(cfg, model, x0, xref, keys, T, **kw):
    B = x0.shape[0]
    return event_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T, substep_states=True,
                          **{"plants": None, **{REF_NAME.get(k, k): v for k, v in for_ref(kw, B, cfg.num_motors).items()}})


def test_reference_changes_every_faulted_episode_and_no_unfaulted_one():
    """Through the loop reference: an episode whose chain leaves state 0 differs from the fault-free run from the onset tick on — in its states and, from the next
    solve on, in its solves — and an episode without an onset equals the fault-free run bit for bit; a dropped solve holds the measurement."""
    name = "iris_k3_shared"
    c = CASES[name]
    B, T = c["B"], c["T"]
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B, 191)
    x0 = np.nan_to_num(x0, nan=0.1, posinf=0.2)               # (finite episodes: a NaN state hides every later change)
    ev = case_events(name)
    fe = {k: v for k, v in ev.items() if k.startswith("fault_")}
    on, cl, md = (np.repeat(v, B, axis=0) for v in fe["fault_process"].arrays(B, 4))
    on[B - 1] = 0                                              # the last episode never fails
    fe["fault_process"] = FaultProcess.from_thresholds(on, cl, md)
    free = _ref(cfg, model, x0, xref, keys, T, **kw)
    got = _ref(cfg, model, x0, xref, keys, T, **kw, **fe)
    st = got[-2]
    assert st.shape == (B, 4, 2) and len(got) == len(free) + 3
    faulted = (st[:, :, 1] >= 0).any(axis=1)
    assert faulted.any() and (~faulted).any()
    for b in range(B):
        if not faulted[b]:
            for g, w in zip(got[:7] + got[-1:], free):
                assert g[b].tobytes() == w[b].tobytes()
            continue
        k1 = int(np.where(st[b, :, 1] >= 0, st[b, :, 1], T).min())
        assert got[0][b, :k1 + 1].tobytes() == free[0][b, :k1 + 1].tobytes()                      # nothing before the onset tick's plant step
        assert bits_differ(got[0][b, k1 + 1:], free[0][b, k1 + 1:]) > 0
        j1 = k1 // S2 + 1                                                                          # the first solve that starts from a changed state
        assert got[2][b, :j1].tobytes() == free[2][b, :j1].tobytes()
        if j1 < got[2].shape[1]:
            assert bits_differ(got[2][b, j1:], free[2][b, j1:]) > 0
    # dropouts: a dropped solve starts from the held measurement, and an episode equals the run without the chain up to its first dropout
    de = {k: v for k, v in ev.items() if k.startswith(("drop_", "meas_"))}
    seen_ = _ref(cfg, model, x0, xref, keys, T, **kw, meas_valid=np.ones(3, int), meas_keys=ev["meas_keys"])
    dropped = _ref(cfg, model, x0, xref, keys, T, **kw, **de)
    flags, xmeas = dropped[-4], dropped[7]
    assert flags.shape == (B, 3) and (flags == 0).any() and flags.all(axis=1).any()
    for b in range(B):
        for j in range(3):
            if flags[b, j] == 0:
                assert xmeas[b, j].tobytes() == (xmeas[b, j - 1] if j else x0[b]).tobytes()
        if flags[b].all():
            for g, w in zip(dropped[:10] + dropped[-1:], seen_):
                assert g[b].tobytes() == w[b].tobytes()
        else:                                                  # (a solve dropped after solve 0 starts from another state than the plant's)
            j = int(np.argmin(flags[b]))
            assert dropped[7][b, :j].tobytes() == seen_[7][b, :j].tobytes()
            if j > 0:
                assert bits_differ(dropped[7][b, j], seen_[7][b, j]) > 0


def test_statistics_of_the_chains_over_fifty_thousand_steps():
    """B = 1, one fixed key, 50,000 steps: onsets over steps in state 0, clears over steps in a failed state and the split of the onsets among three modes each lie
    within five binomial standard errors of threshold / 2^32; so do the dropout chain's two ratios."""
    N = 50000
    fpr = FaultProcess(np.array([[0.08, 0.05, 0.12]]), np.array([[0.3, 0.3, 0.3]]), np.zeros((1, 3, 2), F))
    on, cl, md = fpr.arrays(1, 1)
    key = prng.PRNGKey(20261021)[None]
    _, _, st, s = fault_rows(key, on, cl, md, None, N)
    s = s[0, :, 0]
    prev = np.concatenate([[0], s[:-1]])

    def near(hits, trials, p, what):
        assert trials > 1000, what
        assert abs(hits / trials - p) <= 5.0 * np.sqrt(p * (1.0 - p) / trials), (what, hits, trials, p)
    p_on = on[0, 0].astype(np.float64) / 2.0**32                     # cumulative
    n0 = int((prev == 0).sum())
    onsets = (prev == 0) & (s > 0)
    near(int(onsets.sum()), n0, p_on[2], "onset")
    near(int(((prev > 0) & (s == 0)).sum()), int((prev > 0).sum()), cl[0, 0, 0] / 2.0**32, "clear")
    lo = 0.0
    for j in range(3):
        near(int((onsets & (s == j + 1)).sum()), n0, p_on[j] - lo, f"mode {j}")
        lo = p_on[j]
    assert st[0, 0, 1] == int(np.argmax(onsets))
    dp = Dropouts(0.2, 0.35)
    dr, re_ = dp.arrays(1)
    _, _, dn, d = drop_rows(key, dr, re_, None, N)
    d = d[0]
    dprev = np.concatenate([[0], d[:-1]])
    near(int(((dprev == 0) & (d == 1)).sum()), int((dprev == 0).sum()), dr[0] / 2.0**32, "drop")
    near(int(((dprev == 1) & (d == 0)).sum()), int((dprev == 1).sum()), re_[0] / 2.0**32, "recover")
    assert dn[0, 1] == int(d.sum())


def test_threshold_endpoints_and_their_formation():
    """A threshold of 0 never fires, exactly; 2^32 - 1 fires on every word but one; thresholds are floor(p 2^32) formed once in float64, the onset ones cumulated in
    float64 first; from_rates maps an infinite duration to 0 and a rate to 1 - exp(-rate dt)."""
    key = np.stack([prng.PRNGKey(5 + b) for b in range(4)])
    z = np.zeros((1, 2, 2), U32)
    md = np.zeros((1, 2, 2, 2), F)
    rows, _, st, s = fault_rows(key, z, z, md, None, 400)
    assert not s.any() and (st[:, :, 1] == -1).all() and (rows == np.array([1, 0], F)).all()
    top = np.full((1, 2, 2), 0xFFFFFFFF, U32)
    _, _, st, s = fault_rows(key, top, z, md, None, 50)
    assert (s == 1).all() and (st[:, :, 1] == 0).all()                       # failed at tick 0 from state 0, and permanent with clear = 0
    _, _, _, s = fault_rows(key, top, top, md, None, 50)
    assert (s[:, 0::2] == 1).all() and (s[:, 1::2] == 0).all()               # one transition per step: fail, clear, fail, ...
    _, _, dn, d = drop_rows(key, 0, 0xFFFFFFFF, None, 300)
    assert not d.any() and not dn.any()
    _, _, dn, d = drop_rows(key, 0, 0, np.array([[1, 4]] * 4), 300)
    assert d.all() and (dn == (1, 304)).all()                                # a chain that starts dropped and never recovers
    rng = np.random.default_rng(3)
    p = rng.uniform(0.0, 0.3, (5, 3))
    fpr = FaultProcess(p, 0.25, np.zeros((5, 3, 2), F))
    cum = np.cumsum(p.astype(np.float64), axis=-1)
    assert fpr.onset.dtype == U32 and np.array_equal(fpr.onset[0], np.floor(cum * 2.0**32).astype(np.uint64).astype(U32)) and (np.diff(fpr.onset[0].astype(np.int64)) >= 0).all()
    assert (fpr.clear == U32(1 << 30)).all()
    one = FaultProcess(np.array([[1.0]]), np.array([[1.0]]), np.zeros((1, 1, 2), F))
    assert one.onset[0, 0, 0] == 0xFFFFFFFF == one.clear[0, 0, 0]           # min(2^32 - 1, .): "always" is not expressible
    assert FaultProcess(np.zeros((2, 2)), 0.0, np.zeros((2, 2, 2), F)).onset.sum() == 0
    fr = FaultProcess.from_rates(np.array([[0.5, 2.0]]), np.array([[np.inf, 0.2]]), 0.05, np.zeros((1, 2, 2), F))
    p2 = 1.0 - np.exp(-np.array([0.5, 2.0]) * 0.05)
    assert np.array_equal(fr.onset[0, 0], np.floor(np.cumsum(-np.expm1(-np.array([0.5, 2.0]) * 0.05)) * 2.0**32).astype(np.uint64).astype(U32))
    assert abs(int(fr.onset[0, 0, 0]) - p2[0] * 2.0**32) < 2.0**10 and fr.clear[0, 0, 0] == 0 and fr.clear[0, 0, 1] == int(np.floor(-np.expm1(-0.05 / 0.2) * 2.0**32))
    dr = Dropouts.from_rates(1.0, np.inf, 0.1)
    assert dr.recover[0] == 0 and dr.drop[0] == int(np.floor(-np.expm1(-0.1) * 2.0**32))
    th = FaultProcess.from_thresholds(np.array([[7, 7, 9]]), np.array([[1, 2, 3]]), np.zeros((1, 3, 2), F))
    assert th.onset.tolist() == [[[7, 7, 9]]] and th.clear.tolist() == [[[1, 2, 3]]] and th.n_modes == 3
    assert Dropouts.from_thresholds(5, np.array([6, 7])).arrays(2)[0].tolist() == [5, 5]
    on, cl, mm = fpr.arrays(4, 5)
    assert on.shape == (1, 5, 3) and mm.shape == (1, 5, 3, 2) and on.flags.c_contiguous


def test_event_summary_reduces_the_fault_states():
    st = np.array([[[0, -1], [2, 4]], [[0, -1], [0, -1]], [[1, 0], [0, 3]]], np.int32)
    z = score_init(3)
    z["first_fail_row"][0] = 2
    out = event_summary(st, z)
    assert (out["episodes"], out["faulted"]) == (3, 2) and out["onsets_per_motor"].tolist() == [1, 2] and out["first_onset_tick"].tolist() == [4, -1, 0]
    assert out["fail_rate_faulted"] == 0.5 and out["fail_rate_unfaulted"] == 0.0
    assert "fail_rate_faulted" not in event_summary(st)
    assert np.isnan(event_summary(st[1:2], z[1:2])["fail_rate_faulted"])
    with pytest.raises(ValueError):
        event_summary(st[0])


def test_simulate_passes_the_chains_through_frameless(monkeypatch):
    """MpcProblem.simulate: the chains of one episode, the global tick from curr_t, the values behind the Gauss-Markov ones and in front of xsub, unconverted."""
    cfg = score_cfg()
    model = synthetic_hexa() if cfg.num_motors == 6 else synthetic_iris()
    m, T, n = cfg.num_motors, 5, 2
    prob = MpcProblem(cfg=cfg, model=model)
    seen = {}

    def closed_loop(x0, xref, rng, T_, **kw):
        seen.update(kw)
        Ns = num_solves(T_, kw["solve_period"])
        out = (np.zeros((1, T_ + 1, 13), F), np.zeros((1, T_, m), F), np.zeros((1, Ns, 8), F), np.zeros((1, cfg.horizon, m), F), np.zeros(1, F), np.zeros((1, 2), U32),
               np.zeros((1, m), F), np.zeros((1, Ns, 13), F), np.zeros((1, 2), U32), np.zeros((1, 13), F))
        out += (np.full((1, T_, m, 2), 3.0, F), np.full((1, 2), 4, U32), np.full((1, m, 2), 5, np.int32), np.full((1, Ns), 6, np.int32), np.full((1, 2), 7, U32),
                np.full((1, 2), 8, np.int32), np.zeros((1, T_ * n, 13), F))
        return out

    class Fake:
        pass
    fake = Fake()
    fake.closed_loop = closed_loop
    monkeypatch.setattr(prob, "solver", lambda: fake)
    fpr = FaultProcess(np.full((m, 2), 0.1), 0.3, np.zeros((m, 2, 2), F))
    dp = Dropouts(0.3, 0.4)
    x = np.zeros(13, F); x[6] = 1.0
    dt0 = float(cfg.time_steps[0])
    out = prob.simulate(x, np.zeros(2, U32), T, curr_t=9 * dt0, solve_period=2, plant_substeps=n, substep_states=True, fault_process=fpr, fault_rng=np.array([1, 2], U32),
                        fault_state=np.zeros((m, 2), np.int32), drop_process=dp, drop_rng=np.array([3, 4], U32), meas_rng=np.array([5, 6], U32))
    assert seen["fault_process"] is fpr and seen["drop_process"] is dp and seen["fault_tick0"] == 9 and seen["fault_keys"].tolist() == [[1, 2]]
    assert seen["fault_state_in"].shape == (1, m, 2) and seen["drop_state_in"] is None and seen["drop_keys"].tolist() == [[3, 4]]
    assert len(out) == 5 + 2 + 6 + 1
    assert [np.asarray(v).shape for v in out[7:13]] == [(T, m, 2), (2,), (m, 2), (3,), (2,), (2,)]
    assert [int(np.asarray(v).flat[0]) for v in out[7:13]] == [3, 4, 5, 6, 7, 8] and out[-1].shape == (T * n, 13)
