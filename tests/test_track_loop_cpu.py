"""Reference windows and score targets cut from a trajectory (SPEC.md §11j) without a GPU: the ABI surface of the two new entry points, every refusal of
sdempc_closed_loop_batch_tracked and sdempc_reference_windows before a device is touched, the Python keywords and their routing, the ten wrong generators of
tests/track_loop_ref.py on the committed cases (tests/track_cases.py), exactness on the knots, solver.Trajectory against the reference and the reference against
a float64 interpolant."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_census
from cases import ROOT, bits_differ
from sde4mbrl_px4_amd import _abi, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import Score, SdeMpcSolver, Trajectory
from timed_loop_ref import num_solves
from track_cases import B5, S2, T6, TICK0S, lemniscate_table, params, raw_tables, tables, track_cfg
from track_loop_ref import MUTANTS, row, track_rows, track_targets

F = np.float32
NEW, WIN = "sdempc_closed_loop_batch_tracked", "sdempc_reference_windows"


def test_abi_surface_of_the_tracked_entry_points_and_no_new_kernel():
    """FAILS before SPEC.md §11j: the library then has neither symbol."""
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    fields = ["struct_size", "n_tables", "knots", "t", "x", "period", "table_of", "phase", "rate", "offset", "tick0", "renorm", "score_targets"]
    body = re.search(r"typedef struct sdempc_track_cfg \{(.*?)\} sdempc_track_cfg;", hdr, re.S).group(1)
    assert [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.strip().splitlines()] == fields
    R = _abi.SdempcTrackCfg
    assert [f[0] for f in R._fields_] == fields and C.sizeof(R) == 88 and (R.knots.offset, R.offset.offset, R.tick0.offset, R.score_targets.offset) == (8, 64, 72, 80)
    names = lambda p: [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", p, flags=re.S).split(",")]      # noqa: E731
    proto = re.search(r"int " + NEW + r"\((.*?)\);", hdr, re.S).group(1)
    dproto = re.search(r"int sdempc_closed_loop_batch_drawn\((.*?)\);", hdr, re.S).group(1)
    assert names(proto) == ["h", "track"] + names(dproto)[1:]                  # every argument of the drawn entry point after h, in its order
    assert names(re.search(r"int " + WIN + r"\((.*?)\);", hdr, re.S).group(1)) == ["h", "track", "B", "n", "ticks", "out"]
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, NEW) and hasattr(lib, WIN)
    assert NEW in _abi.EXPORTED_SYMBOLS and WIN in _abi.EXPORTED_SYMBOLS
    fn, da = _abi.tracked_entry(lib), _abi.drawn_entry(lib).argtypes
    assert list(fn.argtypes[2:]) == list(da[1:]) and fn.argtypes[0] is da[0] and fn.argtypes[1]._type_ is R and fn.restype is C.c_int
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    for name in (NEW, WIN):
        assert re.search(r"\nint " + name + r"\([^{]*\{\n\s*return guarded\(", src)
    # the trajectory is an argument of an existing kernel: the built kernel set is the census table, in both directions
    built = kernel_census.built_kernels()
    assert built is not None and built == kernel_census.table_names()
    assert ("sdempc_broadcast_rows_kernel", "") in built


def _call(lib, h, cfg, blob, B=4, T=5, S=2, n=2, track=True, size=None, n_tables=2, knots=(3, 2), t=(0.0, 1.0, 2.0, 0.5, 0.75), x="ok", period=(2.0, 0.0),
          table_of=None, phase=None, rate=None, offset=None, tick0=0, renorm=1, targets=0, xref=False, xref_solves=0, score=False, score_ref=False, null=(), windows=None):
    """One sdempc_closed_loop_batch_tracked call (windows=int32 ticks: one sdempc_reference_windows call) on small neutral inputs; every field of the track cfg
    can be overridden. None for knots / t / x / period passes NULL."""
    fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    H, m = cfg.horizon, cfg.num_motors
    Tb, Bb = max(T, 1), max(B, 1)
    Ns = num_solves(Tb, max(S, 1))
    x0 = np.zeros((Bb, 13), F); x0[:, 6] = 1.0
    xr = np.zeros((1, 1, H + 1, 13), F); xr[..., 6] = 1.0
    k0 = np.zeros((Bb, 2), np.uint32)
    bufs_ = dict(xs=np.zeros((Bb, Tb + 1, 13), F), us=np.zeros((Bb, Tb, m), F), info=np.zeros((Bb, Ns, 8), F))
    p = {k: (None if k in null else v.ctypes.data_as(fp)) for k, v in bufs_.items()}
    kn = None if knots is None else np.asarray(knots, np.int32)
    tt = None if t is None else np.asarray(t, F)
    if isinstance(x, str):
        xx = np.zeros((max(len(t) if t is not None else 1, 1), 13), F); xx[:, 6] = 1.0
    else:
        xx = None if x is None else np.ascontiguousarray(x, F)
    pp = None if period is None else np.asarray(period, F)
    arr = lambda v, dt: None if v is None else np.ascontiguousarray(v, dt)           # noqa: E731
    of, ph, rt, off = arr(table_of, np.int32), arr(phase, F), arr(rate, F), arr(offset, F)
    ptr = lambda a, ty: None if a is None else a.ctypes.data_as(ty)                  # noqa: E731
    tk = _abi.SdempcTrackCfg(C.sizeof(_abi.SdempcTrackCfg) if size is None else size, n_tables, ptr(kn, i32p), ptr(tt, fp), ptr(xx, fp), ptr(pp, fp), ptr(of, i32p),
                             ptr(ph, fp), ptr(rt, fp), ptr(off, fp), tick0, renorm, targets)
    if windows is not None:
        wk = np.asarray(windows, np.int32)
        out = np.zeros((max(len(wk), 1), Bb, H + 1, 13), F)
        return _abi.reference_windows_entry(lib)(h, C.byref(tk) if track else None, B, len(wk), wk.ctypes.data_as(i32p), out.ctypes.data_as(fp))
    g = np.zeros((1, 1, 13), F)
    zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg), 0, 1.0, 0.5, 4.0, g.ctypes.data_as(fp) if score_ref else None, 1, 1)
    zo = np.zeros((Bb, 16), np.uint32)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S, 0, 0.0)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 1, n, 0.0, -1, -1)
    bufs = (C.c_char_p * 1)(blob)
    sz = (C.c_size_t * 1)(len(blob))
    return _abi.tracked_entry(lib)(
        h, C.byref(tk) if track else None, None, None, C.byref(zc) if score else None, None, None, None, None, None, None, None, None, None, C.byref(tc), C.byref(pc),
        C.cast(bufs, C.POINTER(C.c_void_p)), sz, None, B, T, x0.ctypes.data_as(fp), xr.ctypes.data_as(fp) if xref else None, xref_solves, 1, k0.ctypes.data_as(u32p),
        None, None, None, p["xs"], p["us"], None if p["info"] is None else C.cast(p["info"], C.POINTER(_abi.SdempcInfo)), None, None, None, None,
        None, None, None, None, None, None, None, None, None, None, zo.ctypes.data_as(u32p) if score else None, None, None, None, None, None, None)


def test_tracked_argument_checks_make_no_hip_call():
    import torch
    lib = _abi.load_library()
    cfg = track_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EDEVICE, ECAPACITY = -1, -3, -5
    B = 4
    nan, inf = float("nan"), float("inf")
    xbad = np.zeros((5, 13), F); xbad[4, 12] = nan

    def one(n, i, v, base=0.0):
        a = np.full(n, base, F)
        a[i] = v
        return a
    try:
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(size=80), EINVAL, "track: struct_size"),
            (dict(size=0, T=0), EINVAL, "track: struct_size"),                         # the track struct is looked at first
            (dict(n_tables=0), EINVAL, "n_tables"),
            (dict(knots=(3, 0)), EINVAL, "fewer than 1 knot"),
            (dict(knots=None), EINVAL, "knots, t or x is NULL"),
            (dict(t=None), EINVAL, "knots, t or x is NULL"),
            (dict(x=None), EINVAL, "knots, t or x is NULL"),
            (dict(t=(0.0, 1.0, 1.0, 0.5, 0.75)), EINVAL, "strictly increasing"),
            (dict(t=(0.0, 1.0, 2.0, 0.75, 0.5)), EINVAL, "strictly increasing"),
            (dict(t=(0.0, 1.0, 2.0, 0.5, inf)), EINVAL, "strictly increasing"),
            (dict(t=(0.0, nan, 2.0, 0.5, 0.75)), EINVAL, "strictly increasing"),
            (dict(x=xbad), EINVAL, "x holds"),
            (dict(period=(2.0, -1.0)), EINVAL, "period must be"),
            (dict(period=(inf, 0.0)), EINVAL, "period must be"),
            (dict(period=(nan, 0.0)), EINVAL, "period must be"),
            (dict(period=(2.5, 0.0)), EINVAL, "periodic table"),                       # t[L-1] != period
            (dict(t=(0.5, 1.0, 2.0, 0.5, 0.75)), EINVAL, "periodic table"),            # t[0] != 0
            (dict(table_of=(0, 1, 2, 0)), EINVAL, "table_of"),
            (dict(table_of=(0, -1, 1, 0)), EINVAL, "table_of"),
            (dict(phase=one(B, 3, nan)), EINVAL, "phase"),
            (dict(phase=one(B, 0, -inf)), EINVAL, "phase"),
            (dict(offset=one(B * 3, 11, inf)), EINVAL, "offset"),
            (dict(rate=one(B, 2, -0.5, 1.0)), EINVAL, "rate"),
            (dict(rate=one(B, 3, inf, 1.0)), EINVAL, "rate"),
            (dict(rate=one(B, 1, nan, 1.0)), EINVAL, "rate"),
            (dict(renorm=2), EINVAL, "renorm and score_targets"),
            (dict(tick0=-1), EINVAL, "tick0 must"),
            (dict(tick0=(1 << 24) - 5), EINVAL, "below 2^24"),
            (dict(tick0=(1 << 24) - 5, windows=(0, 5)), EINVAL, "2^24"),
            (dict(windows=(0, -1)), EINVAL, "tick"),
            (dict(windows=()), EINVAL, "n must"),
            (dict(windows=(0,), track=False), EINVAL, "cfg is NULL"),
            (dict(windows=(0,), size=4), EINVAL, "track: struct_size"),
            (dict(windows=(0,), rate=one(B, 2, -0.5, 1.0)), EINVAL, "rate"),
            (dict(windows=(0,), B=5), ECAPACITY, "max_batch"),
            # an array and a trajectory for the same thing
            (dict(xref=True, xref_solves=1), EINVAL, "xref must be NULL"),
            (dict(xref_solves=1), EINVAL, "xref must be NULL"),
            (dict(targets=1), EINVAL, "needs a score cfg"),
            (dict(targets=1, score=True, score_ref=True), EINVAL, "score_ref must be NULL"),
            (dict(score=True), EINVAL, "score_ref is NULL"),                           # without score_targets the score needs its array
            # everything the drawn entry point refuses, behind a valid track cfg
            (dict(null=("xs",)), EINVAL, "NULL host pointer"),
            (dict(T=0), EINVAL, "T must"),
            (dict(B=5), ECAPACITY, "max_batch"),
            (dict(S=0), EINVAL, "solve_period"),
            (dict(track=False), EINVAL, "xref_solves must be"),                        # no track and no xref: the drawn call's own refusal
        ]
        for kw, want, word in cases:
            rc = _call(lib, h, cfg, blob, **kw)
            msg = lib.sdempc_last_error(h).decode()
            assert rc == want, (sorted(kw), rc, msg)
            assert word in msg, (word, msg)
            assert lib.sdempc_device_ready(h) == 0
        # valid arguments reach the device
        good = 0 if torch.cuda.is_available() else EDEVICE
        for kw in (dict(), dict(period=None), dict(table_of=(0, 1, 1, 0), phase=one(B, 1, -3.0), rate=one(B, 0, 0.0, 1.0), offset=one(B * 3, 2, 5.0)), dict(renorm=0),
                   dict(targets=1, score=True, null=("xs", "us", "info")), dict(tick0=(1 << 24) - 6), dict(windows=(0, 7)), dict(track=False, xref=True, xref_solves=1),
                   dict(n_tables=1, knots=(1,), t=(3.0,), period=(0.0,))):
            rc = _call(lib, h, cfg, blob, **kw)
            assert rc == good, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_checks_the_track_keywords():
    cfg = track_cfg()
    model = synthetic_iris()
    B, T = 3, 5
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    tr = tables()
    with pytest.raises(ValueError, match="xref must be None"):
        S.closed_loop(x0, xref, k, T, track=tr[0])
    for kw in (dict(track_of=np.zeros(B, np.int32)), dict(track_phase=0.5), dict(track_rate=np.ones(B, F)), dict(track_offset=np.zeros(3, F)), dict(track_tick0=0),
               dict(track_renorm=False), dict(score=Score(), score_ref="track")):
        with pytest.raises(ValueError, match="need track=Trajectory"):
            S.closed_loop(x0, xref, k, T, **kw)
    for kw in (dict(track=(0.0, 1.0)), dict(track=[]), dict(track=tr, track_of=np.full(B, 4)), dict(track=tr, track_of=np.zeros(B + 1, np.int32)), dict(track=tr[0], track_rate=-1.0),
               dict(track=tr[0], track_phase=np.nan), dict(track=tr[0], track_offset=np.zeros((B, 2), F)), dict(track=tr[0], track_tick0=-1),
               dict(track=tr[0], track_tick0=(1 << 24) - T), dict(track=tr[0], score_ref="track")):
        with pytest.raises(ValueError):
            S.closed_loop(x0, None, k, T, **kw)
    for bad in (dict(ticks=[]), dict(ticks=[-1]), dict(ticks=[1 << 24]), dict(ticks=[0], B=0)):
        with pytest.raises(ValueError):
            S.reference_windows(tr, **{"B": B, **bad})
    assert not S.device_ready()
    S.close()
    t, x, _ = raw_tables()[1]
    for bad in (dict(t=t[::-1], x=x), dict(t=t, x=x[:, :12]), dict(t=t, x=x, period=-1.0), dict(t=t, x=x, period=1.0), dict(t=np.r_[t[:4], np.inf], x=x),
                dict(t=t, x=np.where(np.arange(13) == 3, np.nan, x)), dict(t=t[:0], x=x[:0])):
        with pytest.raises(ValueError):
            Trajectory.from_knots(**bad)
    prob = MpcProblem(cfg=cfg, model=model)
    with pytest.raises(ValueError, match="need track"):
        prob.simulate(np.zeros(13, F), np.zeros(2, np.uint32), T, track_rate=1.0)
    with pytest.raises(ValueError, match="no trajectory"):
        prob.trajectory(0.0, 1.0, 5)


def test_routing_of_the_track_keywords(monkeypatch):
    """A call without the new keywords reaches the entry point it reached before, with the same arguments; track= reaches the tracked one, with a NULL xref, and
    returns the tuple the same call returned with an array."""
    cfg = track_cfg()
    B, T, n = 3, 5, 2
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=B)
    seen = {}

    def fake(name):
        def entry(lib):
            def call(h, *args):
                seen["name"], seen["args"] = name, args
                return 0
            return call
        return entry
    for e in ("tracked", "drawn", "scored", "aged", "observed", "fault", "rate", "scenario", "timed"):
        monkeypatch.setattr(_abi, e + "_entry", fake(e))
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    g = np.zeros((T, 1, 13), F)
    tm = dict(solve_period=2, plant_substeps=n)
    from sde4mbrl_px4_amd.solver import GaussMarkov
    gd = GaussMarkov(np.arange(1.0, 7.0), 0.5, 0.05)
    before = {}
    for name, kw in (("timed", dict(tm)), ("fault", dict(tm, substep_states=True)), ("scored", dict(tm, score=Score(), score_ref=g)),
                     ("drawn", dict(tm, dist_process=gd, dist_keys=k, score=Score(), score_ref=g))):
        out = S.closed_loop(x0, xref, k, T, **kw)
        assert seen["name"] == name
        before[name] = (len(seen["args"]), [None if v is None else (v.shape, v.dtype) for v in out])
    tr = tables()
    of, ph, rt, off = params(B)
    out = S.closed_loop(x0, None, k, T, **tm, track=tr, track_of=of, track_phase=ph, track_rate=rt, track_offset=off, track_tick0=7)
    a = seen["args"]
    assert seen["name"] == "tracked" and len(a) == before["drawn"][0] + 1
    assert [(v.shape, v.dtype) for v in out] == before["timed"][1]                      # nothing new comes back
    tk = a[0]._obj
    assert (tk.struct_size, tk.n_tables, tk.tick0, tk.renorm, tk.score_targets) == (88, 4, 7, 1, 0)
    assert list(np.ctypeslib.as_array(tk.knots, (4,))) == [37, 5, 2, 1] and np.ctypeslib.as_array(tk.rate, (B,)).tobytes() == rt.tobytes()
    assert all(v is None for v in a[1:13])                                              # no process, score, age, obs, fault, rate or scenario cfg
    i = 1 + 17                                                                          # h is not in args: track, 2 procs, score 2, age 2, obs 3, fault, rate, scenario, timing, plant cfg, blobs, sizes, plant_of
    assert (a[i], a[i + 1]) == (B, T) and a[i + 3] is None and a[i + 4] == 0            # xref NULL, xref_solves 0
    # defaults: every per-episode pointer NULL, one table
    out = S.closed_loop(x0, None, k, T, **tm, track=tr[1], score=Score(), score_ref="track", outputs=False)
    tk = seen["args"][0]._obj
    assert (tk.n_tables, tk.tick0, tk.renorm, tk.score_targets) == (1, 0, 1, 1) and not tk.table_of and not tk.phase and not tk.rate and not tk.offset
    zc = seen["args"][3]._obj
    assert not zc.score_ref
    assert [None if v is None else (v.shape, v.dtype) for v in out] == [None, None, None] + before["scored"][1][3:]
    assert not S.device_ready()
    S.close()


def test_simulate_passes_a_trajectory_through(monkeypatch):
    cfg = track_cfg()
    prob = MpcProblem(cfg=cfg, model=synthetic_iris(), state_from_traj=W.lemniscate_state, convert_to_enu=False)
    tr = prob.trajectory(0.0, 8.0, 33, period=8.0)
    assert isinstance(tr, Trajectory) and tr.t.shape == (33,) and tr.period == F(8.0) and bits_differ(tr.x, W.lemniscate_state(np.linspace(0.0, 8.0, 33))) == 0
    seen = {}

    class Fake:
        def closed_loop(self, x0, xref, keys, T, **kw):
            seen.update(kw, xref=xref)
            B = 1
            return (np.zeros((B, T + 1, 13), F), np.zeros((B, T, 4), F), np.zeros((B, T, 8), F), np.zeros((B, cfg.horizon, 4), F), np.zeros(B, F), np.zeros((B, 2), np.uint32),
                    np.zeros((B, 4), F), np.zeros(B, np.dtype(_abi.SCORE_FIELDS)))
    monkeypatch.setattr(prob, "solver", lambda: Fake())
    x = np.zeros(13, F); x[6] = 1.0
    out = prob.simulate(x, np.zeros(2, np.uint32), 4, curr_t=0.35, track=tr, track_phase=0.5, track_rate=1.5, score=Score())
    assert seen["xref"] is None and seen["track"] is tr and seen["track_tick0"] == 7 and seen["track_phase"] == 0.5 and seen["track_rate"] == 1.5 and seen["score_ref"] == "track"
    assert len(out) == 6


@pytest.fixture(scope="module")
def rows():
    """The windows and targets of the committed cases: B = 5, T = 6, S = 2 at both tick0 values, every table shift."""
    ts = np.asarray(track_cfg().time_steps)
    tb = raw_tables()
    out = {}
    for tick0 in TICK0S:
        for shift in range(4):
            of, ph, rt, off = params(B5, shift)
            par = dict(table_of=of, phase=ph, rate=rt, offset=off)
            out[tick0, shift] = (par, track_rows(tb, ts, [tick0 + j * S2 for j in range(num_solves(T6, S2))], B5, **par), track_targets(tb, ts, [tick0 + k for k in range(T6)], B5, **par))
    return ts, tb, out


@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_generators_differ_on_the_cases(rows, mutant):
    """Each of the ten wrong generators changes a bit of the windows or the targets of the five episodes (shift 0), at tick0 = 0 or 1000."""
    ts, tb, out = rows
    d = 0
    for tick0 in TICK0S:
        par, win, tgt = out[tick0, 0]
        d += bits_differ(track_rows(tb, ts, [tick0 + j * S2 for j in range(num_solves(T6, S2))], B5, mutant=mutant, **par), win)
        d += bits_differ(track_targets(tb, ts, [tick0 + k for k in range(T6)], B5, mutant=mutant, **par), tgt)
    assert d > 0, mutant


def test_the_cases_hold_what_the_mutants_need(rows):
    ts, tb, out = rows
    from track_loop_ref import clock, offsets
    assert bits_differ(offsets(ts)[:len(ts) + 1], offsets(ts, "c_float32")[:len(ts) + 1]) > 0         # the two sums for c differ inside the window
    assert clock(1000, ts[0]) != clock(1000, ts[0], "clock_accumulated")                            # and the clock's rounding matters at tick0 = 1000
    par, win, tgt = out[0, 0]
    raw = track_rows(tb, ts, [0], B5, **dict(par, renorm=False))
    nrm = np.linalg.norm(raw[0, :, :, 6:10].astype(np.float64), axis=-1)
    assert nrm.min() < 0.99                                                                          # visibly non-unit before the renormalisation
    assert np.abs(np.linalg.norm(win[..., 6:10].astype(np.float64), axis=-1) - 1.0).max() < 3e-7
    t37 = tb[0][0]
    assert par["phase"][0] == t37[5] and bits_differ(raw[0, 0, 0], tb[0][1][5]) == 0                 # episode 0 starts ON a knot
    assert par["rate"][3] == 0 and bits_differ(win[:, 3], np.broadcast_to(win[0, 3, 0], win[:, 3].shape)) == 0      # a held point: every row of every window
    assert len({len(t[0]) for t in tb}) == 4 and sorted(len(t[0]) for t in tb) == [1, 2, 5, 37]
    for t, x, p in tb[:3]:
        assert len(set(np.diff(t.astype(np.float64)).round(6))) == len(t) - 1                       # non-uniform spacing


def test_a_row_at_a_knot_is_the_knot_bit_for_bit():
    """tau equal to t[i]: a = 0 and fma(0, dx, x[i]) = x[i], for every knot that starts a segment (and the only knot of a one-knot table), through the reference
    and through solver.Trajectory. The LAST knot of a clamped table is reached from the segment before it, with a = fl((t[L-1] - t[L-2]) w), which need not be 1
    to the last bit; tau = period of a periodic table wraps to 0 and gives the first knot exactly."""
    for (t, x, p), tr in zip(raw_tables(), tables()):
        for i in range(len(t)):
            if len(t) > 1 and i == len(t) - 1 and not p > 0:
                continue
            y = row((t, x, p), F(0.0), t[i], F(1.0), np.zeros(3, F), renorm=False)
            want = x[i] if not (p > 0 and i == len(t) - 1) else x[0]
            assert bits_differ(y, want) == 0, (len(t), i)
            assert bits_differ(tr.rows(F(0.0), t[i], 1.0, renorm=False), want) == 0, (len(t), i)


def test_trajectory_windows_are_the_reference(rows):
    """solver.Trajectory.windows / .targets (vectorised, searchsorted) against track_rows / track_targets (one row at a time, the stated bisection)."""
    ts, tb, out = rows
    tr = tables()
    for (tick0, shift), (par, win, tgt) in out.items():
        for b in range(B5):
            T = tr[par["table_of"][b]]
            got = T.windows(ts, [tick0 + j * S2 for j in range(num_solves(T6, S2))], par["phase"][b], par["rate"][b], par["offset"][b])
            assert bits_differ(got, win[:, b]) == 0, (tick0, shift, b)
            got = T.targets(ts, [tick0 + k for k in range(T6)], par["phase"][b], par["rate"][b], par["offset"][b])
            assert bits_differ(got, tgt[:, b]) == 0, (tick0, shift, b)
    # renorm off and the defaults
    w0 = tr[0].windows(ts, [3], renorm=False)
    assert bits_differ(w0, track_rows(tb, ts, [3], 1, renorm=False)[:, 0]) == 0


def test_trajectory_constructors():
    t, x, _ = raw_tables()[1]
    flipped = x.copy()
    flipped[2, 6:10] = -flipped[2, 6:10]
    flipped[3, 6:10] = -flipped[3, 6:10]
    tr = Trajectory.from_knots(t, flipped)
    assert bits_differ(tr.x, x) == 0                     # signs flipped back by exact negation, nothing else touched
    assert flipped[2, 6] == -x[2, 6]                     # (the caller's array is not written)
    with pytest.raises(ValueError, match="spans one period"):
        Trajectory.from_function(W.lemniscate_state, 1.0, 9.0, 17, period=1.0)
    fn = Trajectory.from_function(W.lemniscate_state, 1.0, 9.0, 17, period=8.0)
    assert fn.t[0] == 0 and fn.t[-1] == fn.period == F(8.0) and bits_differ(fn.x, W.lemniscate_state(np.linspace(1.0, 9.0, 17))) == 0
    one = Trajectory.from_function(W.lemniscate_state, 2.0, 2.0, 1)
    assert one.t.shape == (1,) and bits_differ(one.windows([0.1, 0.1], [0, 5], renorm=False), np.broadcast_to(one.x[0], (2, 3, 13))) == 0

    class Csv:
        t = np.array([2.0, 2.5, 4.0])

        def state(self, s):
            return W.lemniscate_state(s)
    c = Trajectory.from_csv(Csv())
    assert np.array_equal(c.t, np.array([0.0, 0.5, 2.0], F)) and bits_differ(c.x, W.lemniscate_state(Csv.t)) == 0
    assert Trajectory.from_csv(Csv(), n=9).t.shape == (9,)


def test_reference_against_a_float64_interpolant():
    """track_rows on the 37-knot lemniscate (rate 1, phase 0, no offset, no renormalisation, clock values below the period: tau = u exactly) against the float64
    linear interpolant of the SAME float32 knots at the SAME clock values. The bound is derived, not measured. With eps = 2^-24 (unit roundoff), D the largest
    |x[i+1][c] - x[i][c]| and M the largest |x[i][c]| of the table, and a* = (tau - t[i]) / (t[i+1] - t[i]) in [0, 1]:
      d  = fl(tau - t[i])          = (tau - t[i]) (1 + e1)
      w  = fl(1 / (t[i+1] - t[i])) = (1 / (t[i+1] - t[i])) (1 + e2)            (formed in float64, one rounding to float32)
      a  = fl(d w)                 = a* (1 + e1)(1 + e2)(1 + e3)               so |a - a*| <= 3 eps + O(eps^2)
      dx = fl(x[i+1] - x[i])       = (x[i+1] - x[i]) (1 + e4)
      y  = fl(a dx + x[i])         = (a dx + x[i]) (1 + e5)                    (one rounding: an fma)
    so |a dx - a* (x[i+1] - x[i])| <= (3 eps + eps + O(eps^2)) D and |y - y*| <= 4 eps D + eps (M + 4 eps D) + O(eps^2): below eps (4.1 D + 1.1 M), the
    second-order terms (a few eps^2 (D + M), nine orders below) and the float64 interpolant's own error (2^-53 relative) inside the 0.1 margins. With M near
    1.6 and D near 0.35 that is about two ulps of the largest component."""
    t, x, p = lemniscate_table()
    ts = np.asarray(track_cfg().time_steps)
    ticks = list(range(0, 140, 3))
    from track_loop_ref import clock, offsets
    c = offsets(ts)[:len(ts) + 1]
    u = np.array([[F(clock(k, ts[0]) + ci) for ci in c] for k in ticks], F)
    assert u.max() < p
    got = track_rows([(t, x, p)], ts, ticks, 1, renorm=False)[:, 0].astype(np.float64)
    t64, x64, u64 = t.astype(np.float64), x.astype(np.float64), u.astype(np.float64)
    i = np.clip(np.searchsorted(t64, u64, side="right") - 1, 0, len(t) - 2)
    a = ((u64 - t64[i]) / (t64[i + 1] - t64[i]))[..., None]
    want = x64[i] + a * (x64[i + 1] - x64[i])
    eps = 2.0 ** -24
    D, M = np.abs(np.diff(x64, axis=0)).max(), np.abs(x64).max()
    bound = eps * (4.1 * D + 1.1 * M)
    assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
    assert bound < 4 * np.spacing(F(M))                  # a few float32 ulps of the largest component
