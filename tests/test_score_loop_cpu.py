"""Episode scores formed on the device (SPEC.md §11h) without a GPU: header / binding / library agree on the new symbol at ABI version 3 and no kernel was added,
every refusal of sdempc_closed_loop_batch_scored (no HIP call may happen before them) and of the Python surface, the positions of the score in the returned
tuples, the rounding of Score's thresholds, the reference of tests/score_loop_ref.py against a direct float64 evaluation, the conditions the cases of
tests/score_cases.py must meet (every cause bit set somewhere and clear somewhere, ...), the discrimination of six wrong scores on those cases, continuation of
the reference through score_in, and score_summary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_census
from age_loop_ref import age_loop_ref
from cases import ROOT
from loop_cases import REF_NAME
from score_cases import B5, FINITE, S2, T5, T6, score_cfg, scored_episodes, targets, thresholds_from, together
from score_loop_ref import MUTANTS, WORDS, as_words, initial_rows, row_terms, score_rows, words_differ
from sde4mbrl_px4_amd import _abi, synthetic_iris
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, Score, SdeMpcSolver, score_init, score_summary
from sde4mbrl_px4_amd.utils import enu2ned
from timed_loop_ref import num_solves

F = np.float32
NEW = "sdempc_closed_loop_batch_scored"
W = {n: i for i, (n, _) in enumerate(_abi.SCORE_FIELDS)}


def ref(cfg, model, x0, xref, keys, T, **kw):
    """age_loop_ref for the keyword arguments of SdeMpcSolver.closed_loop, always with xsub as the last value."""
    return age_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T, substep_states=True, **{"plants": None, **{REF_NAME.get(k, k): v for k, v in kw.items()}})


def test_abi_surface_of_the_scored_entry_point_and_no_new_kernel():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_score_cfg \{[^}]*struct_size;[^}]*substeps;[^}]*r2_pos;[^}]*cos_min;[^}]*w2_max;[^}]*const float\* score_ref;[^}]*ref_ticks;"
                     r"[^}]*ref_batch;[^}]*\}", hdr)
    R = _abi.SdempcScoreCfg
    assert C.sizeof(R) == 40 and (R.substeps.offset, R.r2_pos.offset, R.cos_min.offset, R.w2_max.offset, R.score_ref.offset, R.ref_ticks.offset, R.ref_batch.offset) == \
        (4, 8, 12, 16, 24, 32, 36)
    assert int(re.search(r"#define\s+SDEMPC_SCORE_WORDS\s+(\d+)", hdr).group(1)) == 16 == _abi.SCORE_WORDS == len(_abi.SCORE_FIELDS) == WORDS
    assert SCORE_DTYPE.itemsize == 64 and [SCORE_DTYPE.fields[n][1] for n, _ in _abi.SCORE_FIELDS] == list(range(0, 64, 4))
    assert NEW in _abi.EXPORTED_SYMBOLS and f"int {NEW}(" in hdr
    proto = re.search(r"int " + NEW + r"\((.*?)\);", hdr, re.S).group(1)
    assert re.search(r"sdempc_score_cfg\* score[^,]*,\s*const uint32_t\* score_in[^,]*,\s*const sdempc_age_cfg\* age_cfg", proto)
    assert re.search(r"float\* xhist_next[^,]*,\s*uint32_t\* score_out[^,]*$", proto.strip())
    # ... and between the two every argument of the aged entry point, in its order
    aproto = re.search(r"int sdempc_closed_loop_batch_aged\((.*?)\);", hdr, re.S).group(1)
    names = lambda p: [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", p, flags=re.S).split(",")]      # noqa: E731
    assert names(proto)[3:-1] == names(aproto)[1:] and names(proto)[0] == names(aproto)[0] == "h"
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, NEW)
    fn = _abi.scored_entry(lib)
    assert len(fn.argtypes) == len(_abi.aged_entry(lib).argtypes) + 3 and fn.restype is C.c_int
    assert fn.argtypes[1]._type_ is _abi.SdempcScoreCfg and fn.argtypes[3]._type_ is _abi.SdempcAgeCfg
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint " + NEW + r"\([^{]*\{\n\s*return guarded\(", src)
    # the scoring is an argument of an existing kernel: the built kernel set is the census table, in both directions
    built = kernel_census.built_kernels()
    assert built is not None and built == kernel_census.table_names()
    assert ("sdempc_loop_keys_period_kernel", "") in built


def _call(lib, h, cfg, blob, B=4, T=5, S=2, n=2, score=True, z_size=None, substeps=0, thr=(1.0, 0.5, 4.0), sref="ok", ref_ticks=None, ref_batch=None, z_in=False,
          z_out=None, null=(), age_cfg=False, obs=False, D=0, rate=False):
    """One sdempc_closed_loop_batch_scored call on small neutral inputs; every field of the score cfg can be overridden, and a few of the layers below. `null`
    names the per-row outputs passed as NULL."""
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    H, m = cfg.horizon, cfg.num_motors
    Tb = max(T, 1)
    Ns = num_solves(Tb, max(S, 1))
    x0 = np.zeros((B, 13), F); x0[:, 6] = 1.0
    xref = np.zeros((1, 1, H + 1, 13), F); xref[..., 6] = 1.0
    keys, qk = np.zeros((B, 2), np.uint32), np.zeros((B, 2), np.uint32)
    bufs_ = dict(xs=np.zeros((B, Tb + 1, 13), F), us=np.zeros((B, Tb, m), F), info=np.zeros((B, Ns, 8), F), ws=np.zeros((B, Tb, 4), F),
                 xsub=np.zeros((B, Tb * max(n, 1), 13), F), xmeas=np.zeros((B, Ns, 13), F))
    p = {k: (None if k in null else v.ctypes.data_as(fp)) for k, v in bufs_.items()}
    if not rate:
        p["ws"] = None
    if not obs:
        p["xmeas"] = None
    b_qn, b_xn = np.zeros((B, 2), np.uint32), np.zeros((B, 13), F)
    g = np.zeros((Tb, B, 13), F) if isinstance(sref, str) else (None if sref is None else np.ascontiguousarray(sref, F))
    zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg) if z_size is None else z_size, substeps, thr[0], thr[1], thr[2], None if g is None else g.ctypes.data_as(fp),
                             (1 if g is None else g.shape[0]) if ref_ticks is None else ref_ticks, (1 if g is None else g.shape[1]) if ref_batch is None else ref_batch)
    zi, zo = initial_rows(B), np.zeros((B, 16), np.uint32)
    z_out = score if z_out is None else z_out
    ac = _abi.SdempcAgeCfg(C.sizeof(_abi.SdempcAgeCfg), None, 1, 1, 0, 1)
    sg = np.full((1, 1, 12), 0.01, F)
    oc = _abi.SdempcObsCfg(C.sizeof(_abi.SdempcObsCfg), sg.ctypes.data_as(fp), None, 1, 1, None, 1, 1)
    rc_ = _abi.SdempcRateCfg()
    rc_.struct_size = C.sizeof(_abi.SdempcRateCfg)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S, D, 0.0)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 1, n, 0.0, -1, -1)
    bufs = (C.c_char_p * 1)(blob)
    sz = (C.c_size_t * 1)(len(blob))
    return _abi.scored_entry(lib)(
        h, C.byref(zc) if score else None, zi.ctypes.data_as(u32p) if z_in else None, C.byref(ac) if age_cfg else None, None,
        C.byref(oc) if obs else None, qk.ctypes.data_as(u32p) if obs else None, None, None, C.byref(rc_) if rate else None, None, C.byref(tc), C.byref(pc),
        C.cast(bufs, C.POINTER(C.c_void_p)), sz, None, B, T, x0.ctypes.data_as(fp), xref.ctypes.data_as(fp), 1, 1, keys.ctypes.data_as(u32p), None, None, None,
        p["xs"], p["us"], None if p["info"] is None else C.cast(p["info"], C.POINTER(_abi.SdempcInfo)), None, None, None, None,
        None, None, p["ws"], None, None, p["xsub"],
        p["xmeas"], b_qn.ctypes.data_as(u32p) if obs else None, b_xn.ctypes.data_as(fp) if obs else None, None, zo.ctypes.data_as(u32p) if z_out else None)


def test_scored_argument_checks_make_no_hip_call():
    import torch
    lib = _abi.load_library()
    cfg = score_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EDEVICE, ECAPACITY = -1, -3, -5
    B, T = 4, 5
    nan, inf = float("nan"), float("inf")
    try:
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(z_size=32), EINVAL, "score: struct_size"),
            (dict(z_size=32, T=0), EINVAL, "score: struct_size"),                      # the struct is looked at first
            (dict(substeps=2), EINVAL, "score: substeps"),
            (dict(substeps=-1), EINVAL, "score: substeps"),
            (dict(ref_ticks=0), EINVAL, "ref_ticks"),
            (dict(ref_ticks=3), EINVAL, "ref_ticks"),
            (dict(sref=np.zeros((3, B, 13), F)), EINVAL, "ref_ticks"),               # Ns rows instead of T
            (dict(ref_batch=0), EINVAL, "ref_batch"),
            (dict(ref_batch=B + 1), EINVAL, "ref_batch"),
            (dict(sref=np.zeros((T, 2, 13), F)), EINVAL, "ref_batch"),
            (dict(sref=None), EINVAL, "score_ref is NULL"),
            (dict(z_out=False), EINVAL, "score_out is NULL"),
            (dict(thr=(nan, 0.5, 4.0)), EINVAL, "threshold is NaN"),
            (dict(thr=(1.0, nan, 4.0)), EINVAL, "threshold is NaN"),
            (dict(thr=(1.0, 0.5, nan)), EINVAL, "threshold is NaN"),
            # score pointers and NULL per-row outputs without a cfg
            (dict(score=False, z_in=True), EINVAL, "without a score cfg"),
            (dict(score=False, z_out=True), EINVAL, "without a score cfg"),
            (dict(score=False, null=("xs",)), EINVAL, "NULL host pointer"),
            (dict(score=False, null=("us",)), EINVAL, "NULL host pointer"),
            (dict(score=False, null=("info",)), EINVAL, "NULL host pointer"),
            (dict(score=False, rate=True, null=("ws",)), EINVAL, "ws is NULL"),
            # everything the aged entry point refuses, behind a valid score cfg
            (dict(age_cfg=True), EINVAL, "needs an obs cfg"),
            (dict(D=5), EINVAL, "solve_delay"),
            (dict(T=0, sref=np.zeros((1, 1, 13), F)), EINVAL, "T must"),
            (dict(B=5), ECAPACITY, "max_batch"),
            (dict(n=0), EINVAL, "substeps"),
        ]
        for kw, want, word in cases:
            rc = _call(lib, h, cfg, blob, **kw)
            msg = lib.sdempc_last_error(h).decode()
            assert rc == want, (sorted(kw), rc, msg)
            assert word in msg, (word, msg)
            assert lib.sdempc_device_ready(h) == 0
        # valid arguments reach the device: every NULL that is allowed, the four shapes of score_ref, thresholds that are off, a NULL cfg (the aged call)
        good = 0 if torch.cuda.is_available() else EDEVICE
        every = ("xs", "us", "info", "ws", "xsub", "xmeas")
        for kw in (dict(), dict(substeps=1), dict(sref=np.zeros((1, B, 13), F)), dict(sref=np.zeros((T, 1, 13), F)), dict(sref=np.zeros((1, 1, 13), F)),
                   dict(thr=(inf, -inf, inf)), dict(thr=(0.0, 1.0, 0.0)), dict(z_in=True), dict(null=every), dict(null=every, obs=True, age_cfg=True, substeps=1),
                   dict(null=("us",)), dict(score=False), dict(score=False, obs=True, age_cfg=True), dict(T=1, sref=np.zeros((1, B, 13), F))):
            rc = _call(lib, h, cfg, blob, **kw)
            assert rc == good, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_checks_the_score_keywords():
    cfg = score_cfg()
    model = synthetic_iris()
    B, T = 3, 5
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    g = np.zeros((T, B, 13), F)
    for kw in (dict(score_ref=g), dict(score_in=score_init(B)), dict(outputs=False)):                # each needs score
        with pytest.raises(ValueError, match="need score"):
            S.closed_loop(x0, xref, k, T, **kw)
    for kw in (dict(score=1.0, score_ref=g), dict(score=Score()), dict(score=Score(), score_ref=g[:3]), dict(score=Score(), score_ref=g[:, :2]),
               dict(score=Score(), score_ref=np.zeros((B, 13), F)), dict(score=Score(), score_ref=g[..., :12]), dict(score=Score(), score_ref=g, score_in=score_init(2)),
               dict(score=Score(), score_ref=g, score_in=np.zeros((B, 16), np.uint32))):
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    for bad in (dict(pos_radius=-1.0), dict(tilt_max=float("nan")), dict(rate_max=-0.5)):
        with pytest.raises(ValueError):
            Score(**bad)
    assert not S.device_ready()
    S.close()
    prob = MpcProblem(cfg=cfg, model=model)
    with pytest.raises(ValueError, match="needs score"):
        prob.simulate(np.zeros(13, F), np.zeros(2, np.uint32), T, score_ref=np.zeros(13, F))
    with pytest.raises(ValueError, match="score_ref must be"):
        prob.simulate(np.zeros(13, F), np.zeros(2, np.uint32), T, score=Score(), score_ref=np.zeros((T - 1, 13), F))


def test_tuple_positions_of_the_score_and_null_outputs(monkeypatch):
    """The score sits behind every other value and in front of xsub; outputs=False passes NULL for the six per-row outputs and returns None in their places; a
    call without score keywords does not reach the new entry point."""
    cfg = score_cfg()
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
    for e in ("scored", "aged", "observed", "fault"):
        monkeypatch.setattr(_abi, e + "_entry", fake(e))
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    g = np.zeros((T, 1, 13), F)
    obs = dict(meas_noise=np.full(12, 0.01, F), meas_keys=k)
    tm = dict(solve_period=2, plant_substeps=n)
    out = S.closed_loop(x0, xref, k, T, **tm, **obs, meas_age=1)
    assert seen["name"] == "aged" and len(out) == 11
    n_aged = len(seen["args"])
    sc = Score(pos_radius=2.0, tilt_max=1.0, rate_max=3.0, substeps=True)
    out = S.closed_loop(x0, xref, k, T, **tm, score=sc, score_ref=g)                                  # nothing observed: NULL obs and age cfgs
    a = seen["args"]
    assert seen["name"] == "scored" and len(a) == n_aged + 3 and len(out) == 8 and out[-1].dtype == SCORE_DTYPE and out[-1].shape == (B,)
    zc = a[0]._obj
    assert (zc.struct_size, zc.substeps, zc.ref_ticks, zc.ref_batch) == (40, 1, T, 1) and (F(zc.r2_pos), F(zc.cos_min), F(zc.w2_max)) == sc.thresholds()
    assert a[1] is None and a[2] is None and a[3] is None and a[4] is None and a[-1] is not None
    out = S.closed_loop(x0, xref, k, T, **tm, **obs, meas_age=1, substep_states=True, rate_loop=None, score=Score(), score_ref=g[0, 0], score_in=score_init(B))
    a = seen["args"]
    assert len(out) == 13 and out[-2].dtype == SCORE_DTYPE and out[-1].shape == (B, T * n, 13) and out[-3].shape == (B, 1, 13)
    assert a[1] is not None and a[2] is not None and (a[0]._obj.ref_ticks, a[0]._obj.ref_batch, a[0]._obj.substeps) == (1, 1, 0)
    from rate_loop_cases import rate_loop
    out = S.closed_loop(x0, xref, k, T, **tm, **obs, substep_states=True, rate_loop=rate_loop("soft"), score=Score(), score_ref=g, outputs=False)
    names = ("xs", "us", "info", "u_next", "stepsize_next", "keys_next", "u_act_next", "ws", "rate_integ_next", "rate_tail_next", "xmeas", "meas_keys_next", "xmeas_next",
             "score", "xsub")
    assert len(out) == len(names)
    for nm, v in zip(names, out):
        assert (v is None) == (nm in ("xs", "us", "info", "ws", "xmeas", "xsub")), nm
    a = seen["args"]
    at = lambda i: a[i] is None                       # noqa: E731  (positions in the C call, counted from the end: ..., xsub, xmeas, q_next, xm_next, xhist_next, score_out)
    assert at(-6) and at(-5) and not at(-4) and not at(-3) and at(-2) and not at(-1)
    out = S.closed_loop(x0, xref, k, T, **tm, substep_states=True)
    assert seen["name"] == "fault" and len(out) == 8
    assert not S.device_ready()
    S.close()


def test_score_thresholds_are_computed_in_float64_and_rounded_once():
    s = Score()
    assert s.thresholds() == (F(np.inf), F(-np.inf), F(np.inf)) and not s.substeps
    assert Score(tilt_max=4.0).cos_min == F(-np.inf) and Score(tilt_max=np.pi).cos_min == F(-np.inf)
    assert Score(pos_radius=0.0, tilt_max=0.0, rate_max=0.0).thresholds() == (F(0.0), F(1.0), F(0.0))
    rng = np.random.default_rng(5)
    twice = 0
    for r, t, w in zip(rng.uniform(0.01, 30.0, 400), rng.uniform(0.0, 3.1, 400), rng.uniform(0.01, 60.0, 400)):
        s = Score(pos_radius=r, tilt_max=t, rate_max=w)
        assert s.r2_pos == F(np.float64(r) ** 2) and s.cos_min == F(np.cos(np.float64(t))) and s.w2_max == F(np.float64(w) ** 2)
        assert all(v.dtype == F for v in s.thresholds())
        twice += s.r2_pos != F(F(r) * F(r))
    assert twice > 0                                   # squaring the rounded radius is a different number often enough to matter
    assert Score(pos_radius=1e30).r2_pos == F(np.inf)  # an overflowing square switches the criterion off


@pytest.fixture(scope="module")
def shared():
    """The oracle loops every test below needs, computed once: the episodes of score_cases.py at T = 6 (whole periods) and T = 5 (a ragged last period), and one
    run with a fault, a gust, a plant switch and an aged measurement through a rate loop."""
    cfg = score_cfg()
    model = synthetic_iris()
    x0, xref, keys, kw = scored_episodes(cfg, B5, 171)
    runs = {T: ref(cfg, model, x0, xref, keys, T, **kw) for T in (T5, T6)}
    runs["together"] = ref(cfg, model, x0, xref, keys, T5, **kw, **together(model, x0, cfg.horizon, "stiff"))
    return cfg, model, x0, xref, keys, kw, runs


def scores_of(cfg, run, g, score, T, substeps, **more):
    return score_rows(run[0], run[1], run[2], run[-1], g, cfg, score.thresholds(), substeps, S2, **more)


def test_reference_against_a_float64_evaluation(shared):
    """row_terms and the sums of score_rows against the same quantities in float64, to float32 rounding; the counters exactly."""
    cfg, model, x0, xref, keys, kw, runs = shared
    xs, us, info, xsub = runs[T5][0], runs[T5][1], runs[T5][2], runs[T5][-1]
    g = targets(xref, T5)
    off = Score()
    for substeps in (False, True):
        z = scores_of(cfg, runs[T5], g, off, T5, substeps)
        rows = xsub if substeps else xs[:, 1:]
        n = rows.shape[1] // T5
        for b in FINITE:
            x = rows[b].astype(np.float64)
            gg = np.repeat(g[:, b].astype(np.float64), n, axis=0)
            dp = ((x[:, :3] - gg[:, :3]) ** 2).sum(1)
            c = 1.0 - 2.0 * (x[:, 7] ** 2 + x[:, 8] ** 2)
            w2 = (x[:, 10:13] ** 2).sum(1)
            f = z[b].view(F)
            assert z[b, W["rows"]] == T5 * n and z[b, W["first_fail_row"]] == 0xFFFFFFFF and z[b, W["causes"]] == 0 and z[b, W["fail_rows"]] == 0
            np.testing.assert_allclose(f[W["sum_dp"]], dp.sum(), rtol=1e-5)
            np.testing.assert_allclose(f[W["max_dp"]], dp.max(), rtol=1e-6)
            assert z[b, W["max_dp_row"]] == int(np.argmax(dp))
            np.testing.assert_allclose(f[W["last_dp"]], dp[-1], rtol=1e-6)
            np.testing.assert_allclose(f[W["sum_dv"]], ((x[:, 3:6] - gg[:, 3:6]) ** 2).sum(), rtol=1e-5)
            np.testing.assert_allclose(f[W["min_cos_tilt"]], c.min(), rtol=1e-6)
            np.testing.assert_allclose(f[W["max_w2"]], w2.max(), rtol=1e-6)
            u = us[b].astype(np.float64)
            np.testing.assert_allclose(f[W["sum_du2"]], ((u - np.asarray(cfg.uref, np.float64)) ** 2).sum(), rtol=1e-5, atol=1e-12)
            assert z[b, W["sum_steps"]] == int(info[b, :, 2].sum()) and z[b, W["sum_ls_trials"]] == int(info[b, :, 7].sum())
    # the substep rows at the tick ends are the tick rows
    n = xsub.shape[1] // T5
    assert xsub[:, n - 1::n].tobytes() == xs[:, 1:].tobytes()
    assert row_terms(np.full(13, np.nan, F), g[0, 0])[4] and row_terms(np.r_[np.zeros(12, F), F(-np.inf)], g[0, 0])[4] and not row_terms(np.zeros(13, F), g[0, 0])[4]


@pytest.mark.parametrize("substeps", [False, True], ids=["ticks", "substeps"])
def test_the_cases_set_and_clear_every_bit(shared, substeps):
    """What score_cases.py promises, on the oracle's own trajectories: each of the cause bits 1, 2 and 4 set in at least one episode and clear in at least one, words 11
    and 15 non-zero in one episode and zero in another, the non-finite episodes end with cause bit 8 and nothing else does."""
    cfg, model, x0, xref, keys, kw, runs = shared
    for T in (T5, T6):
        run = runs[T]
        g = targets(xref, T)
        score = thresholds_from(run[0], run[-1], g, substeps=substeps)
        z = scores_of(cfg, run, g, score, T, substeps)
        causes = z[:, W["causes"]]
        for bit in (1, 2, 4):
            assert (causes[list(FINITE)] & bit != 0).any() and (causes[list(FINITE)] & bit == 0).any(), (bit, causes)
        assert (causes[[3, 4]] & 8 == 8).all() and (causes[list(FINITE)] & 8 == 0).all() and (causes[[3, 4]] & 1 == 1).all()
        assert z[3, W["first_fail_row"]] == 0 and z[4, W["first_fail_row"]] == 0 and z[3, W["fail_rows"]] == z[3, W["rows"]]
        assert np.isinf(z[3].view(F)[W["max_dp"]]) and z[3, W["max_dp_row"]] == 0                   # tied from row 0 on: the first occurrence
        assert np.isnan(z[4].view(F)[W["sum_dp"]]) and z[4].view(F)[W["max_dp"]] == 0.0             # a NaN never becomes the maximum
        sat, flat = z[:, W["saturated"]], z[:, W["no_decrease"]]
        assert sat[1] >= cfg.num_motors and sat[0] == 0, sat
        assert flat[2] == num_solves(T, S2) and flat[3] == num_solves(T, S2) and flat[0] == 0 and flat[1] == 0, flat
        assert (z[list(FINITE), W["sum_steps"]] > 0).all() and z[3, W["sum_steps"]] == 0
        ok = causes == 0
        assert ((z[:, W["first_fail_row"]] == 0xFFFFFFFF) == ok).all() and ((z[:, W["fail_rows"]] == 0) == ok).all()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_scores_differ_on_the_cases(shared, mutant):
    cfg, model, x0, xref, keys, kw, runs = shared
    total = 0
    for T in (T5, T6):
        for substeps in (False, True):
            run = runs[T]
            g = targets(xref, T)
            score = thresholds_from(run[0], run[-1], g, substeps=substeps)
            right = scores_of(cfg, run, g, score, T, substeps)
            d = words_differ(right, scores_of(cfg, run, g, score, T, substeps, mutant=mutant))
            assert d > 0, (mutant, T, substeps)
            total += d
    assert total > 0


def test_the_score_is_per_episode_and_independent_of_the_other_rows(shared):
    """Scoring a subset of the episodes gives the subset of the scores; the four shapes of score_ref agree where their rows agree."""
    cfg, model, x0, xref, keys, kw, runs = shared
    run = runs["together"]
    g = targets(xref, T5)
    score = thresholds_from(runs[T5][0], runs[T5][-1], g)
    z = scores_of(cfg, run, g, score, T5, False)
    for eps in ([0], [4, 2], [1, 3]):
        sub = score_rows(run[0][eps], run[1][eps], run[2][eps], run[-1][eps], g[:, eps], cfg, score.thresholds(), False, S2)
        assert words_differ(sub, z[eps]) == 0
    g1 = targets(xref, T5, per_episode=False)
    assert words_differ(scores_of(cfg, run, g1, score, T5, False)[1:2], z[1:2]) == 0                # the shared column is episode 1's
    gt = targets(xref, T5, per_tick=False)
    zt = scores_of(cfg, run, gt, score, T5, True)
    assert words_differ(zt, scores_of(cfg, run, np.repeat(gt, T5, axis=0), score, T5, True)) == 0
    assert words_differ(zt, scores_of(cfg, run, g, score, T5, True)) > 0


@pytest.mark.parametrize("substeps", [False, True], ids=["ticks", "substeps"])
def test_continuation_of_the_reference(shared, substeps):
    """T = 6 at S = 2 as 4 + 2 and as 2 + 2 + 2 through score_in: word for word the score of the whole run."""
    cfg, model, x0, xref, keys, kw, runs = shared
    run = runs[T6]
    xs, us, info, xsub = run[0], run[1], run[2], run[-1]
    g = targets(xref, T6)
    score = thresholds_from(xs, xsub, g, substeps=substeps)
    whole = scores_of(cfg, run, g, score, T6, substeps)
    n = xsub.shape[1] // T6
    for cuts in ((0, 4, 6), (0, 2, 4, 6)):
        z = None
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            z = score_rows(xs[:, t0:t1 + 1], us[:, t0:t1], info[:, t0 // S2:t1 // S2], xsub[:, t0 * n:t1 * n], g[t0:t1], cfg, score.thresholds(), substeps, S2, score_in=z)
        assert words_differ(z, whole) == 0
    assert as_words(score_init(B5)).tobytes() == initial_rows(B5).tobytes()


def test_score_summary():
    z = score_init(4)
    z["rows"] = [10, 10, 5, 0]
    z["sum_dp"] = [2.5, 40.0, 0.0, 0.0]
    z["min_cos_tilt"] = [0.5, 0.0, 1.0, np.inf]
    z["first_fail_row"][1] = 3
    z["sum_steps"], z["sum_ls_trials"] = [6, 9, 3, 0], [12, 30, 3, 0]
    s = score_summary(z)
    assert s["success_rate"] == 0.75 and s["mean_steps"] is None and s["mean_ls_trials"] is None
    np.testing.assert_allclose(s["rms_pos_err"][:3], [0.5, 2.0, 0.0])
    assert np.isnan(s["rms_pos_err"][3])
    np.testing.assert_allclose(s["worst_tilt_deg"], 90.0)
    s = score_summary(z, solves=3)
    np.testing.assert_allclose([s["mean_steps"], s["mean_ls_trials"]], [18 / 12, 45 / 12])
    with pytest.raises(ValueError):
        score_summary(np.zeros((4, 16), np.uint32))


@pytest.mark.parametrize("to_enu", [False, True], ids=["solver_frame", "enu"])
def test_simulate_forwards_the_score_and_its_target(monkeypatch, to_enu):
    """MpcProblem.simulate: the default target is the reference at the END of each tick (the trajectory at curr_t + (k + 1) dt_0, else xdes); a given one is in the
    frame of x and flipped like xs; the score row sits behind the other values, xsub last."""
    from sde4mbrl_px4_amd import workload
    cfg = score_cfg()
    T, n = 4, 2
    seen = {}

    class Fake:
        def closed_loop(self, x0, xref, keys, T, **kw):
            seen.update(kw)
            z = lambda *s: np.zeros(s, F)                 # noqa: E731
            out = (z(1, T + 1, 13), z(1, T, 4), z(1, -(-T // 2), 8), z(1, cfg.horizon, 4), z(1), np.zeros((1, 2), np.uint32), z(1, 4), score_init(1))
            return out + ((z(1, T * n, 13),) if kw.get("substep_states") else ())
    x = np.zeros(13, F); x[6] = 1.0; x[:3] = (1.0, 2.0, 3.0)
    for traj in (None, workload.lemniscate_state):
        prob = MpcProblem(cfg=cfg, model=synthetic_iris(), state_from_traj=traj, convert_to_enu=to_enu)
        monkeypatch.setattr(prob, "solver", lambda: Fake())
        out = prob.simulate(x, np.zeros(2, np.uint32), T, curr_t=0.3, solve_period=2, plant_substeps=n, score=Score(), substep_states=True)
        assert len(out) == 7 and out[-2].dtype == SCORE_DTYPE and out[-1].shape == (T * n, 13)
        g = seen["score_ref"]
        if traj is None:
            want = enu2ned(x, np) if to_enu else x
            assert g.shape == (1, 1, 13) and g.tobytes() == np.asarray(want, F).tobytes()
        else:
            dt0 = float(cfg.time_steps[0])
            want = np.asarray(traj(0.3 + (np.arange(T) + 1.0) * dt0), F)
            assert g.shape == (T, 1, 13) and g[:, 0].tobytes() == want.tobytes()
        given = np.arange(T * 13, dtype=F).reshape(T, 13)
        out = prob.simulate(x, np.zeros(2, np.uint32), T, solve_period=2, plant_substeps=n, score=Score(), score_ref=given)
        assert len(out) == 6 and out[-1].dtype == SCORE_DTYPE
        assert seen["score_ref"][:, 0].tobytes() == np.asarray(enu2ned(given, np) if to_enu else given, F).tobytes()
