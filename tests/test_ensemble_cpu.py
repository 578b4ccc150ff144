"""The per-row ensemble words without a GPU (SPEC.md §11m): the cases of tests/ensemble_cases.py CAN fail — the tree sum differs from np.sum and from the plain
sequential sum, the two inclusion rules differ, episodes fail at different rows, the gust drives an episode non-finite, the empty cohort reads as stated, no
channel is -0 or NaN — and each of the ten one-line-wrong reducers of tests/ensemble_ref.py changes a compared word. Then ensemble_summary's arithmetic, the
header / EXPORTED_SYMBOLS / library agreement, every refusal of the C ABI in its documented order before a HIP call, and the routing of the Python keywords."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ensemble_cases as EC
from cases import ROOT
from ensemble_ref import BASE, MUTANTS, butterfly_sum, ens_words_differ, ensemble_ref
from score_cases import targets
from score_loop_ref import NONE, row_terms, score_rows
from sde4mbrl_px4_amd import _abi, synthetic_iris
from sde4mbrl_px4_amd.solver import Ensemble, Score, SdeMpcSolver, ensemble_summary

F = np.float32
U = np.uint32
CPU_CASES = [c for c in EC.CASES if c[0] in (1, 65, 257, 300, 600)]          # the oracle loops of the larger half are shared with nothing else here


def case(B):
    return EC.prepared(*[c for c in EC.CASES if c[0] == B][0])


@pytest.fixture(scope="module")
def continued():
    """B = 65, the oracle flown for 2 T ticks: (second-half rows, targets, final words, words after the first half, cohort, edges, thresholds) of a run
    continued through score_in, whose second call scores rows T .. 2T-1."""
    B, T = 65, 2 * EC.T4
    cfg, model, x0, xref, keys, kw = EC.inputs(B, T=T)
    want = EC.oracle_loop(cfg, model, x0, xref, keys, T, **kw)
    g = targets(xref, T)
    score = EC.thresholds_from(want[0], want[-1], g, finite=EC.finite_episodes(want[-1]))
    z_half = score_rows(want[0][:, :EC.T4 + 1], want[1][:, :EC.T4], want[2][:, :2], want[-1][:, :EC.T4 * EC.N2], g[:EC.T4], cfg, score.thresholds(), False, EC.S2)
    z_full = score_rows(want[0], want[1], want[2], want[-1], g, cfg, score.thresholds(), False, EC.S2)
    return dict(rows=want[0][:, EC.T4 + 1:], g=g[EC.T4:], z=z_full, z_half=z_half, cohort=EC.cohorts(B, 3), thr=score.thresholds(), all_rows=want[0][:, 1:], g_all=g)


def test_tree_sum_differs_from_numpy_and_from_the_sequential_sum():
    """At B = 600 (three blocks) some cell's sum differs in a bit from np.sum and from the plain left-to-right sum, and the reversed block order shows too."""
    c = case(600)
    v, nf, _ = c["terms"]
    seq = EC.reference(c, mutant="sequential_sum")
    assert ens_words_differ(seq, c["words"]) > 0
    assert ens_words_differ(EC.reference(c, mutant="blocks_reversed"), c["words"]) > 0
    cells = [np.where(~nf[i], v[i, :, k], F(0.0)).astype(F) for i in range(v.shape[0]) for k in range(4)]           # over = "all", one cohort: every finite row
    assert any(butterfly_sum(x).tobytes() != np.sum(x, dtype=F).tobytes() for x in cells)
    assert any(butterfly_sum(x).tobytes() != butterfly_sum(x, "sequential_sum").tobytes() for x in cells)


def test_inclusion_rules_differ_and_episodes_fail_at_different_rows():
    c = case(300)
    other = EC.reference(c, over=0)
    assert ens_words_differ(other, c["words"]) > 0
    assert np.array_equal(other[..., 0], c["words"][..., 0]) and (other[..., 1] >= c["words"][..., 1]).all()
    first = c["z"][:, 8]
    assert (first == 0).any() and ((first > 0) & (first != NONE)).any() and (first == NONE).any()
    # the survival curve falls over the rows and the faulted cohort is not the unfaulted one
    failed = c["words"][:, :2, 2].astype(np.int64)
    assert (np.diff(failed, axis=0) >= 0).all() and failed[-1].sum() > failed[0].sum() and not np.array_equal(c["words"][:, 0], c["words"][:, 1])


@pytest.mark.parametrize("B", [65, 257, 300, 600])
def test_empty_cohort_and_the_gust(B):
    """Cohort 2 of the G = 3 cases has no episode: (0, .., +0, +inf, -inf, ..). Episode 2's rows go non-finite after the gust of tick 1, through finite inputs."""
    c = case(B)
    w = c["words"][:, 2]
    want = np.zeros(BASE + 4 * c["E"], U)
    for k in range(4):
        want[9 + 3 * k], want[10 + 3 * k] = np.asarray([np.inf, -np.inf], F).view(U)
    assert (w == want).all()
    nf = c["terms"][1]
    assert np.isfinite(c["x0"]).all() and np.isfinite(c["kw"]["disturbance"]).all()
    assert not nf[0].any() and nf[-1, EC.GUST_EPISODE] and nf[-1].sum() == 1
    assert c["words"][-1, :, 7].sum() == 1 and c["words"][-1, 0, 7] == 1                    # (episode 2 is even: cohort 0)
    if not c["over"]:
        assert c["words"][-1, 0, 1] == c["words"][-1, 0, 0] - 1                              # every finite row is included


def test_no_channel_is_negative_zero_or_nan():
    """On the cases' finite rows, and on finite rows and targets pushed to the ends of the float32 range: no channel is NaN, none is -0 (+inf and -inf do occur), so
    "v < cur replaces" gives one minimum in any order."""
    for B in (65, 300):
        v, nf, _ = case(B)["terms"]
        fin = v[~nf]
        assert not np.isnan(fin).any() and not ((fin == 0) & np.signbit(fin)).any()
    rng = np.random.default_rng(5)
    big = np.float32(np.finfo(np.float32).max)
    pool = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, np.sqrt(0.5), big, -big, 1e-30, -1e-30, 1e-45, 3e19, -3e19], F)
    seen_inf = False
    for _ in range(400):
        x, g = rng.choice(pool, 13), rng.choice(pool, 13)
        dp, dv, c, w2, nf = row_terms(x, g)
        vals = np.array([dp, dv, c, w2], F)
        assert not nf and not np.isnan(vals).any() and not ((vals == 0) & np.signbit(vals)).any(), (x, g, vals)
        seen_inf = seen_inf or np.isinf(vals).any()
    assert seen_inf
    x = np.zeros(13, F); x[7] = F(0.5); x[8] = F(0.5)                                # c = fma(-2, 0.5, 1) = +0 exactly
    assert row_terms(x, np.zeros(13, F))[2].tobytes() == F(0.0).tobytes()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_each_wrong_reducer_changes_a_compared_word(mutant, continued):
    """The ten one-line-wrong reducers: each differs from the reference on a case the GPU test compares (the continuation for the two that need a score_in)."""
    if mutant in ("local_row_index", "first_before_scoring"):
        k = continued
        edges = case(65)["ens"].edges
        right = ensemble_ref(k["rows"], k["g"], k["z"], k["cohort"], edges, k["thr"], 3, 1)
        wrong = ensemble_ref(k["rows"], k["g"], k["z"], k["cohort"], edges, k["thr"], 3, 1, mutant=mutant, words_before=k["z_half"])
        whole = ensemble_ref(k["all_rows"], k["g_all"], k["z"], k["cohort"], edges, k["thr"], 3, 1)
        assert ens_words_differ(right, whole[EC.T4:]) == 0                              # the continuation IS rows T .. 2T-1 of the long run
        assert ens_words_differ(wrong, right) > 0
        return
    hits = 0
    for B in (300, 600):
        c = case(B)
        hits += ens_words_differ(EC.reference(c, mutant=mutant), c["words"]) > 0
    assert hits == 2 or (hits == 1 and mutant in ("blocks_reversed", "chained_block_sum", "sequential_sum")), (mutant, hits)


def test_reference_words_add_up():
    """Counts of the cohorts add up to B in every row; included <= cohort; the edge counts ascend along a channel and stay <= included."""
    for cs in CPU_CASES:
        c = EC.prepared(*cs)
        w = c["words"]
        assert (w[..., 0].sum(axis=1) == c["B"]).all() and (w[..., 1] <= w[..., 0]).all() and w.shape == (EC.T4 * c["rpt"], c["G"], BASE + 4 * c["E"])
        if c["E"]:
            cnt = w[..., BASE:].reshape(w.shape[0], w.shape[1], 4, c["E"]).astype(np.int64)
            assert (np.diff(cnt, axis=-1) >= 0).all() and (cnt <= w[..., 1, None, None]).all()


def test_ensemble_edges_and_summary_arithmetic():
    ens = Ensemble(pos_edges=[2.0, 0.5], vel_edges=[1.0], tilt_edges_deg=[10.0, 60.0, 30.0], rate_edges=[3.0], over="all", n_cohorts=2)
    assert ens.n_edges == 3 and ens.words == 32 and ens.counts == (2, 1, 3, 1)
    assert ens.edges[0].tolist() == [0.25, 4.0, np.inf] and ens.edges[1].tolist() == [1.0, np.inf, np.inf] and ens.edges[3].tolist() == [9.0, np.inf, np.inf]
    assert ens.tilt_edges_deg.tolist() == [60.0, 30.0, 10.0] and np.allclose(ens.edges[2], np.cos(np.radians([60.0, 30.0, 10.0])), rtol=1e-7)
    assert (ens.edges[:, 1:] >= ens.edges[:, :-1]).all()
    with pytest.raises(ValueError):
        Ensemble(over="dead")
    with pytest.raises(ValueError):
        Ensemble(pos_edges=[-1.0])
    with pytest.raises(ValueError):
        Ensemble(pos_edges=np.arange(17.0))
    with pytest.raises(ValueError):
        Ensemble.from_device_edges(np.array([[2.0, 1.0]] * 4, F))
    w = np.zeros((1, 2, 32), U)
    fl = w[..., 8:20].view(F)
    # cohort 0: 10 episodes, 8 included, 3 failed by now, 2 failing now (1 position, 1 tilt and rate); sums over the 8 included
    w[0, 0, :8] = [10, 8, 3, 2, 1, 1, 1, 0]
    fl[0, 0] = [8.0, 0.25, 4.0, 2.0, 0.0, 1.0, 6.0, 0.5, 1.0, 32.0, 1.0, 9.0]
    w[0, 0, 20:23] = [2, 8, 8]            # dp < 0.25, < 4, < inf
    w[0, 0, 23:26] = [6, 8, 8]            # dv < 1
    w[0, 0, 26:29] = [1, 2, 6]            # tilted more than 60, 30, 10 degrees
    w[0, 0, 29:32] = [4, 8, 8]            # w2 < 9
    fl[0, 1] = [0.0, np.inf, -np.inf] * 4
    s = ensemble_summary(w, ens, quantiles=(0.25, 0.75))
    assert s["n"].tolist() == [[10, 0]] and s["n_in"].tolist() == [[8, 0]]
    assert s["survival"][0, 0] == 0.7 and s["fail_now"][0, 0] == 0.2 and s["fail_now_by_cause"]["position"][0, 0] == 0.1 and s["fail_now_by_cause"]["nonfinite"][0, 0] == 0.0
    assert s["rms_pos"][0, 0] == 1.0 and s["rms_vel"][0, 0] == 0.5 and s["mean_cos_tilt"][0, 0] == 0.75 and s["rms_rate"][0, 0] == 2.0
    assert s["min_pos"][0, 0] == 0.5 and s["max_pos"][0, 0] == 2.0 and s["max_vel"][0, 0] == 1.0 and s["max_rate"][0, 0] == 3.0
    assert np.isclose(s["max_tilt_deg"][0, 0], 60.0) and np.isclose(s["min_tilt_deg"][0, 0], 0.0)
    assert s["cdf_pos"][0, 0].tolist() == [0.25, 1.0] and s["cdf_vel"][0, 0].tolist() == [0.75] and s["frac_tilt_above"][0, 0].tolist() == [0.125, 0.25, 0.75]
    assert s["q_pos"][0, 0].tolist() == [0.5, 2.0] and s["q_vel"][0, 0].tolist() == [1.0, 1.0] and s["q_tilt_deg"][0, 0].tolist() == [10.0, 30.0]
    assert s["q_rate"][0, 0, 0] == 3.0
    for k in ("survival", "fail_now", "rms_pos", "min_pos", "max_tilt_deg"):
        assert np.isnan(s[k][0, 1]), k
    assert np.isnan(s["q_pos"][0, 1]).all()
    with pytest.raises(ValueError):
        ensemble_summary(w[..., :31], ens)


def _names(proto):
    return [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]


def test_symbols_struct_and_header():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define SDEMPC_ABI_VERSION (\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION
    assert int(re.search(r"#define SDEMPC_ENSEMBLE_BASE_WORDS (\d+)", hdr).group(1)) == _abi.ENSEMBLE_BASE_WORDS == BASE
    body = re.search(r"typedef struct sdempc_ensemble_cfg \{(.*?)\} sdempc_ensemble_cfg;", hdr, re.S).group(1)
    fields = [re.sub(r"/\*.*?\*/", "", ln).strip().rstrip(";").split()[-1].lstrip("*") for ln in body.strip().splitlines()]
    Ec = _abi.SdempcEnsembleCfg
    assert [f[0] for f in Ec._fields_] == fields == ["struct_size", "n_cohorts", "n_edges", "over", "cohort", "edges"]
    assert C.sizeof(Ec) == 32 and Ec.cohort.offset == 16 and Ec.edges.offset == 24
    new = re.search(r"int sdempc_closed_loop_batch_ensemble\((.*?)\);", hdr, re.S).group(1)
    old = re.search(r"int sdempc_closed_loop_batch_baseline\((.*?)\);", hdr, re.S).group(1)
    assert _names(new) == ["h", "ens", "ens_out"] + _names(old)[1:]
    lib = _abi.load_library()
    assert hasattr(lib, "sdempc_closed_loop_batch_ensemble") and "sdempc_closed_loop_batch_ensemble" in _abi.EXPORTED_SYMBOLS
    assert all(hasattr(lib, s) for s in _abi.EXPORTED_SYMBOLS)
    fn, ba = _abi.ensemble_entry(lib), _abi.baseline_entry(lib).argtypes
    assert list(fn.argtypes[3:]) == list(ba[1:]) and fn.argtypes[1]._type_ is Ec and fn.argtypes[2]._type_ is C.c_uint32 and fn.restype is C.c_int
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint sdempc_closed_loop_batch_ensemble\([^{]*\{\n\s*return guarded\(", src)


def _call(lib, h, blob, B=4, T=4, H=6, m=4, **over):
    """One sdempc_closed_loop_batch_ensemble call on small neutral inputs, its arguments filled by NAME from the header's prototype; `over` replaces arguments."""
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    names = _names(re.search(r"int sdempc_closed_loop_batch_ensemble\((.*?)\);", hdr, re.S).group(1))
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    Bb, Tb = max(B, 1), max(T, 1)
    x0 = np.zeros((Bb, 13), F); x0[:, 6] = 1.0
    xref = np.zeros((1, 1, H + 1, 13), F); xref[..., 6] = 1.0
    k0 = np.zeros((Bb, 2), U)
    xs, us, info = np.zeros((Bb, Tb + 1, 13), F), np.zeros((Bb, Tb, m), F), np.zeros((Bb, Tb, 8), F)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), 1, 0, 0.0)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 1, 1, 0.0, -1, -1)
    bufs = (C.c_char_p * 1)(blob)
    sz = (C.c_size_t * 1)(len(blob))
    keep = [x0, xref, k0, xs, us, info, tc, pc, bufs, sz]
    args = {n: None for n in names}
    args.update(h=h, timing=C.byref(tc), pc=C.byref(pc), plant_blobs=C.cast(bufs, C.POINTER(C.c_void_p)), plant_blob_bytes=sz, B=B, T=T, x0=x0.ctypes.data_as(fp),
                xref=xref.ctypes.data_as(fp), xref_solves=1, xref_batch=1, keys=k0.ctypes.data_as(u32p), xs=xs.ctypes.data_as(fp), us=us.ctypes.data_as(fp),
                info=C.cast(info.ctypes.data_as(fp), C.POINTER(_abi.SdempcInfo)))
    args.update(over)
    rc = _abi.ensemble_entry(lib)(*[args[n] for n in names])
    del keep
    return rc


def test_refusals_come_first_and_in_order():
    """Every refusal of SPEC.md §11m through the C ABI, before any HIP call (there is no device here), in the documented order: a call wrong in two ways is refused
    for the EARLIER reason; and they come before everything the baseline entry point refuses."""
    lib = _abi.load_library()
    cfg = EC.ens_cfg(num_particles=1)
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    B, T = 4, 4
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), B, C.byref(h)) == 0
    EINVAL = -1
    i32p, fp, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    sref = np.zeros((1, 1, 13), F)
    zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg), 0, np.inf, -np.inf, np.inf, sref.ctypes.data_as(fp), 1, 1)
    z_out = np.zeros((B, 16), U)
    ens_out = np.zeros((T, 3, BASE + 4 * 2), U)
    good_edges = np.array([[1.0, 2.0], [1.0, 1.0], [-np.inf, 0.5], [0.0, np.inf]], F)
    good_cohort = np.array([0, 2, 1, 0], np.int32)

    def ens(size=None, G=3, E=2, over=1, cohort=good_cohort, edges=good_edges):
        e = _abi.SdempcEnsembleCfg(C.sizeof(_abi.SdempcEnsembleCfg) if size is None else size, G, E, over, None if cohort is None else cohort.ctypes.data_as(i32p),
                                   None if edges is None else edges.ctypes.data_as(fp))
        return e

    def run(e, out=ens_out, score=True, **kw):
        a = dict(ens=None if e is None else C.byref(e), ens_out=None if out is None else out.ctypes.data_as(u32p))
        if score:
            a.update(score=C.byref(zc if score is True else score), score_out=z_out.ctypes.data_as(u32p))
        a.update(kw)
        rc = _call(lib, h, blob, B, a.pop("T", T), **a)
        return rc, lib.sdempc_last_error(h).decode()

    nan_edges = good_edges.copy(); nan_edges[2, 1] = np.nan
    down_edges = good_edges.copy(); down_edges[3] = [2.0, 1.0]
    both_edges = down_edges.copy(); both_edges[0, 0] = np.nan
    bad_cohort = np.array([0, 1, 3, 0], np.int32)
    neg_cohort = np.array([0, -1, 1, 0], np.int32)
    bad_zc = _abi.SdempcScoreCfg(4, 0, np.inf, -np.inf, np.inf, sref.ctypes.data_as(fp), 1, 1)
    # in the documented order; each later entry is ALSO wrong in every way a following entry is, where that is possible, and is refused for its own reason
    ladder = [
        (dict(e=None, out=ens_out), "given together"),
        (dict(e=ens(size=8, G=0), out=None), "given together"),
        (dict(e=ens(size=8, G=0, E=17, over=2, edges=both_edges, cohort=bad_cohort), score=False), "struct_size"),
        (dict(e=ens(G=0, E=17, over=2, edges=both_edges, cohort=bad_cohort), score=False), "n_cohorts"),
        (dict(e=ens(G=17, E=17, over=2), score=False), "n_cohorts"),
        (dict(e=ens(E=17, over=2, cohort=bad_cohort), score=False), "n_edges"),
        (dict(e=ens(E=-1, over=2), score=False), "n_edges"),
        (dict(e=ens(over=2, edges=both_edges, cohort=bad_cohort), score=False), "over must be"),
        (dict(e=ens(over=-1), score=False), "over must be"),
        (dict(e=ens(edges=None, cohort=bad_cohort), score=False), "edges is NULL"),
        (dict(e=ens(edges=both_edges, cohort=bad_cohort), score=False), "an edge is NaN"),
        (dict(e=ens(edges=nan_edges), score=False), "an edge is NaN"),
        (dict(e=ens(edges=down_edges, cohort=bad_cohort), score=False), "must ascend"),
        (dict(e=ens(cohort=bad_cohort), score=False), "cohort entry"),
        (dict(e=ens(cohort=neg_cohort), score=False), "cohort entry"),
        (dict(e=ens(), score=False), "needs a score cfg"),
        (dict(e=ens(), score=False, timing=None), "needs a score cfg"),                   # (before what the baseline entry point refuses)
        (dict(e=ens(), score=bad_zc), "score: struct_size"),
        (dict(e=ens(), timing=None), "timing"),
    ]
    for kw, msg in ladder:
        rc, err = run(**kw)
        assert rc == EINVAL and msg in err, (msg, err)
    # a complete call gets past every refusal (and then fails on the missing device, or runs where there is one); so do E = 0 without edges, a NULL cohort array,
    # equal neighbouring edges (good_edges[1]) and infinite edges; ens NULL with ens_out NULL is the baseline entry point's own call
    for e in (ens(), ens(E=0, edges=None), ens(cohort=None), ens(G=1, cohort=None)):
        rc, err = run(e)
        assert rc != EINVAL, err
    rc, err = run(None, out=None)
    assert rc != EINVAL, err
    rc, err = run(None, out=None, score=False, T=0)
    assert rc == EINVAL and "T must be >= 1" in err
    lib.sdempc_destroy(h)


def test_python_keywords_route_and_refuse(monkeypatch):
    """Without ensemble= the call goes to the entry point it went to before (the ensemble entry point is not even looked up); with it, to the new one. The Python
    surface refuses what it can see."""
    B = 4
    cfg, model, x0, xref, keys, kw = EC.inputs(B, num_particles=1)
    g = targets(xref, EC.T4)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    score = Score(pos_radius=1.0)
    ens = Ensemble(pos_edges=[0.5, 1.0])

    class Routed(Exception):
        pass

    def stop(name):
        def entry(lib):
            def fn(*a):
                raise Routed(name)
            return fn
        return entry
    for name in ("ensemble_entry", "baseline_entry", "events_entry", "scored_entry", "fault_entry"):
        monkeypatch.setattr(_abi, name, stop(name))
    for call, want in ((dict(score=score, score_ref=g), "scored_entry"), (dict(), "fault_entry"), (dict(score=score, score_ref=g, ensemble=ens), "ensemble_entry"),
                       (dict(score=score, score_ref=g, ensemble=ens, cohort=np.arange(B) % 2, outputs=False), "ensemble_entry")):
        with pytest.raises(Routed, match=want):
            S.closed_loop(x0, xref, keys, EC.T4, **kw, **call)
    with pytest.raises(ValueError, match="cohort needs ensemble"):
        S.closed_loop(x0, xref, keys, EC.T4, score=score, score_ref=g, cohort=np.zeros(B, int), **kw)
    with pytest.raises(ValueError, match="ensemble needs score"):
        S.closed_loop(x0, xref, keys, EC.T4, ensemble=ens, **kw)
    with pytest.raises(ValueError, match="must be an Ensemble"):
        S.closed_loop(x0, xref, keys, EC.T4, score=score, score_ref=g, ensemble="all", **kw)
    with pytest.raises(ValueError, match="cohort must be int"):
        S.closed_loop(x0, xref, keys, EC.T4, score=score, score_ref=g, ensemble=ens, cohort=np.zeros(B + 1, int), **kw)
    with pytest.raises(ValueError, match="cohort must hold entries"):
        S.closed_loop(x0, xref, keys, EC.T4, score=score, score_ref=g, ensemble=Ensemble(n_cohorts=2), cohort=np.array([0, 1, 2, 0]), **kw)
    with pytest.raises(ValueError, match="cohort must hold entries"):
        S.closed_loop(x0, xref, keys, EC.T4, score=score, score_ref=g, ensemble=ens, cohort=np.array([0, 16, 2, 0]), **kw)
    S.close()
