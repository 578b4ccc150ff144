"""Without a GPU: the retiring closed loop's reference (SPEC.md §11n, tests/retire_ref.py) against its own properties and against thirteen deliberately wrong
variants, each of which must change a compared word or list entry; the live list's restatement at the wave and block edges; every refusal through the C ABI, in
order and before any HIP call; the Python keywords' routing; the exported symbol and the ABI version; retire_summary."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import retire_cases as RC
from cases import ROOT, bits_differ
from retire_ref import LIST_MUTANTS, LOOP_MUTANTS, live_list, retire_loop_ref
from score_loop_ref import NONE, score_rows
from sde4mbrl_px4_amd import _abi, synthetic_iris
from sde4mbrl_px4_amd.solver import Ensemble, Score, SdeMpcSolver, retire_summary

F = np.float32
U = np.uint32


def values_differ(a, b):
    """Number of differing words between two tuples of reference values."""
    n = 0
    for v, w in zip(a, b):
        n += bits_differ(v, w) if v.dtype == np.float32 else int((np.asarray(v) != np.asarray(w)).sum())
    return n


def test_reference_properties():
    """Rows and words equal the unretired reference through the failing period; an episode that never fails is identical throughout; after its retirement an
    episode's info rows are the held ones, and its rows DO change (it flies a held table)."""
    c = RC.prepared(5)
    at = c["retired_at"]
    assert (at > 0).any() and (at < 0).any() and c["live"].tolist() == [int((np.where(at < 0, 99, at) > j).sum()) for j in range(RC.NS4)]
    zp, z = c["z_plain"], c["z"]
    for b in range(5):
        one = tuple(v[b:b + 1] for v in c["vals"])
        two = tuple(v[b:b + 1] for v in c["plain"])
        if at[b] < 0:
            assert values_differ(one, two) == 0 and (z[b] == zp[b]).all()
            continue
        Tb = int(at[b]) * RC.S2
        assert bits_differ(one[0][:, :Tb + 1], two[0][:, :Tb + 1]) == 0 and bits_differ(one[1][:, :Tb], two[1][:, :Tb]) == 0
        assert bits_differ(one[2][:, :at[b]], two[2][:, :at[b]]) == 0 and bits_differ(one[-1][:, :Tb * RC.N2], two[-1][:, :Tb * RC.N2]) == 0
        assert bits_differ(one[0][:, Tb + 1:], two[0][:, Tb + 1:]) > 0
        held = one[2][0, at[b]:]
        assert (held[:, [0, 2, 3, 4, 5, 6, 7]] == 0).all() and (held[:, 1] == one[4][0]).all()
        assert np.array_equal(one[5], two[5])                                 # the key schedule is the unretired run's
        assert z[b, 8] == zp[b, 8] != NONE and z[b, 0] == Tb and zp[b, 0] == RC.T8
        trunc = score_rows(two[0][:, :Tb + 1], two[1][:, :Tb], two[2][:, :at[b]], two[-1][:, :Tb * RC.N2], c["g"][:Tb, b:b + 1], c["cfg"], c["score"].thresholds(),
                           False, RC.S2)
        assert (z[b] == trunc[0]).all()


def test_two_calls_equal_one():
    """The reference flown 4 + 4 through score_in and the continuation values against the reference flown 8: every score word, retired_at and live composed, every
    key, and every row of the episodes live at the cut; an episode retired before the cut agrees through its failing period (behind the cut it flies the second
    call's entry tables: the rule that a call's tables do not depend on what came before it)."""
    c = RC.prepared(5)
    cfg, x0, xref, keys, kw, g, score = c["cfg"], c["x0"], c["xref"], c["keys"], c["kw"], c["g"], c["score"]
    half = RC.T8 // 2
    ka = dict(kw, fault=kw["fault"][:half])
    va, za, rta, la, _ = retire_loop_ref(RC.run_ref_for(RC.age_loop_ref, cfg, c["model"], x0, xref, keys, half, **ka), cfg, x0, g[:half], score.thresholds(), False,
                                         RC.S2, RC.N2, half)
    kb = dict(kw, fault=kw["fault"][half:], u_init=va[3], stepsize_in=va[4], u_act_in=va[6])
    vb, zb, rtb, lb, _ = retire_loop_ref(RC.run_ref_for(RC.age_loop_ref, cfg, c["model"], va[0][:, -1], xref, va[5], half, **kb), cfg, va[0][:, -1], g[half:],
                                         score.thresholds(), False, RC.S2, RC.N2, half, score_in=za)
    at = np.where(c["retired_at"] < 0, 1 << 30, c["retired_at"])
    assert (zb == c["z"]).all() and np.array_equal(np.concatenate([la, lb]), c["live"])
    assert np.array_equal(rta, np.where(at < 2, at, -1)) and np.array_equal(rtb, np.where(at <= 2, 0, np.where(at < RC.NS4, at - 2, -1))) and (rtb == 0).any()
    assert np.array_equal(vb[5], c["vals"][5])
    joined = (np.concatenate([va[0], vb[0][:, 1:]], axis=1), np.concatenate([va[1], vb[1]], axis=1), np.concatenate([va[2], vb[2]], axis=1)) + vb[3:7]
    alive = at > 2
    assert values_differ(tuple(v[alive] for v in joined), tuple(v[alive] for v in c["vals"][:7])) == 0
    for e in np.flatnonzero(~alive):
        Tb = int(at[e]) * RC.S2
        assert bits_differ(joined[0][e, :Tb + 1], c["vals"][0][e, :Tb + 1]) == 0 and bits_differ(joined[1][e, :Tb], c["vals"][1][e, :Tb]) == 0


@pytest.mark.parametrize("mutant", LOOP_MUTANTS)
def test_wrong_loops_differ(mutant):
    """Each wrong variant changes a compared output of the mixed case (for "entry_ignored": of its continuation, where an episode is retired at entry)."""
    c = RC.prepared(5, substeps=True, P=33)
    cfg, g, th = c["cfg"], c["g"], c["score"].thresholds()
    if mutant != "entry_ignored":
        vals, z, rt, live, _ = retire_loop_ref(c["run_ref"], cfg, c["x0"], g, th, True, RC.S2, RC.N2, RC.T8, mutant=mutant, first=c["first"])
        n = values_differ(vals, c["vals"]) + int((z != c["z"]).sum()) + int((rt != c["retired_at"]).sum()) + int((live != c["live"]).sum())
        assert n > 0, mutant
        return
    z_in = c["z"]                                            # the mixed case's final words: three episodes have failed
    assert (z_in[:, 8] != NONE).any()
    run = RC.run_ref_for(RC.age_loop_ref, cfg, c["model"], c["x0"], c["xref"], c["keys"], RC.T8, **c["kw"])
    plain = run(None)
    first = (plain, score_rows(plain[0], plain[1], plain[2], plain[-1], g, cfg, th, True, RC.S2, score_in=z_in))
    good = retire_loop_ref(run, cfg, c["x0"], g, th, True, RC.S2, RC.N2, RC.T8, score_in=z_in, first=first)
    bad = retire_loop_ref(run, cfg, c["x0"], g, th, True, RC.S2, RC.N2, RC.T8, score_in=z_in, mutant=mutant, first=first)
    assert (good[2] == 0).any() and good[3][0] < 5
    assert values_differ(bad[0], good[0]) + int((bad[1] != good[1]).sum()) + int((bad[2] != good[2]).sum()) + int((bad[3] != good[3]).sum()) > 0


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 300, 600])
def test_live_list_is_the_ascending_list(B):
    rng = np.random.default_rng(B)
    for flags in (rng.random(B) < 0.5, np.ones(B, bool), np.zeros(B, bool), RC.pattern(B)):
        lst, n_live, blk = live_list(flags)
        assert n_live == int(flags.sum()) and np.array_equal(lst, np.flatnonzero(flags)) and blk.sum() == n_live and blk.size == -(-B // 256)


@pytest.mark.parametrize("mutant", LIST_MUTANTS)
def test_wrong_lists_differ(mutant):
    """On the pattern of the GPU test at B = 600: flips at 63|64 and 255|256, block 1 wholly retired, block 2 wholly live."""
    flags = RC.pattern(600)
    assert flags[63] and not flags[64] and flags[255] and not flags[256:512].any() and flags[512:].all()
    good, n, _ = live_list(flags)
    bad, nb, _ = live_list(flags, mutant)
    assert nb != n or not np.array_equal(bad, good), mutant


def test_retire_summary():
    s = retire_summary(np.array([-1, 0, 2, -1], np.int32), np.array([3, 3, 2], np.int32), 4)
    assert s == dict(solves_run=8, solves_saved=4, saved_share=4 / 12, retired=2, retired_at_entry=1)
    assert retire_summary(np.zeros(0, np.int32), np.zeros(0, np.int32), 0)["saved_share"] == 0.0
    with pytest.raises(ValueError, match="retired_at must be int"):
        retire_summary(np.zeros(3, np.int32), np.zeros(2, np.int32), 4)
    with pytest.raises(ValueError, match="live must be int"):
        retire_summary(np.zeros(4, np.int32), np.array([5], np.int32), 4)
    c = RC.prepared(5)
    s = retire_summary(c["retired_at"], c["live"], 5)
    assert s["solves_run"] == int(c["live"].sum()) and s["retired"] == int((c["retired_at"] >= 0).sum()) and 0 < s["saved_share"] < 1


def test_symbol_is_exported_and_the_abi_version_stays():
    lib = _abi.load_library()
    assert "sdempc_closed_loop_batch_retire" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "sdempc_closed_loop_batch_retire")
    assert lib.sdempc_abi_version() == 3
    fn = _abi.retire_entry(lib)
    ens = _abi.ensemble_entry(lib)
    assert list(fn.argtypes[4:]) == list(ens.argtypes[1:]) and len(fn.argtypes) == len(ens.argtypes) + 3
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert len(_names(re.search(r"int sdempc_closed_loop_batch_retire\((.*?)\);", hdr, re.S).group(1))) == len(fn.argtypes)
    api = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"int sdempc_closed_loop_batch_retire\([^{]*\{\s*return guarded\(h,", api)


def _names(proto):
    return [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]


def _call(lib, h, blob, B=4, T=4, H=6, m=4, **over):
    """One sdempc_closed_loop_batch_retire call on small neutral inputs, its arguments filled by NAME from the header's prototype; `over` replaces arguments."""
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    names = _names(re.search(r"int sdempc_closed_loop_batch_retire\((.*?)\);", hdr, re.S).group(1))
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
    rc = _abi.retire_entry(lib)(*[args[n] for n in names])
    del keep
    return rc


def test_refusals_come_first_and_in_order():
    """Every refusal of SPEC.md §11n through the C ABI, before any HIP call (there is no device here), in the documented order: a call wrong in two ways is refused
    for the EARLIER reason; and they come before everything the ensemble entry point refuses."""
    lib = _abi.load_library()
    ccfg, keep = RC.retire_cfg(num_particles=1).to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    B, T = 4, 4
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), B, C.byref(h)) == 0
    EINVAL = -1
    i32p, fp, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    sref = np.zeros((1, 1, 13), F)
    zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg), 0, np.inf, -np.inf, np.inf, sref.ctypes.data_as(fp), 1, 1)
    z_out = np.zeros((B, 16), U)
    ens_out = np.zeros((T, 1, 20), U)
    retired_at, live = np.zeros(B, np.int32), np.zeros(T, np.int32)

    def cfg(size=None, reserved=0):
        return _abi.SdempcRetireCfg(C.sizeof(_abi.SdempcRetireCfg) if size is None else size, reserved)

    def ens(over=1, G=1):
        return _abi.SdempcEnsembleCfg(C.sizeof(_abi.SdempcEnsembleCfg), G, 0, over, None, None)

    def run(y, at=retired_at, lv=live, e=None, score=True, **kw):
        a = dict(retire=None if y is None else C.byref(y), retired_at=None if at is None else at.ctypes.data_as(i32p),
                 live_per_solve=None if lv is None else lv.ctypes.data_as(i32p))
        if e is not None:
            a.update(ens=C.byref(e), ens_out=ens_out.ctypes.data_as(u32p))
        if score:
            a.update(score=C.byref(zc), score_out=z_out.ctypes.data_as(u32p))
        a.update(kw)
        rc = _call(lib, h, blob, B, a.pop("T", T), **a)
        return rc, lib.sdempc_last_error(h).decode()

    ladder = [
        (dict(y=None), "given together"),
        (dict(y=cfg(size=4, reserved=1), at=None, score=False), "given together"),
        (dict(y=cfg(size=4, reserved=1), lv=None, score=False), "given together"),
        (dict(y=cfg(size=4, reserved=1), e=ens(over=0), score=False), "retire: struct_size"),
        (dict(y=cfg(reserved=1), e=ens(over=0), score=False), "reserved must be 0"),
        (dict(y=cfg(), e=ens(over=0), score=False), "needs a score cfg"),
        (dict(y=cfg(), score=False, timing=None), "needs a score cfg"),
        (dict(y=cfg(), e=ens(over=0, G=0)), "may not be combined with retire"),
        (dict(y=cfg(), e=ens(G=0)), "n_cohorts"),                                      # (then what the ensemble entry point refuses, in its order)
        (dict(y=cfg(), timing=None), "timing"),
    ]
    for kw, msg in ladder:
        rc, err = run(**kw)
        assert rc == EINVAL and msg in err, (msg, err)
    # a complete call gets past every refusal (and then fails on the missing device, or runs where there is one), with and without an "alive" ensemble; a NULL cfg
    # with NULL outputs is the ensemble entry point's own call
    for kw in (dict(y=cfg()), dict(y=cfg(), e=ens()), dict(y=None, at=None, lv=None), dict(y=None, at=None, lv=None, e=ens(over=0))):
        rc, err = run(**kw)
        assert rc != EINVAL, err
    rc, err = run(None, at=None, lv=None, score=False, T=0)
    assert rc == EINVAL and "T must be >= 1" in err
    lib.sdempc_destroy(h)


def test_python_keywords_route_and_refuse(monkeypatch):
    """Without retire= the call goes to the entry point it went to before (the retire entry point is not even looked up); with it, to the new one, with or without
    an ensemble and a controller. The Python surface refuses what it can see — among it every route on which no score is formed."""
    B = 4
    cfg, model, x0, xref, keys, kw = RC.inputs(B, num_particles=1)
    g = RC.targets(xref, RC.T8)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    score = Score(pos_radius=1.0)

    class Routed(Exception):
        pass

    def stop(name):
        def entry(lib):
            def fn(*a):
                raise Routed(name)
            return fn
        return entry
    for name in ("retire_entry", "ensemble_entry", "scored_entry", "fault_entry"):
        monkeypatch.setattr(_abi, name, stop(name))
    scored = dict(score=score, score_ref=g)
    for call, want in ((scored, "scored_entry"), (dict(), "fault_entry"), (dict(scored, ensemble=Ensemble()), "ensemble_entry"), (dict(scored, retire=False), "scored_entry"),
                       (dict(scored, retire=True), "retire_entry"), (dict(scored, retire=True, outputs=False), "retire_entry"),
                       (dict(scored, retire=True, ensemble=Ensemble(pos_edges=[0.5])), "retire_entry")):
        with pytest.raises(Routed, match=want):
            S.closed_loop(x0, xref, keys, RC.T8, **kw, **call)
    with pytest.raises(ValueError, match="retire needs score"):
        S.closed_loop(x0, xref, keys, RC.T8, retire=True, **kw)
    with pytest.raises(ValueError, match="retire needs score"):                # (no plant, none of the timed-loop arguments: the plain route)
        S.closed_loop(x0, xref, keys, RC.T8, retire=True)
    with pytest.raises(ValueError, match="retire needs score"):
        S.closed_loop(x0, xref, keys, RC.T8, retire=True, plant=model)
    with pytest.raises(ValueError, match='Ensemble\\(over="all"\\)'):
        S.closed_loop(x0, xref, keys, RC.T8, retire=True, ensemble=Ensemble(over="all"), **scored, **kw)
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    import inspect
    assert "retire" in inspect.signature(MpcProblem.simulate).parameters and "retire" in inspect.signature(SdeMpcSolver.closed_loop).parameters
    S.close()
