"""Gusts and estimator bias drawn on the device (SPEC.md §11i) without a GPU: header / binding / library agree on the new symbol at ABI version 3 and no kernel was
added, every refusal of sdempc_closed_loop_batch_drawn (no HIP call may happen before them) and of the Python surface, the positions of the new values in the
returned tuples, the single rounding of GaussMarkov's coefficients, the frame rules of MpcProblem.simulate, the row generator of tests/process_loop_ref.py — its
restated normal against the oracle's, continuation, neutrality, the discrimination of its six mutants on the cases of tests/process_cases.py — and the moments
of a long reference run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_census
import orc
from age_loop_ref import age_loop_ref
from cases import ROOT, bits_differ
from loop_cases import REF_NAME
from process_cases import B5, S2, T5, T6, VALID, W_BIAS, W_DIST, bias_rows, chain_keys, disturbance, drawn, for_ref, score_cfg, scored_episodes
from process_loop_ref import MUTANTS, ROW_MUTANTS, draw, process_loop_ref, process_rows
from sde4mbrl_px4_amd import _abi, synthetic_iris
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, GaussMarkov, Score, SdeMpcSolver, gauss_markov_bias
from timed_loop_ref import num_solves

F = np.float32
NEW = "sdempc_closed_loop_batch_drawn"


def ref(loop, cfg, model, x0, xref, keys, T, **kw):
    """A reference loop for the keyword arguments of SdeMpcSolver.closed_loop, always with xsub as the last value."""
    return loop(cfg, model, x0=x0, xref=xref, keys=keys, T=T, substep_states=True, **{"plants": None, **{REF_NAME.get(k, k): v for k, v in kw.items()}})


def test_abi_surface_of_the_drawn_entry_point_and_no_new_kernel():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_process_cfg \{[^}]*struct_size;[^}]*batch;[^}]*const float\* rho;[^}]*const float\* scale;[^}]*const uint32_t\* keys;"
                     r"[^}]*const float\* state_in;[^}]*\}", hdr)
    R = _abi.SdempcProcessCfg
    assert C.sizeof(R) == 40 and (R.struct_size.offset, R.batch.offset, R.rho.offset, R.scale.offset, R.keys.offset, R.state_in.offset) == (0, 4, 8, 16, 24, 32)
    assert NEW in _abi.EXPORTED_SYMBOLS and f"int {NEW}(" in hdr
    proto = re.search(r"int " + NEW + r"\((.*?)\);", hdr, re.S).group(1)
    sproto = re.search(r"int sdempc_closed_loop_batch_scored\((.*?)\);", hdr, re.S).group(1)
    names = lambda p: [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", p, flags=re.S).split(",")]      # noqa: E731
    # the scored prototype plus the new arguments, in order: two cfgs behind h, six outputs at the end
    assert names(proto) == ["h", "dist_proc", "bias_proc"] + names(sproto)[1:] + ["dist_rows", "dist_keys_next", "dist_state_next", "bias_rows", "bias_keys_next",
                                                                                "bias_state_next"]
    bare = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert re.search(r"const sdempc_process_cfg\* dist_proc\s*,\s*const sdempc_process_cfg\* bias_proc\s*,\s*const sdempc_score_cfg\* score", bare)
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, NEW)
    fn = _abi.drawn_entry(lib)
    sa = _abi.scored_entry(lib).argtypes
    assert list(fn.argtypes[3:-6]) == list(sa[1:]) and fn.argtypes[0] is sa[0] and fn.restype is C.c_int
    assert fn.argtypes[1]._type_ is _abi.SdempcProcessCfg and fn.argtypes[2]._type_ is _abi.SdempcProcessCfg
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    assert list(fn.argtypes[-6:]) == [fp, u32p, fp] * 2
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint " + NEW + r"\([^{]*\{\n\s*return guarded\(", src)
    # the processes are an argument of an existing kernel: the built kernel set is the census table, in both directions
    built = kernel_census.built_kernels()
    assert built is not None and built == kernel_census.table_names()
    assert ("sdempc_loop_keys_period_kernel", "") in built


def _call(lib, h, cfg, blob, B=4, T=5, S=2, n=2, dist=True, bias=True, size=None, batch=None, rho="ok", scale="ok", keys=True, state=None, obs=None, obs_keys=None,
          outs=None, score=False, null=(), D=0):
    """One sdempc_closed_loop_batch_drawn call on small neutral inputs; every field of the two process cfgs can be overridden (size / batch / rho / scale / keys /
    state apply to BOTH cfgs that are given). `outs` names the new outputs passed (default: those of the cfgs given); `null` the per-row outputs passed as NULL."""
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    H, m = cfg.horizon, cfg.num_motors
    Tb, Bb = max(T, 1), max(B, 1)
    Ns = num_solves(Tb, max(S, 1))
    x0 = np.zeros((Bb, 13), F); x0[:, 6] = 1.0
    xref = np.zeros((1, 1, H + 1, 13), F); xref[..., 6] = 1.0
    k0, qk = np.zeros((Bb, 2), np.uint32), np.zeros((Bb, 2), np.uint32)
    bufs_ = dict(xs=np.zeros((Bb, Tb + 1, 13), F), us=np.zeros((Bb, Tb, m), F), info=np.zeros((Bb, Ns, 8), F))
    p = {k: (None if k in null else v.ctypes.data_as(fp)) for k, v in bufs_.items()}
    obs = bias if obs is None else obs
    obs_keys = obs if obs_keys is None else obs_keys
    oc = _abi.SdempcObsCfg(C.sizeof(_abi.SdempcObsCfg), None, None, 1, 1, None, 1, 1)          # (no sigma, beta or valid: legal with a bias process)
    b_xm, b_qn, b_xn = np.zeros((Bb, Ns, 13), F), np.zeros((Bb, 2), np.uint32), np.zeros((Bb, 13), F)
    g = np.zeros((1, 1, 13), F)
    zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg), 0, 1.0, 0.5, 4.0, g.ctypes.data_as(fp), 1, 1)
    zo = np.zeros((Bb, 16), np.uint32)
    keep, cfgs, new = [], [], {}
    for name, W, on, N in (("dist", 6, dist, Tb), ("bias", 12, bias, Ns)):
        rows = B if batch is None else batch
        fits = lambda v: np.ndim(v) == 0 or np.shape(v)[-1] == W           # noqa: E731  (an array of the other process's width leaves this cfg at its default)
        r = np.full((max(rows, 1), W), 0.5, F) if isinstance(rho, str) or (rho is not None and not fits(rho)) else (None if rho is None else np.ascontiguousarray(rho, F))
        s = np.full((max(rows, 1), W), 0.1, F) if isinstance(scale, str) or (scale is not None and not fits(scale)) else (None if scale is None else np.ascontiguousarray(scale, F))
        kk = np.zeros((Bb, 2), np.uint32)
        st = None if state is None or not fits(state) else np.ascontiguousarray(np.broadcast_to(np.asarray(state, F), (Bb, W)))
        pcf = _abi.SdempcProcessCfg(C.sizeof(_abi.SdempcProcessCfg) if size is None else size, rows, None if r is None else r.ctypes.data_as(fp),
                                    None if s is None else s.ctypes.data_as(fp), kk.ctypes.data_as(u32p) if keys else None, None if st is None else st.ctypes.data_as(fp))
        keep += [r, s, kk, st, pcf]
        cfgs.append(C.byref(pcf) if on else None)
        o = (np.zeros((Bb, N, W), F), np.zeros((Bb, 2), np.uint32), np.zeros((Bb, W), F))
        keep += list(o)
        want = on if outs is None else name in outs
        new[name] = [o[0].ctypes.data_as(fp), o[1].ctypes.data_as(u32p), o[2].ctypes.data_as(fp)] if want else [None, None, None]
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S, D, 0.0)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 1, n, 0.0, -1, -1)
    bufs = (C.c_char_p * 1)(blob)
    sz = (C.c_size_t * 1)(len(blob))
    return _abi.drawn_entry(lib)(
        h, cfgs[0], cfgs[1], C.byref(zc) if score else None, None, None, None,
        C.byref(oc) if obs else None, qk.ctypes.data_as(u32p) if obs_keys else None, None, None, None, None, C.byref(tc), C.byref(pc),
        C.cast(bufs, C.POINTER(C.c_void_p)), sz, None, B, T, x0.ctypes.data_as(fp), xref.ctypes.data_as(fp), 1, 1, k0.ctypes.data_as(u32p), None, None, None,
        p["xs"], p["us"], None if p["info"] is None else C.cast(p["info"], C.POINTER(_abi.SdempcInfo)), None, None, None, None,
        None, None, None, None, None, None,
        b_xm.ctypes.data_as(fp) if obs and "xs" not in null else None, b_qn.ctypes.data_as(u32p) if obs else None, b_xn.ctypes.data_as(fp) if obs else None, None,
        zo.ctypes.data_as(u32p) if score else None, *new["dist"], *new["bias"])


def test_drawn_argument_checks_make_no_hip_call():
    import torch
    lib = _abi.load_library()
    cfg = score_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EDEVICE, ECAPACITY = -1, -3, -5
    B = 4
    nan, inf = float("nan"), float("inf")

    def one(W, i, v, base):
        a = np.full((B, W), base, F)
        a[B - 1, i] = v
        return a
    try:
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(size=32), EINVAL, "process: struct_size"),
            (dict(size=32, T=0), EINVAL, "process: struct_size"),                      # the structs are looked at first
            (dict(bias=False, size=44), EINVAL, "process: struct_size"),
            (dict(dist=False, size=0), EINVAL, "process: struct_size"),
            (dict(batch=0), EINVAL, "batch must be 1 or B"),
            (dict(batch=2), EINVAL, "batch must be 1 or B"),
            (dict(batch=B + 1), EINVAL, "batch must be 1 or B"),
            (dict(rho=None), EINVAL, "rho, scale or keys is NULL"),
            (dict(scale=None), EINVAL, "rho, scale or keys is NULL"),
            (dict(keys=False), EINVAL, "rho, scale or keys is NULL"),
            (dict(bias=False, rho=one(6, 5, nan, 0.5)), EINVAL, "rho holds"),
            (dict(bias=False, rho=one(6, 0, -0.25, 0.5)), EINVAL, "rho holds"),
            (dict(bias=False, rho=one(6, 3, 1.0000001, 0.5)), EINVAL, "rho holds"),
            (dict(dist=False, rho=one(12, 11, inf, 0.5)), EINVAL, "rho holds"),
            (dict(bias=False, scale=one(6, 5, nan, 0.1)), EINVAL, "scale holds"),
            (dict(bias=False, scale=one(6, 2, inf, 0.1)), EINVAL, "scale holds"),
            (dict(dist=False, scale=one(12, 11, -1e-3, 0.1)), EINVAL, "scale holds"),
            (dict(bias=False, state=one(6, 5, nan, 0.0)), EINVAL, "state_in holds"),
            (dict(dist=False, state=one(12, 7, -inf, 0.0)), EINVAL, "state_in holds"),
            (dict(obs_keys=False, obs=True), EINVAL, "bias_proc needs"),
            (dict(obs=False), EINVAL, "bias_proc needs"),
            # a new output without its cfg
            (dict(dist=False, outs=("dist", "bias")), EINVAL, "without dist_proc"),
            (dict(bias=False, outs=("dist", "bias")), EINVAL, "without bias_proc"),
            (dict(dist=False, bias=False, outs=("bias",), obs=False), EINVAL, "without bias_proc"),
            # everything the scored entry point refuses, behind valid process cfgs
            (dict(null=("xs",)), EINVAL, "NULL host pointer"),
            (dict(D=5), EINVAL, "solve_delay"),
            (dict(T=0), EINVAL, "T must"),
            (dict(B=5, batch=1), ECAPACITY, "max_batch"),
            (dict(n=0), EINVAL, "substeps"),
            (dict(S=0), EINVAL, "solve_period"),
        ]
        for kw, want, word in cases:
            rc = _call(lib, h, cfg, blob, **kw)
            msg = lib.sdempc_last_error(h).decode()
            assert rc == want, (sorted(kw), rc, msg)
            assert word in msg, (word, msg)
            assert lib.sdempc_device_ready(h) == 0
        # valid arguments reach the device: each process alone, shared coefficients, the bounds of rho, a zero scale, a state, no new outputs, NULL rows under a score,
        # both cfgs NULL (the scored call)
        good = 0 if torch.cuda.is_available() else EDEVICE
        for kw in (dict(), dict(bias=False), dict(dist=False), dict(batch=1), dict(rho=np.zeros((B, 12), F), dist=False), dict(rho=np.ones((B, 6), F), bias=False),
                   dict(scale=np.zeros((B, 6), F), bias=False), dict(state=0.25), dict(outs=()), dict(score=True, null=("xs", "us", "info")), dict(dist=False, bias=False),
                   dict(dist=False, bias=False, score=True), dict(T=1)):
            rc = _call(lib, h, cfg, blob, **kw)
            assert rc == good, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_checks_the_process_keywords():
    cfg = score_cfg()
    model = synthetic_iris()
    B, T = 3, 5
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    gm = GaussMarkov(1.0, 0.5, 0.05)
    for kw in (dict(dist_keys=k), dict(dist_state_in=np.zeros((B, 6), F)), dict(bias_keys=k), dict(bias_state_in=np.zeros((B, 12), F))):      # each needs its process
        with pytest.raises(ValueError, match="_process=GaussMarkov"):
            S.closed_loop(x0, xref, k, T, **kw)
    for kw in (dict(dist_process=gm), dict(bias_process=gm, meas_keys=k)):                                      # a process needs its keys
        with pytest.raises(ValueError, match="_keys .* is required"):
            S.closed_loop(x0, xref, k, T, **kw)
    with pytest.raises(ValueError, match="meas_keys"):
        S.closed_loop(x0, xref, k, T, bias_process=gm, bias_keys=k)
    for kw in (dict(dist_process=(0.5, 0.1), dist_keys=k), dict(dist_process=gm, dist_keys=k[:2]), dict(dist_process=gm, dist_keys=k, dist_state_in=np.zeros((B, 12), F)),
               dict(dist_process=GaussMarkov(np.ones(12), 0.5, 0.05), dist_keys=k), dict(bias_process=GaussMarkov(np.ones((2, 12)), 0.5, 0.05), bias_keys=k, meas_keys=k),
               dict(dist_process=gm, dist_keys=k, dist_state_in=np.full((B, 6), np.nan, F)), dict(dist_process=gm, dist_keys=k, outputs=False)):
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    for bad in (dict(std=-1.0, tau=1.0, dt=0.1), dict(std=1.0, tau=0.0, dt=0.1), dict(std=1.0, tau=1.0, dt=0.0), dict(std=np.inf, tau=1.0, dt=0.1)):
        with pytest.raises(ValueError):
            GaussMarkov(**bad)
    for rho, scale in ((1.5, 0.1), (-0.1, 0.1), (0.5, -0.1), (0.5, np.inf), (np.nan, 0.1)):
        with pytest.raises(ValueError):
            GaussMarkov.from_coeffs(rho, scale)
    assert not S.device_ready()
    S.close()
    prob = MpcProblem(cfg=cfg, model=model)
    z2 = np.zeros(2, np.uint32)
    with pytest.raises(ValueError, match="need dist_process"):
        prob.simulate(np.zeros(13, F), z2, T, dist_rng=z2)
    with pytest.raises(ValueError, match="need bias_process"):
        prob.simulate(np.zeros(13, F), z2, T, bias_state=np.zeros(12, F))
    with pytest.raises(ValueError, match="dist_rng .* is required"):
        prob.simulate(np.zeros(13, F), z2, T, dist_process=gm)
    with pytest.raises(ValueError, match="meas_rng"):
        prob.simulate(np.zeros(13, F), z2, T, bias_process=gm, bias_rng=z2)


def test_tuple_positions_of_the_process_values(monkeypatch):
    """The process values sit behind the score and in front of xsub, the disturbance process first; outputs=False returns None for the rows; a call without a process
    keyword does not reach the new entry point."""
    cfg = score_cfg()
    B, T, n = 3, 5, 2
    Ns = num_solves(T, 2)
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=B)
    seen = {}

    def fake(name):
        def entry(lib):
            def call(h, *args):
                seen["name"], seen["args"] = name, args
                return 0
            return call
        return entry
    for e in ("drawn", "scored", "aged", "observed", "fault"):
        monkeypatch.setattr(_abi, e + "_entry", fake(e))
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    g = np.zeros((T, 1, 13), F)
    tm = dict(solve_period=2, plant_substeps=n)
    gd, gb = GaussMarkov(np.arange(1.0, 7.0), 0.5, 0.05), GaussMarkov(np.ones((B, 12)), np.full(12, 2.0), 0.1)
    out = S.closed_loop(x0, xref, k, T, **tm, score=Score(), score_ref=g)
    assert seen["name"] == "scored" and len(out) == 8
    n_scored = len(seen["args"])
    # the disturbance process alone: no observation, no score — NULL in every cfg position but the first
    out = S.closed_loop(x0, xref, k, T, **tm, dist_process=gd, dist_keys=k)
    a = seen["args"]
    assert seen["name"] == "drawn" and len(a) == n_scored + 8 and len(out) == 10
    assert [v.shape for v in out[7:]] == [(B, T, 6), (B, 2), (B, 6)] and out[8].dtype == np.uint32
    assert a[0] is not None and all(v is None for v in a[1:9]) and all(v is not None for v in a[-6:-3]) and all(v is None for v in a[-3:]) and a[-7] is None
    pc = a[0]._obj
    assert (pc.struct_size, pc.batch) == (40, 1) and pc.state_in is None or not pc.state_in
    assert np.ctypeslib.as_array(pc.rho, (6,)).tobytes() == gd.rho.tobytes() and np.ctypeslib.as_array(pc.scale, (6,)).tobytes() == gd.scale.tobytes()
    # the bias process alone makes the call an observed one with an empty obs cfg
    out = S.closed_loop(x0, xref, k, T, **tm, bias_process=gb, bias_keys=k, meas_keys=k, bias_state_in=np.ones((B, 12), F))
    a = seen["args"]
    assert seen["name"] == "drawn" and len(out) == 13 and [v.shape for v in out[7:]] == [(B, Ns, 13), (B, 2), (B, 13), (B, Ns, 12), (B, 2), (B, 12)]
    assert a[0] is None and a[1] is not None and a[1]._obj.batch == B and a[6] is not None and a[7] is not None
    oc = a[6]._obj
    assert not oc.sigma and not oc.beta and not oc.valid
    assert all(v is None for v in a[-6:-3]) and all(v is not None for v in a[-3:])
    # both, with a score and xsub: score, dist values, bias values, xsub
    out = S.closed_loop(x0, xref, k, T, **tm, dist_process=gd, dist_keys=k, bias_process=gb, bias_keys=k, meas_keys=k, score=Score(), score_ref=g, substep_states=True)
    assert len(out) == 18 and out[10].dtype == SCORE_DTYPE and [v.shape for v in out[11:]] == [(B, T, 6), (B, 2), (B, 6), (B, Ns, 12), (B, 2), (B, 12), (B, T * n, 13)]
    a = seen["args"]
    assert a[2] is not None and a[-7] is not None and all(v is not None for v in a[-6:])
    out = S.closed_loop(x0, xref, k, T, **tm, dist_process=gd, dist_keys=k, bias_process=gb, bias_keys=k, meas_keys=k, score=Score(), score_ref=g, substep_states=True,
                        outputs=False)
    names = ("xs", "us", "info", "u_next", "stepsize_next", "keys_next", "u_act_next", "xmeas", "meas_keys_next", "xmeas_next", "score", "dist_rows", "dist_keys_next",
             "dist_state_next", "bias_rows", "bias_keys_next", "bias_state_next", "xsub")
    assert len(out) == len(names)
    for nm, v in zip(names, out):
        assert (v is None) == (nm in ("xs", "us", "info", "xmeas", "dist_rows", "bias_rows", "xsub")), nm
    a = seen["args"]
    assert a[-6] is None and a[-5] is not None and a[-4] is not None and a[-3] is None and a[-2] is not None and a[-1] is not None
    out = S.closed_loop(x0, xref, k, T, **tm, substep_states=True)
    assert seen["name"] == "fault" and len(out) == 8
    assert not S.device_ready()
    S.close()


def test_gauss_markov_coefficients_are_computed_in_float64_and_rounded_once():
    rng = np.random.default_rng(7)
    twice = 0
    for std, tau, dt in zip(rng.uniform(0.01, 3.0, 400), rng.uniform(0.02, 5.0, 400), rng.uniform(0.005, 0.2, 400)):
        gm = GaussMarkov(std, tau, dt)
        rho = np.exp(-np.float64(dt) / np.float64(tau))
        assert gm.rho.dtype == F and gm.scale.dtype == F
        assert gm.rho == F(rho) and gm.scale == F(np.float64(std) * np.sqrt(1.0 - rho * rho))
        r32 = F(rho)
        twice += gm.scale != F(F(std) * np.sqrt(F(1.0) - r32 * r32))
    assert twice > 0                                   # the scale of the rounded rho is a different number often enough to matter
    # the recipe of gauss_markov_bias, coefficient for coefficient
    std, tau = rng.uniform(0.01, 0.1, (3, 12)), rng.uniform(0.5, 2.0, 12)
    gm = GaussMarkov(std, tau, 0.1)
    rho = np.exp(-0.1 / np.broadcast_to(tau, (3, 12)))
    assert gm.rho.tobytes() == rho.astype(F).tobytes() and gm.scale.tobytes() == (std * np.sqrt(1.0 - rho * rho)).astype(F).tobytes()
    r, s = gm.coeffs(3, 12)
    assert r.shape == s.shape == (3, 12) and r.flags.c_contiguous and r.tobytes() == gm.rho.tobytes()
    r, s = GaussMarkov(0.5, 1.0, 0.1).coeffs(3, 6)
    assert r.shape == s.shape == (1, 6) and (r == r[0, 0]).all()
    p = GaussMarkov.from_coeffs(F(0.9), np.full(6, 0.25, F))
    assert p.rho.dtype == F and p.coeffs(4, 6)[0].tobytes() == np.full((1, 6), 0.9, F).tobytes() and p.coeffs(4, 6)[1].tobytes() == np.full((1, 6), 0.25, F).tobytes()
    np.testing.assert_allclose(p.std, 0.25 / np.sqrt(1.0 - np.float64(F(0.9)) ** 2))
    g = GaussMarkov(np.arange(1.0, 7.0), 0.5, 0.05).stationary_state(np.random.default_rng(1), 2000)
    assert g.shape == (2000, 6) and g.dtype == F
    np.testing.assert_allclose(g.std(axis=0), np.arange(1.0, 7.0), rtol=0.1)
    assert GaussMarkov(1.0, 0.5, 0.05).stationary_state(np.random.default_rng(1), 3, W=12).shape == (3, 12)
    with pytest.raises(ValueError):
        GaussMarkov(1.0, 0.5, 0.05).stationary_state(np.random.default_rng(1), 3)
    assert "bias_process" in gauss_markov_bias.__doc__


def test_restated_normal_is_the_oracles():
    """normal_from_bits (needed by the pair_adjacent mutant only) equals orc.normal on the oracle's pairing, bit for bit, in both branches of erfinv."""
    tail = 0
    for seed in range(60):
        key = np.array([seed * 2654435761 % 2**32, seed + 17], np.uint32)
        for W in (6, 12):
            want = orc.normal(key, W)
            got = draw(key, W)
            assert got.tobytes() == want.tobytes(), (seed, W)
            assert draw(key, W, "adjacent").tobytes() != want.tobytes()
            tail += int((np.abs(want) > 2.9).sum())
    assert tail > 0                                    # the tail polynomial was reached


@pytest.mark.parametrize("to_enu", [False, True], ids=["solver_frame", "enu"])
def test_simulate_frame_rules_of_the_processes(monkeypatch, to_enu):
    """MpcProblem.simulate under convert_to_enu: rho and scale take the permutation without the sign (as meas_noise), the states in and out and the returned rows the
    signed vector rules of disturbance and meas_bias; the process values sit behind the score, xsub last."""
    cfg = score_cfg()
    T, n = 4, 2
    Ns = 2
    seen = {}
    rows6 = np.arange(1, T * 6 + 1, dtype=F).reshape(1, T, 6)
    rows12 = np.arange(1, Ns * 12 + 1, dtype=F).reshape(1, Ns, 12)
    g6, g12 = -np.arange(1, 7, dtype=F)[None], np.arange(1, 13, dtype=F)[None]

    class Fake:
        def closed_loop(self, x0, xref, keys, T, **kw):
            seen.clear()
            seen.update(kw)
            z = lambda *s: np.zeros(s, F)                 # noqa: E731
            from sde4mbrl_px4_amd.solver import score_init
            out = (z(1, T + 1, 13), z(1, T, 4), z(1, Ns, 8), z(1, cfg.horizon, 4), z(1), np.zeros((1, 2), np.uint32), z(1, 4), z(1, Ns, 13), np.full((1, 2), 5, np.uint32),
                   z(1, 13), score_init(1), rows6, np.full((1, 2), 6, np.uint32), g6, rows12, np.full((1, 2), 7, np.uint32), g12)
            return out + ((z(1, T * n, 13),) if kw.get("substep_states") else ())
    x = np.zeros(13, F); x[6] = 1.0
    prob = MpcProblem(cfg=cfg, model=synthetic_iris(), convert_to_enu=to_enu)
    monkeypatch.setattr(prob, "solver", lambda: Fake())
    gd = GaussMarkov(np.arange(1.0, 7.0), np.arange(1.0, 7.0), 0.05)
    gb = GaussMarkov(np.arange(1.0, 13.0), np.arange(2.0, 14.0), 0.1)
    sd, sb = np.arange(10, 16, dtype=F), np.arange(20, 32, dtype=F)
    k2 = np.zeros(2, np.uint32)
    out = prob.simulate(x, k2, T, solve_period=2, plant_substeps=n, score=Score(), substep_states=True, dist_process=gd, dist_rng=np.array([1, 2], np.uint32), dist_state=sd,
                        bias_process=gb, bias_rng=np.array([3, 4], np.uint32), bias_state=sb, meas_rng=np.array([8, 9], np.uint32))
    p6, s6 = ([1, 0, 2, 3, 4, 5], np.array([1, 1, -1, 1, -1, -1], F)) if to_enu else (list(range(6)), np.ones(6, F))
    p12, s12 = ([1, 0, 2, 4, 3, 5, 6, 7, 8, 9, 10, 11], np.array([1, 1, -1, 1, 1, -1, 1, -1, -1, 1, -1, -1], F)) if to_enu else (list(range(12)), np.ones(12, F))
    d, b = seen["dist_process"], seen["bias_process"]
    assert d.coeffs(1, 6)[0].tobytes() == gd.rho[p6].tobytes() and d.coeffs(1, 6)[1].tobytes() == gd.scale[p6].tobytes()          # the permutation, no sign
    assert b.coeffs(1, 12)[0].tobytes() == gb.rho[p12].tobytes() and b.coeffs(1, 12)[1].tobytes() == gb.scale[p12].tobytes()
    assert seen["dist_state_in"].tobytes() == (sd[p6] * s6).tobytes() and seen["bias_state_in"].tobytes() == (sb[p12] * s12).tobytes()
    assert seen["dist_keys"].tolist() == [[1, 2]] and seen["bias_keys"].tolist() == [[3, 4]] and seen["meas_keys"].tolist() == [[8, 9]]
    assert "meas_noise" not in seen and "meas_bias" not in seen
    # (xs, us, info, state, key), xmeas, meas key, score, dist rows / key / state, bias rows / key / state, xsub
    assert len(out) == 15 and out[7].dtype == SCORE_DTYPE and out[-1].shape == (T * n, 13)
    assert np.asarray(out[8]).tobytes() == (rows6[0][:, p6] * s6).tobytes() and out[9].tolist() == [6, 6] and np.asarray(out[10]).tobytes() == (g6[0][p6] * s6).tobytes()
    assert np.asarray(out[11]).tobytes() == (rows12[0][:, p12] * s12).tobytes() and out[12].tolist() == [7, 7] and np.asarray(out[13]).tobytes() == (g12[0][p12] * s12).tobytes()
    # no state: None goes through; the disturbance process alone is not an observed call
    prob.simulate(x, k2, T, solve_period=2, plant_substeps=n, dist_process=gd, dist_rng=k2)
    assert seen["dist_state_in"] is None and "meas_keys" not in seen and "bias_process" not in seen


def _gm(rows, W, seed):
    r = np.random.default_rng(seed)
    return r.uniform(0.2, 0.98, (rows, W)).astype(F), r.uniform(0.05, 1.0, (rows, W)).astype(F)


@pytest.mark.parametrize("W", [W_DIST, W_BIAS])
def test_process_rows_recurrence_and_continuation(W):
    """The generator is its own recurrence on the oracle's split and normal; N steps equal any cut of them through (keys_next, state_next); a scheduled input is one
    float32 add; shared coefficients are row 0 for every episode."""
    B, N = 3, 7
    keys = chain_keys(B, 900)
    rho, scale = _gm(B, W, 1)
    g0 = np.random.default_rng(2).normal(size=(B, W)).astype(F)
    rows, kn, gn = process_rows(keys, rho, scale, g0, N, W)
    assert rows.shape == (B, N, W) and rows.dtype == F and kn.dtype == np.uint32
    for b in range(B):
        c, g = keys[b], g0[b]
        for k in range(N):
            c, e = orc.split(c, 2)
            xi = orc.normal(e, W)
            g = ((rho[b].astype(np.float64) * g.astype(np.float64)) + (scale[b] * xi).astype(F).astype(np.float64)).astype(F)      # (fma: one rounding of the exact sum)
            assert rows[b, k].tobytes() == g.tobytes()
        assert np.array_equal(kn[b], c) and gn[b].tobytes() == g.tobytes()
    for cut in (1, 3, 6):
        r1, k1, g1 = process_rows(keys, rho, scale, g0, cut, W)
        r2, k2, g2 = process_rows(k1, rho, scale, g1, N - cut, W)
        assert np.concatenate([r1, r2], axis=1).tobytes() == rows.tobytes() and np.array_equal(k2, kn) and g2.tobytes() == gn.tobytes()
    d = np.random.default_rng(3).normal(size=(N, B, W)).astype(F)
    rs, ks, gs = process_rows(keys, rho, scale, g0, N, W, scheduled=d)
    assert rs.tobytes() == (d.transpose(1, 0, 2) + rows).astype(F).tobytes() and np.array_equal(ks, kn) and gs.tobytes() == gn.tobytes()
    assert process_rows(keys, rho, scale, g0, N, W, scheduled=d[:1, :1])[0].tobytes() == (d[0, 0] + rows).astype(F).tobytes()
    shared = process_rows(keys, rho[:1], scale[:1], g0, N, W)[0]
    assert shared[0].tobytes() == rows[0].tobytes() and shared[1].tobytes() != rows[1].tobytes()
    assert process_rows(keys, rho, scale, None, N, W)[0].tobytes() == process_rows(keys, rho, scale, np.zeros((B, W), F), N, W)[0].tobytes()
    for mutant in ROW_MUTANTS:
        assert process_rows(keys, rho, scale, g0, N, W, mutant=mutant)[0].tobytes() != rows.tobytes(), mutant


@pytest.fixture(scope="module")
def shared():
    """The reference loops the tests below need, computed once: the episodes of score_cases.py at T = 6 with both processes on top of a scheduled disturbance, a
    scheduled bias and the dropout pattern of obs_cases.py."""
    cfg = score_cfg()
    model = synthetic_iris()
    B, T = B5, T6
    Ns = num_solves(T, S2)
    x0, xref, keys, kw = scored_episodes(cfg, B, 181)
    valid = np.ascontiguousarray(VALID[:Ns, :B])
    kw = dict(kw, disturbance=disturbance(T, B), meas_bias=bias_rows(Ns, B), meas_valid=valid, **drawn(B))
    run = ref(process_loop_ref, cfg, model, x0, xref, keys, T, **for_ref(kw, B))
    return cfg, model, x0, xref, keys, kw, run


def test_reference_loop_is_the_aged_loop_on_the_generated_rows(shared):
    cfg, model, x0, xref, keys, kw, run = shared
    B, T = B5, T6
    assert len(run) == 17                              # 7 + (xmeas, q, xm) + 3 + 3 + xsub
    dist_rows, bias_rows_ = run[10], run[13]
    assert dist_rows.shape == (B, T, 6) and bias_rows_.shape == (B, num_solves(T, S2), 12) and run[11].dtype == np.uint32 and run[12].shape == (B, 6)
    plain = {k: v for k, v in kw.items() if not k.startswith(("dist_", "bias_"))}
    plain.update(disturbance=dist_rows.transpose(1, 0, 2), meas_bias=bias_rows_.transpose(1, 0, 2))
    want = ref(age_loop_ref, cfg, model, x0, xref, keys, T, **plain)
    assert len(want) == 11
    for g, w in zip(run[:10] + run[-1:], want):
        assert bits_differ(np.asarray(g), np.asarray(w)) == 0 if g.dtype == F else np.array_equal(g, w)
    fk = for_ref(kw, B)
    r6, k6, g6 = process_rows(kw["dist_keys"], *fk["dist_process"], kw["dist_state_in"], T, 6, scheduled=kw["disturbance"])
    assert r6.tobytes() == dist_rows.tobytes() and np.array_equal(k6, run[11]) and g6.tobytes() == run[12].tobytes()
    # the last state is the last row without its scheduled part
    r6_, _, _ = process_rows(kw["dist_keys"], *fk["dist_process"], kw["dist_state_in"], T, 6)
    assert r6_[:, -1].tobytes() == run[12].tobytes()


def test_continuation_of_the_reference(shared):
    """T = 6 at S = 2 as 2 + 4 through every *_next value: bit for bit the whole run."""
    cfg, model, x0, xref, keys, kw, run = shared
    B, T = B5, T6
    fk = for_ref(kw, B)
    cut = 2

    def part(t0, t1, prev):
        k = dict(fk)
        k.update(disturbance=kw["disturbance"][t0:t1], meas_bias=kw["meas_bias"][t0 // S2:t1 // S2], meas_valid=kw["meas_valid"][t0 // S2:t1 // S2])
        if prev is not None:
            k.update(u_init=prev[3], stepsize_in=prev[4], u_act_in=prev[6], meas_keys=prev[8], xmeas_in=prev[9], dist_keys=prev[11], dist_state_in=prev[12],
                     bias_keys=prev[14], bias_state_in=prev[15])
        return ref(process_loop_ref, cfg, model, x0 if prev is None else prev[0][:, -1], xref, keys if prev is None else prev[5], t1 - t0, **k)
    a = part(0, cut, None)
    b = part(cut, T, a)
    finite = [0, 1, 2]
    assert np.concatenate([a[0], b[0][:, 1:]], axis=1)[finite].tobytes() == run[0][finite].tobytes()
    assert np.concatenate([a[10], b[10]], axis=1).tobytes() == run[10].tobytes() and np.concatenate([a[13], b[13]], axis=1).tobytes() == run[13].tobytes()
    for i in (3, 4, 5, 6, 8, 11, 12, 14, 15):
        assert np.asarray(b[i])[finite].tobytes() == np.asarray(run[i])[finite].tobytes(), i


@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_processes_differ_on_the_cases(shared, mutant):
    """Each mutant changes a compared bit on the cases: the rows themselves, and through them the states of the finite episodes."""
    cfg, model, x0, xref, keys, kw, run = shared
    B, T = B5, T6
    fk = for_ref(kw, B)
    Ns = num_solves(T, S2)
    sd = np.ascontiguousarray(np.asarray(kw["disturbance"], F))
    sb = np.ascontiguousarray(np.asarray(kw["meas_bias"], F))
    step6 = np.repeat((np.arange(T) % S2 == 0)[:, None], B, axis=1) if mutant == "dist_per_solve" else None
    step12 = (kw["meas_valid"] != 0) if mutant == "bias_held_on_dropout" else None
    rm = mutant if mutant in ROW_MUTANTS else None
    r6 = process_rows(kw["dist_keys"], *fk["dist_process"], kw["dist_state_in"], T, 6, scheduled=sd, mutant=rm, step=step6)
    r12 = process_rows(kw["bias_keys"], *fk["bias_process"], kw["bias_state_in"], Ns, 12, scheduled=sb, mutant=rm, step=step12)
    d6 = bits_differ(r6[0], run[10]) + bits_differ(r6[2], run[12]) + int((r6[1] != run[11]).sum())
    d12 = bits_differ(r12[0], run[13]) + bits_differ(r12[2], run[15]) + int((r12[1] != run[14]).sum())
    if mutant == "dist_per_solve":
        assert d6 > 0 and d12 == 0
    elif mutant == "bias_held_on_dropout":
        assert d12 > 0 and d6 == 0
    else:
        assert d6 > 0 and d12 > 0, (mutant, d6, d12)
    # ... and the loop sees it (one finite episode is enough to show it)
    wrong = ref(process_loop_ref, cfg, model, x0, xref, keys, T, episodes=[0, 1], mutant=mutant, **fk)
    assert bits_differ(wrong[0][:2], run[0][:2]) > 0, mutant


def test_neutral_process_is_the_aged_loop(shared):
    """scale = 0, state_in = 0 and a scheduled disturbance without negative zeros: the rows are the scheduled rows and the loop is age_loop_ref with that
    disturbance, bit for bit (rho arbitrary: g stays +0, and d + 0 = d unless d is -0)."""
    cfg, model, x0, xref, keys, kw, run = shared
    B, T = 3, T5
    Ns = num_solves(T, S2)
    x0, xref, keys = x0[:B], xref[:, :B], keys[:B]
    base = {k: (v[:B] if k in ("u_init", "stepsize_in") else v) for k, v in scored_episodes(cfg, B5, 181)[3].items()}
    d = disturbance(T, B).copy()
    d[d == 0] = 0.0                                    # (no negative zero)
    assert not np.signbit(d[d == 0]).any()
    sb = bias_rows(Ns, B)
    valid = np.ascontiguousarray(VALID[:Ns, :B])
    rho6, rho12 = _gm(B, 6, 4)[0], _gm(1, 12, 5)[0]
    neutral = dict(dist_process=(rho6, np.zeros((B, 6), F)), dist_keys=chain_keys(B, 700), dist_state_in=np.zeros((B, 6), F),
                   bias_process=(rho12, np.zeros((1, 12), F)), bias_keys=chain_keys(B, 800), bias_state_in=None)
    obs = dict(meas_keys=kw["meas_keys"][:B], meas_valid=valid)
    got = ref(process_loop_ref, cfg, model, x0, xref, keys, T, **base, disturbance=d, meas_bias=sb, **obs, **neutral)
    want = ref(age_loop_ref, cfg, model, x0, xref, keys, T, **base, disturbance=d, meas_bias=sb, **obs)
    for g, w in zip(got[:10] + got[-1:], want):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes()
    assert got[10].tobytes() == d.transpose(1, 0, 2).tobytes() and got[13].tobytes() == sb.transpose(1, 0, 2).tobytes()
    assert not got[12].any() and not got[15].any() and not np.array_equal(got[11], neutral["dist_keys"])      # the chains advance all the same


def test_moments_of_a_long_reference_run():
    """The reference alone: B = 1, W = 6, rho = 0.9, scale = sqrt(1 - 0.81), N = 20,000 steps from a stationary start, one fixed key (so the test is deterministic).
    The sample deviation is within 8 % of 1 and the lag-1 autocorrelation within 0.016 of 0.9 — each five standard errors of an AR(1) estimate at that N:
    sqrt(2 (1 + rho^2) / ((1 - rho^2) N)) / 2 ~ 1.5 % for the deviation, sqrt((1 - rho^2) / N) ~ 0.0031 for the correlation. A wrong scale, or a draw re-used
    across components, fails it."""
    N, W = 20000, 6
    rho = np.full((1, W), 0.9, F)
    scale = np.full((1, W), np.sqrt(1.0 - 0.81), F)
    g0 = np.random.default_rng(11).standard_normal((1, W)).astype(F)
    rows, _, _ = process_rows(np.array([[2024, 11]], np.uint32), rho, scale, g0, N, W)
    x = rows[0].astype(np.float64)
    for i in range(W):
        sd = x[:, i].std()
        r1 = np.corrcoef(x[:-1, i], x[1:, i])[0, 1]
        assert abs(sd - 1.0) < 0.08, (i, sd)
        assert abs(r1 - 0.9) < 0.016, (i, r1)
    # components are separate draws: no pair of components correlates beyond five standard errors of two independent AR(1) series, sqrt((1 + rho^2) / ((1 - rho^2) N))
    c = np.corrcoef(x.T)
    assert np.abs(c[~np.eye(W, dtype=bool)]).max() < 5.0 * np.sqrt((1 + 0.81) / ((1 - 0.81) * N))
