"""Closed loop on a measured state (SPEC.md §11f) without a GPU: header / binding / library agree on the new symbol at ABI version 3, every refusal of
sdempc_closed_loop_batch_observed (no HIP call may happen before them) and of the Python surface, the reference of tests/obs_loop_ref.py against
fault_loop_ref with a neutral observation, the discrimination of six wrong loops on the inputs of the GPU cases (tests/obs_cases.py), the dropout rules (a
dropout at solve 0 holds xmeas_in or x0, consecutive dropouts hold one row, the chain advances through them), continuation, the moments of `measure` and
the frame rules of MpcProblem.simulate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
from cases import ROOT, bits_differ
from fault_loop_ref import fault_loop_ref
from obs_cases import B5, D1, N2, NS3, S2, T5, VALID, bias_rows, dead_motor, episodes, full_case, held, meas_keys, noise_rows, obs_cfg, observation
from obs_loop_ref import MUTANTS, measure, obs_loop_ref
from loop_cases import REF_NAME
from sde4mbrl_px4_amd import _abi, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import SdeMpcSolver
from sde4mbrl_px4_amd.utils import enu2ned
from timed_loop_ref import num_solves

F = np.float32
NEW = "sdempc_closed_loop_batch_observed"


def ref(cfg, model, x0, xref, keys, T, **kw):
    """obs_loop_ref for the keyword arguments of SdeMpcSolver.closed_loop."""
    return obs_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T, **{"plants": None, **{REF_NAME.get(k, k): v for k, v in kw.items()}})


def test_abi_surface_of_the_observed_entry_point():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_obs_cfg \{[^}]*struct_size;[^}]*const float\* sigma;[^}]*const float\* beta;[^}]*obs_solves;[^}]*obs_batch;"
                     r"[^}]*const int32_t\* valid;[^}]*valid_solves;[^}]*valid_batch;[^}]*\}", hdr)
    R = _abi.SdempcObsCfg
    assert C.sizeof(R) == 48 and R.sigma.offset == 8 and R.beta.offset == 16 and R.obs_solves.offset == 24 and R.obs_batch.offset == 28
    assert R.valid.offset == 32 and R.valid_solves.offset == 40 and R.valid_batch.offset == 44
    assert NEW in _abi.EXPORTED_SYMBOLS and f"int {NEW}(" in hdr
    proto = re.search(r"int " + NEW + r"\((.*?)\);", hdr, re.S).group(1)
    assert re.search(r"sdempc_obs_cfg\* obs[^,]*,\s*const uint32_t\* obs_keys[^,]*,\s*const float\* xmeas_in[^,]*,\s*const sdempc_fault_cfg\* fault_cfg", proto)
    assert re.search(r"float\* xsub[^,]*,\s*float\* xmeas[^,]*,\s*uint32_t\* obs_keys_next[^,]*,\s*float\* xmeas_next[^,]*$", proto.strip())
    # ... and between the two every argument of the fault entry point, in its order
    fproto = re.search(r"int sdempc_closed_loop_batch_fault\((.*?)\);", hdr, re.S).group(1)
    names = lambda p: [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", p, flags=re.S).split(",")]      # noqa: E731
    assert names(proto)[4:-3] == names(fproto)[1:] and names(proto)[0] == names(fproto)[0] == "h"
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3 and hasattr(lib, NEW)
    fn = _abi.observed_entry(lib)
    assert len(fn.argtypes) == len(_abi.fault_entry(lib).argtypes) + 6 and fn.restype is C.c_int
    assert fn.argtypes[1]._type_ is _abi.SdempcObsCfg and fn.argtypes[4]._type_ is _abi.SdempcFaultCfg
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert re.search(r"\nint " + NEW + r"\([^{]*\{\n\s*return guarded\(", src)


class _Call:
    """ctypes buffers of one sdempc_closed_loop_batch_observed call; every field can be overridden."""

    def __init__(self, cfg, B=4, T=5):
        self.B, self.T, self.H, self.m = B, T, cfg.horizon, cfg.num_motors

    def __call__(self, lib, h, blobs, obs=True, o_size=None, sigma="ok", beta="ok", obs_solves=None, obs_batch=None, valid="ok", valid_solves=None, valid_batch=None,
                 okeys=True, xm_in=False, xmeas=None, okeys_next=None, xm_next=None, fault=None, f_size=None, rate=False, ws=None, S=2, D=0, alpha=0.0,
                 kp=(0.1, 0.1, 0.1), null_xs=False, substeps=2, xref_solves=1, B=None, T=None, xsub=False, t_size=None):
        fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        B = self.B if B is None else B
        T = self.T if T is None else T
        Tb = max(T, 1)
        Ns = num_solves(Tb, max(S, 1))
        x0 = np.zeros((B, 13), F); x0[:, 6] = 1.0
        xref = np.zeros((max(xref_solves, 1), 1, self.H + 1, 13), F); xref[..., 6] = 1.0
        keys, qk = np.zeros((B, 2), np.uint32), np.zeros((B, 2), np.uint32)
        xs, us, info = np.zeros((B, Tb + 1, 13), F), np.zeros((B, Tb, self.m), F), np.zeros((B, Ns, 8), F)
        b_ws, b_gn, b_tn = np.zeros((B, Tb, 4), F), np.zeros((B, 3), F), np.zeros((B, self.H, 3), F)
        b_xsub = np.zeros((B, Tb * max(substeps, 1), 13), F)
        b_xmi, b_xm, b_qn, b_xn = np.zeros((B, 13), F), np.zeros((B, Ns, 13), F), np.zeros((B, 2), np.uint32), np.zeros((B, 13), F)
        xmeas = obs if xmeas is None else xmeas                     # (the observation outputs follow `obs` unless stated)
        okeys_next = obs if okeys_next is None else okeys_next
        xm_next = obs if xm_next is None else xm_next
        ws = rate if ws is None else ws
        rc = _abi.SdempcRateCfg()
        rc.struct_size = C.sizeof(rc)
        for a in range(3):
            rc.kp[a], rc.ki_dt[a], rc.integ_limit[a] = kp[a], 0.0, 0.1
        sg = np.full((Ns, B, 12), 0.01, F) if isinstance(sigma, str) else (None if sigma is None else np.ascontiguousarray(sigma, F))
        be = np.full((Ns, B, 12), -0.01, F) if isinstance(beta, str) else (None if beta is None else np.ascontiguousarray(beta, F))
        va = np.ones((Ns, B), np.int32) if isinstance(valid, str) else (None if valid is None else np.ascontiguousarray(valid, np.int32))
        rows = sg if sg is not None else be
        oc = _abi.SdempcObsCfg(C.sizeof(_abi.SdempcObsCfg) if o_size is None else o_size, None if sg is None else sg.ctypes.data_as(fp),
                               None if be is None else be.ctypes.data_as(fp),
                               (1 if rows is None else rows.shape[0]) if obs_solves is None else obs_solves,
                               (1 if rows is None else rows.shape[1]) if obs_batch is None else obs_batch,
                               None if va is None else va.ctypes.data_as(i32p),
                               (1 if va is None else va.shape[0]) if valid_solves is None else valid_solves,
                               (1 if va is None else va.shape[1]) if valid_batch is None else valid_batch)
        f = None if fault is None else np.ascontiguousarray(fault, F)
        fc = _abi.SdempcFaultCfg(C.sizeof(_abi.SdempcFaultCfg) if f_size is None else f_size, None if f is None else f.ctypes.data_as(fp),
                                 1 if f is None else f.shape[0], 1 if f is None else f.shape[1])
        tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg) if t_size is None else t_size, S, D, alpha)
        pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), len(blobs), substeps, 0.0, -1, -1)
        bufs = (C.c_char_p * max(len(blobs), 1))(*blobs)
        sz = (C.c_size_t * max(len(blobs), 1))(*[len(b) for b in blobs])
        return _abi.observed_entry(lib)(
            h, C.byref(oc) if obs else None, qk.ctypes.data_as(u32p) if okeys else None, b_xmi.ctypes.data_as(fp) if xm_in else None,
            C.byref(fc) if (f is not None or f_size is not None) else None, C.byref(rc) if rate else None, None, C.byref(tc), C.byref(pc),
            C.cast(bufs, C.POINTER(C.c_void_p)), sz, None, B, T, x0.ctypes.data_as(fp),
            xref.ctypes.data_as(fp), xref_solves, 1, keys.ctypes.data_as(u32p), None, None, None, None if null_xs else xs.ctypes.data_as(fp),
            us.ctypes.data_as(fp), info.ctypes.data_as(C.POINTER(_abi.SdempcInfo)), None, None, None, None,
            None, None, b_ws.ctypes.data_as(fp) if ws else None, b_gn.ctypes.data_as(fp) if rate else None, b_tn.ctypes.data_as(fp) if rate else None,
            b_xsub.ctypes.data_as(fp) if xsub else None,
            b_xm.ctypes.data_as(fp) if xmeas else None, b_qn.ctypes.data_as(u32p) if okeys_next else None, b_xn.ctypes.data_as(fp) if xm_next else None)


def test_observed_argument_checks_make_no_hip_call():
    import torch
    lib = _abi.load_library()
    cfg = obs_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    hexa = synthetic_hexa().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EBLOB, EDEVICE, ECAPACITY = -1, -2, -3, -5
    B, T, Ns = 4, 5, 3
    nan, inf = float("nan"), float("inf")
    ok = np.full((Ns, B, 12), 0.01, F)
    neg = ok.copy(); neg[1, 2, 7] = -1e-30
    nan_s = ok.copy(); nan_s[2, 3, 11] = nan                      # the very last entry
    inf_s = ok.copy(); inf_s[0, 0, 0] = inf
    nan_b = ok.copy(); nan_b[2, 1, 5] = nan
    inf_b = ok.copy(); inf_b[2, 3, 11] = -inf
    ok_v = np.ones((Ns, B), np.int32)
    two_v = ok_v.copy(); two_v[2, 3] = 2
    neg_v = ok_v.copy(); neg_v[0, 1] = -1
    bad_f = np.ones((1, 1, 4, 2), F); bad_f[0, 0, 3, 1] = nan
    try:
        call = _Call(cfg, B, T)               # S = 2 (Ns = 3), n = 2
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(o_size=40), EINVAL, "obs: struct_size"),
            (dict(o_size=40, sigma=None, beta=None, valid=None), EINVAL, "obs: struct_size"),
            (dict(sigma=ok[:2]), EINVAL, "obs_solves"),
            (dict(obs_solves=0), EINVAL, "obs_solves"),
            (dict(sigma=None, beta=ok[:2]), EINVAL, "obs_solves"),
            (dict(sigma=ok[:, :2], beta=ok[:, :2]), EINVAL, "obs_batch"),
            (dict(obs_batch=B + 1), EINVAL, "obs_batch"),
            (dict(valid=ok_v[:2]), EINVAL, "valid_solves"),
            (dict(valid_solves=T), EINVAL, "valid_solves"),
            (dict(valid=ok_v[:, :3]), EINVAL, "valid_batch"),
            (dict(valid_batch=0), EINVAL, "valid_batch"),
            (dict(sigma=neg), EINVAL, "sigma holds a non-finite or negative"),
            (dict(sigma=nan_s), EINVAL, "sigma holds a non-finite or negative"),
            (dict(sigma=inf_s), EINVAL, "sigma holds a non-finite or negative"),
            (dict(sigma=nan_s[2:, 3:], beta=None), EINVAL, "sigma holds a non-finite or negative"),
            (dict(beta=nan_b), EINVAL, "beta holds a non-finite"),
            (dict(beta=inf_b), EINVAL, "beta holds a non-finite"),
            (dict(sigma=None, beta=inf_b[2:, 3:]), EINVAL, "beta holds a non-finite"),
            (dict(valid=two_v), EINVAL, "other than 0 / 1"),
            (dict(valid=neg_v), EINVAL, "other than 0 / 1"),
            (dict(okeys=False), EINVAL, "obs_keys is NULL"),
            # an observation pointer without an obs cfg, one at a time
            (dict(obs=False), EINVAL, "without an obs cfg"),
            (dict(obs=False, okeys=False, xm_in=True), EINVAL, "without an obs cfg"),
            (dict(obs=False, okeys=False, xmeas=True), EINVAL, "without an obs cfg"),
            (dict(obs=False, okeys=False, okeys_next=True), EINVAL, "without an obs cfg"),
            (dict(obs=False, okeys=False, xm_next=True), EINVAL, "without an obs cfg"),
            # ... and everything the fault entry point refuses (a sample of each layer; the shared path is that of tests/test_fault_loop_cpu.py)
            (dict(f_size=20), EINVAL, "fault: struct_size"),
            (dict(fault=bad_f), EINVAL, "non-finite"),
            (dict(fault=np.ones((2, 1, 4, 2), F)), EINVAL, "fault_ticks"),
            (dict(ws=True), EINVAL, "without a rate cfg"),
            (dict(rate=True, kp=(0.1, nan, 0.1)), EINVAL, "non-finite gain"),
            (dict(rate=True, ws=False), EINVAL, "ws is NULL"),
            (dict(null_xs=True), EINVAL, "NULL host pointer"),
            (dict(t_size=12), EINVAL, "struct_size"),
            (dict(S=0), EINVAL, "solve_period"),
            (dict(D=5), EINVAL, "solve_delay"),
            (dict(alpha=nan), EINVAL, "lag_alpha"),
            (dict(xref_solves=5), EINVAL, "xref_solves"),
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
        # valid arguments reach the device: every NULL that is allowed, broadcast axes, ignored axes of absent rows, extreme but finite rows, obs NULL (the fault call)
        good = 0 if torch.cuda.is_available() else EDEVICE
        big = ok.copy(); big[...] = 3.0e38
        for kw in (dict(), dict(sigma=None), dict(beta=None), dict(valid=None), dict(sigma=None, beta=None, valid=None, obs_solves=99, obs_batch=-1),
                   dict(valid=None, valid_solves=99, valid_batch=-3), dict(xm_in=True), dict(xmeas=False, okeys_next=False, xm_next=False),
                   dict(sigma=ok[:1], beta=ok[:1]), dict(sigma=ok[:, :1], beta=ok[:, :1]), dict(sigma=ok[:1, :1], beta=None), dict(valid=ok_v[:1]),
                   dict(valid=ok_v[:, :1] * 0), dict(sigma=big, beta=-big), dict(rate=True, xsub=True, fault=np.ones((1, 1, 4, 2), F)),
                   dict(obs=False, okeys=False)):
            rc = call(lib, h, **{"blobs": [blob], **kw})
            assert rc == good, (sorted(kw), rc, lib.sdempc_last_error(h).decode())
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_checks_the_measurement_keywords():
    cfg = obs_cfg()
    model = synthetic_iris()
    B, T = 3, 5
    S = SdeMpcSolver(cfg, model, max_batch=B)
    x0 = np.zeros((B, 13), F)
    xref = np.zeros((cfg.horizon + 1, 13), F)
    k = np.zeros((B, 2), np.uint32)
    one = np.full(12, 0.01, F)
    with pytest.raises(ValueError, match="meas_keys"):
        S.closed_loop(x0, xref, k, T, meas_noise=one)
    with pytest.raises(ValueError, match="meas_keys"):
        S.closed_loop(x0, xref, k, T, meas_valid=np.ones(T, np.int32))
    for kw in (dict(meas_keys=k), dict(xmeas_in=x0),                                                         # neither does anything without one of the three
               dict(meas_noise=-one, meas_keys=k), dict(meas_noise=one * np.nan, meas_keys=k), dict(meas_bias=one * np.inf, meas_keys=k),
               dict(meas_noise=np.ones(13, F), meas_keys=k), dict(meas_noise=np.ones((2, 12), F), meas_keys=k, solve_period=2),           # Ns = 3
               dict(meas_noise=np.ones((3, 2, 12), F), meas_keys=k, solve_period=2), dict(meas_valid=np.ones(2, np.int32), meas_keys=k, solve_period=2),
               dict(meas_valid=np.full(3, 2), meas_keys=k, solve_period=2), dict(meas_noise=one, meas_keys=k[:2]),
               dict(meas_noise=one, meas_keys=k, xmeas_in=x0[:2]),
               dict(meas_noise=one, meas_keys=k, solve_period=2, solve_delay=3)):                           # the timing checks still apply
        with pytest.raises(ValueError):
            S.closed_loop(x0, xref, k, T, **kw)
    assert not S.device_ready()
    S.close()


@pytest.fixture(scope="module")
def shared():
    """The right loop on the inputs of the GPU cases, computed once: {rate loop name: the full case's result}."""
    cfg = obs_cfg()
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 111)
    runs = {rate: ref(cfg, model, x0, xref, keys, T5, substep_states=True, **full_case(model, rate)) for rate in (None, "stiff")}
    return cfg, model, x0, xref, keys, runs


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_neutral_observation_is_the_fault_loop(rate):
    """sigma and beta zero (given as zeros, and as None), always valid: fault_loop_ref bit for bit — with a rate loop, a fault, S = 2 and substeps = 2."""
    cfg = obs_cfg()
    model = synthetic_iris()
    B = 2
    x0, xref, keys = episodes(cfg, B, 112)
    assert not np.signbit(x0[x0 == 0]).any()                     # (no -0 component: a neutral observation would turn it into +0)
    kw = {k: v for k, v in full_case(model, rate, B=B).items() if not k.startswith("meas_") and k != "xmeas_in"}
    kw = {REF_NAME.get(k, k): v for k, v in kw.items()}
    want = fault_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T5, substep_states=True, **kw)
    for more in (dict(), dict(meas_noise=np.zeros(12, F), meas_bias=np.zeros((NS3, B, 12), F), meas_valid=np.ones(NS3, np.int32), xmeas_in=held(B))):
        got = obs_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T5, substep_states=True, meas_keys=meas_keys(B), **more, **kw)
        assert len(got) == len(want) + 3
        for g, w in zip(got[:-4] + got[-1:], want):
            assert g.tobytes() == w.tobytes()
        assert got[-4].tobytes() == got[0][:, 0:T5:S2].tobytes() and got[-2].tobytes() == got[-4][:, -1].tobytes()       # xmeas is x at each solve
    assert obs_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T5, substep_states=True, **kw)[0].tobytes() == want[0].tobytes()      # meas_keys None: the call itself


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
def test_dropout_rules_on_the_shared_case(shared, rate):
    cfg, model, x0, xref, keys, runs = shared
    run = runs[rate]
    xs, xmeas, q_next, xm_next = run[0], run[-4], run[-3], run[-2]
    kw = full_case(model, rate)
    assert all(np.isfinite(v).all() for v in run if v.dtype == F)
    sigma, beta, xin = kw["meas_noise"], kw["meas_bias"], kw["xmeas_in"]
    for b in range(B5):
        q, row = kw["meas_keys"][b], xin[b]
        for j in range(NS3):
            q, me = orc.split(q, 2)                               # the chain of an always-valid run: one split per solve
            if VALID[j, b]:
                row = measure(xs[b, j * S2], me, sigma[j, b], beta[j, b])     # ... so the draw after a dropout is the one that run makes at this solve
            assert xmeas[b, j].tobytes() == row.tobytes(), (b, j)
        assert np.array_equal(q_next[b], q) and xm_next[b].tobytes() == row.tobytes()
    assert xmeas[0, 0].tobytes() == xin[0].tobytes() and xmeas[3, 0].tobytes() == xin[3].tobytes()          # a dropout at solve 0 holds xmeas_in
    assert xmeas[1, 1].tobytes() == xmeas[1, 2].tobytes() == xmeas[1, 0].tobytes()                          # two consecutive dropouts hold the same row
    assert xmeas[3, 1].tobytes() == xin[3].tobytes()
    # ... and x0 when xmeas_in is None; nothing else of episode 0 changes before its first valid solve's consequences
    eps = [0, 3]
    no_in = ref(cfg, model, x0, xref, keys, T5, substep_states=True, episodes=eps, **{**kw, "xmeas_in": None})
    assert no_in[-4][0, 0].tobytes() == x0[0].tobytes() and no_in[-4][3, 0].tobytes() == no_in[-4][3, 1].tobytes() == x0[3].tobytes()
    assert bits_differ(no_in[0][eps], xs[eps]) > 0                                                          # (the held row does reach the solve)
    # the observation never touches the main chain: an unobserved run ends on the same keys
    plain = {REF_NAME.get(k, k): v for k, v in kw.items() if not k.startswith("meas_") and k != "xmeas_in"}
    assert np.array_equal(fault_loop_ref(cfg, model, x0=x0, xref=xref, keys=keys, T=T5, episodes=[2], **plain)[5][2], run[5][2])
    # the measurement is not the state: every valid solve's row differs from x in all four groups
    for sl in (slice(0, 3), slice(3, 6), slice(6, 10), slice(10, 13)):
        assert bits_differ(xmeas[2, :, sl], xs[2, 0:T5:S2, sl]) > 0


@pytest.mark.parametrize("rate", [None, "stiff"], ids=["motors", "rate"])
@pytest.mark.parametrize("mutant", MUTANTS)
def test_wrong_loops_differ_on_the_shared_case(shared, mutant, rate):
    cfg, model, x0, xref, keys, runs = shared
    eps = [0, 4]                              # a dropout followed by valid solves; valid solves followed by a dropout
    right = runs[rate]
    wrong = ref(cfg, model, x0, xref, keys, T5, substep_states=True, mutant=mutant, episodes=eps, **full_case(model, rate))
    assert len(right) == len(wrong)
    assert sum(bits_differ(r[eps], w[eps]) for r, w in zip(right, wrong) if r.dtype == F) > 0, (mutant, rate)
    assert bits_differ(right[-4][eps], wrong[-4][eps]) > 0                   # each of them shows in xmeas itself
    assert np.array_equal(right[5][eps], wrong[5][eps])                      # the main chain is S and T only


def test_continuation_split_at_a_multiple_of_the_period(shared):
    """T = 5 as 4 + 1 at S = 2: every schedule sliced at tick 4, the observation rows at solve 2."""
    cfg, model, x0, xref, keys, runs = shared
    full, kw = runs["stiff"], full_case(model, "stiff")
    cut = lambda v, a, b: None if v is None else v[a:b]                   # noqa: E731
    ticks, solves = ("plant_of", "disturbance", "fault"), ("meas_noise", "meas_bias", "meas_valid")
    part = lambda t0, t1, j0, j1: {k: (cut(v, t0, t1) if k in ticks else cut(v, j0, j1) if k in solves else v) for k, v in kw.items()}       # noqa: E731
    a = ref(cfg, model, x0, xref, keys, 4, substep_states=True, **part(0, 4, 0, 2))
    nxt = dict(u_init=a[3], stepsize_in=a[4], u_act_in=a[6], rate_integ_in=a[8], rate_tail_in=a[9], meas_keys=a[-3], xmeas_in=a[-2])
    b = ref(cfg, model, a[0][:, -1], xref, a[5], 1, substep_states=True, **{**part(4, 5, 2, 3), **nxt})
    cat = lambda i: np.concatenate([a[i], b[i]], 1)                       # noqa: E731
    joined = (np.concatenate([a[0], b[0][:, 1:]], 1), cat(1), cat(2)) + tuple(b[3:7]) + (cat(7),) + tuple(b[8:10]) + (cat(10),) + tuple(b[11:13]) + (cat(13),)
    assert len(joined) == len(full) == 14
    for i, (g, w) in enumerate(zip(joined, full)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), i


def test_moments_of_the_measurement():
    """measure over 4,096 consecutive keys from the identity state (p = v = omega = 0, attitude (1, 0, 0, 0): then e is read back exactly, e = xm for the
    additive groups and 2 xm[7..9] for the attitude). With N samples of a normal the sample mean has deviation sigma / sqrt(N) and the sample deviation
    sigma / sqrt(2 N): both bounds are five of those."""
    N = 4096
    x = np.zeros(13, F); x[6] = 1.0
    sigma, beta = noise_rows(1, 1)[0, 0], bias_rows(1, 1)[0, 0]
    sigma[4] = F(0.07)                                            # (noise_rows plants an exact zero there)
    e = np.zeros((N, 12))
    for k in range(N):
        xm = measure(x, np.array([7, k], np.uint32), sigma, beta)
        assert xm[6] == 1.0
        e[k] = np.concatenate([xm[0:6], 2.0 * xm[7:10].astype(np.float64), xm[10:13]])
    s64 = sigma.astype(np.float64)
    r_mean = np.abs(e.mean(0) - beta) / (s64 / np.sqrt(N))
    r_dev = np.abs(e.std(0, ddof=1) - s64) / (s64 / np.sqrt(2 * N))
    print("worst |mean - beta| / (sigma / sqrt N):", float(r_mean.max()), "worst |dev - sigma| / (sigma / sqrt 2N):", float(r_dev.max()))
    assert (r_mean < 5.0).all(), r_mean
    assert (r_dev < 5.0).all(), r_dev
    # a zero scale leaves the bias alone, whatever the draw
    sigma0 = sigma.copy(); sigma0[4] = 0.0
    assert all(measure(x, np.array([7, k], np.uint32), sigma0, beta)[4] == beta[4] for k in range(8))


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
        self.xmeas, self.qn = rng.normal(size=(1, Ns, 13)).astype(F), np.array([[5, 6]], np.uint32)
        self.xsub = rng.normal(size=(1, T * self.n, 13)).astype(F)
        if "meas_keys" in kw:
            out += (self.xmeas, self.qn, self.xmeas[:, -1].copy())
        return out + (self.xsub,) if kw.get("substep_states") else out


@pytest.mark.parametrize("to_enu", [True, False])
def test_simulate_frame_rules(to_enu):
    """sigma and beta are given in the frame of x: under convert_to_enu the p and v triples follow (x, y, z) -> (y, x, -z), the theta and omega triples
    (wx, wy, wz) -> (wx, -wy, -wz), a scale without the sign; xmeas comes back in the frame of x row by row."""
    cfg = obs_cfg()
    T, n, m, Ns = 5, 2, 4, 3
    prob = MpcProblem(cfg=cfg, model=synthetic_iris(), convert_to_enu=to_enu)
    fake = _FakeSolver(m, cfg.horizon, n)
    prob._solver, prob._pid = fake, os.getpid()
    x = np.zeros(13, F); x[6] = 1.0
    s = np.arange(1, 13, dtype=F) / 100                                   # every component distinct
    be = np.stack([np.arange(1, 13, dtype=F) * (j + 1) / -50 for j in range(Ns)])
    v = np.array([1, 0, 1])
    out = prob.simulate(x, np.zeros(2, np.uint32), T, plant_substeps=n, solve_period=2, meas_noise=s, meas_bias=be, meas_valid=v, meas_rng=np.array([3, 4], np.uint32),
                        substep_states=True)
    assert len(out) == 8 and out[5].shape == (Ns, 13) and out[7].shape == (T * n, 13) and np.array_equal(out[6], [5, 6])
    want = np.stack([enu2ned(r, np) for r in fake.xmeas[0]]) if to_enu else fake.xmeas[0]
    assert out[5].tobytes() == np.ascontiguousarray(want, F).tobytes()
    want = np.stack([enu2ned(r, np) for r in fake.xsub[0]]) if to_enu else fake.xsub[0]
    assert out[7].tobytes() == np.ascontiguousarray(want, F).tobytes()
    if to_enu:                                                            # converted by hand
        s_w = np.array([s[1], s[0], s[2], s[4], s[3], s[5], s[6], s[7], s[8], s[9], s[10], s[11]], F)
        b_w = np.stack([[r[1], r[0], -r[2], r[4], r[3], -r[5], r[6], -r[7], -r[8], r[9], -r[10], -r[11]] for r in be]).astype(F)
    else:
        s_w, b_w = s, be
    assert fake.kw["meas_noise"].shape == (1, 1, 12) and fake.kw["meas_noise"].tobytes() == s_w.tobytes()
    assert fake.kw["meas_bias"].shape == (Ns, 1, 12) and fake.kw["meas_bias"].tobytes() == b_w.tobytes()
    assert fake.kw["meas_valid"].shape == (Ns, 1) and np.array_equal(fake.kw["meas_valid"][:, 0], v)
    assert fake.kw["meas_keys"].shape == (1, 2) and np.array_equal(fake.kw["meas_keys"][0], [3, 4])
    out = prob.simulate(x, np.zeros(2, np.uint32), T, plant_substeps=n, solve_period=2, meas_bias=be[0], meas_rng=np.array([3, 4], np.uint32))
    assert len(out) == 7 and "meas_noise" not in fake.kw and fake.kw["meas_bias"].shape == (1, 1, 12)
    out = prob.simulate(x, np.zeros(2, np.uint32), T, plant_substeps=n, solve_period=2)
    assert len(out) == 5 and not any(k.startswith("meas_") for k in fake.kw)
    for bad in (dict(meas_noise=s), dict(meas_rng=np.zeros(2, np.uint32)), dict(meas_noise=np.ones((T, 12), F), meas_rng=np.zeros(2, np.uint32)),
                dict(meas_valid=np.ones(T, int), meas_rng=np.zeros(2, np.uint32)), dict(meas_bias=np.ones(13, F), meas_rng=np.zeros(2, np.uint32))):
        with pytest.raises(ValueError):
            prob.simulate(x, np.zeros(2, np.uint32), T, solve_period=2, **bad)
