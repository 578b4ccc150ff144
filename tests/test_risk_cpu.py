"""Predicted risk (SPEC.md §12a) without a GPU: the C ABI's new entry points and their refusals, the NumPy restatement tests/risk_ref.py against its own scalar
form, against the oracle's cost (the anchor) and against tests/tube_ref.py, the wrong reducers of risk_ref.MUTANTS against the cases of tests/risk_cases.py, the
conditions those cases must meet, and the quantile / tail mapping of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import risk_cases as RC
import risk_ref as RR
import tube_cases as TC
import tube_ref as TR
from cases import bits_differ
from sde4mbrl_px4_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdempc_risk_batch", "sdempc_risk_batch_keys", "sdempc_risk_batch_dev")
F = np.float32


# ---- ABI and entry points --------------------------------------------------------------------------------------------------------------
def test_header_abi_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_risk_cfg \{[^}]*int32_t struct_size;[^}]*int32_t centre_mode;[^}]*int32_t tail_k;[^}]*int32_t n_ranks;[^}]*int32_t ranks\[8\];[^}]*\}", hdr)
    assert C.sizeof(_abi.SdempcRiskCfg) == 4 * 12
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and f"int {name}(" in hdr and hasattr(lib, name), name
        assert re.search(r"\nint " + name + r"\([^{]*\{\n\s*return guarded\(", src), name
    assert "d_risk" in re.search(r"SDEMPC_OPT_TEST_WS_FILL\s+-1 none.*?SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES", hdr, re.S).group(0)
    assert re.search(r"dev_alloc\(h, h->d_risk, [^;]*, true\)", src)          # filled under SDEMPC_OPT_TEST_WS_FILL like the other staging buffers


def _handle(max_batch=2, name="h6_p33"):
    cfg_py, model = TC.config(name)
    lib = _abi.load_library()
    cfg, keep = cfg_py.to_cfg()
    blob = model.to_blob()
    buf = C.create_string_buffer(blob, len(blob))
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(cfg), buf, len(blob), max_batch, C.byref(h)) == 0
    return lib, h, (cfg, keep, buf)


def _cfg(centre_mode=0, tail_k=3, ranks=(0, 16, 32)):
    cfg = _abi.SdempcRiskCfg()
    cfg.struct_size = C.sizeof(cfg)
    cfg.centre_mode, cfg.tail_k, cfg.n_ranks = centre_mode, tail_k, len(ranks)
    for k, r in enumerate(ranks):
        cfg.ranks[k] = r
    return cfg


def test_refusals_come_before_any_device_work():
    """Every one of these returns its code from the host checks: none may reach the first HIP call (which, without a GPU, would answer SDEMPC_EDEVICE)."""
    lib, h, keep = _handle(2)
    risk, risk_keys, risk_dev = _abi.risk_entries(lib)
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    d = np.zeros(4096, F).ctypes.data_as(fp)
    k = np.zeros(4096, np.uint32).ctypes.data_as(u32p)
    inf = np.full(64, np.inf, F)
    lo, hi = (-inf).ctypes.data_as(fp), inf.ctypes.data_as(fp)
    cfg = _cfg()
    err = lambda: lib.sdempc_last_error(h).decode()
    host = lambda c, B=1, x0=d, lo=lo, hi=hi, centre=None, outs=(d, k, d, k, k, d, d, d): risk(h, C.byref(c) if c is not None else None, B, x0, d, d, d, lo, hi, centre, *outs)
    none = (None,) * 8
    assert not lib.sdempc_device_ready(h)
    # capacity
    assert host(cfg, 3) == -5 and "max_batch" in err()
    assert risk_keys(h, C.byref(cfg), 3, d, d, d, k, lo, hi, None, d, k, d, k, k, d, d, d) == -5
    assert risk_dev(h, C.byref(cfg), 3, 1, 1, None, 1, 1, 1, 1, 1, 1, 1, 1, None) == -5
    assert host(cfg, 0) == -1
    # NULL inputs, NULL cfg, no output at all (cost alone is none)
    assert host(cfg, x0=None) == -1 and "NULL" in err()
    assert risk_keys(h, C.byref(cfg), 1, d, d, d, None, lo, hi, None, d, k, d, k, k, d, d, d) == -1 and "NULL" in err()
    assert host(None) == -1 and "NULL sdempc_risk_cfg" in err()
    assert host(cfg, outs=none) == -1 and "no output" in err()
    assert host(cfg, outs=(d,) + none[1:]) == -1 and "no output" in err()
    assert risk_dev(h, C.byref(cfg), 1, 1, 1, None, 1, None, None, None, None, None, None, None, None) == -1 and "no output" in err()
    # exit outputs without the bounds they are counted against; one bound without the other
    for outs in ((None, k, None, None, None, None, None, None), (None, None, None, k, None, None, None, None), (None, None, None, None, k, None, None, None)):
        assert host(cfg, lo=None, hi=None, outs=outs) == -1 and "need bounds" in err(), outs
    assert risk_dev(h, C.byref(cfg), 1, None, None, None, 1, None, None, 1, None, None, None, None, None) == -1 and "need bounds" in err()
    assert host(cfg, hi=None) == -1 and "come together" in err()
    # jx outputs and centre_mode 2 need xref (device form: the host forms always have it)
    assert risk_dev(h, C.byref(cfg), 1, None, None, None, None, None, 1, None, None, None, None, None, None) == -1 and "need xref" in err()
    assert risk_dev(h, C.byref(_cfg(2)), 1, 1, 1, None, None, 1, None, None, None, None, None, None, None) == -1 and "need xref" in err()
    # struct_size, centre_mode, centre rows
    bad = _cfg()
    bad.struct_size = 12
    assert host(bad) == -1 and "struct_size" in err()
    assert risk_dev(h, C.byref(bad), 1, 1, 1, None, 1, 1, None, None, None, None, None, None, None) == -1 and "struct_size" in err()
    for mode in (-1, 4):
        assert host(_cfg(mode)) == -1 and "centre_mode" in err(), mode
    assert host(_cfg(1)) == -1 and "centre rows" in err()
    # ranks and tail
    for ranks in ((), (0,) * 9, (33,), (0, -1)):
        c = _cfg(ranks=ranks[:8])
        c.n_ranks = len(ranks)
        assert host(c) == -1 and ("n_ranks" in err() or "rank" in err()), ranks
    for tk in (0, -2, 34):
        assert host(_cfg(tail_k=tk)) == -1 and "tail_k" in err(), tk
    # a NaN bound in host memory
    nanb = inf.copy()
    nanb[4] = np.nan
    assert host(cfg, hi=nanb.ctypes.data_as(fp)) == -1 and "NaN" in err()
    assert risk_keys(h, C.byref(cfg), 1, d, d, d, k, nanb.ctypes.data_as(fp), hi, None, d, k, d, k, k, d, d, d) == -1 and "NaN" in err()
    assert not lib.sdempc_device_ready(h)                      # none of the above touched the device
    lib.sdempc_destroy(h)


def test_no_refusal_touches_the_device():
    lib, h, keep = _handle(2)
    risk, _, risk_dev = _abi.risk_entries(lib)
    fp = C.POINTER(C.c_float)
    d = np.zeros(4096, F).ctypes.data_as(fp)
    for c in (_cfg(7), _cfg(tail_k=99), _cfg(ranks=(40,))):
        assert risk(h, C.byref(c), 1, d, d, d, d, None, None, None, d, None, d, None, None, d, d, d) == -1
        assert risk_dev(h, C.byref(c), 1, None, None, None, 1, None, 1, None, None, 1, 1, 1, None) == -1
    assert not lib.sdempc_device_ready(h)
    lib.sdempc_destroy(h)


def test_rank_outputs_are_limited_and_the_others_are_not():
    """jq and jtail above the selection stage's particle limit (4096 >= 1024) are SDEMPC_EINVAL from the host checks; the same call without them passes them
    (and, without a GPU, ends at the device)."""
    assert _abi.RISK_RANK_MAX_P >= 1024
    cfg_py, model = TC.config("h6_p33")
    lib = _abi.load_library()
    cfg, keep = cfg_py.replace(num_particles=_abi.RISK_RANK_MAX_P + 1).to_cfg()
    blob = model.to_blob()
    buf = C.create_string_buffer(blob, len(blob))
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(cfg), buf, len(blob), 1, C.byref(h)) == 0
    risk_dev = _abi.risk_entries(lib)[2]
    c = _cfg()
    assert risk_dev(h, C.byref(c), 1, None, None, None, 1, None, None, None, None, None, 1, None, None) == -1 and "4096" in lib.sdempc_last_error(h).decode()
    assert risk_dev(h, C.byref(c), 1, None, None, None, 1, None, None, None, None, None, None, 1, None) == -1
    assert not lib.sdempc_device_ready(h)
    lib.sdempc_destroy(h)


def test_python_interface_exists():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.solver import Risk, SdeMpcSolver, quantile_ranks, tail_count
    assert Risk._fields == ("cost", "exit", "jx", "first_exit", "outside_any", "jstat", "jq", "jtail")
    for name in ("risk", "risk_keys", "risk_dev"):
        assert callable(getattr(SdeMpcSolver, name))
    assert callable(MpcProblem.m_risk)
    first = np.array([[0, 1, 0, 2, 1]], np.uint32)              # H = 3, P = 4: one particle never leaves
    r = Risk.of(4, np.zeros(1, F), None, None, first, np.zeros((1, 4), np.uint32), np.zeros((1, 4), F), None, None)
    assert r.P == 4 and r.p_ever.tolist() == [0.75] and r.survival.tolist() == [[1.0, 0.75, 0.75, 0.25]]
    assert r._replace(cost=np.ones(1, F)).P == 4
    with pytest.raises(ValueError, match="particle count"):
        Risk(*r).p_ever
    with pytest.raises(ValueError, match="no bounds"):
        r._replace(first_exit=None).survival
    # quantile q -> rank ceil(q P) - 1 clamped; tail alpha -> max(1, ceil(alpha P)), an integer is k
    assert quantile_ranks((0.0, 0.5, 0.9, 1.0, 0.01, 0.99), 128) == [0, 63, 115, 127, 1, 126]
    assert quantile_ranks((0.0, 0.5, 1.0), 1) == [0, 0, 0] and quantile_ranks((0.5,), 33) == [16] and quantile_ranks((1.5, -1.0), 10) == [9, 0]
    assert [tail_count(a, 128) for a in (0.05, 0.1, 1.0, 1e-9)] == [7, 13, 128, 1] and tail_count(5, 128) == 5 and tail_count(np.int64(3), 9) == 3
    assert tail_count(0.1, 1) == 1


# ---- the reference against itself, the oracle and the tube -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_vectorised_and_scalar_restatements_agree(name):
    R = RC.reference(name)
    b = RR.risk_scalar(R["traj"], R["cfg"], R["model"], R["xref"], R["lo"], R["hi"], R["xmean"], R["ranks"], R["tail_k"])
    assert RR.outputs_differ(R["want"], b) == 0


@pytest.mark.parametrize("which", ["ties", "state_constr", "nonfinite", "absolute_box"])
def test_restatements_agree_on_the_special_cases(which):
    R = {"ties": RC.tie_case, "state_constr": RC.state_constr_case, "nonfinite": RC.nonfinite_case}.get(which, lambda: RC.reference("h6_p31"))()
    centre = None if which == "absolute_box" else R.get("centre", R["xmean"])
    a = RC.want(R, centre)
    b = RR.risk_scalar(R["traj"], R["cfg"], R["model"], R["xref"], R["lo"], R["hi"], centre, R["ranks"], R["tail_k"])
    assert RR.outputs_differ(a, b) == 0


@pytest.mark.parametrize("name", RC.NAMES)
def test_anchor_mean_tracking_cost_is_the_oracles_cost(name):
    """With res_mult = uerr = u_slew_coeff = u_slew_constr_coeff = 0 the rollout's cost is the §6.1 particle sum of Jx times float32 1/P: bit for bit."""
    R = RC.anchor_case(name)
    assert bits_differ(R["want"]["jstat"][:, 0], R["cost"]) == 0
    assert bits_differ(R["traj"], RC.reference(name)["traj"]) == 0          # the dynamics do not see the cost
    assert bits_differ(RC.reference(name)["want"]["jx"], R["want"]["jx"]) == 0      # ... and Jx does not see the other cost terms
    assert (RC.reference(name)["cost"] > R["cost"]).all()


@pytest.mark.parametrize("name", ("h6_p33", "h6_p130", "h7_m6_p33"))
def test_outside_any_against_the_tubes_outside(name):
    """One bounded component and no centre: outside_any[t] is the tube's outside[t][i]. Any box: max_i outside[t][i] <= outside_any[t] <= min(P, sum_i)."""
    R = RC.reference(name)
    P = R["cfg"].num_particles
    T = TC.reference(name)
    for i in (0, 4, 11):
        lo, hi = np.full((RC.B, 13), -np.inf, F), np.full((RC.B, 13), np.inf, F)
        lo[:, i], hi[:, i] = T["lo"][i], T["hi"][i]
        got = RC.want(R, None, lo, hi)["outside_any"]
        want = TR.tube(R["traj"], lo[0], hi[0])["outside"][:, :, i]
        assert np.array_equal(got, want) and 0 < got.sum() < got.size * P, i
    dev = R["traj"] - R["xmean"][:, None]
    for b in range(RC.B):
        per = TR.tube(dev[b:b + 1], R["lo"][b], R["hi"][b])["outside"][0].astype(np.int64)           # [H+1][13] of the deviations
        anyo = R["want"]["outside_any"][b].astype(np.int64)
        assert (per.max(axis=1) <= anyo).all() and (anyo <= np.minimum(P, per.sum(axis=1))).all()
        assert (anyo > per.max(axis=1)).any()                  # the joint count is not a marginal one


@pytest.mark.parametrize("name", RC.NAMES)
def test_histogram_and_single_particle(name):
    R = RC.reference(name)
    P, H = R["cfg"].num_particles, R["cfg"].horizon
    w = R["want"]
    assert (w["first_exit"].sum(axis=1) == P).all() and w["first_exit"].shape == (RC.B, H + 2)
    for b in range(RC.B):
        assert np.array_equal(w["first_exit"][b], np.bincount(w["exit"][b], minlength=H + 2))
    assert (w["jstat"][:, 2] <= w["jq"][:, 0]).all() and (w["jq"][:, 0] == w["jstat"][:, 2]).all() and (w["jq"][:, -1] == w["jstat"][:, 3]).all()
    assert (np.diff(w["jq"], axis=1) >= 0).all() and (w["jtail"] >= w["jstat"][:, 0]).all() and (w["jtail"] <= w["jstat"][:, 3]).all()
    if P == 1:
        assert (w["jstat"][:, 1] == 0).all() and not np.signbit(w["jstat"][:, 1]).any()
        assert (w["jq"] == w["jx"]).all() and (w["jtail"] == w["jx"][:, 0]).all() and (w["jstat"][:, 0] == w["jx"][:, 0]).all()


@pytest.mark.parametrize("name", RC.NAMES)
def test_cases_can_tell(name):
    """The conditions the cases were built for, so that they cannot silently lapse: every instance with P >= 31 has particles that leave and particles that never
    do, at least three occupied exit steps, and a step at which fewer particles are outside than have left so far (re-entries). A static absolute box cannot
    do that here: every particle leaves it at t = 0 (the reason the box sits on a deviation)."""
    R = RC.reference(name)
    P, H = R["cfg"].num_particles, R["cfg"].horizon
    w = R["want"]
    if P < 31:
        return
    for b in range(RC.B):
        fe, anyo = w["first_exit"][b].astype(np.int64), w["outside_any"][b].astype(np.int64)
        assert 0 < fe[H + 1] < P, (b, fe)
        assert (fe[:H + 1] > 0).sum() >= 3, (b, fe)
        assert (anyo < np.cumsum(fe[:H + 1])).any(), (b, anyo, fe)
    # on a bound means inside: each bound is attained by a particle, and that particle's deviation is inside
    dev = R["traj"] - R["xmean"][:, None]
    for b in range(RC.B):
        for i in RC.BOUNDED:
            assert (dev[b, :, 1:, i] == R["lo"][b, i]).any() and (dev[b, :, 1:, i] == R["hi"][b, i]).any()
    absolute = RC.want(R, None)
    assert (absolute["first_exit"][:, 0] == P).all()


def test_special_cases_are_what_they_claim():
    T = RC.tie_case()
    jx = T["want"]["jx"]
    assert all(len({jx[b, p].tobytes() for p in RC.TIED}) == 1 for b in range(RC.B))
    rank = np.argsort(np.argsort(jx, axis=1, kind="stable"), axis=1, kind="stable")
    n_in = (rank[:, list(RC.TIED)] >= 33 - T["tail_k"]).sum(axis=1)
    assert ((n_in > 0) & (n_in < 3)).any(), (T["tail_k"], n_in)            # the tail cuts through the trio
    S, base = RC.state_constr_case(), RC.reference("h6_p33")
    assert bits_differ(S["traj"], base["traj"]) == 0
    assert (S["want"]["jx"] > base["want"]["jx"]).mean() > 0.5 and (S["want"]["jx"] >= base["want"]["jx"]).all()
    N = RC.nonfinite_case()
    assert np.isnan(N["traj"][1]).all() and np.isfinite(N["traj"][[0, 2]]).all()
    w = N["want"]
    assert w["first_exit"][1, 0] == 33 and (w["exit"][1] == 0).all() and (w["outside_any"][1] == 33).all()
    assert np.isnan(w["jq"][1]).all() and np.isnan(w["jtail"][1]) and np.isnan(w["jstat"][1, :2]).all() and w["jstat"][1, 2] == np.inf and w["jstat"][1, 3] == -np.inf
    for b in (0, 2):
        assert all(base["want"][k][b].tobytes() == w[k][b].tobytes() for k in RR.OUTPUTS), b


def _mutant_inputs():
    for name in RC.NAMES:
        R = RC.reference(name)
        yield name, R, R["xmean"]
    yield "h6_p33_absolute", RC.reference("h6_p33"), None
    yield "ties", RC.tie_case(), RC.tie_case()["xmean"]
    yield "state_constr", RC.state_constr_case(), RC.state_constr_case()["xmean"]
    yield "nonfinite", RC.nonfinite_case(), RC.nonfinite_case()["centre"]


def test_every_mutant_changes_a_compared_word():
    assert len(RR.MUTANTS) >= 10
    caught = {m: [] for m in RR.MUTANTS}
    for name, R, centre in _mutant_inputs():
        right = RC.want(R, centre)
        for m in RR.MUTANTS:
            wrong = RR.risk(R["traj"], R["cfg"], R["model"], R["xref"], R["lo"], R["hi"], centre, R["ranks"], R["tail_k"], mutant=m)
            if RR.outputs_differ(right, wrong):
                caught[m].append(name)
    print({m: len(v) for m, v in caught.items()})
    assert all(caught.values()), [m for m, v in caught.items() if not v]
    assert caught["ties_descending"] == ["ties"]                   # only equal values can tell the tie-break
    assert "h6_p32" not in caught["padded_lanes_included"]         # no padded lane at P = 32
    assert "nonfinite" in caught["nan_not_counted"] and "h6_p33_absolute" in caught["scan_from_1"]


# ---- no new kernel symbol ----------------------------------------------------------------------------------------------------------------
def test_the_reducer_is_a_mode_of_the_noise_kernel():
    """No new __global__ symbol: the reducer's file declares no kernel, sdempc_prng.hip still has its five, and no built kernel is named for the risk."""
    import kernel_census as kc
    csrc = os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc")
    assert "__global__" not in open(os.path.join(csrc, "sdempc_risk.inc.h")).read()
    prng = open(os.path.join(csrc, "sdempc_prng.hip")).read()
    assert prng.count("__global__") == 5 and '#include "sdempc_risk.inc.h"' in prng
    for where in (kc.CSRC, kc.AV_DIR):
        built = kc.built_kernels(where)
        if built is None and where == kc.AV_DIR and not os.path.exists(os.path.join(where, "libsdempc.so")):
            continue
        assert built is not None, f"libsdempc.so / its objects are not built in {where}, or nm is missing"
        assert ("sdempc_noise_kernel", "") in built and not [k for k in built if "risk" in k[0].lower()]
