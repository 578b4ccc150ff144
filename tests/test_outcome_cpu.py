"""Predicted outcome (SPEC.md §12c) without a GPU: the reference's per-particle words EQUAL the episode score of tests/score_loop_ref.py (a particle is an
episode), the invariants between the outputs, the wrong reducers, every refusal through the C ABI before any device work, the Python conveniences, and that the
reducer is a mode of the noise kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import outcome_cases as OC
import outcome_ref as OR
import score_loop_ref as SR
from sde4mbrl_px4_amd import _abi
from sde4mbrl_px4_amd import solver as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdempc_outcome_batch", "sdempc_outcome_batch_keys", "sdempc_outcome_batch_dev")
F = np.float32
U = np.uint32


def _variants(name):
    """(what, traj, kwargs of outcome_ref.outcome) of a case: the xref window, the four target shapes, and the special tensor where the case has the particles"""
    R = OC.reference(name)
    out = [("xref", R["traj"], dict(xref=R["xref"]))]
    for ps, pi in OC.TARGET_SHAPES:
        out.append((f"rows step={ps} inst={pi}", R["traj"], dict(target=OC.targets(R["xref"], ps, pi))))
    if R["cfg"].num_particles >= 8:
        out.append(("special", OC.synthetic_special(name), dict(xref=R["xref"])))
        out.append(("special, one target row", OC.synthetic_special(name), dict(target=OC.targets(R["xref"], False, True))))
    return R, out


# ---- the anchor: a particle is an episode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.NAMES)
def test_particle_words_equal_the_episode_score_of_the_particles_rows(name):
    """words[b][p] == words 0 .. 10 of score_loop_ref.score_rows run on particle p's rows as an episode of T = H ticks: xs = the particle's H + 1 states, zero
    us / info, S = 1, the same thresholds, the target rows tick-major. Integer words exactly, float words by bit pattern with NaNs as a class."""
    R, variants = _variants(name)
    cfg = R["cfg"]
    H, m = cfg.horizon, cfg.num_motors
    for what, traj, kw in variants:
        got = OR.outcome(traj, R["thresholds"], ranks=R["ranks"], **kw)["words"]
        g = OR.target_rows(OC.B, H, kw.get("xref"), kw.get("target"))
        P = traj.shape[1] if name != "h6_p300" else 40                     # (the scalar reference walks one row at a time: a slice of the largest case)
        for b in range(OC.B):
            xs = traj[b, :P]                                               # P episodes of H ticks
            ref = np.ascontiguousarray(np.broadcast_to(g[b, 1:, None, :], (H, P, 13)))       # [T][episode][13]
            want = SR.score_rows(xs, np.zeros((P, H, m), F), np.zeros((P, H, 8), F), None, ref, cfg, R["thresholds"], False, 1)
            a, w = np.zeros((P, 16), U), np.zeros((P, 16), U)
            a[:, :11], w[:, :11] = got[b, :P], want[:, :11]
            assert SR.words_differ(a, w) == 0, (name, what, b)


# ---- invariants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.NAMES)
def test_invariants_between_the_outputs(name):
    R, variants = _variants(name)
    H = R["cfg"].horizon
    for what, traj, kw in variants:
        P = traj.shape[1]
        o = OR.outcome(traj, R["thresholds"], ranks=R["ranks"], **kw)
        w = o["words"]
        assert (o["first_fail"].sum(axis=1) == P).all(), (name, what)
        assert (o["fail_step"][..., 4:5] >= o["fail_step"][..., :4]).all() and (o["fail_step"][..., 4] <= o["fail_step"][..., :4].sum(axis=-1)).all()
        assert (o["fail_step"] <= P).all() and (w[..., 0] == H).all()
        for k in range(4):
            assert np.array_equal(o["cause_ever"][:, k], ((w[..., 9] >> U(k)) & 1).sum(axis=1)), (name, what, k)
            assert (o["cause_ever"][:, k] >= o["fail_step"][..., k].max(axis=1)).all()
        assert np.array_equal(o["first_fail"][:, H], (w[..., 8] == SR.NONE).sum(axis=1)) and np.array_equal(w[..., 8] == SR.NONE, w[..., 9] == 0)
        assert np.array_equal(o["fail_step"][..., 4].sum(axis=1), w[..., 10].sum(axis=1))        # rows with a cause, counted both ways
        # the failures of row r are at least the first failures of row r, and the survivors only shrink
        assert (o["fail_step"][..., 4] >= o["first_fail"][:, :H]).all()
        # no channel and no aggregate is -0.0: the order's two zeros never meet here (outcome_ref's docstring)
        for q in ("chan_stat", "agg_stat", "chan_q", "agg_q"):
            if o[q] is not None:
                assert not (o[q].view(U) == 0x80000000).any(), (name, what, q)
        rk = list(R["ranks"] or ())
        if 0 in rk and P - 1 in rk:
            lo, hi = rk.index(0), rk.index(P - 1)
            fin = ~np.isnan(o["chan_q"][..., hi])                          # a NaN sorts on top: the column has one iff the top rank is one
            assert np.array_equal(o["chan_q"][..., lo][fin], o["chan_stat"][..., 1][fin]) and np.array_equal(o["chan_q"][..., hi][fin], o["chan_stat"][..., 2][fin])
            fin = ~np.isnan(o["agg_q"][..., hi])
            assert np.array_equal(o["agg_q"][..., lo][fin], o["agg_stat"][..., 1][fin]) and np.array_equal(o["agg_q"][..., hi][fin], o["agg_stat"][..., 2][fin])
            # every order statistic of an aggregate is one particle's word
            for b in range(OC.B):
                for j, wd in enumerate(OR.AGG_WORDS):
                    have = set(w[b, :, wd].tolist()) | {0x7FC00000}
                    assert set(o["agg_q"][b, j].view(U).tolist()) <= have, (name, what, b, j)


def test_the_special_tensor_is_what_it_claims():
    R = OC.reference("h6_p33")
    o = OR.outcome(OC.synthetic_special("h6_p33"), R["thresholds"], xref=R["xref"], ranks=[0, 16, 32])
    w = o["words"]
    assert (w[0, 0] == w[0, 1]).all()                                                            # the tie
    assert ((w[:, 2:5, 9] & 8) == 8).all() and np.isnan(w[0, 2:5, 1].view(F)).all()              # NaN particles: bit 8, a poisoned sum
    assert (w[0, 2:5, 2] == 0).all() and (w[0, 2:5, 8] == 0).all()                               # a NaN dp never becomes the maximum; they fail at row 0
    assert (o["cause_ever"][1] == 33).all() and o["first_fail"][1, 0] == 33                      # the all-NaN instance
    assert (o["chan_q"][1].view(U) == 0x7FC00000).all() and np.isposinf(o["chan_stat"][1, :, :, 1]).all() and np.isneginf(o["chan_stat"][1, :, :, 2]).all()
    assert np.isposinf(w[2, 5, 2].view(F)) and w[2, 5, 3] == 0                                   # +inf is the maximum from its first row on
    assert np.isposinf(o["chan_stat"][2, 2, 0, 1:]).all() and np.isnan(o["chan_stat"][2, 2, 0, 0])       # t = 3: +inf beside three NaNs — min = max = +inf, a NaN mean
    assert np.isnan(o["chan_q"][0, :, :, 2]).all() and not np.isnan(o["chan_q"][0, :, :, 1]).any()       # rank 32 of 33 with three NaNs; the median is a number


# ---- wrong reducers ----------------------------------------------------------------------------------------------------------------------
def test_every_wrong_reducer_changes_a_compared_word():
    caught = {m: 0 for m in OR.MUTANTS}
    for name in ("h6_p33", "h6_p70", "h6_p130", "h6_p300", "h7_m6_p33"):
        R, variants = _variants(name)
        for what, traj, kw in variants:
            want = OR.outcome(traj, R["thresholds"], ranks=R["ranks"], **kw)
            for m in OR.MUTANTS:
                caught[m] += OR.differs(OR.outcome(traj, R["thresholds"], ranks=R["ranks"], mutant=m, **kw), want)
    assert len(OR.MUTANTS) >= 10 and all(n > 0 for n in caught.values()), caught
    # the one that cannot show: the order with -0 and +0 tied selects the same words, because no channel is ever -0
    R, variants = _variants("h6_p70")
    for what, traj, kw in variants:
        assert OR.differs(OR.outcome(traj, R["thresholds"], ranks=R["ranks"], mutant="zeros_tied", **kw), OR.outcome(traj, R["thresholds"], ranks=R["ranks"], **kw)) == 0


def test_differs_tells_bits_from_values():
    R = OC.reference("h6_p33")
    a = {k: (None if v is None else v.copy()) for k, v in R["want"].items()}
    assert OR.differs(a, R["want"]) == 0
    a["chan_stat"][0, 0, 0, 0] = np.nextafter(a["chan_stat"][0, 0, 0, 0], F(np.inf))
    a["first_fail"][1, 2] += 1
    a["words"][2, 3, 5] ^= 1
    assert OR.differs(a, R["want"]) == 3


# ---- ABI and entry points --------------------------------------------------------------------------------------------------------------
def test_header_abi_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    fields = ("int32_t struct_size", "float r2_pos", "float cos_min", "float w2_max", "int32_t target_mode", "int32_t tgt_steps", "int32_t tgt_batch", "int32_t n_ranks",
              r"int32_t ranks\[8\]")
    assert re.search(r"typedef struct sdempc_outcome_cfg \{[^}]*" + r";[^}]*".join(fields) + r";[^}]*\}", hdr)
    assert C.sizeof(_abi.SdempcOutcomeCfg) == 4 * 16 and [f[0] for f in _abi.SdempcOutcomeCfg._fields_] == [re.sub(r"\\?\[.*", "", f.split()[-1]) for f in fields]
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and f"int {name}(" in hdr and hasattr(lib, name), name
        assert re.search(r"\nint " + name + r"\([^{]*\{\n\s*return guarded\(", src), name
    assert len(_abi.outcome_entries(lib)) == 3
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.lib_path()], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    assert set(NEW) <= exported
    assert re.search(r"dev_alloc\(h, h->d_outcome, [^;]*, true\)", src)       # filled under SDEMPC_OPT_TEST_WS_FILL like the other staging buffers
    assert _abi.OUTCOME_RANK_MAX_P == OC.RANK_MAX_P == int(re.search(r"OUTCOME_RANK_MAX_P = (\d+);", open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_kernels.h")).read()).group(1))


def _handle(max_batch=2, name="h6_p33"):
    cfg_py, model = OC.config(name)
    lib = _abi.load_library()
    cfg, keep = cfg_py.to_cfg()
    blob = model.to_blob()
    buf = C.create_string_buffer(blob, len(blob))
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(cfg), buf, len(blob), max_batch, C.byref(h)) == 0
    return lib, h, (cfg, keep, buf)


def _cfg(ranks=(0, 16, 32), thresholds=(1.0, 0.5, 4.0), target=None):
    cfg = _abi.SdempcOutcomeCfg()
    cfg.struct_size = C.sizeof(cfg)
    cfg.r2_pos, cfg.cos_min, cfg.w2_max = thresholds
    cfg.n_ranks = len(ranks)
    for k, r in enumerate(ranks[:8]):
        cfg.ranks[k] = r
    if target is not None:
        cfg.target_mode, cfg.tgt_steps, cfg.tgt_batch = target
    return cfg


def test_refusals_come_before_any_device_work_in_the_documented_order():
    """Every one of these returns its code from the host checks: none may reach the first HIP call (which, without a GPU, would answer SDEMPC_EDEVICE). A request
    wrong in two ways is refused for the EARLIER reason of the documented order: struct_size, NaN threshold, no output, ranks, particle limit, target_mode,
    tgt_steps, tgt_batch, target NULL."""
    lib, h, keep = _handle(2)
    oc, oc_keys, oc_dev = _abi.outcome_entries(lib)
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    d = np.zeros(8192, F).ctypes.data_as(fp)
    k = np.zeros(8192, U).ctypes.data_as(u32p)
    all_outs = (k, k, k, k, d, d, d, d)
    err = lambda: lib.sdempc_last_error(h).decode()
    host = lambda c, B=1, x0=d, target=None, outs=all_outs: oc(h, C.byref(c) if c is not None else None, B, x0, d, d, d, target, d, *outs)
    keyed = lambda c, B=1, keys=k, target=None, outs=all_outs: oc_keys(h, C.byref(c) if c is not None else None, B, d, d, d, keys, target, d, *outs)
    dev = lambda c, B=1, target=None, xref=1, outs=(1,) * 8: oc_dev(h, C.byref(c) if c is not None else None, B, target, xref, *outs, None)
    assert not lib.sdempc_device_ready(h)
    cfg = _cfg()
    # capacity, NULL inputs, NULL cfg
    assert host(cfg, 3) == -5 and "max_batch" in err()
    assert keyed(cfg, 3) == -5 and dev(cfg, 3) == -5
    assert host(cfg, 0) == -1
    assert host(cfg, x0=None) == -1 and "NULL" in err()
    assert keyed(cfg, keys=None) == -1 and "NULL" in err()
    for call in (host, keyed, dev):
        assert call(None) == -1 and "NULL sdempc_outcome_cfg" in err()
    # 1. struct_size — before a NaN threshold and before "no output"
    bad = _cfg(thresholds=(np.nan, 0.5, 4.0))
    bad.struct_size = 60
    for call in (host, keyed, dev):
        assert call(bad, outs=(None,) * 8) == -1 and "struct_size" in err()
    # 2. a NaN threshold, each of the three — before "no output" and before the ranks
    for i in range(3):
        t = [1.0, 0.5, 4.0]
        t[i] = np.nan
        for call in (host, keyed, dev):
            assert call(_cfg(ranks=(99,), thresholds=t), outs=(None,) * 8) == -1 and "NaN" in err(), i
    # 3. all outputs NULL (cost alone is none) — before the ranks
    for call in (host, keyed, dev):
        assert call(_cfg(ranks=(99,)), outs=(None,) * 8) == -1 and "no output" in err()
    # 4. K and the ranks, only where a *_q output is given — before the target
    for ranks in ((), (0,) * 9, (33,), (0, -1), (0, 1, 2, 3, 4, 5, 6, 33)):
        c = _cfg(ranks, target=(7, 3, 5))
        for call in (host, keyed, dev):
            assert call(c) == -1 and ("n_ranks" in err() or "rank" in err()), ranks
        no_q = (k, k, k, k, d, None, d, None)
        assert host(c, outs=no_q) == -1 and "target_mode" in err(), ranks          # without a *_q output the ranks are not looked at
    # 5. target_mode, then tgt_steps, then tgt_batch, then the rows themselves
    assert host(_cfg(target=(2, 3, 5))) == -1 and "target_mode" in err()
    assert dev(_cfg(target=(-1, 7, 1))) == -1 and "target_mode" in err()
    for steps in (0, 2, 6, 8):
        assert host(_cfg(target=(1, steps, 5)), target=None) == -1 and "tgt_steps" in err(), steps
    for call in (host, keyed):
        assert call(_cfg(target=(1, 7, 2)), B=1, target=None) == -1 and "tgt_batch" in err()
    assert dev(_cfg(target=(1, 1, 3)), B=2, target=None) == -1 and "tgt_batch" in err()
    for steps, batch, B in ((1, 1, 1), (7, 1, 2), (1, 2, 2), (7, 2, 2)):
        for call in (host, keyed, dev):
            assert call(_cfg(target=(1, steps, batch)), B=B, target=None) == -1 and "needs the caller's target rows" in err(), (steps, batch)
    assert dev(_cfg(), xref=None) == -1 and "needs xref" in err()               # the device form in xref mode without the window
    assert not lib.sdempc_device_ready(h)                      # none of the above touched the device
    lib.sdempc_destroy(h)


def test_the_particle_limit_refuses_the_order_statistics_only():
    """P = 130: chan_q / agg_q are SDEMPC_EINVAL in the host checks; without them the request passes every host check (the call then stops at the device, which is
    absent here, or succeeds)."""
    lib, h, keep = _handle(1, "h6_p130")
    oc_dev = _abi.outcome_entries(lib)[2]
    cfg = _cfg((0, 64, 129))
    for outs in ((1,) * 8, (None,) * 5 + (1, None, None), (None,) * 7 + (1,)):
        assert oc_dev(h, C.byref(cfg), 1, None, 1, *outs, None) == -1 and "128 particles" in lib.sdempc_last_error(h).decode()
    assert oc_dev(h, C.byref(_cfg((130,))), 1, None, 1, *(1,) * 8, None) == -1 and "rank" in lib.sdempc_last_error(h).decode()    # the ranks come first
    assert not lib.sdempc_device_ready(h)
    rc = oc_dev(h, C.byref(cfg), 1, None, 1, 1, 1, 1, 1, 1, None, 1, None, None)
    assert rc != -1 or "128 particles" not in lib.sdempc_last_error(h).decode()
    lib.sdempc_destroy(h)
    lib, h, keep = _handle(1, "h6_p128")
    rc = _abi.outcome_entries(lib)[2](h, C.byref(_cfg((0, 64, 127))), 1, None, 1, *(1,) * 8, None)
    assert "128 particles" not in lib.sdempc_last_error(h).decode() and "rank" not in lib.sdempc_last_error(h).decode(), rc
    # the switched-off thresholds are no refusal
    rc = _abi.outcome_entries(lib)[2](h, C.byref(_cfg((0,), thresholds=(np.inf, -np.inf, np.inf))), 1, None, 1, *(1,) * 8, None)
    assert rc != 0 and "NaN" not in lib.sdempc_last_error(h).decode()       # (no device, or no rollout held: never a launch)
    lib.sdempc_destroy(h)


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def test_python_interface_and_conveniences():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    for name in ("outcome", "outcome_keys", "outcome_dev"):
        assert callable(getattr(SV.SdeMpcSolver, name))
    assert callable(MpcProblem.m_outcome)
    assert SV.Outcome._fields == ("cost", "words") + OR.OUTPUTS[1:]
    R = OC.reference("h6_p70")
    w = R["want"]
    P, H = 70, 6
    o = SV.Outcome.of(P, R["ranks"], None, R["cost"], w["words"], w["fail_step"], w["first_fail"], w["cause_ever"], w["chan_stat"], w["chan_q"], w["agg_stat"], w["agg_q"])
    assert o.P == P and o.ranks == R["ranks"] and o._replace(words=None).P == P
    never = w["first_fail"][:, H].astype(np.float64)
    assert np.array_equal(o.p_fail, 1.0 - never / P) and o.survival.shape == (OC.B, H)
    assert np.allclose(o.survival[:, -1], never / P) and (np.diff(o.survival, axis=1) <= 0).all()
    assert np.array_equal(o.p_cause, w["cause_ever"] / P)
    k = R["ranks"].index(P // 2)
    assert np.array_equal(o.pos_err(k), np.sqrt(w["chan_q"][..., 0, k].astype(np.float64)))
    assert np.array_equal(o.tilt_deg(k), np.degrees(np.arccos(np.clip(w["chan_q"][..., 2, k].astype(np.float64), -1, 1))))
    # the second map is decreasing: the smallest cosine is the largest tilt
    lo, hi = R["ranks"].index(0), R["ranks"].index(P - 1)
    assert (o.tilt_deg(lo) >= o.tilt_deg(hi)).all() and (o.pos_err(lo) <= o.pos_err(hi)).all()
    with pytest.raises(ValueError, match="chan_q was not computed"):
        o._replace(chan_q=None).pos_err(0)
    with pytest.raises(ValueError, match="no particle count"):
        SV.Outcome(*o).p_fail
    # a Score's thresholds ARE the cfg's: one object for a campaign and a prediction
    sc = SV.Score(pos_radius=1.5, tilt_max=np.radians(45.0), rate_max=3.0)
    cfg = _cfg(thresholds=[float(t) for t in sc.thresholds()])
    assert (F(cfg.r2_pos), F(cfg.cos_min), F(cfg.w2_max)) == sc.thresholds()
    off = SV.Score().thresholds()
    assert np.isposinf(off[0]) and np.isneginf(off[1]) and np.isposinf(off[2])


# ---- no new kernel symbol ----------------------------------------------------------------------------------------------------------------
def test_the_reducer_is_a_mode_of_the_noise_kernel():
    """No new __global__ symbol: the reducer's file declares no kernel, sdempc_prng.hip still has its five, and no built kernel is named for the outcome."""
    import kernel_census as kc
    csrc = os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc")
    assert "__global__" not in open(os.path.join(csrc, "sdempc_outcome.inc.h")).read()
    prng = open(os.path.join(csrc, "sdempc_prng.hip")).read()
    assert prng.count("__global__") == 5 and prng.index('#include "sdempc_band.inc.h"') < prng.index('#include "sdempc_outcome.inc.h"')
    assert "__launch_bounds__(256, 8) sdempc_noise_kernel" in prng
    for where in (kc.CSRC, kc.AV_DIR):
        built = kc.built_kernels(where)
        if built is None and where == kc.AV_DIR and not os.path.exists(os.path.join(where, "libsdempc.so")):
            continue
        assert built is not None, f"libsdempc.so / its objects are not built in {where}, or nm is missing"
        assert ("sdempc_noise_kernel", "") in built and not [k for k in built if "outcome" in k[0].lower()]
