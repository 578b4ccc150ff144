"""The geometric baseline controller without a GPU (SPEC.md §11l): the float32 reference (tests/geo_ref.py) against its census, its ten mutants and its float64
restatement on the cases of tests/geo_cases.py; hover; a converging CPU closed loop on the oracle plant; GeometricController.from_yaml / for_model; every refusal
of the C ABI before a HIP call; the symbols and the header version.

Measured on the cases below (deterministic, CPU, 2724 commands, the guard states left out): the largest deviation of the float32 restatement from the float64 one is
MEASURED_DC = 6.952e-8 in the thrust command (about one ulp of a command near 0.6) and MEASURED_DW = 3.727e-6 rad/s in a body-rate command (inv_tau, up to 14 / s,
multiplies the difference of two dot products of unit vectors, each good to a few ulps of 1). The test asserts twice those values; the margin only absorbs
later edits of the cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geo_cases as G
from cases import ROOT, asymmetric_model
from geo_loop_ref import geo_loop_ref
from geo_ref import MUTANTS, PAR_NAMES, geo_command, geo_command64, geo_commands, par_row
from rate_loop_ref import rate_loop_ref
from score_loop_ref import score_rows
from sde4mbrl_px4_amd import _abi, prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SCORE_DTYPE, GeometricController, RateLoop, Score

F = np.float32
MEASURED_DC = 6.952e-8
MEASURED_DW = 3.727e-6
YAML = os.path.join(ROOT, "tests", "golden", "reference_geoctrl_yaml", "iris_geoctrl.yaml")


def command_cases():
    """(m, cfg, x, xref, par, accel_ff, ref_row, inv_dt): the stand-alone cases (B = 257, one set and per-episode sets) and the loops' episodes (B = 5), with and
    without feed-forward, for every motor count."""
    for m in G.MOTORS:
        cfg, model = G.geo_cfg(m), asymmetric_model(m)
        for B, per_episode in ((G.B257, False), (G.B257, True), (G.B5, False)):
            for ff, row in ((False, 0), (True, 2)):
                ctl = G.controller(model, B if per_episode else None, ff, row)
                par, inv_dt = G.params(ctl, cfg, B)
                x, xref = G.states(cfg, model, ctl, B)
                yield m, cfg, x, xref, par, ff, row, inv_dt


CASES = list(command_cases())
WANT = [geo_commands(x, xref, par, ff, row, inv_dt) for _, _, x, xref, par, ff, row, inv_dt in CASES]          # computed once, shared, never changed


def test_census_shows_every_branch():
    """The acceleration clip active and inactive, the thrust clamp at c_lo, at c_hi and inside, the guard taken, feed-forward on and off — and every state finite."""
    census = {}
    for (_, _, x, xref, par, ff, row, inv_dt), want in zip(CASES, WANT):
        assert np.isfinite(x).all() and np.isfinite(xref).all()
        got = geo_commands(x, xref, par, ff, row, inv_dt, census=census)
        assert got.tobytes() == want.tobytes() and np.isfinite(got).all()
    for k in ("clip", "no_clip", "lo", "hi", "inside", "guard", "ff", "no_ff"):
        assert census.get(k, 0) > 0, (k, census)
    # each motor count on its own shows the clamp at both ends (the cases of the GPU test are per motor count)
    for m in G.MOTORS:
        cm = {}
        for (mm, _, x, xref, par, ff, row, inv_dt) in CASES:
            if mm == m:
                geo_commands(x, xref, par, ff, row, inv_dt, census=cm)
        assert all(cm.get(k, 0) > 0 for k in ("clip", "no_clip", "lo", "hi", "inside", "guard")), (m, cm)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_changes_a_compared_bit(mutant):
    differs = 0
    for (_, _, x, xref, par, ff, row, inv_dt), want in zip(CASES, WANT):
        got = geo_commands(x, xref, par, ff, row, inv_dt, mutant=mutant)
        differs += int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert differs > 0


def test_float32_restatement_stays_near_the_float64_one():
    dc = dw = 0.0
    n = 0
    for (_, cfg, x, xref, par, ff, row, inv_dt), want in zip(CASES, WANT):
        for b in range(x.shape[0]):
            if b % 8 == 4:                 # the guard case: float64 algebra has no value there
                continue
            c64, w64 = geo_command64(x[b], xref[b], par_row(par, b), ff, row, float(F(cfg.time_steps[row])))
            dc = max(dc, abs(float(want[b, 0]) - c64))
            dw = max(dw, float(np.abs(want[b, 1:].astype(np.float64) - w64).max()))
            n += 1
    print(f"float32 against float64 over {n} commands: |dc| <= {dc:.3e}, |dw| <= {dw:.3e} rad/s")
    assert n > 1000 and dc <= 2 * MEASURED_DC and dw <= 2 * MEASURED_DW


def test_hover_on_target_is_exact():
    """On the target, level and at rest: omega* = 0 and c = clamp(fma(kT, g, k0)) exactly, whatever the heading of the reference."""
    from geo_ref import clamp, fma
    for m in G.MOTORS:
        cfg, model = G.geo_cfg(m), asymmetric_model(m)
        ctl = G.controller(model)
        par, inv_dt = G.params(ctl, cfg, 1)
        p = par_row(par, 0)
        x = np.zeros(13, F); x[0:3] = [0.5, -1.25, 2.0]; x[6] = 1.0
        xref = np.tile(x, (cfg.horizon + 1, 1))
        c, w = geo_command(x, xref, p)
        assert w.tobytes() == np.zeros(3, F).tobytes()
        assert c == clamp(fma(p["kT"], p["g"], p["k0"]), p["c_lo"], p["c_hi"]) and p["c_lo"] < c < p["c_hi"]
        u_h = GeometricController.hover_calibration(model)[0]
        assert abs(float(c) - u_h) < 2e-6                    # the calibrated thrust map returns the hover command


CONV = dict(kp=[4.0, 4.0, 6.0], kv=[2.5, 2.5, 3.25], max_acc=7.0, attctrl_tau=0.2)
CONV_RATE = dict(kp=[0.08, 0.08, 0.16], ki=0.1, integ_limit=0.02)


def _fly(mutant=None, f64=False, T=100):
    from scenario_cases import small_cfg
    cfg = small_cfg(horizon=6, num_short_dt=6, num_particles=1)
    model = synthetic_iris()
    ctl = GeometricController.for_model(model, **CONV)
    lo, hi = np.asarray(cfg.input_bound, F).T
    _, par = ctl.arrays(1, lo, hi)
    x0 = W.HOVER.copy()[None].astype(F)
    x0[0, 0] += 0.5
    xref = W.constant_reference(W.HOVER, cfg.horizon)[None, None]
    out = geo_loop_ref(rate_loop_ref, par, cfg, model, x0, mutant=mutant, f64=f64, plants=None, xref=xref, keys=np.array([prng.PRNGKey(5)]), T=T,
                       rate_loop=RateLoop(**CONV_RATE), S=1, D=0, alpha=0.35, substeps=4)
    xs, us, info = out[0], out[1], out[2]
    score = Score(pos_radius=1.0, tilt_max=np.deg2rad(35.0), rate_max=6.0)
    z = score_rows(xs, us, info, None, W.HOVER[None, None].astype(F), cfg, score.thresholds(), False, 1)
    z = np.ascontiguousarray(z).view(SCORE_DTYPE).reshape(-1)
    err = np.linalg.norm(xs[0, :, 0:3].astype(np.float64) - W.HOVER[0:3], axis=1)
    return err, z


def test_cpu_closed_loop_converges_and_the_wrong_signs_do_not():
    """0.5 m off the target on the oracle plant (its own noise included), 100 ticks of 0.05 s with four substeps: the float64 restatement and the float32 one both end
    under half the initial error with no Score failure; the controller with the velocity error's sign wrong, or gravity subtracted, does not."""
    for f64 in (True, False):
        err, z = _fly(f64=f64)
        assert err[0] == pytest.approx(0.5) and err[-1] < 0.5 * err[0], (f64, err[-1])
        assert z["first_fail_row"][0] == 0xFFFFFFFF and z["causes"][0] == 0, (f64, z)
    for mutant in ("velocity_sign", "gravity_subtracted"):
        err, z = _fly(mutant=mutant)
        assert not (err[-1] < 0.5 * err[0]) or z["first_fail_row"][0] != 0xFFFFFFFF, mutant


def test_from_yaml_reads_the_reference_settings(tmp_path):
    c = GeometricController.from_yaml(YAML)
    assert c.kp.tolist() == [[8.0, 8.0, 10.0]] and np.allclose(c.kv, [[1.5, 1.5, 3.3]]) and c.max_acc.tolist() == [7.0] and c.gravity.tolist() == [F(9.81)]
    assert c.attctrl_tau.tolist() == [F(0.1)] and c.inv_tau[0] == F(1) / F(0.1) and c.thrust_const.tolist() == [F(0.05)] and c.thrust_offset.tolist() == [F(0.22)]
    assert c.batch == 1 and not c.accel_ff and c.ref_row == 0
    txt = open(YAML).read()
    for bad in ("ctrl_mode: 1", "drag_dx: 0.1", "feedthrough_enable: true"):
        key = bad.split(":")[0]
        f = tmp_path / (key + ".yaml")
        f.write_text(re.sub(rf"^{key}:[^#\n]*", bad + " ", txt, flags=re.M))
        with pytest.raises(NotImplementedError):
            GeometricController.from_yaml(str(f))
    assert GeometricController.from_yaml(YAML, accel_ff=True, ref_row=1).accel_ff


def test_for_model_against_a_float64_hover_solve():
    for m in G.MOTORS:
        model = asymmetric_model(m)
        u_h, kT, k0 = GeometricController.hover_calibration(model)
        ct2, ct1, ct0 = (float(v) for v in model.thrust_poly)
        # bisection on the thrust balance, independent of the closed form
        lo, hi = 0.0, 2.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if m * (ct2 * mid * mid + ct1 * mid + ct0) < model.mass * model.grav else (lo, mid)
        assert abs(u_h - lo) < 1e-12
        # d(acceleration along the body axis) / du at hover is 1 / kT
        h = 1e-6
        acc = lambda u: m * (ct2 * u * u + ct1 * u + ct0) / model.mass      # noqa: E731
        assert abs((acc(u_h + h) - acc(u_h - h)) / (2 * h) - 1.0 / kT) < 1e-6 / kT
        c = GeometricController.for_model(model, **G.GAINS)
        assert c.thrust_const[0] == F(kT) and c.thrust_offset[0] == F(k0) and c.gravity[0] == F(model.grav)
    with pytest.raises(ValueError):
        GeometricController(kp=[1, 2], kv=1, max_acc=1, attctrl_tau=1, gravity=9.8, thrust_const=0.1, thrust_offset=0.1)
    with pytest.raises(ValueError):
        GeometricController(kp=-1.0, kv=1, max_acc=1, attctrl_tau=1, gravity=9.8, thrust_const=0.1, thrust_offset=0.1)
    with pytest.raises(ValueError):
        GeometricController(kp=np.ones((3, 3)), kv=np.ones((4, 3)), max_acc=1, attctrl_tau=1, gravity=9.8, thrust_const=0.1, thrust_offset=0.1)


def test_symbols_struct_and_header_version():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define SDEMPC_ABI_VERSION (\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION
    body = re.search(r"typedef struct sdempc_geo_cfg \{(.*?)\} sdempc_geo_cfg;", hdr, re.S).group(1)
    fields = [re.sub(r"/\*.*?\*/", "", ln).strip().rstrip(";").split()[-1].lstrip("*") for ln in body.strip().splitlines()]
    Gc = _abi.SdempcGeoCfg
    assert [f[0] for f in Gc._fields_] == fields == ["struct_size", "batch"] + list(PAR_NAMES) + ["accel_ff", "ref_row", "inv_dt"]
    assert C.sizeof(Gc) == 8 + 9 * 8 + 16 and Gc.kp.offset == 8 and Gc.accel_ff.offset == 80 and Gc.inv_dt.offset == 88
    names = lambda p: [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", p, flags=re.S).split(",")]      # noqa: E731
    new = re.search(r"int sdempc_closed_loop_batch_baseline\((.*?)\);", hdr, re.S).group(1)
    old = re.search(r"int sdempc_closed_loop_batch_events\((.*?)\);", hdr, re.S).group(1)
    assert names(new) == ["h", "geo"] + names(old)[1:]
    lib = _abi.load_library()
    for s in ("sdempc_closed_loop_batch_baseline", "sdempc_geo_command_batch"):
        assert hasattr(lib, s) and s in _abi.EXPORTED_SYMBOLS
    fn, ea = _abi.baseline_entry(lib), _abi.events_entry(lib).argtypes
    assert list(fn.argtypes[2:]) == list(ea[1:]) and fn.argtypes[1]._type_ is Gc and fn.restype is C.c_int
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    for s in ("sdempc_closed_loop_batch_baseline", "sdempc_geo_command_batch"):
        assert re.search(r"\nint " + s + r"\([^{]*\{\n\s*return guarded\(", src)


def _geo(B=4, H=6, size=None, batch=None, null=None, accel_ff=0, ref_row=0, inv_dt=0.0, **over):
    """(cfg struct, arrays kept alive): valid parameter sets for the synthetic Iris with input bounds [1e-4, 1]; `over` replaces arrays, `null` names one passed NULL."""
    rows = B if batch is None else batch
    n = max(rows, 1)
    arr = dict(kp=np.full((n, 3), 4.0, F), kv=np.full((n, 3), 2.0, F), amax=np.full(n, 7.0, F), inv_tau=np.full(n, 5.0, F), g=np.full(n, 9.81, F),
               kT=np.full(n, 0.04, F), k0=np.full(n, 0.3, F), c_lo=np.full(n, 0.1, F), c_hi=np.full(n, 0.9, F))
    for k, v in over.items():
        arr[k] = np.ascontiguousarray(v, F)
    fp = C.POINTER(C.c_float)
    g = _abi.SdempcGeoCfg(C.sizeof(_abi.SdempcGeoCfg) if size is None else size, rows, *[None if k == null else arr[k].ctypes.data_as(fp) for k in PAR_NAMES],
                          accel_ff, ref_row, inv_dt)
    return g, arr


def _loop(lib, h, blob, g, B=4, T=4, H=6, m=4, rate=True, weight=0.0, fsize=None):
    """One sdempc_closed_loop_batch_baseline call on small neutral inputs."""
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    Bb, Tb = max(B, 1), max(T, 1)
    x0 = np.zeros((Bb, 13), F); x0[:, 6] = 1.0
    xref = np.zeros((1, 1, H + 1, 13), F); xref[..., 6] = 1.0
    k0 = np.zeros((Bb, 2), np.uint32)
    xs, us, info, ws = np.zeros((Bb, Tb + 1, 13), F), np.zeros((Bb, Tb, m), F), np.zeros((Bb, Tb, 8), F), np.zeros((Bb, Tb, 4), F)
    rc = _abi.SdempcRateCfg()
    rc.struct_size = C.sizeof(_abi.SdempcRateCfg)
    rc.motor_weight = weight
    fpc = None
    if fsize is not None:
        fpc = _abi.SdempcFaultProcessCfg(fsize, 1, 1, None, None, None, None, None, 0)
    tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), 1, 0, 0.0)
    pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), 1, 1, 0.0, -1, -1)
    bufs = (C.c_char_p * 1)(blob)
    sz = (C.c_size_t * 1)(len(blob))
    return _abi.baseline_entry(lib)(
        h, None if g is None else C.byref(g), None if fpc is None else C.byref(fpc), None, None, None, None, None, None, None, None, None, None, None, None,
        C.byref(rc) if rate else None, None, C.byref(tc), C.byref(pc), C.cast(bufs, C.POINTER(C.c_void_p)), sz, None, B, T, x0.ctypes.data_as(fp),
        xref.ctypes.data_as(fp), 1, 1, k0.ctypes.data_as(u32p), None, None, None, xs.ctypes.data_as(fp), us.ctypes.data_as(fp),
        C.cast(info.ctypes.data_as(fp), C.POINTER(_abi.SdempcInfo)), None, None, None, None, None, None, ws.ctypes.data_as(fp) if rate else None, None, None,
        None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None)


def test_refusals_come_before_any_hip_call():
    """Every refusal of SPEC.md §11l through the C ABI, with SDEMPC_EINVAL and its message; a complete call gets past them (and fails on the missing device, or
    runs where there is one)."""
    lib = _abi.load_library()
    from scenario_cases import small_cfg
    cfg = small_cfg(horizon=6, num_short_dt=6, num_particles=1)
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL = -1
    nan, inf = float("nan"), float("inf")
    B = 4
    want_inv_dt = float(F(1) / F(cfg.time_steps[0]))

    def bad(k, v, row=B - 1, col=None):
        a = {"kp": np.full((B, 3), 4.0, F), "kv": np.full((B, 3), 2.0, F)}.get(k, None)
        if a is None:
            a = _geo(B)[1][k].copy()
        if col is None:
            a[row] = v
        else:
            a[row, col] = v
        return {k: a}
    cases = [(dict(cfg=None), "cfg NULL"), (dict(size=80), "struct_size"), (dict(batch=0), "batch must be 1 or B"), (dict(batch=2), "batch must be 1 or B"),
             (dict(accel_ff=2), "accel_ff"), (dict(ref_row=-1), "ref_row"), (dict(ref_row=6), "ref_row"), (dict(inv_dt=19.0), "inv_dt"), (dict(inv_dt=nan), "inv_dt"),
             (bad("kp", -1.0, col=2), "kp / kv"), (bad("kv", nan, col=0), "kp / kv"), (bad("kp", inf, col=1), "kp / kv"), (bad("amax", -0.5), "amax, inv_tau or g"),
             (bad("inv_tau", inf), "amax, inv_tau or g"), (bad("g", nan), "amax, inv_tau or g"), (bad("kT", nan), "kT or k0"), (bad("k0", -inf), "kT or k0"),
             (bad("c_lo", 0.95), "c_lo must not exceed c_hi"), (bad("c_lo", 0.0), "input_bound"), (bad("c_hi", 1.5), "input_bound"), (bad("c_hi", nan), "c_hi")]
    cases += [(dict(null=k), "parameter array is NULL") for k in PAR_NAMES]
    for kw, msg in cases:
        g, keep_ = (None, None) if "cfg" in kw else _geo(B, **kw)
        assert _loop(lib, h, blob, g, B) == EINVAL, (kw, msg)
        assert msg in lib.sdempc_last_error(h).decode(), (msg, lib.sdempc_last_error(h).decode())
    ok, keep_ = _geo(B)
    assert _loop(lib, h, blob, ok, B, rate=False) == EINVAL and "needs a rate cfg" in lib.sdempc_last_error(h).decode()
    assert _loop(lib, h, blob, ok, B, weight=0.25) == EINVAL and "motor_weight must be 0" in lib.sdempc_last_error(h).decode()
    assert _loop(lib, h, blob, ok, B, fsize=8) == EINVAL and "fault_proc struct_size" in lib.sdempc_last_error(h).decode()      # what the events route refuses
    assert _loop(lib, h, blob, ok, B, T=0) == EINVAL and "T must be >= 1" in lib.sdempc_last_error(h).decode()
    assert _loop(lib, h, blob, ok, 5) == EINVAL                                                                                   # batch 4 is neither 1 nor B = 5
    g1, keep1 = _geo(B, inv_dt=want_inv_dt, batch=1)
    assert _loop(lib, h, blob, g1, B) != EINVAL                                                                                  # the stated inv_dt and one shared set pass
    # the stand-alone entry point checks the same cfg
    fp = C.POINTER(C.c_float)
    x, xr, out = np.zeros((B, 13), F), np.zeros((1, 7, 13), F), np.zeros((B, 4), F)
    cmd = _abi.geo_command_entry(lib)
    gb, keepb = _geo(B, **bad("amax", nan))
    assert cmd(h, C.byref(gb), B, x.ctypes.data_as(fp), xr.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) == EINVAL
    assert cmd(h, C.byref(ok), B, x.ctypes.data_as(fp), xr.ctypes.data_as(fp), 2, out.ctypes.data_as(fp)) == EINVAL and "Bx" in lib.sdempc_last_error(h).decode()
    assert cmd(h, C.byref(ok), B, None, xr.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) == EINVAL
    assert cmd(h, C.byref(ok), B, x.ctypes.data_as(fp), xr.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) != EINVAL
    lib.sdempc_destroy(h)


def test_python_surface_refuses_a_controller_without_a_rate_loop():
    from sde4mbrl_px4_amd.solver import SdeMpcSolver
    cfg, model = G.geo_cfg(4), asymmetric_model(4)
    ctl = G.controller(model)
    x0, xref, keys = G.episodes(cfg, model, ctl)
    S = SdeMpcSolver(cfg, model, max_batch=G.B5)
    with pytest.raises(ValueError, match="rate_loop"):
        S.closed_loop(x0, xref, keys, G.T6, controller=ctl)
    with pytest.raises(ValueError, match="motor_weight"):
        S.closed_loop(x0, xref, keys, G.T6, controller=ctl, rate_loop=G.rate_loop(motor_weight=0.5))
    with pytest.raises(ValueError, match="GeometricController"):
        S.closed_loop(x0, xref, keys, G.T6, controller="geo", rate_loop=G.rate_loop())
    with pytest.raises(ValueError, match="ref_row"):
        S.geo_command(x0, xref[0], G.controller(model, ref_row=6))
    with pytest.raises(ValueError, match="B = 3"):
        S.geo_command(x0, xref[0], G.controller(model, 3))
    S.close()
