"""Closed loop against a separate plant (SPEC.md §11a) without a GPU: every refusal of sdempc_closed_loop_batch_plant (no HIP call may happen
before them), the ABI version, RotorSDEModel.perturbed, the CPU reference of tests/plant_loop_ref.py against closed_loop_ref, and the
bits(p, 6 n) layout of the plant noise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
from cases import CDIR, ROOT
from closed_loop_ref import closed_loop_ref
from plant_loop_ref import plant_cfg, plant_dt, plant_loop_ref
from sde4mbrl_px4_amd import _abi, load_mpc_config, prng, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver


def small_cfg(**kw):
    c1 = load_mpc_config(os.path.join(CDIR, "c1_iris_posctrl_h20_p32.yaml"))
    return c1.replace(**{"horizon": 10, "num_short_dt": 10, "num_particles": 33, "max_iter": 8, "max_no_improvement_iter": 8, **kw})


def test_abi_version_is_three_everywhere():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3
    assert _abi.ABI_VERSION == 3
    assert _abi.load_library().sdempc_abi_version() == 3
    assert int(re.search(r"#define\s+SDEMPC_PLANT_MAX_SUBSTEPS\s+(\d+)", hdr).group(1)) == _abi.PLANT_MAX_SUBSTEPS
    assert C.sizeof(_abi.SdempcPlantCfg) == 24
    assert "sdempc_closed_loop_batch_plant" in _abi.EXPORTED_SYMBOLS


class _Call:
    """ctypes buffers of one sdempc_closed_loop_batch_plant call; every field can be overridden."""

    def __init__(self, cfg, B=4, T=3):
        H, m = cfg.horizon, cfg.num_motors
        self.B, self.T = B, T
        self.x0 = np.zeros((B, 13), np.float32)
        self.xref = np.zeros((1, 1, H + 1, 13), np.float32)
        self.keys = np.zeros((B, 2), np.uint32)
        self.xs = np.zeros((B, T + 1, 13), np.float32)
        self.us = np.zeros((B, T, m), np.float32)
        self.info = np.zeros((B, T, 8), np.float32)

    def __call__(self, lib, h, blobs, sizes=None, plant_of=None, num_plants=None, substeps=1, dt=0.0, mlp_dtype=-1, math_mode=-1, struct_size=None,
                 null_cfg=False, null_blobs=False, null_sizes=False):
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        Np = len(blobs) if num_plants is None else num_plants
        pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg) if struct_size is None else struct_size, Np, substeps, dt, mlp_dtype, math_mode)
        bufs = (C.c_char_p * max(len(blobs), 1))(*blobs)
        sz = (C.c_size_t * max(len(blobs), 1))(*(sizes if sizes is not None else [len(b) for b in blobs]))
        of = None if plant_of is None else np.ascontiguousarray(plant_of, np.int32)
        return lib.sdempc_closed_loop_batch_plant(
            h, None if null_cfg else C.byref(pc), None if null_blobs else C.cast(bufs, C.POINTER(C.c_void_p)), None if null_sizes else sz,
            None if of is None else of.ctypes.data_as(C.POINTER(C.c_int32)), self.B, self.T, self.x0.ctypes.data_as(fp),
            self.xref.ctypes.data_as(fp), 1, 1, self.keys.ctypes.data_as(u32p), None, None, self.xs.ctypes.data_as(fp), self.us.ctypes.data_as(fp),
            self.info.ctypes.data_as(C.POINTER(_abi.SdempcInfo)), None, None, None)


def test_plant_argument_checks_make_no_hip_call():
    lib = _abi.load_library()
    cfg = small_cfg()
    ccfg, keep = cfg.to_cfg()
    blob = synthetic_iris().to_blob()
    bad_magic = b"\x00" + blob[1:]
    hexa = synthetic_hexa().to_blob()
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(ccfg), blob, len(blob), 4, C.byref(h)) == 0
    EINVAL, EBLOB = -1, -2
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    assert re.search(r"#define\s+SDEMPC_EINVAL\s+\(-1\)", hdr) and re.search(r"#define\s+SDEMPC_EBLOB\s+\(-2\)", hdr)
    try:
        call = _Call(cfg)
        cases = [  # (keyword arguments, expected code, a word of the message)
            (dict(blobs=[blob], struct_size=20), EINVAL, "struct_size"),
            (dict(blobs=[blob], null_cfg=True), EINVAL, "struct_size"),
            (dict(blobs=[blob], num_plants=0), EINVAL, "num_plants"),
            (dict(blobs=[blob] * 5, num_plants=5), EINVAL, "num_plants"),                 # Np > B
            (dict(blobs=[blob], substeps=0), EINVAL, "substeps"),
            (dict(blobs=[blob], substeps=_abi.PLANT_MAX_SUBSTEPS + 1), EINVAL, "substeps"),
            (dict(blobs=[blob], dt=-0.01), EINVAL, "dt"),
            (dict(blobs=[blob], dt=float("inf")), EINVAL, "dt"),
            (dict(blobs=[blob], dt=float("nan")), EINVAL, "dt"),
            (dict(blobs=[blob], mlp_dtype=3), EINVAL, "mlp_dtype"),
            (dict(blobs=[blob], mlp_dtype=-2), EINVAL, "mlp_dtype"),
            (dict(blobs=[blob], math_mode=2), EINVAL, "math_mode"),
            (dict(blobs=[blob], math_mode=-2), EINVAL, "math_mode"),
            (dict(blobs=[blob], null_blobs=True), EINVAL, "blob table"),
            (dict(blobs=[blob], null_sizes=True), EINVAL, "blob table"),
            (dict(blobs=[blob, blob]), EINVAL, "plant_of"),                               # plant_of NULL with 1 < Np < B
            (dict(blobs=[blob, blob], plant_of=[0, 1, 2, 0]), EINVAL, "index"),
            (dict(blobs=[blob, blob], plant_of=[0, -1, 1, 0]), EINVAL, "index"),
            (dict(blobs=[blob], sizes=[len(blob) - 4]), EBLOB, "too small"),
            (dict(blobs=[blob, bad_magic], plant_of=[0, 1, 0, 1]), EBLOB, "header"),
            (dict(blobs=[hexa]), EINVAL, "num_motors"),
        ]
        for kw, want, word in cases:
            rc = call(lib, h, **kw)
            msg = lib.sdempc_last_error(h).decode()
            assert rc == want, (kw.keys(), rc, msg)
            assert word in msg, (word, msg)
            assert lib.sdempc_device_ready(h) == 0
        # the checks of the plain closed loop come first and are the same
        for B, T, want in ((5, 3, -5), (4, 0, EINVAL)):
            c2 = _Call(cfg, B, max(T, 1))
            c2.T = T
            assert c2(lib, h, blobs=[blob]) == want
            assert lib.sdempc_device_ready(h) == 0
    finally:
        lib.sdempc_destroy(h)


def test_python_surface_refuses_plant_keywords_without_a_plant():
    cfg = small_cfg()
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=1)
    x0 = np.zeros((1, 13), np.float32)
    xref = np.zeros((cfg.horizon + 1, 13), np.float32)
    with pytest.raises(ValueError):
        S.closed_loop(x0, xref, np.zeros((1, 2), np.uint32), 1, plant_substeps=2)
    with pytest.raises(ValueError):
        S.closed_loop(x0, xref, np.zeros((1, 2), np.uint32), 1, plant=synthetic_iris(), plant_mlp_dtype="f64")
    assert not S.device_ready()
    S.close()


GROUPS = {"mass": ("mass",), "inertia": ("inertia",), "thrust": ("thrust_poly",), "moment": ("moment_poly",), "sigma": ("sigma",), "residual": ("W2",)}
FIELDS = ("mass", "grav", "b3n") + synthetic_iris()._ARRAY_FIELDS


def _field_bytes(model, name):
    return np.asarray(getattr(model, name), np.float32).tobytes()


def test_perturbed_is_deterministic_and_touches_only_the_named_groups():
    base = synthetic_iris()
    before = base.to_blob()
    zero = base.perturbed(np.random.default_rng(3))
    assert zero.to_blob() == before and zero is not base
    amounts = dict(mass=0.2, inertia=0.2, thrust=0.2, moment=0.1, sigma=0.3, residual=0.2)
    a = base.perturbed(np.random.default_rng(1), **amounts)
    b = base.perturbed(np.random.default_rng(1), **amounts)
    c = base.perturbed(np.random.default_rng(2), **amounts)
    assert a.to_blob() == b.to_blob() and a.to_blob() != c.to_blob() and a.to_blob() != before
    assert base.to_blob() == before                                          # the input is untouched
    assert not np.shares_memory(a.W2, base.W2) and not np.shares_memory(a.W1z, base.W1z)
    for kw, fields in GROUPS.items():
        one = base.perturbed(np.random.default_rng(1), **{kw: 0.2})
        for f in FIELDS:
            changed = _field_bytes(one, f) != _field_bytes(base, f)
            assert changed == (f in fields), (kw, f)
        # a keyword never moves another group's draw: the group's values are those of the all-groups model
        for f in fields:
            if kw not in ("moment", "sigma"):                                # (their amounts differ between the two calls)
                assert _field_bytes(one, f) == _field_bytes(a, f), (kw, f)
        lo, hi = np.float32(1 - 0.2), np.float32(1 + 0.2)
        for f in fields:
            with np.errstate(invalid="ignore"):
                ratio = np.asarray(getattr(one, f), np.float32) / np.asarray(getattr(base, f), np.float32)
            ratio = ratio[np.isfinite(ratio)]                                # (thrust_poly's constant term is zero)
            assert ((ratio >= lo - 1e-6) & (ratio <= hi + 1e-6)).all(), (kw, f)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_plant_noise_is_one_draw_of_six_n(n):
    r0 = prng.PRNGKey(77 + n)
    r1, _ = orc.split(r0, 2)
    _, p = orc.split(r1, 2)
    bits = prng.random_bits(p, 6 * n)
    assert np.array_equal(orc.random_bits(p, 6 * n), bits)
    # SPEC.md §7.1: counter i pairs with i + 3 n — element i is the first word of block (i, i + 3 n), element 3 n + i the second
    for i in range(3 * n):
        w0, w1 = orc.threefry2x32(p, i, i + 3 * n)
        assert (int(bits[i]), int(bits[3 * n + i])) == (w0, w1)
    want = np.array([orc.lib().orc_bits_to_normal(int(v)) for v in bits], np.float32)
    assert orc.normal(p, 6 * n).tobytes() == want.tobytes()


def test_plant_cfg_holds_the_float32_step_length():
    cfg = small_cfg()
    for n in (1, 2, 3, 4, 7, 64):
        d = plant_dt(cfg, n)
        assert d.dtype == np.float32 and d == np.float32(cfg.time_steps[0]) / np.float32(n)
        assert np.float32(plant_cfg(cfg, n).time_steps[0]).tobytes() == d.tobytes()
    assert np.float32(plant_cfg(cfg, 4, dt=0.0137).time_steps[0]) == np.float32(0.0137)
    pc = plant_cfg(cfg, 1, mlp_dtype="f16", math_mode="fast")
    assert (pc.mlp_dtype, pc.math_mode, cfg.mlp_dtype, cfg.math_mode) == ("f16", "fast", "f32", "exact")


def _episodes(cfg, B, seed):
    x0 = W.random_initial_states(B, seed)
    xref = np.stack([W.reference_window(0.1 * b, cfg.time_steps) for b in range(B)])[None]
    keys = np.stack([prng.PRNGKey(seed + b) for b in range(B)])
    return x0, xref, keys


@pytest.mark.parametrize("math_mode", ["exact", "fast"])
def test_reference_with_own_model_is_the_plain_closed_loop(math_mode):
    cfg = small_cfg(mlp_dtype="f32x3", math_mode=math_mode)
    model = synthetic_iris()
    B, T = 3, 5
    x0, xref, keys = _episodes(cfg, B, 20)
    want = closed_loop_ref(cfg, model, x0, xref, keys, T)
    got = plant_loop_ref(cfg, model, model, x0, xref, keys, T)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    per = plant_loop_ref(cfg, model, [model] * B, x0, xref, keys, T)
    for g, w in zip(per, want):
        assert g.tobytes() == w.tobytes()


def test_reference_with_perturbed_plants_moves_and_stays_finite():
    """The inputs of the GPU tests test something: perturbed plants leave the unperturbed trajectories, on finite numbers."""
    cfg = small_cfg(mlp_dtype="f32x3", max_iter=3, max_no_improvement_iter=3)
    model = synthetic_iris()
    B, T = 2, 3
    x0, xref, keys = _episodes(cfg, B, 20)
    rng = np.random.default_rng(1)
    plants = [model.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, residual=0.2) for _ in range(B)]
    own = closed_loop_ref(cfg, model, x0, xref, keys, T)
    for n in (1, 4):
        got = plant_loop_ref(cfg, model, plants, x0, xref, keys, T, substeps=n)
        assert np.isfinite(got[0]).all()
        assert got[0].tobytes() != own[0].tobytes()
        assert got[0][:, 0].tobytes() == x0.tobytes() and np.array_equal(got[5], own[5])       # the key schedule does not depend on the plant
    # results depend on blob[plant_of[b]] only: a permuted list with the inverse map is the same loop
    a = plant_loop_ref(cfg, model, plants, x0, xref, keys, T, substeps=4)
    b = plant_loop_ref(cfg, model, plants[::-1], x0, xref, keys, T, substeps=4, plant_of=[1, 0])
    for g, w in zip(a, b):
        assert g.tobytes() == w.tobytes()
