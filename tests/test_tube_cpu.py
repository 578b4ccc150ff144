"""The predicted tube (SPEC.md §12) without a GPU: the C ABI's new entry points and their refusals, the NumPy restatement tests/tube_ref.py against the oracle
and against its own scalar form, the wrong reducers of tube_ref.MUTANTS against the committed cases, and the properties the arithmetic must have."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tube_cases as TC
import tube_ref as TR
from sde4mbrl_px4_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdempc_tube_batch", "sdempc_tube_batch_keys", "sdempc_tube_batch_dev")
F = np.float32


# ---- ABI and entry points --------------------------------------------------------------------------------------------------------------
def test_header_abi_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_tube_cfg \{[^}]*int32_t struct_size;[^}]*float lo\[SDEMPC_NX\], hi\[SDEMPC_NX\];[^}]*\}", hdr)
    assert C.sizeof(_abi.SdempcTubeCfg) == 4 + 2 * 13 * 4
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3
    assert hasattr(lib, "sdempc_tube_batch")
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and f"int {name}(" in hdr and hasattr(lib, name), name
        assert re.search(r"\nint " + name + r"\([^{]*\{\n\s*return guarded\(", src), name
    assert "d_tube" in re.search(r"SDEMPC_OPT_TEST_WS_FILL\s+-1 none.*?SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES", hdr, re.S).group(0)
    assert re.search(r"dev_alloc\(h, h->d_tube, [^;]*, true\)", src)          # filled under SDEMPC_OPT_TEST_WS_FILL like the other staging buffers


def _handle(max_batch=2):
    cfg_py, model = TC.config("h6_p33")
    lib = _abi.load_library()
    cfg, keep = cfg_py.to_cfg()
    blob = model.to_blob()
    buf = C.create_string_buffer(blob, len(blob))
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(cfg), buf, len(blob), max_batch, C.byref(h)) == 0
    return lib, h, (cfg, keep, buf)


def test_refusals_come_before_any_device_work():
    """Every one of these returns its code from the host checks: none may reach the first HIP call (which, without a GPU, would answer SDEMPC_EDEVICE)."""
    lib, h, keep = _handle(2)
    tube, tube_keys, tube_dev = _abi.tube_entries(lib)
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    d = np.zeros(4096, F).ctypes.data_as(fp)
    k = np.zeros(16, np.uint32).ctypes.data_as(u32p)
    cfg = _abi.SdempcTubeCfg()
    cfg.struct_size = C.sizeof(cfg)
    for i in range(13):
        cfg.lo[i], cfg.hi[i] = -np.inf, np.inf
    err = lambda: lib.sdempc_last_error(h).decode()
    assert not lib.sdempc_device_ready(h)
    # capacity
    assert tube(h, C.byref(cfg), 3, d, d, d, d, d, d, d, d, d, k) == -5 and "max_batch" in err()
    assert tube_keys(h, C.byref(cfg), 3, d, d, d, k, d, d, d, d, d, k) == -5
    assert tube_dev(h, C.byref(cfg), 3, 1, 1, 1, 1, 1, None) == -5
    assert tube(h, C.byref(cfg), 0, d, d, d, d, d, d, d, d, d, k) == -1
    # NULL inputs, no plane at all
    assert tube(h, C.byref(cfg), 1, None, d, d, d, d, d, d, d, d, k) == -1 and "NULL" in err()
    assert tube_keys(h, C.byref(cfg), 1, d, d, d, None, d, d, d, d, d, k) == -1 and "NULL" in err()
    assert tube(h, C.byref(cfg), 1, d, d, d, d, d, None, None, None, None, None) == -1 and "no output plane" in err()
    assert tube_dev(h, None, 1, None, None, None, None, None, None) == -1 and "no output plane" in err()
    # outside without the bounds it counts against
    assert tube(h, None, 1, d, d, d, d, d, d, d, d, d, k) == -1 and "outside needs" in err()
    assert tube_dev(h, None, 1, None, None, None, None, 1, None) == -1 and "outside needs" in err()
    # struct_size, NaN bound
    bad = _abi.SdempcTubeCfg.from_buffer_copy(cfg)
    bad.struct_size = 12
    assert tube(h, C.byref(bad), 1, d, d, d, d, d, d, d, d, d, k) == -1 and "struct_size" in err()
    assert tube_dev(h, C.byref(bad), 1, 1, None, None, None, None, None) == -1 and "struct_size" in err()
    nanb = _abi.SdempcTubeCfg.from_buffer_copy(cfg)
    nanb.hi[4] = np.nan
    assert tube(h, C.byref(nanb), 1, d, d, d, d, d, d, d, d, d, k) == -1 and "NaN" in err()
    assert not lib.sdempc_device_ready(h)                      # none of the above touched the device
    lib.sdempc_destroy(h)


def test_python_interface_exists():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    from sde4mbrl_px4_amd.solver import SdeMpcSolver, Tube
    assert Tube._fields == ("cost", "mean", "var", "min", "max", "outside")
    for name in ("tube", "tube_keys", "tube_dev"):
        assert callable(getattr(SdeMpcSolver, name))
    assert callable(MpcProblem.m_tube)
    t = Tube.of(4, np.zeros(1, F), np.zeros((1, 2, 13), F), np.full((1, 2, 13), 4.0, F), np.zeros((1, 2, 13), F), np.zeros((1, 2, 13), F), np.full((1, 2, 13), 3, np.uint32))
    assert t.std.dtype == np.float32 and (t.std == 2.0).all() and (t.p_outside == 0.75).all() and len(t) == 6
    assert t._replace(cost=np.ones(1, F)).P == 4               # the particle count follows _replace ...
    with pytest.raises(ValueError, match="particle count"):    # ... and a Tube that never got one refuses, it does not divide by a guess
        Tube(*t).p_outside


# ---- the reference against the oracle, against itself, against the wrong reducers ------------------------------------------------------------
@pytest.mark.parametrize("name", TC.NAMES)
def test_reference_mean_is_the_oracles_mean_bit_for_bit(name):
    R = TC.reference(name)
    got = TR.tube(R["traj"], R["lo"], R["hi"])
    assert got["mean"].tobytes() == R["xmean"].tobytes()
    assert np.isfinite(R["traj"]).all()


@pytest.mark.parametrize("name", TC.NAMES)
def test_vectorised_and_scalar_restatements_agree(name):
    R = TC.reference(name)
    a, b = TR.tube(R["traj"], R["lo"], R["hi"]), TR.tube_scalar(R["traj"], R["lo"], R["hi"])
    for k in TR.PLANES:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", TC.NAMES)
def test_cases_can_tell(name):
    """In the oracle's own tensor: at least a third of the bounded columns (t >= 1) have 0 < outside < P (P = 1 cannot: there, both counts occur), and the variance
    is positive in every velocity and body-rate column at t >= 1."""
    R = TC.reference(name)
    P = R["cfg"].num_particles
    got = TR.tube(R["traj"], R["lo"], R["hi"])
    out = got["outside"][:, 1:, list(TC.BOUNDED)]
    if P > 1:
        frac = ((out > 0) & (out < P)).mean()
        assert frac >= 1.0 / 3.0, frac
        assert (got["var"][:, 1:, [3, 4, 5, 10, 11, 12]] > 0).all()
    else:
        assert (out == 0).any() and (out == 1).any()
    assert (got["outside"][:, :, 6:10] == 0).all()             # unbounded components: only a NaN would count
    x0 = R["x0"]
    assert len({x0[b].tobytes() for b in range(TC.B)}) == TC.B


def _mutant_inputs():
    """the committed cases, and one of them with a non-finite instance (NaNs in the tensor: what `nan_not_counted` needs)"""
    for name in TC.NAMES:
        R = TC.reference(name)
        yield name, R["traj"], R["lo"], R["hi"]
    R = TC.reference("h6_p33")
    x0, u, xref, noise = TC.nonfinite_variant("h6_p33")
    _, traj, _ = TC.oracle_rollout(R["cfg"], R["model"], x0, u, xref, noise)
    assert np.isnan(traj[1]).any() and np.isfinite(traj[0]).all() and np.isfinite(traj[2]).all()
    yield "h6_p33_nonfinite", traj, R["lo"], R["hi"]


def test_every_mutant_changes_a_compared_word():
    assert len(TR.MUTANTS) >= 8
    caught = {m: [] for m in TR.MUTANTS}
    for name, traj, lo, hi in _mutant_inputs():
        right = TR.tube(traj, lo, hi)
        for m in TR.MUTANTS:
            if TR.planes_differ(right, TR.tube(traj, lo, hi, mutant=m)):
                caught[m].append(name)
    print({m: len(v) for m, v in caught.items()})
    assert all(caught.values()), [m for m, v in caught.items() if not v]
    assert "h6_p130" in caught["slots_sequential"]            # five groups: the only case where the slot order shows
    assert caught["padded_lanes_included"] and "h6_p32" not in caught["padded_lanes_included"]       # no padded lane at P = 32


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_single_particle_has_no_spread():
    R = TC.reference("h6_p1")
    got = TR.tube(R["traj"], R["lo"], R["hi"])
    v = R["traj"][:, 0]
    assert (got["var"] == 0).all() and not np.signbit(got["var"]).any()
    assert (got["min"] == v).all() and (got["max"] == v).all() and (got["mean"] == v).all()


@pytest.mark.parametrize("name", ("h6_p33", "h6_p130"))
def test_scaling_by_two_is_exact(name):
    R = TC.reference(name)
    a = TR.tube(R["traj"])
    b = TR.tube(R["traj"] * F(2.0))
    for k, s in (("mean", 2.0), ("min", 2.0), ("max", 2.0), ("var", 4.0)):
        assert (a[k] * F(s)).tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", TC.NAMES)
def test_variance_against_float64(name):
    """var against np.var (float64) of the same float32 tensor, within the bound of the §6.1 tree.

    u = 2^-24, gamma(k) = k u / (1 - k u). A §6.1 sum passes every addend through at most D = 5 (butterfly) + ceil(G / 4) (its slot) + 3 (the slot total) additions, so
    the computed sum is sum_p v_p (1 + theta_p) with |theta_p| <= gamma(D). The factor 1/P is a rounded reciprocal and a rounded product: two more. Hence the rounded
    mean m has |m - mu| <= e_m = gamma(D + 2) * A with A = mean |v_p|. Every term of the second sum is non-negative: d_p = fl(v_p - m) and q_p = fl(d_p d_p) carry
    three roundings, the sum D, the factor two, so var = V (1 + theta), |theta| <= gamma(D + 5), where V = mean (v_p - m)^2 = sigma^2 + (m - mu)^2 exactly. So
        |var - sigma^2| <= gamma(D + 5) (sigma^2 + e_m^2) + e_m^2.
    (No value here is near the underflow threshold; the float64 reference's own error, ~1e-16 relative, is below one unit of the bound's last digit.)"""
    R = TC.reference(name)
    P = R["cfg"].num_particles
    G = (P + 31) // 32
    D = 5 + (G + 3) // 4 + 3
    u = 2.0 ** -24
    gamma = lambda k: k * u / (1.0 - k * u)
    v = R["traj"].astype(np.float64)
    sig2 = v.var(axis=1)
    A = np.abs(v).mean(axis=1)
    e_m = gamma(D + 2) * A
    bound = gamma(D + 5) * (sig2 + e_m ** 2) + e_m ** 2
    got = TR.tube(R["traj"])["var"].astype(np.float64)
    err = np.abs(got - sig2)
    print(name, "max err / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (got >= 0).all()


# ---- no new kernel symbol ----------------------------------------------------------------------------------------------------------------
def test_the_reducer_is_a_mode_of_the_noise_kernel():
    """No new __global__ symbol: the built kernels are those of the census table (tests/test_kernel_census_cpu.py holds both directions), the reducer's file
    declares no kernel, and the noise kernel is still one census entry."""
    import kernel_census as kc
    csrc = os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc")
    assert "__global__" not in open(os.path.join(csrc, "sdempc_tube.inc.h")).read()
    prng = open(os.path.join(csrc, "sdempc_prng.hip")).read()
    assert prng.count("__global__") == 5 and '#include "sdempc_tube.inc.h"' in prng
    assert ("sdempc_noise_kernel", "") in kc.ELSEWHERE
    for where in (kc.CSRC, kc.AV_DIR):
        built = kc.built_kernels(where)
        if built is None and where == kc.AV_DIR and not os.path.exists(os.path.join(where, "libsdempc.so")):
            continue                                           # the optional all-variants build is absent: the default build has been checked
        assert built is not None, f"libsdempc.so / its objects are not built in {where}, or nm is missing"
        assert ("sdempc_noise_kernel", "") in built and not [k for k in built if "tube" in k[0].lower()]
