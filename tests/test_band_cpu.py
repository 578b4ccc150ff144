"""Predicted bands (SPEC.md §12b) without a GPU: the C ABI's new entry points and their refusals, the NumPy restatement tests/band_ref.py against its own
definition form, the identities §12b states, the wrong reducers of band_ref.MUTANTS against the cases of tests/band_cases.py, the conditions those cases must
meet, the quantile -> rank mapping, and the host helpers Bands.pit / inside and solver.calibration."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import band_cases as BC
import band_ref as BR
import tube_ref as TR
from sde4mbrl_px4_amd import _abi
from sde4mbrl_px4_amd import solver as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdempc_bands_batch", "sdempc_bands_batch_keys", "sdempc_bands_batch_dev")
F = np.float32
SMALL = tuple(n for n in BC.NAMES if BC.shape(n)[2] <= 130)


# ---- ABI and entry points --------------------------------------------------------------------------------------------------------------
def test_header_abi_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "sdempc.h")).read()
    src = open(os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc", "sdempc_api.cpp")).read()
    assert int(re.search(r"#define\s+SDEMPC_ABI_VERSION\s+(\d+)", hdr).group(1)) == 3 == _abi.ABI_VERSION      # no version change
    assert re.search(r"typedef struct sdempc_bands_cfg \{[^}]*int32_t struct_size;[^}]*int32_t n_ranks;[^}]*int32_t ranks\[8\];[^}]*\}", hdr)
    assert C.sizeof(_abi.SdempcBandsCfg) == 4 * 10
    lib = _abi.load_library()
    assert lib.sdempc_abi_version() == 3
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and f"int {name}(" in hdr and hasattr(lib, name), name
        assert re.search(r"\nint " + name + r"\([^{]*\{\n\s*return guarded\(", src), name
    assert len(_abi.bands_entries(lib)) == 3
    # the dynamic symbol table of the built library
    nm = subprocess.run(["nm", "-D", "--defined-only", _abi.lib_path()], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    assert set(NEW) <= exported
    assert re.search(r"dev_alloc\(h, h->d_band, [^;]*, true\)", src)          # filled under SDEMPC_OPT_TEST_WS_FILL like the other staging buffers


def _handle(max_batch=2, name="h6_p33"):
    cfg_py, model = BC.config(name)
    lib = _abi.load_library()
    cfg, keep = cfg_py.to_cfg()
    blob = model.to_blob()
    buf = C.create_string_buffer(blob, len(blob))
    h = C.c_void_p()
    assert lib.sdempc_create(C.byref(cfg), buf, len(blob), max_batch, C.byref(h)) == 0
    return lib, h, (cfg, keep, buf)


def _cfg(ranks=(0, 16, 32)):
    cfg = _abi.SdempcBandsCfg()
    cfg.struct_size = C.sizeof(cfg)
    cfg.n_ranks = len(ranks)
    for k, r in enumerate(ranks[:8]):
        cfg.ranks[k] = r
    return cfg


def test_refusals_come_before_any_device_work():
    """Every one of these returns its code from the host checks: none may reach the first HIP call (which, without a GPU, would answer SDEMPC_EDEVICE)."""
    lib, h, keep = _handle(2)
    bands, bands_keys, bands_dev = _abi.bands_entries(lib)
    fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    d = np.zeros(4096, F).ctypes.data_as(fp)
    k = np.zeros(4096, np.uint32).ctypes.data_as(u32p)
    cfg = _cfg()
    err = lambda: lib.sdempc_last_error(h).decode()
    ref = lambda c: C.byref(c) if c is not None else None
    host = lambda c, B=1, x0=d, obs=d, outs=(d, d, k, k): bands(h, ref(c), B, x0, d, d, d, obs, *outs)
    assert not lib.sdempc_device_ready(h)
    # capacity
    assert host(cfg, 3) == -5 and "max_batch" in err()
    assert bands_keys(h, ref(cfg), 3, d, d, d, k, d, d, d, k, k) == -5
    assert bands_dev(h, ref(cfg), 3, 1, 1, 1, 1, None) == -5
    assert host(cfg, 0) == -1
    # NULL inputs, no output at all (cost alone is none)
    assert host(cfg, x0=None) == -1 and "NULL" in err()
    assert bands_keys(h, ref(cfg), 1, d, d, d, None, d, d, d, k, k) == -1 and "NULL" in err()
    assert host(cfg, outs=(None,) * 4) == -1 and "no output" in err()
    assert host(cfg, outs=(d, None, None, None)) == -1 and "no output" in err()
    assert bands_dev(h, ref(cfg), 1, 1, None, None, None, None) == -1 and "no output" in err()
    # below / at without the observed rows; q without a cfg
    for outs in ((None, None, k, None), (None, None, None, k), (None, d, k, k)):
        assert host(cfg, obs=None, outs=outs) == -1 and "need the observed rows" in err(), outs
    assert bands_dev(h, ref(cfg), 1, None, None, 1, None, None) == -1 and "need the observed rows" in err()
    assert host(None) == -1 and "needs a sdempc_bands_cfg" in err()
    assert bands_dev(h, None, 1, None, 1, None, None, None) == -1 and "needs a sdempc_bands_cfg" in err()
    # struct_size
    bad = _cfg()
    bad.struct_size = 12
    assert host(bad) == -1 and "struct_size" in err()
    assert bands_dev(h, ref(bad), 1, 1, None, 1, 1, None) == -1 and "struct_size" in err()       # even where q is not asked for
    # ranks
    for ranks in ((), (0,) * 9, (33,), (0, -1), (0, 1, 2, 3, 4, 5, 6, 33)):
        c = _cfg(ranks)
        assert host(c) == -1 and ("n_ranks" in err() or "rank" in err()), ranks
        assert bands_keys(h, ref(c), 1, d, d, d, k, d, d, d, k, k) == -1, ranks
        assert bands_dev(h, ref(c), 1, None, 1, None, None, None) == -1, ranks
    assert not lib.sdempc_device_ready(h)                      # none of the above touched the device
    lib.sdempc_destroy(h)


def test_no_particle_limit_in_the_host_checks():
    """P = 1024 (C5's particle count): a rank up to P - 1 passes the host checks (the call then fails at the device, which is absent here, or succeeds)."""
    lib, h, keep = _handle(1, "h6_p1024")
    bands_dev = _abi.bands_entries(lib)[2]
    assert bands_dev(h, C.byref(_cfg((1024,))), 1, None, 1, None, None, None) == -1 and "rank" in lib.sdempc_last_error(h).decode()
    assert not lib.sdempc_device_ready(h)
    lib.sdempc_destroy(h)


def test_python_interface_exists():
    from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
    for name in ("bands", "bands_keys", "bands_dev"):
        assert callable(getattr(SV.SdeMpcSolver, name))
    assert callable(MpcProblem.m_bands) and callable(SV.calibration) and SV.Bands._fields == ("cost", "q", "below", "at")
    v = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, np.nan], F)
    assert np.array_equal(SV.band_keys(v), BR.keys(v)) and (np.diff(BR.keys(v).astype(np.int64)) > 0).all()
    assert BR.words(BR.keys(v))[:-1].tobytes() == v[:-1].tobytes() and BR.words(BR.keys(v)).view(np.uint32)[-1] == 0x7FC00000
    assert [BR.key_scalar(x) for x in v] == [int(x) for x in BR.keys(v)]
    odd_nans = np.array([0x7F800001, 0xFFC00000, 0x7FFFFFFF, 0xFF800001], np.uint32).view(F)
    assert (BR.keys(odd_nans) == 0xFFFFFFFF).all()


# ---- quantile -> rank ------------------------------------------------------------------------------------------------------------------
def test_quantile_to_rank_mapping():
    assert SV.quantile_ranks((0.0, 0.05, 0.5, 0.95, 1.0), 128) == [0, 6, 63, 121, 127] == BR.quantile_ranks((0.0, 0.05, 0.5, 0.95, 1.0), 128)
    assert SV.quantile_ranks((0.0, 0.5, 1.0), 1) == [0, 0, 0]
    assert SV.quantile_ranks((0.5,), 33) == [16] and SV.quantile_ranks((0.25, 0.75), 4) == [0, 2]
    assert SV.quantile_ranks((-0.1, 1.5), 10) == [0, 9]                       # clamped
    # the wrong mapping differs, and selects other words on a committed case
    R = BC.reference("h6_p70")
    good, wrong = BR.quantile_ranks((0.05, 0.5, 0.95), 70), BR.quantile_ranks_floor((0.05, 0.5, 0.95), 70)
    assert good == [3, 34, 66] and wrong == [3, 35, 66]
    assert BR.bands(R["traj"], good)["q"].tobytes() != BR.bands(R["traj"], wrong)["q"].tobytes()


# ---- the restatements --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_vectorised_and_definition_restatements_agree(name):
    R = BC.reference(name)
    H = R["cfg"].horizon
    cols = [(b, t, i) for b in range(BC.B) for t in (0, 1, H) for i in range(13)]
    a = BR.bands_def(R["traj"], R["ranks"], R["obs"], columns=cols)
    for b, t, i in cols:
        assert a["q"][b, :, t, i].tobytes() == R["want"]["q"][b, :, t, i].tobytes(), (b, t, i)
        assert a["below"][b, t, i] == R["want"]["below"][b, t, i] and a["at"][b, t, i] == R["want"]["at"][b, t, i], (b, t, i)


def test_restatements_agree_on_the_special_values_and_a_large_case():
    traj, x0, obs = BC.synthetic_special("h6_p33")
    rk = [32, 0, 16, 1, 31, 16, 29, 28]
    a, b = BR.bands_def(traj, rk, obs), BR.bands(traj, rk, obs)
    assert BR.differs(a, b) == 0
    R = BC.reference("h6_p300")
    cols = [(0, 2, 3), (1, 6, 12), (2, 0, 6)]
    a = BR.bands_def(R["traj"], R["ranks"], R["obs"], columns=cols)
    for c in cols:
        idx = (c[0], slice(None)) + c[1:]
        assert a["q"][idx].tobytes() == R["want"]["q"][idx].tobytes() and a["below"][c] == R["want"]["below"][c] and a["at"][c] == R["want"]["at"][c]


# ---- identities that hold by construction -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.NAMES)
def test_identities(name):
    R = BC.reference(name)
    traj, P = R["traj"], R["cfg"].num_particles
    full = BR.bands(traj, list(range(P)) if P <= 130 else [0, 1, P // 3, P // 2, P - 2, P - 1], R["obs"])
    # rank 0 / rank P-1 are the tube's min / max by value (no NaN in these tensors)
    assert not np.isnan(traj).any()
    ends = BR.bands(traj, [0, P - 1])["q"]
    tube = TR.tube(traj, np.full(13, -np.inf, F), np.full(13, np.inf, F))
    assert (ends[:, 0] == tube["min"]).all() and (ends[:, 1] == tube["max"]).all()
    # q is non-decreasing in the rank, in key order
    assert (np.diff(BR.keys(full["q"]).astype(np.int64), axis=1) >= 0).all()
    # with obs = q[k]: below <= ranks[k] < below + at
    for k, r in enumerate(R["ranks"]):
        o = BR.bands(traj, None, R["want"]["q"][:, k])
        assert (o["below"] <= r).all() and (r < o["below"].astype(np.int64) + o["at"]).all(), (k, r)
    # permuting the particles changes no word
    perm = np.random.default_rng(1).permutation(P)
    assert BR.differs(BR.bands(traj[:, perm], R["ranks"], R["obs"]), R["want"]) == 0
    # t = 0: every rank returns x0; obs = x0 has nothing below and every particle at it
    assert (R["want"]["q"][:, :, 0].view(np.uint32) == R["x0"].view(np.uint32)[:, None]).all()
    assert (R["want"]["below"][:, 0] == 0).all() and (R["want"]["at"][:, 0] == P).all()
    # a NaN observation: below = the non-NaN particles, at = the NaN ones
    nan = np.isnan(R["obs"])
    assert nan.any() and (R["want"]["below"][nan] == P).all() and (R["want"]["at"][nan] == 0).all()


def test_special_values_are_what_they_claim():
    traj, x0, obs = BC.synthetic_special("h6_p33")
    P = 33
    rk = [0, 1, 29, 30, 32]
    w = BR.bands(traj, rk, obs)
    zc = BC.ZERO_COMPONENT
    assert (w["q"][1].view(np.uint32) == 0x7FC00000).all()                        # the all-NaN instance
    assert (w["q"][0, :, 0, zc].view(np.uint32) == 0x80000000).all()              # -0.0 kept
    assert w["below"][0, 0, zc] == P and w["at"][0, 0, zc] == 0                   # obs +0.0 lies above P particles at -0.0
    assert w["below"][2, 0, zc] == 0 and w["at"][2, 0, zc] == P
    assert (w["q"][0, 3:, 1:].view(np.uint32) == 0x7FC00000).all() and not np.isnan(w["q"][0, :3, 1:]).any()     # three NaN particles: ranks 30 .. 32
    nan = np.isnan(obs[0, 1:])
    assert (w["below"][0, 1:][nan] == P - 3).all() and (w["at"][0, 1:][nan] == 3).all()
    assert (w["at"][0][obs[0].view(np.uint32) == traj[0, 0].view(np.uint32)] >= 2).all()                          # ties: particle 1 repeats particle 0
    col = BR.bands(traj, list(range(P)))["q"][0, :, 3, 2].view(np.uint32)         # the column with both zeros: -0.0 twice, then +0.0
    z = np.flatnonzero((col & 0x7FFFFFFF) == 0)
    assert len(z) == P - 3 and (col[z[:2]] == 0x80000000).all() and (col[z[2:]] == 0).all()


# ---- the cases can tell the wrong reducers apart ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in BC.NAMES if BC.shape(n)[2] > 1])
def test_observation_mix(name):
    """with the reference alone: at least a third of the non-NaN columns have 0 < below < P"""
    R = BC.reference(name)
    P = R["cfg"].num_particles
    ok = ~np.isnan(R["obs"])
    b = R["want"]["below"]
    assert ((b > 0) & (b < P))[ok].mean() >= 1 / 3
    assert (R["want"]["at"][ok] >= 1).mean() >= 0.3 and (b[ok] == 0).any() and (b[ok] == P).any()
    assert 0.03 <= (~ok).mean() <= 0.09                                           # about one column in sixteen


def test_every_mutant_changes_a_compared_word():
    caught = {m: [] for m in BR.MUTANTS}
    sets = {n: (BC.reference(n)["traj"], list(BC.reference(n)["ranks"]), BC.reference(n)["obs"]) for n in BC.NAMES}
    traj, _, obs = BC.synthetic_special("h6_p33")
    sets["special"] = (traj, [32, 0, 16, 1, 31, 16], obs)
    for n, (traj, rk, obs) in sets.items():
        good = BR.bands(traj, rk, obs)
        for m, fn in BR.MUTANTS.items():
            if BR.differs(fn(traj, rk, obs), good):
                caught[m].append(n)
    assert len(BR.MUTANTS) >= 10
    for m, where in caught.items():
        assert where, f"no case tells the wrong reducer {m} from the right one"
    assert "h6_p32" not in caught["padded_lanes"] and "h6_p128" not in caught["padded_lanes"]      # no padded lane there
    assert "h6_p33" in caught["padded_lanes"] and "h6_p130" in caught["padded_lanes"]
    assert caught["float_less_than"] == ["special"] and "special" in caught["nan_below_numbers"]  # only the two zeros / a NaN particle can tell
    assert "h6_p31" not in caught["rank_inside_one_group"] and "h6_p70" in caught["rank_inside_one_group"]
    assert set(caught["at_never_nan"]) == {"special"}                                             # the oracle's tensors hold no NaN particle


# ---- host helpers -------------------------------------------------------------------------------------------------------------------------
def _hand_made():
    """P = 4, one instance, H + 1 = 1 step ... as [B=1][T=2][13] planes with a few hand-set columns"""
    P, T = 4, 2
    q = np.zeros((1, 2, T, 13), F)
    q[0, 0], q[0, 1] = -1.0, 2.0
    q[0, 0, 0, 2], q[0, 1, 0, 2] = -0.0, 0.0
    obs = np.zeros((1, T, 13), F)
    below = np.zeros((1, T, 13), np.uint32)
    at = np.zeros((1, T, 13), np.uint32)
    obs[0, 0, 0], below[0, 0, 0], at[0, 0, 0] = 0.5, 2, 0          # pit 0.5
    obs[0, 0, 1], below[0, 0, 1], at[0, 0, 1] = -1.0, 0, 1         # on the lower band: pit 0.125
    obs[0, 0, 2], below[0, 0, 2], at[0, 0, 2] = 0.0, 2, 2          # +0.0 in [-0.0, +0.0]: pit 0.75
    obs[0, 0, 3], below[0, 0, 3], at[0, 0, 3] = 2.5, 4, 0          # above: pit 1
    obs[0, 0, 4], below[0, 0, 4], at[0, 0, 4] = -3.0, 0, 0         # below: pit 0
    obs[0, 0, 5], below[0, 0, 5], at[0, 0, 5] = np.nan, 4, 0       # masked
    obs[0, 1, :], below[0, 1, :], at[0, 1, :] = 0.0, 1, 2          # pit 0.5
    return SV.Bands.of(P, (0, 3), (0.0, 1.0), obs, np.zeros(1, F), q, below, at)


def test_pit_inside_and_calibration_on_a_hand_made_example():
    bd = _hand_made()
    pit = bd.pit
    assert pit.dtype == np.float64 and pit.shape == (1, 2, 13)
    assert list(pit[0, 0, :5]) == [0.5, 0.125, 0.75, 1.0, 0.0] and np.isnan(pit[0, 0, 5]) and (pit[0, 1] == 0.5).all()
    ins = bd.inside(0, 1)
    assert list(ins[0, 0, :6]) == [True, True, True, False, False, False] and ins[0, 1].all()
    bd2 = bd._replace(q=bd.q.copy())
    bd2.q[0, 0, 0, 2] = 0.0                                        # the lower band +0.0, the observation -0.0: outside in key order
    bd2.observed = bd.observed.copy()
    bd2.observed[0, 0, 2] = -0.0
    assert not bd2.inside(0, 1)[0, 0, 2] and bd2.P == 4
    with pytest.raises(ValueError):
        bd.median
    assert SV.Bands.of(4, (1,), (0.5,), None, np.zeros(1, F), bd.q[:, :1], None, None).median.tobytes() == bd.band(0).tobytes()
    with pytest.raises(ValueError):
        SV.Bands.of(4, (1,), (0.5,), None, np.zeros(1, F), bd.q[:, :1], None, None).pit
    cal = SV.calibration([bd, bd], bins=4, levels=(0.5, 0.9))
    assert cal["hist"].shape == (2, 13, 4) and cal["n"].shape == (2, 13) and cal["coverage"].shape == (2, 2, 13)
    assert cal["n"][0, 5] == 0 and cal["hist"][0, 5].sum() == 0 and np.isnan(cal["coverage"][:, 0, 5]).all()     # the masked column
    assert cal["n"][0, 0] == 2 and list(cal["hist"][0, 0]) == [0, 0, 2, 0]                                       # pit 0.5 -> bin 2 of 4
    assert list(cal["hist"][0, 1]) == [2, 0, 0, 0] and list(cal["hist"][0, 3]) == [0, 0, 0, 2]                   # pit 0.125; pit 1 in the last bin
    assert cal["coverage"][0, 0, 0] == 1.0 and cal["coverage"][0, 0, 1] == 0.0 and cal["coverage"][1, 0, 1] == 1.0   # 0.125: outside 50 %, inside 90 %
    assert cal["coverage"][1, 0, 3] == 0.0 and cal["coverage"][0, 0, 2] == 1.0                                   # 1.0 outside both; 0.75 on the 50 % edge


def test_calibration_of_uniform_ranks_is_flat():
    """2,000 synthetic columns whose observation has a uniformly distributed rank among P = 128 distinct particles: `below` uniform on 0 .. 128, at = 0, so
    pit = below / 128 takes 129 equally likely values, of which bin j of 10 holds k_j (12 or 13; the value 1 falls into the last bin): the count of bin j is
    binomial with n = 2000, p_j = k_j / 129. The bound is 4 sigma of that binomial, sqrt(n p (1 - p)) ~ 13.4, i.e. about 54 counts around n p ~ 200; the same
    for the coverage of the central intervals, whose p is the share of the 129 values with |pit - 1/2| <= level / 2. A derivation, not a measurement."""
    n, P, bins = 2000, 128, 10
    rng = np.random.default_rng(12)
    below = rng.integers(0, P + 1, size=(n, 1, 1)).astype(np.uint32)
    bd = SV.Bands.of(P, None, None, np.zeros((n, 1, 1), F), np.zeros(n, F), None, below, np.zeros((n, 1, 1), np.uint32))
    cal = SV.calibration(bd, bins=bins, levels=(0.5, 0.9))
    vals = np.arange(P + 1) / P
    idx = np.clip(np.floor(vals * bins).astype(int), 0, bins - 1)
    assert cal["n"][0, 0] == n and cal["hist"][0, 0].sum() == n
    for j in range(bins):
        p = (idx == j).sum() / (P + 1)
        assert abs(cal["hist"][0, 0, j] - n * p) <= 4 * np.sqrt(n * p * (1 - p)), (j, cal["hist"][0, 0, j], n * p)
    for i, lv in enumerate((0.5, 0.9)):
        p = (np.abs(vals - 0.5) <= lv / 2).sum() / (P + 1)
        assert abs(cal["coverage"][i, 0, 0] - p) <= 4 * np.sqrt(p * (1 - p) / n), (lv, cal["coverage"][i, 0, 0], p)


# ---- no new kernel symbol ----------------------------------------------------------------------------------------------------------------
def test_the_reducer_is_a_mode_of_the_noise_kernel():
    """No new __global__ symbol: the reducer's file declares no kernel, sdempc_prng.hip still has its five, and no built kernel is named for the bands."""
    import kernel_census as kc
    csrc = os.path.join(ROOT, "sde4mbrl_px4_amd", "csrc")
    assert "__global__" not in open(os.path.join(csrc, "sdempc_band.inc.h")).read()
    prng = open(os.path.join(csrc, "sdempc_prng.hip")).read()
    assert prng.count("__global__") == 5 and '#include "sdempc_band.inc.h"' in prng
    for where in (kc.CSRC, kc.AV_DIR):
        built = kc.built_kernels(where)
        if built is None and where == kc.AV_DIR and not os.path.exists(os.path.join(where, "libsdempc.so")):
            continue
        assert built is not None, f"libsdempc.so / its objects are not built in {where}, or nm is missing"
        assert ("sdempc_noise_kernel", "") in built and not [k for k in built if "band" in k[0].lower()]
