"""ctypes mirror of include/sdempc.h (struct layouts + library loader)."""
import ctypes as C
import os

NX = 13
NNOISE = 6
MAX_MOTORS = 8
HID = 32
BLOB_MAGIC = 0x31454453
BLOB_HEADER_INTS = 16
BLOB_FLOATS = 2120

_F8 = C.c_float * MAX_MOTORS
_F3 = C.c_float * 3


class SdempcCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("horizon", C.c_int32),
        ("num_particles", C.c_int32),
        ("num_motors", C.c_int32),
        ("time_steps", C.POINTER(C.c_float)),
        ("discount", C.c_float),
        ("uref", _F8),
        ("uerr", C.c_float),
        ("perr", _F3), ("verr", _F3), ("qerr", _F3), ("werr", _F3),
        ("res_mult", C.c_float),
        ("u_slew_coeff", C.c_float),
        ("has_slew_constr", C.c_int32),
        ("u_slew_lo", _F8), ("u_slew_hi", _F8),
        ("u_slew_constr_coeff", C.c_float),
        ("u_lo", _F8), ("u_hi", _F8),
        ("max_iter", C.c_int32),
        ("max_no_improvement_iter", C.c_int32),
        ("use_moment_scale", C.c_int32),
        ("moment_scale", C.c_float),
        ("beta_init", C.c_float),
        ("atol", C.c_float), ("rtol", C.c_float),
        ("stepsize", C.c_float),
        ("ls_init_stepsize", C.c_float), ("ls_max_stepsize", C.c_float), ("ls_coef", C.c_float),
        ("ls_decrease_factor", C.c_float), ("ls_increase_factor", C.c_float),
        ("ls_reset_option", C.c_int32),
        ("ls_maxls", C.c_int32),
        ("mlp_dtype", C.c_int32),
        ("math_mode", C.c_int32),
        ("num_state_constr", C.c_int32),
        ("state_id", C.c_int32 * NX),
        ("state_w", C.c_float * NX), ("state_lo", C.c_float * NX), ("state_hi", C.c_float * NX),
    ]


class SdempcInfo(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "avg_linesearch", "stepsize", "num_steps", "grad_sqr", "avg_stepsize", "init_cost", "opt_cost",
        "num_ls_trials")]


class SdempcPlantCfg(C.Structure):
    """sdempc_plant_cfg (SPEC.md §11a): the plant set of sdempc_closed_loop_batch_plant."""
    _fields_ = [("struct_size", C.c_int32), ("num_plants", C.c_int32), ("substeps", C.c_int32), ("dt", C.c_float),
                ("mlp_dtype", C.c_int32), ("math_mode", C.c_int32)]


class SdempcTimingCfg(C.Structure):
    """sdempc_timing_cfg (SPEC.md §11b): solve period, solve delay and motor lag of sdempc_closed_loop_batch_timed."""
    _fields_ = [("struct_size", C.c_int32), ("solve_period", C.c_int32), ("solve_delay", C.c_int32), ("lag_alpha", C.c_float)]


class SdempcScenarioCfg(C.Structure):
    """sdempc_scenario_cfg (SPEC.md §11c): the disturbance schedule and the rows of the plant schedule of sdempc_closed_loop_batch_scenario."""
    _fields_ = [("struct_size", C.c_int32), ("dist", C.POINTER(C.c_float)), ("dist_ticks", C.c_int32), ("dist_batch", C.c_int32),
                ("plant_ticks", C.c_int32)]


class SdempcRateCfg(C.Structure):
    """sdempc_rate_cfg (SPEC.md §11d): gains, limits, mixer and blend of the rate loop of sdempc_closed_loop_batch_rate."""
    _fields_ = [("struct_size", C.c_int32), ("kp", _F3), ("ki_dt", _F3), ("integ_limit", _F3), ("mixer", (C.c_float * 3) * MAX_MOTORS),
                ("motor_weight", C.c_float), ("inv_m", C.c_float)]


class SdempcFaultCfg(C.Structure):
    """sdempc_fault_cfg (SPEC.md §11e): the per-motor fault schedule of sdempc_closed_loop_batch_fault."""
    _fields_ = [("struct_size", C.c_int32), ("fault", C.POINTER(C.c_float)), ("fault_ticks", C.c_int32), ("fault_batch", C.c_int32)]


class SdempcObsCfg(C.Structure):
    """sdempc_obs_cfg (SPEC.md §11f): noise scale, bias and validity of the measured state of sdempc_closed_loop_batch_observed."""
    _fields_ = [("struct_size", C.c_int32), ("sigma", C.POINTER(C.c_float)), ("beta", C.POINTER(C.c_float)), ("obs_solves", C.c_int32), ("obs_batch", C.c_int32),
                ("valid", C.POINTER(C.c_int32)), ("valid_solves", C.c_int32), ("valid_batch", C.c_int32)]


class SdempcAgeCfg(C.Structure):
    """sdempc_age_cfg (SPEC.md §11g): the age of the estimate per solve and episode, the depth of the history and the renormalise flag of sdempc_closed_loop_batch_aged."""
    _fields_ = [("struct_size", C.c_int32), ("age", C.POINTER(C.c_int32)), ("age_solves", C.c_int32), ("age_batch", C.c_int32), ("age_max", C.c_int32),
                ("renormalise", C.c_int32)]


class SdempcScoreCfg(C.Structure):
    """sdempc_score_cfg (SPEC.md §11h): which rows are scored, the three thresholds and the target rows of sdempc_closed_loop_batch_scored."""
    _fields_ = [("struct_size", C.c_int32), ("substeps", C.c_int32), ("r2_pos", C.c_float), ("cos_min", C.c_float), ("w2_max", C.c_float),
                ("score_ref", C.POINTER(C.c_float)), ("ref_ticks", C.c_int32), ("ref_batch", C.c_int32)]


SCORE_WORDS = 16         # include/sdempc.h: SDEMPC_SCORE_WORDS
# the score row of an episode as a structured array: the word table of SPEC.md §11h, in order
SCORE_FIELDS = [("rows", "<u4"), ("sum_dp", "<f4"), ("max_dp", "<f4"), ("max_dp_row", "<u4"), ("last_dp", "<f4"), ("sum_dv", "<f4"), ("min_cos_tilt", "<f4"),
                ("max_w2", "<f4"), ("first_fail_row", "<u4"), ("causes", "<u4"), ("fail_rows", "<u4"), ("saturated", "<u4"), ("sum_du2", "<f4"),
                ("sum_steps", "<u4"), ("sum_ls_trials", "<u4"), ("no_decrease", "<u4")]

class SdempcProcessCfg(C.Structure):
    """sdempc_process_cfg (SPEC.md §11i): the coefficients, the key chain and the start state of one first-order Gauss-Markov process of
    sdempc_closed_loop_batch_drawn (width 6: the disturbance, width 12: the estimator bias)."""
    _fields_ = [("struct_size", C.c_int32), ("batch", C.c_int32), ("rho", C.POINTER(C.c_float)), ("scale", C.POINTER(C.c_float)),
                ("keys", C.POINTER(C.c_uint32)), ("state_in", C.POINTER(C.c_float))]


class SdempcTrackCfg(C.Structure):
    """sdempc_track_cfg (SPEC.md §11j): the trajectory set of sdempc_closed_loop_batch_tracked / sdempc_reference_windows — tables end to end, and per episode the
    table, phase, rate and offset (each may be NULL)."""
    _fields_ = [("struct_size", C.c_int32), ("n_tables", C.c_int32), ("knots", C.POINTER(C.c_int32)), ("t", C.POINTER(C.c_float)), ("x", C.POINTER(C.c_float)),
                ("period", C.POINTER(C.c_float)), ("table_of", C.POINTER(C.c_int32)), ("phase", C.POINTER(C.c_float)), ("rate", C.POINTER(C.c_float)),
                ("offset", C.POINTER(C.c_float)), ("tick0", C.c_int32), ("renorm", C.c_int32), ("score_targets", C.c_int32)]


class SdempcTubeCfg(C.Structure):
    """sdempc_tube_cfg (SPEC.md §12): the per-component bounds the tube's `outside` plane counts against (-inf / +inf: none)."""
    _fields_ = [("struct_size", C.c_int32), ("lo", C.c_float * NX), ("hi", C.c_float * NX)]


class SdempcRiskCfg(C.Structure):
    """sdempc_risk_cfg (SPEC.md §12a): where the exit box sits (centre_mode 0 none, 1 caller's rows, 2 xref, 3 particle mean), the tail size of jtail and the
    ranks of jq."""
    _fields_ = [("struct_size", C.c_int32), ("centre_mode", C.c_int32), ("tail_k", C.c_int32), ("n_ranks", C.c_int32), ("ranks", C.c_int32 * 8)]


class SdempcBandsCfg(C.Structure):
    """sdempc_bands_cfg (SPEC.md §12b): the ranks (0-based, in the key order over the valid particles) whose values fill the planes of q."""
    _fields_ = [("struct_size", C.c_int32), ("n_ranks", C.c_int32), ("ranks", C.c_int32 * 8)]


class SdempcOutcomeCfg(C.Structure):
    """sdempc_outcome_cfg (SPEC.md §12c): the three thresholds of the episode score (§11h), where the target rows come from (target_mode 0 the call's xref, 1 the
    caller's rows [tgt_batch][tgt_steps][13]) and the ranks of chan_q / agg_q."""
    _fields_ = [("struct_size", C.c_int32), ("r2_pos", C.c_float), ("cos_min", C.c_float), ("w2_max", C.c_float), ("target_mode", C.c_int32),
                ("tgt_steps", C.c_int32), ("tgt_batch", C.c_int32), ("n_ranks", C.c_int32), ("ranks", C.c_int32 * 8)]


BANDS_MAX_RANKS = 8       # sdempc_bands_cfg.ranks
OUTCOME_MAX_RANKS = 8     # sdempc_outcome_cfg.ranks
OUTCOME_RANK_MAX_P = 128  # chan_q / agg_q are refused above this particle count
OUTCOME_WORDS = 11        # words 0 .. 10 of the score table (SCORE_FIELDS) per particle
RISK_MAX_RANKS = 8        # sdempc_risk_cfg.ranks
RISK_RANK_MAX_P = 4096    # jq / jtail are refused above this particle count

PLANT_MAX_SUBSTEPS = 64  # include/sdempc.h: SDEMPC_PLANT_MAX_SUBSTEPS

INFO_FIELDS = [f[0] for f in SdempcInfo._fields_]

# execution options of a handle (include/sdempc.h, SDEMPC_OPT_*)
OPTIONS = {"lane": 1, "coop": 2, "spec": 3, "pk": 4, "ustg": 5, "coop_launch": 6, "coop_fence": 7, "coop_spin_us": 8, "device_cus": 9, "duo": 10, "hex": 11, "test_absent_wg": 12, "test_ws_fill": 13,
           "test_loop_chunk_bytes": 14}

ABI_VERSION = 3          # include/sdempc.h: SDEMPC_ABI_VERSION (the layout of SdempcCfg / SdempcInfo below)

_LIB = None


def lib_path():
    """csrc/libsdempc.so; SDEMPC_LIB may name another build of the same library (kernel A/B runs)."""
    override = os.environ.get("SDEMPC_LIB")
    if override:
        return os.path.abspath(override)
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libsdempc.so")


def load_library(path=None):
    """Load csrc/libsdempc.so. Fails loudly: there is no CPU fallback for the product path. With `path`: that build of the library instead, beside the
    package's own and not remembered (A/B runs of two builds in one process: SdeMpcSolver(..., lib_path=))."""
    global _LIB
    if path is None and _LIB is not None:
        return _LIB
    explicit = path is not None
    path = os.path.abspath(path) if explicit else lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C sde4mbrl_px4_amd/csrc). sde4mbrl_px4_amd has no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, fp = C.c_void_p, C.c_int32, C.POINTER(C.c_float)
    lib.sdempc_create.argtypes = [C.POINTER(SdempcCfg), vp, C.c_size_t, i32, C.POINTER(vp)]
    lib.sdempc_create.restype = C.c_int
    lib.sdempc_destroy.argtypes = [vp]
    lib.sdempc_destroy.restype = None
    lib.sdempc_last_error.argtypes = [vp]
    lib.sdempc_last_error.restype = C.c_char_p
    lib.sdempc_abi_version.restype = C.c_int
    got = lib.sdempc_abi_version()
    if got != ABI_VERSION:       # a stale build (or an SDEMPC_LIB override made against an older header) would read SdempcCfg past its end
        raise RuntimeError(f"{path} reports ABI version {got}, this package's struct layouts are version {ABI_VERSION} "
                           "(include/sdempc.h: SDEMPC_ABI_VERSION): rebuild the library (make -C sde4mbrl_px4_amd/csrc)")
    lib.sdempc_build_flags.restype = C.c_int
    lib.sdempc_set_device.argtypes = [vp, i32]
    lib.sdempc_device_ready.argtypes = [vp]
    lib.sdempc_device_ready.restype = C.c_int
    lib.sdempc_set_option.argtypes = [vp, i32, i32]
    lib.sdempc_set_option.restype = C.c_int
    lib.sdempc_get_option.argtypes = [vp, i32, C.POINTER(i32)]
    lib.sdempc_get_option.restype = C.c_int
    lib.sdempc_reset.argtypes = [vp, fp, fp, fp, C.POINTER(SdempcInfo)]
    lib.sdempc_rollout_batch.argtypes = [vp, i32, fp, fp, fp, fp, fp, fp, fp]
    lib.sdempc_grad_batch.argtypes = [vp, i32, fp, fp, fp, fp, fp, fp]
    lib.sdempc_solve_batch.argtypes = [vp, i32, fp, fp, fp, fp, fp, fp, fp, C.POINTER(SdempcInfo)]
    lib.sdempc_noise_dev_floats.argtypes = [vp, i32]
    lib.sdempc_noise_dev_floats.restype = C.c_size_t
    lib.sdempc_traj_dev_floats.argtypes = [vp, i32]
    lib.sdempc_traj_dev_floats.restype = C.c_size_t
    lib.sdempc_noise_to_device_layout.argtypes = [vp, i32, fp, fp]
    lib.sdempc_noise_to_device_layout_dev.argtypes = [vp, i32, vp, vp, vp]
    lib.sdempc_traj_to_canonical_dev.argtypes = [vp, i32, vp, vp]
    lib.sdempc_solve_batch_dev.argtypes = [vp, i32] + [vp] * 9
    lib.sdempc_rollout_batch_dev.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.sdempc_grad_batch_dev.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    u32p = C.POINTER(C.c_uint32)
    lib.sdempc_noise_from_keys_dev.argtypes = [vp, i32, u32p, vp, vp]
    lib.sdempc_noise_from_keys.argtypes = [vp, i32, u32p, fp]
    lib.sdempc_solve_batch_keys.argtypes = [vp, i32, fp, fp, u32p, fp, fp, fp, fp, C.POINTER(SdempcInfo)]
    lib.sdempc_closed_loop_batch.argtypes = [vp, i32, i32, fp, fp, i32, i32, u32p, fp, fp, fp, fp, C.POINTER(SdempcInfo), fp, fp, u32p]
    lib.sdempc_closed_loop_batch_plant.argtypes = [vp, C.POINTER(SdempcPlantCfg), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(i32)] + \
        lib.sdempc_closed_loop_batch.argtypes[1:]
    # (sdempc_closed_loop_batch_timed is not part of ABI version 3's first builds: timed_entry() resolves it by symbol on first use)
    lib.sdempc_solve_status.argtypes = [vp]
    lib.sdempc_solve_status.restype = C.c_int
    lib.sdempc_layout_fallbacks.argtypes = [vp]
    lib.sdempc_layout_fallbacks.restype = C.c_int32
    lib.sdempc_work_counters.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    lib.sdempc_work_counters.restype = C.c_int
    lib.sdempc_last_kernel_name.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.sdempc_last_kernel_name.restype = C.c_int
    lib.sdempc_last_kernel_ms.argtypes = [vp]
    lib.sdempc_last_kernel_ms.restype = C.c_float
    for name in ("sdempc_set_device", "sdempc_reset", "sdempc_rollout_batch", "sdempc_grad_batch", "sdempc_solve_batch",
                 "sdempc_noise_to_device_layout", "sdempc_solve_batch_dev", "sdempc_rollout_batch_dev",
                 "sdempc_grad_batch_dev", "sdempc_noise_to_device_layout_dev", "sdempc_traj_to_canonical_dev",
                 "sdempc_noise_from_keys_dev", "sdempc_noise_from_keys", "sdempc_solve_batch_keys", "sdempc_closed_loop_batch",
                 "sdempc_closed_loop_batch_plant"):
        getattr(lib, name).restype = C.c_int
    if not explicit:
        _LIB = lib
    return lib


def timed_entry(lib):
    """sdempc_closed_loop_batch_timed (SPEC.md §11b) with its prototype set. The ABI version did not change with it, so a library built from an
    older tree of the same version may lack it: detected here, by symbol, and only when a call needs it."""
    try:
        fn = lib.sdempc_closed_loop_batch_timed
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_timed (SPEC.md §11b): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(lib.sdempc_closed_loop_batch_plant.argtypes)        # h, plant cfg, blobs, sizes, plant_of, B, T, x0, xref, n, n, keys, u_init, stepsize_in, xs, us, info, 3 x next
        fp = C.POINTER(C.c_float)
        fn.argtypes = [a[0], C.POINTER(SdempcTimingCfg)] + a[1:14] + [fp] + a[14:] + [fp]
        fn.restype = C.c_int
    return fn


def scenario_entry(lib):
    """sdempc_closed_loop_batch_scenario (SPEC.md §11c) with its prototype set: the timed entry point's arguments behind a scenario cfg. Detected by
    symbol and only when a call needs it, as timed_entry is (no ABI version change)."""
    try:
        fn = lib.sdempc_closed_loop_batch_scenario
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_scenario (SPEC.md §11c): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(timed_entry(lib).argtypes)
        fn.argtypes = [a[0], C.POINTER(SdempcScenarioCfg)] + a[1:]
        fn.restype = C.c_int
    return fn


def rate_entry(lib):
    """sdempc_closed_loop_batch_rate (SPEC.md §11d) with its prototype set: the scenario entry point's arguments behind a rate cfg (the scenario cfg may be
    NULL), then rate_integ_in, rate_tail_in, ws, rate_integ_next, rate_tail_next. Detected by symbol and only when a call needs it, as scenario_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_rate
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_rate (SPEC.md §11d): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(scenario_entry(lib).argtypes)
        fp = C.POINTER(C.c_float)
        fn.argtypes = [a[0], C.POINTER(SdempcRateCfg)] + a[1:] + [fp] * 5
        fn.restype = C.c_int
    return fn


def fault_entry(lib):
    """sdempc_closed_loop_batch_fault (SPEC.md §11e) with its prototype set: the rate entry point's arguments (the rate cfg and the scenario cfg may be NULL)
    behind a fault cfg (may be NULL), then xsub. Detected by symbol and only when a call needs it, as rate_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_fault
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_fault (SPEC.md §11e): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(rate_entry(lib).argtypes)
        fn.argtypes = [a[0], C.POINTER(SdempcFaultCfg)] + a[1:] + [C.POINTER(C.c_float)]
        fn.restype = C.c_int
    return fn


def observed_entry(lib):
    """sdempc_closed_loop_batch_observed (SPEC.md §11f) with its prototype set: an obs cfg (may be NULL), obs_keys and xmeas_in in front of the fault entry point's
    arguments, then xmeas, obs_keys_next, xmeas_next. Detected by symbol and only when a call needs it, as fault_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_observed
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_observed (SPEC.md §11f): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(fault_entry(lib).argtypes)
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        fn.argtypes = [a[0], C.POINTER(SdempcObsCfg), u32p, fp] + a[1:] + [fp, u32p, fp]
        fn.restype = C.c_int
    return fn


def aged_entry(lib):
    """sdempc_closed_loop_batch_aged (SPEC.md §11g) with its prototype set: an age cfg (may be NULL) and xhist_in in front of the observed entry point's arguments,
    then xhist_next. Detected by symbol and only when a call needs it, as observed_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_aged
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_aged (SPEC.md §11g): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(observed_entry(lib).argtypes)
        fp = C.POINTER(C.c_float)
        fn.argtypes = [a[0], C.POINTER(SdempcAgeCfg), fp] + a[1:] + [fp]
        fn.restype = C.c_int
    return fn


def scored_entry(lib):
    """sdempc_closed_loop_batch_scored (SPEC.md §11h) with its prototype set: a score cfg (may be NULL) and score_in in front of the aged entry point's arguments,
    then score_out. Detected by symbol and only when a call needs it, as aged_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_scored
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_scored (SPEC.md §11h): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(aged_entry(lib).argtypes)
        u32p = C.POINTER(C.c_uint32)
        fn.argtypes = [a[0], C.POINTER(SdempcScoreCfg), u32p] + a[1:] + [u32p]
        fn.restype = C.c_int
    return fn


def drawn_entry(lib):
    """sdempc_closed_loop_batch_drawn (SPEC.md §11i) with its prototype set: the two process cfgs (each may be NULL) in front of the scored entry point's arguments,
    then rows, keys_next and state_next of the disturbance process and of the bias process. Detected by symbol and only when a call needs it, as scored_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_drawn
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_drawn (SPEC.md §11i): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(scored_entry(lib).argtypes)
        fp, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        fn.argtypes = [a[0], C.POINTER(SdempcProcessCfg), C.POINTER(SdempcProcessCfg)] + a[1:] + [fp, u32p, fp] * 2
        fn.restype = C.c_int
    return fn


def tracked_entry(lib):
    """sdempc_closed_loop_batch_tracked (SPEC.md §11j) with its prototype set: a track cfg (may be NULL) in front of the drawn entry point's arguments; nothing new
    comes back. Detected by symbol and only when a call needs it, as drawn_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_tracked
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_tracked (SPEC.md §11j): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(drawn_entry(lib).argtypes)
        fn.argtypes = [a[0], C.POINTER(SdempcTrackCfg)] + a[1:]
        fn.restype = C.c_int
    return fn


class SdempcFaultProcessCfg(C.Structure):
    """sdempc_fault_process_cfg (SPEC.md §11k): thresholds, modes, key chain, start state and global tick of the motor-fault chain of
    sdempc_closed_loop_batch_events."""
    _fields_ = [("struct_size", C.c_int32), ("n_modes", C.c_int32), ("batch", C.c_int32), ("onset", C.POINTER(C.c_uint32)), ("clear", C.POINTER(C.c_uint32)),
                ("modes", C.POINTER(C.c_float)), ("keys", C.POINTER(C.c_uint32)), ("state_in", C.POINTER(C.c_int32)), ("tick0", C.c_int32)]


class SdempcDropoutProcessCfg(C.Structure):
    """sdempc_dropout_process_cfg (SPEC.md §11k): thresholds, key chain and start state of the estimator-dropout chain of sdempc_closed_loop_batch_events."""
    _fields_ = [("struct_size", C.c_int32), ("batch", C.c_int32), ("drop", C.POINTER(C.c_uint32)), ("recover", C.POINTER(C.c_uint32)),
                ("keys", C.POINTER(C.c_uint32)), ("state_in", C.POINTER(C.c_int32))]


def events_entry(lib):
    """sdempc_closed_loop_batch_events (SPEC.md §11k) with its prototype set: the two event cfgs (each may be NULL) in front of the tracked entry point's arguments,
    then rows, keys_next and state_next of the fault chain and of the dropout chain. Detected by symbol and only when a call needs it, as tracked_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_events
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_events (SPEC.md §11k): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(tracked_entry(lib).argtypes)
        fp, u32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        fn.argtypes = [a[0], C.POINTER(SdempcFaultProcessCfg), C.POINTER(SdempcDropoutProcessCfg)] + a[1:] + [fp, u32p, i32p, i32p, u32p, i32p]
        fn.restype = C.c_int
    return fn


class SdempcGeoCfg(C.Structure):
    """sdempc_geo_cfg (SPEC.md §11l): the parameter sets of the geometric baseline controller of sdempc_closed_loop_batch_baseline / sdempc_geo_command_batch."""
    _fields_ = [("struct_size", C.c_int32), ("batch", C.c_int32)] + \
               [(n, C.POINTER(C.c_float)) for n in ("kp", "kv", "amax", "inv_tau", "g", "kT", "k0", "c_lo", "c_hi")] + \
               [("accel_ff", C.c_int32), ("ref_row", C.c_int32), ("inv_dt", C.c_float)]


def baseline_entry(lib):
    """sdempc_closed_loop_batch_baseline (SPEC.md §11l) with its prototype set: a geo cfg in front of the events entry point's arguments; nothing new comes back.
    Detected by symbol and only when a call needs it, as events_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_baseline
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_baseline (SPEC.md §11l): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(events_entry(lib).argtypes)
        fn.argtypes = [a[0], C.POINTER(SdempcGeoCfg)] + a[1:]
        fn.restype = C.c_int
    return fn


class SdempcEnsembleCfg(C.Structure):
    """sdempc_ensemble_cfg (SPEC.md §11m): cohorts, edges and the inclusion rule of the per-row ensemble reducer of sdempc_closed_loop_batch_ensemble."""
    _fields_ = [("struct_size", C.c_int32), ("n_cohorts", C.c_int32), ("n_edges", C.c_int32), ("over", C.c_int32), ("cohort", C.POINTER(C.c_int32)),
                ("edges", C.POINTER(C.c_float))]


ENSEMBLE_BASE_WORDS = 20         # SDEMPC_ENSEMBLE_BASE_WORDS: a row of (scored row, cohort) holds 20 + 4 * n_edges words


def ensemble_entry(lib):
    """sdempc_closed_loop_batch_ensemble (SPEC.md §11m) with its prototype set: an ensemble cfg (may be NULL) and ens_out in front of the baseline entry point's
    arguments (whose geo cfg may be NULL here: the MPC). Detected by symbol and only when a call needs it, as baseline_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_ensemble
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_ensemble (SPEC.md §11m): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(baseline_entry(lib).argtypes)
        fn.argtypes = [a[0], C.POINTER(SdempcEnsembleCfg), C.POINTER(C.c_uint32)] + a[1:]
        fn.restype = C.c_int
    return fn


class SdempcRetireCfg(C.Structure):
    """sdempc_retire_cfg (SPEC.md §11n): its presence retires failed episodes at the next solve-period boundary in sdempc_closed_loop_batch_retire."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32)]


def retire_entry(lib):
    """sdempc_closed_loop_batch_retire (SPEC.md §11n) with its prototype set: a retire cfg (may be NULL), retired_at and live_per_solve in front of the ensemble
    entry point's arguments. Detected by symbol and only when a call needs it, as ensemble_entry is."""
    try:
        fn = lib.sdempc_closed_loop_batch_retire
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_closed_loop_batch_retire (SPEC.md §11n): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        a = list(ensemble_entry(lib).argtypes)
        fn.argtypes = [a[0], C.POINTER(SdempcRetireCfg), C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + a[1:]
        fn.restype = C.c_int
    return fn


def geo_command_entry(lib):
    """sdempc_geo_command_batch (SPEC.md §11l) with its prototype set. Detected by symbol and only when a call needs it, as baseline_entry is."""
    try:
        fn = lib.sdempc_geo_command_batch
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_geo_command_batch (SPEC.md §11l): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        fp = C.POINTER(C.c_float)
        fn.argtypes = [C.c_void_p, C.POINTER(SdempcGeoCfg), C.c_int32, fp, fp, C.c_int32, fp]
        fn.restype = C.c_int
    return fn


def reference_windows_entry(lib):
    """sdempc_reference_windows (SPEC.md §11j) with its prototype set. Detected by symbol and only when a call needs it, as tracked_entry is."""
    try:
        fn = lib.sdempc_reference_windows
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_reference_windows (SPEC.md §11j): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fn.argtypes is None:
        fn.argtypes = [C.c_void_p, C.POINTER(SdempcTrackCfg), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        fn.restype = C.c_int
    return fn


def tube_entries(lib):
    """sdempc_tube_batch, sdempc_tube_batch_keys and sdempc_tube_batch_dev (SPEC.md §12) with their prototypes set. Detected by symbol and only when a call
    needs them, as the closed-loop entry points are (no ABI version change)."""
    try:
        fns = lib.sdempc_tube_batch, lib.sdempc_tube_batch_keys, lib.sdempc_tube_batch_dev
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_tube_batch (SPEC.md §12): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fns[0].argtypes is None:
        vp, i32, fp, u32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        cfgp = C.POINTER(SdempcTubeCfg)
        fns[0].argtypes = [vp, cfgp, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp, u32p]
        fns[1].argtypes = [vp, cfgp, i32, fp, fp, fp, u32p, fp, fp, fp, fp, fp, u32p]
        fns[2].argtypes = [vp, cfgp, i32, vp, vp, vp, vp, vp, vp]
        for f in fns:
            f.restype = C.c_int
    return fns


def risk_entries(lib):
    """sdempc_risk_batch, sdempc_risk_batch_keys and sdempc_risk_batch_dev (SPEC.md §12a) with their prototypes set; detected by symbol, as tube_entries does."""
    try:
        fns = lib.sdempc_risk_batch, lib.sdempc_risk_batch_keys, lib.sdempc_risk_batch_dev
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_risk_batch (SPEC.md §12a): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fns[0].argtypes is None:
        vp, i32, fp, u32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        cfgp = C.POINTER(SdempcRiskCfg)
        outs = [fp, u32p, fp, u32p, u32p, fp, fp, fp]          # cost, exit, jx, first_exit, outside_any, jstat, jq, jtail
        fns[0].argtypes = [vp, cfgp, i32, fp, fp, fp, fp, fp, fp, fp] + outs
        fns[1].argtypes = [vp, cfgp, i32, fp, fp, fp, u32p, fp, fp, fp] + outs
        fns[2].argtypes = [vp, cfgp, i32] + [vp] * 12
        for f in fns:
            f.restype = C.c_int
    return fns


def bands_entries(lib):
    """sdempc_bands_batch, sdempc_bands_batch_keys and sdempc_bands_batch_dev (SPEC.md §12b) with their prototypes set; detected by symbol, as tube_entries does."""
    try:
        fns = lib.sdempc_bands_batch, lib.sdempc_bands_batch_keys, lib.sdempc_bands_batch_dev
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_bands_batch (SPEC.md §12b): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fns[0].argtypes is None:
        vp, i32, fp, u32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        cfgp = C.POINTER(SdempcBandsCfg)
        fns[0].argtypes = [vp, cfgp, i32, fp, fp, fp, fp, fp, fp, fp, u32p, u32p]      # x0, u, xref, noise, obs, cost, q, below, at
        fns[1].argtypes = [vp, cfgp, i32, fp, fp, fp, u32p, fp, fp, fp, u32p, u32p]
        fns[2].argtypes = [vp, cfgp, i32, vp, vp, vp, vp, vp]
        for f in fns:
            f.restype = C.c_int
    return fns


def outcome_entries(lib):
    """sdempc_outcome_batch, sdempc_outcome_batch_keys and sdempc_outcome_batch_dev (SPEC.md §12c) with their prototypes set; detected by symbol, as tube_entries does."""
    try:
        fns = lib.sdempc_outcome_batch, lib.sdempc_outcome_batch_keys, lib.sdempc_outcome_batch_dev
    except AttributeError:
        raise RuntimeError(f"{lib_path()} has no sdempc_outcome_batch (SPEC.md §12c): rebuild the library (make -C sde4mbrl_px4_amd/csrc)") from None
    if fns[0].argtypes is None:
        vp, i32, fp, u32p = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        cfgp = C.POINTER(SdempcOutcomeCfg)
        outs = [fp, u32p, u32p, u32p, u32p, fp, fp, fp, fp]    # cost, words, fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat, agg_q
        fns[0].argtypes = [vp, cfgp, i32, fp, fp, fp, fp, fp] + outs       # x0, u, xref, noise, target
        fns[1].argtypes = [vp, cfgp, i32, fp, fp, fp, u32p, fp] + outs
        fns[2].argtypes = [vp, cfgp, i32] + [vp] * 11
        for f in fns:
            f.restype = C.c_int
    return fns


EXPORTED_SYMBOLS = [
    "sdempc_create", "sdempc_destroy", "sdempc_last_error", "sdempc_abi_version", "sdempc_build_flags", "sdempc_set_device", "sdempc_device_ready", "sdempc_set_option", "sdempc_get_option", "sdempc_reset",
    "sdempc_rollout_batch", "sdempc_grad_batch", "sdempc_solve_batch", "sdempc_noise_dev_floats",
    "sdempc_traj_dev_floats", "sdempc_noise_to_device_layout", "sdempc_solve_batch_dev", "sdempc_rollout_batch_dev",
    "sdempc_grad_batch_dev", "sdempc_last_kernel_ms", "sdempc_last_kernel_name", "sdempc_work_counters", "sdempc_solve_status", "sdempc_layout_fallbacks", "sdempc_noise_to_device_layout_dev", "sdempc_traj_to_canonical_dev",
    "sdempc_noise_from_keys_dev", "sdempc_noise_from_keys", "sdempc_solve_batch_keys", "sdempc_closed_loop_batch",
    "sdempc_closed_loop_batch_plant", "sdempc_closed_loop_batch_timed", "sdempc_closed_loop_batch_scenario",
    "sdempc_closed_loop_batch_rate", "sdempc_closed_loop_batch_fault", "sdempc_closed_loop_batch_observed",
    "sdempc_closed_loop_batch_aged", "sdempc_closed_loop_batch_scored", "sdempc_closed_loop_batch_drawn",
    "sdempc_closed_loop_batch_tracked", "sdempc_reference_windows", "sdempc_closed_loop_batch_events",
    "sdempc_closed_loop_batch_baseline", "sdempc_geo_command_batch", "sdempc_closed_loop_batch_ensemble",
    "sdempc_closed_loop_batch_retire",
    "sdempc_tube_batch", "sdempc_tube_batch_keys", "sdempc_tube_batch_dev",
    "sdempc_risk_batch", "sdempc_risk_batch_keys", "sdempc_risk_batch_dev",
    "sdempc_bands_batch", "sdempc_bands_batch_keys", "sdempc_bands_batch_dev",
    "sdempc_outcome_batch", "sdempc_outcome_batch_keys", "sdempc_outcome_batch_dev",
]
