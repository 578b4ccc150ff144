"""Thin Python binding of the C ABI (include/sdempc.h): batched rollout / gradient / solve on MI355X.

Host code stays in Python (as in the reference, whose MPC node is Python calling compiled JAX
callables, sde_control.py:681-721); all hot-path arithmetic happens in csrc/libsdempc.so.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _abi
from ._abi import INFO_FIELDS, SdempcInfo


class SdempcError(RuntimeError):
    pass


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


MLP_DTYPES = {"f32": 0, "f16": 1, "f32x3": 2}      # sdempc_cfg::mlp_dtype / sdempc_plant_cfg::mlp_dtype (as MPCConfig.to_cfg)
MATH_MODES = {"exact": 0, "fast": 1}


def _abi_enum(table, value, what):
    """'f32x3' -> 2; integers pass through."""
    if isinstance(value, str):
        if value not in table:
            raise ValueError(f"{what}: unknown value {value!r} (one of {sorted(table)})")
        return table[value]
    return int(value)


class RateLoop:
    """The vehicle's inner body-rate loop behind the node's thrust and body-rate setpoint interface (SPEC.md §11d): a PI controller on the rate error per
    body axis, a mixer that spreads its torque demand over the motors around the solution's mean thrust, and the node's `weight_motors` blend between
    that command and the solution's own motor values. kp / ki / integ_limit: a scalar (all three axes) or three values (roll, pitch, yaw); ki is per second
    (the loop integrates with the plant's step length); integ_limit bounds the integrator state (0: no integral action survives). mixer f32[m][3]: None
    takes the controller model's rate_mixer(). motor_weight in [0, 1] is weight_motors / 100: 0 flies the rate setpoints only (the node's default), 1 the
    motor values only (the integrator still runs). No D-term, no gyro filter, no attitude loop."""

    def __init__(self, kp, ki=0.0, integ_limit=0.0, mixer=None, motor_weight=0.0):
        def axes(v, what):
            a = np.asarray(v, np.float32)
            if a.ndim == 0:
                a = np.full(3, a, np.float32)
            if a.shape != (3,):
                raise ValueError(f"RateLoop: {what} must be a scalar or three values, got shape {a.shape}")
            if not np.isfinite(a).all():
                raise ValueError(f"RateLoop: {what} holds a non-finite value")
            return np.ascontiguousarray(a)

        self.kp, self.ki, self.integ_limit = axes(kp, "kp"), axes(ki, "ki"), axes(integ_limit, "integ_limit")
        if (self.integ_limit < 0).any():
            raise ValueError("RateLoop: integ_limit must be >= 0")
        self.motor_weight = float(np.float32(motor_weight))
        if not (0.0 <= self.motor_weight <= 1.0):
            raise ValueError("RateLoop: motor_weight must be in [0, 1] (the node's weight_motors / 100)")
        self.mixer = None
        if mixer is not None:
            mx = np.ascontiguousarray(mixer, dtype=np.float32)
            if mx.ndim != 2 or mx.shape[1] != 3 or not (1 <= mx.shape[0] <= _abi.MAX_MOTORS):
                raise ValueError(f"RateLoop: mixer must be f32[m][3], got {mx.shape}")
            if not np.isfinite(mx).all():
                raise ValueError("RateLoop: mixer holds a non-finite value")
            self.mixer = mx

    def __repr__(self):
        return f"RateLoop(kp={self.kp.tolist()}, ki={self.ki.tolist()}, integ_limit={self.integ_limit.tolist()}, mixer={self.mixer!r}, motor_weight={self.motor_weight})"


class GeometricController:
    """The geometric baseline controller (SPEC.md §11l): PD position feedback with a clip on the norm of the acceleration, a desired attitude from the desired
    acceleration and the reference heading, the SO(3) attitude error as body-rate commands and a collective thrust along the current body z axis. It publishes the
    interface a RateLoop consumes, so closed_loop(controller=..., rate_loop=...) flies it in place of the MPC's solves, everything else untouched. kp / kv: a
    scalar, three values (x, y, z) or f32[B][3] (one set per episode); max_acc, attctrl_tau, gravity, thrust_const, thrust_offset, thrust_min, thrust_max: a
    scalar or f32[B]. The thrust command is clamp(thrust_const * (a_des . z_body) + thrust_offset, thrust_min, thrust_max) in the model's motor units (None: the
    tightest input bound of the handle's motors); accel_ff adds the window's velocity difference of rows ref_row, ref_row + 1 over its time step as a feed-forward
    acceleration. Not built: the quaternion-error mode, rotor drag, feed-through."""

    def __init__(self, kp, kv, max_acc, attctrl_tau, gravity, thrust_const, thrust_offset, thrust_min=None, thrust_max=None, accel_ff=False, ref_row=0):
        def rows(v, what, width, nonneg=True):
            a = np.asarray(v, np.float32)
            if width == 3 and a.ndim == 0:
                a = np.full(3, a, np.float32)
            a = a.reshape((1,) + a.shape) if a.ndim == (1 if width == 3 else 0) else a
            if a.ndim != (2 if width == 3 else 1) or (width == 3 and a.shape[1] != 3) or a.shape[0] < 1:
                raise ValueError(f"GeometricController: {what} must be a scalar" + (", three values or f32[B][3]" if width == 3 else " or f32[B]") + f", got shape {np.shape(v)}")
            if not np.isfinite(a).all() or (nonneg and (a < 0).any()):
                raise ValueError(f"GeometricController: {what} holds a non-finite" + (" or negative" if nonneg else "") + " value")
            return np.ascontiguousarray(a)

        self.kp, self.kv = rows(kp, "kp", 3), rows(kv, "kv", 3)
        self.max_acc, self.gravity = rows(max_acc, "max_acc", 1), rows(gravity, "gravity", 1)
        tau = rows(attctrl_tau, "attctrl_tau", 1)
        if (tau <= 0).any():
            raise ValueError("GeometricController: attctrl_tau must be > 0")
        self.attctrl_tau = tau
        self.inv_tau = (np.float32(1.0) / tau).astype(np.float32)
        self.thrust_const, self.thrust_offset = rows(thrust_const, "thrust_const", 1, False), rows(thrust_offset, "thrust_offset", 1, False)
        self.thrust_min = None if thrust_min is None else rows(thrust_min, "thrust_min", 1, False)
        self.thrust_max = None if thrust_max is None else rows(thrust_max, "thrust_max", 1, False)
        self.accel_ff, self.ref_row = bool(accel_ff), int(ref_row)
        if self.ref_row < 0:
            raise ValueError("GeometricController: ref_row must be >= 0")
        sizes = {a.shape[0] for a in self._params() if a is not None and a.shape[0] > 1}
        if len(sizes) > 1:
            raise ValueError(f"GeometricController: per-episode parameters disagree on B: {sorted(sizes)}")
        self.batch = sizes.pop() if sizes else 1

    def _params(self):
        return (self.kp, self.kv, self.max_acc, self.inv_tau, self.gravity, self.thrust_const, self.thrust_offset, self.thrust_min, self.thrust_max)

    @classmethod
    def from_yaml(cls, path, **kw):
        """The reference's controller settings file, keys verbatim: attctrl_tau, norm_thrust_const, norm_thrust_offset, max_acc, gravity, Kp_*, Kv_*. Its thrust
        constants belong to PX4's normalised thrust: for_model calibrates them for a model of this package. trajectory_path is ignored."""
        import yaml
        with open(path) as f:
            d = yaml.safe_load(f)
        if int(d.get("ctrl_mode", 2)) != 2:
            raise NotImplementedError("GeometricController: ctrl_mode 1 (quaternion error) needs a division, which SPEC.md §3 does not have; only ctrl_mode 2 is built")
        if any(float(d.get(k, 0.0)) != 0.0 for k in ("drag_dx", "drag_dy", "drag_dz")):
            raise NotImplementedError("GeometricController: rotor drag is not built (drag_d* must be 0)")
        if bool(d.get("feedthrough_enable", False)):
            raise NotImplementedError("GeometricController: feedthrough_enable is not built")
        args = dict(kp=[d["Kp_x"], d["Kp_y"], d["Kp_z"]], kv=[d["Kv_x"], d["Kv_y"], d["Kv_z"]], max_acc=d["max_acc"], attctrl_tau=d["attctrl_tau"], gravity=d["gravity"],
                    thrust_const=d["norm_thrust_const"], thrust_offset=d["norm_thrust_offset"])
        args.update(kw)
        return cls(**args)

    @staticmethod
    def hover_calibration(model):
        """(u_h, kT, k0) in float64 for a RotorSDEModel: the hover command u_h solves m (ct2 u^2 + ct1 u + ct0) = mass grav; kT = mass / (m (2 ct2 u_h + ct1)) is
        the command per acceleration along the body axis there, k0 = u_h - kT grav."""
        m, mass, grav = int(model.num_motors), float(model.mass), float(model.grav)
        ct2, ct1, ct0 = (float(v) for v in np.asarray(model.thrust_poly, np.float64))
        c = ct0 - mass * grav / m
        if ct2 == 0.0:
            u_h = -c / ct1
        else:
            disc = ct1 * ct1 - 4.0 * ct2 * c
            if disc < 0:
                raise ValueError("GeometricController.for_model: the model cannot hover (no real hover command)")
            u_h = (-ct1 + np.sqrt(disc)) / (2.0 * ct2)
        kT = mass / (m * (2.0 * ct2 * u_h + ct1))
        return u_h, kT, u_h - kT * grav

    @classmethod
    def for_model(cls, model, **gains):
        """A controller whose thrust map is calibrated for `model` (hover_calibration, rounded to float32) and whose gravity is the model's; the gains (kp, kv,
        max_acc, attctrl_tau, and optionally thrust_min, thrust_max, accel_ff, ref_row) are the caller's."""
        _, kT, k0 = cls.hover_calibration(model)
        gains.setdefault("gravity", float(model.grav))
        return cls(thrust_const=float(np.float32(kT)), thrust_offset=float(np.float32(k0)), **gains)

    def arrays(self, B, u_lo, u_hi):
        """The parameter sets as the C ABI takes them: (batch, dict of contiguous f32 arrays with `batch` rows), batch 1 or B. thrust_min / thrust_max None: the
        tightest of the motors' input bounds u_lo / u_hi."""
        if self.batch not in (1, B):
            raise ValueError(f"GeometricController: per-episode parameters are for B = {self.batch}, the call has B = {B}")
        lo = np.full(1, np.max(np.asarray(u_lo, np.float32)), np.float32) if self.thrust_min is None else self.thrust_min
        hi = np.full(1, np.min(np.asarray(u_hi, np.float32)), np.float32) if self.thrust_max is None else self.thrust_max
        if lo.shape[0] not in (1, self.batch) or hi.shape[0] not in (1, self.batch):
            raise ValueError("GeometricController: thrust_min / thrust_max disagree with the other parameters on B")
        if (np.broadcast_to(lo, (self.batch,)) > np.broadcast_to(hi, (self.batch,))).any():
            raise ValueError("GeometricController: thrust_min must not exceed thrust_max")
        names = ("kp", "kv", "amax", "inv_tau", "g", "kT", "k0", "c_lo", "c_hi")
        vals = (self.kp, self.kv, self.max_acc, self.inv_tau, self.gravity, self.thrust_const, self.thrust_offset, lo, hi)
        return self.batch, {n: np.ascontiguousarray(np.broadcast_to(v, (self.batch,) + v.shape[1:]), dtype=np.float32) for n, v in zip(names, vals)}

    def __repr__(self):
        return (f"GeometricController(kp={self.kp.tolist()}, kv={self.kv.tolist()}, max_acc={self.max_acc.tolist()}, attctrl_tau={self.attctrl_tau.tolist()}, "
                f"gravity={self.gravity.tolist()}, thrust_const={self.thrust_const.tolist()}, thrust_offset={self.thrust_offset.tolist()}, accel_ff={self.accel_ff}, "
                f"ref_row={self.ref_row})")


def fault_schedule(T, B, m):
    """The neutral per-motor fault schedule f32[T][B][m][2] of closed_loop(fault=...) (SPEC.md §11e): every row (kappa, beta) = (1, 0), to be edited in place.
    Row (k, b, l) acts on every plant substep of control tick k of episode b: what reaches rotor l is fma(kappa, a_l, beta), a_l the motor state (which
    the fault does not change, and of which neither the solve nor the rate loop is told). Recipes, for motor l of episode b from tick k on:
        a dead motor                 f[k:, b, l] = (0, 0)        (thrust ct0, no moment, the plant's residual sees a command of 0)
        a loss of effectiveness      f[k:, b, l] = (kappa, 0)    with 0 < kappa < 1
        a motor stuck at c           f[k:, b, l] = (0, c)
        a bias                       f[k:, b, l] = (1, delta)
    Rows change at tick starts only (ticks inside a solve period included); nothing is clamped."""
    f = np.zeros((int(T), int(B), int(m), 2), np.float32)
    f[..., 0] = 1.0
    return f


def gauss_markov_bias(Ns, B, std, tau, solve_dt, rng, state=None):
    """COLOURED estimator noise for closed_loop(meas_bias=...) (SPEC.md §11g): beta f32[Ns][B][12], a first-order Gauss-Markov process per component and episode,
    sampled once per solve. With rho = exp(-solve_dt / tau) (solve_dt the time between two solves, tau the correlation time, both in seconds):
        b_j = rho * b_{j-1} + std * sqrt(1 - rho^2) * w_j,   w_j standard normal from `rng` (a numpy Generator),
    so that every b_j has deviation std (the stationary one) and consecutive rows correlate with rho. std and tau are scalars or broadcast against [B][12] (order p, v,
    theta, omega, as meas_bias). `state` f64[B][12] is b_{-1} (the second value a previous call returned, to continue a run); None draws it from the stationary
    distribution. Computed in float64 and cast once. Returns (beta, state): the rows and the last b in float64. This is the answer to "coloured noise": the device
    loop needs no keyword for it, since meas_bias rows carry any error sequence the caller draws; add white noise on top with meas_noise.
    closed_loop(bias_process=GaussMarkov(...), bias_keys=...) draws the same process on the device from keys (SPEC.md §11i), with no host rows at all."""
    Ns, B = int(Ns), int(B)
    std = np.broadcast_to(np.asarray(std, np.float64), (B, 12))
    tau = np.broadcast_to(np.asarray(tau, np.float64), (B, 12))
    if Ns < 1 or B < 1 or not (np.isfinite(std).all() and (std >= 0).all()) or not (tau > 0).all() or not float(solve_dt) > 0:
        raise ValueError("gauss_markov_bias: Ns, B >= 1, std finite and >= 0, tau > 0 and solve_dt > 0 are required")
    rho = np.exp(-float(solve_dt) / tau)
    scale = std * np.sqrt(1.0 - rho * rho)
    b = std * rng.standard_normal((B, 12)) if state is None else np.array(state, np.float64).reshape(B, 12)
    out = np.empty((Ns, B, 12), np.float64)
    for j in range(Ns):
        b = rho * b + scale * rng.standard_normal((B, 12))
        out[j] = b
    return out.astype(np.float32), b


class GaussMarkov:
    """A first-order Gauss-Markov process per component and episode, drawn ON THE DEVICE from a key chain (SPEC.md §11i): closed_loop(dist_process=...) steps it once
    per control tick into the disturbance row (width 6: w_v, w_omega), closed_loop(bias_process=...) once per solve into the estimator bias (width 12: p, v, theta,
    omega). One step is g <- fma(rho, g, scale * xi), xi a standard normal of the step's key. GaussMarkov(std, tau, dt): std the stationary deviation, tau the
    correlation time and dt the time between two steps (a control tick or a solve period), both in seconds; rho = exp(-dt / tau) and scale = std * sqrt(1 - rho^2) are
    computed in float64 and cast to float32 once, as gauss_markov_bias does. std and tau are scalars or broadcast against [B][W]. from_coeffs(rho, scale) takes the
    two float32 coefficients as they are (rho in [0, 1], scale finite and >= 0)."""

    def __init__(self, std, tau, dt):
        std, tau = np.asarray(std, np.float64), np.asarray(tau, np.float64)
        if not (np.isfinite(std).all() and (std >= 0).all()) or not (tau > 0).all() or not float(dt) > 0:
            raise ValueError("GaussMarkov: std finite and >= 0, tau > 0 and dt > 0 are required")
        rho = np.exp(-float(dt) / tau)
        std, rho = np.broadcast_arrays(std, rho)
        self.std = np.array(std, np.float64)
        self.rho = np.asarray(rho, np.float64).astype(np.float32)
        self.scale = (std * np.sqrt(1.0 - rho * rho)).astype(np.float32)

    @classmethod
    def from_coeffs(cls, rho, scale):
        rho, scale = np.broadcast_arrays(np.asarray(rho, np.float32), np.asarray(scale, np.float32))
        if not (np.isfinite(scale).all() and (scale >= 0).all()) or not ((rho >= 0).all() and (rho <= 1).all()):
            raise ValueError("GaussMarkov.from_coeffs: rho in [0, 1] and scale finite and >= 0 are required")
        self = cls.__new__(cls)
        self.rho, self.scale = np.array(rho, np.float32), np.array(scale, np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = self.rho.astype(np.float64)
            self.std = np.where(self.scale > 0, self.scale.astype(np.float64) / np.sqrt(1.0 - r * r), 0.0)
        return self

    def coeffs(self, B, W):
        """(rho, scale) as contiguous f32[Bp][W], Bp = 1 (one row for all episodes) or B."""
        out = []
        for a in (self.rho, self.scale):
            a = a.reshape((1,) * (2 - a.ndim) + a.shape) if a.ndim < 2 else a
            if a.ndim != 2 or a.shape[0] not in (1, B) or a.shape[1] not in (1, W):
                raise ValueError(f"GaussMarkov: std / tau must be scalars or broadcast against [{B}][{W}], got {a.shape}")
            out.append(np.ascontiguousarray(np.broadcast_to(a, (a.shape[0], W)), np.float32))
        return out[0], out[1]

    def stationary_state(self, rng, B, W=None):
        """A start from the stationary distribution: std * N(0, 1) from `rng` (a numpy Generator), f32[B][W]. W defaults to the last axis of std / tau."""
        if W is None:
            W = self.std.shape[-1] if self.std.ndim else 0
        if W not in (6, 12):
            raise ValueError("GaussMarkov.stationary_state: pass W=6 (disturbance) or W=12 (bias) when std and tau do not carry the component axis")
        if not np.isfinite(self.std).all():
            raise ValueError("GaussMarkov.stationary_state: a component with rho = 1 has no stationary distribution")
        return (np.broadcast_to(self.std, (int(B), W)) * rng.standard_normal((int(B), W))).astype(np.float32)

    def __repr__(self):
        return f"GaussMarkov.from_coeffs(rho={self.rho.tolist()}, scale={self.scale.tolist()})"


def _threshold_words(p, what):
    """min(2^32 - 1, floor(p * 2^32)) of probabilities in [0, 1], formed once in float64 (SPEC.md §11k): a word w drawn uniformly fires when w < threshold, so 0 never
    fires and 2^32 - 1 fires on all but one word."""
    p = np.asarray(p, np.float64)
    if not (np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()):
        raise ValueError(f"{what}: probabilities must lie in [0, 1]")
    return np.minimum(np.floor(p * 4294967296.0), 4294967295.0).astype(np.uint32)


def _rate_probability(rate_per_s, dt):
    return -np.expm1(-np.asarray(rate_per_s, np.float64) * float(dt))


def _duration_probability(mean_duration_s, dt):
    d = np.asarray(mean_duration_s, np.float64)
    if not (d > 0).all():
        raise ValueError("from_rates: mean_duration_s must be > 0 (inf: never clears)")
    with np.errstate(divide="ignore"):
        return np.where(np.isinf(d), 0.0, -np.expm1(-float(dt) / d))


class FaultProcess:
    """Motor faults at RANDOM times, drawn ON THE DEVICE from a key chain (SPEC.md §11k): closed_loop(fault_process=...) steps, per episode and motor, a Markov chain
    with K <= 4 failure modes once per control tick. FaultProcess(p_onset, p_clear, modes): p_onset f64[m][K] or [B][m][K] is the probability PER TICK that a healthy
    motor enters mode j (not cumulative; a row's sum may not exceed 1), p_clear, same shape, the probability per tick that a motor in mode j recovers (0: the failure
    is permanent), modes f32[m][K][2] or [B][m][K][2] the fault row (kappa, beta) of each mode, as a row of closed_loop(fault=...) — see fault_schedule() for the
    recipes. The device compares threefry words with uint32 thresholds min(2^32 - 1, floor(p * 2^32)), the onset ones cumulated in float64 first, so a probability of
    0 is exactly never and 1 is all but one word in 2^32 ("always" is not expressible). from_rates(rate_per_s, mean_duration_s, dt, modes) takes failure rates
    [1/s] and mean durations [s] (inf: permanent) with dt the control tick: p = 1 - exp(-rate dt), p_clear = 1 - exp(-dt / duration). from_thresholds(onset, clear,
    modes) takes the words as they are (onset cumulative, nondecreasing along K)."""

    def __init__(self, p_onset, p_clear, modes):
        p_onset = np.asarray(p_onset, np.float64)
        if p_onset.ndim not in (2, 3):
            raise ValueError(f"FaultProcess: p_onset must be [m][K] or [B][m][K], got {p_onset.shape}")
        if not (np.isfinite(p_onset).all() and (p_onset >= 0).all()):
            raise ValueError("FaultProcess: probabilities must lie in [0, 1]")
        cum = np.cumsum(p_onset, axis=-1)
        if (cum[..., -1] > 1.0).any():
            raise ValueError("FaultProcess: the onset probabilities of a motor sum to more than 1")
        self._set(_threshold_words(cum, "FaultProcess"), _threshold_words(np.broadcast_to(np.asarray(p_clear, np.float64), p_onset.shape), "FaultProcess"), modes)

    def _set(self, onset, clear, modes):
        onset, clear = np.asarray(onset), np.asarray(clear)
        if onset.ndim not in (2, 3) or clear.shape != onset.shape or not 1 <= onset.shape[-1] <= 4:
            raise ValueError(f"FaultProcess: onset and clear must both be [m][K] or [B][m][K] with 1 <= K <= 4, got {onset.shape} and {clear.shape}")
        for a in (onset, clear):
            if a.dtype.kind not in "iu" or (a < 0).any() or (a > 0xFFFFFFFF).any():
                raise ValueError("FaultProcess: thresholds must be integers in [0, 2^32)")
        if (np.diff(onset.astype(np.int64), axis=-1) < 0).any():
            raise ValueError("FaultProcess: an onset row decreases (the thresholds are cumulative)")
        self.onset = (onset if onset.ndim == 3 else onset[None]).astype(np.uint32)
        self.clear = (clear if clear.ndim == 3 else clear[None]).astype(np.uint32)
        md = np.asarray(modes, np.float32)
        if md.ndim not in (3, 4) or md.shape[-3:] != self.onset.shape[1:] + (2,):
            raise ValueError(f"FaultProcess: modes must be [m][K][2] or [B][m][K][2] for thresholds {self.onset.shape[1:]}, got {md.shape}")
        if not np.isfinite(md).all():
            raise ValueError("FaultProcess: modes holds a non-finite entry")
        self.modes = md if md.ndim == 4 else md[None]
        self.n_modes = int(self.onset.shape[-1])

    @classmethod
    def from_rates(cls, rate_per_s, mean_duration_s, dt, modes):
        if not float(dt) > 0:
            raise ValueError("FaultProcess.from_rates: dt > 0 is required")
        rate = np.asarray(rate_per_s, np.float64)
        if not (np.isfinite(rate).all() and (rate >= 0).all()):
            raise ValueError("FaultProcess.from_rates: rates must be finite and >= 0")
        return cls(_rate_probability(rate, dt), _duration_probability(np.broadcast_to(np.asarray(mean_duration_s, np.float64), rate.shape), dt), modes)

    @classmethod
    def from_thresholds(cls, onset, clear, modes):
        self = cls.__new__(cls)
        self._set(onset, clear, modes)
        return self

    def arrays(self, B, m):
        """(onset, clear) as contiguous u32[Bp][m][K] and modes as f32[Bp][m][K][2], Bp = 1 (one set for all episodes) or B."""
        Bp = max(self.onset.shape[0], self.modes.shape[0])
        if self.onset.shape[1] != m or Bp not in (1, B) or self.onset.shape[0] not in (1, Bp) or self.modes.shape[0] not in (1, Bp):
            raise ValueError(f"FaultProcess: thresholds {self.onset.shape} and modes {self.modes.shape} do not fit {B} episodes of {m} motors")
        K = self.n_modes
        return (np.ascontiguousarray(np.broadcast_to(self.onset, (Bp, m, K))), np.ascontiguousarray(np.broadcast_to(self.clear, (Bp, m, K))),
                np.ascontiguousarray(np.broadcast_to(self.modes, (Bp, m, K, 2))))

    def __repr__(self):
        return f"FaultProcess.from_thresholds(onset={self.onset.tolist()}, clear={self.clear.tolist()}, modes={self.modes.tolist()})"


class Dropouts:
    """Bursty loss of the state estimate, drawn ON THE DEVICE from a key chain (SPEC.md §11k): closed_loop(drop_process=...) steps a two-state chain per episode once
    per SOLVE, valid or not; while it is in the dropped state the solve's measurement is held, as under meas_valid = 0. Dropouts(p_drop, p_recover): the
    probability per solve of dropping out and of recovering, scalars or f64[B]. Thresholds as in FaultProcess. from_rates(rate_per_s, mean_duration_s, dt) with dt
    the time between two solves; from_thresholds(drop, recover) takes the words as they are."""

    def __init__(self, p_drop, p_recover):
        self._set(_threshold_words(p_drop, "Dropouts"), _threshold_words(p_recover, "Dropouts"))

    def _set(self, drop, recover):
        drop, recover = np.broadcast_arrays(np.atleast_1d(drop), np.atleast_1d(recover))
        for a in (drop, recover):
            if a.ndim != 1 or a.dtype.kind not in "iu" or (a < 0).any() or (a > 0xFFFFFFFF).any():
                raise ValueError("Dropouts: thresholds must be integers in [0, 2^32), scalars or [B]")
        self.drop, self.recover = drop.astype(np.uint32), recover.astype(np.uint32)

    @classmethod
    def from_rates(cls, rate_per_s, mean_duration_s, dt):
        if not float(dt) > 0:
            raise ValueError("Dropouts.from_rates: dt > 0 is required")
        rate = np.asarray(rate_per_s, np.float64)
        if not (np.isfinite(rate).all() and (rate >= 0).all()):
            raise ValueError("Dropouts.from_rates: rates must be finite and >= 0")
        return cls(_rate_probability(rate, dt), _duration_probability(mean_duration_s, dt))

    @classmethod
    def from_thresholds(cls, drop, recover):
        self = cls.__new__(cls)
        self._set(np.asarray(drop), np.asarray(recover))
        return self

    def arrays(self, B):
        """(drop, recover) as contiguous u32[Bp], Bp = 1 or B."""
        if self.drop.shape[0] not in (1, B):
            raise ValueError(f"Dropouts: thresholds {self.drop.shape} do not fit {B} episodes")
        return np.ascontiguousarray(self.drop), np.ascontiguousarray(self.recover)

    def __repr__(self):
        return f"Dropouts.from_thresholds(drop={self.drop.tolist()}, recover={self.recover.tolist()})"


def event_summary(fault_state, score=None):
    """Host reduction of fault_state_next int32[B][m][2] (SPEC.md §11k): episodes with any onset, onsets per motor (episodes whose motor l left state 0 at least
    once), the first onset tick per episode (-1: none) and, with the score words of the same run, the failure rate among faulted and among unfaulted episodes (NaN
    for an empty group). An episode failed when its score has a first failing row."""
    st = np.asarray(fault_state)
    if st.ndim != 3 or st.shape[2] != 2:
        raise ValueError(f"event_summary: fault_state must be int[B][m][2], got {st.shape}")
    first = st[:, :, 1]
    hit = first >= 0
    faulted = hit.any(axis=1)
    out = {"episodes": int(st.shape[0]), "faulted": int(faulted.sum()), "onsets_per_motor": hit.sum(axis=0).astype(np.int64),
           "first_onset_tick": np.where(faulted, np.where(hit, first, np.iinfo(np.int32).max).min(axis=1), -1).astype(np.int64)}
    if score is not None:
        score = np.asarray(score)
        if score.dtype != SCORE_DTYPE or score.shape != (st.shape[0],):
            raise ValueError("event_summary: score must be the structured score array [B] of the same run")
        failed = score["first_fail_row"] != 0xFFFFFFFF
        out["fail_rate_faulted"] = float(failed[faulted].mean()) if faulted.any() else float("nan")
        out["fail_rate_unfaulted"] = float(failed[~faulted].mean()) if (~faulted).any() else float("nan")
    return out


class Score:
    """What closed_loop(score=...) scores an episode against (SPEC.md §11h): pos_radius [m] around the tick's target, tilt_max [rad] from the vertical, rate_max
    [rad/s] on the body-rate vector; substeps=True scores the plant's substep states instead of the tick states. The device compares squares and a cosine, so
    the three float32 thresholds are formed here: r2_pos = pos_radius^2, cos_min = cos(tilt_max), w2_max = rate_max^2, each computed in float64 and rounded to
    float32 ONCE (so a squared threshold is not the square of the rounded radius). The defaults (inf, pi, inf) give +inf, -inf, +inf: the criterion is off —
    tilt_max >= pi maps to -inf, not to cos(pi), since c >= -1 would still fail at c = -1 - ulp. A row fails a criterion when it is not inside it: dp <= r2_pos,
    c >= cos_min, w2 <= w2_max, and a NaN is never inside."""

    def __init__(self, pos_radius=np.inf, tilt_max=np.pi, rate_max=np.inf, substeps=False):
        r, t, w = float(pos_radius), float(tilt_max), float(rate_max)
        if not (r >= 0.0) or not (t >= 0.0) or not (w >= 0.0):
            raise ValueError("Score: pos_radius, tilt_max and rate_max must be >= 0 (and not NaN)")
        self.pos_radius, self.tilt_max, self.rate_max, self.substeps = r, t, w, bool(substeps)
        with np.errstate(over="ignore"):
            self.r2_pos = np.float32(np.float64(r) * np.float64(r))
            self.cos_min = np.float32(-np.inf) if t >= np.pi else np.float32(np.cos(np.float64(t)))
            self.w2_max = np.float32(np.float64(w) * np.float64(w))

    def thresholds(self):
        """(r2_pos, cos_min, w2_max) as float32."""
        return self.r2_pos, self.cos_min, self.w2_max

    def __repr__(self):
        return f"Score(pos_radius={self.pos_radius}, tilt_max={self.tilt_max}, rate_max={self.rate_max}, substeps={self.substeps})"


# Host arithmetic of Trajectory.rows only (a restatement for users: planning, plots). The AUTHORITATIVE statement of these two functions is oracle/sde_mpc_numpy.py
# (fma, rsqrt; SPEC.md §3), which the device is tested against; the package may import neither oracle/ nor tests/, so they are restated here, and
# tests/test_track_loop_cpu.py holds Trajectory.windows bit for bit to tests/track_loop_ref.py, which is written with the oracle's. Change the oracle's first.
def _fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding: the product is exact in float64, the sum is corrected to round-to-odd there, then cast."""
    a, b, c = np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(p + c64)
        t = s - p
        e = (p - (s - t)) + (c64 - t)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _rsqrt32(a):
    """The software reciprocal square root of SPEC.md §3.2, in float32."""
    a = np.asarray(a, np.float32)
    y = (np.uint32(0x5F3759DF) - (a.view(np.uint32) >> np.uint32(1))).view(np.float32)
    h = np.float32(0.5) * a
    for _ in range(3):
        y = y * _fma32(-h, y * y, np.float32(1.5))
    return y


class Trajectory:
    """A piecewise-linear trajectory table for closed_loop(track=...) and reference_windows (SPEC.md §11j): L >= 1 knots, times t f32[L] (finite, strictly
    increasing) and states x f32[L][13] IN THE SOLVER'S FRAME, as every reference window is. period = 0 clamps at the ends; period > 0 wraps the trajectory time
    (then t[0] = 0 and t[L-1] = period are required, and the last knot should repeat the first). The device cuts every solve's window and every tick's score target
    from the table, per episode through a phase, a rate >= 0 and a position offset: row(u) is the table at tau = fma(rate, u, phase), linearly interpolated in
    float32, position + offset, velocity and body rates times rate, the attitude (interpolated component by component) scaled to unit length when asked. The
    constructors flip knot quaternion signs (an exact negation) so that consecutive knots have a non-negative dot product; nothing else is touched. This is a
    different arithmetic from a float64 state_from_traj evaluated on the host: the same trajectory to a few float32 ulps of a linear interpolant, not bit for bit."""

    def __init__(self, t, x, period=0.0):
        t = np.ascontiguousarray(t, dtype=np.float32).reshape(-1)
        x = np.array(x, dtype=np.float32, order="C")
        L = t.shape[0]
        if L < 1 or x.shape != (L, 13):
            raise ValueError(f"Trajectory: t must be f32[L] with L >= 1 and x f32[L][13], got {t.shape} and {x.shape}")
        if not np.isfinite(t).all() or (L > 1 and not (np.diff(t) > 0).all()):
            raise ValueError("Trajectory: t must be finite and strictly increasing (in float32)")
        if not np.isfinite(x).all():
            raise ValueError("Trajectory: x holds a non-finite entry")
        period = np.float32(period)
        if not np.isfinite(period) or period < 0:
            raise ValueError("Trajectory: period must be finite and >= 0")
        if period > 0 and (t[0] != 0 or t[-1] != period):
            raise ValueError("Trajectory: a periodic table needs t[0] = 0 and t[L-1] = period (in float32)")
        for i in range(1, L):          # (sequential: each knot against the one before it, as already flipped)
            if np.dot(x[i - 1, 6:10].astype(np.float64), x[i, 6:10].astype(np.float64)) < 0:
                x[i, 6:10] = -x[i, 6:10]
        self.t, self.x, self.period = t, x, period

    @classmethod
    def from_knots(cls, t, x, period=0.0):
        return cls(t, x, period)

    @classmethod
    def from_function(cls, state_fn, t0, t1, n, period=0.0):
        """n >= 1 knots of state_fn (t f64[n] -> [n][13], e.g. a loaded state_from_traj or workload.lemniscate_state) at equal spacing over [t0, t1]. The knot times
        become the table's times MINUS t0, so that trajectory time 0 is t0. period > 0 makes the table periodic and must then be the sampled span: float32(period) ==
        float32(t1 - t0), the last knot's time (ValueError otherwise)."""
        n = int(n)
        if n < 1 or not float(t1) >= float(t0):
            raise ValueError("Trajectory.from_function: n >= 1 and t1 >= t0 are required")
        ts = np.linspace(float(t0), float(t1), n) if n > 1 else np.array([float(t0)])
        x = np.asarray(state_fn(ts), np.float32).reshape(n, 13)
        t = (ts - float(t0)).astype(np.float32)
        if float(period) > 0 and np.float32(period) != t[-1]:
            raise ValueError(f"Trajectory.from_function: a periodic table spans one period: period = {float(period)} but t1 - t0 = {float(t[-1])} (in float32)")
        return cls(t, x, period)

    @classmethod
    def from_csv(cls, csv, n=None, period=0.0):
        """From a utils.TrajectoryCSV (its own samples as knots, times from its first sample; n given: n equally spaced samples of its interpolant). The CSV's
        state() forms the yaw quaternion and, for a file in NED, the frame flip: the table holds what state() returns."""
        if n is None:
            ts = np.asarray(csv.t, np.float64)
            return cls((ts - ts[0]).astype(np.float32), np.asarray(csv.state(ts), np.float32), period)
        return cls.from_function(csv.state, float(csv.t[0]), float(csv.t[-1]), n, period)

    def rows(self, u, phase=0.0, rate=1.0, offset=(0.0, 0.0, 0.0), renorm=True):
        """row(u) of SPEC.md §11j for clock values u f32[...] and ONE episode's (phase, rate, offset): f32[...][13], in the device's arithmetic."""
        F = np.float32
        u = np.asarray(u, F)
        rate, phase, offset = F(rate), F(phase), np.asarray(offset, F).reshape(3)
        t, x, L = self.t, self.x, self.t.shape[0]
        if L == 1:
            y = np.broadcast_to(x[0], u.shape + (13,)).copy()
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                tau = _fma32(rate, u, phase)
                if self.period > 0:
                    inv = F(1.0 / np.float64(self.period))
                    n = np.floor(tau * inv).astype(F)
                    tau = _fma32(-n, self.period, tau)
                tau = np.where(tau > t[0], tau, t[0]).astype(F)
                tau = np.where(tau < t[-1], tau, t[-1]).astype(F)
            i = np.clip(np.searchsorted(t, tau, side="right") - 1, 0, L - 2)       # the largest index in [0, L-2] with t[i] <= tau
            w = (1.0 / (t[1:].astype(np.float64) - t[:-1].astype(np.float64))).astype(F)
            a = ((tau - t[i]).astype(F) * w[i]).astype(F)
            y = _fma32(a[..., None], (x[i + 1] - x[i]).astype(F), x[i])
        y[..., 0:3] = y[..., 0:3] + offset
        y[..., 3:6] = y[..., 3:6] * rate
        y[..., 10:13] = y[..., 10:13] * rate
        if renorm:
            q0, q1, q2, q3 = y[..., 6], y[..., 7], y[..., 8], y[..., 9]
            r = _rsqrt32(_fma32(q3, q3, _fma32(q2, q2, _fma32(q1, q1, (q0 * q0).astype(F)))))
            y[..., 6:10] = y[..., 6:10] * r[..., None]
        return y

    def windows(self, time_steps, ticks, phase=0.0, rate=1.0, offset=(0.0, 0.0, 0.0), renorm=True):
        """Host restatement of what the device cuts for ONE episode: the reference windows f32[n][H+1][13] of the solves at the global ticks `ticks` int[n]
        (row i at u = float32(k) * float32(time_steps[0]) + c[i], c the float64 cumulative sum of time_steps cast once), for planning and plotting."""
        F = np.float32
        ts = np.asarray(time_steps, F)
        k = np.asarray(ticks, np.int64).reshape(-1)
        if k.size and (k.min() < 0 or k.max() >= 1 << 24):
            raise ValueError("Trajectory.windows: ticks must be in [0, 2^24)")
        c = np.concatenate([[0.0], np.cumsum(ts.astype(np.float64))]).astype(F)
        theta = (k.astype(F) * F(ts[0])).astype(F)
        return self.rows((theta[:, None] + c[None, :]).astype(F), phase, rate, offset, renorm)

    def targets(self, time_steps, ticks, phase=0.0, rate=1.0, offset=(0.0, 0.0, 0.0), renorm=True):
        """The score targets f32[n][13] of the ticks `ticks`: the row at u = float32(k + 1) * float32(time_steps[0])."""
        k = np.asarray(ticks, np.int64).reshape(-1) + 1
        return self.rows((k.astype(np.float32) * np.asarray(time_steps, np.float32)[0]).astype(np.float32), phase, rate, offset, renorm)

    def __repr__(self):
        return f"Trajectory(L={self.t.shape[0]}, t=[{float(self.t[0])}, {float(self.t[-1])}], period={float(self.period)})"


SCORE_DTYPE = np.dtype(_abi.SCORE_FIELDS)          # one episode's 16 score words (SPEC.md §11h), 64 bytes
SCORE_CAUSES = {"position": 1, "tilt": 2, "rate": 4, "nonfinite": 8}


def score_init(B):
    """The initial score rows of B episodes (what score_in=None means): zeros, min_cos_tilt = +inf, first_fail_row = 0xffffffff."""
    z = np.zeros(int(B), SCORE_DTYPE)
    z["min_cos_tilt"] = np.inf
    z["first_fail_row"] = 0xFFFFFFFF
    return z


def score_summary(score, solves=None):
    """Host convenience on the structured score array [B] that closed_loop(score=...) returns. A dict of
        success_rate      fraction of episodes without a failing row (first_fail_row all ones)
        rms_pos_err       f64[B], sqrt(sum_dp / rows) per episode (NaN for an episode without rows)
        worst_tilt_deg    the largest tilt of any episode: degrees(acos(min over episodes of min_cos_tilt, clipped to [-1, 1])); NaN if that minimum is
        mean_steps        optimiser iterations per solve, sum(sum_steps) / (B * solves)
        mean_ls_trials    line-search trials per solve, sum(sum_ls_trials) / (B * solves)
    The score words hold no solve count, so the last two need `solves`, the number of solves per episode over everything the score covers (Ns of every call
    the score was carried through, added up); without it they are None. Reductions across episodes stay on the host: B words per metric."""
    z = np.asarray(score)
    if z.dtype != SCORE_DTYPE or z.ndim != 1:
        raise ValueError(f"score_summary: expected the structured score array [B] of closed_loop(score=...), got dtype {z.dtype} and shape {z.shape}")
    B = z.shape[0]
    rows = z["rows"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rms = np.sqrt(z["sum_dp"].astype(np.float64) / rows)
        cmin = np.float64(z["min_cos_tilt"].min()) if B else np.float64(np.nan)
        if np.isnan(z["min_cos_tilt"]).any():
            cmin = np.float64(np.nan)
        tilt = np.degrees(np.arccos(np.clip(cmin, -1.0, 1.0)))
    out = dict(success_rate=float(np.mean(z["first_fail_row"] == 0xFFFFFFFF)) if B else float("nan"), rms_pos_err=rms, worst_tilt_deg=float(tilt),
               mean_steps=None, mean_ls_trials=None)
    if solves is not None:
        if int(solves) < 1:
            raise ValueError("score_summary: solves must be >= 1")
        out["mean_steps"] = float(z["sum_steps"].astype(np.float64).sum() / (B * int(solves)))
        out["mean_ls_trials"] = float(z["sum_ls_trials"].astype(np.float64).sum() / (B * int(solves)))
    return out


ENSEMBLE_CHANNELS = ("dp", "dv", "c", "w2")        # the device's channel order (SPEC.md §11m): squared position error, squared velocity error, tilt cosine, squared rate


class Ensemble:
    """What closed_loop(ensemble=...) reduces over the EPISODES, per scored row and cohort (SPEC.md §11m): counts, the survival curve, sum / min / max of the score's
    four channels and, per channel, cumulative counts against edges given here in the user's units — pos_edges [m], vel_edges [m/s], tilt_edges_deg [degrees],
    rate_edges [rad/s]. The device compares squares and a cosine, as the score does, so the edges are squared (or their cosine taken) in float64, rounded to float32
    ONCE and sorted ascending in the DEVICE's order; channels with fewer edges than the longest are filled up with +inf (every included finite value is below it).
    A tilt edge counts the episodes tilted MORE than the edge (c < cos(edge)), and the cosine sorts the tilt edges into DESCENDING degrees: tilt_edges_deg holds
    them in that device order. over="alive" includes an episode in a row's statistics only while it has not failed before that row; over="all" every finite row.
    n_cohorts (1 .. 16; None: taken from the cohort array of the call, max + 1) lets a cohort be empty."""

    def __init__(self, pos_edges=(), vel_edges=(), tilt_edges_deg=(), rate_edges=(), over="alive", n_cohorts=None):
        if over not in ("alive", "all"):
            raise ValueError('Ensemble: over must be "alive" or "all"')
        if n_cohorts is not None and not (1 <= int(n_cohorts) <= 16):
            raise ValueError("Ensemble: n_cohorts must be between 1 and 16")
        self.over, self.n_cohorts = over, None if n_cohorts is None else int(n_cohorts)
        user = [np.atleast_1d(np.asarray(e, np.float64)).ravel() for e in (pos_edges, vel_edges, tilt_edges_deg, rate_edges)]
        for name, e in zip(("pos_edges", "vel_edges", "tilt_edges_deg", "rate_edges"), user):
            if np.isnan(e).any() or (e < 0).any():
                raise ValueError(f"Ensemble: {name} must hold values >= 0 (and no NaN)")
        if (user[2] > 180.0).any():
            raise ValueError("Ensemble: tilt_edges_deg must lie in [0, 180]")
        self.pos_edges, self.vel_edges, self.rate_edges = (np.sort(e) for e in (user[0], user[1], user[3]))
        self.tilt_edges_deg = np.sort(user[2])[::-1].copy()
        with np.errstate(over="ignore"):
            dev = [np.float32(self.pos_edges * self.pos_edges), np.float32(self.vel_edges * self.vel_edges), np.float32(np.cos(np.radians(self.tilt_edges_deg))),
                   np.float32(self.rate_edges * self.rate_edges)]
        self.counts = tuple(int(d.size) for d in dev)            # edges per channel that the caller gave
        self.n_edges = max(self.counts)
        if self.n_edges > 16:
            raise ValueError("Ensemble: at most 16 edges per channel")
        self.edges = np.full((4, self.n_edges), np.inf, np.float32)
        for k, d in enumerate(dev):
            self.edges[k, :d.size] = np.sort(d)                   # (rounding keeps the order; equal neighbours are allowed)
        self.words = _abi.ENSEMBLE_BASE_WORDS + 4 * self.n_edges

    @classmethod
    def from_device_edges(cls, edges, over="alive", n_cohorts=None):
        """An Ensemble whose edges are given as the device compares them: f32[4][E] for (dp, dv, c, w2) — squared metres, squared m/s, a cosine, squared rad/s —
        each row ascending, no NaN. For edges derived from a Score's own thresholds (Score.thresholds()) or from recorded channel values; the user-unit edges are
        their square roots and arc cosines."""
        e = np.ascontiguousarray(edges, np.float32)
        if e.ndim != 2 or e.shape[0] != 4 or e.shape[1] > 16 or np.isnan(e).any() or (e[:, 1:] < e[:, :-1]).any():
            raise ValueError("Ensemble.from_device_edges: edges must be f32[4][E], E <= 16, every row ascending, no NaN")
        self = cls(over=over, n_cohorts=n_cohorts)
        with np.errstate(invalid="ignore"):
            self.pos_edges, self.vel_edges, self.rate_edges = (np.sqrt(e[k].astype(np.float64)) for k in (0, 1, 3))
            self.tilt_edges_deg = np.degrees(np.arccos(np.clip(e[2].astype(np.float64), -1.0, 1.0)))
        self.counts, self.n_edges, self.edges = (e.shape[1],) * 4, e.shape[1], e
        self.words = _abi.ENSEMBLE_BASE_WORDS + 4 * self.n_edges
        return self

    def __repr__(self):
        return (f"Ensemble(pos_edges={self.pos_edges.tolist()}, vel_edges={self.vel_edges.tolist()}, tilt_edges_deg={self.tilt_edges_deg.tolist()}, "
                f"rate_edges={self.rate_edges.tolist()}, over={self.over!r}, n_cohorts={self.n_cohorts})")


def ensemble_summary(words, ensemble, quantiles=(0.5, 0.9)):
    """Host arithmetic on the word array u32[R][G][W] that closed_loop(ensemble=...) returns (SPEC.md §11m), per scored row and cohort, float64[R][G] unless said
    otherwise (NaN where a ratio has an empty denominator):
        n, n_in           episodes of the cohort, episodes included in the statistics (int64)
        survival          1 - (episodes failed by this row) / n
        fail_now          (episodes whose row violates a criterion) / n;  fail_now_by_cause: the same per SCORE_CAUSES name
        rms_pos, rms_vel  sqrt(sum / n_in) of the squared position / velocity error over the included episodes
        mean_cos_tilt, rms_rate   sum / n_in of the tilt cosine, sqrt(sum / n_in) of the squared rate
        min_pos, max_pos, min_vel, max_vel, min_rate, max_rate   square roots of the extrema;  min_tilt_deg, max_tilt_deg from the largest / smallest cosine
        cdf_pos, cdf_vel, cdf_rate   [R][G][edges given]: fraction of the included episodes BELOW each edge;  frac_tilt_above: fraction tilted MORE than each
                          tilt edge (in the order of ensemble.tilt_edges_deg)
        q_pos, q_vel, q_tilt_deg, q_rate   [R][G][len(quantiles)]: the smallest edge below which (for tilt: at or below which) at least that fraction of the
                          included episodes lies — an upper estimate no finer than the edges; NaN where no edge reaches the level."""
    w = np.ascontiguousarray(words)
    if not isinstance(ensemble, Ensemble):
        raise ValueError("ensemble_summary: ensemble must be the Ensemble the words were formed with")
    if w.dtype != np.uint32 or w.ndim != 3 or w.shape[2] != ensemble.words:
        raise ValueError(f"ensemble_summary: words must be uint32[R][G][{ensemble.words}], got dtype {w.dtype} and shape {w.shape}")
    E = ensemble.n_edges
    n, n_in = w[..., 0].astype(np.int64), w[..., 1].astype(np.int64)
    fl = w[..., 8:20].view(np.float32).astype(np.float64).reshape(w.shape[0], w.shape[1], 4, 3)
    out = {"n": n, "n_in": n_in}
    with np.errstate(invalid="ignore", divide="ignore"):
        nf, ni = n.astype(np.float64), n_in.astype(np.float64)
        out["survival"] = 1.0 - w[..., 2] / nf
        out["fail_now"] = w[..., 3] / nf
        out["fail_now_by_cause"] = {name: w[..., 4 + i] / nf for i, name in enumerate(SCORE_CAUSES)}
        mean = fl[..., 0] / ni[..., None]
        out["rms_pos"], out["rms_vel"], out["mean_cos_tilt"], out["rms_rate"] = np.sqrt(mean[..., 0]), np.sqrt(mean[..., 1]), mean[..., 2], np.sqrt(mean[..., 3])
        empty = n_in == 0
        for k, name in ((0, "pos"), (1, "vel"), (3, "rate")):
            out["min_" + name] = np.where(empty, np.nan, np.sqrt(fl[..., k, 1]))
            out["max_" + name] = np.where(empty, np.nan, np.sqrt(fl[..., k, 2]))
        out["min_tilt_deg"] = np.where(empty, np.nan, np.degrees(np.arccos(np.clip(fl[..., 2, 2], -1.0, 1.0))))
        out["max_tilt_deg"] = np.where(empty, np.nan, np.degrees(np.arccos(np.clip(fl[..., 2, 1], -1.0, 1.0))))
        cnt = w[..., 20:].reshape(w.shape[0], w.shape[1], 4, E).astype(np.float64) / ni[..., None, None]
        levels = np.atleast_1d(np.asarray(quantiles, np.float64))
        for k, name, edges in ((0, "pos", ensemble.pos_edges), (1, "vel", ensemble.vel_edges), (3, "rate", ensemble.rate_edges)):
            cdf = cnt[..., k, :edges.size]
            out["cdf_" + name] = cdf
            out["q_" + name] = _edge_quantiles(cdf, edges, levels)
        above = cnt[..., 2, :ensemble.tilt_edges_deg.size]
        out["frac_tilt_above"] = above
        out["q_tilt_deg"] = _edge_quantiles((1.0 - above)[..., ::-1], ensemble.tilt_edges_deg[::-1], levels)
    return out


def retire_summary(retired_at, live, B):
    """Host arithmetic on the two arrays closed_loop(retire=True) returns (SPEC.md §11n): retired_at int32[B] and live int32[Ns]. Returns a dict: "solves_run"
    sum(live), "solves_saved" B * Ns - sum(live), "saved_share" their ratio to B * Ns (0 for an empty call), "retired" the episodes with retired_at >= 0 and
    "retired_at_entry" those with retired_at == 0."""
    r, l, B = np.asarray(retired_at), np.asarray(live), int(B)
    if r.dtype.kind not in "iu" or r.shape != (B,):
        raise ValueError(f"retire_summary: retired_at must be int[{B}], got dtype {r.dtype} and shape {r.shape}")
    if l.dtype.kind not in "iu" or l.ndim != 1 or (l.size and (l.min() < 0 or l.max() > B)):
        raise ValueError(f"retire_summary: live must be int[Ns] with entries in [0, {B}]")
    total, run = B * int(l.size), int(l.astype(np.int64).sum())
    return {"solves_run": run, "solves_saved": total - run, "saved_share": (total - run) / total if total else 0.0,
            "retired": int((r >= 0).sum()), "retired_at_entry": int((r == 0).sum())}


def _edge_quantiles(cdf, edges, levels):
    """[..][len(levels)]: the smallest of the ascending edges whose cumulative fraction cdf[.., j] reaches each level; NaN where none does (or the cdf is NaN)."""
    out = np.full(cdf.shape[:-1] + (levels.size,), np.nan)
    for i, q in enumerate(levels):
        hit = cdf >= q
        first = np.argmax(hit, axis=-1) if edges.size else np.zeros(cdf.shape[:-1], np.int64)
        if edges.size:
            out[..., i] = np.where(hit.any(axis=-1), edges[first], np.nan)
    return out


class _TubeFields(NamedTuple):
    cost: np.ndarray
    mean: np.ndarray
    var: np.ndarray
    min: np.ndarray
    max: np.ndarray
    outside: np.ndarray


class Tube(_TubeFields):
    """The predicted tube of a rollout (SPEC.md §12), a named tuple (cost, mean, var, min, max, outside): per step t and state component i, over the P
    particles. cost is f32[B]; mean, var, min, max are f32[B][H+1][13]; outside is uint32[B][H+1][13], the number of particles outside [lo_i, hi_i] (a NaN
    counts). The particle count rides along as the attribute P (not a field): Tube.of(P, ...) sets it, and a Tube made any other way (the constructor,
    _replace, _make) has none — p_outside then refuses instead of dividing by a guess."""
    P = None

    @classmethod
    def of(cls, P, *planes):
        t = cls(*planes)
        t.P = int(P)
        return t

    def _replace(self, **kw):
        t = super()._replace(**kw)
        t.P = self.P                      # (the particle count of the tube the planes came from)
        return t

    @property
    def std(self):
        """sqrt of the population variance, float32"""
        return np.sqrt(self.var, dtype=np.float32)

    @property
    def p_outside(self):
        """outside / P: the empirical probability of leaving the bounds, per step and component"""
        if self.P is None:
            raise ValueError("Tube.p_outside: this Tube carries no particle count (build it with Tube.of(P, ...))")
        return self.outside / self.P


class _RiskFields(NamedTuple):
    cost: np.ndarray
    exit: object
    jx: object
    first_exit: object
    outside_any: object
    jstat: np.ndarray
    jq: object
    jtail: object


class Risk(_RiskFields):
    """Predicted risk of a rollout (SPEC.md §12a), a named tuple (cost, exit, jx, first_exit, outside_any, jstat, jq, jtail). cost f32[B] is the rollout's
    expected cost. exit uint32[B][P] (first step outside the box, H+1: never) and jx f32[B][P] (tracking cost per particle) are None unless asked for
    (want_particles). first_exit uint32[B][H+2] is the histogram of exit (bin H+1: never), outside_any uint32[B][H+1] the particles outside at each step — both None
    without bounds. jstat f32[B][4]: mean, population variance, min, max of jx. jq f32[B][Q]: the quantiles asked for; jtail f32[B]: the mean of the tail (CVaR);
    None when not asked for. The particle count rides along as the attribute P (Risk.of sets it), as on Tube."""
    P = None

    @classmethod
    def of(cls, P, *fields):
        r = cls(*fields)
        r.P = int(P)
        return r

    def _replace(self, **kw):
        r = super()._replace(**kw)
        r.P = self.P
        return r

    def _need(self, what):
        if self.P is None:
            raise ValueError(f"Risk.{what}: this Risk carries no particle count (build it with Risk.of(P, ...))")
        if self.first_exit is None:
            raise ValueError(f"Risk.{what}: no bounds were given, so there is no exit histogram")

    @property
    def p_ever(self):
        """1 - first_exit[..., H+1] / P: the empirical probability that a particle EVER leaves the box within the horizon"""
        self._need("p_ever")
        return 1.0 - self.first_exit[..., -1] / self.P

    @property
    def survival(self):
        """[..., H+1]: the fraction of particles that have not left the box up to and including step t"""
        self._need("survival")
        return 1.0 - np.cumsum(self.first_exit[..., :-1], axis=-1) / self.P


def quantile_ranks(quantiles, P):
    """SPEC.md §12a: quantile q -> rank ceil(q P) - 1, clamped to [0, P-1] (rank 0: the smallest)"""
    import math
    return [min(P - 1, max(0, math.ceil(float(q) * P) - 1)) for q in quantiles]


def band_keys(v):
    """SPEC.md §12b: the uint32 key of every float32 word of v — -inf < ... < -0 < +0 < ... < +inf < NaN as unsigned integers, all NaNs one key"""
    v = np.ascontiguousarray(v, np.float32)
    u = v.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


class _BandsFields(NamedTuple):
    cost: np.ndarray
    q: object
    below: object
    at: object


class Bands(_BandsFields):
    """Predicted bands of a rollout (SPEC.md §12b), a named tuple (cost, q, below, at). cost f32[B] is the rollout's expected cost. q f32[B][Q][H+1][13]:
    plane k is, per step and state component, the value at rank ranks[k] of the key order over the P particles (None when no rank was asked for). below, at
    uint32[B][H+1][13]: how many particles lie below / at the observed value (None without `observed`). The particle count P, the ranks, the quantiles they
    came from (None when ranks were given directly) and the observed rows ride along as attributes: Bands.of sets them."""
    P = None
    ranks = None
    quantiles = None
    observed = None

    @classmethod
    def of(cls, P, ranks, quantiles, observed, *fields):
        r = cls(*fields)
        r.P, r.ranks, r.quantiles, r.observed = int(P), (None if ranks is None else tuple(int(k) for k in ranks)), (None if quantiles is None else tuple(quantiles)), observed
        return r

    def _replace(self, **kw):
        r = super()._replace(**kw)
        r.P, r.ranks, r.quantiles, r.observed = self.P, self.ranks, self.quantiles, self.observed
        return r

    def band(self, k):
        """plane k of q: [..., H+1, 13]"""
        if self.q is None:
            raise ValueError("Bands.band: no rank was asked for")
        return self.q[..., k, :, :]

    @property
    def median(self):
        """the plane of quantile 0.5; only when 0.5 was among the quantiles asked for"""
        if self.quantiles is None or 0.5 not in self.quantiles:
            raise ValueError("Bands.median: 0.5 was not among the quantiles asked for")
        return self.band(self.quantiles.index(0.5))

    def _need_obs(self, what):
        if self.below is None or self.at is None or self.observed is None or self.P is None:
            raise ValueError(f"Bands.{what}: no observed rows were given (or this Bands was not built with Bands.of)")

    @property
    def pit(self):
        """(below + at / 2) / P in float64: the mid-rank of the observed value in the predicted distribution (the PIT value); NaN where the observation was NaN"""
        self._need_obs("pit")
        v = (self.below.astype(np.float64) + 0.5 * self.at.astype(np.float64)) / self.P
        return np.where(np.isnan(self.observed), np.nan, v)

    def inside(self, k_lo, k_hi):
        """boolean plane: key(q[k_lo]) <= key(observed) <= key(q[k_hi]); False where the observation was NaN"""
        self._need_obs("inside")
        ko = band_keys(self.observed)
        ok = (band_keys(self.band(k_lo)) <= ko) & (ko <= band_keys(self.band(k_hi)))
        return ok & ~np.isnan(self.observed)


def calibration(bands, bins=10, levels=(0.5, 0.9)):
    """Calibration table from one Bands or a list of them (every instance of every one is a sample; all of one horizon). Per horizon step and component:
    `hist` int64[H+1][13][bins], the histogram of the PIT values over the samples (bin j: j / bins <= pit < (j + 1) / bins, pit = 1 in the last);
    `n` int64[H+1][13], the samples counted — columns whose observation was NaN are left out; `coverage` float64[len(levels)][H+1][13], the fraction of samples
    with |pit - 1/2| <= level / 2 (the central interval of that nominal level; NaN where n = 0); `levels` as given. A calibrated model has a flat histogram and
    coverage equal to the level; coverage above it says the model's sigma is too wide."""
    if isinstance(bands, Bands):
        bands = [bands]
    pit = np.concatenate([np.asarray(b.pit, np.float64).reshape((-1,) + b.pit.shape[-2:]) for b in bands], axis=0)
    ok = ~np.isnan(pit)
    n = ok.sum(axis=0).astype(np.int64)
    idx = np.clip(np.floor(np.where(ok, pit, 0.0) * bins).astype(np.int64), 0, bins - 1)
    hist = np.zeros(pit.shape[1:] + (bins,), np.int64)
    for j in range(bins):
        hist[..., j] = ((idx == j) & ok).sum(axis=0)
    cov = np.full((len(levels),) + pit.shape[1:], np.nan, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, lv in enumerate(levels):
            hit = (np.abs(np.where(ok, pit, np.inf) - 0.5) <= 0.5 * float(lv)).sum(axis=0)
            cov[i] = np.where(n > 0, hit / np.maximum(n, 1), np.nan)
    return {"hist": hist, "n": n, "coverage": cov, "levels": tuple(float(v) for v in levels), "bins": int(bins)}


class _OutcomeFields(NamedTuple):
    cost: np.ndarray
    words: object
    fail_step: np.ndarray
    first_fail: np.ndarray
    cause_ever: np.ndarray
    chan_stat: np.ndarray
    chan_q: object
    agg_stat: np.ndarray
    agg_q: object


OUTCOME_CHANNELS = ("dp", "dv", "c", "w2")                # chan_stat / chan_q: squared position error, squared velocity error, tilt cosine, squared body rate
OUTCOME_AGGREGATES = ("sum_dp", "max_dp", "min_c", "max_w2")      # agg_stat / agg_q: score words 1, 2, 6, 7 of each particle


class Outcome(_OutcomeFields):
    """Predicted outcome of a rollout (SPEC.md §12c): every particle scored as closed_loop(score=...) scores an episode (§11h), a named tuple (cost, words,
    fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat, agg_q). cost f32[B] is the rollout's expected cost. words uint32[B][P][11] (words 0 .. 10
    of the score table per particle) is None unless asked for (want_particles). fail_step uint32[B][H][5]: particles failing at row r = t - 1 by cause
    (radius, tilt, rate, non-finite) and by any; first_fail uint32[B][H+1]: histogram of the first failing row, slot H: never; cause_ever uint32[B][4].
    chan_stat f32[B][H][4][3]: mean, min, max per row of the channels OUTCOME_CHANNELS; agg_stat f32[B][4][3] the same over OUTCOME_AGGREGATES. chan_q
    f32[B][H][4][K], agg_q f32[B][4][K]: the order statistics at `ranks` (None when none were asked for). The particle count, the ranks and the quantiles
    they came from ride along as attributes (Outcome.of sets them)."""
    P = None
    ranks = None
    quantiles = None

    @classmethod
    def of(cls, P, ranks, quantiles, *fields):
        r = cls(*fields)
        r.P, r.ranks, r.quantiles = int(P), None if ranks is None else tuple(ranks), None if quantiles is None else tuple(quantiles)
        return r

    def _replace(self, **kw):
        r = super()._replace(**kw)
        r.P, r.ranks, r.quantiles = self.P, self.ranks, self.quantiles
        return r

    def _need(self, what, field="first_fail"):
        if self.P is None:
            raise ValueError(f"Outcome.{what}: this Outcome carries no particle count (build it with Outcome.of(P, ...))")
        if getattr(self, field) is None:
            raise ValueError(f"Outcome.{what}: {field} was not computed")

    @property
    def p_fail(self):
        """1 - first_fail[..., H] / P: the predicted probability that the score's criteria fail somewhere within the horizon"""
        self._need("p_fail")
        return 1.0 - self.first_fail[..., -1] / self.P

    @property
    def survival(self):
        """[..., H]: the fraction of particles that have not failed up to and including row r (state x_{r+1})"""
        self._need("survival")
        return 1.0 - np.cumsum(self.first_fail[..., :-1], axis=-1) / self.P

    @property
    def p_cause(self):
        """[..., 4]: the fraction of particles that ever fail by radius, tilt, rate, non-finite (SCORE_CAUSES); they overlap"""
        self._need("p_cause", "cause_ever")
        return self.cause_ever / self.P

    def pos_err(self, k):
        """[..., H]: sqrt of order statistic k of dp per row — the position error [m] at rank ranks[k] (sqrt is increasing: the rank carries over)"""
        self._need("pos_err", "chan_q")
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.chan_q[..., 0, k].astype(np.float64))

    def tilt_deg(self, k):
        """[..., H]: the tilt [deg] of order statistic k of the tilt cosine c per row. arccos is DEcreasing: rank ranks[k] of c is rank P - 1 - ranks[k] of the
        tilt, so the 95 % tilt comes from the 5 % quantile of c."""
        self._need("tilt_deg", "chan_q")
        with np.errstate(invalid="ignore"):
            return np.degrees(np.arccos(np.clip(self.chan_q[..., 2, k].astype(np.float64), -1.0, 1.0)))


def tail_count(tail, P):
    """SPEC.md §12a: a fraction alpha -> max(1, ceil(alpha P)); an integer is the count itself"""
    import math
    if isinstance(tail, (int, np.integer)) and not isinstance(tail, bool):
        return int(tail)
    return max(1, math.ceil(float(tail) * P))


class SdeMpcSolver:
    """One solver handle = one (MPC config, model). Single-threaded, like the reference's solver
    objects (one blocking call at a time, sde_control.py:420)."""

    def __init__(self, mpc_cfg, model, max_batch: int = 1, device: int = 0, options=None, lib_path=None):
        self.lib = _abi.load_library(lib_path)          # lib_path: another build of libsdempc.so for this handle alone (A/B runs in one process)
        self.cfg_py = mpc_cfg
        self.cfg, self._keep = mpc_cfg.to_cfg()
        blob = model.to_blob() if hasattr(model, "to_blob") else bytes(model)
        self._blob = C.create_string_buffer(blob, len(blob))
        self.H, self.P, self.m = mpc_cfg.horizon, mpc_cfg.num_particles, mpc_cfg.num_motors
        self.max_batch = int(max_batch)
        h = C.c_void_p()
        rc = self.lib.sdempc_create(C.byref(self.cfg), self._blob, len(blob), self.max_batch, C.byref(h))
        if rc != 0:
            raise SdempcError(f"sdempc_create failed ({rc}): {self.lib.sdempc_last_error(None).decode()}")
        self._h = h
        if device:
            self._check(self.lib.sdempc_set_device(self._h, int(device)))
        for k, v in (options or {}).items():
            self.set_option(k, v)

    # ---- execution options (include/sdempc.h SDEMPC_OPT_*): layout choices, never a bit of the results ----
    def set_option(self, name: str, value: int):
        self._check(self.lib.sdempc_set_option(self._h, _abi.OPTIONS[name], int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int32()
        self._check(self.lib.sdempc_get_option(self._h, _abi.OPTIONS[name], C.byref(v)))
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.sdempc_destroy(self._h)
            self._h = None

    def detach(self):
        """Forget the handle WITHOUT destroying it: for a handle inherited through fork(), whose HIP objects belong to the parent's
        context (sdempc_destroy would call hipFree / hipStreamDestroy on it). The few host bytes are leaked on purpose."""
        self._h = None

    def device_ready(self) -> bool:
        """Has this handle initialised the GPU (device buffers, stream)? Host-only query."""
        return bool(getattr(self, "_h", None)) and bool(self.lib.sdempc_device_ready(self._h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SdempcError(f"sdempc error {rc}: {self.lib.sdempc_last_error(self._h).decode()}")

    # ---- m_reset ------------------------------------------------------------------------------
    def reset(self, x=None, xdes=None):
        x = _f32(np.zeros(13) if x is None else x, (13,))
        xdes = _f32(x if xdes is None else xdes, (13,))
        yk = np.zeros((self.H, self.m), np.float32)
        info = SdempcInfo()
        self._check(self.lib.sdempc_reset(self._h, _fp(x), _fp(xdes), _fp(yk), C.byref(info)))
        return yk, {k: getattr(info, k) for k in INFO_FIELDS}

    # ---- batched host-pointer entry points ------------------------------------------------------
    def rollout(self, x0, u, xref, noise, want_traj=False, want_mean=False):
        x0 = _f32(x0)
        B = x0.shape[0]
        x0, u = _f32(x0, (B, 13)), _f32(u, (B, self.H, self.m))
        xref, noise = _f32(xref, (B, self.H + 1, 13)), _f32(noise, (B, self.P, self.H, 6))
        cost = np.zeros(B, np.float32)
        traj = np.zeros((B, self.P, self.H + 1, 13), np.float32) if want_traj else None
        mean = np.zeros((B, self.H + 1, 13), np.float32) if want_mean else None
        self._check(self.lib.sdempc_rollout_batch(self._h, B, _fp(x0), _fp(u), _fp(xref), _fp(noise), _fp(cost),
                                                  _fp(traj) if want_traj else None, _fp(mean) if want_mean else None))
        return cost, traj, mean

    def grad(self, x0, u, xref, noise):
        x0 = _f32(x0)
        B = x0.shape[0]
        x0, u = _f32(x0, (B, 13)), _f32(u, (B, self.H, self.m))
        xref, noise = _f32(xref, (B, self.H + 1, 13)), _f32(noise, (B, self.P, self.H, 6))
        cost = np.zeros(B, np.float32)
        g = np.zeros((B, self.H, self.m), np.float32)
        self._check(self.lib.sdempc_grad_batch(self._h, B, _fp(x0), _fp(u), _fp(xref), _fp(noise), _fp(cost), _fp(g)))
        return cost, g

    def solve(self, x0, xref, noise, u_init, stepsize_in):
        x0 = _f32(x0)
        B = x0.shape[0]
        x0, u_init = _f32(x0, (B, 13)), _f32(u_init, (B, self.H, self.m))
        xref, noise = _f32(xref, (B, self.H + 1, 13)), _f32(noise, (B, self.P, self.H, 6))
        stepsize_in = _f32(stepsize_in, (B,))
        uopt = np.zeros((B, self.H, self.m), np.float32)
        xevol = np.zeros((B, self.H + 1, 13), np.float32)
        info = (SdempcInfo * B)()
        self._check(self.lib.sdempc_solve_batch(self._h, B, _fp(x0), _fp(xref), _fp(noise), _fp(u_init), _fp(stepsize_in),
                                                _fp(uopt), _fp(xevol), info))
        info_np = np.frombuffer(info, dtype=np.float32).reshape(B, 8).copy()
        return uopt, xevol, info_np

    # ---- key-derived noise (SPEC.md §7): keys uint32[B][2], JAX threefry conventions ------------------
    @staticmethod
    def _keys(keys, B=None):
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        if k.ndim != 2 or k.shape[1] != 2 or (B is not None and k.shape[0] != B):
            raise ValueError(f"keys must be uint32[B][2], got {k.shape}")
        return k

    def solve_keys(self, x0, xref, keys, u_init, stepsize_in):
        """m_mpc's mapping: the noise of instance b is normal(keys[b], (P, H, 6)), drawn on the device."""
        x0 = _f32(x0)
        B = x0.shape[0]
        x0, u_init = _f32(x0, (B, 13)), _f32(u_init, (B, self.H, self.m))
        xref, keys, stepsize_in = _f32(xref, (B, self.H + 1, 13)), self._keys(keys, B), _f32(stepsize_in, (B,))
        uopt = np.zeros((B, self.H, self.m), np.float32)
        xevol = np.zeros((B, self.H + 1, 13), np.float32)
        info = (SdempcInfo * B)()
        self._check(self.lib.sdempc_solve_batch_keys(self._h, B, _fp(x0), _fp(xref), keys.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                     _fp(u_init), _fp(stepsize_in), _fp(uopt), _fp(xevol), info))
        return uopt, xevol, np.frombuffer(info, dtype=np.float32).reshape(B, 8).copy()

    # ---- predicted tube (SPEC.md §12): per-step particle spread and bound exceedance, reduced on the device ----
    @staticmethod
    def _tube_cfg(lo, hi):
        """lo / hi: 13 values each, None: no bound on any component (-inf / +inf)"""
        cfg = _abi.SdempcTubeCfg()
        cfg.struct_size = C.sizeof(_abi.SdempcTubeCfg)
        lo = _f32(np.full(13, -np.inf) if lo is None else lo, (13,))
        hi = _f32(np.full(13, np.inf) if hi is None else hi, (13,))
        for i in range(13):
            cfg.lo[i], cfg.hi[i] = float(lo[i]), float(hi[i])
        return cfg

    def _tube_call(self, fn, x0, u, xref, draw, lo, hi):
        B = x0.shape[0]
        x0, u, xref = _f32(x0, (B, 13)), _f32(u, (B, self.H, self.m)), _f32(xref, (B, self.H + 1, 13))
        cfg = self._tube_cfg(lo, hi)
        cost = np.zeros(B, np.float32)
        mean, var, mn, mx = (np.zeros((B, self.H + 1, 13), np.float32) for _ in range(4))
        outside = np.zeros((B, self.H + 1, 13), np.uint32)
        self._check(fn(self._h, C.byref(cfg), B, _fp(x0), _fp(u), _fp(xref), draw, _fp(cost), _fp(mean), _fp(var), _fp(mn), _fp(mx),
                       outside.ctypes.data_as(C.POINTER(C.c_uint32))))
        return Tube.of(self.P, cost, mean, var, mn, mx, outside)

    def tube(self, x0, u, xref, noise, lo=None, hi=None) -> Tube:
        """One rollout of u per instance with its particle x horizon tensor reduced on the device: Tube(cost, mean, var, min, max, outside). mean is the
        rollout's xmean bit for bit; outside counts the particles outside [lo_i, hi_i] (13 values each, default: no bound — then only NaNs count)."""
        x0 = _f32(x0)
        noise = _f32(noise, (x0.shape[0], self.P, self.H, 6))
        return self._tube_call(_abi.tube_entries(self.lib)[0], x0, u, xref, _fp(noise), lo, hi)

    def tube_keys(self, x0, u, xref, keys, lo=None, hi=None) -> Tube:
        """tube() with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as solve_keys draws it."""
        x0 = _f32(x0)
        keys = self._keys(keys, x0.shape[0])
        return self._tube_call(_abi.tube_entries(self.lib)[1], x0, u, xref, keys.ctypes.data_as(C.POINTER(C.c_uint32)), lo, hi)

    def tube_dev(self, B, mean, var, min, max, outside=None, lo=None, hi=None, stream=0):
        """Device pointers (each may be None): reduces the tensor the last rollout_dev(store_traj=True) of at least B instances left in the handle into
        f32[B][H+1][13] planes (outside: uint32). Refused after a grad_dev, a solve_dev or a smaller rollout, as traj_to_canonical_dev is."""
        cfg = self._tube_cfg(lo, hi) if (outside is not None or lo is not None or hi is not None) else None
        self._check(_abi.tube_entries(self.lib)[2](self._h, C.byref(cfg) if cfg is not None else None, B, mean, var, min, max, outside, C.c_void_p(stream)))

    # ---- predicted risk (SPEC.md §12a): joint exit probability and tracking-cost tail, reduced on the device ----
    def _risk_cfg(self, centre, tail, quantiles):
        """-> (cfg, centre rows or None). centre: None (absolute box), "xref", "mean", or rows [B][H+1][13]"""
        cfg = _abi.SdempcRiskCfg()
        cfg.struct_size = C.sizeof(_abi.SdempcRiskCfg)
        rows = None
        if centre is None:
            cfg.centre_mode = 0
        elif isinstance(centre, str):
            if centre not in ("xref", "mean"):
                raise ValueError('centre: None, "xref", "mean" or an array [B][H+1][13]')
            cfg.centre_mode = 2 if centre == "xref" else 3
        else:
            cfg.centre_mode, rows = 1, centre
        if tail is not None:
            cfg.tail_k = tail_count(tail, self.P)
        if quantiles is not None:
            ranks = quantile_ranks(quantiles, self.P)
            if not 1 <= len(ranks) <= _abi.RISK_MAX_RANKS:
                raise ValueError(f"quantiles: 1 to {_abi.RISK_MAX_RANKS} values")
            cfg.n_ranks = len(ranks)
            for k, r in enumerate(ranks):
                cfg.ranks[k] = r
        return cfg, rows

    @staticmethod
    def _bounds(b, B, fill):
        """a bound: None (none on any component), [13] (broadcast over the batch) or [B][13]"""
        a = np.full(13, fill, np.float32) if b is None else np.asarray(b, np.float32)
        return np.ascontiguousarray(np.broadcast_to(a, (B, 13)), np.float32)

    def _risk_call(self, fn, x0, u, xref, draw, lo, hi, centre, tail, quantiles, want_particles):
        B = x0.shape[0]
        H, P = self.H, self.P
        x0, u, xref = _f32(x0, (B, 13)), _f32(u, (B, H, self.m)), _f32(xref, (B, H + 1, 13))
        cfg, rows = self._risk_cfg(centre, tail, quantiles)
        bounded = lo is not None or hi is not None
        lo_a, hi_a = (self._bounds(lo, B, -np.inf), self._bounds(hi, B, np.inf)) if bounded else (None, None)
        rows = _f32(rows, (B, H + 1, 13)) if rows is not None else None
        u32p = C.POINTER(C.c_uint32)
        cost = np.zeros(B, np.float32)
        ex = np.zeros((B, P), np.uint32) if want_particles and bounded else None
        jx = np.zeros((B, P), np.float32) if want_particles else None
        first = np.zeros((B, H + 2), np.uint32) if bounded else None
        anyo = np.zeros((B, H + 1), np.uint32) if bounded else None
        jstat = np.zeros((B, 4), np.float32)
        jq = np.zeros((B, cfg.n_ranks), np.float32) if cfg.n_ranks else None
        jtail = np.zeros(B, np.float32) if tail is not None else None
        f = lambda a: _fp(a) if a is not None else None
        w = lambda a: a.ctypes.data_as(u32p) if a is not None else None
        self._check(fn(self._h, C.byref(cfg), B, _fp(x0), _fp(u), _fp(xref), draw, f(lo_a), f(hi_a), f(rows), _fp(cost), w(ex), f(jx), w(first), w(anyo),
                       _fp(jstat), f(jq), f(jtail)))
        return Risk.of(P, cost, ex, jx, first, anyo, jstat, jq, jtail)

    def risk(self, x0, u, xref, noise, lo=None, hi=None, centre=None, tail=None, quantiles=None, want_particles=False) -> Risk:
        """One rollout of u per instance with its particle x horizon tensor reduced on the device to trajectory-level statistics (SPEC.md §12a): Risk(cost, exit,
        jx, first_exit, outside_any, jstat, jq, jtail). lo / hi: the box, [13] (broadcast) or [B][13], around `centre`: None (absolute), "xref", "mean" (the
        particle mean) or rows [B][H+1][13]. tail: a fraction alpha (k = max(1, ceil(alpha P))) or an integer k of worst particles; quantiles: up to 8 values
        in [0, 1] (rank ceil(q P) - 1). want_particles: also the per-particle planes exit and jx."""
        x0 = _f32(x0)
        noise = _f32(noise, (x0.shape[0], self.P, self.H, 6))
        return self._risk_call(_abi.risk_entries(self.lib)[0], x0, u, xref, _fp(noise), lo, hi, centre, tail, quantiles, want_particles)

    def risk_keys(self, x0, u, xref, keys, lo=None, hi=None, centre=None, tail=None, quantiles=None, want_particles=False) -> Risk:
        """risk() with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as solve_keys draws it."""
        x0 = _f32(x0)
        keys = self._keys(keys, x0.shape[0])
        return self._risk_call(_abi.risk_entries(self.lib)[1], x0, u, xref, keys.ctypes.data_as(C.POINTER(C.c_uint32)), lo, hi, centre, tail, quantiles,
                               want_particles)

    def risk_dev(self, B, xref=None, lo=None, hi=None, centre=None, tail=None, quantiles=None, exit=None, jx=None, first_exit=None, outside_any=None, jstat=None,
                 jq=None, jtail=None, stream=0):
        """Device pointers (each may be None): reduces the tensor the last rollout_dev(store_traj=True) of at least B instances left in the handle. lo / hi:
        pointers to f32[B][13]; centre: None, "xref", "mean" or a pointer to f32[B][H+1][13]; xref: pointer to f32[B][H+1][13] (for jx, jstat, jq, jtail and
        centre="xref"). Outputs: exit u32[B][P], jx f32[B][P], first_exit u32[B][H+2], outside_any u32[B][H+1], jstat f32[B][4], jq f32[B][len(quantiles)],
        jtail f32[B]. Refused after a grad_dev, a solve_dev or a smaller rollout, as tube_dev is."""
        cfg, rows = self._risk_cfg(centre, tail, quantiles)
        self._check(_abi.risk_entries(self.lib)[2](self._h, C.byref(cfg), B, lo, hi, rows, xref, exit, jx, first_exit, outside_any, jstat, jq, jtail,
                                                   C.c_void_p(stream)))

    # ---- predicted bands (SPEC.md §12b): per-step particle quantiles and observation ranks, reduced on the device ----
    def _bands_cfg(self, quantiles, ranks):
        """-> (cfg or None, ranks or None, quantiles or None). ranks given: they are used as they are and quantiles is ignored."""
        if ranks is None and quantiles is None:
            return None, None, None
        if ranks is None:
            quantiles = tuple(float(q) for q in quantiles)
            ranks = quantile_ranks(quantiles, self.P)
        else:
            quantiles, ranks = None, [int(r) for r in ranks]
        if not 1 <= len(ranks) <= _abi.BANDS_MAX_RANKS:
            raise ValueError(f"quantiles / ranks: 1 to {_abi.BANDS_MAX_RANKS} values")
        cfg = _abi.SdempcBandsCfg()
        cfg.struct_size = C.sizeof(_abi.SdempcBandsCfg)
        cfg.n_ranks = len(ranks)
        for k, r in enumerate(ranks):
            cfg.ranks[k] = r
        return cfg, ranks, quantiles

    def _bands_call(self, fn, x0, u, xref, draw, quantiles, ranks, observed):
        B = x0.shape[0]
        H = self.H
        x0, u, xref = _f32(x0, (B, 13)), _f32(u, (B, H, self.m)), _f32(xref, (B, H + 1, 13))
        cfg, ranks, quantiles = self._bands_cfg(quantiles, ranks)
        obs = _f32(observed, (B, H + 1, 13)) if observed is not None else None
        u32p = C.POINTER(C.c_uint32)
        cost = np.zeros(B, np.float32)
        q = np.zeros((B, cfg.n_ranks, H + 1, 13), np.float32) if cfg is not None else None
        below = np.zeros((B, H + 1, 13), np.uint32) if obs is not None else None
        at = np.zeros((B, H + 1, 13), np.uint32) if obs is not None else None
        f = lambda a: _fp(a) if a is not None else None
        w = lambda a: a.ctypes.data_as(u32p) if a is not None else None
        self._check(fn(self._h, C.byref(cfg) if cfg is not None else None, B, _fp(x0), _fp(u), _fp(xref), draw, f(obs), _fp(cost), f(q), w(below), w(at)))
        return Bands.of(self.P, ranks, quantiles, obs, cost, q, below, at)

    def bands(self, x0, u, xref, noise, quantiles=(0.05, 0.5, 0.95), ranks=None, observed=None) -> Bands:
        """One rollout of u per instance with its particle x horizon tensor reduced on the device to per-step quantiles across the particles (SPEC.md §12b):
        Bands(cost, q, below, at). quantiles: up to 8 values in [0, 1], each the rank ceil(q P) - 1 of the key order (quantile_ranks); ranks: the 0-based ranks
        themselves instead. observed f32[B][H+1][13]: rows to rank in the predicted distribution (NaN where there is none) — below / at count the particles
        below / at them; None: neither is computed. quantiles=None and ranks=None: no q."""
        x0 = _f32(x0)
        noise = _f32(noise, (x0.shape[0], self.P, self.H, 6))
        return self._bands_call(_abi.bands_entries(self.lib)[0], x0, u, xref, _fp(noise), quantiles, ranks, observed)

    def bands_keys(self, x0, u, xref, keys, quantiles=(0.05, 0.5, 0.95), ranks=None, observed=None) -> Bands:
        """bands() with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as solve_keys draws it."""
        x0 = _f32(x0)
        keys = self._keys(keys, x0.shape[0])
        return self._bands_call(_abi.bands_entries(self.lib)[1], x0, u, xref, keys.ctypes.data_as(C.POINTER(C.c_uint32)), quantiles, ranks, observed)

    def bands_dev(self, B, quantiles=None, ranks=None, observed=None, q=None, below=None, at=None, stream=0):
        """Device pointers (each may be None): reduces the tensor the last rollout_dev(store_traj=True) of at least B instances left in the handle. observed:
        pointer to f32[B][H+1][13]; q f32[B][Q][H+1][13] (Q = len(quantiles) or len(ranks)), below / at uint32[B][H+1][13]. Refused after a grad_dev, a
        solve_dev or a smaller rollout, as tube_dev is."""
        cfg, _, _ = self._bands_cfg(quantiles, ranks)
        self._check(_abi.bands_entries(self.lib)[2](self._h, C.byref(cfg) if cfg is not None else None, B, observed, q, below, at, C.c_void_p(stream)))

    # ---- predicted outcome (SPEC.md §12c): the score's failure criteria over the particles, reduced on the device ----
    def _outcome_cfg(self, score, target, ranks, quantiles, B):
        """-> (cfg, target rows or None, ranks or None, quantiles or None). score: a Score (its substeps flag plays no part: a rollout has none); target: None
        (the call's xref) or rows [Bt][Ht][13] / [Ht][13] / [13] with Ht in {1, H+1}, Bt in {1, B}; ranks given: used as they are and quantiles is ignored."""
        score = Score() if score is None else score
        cfg = _abi.SdempcOutcomeCfg()
        cfg.struct_size = C.sizeof(_abi.SdempcOutcomeCfg)
        cfg.r2_pos, cfg.cos_min, cfg.w2_max = (float(t) for t in score.thresholds())
        rows = None
        if target is not None:
            rows = np.asarray(target, np.float32)
            if rows.ndim == 1:
                rows = rows[None, None]
            elif rows.ndim == 2:
                rows = rows[None]
            if rows.ndim != 3 or rows.shape[2] != 13:
                raise ValueError("target: rows [Bt][Ht][13], [Ht][13] or [13]")
            rows = np.ascontiguousarray(rows)
            cfg.target_mode, cfg.tgt_batch, cfg.tgt_steps = 1, rows.shape[0], rows.shape[1]
        if ranks is None and quantiles is not None:
            quantiles = tuple(float(q) for q in quantiles)
            ranks = quantile_ranks(quantiles, self.P)
        elif ranks is not None:
            quantiles, ranks = None, [int(r) for r in ranks]
        if ranks is not None:
            if not 1 <= len(ranks) <= _abi.OUTCOME_MAX_RANKS:
                raise ValueError(f"quantiles / ranks: 1 to {_abi.OUTCOME_MAX_RANKS} values")
            cfg.n_ranks = len(ranks)
            for k, r in enumerate(ranks):
                cfg.ranks[k] = r
        return cfg, rows, ranks, quantiles

    def _outcome_call(self, fn, x0, u, xref, draw, score, target, ranks, quantiles, want_particles):
        B = x0.shape[0]
        H, P = self.H, self.P
        x0, u, xref = _f32(x0, (B, 13)), _f32(u, (B, H, self.m)), _f32(xref, (B, H + 1, 13))
        cfg, rows, ranks, quantiles = self._outcome_cfg(score, target, ranks, quantiles, B)
        K = cfg.n_ranks
        u32p = C.POINTER(C.c_uint32)
        cost = np.zeros(B, np.float32)
        words = np.zeros((B, P, _abi.OUTCOME_WORDS), np.uint32) if want_particles else None
        fail_step = np.zeros((B, H, 5), np.uint32)
        first_fail = np.zeros((B, H + 1), np.uint32)
        cause_ever = np.zeros((B, 4), np.uint32)
        chan_stat = np.zeros((B, H, 4, 3), np.float32)
        chan_q = np.zeros((B, H, 4, K), np.float32) if K else None
        agg_stat = np.zeros((B, 4, 3), np.float32)
        agg_q = np.zeros((B, 4, K), np.float32) if K else None
        f = lambda a: _fp(a) if a is not None else None
        w = lambda a: a.ctypes.data_as(u32p) if a is not None else None
        self._check(fn(self._h, C.byref(cfg), B, _fp(x0), _fp(u), _fp(xref), draw, f(rows), _fp(cost), w(words), w(fail_step), w(first_fail), w(cause_ever),
                       _fp(chan_stat), f(chan_q), _fp(agg_stat), f(agg_q)))
        return Outcome.of(P, ranks, quantiles, cost, words, fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat, agg_q)

    def outcome(self, x0, u, xref, noise, score=None, target=None, ranks=None, quantiles=(0.5, 0.95), want_particles=False) -> Outcome:
        """One rollout of u per instance with every particle of its particle x horizon tensor scored on the device as closed_loop(score=...) scores an episode
        (SPEC.md §12c): Outcome(cost, words, fail_step, first_fail, cause_ever, chan_stat, chan_q, agg_stat, agg_q). score: a Score — the SAME object a
        campaign is scored with, so predicted and flown failure rates share one definition (default Score(): every criterion off, only non-finite states
        fail). target: None scores row t against row t of xref; rows [Bt][Ht][13], [Ht][13] or [13] (Ht in {1, H+1}, Bt in {1, B}) against those. quantiles:
        up to 8 values in [0, 1] (rank ceil(q P) - 1, quantile_ranks) or ranks: the 0-based ranks themselves; both None: no order statistics (they are
        refused above P = 128). want_particles: also the per-particle score words."""
        x0 = _f32(x0)
        noise = _f32(noise, (x0.shape[0], self.P, self.H, 6))
        return self._outcome_call(_abi.outcome_entries(self.lib)[0], x0, u, xref, _fp(noise), score, target, ranks, quantiles, want_particles)

    def outcome_keys(self, x0, u, xref, keys, score=None, target=None, ranks=None, quantiles=(0.5, 0.95), want_particles=False) -> Outcome:
        """outcome() with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as solve_keys draws it."""
        x0 = _f32(x0)
        keys = self._keys(keys, x0.shape[0])
        return self._outcome_call(_abi.outcome_entries(self.lib)[1], x0, u, xref, keys.ctypes.data_as(C.POINTER(C.c_uint32)), score, target, ranks, quantiles,
                                  want_particles)

    def outcome_dev(self, B, score=None, target=None, tgt_steps=None, tgt_batch=None, xref=None, ranks=None, quantiles=None, words=None, fail_step=None,
                    first_fail=None, cause_ever=None, chan_stat=None, chan_q=None, agg_stat=None, agg_q=None, stream=0):
        """Device pointers (each may be None): reduces the tensor the last rollout_dev(store_traj=True) of at least B instances left in the handle. target: None
        (then xref, a pointer to f32[B][H+1][13], gives the target rows) or a pointer to f32[tgt_batch][tgt_steps][13]. Outputs: words u32[B][P][11],
        fail_step u32[B][H][5], first_fail u32[B][H+1], cause_ever u32[B][4], chan_stat f32[B][H][4][3], chan_q f32[B][H][4][K], agg_stat f32[B][4][3], agg_q
        f32[B][4][K] (K = len(quantiles) or len(ranks)). Refused after a grad_dev, a solve_dev or a smaller rollout, as tube_dev is."""
        cfg, _, _, _ = self._outcome_cfg(score, None, ranks, quantiles, B)
        if target is not None:
            cfg.target_mode = 1
            cfg.tgt_steps = self.H + 1 if tgt_steps is None else int(tgt_steps)
            cfg.tgt_batch = B if tgt_batch is None else int(tgt_batch)
        self._check(_abi.outcome_entries(self.lib)[2](self._h, C.byref(cfg), B, target, xref, words, fail_step, first_fail, cause_ever, chan_stat, chan_q,
                                                      agg_stat, agg_q, C.c_void_p(stream)))

    def closed_loop(self, x0, xref, keys, T, u_init=None, stepsize_in=None, plant=None, plant_of=None, plant_substeps=1, plant_dt=None,
                    plant_mlp_dtype=None, plant_math_mode=None, solve_period=1, solve_delay=0, motor_lag=0.0, u_act_in=None, disturbance=None,
                    rate_loop=None, rate_integ_in=None, rate_tail_in=None, fault=None, substep_states=False, meas_noise=None, meas_bias=None, meas_valid=None,
                    meas_keys=None, xmeas_in=None, meas_age=None, meas_age_max=None, meas_renorm=False, xhist_in=None, score=None, score_ref=None, score_in=None,
                    outputs=True, dist_process=None, dist_keys=None, dist_state_in=None, bias_process=None, bias_keys=None, bias_state_in=None,
                    track=None, track_of=None, track_phase=None, track_rate=None, track_offset=None, track_tick0=None, track_renorm=None,
                    fault_process=None, fault_keys=None, fault_state_in=None, fault_tick0=0, drop_process=None, drop_keys=None, drop_state_in=None, controller=None, ensemble=None, cohort=None,
                    retire=False):
        """B episodes of T closed-loop ticks on the device (SPEC.md §11, sdempc_closed_loop_batch): solve, apply uopt[0], one step of the
        model under its own noise draw, warm-start from the shifted solution. x0 f32[B][13]; keys uint32[B][2]; xref f32[Tx][Bx][H+1][13]
        with Tx in {1, T} (one window on every tick, or one per tick) and Bx in {1, B} (shared, or one per episode), or a single window
        f32[H+1][13]; u_init [B][H][m] / stepsize_in [B] default to what reset() gives. Returns
        (xs [B][T+1][13], us [B][T][m], info [B][T][8], u_next [B][H][m], stepsize_next [B], keys_next uint32[B][2]).

        plant (SPEC.md §11a, sdempc_closed_loop_batch_plant): the vehicle the controller flies when it is NOT the controller's model — a
        RotorSDEModel or a blob (one plant for every episode), or a sequence of Np of them with plant_of int[B] naming each episode's plant
        (optional when Np is 1 or B: all 0 / identity). plant_substeps Euler–Maruyama steps per tick with the applied control held;
        plant_dt their length (None: float32(time_steps[0]) / float32(plant_substeps)); plant_mlp_dtype / plant_math_mode the arithmetic
        of the plant step (None: the handle's) — pin them to compare two controller arithmetics on one and the same vehicle. With
        plant=None every plant_* argument must keep its default and the call is sdempc_closed_loop_batch, unchanged.

        solve_period / solve_delay / motor_lag / u_act_in (SPEC.md §11b, sdempc_closed_loop_batch_timed): the controller at the node's timing — a solve
        every solve_period ticks, whose solution is applied solve_delay plant substeps after the state it was computed from (0 .. solve_period *
        plant_substeps; until then the vehicle flies the previous solution's tail, row by row), and a first-order motor lag a <- a + motor_lag (c - a)
        per plant substep (0: off) from the motor state u_act_in [B][m] (None: u_init[:, 0]). With all four at their defaults the call is exactly the
        one above. Otherwise xref is f32[Tx][Bx][H+1][13] with Tx in {1, Ns}, Ns = ceil(T / solve_period) (one window per SOLVE), info is [B][Ns][8], the
        plant defaults to the handle's own model, and a 7-tuple comes back: the six above and u_act_next [B][m]. Carrying (xs[:, -1], u_next,
        stepsize_next, keys_next, u_act_next) into the next call continues the episodes bit for bit when T is a multiple of solve_period.

        disturbance / a 2-D plant_of (SPEC.md §11c, sdempc_closed_loop_batch_scenario): things that happen to a vehicle during an episode. disturbance is
        f32[Td][Bd][6] with Td in {1, T} (per control TICK) and Bd in {1, B}, or [T][6] (shared by all episodes), or [6] (constant); row (k, b) is an external
        linear acceleration in the solver's world frame and an external angular acceleration in the body frame, added to v and omega after every plant
        substep of tick k: fma(w, dt_plant, .). A [B][6] array is not accepted (it cannot be told from [T][6]). plant_of int[T][B] names the plant of every
        tick: a switch at a tick start changes the vehicle only (state, motor state, keys and warm start carry over), and the set may then hold up to B * T
        plants. With disturbance=None and a 1-D plant_of the call takes the routes above, unchanged; otherwise it is the timed call (7-tuple, xref and info
        per solve, the plant defaulting to the handle's own model) with the schedules applied.

        rate_loop / rate_integ_in / rate_tail_in (SPEC.md §11d, sdempc_closed_loop_batch_rate): the loop the node flies at its default weight_motors = 0 —
        the solution goes to the vehicle as a table of mean thrust and predicted body rates, and the vehicle's own rate loop (a RateLoop: PI on the rate
        error, mixer, blend with the motor values) turns it into motor commands on EVERY plant substep, from the plant's current body rates. So between two
        solves the vehicle still rejects gusts and model error. With rate_loop given the call is the timed / scenario call (xref and info per solve, the
        plant defaulting to the handle's own model, every keyword above still applies) and TEN values come back: the seven above, then
        ws [B][T][4] (the setpoint (mean thrust, rates[3]) in force at each tick's first substep), rate_integ_next [B][3] (the integrator state) and
        rate_tail_next [B][H][3] (the last solve's predicted rates, shifted as the warm start is: what is flown until the next solution arrives). Carrying
        those two back in as rate_integ_in / rate_tail_in (default: zeros) with the five items above continues the episodes bit for bit when T is a
        multiple of solve_period. us stays the motor state at each tick's first substep. rate_integ_in / rate_tail_in without rate_loop raise ValueError;
        with rate_loop=None nothing of this paragraph is touched.

        fault / substep_states (SPEC.md §11e, sdempc_closed_loop_batch_fault): fault is a per-motor schedule f32[Tf][Bf][m][2] with Tf in {1, T} (per control
        TICK) and Bf in {1, B}, or [T][m][2] (shared by all episodes), or [m][2] (constant); row (k, b, l) = (kappa, beta), and in every plant substep of tick k
        what reaches rotor l is fma(kappa, a_l, beta) — see fault_schedule() for the neutral array and the recipes (dead, weakened, stuck, biased). The motor
        state a (us, u_act_next, the lag) is untouched, and neither the solve nor the rate loop is told: they see the fault through the state only.
        substep_states=True appends xsub [B][T * plant_substeps][13] as the LAST returned value: the plant state after every substep, so
        xsub[:, plant_substeps - 1::plant_substeps] is xs[:, 1:] bit for bit. Either one makes the call the timed one (xref and info per solve, the plant
        defaulting to the handle's own model; every keyword above still applies); fault alone does not change the returned tuple. With fault=None and
        substep_states=False nothing of this paragraph is touched.

        meas_noise / meas_bias / meas_valid / meas_keys / xmeas_in (SPEC.md §11f, sdempc_closed_loop_batch_observed): the controller reads an ESTIMATE of the state, as
        the node does, not the plant's state to the last bit. meas_noise (the scale sigma, finite and >= 0) and meas_bias (beta, finite) are f32[No][Bo][12] with No
        in {1, Ns} (per SOLVE) and Bo in {1, B}, or [Ns][12] (shared by all episodes), or [12] (constant), in the order p, v, theta, omega; meas_valid is
        int[Nv][Bv] with the same axis rule, or [Ns]: 1 a measurement, 0 a dropout. Solve j starts from xm instead of the plant state x: on a valid solve
        e = fma(sigma, normal(me, (12,)), beta) with (q, me) = split(q) on the observation chain meas_keys uint32[B][2] (required; it advances at every solve, valid
        or not, and never touches `keys`), xm = x + e on position, velocity and body rates, and the attitude times (1, e[6:9] / 2) from the right, not renormalised;
        on a dropout xm stays what it was (initially xmeas_in [B][13]; None: x0). The plant and the rate loop are untouched: they see the estimate through the
        solves only. Either of the first three makes the call the timed one (xref and info per solve, the plant defaulting to the handle's own model; every keyword
        above still applies), and xmeas [B][Ns][13] (what each solve started from), meas_keys_next uint32[B][2] and xmeas_next [B][13] are appended to the returned
        tuple; xsub, when requested, stays the LAST value. Carrying the last two back in with the items above continues the episodes bit for bit when T is a multiple
        of solve_period. meas_keys or xmeas_in without one of the first three, or one of them without meas_keys, raise ValueError; with none of the five given
        nothing of this paragraph is touched.

        meas_age / meas_age_max / meas_renorm / xhist_in (SPEC.md §11g, sdempc_closed_loop_batch_aged): INPUT-side latency and a unit attitude. meas_age is the age of
        the estimate in PLANT SUBSTEPS: an int, int[Ns] (per solve) or int[Na][Ba] with Na in {1, Ns} and Ba in {1, B}. A valid solve with age A forms its measurement
        from the plant state A substeps before the solve, not from the current one (solve_delay is the other half: the solution arriving late). The loop keeps the last
        meas_age_max substep states (default: the largest entry; at most min(solve_period, T) * plant_substeps, one period of memory); before the run they are
        xhist_in [B][age_max][13], oldest first (None: the vehicle sat at x0). meas_renorm=True scales the attitude of the measurement to unit length (software
        rsqrt). A dropout does neither. Each of the four needs the observation keywords above (ValueError otherwise). With age_max > 0, xhist_next
        [B][age_max][13] (the last age_max substep states before the run's end) is appended after xmeas_next; xsub stays the LAST value; carried back in as xhist_in
        with the other continuation values it continues the episodes bit for bit when T is a multiple of solve_period. Every age 0 without meas_renorm reproduces
        the paragraph above bit for bit. Coloured estimator noise needs no keyword: gauss_markov_bias draws meas_bias rows of a first-order Gauss-Markov process.
        With none of the four given nothing of this paragraph is touched.

        score / score_ref / score_in / outputs (SPEC.md §11h, sdempc_closed_loop_batch_scored): the evaluator. score is a Score (a position radius, a tilt and a body-rate
        limit, each off by default; substeps=True scores every plant substep state instead of every tick state); score_ref, required with it, is the target each row
        is compared with, f32[Tr][Br][13] with Tr in {1, T} (per control TICK: the target of x_{k+1} and of the substep states of tick k is row k) and Br in {1, B}, or
        [T][13] (shared by all episodes), or [13] (constant), in the solver's frame. The device forms 16 words per episode from rows it already holds — rows scored,
        sum / max (and where) / last of the squared position error, sum of the squared velocity error, the smallest tilt cosine, the largest squared rate, the first
        failing row, the causes (SCORE_CAUSES) and the number of failing rows, saturated motor commands, squared control effort, iterations, line-search trials and
        solves without a decrease — and they come back as ONE more value, a structured array [B] of dtype SCORE_DTYPE (score_summary reduces it), placed behind
        every value above; xsub, when requested, stays the LAST value. score makes the call the timed one (xref and info per solve, the plant defaulting to the
        handle's own model; every keyword above still applies). score_in [B] (a score a previous call returned; None: score_init(B)) continues it: word for word the
        score of the joined run when the first call's T is a multiple of solve_period. outputs=False passes NULL for the per-row outputs — xs, us, info, ws, xmeas and
        xsub are then neither copied back nor scattered, and None stands in their places in the returned tuple; the continuation values and the score are
        unchanged. The score depends on nothing but the episode: not on B, the chunking or the outputs requested. score_ref / score_in / outputs=False without score
        raise ValueError; with none of the four given nothing of this paragraph is touched.

        dist_process / dist_keys / dist_state_in and bias_process / bias_keys / bias_state_in (SPEC.md §11i, sdempc_closed_loop_batch_drawn): gusts and estimator bias
        DRAWN ON THE DEVICE, so that a campaign is described by keys and O(B) parameters instead of [T][B][6] and [Ns][B][12] host arrays. Each process is a GaussMarkov
        (rho and scale per component, shared or per episode) with its own key chain uint32[B][2] (required) and a start state f32[B][W] (None: zeros;
        GaussMarkov.stationary_state draws a stationary one). dist_process (W = 6) takes one step per control TICK, ticks inside a solve period included, and its state
        g is the tick's disturbance row (added, in float32, to the row of `disturbance` when that is given as well); it makes the call a scenario run. bias_process
        (W = 12) takes one step per SOLVE, valid or not — a dropout holds the estimate, the error process keeps running — and g is the solve's beta (added to the row
        of `meas_bias` when given); it makes the call an observed one and needs meas_keys, whose chain it does not touch. Behind the score and before xsub (which
        stays LAST) come, with dist_process, dist_rows f32[B][T][6] (the rows the plant read), dist_keys_next and dist_state_next, and with bias_process bias_rows
        f32[B][Ns][12], bias_keys_next and bias_state_next; the rows are None under outputs=False. Carrying the *_next values back in continues the run bit for bit:
        the disturbance process for any T, the bias process when T is a multiple of solve_period. A process without its keys, or keys / a state without the process,
        raises ValueError; with none of the six given nothing of this paragraph is touched.

        track / track_of / track_phase / track_rate / track_offset / track_tick0 / track_renorm (SPEC.md §11j, sdempc_closed_loop_batch_tracked): TRAJECTORY TRACKING
        with the reference windows CUT ON THE DEVICE, so that what the controller is asked to fly is a small table and O(B) numbers instead of an [Ns][B][H+1][13] host
        array. track is a Trajectory or a sequence of them (track_of int[B] then names each episode's table; None: table 0), and xref must be None. Episode b flies its
        table from track_phase[b] (f32[B] or a scalar; None: 0) at track_rate[b] >= 0 times its speed (None: 1; 0 holds the point at the phase) shifted by
        track_offset[b] (f32[B][3] or f32[3]; None: 0): row i of the window of the solve at global tick k = track_tick0 + tick is the table at
        tau = fma(rate, float32(k) * dt_0 + c_i, phase), c the cumulative time_steps — wrapped into a periodic table, clamped to a clamped one —, with the velocity and
        body rates scaled by the rate and, unless track_renorm=False, the interpolated attitude scaled to unit length. score_ref="track" cuts the score targets from
        the same tables (the target of x_{k+1} is the row at float32(k + 1) * dt_0). The call is the timed one (info per solve, the plant defaulting to the handle's
        own model; every keyword above still applies) and the returned tuple is unchanged: nothing new comes back. Windows and targets depend on the global tick
        alone, so passing track_tick0 + T as the next call's track_tick0 with the other continuation values continues the run bit for bit, under the conditions
        stated above for them. xref together with track, a track_* keyword or score_ref="track" without track, raise ValueError; with none of the seven given
        nothing of this paragraph is touched.

        fault_process / fault_keys / fault_state_in / fault_tick0 and drop_process / drop_keys / drop_state_in (SPEC.md §11k, sdempc_closed_loop_batch_events): motor
        faults and estimator dropouts at RANDOM TIMES, drawn on the device in integers alone, so that a reliability campaign is described by keys and O(B) thresholds
        instead of a [T][B][m][2] fault array and an [Ns][B] flag array. fault_process is a FaultProcess with its own key chain fault_keys uint32[B][2] (required):
        per episode and motor a Markov chain with up to four failure modes takes one step per control TICK, ticks inside a solve period included, and the row the
        plant reads at tick k is the mode's (kappa, beta) while the motor is failed and otherwise the row of `fault` (when given as well) or the neutral (1, 0). The
        state after the step of tick k is the state during it, so a motor can be failed at tick 0. fault_state_in int32[B][m][2] (None: healthy) holds per motor
        (state, first): first is the GLOBAL tick fault_tick0 + k of the first onset, or -1. It makes the call a faulted one. drop_process is a Dropouts with its own
        chain drop_keys: one step per SOLVE, valid or not, before the measurement is formed; the solve is a dropout while the chain is in its dropped state, or where
        meas_valid (when given as well) says so. drop_state_in int32[B][2] (None: zeros) is (state, solves dropped). It makes the call an observed one and needs
        meas_keys, whose chain it does not touch. Behind the bias process's values and before xsub (which stays LAST) come, with fault_process, fault_rows
        f32[B][T][m][2] (the rows the plant read), fault_keys_next and fault_state_next, and with drop_process valid_rows int32[B][Ns] (the flags the measurement
        read), valid_keys_next and valid_state_next; the rows are None under outputs=False. Carrying the *_next values back in continues a chain bit for bit: the
        fault chain for any T (with fault_tick0 + T as the next fault_tick0), the dropout chain when T is a multiple of solve_period. event_summary reduces
        fault_state_next. A process without its keys, or keys / a state / a tick without the process, raises ValueError; with none of the seven given nothing of
        this paragraph is touched.

        controller (SPEC.md §11l, sdempc_closed_loop_batch_baseline): the BASELINE. A GeometricController replaces the solve of every solve period, and nothing else:
        from the state the solve would have started from (the plant's, or the estimate) and rows ref_row, ref_row + 1 of the episode's reference window it forms a
        collective thrust and three body rates on the device, and the period flies them through rate_loop (required, with motor_weight 0; ValueError otherwise)
        exactly as it flies a solution's table. Keys, gusts, faults, estimator, windows, score, chunking and continuation are untouched, so a second call with the
        same arguments and controller=None flies the MPC under the same conditions and the two scores are a paired comparison. The returned tuple is the rate
        route's: u_next holds thrust rows (every motor the thrust command), info rows are (0, stepsize, 0, ...) and the step size is handed through. Parameters may
        be one set or one per episode. With controller=None nothing of this paragraph is touched.

        ensemble / cohort (SPEC.md §11m, sdempc_closed_loop_batch_ensemble): TIME-RESOLVED histories of the batch, reduced over the EPISODES on the device. ensemble
        is an Ensemble (edges per channel, over="alive" or "all") and needs score (ValueError otherwise); cohort int[B] (None: all 0) puts every episode into one of
        up to 16 groups — faulted / unfaulted, a parameter cell, a controller arm. For every scored row of the call (T of them, or T * plant_substeps with a substep
        score) and every cohort the device forms 20 + 4 * n_edges words from the rows, targets and thresholds the score reads: the cohort's size, the episodes
        included, failed by now (the survival curve) and violating each criterion in this row, sum / min / max of the squared position and velocity errors, the
        tilt cosine and the squared rate over the included episodes, and how many of them lie below each edge. They come back as ONE more value, uint32[R][G][W],
        right behind the score (ensemble_summary reduces it); nothing else in the returned tuple moves or changes, and the words are the same under outputs=False
        and any chunking. A float sum has one fixed association over blocks of 256 consecutive episodes, so the words depend on B and on the order of the episodes.
        A run continued through score_in keeps counting rows, so its words are the later rows of the joined run. With controller=None the MPC is flown, with a
        controller the baseline: one Ensemble and one cohort array give the two arms of a paired comparison. cohort without ensemble raises ValueError; with neither
        given nothing of this paragraph is touched.

        retire (SPEC.md §11n, sdempc_closed_loop_batch_retire): with retire=True an episode whose score records a failure — a first failing row, from this call's
        rows or from score_in — is RETIRED at the next solve-period boundary: it is neither solved nor scored from then on, and everything else about it proceeds as
        before (the plant flies its held table, its chains and keys advance, its info rows are (0, stepsize, 0, ...)). Only the live episodes are solved, in a dense
        batch, so the device time of a campaign falls with the retired share. Needs score (ValueError otherwise); with ensemble= only over="alive" (ValueError for
        over="all": the rows of a retired episode are not a fleet statistic). An episode that never fails has every row and every score word bit-identical to the
        run without retire; one that fails has identical rows through the end of its failing period, where its score words freeze. TWO more values come back right
        behind the score (and the ensemble words, if any): retired_at int32[B], the first solve index of this call at which the episode was not solved (0: retired
        at entry, -1: never), and live int32[Ns], the number of episodes solved at each solve (retire_summary reduces them). A run cut in two through score_in and
        the *_next outputs gives the single call's score, keys and every row of the episodes live at the cut (an episode retired before the cut flies the second
        call's warm start behind it: its held table is not carried across calls). With controller= the baseline skips retired episodes by the same mask. retire=False: nothing of this
        paragraph is touched."""
        x0 = _f32(x0)
        B, T = x0.shape[0], int(T)
        x0 = _f32(x0, (B, 13))
        keys = self._keys(keys, B)
        tracked = track is not None
        score_track = isinstance(score_ref, str) and score_ref == "track"
        if not tracked and (track_of is not None or track_phase is not None or track_rate is not None or track_offset is not None or track_tick0 is not None or
                            track_renorm is not None or score_track):
            raise ValueError('closed_loop: track_of / track_phase / track_rate / track_offset / track_tick0 / track_renorm / score_ref="track" need track=Trajectory(...)')
        if tracked:
            if xref is not None:
                raise ValueError("closed_loop: xref must be None with track=... (an array and a trajectory for the same thing cannot both be meant)")
            tick0_ = 0 if track_tick0 is None else int(track_tick0)
            if tick0_ < 0 or tick0_ + max(T, 0) >= 1 << 24:
                raise ValueError("closed_loop: track_tick0 must be >= 0 and track_tick0 + T below 2^24")
            tkc, keep_track = self._track_cfg(track, B, track_of, track_phase, track_rate, track_offset, tick0_, True if track_renorm is None else track_renorm, score_track)
            if score_track:
                score_ref = None
            xref = np.zeros((0, 1, self.H + 1, 13), np.float32)        # (NULL and 0 solves at the entry point)
        xref = _f32(xref)
        if xref.ndim == 2:
            xref = xref[None, None]
        if xref.ndim != 4 or xref.shape[2:] != (self.H + 1, 13):
            raise ValueError(f"xref must be f32[Tx][Bx][{self.H + 1}][13] or f32[{self.H + 1}][13], got {xref.shape}")
        xref = np.ascontiguousarray(xref)
        dist = sched = None
        if disturbance is not None:
            dist = _f32(disturbance)
            if dist.ndim == 1 and dist.shape == (6,):
                dist = dist[None, None]
            elif dist.ndim == 2 and dist.shape == (T, 6):
                dist = dist[:, None]
            if dist.ndim != 3 or dist.shape[2] != 6 or dist.shape[0] not in (1, T) or dist.shape[1] not in (1, B):
                raise ValueError(f"closed_loop: disturbance must be f32[Td][Bd][6] with Td in (1, {T}) and Bd in (1, {B}), f32[{T}][6] or f32[6], "
                                 f"got {np.shape(disturbance)}")
            if not np.isfinite(dist).all():
                raise ValueError("closed_loop: disturbance holds a non-finite entry")
            dist = np.ascontiguousarray(dist)
        if plant_of is not None and np.ndim(plant_of) == 2:
            sched = np.ascontiguousarray(plant_of, dtype=np.int32)
            if sched.shape[0] not in (1, T) or sched.shape[1] != B:
                raise ValueError(f"closed_loop: a 2-D plant_of must be int[Tp][{B}] with Tp in (1, {T}), got {sched.shape}")
            if plant is None:
                raise ValueError("closed_loop: plant_of needs plant=...")
        scenario = dist is not None or sched is not None
        flt = None
        if fault is not None:
            flt = _f32(fault)
            if flt.ndim == 2 and flt.shape == (self.m, 2):
                flt = flt[None, None]
            elif flt.ndim == 3 and flt.shape == (T, self.m, 2):
                flt = flt[:, None]
            if flt.ndim != 4 or flt.shape[2:] != (self.m, 2) or flt.shape[0] not in (1, T) or flt.shape[1] not in (1, B):
                raise ValueError(f"closed_loop: fault must be f32[Tf][Bf][{self.m}][2] with Tf in (1, {T}) and Bf in (1, {B}), f32[{T}][{self.m}][2] or "
                                 f"f32[{self.m}][2], got {np.shape(fault)}")
            if not np.isfinite(flt).all():
                raise ValueError("closed_loop: fault holds a non-finite entry")
            flt = np.ascontiguousarray(flt)
        procs = {}
        for name, W_, proc, pk, ps in (("dist", 6, dist_process, dist_keys, dist_state_in), ("bias", 12, bias_process, bias_keys, bias_state_in)):
            if proc is None:
                if pk is not None or ps is not None:
                    raise ValueError(f"closed_loop: {name}_keys / {name}_state_in need {name}_process=GaussMarkov(...)")
                continue
            if not isinstance(proc, GaussMarkov):
                raise ValueError(f"closed_loop: {name}_process must be a GaussMarkov")
            if pk is None:
                raise ValueError(f"closed_loop: {name}_keys (uint32[B][2], the process chain) is required with {name}_process")
            rho_, scale_ = proc.coeffs(B, W_)
            if not (np.isfinite(rho_).all() and (rho_ >= 0).all() and (rho_ <= 1).all() and np.isfinite(scale_).all() and (scale_ >= 0).all()):
                raise ValueError(f"closed_loop: {name}_process needs rho in [0, 1] and scale finite and >= 0")
            ps = None if ps is None else _f32(ps, (B, W_))
            if ps is not None and not np.isfinite(ps).all():
                raise ValueError(f"closed_loop: {name}_state_in holds a non-finite entry")
            procs[name] = (W_, rho_, scale_, self._keys(pk, B), ps)
        drawn = bool(procs)
        evts = {}
        if fault_process is None:
            if fault_keys is not None or fault_state_in is not None or fault_tick0 != 0:
                raise ValueError("closed_loop: fault_keys / fault_state_in / fault_tick0 need fault_process=FaultProcess(...)")
        else:
            if not isinstance(fault_process, FaultProcess):
                raise ValueError("closed_loop: fault_process must be a FaultProcess")
            if fault_keys is None:
                raise ValueError("closed_loop: fault_keys (uint32[B][2], the fault chain) is required with fault_process")
            f_tick0 = int(fault_tick0)
            if f_tick0 < 0 or f_tick0 + max(T, 0) >= 1 << 24:
                raise ValueError("closed_loop: fault_tick0 must be >= 0 and fault_tick0 + T below 2^24")
            f_on, f_cl, f_md = fault_process.arrays(B, self.m)
            f_st = None
            if fault_state_in is not None:
                f_st = np.ascontiguousarray(fault_state_in, dtype=np.int32)
                if f_st.shape != (B, self.m, 2) or (f_st[..., 0] < 0).any() or (f_st[..., 0] > fault_process.n_modes).any() or (f_st[..., 1] < -1).any():
                    raise ValueError(f"closed_loop: fault_state_in must be int32[{B}][{self.m}][2] of (state in 0 .. n_modes, first tick >= -1)")
            evts["fault"] = (f_on, f_cl, f_md, self._keys(fault_keys, B), f_st, f_tick0)
        if drop_process is None:
            if drop_keys is not None or drop_state_in is not None:
                raise ValueError("closed_loop: drop_keys / drop_state_in need drop_process=Dropouts(...)")
        else:
            if not isinstance(drop_process, Dropouts):
                raise ValueError("closed_loop: drop_process must be a Dropouts")
            if drop_keys is None:
                raise ValueError("closed_loop: drop_keys (uint32[B][2], the dropout chain) is required with drop_process")
            d_dr, d_re = drop_process.arrays(B)
            d_st = None
            if drop_state_in is not None:
                d_st = np.ascontiguousarray(drop_state_in, dtype=np.int32)
                if d_st.shape != (B, 2) or (d_st[:, 0] < 0).any() or (d_st[:, 0] > 1).any() or (d_st[:, 1] < 0).any():
                    raise ValueError(f"closed_loop: drop_state_in must be int32[{B}][2] of (state in 0 .. 1, solves dropped >= 0)")
            evts["drop"] = (d_dr, d_re, self._keys(drop_keys, B), d_st)
        events = bool(evts)
        scenario = scenario or "dist" in procs
        observed = meas_noise is not None or meas_bias is not None or meas_valid is not None or "bias" in procs or "drop" in evts
        if not observed and (meas_keys is not None or xmeas_in is not None):
            raise ValueError("closed_loop: meas_keys / xmeas_in need one of meas_noise / meas_bias / meas_valid / bias_process")
        if observed:
            if meas_keys is None:
                raise ValueError("closed_loop: meas_keys (uint32[B][2], the observation chain) is required with meas_noise / meas_bias / meas_valid / bias_process")
            meas_keys = self._keys(meas_keys, B)
            Ns_o = -(-max(T, 0) // max(int(solve_period), 1))

            def rows(v, what, tail, dtype):
                a = np.ascontiguousarray(v, dtype=dtype)
                if a.ndim == len(tail) and a.shape == tail:
                    a = a[None, None]
                elif a.ndim == len(tail) + 1 and a.shape == (Ns_o,) + tail:
                    a = a[:, None]
                if a.ndim != len(tail) + 2 or a.shape[2:] != tail or a.shape[0] not in (1, Ns_o) or a.shape[1] not in (1, B):
                    t = "".join(f"[{n}]" for n in tail)
                    raise ValueError(f"closed_loop: {what} must be [No][Bo]{t} with No in (1, {Ns_o}) and Bo in (1, {B}), [{Ns_o}]{t}" + (f" or {t}" if tail else "") +
                                     f", got {np.shape(v)}")
                return np.ascontiguousarray(a)
            obs_sigma = None if meas_noise is None else rows(meas_noise, "meas_noise", (12,), np.float32)
            obs_beta = None if meas_bias is None else rows(meas_bias, "meas_bias", (12,), np.float32)
            obs_valid = None
            if meas_valid is not None:
                obs_valid = rows(np.asarray(meas_valid).astype(np.int64), "meas_valid", (), np.int64)
                if not np.isin(obs_valid, (0, 1)).all():
                    raise ValueError("closed_loop: meas_valid holds an entry other than 0 / 1")
                obs_valid = np.ascontiguousarray(obs_valid, dtype=np.int32)
            if obs_sigma is not None and not (np.isfinite(obs_sigma).all() and (obs_sigma >= 0).all()):
                raise ValueError("closed_loop: meas_noise holds a non-finite or negative entry")
            if obs_beta is not None and not np.isfinite(obs_beta).all():
                raise ValueError("closed_loop: meas_bias holds a non-finite entry")
            if obs_sigma is not None and obs_beta is not None and obs_sigma.shape != obs_beta.shape:      # (one pair of axes for both: sdempc_obs_cfg)
                shape = (max(obs_sigma.shape[0], obs_beta.shape[0]), max(obs_sigma.shape[1], obs_beta.shape[1]), 12)
                obs_sigma, obs_beta = np.ascontiguousarray(np.broadcast_to(obs_sigma, shape)), np.ascontiguousarray(np.broadcast_to(obs_beta, shape))
            if xmeas_in is not None:
                xmeas_in = _f32(xmeas_in, (B, 13))
        aged = meas_age is not None or meas_age_max is not None or bool(meas_renorm) or xhist_in is not None
        if aged and not observed:
            raise ValueError("closed_loop: meas_age / meas_age_max / meas_renorm / xhist_in need one of meas_noise / meas_bias / meas_valid (and meas_keys)")
        age_rows, age_max = None, 0
        if aged:
            if meas_age is not None:
                a = np.asarray(meas_age)
                if a.dtype.kind not in "iu":
                    raise ValueError("closed_loop: meas_age must hold integers (plant substeps)")
                age_rows = rows(a.astype(np.int64).reshape(1, 1) if a.ndim == 0 else a.astype(np.int64), "meas_age", (), np.int64)
                if age_rows.min() < 0:
                    raise ValueError("closed_loop: meas_age holds a negative entry")
            age_max = int(meas_age_max) if meas_age_max is not None else (0 if age_rows is None else int(age_rows.max()))
            lim = min(max(int(solve_period), 1), max(T, 1)) * int(plant_substeps)
            if age_max < 0 or age_max > lim:
                raise ValueError(f"closed_loop: meas_age_max must be between 0 and min(solve_period, T) * plant_substeps = {lim} (one period of memory), got {age_max}")
            if age_rows is not None:
                if age_rows.max() > age_max:
                    raise ValueError(f"closed_loop: meas_age holds an entry above meas_age_max = {age_max}")
                age_rows = np.ascontiguousarray(age_rows, dtype=np.int32)
            if xhist_in is not None:
                if age_max == 0:
                    raise ValueError("closed_loop: xhist_in needs meas_age_max > 0")
                xhist_in = _f32(xhist_in, (B, age_max, 13))
        scored = score is not None
        if not scored and (score_ref is not None or score_in is not None or not outputs):
            raise ValueError("closed_loop: score_ref / score_in / outputs=False need score=Score(...)")
        if scored:
            if not isinstance(score, Score):
                raise ValueError("closed_loop: score must be a Score")
            if score_ref is None and not score_track:
                raise ValueError("closed_loop: score_ref (the target of every tick, f32[Tr][Br][13]) is required with score")
            sref = np.zeros((1, 1, 13), np.float32) if score_track else _f32(score_ref)
            if sref.ndim == 1 and sref.shape == (13,):
                sref = sref[None, None]
            elif sref.ndim == 2 and sref.shape == (T, 13):
                sref = sref[:, None]
            if sref.ndim != 3 or sref.shape[2] != 13 or sref.shape[0] not in (1, T) or sref.shape[1] not in (1, B):
                raise ValueError(f"closed_loop: score_ref must be f32[Tr][Br][13] with Tr in (1, {T}) and Br in (1, {B}), f32[{T}][13] or f32[13], got {np.shape(score_ref)}")
            sref = np.ascontiguousarray(sref)
            if score_in is not None:
                score_in = np.ascontiguousarray(score_in)
                if score_in.dtype != SCORE_DTYPE or score_in.shape != (B,):
                    raise ValueError(f"closed_loop: score_in must be the structured score array [{B}] a previous call returned, got dtype {score_in.dtype} and shape {score_in.shape}")
        if score_track and not scored:
            raise ValueError('closed_loop: score_ref="track" needs score=Score(...)')
        baseline = controller is not None
        if baseline:
            if not isinstance(controller, GeometricController):
                raise ValueError("closed_loop: controller must be a GeometricController")
            if rate_loop is None:
                raise ValueError("closed_loop: controller= publishes thrust and body rates and needs rate_loop=RateLoop(...)")
            if not isinstance(rate_loop, RateLoop) or rate_loop.motor_weight != 0.0:
                raise ValueError("closed_loop: controller= needs a RateLoop with motor_weight 0 (its table holds no motor values)")
            gc, keep_g = self._geo_cfg(controller, B)
        ensembled = ensemble is not None
        if cohort is not None and not ensembled:
            raise ValueError("closed_loop: cohort needs ensemble=Ensemble(...)")
        if ensembled:
            if not isinstance(ensemble, Ensemble):
                raise ValueError("closed_loop: ensemble must be an Ensemble")
            if not scored:
                raise ValueError("closed_loop: ensemble needs score=Score(...) (it reduces the score's own quantities)")
            coh = None
            if cohort is not None:
                coh = np.asarray(cohort)
                if coh.dtype.kind not in "iu" or coh.shape != (B,):
                    raise ValueError(f"closed_loop: cohort must be int[{B}], got dtype {coh.dtype} and shape {coh.shape}")
                coh = np.ascontiguousarray(coh, dtype=np.int32)
            n_coh = ensemble.n_cohorts if ensemble.n_cohorts is not None else (1 if coh is None or B == 0 else int(coh.max()) + 1)
            if not (1 <= n_coh <= 16) or (coh is not None and B > 0 and (coh.min() < 0 or coh.max() >= n_coh)):
                raise ValueError(f"closed_loop: cohort must hold entries in [0, {n_coh}) and at most 16 cohorts")
        retiring = bool(retire)
        if retiring:
            if not scored:
                raise ValueError("closed_loop: retire needs score=Score(...) (an episode is retired by its score)")
            if ensembled and ensemble.over != "alive":
                raise ValueError('closed_loop: retire may not be combined with Ensemble(over="all") (the rows of a retired episode are not a fleet statistic)')
        ens_args = ensembled or retiring          # (the retire entry point takes the ensemble one's arguments, its ensemble cfg NULL without an ensemble)
        baseline_args = baseline or ens_args      # (the ensemble entry point takes the baseline one's arguments, its geo cfg NULL without a controller)
        faulted = flt is not None or bool(substep_states) or observed or scored or drawn or tracked or events or baseline
        full = scored or drawn or tracked or events or baseline          # the entry points from the scored one on take every layer's arguments, NULL where a layer is absent
        if rate_loop is None and (rate_integ_in is not None or rate_tail_in is not None):
            raise ValueError("closed_loop: rate_integ_in / rate_tail_in need rate_loop=...")
        if rate_loop is not None and not isinstance(rate_loop, RateLoop):
            raise ValueError("closed_loop: rate_loop must be a RateLoop")
        timed = scenario or faulted or rate_loop is not None or not (solve_period == 1 and solve_delay == 0 and motor_lag == 0.0 and u_act_in is None)
        Ns = T
        if timed:
            S_, D_, alpha = int(solve_period), int(solve_delay), float(np.float32(motor_lag))
            if S_ < 1:
                raise ValueError("closed_loop: solve_period must be >= 1")
            if D_ < 0 or D_ > S_ * int(plant_substeps):
                raise ValueError(f"closed_loop: solve_delay must be between 0 and solve_period * plant_substeps = {S_ * int(plant_substeps)} plant substeps "
                                 "(the worker runs one solve at a time)")
            if not (0.0 <= alpha <= 1.0):
                raise ValueError("closed_loop: motor_lag must be 0 (off) or in (0, 1]")
            Ns = -(-max(T, 0) // S_)
            if plant is None:       # the entry point always takes a plant set: the handle's own model, prepared as sdempc_create prepared it
                if plant_of is not None or plant_dt is not None or plant_mlp_dtype is not None or plant_math_mode is not None:
                    raise ValueError("closed_loop: plant_of / plant_dt / plant_mlp_dtype / plant_math_mode need plant=...")
                plant = self._blob.raw
        u_p = s_p = a_p = None
        if u_act_in is not None:
            u_act_in = _f32(u_act_in, (B, self.m))
            a_p = _fp(u_act_in)
        if u_init is not None:
            u_init = _f32(u_init, (B, self.H, self.m))
            u_p = _fp(u_init)
        if stepsize_in is not None:
            stepsize_in = _f32(stepsize_in, (B,))
            s_p = _fp(stepsize_in)
        xs = np.zeros((B, max(T, 0) + 1, 13), np.float32)
        us = np.zeros((B, max(T, 0), self.m), np.float32)
        info = np.zeros((B, max(Ns, 0), 8), np.float32)
        u_next = np.zeros((B, self.H, self.m), np.float32)
        s_next = np.zeros(B, np.float32)
        k_next = np.zeros((B, 2), np.uint32)
        u32p = C.POINTER(C.c_uint32)
        common = (B, T, _fp(x0), None if tracked else _fp(xref), int(xref.shape[0]), int(xref.shape[1]), keys.ctypes.data_as(u32p), u_p, s_p)
        outs = (_fp(xs), _fp(us), info.ctypes.data_as(C.POINTER(SdempcInfo)), _fp(u_next), _fp(s_next), k_next.ctypes.data_as(u32p))
        ret = (xs, us, info, u_next, s_next, k_next)
        if not outputs:             # (scored, checked above) NULL per-row outputs, None in their places
            outs, ret = (None, None, None) + outs[3:], (None, None, None) + ret[3:]
        if plant is None:
            if plant_of is not None or plant_substeps != 1 or plant_dt is not None or plant_mlp_dtype is not None or plant_math_mode is not None:
                raise ValueError("closed_loop: plant_of / plant_substeps / plant_dt / plant_mlp_dtype / plant_math_mode need plant=...")
            self._check(self.lib.sdempc_closed_loop_batch(self._h, *common, *outs))
            return ret
        plants = [plant] if hasattr(plant, "to_blob") or isinstance(plant, (bytes, bytearray, memoryview)) else list(plant)
        blobs = [p.to_blob() if hasattr(p, "to_blob") else bytes(p) for p in plants]
        Np = len(blobs)
        bufs = (C.c_char_p * max(Np, 1))(*blobs)
        sizes = (C.c_size_t * max(Np, 1))(*[len(b) for b in blobs])
        of_p = None
        if sched is not None:
            of_p = sched.ctypes.data_as(C.POINTER(C.c_int32))
        elif plant_of is not None:
            plant_of = np.ascontiguousarray(plant_of, dtype=np.int32)
            if plant_of.shape != (B,):
                raise ValueError(f"plant_of must be int[{B}], got {plant_of.shape}")
            of_p = plant_of.ctypes.data_as(C.POINTER(C.c_int32))
        pc = _abi.SdempcPlantCfg(C.sizeof(_abi.SdempcPlantCfg), Np, int(plant_substeps), 0.0 if plant_dt is None else float(np.float32(plant_dt)),
                                 -1 if plant_mlp_dtype is None else _abi_enum(MLP_DTYPES, plant_mlp_dtype, "plant_mlp_dtype"),
                                 -1 if plant_math_mode is None else _abi_enum(MATH_MODES, plant_math_mode, "plant_math_mode"))
        # Each layer puts one more configuration pointer in front of the layer below (include/sdempc.h); from the timed one on u_act_in sits before
        # the outputs, and the layer's own outputs follow them in the C call as in the returned tuple.
        lead, u_act, more = [C.byref(pc)], (), ()
        if timed:
            tc = _abi.SdempcTimingCfg(C.sizeof(_abi.SdempcTimingCfg), S_, D_, alpha)
            a_next = np.zeros((B, self.m), np.float32)
            lead, u_act, more, ret = [C.byref(tc)] + lead, (a_p,), (_fp(a_next),), ret + (a_next,)
        if scenario:
            sc = _abi.SdempcScenarioCfg(C.sizeof(_abi.SdempcScenarioCfg), None if dist is None else _fp(dist), 1 if dist is None else dist.shape[0],
                                        1 if dist is None else dist.shape[1], 1 if sched is None else sched.shape[0])
            lead = [C.byref(sc)] + lead
        if rate_loop is not None:
            rc_, keep = self._rate_cfg(rate_loop, plant_substeps, plant_dt)
            g_p = t_p = None
            if rate_integ_in is not None:
                rate_integ_in = _f32(rate_integ_in, (B, 3))
                g_p = _fp(rate_integ_in)
            if rate_tail_in is not None:
                rate_tail_in = _f32(rate_tail_in, (B, self.H, 3))
                t_p = _fp(rate_tail_in)
            ws = np.zeros((B, max(T, 0), 4), np.float32)
            g_next = np.zeros((B, 3), np.float32)
            t_next = np.zeros((B, self.H, 3), np.float32)
            lead = [C.byref(rc_)] + (lead if scenario else [None] + lead)       # (no scenario: a NULL scenario cfg)
            if not outputs:
                ws = None
            more, ret = more + (g_p, t_p, None if ws is None else _fp(ws), _fp(g_next), _fp(t_next)), ret + (ws, g_next, t_next)
        if faulted:                 # the rate entry point's arguments (rate cfg, scenario cfg: NULL where absent) behind the fault cfg, then xsub
            if rate_loop is None:
                lead, more = [None] + (lead if scenario else [None] + lead), more + (None,) * 5
            fc = None
            if flt is not None:
                fc = _abi.SdempcFaultCfg(C.sizeof(_abi.SdempcFaultCfg), _fp(flt), flt.shape[0], flt.shape[1])
            xsub = np.zeros((B, max(T, 0) * int(plant_substeps), 13), np.float32) if substep_states and outputs else None
            lead, more = [None if fc is None else C.byref(fc)] + lead, more + (None if xsub is None else _fp(xsub),)
            if observed:            # the fault entry point's arguments behind (obs cfg, obs_keys, xmeas_in), then xmeas, obs_keys_next, xmeas_next
                rows_ = obs_sigma if obs_sigma is not None else obs_beta
                oc = _abi.SdempcObsCfg(C.sizeof(_abi.SdempcObsCfg), None if obs_sigma is None else _fp(obs_sigma), None if obs_beta is None else _fp(obs_beta),
                                       1 if rows_ is None else rows_.shape[0], 1 if rows_ is None else rows_.shape[1],
                                       None if obs_valid is None else obs_valid.ctypes.data_as(C.POINTER(C.c_int32)),
                                       1 if obs_valid is None else obs_valid.shape[0], 1 if obs_valid is None else obs_valid.shape[1])
                xmeas = np.zeros((B, max(Ns, 0), 13), np.float32) if outputs else None
                q_next = np.zeros((B, 2), np.uint32)
                xm_next = np.zeros((B, 13), np.float32)
                lead = [C.byref(oc), meas_keys.ctypes.data_as(u32p), None if xmeas_in is None else _fp(xmeas_in)] + lead
                more, ret = more + (None if xmeas is None else _fp(xmeas), q_next.ctypes.data_as(u32p), _fp(xm_next)), ret + (xmeas, q_next, xm_next)
            elif full:              # (no observation: a NULL obs cfg and NULL observation pointers)
                lead, more = [None, None, None] + lead, more + (None, None, None)
            if aged:                # the observed entry point's arguments behind (age cfg, xhist_in), then xhist_next
                ac = _abi.SdempcAgeCfg(C.sizeof(_abi.SdempcAgeCfg), None if age_rows is None else age_rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                       1 if age_rows is None else age_rows.shape[0], 1 if age_rows is None else age_rows.shape[1], age_max, int(bool(meas_renorm)))
                xh_next = np.zeros((B, age_max, 13), np.float32) if age_max > 0 else None
                lead = [C.byref(ac), None if xhist_in is None else _fp(xhist_in)] + lead
                more = more + (None if xh_next is None else _fp(xh_next),)
                if xh_next is not None:
                    ret = ret + (xh_next,)
            elif full:              # (no age: a NULL age cfg and NULL history pointers)
                lead, more = [None, None] + lead, more + (None,)
            if scored:              # the aged entry point's arguments behind (score cfg, score_in), then score_out
                zc = _abi.SdempcScoreCfg(C.sizeof(_abi.SdempcScoreCfg), int(score.substeps), float(score.r2_pos), float(score.cos_min), float(score.w2_max), None if score_track else _fp(sref),
                                         sref.shape[0], sref.shape[1])
                z_out = np.zeros(B, SCORE_DTYPE)
                lead = [C.byref(zc), None if score_in is None else score_in.ctypes.data_as(u32p)] + lead
                more, ret = more + (z_out.ctypes.data_as(u32p),), ret + (z_out,)
                if ensembled:       # (the word array sits right behind the score; its pointer leads the C call, below)
                    ens_words = np.zeros((max(T, 0) * (int(plant_substeps) if score.substeps else 1), n_coh, ensemble.words), np.uint32)
                    ret = ret + (ens_words,)
                if retiring:        # (behind the score and the ensemble words; their pointers lead the C call, below)
                    retired_at, live = np.full(B, -1, np.int32), np.zeros(max(Ns, 0), np.int32)
                    ret = ret + (retired_at, live)
            elif drawn or tracked or events or baseline:  # (no score: a NULL score cfg and NULL score pointers)
                lead, more = [None, None] + lead, more + (None,)
            if drawn or tracked or events or baseline_args:   # the scored entry point's arguments behind (dist_proc, bias_proc), then rows, keys_next and state_next of each process
                cfgs, keep_p = [], []
                for name, Nrows in (("dist", max(T, 0)), ("bias", max(Ns, 0))):
                    if name not in procs:
                        cfgs.append(None)
                        more = more + (None, None, None)
                        continue
                    W_, rho_, scale_, pk, ps = procs[name]
                    pcfg = _abi.SdempcProcessCfg(C.sizeof(_abi.SdempcProcessCfg), rho_.shape[0], _fp(rho_), _fp(scale_), pk.ctypes.data_as(u32p), None if ps is None else _fp(ps))
                    keep_p.append(pcfg)
                    cfgs.append(C.byref(pcfg))
                    p_rows = np.zeros((B, Nrows, W_), np.float32) if outputs else None
                    p_keys, p_state = np.zeros((B, 2), np.uint32), np.zeros((B, W_), np.float32)
                    more = more + (None if p_rows is None else _fp(p_rows), p_keys.ctypes.data_as(u32p), _fp(p_state))
                    ret = ret + (p_rows, p_keys, p_state)
                lead = cfgs + lead
            if tracked:             # the drawn entry point's arguments behind the track cfg; nothing new comes back
                lead = [C.byref(tkc)] + lead
            elif events or baseline_args:    # (no track: a NULL track cfg)
                lead = [None] + lead
            if events or baseline_args:  # the tracked entry point's arguments behind (fault_proc, drop_proc), then rows, keys_next and state_next of each chain
                i32p = C.POINTER(C.c_int32)
                ecfgs, keep_e = [None, None], []
                if "fault" in evts:
                    f_on, f_cl, f_md, fk, f_st, f_tick0 = evts["fault"]
                    fpc = _abi.SdempcFaultProcessCfg(C.sizeof(_abi.SdempcFaultProcessCfg), f_on.shape[2], f_on.shape[0], f_on.ctypes.data_as(u32p), f_cl.ctypes.data_as(u32p),
                                                     _fp(f_md), fk.ctypes.data_as(u32p), None if f_st is None else f_st.ctypes.data_as(i32p), f_tick0)
                    keep_e.append(fpc)
                    ecfgs[0] = C.byref(fpc)
                    f_rows = np.zeros((B, max(T, 0), self.m, 2), np.float32) if outputs else None
                    fk_next, fs_next = np.zeros((B, 2), np.uint32), np.zeros((B, self.m, 2), np.int32)
                    more = more + (None if f_rows is None else _fp(f_rows), fk_next.ctypes.data_as(u32p), fs_next.ctypes.data_as(i32p))
                    ret = ret + (f_rows, fk_next, fs_next)
                else:
                    more = more + (None, None, None)
                if "drop" in evts:
                    d_dr, d_re, dk, d_st = evts["drop"]
                    dpc = _abi.SdempcDropoutProcessCfg(C.sizeof(_abi.SdempcDropoutProcessCfg), d_dr.shape[0], d_dr.ctypes.data_as(u32p), d_re.ctypes.data_as(u32p),
                                                       dk.ctypes.data_as(u32p), None if d_st is None else d_st.ctypes.data_as(i32p))
                    keep_e.append(dpc)
                    ecfgs[1] = C.byref(dpc)
                    v_rows = np.zeros((B, max(Ns, 0)), np.int32) if outputs else None
                    vk_next, vs_next = np.zeros((B, 2), np.uint32), np.zeros((B, 2), np.int32)
                    more = more + (None if v_rows is None else v_rows.ctypes.data_as(i32p), vk_next.ctypes.data_as(u32p), vs_next.ctypes.data_as(i32p))
                    ret = ret + (v_rows, vk_next, vs_next)
                else:
                    more = more + (None, None, None)
                lead = ecfgs + lead
            if baseline:            # the events entry point's arguments behind the geo cfg; nothing new comes back
                lead = [C.byref(gc)] + lead
            elif ens_args:          # (no controller: a NULL geo cfg)
                lead = [None] + lead
            if ensembled:           # the baseline entry point's arguments behind (ensemble cfg, ens_out)
                ec = _abi.SdempcEnsembleCfg(C.sizeof(_abi.SdempcEnsembleCfg), n_coh, ensemble.n_edges, 1 if ensemble.over == "alive" else 0,
                                            None if coh is None else coh.ctypes.data_as(C.POINTER(C.c_int32)), _fp(ensemble.edges) if ensemble.n_edges else None)
                lead = [C.byref(ec), ens_words.ctypes.data_as(u32p)] + lead
            elif retiring:          # (no ensemble: a NULL ensemble cfg and no word array)
                lead = [None, None] + lead
            if retiring:            # the ensemble entry point's arguments behind (retire cfg, retired_at, live_per_solve)
                yc = _abi.SdempcRetireCfg(C.sizeof(_abi.SdempcRetireCfg), 0)
                lead = [C.byref(yc), retired_at.ctypes.data_as(C.POINTER(C.c_int32)), live.ctypes.data_as(C.POINTER(C.c_int32))] + lead
            if substep_states:
                ret = ret + (xsub,)
        # the entry point, from (timed, scenario, rate_loop, faulted) alone; only the one that is called is looked up
        if retiring:
            entry = _abi.retire_entry(self.lib)
        elif ensembled:
            entry = _abi.ensemble_entry(self.lib)
        elif baseline:
            entry = _abi.baseline_entry(self.lib)
        elif events:
            entry = _abi.events_entry(self.lib)
        elif tracked:
            entry = _abi.tracked_entry(self.lib)
        elif drawn:
            entry = _abi.drawn_entry(self.lib)
        elif scored:
            entry = _abi.scored_entry(self.lib)
        elif aged:
            entry = _abi.aged_entry(self.lib)
        elif observed:
            entry = _abi.observed_entry(self.lib)
        elif faulted:
            entry = _abi.fault_entry(self.lib)
        elif rate_loop is not None:
            entry = _abi.rate_entry(self.lib)
        elif scenario:
            entry = _abi.scenario_entry(self.lib)
        elif timed:
            entry = _abi.timed_entry(self.lib)
        else:
            entry = self.lib.sdempc_closed_loop_batch_plant
        self._check(entry(self._h, *lead, C.cast(bufs, C.POINTER(C.c_void_p)), sizes, of_p, *common, *u_act, *outs, *more))
        return ret

    def _track_cfg(self, track, B, track_of, phase, rate, offset, tick0, renorm, score_targets):
        """sdempc_track_cfg of one Trajectory or a sequence of them for B episodes, and what must stay alive while it is in use."""
        tables = [track] if isinstance(track, Trajectory) else list(track)
        if not tables or not all(isinstance(t, Trajectory) for t in tables):
            raise ValueError("closed_loop: track must be a Trajectory or a non-empty sequence of them")
        knots = np.array([t.t.shape[0] for t in tables], np.int32)
        t_all = np.ascontiguousarray(np.concatenate([t.t for t in tables]), np.float32)
        x_all = np.ascontiguousarray(np.concatenate([t.x for t in tables]), np.float32)
        period = np.array([t.period for t in tables], np.float32)
        keep = [knots, t_all, x_all, period]
        i32p = C.POINTER(C.c_int32)

        def per_episode(v, tail, what, dtype=np.float32):
            if v is None:
                return None
            a = np.asarray(v, dtype)
            if a.shape == tail:
                a = np.broadcast_to(a, (B,) + tail)
            if a.shape != (B,) + tail:
                raise ValueError(f"closed_loop: {what} must have shape {(B,) + tail}" + (f" or {tail}" if tail else " or be a scalar") + f", got {np.shape(v)}")
            a = np.ascontiguousarray(a, dtype)
            keep.append(a)
            return a
        of = None
        if track_of is not None:
            of = np.asarray(track_of)
            if of.dtype.kind not in "iu" or of.shape != (B,) or of.min() < 0 or of.max() >= len(tables):
                raise ValueError(f"closed_loop: track_of must be int[{B}] with entries in [0, {len(tables)})")
            of = np.ascontiguousarray(of, np.int32)
            keep.append(of)
        ph, rt, off = per_episode(phase, (), "track_phase"), per_episode(rate, (), "track_rate"), per_episode(offset, (3,), "track_offset")
        if (ph is not None and not np.isfinite(ph).all()) or (off is not None and not np.isfinite(off).all()):
            raise ValueError("closed_loop: track_phase / track_offset hold a non-finite entry")
        if rt is not None and not (np.isfinite(rt).all() and (rt >= 0).all()):
            raise ValueError("closed_loop: track_rate must be finite and >= 0")
        cfg = _abi.SdempcTrackCfg(C.sizeof(_abi.SdempcTrackCfg), len(tables), knots.ctypes.data_as(i32p), _fp(t_all), _fp(x_all), _fp(period),
                                  None if of is None else of.ctypes.data_as(i32p), None if ph is None else _fp(ph), None if rt is None else _fp(rt),
                                  None if off is None else _fp(off), int(tick0), int(bool(renorm)), int(bool(score_targets)))
        return cfg, keep

    def reference_windows(self, track, ticks, B, track_of=None, track_phase=None, track_rate=None, track_offset=None, track_tick0=0, track_renorm=True):
        """The reference windows f32[n][B][H+1][13] the device cuts from `track` for B episodes at the global ticks track_tick0 + ticks[g] (SPEC.md §11j,
        sdempc_reference_windows): the launch closed_loop(track=...) makes in front of every solve, with no loop around it — for callers of solve_keys who want
        device-formed windows. The track_* keywords are closed_loop's."""
        k = np.ascontiguousarray(np.asarray(ticks, np.int64).reshape(-1))
        if k.size < 1 or k.min() < 0 or int(track_tick0) < 0 or k.max() + int(track_tick0) >= 1 << 24:
            raise ValueError("reference_windows: ticks must be a non-empty int array with 0 <= track_tick0 + tick < 2^24")
        k = np.ascontiguousarray(k, np.int32)
        B = int(B)
        if B < 1:
            raise ValueError("reference_windows: B must be >= 1")
        cfg, keep = self._track_cfg(track, B, track_of, track_phase, track_rate, track_offset, int(track_tick0), track_renorm, False)
        out = np.zeros((k.shape[0], B, self.H + 1, 13), np.float32)
        self._check(_abi.reference_windows_entry(self.lib)(self._h, C.byref(cfg), B, k.shape[0], k.ctypes.data_as(C.POINTER(C.c_int32)), _fp(out)))
        del keep
        return out

    def _geo_cfg(self, controller, B):
        """sdempc_geo_cfg of a GeometricController for B episodes on this handle, and what must stay alive while it is in use."""
        if controller.ref_row > self.H - 1:
            raise ValueError(f"controller.ref_row must be between 0 and H - 1 = {self.H - 1}, got {controller.ref_row}")
        bounds = np.asarray(self.cfg_py.input_bound, np.float32)
        batch, arr = controller.arrays(B, bounds[:, 0], bounds[:, 1])
        inv_dt = np.float32(1.0) / np.float32(self.cfg_py.time_steps[controller.ref_row])
        gc = _abi.SdempcGeoCfg(C.sizeof(_abi.SdempcGeoCfg), batch, *[_fp(arr[n]) for n in ("kp", "kv", "amax", "inv_tau", "g", "kT", "k0", "c_lo", "c_hi")],
                               int(controller.accel_ff), controller.ref_row, float(inv_dt))
        return gc, arr

    def geo_command(self, x, xref, controller):
        """The geometric controller alone (SPEC.md §11l, sdempc_geo_command_batch): (c, omega*) f32[B][4] for states x f32[B][13] and windows xref f32[Bx][H+1][13]
        (Bx in {1, B}, or one window f32[H+1][13]), formed by the device code the closed loop runs."""
        if not isinstance(controller, GeometricController):
            raise ValueError("geo_command: controller must be a GeometricController")
        x = _f32(x)
        B = x.shape[0]
        x = _f32(x, (B, 13))
        xref = _f32(xref)
        if xref.ndim == 2:
            xref = xref[None]
        if xref.ndim != 3 or xref.shape[1:] != (self.H + 1, 13) or xref.shape[0] not in (1, B):
            raise ValueError(f"geo_command: xref must be f32[Bx][{self.H + 1}][13] with Bx in (1, {B}) or f32[{self.H + 1}][13], got {xref.shape}")
        xref = np.ascontiguousarray(xref)
        gc, keep = self._geo_cfg(controller, B)
        out = np.zeros((B, 4), np.float32)
        self._check(_abi.geo_command_entry(self.lib)(self._h, C.byref(gc), B, _fp(x), _fp(xref), xref.shape[0], _fp(out)))
        return out

    def _rate_cfg(self, rate_loop, plant_substeps, plant_dt):
        """sdempc_rate_cfg of a RateLoop for this handle: ki_dt = float32(ki) * float32(dt_plant), the default mixer from the controller's rotor tables (as
        the blob holds them), inv_m = float32(1) / float32(m)."""
        m = self.m
        mixer = rate_loop.mixer
        if mixer is None:
            from .model import rate_mixer
            f = np.frombuffer(self._blob.raw, np.float32, _abi.BLOB_FLOATS, 4 * _abi.BLOB_HEADER_INTS)
            mixer = rate_mixer(f[16:16 + m], f[24:24 + m], f[32:32 + m])
        if mixer.shape != (m, 3):
            raise ValueError(f"closed_loop: rate_loop.mixer must be f32[{m}][3], got {mixer.shape}")
        dt = np.float32(plant_dt) if plant_dt is not None and float(plant_dt) != 0.0 else np.float32(self.cfg_py.time_steps[0]) / np.float32(int(plant_substeps))
        rc = _abi.SdempcRateCfg()
        rc.struct_size = C.sizeof(_abi.SdempcRateCfg)
        ki_dt = (rate_loop.ki * np.float32(dt)).astype(np.float32)
        for a in range(3):
            rc.kp[a], rc.ki_dt[a], rc.integ_limit[a] = float(rate_loop.kp[a]), float(ki_dt[a]), float(rate_loop.integ_limit[a])
        for l in range(m):
            for a in range(3):
                rc.mixer[l][a] = float(mixer[l, a])
        rc.motor_weight = rate_loop.motor_weight
        rc.inv_m = float(np.float32(1.0) / np.float32(m))
        return rc, mixer

    def noise_from_keys(self, keys):
        """The canonical noise tensors f32[B][P][H][6] the device draws from keys (inspection / parity tests)."""
        keys = self._keys(keys)
        B = keys.shape[0]
        out = np.zeros((B, self.P, self.H, 6), np.float32)
        self._check(self.lib.sdempc_noise_from_keys(self._h, B, keys.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(out)))
        return out

    def noise_from_keys_dev(self, keys, noise_out, stream=0):
        """keys: host uint32[B][2]; noise_out: device pointer to sdempc_noise_dev_floats(B) floats (device layout)."""
        keys = self._keys(keys)
        self._check(self.lib.sdempc_noise_from_keys_dev(self._h, keys.shape[0], keys.ctypes.data_as(C.POINTER(C.c_uint32)), noise_out,
                                                        C.c_void_p(stream)))

    # ---- device-resident entry points (torch tensors or raw device pointers) ---------------------
    def noise_to_device_layout(self, noise):
        noise = _f32(noise)
        B = noise.shape[0]
        out = np.zeros(self.lib.sdempc_noise_dev_floats(self._h, B), np.float32)
        self._check(self.lib.sdempc_noise_to_device_layout(self._h, B, _fp(noise), _fp(out)))
        return out.reshape(B, (self.P + 31) // 32, self.H, 6, 32)

    def noise_to_device_layout_dev(self, B, noise_canonical, noise_out, stream=0):
        """Device pointers: canonical f32[B][P][H][6] -> f32[B][G][H][6][32] (LDS-tiled transpose on the GPU)."""
        self._check(self.lib.sdempc_noise_to_device_layout_dev(self._h, B, noise_canonical, noise_out, C.c_void_p(stream)))

    def traj_to_canonical_dev(self, B, traj_out, stream=0):
        """Particle x horizon tensor of the last rollout_dev(store_traj=True) / grad_dev -> canonical f32[B][P][H+1][13]."""
        self._check(self.lib.sdempc_traj_to_canonical_dev(self._h, B, traj_out, C.c_void_p(stream)))

    def solve_dev(self, B, x0, xref, noise_dev, u_init, stepsize, uopt, xevol, info, stream=0):
        """All arguments are device pointers (ints). info: f32[B][8]."""
        self._check(self.lib.sdempc_solve_batch_dev(self._h, B, x0, xref, noise_dev, u_init, stepsize, uopt, xevol, info,
                                                    C.c_void_p(stream)))

    def rollout_dev(self, B, x0, u, xref, noise_dev, cost, xmean=None, store_traj=False, stream=0):
        self._check(self.lib.sdempc_rollout_batch_dev(self._h, B, x0, u, xref, noise_dev, cost, xmean, int(store_traj),
                                                      C.c_void_p(stream)))

    def grad_dev(self, B, x0, u, xref, noise_dev, cost, grad, stream=0):
        self._check(self.lib.sdempc_grad_batch_dev(self._h, B, x0, u, xref, noise_dev, cost, grad, C.c_void_p(stream)))

    def solve_status(self):
        """After synchronising the stream of the last solve_dev call: raises SdempcError if a grid barrier of a cooperative layout
        gave up (results invalid; the handle then stays on the one-workgroup-per-instance layouts, so the call can be repeated)."""
        self._check(self.lib.sdempc_solve_status(self._h))

    def layout_fallbacks(self) -> int:
        return int(self.lib.sdempc_layout_fallbacks(self._h))

    def work_counters(self, reset: bool = False):
        """(solves, gradient evaluations, forward-only rollouts) done by this handle's solve launches so far (sdempc_work_counters)."""
        return self.work_counters_full(reset)[:3]

    def work_counters_full(self, reset: bool = False):
        """work_counters() plus a fourth word: how many of the counted line-search trials were settled without a rollout (a negative
        Armijo bound under non-negative cost weights, SPEC.md §8). The rollouts actually run are [2] - [3]."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.sdempc_work_counters(self._h, out, int(reset)))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def settled_trials(self) -> int:
        """Line-search trials this handle's solve launches have settled without a rollout so far (work_counters_full()[3])."""
        return self.work_counters_full()[3]

    def last_kernel_name(self) -> str:
        """Kernel instantiation the last *_dev launch started, as rocprofv3 prints it (sdempc_last_kernel_name)."""
        buf = C.create_string_buffer(512)
        self._check(self.lib.sdempc_last_kernel_name(self._h, buf, 512))
        return buf.value.decode()

    def last_kernel_ms(self) -> float:
        return float(self.lib.sdempc_last_kernel_ms(self._h))
