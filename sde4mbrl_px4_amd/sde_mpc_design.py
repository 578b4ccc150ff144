"""Drop-in for `sde4mbrlExamples.rotor_uav.sde_mpc_design` (import site sde_control.py:12).

`load_mpc_from_cfgfile(mpc_dir, convert_to_enu=True)` returns
    cfg_dict, (m_reset, m_mpc), state_from_traj, None
with the call signatures the reference node uses:
    m_reset(x=, rng=, xdes=) -> opt_state                                     sde_control.py:702,706,345-346,389-394
    m_mpc(x, rng, opt_state, curr_t=, xdes=) -> (uopt, opt_state, rng, xevol)  sde_control.py:713,717,349-350,400-416
    state_from_traj(t) -> f32[13]  (None for position-control YAMLs)           sde_control.py:164,177,206,694
    cfg_dict['_time_steps'][0] = dt                                            sde_control.py:167,174
Returned arrays are numpy arrays wrapped so that `.block_until_ready()` exists (sde_control.py:420,707,718).
opt_state exposes yk and the seven telemetry scalars read at sde_control.py:444-450,646-647.

Frame contract (SPEC.md §1a). The node hands over the vehicle state `x` as it arrives in the MPC_FULL_STATE message, documented as
NED (sde_control.py:228-232,246), while every target it builds is ENU: the position set-point (:186-192), `state_from_traj` (:206,
trajectory CSVs are ENU), and the hold target `enu2ned(curr_state, np)` (:400), i.e. the NED state flipped to ENU. The factory is
called with `convert_to_enu=True` (:685): the solver converts `x` itself. So, with convert_to_enu=True, m_mpc maps x -> enu2ned(x)
(the flip is an involution), solves in ENU / FLU (the frame of SPEC.md §5), takes `xdes` / `state_from_traj` as ENU, and returns
`xevol` flipped back to the frame of `x` (its body rates, rows 10..12, go to the FCU: sde_control.py:432). `uopt` is frame-free.
With convert_to_enu=False nothing is converted: x, xdes and the trajectory are taken to be in the solver's frame already.

The solve itself runs in the HIP kernels behind include/sdempc.h; this module is host glue only.
"""
from __future__ import annotations

import os
import warnings
from dataclasses import dataclass, field
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import prng, workload
from .config import MPCConfig, load_mpc_config
from .model import RotorSDEModel, synthetic_hexa, synthetic_iris
from .utils import TrajectoryCSV, enu2ned


class DeviceArray(np.ndarray):
    """numpy array with the one JAX-array method the reference calls."""

    def block_until_ready(self):
        return self


def _arr(a) -> DeviceArray:
    return np.ascontiguousarray(a, dtype=np.float32).view(DeviceArray)


class OptState(NamedTuple):
    """Optimiser state threaded through successive m_mpc calls (sde_control.py:345,400-416,444-450)."""
    yk: DeviceArray                # [H, m] warm start for the next solve
    avg_linesearch: np.float32
    stepsize: np.float32
    num_steps: np.float32
    grad_sqr: np.float32
    avg_stepsize: np.float32
    init_cost: np.float32
    opt_cost: np.float32
    num_ls_trials: np.float32 = np.float32(0.0)


def _next_key(rng):
    """SPEC.md §7.3: `new_rng, sub = split(rng)` with JAX's threefry2x32 split; the solve draws its noise tensor as
    normal(sub, (P, H, 6)) on the device. Returns (new_rng, sub), both uint32[2]."""
    k = prng.split(np.asarray(rng, dtype=np.uint32).reshape(2), 2)
    return k[0].copy(), k[1].copy()


@dataclass
class MpcProblem:
    """One loaded MPC YAML: config, model, solver handle (created lazily) and reference source."""
    cfg: MPCConfig
    model: RotorSDEModel
    state_from_traj: Optional[Callable] = None
    shift_warm_start: bool = True
    convert_to_enu: bool = True           # sde_control.py:685; see the frame contract in the module docstring
    _solver: object = field(default=None, repr=False)
    _pid: int = field(default=-1, repr=False)

    def solver(self):
        # HIP contexts do not survive fork(): the reference builds its solvers in the parent and uses them in the forked mpc_process
        # (sde_control.py:69-75,723-728), so the handle is (re)created per process. A handle inherited through fork() is never
        # touched again: no HIP call may run on the parent's context in the child, not even the frees of sdempc_destroy, so it is
        # detached (leaked). If the parent had already initialised the GPU through it (a real solve before the fork) the child's HIP
        # runtime is unusable: fail loudly instead of hanging inside the control process.
        if self._solver is not None and self._pid != os.getpid():
            inherited, self._solver = self._solver, None
            was_ready = inherited.device_ready()
            inherited.detach()
            if was_ready:
                raise RuntimeError(
                    "sde4mbrl_px4_amd: this process was forked after its parent had already run a solve on the GPU (HIP state does "
                    "not survive fork()). Keep real solver calls out of the parent: the first call of each compiled callable there is "
                    "answered by a shape probe (jax_shim, SDEMPC_PREFORK), or start the worker with the 'spawn' method.")
        if self._solver is None:
            from .solver import SdeMpcSolver
            self._solver = SdeMpcSolver(self.cfg, self.model, max_batch=1)
            self._pid = os.getpid()
        return self._solver

    def xref(self, curr_t: float, xdes) -> np.ndarray:
        if self.state_from_traj is not None:
            return workload.reference_window(float(curr_t), self.cfg.time_steps, self.state_from_traj)
        return workload.constant_reference(np.asarray(xdes, np.float32), self.cfg.horizon)

    def trajectory(self, t0: float, t1: float, n: int, period: float = 0.0):
        """The loaded state_from_traj sampled at n knots over [t0, t1] as a solver.Trajectory (SPEC.md §11j): what simulate(track=...) and
        SdeMpcSolver.closed_loop(track=...) take. state_from_traj returns solver-frame states, as every reference window is; trajectory time 0 is t0."""
        if self.state_from_traj is None:
            raise ValueError("MpcProblem.trajectory: no trajectory is loaded (a position-control configuration)")
        from .solver import Trajectory
        return Trajectory.from_function(self.state_from_traj, t0, t1, n, period)

    # ---- the two callables ------------------------------------------------------------------------
    def m_reset(self, x=None, rng=None, xdes=None) -> OptState:
        H, m = self.cfg.horizon, self.cfg.num_motors
        yk = np.tile(np.asarray(self.cfg.uref, np.float32), (H, 1))
        s0 = self.cfg.ls_init_stepsize if self.cfg.ls_maxls > 0 else self.cfg.stepsize
        z = np.float32(0.0)
        return OptState(_arr(yk), z, np.float32(s0), z, z, z, z, z, z)

    def shape_probe_m_mpc(self, x, rng, opt_state: OptState, curr_t=0.0, xdes=None):
        """Outputs with the shapes/dtypes of m_mpc and no device work (see jax_shim._Compiled): the warm start as uopt,
        the current state repeated as xevol. Used only for the reference's pre-fork warm-up calls."""
        x = np.asarray(x, np.float32).reshape(13)
        nan = np.float32(np.nan)       # marks the state as "not the result of a solve": num_steps 0, costs NaN (jax_shim warns as well)
        marked = opt_state._replace(num_steps=np.float32(0.0), init_cost=nan, opt_cost=nan)
        return _arr(np.asarray(opt_state.yk, np.float32)), marked, rng, _arr(np.tile(x, (self.cfg.horizon + 1, 1)))

    def m_mpc(self, x, rng, opt_state: OptState, curr_t=0.0, xdes=None):
        x = np.asarray(x, np.float32).reshape(13)
        xs = enu2ned(x, np) if self.convert_to_enu else x           # vehicle state in the solver's frame (module docstring)
        xdes = xs if xdes is None else np.asarray(xdes, np.float32).reshape(13)
        new_rng, sub = _next_key(rng)
        xref = self.xref(float(curr_t), xdes)[None]
        u0 = np.asarray(opt_state.yk, np.float32)[None]
        uopt, xevol, info = self.solver().solve_keys(xs[None], xref, sub[None], u0, np.array([opt_state.stepsize], np.float32))
        if self.convert_to_enu:                                     # predicted states back in the frame of x
            xevol = enu2ned(xevol, np)
        uo = uopt[0]
        yk = np.concatenate([uo[1:], uo[-1:]], axis=0) if self.shift_warm_start else uo
        i = info[0]
        st = OptState(_arr(yk), np.float32(i[0]), np.float32(i[1]), np.float32(i[2]), np.float32(i[3]), np.float32(i[4]),
                      np.float32(i[5]), np.float32(i[6]), np.float32(i[7]))
        return _arr(uo), st, new_rng, _arr(xevol[0])

    def m_tube(self, x, rng, uopt, curr_t=0.0, xdes=None, lo=None, hi=None):
        """The predicted tube (SPEC.md §12) of the plan `uopt` on the noise m_mpc(x, rng, ...) solved on: the same key rule (SPEC.md §7.3, `sub` of
        split(rng, 2)), the same reference window, one rollout, its particle x horizon tensor reduced on the device. Returns a solver.Tube whose planes are
        [H+1][13] (cost a scalar array) IN THE SOLVER'S FRAME — variance, extrema and counts per component do not survive the attitude part of the frame flip —
        and so are lo / hi. With the uopt m_mpc returned, `mean` is that call's xevol bit for bit (through enu2ned when convert_to_enu is set). rng is not
        consumed: pass the key that went INTO m_mpc."""
        from .solver import Tube
        x = np.asarray(x, np.float32).reshape(13)
        xs = enu2ned(x, np) if self.convert_to_enu else x
        xdes = xs if xdes is None else np.asarray(xdes, np.float32).reshape(13)
        _, sub = _next_key(rng)
        xref = self.xref(float(curr_t), xdes)[None]
        u = np.asarray(uopt, np.float32).reshape(1, self.cfg.horizon, self.cfg.num_motors)
        t = self.solver().tube_keys(xs[None], u, xref, sub[None], lo=lo, hi=hi)
        return Tube.of(t.P, *(a[0] for a in t))

    def m_risk(self, x, rng, uopt, curr_t=0.0, xdes=None, lo=None, hi=None, centre=None, tail=None, quantiles=None, want_particles=False):
        """Predicted risk (SPEC.md §12a) of the plan `uopt` on the noise m_mpc(x, rng, ...) solved on: the key rule of m_tube (SPEC.md §7.3), the same reference
        window, one rollout, its tensor reduced on the device. Returns a solver.Risk without the batch axis, IN THE SOLVER'S FRAME, as lo / hi / centre rows are.
        rng is not consumed: pass the key that went INTO m_mpc."""
        from .solver import Risk
        x = np.asarray(x, np.float32).reshape(13)
        xs = enu2ned(x, np) if self.convert_to_enu else x
        xdes = xs if xdes is None else np.asarray(xdes, np.float32).reshape(13)
        _, sub = _next_key(rng)
        xref = self.xref(float(curr_t), xdes)[None]
        u = np.asarray(uopt, np.float32).reshape(1, self.cfg.horizon, self.cfg.num_motors)
        if centre is not None and not isinstance(centre, str):
            centre = np.asarray(centre, np.float32)[None]
        r = self.solver().risk_keys(xs[None], u, xref, sub[None], lo=lo, hi=hi, centre=centre, tail=tail, quantiles=quantiles, want_particles=want_particles)
        return Risk.of(r.P, *(None if a is None else a[0] for a in r))

    def m_bands(self, x, rng, uopt, curr_t=0.0, xdes=None, quantiles=(0.05, 0.5, 0.95), ranks=None, observed=None):
        """Predicted bands (SPEC.md §12b) of the plan `uopt` on the noise m_mpc(x, rng, ...) solved on: the key rule of m_tube (SPEC.md §7.3), the same reference
        window, one rollout, its tensor reduced on the device. Returns a solver.Bands without the batch axis, IN THE SOLVER'S FRAME (§1a), as the rows of
        `observed` [H+1][13] are (NaN where there is none). rng is not consumed: pass the key that went INTO m_mpc."""
        from .solver import Bands
        x = np.asarray(x, np.float32).reshape(13)
        xs = enu2ned(x, np) if self.convert_to_enu else x
        xdes = xs if xdes is None else np.asarray(xdes, np.float32).reshape(13)
        _, sub = _next_key(rng)
        xref = self.xref(float(curr_t), xdes)[None]
        u = np.asarray(uopt, np.float32).reshape(1, self.cfg.horizon, self.cfg.num_motors)
        if observed is not None:
            observed = np.asarray(observed, np.float32).reshape(1, self.cfg.horizon + 1, 13)
        r = self.solver().bands_keys(xs[None], u, xref, sub[None], quantiles=quantiles, ranks=ranks, observed=observed)
        return Bands.of(r.P, r.ranks, r.quantiles, None if r.observed is None else r.observed[0], *(None if a is None else a[0] for a in r))

    def m_outcome(self, x, rng, uopt, curr_t=0.0, xdes=None, score=None, target=None, ranks=None, quantiles=(0.5, 0.95), want_particles=False):
        """Predicted outcome (SPEC.md §12c) of the plan `uopt` on the noise m_mpc(x, rng, ...) solved on: the key rule of m_tube (SPEC.md §7.3), the same
        reference window, one rollout, every particle scored on the device with the criteria of `score` (a solver.Score, the one a simulate(score=...) campaign
        uses). Returns a solver.Outcome without the batch axis. target: None (the reference window) or rows [H+1][13] / [13] IN THE SOLVER'S FRAME, as m_risk's
        centre rows are. rng is not consumed: pass the key that went INTO m_mpc."""
        from .solver import Outcome
        x = np.asarray(x, np.float32).reshape(13)
        xs = enu2ned(x, np) if self.convert_to_enu else x
        xdes = xs if xdes is None else np.asarray(xdes, np.float32).reshape(13)
        _, sub = _next_key(rng)
        xref = self.xref(float(curr_t), xdes)[None]
        u = np.asarray(uopt, np.float32).reshape(1, self.cfg.horizon, self.cfg.num_motors)
        if target is not None:
            target = np.asarray(target, np.float32).reshape(1, -1, 13)
        r = self.solver().outcome_keys(xs[None], u, xref, sub[None], score=score, target=target, ranks=ranks, quantiles=quantiles, want_particles=want_particles)
        return Outcome.of(r.P, r.ranks, r.quantiles, *(None if a is None else a[0] for a in r))


    def simulate(self, x, rng, T, curr_t=0.0, xdes=None, opt_state: Optional[OptState] = None, plant=None, plant_substeps=1, plant_dt=None,
                 plant_mlp_dtype=None, plant_math_mode=None, solve_period=1, solve_delay=0, motor_lag=0.0, disturbance=None, plant_of=None, rate_loop=None,
                 fault=None, substep_states=False, meas_noise=None, meas_bias=None, meas_valid=None, meas_rng=None, meas_age=None, meas_renorm=False,
                 score=None, score_ref=None, dist_process=None, dist_rng=None, dist_state=None, bias_process=None, bias_rng=None, bias_state=None,
                 track=None, track_phase=None, track_rate=None, fault_process=None, fault_rng=None, fault_state=None, drop_process=None, drop_rng=None,
                 drop_state=None, controller=None, retire=False):
        """T ticks of m_mpc in closed loop with the model itself as the plant, on the device (SPEC.md §11): solve, apply uopt[0], one
        Euler–Maruyama step of the controller's own model under a fresh noise draw, warm-start from the shifted solution. Equivalent to
        T calls of m_mpc, each followed by that step, but with no host round trip per tick. `x` is converted into the solver's frame once
        and the states back once (not per tick). Tick k tracks self.xref(curr_t + k * dt_0, xdes) when a trajectory is loaded, else xdes
        (default: the initial state). opt_state None starts from m_reset. Returns (xs f32[T+1][13] with xs[0] = x, us f32[T][m],
        info f32[T][8], the OptState after the last tick, the key after the last tick).
        plant / plant_*: fly another vehicle than the controller's model (a RotorSDEModel or a blob), stepped plant_substeps times per tick —
        the arguments of SdeMpcSolver.closed_loop (SPEC.md §11a), passed through for this one episode.
        solve_period / solve_delay / motor_lag: the controller at the node's timing (SPEC.md §11b) — a solve every solve_period ticks, applied
        solve_delay plant substeps late, through a first-order motor lag. Solve j then tracks self.xref(curr_t + j * solve_period * dt_0, xdes), info is
        f32[Ns][8] with Ns = ceil(T / solve_period), and the motor state starts at the warm start's first row.
        disturbance / plant_of: a scenario (SPEC.md §11c) — disturbance f32[T][6] or f32[6], an external linear (world) and angular (body) acceleration per
        tick GIVEN IN THE FRAME OF x (under convert_to_enu the vector rules of enu2ned take it into the solver's frame, exactly: (x, y, z) -> (y, x, -z) and
        (wx, wy, wz) -> (wx, -wy, -wz)); plant_of int[T] names, per tick, which member of the sequence `plant` flies the tick (a payload dropped at
        tick k: plant=[loaded, empty], plant_of = [0] * k + [1] * (T - k)). Either one makes the call the timed one (info per solve).
        rate_loop: a solver.RateLoop (SPEC.md §11d) — the vehicle flies the solution's thrust and body-rate setpoints through its own rate loop on every plant
        substep, as behind the node's setpoint interface; passed through, the call is then the timed one. Gains and mixer act on body-frame quantities of
        the solver's frame. The returned values are the same five.
        fault / substep_states (SPEC.md §11e): fault f32[T][m][2] or f32[m][2], a per-motor row (kappa, beta) per tick — what reaches rotor l is
        fma(kappa, a_l, beta) (solver.fault_schedule has the recipes: dead, weakened, stuck, biased); motor commands have no frame, so nothing is converted.
        substep_states=True appends xsub f32[T * plant_substeps][13], the plant state after every substep, as a SIXTH value, flipped into the frame of x row by
        row like xs[1:]. Either one makes the call the timed one.
        meas_noise / meas_bias / meas_valid / meas_rng (SPEC.md §11f): the controller solves from an ESTIMATE of the state — meas_noise (sigma >= 0) and meas_bias
        f32[Ns][12] or f32[12] in the order p, v, theta, omega, GIVEN IN THE FRAME OF x (under convert_to_enu the p and v triples follow the world-vector rule
        (x, y, z) -> (y, x, -z) and the theta and omega triples the body-vector rule (wx, wy, wz) -> (wx, -wy, -wz), exactly as `disturbance`; a scale takes the
        permutation without the sign), meas_valid int[Ns] (0: a dropout, the last estimate is held; initially x itself), meas_rng uint32[2] the observation key
        (required with any of the three; the main key `rng` is never disturbed). Any of the three makes the call the timed one and appends TWO values behind the
        five: xmeas f32[Ns][13], what each solve started from, flipped into the frame of x row by row like xs[1:], and the observation key after the last solve
        (xmeas[-1] is the held measurement that continues the run). xsub, when requested, stays the LAST value.
        meas_age / meas_renorm (SPEC.md §11g; each needs one of the three above): meas_age, an int or int[Ns], is the age of the estimate in PLANT SUBSTEPS — a
        valid solve measures the state that many substeps back (before the run the vehicle sat at x; at most min(solve_period, T) * plant_substeps) —, and
        meas_renorm=True scales the measured attitude to unit length. Ages have no frame. With a largest age A > 0 the last A substep states before the run's end,
        f32[A][13], oldest first, follow the observation key, flipped into the frame of x row by row like xs[1:]; xsub stays the LAST value.
        score / score_ref (SPEC.md §11h): score is a solver.Score; the episode's 16 score words, formed on the device, are appended behind every value above as a
        structured array [1] (solver.SCORE_DTYPE; xsub stays the LAST value), and the call is the timed one. score_ref f32[T][13] or f32[13] is the target each scored
        state of tick k is compared with, GIVEN IN THE FRAME OF x and converted by enu2ned like xs. Its default is the reference at the END of each tick: the loaded
        trajectory at curr_t + (k + 1) * dt_0 (already in the solver's frame, as every reference window is), else xdes. score_ref without score raises ValueError.
        dist_process / dist_rng / dist_state and bias_process / bias_rng / bias_state (SPEC.md §11i): a solver.GaussMarkov drawn on the device — a gust per control
        tick (width 6, added to `disturbance` when given) or an estimator bias per solve (width 12, added to `meas_bias` when given; the call is then an observed one
        and needs meas_rng) — with its own key uint32[2] (required) and a start state f32[W] (None: zeros), GIVEN IN THE FRAME OF x. Under convert_to_enu the
        coefficients rho and scale take the permutation without the sign, as meas_noise does, and the state in, the state out and the returned rows follow the signed
        vector rules of `disturbance` and `meas_bias`. Behind the score and before xsub come, per process given (disturbance first), its rows f32[T][6] / f32[Ns][12],
        its key after the run and its state after the run. A key or a state without its process raises ValueError.
        track / track_phase / track_rate (SPEC.md §11j): a solver.Trajectory IN THE SOLVER'S FRAME (self.trajectory samples the loaded state_from_traj into one),
        passed through: the device cuts the window of every solve and, with a score and no score_ref, the target of every tick from the table, entered at
        track_phase and flown at track_rate times its speed; the global tick of the run's first tick is round(curr_t / dt_0). This is a DIFFERENT arithmetic
        from the state_from_traj route above, which stays as it is, float64 and all: float32 interpolation between the knots, the same trajectory to a few
        ulps of a linear interpolant and no further. xdes is then not read; the returned values are the same. track_phase / track_rate without track raise
        ValueError.
        fault_process / fault_rng / fault_state and drop_process / drop_rng / drop_state (SPEC.md §11k): a solver.FaultProcess (motor failures at random ticks; the
        call is then a faulted one) and a solver.Dropouts (bursty loss of the estimate, stepped per solve; the call is then an observed one and needs meas_rng),
        each drawn on the device from its own key uint32[2] (required), passed through for this one episode. fault_state int32[m][2] is (state, first onset tick)
        per motor (None: healthy), drop_state int32[2] (state, solves dropped) (None: zeros); the global tick of the run's first tick is round(curr_t / dt_0), as
        for track. Motor rows and flags have no frame, so nothing is converted. Behind the Gauss-Markov values and before xsub come, per chain given (faults first),
        its rows f32[T][m][2] / int32[Ns] as the plant / the measurement read them, its key after the run and its state after the run. A key or a state without
        its process raises ValueError.
        controller (SPEC.md §11l): a solver.GeometricController flies the episode in place of the MPC's solves — the baseline — through rate_loop (required), passed
        through for this one episode; its gains act on quantities of the solver's frame. Everything above still applies and the returned values are the same: the
        OptState then holds thrust rows and zero telemetry.
        retire (SPEC.md §11n; needs score): with retire=True the episode is neither solved nor scored from the solve-period boundary after its first failing row
        on — it flies its held table to the end — passed through for this one episode. Behind the score come retired_at, the first solve index at which it was not
        solved (-1: never), and live int32[Ns], 1 for every solve that ran."""
        if retire and score is None:
            raise ValueError("MpcProblem.simulate: retire needs score=Score(...)")
        if not self.shift_warm_start:
            raise ValueError("MpcProblem.simulate: the closed loop always warm-starts from the shifted solution (shift_warm_start=True)")
        T = int(T)
        x = np.asarray(x, np.float32).reshape(13)
        xs0 = enu2ned(x, np) if self.convert_to_enu else x
        xdes = xs0 if xdes is None else np.asarray(xdes, np.float32).reshape(13)
        if track is None and (track_phase is not None or track_rate is not None):
            raise ValueError("MpcProblem.simulate: track_phase / track_rate need track=Trajectory(...)")
        if track is not None:
            xref = None
        elif self.state_from_traj is not None:
            dt0 = float(self.cfg.time_steps[0])
            S = int(solve_period)
            xref = np.stack([self.xref(float(curr_t) + j * S * dt0, xdes) for j in range(-(-T // max(S, 1)))])[:, None]
        else:
            xref = self.xref(float(curr_t), xdes)[None, None]
        rng = np.asarray(rng, dtype=np.uint32).reshape(1, 2)
        u0 = s0 = None
        if opt_state is not None:
            u0 = np.asarray(opt_state.yk, np.float32)[None]
            s0 = np.array([opt_state.stepsize], np.float32)
        if disturbance is not None:
            w = np.asarray(disturbance, np.float32)
            if w.shape not in ((6,), (T, 6)):
                raise ValueError(f"MpcProblem.simulate: disturbance must be f32[{T}][6] or f32[6], got {w.shape}")
            if self.convert_to_enu:
                w = np.stack([w[..., 1], w[..., 0], -w[..., 2], w[..., 3], -w[..., 4], -w[..., 5]], axis=-1)
            disturbance = np.ascontiguousarray(w, np.float32)
        if plant_of is not None:
            plant_of = np.asarray(plant_of, np.int32)
            if plant_of.shape != (T,):
                raise ValueError(f"MpcProblem.simulate: plant_of must be int[{T}] (one episode: the plant of every tick), got {plant_of.shape}")
            plant_of = plant_of[:, None]
        more = {} if rate_loop is None else {"rate_loop": rate_loop}
        if track is not None:
            more.update(track=track, track_phase=track_phase, track_rate=track_rate, track_tick0=int(round(float(curr_t) / float(self.cfg.time_steps[0]))))
        if fault is not None:
            f = np.asarray(fault, np.float32)
            m = self.cfg.num_motors
            if f.shape not in ((m, 2), (T, m, 2)):
                raise ValueError(f"MpcProblem.simulate: fault must be f32[{T}][{m}][2] or f32[{m}][2], got {f.shape}")
            more["fault"] = f[None, None] if f.ndim == 2 else f[:, None]
        if substep_states:
            more["substep_states"] = True
        observed = meas_noise is not None or meas_bias is not None or meas_valid is not None or bias_process is not None or drop_process is not None
        if observed:
            if meas_rng is None:
                raise ValueError("MpcProblem.simulate: meas_rng (uint32[2], the observation key) is required with meas_noise / meas_bias / meas_valid / bias_process / "
                                 "drop_process")
            Ns = -(-T // max(int(solve_period), 1))
            for name, v, signed in (("meas_noise", meas_noise, False), ("meas_bias", meas_bias, True)):
                if v is None:
                    continue
                e = np.asarray(v, np.float32)
                if e.shape not in ((12,), (Ns, 12)):
                    raise ValueError(f"MpcProblem.simulate: {name} must be f32[{Ns}][12] or f32[12], got {e.shape}")
                if self.convert_to_enu:
                    sg = np.float32(-1.0 if signed else 1.0)
                    e = np.stack([e[..., 1], e[..., 0], sg * e[..., 2], e[..., 4], e[..., 3], sg * e[..., 5], e[..., 6], sg * e[..., 7], sg * e[..., 8],
                                  e[..., 9], sg * e[..., 10], sg * e[..., 11]], axis=-1)
                e = np.ascontiguousarray(e, np.float32)
                more[name] = e[None, None] if e.ndim == 1 else e[:, None]
            if meas_valid is not None:
                v = np.asarray(meas_valid)
                if v.shape != (Ns,):
                    raise ValueError(f"MpcProblem.simulate: meas_valid must be int[{Ns}] (one episode: a flag per solve), got {v.shape}")
                more["meas_valid"] = v[:, None]
            more["meas_keys"] = np.asarray(meas_rng, dtype=np.uint32).reshape(1, 2)
        elif meas_rng is not None:
            raise ValueError("MpcProblem.simulate: meas_rng needs one of meas_noise / meas_bias / meas_valid")
        if (meas_age is not None or meas_renorm) and not observed:
            raise ValueError("MpcProblem.simulate: meas_age / meas_renorm need one of meas_noise / meas_bias / meas_valid")
        hist = False
        if meas_age is not None:
            a = np.asarray(meas_age)
            if a.dtype.kind not in "iu" or a.shape not in ((), (Ns,)):
                raise ValueError(f"MpcProblem.simulate: meas_age must be an int or int[{Ns}] (plant substeps), got {a.dtype}{a.shape}")
            more["meas_age"] = a.reshape(1, 1) if a.ndim == 0 else a[:, None]
            hist = int(a.max()) > 0
        if meas_renorm:
            more["meas_renorm"] = True
        drawn = []
        for name, idx, sgn, proc, pk, ps in (("dist", _PERM6, _SIGN6, dist_process, dist_rng, dist_state), ("bias", _PERM12, _SIGN12, bias_process, bias_rng, bias_state)):
            if proc is None:
                if pk is not None or ps is not None:
                    raise ValueError(f"MpcProblem.simulate: {name}_rng / {name}_state need {name}_process=GaussMarkov(...)")
                continue
            if pk is None:
                raise ValueError(f"MpcProblem.simulate: {name}_rng (uint32[2], the process key) is required with {name}_process")
            from .solver import GaussMarkov
            if not isinstance(proc, GaussMarkov):
                raise ValueError(f"MpcProblem.simulate: {name}_process must be a solver.GaussMarkov")
            W = len(idx)
            rho, scale = proc.coeffs(1, W)
            g0 = None if ps is None else np.asarray(ps, np.float32).reshape(1, W)
            if self.convert_to_enu:        # (a scale takes the permutation without the sign; a state is a signed vector)
                rho, scale = rho[:, idx], scale[:, idx]
                g0 = None if g0 is None else np.ascontiguousarray(g0[:, idx] * sgn)
            more.update({f"{name}_process": GaussMarkov.from_coeffs(rho, scale), f"{name}_keys": np.asarray(pk, dtype=np.uint32).reshape(1, 2), f"{name}_state_in": g0})
            drawn.append((idx, sgn))
        n_evt = 0
        for name, proc, pk, ps, shape in (("fault", fault_process, fault_rng, fault_state, (1, self.cfg.num_motors, 2)), ("drop", drop_process, drop_rng, drop_state, (1, 2))):
            if proc is None:
                if pk is not None or ps is not None:
                    raise ValueError(f"MpcProblem.simulate: {name}_rng / {name}_state need {name}_process=...")
                continue
            if pk is None:
                raise ValueError(f"MpcProblem.simulate: {name}_rng (uint32[2], the chain's key) is required with {name}_process")
            more.update({f"{name}_process": proc, f"{name}_keys": np.asarray(pk, dtype=np.uint32).reshape(1, 2),
                         f"{name}_state_in": None if ps is None else np.asarray(ps, np.int32).reshape(shape)})
            if name == "fault":
                more["fault_tick0"] = int(round(float(curr_t) / float(self.cfg.time_steps[0])))
            n_evt += 1
        if score is None and score_ref is not None:
            raise ValueError("MpcProblem.simulate: score_ref needs score=Score(...)")
        if score is not None:
            if score_ref is not None:
                g = np.asarray(score_ref, np.float32)
                if g.shape not in ((13,), (T, 13)):
                    raise ValueError(f"MpcProblem.simulate: score_ref must be f32[{T}][13] or f32[13], got {g.shape}")
                if self.convert_to_enu:
                    g = enu2ned(g, np)
            elif track is not None:
                g = None
            elif self.state_from_traj is not None:
                dt0 = float(self.cfg.time_steps[0])
                g = np.asarray(self.state_from_traj(float(curr_t) + (np.arange(T, dtype=np.float64) + 1.0) * dt0), np.float32).reshape(T, 13)
            else:
                g = xdes
            if g is None:
                more.update(score=score, score_ref="track")
            else:
                g = np.ascontiguousarray(g, np.float32)
                more.update(score=score, score_ref=g[None, None] if g.ndim == 1 else g[:, None])
        out = self.solver().closed_loop(
            xs0[None], xref, rng, T, u_init=u0, stepsize_in=s0, plant=plant, plant_substeps=plant_substeps, plant_dt=plant_dt,
            plant_mlp_dtype=plant_mlp_dtype, plant_math_mode=plant_math_mode, solve_period=solve_period, solve_delay=solve_delay, motor_lag=motor_lag,
            disturbance=disturbance, plant_of=plant_of, **more, **({} if controller is None else {"controller": controller}), **({"retire": True} if retire else {}))
        xs, us, info, u_next, s_next, k_next = out[:6]
        xs = xs[0]
        if self.convert_to_enu:
            xs = np.concatenate([x[None], enu2ned(xs[1:], np)], axis=0)
        i = info[0, -1]
        st = OptState(_arr(u_next[0]), np.float32(i[0]), np.float32(s_next[0]), np.float32(i[2]), np.float32(i[3]), np.float32(i[4]),
                      np.float32(i[5]), np.float32(i[6]), np.float32(i[7]))
        ret = (_arr(xs), _arr(us[0]), _arr(info[0]), st, k_next[0].copy())
        erows = ()
        if n_evt:                       # the event chains' values sit behind the Gauss-Markov values, in front of xsub: rows, key and state of each, frameless
            tail = out[-1:] if substep_states else ()
            body = out[:-1] if substep_states else out
            erows = tuple(v[0].copy() for v in body[len(body) - 3 * n_evt:])
            out = body[:len(body) - 3 * n_evt] + tail
        prows = ()
        if drawn:                       # the processes' values sit behind the score, in front of xsub: rows, key and state of each, back in the frame of x
            tail = out[-1:] if substep_states else ()
            body = out[:-1] if substep_states else out
            vals, body = body[len(body) - 3 * len(drawn):], body[:len(body) - 3 * len(drawn)]
            for i, (idx, sgn) in enumerate(drawn):
                rows_, k_, g_ = vals[3 * i][0], vals[3 * i + 1][0], vals[3 * i + 2][0]
                if self.convert_to_enu:
                    rows_, g_ = rows_[..., idx] * sgn, g_[..., idx] * sgn
                prows += (_arr(np.ascontiguousarray(rows_, np.float32)), k_.copy(), _arr(np.ascontiguousarray(g_, np.float32)))
            out = body + tail
        zrow = None
        yvals = ()
        if retire:                      # retired_at and live sit behind the score, in front of xsub
            tail = out[-1:] if substep_states else ()
            body = out[:-1] if substep_states else out
            yvals = (int(body[-2][0]), body[-1].copy())
            out = body[:-2] + tail
        if score is not None:           # the score sits behind every other value, in front of xsub
            zrow = out[-2] if substep_states else out[-1]
            out = out[:-2] + out[-1:] if substep_states else out[:-1]
        if observed:
            o = out[:-1] if substep_states else out
            if hist:
                o, xhist = o[:-1], o[-1][0]
            xmeas, q_next = o[-3][0], o[-2][0]
            ret += (_arr(enu2ned(xmeas, np) if self.convert_to_enu else xmeas), q_next.copy())
            if hist:
                ret += (_arr(enu2ned(xhist, np) if self.convert_to_enu else xhist),)
        if zrow is not None:
            ret += (zrow,)
        ret += yvals
        ret += prows + erows
        if substep_states:
            xsub = out[-1][0]
            ret += (_arr(enu2ned(xsub, np) if self.convert_to_enu else xsub),)
        return ret

# SPEC.md §11c / §11f under convert_to_enu: a world vector (x, y, z) -> (y, x, -z), a body vector (wx, wy, wz) -> (wx, -wy, -wz); each map is its own inverse
_PERM6 = np.array([1, 0, 2, 3, 4, 5])
_SIGN6 = np.array([1, 1, -1, 1, -1, -1], np.float32)
_PERM12 = np.array([1, 0, 2, 4, 3, 5, 6, 7, 8, 9, 10, 11])
_SIGN12 = np.array([1, 1, -1, 1, 1, -1, 1, -1, -1, 1, -1, -1], np.float32)


def _allow_synthetic(flag) -> bool:
    return bool(flag) if flag is not None else os.environ.get("SDEMPC_ALLOW_SYNTHETIC") == "1"


def _pick_model(cfg: MPCConfig, model, allow_synthetic=None) -> RotorSDEModel:
    """The vehicle model: `model` if given; else what `learned_model_params` names (iris_sitl_traj_mpc.yaml:3). A configured file that
    cannot be honoured raises — the synthetic vehicle replaces it only on request (allow_synthetic=True / SDEMPC_ALLOW_SYNTHETIC=1),
    and never silently."""
    if model is not None:
        return model
    lm = os.path.expanduser(cfg.learned_model_params) if cfg.learned_model_params else None
    why = None
    if lm is None:
        why = "the MPC YAML names no learned_model_params"
    elif not os.path.exists(lm):
        why = f"learned_model_params '{lm}' does not exist (the reference's pickles live in the external sde4mbrl repository)"
    elif lm.endswith(".npz"):
        m = RotorSDEModel.load_npz(lm)
        if m.num_motors != cfg.num_motors:
            raise ValueError(f"{lm}: model has {m.num_motors} motors, config has {cfg.num_motors}")
        return m
    elif lm.endswith(".pkl"):
        # a pickle of the external sde4mbrl repo: its layout is not in the reference, so it is read only when the user states the
        # layout in <name>.mapping.yaml beside it (importer.py)
        mp = lm[:-4] + ".mapping.yaml"
        if os.path.exists(mp):
            from .importer import import_sde_pickle
            mdl = import_sde_pickle(lm, mp)
            if mdl.num_motors != cfg.num_motors:
                raise ValueError(f"{lm}: model has {mdl.num_motors} motors, config has {cfg.num_motors}")
            return mdl
        why = f"'{lm}' is a pickle without a layout description '{mp}' (importer.py)"
    else:
        why = f"learned_model_params '{lm}': unknown file type (expected .npz, or .pkl with a .mapping.yaml)"
    if lm is not None and not _allow_synthetic(allow_synthetic):
        raise FileNotFoundError(f"sde4mbrl_px4_amd: {why}. Pass model=..., fix the path, or opt in to the synthetic stand-in vehicle "
                                "with allow_synthetic=True / SDEMPC_ALLOW_SYNTHETIC=1.")
    warnings.warn(f"sde4mbrl_px4_amd: {why}: using this build's SYNTHETIC {'iris' if cfg.num_motors == 4 else 'hexa'} vehicle "
                  "(model.py; random residual weights, not a learned model)", stacklevel=3)
    return synthetic_iris() if cfg.num_motors == 4 else synthetic_hexa()


def load_mpc_problem(mpc_dir: str, convert_to_enu: bool = True, model=None, horizon=None, num_particles=None,
                     trajectory=None, overrides=None, allow_synthetic=None) -> MpcProblem:
    cfg = load_mpc_config(mpc_dir)
    over = dict(overrides or {})
    if horizon is not None:
        over.update(horizon=int(horizon), num_short_dt=int(horizon))
    if num_particles is not None:
        over.update(num_particles=int(num_particles))
    if over:
        cfg = cfg.replace(**over)
    sft = None
    if trajectory is not None:
        sft = trajectory
    elif cfg.trajectory_path:
        path = os.path.expanduser(cfg.trajectory_path)
        if os.path.exists(path):
            sft = TrajectoryCSV(path, ned=not convert_to_enu)
        elif _allow_synthetic(allow_synthetic):
            # the shipped YAMLs point at CSVs of the external repo: analytic lemniscate instead, on request only
            warnings.warn(f"sde4mbrl_px4_amd: trajectory_path '{path}' does not exist: using the analytic lemniscate stand-in", stacklevel=2)
            sft = workload.lemniscate_state
        else:
            raise FileNotFoundError(f"sde4mbrl_px4_amd: trajectory_path '{path}' does not exist. Pass trajectory=..., fix the path, or opt "
                                    "in to the analytic lemniscate with allow_synthetic=True / SDEMPC_ALLOW_SYNTHETIC=1.")
    return MpcProblem(cfg=cfg, model=_pick_model(cfg, model, allow_synthetic), state_from_traj=sft, convert_to_enu=bool(convert_to_enu))


def load_mpc_from_cfgfile(mpc_dir: str, convert_to_enu: bool = True, **kw):
    """Reference-shaped factory (sde_control.py:685)."""
    prob = load_mpc_problem(mpc_dir, convert_to_enu=convert_to_enu, **kw)
    cfg_dict = {"_time_steps": prob.cfg.time_steps, "horizon": prob.cfg.horizon, "num_particles": prob.cfg.num_particles,
                "cost_params": {"uref": list(prob.cfg.uref)}, "_problem": prob}
    sft = None
    if prob.state_from_traj is not None:
        def sft(t, _f=prob.state_from_traj):
            return _arr(np.asarray(_f(np.float64(t)), np.float32).reshape(13))
    return cfg_dict, (prob.m_reset, prob.m_mpc), sft, None
