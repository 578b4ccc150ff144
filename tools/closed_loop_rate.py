"""Rate of the batched closed loop (SPEC.md §11, sdempc_closed_loop_batch) against the same ticks driven from Python.

  1. Per-tick wall time at B = 1 (shipped P = 1 YAML, C1): MpcProblem.simulate over T ticks against a Python loop of m_mpc whose host step
     takes the solver's own one-step prediction xevol[1] as the next state (plus the host-side key split of the plant noise). That host step
     costs next to nothing (no model evaluation on the host: the package has none, and the CPU oracle is test infrastructure), so the
     ratio is a lower bound on what the device loop saves. The two follow different trajectories from the same start, so iteration counts
     and kernel times differ a little; the kernel trace below splits the closed loop's own tick.
  2. Episode-ticks per second at C2 (arithmetic of bench.py: f32x3 / fast) with B = 12,288, against one batch solve of the same B.
  3. --plant one | per-episode [--substeps N]: the same two measurements against a separate plant (SPEC.md §11a) — one perturbed vehicle for every
     episode, or one per episode (domain randomisation); `own` (default) is the plain loop, the handle's model as the plant. The plants' blobs
     are made before the clock starts (RotorSDEModel.perturbed + to_blob is host work of the caller, not of the loop).
     --repeats R times the C2 loop R times on one handle (run-to-run spread of one session).
  4. --small-batch B: ticks per second of a SMALL loop (C1, B episodes, --ticks ticks, one hold window), where a tick is a millisecond-scale solve and
     the launches around it are a visible share — the size at which one plant launch per solve period (SPEC.md §11b) matters. --plant self is the
     handle's own model through sdempc_closed_loop_batch_plant; --timed sends the call through sdempc_closed_loop_batch_timed even at --period 1
     --delay 0 --lag 0 (the same arithmetic, one period kernel per tick); --period S --delay D --lag ALPHA set the timing. Nothing else runs in this mode.
     With SDEMPC_LIB naming a library of the parent commit the default keywords measure that commit's entry points from the same process setup.
  5. --disturbance / --plant-switch K: the same loops with a scenario (SPEC.md §11c, sdempc_closed_loop_batch_scenario) — a random disturbance row per tick
     and episode, and / or every episode changing its plant at tick K (--plant self or one: to one perturbed vehicle; per-episode: to its neighbour's).
     They apply to --small-batch and to the C2 loop, where --timed / --period / --delay / --lag now apply too (one reference window per solve).
  6. --rate-loop: the same loops flown through the rate-setpoint interface (SPEC.md §11d, sdempc_closed_loop_batch_rate): a PI rate loop with the model's own mixer on
     every plant substep (the control table is re-formed on every substep). Applies to --small-batch and to the C2 loop.
  7. --fault / --substep-states: the same loops through sdempc_closed_loop_batch_fault (SPEC.md §11e) — a fault schedule with a row per tick and episode (every
     episode loses one motor at tick T / 2, the motor drawn per episode, and flies a biased one throughout) and / or the state after every plant substep copied back.
     Applies to --small-batch and to the C2 loop; either one makes the call the timed one.
  8. --observe: the same loops on a measured state (SPEC.md §11f, sdempc_closed_loop_batch_observed) — a noise and a bias row per solve and episode, and every
     episode's estimator dropping one solve in four. Applies to --small-batch and to the C2 loop; it makes the call the timed one.
  9. --age A [--renorm]: with --observe, the estimate of every valid solve is up to A plant substeps old (SPEC.md §11g, sdempc_closed_loop_batch_aged) — an age per
     solve and episode drawn from 0 .. A, a history of A rows — and --renorm scales its attitude to unit length. A <= min(period, T) * substeps. With A > 0 the run
     takes the §11e kernels with a substep region in the chunk.
 10. --score [--no-outputs] [--score-substeps]: the same loops scored on the device (SPEC.md §11h, sdempc_closed_loop_batch_scored) — a radius of 1 m, a tilt of 0.6 rad
     and a rate of 6 rad/s around a hover target per tick and episode (the target rows are staged per chunk), one scoring launch per chunk; --score-substeps scores every
     plant substep state (a substep region in the chunk); --no-outputs passes NULL for the per-row outputs, so nothing but the continuation values and B x 64 bytes of
     score come back. Applies to --small-batch and to the C2 loop; it makes the call the timed one. The last run's score_summary is printed.
 11. --dist-process / --bias-process: gusts and estimator bias drawn on the device from key chains (SPEC.md §11i, sdempc_closed_loop_batch_drawn) instead of host rows — a
     first-order Gauss-Markov process per component and episode, coefficients per episode: --dist-process one step per control tick (deviations around 1 m/s^2 and
     1.5 rad/s^2, correlation times around 0.3 s; with --disturbance as well the host rows are the scheduled part the process is added to), --bias-process one step
     per solve with --observe, whose meas_bias rows it REPLACES (noise and dropouts stay host rows). Apply to --small-batch and to the C2 loop; either makes the call
     the timed one. So `--disturbance --observe` against `--dist-process --observe --bias-process` is host rows against keys for the same two ingredients.
 12. --track: the reference windows cut on the device from a trajectory table (SPEC.md §11j, sdempc_closed_loop_batch_tracked) instead of a host xref array — the
     lemniscate as a periodic table of 161 knots, every episode entering it at its own phase and flying it at its own rate (0.8 .. 1.2); with --score the targets are cut
     from the table as well. It makes the call the timed one. --per-episode-xref gives --small-batch the route it replaces: a host array with a window per solve and
     episode on the same lemniscate (the C2 loop always stages one). So `--timed --per-episode-xref` against `--track` is the array route against the table.
 13. --fault-process / --drop-process: motor faults and estimator dropouts drawn on the device from key chains (SPEC.md §11k, sdempc_closed_loop_batch_events) instead of
     host rows — --fault-process a Markov chain per episode and motor with two modes (dead, and weakened to 60 %), around one failure per 4 s of flight and motor,
     lasting 1 s on average, thresholds per episode (with --fault as well the host rows are the schedule a healthy motor reads); --drop-process, with --observe, a
     two-state chain per episode stepped per solve (one solve in four dropped, bursts of two solves), whose flags REPLACE the meas_valid rows (noise and bias stay host
     rows). Apply to --small-batch and to the C2 loop; either makes the call the timed one. So `--fault --observe` against `--fault-process --observe --drop-process`
     is host rows against keys for the same two ingredients.
 14. --controller geo: the same loops flown by the geometric baseline controller (SPEC.md §11l, sdempc_closed_loop_batch_baseline) in place of the MPC's solves — gains
     calibrated for the model (GeometricController.for_model), one set for every episode, through the rate loop of --rate-loop (implied). Applies to --small-batch and
     to the C2 loop; everything above still applies, so the same command with and without it is the paired comparison of SPEC.md §11l. The "one batch solve" figure
     beside the C2 loop is then the MPC's solve, for scale: the baseline's period has no solve in it.
 15. --ensemble G E: with --score, the per-row ensemble histories over the episodes (SPEC.md §11m, sdempc_closed_loop_batch_ensemble) — G cohorts dealt out round robin,
     E edges per channel (position error up to 2 m, velocity error up to 4 m/s, tilt up to 60 degrees, rate up to 8 rad/s), over = alive. After every chunk's scoring
     launch the key kernel runs twice more (partial words per block of 256 episodes, then the blocks in order) and R x G x (20 + 4 E) words come back. Applies to
     --small-batch and to the C2 loop; the same command without it takes the entry point it took before. The last run's survival and RMS position error per row of
     cohort 0 are printed.
 16. --retire [--failed-at-entry F]: with --score, failed episodes are retired at the next solve-period boundary and only the live set is solved (SPEC.md §11n,
     sdempc_closed_loop_batch_retire) — scoring once per period, n_live read back in front of every solve (one synchronisation per period), the solve on the gathered
     live set. --failed-at-entry F marks the fraction F of the episodes (every episode b with b mod 1000 < 1000 F) as failed in score_in, with or without --retire:
     without it those episodes are flown and solved like the rest, which is the baseline the gain is measured against. Applies to --small-batch and to the C2
     loop; the same command without --retire takes the entry point it took before. The last run's retire_summary is printed. --score-wide switches every threshold
     of --score off, so that no finite episode fails: with --retire that leaves the per-period read-back and scoring as the only difference, and with
     --failed-at-entry F exactly the marked share is retired.
usage: python tools/closed_loop_rate.py [--ticks 40] [--c2-ticks 3] [--skip-c2] [--skip-b1] [--plant own|self|one|per-episode] [--substeps N] [--repeats R]
                                        [--small-batch B] [--timed] [--period S] [--delay D] [--lag ALPHA] [--disturbance] [--plant-switch K] [--rate-loop]
                                        [--fault] [--substep-states] [--observe] [--age A] [--renorm]
                                        [--score] [--no-outputs] [--score-substeps] [--dist-process] [--bias-process] [--track] [--per-episode-xref]
                                        [--fault-process] [--drop-process] [--controller geo] [--ensemble G E]
                                        [--retire] [--failed-at-entry F] [--score-wide]
Run under `rocprofv3 --kernel-trace --stats -- python tools/closed_loop_rate.py --skip-c2 --loop-only` for the kernel split of a tick
(solve kernel against key schedule, noise, plant step)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from sde4mbrl_px4_amd import load_mpc_config, prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.sde_mpc_design import MpcProblem
from sde4mbrl_px4_amd.solver import SdeMpcSolver

ap = argparse.ArgumentParser()
ap.add_argument("--ticks", type=int, default=40)
ap.add_argument("--c2-ticks", type=int, default=3)
ap.add_argument("--skip-c2", action="store_true")
ap.add_argument("--loop-only", action="store_true", help="B = 1 closed loops only (no Python-driven comparison): for a kernel trace")
ap.add_argument("--skip-b1", action="store_true", help="skip the B = 1 part")
ap.add_argument("--plant", choices=("own", "self", "one", "per-episode"), default="own")
ap.add_argument("--substeps", type=int, default=1)
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--small-batch", type=int, default=0, help="C1 with this many episodes: ticks/s of a loop whose ticks are millisecond-scale solves")
ap.add_argument("--timed", action="store_true", help="--small-batch: go through sdempc_closed_loop_batch_timed whatever the timing")
ap.add_argument("--period", type=int, default=1)
ap.add_argument("--delay", type=int, default=0)
ap.add_argument("--lag", type=float, default=0.0)
ap.add_argument("--disturbance", action="store_true", help="a disturbance row per tick and episode (SPEC.md §11c)")
ap.add_argument("--plant-switch", type=int, default=-1, metavar="K", help="every episode changes its plant at tick K (SPEC.md §11c; needs --plant self, one or per-episode)")
ap.add_argument("--rate-loop", action="store_true", help="fly the thrust and body-rate setpoints through a PI rate loop (SPEC.md §11d)")
ap.add_argument("--fault", action="store_true", help="a per-motor fault row per tick and episode (SPEC.md §11e)")
ap.add_argument("--substep-states", action="store_true", help="copy the state after every plant substep back (SPEC.md §11e)")
ap.add_argument("--observe", action="store_true", help="solve from a measured state: noise, bias and dropouts per solve and episode (SPEC.md §11f)")
ap.add_argument("--age", type=int, default=-1, metavar="A", help="with --observe: estimates up to A plant substeps old, an age per solve and episode (SPEC.md §11g)")
ap.add_argument("--renorm", action="store_true", help="with --observe: renormalise the measured attitude (SPEC.md §11g)")
ap.add_argument("--score", action="store_true", help="score every episode on the device (SPEC.md §11h)")
ap.add_argument("--no-outputs", action="store_true", help="with --score: NULL per-row outputs, only the continuation values and the score come back")
ap.add_argument("--score-substeps", action="store_true", help="with --score: score every plant substep state instead of every tick state")
ap.add_argument("--dist-process", action="store_true", help="gusts drawn on the device, one Gauss-Markov step per control tick (SPEC.md §11i)")
ap.add_argument("--bias-process", action="store_true", help="with --observe: the estimator bias drawn on the device, one Gauss-Markov step per solve, instead of meas_bias rows (SPEC.md §11i)")
ap.add_argument("--track", action="store_true", help="reference windows (and score targets) cut on the device from a trajectory table, per-episode phase and rate (SPEC.md §11j)")
ap.add_argument("--per-episode-xref", action="store_true", help="--small-batch: a host xref array with a lemniscate window per solve and episode instead of one hold window")
ap.add_argument("--fault-process", action="store_true", help="motor faults drawn on the device, one step of a Markov chain per motor and control tick (SPEC.md §11k)")
ap.add_argument("--drop-process", action="store_true", help="with --observe: estimator dropouts drawn on the device, one step per solve, instead of meas_valid rows (SPEC.md §11k)")
ap.add_argument("--controller", choices=("mpc", "geo"), default="mpc", help="geo: the geometric baseline controller in place of the solves, through the rate loop (SPEC.md §11l)")
ap.add_argument("--ensemble", type=int, nargs=2, metavar=("G", "E"), help="with --score: per-row ensemble words over the episodes, G cohorts and E edges per channel (SPEC.md §11m)")
ap.add_argument("--score-wide", action="store_true", help="with --score: every threshold off (infinite radius, tilt and rate), so that no finite episode fails")
ap.add_argument("--retire", action="store_true", help="with --score: retire failed episodes at the next solve-period boundary and solve only the live set (SPEC.md §11n)")
ap.add_argument("--failed-at-entry", type=float, default=0.0, metavar="F", help="with --score: mark this fraction of the episodes as failed in score_in")
a = ap.parse_args()
if (a.retire or a.failed_at_entry or a.score_wide) and not a.score:
    ap.error("--retire / --failed-at-entry / --score-wide need --score")
if not 0.0 <= a.failed_at_entry <= 1.0:
    ap.error("--failed-at-entry: F in [0, 1]")
if a.ensemble and not a.score:
    ap.error("--ensemble needs --score")
if a.ensemble and not (1 <= a.ensemble[0] <= 16 and 0 <= a.ensemble[1] <= 16):
    ap.error("--ensemble: G in 1 .. 16, E in 0 .. 16")
if a.controller == "geo":
    a.rate_loop = True
if a.drop_process and not a.observe:
    ap.error("--drop-process needs --observe")
if a.track and a.per_episode_xref:
    ap.error("--track replaces the xref array: not with --per-episode-xref")
if a.bias_process and not a.observe:
    ap.error("--bias-process needs --observe")
if (a.age >= 0 or a.renorm) and not a.observe:
    ap.error("--age / --renorm need --observe")
if (a.no_outputs or a.score_substeps) and not a.score:
    ap.error("--no-outputs / --score-substeps need --score")
model = synthetic_iris()
DT_TICK = 0.05      # the first step length of the shipped configurations: the time between two control ticks
if a.plant == "own" and a.substeps != 1:
    ap.error("--substeps needs --plant one or per-episode")


def plant_kw(B):
    """keyword arguments of closed_loop / simulate for --plant: blobs of vehicles perturbed by +-20 % in mass, inertia, thrust curve and W2"""
    if a.plant == "own":
        return {}
    if a.plant == "self":
        return {"plant": model.to_blob(), "plant_substeps": a.substeps}
    rng = np.random.default_rng(1)
    n = 1 if a.plant == "one" else B
    blobs = [model.perturbed(rng, mass=0.2, inertia=0.2, thrust=0.2, residual=0.2).to_blob() for _ in range(n)]
    return {"plant": blobs[0] if a.plant == "one" else blobs, "plant_substeps": a.substeps}


def scenario_kw(kw, B, T):
    """kw plus the schedules of --disturbance / --plant-switch for a call of T ticks"""
    kw = dict(kw)
    if a.rate_loop:
        from sde4mbrl_px4_amd.solver import RateLoop
        kw["rate_loop"] = RateLoop(kp=[0.03, 0.03, 0.08], ki=[0.3, 0.3, 0.5], integ_limit=0.05)
    if a.controller == "geo":
        from sde4mbrl_px4_amd.solver import GeometricController
        kw["controller"] = GeometricController.for_model(model, kp=[4.0, 4.0, 6.0], kv=[2.5, 2.5, 3.25], max_acc=7.0, attctrl_tau=0.2)
    if a.fault:
        from sde4mbrl_px4_amd.solver import fault_schedule
        rng = np.random.default_rng(6)
        f = fault_schedule(T, B, model.num_motors)
        f[T // 2:, np.arange(B), rng.integers(0, model.num_motors, B)] = (0.0, 0.0)
        f[:, np.arange(B), rng.integers(0, model.num_motors, B), 1] += np.float32(0.03)
        kw["fault"] = f
    if a.substep_states:
        kw["substep_states"] = True
    if a.observe:
        Ns = -(-T // max(a.period, 1))
        rng = np.random.default_rng(7)
        scale = np.repeat(np.array([0.05, 0.1, 0.02, 0.05], np.float32), 3)          # p [m], v [m/s], theta [rad], omega [rad/s]
        kw["meas_noise"] = (scale * rng.uniform(0.5, 1.5, (Ns, B, 12))).astype(np.float32)
        kw["meas_bias"] = (scale * rng.uniform(-0.5, 0.5, (Ns, B, 12))).astype(np.float32)
        kw["meas_valid"] = (rng.integers(0, 4, (Ns, B)) != 0).astype(np.int32)
        kw["meas_keys"] = np.stack([prng.PRNGKey(9000 + b) for b in range(B)])
        if a.age >= 0:
            kw["meas_age"] = rng.integers(0, a.age + 1, (Ns, B)).astype(np.int32)
            kw["meas_age_max"] = a.age
        if a.renorm:
            kw["meas_renorm"] = True
    if a.dist_process or a.bias_process:
        from sde4mbrl_px4_amd.solver import GaussMarkov
        rng = np.random.default_rng(8)
        if a.dist_process:
            gm = GaussMarkov(np.array([1.0, 1.0, 0.6, 1.5, 1.5, 1.0]) * rng.uniform(0.5, 1.5, (B, 6)), rng.uniform(0.1, 0.6, (B, 6)), DT_TICK)
            kw.update(dist_process=gm, dist_keys=np.stack([prng.PRNGKey(20000 + b) for b in range(B)]), dist_state_in=gm.stationary_state(rng, B))
        if a.bias_process:
            scale = np.repeat(np.array([0.05, 0.1, 0.02, 0.05]), 3)
            gm = GaussMarkov(0.3 * scale * rng.uniform(0.5, 1.5, (B, 12)), rng.uniform(0.3, 2.0, (B, 12)), DT_TICK * max(a.period, 1))
            kw.pop("meas_bias")
            kw.update(bias_process=gm, bias_keys=np.stack([prng.PRNGKey(30000 + b) for b in range(B)]), bias_state_in=gm.stationary_state(rng, B))
    if a.fault_process or a.drop_process:
        from sde4mbrl_px4_amd.solver import Dropouts, FaultProcess
        rng = np.random.default_rng(12)
        m = model.num_motors
        if a.fault_process:
            modes = np.zeros((B, m, 2, 2), np.float32)
            modes[:, :, 1, 0] = rng.uniform(0.5, 0.7, (B, m))
            fp = FaultProcess.from_rates(rng.uniform(0.08, 0.17, (B, m, 2)), rng.uniform(0.5, 1.5, (B, m, 2)), DT_TICK, modes)
            kw.update(fault_process=fp, fault_keys=np.stack([prng.PRNGKey(40000 + b) for b in range(B)]))
        if a.drop_process:
            kw.pop("meas_valid")
            kw.update(drop_process=Dropouts(rng.uniform(0.12, 0.22, B), rng.uniform(0.4, 0.6, B)), drop_keys=np.stack([prng.PRNGKey(50000 + b) for b in range(B)]))
    if a.score:
        from sde4mbrl_px4_amd.solver import Score
        kw["score"] = Score(substeps=a.score_substeps) if a.score_wide else Score(pos_radius=1.0, tilt_max=0.6, rate_max=6.0, substeps=a.score_substeps)
        kw["score_ref"] = "track" if a.track else np.ascontiguousarray(np.broadcast_to(np.asarray(W.HOVER, np.float32), (T, B, 13)))
        if a.no_outputs:
            kw["outputs"] = False
        if a.failed_at_entry > 0.0:
            from sde4mbrl_px4_amd.solver import score_init
            z = score_init(B)
            z["first_fail_row"][(np.arange(B) % 1000) < int(round(1000 * a.failed_at_entry))] = 0
            kw["score_in"] = z
        if a.retire:
            kw["retire"] = True
        if a.ensemble:
            from sde4mbrl_px4_amd.solver import Ensemble
            G_, E_ = a.ensemble
            grid = np.arange(1, E_ + 1) / max(E_, 1)
            kw["ensemble"] = Ensemble(pos_edges=2.0 * grid, vel_edges=4.0 * grid, tilt_edges_deg=60.0 * grid, rate_edges=8.0 * grid, over="alive", n_cohorts=G_)
            kw["cohort"] = (np.arange(B) % G_).astype(np.int32)
    if a.track:
        kw.update(track_kw(B))
    if a.disturbance:
        kw["disturbance"] = np.random.default_rng(2).uniform(-2.0, 2.0, (T, B, 6)).astype(np.float32)
    if a.plant_switch >= 0:
        if a.plant == "own":
            ap.error("--plant-switch needs --plant self, one or per-episode")
        if isinstance(kw["plant"], list):
            before, after = np.arange(B), (np.arange(B) + 1) % B
        else:
            kw["plant"] = [kw["plant"], model.perturbed(np.random.default_rng(5), mass=0.2, inertia=0.2, thrust=0.2, residual=0.2).to_blob()]
            before, after = np.zeros(B), np.ones(B)
        kw["plant_of"] = np.stack([before if k < a.plant_switch else after for k in range(T)]).astype(np.int32)
    return kw


def track_kw(B):
    """keyword arguments of closed_loop for --track: the lemniscate as a periodic table, per-episode phase and rate"""
    from sde4mbrl_px4_amd.solver import Trajectory
    rng = np.random.default_rng(11)
    return dict(track=Trajectory.from_function(W.lemniscate_state, 0.0, 8.0, 161, period=8.0), track_phase=(0.05 * (np.arange(B) % 160)).astype(np.float32),
                track_rate=rng.uniform(0.8, 1.2, B).astype(np.float32))


def lemniscate_windows(cfg, B, T):
    """xref f32[Ns][B][H+1][13]: a moving window per episode and solve, the largest staging the loop does"""
    return np.stack([np.stack([W.reference_window(0.05 * (b % 160) + k * float(cfg.time_steps[0]), cfg.time_steps) for b in range(B)]) for k in range(0, T, a.period)])


def timing_kw(cfg, B):
    if not (a.timed or a.period != 1 or a.delay or a.lag):
        return {}
    return dict(solve_period=a.period, solve_delay=a.delay, motor_lag=a.lag, u_act_in=np.tile(np.asarray(cfg.uref, np.float32)[: cfg.num_motors], (B, 1)))


tag = "" if a.plant == "own" else f" plant={a.plant} substeps={a.substeps}"
if a.timed or a.period != 1 or a.delay or a.lag:
    tag += f" timed S={a.period} D={a.delay} alpha={a.lag}"
if a.disturbance:
    tag += " disturbance"
if a.plant_switch >= 0:
    tag += f" plant-switch at {a.plant_switch}"
if a.controller == "geo":
    tag += " controller=geo"
if a.rate_loop:
    tag += " rate-loop"
if a.fault:
    tag += " fault"
if a.substep_states:
    tag += " substep-states"
if a.observe:
    tag += " observe"
if a.age >= 0:
    tag += f" age<={a.age}"
if a.renorm:
    tag += " renorm"
if a.dist_process:
    tag += " dist-process"
if a.bias_process:
    tag += " bias-process"
if a.fault_process:
    tag += " fault-process"
if a.drop_process:
    tag += " drop-process"
if a.track:
    tag += " track"
if a.per_episode_xref:
    tag += " per-episode-xref"
if a.score:
    tag += " score" + ("/substeps" if a.score_substeps else "") + ("/wide" if a.score_wide else "") + (" no-outputs" if a.no_outputs else "")
if a.ensemble:
    tag += f" ensemble G={a.ensemble[0]} E={a.ensemble[1]}"
if a.failed_at_entry:
    tag += f" failed-at-entry={a.failed_at_entry:g}"
if a.retire:
    tag += " retire"


def report_score(out, T, pk_ens=None):
    """score_summary of a scored call's result (the score sits behind every other value, in front of xsub)"""
    if not a.score:
        return
    from sde4mbrl_px4_amd.solver import score_summary
    at = -1 - (1 if a.substep_states else 0) - 3 * (int(a.dist_process) + int(a.bias_process) + int(a.fault_process) + int(a.drop_process))      # the score sits in front of the process values and of xsub
    if a.retire:               # (retired_at and live sit behind the score and the ensemble words)
        from sde4mbrl_px4_amd.solver import retire_summary
        r = retire_summary(out[at - 1], out[at], out[at - 1].shape[0])
        print(f"  retire: {r['solves_run']} solves run, {r['solves_saved']} saved ({100 * r['saved_share']:.1f} %), {r['retired']} episodes retired, "
              f"{r['retired_at_entry']} of them at entry; live per solve " + " ".join(str(int(v)) for v in out[at]), flush=True)
        at -= 2
    if a.ensemble:             # (the ensemble words sit right behind the score)
        from sde4mbrl_px4_amd.solver import ensemble_summary
        e = ensemble_summary(out[at], pk_ens)
        print("  ensemble, cohort 0: survival per row " + " ".join(f"{v:.3f}" for v in e["survival"][:, 0]) + "; RMS position error [m] " +
              " ".join(f"{v:.3f}" for v in e["rms_pos"][:, 0]), flush=True)
        at -= 1
    s = score_summary(out[at], solves=-(-T // max(a.period, 1)))
    print(f"  score: success {s['success_rate']:.3f}, median RMS position error {float(np.median(s['rms_pos_err'])):.3f} m, worst tilt {s['worst_tilt_deg']:.1f} deg, "
          f"{s['mean_steps']:.2f} iterations and {s['mean_ls_trials']:.2f} trials per solve", flush=True)

if a.small_batch:
    cfg = load_mpc_config(os.path.join(ROOT, "configs", "c1_iris_posctrl_h20_p32.yaml"))
    B, T = a.small_batch, a.ticks
    x0 = W.random_initial_states(B, 3)
    hold = W.constant_reference(W.HOVER, cfg.horizon)
    keys = prng.split(prng.PRNGKey(10), B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    kw = {**plant_kw(B), **timing_kw(cfg, B)}
    window = lambda n: None if a.track else lemniscate_windows(cfg, B, n) if a.per_episode_xref else hold      # noqa: E731
    S.closed_loop(x0, window(2 * a.period), keys, 2 * a.period, **scenario_kw(kw, B, 2 * a.period))       # warm-up: device buffers, workspaces
    kw = scenario_kw(kw, B, T)
    xr = window(T)
    for rep in range(a.repeats):
        t = time.perf_counter()
        out = S.closed_loop(x0, xr, keys, T, **kw)
        dt = time.perf_counter() - t
        print(f"C1 B={B} T={T}{tag}: {T / dt:8.1f} ticks/s ({B * T / dt:9.1f} episode-ticks/s, {dt * 1e3 / T:.3f} ms/tick)", flush=True)
    report_score(out, T, kw.get("ensemble"))
    S.close()
    sys.exit(0)

for name in (() if a.skip_b1 else ("iris_traj_shipped_h20_p1", "c1_iris_posctrl_h20_p32")):
    cfg = load_mpc_config(os.path.join(ROOT, "configs", name + ".yaml"))
    prob = MpcProblem(cfg=cfg, model=model, state_from_traj=W.lemniscate_state if cfg.trajectory_path else None)
    x = W.random_initial_states(1, 4)[0]
    rng = prng.PRNGKey(10)
    pk = plant_kw(1)
    if pk:
        pk["plant"] = pk["plant"] if a.plant == "one" else pk["plant"][0]
    prob.simulate(x, rng, 3, **pk)                           # warm-up: device buffers, workspaces
    t = time.perf_counter()
    xs, us, info, st, _ = prob.simulate(x, rng, a.ticks, **pk)
    dev = (time.perf_counter() - t) * 1e3 / a.ticks
    if a.loop_only:
        print(f"{name:26s} B=1{tag}: closed_loop {dev:7.3f} ms/tick over {a.ticks} ticks", flush=True)
        continue
    # the same ticks from Python: m_mpc, the key split of the plant noise, and the predicted state after one step as the next state
    st = prob.m_reset(x=x, rng=rng)
    r = rng.copy()
    xk = x.copy()
    t = time.perf_counter()
    for k in range(a.ticks):
        uo, st, r1, xevol = prob.m_mpc(xk, r, st, curr_t=k * float(cfg.time_steps[0]))
        r, p = prng.split(r1, 2)
        xk = np.asarray(xevol)[1].astype(np.float32)         # (in the frame of x, as m_mpc returns it)
    host = (time.perf_counter() - t) * 1e3 / a.ticks
    print(f"{name:26s} B=1: closed_loop {dev:7.3f} ms/tick; m_mpc loop {host:7.3f} ms/tick (x{host / dev:.2f})", flush=True)

if not a.skip_c2:
    cfg = load_mpc_config(os.path.join(ROOT, "configs", "c2_iris_traj_h50_p128.yaml")).replace(mlp_dtype="f32x3", math_mode="fast")
    B, T = 12288, a.c2_ticks
    x0 = W.random_initial_states(B, 3)
    xref = lemniscate_windows(cfg, B, 1 if a.track else T)   # (--track: one window per episode for the batch solve; the loop cuts its own)
    keys = prng.split(prng.PRNGKey(10), B)
    S = SdeMpcSolver(cfg, model, max_batch=B)
    yk, i0 = S.reset()
    u0 = np.tile(yk[None], (B, 1, 1))
    s0 = np.full(B, i0["stepsize"], np.float32)
    S.solve_keys(x0, xref[0], keys, u0, s0)                 # warm-up
    t = time.perf_counter()
    S.solve_keys(x0, xref[0], keys, u0, s0)
    one = time.perf_counter() - t
    pk = scenario_kw({**plant_kw(B), **timing_kw(cfg, B)}, B, T)
    for rep in range(a.repeats):
        t = time.perf_counter()
        out = S.closed_loop(x0, None if a.track else xref, keys, T, u_init=u0, stepsize_in=s0, **pk)
        loop = time.perf_counter() - t
        print(f"C2 f32x3/fast B={B}{tag}: closed_loop {B * T / loop:8.1f} episode-ticks/s ({loop / T:.3f} s/tick, T = {T}); one batch solve_keys "
              f"{B / one:8.1f} solves/s ({one:.3f} s); ratio {(B * T / loop) / (B / one):.3f}", flush=True)
    report_score(out, T, pk.get("ensemble"))
    S.close()
