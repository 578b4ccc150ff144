"""Rate of the predicted-outcome reducer (SPEC.md §12c) against the only route that existed before it, and of the kernel that hosts it against the parent commit's.

Configuration C2 (H = 50, P = 128) in the arithmetic bench.py reports (f32x3 / fast) at B = 12,288 — or, where the device's memory does not allow that, the
largest halving of it that does; the B used is printed. One process; after one warm-up of every step, --reps (5) repetitions in which the steps are INTERLEAVED
(every other repetition the two libraries trade places), each step timed by a host clock around work that ends in a device synchronise and guarded by its own
watchdog thread (--step-timeout seconds: the process then exits with 124 and starts nothing more). Per step: the median and the max-to-min spread.

  (a) outcome_dev with all eight outputs (two quantiles), with the six that need no selection, and with first_fail + fail_step alone (the failure curve: the
      sweep phase only). Against traj_to_canonical_dev of the same tensor — THE YARDSTICK, the device half of the route via rollout(want_traj=True): tensor read
      once and written once (the copy to the host and the NumPy loop come on top of it and are not timed).
  (b) with --parent-lib PATH: the noise, tube, risk and bands forms of the hosting kernel on a second handle bound to a library built from the parent commit, in
      the same repetitions. Each new median has to lie inside the parent's own max-to-min spread.
usage: python tools/outcome_rate.py [--batch 12288] [--reps 5] [--step-timeout 60] [--parent-lib PATH] [--out FILE]"""
import argparse
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12288)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=60)
ap.add_argument("--parent-lib", default=None, help="libsdempc.so of the parent commit: times its noise, tube, risk and bands forms beside the new ones")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()

import torch

from sde4mbrl_px4_amd import load_mpc_config, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import Score, SdempcError, SdeMpcSolver

if not torch.cuda.is_available():
    sys.exit("tools/outcome_rate.py: no GPU: nothing is measured without one")

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _expired():
    print(f"tools/outcome_rate.py: a step ran past its {a.step_timeout} s: stopping here", flush=True)
    os._exit(124)


def step(fn):
    """one step under its own watchdog thread: host clock around the call and the synchronise that ends it, in milliseconds"""
    dog = threading.Timer(a.step_timeout, _expired)
    dog.daemon = True
    dog.start()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    dog.cancel()
    return dt


cfg = load_mpc_config(os.path.join(ROOT, "configs", "c2_iris_traj_h50_p128.yaml")).replace(mlp_dtype="f32x3", math_mode="fast")
model = synthetic_iris()
H, P, m = cfg.horizon, cfg.num_particles, cfg.num_motors
C = (H + 1) * 13


def make(B, lib_path=None):
    return SdeMpcSolver(cfg, model, max_batch=B, lib_path=lib_path)


B = a.batch
while True:
    try:
        S = make(B)
        st = torch.cuda.current_stream().cuda_stream
        keys = np.stack([np.arange(B, dtype=np.uint32) * 0, np.arange(B, dtype=np.uint32) + 1], axis=1).astype(np.uint32)
        noise = torch.empty(S.lib.sdempc_noise_dev_floats(S._h, B), dtype=torch.float32, device="cuda")
        x0 = torch.from_numpy(W.random_initial_states(B, 0)).cuda()
        xref = torch.from_numpy(np.stack([W.reference_window(0.05 * (b % 160), cfg.time_steps) for b in range(B)])).cuda()
        u = torch.from_numpy(np.tile(np.asarray(cfg.uref, np.float32), (B, H, 1))).cuda()
        cost = torch.empty(B, dtype=torch.float32, device="cuda")
        rows = torch.empty((B, H + 1, 13), dtype=torch.float32, device="cuda")       # the rollout's mean rows: the observation and the risk's centre rows
        canon = torch.empty((B, P, H + 1, 13), dtype=torch.float32, device="cuda")
        planes = [torch.empty((B, H + 1, 13), dtype=torch.float32 if k < 4 else torch.int32, device="cuda") for k in range(5)]
        q = torch.empty((B, 8, H + 1, 13), dtype=torch.float32, device="cuda")
        below, at = (torch.empty((B, H + 1, 13), dtype=torch.int32, device="cuda") for _ in range(2))
        o_bufs = dict(words=torch.empty((B, P, 11), dtype=torch.int32, device="cuda"), fail_step=torch.empty((B, H, 5), dtype=torch.int32, device="cuda"),
                      first_fail=torch.empty((B, H + 1), dtype=torch.int32, device="cuda"), cause_ever=torch.empty((B, 4), dtype=torch.int32, device="cuda"),
                      chan_stat=torch.empty((B, H, 4, 3), dtype=torch.float32, device="cuda"), chan_q=torch.empty((B, H, 4, 2), dtype=torch.float32, device="cuda"),
                      agg_stat=torch.empty((B, 4, 3), dtype=torch.float32, device="cuda"), agg_q=torch.empty((B, 4, 2), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        S.noise_from_keys_dev(keys, noise.data_ptr(), st)
        S.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise.data_ptr(), cost.data_ptr(), rows.data_ptr(), True, st)      # (allocates the workspaces)
        torch.cuda.synchronize()
        break
    except (SdempcError, RuntimeError) as e:
        if B <= 256 or "memory" not in str(e).lower():
            raise
        say(f"B = {B}: {str(e).splitlines()[0]} -> halving")
        S = noise = x0 = xref = u = cost = rows = canon = planes = q = below = at = o_bufs = None
        torch.cuda.empty_cache()
        B //= 2

lo = np.array([-2, -2, -2, -3, -3, -3, -np.inf, -np.inf, -np.inf, -np.inf, -4, -4, -4], np.float32)
hi = -lo
box = np.array([0.05, 0.05, 0.05, 0.3, 0.3, 0.3, np.inf, np.inf, np.inf, np.inf, 1.0, 1.0, 1.0], np.float32)
rlo = torch.from_numpy(np.tile(-box, (B, 1))).cuda()
rhi = torch.from_numpy(np.tile(box, (B, 1))).cuda()
Q3 = (0.05, 0.5, 0.95)
tensor_bytes = 4 * S.lib.sdempc_traj_dev_floats(S._h, B)
say(f"device: {torch.cuda.get_device_name(0)}; C2 (H = {H}, P = {P}, {(P + 31) // 32} particle groups), mlp_dtype f32x3, math_mode fast, B = {B}"
    + ("" if B == a.batch else f" (asked for {a.batch})"))
say(f"particle x horizon tensor: {tensor_bytes / 1e9:.3f} GB")


def risk_outs(S_):
    return dict(exit=torch.empty((B, P), dtype=torch.int32, device="cuda"), jx=torch.empty((B, P), dtype=torch.float32, device="cuda"),
                first_exit=torch.empty((B, H + 2), dtype=torch.int32, device="cuda"), outside_any=torch.empty((B, H + 1), dtype=torch.int32, device="cuda"),
                jstat=torch.empty((B, 4), dtype=torch.float32, device="cuda"), jq=torch.empty((B, 4), dtype=torch.float32, device="cuda"),
                jtail=torch.empty(B, dtype=torch.float32, device="cuda"))


def risk_call(S_, outs):
    kw = dict(xref=xref.data_ptr(), lo=rlo.data_ptr(), hi=rhi.data_ptr(), centre=rows.data_ptr(), tail=0.1, quantiles=(0.0, 0.5, 0.9, 1.0), stream=st)
    kw.update({k: v.data_ptr() for k, v in outs.items()})
    return lambda: S_.risk_dev(B, **kw)


OUT_ALL, OUT_NOQ, OUT_CURVE, BANDS3, CANON, TUBE, RISK, NOISE = ("outcome_dev, all eight outputs, 2 quantiles", "outcome_dev, the six without a selection",
                                                                  "outcome_dev, first_fail + fail_step", "bands_dev, 3 quantiles + below + at", "traj_to_canonical_dev",
                                                                  "tube_dev, five planes", "risk_dev, all outputs, centre rows", "noise_from_keys_dev")
SCORE = Score(pos_radius=0.5, tilt_max=np.radians(45.0), rate_max=3.0)


def outcome_call(names, quantiles=None):
    kw = {k: o_bufs[k].data_ptr() for k in names}
    return lambda: S.outcome_dev(B, score=SCORE, xref=xref.data_ptr(), quantiles=quantiles, stream=st, **kw)


NOQ = ("words", "fail_step", "first_fail", "cause_ever", "chan_stat", "agg_stat")
r_new = risk_outs(S)
steps = {
    "rollout_dev(store_traj=1)": lambda: S.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise.data_ptr(), cost.data_ptr(), None, True, st),
    OUT_ALL: outcome_call(tuple(o_bufs), (0.5, 0.95)),
    OUT_NOQ: outcome_call(NOQ),
    OUT_CURVE: outcome_call(("first_fail", "fail_step")),
    BANDS3: lambda: S.bands_dev(B, quantiles=Q3, observed=rows.data_ptr(), q=q.data_ptr(), below=below.data_ptr(), at=at.data_ptr(), stream=st),
    CANON: lambda: S.traj_to_canonical_dev(B, canon.data_ptr(), st),
    TUBE: lambda: S.tube_dev(B, *[p.data_ptr() for p in planes], lo=lo, hi=hi, stream=st),
    RISK: risk_call(S, r_new),
    NOISE: lambda: S.noise_from_keys_dev(keys, noise.data_ptr(), st),
}
PAR = " (parent library)"
if a.parent_lib:
    Sp = make(B, a.parent_lib)
    assert not hasattr(Sp.lib, "sdempc_outcome_batch"), "--parent-lib names a library that already has the outcome entry points"
    noise_p = torch.empty_like(noise)
    planes_p = [torch.empty_like(p) for p in planes]
    r_par = risk_outs(Sp)
    q_p, below_p, at_p = torch.empty_like(q), torch.empty_like(below), torch.empty_like(at)
    Sp.noise_from_keys_dev(keys, noise_p.data_ptr(), st)
    Sp.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise_p.data_ptr(), cost.data_ptr(), None, True, st)     # (the parent handle's own tensor)
    torch.cuda.synchronize()
    steps[TUBE + PAR] = lambda: Sp.tube_dev(B, *[p.data_ptr() for p in planes_p], lo=lo, hi=hi, stream=st)
    steps[RISK + PAR] = risk_call(Sp, r_par)
    steps[BANDS3 + PAR] = lambda: Sp.bands_dev(B, quantiles=Q3, observed=rows.data_ptr(), q=q_p.data_ptr(), below=below_p.data_ptr(), at=at_p.data_ptr(), stream=st)
    steps[NOISE + PAR] = lambda: Sp.noise_from_keys_dev(keys, noise_p.data_ptr(), st)

for fn in steps.values():        # warm-up of every step
    step(fn)
times = {k: [] for k in steps}
order = list(steps)
swapped = list(order)
if a.parent_lib:                 # every other repetition the two libraries trade places, so that neither always runs behind the other
    for k in (TUBE, RISK, BANDS3, NOISE):
        i, j = swapped.index(k), swapped.index(k + PAR)
        swapped[i], swapped[j] = swapped[j], swapped[i]
for r in range(a.reps):          # interleaved
    for k in (swapped if r % 2 else order):
        times[k].append(step(steps[k]))
if a.parent_lib:
    assert torch.equal(noise, noise_p), "the two libraries drew different noise"
    assert all(torch.equal(p, w) for p, w in zip(planes, planes_p)), "the two libraries' tube planes differ"
    assert all(torch.equal(r_new[k].view(torch.int32), r_par[k].view(torch.int32)) for k in r_new), "the two libraries' risk outputs differ"
    n3 = B * 3 * C                   # (three planes per instance: the first n3 words of the eight-plane buffers)
    assert torch.equal(q.view(torch.int32).flatten()[:n3], q_p.view(torch.int32).flatten()[:n3]) and torch.equal(below, below_p) and torch.equal(at, at_p), \
        "the two libraries' bands outputs differ"

say(f"{a.reps} interleaved repetitions after one warm-up; ms per call (host clock around launch + synchronise):")
med = {}
for k, t in times.items():
    med[k] = float(np.median(t))
    say(f"  {k:44s} median {med[k]:9.3f}   min {min(t):9.3f}   max {max(t):9.3f}   max/min {max(t) / min(t):6.3f}   all {' '.join(f'{x:.3f}' for x in t)}")
out_bytes = {k: v.numel() * 4 for k, v in o_bufs.items()}
say(f"(a) effective rate, outcome_dev all outputs (tensor once + {sum(out_bytes.values()) / 1e6:.1f} MB out; the rows phase reads the tensor's lines again, from "
    f"the cache or not): {(tensor_bytes + sum(out_bytes.values())) / (med[OUT_ALL] * 1e-3) / 1e12:6.3f} TB/s")
say(f"(a) effective rate, outcome_dev first_fail + fail_step (tensor once): {tensor_bytes / (med[OUT_CURVE] * 1e-3) / 1e12:6.3f} TB/s")
say(f"(a) effective rate, traj_to_canonical_dev (tensor read + written): {2 * tensor_bytes / (med[CANON] * 1e-3) / 1e12:6.3f} TB/s")
say(f"(a) outcome_dev / traj_to_canonical_dev time: all outputs {med[OUT_ALL] / med[CANON]:.3f};  without a selection {med[OUT_NOQ] / med[CANON]:.3f};  "
    f"first_fail + fail_step {med[OUT_CURVE] / med[CANON]:.3f}")
if a.parent_lib:
    for k in (NOISE, TUBE, RISK, BANDS3):
        tp, tn = times[k + PAR], med[k]
        verdict = "inside" if min(tp) <= tn <= max(tp) else "BELOW it (the new library is faster than the parent's fastest call)" if tn < min(tp) else "ABOVE it (slower)"
        say(f"(b) {k}: new median {tn:.3f} ms; parent median {float(np.median(tp)):.3f} ms, parent's own spread [{min(tp):.3f}, {max(tp):.3f}] ms -> {verdict}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
S.close()
if a.parent_lib:
    Sp.close()
