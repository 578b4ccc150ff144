"""Rate of the predicted-risk reducer (SPEC.md §12a) against the only route that existed before it, and of the two older modes of its hosting kernel against the
parent commit's library.

Configuration C2 (H = 50, P = 128) in the arithmetic bench.py reports (f32x3 / fast) at B = 12,288 — or, where the device's memory does not allow that, the largest
halving of it that does; the B used is printed. One process; after one warm-up of every step, --reps (5) repetitions in which the steps are INTERLEAVED, each step
timed by a host clock around work that ends in a device synchronise and guarded by its own watchdog thread (--step-timeout seconds: the process then exits with 124 and
starts nothing more; a process that cannot even exit is the business of the `timeout -k` the tool is run under). Per step: the median and the max-to-min spread.

  1. rollout_dev(store_traj=1): the rollout that leaves the particle x horizon tensor in the handle.
  2. risk_dev with all seven outputs (box around the particle mean, centre_mode 3, so the tube's mean launch is part of it; four quantiles, a 10 % tail): reads the
     tensor once (plus once for the mean) and writes 2 P + 2 H + 16 words per instance.
  3. traj_to_canonical_dev of the same tensor — THE YARDSTICK: it reads the tensor once and writes it once, and it is the device half of the route via
     rollout(want_traj=True) (the copy to the host and the NumPy reduction come on top of it and are not timed here).
  4. tube_dev with five planes, and noise_from_keys_dev at the same B (the two older modes of the kernel that hosts the reducer); with --parent-lib PATH the same
     two calls on a second handle bound to a library built from the parent commit, in the same repetitions (the two libraries trade places every other
     repetition): the new medians have to lie inside the parent's own run-to-run spread.
  Also timed: risk_dev with caller's centre rows (centre_mode 1: the reducer's launch alone) and risk_dev without the rank outputs.

usage: python tools/risk_rate.py [--batch 12288] [--reps 5] [--step-timeout 60] [--parent-lib PATH] [--out FILE]"""
import argparse
import os
import threading
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=12288)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=60)
ap.add_argument("--parent-lib", default=None, help="libsdempc.so of the parent commit: times its noise_from_keys_dev and tube_dev beside the new ones")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()

import torch

from sde4mbrl_px4_amd import _abi, load_mpc_config, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdempcError, SdeMpcSolver

if not torch.cuda.is_available():
    sys.exit("tools/risk_rate.py: no GPU: nothing is measured without one")

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def _expired():
    print(f"tools/risk_rate.py: a step ran past its {a.step_timeout} s: stopping here", flush=True)
    os._exit(124)


def step(fn):
    """one step under its own watchdog — a timer THREAD, which fires while the main thread sits in a blocking HIP call or synchronise (those release the
    interpreter lock) and ends the process: host clock around the call and the synchronise that ends it, in milliseconds"""
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
    """a handle of max_batch B, bound to the library at lib_path (default: this tree's)"""
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
        canon = torch.empty((B, P, H + 1, 13), dtype=torch.float32, device="cuda")
        planes = [torch.empty((B, H + 1, 13), dtype=torch.float32 if k < 4 else torch.int32, device="cuda") for k in range(5)]
        torch.cuda.synchronize()
        S.noise_from_keys_dev(keys, noise.data_ptr(), st)
        S.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise.data_ptr(), cost.data_ptr(), None, True, st)      # (allocates the workspaces)
        torch.cuda.synchronize()
        break
    except (SdempcError, RuntimeError) as e:
        if B <= 256 or "memory" not in str(e).lower():
            raise
        say(f"B = {B}: {str(e).splitlines()[0]} -> halving")
        S = noise = x0 = xref = u = cost = canon = planes = None
        torch.cuda.empty_cache()
        B //= 2

lo = np.array([-2, -2, -2, -3, -3, -3, -np.inf, -np.inf, -np.inf, -np.inf, -4, -4, -4], np.float32)
hi = -lo
QUANTILES = (0.0, 0.5, 0.9, 1.0)
box = np.array([0.05, 0.05, 0.05, 0.3, 0.3, 0.3, np.inf, np.inf, np.inf, np.inf, 1.0, 1.0, 1.0], np.float32)       # around the centre rows
rlo = torch.from_numpy(np.tile(-box, (B, 1))).cuda()
rhi = torch.from_numpy(np.tile(box, (B, 1))).cuda()
rows = torch.empty((B, H + 1, 13), dtype=torch.float32, device="cuda")           # centre rows of the centre_mode 1 step: the rollout's own mean
r_exit = torch.empty((B, P), dtype=torch.int32, device="cuda")
r_jx = torch.empty((B, P), dtype=torch.float32, device="cuda")
r_first = torch.empty((B, H + 2), dtype=torch.int32, device="cuda")
r_any = torch.empty((B, H + 1), dtype=torch.int32, device="cuda")
r_jstat = torch.empty((B, 4), dtype=torch.float32, device="cuda")
r_jq = torch.empty((B, len(QUANTILES)), dtype=torch.float32, device="cuda")
r_jtail = torch.empty(B, dtype=torch.float32, device="cuda")
S.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise.data_ptr(), cost.data_ptr(), rows.data_ptr(), True, st)
torch.cuda.synchronize()
tensor_bytes = 4 * S.lib.sdempc_traj_dev_floats(S._h, B)
plane_bytes = 5 * 4 * B * C
risk_bytes = 4 * B * (2 * P + 2 * H + 3 + 4 + len(QUANTILES) + 1)
say(f"device: {torch.cuda.get_device_name(0)}; C2 (H = {H}, P = {P}), mlp_dtype f32x3, math_mode fast, B = {B}" + ("" if B == a.batch else f" (asked for {a.batch})"))
say(f"particle x horizon tensor: {tensor_bytes / 1e9:.3f} GB; risk outputs: {risk_bytes / 1e6:.1f} MB; five tube planes: {plane_bytes / 1e6:.1f} MB")


def risk_call(centre, ranks=True):
    kw = dict(xref=xref.data_ptr(), lo=rlo.data_ptr(), hi=rhi.data_ptr(), centre=centre, exit=r_exit.data_ptr(), jx=r_jx.data_ptr(), first_exit=r_first.data_ptr(),
              outside_any=r_any.data_ptr(), jstat=r_jstat.data_ptr(), stream=st)
    if ranks:
        kw.update(tail=0.1, quantiles=QUANTILES, jq=r_jq.data_ptr(), jtail=r_jtail.data_ptr())
    return lambda: S.risk_dev(B, **kw)


RISK, RISK1, RISK_NR, CANON, TUBE, NOISE = ("risk_dev, all outputs, centre = mean", "risk_dev, all outputs, centre rows", "risk_dev, no rank outputs, centre rows",
                                            "traj_to_canonical_dev", "tube_dev, five planes", "noise_from_keys_dev")
steps = {
    "rollout_dev(store_traj=1)": lambda: S.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise.data_ptr(), cost.data_ptr(), None, True, st),
    RISK: risk_call("mean"),
    RISK1: risk_call(rows.data_ptr()),
    RISK_NR: risk_call(rows.data_ptr(), ranks=False),
    CANON: lambda: S.traj_to_canonical_dev(B, canon.data_ptr(), st),
    TUBE: lambda: S.tube_dev(B, *[p.data_ptr() for p in planes], lo=lo, hi=hi, stream=st),
    NOISE: lambda: S.noise_from_keys_dev(keys, noise.data_ptr(), st),
}
PAR = " (parent library)"
if a.parent_lib:
    Sp = make(B, a.parent_lib)
    assert not hasattr(Sp.lib, "sdempc_risk_batch"), "--parent-lib names a library that already has the risk entry points"
    noise_p = torch.empty_like(noise)
    planes_p = [torch.empty_like(p) for p in planes]
    Sp.noise_from_keys_dev(keys, noise_p.data_ptr(), st)
    Sp.rollout_dev(B, x0.data_ptr(), u.data_ptr(), xref.data_ptr(), noise_p.data_ptr(), cost.data_ptr(), None, True, st)     # (the parent handle's own tensor)
    torch.cuda.synchronize()
    steps[TUBE + PAR] = lambda: Sp.tube_dev(B, *[p.data_ptr() for p in planes_p], lo=lo, hi=hi, stream=st)
    steps[NOISE + PAR] = lambda: Sp.noise_from_keys_dev(keys, noise_p.data_ptr(), st)

for fn in steps.values():        # warm-up of every step
    step(fn)
times = {k: [] for k in steps}
order = list(steps)
swapped = list(order)
if a.parent_lib:                 # every other repetition the two libraries trade places, so that neither always runs behind the other
    for k in (TUBE, NOISE):
        i, j = swapped.index(k), swapped.index(k + PAR)
        swapped[i], swapped[j] = swapped[j], swapped[i]
for r in range(a.reps):          # interleaved
    for k in (swapped if r % 2 else order):
        times[k].append(step(steps[k]))
if a.parent_lib:
    assert torch.equal(noise, noise_p), "the two libraries drew different noise"
    assert all(torch.equal(p, q) for p, q in zip(planes, planes_p)), "the two libraries' tube planes differ"
pe = 1.0 - r_first[:, -1].float().cpu().numpy() / P
say(f"sanity: p_ever over the batch min {pe.min():.3f} median {float(np.median(pe)):.3f} max {pe.max():.3f}; first_exit sums to P: {bool((r_first.sum(dim=1) == P).all())}")

say(f"{a.reps} interleaved repetitions after one warm-up; ms per call (host clock around launch + synchronise):")
med = {}
for k, t in times.items():
    med[k] = float(np.median(t))
    say(f"  {k:42s} median {med[k]:9.3f}   min {min(t):9.3f}   max {max(t):9.3f}   max/min {max(t) / min(t):6.3f}   all {' '.join(f'{x:.3f}' for x in t)}")
say(f"effective rate, risk_dev centre rows (tensor once + outputs): {(tensor_bytes + risk_bytes) / (med[RISK1] * 1e-3) / 1e9:8.1f} GB/s")
say(f"effective rate, risk_dev centre = mean (tensor twice + outputs): {(2 * tensor_bytes + risk_bytes) / (med[RISK] * 1e-3) / 1e9:8.1f} GB/s")
say(f"effective rate, traj_to_canonical_dev (tensor read + written): {2 * tensor_bytes / (med[CANON] * 1e-3) / 1e9:8.1f} GB/s")
for k in (RISK, RISK1, RISK_NR):
    ratio = med[k] / med[CANON]
    say(f"{k} / traj_to_canonical_dev time: {ratio:.3f}" + ("" if ratio < 1 else "   NOT below 1: the reducer is no faster than the relayout it replaces"))
if a.parent_lib:
    for k in (TUBE, NOISE):
        tp, tn = times[k + PAR], med[k]
        verdict = "inside" if min(tp) <= tn <= max(tp) else "BELOW it (the new library is faster than the parent's fastest call)" if tn < min(tp) else "ABOVE it (slower)"
        say(f"{k} A/B: new median {tn:.3f} ms; parent median {float(np.median(tp)):.3f} ms, parent's own spread [{min(tp):.3f}, {max(tp):.3f}] ms -> {verdict}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
S.close()
if a.parent_lib:
    Sp.close()
