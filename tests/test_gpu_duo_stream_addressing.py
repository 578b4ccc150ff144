"""The duo sweeps' per-step streams against the oracle, bit for bit. duo_rollout and duo_cost_grad (sdempc_duo.inc.h) address the trajectory rows,
the noise rows, the step scalars and MODE 4's register prefetch of the next step's noise as: uniform base of the pair and step + one loop-invariant
32-bit byte offset per lane (group, column) + the row in the instruction's immediate offset. Shapes at which such an address can go wrong:
  P = 33   group B holds one valid particle
  P = 70   three groups: the second pair has no group B, its upper lane half shadows group A at lane offset 0 and must not store
  P = 130  five groups, four-wave team: a wave walks several pairs, every pair with bases of its own
with m = 4 and m = 6, H in {3, 8} with both step lengths of the time grid (MODE 3, noise through the LDS staging rows: f32x3 / fast, B = 3,
max_iter = 3), and the MODE 4 kernels (next step's noise rows prefetched into registers), which tests/test_gpu_duo_lane_plumbing.py does not
reach: the shortest horizon at which the dispatcher picks MODE 4 for a two-wave team (kernel_census: the dispatcher's own LDS arithmetic), P = 64
and P = 70, max_iter = 2, f32x3 / fast and f32 / exact. The kernel that ran is asserted by name.
solve() runs the duo kernels (uopt, xevol and the eight telemetry words depend on every stream); grad() is the library's stand-alone gradient
kernel, which keeps one group per wave: it is compared as well, as the same problem's second witness."""
import functools

import numpy as np
import pytest

import kernel_census as kc
import orc
from cases import bits_differ
from sde4mbrl_px4_amd import MPCConfig, synthetic_hexa, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu

B = 3
OPTIONS = dict(coop=0, pk=0, duo=1)


@functools.lru_cache(maxsize=None)
def _h_mode4(m):
    """launch_duo_small -> launch_duo_m<TeamBlock2>: the pair of two-wave teams no longer fits and dropping the staging rows buys a workgroup per CU"""
    return kc.shortest_h(lambda H: not kc.pair_fits(H, m) and kc.duo_pick(H, m, 2) == 2)


def _cases():
    out = [("f32x3", "fast", P, m, H, 3, 3) for P in (33, 70, 130) for m in (4, 6) for H in (3, 8)]
    out += [(mlp, math, P, m, _h_mode4(m), 4, 2) for mlp, math in (("f32x3", "fast"), ("f32", "exact")) for P in (64, 70) for m in (4, 6)]
    return out


def _cfg(mlp, math, P, m, H, max_iter):
    # num_short_dt < H: short and long steps both occur; the long horizons take shorter steps, so that they span seconds as the short ones do
    dts = dict(long_step_dt=0.1) if H <= 20 else dict(short_step_dt=0.01, long_step_dt=0.02)
    kw = dict(horizon=H, num_short_dt=H // 2, num_particles=P, u_slew_coeff=1.0, max_iter=max_iter, max_no_improvement_iter=3,
              mlp_dtype=mlp, math_mode=math, **dts)
    if m == 6:
        kw.update(input_id=list(range(6)), input_bound=[[1e-4, 1.0]] * 6, uref=[0.42] * 6)
    return MPCConfig(**kw)


@functools.lru_cache(maxsize=None)
def _problem(P, m, H):
    """Inputs of one geometry, shared by the arithmetics that run it (never modified)."""
    rng = np.random.default_rng(900 + P + m)
    x0 = W.random_initial_states(B, 19 + m)
    cfg = _cfg("f32", "exact", P, m, H, 3)
    xref = np.stack([W.reference_window(0.13 * b, cfg.time_steps) for b in range(B)])
    noise = W.make_noise(B, P, H, 31 + P)
    u = np.clip(np.asarray(cfg.uref, np.float32) + 0.1 * rng.standard_normal((B, H, m)), 1e-4, 1).astype(np.float32)
    for a in (x0, xref, noise, u):
        a.setflags(write=False)
    return x0, xref, noise, u


@pytest.mark.parametrize("mlp,math,P,m,H,mode,max_iter", _cases())
def test_duo_streams_match_oracle_bit_for_bit(mlp, math, P, m, H, mode, max_iter):
    cfg = _cfg(mlp, math, P, m, H, max_iter)
    model = synthetic_iris() if m == 4 else synthetic_hexa()
    x0, xref, noise, u = _problem(P, m, H)
    step = 0.01 if mode == 3 else 1e-4                 # (the long horizon wants a shorter first step to accept one)
    s0 = np.full(B, step, np.float32)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=OPTIONS)
    gc, grad = S.grad(x0, u, xref, noise)
    uopt, xevol, info = S.solve(x0, xref, noise, u, s0)
    kname = S.last_kernel_name()
    S.close()
    name, ns = kc.normalise(kname)
    f = kc.F16_OF[mlp]
    if mode == 4:
        assert (name, ns) == (f"sdempc_solve_kernel<TeamBlock2, {m}, {f}, false, 4, true>", math), kname
    else:
        team = "TeamBlock" if P > 128 else "TeamPairT<2>"
        assert (name, ns) == (f"sdempc_solve_kernel<{team}, {m}, {f}, false, 3, false>", math), kname
    O = orc.Oracle(cfg, model)
    for b in range(B):
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0, ("grad", b)
        uo, xe, io, _ = O.solve(x0[b], xref[b], noise[b], u[b], step)
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, ("solve", b)
        assert io[2] >= 1, io                        # an iteration ran: the adjoint sweep's sums reached the result
