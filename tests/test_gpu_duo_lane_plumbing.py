"""The duo layout's lane plumbing against the oracle, bit for bit: the paired layer-1 operands (three v_permlane32_swap form the B operands of
both MLP passes, sdempc_duo.inc.h duo_pair_inputs) and the paired particle sums of the adjoint's per-step outputs (two values per register
through v_permlane16_swap, group_bfly32_pairs / group_pair_store). Particle counts at which either can go wrong:
  P = 33   group B holds one valid particle
  P = 64   a full pair
  P = 70   three groups: the second pair has no group B, its upper lane half shadows group A and must neither store nor add
  P = 97   two waves per team, the last group one particle
  P = 130  five groups, four-wave team
with m = 4 and m = 6 (8 and 10 adjoint outputs per step: four and five register pairs), H in {3, 8} with both step lengths of the time grid,
every mlp_dtype and math_mode: the full cross product, 120 cases. B = 3 and max_iter = 3 keep a case well under a second.
solve() runs the duo kernels (forward sweeps, adjoint sweep, per-step sums: uopt, xevol and the eight telemetry words depend on all of them);
grad() is the library's stand-alone gradient kernel, which keeps one group per wave: it is compared as well, as the same problem's second witness."""
import functools
import re

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
MODE = {"f32": 0, "f16": 1, "f32x3": 2}
PS = (33, 64, 70, 97, 130)
OPTIONS = dict(coop=0, pk=0, duo=1)


def _cases():
    return [(mlp, math, P, m, H) for mlp in ("f32x3", "f32", "f16") for math in ("fast", "exact") for P in PS for m in (4, 6) for H in (3, 8)]


@functools.lru_cache(maxsize=None)
def _problem(P, m, H):
    """Inputs of one geometry, shared by the arithmetics that run it (never modified)."""
    rng = np.random.default_rng(700 + P + m)
    x0 = W.random_initial_states(B, 17 + m)
    cfg = _cfg("f32", "exact", P, m, H)
    xref = np.stack([W.reference_window(0.13 * b, cfg.time_steps) for b in range(B)])
    noise = W.make_noise(B, P, H, 29 + P)
    u = np.clip(np.asarray(cfg.uref, np.float32) + 0.1 * rng.standard_normal((B, H, m)), 1e-4, 1).astype(np.float32)
    for a in (x0, xref, noise, u):
        a.setflags(write=False)
    return x0, xref, noise, u


def _cfg(mlp, math, P, m, H):
    kw = dict(horizon=H, num_short_dt=H // 2, long_step_dt=0.1, num_particles=P, u_slew_coeff=1.0, max_iter=3, max_no_improvement_iter=3,
              mlp_dtype=mlp, math_mode=math)           # num_short_dt < H: short and long steps both occur
    if m == 6:
        kw.update(input_id=list(range(6)), input_bound=[[1e-4, 1.0]] * 6, uref=[0.42] * 6)
    return MPCConfig(**kw)


@pytest.mark.parametrize("mlp,math,P,m,H", _cases())
def test_duo_solve_and_grad_match_oracle_bit_for_bit(mlp, math, P, m, H):
    cfg = _cfg(mlp, math, P, m, H)
    model = synthetic_iris() if m == 4 else synthetic_hexa()
    x0, xref, noise, u = _problem(P, m, H)
    s0 = np.full(B, 0.01, np.float32)
    S = SdeMpcSolver(cfg, model, max_batch=B, options=OPTIONS)
    gc, grad = S.grad(x0, u, xref, noise)
    uopt, xevol, info = S.solve(x0, xref, noise, u, s0)
    kname = S.last_kernel_name()
    S.close()
    # MODE 3 of sdempc_solve_kernel: the duo layout with noise staging rows, the instantiations that carry the paired forms (MODE 4, without
    # staging rows — horizons far longer than these — keeps the broadcast form and the one-value-per-register sums)
    name, mode = kc.normalise(kname)
    assert mode == math and re.fullmatch(rf"sdempc_solve_kernel<Team\w+(<\d>)?, {m}, {MODE[mlp]}, false, 3, (true|false)>", name), kname
    O = orc.Oracle(cfg, model)
    for b in range(B):
        c2, g2 = O.grad(x0[b], u[b], xref[b], noise[b])
        assert gc[b] == np.float32(c2) and bits_differ(grad[b], g2.astype(np.float32)) == 0, ("grad", b)
        uo, xe, io, _ = O.solve(x0[b], xref[b], noise[b], u[b], 0.01)
        assert bits_differ(uopt[b], uo) == 0 and bits_differ(xevol[b], xe) == 0 and bits_differ(info[b], io) == 0, ("solve", b)
        assert io[2] >= 1, io                        # an iteration ran: the adjoint sweep's sums reached the result
