"""Line-search trials settled without a rollout (SPEC.md §8, implementation note; sdempc_work_counters out[3]).

With every cost weight of a handle >= 0 no cost is negative, so a trial whose Armijo bound thr = fma(ls_coef, g.d1, c_y) is negative is rejected
whatever its rollout would return; solve_instance (sdempc_kernels.hip) forms the bound first and rolls such a trial out only when it is the last of
its line search. Results must not change: uopt, xevol and the eight telemetry words are the oracle's bit for bit (the oracle evaluates every trial).

The case. C2's constants at short horizons never have thr < 0 with the YAML's step size and coefficient. With ls_coef = 0.5, stepsize_in = 1.0,
max_iter = 14, H = 12 and the first two instances of the bench batch (W.random_initial_states(2, 0), reference_window(0.05 b), keys
split(PRNGKey(10), 2)) instance 1 has, on the CPU oracle (tests/tools/armijo_census.py --horizon 12 --particles P --ls-coef 0.5 --stepsize-in 1.0
--max-iter 14 --instances 2 [--mlp-dtype f32x3 --math-mode fast]), in f32 / exact and in f32x3 / fast alike:
    P = 40: 10 trials with thr < 0, 8 of them not the last of their line search;  P = 1: 13 and 11;  instance 0: none at either P.
The duo kernels without noise staging rows (MODE 4) are dispatched from H = 51 on (m = 4; kernel_census: the dispatcher's own LDS arithmetic). At
H = 51, P = 40, max_iter = 8 C2's own step size and coefficient reach the case (as they do at the bench shape): 20 + 19 non-final trials with
thr < 0 on instances 0 and 1, in both arithmetics (same tool, --horizon 51 --particles 40 --max-iter 8).
out[3] must equal these counts: a trial is settled iff it is non-final and thr < 0, and thr has the oracle's bits."""
import functools
import os

import numpy as np
import pytest

import kernel_census as kc
import orc
from cases import CDIR, bits_differ
from sde4mbrl_px4_amd import load_mpc_config, prng, synthetic_iris
from sde4mbrl_px4_amd import workload as W
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu

B = 2
ARITH = [("f32x3", "fast"), ("f32", "exact")]


@functools.lru_cache(maxsize=None)
def _h_mode4():
    return kc.shortest_h(lambda H: not kc.pair_fits(H, 4) and kc.duo_pick(H, 4, 2) == 2)


# layout -> (P, H, handle options as tests/test_gpu_parity.py sets them, MODE template argument of the kernel that must run (None: not asserted),
#            settled trials of instances (0, 1) from tests/tools/armijo_census.py)
def _layouts():
    return {"tile": (40, 12, dict(lane=0, coop=0, duo=0), 0, (0, 8)),
            "single_particle": (1, 12, dict(coop=0), None, (0, 11)),      # (f32: the lane layout, MODE 1; f32x3: a one-wave tile team, MODE 0)
            "duo_staging_rows": (40, 12, dict(coop=0, pk=0, duo=1), 3, (0, 8)),
            "duo_no_staging_rows": (40, _h_mode4(), dict(coop=0, pk=0, duo=1), 4, (20, 19))}


def _cfg(mlp, math, P, H, **kw):
    cfg = load_mpc_config(os.path.join(CDIR, "c2_iris_traj_h50_p128.yaml")).replace(horizon=H, num_particles=P, mlp_dtype=mlp, math_mode=math)
    if H == 12:
        return cfg.replace(ls_coef=0.5, max_iter=14, **kw), 1.0
    return cfg.replace(max_iter=8, **kw), cfg.ls_init_stepsize


@functools.lru_cache(maxsize=None)
def _problem(P, H):
    """The first two instances of the bench batch at this shape (never modified)."""
    cfg, _ = _cfg("f32", "exact", P, H)
    x0 = W.random_initial_states(B, 0)
    xref = np.stack([W.reference_window(0.05 * b, cfg.time_steps) for b in range(B)])
    keys = prng.split(prng.PRNGKey(10), B)
    noise = np.stack([orc.noise_from_key(keys[b], P, H) for b in range(B)])
    u0 = np.tile(np.asarray(cfg.uref, np.float32), (B, H, 1))
    for a in (x0, xref, noise, u0):
        a.setflags(write=False)
    return x0, xref, noise, u0


@functools.lru_cache(maxsize=None)
def _oracle(mlp, math, P, H, variant):
    """The oracle's (uopt, xevol, info) of both instances, shared by the layouts that run this shape."""
    cfg, step = _cfg(mlp, math, P, H, **dict(variant))
    x0, xref, noise, u0 = _problem(P, H)
    O = orc.Oracle(cfg, synthetic_iris())
    return [O.solve(x0[b], xref[b], noise[b], u0[b], step)[:3] for b in range(B)]


def _run(layout, mlp, math, idx=(0, 1), **variant):
    """Solve instances idx of the pair on the GPU in this layout; -> (work counters[4], info) after the bit-for-bit comparison with the oracle."""
    P, H, opts, mode, _ = _layouts()[layout]
    cfg, step = _cfg(mlp, math, P, H, **variant)
    x0, xref, noise, u0 = (a[list(idx)] for a in _problem(P, H))
    n = len(idx)
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=n, options=opts)
    uopt, xevol, info = S.solve(x0, xref, noise, u0, np.full(n, step, np.float32))
    kname, wc = S.last_kernel_name(), S.work_counters_full()
    S.close()
    name, ns = kc.normalise(kname)
    assert ns == math, kname
    if mode is not None:
        assert name.startswith("sdempc_solve_kernel<") and name.rstrip(">").split(", ")[-2] == str(mode), kname
    ref = _oracle(mlp, math, P, H, tuple(sorted(variant.items())))
    for i, b in enumerate(idx):
        uo, xe, io = ref[b]
        assert bits_differ(uopt[i], uo) == 0 and bits_differ(xevol[i], xe) == 0 and bits_differ(info[i], io) == 0, (layout, b, info[i], io)
    print(f"{layout} {mlp}/{math} {kname}: work counters {wc}, N_it {info[:, 2]}, N_ls {info[:, 7]}")
    assert wc[0] == n and wc[2] == int(info[:, 7].sum()) + 2 * n, wc          # every trial is still counted as a rollout
    return wc, info


@pytest.mark.parametrize("mlp,math", ARITH)
@pytest.mark.parametrize("layout", ["tile", "single_particle", "duo_staging_rows", "duo_no_staging_rows"])
def test_settled_trials_leave_the_results_bit_identical(layout, mlp, math):
    wc, info = _run(layout, mlp, math)
    assert 1 <= wc[3] <= int((info[:, 7] - info[:, 2]).sum()), wc              # at most every non-final trial (one trial per iteration is its search's last or accepted one)
    assert wc[3] == sum(_layouts()[layout][4]), wc                             # the CPU census: non-final trials with thr < 0


@pytest.mark.parametrize("layout", ["tile", "single_particle", "duo_staging_rows"])
def test_an_instance_without_a_negative_bound_settles_nothing(layout):
    wc, _ = _run(layout, "f32", "exact", idx=(0,))
    assert wc[3] == 0, wc


@pytest.mark.parametrize("mlp,math", ARITH)
@pytest.mark.parametrize("layout", ["tile", "single_particle", "duo_staging_rows", "duo_no_staging_rows"])
def test_one_negative_weight_switches_the_shortcut_off(layout, mlp, math):
    """A cost can then be negative: every trial is rolled out, as before."""
    wc, _ = _run(layout, mlp, math, verr=(-1e-3, 5.0, 10.0))
    assert wc[3] == 0, wc


@pytest.mark.parametrize("layout", ["tile", "single_particle", "duo_staging_rows", "duo_no_staging_rows"])
def test_the_only_trial_of_a_line_search_is_always_rolled_out(layout):
    wc, info = _run(layout, "f32x3", "fast", ls_maxls=1)
    assert wc[3] == 0 and np.array_equal(info[:, 7], info[:, 2]), wc


def test_settled_trials_accessor_and_reset():
    P, H, opts, _, counts = _layouts()["tile"]
    cfg, step = _cfg("f32", "exact", P, H)
    x0, xref, noise, u0 = _problem(P, H)
    S = SdeMpcSolver(cfg, synthetic_iris(), max_batch=B, options=opts)
    assert S.settled_trials() == 0
    S.solve(x0, xref, noise, u0, np.full(B, step, np.float32))
    assert S.settled_trials() == sum(counts) and len(S.work_counters()) == 3
    S.work_counters(reset=True)
    assert S.work_counters_full() == (0, 0, 0, 0)
    S.close()
