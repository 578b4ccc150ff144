"""The five closed-loop entry points at the settings where SPEC.md §11a .. §11d say one of them IS the one below it: sdempc_closed_loop_batch_plant with
the handle's own model and one substep is sdempc_closed_loop_batch; _scenario with no disturbance and a one-row plant schedule is _timed; _rate with no
scenario and motor_weight = 1 is _timed on the seven values they share. (_timed at S = 1, D = 0, alpha = 0 is _plant:
tests/test_gpu_timed_loop.py::test_period_one_no_delay_no_lag_is_the_existing_loop.) The two sides of each equality run different kernel instantiations
built from the same pieces (sdempc_loop.inc.h), so every common output must agree in every bit.

Shapes of tests/scenario_cases.py, the smallest at which these kernels can go wrong: H = 4, B = 5 (a partly empty last workgroup), T = 7 with S = 3 (a
partial last period), P in {1, 33}, n in {1, 3}, one shared plant and per-episode plants with a plant_of that repeats an index."""

import numpy as np
import pytest

from loop_cases import NAMES, same
from rate_loop_cases import rate_loop
from scenario_cases import ALPHA, B5, S3, T7, episodes, motor_state, perturbed_plants, small_cfg
from sde4mbrl_px4_amd import synthetic_iris
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu

PLANT_OF = np.array([0, 1, 2, 1, 0], np.int32)


class CalledEntry:
    """A solver's library handle that notes which closed-loop entry point was CALLED last (looking one up, as the prototype helpers do, does not count)."""

    def __init__(self, lib):
        self._lib, self.last = lib, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("sdempc_closed_loop_batch"):
            return fn
        note = self

        class Entry:
            def __call__(self, *args):
                note.last = name
                return fn(*args)

            def __getattr__(self, key):
                return getattr(fn, key)

            def __setattr__(self, key, value):
                setattr(fn, key, value)

        return Entry()


@pytest.mark.parametrize("mlp_dtype,math_mode", [("f32", "exact"), ("f32x3", "fast")])
@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("P,n", [(1, 1), (33, 3)])
def test_each_entry_at_its_degenerate_setting_is_the_entry_below(P, n, per_episode, mlp_dtype, math_mode):
    cfg = small_cfg(num_particles=P, mlp_dtype=mlp_dtype, math_mode=math_mode)
    model = synthetic_iris()
    x0, xref, keys = episodes(cfg, B5, 70)
    pl = perturbed_plants(model, 3)
    ua = motor_state(B5, 4)
    S = SdeMpcSolver(cfg, model, max_batch=B5)
    S.lib = CalledEntry(S.lib)

    def loop(entry, **kw):
        out = S.closed_loop(x0, xref, keys, T7, **kw)
        assert S.lib.last == "sdempc_closed_loop_batch" + entry, (entry, S.lib.last)
        return out

    # _plant with the handle's own model, one substep == the plain entry
    own = dict(plant=[model] * 3, plant_of=PLANT_OF) if per_episode else dict(plant=model)
    same(loop("_plant", **own), loop(""), names=NAMES[:6])
    vehicle = dict(plant=pl, plant_of=PLANT_OF, plant_substeps=n) if per_episode else dict(plant=pl[1], plant_substeps=n)
    # _scenario with no disturbance and a one-row schedule == _timed
    timing = dict(solve_period=S3, solve_delay=n + 1, motor_lag=ALPHA, u_act_in=ua)
    timed = loop("_timed", **vehicle, **timing)
    one_row = dict(plant=pl, plant_of=PLANT_OF[None]) if per_episode else dict(plant=[pl[1]], plant_of=np.zeros((1, B5), np.int32))
    same(loop("_scenario", **{**vehicle, **one_row}, **timing), timed, names=NAMES[:7])
    # _rate with sc == NULL and motor_weight = 1 == _timed on the seven shared outputs
    rated = loop("_rate", rate_loop=rate_loop("stiff", motor_weight=1.0), **vehicle, **timing)
    assert len(rated) == 10
    same(rated[:7], timed, names=NAMES[:7])
    assert np.isfinite(timed[0]).all() and timed[0][:, 0].tobytes() == x0.tobytes()
    S.solve_status()
    S.close()
