"""Mixed batches through multi-round persistent duo launches, EVERY position against the oracle bit for bit.

The pools of tests/mixed_batch_cases.py (tests/test_mixed_batch_cpu.py proves what they hold) put guarded, one-iteration and full-length solves of
distinct instances on one team one after another: whatever a solve leaves behind in the LDS carve, the workspace slot, the staging rows, the
reduction scratch or a spilled optimiser scalar must not reach the next one. Batch sizes follow from the device's compute units (two rounds and
a bit: striped; three and a bit: ticketed); every launch is checked by kernel name, work counters and layout fallbacks."""
import functools

import numpy as np
import pytest

import kernel_census as kc
import mixed_batch_cases as mb
from cases import bits_differ
from sde4mbrl_px4_amd.solver import SdeMpcSolver

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_cus():
    cfg, model, x0, xref, noise, u, s0, _ = mb.batch("guard", mb.P2, 1)
    S = SdeMpcSolver(cfg, model, max_batch=1)
    S.solve(x0, xref, noise, u, s0)
    cus = S.get_option("device_cus")
    S.close()
    assert cus >= 16
    return cus


@functools.lru_cache(maxsize=None)
def _expected(L, B):
    """The oracle's (uopt, xevol, info) of the pool, gathered over the positions of the batch; the endings per pool instance."""
    ref = mb.reference(L.pool, L.P, L.m, L.math, L.mlp)
    idx = mb.order(B, mb.POOLS[L.pool].K)
    want = tuple(np.stack([r[j] for r in ref])[idx] for j in range(3))
    return ref, idx, want, [mb.ending(r) for r in ref]


def _compare(L, got, B, slots, what):
    ref, idx, want, ends = _expected(L, B)
    if sum(bits_differ(g, w) for g, w in zip(got, want)) == 0:
        return
    bad = [b for b in range(B) if any(bits_differ(g[b], w[b]) for g, w in zip(got, want))]
    before = lambda b: ends[idx[b - slots]] if b >= slots else "-"
    lines = [f"b = {b}: pool instance {idx[b]} ({ends[idx[b]]}) after {before(b)}; words (uopt, xevol, info) "
             f"{tuple(bits_differ(g[b], w[b]) for g, w in zip(got, want))}" for b in bad[:16]]
    pattern = sorted({(before(b), ends[idx[b]]) for b in bad})
    pytest.fail(f"{L.id} {what}: {len(bad)} of {B} positions differ from the oracle ({slots} team slots); (ending before, ending) of the failing "
                f"positions: {pattern}\n" + "\n".join(lines))


def _solver(L, B, **more):
    cfg, model, x0, xref, noise, u, s0, idx = mb.batch(L.pool, L.P, B, L.m)
    cfg = cfg.replace(math_mode=L.math, mlp_dtype=L.mlp)
    return SdeMpcSolver(cfg, model, max_batch=B, options={**dict(L.options), **more}), (x0, xref, noise, u, s0)


def _launch(L, S, inputs, B, slots, kernel, what=""):
    """One launch of the handle: kernel name, every position, work counters, layout fallbacks. -> the outputs."""
    ref, idx, _, ends = _expected(L, B)
    S.work_counters(reset=True)
    got = S.solve(*inputs)
    name, wc = S.last_kernel_name(), S.work_counters_full()
    S.solve_status()
    print(f"{L.id} {what}: {kc.normalise(name)} B = {B}, {slots} team slots, work counters {wc}")
    assert kc.normalise(name) == (kernel, L.math), name
    _compare(L, got, B, slots, what)
    assert wc[:3] == mb.expected_work(ref, idx), (wc, mb.expected_work(ref, idx))
    if (L.math, L.mlp) == ("exact", "f32"):
        assert wc[3] == int(np.asarray(mb.settled_trials(L.pool, L.P, L.m))[idx].sum()), wc
    assert S.layout_fallbacks() == 0
    return got


def _arranged(L, cus):
    """Before the launch: the batch has the rounds it is meant to have on this device, and a striped one puts every abnormal ending in front of and
    behind a full-length solve on some team."""
    slots, B = L.slots(cus), L.B(cus)
    assert mb.ticketed(B, slots) == (L.how == "ticketed") and B >= 6 * cus
    if L.how == "striped":
        _, idx, _, ends = _expected(L, B)
        need = mb.required_successions(ends)
        assert len(need) >= 4 and need <= mb.successions(idx, ends, slots), sorted(need - mb.successions(idx, ends, slots))
    return slots, B


SINGLE = [L for L in mb.LAUNCHES if L.team != "TeamPairT<6>"]


@pytest.mark.parametrize("L", SINGLE, ids=lambda L: L.id)
def test_every_position_of_a_mixed_batch(L):
    slots, B = _arranged(L, device_cus())
    S, inputs = _solver(L, B)
    _launch(L, S, inputs, B, slots, L.kernel())
    S.close()


@pytest.mark.parametrize("L", [L for L in mb.LAUNCHES if L.team == "TeamPairT<6>"], ids=lambda L: L.id)
def test_six_team_workgroups_against_the_oracle_and_against_two_team_workgroups(L):
    """The same batch in six-team workgroups (a launch that fills the device) and, on the same handle, in two-team workgroups: whole outputs
    identical; a ticketed launch repeated on the handle (the ticket word is never reset) as well."""
    slots, B = _arranged(L, device_cus())
    pair = mb.kernel_name("TeamPairT<2>", L.m, L.mlp)
    assert slots == mb.team_slots(pair, L.H(), L.m, device_cus())
    S, inputs = _solver(L, B)
    hexa = _launch(L, S, inputs, B, slots, L.kernel(), "hex=1")
    if L.how == "ticketed":
        again = _launch(L, S, inputs, B, slots, L.kernel(), "hex=1, second ticketed launch")
        assert all(bits_differ(a, b) == 0 for a, b in zip(hexa, again))
    S.set_option("hex", 0)
    two = _launch(L, S, inputs, B, slots, pair, "hex=0")
    assert all(bits_differ(a, b) == 0 for a, b in zip(hexa, two))
    S.close()


def test_poisoned_workspaces_change_nothing():
    """Every workspace of the handle filled with 0xFF bytes before the first device call: no solve of the batch reads what it has not written."""
    L = next(L for L in mb.LAUNCHES if L.pool == "guard" and L.team == "TeamPairT<2>" and L.how == "striped")
    slots, B = _arranged(L, device_cus())
    S, inputs = _solver(L, B, test_ws_fill=255)
    assert S.get_option("test_ws_fill") == 255 and not S.device_ready()
    _launch(L, S, inputs, B, slots, L.kernel(), "test_ws_fill=255")
    S.close()
