"""The solve-path cases of tests/solve_paths.py on the CPU: the oracle's event record against the NumPy restatement's, the paths each case is
there for, the coverage of every named path and of every reachable cell of {source of the next gradient} x {groups per instance}, the ten
one-line-wrong optimisers, and the committed coverage matrix. No GPU."""
import os

import numpy as np
import pytest

import orc
import solve_paths as sp
from cases import bits_differ

import sys
sys.path.insert(0, os.path.join(sp.ROOT, "oracle"))
import sde_mpc_numpy as R  # noqa: E402


@pytest.mark.parametrize("name,b", [("mix_p80", 3), ("restart_p80", 4)])
def test_event_record_of_the_oracle_and_of_the_numpy_restatement_agree(name, b):
    """The optimiser of oracle/sde_mpc_numpy.py, fed the C oracle's cost and gradient (the arrangement of tests/test_second_restatement_cpu.py),
    writes the same event record, field for field and bit for bit, and the record changes nothing of the solve."""
    cfg, model, x0, xref, noise, u, s = sp.problem(name)
    O = orc.Oracle(cfg, model)
    uo, xe, io, ev = O.solve_events(x0[b], xref[b], noise[b], u[b], float(s))
    u1, x1, i1, _ = O.solve(x0[b], xref[b], noise[b], u[b], float(s))
    assert bits_differ(uo, u1) == 0 and bits_differ(xe, x1) == 0 and bits_differ(io, i1) == 0
    N = R.Restatement(cfg, model)
    events = []
    un, inf = N.solve(lambda uu: O.rollout(x0[b], uu, xref[b], noise[b])[0], lambda yy: O.grad(x0[b], yy, xref[b], noise[b]), u[b], float(s), events=events)
    assert bits_differ(un, uo) == 0 and bits_differ(inf, io) == 0
    assert len(events) == len(ev) >= 8
    for k, e in enumerate(events):
        row = np.array([e[f] for f in orc.EVENT_FIELDS], np.float32)
        assert bits_differ(row, ev[k]) == 0, (k, dict(zip(orc.EVENT_FIELDS, zip(row, ev[k]))))


@pytest.mark.parametrize("name", list(sp.CASES))
def test_case_reaches_the_paths_it_declares(name):
    c = sp.CASES[name]
    ref = sp.reference(name)
    seen = sp.census([r[3] for r in ref])
    assert set(c.declares) <= set(sp.PATH_NAMES) and c.declares
    assert set(c.declares) <= seen, sorted(set(c.declares) - seen)
    assert c.cfg["horizon"] <= 12 and c.cfg["max_iter"] <= 12 and c.P in (1, 20, 80, 100)
    if name not in sp.GUARD_CASES:
        assert all(np.isfinite(a).all() for r in ref for a in r[:3]), name


def test_union_of_the_cases_is_every_path():
    seen = sp.census([r[3] for name in sp.CASES for r in sp.reference(name)])
    assert seen == set(sp.PATH_NAMES), sorted(set(sp.PATH_NAMES) - seen)
    # ... and in the configurations the GPU tests run (a batch may hold fewer instances than the pool), per kernel
    for kernels in (("spec",), ("coop", "tile", "duo", "lane")):
        got = set()
        for conf in sp.configurations():
            if conf[1] in kernels and conf[4] == "exact" and conf[5] == "f32":
                got |= sp.census(sp.records_of(conf))
        assert got == set(sp.PATH_NAMES), (kernels, sorted(set(sp.PATH_NAMES) - got))


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_every_reachable_source_x_groups_cell_is_covered_on_256_compute_units(math):
    """Every cell of {y1, y2, y3, xk, recompute after a sequential trial, recompute because the role is absent} x ng = 2..7 that the role order
    allows is visited by a (case, batch) pair of the GPU test, in exact as a whole and in the fast subset again; so is each trial shape."""
    assert {conf[2] for conf in sp.configurations() if conf[1] == "spec" and conf[4] == math} == set(sp.NGS)
    assert all(conf[3] is not None for conf in sp.configurations())
    cc, shapes = sp.covered_cells()
    got = {cell for cell, confs in cc.items() if any(c[4] == math for c in confs)}
    assert got == set(sp.REACHABLE_CELLS), (sorted(set(sp.REACHABLE_CELLS) - got), sorted(got - set(sp.REACHABLE_CELLS)))
    assert all(any(c[4] == math for c in shapes.get(sh, [])) for sh in ("one", "two", "three"))


def test_role_model_on_hand_made_rows():
    row = lambda nls, acc, cause=0: dict(nls=nls, accepted=acc, cause=cause)
    src = sp.next_gradient_source
    assert [src(g, 4, row(1, 1)) for g in sp.NGS] == ["recompute_absent"] * 3 + ["y1"] * 3
    assert [src(g, 1, row(1, 1)) for g in sp.NGS] == ["recompute_absent"] + ["y1"] * 5              # one trial: the group of S(y2) takes y1
    assert [src(g, 4, row(2, 1)) for g in sp.NGS] == ["recompute_absent"] + ["y2"] * 5
    assert [src(g, 4, row(3, 1)) for g in sp.NGS] == ["recompute_sequential"] * 4 + ["recompute_absent", "y3"]
    assert [src(g, 4, row(4, 1)) for g in sp.NGS] == ["recompute_sequential"] * 6
    assert [src(g, 4, row(4, 0)) for g in sp.NGS] == ["recompute_absent"] * 2 + ["xk"] * 4
    assert src(7, 4, row(1, 1, cause=1)) is None and src(7, 4, row(2, 0, cause=3)) is None
    assert [sp.trial_shape(g, 3) for g in sp.NGS] == ["two"] * 4 + ["three"] * 2 and sp.trial_shape(7, 2) == "two" and sp.trial_shape(7, 0) == "one"
    assert [sp.spec_groups(80, B, 256) for B in range(1, 8)] == [7, 6, 4, 3, 2, 2, 0] and sp.spec_groups(100, 2, 256) == 5


@pytest.mark.parametrize("mutant", orc.MUTANTS)
def test_every_wrong_optimiser_changes_a_compared_bit(mutant):
    """Each one-line-wrong optimiser (oracle/sde_mpc_oracle.c, MUT_*) differs from SPEC.md §8 in uopt, xevol or info on at least one instance
    of the table: a kernel with that mistake cannot pass tests/test_gpu_solve_paths.py."""
    shown = []
    for name in sp.CASES:
        cfg, model, x0, xref, noise, u, s = sp.problem(name)
        O = orc.Oracle(cfg, model)
        for b, (uo, xe, io, _) in enumerate(sp.reference(name)):
            with orc.mutant(mutant):
                um, xm, im, _ = O.solve(x0[b], xref[b], noise[b], u[b], float(s))
            if bits_differ(um, uo) + bits_differ(xm, xe) + bits_differ(im, io):
                shown.append((name, b))
                break
    assert shown, f"{mutant} changes no compared bit on any case"
    # the hook is off again: the normative path
    name = shown[0][0]
    cfg, model, x0, xref, noise, u, s = sp.problem(name)
    b = shown[0][1]
    un = orc.Oracle(cfg, model).solve(x0[b], xref[b], noise[b], u[b], float(s))[0]
    assert bits_differ(un, sp.reference(name)[b][0]) == 0


def test_committed_matrix_is_current():
    with open(sp.MATRIX_MD) as f:
        assert f.read() == sp.matrix_markdown(), "tests/SOLVE_PATHS.md is stale: run python tests/solve_paths.py"
