"""The solve-path cases of tests/solve_paths.py on the CPU: the oracle's event record against the NumPy restatement's, the paths each case is
there for, the coverage of every named path and of every reachable cell of {source of the next gradient} x {groups per instance}, the ten
one-line-wrong optimisers, and the committed coverage matrix. No GPU."""
import os

import numpy as np
import pytest

import kernel_census as kc
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


# ---- the duo kernels: twins, team shapes, path coverage and the wrong optimisers on the duo case set alone ----------------------------------
@pytest.mark.parametrize("name", list(sp.DUO_CASES))
def test_duo_twin_reaches_the_paths_it_declares(name):
    c = sp.DUO_CASES[name]
    ref = sp.reference(name)
    seen = sp.census([r[3] for r in ref])
    assert c.declares and set(c.declares) <= set(sp.PATH_NAMES)
    assert set(c.declares) <= seen, sorted(set(c.declares) - seen)
    if name.endswith("_h4"):
        assert c.cfg["horizon"] == sp.h_mode4(c.m) and c.cfg["max_iter"] <= 6
    else:
        assert c.cfg["horizon"] <= 12 and c.cfg["max_iter"] <= 12
    assert 33 <= c.P <= 128 or c.P == 130
    assert c.m in (4, 6) and not c.spec_ng and not c.fast_ng
    if name not in sp.DUO_GUARD_CASES:
        assert all(np.isfinite(a).all() for r in ref for a in r[:3]), name


def test_existing_cases_are_untouched_by_the_twins():
    assert not set(sp.CASES) & set(sp.DUO_CASES) and sp.ALL_CASES["mix_p80"] is sp.CASES["mix_p80"]
    assert sp.SEQUENTIAL["duo"] == (dict(coop=0, pk=0, duo=1), ("mix_p80",)) and sp.SEQUENTIAL["tile"][1] == tuple(sp.CASES)
    for n in sp.P40_TWINS:
        base, twin = sp.CASES[n], sp.DUO_CASES[f"{sp._stem(n)}_p40"]
        assert {k: v for k, v in twin.cfg.items() if k != "num_particles"} == {k: v for k, v in base.cfg.items() if k != "num_particles"}
        assert (twin.seed, twin.s_in, twin.warm, twin.x0_scale, twin.declares, twin.m) == (base.seed, base.s_in, base.warm, base.x0_scale, base.declares, base.m)
    # every case that can take the duo layout in the default build does, in the pair
    pair = set(sp.DUO["pair"][4])
    assert {n for n, c in sp.CASES.items() if c.P >= 33} <= pair and len(pair) == len(sp.DUO["pair"][4])
    assert {n for n, c in sp.CASES.items() if c.P < 33} - {"tri_p20"} == set(sp.P40_TWINS) and sp.CASES["tri_p20"].m == 3


def test_dispatcher_takes_each_duo_team_shape_for_its_cases():
    """The dispatcher's own arithmetic (tests/kernel_census.py: pair_fits, duo_pick, shortest_h) at every (entry, case) of sp.DUO."""
    assert set(sp.DUO) == {"pair", "block2_ustg", "block2_mode4", "block_p130"}
    for lay, (opts, team, mode, ustg, names) in sp.DUO.items():
        assert names
        for n in names:
            c = sp.ALL_CASES[n]
            H, G = c.cfg["horizon"], (c.P + 31) // 32
            assert opts["coop"] == 0 and (opts.get("duo") == 1 or G > 4)
            if team == "TeamBlock":
                assert G >= 5 and c.P == 130 and kc.duo_pick(H, c.m, 4, opts.get("ustg", -1)) == 0 and (mode, ustg) == (3, False)
                continue
            assert 2 <= G <= 4 and sp.POOL < 6 * 16          # (no six-team workgroups at this batch on any device)
            if team == "TeamPairT<2>":
                assert kc.pair_fits(H, c.m) and opts.get("ustg", -1) != 1 and (mode, ustg) == (3, False)
            elif mode == 3:
                assert opts["ustg"] == 1 and ustg and kc.duo_pick(H, c.m, 2, 1) == 1 and H <= 12
            else:
                assert ustg and H == kc.shortest_h(lambda h: not kc.pair_fits(h, c.m) and kc.duo_pick(h, c.m, 2) == 2)
                assert not kc.pair_fits(H, c.m) and kc.duo_pick(H, c.m, 2, opts.get("ustg", -1)) == 2
            assert sp.duo_kernel(lay, n) == f"sdempc_solve_kernel<{team}, {c.m}, 0, false, {mode}, {'true' if ustg else 'false'}>"
    built = kc.built_kernels()
    if built is not None:
        want = {(sp.duo_kernel(lay, n), "exact") for lay, e in sp.DUO.items() for n in e[4]}
        want |= {(sp.duo_kernel("pair", n, mlp), "exact" if math == "exact" else "fast") for n, mlp, math in sp.DUO_ARITH}
        assert want <= built, sorted(want - built)


def _duo_records(layouts, arith=False):
    return [rec for conf in sp.configurations() if conf[1] in layouts and ((conf[4], conf[5]) == ("exact", "f32") or arith) for rec in sp.records_of(conf)]


def test_pair_configurations_reach_every_path():
    seen = sp.census(_duo_records(("pair",)))
    assert seen == set(sp.PATH_NAMES), sorted(set(sp.PATH_NAMES) - seen)


@pytest.mark.parametrize("layout", ["block2_ustg", "block2_mode4", "block_p130"])
def test_each_other_duo_team_shape_reaches_the_required_paths(layout):
    seen = sp.census(_duo_records((layout,)))
    missing = [r for r in sp.DUO_REQUIRED if not ({r} if isinstance(r, str) else set(r)) & seen]
    assert not missing, (layout, missing)
    flat = {n for r in sp.DUO_REQUIRED for n in ((r,) if isinstance(r, str) else r)}
    assert flat <= set(sp.PATH_NAMES) and len(sp.DUO_REQUIRED) == 10


def test_duo_arithmetic_cases_are_a_guard_case_and_a_case_of_mixed_endings():
    assert {(mlp, math) for _, mlp, math in sp.DUO_ARITH} == {("f16", "exact"), ("f32x3", "exact"), ("f32x3", "fast"), ("f16", "fast")}
    for name, mlp, math in sp.DUO_ARITH:
        assert name in sp.DUO["pair"][4]
        causes = {int(r[3].col("cause")[-1]) for r in sp.reference(name, math, mlp)}
        assert causes == {4} if name.startswith("guard_") else len(causes) >= 2, (name, mlp, math, causes)


@pytest.mark.parametrize("mutant", orc.MUTANTS)
def test_every_wrong_optimiser_changes_a_compared_bit_on_the_duo_case_set(mutant):
    """As above, on the cases that the duo kernels run and on nothing else."""
    names = list(dict.fromkeys(n for e in sp.DUO.values() for n in e[4]))
    shown = None
    for name in names:
        cfg, model, x0, xref, noise, u, s = sp.problem(name)
        O = orc.Oracle(cfg, model)
        for b, (uo, xe, io, _) in enumerate(sp.reference(name)):
            with orc.mutant(mutant):
                um, xm, im, _ = O.solve(x0[b], xref[b], noise[b], u[b], float(s))
            if bits_differ(um, uo) + bits_differ(xm, xe) + bits_differ(im, io):
                shown = (name, b)
                break
        if shown:
            break
    assert shown, f"{mutant} changes no compared bit on any duo case"
    name, b = shown
    cfg, model, x0, xref, noise, u, s = sp.problem(name)
    assert bits_differ(orc.Oracle(cfg, model).solve(x0[b], xref[b], noise[b], u[b], float(s))[0], sp.reference(name)[b][0]) == 0          # the hook is off again


def test_committed_matrix_is_current():
    with open(sp.MATRIX_MD) as f:
        assert f.read() == sp.matrix_markdown(), "tests/SOLVE_PATHS.md is stale: run python tests/solve_paths.py"
