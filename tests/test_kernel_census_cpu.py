"""The kernel census of tests/kernel_census.py on the CPU: the table against the symbol table of the built library, every row's problem against
the oracle alone (a row whose solve does not move, or whose gradient has a dead motor column, could not tell a wrong kernel from a right one), the
unreachable kernels, and the committed matrix tests/KERNELS.md. No GPU.

Two builds, two tables. The default build (csrc/libsdempc.so) carries exactly table_names(). The all-variants build (make allvariants:
csrc/allvariants/libsdempc.so; sdempc_build_flags() & 1) carries those and the kernels of ALL_ROWS (the generic motor count in every layout, the
packed-tanh latency instantiations), again exactly, in both directions; so does a library at the default path that was itself built with
EXTRA=-DSDEMPC_ALL_VARIANTS=1. The new rows' problems are held to the same conditions as the default ones."""
import numpy as np
import pytest

import kernel_census as kc
import orc

EV = orc.EVENT_FIELDS


def _built(where=kc.CSRC):
    built = kc.built_kernels(where)
    if built is None:
        pytest.skip(f"libsdempc.so / its objects are not built in {where}, or nm is missing")
    return built


def test_normalise_strips_what_the_two_spellings_differ_in():
    stub = ("0000000000000000 W void sdempc::fastm::__device_stub__sdempc_loop_period_kernel<1, true, false, true>(sdempc::KArgs, sdempc::LoopAdvance, "
            "std::conditional<true, sdempc::LoopScenario, sdempc::fastm::LoopAbsent>::type)")
    import re
    assert kc.normalise(re.sub(r"^[0-9a-fA-F]*\s+\S\s+", "", stub)) == ("sdempc_loop_period_kernel<1, true, false, true>", "fast")
    assert kc.normalise("sdempc::exact::sdempc_solve_kernel<sdempc::exact::TeamPairT<2>, 4, 2, false, 3, false>") == \
        ("sdempc_solve_kernel<TeamPairT<2>, 4, 2, false, 3, false>", "exact")
    assert kc.normalise("void sdempc::exact::__device_stub__sdempc_solve_spec_kernel<6, true>(sdempc::KArgs)") == ("sdempc_solve_spec_kernel<6, true>", "exact")
    assert kc.normalise("sdempc::__device_stub__sdempc_noise_kernel(unsigned int const*, float*, int, int, int, int)") == ("sdempc_noise_kernel", "")


def test_table_names_exactly_the_kernels_of_the_build():
    """Both directions in the default build: a kernel nobody dispatches and a row for a kernel that no longer exists both fail."""
    from sde4mbrl_px4_amd import _abi
    built, table = _built(), kc.table_names()
    per_mode = {md: sum(m == md for _, m in built) for md in ("exact", "fast", "")}
    print(f"built: {len(built)} kernels ({per_mode}); table: {len(kc.ROWS)} rows + {len(kc.ELSEWHERE)} mapped to existing tests + {len(kc.UNREACHED)} unreachable")
    missing = sorted(table - built)
    assert not missing, f"in the table but not built: {missing}"
    extra = set(built - table)
    if _abi.load_library().sdempc_build_flags() & 1:
        print(f"all-variants build at the default path: {len(extra)} kernels beyond the default table")
        assert extra == kc.all_names(), f"in no row of ALL_ROWS: {sorted(extra - kc.all_names())}; in ALL_ROWS but not built: {sorted(kc.all_names() - extra)}"
    else:
        assert not extra, f"built but in no row, no existing test and not declared unreachable: {sorted(extra)}"


def test_both_tables_name_exactly_the_kernels_of_the_all_variants_build():
    """csrc/allvariants: the default table's names and ALL_ROWS' names, both directions."""
    built, table = _built(kc.AV_DIR), kc.table_names() | kc.all_names()
    print(f"built: {len(built)} kernels; tables: {len(kc.table_names())} + {len(kc.all_names())}")
    assert not sorted(table - built), f"in the tables but not built: {sorted(table - built)}"
    assert not sorted(built - table), f"built but in no row, no existing test and not declared unreachable: {sorted(built - table)}"


def test_table_is_one_entry_per_kernel():
    rows = [(r.kernel, r.mode) for r in kc.ROWS]
    assert len(set(rows)) == len(rows) and len({r.id for r in kc.ROWS}) == len(rows)
    assert not (set(rows) & set(kc.ELSEWHERE)) and not (set(rows) & set(kc.UNREACHED)) and not (set(kc.ELSEWHERE) & set(kc.UNREACHED))
    assert len(kc.UNREACHED) <= 4 and all(why for why in kc.UNREACHED.values())
    # the all-variants rows: one untagged row per kernel, none of them a kernel of the default table; ids unique across both tables
    plain = [(r.kernel, r.mode) for r in kc.ALL_ROWS if not r.tag]
    assert len(set(plain)) == len(plain) == len(kc.all_names()) == 71 and not (set(plain) & kc.table_names())
    tagged = [r for r in kc.ALL_ROWS if r.tag]
    assert [(r.kernel, r.batch) for r in tagged] == [("sdempc_solve_kernel<TeamBlock, 4, 0, true, 0, false>", "cus"),
                                                     ("sdempc_solve_kernel<TeamBlock, 4, 0, false, 0, false>", "cus + 1")]
    assert len({r.id for r in kc.ROWS + kc.ALL_ROWS}) == len(kc.ROWS) + len(kc.ALL_ROWS)
    assert all(r.m == kc.GENERIC_M for r in kc.ALL_ROWS if ", 8, " in r.kernel or "<8, " in r.kernel)
    for r in kc.ROWS + kc.ALL_ROWS:
        assert r.mode in kc.MODES and r.kind in ("solve", "solve_keys", "grad", "rollout") and r.mlp in kc.F16_OF
        assert "test_absent_wg" not in dict(r.options), r.id
        assert 1 <= r.B(256) and sorted(r.sample(256))[-1] == r.B(256) - 1 and len(r.sample(256)) <= 4
        assert r.cfg_kw()["max_iter"] in (3, 4) and (6 <= r.H <= 12 or r.note), r.id      # a longer horizon carries its derivation


def test_rows_chosen_by_the_lds_budget_sit_on_the_threshold():
    """The shortest horizon of each derived row: one step shorter and the dispatcher's arithmetic picks another instantiation."""
    derived = [r for r in kc.ROWS + kc.ALL_ROWS if r.H > 12]
    assert len(derived) == 48 + 24
    for r in derived:
        M = r.m
        if "TeamBlock, " in r.kernel and r.kernel.endswith("false, 0, true>"):
            assert kc.global_table(r.H, M) and not kc.global_table(r.H - 1, M), r.id
        elif "TeamBlock2" in r.kernel and r.kernel.endswith("3, false>"):
            assert not kc.pair_fits(r.H, M) and kc.pair_fits(r.H - 1, M) and kc.duo_pick(r.H, M, 2, 0) == 0, r.id
        elif "TeamBlock2" in r.kernel and r.kernel.endswith("4, true>"):
            assert not kc.pair_fits(r.H, M) and kc.duo_pick(r.H, M, 2) == 2 and (kc.pair_fits(r.H - 1, M) or kc.duo_pick(r.H - 1, M, 2) != 2), r.id
        elif "TeamBlock, " in r.kernel and r.kernel.endswith("4, true>"):
            assert kc.duo_pick(r.H, M, 4) == 2 and kc.duo_pick(r.H - 1, M, 4) != 2, r.id
        else:
            raise AssertionError(f"{r.id}: a long horizon without a threshold to sit on")
        assert kc.smem_bytes(r.H, M, 1, False, True, 4) <= 160 * 1024


def test_existing_tests_named_for_the_unnamed_kernels_exist():
    """module::function[parametrisation] of every kernel mapped to an existing test: the module has that function, and each parameter value occurs
    in the module's text (a renamed test or a dropped parametrisation fails here)."""
    import os
    import re
    for (kernel, mode), test in kc.ELSEWHERE.items():
        mod, rest = test.split("::")
        fn, params = re.match(r"(\w+)(?:\[(.*)\])?$", rest).groups()
        src = open(os.path.join(kc.ROOT, "tests", mod + ".py")).read()
        assert f"def {fn}(" in src, test
        src += open(os.path.join(kc.ROOT, "tests", "loop_cases.py")).read()
        assert all(re.search(rf"\b{re.escape(tok)}\b", src) for tok in (params or "").split("-") if tok), test
        assert mod.startswith("test_gpu_"), test
    # the closed loop: seven routes x six arithmetics, both namespaces
    loop = [k for k in kc.ELSEWHERE if "loop_tick" in k[0] or "loop_period" in k[0]]
    assert len(loop) == 42 and sum(m == "fast" for _, m in loop) == 21


@pytest.mark.parametrize("row", [r for r in kc.ROWS + kc.ALL_ROWS if r.kind in ("solve", "solve_keys")], ids=lambda r: r.id)
def test_every_solve_row_can_fail(row):
    """The oracle alone, on the sampled instances: at least two iterations, at least one accepted step (uopt differs from the warm start in some
    word), all outputs finite."""
    prob, ref = kc.reference(row)
    assert sorted(ref) == row.sample()
    for b, (uopt, xevol, info, ev) in ref.items():
        assert info[2] >= 2, (b, info)
        assert ev[:, EV.index("accepted")].sum() >= 1 and info[6] < info[5], (b, info)
        start = np.clip(prob["u"][b], *np.asarray(row.cfg().input_bound, np.float32).T)
        assert (uopt.view(np.uint32) != start.view(np.uint32)).any(), b
        assert np.isfinite(uopt).all() and np.isfinite(xevol).all() and np.isfinite(info).all(), b


@pytest.mark.parametrize("row", [r for r in kc.ROWS if r.kind in ("grad", "rollout")], ids=lambda r: r.id)
def test_every_gradient_and_rollout_row_can_fail(row):
    """The gradient of the row's problem is finite and non-zero in every motor column (for a rollout row: the gradient at the rolled-out controls, so
    that every motor reaches the compared cost, trajectory and mean)."""
    prob, ref = kc.reference(row)
    O = orc.Oracle(row.cfg(), row.model())
    for b, res in ref.items():
        c, g = res if row.kind == "grad" else O.grad(prob["x0"][b], prob["u"][b], prob["xref"][b], kc.noise_of(prob, row, b))
        assert np.isfinite(c) and np.isfinite(g).all() and (np.abs(g).max(axis=0) > 0).all(), (b, np.abs(g).max(axis=0))
        assert all(np.isfinite(np.asarray(a, np.float64)).all() for a in res), b


def test_committed_matrix_is_current():
    with open(kc.KERNELS_MD) as f:
        assert f.read() == kc.kernels_markdown(), "tests/KERNELS.md is stale: run python tests/kernel_census.py"
    with open(kc.KERNELS_ALL_MD) as f:
        assert f.read() == kc.kernels_all_markdown(), "tests/KERNELS_ALL.md is stale: run python tests/kernel_census.py"
