"""The pools and the arrangement of tests/mixed_batch_cases.py on the CPU, from the oracle's records alone: each pool ends in several ways, holds
the iteration counts and the two kinds of guarded solve the GPU test is about, every two of its instances can be told apart, and the striped order
of every launch puts each abnormal ending in front of and behind a full-length solve on some team. No GPU."""
import itertools

import numpy as np
import pytest

import kernel_census as kc
import mixed_batch_cases as mb
import orc
from cases import asymmetric_problem, bits_differ

POOLS = sorted({(L.pool, L.P, L.m) for L in mb.LAUNCHES})


def test_pool_shapes_are_what_the_launches_need():
    assert {p for p, _, _ in POOLS} == set(mb.POOLS)
    for name, p in mb.POOLS.items():
        assert (16 <= p.K <= 32 and p.max_iter <= 12) if name != "mode4" else (p.K <= 12 and p.max_iter <= 6), name
    for pool, P, m in POOLS:
        cfg = mb.pool_cfg(pool, P, m)
        assert cfg.max_iter == mb.POOLS[pool].max_iter and cfg.num_particles == P <= 160
        assert cfg.horizon == (mb.h_mode4(m) if pool == "mode4" else mb.POOLS[pool].H) and (pool == "mode4" or cfg.horizon <= 10)
    assert (mb.P2 + 31) // 32 == 3 and (mb.P4 + 31) // 32 == 5
    # every instance has inputs of its own
    for pool, P, m in POOLS:
        _, _, x0, xref, noise, u, s = mb.problem(pool, P, m)
        for a in (x0, xref, noise, u, s):
            flat = a.reshape(len(a), -1)
            assert all(flat[i].tobytes() != flat[j].tobytes() for i, j in itertools.combinations(range(len(a)), 2)), (pool, P, m)


def test_u_opt_instances_start_where_the_oracle_ended():
    for pool, P, m in POOLS:
        cfg, model, x0, xref, noise, u, s = mb.problem(pool, P, m)
        O = orc.Oracle(cfg, model)
        i = mb.POOLS[pool].kinds.index("u_opt")
        u_first = asymmetric_problem(cfg, mb.POOLS[pool].K, mb.POOLS[pool].seed)[3][i]
        assert bits_differ(O.solve(x0[i], xref[i], noise[i], u_first, float(s[i]))[0], u[i]) == 0, (pool, P, m)


@pytest.mark.parametrize("pool,P,m", POOLS)
def test_pool_conditions(pool, P, m):
    ref, p = mb.reference(pool, P, m), mb.POOLS[pool]
    ends = mb.endings(pool, P, m)
    causes = {int(r[3].col("cause")[-1]) for r in ref}
    assert len(causes) >= 4, causes                                                                  # 1. at least four different causes
    counts = {int(r[2][2]) for r in ref}
    assert {0, 1, p.max_iter} <= counts, counts                                                      # 2. iteration counts 0, 1 and max_iter
    assert "k0_nonfinite" in ends and "k0_finite" in ends, ends                                      # 3. guard at k = 0, non-finite and finite xevol
    for r, e in zip(ref, ends):
        if e == "k0_nonfinite":
            assert not np.isfinite(r[1]).all() and len(r[3].ev) == 1 and r[3].col("cause")[0] == 4
        if e == "k0_finite":
            assert np.isfinite(r[1]).all() and len(r[3].ev) == 1 and r[3].col("cause")[0] == 4
        if e == "full":
            assert int(r[2][2]) == p.max_iter and all(np.isfinite(a).all() for a in r[:3])
        if e == "tol1":
            assert int(r[2][2]) == 1 and r[3].col("cause")[-1] == 2
        if e == "kgt0":
            assert r[3].col("cause")[-1] == 4 and len(r[3].ev) > 1
    assert 3 * ends.count("full") >= p.K, ends                                                        # 4. a third runs to max_iter, finite
    for (i, a), (j, b) in itertools.combinations(enumerate(ref), 2):                                 # 5. any two can be told apart
        assert bits_differ(a[0], b[0]) > 0, (i, j, "uopt")
        assert not np.isnan(a[2]).all() and not np.isnan(b[2]).all()          # (no info row of these pools is all-NaN)
        assert bits_differ(a[2], b[2]) > 0, (i, j, "info")
    assert "tol1" in ends and ("kgt0" in ends) == (p.base == "guard_kgt0_p80")


def test_both_pools_together_hold_every_abnormal_kind():
    assert set(mb.ABNORMAL) <= set(mb.endings("mix", mb.P2)) | set(mb.endings("guard", mb.P2))
    assert set(mb.ABNORMAL) <= set(mb.endings("guard", mb.P2)) and set(mb.ABNORMAL) <= set(mb.endings("guard", mb.P4))


def test_team_slots_restate_the_grid_of_a_persistent_launch():
    """156 KiB of LDS per CU, twelve waves per CU: 1,536 team slots on 256 CUs for every two-wave shape at these horizons, 768 for the four-wave team."""
    for L in mb.LAUNCHES:
        want = 768 if L.team == "TeamBlock" else 1536
        assert L.slots(256) == want, (L.id, L.slots(256))
        assert mb.ticketed(L.B(256), L.slots(256)) == (L.how == "ticketed")
        assert L.B(256) >= 6 * 256
    assert mb.team_slots(mb.kernel_name("TeamBlock", 4, "f32", 4, True), 175, 4, 256) == 3 * 256
    assert mb.team_slots(mb.kernel_name("TeamPairT<2>", 4, "f32"), 50, 4, 256) == 6 * 256          # the benchmark's C2 shape
    assert mb.team_slots(mb.kernel_name("TeamBlock2", 4, "f32", 3, False), 200, 4, 256) < 6 * 256    # LDS-bound


def test_launch_kernels_are_what_the_dispatcher_picks():
    """The dispatcher's arithmetic (tests/kernel_census.py) at the pools' horizons: the pair fits at H <= 10, the MODE 4 horizon is the shortest
    one that selects it, ustg = 1 gives MODE 3 with the global table at a short horizon."""
    names = {kc.normalise(L.kernel())[0] for L in mb.LAUNCHES}
    for t in ("TeamPairT<2>, 4, 0, false, 3, false", "TeamPairT<6>, 4, 0, false, 3, false", "TeamBlock2, 4, 0, false, 3, true", "TeamBlock2, 4, 0, false, 4, true",
              "TeamBlock, 4, 0, false, 3, false", "TeamPairT<2>, 6, 0, false, 3, false", "TeamPairT<2>, 4, 1, false, 3, false", "TeamPairT<2>, 4, 2, false, 3, false",
              "TeamBlock, 4, 1, false, 3, false", "TeamBlock, 4, 2, false, 3, false"):
        assert f"sdempc_solve_kernel<{t}>" in names, t
    for L in mb.LAUNCHES:
        H, o = L.H(), dict(L.options)
        if L.team.startswith("TeamPairT"):
            assert kc.pair_fits(H, L.m) and kc.smem_bytes(H, L.m, 6, False, True, 12) <= kc.LDS_CAP
            assert kc.throughput_kernel(H, L.P, L.m, mb.MODE[L.mlp], L.B(256) if o.get("hex", 1) else 6 * 256 - 1) == L.kernel()
        elif L.team == "TeamBlock2":
            assert (not kc.pair_fits(H, L.m) and o["hex"] == 0) or o.get("ustg") == 1
            assert kc.duo_pick(H, L.m, 2, o.get("ustg", -1)) == (2 if L.mode == 4 else 1)
            assert L.mode == 3 or H == mb.h_mode4(L.m) == kc.shortest_h(lambda h: not kc.pair_fits(h, L.m) and kc.duo_pick(h, L.m, 2) == 2)
        else:
            assert L.P > 128 and kc.duo_pick(H, L.m, 4) == 0
            assert kc.throughput_kernel(H, L.P, L.m, mb.MODE[L.mlp], L.B(256)) == L.kernel()


def test_order_is_fixed_and_no_stride_repeats_an_instance():
    idx = mb.order(4699, 24)
    assert np.array_equal(idx, mb.order(4699, 24)) and set(idx.tolist()) == set(range(24))
    assert not np.array_equal(idx[:1536], idx[1536:3072])
    for stride in (768, 1536):
        same = (idx[:-stride] == idx[stride:]).mean()
        assert same < 0.1, (stride, same)          # (b % K at a stride that K divides: 1.0)


@pytest.mark.parametrize("L", [L for L in mb.LAUNCHES if L.how == "striped"], ids=lambda L: L.id)
def test_striped_launch_puts_every_abnormal_ending_next_to_a_full_solve_on_some_team_at_256_cus(L):
    cus = 256
    ends = mb.endings(L.pool, L.P, L.m, L.math, L.mlp)
    slots, B = L.slots(cus), L.B(cus)
    assert not mb.ticketed(B, slots)
    idx = mb.order(B, mb.POOLS[L.pool].K)
    need = mb.required_successions(ends)
    assert len(need) >= 4
    got = mb.successions(idx, ends, slots)
    assert need <= got, sorted(need - got)
    # the same from the teams' own sequences
    seq = mb.team_sequences(B, slots)
    assert sorted(b for t in seq for b in t) == list(range(B)) and max(map(len, seq)) == 3 and min(map(len, seq)) == 2
    assert got == {(ends[idx[a]], ends[idx[b]]) for t in seq for a, b in zip(t, t[1:])}


def test_endings_hold_in_every_arithmetic_that_is_launched():
    """The other arithmetics keep what the launches are about: guarded, one-iteration and full-length solves side by side."""
    for key in sorted({(L.pool, L.P, L.m, L.math, L.mlp) for L in mb.LAUNCHES if (L.math, L.mlp) != ("exact", "f32")}):
        ends = mb.endings(*key)
        assert {"k0_nonfinite", "k0_finite", "tol1", "full"} <= set(ends) and 3 * ends.count("full") >= len(ends), (key, ends)


def test_expected_work_and_settled_trials_on_the_pool():
    ref = mb.reference("guard", mb.P2)
    n, grads, fwd = mb.expected_work(ref, [0, 0, 4])
    one = lambda i: mb.expected_work(ref, [i])
    assert n == 3 and grads == 2 * one(0)[1] + one(4)[1] and fwd == 2 * one(0)[2] + one(4)[2]
    assert one(4)[1:] == (1, 2) and mb.endings("guard", mb.P2)[4] == "k0_nonfinite"          # the guard's gradient; the initial cost and the final mean
    st = mb.settled_trials("guard", mb.P2)
    assert len(st) == mb.POOLS["guard"].K and all(0 <= v <= int(r[2][7]) for v, r in zip(st, ref))
