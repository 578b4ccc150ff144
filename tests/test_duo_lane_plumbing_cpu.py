"""A NumPy model of the two lane-swap instructions, as xor32_sum / xor16_sum (sdempc_kernels.hip) and tools/lane_probe.hip state them, and on it the
two rearrangements of the duo layout's lane plumbing:
  * duo_pair_inputs: three v_permlane32_swap of (z[2 s], z[2 s + 1]) yield exactly the layer-1 B operands that six half_split broadcasts followed by the per-half
    select `h ? z[2 s + 1] : z[2 s]` yield, for pass A and for pass B;
  * group_bfly32_pairs / group_pair_store: the reduction of N per-lane values over each 32-lane group, two values per register, adds at every stage and for
    every value the same unordered operand pairs as group_bfly32 does, and leaves the totals in lanes 0 and 16 of each group (N = 8, 9, 10).
A wave is an array of 64 lanes; rows are 16 lanes, halves 32."""
import numpy as np
import pytest

LANES = np.arange(64)
ROW, HALF = LANES >> 4, LANES >> 5


# ---- the instructions ----------------------------------------------------------------------------------------------------------------------
def permlane32_swap(a, b):
    """v_permlane32_swap a, b: a's upper half and b's lower half change places -> {a.lo, b.lo}, {a.hi, b.hi}"""
    a, b = np.asarray(a), np.asarray(b)
    return np.concatenate([a[:32], b[:32]]), np.concatenate([a[32:], b[32:]])


def permlane16_swap(a, b):
    """v_permlane16_swap a, b: a's odd rows and b's even rows change places -> {a.r0, b.r0, a.r2, b.r2}, {a.r1, b.r1, a.r3, b.r3}"""
    a, b = np.asarray(a), np.asarray(b)
    r = lambda v, i: v[16 * i:16 * i + 16]
    return np.concatenate([r(a, 0), r(b, 0), r(a, 2), r(b, 2)]), np.concatenate([r(a, 1), r(b, 1), r(a, 3), r(b, 3)])


def row_ror(v, n):
    """DPP row_ror:n — lane i of a row reads lane (i - n) mod 16 of the same row"""
    return np.asarray(v)[(ROW << 4) | ((LANES - n) & 15)]


def quad_perm(v, p):
    """DPP quad_perm — lane i reads lane p[i & 3] of its quad"""
    return np.asarray(v)[(LANES & ~3) | np.asarray(p)[LANES & 3]]


# ---- the kernels' helpers on the model, generic in the addition ---------------------------------------------------------------------------------
def dpp_stages(s, add, trace):
    for src in (lambda v: row_ror(v, 8), lambda v: row_ror(v, 4), lambda v: quad_perm(v, [2, 3, 0, 1]), lambda v: quad_perm(v, [1, 0, 3, 2])):
        s = add(s, src(s))
        trace.append(s)
    return s


def group_bfly32(v, add, trace=None):
    trace = [] if trace is None else trace
    r0, r1 = permlane16_swap(v, v)              # xor16_sum: the value and an opaque copy of it
    s = add(r0, r1)
    trace.append(s)
    return dpp_stages(s, add, trace)


def group_bfly32_pairs(vals, add, traces):
    """vals: N lane arrays. Returns what the kernel leaves in v[]: v[2 i] = the pair's register, v[N - 1] of an odd N = its plain butterfly."""
    vals = list(vals)
    N = len(vals)
    for i in range(0, N - 1, 2):
        r0, r1 = permlane16_swap(vals[i], vals[i + 1])
        s = add(r0, r1)
        traces[i] = [s]
        vals[i] = dpp_stages(s, add, traces[i])
    if N & 1:
        traces[N - 1] = []
        vals[N - 1] = group_bfly32(vals[N - 1], add, traces[N - 1])
    return vals


def group_pair_store(vals, own):
    """dst[half][k] as the masked stores write it; every slot must be written exactly once per owning half."""
    N = len(vals)
    dst = [[None] * N for _ in range(2)]
    j = LANES & 31
    for lane in LANES:
        wr = own[lane] and (j[lane] & 15) == 0
        for i in range(0, N - 1, 2):
            if wr:
                k = i + (j[lane] >> 4)
                assert dst[HALF[lane]][k] is None
                dst[HALF[lane]][k] = vals[i][lane]
        if (N & 1) and wr and j[lane] == 0:
            assert dst[HALF[lane]][N - 1] is None
            dst[HALF[lane]][N - 1] = vals[N - 1][lane]
    return dst


# ---- A. paired inputs ------------------------------------------------------------------------------------------------------------------------------
def test_three_swaps_yield_the_operands_of_half_split_and_select():
    rng = np.random.default_rng(0)
    z = [rng.standard_normal(64).astype(np.float32) for _ in range(6)]          # lanes 0..31: group A's particles, 32..63: group B's
    zA, zB = zip(*[permlane32_swap(v, v.copy()) for v in z])                      # half_split: {v.lo, v.lo}, {v.hi, v.hi}
    for k in range(6):
        assert np.array_equal(zA[k], np.tile(z[k][:32], 2)) and np.array_equal(zB[k], np.tile(z[k][32:], 2))
    for s in range(3):
        bA, bB = permlane32_swap(z[2 * s], z[2 * s + 1])
        assert bA.tobytes() == np.where(HALF == 1, zA[2 * s + 1], zA[2 * s]).tobytes()
        assert bB.tobytes() == np.where(HALF == 1, zB[2 * s + 1], zB[2 * s]).tobytes()


# ---- B. paired group sums --------------------------------------------------------------------------------------------------------------------------
def _sym_add(a, b):
    """An addition as the unordered pair of its operands (IEEE addition commutes): nested frozensets record the whole tree."""
    return np.array([frozenset((x, y)) for x, y in zip(a, b)], dtype=object)


def _leaves(N):
    out = []
    for k in range(N):
        v = np.empty(64, dtype=object)
        for l in range(64):
            v[l] = (k, l)
        out.append(v)
    return out


@pytest.mark.parametrize("N", [8, 9, 10])
def test_paired_reduction_adds_the_same_operand_pairs_as_group_bfly32(N):
    vals = _leaves(N)
    old = {}
    for k in range(N):
        old[k] = []
        group_bfly32(vals[k], _sym_add, old[k])
    new = {}
    out = group_bfly32_pairs(vals, _sym_add, new)
    for k in range(N):
        paired = k < (N & ~1)
        reg, odd = (k & ~1, k & 1) if paired else (k, 0)
        assert len(new[reg]) == len(old[k]) == 5
        for stage in range(5):
            for half in range(2):
                for col in range(16):
                    # value k of a pair lives in rows 2 half (even k) / 2 half + 1 (odd k) of the pair's register; column col of either row of the
                    # plain butterfly holds the same unordered pair (partner lanes are equal after every stage)
                    lane_new = 32 * half + 16 * odd + col
                    for row in range(2):
                        assert new[reg][stage][lane_new] == old[k][stage][32 * half + 16 * row + col], (k, stage, half, col)
                    if not paired:
                        assert new[reg][stage][lane_new + 16] == old[k][stage][lane_new]
    # the totals: lanes j == 0 and j == 16 of each group, stored once each, equal to the plain butterfly's
    dst = group_pair_store(out, np.ones(64, bool))
    for half in range(2):
        for k in range(N):
            assert dst[half][k] == old[k][4][32 * half], (half, k)
            leaves = set()
            def walk(n):
                if isinstance(n, frozenset):
                    for c in n: walk(c)
                else:
                    leaves.add(n)
            walk(dst[half][k])
            assert leaves == {(k, 32 * half + l) for l in range(32)}          # every particle of the group, nothing of the other half or value


@pytest.mark.parametrize("N", [8, 9, 10])
def test_paired_reduction_gives_the_bits_of_group_bfly32_and_respects_ownership(N):
    rng = np.random.default_rng(N)
    vals = [(rng.standard_normal(64) * np.exp2(rng.integers(-20, 20, 64))).astype(np.float32) for _ in range(N)]
    fadd = lambda a, b: (a + b).astype(np.float32)
    plain = [group_bfly32(v, fadd) for v in vals]
    out = group_bfly32_pairs(vals, fadd, {})
    own = HALF == 0                                   # a pair without a group B: the upper half must not store
    dst = group_pair_store(out, own)
    for k in range(N):
        assert np.float32(dst[0][k]).tobytes() == plain[k][0].tobytes()
        assert dst[1][k] is None
    dst = group_pair_store(out, np.ones(64, bool))
    for half in range(2):
        for k in range(N):
            assert np.float32(dst[half][k]).tobytes() == plain[k][32 * half].tobytes()
