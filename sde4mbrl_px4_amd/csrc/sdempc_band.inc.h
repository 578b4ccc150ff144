// sdempc_band.inc.h — predicted bands (SPEC.md §12b): per column of the particle x horizon tensor a store_traj rollout left in the handle, the values at up
// to eight requested ranks of the total key order over the valid particles (q), and the number of particles below / at an observed value (below, at).
// Included by sdempc_prng.hip after sdempc_tube.inc.h and sdempc_risk.inc.h: the reducer runs as one more mode of sdempc_noise_kernel, selected by
// BandArgs::traj.
//
// Path replaced (reference): none on the device — the reference returns the particle mean only (xevol, sde_control.py:698,717); a quantile across particles
// was np.sort on the host over rollout(want_traj=True), i.e. a relayout and a copy of the whole tensor.
//
// Mapping: the tube's grid (sdempc_tube.inc.h) — a workgroup takes one instance and one tile of 32 columns, each of its eight 32-lane halves the four columns
// c = tile*32 + half + 8 j; every (b, g, c) row is one 128-byte line with the particle in the lane. No LDS, no matrix pipe, no arithmetic on the values: every
// word becomes its uint32 key (one total order, NaN on top), and everything below is unsigned compares.
//   G <= 4 (up to P = 128): the column's <= 4 words per lane are loaded once — the next column's are requested before this one's network runs — and sorted where they are: a
//     bitonic network over 128 elements, element e = 4 lane + register, so that the partner distances 1 and 2 are register pairs of one lane and 4 .. 64 are
//     the lane partners l ^ 1, 2, 4, 8, 16 (quad_perm, quad_perm, ds_swizzle, row_ror:8 — exact inside a row of 16 —, ds_swizzle). Padded lanes carry key
//     0xFFFFFFFF and sort to the top, beside the NaNs they are indistinguishable from; a rank < P never reaches past the valid ones. Rank r then sits in
//     register r & 3 of lane r >> 2; lane k of the half fetches rank ranks[k] (four ds_bpermute, one per register, serve all Q ranks). 28 compare-exchange steps: 15 across lanes (per register: one lane move, min, max, select) and
//     13 inside a lane (per pair: min, max, two selects) — about 350 VALU instructions per column whatever Q is.
//   G > 4: nothing is kept. Per column 32 rounds, most significant bit first: pivot_k = prefix_k | bit for every requested rank k at once, one pass over the
//     column's G lines (from the cache after the first round), per line one key conversion and per rank one compare, ballot and popcount; the rank's prefix
//     takes the bit where at most ranks[k] keys lie below the pivot. The prefix after bit 0 is the key of that rank. Per column about 32 G (6 + 4 Q)
//     instructions, no register per group and no particle limit.
//   below / at: one compare pass with ballot + popcount over the keys (before the sort; the padded lanes masked), as the tube's `outside`.
// Per column lane k (< Q) of the half stores plane k's word (one store instruction for all planes) and lane 0 stores below / at.
#pragma once

namespace sdempc {

// SPEC.md §12b: the key of a word — -inf < ... < -0 < +0 < ... < +inf < NaN as unsigned integers, all NaNs one key
DI uint32_t band_key(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t k = (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
    return v != v ? 0xFFFFFFFFu : k;
}
// the word of a key; the NaN key gives the quiet NaN 0x7FC00000
DI uint32_t band_word(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    return k == 0xFFFFFFFFu ? 0x7FC00000u : u;
}

template <int CTRL>
DI uint32_t band_dpp(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
// value of lane l ^ M inside the 32-lane half (M = 1, 2, 4, 8, 16): the TRUE xor partners — a sort has no periodic rows to lean on
template <int M>
DI uint32_t band_xor(uint32_t v) {
    if constexpr (M == 1) return band_dpp<0xB1>(v);                                              // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return band_dpp<0x4E>(v);                                         // quad_perm [2,3,0,1]
    else if constexpr (M == 4) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);     // bit mode: and 0x1f, or 0, xor 0x04
    else if constexpr (M == 8) return band_dpp<0x128>(v);                                        // row_ror:8 (l ^ 8 inside a row of 16)
    else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);                           // bit mode: xor 0x10
}
DI uint32_t band_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
DI uint32_t band_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// one compare-exchange step across lanes: partner lane l ^ M; up: this lane keeps the smaller key
template <int M>
DI void band_cx_lanes(uint32_t* a, bool up) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t o = band_xor<M>(a[s]);
        const uint32_t lo = band_min(a[s], o), hi = band_max(a[s], o);
        a[s] = up ? lo : hi;
    }
}
// one compare-exchange step inside a lane: register pairs (s, s ^ J), J = 1 or 2; asc: the lower register keeps the smaller key
template <int J>
DI void band_cx_regs(uint32_t* a, bool asc) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s & J) continue;
        const uint32_t lo = band_min(a[s], a[s ^ J]), hi = band_max(a[s], a[s ^ J]);
        a[s] = asc ? lo : hi;
        a[s ^ J] = asc ? hi : lo;
    }
}
// the steps j = K/2 .. 1 of merge level K (K = 8 .. 128) of the bitonic network over e = 4 l + s; the run of K elements that e lies in ascends where (e & K) == 0
template <int K>
DI void band_merge(uint32_t* a, int l) {
    // (the lane predicates of a level are formed here, from an opaque copy of l: hoisted out of the column loop, the 30-odd lane masks of the network would
    // each hold a scalar register pair for the whole kernel)
    asm volatile("" : "+v"(l));
    const bool asc = (l & (K >> 2)) == 0;                // (K = 128: l < 32, every run ascends)
    if constexpr (K >= 128) band_cx_lanes<16>(a, ((l & 16) == 0) == asc);
    if constexpr (K >= 64) band_cx_lanes<8>(a, ((l & 8) == 0) == asc);
    if constexpr (K >= 32) band_cx_lanes<4>(a, ((l & 4) == 0) == asc);
    if constexpr (K >= 16) band_cx_lanes<2>(a, ((l & 2) == 0) == asc);
    band_cx_lanes<1>(a, ((l & 1) == 0) == asc);
    band_cx_regs<2>(a, asc);
    band_cx_regs<1>(a, asc);
}
// 128 keys of a half (a[s] of lane l is element 4 l + s) into ascending order
DI void band_sort128(uint32_t* a, int l) {
    {   // level 2: pairs (0,1) ascend, (2,3) descend
        const uint32_t lo0 = band_min(a[0], a[1]), hi0 = band_max(a[0], a[1]), lo1 = band_min(a[2], a[3]), hi1 = band_max(a[2], a[3]);
        a[0] = lo0; a[1] = hi0; a[2] = hi1; a[3] = lo1;
    }
    {   // level 4: the lane's four ascend in even lanes, descend in odd ones
        asm volatile("" : "+v"(l));
        const bool asc = (l & 1) == 0;
        band_cx_regs<2>(a, asc);
        band_cx_regs<1>(a, asc);
    }
    band_merge<8>(a, l);
    band_merge<16>(a, l);
    band_merge<32>(a, l);
    band_merge<64>(a, l);
    band_merge<128>(a, l);
}

// popcount of this half's 32 bits of a ballot
DI uint32_t band_count(bool pred) {
    const unsigned long long m = __ballot(pred);
    return (uint32_t)__builtin_popcount((uint32_t)(threadIdx.x & 32u ? m >> 32 : m));
}

// The four columns of one half, G <= 4: sorted in registers. The next column's words are requested before this one's network runs. rank_l: ranks[l] in lane
// l < n_ranks of each half — lane k fetches the column's rank-k key itself and stores plane k's word, so one ds_bpermute per register and one store serve all
// requested ranks, and no rank sits in a scalar register across the network.
DI void band_columns_sort(const BandArgs& N, int P, int G, int b, int nq, int rank_l) {
    const int C = N.C, l = threadIdx.x & 31, half = threadIdx.x >> 5;
    const size_t gstride = (size_t)C * 32;
    const float* tb = N.traj + (size_t)b * G * gstride + l;
    const bool want_obs = N.obs != nullptr;
    float nx[4];                                         // (constant indices after unrolling: registers)
    {
        const int c = blockIdx.x * 32 + half;
#pragma unroll
        for (int s = 0; s < 4; ++s) nx[s] = c < C && s < G ? tb[(size_t)c * 32 + (size_t)s * gstride] : 0.0f;
    }
#pragma nounroll
    for (int j = 0; j < 4; ++j) {
        const int c = blockIdx.x * 32 + half + 8 * j;
        if (c >= C) break;                               // (uniform in the half; every cross-lane step below stays inside it)
        const size_t o = (size_t)b * C + c;
        uint32_t a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = s * 32 + l < P ? band_key(nx[s]) : 0xFFFFFFFFu;
        {
            const int cn = c + 8;
#pragma unroll
            for (int s = 0; s < 4; ++s) nx[s] = j < 3 && cn < C && s < G ? tb[(size_t)cn * 32 + (size_t)s * gstride] : 0.0f;
        }
        if (want_obs) {                                  // (wave-uniform)
            const uint32_t ko = band_key(N.obs[o]);
            uint32_t below = 0u, at = 0u;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool valid = s * 32 + l < P;
                below += band_count(valid && a[s] < ko);
                at += band_count(valid && a[s] == ko);
            }
            if (l == 0) {
                if (N.below) N.below[o] = below;
                if (N.at) N.at[o] = at;
            }
        }
        if (nq) {                                        // (wave-uniform)
            band_sort128(a, l);
            // rank r is register r & 3 of lane r >> 2
            const int src = (int)((threadIdx.x & 32u) + (unsigned)(rank_l >> 2)) * 4;
            const uint32_t x0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[0]), x1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[1]);
            const uint32_t x2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[2]), x3 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)a[3]);
            const int rs = rank_l & 3;
            const uint32_t x = rs == 0 ? x0 : rs == 1 ? x1 : rs == 2 ? x2 : x3;
            if (l < nq) N.q[((size_t)b * nq + l) * C + c] = __uint_as_float(band_word(x));
        }
    }
}

// The four columns of one half, any G: selected bit by bit over the column's lines; nothing is kept. Lane k of the half stores plane k's word.
DI void band_columns_select(const BandArgs& N, int P, int G, int b, int nq) {
    const int C = N.C, l = threadIdx.x & 31, half = threadIdx.x >> 5;
    const size_t gstride = (size_t)C * 32;
    const float* tb = N.traj + (size_t)b * G * gstride + l;
    const bool want_obs = N.obs != nullptr;
#pragma nounroll
    for (int j = 0; j < 4; ++j) {
        const int c = blockIdx.x * 32 + half + 8 * j;
        if (c >= C) break;                               // (uniform in the half)
        const size_t o = (size_t)b * C + c;
        const float* col = tb + (size_t)c * 32;
        if (want_obs) {                                  // (wave-uniform)
            const uint32_t ko = band_key(N.obs[o]);
            uint32_t below = 0u, at = 0u;
            for (int g = 0; g < G; ++g) {
                const bool valid = g * 32 + l < P;
                const uint32_t key = band_key(col[(size_t)g * gstride]);
                below += band_count(valid && key < ko);
                at += band_count(valid && key == ko);
            }
            if (l == 0) {
                if (N.below) N.below[o] = below;
                if (N.at) N.at[o] = at;
            }
        }
        if (nq) {                                        // (wave-uniform)
            uint32_t sel[BAND_MAX_RANKS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};     // (constant indices after unrolling: registers)
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t m = 1u << bit;
                uint32_t cnt[BAND_MAX_RANKS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                for (int g = 0; g < G; ++g) {
                    const bool valid = g * 32 + l < P;
                    const uint32_t key = band_key(col[(size_t)g * gstride]);
#pragma unroll
                    for (int k = 0; k < BAND_MAX_RANKS; ++k)
                        if (k < nq) cnt[k] += band_count(valid && key < (sel[k] | m));
                }
#pragma unroll
                for (int k = 0; k < BAND_MAX_RANKS; ++k)     // (constant indices into the argument: no copy of it in scratch)
                    if (k < nq && cnt[k] <= (uint32_t)N.ranks[k]) sel[k] |= m;
            }
            uint32_t x = sel[0];
#pragma unroll
            for (int k = 1; k < BAND_MAX_RANKS; ++k) x = l == k ? sel[k] : x;
            if (l < nq) N.q[((size_t)b * nq + l) * C + c] = __uint_as_float(band_word(x));
        }
    }
}

// the bands mode of sdempc_noise_kernel: blockIdx.x = column tile, b = instance. P, G as in the noise mode.
DI void band_reduce(const BandArgs& N, int P, int G, int b) {
    const int nq = N.q ? N.n_ranks : 0;
    if (G <= 4) {                                        // (wave-uniform)
        const int l = threadIdx.x & 31;
        int rank_l = 0;
#pragma unroll
        for (int k = 0; k < BAND_MAX_RANKS; ++k) rank_l = l == k ? N.ranks[k] : rank_l;  // (constant indices into the argument: no copy of it in scratch)
        band_columns_sort(N, P, G, b, nq, rank_l);
    } else band_columns_select(N, P, G, b, nq);
}

}  // namespace sdempc
