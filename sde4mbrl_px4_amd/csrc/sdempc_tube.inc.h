// sdempc_tube.inc.h — the predicted tube (SPEC.md §12): per-step particle mean, variance, extrema and bound exceedance of the particle x horizon
// tensor a store_traj rollout left in the handle, reduced where it lies. Included by sdempc_prng.hip: the reducer runs as a mode of
// sdempc_noise_kernel (the kernel that owns the particle-minor [..][32] layouts at 256 threads), selected by TubeArgs::traj.
//
// Path replaced (reference): none on the device — the reference returns the particle mean only (xevol, sde_control.py:698,717); the spread was a
// host reduction over rollout(want_traj=True), i.e. a relayout and a copy of the whole tensor.
//
// Mapping: HBM-read-bound, no LDS, no matrix pipe. The tensor is f32[B][G][C][32] (C = (H+1)*13): every (b, g, c) row is one 128-byte line with the
// particle in the lane. A workgroup takes one instance and one tile of 32 columns; each of its eight 32-lane halves takes the four columns
// c = tile*32 + half + 8 j, so the two halves of a wave64 read neighbouring lines (256 contiguous bytes per load). Per column the half loops
// over the groups g: load, mask the padded lanes, xor butterfly 16, 8, 4, 2, 1 inside the half (ds_swizzle bit mode for 16 — it stays inside 32
// lanes — and DPP row rotations / quad permutations below, which are the xor partners once a row is periodic), slot g mod 4. The variance needs the
// rounded mean first, so it is a second loop over the same lines (they come from the cache: 16 KB per workgroup at G = 4). Lane j of a half then
// stores column j's results: one store instruction per plane.
#pragma once

namespace sdempc {

template <int CTRL>
DI float tube_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// value of lane l ^ 16: ds_swizzle bit mode, and_mask 0x1f, or_mask 0, xor_mask 0x10 (the pattern acts inside groups of 32 lanes)
DI float tube_xor16(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)); }

// SPEC.md §6.1 butterfly of one 32-lane group: the total in every lane
DI float tube_sum32(float v) {
    v = v + tube_xor16(v);
    v = v + tube_dpp<0x128>(v);   // row_ror:8
    v = v + tube_dpp<0x124>(v);   // row_ror:4 (rows are 8-periodic now)
    v = v + tube_dpp<0x4E>(v);    // quad_perm [2,3,0,1]
    v = v + tube_dpp<0xB1>(v);    // quad_perm [1,0,3,2]
    return v;
}
DI float tube_min32(float v) {
    v = __builtin_fminf(v, tube_xor16(v));
    v = __builtin_fminf(v, tube_dpp<0x128>(v));
    v = __builtin_fminf(v, tube_dpp<0x124>(v));
    v = __builtin_fminf(v, tube_dpp<0x4E>(v));
    v = __builtin_fminf(v, tube_dpp<0xB1>(v));
    return v;
}
DI float tube_max32(float v) {
    v = __builtin_fmaxf(v, tube_xor16(v));
    v = __builtin_fmaxf(v, tube_dpp<0x128>(v));
    v = __builtin_fmaxf(v, tube_dpp<0x124>(v));
    v = __builtin_fmaxf(v, tube_dpp<0x4E>(v));
    v = __builtin_fmaxf(v, tube_dpp<0xB1>(v));
    return v;
}

// one pass over the groups of a column: the §6.1 sum of f(v_p) over the valid particles, f = identity (SQ false) or (v_p - mean)^2 (SQ true: one subtraction
// from the rounded mean, one rounded product). EXT: extrema and the exceedance count beside it. load(g, s) is lane l's word of group g = 4 k + s.
template <bool SQ, bool EXT, class Load>
DI float tube_pass(Load load, int P, int G, int l, float mean, float lo, float hi, bool want_out, float& mn, float& mx, uint32_t& cnt) {
    float S[4] = {0.0f, 0.0f, 0.0f, 0.0f};               // (constant indices after unrolling: registers)
    for (int g0 = 0; g0 < G; g0 += 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int g = g0 + s;
            if (g < G) {                                 // (wave-uniform)
                const bool valid = g * 32 + l < P;
                const float v = load(g, s);
                float e = v;
                if constexpr (SQ) { const float d = v - mean; e = d * d; }
                S[s] = S[s] + tube_sum32(valid ? e : 0.0f);
                if constexpr (EXT) {
                    mn = __builtin_fminf(mn, tube_min32(valid ? v : __builtin_inff()));
                    mx = __builtin_fmaxf(mx, tube_max32(valid ? v : -__builtin_inff()));
                    if (want_out) {                      // (wave-uniform)
                        const unsigned long long m = __ballot(valid && !(v >= lo && v <= hi));
                        cnt += (uint32_t)__builtin_popcount((uint32_t)(threadIdx.x & 32u ? m >> 32 : m));
                    }
                }
            }
        }
    }
    return ((S[0] + S[1]) + S[2]) + S[3];
}

// The four columns of one half. KEEP (G <= 4, the shipped configurations up to P = 128): all 16 words of the half's lane are loaded up front — 16 loads in flight per
// lane — and both passes run from registers, so the tensor is read once. Otherwise both passes load, group by group.
template <bool KEEP>
DI void tube_columns(const TubeArgs& T, int P, int G, int b, float lo_l, float hi_l) {
    const int C = T.C, l = threadIdx.x & 31, half = threadIdx.x >> 5;
    const size_t gstride = (size_t)C * 32;
    const float* tb = T.traj + (size_t)b * G * gstride + l;
    const bool want_out = T.outside != nullptr;
    float vc[4][4];                                      // (constant indices after unrolling: registers; KEEP only)
    if constexpr (KEEP) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = blockIdx.x * 32 + half + 8 * j;
#pragma unroll
            for (int s = 0; s < 4; ++s) vc[j][s] = c < C && s < G ? tb[(size_t)c * 32 + (size_t)s * gstride] : 0.0f;
        }
    }
    float r_mean = 0.0f, r_var = 0.0f, r_min = 0.0f, r_max = 0.0f;
    uint32_t r_cnt = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = blockIdx.x * 32 + half + 8 * j;
        if (c >= C) continue;                            // (uniform in the half; every cross-lane step below stays inside it)
        const float* col = tb + (size_t)c * 32;
        auto load = [&](int g, int s) {
            if constexpr (KEEP) return vc[j][s];
            else return col[(size_t)g * gstride];
        };
        float lo = 0.0f, hi = 0.0f;
        if (want_out) {
            const int src = (int)((threadIdx.x & 32u) + (unsigned)(c % 13)) * 4;
            lo = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, lo_l)));
            hi = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, hi_l)));
        }
        float mn = __builtin_inff(), mx = -__builtin_inff(), dummy0 = 0.0f, dummy1 = 0.0f;
        uint32_t cnt = 0u, dummy2 = 0u;
        const float mean = tube_pass<false, true>(load, P, G, l, 0.0f, lo, hi, want_out, mn, mx, cnt) * T.invP;
        float var = 0.0f;
        if (T.var) var = tube_pass<true, false>(load, P, G, l, mean, 0.0f, 0.0f, false, dummy0, dummy1, dummy2) * T.invP;   // (wave-uniform)
        if (l == j) { r_mean = mean; r_var = var; r_min = mn; r_max = mx; r_cnt = cnt; }
    }
    const int c = blockIdx.x * 32 + half + 8 * l;
    if (l < 4 && c < C) {
        const size_t o = (size_t)b * C + c;
        if (T.mean) T.mean[o] = r_mean;
        if (T.var) T.var[o] = r_var;
        if (T.mn) T.mn[o] = r_min;
        if (T.mx) T.mx[o] = r_max;
        if (want_out) T.outside[o] = r_cnt;
    }
}

// the tube mode of sdempc_noise_kernel: blockIdx.x = column tile, b = instance. P, G as in the noise mode.
DI void tube_reduce(const TubeArgs& T, int P, int G, int b) {
    const int l = threadIdx.x & 31;
    // bounds of component i in lane i of each half (constant indices into the argument: no copy of it in scratch); a column fetches its pair by ds_bpermute
    float lo_l = 0.0f, hi_l = 0.0f;
    if (T.outside) {
#pragma unroll
        for (int i = 0; i < 13; ++i) { lo_l = l == i ? T.lo[i] : lo_l; hi_l = l == i ? T.hi[i] : hi_l; }
    }
    if (G <= 4) tube_columns<true>(T, P, G, b, lo_l, hi_l);          // (wave-uniform)
    else tube_columns<false>(T, P, G, b, lo_l, hi_l);
}

}  // namespace sdempc
