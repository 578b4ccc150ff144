// sdempc_risk.inc.h — predicted risk (SPEC.md §12a): per particle the first step at which it leaves a per-instance box around a per-step centre row and its
// tracking cost Jx_p; per instance the first-exit histogram, the per-step count of particles outside, mean / variance / extrema of Jx, order statistics of Jx
// and the mean of its tail_k worst values. Reduced from the particle x horizon tensor a store_traj rollout left in the handle, where it lies. Included by
// sdempc_prng.hip after sdempc_tube.inc.h (whose half-wave butterflies it uses): the reducer runs as one more mode of sdempc_noise_kernel, selected by
// RiskArgs::traj.
//
// Path replaced (reference): none on the device — the reference returns the particle mean and the expected cost only (sde_control.py:698,717); every
// trajectory-level statistic was a host reduction over rollout(want_traj=True), i.e. a relayout and a copy of the whole tensor.
//
// Mapping: HBM-read-bound; one workgroup of 256 threads per instance, eight 32-lane halves. Half h takes the particle groups g = h, h + 8, ... with the
// particle in the lane and walks t = 0 .. H in order: 13 loads of one 128-byte line each per step, addresses independent of the data, issued together; the
// other waves of the CU cover their latency (holding the next step's row in registers as well cost the hosting kernel two waves per SIMD of occupancy for
// every mode, so it is not done). xref / centre / disc / the cost weights are uniform per instance (scalar loads); the box lies in LDS. Per step: the outside flag, one
// ballot + popcount into an LDS counter per step (outside_any), the running first exit, and J = fma(disc[t-1], l_x(x_t, xref_t), J). After the sweep:
// the exit histogram by LDS atomics, Jx into LDS, the §6.1 group totals / extrema into LDS. Then every thread folds the group totals in ascending g into
// slot g mod 4 (mean), the halves form the variance terms and — where order statistics are asked for — every particle counts the particles in front of it
// in the total order over the LDS copy of Jx (P compares per particle, broadcast reads), which gives its rank; the tail values stay in their own lanes for
// the §6.1 sum. Padded lanes are masked everywhere. Dynamic LDS only (sized by the launcher): the noise and tube modes allocate none.
#pragma once

namespace sdempc {

// SPEC.md §5.3 restated (the arithmetic of stage_cost<false, true> in sdempc_step.inc.h, which hangs on KArgs and the rollout's includes; tests pin the two
// to each other through the anchor: the particle mean of Jx is the rollout's cost bit for bit where the cost has no other term). x: the particle's state,
// xr: the reference row (uniform).
DI float risk_stage_cost(const RiskArgs& R, const float* x, const float* xr) {
    float l = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float e = x[i] - xr[i]; const float w = R.perr[i] * e; l = FMA(w, e, l); }
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float e = x[3 + i] - xr[3 + i]; const float w = R.verr[i] * e; l = FMA(w, e, l); }
#pragma unroll
    for (int i = 0; i < 3; ++i) { const float e = x[10 + i] - xr[10 + i]; const float w = R.werr[i] * e; l = FMA(w, e, l); }
    const float qw = x[6], qx = x[7], qy = x[8], qz = x[9], rw = xr[6], rx = xr[7], ry = xr[8], rz = xr[9];
    const float ex = FMA(rz, qy, FMA(-ry, qz, FMA(-rx, qw, rw * qx)));
    const float ey = FMA(-rz, qx, FMA(-ry, qw, FMA(rx, qz, rw * qy)));
    const float ez = FMA(-rz, qw, FMA(ry, qx, FMA(-rx, qy, rw * qz)));
    const float wxe = R.qerr[0] * ex, wye = R.qerr[1] * ey, wze = R.qerr[2] * ez;
    l = FMA(wxe, ex, l); l = FMA(wye, ey, l); l = FMA(wze, ez, l);
    if (__builtin_expect(R.sc_n != 0, 0)) {              // state_constr, penalty form: ascending state index, a rolled loop on the cold path
#pragma nounroll
        for (int k = 0; k < R.sc_n; ++k) {
            const int i = R.sc_tab[k].id;
            const float w = R.sc_tab[k].w;
            float xi = x[0];
#pragma unroll
            for (int jx = 1; jx < 13; ++jx) xi = (i == jx) ? x[jx] : xi;
            float hi = xi - R.sc_tab[k].hi; hi = hi < 0.0f ? 0.0f : hi;
            float lo = R.sc_tab[k].lo - xi; lo = lo < 0.0f ? 0.0f : lo;
            l = FMA(w * hi, hi, l);
            l = FMA(w * lo, lo, l);
        }
    }
    return l;
}

// group totals [G] in LDS -> the §6.1 total: slot g mod 4 in ascending g, ((S0 + S1) + S2) + S3 (every thread, broadcast reads)
DI float risk_slots(const float* T, int G) {
    float S[4] = {0.0f, 0.0f, 0.0f, 0.0f};               // (constant indices after unrolling: registers)
    for (int g0 = 0; g0 < G; g0 += 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (g0 + s < G) S[s] = S[s] + T[g0 + s];
    }
    return ((S[0] + S[1]) + S[2]) + S[3];
}

// dynamic LDS of one workgroup (risk_lds_words_host, sdempc_kernels.h): any[H+1] hist[H+2] jx[G*32] gsum[G] gmin[G] gmax[G] gvar[G] gtail[G] box[26]
// the risk mode of sdempc_noise_kernel: one workgroup per instance b. P, G as in the noise mode.
DI void risk_reduce(const RiskArgs& R, int P, int G, int b) {
    extern __shared__ uint32_t risk_lds[];
    const int H = R.H, C = (H + 1) * 13;
    const int tid = threadIdx.x, l = tid & 31, half = tid >> 5;
    uint32_t* s_any = risk_lds;                          // [H+1]
    uint32_t* s_hist = s_any + (H + 1);                  // [H+2]
    float* s_jx = (float*)(s_hist + (H + 2));            // [G*32]
    float* s_gsum = s_jx + (size_t)G * 32;               // [G] each
    float* s_gmin = s_gsum + G;
    float* s_gmax = s_gmin + G;
    float* s_gvar = s_gmax + G;
    float* s_gtail = s_gvar + G;
    float* s_box = s_gtail + G;                          // lo[13] hi[13] of the instance (broadcast reads: the sweep keeps its registers for the rows in flight)
    const bool want_x = R.lo != nullptr;                 // exit, first_exit, outside_any (wave-uniform)
    const bool want_j = R.jx || R.jstat || R.jq || R.jtail;
    for (int i = tid; i < 2 * H + 3; i += 256) s_any[i] = 0u;

    const float* xrb = R.xref ? R.xref + (size_t)b * C : nullptr;
    const float* cb = R.centre ? R.centre + (size_t)b * C : nullptr;
    if (want_x && tid < 26) s_box[tid] = tid < 13 ? R.lo[(size_t)b * 13 + tid] : R.hi[(size_t)b * 13 + tid - 13];
    __syncthreads();
    const size_t gstride = (size_t)C * 32;
    for (int g = half; g < G; g += 8) {                  // (uniform in the half; every cross-lane step below stays inside it)
        const int p = g * 32 + l;
        const bool valid = p < P;
        const float* tp = R.traj + ((size_t)b * G + g) * gstride + l;
        uint32_t ex = (uint32_t)(H + 1);
        float J = 0.0f;
        for (int t = 0; t <= H; ++t) {
            float xa[13];
#pragma unroll
            for (int i = 0; i < 13; ++i) xa[i] = tp[(size_t)(t * 13 + i) * 32];
            if (want_x) {
                bool out = false;
#pragma unroll
                for (int i = 0; i < 13; ++i) {
                    const float e = cb ? xa[i] - cb[t * 13 + i] : xa[i];
                    out = out | !((e >= s_box[i]) & (e <= s_box[13 + i]));     // (no short circuit: thirteen nested branches otherwise)
                }
                out = out & valid;
                const unsigned long long m = __ballot(out);
                const uint32_t n = (uint32_t)__builtin_popcount((uint32_t)(tid & 32 ? m >> 32 : m));
                if (l == 0 && n) atomicAdd(&s_any[t], n);
                if (out && ex == (uint32_t)(H + 1)) ex = (uint32_t)t;
            }
            if (want_j && t >= 1) J = FMA(R.disc[t - 1], risk_stage_cost(R, xa, xrb + t * 13), J);
        }
        if (want_x && valid) {
            atomicAdd(&s_hist[ex], 1u);
            if (R.exit) R.exit[(size_t)b * P + p] = ex;
        }
        if (want_j) {
            if (valid && R.jx) R.jx[(size_t)b * P + p] = J;
            s_jx[p] = valid ? J : 0.0f;
            const float tot = tube_sum32(valid ? J : 0.0f);
            const float mn = tube_min32(valid ? J : __builtin_inff());
            const float mx = tube_max32(valid ? J : -__builtin_inff());
            if (l == 0) { s_gsum[g] = tot; s_gmin[g] = mn; s_gmax[g] = mx; }
        }
    }
    __syncthreads();

    if (want_x) {
        if (R.outside_any)
            for (int t = tid; t <= H; t += 256) R.outside_any[(size_t)b * (H + 1) + t] = s_any[t];
        if (R.first_exit)
            for (int t = tid; t <= H + 1; t += 256) R.first_exit[(size_t)b * (H + 2) + t] = s_hist[t];
    }
    if (!R.jstat && !R.jq && !R.jtail) return;           // (wave-uniform)

    const float mean = risk_slots(s_gsum, G) * R.invP;
    const bool want_rank = R.jq || R.jtail;
    for (int g = half; g < G; g += 8) {
        const int p = g * 32 + l;
        const bool valid = p < P;
        const float a = s_jx[p];
        if (R.jstat) {
            const float d = a - mean;
            const float q = tube_sum32(valid ? d * d : 0.0f);
            if (l == 0) s_gvar[g] = q;
        }
        if (want_rank) {
            // rank of p in the total order: numbers by < / ==, a NaN above every number, all NaNs equal, ties by particle index
            const bool an = a != a;
            int rank = 0;
            for (int q = 0; q < P; ++q) {
                const float c = s_jx[q];
                const bool cn = c != c;
                const bool less = c < a || (an && !cn);
                const bool same = c == a || (an && cn);
                rank += (less || (same && q < p)) ? 1 : 0;
            }
            if (R.jq && valid) {
#pragma unroll
                for (int k = 0; k < 8; ++k)                  // (constant indices into the argument: no copy of it in scratch)
                    if (k < R.n_ranks && rank == R.ranks[k]) R.jq[(size_t)b * R.n_ranks + k] = a;
            }
            if (R.jtail) {
                const float v = tube_sum32(valid && rank >= P - R.tail_k ? a : 0.0f);
                if (l == 0) s_gtail[g] = v;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (R.jstat) {
            float mn = __builtin_inff(), mx = -__builtin_inff();
            for (int g = 0; g < G; ++g) { mn = __builtin_fminf(mn, s_gmin[g]); mx = __builtin_fmaxf(mx, s_gmax[g]); }
            float* o = R.jstat + (size_t)b * 4;
            o[0] = mean;
            o[1] = risk_slots(s_gvar, G) * R.invP;
            o[2] = mn;
            o[3] = mx;
        }
        if (R.jtail) R.jtail[b] = risk_slots(s_gtail, G) * R.inv_tail;
    }
}

}  // namespace sdempc
