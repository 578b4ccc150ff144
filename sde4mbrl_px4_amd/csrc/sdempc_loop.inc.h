// sdempc_loop.inc.h — the plant of the batched closed loop (SPEC.md §11): one Euler–Maruyama step of the handle's own model per episode and
// tick, plus the hand-over to the next tick's solve (applied control, shifted warm start, step size); §11a: a separate plant; §11b: a whole solve period; §11c: a period with a scenario; §11d: a period flown through the rate-setpoint interface.
// Fragment of sdempc_kernels.hip, translation unit SDEMPC_TU = 4: included inside namespace sdempc::{exact|fastm} (compiled once per math mode).
//
// The step is the rollout's own device code: step_fwd at t = 0 on a control table built by block_prepass, i.e. the arithmetic of step 0
// of every rollout (Oracle.step(x, u, xi, t=0)), in every mlp_dtype and math mode. One wave per episode, four episodes per workgroup
// (TeamWave): all 32 particle columns of the tile carry the same state and noise, and lane 0's copy is the result. The kernel gets the
// handle's argument block with H = 1 (a one-step horizon: the staged tables and the control table hold step 0 only); L.H is the solve's horizon.
// Arguments: LoopAdvance (sdempc_kernels.h).
template <int F16>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_advance_kernel(KArgs a, LoopAdvance L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = L.H, m = a.m;
    const int tid = TeamWave::tid();
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    Smem sm = carve(smem, 1, m, TeamWave::team());
    WaveW ww;
    load_weights(a, sm, ww, threadIdx.x, TeamWave::BNT);
    __syncthreads();
    if (b >= L.B) return;           // (wave-uniform; no workgroup-wide barrier below)
    const int lane = tid & 63, h = lane >> 5;
    const float* uo = L.uopt + (size_t)b * H * m;
    block_prepass<TeamWave>(a, sm, uo, tid);          // control table row 0 from uopt_k[0]
    float x[NX], xn[NX], xi[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
#pragma unroll
    for (int i = 0; i < NN; ++i) xi[i] = L.xi[(size_t)b * NN + i];
    TeamWave::sync();
    StepAux A;
    step_fwd<F16, false>(a, sm, ww, 0, h, lane, x, xi, xn, A);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) { L.x[(size_t)b * NX + i] = xn[i]; L.xs[(size_t)b * NX + i] = xn[i]; }
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (lane < m) L.us[(size_t)b * m + lane] = uo[lane];
    float* un = L.u + (size_t)b * H * m;
    for (int e = tid; e < H * m; e += TeamWave::NT) {   // y_{k+1} = [uopt_k[1:], uopt_k[H-1]]
        const int t = e / m;
        un[e] = uo[(t + 1 < H ? t + 1 : t) * m + (e - t * m)];
    }
}

// SPEC.md §11a: the same hand-over behind a SEPARATE plant — episode b is stepped by the model Q names for it, Q.substeps times at the plant's own step
// length and in the plant's own arithmetic (this kernel's namespace and F16 are the plant's, independent of the solve's), the applied control held.
// The argument block arrives as for the kernel above (H = 1; dt -> the plant's step length) and the wave works on a copy `a`: with per-episode plants (Q.models) the wave
// replaces a.M, a.wts and a.sdt by its plant's, read through a readfirstlane'd index (wave-uniform addresses, before the kernel's first store: scalar
// loads, so the model constants stay in SGPRs as the kernel arguments they replace do), and stages its OWN LDS images — the workgroup's LDS holds four
// carves of one team each instead of one carve of four teams (16 KB per episode, 64 KB per workgroup: two workgroups per CU). With one shared plant the
// four episodes share one carve, as above. block_prepass indexes the rotor tables of a.M by a run-time motor index, which a kernel argument serves by a
// scalar load at a computed offset but a modified copy could only serve from scratch: the per-episode path hands it the wave's argument block in LDS
// (plant_kargs_floats() floats per wave behind the carves) and keeps the register copy for step_fwd, whose indices are all static.
// The prepass runs once per tick (control table row 0 from uopt_k[0] with the plant's polynomials and W1u); every substep is step_fwd at t = 0, xn fed back.
__host__ __device__ constexpr int plant_kargs_floats() { return (int)((sizeof(KArgs) + 15) / 16 * 4); }
template <int F16>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_plant_kernel(KArgs a0, LoopAdvance L, LoopPlant Q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    KArgs a = a0;                   // (a0 stays the untouched kernel argument: the shared-plant prepass indexes it at run time)
    const int H = L.H, m = a.m;
    const int tid = TeamWave::tid();
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    const bool per = Q.models != nullptr, live = b < L.B;      // (both wave-uniform)
    if (per && live) {
        const int p = __builtin_amdgcn_readfirstlane(Q.plant_of ? Q.plant_of[b] : b);
        a.M = Q.models[p];
        a.wts = Q.wts + (size_t)p * Q.wts_stride;
        a.sdt = Q.sdt + (size_t)p * NN;
    }
    Smem sm = per ? carve(smem + (size_t)TeamWave::team() * smem_floats(1, m, 1), 1, m, 0) : carve(smem, 1, m, TeamWave::team());
    WaveW ww;
    load_weights(a, sm, ww, per ? tid : (int)threadIdx.x, per ? TeamWave::NT : TeamWave::BNT);
    KArgs* const lk = reinterpret_cast<KArgs*>(smem + TeamWave::IPB * smem_floats(1, m, 1) + (size_t)TeamWave::team() * plant_kargs_floats());
    if (per && tid == 0) { lk->H = 1; lk->m = m; lk->M = a.M; }        // (what block_prepass reads)
    __syncthreads();
    if (!live) return;              // (wave-uniform; no workgroup-wide barrier below)
    const int lane = tid & 63, h = lane >> 5;
    const float* uo = L.uopt + (size_t)b * H * m;
    if (per) block_prepass<TeamWave>(*lk, sm, uo, tid);
    else block_prepass<TeamWave>(a0, sm, uo, tid);
    float x[NX], xn[NX], xi[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
    TeamWave::sync();
    const float* xrow = L.xi + (size_t)b * Q.substeps * NN;
#pragma nounroll
    for (int j = 0; j < Q.substeps; ++j) {
#pragma unroll
        for (int i = 0; i < NN; ++i) xi[i] = xrow[j * NN + i];
        StepAux A;
        step_fwd<F16, false>(a, sm, ww, 0, h, lane, x, xi, xn, A);
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = xn[i];
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) { L.x[(size_t)b * NX + i] = x[i]; L.xs[(size_t)b * NX + i] = x[i]; }
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (lane < m) L.us[(size_t)b * m + lane] = uo[lane];
    float* un = L.u + (size_t)b * H * m;
    for (int e = tid; e < H * m; e += TeamWave::NT) {   // y_{k+1} = [uopt_k[1:], uopt_k[H-1]]
        const int t = e / m;
        un[e] = uo[(t + 1 < H ? t + 1 : t) * m + (e - t * m)];
    }
}

hipError_t launch_loop_plant(const KArgs& a, const LoopAdvance& L, const LoopPlant& Q, hipStream_t st) {
    if (L.B < 1 || L.H != a.H || Q.substeps < 1 || (Q.models && (!Q.wts || !Q.sdt || Q.wts_stride < BLOB_FLOATS + VJP_BASE))) return hipErrorInvalidValue;
    KArgs k = a;
    k.H = 1;
    const size_t sb = Q.models ? TeamWave::IPB * (smem_bytes(1, k.m, 1) + sizeof(float) * plant_kargs_floats()) : smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    return with_f16(k.f16, [&](auto F16) {
        if (sb > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)sdempc_loop_plant_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb);
            if (e != hipSuccess) return e;
        }
        sdempc_loop_plant_kernel<F16><<<grid, TeamWave::BNT, sb, st>>>(k, L, Q);
        return hipGetLastError();
    });
}

// SPEC.md §11b: a whole solve period behind the same plant set — R.ticks control ticks of Q.substeps Euler–Maruyama steps each in ONE launch, so that a loop
// whose ticks are millisecond-scale solves does not pay a launch per plant step. The prologue is the kernel's above (shared or per-episode LDS carves, the
// wave's argument block in LDS for the per-episode prepass). Substep q = i * substeps + jj of the period flies row min(i, H - 1) of the previous solution's
// tail (L.u: the warm start y_j) while q < R.arrive and of this period's solution (L.uopt) from then on; the arrival point is the same for every episode,
// so the choice is wave-uniform. Lane l < m carries motor l's state: a_l <- fma(alpha, c_l - a_l, a_l) before every substep, or a_l = c_l with the lag off.
// The applied control row lives in the team's sm.v[5] (an optimiser vector the step does not use) and block_prepass reruns whenever it can have changed:
// every substep with the lag on, at tick starts and at the arrival substep otherwise (rerunning it on an unchanged row writes the same table).
// Every read of the warm start precedes its rewrite: the commands are read inside the substep loop, the shifted rows are written after it, by the same wave.
template <int F16>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_period_kernel(KArgs a0, LoopAdvance L, LoopPlant Q, LoopPeriod R) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    KArgs a = a0;
    const int H = L.H, m = a.m;
    const int tid = TeamWave::tid();
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    const bool per = Q.models != nullptr, live = b < L.B;      // (both wave-uniform)
    if (per && live) {
        const int p = __builtin_amdgcn_readfirstlane(Q.plant_of ? Q.plant_of[b] : b);
        a.M = Q.models[p];
        a.wts = Q.wts + (size_t)p * Q.wts_stride;
        a.sdt = Q.sdt + (size_t)p * NN;
    }
    Smem sm = per ? carve(smem + (size_t)TeamWave::team() * smem_floats(1, m, 1), 1, m, 0) : carve(smem, 1, m, TeamWave::team());
    WaveW ww;
    load_weights(a, sm, ww, per ? tid : (int)threadIdx.x, per ? TeamWave::NT : TeamWave::BNT);
    KArgs* const lk = reinterpret_cast<KArgs*>(smem + TeamWave::IPB * smem_floats(1, m, 1) + (size_t)TeamWave::team() * plant_kargs_floats());
    if (per && tid == 0) { lk->H = 1; lk->m = m; lk->M = a.M; }        // (what block_prepass reads)
    __syncthreads();
    if (!live) return;              // (wave-uniform; no workgroup-wide barrier below)
    const int lane = tid & 63, h = lane >> 5, n = Q.substeps;
    const bool lag = R.alpha > 0.0f, mine = lane < m;
    const float* uo = L.uopt + (size_t)b * H * m;
    float* yw = L.u + (size_t)b * H * m;
    float* act = sm.v[5];           // [m] the applied control of the current substep
    float am = mine ? R.act[(size_t)b * m + lane] : 0.0f;
    float x[NX], xn[NX], xi[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
    const float* xrow = L.xi + (size_t)b * R.xi_ticks * n * NN;
#pragma nounroll
    for (int i = 0; i < R.ticks; ++i) {
        const int row = (i < H - 1 ? i : H - 1) * m;
#pragma nounroll
        for (int jj = 0; jj < n; ++jj) {
            const int q = i * n + jj;
            if (lag || jj == 0 || q == R.arrive) {
                if (mine) {
                    const float c = (q >= R.arrive ? uo : yw)[row + lane];
                    am = lag ? FMA(R.alpha, c - am, am) : c;
                    act[lane] = am;
                }
                TeamWave::sync();       // (the row is written, the previous substep's reads of the control table are done)
                if (per) block_prepass<TeamWave>(*lk, sm, act, tid);
                else block_prepass<TeamWave>(a0, sm, act, tid);
                TeamWave::sync();
            }
            if (jj == 0 && mine) L.us[((size_t)i * L.B + b) * m + lane] = am;
#pragma unroll
            for (int e = 0; e < NN; ++e) xi[e] = xrow[q * NN + e];
            StepAux A;
            step_fwd<F16, false>(a, sm, ww, 0, h, lane, x, xi, xn, A);
#pragma unroll
            for (int e = 0; e < NX; ++e) x[e] = xn[e];
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < NX; ++e) L.xs[((size_t)i * L.B + b) * NX + e] = x[e];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) L.x[(size_t)b * NX + i] = x[i];
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (mine) R.act[(size_t)b * m + lane] = am;
    for (int e = tid; e < H * m; e += TeamWave::NT) {   // y_{j+1}: row t = uopt_j[min(t + S, H - 1)]
        const int t = e / m, ts = t + R.shift < H ? t + R.shift : H - 1;
        yw[e] = uo[ts * m + (e - t * m)];
    }
}

hipError_t launch_loop_period(const KArgs& a, const LoopAdvance& L, const LoopPlant& Q, const LoopPeriod& R, hipStream_t st) {
    if (L.B < 1 || L.H != a.H || Q.substeps < 1 || (Q.models && (!Q.wts || !Q.sdt || Q.wts_stride < BLOB_FLOATS + VJP_BASE))) return hipErrorInvalidValue;
    if (!R.act || R.ticks < 1 || R.xi_ticks < R.ticks || R.shift < 1 || R.shift > a.H || R.arrive < 0 || !(R.alpha >= 0.0f && R.alpha <= 1.0f)) return hipErrorInvalidValue;
    KArgs k = a;
    k.H = 1;
    const size_t sb = Q.models ? TeamWave::IPB * (smem_bytes(1, k.m, 1) + sizeof(float) * plant_kargs_floats()) : smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    return with_f16(k.f16, [&](auto F16) {
        if (sb > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)sdempc_loop_period_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb);
            if (e != hipSuccess) return e;
        }
        sdempc_loop_period_kernel<F16><<<grid, TeamWave::BNT, sb, st>>>(k, L, Q, R);
        return hipGetLastError();
    });
}

// SPEC.md §11c: the period kernel with a SCENARIO — per control tick an external acceleration on the state (a disturbance row, held over the tick's substeps)
// and the plant that flies the tick (a plant index per tick and episode). Body, hand-over and every argument of sdempc_loop_period_kernel; what differs:
//  * the disturbance row of tick i is six floats at a wave-uniform address; after every step_fwd the register copy of x takes v_e <- fma(w_v[e], dtp, v_e)
//    and omega_e <- fma(w_om[e], dtp, omega_e), dtp the plant's step length — six fmas, applied whenever a schedule is given (zero rows included);
//  * the ticks of the period are walked in RUNS of ticks that name one plant. A run starts by staging that plant into the wave's own LDS carve (load_weights,
//    WaveW, the wave's argument block for the prepass; TeamWave::sync on both sides), so inside a run the model constants are what they are in the period kernel:
//    values defined before the tick loop, not loop-carried ones. The first run's staging is the period kernel's prologue. The state x, the motor state, the
//    applied-control row and the noise rows carry over a switch untouched; sigma sqrt(dt) travels with the weights (sm.sdt), the rotor tables with lk->M.
//    The wave's argument block goes from global memory to LDS lane by lane (no register copy indexed at run time, hence no scratch on its way).
//  * one shared plant (Q.models == null): nothing to switch, the four episodes share one carve as before and C.plant is not read.
template <int F16>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_scenario_kernel(KArgs a0, LoopAdvance L, LoopPlant Q, LoopPeriod R, LoopScenario C) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = L.H, m = a0.m;
    const int tid = TeamWave::tid();
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    const bool per = Q.models != nullptr, live = b < L.B;      // (both wave-uniform)
    Smem sm = per ? carve(smem + (size_t)TeamWave::team() * smem_floats(1, m, 1), 1, m, 0) : carve(smem, 1, m, TeamWave::team());
    WaveW ww;
    KArgs* const lk = reinterpret_cast<KArgs*>(smem + TeamWave::IPB * smem_floats(1, m, 1) + (size_t)TeamWave::team() * plant_kargs_floats());
    if (!per) {                     // (workgroup-uniform: a kernel argument)
        load_weights(a0, sm, ww, threadIdx.x, TeamWave::BNT);
        __syncthreads();
    }
    if (!live) return;              // (wave-uniform; no workgroup-wide barrier below)
    const int lane = tid & 63, h = lane >> 5, n = Q.substeps;
    const bool lag = R.alpha > 0.0f, mine = lane < m, gust = C.dist != nullptr;
    const float* uo = L.uopt + (size_t)b * H * m;
    float* yw = L.u + (size_t)b * H * m;
    float* act = sm.v[5];           // [m] the applied control of the current substep
    float am = mine ? R.act[(size_t)b * m + lane] : 0.0f;
    float x[NX], xn[NX], xi[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
    const float* xrow = L.xi + (size_t)b * R.xi_ticks * n * NN;
    const float* drow = gust ? C.dist + (size_t)b * C.dist_ep_stride : nullptr;
    const int* prow = per ? C.plant + b : nullptr;
    int i = 0;
#pragma nounroll
    while (i < R.ticks) {           // one run of ticks that name the same plant
        KArgs a = a0;
        int iend = R.ticks;
        if (per) {
            const int p = __builtin_amdgcn_readfirstlane(prow[(size_t)i * C.plant_tick_stride]);
            iend = i + 1;
#pragma nounroll
            while (iend < R.ticks && __builtin_amdgcn_readfirstlane(prow[(size_t)iend * C.plant_tick_stride]) == p) ++iend;
            a.M = Q.models[p];
            a.wts = Q.wts + (size_t)p * Q.wts_stride;
            a.sdt = Q.sdt + (size_t)p * NN;
            TeamWave::sync();       // (the previous run's reads of the carve are done)
            load_weights(a, sm, ww, tid, TeamWave::NT);
            if (tid == 0) { lk->H = 1; lk->m = m; }
            const float* msrc = reinterpret_cast<const float*>(Q.models + p);
            float* mdst = reinterpret_cast<float*>(&lk->M);
            for (int e = tid; e < (int)(sizeof(ModelK) / sizeof(float)); e += TeamWave::NT) mdst[e] = msrc[e];      // (what block_prepass reads)
            TeamWave::sync();
        }
#pragma nounroll
        for (; i < iend; ++i) {
            const int row = (i < H - 1 ? i : H - 1) * m;
            float w[NN];
#pragma unroll
            for (int e = 0; e < NN; ++e)
                w[e] = gust ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, drow[(size_t)i * C.dist_tick_stride + e]))) : 0.0f;
#pragma nounroll
            for (int jj = 0; jj < n; ++jj) {
                const int q = i * n + jj;
                if (lag || jj == 0 || q == R.arrive) {
                    if (mine) {
                        const float c = (q >= R.arrive ? uo : yw)[row + lane];
                        am = lag ? FMA(R.alpha, c - am, am) : c;
                        act[lane] = am;
                    }
                    TeamWave::sync();       // (the row is written, the previous substep's reads of the control table are done)
                    if (per) block_prepass<TeamWave>(*lk, sm, act, tid);
                    else block_prepass<TeamWave>(a0, sm, act, tid);
                    TeamWave::sync();
                }
                if (jj == 0 && mine) L.us[((size_t)i * L.B + b) * m + lane] = am;
#pragma unroll
                for (int e = 0; e < NN; ++e) xi[e] = xrow[q * NN + e];
                StepAux A;
                step_fwd<F16, false>(a, sm, ww, 0, h, lane, x, xi, xn, A);
#pragma unroll
                for (int e = 0; e < NX; ++e) x[e] = xn[e];
                if (gust) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) { x[3 + e] = FMA(w[e], C.dtp, x[3 + e]); x[10 + e] = FMA(w[3 + e], C.dtp, x[10 + e]); }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < NX; ++e) L.xs[((size_t)i * L.B + b) * NX + e] = x[e];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) L.x[(size_t)b * NX + i] = x[i];
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (mine) R.act[(size_t)b * m + lane] = am;
    for (int e = tid; e < H * m; e += TeamWave::NT) {   // y_{j+1}: row t = uopt_j[min(t + S, H - 1)]
        const int t = e / m, ts = t + R.shift < H ? t + R.shift : H - 1;
        yw[e] = uo[ts * m + (e - t * m)];
    }
}

hipError_t launch_loop_scenario(const KArgs& a, const LoopAdvance& L, const LoopPlant& Q, const LoopPeriod& R, const LoopScenario& C, hipStream_t st) {
    if (L.B < 1 || L.H != a.H || Q.substeps < 1 || (Q.models && (!Q.wts || !Q.sdt || Q.wts_stride < BLOB_FLOATS + VJP_BASE))) return hipErrorInvalidValue;
    if (!R.act || R.ticks < 1 || R.xi_ticks < R.ticks || R.shift < 1 || R.shift > a.H || R.arrive < 0 || !(R.alpha >= 0.0f && R.alpha <= 1.0f)) return hipErrorInvalidValue;
    if ((Q.models && !C.plant) || (C.plant_tick_stride != 0 && C.plant_tick_stride != L.B)) return hipErrorInvalidValue;
    if (C.dist_tick_stride < 0 || (C.dist_ep_stride != 0 && C.dist_ep_stride != NN) || !(C.dtp > 0.0f)) return hipErrorInvalidValue;
    KArgs k = a;
    k.H = 1;
    const size_t sb = Q.models ? TeamWave::IPB * (smem_bytes(1, k.m, 1) + sizeof(float) * plant_kargs_floats()) : smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    return with_f16(k.f16, [&](auto F16) {
        if (sb > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)sdempc_loop_scenario_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb);
            if (e != hipSuccess) return e;
        }
        sdempc_loop_scenario_kernel<F16><<<grid, TeamWave::BNT, sb, st>>>(k, L, Q, R, C);
        return hipGetLastError();
    });
}

// SPEC.md §11d: the scenario kernel with the vehicle's inner RATE LOOP in front of the motor lag — the loop the node flies through its thrust and body-rate
// setpoint interface. Body, hand-over and every argument of sdempc_loop_scenario_kernel (runs of ticks per plant, shared or per-episode LDS carves; C.dist and
// C.plant null when no scenario is given); what differs:
//  * the command of a substep is no longer a row of the solution but what the rate loop makes of it and of the plant's CURRENT body rates, so it changes on every
//    substep and block_prepass reruns on every substep, between the same pair of TeamWave::sync();
//  * the setpoint row (the m motor values, the three rates) sits at wave-uniform addresses and every lane reads all of it: the thrust is the sum of the m values in
//    index order in every lane (the order is part of the SPEC: no cross-lane reduction), the rate error, the integrator and the torque demand are wave-uniform
//    values computed redundantly by every lane from lane 0's copy of omega (readfirstlane), and lane l < m forms motor l's command;
//  * gains, mixer and bounds are kernel arguments: the gains are read at static indices, row l of the mixer and of the bounds by lane l from the UNTOUCHED argument W
//    (a load from the argument segment at a computed offset; a copy of W indexed at run time would live in scratch), once, before the tick loop;
//  * the rate tail W.wt is read inside the substep loop and rewritten, shifted like the warm start, after it, by the same wave; the integrator W.g goes in and out
//    like the motor state; W.ws takes the setpoint in force at each tick's first substep.
template <int F16>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_rate_kernel(KArgs a0, LoopAdvance L, LoopPlant Q, LoopPeriod R, LoopScenario C, LoopRate W) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int H = L.H, m = a0.m;
    const int tid = TeamWave::tid();
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    const bool per = Q.models != nullptr, live = b < L.B;      // (both wave-uniform)
    Smem sm = per ? carve(smem + (size_t)TeamWave::team() * smem_floats(1, m, 1), 1, m, 0) : carve(smem, 1, m, TeamWave::team());
    WaveW ww;
    KArgs* const lk = reinterpret_cast<KArgs*>(smem + TeamWave::IPB * smem_floats(1, m, 1) + (size_t)TeamWave::team() * plant_kargs_floats());
    if (!per) {                     // (workgroup-uniform: a kernel argument)
        load_weights(a0, sm, ww, threadIdx.x, TeamWave::BNT);
        __syncthreads();
    }
    if (!live) return;              // (wave-uniform; no workgroup-wide barrier below)
    const int lane = tid & 63, h = lane >> 5, n = Q.substeps;
    const bool lag = R.alpha > 0.0f, mine = lane < m, gust = C.dist != nullptr;
    const float* uo = L.uopt + (size_t)b * H * m;
    float* yw = L.u + (size_t)b * H * m;
    const float* xe = W.xevol + (size_t)b * (H + 1) * NX;
    float* wt = W.wt + (size_t)b * H * 3;
    float* act = sm.v[5];           // [m] the applied control of the current substep
    float am = mine ? R.act[(size_t)b * m + lane] : 0.0f;
    const int ml = mine ? lane : 0;                             // (lanes >= m compute motor 0's command and drop it)
    const float M0 = W.M[ml][0], M1 = W.M[ml][1], M2 = W.M[ml][2], ulo = W.lo[ml], uhi = W.hi[ml];
    float g[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) g[e] = W.g[(size_t)b * 3 + e];
    float x[NX], xn[NX], xi[NN];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
    const float* xrow = L.xi + (size_t)b * R.xi_ticks * n * NN;
    const float* drow = gust ? C.dist + (size_t)b * C.dist_ep_stride : nullptr;
    const int* prow = per ? C.plant + b : nullptr;
    int i = 0;
#pragma nounroll
    while (i < R.ticks) {           // one run of ticks that name the same plant
        KArgs a = a0;
        int iend = R.ticks;
        if (per) {
            const int p = __builtin_amdgcn_readfirstlane(prow[(size_t)i * C.plant_tick_stride]);
            iend = i + 1;
#pragma nounroll
            while (iend < R.ticks && __builtin_amdgcn_readfirstlane(prow[(size_t)iend * C.plant_tick_stride]) == p) ++iend;
            a.M = Q.models[p];
            a.wts = Q.wts + (size_t)p * Q.wts_stride;
            a.sdt = Q.sdt + (size_t)p * NN;
            TeamWave::sync();       // (the previous run's reads of the carve are done)
            load_weights(a, sm, ww, tid, TeamWave::NT);
            if (tid == 0) { lk->H = 1; lk->m = m; }
            const float* msrc = reinterpret_cast<const float*>(Q.models + p);
            float* mdst = reinterpret_cast<float*>(&lk->M);
            for (int e = tid; e < (int)(sizeof(ModelK) / sizeof(float)); e += TeamWave::NT) mdst[e] = msrc[e];      // (what block_prepass reads)
            TeamWave::sync();
        }
#pragma nounroll
        for (; i < iend; ++i) {
            const int r = i < H - 1 ? i : H - 1, row = r * m;
            float w[NN];
#pragma unroll
            for (int e = 0; e < NN; ++e)
                w[e] = gust ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, drow[(size_t)i * C.dist_tick_stride + e]))) : 0.0f;
#pragma nounroll
            for (int jj = 0; jj < n; ++jj) {
                const int q = i * n + jj;
                const bool fresh = q >= R.arrive;               // (wave-uniform: the arrival point is the same for every episode)
                const float* us_ = (fresh ? uo : yw) + row;     // the motor row in force
                const float* ws_ = fresh ? xe + (size_t)(r + 1) * NX + 10 : wt + (size_t)r * 3;     // the rate row in force
                float cbar = us_[0];                            // 1. setpoint: thrust, the sum left to right in every lane
#pragma nounroll
                for (int l = 1; l < m; ++l) cbar = cbar + us_[l];
                cbar = cbar * W.inv_m;
                float tau[3], wsp[3];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    wsp[e] = ws_[e];
                    const float om = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x[10 + e])));
                    const float er = wsp[e] - om;               // 2. error, against the state of THIS substep
                    const float gi = FMA(W.ki_dt[e], er, g[e]), gl = W.glim[e];
                    g[e] = gi < -gl ? -gl : (gi > gl ? gl : gi);        // 3. integrator
                    tau[e] = FMA(W.kp[e], er, g[e]);            // 4. torque demand, with the updated integrator
                }
                const float ul = us_[ml];
                const float mx = FMA(M2, tau[2], FMA(M1, tau[1], FMA(M0, tau[0], cbar)));
                const float cw = mx < ulo ? ulo : (mx > uhi ? uhi : mx);       // 5. mixer, clamped to the input bounds
                const float c = W.w == 0.0f ? cw : (W.w == 1.0f ? ul : FMA(W.w, ul - cw, cw));      // 6. blend
                if (mine) {
                    am = lag ? FMA(R.alpha, c - am, am) : c;
                    act[lane] = am;
                }
                TeamWave::sync();       // (the row is written, the previous substep's reads of the control table are done)
                if (per) block_prepass<TeamWave>(*lk, sm, act, tid);
                else block_prepass<TeamWave>(a0, sm, act, tid);
                TeamWave::sync();
                if (jj == 0) {
                    if (mine) L.us[((size_t)i * L.B + b) * m + lane] = am;
                    if (lane == 0) {
                        float* wo = W.ws + ((size_t)i * L.B + b) * 4;
                        wo[0] = cbar; wo[1] = wsp[0]; wo[2] = wsp[1]; wo[3] = wsp[2];
                    }
                }
#pragma unroll
                for (int e = 0; e < NN; ++e) xi[e] = xrow[q * NN + e];
                StepAux A;
                step_fwd<F16, false>(a, sm, ww, 0, h, lane, x, xi, xn, A);
#pragma unroll
                for (int e = 0; e < NX; ++e) x[e] = xn[e];
                if (gust) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) { x[3 + e] = FMA(w[e], C.dtp, x[3 + e]); x[10 + e] = FMA(w[3 + e], C.dtp, x[10 + e]); }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < NX; ++e) L.xs[((size_t)i * L.B + b) * NX + e] = x[e];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) L.x[(size_t)b * NX + i] = x[i];
#pragma unroll
        for (int e = 0; e < 3; ++e) W.g[(size_t)b * 3 + e] = g[e];
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (mine) R.act[(size_t)b * m + lane] = am;
    for (int e = tid; e < H * m; e += TeamWave::NT) {   // y_{j+1}: row t = uopt_j[min(t + S, H - 1)]
        const int t = e / m, ts = t + R.shift < H ? t + R.shift : H - 1;
        yw[e] = uo[ts * m + (e - t * m)];
    }
    for (int e = tid; e < H * 3; e += TeamWave::NT) {   // rate tail: row t = xevol_j[min(t + S, H - 1) + 1][10..12]
        const int t = e / 3, ts = t + R.shift < H ? t + R.shift : H - 1;
        wt[e] = xe[(size_t)(ts + 1) * NX + 10 + (e - t * 3)];
    }
}

hipError_t launch_loop_rate(const KArgs& a, const LoopAdvance& L, const LoopPlant& Q, const LoopPeriod& R, const LoopScenario& C, const LoopRate& W, hipStream_t st) {
    if (L.B < 1 || L.H != a.H || Q.substeps < 1 || (Q.models && (!Q.wts || !Q.sdt || Q.wts_stride < BLOB_FLOATS + VJP_BASE))) return hipErrorInvalidValue;
    if (!R.act || R.ticks < 1 || R.xi_ticks < R.ticks || R.shift < 1 || R.shift > a.H || R.arrive < 0 || !(R.alpha >= 0.0f && R.alpha <= 1.0f)) return hipErrorInvalidValue;
    if ((Q.models && !C.plant) || (C.plant_tick_stride != 0 && C.plant_tick_stride != L.B)) return hipErrorInvalidValue;
    if (C.dist_tick_stride < 0 || (C.dist_ep_stride != 0 && C.dist_ep_stride != NN) || !(C.dtp > 0.0f)) return hipErrorInvalidValue;
    if (!W.xevol || !W.wt || !W.g || !W.ws || !(W.w >= 0.0f && W.w <= 1.0f) || a.m < 1 || a.m > 8) return hipErrorInvalidValue;
    KArgs k = a;
    k.H = 1;
    const size_t sb = Q.models ? TeamWave::IPB * (smem_bytes(1, k.m, 1) + sizeof(float) * plant_kargs_floats()) : smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    return with_f16(k.f16, [&](auto F16) {
        if (sb > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)sdempc_loop_rate_kernel<F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb);
            if (e != hipSuccess) return e;
        }
        sdempc_loop_rate_kernel<F16><<<grid, TeamWave::BNT, sb, st>>>(k, L, Q, R, C, W);
        return hipGetLastError();
    });
}

hipError_t launch_loop_advance(const KArgs& a, const LoopAdvance& L, hipStream_t st) {
    if (L.B < 1 || L.H != a.H) return hipErrorInvalidValue;
    KArgs k = a;
    k.H = 1;
    const size_t sb = smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    return with_f16(k.f16, [&](auto F16) {
        sdempc_loop_advance_kernel<F16><<<grid, TeamWave::BNT, sb, st>>>(k, L);
        return hipGetLastError();
    });
}
