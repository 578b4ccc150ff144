// sdempc_loop.inc.h — the plant of the batched closed loop (SPEC.md §11): one Euler–Maruyama step of the handle's own model per episode and
// tick, plus the hand-over to the next tick's solve (applied control, shifted warm start, step size); §11a: a separate plant; §11b: a whole solve period; §11c: a period with a scenario; §11d: a period flown through the rate-setpoint interface; §11e: per-motor actuator faults and substep-resolution states.
// Fragment of sdempc_kernels.hip, translation unit SDEMPC_TU = 4: included inside namespace sdempc::{exact|fastm} (compiled once per math mode).
//
// The step is the rollout's own device code: step_fwd at t = 0 on a control table built by block_prepass, i.e. the arithmetic of step 0
// of every rollout (Oracle.step(x, u, xi, t=0)), in every mlp_dtype and math mode. One wave per episode, four episodes per workgroup
// (TeamWave): all 32 particle columns of the tile carry the same state and noise, and lane 0's copy is the result. The kernels get the
// handle's argument block with H = 1 (a one-step horizon: the staged tables and the control table hold step 0 only); L.H is the solve's horizon.
//
// Two kernels, built from the four pieces below (prologue, stage_plant, prepass + substep, hand-over), each of which exists once:
//  * sdempc_loop_tick_kernel (§11, §11a): one control tick, the prepass straight from the solution's first row;
//  * sdempc_loop_period_kernel<F16, SCEN, RATE, FAULT> (§11b .. §11e): a whole solve period, the command going through the motor lag and an LDS row.
// Arguments: LoopAdvance, LoopPlant, LoopPeriod, LoopScenario, LoopRate, LoopFault (sdempc_kernels.h).
//
// The plant set (§11a). The argument block a0 arrives with the PLANT's arithmetic (the kernel's namespace and F16 are the plant's, independent of the solve's) and
// dt -> the plant's step length. With one shared plant (Q.models == null) a0 carries it and the four episodes of a workgroup share one LDS carve. With per-episode
// plants the workgroup's LDS holds four carves of one team each (16 KB per episode, 64 KB per workgroup: two workgroups per CU) and every wave stages the plant
// it flies into its own (stage_plant). block_prepass indexes the rotor tables of its argument block by a run-time motor index, which a kernel argument serves by a
// scalar load at a computed offset but a modified copy could only serve from scratch: the per-episode path hands it the wave's argument block in LDS
// (plant_kargs_floats() floats per wave behind the carves) and keeps the register copy for step_fwd, whose indices are all static. So a0 stays the UNTOUCHED
// kernel argument everywhere: it is what the shared-plant prepass indexes at run time.
__host__ __device__ constexpr int plant_kargs_floats() { return (int)((sizeof(KArgs) + 15) / 16 * 4); }

// what a wave knows of itself and of its LDS once the prologue is through
struct LoopWave {
    Smem sm;                // the carve the wave steps in: the workgroup's (one shared plant) or its own (per-episode plants)
    WaveW ww;
    KArgs* lk;              // per-episode plants: the wave's argument block in LDS (what block_prepass reads)
    int b, tid, lane, h;    // episode (wave-uniform), thread of the team, lane, lane half
    bool per;               // per-episode plants (wave-uniform: a kernel argument)
};

// Prologue: the wave's episode, its carve and its argument block in LDS; one shared plant is staged here, by the whole workgroup. Returns whether the wave has an
// episode: the kernel returns at once if not (wave-uniform), so every barrier after the prologue is TeamWave::sync(), never __syncthreads().
DI bool loop_prologue(float* smem, const KArgs& a0, const LoopAdvance& L, const LoopPlant& Q, LoopWave& w) {
    const int m = a0.m;
    w.tid = TeamWave::tid(); w.lane = w.tid & 63; w.h = w.lane >> 5;
    w.b = __builtin_amdgcn_readfirstlane(blockIdx.x * TeamWave::IPB + TeamWave::team());
    w.per = Q.models != nullptr;
    w.sm = w.per ? carve(smem + (size_t)TeamWave::team() * smem_floats(1, m, 1), 1, m, 0) : carve(smem, 1, m, TeamWave::team());
    w.lk = reinterpret_cast<KArgs*>(smem + TeamWave::IPB * smem_floats(1, m, 1) + (size_t)TeamWave::team() * plant_kargs_floats());
    if (!w.per) {                   // (workgroup-uniform)
        load_weights(a0, w.sm, w.ww, threadIdx.x, TeamWave::BNT);
        __syncthreads();
    }
    return w.b < L.B;
}

// Per-episode plants: the wave takes plant p. `a` (a copy of a0) gets p's M, wts and sdt, read through the readfirstlane'd index (wave-uniform addresses: scalar
// loads, so the model constants stay in SGPRs as the kernel arguments they replace do); the wave's own carve gets p's images and tables (sigma sqrt(dt) travels
// with the weights: sm.sdt) and the wave's argument block in LDS p's rotor tables, from global memory lane by lane (no register copy indexed at run time, hence
// no scratch on its way). TeamWave::sync on both sides: the earlier reads of the carve are done, the new images are written.
DI void stage_plant(const LoopPlant& Q, int p, KArgs& a, LoopWave& w) {
    a.M = Q.models[p];
    a.wts = Q.wts + (size_t)p * Q.wts_stride;
    a.sdt = Q.sdt + (size_t)p * NN;
    TeamWave::sync();
    load_weights(a, w.sm, w.ww, w.tid, TeamWave::NT);
    if (w.tid == 0) { w.lk->H = 1; w.lk->m = a.m; }
    const float* msrc = reinterpret_cast<const float*>(Q.models + p);
    float* mdst = reinterpret_cast<float*>(&w.lk->M);
    for (int e = w.tid; e < (int)(sizeof(ModelK) / sizeof(float)); e += TeamWave::NT) mdst[e] = msrc[e];      // (what block_prepass reads)
    TeamWave::sync();
}

// Control table row 0 from the m applied controls at u, with the wave's plant's polynomials and W1u. The first sync: u is written (where it is an LDS row) and
// the previous substep's reads of the control table are done.
DI void loop_prepass(const KArgs& a0, const LoopWave& w, const float* u) {
    TeamWave::sync();
    if (w.per) block_prepass<TeamWave>(*w.lk, w.sm, u, w.tid);
    else block_prepass<TeamWave>(a0, w.sm, u, w.tid);
    TeamWave::sync();
}

// One Euler–Maruyama step of the plant on the control table as it stands: step_fwd at t = 0 under the noise row xi_row, the new state fed back into x. With a
// disturbance (gust; SPEC.md §11c) the register copy of x then takes v_e <- fma(wd[e], dtp, v_e) and omega_e <- fma(wd[3 + e], dtp, omega_e), dtp the plant's
// step length: six fmas, applied whenever a schedule is given (zero rows included).
template <int F16>
DI void loop_substep(const KArgs& a, const LoopWave& w, const float* xi_row, float* x, bool gust, const float* wd, float dtp) {
    float xn[NX], xi[NN];
#pragma unroll
    for (int e = 0; e < NN; ++e) xi[e] = xi_row[e];
    StepAux A;
    step_fwd<F16, false>(a, w.sm, w.ww, 0, w.h, w.lane, x, xi, xn, A);
#pragma unroll
    for (int e = 0; e < NX; ++e) x[e] = xn[e];
    if (gust) {
#pragma unroll
        for (int e = 0; e < 3; ++e) { x[3 + e] = FMA(wd[e], dtp, x[3 + e]); x[10 + e] = FMA(wd[3 + e], dtp, x[10 + e]); }
    }
}

// Hand-over to the next solve: the state, the step size (info[1]), the sticky gave_up flag from the cooperative barrier word, the motor state (act: [B][m], or
// null) and the warm start, row t <- uopt[min(t + shift, H - 1)]. Every read of the warm start by this wave has happened before: it is rewritten here.
DI void loop_handover(const LoopAdvance& L, const LoopWave& w, int m, const float* x, const float* uo, int shift, float* act, float am) {
    const int H = L.H, b = w.b;
    if (w.lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) L.x[(size_t)b * NX + i] = x[i];
        L.step[b] = L.info[(size_t)b * 8 + 1];
        if (L.coop_bar && L.coop_bar[(size_t)COOP_BAR_WORDS * b + 1] != 0u) *L.gave_up = 1u;
    }
    if (act && w.lane < m) act[(size_t)b * m + w.lane] = am;
    float* un = L.u + (size_t)b * H * m;
    for (int e = w.tid; e < H * m; e += TeamWave::NT) {
        const int t = e / m, ts = t + shift < H ? t + shift : H - 1;
        un[e] = uo[ts * m + (e - t * m)];
    }
}

// SPEC.md §11, §11a: one control tick. Episode b is stepped by the model Q names for it (the handle's own: Q.models null, Q.substeps 1), Q.substeps times at the
// plant's own step length, the applied control uopt_k[0] held: the prepass runs once per tick, straight from the solution (no LDS row in between), and every
// substep is step_fwd at t = 0, xn fed back. The plant index is read before the kernel's first store. L.xi is [B][substeps][6].
// PLANT false: the plain loop (§11) as an instantiation of its own — no plant set and one substep known at compile time, which keeps it at the registers (and, in
// exact f32 / f16, the four waves per SIMD) it has always had; Q is not read.
template <int F16, bool PLANT>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_tick_kernel(KArgs a0, LoopAdvance L, LoopPlant Q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (!PLANT) { Q = LoopPlant{}; Q.substeps = 1; }
    LoopWave w;
    if (!loop_prologue(smem, a0, L, Q, w)) return;
    const int H = L.H, m = a0.m, b = w.b;
    KArgs a = a0;
    if (w.per) stage_plant(Q, __builtin_amdgcn_readfirstlane(Q.plant_of ? Q.plant_of[b] : b), a, w);
    const float* uo = L.uopt + (size_t)b * H * m;
    float x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
    loop_prepass(a0, w, uo);
    const float* xrow = L.xi + (size_t)b * Q.substeps * NN;
#pragma nounroll
    for (int j = 0; j < Q.substeps; ++j) loop_substep<F16>(a, w, xrow + j * NN, x, false, nullptr, 0.0f);
    if (w.lane == 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) L.xs[(size_t)b * NX + i] = x[i];
    }
    if (w.lane < m) L.us[(size_t)b * m + w.lane] = uo[w.lane];
    loop_handover(L, w, m, x, uo, 1, nullptr, 0.0f);      // y_{k+1} = [uopt_k[1:], uopt_k[H-1]]
}

// SPEC.md §11b: a whole solve period behind the same plant set — R.ticks control ticks of Q.substeps Euler–Maruyama steps each in ONE launch, so that a loop
// whose ticks are millisecond-scale solves does not pay a launch per plant step. Substep q = i * substeps + jj of the period flies row min(i, H - 1) of the
// previous solution's tail (L.u: the warm start y_j) while q < R.arrive and of this period's solution (L.uopt) from then on; the arrival point is the same for
// every episode, so the choice is wave-uniform. Lane l < m carries motor l's state: a_l <- fma(alpha, c_l - a_l, a_l) before every substep, or a_l = c_l with the
// lag off. The applied control row lives in the team's sm.v[5] (an optimiser vector the step does not use) and the prepass reruns whenever it can have changed:
// every substep with the lag on, at tick starts and at the arrival substep otherwise (rerunning it on an unchanged row writes the same table).
// Every read of the warm start precedes its rewrite: the commands are read inside the substep loop, the shifted rows are written after it, by the same wave.
//
// The ticks of the period are walked in RUNS of ticks that name one plant. A run starts by staging that plant (stage_plant), so inside a run the model constants
// are values defined before the tick loop, not loop-carried ones. The state x, the motor state, the applied-control row and the noise rows carry over a switch
// untouched. Without SCEN the period is one run, flown by plant Q.plant_of[b] (or b); with one shared plant (Q.models == null) there is nothing to stage or to
// switch, and neither Q.plant_of nor C.plant is read.
//
// SCEN (SPEC.md §11c): a scenario — the plant that flies each tick (C.plant: a plant index per tick and episode, which replaces Q.plant_of) and per control tick an
// external acceleration on the state (C.dist: a disturbance row, six floats at a wave-uniform address, held over the tick's substeps; see loop_substep).
//
// RATE (SPEC.md §11d, with SCEN; C.dist and C.plant null when no scenario is given): the vehicle's inner RATE LOOP in front of the motor lag — the loop the node
// flies through its thrust and body-rate setpoint interface.
//  * the command of a substep is no longer a row of the solution but what the rate loop makes of it and of the plant's CURRENT body rates, so it changes on every
//    substep and the prepass reruns on every substep;
//  * the setpoint row (the m motor values, the three rates) sits at wave-uniform addresses and every lane reads all of it: the thrust is the sum of the m values in
//    index order in every lane (the order is part of the SPEC: no cross-lane reduction), the rate error, the integrator and the torque demand are wave-uniform
//    values computed redundantly by every lane from lane 0's copy of omega (readfirstlane), and lane l < m forms motor l's command;
//  * gains, mixer and bounds are kernel arguments: the gains are read at static indices, row l of the mixer and of the bounds by lane l from the UNTOUCHED argument W
//    (a load from the argument segment at a computed offset; a copy of W indexed at run time would live in scratch), once, before the tick loop;
//  * the rate tail W.wt is read inside the substep loop and rewritten, shifted like the warm start, after it, by the same wave; the integrator W.g goes in and out
//    like the motor state; W.ws takes the setpoint in force at each tick's first substep.
//
// FAULT (SPEC.md §11e, with SCEN; with or without RATE): two optional additions, each behind a pointer that may be null.
//  * V.fault: a row (kappa_l, beta_l) per control tick, episode and motor. Lane l < m loads its pair once per tick, before the substep loop, and what it writes
//    into the LDS command row the prepass reads is fma(kappa_l, a_l, beta_l) — NOT into its motor state: the lag, us and the hand-over keep a_l. Without lag and
//    without rate loop the row is rewritten only when `moved`; a fault row changes at a tick start, which always is one, so the faulted value is what is in the
//    row whenever the control table is formed. The fma is applied whenever a schedule is given, neutral rows (1, 0) included.
//  * V.xsub: lane 0 stores the state after every substep (after the gust fmas), substep rows B episodes apart like the tick rows of L.xs.
// Without SCEN / RATE / FAULT the kernel takes an empty LoopAbsent in place of C / W / V: its argument segment is what the feature needs, no more.
struct LoopAbsent {};
template <int F16, bool SCEN, bool RATE, bool FAULT>
__global__ void __launch_bounds__(TeamWave::BNT) sdempc_loop_period_kernel(KArgs a0, LoopAdvance L, LoopPlant Q, LoopPeriod R, std::conditional_t<SCEN, LoopScenario, LoopAbsent> C,
                                                                           std::conditional_t<RATE, LoopRate, LoopAbsent> W, std::conditional_t<FAULT, LoopFault, LoopAbsent> V) {
    static_assert(SCEN || !RATE, "the rate loop comes with the scenario's arguments");
    static_assert(SCEN || !FAULT, "faults and substep states come with the scenario's arguments");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    LoopWave w;
    if (!loop_prologue(smem, a0, L, Q, w)) return;
    const int H = L.H, m = a0.m, b = w.b, lane = w.lane, n = Q.substeps;
    const bool lag = R.alpha > 0.0f, mine = lane < m;
    bool gust = false;              // a disturbance schedule is given
    float dtp = 0.0f;
    const float* drow = nullptr;
    if constexpr (SCEN) {
        gust = C.dist != nullptr;
        dtp = C.dtp;
        if (gust) drow = C.dist + (size_t)b * C.dist_ep_stride;
    }
    const float* uo = L.uopt + (size_t)b * H * m;
    float* yw = L.u + (size_t)b * H * m;
    const float* xe = nullptr;
    float* wt = nullptr;
    float* act = w.sm.v[5];         // [m] the applied control of the current substep
    float am = mine ? R.act[(size_t)b * m + lane] : 0.0f;
    const int ml = mine ? lane : 0;                             // (lanes >= m compute motor 0's command and drop it)
    float M0 = 0.0f, M1 = 0.0f, M2 = 0.0f, ulo = 0.0f, uhi = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (RATE) {
        xe = W.xevol + (size_t)b * (H + 1) * NX;
        wt = W.wt + (size_t)b * H * 3;
        M0 = W.M[ml][0]; M1 = W.M[ml][1]; M2 = W.M[ml][2]; ulo = W.lo[ml]; uhi = W.hi[ml];
#pragma unroll
        for (int e = 0; e < 3; ++e) g[e] = W.g[(size_t)b * 3 + e];
    }
    float x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = L.x[(size_t)b * NX + i];
    const float* xrow = L.xi + (size_t)b * R.xi_ticks * n * NN;
    bool faulty = false;            // a fault schedule is given
    const float* frow = nullptr;
    float* xsub = nullptr;
    if constexpr (FAULT) {
        faulty = V.fault != nullptr;
        if (faulty) frow = V.fault + (size_t)b * V.fault_ep_stride + 2 * ml;
        if (V.xsub) xsub = V.xsub + (size_t)b * NX;
    }
    int i = 0;
    auto fly = [&](const KArgs& a, int iend) __attribute__((always_inline)) {      // the ticks [i, iend) of one run: `a` holds the plant that flies them
#pragma nounroll
        for (; i < iend; ++i) {
            const int r = i < H - 1 ? i : H - 1, row = r * m;
            float wd[NN];
#pragma unroll
            for (int e = 0; e < NN; ++e) wd[e] = 0.0f;
            if constexpr (SCEN) {
                if (gust) {
#pragma unroll
                    for (int e = 0; e < NN; ++e)
                        wd[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, drow[(size_t)i * C.dist_tick_stride + e])));
                }
            }
            float fk = 1.0f, fb = 0.0f;                         // the fault row of this tick: lane l < m holds motor l's (kappa, beta)
            if constexpr (FAULT) {
                if (faulty) { fk = frow[(size_t)i * V.fault_tick_stride]; fb = frow[(size_t)i * V.fault_tick_stride + 1]; }
            }
#pragma nounroll
            for (int jj = 0; jj < n; ++jj) {
                const int q = i * n + jj;
                const bool fresh = q >= R.arrive;               // (wave-uniform: the arrival point is the same for every episode)
                bool moved = true;                              // the command can have changed since the last prepass
                float c = 0.0f;
                if constexpr (RATE) {
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
                    c = W.w == 0.0f ? cw : (W.w == 1.0f ? ul : FMA(W.w, ul - cw, cw));      // 6. blend
                    if (jj == 0 && lane == 0) {
                        float* wo = W.ws + ((size_t)i * L.B + b) * 4;
                        wo[0] = cbar; wo[1] = wsp[0]; wo[2] = wsp[1]; wo[3] = wsp[2];
                    }
                } else {
                    moved = lag || jj == 0 || q == R.arrive;
                    if (moved && mine) c = (fresh ? uo : yw)[row + lane];
                }
                if (moved) {
                    if (mine) {
                        am = lag ? FMA(R.alpha, c - am, am) : c;
                        if constexpr (FAULT) act[lane] = faulty ? FMA(fk, am, fb) : am;      // (between the command and the rotor: am stays the lag state)
                        else act[lane] = am;
                    }
                    loop_prepass(a0, w, act);
                }
                if (jj == 0 && mine) L.us[((size_t)i * L.B + b) * m + lane] = am;
                loop_substep<F16>(a, w, xrow + q * NN, x, gust, wd, dtp);
                if constexpr (FAULT) {
                    if (xsub && lane == 0) {
#pragma unroll
                        for (int e = 0; e < NX; ++e) xsub[(size_t)q * L.B * NX + e] = x[e];
                    }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int e = 0; e < NX; ++e) L.xs[((size_t)i * L.B + b) * NX + e] = x[e];
            }
        }
    };
    if constexpr (SCEN) {
#pragma nounroll
        while (i < R.ticks) {       // one run of ticks that name the same plant
            KArgs a = a0;
            int iend = R.ticks;
            if (w.per) {
                const int* prow = C.plant + b;
                const int p = __builtin_amdgcn_readfirstlane(prow[(size_t)i * C.plant_tick_stride]);
                iend = i + 1;
#pragma nounroll
                while (iend < R.ticks && __builtin_amdgcn_readfirstlane(prow[(size_t)iend * C.plant_tick_stride]) == p) ++iend;
                stage_plant(Q, p, a, w);
            }
            fly(a, iend);
        }
    } else {                        // one run, staged before the kernel's first store
        KArgs a = a0;
        if (w.per) stage_plant(Q, __builtin_amdgcn_readfirstlane(Q.plant_of ? Q.plant_of[b] : b), a, w);
        fly(a, R.ticks);
    }
    if constexpr (RATE) {
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) W.g[(size_t)b * 3 + e] = g[e];
        }
    }
    loop_handover(L, w, m, x, uo, R.shift, R.act, am);     // y_{j+1}: row t = uopt_j[min(t + S, H - 1)]
    if constexpr (RATE) {
        for (int e = w.tid; e < H * 3; e += TeamWave::NT) {   // rate tail: row t = xevol_j[min(t + S, H - 1) + 1][10..12]
            const int t = e / 3, ts = t + R.shift < H ? t + R.shift : H - 1;
            wt[e] = xe[(size_t)(ts + 1) * NX + 10 + (e - t * 3)];
        }
    }
}

// what a launch refuses, per argument struct (each checked where its struct is used)
inline bool loop_ok(const KArgs& a, const LoopAdvance& L, const LoopPlant& Q) {
    return !(L.B < 1 || L.H != a.H || Q.substeps < 1 || (Q.models && (!Q.wts || !Q.sdt || Q.wts_stride < BLOB_FLOATS + VJP_BASE)));
}
inline bool loop_ok(const KArgs& a, const LoopPeriod& R) {
    return !(!R.act || R.ticks < 1 || R.xi_ticks < R.ticks || R.shift < 1 || R.shift > a.H || R.arrive < 0 || !(R.alpha >= 0.0f && R.alpha <= 1.0f));
}
inline bool loop_ok(const LoopAdvance& L, const LoopPlant& Q, const LoopScenario& C) {
    return !((Q.models && !C.plant) || (C.plant_tick_stride != 0 && C.plant_tick_stride != L.B)) &&
           !(C.dist_tick_stride < 0 || (C.dist_ep_stride != 0 && C.dist_ep_stride != NN) || !(C.dtp > 0.0f));
}
inline bool loop_ok(const KArgs& a, const LoopRate& W) {
    return !(!W.xevol || !W.wt || !W.g || !W.ws || !(W.w >= 0.0f && W.w <= 1.0f) || a.m < 1 || a.m > 8);
}
inline bool loop_ok(const KArgs& a, const LoopFault& V) {
    return !(V.fault_tick_stride < 0 || (V.fault_ep_stride != 0 && V.fault_ep_stride != 2 * a.m) || a.m < 1 || a.m > 8);
}

// LDS of a workgroup (one carve of four teams, or four carves of one team and the four argument blocks), the opt-in above 64 KB, one wave per episode, the launch.
// `more`: the kernel's arguments after (KArgs, LoopAdvance, LoopPlant).
template <class Kernel, class... More>
hipError_t loop_launch(Kernel kernel, const KArgs& a, const LoopAdvance& L, const LoopPlant& Q, hipStream_t st, const More&... more) {
    KArgs k = a;
    k.H = 1;
    const size_t sb = Q.models ? TeamWave::IPB * (smem_bytes(1, k.m, 1) + sizeof(float) * plant_kargs_floats()) : smem_bytes(1, k.m, TeamWave::IPB);
    const dim3 grid((L.B + TeamWave::IPB - 1) / TeamWave::IPB);
    if (sb > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sb);
        if (e != hipSuccess) return e;
    }
    kernel<<<grid, TeamWave::BNT, sb, st>>>(k, L, Q, more...);
    return hipGetLastError();
}

// launch_loop of sdempc_kernels.h in this math mode
hipError_t launch_loop(const KArgs& a, const LoopAdvance& L, const LoopPlant* Q, const LoopPeriod* R, const LoopScenario* C, const LoopRate* W, hipStream_t st, const LoopFault* V) {
    LoopPlant own{};                // no plant set: the handle's own model (a's), one step per tick
    own.substeps = 1;
    const LoopPlant& q = Q ? *Q : own;
    if (!loop_ok(a, L, q) || (R && !loop_ok(a, *R)) || (C && !loop_ok(L, q, *C)) || (W && !loop_ok(a, *W)) || (V && !loop_ok(a, *V))) return hipErrorInvalidValue;
    if ((C && !R) || (W && !C) || (V && !C)) return hipErrorInvalidValue;
    return with_f16(a.f16, [&](auto F16) {
        if (!R) return Q ? loop_launch(sdempc_loop_tick_kernel<F16, true>, a, L, q, st) : loop_launch(sdempc_loop_tick_kernel<F16, false>, a, L, q, st);
        if (V && W) return loop_launch(sdempc_loop_period_kernel<F16, true, true, true>, a, L, q, st, *R, *C, *W, *V);
        if (V) return loop_launch(sdempc_loop_period_kernel<F16, true, false, true>, a, L, q, st, *R, *C, LoopAbsent{}, *V);
        if (W) return loop_launch(sdempc_loop_period_kernel<F16, true, true, false>, a, L, q, st, *R, *C, *W, LoopAbsent{});
        if (C) return loop_launch(sdempc_loop_period_kernel<F16, true, false, false>, a, L, q, st, *R, *C, LoopAbsent{}, LoopAbsent{});
        return loop_launch(sdempc_loop_period_kernel<F16, false, false, false>, a, L, q, st, *R, LoopAbsent{}, LoopAbsent{}, LoopAbsent{});
    });
}
