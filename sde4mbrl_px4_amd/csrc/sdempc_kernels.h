// sdempc_kernels.h — kernel argument block shared by the HIP kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// Which instantiations a build carries (DESIGN.md §2 "Instantiation set"). The default build holds what a handle with default options can be
// dispatched to for the reference's vehicles (m = 4 Iris, m = 6 Hexa) in every layout, plus the GENERIC motor count (the 8-slot, zero-padded
// instantiation: any m <= 8) in the one-group-per-wave tile layouts and the single-particle lane layout only. `make EXTRA=-DSDEMPC_ALL_VARIANTS=1`
// adds the generic motor count in the duo / six-team / cooperative / speculative layouts and the packed-f32 tanh instantiations of the exact tile
// layout (SDEMPC_OPT_PK; TeamBlock8): + 91 solve kernels, + 10 MB, + 7 CPU-minutes (tests/tools/soak.py draws them when they are there).
#ifndef SDEMPC_ALL_VARIANTS
#define SDEMPC_ALL_VARIANTS 0
#endif

namespace sdempc {

// float payload of the model blob (SPEC.md §2; include/sdempc.h: SDEMPC_BLOB_FLOATS), offsets in floats — one statement for the kernels and for sdempc_create
namespace blob {
constexpr int SF = 40;                   // sF[3], sT[3]
constexpr int SIGMA = 48;
constexpr int W1Z = 56, B1 = W1Z + 64 * 6, W1U = B1 + 64, W2 = W1U + 32 * 8, B2 = W2 + 32 * 32, W3 = B2 + 32, B3 = W3 + 8 * 32, W3N = B3 + 8, B3N = W3N + 32;
constexpr int FLOATS = B3N + 8;
static_assert(FLOATS == 2120, "include/sdempc.h: SDEMPC_BLOB_FLOATS");
}

struct ModelK {  // physics prior + small output-layer constants (SPEC.md §2), passed in SGPRs
    float inv_mass, grav, J[3], iJ[3], ct2, ct1, ct0, cm2, cm1;
    float rx[8], ry[8], dir[8];
    float sF[3], sT[3];
    float b3[6], b3n;
    float adj_s0, adj_i0;   // SPEC.md §10e (math_mode fast + f32x3): -2 * 2^eoff and 2^-eoff, the handle's scale offset of the adjoint's binary16 contractions
};
struct CostK {
    float perr[3], verr[3], qerr[3], werr[3];
    float res_mult, uerr, slew, slew_cc;
    int has_sc;
    float slew_lo[8], slew_hi[8], uref[8], ulo[8], uhi[8];
    int sc_n;                          // state_constr (SPEC.md §5.3): number of bounded states, 0: none
    struct StateBound { int id; float w, lo, hi; };
    const StateBound* sc_tab;          // device table [sc_n], ascending state index (owned by the handle)
};
struct ApgK {
    int max_iter, max_noimp, maxls, reset_inc;
    float atol, rtol, stepsize, smax, coef, dec, inc;
};
// Host-side dispatch options of one handle (include/sdempc.h: sdempc_set_option / SDEMPC_OPT_*). Travels inside KArgs so that the
// launchers see it; device code reads only coop_fence.
struct LaunchOpts {
    int cus;           // compute units of the handle's device (hipDeviceAttributeMultiprocessorCount), set when the device is bound
    int lane;          // 1: single-particle lane layout for P == 1 (default), 0: tile layout
    int coop;          // 1: cooperative multi-workgroup layouts for small batches (default), 0: off
    int spec;          // 1: speculative variant of the cooperative layout for the smallest batches (default), 0: off
    int pk;            // -1: packed-f32 tanh instantiation when the grid leaves one wave per SIMD (default), 0 / 1: forced
    int ustg;          // -1: per-step control table in global memory when that raises occupancy (default), 0 / 1: forced
    int coop_launch;   // 1: hipLaunchCooperativeKernel for the cooperative layouts, 0: plain launch of a grid sized to be resident (default)
    int duo;           // throughput launches in the duo tile layout (64 particles per wave): -1 auto (= on for multi-group instances), 0 off, 1 on
    int coop_fence;    // 1: agent-scope release / acquire fences around the grid barrier, 0: sc1 write-through hand-off only (default)
    int absent_wg;     // fault injection (tests): >= 0: that workgroup of a cooperative-layout grid leaves at once, as if it had never become resident; -1 (default): none
    int hex;           // 1: launches that fill every two-wave team slot of the device run one six-team workgroup per CU (default), 0: two-team workgroups always
};
constexpr int COOP_BAR_WORDS = 4;
struct KArgs {
    int H, P, m, G;
    int B;                     // instances in this launch (set by the launcher)
    float invP;
    ModelK M;
    CostK C;
    ApgK A;
    // device tables (owned by the handle)
    const float* dt;    // [H]
    const float* sdt;   // [H][6]  sigma_i * sqrt(dt_t)
    const float* disc;  // [H+1]   discount^t / H
    const float* beta;  // [max_iter+2] momentum table
    const float* wts;   // blob float payload
    // per call
    const float* x0;           // [B][13]
    const float* u;            // [B][H][m]   control sequence (rollout/grad) or warm start (solve)
    const float* xref;         // [B][H+1][13]
    const float* noise;        // [B][G][H][6][32]
    const float* stepsize_in;  // [B] (solve)
    float* traj;               // [B][G][H+1][13][32] workspace
    float* act;                // [B][G][H][ACT_STRIDE] activation checkpoint of the gradient's forward sweep
    float* part;               // [B][G][part_stride(H)] per-group particle sums (adjoint outputs per step / mean trajectory), SPEC.md §6.1
    float* cost;               // [B]
    float* grad;               // [B][H][m]
    float* xmean;              // [B][H+1][13] or null
    float* uopt;               // [B][H][m]
    float* info;               // [B][8] raw: sum_ls, stepsize, nit, grad_sqr, sum_s, c_init, c_opt, nls_total
    int store_traj;
    int ws_rows;               // rows (instances or team slots) of traj / act / part / ustg the handle has allocated (launchers refuse a grid that needs more)
    int f16;                   // mlp_dtype: 0 f32; 1 fp16-operand MLP contractions in the forward step (SPEC.md §9); 2 layer-2 / W2^T contractions as three-limb bf16 splits (§9b)
    // cooperative latency path (one instance over coop_nwg workgroups; workspace owned by the handle, see sdempc_api.cpp)
    int coop_nwg;
    int coop_ngrp;             // speculative variant: groups of coop_nwg workgroups per instance (2..7: SPEC_GROUPS)
    unsigned* coop_bar;        // [B][COOP_BAR_WORDS]: grid-barrier counter, error flag, arrivals of the streamed hand-off, pad (zeroed before every launch)
    float* ustg;               // [B][H][36] per-step control table in global memory (long horizons: keeps it out of LDS), or NULL
    unsigned coop_spin;        // time one grid barrier may wait before it gives up, in ticks of the 100 MHz s_memrealtime clock (10 ns)
    float* coop_pp;            // [B][2][part_stride(H)][G*32]
    float* coop_ck;            // [B][P][H+1][160]
    unsigned long long* work;  // [4] cumulative work of sdempc_solve_kernel launches: solves, gradient evaluations, forward-only rollouts (every line-search
                               // trial counted), and how many of those trials were settled without a rollout (nonneg below);
                               // [4] (as unsigned) the instance ticket word of the persistent launches (see ticket_base)
    int tickets;               // persistent launches: 1 = instances beyond the grid's first ones are handed out by the ticket word (set by the launcher)
    unsigned ticket_base;      // value of the ticket word when this launch starts (set by the launcher from *ticket_host)
    unsigned* ticket_host;     // HOST memory, owned by the handle: running total of the ticket word (it is never reset: every ticketed launch of B
                               // instances advances it by exactly B — B - S successful draws and one failing draw by each of the S teams)
    int fast;                  // SPEC.md §10: hardware transcendentals (selects the fastm translation unit; host-side switch)
    int nonneg;                // 1: every weight that enters a cost (C.perr .. C.slew_cc, the state-bound weights, disc[]) is >= 0 and not NaN, so no cost is
                               // negative and a line-search trial whose Armijo bound is negative is rejected without its rollout (SPEC.md §8; set at create)
    LaunchOpts opt;
};

// floats per (instance, group) row of KArgs::part: max(H*12 adjoint sums, (H+1)*13 state sums) + the group's cost total in the
// last element; multiple of 4
__host__ __device__ inline int part_stride(int H) { const int a = H * 12, b = (H + 1) * 13; return ((a > b ? a : b) + 1 + 3) & ~3; }
// Activation checkpoint of the gradient's forward sweep, floats per (instance, group, step): h2 tile (4 chunks x 64 lanes x 4) + step
// scalars (32 x 8). Checkpointing layer-1 tiles too was measured slower (HBM).
constexpr int ACT_STRIDE = 1280;
size_t smem_bytes(int H, int m, int ipb);   // ipb: instances (teams) per workgroup
// host function pointer of the kernel the calling thread launched last through the launch_* functions below (for sdempc_last_kernel_name)
void note_kernel(const void* host_fn);
const void* last_launched_kernel();
// The launchers and solve_workspace_rows serve both math modes: each picks sdempc::exact or sdempc::fastm (SPEC.md §10: the same source built with
// hardware transcendentals) from KArgs::fast.
// Cooperative latency path of the solve (exact f32, P >= 2): workgroups per instance, workspace sizes, launcher.
// coop_max_instances: how many instances fit one workgroup per CU on the current device (0 = path unavailable for this shape)
int coop_nwg(int P);
int coop_max_instances(int P, int H, int m, const LaunchOpts& o);
size_t coop_pp_floats(int H, int G);           // per instance
size_t coop_ck_floats(int H, int P);           // per instance
hipError_t launch_solve_coop(const KArgs& a, int B, hipStream_t st);
// speculative variant for the smallest batches (4 groups of workgroups per instance: two trials and two candidate gradients at once)
int spec_max_instances(int P, int H, int m, const LaunchOpts& o);
hipError_t launch_solve_spec(const KArgs& a, int B, hipStream_t st);
int team_ipb(int G, int H, int m);            // 4 when one wave owns an instance (G == 1 and LDS permits), else 1
hipError_t launch_rollout(const KArgs& a, int B, hipStream_t st);
hipError_t launch_grad(const KArgs& a, int B, hipStream_t st);
hipError_t launch_solve(const KArgs& a, int B, hipStream_t st);
// rows of KArgs::traj / act / part / ustg a solve launch of B instances indexes (B, or the team slots of a persistent launch)
int solve_workspace_rows(const KArgs& a, int B);
// SPEC.md §11, the batched closed loop: per-tick plant step and hand-over to the next solve (sdempc_loop.inc.h, translation unit SDEMPC_TU = 4)
struct LoopAdvance {
    const float* uopt;          // [B][H][m] this tick's solutions
    const float* info;          // [B][8] this tick's telemetry (step size at [1])
    const float* xi;            // [B][6] plant noise of this tick
    const unsigned* coop_bar;   // [B][COOP_BAR_WORDS] of this tick's cooperative-layout solve, or null
    float* x;                   // [B][13] x_k in, x_{k+1} out (the next solve's initial states)
    float* u;                   // [B][H][m] warm start of the next solve
    float* step;                // [B] step size of the next solve
    float* xs;                  // [B][13] x_{k+1} (output row of this tick)
    float* us;                  // [B][m] applied control uopt_k[0] (output row of this tick)
    unsigned* gave_up;          // one word, sticky: a grid barrier of a cooperative-layout solve of this loop gave up
    int B, H;
};
// SPEC.md §11a, the closed loop against a separate plant: which model steps episode b, and how often per tick. LoopAdvance::xi is [B][substeps][6] here.
// models == null: ONE plant for every episode — the launch's KArgs carry it (M, wts, sdt) and the four episodes of a workgroup share its LDS images,
// as without a plant set. Otherwise episode b is stepped by plant p = plant_of ? plant_of[b] : b, and every wave stages its own images.
struct LoopPlant {
    const ModelK* models;       // [Np] physics prior and output-layer constants of each prepared plant, or null
    const float* wts;           // [Np][wts_stride] prepared blob payloads (math_mode fast: forward block, then the block of the vector-Jacobian products)
    const float* sdt;           // [Np][6] sigma_i * sqrt(dt) of each plant
    const int* plant_of;        // [B] plant index of each episode, or null (identity)
    int wts_stride;             // floats between two plants' payloads
    int substeps;               // Euler–Maruyama steps per tick, the applied control held (>= 1)
};
// SPEC.md §11b, the closed loop at the node's timing: ONE launch advances a whole solve period — `ticks` control ticks of Q.substeps plant steps each —
// flying the previous solution's tail (LoopAdvance::u, the warm start y_j) until plant substep `arrive` of the period and this period's solution
// (LoopAdvance::uopt) from then on, through a first-order motor lag. Here LoopAdvance::xi is [B][xi_ticks][substeps][6], xs / us are [ticks][B][13] / [ticks][B][m]
// (tick rows B episodes apart) and LoopAdvance::u is read for the commands, then rewritten shifted by `shift` rows.
struct LoopPeriod {
    float* act;                 // [B][m] motor state a: in, and out after the period's last substep
    float alpha;                // motor lag: 0 off (a = c exactly), else a <- fma(alpha, c - a, a) before every substep
    int ticks;                  // control ticks of this period: min(S, T - j S), >= 1
    int xi_ticks;               // tick rows per episode in LoopAdvance::xi (>= ticks)
    int shift;                  // rows the warm start moves up: min(S, H) (row t <- uopt[min(t + shift, H - 1)])
    int arrive;                 // substep index inside the period at which the command source switches from y_j to uopt_j; >= ticks * substeps: never
};
// SPEC.md §11c, the closed loop with a scenario: the period launch plus a disturbance row per control tick and a plant index per control tick. Both
// pointers address the PERIOD's first tick (the host steps them from period to period); tick i of the period reads row i, or row 0 when the stride is 0.
struct LoopScenario {
    const float* dist;          // (w_v[3], w_omega[3]) of tick i, episode b at dist[i * dist_tick_stride + b * dist_ep_stride + 0..5], or null: no disturbance
    int dist_tick_stride;       // floats between two ticks' rows: Bd * 6, or 0 (one row for every tick)
    int dist_ep_stride;         // floats between two episodes' rows: 6, or 0 (one row for every episode)
    const int* plant;           // plant index of tick i, episode b at plant[i * plant_tick_stride + b]; required with per-episode plants (LoopPlant::models),
                                // where it replaces LoopPlant::plant_of; ignored with one shared plant
    int plant_tick_stride;      // B, or 0 (one row for every tick)
    float dtp;                  // the plant's step length (what LoopAdvance's KArgs::dt points at)
};
// SPEC.md §11d, the closed loop through the rate-setpoint interface: the scenario launch (C.dist / C.plant may be null: no scenario) with the vehicle's inner
// rate loop in front of the motor lag. On every plant substep the command is formed from the setpoint row in force — mean thrust of the motor row, body rates
// of this period's mean trajectory (xevol row r + 1) or, before the solution arrives, of the rate tail (row r) — and the plant's CURRENT body rates: PI on the
// rate error with a clamped integrator, mixer clamped to the input bounds, blend with the motor row. Gains, mixer and bounds travel by value (wave-uniform
// kernel arguments); lane l < m reads row l of the mixer and the bounds from the argument itself.
struct LoopRate {
    float kp[3], ki_dt[3], glim[3];     // per body axis: proportional gain, integral gain times the plant's step length, integrator limit (>= 0)
    float M[8][3];                      // mixer: motor l takes M[l][a] of the torque demand about axis a
    float lo[8], hi[8];                 // input bounds of motor l
    float inv_m;                        // float32(1) / float32(m)
    float w;                            // blend weight of the motor row: 0 rate setpoints only, 1 motor values only
    const float* xevol;                 // [B][H+1][13] this period's mean trajectories (rates at [10..12])
    float* wt;                          // [B][H][3] rate tail: read before the arrival, then rewritten from xevol shifted by LoopPeriod::shift rows
    float* g;                           // [B][3] integrator state: in, and out after the period's last substep
    float* ws;                          // [ticks][B][4] (mean thrust, rates[3]) in force at each tick's first substep
};
// SPEC.md §11e, per-motor actuator faults and substep-resolution states: the scenario or rate launch with two optional additions, either pointer may be null.
// A fault row (kappa_l, beta_l) per control tick, episode and motor sits between the motor state and the rotor: what the plant's control table is formed from
// is fma(kappa_l, a_l, beta_l), the motor state a_l itself (the lag state, us, u_act_next) is untouched. Like LoopScenario's pointers, both address the PERIOD's
// first tick (first substep row); tick i of the period reads row i, or row 0 when the stride is 0.
struct LoopFault {
    const float* fault;         // (kappa, beta) of tick i, episode b, motor l at fault[i * fault_tick_stride + b * fault_ep_stride + 2 * l + 0..1], or null: no fault
    int fault_tick_stride;      // floats between two ticks' rows: Bf * m * 2, or 0 (one row for every tick)
    int fault_ep_stride;        // floats between two episodes' rows: m * 2, or 0 (one row for every episode)
    float* xsub;                // [ticks * substeps][B][13] the state after every plant substep (disturbance fmas included), substep rows B episodes apart, or null
};
// The plant launch of every closed loop. Q null: the handle's own model, one step per tick (SPEC.md §11); otherwise `a` is the handle's argument block with the PLANT's
// arithmetic (f16, fast: the plant's math mode picks the kernel's), dt -> one float (the plant's step length) and, for one shared plant, its M / wts / sdt.
// R null: one control tick; otherwise a whole solve period, with a scenario if C is given (needs R) and through the rate loop if W is given (needs C).
// V given (needs C): the FAULT instantiations of the period kernel; V null: the launches of §11 .. §11d, whatever they were.
hipError_t launch_loop(const KArgs& a, const LoopAdvance& L, const LoopPlant* Q, const LoopPeriod* R, const LoopScenario* C, const LoopRate* W, hipStream_t st,
                       const LoopFault* V = nullptr);
// the tick's key schedule (sdempc_prng.hip): keys r_k -> r_{k+1} in place, the solve's noise keys into sub_dev u32[B][2], the plant noise into
// xi_dev f32[B][substeps][6]: ONE draw normal(p, 6 * substeps) per episode (SPEC.md §7.1: counter i pairs with i + 3 * substeps), row j for substep j
hipError_t launch_loop_keys(uint32_t* keys_dev, uint32_t* sub_dev, float* xi_dev, int B, hipStream_t st, int substeps = 1);
// SPEC.md §11b: the key schedule of one solve period — tick 0 is the schedule above, every later tick advances the key by ONE split (no solve, no solve
// key) and draws its plant noise the same way. xi_dev f32[B][xi_ticks][substeps][6], rows 0 .. ticks-1 written.
// SPEC.md §11f, the closed loop on a measured state: what the period's key-schedule thread of episode b does beside its schedule, right before solve j. It
// advances the observation key q_b by one split and, unless valid says 0, rewrites the held measurement xm_b from the plant state x_b: additive errors
// e_i = fma(sigma_i, xi_i, beta_i) on position, velocity and body rates, a small body-frame rotation on the attitude (xi = normal(me, (12,))). The solve
// then starts from xm instead of x. The row pointers address SOLVE j's rows (the host steps them from period to period). q null: absent — the kernel then
// makes no memory access it did not make before.
// SPEC.md §11g, an aged and renormalised estimate: with `age` given the measurement of episode b is formed from the plant state A = age[b * age_ep_stride] plant
// substeps before the solve — history row age_max - A (row i holds every episode's state age_max - i substeps back) — instead of x; A = 0 reads x. With
// `renorm` set the attitude of xm is scaled by the software rsqrt (SPEC.md §3.2) of its squared length after the product. Neither happens on a dropout. The
// defaults (null, 0) mean absent: an un-aged, un-normalised run makes no memory access it did not make before.
struct LoopObserve {
    uint32_t* q;                // [B][2] observation keys, advanced in place at every solve; null: no observation
    const float* x;             // [B][13] the plant state at the period's first tick
    float* xm;                  // [B][13] the held measurement: in, and out (what the solve reads)
    float* xmeas;               // [B][13] output row of this solve: xm after the update
    const float* sigma;         // noise scale of episode b at sigma[b * ep_stride + 0..11] (p, v, theta, omega), or null: zeros
    const float* beta;          // bias, same layout, or null: zeros
    int ep_stride;              // floats between two episodes' rows of sigma / beta: 12, or 0 (one row for every episode)
    const int32_t* valid;       // valid[b * valid_ep_stride] == 0: a dropout, xm stays as it is; null: always valid
    int valid_ep_stride;        // 1, or 0 (one flag for every episode)
    const float* hist;          // [age_max][hist_row_stride] the last age_max substep states before this solve, oldest first, episode b at + b * 13; read only where A > 0
    int hist_row_stride;        // floats between two history rows (>= B * 13)
    const int32_t* age;         // age[b * age_ep_stride] in [0, age_max]: the age of episode b's estimate at this solve, in plant substeps; null: every age 0
    int age_ep_stride;          // 1, or 0 (one age for every episode)
    int age_max;                // rows of hist
    int renorm;                 // 1: renormalise the attitude of xm (wave-uniform); 0: leave the product as it is
};
// SPEC.md §11h, scoring episodes on the device: ONE further launch of the period's key-schedule kernel at the end of every chunk, in its scoring form (ticks = 0,
// an empty LoopObserve, null key buffers: the key words are neither read nor written). Thread b walks the chunk's rows of episode b in time order and updates the
// episode's 16 score words (include/sdempc.h: the table at sdempc_score_cfg) from words[b] back to words[b]. All row buffers are [row][B][.]: the chunk's own.
// words null means absent: the period launches pass that, and the kernel then makes no memory access it did not make before.
struct LoopScore {
    uint32_t* words;            // [B][16] the score words: in, and out; null: no scoring
    const float* rows;          // [ticks * rows_per_tick][B][13] the scored rows in time order: the chunk's xs rows (rows_per_tick 1) or xsub rows (the plant's substeps)
    const float* us;            // [ticks][B][m] the chunk's applied controls
    const float* info;          // [solves][B][8] the chunk's telemetry rows
    const float* ref;           // target of chunk tick i, episode b at ref[i * ref_tick_stride + b * ref_ep_stride + 0..12] (position [0..2] and velocity [3..5] are read)
    int ref_tick_stride;        // floats between two ticks' targets: Br * 13, or 0 (one target for every tick)
    int ref_ep_stride;          // floats between two episodes' targets: 13, or 0 (one target for every episode)
    int ticks, rows_per_tick, solves;   // of this chunk
    int m;
    float r2_pos, cos_min, w2_max;      // thresholds: squared radius, cosine of the tilt, squared rate (+inf, -inf, +inf: off); never NaN
    float u_lo[8], u_hi[8], uref[8];    // of motor j < m (wave-uniform kernel arguments, read at constant indices)
    const int32_t* live;        // SPEC.md §11n: [B], episode b is scored only where live[b] != 0; null: every episode (not one access more)
};
// SPEC.md §11i, gusts and estimator bias drawn on the device: a first-order Gauss-Markov process per component and episode, stepped by the period's key-schedule
// thread of episode b beside its schedule. One step: (c, e) = split(c), xi = normal(e, (W,)) (counter i pairs with i + W / 2), t_i = scale_i * xi_i (rounded),
// g_i = fma(rho_i, g_i, t_i), row_i = g_i, or d_i + g_i when a scheduled input d is given as well. The disturbance half (W = 6) takes one step per control tick of
// the period and writes row (i, b) of dst, f32[ticks][B][6], which the plant launch then reads as its LoopScenario::dist (tick stride B * 6, episode stride 6); sched
// addresses the PERIOD's first tick. The bias half (W = 12) takes one step per launch, before the measurement is formed, dropout or not, and writes dst[b], f32[B][12]:
// the beta of this solve, read back by the same thread in place of LoopObserve::beta (which must then be null; the scheduled rows go to sched, of SOLVE j). chain
// null means absent: the kernel then makes no memory access it did not make before.
struct LoopProcessHalf {
    uint32_t* chain;            // [B][2] the process key chain, advanced in place; null: no process
    float* state;               // [B][W] g: in, and out
    const float* rho;           // rho of episode b at rho[b * par_ep_stride + 0..W-1]
    const float* scale;         // scale, same layout
    int par_ep_stride;          // floats between two episodes' rows of rho / scale: W, or 0 (one row for every episode)
    const float* sched;         // the scheduled input d of step i, episode b at sched[i * sched_tick_stride + b * sched_ep_stride + 0..W-1], or null: none
    int sched_tick_stride;      // floats between two steps' rows: Bd * W, or 0 (one row for every step)
    int sched_ep_stride;        // floats between two episodes' rows: W, or 0 (one row for every episode)
    float* dst;                 // the rows written: [ticks][B][6] (disturbance) or [B][12] (bias)
};
struct LoopProcess {
    LoopProcessHalf dist;       // W = 6, one step per control tick
    LoopProcessHalf bias;       // W = 12, one step per solve; needs LoopObserve::q
};
// SPEC.md §11k, motor faults and estimator dropouts drawn on the device: a finite Markov chain per lane, stepped by the period's key-schedule thread of episode b
// beside its schedule. A chain has K modes besides state 0. One step: (c, e) = split(c), w = random_bits(e, lanes) (counter k pairs with k + ceil(lanes / 2), a zero
// counter in an odd count's last block), and per lane with state s and word w_l: from s = 0 to j + 1 for the smallest j < K with w_l < onset[l][j] (else 0), from
// s > 0 to 0 if w_l < clear[l][s - 1] (else s). Integer compares only; a threshold of 0 never fires. One transition per step.
// The fault half (lanes = m <= 8) takes one step per control tick of the period and writes row (i, b) of dst, f32[ticks][B][m][2], which the plant launch then reads
// as its LoopFault::fault (tick stride B * m * 2, episode stride 2 m): in state 0 the scheduled row, or (1, 0) without a schedule; in state s > 0 the words of
// modes[l][s - 1], untouched. The episode's row of `chain` holds the key and (s, first) per motor: first = tick0 + i of the first step that left state 0, or -1. sched addresses the PERIOD's first
// tick. The dropout half (one lane, K = 1) takes one step per launch, before the measurement is formed, and writes dst[b] = (s == 0) & scheduled flag: the valid flag
// of this solve, which LoopObserve::valid must then address (episode stride 1; the scheduled flags go to sched, of SOLVE j). state holds (s, n_dropped). chain null
// means absent: the kernel then makes no memory access it did not make before.
constexpr int EVENT_EP_WORDS = 2 + 2 * 8;            // words of one episode's row of the fault chain: the key u32[2], then (s, first) i32 of motor l at 2 + 2 l
constexpr int EVENT_PAR_WORDS = 32 + 32 + 64;        // words of one row of fault parameters: onset u32[8][4], clear u32[8][4], modes f32[8][4][2] (motor l < m, mode j < K used)
struct LoopEventFault {
    uint32_t* chain;            // [B][EVENT_EP_WORDS] key and per-motor (s, first) of every episode, advanced in place; null: no chain
    const uint32_t* par;        // the parameters of episode b at par[b * par_ep_stride + ..]: onset cumulative and nondecreasing, clear, modes (kappa, beta) as words
    int par_ep_stride;          // EVENT_PAR_WORDS, or 0 (one row for every episode: every lane of a wave loads one address)
    int K, m;                   // modes 1..4, motors 1..8
    int tick0;                  // the global tick of the period's first tick (>= 0)
    const uint32_t* sched;      // the scheduled row of tick i, episode b at sched[i * sched_tick_stride + b * sched_ep_stride + 2 * l + 0..1] (words of floats), or null: (1, 0)
    int sched_tick_stride;      // words between two ticks' rows: Bf * m * 2, or 0
    int sched_ep_stride;        // words between two episodes' rows: m * 2, or 0
    uint32_t* dst;              // [ticks][B][m][2] the rows written (words of floats)
};
struct LoopEventDrop {
    uint32_t* chain;            // [B][2]; null: no chain
    int32_t* state;             // [B][2] (s, n_dropped): in, and out
    const uint32_t* drop;       // threshold of dropping of episode b at drop[b * par_ep_stride]
    const uint32_t* recover;    // threshold of recovering, same layout
    int par_ep_stride;          // 1, or 0 (one pair for every episode)
    const int32_t* sched;       // the scheduled flag of episode b at sched[b * sched_ep_stride], or null: 1
    int sched_ep_stride;        // 1, or 0
    int32_t* dst;               // [B] the flags written
};
struct LoopEvents {
    LoopEventFault fault;       // one step per control tick
    LoopEventDrop drop;         // one step per solve; needs LoopObserve::q, and LoopObserve::valid == dst
};
// SPEC.md §11l, the geometric baseline controller: ONE further launch of the period's key-schedule kernel per solve period, in its BASELINE form (ticks = 0, empty
// LoopObserve / LoopScore / LoopProcess / LoopEvents, null key buffers: the key words are neither read nor written), where the solve is launched otherwise. Thread b
// forms (c, omega*) of episode b from the state the solve would have started from and rows ref_row, ref_row + 1 of its reference window (sdempc_geo.inc.h) and
// fills what the rate-loop plant launch reads: uopt[b][t][l] = c, xevol[b][0] = x, xevol[b][t >= 1] = (0 .. 0, omega*), info[b] = (0, step[b], 0 ..). With `out`
// given it stores (c, omega*) there and nothing else (sdempc_geo_command_batch). x null means absent: every other launch passes that, and the kernel then makes no
// memory access it did not make before.
constexpr int GEO_PAR_WORDS = 16;                    // floats of one parameter row: kp[3], kv[3], amax, inv_tau, g, kT, k0, c_lo, c_hi, 3 unused
struct LoopBaseline {
    const float* x;             // [B][13] the state each command is formed from; null: not the baseline form
    const float* xref;          // the window of episode b at xref + b * xref_ep_stride, rows of 13 floats
    int xref_ep_stride;         // (H + 1) * 13, or 0 (one window for every episode)
    const float* par;           // the parameter row of episode b at par + b * par_ep_stride
    int par_ep_stride;          // GEO_PAR_WORDS, or 0 (one row for every episode: every lane of a wave loads one address)
    int accel_ff;               // 1: feed-forward acceleration from the velocities of rows ref_row, ref_row + 1 (wave-uniform)
    int ref_row;                // 0 .. H - 1
    float inv_dt;               // float32(1) / float32(time_steps[ref_row])
    int H, m;
    float* uopt;                // [B][H][m]
    float* xevol;               // [B][H+1][13]
    float* info;                // [B][8]
    const float* step;          // [B] the step size handed through
    float* out;                 // [B][4] (c, omega*), or null: the tables above
    const int32_t* live;        // SPEC.md §11n: [B], where live[b] == 0 only the info row is written and the tables stay; null: every episode (not one access more)
};
// SPEC.md §11m, per-row ensemble histories over the episodes, by cohort: TWO further forms of the period's key-schedule kernel (ticks = 0, every other struct empty,
// null key buffers), launched after a chunk's scoring launch on rows, targets and thresholds that launch read (sdempc_ensemble.inc.h). The PARTIAL form (combine 0)
// runs on a grid of (blocks of 256 consecutive episodes) x nrows and writes part[i][k][g][W]; the COMBINE form (combine 1) runs one thread per (row, cohort, word),
// walks the blocks in ascending order and writes out[i][g][W]. W = ENS_BASE_WORDS + 4 E words (the table at sdempc_ensemble_cfg, include/sdempc.h). Both forms
// branch off before the kernel's `b >= B` return: the partial form has workgroup barriers and masks instead. part null means absent: every other launch passes
// that, and the kernel then makes no memory access it did not make before.
constexpr int ENS_MAX_COHORTS = 16, ENS_MAX_EDGES = 16, ENS_BASE_WORDS = 20, ENS_MAX_WORDS = ENS_BASE_WORDS + 4 * ENS_MAX_EDGES;
struct LoopEnsemble {
    uint32_t* part;             // [nrows][nblk][G][W] per-block partial words; null: neither form
    uint32_t* out;              // [nrows][G][W] the combined words (combine form)
    const uint32_t* words;      // [B][16] the score words AFTER the chunk's scoring launch (words 0 and 8 are read)
    const int32_t* cohort;      // [B] cohort of each episode, in [0, G)
    const float* edges;         // [4][E] ascending edges of the channels dp, dv, c, w2 (not read with E = 0)
    const float* rows;          // LoopScore::rows of the chunk
    const float* ref;           // LoopScore::ref, with its two strides
    int ref_tick_stride, ref_ep_stride, rows_per_tick;
    int chunk_rows;             // rows the chunk's scoring launch counted: chunk row j has the global index words[b][0] - chunk_rows + j
    int row0, nrows;            // this launch reduces chunk rows row0 .. row0 + nrows - 1
    int nblk;                   // ceil(B / 256)
    int G, E, over;             // cohorts 1 .. 16, edges per channel 0 .. 16, 1: only episodes that have not failed before the row are included
    int combine;                // 0: the partial form, 1: the combine form (wave-uniform)
    float r2_pos, cos_min, w2_max;      // LoopScore's
    const uint32_t* count;      // SPEC.md §11n: [B] rows of episode b up to the end of the chunk, read in place of word 0 (which a retired episode froze); null: word 0
};
// SPEC.md §11n, retiring failed episodes: TWO further forms of the period's key-schedule kernel (ticks = 0, every other struct empty, null key buffers), launched
// after a period's scoring launch, one thread per episode on a grid of ceil(B / 256) blocks (sdempc_retire.inc.h). The COUNT form (place 0) updates live[b] from
// word 8 of the episode's score words, stamps retired_at where an episode leaves the live set, and writes the block's live count to blk[k]; the PLACE form (place 1)
// writes the ascending list of live episodes and n_live. Both branch off before the kernel's `b >= B` return (a workgroup barrier; threads past B are masked).
// live null means absent: every other launch passes that, and the kernel then makes no memory access it did not make before.
struct LoopRetire {
    int32_t* live;              // [B] 1: still solved and scored; null: neither form
    const uint32_t* words;      // [B][16] the score words after the period's scoring launch (word 8 is read; word 0 with init and count)
    int32_t* retired_at;        // [B] the call's first solve the episode is left out of, -1: none
    uint32_t* blk;              // [nblk] live episodes of each block of 256
    int32_t* list;              // [B] the live episodes, ascending; entries past n_live are not written
    int32_t* n_live;            // [1]
    uint32_t* count;            // [B] scored-or-not rows of each episode so far (LoopEnsemble::count), or null
    int solve;                  // what retired_at takes: the index of the call's next solve, or -1 when this was its last period
    int rows;                   // rows of the period just scored, added to count
    int nblk;                   // ceil(B / 256)
    int place;                  // 0: the count form, 1: the place form (wave-uniform)
    int init;                   // 1 (count form): the call's entry — live from word 8 alone, retired_at = -1 or 0, count = word 0
};
hipError_t launch_loop_keys_period(uint32_t* keys_dev, uint32_t* sub_dev, float* xi_dev, int B, int ticks, int xi_ticks, int substeps, hipStream_t st,
                                   const LoopObserve& O = LoopObserve{}, const LoopScore& Z = LoopScore{}, const LoopProcess& G = LoopProcess{},
                                   const LoopEvents& E = LoopEvents{}, const LoopBaseline& A = LoopBaseline{}, const LoopEnsemble& N = LoopEnsemble{},
                                   const LoopRetire& Y = LoopRetire{});
// SPEC.md §11j, reference windows and score targets cut from a trajectory on the device: the row-filling launch below in its TRACKING form. The tables of a set lie
// end to end: table j owns knots first[j] .. first[j] + knots[j] - 1 of t / w / x (w[i] = float32(1 / (t[i+1] - t[i])) formed by the library in float64; the last w of
// a table is not read). Thread i of the launch writes one whole row of 13 floats, row i of out f32[groups][B][rows][13]: group g is tick tick0 + g, its clock value
// theta = float32(tick) * dt, and row r of episode b is the trajectory of table_of[b] at u = theta + c[r], through (phase, rate, offset) of b. A reference window is
// rows = H + 1 of ONE group; the score targets of a chunk are rows = 1 (c[0] = 0) of one group per tick, tick0 the chunk's first tick + 1.
// t null means absent: the launch then copies rows as it always did and makes no memory access it did not make before.
struct LoopTrack {
    const float* t;             // [sum L] knot times, table after table; null: no trajectory
    const float* w;             // [sum L] reciprocal segment lengths
    const float* x;             // [sum L][13] knot states, in the solver's frame
    const int32_t* first;       // [n_tables] index of each table's first knot
    const int32_t* knots;       // [n_tables] L >= 1 of each table
    const float* period;        // [n_tables] 0: clamp at the ends; > 0: wrap (t[0] = 0 and t[L-1] = period)
    const float* inv_period;    // [n_tables] float32(1 / float64(period)), 0 where the period is 0
    const float* c;             // [rows] clock offsets of the rows: c[0] = 0, c[i] = float32(float64 sum of time_steps[0 .. i-1])
    const int32_t* table_of;    // [B] table of each episode
    const float* phase;         // [B]
    const float* rate;          // [B] >= 0
    const float* offset;        // [B][3]
    float dt;                   // float32(time_steps[0])
    int tick0;                  // global tick of group 0 (tick0 + groups - 1 < 2^24)
    int B, rows, groups;
    int renorm;                 // 1: scale the attitude of every row to unit length, software rsqrt (wave-uniform)
};
// SPEC.md §11n, the dense solve of the live set: the row-filling launch in its GATHER form (scatter 0: row list[i] of every segment's src to row i of its dst) and
// its SCATTER form (scatter 1: row i to row list[i]), bit copies of `words` 4-byte words per row (sdempc_retire.inc.h). The scatter form also writes the held info
// row (0, held_step[b], 0 ..) of every episode with live[b] == 0 and sets *gave_up where word 1 of a dense instance's cooperative barrier is set (coop_bar null:
// the solve took no cooperative layout). list null means absent: every other launch passes that, and the kernel then makes no memory access it did not make before.
constexpr int COMPACT_SEGS = 5;
struct LoopCompact {
    const int32_t* list;        // [n] live episodes, ascending; null: neither form
    int n, B, i0;               // dense rows, episodes, first dense row of this launch (set by the launcher)
    int scatter, nseg;
    struct Seg { const uint32_t* src; uint32_t* dst; int words; int vec; } seg[COMPACT_SEGS];    // vec is set by the launcher: 16-byte copies
    const int32_t* live;        // [B] (scatter form)
    float* held_info;           // [B][8] the solve's info rows (scatter form)
    const float* held_step;     // [B] the current step sizes (scatter form)
    const unsigned* coop_bar;   // [n][COOP_BAR_WORDS] of the dense solve, or null
    unsigned* gave_up;          // the loop's sticky flag
};
// rows_dev[b][0..n) = row_dev[0..n) for b < B; or, with K.t given (row_dev, n and B are then not read): rows_dev[g][b][r][0..13) from the trajectory set K;
// or, with Q.list given (nothing else is read): the gather or scatter form
hipError_t launch_broadcast_rows(const float* row_dev, float* rows_dev, int n, int B, hipStream_t st, const LoopTrack& K = LoopTrack{}, const LoopCompact& Q = LoopCompact{});
// canonical [B][P][C] <-> device [B][G][C][32] (to_dev: zero-pads particles >= P)
hipError_t launch_relayout(bool to_dev, const float* in, float* out, int B, int P, int G, int C, hipStream_t st);
// SPEC.md §7: noise of B instances from their threefry keys (device u32[B][2]) straight into the device layout [B][G][H][6][32]
hipError_t launch_noise_from_keys(const uint32_t* keys_dev, float* out, int B, int P, int G, int H, hipStream_t st);
// SPEC.md §12, the predicted tube: the noise kernel in its TUBE form (sdempc_tube.inc.h). It reduces the particle x horizon tensor f32[B][G][C][32], C = (H+1)*13, over
// the valid particles of every (instance, column): mean, population variance, extrema and the number of particles outside [lo_i, hi_i] (i = c mod 13), each plane
// [B][C] and each optional. traj null means absent: every noise launch passes that, and the kernel then makes no memory access it did not make before.
struct TubeArgs {
    const float* traj;          // [B][G][C][32] the tensor a store_traj rollout left (KArgs::traj); null: the noise mode
    float* mean;                // [B][C] or null
    float* var;                 // [B][C] or null
    float* mn;                  // [B][C] or null
    float* mx;                  // [B][C] or null
    uint32_t* outside;          // [B][C] or null: no bounds (lo / hi are then not read)
    float lo[13], hi[13];       // bounds per state component, -inf / +inf: none (wave-uniform kernel arguments, read at constant indices)
    float invP;                 // float32(1) / float32(P), as KArgs::invP
    int C;                      // columns per instance
};
hipError_t launch_tube(const TubeArgs& T, int B, int P, int G, int H, hipStream_t st);
// SPEC.md §12a, predicted risk: the noise kernel in its RISK form (sdempc_risk.inc.h), one workgroup per instance. It walks the same tensor particle by particle:
// first exit from the per-instance box [lo, hi] around the centre rows, the tracking cost Jx_p, and per instance the exit histogram, the per-step outside count,
// mean / variance / extrema, order statistics and the tail mean of Jx. Every output is optional. traj null means absent: every noise and tube launch passes that,
// and the kernel then makes no memory access it did not make before.
constexpr int RISK_MAX_RANKS = 8;
constexpr int RISK_RANK_MAX_P = 4096;   // the selection stage counts P particles per particle: the rank outputs (jq, jtail) are refused above this
constexpr size_t RISK_MAX_LDS = 64 * 1024;
// 4-byte words of workgroup memory of the risk form: any[H+1] hist[H+2] jx[G*32], five group arrays [G] and the instance's box [26] (sdempc_risk.inc.h)
inline size_t risk_lds_words_host(int H, int G) { return (size_t)(2 * H + 3) + (size_t)G * 37 + 26; }
struct RiskArgs {
    const float* traj;          // [B][G][C][32], C = (H+1)*13 (KArgs::traj); null: not the risk mode
    const float* xref;          // [B][H+1][13]; needed for Jx
    const float* centre;        // [B][H+1][13] or null: e = x
    const float* lo;            // [B][13] or null: no exit outputs (hi is then not read)
    const float* hi;            // [B][13]
    const float* disc;          // [H+1] (KArgs::disc)
    const CostK::StateBound* sc_tab;
    uint32_t* exit;             // [B][P] or null
    float* jx;                  // [B][P] or null
    uint32_t* first_exit;       // [B][H+2] or null
    uint32_t* outside_any;      // [B][H+1] or null
    float* jstat;               // [B][4] or null
    float* jq;                  // [B][n_ranks] or null
    float* jtail;               // [B] or null
    float perr[3], verr[3], qerr[3], werr[3];   // CostK's
    float invP, inv_tail;       // float32(1) / float32(P), float32(1) / float32(tail_k)
    int H, sc_n, tail_k, n_ranks;
    int ranks[RISK_MAX_RANKS];
};
hipError_t launch_risk(const RiskArgs& R, int B, int P, int G, hipStream_t st);
// SPEC.md §12b, predicted bands: the noise kernel in its BANDS form (sdempc_band.inc.h), on the tube's grid. Per (instance, column) of the same tensor, over the valid
// particles in the total key order: the values at n_ranks requested ranks (q, plane k = rank ranks[k]) and the number of particles below / at the observed word of
// that column. Every output is optional. traj null means absent: every noise, tube and risk launch passes that, and the kernel then makes no memory access it did
// not make before.
constexpr int BAND_MAX_RANKS = 8;
struct BandArgs {
    const float* traj;          // [B][G][C][32], C = (H+1)*13 (KArgs::traj); null: not the bands mode
    const float* obs;           // [B][C] observed rows, or null: below / at are then not written
    float* q;                   // [B][n_ranks][C] or null (n_ranks / ranks are then not read)
    uint32_t* below;            // [B][C] or null
    uint32_t* at;               // [B][C] or null
    int C;                      // columns per instance
    int n_ranks;                // 1 .. BAND_MAX_RANKS
    int ranks[BAND_MAX_RANKS];  // each in [0, P); neither sorted nor distinct (wave-uniform kernel arguments, read at constant indices)
};
hipError_t launch_bands(const BandArgs& N, int B, int P, int G, int H, hipStream_t st);
// SPEC.md §12c, predicted outcome: the noise kernel in its OUTCOME form (sdempc_outcome.inc.h), one workgroup per instance. Every particle of the same tensor is
// scored as §11h scores an episode — rows x_1 .. x_H against the target rows, the channels dp, dv, c, w2, the cause bits — and the words and channels are reduced
// over the valid particles. Every output is optional. traj null means absent: every noise, tube, risk and bands launch passes that, and the kernel then makes no
// memory access it did not make before.
constexpr int OUTCOME_MAX_RANKS = 8;
constexpr int OUTCOME_WORDS = 11;        // words 0 .. 10 of the §11h table
constexpr int OUTCOME_RANK_MAX_P = 128;  // the selection is the in-register sort over four groups: the order statistics (chan_q, agg_q) are refused above this
// 4-byte words of workgroup memory of the outcome form: fail[5 H] hist[H+1] cause[4] gs[G][12] val[G*32][4] (sdempc_outcome.inc.h); capped by RISK_MAX_LDS
inline size_t outcome_lds_words_host(int H, int G) { return (size_t)(6 * H + 5) + (size_t)G * 140; }
struct OutcomeArgs {
    const float* traj;          // [B][G][C][32], C = (H+1)*13 (KArgs::traj); null: not the outcome mode
    const float* tgt;           // target rows: row t of instance b is tgt + b * tgt_bstride + t * tgt_tstride (13 floats; 6 are read)
    uint32_t* words;            // [B][P][11] or null
    uint32_t* fail_step;        // [B][H][5] or null
    uint32_t* first_fail;       // [B][H+1] or null
    uint32_t* cause_ever;       // [B][4] or null
    float* chan_stat;           // [B][H][4][3] or null
    float* chan_q;              // [B][H][4][n_ranks] or null
    float* agg_stat;            // [B][4][3] or null
    float* agg_q;               // [B][4][n_ranks] or null
    float r2_pos, cos_min, w2_max, invP;
    int tgt_bstride, tgt_tstride;   // floats; 0 on a size-1 axis
    int H;
    int n_ranks;                // 1 .. OUTCOME_MAX_RANKS where chan_q or agg_q is given
    int ranks[OUTCOME_MAX_RANKS];   // each in [0, P); neither sorted nor distinct
};
hipError_t launch_outcome(const OutcomeArgs& W, int B, int P, int G, hipStream_t st);

}  // namespace sdempc
