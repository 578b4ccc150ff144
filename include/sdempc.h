/*
 * sdempc.h — C ABI of the MI355X-native MPC inner loop (neural-SDE rollout + APG trajectory optimiser).
 *
 * This is the drop-in boundary for ONE path of wuwushrek/sde4mbrl_px4: the solver that
 * `sde4mbrl_px4/mpc_controller/sde_control.py` obtains from
 * `load_mpc_from_cfgfile(mpc_dir, convert_to_enu=True)` (sde_control.py:685) and calls per control
 * tick as `m_reset(x=, rng=, xdes=)` (sde_control.py:345-346,389-394,706) and
 * `m_mpc(x, rng, opt_state, curr_t=, xdes=)` (sde_control.py:349-350,400-416,717).
 * The reference has no C interface for this path (the arithmetic lives in the un-vendored JAX package
 * sde4mbrl); this header is what a ctypes binding on the reference side binds.
 *
 * Conventions
 *   - plain pointers + sizes, no C++ / torch types; every entry point returns 0 on success or a
 *     negative SDEMPC_E* code, never aborts or throws (an exception would silently kill the
 *     reference's `mpc_process`, sde_control.py:365-419 has no try/except).
 *   - state vector f32[13] = [x,y,z, vx,vy,vz, qw,qx,qy,qz, wx,wy,wz] (sde_control.py:246,747).
 *   - "host" entry points take host pointers (caller owns them) and stage through device buffers
 *     owned by the handle; "_dev" entry points take device pointers already resident in HBM and a
 *     hipStream_t passed as void*.
 *   - canonical tensor layouts (row-major, innermost last):
 *       x0    f32[B][13]            initial states
 *       u     f32[B][H][m]          control sequences (normalised PWM)
 *       xref  f32[B][H+1][13]       reference states at t_0..t_H
 *       noise f32[B][P][H][6]       N(0,1) draws for the 6 noisy state dims (v, omega)
 *       traj  f32[B][P][H+1][13]    particle x horizon tensor
 *       uopt  f32[B][H][m], xevol f32[B][H+1][13] (particle mean), info f32[B][8]
 *   - a handle is single-threaded; the HIP context is created lazily on the first call that needs
 *     the device, in the calling process (safe to create the handle before fork()).
 */
#ifndef SDEMPC_H
#define SDEMPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's struct layouts and entry points; sdempc_abi_version() returns the one the library was built with. A binding
 * compares the two before it passes a struct (2: sdempc_cfg grew the state_constr fields, handle options, work counters; 3: sdempc_plant_cfg and
 * sdempc_closed_loop_batch_plant). */
#define SDEMPC_ABI_VERSION 3

#define SDEMPC_NX 13          /* state dims */
#define SDEMPC_NNOISE 6       /* noisy state dims: v(3), omega(3) */
#define SDEMPC_MAX_MOTORS 8
#define SDEMPC_HID 32         /* hidden width of the residual / density MLPs */
#define SDEMPC_BLOB_MAGIC 0x31454453 /* "SDE1" */
#define SDEMPC_BLOB_HEADER_INTS 16
#define SDEMPC_BLOB_FLOATS 2120

/* error codes */
#define SDEMPC_OK 0
#define SDEMPC_EINVAL (-1)    /* bad argument / config */
#define SDEMPC_EBLOB (-2)     /* malformed model blob */
#define SDEMPC_EDEVICE (-3)   /* HIP error (message in sdempc_last_error) */
#define SDEMPC_ENOMEM (-4)
#define SDEMPC_ECAPACITY (-5) /* batch larger than max_batch given at create */

/* Hyper-parameters: one-to-one with the reference's MPC YAML schema
 * (launch/iris_sitl_traj_mpc.yaml:8-85, launch/iris_sitl_posctrl_mpc.yaml:6-101). */
typedef struct sdempc_cfg {
    int32_t struct_size;              /* sizeof(sdempc_cfg), ABI check */
    int32_t horizon;                  /* H            (yaml: horizon) */
    int32_t num_particles;            /* P            (yaml: num_particles) */
    int32_t num_motors;               /* m            (len(input_constr.input_id)) */
    const float* time_steps;          /* [H] dt per step (yaml: num_short_dt/short_step_dt/long_step_dt) */
    float discount;                   /* yaml: discount */
    /* cost_params */
    float uref[SDEMPC_MAX_MOTORS];
    float uerr;
    float perr[3], verr[3], qerr[3], werr[3];
    float res_mult;
    float u_slew_coeff;
    int32_t has_slew_constr;          /* 1 if cost_params.u_slew_constr present */
    float u_slew_lo[SDEMPC_MAX_MOTORS], u_slew_hi[SDEMPC_MAX_MOTORS];
    float u_slew_constr_coeff;
    /* input_constr.input_bound (enforce_ubound) */
    float u_lo[SDEMPC_MAX_MOTORS], u_hi[SDEMPC_MAX_MOTORS];
    /* apg_mpc */
    int32_t max_iter;
    int32_t max_no_improvement_iter;
    int32_t use_moment_scale;         /* 0: yaml moment_scale null */
    float moment_scale;
    float beta_init;
    float atol, rtol;
    float stepsize;                   /* used when ls_maxls == 0 */
    float ls_init_stepsize, ls_max_stepsize, ls_coef, ls_decrease_factor, ls_increase_factor;
    int32_t ls_reset_option;          /* 0 conservative, 1 increase */
    int32_t ls_maxls;
    /* extension (not a reference YAML key): arithmetic of the MLP contractions. All three are reproduced bit for bit by the CPU oracle.
     * 0 = f32 fma chains (v_mfma_f32_32x32x2_f32; default);
     * 1 = fp16 operands rounded toward zero, f32 accumulate, in the forward rollout (v_mfma_f32_32x32x16_f16; BASELINE config C5; SPEC.md §9);
     * 2 = f32x3: f32 operands, the two 32x32 contractions of a step (layer 2 of the drift net and its transpose in the adjoint) evaluated as
     *     three-limb bf16 splits of both operands on v_mfma_f32_32x32x16_bf16 — f32-level accuracy on the matrix pipe (SPEC.md §9b). */
    int32_t mlp_dtype;
    /* extension (not a reference YAML key): 0 = exact (default): tanh / sigmoid / reciprocal square root in the bit-reproducible
     * software forms of SPEC.md §3, results identical to the CPU oracle bit for bit. 1 = fast: the same kernels with the
     * hardware transcendentals (v_exp_f32, v_rcp_f32, v_rsq_f32) and the hidden activation kept as 1 / (1 + 2^a') with its affine maps folded into the
     * weights by sdempc_create (SPEC.md §10, §10b); about 1e-7 relative per operation away from the exact path, and — through the oracle's model of the three
     * instructions (SPEC.md §10a) — compared with the CPU oracle bit for bit as well. With mlp_dtype 1 or 2 the mode rescales the rows of W3 by exact
     * powers of two (compensated in the residual scales: the same model) when they lie outside [2^-4, 2^2), and REFUSES (SDEMPC_EINVAL from sdempc_create
     * and from a call that prepares a plant) a model its binary16 limbs cannot carry: a limb operand weight beyond 65504, eoff < 8, 0 < C2 < 2^-6, a row
     * rescale that would round (SPEC.md §10e, "What the mode accepts"). */
    int32_t math_mode;
    /* state_constr (launch/iris_sitl_traj_mpc.yaml:16-29; commented out in every YAML the reference ships), penalty form
     * (slack_proximal: False): stage cost += sum_k state_w[k] * (max(0, x[id_k] - hi_k)^2 + max(0, lo_k - x[id_k])^2) at x_{t+1},
     * state_w = state_penalty * constr_pen (host float32), ids strictly ascending, in the solver's frame. SPEC.md §5.3. */
    int32_t num_state_constr;         /* 0: none */
    int32_t state_id[SDEMPC_NX];
    float state_w[SDEMPC_NX], state_lo[SDEMPC_NX], state_hi[SDEMPC_NX];
} sdempc_cfg;

/* Optimiser telemetry: the 7 scalars the reference reads from opt_state
 * (sde_control.py:444-450, msg/OptMPCState.msg:6-22) + the line-search trial count. */
typedef struct sdempc_info {
    float avg_linesearch;
    float stepsize;
    float num_steps;
    float grad_sqr;
    float avg_stepsize;
    float init_cost;
    float opt_cost;
    float num_ls_trials;              /* total trial rollouts N_ls (for the roofline accounting) */
} sdempc_info;

typedef struct sdempc_handle sdempc_handle;

/* ---- lifetime ----------------------------------------------------------------------------- */
/* Replaces: construction inside load_mpc_from_cfgfile (sde_control.py:685). Host-only; no HIP call. */
int sdempc_create(const sdempc_cfg* cfg, const void* model_blob, size_t blob_bytes,
                  int32_t max_batch, sdempc_handle** out);
void sdempc_destroy(sdempc_handle* h);
const char* sdempc_last_error(const sdempc_handle* h);   /* h may be NULL: last create error */
int sdempc_abi_version(void);
/* What the library was built with (no reference counterpart). Bit 0 (SDEMPC_BUILD_ALL_VARIANTS): the build carries every kernel instantiation
 * (`make EXTRA=-DSDEMPC_ALL_VARIANTS=1`): the generic motor count (m other than 4 / 6) in the duo / six-team / cooperative / speculative layouts
 * too, and the packed-tanh instantiations behind SDEMPC_OPT_PK = 1. The default build runs a generic motor count in the one-group-per-wave tile
 * layouts (and P = 1 in the lane layout) and refuses SDEMPC_OPT_PK = 1; results never depend on the layout. */
#define SDEMPC_BUILD_ALL_VARIANTS 1
int sdempc_build_flags(void);

/* Binds the handle to a HIP device ordinal (default 0). Must precede the first device call. */
int sdempc_set_device(sdempc_handle* h, int32_t device);

/* 1 once the handle has initialised the GPU (first device call), else 0. Host-only, no HIP call: lets the caller of a forked
 * process (the reference forks mpc_process after building its solvers, sde_control.py:69-75,723-728) tell a handle that is safe
 * to use from one whose HIP state belongs to the parent and must be abandoned without sdempc_destroy. */
int sdempc_device_ready(const sdempc_handle* h);

/* ---- execution options (per handle) ---------------------------------------------------------
 * How a call is laid out on the GPU; none of them changes a bit of any result. No reference counterpart (the reference's
 * solver objects, sde_control.py:681-721, have no such knobs). The environment variables named below only give the DEFAULT of
 * a handle created afterwards (read once inside sdempc_create); nothing on the launch path reads the environment.
 *   key                       values                         default  environment default
 *   SDEMPC_OPT_LANE           0 / 1                          1        SDEMPC_LANE          P == 1 instances in the single-particle lane layout
 *   SDEMPC_OPT_COOP           0 / 1                          1        SDEMPC_COOP          small batches spread over many workgroups (latency layouts);
 *                                                                                          setting 1 also re-arms a handle that fell back (sdempc_layout_fallbacks)
 *   SDEMPC_OPT_SPEC           0 / 1                          1        SDEMPC_SPEC          speculative variant of the cooperative layout (smallest batches)
 *   SDEMPC_OPT_PK             -1 auto / 0 / 1                -1       SDEMPC_PK            packed-f32 tanh instantiation of the tile layout (auto: grid <= CUs)
 *   SDEMPC_OPT_USTG           -1 auto / 0 / 1                -1       SDEMPC_USTG          per-step control table in global memory instead of LDS (auto: long horizons)
 *   SDEMPC_OPT_DUO            -1 auto / 0 / 1                -1       SDEMPC_DUO           throughput launches: 64 particles per wave (two 32-particle groups; auto = on for P > 32)
 *   SDEMPC_OPT_HEX            0 / 1                          1        SDEMPC_HEX           launches that fill every two-wave team slot of the device: one six-team
 *                                                                                          workgroup per CU (weights staged once per CU) instead of three two-team ones
 *   SDEMPC_OPT_COOP_LAUNCH    0 / 1                          0        SDEMPC_COOP_LAUNCH   hipLaunchCooperativeKernel for the cooperative layouts
 *   SDEMPC_OPT_COOP_FENCE     0 / 1                          0        SDEMPC_COOP_FENCE    agent-scope release / acquire fences around the grid barrier and the arrival counter
 *   SDEMPC_OPT_COOP_SPIN_US   -1 derived / >= 0 microseconds -1       SDEMPC_COOP_SPIN_US  how long one grid barrier / polled hand-off of a cooperative layout may wait
 *                                                                                          before the launch gives up (derived: 5 x the handle's last completed
 *                                                                                          cooperative solve, clamped to 2..100 ms; 100 ms before the first)
 *   SDEMPC_OPT_TEST_ABSENT_WG -1 none / >= 0 workgroup index -1       (none)               FAULT INJECTION for the tests of the bounded waits: that workgroup of a
 *                                                                                          cooperative-layout grid leaves at once, as a workgroup that never became
 *                                                                                          resident would; the launch then gives up within its spin budget
 *   SDEMPC_OPT_TEST_WS_FILL   -1 none / 0..255 byte value    -1       (none)               POISON for the tests of handle state: every float-valued device buffer the handle
 *                                                                                          allocates from then on (set it before the first device call to reach all of them)
 *                                                                                          is filled with that byte right after its hipMalloc, complete before the call goes
 *                                                                                          on to its launches; 255 makes every word a NaN pattern. Results do not change:
 *                                                                                          no kernel may read a word of these buffers that the same call has not written.
 *                                                                                          Filled: the workspaces (particle x horizon tensor, activation checkpoint,
 *                                                                                          partial sums, control table), the cooperative layouts' per-particle outputs and
 *                                                                                          checkpoint rows, the noise buffers, the staging copies of inputs and outputs (the tube planes of
 *                                                                                          sdempc_tube_batch, d_tube, the band planes of sdempc_bands_batch, d_band, the risk rows of sdempc_risk_batch, d_risk, and the outcome rows of sdempc_outcome_batch, d_outcome, among them),
 *                                                                                          the closed loop's key / chunk / plant / rate-state / observation / history buffers (the chunk buffer includes the
 *                                                                                          staged disturbance rows and plant-schedule rows of a scenario). (The particle x horizon tensor is
 *                                                                                          zeroed at allocation otherwise; nothing depends on that.) Keep their initial value:
 *                                                                                          - the work counters and the ticket word: running totals, zero at creation by
 *                                                                                            definition (sdempc_work_counters, sdempc_solve_status compare against them);
 *                                                                                          - the grid-barrier words of the cooperative layouts: arrival counters and the
 *                                                                                            give-up flag, integers zeroed on the stream ahead of every launch — a poisoned
 *                                                                                            flag could not be told from a barrier that gave up;
 *                                                                                          - the tags of the tagged hand-off words inside the per-particle outputs: the
 *                                                                                            buffer is filled at allocation, but its per-launch clear (by the host for the
 *                                                                                            speculative layout, by the kernel's first workgroup for the plain cooperative
 *                                                                                            one) stays, and comes after the fill: a tag is a flag, not data;
 *                                                                                          - tables and key buffers copied whole from the host before their first use.
 *   SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES -1 built-in / >= 0 bytes  -1     (none)               TEST AID for the chunk boundaries of the closed loop: device bytes the per-tick buffers
 *                                                                                          of one chunk may take (-1: the built-in 256 MiB). A chunk always holds at least one
 *                                                                                          solve period, so 0 or 1 cuts a run into one chunk per period. Results do not change.
 *   SDEMPC_OPT_DEVICE_CUS     read-only                                                    compute units of the handle's device (after the first device call)
 */
#define SDEMPC_OPT_LANE 1
#define SDEMPC_OPT_COOP 2
#define SDEMPC_OPT_SPEC 3
#define SDEMPC_OPT_PK 4
#define SDEMPC_OPT_USTG 5
#define SDEMPC_OPT_COOP_LAUNCH 6
#define SDEMPC_OPT_COOP_FENCE 7
#define SDEMPC_OPT_COOP_SPIN_US 8
#define SDEMPC_OPT_DEVICE_CUS 9
#define SDEMPC_OPT_DUO 10
#define SDEMPC_OPT_HEX 11
#define SDEMPC_OPT_TEST_ABSENT_WG 12
#define SDEMPC_OPT_TEST_WS_FILL 13
#define SDEMPC_OPT_TEST_LOOP_CHUNK_BYTES 14
int sdempc_set_option(sdempc_handle* h, int32_t key, int32_t value);
int sdempc_get_option(const sdempc_handle* h, int32_t key, int32_t* value);

/* ---- m_reset (sde_control.py:702-707,345-346,389-394) -------------------------------------- */
/* Host-only. Fills yk[H][m] with the hover guess uref and info with the initial telemetry. */
int sdempc_reset(sdempc_handle* h, const float* x, const float* xdes, float* yk, sdempc_info* info);

/* ---- hot-path pieces, batched, host pointers ----------------------- */
/* A4+A5: Euler–Maruyama rollout + expected cost. traj/xmean may be NULL. */
int sdempc_rollout_batch(sdempc_handle* h, int32_t B, const float* x0, const float* u,
                         const float* xref, const float* noise,
                         float* cost /*[B]*/, float* traj /*[B][P][H+1][13] or NULL*/,
                         float* xmean /*[B][H+1][13] or NULL*/);
/* A6 (gradient): cost and d cost / d u by the adjoint pass. */
int sdempc_grad_batch(sdempc_handle* h, int32_t B, const float* x0, const float* u,
                      const float* xref, const float* noise,
                      float* cost /*[B]*/, float* grad /*[B][H][m]*/);
/* A3: the solve. u_init = warm start (opt_state.yk), stepsize_in = opt_state.stepsize.
 * Execution layout is chosen per call and never changes a bit of the result: P = 1 instances (all YAMLs the reference ships) run in a
 * single-particle layout; batches small enough that all workgroups are resident at once (C2: up to 15 instances) are spread over many
 * workgroups, one particle per wave, with one bounded grid barrier per rollout, and for the smallest batches additionally evaluate up to three
 * line-search trials and the candidate gradients of the next iteration at once, handing the per-particle outputs over as tagged words that the
 * workgroups poll (bounded like the barrier) instead of through a barrier (C2 single solve: 20 ms instead of 158 ms); larger
 * batches run one workgroup per instance in the 32-particle MFMA tile layout (throughput). The cooperative layouts assume that no other
 * kernel occupies the GPU while they run; if their workgroups cannot all become resident the barrier gives up after a bounded time
 * (SDEMPC_OPT_COOP_SPIN_US) and the telemetry of the launch is NaN. The host-pointer entry points then run the same batch once more in the
 * one-workgroup-per-instance layout (identical results) and the handle stays off the cooperative layouts from then on
 * (sdempc_layout_fallbacks counts these events); callers of sdempc_solve_batch_dev ask sdempc_solve_status. */
int sdempc_solve_batch(sdempc_handle* h, int32_t B, const float* x0, const float* xref,
                       const float* noise, const float* u_init /*[B][H][m]*/,
                       const float* stepsize_in /*[B]*/,
                       float* uopt /*[B][H][m]*/, float* xevol /*[B][H+1][13]*/,
                       sdempc_info* info /*[B]*/);

/* ---- device-resident variants (benchmarks, multi-instance serving) -------------------------- */
/* noise_dev uses the device layout produced by sdempc_noise_to_device_layout / _dev:
 *   f32[B][G][H][6][32] with G = ceil(P/32), particle p -> (g = p/32, lane = p%32). */
size_t sdempc_noise_dev_floats(const sdempc_handle* h, int32_t B);
size_t sdempc_traj_dev_floats(const sdempc_handle* h, int32_t B);
int sdempc_noise_to_device_layout(const sdempc_handle* h, int32_t B, const float* noise_host, float* out_host);
/* The same conversion on the device: canonical f32[B][P][H][6] at noise_canonical_dev -> device layout at
 * noise_out_dev (sdempc_noise_dev_floats(h, B) floats; padded particles are written as zeros). */
int sdempc_noise_to_device_layout_dev(sdempc_handle* h, int32_t B, const void* noise_canonical_dev,
                                      void* noise_out_dev, void* stream);
/* Copies the particle x horizon tensor that the last sdempc_rollout_batch_dev(store_traj=1)
 * or sdempc_grad_batch_dev of the first B instances left in the handle to traj_out_dev as canonical
 * f32[B][P][H+1][13]. Enqueue it on the stream of that call. */
int sdempc_traj_to_canonical_dev(sdempc_handle* h, int32_t B, void* traj_out_dev, void* stream);
int sdempc_solve_batch_dev(sdempc_handle* h, int32_t B, const void* x0_dev, const void* xref_dev,
                           const void* noise_dev, const void* u_init_dev, const void* stepsize_dev,
                           void* uopt_dev, void* xevol_dev, void* info_dev /*f32[B][8]*/,
                           void* stream);
int sdempc_rollout_batch_dev(sdempc_handle* h, int32_t B, const void* x0_dev, const void* u_dev,
                             const void* xref_dev, const void* noise_dev, void* cost_dev,
                             void* xmean_dev /*or NULL*/, int32_t store_traj, void* stream);
int sdempc_grad_batch_dev(sdempc_handle* h, int32_t B, const void* x0_dev, const void* u_dev,
                          const void* xref_dev, const void* noise_dev, void* cost_dev,
                          void* grad_dev, void* stream);

/* ---- key-derived noise (SPEC.md §7) ---------------------------------------------------------- */
/* The reference threads a JAX PRNG key through every solver call: jax.random.PRNGKey(seed) and its 3-way split
 * (sde_control.py:338-341), `rng` in and out of m_reset / m_mpc (sde_control.py:345-350,400-416,698,706,717). A key is
 * uint32[2] with JAX's threefry2x32 conventions (PRNGKey(seed) = {seed >> 32, seed & 0xffffffff}; the host-side split lives in
 * sde4mbrl_px4_amd/prng.py). These entry points draw the noise tensor of instance b as normal(keys[b], (P, H, 6)) on the
 * device, so only 8 bytes per instance cross the boundary. keys is a HOST pointer, u32[B][2], in all three. */
int sdempc_noise_from_keys_dev(sdempc_handle* h, int32_t B, const uint32_t* keys, void* noise_out_dev /* device layout,
                               sdempc_noise_dev_floats(h, B) floats */, void* stream);
int sdempc_noise_from_keys(sdempc_handle* h, int32_t B, const uint32_t* keys, float* noise /* host, canonical [B][P][H][6] */);
/* A3 with key-derived noise: what m_mpc(x, rng, opt_state, ...) maps to. */
int sdempc_solve_batch_keys(sdempc_handle* h, int32_t B, const float* x0, const float* xref, const uint32_t* keys,
                            const float* u_init /*[B][H][m]*/, const float* stepsize_in /*[B]*/,
                            float* uopt /*[B][H][m]*/, float* xevol /*[B][H+1][13]*/, sdempc_info* info /*[B]*/);

/* ---- predicted tube (SPEC.md §12) --------------------------------------------------------------
 * The solve rolls out P particles per instance and returns their mean (xevol). These entry points reduce the same particle x horizon tensor where it lies
 * on the device to five planes per instance, each [H+1][13] (column c = t * 13 + i), over the valid particles p < P:
 *   mean     the particle mean — bit for bit the xmean of the same rollout;
 *   var      the population variance about that rounded mean (P = 1: exactly 0);
 *   min, max the extrema (NaN operands ignored; +inf / -inf where every particle is NaN);
 *   outside  uint32: how many particles have !(x >= lo[i] && x <= hi[i]) — a NaN counts — the empirical chance-constraint estimate per step and component
 *            (divide by P on the host). -inf / +inf in lo / hi: no bound on that component.
 * Each plane pointer may be NULL (not computed, not written); at least one must be given, and outside needs cfg. cfg may be NULL otherwise; a NaN bound or a
 * wrong struct_size is SDEMPC_EINVAL. Every argument is checked before the first HIP call. */
typedef struct sdempc_tube_cfg {
    int32_t struct_size;   /* sizeof(sdempc_tube_cfg) */
    float lo[SDEMPC_NX], hi[SDEMPC_NX];
} sdempc_tube_cfg;
/* Reduces the tensor that the last sdempc_rollout_batch_dev(store_traj=1) of at least B instances left in the handle; device pointers, f32[B][H+1][13]
 * (outside_dev: u32). Refused like sdempc_traj_to_canonical_dev when the workspace holds fewer instances: after a gradient evaluation, a solve, a smaller
 * rollout or a workspace reallocation. Enqueue it on the stream of that rollout. */
int sdempc_tube_batch_dev(sdempc_handle* h, const sdempc_tube_cfg* cfg /*or NULL*/, int32_t B, void* mean_dev, void* var_dev, void* min_dev, void* max_dev,
                          void* outside_dev, void* stream);
/* Host pointers: one rollout of u (as sdempc_rollout_batch; cost [B] may be NULL) with the tensor kept, the reduction, the requested planes copied back. */
int sdempc_tube_batch(sdempc_handle* h, const sdempc_tube_cfg* cfg /*or NULL*/, int32_t B, const float* x0, const float* u, const float* xref,
                      const float* noise, float* cost /*[B] or NULL*/, float* mean, float* var, float* min, float* max, uint32_t* outside);
/* The same with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)) (keys: host u32[B][2]), as sdempc_solve_batch_keys does: with the
 * uopt and the keys of a solve, mean is that solve's xevol bit for bit. */
int sdempc_tube_batch_keys(sdempc_handle* h, const sdempc_tube_cfg* cfg /*or NULL*/, int32_t B, const float* x0, const float* u, const float* xref,
                           const uint32_t* keys, float* cost /*[B] or NULL*/, float* mean, float* var, float* min, float* max, uint32_t* outside);

/* ---- predicted risk (SPEC.md §12a) --------------------------------------------------------------
 * Trajectory-level statistics of the same particle x horizon tensor, reduced where it lies on the device. Per instance b the caller gives a box lo[b][13],
 * hi[b][13] (-inf / +inf: no bound on that component; a NaN bound in host memory is SDEMPC_EINVAL) around a per-step centre row c[b][t][13] chosen by
 * cfg->centre_mode: 0 none (the box is absolute), 1 the caller's rows centre[B][H+1][13], 2 the call's xref, 3 the tensor's own particle mean (the mean plane of
 * sdempc_tube_batch, formed first). Particle p is outside at step t iff !(e >= lo_i && e <= hi_i) for some i, e = x - c one float32 subtraction: a NaN is
 * outside, a particle ON a bound inside. Outputs, each optional (NULL: not computed, not written), at least one:
 *   exit        u32[B][P]     first t in 0..H at which p is outside, H+1: never
 *   jx          f32[B][P]     tracking cost Jx_p = sum_t disc[t] * l_x(x_{t+1}^p, xref_{t+1}): the state-error part of the cost (SPEC.md §5.3, state bounds included)
 *   first_exit  u32[B][H+2]   histogram of exit over the particles; bin H+1: never (P(ever leaves) = 1 - first_exit[H+1] / P)
 *   outside_any u32[B][H+1]   particles outside at step t (re-entries make it differ from the cumulative histogram)
 *   jstat       f32[B][4]     mean, population variance about the rounded mean, min, max of jx
 *   jq          f32[B][n_ranks]  jx of rank cfg->ranks[q] (0: smallest) in the total order: numbers by value, a NaN above every number, ties by particle index
 *   jtail       f32[B]        mean of the cfg->tail_k largest jx in that order (CVaR)
 * exit, first_exit and outside_any need lo and hi; jq needs 1 <= n_ranks <= 8 and 0 <= ranks[q] < P; jtail needs 1 <= tail_k <= P; jq and jtail are refused
 * for P > 4096 (the selection stage counts P particles per particle), and every output when 4 (2 H + 29 + 37 ceil(P / 32)) bytes exceed 64 KiB of workgroup
 * memory. Every argument is checked before the first HIP call. */
typedef struct sdempc_risk_cfg {
    int32_t struct_size;   /* sizeof(sdempc_risk_cfg) */
    int32_t centre_mode;   /* 0 none, 1 centre rows, 2 xref, 3 particle mean */
    int32_t tail_k;        /* jtail: number of worst particles */
    int32_t n_ranks;       /* jq: number of ranks */
    int32_t ranks[8];
} sdempc_risk_cfg;
/* Reduces the tensor that the last sdempc_rollout_batch_dev(store_traj=1) of at least B instances left in the handle; device pointers. lo_dev / hi_dev
 * f32[B][13] (NULL: no exit outputs), centre_dev f32[B][H+1][13] (centre_mode 1), xref_dev f32[B][H+1][13] (needed for jx, jstat, jq, jtail and centre_mode 2).
 * Bounds in device memory cannot be inspected: a NaN bound there puts every particle outside. Refused like sdempc_tube_batch_dev when the workspace holds
 * fewer instances. Enqueue it on the stream of that rollout. */
int sdempc_risk_batch_dev(sdempc_handle* h, const sdempc_risk_cfg* cfg, int32_t B, const void* lo_dev, const void* hi_dev, const void* centre_dev, const void* xref_dev,
                          void* exit_dev, void* jx_dev, void* first_exit_dev, void* outside_any_dev, void* jstat_dev, void* jq_dev, void* jtail_dev, void* stream);
/* Host pointers: ONE rollout of u (as sdempc_rollout_batch; cost [B] may be NULL) with the tensor kept, the reduction, the requested outputs copied back.
 * lo / hi [B][13] or both NULL; centre [B][H+1][13] (centre_mode 1) or NULL. */
int sdempc_risk_batch(sdempc_handle* h, const sdempc_risk_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise, const float* lo,
                      const float* hi, const float* centre, float* cost /*[B] or NULL*/, uint32_t* exit, float* jx, uint32_t* first_exit, uint32_t* outside_any,
                      float* jstat, float* jq, float* jtail);
/* The same with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as sdempc_solve_batch_keys does. */
int sdempc_risk_batch_keys(sdempc_handle* h, const sdempc_risk_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys,
                           const float* lo, const float* hi, const float* centre, float* cost /*[B] or NULL*/, uint32_t* exit, float* jx, uint32_t* first_exit,
                           uint32_t* outside_any, float* jstat, float* jq, float* jtail);

/* ---- predicted bands (SPEC.md §12b) --------------------------------------------------------------
 * Per-step quantiles across the particles and the rank of an observed state in the predicted distribution, from the same particle x horizon tensor, reduced
 * where it lies on the device. Every word v is ordered by its key: u = bits(v); key = 0xFFFFFFFF for a NaN, else u ^ 0xFFFFFFFF where the sign bit is set,
 * else u ^ 0x80000000 — so -inf < ... < -0 < +0 < ... < +inf < NaN, all NaNs equal, and equal keys are identical words (no tie-break exists). Per
 * instance and column c = t * 13 + i, over the valid particles p < P, each output optional (NULL: not computed, not written), at least one:
 *   q      f32[B][n_ranks][H+1][13]  plane k: the value with the cfg->ranks[k]-th smallest key (0-based; ranks neither sorted nor distinct). No arithmetic
 *                                    touches it: bit for bit one particle's word, -0 / +0 kept apart; a selected NaN is 0x7FC00000.
 *   below  u32[B][H+1][13]           particles with key < key(obs[c])
 *   at     u32[B][H+1][13]           particles with key == key(obs[c])
 * obs f32[B][H+1][13] are the observed rows. A NaN there is not refused: below = the non-NaN particles, at = the NaN ones; use it for rows the caller does
 * not have and mask them. q needs cfg with 1 <= n_ranks <= 8 and 0 <= ranks[k] < P; below / at need obs; a wrong struct_size is SDEMPC_EINVAL. No particle
 * limit. Every argument is checked before the first HIP call. */
typedef struct sdempc_bands_cfg {
    int32_t struct_size;   /* sizeof(sdempc_bands_cfg) */
    int32_t n_ranks;       /* q: number of planes */
    int32_t ranks[8];
} sdempc_bands_cfg;
/* Reduces the tensor that the last sdempc_rollout_batch_dev(store_traj=1) of at least B instances left in the handle; device pointers. Refused like
 * sdempc_tube_batch_dev when the workspace holds fewer instances. Enqueue it on the stream of that rollout. */
int sdempc_bands_batch_dev(sdempc_handle* h, const sdempc_bands_cfg* cfg /*or NULL without q*/, int32_t B, const void* obs_dev /*or NULL*/, void* q_dev, void* below_dev,
                           void* at_dev, void* stream);
/* Host pointers: ONE rollout of u (as sdempc_rollout_batch; cost [B] may be NULL) with the tensor kept, the reduction, the requested outputs copied back. */
int sdempc_bands_batch(sdempc_handle* h, const sdempc_bands_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise,
                       const float* obs /*[B][H+1][13] or NULL*/, float* cost /*[B] or NULL*/, float* q, uint32_t* below, uint32_t* at);
/* The same with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as sdempc_solve_batch_keys does. */
int sdempc_bands_batch_keys(sdempc_handle* h, const sdempc_bands_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys,
                            const float* obs /*[B][H+1][13] or NULL*/, float* cost /*[B] or NULL*/, float* q, uint32_t* below, uint32_t* at);

/* ---- predicted outcome (SPEC.md §12c) --------------------------------------------------------------
 * The failure criteria of the episode score (SPEC.md §11h) asked of the prediction: every particle of the same particle x horizon tensor is scored as if it
 * were an episode, where the tensor lies on the device. Scored rows are x_t, t = 1 .. H (row index r = t - 1); the target of row t is row t of the call's xref
 * (target_mode 0) or of the caller's rows target f32[tgt_batch][tgt_steps][13] (target_mode 1; tgt_steps 1 or H+1, tgt_batch 1 or B; an index into a size-1
 * axis is 0). Per row and particle: dp, dv, c, w2, nf and the cause bits 1 radius, 2 tilt, 4 rate, 8 non-finite, exactly as §11h forms them against r2_pos,
 * cos_min, w2_max (+inf / -inf / +inf: criterion off; a NaN threshold is SDEMPC_EINVAL). Outputs over the valid particles, each optional (NULL: not
 * computed, not written), at least one:
 *   words      u32[B][P][11]        words 0 .. 10 of the §11h score table of particle p over its H rows, from the initial row
 *   fail_step  u32[B][H][5]         particles whose row r carries cause bit k = 0 .. 3; slot 4: any cause
 *   first_fail u32[B][H+1]          histogram of word 8 (first failing row); slot H: never failed. The sum is P.
 *   cause_ever u32[B][4]            particles whose word 9 has bit k
 *   chan_stat  f32[B][H][4][3]      per row and channel (dp, dv, c, w2): mean (the particle sum of SPEC.md §6.1 times float32 1/P), min, max (NaN ignored)
 *   chan_q     f32[B][H][4][n_ranks]  per row and channel the value of rank cfg->ranks[k] in the key order of the bands (-0 < +0, NaN above +inf)
 *   agg_stat   f32[B][4][3]         the same three statistics over the particles' words 1 (sum dp), 2 (max dp), 6 (min c), 7 (max w2)
 *   agg_q      f32[B][4][n_ranks]   the same order statistics over those four words
 * chan_q and agg_q need 1 <= n_ranks <= 8 and 0 <= ranks[k] < P and are refused for P > 128 (the selection sorts four particle groups in registers); every
 * output is refused when 4 (6 H + 5 + 140 ceil(P / 32)) bytes exceed 64 KiB of workgroup memory. Refusals, in this order, before the first HIP call: a wrong
 * struct_size; a NaN threshold; all outputs NULL; n_ranks or a rank out of range, then P > 128, where chan_q or agg_q is given; target_mode outside {0, 1};
 * in target_mode 1 tgt_steps or tgt_batch outside their sets, then target NULL; in target_mode 0 a NULL xref_dev. */
typedef struct sdempc_outcome_cfg {
    int32_t struct_size;   /* sizeof(sdempc_outcome_cfg) */
    float r2_pos;          /* radius^2 [m^2] around the target position */
    float cos_min;         /* cosine of the largest tilt */
    float w2_max;          /* |body rate|^2 [rad^2/s^2] */
    int32_t target_mode;   /* 0 the call's xref, 1 the caller's rows */
    int32_t tgt_steps;     /* target_mode 1: 1 or H+1 */
    int32_t tgt_batch;     /* target_mode 1: 1 or B */
    int32_t n_ranks;       /* chan_q, agg_q: number of ranks */
    int32_t ranks[8];
} sdempc_outcome_cfg;
/* Reduces the tensor that the last sdempc_rollout_batch_dev(store_traj=1) of at least B instances left in the handle; device pointers. target_dev
 * f32[tgt_batch][tgt_steps][13] (target_mode 1), xref_dev f32[B][H+1][13] (target_mode 0). Refused like sdempc_tube_batch_dev when the workspace holds fewer
 * instances. Enqueue it on the stream of that rollout. */
int sdempc_outcome_batch_dev(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const void* target_dev, const void* xref_dev, void* words_dev,
                             void* fail_step_dev, void* first_fail_dev, void* cause_ever_dev, void* chan_stat_dev, void* chan_q_dev, void* agg_stat_dev,
                             void* agg_q_dev, void* stream);
/* Host pointers: ONE rollout of u (as sdempc_rollout_batch; cost [B] may be NULL) with the tensor kept, the reduction, the requested outputs copied back.
 * target [tgt_batch][tgt_steps][13] (target_mode 1) or NULL. */
int sdempc_outcome_batch(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const float* noise,
                         const float* target, float* cost /*[B] or NULL*/, uint32_t* words, uint32_t* fail_step, uint32_t* first_fail, uint32_t* cause_ever,
                         float* chan_stat, float* chan_q, float* agg_stat, float* agg_q);
/* The same with the noise of instance b drawn on the device as normal(keys[b], (P, H, 6)), as sdempc_solve_batch_keys does. */
int sdempc_outcome_batch_keys(sdempc_handle* h, const sdempc_outcome_cfg* cfg, int32_t B, const float* x0, const float* u, const float* xref, const uint32_t* keys,
                              const float* target, float* cost /*[B] or NULL*/, uint32_t* words, uint32_t* fail_step, uint32_t* first_fail,
                              uint32_t* cause_ever, float* chan_stat, float* chan_q, float* agg_stat, float* agg_q);

/* ---- batched closed loop (SPEC.md §11) ---------------------------------------------------------
 * B independent episodes of T control ticks, entirely on the device: per tick, the solve of sdempc_solve_batch_keys on the episode's
 * state, then one Euler–Maruyama step of the handle's own model (step 0 of a rollout: dt = time_steps[0], sigma sqrt(dt), the handle's
 * mlp_dtype and math_mode) under the first control of the solution and its own noise draw. No reference counterpart: the reference closes
 * the loop only through PX4 SITL + Gazebo, one trajectory in real time. Episode b, solver frame, for tick k = 0 .. T-1:
 *   (r', s) = split(r_k); solve with noise normal(s, (P, H, 6)), warm start y_k, step size s_k, reference xref[k or 0][b or 0];
 *   (r_{k+1}, p) = split(r'); x_{k+1} = step(x_k, uopt_k[0], normal(p, (6,)));
 *   y_{k+1} = [uopt_k[1:], uopt_k[H-1]]; s_{k+1} = info_k.stepsize.
 * Host pointers:
 *   x0 [B][13]; xref [xref_ticks][xref_batch][H+1][13] with xref_ticks 1 (one window on every tick) or T, xref_batch 1 (shared by
 *   every episode) or B; keys u32[B][2] (r_0); u_init [B][H][m] and stepsize_in [B], or NULL for what sdempc_reset gives (uref tiled;
 *   ls_init_stepsize if ls_maxls > 0, else stepsize).
 *   Outputs: xs [B][T+1][13] (xs[b][0] = x0[b]), us [B][T][m] (the applied uopt_k[0]), info [B][T]; optionally (else NULL), to continue
 *   the episodes: u_next [B][H][m] = y_T, stepsize_next [B] = s_T, keys_next u32[B][2] = r_T.
 * Each tick's solve goes through sdempc_solve_batch_dev, so the layout choice is that of a solve of B instances and never changes a
 * bit. The ticks are enqueued without a host synchronisation; outputs are copied back in chunks of ticks (at most 256 MiB of device
 * buffers per chunk), so T is not bounded by device memory. A cooperative-layout barrier that gave up, or a ticket count that is off,
 * is detected at the end of a chunk, and the whole batch then runs once more from the inputs in the one-workgroup-per-instance layouts.
 * Non-finite states are not special-cased: they flow into the next solve as any state does (SPEC.md §3.7, §8). */
int sdempc_closed_loop_batch(sdempc_handle* h, int32_t B, int32_t T, const float* x0,
                             const float* xref, int32_t xref_ticks, int32_t xref_batch,
                             const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                             float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][T]*/,
                             float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                             uint32_t* keys_next /*[B][2] or NULL*/);

/* ---- batched closed loop against a separate plant (SPEC.md §11a) -------------------------------
 * sdempc_closed_loop_batch with the vehicle NOT the controller's model: episode b is stepped by plant_blobs[plant_of[b]] (model blobs of SPEC.md §2
 * with the handle's motor count), `substeps` Euler–Maruyama steps of length `dt` per control tick with the applied control uopt_k[0] held, in the
 * plant's own mlp_dtype / math_mode — each blob prepared for that arithmetic exactly as sdempc_create prepares the handle's. No reference counterpart
 * (the reference's plant is PX4 SITL + Gazebo). Tick k of episode b is that of sdempc_closed_loop_batch except
 *   (r_{k+1}, p) = split(r'); Xi = normal(p, (substeps, 6)), ONE draw of 6 * substeps values (SPEC.md §7.1: counter i pairs with i + 3 * substeps);
 *   z_0 = x_k; z_{j+1} = step_plant(z_j, uopt_k[0], Xi[j]); x_{k+1} = z_substeps.
 * With num_plants = 1, the handle's own blob, substeps = 1, dt = 0 and both arithmetic fields -1 the results are bit-identical to
 * sdempc_closed_loop_batch. Results depend only on plant_blobs[plant_of[b]], never on B, on the order or multiplicity of the blobs or on the layout
 * of the solves. The plants are prepared on the host and staged to the device once per call. Every argument is checked before the first HIP call:
 * SDEMPC_EINVAL for struct_size, num_plants outside 1 .. B, substeps outside 1 .. SDEMPC_PLANT_MAX_SUBSTEPS, dt negative or not finite, an arithmetic
 * field outside its values, plant_of NULL with 1 < num_plants < B, an index outside [0, num_plants), a motor count that differs from the handle's;
 * SDEMPC_EBLOB for a short blob or a bad header. All other arguments, outputs, chunking and the re-run are those of sdempc_closed_loop_batch. */
#define SDEMPC_PLANT_MAX_SUBSTEPS 64
typedef struct sdempc_plant_cfg {
    int32_t struct_size;   /* sizeof(sdempc_plant_cfg) */
    int32_t num_plants;    /* Np: 1 .. B */
    int32_t substeps;      /* n: plant steps per control tick, 1 .. SDEMPC_PLANT_MAX_SUBSTEPS */
    float dt;              /* plant step length; 0: (float)time_steps[0] / (float)n, one float32 division */
    int32_t mlp_dtype;     /* arithmetic of the plant step: 0 f32, 1 f16, 2 f32x3; -1: the handle's */
    int32_t math_mode;     /* 0 exact, 1 fast; -1: the handle's */
} sdempc_plant_cfg;
int sdempc_closed_loop_batch_plant(sdempc_handle* h, const sdempc_plant_cfg* pc,
                                   const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                   const int32_t* plant_of /*[B]; NULL: all 0 if num_plants == 1, identity if num_plants == B*/,
                                   int32_t B, int32_t T, const float* x0,
                                   const float* xref, int32_t xref_ticks, int32_t xref_batch,
                                   const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                   float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][T]*/,
                                   float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                   uint32_t* keys_next /*[B][2] or NULL*/);

/* ---- batched closed loop at the node's timing (SPEC.md §11b) ------------------------------------
 * sdempc_closed_loop_batch_plant with a controller that is as late as the reference node's: its MPC worker solves asynchronously, one solve at a time
 * (sde_control.py:365-450), and the state callback keeps flying the latest finished solution, indexed by the time since the state it was computed from
 * (sde_control.py:283-306). Three parameters, uniform over the batch: a solve every `solve_period` = S control ticks (Ns = ceil(T / S) solves), whose
 * solution arrives `solve_delay` = D plant substeps after the state it was computed from (0 <= D <= S * substeps: one solve at a time), and a first-order
 * motor lag `lag_alpha` (0: off). Period j covers ticks k = j S + i, i = 0 .. min(S, T - j S) - 1; episode b carries (x, r, y, s, a), a the motor state [m]:
 *   i = 0:  (r', sub) = split(r); solve j on x with noise normal(sub, (P, H, 6)), warm start y, step size s, reference xref[j or 0][b or 0]; (r, p) = split(r');
 *   i > 0:  (r, p) = split(r);                                           (no solve)
 *   Xi = normal(p, (substeps, 6)), one draw as in sdempc_closed_loop_batch_plant; for substep jj, q = i * substeps + jj:
 *     c = (q >= D ? uopt_j : y)[min(i, H-1)];  a_l = fma(alpha, c_l - a_l, a_l) if alpha > 0, else a = c exactly;  x = step_plant(x, a, Xi[jj]);
 *   xs[b][k+1] = x after the tick's last substep; us[b][k] = the a that substep 0 of tick k applied;
 *   after the period's last tick: y = rows uopt_j[min(t + S, H-1)], s = info_j.stepsize.
 * Until the first solution arrives the vehicle flies the initial warm start (u_init; NULL: uref, the hover command). A plant set is always given (the
 * handle's own blob for the controller's model). u_act_in [B][m] is the initial motor state (NULL: u_init[b][0]). info is [B][Ns]; xref is
 * [xref_solves][xref_batch][H+1][13] with xref_solves 1 or Ns. To continue: u_next, stepsize_next, keys_next and u_act_next [B][m] (each may be NULL); the
 * continuation is bit-exact when T is a multiple of S. S = 1, D = 0, alpha = 0 is sdempc_closed_loop_batch_plant bit for bit. One kernel launch advances
 * the plant by a whole period. Every argument is checked before the first HIP call: SDEMPC_EINVAL for struct_size, S < 1, D outside [0, S * substeps],
 * alpha negative, above 1 or not finite, xref_solves not 1 or Ns, and for everything sdempc_closed_loop_batch_plant refuses. Outputs, chunking (by
 * whole periods) and the re-run are those of sdempc_closed_loop_batch. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_timing_cfg {
    int32_t struct_size;   /* sizeof(sdempc_timing_cfg) */
    int32_t solve_period;  /* S: control ticks per solve, >= 1 */
    int32_t solve_delay;   /* D: plant substeps until a solution is applied, 0 .. S * substeps */
    float lag_alpha;       /* motor lag per plant substep: 0 off, else 0 < alpha <= 1 */
} sdempc_timing_cfg;
int sdempc_closed_loop_batch_timed(sdempc_handle* h, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                   const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                   const int32_t* plant_of /*[B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                   const float* xref, int32_t xref_solves, int32_t xref_batch,
                                   const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                   const float* u_act_in /*[B][m] or NULL*/,
                                   float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][Ns]*/,
                                   float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                   uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/);

/* ---- batched closed loop with a scenario (SPEC.md §11c) -----------------------------------------
 * sdempc_closed_loop_batch_timed with two optional per-tick schedules: things that HAPPEN to a vehicle during an episode. With dist NULL and plant_ticks 1
 * the call is sdempc_closed_loop_batch_timed bit for bit.
 *   Disturbance: dist f32[dist_ticks][dist_batch][6], dist_ticks 1 or T (per control TICK, not per solve), dist_batch 1 or B, tick-major like xref; an index
 *   into a size-1 axis is 0. Row (k, b) = (w_v[3], w_om[3]): an external linear acceleration in the solver's world frame and an external angular acceleration
 *   in the body frame, held over every substep of tick k. After each x = step_plant(x, a, Xi[jj]) of tick k:
 *     v_i = fma(w_v[i], dt_p, v_i) (x[3 + i]); om_i = fma(w_om[i], dt_p, om_i) (x[10 + i]), i = 0..2, dt_p the plant's float32 step length (what step_plant
 *   uses). Position and attitude are untouched. The six fmas are applied whenever dist is given, zero rows included (a zero row changes nothing but a -0
 *   component, which becomes +0). xs[b][k+1] is the state after the last substep's fmas.
 *   Plant schedule: plant_of is int32[plant_ticks][B], plant_ticks 1 (the plant_of of sdempc_closed_loop_batch_plant) or T: tick k of episode b is stepped by
 *   plant_blobs[plant_of[k or 0][b]]. A switch happens at a tick start (also in the middle of a solve period) and changes the vehicle only: physics prior, W1u
 *   (the control table is re-formed from the new blob) and sigma sqrt(dt_p); x, the motor state, keys, warm start and the plant set's dt and arithmetic carry
 *   over. With plant_ticks = T num_plants may be up to B * T (one episode that drops a payload needs two blobs) and plant_of must be given.
 * Results depend only on the blobs an episode names, never on B, on the order or multiplicity of the set or on the layout of the solves; the key schedule
 * depends on S and T only; continuation from (xs[:, T], u_next, stepsize_next, keys_next, u_act_next) with the schedules sliced at T is bit-exact when T is a
 * multiple of S. The chunk's disturbance and schedule rows are staged per chunk, like moving references. Every argument is checked before the first HIP call:
 * SDEMPC_EINVAL for struct_size, dist_ticks not 1 or T, dist_batch not 1 or B, plant_ticks not 1 or T, a non-finite dist entry, a scheduled index outside
 * [0, num_plants), num_plants outside 1 .. B * plant_ticks, plant_of NULL with plant_ticks > 1 (or where sdempc_closed_loop_batch_plant refuses it), and for
 * everything sdempc_closed_loop_batch_timed refuses. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_scenario_cfg {
    int32_t struct_size;   /* sizeof(sdempc_scenario_cfg) */
    const float* dist;     /* [dist_ticks][dist_batch][6] or NULL: no disturbance */
    int32_t dist_ticks;    /* 1 or T (ignored when dist is NULL) */
    int32_t dist_batch;    /* 1 or B (ignored when dist is NULL) */
    int32_t plant_ticks;   /* Tp: 1 or T; plant_of is [plant_ticks][B] */
} sdempc_scenario_cfg;
int sdempc_closed_loop_batch_scenario(sdempc_handle* h, const sdempc_scenario_cfg* scenario, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                      const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                      const float* xref, int32_t xref_solves, int32_t xref_batch,
                                      const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                      const float* u_act_in /*[B][m] or NULL*/,
                                      float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][Ns]*/,
                                      float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                      uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/);

/* ---- batched closed loop through the rate-setpoint interface (SPEC.md §11d) ----------------------
 * sdempc_closed_loop_batch_scenario flown the way the reference node flies: every solve is post-processed into a table of mean thrust and predicted body rates
 * (sde_control.py:428-432) that goes to the vehicle next to the motor values, with weight_motors (srv/FollowTraj.srv:10; it starts at 0, sde_control.py:63: rate
 * setpoints only), and the vehicle's own rate controller tracks the rates far more often than the MPC solves. Here that controller runs on EVERY plant substep,
 * in front of the motor lag. Episode b carries, beside (x, r, y, s, a), a rate integrator g[3] and a rate tail wt[H][3]. In substep q = i * substeps + jj of period
 * j, with r = min(i, H-1) and the source this period's solution when q >= D, else the tail (all float32; fma is the fused one):
 *   u_r = (q >= D ? uopt_j : y)[r];  cbar = (u_r[0] + ... + u_r[m-1]) * inv_m (sum left to right; inv_m = 1.0f / (float)m);
 *   wsp = q >= D ? xevol_j[r+1][10..12] : wt[r];           e = wsp - x[10..12] (the CURRENT state);
 *   g_a = clamp(fma(ki_dt_a, e_a, g_a), -integ_limit_a, integ_limit_a);   tau_a = fma(kp_a, e_a, g_a)   (clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v));
 *   cw_l = clamp(fma(mixer[l][2], tau_2, fma(mixer[l][1], tau_1, fma(mixer[l][0], tau_0, cbar))), u_lo[l], u_hi[l])  (the handle's input bounds);
 *   c_l = cw_l if motor_weight == 0; u_r[l] if motor_weight == 1; else fma(motor_weight, u_r[l] - cw_l, cw_l);
 *   then the substep of sdempc_closed_loop_batch_scenario with command c: motor lag, plant step, disturbance fmas.
 * After the period wt[t] = xevol_j[min(t + S, H-1) + 1][10..12]. The blend is this build's definition of weight_motors / 100 (its PX4-side meaning is not in the
 * reference). For m = 4 cbar equals the node's np.sum(...) / m bit for bit; for m in {3, 5, 6, 7} the multiplication by inv_m may differ from a division by 1 ulp.
 * `scenario` may be NULL (no disturbance, plant_of one row). rate_integ_in [B][3] and rate_tail_in [B][H][3] may be NULL (zeros; the tail is never read when
 * solve_delay is 0). Outputs beside the scenario entry point's: ws [B][T][4] = (cbar, wsp[3]) in force at each tick's first substep (required);
 * rate_integ_next [B][3] and rate_tail_next [B][H][3] (each may be NULL), which continue the episodes bit for bit together with the other five when T is a
 * multiple of S. us stays the motor state at each tick's first substep. Every argument is checked before the first HIP call: SDEMPC_EINVAL for struct_size,
 * a non-finite gain, limit or mixer entry (rows below the handle's motor count), a negative limit, motor_weight outside [0, 1], inv_m neither 0 nor
 * (float)1 / (float)m, ws NULL, and for everything sdempc_closed_loop_batch_scenario refuses. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_rate_cfg {
    int32_t struct_size;                     /* sizeof(sdempc_rate_cfg) */
    float kp[3];                             /* proportional gain per body axis (roll, pitch, yaw) */
    float ki_dt[3];                          /* integral gain times the plant's step length, formed by the caller in float32 */
    float integ_limit[3];                    /* bound of |g_a|, >= 0 */
    float mixer[SDEMPC_MAX_MOTORS][3];       /* motor l takes mixer[l][a] of the torque demand about axis a */
    float motor_weight;                      /* weight_motors / 100: 0 rate setpoints only .. 1 motor values only */
    float inv_m;                             /* (float)1 / (float)m as the caller formed it, or 0: the library forms it */
} sdempc_rate_cfg;
int sdempc_closed_loop_batch_rate(sdempc_handle* h, const sdempc_rate_cfg* rate, const sdempc_scenario_cfg* scenario /*or NULL*/,
                                  const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                  const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                  const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                  const float* xref, int32_t xref_solves, int32_t xref_batch,
                                  const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                  const float* u_act_in /*[B][m] or NULL*/,
                                  float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][Ns]*/,
                                  float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                  uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                  const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                  float* ws /*[B][T][4]*/, float* rate_integ_next /*[B][3] or NULL*/, float* rate_tail_next /*[B][H][3] or NULL*/);

/* ---- batched closed loop with per-motor actuator faults and substep-resolution states (SPEC.md §11e) ---
 * sdempc_closed_loop_batch_rate (`rate` given) or sdempc_closed_loop_batch_scenario (`rate` NULL; `scenario` may be NULL here too) with two optional additions.
 * With fault_cfg NULL (or fault_cfg->fault NULL) and xsub NULL the call is that entry point bit for bit.
 *   Fault schedule: fault f32[fault_ticks][fault_batch][m][2], fault_ticks 1 or T (per control TICK, not per solve), fault_batch 1 or B, tick-major like dist; an
 *   index into a size-1 axis is 0. Row (k, b, l) = (kappa_l, beta_l). In every plant substep of tick k the motor state a is updated first (the lag of
 *   sdempc_closed_loop_batch_timed, behind the rate loop's command if one is given); then
 *     at_l = fma(kappa_l, a_l, beta_l);   x = step_plant(x, at, Xi[jj]);   then the disturbance fmas, if dist is given.
 *   The motor state does not change: a itself is the lag state, the next substep's a, us[b][k] and u_act_next. The fault sits between the command and the rotor,
 *   and nobody is told: neither the solve nor the rate loop sees it except through the state. A dead motor is (0, 0) (thrust ct0, moment 0, the plant's W1u sees 0),
 *   a loss of effectiveness (kappa, 0) with 0 < kappa < 1, a motor stuck at c (0, c), a bias (1, delta). Rows change at tick starts only (ticks inside a solve
 *   period included). The fma is applied whenever a schedule is given, neutral rows (1, 0) included (a neutral row changes nothing but an a_l of -0, which
 *   reaches the plant as +0). Nothing is clamped: what reaches the plant is the caller's statement.
 *   Substep states: xsub f32[B][T * substeps][13], xsub[b][k * substeps + jj] = the plant state after substep jj of tick k, disturbance fmas included; so
 *   xsub[b][k * substeps + substeps - 1] is xs[b][k+1] bit for bit. Available with or without a fault schedule and with or without a rate loop.
 * With `rate` NULL the five rate-only pointers (rate_integ_in, rate_tail_in, ws, rate_integ_next, rate_tail_next) must be NULL. Key schedule, solve, warm start,
 * step size, rate tail, integrator, chunking, continuation (bit-exact when T is a multiple of S, the schedules sliced at T) and the plant schedule are those of
 * the entry points above. The chunk's fault rows are staged per chunk like dist; its xsub rows are counted in the chunk's bytes and copied back with the other
 * outputs. Every argument is checked before the first HIP call: SDEMPC_EINVAL for struct_size, fault_ticks not 1 or T, fault_batch not 1 or B, a non-finite
 * fault entry, a rate-only pointer without `rate`, and for everything sdempc_closed_loop_batch_rate / _scenario refuse. No ABI version change: detect the
 * entry point by its symbol. */
typedef struct sdempc_fault_cfg {
    int32_t struct_size;   /* sizeof(sdempc_fault_cfg) */
    const float* fault;    /* [fault_ticks][fault_batch][m][2] = (kappa, beta), or NULL: no fault */
    int32_t fault_ticks;   /* 1 or T (ignored when fault is NULL) */
    int32_t fault_batch;   /* 1 or B (ignored when fault is NULL) */
} sdempc_fault_cfg;
int sdempc_closed_loop_batch_fault(sdempc_handle* h, const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                   const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                   const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                   const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                   const float* xref, int32_t xref_solves, int32_t xref_batch,
                                   const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                   const float* u_act_in /*[B][m] or NULL*/,
                                   float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][Ns]*/,
                                   float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                   uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                   const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                   float* ws /*[B][T][4]; NULL without rate*/, float* rate_integ_next /*[B][3] or NULL*/, float* rate_tail_next /*[B][H][3] or NULL*/,
                                   float* xsub /*[B][T * substeps][13] or NULL*/);

/* ---- batched closed loop on a measured state (SPEC.md §11f) -------------------------------------------
 * sdempc_closed_loop_batch_fault with a controller that reads an ESTIMATE of the state, as the reference node does (its mpc_state_callback gets the FCU's
 * estimate, not the truth): noise, bias and dropouts on the state that goes INTO each solve. The plant is untouched, and the rate loop keeps reading the
 * plant's current body rates. With `obs` NULL the call is sdempc_closed_loop_batch_fault bit for bit; obs_keys, xmeas_in, xmeas, obs_keys_next and xmeas_next
 * must then be NULL. Beside the state of that entry point episode b carries an observation key q (a chain of its own: the main chain is never disturbed) and
 * the held measurement xm[13]. At solve j, with x the plant state at the period's first tick (all float32; fma is the fused one):
 *   (q, me) = split(q)                                   at EVERY solve, valid or not
 *   if valid[j or 0][b or 0]:
 *     xi = normal(me, (12,))                             (SPEC.md §7.1: counter i pairs with i + 6)
 *     e_i = fma(sigma_i, xi_i, beta_i), i = 0..11        rows sigma[j or 0][b or 0], beta[j or 0][b or 0], in the order p, v, theta, omega
 *     xm[0..2] = x[0..2] + e[0..2];  xm[3..5] = x[3..5] + e[3..5];  xm[10..12] = x[10..12] + e[9..11]
 *     h_a = 0.5f * e[6 + a];  (w, x, y, z) = x[6..9]     the attitude times (1, h) from the right: a small body-frame rotation, NOT renormalised
 *     xm[6] = fma(-z, h2, fma(-y, h1, fma(-x, h0, w)));  xm[7] = fma(-z, h1, fma(y, h2, fma(w, h0, x)));
 *     xm[8] = fma(-x, h2, fma(z, h0, fma(w, h1, y)));    xm[9] = fma(-y, h0, fma(x, h1, fma(w, h2, z)))
 *   else xm stays as it is                               a dropout: the estimator repeats its last output
 *   solve j starts from xm instead of x; everything else is sdempc_closed_loop_batch_fault.
 * sigma (noise scale, finite and >= 0) and beta (bias, finite) are f32[obs_solves][obs_batch][12], obs_solves 1 or Ns, obs_batch 1 or B, solve-major like xref;
 * valid is int32[valid_solves][valid_batch] with the same axis rule; an index into a size-1 axis is 0. sigma or beta NULL: zeros; valid NULL: always valid.
 * The held measurement starts as xmeas_in [B][13] (NULL: x0). The formulas run whenever `obs` is given: a neutral observation (sigma and beta zero, always
 * valid) reproduces sdempc_closed_loop_batch_fault bit for bit except that a component of x equal to -0 reaches the solve as +0. Nothing is clamped or
 * renormalised: what reaches the solver is the caller's statement. The main key chain depends on S and T only, the observation chain on the number of solves
 * only. Outputs: xmeas [B][Ns][13] = what solve j was started from (a held row on a dropout; may be NULL); obs_keys_next u32[B][2] and xmeas_next [B][13]
 * (each may be NULL) continue the episodes bit for bit, together with the other continuation values, when T is a multiple of S. The chunk's sigma / beta / valid
 * rows are staged per chunk when they move, like moving references; its xmeas rows are counted in the chunk's bytes and copied back with info. Every argument
 * is checked before the first HIP call: SDEMPC_EINVAL for struct_size, obs_solves / valid_solves not 1 or Ns, obs_batch / valid_batch not 1 or B, a non-finite
 * or negative sigma, a non-finite beta, a valid entry other than 0 / 1, obs_keys NULL with `obs` given, an observation pointer without `obs`, and for
 * everything sdempc_closed_loop_batch_fault refuses. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_obs_cfg {
    int32_t struct_size;   /* sizeof(sdempc_obs_cfg) */
    const float* sigma;    /* [obs_solves][obs_batch][12] noise scale, or NULL: zeros */
    const float* beta;     /* [obs_solves][obs_batch][12] bias, or NULL: zeros */
    int32_t obs_solves;    /* 1 or Ns (ignored when sigma and beta are NULL) */
    int32_t obs_batch;     /* 1 or B (ignored when sigma and beta are NULL) */
    const int32_t* valid;  /* [valid_solves][valid_batch] 1: a measurement, 0: a dropout; or NULL: always valid */
    int32_t valid_solves;  /* 1 or Ns (ignored when valid is NULL) */
    int32_t valid_batch;   /* 1 or B (ignored when valid is NULL) */
} sdempc_obs_cfg;
int sdempc_closed_loop_batch_observed(sdempc_handle* h, const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]*/, const float* xmeas_in /*[B][13] or NULL*/,
                                      const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                      const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                      const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                      const float* xref, int32_t xref_solves, int32_t xref_batch,
                                      const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                      const float* u_act_in /*[B][m] or NULL*/,
                                      float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][Ns]*/,
                                      float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                      uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                      const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                      float* ws /*[B][T][4]; NULL without rate*/, float* rate_integ_next /*[B][3] or NULL*/, float* rate_tail_next /*[B][H][3] or NULL*/,
                                      float* xsub /*[B][T * substeps][13] or NULL*/,
                                      float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/);

/* ---- batched closed loop from an aged, renormalised state estimate (SPEC.md §11g) -----------------------
 * sdempc_closed_loop_batch_observed with INPUT-side latency: the state the estimate is an estimate OF is already old when the solve starts (the reference node's
 * mpc_state_callback hands the solver a state stamped msg.time_usec), and a real estimator emits a unit quaternion. solve_delay models the other half, the
 * solution arriving late. With `age_cfg` NULL the call is sdempc_closed_loop_batch_observed bit for bit, with the same launches; xhist_in and xhist_next must
 * then be NULL. Let n = plant substeps, S = solve_period and z_k episode b's plant state after global plant substep k (gust fmas included), so z_0 = x0 and
 * z_{T n} = xs[b][T]; solve j happens at c = j S n. Beside the state of that entry point episode b carries the last age_max substep states before c: for k < 0,
 * z_k = xhist_in[b][age_max + k] (oldest first; xhist_in NULL: every row is x0, the vehicle sat there). At solve j, when the solve is valid:
 *   A  = age[j or 0][b or 0]                   0 <= A <= age_max, in plant substeps
 *   x  = z_{c - A}                             (A = 0: the plant state, the observed entry point exactly)
 *   xm = the formulas of that entry point on this x (chain, draws, e, sums, attitude product: unchanged)
 *   if renormalise: (q0..q3) = xm[6..9]; s = fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0))); r = rsqrt(s) (SPEC.md §3.2, the software form whatever the handle's
 *                   math_mode); xm[6 + i] = q_i * r
 * On a dropout nothing of this runs: xm is held, the observation chain still advances. The plant, the rate loop, the main key chain and the observation chain are
 * untouched. age is int32[age_solves][age_batch], age_solves 1 or Ns, age_batch 1 or B, solve-major, an index into a size-1 axis is 0; NULL: every age 0.
 * 0 <= age_max <= min(S, T) * n: one period of memory. Output xhist_next [B][age_max][13] = z_{T n - age_max} .. z_{T n - 1} (may be NULL): carried back in as
 * xhist_in with the other continuation values it continues the episodes bit for bit when T is a multiple of S. Every age 0 and renormalise 0 reproduce
 * sdempc_closed_loop_batch_observed bit for bit, whatever age_max is. With age_max > 0 the history is fed on the device from the substep rows of the chunk (the
 * xsub region then exists in the chunk, and counts in its bytes, whether or not xsub is asked for). Every argument is checked before the first HIP call:
 * SDEMPC_EINVAL for struct_size, an age cfg without `obs`, a history pointer without an age cfg, age_max outside [0, min(S, T) * n], age_solves not 1 or Ns,
 * age_batch not 1 or B, an age entry outside [0, age_max], renormalise other than 0 / 1, a history pointer with age_max 0, and for everything
 * sdempc_closed_loop_batch_observed refuses. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_age_cfg {
    int32_t struct_size;   /* sizeof(sdempc_age_cfg) */
    const int32_t* age;    /* [age_solves][age_batch] age of the estimate in plant substeps, or NULL: every age 0 */
    int32_t age_solves;    /* 1 or Ns (ignored when age is NULL) */
    int32_t age_batch;     /* 1 or B (ignored when age is NULL) */
    int32_t age_max;       /* rows of the history, 0 .. min(S, T) * substeps */
    int32_t renormalise;   /* 1: the attitude of xm is scaled to unit length; 0: left as the product gives it */
} sdempc_age_cfg;
int sdempc_closed_loop_batch_aged(sdempc_handle* h, const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                  const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]*/, const float* xmeas_in /*[B][13] or NULL*/,
                                  const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                  const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                  const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                  const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                  const float* xref, int32_t xref_solves, int32_t xref_batch,
                                  const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                  const float* u_act_in /*[B][m] or NULL*/,
                                  float* xs /*[B][T+1][13]*/, float* us /*[B][T][m]*/, sdempc_info* info /*[B][Ns]*/,
                                  float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                  uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                  const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                  float* ws /*[B][T][4]; NULL without rate*/, float* rate_integ_next /*[B][3] or NULL*/, float* rate_tail_next /*[B][H][3] or NULL*/,
                                  float* xsub /*[B][T * substeps][13] or NULL*/,
                                  float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                  float* xhist_next /*[B][age_max][13] or NULL*/);

/* ---- batched closed loop scored on the device, per-row outputs optional (SPEC.md §11h) -------------------
 * sdempc_closed_loop_batch_aged plus the evaluator: per episode a score row of 16 32-bit words, formed on the device from the rows the loop already holds, so that a
 * campaign's questions (did the episode leave a radius, tip over, spin up, go non-finite — and when; how far off was it; how hard did the solver work) cost B * 64 bytes
 * of output whatever T is. With `score` NULL the call IS sdempc_closed_loop_batch_aged bit for bit, with the same launches; score_in and score_out must then be NULL and
 * no per-row output may be. With `score` given each of xs, us, info, ws, xsub and xmeas may be NULL: a NULL output is neither copied to the host nor scattered; every
 * other output, and every value of those that are given, is what the call without a score gives. The continuation outputs keep their meaning.
 * Scored rows, in time order: with substeps = 0 the tick states x_{k+1} (xs[b][k + 1]), k = 0 .. T-1; with substeps = 1 the plant's substep states (xsub[b][.], n per
 * tick; the xsub region then exists in the chunk, and counts in its bytes, whether or not xsub is asked for). Each row x of tick k is compared with the target
 * g = score_ref[k or 0][b or 0] (13 floats in the solver's frame; position and velocity are read), in float32, every fma explicit:
 *   e_i = x_i - g_i (i < 3); dp = fma(e2, e2, fma(e1, e1, e0 e0)); dv likewise on indices 3..5
 *   c  = fma(-2, qx qx + qy qy, 1)     (qx = x[7], qy = x[8]: the cosine of the tilt, SPEC.md §5.2);   w2 = fma(w2, w2, fma(w1, w1, w0 w0)) on x[10..12]
 *   nf = some component of x fails |x_i| < inf
 *   cause = 1 if !(dp <= r2_pos) | 2 if !(c >= cos_min) | 4 if !(w2 <= w2_max) | 8 if nf          (a NaN fails every comparison)
 * The thresholds arrive squared / as a cosine (no device sqrt or acos); +inf, -inf, +inf switch a criterion off. The words of episode b:
 *    0 u32 rows scored so far (its value before the increment is the row's index r)      8 u32 r of the first row with a non-zero cause; 0xffffffff: none
 *    1 f32 sum of dp, plain adds in row order                                             9 u32 OR of all causes
 *    2 f32 max dp (dp > max replaces it; initially 0)                                    10 u32 rows with a non-zero cause
 *    3 u32 r of that maximum (first occurrence)                                          11 u32 per tick, from us: motors with u_j <= u_lo_j or u_j >= u_hi_j
 *    4 f32 dp of the last row                                                            12 f32 per tick: a = 0; a = fma(d_j, d_j, a), d_j = u_j - uref_j, j ascending; sum + a
 *    5 f32 sum of dv                                                                     13 u32 per solve, from info: sum of (u32)num_steps
 *    6 f32 min c (c < min replaces it; initially +inf)                                   14 u32 per solve: sum of (u32)num_ls_trials
 *    7 f32 max w2 (initially 0)                                                          15 u32 per solve: solves with !(opt_cost < init_cost)
 * ((u32)v is v itself where 0 <= v < 2^32 and 0 otherwise, a NaN included.) score_in NULL starts from the initial row (zeros, word 6 = +inf, word 8 = 0xffffffff); carrying
 * score_out back in as score_in with the other continuation values continues the score word for word when T is a multiple of solve_period. The score does not depend on B,
 * on chunking, on the layout of the solves or on which outputs were requested. score_ref is [ref_ticks][ref_batch][13], ref_ticks 1 or T, ref_batch 1 or B, tick-major, an
 * index into a size-1 axis is 0. Every argument is checked before the first HIP call: SDEMPC_EINVAL for struct_size, substeps outside 0 / 1, ref_ticks not 1 or T, ref_batch
 * not 1 or B, score_ref or score_out NULL, a NaN threshold, score_in or score_out without `score`, a NULL xs / us / info (ws with a rate cfg) without `score`, and for everything
 * sdempc_closed_loop_batch_aged refuses. No ABI version change: detect the entry point by its symbol. */
#define SDEMPC_SCORE_WORDS 16
typedef struct sdempc_score_cfg {
    int32_t struct_size;     /* sizeof(sdempc_score_cfg) */
    int32_t substeps;        /* 0: the tick states are scored; 1: the plant's substep states */
    float r2_pos;            /* squared position radius [m^2]; +inf: off */
    float cos_min;           /* cosine of the largest tilt; -inf: off */
    float w2_max;            /* squared body-rate limit [rad^2/s^2]; +inf: off */
    const float* score_ref;  /* [ref_ticks][ref_batch][13] the target of each tick */
    int32_t ref_ticks;       /* 1 or T */
    int32_t ref_batch;       /* 1 or B */
} sdempc_score_cfg;
int sdempc_closed_loop_batch_scored(sdempc_handle* h, const sdempc_score_cfg* score /*or NULL*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                    const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                    const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                    const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                    const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                    const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                    const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                    const float* xref, int32_t xref_solves, int32_t xref_batch,
                                    const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                    const float* u_act_in /*[B][m] or NULL*/,
                                    float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                    sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                    float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                    uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                    const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                    float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                    float* rate_tail_next /*[B][H][3] or NULL*/,
                                    float* xsub /*[B][T * substeps][13] or NULL*/,
                                    float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                    float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/);

/* ---- batched closed loop with gusts and estimator bias drawn on the device (SPEC.md §11i) -------------------
 * sdempc_closed_loop_batch_scored plus two optional first-order Gauss-Markov processes per episode, stepped on the device from key chains, so that the stochastic
 * inputs of a campaign are keys and O(B) coefficients instead of [T][B][6] and [Ns][B][12] host arrays. With both cfgs NULL the call IS
 * sdempc_closed_loop_batch_scored bit for bit, with the same launches; the six new outputs must then be NULL.
 * A process of width W (dist_proc: W = 6, the disturbance w_v[3], w_omega[3]; bias_proc: W = 12, the estimator bias p, v, theta, omega) holds per episode b a key
 * chain c_b, a state g_b f32[W] and coefficients rho, scale f32[W] (one row for all episodes, or one per episode). One step, in float32:
 *   (c, e) = split(c)              the first half continues the chain, the second is the draw key
 *   xi     = normal(e, (W,))       counter i pairs with i + W / 2
 *   t_i    = scale_i * xi_i        one rounding; never contracted into the fma
 *   g_i    = fma(rho_i, g_i, t_i)
 *   row_i  = g_i, or d_i + g_i when a scheduled input of that kind is given as well (d its row (k or 0, b or 0); one float32 add)
 * dist_proc takes one step per control tick k = 0 .. T-1, ticks inside a solve period included; row is the disturbance row of tick k and episode b, read by the plant
 * exactly as a row of scenario->dist is. It makes the run a scenario run, as `dist` does. bias_proc takes one step per solve j, valid or not (a dropout holds the
 * estimate, the error process keeps running), before the measurement is formed; row is the beta of that solve (e = fma(sigma, normal(me, 12), row), unchanged). It
 * makes the run an observed one: it needs an obs cfg — whose sigma, beta and valid may all be NULL — and obs_keys, whose chain it does not touch.
 * dist_rows / bias_rows are per-row outputs (the rows as the plant / the measurement read them): NULL means neither copied back nor scattered. The *_next outputs
 * continue the processes bit for bit when carried back in as keys / state_in: the disturbance process for any T, the bias process when T is a multiple of
 * solve_period. Every argument is checked before the first HIP call: SDEMPC_EINVAL for a wrong struct_size, batch not 1 or B, a NULL rho, scale or keys, a non-finite
 * entry of rho, scale or state_in, rho outside [0, 1], a negative scale, bias_proc without obs_keys, a new output without its cfg, and for everything
 * sdempc_closed_loop_batch_scored refuses. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_process_cfg {
    int32_t struct_size;      /* sizeof(sdempc_process_cfg) */
    int32_t batch;            /* rows of rho / scale: 1 or B */
    const float* rho;         /* [batch][W], each in [0, 1] */
    const float* scale;       /* [batch][W], finite, >= 0 */
    const uint32_t* keys;     /* [B][2] the process chain */
    const float* state_in;    /* [B][W] or NULL: zeros */
} sdempc_process_cfg;
int sdempc_closed_loop_batch_drawn(sdempc_handle* h, const sdempc_process_cfg* dist_proc /*or NULL, W = 6*/, const sdempc_process_cfg* bias_proc /*or NULL, W = 12*/,
                                   const sdempc_score_cfg* score /*or NULL*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                   const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                   const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                   const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                   const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                   const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                   const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                   const float* xref, int32_t xref_solves, int32_t xref_batch,
                                   const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                   const float* u_act_in /*[B][m] or NULL*/,
                                   float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                   sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                   float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                   uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                   const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                   float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                   float* rate_tail_next /*[B][H][3] or NULL*/,
                                   float* xsub /*[B][T * substeps][13] or NULL*/,
                                   float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                   float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/,
                                   float* dist_rows /*[B][T][6] or NULL*/, uint32_t* dist_keys_next /*[B][2] or NULL*/, float* dist_state_next /*[B][6] or NULL*/,
                                   float* bias_rows /*[B][Ns][12] or NULL*/, uint32_t* bias_keys_next /*[B][2] or NULL*/, float* bias_state_next /*[B][12] or NULL*/);

/* ---- batched closed loop tracking a trajectory: reference windows and score targets cut on the device (SPEC.md §11j) -------------------
 * sdempc_closed_loop_batch_drawn plus an optional trajectory set, from which the device forms every solve's reference window (and, if asked, every tick's score
 * target) where the solve reads it, so that what the controller is asked to fly is a small table and O(B) numbers instead of an [Ns][B][H+1][13] host array. With
 * `track` NULL the call IS sdempc_closed_loop_batch_drawn bit for bit, with the same launches.
 * A set holds n_tables piecewise-linear tables, end to end: table j has L = knots[j] >= 1 knots (t strictly increasing and finite; x[L][13] in the solver's frame, taken
 * as given) and a period (NULL or 0: clamp at the ends; > 0: wrap, and then t[0] = 0 and t[L-1] = period). Episode b flies table table_of[b] (NULL: table 0) with
 * phase[b] (NULL: 0), rate[b] >= 0 (NULL: 1) and offset[b][3] (NULL: 0). All arithmetic is float32, every multiply and fma as written:
 *   w[i]   = float32(1 / (float64(t[i+1]) - float64(t[i])))                      formed once by the library
 *   dt     = time_steps[0];  c[i] = float32(sum_{r<i} float64(time_steps[r])), c[0] = 0;  theta(k) = float32(k) * dt for the GLOBAL tick k = tick0 + tick in the call
 *   row(u): tau = fma(rate, u, phase);  period > 0: n = floor(tau * float32(1 / float64(period))), tau = fma(-n, period, tau);  tau = min(max(tau, t[0]), t[L-1]);
 *           i = the largest index in [0, L-2] with t[i] <= tau (bisection from lo = 0, hi = L-1);  a = (tau - t[i]) * w[i];  y_c = fma(a, x[i+1][c] - x[i][c], x[i][c])
 *           (L = 1: y = x[0]);  y[0..2] += offset;  y[3..5] *= rate;  y[10..12] *= rate;  renorm set: y[6..9] scaled to unit length as sdempc_age_cfg::renormalise does
 * Row i = 0 .. H of the window of the solve at tick k is row(theta(k) + c[i]); the score target of tick k (of x_{k+1} and of tick k's substep rows) is
 * row(theta(k + 1)). Nothing else enters, so the chunking, a re-run, the outputs requested and B change no bit, and passing tick0 + T as the next call's tick0
 * continues the run. With `track` given xref must be NULL and xref_solves 0 (xref_batch is not read); with score_targets set a score cfg must be present and its
 * score_ref NULL (ref_ticks / ref_batch are not read). Checked before the first HIP call, the track struct first: SDEMPC_EINVAL for a wrong struct_size,
 * n_tables < 1, a NULL knots, t or x, a knot count below 1, a non-increasing or non-finite t, a non-finite x, a negative or non-finite period, a periodic table
 * whose t[0] != 0 or t[L-1] != period, table_of outside the set, a non-finite phase or offset, a negative or non-finite rate, renorm or score_targets other than
 * 0 / 1, tick0 < 0, tick0 + T >= 2^24, xref or score_ref given beside it, and for everything sdempc_closed_loop_batch_drawn refuses. No ABI version change: detect
 * the entry points by their symbols. */
typedef struct sdempc_track_cfg {
    int32_t struct_size;      /* sizeof(sdempc_track_cfg) */
    int32_t n_tables;         /* >= 1 */
    const int32_t* knots;     /* [n_tables] L of each table, >= 1 */
    const float* t;           /* [sum L] knot times, table after table */
    const float* x;           /* [sum L][13] knot states */
    const float* period;      /* [n_tables] or NULL: every table clamps */
    const int32_t* table_of;  /* [B] or NULL: table 0 */
    const float* phase;       /* [B] or NULL: 0 */
    const float* rate;        /* [B] or NULL: 1 */
    const float* offset;      /* [B][3] or NULL: 0 */
    int32_t tick0;            /* global tick of the call's first tick, >= 0 */
    int32_t renorm;           /* 1: unit attitude in every row; 0: the interpolated one */
    int32_t score_targets;    /* 1: the score targets are cut from the set as well (score cfg with score_ref NULL); 0: score_ref as before */
} sdempc_track_cfg;
int sdempc_closed_loop_batch_tracked(sdempc_handle* h, const sdempc_track_cfg* track /*or NULL*/,
                                     const sdempc_process_cfg* dist_proc /*or NULL, W = 6*/, const sdempc_process_cfg* bias_proc /*or NULL, W = 12*/,
                                     const sdempc_score_cfg* score /*or NULL*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                     const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                     const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                     const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                     const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                     const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                     const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                     const float* xref /*NULL with track*/, int32_t xref_solves /*0 with track*/, int32_t xref_batch,
                                     const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                     const float* u_act_in /*[B][m] or NULL*/,
                                     float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                     sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                     float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                     uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                     const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                     float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                     float* rate_tail_next /*[B][H][3] or NULL*/,
                                     float* xsub /*[B][T * substeps][13] or NULL*/,
                                     float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                     float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/,
                                     float* dist_rows /*[B][T][6] or NULL*/, uint32_t* dist_keys_next /*[B][2] or NULL*/, float* dist_state_next /*[B][6] or NULL*/,
                                     float* bias_rows /*[B][Ns][12] or NULL*/, uint32_t* bias_keys_next /*[B][2] or NULL*/, float* bias_state_next /*[B][12] or NULL*/);
/* The same launch with no loop around it: out[g][b] is the reference window f32[H+1][13] of episode b at global tick track->tick0 + ticks[g] (ticks[g] >= 0, the sum
 * below 2^24), formed on the device and copied back — for callers of sdempc_solve_batch_keys who want device-formed windows, and the direct handle on the device code
 * of this section. `track` is required and checked as above (score_targets is not read). */
int sdempc_reference_windows(sdempc_handle* h, const sdempc_track_cfg* track, int32_t B, int32_t n, const int32_t* ticks /*[n]*/, float* out /*[n][B][H+1][13]*/);

/* ---- batched closed loop with motor faults and estimator dropouts drawn on the device (SPEC.md §11k) -------------------
 * sdempc_closed_loop_batch_tracked plus two optional finite Markov chains per episode, stepped on the device from key chains of their own, so that WHEN a motor fails
 * and WHEN the position source drops out are keys and O(B) thresholds instead of a [T][B][m][2] fault array and an [Ns][B] flag array. With both cfgs NULL the call IS
 * sdempc_closed_loop_batch_tracked bit for bit, with the same launches; the six new outputs must then be NULL.
 * A chain has K modes besides state 0 (1 <= K <= 4) and per episode b a key chain c_b; per lane a state s in 0 .. K, cumulative nondecreasing thresholds
 * onset u32[K] and thresholds clear u32[K]. One step, in integers alone:
 *   (c, e) = split(c)                  the first half continues the chain, the second is the draw key
 *   w      = random_bits(e, lanes)     SPEC.md §7.1; an odd count's last block has a zero second counter
 *   s == 0: s' = j + 1 for the smallest j < K with w_l < onset[l][j], else 0
 *   s  > 0: s' = 0 if w_l < clear[l][s-1], else s
 * One transition per step: a lane that fails in a step is not tested for clearing in that step. A threshold of 0 never fires (clear = 0: a permanent failure; onset
 * all zero: never fails); 0xFFFFFFFF fires on all but one word in 2^32, so "always" is not expressible. The state AFTER the step of tick k (solve j) is the state
 * DURING it: a lane can be failed at tick 0 from state 0.
 * fault_proc: lanes = m, one step per control tick k = 0 .. T-1, ticks inside a solve period included. The row (k, b, l) the plant reads (as a row of
 * sdempc_fault_cfg::fault) is, in state 0, the scheduled row if fault_cfg gives a schedule as well, else (1, 0); in state s' > 0 it is modes[l][s'-1] = (kappa, beta).
 * No arithmetic is done on the rows. It makes the run a faulted one. The state is two int32 per motor, (s, first): first = tick0 + k of the first step that left
 * state 0, or -1. drop_proc: one lane, K = 1, one step per solve j, valid or not, before the measurement is formed; the solve's valid flag is (s' == 0), ANDed with
 * the scheduled flag if sdempc_obs_cfg::valid is given as well. The state is (s, n_dropped), n_dropped the solves with s' = 1. It makes the run an observed one: it
 * needs an obs cfg, whose pointers may all be NULL, and obs_keys, whose chain it does not touch. Neither chain touches any other chain of the run.
 * fault_rows / valid_rows are per-row outputs (the rows as the plant / the measurement read them): NULL means neither copied back nor scattered. The *_next outputs
 * continue a chain bit for bit when carried back in as keys / state_in: the fault chain for any T (pass tick0 + T as the next tick0), the dropout chain when T is a
 * multiple of solve_period. Checked before the first HIP call and before everything else, in this order: SDEMPC_EINVAL for a new output without its cfg; then for
 * fault_proc a wrong struct_size, n_modes outside 1 .. 4, batch not 1 or B, a NULL onset, clear, modes or keys, an onset row that decreases, a non-finite mode entry,
 * a state_in with s outside 0 .. n_modes or first < -1, tick0 < 0 or tick0 + T >= 2^24; then for drop_proc a wrong struct_size, batch not 1 or B, a NULL drop, recover
 * or keys, a state_in with s outside 0 .. 1 or n_dropped < 0; then drop_proc without obs_keys; then everything sdempc_closed_loop_batch_tracked refuses. No ABI version
 * change: detect the entry point by its symbol. */
typedef struct sdempc_fault_process_cfg {
    int32_t struct_size;      /* sizeof(sdempc_fault_process_cfg) */
    int32_t n_modes;          /* K, 1 .. 4 */
    int32_t batch;            /* rows of onset / clear / modes: 1 or B */
    const uint32_t* onset;    /* [batch][m][K] cumulative, nondecreasing along K */
    const uint32_t* clear;    /* [batch][m][K] */
    const float* modes;       /* [batch][m][K][2] (kappa, beta), finite */
    const uint32_t* keys;     /* [B][2] the fault chain */
    const int32_t* state_in;  /* [B][m][2] (s, first) or NULL: (0, -1) */
    int32_t tick0;            /* global tick of the call's first tick, >= 0 */
} sdempc_fault_process_cfg;
typedef struct sdempc_dropout_process_cfg {
    int32_t struct_size;      /* sizeof(sdempc_dropout_process_cfg) */
    int32_t batch;            /* rows of drop / recover: 1 or B */
    const uint32_t* drop;     /* [batch] threshold of dropping out */
    const uint32_t* recover;  /* [batch] threshold of recovering */
    const uint32_t* keys;     /* [B][2] the dropout chain */
    const int32_t* state_in;  /* [B][2] (s, n_dropped) or NULL: (0, 0) */
} sdempc_dropout_process_cfg;
int sdempc_closed_loop_batch_events(sdempc_handle* h, const sdempc_fault_process_cfg* fault_proc /*or NULL*/, const sdempc_dropout_process_cfg* drop_proc /*or NULL*/,
                                    const sdempc_track_cfg* track /*or NULL*/,
                                    const sdempc_process_cfg* dist_proc /*or NULL, W = 6*/, const sdempc_process_cfg* bias_proc /*or NULL, W = 12*/,
                                    const sdempc_score_cfg* score /*or NULL*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                    const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                    const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                    const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*or NULL*/,
                                    const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                    const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                    const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                    const float* xref /*NULL with track*/, int32_t xref_solves /*0 with track*/, int32_t xref_batch,
                                    const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                    const float* u_act_in /*[B][m] or NULL*/,
                                    float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                    sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                    float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                    uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                    const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                    float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                    float* rate_tail_next /*[B][H][3] or NULL*/,
                                    float* xsub /*[B][T * substeps][13] or NULL*/,
                                    float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                    float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/,
                                    float* dist_rows /*[B][T][6] or NULL*/, uint32_t* dist_keys_next /*[B][2] or NULL*/, float* dist_state_next /*[B][6] or NULL*/,
                                    float* bias_rows /*[B][Ns][12] or NULL*/, uint32_t* bias_keys_next /*[B][2] or NULL*/, float* bias_state_next /*[B][12] or NULL*/,
                                    float* fault_rows /*[B][T][m][2] or NULL*/, uint32_t* fault_keys_next /*[B][2] or NULL*/, int32_t* fault_state_next /*[B][m][2] or NULL*/,
                                    int32_t* valid_rows /*[B][Ns] or NULL*/, uint32_t* valid_keys_next /*[B][2] or NULL*/, int32_t* valid_state_next /*[B][2] or NULL*/);

/* ---- batched closed loop flown by the geometric baseline controller (SPEC.md §11l) -------------------
 * sdempc_closed_loop_batch_events with the solve of every solve period, and nothing else, replaced by a geometric tracking controller evaluated on the device: PD
 * position feedback with a clip on the norm of the acceleration, a desired attitude from the desired acceleration and the reference heading, the SO(3) attitude
 * error as body-rate commands and a collective thrust. It publishes what the rate loop of sdempc_closed_loop_batch_rate consumes, so `rate` is required and its
 * motor_weight must be 0. Key schedule (the split that feeds the solve's noise still happens; the noise is not drawn), measured / aged state, reference window (xref
 * or track), plant, rate loop, lag, delay, period, scenario, faults, processes, events, score, chunking and continuation are that entry point's, untouched: the same
 * keys and processes fly the MPC through it and the baseline through this one, and the two score arrays are a paired comparison.
 * Per episode and solve, all in float32, every product and fma as written (SPEC.md §11l fixes the order; rsqrt is the software form of SPEC.md §3.2 whatever the
 * handle's math_mode; R(q) is SPEC.md §5.2's): x = (p, v, q, w) the state the solve would have started from (the plant's, or the estimate xm), w0 / w1 rows ref_row
 * and ref_row + 1 of the episode's window.
 *   e_p = p - p(w0), e_v = v - v(w0);  a_i = -fma(kv_i, e_v_i, kp_i e_p_i);  n2 = fma(a2, a2, fma(a1, a1, a0 a0));  if n2 > amax amax: a = a (amax rsqrt(n2))
 *   ff_i = accel_ff ? (v_i(w1) - v_i(w0)) inv_dt : 0;  d = (a0 + ff0, a1 + ff1, (a2 + ff2) + g)
 *   nd = |d|^2 (same chain);  zb = d rsqrt(nd);  xc = (R00, R10, 0) of R(q(w0));  y = zb x xc;  ny = |y|^2;  yb = y rsqrt(ny);  xb = yb x zb;  Rd = [xb yb zb]
 *   M = Rd^T R(q);  w* = inv_tau (M12 - M21, M20 - M02, M01 - M10)
 *   c = clamp(fma(kT, d . zb_cur, k0), c_lo, c_hi), zb_cur the third column of R(q), the CURRENT attitude
 *   unless nd > 0 and ny > 0 (zero or NaN): w* = 0 and c = clamp(k0, c_lo, c_hi)
 * The period then flies the table uopt[t][l] = c (t < H, l < m), xevol[0] = x, xevol[t][10..12] = w* (t = 1 .. H, every other word 0); info of the solve is
 * (0, stepsize, 0, 0, 0, 0, 0, 0) and the step size is handed through. u_next holds thrust rows.
 * The parameter arrays hold `batch` sets, 1 or B (a campaign can sweep them). inv_dt 0 lets the library form float32(1) / float32(time_steps[ref_row]).
 * Checked before the first HIP call, SDEMPC_EINVAL for: geo NULL or a wrong struct_size, batch not 1 or B, a NULL parameter array, accel_ff other than 0 / 1, ref_row
 * outside [0, H - 1], inv_dt neither 0 nor the value above, a non-finite or negative kp, kv, amax, inv_tau or g, a non-finite kT or k0, c_lo > c_hi or either outside
 * some motor's input_bound, no rate cfg, motor_weight != 0; then everything sdempc_closed_loop_batch_events refuses. Not built (SPEC.md §11l): the quaternion-error
 * mode, rotor drag, feed-through, a controller per plant substep, a baseline that is told of a fault. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_geo_cfg {
    int32_t struct_size;   /* sizeof(sdempc_geo_cfg) */
    int32_t batch;         /* parameter sets: 1 or B */
    const float* kp;       /* [batch][3] position gains, finite and >= 0 */
    const float* kv;       /* [batch][3] velocity gains, finite and >= 0 */
    const float* amax;     /* [batch] clip of |a_fb|, finite and >= 0 */
    const float* inv_tau;  /* [batch] 1 / attitude time constant, finite and >= 0 */
    const float* g;        /* [batch] gravity, finite and >= 0 */
    const float* kT;       /* [batch] thrust per acceleration, finite */
    const float* k0;       /* [batch] thrust offset, finite */
    const float* c_lo;     /* [batch] thrust clamp, inside every motor's input_bound */
    const float* c_hi;     /* [batch] */
    int32_t accel_ff;      /* 1: feed-forward acceleration from the window's velocities */
    int32_t ref_row;       /* 0 .. H - 1 */
    float inv_dt;          /* 0, or float32(1) / float32(time_steps[ref_row]) */
} sdempc_geo_cfg;
int sdempc_closed_loop_batch_baseline(sdempc_handle* h, const sdempc_geo_cfg* geo,
                                        const sdempc_fault_process_cfg* fault_proc /*or NULL*/, const sdempc_dropout_process_cfg* drop_proc /*or NULL*/,
                                      const sdempc_track_cfg* track /*or NULL*/,
                                      const sdempc_process_cfg* dist_proc /*or NULL, W = 6*/, const sdempc_process_cfg* bias_proc /*or NULL, W = 12*/,
                                      const sdempc_score_cfg* score /*or NULL*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                      const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                      const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                      const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*required*/,
                                      const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                      const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                      const float* xref /*NULL with track*/, int32_t xref_solves /*0 with track*/, int32_t xref_batch,
                                      const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                      const float* u_act_in /*[B][m] or NULL*/,
                                      float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                      sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                      float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                      uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                      const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                      float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                      float* rate_tail_next /*[B][H][3] or NULL*/,
                                      float* xsub /*[B][T * substeps][13] or NULL*/,
                                      float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                      float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/,
                                      float* dist_rows /*[B][T][6] or NULL*/, uint32_t* dist_keys_next /*[B][2] or NULL*/, float* dist_state_next /*[B][6] or NULL*/,
                                      float* bias_rows /*[B][Ns][12] or NULL*/, uint32_t* bias_keys_next /*[B][2] or NULL*/, float* bias_state_next /*[B][12] or NULL*/,
                                      float* fault_rows /*[B][T][m][2] or NULL*/, uint32_t* fault_keys_next /*[B][2] or NULL*/, int32_t* fault_state_next /*[B][m][2] or NULL*/,
                                      int32_t* valid_rows /*[B][Ns] or NULL*/, uint32_t* valid_keys_next /*[B][2] or NULL*/, int32_t* valid_state_next /*[B][2] or NULL*/);
/* The controller alone: out[b] = (c, w*[3]) for state x[b] and window xref[b or 0] (Bx 1 or B), with the parameter sets of `geo` (batch 1 or B). For users, and the
 * direct handle on the device code of this section. Checked as above where it applies (no rate cfg is involved: the clamp bounds are still checked). */
int sdempc_geo_command_batch(sdempc_handle* h, const sdempc_geo_cfg* geo, int32_t B, const float* x /*[B][13]*/, const float* xref /*[Bx][H+1][13]*/, int32_t Bx,
                             float* out /*[B][4]*/);

/* ---- batched closed loop with per-row ensemble histories over the episodes, by cohort (SPEC.md §11m) -------------------
 * sdempc_closed_loop_batch_baseline plus a reducer over the EPISODES: for every scored row i = 0 .. R-1 of the call (R = T, or T * substeps with a substep score)
 * and every cohort g < n_cohorts one row of W = SDEMPC_ENSEMBLE_BASE_WORDS + 4 * n_edges 32-bit words, formed on the device from the rows, targets and thresholds
 * the score reads — the survival curve, the failures by cause, and sum / min / max / cumulative edge counts of the score's channels dp, dv, c, w2 — so that the
 * time-resolved curves of a campaign cost R * G * W words of output whatever B is. With `ens` NULL the call IS sdempc_closed_loop_batch_baseline bit for bit, with
 * the same launches (ens_out must then be NULL). `geo` may be NULL here: the episodes are then flown by the MPC's own solves, exactly as
 * sdempc_closed_loop_batch_events flies them (`rate` is then optional again), and the same ensemble cfg reduces both sides of a paired comparison.
 * Per episode b and scored row, with (dp, dv, c, w2, nf, cause) of that row exactly as the score forms them (above, at sdempc_score_cfg): r_b is the row's index — the
 * value score word 0 had before the row was counted, so a run continued through score_in keeps counting — and f_b the episode's score word 8 after the chunk was
 * scored (0xffffffff: never). "Failed before the row" is f_b < r_b, "failed by now" f_b <= r_b, both unsigned. The episode is INCLUDED in the statistics of its cohort when
 * nf = 0 and, with over = 1, it has not failed before the row; over = 0 includes every finite row. The words of (i, g):
 *    0 u32 episodes of the cohort                          3 u32 episodes of the cohort whose row has cause != 0
 *    1 u32 episodes included                               4 .. 7 u32 episodes of the cohort whose row has cause bit 1, 2, 4, 8
 *    2 u32 episodes of the cohort failed by now            8 + 3k + {0, 1, 2} f32 sum, min, max of channel k in (dp, dv, c, w2) over the included episodes
 *   20 + k * n_edges + j u32 included episodes with v_k < edges[k][j]
 * min starts at +inf and v < min replaces it, max starts at -inf and v > max replaces it; no channel can be -0 and finite rows and targets give no NaN, so both are
 * independent of order. A float sum has ONE association: episodes in blocks of 256 consecutive b; in a block, lane l holds v if its episode is included and +0
 * otherwise; per wave of 64 lanes, for d = 1, 2, 4, 8, 16, 32 every lane forms x_l + x_(l xor d); the block sum is (s0 + s1) + (s2 + s3) of its four waves; the
 * total starts at +0 and adds the block sums in ascending order. An empty cohort reads (0, .., +0, +inf, -inf, .., 0). The words do not depend on chunking, on
 * which outputs were requested or on the layout of the solves; they DO depend on B and on the order of the episodes (the sums' association).
 * Checked before the first HIP call, in this order and in front of everything else, SDEMPC_EINVAL for: ens without ens_out or ens_out without ens, a wrong
 * struct_size, n_cohorts outside 1 .. 16, n_edges outside 0 .. 16, over other than 0 / 1, edges NULL with n_edges > 0, a NaN edge, edges of a channel that
 * descend (equal neighbours pass), a cohort entry outside [0, n_cohorts), ens without a score cfg; then everything sdempc_closed_loop_batch_baseline (geo NULL:
 * sdempc_closed_loop_batch_events) refuses. No ABI version change: detect the entry point by its symbol. */
#define SDEMPC_ENSEMBLE_BASE_WORDS 20
typedef struct sdempc_ensemble_cfg {
    int32_t struct_size;     /* sizeof(sdempc_ensemble_cfg) */
    int32_t n_cohorts;       /* G, 1 .. 16 */
    int32_t n_edges;         /* E, 0 .. 16 edges per channel */
    int32_t over;            /* 1: episodes that have not failed before the row ("alive"); 0: every finite row */
    const int32_t* cohort;   /* [B] cohort of each episode, in [0, G); NULL: all 0 */
    const float* edges;      /* [4][E] ascending edges of dp, dv, c, w2; may be NULL with E = 0 */
} sdempc_ensemble_cfg;
int sdempc_closed_loop_batch_ensemble(sdempc_handle* h, const sdempc_ensemble_cfg* ens /*or NULL*/, uint32_t* ens_out /*[R][G][W]; NULL without ens*/,
                                      const sdempc_geo_cfg* geo /*or NULL: the MPC*/,
                                        const sdempc_fault_process_cfg* fault_proc /*or NULL*/, const sdempc_dropout_process_cfg* drop_proc /*or NULL*/,
                                      const sdempc_track_cfg* track /*or NULL*/,
                                      const sdempc_process_cfg* dist_proc /*or NULL, W = 6*/, const sdempc_process_cfg* bias_proc /*or NULL, W = 12*/,
                                      const sdempc_score_cfg* score /*or NULL*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                      const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                      const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                      const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*required with geo*/,
                                      const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                      const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                      const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                      const float* xref /*NULL with track*/, int32_t xref_solves /*0 with track*/, int32_t xref_batch,
                                      const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                      const float* u_act_in /*[B][m] or NULL*/,
                                      float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                      sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                      float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                      uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                      const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                      float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                      float* rate_tail_next /*[B][H][3] or NULL*/,
                                      float* xsub /*[B][T * substeps][13] or NULL*/,
                                      float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                      float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/,
                                      float* dist_rows /*[B][T][6] or NULL*/, uint32_t* dist_keys_next /*[B][2] or NULL*/, float* dist_state_next /*[B][6] or NULL*/,
                                      float* bias_rows /*[B][Ns][12] or NULL*/, uint32_t* bias_keys_next /*[B][2] or NULL*/, float* bias_state_next /*[B][12] or NULL*/,
                                      float* fault_rows /*[B][T][m][2] or NULL*/, uint32_t* fault_keys_next /*[B][2] or NULL*/, int32_t* fault_state_next /*[B][m][2] or NULL*/,
                                      int32_t* valid_rows /*[B][Ns] or NULL*/, uint32_t* valid_keys_next /*[B][2] or NULL*/, int32_t* valid_state_next /*[B][2] or NULL*/);

/* ---- batched closed loop that retires failed episodes and solves only the live set (SPEC.md §11n) -----------------------
 * sdempc_closed_loop_batch_ensemble with one more rule: an episode whose score records a failure (word 8 != 0xffffffff, from this call's rows or from score_in) is
 * RETIRED at the next solve-period boundary. With `retire` NULL the call IS sdempc_closed_loop_batch_ensemble bit for bit, with the same launches (retired_at and
 * live_per_solve must then be NULL). Per solve j of the call: live_0(b) = word 8 of score_in[b] is all ones (no score_in: every episode); live_{j+1}(b) = live_j(b)
 * and word 8 is still all ones after period j's rows were scored. It depends on the rows alone — not on chunking, B or the outputs requested.
 *  - A live episode is solved as ever, in a dense batch of n_live_j instances (results do not depend on an instance's position or the batch size).
 *  - A retired episode gets no solve: its uopt / xevol tables stay as they are and its info row of that solve is (0, stepsize, 0, 0, 0, 0, 0, 0), so the step size is
 *    held. The plant launch, the key schedule, the observation, process and event chains, the history and the windows run over all B as ever (the solve's subkey is
 *    split and not used). At the call's entry every episode's uopt table is the warm start (u_init, or uref tiled) and every row of its xevol table is x0[b]: an
 *    episode retired at entry flies that, whatever the handle did before.
 *  - Scoring runs once per PERIOD: period j's rows, us rows and info row are scored for episode b only where live_j(b); a retired episode's 16 words are frozen at
 *    the end of the period of its first failure. An episode that never fails has every word and every row bit-identical to the call without `retire`.
 *  - With `geo` the controller skips retired episodes by the same mask (nothing is compacted); their info rows are the held ones.
 *  - An ensemble cfg must have over = 1: the rows of a retired episode are not a fleet statistic, and over = 1 leaves them out.
 * retired_at[b]: the first solve index of THIS call at which b was not solved (0: retired at entry), -1: none (an episode failing in the call's last period is
 * retired by the next call). live_per_solve[j] = n_live_j. A run cut in two through score_in and the *_next outputs composes: the second call's score words, keys
 * and chains are the single call's, its retired_at counts from its own first solve, and every row of an episode live at the cut is the single call's; an episode
 * retired before the cut agrees through its failing period and flies the second call's entry tables behind the cut (its held tables are not carried across calls).
 * Checked before the first HIP call, in this order and in front of everything else, SDEMPC_EINVAL for: retire without retired_at / live_per_solve or either of them
 * without retire, a wrong struct_size, reserved != 0, retire without a score cfg, retire with an ensemble cfg whose over is 0; then everything
 * sdempc_closed_loop_batch_ensemble refuses. No ABI version change: detect the entry point by its symbol. */
typedef struct sdempc_retire_cfg {
    int32_t struct_size;     /* sizeof(sdempc_retire_cfg) */
    int32_t reserved;        /* 0 */
} sdempc_retire_cfg;
int sdempc_closed_loop_batch_retire(sdempc_handle* h, const sdempc_retire_cfg* retire /*or NULL*/, int32_t* retired_at /*[B]; NULL without retire*/,
                                    int32_t* live_per_solve /*[Ns]; NULL without retire*/,
                                    const sdempc_ensemble_cfg* ens /*or NULL*/, uint32_t* ens_out /*[R][G][W]; NULL without ens*/,
                                    const sdempc_geo_cfg* geo /*or NULL: the MPC*/,
                                    const sdempc_fault_process_cfg* fault_proc /*or NULL*/, const sdempc_dropout_process_cfg* drop_proc /*or NULL*/,
                                    const sdempc_track_cfg* track /*or NULL*/,
                                    const sdempc_process_cfg* dist_proc /*or NULL, W = 6*/, const sdempc_process_cfg* bias_proc /*or NULL, W = 12*/,
                                    const sdempc_score_cfg* score /*required with retire*/, const uint32_t* score_in /*[B][16] or NULL*/,
                                    const sdempc_age_cfg* age_cfg /*or NULL*/, const float* xhist_in /*[B][age_max][13] or NULL*/,
                                    const sdempc_obs_cfg* obs /*or NULL*/, const uint32_t* obs_keys /*[B][2]; NULL without obs*/, const float* xmeas_in /*[B][13] or NULL*/,
                                    const sdempc_fault_cfg* fault_cfg /*or NULL*/, const sdempc_rate_cfg* rate /*required with geo*/,
                                    const sdempc_scenario_cfg* scenario /*or NULL*/, const sdempc_timing_cfg* timing, const sdempc_plant_cfg* pc,
                                    const void* const* plant_blobs /*[num_plants]*/, const size_t* plant_blob_bytes /*[num_plants]*/,
                                    const int32_t* plant_of /*[plant_ticks][B] or NULL*/, int32_t B, int32_t T, const float* x0,
                                    const float* xref /*NULL with track*/, int32_t xref_solves /*0 with track*/, int32_t xref_batch,
                                    const uint32_t* keys, const float* u_init /*or NULL*/, const float* stepsize_in /*or NULL*/,
                                    const float* u_act_in /*[B][m] or NULL*/,
                                    float* xs /*[B][T+1][13]; may be NULL with score*/, float* us /*[B][T][m]; may be NULL with score*/,
                                    sdempc_info* info /*[B][Ns]; may be NULL with score*/,
                                    float* u_next /*[B][H][m] or NULL*/, float* stepsize_next /*[B] or NULL*/,
                                    uint32_t* keys_next /*[B][2] or NULL*/, float* u_act_next /*[B][m] or NULL*/,
                                    const float* rate_integ_in /*[B][3] or NULL*/, const float* rate_tail_in /*[B][H][3] or NULL*/,
                                    float* ws /*[B][T][4]; NULL without rate; may be NULL with score*/, float* rate_integ_next /*[B][3] or NULL*/,
                                    float* rate_tail_next /*[B][H][3] or NULL*/,
                                    float* xsub /*[B][T * substeps][13] or NULL*/,
                                    float* xmeas /*[B][Ns][13] or NULL*/, uint32_t* obs_keys_next /*[B][2] or NULL*/, float* xmeas_next /*[B][13] or NULL*/,
                                    float* xhist_next /*[B][age_max][13] or NULL*/, uint32_t* score_out /*[B][16]; NULL without score*/,
                                    float* dist_rows /*[B][T][6] or NULL*/, uint32_t* dist_keys_next /*[B][2] or NULL*/, float* dist_state_next /*[B][6] or NULL*/,
                                    float* bias_rows /*[B][Ns][12] or NULL*/, uint32_t* bias_keys_next /*[B][2] or NULL*/, float* bias_state_next /*[B][12] or NULL*/,
                                    float* fault_rows /*[B][T][m][2] or NULL*/, uint32_t* fault_keys_next /*[B][2] or NULL*/, int32_t* fault_state_next /*[B][m][2] or NULL*/,
                                    int32_t* valid_rows /*[B][Ns] or NULL*/, uint32_t* valid_keys_next /*[B][2] or NULL*/, int32_t* valid_state_next /*[B][2] or NULL*/);


/* After the stream of the last sdempc_solve_batch_dev call has been synchronised: SDEMPC_OK, or SDEMPC_EDEVICE when a grid barrier of
 * a cooperative layout gave up (results of that call invalid, telemetry NaN). The handle then stays off the cooperative layouts, so
 * repeating the call runs in the one-workgroup-per-instance layout. Also SDEMPC_EDEVICE when a large throughput launch that hands its
 * instances out by ticket (three rounds of the persistent grid or more) ended with a ticket count other than the one the host expects:
 * instances of that launch may then be unsolved (the handle re-synchronises itself; repeat the call). Such launches are issued one at a
 * time per handle, in order, and cannot be captured into a hipGraph (the launch carries the ticket base of its own moment). New in this
 * build (no reference counterpart: the reference's solver call, sde_control.py:405-416, either returns or kills the process). */
int sdempc_solve_status(sdempc_handle* h);
/* Number of times this handle left the cooperative layouts because a grid barrier gave up (0 in normal operation). */
int32_t sdempc_layout_fallbacks(const sdempc_handle* h);

/* Work the solve launches of this handle have actually done since creation (or the last reset), summed over instances:
 * out[0] solves, out[1] gradient evaluations (forward + adjoint sweep), out[2] forward-only rollouts (line-search trials, the
 * initial-cost and the final mean-trajectory rollout; every trial is counted, so out[2] is sum(info[7]) + 2 per solve), out[3] the
 * number of those trials that were settled without a rollout: with every cost weight of the handle >= 0 a cost cannot be negative, so a
 * trial whose Armijo bound fma(ls_coef, g.d, c_y) is negative is rejected unevaluated unless it is the last trial of its line search
 * (SPEC.md §8; results are unchanged). The rollouts actually run are out[2] - out[3]. An iteration whose extrapolation point did not move re-uses
 * its gradient instead of evaluating it again, so out[1] can be below the sum of the iteration counts. Counted by the
 * one-team-per-instance and plain cooperative layouts (the speculative latency layout evaluates extra, discarded rollouts and is
 * not counted). Call after the stream of the last solve has been synchronised. Roofline accounting of bench.py. */
int sdempc_work_counters(sdempc_handle* h, uint64_t out[4], int32_t reset);

/* Name of the kernel instantiation the last *_dev launch of this handle started, as a profiler prints it (demangled, without the
 * argument list), e.g. "sdempc::exact::sdempc_solve_kernel<sdempc::exact::TeamBlock, 4, false, false, 0, false>"; empty before the first
 * launch. For bench.py's roofline record and for matching rocprofv3 kernel traces. */
int sdempc_last_kernel_name(const sdempc_handle* h, char* buf, size_t n);

/* Times the last *_dev launch on its own stream with HIP events (ms); <0 if unavailable. */
float sdempc_last_kernel_ms(const sdempc_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* SDEMPC_H */
