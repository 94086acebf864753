/*
 * slam_hip.h -- C-ABI of libslam_hip.so, the MI355X (gfx950) implementation of
 * the per-step SLAM state-estimation hot path of takuyani/SLAM-Robot_Simu.
 *
 * The reference is pure Python/NumPy with no FFI of its own; these entry points
 * are what a ctypes binding of its estimator classes binds.
 * Every function below names the reference interface it replaces.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Host buffers are caller-owned and are only
 *     read/written during the call; device memory is owned by the handle.
 *   - Return 0 on success, a negative SLAM_ERR_* code on failure;
 *     slam_last_error() (thread-local) describes the last failure.
 *   - A handle is not thread-safe (the reference is single-threaded).
 *   - All arithmetic is IEEE fp64, as in the reference.
 */
#ifndef SLAM_HIP_H
#define SLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_OK 0
#define SLAM_ERR_ARG (-1)
#define SLAM_ERR_HIP (-2)
/* particle_filter.py:219: a resample position beyond the last cumulative
 * weight raises IndexError in the reference; the device clamps to NP-1 and
 * reports this code from the call that hit it. */
#define SLAM_ERR_INDEX (-3)
#define SLAM_ERR_STATE (-4)
/* slam_graph_optimize: the PCG solve of an iteration did not converge within
 * pcg_max_iter (the dense path's singular gate is not an error: is_calc = 0
 * ends the loop as in graph_based_slam.py:706-709). */
#define SLAM_ERR_SOLVE (-5)
#define SLAM_ERR_COMM (-6)

int slam_version(void);
const char* slam_last_error(void);
int slam_device_count(int* n);

/* ====================================================================
 * Particle filter -- replaces ParticleFilter (particle_filter.py:18-237)
 * ==================================================================== */
typedef struct slam_pf slam_pf;

enum { SLAM_MOTION_LINEAR = 0,     /* particle_filter.py:121-142 (x' = A x + B u) + N(0,Q) */
       SLAM_MOTION_VELOCITY = 1 }; /* motion_model.py:31-62 (sample_motion_model_velocity) */
enum { SLAM_LIK_PRODUCT = 0,       /* particle_filter.py:185-192: sequential product of NL densities */
       SLAM_LIK_LOGSUM = 1 };      /* same density as exp(-sum(q)/2) * den^-NL (one exp per particle) */

typedef struct {
    double dt;            /* particle_filter.py:30  DT_s = period_ms / 1000 */
    double ess_threshold; /* particle_filter.py:33  ESS_TH = NP / 100 */
    double r_cov[4];      /* particle_filter.py:68-70 R (2x2, row-major) */
    double q_factor[9];   /* device-RNG noise map: noise_j = sum_k g_k q_factor[3k+j]
                             (numpy: sqrt(s)[:,None]*v of svd(Q), particle_filter.py:165) */
    double alphas[6];     /* motion_model.py:20-29 a1..a6 (velocity motion model) */
    double x0[3];         /* particle_filter.py:74-81 initial pose of every particle */
    uint64_t seed;        /* device RNG (Philox-4x32-10) key */
    int32_t motion;       /* SLAM_MOTION_* */
    int32_t likelihood;   /* SLAM_LIK_* */
} slam_pf_config;

typedef struct {
    double x_est[3];      /* particle_filter.py:117  px[:, argmax] */
    double cov[9];        /* weighted particle covariance (np.cov(px, aweights=pw, bias=True)) */
    double max_val;       /* particle_filter.py:115 */
    double ess;           /* 1 / sum(w^2) of the normalised weights after this step */
    double weight_sum;    /* particle_filter.py:234 np.sum before normalisation */
    int64_t max_idx;      /* particle_filter.py:116 (first index on ties) */
    int32_t resampled;    /* this step ran the resampling branch (particle_filter.py:211) */
    int32_t resample_next;/* ess < ESS_TH: the next step will resample */
    int32_t status;       /* bit0: resample clamp (reference IndexError); bit1: exact-scan fallback */
    int32_t n_special;    /* exact-cumsum diagnostics: sequentially folded elements */
    int32_t ess_near;     /* |ess - ESS_TH| <= band * ESS_TH: the reference's `1 / (pw @ pw.T)`
                             (particle_filter.py:210, BLAS order) could decide resample_next
                             differently; the drop-in confirms such steps on the host */
    int32_t dd_waves;     /* closed-form log-sum: wavefronts that took the double-double form
                             (a sharded step's result: the first held shard's count only) */
} slam_pf_result;

/* ParticleFilter.__init__ (particle_filter.py:21-84).  landmarks: n_landmarks x 2 row-major. */
int slam_pf_create(const slam_pf_config* cfg, int64_t n_particles, int32_t n_landmarks,
                   const double* landmarks, int device, slam_pf** out);
int slam_pf_destroy(slam_pf* h);
int slam_pf_set_landmarks(slam_pf* h, const double* landmarks);
/* Any pointer may be NULL (left unchanged).  Arrays of NP doubles. */
int slam_pf_set_state(slam_pf* h, const double* x, const double* y, const double* th,
                      const double* w);
int slam_pf_get_state(slam_pf* h, double* x, double* y, double* th, double* w);
/* The last step's weights before normalisation (w_un = pw * bn, particle_filter.py:194)
 * and the divisor the device formed for them (np.sum(w_un) in numpy's order,
 * :234; = slam_pf_result.weight_sum of that step; 1 after set_state / resample).
 * The current weights are w_un / s (:235, NaN -> 1/NP).  Either pointer may be
 * NULL.  Lets a caller pin the step-end np.sum and the reductions against
 * numpy on the device's own w_un.  Every handle keeps its weights in this
 * form (a shard: its local w_un). */
int slam_pf_get_weights_raw(slam_pf* h, double* w_un, double* s);

/* One estimator step of main_pf (particle_filter.py:102-117):
 * resampling (if the previous step's ESS < ESS_TH) -> predict -> likelihood ->
 * normalise -> estimate.
 *   control:  (v, omega)                         (particle_filter.py:46-58)
 *   z:        NL x 2 robot-frame observations    (particle_filter.py:151-153)
 *   noise:    NP x 3 host array or NULL.  LINEAR: additive (x, y, yaw) noise =
 *             np.random.multivariate_normal(0, Q, NP) (particle_filter.py:165);
 *             VELOCITY: standard normals in draw order (v, w, gamma) per particle
 *             (motion_model.py:46-48).  NULL: on-device Philox stream.
 *   u_resample: rand() of particle_filter.py:214 (ofs = u / NP); NaN: device RNG. */
int slam_pf_step(slam_pf* h, const double* control, const double* z, const double* noise,
                 double u_resample, slam_pf_result* res);

/* Stage entry points (the reference's private methods). */
int slam_pf_resample(slam_pf* h, double u_resample, int32_t force, int32_t* resampled);  /* __resampling :200-224 */
int slam_pf_predict(slam_pf* h, const double* control, const double* noise);            /* __predict :156-168 */
int slam_pf_update(slam_pf* h, const double* z, slam_pf_result* res);                    /* __likelihood + estimate :113-117 */
/* Exact systematic-resampling indices for the CURRENT weights (idx_out: NP int64). */
int slam_pf_resample_indices(slam_pf* h, double u_resample, int64_t* idx_out, int32_t* n_special);
/* numpy-order np.sum of the current weights (particle_filter.py:234). */
int slam_pf_weight_sum(slam_pf* h, double* sum_out);
/* Diagnostics: the device RNG's six standard normals of particle pairs
 * [p0, p0 + count) at RNG step rstep (the perf-mode motion noise, Philox-4x32-10
 * / Philox-2x32-10 + Box-Muller; not a reference interface), out: count x 6. */
int slam_debug_pair_normals(int device, uint64_t p0, int64_t count, uint32_t rstep, uint64_t seed,
                            double* out);
/* Diagnostics: one routine of csrc/fastmath.hpp run on the device, one lane per
 * argument, through the inline function the production kernels call (tables in
 * LDS as production stages them; not a reference interface).  in: n x 4
 * operands, out: n x 2 results; unused operands are ignored, unused results 0.
 *   sin/cos routines:  in (x), out (sin, cos)
 *   ROTATE_SC:         in (s, c, sd, cd), out (sin, cos) of the sum
 *   exp / sqrt:        in (x), out (value)
 *   RNG_*_TAB, RNG_SINCOS2PI: in (the 32-bit word as a double); the uniform is
 *                      (word + 1) 2^-32 as in the Box-Muller pair
 *   RNG_LOG_SCALED:    in (d, e), out log(d 2^e) */
enum { SLAM_MATH_FAST_SINCOS = 0,
       SLAM_MATH_SMALL_SINCOS = 1,
       SLAM_MATH_ROTATE_SC = 2,
       SLAM_MATH_HEADING_SINCOS_TAB = 3,
       SLAM_MATH_EXP_LEAN = 4,
       SLAM_MATH_EXP_TAB = 5,            /* exp_tab<false> */
       SLAM_MATH_EXP_TAB_NONPOS = 6,     /* exp_tab<true> */
       SLAM_MATH_EXP_NHALF = 7,          /* exp_nhalf<false> */
       SLAM_MATH_EXP_NHALF_NONPOS = 8,   /* exp_nhalf<true> */
       SLAM_MATH_SQRT_POS = 9,
       SLAM_MATH_RNG_LOG_TAB = 10,
       SLAM_MATH_RNG_SINCOS2PI_TAB = 11,
       SLAM_MATH_RNG_LOG_SCALED = 12,
       SLAM_MATH_RNG_SINCOS2PI = 13,
       SLAM_MATH_COUNT = 14 };
int slam_debug_math(int device, int32_t fn, int64_t n, const double* in /* n x 4 */,
                    double* out /* n x 2 */);
/* Diagnostics: what this library holds in this process right now, over all
 * handles and the stateless entry points' scratch: out[0] device bytes, out[1]
 * pinned host bytes, out[2] events.  Exact counts kept by the library's one
 * allocator (not a free-memory query, which other users of the card move). */
int slam_debug_live_resources(int64_t out[3]);

/* Device-resident multi-step run (bench path): observations for n_steps steps
 * are uploaded once; steps are enqueued back to back with no host sync.  A
 * run is one setup launch (controls read from pinned host memory, counters,
 * the first step's closed-form words unless the previous run's last step
 * formed them for the same control), the steps' graphs (1/2/4/8-step shapes,
 * binary decomposition of n_steps), and one wait: the last step's finalize
 * stores the batch's result records into pinned host memory itself. */
int slam_pf_load_observations(slam_pf* h, int32_t n_steps, const double* z_all);
int slam_pf_run(slam_pf* h, int32_t first_step, int32_t n_steps, const double* controls,
                slam_pf_result* results);

/* Kernel timing (HIP events on the handle's stream; disables step graphs).
 * kernel: 0 = fused resample-gather+predict+likelihood, 1 = np.sum order
 * sums + normalise + reductions, 2 = exact-cumsum passes, 3 = whole step. */
int slam_pf_enable_timing(slam_pf* h, int32_t on);
int slam_pf_timing(slam_pf* h, int32_t kernel, double* total_ms, int64_t* launches);
/* slam_pf_run replays one captured hipGraph per step (default on). */
int slam_pf_set_graphs(slam_pf* h, int32_t on);
/* Capture every graph slam_pf_run will replay (1-, 2-, 4- and 8-step graphs for
 * both ping-pong parities) without running them, so that no capture lands in
 * a timed run; *capture_ms (may be NULL) = host time spent.  Graphs are
 * dropped (and captured again on demand) by the calls that change a step's
 * launches (set_stream, set_scan_merged, set_ess_band, the device stream). */
int slam_pf_prepare_graphs(slam_pf* h, double* capture_ms);
/* Exact cumsum of a resample step in one launch (on = default where the grid
 * is co-resident; SLAM_ERR_ARG elsewhere) or in two; bit-identical results. */
int slam_pf_set_scan_merged(slam_pf* h, int32_t on);
/* Overrides the resample decision of the next step (particle_filter.py:210-211,
 * `ess < ESS_TH`): the caller re-forms ESS as the reference does, `1 / (pw @ pw.T)`
 * on the host's BLAS, when the device's ESS lies within rounding of the
 * threshold (the device sums in its own fixed order).  Single-GPU handles. */
int slam_pf_set_resample_next(slam_pf* h, int32_t on);
/* Band of slam_pf_result.ess_near, relative to ESS_TH (default 1e-9): the steps
 * whose device ESS lies this close to the threshold, where the reference's BLAS
 * dot (particle_filter.py:210) could order the sum differently. */
int slam_pf_set_ess_band(slam_pf* h, double band);
/* external != 0: run on the caller's HIP stream (e.g. torch.cuda.current_stream();
 * NULL = the default stream).  external == 0: a private stream again. */
int slam_pf_set_stream(slam_pf* h, void* hip_stream, int32_t external);

/* ====================================================================
 * Particle-filter ensemble -- n_filters independent ParticleFilter instances
 * (particle_filter.py:18-237) of n_particles <= 8192 each (the reference's
 * NP = 1000): Monte-Carlo repetitions over seeds or maps, parameter sweeps,
 * one filter per robot.  The filters share NP, NL, the motion model, the
 * likelihood form and dt; landmarks, R, the noise map / alphas, x0, the ESS
 * threshold and the seed are per filter (cfgs[b]).  One workgroup runs one
 * filter's whole step, and a run of any number of steps is one launch.
 * Filter b with device noise draws the stream of a slam_pf created from
 * cfgs[b] (n_global = NP): its particles, weights, np.sum, maximum and
 * estimate are bit-identical to that handle's (SLAM_LIK_PRODUCT; the log-sum
 * form here is the landmark loop, not the closed-form expansion).
 * Arrays carry a leading filter axis.  A filter's resample clamp (the
 * reference's IndexError) sets bit 0 of its record's status and does not fail
 * the call; a flagged exact-cumsum fallback sets bit 1.
 * ==================================================================== */
typedef struct slam_pfb slam_pfb;
/* cfgs: n_filters records; motion, likelihood and dt must agree across them
 * (SLAM_ERR_ARG otherwise).  landmarks: n_filters x n_landmarks x 2.
 * 1 <= n_particles <= 8192, n_landmarks >= 1. */
int slam_pfb_create(const slam_pf_config* cfgs, int32_t n_filters, int32_t n_particles,
                    int32_t n_landmarks, const double* landmarks, int device, slam_pfb** out);
int slam_pfb_destroy(slam_pfb* h);
int slam_pfb_info(slam_pfb* h, int32_t* n_filters, int32_t* n_particles, int32_t* n_landmarks);
/* arrays [n_filters][n_particles]; any pointer may be NULL (left unchanged / not read).
 * Setting w also sets every filter's next resample decision from it (:210-211). */
int slam_pfb_set_state(slam_pfb* h, const double* x, const double* y, const double* th,
                       const double* w);
int slam_pfb_get_state(slam_pfb* h, double* x, double* y, double* th, double* w);
/* like slam_pf_get_weights_raw: w_un [B][NP], s [B] */
int slam_pfb_get_weights_raw(slam_pfb* h, double* w_un, double* s);
/* per-filter override of the next step's resample decision: flags[B], -1 keeps the device's */
int slam_pfb_set_resample_next(slam_pfb* h, const int32_t* flags);
int slam_pfb_set_ess_band(slam_pfb* h, double band);
/* one step of every filter: control [B][2], z [B][NL][2], noise [B][NP][3] or NULL
 * (device RNG), u_resample [B] or NULL (NaN entries / NULL: device RNG), res [B] */
int slam_pfb_step(slam_pfb* h, const double* control, const double* z, const double* noise,
                  const double* u_resample, slam_pf_result* res);
/* device-resident: z_all [n_steps][B][NL][2]; controls [n_steps][B][2] (the steps of
 * this call); results [n_steps][B].  One launch per run call, no hipGraph. */
int slam_pfb_load_observations(slam_pfb* h, int32_t n_steps, const double* z_all);
int slam_pfb_run(slam_pfb* h, int32_t first_step, int32_t n_steps, const double* controls,
                 slam_pf_result* results);
/* exact systematic-resampling indices of every filter's CURRENT weights: idx [B][NP]
 * (u_resample as in slam_pfb_step).  SLAM_ERR_INDEX, with the indices filled and
 * clamped, when a filter's position lies beyond its last cumulative weight. */
int slam_pfb_resample_indices(slam_pfb* h, const double* u_resample, int64_t* idx_out);
/* HIP-event time of the last step / run call (ms) and its launches (always 1) */
int slam_pfb_timing(slam_pfb* h, double* ms, int64_t* launches);

/* ====================================================================
 * MotionModel -- replaces motion_model.py:14-86 for a batch of poses
 * (batch = 1 is the reference's single call).
 *   params:  dt, a1..a6                                   (motion_model.py:20-29)
 *   poses:   n x 3 (x, y, theta) host array; out: n x 3 (may alias poses)
 *   normals: n x 3 standard normals, per pose in the draw order (v, w, gamma)
 *            of moveWithNoise (:46-48; the std handed to normal() is sigma**2,
 *            kept); NULL: moveWithoutNoise (:64-86).
 * ==================================================================== */
int slam_motion_velocity(const double* params, int64_t n, const double* poses, double v, double w,
                         const double* normals, double* out, int device);

/* ====================================================================
 * RCCL communicator (one process per GPU).  RCCL is loaded at run time
 * (dlopen librccl.so.1); slam_comm_unique_id on one rank, the 128 bytes
 * broadcast by the caller's bootstrap, slam_comm_create on every rank.
 * ==================================================================== */
typedef struct slam_comm slam_comm;
int slam_comm_unique_id(uint8_t* id_out /* 128 bytes */);
int slam_comm_create(const uint8_t* id, int32_t world, int32_t rank, int device, slam_comm** out);
int slam_comm_destroy(slam_comm* comm);
int slam_comm_info(slam_comm* comm, int32_t* world, int32_t* rank);
/* recv (host, world * bytes) <- send (host, bytes) of every rank (bootstrap data) */
int slam_comm_all_gather_host(slam_comm* comm, const void* send, void* recv, int64_t bytes);

/* ====================================================================
 * Sharded particle filter, device-resident step (BASELINE config 3).
 * One filter of n_global particles split into contiguous shards; a
 * slam_dist groups the shards this process holds -- all of them (LOCAL:
 * several shards on one GPU, phases enqueued shard by shard on one stream) or
 * one (one process per GPU).  Exchanges are peer-memory pushes into every
 * rank's exchange region (fine-grained HBM, opened by the peers through IPC
 * handles) with device-side signalling; every kernel gates on the device
 * resample flag, so a step needs no host decision and slam_dist_run replays
 * K steps per hipGraph.  Results are identical on every rank and bit-identical
 * to one handle holding all particles (particle_filter.py:102-117).
 * ==================================================================== */
typedef struct slam_dist slam_dist;
/* the standard split: rank r holds [gbase, gbase + n_local) */
int slam_dist_shard_range(int64_t n_global, int32_t world, int32_t rank, int64_t* gbase,
                          int64_t* n_local);
/* a shard handle for slam_dist (device RNG; every shard but the last holds a
 * multiple of 8192 particles) */
int slam_pf_create_dist_shard(const slam_pf_config* cfg, int64_t n_local, int64_t n_global,
                              int64_t gbase, int32_t n_landmarks, const double* landmarks, int device,
                              slam_pf** out);
/* shards: the held shards in rank order (n_held == world: LOCAL, ranks 0..world-1;
 * n_held == 1: rank rank0, connect before stepping).  The shards must outlive it. */
int slam_dist_create(slam_pf** shards, int32_t n_held, int32_t world, int32_t rank0, slam_dist** out);
int slam_dist_destroy(slam_dist* d);
/* bootstrap blob per rank: the exchange region's IPC handle and the GPU's PCI bus id */
int slam_dist_handle_size(int64_t* bytes);
int slam_dist_export(slam_dist* d, void* blob);                 /* n_held x handle size */
/* world x handle size, rank order.  Preflight: every peer GPU must be visible and
 * reachable (hipDeviceCanAccessPeer), else SLAM_ERR_COMM before any IPC mapping. */
int slam_dist_connect(slam_dist* d, const void* all_blobs);
int slam_dist_connect_comm(slam_dist* d, slam_comm* comm);      /* export + RCCL all-gather + connect */
/* Collective exchange instead of the peer-memory stores (the fallback when a peer's
 * region cannot be mapped; replaces connect): every step's record all-gather
 * (particle_filter.py:234 normalisation across shards: the ranks' np.sum buffer
 * partials gathered, then folded in rank order on every rank -- bit-identical to
 * one GPU) and, on resample steps, the specials' and items' exchanges as RCCL
 * all-gathers and grouped send/recv between the step's kernels.  comm: an RCCL
 * communicator of the filter's world (one held shard, rank = comm rank); NULL with
 * every shard held (LOCAL), the collectives then being device copies.  Steps are
 * host-orchestrated (no hipGraphs; the host reads the resample flag each step and
 * the exchanged counts on resample steps). */
int slam_dist_set_collective(slam_dist* d, slam_comm* comm);
/* one step from host inputs (observations staged in slot 0, device RNG) */
int slam_dist_step(slam_dist* d, const double* control, const double* z, slam_pf_result* res);
/* Every wait on a peer is bounded (~2^24 polls); one that expires returns
 * SLAM_ERR_COMM and marks the handle dead: every later step or run of it fails
 * at once with SLAM_ERR_COMM (the shards' exchange state is no longer
 * consistent).  Recover by destroying and recreating every shard and the
 * slam_dist on every rank. */
int slam_dist_load_observations(slam_dist* d, int32_t n_steps, const double* z_all);
int slam_dist_run(slam_dist* d, int32_t first_step, int32_t n_steps, const double* controls,
                  slam_pf_result* results);
/* slam_pf_prepare_graphs for the sharded step (after connect) */
int slam_dist_prepare_graphs(slam_dist* d, double* capture_ms);
/* resample exchange form: 1 = one launch (the default with one held shard whose
 * scan grid is co-resident), 0 = five launches; on < 0 only reports */
int slam_dist_set_merged(slam_dist* d, int32_t on, int32_t* active);

/* ====================================================================
 * EKF localisation -- replaces ExtendedKalmanFilter
 * (extended_kalman_filter.py:17-205) for a batch of independent filters
 * (batch = 1 is the reference's single filter).  State on the device is
 * structure-of-arrays: x[3][batch], P[9][batch] (row-major 3x3).
 * ==================================================================== */
typedef struct slam_ekf slam_ekf;

typedef struct {
    double dt;            /* extended_kalman_filter.py:29  DT_s */
    double vel;           /* :46-48  V (control, also in jacobF :188) */
    double omega;         /* :46     omega */
    double q[9];          /* :62-66  Q (process noise, 3x3) */
    double r[4];          /* :68-70  R (observation noise, 2x2) */
    double x0[3];         /* :74-79  initial estimate */
    double p0[9];         /* :81-84  initial covariance */
    int32_t motion;       /* SLAM_MOTION_LINEAR: the reference's __f / jacobF / Q (:160-194);
                             SLAM_MOTION_VELOCITY: prediction driven by motion_model.py --
                             f = moveWithoutNoise (:64-86), its Jacobian G, and
                             Q = V M V^T from a1..a6 (M = diag(sv^4, sw^4): the std handed
                             to np.random.normal is sigma**2, :43-48) + the gamma yaw term */
    int32_t pad0;
    double alphas[6];     /* motion_model.py:20-29 a1..a6 (VELOCITY) */
} slam_ekf_config;

/* ExtendedKalmanFilter.__init__: every filter starts at (x0, p0). */
int slam_ekf_create(const slam_ekf_config* cfg, int64_t batch, int device, slam_ekf** out);
int slam_ekf_destroy(slam_ekf* h);
int slam_ekf_set_state(slam_ekf* h, const double* x /* batch x 3 */, const double* P /* batch x 9 */);
int slam_ekf_get_state(slam_ekf* h, double* x /* batch x 3 */, double* P /* batch x 9 */);
/* The filter half of main_ekf (extended_kalman_filter.py:108-128): prediction
 * with jacobF, Kalman gain with inv(S), update, limit_angle on the yaw,
 * P = (I - G C) P_m.  control = {v, omega} or NULL for the configured values;
 * z: batch x 2 world positions (:141-146).  Outputs may be NULL. */
int slam_ekf_step(slam_ekf* h, const double* control, const double* z, double* x_hat_m,
                  double* x_hat, double* P);
/* n_steps filter steps in one launch (state stays in registers):
 * z_all: n_steps x batch x 2; x_hat_all: n_steps x batch x 3 or NULL;
 * the final state is kept in the handle. */
int slam_ekf_run(slam_ekf* h, int32_t n_steps, const double* control, const double* z_all,
                 double* x_hat_all);
/* Device-resident variant (bench path): z_dev / x_hat_dev are device pointers
 * (x_hat_dev may be NULL); asynchronous on the handle's stream. */
int slam_ekf_run_device(slam_ekf* h, int32_t n_steps, const double* control, const double* z_dev,
                        double* x_hat_dev);
/* Bench path without foreign device buffers: upload n_steps x batch x 2
 * observations once, then run them from HBM (asynchronous; the estimates of
 * every step are kept on the device when keep_history != 0). */
int slam_ekf_load_observations(slam_ekf* h, int32_t n_steps, const double* z_all);
int slam_ekf_run_loaded(slam_ekf* h, int32_t n_steps, const double* control, int32_t keep_history);
int slam_ekf_synchronize(slam_ekf* h);

/* ====================================================================
 * EKF-SLAM (BASELINE config 4, an extension: the reference has no EKF-SLAM).
 * State mu = (robot x, y, yaw, landmark_0 x, y, phi, ...), n = 3 + 3 * n_lm;
 * P is n x n fp64 in HBM (7.2 GB at n = 30,003).  Robot motion is the
 * reference EKF's model (extended_kalman_filter.py:160-194); the landmark
 * measurement is graph_based_slam.py's ScanSensor (range, bearing,
 * orientation; :150-153) with its covariance (:187-194).
 * ==================================================================== */
typedef struct slam_ekfslam slam_ekfslam;

typedef struct {
    double dt;            /* motion step (s) */
    double q_robot[9];    /* robot process noise */
    double r_dist;        /* ScanSensor range noise fraction  (graph_based_slam.py:187-192) */
    double r_dir;         /* bearing noise (rad) */
    double r_orient;      /* orientation noise (rad) */
    int32_t motion;       /* robot motion: SLAM_MOTION_LINEAR (+ q_robot) or SLAM_MOTION_VELOCITY
                             (motion_model.py, as slam_ekf_config.motion; q_robot unused) */
    int32_t pad0;
    double alphas[6];     /* motion_model.py a1..a6 (VELOCITY) */
} slam_ekfslam_config;

int slam_ekfslam_create(const slam_ekfslam_config* cfg, int64_t n_landmarks, int device,
                        slam_ekfslam** out);
int slam_ekfslam_destroy(slam_ekfslam* h);
/* mu: n; P: n x n row-major (only the lower triangle is read). */
int slam_ekfslam_set_state(slam_ekfslam* h, const double* mu, const double* P);
/* mu: n; P <- diag(p_diag) (n values) without an n x n host buffer. */
int slam_ekfslam_init_diag(slam_ekfslam* h, const double* mu, const double* p_diag);
/* P may be NULL; when given it receives the full symmetric n x n matrix. */
int slam_ekfslam_get_state(slam_ekfslam* h, double* mu, double* P);
/* k rows of the symmetric P (rows[k] indices; out: k x n), O(k n) -- for
 * checking a 7.2 GB P without copying it to the host. */
int slam_ekfslam_get_rows(slam_ekfslam* h, int64_t k, const int64_t* rows, double* out);
/* Prediction: robot pose through the motion model, P <- F P F^T + Q on the
 * robot rows/columns (O(n)). control = {v, omega}. */
int slam_ekfslam_predict(slam_ekfslam* h, const double* control);
/* Batched update with k observed landmarks: ids[k], obs[k x 3] (range,
 * bearing, orientation).  K = P H^T S^-1, mu += K e, P <- P - K (P H^T)^T
 * (a rank-3k update of the lower triangle: the HBM-bound kernel). */
int slam_ekfslam_update(slam_ekfslam* h, int32_t k, const int64_t* ids, const double* obs);
int slam_ekfslam_step(slam_ekfslam* h, const double* control, int32_t k, const int64_t* ids,
                      const double* obs);
/* Device time of the last update (ms): out[5] = {H + P H^T gather, S^-1, K and mu,
 * rank-3k covariance update, 0}. */
int slam_ekfslam_timing(slam_ekfslam* h, double* out);

/* What a handle holds and which kernels its last update launched (recorded
 * where slam_ekfslam_update takes the branch; all three are 0 before the first
 * update). */
enum { SLAM_EKS_RANK_NONE = 0,
       SLAM_EKS_RANK_FRAG_2X4 = 1,     /* fragment-streaming, 8 waves of 32 x 64 (default, M <= 64) */
       SLAM_EKS_RANK_FRAG_2X2 = 2,     /* fragment-streaming, 16 waves of 32 x 32 (SLAM_EKS_KERNEL=frag16) */
       SLAM_EKS_RANK_FRAG_2X4_PF = 3,  /* 2 x 4 with a moved P prefetch (SLAM_EKS_KERNEL=pfmid|pf0, M = 60) */
       SLAM_EKS_RANK_PIPE = 4,         /* pipelined, LDS operands (SLAM_EKS_KERNEL=pipe, M <= 64) */
       SLAM_EKS_RANK_LDS = 5 };        /* LDS-staged in k-chunks of 32 (M > 64) */
enum { SLAM_EKS_APPLY_NONE = 0,
       SLAM_EKS_APPLY_MFMA = 1,        /* K = PH^T S^-1 by MFMA tiles (M <= 64) */
       SLAM_EKS_APPLY_LDS = 2 };       /* one wave per row, S^-1 in LDS (M > 64 or SLAM_EKS_APPLY=lds) */

typedef struct {
    int64_t n;            /* state size 3 + 3 n_landmarks */
    int64_t ld;           /* row pitch of P in doubles */
    int64_t n_pad;        /* n rounded up to the 128-row tile */
    int64_t n_tiles;      /* 128 x 128 tiles of the lower triangle */
    int64_t frag_grid;    /* resident grid of the fragment-streaming rank update */
    int64_t pipe_grid;    /* resident grid of the pipelined rank update */
    int32_t last_m;       /* operand width M = 4 ceil(3k / 4) of the last update */
    int32_t last_rank;    /* SLAM_EKS_RANK_* of the last update */
    int32_t last_apply;   /* SLAM_EKS_APPLY_* of the last update */
    int32_t pad0;
} slam_ekfslam_info_t;

int slam_ekfslam_info(slam_ekfslam* h, slam_ekfslam_info_t* out);

/* --------------------------------------------------------------------
 * EKF-SLAM without ids: maximum-likelihood association, landmark
 * initialisation, a map that grows from nothing (the rule is the
 * one of the associating FastSLAM handles below).
 *
 * An associating handle has a capacity cap (n = 3 + 3 cap) and holds
 * count <= cap landmarks in slots 0..count-1, in creation order; nothing is
 * removed unless the handle prunes (slam_ekfslam_set_pruning, after the
 * FastSLAM pruning block below; off by default) or the caller removes slots by
 * hand (slam_ekfslam_remove).  Rows and columns of P and entries of mu at or
 * beyond n_act = 3 + 3 count are exactly zero and stay so.
 *
 * slam_ekfslam_observe(h, k, obs, assoc_out) takes 0 <= k <= 40 observations
 * (range, bearing, orientation) without identity.  count0 is the count at
 * entry; every score uses the state at entry (the predicted state).
 *  1. Score.  For each observation t in turn and each slot j < count0 not yet
 *     matched in this call: l_tj = -(e^T S^-1 e + ln det S) / 2 - (3/2) ln 2 pi
 *     with e the wrapped innovation of the ScanSensor model and
 *     S = [Hr Hl] P[{r,j},{r,j}] [Hr Hl]^T + R(obs_t[0]) (3 x 3, from the 6 x 6
 *     block of P over the robot and slot j; Hr, Hl, R as in the update).
 *  2. Choose.  The largest score wins, the lowest slot on a tie, a NaN score
 *     never.  Without a candidate, or with l_best < log_p_new, the observation
 *     is new (assoc_out[t] = -1), or dropped when no slot is left (-2).
 *     Otherwise it is matched to that slot (assoc_out[t] = slot), which is then
 *     excluded for the rest of the call.  A slot created in this call is never
 *     a candidate.
 *  3. Update.  The matched observations, in observation order, make one batched
 *     update: slam_ekfslam_update's arithmetic with those slots as ids, over
 *     the active prefix only.  No match, no update.
 *  4. Initialise.  Each new observation, in observation order, from the
 *     posterior mu_r, P of step 3, into slot s = count (count then grows by
 *     one).  With psi = pi/2 - yaw, c = cos psi, s = sin psi, rx = d cos b,
 *     ry = d sin b, dx = c rx + s ry, dy = -s rx + c ry:
 *       mu_s = (x + dx, y + dy, wrap(o - psi)),
 *       G_r = [[1, 0, -dy], [0, 1, dx], [0, 0, 1]],
 *       G_z = [[dx/d, -dy, 0], [dy/d, dx, 0], [0, 0, 1]],
 *       P_s,i = G_r P_r,i for every column i < 3 + 3 s (landmarks initialised
 *       earlier in the same call included), P_ss = G_r P_rr G_r^T + G_z R G_z^T.
 * obs must be finite and the ranges positive, else SLAM_ERR_ARG before any HIP
 * call (slam_ekfslam_check_observations is that check alone, host only).
 * slam_ekfslam_predict touches the active rows only; slam_ekfslam_update on an
 * associating handle checks its ids against count and walks the prefix too.
 * -------------------------------------------------------------------- */
typedef struct {
    double log_p_new;     /* ln of the likelihood below which an observation starts a landmark */
    int32_t record;       /* keep the last call's scores for slam_ekfslam_get_scores */
    int32_t pad;
} slam_ekfslam_assoc_config;

int slam_ekfslam_create_assoc(const slam_ekfslam_config* cfg, const slam_ekfslam_assoc_config* acfg,
                              int64_t capacity, int device, slam_ekfslam** out);
int slam_ekfslam_check_observations(int32_t k, const double* obs);
/* assoc_out (k entries: slot, -1 new, -2 dropped) may be NULL. */
int slam_ekfslam_observe(slam_ekfslam* h, int32_t k, const double* obs, int32_t* assoc_out);
/* slam_ekfslam_predict followed by slam_ekfslam_observe. */
int slam_ekfslam_step_assoc(slam_ekfslam* h, const double* control, int32_t k, const double* obs,
                            int32_t* assoc_out);
int slam_ekfslam_get_count(slam_ekfslam* h, int32_t* count);
/* For placing a state (slam_ekfslam_set_state): the caller keeps the zero tail. */
int slam_ekfslam_set_count(slam_ekfslam* h, int32_t count);
/* The last observe's k x count0 scores (record set), row-major. */
int slam_ekfslam_get_scores(slam_ekfslam* h, double* out);

typedef struct {
    int64_t n_act;        /* 3 + 3 count */
    int64_t tiles;        /* 128 x 128 tiles the last observe's update walked (0: no update) */
    int32_t count;
    int32_t count0;       /* count at the last observe's entry */
    int32_t matched;      /* of the last observe */
    int32_t created;
    int32_t dropped;
    int32_t pad0;
} slam_ekfslam_assoc_info_t;

int slam_ekfslam_assoc_info(slam_ekfslam* h, slam_ekfslam_assoc_info_t* out);
/* Device time of the last observe (ms): out[4] = {scan, assign, update, initialise}. */
int slam_ekfslam_assoc_timing(slam_ekfslam* h, double* out);

/* ====================================================================
 * FastSLAM 1.0 with known data association (an extension: the reference's
 * particle filter localises against a known map); per-particle
 * maximum-likelihood association follows below.  Every particle carries a
 * pose, a weight and, per landmark, a mean (mx, my) and a symmetric 2 x 2
 * covariance (pxx, pxy, pyy) -- one small EKF per particle and landmark.  A
 * step observes any k <= NL landmarks (ScanSensor's range, bearing,
 * orientation; graph_based_slam.py:150-153) with known ids; whether a landmark
 * has been seen is a property of the filter, not of the particle.
 *
 * One step, in the reference's order (particle_filter.py:102-117):
 *   1. resample if the previous step's ESS < ESS_TH: slam_pf's exact systematic
 *      resampling; the gather moves the pose and the map rows of every seen
 *      landmark;
 *   2. predict: slam_pf's (linear or velocity motion, host noise or the
 *      handle's Philox stream with slam_pf's counters);
 *   3. per observation t in the order given (landmark j, z = (d, phi, psi)),
 *      psi_p = pi/2 - theta_p, R = diag((d r_dist)^2, (d sin r_dir)^2):
 *      orientation term (use_orient): e = wrap(psi - wrap(psi_p)),
 *      L_p -= e^2 / (2 (r_dir^2 + r_orient^2));
 *      j unseen: mean = pose + Rot(psi_p)^T (d cos phi, d sin phi), covariance
 *      through the inverse landmark Jacobian, no weight term;
 *      j seen: EKF update with H = d(range, bearing)/d(landmark),
 *      S = H P H^T + R, L_p -= (e^T S^-1 e + ln det S) / 2, K = P H^T S^-1,
 *      mean += K e, P <- P - K S K^T;
 *   4. w_un = w exp(L_p - max_p L_p) (log domain: a product of 300 densities
 *      overflows fp64);
 *   5. slam_pf's step end (np.sum-order sum, normalise, argmax, estimate,
 *      weighted covariance, ESS, resample_next, ess_near) into one
 *      slam_pf_result whose weight_sum is the sum of the shifted w_un.
 * ==================================================================== */
typedef struct slam_fs slam_fs;

typedef struct {
    slam_pf_config pf;    /* dt, ess_threshold, q_factor, alphas, x0, seed, motion;
                             r_cov and likelihood are ignored */
    double r_dist;        /* ScanSensor range noise fraction (graph_based_slam.py:187-192) */
    double r_dir;         /* bearing noise (rad) */
    double r_orient;      /* orientation noise (rad) */
    int32_t use_orient;   /* weigh the observed orientation against the particle's heading */
    int32_t pad0;
} slam_fs_config;

/* The argument rules of one step's observations, without a handle or a device:
 * SLAM_ERR_ARG for k < 0, k > n_landmarks, an id outside [0, n_landmarks), a
 * duplicate id, d <= 0 or a non-finite value.  slam_fs_step, slam_fs_update
 * and slam_fs_load_observations apply the same rules before any HIP call. */
int slam_fs_check_observations(int32_t n_landmarks, int32_t k, const int64_t* ids, const double* obs);

/* 1 <= n_particles <= 2^24, n_landmarks >= 1; the two map halves take
 * 2 x 40 B x n_landmarks x n_particles (SLAM_ERR_HIP when they do not fit). */
int slam_fs_create(const slam_fs_config* cfg, int64_t n_particles, int32_t n_landmarks, int device,
                   slam_fs** out);
int slam_fs_destroy(slam_fs* h);
/* any pointer may be NULL; n_seen: landmarks observed so far */
int slam_fs_info(slam_fs* h, int64_t* n_particles, int32_t* n_landmarks, int32_t* n_seen);

/* x, y, th, w as slam_pf_set_state / slam_pf_get_state */
int slam_fs_set_state(slam_fs* h, const double* x, const double* y, const double* th,
                      const double* w);
int slam_fs_get_state(slam_fs* h, double* x, double* y, double* th, double* w);
int slam_fs_set_resample_next(slam_fs* h, int32_t on);
/* seen[NL] (int32), mean[NP][NL][2], cov[NP][NL][3] (pxx, pxy, pyy) */
int slam_fs_set_maps(slam_fs* h, const int32_t* seen, const double* mean, const double* cov);
/* any pointer may be NULL; unseen landmarks come back as NaN */
int slam_fs_get_maps(slam_fs* h, int32_t* seen, double* mean, double* cov);
/* one particle's map, O(NL): mean[NL][2], cov[NL][3].  The map estimate is
 * the map of slam_pf_result.max_idx, as x_est is its pose. */
int slam_fs_get_map(slam_fs* h, int64_t particle, int32_t* seen, double* mean, double* cov);

/* control (v, omega); k observations: ids[k], obs[k][3] (range, bearing,
 * orientation); noise and u_resample as slam_pf_step. */
int slam_fs_step(slam_fs* h, const double* control, int32_t k, const int64_t* ids, const double* obs,
                 const double* noise, double u_resample, slam_pf_result* res);
/* Stages: resample (force != 0: whatever the flag), predict, map update +
 * weights + step end on the current particles. */
int slam_fs_resample(slam_fs* h, double u_resample, int32_t force, int32_t* resampled);
int slam_fs_predict(slam_fs* h, const double* control, const double* noise);
int slam_fs_update(slam_fs* h, int32_t k, const int64_t* ids, const double* obs,
                   slam_pf_result* res);

/* Multi-step run: the observations of n_steps steps are uploaded once
 * (counts[n_steps]; ids and obs hold the steps' lists one after the other),
 * slam_fs_run steps through [first_step, first_step + n_steps) with the
 * device RNG; results identical to slam_fs_step called in turn (noise NULL,
 * u_resample NaN).  The host reads the resample flag once per step. */
int slam_fs_load_observations(slam_fs* h, int32_t n_steps, const int32_t* counts, const int64_t* ids,
                              const double* obs);
int slam_fs_run(slam_fs* h, int32_t first_step, int32_t n_steps, const double* controls,
                slam_pf_result* results);
/* HIP-event time (ms) of the last step's phases: out[4] = {map gather, predict,
 * map update + weights, step end}; 0 for a phase that did not run. */
int slam_fs_timing(slam_fs* h, double* out);

/* --------------------------------------------------------------------
 * Per-particle maximum-likelihood data association.  A range / bearing
 * sensor returns (d, phi, psi) triples with no identity; an associating
 * handle lets every particle decide for itself which of its own landmarks an
 * observation belongs to.  Particle p holds cnt_p <= cap landmarks in slots
 * 0..cnt_p-1 of its map, in the order it created them; landmarks are never
 * removed unless the handle prunes (slam_fs_set_pruning, below; off by default).
 *
 * A step keeps the order above; resample, predict and the step end are
 * unchanged (the gather moves the counts with the poses, and the map rows
 * below a particle's own count).  The update, for every particle, with cnt0_p
 * the count when the update starts, and for each observation z = (d, phi, psi)
 * in the order given:
 *   1. the orientation term as in step 3 above (use_orient);
 *   2. the candidates are the slots j < cnt0_p that no earlier observation of
 *      this update has matched in this particle (a scan sees each landmark
 *      once; a slot created during this update is never a candidate);
 *   3. l_j = -(e^T S^-1 e + ln det S) / 2 - ln(2 pi), with e, S, H and R of the
 *      known-association update;
 *   4. best = the largest l_j, the lowest slot on a tie;
 *   5. no candidate, or l_best < log_p_new: a new landmark -- slot cnt_p takes
 *      the first-sighting mean and covariance and cnt_p grows by one, or, when
 *      cnt_p == cap, the observation is dropped and the map does not change;
 *      either way L_p += log_p_new;
 *   6. otherwise slot best takes the EKF update and L_p += l_best.
 * Then w_un = w exp(L_p - max_p L_p) and the step end as above.
 *
 * On an associating handle ids must be NULL in slam_fs_step, slam_fs_update
 * and slam_fs_load_observations, and 0 <= k <= SLAM_FS_ASSOC_MAX_OBS (not
 * bounded by cap); d > 0 and finiteness as slam_fs_check_observations; all
 * checked before any HIP call.  slam_fs_set_maps ignores seen (it may be
 * NULL); slam_fs_get_maps and slam_fs_get_map return NaN for slots j >= cnt_p,
 * slam_fs_get_maps reports seen[j] = (j < max_p cnt_p), slam_fs_get_map
 * seen[j] = (j < cnt_p); slam_fs_info reports n_landmarks = cap and n_seen =
 * max_p cnt_p.  Every other entry point works as on any handle.
 * -------------------------------------------------------------------- */
#define SLAM_FS_ASSOC_MAX_OBS 4096

typedef struct {
    double log_p_new;     /* log likelihood of "a landmark not in the map yet" (finite) */
    int32_t record;       /* keep the last update's choices for slam_fs_get_assoc
                             (4 B x k x n_particles written per update) */
    int32_t pad0;
} slam_fs_assoc_config;

/* max_landmarks >= 1 is the capacity cap of every particle's map; beside the
 * two map halves the handle holds 4 B x cap x n_particles of match stamps. */
int slam_fs_create_assoc(const slam_fs_config* cfg, const slam_fs_assoc_config* acfg,
                         int64_t n_particles, int32_t max_landmarks, int device, slam_fs** out);
/* counts[NP], each in [0, cap].  SLAM_ERR_ARG on a known-association handle. */
int slam_fs_set_counts(slam_fs* h, const int32_t* counts);
int slam_fs_get_counts(slam_fs* h, int32_t* counts);
/* out[k][NP], k of the last update (of slam_fs_run: its last step): the slot
 * matched, -1 for a new landmark, -2 for a dropped observation.  SLAM_ERR_ARG
 * unless the handle was created with record != 0.  On a pruning handle the
 * slot numbers are those in force during the update, before the compaction. */
int slam_fs_get_assoc(slam_fs* h, int32_t* out);

/* --------------------------------------------------------------------
 * FastSLAM 2.0: poses drawn from the observation-informed proposal.  A
 * proposal handle has known data association and SLAM_MOTION_LINEAR; instead
 * of drawing the pose from the motion model alone and weighing it against the
 * scan afterwards, every particle filters its pose through the step's scan
 * first and draws from the result.  Q = F^T F of cfg.pf.q_factor,
 * Q[i][j] = sum_k F[3k+i] F[3k+j] (k ascending), formed once at create.
 *
 * One step:
 *   1. resample: exactly as on a known-association handle;
 *   2. proposal, per particle: mu = the noise-free linear motion of the pose
 *      (x + v (dt cos th), y + v (dt sin th), wrap(th + omega dt)), Sigma = Q
 *      (six entries, symmetric), L = 0; then for each observation t in the order
 *      given (landmark j, z = (d, phi, psi)):
 *      orientation (use_orient; seen landmark or not):
 *        e = wrap(psi - wrap(pi/2 - mu_th)), s_o = Sigma_thth + vo
 *        (vo = r_dir^2 + r_orient^2), L -= (e^2 / s_o + ln s_o) / 2, and the
 *        scalar Kalman update with H = (0, 0, -1): col = Sigma[:, th],
 *        k = col / s_o, mu -= k e, Sigma_ab -= k_a col_b (a <= b);
 *      j unseen: nothing more (a first sighting carries no pose information);
 *      j seen: linearised at the current mu and the landmark's prior (m_j, P_j):
 *        dx, dy, q, r, bearing, H_m and R as in step 3 of the 1.0 update with the
 *        pose mu; H_x = [-H_m | (0, -1)^T] (2 x 3); A = Sigma H_x^T (3 x 2);
 *        S = H_m P_j H_m^T + R + H_x A (S_01 from row 0 of H_x);
 *        e = (d - r, wrap(phi - bearing)); L -= (e^T S^-1 e + ln det S) / 2;
 *        K = A S^-1 through the 2 x 2 adjugate; mu += K e;
 *        Sigma_ab -= K_a0 A_b0 + K_a1 A_b1 (a <= b);
 *   3. sample: Lc = the lower Cholesky factor of Sigma (l00 = sqrt(S00),
 *      l10 = S01 / l00, l20 = S02 / l00, l11 = sqrt(S11 - l10^2),
 *      l21 = (S12 - l20 l10) / l11, l22 = sqrt(S22 - l20^2 - l21^2)); the pose is
 *      mu + Lc xi, theta not wrapped (as slam_pf).  noise non-NULL:
 *      xi = noise[p][0..2] -- three STANDARD normals per particle, not the
 *      Q-shaped noise a 1.0 handle takes.  noise NULL: the three normals the
 *      handle's predict would have given the particle at this step (particle 2p
 *      the first three, 2p + 1 the last three of its pair's six); the step
 *      counter advances as in a 1.0 step.  A non-positive pivot is not guarded:
 *      it gives NaN, as any degenerate input;
 *   4. maps, at the sampled pose and per observation in order: the first-sighting
 *      initialisation or the EKF update of step 3 of the 1.0 contract, without
 *      its weight term; then the landmarks are marked seen;
 *   5. w_un = w exp(L - max_p L) and the step end, unchanged.
 * With k = 0 a step is mu + chol(Q) xi with all weights kept.
 *
 * The copies of a resampled particle share mu, Sigma and L, so in the step
 * after a resampling they carry bit-equal weights (the pose noise no longer
 * enters the weight); max_idx is then the first of equals, as np.argmax.
 *
 * slam_fs_step, slam_fs_load_observations / slam_fs_run, slam_fs_resample, the
 * state and map accessors, slam_fs_info and slam_fs_timing work as on a
 * known-association handle.  One launch does steps 2 to 4, so slam_fs_timing's
 * out[1] is motion + proposal + sampling + map update and out[2] the weights
 * alone.  slam_fs_predict and slam_fs_update return SLAM_ERR_ARG: the proposal
 * needs the step's control and scan together.
 * -------------------------------------------------------------------- */
typedef struct {
    int32_t record;       /* keep each step's mu, Sigma for slam_fs_get_proposal
                             (72 B x n_particles written per step) */
    int32_t pad0;
} slam_fs_proposal_config;

/* slam_fs_create's rules; in addition SLAM_ERR_ARG before any HIP call for a
 * NULL cfg, pcfg or out and for cfg->pf.motion != SLAM_MOTION_LINEAR (the
 * velocity model needs a per-particle V M V^T). */
int slam_fs_create_proposal(const slam_fs_config* cfg, const slam_fs_proposal_config* pcfg,
                            int64_t n_particles, int32_t n_landmarks, int device, slam_fs** out);
/* The last step's mu, Sigma and L before sampling: mean[NP][3], cov[NP][6]
 * (00 01 02 11 12 22), L[NP]; any pointer may be NULL.  SLAM_ERR_ARG unless the
 * handle was created by slam_fs_create_proposal with record != 0 and has
 * stepped. */
int slam_fs_get_proposal(slam_fs* h, double* mean, double* cov, double* L);

/* --------------------------------------------------------------------
 * FastSLAM 2.0 without ids: data association under the proposal.  The handle
 * is an associating handle (particle p holds cnt_p <= cap landmarks in slots
 * 0..cnt_p-1) and a proposal handle (Q = F^T F, SLAM_MOTION_LINEAR) at once;
 * the association score marginalises the pose uncertainty of the proposal.
 *
 * One step:
 *   1. resample: exactly as on an associating handle (poses, counts, and the
 *      map rows below the source's count);
 *   2. proposal with association, per particle: mu = the noise-free linear
 *      motion, Sigma = Q, L = 0, cnt0_p = the count at the start, c = cnt0_p;
 *      then for each observation (d, phi, psi) in the order given:
 *      a. the orientation step of the proposal handle (use_orient), unchanged:
 *         s_o, L -= (e^2 / s_o + ln s_o) / 2, the scalar update of mu, Sigma;
 *      b. the candidates are the slots j < cnt0_p that no earlier observation of
 *         this step has matched in this particle (a slot created in this step is
 *         never a candidate);
 *      c. l_j = -(e^T S^-1 e + ln det S) / 2 - ln(2 pi) with e and S of the
 *         proposal handle's seen-landmark step, linearised at the current mu and
 *         the slot's prior (m_j, P_j): A = Sigma H_x^T,
 *         S = H_m P_j H_m^T + R + H_x A -- the associating handle's score with
 *         the pose covariance folded into S (equal to it where Sigma = 0);
 *      d. best = the largest l_j; the comparison is strict, so the lowest slot
 *         wins a tie and a NaN never wins;
 *      e. no candidate, or l_best < log_p_new: L += log_p_new, mu and Sigma do
 *         not change (a first sighting carries no pose information); the choice
 *         is -1 and c += 1 if c < cap, otherwise the choice is -2.  Otherwise
 *         L += l_best, the Kalman update of mu and Sigma with slot best
 *         (K = A S^-1 through the adjugate), the slot is marked matched, and the
 *         choice is best;
 *   3. sample: step 3 of the proposal handle, unchanged (noise non-NULL: three
 *      STANDARD normals per particle);
 *   4. maps at the sampled pose, per observation in order and by the recorded
 *      choice: a slot >= 0 takes the EKF update of that slot without the weight
 *      term, -1 the first-sighting mean and covariance in slot cnt_p and then
 *      cnt_p += 1, -2 nothing.  Step 2 reads every prior before any slot is
 *      rewritten;
 *   5. w_un = w exp(L - max_p L) and the step end, unchanged.
 * With k = 0 a step is mu + chol(Q) xi, with weights and counts kept.  The
 * copies of a resampled particle share mu, Sigma, L, map and choices, so they
 * carry bit-equal weights and max_idx is the first of equals.
 *
 * ids must be NULL and 0 <= k <= SLAM_FS_ASSOC_MAX_OBS.  slam_fs_predict and
 * slam_fs_update return SLAM_ERR_ARG as on a proposal handle.
 * slam_fs_set_counts / get_counts, the map accessors, slam_fs_info,
 * slam_fs_resample and slam_fs_load_observations / slam_fs_run behave as on an
 * associating handle; slam_fs_timing's phases mean what they mean on a proposal
 * handle.  slam_fs_get_proposal works when pcfg->record is set.
 * slam_fs_get_assoc works after any step with k > 0 whatever acfg->record says:
 * the choices stay in memory between the kernel's passes (4 B x k x
 * n_particles; SLAM_ERR_HIP from the step if that does not fit).
 *
 * SLAM_ERR_ARG before any HIP call for a NULL cfg, acfg, pcfg or out, a
 * non-finite log_p_new, max_landmarks < 1, cfg->pf.motion !=
 * SLAM_MOTION_LINEAR, and slam_fs_create's own cases.
 * -------------------------------------------------------------------- */
int slam_fs_create_assoc_proposal(const slam_fs_config* cfg, const slam_fs_assoc_config* acfg,
                                  const slam_fs_proposal_config* pcfg, int64_t n_particles,
                                  int32_t max_landmarks, int device, slam_fs** out);

/* --------------------------------------------------------------------
 * Landmark evidence and removal of unsupported landmarks: an optional mode of
 * both associating handle kinds, off by default (a handle that never turns it
 * on launches what it launched before, with the same arguments).  Each slot
 * j < cnt_p of each particle carries an int32 evidence value ev_p[j].
 *
 * The pruning pass runs after the map update (steps 3 and 4 of the contracts
 * above), on every slam_fs_step and stand-alone slam_fs_update, k = 0
 * included: an empty scan is evidence too.  For particle p let cnt0_p be the
 * count before the update, cnt_p the count after it, and (x, y, th) the
 * particle's current pose (after predict on a slam_fs_create_assoc handle, the
 * sampled pose on a slam_fs_create_assoc_proposal handle).  For every slot
 * j < cnt_p, in slot order:
 *   1. j >= cnt0_p (created by this update): ev = init;
 *   2. an observation of this update matched the slot: ev = min(ev + hit, ev_max);
 *   3. otherwise, with (mx, my) the slot's mean: dx = mx - x, dy = my - y, and
 *      with c, s = cos, sin(pi/2 - th): rx = c dx - s dy, ry = s dx + c dy.
 *      The landmark is in view when dx dx + dy dy <= view_range view_range and,
 *      with use_angle, also ry >= |rx| view_tan; a comparison with a NaN counts
 *      as not in view.  In view: ev -= miss (the value saturates at INT32_MIN);
 *      out of view: unchanged;
 *   4. slots with ev < remove_below are removed: the surviving slots keep their
 *      order and move down to slots 0..cnt'_p-1 with their mean, covariance and
 *      evidence, bit for bit; cnt_p = cnt'_p, and removed_p is the difference.
 * The weights of the step do not depend on the pass.  Resampling gathers the
 * evidence rows with the maps, so the copies of a particle share them.
 * slam_fs_get_assoc's slot numbers are those in force during the update,
 * before the compaction; slam_fs_info, slam_fs_get_counts and the map
 * accessors report the state after the pass.  slam_fs_run equals slam_fs_step
 * in turn, pass included.  slam_fs_timing keeps its four phases: the pass
 * belongs to phase 2, the evidence gather to phase 0.
 *
 * slam_fs_set_pruning may be called between steps any number of times; NULL
 * turns the mode off.  Turning it on (from off) gives every live slot init and
 * clears removed; a call on a handle that is already pruning only replaces the
 * configuration.  The first turning on allocates 2 x 4 B x cap x n_particles
 * of evidence (SLAM_ERR_HIP if that does not fit).  slam_fs_set_counts on a
 * pruning handle resets the live slots to init; slam_fs_set_evidence then
 * overrides.  SLAM_ERR_ARG: a known-association handle, a bad configuration
 * (before any HIP call), and from the three accessors while pruning is off.
 * -------------------------------------------------------------------- */
typedef struct {
    double  view_range;    /* > 0, finite: a landmark counts as in view up to this range of the particle */
    double  view_tan;      /* used when use_angle: in view iff ry >= |rx| * view_tan (ScanSensor's
                              fan of half-angle a: view_tan = tan(pi/2 - a)); not NaN then */
    int32_t use_angle;     /* 0: range only */
    int32_t init, hit, miss;      /* evidence of a new landmark; added on a match; subtracted on
                                     an in-view miss (hit, miss >= 0) */
    int32_t ev_max;        /* evidence saturates here (>= init) */
    int32_t remove_below;  /* a landmark whose evidence is < this after the step is removed
                              (init >= remove_below) */
} slam_fs_prune_config;

/* Host only, like slam_fs_check_observations: SLAM_ERR_ARG for NULL, a
 * non-finite or <= 0 view_range, a NaN view_tan with use_angle, hit < 0 or
 * miss < 0, ev_max < init, init < remove_below. */
int slam_fs_check_prune_config(const slam_fs_prune_config* cfg);
int slam_fs_set_pruning(slam_fs* h, const slam_fs_prune_config* cfg);
/* ev[NP][cap]; the slots j >= cnt_p are ignored by set and 0 from get */
int slam_fs_set_evidence(slam_fs* h, const int32_t* ev);
int slam_fs_get_evidence(slam_fs* h, int32_t* ev);
/* removed[NP]: the last pass's removals per particle (0 before any pass) */
int slam_fs_get_removed(slam_fs* h, int32_t* removed);

/* --------------------------------------------------------------------
 * EKF-SLAM without ids: landmark evidence and removal from the map (DESIGN
 * 11h).  An optional mode of an associating slam_ekfslam handle, off by
 * default: a handle that never turns it on launches what it launched before,
 * with the same arguments.  The configuration is slam_fs_prune_config, checked
 * by slam_fs_check_prune_config: both estimators take the same one.  Each slot
 * j < count carries an int32 evidence value ev[j].
 *
 * The pass runs at the end of every slam_ekfslam_observe and
 * slam_ekfslam_step_assoc, after steps 3 and 4 of the contract above, k = 0
 * included: an empty scan is evidence too.  slam_ekfslam_update with ids leaves
 * the evidence alone.  Let count0 be the count at entry, count the count after
 * the initialisation and (x, y, th) the posterior robot pose mu[0..2].  For
 * every slot j < count, in slot order:
 *   1. j >= count0 (created by this call): ev = init;
 *   2. an observation of this call matched the slot: ev = min(ev + hit, ev_max);
 *   3. otherwise, with (mx, my) = mu[3 + 3 j], mu[4 + 3 j]: dx = mx - x,
 *      dy = my - y, and with c, s = cos, sin(pi/2 - th): rx = c dx - s dy,
 *      ry = s dx + c dy.  The landmark is in view when
 *      dx dx + dy dy <= view_range view_range and, with use_angle, also
 *      ry >= |rx| view_tan; a comparison with a NaN counts as not in view.  In
 *      view: ev -= miss (the value saturates at INT32_MIN); out of view:
 *      unchanged;
 *   4. slots with ev < remove_below are removed.
 * Removal: with keep the surviving old slots in order and
 * idx = [0, 1, 2] + [3 + 3 j + a for j in keep, a in 0..2]: mu' = mu[idx],
 * P' = P[idx][:, idx], ev' = ev[keep], all bit for bit, in place; everything at
 * or beyond the new n_act is exactly zero again in mu and in the rows of the
 * lower triangle that the handle stores (slam_ekfslam_get_state mirrors it),
 * which restores the invariant above.
 *
 * assoc_out keeps the slot numbers in force during the update, before the
 * compaction; slam_ekfslam_get_count, slam_ekfslam_assoc_info, the state
 * accessors and slam_ekfslam_get_evidence report the state after it.  An
 * observation dropped for lack of room stays dropped in that call: the slots
 * the pass frees are there for the next one.
 *
 * slam_ekfslam_set_pruning: NULL turns the mode off; turning it on (from off)
 * gives every live slot init; on a handle that already prunes the call only
 * replaces the configuration.  SLAM_ERR_ARG before any HIP call for a NULL or
 * known-id handle or a bad configuration.  slam_ekfslam_set_count on a pruning
 * handle resets the live slots to init; slam_ekfslam_set_evidence then
 * overrides.  set / get_evidence take int32[cap]: the slots at or beyond count
 * are ignored by set and read 0 from get; SLAM_ERR_ARG while pruning is off.
 *
 * slam_ekfslam_remove(h, n, slots) removes the named slots now, whether the
 * handle prunes or not (their evidence goes with them when it does): a map
 * managed by hand.  slots must be strictly increasing and < count, else
 * SLAM_ERR_ARG before any HIP call; n = 0 is a no-op.
 * -------------------------------------------------------------------- */
int slam_ekfslam_set_pruning(slam_ekfslam* h, const slam_fs_prune_config* cfg);
int slam_ekfslam_set_evidence(slam_ekfslam* h, const int32_t* ev);
int slam_ekfslam_get_evidence(slam_ekfslam* h, int32_t* ev);
int slam_ekfslam_remove(slam_ekfslam* h, int32_t n, const int32_t* slots);

typedef struct {
    int32_t count_before;  /* of the last pass or slam_ekfslam_remove (0 before any) */
    int32_t removed;
    int32_t moved;         /* surviving slots that changed place */
    int32_t first;         /* first removed slot, -1 if none */
    double  evidence_ms;   /* device time of the evidence (or mask) kernel */
    double  compact_ms;    /* ... of the compaction's launches (0: none ran) */
} slam_ekfslam_prune_info_t;

int slam_ekfslam_prune_info(slam_ekfslam* h, slam_ekfslam_prune_info_t* out);

/* ====================================================================
 * Graph-based SLAM -- replaces TrajectoryEstimator's linearise-and-solve
 * (graph_based_slam.py: setPairObs :362-439, updateEstPose :452-514) and
 * the Gauss-Newton loop of Robot.estimateOpticalTrajectory (:685-715).
 * ==================================================================== */
typedef struct slam_graph slam_graph;

/* One pair of half-edges of the same landmark (HalfEdge :259-300), already
 * ordered as setPairObs orders them (:371-384: "bfr" is the earlier time).
 * The estimate of pose_* is linearised; time_* selects the block of H
 * (its rank among the edge set's times, :478-482) and the pose updated. */
typedef struct {
    int64_t time_bfr, pose_bfr, time_aft, pose_aft;
    double obs_bfr[3];    /* Observation (:20-75): distance, direction, orientation */
    double obs_aft[3];
} slam_graph_edge;

enum { SLAM_GRAPH_AUTO = 0,   /* dense up to 2048 unknowns, PCG above */
       SLAM_GRAPH_DENSE = 1,  /* LU: det, cond and the reference's gate (:494-498) */
       SLAM_GRAPH_PCG = 2 };  /* block-Jacobi PCG on the 3x3 block-sparse H (config 5) */

typedef struct {
    double r_dist;        /* ScanSensor range noise gain (setNoiseParam(5,2,2) :604 -> 0.05) */
    double r_dir;         /* bearing sigma (rad) */
    double r_orient;      /* orientation sigma (rad) */
    double anchor;        /* :475  H[0:3,0:3] += anchor * I  (1e4) */
    double det_min;       /* :496  0.1 < det */
    double cond_max;      /* :496  cond < 1e15 */
    double pcg_tol;       /* PCG: relative residual */
    int32_t pcg_max_iter;
    int32_t solver;       /* SLAM_GRAPH_* */
    double cond_tol;      /* PCG path, cond estimate: a side stops when its Ritz value moved
                             less than cond_tol (relative) over 16 iterations (<= 0: 1e-5) */
    int32_t cond_max_iter;  /* estimate iterations cap (<= 0: 3000) */
    int32_t cond_mode;    /* SLAM_GRAPH_COND_* */
} slam_graph_config;

/* The PCG path's gate (:494-496).  SLAM_GRAPH_COND_ESTIMATE: cond = the extreme
 * eigenvalues of H by LOBPCG on a second stream beside the solve, the
 * reference's `cond < cond_max` from a converged estimate, det not formed
 * (NaN).  SLAM_GRAPH_COND_MARGIN (the Python default; formerly named
 * SLAM_GRAPH_COND_CERTIFY): an estimate with margins, NOT a certificate -- the
 * same estimate stops as soon as its Ritz ratio clears cond_max by a factor 100
 * (or converges: a factor 10; a converged estimate inside that band decides
 * by its own value), and the det half is decided from a log-det interval (M
 * the block diagonal of H, P = M^-1/2 H M^-1/2: [log det M + c(a)(tr P^2 - n),
 * log det M]) whose upper end is rigorous and whose lower end holds unless the
 * estimate's lambda_min over-estimates lambda_min(H) by more than 1000x (a =
 * lambda~min / (1000 max tr M_i)); a half neither decides takes the dense
 * path's value when n <= 2048, else the update is not solved and flagged
 * undecided (slam_graph_gate_info).  SLAM_GRAPH_COND_OFF: no gate
 * (cond NaN, the solve's convergence alone). */
enum { SLAM_GRAPH_COND_ESTIMATE = 0, SLAM_GRAPH_COND_OFF = 1, SLAM_GRAPH_COND_MARGIN = 2,
       SLAM_GRAPH_COND_CERTIFY = SLAM_GRAPH_COND_MARGIN /* former name of the same mode */ };

int slam_graph_create(const slam_graph_config* cfg, int device, slam_graph** out);
int slam_graph_destroy(slam_graph* h);
/* TrajectoryEstimator's pose list (mPosesEst): n_poses x 3. */
int slam_graph_set_poses(slam_graph* h, int64_t n_poses, const double* poses);
int slam_graph_get_poses(slam_graph* h, double* poses);
/* The pairs setPairObs received (builds the block structure once). */
int slam_graph_set_edges(slam_graph* h, int64_t n_edges, const slam_graph_edge* edges);
/* Odometry edges (no reference counterpart): pose b ("bfr", the
 * earlier one) tied to pose a ("aft") by a measured relative motion rel = (zx,
 * zy, ztheta) in the axes of pose b, with standard deviations sigma.  With c =
 * cos theta_b, s = sin theta_b, dx = x_a - x_b, dy = y_a - y_b:
 *   err   = (c dx + s dy - zx, -s dx + c dy - zy, wrap(wrap(theta_a - theta_b) - ztheta))
 *   Omega = diag(1/sigma_x^2, 1/sigma_y^2, 1/sigma_theta^2)
 *   J_b   = [[-c, -s, -s dx + c dy], [s, -c, -c dx - s dy], [0, 0, -1]]
 *   J_a   = [[ c,  s, 0], [-s, c, 0], [0, 0, 1]]
 * and the edge's 42 values are those of a landmark edge, in the same order.
 * The record shares its size and its index prefix with slam_graph_edge. */
typedef struct {
    int64_t time_bfr, pose_bfr, time_aft, pose_aft;   /* as slam_graph_edge */
    double rel[3];
    double sigma[3];
} slam_graph_odom;                                     /* 80 bytes */
/* slam_graph_set_edges with n_odom odometry edges behind the landmark pairs:
 * the handle's edge set is the concatenation, landmark edges first, E =
 * n_edges + n_odom columns.  slam_graph_get_system's `blocks`, slam_graph_chi2's
 * per-edge arrays and slam_graph_get_edge_weights are over all E columns in that
 * order, and slam_graph_chi2's totals are those of the whole set (bit-identical
 * from call to call; they depend on (n_edges, n_odom) alone).  Odometry edges
 * are never down-weighted: w = 1 and rho = chi2 under every robust kind (the
 * weights reject wrong pairings, and an odometry edge has no association to get
 * wrong).  A pose that no landmark pair touches but an odometry edge does is
 * among the set's times: it is updated, and slam_graph_marginals covers it.
 * slam_graph_set_edges(h, n, e) is slam_graph_set_edges_odom(h, n, e, 0, NULL):
 * with n_odom = 0 the handle launches the kernels and computes the bits it
 * did before this entry existed.
 *
 * SLAM_ERR_ARG, checked on the host before any HIP call (the handle is left as
 * it was): a NULL handle, a negative count, a NULL array with a positive
 * count, poses not set, a pose / time index out of range, time_bfr == time_aft
 * in an odometry edge, a non-finite rel, and a sigma component that is not
 * finite and > 0. */
int slam_graph_set_edges_odom(slam_graph* h, int64_t n_edges, const slam_graph_edge* edges,
                              int64_t n_odom, const slam_graph_odom* odom);
/* updateEstPose: linearise every edge at the current poses, assemble H and
 * b, gate, solve, update the poses.  stats[4] = {is_calc, sum delta^2, det,
 * cond} (:514).  On the PCG path det is NaN (not formed at this size) and cond
 * is the LOBPCG estimate lambda_max / lambda_min of H (inf when H is not
 * positive definite; NaN with SLAM_GRAPH_COND_OFF): is_calc = 1 means PCG
 * converged with positive curvature and a converged estimate gave cond <
 * cond_max (:496), 0 that the gate rejected H -- including an estimate that
 * reached cond_max_iter unconverged (cond_info status 3: its ratio only bounds
 * cond from below) -- or PCG hit pcg_max_iter (poses unchanged either way). */
int slam_graph_update(slam_graph* h, double* stats);
/* estimateOpticalTrajectory's loop: update until sum delta^2 < delta_sum_th
 * (:692-706) or max_iter; stats: max_iter x 4 (or NULL).  Returns
 * SLAM_ERR_SOLVE (with *n_iter set) when a PCG solve fails to converge. */
int slam_graph_optimize(slam_graph* h, double delta_sum_th, int32_t max_iter, double* stats,
                        int32_t* n_iter);
/* Members (no reference counterpart): many graphs of the dense
 * path's size in one handle, advanced together with one launch per phase.
 * Members are disjoint contiguous ranges of the handle's poses: member m holds
 * poses [pose_off[m], pose_off[m + 1]).  Each is a graph of its own, with its
 * own anchor (on the first of its times), gate, dense solve, sum delta^2 and
 * stopping iteration.  The contract: member m is bit for bit what a stand-alone
 * handle with the same slam_graph_config and robust kind returns that is given
 * member m's poses and member m's edges alone (its landmark pairs in their
 * order, then its odometry edges in theirs) -- the poses, every stats row, the
 * iteration count, delta, the assembled H and b and the edge weights --
 * whatever the other members are, however many there are and in whatever
 * order they stand.
 *
 * slam_graph_set_members: after slam_graph_set_poses and before
 * slam_graph_set_edges(_odom).  pose_off[0] = 0, pose_off[n_members] = the
 * pose count, the offsets increase strictly, no member has more than 682 poses
 * (2046 unknowns: the dense path's limit), and the handle's solver is not
 * SLAM_GRAPH_PCG.  n_members = 0 returns the handle to the plain form.  The
 * call clears the edge set; slam_graph_set_poses clears the members and their
 * edge set.
 *
 * slam_graph_set_edges(_odom) on a handle with members additionally requires
 * both pose indices and both times of every edge in one member's range (times
 * index poses).  The columns of the union are all landmark pairs, then all
 * odometry edges, as ever; within each group a member's edges keep their
 * relative order, need not be contiguous, and the members need not come in
 * order.  slam_graph_get_system, get_bsr, get_delta, get_poses, chi2,
 * get_edge_weights, set_robust (one kind for the handle) and set_precond
 * (accepted, without effect) work on the union: H is block diagonal by member,
 * a member's block rows are the ranks of its times.  get_system's dense H is
 * limited to 2048 unknowns of the union; get_bsr has no limit.
 *
 * Every violation is SLAM_ERR_ARG, found on the host before any HIP call, and
 * leaves the handle as it was.  On a handle with members slam_graph_update,
 * slam_graph_optimize, slam_graph_marginals and slam_graph_apply_precond
 * return SLAM_ERR_ARG (the union with one anchor per member is not the system
 * they describe), and so do the two calls below on a handle without members.
 *
 * slam_graph_update_members: one updateEstPose of every member; stats is
 * [n_members][4], rows as slam_graph_update's.  A member with no edge or with
 * a single time gets a zero row; is_calc = 0 in a member is not an error.
 *
 * slam_graph_optimize_members: every member runs slam_graph_optimize's loop on
 * its own sum delta^2 (is_calc = 0 gives 0 and ends that member's loop).
 * Member m stops after its own n_iter[m] updates; from then on nothing it owns
 * is written (its poses, its columns of the blocks, its weights, its slots of
 * H, its rows of b and delta), so every query afterwards shows the system of
 * its last own update.  stats is [n_members][max_iter][4] or NULL, rows beyond
 * n_iter[m] zero; n_iter is [n_members].  The call ends when no member is
 * active. */
int slam_graph_set_members(slam_graph* h, int64_t n_members, const int64_t* pose_off /* [n_members + 1] */);
int slam_graph_update_members(slam_graph* h, double* stats /* [n_members][4] */);
int slam_graph_optimize_members(slam_graph* h, double delta_sum_th, int32_t max_iter,
                                double* stats /* [n_members][max_iter][4] or NULL */,
                                int32_t* n_iter /* [n_members] */);
/* The last assembled system: times (n_times), H (3n_times squared, dense, or
 * NULL), b (3 n_times or NULL), blocks (n_edges x 42: BB, BA, AB, AA, b_B, b_A
 * or NULL).  n_times may be queried with everything else NULL.  n_edges here is
 * all E columns of the set: the landmark edges, then the odometry edges. */
int slam_graph_get_system(slam_graph* h, int64_t* n_times, int64_t* times, double* H, double* b,
                          double* blocks);
/* The block-sparse H of the last update (block rows/columns are time ranks,
 * vals: n_slots x 9 row-major 3x3) and its solution delta (3 n_times);
 * n_slots may be queried with the arrays NULL. */
int slam_graph_get_bsr(slam_graph* h, int64_t* n_slots, int64_t* rows, int64_t* cols, double* vals);
int slam_graph_get_delta(slam_graph* h, double* delta);
/* Device time of the last update (ms): out[5] = {linearise, assemble, solve,
 * pose update, PCG iterations}. */
int slam_graph_timing(slam_graph* h, double* out);
/* The last PCG-path update's cond estimate: out[7] = {iterations, status (1
 * converged, 2 stopped early: cond >= cond_max for certain, 3 cond_max_iter
 * reached, 4 not positive definite), lambda_min, lambda_max, iterations of the
 * min side, of the max side, device time (ms)}.  Zeros after a dense update. */
int slam_graph_cond_info(slam_graph* h, double* out);
/* The last PCG-path update's gate (SLAM_GRAPH_COND_MARGIN): out[14] =
 * {decided by (1 the estimate with its margins and the log-det bounds, 2 a
 * half by the dense path), det decision (1 passed by the interval's lower end
 * at the 1000x margin / 0 rejected by its (rigorous) upper end, 3 / 2 by the
 * dense LU det, -1 undecided: not solved), cond decision (1 passed / 0
 * rejected by the estimate with its margin, 5 passed by a converged estimate
 * inside the margin band, 3 / 2 by the dense Lanczos cond, -1 undecided), log
 * det H lower end, upper end, cond (the value the decision used),
 * lambda_min(H), lambda_max(H) (the estimate's Ritz values), tr(P^2), n,
 * estimate iterations, host ms, det margin (the largest factor by which the
 * Ritz lambda_min may over-estimate lambda_min(H) with the lower end still
 * above ln det_min; 0 if none), cond margin (cond_max / cond)}.  Zeros after a
 * dense update, in the other modes, and when the estimate rejected H for
 * certain (cond_info status 2 / 4). */
int slam_graph_gate_info(slam_graph* h, double* out);
/* Joint marginal covariance of the poses at `times` (m distinct times of the
 * current edge set): cov[3m][3m] row-major, block (a, b) = rows of times[a],
 * columns of times[b] of H^-1.  relinearize = 1: H is linearised and assembled
 * at the current poses first (the covariance belongs to what slam_graph_get_poses
 * returns; slam_graph_get_system / get_bsr afterwards return this system);
 * relinearize = 0: the last assembled system, i.e. the matrix updateEstPose
 * inverted (:497).  info[6] = {is_calc, passes, max iterations of a column,
 * worst final relative residual, device ms, columns per pass}.
 *
 * Arguments, checked on the host before any launch (SLAM_ERR_ARG): NULL
 * pointers, m < 1, a time that is not among the edge set's times
 * (slam_graph_get_system's `times`), a time given twice, relinearize = 0 with
 * nothing assembled since the last slam_graph_set_edges, and a dense request
 * above 2048 unknowns.  With no edges, or 3 n_times <= 3, is_calc = 0 as in
 * slam_graph_update.  is_calc = 0 is not an error: the call returns SLAM_OK
 * with cov filled with NaN, as slam_graph_update returns SLAM_OK with
 * stats[0] = 0.
 *
 * Dense path (solver dense, or auto with n <= 2048): is_calc is the reference's
 * gate det_min < det && cond < cond_max (:496) on this H, from the LU and
 * Lanczos kernels of slam_graph_update; the 3m columns are substituted through
 * that LU, one workgroup each (passes = 1, iterations and residual 0, columns
 * per pass = 3m).
 * PCG path: passes of up to `columns per pass` independent block-Jacobi
 * preconditioned CGs on H x = e_j from x = 0; is_calc = 1 means every column
 * converged to cfg.pcg_tol (relative residual) within cfg.pcg_max_iter with
 * positive curvature; the call stops after the first pass that has a column
 * which did not (max iterations = the cap then).  The eigenvalue estimate and
 * the margin gate of slam_graph_update are NOT re-run: slam_graph_cond_info and
 * slam_graph_gate_info still describe the last update.  A column's bits do not
 * depend on what else is asked for, in which order, or on the columns per pass.
 *
 * The call does not move the poses and leaves slam_graph_get_delta,
 * slam_graph_timing, cond_info, gate_info and the warm starts of the next
 * update alone; its vectors are its own (allocated on first use, grow-only,
 * released by slam_graph_destroy).  cov is not symmetrised: H is symmetric only
 * to rounding (Omega = inv(...), :416), and so is its inverse. */
int slam_graph_marginals(slam_graph* h, int64_t m, const int64_t* times, int32_t relinearize,
                         double* cov, double* info);
/* columns per pass of the PCG path: 1, 2, 4 or 8 (0: the default, 4);
 * for A/B and tests */
int slam_graph_set_marginal_cols(slam_graph* h, int32_t cols);
/* Robust edge weights (no reference counterpart): iteratively
 * re-weighted least squares inside the linearisation.  For edge e, with err and
 * Omega as setPairObs forms them (:404-417), chi2_e = err^T Omega err; the
 * weight w_e multiplies all six blocks and both right-hand-side parts of the
 * edge, and is recomputed at every linearisation of the Gauss-Newton loop:
 *   SLAM_GRAPH_ROBUST_NONE    w = 1                                    rho = chi2
 *   SLAM_GRAPH_ROBUST_HUBER   w = 1 for chi2 <= k^2, else k/sqrt(chi2) rho = chi2, else 2k sqrt(chi2) - k^2
 *   SLAM_GRAPH_ROBUST_CAUCHY  w = 1 / (1 + chi2/k^2)                   rho = k^2 ln(1 + chi2/k^2)
 *   SLAM_GRAPH_ROBUST_DCS     w = s^2, s = min(1, 2P/(P + chi2))       rho = s^2 chi2 + P (1 - s)^2
 * (param = k, or P for dcs).  chi2 = 0 gives w = 1 exactly.  The default is
 * none: a handle on which slam_graph_set_robust is never called, or called
 * with none, runs the unweighted kernel and computes bit for bit what it
 * computed before the call existed.  Assembly, both solvers and the gate see
 * the weighted blocks; slam_graph_marginals with relinearize = 1 on a robust
 * handle therefore returns blocks of the inverse of the WEIGHTED H.  Above 2048
 * unknowns SLAM_GRAPH_COND_MARGIN may leave the det half of the gate undecided
 * on a weighted system (is_calc = 0, slam_graph_gate_info says so; measured at
 * 50,000 poses): use SLAM_GRAPH_COND_ESTIMATE or _OFF there.
 *
 * slam_graph_set_robust: SLAM_ERR_ARG, checked on the host before anything
 * else, for a NULL handle, an unknown kind, a non-finite param, and param <= 0
 * with a kind other than none.  May be called at any time; takes effect at the
 * next linearisation (slam_graph_update / optimize / marginals with
 * relinearize = 1). */
enum { SLAM_GRAPH_ROBUST_NONE = 0, SLAM_GRAPH_ROBUST_HUBER = 1, SLAM_GRAPH_ROBUST_CAUCHY = 2,
       SLAM_GRAPH_ROBUST_DCS = 3 };
int slam_graph_set_robust(slam_graph* h, int32_t kind, double param);
/* Chi-square of the edge set at the current poses under the handle's kind (one
 * lane per edge: err and Omega only, no Jacobians and no blocks).  totals[4] =
 * {sum chi2, sum rho, max chi2, number of edges with w < 0.1}; chi2 and weight
 * receive n_edges values each (or NULL).  The totals are folded in a fixed
 * order: bit-identical from call to call.  The call moves nothing and leaves
 * slam_graph_get_system, get_delta, timing, cond_info, gate_info and
 * slam_graph_get_edge_weights alone.  With no edges it returns SLAM_OK with the
 * totals zero.  SLAM_ERR_ARG for a NULL handle or NULL totals (checked before
 * the handle is read; the outputs are not written).  With odometry edges
 * (slam_graph_set_edges_odom) n_edges is all E columns, landmark edges first,
 * and the odometry columns carry w = 1, rho = chi2. */
int slam_graph_chi2(slam_graph* h, double* totals, double* chi2, double* weight);
/* chi2_e and w_e as the last linearisation stored them (n_edges each, or NULL):
 * the weights the last assembled H actually used, i.e. those at the poses
 * BEFORE the update that linearised.  SLAM_ERR_ARG when nothing has been
 * linearised since slam_graph_set_edges, and when that linearisation ran with
 * kind none: the unweighted kernel stores no rows (every weight was 1), and
 * the poses it ran at are gone after the update -- use slam_graph_chi2.  Over
 * all E columns, landmark edges first (odometry columns: w = 1). */
int slam_graph_get_edge_weights(slam_graph* h, double* chi2, double* weight);
/* Preconditioner of the PCG path (no reference counterpart).  The
 * default is block-Jacobi: the inverses of the diagonal 3x3 blocks.  The chain
 * preconditioner M follows consecutive rows, which is where odometry edges put
 * their off-diagonal blocks.  With the rows in the order of
 * slam_graph_get_system's `times` (nt of them), S the segment length in poses,
 * D_r the assembled diagonal block of row r and U_r the assembled block (r, r+1)
 * when that slot exists and floor(r / S) == floor((r + 1) / S), else 0 (a missing
 * slot, a segment end and the end of the system are the same case):
 *   M = block-tridiagonal(U_{r-1}^T, D_r, U_r)    (H's own (r+1, r) block is not read)
 *   factor, once per linearisation:
 *     S_r = D_r at a segment start, else D_r - U_{r-1}^T G_{r-1}
 *     Sinv_r = S_r^-1 (the 3x3 LU route of block-Jacobi),  G_r = Sinv_r U_r
 *   apply z = M^-1 r:
 *     forward   y_r = r_r - G_{r-1}^T y_{r-1}   (y_r = r_r at a segment start)
 *     backward  z_r = Sinv_r y_r - G_r z_{r+1}  (z_r = Sinv_r y_r at a segment end)
 * M is positive semi-definite by construction (an edge between adjacent rows of
 * one segment is kept whole, of every other edge its two diagonal parts), and it
 * is algebra on the assembled matrix: pairs only, odometry only, mixed and
 * robust-weighted systems alike.  S = 1 is block-Jacobi in other arithmetic.
 *
 * slam_graph_set_precond: segment must be 1, 2, 4, 8, 16, 32 or 64 (0 means 64;
 * a PCG workgroup owns 64 whole poses) and is ignored for block-Jacobi.
 * SLAM_ERR_ARG, checked on the host before the handle changes, for a NULL
 * handle, an unknown kind and any other segment.  Takes effect at the next
 * linearisation.  A handle on which it is never called, or called with
 * block-Jacobi, launches what it launched before the call existed and returns
 * the same bits.  On the dense path it is accepted and has no effect.  The
 * condition estimate, the gate and slam_graph_marginals keep block-Jacobi.
 * When the factor meets a bad pivot (a leading minor of S_r that is not
 * positive, or a value that is not finite) the solve ends as "not positive
 * definite" at iteration 0: is_calc = 0 and no error code, the outcome of the
 * PCG's curvature gate.
 *
 * slam_graph_precond_info: out[4] = {kind in force, segment in force (1 for
 * block-Jacobi), off-diagonal blocks the last factor used, bad pivots}; the
 * last two are 0 until a chain factor has run on the assembled system.
 *
 * slam_graph_apply_precond: z = M^-1 r for a host vector of 3 nt values by the
 * preconditioner in force on the last assembled system (factored here if no
 * solve has done it: the dense path, slam_graph_marginals with relinearize =
 * 1); with block-Jacobi z = minv r.  SLAM_ERR_ARG for a NULL argument and when
 * nothing has been assembled since slam_graph_set_edges.  It moves no pose and
 * leaves slam_graph_get_delta, timing, cond_info, gate_info and the warm starts
 * alone.  For the tests, and for a caller's own Krylov method on
 * slam_graph_get_bsr. */
#define SLAM_GRAPH_PRECOND_BLOCK_JACOBI 0
#define SLAM_GRAPH_PRECOND_CHAIN        1
int slam_graph_set_precond(slam_graph* h, int32_t kind, int32_t segment);
int slam_graph_precond_info(slam_graph* h, double* out /* [4] */);
int slam_graph_apply_precond(slam_graph* h, const double* r, double* z);
/* HalfEdge (graph_based_slam.py:259-300) with its Observation (:20-75). */
typedef struct {
    int64_t time, pose, landmark;
    double obs[3];        /* distance, direction, orientation */
} slam_graph_half;

/* Robot.estimateOpticalTrajectory's pairing (:697-703): for every landmark id
 * in 0..n_landmarks-1, each 2-combination of its half-edges in recording
 * order (itertools.combinations), ordered as setPairObs orders it (:371-384:
 * the later time is "aft", ties keep the combination order).  Half-edges of
 * other landmark ids never pair.  The half-edges are grouped per landmark on
 * the host (stable, O(n_halves)); the combinations are expanded on the device,
 * one lane per edge.  With edges == NULL only *n_edges is returned; otherwise
 * edges (host, *n_edges records) receives the edge list. */
int slam_graph_pair_halves(int64_t n_halves, const slam_graph_half* halves, int64_t n_landmarks,
                           int device, int64_t* n_edges, slam_graph_edge* edges);
/* The landmark map of the trajectory (no reference counterpart).
 * Conditional on the poses the landmarks are independent, and landmark l is the
 * information-weighted fusion of the half-edges that observe it.  With (x, y,
 * theta) the handle's current estimate of half-edge k's pose, (d, dir) its range
 * and bearing and the handle's r_dist, r_dir:
 *   ang    = dir + theta - pi/2                (the angle of the pair edges' covariance)
 *   L_k    = (x + d cos ang, y + d sin ang)
 *   W_k    = R(ang) diag(1 / (d r_dist)^2, 1 / (d sin r_dir)^2) R(ang)^T
 *   Lam_l  = sum_k W_k     eta_l = sum_k W_k (L_k - L_k0)     k0: l's first half-edge as recorded
 *   cov_l  = Lam_l^-1      mean_l = L_k0 + cov_l eta_l
 *   chi2_k = (L_k - mean_l)^T W_k (L_k - mean_l)      chi2_l = sum_k chi2_k
 * The measured orientation does not enter (it is the robot's compass reading,
 * not a property of the landmark): the map is conditional on the estimated
 * headings.  The covariance is that of the observations alone: the uncertainty
 * of the poses is NOT in it.  The robust kind does not enter either: every
 * observation counts fully, and half_chi2 is what shows a mis-identified one.
 * A landmark seen once has mean = L_k exactly, cov = W_k^-1 and chi2 = 0
 * exactly; a landmark nobody saw has count 0 and NaN mean, cov and chi2.
 *
 * The sums are folded in a fixed shape that depends on the landmark's own count
 * alone (chunks of 256 half-edges counted from its first, a fixed tree inside a
 * chunk, the chunks in order; no floating-point atomics): the results are
 * bit-identical from call to call, and a landmark's mean, cov and chi2 are
 * bit-identical whatever other landmarks and half-edges are in the set and
 * wherever its own stand among them, given the same relative order.
 *
 * slam_graph_set_observations uploads the half-edges and groups them per
 * landmark once (stable).  A half-edge whose landmark id lies outside [0,
 * n_landmarks) is ignored, as slam_graph_pair_halves ignores it; its half_chi2
 * comes back NaN.  n_halves = 0 clears the observations; slam_graph_set_poses
 * with a different pose count and slam_graph_set_members drop them.
 * SLAM_ERR_ARG, checked on the host before any HIP call (the handle is left as
 * it was): a NULL handle, a negative count, a NULL array with a positive
 * count, poses not set, a handle that has members (slam_graph_set_members), a
 * pose index out of range, a non-finite observation, and a distance <= 0.
 *
 * slam_graph_landmarks evaluates the map at the current poses: mean [NL][2],
 * cov [NL][4] row-major, count [NL], chi2 [NL], half_chi2 [n_halves] in input
 * order; any output may be NULL (with chi2 and half_chi2 both NULL the
 * chi-square pass is not launched).  SLAM_ERR_ARG for a NULL handle and
 * without observations.  It moves no pose and leaves slam_graph_get_system,
 * get_delta, timing, cond_info, gate_info, chi2, the edge weights and the
 * marginals alone; its arrays are its own (made by the first
 * slam_graph_set_observations, grow-only, released by slam_graph_destroy).  A
 * handle that is never given observations allocates nothing for the map,
 * launches what it launched before and computes the same bits.
 *
 * slam_graph_map_timing: out[2] = {device ms of the last evaluation's kernels,
 * their number}; slam_graph_map_kernel_timing: out[5] = the ms of each, in
 * launch order (contributions, fold, mean and cov, chi-square fold, chi-square
 * per landmark; 0 for one that was not launched). */
int slam_graph_set_observations(slam_graph* h, int64_t n_halves, const slam_graph_half* halves,
                                int64_t n_landmarks);
int slam_graph_landmarks(slam_graph* h, double* mean /* [NL][2] */, double* cov /* [NL][4] */,
                         int64_t* count /* [NL] */, double* chi2 /* [NL] */,
                         double* half_chi2 /* [n_halves], input order */);
int slam_graph_map_timing(slam_graph* h, double* out /* [2] */);
int slam_graph_map_kernel_timing(slam_graph* h, double* out /* [5] */);
/* One-shot form: poses in/out, stats[4] as slam_graph_update. */
int slam_graph_linearize_solve(const slam_graph_config* cfg, const slam_graph_edge* edges,
                               int64_t n_edges, double* poses, int64_t n_poses, double* stats,
                               int device);

/* ====================================================================
 * ScanSensor.scan (graph_based_slam.py:128-172) over poses x landmarks.
 * yaw_cs[p] = (cos(yaw), sin(yaw), yaw) with yaw = BASE_ANG - theta_p (NumPy's
 * values); tan_scan = tan(BASE_ANG - scan angle).  detect / obs are p-major
 * [n_poses][n_landmarks] (flag; dist, dir, orient).  slam_scan_noise adds the
 * reference's noise to n observations from 3n standard normals in its draw
 * order (dist, dir, orient per detected landmark).
 * ==================================================================== */
int slam_scan_detect(int64_t n_poses, const double* poses, const double* yaw_cs, int64_t n_landmarks,
                     const double* landmarks, double range, double tan_scan, int32_t* detect,
                     double* obs, int device);
int slam_scan_noise(int64_t n, const double* clean, const double* normals, double r_dist,
                    double r_dir, double r_orient, double* out, int device);

/* ErrorEllipse.calc_error_ellipse (mylib/error_ellipse.py:39-55) over n 2x2
 * covariances (row-major [n][4]): out[n][3] = (major, minor, angle); chi from
 * the chi-squared table on the host; column_vectors = 0 keeps the reference's
 * vec[idxmax] row quirk (:51). */
int slam_error_ellipse(int64_t n, const double* covs, double chi, int32_t column_vectors,
                       double* out, int device);

/* ====================================================================
 * NumPy's legacy RandomState stream on the device (MT19937 + polar
 * Box-Muller with the cached normal): the reference's noise source
 * (particle_filter.py:152, :165, :214; motion_model.py:46-48), drawn
 * bit-identically.  State = np.random.get_state()[1:5]: key[624], pos,
 * has_gauss, cached_gaussian.  log() is glibc's, restated with the table of
 * this process's libm (checked against its log() on first use).
 * ==================================================================== */
typedef struct slam_mt slam_mt;
int slam_mt_create(const uint32_t* key, int32_t pos, int32_t has_gauss, double gauss, int device,
                   slam_mt** out);
int slam_mt_destroy(slam_mt* h);
int slam_mt_set_state(slam_mt* h, const uint32_t* key, int32_t pos, int32_t has_gauss, double gauss);
int slam_mt_get_state(slam_mt* h, uint32_t* key, int32_t* pos, int32_t* has_gauss, double* gauss);
/* RandomState.random_sample(n) / standard_normal(n) into host arrays */
int slam_mt_random_sample(slam_mt* h, int64_t n, double* out);
int slam_mt_standard_normal(slam_mt* h, int64_t n, double* out);
/* jump-ahead (host): the 624-word window n_words further along the stream
 * than `window` (word 0's low 31 bits are not part of the MT19937 state and
 * come back unspecified) -- x^n mod the MT19937 characteristic polynomial */
int slam_mt_jump_window(const uint32_t* window, uint64_t n_words, uint32_t* out);
/* glibc's log restated (host; the function the device kernels evaluate) */
int slam_glibc_log(int64_t n, const double* x, double* out);

/* Particle filter with the reference's own noise stream on the device
 * (main_pf, particle_filter.py:86-119): each step draws [rand() if resampling]
 * -> mvn(0, Q, NP) -> mvn(0, R, NL) from the device stream, observes the
 * landmarks from the true pose on the device (__observation :144-154) and runs
 * the estimator.  r_factor = sqrt(s)[:, None] * v of svd(R) (row-major 2x2).
 * truth[4] per step = (x, y, cos(yaw'), sin(yaw')) of the true pose with
 * yaw' = pi/2 - theta (mylib/transform.py:31-35, NumPy's cos / sin). */
int slam_pf_set_rng_mt19937(slam_pf* h, const uint32_t* key, int32_t pos, int32_t has_gauss,
                            double gauss, const double* r_factor);
int slam_pf_get_rng_mt19937(slam_pf* h, uint32_t* key, int32_t* pos, int32_t* has_gauss,
                            double* gauss);
/* the device stream's word ring: out[4] = ring bytes, segments per refill
 * round, words per segment, requests one round feeds (at least) */
int slam_pf_rng_mt19937_info(slam_pf* h, int64_t* out);
int slam_pf_step_truth(slam_pf* h, const double* control, const double* truth, double* z_out,
                       slam_pf_result* res);
/* device-resident batch: truth[n_steps][4]; slam_pf_run then simulates the
 * observations of steps [first, first + k) on the device */
int slam_pf_load_truth(slam_pf* h, int32_t n_steps, const double* truth);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_HIP_H */
