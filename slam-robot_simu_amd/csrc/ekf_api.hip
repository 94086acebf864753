// ekf_api.hip -- C-ABI of the EKF localisation filter (batched) and of
// EKF-SLAM (include/slam_hip.h).
//
// ExtendedKalmanFilter (extended_kalman_filter.py:17-205) -> slam_ekf_*;
// EKF-SLAM (BASELINE config 4) -> slam_ekfslam_*.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_mem.hpp"
#include "ekf_kernels.inl"
#include "ekf_assoc.inl"
#include "eks_prune.hpp"

using namespace slam;

struct slam_ekf {
    slam_ekf_config cfg;
    int device = 0;
    int64_t batch = 0;
    hipStream_t stream = nullptr;
    DeviceMem mem;
    double* xs = nullptr;          // [3][B]
    double* Ps = nullptr;          // [9][B]
    double* z = nullptr;           // staging [steps][B][2]
    double* xh = nullptr;          // staging [steps][B][3]
    double* xm = nullptr;          // [B][3]
    int32_t cap_steps = 0;
};

struct slam_ekfslam {
    slam_ekfslam_config cfg;
    int device = 0;
    int64_t n_lm = 0, n = 0, ld = 0, n_pad = 0;
    int64_t pipe_grid = 0;         // persistent rank-update grid (resident workgroups, x8)
    int64_t frag_grid = 0;         // resident grid of the fragment-streaming rank update
    int32_t kernel_sel = 0;        // 0: fragment-streaming (m <= 64), 1: LDS-staged
    int32_t frag_shape = 0;        // 0: 8 waves of 32 x 64, 1: 16 waves of 32 x 32
    int32_t frag_pf = 0;           // experiment: where the next P block is requested
    int32_t apply_lds = 0;         // SLAM_EKS_APPLY=lds: the one-wave-per-row K = PH^T S^-1
    hipStream_t stream = nullptr;
    DeviceMem mem;
    double* P = nullptr;           // n x ld, lower triangle current
    double* mu = nullptr;          // n
    double* pht = nullptr;         // n_pad x M
    double* kg = nullptr;          // n_pad x M
    double* kf = nullptr;          // -K quad-major: [M/4][n_pad][4]
    double* hf = nullptr;          // PH^T quad-major
    double* hs = nullptr;          // kEksMaxM/3 x 18
    double* e = nullptr;           // M
    double* rd = nullptr;          // M
    double* sinv = nullptr;        // M x M
    int64_t* ids = nullptr;        // k
    double* diag = nullptr;        // n (init_diag staging)
    hipEvent_t ev[6] = {};
    double last_ms[5] = {0, 0, 0, 0, 0};
    int32_t last_m = 0;            // slam_ekfslam_info: the last update's operand width
    int32_t last_rank = SLAM_EKS_RANK_NONE;     // ... and the kernels it launched
    int32_t last_apply = SLAM_EKS_APPLY_NONE;
    // associating handle (slam_ekfslam_create_assoc): n_lm is the capacity
    bool assoc = false;
    slam_ekfslam_assoc_config acfg{};
    int32_t count = 0;             // landmarks held: slots 0..count-1
    double* scores = nullptr;      // [kEksMaxObs][n_lm]
    int32_t* taken = nullptr;      // n_lm
    int32_t* res = nullptr;        // {matched, new count, assoc[kEksMaxObs]}
    hipEvent_t aev[5] = {};
    double assoc_ms[4] = {0, 0, 0, 0};
    int32_t last_k = 0, last_count0 = 0;
    int32_t last_matched = 0, last_new = 0, last_dropped = 0;
    int64_t last_tiles = 0;        // tiles the last update walked
    // landmark evidence and removal (slam_ekfslam_set_pruning / _remove; DESIGN
    // 11h); buffers and events from the first use
    bool prune = false;
    slam_fs_prune_config prcfg{};
    int32_t* evd = nullptr;        // n_lm: evidence of the slots below count
    int32_t* psrc = nullptr;       // n_lm: the old slot of new slot w
    int32_t* pmask = nullptr;      // n_lm: slam_ekfslam_remove's flags
    int32_t* pres = nullptr;       // kEksPrWords
    hipEvent_t pev[3] = {};
    int32_t pr_before = 0, pr_removed = 0, pr_moved = 0, pr_first = -1;
    double pr_ms[2] = {0, 0};      // evidence kernel, compaction

    // rows of the state in use: all of it, or an associating handle's prefix
    int64_t n_act() const { return assoc ? 3 + 3 * (int64_t)count : n; }
};

namespace {

EKFConst ekf_const(const slam_ekf_config& c) {
    EKFConst k;
    k.dt = c.dt;
    k.vel = c.vel;
    k.omega = c.omega;
    for (int i = 0; i < 9; ++i) k.q[i] = c.q[i];
    for (int i = 0; i < 4; ++i) k.r[i] = c.r[i];
    k.motion = c.motion;
    for (int i = 0; i < 6; ++i) k.alphas[i] = c.alphas[i];
    return k;
}

int ekf_reserve(slam_ekf* h, int32_t steps) {
    if (steps <= h->cap_steps) return SLAM_OK;
    h->mem.release(h->z);
    h->mem.release(h->xh);
    h->cap_steps = 0;
    int rc;
    if ((rc = h->mem.alloc(&h->z, (size_t)steps * h->batch * 2)) ||
        (rc = h->mem.alloc(&h->xh, (size_t)steps * h->batch * 3)))
        return rc;
    h->cap_steps = steps;
    return SLAM_OK;
}

// host AoS [B][k] <-> device SoA [k][B]
int ekf_upload_soa(slam_ekf* h, double* dst, const double* src, int k) {
    std::vector<double> t((size_t)k * h->batch);
    for (int64_t b = 0; b < h->batch; ++b)
        for (int q = 0; q < k; ++q) t[(size_t)q * h->batch + b] = src[b * k + q];
    SLAM_HIP_TRY(hipMemcpyAsync(dst, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int ekf_download_soa(slam_ekf* h, double* dst, const double* src, int k) {
    std::vector<double> t((size_t)k * h->batch);
    SLAM_HIP_TRY(hipMemcpyAsync(t.data(), src, t.size() * sizeof(double), hipMemcpyDeviceToHost,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    for (int64_t b = 0; b < h->batch; ++b)
        for (int q = 0; q < k; ++q) dst[b * k + q] = t[(size_t)q * h->batch + b];
    return SLAM_OK;
}

int ekf_launch(slam_ekf* h, int32_t steps, const double* control, double* xm_last,
               double* xh_all) {
    const double v = control ? control[0] : h->cfg.vel;
    const double om = control ? control[1] : h->cfg.omega;
    const int64_t blocks = (h->batch + 255) / 256;
    hipLaunchKernelGGL(ekf_run_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->batch,
                       steps, ekf_const(h->cfg), v, om, h->xs, h->Ps, h->z, xh_all, xm_last);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// ---------------------------------------------------------------- EKF-SLAM
// acfg: NULL for a known-id handle
int eks_create(const slam_ekfslam_config* cfg, const slam_ekfslam_assoc_config* acfg,
               int64_t n_landmarks, int device, slam_ekfslam** out);

EksConst eks_const(const slam_ekfslam_config& c) {
    EksConst k;
    k.dt = c.dt;
    for (int i = 0; i < 9; ++i) k.q[i] = c.q_robot[i];
    k.r_dist = c.r_dist;
    k.r_dir = c.r_dir;
    k.r_orient = c.r_orient;
    k.motion = c.motion;
    for (int i = 0; i < 6; ++i) k.alphas[i] = c.alphas[i];
    return k;
}

int eks_predict(slam_ekfslam* h, const double* control) {
    const double v = control[0], om = control[1];
    const int64_t n = h->n_act(), rows = n - 3;
    if (rows > 0)
        hipLaunchKernelGGL(eks_predict_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256),
                           0, h->stream, h->P, n, h->ld, h->mu, eks_const(h->cfg), v, om);
    hipLaunchKernelGGL(eks_predict_pose_kernel, dim3(1), dim3(64), 0, h->stream, h->P, h->ld,
                       h->mu, eks_const(h->cfg), v, om);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int eks_update(slam_ekfslam* h, int32_t k, const int64_t* ids, const double* obs) {
    SLAM_ARG_CHECK(k >= 1 && 3 * k <= kEksMaxM, "slam_ekfslam_update: need 1 <= k <= 40");
    for (int32_t t = 0; t < k; ++t)
        SLAM_ARG_CHECK(ids[t] >= 0 && ids[t] < (h->assoc ? h->count : h->n_lm),
                       "slam_ekfslam_update: landmark id out of range");
    // the rows the kernels walk: the whole state, or an associating handle's
    // active prefix and its own 128-row round-up (the rest of P is zero)
    const int64_t n = h->n_act();
    const int64_t n_pad = h->assoc ? (n + kEksTile - 1) / kEksTile * kEksTile : h->n_pad;
    const int32_t m = 3 * k;
    const int32_t M = (m + 3) / 4 * 4;
    h->last_m = M;
    EksObs ob{};
    for (int32_t t = 0; t < k; ++t) ob.ids[t] = ids[t];
    for (int32_t u = 0; u < 3 * k; ++u) ob.obs[u] = obs[u];
    const EksConst c = eks_const(h->cfg);
    SLAM_HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(eks_build_kernel, dim3(1), dim3(128), 0, h->stream, h->mu, ob, h->ids, k,
                       M, c, h->hs, h->e, h->rd);
    hipLaunchKernelGGL(eks_pht_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0,
                       h->stream, h->P, n, h->ld, n_pad, h->ids, h->hs, k, M, h->pht);
    SLAM_HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    const size_t sbytes = (size_t)M * M * sizeof(double);
    hipLaunchKernelGGL(eks_gain_kernel, dim3(1), dim3(1024), sbytes, h->stream, h->pht, h->ids,
                       h->hs, h->rd, k, M, h->sinv);
    SLAM_HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    const int64_t apply_grid = std::min<int64_t>(512, (n_pad + 15) / 16);
    if (M <= 64 && !h->apply_lds) {
        hipLaunchKernelGGL(eks_apply_mfma_kernel, dim3((unsigned)((n_pad / 16 + 3) / 4)), dim3(256),
                           0, h->stream, h->pht, h->sinv, h->e, n, n_pad, M, h->kg, h->mu);
        h->last_apply = SLAM_EKS_APPLY_MFMA;
    } else {
        hipLaunchKernelGGL(eks_apply_kernel, dim3((unsigned)apply_grid), dim3(kEksApplyThreads),
                           sbytes, h->stream, h->pht, h->sinv, h->e, n, n_pad, M, h->kg, h->mu);
        h->last_apply = SLAM_EKS_APPLY_LDS;
    }
    SLAM_HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    const int64_t nt = n_pad / kEksTile;
    const int64_t tiles = nt * (nt + 1) / 2;
    h->last_tiles = tiles;
#ifndef SLAM_EKS_PIPE
#define SLAM_EKS_PIPE 1
#endif
    if (h->frag_grid > 0 && M <= kEksPipeK && h->kernel_sel == 0) {
        const int64_t tot = n_pad * M;
        hipLaunchKernelGGL(eks_frag_layout_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                           h->stream, h->kg, h->pht, n_pad, M, h->kf, h->hf);
#define SLAM_EKS_FRAG_S(QQ, WM, WN)                                                               \
    hipLaunchKernelGGL((eks_rank_update_frag_kernel<QQ, WM, WN>), dim3((unsigned)h->frag_grid),   \
                       dim3(EksFragShape<WM, WN>::kThreads), 0, h->stream, h->P, n, h->ld,         \
                       h->kf, h->hf, n_pad, tiles)
#define SLAM_EKS_FRAG(QQ)                                                                         \
    case QQ:                                                                                      \
        if (h->frag_shape == 1) {                                                                 \
            SLAM_EKS_FRAG_S(QQ, 2, 2);                                                            \
            h->last_rank = SLAM_EKS_RANK_FRAG_2X2;                                                \
        } else {                                                                                  \
            SLAM_EKS_FRAG_S(QQ, 2, 4);                                                            \
            h->last_rank = SLAM_EKS_RANK_FRAG_2X4;                                                \
        }                                                                                         \
        break
#define SLAM_EKS_FRAG_P(QQ, PF)                                                                   \
    hipLaunchKernelGGL((eks_rank_update_frag_kernel<QQ, 2, 4, PF>), dim3((unsigned)h->frag_grid), \
                       dim3(EksFragShape<2, 4>::kThreads), 0, h->stream, h->P, n, h->ld,           \
                       h->kf, h->hf, n_pad, tiles)
        if (M / 4 == 15 && h->frag_pf == 1) {
            SLAM_EKS_FRAG_P(15, 7);
            h->last_rank = SLAM_EKS_RANK_FRAG_2X4_PF;
        } else if (M / 4 == 15 && h->frag_pf == 2) {
            SLAM_EKS_FRAG_P(15, 0);
            h->last_rank = SLAM_EKS_RANK_FRAG_2X4_PF;
        } else switch (M / 4) {
            SLAM_EKS_FRAG(1); SLAM_EKS_FRAG(2); SLAM_EKS_FRAG(3); SLAM_EKS_FRAG(4);
            SLAM_EKS_FRAG(5); SLAM_EKS_FRAG(6); SLAM_EKS_FRAG(7); SLAM_EKS_FRAG(8);
            SLAM_EKS_FRAG(9); SLAM_EKS_FRAG(10); SLAM_EKS_FRAG(11); SLAM_EKS_FRAG(12);
            SLAM_EKS_FRAG(13); SLAM_EKS_FRAG(14); SLAM_EKS_FRAG(15); SLAM_EKS_FRAG(16);
            default: return fail(SLAM_ERR_ARG, "slam_ekfslam_update: bad operand width");
        }
#undef SLAM_EKS_FRAG_S
#undef SLAM_EKS_FRAG_P
#undef SLAM_EKS_FRAG
    } else if (SLAM_EKS_PIPE && h->pipe_grid > 0 && M <= kEksPipeK) {
        hipLaunchKernelGGL(eks_rank_update_pipelined_kernel, dim3((unsigned)h->pipe_grid),
                           dim3(kEksPipeThreads), 0, h->stream, h->P, n, h->ld, h->kg, h->pht, M,
                           tiles);
        h->last_rank = SLAM_EKS_RANK_PIPE;
    } else {
        const int64_t grid = (tiles + 7) / 8 * 8;
        hipLaunchKernelGGL(eks_rank_update_kernel, dim3((unsigned)grid), dim3(kEksThreads), 0,
                           h->stream, h->P, n, h->ld, h->kg, h->pht, M, tiles);
        h->last_rank = SLAM_EKS_RANK_LDS;
    }
    SLAM_HIP_TRY(hipEventRecord(h->ev[4], h->stream));
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int eks_collect_timing(slam_ekfslam* h) {
    SLAM_HIP_TRY(hipEventSynchronize(h->ev[4]));
    float ms;
    for (int q = 0; q < 4; ++q) {
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
        h->last_ms[q] = ms;
    }
    return SLAM_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ EKF
int slam_ekf_create(const slam_ekf_config* cfg, int64_t batch, int device, slam_ekf** out) {
    SLAM_ARG_CHECK(cfg && out && batch >= 1, "slam_ekf_create: bad arguments");
    SLAM_ARG_CHECK(cfg->motion == SLAM_MOTION_LINEAR || cfg->motion == SLAM_MOTION_VELOCITY,
                   "slam_ekf_create: bad motion model");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(SLAM_ERR_ARG, "slam_ekf_create: no such HIP device");
    SLAM_HIP_TRY(hipSetDevice(device));
    HandlePtr<slam_ekf, slam_ekf_destroy> hp(new slam_ekf());
    slam_ekf* h = hp.get();
    h->cfg = *cfg;
    h->device = device;
    h->batch = batch;
    DeviceMem& m = h->mem;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        m.alloc(&h->xs, 3 * (size_t)batch) || m.alloc(&h->Ps, 9 * (size_t)batch) ||
        m.alloc(&h->xm, 3 * (size_t)batch))
        return fail(SLAM_ERR_HIP, "slam_ekf_create: allocation failed");
    std::vector<double> x0((size_t)batch * 3), p0((size_t)batch * 9);
    for (int64_t b = 0; b < batch; ++b) {
        std::memcpy(&x0[b * 3], cfg->x0, 3 * sizeof(double));
        std::memcpy(&p0[b * 9], cfg->p0, 9 * sizeof(double));
    }
    int rc = slam_ekf_set_state(h, x0.data(), p0.data());
    if (rc != SLAM_OK) return rc;
    *out = hp.release();
    return SLAM_OK;
}

int slam_ekf_destroy(slam_ekf* h) {
    if (!h) return SLAM_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SLAM_OK;
}

int slam_ekf_set_state(slam_ekf* h, const double* x, const double* P) {
    SLAM_ARG_CHECK(h, "slam_ekf_set_state: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (x) {
        int rc = ekf_upload_soa(h, h->xs, x, 3);
        if (rc) return rc;
    }
    if (P) {
        int rc = ekf_upload_soa(h, h->Ps, P, 9);
        if (rc) return rc;
    }
    return SLAM_OK;
}

int slam_ekf_get_state(slam_ekf* h, double* x, double* P) {
    SLAM_ARG_CHECK(h, "slam_ekf_get_state: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (x) {
        int rc = ekf_download_soa(h, x, h->xs, 3);
        if (rc) return rc;
    }
    if (P) {
        int rc = ekf_download_soa(h, P, h->Ps, 9);
        if (rc) return rc;
    }
    return SLAM_OK;
}

int slam_ekf_step(slam_ekf* h, const double* control, const double* z, double* x_hat_m,
                  double* x_hat, double* P) {
    SLAM_ARG_CHECK(h && z, "slam_ekf_step: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = ekf_reserve(h, 1);
    if (rc) return rc;
    SLAM_HIP_TRY(hipMemcpyAsync(h->z, z, h->batch * 2 * sizeof(double), hipMemcpyHostToDevice,
                                h->stream));
    rc = ekf_launch(h, 1, control, h->xm, nullptr);
    if (rc) return rc;
    if (x_hat_m) {
        SLAM_HIP_TRY(hipMemcpyAsync(x_hat_m, h->xm, h->batch * 3 * sizeof(double),
                                    hipMemcpyDeviceToHost, h->stream));
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return slam_ekf_get_state(h, x_hat, P);
}

int slam_ekf_run(slam_ekf* h, int32_t n_steps, const double* control, const double* z_all,
                 double* x_hat_all) {
    SLAM_ARG_CHECK(h && z_all && n_steps >= 1, "slam_ekf_run: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = ekf_reserve(h, n_steps);
    if (rc) return rc;
    const size_t zb = (size_t)n_steps * h->batch * 2 * sizeof(double);
    SLAM_HIP_TRY(hipMemcpyAsync(h->z, z_all, zb, hipMemcpyHostToDevice, h->stream));
    rc = ekf_launch(h, n_steps, control, h->xm, x_hat_all ? h->xh : nullptr);
    if (rc) return rc;
    if (x_hat_all)
        SLAM_HIP_TRY(hipMemcpyAsync(x_hat_all, h->xh, (size_t)n_steps * h->batch * 3 * sizeof(double),
                                    hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

// Device-resident variant for the bench: observations already on the device
// (z_dev: n_steps x B x 2), estimates to x_hat_dev (or NULL).  Asynchronous.
int slam_ekf_run_device(slam_ekf* h, int32_t n_steps, const double* control, const double* z_dev,
                        double* x_hat_dev) {
    SLAM_ARG_CHECK(h && z_dev && n_steps >= 1, "slam_ekf_run_device: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const double v = control ? control[0] : h->cfg.vel;
    const double om = control ? control[1] : h->cfg.omega;
    const int64_t blocks = (h->batch + 255) / 256;
    hipLaunchKernelGGL(ekf_run_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->batch,
                       n_steps, ekf_const(h->cfg), v, om, h->xs, h->Ps, z_dev, x_hat_dev, h->xm);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int slam_ekf_load_observations(slam_ekf* h, int32_t n_steps, const double* z_all) {
    SLAM_ARG_CHECK(h && z_all && n_steps >= 1, "slam_ekf_load_observations: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = ekf_reserve(h, n_steps);
    if (rc) return rc;
    SLAM_HIP_TRY(hipMemcpyAsync(h->z, z_all, (size_t)n_steps * h->batch * 2 * sizeof(double),
                                hipMemcpyHostToDevice, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekf_run_loaded(slam_ekf* h, int32_t n_steps, const double* control, int32_t keep_history) {
    SLAM_ARG_CHECK(h && n_steps >= 1 && n_steps <= h->cap_steps,
                   "slam_ekf_run_loaded: load at least n_steps observations first");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    return ekf_launch(h, n_steps, control, h->xm, keep_history ? h->xh : nullptr);
}

int slam_ekf_synchronize(slam_ekf* h) {
    SLAM_ARG_CHECK(h, "slam_ekf_synchronize: NULL handle");
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

// ------------------------------------------------------------- EKF-SLAM
int slam_ekfslam_create(const slam_ekfslam_config* cfg, int64_t n_landmarks, int device,
                        slam_ekfslam** out) {
    SLAM_ARG_CHECK(cfg && out && n_landmarks >= 1, "slam_ekfslam_create: bad arguments");
    return eks_create(cfg, nullptr, n_landmarks, device, out);
}

int slam_ekfslam_create_assoc(const slam_ekfslam_config* cfg, const slam_ekfslam_assoc_config* acfg,
                              int64_t capacity, int device, slam_ekfslam** out) {
    SLAM_ARG_CHECK(cfg && acfg && out, "slam_ekfslam_create_assoc: NULL argument");
    *out = nullptr;
    SLAM_ARG_CHECK(capacity >= 1 && capacity <= (int64_t)1 << 24,
                   "slam_ekfslam_create_assoc: capacity must be in 1..2^24");
    SLAM_ARG_CHECK(std::isfinite(acfg->log_p_new),
                   "slam_ekfslam_create_assoc: log_p_new must be finite");
    return eks_create(cfg, acfg, capacity, device, out);
}

}  // extern "C"

namespace {

int eks_create(const slam_ekfslam_config* cfg, const slam_ekfslam_assoc_config* acfg,
               int64_t n_landmarks, int device, slam_ekfslam** out) {
    SLAM_ARG_CHECK(cfg->motion == SLAM_MOTION_LINEAR || cfg->motion == SLAM_MOTION_VELOCITY,
                   "slam_ekfslam_create: bad motion model");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(SLAM_ERR_ARG, "slam_ekfslam_create: no such HIP device");
    SLAM_HIP_TRY(hipSetDevice(device));
    HandlePtr<slam_ekfslam, slam_ekfslam_destroy> hp(new slam_ekfslam());
    slam_ekfslam* h = hp.get();
    h->cfg = *cfg;
    h->device = device;
    h->n_lm = n_landmarks;
    h->n = 3 + 3 * n_landmarks;
    // rows start on 128-byte lines: a tile row segment (16 lanes x 8 B) is one line
#ifndef SLAM_EKS_LD_ALIGN
#define SLAM_EKS_LD_ALIGN 16
#endif
#ifndef SLAM_EKS_LD_SKEW
#define SLAM_EKS_LD_SKEW 0
#endif
    h->ld = (h->n + SLAM_EKS_LD_ALIGN - 1) / SLAM_EKS_LD_ALIGN * SLAM_EKS_LD_ALIGN + SLAM_EKS_LD_SKEW;
    h->n_pad = (h->n + kEksTile - 1) / kEksTile * kEksTile;
    {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, eks_rank_update_pipelined_kernel,
                                                         kEksPipeThreads, 0) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) ==
                hipSuccess)
            h->pipe_grid = (int64_t)per_cu * cus / 8 * 8;
        // SLAM_EKS_KERNEL=pipe selects the LDS-staged kernel, =frag16 the
        // 16-wave fragment shape (comparison runs); default: 8 waves of 32 x 64
        const char* ks = std::getenv("SLAM_EKS_KERNEL");
        const std::string sel = ks ? ks : "";
        h->kernel_sel = sel == "pipe" ? 1 : 0;
        h->frag_shape = (sel == "frag16") ? 1 : 0;
        h->frag_pf = sel == "pfmid" ? 1 : sel == "pf0" ? 2 : 0;
        const char* ap = std::getenv("SLAM_EKS_APPLY");
        h->apply_lds = (ap && std::string(ap) == "lds") ? 1 : 0;
        const hipError_t oe =
            h->frag_shape == 1
                ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, eks_rank_update_frag_kernel<15, 2, 2>, EksFragShape<2, 2>::kThreads, 0)
                : hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, eks_rank_update_frag_kernel<15, 2, 4>, EksFragShape<2, 4>::kThreads, 0);
        if (oe == hipSuccess && cus > 0) h->frag_grid = (int64_t)std::max(per_cu, 1) * cus / 8 * 8;
    }
    const size_t pbytes = (size_t)h->n * h->ld * sizeof(double);
    const size_t rows = (size_t)h->n_pad * kEksMaxM;
    DeviceMem& m = h->mem;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        m.alloc(&h->P, (size_t)h->n * h->ld) || m.alloc(&h->mu, (size_t)h->n) ||
        m.alloc(&h->pht, rows) || m.alloc(&h->kg, rows) ||
        m.alloc(&h->kf, (size_t)h->n_pad * kEksPipeK) || m.alloc(&h->hf, (size_t)h->n_pad * kEksPipeK) ||
        m.alloc(&h->hs, (kEksMaxM / 3) * 18) || m.alloc(&h->e, kEksMaxM) || m.alloc(&h->rd, kEksMaxM) ||
        m.alloc(&h->sinv, kEksMaxM * kEksMaxM) || m.alloc(&h->ids, kEksMaxM / 3) ||
        m.alloc(&h->diag, (size_t)h->n))
        return fail(SLAM_ERR_HIP, "slam_ekfslam_create: allocation failed (P is n^2 fp64)");
    for (auto& e : h->ev)
        if (m.event(&e)) return fail(SLAM_ERR_HIP, "slam_ekfslam_create: event creation failed");
    if (hipMemsetAsync(h->P, 0, pbytes, h->stream) != hipSuccess ||
        hipMemsetAsync(h->mu, 0, h->n * sizeof(double), h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(SLAM_ERR_HIP, "slam_ekfslam_create: initialisation failed");
    const size_t big = (size_t)kEksMaxM * kEksMaxM * sizeof(double);
    if (hipFuncSetAttribute((const void*)eks_gain_kernel,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)big) != hipSuccess ||
        hipFuncSetAttribute((const void*)eks_apply_kernel,
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)big) != hipSuccess)
        return fail(SLAM_ERR_HIP, "slam_ekfslam_create: LDS attribute failed");
    if (acfg) {
        h->assoc = true;
        h->acfg = *acfg;
        if (m.alloc(&h->scores, (size_t)kEksMaxObs * n_landmarks) ||
            m.alloc(&h->taken, (size_t)n_landmarks) || m.alloc(&h->res, 2 + kEksMaxObs))
            return fail(SLAM_ERR_HIP, "slam_ekfslam_create_assoc: allocation failed");
        for (auto& e : h->aev)
            if (m.event(&e))
                return fail(SLAM_ERR_HIP, "slam_ekfslam_create_assoc: event creation failed");
    }
    *out = hp.release();
    return SLAM_OK;
}

// k observations without ids: finite, range > 0 (host only)
int eks_check_observations(const char* who, int32_t k, const double* obs) {
    SLAM_ARG_CHECK(k >= 0 && k <= kEksMaxObs, std::string(who) + ": need 0 <= k <= 40");
    SLAM_ARG_CHECK(k == 0 || obs, std::string(who) + ": NULL observations");
    for (int32_t u = 0; u < 3 * k; ++u)
        SLAM_ARG_CHECK(std::isfinite(obs[u]), std::string(who) + ": observations must be finite");
    for (int32_t t = 0; t < k; ++t)
        SLAM_ARG_CHECK(obs[3 * t] > 0.0, std::string(who) + ": ranges must be positive");
    return SLAM_OK;
}

// The buffers and events of the evidence pass and of slam_ekfslam_remove.
int eks_prune_reserve(slam_ekfslam* h) {
    if (h->psrc) return SLAM_OK;
    DeviceMem& m = h->mem;
    int rc;
    if ((rc = m.alloc(&h->evd, (size_t)h->n_lm)) || (rc = m.alloc(&h->pmask, (size_t)h->n_lm)) ||
        (rc = m.alloc(&h->pres, (size_t)kEksPrWords)) || (rc = m.event(&h->pev[0])) ||
        (rc = m.event(&h->pev[1])) || (rc = m.event(&h->pev[2])) ||
        (rc = m.alloc(&h->psrc, (size_t)h->n_lm)))
        return rc;
    return SLAM_OK;
}

// every slot at init: the slots at or beyond count are never read (a slot that
// a call creates takes init)
int eks_evidence_init(slam_ekfslam* h) {
    SLAM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->evd, h->prcfg.init, (size_t)h->n_lm, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

// After the evidence or mask kernel (between pev[0] and pev[1]): the result
// words to the host, the compaction where something was removed, the new count.
int eks_prune_finish(slam_ekfslam* h, int32_t count) {
    int32_t res[kEksPrWords];
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipMemcpyAsync(res, h->pres, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    const int32_t cn = res[kEksPrCount], first = res[kEksPrFirst];
    if (cn < 0 || cn > count || res[kEksPrRemoved] != count - cn ||
        (cn < count) != (first >= 0 && first <= cn))
        return fail(SLAM_ERR_STATE, "slam_ekfslam: inconsistent removal");
    h->pr_before = count;
    h->pr_removed = count - cn;
    h->pr_moved = res[kEksPrMoved];
    h->pr_first = first;
    h->pr_ms[1] = 0.0;
    float ms;
    if (cn < count) {
        eks_compact_launch(h->stream, h->P, h->ld, h->mu, h->psrc, first, cn, count);
        SLAM_HIP_TRY(hipEventRecord(h->pev[2], h->stream));
        SLAM_HIP_TRY(hipGetLastError());
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->pev[1], h->pev[2]));
        h->pr_ms[1] = ms;
        h->count = cn;
    }
    SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->pev[0], h->pev[1]));
    h->pr_ms[0] = ms;
    return SLAM_OK;
}

// The evidence pass at the end of an observe (include/slam_hip.h); matched:
// the assign kernel ran in this call and left its marks in taken.
int eks_prune_pass(slam_ekfslam* h, int32_t count0, bool matched) {
    const slam_fs_prune_config& pc = h->prcfg;
    const EksPrune P{pc.view_range * pc.view_range, pc.view_tan, pc.init, pc.hit, pc.miss,
                     pc.ev_max, pc.remove_below};
    SLAM_HIP_TRY(hipEventRecord(h->pev[0], h->stream));
    eks_evidence_launch(h->stream, pc.use_angle != 0, h->mu, count0, h->count,
                        matched ? h->taken : nullptr, P, h->evd, h->psrc, h->pres);
    SLAM_HIP_TRY(hipEventRecord(h->pev[1], h->stream));
    return eks_prune_finish(h, h->count);
}

// Score, choose, update over the active prefix, initialise (include/slam_hip.h).
int eks_observe(slam_ekfslam* h, int32_t k, const double* obs, int32_t* assoc_out) {
    const EksConst c = eks_const(h->cfg);
    const int32_t count0 = h->count;
    const int64_t cap = h->n_lm;
    h->last_k = k;
    h->last_count0 = count0;
    h->last_matched = h->last_new = h->last_dropped = 0;
    h->last_tiles = 0;
    for (double& v : h->assoc_ms) v = 0.0;
    if (k == 0) return h->prune ? eks_prune_pass(h, count0, false) : SLAM_OK;   // an empty scan is evidence too
    SLAM_HIP_TRY(hipEventRecord(h->aev[0], h->stream));
    if (count0 > 0) {
        EksScan sc{};
        for (int32_t u = 0; u < 3 * k; ++u) sc.obs[u] = obs[u];
        hipLaunchKernelGGL(eks_scan_kernel,
                           dim3((unsigned)((count0 + kEksScanThreads - 1) / kEksScanThreads)),
                           dim3(kEksScanThreads), 0, h->stream, h->P, h->ld, h->mu, count0, k, sc, c,
                           cap, h->scores);
    }
    SLAM_HIP_TRY(hipEventRecord(h->aev[1], h->stream));
    hipLaunchKernelGGL(eks_assign_kernel, dim3(1), dim3(kEksAssignThreads), 0, h->stream, h->scores,
                       cap, count0, (int32_t)cap, k, h->acfg.log_p_new, h->taken, h->res);
    SLAM_HIP_TRY(hipEventRecord(h->aev[2], h->stream));
    SLAM_HIP_TRY(hipGetLastError());
    int32_t res[2 + kEksMaxObs];
    SLAM_HIP_TRY(hipMemcpyAsync(res, h->res, (2 + k) * sizeof(int32_t), hipMemcpyDeviceToHost,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    // the matched and the new observations, each in observation order: the
    // update and the initialisation take them in their kernel arguments
    int64_t ids[kEksMaxObs];
    double mobs[3 * kEksMaxObs];
    EksNew nw{};
    int32_t nm = 0;
    for (int32_t t = 0; t < k; ++t) {
        const int32_t a = res[2 + t];
        if (assoc_out) assoc_out[t] = a;
        if (a >= 0) {
            ids[nm] = a;
            for (int q = 0; q < 3; ++q) mobs[3 * nm + q] = obs[3 * t + q];
            ++nm;
        } else if (a == -1) {
            for (int q = 0; q < 3; ++q) nw.obs[3 * nw.n_new + q] = obs[3 * t + q];
            ++nw.n_new;
        } else {
            ++h->last_dropped;
        }
    }
    if (nm != res[0] || count0 + nw.n_new != res[1] || res[1] > cap)
        return fail(SLAM_ERR_STATE, "slam_ekfslam_observe: inconsistent assignment");
    h->last_matched = nm;
    h->last_new = nw.n_new;
    if (nm > 0) {
        int rc = eks_update(h, nm, ids, mobs);
        if (rc) return rc;
    }
    if (nw.n_new > 0) {
        SLAM_HIP_TRY(hipEventRecord(h->aev[3], h->stream));
        const int64_t cols = 3 + 3 * (int64_t)(count0 + nw.n_new);
        hipLaunchKernelGGL(eks_init_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)nw.n_new),
                           dim3(256), 0, h->stream, h->P, h->ld, h->mu, count0, nw, c);
        SLAM_HIP_TRY(hipEventRecord(h->aev[4], h->stream));
        SLAM_HIP_TRY(hipGetLastError());
        h->count = count0 + nw.n_new;
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    float ms;
    SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->aev[0], h->aev[1]));
    h->assoc_ms[0] = ms;
    SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->aev[1], h->aev[2]));
    h->assoc_ms[1] = ms;
    if (nm > 0) {
        int rc = eks_collect_timing(h);
        if (rc) return rc;
        h->assoc_ms[2] = h->last_ms[0] + h->last_ms[1] + h->last_ms[2] + h->last_ms[3];
    }
    if (nw.n_new > 0) {
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->aev[3], h->aev[4]));
        h->assoc_ms[3] = ms;
    }
    return h->prune ? eks_prune_pass(h, count0, true) : SLAM_OK;
}

}  // namespace

extern "C" {

int slam_ekfslam_check_observations(int32_t k, const double* obs) {
    return eks_check_observations("slam_ekfslam_check_observations", k, obs);
}

int slam_ekfslam_observe(slam_ekfslam* h, int32_t k, const double* obs, int32_t* assoc_out) {
    SLAM_ARG_CHECK(h, "slam_ekfslam_observe: NULL handle");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_observe: not an associating handle");
    int rc = eks_check_observations("slam_ekfslam_observe", k, obs);
    if (rc) return rc;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    return eks_observe(h, k, obs, assoc_out);
}

int slam_ekfslam_step_assoc(slam_ekfslam* h, const double* control, int32_t k, const double* obs,
                            int32_t* assoc_out) {
    SLAM_ARG_CHECK(h && control, "slam_ekfslam_step_assoc: NULL argument");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_step_assoc: not an associating handle");
    int rc = eks_check_observations("slam_ekfslam_step_assoc", k, obs);
    if (rc) return rc;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    rc = eks_predict(h, control);
    if (rc) return rc;
    rc = eks_observe(h, k, obs, assoc_out);
    if (rc) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_get_count(slam_ekfslam* h, int32_t* count) {
    SLAM_ARG_CHECK(h && count, "slam_ekfslam_get_count: NULL argument");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_get_count: not an associating handle");
    *count = h->count;
    return SLAM_OK;
}

int slam_ekfslam_set_count(slam_ekfslam* h, int32_t count) {
    SLAM_ARG_CHECK(h, "slam_ekfslam_set_count: NULL handle");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_set_count: not an associating handle");
    SLAM_ARG_CHECK(count >= 0 && count <= h->n_lm, "slam_ekfslam_set_count: need 0 <= count <= capacity");
    h->count = count;
    if (h->prune) {
        SLAM_HIP_TRY(hipSetDevice(h->device));
        return eks_evidence_init(h);
    }
    return SLAM_OK;
}

int slam_ekfslam_set_pruning(slam_ekfslam* h, const slam_fs_prune_config* c) {
    SLAM_ARG_CHECK(h, "slam_ekfslam_set_pruning: NULL handle");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_set_pruning: not an associating handle");
    if (!c) {
        h->prune = false;
        return SLAM_OK;
    }
    int rc = slam_fs_check_prune_config(c);
    if (rc) return rc;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if ((rc = eks_prune_reserve(h))) return rc;
    const bool was = h->prune;
    h->prcfg = *c;
    h->prcfg.use_angle = c->use_angle ? 1 : 0;
    h->prune = true;
    return was ? SLAM_OK : eks_evidence_init(h);     // turned on: every live slot starts at init
}

int slam_ekfslam_set_evidence(slam_ekfslam* h, const int32_t* ev) {
    SLAM_ARG_CHECK(h && ev, "slam_ekfslam_set_evidence: NULL argument");
    SLAM_ARG_CHECK(h->prune, "slam_ekfslam_set_evidence: pruning is off");
    if (h->count == 0) return SLAM_OK;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    SLAM_HIP_TRY(hipMemcpyAsync(h->evd, ev, sizeof(int32_t) * (size_t)h->count, hipMemcpyHostToDevice,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_get_evidence(slam_ekfslam* h, int32_t* ev) {
    SLAM_ARG_CHECK(h && ev, "slam_ekfslam_get_evidence: NULL argument");
    SLAM_ARG_CHECK(h->prune, "slam_ekfslam_get_evidence: pruning is off");
    std::fill(ev + h->count, ev + h->n_lm, 0);
    if (h->count == 0) return SLAM_OK;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    SLAM_HIP_TRY(hipMemcpyAsync(ev, h->evd, sizeof(int32_t) * (size_t)h->count, hipMemcpyDeviceToHost,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_remove(slam_ekfslam* h, int32_t n, const int32_t* slots) {
    SLAM_ARG_CHECK(h, "slam_ekfslam_remove: NULL handle");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_remove: not an associating handle");
    SLAM_ARG_CHECK(n >= 0 && (n == 0 || slots), "slam_ekfslam_remove: bad arguments");
    for (int32_t q = 0; q < n; ++q)
        SLAM_ARG_CHECK(slots[q] >= 0 && slots[q] < h->count && (q == 0 || slots[q] > slots[q - 1]),
                       "slam_ekfslam_remove: slots must be strictly increasing and below count");
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = eks_prune_reserve(h);
    if (rc) return rc;
    std::vector<int32_t> mask((size_t)h->count, 0);
    for (int32_t q = 0; q < n; ++q) mask[(size_t)slots[q]] = 1;
    SLAM_HIP_TRY(hipMemcpyAsync(h->pmask, mask.data(), sizeof(int32_t) * mask.size(),
                                hipMemcpyHostToDevice, h->stream));
    SLAM_HIP_TRY(hipEventRecord(h->pev[0], h->stream));
    eks_mask_launch(h->stream, h->pmask, h->count, h->prune ? h->evd : nullptr, h->psrc, h->pres);
    SLAM_HIP_TRY(hipEventRecord(h->pev[1], h->stream));
    return eks_prune_finish(h, h->count);
}

static_assert(sizeof(slam_ekfslam_prune_info_t) == 32,
              "slamhip/_lib.py EKFSLAMPruneInfo mirrors this layout");

int slam_ekfslam_prune_info(slam_ekfslam* h, slam_ekfslam_prune_info_t* out) {
    SLAM_ARG_CHECK(h && out, "slam_ekfslam_prune_info: NULL argument");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_prune_info: not an associating handle");
    *out = slam_ekfslam_prune_info_t{h->pr_before, h->pr_removed, h->pr_moved, h->pr_first,
                                     h->pr_ms[0], h->pr_ms[1]};
    return SLAM_OK;
}

int slam_ekfslam_get_scores(slam_ekfslam* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_ekfslam_get_scores: NULL argument");
    SLAM_ARG_CHECK(h->assoc && h->acfg.record,
                   "slam_ekfslam_get_scores: the handle was not created with record set");
    if (h->last_k == 0 || h->last_count0 == 0) return SLAM_OK;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const size_t w = (size_t)h->last_count0 * sizeof(double);
    SLAM_HIP_TRY(hipMemcpy2DAsync(out, w, h->scores, (size_t)h->n_lm * sizeof(double), w, h->last_k,
                                  hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

static_assert(sizeof(slam_ekfslam_assoc_info_t) == 40,
              "slamhip/_lib.py EKFSLAMAssocInfo mirrors this layout");

int slam_ekfslam_assoc_info(slam_ekfslam* h, slam_ekfslam_assoc_info_t* out) {
    SLAM_ARG_CHECK(h && out, "slam_ekfslam_assoc_info: NULL argument");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_assoc_info: not an associating handle");
    *out = slam_ekfslam_assoc_info_t{};
    out->n_act = h->n_act();
    out->tiles = h->last_tiles;
    out->count = h->count;
    out->count0 = h->last_count0;
    out->matched = h->last_matched;
    out->created = h->last_new;
    out->dropped = h->last_dropped;
    return SLAM_OK;
}

int slam_ekfslam_assoc_timing(slam_ekfslam* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_ekfslam_assoc_timing: NULL argument");
    SLAM_ARG_CHECK(h->assoc, "slam_ekfslam_assoc_timing: not an associating handle");
    for (int q = 0; q < 4; ++q) out[q] = h->assoc_ms[q];
    return SLAM_OK;
}

int slam_ekfslam_destroy(slam_ekfslam* h) {
    if (!h) return SLAM_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SLAM_OK;
}

int slam_ekfslam_set_state(slam_ekfslam* h, const double* mu, const double* P) {
    SLAM_ARG_CHECK(h, "slam_ekfslam_set_state: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (mu)
        SLAM_HIP_TRY(hipMemcpyAsync(h->mu, mu, h->n * sizeof(double), hipMemcpyHostToDevice,
                                    h->stream));
    if (P)
        SLAM_HIP_TRY(hipMemcpy2DAsync(h->P, h->ld * sizeof(double), P, h->n * sizeof(double),
                                      h->n * sizeof(double), h->n, hipMemcpyHostToDevice,
                                      h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_init_diag(slam_ekfslam* h, const double* mu, const double* p_diag) {
    SLAM_ARG_CHECK(h && p_diag, "slam_ekfslam_init_diag: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (mu)
        SLAM_HIP_TRY(hipMemcpyAsync(h->mu, mu, h->n * sizeof(double), hipMemcpyHostToDevice,
                                    h->stream));
    SLAM_HIP_TRY(hipMemsetAsync(h->P, 0, (size_t)h->n * h->ld * sizeof(double), h->stream));
    SLAM_HIP_TRY(hipMemcpyAsync(h->diag, p_diag, h->n * sizeof(double), hipMemcpyHostToDevice,
                                h->stream));
    hipLaunchKernelGGL(eks_diag_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0,
                       h->stream, h->P, h->n, h->ld, h->diag);
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_get_state(slam_ekfslam* h, double* mu, double* P) {
    SLAM_ARG_CHECK(h, "slam_ekfslam_get_state: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (mu)
        SLAM_HIP_TRY(hipMemcpyAsync(mu, h->mu, h->n * sizeof(double), hipMemcpyDeviceToHost,
                                    h->stream));
    if (P) {
        // symmetrise row blocks through the K scratch (n_pad x kEksMaxM doubles)
        const int64_t chunk = std::max<int64_t>(1, (h->n_pad * kEksMaxM) / h->n);
        for (int64_t i0 = 0; i0 < h->n; i0 += chunk) {
            const int64_t rows = std::min<int64_t>(chunk, h->n - i0);
            hipLaunchKernelGGL(eks_symmetrize_kernel, dim3((unsigned)((h->n + 255) / 256),
                               (unsigned)rows), dim3(256), 0, h->stream, h->P, h->n, h->ld, i0,
                               h->kg);
            SLAM_HIP_TRY(hipGetLastError());
            SLAM_HIP_TRY(hipMemcpyAsync(P + i0 * h->n, h->kg, rows * h->n * sizeof(double),
                                        hipMemcpyDeviceToHost, h->stream));
            SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_get_rows(slam_ekfslam* h, int64_t k, const int64_t* rows, double* out) {
    SLAM_ARG_CHECK(h && (k == 0 || (rows && out)) && k >= 0, "slam_ekfslam_get_rows: bad argument");
    for (int64_t r = 0; r < k; ++r)
        SLAM_ARG_CHECK(rows[r] >= 0 && rows[r] < h->n, "slam_ekfslam_get_rows: row out of range");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    // batches of rows through the K scratch (n_pad x kEksMaxM doubles) and the
    // id scratch (kEksMaxM / 3 int64)
    const int64_t chunk = std::min<int64_t>(kEksMaxM / 3,
                                            std::max<int64_t>(1, (h->n_pad * kEksMaxM) / h->n));
    for (int64_t r0 = 0; r0 < k; r0 += chunk) {
        const int64_t cnt = std::min<int64_t>(chunk, k - r0);
        SLAM_HIP_TRY(hipMemcpyAsync(h->ids, rows + r0, cnt * sizeof(int64_t), hipMemcpyHostToDevice,
                                    h->stream));
        hipLaunchKernelGGL(eks_gather_rows_kernel, dim3((unsigned)((h->n + 255) / 256), (unsigned)cnt),
                           dim3(256), 0, h->stream, h->P, h->n, h->ld, h->ids, h->kg);
        SLAM_HIP_TRY(hipGetLastError());
        SLAM_HIP_TRY(hipMemcpyAsync(out + r0 * h->n, h->kg, cnt * h->n * sizeof(double),
                                    hipMemcpyDeviceToHost, h->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return SLAM_OK;
}

int slam_ekfslam_predict(slam_ekfslam* h, const double* control) {
    SLAM_ARG_CHECK(h && control, "slam_ekfslam_predict: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = eks_predict(h, control);
    if (rc) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_update(slam_ekfslam* h, int32_t k, const int64_t* ids, const double* obs) {
    SLAM_ARG_CHECK(h && ids && obs, "slam_ekfslam_update: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = eks_update(h, k, ids, obs);
    if (rc) return rc;
    rc = eks_collect_timing(h);
    if (rc) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_step(slam_ekfslam* h, const double* control, int32_t k, const int64_t* ids,
                      const double* obs) {
    SLAM_ARG_CHECK(h && control && ids && obs, "slam_ekfslam_step: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = eks_predict(h, control);
    if (rc) return rc;
    rc = eks_update(h, k, ids, obs);
    if (rc) return rc;
    rc = eks_collect_timing(h);
    if (rc) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_ekfslam_timing(slam_ekfslam* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_ekfslam_timing: NULL argument");
    for (int q = 0; q < 5; ++q) out[q] = h->last_ms[q];
    return SLAM_OK;
}

static_assert(sizeof(slam_ekfslam_info_t) == 64, "slamhip/_lib.py EKFSLAMInfo mirrors this layout");

int slam_ekfslam_info(slam_ekfslam* h, slam_ekfslam_info_t* out) {
    SLAM_ARG_CHECK(h && out, "slam_ekfslam_info: NULL argument");
    const int64_t nt = h->n_pad / kEksTile;
    *out = slam_ekfslam_info_t{};
    out->n = h->n;
    out->ld = h->ld;
    out->n_pad = h->n_pad;
    out->n_tiles = nt * (nt + 1) / 2;
    out->frag_grid = h->frag_grid;
    out->pipe_grid = h->pipe_grid;
    out->last_m = h->last_m;
    out->last_rank = h->last_rank;
    out->last_apply = h->last_apply;
    return SLAM_OK;
}

}  // extern "C"
