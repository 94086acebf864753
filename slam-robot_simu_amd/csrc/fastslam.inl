// fastslam.inl -- gfx950 kernels of FastSLAM 1.0 with known data association
// (included by fs_api.inl): the per-particle landmark EKFs with their log
// weights, the weight pass, and the resampling gather of whole maps; below
// them the kernels of per-particle maximum-likelihood association, the one
// kernel of FastSLAM 2.0's observation-informed proposal, and last that
// proposal with the association inside it.
//
// Every formula is one device function at the top of the file (all of them
// inlined: the library is built with -ffp-contract=off, so a kernel's roundings
// are those of the expressions here, in their order); the kernels below differ
// in what they loop over and in what they keep.  Map layout: fs_common.hpp.
#include "fs_common.hpp"

namespace slam {

constexpr int kFsObsLds = 128;      // observations staged per pass (9.3 KB of LDS)
constexpr double kFsLn2Pi = 1.8378770664093453;     // np.log(2 * np.pi)

// One observation with its particle-independent terms (formed on the host
// once per step, or once per loaded run)
struct FsObs {
    double d, phi, psi;     // range, bearing, orientation
    double r0, r1;          // (d r_dist)^2, (d sin r_dir)^2
    double rx, ry;          // d cos phi, d sin phi
    double vo;              // r_dir^2 + r_orient^2
    int64_t id;
};

// Where an observation is taken from: the position, and s, c = sincos(pi/2 - theta)
struct FsFrame {
    double x, y, s, c;
};

__device__ __forceinline__ FsFrame fs_frame(const double x, const double y, const double th) {
    FsFrame F{x, y, 0.0, 0.0};
    sincos(kHalfPi - th, &F.s, &F.c);
    return F;
}

// One range and bearing with their noise variances, and the same point in
// the robot's frame
struct FsZ {
    double d, phi, r0, r1, rx, ry;
};

// ---- staging: a block's next kFsObsLds observations in LDS, without ids (a
// scan) or with them and with seen[id]
struct FsScanLds {
    static constexpr bool kIds = false;
    double d[kFsObsLds], phi[kFsObsLds], psi[kFsObsLds], r0[kFsObsLds], r1[kFsObsLds],
        rx[kFsObsLds], ry[kFsObsLds], vo[kFsObsLds];
    __device__ __forceinline__ FsZ z(const int32_t t) const {
        return FsZ{d[t], phi[t], r0[t], r1[t], rx[t], ry[t]};
    }
};
struct FsObsLds : FsScanLds {
    static constexpr bool kIds = true;
    int64_t id[kFsObsLds];
    int32_t seen[kFsObsLds];
};

// The next cnt <= kFsObsLds of obs[base .. nobs) into so (seen is read only with
// ids); returns cnt.  Every lane must reach both barriers.
template <typename Lds>
__device__ __forceinline__ int32_t fs_stage(Lds& so, const FsObs* __restrict__ obs,
                                            const int32_t* __restrict__ seen, const int32_t base,
                                            const int32_t nobs) {
    const int32_t cnt = nobs - base < kFsObsLds ? nobs - base : kFsObsLds;
    __syncthreads();
    if ((int32_t)threadIdx.x < cnt) {
        const FsObs o = obs[base + threadIdx.x];
        so.d[threadIdx.x] = o.d;
        so.phi[threadIdx.x] = o.phi;
        so.psi[threadIdx.x] = o.psi;
        so.r0[threadIdx.x] = o.r0;
        so.r1[threadIdx.x] = o.r1;
        so.rx[threadIdx.x] = o.rx;
        so.ry[threadIdx.x] = o.ry;
        so.vo[threadIdx.x] = o.vo;
        if constexpr (Lds::kIds) {
            so.id[threadIdx.x] = o.id;
            so.seen[threadIdx.x] = seen[o.id];
        }
    }
    __syncthreads();
    return cnt;
}

// ---- the innovation of observation z of landmark lm from F: H the landmark
// Jacobian, T = P H^T, S = H T + R, e the residual
struct FsInnov {
    double h00, h01, h10, h11, t00, t01, t10, t11, s00, s01, s11, det, e0, e1;
};

__device__ __forceinline__ FsInnov fs_innov(const FsLm& lm, const FsFrame& F, const FsZ& z) {
    const double dx = lm.mx - F.x, dy = lm.my - F.y;
    const double q = dx * dx + dy * dy, r = sqrt(q);
    const double bearing = atan2(F.s * dx + F.c * dy, F.c * dx - F.s * dy);
    FsInnov in;
    in.h00 = dx / r, in.h01 = dy / r, in.h10 = -dy / q, in.h11 = dx / q;
    in.t00 = lm.pxx * in.h00 + lm.pxy * in.h01, in.t01 = lm.pxx * in.h10 + lm.pxy * in.h11;
    in.t10 = lm.pxy * in.h00 + lm.pyy * in.h01, in.t11 = lm.pxy * in.h10 + lm.pyy * in.h11;
    in.s00 = in.h00 * in.t00 + in.h01 * in.t10 + z.r0;
    in.s01 = in.h00 * in.t01 + in.h01 * in.t11;
    in.s11 = in.h10 * in.t01 + in.h11 * in.t11 + z.r1;
    in.det = in.s00 * in.s11 - in.s01 * in.s01;
    in.e0 = z.d - r, in.e1 = wrap_angle(z.phi - bearing);
    return in;
}

// The log density of the residual without its constant: -(e^T S^-1 e + log det S) / 2
__device__ __forceinline__ double fs_score(const FsInnov& in) {
    const double maha =
        (in.e0 * in.e0 * in.s11 - 2.0 * (in.e0 * in.e1) * in.s01 + in.e1 * in.e1 * in.s00) / in.det;
    return -(maha + log(in.det)) / 2.0;
}

// The Kalman update of the landmark in row m by observation z from F, stored
// where store holds; returns the observation's score under the prior
__device__ __forceinline__ double fs_landmark_update(double* m, const int64_t npad,
                                                     const FsFrame& F, const FsZ& z,
                                                     const bool store) {
    const FsLm lm = fs_lm_load(m, npad);
    const FsInnov in = fs_innov(lm, F, z);
    const double k00 = (in.t00 * in.s11 - in.t01 * in.s01) / in.det,
                 k01 = (in.t01 * in.s00 - in.t00 * in.s01) / in.det;
    const double k10 = (in.t10 * in.s11 - in.t11 * in.s01) / in.det,
                 k11 = (in.t11 * in.s00 - in.t10 * in.s01) / in.det;
    const double m00 = k00 * in.s00 + k01 * in.s01, m01 = k00 * in.s01 + k01 * in.s11;
    const double m10 = k10 * in.s00 + k11 * in.s01, m11 = k10 * in.s01 + k11 * in.s11;
    if (store)
        fs_lm_store(m, npad,
                    FsLm{lm.mx + (k00 * in.e0 + k01 * in.e1), lm.my + (k10 * in.e0 + k11 * in.e1),
                         lm.pxx - (m00 * k00 + m01 * k01), lm.pxy - (m00 * k10 + m01 * k11),
                         lm.pyy - (m10 * k10 + m11 * k11)});
    return fs_score(in);
}

// First sighting: the observation placed in the world, and its covariance
// through the inverse of the landmark Jacobian
__device__ __forceinline__ void fs_landmark_init(double* m, const int64_t npad, const FsFrame& F,
                                                 const FsZ& z, const bool store) {
    const double R0 = z.r0, R1 = z.r1;
    const double dx = F.c * z.rx + F.s * z.ry, dy = -F.s * z.rx + F.c * z.ry;
    const double q = dx * dx + dy * dy, r = sqrt(q);
    const double a00 = dx / r, a01 = -dy, a10 = dy / r, a11 = dx;
    if (store)
        fs_lm_store(m, npad,
                    FsLm{F.x + dx, F.y + dy, a00 * a00 * R0 + a01 * a01 * R1,
                         a00 * a10 * R0 + a01 * a11 * R1, a10 * a10 * R0 + a11 * a11 * R1});
}

// ---- FastSLAM 2.0's three-state Kalman filter on the pose
struct FsPropQ {
    double q00, q01, q02, q11, q12, q22;    // Q = F^T F of the handle's q_factor
};

struct FsPose {
    double x, y, t;                         // the mean
    double c00, c01, c02, c11, c12, c22;    // the covariance's upper triangle
};

// The noise-free motion (predict_particle's linear model without its noise) with covariance Q
__device__ __forceinline__ FsPose fs_pose_predict(const double x, const double y, const double th,
                                                  const double dt, const double v, const double om,
                                                  const FsPropQ& Q) {
    double sn, cs;
    fast_sincos(th, &sn, &cs);
    return FsPose{x + v * (dt * cs), y + v * (dt * sn), wrap_angle(th + om * dt),
                  Q.q00, Q.q01, Q.q02, Q.q11, Q.q12, Q.q22};
}

// The scalar update by an observed orientation zpsi (variance vo) with
// H = (0, 0, -1); its log density goes to L
__device__ __forceinline__ void fs_pose_orient_update(FsPose& P, double& L, const double zpsi,
                                                      const double vo) {
    const double e = wrap_angle(zpsi - wrap_angle(kHalfPi - P.t));
    const double so = P.c22 + vo;
    L -= (e * e / so + log(so)) / 2.0;
    const double k0 = P.c02 / so, k1 = P.c12 / so, k2 = P.c22 / so;
    const double b0 = P.c02, b1 = P.c12, b2 = P.c22;
    P.x -= k0 * e;
    P.y -= k1 * e;
    P.t -= k2 * e;
    P.c00 -= k0 * b0;
    P.c01 -= k0 * b1;
    P.c02 -= k0 * b2;
    P.c11 -= k1 * b1;
    P.c12 -= k1 * b2;
    P.c22 -= k2 * b2;
}

// A = Sigma H_x^T with H_x = [-H_m | (0, -1)^T]
struct FsInnovPose {
    double a00, a01, a10, a11, a20, a21;
};

// An innovation taken at the pose's mean, extended by the pose's covariance:
// S = H_m P H_m^T + R + H_x A in place, and A returned
__device__ __forceinline__ FsInnovPose fs_innov_pose(FsInnov& in, const FsPose& P) {
    FsInnovPose A;
    A.a00 = -(P.c00 * in.h00 + P.c01 * in.h01), A.a01 = -(P.c00 * in.h10 + P.c01 * in.h11) - P.c02;
    A.a10 = -(P.c01 * in.h00 + P.c11 * in.h01), A.a11 = -(P.c01 * in.h10 + P.c11 * in.h11) - P.c12;
    A.a20 = -(P.c02 * in.h00 + P.c12 * in.h01), A.a21 = -(P.c02 * in.h10 + P.c12 * in.h11) - P.c22;
    in.s00 -= in.h00 * A.a00 + in.h01 * A.a10;
    in.s01 -= in.h00 * A.a01 + in.h01 * A.a11;
    in.s11 -= in.h10 * A.a01 + in.h11 * A.a11 + A.a21;
    in.det = in.s00 * in.s11 - in.s01 * in.s01;
    return A;
}

// The pose's Kalman update by observation z of the landmark in row m (only
// read), linearised at the mean; returns the observation's score
__device__ __forceinline__ double fs_pose_update(FsPose& P, const FsLm& lm, const FsFrame& F,
                                                 const FsZ& z) {
    FsInnov in = fs_innov(lm, F, z);
    const FsInnovPose A = fs_innov_pose(in, P);
    const double k00 = (A.a00 * in.s11 - A.a01 * in.s01) / in.det,
                 k01 = (A.a01 * in.s00 - A.a00 * in.s01) / in.det;
    const double k10 = (A.a10 * in.s11 - A.a11 * in.s01) / in.det,
                 k11 = (A.a11 * in.s00 - A.a10 * in.s01) / in.det;
    const double k20 = (A.a20 * in.s11 - A.a21 * in.s01) / in.det,
                 k21 = (A.a21 * in.s00 - A.a20 * in.s01) / in.det;
    P.x += k00 * in.e0 + k01 * in.e1;
    P.y += k10 * in.e0 + k11 * in.e1;
    P.t += k20 * in.e0 + k21 * in.e1;
    P.c00 -= k00 * A.a00 + k01 * A.a01;
    P.c01 -= k00 * A.a10 + k01 * A.a11;
    P.c02 -= k00 * A.a20 + k01 * A.a21;
    P.c11 -= k10 * A.a10 + k11 * A.a11;
    P.c12 -= k10 * A.a20 + k11 * A.a21;
    P.c22 -= k20 * A.a20 + k21 * A.a21;
    return fs_score(in);
}

// ---- association: the best of a particle's unmatched slots for
// observation z from F.  The wave walks the slots below jmax, its largest
// count: every lane reads the same row (512 contiguous bytes per component, 256
// of stamps); lanes past their own count cnt0 or on a slot already matched in
// this call are masked.  Without a candidate best is -inf and bj -1.
__device__ __forceinline__ void fs_best_slot(const double* map, const int32_t* stamp,
                                             const int64_t npad, const int64_t p,
                                             const int32_t jmax, const int32_t cnt0,
                                             const int32_t call, const FsFrame& F, const FsZ& z,
                                             double& best, int32_t& bj) {
    best = -INFINITY;
    bj = -1;
#pragma unroll 1
    for (int32_t j = 0; j < jmax; ++j) {
        const int32_t st = stamp[(size_t)j * (size_t)npad + (size_t)p];
        const FsLm lm = fs_lm_load(fs_row(map, j, npad, p), npad);
        const double l = fs_score(fs_innov(lm, F, z)) - kFsLn2Pi;
        // strictly greater: a tie keeps the lowest slot; NaN never wins
        if (j < cnt0 && st != call && l > best) {
            best = l;
            bj = j;
        }
    }
}

// The draw's three standard normals: noise[p][0..2] (HOSTNOISE) or the
// particle's half of its pair's device normals, as the fused kernel deals them
struct FsXi {
    double xi0, xi1, xi2;
};

template <bool HOSTNOISE>
__device__ __forceinline__ FsXi fs_normals(const int64_t p, const double* __restrict__ noise,
                                           const uint32_t rstep, const uint64_t seed,
                                           const RngTabs& rtab) {
    if constexpr (HOSTNOISE) {
        return FsXi{noise[3 * p], noise[3 * p + 1], noise[3 * p + 2]};
    } else {
        double g[6];
        pair_normals((uint64_t)p >> 1, rstep, seed, rtab, g);
        const bool odd = (p & 1) != 0;
        return FsXi{odd ? g[3] : g[0], odd ? g[4] : g[1], odd ? g[5] : g[2]};
    }
}

// The draw: pose = mean + chol(cov) xi (a non-positive pivot gives NaN), as
// the frame of the sampled pose and its heading th
__device__ __forceinline__ FsFrame fs_pose_draw(const FsPose& P, const FsXi& xi, double& th) {
    const double xi0 = xi.xi0, xi1 = xi.xi1, xi2 = xi.xi2;
    const double l00 = sqrt(P.c00), l10 = P.c01 / l00, l20 = P.c02 / l00;
    const double l11 = sqrt(P.c11 - l10 * l10), l21 = (P.c12 - l20 * l10) / l11;
    const double l22 = sqrt(P.c22 - l20 * l20 - l21 * l21);
    th = P.t + (l20 * xi0 + l21 * xi1 + l22 * xi2);
    return fs_frame(P.x + l00 * xi0, P.y + (l10 * xi0 + l11 * xi1), th);
}

// rec: [9][npad], the mean and the covariance (00 01 02 11 12 22) before sampling
__device__ __forceinline__ void fs_pose_record(double* __restrict__ rec, const int64_t npad,
                                               const int64_t p, const FsPose& P) {
    rec[p] = P.x;
    rec[(size_t)npad + p] = P.y;
    rec[2 * (size_t)npad + p] = P.t;
    rec[3 * (size_t)npad + p] = P.c00;
    rec[4 * (size_t)npad + p] = P.c01;
    rec[5 * (size_t)npad + p] = P.c02;
    rec[6 * (size_t)npad + p] = P.c11;
    rec[7 * (size_t)npad + p] = P.c12;
    rec[8 * (size_t)npad + p] = P.c22;
}

// ------------------------------------------------------------------------
// FastSLAM 1.0 with known association
// ------------------------------------------------------------------------
// One lane per particle, a loop over the step's observations (staged in LDS
// kFsObsLds at a time).  Writes the particle's log weight L and the block's
// maximum of L.
__global__ __launch_bounds__(kFsThreads) void fs_update_kernel(
    const int64_t n, const int64_t npad, const double* __restrict__ xs,
    const double* __restrict__ ys, const double* __restrict__ ts, double* __restrict__ map,
    const int32_t nobs, const FsObs* __restrict__ obs, const int32_t* __restrict__ seen,
    const int32_t use_orient, double* __restrict__ L_out, double* __restrict__ bmax) {
    __shared__ FsObsLds so;
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    const bool valid = p < n;
    const int64_t pc = valid ? p : n - 1;
    const FsFrame F = fs_frame(xs[pc], ys[pc], ts[pc]);
    const double psi_w = wrap_angle(kHalfPi - ts[pc]);
    double L = 0.0;
    for (int32_t base = 0; base < nobs; base += kFsObsLds) {
        const int32_t cnt = fs_stage(so, obs, seen, base, nobs);
        for (int32_t t = 0; t < cnt; ++t) {
            const FsZ z = so.z(t);
            double* m = fs_row(map, so.id[t], npad, pc);
            if (use_orient) {
                const double e = wrap_angle(so.psi[t] - psi_w);
                L -= e * e / (2.0 * so.vo[t]);
            }
            if (so.seen[t])
                L += fs_landmark_update(m, npad, F, z, valid);
            else
                fs_landmark_init(m, npad, F, z, valid);
        }
    }
    if (valid) L_out[p] = L;
    const double bm = fs_block_max(valid ? L : -INFINITY);
    if (threadIdx.x == 0) bmax[blockIdx.x] = bm;
}

// The grid maximum: a plain fold of the block maxima
__global__ __launch_bounds__(kFsThreads) void fs_max_fold_kernel(const double* __restrict__ bmax,
                                                                 const int32_t nb,
                                                                 double* __restrict__ gmax) {
    double v = -INFINITY;
    for (int32_t b = threadIdx.x; b < nb; b += kFsThreads) v = fmax(v, bmax[b]);
    v = fs_block_max(v);
    if (threadIdx.x == 0) *gmax = v;
}

// w_un = w exp(L - max L): the weights in the log domain (a product of k
// densities overflows fp64 near k = 300)
__global__ __launch_bounds__(kFsThreads) void fs_weight_kernel(const int64_t n,
                                                               const double* __restrict__ L,
                                                               const double* __restrict__ gmax,
                                                               double* __restrict__ w_un) {
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= n) return;
    w_un[p] = w_un[p] * exp(L[p] - *gmax);
}

__global__ __launch_bounds__(kFsThreads) void fs_mark_seen_kernel(const int32_t nobs,
                                                                  const FsObs* __restrict__ obs,
                                                                  int32_t* __restrict__ seen) {
    const int32_t t = (int32_t)(blockIdx.x * kFsThreads + threadIdx.x);
    if (t < nobs) seen[obs[t].id] = 1;
}

// Resampling gather of the maps: particle p of the other ping-pong half takes
// the rows of its source idx[p] for every seen landmark (list[0..nlist)).
// blockIdx.y walks the seen landmarks; idx is non-decreasing, so the lanes of
// a wave read neighbouring or equal addresses in each of the five components.
__global__ __launch_bounds__(kFsThreads) void fs_map_gather_kernel(
    const int64_t n, const int64_t npad, const int32_t* __restrict__ idx,
    const int32_t* __restrict__ list, const int32_t nlist, const double* __restrict__ src,
    double* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= n) return;
    const int64_t q = idx[p];
    for (int32_t k = blockIdx.y; k < nlist; k += gridDim.y)
        fs_row_copy(fs_row(src, list[k], npad, q), fs_row(dst, list[k], npad, p), npad);
}

// host layout [NP][NL][ncomp] <-> component-major device layout; comp0 = 0
// (the means, ncomp 2) or 2 (the covariances, ncomp 3).  An unseen landmark
// reads back as NaN.
__global__ __launch_bounds__(kFsThreads) void fs_map_pack_kernel(
    const int64_t n, const int64_t npad, const int32_t nl, const int64_t p0, const int64_t count,
    const int32_t comp0, const int32_t ncomp, const int32_t* __restrict__ seen,
    const double* __restrict__ map, double* __restrict__ out) {
    const int64_t p = p0 + (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= p0 + count || p >= n) return;
    for (int32_t j = blockIdx.y; j < nl; j += gridDim.y) {
        const bool sj = seen[j] != 0;
        for (int32_t c = 0; c < ncomp; ++c)
            out[((size_t)(p - p0) * nl + j) * ncomp + c] =
                sj ? map[((size_t)kFsComp * j + comp0 + c) * (size_t)npad + (size_t)p] : NAN;
    }
}

__global__ __launch_bounds__(kFsThreads) void fs_map_unpack_kernel(
    const int64_t n, const int64_t npad, const int32_t nl, const int32_t comp0, const int32_t ncomp,
    const double* __restrict__ in, double* __restrict__ map) {
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= n) return;
    for (int32_t j = blockIdx.y; j < nl; j += gridDim.y)
        for (int32_t c = 0; c < ncomp; ++c)
            map[((size_t)kFsComp * j + comp0 + c) * (size_t)npad + (size_t)p] =
                in[((size_t)p * nl + j) * ncomp + c];
}

// ------------------------------------------------------------------------
// Per-particle maximum-likelihood data association.  Particle p
// holds cnt[p] landmarks in slots 0..cnt[p]-1 of the same component-major map;
// stamp[j * npad + p] is the number of the update call that last matched slot
// j of particle p (a scan sees each landmark once).
// ------------------------------------------------------------------------
// One lane per particle.  Per observation the best slot (fs_best_slot) is
// updated from a re-read of its row; without a candidate, or below log_p_new,
// the observation starts slot cnt (dropped at cap).
// assoc (NULL unless recorded) takes the choice: slot, -1 new, -2 dropped.
__global__ __launch_bounds__(kFsThreads) void fs_assoc_update_kernel(
    const int64_t n, const int64_t npad, const double* __restrict__ xs,
    const double* __restrict__ ys, const double* __restrict__ ts, double* __restrict__ map,
    int32_t* __restrict__ cnt_io, int32_t* __restrict__ stamp, const int32_t call,
    const int32_t cap, const int32_t nobs, const FsObs* __restrict__ obs, const int32_t use_orient,
    const double log_p_new, int32_t* __restrict__ assoc, double* __restrict__ L_out,
    double* __restrict__ bmax, int32_t* __restrict__ bcnt) {
    __shared__ FsScanLds so;
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    const bool valid = p < n;
    const int64_t pc = valid ? p : n - 1;
    const FsFrame F = fs_frame(xs[pc], ys[pc], ts[pc]);
    const double psi_w = wrap_angle(kHalfPi - ts[pc]);
    const int32_t cnt0 = valid ? cnt_io[p] : 0;     // padding lanes: no candidates, no stores
    const int32_t jmax = __builtin_amdgcn_readfirstlane(fs_wave_max(cnt0));
    int32_t cnt = cnt0;
    double L = 0.0;
    for (int32_t base = 0; base < nobs; base += kFsObsLds) {
        const int32_t m_obs = fs_stage(so, obs, nullptr, base, nobs);
        for (int32_t t = 0; t < m_obs; ++t) {
            const FsZ z = so.z(t);
            if (use_orient) {
                const double e = wrap_angle(so.psi[t] - psi_w);
                L -= e * e / (2.0 * so.vo[t]);
            }
            double best;
            int32_t bj;
            fs_best_slot(map, stamp, npad, pc, jmax, cnt0, call, F, z, best, bj);
            int32_t a;
            if (bj < 0 || best < log_p_new) {
                L += log_p_new;
                a = -2;
                if (cnt < cap) {
                    fs_landmark_init(fs_row(map, cnt, npad, pc), npad, F, z, valid);
                    a = -1;
                    ++cnt;
                }
            } else {
                // bj >= 0 implies a valid lane (padding lanes have no candidates)
                L += best;
                fs_landmark_update(fs_row(map, bj, npad, pc), npad, F, z, true);
                stamp[(size_t)bj * (size_t)npad + (size_t)pc] = call;
                a = bj;
            }
            if (assoc && valid) assoc[(size_t)(base + t) * (size_t)npad + (size_t)p] = a;
        }
    }
    if (valid) {
        L_out[p] = L;
        cnt_io[p] = cnt;
    }
    double bm = valid ? L : -INFINITY;
    int32_t bc = valid ? cnt : 0;
    fs_block_max(bm, bc);
    if (threadIdx.x == 0) {
        bmax[blockIdx.x] = bm;
        bcnt[blockIdx.x] = bc;
    }
}

// fs_max_fold_kernel with the block maxima of the counts beside it; the
// largest count goes to the host's coherent word (read with the step's record)
__global__ __launch_bounds__(kFsThreads) void fs_assoc_fold_kernel(
    const double* __restrict__ bmax, const int32_t* __restrict__ bcnt, const int32_t nb,
    double* __restrict__ gmax, int32_t* __restrict__ cmax_host) {
    double v = -INFINITY;
    int32_t u = 0;
    for (int32_t b = threadIdx.x; b < nb; b += kFsThreads) {
        v = fmax(v, bmax[b]);
        u = bcnt[b] > u ? bcnt[b] : u;
    }
    fs_block_max(v, u);
    if (threadIdx.x == 0) {
        *gmax = v;
        *cmax_host = u;
    }
}

// Resampling gather of an associating handle: the counts move with the poses
// (blockIdx.y == 0), and particle p takes the rows of its source below the
// source's own count, of the rows below nrows >= max cnt that the grid walks.
__global__ __launch_bounds__(kFsThreads) void fs_assoc_gather_kernel(
    const int64_t n, const int64_t npad, const int32_t* __restrict__ idx, const int32_t nrows,
    const double* __restrict__ src, double* __restrict__ dst, const int32_t* __restrict__ cnt_src,
    int32_t* __restrict__ cnt_dst) {
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= n) return;
    const int64_t q = idx[p];
    const int32_t cq = cnt_src[q];
    if (blockIdx.y == 0) cnt_dst[p] = cq;
    const int32_t lim = cq < nrows ? cq : nrows;
    for (int32_t j = blockIdx.y; j < lim; j += gridDim.y)
        fs_row_copy(fs_row(src, j, npad, q), fs_row(dst, j, npad, p), npad);
}

// fs_map_pack_kernel masked by the particle's own count instead of seen[j]
__global__ __launch_bounds__(kFsThreads) void fs_assoc_pack_kernel(
    const int64_t n, const int64_t npad, const int32_t nl, const int64_t p0, const int64_t count,
    const int32_t comp0, const int32_t ncomp, const int32_t* __restrict__ cnt,
    const double* __restrict__ map, double* __restrict__ out) {
    const int64_t p = p0 + (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= p0 + count || p >= n) return;
    const int32_t cp = cnt[p];
    for (int32_t j = blockIdx.y; j < nl; j += gridDim.y)
        for (int32_t c = 0; c < ncomp; ++c)
            out[((size_t)(p - p0) * nl + j) * ncomp + c] =
                j < cp ? map[((size_t)kFsComp * j + comp0 + c) * (size_t)npad + (size_t)p] : NAN;
}

// ------------------------------------------------------------------------
// FastSLAM 2.0: the pose is drawn from the proposal that has seen
// the step's scan.  Known association, linear motion.
// ------------------------------------------------------------------------
// One lane per particle, one launch, two passes over the step's observations.
// Pass 1 runs the three-state Kalman filter on the pose: from the noise-free
// motion with covariance Q through the orientation of every observation and
// the range and bearing of every seen landmark (linearised at the current
// mean and the landmark's prior), collecting the log weight L on the way.  The
// pose is then drawn (fs_pose_draw).  Pass 2 is fs_update_kernel's map update
// at that pose, without the weight term.  The poses go to the other ping-pong
// half; the previous weights are normalised in place (w_un / s, as the 1.0
// predict leaves them).  rec (NULL unless recorded): fs_pose_record.
// Three waves per SIMD, no scratch, as fs_update_kernel; held to four the
// compiler spills 22 to 90 registers.
template <bool HOSTNOISE>
__global__ __launch_bounds__(kFsThreads) void
fs_proposal_kernel(const int64_t n, const int64_t npad, const double* __restrict__ xs,
                   const double* __restrict__ ys, const double* __restrict__ ts,
                   double* __restrict__ xo, double* __restrict__ yo, double* __restrict__ to,
                   double* __restrict__ w_un, const double* __restrict__ s_in,
                   const double np_recip, double* __restrict__ map, const int32_t nobs,
                   const FsObs* __restrict__ obs, const int32_t* __restrict__ seen,
                   const int32_t use_orient, const double dt, const double v, const double om,
                   const FsPropQ Q, const double* __restrict__ noise, const uint32_t rstep,
                   const uint64_t seed, double* __restrict__ rec, double* __restrict__ L_out,
                   double* __restrict__ bmax) {
    __shared__ FsObsLds so;
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    const bool valid = p < n;
    const int64_t pc = valid ? p : n - 1;
    // host normals: loaded ahead of the filter, which hides the load.  The
    // device RNG runs after it, where only the pose and L are live (drawn first
    // it costs a wave per SIMD: DESIGN 11d); its tables are staged here.
    FsXi xi{};
    RngTabs rtab{};
    if constexpr (HOSTNOISE) {
        xi = fs_normals<true>(pc, noise, rstep, seed, rtab);
    } else {
        __shared__ RngTabsLds s_rng;
        rtab = rng_tabs_stage(&s_rng, (int)threadIdx.x, kFsThreads);
        __syncthreads();
    }
    const double wprev = w_un[pc];
    FsPose P = fs_pose_predict(xs[pc], ys[pc], ts[pc], dt, v, om, Q);
    double L = 0.0;
    // ---- pass 1: the proposal
    for (int32_t base = 0; base < nobs; base += kFsObsLds) {
        const int32_t cnt = fs_stage(so, obs, seen, base, nobs);
        for (int32_t t = 0; t < cnt; ++t) {
            if (use_orient) fs_pose_orient_update(P, L, so.psi[t], so.vo[t]);
            if (!so.seen[t]) continue;          // a first sighting carries no pose information
            // the row's loads ahead of the sincos, which hides them (behind it the
            // launch is 2 to 5 % slower: profiles/fastslam_shared_ab.txt)
            const FsLm lm = fs_lm_load(fs_row(map, so.id[t], npad, pc), npad);
            L += fs_pose_update(P, lm, fs_frame(P.x, P.y, P.t), so.z(t));
        }
    }
    if constexpr (!HOSTNOISE) xi = fs_normals<false>(pc, noise, rstep, seed, rtab);
    double th;
    const FsFrame F = fs_pose_draw(P, xi, th);
    if (valid) {
        xo[p] = F.x;
        yo[p] = F.y;
        to[p] = th;
        w_un[p] = norm_w(wprev, *s_in, np_recip);
        L_out[p] = L;
        if (rec) fs_pose_record(rec, npad, p, P);
    }
    // ---- pass 2: the maps at the sampled pose
    for (int32_t base = 0; base < nobs; base += kFsObsLds) {
        const int32_t cnt = fs_stage(so, obs, seen, base, nobs);
        for (int32_t t = 0; t < cnt; ++t) {
            const FsZ z = so.z(t);
            double* m = fs_row(map, so.id[t], npad, pc);
            if (so.seen[t])
                fs_landmark_update(m, npad, F, z, valid);
            else
                fs_landmark_init(m, npad, F, z, valid);
        }
    }
    const double bm = fs_block_max(valid ? L : -INFINITY);
    if (threadIdx.x == 0) bmax[blockIdx.x] = bm;
}

// ------------------------------------------------------------------------
// FastSLAM 2.0 with per-particle maximum-likelihood association:
// the scan of fs_assoc_update_kernel with fs_proposal_kernel's three-state
// filter inside it.  No ids, linear motion.
//
// This kernel alone writes its expressions out instead of calling the
// functions above (every one of them states the same formula): it holds 166 /
// 167 of the 168 registers that three waves per SIMD allow, its schedule moves
// with any change to its source, and calling the shared functions cost the
// launch 1.3 to 2.4 % at 2^12 and 2^16 particles, of which no arrangement of a
// single call site recovered more than a third (DESIGN 11e,
// profiles/fastslam_shared_ab.txt).  A fix to a formula above is made here too;
// the lockstep tests hold both to the same oracle.
// ------------------------------------------------------------------------
// The block's next kFsObsLds observations into LDS, without ids (fs_stage's stores)
#define SLAM_FS_STAGE_SCAN(base, cnt)                                                            \
    __syncthreads();                                                                             \
    if ((int32_t)threadIdx.x < (cnt)) {                                                          \
        const FsObs o = obs[(base) + threadIdx.x];                                               \
        s_d[threadIdx.x] = o.d;                                                                  \
        s_phi[threadIdx.x] = o.phi;                                                              \
        s_psi[threadIdx.x] = o.psi;                                                              \
        s_r0[threadIdx.x] = o.r0;                                                                \
        s_r1[threadIdx.x] = o.r1;                                                                \
        s_rx[threadIdx.x] = o.rx;                                                                \
        s_ry[threadIdx.x] = o.ry;                                                                \
        s_vo[threadIdx.x] = o.vo;                                                                \
    }                                                                                            \
    __syncthreads();

// One lane per particle, one launch, two passes over the step's observations.
// Pass 1 is fs_proposal_kernel's filter on the pose with the association
// inside it: per observation the wave walks the slots below its largest count
// (every lane loads the same row and stamp; lanes past their own count or on a
// slot already matched in this call are masked), each candidate scored at the
// current mean with the pose covariance folded into S.  Only the best score
// and slot are kept: the chosen slot is re-read and its A, S and e recomputed
// for the Kalman update of the pose.  The choice (slot, -1 new, -2 dropped)
// goes to assoc[t][npad]; the maps are only read.  Then the draw, as
// fs_proposal_kernel's, and pass 2: the lane's own choices read back, and the
// map update of fs_update_kernel at the sampled pose (a new landmark in slot
// cnt).  Padding lanes have no candidates and store nothing.
// Three waves per SIMD (166 / 167 VGPRs, no scratch), as its parents.
template <bool HOSTNOISE>
__global__ __launch_bounds__(kFsThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void
fs_assoc_proposal_kernel(
    const int64_t n, const int64_t npad, const double* __restrict__ xs,
    const double* __restrict__ ys, const double* __restrict__ ts, double* __restrict__ xo,
    double* __restrict__ yo, double* __restrict__ to, double* __restrict__ w_un,
    const double* __restrict__ s_in, const double np_recip, double* __restrict__ map,
    int32_t* __restrict__ cnt_io, int32_t* __restrict__ stamp, const int32_t call,
    const int32_t cap, const int32_t nobs, const FsObs* __restrict__ obs, const int32_t use_orient,
    const double dt, const double v, const double om, const FsPropQ Q, const double log_p_new,
    const double* __restrict__ noise, const uint32_t rstep, const uint64_t seed,
    int32_t* assoc, double* __restrict__ rec, double* __restrict__ L_out,
    double* __restrict__ bmax, int32_t* __restrict__ bcnt) {
    __shared__ double s_d[kFsObsLds], s_phi[kFsObsLds], s_psi[kFsObsLds], s_r0[kFsObsLds],
        s_r1[kFsObsLds], s_rx[kFsObsLds], s_ry[kFsObsLds], s_vo[kFsObsLds];
    __shared__ double s_wmax[kFsThreads / 64];
    __shared__ int32_t s_cmax[kFsThreads / 64];
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    const bool valid = p < n;
    const int64_t pc = valid ? p : n - 1;
    // the device RNG runs after pass 1; its tables are staged here
    RngTabs rtab{};
    if constexpr (!HOSTNOISE) {
        __shared__ RngTabsLds s_rng;
        rtab = rng_tabs_stage(&s_rng, (int)threadIdx.x, kFsThreads);
        __syncthreads();
    }
    // noise-free motion: predict_particle's linear model without its noise
    double mux, muy, mut;
    {
        const double x = xs[pc], y = ys[pc], th = ts[pc];
        double sn, cs;
        fast_sincos(th, &sn, &cs);
        mux = x + v * (dt * cs);
        muy = y + v * (dt * sn);
        mut = wrap_angle(th + om * dt);
    }
    double c00 = Q.q00, c01 = Q.q01, c02 = Q.q02, c11 = Q.q11, c12 = Q.q12, c22 = Q.q22;
    const int32_t cnt0 = valid ? cnt_io[p] : 0;     // padding lanes: no candidates, no stores
    // the wave's largest count, bit by bit through ballots: a scalar, and no
    // shuffle addresses stay live across pass 1 for the reductions at the end
    // (which costs the third wave per SIMD: DESIGN 11e)
    int32_t jmax = 0;
#pragma unroll
    for (int b = 30; b >= 0; --b) {
        const int32_t probe = jmax | (int32_t(1) << b);
        if (__ballot(cnt0 >= probe) != 0) jmax = probe;
    }
    int32_t cnew = cnt0;                            // the count after this step
    double L = 0.0;
    // ---- pass 1: the proposal with the association
    for (int32_t base = 0; base < nobs; base += kFsObsLds) {
        const int32_t m_obs = nobs - base < kFsObsLds ? nobs - base : kFsObsLds;
        SLAM_FS_STAGE_SCAN(base, m_obs)
#pragma unroll 1
        for (int32_t t = 0; t < m_obs; ++t) {
            if (use_orient) {
                // scalar update with H = (0, 0, -1)
                const double e = wrap_angle(s_psi[t] - wrap_angle(kHalfPi - mut));
                const double so = c22 + s_vo[t];
                L -= (e * e / so + log(so)) / 2.0;
                const double k0 = c02 / so, k1 = c12 / so, k2 = c22 / so;
                const double b0 = c02, b1 = c12, b2 = c22;
                mux -= k0 * e;
                muy -= k1 * e;
                mut -= k2 * e;
                c00 -= k0 * b0;
                c01 -= k0 * b1;
                c02 -= k0 * b2;
                c11 -= k1 * b1;
                c12 -= k1 * b2;
                c22 -= k2 * b2;
            }
            double s, c;
            sincos(kHalfPi - mut, &s, &c);
            double best = -INFINITY;
            int32_t bj = -1;
            {
                const double R0 = s_r0[t], R1 = s_r1[t], zd = s_d[t], zphi = s_phi[t];
#pragma unroll 1
                for (int32_t j = 0; j < jmax; ++j) {
                    const size_t row = (size_t)kFsComp * (size_t)j * (size_t)npad + (size_t)pc;
                    const int32_t st = stamp[(size_t)j * (size_t)npad + (size_t)pc];
                    const double mx = map[row], my = map[row + (size_t)npad];
                    const double pxx = map[row + 2 * (size_t)npad],
                                 pxy = map[row + 3 * (size_t)npad],
                                 pyy = map[row + 4 * (size_t)npad];
                    const double dx = mx - mux, dy = my - muy;
                    const double q = dx * dx + dy * dy, r = sqrt(q);
                    const double bearing = atan2(s * dx + c * dy, c * dx - s * dy);
                    const double h00 = dx / r, h01 = dy / r, h10 = -dy / q, h11 = dx / q;
                    const double t00 = pxx * h00 + pxy * h01, t01 = pxx * h10 + pxy * h11;
                    const double t10 = pxy * h00 + pyy * h01, t11 = pxy * h10 + pyy * h11;
                    const double a00 = -(c00 * h00 + c01 * h01),
                                 a01 = -(c00 * h10 + c01 * h11) - c02;
                    const double a10 = -(c01 * h00 + c11 * h01),
                                 a11 = -(c01 * h10 + c11 * h11) - c12;
                    const double a21 = -(c02 * h10 + c12 * h11) - c22;
                    const double s00 = (h00 * t00 + h01 * t10 + R0) - (h00 * a00 + h01 * a10);
                    const double s01 = (h00 * t01 + h01 * t11) - (h00 * a01 + h01 * a11);
                    const double s11 = (h10 * t01 + h11 * t11 + R1) - (h10 * a01 + h11 * a11 + a21);
                    const double det = s00 * s11 - s01 * s01;
                    const double e0 = zd - r, e1 = wrap_angle(zphi - bearing);
                    const double maha =
                        (e0 * e0 * s11 - 2.0 * (e0 * e1) * s01 + e1 * e1 * s00) / det;
                    const double l = -(maha + log(det)) / 2.0 - kFsLn2Pi;
                    // strictly greater: a tie keeps the lowest slot; NaN never wins
                    if (j < cnt0 && st != call && l > best) {
                        best = l;
                        bj = j;
                    }
                }
            }
            int32_t a;
            if (bj < 0 || best < log_p_new) {
                // a first sighting carries no pose information
                L += log_p_new;
                a = -2;
                if (cnew < cap) {
                    a = -1;
                    ++cnew;
                }
            } else {
                const double R0 = s_r0[t], R1 = s_r1[t];
                const double* m = map + (size_t)kFsComp * (size_t)bj * (size_t)npad + (size_t)pc;
                const double mx = m[0], my = m[(size_t)npad];
                const double pxx = m[2 * (size_t)npad], pxy = m[3 * (size_t)npad],
                             pyy = m[4 * (size_t)npad];
                const double dx = mx - mux, dy = my - muy;
                const double q = dx * dx + dy * dy, r = sqrt(q);
                const double bearing = atan2(s * dx + c * dy, c * dx - s * dy);
                const double h00 = dx / r, h01 = dy / r, h10 = -dy / q, h11 = dx / q;
                const double t00 = pxx * h00 + pxy * h01, t01 = pxx * h10 + pxy * h11;
                const double t10 = pxy * h00 + pyy * h01, t11 = pxy * h10 + pyy * h11;
                // A = Sigma H_x^T with H_x = [-H_m | (0, -1)^T]
                const double a00 = -(c00 * h00 + c01 * h01), a01 = -(c00 * h10 + c01 * h11) - c02;
                const double a10 = -(c01 * h00 + c11 * h01), a11 = -(c01 * h10 + c11 * h11) - c12;
                const double a20 = -(c02 * h00 + c12 * h01), a21 = -(c02 * h10 + c12 * h11) - c22;
                // S = H_m P H_m^T + R + H_x A
                const double s00 = (h00 * t00 + h01 * t10 + R0) - (h00 * a00 + h01 * a10);
                const double s01 = (h00 * t01 + h01 * t11) - (h00 * a01 + h01 * a11);
                const double s11 = (h10 * t01 + h11 * t11 + R1) - (h10 * a01 + h11 * a11 + a21);
                const double det = s00 * s11 - s01 * s01;
                const double e0 = s_d[t] - r, e1 = wrap_angle(s_phi[t] - bearing);
                L += best;
                const double k00 = (a00 * s11 - a01 * s01) / det, k01 = (a01 * s00 - a00 * s01) / det;
                const double k10 = (a10 * s11 - a11 * s01) / det, k11 = (a11 * s00 - a10 * s01) / det;
                const double k20 = (a20 * s11 - a21 * s01) / det, k21 = (a21 * s00 - a20 * s01) / det;
                mux += k00 * e0 + k01 * e1;
                muy += k10 * e0 + k11 * e1;
                mut += k20 * e0 + k21 * e1;
                c00 -= k00 * a00 + k01 * a01;
                c01 -= k00 * a10 + k01 * a11;
                c02 -= k00 * a20 + k01 * a21;
                c11 -= k10 * a10 + k11 * a11;
                c12 -= k10 * a20 + k11 * a21;
                c22 -= k20 * a20 + k21 * a21;
                // bj >= 0 implies a valid lane (padding lanes have no candidates)
                stamp[(size_t)bj * (size_t)npad + (size_t)pc] = call;
                a = bj;
            }
            if (valid) assoc[(size_t)(base + t) * (size_t)npad + (size_t)p] = a;
        }
    }
    // ---- sample: pose = mean + chol(cov) xi (a non-positive pivot gives NaN)
    double xi0, xi1, xi2;
    if constexpr (HOSTNOISE) {
        xi0 = noise[3 * pc];
        xi1 = noise[3 * pc + 1];
        xi2 = noise[3 * pc + 2];
    } else {
        double g[6];
        pair_normals((uint64_t)pc >> 1, rstep, seed, rtab, g);
        const bool odd = (pc & 1) != 0;
        xi0 = odd ? g[3] : g[0];
        xi1 = odd ? g[4] : g[1];
        xi2 = odd ? g[5] : g[2];
    }
    const double l00 = sqrt(c00), l10 = c01 / l00, l20 = c02 / l00;
    const double l11 = sqrt(c11 - l10 * l10), l21 = (c12 - l20 * l10) / l11;
    const double l22 = sqrt(c22 - l20 * l20 - l21 * l21);
    const double x = mux + l00 * xi0;
    const double y = muy + (l10 * xi0 + l11 * xi1);
    const double th = mut + (l20 * xi0 + l21 * xi1 + l22 * xi2);
    if (valid) {
        xo[p] = x;
        yo[p] = y;
        to[p] = th;
        w_un[p] = norm_w(w_un[p], *s_in, np_recip);
        L_out[p] = L;
        cnt_io[p] = cnew;
        if (rec) {
            rec[p] = mux;
            rec[(size_t)npad + p] = muy;
            rec[2 * (size_t)npad + p] = mut;
            rec[3 * (size_t)npad + p] = c00;
            rec[4 * (size_t)npad + p] = c01;
            rec[5 * (size_t)npad + p] = c02;
            rec[6 * (size_t)npad + p] = c11;
            rec[7 * (size_t)npad + p] = c12;
            rec[8 * (size_t)npad + p] = c22;
        }
    }
    // ---- pass 2: the maps at the sampled pose, by the recorded choices
    // (fs_update_kernel's expressions).  Pass 1 read every prior it needed.
    const double psi_p = kHalfPi - th;
    double s, c;
    sincos(psi_p, &s, &c);
    int32_t cnt = cnt0;
    for (int32_t base = 0; base < nobs; base += kFsObsLds) {
        const int32_t m_obs = nobs - base < kFsObsLds ? nobs - base : kFsObsLds;
        SLAM_FS_STAGE_SCAN(base, m_obs)
#pragma unroll 1
        for (int32_t t = 0; t < m_obs; ++t) {
            // the lane's own store of pass 1; padding lanes do nothing
            const int32_t a = valid ? assoc[(size_t)(base + t) * (size_t)npad + (size_t)p] : -2;
            const double R0 = s_r0[t], R1 = s_r1[t];
            if (a == -1) {
                double* m = map + (size_t)kFsComp * (size_t)cnt * (size_t)npad + (size_t)pc;
                const double rx = s_rx[t], ry = s_ry[t];
                const double dx = c * rx + s * ry, dy = -s * rx + c * ry;
                const double q = dx * dx + dy * dy, r = sqrt(q);
                const double a00 = dx / r, a01 = -dy, a10 = dy / r, a11 = dx;
                m[0] = x + dx;
                m[(size_t)npad] = y + dy;
                m[2 * (size_t)npad] = a00 * a00 * R0 + a01 * a01 * R1;
                m[3 * (size_t)npad] = a00 * a10 * R0 + a01 * a11 * R1;
                m[4 * (size_t)npad] = a10 * a10 * R0 + a11 * a11 * R1;
                ++cnt;
            } else if (a >= 0) {
                double* m = map + (size_t)kFsComp * (size_t)a * (size_t)npad + (size_t)pc;
                const double mx = m[0], my = m[(size_t)npad];
                const double pxx = m[2 * (size_t)npad], pxy = m[3 * (size_t)npad],
                             pyy = m[4 * (size_t)npad];
                const double dx = mx - x, dy = my - y;
                const double q = dx * dx + dy * dy, r = sqrt(q);
                const double bearing = atan2(s * dx + c * dy, c * dx - s * dy);
                const double h00 = dx / r, h01 = dy / r, h10 = -dy / q, h11 = dx / q;
                const double t00 = pxx * h00 + pxy * h01, t01 = pxx * h10 + pxy * h11;
                const double t10 = pxy * h00 + pyy * h01, t11 = pxy * h10 + pyy * h11;
                const double s00 = h00 * t00 + h01 * t10 + R0;
                const double s01 = h00 * t01 + h01 * t11;
                const double s11 = h10 * t01 + h11 * t11 + R1;
                const double det = s00 * s11 - s01 * s01;
                const double e0 = s_d[t] - r, e1 = wrap_angle(s_phi[t] - bearing);
                const double k00 = (t00 * s11 - t01 * s01) / det, k01 = (t01 * s00 - t00 * s01) / det;
                const double k10 = (t10 * s11 - t11 * s01) / det, k11 = (t11 * s00 - t10 * s01) / det;
                const double m00 = k00 * s00 + k01 * s01, m01 = k00 * s01 + k01 * s11;
                const double m10 = k10 * s00 + k11 * s01, m11 = k10 * s01 + k11 * s11;
                m[0] = mx + (k00 * e0 + k01 * e1);
                m[(size_t)npad] = my + (k10 * e0 + k11 * e1);
                m[2 * (size_t)npad] = pxx - (m00 * k00 + m01 * k01);
                m[3 * (size_t)npad] = pxy - (m00 * k10 + m01 * k11);
                m[4 * (size_t)npad] = pyy - (m10 * k10 + m11 * k11);
            }
        }
    }
    const double wm = fs_wave_max(valid ? L : -INFINITY);
    const int32_t cm = fs_wave_max(valid ? cnew : 0);
    if ((threadIdx.x & 63) == 0) {
        s_wmax[threadIdx.x >> 6] = wm;
        s_cmax[threadIdx.x >> 6] = cm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double u = s_wmax[0];
        int32_t k = s_cmax[0];
#pragma unroll
        for (int w = 1; w < kFsThreads / 64; ++w) {
            u = fmax(u, s_wmax[w]);
            k = s_cmax[w] > k ? s_cmax[w] : k;
        }
        bmax[blockIdx.x] = u;
        bcnt[blockIdx.x] = k;
    }
}
#undef SLAM_FS_STAGE_SCAN

}  // namespace slam
