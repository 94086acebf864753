// graph_map.inl -- the landmark map of the current trajectory (gfx950).
//
// Conditional on the poses the landmarks are independent: landmark l is the
// information-weighted fusion of the half-edges that observe it.  With (x, y,
// theta) the current estimate of half-edge k's pose and (d, dir) its range and
// bearing (the measured orientation does not enter):
//   ang  = dir + theta - pi/2                  v0 = (d r_dist)^2, v1 = (d sin r_dir)^2
//   L_k  = (x + d cos ang, y + d sin ang)      (meas_var_angle: meas_cov_world's statement)
//   W_k  = R(ang) diag(1/v0, 1/v1) R(ang)^T    = C_k^-1, C_k the upper 2x2 of meas_cov_world
//   Lam  = sum_k W_k         eta = sum_k W_k (L_k - L_k0)      k0: the landmark's first half-edge
//   cov  = Lam^-1            mean = L_k0 + cov eta
//   chi2_k = (L_k - mean)^T W_k (L_k - mean)   chi2_l = sum_k chi2_k
// The covariance is that of the observations alone: the uncertainty of the
// poses is not in it.
//
// The half-edges are grouped per landmark once (stable; a CSR of offsets), and
// each landmark's run is cut into chunks of kMapChunk counted from its own
// first half-edge.  One workgroup folds one chunk: a lane per half-edge (lanes
// past the landmark's end hold zeros), the xor tree of a wave, the four wave
// sums in order.  graph_map_finish_kernel then adds a landmark's chunk sums in
// chunk order.  Both shapes depend on the landmark's own count alone and no
// value crosses from one landmark to another, so a landmark's results are the
// same bits whatever else is in the set and wherever its half-edges stand.  No
// floating-point atomics.
#pragma once

#include "graph_kernels.inl"

namespace slam {

constexpr int kMapChunk = 256;    // W: half-edges of a fold chunk = lanes of its workgroup
constexpr int kMapTerms = 5;      // SoA rows of a half-edge: L_x, L_y, W_00, W_01, W_11
constexpr int kMapSums = 5;       // Lam_00, Lam_01, Lam_11, eta_0, eta_1

// W (L - m) of one half-edge: the product both eta and chi2 are made of
__device__ __forceinline__ void map_w_times(const double w00, const double w01, const double w11,
                                            const double dx, const double dy, double& t0,
                                            double& t1) {
    t0 = fma(w01, dy, w00 * dx);
    t1 = fma(w11, dy, w01 * dx);
}

// One lane per grouped half-edge: L_k and the three distinct entries of W_k to
// term ([kMapTerms][G]).
__global__ __launch_bounds__(256) void graph_map_contrib_kernel(
    const int64_t G, const int64_t* __restrict__ gpose, const double* __restrict__ gobs,
    const double* __restrict__ poses, const GraphConst g, double* __restrict__ term) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= G) return;
    const double* x = poses + 3 * gpose[k];
    const double d = gobs[k], dir = gobs[G + k];
    double v0, v1, ang, s, c;
    meas_var_angle(d, dir, x[2], g, v0, v1, ang);
    sincos(ang, &s, &c);
    const double i0 = 1.0 / v0, i1 = 1.0 / v1;
    // (R D) R^T as meas_cov_world forms it, with D = diag(i0, i1)
    const double rd00 = c * i0, rd01 = -s * i1, rd10 = s * i0, rd11 = c * i1;
    term[k] = fma(d, c, x[0]);
    term[G + k] = fma(d, s, x[1]);
    term[2 * G + k] = fma(rd01, -s, rd00 * c);
    term[3 * G + k] = fma(rd01, c, rd00 * s);
    term[4 * G + k] = fma(rd11, c, rd10 * s);
}

// One workgroup per chunk (clm: its landmark, cfirst: its first grouped
// half-edge).  CHI2 = false: the five sums of the chunk, eta against L_k0 read
// through the CSR, to part ([kMapSums][NC]).  CHI2 = true: chi2_k against
// mean_l, scattered to the input order (gsrc), and the chunk's sum of them to
// part ([NC]).
template <bool CHI2>
__global__ __launch_bounds__(kMapChunk) void graph_map_fold_kernel(
    const int64_t G, const int64_t NC, const int64_t* __restrict__ clm,
    const int64_t* __restrict__ cfirst, const int64_t* __restrict__ lstart,
    const double* __restrict__ term, const double* __restrict__ mean,
    const int64_t* __restrict__ gsrc, double* __restrict__ part, double* __restrict__ half_chi2) {
    constexpr int K = CHI2 ? 1 : kMapSums;
    __shared__ double sh[K * kMapChunk / 64];
    const int64_t c = blockIdx.x;
    const int64_t l = clm[c];
    const int64_t k = cfirst[c] + threadIdx.x;
    double v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = 0.0;
    if (k < lstart[l + 1]) {
        const double w00 = term[2 * G + k], w01 = term[3 * G + k], w11 = term[4 * G + k];
        double ox, oy;      // what L_k is measured from: L_k0, or the mean
        if constexpr (CHI2) {
            ox = mean[2 * l];
            oy = mean[2 * l + 1];
        } else {
            const int64_t k0 = lstart[l];
            ox = term[k0];
            oy = term[G + k0];
        }
        const double dx = term[k] - ox, dy = term[G + k] - oy;
        double t0, t1;
        map_w_times(w00, w01, w11, dx, dy, t0, t1);
        if constexpr (CHI2) {
            v[0] = fma(dy, t1, dx * t0);
            half_chi2[gsrc[k]] = v[0];
        } else {
            v[0] = w00;
            v[1] = w01;
            v[2] = w11;
            v[K - 2] = t0;
            v[K - 1] = t1;
        }
    }
    block_sumK_fixed<kMapChunk, K>(v, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < K; ++j) part[j * NC + c] = v[j];
}

// One lane per landmark: its chunk sums in chunk order (coff: the CSR of chunks
// per landmark).  CHI2 = false: cov = Lam^-1 (2x2 closed form) and mean = L_k0 +
// cov eta; CHI2 = true: chi2_l.  A landmark nobody saw gets NaN.
template <bool CHI2>
__global__ __launch_bounds__(64) void graph_map_finish_kernel(
    const int64_t NL, const int64_t G, const int64_t NC, const int64_t* __restrict__ coff,
    const int64_t* __restrict__ lstart, const double* __restrict__ part,
    const double* __restrict__ term, double* __restrict__ mean, double* __restrict__ cov,
    double* __restrict__ chi2) {
    constexpr int K = CHI2 ? 1 : kMapSums;
    const int64_t l = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (l >= NL) return;
    const int64_t c0 = coff[l], c1 = coff[l + 1];
    const double nan = __builtin_nan("");
    double a[K];
#pragma unroll
    for (int j = 0; j < K; ++j) a[j] = (c0 < c1) ? part[j * NC + c0] : nan;
    for (int64_t c = c0 + 1; c < c1; ++c)
#pragma unroll
        for (int j = 0; j < K; ++j) a[j] += part[j * NC + c];
    if constexpr (CHI2) {
        chi2[l] = a[0];
    } else {
        const double det = fma(-a[1], a[1], a[0] * a[2]);
        const double c00 = a[2] / det, c01 = -a[1] / det, c11 = a[0] / det;
        cov[4 * l] = c00;
        cov[4 * l + 1] = c01;
        cov[4 * l + 2] = c01;
        cov[4 * l + 3] = c11;
        double m0 = nan, m1 = nan;
        if (c0 < c1) {
            const int64_t k0 = lstart[l];
            double t0, t1;
            map_w_times(c00, c01, c11, a[K - 2], a[K - 1], t0, t1);
            m0 = term[k0] + t0;
            m1 = term[G + k0] + t1;
        }
        mean[2 * l] = m0;
        mean[2 * l + 1] = m1;
    }
}

}  // namespace slam
