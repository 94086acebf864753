// ekf_assoc.inl -- EKF-SLAM without ids: the kernels of an
// associating slam_ekfslam handle.  Included by ekf_api.hip after
// ekf_kernels.inl, whose update kernels the handle launches unchanged over the
// active prefix of the state.
//
//   eks_scan_kernel    l[t][j]: log-likelihood of observation t under slot j
//   eks_assign_kernel  the sequential greedy choice over the score rows
//   eks_init_kernel    state and covariance augmentation with the new landmarks
#pragma once

#include "ekf_kernels.inl"

namespace slam {

constexpr int kEksMaxObs = kEksMaxM / 3;          // 40 observations per call
constexpr int kEksScanThreads = 256;
constexpr int kEksAssignThreads = 1024;
constexpr double kLn2Pi = 1.8378770664093453;     // np.log(2 * np.pi)

struct EksScan {
    double obs[3 * kEksMaxObs];
};

// diag(scan_cov(range)) (graph_based_slam.py:187-194), eks_build_kernel's order
__device__ __forceinline__ void eks_scan_cov(const double rng, const EksConst& c, double (&R)[3]) {
    const double d = rng * c.r_dist;
    const double sd = rng * sin(c.r_dir);
    R[0] = d * d;
    R[1] = sd * sd;
    R[2] = c.r_dir * c.r_dir + c.r_orient * c.r_orient;
}

// One lane per candidate slot j < count.  What does not depend on the
// observation is formed once, in registers: the slot's mean, the 9 + 6
// covariance numbers P_jr, P_jj (P_rr is the same for every lane), the
// predicted measurement and A = [Hr Hl] P[{r,j},{r,j}] [Hr Hl]^T.  The lane
// then walks the observations (staged in LDS): S = A + R_t, its determinant and
// e^T S^-1 e through the cofactors, l[t][j] stored coalesced over j.
// P_jj and P_jr are row reads of the lower triangle (rows 3+3j..5+3j, one
// 128-byte line each for P_jr, and the three diagonal lines).
__global__ __launch_bounds__(kEksScanThreads) void eks_scan_kernel(
    const double* __restrict__ P, const int64_t ld, const double* __restrict__ mu,
    const int32_t count, const int32_t k, const EksScan ob, const EksConst c, const int64_t stride,
    double* __restrict__ scores) {
    __shared__ double so[3 * kEksMaxObs], sr[3 * kEksMaxObs];
    for (int t = threadIdx.x; t < k; t += blockDim.x) {
        double R[3];
        eks_scan_cov(ob.obs[3 * t], c, R);
        for (int a = 0; a < 3; ++a) {
            so[3 * t + a] = ob.obs[3 * t + a];
            sr[3 * t + a] = R[a];
        }
    }
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const int64_t c0 = 3 + 3 * j;
    // the 6 x 6 block over (robot, slot j), symmetric
    double B[6][6];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            B[a][b] = B[b][a] = P[a * ld + b];
            B[3 + a][3 + b] = B[3 + b][3 + a] = P[(c0 + a) * ld + c0 + b];
        }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) B[3 + a][b] = B[b][3 + a] = P[(c0 + a) * ld + b];
    const double xr = mu[0], yr = mu[1], th = mu[2];
    const double lx = mu[c0], ly = mu[c0 + 1], lp = mu[c0 + 2];
    const double psi = kHalfPi - th;
    double s, co;
    sincos(psi, &s, &co);
    const double dx = lx - xr, dy = ly - yr;
    const double rx = co * dx - s * dy;
    const double ry = s * dx + co * dy;
    const double zh[3] = {hypot(rx, ry), atan2(ry, rx), wrap_angle(psi + lp)};
    const double q = dx * dx + dy * dy;
    const double r = sqrt(q);
    const double H[3][6] = {{-dx / r, -dy / r, 0.0, dx / r, dy / r, 0.0},
                            {dy / q, -dx / q, -1.0, -dy / q, dx / q, 0.0},
                            {0.0, 0.0, -1.0, 0.0, 0.0, 1.0}};
    double T[3][6];                       // H B, columns ascending
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            double acc = H[a][0] * B[0][v];
#pragma unroll
            for (int u = 1; u < 6; ++u) acc = fma(H[a][u], B[u][v], acc);
            T[a][v] = acc;
        }
    double A[3][3];                       // T H^T, lower triangle
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
            double acc = T[a][0] * H[b][0];
#pragma unroll
            for (int u = 1; u < 6; ++u) acc = fma(T[a][u], H[b][u], acc);
            A[a][b] = acc;
        }
    for (int t = 0; t < k; ++t) {
        const double e0 = so[3 * t] - zh[0];
        const double e1 = wrap_angle(so[3 * t + 1] - zh[1]);
        const double e2 = wrap_angle(so[3 * t + 2] - zh[2]);
        const double s00 = A[0][0] + sr[3 * t], s11 = A[1][1] + sr[3 * t + 1],
                     s22 = A[2][2] + sr[3 * t + 2];
        const double s01 = A[1][0], s02 = A[2][0], s12 = A[2][1];
        const double c00 = s11 * s22 - s12 * s12;
        const double c01 = s02 * s12 - s01 * s22;
        const double c02 = s01 * s12 - s02 * s11;
        const double c11 = s00 * s22 - s02 * s02;
        const double c12 = s01 * s02 - s00 * s12;
        const double c22 = s00 * s11 - s01 * s01;
        const double det = (s00 * c00 + s01 * c01) + s02 * c02;
        const double dg = (e0 * e0 * c00 + e1 * e1 * c11) + e2 * e2 * c22;
        const double od = (e0 * e1 * c01 + e0 * e2 * c02) + e1 * e2 * c12;
        const double quad = (dg + 2.0 * od) / det;
        scores[(int64_t)t * stride + j] = -0.5 * (quad + log(det)) - 1.5 * kLn2Pi;
    }
}

// (score, slot) of the better candidate: the larger score, the lower slot on a
// tie; slot < 0 is "none" (a NaN score never becomes a candidate).
__device__ __forceinline__ void eks_better(double& l, int32_t& j, const double lo, const int32_t jo) {
    if (jo >= 0 && (j < 0 || lo > l || (lo == l && jo < j))) {
        l = lo;
        j = jo;
    }
}

// The greedy choice, observation by observation, in one workgroup: every lane
// keeps the best of its slots (j = tid, tid + 1024, ...), a 64-lane butterfly
// and one LDS round over the 16 waves give the winner, lane 0 decides and
// marks the slot taken.  res: {matched, new count, assoc[k]}.
__global__ __launch_bounds__(kEksAssignThreads) void eks_assign_kernel(
    const double* __restrict__ scores, const int64_t stride, const int32_t count0,
    const int32_t cap, const int32_t k, const double log_p_new, int32_t* __restrict__ taken,
    int32_t* __restrict__ res) {
    __shared__ double wl[kEksAssignThreads / 64];
    __shared__ int32_t wj[kEksAssignThreads / 64];
    __shared__ int32_t s_count, s_matched;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int32_t j = tid; j < count0; j += kEksAssignThreads) taken[j] = 0;
    if (tid == 0) {
        s_count = count0;
        s_matched = 0;
    }
    __syncthreads();
    for (int t = 0; t < k; ++t) {
        const double* row = scores + (int64_t)t * stride;
        double l = 0.0;
        int32_t jb = -1;
        for (int32_t j = tid; j < count0; j += kEksAssignThreads) {
            const double v = row[j];
            if (!taken[j] && v == v) eks_better(l, jb, v, j);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double lo = __shfl_xor(l, d, 64);
            const int32_t jo = __shfl_xor(jb, d, 64);
            eks_better(l, jb, lo, jo);
        }
        if (lane == 0) {
            wl[wave] = l;
            wj[wave] = jb;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kEksAssignThreads / 64; ++w) eks_better(l, jb, wl[w], wj[w]);
            int32_t a;
            if (jb < 0 || l < log_p_new) {
                if (s_count < cap) {
                    a = -1;
                    ++s_count;
                } else {
                    a = -2;
                }
            } else {
                a = jb;
                taken[jb] = 1;
                ++s_matched;
            }
            res[2 + t] = a;
        }
        __syncthreads();                  // taken[] and wl / wj before the next row
    }
    if (tid == 0) {
        res[0] = s_matched;
        res[1] = s_count;
    }
}

struct EksNew {
    int32_t n_new;
    int32_t pad0;
    double obs[3 * kEksMaxObs];           // the new observations, in observation order
};

// What initialising one landmark from (range d, bearing b, orientation o) at
// the pose (x, y, th) needs: the offset (dx, dy) of g(x, z) and psi.
struct EksInit {
    double dx, dy, d, psi, o;
};

__device__ __forceinline__ EksInit eks_init_of(const double* obs, const double th) {
    EksInit g;
    g.d = obs[0];
    g.o = obs[2];
    g.psi = kHalfPi - th;
    double s, c, sb, cb;
    sincos(g.psi, &s, &c);
    sincos(obs[1], &sb, &cb);
    const double rx = g.d * cb, ry = g.d * sb;
    g.dx = c * rx + s * ry;
    g.dy = -s * rx + c * ry;
    return g;
}

// Row a of G_r applied to the column (p0, p1, p2) of P_r,.
__device__ __forceinline__ double eks_gr_row(const EksInit& g, const int a, const double p0,
                                             const double p1, const double p2) {
    return a == 0 ? p0 - g.dy * p2 : a == 1 ? p1 + g.dx * p2 : p2;
}

// Grid: column chunks x new landmarks.  Block (cx, i) writes the three rows of
// slot s = count + i of the lower triangle: P_s,c = G_r P_r,c for c < 3 + 3 s and
// the diagonal block G_r P_rr G_r^T + G_z R G_z^T.  P_r,c of an older column is
// the posterior's first-three-columns entry P[c][0..2] (one line per row c);
// of a column created in this call it is that landmark's own G_r P_rr, formed
// again here as its block stores it (no block reads what another writes).
// Block (0, i) also writes mu_s.
__global__ __launch_bounds__(256) void eks_init_kernel(double* __restrict__ P, const int64_t ld,
                                                       double* __restrict__ mu, const int32_t count,
                                                       const EksNew nw, const EksConst c) {
    const int i = blockIdx.y;
    const int64_t s = (int64_t)count + i;
    const int64_t r0 = 3 + 3 * s;
    const int64_t n_old = 3 + 3 * (int64_t)count;
    const double x = mu[0], y = mu[1], th = mu[2];
    const EksInit g = eks_init_of(nw.obs + 3 * i, th);
    double Prr[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) Prr[a][b] = Prr[b][a] = P[a * ld + b];
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col == 0) {
        mu[r0] = x + g.dx;
        mu[r0 + 1] = y + g.dy;
        mu[r0 + 2] = wrap_angle(g.o - g.psi);
    }
    if (col >= r0 + 3) return;
    double p[3];                          // P_r,col
    if (col < 3) {
        for (int b = 0; b < 3; ++b) p[b] = Prr[b][col];
    } else if (col < n_old) {
        for (int b = 0; b < 3; ++b) p[b] = P[col * ld + b];
    } else {
        // a landmark of this call (itself included: the diagonal block)
        const int64_t i2 = (col - n_old) / 3;
        const int a2 = (int)((col - n_old) % 3);
        const EksInit g2 = eks_init_of(nw.obs + 3 * i2, th);
        for (int b = 0; b < 3; ++b) p[b] = eks_gr_row(g2, a2, Prr[0][b], Prr[1][b], Prr[2][b]);
    }
    if (col < r0) {
        for (int a = 0; a < 3; ++a) P[(r0 + a) * ld + col] = eks_gr_row(g, a, p[0], p[1], p[2]);
        return;
    }
    // diagonal block, lower triangle: rows a >= cc
    const int cc = (int)(col - r0);
    double R[3];
    eks_scan_cov(g.d, c, R);
    const double ux = g.dx / g.d, uy = g.dy / g.d;
    double Z[3][3] = {};
    Z[0][0] = ux * ux * R[0] + g.dy * g.dy * R[1];
    Z[1][0] = ux * uy * R[0] - g.dy * g.dx * R[1];
    Z[1][1] = uy * uy * R[0] + g.dx * g.dx * R[1];
    Z[2][2] = R[2];
    for (int a = cc; a < 3; ++a)
        P[(r0 + a) * ld + col] = eks_gr_row(g, a, p[0], p[1], p[2]) + Z[a][cc];
}

}  // namespace slam
