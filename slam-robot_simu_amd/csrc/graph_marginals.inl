// graph_marginals.inl -- kernels of slam_graph_marginals (include/slam_hip.h;
// DESIGN 8.2): selected columns of H^-1, i.e. the joint marginal covariance of
// a handful of poses.  Included by graph_api.hip after graph_kernels.inl.
//
// Dense path: one workgroup per requested column substitutes e_j through the
// LU and pivots graph_lu_kernel left, the column held in LDS.
//
// PCG path: a block of W independent block-Jacobi preconditioned CGs on
// H x_c = e_{j_c}, x_c = 0 at the start.  The vectors are unknown-major with
// the W columns contiguous (v[i][W]), so one 72-byte block of H is loaded
// once per W columns and its gather is 3 W contiguous doubles.  Workgroup
// geometry, the order of every column's fused multiply-adds and the shape of
// every fold are those of the single-column kernels and do not depend on W:
// a column's bits are the same at any width and in any company.  Each column
// has its own rho, alpha, beta, status and iteration count (MargState); a
// column whose status is final is not written any more.  Synchronisation is
// by kernel boundaries only.
#pragma once

namespace slam {

constexpr int kMargMaxCols = 8;     // widest pass instantiated (16 spills: DESIGN 8.2)

struct MargState {
    double rho[2][kMargMaxCols];    // rho_k = r_k . z_k in slot k & 1
    double rr0[kMargMaxCols], rr[kMargMaxCols];
    int32_t iter[kMargMaxCols];
    int32_t status[kMargMaxCols];   // 0 running, 1 converged, 2 curvature <= 0, 3 pcg_max_iter
    int32_t done[2];                // [k & 1]: every column was final at the SpMM launch of iteration k
};

// bit c set: column c is still running
template <int W>
__device__ __forceinline__ uint32_t marg_active(const MargState* __restrict__ st) {
    uint32_t act = 0;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (st->status[c] == 0) act |= 1u << c;
    return act;
}

// per-lane part of the fold of K = NK * W partial arrays part[(a nb + w) W + c],
// a = a0 .. a0 + NK - 1: workgroups w = lane, lane + NT, ... in ascending order
template <int NT, int W, int NK>
__device__ __forceinline__ void marg_fold_lane(const double* __restrict__ part, const int64_t nb,
                                               const int a0, double* f) {
#pragma unroll
    for (int j = 0; j < NK * W; ++j) f[j] = 0.0;
    for (int64_t w = threadIdx.x; w < nb; w += NT)
#pragma unroll
        for (int a = 0; a < NK; ++a)
#pragma unroll
            for (int c = 0; c < W; ++c) f[a * W + c] += part[((a0 + a) * nb + w) * W + c];
}

// The same folds in a launch of their own (one workgroup of NT threads, the
// totals to tot[a W + c]): the alternative to every workgroup folding the
// partials redundantly; the consumers then run with PRE = true.  Same lanes,
// same tree, same bits (SLAM_GRAPH_MARG_FOLD=1, for the A/B of DESIGN 8.2).
template <int NT, int W, int NK>
__global__ __launch_bounds__(NT) void graph_marg_fold_kernel(const int64_t nb,
                                                             const double* __restrict__ part,
                                                             const int a0,
                                                             double* __restrict__ tot) {
    __shared__ double sh[NK * W * NT / 64];
    double f[NK * W];
    marg_fold_lane<NT, W, NK>(part, nb, a0, f);
    block_sumK_fixed<NT, NK * W>(f, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < NK * W; ++j) tot[a0 * W + j] = f[j];
}

// x = 0, r = e_j, z = M^-1 r; partials r.z, r.r; the pass's state.  Column c of
// the pass is request j0 + c (unknown qidx[j0 + c]); columns past M are padding,
// final from the start.
template <int W>
__global__ __launch_bounds__(kPcgThreads) void graph_marg_start_kernel(
    const int64_t n, const double* __restrict__ minv, const int64_t* __restrict__ qidx,
    const int64_t j0, const int64_t M, double* __restrict__ x, double* __restrict__ r,
    double* __restrict__ z, double* __restrict__ part, MargState* __restrict__ st) {
    __shared__ double sh[2 * W * kPcgThreads / 64];
    __shared__ double rs[kPcgThreads * W];
    const int64_t nb = gridDim.x;
    const int64_t i = (int64_t)blockIdx.x * kPcgThreads + threadIdx.x;
    double ri[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        ri[c] = (i < n && j0 + c < M && qidx[j0 + c] == i) ? 1.0 : 0.0;
        rs[threadIdx.x * W + c] = ri[c];
    }
    __syncthreads();
    double f[2 * W];
#pragma unroll
    for (int j = 0; j < 2 * W; ++j) f[j] = 0.0;
    if (i < n) {
        const int a = (int)(i % 3);
        const double* m = minv + (i - a) * 3 + 3 * a;
        const double m0 = m[0], m1 = m[1], m2 = m[2];
        const double* rb = rs + (threadIdx.x - a) * W;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            double zi = m0 * rb[c];
            zi = fma(m1, rb[W + c], zi);
            zi = fma(m2, rb[2 * W + c], zi);
            x[i * W + c] = 0.0;
            r[i * W + c] = ri[c];
            z[i * W + c] = zi;
            f[c] = zi * ri[c];
            f[W + c] = ri[c] * ri[c];
        }
    }
    block_sumK_fixed<kPcgThreads, 2 * W>(f, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            part[(nb + blockIdx.x) * W + c] = f[c];
            part[(2 * nb + blockIdx.x) * W + c] = f[W + c];
        }
    if (pcg_lead()) {
        for (int c = 0; c < kMargMaxCols; ++c) {
            st->rho[0][c] = st->rho[1][c] = 0.0;
            st->rr0[c] = st->rr[c] = 0.0;
            st->iter[c] = 0;
            st->status[c] = (c < W && j0 + c < M) ? 0 : 1;
        }
        st->done[0] = st->done[1] = 0;
    }
}

// iteration k, first launch (graph_pcg_dir_spmv_kernel for W columns): every
// column's rho_k and convergence test from its r.z / r.r partials, then
//   p_k = z + beta p_{k-1},   q_k = H p_k = H z + beta q_{k-1}
// on the columns still running; partials p.q.  A group of 8 lanes per block
// row, each lane one whole 3x3 block at a time against the 3 W gathered
// doubles of z; 3 W accumulators per lane, folded over the group by the fixed
// xor tree.
template <int W, bool PRE>
__global__ __launch_bounds__(kSpmvThreads) void graph_marg_dir_spmm_kernel(
    const int64_t nt, const int32_t k, const int64_t* __restrict__ rptr,
    const int64_t* __restrict__ col, const double* __restrict__ val,
    const double* __restrict__ z, double* __restrict__ p, double* __restrict__ q,
    double* __restrict__ part, const double* __restrict__ tot, MargState* __restrict__ st,
    const double tol, const int32_t max_iter) {
    __shared__ double sh[2 * W * kSpmvThreads / 64];
    // the flag read here was written by an earlier launch, the one written is
    // read by later ones: no workgroup sees this launch's own decision early
    if (k > 0 && st->done[(k - 1) & 1]) {
        if (pcg_lead()) st->done[k & 1] = 1;
        return;
    }
    uint32_t act = marg_active<W>(st);
    const int64_t nb = gridDim.x;
    double f[2 * W];                 // [c] r.z, [W + c] r.r
    if (PRE) {
#pragma unroll
        for (int j = 0; j < 2 * W; ++j) f[j] = tot[W + j];
    } else {
        marg_fold_lane<kSpmvThreads, W, 2>(part, nb, 1, f);
        block_sumK_fixed<kSpmvThreads, 2 * W>(f, sh);
    }
    double beta[W];
    const uint32_t was = act;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const double rz = f[c], rr = f[W + c];
        int status = 0;
        beta[c] = 0.0;
        if (k == 0) {
            if (rr == 0.0) status = 1;
        } else {
            if (rr <= tol * tol * st->rr0[c]) status = 1;
            else if (k >= max_iter) status = 3;
            beta[c] = rz / st->rho[(k - 1) & 1][c];
        }
        if (status) act &= ~(1u << c);
        if (pcg_lead() && ((was >> c) & 1u)) {
            st->rho[k & 1][c] = rz;
            st->rr[c] = rr;
            st->iter[c] = k;
            if (k == 0) st->rr0[c] = rr;
            st->status[c] = status;
        }
    }
    if (act == 0) {
        if (pcg_lead()) st->done[k & 1] = 1;
        return;
    }
    const int g = threadIdx.x & (kSpmvGroup - 1);
    const int64_t rw = (int64_t)blockIdx.x * (kSpmvThreads / kSpmvGroup) + threadIdx.x / kSpmvGroup;
    double a0[W], a1[W], a2[W];
#pragma unroll
    for (int c = 0; c < W; ++c) a0[c] = a1[c] = a2[c] = 0.0;
    if (rw < nt) {
        const int64_t s1 = rptr[rw + 1];
        for (int64_t s = rptr[rw] + g; s < s1; s += kSpmvGroup) {
            const double* v = val + s * 9;
            double b[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) b[j] = v[j];
            const double* zc = z + 3 * col[s] * W;
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const double zj = zc[j * W + c];
                    a0[c] = fma(b[j], zj, a0[c]);
                    a1[c] = fma(b[3 + j], zj, a1[c]);
                    a2[c] = fma(b[6 + j], zj, a2[c]);
                }
        }
    }
#pragma unroll
    for (int d = 1; d < kSpmvGroup; d <<= 1)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            a0[c] += __shfl_xor(a0[c], d, 64);
            a1[c] += __shfl_xor(a1[c], d, 64);
            a2[c] += __shfl_xor(a2[c], d, 64);
        }
    double pq[W];
#pragma unroll
    for (int c = 0; c < W; ++c) pq[c] = 0.0;
    if (rw < nt && g < 3) {
        const int64_t i = (3 * rw + g) * W;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (!((act >> c) & 1u)) continue;
            const double hz = (g == 0) ? a0[c] : (g == 1) ? a1[c] : a2[c];
            const double zi = z[i + c];
            const double pi = (k > 0) ? fma(beta[c], p[i + c], zi) : zi;
            const double qi = (k > 0) ? fma(beta[c], q[i + c], hz) : hz;
            p[i + c] = pi;
            q[i + c] = qi;
            pq[c] = qi * pi;
        }
    }
    block_sumK_fixed<kSpmvThreads, W>(pq, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < W; ++c) part[blockIdx.x * W + c] = pq[c];
}

// iteration k, second launch (graph_pcg_step_kernel for W columns): per column
// alpha = rho_k / p.q (curvature gate), x += alpha p, r -= alpha q, z = M^-1 r;
// partials r.z, r.r
template <int W, bool PRE>
__global__ __launch_bounds__(kPcgThreads) void graph_marg_step_kernel(
    const int64_t n, const int32_t k, const double* __restrict__ minv,
    const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ x,
    double* __restrict__ r, double* __restrict__ z, double* __restrict__ part,
    const double* __restrict__ tot, MargState* __restrict__ st) {
    __shared__ double sh[2 * W * kPcgThreads / 64];
    __shared__ double rs[kPcgThreads * W];
    if (st->done[k & 1]) return;
    uint32_t act = marg_active<W>(st);
    const int64_t nb = gridDim.x;
    const int64_t i = (int64_t)blockIdx.x * kPcgThreads + threadIdx.x;
    double pq[W];
    if (PRE) {
#pragma unroll
        for (int c = 0; c < W; ++c) pq[c] = tot[c];
    } else {
        marg_fold_lane<kPcgThreads, W, 1>(part, nb, 0, pq);
        block_sumK_fixed<kPcgThreads, W>(pq, sh);
    }
    const uint32_t was = act;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (((was >> c) & 1u) && !(pq[c] > 0.0)) {      // not positive definite along p
            act &= ~(1u << c);
            if (pcg_lead()) st->status[c] = 2;
        }
    if (act == 0) return;            // the next SpMM launch finds every column final
    double ri[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        ri[c] = 0.0;
        if (i < n && ((act >> c) & 1u)) {
            const double alpha = st->rho[k & 1][c] / pq[c];
            const int64_t e = i * W + c;
            x[e] = fma(alpha, p[e], x[e]);
            ri[c] = fma(-alpha, q[e], r[e]);
            r[e] = ri[c];
        }
        rs[threadIdx.x * W + c] = ri[c];
    }
    __syncthreads();
    double f[2 * W];
#pragma unroll
    for (int j = 0; j < 2 * W; ++j) f[j] = 0.0;
    if (i < n) {
        const int a = (int)(i % 3);
        const double* m = minv + (i - a) * 3 + 3 * a;
        const double m0 = m[0], m1 = m[1], m2 = m[2];
        const double* rb = rs + (threadIdx.x - a) * W;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (!((act >> c) & 1u)) continue;
            double zi = m0 * rb[c];
            zi = fma(m1, rb[W + c], zi);
            zi = fma(m2, rb[2 * W + c], zi);
            z[i * W + c] = zi;
            f[c] = zi * ri[c];
            f[W + c] = ri[c] * ri[c];
        }
    }
    block_sumK_fixed<kPcgThreads, 2 * W>(f, sh);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < W; ++c) {
            part[(nb + blockIdx.x) * W + c] = f[c];
            part[(2 * nb + blockIdx.x) * W + c] = f[W + c];
        }
}

// the M requested rows of the pass's columns into cov (M x M row-major):
// cov[j][j0 + c] = x_c[qidx[j]]
__global__ __launch_bounds__(256) void graph_marg_extract_kernel(
    const int64_t M, const int W, const int64_t j0, const int64_t* __restrict__ qidx,
    const double* __restrict__ x, double* __restrict__ cov) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * W) return;
    const int64_t j = t / W;
    const int c = (int)(t - j * W);
    if (j0 + c < M) cov[j * M + j0 + c] = x[qidx[j] * W + c];
}

// Dense path: column qidx[blockIdx.x] of (LU)^-1 by getrs on e_j, the column in
// LDS; only the M requested rows leave the workgroup.  The permuted e_j is zero
// above the row the pivots carried its 1 to, so the forward substitution
// starts there.
constexpr int kMargDenseThreads = 256;
__global__ __launch_bounds__(kMargDenseThreads) void graph_marg_lu_cols_kernel(
    const double* __restrict__ LU, const int n, const int32_t* __restrict__ piv,
    const int64_t* __restrict__ qidx, const int64_t M, double* __restrict__ cov) {
    __shared__ double x[kGraphDenseMax];
    __shared__ int s_k0;
    const int tid = threadIdx.x;
    const int64_t jc = blockIdx.x;
    const int j = (int)qidx[jc];
    for (int i = tid; i < n; i += kMargDenseThreads) x[i] = (i == j) ? 1.0 : 0.0;
    __syncthreads();
    if (tid == 0) {
        int pos = j;
        for (int k = 0; k < n; ++k) {
            const int pk = piv[k];
            if (pk != k) {
                const double t = x[k];
                x[k] = x[pk];
                x[pk] = t;
                if (pos == k) pos = pk;
                else if (pos == pk) pos = k;
            }
        }
        s_k0 = pos;
    }
    __syncthreads();
    for (int k = s_k0; k < n; ++k) {       // unit lower
        const double xk = x[k];
        for (int i = k + 1 + tid; i < n; i += kMargDenseThreads)
            x[i] = fma(-xk, LU[(int64_t)i * n + k], x[i]);
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {     // upper
        if (tid == 0) x[k] /= LU[(int64_t)k * n + k];
        __syncthreads();
        const double xk = x[k];
        for (int i = tid; i < k; i += kMargDenseThreads)
            x[i] = fma(-xk, LU[(int64_t)i * n + k], x[i]);
        __syncthreads();
    }
    for (int64_t jr = tid; jr < M; jr += kMargDenseThreads) cov[jr * M + jc] = x[qidx[jr]];
}

}  // namespace slam
