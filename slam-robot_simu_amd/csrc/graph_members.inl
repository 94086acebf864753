// graph_members.inl -- a handle whose poses are split into members: disjoint
// contiguous ranges, each a graph of its own (slam_graph_set_members; DESIGN
// 8.6).  The union's H is block diagonal by member, so the structure build and
// the per-edge / per-slot / per-row arithmetic of graph_kernels.inl run on the
// union unchanged; the kernels here are the member-aware launches of those
// bodies (a lane returns when its member is not active) and the dense kernels
// with one workgroup per member on the member's own n_m x n_m buffers.  Every
// body is the device function the plain kernel calls, so member m has the bits
// of a stand-alone handle holding member m alone.
#pragma once

#include "graph_kernels.inl"

namespace slam {

// One member: its block rows in the union (the distinct times of its edges are
// contiguous ranks, since its poses are a contiguous range) and where its dense
// buffers start.  n = 0: never solved (no edge, or 3 rows <= 3).
struct GraphMember {
    int64_t row0;      // first block row
    int64_t a_off;     // A, LU, S: n x n each
    int64_t v_off;     // V: n (n + 1)
    int64_t l_off;     // lan: 3 n + 8
    int64_t p_off;     // piv: max(n, 1)
    int32_t rows;      // block rows
    int32_t n;         // unknowns of its dense system
};

constexpr int kMemberOut = 5;         // per member: LU sign, log|det|, zero pivot; Lanczos max, min
constexpr int kMemberSplit = 4;       // workgroups per member of the element-wise dense kernels
constexpr int kMemberParts = (kGraphDenseMax / 3 + 255) / 256;   // partials of 256 poses

// member index of every BSR slot from its block row's
__global__ __launch_bounds__(256) void graph_member_slot_kernel(const int64_t n_slots,
                                                                const int64_t* __restrict__ srow,
                                                                const int32_t* __restrict__ mrow,
                                                                int32_t* __restrict__ mslot) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_slots) mslot[s] = mrow[srow[s]];
}

// ---- linearise: one lane per edge, as graph_linearize_kernel / _odom_kernel
template <int KIND>
__global__ __launch_bounds__(256) void graph_member_linearize_kernel(
    const int64_t n_lm, const int64_t E, const slam_graph_edge* __restrict__ edges,
    const double* __restrict__ poses, const GraphConst g, double* __restrict__ blocks,
    const double param, double* __restrict__ rows, const int32_t* __restrict__ medge,
    const int32_t* __restrict__ active) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_lm || !active[medge[e]]) return;
    linearize_edge<KIND>(e, E, edges, poses, g, blocks, param, rows);
}

__global__ __launch_bounds__(256) void graph_member_linearize_odom_kernel(
    const int64_t n_lm, const int64_t E, const slam_graph_edge* __restrict__ edges,
    const double* __restrict__ poses, double* __restrict__ blocks, double* __restrict__ rows,
    const int32_t* __restrict__ medge, const int32_t* __restrict__ active) {
    const int64_t e = n_lm + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || !active[medge[e]]) return;
    linearize_odom_edge(e, E, edges, poses, blocks, rows);
}

// ---- assemble: the anchor goes on the diagonal slot of the member's first row
__global__ __launch_bounds__(256) void graph_member_assemble_h_kernel(
    const int64_t n_slots, const int64_t E, const int64_t* __restrict__ cptr,
    const int64_t* __restrict__ clist, const double* __restrict__ blocks, const double anchor,
    double* __restrict__ val, const int32_t* __restrict__ mslot,
    const GraphMember* __restrict__ mem, const int64_t* __restrict__ dslot,
    const int32_t* __restrict__ active) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_slots * 9) return;
    const int64_t s = t / 9;
    const int q = (int)(t - s * 9);
    const int32_t m = mslot[s];
    if (!active[m]) return;
    const bool anchored = (s == dslot[mem[m].row0]) && diag_entry(q);
    val[t] = assemble_h_entry(s, q, anchored ? anchor : 0.0, E, cptr, clist, blocks);
}

__global__ __launch_bounds__(256) void graph_member_assemble_b_kernel(
    const int64_t n_rows, const int64_t E, const int64_t* __restrict__ bptr,
    const int64_t* __restrict__ blist, const double* __restrict__ blocks, double* __restrict__ b,
    const int32_t* __restrict__ mrow, const int32_t* __restrict__ active) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows * 3) return;
    const int64_t r = t / 3;
    if (!active[mrow[r]]) return;
    b[t] = assemble_b_entry(r, (int)(t - r * 3), E, bptr, blist, blocks);
}

// ---- BSR -> the members' dense matrices
// A_m = 0 for every active member (grid: members x kMemberSplit)
__global__ __launch_bounds__(kGraphThreads) void graph_member_zero_kernel(
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active, double* __restrict__ A) {
    const int m = blockIdx.x;
    if (!active[m]) return;
    const GraphMember gm = mem[m];
    double* a = A + gm.a_off;
    const int64_t nn = (int64_t)gm.n * gm.n;
    for (int64_t t = (int64_t)blockIdx.y * kGraphThreads + threadIdx.x; t < nn;
         t += (int64_t)gridDim.y * kGraphThreads)
        a[t] = 0.0;
}

// one lane per (slot, entry): row and column relative to the member's first row
__global__ __launch_bounds__(256) void graph_member_scatter_kernel(
    const int64_t n_slots, const int64_t* __restrict__ srow, const int64_t* __restrict__ scol,
    const double* __restrict__ val, const int32_t* __restrict__ mslot,
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active, double* __restrict__ A) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_slots * 9) return;
    const int64_t s = t / 9;
    const int q = (int)(t - s * 9);
    const int32_t m = mslot[s];
    if (!active[m]) return;
    const GraphMember gm = mem[m];
    const int64_t r = srow[s] - gm.row0, c = scol[s] - gm.row0;
    A[gm.a_off + (3 * r + q / 3) * gm.n + 3 * c + q % 3] = val[t];
}

// S_m = (A_m + A_m^T) / 2 and the copy LU_m = A_m the factorisation overwrites
__global__ __launch_bounds__(kGraphThreads) void graph_member_symmetrize_kernel(
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active,
    const double* __restrict__ A, double* __restrict__ S, double* __restrict__ LU) {
    const int m = blockIdx.x;
    if (!active[m]) return;
    const GraphMember gm = mem[m];
    const double* a = A + gm.a_off;
    const int64_t nn = (int64_t)gm.n * gm.n;
    for (int64_t t = (int64_t)blockIdx.y * kGraphThreads + threadIdx.x; t < nn;
         t += (int64_t)gridDim.y * kGraphThreads) {
        S[gm.a_off + t] = symmetrize_entry(a, gm.n, t);
        LU[gm.a_off + t] = a[t];
    }
}

// ---- the dense kernels, one workgroup per member
__global__ __launch_bounds__(kGraphThreads) void graph_member_lu_kernel(
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active, double* __restrict__ LU,
    int32_t* __restrict__ piv, double* __restrict__ out) {
    const int m = blockIdx.x;
    if (!active[m]) return;
    const GraphMember gm = mem[m];
    graph_lu_body(LU + gm.a_off, gm.n, piv + gm.p_off, out + (int64_t)kMemberOut * m);
}

__global__ __launch_bounds__(kGraphThreads) void graph_member_lanczos_kernel(
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active,
    const double* __restrict__ S, double* __restrict__ V, double* __restrict__ lan,
    double* __restrict__ out, const uint64_t seed) {
    const int m = blockIdx.x;
    if (!active[m]) return;
    const GraphMember gm = mem[m];
    double* l = lan + gm.l_off;
    graph_lanczos_body(S + gm.a_off, gm.n, V + gm.v_off, l, l + gm.n, l + 2 * gm.n,
                       out + (int64_t)kMemberOut * m + 3, seed);
}

// pass: the host's gate on the member's det and cond
__global__ __launch_bounds__(kGraphThreads) void graph_member_lu_solve_kernel(
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active,
    const int32_t* __restrict__ pass, const double* __restrict__ LU, const int32_t* __restrict__ piv,
    const double* __restrict__ b, double* __restrict__ delta) {
    const int m = blockIdx.x;
    if (!active[m] || !pass[m]) return;
    const GraphMember gm = mem[m];
    graph_lu_solve_body(LU + gm.a_off, gm.n, piv + gm.p_off, b + 3 * gm.row0, delta + 3 * gm.row0);
}

// ---- pose update and sum delta^2 of a member in the stand-alone order: partials
// over 256 poses counted from the member's first row (graph_pose_update_kernel's
// block_sum_fixed<256>: the lanes past 255 add zeros to waves the sum does not
// read), then graph_dsum_kernel's fold over the 1024 lanes.
__global__ __launch_bounds__(1024) void graph_member_pose_update_kernel(
    const GraphMember* __restrict__ mem, const int32_t* __restrict__ active,
    const int32_t* __restrict__ pass, const int64_t* __restrict__ times,
    const double* __restrict__ delta, double* __restrict__ poses, double* __restrict__ dsum) {
    __shared__ double sh[16];
    __shared__ double part[kMemberParts];
    const int m = blockIdx.x;
    if (!active[m] || !pass[m]) return;
    const GraphMember gm = mem[m];
    const int nparts = (gm.rows + 255) / 256;
    for (int k = 0; k < nparts; ++k) {
        const int i = k * 256 + (int)threadIdx.x;
        double s = 0.0;
        if (threadIdx.x < 256 && i < gm.rows) s = pose_update_row(gm.row0 + i, times, delta, poses);
        s = block_sum_fixed<256>(s, sh);
        if (threadIdx.x == 0) part[k] = s;
    }
    __syncthreads();
    const double s = dsum_fold(nparts, part, sh);
    if (threadIdx.x == 0) dsum[m] = s;
}

}  // namespace slam
