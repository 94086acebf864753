// eks_prune.hip -- gfx950 kernels of landmark evidence and the removal of
// landmarks from an associating EKF-SLAM handle (include/slam_hip.h,
// slam_ekfslam_set_pruning / slam_ekfslam_remove), with their
// launchers (eks_prune.hpp).
//
// A translation unit of its own, as fs_prune.hip is: ekf_api's code object --
// every older EKF and EKF-SLAM kernel -- stays byte for byte what it was.
//
// State layout as ekf_kernels.inl's: mu[n], P row-major with pitch ld, the
// lower triangle (column <= row) current.  Slot j holds rows 3 + 3 j .. 5 + 3 j.
//
// The compaction moves every element to an address at or below its own.  No
// workgroup reads an address that another workgroup of the same launch writes
// and none waits for another: the column pass gives a workgroup whole rows, the
// row pass gives it whole columns.
#include <cstdint>

#include "eks_prune.hpp"

namespace slam {

namespace {

enum { kEvRange = 0, kEvAngle = 1, kEvMask = 2 };

// old row (or column) of new row w; rows below r_first keep their place
__device__ __forceinline__ int64_t eks_src_row(const int32_t* __restrict__ src, const int64_t r_first,
                                               const int64_t w) {
    if (w < r_first) return w;
    const int64_t s = (w - 3) / 3;
    return 3 + 3 * (int64_t)src[s] + ((w - 3) - 3 * s);
}

// row[c] = row[src(c)] for c in [c_begin, c_end), left to right in chunks: the
// workgroup reads a chunk completely, passes the barrier, then writes it.  A
// chunk's sources lie at or beyond its own first column, so they are beyond
// everything written before it.  The source columns of the next chunk (a read
// of src) are requested while the chunk's own loads are in flight: one memory
// round trip per chunk on the critical path, not two.
__device__ __forceinline__ void eks_compact_segment(double* row, const int32_t* __restrict__ src,
                                                    const int64_t r_first, const int64_t c_begin,
                                                    const int64_t c_end) {
    int64_t sc[kEksColUnroll];                  // source column, -1 beyond the segment
#pragma unroll
    for (int u = 0; u < kEksColUnroll; ++u) {
        const int64_t c = c_begin + u * kEksColThreads + threadIdx.x;
        sc[u] = c < c_end ? eks_src_row(src, r_first, c) : -1;
    }
    for (int64_t c0 = c_begin; c0 < c_end; c0 += kEksColChunk) {
        double v[kEksColUnroll];
#pragma unroll
        for (int u = 0; u < kEksColUnroll; ++u) v[u] = sc[u] >= 0 ? row[sc[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < kEksColUnroll; ++u) {
            const int64_t c = c0 + kEksColChunk + u * kEksColThreads + threadIdx.x;
            sc[u] = c < c_end ? eks_src_row(src, r_first, c) : -1;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kEksColUnroll; ++u) {
            const int64_t c = c0 + u * kEksColThreads + threadIdx.x;
            if (c < c_end) row[c] = v[u];
        }
    }
}

}  // namespace

// One workgroup; lanes stride over the slots in chunks of kEksEvThreads.  Per
// chunk: the slot's new evidence and keep flag, a workgroup-wide exclusive scan
// of the flags (64-lane shuffle scan, the 16 wave totals through LDS), then the
// kept slot's evidence to ev[w] and its old number to src[w].  w <= j, and the
// chunk's evidence was read before the scan's barrier: in place.
template <int MODE>
__global__ __launch_bounds__(kEksEvThreads) void eks_evidence_kernel(
    const double* __restrict__ mu, const int32_t count0, const int32_t count,
    const int32_t* __restrict__ taken, const int32_t* __restrict__ mask, const EksPrune P,
    int32_t* ev, int32_t* __restrict__ src, int32_t* __restrict__ res) {
    __shared__ int32_t s_tot[2][kEksEvThreads / 64];
    __shared__ int32_t s_first;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_first = count;
    double x = 0.0, y = 0.0, s = 0.0, c = 0.0;
    if constexpr (MODE != kEvMask) {
        x = mu[0];
        y = mu[1];
        if constexpr (MODE == kEvAngle) sincos(kHalfPi - mu[2], &s, &c);
    }
    __syncthreads();
    int32_t base = 0;
    int par = 0;
    for (int32_t j0 = 0; j0 < count; j0 += kEksEvThreads, par ^= 1) {
        const int32_t j = j0 + tid;
        const bool valid = j < count;
        int64_t e = 0;
        bool keep = false;
        if (valid) {
            if constexpr (MODE == kEvMask) {
                e = ev ? ev[j] : 0;
                keep = mask[j] == 0;
            } else {
                e = ev[j];
                if (j >= count0) {
                    e = P.init;
                } else if (taken && taken[j]) {
                    e += P.hit;
                    e = e < P.ev_max ? e : P.ev_max;
                } else {
                    const double dx = mu[3 + 3 * (int64_t)j] - x, dy = mu[4 + 3 * (int64_t)j] - y;
                    bool in = dx * dx + dy * dy <= P.vr2;       // false on NaN
                    if constexpr (MODE == kEvAngle) {
                        const double rx = c * dx - s * dy, ry = s * dx + c * dy;
                        in = in && ry >= fabs(rx) * P.view_tan;
                    }
                    if (in) {
                        e -= P.miss;
                        e = e > INT32_MIN ? e : INT32_MIN;
                    }
                }
                keep = e >= P.remove_below;
            }
        }
        int32_t inc = keep ? 1 : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t u = __shfl_up(inc, d, 64);
            if (lane >= d) inc += u;
        }
        if (lane == 63) s_tot[par][wave] = inc;
        if (valid && !keep) atomicMin(&s_first, j);
        __syncthreads();
        int32_t before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kEksEvThreads / 64; ++k) {
            const int32_t t = s_tot[par][k];
            before += k < wave ? t : 0;
            total += t;
        }
        if (keep) {
            const int32_t w = base + before + inc - 1;
            if (ev) ev[w] = (int32_t)e;
            src[w] = j;
        }
        base += total;
    }
    __syncthreads();
    if (tid == 0) {
        const int32_t first = s_first < count ? s_first : -1;
        res[kEksPrCount] = base;
        res[kEksPrRemoved] = count - base;
        res[kEksPrMoved] = first >= 0 ? base - first : 0;
        res[kEksPrFirst] = first;
    }
}

// Column pass.  Block b < rows: new row w = r_first + b, still at its old place
// i = src(w); its columns [r_first, w] take the kept columns' values, in place.
// The last block does the same to mu over [r_first, n_new).
__global__ __launch_bounds__(kEksColThreads) void eks_compact_cols_kernel(
    double* P, const int64_t ld, double* mu, const int32_t* __restrict__ src, const int64_t r_first,
    const int64_t n_new) {
    const int64_t w = r_first + blockIdx.x;
    if (w == n_new) {
        eks_compact_segment(mu, src, r_first, r_first, n_new);
        return;
    }
    const int64_t i = eks_src_row(src, r_first, w);
    eks_compact_segment(P + i * ld, src, r_first, r_first, w + 1);
}

// Row pass.  A one-wave workgroup owns a strip of kEksRowStrip columns (one
// 128-byte line of a row) and walks the new rows top to bottom, 64 / strip rows
// per load instruction and kEksRowBatch of those in flight per lane before the
// first store.  Row w comes from row src(w) > w: what a batch overwrites lies
// above every row that it or a later batch still has to read.  The next batch's
// source rows are requested while the batch's loads are in flight.
__global__ __launch_bounds__(64) void eks_compact_rows_kernel(double* P, const int64_t ld,
                                                              const int32_t* __restrict__ src,
                                                              const int64_t r_first,
                                                              const int64_t n_new) {
    constexpr int kRows = 64 / kEksRowStrip;               // rows per load instruction
    const int64_t c = (int64_t)blockIdx.x * kEksRowStrip + (threadIdx.x % kEksRowStrip);
    const int rl = threadIdx.x / kEksRowStrip;
    const int64_t c_strip = (int64_t)blockIdx.x * kEksRowStrip;
    const int64_t w_begin = r_first > c_strip ? r_first : c_strip;
    int64_t sr[kEksRowBatch];                   // source row, -1 where the lane has nothing to move
#pragma unroll
    for (int b = 0; b < kEksRowBatch; ++b) {
        const int64_t w = w_begin + b * kRows + rl;
        sr[b] = (w < n_new && c <= w) ? eks_src_row(src, r_first, w) : -1;
    }
    for (int64_t w0 = w_begin; w0 < n_new; w0 += kRows * kEksRowBatch) {
        double v[kEksRowBatch];
#pragma unroll
        for (int b = 0; b < kEksRowBatch; ++b) v[b] = sr[b] >= 0 ? P[sr[b] * ld + c] : 0.0;
#pragma unroll
        for (int b = 0; b < kEksRowBatch; ++b) {
            const int64_t w = w0 + kRows * kEksRowBatch + b * kRows + rl;
            sr[b] = (w < n_new && c <= w) ? eks_src_row(src, r_first, w) : -1;
        }
#pragma unroll
        for (int b = 0; b < kEksRowBatch; ++b) {
            const int64_t w = w0 + b * kRows + rl;
            if (w < n_new && c <= w) P[w * ld + c] = v[b];
        }
    }
}

// The vacated rows [n_new, n_old) of P over the columns [0, n_old), and (last
// block) the same entries of mu, to zero.
__global__ __launch_bounds__(kEksColThreads) void eks_compact_zero_kernel(double* __restrict__ P,
                                                                          const int64_t ld,
                                                                          double* __restrict__ mu,
                                                                          const int64_t n_new,
                                                                          const int64_t n_old) {
    const int64_t i = n_new + blockIdx.x;
    if (i == n_old) {
        for (int64_t q = n_new + threadIdx.x; q < n_old; q += kEksColThreads) mu[q] = 0.0;
        return;
    }
    double* row = P + i * ld;
    for (int64_t q = threadIdx.x; q < n_old; q += kEksColThreads) row[q] = 0.0;
}

void eks_evidence_launch(hipStream_t stream, bool use_angle, const double* mu, int32_t count0,
                         int32_t count, const int32_t* taken, const EksPrune& P, int32_t* ev,
                         int32_t* src, int32_t* res) {
    if (use_angle)
        eks_evidence_kernel<kEvAngle><<<1, kEksEvThreads, 0, stream>>>(mu, count0, count, taken,
                                                                       nullptr, P, ev, src, res);
    else
        eks_evidence_kernel<kEvRange><<<1, kEksEvThreads, 0, stream>>>(mu, count0, count, taken,
                                                                       nullptr, P, ev, src, res);
}

void eks_mask_launch(hipStream_t stream, const int32_t* mask, int32_t count, int32_t* ev,
                     int32_t* src, int32_t* res) {
    eks_evidence_kernel<kEvMask><<<1, kEksEvThreads, 0, stream>>>(nullptr, count, count, nullptr,
                                                                  mask, EksPrune{}, ev, src, res);
}

void eks_compact_launch(hipStream_t stream, double* P, int64_t ld, double* mu, const int32_t* src,
                        int32_t first, int32_t count_new, int32_t count_old) {
    const int64_t r_first = 3 + 3 * (int64_t)first;
    const int64_t n_new = 3 + 3 * (int64_t)count_new, n_old = 3 + 3 * (int64_t)count_old;
    if (n_new > r_first) {
        eks_compact_cols_kernel<<<(unsigned)(n_new - r_first + 1), kEksColThreads, 0, stream>>>(
            P, ld, mu, src, r_first, n_new);
        eks_compact_rows_kernel<<<(unsigned)((n_new + kEksRowStrip - 1) / kEksRowStrip), 64, 0,
                                  stream>>>(P, ld, src, r_first, n_new);
    }
    eks_compact_zero_kernel<<<(unsigned)(n_old - n_new + 1), kEksColThreads, 0, stream>>>(
        P, ld, mu, n_new, n_old);
}

}  // namespace slam
