// fs_prune.hip -- gfx950 kernels of landmark evidence and the removal of
// unsupported landmarks on an associating FastSLAM handle (include/slam_hip.h,
// slam_fs_set_pruning), with their launchers (fs_prune.hpp).
//
// A translation unit of its own, not a part of fastslam.inl: a change here
// leaves pf_api's code object -- the particle filter's and the other FastSLAM
// kernels -- byte for byte what it was, placement included (time
// bars).  What the two share is fs_common.hpp.
//
// Map layout: fs_common.hpp; the evidence and the match stamps are rows
// [cap][npad] of int32.
#include <cstdint>

#include "fs_common.hpp"
#include "fs_prune.hpp"

namespace slam {

// One lane per particle; the wave walks the slots below its largest count.
// Every lane loads the row's mx, my, stamp and evidence (coalesced rows, lanes
// at or above their own count masked); cnt0 is the count before the update (a
// copy taken ahead of it), call the update's number (-1: nothing was matched).
// A kept slot goes to the lane's write index w: its evidence always, its five
// map components only where w < j -- the three covariance components are
// loaded on those lanes alone.  Writes the counts, removed and the block maxima
// of the new counts.  Padding lanes hold nothing and store nothing.
template <bool ANGLE>
__global__ __launch_bounds__(kFsThreads) void fs_prune_kernel(
    const int64_t n, const int64_t npad, const double* __restrict__ xs,
    const double* __restrict__ ys, const double* __restrict__ ts, double* __restrict__ map,
    int32_t* __restrict__ cnt_io, const int32_t* __restrict__ cnt_before,
    const int32_t* __restrict__ stamp, const int32_t call, const int32_t cap, const FsPrune P,
    int32_t* __restrict__ ev, int32_t* __restrict__ removed, int32_t* __restrict__ bcnt) {
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    const bool valid = p < n;
    const int64_t pc = valid ? p : n - 1;
    const double x = xs[pc], y = ys[pc];
    double s = 0.0, c = 0.0;
    if constexpr (ANGLE) sincos(kHalfPi - ts[pc], &s, &c);
    int32_t cnt = valid ? cnt_io[p] : 0;
    cnt = cnt < cap ? cnt : cap;
    const int32_t cnt0 = cnt_before[pc];
    const int32_t jmax = __builtin_amdgcn_readfirstlane(fs_wave_max(cnt));
    int32_t w = 0;
    for (int32_t j = 0; j < jmax; ++j) {
        const size_t erow = (size_t)j * (size_t)npad + (size_t)pc;
        const double* m = fs_row(map, j, npad, pc);
        const double mx = m[0], my = m[(size_t)npad];
        const int32_t st = stamp[erow];
        int64_t e = ev[erow];
        if (j >= cnt0) {
            e = P.init;
        } else if (st == call) {
            e += P.hit;
            e = e < P.ev_max ? e : P.ev_max;
        } else {
            const double dx = mx - x, dy = my - y;
            bool in = dx * dx + dy * dy <= P.vr2;       // false on NaN
            if constexpr (ANGLE) {
                const double rx = c * dx - s * dy, ry = s * dx + c * dy;
                in = in && ry >= fabs(rx) * P.view_tan;
            }
            if (in) {
                e -= P.miss;
                e = e > INT32_MIN ? e : INT32_MIN;
            }
        }
        if (j < cnt && e >= P.remove_below) {
            const size_t wrow = (size_t)w * (size_t)npad + (size_t)pc;
            ev[wrow] = (int32_t)e;
            if (w < j) {
                fs_row_copy(m, fs_row(map, w, npad, pc), npad);
            }
            ++w;
        }
    }
    if (valid) {
        cnt_io[p] = w;
        removed[p] = cnt - w;
    }
    const int32_t bc = fs_block_max(w);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = bc;
}

// fs_assoc_fold_kernel's count half alone: the largest count after the pass
// goes to the host's coherent word
__global__ __launch_bounds__(kFsThreads) void fs_prune_fold_kernel(
    const int32_t* __restrict__ bcnt, const int32_t nb, int32_t* __restrict__ cmax_host) {
    int32_t u = 0;
    for (int32_t b = threadIdx.x; b < nb; b += kFsThreads) u = bcnt[b] > u ? bcnt[b] : u;
    u = fs_block_max(u);
    if (threadIdx.x == 0) *cmax_host = u;
}

// The evidence rows through the resampling indices, beside
// fs_assoc_gather_kernel: particle p takes the rows of its source below the
// source's own count (cnt_src: the counts before the gather).
__global__ __launch_bounds__(kFsThreads) void fs_prune_gather_kernel(
    const int64_t n, const int64_t npad, const int32_t* __restrict__ idx, const int32_t nrows,
    const int32_t* __restrict__ cnt_src, const int32_t* __restrict__ src,
    int32_t* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * kFsThreads + threadIdx.x;
    if (p >= n) return;
    const int64_t q = idx[p];
    const int32_t cq = cnt_src[q];
    const int32_t lim = cq < nrows ? cq : nrows;
    for (int32_t j = blockIdx.y; j < lim; j += gridDim.y)
        dst[(size_t)j * (size_t)npad + (size_t)p] = src[(size_t)j * (size_t)npad + (size_t)q];
}

void fs_prune_launch(hipStream_t stream, bool use_angle, int32_t nb, int64_t n, int64_t npad,
                     const double* xs, const double* ys, const double* ts, double* map,
                     int32_t* cnt_io, const int32_t* cnt_before, const int32_t* stamp, int32_t call,
                     int32_t cap, const FsPrune& P, int32_t* ev, int32_t* removed, int32_t* bcnt,
                     int32_t* cmax_host) {
    if (use_angle)
        fs_prune_kernel<true><<<nb, kFsThreads, 0, stream>>>(
            n, npad, xs, ys, ts, map, cnt_io, cnt_before, stamp, call, cap, P, ev, removed, bcnt);
    else
        fs_prune_kernel<false><<<nb, kFsThreads, 0, stream>>>(
            n, npad, xs, ys, ts, map, cnt_io, cnt_before, stamp, call, cap, P, ev, removed, bcnt);
    fs_prune_fold_kernel<<<1, kFsThreads, 0, stream>>>(bcnt, nb, cmax_host);
}

void fs_prune_gather_launch(hipStream_t stream, dim3 grid, int64_t n, int64_t npad,
                            const int32_t* idx, int32_t nrows, const int32_t* cnt_src,
                            const int32_t* src, int32_t* dst) {
    fs_prune_gather_kernel<<<grid, kFsThreads, 0, stream>>>(n, npad, idx, nrows, cnt_src, src,
                                                                 dst);
}

}  // namespace slam
