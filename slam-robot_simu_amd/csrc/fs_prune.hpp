// fs_prune.hpp -- launch interface of the landmark evidence pass and its
// resampling gather (fs_prune.hip), used by fs_api.inl.
#pragma once

#include "common.hpp"

namespace slam {

struct FsPrune {
    double vr2, view_tan;       // view_range^2; in view iff ry >= |rx| view_tan (with the angle)
    int32_t init, hit, miss, ev_max, remove_below;
};

// fs_prune_kernel over nb blocks, then fs_prune_fold_kernel: the pass on the
// current maps, counts and evidence, and the largest count after it to
// cmax_host (a device address of the host's coherent word)
void fs_prune_launch(hipStream_t stream, bool use_angle, int32_t nb, int64_t n, int64_t npad,
                     const double* xs, const double* ys, const double* ts, double* map,
                     int32_t* cnt_io, const int32_t* cnt_before, const int32_t* stamp, int32_t call,
                     int32_t cap, const FsPrune& P, int32_t* ev, int32_t* removed, int32_t* bcnt,
                     int32_t* cmax_host);

// fs_prune_gather_kernel: the evidence rows below nrows through the resampling indices
void fs_prune_gather_launch(hipStream_t stream, dim3 grid, int64_t n, int64_t npad,
                            const int32_t* idx, int32_t nrows, const int32_t* cnt_src,
                            const int32_t* src, int32_t* dst);

}  // namespace slam
