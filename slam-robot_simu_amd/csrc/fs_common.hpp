// fs_common.hpp -- what the FastSLAM kernels of fastslam.inl and fs_prune.hip
// share: the block size, the map's row layout with its copy, and the wave and
// block maxima.
//
// Map layout: component-major per landmark,
//     map[(5 j + c) * npad + p],   c = mx, my, pxx, pxy, pyy
// so that a wave's 64 particles read and write 512 contiguous bytes per
// component in the update, and the gather -- whose source indices are
// non-decreasing in p -- reads neighbouring or equal addresses.
#pragma once

#include "common.hpp"

namespace slam {

constexpr int kFsThreads = 256;
constexpr int kFsComp = 5;

// One landmark of one particle: the mean and the covariance's upper triangle
struct FsLm {
    double mx, my, pxx, pxy, pyy;
};

// Row j of particle p: its components lie npad apart from the returned address
template <typename T>
__device__ __forceinline__ T* fs_row(T* map, const size_t j, const int64_t npad, const int64_t p) {
    return map + (size_t)kFsComp * j * (size_t)npad + (size_t)p;
}

__device__ __forceinline__ FsLm fs_lm_load(const double* m, const int64_t npad) {
    return FsLm{m[0], m[(size_t)npad], m[2 * (size_t)npad], m[3 * (size_t)npad],
                m[4 * (size_t)npad]};
}

__device__ __forceinline__ void fs_lm_store(double* m, const int64_t npad, const FsLm& v) {
    m[0] = v.mx;
    m[(size_t)npad] = v.my;
    m[2 * (size_t)npad] = v.pxx;
    m[3 * (size_t)npad] = v.pxy;
    m[4 * (size_t)npad] = v.pyy;
}

// Five loads, then five stores
__device__ __forceinline__ void fs_row_copy(const double* a, double* b, const int64_t npad) {
    fs_lm_store(b, npad, fs_lm_load(a, npad));
}

__device__ __forceinline__ double fs_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ int32_t fs_max(int32_t a, int32_t b) { return b > a ? b : a; }

template <typename T>
__device__ __forceinline__ T fs_wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fs_max(v, __shfl_xor(v, o, 64));
    return v;
}

// The maximum over a block of kFsThreads: the wave maxima to LDS, a barrier
// that every lane must reach, and thread 0 -- which alone holds the result --
// folds them.  The maximum is order-free, so it is deterministic (no
// floating-point atomics).  The LDS slots belong to the function and its
// type: a kernel calls fs_block_max once per type, or puts a barrier between
// two calls (nothing else keeps the second call's stores from thread 0's reads
// of the first).
template <typename T>
__device__ __forceinline__ void fs_wave_max_put(T* s_w, const T v) {
    const T wm = fs_wave_max(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = wm;
}

template <typename T>
__device__ __forceinline__ T fs_wave_max_fold(const T* s_w) {
    T v = s_w[0];
#pragma unroll
    for (int w = 1; w < kFsThreads / 64; ++w) v = fs_max(v, s_w[w]);
    return v;
}

template <typename T>
__device__ __forceinline__ T fs_block_max(T v) {
    __shared__ T s_v[kFsThreads / 64];
    fs_wave_max_put(s_v, v);
    __syncthreads();
    if (threadIdx.x == 0) v = fs_wave_max_fold(s_v);
    return v;
}

// Two maxima behind one barrier
template <typename T, typename U>
__device__ __forceinline__ void fs_block_max(T& v, U& u) {
    __shared__ T s_v[kFsThreads / 64];
    __shared__ U s_u[kFsThreads / 64];
    fs_wave_max_put(s_v, v);
    fs_wave_max_put(s_u, u);
    __syncthreads();
    if (threadIdx.x == 0) {
        v = fs_wave_max_fold(s_v);
        u = fs_wave_max_fold(s_u);
    }
}

}  // namespace slam
