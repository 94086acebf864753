// pf_kernels.inl -- gfx950 kernels of the particle-filter step (included by pf_api.hip).
// The device helpers they share with the ensemble kernel are in pf_device.inl.
#include "pf_device.inl"

namespace slam {


// The fused step kernel: [resample gather +] predict + likelihood + weight,
// for single-GPU handles and shards alike.  The particle arrays are padded to
// whole blocks and a handle's first particle has an even global index: lane t
// of block b holds the consecutive particles b kPartPer + kDeferPPT t + k --
// 16-byte loads and stores, one device-RNG pair per particle pair.  The
// previous weights are w_un / s (deferred normalisation: w_un is read and
// rewritten in place), and the block epilogue leaves the partials the step
// end reduces, so that no pass over the particles normalises.
// Four waves per SIMD (<= 128 VGPRs): the log-sum kernel's slow-path product
// would otherwise push it to 129 and three waves.
#ifndef SLAM_FUSED_WPE
#define SLAM_FUSED_WPE 4
#endif
#if SLAM_FUSED_WPE > 0
#define SLAM_FUSED_ATTR __attribute__((amdgpu_waves_per_eu(SLAM_FUSED_WPE)))
#else
#define SLAM_FUSED_ATTR
#endif
// The fused kernel's argument segment, member for member SLAM_FUSED_PARAMS
// (every member is 8-byte aligned and a multiple of 8 bytes long, so the
// struct's layout is the segment's).  What the kernel needs only behind the
// RNG and the likelihood -- the output pointers, flags, n, refp, the block
// partials' slab -- it reads from here at that point (kernarg_view), and the
// likelihood its constants, so that no scalar register holds them from the
// kernel's start.
struct FusedArgs {
    int64_t n;
    const double *xs, *ys, *ts;
    double *xo, *yo, *to, *w_un;
    const double* c;
    int32_t* flags;
    const double *noise, *lm;
    StepIO io;
    PredictConst pc;
    LikConst lc;
    uint64_t seed;
    const double *s_in, *refp;
    DeferParts dp;
};
static_assert(sizeof(StepIO) % 8 == 0 && sizeof(PredictConst) % 8 == 0 && sizeof(LikConst) % 8 == 0 &&
                  sizeof(DeferParts) % 8 == 0 && alignof(FusedArgs) == 8,
              "FusedArgs is the argument segment's layout");

// One fused block's tile (blk: 256 lanes x P particles): the body of
// pf_fused_kernel (a persistent grid walking tiles measured slower: DESIGN 4.4).
// Returns the lane's first new weight (what follows the tile anchors its own
// kernarg_view on it).
template <int MOTION, int LIK, bool HOSTNOISE, bool WT>
__device__ __forceinline__ double pf_fused_tile(
    const int64_t blk, const int32_t st, const uint32_t rstep, const int32_t rflag,
    const double* __restrict__ zs, const int wave_s, const RngTabs& rtab,
    const int64_t n, const double* __restrict__ xs, const double* __restrict__ ys,
    const double* __restrict__ ts, double* __restrict__ xo, double* __restrict__ yo,
    double* __restrict__ to, double* __restrict__ w_un,
    const double* __restrict__ c, int32_t* __restrict__ flags, const double* __restrict__ noise,
    const double* __restrict__ lm, const StepIO& io, const PredictConst& pc, const LikConst& lc,
    const uint64_t seed, const double* __restrict__ s_in, const double* __restrict__ refp,
    const DeferParts& dp) {
    constexpr int P = kDeferPPT;
    // the pair stores: write-through (WT: st_wt_pair), so
    // that the launch leaves none of its 32 B per particle dirty in L2 for the
    // kernel's end to write back, or plain.  A template flag and not a branch:
    // the compiler takes the asm store for a write to any address and turns
    // the wave-uniform loads behind it into per-lane ones, which the large
    // handles' launches pay for without gaining.
    auto st_pair = [](double* p, const double a, const double b) {
        if constexpr (WT) st_wt_pair(p, a, b);
        else *reinterpret_cast<double2*>(p) = double2{a, b};
    };
    const int64_t base = blk * (256 * P);
    const int64_t i0 = base + P * (int64_t)threadIdx.x;
    bool valid[P];
    int64_t idx[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        valid[k] = i0 + k < n;
        idx[k] = valid[k] ? i0 + k : n - 1;
    }

    // ---- every load of the lane first (the previous weights and, without a
    //      resample gather, the particle pair), so that their latency runs
    //      under the device RNG below; the weights are consumed at the end
    double wprev[P];
    double lx[P], ly[P], lt[P];
#pragma unroll
    for (int h = 0; h < P; h += 2) {
        const double2 wu = *reinterpret_cast<const double2*>(w_un + i0 + h);
        wprev[h] = wu.x;
        wprev[h + 1] = wu.y;
    }
    if (rflag != 1) {
#pragma unroll
        for (int h = 0; h < P; h += 2) {
            const double2 a = *reinterpret_cast<const double2*>(xs + i0 + h);
            const double2 b = *reinterpret_cast<const double2*>(ys + i0 + h);
            const double2 c2 = *reinterpret_cast<const double2*>(ts + i0 + h);
            lx[h] = a.x;
            lx[h + 1] = a.y;
            ly[h] = b.x;
            ly[h + 1] = b.y;
            lt[h] = c2.x;
            lt[h + 1] = c2.y;
        }
    }
    // host / pre-drawn noise of the lane's particles (particle-major [n][3]):
    // three 16-byte loads per pair, issued with the others; the ragged last
    // block's lanes past n read particle n - 1's (idx[])
    double gn[P][3];
    if (HOSTNOISE && MOTION != kMotionNone) {
        if (i0 + P <= n) {
#pragma unroll
            for (int h = 0; h < P; h += 2) {
                const double2* q2 = reinterpret_cast<const double2*>(noise + 3 * (i0 + h));
                const double2 a = q2[0], b = q2[1], c3 = q2[2];
                gn[h][0] = a.x;
                gn[h][1] = a.y;
                gn[h][2] = b.x;
                gn[h + 1][0] = b.y;
                gn[h + 1][1] = c3.x;
                gn[h + 1][2] = c3.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < P; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) gn[k][j] = noise[3 * idx[k] + j];
        }
    }

    // ---- source particles: the resample gather (rflag 1: search the exact
    //      cumsum here; 2: already gathered) or the particles themselves
    double x[P], y[P], th[P];
    if (rflag == 1 && !flags[kFlagFallback]) {
        // the expand pass's inverse map: run starts in mark[], the block's
        // first source in carry[]; a running max over the block's positions
        __shared__ int32_t s_wmax[4];
        const uint32_t mgen = (uint32_t)flags[kFlagMarkGen];
        int32_t r[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const int64_t mk = valid[k] ? dp.mark[i0 + k] : -1;
            r[k] = ((uint64_t)mk >> 32) == mgen ? (int32_t)mk : -1;
            if (k > 0) r[k] = r[k] > r[k - 1] ? r[k] : r[k - 1];
        }
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int32_t before;
        const int32_t v = wave_max_scan_i32(r[P - 1], before);
        if (lane == 63) s_wmax[wave] = v;
        __syncthreads();
        int32_t run = dp.carry[blk];
        for (int w = 0; w < wave; ++w) run = s_wmax[w] > run ? s_wmax[w] : run;
        run = before > run ? before : run;
        const double* gx = xs - dp.goff;                         // the gather base
        const double* gy = ys - dp.goff;
        const double* gt = ts - dp.goff;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            int64_t src = r[k] > run ? r[k] : run;
            if (src >= dp.glim) {
                src = dp.goff + n - 1;                           // IndexError in the reference
                if (valid[k]) atomicOr(&flags[kFlagStatus], 1);
            }
            src = src < 0 ? 0 : src;
            x[k] = gx[src];
            y[k] = gy[src];
            th[k] = gt[src];
        }
    } else if (rflag == 1) {
        // bracket: the sources of the block's first and last positions (two
        // lanes of different waves search the whole cumsum); every lane then
        // searches only between them (the index map is monotone), a few
        // probes when the weight is concentrated -- which it is whenever
        // ESS < NP/100 triggered the resample
        __shared__ int64_t s_br[2];
        const double ofs = resample_offset(io.ofs[st], pc.np_recip, seed, rstep);
        const int64_t ilast = (base + 256 * P < n ? base + 256 * P : n) - 1;
        if (threadIdx.x == 0) s_br[0] = search_c(c, 0, n, (double)base * pc.rstep + ofs);
        if (threadIdx.x == 64 || (blockDim.x <= 64 && threadIdx.x == 0))
            s_br[1] = search_c(c, 0, n, (double)ilast * pc.rstep + ofs);
        __syncthreads();
        int64_t lo = s_br[0];
        const int64_t hi = s_br[1] < n ? s_br[1] + 1 : n;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            int64_t src = search_c(c, lo, hi, (double)idx[k] * pc.rstep + ofs);   // arange value + ofs
            lo = src;
            if (src >= n) {
                src = n - 1;                                     // IndexError in the reference
                if (valid[k]) atomicOr(&flags[kFlagStatus], 1);
            }
            x[k] = xs[src];
            y[k] = ys[src];
            th[k] = ts[src];
        }
    } else {
#pragma unroll
        for (int k = 0; k < P; ++k) {
            x[k] = lx[k];
            y[k] = ly[k];
            th[k] = lt[k];
        }
    }

    // ---- standard normals of the motion noise
    double g[P][3];
    if (MOTION == kMotionNone) {
#pragma unroll
        for (int k = 0; k < P; ++k) g[k][0] = g[k][1] = g[k][2] = 0.0;
    } else if (HOSTNOISE) {
#pragma unroll
        for (int k = 0; k < P; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) g[k][j] = gn[k][j];
    } else {
        const uint64_t gi = (uint64_t)(pc.gbase + i0);
        double h[6];
#pragma unroll
        for (int pr = 0; pr < P / 2; ++pr) {                  // gi even: whole pairs
#ifdef SLAM_PROBE_NO_RNG                                      // instruction-count probe only
            for (int j = 0; j < 6; ++j) h[j] = 0.0;
#else
            pair_normals((gi >> 1) + pr, rstep, seed, rtab, h);
#endif
#pragma unroll
            for (int j = 0; j < 6; ++j) g[2 * pr + j / 3][j % 3] = h[j];
        }
        if (MOTION == SLAM_MOTION_LINEAR) {                   // noise_j = sum_k g_k q[k][j]
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const double h0 = g[k][0], h1 = g[k][1], h2 = g[k][2];
                g[k][0] = h0 * pc.q[0] + h1 * pc.q[3] + h2 * pc.q[6];
                g[k][1] = h0 * pc.q[1] + h1 * pc.q[4] + h2 * pc.q[7];
                g[k][2] = h0 * pc.q[2] + h1 * pc.q[5] + h2 * pc.q[8];
            }
        }
    }

    FPROBE(2, g[P - 1][2]);
    // ---- predict (control of this step: particle_filter.py:46-58 / motion_model.py:40-45)
    const double v = io.ctl[2 * st], om = io.ctl[2 * st + 1];
    double xv[P], yv[P], tv[P], sp[P], cp[P];
#pragma unroll
    for (int k = 0; k < P; ++k)
        predict_particle<MOTION>(x[k], y[k], th[k], v, om, g[k][0], g[k][1], g[k][2], pc, xv[k],
                                 yv[k], tv[k], sp[k], cp[k], rtab);
    // padded arrays: the pair is stored whole.  The log-sum kernel's
    // write-through stores wait for the likelihood (kLate): behind an asm store
    // the compiler re-reads the closed form's wave-uniform words with vector
    // loads, and the wait for those is a wait for the stores before them (one
    // in-order counter) -- the drain this path is meant to avoid
    constexpr bool kLate = WT && LIK != SLAM_LIK_PRODUCT;
    if constexpr (!kLate) {
#pragma unroll
        for (int h = 0; h < P; h += 2) {
            st_pair(xo + i0 + h, xv[h], xv[h + 1]);
            st_pair(yo + i0 + h, yv[h], yv[h + 1]);
            st_pair(to + i0 + h, tv[h], tv[h + 1]);
        }
    }

    FPROBE(3, xv[P - 1] + sp[P - 1]);
    // previous weights: particle_filter.py:222 (a resampled step starts from
    // 1/NP) / :235-236 (w_un / s, NaN -> 1/NP)
    double pw[P];
    const double s_prev = *s_in;
#pragma unroll
    for (int k = 0; k < P; ++k)
        pw[k] = rflag ? pc.np_recip : norm_w(wprev[k], s_prev, pc.np_recip);
    // ---- likelihood and weight (particle_filter.py:170-198)
    double bn[P];
#ifdef SLAM_PROBE_NO_LIK                                   // timing probe only: not exact
#pragma unroll
    for (int k = 0; k < P; ++k) bn[k] = exp_lean(-1e-3 * (xv[k] + yv[k] + sp[k] + cp[k]));
    const int lane_dd = 0;
#else
    int lane_dd;
    if constexpr (LIK == SLAM_LIK_PRODUCT) {
        lane_dd = likelihood_lanes<LIK, P>(xv, yv, sp, cp, lm, zs, io.zc + (size_t)st * kZcWords,
                                           lc, bn, wave_s, pw);
    } else {
        // the likelihood's constants from the argument segment, word by word
        // where the closed form uses them.  (The pointers it loads through
        // stay the kernel's own parameters: a pointer read from the segment
        // is not known to be unaliased, and the loads through it would be
        // per-lane ones.)
        const SLAM_KARG FusedArgs* km = kernarg_view<FusedArgs>(xv[0]);
        lane_dd = likelihood_lanes<LIK, P>(xv, yv, sp, cp, lm, zs, io.zc + (size_t)st * kZcWords,
                                           km->lc, bn, wave_s, pw);
    }
#endif
    FPROBE(4, bn[P - 1]);
    // ---- the step's outputs.  Everything from here on takes its arguments
    //      from the argument segment (ka) and forms the block's base and the
    //      lanes' validity again (b2: the block index, which is blk, behind an
    //      empty asm, or the compiler keeps the values of the kernel's start),
    //      so that none of them is held across the RNG and the likelihood
    const SLAM_KARG FusedArgs* ka = kernarg_view<FusedArgs>(bn[0]);
    int32_t* const flags_l = ka->flags;
    if (__ballot(lane_dd) != 0 && __lane_id() == 0) atomicAdd(&flags_l[kFlagDDWaves], 1);
    uint32_t b2 = blockIdx.x;
    asm("" : "+s"(b2) : "v"(bn[0]));
    const int64_t n_l = ka->n;
    const int64_t base_l = (int64_t)b2 * (256 * P);
    const int64_t i0_l = base_l + P * (((int64_t)wave_s << 6) | (int64_t)__lane_id());
    double wv[P];
#pragma unroll
    for (int k = 0; k < P; ++k) wv[k] = i0_l + k < n_l ? pw[k] * bn[k] : 0.0;   // particle_filter.py:194
    if constexpr (kLate) {
        double* const xo_l = ka->xo;
        double* const yo_l = ka->yo;
        double* const to_l = ka->to;
#pragma unroll
        for (int h = 0; h < P; h += 2) {
            st_pair(xo_l + i0_l + h, xv[h], xv[h + 1]);
            st_pair(yo_l + i0_l + h, yv[h], yv[h + 1]);
            st_pair(to_l + i0_l + h, tv[h], tv[h + 1]);
        }
    }
    double* const w_un_l = ka->w_un;
#pragma unroll
    for (int h = 0; h < P; h += 2) st_pair(w_un_l + i0_l + h, wv[h], wv[h + 1]);
#ifndef SLAM_NO_EPILOGUE
    DeferParts dpl{};
    dpl.slab = ka->dp.slab;
    dpl.stride = ka->dp.stride;
    defer_epilogue(base_l, n_l, wv, xv, yv, tv, ka->refp, dpl, wave_s, (int)b2);
#endif
    FPROBE(5, wv[0]);
    return wv[0];
}

// The step's first fused block, after its own particles: the NEXT step's
// closed-form words (StepIO.zc) -- its eight sums (two per wave)
// and its expansion about this step's refp (the estimate two steps before it)
// moved twice.  Off the step's critical path: the next launch reads them; a
// step staged by the host is prepared again by its prestep.
template <int MOTION>
__device__ __forceinline__ void pf_fused_prep_next(const int wave_s, const double after) {
    if (MOTION == kMotionNone || blockIdx.x != 0) return;
    // (its arguments from the argument segment, as the tile's outputs, and
    // the step index read again: the step end advances it, after this launch)
    const SLAM_KARG FusedArgs* ka = kernarg_view<FusedArgs>(after);
    if (!ka->lc.closed) return;
    const int32_t st = __builtin_amdgcn_readfirstlane(ka->io.ctr[0]);
    if (st + 1 < ka->io.cap) {
        const StepIO io = karg_copy<StepIO>(ka->io);
        const PredictConst pc = karg_copy<PredictConst>(ka->pc);
        const LikConst lc = karg_copy<LikConst>(ka->lc);
        const double* __restrict__ lm = ka->lm;
        const double* __restrict__ refp = ka->refp;
        __shared__ double s_prep[16];
        const int32_t sn = st + 1;
        closed_prep_sums(lm, io.z + (size_t)sn * 2 * lc.nl, lc.nl, wave_s, 4, s_prep);
        __syncthreads();
        if (threadIdx.x == 0) {
            double px, py, pth;
            closed_prep_reference(refp, 2, io.ctl[2 * sn], io.ctl[2 * sn + 1], pc.dt, io.motion,
                                  px, py, pth);
            closed_prep_constants(s_prep, lc.nl, px, py, pth, io.zc + (size_t)sn * kZcWords);
        }
    }
}

#define SLAM_FUSED_PARAMS                                                                          \
    const int64_t n, const double* __restrict__ xs, const double* __restrict__ ys,                  \
        const double* __restrict__ ts, double* __restrict__ xo, double* __restrict__ yo,            \
        double* __restrict__ to, double* __restrict__ w_un,                                         \
        const double* __restrict__ c, int32_t* __restrict__ flags,                                  \
        const double* __restrict__ noise, const double* __restrict__ lm, StepIO io,                 \
        PredictConst pc, LikConst lc, uint64_t seed, const double* __restrict__ s_in,               \
        const double* __restrict__ refp, DeferParts dp
#define SLAM_FUSED_ARGS n, xs, ys, ts, xo, yo, to, w_un, c, flags, noise, lm, io, pc, lc, seed, \
                        s_in, refp, dp

// The step's uniform inputs and the RNG tables (every lane reaches the barrier)
#define SLAM_FUSED_PROLOGUE                                                                      \
    const int32_t st = io.ctr[0];                                                                \
    const uint32_t rstep = (uint32_t)io.ctr[1];                                                  \
    const int32_t rflag = flags[kFlagResample];                                                  \
    const double* __restrict__ zs = io.z + (size_t)st * 2 * (size_t)(lc.nl > 0 ? lc.nl : 1);     \
    const int wave_s = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);                    \
    __shared__ RngTabsLds s_rng;                                                                 \
    RngTabs rtab{};                                                                              \
    if constexpr ((MOTION != kMotionNone && !HOSTNOISE) ||                                      \
                  (MOTION == SLAM_MOTION_VELOCITY && SLAM_TAB_SINCOS)) {                         \
        rtab = rng_tabs_stage(&s_rng, (int)threadIdx.x, 256);                                    \
        __syncthreads();                                                                         \
    }

template <int MOTION, int LIK, bool HOSTNOISE, bool WT>
__global__ __launch_bounds__(256) SLAM_FUSED_ATTR void pf_fused_kernel(SLAM_FUSED_PARAMS) {
    static_assert(kDeferPPT % 2 == 0, "the fused kernel moves particle pairs");
    SLAM_FUSED_PROLOGUE
    const double w0 = pf_fused_tile<MOTION, LIK, HOSTNOISE, WT>(blockIdx.x, st, rstep, rflag, zs,
                                                                wave_s, rtab, SLAM_FUSED_ARGS);
    pf_fused_prep_next<MOTION>(wave_s, w0);
}

// ====================================================================
// numpy-order chunk sums (np.sum: 8192-element buffers, pairwise inside)
// ====================================================================
// Full chunk: 512 threads = 64 leaves x 8 accumulators; accumulator k of leaf
// L sums elements L*128 + k + 8m (m = 0..15) left to right; leaves combine as
// a perfect binary tree, which the xor-butterfly reproduces exactly.
// Tail chunk (< 8192): host-built leaf table + post-order combine program.
// With s_out != null the last block folds the partials left to right.
__global__ __launch_bounds__(512) void chunk_sum_kernel(
    const double* __restrict__ w, const int64_t n, double* __restrict__ part,
    const int32_t* __restrict__ tail_leaves, const int32_t* __restrict__ tail_ops,
    const int32_t n_tail_leaves, const int32_t n_tail_ops, unsigned* __restrict__ counter,
    double* __restrict__ s_out) {
    __shared__ double sh[1024];
    const int64_t base = (int64_t)blockIdx.x * kSumChunk;
    const int64_t len = (n - base < kSumChunk) ? (n - base) : kSumChunk;
    const int t = threadIdx.x;
    double blk = 0.0;
    if (len == kSumChunk) {
        const int leaf = t >> 3, k = t & 7;
        const double* p = w + base + leaf * 128 + k;
        double r = p[0];
#pragma unroll
        for (int m = 1; m < 16; ++m) r = r + p[8 * m];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) r = r + __shfl_xor(r, d, 64);
        if ((t & 63) == 0) sh[t >> 6] = r;
        __syncthreads();
        if (t == 0) blk = ((sh[0] + sh[1]) + (sh[2] + sh[3])) + ((sh[4] + sh[5]) + (sh[6] + sh[7]));
    } else {
        // tail: leaves of <= 128 elements, one per thread
        for (int L = t; L < n_tail_leaves; L += blockDim.x) {
            const int lo = tail_leaves[2 * L], cnt = tail_leaves[2 * L + 1];
            const double* a = w + base + lo;
            double res;
            if (cnt < 8) {
                res = 0.0;
                for (int i = 0; i < cnt; ++i) res = res + a[i];
            } else {
                double r[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = a[k];
                int i = 8;
                const int stop = cnt - (cnt % 8);
                for (; i < stop; i += 8) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) r[k] = r[k] + a[i + k];
                }
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (; i < cnt; ++i) res = res + a[i];
            }
            sh[L] = res;
        }
        __syncthreads();
        if (t == 0) {
            double stk[16];
            int sp = 0;
            for (int o = 0; o < n_tail_ops; ++o) {
                const int op = tail_ops[o];
                if (op >= 0) {
                    stk[sp++] = sh[op];
                } else {
                    const double b = stk[--sp];
                    const double a = stk[--sp];
                    stk[sp++] = a + b;
                }
            }
            blk = stk[0];
        }
    }
    if (t == 0) st_wt_d(&part[blockIdx.x], blk);
    if (!s_out) return;
    if (!arrive_last(counter)) return;
    double s = 0.0;                                   // buffer partials left to right
    const int nc = gridDim.x;
    for (int c0 = 0; c0 < nc; c0 += 1024) {
        const int cnt = min(1024, nc - c0);
        __syncthreads();
        for (int k = t; k < cnt; k += blockDim.x) sh[k] = ld_wt_d(&part[c0 + k]);
        __syncthreads();
        if (t == 0)
            for (int k = 0; k < cnt; ++k) s = s + sh[k];
    }
    if (t == 0) *s_out = s;
}

// exclusive scan of a small per-block array (write-through words) by one block
template <typename T, int NT>
__device__ void block_scan_array(const T* in, T* out, const int nb, T* total, T* sh,
                                 const bool wt = false) {
    const int per = (nb + NT - 1) / NT;
    const int b0 = threadIdx.x * per;
    auto ld = [](const T* p) -> T {
        if constexpr (sizeof(T) == 8) {
            const uint64_t u = ld_wt(p);
            T v;
            __builtin_memcpy(&v, &u, 8);
            return v;
        } else {
            return (T)ld_wt_i((const int32_t*)p);
        }
    };
    // up to kMaxPer words per thread stay in registers between the two passes
    // (one memory round trip instead of two)
    constexpr int kMaxPer = 8;
    const bool cached = per <= kMaxPer;
    T cv[kMaxPer];
    T loc = T(0);
    if (cached) {
#pragma unroll
        for (int k = 0; k < kMaxPer; ++k) {
            cv[k] = (k < per && b0 + k < nb) ? ld(in + b0 + k) : T(0);
            loc = loc + cv[k];
        }
    } else {
        for (int k = 0; k < per; ++k)
            if (b0 + k < nb) loc = loc + ld(in + b0 + k);
    }
    T tot;
    T ex = block_excl_scan<T, NT>(loc, sh, tot);
    auto st = [wt](T* p, const T v) {
        if (!wt) {
            *p = v;
        } else if constexpr (sizeof(T) == 8) {
            uint64_t u;
            __builtin_memcpy(&u, &v, 8);
            st_wt(p, u);
        } else {
            st_wt_i((int32_t*)p, (int32_t)v);
        }
    };
    if (cached) {
#pragma unroll
        for (int k = 0; k < kMaxPer; ++k)
            if (k < per && b0 + k < nb) {
                st(out + b0 + k, ex);
                ex = ex + cv[k];
            }
    } else {
        for (int k = 0; k < per; ++k)
            if (b0 + k < nb) {
                const T v = ld(in + b0 + k);
                st(out + b0 + k, ex);
                ex = ex + v;
            }
    }
    if (threadIdx.x == 0 && total) st(total, tot);
}

// The two tile-total scans of the exact cumsum (increments k: u64, special
// counts f: i32) with both arrays' loads issued together (one memory round
// trip for both); the same sums as two block_scan_array calls.
template <int NT, int kC = 8>
__device__ __forceinline__ void block_scan_pair(const uint64_t* kin, uint64_t* kout, uint64_t* ktotal,
                                const int32_t* fin, int32_t* fout, int32_t* ftotal, const int nb,
                                uint64_t* shk, int32_t* shf, int32_t* f_lds = nullptr,
                                uint64_t* k_lds = nullptr, const bool lds_only = false) {
    // lds_only (the merged launch, whose blocks get their offsets from the
    // hand-off records): no global copy where both LDS copies are kept
    const bool plain = !(lds_only && f_lds && k_lds);
    auto put = [&](const int e, const uint64_t kex, const int32_t fex) {
        if (plain) {
            st_wt(kout + e, kex);
            st_wt_i(fout + e, fex);
        }
        if (f_lds) f_lds[e] = fex;
        if (k_lds) k_lds[e] = kex;
    };
    // Up to two entries per thread: thread-contiguous, in registers, one
    // block scan per array.  Beyond, coalesced: wave w owns the contiguous
    // span [w*span, (w+1)*span) and walks it in rounds of 64 consecutive
    // entries (one per lane), kC rounds' loads in flight; each round is a DPP
    // wave scan.  (The thread-contiguous layout touches one cache line per
    // lane per access: 17-27 us for the 4,096 tile totals of NP = 2^23 in one
    // CU, against 7 us here.)
    constexpr int W = NT / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (nb <= 2 * NT) {
        const int b0 = 2 * threadIdx.x;
        uint64_t k2[2];
        int32_t f2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool ok = b0 + k < nb;
            k2[k] = ok ? ld_wt(kin + b0 + k) : 0;
            f2[k] = ok ? ld_wt_i(fin + b0 + k) : 0;
        }
        uint64_t ktot;
        int32_t ftot;
        uint64_t kex = block_excl_scan<uint64_t, NT>(k2[0] + k2[1], shk, ktot);
        int32_t fex = block_excl_scan<int32_t, NT>(f2[0] + f2[1], shf, ftot);
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (b0 + k < nb) {
                put(b0 + k, kex, fex);
                kex = kex + k2[k];
                fex = fex + f2[k];
            }
        if (threadIdx.x == 0) {
            st_wt(ktotal, ktot);
            st_wt_i(ftotal, ftot);
        }
        return;
    }
    const int span = ((nb + W * 64 - 1) / (W * 64)) * 64;
    const int R = span / 64;
    const int e0 = wid * span + lane;
    uint64_t kv[kC];
    int32_t fv[kC];
    uint64_t kloc = 0;
    int32_t floc = 0;
    for (int r0 = 0; r0 < R; r0 += kC) {
#pragma unroll
        for (int r = 0; r < kC; ++r) {
            const int e = e0 + (r0 + r) * 64;
            const bool ok = r0 + r < R && e < nb;
            kv[r] = ok ? ld_wt(kin + e) : 0;
            fv[r] = ok ? ld_wt_i(fin + e) : 0;
        }
#pragma unroll
        for (int r = 0; r < kC; ++r) {
            kloc = kloc + kv[r];
            floc = floc + fv[r];
        }
    }
    uint64_t ktot;
    int32_t ftot;
    // lane 0's exclusive prefix over the block = the sum of the lower waves
    uint64_t krun = readlane_int(block_excl_scan<uint64_t, NT>(kloc, shk, ktot), 0);
    int32_t frun = readlane_int(block_excl_scan<int32_t, NT>(floc, shf, ftot), 0);
    for (int r0 = 0; r0 < R; r0 += kC) {
        if (R > kC) {                              // (one chunk: still in registers)
#pragma unroll
            for (int r = 0; r < kC; ++r) {
                const int e = e0 + (r0 + r) * 64;
                const bool ok = r0 + r < R && e < nb;
                kv[r] = ok ? ld_wt(kin + e) : 0;
                fv[r] = ok ? ld_wt_i(fin + e) : 0;
            }
        }
#pragma unroll
        for (int r = 0; r < kC; ++r) {
            if (r0 + r < R) {                      // (wave-uniform)
                const uint64_t ki = wave_incl_scan(kv[r]);
                const int32_t fi = wave_incl_scan(fv[r]);
                const int e = e0 + (r0 + r) * 64;
                if (e < nb) {
                    put(e, krun + (ki - kv[r]), frun + (fi - fv[r]));
                }
                krun += readlane_int(ki, 63);
                frun += readlane_int(fi, 63);
            }
        }
    }
    if (threadIdx.x == 0) {
        st_wt(ktotal, ktot);
        st_wt_i(ftotal, ftot);
    }
}

// ====================================================================
// reductions of the step end (particle_filter.py:226-237): block partials,
// their fixed-order combination and the step's result record
// ====================================================================
__device__ __forceinline__ void bp_zero(BlockPartial& a) {
    a.maxv = -1.0;
    a.maxi = INT64_MAX;
    a.sw = a.sw2 = 0.0;
    for (int k = 0; k < 3; ++k) a.m1[k] = 0.0;
    for (int k = 0; k < 6; ++k) a.m2[k] = 0.0;
}

__device__ __forceinline__ void bp_merge(BlockPartial& r, const BlockPartial& o) {
    if (o.maxv > r.maxv || (o.maxv == r.maxv && o.maxi < r.maxi)) {
        r.maxv = o.maxv;
        r.maxi = o.maxi;
    }
    r.sw += o.sw;
    r.sw2 += o.sw2;
    for (int q = 0; q < 3; ++q) r.m1[q] += o.m1[q];
    for (int q = 0; q < 6; ++q) r.m2[q] += o.m2[q];
}

// xor-butterfly over the 64 lanes (lower lane always on the left: a fixed tree)
template <int W = 64>
__device__ __forceinline__ void bp_wave_reduce(BlockPartial& a) {
#pragma unroll
    for (int d = 1; d < W; d <<= 1) {
        BlockPartial o;
        o.maxv = __shfl_xor(a.maxv, d, 64);
        o.maxi = __shfl_xor(a.maxi, d, 64);
        o.sw = __shfl_xor(a.sw, d, 64);
        o.sw2 = __shfl_xor(a.sw2, d, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) o.m1[k] = __shfl_xor(a.m1[k], d, 64);
#pragma unroll
        for (int k = 0; k < 6; ++k) o.m2[k] = __shfl_xor(a.m2[k], d, 64);
        if (threadIdx.x & d) {
            bp_merge(o, a);
            a = o;
        } else {
            bp_merge(a, o);
        }
    }
}

// block-level fixed-order reduction of per-thread partials (result in thread 0):
// a butterfly inside every wave, then a butterfly over the wave partials in wave 0
__device__ __forceinline__ BlockPartial bp_block_reduce(BlockPartial a, BlockPartial* shp) {
    bp_wave_reduce(a);
    const int nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) shp[threadIdx.x >> 6] = a;
    __syncthreads();
    BlockPartial r;
    if (threadIdx.x < 64) {
        if ((int)threadIdx.x < nw) r = shp[threadIdx.x];
        else bp_zero(r);
        if (nw > 8) bp_wave_reduce<16>(r);
        else if (nw > 4) bp_wave_reduce<8>(r);
        else bp_wave_reduce<4>(r);
    }
    __syncthreads();
    return r;
}

// result record from the combined partial; x_est is given (the particle at
// the argmax, taken from the fused blocks' partials)
// The flag words the step's record reads (fetched early by the finalize, whose
// record is on the step's critical path)
struct FlagWords {
    int32_t resample, status, n_special, dd_waves, mark_gen;
};
__device__ __forceinline__ FlagWords load_flag_words(const int32_t* flags) {
    return FlagWords{flags[kFlagResample], flags[kFlagStatus], flags[kFlagNSpecial],
                     flags[kFlagDDWaves], flags[kFlagMarkGen]};
}

// with_cov false (a split step end, pf_finalize.inl): the record's cov is
// formed by its reader from the step's FinMoments; zeros here
__device__ int32_t write_result_fw(const BlockPartial& r, const double* xe, double* refp,
                                const double (&rp)[3], const double s, int32_t* flags,
                                const FlagWords fw, const double ess_th,
                                const double ess_band, slam_pf_result* res,
                                const int32_t resampled_known, slam_pf_result* res_host = nullptr,
                                const bool with_cov = true) {
    slam_pf_result o;
    o.max_idx = r.maxi;
    o.max_val = r.maxv;
    o.x_est[0] = xe[0];
    o.x_est[1] = xe[1];
    o.x_est[2] = xe[2];
    if (with_cov) {
        cov_from_moments(r.sw, r.m1, r.m2, o.cov);
    } else {
        for (int a = 0; a < 9; ++a) o.cov[a] = 0.0;
    }
    o.ess = 1.0 / r.sw2;
    o.weight_sum = s;
    o.resampled = resampled_known >= 0 ? resampled_known : (fw.resample != 0);
    o.resample_next = (o.ess < ess_th) ? 1 : 0;
    o.ess_near = (fabs(o.ess - ess_th) <= ess_band * ess_th) ? 1 : 0;
    o.status = fw.status;
    o.n_special = fw.n_special;
    o.dd_waves = fw.dd_waves;
    flags[kFlagDDWaves] = 0;
    flags[kFlagResample] = o.resample_next;
    flags[kFlagMarkGen] = fw.mark_gen + 1;
    flags[kFlagStatus] = 0;
    // the estimate, kept two steps deep as the expansion's reference
    // (closed_prep_reference: the argmax particle is the same bits however
    // the filter is sharded, which a summed mean would not be)
    for (int k = 0; k < 3; ++k) {
        refp[4 + k] = rp[k];
        refp[k] = o.x_est[k];
    }
    refp[7] = 2.0;
    *res = o;
    if (res_host) *res_host = o;
    return o.resample_next;
}

// returns resample_next (the flag it stored)
__device__ int32_t write_result_xe(const BlockPartial& r, const double* xe, double* refp,
                                const double s, int32_t* flags, const double ess_th,
                                const double ess_band, slam_pf_result* res,
                                const int32_t resampled_known, slam_pf_result* res_host = nullptr) {
    const double rp[3] = {refp[0], refp[1], refp[2]};
    return write_result_fw(r, xe, refp, rp, s, flags, load_flag_words(flags), ess_th, ess_band, res,
                           resampled_known, res_host);
}

// np.sum of one full 8192-element buffer from its 64 leaf sums (perfect
// pairwise tree, left + right at every node).
__device__ __forceinline__ double chunk_tree64(const double* __restrict__ L) {
    double stk[7];
    for (int i = 0; i < 64; ++i) {
        double v = L[i];
        int b = 0;
        for (; (i >> b) & 1; ++b) v = stk[b] + v;
        stk[b] = v;
    }
    return stk[6];
}

// np.sum of a tail buffer (< 8192 elements) from raw weights: leaves by the
// block's lanes, the post-order program by lane 0 (as chunk_sum_kernel).
__device__ double tail_chunk_sum(const double* __restrict__ w, const int32_t* __restrict__ leaves,
                                 const int32_t* __restrict__ ops, const int32_t n_leaves,
                                 const int32_t n_ops, double* sh) {
    for (int L = threadIdx.x; L < n_leaves; L += blockDim.x) {
        const int lo = leaves[2 * L], cnt = leaves[2 * L + 1];
        const double* a = w + lo;
        double res;
        if (cnt < 8) {
            res = 0.0;
            for (int i = 0; i < cnt; ++i) res = res + a[i];
        } else {
            double r[8];
            for (int k = 0; k < 8; ++k) r[k] = a[k];
            int i = 8;
            const int stop = cnt - (cnt % 8);
            for (; i < stop; i += 8)
                for (int k = 0; k < 8; ++k) r[k] = r[k] + a[i + k];
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (; i < cnt; ++i) res = res + a[i];
        }
        sh[L] = res;
    }
    __syncthreads();
    double out = 0.0;
    if (threadIdx.x == 0) {
        double stk[16];
        int sp = 0;
        for (int o = 0; o < n_ops; ++o) {
            const int op = ops[o];
            if (op >= 0) {
                stk[sp++] = sh[op];
            } else {
                const double b = stk[--sp];
                const double a = stk[--sp];
                stk[sp++] = a + b;
            }
        }
        out = stk[0];
    }
    __syncthreads();
    return out;
}

#include "pf_finalize.inl"

// w = w_un / s (NaN -> 1/NP): materialise the current weights (get_state, np.sum)
__global__ __launch_bounds__(256) void normalize_only_kernel(const int64_t n,
                                                             const double* __restrict__ w_un,
                                                             const double* __restrict__ s,
                                                             const double np_recip,
                                                             double* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = norm_w(w_un[i], *s, np_recip);
}

// S1: fused-block (kPartPer) totals of w = w_un / s and their prefix.
__global__ __launch_bounds__(kPartPer) void scan_bsum256_kernel(
    const double* __restrict__ w_un, const double* __restrict__ s_in, const double np_recip,
    const int64_t n, double* __restrict__ bsum, double* __restrict__ boff,
    unsigned* __restrict__ counter) {
    __shared__ double sh[kPartPer / 64 + 1];
    const int64_t i = (int64_t)blockIdx.x * kPartPer + threadIdx.x;
    const double v = (i < n) ? norm_w(w_un[i], *s_in, np_recip) : 0.0;
    double tot;
    block_excl_scan<double, kPartPer>(v, sh, tot);
    if (threadIdx.x == 0) st_wt_d(&bsum[blockIdx.x], tot);
    if (!arrive_last(counter)) return;
    block_scan_array<double, kPartPer>(bsum, boff, gridDim.x, boff + gridDim.x, sh);
}

// ====================================================================
// exact sequential cumsum (np.cumsum, particle_filter.py:212)
// ====================================================================
// the weight an exact-cumsum pass reads: w_un / s (s_div), or w itself where
// the caller passes normalised weights (s_div null)
__device__ __forceinline__ double scan_w(const double* __restrict__ w, const int64_t i,
                                         const double* __restrict__ s_div, const double np_recip) {
    return s_div ? norm_w(w[i], *s_div, np_recip) : w[i];
}

// S3: classify every element; k_i = increment on the run's ulp grid.  The last
// block scans the per-block special counts and increment sums.
// base_off: approximate cumsum before local element 0 (other ranks' weight).
__global__ __launch_bounds__(kScanThreads) void scan_classify_kernel(
    const double* __restrict__ w, const int64_t n, const double* __restrict__ boff,
    const double* __restrict__ base_off, double* __restrict__ approx,
    uint64_t* __restrict__ kincl, int32_t* __restrict__ fexcl, uint64_t* __restrict__ bk,
    int32_t* __restrict__ bf, uint64_t* __restrict__ boffk, int32_t* __restrict__ bofff,
    uint64_t* __restrict__ ktot, int32_t* __restrict__ nspec, const double delta,
    const int64_t gbase, unsigned* __restrict__ counter, const int32_t* __restrict__ flags,
    const int32_t force, const double* __restrict__ s_div, const double np_recip,
    const int32_t gran) {
    if (!force && flags[kFlagResample] != 1) return;
    __shared__ double shd[kScanThreads / 64 + 1];
    __shared__ uint64_t shk[kScanThreads / 64 + 1];
    __shared__ int32_t shf[kScanThreads / 64 + 1];
    const int64_t base = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * kScanPer;
    double v[kScanPer];
    double loc = 0.0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        v[k] = (base + k < n) ? scan_w(w, base + k, s_div, np_recip) : 0.0;
        loc += v[k];
    }
    double dtot;
    double run = block_excl_scan<double, kScanThreads>(loc, shd, dtot) +
                 boff[(int64_t)blockIdx.x * (kScanBlock / gran)] +
                 (base_off ? *base_off : 0.0);
    uint64_t kk[kScanPer];
    int32_t ff[kScanPer];
    uint64_t ksum = 0;
    int32_t fsum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        const double prev = run;
        run = run + v[k];
        const int64_t gi = gbase + base + k;
        bool reg = (gi != 0) && (base + k < n);
        uint64_t inc = 0;
        if (reg) {
            const int E = sum_binade(run);
            reg = (sum_binade(prev) == E);
            if (reg && E != -1022) reg = prev >= ldexp(1.0, E) * (1.0 + delta);
            if (reg) reg = run <= ldexp(1.0, E + 1) * (1.0 - delta);
            if (reg) {
                const double t = ldexp(v[k], 52 - E);
                const double fl = floor(t);
                reg = (t - fl) != 0.5;
                inc = (uint64_t)rint(t);
            }
        }
        kk[k] = reg ? inc : 0;
        ff[k] = (reg || base + k >= n) ? 0 : 1;
        ksum += kk[k];
        fsum += ff[k];
        if (base + k < n) approx[base + k] = run;
    }
    uint64_t ktot_b;
    int32_t ftot_b;
    uint64_t kex = block_excl_scan<uint64_t, kScanThreads>(ksum, shk, ktot_b);
    int32_t fex = block_excl_scan<int32_t, kScanThreads>(fsum, shf, ftot_b);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (base + k < n) {
            kex += kk[k];
            kincl[base + k] = kex;
            fexcl[base + k] = (fex << 1) | ff[k];
            fex += ff[k];
        }
    }
    if (threadIdx.x == 0) {
        st_wt(&bk[blockIdx.x], ktot_b);
        st_wt_i(&bf[blockIdx.x], ftot_b);
    }
    if (!arrive_last(counter)) return;
    block_scan_array<uint64_t, kScanThreads>(bk, boffk, gridDim.x, ktot, shk);
    __syncthreads();
    block_scan_array<int32_t, kScanThreads>(bf, bofff, gridDim.x, nspec, shf);
}

// S6: sequential fold over the ordered special elements (one block; tiles in
// LDS).  Runs of regular elements are added as one exact integer multiple of
// their binade's ulp.  Falls back to the plain sequential recurrence if a
// run check fails (flags status bit 1).
__device__ void serial_fold(const SpecialIn* __restrict__ spec, SpecialOut* __restrict__ out,
                            const int32_t M, const uint64_t ktot, const int64_t n_total,
                            int32_t* __restrict__ flags, const double* __restrict__ w,
                            double* __restrict__ c, const int64_t n_local, const bool wt_loads,
                            const double* __restrict__ s_div, const double np_recip) {
    __shared__ SpecialIn tile[257];
    __shared__ int bad;
    double s = 0.0;
    if (threadIdx.x == 0) {
        bad = 0;
        flags[kFlagNSpecial] = M;
    }
    for (int32_t t0 = 0; t0 < M; t0 += 256) {
        __syncthreads();
        const int32_t cnt = min(257, M - t0);
        for (int k = threadIdx.x; k < cnt; k += blockDim.x)
            tile[k] = wt_loads ? ld_wt_struct(&spec[t0 + k]) : spec[t0 + k];
        __syncthreads();
        if (threadIdx.x == 0 && !bad) {
            const int lim = min(256, M - t0);
            for (int k = 0; k < lim; ++k) {
                const SpecialIn& e = tile[k];
                s = s + e.w;
                SpecialOut o;
                o.cs = s;
                o.P = e.P;
                o.E = e.E;
                o.pad = 0;
                const bool last = (t0 + k + 1 >= M);
                const int64_t nxt = last ? n_total : tile[k + 1].idx;
                if (nxt - e.idx > 1) {
                    const uint64_t K = (last ? ktot : tile[k + 1].P) - e.P;
                    const int E = e.E;
                    if (sum_binade(s) != E) { bad = 1; break; }
                    const double s2 = s + (double)K * ldexp(1.0, E - 52);
                    const double hi = (E == -1022) ? 0x1p-1021 : ldexp(1.0, E + 1);
                    if (!(s2 < hi) || (double)K >= 0x1p53) { bad = 1; break; }
                    s = s2;
                }
                out[t0 + k] = o;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && bad) {
        flags[kFlagStatus] |= 2;
        flags[kFlagFallback] = 1;
        double r = 0.0;
        for (int64_t i = 0; i < n_local; ++i) {
            r = r + scan_w(w, i, s_div, np_recip);
            c[i] = r;
        }
    } else if (threadIdx.x == 0) {
        flags[kFlagFallback] = 0;
    }
}

// ====================================================================
// Lean exact cumsum (single-GPU handles), one WAVE per 512-element tile (a
// fused block's particles): no per-element scratch and no block barrier in
// the per-tile work -- the tile's prefix sums are wave scans.  Pass A
// classifies each tile and stages its few special elements; its last block
// places them in global order and folds them; pass C expands c from the
// classification (kept in registers in the merged launch, recomputed in the
// two-launch form) and writes the inverse resample map.  Reads w once (twice
// in the two-launch form), writes c once.
// ====================================================================
constexpr int kWaveTile = 64 * kScanPer;                 // 512 elements
static_assert(kWaveTile == kPartPer, "a scan tile is a fused block (boff, carry indexing)");
constexpr int kTilesPerBlock = kScanThreads / 64;

struct TileScan {
    uint64_t kex;            // exclusive prefix of the tile-local increments (this lane)
    int32_t fex;             // exclusive prefix of the tile-local special count (this lane)
    uint64_t kk[kScanPer];   // increments of this lane's elements (0 for specials)
    int32_t ff[kScanPer];    // special flags
    double v[kScanPer];      // the weights
    int E[kScanPer];         // binade of the approximate prefix after the element
};

// exclusive wave scan; `total` = the wave's sum (every lane)
template <typename T>
__device__ __forceinline__ T wave_excl_scan(const T v, T& total) {
    const T inc = wave_incl_scan(v);
    if constexpr (std::is_integral<T>::value) {
        total = readlane_int(inc, 63);
        return inc - v;
    } else {
        T ex = __shfl_up(inc, 1, 64);
        if ((threadIdx.x & 63) == 0) ex = T(0);
        total = __shfl(inc, 63, 64);
        return ex;
    }
}

// Tile `tile` of the weights w = w_un / s, lane l owns elements 8l .. 8l+7
// (four 16-byte loads; w_un is padded to whole tiles).  off: the approximate
// prefix before the tile (the finalize pass's fused-block prefix).
__device__ __forceinline__ void wave_tile_classify(const double* __restrict__ w_un,
                                                   const double s, const double np_recip,
                                                   const int64_t n, const int64_t tile,
                                                   const double off, const double delta,
                                                   TileScan& ts, uint64_t& ktile,
                                                   int32_t& ftile) {
    const int lane = threadIdx.x & 63;
    const int64_t base = tile * kWaveTile + 8 * lane;
#pragma unroll
    for (int h = 0; h < kScanPer; h += 2) {
        const double2 w2 = *reinterpret_cast<const double2*>(w_un + base + h);
        ts.v[h] = (base + h < n) ? norm_w(w2.x, s, np_recip) : 0.0;
        ts.v[h + 1] = (base + h + 1 < n) ? norm_w(w2.y, s, np_recip) : 0.0;
    }
    double loc = 0.0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) loc += ts.v[k];
    // the approximate prefix (any fixed order: the classification's margins
    // cover its error, and pass C recomputes it with this same code)
    double wtot;
    double run = wave_excl_scan_rows(loc, wtot) + off;
    uint64_t ksum = 0;
    int32_t fsum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        const double prev = run;
        run = run + ts.v[k];
        const int64_t gi = base + k;
        bool reg = (gi != 0) && (gi < n);
        uint64_t inc = 0;
        const int E = sum_binade(run);
        if (reg) {
            reg = (sum_binade(prev) == E);
            if (reg && E != -1022) reg = prev >= ldexp(1.0, E) * (1.0 + delta);
            if (reg) reg = run <= ldexp(1.0, E + 1) * (1.0 - delta);
            if (reg) {
                const double tt = ldexp(ts.v[k], 52 - E);
                const double fl = floor(tt);
                reg = (tt - fl) != 0.5;
                inc = (uint64_t)rint(tt);
            }
        }
        ts.kk[k] = reg ? inc : 0;
        ts.ff[k] = (reg || gi >= n) ? 0 : 1;
        ts.E[k] = E;
        ksum += ts.kk[k];
        fsum += ts.ff[k];
    }
    ts.kex = wave_excl_scan(ksum, ktile);
    ts.fex = wave_excl_scan(fsum, ftile);
}

// The four tiles of a block combine their totals (LDS, one barrier): the
// block's staging area, its (k, f) totals and the tiles' exclusive offsets
// inside the block.  The last arriver then scans one total per block.
__device__ __forceinline__ void block_tile_offsets(const uint64_t ktile, const int32_t ftile,
                                                   uint64_t& kofs, int32_t& fofs,
                                                   uint64_t& kblk, int32_t& fblk) {
    __shared__ uint64_t s_kt[kTilesPerBlock];
    __shared__ int32_t s_ft[kTilesPerBlock];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_kt[wave] = ktile;
        s_ft[wave] = ftile;
    }
    __syncthreads();
    kofs = 0;
    fofs = 0;
    kblk = 0;
    fblk = 0;
#pragma unroll
    for (int w = 0; w < kTilesPerBlock; ++w) {
        if (w < wave) {
            kofs += s_kt[w];
            fofs += s_ft[w];
        }
        kblk += s_kt[w];
        fblk += s_ft[w];
    }
}

// Stage a classified tile's specials in its block's area (block-local P,
// write-through); thread 0 publishes the block totals.
__device__ __forceinline__ void wave_tile_stage(const int64_t b, const int64_t tile,
                                                const TileScan& ts,
                                                const uint64_t kofs, const int32_t fofs,
                                                const uint64_t kblk, const int32_t fblk,
                                                SpecialIn* __restrict__ stage,
                                                uint64_t* __restrict__ bk,
                                                int32_t* __restrict__ bf) {
    const int lane = threadIdx.x & 63;
    uint64_t kex = kofs + ts.kex;
    int32_t fex = fofs + ts.fex;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        kex += ts.kk[k];
        if (ts.ff[k]) {
            SpecialIn r;
            r.idx = tile * kWaveTile + 8 * lane + k;
            r.P = kex;                                  // block-local inclusive prefix
            r.w = ts.v[k];
            r.E = ts.E[k];
            r.pad = 0;
            st_wt_struct(&stage[b * kScanBlock + fex], r);
            ++fex;
        }
    }
    if (threadIdx.x == 0) {
        st_wt(&bk[b], kblk);
        st_wt_i(&bf[b], fblk);
    }
}


// The lean path's place + fold (last block of pass A): the M specials, in
// global order, are located in the tiles' staging areas (tile offsets bofff in
// LDS, searched per lane), given their global P, and folded by wave 0 in
// chunks of 64: lane l precomputes everything that does not depend on the
// running sum (the exact run increment K u of the following regular run, the
// binade bounds the checks use), then the running sum walks the 64 lanes --
// two dependent adds per special, operands read from the lanes into SGPRs.
// Bit-identical to serial_fold; a failed run check takes the same fallback
// (the plain sequential recurrence, flagged).
// The merged launch (hand != null in lean_last_block) stores the folded
// specials as tagged granules instead (tag_out, epoch) and keeps the first
// kFoldSpecLds of them and the tiles' k offsets in LDS (s_so, s_offk) for the
// hand-off records.  Returns the failed-run-check verdict to every thread;
// lean_fold_finish then publishes it and runs the fallback.
constexpr int kFoldTilesLds = 4096;
constexpr int kFoldTilesHand = 1024;  // the merged launch (its co-resident grids fit)
constexpr int kFoldSpecLds = 256;
__device__ __forceinline__ bool lean_place_fold(const SpecialIn* __restrict__ stage,
                                const uint64_t* __restrict__ boffk,
                                const int32_t* __restrict__ bofff, const int ntiles,
                                const int32_t M, const uint64_t ktot, const int64_t n,
                                SpecialOut* __restrict__ out, int32_t* __restrict__ flags,
                                int32_t* __restrict__ s_off, const int lds_tiles,
                                const uint64_t* __restrict__ s_offk = nullptr,
                                uint64_t* __restrict__ tag_out = nullptr, const uint32_t epoch = 0,
                                SpecialOut* __restrict__ s_so = nullptr,
                                uint64_t* __restrict__ hand = nullptr) {
    // s_off (and s_offk): the tiles' offsets in LDS (lds_tiles words), already
    // filled by the scan that produced bofff (boffk) when ntiles fits
    __shared__ int s_bad;
    const bool in_lds = ntiles <= lds_tiles;
    const bool k_in_lds = s_offk && in_lds;
    __shared__ int s_issued;
    if (threadIdx.x == 0) {
        s_bad = 0;
        s_issued = M <= 0;
        flags[kFlagNSpecial] = M;
    }
    __syncthreads();
    if (threadIdx.x >= 64) {
        // hand (the merged launch): the other waves write every block's offsets
        // into its hand-off record meanwhile (ntiles is the block count there).
        // One write-through store per lane is one fabric write, a thousand of
        // them queue for microseconds in this CU's memory pipeline, and the
        // fold's own loads would wait behind them: they start once wave 0 has
        // issued its first chunk's loads, and travel while the chain runs.
        if (hand) {
            while (*(volatile int*)&s_issued == 0) __builtin_amdgcn_s_sleep(1);
            for (int b = threadIdx.x - 64; b < ntiles; b += kScanThreads - 64) {
                const uint64_t k = k_in_lds ? s_offk[b] : ld_wt(&boffk[b]);
                const int32_t f = in_lds ? s_off[b] : ld_wt_i(&bofff[b]);
                st_offsets_tagged(hand + (int64_t)b * kHandGranules, k, f, epoch);
            }
        }
    } else {
        const int lane = threadIdx.x;
        // special m: its tile (last tile whose offset is <= m), then the staged
        // record's loads; returns the tile (P is block-local until its offset is added)
        auto load_special = [&](const int64_t m, SpecialIn& e) -> int {
            int lo = 0, hi = ntiles - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                const int32_t o = in_lds ? s_off[mid] : ld_wt_i(&bofff[mid]);
                if (o <= m) lo = mid;
                else hi = mid - 1;
            }
            const int32_t o = in_lds ? s_off[lo] : ld_wt_i(&bofff[lo]);
            e = ld_wt_struct(&stage[(int64_t)lo * kScanBlock + (m - o)]);
            return lo;
        };
        double s = 0.0;
        bool bad = false;
        // chunks of 63 specials: lane 63 only supplies the next chunk's first
        for (int64_t t0 = 0; t0 < M; t0 += 63) {
            const int64_t m = t0 + lane;
            SpecialIn e{};
            int tile = 0;
            if (m < M) tile = load_special(m, e);
            if (t0 == 0 && lane == 0) *(volatile int*)&s_issued = 1;
            if (m < M) e.P += k_in_lds ? s_offk[tile] : ld_wt(&boffk[tile]);
            // the following special's index and prefix (or the end of the array)
            int64_t nidx = __shfl_down((long long)e.idx, 1, 64);
            uint64_t nP = (uint64_t)__shfl_down((long long)e.P, 1, 64);
            if (m + 1 >= M) {
                nidx = n;
                nP = ktot;
            }
            const bool mine = (lane < 63) && (m < M);
            const bool run = mine && (nidx - e.idx > 1);
            const uint64_t K = nP - e.P;
            const int E = e.E;
            double lo = -__builtin_inf(), hi = __builtin_inf(), ku = 0.0;
            if (run) {
                lo = (E == -1022) ? 0.0 : ldexp(1.0, E);
                hi = (E == -1022) ? 0x1p-1021 : ldexp(1.0, E + 1);
                ku = (double)K * ldexp(1.0, E - 52);
                if ((double)K >= 0x1p53) bad = true;
            }
            const double w = mine ? e.w : 0.0;
            // the chain: two dependent adds per special, the operands read into
            // scalars (fully unrolled: the reads do not wait on the chain); each
            // lane keeps the sums at its own special and checks its binade after
            double cs = 0.0, cr = 0.0;
            const int lim = (M - t0 < 63) ? (int)(M - t0) : 63;
#pragma unroll
            for (int l = 0; l < 63; ++l) {
                if (l < lim) {                            // wave-uniform
                    s = s + readlane_d(w, l);             // the special element's own add
                    if (lane == l) cs = s;
                    s = s + readlane_d(ku, l);            // the run: K ulps, exact
                    if (lane == l) cr = s;
                }
            }
            if (lane < lim && (!(cs >= lo) || !(cs < hi) || !(cr < hi))) bad = true;   // its run keeps the binade
            if (mine) {
                SpecialOut o;
                o.cs = cs;
                o.P = e.P;
                o.E = e.E;
                o.pad = 0;
                if (tag_out) st_spec_tagged(tag_out, m, o, epoch);
                else st_wt_struct(&out[m], o);
                if (s_so && m < kFoldSpecLds) s_so[m] = o;
            }
        }
        if (__any(bad) && lane == 0) s_bad = 1;
    }
    __syncthreads();
    return s_bad != 0;
}

// The fold's verdict for the passes that follow, and the fallback itself
__device__ __forceinline__ void lean_fold_finish(const bool bad, const int64_t n,
                                                 int32_t* __restrict__ flags,
                                                 const double* __restrict__ w_un,
                                                 const double* __restrict__ s_in,
                                                 const double np_recip, double* __restrict__ c) {
    if (threadIdx.x == 0) {
        if (bad) {
            flags[kFlagStatus] |= 2;
            st_wt_i(&flags[kFlagFallback], 1);
            double r = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                r = r + norm_w(w_un[i], *s_in, np_recip);
                c[i] = r;
            }
        } else {
            st_wt_i(&flags[kFlagFallback], 0);
        }
    }
}

// Number of systematic positions at or below v: #{i in [0, n) :
// fl(fl(i (1/NP)) + ofs) <= v} (particle_filter.py:213-215; the positions are
// monotone in i).  An estimate from the inverse, then exact steps.
// The count is carried as a double (exact: n < 2^31), so the position of index
// i is fl(fl(i (1/NP)) + ofs) without an int64 -> double conversion per probe.
__device__ __forceinline__ int64_t positions_upto(const double v, const int64_t n,
                                                  const double rstep, const double ofs) {
    if (!(v >= ofs)) return 0;
    const double dn = (double)n;
    double e = floor((v - ofs) * dn) + 1.0;
    e = e < 0.0 ? 0.0 : (e > dn ? dn : e);
    while (e > 0.0 && (e - 1.0) * rstep + ofs > v) e = e - 1.0;
    while (e < dn && e * rstep + ofs <= v) e = e + 1.0;
    return (int64_t)e;
}

// Pass C for one tile, once the specials are folded: every c_i from the
// tile's classification and the folded specials, then the inverse resample
// map.  Source j serves the positions i with c_{j-1} < pos_i <= c_j (the
// lower_bound of particle_filter.py:218-220), a run [s_j, e_j) with s_j =
// #positions <= c_{j-1}.  A selected element marks the start of its run
// (mark[s_j] = tagged j) and gives every fused block whose first position lies
// in the run its carry (carry[fb] = j); positions past the last cumulative
// weight (the reference's IndexError) are marked with j = n.  The fused block
// then reads its marks and carry and takes a running max -- no search.
// bkb, bfb: the block's global offsets (boffk[b], bofff[b]).  SO reads folded
// special m: SoPlain after a launch boundary, SoTagged inside the merged
// launch, where a special that never arrives (`lost`) makes the wave skip its
// tile with status bit 3.
struct SoPlain {
    const SpecialOut* __restrict__ so;
    __device__ __forceinline__ SpecialOut operator()(const int32_t m, bool&) const { return so[m]; }
};
struct SoTagged {
    const uint64_t* __restrict__ tag;
    uint32_t epoch;
    int32_t m0;              // the special of the block's record (the one before the block)
    SpecialOut p0;
    __device__ __forceinline__ SpecialOut operator()(const int32_t m, bool& lost) const {
        return m == m0 ? p0 : ld_spec_tagged(tag, m, epoch, lost);
    }
};
template <typename SO>
__device__ void wave_tile_expand(const int64_t tile, const TileScan& ts, const int64_t n,
                                 const uint64_t bkb, const int32_t bfb, const uint64_t kofs,
                                 const int32_t fofs, const SO& ld_so, int32_t* __restrict__ flags,
                                 double* __restrict__ c, int64_t* __restrict__ mark,
                                 int32_t* __restrict__ carry, const double ofs, const int64_t gen,
                                 const PredictConst& pc, const bool store_c = true) {
    const int lane = threadIdx.x & 63;
    const uint64_t bk0 = bkb + kofs;                // the tile's global offsets
    const int32_t bf0 = bfb + fofs;
    uint64_t kin = bk0 + ts.kex;
    int32_t m = bf0 + ts.fex;
    double out[kScanPer];
    bool lost = false;
    SpecialOut p = ld_so(m > 0 ? m - 1 : 0, lost);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        kin += ts.kk[k];
        if (ts.ff[k]) {
            p = ld_so(m, lost);
            out[k] = p.cs;
            ++m;
        } else {
            out[k] = p.cs + (double)(kin - p.P) * ldexp(1.0, p.E - 52);
        }
    }
    // element j0 - 1 of the tile's first lane, from its run's special
    double cfirst = -__builtin_inf();
    if (lane == 0 && tile != 0 && mark) {
        const SpecialOut q = ld_so(bf0 - 1, lost);
        cfirst = q.cs + (double)(bk0 - q.P) * ldexp(1.0, q.E - 52);
    }
    if (__any(lost)) {                             // (never with SoPlain)
        if (lane == 0) atomicOr(&flags[kFlagStatus], 8);
        return;
    }
    const int64_t j0 = tile * kWaveTile + 8 * lane;
    if (store_c) {                                 // (the device-decided step needs only the marks)
#pragma unroll
        for (int h = 0; h < kScanPer; h += 2)      // c is padded to whole tiles
            *reinterpret_cast<double2*>(c + j0 + h) = double2{out[h], out[h + 1]};
    }
    PROBE_MAX(6);
    if (!mark) return;
    // ---- inverse map: runs of this lane's elements
    double cprev = __shfl_up(out[kScanPer - 1], 1, 64);
    if (lane == 0) cprev = cfirst;
    int64_t sj = positions_upto(cprev, n, pc.rstep, ofs);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        const int64_t j = j0 + k;
        const bool ok = j < n;
        const int64_t ej = ok ? positions_upto(out[k], n, pc.rstep, ofs) : sj;
        // the fused blocks whose first position lies in the run
        int64_t flo = 0, fhi = 0, val = j;
        if (ok && ej > sj) {
            mark[sj] = gen | j;
            flo = (sj + kPartPer - 1) / kPartPer;
            fhi = (ej + kPartPer - 1) / kPartPer;
        }
        if (ok && j == n - 1 && ej < n) mark[ej] = gen | n;
        // carries, written by the whole wave (a heavy element may own many)
        uint64_t act = __ballot(fhi > flo);
        while (act) {
            const int l = __ffsll((unsigned long long)act) - 1;
            act &= act - 1;
            const int64_t L = __shfl(flo, l, 64), H = __shfl(fhi, l, 64);
            const int32_t J = (int32_t)__shfl(val, l, 64);
            for (int64_t f = L + lane; f < H; f += 64) carry[f] = J;
        }
        const bool beyond = ok && j == n - 1 && ej < n;
        if (__any(beyond)) {
            const int l = __ffsll((unsigned long long)__ballot(beyond)) - 1;
            const int64_t e2 = __shfl(ej, l, 64);
            for (int64_t f = (e2 + kPartPer - 1) / kPartPer + lane; f * kPartPer < n; f += 64)
                carry[f] = (int32_t)n;
        }
        sj = ej;
    }
    PROBE_MAX(7);
}

// the last block of pass A: block-total scans, then place + fold; HAND (the
// merged launch): and the hand-off to the waiting blocks -- false if this
// block's own record could not be formed
template <int kC, bool HAND = false>
__device__ __forceinline__ bool lean_last_block(uint64_t* __restrict__ bk, int32_t* __restrict__ bf,
                                                uint64_t* __restrict__ boffk,
                                                int32_t* __restrict__ bofff,
                                                uint64_t* __restrict__ ktot,
                                                int32_t* __restrict__ nspec, const int nblocks,
                                                const SpecialIn* __restrict__ stage,
                                                const int64_t n, SpecialOut* __restrict__ spec_out,
                                                int32_t* __restrict__ flags,
                                                const double* __restrict__ w_un,
                                                const double* __restrict__ s_in,
                                                const double np_recip, double* __restrict__ c,
                                                uint64_t* __restrict__ hand = nullptr,
                                                uint64_t* __restrict__ spec_tag = nullptr,
                                                const uint32_t epoch = 0,
                                                uint32_t* __restrict__ s_rec = nullptr) {
    __shared__ uint64_t shk[kScanThreads / 64 + 1];
    __shared__ int32_t shf[kScanThreads / 64 + 1];
    constexpr int kTiles = HAND ? kFoldTilesHand : kFoldTilesLds;
    __shared__ int32_t s_off[kTiles];
    bool go = true;
    PROBE_AT(1);
    if constexpr (!HAND) {
        block_scan_pair<kScanThreads, kC>(bk, boffk, ktot, bf, bofff, nspec, nblocks, shk, shf,
                                      nblocks <= kTiles ? s_off : nullptr);
        __syncthreads();
        PROBE_AT(2);
        const bool bad = lean_place_fold(stage, boffk, bofff, nblocks, ld_wt_i(nspec), ld_wt(ktot),
                                         n, spec_out, flags, s_off, kTiles);
        PROBE_AT(4);
        lean_fold_finish(bad, n, flags, w_un, s_in, np_recip, c);
    } else {
        // the merged launch: the scan leaves every block's offsets in its
        // hand-off record (they travel while the fold runs), the fold the
        // specials as tagged granules, and the verdict goes to the replicas;
        // this block's own nine words come from LDS (a special beyond the
        // LDS copies: through its tags)
        __shared__ uint64_t s_offk[kTiles];
        __shared__ SpecialOut s_so[kFoldSpecLds];
        const bool in_lds = nblocks <= kTiles;
        block_scan_pair<kScanThreads, kC>(bk, boffk, ktot, bf, bofff, nspec, nblocks, shk, shf,
                                      in_lds ? s_off : nullptr, in_lds ? s_offk : nullptr, true);
        __syncthreads();
        PROBE_AT(2);
        const bool bad = lean_place_fold(stage, boffk, bofff, nblocks, ld_wt_i(nspec), ld_wt(ktot),
                                         n, spec_out, flags, s_off, kTiles, s_offk, spec_tag, epoch,
                                         s_so, hand);
        PROBE_AT(4);
        if (threadIdx.x < kHandReplicas)
            st_granule(hand + (int64_t)(nblocks + threadIdx.x) * kHandGranules, bad ? 1u : 0u, epoch);
        bool lost = false;
        if (threadIdx.x == 0) {
            const int b = (int)blockIdx.x;
            const uint64_t k = in_lds ? s_offk[b] : ld_wt(&boffk[b]);
            const int32_t f = in_lds ? s_off[b] : ld_wt_i(&bofff[b]);
            const int32_t m = f > 0 ? f - 1 : 0;
            const SpecialOut p = m < kFoldSpecLds ? s_so[m] : ld_spec_tagged(spec_tag, m, epoch, lost);
            const uint64_t cs = (uint64_t)__double_as_longlong(p.cs);
            s_rec[kHandK0] = (uint32_t)k;
            s_rec[kHandK1] = (uint32_t)(k >> 32);
            s_rec[kHandF] = (uint32_t)f;
            s_rec[kHandCs0] = (uint32_t)cs;
            s_rec[kHandCs1] = (uint32_t)(cs >> 32);
            s_rec[kHandP0] = (uint32_t)p.P;
            s_rec[kHandP1] = (uint32_t)(p.P >> 32);
            s_rec[kHandE] = (uint32_t)p.E;
            s_rec[kHandFallback] = bad ? 1u : 0u;
        }
        go = !__syncthreads_or(lost);
        lean_fold_finish(bad, n, flags, w_un, s_in, np_recip, c);
    }
    return go;
}

// A stand-alone exact cumsum's run marks retired (pf_api.hip retire_scan_marks)
__global__ void mark_gen_bump_kernel(int32_t* __restrict__ flags) {
    flags[kFlagMarkGen] = flags[kFlagMarkGen] + 1;
}

// Pass A (two-launch form): classify and stage every tile; the last block
// scans the tile totals, places and folds.  (A grid-stride form over the
// co-resident blocks measured slower: 50 + 57 against 45 + 45 us at 2^23 --
// the passes are VALU-bound and the loop raised their VGPRs, 5 waves/SIMD.)
__global__ __launch_bounds__(kScanThreads) void scan_lean_classify_kernel(
    const double* __restrict__ w_un, const double* __restrict__ s_in, const double np_recip,
    const int64_t n, const double* __restrict__ boff, const double delta,
    SpecialIn* __restrict__ stage, uint64_t* __restrict__ bk, int32_t* __restrict__ bf,
    uint64_t* __restrict__ boffk, int32_t* __restrict__ bofff, uint64_t* __restrict__ ktot,
    int32_t* __restrict__ nspec, unsigned* __restrict__ counter, int32_t* __restrict__ flags,
    const int32_t force, SpecialOut* __restrict__ spec_out, double* __restrict__ c,
    const int ntiles) {
    if (!force && flags[kFlagResample] != 1) return;
    if (blockIdx.x == 0) PROBE_AT(0);
    const int64_t tile = (int64_t)blockIdx.x * kTilesPerBlock + (threadIdx.x >> 6);
    TileScan ts;
    uint64_t ktile = 0, kofs, kblk;
    int32_t ftile = 0, fofs, fblk;
    if (tile < ntiles)
        wave_tile_classify(w_un, *s_in, np_recip, n, tile, boff[tile], delta, ts, ktile, ftile);
    block_tile_offsets(ktile, ftile, kofs, fofs, kblk, fblk);
    if (tile < ntiles) wave_tile_stage(blockIdx.x, tile, ts, kofs, fofs, kblk, fblk, stage, bk, bf);
    else if (threadIdx.x == 0) {
        st_wt(&bk[blockIdx.x], kblk);
        st_wt_i(&bf[blockIdx.x], fblk);
    }
    PROBE_MAX(12);
    if (!arrive_last(counter)) return;
    lean_last_block<8>(bk, bf, boffk, bofff, ktot, nspec, (int)gridDim.x, stage, n, spec_out,
                       flags, w_un, s_in, np_recip, c);
}

// Pass C (two-launch form): the identical classification, then the expansion.
__global__ __launch_bounds__(kScanThreads) void scan_lean_expand_kernel(
    const double* __restrict__ w_un, const double* __restrict__ s_in, const double np_recip,
    const int64_t n, const double* __restrict__ boff, const double delta,
    const uint64_t* __restrict__ boffk, const int32_t* __restrict__ bofff,
    const SpecialOut* __restrict__ so, double* __restrict__ c, const int32_t* __restrict__ flags,
    const int32_t force, const StepIO io, const PredictConst pc, const uint64_t seed,
    int64_t* __restrict__ mark, int32_t* __restrict__ carry, const int ntiles) {
    if (!force && flags[kFlagResample] != 1) return;
    if (flags[kFlagFallback]) return;
    if (blockIdx.x == 0) PROBE_AT(5);
    const int64_t tile = (int64_t)blockIdx.x * kTilesPerBlock + (threadIdx.x >> 6);
    const double ofs = mark ? resample_offset(io.ofs[io.ctr[0]], pc.np_recip, seed, (uint32_t)io.ctr[1]) : 0.0;
    const int64_t gen = (int64_t)(uint32_t)flags[kFlagMarkGen] << 32;
    TileScan ts;
    uint64_t ktile = 0, kofs, kblk;
    int32_t ftile = 0, fofs, fblk;
    if (tile < ntiles)
        wave_tile_classify(w_un, *s_in, np_recip, n, tile, boff[tile], delta, ts, ktile, ftile);
    block_tile_offsets(ktile, ftile, kofs, fofs, kblk, fblk);
    PROBE_MAX(9);
    if (tile < ntiles)
        wave_tile_expand(tile, ts, n, boffk[blockIdx.x], bofff[blockIdx.x], kofs, fofs, SoPlain{so},
                         nullptr, c, mark, carry, ofs, gen, pc,
                         force != 0 || !mark);                        // (device-decided: marks only)
}

// Passes A and C in ONE launch (NP up to the co-resident grid, checked on the
// host): classify and stage; the last block scans, places and folds, and what
// the waiting blocks need of that reaches them as tagged granules
// (pf_kernels.hpp): a block's offsets on its own line, the folded specials, the
// fold's verdict in replicas -- polled by a few lanes of the block's wave 0,
// with no fence on either side and no load behind the hand-off that is not
// itself tagged; the blocks waited with their tiles' classification still in
// registers, and every wave expands its tile.  The epoch is the token word + 1, read by every block
// before it arrives and advanced by the last block, so that no record or
// special of an earlier launch carries it.  The wait is bounded: a record that
// never arrives sets status bit 3 and the block skips its expansion instead of
// hanging the device.
__global__ __launch_bounds__(kScanThreads) void scan_lean_merged_kernel(
    const double* __restrict__ w_un, const double* __restrict__ s_in, const double np_recip,
    const int64_t n, const double* __restrict__ boff, const double delta,
    SpecialIn* __restrict__ stage, uint64_t* __restrict__ bk, int32_t* __restrict__ bf,
    uint64_t* __restrict__ boffk, int32_t* __restrict__ bofff, uint64_t* __restrict__ ktot,
    int32_t* __restrict__ nspec, unsigned* __restrict__ counter, int32_t* __restrict__ flags,
    const int32_t force, SpecialOut* __restrict__ spec_out, double* __restrict__ c,
    const StepIO io, const PredictConst pc, const uint64_t seed, int64_t* __restrict__ mark,
    int32_t* __restrict__ carry, int32_t* __restrict__ token_word, uint64_t* __restrict__ hand,
    uint64_t* __restrict__ spec_tag, const int ntiles) {
    if (!force && flags[kFlagResample] != 1) return;
    __shared__ int s_go;
    __shared__ uint32_t s_rec[kHandUsed];
    static_assert(kHandK1 == kHandK0 + 1 && kHandF == kHandK0 + 2 && kHandE == kHandCs0 + 4 &&
                      kHandFallback == kHandCs0 + kSpecGranules,
                  "the poll's lanes map onto HandWord in order");
    if (blockIdx.x == 0) PROBE_AT(0);
    const int32_t token = ld_wt_i(token_word) + 1;     // read before this block arrives
    const uint32_t epoch = (uint32_t)token;
    const double ofs = resample_offset(io.ofs[io.ctr[0]], pc.np_recip, seed, (uint32_t)io.ctr[1]);
    const int64_t gen = (int64_t)(uint32_t)flags[kFlagMarkGen] << 32;
    const int64_t tile = (int64_t)blockIdx.x * kTilesPerBlock + (threadIdx.x >> 6);
    const bool active = tile < ntiles;
    TileScan ts;
    uint64_t ktile = 0, kofs, kblk;
    int32_t ftile = 0, fofs, fblk;
    if (active)
        wave_tile_classify(w_un, *s_in, np_recip, n, tile, boff[tile], delta, ts, ktile, ftile);
    block_tile_offsets(ktile, ftile, kofs, fofs, kblk, fblk);
    if (active) wave_tile_stage(blockIdx.x, tile, ts, kofs, fofs, kblk, fblk, stage, bk, bf);
    else if (threadIdx.x == 0) {
        st_wt(&bk[blockIdx.x], kblk);
        st_wt_i(&bf[blockIdx.x], fblk);
    }
    PROBE_MAX(12);
    if (arrive_last(counter)) {
        const bool go = lean_last_block<4, true>(bk, bf, boffk, bofff, ktot, nspec, (int)gridDim.x,
                                                 stage, n, spec_out, flags, w_un, s_in, np_recip, c,
                                                 hand, spec_tag, epoch, s_rec);
        if (threadIdx.x == 0) {
            st_wt_i(token_word, token);               // the next launch's epoch differs
            if (!go) atomicOr(&flags[kFlagStatus], 8);
            s_go = go;
        }
    } else if (threadIdx.x < 64) {
        // wave 0 gathers the block's nine words: lanes 0..2 its own record's
        // offsets (there long before the fold ends), then lanes 0..4 the
        // special before the block and lane 5 the verdict (its replica)
        const uint64_t* rec = hand + (int64_t)blockIdx.x * kHandGranules;
        const int lane = threadIdx.x;
        uint64_t g = 0;
        int go = 0, it = 0;
        for (; it < kHandSpin; ++it) {
            if (lane < 3) g = ld_wt(rec + lane);
            if (__all(lane >= 3 || (uint32_t)(g >> 32) == epoch)) {
                go = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (lane < 3) s_rec[kHandK0 + lane] = (uint32_t)g;
        const int32_t bfb = __builtin_amdgcn_readlane((int32_t)(uint32_t)g, kHandF);
        const int64_t m0 = bfb > 0 ? bfb - 1 : 0;
        const uint64_t* src = lane < kSpecGranules
                                  ? spec_tag + m0 * kSpecGranules + lane
                                  : hand + (int64_t)(gridDim.x + blockIdx.x % kHandReplicas) * kHandGranules;
        if (go) {
            go = 0;
            for (; it < kHandSpin; ++it) {
                if (lane <= kSpecGranules) g = ld_wt(src);
                if (__all(lane > kSpecGranules || (uint32_t)(g >> 32) == epoch)) {
                    go = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        if (lane <= kSpecGranules) s_rec[kHandCs0 + lane] = (uint32_t)g;
        if (lane == 0) {
            if (!go) atomicOr(&flags[kFlagStatus], 8);   // never came: skip, do not hang
            s_go = go;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0) PROBE_AT(5);
    if (!active || !s_go || s_rec[kHandFallback]) return;
    const uint64_t bkb = ((uint64_t)s_rec[kHandK1] << 32) | s_rec[kHandK0];
    const int32_t bfb = (int32_t)s_rec[kHandF];
    SoTagged so;
    so.tag = spec_tag;
    so.epoch = epoch;
    so.m0 = bfb > 0 ? bfb - 1 : 0;
    so.p0.cs = __longlong_as_double((long long)(((uint64_t)s_rec[kHandCs1] << 32) | s_rec[kHandCs0]));
    so.p0.P = ((uint64_t)s_rec[kHandP1] << 32) | s_rec[kHandP0];
    so.p0.E = (int32_t)s_rec[kHandE];
    so.p0.pad = 0;
    wave_tile_expand(tile, ts, n, bkb, bfb, kofs, fofs, so, flags, c, mark, carry, ofs, gen, pc,
                     force != 0);
}

// gather for the stand-alone resampling stage (particle_filter.py:216-222)
__global__ __launch_bounds__(256) void gather_kernel(
    const int64_t n, const int32_t* __restrict__ idx, const double* __restrict__ xs,
    const double* __restrict__ ys, const double* __restrict__ ts, double* __restrict__ xo,
    double* __restrict__ yo, double* __restrict__ to, double* __restrict__ w, const double np_recip) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = idx[i];
    xo[i] = xs[j];
    yo[i] = ys[j];
    to[i] = ts[j];
    w[i] = np_recip;
}

// stand-alone systematic positions + lower_bound (particle_filter.py:213-221)
__global__ __launch_bounds__(256) void resample_search_kernel(
    const int64_t n, const double* __restrict__ c, int32_t* __restrict__ idx, const double step,
    const double ofs_host, const double np_recip, const uint64_t seed, const uint32_t stepno,
    int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double ofs = resample_offset(ofs_host, np_recip, seed, stepno);
    const double pos = (double)i * step + ofs;
    int64_t lo = lower_bound_c(c, n, pos);
    if (lo >= n) {
        lo = n - 1;
        atomicOr(&flags[kFlagStatus], 1);
    }
    idx[i] = (int32_t)lo;
}

}  // namespace slam
