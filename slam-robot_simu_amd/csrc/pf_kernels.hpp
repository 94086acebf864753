// pf_kernels.hpp -- particle-filter kernel interfaces (device side).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <vector>

#include "common.hpp"

namespace slam {

constexpr int kMotionNone = 2;     // internal: likelihood-only pass

// Per-step closed-form words of the iso log-sum likelihood (StepIO.zc, one
// slot of kZcWords doubles per step), formed on the device at the start of
// every step (closed_prep_*):
//  * kZcSum + 2k, k < 8: S_ll, S_lx, S_ly, S_zz, S_zx, S_zy, D, E as
//    double-double (hi, lo) pairs -- the sums of landmarks / observations of
//    the step (the double-double form of likelihood_lanes);
//  * the expansion about the step's reference pose (p^, c^, s^): F^ = the
//    exact sum of squared residuals at it, A, B (gradient in the rotation)
//    and L2 (landmark second moment about p^) as double-doubles (hi, lo),
//    S_r (residual sum) and L1 (landmark sum about p^) rounded.
enum : int {
    kZcSum = 0,
    kZcPx = 16, kZcPy, kZcC, kZcS,
    kZcFh, kZcFl, kZcA, kZcAl, kZcB, kZcBl, kZcL2, kZcL2l,
    kZcSrx, kZcSry, kZcL1x, kZcL1y,
    kZcWords = 40,
};
constexpr int kClosedWords = kZcWords;
constexpr int kSumChunk = 8192;     // np.sum buffer size (particle_filter.py:234 order)
constexpr int kScanBlock = 2048;    // elements per block of the exact-cumsum passes
constexpr int kScanThreads = 256;
constexpr int kScanPer = kScanBlock / kScanThreads;  // 8
#ifndef SLAM_DEFER_PPT
#define SLAM_DEFER_PPT 2
#endif
constexpr int kDeferPPT = SLAM_DEFER_PPT;            // particles per lane of the fused kernel
constexpr int kPartPer = 256 * kDeferPPT;            // particles per fused block

// Deferred normalisation (every handle): the fused kernel leaves, per
// kPartPer-particle block, its max unnormalised weight M_b with the first index,
// sums scaled by 1/M_b (sum u, sum u^2, sum u d, sum u d d^T with u = w_un/M_b
// and d = particle - refp; scaling keeps squares of tiny likelihoods out of
// the subnormal range) and its np.sum subtree (the pairwise sum of its four
// 128-element leaves).
// Per block also: the largest w_un before the first max (-1 if none), so
// the step end knows without a rescan whether a smaller weight can round to
// the same normalised maximum, and the particle at the first max (x_est).
// The 18 per-block arrays are one slab: array j starts at slab + j stride
// (8-byte entries; stride a multiple of 16, so every array starts on a
// 128-byte line, and at least blocks + 1: the step end loads entry pairs).
// A kernel then carries one pointer and the stride for all of them, which
// keeps the fused kernel's scalar registers free.
constexpr int kDeferArrays = 18;    // pmax, pidx, ppre, pxe[3], ps[11], leaf (the last)
struct DeferParts {
    double* slab;
    int64_t stride;
    __host__ __device__ double* arr(const int j) const { return slab + j * stride; }
    __host__ __device__ double* pmax() const { return arr(0); }
    __host__ __device__ int64_t* pidx() const { return reinterpret_cast<int64_t*>(arr(1)); }
    // max w_un at indices before pidx (-1: none)
    __host__ __device__ double* ppre() const { return arr(2); }
    // particle (x, y, th) at pidx
    __host__ __device__ double* pxe(const int j) const { return arr(3 + j); }
    // sw, sw2, m1[3], m2[6]
    __host__ __device__ double* ps(const int j) const { return arr(6 + j); }
    // [blocks] the block's np.sum subtree (its kPartPer / 128 leaves, pairwise)
    __host__ __device__ double* leaf() const { return arr(kDeferArrays - 1); }
    int64_t* mark;         // [npad] resample-run starts: (RNG step << 32) | source (expand pass)
    int32_t* carry;         // [blocks] source of each fused block's first position
    // the resample gather reads source v at (x - goff)[v]: 0 on single-GPU
    // handles; npad on a sharded handle, whose particle arrays carry npad
    // staging slots on either side (particles received from lower ranks at
    // v = p, its own at npad + j, from higher ranks at 2 npad + p, so the
    // running max over a block's marks stays monotone)
    int64_t goff;
    int64_t glim;           // sources >= glim: the reference's IndexError (n; 3 npad when sharded)
};

// particle_filter.py:179-181 + the mlab.bivariate_normal constants
struct LikConst {
    double sx2, sy2;        // sigmax**2, sigmay**2 (as numpy squares the sqrt)
    double rsx2, rsy2;      // RN(1/sx2), RN(1/sy2) for the FMA-refined quotients
    double rho2;            // 2*rho
    double sxsy;            // sigmax*sigmay
    double d2;              // 2*(1-rho**2)
    double den, rden;       // 2*pi*sx*sy*sqrt(1-rho**2) and RN(1/den)
    double neg_nl_ln_den;   // -NL*log(den) (log-sum form)
    double rsxsy, rd2;      // RN(1/(sx*sy)), RN(1/d2) (log-sum form)
    double fast_min_l;      // log-sum form: L >= this -> exp(L); below, logsum_slow
                            // (every partial product provably stays normal above it)
    double normal_min_l;    // ln(DBL_MIN) + 1: a log prefix above it is a normal partial product
    double neg_ln_den;      // -log(den): log-prefix increment per landmark
    double expand_vmax;     // closed form: the expansion about the step's reference
                            // pose is taken when the particle's bound V <= this
                            // (|dL| <= 1e-14); beyond it the double-double form
    int32_t has_rho;
    int32_t iso;            // sx2 == sy2 and rho == 0 (log-sum shortcut)
    int32_t nl;
    int32_t closed;         // iso log-sum from the per-step landmark/observation sums (StepIO.zc)
};

struct PredictConst {
    double dt;
    double alphas[6];       // motion_model.py:20-29 a1..a6
    double q[9];            // device-RNG noise map for the linear model
    double np_recip;        // 1/NP (particle_filter.py:32), NP = global particle count
    double rstep;           // arange step 1/NP (particle_filter.py:213)
    int64_t n_global;       // global particle count (RNG counter space)
    int64_t gbase;          // global index of local particle 0
};

// Device-resident per-step inputs/outputs of a loaded batch.  Kernels read the
// step index from ctr[0] (advanced by the step end, pf_finalize.inl), so
// one captured step graph replays unchanged for every step.
struct StepIO {
    const double* ctl;      // [cap][2] control (v, omega)
    const double* z;        // [cap][2*NL] robot-frame observations
    double* zc;             // [cap][kZcWords] closed-form words (formed on the device per step)
    const double* ofs;      // [cap] host resample offset (NaN: device RNG)
    slam_pf_result* res;    // [cap] result records
    slam_pf_result* res_host;   // [cap] coherent pinned copy (device address): the last step of
                                // a device-resident batch stores the batch's records there
    int32_t* ctr;           // [0] step within the batch, [1] global RNG step, [2] / [3] the
                            // batch's first / last step (slam_pf_run's setup)
    int32_t cap;            // steps the arrays hold (the step end prepares step ctr[0] + 1 < cap)
    int32_t motion;         // the handle's motion model (reference pose of the expansion)
    double ess_band;        // result.ess_near: |ess - ESS_TH| <= ess_band * ESS_TH
};

struct BlockPartial {
    double maxv;
    int64_t maxi;
    double sw, sw2;
    double m1[3];
    double m2[6];
};

// The record's weighted covariance from the combined moments (sw = sum w,
// m1 = sum w d, m2 = sum w d d^T, upper triangle): one expression for the
// step end and for the host, which completes the records of a batch's split
// step ends (both built with -ffp-contract=off: the same bits).
__host__ __device__ inline void cov_from_moments(const double sw, const double (&m1)[3],
                                                 const double (&m2s)[6], double* cov) {
    const double inv = 1.0 / sw;
    const double mu[3] = {m1[0] * inv, m1[1] * inv, m1[2] * inv};
    const double m2[9] = {m2s[0], m2s[1], m2s[2], m2s[1], m2s[3], m2s[4], m2s[2], m2s[4], m2s[5]};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) cov[3 * a + b] = m2[3 * a + b] * inv - mu[a] * mu[b];
}

// The moments from the step end's totals relative to the global max M
// (tot[0] sum u, tot[2..4] sum u d, tot[5..10] sum u d d^T, u = w_un / M):
// f = M / s, the record's max_val, brings them back to w = w_un / s.
__host__ __device__ inline void moments_from_totals(const double* tot, const double f, double& sw,
                                                    double (&m1)[3], double (&m2)[6]) {
    sw = tot[0] * f;
    for (int j = 0; j < 3; ++j) m1[j] = tot[2 + j] * f;
    for (int j = 0; j < 6; ++j) m2[j] = tot[5 + j] * f;
}

__host__ __device__ inline void cov_from_totals(const double* tot, const double f, double* cov) {
    double sw, m1[3], m2[6];
    moments_from_totals(tot, f, sw, m1, m2);
    cov_from_moments(sw, m1, m2, cov);
}

// Per-step raw totals of a split step end (finalize_fast_kernel<false>,
// pf_finalize.inl), a step-indexed sibling of StepIO.res: workgroup 0 stores
// tot[0..1] and the state, the moment workgroups tot[2..10].  pending: the
// record's cov is cov_from_totals(tot, record.max_val); complete: the record
// holds its cov already (a full or degenerate step end), tot is not read.
enum : int32_t { kMomComplete = 0, kMomPending = 1 };
struct FinMoments {
    double tot[11];
    int32_t state, pad;
};
static_assert(sizeof(FinMoments) % 8 == 0, "moment entries move as 8-byte words");

// What the finalize launch carries besides StepIO (which the fused kernel
// shares and which therefore stays as it is)
struct FinSplit {
    FinMoments* mom;        // [cap] device entries
    FinMoments* mom_host;   // [cap] coherent pinned copy (device address), beside StepIO.res_host
    int32_t par;            // ping-pong parity of the step: the moment workgroups read the
                            // step from ctr[4 + par], workgroup 0 leaves the next one in
                            // ctr[4 + (1 - par)] (no word read and written in one launch)
    int32_t full;           // a stepwise launch: always the full path
};

// ctr words beyond StepIO's four: the step as the moment workgroups read it
constexpr int kCtrMom = 4;
constexpr int kCtrWords = 6;

struct SpecialIn {
    int64_t idx;            // global element index
    uint64_t P;             // inclusive prefix of the integer increments
    double w;
    int32_t E;              // binade of the run that follows
    int32_t pad;
};

struct SpecialOut {
    double cs;              // exact cumsum at the special element
    uint64_t P;
    int32_t E;
    int32_t pad;
};

// Hand-off of the merged exact-cumsum launch: everything its last
// block hands to the waiting blocks travels as naturally aligned 8-byte
// granules {payload (low word), epoch tag (high word)}, each written by one
// write-through store and read by write-through loads until its tag is the
// launch's epoch.  One record per block on a 128-byte line of its own holds
// the block's global offsets (written by the tile-total scan, so they travel
// while the fold runs); the folded specials are kSpecGranules granules each;
// the fold's verdict is one granule in each of kHandReplicas further lines
// (block b polls replica b % kHandReplicas: few pollers per word).  A waiting
// block gathers from these the nine words of HandWord in LDS.
constexpr int kHandGranules = 16;   // granules per record: one 128-byte line
constexpr int kHandReplicas = 32;
enum HandWord {
    kHandK0 = 0,            // boffk[b], low / high half    (record granules 0, 1)
    kHandK1 = 1,
    kHandF = 2,             // bofff[b]                     (record granule 2)
    kHandCs0 = 3,           // folded special bofff[b] - 1 (0 for the first block): cs halves,
    kHandCs1 = 4,
    kHandP0 = 5,            // P halves,
    kHandP1 = 6,
    kHandE = 7,             // E
    kHandFallback = 8,      // the fold fell back to the sequential recurrence
    kHandUsed = 9,
};
constexpr int kSpecGranules = 5;    // cs halves, P halves, E
constexpr int kHandSpin = 1 << 22;  // bounded wait (polls) before a block gives up

// LikConst of a filter from R (row-major 2x2) and the landmark count; allow_closed:
// the handle can form the per-step closed-form words (StepIO.zc).
inline int lik_const_from(const double* R, const int32_t nl, const bool allow_closed, LikConst& lc) {
    // particle_filter.py:179-181 and the bivariate_normal constants, in numpy's order
    const double sx = std::sqrt(R[0]), sy = std::sqrt(R[3]), sxy = std::sqrt(R[1]);
    if (!(sx > 0) || !(sy > 0) || std::isnan(sxy))
        return fail(SLAM_ERR_ARG, "r_cov: need R00 > 0, R11 > 0, R01 >= 0");
    const double rho = sxy / (sx * sy);
    lc.sx2 = sx * sx;
    lc.sy2 = sy * sy;
    lc.rsx2 = 1.0 / lc.sx2;
    lc.rsy2 = 1.0 / lc.sy2;
    lc.rho2 = 2 * rho;
    lc.sxsy = sx * sy;
    lc.d2 = 2 * (1 - rho * rho);
    lc.den = 2 * kPi * sx * sy * std::sqrt(1 - rho * rho);
    lc.rden = 1.0 / lc.den;
    lc.nl = nl;
    lc.neg_nl_ln_den = -(double)nl * std::log(lc.den);
    lc.has_rho = (rho != 0.0) ? 1 : 0;
    lc.rsxsy = 1.0 / lc.sxsy;
    lc.rd2 = 1.0 / lc.d2;
    lc.iso = (lc.sx2 == lc.sy2 && !lc.has_rho) ? 1 : 0;
    // closed-form log-sum (iso, NL > 0); SLAM_PF_CLOSED=0 keeps the landmark loop (diagnostic)
    const char* ce = std::getenv("SLAM_PF_CLOSED");
    lc.closed = (allow_closed && lc.iso && nl > 0 && !(ce && ce[0] == '0')) ? 1 : 0;
    // Log-sum fast-path bound.  A factor is at most 1/den (q >= 0), so the log of
    // the reference's partial product after landmark k is at least
    // L - (NL - k) max(0, -ln den).  L >= ln(DBL_MIN) + NL max(0, -ln den) + 1
    // keeps every partial product of particle_filter.py:192 in the normal range
    // (the 1-nat margin covers the rounding of both sums); below it the kernel
    // takes the reference's sequential product.  Past NL max(0, -ln den) = 700
    // the products may overflow: always the sequential product.
    const double climb = (double)nl * std::max(0.0, -std::log(lc.den));
    lc.normal_min_l = std::log(std::numeric_limits<double>::min()) + 1.0;
    lc.neg_ln_den = -std::log(lc.den);
    lc.fast_min_l = climb > 700.0 ? std::numeric_limits<double>::infinity()
                                  : lc.normal_min_l + climb;
    // closed form: the fp64 expansion while its rounding bound 11 u V stays
    // within |dL| <= 3e-13 (dL = dF / (2 sx2), under a third of the 1e-12
    // parity bar): V rsx2 <= 480; SLAM_PF_EXPAND_VMAX=<factor>
    // scales the bound (0: double-double only)
    const char* ve = std::getenv("SLAM_PF_EXPAND_VMAX");
    const double vf = ve ? std::atof(ve) : 1.0;
    lc.expand_vmax = vf * 480.0 * lc.sx2;
    return SLAM_OK;
}

// device flag words
enum : int {
    kFlagResample = 0,      // resample at the start of the next step (ESS < ESS_TH)
    kFlagStatus = 1,        // bit0 clamp (reference IndexError), bit1 scan fallback
    kFlagNSpecial = 2,
    kFlagFallback = 3,
    kFlagMarkGen = 4,       // tag of the resample-run marks, advanced by every step end
    kFlagScanToken = 5,     // release token of the merged exact-cumsum launch
    kFlagDistDead = 6,      // sharded step: a peer wait expired once (sticky: later waits are skipped)
    kFlagDDWaves = 7,       // closed form: wavefronts of this step that took the double-double form
    kFlagWords = 8,
};

// Closed-form log-sum sums of one step (likelihood_lanes, iso): S_ll = sum |l|^2,
// S_l = sum l, S_zz = sum |z|^2, S_z = sum z, D = sum z.l, E = sum (z_y l_x - z_x l_y),
// each a double-double (hi, lo) -- exact products, compensated sums.  The same
// operations on the host (observations loaded from the caller) and on the
// device (observations simulated there).
struct DDSum {
    double h = 0.0, l = 0.0;
    __host__ __device__ void add(const double bh, const double bl = 0.0) {
        const double t = h + bh;
        const double bb = t - h;
        const double e = ((h - (t - bb)) + (bh - bb)) + (l + bl);
        h = t + e;
        l = e - (h - t);
    }
    __host__ __device__ void add_prod(const double a, const double b) {
        const double p = a * b;
        add(p, fma(a, b, -p));
    }
};

// DDSum of two double-double partials (the second added as (h, l))
__host__ __device__ inline DDSum dd_join(DDSum a, const DDSum& b) {
    a.add(b.h, b.l);
    return a;
}

// component k (0 S_ll, 1 S_lx, 2 S_ly, 3 S_zz, 4 S_zx, 5 S_zy, 6 D, 7 E) of
// landmark j's terms, added to S
__host__ __device__ inline void closed_term(DDSum& S, const int k, const double lx, const double ly,
                                            const double zx, const double zy) {
    switch (k) {
        case 0: S.add_prod(lx, lx); S.add_prod(ly, ly); break;
        case 1: S.add(lx); break;
        case 2: S.add(ly); break;
        case 3: S.add_prod(zx, zx); S.add_prod(zy, zy); break;
        case 4: S.add(zx); break;
        case 5: S.add(zy); break;
        case 6: S.add_prod(zx, lx); S.add_prod(zy, ly); break;
        default: S.add_prod(zy, lx); S.add_prod(-zx, ly); break;
    }
}

// The fixed summation order, shared by host and device: 64 lane partials
// (lane t takes landmarks t, t + 64, ... in order), then a butterfly over the
// lanes (offset 1, 2, ..., 32; the lower lane's partial on the left).
constexpr int kClosedLanes = 64;

__host__ __device__ inline DDSum closed_lane_partial(const int k, const int lane, const double* lm,
                                                     const double* z, const int32_t nl) {
    DDSum S;
    for (int32_t j = lane; j < nl; j += kClosedLanes)
        closed_term(S, k, lm[2 * j], lm[2 * j + 1], z[2 * j], z[2 * j + 1]);
    return S;
}

// numpy's pairwise-sum split of n elements from lo (one np.sum buffer, n <=
// kSumChunk): leaves (lo, count) of at most 128 elements + the post-order
// program that adds them (a leaf's index, or -1: add the two on top)
inline void pairwise_sum_split(int lo, int n, std::vector<int32_t>& leaves, std::vector<int32_t>& ops) {
    if (n <= 128) {
        ops.push_back((int32_t)(leaves.size() / 2));
        leaves.push_back(lo);
        leaves.push_back(n);
        return;
    }
    int h = n / 2;
    h -= h % 8;
    pairwise_sum_split(lo, h, leaves, ops);
    pairwise_sum_split(lo + h, n - h, leaves, ops);
    ops.push_back(-1);
}

}  // namespace slam
