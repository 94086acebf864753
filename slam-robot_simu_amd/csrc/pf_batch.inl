// pf_batch.inl -- gfx950 kernels of the particle-filter ensemble (included by
// pf_batch_api.hip): B independent filters of NP <= 8192 particles each, one
// workgroup per filter, the whole estimator step of main_pf
// (particle_filter.py:102-117) inside the block and a run of n_steps as a loop
// in the block -- filters never talk to each other, so there is no grid-level
// hand-off (no tickets, tokens or release fences) and a run is one launch.
//
// Residency: particle state (x, y, th ping-pong), the unnormalised weights and
// the exact-cumsum scratch of filter b are rows [b][NPpad] in HBM (a filter's
// working set, 7 rows of NPpad doubles, stays in L2); LDS holds the filter's
// landmarks and the step's observations, the RNG / exp tables and the
// reductions' scratch.  Lane t of a pass holds the particle pair 512 p + 2 t
// (16-byte accesses, one device-RNG pair per lane), as the single handle's
// fused kernel does -- the per-particle arithmetic is that kernel's
// (predict_particle, likelihood_lanes), so a member is bit-identical to a
// stand-alone slam_pf with the same seed.
#include "pf_device.inl"

namespace slam {

constexpr int kPfbThreads = 256;
constexpr int kPfbTile = 2 * kPfbThreads;     // particles per pass of the block
constexpr int kPfbMaxN = kSumChunk;           // one np.sum buffer
constexpr int kPfbMaxLeaves = 160;            // leaves of the np.sum tree of n <= 8192 (<= 128 + splits)
constexpr int kPfbLdsNl = 1024;               // landmarks / observations staged in LDS up to this NL

// per-filter constants
struct PfbFilter {
    LikConst lc;
    PredictConst pc;
    uint64_t seed;
    double ess_th;
};

// a special element of the exact cumsum (ties, binade crossings, element 0);
// the fold replaces w by the exact cumulative weight at the element
struct PfbSpecial {
    int32_t idx;
    int32_t E;              // binade of the run that follows
    uint64_t P;             // inclusive prefix of the integer increments
    double w;
};

struct PfbArgs {
    int32_t B, n, npad, nl;
    double* x[2];           // [B][npad] ping-pong
    double* y[2];
    double* th[2];
    double* w_un;           // [B][npad] weights before normalisation
    double* s_cur;          // [B] their np.sum (current weights = w_un / s_cur)
    uint64_t* c;            // [B][npad] exact cumsum (doubles; integer prefixes while it is formed)
    PfbSpecial* spec;       // [B][n]
    int32_t* flags;         // [B] resample at the start of the next step
    const PfbFilter* filt;  // [B]
    const double* lm;       // [B][nl][2]
    const double* ctl;      // [nsteps][B][2] (the call's steps)
    const double* z;        // [loaded steps][B][nl][2], indexed from `first`
    const double* noise;    // [B][n][3] (host-noise kernels)
    const double* ofs;      // [B] host resample offsets (NaN: device RNG) or NULL
    const int32_t* leaves;  // np.sum tree of n elements: (lo, count) per leaf
    const int32_t* ops;     // post-order program: leaf index, or -1 = add the two on top
    int32_t nleaves, nops;
    slam_pf_result* res;    // [n_steps][B] coherent pinned host memory (device address)
    int32_t first, nsteps;  // steps [first, first + nsteps) of ctl / z
    uint32_t stepno;        // RNG step of the first
    int32_t cur;            // ping-pong parity at the first step
    double ess_band;
};

struct PfbPartial {
    double maxv;
    int32_t maxi;
    double q[11];           // sw, sw2, m1[3], m2[6]
};

// ---- exact sequential np.cumsum of w = w_un / s (particle_filter.py:212) in
// the block: each element classified against an approximate prefix (regular:
// its add moves the running sum by a whole number of ulps of the binade,
// whatever the sum's low bits -- no tie, no binade crossing within the
// margin delta), the integer increments prefix-summed, the specials folded in
// order by one lane with each regular run added as one exact multiple of its
// binade's ulp, then every c_j expanded.  A failed run check takes the plain
// sequential loop (status bit 1), as on the single handle.
__device__ void pfb_exact_cumsum(const double* __restrict__ w_un, const double s,
                                 const double np_recip, const int32_t n, const int32_t npad,
                                 uint64_t* __restrict__ ck, PfbSpecial* __restrict__ spec,
                                 double* shd, uint64_t* shk, int32_t* shf, int32_t* s_info) {
    constexpr uint64_t kSpecialBit = 1ull << 63;
    const int32_t ept = npad / kPfbThreads;
    const int32_t j0 = (int32_t)threadIdx.x * ept;
    const double delta = 4.0 * (double)n * 0x1p-53 + 0x1p-45;
    double loc = 0.0;
    for (int32_t k = 0; k < ept; ++k) {
        const int32_t j = j0 + k;
        loc += (j < n) ? norm_w(w_un[j], s, np_recip) : 0.0;
    }
    double dtot;
    double run = block_excl_scan<double, kPfbThreads>(loc, shd, dtot);
    uint64_t ksum = 0;
    int32_t fsum = 0;
    for (int32_t k = 0; k < ept; ++k) {
        const int32_t j = j0 + k;
        if (j >= n) break;
        const double v = norm_w(w_un[j], s, np_recip);
        const double prev = run;
        run = run + v;
        bool reg = (j != 0);
        uint64_t inc = 0;
        const int E = sum_binade(run);
        if (reg) {
            reg = (sum_binade(prev) == E);
            if (reg && E != -1022) reg = prev >= ldexp(1.0, E) * (1.0 + delta);
            if (reg) reg = run <= ldexp(1.0, E + 1) * (1.0 - delta);
            if (reg) {
                const double tt = ldexp(v, 52 - E);
                const double fl = floor(tt);
                reg = (tt - fl) != 0.5;
                inc = (uint64_t)rint(tt);
            }
        }
        if (reg) {
            ck[j] = inc;
            ksum += inc;
        } else {
            ck[j] = kSpecialBit | (uint64_t)(uint32_t)(E + 2048);
            ++fsum;
        }
    }
    uint64_t ktot;
    int32_t M;
    uint64_t kex = block_excl_scan<uint64_t, kPfbThreads>(ksum, shk, ktot);
    const int32_t fex0 = block_excl_scan<int32_t, kPfbThreads>(fsum, shf, M);
    int32_t fex = fex0;
    for (int32_t k = 0; k < ept; ++k) {
        const int32_t j = j0 + k;
        if (j >= n) break;
        const uint64_t u = ck[j];
        if (u & kSpecialBit) {
            PfbSpecial e;
            e.idx = j;
            e.E = (int32_t)(uint32_t)(u & 0xffffu) - 2048;
            e.P = kex;
            e.w = norm_w(w_un[j], s, np_recip);
            spec[fex++] = e;
        } else {
            kex += u;
            ck[j] = kex;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        bool bad = false;
        for (int32_t m = 0; m < M; ++m) {
            const PfbSpecial e = spec[m];
            r = r + e.w;                                    // the special element's own add
            spec[m].w = r;
            const bool last = (m + 1 >= M);
            const int32_t nxt = last ? n : spec[m + 1].idx;
            if (nxt - e.idx > 1) {                          // the regular run behind it: K ulps, exact
                const uint64_t K = (last ? ktot : spec[m + 1].P) - e.P;
                const int E = e.E;
                if (sum_binade(r) != E) { bad = true; break; }
                const double r2 = r + (double)K * ldexp(1.0, E - 52);
                const double hi = (E == -1022) ? 0x1p-1021 : ldexp(1.0, E + 1);
                if (!(r2 < hi) || (double)K >= 0x1p53) { bad = true; break; }
                r = r2;
            }
        }
        s_info[1] = M;
        s_info[2] = bad ? 1 : 0;
        if (bad) {
            s_info[0] |= 2;
            r = 0.0;
            for (int32_t i = 0; i < n; ++i) {
                r = r + norm_w(w_un[i], s, np_recip);
                ck[i] = (uint64_t)__double_as_longlong(r);
            }
        }
    }
    __syncthreads();
    if (!s_info[2]) {
        int32_t m = fex0;
        PfbSpecial p = spec[m > 0 ? m - 1 : 0];
        for (int32_t k = 0; k < ept; ++k) {
            const int32_t j = j0 + k;
            if (j >= n) break;
            const uint64_t u = ck[j];
            double cj;
            if (u & kSpecialBit) {
                p = spec[m++];
                cj = p.w;
            } else {
                cj = p.w + (double)(u - p.P) * ldexp(1.0, p.E - 52);
            }
            ck[j] = (uint64_t)__double_as_longlong(cj);
        }
    }
    __syncthreads();
}

// ---- s = np.sum(w[0:n]) in NumPy's order (particle_filter.py:234; n <= 8192:
// one pairwise tree): n < 8 the plain loop; else leaves of <= 128 elements,
// eight accumulators each (eight lanes per leaf), combined by the host-built
// post-order program (oracle/pf_oracle.py:_pairwise).
__device__ double pfb_numpy_sum(const double* __restrict__ w, const int32_t n,
                                const int32_t* s_leaves, const int32_t nleaves,
                                const int32_t* s_ops, const int32_t nops, double* s_leaf,
                                double* s_stk) {
    if (n < 8) {
        if (threadIdx.x == 0) {
            double r = 0.0;
            for (int32_t i = 0; i < n; ++i) r += w[i];
            s_stk[0] = r;
        }
    } else {
        const int j = threadIdx.x & 7;
        for (int32_t L = (int32_t)threadIdx.x >> 3; L < nleaves; L += kPfbThreads / 8) {
            const int32_t lo = s_leaves[2 * L], m = s_leaves[2 * L + 1];
            const int32_t stop = m - (m % 8);
            double acc = w[lo + j];
            for (int32_t i = 8; i < stop; i += 8) acc += w[lo + i + j];
            double r = acc + __shfl_xor(acc, 1, 64);        // (a0 + a1), (a2 + a3), ...
            r = r + __shfl_xor(r, 2, 64);
            r = r + __shfl_xor(r, 4, 64);
            if (j == 0) {
                for (int32_t i = stop; i < m; ++i) r += w[lo + i];
                s_leaf[L] = r;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int sp = 0;
            for (int32_t k = 0; k < nops; ++k) {
                const int32_t op = s_ops[k];
                if (op >= 0) {
                    s_stk[sp++] = s_leaf[op];
                } else {
                    const double b = s_stk[--sp];
                    const double a = s_stk[--sp];
                    s_stk[sp++] = a + b;
                }
            }
        }
    }
    __syncthreads();
    const double r = s_stk[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void pfb_merge(PfbPartial& r, const double ov, const int32_t oi,
                                          const double* oq) {
    if (ov > r.maxv || (ov == r.maxv && oi < r.maxi)) {
        r.maxv = ov;
        r.maxi = oi;
    }
#pragma unroll
    for (int k = 0; k < 11; ++k) r.q[k] = r.q[k] + oq[k];
}

// The block's shared scratch (one struct: the run and the indices kernel agree on it)
struct PfbShared {
    double shd[kPfbThreads / 64 + 1];
    uint64_t shk[kPfbThreads / 64 + 1];
    int32_t shf[kPfbThreads / 64 + 1];
    int32_t info[4];                 // [0] status bits, [1] specials, [2] cumsum fallback, [3] next flag
    double leaf[kPfbMaxLeaves];
    double stk[32];
    int32_t leaves[2 * kPfbMaxLeaves];
    int32_t ops[2 * kPfbMaxLeaves];
    PfbPartial part[kPfbThreads / 64];
};

// n_steps estimator steps of filter blockIdx.x (particle_filter.py:102-117)
template <int MOTION, int LIK, bool HOSTNOISE>
__global__ __launch_bounds__(kPfbThreads) void pfb_run_kernel(const PfbArgs a) {
    extern __shared__ double s_dyn[];            // landmarks [2 nl], observations [2 nl] (nl <= kPfbLdsNl)
    __shared__ RngTabsLds s_rng;
    __shared__ PfbShared sh;
    const int32_t b = blockIdx.x, tid = threadIdx.x;
    const int32_t n = a.n, npad = a.npad, nl = a.nl;
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const LikConst lc = a.filt[b].lc;
    const PredictConst pc = a.filt[b].pc;
    const uint64_t seed = a.filt[b].seed;
    const double ess_th = a.filt[b].ess_th;
    RngTabs rtab{};
    if constexpr (!HOSTNOISE || (MOTION == SLAM_MOTION_VELOCITY && SLAM_TAB_SINCOS))
        rtab = rng_tabs_stage(&s_rng, tid, kPfbThreads);
    for (int32_t k = tid; k < 2 * a.nleaves; k += kPfbThreads) sh.leaves[k] = a.leaves[k];
    for (int32_t k = tid; k < a.nops; k += kPfbThreads) sh.ops[k] = a.ops[k];
    const size_t off = (size_t)b * (size_t)npad;
    double* __restrict__ w_un = a.w_un + off;
    uint64_t* ck = a.c + off;
    PfbSpecial* spec = a.spec + (size_t)b * (size_t)n;
    const bool staged = nl <= kPfbLdsNl;
    const double* lm = a.lm + (size_t)b * 2 * (size_t)nl;
    if (staged) {
        for (int32_t k = tid; k < 2 * nl; k += kPfbThreads) s_dyn[k] = lm[k];
        lm = s_dyn;
    }
    double s_prev = a.s_cur[b];
    int32_t rflag = a.flags[b];

    for (int32_t step = 0; step < a.nsteps; ++step) {
        const size_t sb = (size_t)(a.first + step) * (size_t)a.B + (size_t)b;
        const uint32_t rstep = a.stepno + (uint32_t)step;
        const int src = (a.cur + step) & 1, dst = src ^ 1;
        const double* __restrict__ xs = a.x[src] + off;
        const double* __restrict__ ys = a.y[src] + off;
        const double* __restrict__ ts = a.th[src] + off;
        double* __restrict__ xo = a.x[dst] + off;
        double* __restrict__ yo = a.y[dst] + off;
        double* __restrict__ to = a.th[dst] + off;
        const double* z = a.z + sb * 2 * (size_t)nl;
        __syncthreads();                          // the previous step's readers are done
        if (staged) {
            for (int32_t k = tid; k < 2 * nl; k += kPfbThreads) s_dyn[2 * nl + k] = z[k];
            z = s_dyn + 2 * nl;
        }
        if (tid == 0) sh.info[0] = sh.info[1] = sh.info[2] = 0;
        __syncthreads();
        const size_t cb = (size_t)step * (size_t)a.B + (size_t)b;     // controls: the call's own steps
        const double v = a.ctl[2 * cb], om = a.ctl[2 * cb + 1];

        // ---- resample (particle_filter.py:200-224): exact cumsum, positions
        double ofs = 0.0;
        if (rflag) {
            pfb_exact_cumsum(w_un, s_prev, pc.np_recip, n, npad, ck, spec, sh.shd, sh.shk, sh.shf,
                             sh.info);
            ofs = resample_offset(a.ofs ? a.ofs[b] : __builtin_nan(""), pc.np_recip, seed, rstep);
        }
        const double* c = reinterpret_cast<const double*>(ck);

        // ---- [gather +] predict + likelihood + weight, a pair per lane
        for (int32_t base = 0; base < npad; base += kPfbTile) {
            const int32_t i0 = base + 2 * tid;
            bool valid[2];
            int32_t idx[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                valid[k] = i0 + k < n;
                idx[k] = valid[k] ? i0 + k : n - 1;
            }
            const double2 wu = *reinterpret_cast<const double2*>(w_un + i0);
            const double wprev[2] = {wu.x, wu.y};
            double x[2], y[2], th[2];
            if (rflag) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    // fl(fl(i (1/NP)) + ofs), left search (the while loop of :218-220)
                    int64_t sidx = search_c(c, 0, n, (double)idx[k] * pc.rstep + ofs);
                    if (sidx >= n) {
                        sidx = n - 1;                        // IndexError in the reference
                        if (valid[k]) atomicOr(&sh.info[0], 1);
                    }
                    x[k] = xs[sidx];
                    y[k] = ys[sidx];
                    th[k] = ts[sidx];
                }
            } else {
                const double2 p = *reinterpret_cast<const double2*>(xs + i0);
                const double2 q = *reinterpret_cast<const double2*>(ys + i0);
                const double2 r = *reinterpret_cast<const double2*>(ts + i0);
                x[0] = p.x; x[1] = p.y;
                y[0] = q.x; y[1] = q.y;
                th[0] = r.x; th[1] = r.y;
            }
            double g[2][3];
            if (HOSTNOISE) {
                const double* nz = a.noise + (size_t)b * 3 * (size_t)n;
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int j = 0; j < 3; ++j) g[k][j] = nz[3 * (size_t)idx[k] + j];
            } else {
                double h[6];
                pair_normals((uint64_t)(i0 >> 1), rstep, seed, rtab, h);
#pragma unroll
                for (int j = 0; j < 6; ++j) g[j / 3][j % 3] = h[j];
                if (MOTION == SLAM_MOTION_LINEAR) {            // noise_j = sum_k g_k q[k][j]
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const double h0 = g[k][0], h1 = g[k][1], h2 = g[k][2];
                        g[k][0] = h0 * pc.q[0] + h1 * pc.q[3] + h2 * pc.q[6];
                        g[k][1] = h0 * pc.q[1] + h1 * pc.q[4] + h2 * pc.q[7];
                        g[k][2] = h0 * pc.q[2] + h1 * pc.q[5] + h2 * pc.q[8];
                    }
                }
            }
            double xv[2], yv[2], tv[2], sp[2], cp[2];
#pragma unroll
            for (int k = 0; k < 2; ++k)
                predict_particle<MOTION>(x[k], y[k], th[k], v, om, g[k][0], g[k][1], g[k][2], pc,
                                         xv[k], yv[k], tv[k], sp[k], cp[k], rtab);
            *reinterpret_cast<double2*>(xo + i0) = double2{xv[0], xv[1]};
            *reinterpret_cast<double2*>(yo + i0) = double2{yv[0], yv[1]};
            *reinterpret_cast<double2*>(to + i0) = double2{tv[0], tv[1]};
            // previous weights: 1/NP after a resample (:222), else w_un / s (:235-236)
            double pw[2], bn[2];
#pragma unroll
            for (int k = 0; k < 2; ++k)
                pw[k] = rflag ? pc.np_recip : norm_w(wprev[k], s_prev, pc.np_recip);
            (void)likelihood_lanes<LIK, 2>(xv, yv, sp, cp, lm, z, nullptr, lc, bn, wave_s, pw);
            *reinterpret_cast<double2*>(w_un + i0) =
                double2{valid[0] ? pw[0] * bn[0] : 0.0, valid[1] ? pw[1] * bn[1] : 0.0};   // :194
        }
        __syncthreads();

        // ---- normalise (:226-237): s = np.sum(w_un), w = w_un / s, NaN -> 1/NP
        const double s = pfb_numpy_sum(w_un, n, sh.leaves, a.nleaves, sh.ops, a.nops, sh.leaf, sh.stk);

        // ---- estimate: max / first argmax (:115-117), moments about particle 0
        PfbPartial p;
        p.maxv = -1.0;
        p.maxi = INT32_MAX;
#pragma unroll
        for (int k = 0; k < 11; ++k) p.q[k] = 0.0;
        const double rx = xo[0], ry = yo[0], rt = to[0];
        for (int32_t i = tid; i < n; i += kPfbThreads) {
            const double w = norm_w(w_un[i], s, pc.np_recip);
            if (w > p.maxv) {                       // i ascends: the first index on ties
                p.maxv = w;
                p.maxi = i;
            }
            const double d0 = xo[i] - rx, d1 = yo[i] - ry, d2 = to[i] - rt;
            p.q[0] += w;
            p.q[1] += w * w;
            p.q[2] += w * d0;
            p.q[3] += w * d1;
            p.q[4] += w * d2;
            p.q[5] += (w * d0) * d0;
            p.q[6] += (w * d0) * d1;
            p.q[7] += (w * d0) * d2;
            p.q[8] += (w * d1) * d1;
            p.q[9] += (w * d1) * d2;
            p.q[10] += (w * d2) * d2;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double ov = __shfl_xor(p.maxv, d, 64);
            const int32_t oi = __shfl_xor(p.maxi, d, 64);
            double oq[11];
#pragma unroll
            for (int k = 0; k < 11; ++k) oq[k] = __shfl_xor(p.q[k], d, 64);
            pfb_merge(p, ov, oi, oq);
        }
        if ((tid & 63) == 0) sh.part[tid >> 6] = p;
        __syncthreads();
        if (tid == 0) {
            for (int wv = 1; wv < kPfbThreads / 64; ++wv)
                pfb_merge(p, sh.part[wv].maxv, sh.part[wv].maxi, sh.part[wv].q);
            if (p.maxi >= n) p.maxi = 0;            // no weight above -1 (caller-set negative weights)
            slam_pf_result o;
            o.max_idx = p.maxi;
            o.max_val = p.maxv;
            o.x_est[0] = xo[p.maxi];
            o.x_est[1] = yo[p.maxi];
            o.x_est[2] = to[p.maxi];
            const double inv = 1.0 / p.q[0];
            const double mu[3] = {p.q[2] * inv, p.q[3] * inv, p.q[4] * inv};
            const double m2[9] = {p.q[5], p.q[6], p.q[7], p.q[6], p.q[8], p.q[9], p.q[7], p.q[9], p.q[10]};
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) o.cov[3 * r + q] = m2[3 * r + q] * inv - mu[r] * mu[q];
            o.ess = 1.0 / p.q[1];
            o.weight_sum = s;
            o.resampled = rflag ? 1 : 0;
            o.resample_next = (o.ess < ess_th) ? 1 : 0;
            o.ess_near = (fabs(o.ess - ess_th) <= a.ess_band * ess_th) ? 1 : 0;
            o.status = sh.info[0];
            o.n_special = sh.info[1];
            o.dd_waves = 0;
            a.res[(size_t)step * (size_t)a.B + (size_t)b] = o;
            sh.info[3] = o.resample_next;
        }
        __syncthreads();
        rflag = sh.info[3];
        s_prev = s;
    }
    if (tid == 0) {
        a.s_cur[b] = s_prev;
        a.flags[b] = rflag;
    }
}

// Exact systematic-resampling indices of every filter's current weights
// (slam_pfb_resample_indices): the cumsum and the search of a resample step,
// nothing moved.  status[b]: bit0 clamp, bit1 fallback; nspec[b]: specials.
__global__ __launch_bounds__(kPfbThreads) void pfb_indices_kernel(const PfbArgs a,
                                                                  int32_t* __restrict__ idx_out,
                                                                  int32_t* __restrict__ status,
                                                                  int32_t* __restrict__ nspec) {
    __shared__ PfbShared sh;
    const int32_t b = blockIdx.x, tid = threadIdx.x;
    const int32_t n = a.n;
    const PredictConst pc = a.filt[b].pc;
    const size_t off = (size_t)b * (size_t)a.npad;
    uint64_t* ck = a.c + off;
    if (tid == 0) sh.info[0] = sh.info[1] = sh.info[2] = 0;
    __syncthreads();
    pfb_exact_cumsum(a.w_un + off, a.s_cur[b], pc.np_recip, n, a.npad, ck,
                     a.spec + (size_t)b * (size_t)n, sh.shd, sh.shk, sh.shf, sh.info);
    const double ofs = resample_offset(a.ofs ? a.ofs[b] : __builtin_nan(""), pc.np_recip,
                                       a.filt[b].seed, a.stepno);
    const double* __restrict__ c = reinterpret_cast<const double*>(ck);
    for (int32_t i = tid; i < n; i += kPfbThreads) {
        int64_t sidx = search_c(c, 0, n, (double)i * pc.rstep + ofs);
        if (sidx >= n) {
            sidx = n - 1;
            atomicOr(&sh.info[0], 1);
        }
        idx_out[(size_t)b * (size_t)n + i] = (int32_t)sidx;
    }
    __syncthreads();
    if (tid == 0) {
        status[b] = sh.info[0];
        nspec[b] = sh.info[1];
    }
}

}  // namespace slam
