// pf_finalize.inl -- end of a deferred-normalisation PF step (included by
// pf_kernels.inl).  Workgroups of 512 lanes (8 waves, two per SIMD: the
// serial parts of the step end -- np.sum's left-to-right buffer chain, the
// result record -- run on a wave that shares its SIMD with one other wave
// only).
//
// What is here, in order:
//   * the formulas of the step end, each one function (the table of DESIGN
//     5.1): (1) fin_load_partials, (2) fin_lane_max / fin_block_add /
//     fin_lane_sums, (3) fin_wg_max / fin_rescale_store, (4) fin_buffer_value,
//     (5) fin_row_sum_tree and fin_row_sum_rows (two orders), (6)
//     fin_fold_slices, (7) fin_argmax_resolve, (8) fin_degenerate_pass, (9)
//     fin_export_records, (10) fin_pair_prefix, (11) fin_stage_candidate;
//     besides fin_load_record, lds_chain_sum and the lane layout fin_blk;
//   * finalize_slices_kernel: NP > 2^20, one workgroup per slice of 2048
//     fused blocks beyond the first (1-5, 10);
//   * fin_next_prefix: the next step's block prefix (10, or a loop);
//   * finalize_general_kernel: the step end for NP > 2^24 (1-9, 11);
//   * fin_moment_group: a moment workgroup of a split step end (1-3, 5);
//   * finalize_fast_kernel<SLICED>: the step end up to 2^24 particles, its
//     loads in an order of its own (1-11; 6 and 10 when SLICED).
// dist_record (pf_dist.inl), the sharded filter's record, calls 1-5 too.
//
// Work: np.sum of the unnormalised weights from the fused blocks' leaf sums
// (particle_filter.py:234), the block partials rescaled to the global max and
// combined in a fixed order (ESS :210 and the weighted covariance), the exact
// max / first argmax of w = w_un / s (:115-117), the result record, the step
// context, s for the next step, and -- when the next step resamples -- the
// prefix of the fused-block weight totals for its exact cumsum (:212).
//
// Latency plan: every lane issues the loads of its four fused blocks and its
// sixteen leaves first (NP <= 2^20: one memory round trip); the argmax
// records of the few candidate blocks are fetched while lane 0 runs the
// serial buffer chain.  Argmax: fl(w_un / s) is monotone in w_un, so the
// first block b with fl(M_b / s) == fl(M / s) holds it; inside b the first
// index of M_b is the answer unless a smaller weight before it rounds to the
// same value (fl(pre_b / s) == fl(M / s)), which is then checked element by
// element.  A non-positive or non-finite s (all weights NaN -> 1/NP, :236)
// takes a slow whole-array pass.

#ifdef SLAM_FIN_PROBE
// [0..5]: the phases of a full step end; [16..21]: of a split one (workgroup
// 0); [24 + g]: the end of moment workgroup g of a split one
__device__ long long g_fin_probe[32];
#define FIN_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_fin_probe[k] = wall_clock64(); } while (0)
#define FIN_STAMP_IF(c, k) do { if (c) g_fin_probe[k] = wall_clock64(); } while (0)
#define FIN_STAMP_AT(base, k) FIN_STAMP((base) + (k))
#else
#define FIN_STAMP(k) do { } while (0)
#define FIN_STAMP_IF(c, k) do { } while (0)
#define FIN_STAMP_AT(base, k) do { } while (0)
#endif

#ifndef SLAM_FIN_THREADS
#define SLAM_FIN_THREADS 512
#endif
constexpr int kFinThreads = SLAM_FIN_THREADS;
constexpr int kFinWaves = kFinThreads / 64;
constexpr int kFinRegBlocks = 2048 / kFinThreads;   // fused blocks held in registers per lane (2048)
constexpr int kFinLeafLanes = 4;            // lanes per 8192-element buffer (16 leaves each)
constexpr int kFinBufPerRound = kFinThreads / kFinLeafLanes;   // 128 buffers per round
constexpr int kFinCand = 8;                 // argmax candidate records staged in LDS
constexpr int kFinBatch = 8;                // loads in flight per lane beyond the registers (NP > 2^20)

struct FinRecord {
    double pre, xe[3];
    int64_t pi;
};

__device__ __forceinline__ void fin_load_record(const DeferParts& dp, const int64_t b, FinRecord& f) {
    f.pre = dp.ppre()[b];
    f.pi = dp.pidx()[b];
#pragma unroll
    for (int j = 0; j < 3; ++j) f.xe[j] = dp.pxe(j)[b];
}

// A lane of the np.sum pass takes 4 consecutive fused blocks of a buffer: each
// block left the pairwise sum of its four 128-element leaves (a perfect
// subtree of the buffer's tree), so (b0 + b1) + (b2 + b3) is the lane's
// 16-leaf subtree.
static_assert(kSumChunk == 16 * kPartPer, "a buffer is 16 fused blocks, 4 per np.sum lane");

// s + a[0] + a[1] + ... + a[cnt - 1], left to right (np.sum's buffer chain),
// with the next 16 LDS words in flight while the current 16 are added
__device__ __forceinline__ double lds_chain_sum(double s, const double* a, const int cnt) {
    constexpr int B = 16;
    int k = 0;
    if (cnt >= 2 * B) {
        // two register batches alternating (no copy between them): batch A
        // holds [k, k + B), B the next B; each is refilled while the other
        // is added
        double ra[B], rb[B];
#pragma unroll
        for (int j = 0; j < B; ++j) ra[j] = a[j];
        for (; k + 2 * B <= cnt; k += 2 * B) {
#pragma unroll
            for (int j = 0; j < B; ++j) rb[j] = a[k + B + j];
            __asm__ volatile("" ::: "memory");          // (the reads before the adds)
            __asm__ volatile("" : "+v"(s));
#pragma unroll
            for (int j = 0; j < B; ++j) s = s + ra[j];
            const int nk = (k + 3 * B <= cnt) ? k + 2 * B : k;   // past the end: a harmless re-read
#pragma unroll
            for (int j = 0; j < B; ++j) ra[j] = a[nk + j];
            __asm__ volatile("" ::: "memory");
            __asm__ volatile("" : "+v"(s));
#pragma unroll
            for (int j = 0; j < B; ++j) s = s + rb[j];
        }
    }
    for (; k < cnt; ++k) s = s + a[k];
    return s;
}

// register block k of lane t (k < kFinRegBlocks): neighbour pairs, increasing in k
__device__ __forceinline__ int64_t fin_blk(const int t, const int k) {
    static_assert(kFinRegBlocks % 2 == 0, "pairs of blocks");
    return 2 * (int64_t)t + (k & 1) + 2 * (int64_t)kFinThreads * (k >> 1);
}

// ---------------------------------------------------------------------------
// The formulas of the step end, each written once (DESIGN 5.1 has the table
// of callers).  Columns of a lane's q[k][] and acc[] hold quantities JQ,
// JQ + 1, ... of the fused kernel's partial sums ps(): 0 = sum u, 1 = sum
// u^2 (scaled by the SQUARE of a ratio of maxima), 2.. = the covariance
// moments.

// (1) The lane's block partials: has[k] and, with PMAX, pm[k] of the blocks
// b_base + fin_blk(tid, k); then q[k][jq + j] = ps(j0 + j) of them, j < NJ.
// Neighbour pairs, one 16-byte load per array (the partial arrays hold nb + 1
// entries).  Called again for a further range it re-forms has[] to the same
// values.
template <bool PMAX, int NJ, int NQ>
__device__ __forceinline__ void fin_load_partials(const DeferParts& dp, const int64_t b_base,
                                                  const int64_t nb, const int j0, const int jq,
                                                  double (&pm)[kFinRegBlocks],
                                                  double (&q)[kFinRegBlocks][NQ],
                                                  bool (&has)[kFinRegBlocks]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int kp = 0; kp < kFinRegBlocks / 2; ++kp) {
        const int64_t b = b_base + fin_blk(tid, 2 * kp);
        has[2 * kp] = b < nb;
        has[2 * kp + 1] = b + 1 < nb;
        const int64_t bb = has[2 * kp] ? b : 0;
        if constexpr (PMAX) {
            const double2 t = *reinterpret_cast<const double2*>(dp.pmax() + bb);
            pm[2 * kp] = t.x;
            pm[2 * kp + 1] = t.y;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const double2 u = *reinterpret_cast<const double2*>(dp.ps(j0 + j) + bb);
            q[2 * kp][jq + j] = u.x;
            q[2 * kp + 1][jq + j] = u.y;
        }
    }
}

// (2a) the largest block max of the lane's register blocks (-1: none)
__device__ __forceinline__ double fin_lane_max(const double (&pm)[kFinRegBlocks],
                                               const bool (&has)[kFinRegBlocks]) {
    double mlane = -1.0;
#pragma unroll
    for (int k = 0; k < kFinRegBlocks; ++k)
        if (has[k]) mlane = fmax(mlane, pm[k]);
    return mlane;
}

// (2b) one block into the lane's sums: r = M_b / mlane; the moments
// (quantities >= 2) only when `full`
template <int JQ, int NQ, int NA>
__device__ __forceinline__ void fin_block_add(const double r, const double (&qq)[NQ], const bool full,
                                              double (&acc)[NA]) {
    static_assert(NQ <= NA, "a sum per quantity");
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        if (JQ + c == 0) acc[c] += r * qq[c];
        else if (JQ + c == 1) acc[c] += (r * r) * qq[c];
        else if (full) acc[c] += r * qq[c];
    }
}

// (2c) the lane's sums over its register blocks, scaled to the lane's max
template <int JQ, int NQ>
__device__ __forceinline__ void fin_lane_sums(const double (&pm)[kFinRegBlocks],
                                              const double (&q)[kFinRegBlocks][NQ],
                                              const bool (&has)[kFinRegBlocks], const double mlane,
                                              const bool full, double (&acc)[NQ]) {
#pragma unroll
    for (int c = 0; c < NQ; ++c) acc[c] = 0.0;
    if (mlane > 0.0) {
        const double rm = 1.0 / mlane;
#pragma unroll
        for (int k = 0; k < kFinRegBlocks; ++k)
            if (has[k]) fin_block_add<JQ>(pm[k] * rm, q[k], full, acc);
    }
}

// (3a) the workgroup's max from the waves' maxima
__device__ __forceinline__ double fin_wg_max(const double* s_wmax) {
    double M = s_wmax[0];
#pragma unroll
    for (int w = 1; w < kFinWaves; ++w) M = fmax(M, s_wmax[w]);
    return M;
}

// (3b) the lane's first NQ sums rescaled from the lane's max to M, into row c
// of s_q (the moments only when `full`)
template <int JQ, int NQ, int NA>
__device__ __forceinline__ void fin_rescale_store(const double (&acc)[NA], const double mlane,
                                                  const double M, const bool full,
                                                  double (*s_q)[kFinThreads]) {
    static_assert(NQ <= NA, "a sum per quantity");
    const double rl = (mlane > 0.0 && M > 0.0) ? mlane / M : 0.0;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
        if (JQ + c == 0) s_q[c][threadIdx.x] = acc[c] * rl;
        else if (JQ + c == 1) s_q[c][threadIdx.x] = acc[c] * (rl * rl);
        else if (full) s_q[c][threadIdx.x] = acc[c] * rl;
    }
}

// (4) np.sum's value of an 8192-element buffer from its four lanes' leaf
// subtrees L (0 where the lane has none): (L0 + L1) + (L2 + L3), then the two
// quad swaps with the lower lane on the left; every lane of the quad gets it
__device__ __forceinline__ double fin_buffer_value(const double (&L)[4], const bool valid) {
    static_assert(kFinLeafLanes == 4, "two quad swaps");
    const int part = threadIdx.x & (kFinLeafLanes - 1);
    double v = valid ? (L[0] + L[1]) + (L[2] + L[3]) : 0.0;
    {
        const double o = dpp_f64<kDppXor1>(v);
        v = (part & 1) ? (o + v) : (v + o);
    }
    {
        const double o = dpp_f64<kDppXor2>(v);
        v = (part & 2) ? (o + v) : (v + o);
    }
    return v;
}

// (5) The transposed reduction of a row of s_q: 8 lane-strided adds, then the
// wave.  Two orders, each kernel keeps its own: `tree` is the xor
// butterfly with the lower lane on the left, whose four 16-lane rows combine
// as (r0 + r1) + (r2 + r3); `rows` is wave_sum_rows, ((r0 + r1) + r2) + r3.
__device__ __forceinline__ double fin_row_strided(const double* row) {
    const int lane = threadIdx.x & 63;
    double r = row[lane];
#pragma unroll
    for (int m = 1; m < kFinThreads / 64; ++m) r = r + row[lane + 64 * m];
    return r;
}
__device__ __forceinline__ double fin_row_sum_tree(const double* row) {
    const int lane = threadIdx.x & 63;
    double r = fin_row_strided(row);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = xor_f64(r, d);
        r = (lane & d) ? (o + r) : (r + o);
    }
    return r;
}
__device__ __forceinline__ double fin_row_sum_rows(const double* row) {
    return wave_sum_rows(fin_row_strided(row));
}

// (6) quantity j's total r plus the later slices' sums q[g][11], each scaled
// to its slice max m[g] and rescaled to M, in slice order (global memory or LDS)
__device__ __forceinline__ double fin_fold_slices(double r, const int j, const int nsl, const double M,
                                                  const double* m, const double* q) {
    for (int g = 1; g < nsl; ++g) {
        const double mg = m[g];
        if (mg > 0.0) {
            const double f = mg / M;
            r = r + q[(int64_t)g * 11 + j] * (j == 1 ? f * f : f);
        }
    }
    return r;
}

// the LDS words of the argmax (the kernels declare them; a wave still at the
// tie decision's s_flag must find it unchanged: the step's later flags, such
// as resample_next, live in words of their own)
struct FinArgmaxLds {
    unsigned long long* s_min;
    int32_t* s_flag;
    int64_t* s_mi;
    double* s_xe;           // [3]
    int* s_ncand;
    int64_t* s_cblk;        // [kFinCand]
    FinRecord* s_crec;      // [kFinCand]
};

// (11) stage block b as an argmax candidate: a slot, then its record (*rec,
// or loaded once the slot is won)
__device__ __forceinline__ void fin_stage_candidate(const FinArgmaxLds& a, const DeferParts& dp,
                                                    const int64_t b, const FinRecord* rec) {
    const int slot = atomicAdd(a.s_ncand, 1);
    if (slot < kFinCand) {
        FinRecord f;
        if (rec) f = *rec;
        else fin_load_record(dp, b, f);
        a.s_cblk[slot] = b;
        a.s_crec[slot] = f;
    }
}

// (7) From the lanes' first blocks cb whose max rounds to mval = fl(M / s)
// (~0: none) to the answer in s_mi / s_xe (whole workgroup): block bc's
// record, staged or loaded; unless a smaller weight ahead of the block max
// rounds to the same maximum (fl(pre / s) == mval), when the block's elements
// are checked one by one.
__device__ __forceinline__ void fin_argmax_resolve(const FinArgmaxLds& a, const unsigned long long cb,
                                                   const int64_t n, const double s, const double mval,
                                                   const double np_recip, const DeferParts& dp,
                                                   const double* __restrict__ w_un,
                                                   const double* __restrict__ xs,
                                                   const double* __restrict__ ys,
                                                   const double* __restrict__ ts) {
    const int tid = threadIdx.x;
    if (cb != ~0ull) atomicMin(a.s_min, cb);
    __syncthreads();
    const int64_t bc = (int64_t)*a.s_min;
    if (tid == 0) {
        // block bc's record: staged, or loaded if bc was not a staged candidate
        int slot = -1;
        const int nc = min(*a.s_ncand, kFinCand);
        for (int j = 0; j < nc; ++j)
            if (a.s_cblk[j] == bc) slot = j;
        FinRecord f;
        if (slot >= 0) {
            f = a.s_crec[slot];
            // (keeps the LDS reads LDS reads: behind pointers the two branches'
            // loads otherwise merge into flat loads of a selected address)
            __asm__ volatile("" ::: "memory");
        } else {
            fin_load_record(dp, bc, f);
        }
        *a.s_mi = f.pi;
        a.s_xe[0] = f.xe[0];
        a.s_xe[1] = f.xe[1];
        a.s_xe[2] = f.xe[2];
        *a.s_flag = (f.pre / s == mval) ? 1 : 0;
        if (*a.s_flag) *a.s_min = ~0ull;
    }
    __syncthreads();
    if (*a.s_flag) {
        // the first index of the block whose w equals mval
        for (int e = tid; e < kPartPer; e += kFinThreads) {
            const int64_t i = bc * kPartPer + e;
            if (i < n && norm_w(w_un[i], s, np_recip) == mval)
                atomicMin(a.s_min, (unsigned long long)i);
        }
        __syncthreads();
        if (tid == 0) {
            const int64_t i = (int64_t)*a.s_min;
            *a.s_mi = i;
            a.s_xe[0] = xs[i];
            a.s_xe[1] = ys[i];
            a.s_xe[2] = ts[i];
        }
    }
}

// (8) The degenerate step (s not positive and finite): every weight through
// the reference's division (norm_w) into a BlockPartial, the workgroup's
// reduction of them, and the estimate's pose into s_xe.  Slow.
__device__ __forceinline__ BlockPartial fin_degenerate_pass(
    const int64_t n, const double* __restrict__ w_un, const double s, const double np_recip,
    const double* __restrict__ xs, const double* __restrict__ ys, const double* __restrict__ ts,
    const double* __restrict__ refp, BlockPartial* shp, double* s_xe) {
    const int tid = threadIdx.x;
    BlockPartial a;
    bp_zero(a);
    const double r0 = refp[0], r1 = refp[1], r2 = refp[2];
    for (int64_t i = tid; i < n; i += kFinThreads) {
        const double v = norm_w(w_un[i], s, np_recip);
        BlockPartial o;
        o.maxv = v;
        o.maxi = i;
        o.sw = v;
        o.sw2 = v * v;
        const double d0 = xs[i] - r0, d1 = ys[i] - r1, d2 = ts[i] - r2;
        const double v0 = v * d0, v1 = v * d1, v2 = v * d2;
        o.m1[0] = v0; o.m1[1] = v1; o.m1[2] = v2;
        o.m2[0] = v0 * d0; o.m2[1] = v0 * d1; o.m2[2] = v0 * d2;
        o.m2[3] = v1 * d1; o.m2[4] = v1 * d2; o.m2[5] = v2 * d2;
        bp_merge(a, o);
    }
    const BlockPartial tot = bp_block_reduce(a, shp);
    if (tid == 0) {
        s_xe[0] = xs[tot.maxi];
        s_xe[1] = ys[tot.maxi];
        s_xe[2] = ts[tot.maxi];
    }
    return tot;
}

// (9) the batch's earlier records (stored by earlier launches) to the host
// buffer, by lanes 1..63; this step's record went there from write_result_*
__device__ __forceinline__ void fin_export_records(const StepIO& io, const bool exp,
                                                   const int32_t b_first, const int32_t st_now) {
    const int tid = threadIdx.x;
    if (exp && tid >= 1 && tid < 64) {
        for (int32_t k = b_first + tid - 1; k < st_now; k += 63) io.res_host[k] = io.res[k];
    }
}

// (10) The two-half exclusive prefix over the lanes of the fused-block totals
// (whole workgroup, one barrier): lane t holds blocks 2t, 2t + 1 of each half
// of 2 kFinThreads blocks.  u0[hf] = (M_b / den) * q0 of the half's first
// block (den = 1: w_un units, x / 1 is x; den = s: the quotient is rounded
// before the product), the pair sums scanned by wave_excl_scan_rows, the wave
// totals through scr (2 kFinWaves doubles of LDS), the second half offset by
// the first half's total tot[0].  pex[hf]: the prefix of block fin_blk(tid,
// 2 hf); its neighbour's is pex[hf] + u0[hf].  An approximate prefix: the exact
// cumsum classifies against it with a margin, any fixed order serves.
__device__ __forceinline__ void fin_pair_prefix(const double (&pm)[kFinRegBlocks],
                                                const double (&q0)[kFinRegBlocks],
                                                const bool (&has)[kFinRegBlocks], const double den,
                                                double* scr, double (&pex)[2], double (&u0)[2],
                                                double (&tot)[2]) {
    static_assert(kFinRegBlocks == 4, "two halves of lane pairs");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        u0[hf] = has[2 * hf] ? (pm[2 * hf] / den) * q0[2 * hf] : 0.0;
        const double u1 = has[2 * hf + 1] ? (pm[2 * hf + 1] / den) * q0[2 * hf + 1] : 0.0;
        double wt;
        pex[hf] = wave_excl_scan_rows(u0[hf] + u1, wt);
        if (lane == 63) scr[hf * kFinWaves + wave] = wt;
    }
    __syncthreads();
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        double base = 0.0, all = 0.0;
#pragma unroll
        for (int w = 0; w < kFinWaves; ++w) {
            if (w < wave) base = base + scr[hf * kFinWaves + w];
            all = all + scr[hf * kFinWaves + w];
        }
        pex[hf] = base + pex[hf];
        tot[hf] = all;
    }
    pex[1] = tot[0] + pex[1];
}

// NP > 2^20 (round 5): slices of 2048 fused blocks beyond the first, one
// workgroup each, laid out like the finalize's register blocks: the slice's
// max M_g, its 11 partial sums scaled to M_g (lane sums over the lane's four
// blocks, rescaled to M_g, then the finalize's transposed reduction), and the
// np.sum value of each of its 128 buffers (pairwise over the buffer's 16
// block subtrees).  The finalize then rescales the slices to the global max
// and continues np.sum's left-to-right chain over the buffer values, instead
// of pulling every block through one CU (a 2^23-particle finalize: 1.7 MB).
// slice g's buffers are g * kFinBufPerRound ...: a slice of 2048 fused blocks
// must be exactly one round of buffers (16 blocks each), i.e. 512 lanes
static_assert(kFinThreads * kFinRegBlocks == 16 * kFinBufPerRound,
              "a finalize slice (2048 fused blocks) must span kFinBufPerRound buffers");
constexpr int kSliceCand = 4;               // argmax candidate blocks a slice lists
struct FinSlices {
    double* m;          // [nsl] slice max (slice 0: the finalize's own)
    double* q;          // [nsl][11] slice sums scaled to the slice max
    double* buf;        // [nfull] np.sum value of each full 8192-element buffer
    int64_t* cblk;      // [nsl][kSliceCand] blocks with M_b within 2^-48 of the slice max
    double* cpm;        // [nsl][kSliceCand] their maxima
    int32_t* ncand;     // [nsl] how many there were (> kSliceCand: the slice is scanned)
    double* pre;        // [nb] the next step's block prefix inside each slice, w_un units
    double* u;          // [nsl] the slice's total of w_un (pre's units)
    int32_t nsl;        // slices of 2048 fused blocks; <= 1: no pre-pass
};

__global__ __launch_bounds__(kFinThreads) void finalize_slices_kernel(const int64_t n,
                                                                      const DeferParts dp,
                                                                      const FinSlices sl) {
    __shared__ double s_q[11][kFinThreads];
    __shared__ double s_wmax[kFinWaves];
    __shared__ int s_nc;
    __shared__ int64_t s_cb[kSliceCand];
    __shared__ double s_cp[kSliceCand];
    __shared__ double s_pw[2][kFinWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = 1 + (int)blockIdx.x;
    if (tid == 0) s_nc = 0;
    const int64_t nb = (n + kPartPer - 1) / kPartPer;
    const int64_t nfull = n / kSumChunk;
    const int64_t b_base = (int64_t)g * kFinThreads * kFinRegBlocks;
    double pm[kFinRegBlocks], q[kFinRegBlocks][11];
    bool has[kFinRegBlocks];
    fin_load_partials<true, 11>(dp, b_base, nb, 0, 0, pm, q, has);
    // the slice's buffers: 4 lanes per buffer, pairwise
    {
        const int part = tid & (kFinLeafLanes - 1);
        const int64_t c = (int64_t)g * kFinBufPerRound + tid / kFinLeafLanes;
        double L[4] = {};
        if (c < nfull) {
            const double* Lp = dp.leaf() + 16 * c + 4 * part;
#pragma unroll
            for (int j = 0; j < 4; ++j) L[j] = Lp[j];
        }
        const double v = fin_buffer_value(L, c < nfull);
        if (part == 0 && c < nfull) sl.buf[c] = v;
    }
    const double mlane = fin_lane_max(pm, has);
    double acc[11];
    fin_lane_sums<0>(pm, q, has, mlane, true, acc);
    const double mx = wave_max_f64(mlane);
    if (lane == 0) s_wmax[wave] = mx;
    __syncthreads();
    const double M = fin_wg_max(s_wmax);
    fin_rescale_store<0, 11>(acc, mlane, M, true, s_q);
    // the slice's argmax candidates (a global candidate in this slice is one:
    // the global max is >= M); the finalize checks them instead of the slice
#pragma unroll
    for (int k = 0; k < kFinRegBlocks; ++k) {
        if (has[k] && pm[k] >= M * (1.0 - 0x1p-48)) {
            const int slot = atomicAdd(&s_nc, 1);
            if (slot < kSliceCand) {
                s_cb[slot] = b_base + fin_blk(tid, k);
                s_cp[slot] = pm[k];
            }
        }
    }
    // the next step's block prefix (S1) inside the slice in w_un units (M_b
    // times the block's sum of w_un / M_b): the finalize scales it by 1 / s
    // and offsets it by the slices before, when the next step resamples
    {
        double q0[kFinRegBlocks], u0[2], pex[2], tot[2];
#pragma unroll
        for (int k = 0; k < kFinRegBlocks; ++k) q0[k] = q[k][0];
        fin_pair_prefix(pm, q0, has, 1.0, &s_pw[0][0], pex, u0, tot);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int64_t b = b_base + fin_blk(tid, 2 * hf);
            if (b + 1 < nb) *reinterpret_cast<double2*>(sl.pre + b) = double2{pex[hf], pex[hf] + u0[hf]};
            else if (b < nb) sl.pre[b] = pex[hf];
        }
        if (tid == 0) sl.u[g] = tot[0] + tot[1];
    }
    for (int j = wave; j < 11; j += kFinWaves) {
        const double r = fin_row_sum_tree(s_q[j]);
        if (lane == 0) sl.q[(int64_t)g * 11 + j] = r;
    }
    if (tid < kSliceCand) {
        const bool in = tid < s_nc;
        sl.cblk[g * kSliceCand + tid] = in ? s_cb[tid] : -1;
        sl.cpm[g * kSliceCand + tid] = in ? s_cp[tid] : -1.0;
    }
    if (tid == 0) {
        sl.m[g] = M;
        sl.ncand[g] = s_nc;
    }
}

// The next step's fused-block totals of w = w_un / s for its exact cumsum
// (S1): boff[b] = the exclusive prefix, boff[nb] = the total.  Called by the
// whole workgroup when the step just finalised resamples next.  pm / q0 /
// has: the lane's register blocks fin_blk(tid, k) (block max, sum of w_un /
// M_b); sh: 2048 doubles of LDS; scr: kFinThreads doubles of LDS.
__device__ void fin_next_prefix(const int64_t n, const int64_t nb, const bool ok, const double s,
                                const double np_recip, const double (&pm)[kFinRegBlocks],
                                const double (&q0)[kFinRegBlocks], const bool (&has)[kFinRegBlocks],
                                const double* __restrict__ w_un, const DeferParts& dp,
                                double* __restrict__ boff, double* sh, double* scr) {
    const int tid = threadIdx.x;
    if (ok && nb <= (int64_t)kFinThreads * kFinRegBlocks) {
        // fused-block totals of w for the next step's exact cumsum (S1) from the
        // registers (round 6), each block's M_b / s rounded before the product
        double ex[2], t0[2], tot[2];
        fin_pair_prefix(pm, q0, has, s, scr, ex, t0, tot);
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int64_t b = fin_blk(tid, 2 * hf);
            if (b + 1 < nb) {
                *reinterpret_cast<double2*>(boff + b) = double2{ex[hf], ex[hf] + t0[hf]};
            } else if (b < nb) {
                boff[b] = ex[hf];
            }
        }
        if (tid == 0) boff[nb] = tot[0] + tot[1];
    } else {
        // fused-block totals of w for the next step's exact cumsum (S1), moved
        // through LDS so that lane t owns the contiguous blocks [t per, (t+1) per)
        auto btot_slow = [&](int64_t b) {
            double v = 0.0;
            const int64_t e = (b + 1) * kPartPer < n ? (b + 1) * kPartPer : n;
            for (int64_t i = b * kPartPer; i < e; ++i) v += norm_w(w_un[i], s, np_recip);
            return v;
        };
        const bool in_lds = ok && nb <= 2048;
        if (in_lds) {
#pragma unroll
            for (int k = 0; k < kFinRegBlocks; ++k)
                if (has[k]) sh[fin_blk(tid, k)] = (pm[k] / s) * q0[k];
        }
        __syncthreads();
        auto btot = [&](int64_t b) {
            if (in_lds) return sh[b];
            if (ok) return (dp.pmax()[b] / s) * dp.ps(0)[b];
            return btot_slow(b);
        };
        const int per = (int)((nb + kFinThreads - 1) / kFinThreads);
        const int64_t b0 = (int64_t)tid * per;
        // batches of kFinBatch totals (their loads together), then the adds in order
        auto btot_batch = [&](const int k0, double (&t)[kFinBatch]) {
#pragma unroll
            for (int u = 0; u < kFinBatch; ++u) {
                const int64_t b = b0 + k0 + u;
                t[u] = (k0 + u < per && b < nb) ? btot(b) : 0.0;
            }
        };
        double loc = 0.0;
        for (int k0 = 0; k0 < per; k0 += kFinBatch) {
            double t[kFinBatch];
            btot_batch(k0, t);
#pragma unroll
            for (int u = 0; u < kFinBatch; ++u)
                if (k0 + u < per && b0 + k0 + u < nb) loc += t[u];
        }
        double total;
        double ex = block_excl_scan<double, kFinThreads>(loc, scr, total);
        for (int k0 = 0; k0 < per; k0 += kFinBatch) {
            double t[kFinBatch];
            btot_batch(k0, t);
#pragma unroll
            for (int u = 0; u < kFinBatch; ++u)
                if (k0 + u < per && b0 + k0 + u < nb) {
                    boff[b0 + k0 + u] = ex;
                    ex = ex + t[u];
                }
        }
        if (tid == 0) boff[nb] = total;
    }
}

// The general step end: any number of slices and buffers (the fast kernel
// below takes what fits its registers and LDS; launch_reduce chooses).
// Requires the slice pre-pass: it is launched only behind
// finalize_slices_kernel (sl.nsl > 1, so NP > 2^20 and at least one full round
// of kFinBufPerRound np.sum buffers).  The workgroup reduces slice 0 (the
// first 2048 fused blocks) from its registers and takes every later slice's
// max, sums and buffer values from the pre-pass.
__global__ __launch_bounds__(kFinThreads) void finalize_general_kernel(
    const int64_t n, const DeferParts dp, const double* __restrict__ w_un,
    double* __restrict__ s_cur, const int32_t* __restrict__ tail_leaves,
    const int32_t* __restrict__ tail_ops, const int32_t n_tail_leaves, const int32_t n_tail_ops,
    const double* __restrict__ xs, const double* __restrict__ ys, const double* __restrict__ ts,
    double* __restrict__ refp, int32_t* __restrict__ flags, const double ess_th, StepIO io,
    const int32_t resampled_known, const double np_recip, double* __restrict__ boff,
    const FinSlices sl, const FinSplit fs) {
    __shared__ double sh[2048];                      // buffer sums / tail leaves / block totals
    __shared__ double s_q[11][kFinThreads];
    __shared__ BlockPartial shp[kFinWaves];
    __shared__ double s_wmax[kFinWaves];
    __shared__ double s_tot[11];
    __shared__ double s_s;
    __shared__ unsigned long long s_min;
    __shared__ int32_t s_flag;
    __shared__ int32_t s_next;      // resample_next: a word of its own (a wave still at
                                    // the tie decision's s_flag must not read it)
    __shared__ int64_t s_mi;
    __shared__ double s_xe[3];
    __shared__ int s_ncand;
    __shared__ int64_t s_cblk[kFinCand];
    __shared__ FinRecord s_crec[kFinCand];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nb = (n + kPartPer - 1) / kPartPer;
    const int64_t nfull = n / kSumChunk;
    const int64_t nch = (n + kSumChunk - 1) / kSumChunk;
    FIN_STAMP(0);
    // the step, and the batch's bounds (the last step exports the batch's records)
    const int32_t st_now = io.ctr[0], b_first = io.ctr[2], b_last = io.ctr[3];
    const bool exp = io.res_host != nullptr && st_now == b_last && b_first <= b_last;
    if (tid == 0) {
        s_ncand = 0;
        s_min = ~0ull;
        s_flag = 0;
    }
    const FinArgmaxLds am{&s_min, &s_flag, &s_mi, s_xe, &s_ncand, s_cblk, s_crec};
    // ---- loads, issued up front: this lane's blocks fin_blk(tid, k) and its leaves
    double pm[kFinRegBlocks], q[kFinRegBlocks][11];
    bool has[kFinRegBlocks];
    fin_load_partials<true, 11>(dp, 0, nb, 0, 0, pm, q, has);
    const int part = tid & (kFinLeafLanes - 1);
    double L[4];                                   // fused-block subtree sums (buffer tid / 4 < nfull)
    {
        const double* Lp = dp.leaf() + 16 * (int64_t)(tid / kFinLeafLanes) + 4 * part;
#pragma unroll
        for (int j = 0; j < 4; ++j) L[j] = Lp[j];
    }
    // ---- lane partial sums scaled to the lane's max (rescaled to the global
    // max once that is known); q dies here except the totals q[k][0]
    const double mlane = fin_lane_max(pm, has);
    double acc[11];
    fin_lane_sums<0>(pm, q, has, mlane, true, acc);
    const double mx = wave_max_f64(mlane);
    if (lane == 0) s_wmax[wave] = mx;
    // ---- np.sum: 8192-element buffers, pairwise inside; slice 0's round of
    // kFinBufPerRound buffers from the leaves here (every lane has one: nfull >=
    // kFinBufPerRound), the later slices' buffer values after
    double s = 0.0;
    {
        const double v = fin_buffer_value(L, true);
        if (part == 0) sh[tid / kFinLeafLanes] = v;
        __syncthreads();
        if (kFinBufPerRound < nfull && tid == 0) {       // not the last round: fold it now
            s = lds_chain_sum(s, sh, kFinBufPerRound);
        }
    }
    int64_t last_cnt = kFinBufPerRound;
    // the slices' buffer values, staged 2048 at a time behind the chain so far
    for (int64_t c0 = kFinBufPerRound; c0 < nfull; c0 += 2048) {
        const int64_t cnt = (nfull - c0 < 2048) ? nfull - c0 : 2048;
        __syncthreads();                                  // lane 0 is done with sh
        for (int64_t k = tid; k < cnt; k += kFinThreads) sh[k] = sl.buf[c0 + k];
        __syncthreads();
        if (c0 + 2048 < nfull && tid == 0) s = lds_chain_sum(s, sh, (int)cnt);
        last_cnt = cnt;
    }
    double M = fin_wg_max(s_wmax);
    {                                                    // the slices' maxima (every wave alike)
        double msl = -1.0;
        for (int g = 1 + lane; g < sl.nsl; g += 64) msl = fmax(msl, sl.m[g]);
        M = fmax(M, wave_max_f64(msl));
    }
    FIN_STAMP(1);
    if (tid == 0) {
        // the last round's buffers left to right (the other waves meanwhile
        // rescale their partials and fetch the argmax candidates)
        __builtin_amdgcn_s_setprio(3);
        s = lds_chain_sum(s, sh, (int)last_cnt);
        __builtin_amdgcn_s_setprio(0);
    }
    fin_rescale_store<0, 11>(acc, mlane, M, true, s_q);
    // argmax records of the candidate blocks (fl(M_b / s) == fl(M / s) needs
    // M_b within 2 ulp of M), staged in LDS
#pragma unroll
    for (int k = 0; k < kFinRegBlocks; ++k)
        if (has[k] && pm[k] >= M * (1.0 - 0x1p-48)) fin_stage_candidate(am, dp, fin_blk(tid, k), nullptr);
    if (nch > nfull) {
        __syncthreads();                                  // sh reused by the tail
        const double tsum = tail_chunk_sum(w_un + nfull * kSumChunk, tail_leaves, tail_ops,
                                           n_tail_leaves, n_tail_ops, sh);
        if (tid == 0) s = s + tsum;
    }
    if (tid == 0) s_s = s;
    __syncthreads();
    s = s_s;
    FIN_STAMP(2);
    const bool ok = (s > 0.0) && !isinf(s) && (M > 0.0);
    BlockPartial tot;
    bp_zero(tot);
    if (ok) {
        // ---- the 11 sums: wave w reduces quantities w and w + 8 (lane-strided
        // reads, then a butterfly with the lower lane on the left)
        for (int j = wave; j < 11; j += kFinWaves) {
            const double r = fin_row_sum_tree(s_q[j]);
            if (lane == 0) s_tot[j] = r;
        }
        __syncthreads();                                 // + the slices, rescaled to M, in order
        if (tid < 11) s_tot[tid] = fin_fold_slices(s_tot[tid], tid, sl.nsl, M, sl.m, sl.q);
        // ---- argmax: the first block whose max rounds to fl(M / s)
        const double mval = M / s;
        unsigned long long cb = ~0ull;
#pragma unroll
        for (int k = kFinRegBlocks - 1; k >= 0; --k)
            if (has[k] && pm[k] >= M * (1.0 - 0x1p-48) && pm[k] / s == mval)
                cb = (unsigned long long)fin_blk(tid, k);
        // the blocks beyond the registers: a batch of loads issued before they
        // are used (one memory round trip per iteration made the 2^23-particle
        // step end 50-110 us)
        const int64_t bx0 = tid + (int64_t)kFinThreads * kFinRegBlocks;
        for (int64_t b0 = bx0; b0 < nb && cb == ~0ull; b0 += kFinBatch * (int64_t)kFinThreads) {
            double v[kFinBatch];
#pragma unroll
            for (int u = 0; u < kFinBatch; ++u) {
                const int64_t b = b0 + (int64_t)u * kFinThreads;
                v[u] = (b < nb) ? dp.pmax()[b] : -1.0;
            }
#pragma unroll
            for (int u = 0; u < kFinBatch; ++u) {
                const int64_t b = b0 + (int64_t)u * kFinThreads;
                if (cb == ~0ull && b < nb && v[u] / s == mval) cb = (unsigned long long)b;
            }
        }
        fin_argmax_resolve(am, cb, n, s, mval, np_recip, dp, w_un, xs, ys, ts);
        if (tid == 0) {
            const double f = M / s;                      // back from max-relative to w_un / s
            tot.maxv = mval;
            tot.maxi = s_mi;
            tot.sw = s_tot[0] * f;
            tot.sw2 = s_tot[1] * (f * f);
            for (int j = 0; j < 3; ++j) tot.m1[j] = s_tot[2 + j] * f;
            for (int j = 0; j < 6; ++j) tot.m2[j] = s_tot[5 + j] * f;
        }
    } else {
        tot = fin_degenerate_pass(n, w_un, s, np_recip, xs, ys, ts, refp, shp, s_xe);
    }
    FIN_STAMP(3);
    if (tid == 0) {
        const int32_t st = io.ctr[0];
        s_next = write_result_xe(tot, s_xe, refp, s, flags, ess_th, io.ess_band, io.res + st,
                                 resampled_known, exp ? io.res_host + st : nullptr);
        io.ctr[0] = st + 1;
        io.ctr[1] = io.ctr[1] + 1;
        *s_cur = s;
    }
    __syncthreads();
    FIN_STAMP(4);
    fin_export_records(io, exp, b_first, st_now);
    if (s_next) {
        double q0[kFinRegBlocks];
#pragma unroll
        for (int k = 0; k < kFinRegBlocks; ++k) q0[k] = q[k][0];
        fin_next_prefix(n, nb, ok, s, np_recip, pm, q0, has, w_un, dp, boff, sh, &s_q[0][0]);
    }
    FIN_STAMP(5);
}

// ---------------------------------------------------------------------------
// NP <= 2^24 (round 6): the same work as
// finalize_general_kernel in an order built around its latencies (phase
// probe).  The leaves are requested first, so np.sum's buffer chain
// starts on lane 0 after one round trip and runs while the block partials are
// still arriving; each wave requests the argmax records of its own candidate
// blocks (within 2^-48 of the wave's max -- a superset of the global
// candidates) as soon as the block maxima arrive; the step context and the
// flag words the record reads are fetched with the partials.  SLICED (NP >
// 2^20, finalize_slices_kernel ran first): the slices' buffer values, maxima,
// sums and argmax candidate lists are fetched in the same first round trip,
// so the chain runs over every buffer from LDS and the argmax checks the
// listed candidates instead of walking the blocks beyond the registers.
//
// NP <= 2^20 (!SLICED), the split step end: a step inside a device-resident
// batch, before the batch's last, runs as 1 + kFinMomGroups workgroups with
// no hand-off between them.  Workgroup 0 is the step end: it loads the
// leaves, pmax and ps(0..1) only (10 of the 28 loads per lane) and writes
// everything the next kernel needs and the record without its cov.  The
// covariance moments ps(2..10), which nothing on the device reads, go to the
// moment workgroups (fin_moment_group): each reduces its share exactly as the
// full path does and stores the raw totals relative to M into the step's
// FinMoments entry; the record's reader forms cov from them
// (cov_from_totals; slam_pf_run after its wait).  The batch's last step and
// every stepwise launch take the full path in workgroup 0 (complete records,
// the moment workgroups return at once), as does a degenerate step (!ok),
// whose entry workgroup 0 marks complete.
constexpr int kFinFastSlices = 16;          // SLICED: NP <= 2^24
constexpr int kFinSlBuf = 4;                // SLICED: slice buffer values per lane (nfull <= 2048)
constexpr int kFinMomGroups = 3;            // moment workgroups of a split step end
constexpr int kFinMomPer = 9 / kFinMomGroups;   // of ps(2..10) each
static_assert(kFinMomGroups * kFinMomPer == 9 && kFinMomPer <= kFinWaves, "ps(2..10), a wave per sum");

// full step end: a stepwise launch, or a step that is not strictly inside a
// batch before its last step (ctr[2..3]: the batch's bounds, -1 without one)
__device__ __forceinline__ bool fin_full_path(const int32_t full, const int32_t st,
                                              const int32_t b_first, const int32_t b_last) {
    return full != 0 || !(b_first <= st && st < b_last);
}

// Moment workgroup g of a split step end: ps(2 + g kFinMomPer ...) over the
// lane layout of fin_blk, scaled to the lane's max, rescaled to M, reduced in
// the full path's order (per quantity: the same bits), stored raw.
__device__ void fin_moment_group(const int g, const int64_t nb, const DeferParts& dp,
                                 const StepIO& io, const FinSplit& fs, double (*s_q)[kFinThreads],
                                 double* s_wmax) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t st = io.ctr[kCtrMom + fs.par], b_first = io.ctr[2], b_last = io.ctr[3];
    double pm[kFinRegBlocks], q[kFinRegBlocks][kFinMomPer];
    bool has[kFinRegBlocks];
    fin_load_partials<true, kFinMomPer>(dp, 0, nb, 2 + g * kFinMomPer, 0, pm, q, has);
    __asm__ volatile("" ::: "memory");                  // requested before the step is looked at
    if (fin_full_path(fs.full, st, b_first, b_last) || st >= io.cap) return;
    const double mlane = fin_lane_max(pm, has);
    const double wm = wave_max_f64(mlane);
    if (lane == 0) s_wmax[wave] = wm;
    double acc[kFinMomPer];
    fin_lane_sums<2>(pm, q, has, mlane, true, acc);     // (any of the moments: quantity >= 2)
    __syncthreads();                                     // s_wmax
    const double M = fin_wg_max(s_wmax);
    fin_rescale_store<2, kFinMomPer>(acc, mlane, M, true, s_q);
    __syncthreads();
    if (wave < kFinMomPer) {
        const double r = fin_row_sum_rows(s_q[wave]);
        if (lane == 0) fs.mom[st].tot[2 + g * kFinMomPer + wave] = r;
    }
#ifdef SLAM_FIN_PROBE
    __syncthreads();
    if (tid == 0) g_fin_probe[24 + g] = wall_clock64();
#endif
}

template <bool SLICED>
__global__ __launch_bounds__(kFinThreads) void finalize_fast_kernel(
    const int64_t n, const DeferParts dp, const double* __restrict__ w_un,
    double* __restrict__ s_cur, const int32_t* __restrict__ tail_leaves,
    const int32_t* __restrict__ tail_ops, const int32_t n_tail_leaves, const int32_t n_tail_ops,
    const double* __restrict__ xs, const double* __restrict__ ys, const double* __restrict__ ts,
    double* __restrict__ refp, int32_t* __restrict__ flags, const double ess_th, StepIO io,
    const int32_t resampled_known, const double np_recip, double* __restrict__ boff,
    const FinSlices sl, const FinSplit fs) {
    static_assert(kFinThreads == 512 && kFinRegBlocks == 4, "the register layout of fin_blk");
    static_assert(kFinSlBuf * kFinThreads + kFinBufPerRound >= 2048, "every buffer of sh");
    static_assert((kFinFastSlices - 1) * 11 <= kFinThreads, "one slice sum per lane");
    __shared__ double s_slm[kFinFastSlices];
    __shared__ double s_slq[kFinFastSlices][11];
    __shared__ int32_t s_slnc[kFinFastSlices];
    __shared__ double s_slu[kFinFastSlices];
    __shared__ double sh[2048];                      // buffer values / tail leaves / block totals
    __shared__ double s_q[11][kFinThreads];
    __shared__ BlockPartial shp[kFinWaves];
    __shared__ double s_wmax[kFinWaves];
    __shared__ double s_tot[11];
    __shared__ double s_s;
    __shared__ unsigned long long s_min;
    __shared__ int32_t s_flag;
    __shared__ int32_t s_next;      // resample_next: a word of its own (a wave still at
                                    // the tie decision's s_flag must not read it)
    __shared__ int64_t s_mi;
    __shared__ double s_xe[3];
    __shared__ int s_ncand;
    __shared__ int64_t s_cblk[kFinCand];
    __shared__ FinRecord s_crec[kFinCand];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nb = (n + kPartPer - 1) / kPartPer;
    const int64_t nfull = n / kSumChunk;
    const int64_t nch = (n + kSumChunk - 1) / kSumChunk;
    if constexpr (!SLICED) {
        if (blockIdx.x > 0) {
            fin_moment_group((int)blockIdx.x - 1, nb, dp, io, fs, s_q, s_wmax);
            return;
        }
    }
#ifdef SLAM_FIN_PROBE
    const long long probe_t0 = wall_clock64();
#endif
    // the step, the batch's bounds, the flag words and the reference the
    // record reads: every lane loads the same words into its own registers,
    // first in its queue, and waits for them only where they are used (the
    // path decision after the loads are out, the record at the end) --
    // through an offset the compiler cannot see as uniform, or it reads them
    // into scalar registers at once, a round trip ahead of the leaves on the
    // wave that runs the chain
    int uni_ofs = 0;
    __asm__ volatile("" : "+v"(uni_ofs));
    const int4 cw = *reinterpret_cast<const int4*>(io.ctr + uni_ofs);
    const int32_t st_now = cw.x, rstep = cw.y, b_first = cw.z, b_last = cw.w;
    static_assert(kFlagResample == 0 && kFlagStatus == 1 && kFlagNSpecial == 2 && kFlagMarkGen == 4 &&
                      kFlagDDWaves == 7 && kFlagWords == 8, "the flag words as two 16-byte loads");
    const int4 fa = *reinterpret_cast<const int4*>(flags + uni_ofs);
    const int4 fb = *reinterpret_cast<const int4*>(flags + 4 + uni_ofs);
    const FlagWords fw{fa.x, fa.y, fa.z, fb.w, fb.x};
    const double2 rp01 = *reinterpret_cast<const double2*>(refp + uni_ofs);
    const double rp[3] = {rp01.x, rp01.y, refp[2 + uni_ofs]};
    if (tid == 0) {
        s_ncand = 0;
        s_min = ~0ull;
        s_flag = 0;
    }
    const FinArgmaxLds am{&s_min, &s_flag, &s_mi, s_xe, &s_ncand, s_cblk, s_crec};
    // ---- loads: the leaves, then the partials of the lane's blocks
    // fin_blk(tid, k), the step context, the flag words
    // SLICED: the slices' buffer values first (the chain reads them right after
    // the first round's), then the leaves
    const int nsl = SLICED ? sl.nsl : 1;
    double bufv[kFinSlBuf] = {};
    if constexpr (SLICED) {
#pragma unroll
        for (int k = 0; k < kFinSlBuf; ++k) {
            const int64_t c = kFinBufPerRound + tid + (int64_t)kFinThreads * k;
            if (c < nfull) bufv[k] = sl.buf[c];
        }
        __asm__ volatile("" ::: "memory");
    }
    const int part = tid & (kFinLeafLanes - 1);
    double L[4];
    {
        const int64_t c = tid / kFinLeafLanes;
        const double* Lp = dp.leaf() + 16 * (c < nfull ? c : 0) + 4 * part;
#pragma unroll
        for (int j = 0; j < 4; ++j) L[j] = Lp[j];
        __asm__ volatile("" ::: "memory");              // the leaves' loads issue first
    }
    double pm[kFinRegBlocks], q[kFinRegBlocks][11];
    bool has[kFinRegBlocks];
    fin_load_partials<true, 0>(dp, 0, nb, 0, 0, pm, q, has);    // the block maxima
    __asm__ volatile("" ::: "memory");                  // then the partial sums
    fin_load_partials<false, 2>(dp, 0, nb, 0, 0, pm, q, has);   // sum u (the prefix), sum u^2 (the ESS)
    // the covariance moments: here on the full path only (a split step end
    // leaves them to the moment workgroups); the path is known once the step
    // counters are in, by when every load above is out
    __asm__ volatile("" ::: "memory");
    const bool full = SLICED || __builtin_amdgcn_readfirstlane((int)(
        fin_full_path(fs.full, st_now, b_first, b_last) || st_now >= io.cap)) != 0;
    const int nq = full ? 11 : 2;
    if (full) {
        fin_load_partials<false, 9>(dp, 0, nb, 2, 2, pm, q, has);
    } else {
#pragma unroll
        for (int k = 0; k < kFinRegBlocks; ++k) {
#pragma unroll
            for (int j = 2; j < 11; ++j) q[k][j] = 0.0;
        }
    }
#ifdef SLAM_FIN_PROBE
    const int pb = full ? 0 : 16;
    if (tid == 0) g_fin_probe[pb] = probe_t0;
#endif
    // SLICED: the slices' maxima, candidate lists and sums
    double slm = -1.0, slq = 0.0, ccp = -1.0, slu = 0.0;
    int64_t ccb = -1;
    int32_t sncv = 0;
    if constexpr (SLICED) {
        if (tid >= 1 && tid < nsl) {
            slm = sl.m[tid];
            sncv = sl.ncand[tid];
            slu = sl.u[tid];
        }
        if (tid < (nsl - 1) * kSliceCand) {
            const int g = 1 + tid / kSliceCand;
            ccb = sl.cblk[g * kSliceCand + tid % kSliceCand];
            ccp = sl.cpm[g * kSliceCand + tid % kSliceCand];     // unlisted: -1
        }
        if (tid < (nsl - 1) * 11) slq = sl.q[11 + tid];
    }
    // every load above is issued before the first use of a leaf (the scheduler
    // would otherwise wait for the leaves between them)
    __asm__ volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 4; ++j) __asm__ volatile("" : "+v"(L[j]));
#pragma unroll
    for (int k = 0; k < kFinSlBuf; ++k) __asm__ volatile("" : "+v"(bufv[k]));
    // ---- np.sum's buffer values (one round of <= 128 buffers, pairwise inside)
    {
        const int64_t c = tid / kFinLeafLanes;
        const double v = fin_buffer_value(L, c < nfull);
        if (part == 0 && c < nfull) sh[c] = v;
    }
    if constexpr (SLICED) {
#pragma unroll
        for (int k = 0; k < kFinSlBuf; ++k) {
            const int64_t c = kFinBufPerRound + tid + (int64_t)kFinThreads * k;
            if (c < nfull) sh[c] = bufv[k];
        }
    }
    __syncthreads();                                     // sh
    FIN_STAMP_AT(pb, 1);
    double s = 0.0;
    if (tid == 0 && nfull > 0) {
        // the buffers left to right while the other waves take their partials
        // (a whole wave walking the lanes by readlane measured slower: 14.9
        // against 8.8 us for the 1,024 buffers of 2^23)
        __builtin_amdgcn_s_setprio(3);
        s = lds_chain_sum(s, sh, (int)nfull);
        __builtin_amdgcn_s_setprio(0);
    }
    // ---- block maxima; each wave's argmax candidates (into registers: the
    // lane's first block within 2^-48 of the wave's max)
    const double mlane = fin_lane_max(pm, has);
    const double wm = wave_max_f64(SLICED ? fmax(mlane, slm) : mlane);   // + the slices' maxima
    if (lane == 0) s_wmax[wave] = wm;
    if constexpr (SLICED) {
        if (tid < nsl) {
            s_slm[tid] = slm;
            s_slnc[tid] = sncv;
            s_slu[tid] = slu;
        }
        if (tid < (nsl - 1) * 11) s_slq[1 + tid / 11][tid % 11] = slq;
    }
    double cpm = -1.0;
    int64_t cblk = -1;
#pragma unroll
    for (int k = kFinRegBlocks - 1; k >= 0; --k) {
        if (has[k] && pm[k] >= wm * (1.0 - 0x1p-48)) {
            cpm = pm[k];
            cblk = fin_blk(tid, k);
        }
    }
    FinRecord cr{};
    if (cblk >= 0) fin_load_record(dp, cblk, cr);
    __asm__ volatile("" ::: "memory");                  // requested before the sums wait
    // ---- lane partial sums scaled to the lane's max
    double acc[11];
    fin_lane_sums<0>(pm, q, has, mlane, full, acc);
    __syncthreads();                                     // s_wmax
    const double M = fin_wg_max(s_wmax);
    fin_rescale_store<0, 11>(acc, mlane, M, full, s_q);
    if (cblk >= 0 && cpm >= M * (1.0 - 0x1p-48)) fin_stage_candidate(am, dp, cblk, &cr);
    // SLICED: the listed candidates of the slices, records staged the same way
    const bool slc = SLICED && ccb >= 0 && ccp >= M * (1.0 - 0x1p-48);
    if (slc) {
        FinRecord f;
        fin_load_record(dp, ccb, f);
        fin_stage_candidate(am, dp, ccb, &f);
    }
    if (nch > nfull) {
        __syncthreads();                                 // sh reused by the tail
        const double tsum = tail_chunk_sum(w_un + nfull * kSumChunk, tail_leaves, tail_ops,
                                           n_tail_leaves, n_tail_ops, sh);
        if (tid == 0) s = s + tsum;
    }
    if (tid == 0) s_s = s;
    __syncthreads();
    s = s_s;
    FIN_STAMP_AT(pb, 2);
    const bool ok = (s > 0.0) && !isinf(s) && (M > 0.0);
    BlockPartial tot;
    bp_zero(tot);
    if (ok) {
        // ---- the 11 sums: wave w reduces quantities w and w + 8 (lane-strided
        // reads, then the wave's rows by DPP: a fixed order, no LDS permutes)
        // (a split step end: sum u and sum u^2 only, one round)
        for (int j = wave; j < nq; j += kFinWaves) {
            const double r = fin_row_sum_rows(s_q[j]);
            if (lane == 0) s_tot[j] = r;
        }
        if constexpr (SLICED) {                         // + the slices, rescaled to M, in order
            __syncthreads();
            if (tid < 11) s_tot[tid] = fin_fold_slices(s_tot[tid], tid, nsl, M, s_slm, &s_slq[0][0]);
        }
        // ---- argmax: the first block whose max rounds to fl(M / s)
        const double mval = M / s;
        unsigned long long cb = ~0ull;
#pragma unroll
        for (int k = kFinRegBlocks - 1; k >= 0; --k)
            if (has[k] && pm[k] >= M * (1.0 - 0x1p-48) && pm[k] / s == mval)
                cb = (unsigned long long)fin_blk(tid, k);
        if constexpr (SLICED) {
            if (slc && ccp / s == mval) cb = min(cb, (unsigned long long)ccb);
            // a slice with more candidates than it listed: all of its blocks
            for (int g = 1; g < nsl; ++g) {
                if (s_slnc[g] > kSliceCand && s_slm[g] >= M * (1.0 - 0x1p-48)) {
                    double v[kFinRegBlocks];
#pragma unroll
                    for (int k = 0; k < kFinRegBlocks; ++k) {
                        const int64_t b = (int64_t)g * kFinThreads * kFinRegBlocks + fin_blk(tid, k);
                        v[k] = b < nb ? dp.pmax()[b] : -1.0;
                    }
#pragma unroll
                    for (int k = kFinRegBlocks - 1; k >= 0; --k) {
                        const int64_t b = (int64_t)g * kFinThreads * kFinRegBlocks + fin_blk(tid, k);
                        if (b < nb && v[k] / s == mval) cb = min(cb, (unsigned long long)b);
                    }
                }
            }
        }
        fin_argmax_resolve(am, cb, n, s, mval, np_recip, dp, w_un, xs, ys, ts);
        if (tid == 0) {
            const double f = M / s;                      // back from max-relative to w_un / s
            tot.maxv = mval;
            tot.maxi = s_mi;
            tot.sw2 = s_tot[1] * (f * f);
            if (full) {
                moments_from_totals(s_tot, f, tot.sw, tot.m1, tot.m2);
            } else {
                // split: the raw totals this workgroup holds; the moment
                // workgroups store theirs, the record's reader forms cov
                fs.mom[st_now].tot[0] = s_tot[0];
                fs.mom[st_now].tot[1] = s_tot[1];
            }
        }
    } else {
        tot = fin_degenerate_pass(n, w_un, s, np_recip, xs, ys, ts, refp, shp, s_xe);
    }
    FIN_STAMP_AT(pb, 3);
    // the batch's last step exports the batch's records (a full step end)
    const bool exp = io.res_host != nullptr && st_now == b_last && b_first <= b_last;
    if (tid == 0) {
        // the record holds its cov unless this is a split step end that went well
        const bool with_cov = full || !ok;
        s_next = write_result_fw(tot, s_xe, refp, rp, s, flags, fw, ess_th, io.ess_band,
                                 io.res + st_now, resampled_known, exp ? io.res_host + st_now : nullptr,
                                 with_cov);
        if constexpr (!SLICED) {
            if (st_now < io.cap) {
                fs.mom[st_now].state = with_cov ? kMomComplete : kMomPending;
                if (exp) fs.mom_host[st_now].state = kMomComplete;
            }
            io.ctr[kCtrMom + (1 - fs.par)] = st_now + 1;   // the next launch's moment workgroups
        }
        io.ctr[0] = st_now + 1;
        io.ctr[1] = rstep + 1;
        *s_cur = s;
    }
    __syncthreads();
    FIN_STAMP_AT(pb, 4);
    fin_export_records(io, exp, b_first, st_now);
    if constexpr (!SLICED) {
        if (exp && tid >= 64) {
            // and their moment entries (complete by the kernel boundary), as words
            constexpr int kW = (int)(sizeof(FinMoments) / 8);
            const uint64_t* src = reinterpret_cast<const uint64_t*>(fs.mom + b_first);
            uint64_t* dst = reinterpret_cast<uint64_t*>(fs.mom_host + b_first);
            const int32_t words = (st_now - b_first) * kW;
            for (int32_t k = tid - 64; k < words; k += kFinThreads - 64) dst[k] = src[k];
        }
    }
    if (s_next) {
        double q0[kFinRegBlocks];
#pragma unroll
        for (int k = 0; k < kFinRegBlocks; ++k) q0[k] = q[k][0];
        if (SLICED && ok) {
            // the slices' own prefixes (finalize_slices_kernel), w_un units:
            // slice 0 from the registers the same way, then every block's
            // (U_0 + ... + U_{g-1} + pre_b) / s
            // slices g >= 1: block 2048 + tid + 512 i (slice 1 + i / 4, coalesced),
            // the first batch of 32 requested before the prefix's barrier
            const int nrest = (nsl - 1) * kFinRegBlocks;
            constexpr int kB = 32;
            auto pre_batch = [&](const int i0, double (&pv)[kB]) {
#pragma unroll
                for (int i = 0; i < kB; ++i) {
                    const int64_t b = (int64_t)kFinThreads * kFinRegBlocks + tid + (int64_t)kFinThreads * (i0 + i);
                    pv[i] = (i0 + i < nrest && b < nb) ? sl.pre[b] : 0.0;
                }
            };
            double pv[kB];
            pre_batch(0, pv);
            double u0[2], pex[2], tot[2];
            fin_pair_prefix(pm, q0, has, 1.0, &s_q[0][0], pex, u0, tot);
            const double rs = 1.0 / s;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int64_t b = fin_blk(tid, 2 * hf);
                if (b + 1 < nb)
                    *reinterpret_cast<double2*>(boff + b) = double2{pex[hf] * rs, (pex[hf] + u0[hf]) * rs};
                else if (b < nb)
                    boff[b] = pex[hf] * rs;
            }
            // U_0 + ... + U_{g-1} for every slice (every lane, in slice order)
            double ubs[kFinFastSlices];
            ubs[0] = 0.0;
            ubs[1] = tot[0] + tot[1];
#pragma unroll
            for (int g = 2; g < kFinFastSlices; ++g) ubs[g] = (g - 1 < nsl) ? ubs[g - 1] + s_slu[g - 1] : ubs[g - 1];
            double utot = ubs[1];
#pragma unroll
            for (int g = 1; g < kFinFastSlices; ++g)
                if (g < nsl) utot = utot + s_slu[g];
#pragma unroll
            for (int i0 = 0; i0 < (kFinFastSlices - 1) * kFinRegBlocks; i0 += kB) {
                if (i0 < nrest) {
                    if (i0 > 0) pre_batch(i0, pv);
#pragma unroll
                    for (int i = 0; i < kB; ++i) {
                        const int64_t b = (int64_t)kFinThreads * kFinRegBlocks + tid + (int64_t)kFinThreads * (i0 + i);
                        if (i0 + i < nrest && b < nb) boff[b] = (ubs[1 + (i0 + i) / kFinRegBlocks] + pv[i]) * rs;
                    }
                }
            }
            if (tid == 0) boff[nb] = utot * rs;
        } else {
            fin_next_prefix(n, nb, ok, s, np_recip, pm, q0, has, w_un, dp, boff, sh, &s_q[0][0]);
        }
    }
    FIN_STAMP_AT(pb, 5);
}
