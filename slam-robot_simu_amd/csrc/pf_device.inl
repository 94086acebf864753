// pf_device.inl -- device helpers of the particle-filter kernels: wave / block
// scans, predict_particle, likelihood_lanes.  Functions and templates only (no
// kernel, no exported symbol), so that pf_kernels.inl (pf_api.hip) and
// pf_batch.inl (pf_batch_api.hip) can both include it.
//
// The single-handle step these serve:
//
// Step = fused [systematic-resample gather +] predict + likelihood ->
//        numpy-order chunk sums -> normalise + reductions + result record.
// The exact sequential cumsum that feeds the resample gather is computed by
// the scan_* passes (launched at the start of a step; they gate on the
// device resample flag, so a device-resident run needs no host decisions).
// Particles are SoA fp64 (x[], y[], th[]) in HBM, one particle per lane.
#include <type_traits>

#include "pf_kernels.hpp"

// Phase stamps of the resample passes (probe builds only: -DSLAM_PROBE,
// read back with slam_probe_read; never in the product library).  PROBE_MAX
// samples every 32nd block: one atomic word taking every block's stamp
// serialises them (~12 ns each) and would time itself.
#ifdef SLAM_PROBE
__device__ unsigned long long g_probe[32];
#define PROBE_AT(k) do { if (threadIdx.x == 0) g_probe[k] = wall_clock64(); } while (0)
#define PROBE_MAX(k) do { if (threadIdx.x == 0 && (blockIdx.x & 31) == 0) atomicMax(&g_probe[k], (unsigned long long)wall_clock64()); } while (0)
#else
#define PROBE_AT(k) do { } while (0)
#define PROBE_MAX(k) do { } while (0)
#endif

namespace slam {

// Fused-kernel phase stamps (probe builds only: -DSLAM_PROBE_FUSED): per block,
// wave 0's wall clock at entry, after the table staging, after the normals,
// after predict (its loads consumed), after the likelihood and at the end.
#ifdef SLAM_PROBE_FUSED
constexpr int kFProbeBlocks = 1 << 14;
__device__ unsigned long long g_fprobe[kFProbeBlocks * 8];
#define FPROBE(k, dep) do { asm volatile("" :: "v"(dep)); \
    if (threadIdx.x == 0 && blockIdx.x < kFProbeBlocks) g_fprobe[blockIdx.x * 8 + (k)] = wall_clock64(); } while (0)
#else
#define FPROBE(k, dep) do { } while (0)
#endif

#ifdef SLAM_PROBE_COUNT_SLOW
__device__ unsigned long long g_probe_slow[2];   // slow particles, blocks with any (probe builds)
#endif

// ====================================================================
// wave / block helpers (wave = 64 lanes)
// ====================================================================
// DPP row_shr:D of a 32- or 64-bit integer; lanes without a source read 0
template <int D, typename T>
__device__ __forceinline__ T dpp_row_shr0(const T v) {
    constexpr int kCtrl = 0x110 + D;
    if constexpr (sizeof(T) == 8) {
        const uint64_t u = (uint64_t)v;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, kCtrl, 0xF, 0xF, false);
        const uint32_t hi =
            (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), kCtrl, 0xF, 0xF, false);
        return (T)(((uint64_t)hi << 32) | lo);
    } else {
        return (T)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
    }
}
template <typename T>
__device__ __forceinline__ T readlane_int(const T v, const int l) {
    if constexpr (sizeof(T) == 8) {
        const uint64_t u = (uint64_t)v;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
        return (T)(((uint64_t)hi << 32) | lo);
    } else {
        return (T)__builtin_amdgcn_readlane((int)v, l);
    }
}

// inclusive wave scan.  Integers (exact in any order): Hillis-Steele inside
// each 16-lane row by DPP row shifts, then the lower rows' totals read into
// scalars; floating point keeps the lane-shuffle order.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    if constexpr (std::is_integral<T>::value) {
        v += dpp_row_shr0<1>(v);
        v += dpp_row_shr0<2>(v);
        v += dpp_row_shr0<4>(v);
        v += dpp_row_shr0<8>(v);
        const T r0 = readlane_int(v, 15), r1 = readlane_int(v, 31), r2 = readlane_int(v, 47);
        const int row = (int)((threadIdx.x & 63) >> 4);
        v += (row >= 1 ? r0 : T(0)) + (row >= 2 ? r1 : T(0)) + (row >= 3 ? r2 : T(0));
        return v;
    } else {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            T o = __shfl_up(v, d, 64);
            if (lane >= d) v = v + o;
        }
        return v;
    }
}

// Exclusive wave scan of non-negative doubles in the integer scan's order (DPP
// row shifts, then the lower rows' totals: ~6x shorter in latency than the
// shuffle form; any fixed order serves an approximate prefix), formed
// without a subtraction (inc - v loses a small prefix ahead of a large
// element: its relative error is unbounded, which the exact cumsum's margins
// do not cover); `total` = the wave's sum (every lane).
__device__ __forceinline__ double wave_excl_scan_rows(double v, double& total) {
    auto sh = [](double x, auto d) {
        return __longlong_as_double((long long)dpp_row_shr0<decltype(d)::value>(
            (uint64_t)__double_as_longlong(x)));
    };
    v = v + sh(v, std::integral_constant<int, 1>{});
    v = v + sh(v, std::integral_constant<int, 2>{});
    v = v + sh(v, std::integral_constant<int, 4>{});
    v = v + sh(v, std::integral_constant<int, 8>{});
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const double r0 = __longlong_as_double((long long)readlane_int(b, 15));
    const double r1 = __longlong_as_double((long long)readlane_int(b, 31));
    const double r2 = __longlong_as_double((long long)readlane_int(b, 47));
    const double r3 = __longlong_as_double((long long)readlane_int(b, 63));
    const int row = (int)((threadIdx.x & 63) >> 4);
    double below = 0.0;
    if (row >= 1) below = r0;
    if (row >= 2) below = below + r1;
    if (row >= 3) below = below + r2;
    total = ((r0 + r1) + r2) + r3;
    const double prev = sh(v, std::integral_constant<int, 1>{});   // the row's inclusive, one lane down
    return (threadIdx.x & 15) ? below + prev : below;
}

// Sum over the wave in the same row order (every lane gets it): the rows'
// inclusive DPP scans, then ((row0 + row1) + row2) + row3.
__device__ __forceinline__ double wave_sum_rows(double v) {
    double total;
    (void)wave_excl_scan_rows(v, total);
    return total;
}

// Exclusive block scan over NT threads; sh needs NT/64+1 entries.  Returns the
// exclusive prefix of v, writes the block total to `total`.
template <typename T, int NT>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    T ex;
    if constexpr (std::is_integral<T>::value) {
        ex = inc - v;
    } else {
        ex = __shfl_up(inc, 1, 64);
        if (lane == 0) ex = T(0);
    }
    if (lane == 63) sh[wid] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = T(0);
        for (int k = 0; k < NT / 64; ++k) {
            const T t = sh[k];
            sh[k] = run;
            run = run + t;
        }
        sh[NT / 64] = run;
    }
    __syncthreads();
    const T r = sh[wid] + ex;
    total = sh[NT / 64];
    __syncthreads();
    return r;
}

// FMA-refined quotient x/d with rd = RN(1/d): q0 = RN(x*rd), r = x - d*q0
// (exact by FMA), q1 = RN(q0 + r*rd) -- the correctly rounded quotient for
// normal operands (Markstein); checked against IEEE division in the tests.
__device__ __forceinline__ double div_refined(double x, double d, double rd) {
    const double q0 = x * rd;
    const double r = fma(-q0, d, x);
    return fma(r, rd, q0);
}

// ---- write-through (sc1) hand-off words, MI355X_MICROARCH "Valid forms" row 1:
// the bytes one block hands to the last-arriving block are stored and loaded
// with agent-scope relaxed atomics (global_store/load ... sc1), the storing
// waves drain (vmcnt(0)) before the block barrier, one lane takes the ticket.
__device__ __forceinline__ void st_wt(void* p, uint64_t v) {
    __hip_atomic_store((uint64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_wt(const void* p) {
    return __hip_atomic_load((uint64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_wt_d(double* p, double v) { st_wt(p, (uint64_t)__double_as_longlong(v)); }
__device__ __forceinline__ double ld_wt_d(const double* p) { return __longlong_as_double((long long)ld_wt(p)); }
__device__ __forceinline__ void st_wt_i(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t ld_wt_i(const int32_t* p) {
    return __hip_atomic_load((int32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// SLAM_FUSED_WT (A/B switch, default 1): the deferred fused kernel's pair
// stores (x, y, th, w_un) write through on handles of at most
// SLAM_FUSED_WT_MAX particles -- the launch's output, 32 B per particle, then
// fits the 32 MiB of L2 -- and are plain stores above (the step
// is 2.7 % shorter at 2^20, even at 2^21, 1-4 % longer at 2^22 and 2^23);
// 0 = plain stores always, 2 = write-through always.
#ifndef SLAM_FUSED_WT
#define SLAM_FUSED_WT 1
#endif
#ifndef SLAM_FUSED_WT_MAX
#define SLAM_FUSED_WT_MAX (1 << 20)
#endif
// A particle pair (16 bytes, 16-byte aligned) as one write-through vector
// store: the line goes to memory while the kernel runs and is dropped from
// the XCD's L2, so nothing of it is left dirty for the kernel boundary to
// write back.  A wave's 64 pairs are eight whole 128-byte lines.
// The compiler does not pad an asm statement's hazards: the trailing s_nop
// keeps the next instruction off the data registers until the store has read
// them.  No wait and no fence: the next reader is the next launch.
__device__ __forceinline__ void st_wt_pair(double* p, const double a, const double b) {
    typedef double f64x2_t __attribute__((ext_vector_type(2)));
    const f64x2_t v = {a, b};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// The kernel's own argument segment as a struct A (A mirrors the kernel's
// parameter list, member for member), to read an argument where it is used
// and not at the kernel's start: a value loaded there occupies scalar registers up to
// its last use, and the fused kernel has none to spare.  The
// empty asm hides the address from the compiler, which would otherwise merge
// these loads with the entry's, and takes `after` (a lane value computed
// where the view is wanted) as an input, which keeps it and the loads behind
// that computation.  Not volatile: a volatile asm counts as a write to any
// address, and the wave-uniform loads of device memory behind it would become
// per-lane ones.  The segment is constant memory: its loads stay scalar even
// behind the write-through stores.
#define SLAM_KARG __attribute__((address_space(4)))
template <typename A>
__device__ __forceinline__ const SLAM_KARG A* kernarg_view(const double after) {
    uint64_t u = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm("" : "+s"(u) : "v"(after));
    return (const SLAM_KARG A*)u;
}
// a struct of the argument segment (or of anywhere) as a plain value
template <typename S, typename R>
__device__ __forceinline__ S karg_copy(const R& r) {
    S v;
    __builtin_memcpy(&v, &r, sizeof(S));
    return v;
}

template <typename S>
__device__ __forceinline__ void st_wt_struct(S* dst, const S& v) {
    static_assert(sizeof(S) % 8 == 0, "8-byte granules");
    const uint64_t* src = reinterpret_cast<const uint64_t*>(&v);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(S) / 8); ++k) st_wt(reinterpret_cast<uint64_t*>(dst) + k, src[k]);
}
template <typename S>
__device__ __forceinline__ S ld_wt_struct(const S* p) {
    S v;
    uint64_t* d = reinterpret_cast<uint64_t*>(&v);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(S) / 8); ++k) d[k] = ld_wt(reinterpret_cast<const uint64_t*>(p) + k);
    return v;
}

// ---- tagged granules (pf_kernels.hpp, the merged exact-cumsum hand-off): a
// granule validates itself, so neither side fences and nothing relies on the
// order in which granules become visible.
__device__ __forceinline__ void st_granule(uint64_t* p, const uint32_t payload, const uint32_t epoch) {
    st_wt(p, ((uint64_t)epoch << 32) | payload);
}
// A block's global offsets into its hand-off record: the two k granules in
// one 16-byte write-through store (each 8-byte half validates itself, so a
// store torn between them is harmless), the f granule in another -- a lane's
// write-through store is one fabric write whatever its size, and the last
// block issues every block's.
__device__ __forceinline__ void st_offsets_tagged(uint64_t* rec, const uint64_t k, const int32_t f,
                                                  const uint32_t epoch) {
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    const u32x4_t v = {(uint32_t)k, epoch, (uint32_t)(k >> 32), epoch};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(rec + kHandK0), "v"(v) : "memory");
    st_granule(rec + kHandF, (uint32_t)f, epoch);
}
// A folded special as kSpecGranules tagged granules
__device__ __forceinline__ void st_spec_tagged(uint64_t* tag, const int64_t m, const SpecialOut& o,
                                               const uint32_t epoch) {
    uint64_t* p = tag + m * kSpecGranules;
    const uint64_t cs = (uint64_t)__double_as_longlong(o.cs);
    st_granule(p + 0, (uint32_t)cs, epoch);
    st_granule(p + 1, (uint32_t)(cs >> 32), epoch);
    st_granule(p + 2, (uint32_t)o.P, epoch);
    st_granule(p + 3, (uint32_t)(o.P >> 32), epoch);
    st_granule(p + 4, (uint32_t)o.E, epoch);
}
// ... polled until every tag is this launch's epoch (bounded: `lost` if not)
__device__ __forceinline__ SpecialOut ld_spec_tagged(const uint64_t* tag, const int64_t m,
                                                     const uint32_t epoch, bool& lost) {
    const uint64_t* p = tag + m * kSpecGranules;
    SpecialOut o{};
    for (int it = 0; it < kHandSpin; ++it) {
        uint64_t g[kSpecGranules];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < kSpecGranules; ++k) g[k] = ld_wt(p + k);
#pragma unroll
        for (int k = 0; k < kSpecGranules; ++k) ok = ok && (uint32_t)(g[k] >> 32) == epoch;
        if (ok) {
            o.cs = __longlong_as_double((long long)((g[1] << 32) | (uint32_t)g[0]));
            o.P = (g[3] << 32) | (uint32_t)g[2];
            o.E = (int32_t)(uint32_t)g[4];
            return o;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    lost = true;
    return o;
}

// ---- last-arriver election (Guideline 16 / microarch "fanin" + "dequeue"):
// every block takes a ticket after publishing its write-through partials.
// One counter word serialises its arrivals (~12 ns each), so the tickets are
// two-level: blocks with equal blockIdx % 8 (one XCD under round-robin
// dispatch) share a counter on a 128-B line of its own, and the last of each
// residue class takes a ticket on the top word.  A ticket block is
// kTicketWords unsigned words; every word is re-zeroed by its last arriver.
constexpr int kTicketStride = 32;                       // 128 B
constexpr int kTicketWords = 9 * kTicketStride;

__device__ __forceinline__ bool arrive_last_n(unsigned* counter, const unsigned expected) {
    __shared__ int last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave drains
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t =
            __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == expected - 1) ? 1 : 0;
        if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return last != 0;
}

__device__ __forceinline__ int ticket_groups() { return gridDim.x < 8 ? (int)gridDim.x : 8; }

// level 1 of the two-level ticket: true in the last block of this residue class
__device__ __forceinline__ bool arrive_group(unsigned* tk) {
    const int G = ticket_groups(), g = blockIdx.x % G;
    const unsigned ng = (gridDim.x - g + G - 1) / G;
    return arrive_last_n(tk + (1 + g) * kTicketStride, ng);
}

__device__ __forceinline__ bool arrive_last(unsigned* tk) {
    if (!arrive_group(tk)) return false;
    return arrive_last_n(tk, (unsigned)ticket_groups());
}

// ---- systematic resampling positions (particle_filter.py:213-215)
__device__ __forceinline__ double resample_offset(const double ofs_host, const double np_recip,
                                                  const uint64_t seed, const uint32_t stepno) {
    if (!isnan(ofs_host)) return ofs_host;
    const u32x4 ctr{0u, 0u, kStreamResample, stepno};
    const u32x4 r = philox4x32(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t m = ((uint64_t)(r.x >> 5) << 26) | (uint64_t)(r.y >> 6);
    return ((double)m * 0x1p-53) * np_recip;                 // rand() * NP_RECIP
}

// first j in [0, n) with c[j] >= pos (the while loop of :218-220); n if none
__device__ __forceinline__ int64_t lower_bound_c(const double* __restrict__ c, const int64_t n,
                                                 const double pos) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (c[mid] < pos) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ====================================================================
// fused [resample gather +] predict + likelihood
//      (particle_filter.py:156-198, :216-222; motion_model.py:31-62)
// ====================================================================
// weight of the current step from the deferred representation:
// particle_filter.py:235-236  w = w_un / s, NaN -> 1/NP
__device__ __forceinline__ double norm_w(const double wu, const double s, const double np_recip) {
    const double v = wu / s;
    return isnan(v) ? np_recip : v;
}

// (value, index) max with the first index on ties (np.argmax)
__device__ __forceinline__ void max_first(double& v, int64_t& i, const double ov, const int64_t oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// ---- wave reductions through DPP lane moves (VALU, no LDS round trip):
// quad_perm [1,0,3,2] is the lane-xor-1 partner (bit-identical to
// __shfl_xor(v, 1)); max / min over the wave by quad swaps, the half-row and
// row mirrors, then the four row results read into scalars.
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(const uint64_t v) {
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(const double v) {
    return __longlong_as_double((long long)dpp_u64<CTRL>((uint64_t)__double_as_longlong(v)));
}
__device__ __forceinline__ uint64_t readlane_u64(const uint64_t v, const int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
// the lane-xor-d partner of a butterfly step (d a constant after unrolling):
// quad swaps by DPP for d = 1, 2, the LDS permute beyond
__device__ __forceinline__ double xor_f64(const double v, const int d) {
    if (d == 1) return dpp_f64<kDppXor1>(v);
    if (d == 2) return dpp_f64<kDppXor2>(v);
    return __shfl_xor(v, d, 64);
}
// inclusive max-scan of an int32 over the wave, and the exclusive value
// (lane 0: -1): row shifts by DPP (lanes without a source read -1), then the
// three lower rows' maxima read into scalars
__device__ __forceinline__ int32_t wave_max_scan_i32(int32_t v, int32_t& excl) {
    constexpr int kRowShr = 0x110;                                      // row_shr:d = 0x110 + d
    int32_t o;
    o = __builtin_amdgcn_update_dpp(-1, v, kRowShr + 1, 0xF, 0xF, false);
    v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(-1, v, kRowShr + 2, 0xF, 0xF, false);
    v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(-1, v, kRowShr + 4, 0xF, 0xF, false);
    v = o > v ? o : v;
    o = __builtin_amdgcn_update_dpp(-1, v, kRowShr + 8, 0xF, 0xF, false);
    v = o > v ? o : v;
    const int lane = (int)__lane_id(), row = lane >> 4;
    const int32_t r0 = __builtin_amdgcn_readlane(v, 15), r1 = __builtin_amdgcn_readlane(v, 31);
    const int32_t r2 = __builtin_amdgcn_readlane(v, 47);
    const int32_t m01 = r0 > r1 ? r0 : r1, m012 = m01 > r2 ? m01 : r2;
    const int32_t below = row == 0 ? -1 : row == 1 ? r0 : row == 2 ? m01 : m012;
    v = below > v ? below : v;
    // lane l - 1's inclusive value: within the row by row_shr:1, the row's
    // first lane takes the rows below
    const int32_t prev = __builtin_amdgcn_update_dpp(-1, v, kRowShr + 1, 0xF, 0xF, false);
    excl = (lane & 15) ? prev : below;
    return v;
}

// integer sums over the wave (every lane gets them; any order is exact)
__device__ __forceinline__ int32_t wave_sum_i32(int32_t v) {
    v += __builtin_amdgcn_mov_dpp(v, kDppXor1, 0xF, 0xF, false);
    v += __builtin_amdgcn_mov_dpp(v, kDppXor2, 0xF, 0xF, false);
    v += __builtin_amdgcn_mov_dpp(v, kDppHalfMirror, 0xF, 0xF, false);
    v += __builtin_amdgcn_mov_dpp(v, kDppMirror, 0xF, 0xF, false);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
           __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    v += dpp_u64<kDppXor1>(v);
    v += dpp_u64<kDppXor2>(v);
    v += dpp_u64<kDppHalfMirror>(v);
    v += dpp_u64<kDppMirror>(v);
    return readlane_u64(v, 0) + readlane_u64(v, 16) + readlane_u64(v, 32) + readlane_u64(v, 48);
}

// max over the wave (every lane gets it); fmax semantics as the butterfly's
__device__ __forceinline__ double wave_max_f64(double v) {
    v = fmax(v, dpp_f64<kDppXor1>(v));
    v = fmax(v, dpp_f64<kDppXor2>(v));
    v = fmax(v, dpp_f64<kDppHalfMirror>(v));
    v = fmax(v, dpp_f64<kDppMirror>(v));
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const double r0 = __longlong_as_double((long long)readlane_u64(b, 0));
    const double r1 = __longlong_as_double((long long)readlane_u64(b, 16));
    const double r2 = __longlong_as_double((long long)readlane_u64(b, 32));
    const double r3 = __longlong_as_double((long long)readlane_u64(b, 48));
    return fmax(fmax(r0, r1), fmax(r2, r3));
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
    int64_t o;
    o = (int64_t)dpp_u64<kDppXor1>((uint64_t)v);
    v = o < v ? o : v;
    o = (int64_t)dpp_u64<kDppXor2>((uint64_t)v);
    v = o < v ? o : v;
    o = (int64_t)dpp_u64<kDppHalfMirror>((uint64_t)v);
    v = o < v ? o : v;
    o = (int64_t)dpp_u64<kDppMirror>((uint64_t)v);
    v = o < v ? o : v;
    const int64_t r0 = (int64_t)readlane_u64((uint64_t)v, 0), r1 = (int64_t)readlane_u64((uint64_t)v, 16);
    const int64_t r2 = (int64_t)readlane_u64((uint64_t)v, 32), r3 = (int64_t)readlane_u64((uint64_t)v, 48);
    const int64_t a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
    return a < b ? a : b;
}

// Deferred-path epilogue of a 256-lane, kPartPer-particle fused block (see
// DeferParts).  Lane t holds particles kDeferPPT t + k (k < kDeferPPT); invalid
// ones carry w = 0.  Three barriers: (1) the wave maxima, (2) the lane-pair
// moment sums and the wave argmax candidates, (3) the segment sums and leaf
// accumulators.  Every sum has a fixed order: per lane over k, lane pairs
// (2l, 2l+1), 16 pair-strided segments of 8 (conflict-free LDS reads) left to
// right, then the 16 segments.
#ifndef SLAM_EPI_FMA
#define SLAM_EPI_FMA 0
#endif
__device__ void defer_epilogue(const int64_t base, const int64_t n, const double* wv,
                               const double* xv, const double* yv, const double* tv,
                               const double* __restrict__ refp, const DeferParts& dp,
                               const int wave_s, const int blk) {
    constexpr int kQ = 11;
    constexpr int kLeaves = kPartPer / 128;
    __shared__ double s_w[kPartPer];
    __shared__ double s_q[kQ * 128];
    __shared__ double s_seg[kQ * 16];
    __shared__ double s_acc[8 * kLeaves];
    __shared__ double s_mv[4], s_pre[4];
    __shared__ int64_t s_mi[4];
    // the thread index from the wave's SGPR index and the lane id (both
    // rematerialised: threadIdx.x itself would be held across the kernel)
    const int lane = (int)__lane_id(), wave = wave_s, t = (wave << 6) | lane;
    // lane max and its first particle, then the wave max
    double m = -1.0;
    int64_t mi = INT64_MAX;
#pragma unroll
    for (int k = 0; k < kDeferPPT; ++k) {
        const int64_t i = base + kDeferPPT * t + k;
        const bool ok = i < n;
        s_w[kDeferPPT * t + k] = ok ? wv[k] : 0.0;
        if (ok && wv[k] > m) {
            m = wv[k];
            mi = i;
        }
    }
    const double mv = wave_max_f64(m);
    if (lane == 0) s_mv[wave] = mv;
    __syncthreads();                                                    // (1)
    const double M = fmax(fmax(s_mv[0], s_mv[1]), fmax(s_mv[2], s_mv[3]));
    // first index holding M in this wave
    const int64_t cand = wave_min_i64((m == M) ? mi : INT64_MAX);
    if (lane == 0) s_mi[wave] = cand;
    // moments scaled by the block max, lane-pair sums into LDS
    const double rs = (M > 0.0) ? 1.0 / M : 0.0;
    const double r0 = refp[0], r1 = refp[1], r2 = refp[2];
    double q[kQ];
#pragma unroll
    for (int j = 0; j < kQ; ++j) q[j] = 0.0;
#pragma unroll
    for (int k = 0; k < kDeferPPT; ++k) {
        const bool ok = base + kDeferPPT * t + k < n;
        const double u = ok ? wv[k] * rs : 0.0;
        const double d0 = xv[k] - r0, d1 = yv[k] - r1, d2 = tv[k] - r2;
        const double ud0 = u * d0, ud1 = u * d1, ud2 = u * d2;
        q[0] += u;
        q[2] += ud0;
        q[3] += ud1;
        q[4] += ud2;
#if SLAM_EPI_FMA
        // the second moments as fused multiply-adds (one rounding each; the
        // partials are the filter's own, not the reference's: cov 1e-6)
        q[1] = fma(u, u, q[1]);
        q[5] = fma(ud0, d0, q[5]);
        q[6] = fma(ud0, d1, q[6]);
        q[7] = fma(ud0, d2, q[7]);
        q[8] = fma(ud1, d1, q[8]);
        q[9] = fma(ud1, d2, q[9]);
        q[10] = fma(ud2, d2, q[10]);
#else
        q[1] += u * u;
        q[5] += ud0 * d0;
        q[6] += ud0 * d1;
        q[7] += ud0 * d2;
        q[8] += ud1 * d1;
        q[9] += ud1 * d2;
        q[10] += ud2 * d2;
#endif
    }
#pragma unroll
    for (int j = 0; j < kQ; ++j) {
        const double o = dpp_f64<kDppXor1>(q[j]);
        q[j] = (lane & 1) ? o + q[j] : q[j] + o;                     // (2l) + (2l+1)
    }
    if (!(lane & 1)) {
#pragma unroll
        for (int j = 0; j < kQ; ++j) s_q[j * 128 + (t >> 1)] = q[j];
    }
    __syncthreads();                                                    // (2)
    // the block's first max index; the largest weight before it; x_est candidate
    int64_t bi = s_mi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) bi = s_mi[w] < bi ? s_mi[w] : bi;
    double pre = -1.0;
#pragma unroll
    for (int k = 0; k < kDeferPPT; ++k) {
        const int64_t i = base + kDeferPPT * t + k;
        if (i < bi) pre = fmax(pre, wv[k]);
        if (i == bi) {
            dp.pxe(0)[blk] = xv[k];
            dp.pxe(1)[blk] = yv[k];
            dp.pxe(2)[blk] = tv[k];
        }
    }
    pre = wave_max_f64(pre);
    if (lane == 0) s_pre[wave] = pre;
    if (t < kQ * 16) {
        // quantity t / 16, segment t % 16: pairs seg, seg + 16, ..., seg + 112
        const double* a = s_q + (t >> 4) * 128 + (t & 15);
        double acc = a[0];
#pragma unroll
        for (int mm = 1; mm < 8; ++mm) acc = acc + a[16 * mm];
        s_seg[t] = acc;
    } else if (t >= 192 && t < 192 + 8 * kLeaves) {
        // leaf (t-192)>>3, accumulator k = t & 7: elements k, k+8, ..., k+120
        const double* a = s_w + ((t - 192) >> 3) * 128 + (t & 7);
        double acc = a[0];
#pragma unroll
        for (int mm = 1; mm < 16; ++mm) acc = acc + a[8 * mm];
        s_acc[t - 192] = acc;
    }
    __syncthreads();                                                    // (3)
    if (t < kQ) {
        double acc = s_seg[16 * t];
        for (int mm = 1; mm < 16; ++mm) acc = acc + s_seg[16 * t + mm];
        dp.ps(t)[blk] = acc;
    } else if (t >= 64 && t < 128) {
        // the block's np.sum subtree: its kLeaves leaves, then their pair sums
        // (wave 1; lane l < kLeaves holds leaf l)
        double v = 0.0;
        if (t - 64 < kLeaves) {
            const double* r = s_acc + 8 * (t - 64);
            v = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        }
#pragma unroll
        for (int d = 1; d < kLeaves; d <<= 1) {
            const double o = xor_f64(v, d);
            v = (lane & d) ? (o + v) : (v + o);
        }
        if (t == 64) dp.leaf()[blk] = v;
    } else if (t == 128) {
        dp.pmax()[blk] = M;
        dp.pidx()[blk] = bi;
        dp.ppre()[blk] = fmax(fmax(s_pre[0], s_pre[1]), fmax(s_pre[2], s_pre[3]));
    }
}

// first j in [lo, hi) with c[j] >= pos, hi if none: the while loop of
// particle_filter.py:218-220 over the exact cumsum, restricted to a bracket
// known to hold the answer
__device__ __forceinline__ int64_t search_c(const double* __restrict__ c, int64_t lo, int64_t hi,
                                            const double pos) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (c[mid] < pos) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Predict one particle (particle_filter.py:129-140, :165-166; motion_model.py:
// 40-56) from its state and standard normals g, and give the likelihood the
// rotation of mylib/transform.py:31-33 for the predicted heading:
// ls = sin(pi/2 - th'), lc = cos(pi/2 - th').
//  * linear model: ls, lc from fast_sincos(pi/2 - th') exactly as the
//    reference forms them (the C1 parity path);
//  * velocity model: sin/cos(th + w dt) and sin/cos(th') by angle addition
//    from sin/cos(th) and the small turn increments w dt and gamma dt (two
//    kernel-only sin/cos instead of two range-reduced ones; within 2 ulp of
//    the direct evaluation).
// SLAM_TAB_SINCOS (default 1): the velocity model's sin/cos(th) from the LDS
// table (heading_sincos_tab) instead of fast_sincos.
#ifndef SLAM_TAB_SINCOS
#define SLAM_TAB_SINCOS 1
#endif
template <int MOTION>
__device__ __forceinline__ void predict_particle(const double x, const double y, const double th,
                                                 const double v, const double om, const double g0,
                                                 const double g1, const double g2,
                                                 const PredictConst& pc, double& xn, double& yn,
                                                 double& tn, double& ls, double& lc,
                                                 const RngTabs& T) {
    if (MOTION == kMotionNone) {           // likelihood-only entry (particle_filter.py:170)
        xn = x;
        yn = y;
        tn = th;
        fast_sincos(kHalfPi - tn, &ls, &lc);
    } else if (MOTION == SLAM_MOTION_LINEAR) {
        // particle_filter.py:129-140 then + v (:166); A = I, B = diag(V, V, w)
        double sn, cs;
        fast_sincos(th, &sn, &cs);
        const double a = pc.dt * cs;
        const double b = pc.dt * sn;
        xn = (x + v * a) + g0;
        yn = (y + v * b) + g1;
        tn = wrap_angle(th + om * pc.dt) + g2;
        fast_sincos(kHalfPi - tn, &ls, &lc);
    } else {
        // motion_model.py:40-56 (the std handed to normal() is sigma**2)
        const double v2 = v * v, w2 = om * om;
        const double sv = (pc.alphas[0] * v2) + (pc.alphas[1] * w2);
        const double sw = (pc.alphas[2] * v2) + (pc.alphas[3] * w2);
        const double sg = (pc.alphas[4] * v2) + (pc.alphas[5] * w2);
        const double vh = v + (0.0 + (sv * sv) * g0);
        const double wh = om + (0.0 + (sw * sw) * g1);
        const double gh = 0.0 + (sg * sg) * g2;
        const double a = vh / wh;
        const double b = wh * pc.dt;
        double s0, c0, sb, cb, s1, c1, se, ce;
#if SLAM_TAB_SINCOS
        heading_sincos_tab(th, T, &s0, &c0);
#else
        (void)T;
        fast_sincos(th, &s0, &c0);
#endif
        small_sincos(b, &sb, &cb);
        rotate_sc(s0, c0, sb, cb, &s1, &c1);                 // (th + w dt)
        xn = (x - (a * s0)) + (a * s1);
        yn = (y + (a * c0)) - (a * c1);
        tn = wrap_angle(th + (wh + gh) * pc.dt);
        small_sincos(gh * pc.dt, &se, &ce);
        rotate_sc(s1, c1, se, ce, &lc, &ls);                 // th' = th + w dt + gamma dt
    }
}

// double-double values (closed-form log-sum): explicit fma, -ffp-contract=off
struct dd_t {
    double h, l;
};
__device__ __forceinline__ dd_t dd_two_prod(const double a, const double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd_t dd_renorm(const double p, const double e) {
    const double r = p + e;
    return {r, e - (r - p)};
}
__device__ __forceinline__ dd_t dd_add2(const dd_t a, const dd_t b) {
    const double t = a.h + b.h;
    const double bb = t - a.h;
    return dd_renorm(t, ((a.h - (t - bb)) + (b.h - bb)) + (a.l + b.l));
}
__device__ __forceinline__ dd_t dd_mul_d(const dd_t a, const double b) {
    const double p = a.h * b;
    return dd_renorm(p, fma(a.h, b, -p) + a.l * b);
}
__device__ __forceinline__ dd_t dd_mul(const dd_t a, const dd_t b) {
    const double p = a.h * b.h;
    return dd_renorm(p, fma(a.h, b.h, -p) + (a.h * b.l + a.l * b.h));
}
__device__ __forceinline__ dd_t dd_scale(const dd_t a, const double p2) {   // p2 = +-2^k: exact
    return {a.h * p2, a.l * p2};
}
__device__ __forceinline__ dd_t dd_neg(const dd_t a) { return {-a.h, -a.l}; }

// ====================================================================
// per-step closed-form words (StepIO.zc slot, pf_kernels.hpp kZc*)
// ====================================================================
// Part 1 (every wave of a block, one sum per wave): the eight landmark /
// observation sums of the step as double-doubles in the fixed order of
// closed_lane_partial (64 lane partials, then a butterfly with the lower lane
// on the left), into sdd[16] (LDS).  The caller barriers before part 2.
__device__ void closed_prep_sums(const double* __restrict__ lm, const double* __restrict__ z,
                                 const int32_t nl, const int wave, const int nwaves, double* sdd) {
    const int lane = (int)__lane_id();
    for (int k = wave; k < 8; k += nwaves) {
        DDSum S = closed_lane_partial(k, lane, lm, z, nl);
#pragma unroll
        for (int d = 1; d < kClosedLanes; d <<= 1) {
            DDSum o;
            o.h = __shfl_xor(S.h, d, 64);
            o.l = __shfl_xor(S.l, d, 64);
            if ((lane & d) == 0) S = dd_join(S, o);
            else S = dd_join(o, S);
        }
        if (lane == 0) {
            sdd[2 * k] = S.h;
            sdd[2 * k + 1] = S.l;
        }
    }
}

// The expansion's reference pose for a step: the estimate two steps back (rp:
// x, y, th; refp[4..6] at the step's start, refp[0..2] at the previous step's
// end) moved `moves` times by the step's control, noise free (motion_model.py
// :64-86 / particle_filter.py:129-140): twice, or once for the first step after
// the handle's creation (refp[7] = 1: the initial pose is the particles' state
// before that step's predict).  Any finite pose gives exact constants; a close
// one keeps every particle on the fp64 expansion.
__device__ void closed_prep_reference(const double* rp, const int moves, const double v,
                                      const double om, const double dt, const int motion,
                                      double& px, double& py, double& pth) {
    px = rp[0];
    py = rp[1];
    pth = rp[2];
    if (!(isfinite(px) && isfinite(py) && fabs(pth) < 1e6)) px = py = pth = 0.0;
    for (int k = 0; k < moves; ++k) {
        double s0, c0;
        fast_sincos(pth, &s0, &c0);
        const double t1 = wrap_angle(pth + om * dt);
        const double a = v / om;
        if (motion == SLAM_MOTION_VELOCITY && om != 0.0 && isfinite(a)) {
            double s1, c1;
            fast_sincos(t1, &s1, &c1);
            px = (px - a * s0) + a * s1;
            py = (py + a * c0) - a * c1;
        } else if (isfinite(v)) {
            px = px + v * (dt * c0);
            py = py + v * (dt * s0);
        }
        if (isfinite(t1)) pth = t1;
    }
}

// Part 2 (one lane): the constants of the expansion about (p^, c^, s^) from the
// eight sums, each formed in double-double from the exact identities
//   l^ = l - p^:  L1 = S_l - NL p^,  L2 = S_ll - 2 p^.S_l + NL |p^|^2,
//   D^ = D - p^.S_z,  E^ = E - (p^_x S_zy - p^_y S_zx),
//   A = c^ L2 - D^,  B = s^ L2 - E^,  S_r = R^ L1 - S_z,
//   F^ = (c^^2 + s^^2) L2 - 2 (c^ D^ + s^ E^) + S_zz
// (F^ = sum_j |R^(l_j - p^) - z_j|^2, A = sum r^.l^, B = sum r^ x l^), then
// rounded (F^, A, B, L2 kept as double-doubles).
__device__ void closed_prep_constants(const double* sdd, const int32_t nl, const double px,
                                      const double py, const double pth, double* __restrict__ zc) {
    double sh, ch;
    fast_sincos(kHalfPi - pth, &sh, &ch);                 // mylib/transform.py:31
    const dd_t Sll{sdd[0], sdd[1]}, Slx{sdd[2], sdd[3]}, Sly{sdd[4], sdd[5]}, Szz{sdd[6], sdd[7]};
    const dd_t Szx{sdd[8], sdd[9]}, Szy{sdd[10], sdd[11]}, Dd{sdd[12], sdd[13]}, Ed{sdd[14], sdd[15]};
    const double fnl = (double)nl;
    const dd_t L1x = dd_add2(Slx, dd_neg(dd_two_prod(fnl, px)));
    const dd_t L1y = dd_add2(Sly, dd_neg(dd_two_prod(fnl, py)));
    const dd_t r2 = dd_add2(dd_two_prod(px, px), dd_two_prod(py, py));
    const dd_t t1 = dd_add2(dd_mul_d(Slx, px), dd_mul_d(Sly, py));
    const dd_t L2 = dd_add2(dd_add2(Sll, dd_scale(t1, -2.0)), dd_mul_d(r2, fnl));
    const dd_t Dh = dd_add2(Dd, dd_neg(dd_add2(dd_mul_d(Szx, px), dd_mul_d(Szy, py))));
    const dd_t Eh = dd_add2(Ed, dd_neg(dd_add2(dd_mul_d(Szy, px), dd_mul_d(Szx, -py))));
    const dd_t A = dd_add2(dd_mul_d(L2, ch), dd_neg(Dh));
    const dd_t B = dd_add2(dd_mul_d(L2, sh), dd_neg(Eh));
    const dd_t Srx = dd_add2(dd_add2(dd_mul_d(L1x, ch), dd_neg(dd_mul_d(L1y, sh))), dd_neg(Szx));
    const dd_t Sry = dd_add2(dd_add2(dd_mul_d(L1x, sh), dd_mul_d(L1y, ch)), dd_neg(Szy));
    const dd_t kk = dd_add2(dd_two_prod(ch, ch), dd_two_prod(sh, sh));
    const dd_t rr = dd_add2(dd_mul_d(Dh, ch), dd_mul_d(Eh, sh));
    const dd_t F = dd_add2(dd_add2(dd_mul(kk, L2), dd_scale(rr, -2.0)), Szz);
    for (int k = 0; k < 16; ++k) zc[kZcSum + k] = sdd[k];
    zc[kZcPx] = px;
    zc[kZcPy] = py;
    zc[kZcC] = ch;
    zc[kZcS] = sh;
    zc[kZcFh] = F.h;
    zc[kZcFl] = F.l;
    zc[kZcA] = A.h;
    zc[kZcAl] = A.l;
    zc[kZcB] = B.h;
    zc[kZcBl] = B.l;
    zc[kZcSrx] = Srx.h;
    zc[kZcSry] = Sry.h;
    zc[kZcL2] = L2.h;
    zc[kZcL2l] = L2.l;
    zc[kZcL1x] = L1x.h;
    zc[kZcL1y] = L1y.h;
}

// Both parts by one block (prestep / observation kernels): refp[4..6] = the
// estimate two steps back, refp[7] the moves from it (2; 1 after creation),
// (v, om) the step's control.
__device__ void closed_prep_block(const double* __restrict__ lm, const double* __restrict__ z,
                                  const int32_t nl, const double* refp, const double v,
                                  const double om, const double dt, const int motion,
                                  double* __restrict__ zc) {
    __shared__ double sdd[16];
    closed_prep_sums(lm, z, nl, (int)(threadIdx.x >> 6), (int)(blockDim.x >> 6), sdd);
    __syncthreads();
    if (threadIdx.x == 0) {
        double px, py, pth;
        closed_prep_reference(refp + 4, refp[7] == 1.0 ? 1 : 2, v, om, dt, motion, px, py, pth);
        closed_prep_constants(sdd, nl, px, py, pth, zc);
    }
}

// One landmark factor in the reference's rounding order
// (particle_filter.py:187-191: mylib/transform.py:31-35 then mlab.bivariate_normal).
template <int RHO = -1>
__device__ __forceinline__ double ref_q(const double xn, const double yn, const double sp,
                                        const double cp, const double lx, const double ly,
                                        const double zx, const double zy, const LikConst& lc);

// TAB: exp from the LDS table htab (product mode; exp_nhalf: the bits of
// exp_tab(-y/2), the table's values halved) instead of exp_lean.  Without
// rho, q >= 0 (a sum of two rounded non-negative quotients), so the argument
// is never positive.
// RHO: 1 / 0 when the caller has hoisted the lc.has_rho test out of its loop.
template <bool TAB = false, int RHO = -1>
__device__ __forceinline__ double ref_factor(const double xn, const double yn, const double sp,
                                             const double cp, const double lx, const double ly,
                                             const double zx, const double zy, const LikConst& lc,
                                             const double2* htab = nullptr) {
    const bool rho = RHO < 0 ? lc.has_rho : RHO > 0;
    const double q = ref_q<RHO>(xn, yn, sp, cp, lx, ly, zx, zy, lc);
    double e;
    if (rho) {
        const double a = (-q) / lc.d2;
        e = TAB ? exp_nhalf<false>(-2.0 * a, htab) : exp_lean(a);   // -2a exact: a's bits
    } else {
        e = TAB ? exp_nhalf<true>(q, htab) : exp_lean((-q) * 0.5);   // d2 == 2 exactly
    }
    return div_refined(e, lc.den, lc.rden);
}

// Log-sum slow path for one particle whose total L may leave the normal range
// somewhere along the reference's sequential product (particle_filter.py:192).
// Walk the log prefix s_j = log(f_1 ... f_j) to the first landmark j0 where it
// drops below ln(DBL_MIN) + 1: up to j0 - 1 the reference's partial product is
// a normal number equal to exp(s_{j0-1}); from j0 on, the factors are formed
// and multiplied exactly as the reference does (ref_factor), so the subnormal
// roundings and the zero set are the reference's.  Once the product is 0 it
// stays 0 (early exit).  The prefix uses the reference's residuals and q
// (ref_factor's rounding order) summed in double-double, so exp(s) is within
// ~1e-13 of the reference's normal-range partial product even for particles
// metres off every landmark (|s| ~ 700, where a plain fp64 chain of 100 sums
// is off by ~5e-12).
template <int RHO>
__device__ __forceinline__ double ref_q(const double xn, const double yn, const double sp,
                                        const double cp, const double lx, const double ly,
                                        const double zx, const double zy, const LikConst& lc) {
    const double dxw = lx - xn;
    const double dyw = ly - yn;
    const double rx = fma(-sp, dyw, cp * dxw);
    const double ry = fma(cp, dyw, sp * dxw);
    const double dx = rx - zx;
    const double dy = ry - zy;
    double q = div_refined(dx * dx, lc.sx2, lc.rsx2) + div_refined(dy * dy, lc.sy2, lc.rsy2);
    if (RHO < 0 ? lc.has_rho : RHO > 0) q = q - ((lc.rho2 * dx) * dy) / lc.sxsy;
    return q;
}

// double from/to lane l (uniform result, SGPR-held)
__device__ __forceinline__ double readlane_d(const double v, const int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// double-double a + b (TwoSum of the high parts, low parts added, renormalised)
__device__ __forceinline__ void dd_add(double& ah, double& al, const double bh, const double bl) {
    const double t = ah + bh;
    const double bb = t - ah;
    const double e = ((ah - (t - bb)) + (bh - bb)) + (al + bl);
    ah = t + e;
    al = e - (ah - t);
}

// One slow particle per WAVE (every lane passes the same particle): the log
// prefix of 64 landmarks at a time -- one ref_q per lane, a double-double
// inclusive wave scan plus the carry of the previous chunks -- then the first
// landmark j0 whose prefix leaves the normal range by ballot, and the exact
// tail from j0 (uniform across the wave).  A lane-serial walk of 100 landmarks
// is a ~10 us dependency chain; this one is a few hundred issue slots.
// inlined: a call costs the fused kernel 176 B of scratch and ~10 us per launch
#ifdef SLAM_SLOW_NOINLINE
#define SLAM_SLOW_ATTR __noinline__
#else
#define SLAM_SLOW_ATTR __forceinline__
#endif
__device__ SLAM_SLOW_ATTR double logsum_slow(const double xn, const double yn, const double sp,
                                           const double cp, const double* __restrict__ lm,
                                           const double* __restrict__ z, const LikConst& lc) {
    const int nl = lc.nl;
    const int lane = (int)__lane_id();
    double ch = 0.0, cl = 0.0;               // sum of q over the landmarks before this chunk
    double s_prev = 0.0;                     // log prefix before j0 (0: empty product = 1)
    int j0 = nl;
    for (int base = 0; base < nl; base += 64) {
        const int j = base + lane;
        double h = (j < nl) ? ref_q(xn, yn, sp, cp, lm[2 * j], lm[2 * j + 1], z[2 * j],
                                     z[2 * j + 1], lc)
                            : 0.0;
        double l = 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // inclusive scan, lower lanes on the left
            const double oh = __shfl_up(h, d, 64), ol = __shfl_up(l, d, 64);
            if (lane >= d) {
                double th = oh, tl = ol;
                dd_add(th, tl, h, l);
                h = th;
                l = tl;
            }
        }
        double th = ch, tl = cl;
        dd_add(th, tl, h, l);                // + the previous chunks
        const double sq = th + tl;
        const double sj = lc.has_rho ? fma(-sq, lc.rd2, (double)(j + 1) * lc.neg_ln_den)
                                     : fma(-0.5, sq, (double)(j + 1) * lc.neg_ln_den);
        const unsigned long long below = __ballot(j < nl && !(sj >= lc.normal_min_l));
        if (below) {
            const int f = __ffsll((long long)below) - 1;     // first lane below
            const double sp_lane = __shfl(sj, f > 0 ? f - 1 : 0, 64);
            j0 = base + f;
            if (f > 0) s_prev = sp_lane;                     // else the previous chunk's last
            break;
        }
        const int last = (nl - base < 64 ? nl - base : 64) - 1;
        s_prev = __shfl(sj, last, 64);
        ch = __shfl(th, 63, 64);
        cl = __shfl(tl, 63, 64);
    }
    // the exact tail: the factors of 64 landmarks at a time, one per lane,
    // then the reference's left-to-right product over them (round 5: the
    // factors used to be formed inside the serial loop, ~60 issue slots per
    // landmark for the whole wave -- several us per slow particle)
    double acc = exp_lean(s_prev);           // s_prev = 0 -> exactly 1 (j0 = 0)
#ifdef SLAM_SLOW_SERIAL_TAIL                                 // A/B diagnostic: the round-4 form
    for (int j = j0; j < nl; ++j) {
        acc = acc * ref_factor(xn, yn, sp, cp, lm[2 * j], lm[2 * j + 1], z[2 * j], z[2 * j + 1], lc);
        if (acc == 0.0) break;
    }
    return acc;
#endif
    for (int base = j0; base < nl && acc != 0.0; base += 64) {
        const int j = base + lane;
        const double f = (j < nl) ? ref_factor(xn, yn, sp, cp, lm[2 * j], lm[2 * j + 1], z[2 * j],
                                               z[2 * j + 1], lc)
                                  : 1.0;
        const int cnt = (nl - base < 64) ? nl - base : 64;
        for (int l = 0; l < cnt; ++l) {
            acc = acc * readlane_d(f, l);
            if (acc == 0.0) break;
        }
    }
    return acc;
}

// Likelihood of P particles of one lane (particle_filter.py:170-192 with
// mylib/transform.py:31-35 per landmark).  The landmark loop is shared: each
// landmark and observation is loaded once (scalar loads, uniform across the
// wave) and applied to the P particles, whose accumulators are independent
// dependency chains.  sp/cp: sin/cos(pi/2 - th) of each particle.
//
// LOGSUM: prod_j exp(-q_j/d2)/den = exp(L), L = -sum_j q_j/d2 - NL ln den, one
// exp per particle.  Two accumulators per particle (the x and y squares) keep
// the rounding of the sum within ~5e-13 relative of the weight on the fast path
// (a single chain reaches 8e-13 at L ~ -650 and 5e-12 at L ~ -700).  A particle whose L is
// below lc.fast_min_l -- where some partial product of the reference's
// sequential loop could have left the normal range (subnormal or zero) --
// takes logsum_slow instead, so the zero set and the subnormal roundings are
// the reference's (identical zero sets, <= 1e-12 relative).
// Returns 1 when one of the lane's particles took the closed form's
// double-double evaluation.
// LC: LikConst, or the fused kernel's in its argument segment (kernarg_view),
// whose words are then loaded where they are used; the helpers of the product
// mode and of the slow path take a plain copy.
template <int LIK, int P, typename LC>
__device__ __forceinline__ int likelihood_lanes(const double* xn, const double* yn,
                                                 const double* sp, const double* cp,
                                                 const double* __restrict__ lm,
                                                 const double* __restrict__ z,
                                                 const double* __restrict__ zc, const LC& lc_in,
                                                 double* bn, const int wave_s, const double* pw) {
    const int nl = lc_in.nl;
    if (LIK == SLAM_LIK_PRODUCT) {
        const LikConst lc = karg_copy<LikConst>(lc_in);
        // the exp table in LDS, t.x halved for exp_nhalf (every lane of the
        // block reaches this barrier)
        __shared__ double2 s_etab[64];
        if (threadIdx.x < 64) {
            const double2 t = kExpTab64[threadIdx.x];
            s_etab[threadIdx.x] = make_double2(t.x * 0.5, t.y);
        }
        __syncthreads();
        double acc[P];
#pragma unroll
        for (int k = 0; k < P; ++k) acc[k] = 1.0;
        // the rho test hoisted: the P particles' chains interleave in one block
        auto walk = [&](auto rho) {
            for (int j = 0; j < nl; ++j) {
                const double lx = lm[2 * j], ly = lm[2 * j + 1], zx = z[2 * j], zy = z[2 * j + 1];
#pragma unroll
                for (int k = 0; k < P; ++k)
                    acc[k] = acc[k] * ref_factor<true, decltype(rho)::value>(xn[k], yn[k], sp[k], cp[k], lx,
                                                                            ly, zx, zy, lc, s_etab);
            }
        };
        if (lc.has_rho) walk(std::integral_constant<int, 1>{});
        else walk(std::integral_constant<int, 0>{});
#pragma unroll
        for (int k = 0; k < P; ++k) bn[k] = acc[k];
        return 0;
    }
    const LC& lc = lc_in;
    double L[P];
    int lane_dd = 0;
    if (lc.closed) {
        // sum_j |R(l_j - p) - z_j|^2 in closed form (iso: q_j = that / sx2).
        // Fast form: the expansion about the step's reference pose (p^, c^, s^),
        // exact as a polynomial identity for any particle (x, y, c, s):
        //   d = p - p^, dc = c - c^, ds = s - s^, (u, v) = R(c, s) d,
        //   F = F^ + 2 (dc A + ds B) + (dc^2 + ds^2) L2            [rotation terms]
        //          - 2 S_r.(u, v) - 2 (dR L1).(u, v) + NL (u^2 + v^2),  dR = [[dc, -ds], [ds, dc]]
        // (DESIGN 4.3).  The rotation terms, which carry the cloud's heading
        // spread (|dc A| and dc^2 L2 reach ~10 while F ~ NL sx2), are formed to
        // ~u^2 from double-double dc, ds (TwoSum) and A, B, L2 (exact products,
        // TwoSum) and summed with F^ in double-double; the translation terms
        // round in fp64 within 11 u V, V = 2 (|gx u| + |gy v| + |Srx u| +
        // |Sry v|) + t5 their magnitudes, so V <= expand_vmax keeps |dL| <=
        // 3e-13 (the worst case; the measured difference to the double-double
        // form is ~1e-14).  Beyond it (a particle far from the reference pose) the
        // double-double form of the same sum from the eight sums.  Either way
        // the exact value of the sum for the particle's rounded c, s up to that
        // bound and one final rounding: the difference to the reference is its
        // own rounding (~1e-14 relative of the weight).
        const double fnl = (double)nl;
        const double phx = zc[kZcPx], phy = zc[kZcPy], chh = zc[kZcC], shh = zc[kZcS];
        const double Fh = zc[kZcFh], Fl = zc[kZcFl];
        const double Ah = zc[kZcA], Al = zc[kZcAl], Bh = zc[kZcB], Bl = zc[kZcBl];
        const double L2h = zc[kZcL2], L2l = zc[kZcL2l];
        const double Srx = zc[kZcSrx], Sry = zc[kZcSry];
        const double L1x = zc[kZcL1x], L1y = zc[kZcL1y];
        bool dd[P];
        int any_dd = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const double c = cp[k], sn = sp[k];
            const double dx = xn[k] - phx, dy = yn[k] - phy;
            const double dc = c - chh, ds = sn - shh;
            const double dcb = dc - c, dsb = ds - sn;                       // TwoSum errors of dc, ds
            const double dce = (c - (dc - dcb)) + (-chh - dcb);
            const double dse = (sn - (ds - dsb)) + (-shh - dsb);
            // rotation terms to ~u^2: 2 t1 = 2 (dc A + ds B), t3 = (dc^2 + ds^2) L2
            const double p1 = dc * Ah, e1 = fma(dc, Ah, -p1);
            const double p2 = ds * Bh, e2 = fma(ds, Bh, -p2);
            const double q1 = dc * dc, f1 = fma(dc, dc, -q1);
            const double q2 = ds * ds, f2 = fma(ds, ds, -q2);
            const double a2 = q1 + q2;
            const double a2b = a2 - q1;
            const double a2e = ((q1 - (a2 - a2b)) + (q2 - a2b)) + (f1 + f2);
            const double p3 = a2 * L2h;
            // + the low parts of dc, ds: 2 (dce dc + dse ds) in t3, (dce A + dse B) in t1
            const double a2x = a2e + 2.0 * fma(dce, dc, dse * ds);
            const double e3 = fma(a2, L2h, -p3) + fma(a2x, L2h, a2 * L2l);
            // translation terms in fp64: t2 = S_r . R d, t4 = dR L1 . R d, t5 = NL |R d|^2
            const double u = fma(c, dx, -(sn * dy));
            const double v = fma(sn, dx, c * dy);
            const double t2 = fma(Srx, u, Sry * v);
            const double gx = fma(dc, L1x, -(ds * L1y)), gy = fma(ds, L1x, dc * L1y);
            const double t4 = fma(gx, u, gy * v);
            const double t5 = fma(u, u, v * v) * fnl;
            // F^h + 2 p1 + 2 p2 + p3 by TwoSum, then every low part
            double h = Fh, lo;
            {
                const double b = 2.0 * p1, t = h + b, bb = t - h;
                lo = (h - (t - bb)) + (b - bb);
                h = t;
            }
            {
                const double b = 2.0 * p2, t = h + b, bb = t - h;
                lo += (h - (t - bb)) + (b - bb);
                h = t;
            }
            {
                const double t = h + p3, bb = t - h;
                lo += (h - (t - bb)) + (p3 - bb);
                h = t;
            }
            const double rot_lo =
                fma(2.0, (e1 + e2) + (fma(dc, Al, ds * Bl) + fma(dce, Ah, dse * Bh)), e3);
            lo = lo + ((Fl + rot_lo) + (fma(-2.0, t2 + t4, t5)));
            const double F = h + lo;
            const double V = fma(2.0, fma(fabs(u), fabs(gx) + fabs(Srx), fabs(v) * (fabs(gy) + fabs(Sry))), t5);
            dd[k] = !(V <= lc.expand_vmax);                                  // also NaN
            any_dd |= dd[k] ? 1 : 0;
            L[k] = nl ? fma(-0.5, F * lc.rsx2, lc.neg_nl_ln_den) : lc.neg_nl_ln_den;
        }
        lane_dd = any_dd;
        // (held as a lane value: as a lane mask it would occupy a scalar
        // register pair across the exp and the slow path below)
        asm("" : "+v"(lane_dd));
        if (any_dd) {
            const dd_t Sll{zc[0], zc[1]}, Slx{zc[2], zc[3]}, Sly{zc[4], zc[5]}, Szz{zc[6], zc[7]};
            const dd_t Szx{zc[8], zc[9]}, Szy{zc[10], zc[11]}, Dd{zc[12], zc[13]}, Ed{zc[14], zc[15]};
#pragma unroll
            for (int k = 0; k < P; ++k) {
                if (!dd[k]) continue;
                const double x = xn[k], y = yn[k], c = cp[k], sn = sp[k];
                const dd_t r2 = dd_add2(dd_two_prod(x, x), dd_two_prod(y, y));          // |p|^2
                const dd_t t1 = dd_add2(dd_mul_d(Slx, x), dd_mul_d(Sly, y));            // p . S_l
                const dd_t p1 = dd_add2(dd_add2(Sll, dd_scale(t1, -2.0)), dd_mul_d(r2, fnl));
                const dd_t kk = dd_add2(dd_two_prod(c, c), dd_two_prod(sn, sn));
                const dd_t q1 = dd_add2(Dd, dd_scale(dd_add2(dd_mul_d(Szx, x), dd_mul_d(Szy, y)), -1.0));
                const dd_t q2 = dd_add2(Ed, dd_scale(dd_add2(dd_mul_d(Szy, x), dd_mul_d(Szx, -y)), -1.0));
                const dd_t rr = dd_add2(dd_mul_d(q1, c), dd_mul_d(q2, sn));
                const dd_t acc = dd_add2(dd_add2(dd_mul(kk, p1), dd_scale(rr, -2.0)), Szz);
                L[k] = nl ? fma(-0.5, acc.h * lc.rsx2, lc.neg_nl_ln_den) : lc.neg_nl_ln_den;
            }
        }
    } else if (lc.iso) {
        double a[P][2];
#pragma unroll
        for (int k = 0; k < P; ++k) a[k][0] = a[k][1] = 0.0;
#pragma unroll 4
        for (int j = 0; j < nl; ++j) {
            const double lx = lm[2 * j], ly = lm[2 * j + 1], zx = z[2 * j], zy = z[2 * j + 1];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const double dxw = lx - xn[k];
                const double dyw = ly - yn[k];
                const double dx = fma(cp[k], dxw, fma(-sp[k], dyw, -zx));
                const double dy = fma(sp[k], dxw, fma(cp[k], dyw, -zy));
                a[k][0] = fma(dx, dx, a[k][0]);
                a[k][1] = fma(dy, dy, a[k][1]);
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) L[k] = fma(-0.5, (a[k][0] + a[k][1]) * lc.rsx2, lc.neg_nl_ln_den);
    } else {
        double a[P][2];
#pragma unroll
        for (int k = 0; k < P; ++k) a[k][0] = a[k][1] = 0.0;
        for (int j = 0; j < nl; j += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (j + h >= nl) break;
                const double lx = lm[2 * (j + h)], ly = lm[2 * (j + h) + 1];
                const double zx = z[2 * (j + h)], zy = z[2 * (j + h) + 1];
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const double dxw = lx - xn[k];
                    const double dyw = ly - yn[k];
                    const double dx = fma(cp[k], dxw, fma(-sp[k], dyw, -zx));
                    const double dy = fma(sp[k], dxw, fma(cp[k], dyw, -zy));
                    double q = fma(dx * lc.rsx2, dx, (dy * lc.rsy2) * dy);
                    if (lc.has_rho) q = q - ((lc.rho2 * dx) * dy) * lc.rsxsy;
                    a[k][h] = a[k][h] + q;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const double s = a[k][0] + a[k][1];
            L[k] = lc.has_rho ? fma(-s, lc.rd2, lc.neg_nl_ln_den) : fma(-0.5, s, lc.neg_nl_ln_den);
        }
    }
    bool slow[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        bn[k] = exp_lean(L[k]);
        slow[k] = !(L[k] >= lc.fast_min_l);                 // also NaN
        // a zero previous weight makes the weight 0 for any finite likelihood,
        // and below fast_min_l the likelihood is finite (a NaN L still goes
        // the reference's way): the exact product is not needed
#ifndef SLAM_NO_ZERO_SKIP                                   // A/B diagnostic
        if (slow[k] && pw[k] == 0.0 && !isnan(L[k])) {
            slow[k] = false;
            bn[k] = 0.0;
        }
#endif
#ifdef SLAM_PROBE_NO_SLOW                                  // timing probe only: not exact
        slow[k] = false;
#endif
    }
    // The few slow particles (bench workload: ~1,500 of 2^20 on every third
    // step, ~100 on the step after) are taken by their own wave, one at a
    // time with all 64 lanes on it: no block barrier and no LDS staging, so a
    // wave without one pays two ballots.  Wave-uniform loops.
#pragma unroll
    for (int k = 0; k < P; ++k) {
        unsigned long long m = __ballot(slow[k]);
#ifdef SLAM_PROBE_COUNT_SLOW                               // probe builds only
        if (__lane_id() == 0 && m) {
            atomicAdd(&g_probe_slow[0], (unsigned long long)__popcll(m));
            atomicAdd(&g_probe_slow[1], 1ull);
        }
#endif
        if (m) {
            const LikConst lcs = karg_copy<LikConst>(lc);
            do {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const double r = logsum_slow(__shfl(xn[k], l, 64), __shfl(yn[k], l, 64),
                                             __shfl(sp[k], l, 64), __shfl(cp[k], l, 64), lm, z, lcs);
                if ((int)__lane_id() == l) bn[k] = r;
            } while (m);
        }
    }
    return lane_dd;
}

}  // namespace slam
