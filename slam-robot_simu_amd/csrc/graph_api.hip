// graph_api.hip -- C-ABI of graph-based SLAM (include/slam_hip.h).
//
// TrajectoryEstimator (graph_based_slam.py:330-581) -> slam_graph_*.  The
// block structure of H and the per-block accumulation plan (which edge parts
// land in which 3x3 block, in the reference's edge order) are built on the
// device once per edge set (graph_build.inl: radix sorts, uniques, binary
// searches; SLAM_GRAPH_HOST_BUILD=1 builds the same arrays on the host, for
// the tests); every Gauss-Newton iteration then runs entirely on the device:
// linearise -> assemble -> solve -> pose update.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "device_mem.hpp"
#include "graph_kernels.inl"
#include "graph_build.inl"
#include "graph_marginals.inl"
#include "graph_members.inl"
#include "graph_map.inl"

using namespace slam;

constexpr int kGateInfo = 14;     // slam_graph_gate_info words

struct slam_graph {
    slam_graph_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    DeviceMem mem;
    DeviceMem dense;               // dense-path buffers (per edge set, small systems only)
    char* arena = nullptr;         // structure + solver buffers of the edge set (grow-only)
    size_t arena_bytes = 0;
    int64_t dense_n = 0;           // unknowns the dense buffers were sized for
    // poses
    int64_t T = 0;
    double* poses = nullptr;
    // edges and structure
    int64_t E = 0, nt = 0, n_slots = 0;
    int64_t E_lm = 0;              // landmark edges: columns [0, E_lm); odometry edges behind them
    std::vector<int64_t> times_h;
    slam_graph_edge* edges = nullptr;
    double* blocks = nullptr;      // [42][E]
    int64_t *times = nullptr, *srow = nullptr, *scol = nullptr, *rptr = nullptr;
    int64_t *cptr = nullptr, *clist = nullptr, *bptr = nullptr, *blist = nullptr;
    int64_t* dslot = nullptr;
    double *val = nullptr, *b = nullptr, *delta = nullptr, *dsum = nullptr;
    // dense path
    double *A = nullptr, *LU = nullptr, *S = nullptr, *V = nullptr, *lan = nullptr;
    int32_t* piv = nullptr;
    double* luout = nullptr;       // [0..2] LU, [3..4] Lanczos
    // PCG
    double *minv = nullptr, *r = nullptr, *z = nullptr, *p = nullptr;
    double* q = nullptr;
    double* part = nullptr;
    PcgState* st = nullptr;
    // condition-number estimate of the PCG path (second stream)
    hipStream_t cstream = nullptr;
    hipEvent_t cev[3] = {};        // [0] operands ready (main stream), [1]/[2] estimate start/end
    double *cx = nullptr, *chx = nullptr, *cp = nullptr, *chp = nullptr;
    double *cw = nullptr, *cw2 = nullptr, *chw = nullptr, *cpart = nullptr;
    CondState* cst = nullptr;
    int64_t* cnt_host = nullptr;   // pinned: the structure build's two counts, then its times
    int64_t cnt_cap = 0;           // (a pageable read-back stalled the host ~7 ms now and then)
    PcgState* pcg_host = nullptr;  // pinned copies of the device states: the polls of the
    CondState* cond_host = nullptr;  // two streams must not block the host (pageable copies do)
    bool cond_warm = false;        // cx holds the previous update's vectors of this edge set
    int32_t cond_last_iters = 0;
    double cond_info[7] = {0, 0, 0, 0, 0, 0, 0};
    // the gate's log-det sums (cond_mode SLAM_GRAPH_COND_MARGIN)
    double* cert_part = nullptr;   // per-workgroup partials of the certificate kernels
    CertState* cert = nullptr;
    CertState* cert_host = nullptr;  // pinned
    double gate_info[kGateInfo] = {};
    hipEvent_t ev[5] = {};
    double last[5] = {0, 0, 0, 0, 0};
    int32_t pcg_last_iters = 0;    // iteration count of the previous PCG solve
    bool pcg_failed = false;       // the last update's PCG solve did not converge
    bool assembled = false;        // val / b hold a system of the current edge set
    // slam_graph_marginals: its own buffers (first use, grow-only) and events
    DeviceMem marg;
    char* marg_arena = nullptr;
    size_t marg_bytes = 0;
    MargState* marg_host = nullptr;  // pinned
    hipEvent_t marg_ev[2] = {};
    int32_t marg_cols = 0;         // columns per pass (0: kMargDefaultCols)
    int32_t marg_last_iters = 0;   // iteration count of the previous pass (first batch length)
    // robust edge weights (slam_graph_set_robust): their own array
    // (first use, grow-only): [2][cap] rows (chi2, w) of the last linearisation,
    // [2][cap] of the last slam_graph_chi2, its partials and totals
    int32_t robust_kind = SLAM_GRAPH_ROBUST_NONE;
    double robust_param = 0.0;
    int32_t lin_kind = -1;         // kind of the last linearisation (-1: none since set_edges)
    DeviceMem robust;
    double* rw = nullptr;
    int64_t rw_cap = 0;            // edges rw was sized for
    // preconditioner of the PCG path (slam_graph_set_precond): the
    // request, and what the last linearisation latched (in force)
    int32_t precond_kind = SLAM_GRAPH_PRECOND_BLOCK_JACOBI, precond_seg = 64;
    int32_t pc_kind = SLAM_GRAPH_PRECOND_BLOCK_JACOBI, pc_seg = 1;
    bool pc_ready = false;         // minv (and fac) hold the factors of the assembled system
    double* fac = nullptr;         // [nt][18]: Sinv, G of the chain factor
    int32_t* pc_cnt = nullptr;     // [0] off-diagonal blocks used, [1] bad pivots
    // members (slam_graph_set_members): B > 0 splits the poses into
    // B graphs of their own.  The index arrays sit in the arena behind the edge
    // set's; the dense buffers above then hold every member's, one after another.
    int64_t B = 0;
    std::vector<int64_t> pose_off;         // [B + 1]
    std::vector<GraphMember> members;      // rows and buffer offsets, once the edge set stands
    int32_t *m_edge = nullptr, *m_slot = nullptr, *m_row = nullptr;   // member of edge / slot / row
    GraphMember* m_desc = nullptr;
    int32_t *m_active = nullptr, *m_pass = nullptr;   // [B]: touched by the next update / gate passed
    double *m_luout = nullptr, *m_dsum = nullptr;     // [B][kMemberOut], [B]
    int32_t* m_flags_host = nullptr;       // pinned [2 B]: active, pass
    double* m_out_host = nullptr;          // pinned [B][kMemberOut], then the B sums
    int64_t m_host_cap = 0;                // members the pinned buffers were sized for
    int64_t m_dense_cap[4] = {0, 0, 0, 0}; // elements of A / LU / S, V, lan, piv the members hold
    // landmark map (slam_graph_set_observations): its own arena and
    // events, made by the first slam_graph_set_observations (grow-only); a handle
    // that never gets observations holds none of it
    DeviceMem map;
    char* map_arena = nullptr;
    size_t map_bytes = 0;
    bool map_set = false;          // observations stand (for the current pose count)
    int64_t map_n = 0, map_G = 0, map_NL = 0, map_NC = 0;   // input / grouped half-edges, landmarks, chunks
    std::vector<int64_t> map_count;        // [NL]
    int64_t *map_gpose = nullptr, *map_gsrc = nullptr, *map_lstart = nullptr;
    int64_t *map_coff = nullptr, *map_clm = nullptr, *map_cfirst = nullptr;
    double *map_gobs = nullptr, *map_term = nullptr, *map_part = nullptr;
    double *map_mean = nullptr, *map_cov = nullptr, *map_chi2 = nullptr, *map_half = nullptr;
    hipEvent_t map_ev[6] = {};
    double map_ms[5] = {0, 0, 0, 0, 0};    // kernels of the last evaluation, in launch order
    double map_last[2] = {0, 0};           // their total (ms), launches
};

namespace {

#define GTRY(x)               \
    do {                      \
        int rc_ = (x);        \
        if (rc_) return rc_;  \
    } while (0)

template <typename T>
int upload(slam_graph* h, T* dst, const std::vector<T>& src) {
    if (src.empty()) return SLAM_OK;
    SLAM_HIP_TRY(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice,
                                h->stream));
    return SLAM_OK;
}

unsigned nblk(int64_t n, int t = 256) { return (unsigned)((n + t - 1) / t); }

// carve 256-byte aligned arrays out of one allocation
struct Carver {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(int64_t count) {
        T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
        off += ((size_t)std::max<int64_t>(count, 1) * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

// the edge set's device arrays, sized by the upper bounds nt <= min(2E, T) and
// slots <= 2E + nt (carve twice: sizes, then pointers); one allocation reused
// while it is large enough
struct BuildScratch {
    int64_t *tl, *tl_s, *keys, *keys_s, *ukeys, *rb, *ra, *sl, *sl_s, *cval, *bkey, *bkey_s, *bval;
    int64_t* cnt;                  // [0] nt, [1] slots
    void* tmp;
    size_t tmp_bytes;
};

int carve_edge_set(slam_graph* h, int64_t E, int64_t nt_ub, size_t tmp_bytes, BuildScratch* bs) {
    const int64_t K = 2 * E + nt_ub;
    const int64_t n = 3 * nt_ub;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c{pass ? h->arena : nullptr};
        h->edges = c.take<slam_graph_edge>(E);
        h->blocks = c.take<double>(42 * E);
        h->times = c.take<int64_t>(nt_ub);
        h->srow = c.take<int64_t>(K);
        h->scol = c.take<int64_t>(K);
        h->rptr = c.take<int64_t>(nt_ub + 1);
        h->cptr = c.take<int64_t>(K + 1);
        h->clist = c.take<int64_t>(4 * E);
        h->bptr = c.take<int64_t>(nt_ub + 1);
        h->blist = c.take<int64_t>(2 * E);
        h->dslot = c.take<int64_t>(nt_ub);
        h->val = c.take<double>(9 * K);
        h->b = c.take<double>(n);
        h->delta = c.take<double>(n);
        h->dsum = c.take<double>(1);
        h->minv = c.take<double>(9 * nt_ub);
        h->r = c.take<double>(n);
        h->z = c.take<double>(n);
        h->p = c.take<double>(n);
        h->q = c.take<double>(n);
        h->part = c.take<double>(3 * (int64_t)nblk(n, kPcgThreads) + 3);
        h->st = c.take<PcgState>(1);
        h->cx = c.take<double>(2 * n);
        h->chx = c.take<double>(2 * n);
        h->cp = c.take<double>(2 * n);
        h->chp = c.take<double>(2 * n);
        h->cw = c.take<double>(2 * n);
        h->cw2 = c.take<double>(2 * n);
        h->chw = c.take<double>(2 * n);
        h->cpart = c.take<double>((2 * kCondGram + 2) * (int64_t)nblk(n, kPcgThreads) + 8);
        h->cst = c.take<CondState>(1);
        h->cert_part = c.take<double>(4 * (int64_t)nblk(nt_ub, kCertThreads) +
                                      (int64_t)nblk(K, kCertThreads) + 8);
        h->cert = c.take<CertState>(1);
        h->luout = c.take<double>(8);
        h->fac = c.take<double>(kChainFac * nt_ub);
        h->pc_cnt = c.take<int32_t>(2);
        if (bs) {
            bs->tl = c.take<int64_t>(2 * E);
            bs->tl_s = c.take<int64_t>(2 * E);
            bs->keys = c.take<int64_t>(K);
            bs->keys_s = c.take<int64_t>(K);
            bs->ukeys = c.take<int64_t>(K);
            bs->rb = c.take<int64_t>(E);
            bs->ra = c.take<int64_t>(E);
            bs->sl = c.take<int64_t>(4 * E);
            bs->sl_s = c.take<int64_t>(4 * E);
            bs->cval = c.take<int64_t>(4 * E);
            bs->bkey = c.take<int64_t>(2 * E);
            bs->bkey_s = c.take<int64_t>(2 * E);
            bs->bval = c.take<int64_t>(2 * E);
            bs->cnt = c.take<int64_t>(2);
            bs->tmp = c.take<char>((int64_t)tmp_bytes);
            bs->tmp_bytes = tmp_bytes;
        }
        // the members' arrays come last, so no offset above depends on them
        const int64_t Bm = h->B;
        h->m_edge = c.take<int32_t>(Bm ? E : 0);
        h->m_slot = c.take<int32_t>(Bm ? K : 0);
        h->m_row = c.take<int32_t>(Bm ? nt_ub : 0);
        h->m_desc = c.take<GraphMember>(Bm);
        h->m_active = c.take<int32_t>(Bm);
        h->m_pass = c.take<int32_t>(Bm);
        h->m_luout = c.take<double>(kMemberOut * Bm);
        h->m_dsum = c.take<double>(Bm);
        if (pass == 0 && c.off > h->arena_bytes) {
            h->mem.release(h->arena);
            h->arena_bytes = 0;
            GTRY(h->mem.alloc(&h->arena, c.off + c.off / 4));
            h->arena_bytes = c.off + c.off / 4;
        }
    }
    return SLAM_OK;
}

// dense-path buffers (n = 3 nt <= kGraphDenseMax), grow-only
int dense_buffers(slam_graph* h, int64_t n) {
    if (n > kGraphDenseMax) return SLAM_OK;
    if (n <= h->dense_n && h->A) return SLAM_OK;
    h->dense.clear();
    h->dense_n = 0;
    for (int64_t& c : h->m_dense_cap) c = 0;
    GTRY(h->dense.alloc(&h->A, n * n));
    GTRY(h->dense.alloc(&h->LU, n * n));
    GTRY(h->dense.alloc(&h->S, n * n));
    GTRY(h->dense.alloc(&h->V, n * (n + 1)));
    GTRY(h->dense.alloc(&h->lan, 3 * n + 8));
    GTRY(h->dense.alloc(&h->piv, std::max<int64_t>(n, 1)));
    h->dense_n = n;
    return SLAM_OK;
}

int finish_structure(slam_graph* h, int64_t E, int64_t nt, int64_t ns) {
    h->E = E;
    h->pcg_last_iters = 0;
    h->cond_warm = false;
    h->cond_last_iters = 0;
    h->nt = nt;
    h->n_slots = ns;
    const int64_t n = 3 * nt;
    if (h->B) return SLAM_OK;                  // the members' buffers: members_layout
    if (n <= kGraphDenseMax) {
        GTRY(dense_buffers(h, n));
    } else {
        h->dense.clear();
        h->A = h->LU = h->S = h->V = h->lan = nullptr;
        h->piv = nullptr;
        h->dense_n = 0;
        for (int64_t& c : h->m_dense_cap) c = 0;
    }
    return SLAM_OK;
}

// member of a pose id / time (members are contiguous ranges of both)
int64_t member_of(const slam_graph* h, const int64_t t) {
    return (std::upper_bound(h->pose_off.begin(), h->pose_off.end(), t) - h->pose_off.begin()) - 1;
}

// After the structure of the union stands: the member index of every edge,
// block row and slot, every member's rows, and the dense buffers of all members
// (sums over the members, grow-only).  The union's distinct times are sorted,
// so a member's rows are the contiguous ranks of its times.
int members_layout(slam_graph* h, const int64_t n_lm, const slam_graph_edge* ed, const int64_t n_od,
                   const slam_graph_odom* od) {
    const int64_t B = h->B;
    std::vector<int32_t> medge((size_t)h->E), mrow((size_t)h->nt);
    for (int64_t e = 0; e < n_lm; ++e) medge[e] = (int32_t)member_of(h, ed[e].time_bfr);
    for (int64_t e = 0; e < n_od; ++e) medge[n_lm + e] = (int32_t)member_of(h, od[e].time_bfr);
    h->members.assign((size_t)B, GraphMember{});
    for (int64_t r = 0; r < h->nt; ++r) {
        const int64_t m = member_of(h, h->times_h[r]);
        mrow[r] = (int32_t)m;
        if (h->members[m].rows++ == 0) h->members[m].row0 = r;
    }
    int64_t need[4] = {0, 0, 0, 0};
    for (GraphMember& g : h->members) {
        g.n = (3 * g.rows > 3) ? 3 * g.rows : 0;         // :469 (leng > 3), as do_update
        const int64_t n = g.n;
        g.a_off = need[0];
        g.v_off = need[1];
        g.l_off = need[2];
        g.p_off = need[3];
        need[0] += n * n;
        need[1] += n * (n + 1);
        need[2] += 3 * n + 8;
        need[3] += std::max<int64_t>(n, 1);
    }
    bool fits = h->A != nullptr && h->dense_n == 0;
    for (int k = 0; k < 4; ++k) fits = fits && need[k] <= h->m_dense_cap[k];
    if (!fits) {
        h->dense.clear();
        h->A = h->LU = h->S = h->V = h->lan = nullptr;
        h->piv = nullptr;
        h->dense_n = 0;
        for (int64_t& c : h->m_dense_cap) c = 0;
        GTRY(h->dense.alloc(&h->A, need[0]));
        GTRY(h->dense.alloc(&h->LU, need[0]));
        GTRY(h->dense.alloc(&h->S, need[0]));
        GTRY(h->dense.alloc(&h->V, need[1]));
        GTRY(h->dense.alloc(&h->lan, need[2]));
        GTRY(h->dense.alloc(&h->piv, need[3]));
        for (int k = 0; k < 4; ++k) h->m_dense_cap[k] = need[k];
    }
    if (h->m_host_cap < B) {
        h->mem.release(h->m_flags_host);
        h->mem.release(h->m_out_host);
        h->m_host_cap = 0;
        GTRY(h->mem.alloc_pinned(&h->m_flags_host, nullptr, (size_t)(2 * B), hipHostMallocDefault));
        GTRY(h->mem.alloc_pinned(&h->m_out_host, nullptr, (size_t)((kMemberOut + 1) * B),
                                 hipHostMallocDefault));
        h->m_host_cap = B;
    }
    GTRY(upload(h, h->m_edge, medge));
    GTRY(upload(h, h->m_row, mrow));
    GTRY(upload(h, h->m_desc, h->members));
    hipLaunchKernelGGL(graph_member_slot_kernel, dim3(nblk(h->n_slots)), dim3(256), 0, h->stream,
                       h->n_slots, h->srow, h->m_row, h->m_slot);
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));     // the uploads read the vectors until here
    return SLAM_OK;
}

// the structure on the device (graph_build.inl)
int build_structure_device(slam_graph* h, const int64_t n_lm, const slam_graph_edge* ed,
                           const int64_t n_od, const slam_graph_odom* od) {
    const int64_t E = n_lm + n_od;
    const int64_t nt_ub = std::min<int64_t>(2 * E, h->T);
    const int64_t K = 2 * E + nt_ub;
    const int tbits = bits_for((uint64_t)h->T);
    const int sbits = bits_for((uint64_t)K);
    hipStream_t s = h->stream;
    // temporary storage of the largest rocPRIM call
    size_t tb = 0, t1 = 0;
    int64_t* np = nullptr;
    auto q = [&](hipError_t e) { return e == hipSuccess; };
    if (!q(rocprim::radix_sort_keys(nullptr, t1, np, np, (size_t)(2 * E), 0, tbits, s))) goto qfail;
    tb = std::max(tb, t1);
    if (!q(rocprim::unique(nullptr, t1, np, np, np, (size_t)(2 * E), rocprim::equal_to<int64_t>(), s)))
        goto qfail;
    tb = std::max(tb, t1);
    if (!q(rocprim::radix_sort_keys(nullptr, t1, np, np, (size_t)K, 0, 64, s))) goto qfail;
    tb = std::max(tb, t1);
    if (!q(rocprim::unique(nullptr, t1, np, np, np, (size_t)K, rocprim::equal_to<int64_t>(), s))) goto qfail;
    tb = std::max(tb, t1);
    if (!q(rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (size_t)(4 * E), 0, sbits, s)))
        goto qfail;
    tb = std::max(tb, t1);
    if (!q(rocprim::radix_sort_pairs(nullptr, t1, np, np, np, np, (size_t)(2 * E), 0, tbits, s)))
        goto qfail;
    tb = std::max(tb, t1);
    {
        BuildScratch bs{};
        GTRY(carve_edge_set(h, E, nt_ub, tb, &bs));
        // the two records share size and index prefix: the odometry edges go behind
        // the landmark edges of the same device array
        if (n_lm)
            SLAM_HIP_TRY(hipMemcpyAsync(h->edges, ed, n_lm * sizeof(slam_graph_edge),
                                        hipMemcpyHostToDevice, s));
        if (n_od)
            SLAM_HIP_TRY(hipMemcpyAsync(h->edges + n_lm, od, n_od * sizeof(slam_graph_odom),
                                        hipMemcpyHostToDevice, s));
        // distinct times (:457-467 order)
        hipLaunchKernelGGL(gb_times_kernel, dim3(nblk(E)), dim3(256), 0, s, E, h->edges, bs.tl);
        size_t t = bs.tmp_bytes;
        if (!q(rocprim::radix_sort_keys(bs.tmp, t, bs.tl, bs.tl_s, (size_t)(2 * E), 0, tbits, s))) goto rfail;
        t = bs.tmp_bytes;
        if (!q(rocprim::unique(bs.tmp, t, bs.tl_s, h->times, bs.cnt, (size_t)(2 * E),
                               rocprim::equal_to<int64_t>(), s)))
            goto rfail;
        // slots of H: unique sorted keys r nt + c
        hipLaunchKernelGGL(gb_keys_kernel, dim3(nblk(std::max(E, nt_ub))), dim3(256), 0, s, E, h->edges,
                           h->times, bs.cnt, nt_ub, bs.rb, bs.ra, bs.keys, bs.bkey, bs.bval);
        t = bs.tmp_bytes;
        if (!q(rocprim::radix_sort_keys(bs.tmp, t, bs.keys, bs.keys_s, (size_t)K, 0, 64, s))) goto rfail;
        t = bs.tmp_bytes;
        if (!q(rocprim::unique(bs.tmp, t, bs.keys_s, bs.ukeys, bs.cnt + 1, (size_t)K,
                               rocprim::equal_to<int64_t>(), s)))
            goto rfail;
        hipLaunchKernelGGL(gb_count_kernel, dim3(1), dim3(1), 0, s, bs.ukeys, bs.cnt + 1);
        hipLaunchKernelGGL(gb_slots_kernel, dim3(nblk(std::max(K, nt_ub + 1))), dim3(256), 0, s, bs.ukeys,
                           bs.cnt + 1, bs.cnt, nt_ub + 1, h->srow, h->scol, h->dslot, h->rptr);
        // H plan: edge parts grouped by slot, edge order kept (stable sort)
        hipLaunchKernelGGL(gb_parts_kernel, dim3(nblk(4 * E)), dim3(256), 0, s, E, bs.rb, bs.ra, bs.cnt,
                           bs.ukeys, bs.cnt + 1, bs.sl, bs.cval);
        t = bs.tmp_bytes;
        if (!q(rocprim::radix_sort_pairs(bs.tmp, t, bs.sl, bs.sl_s, bs.cval, h->clist, (size_t)(4 * E), 0,
                                         sbits, s)))
            goto rfail;
        hipLaunchKernelGGL(gb_offsets_kernel, dim3(nblk(K + 1)), dim3(256), 0, s, bs.sl_s, 4 * E,
                           bs.cnt + 1, K + 1, h->cptr);
        // b plan: (edge, side) grouped by row, edge order kept
        t = bs.tmp_bytes;
        if (!q(rocprim::radix_sort_pairs(bs.tmp, t, bs.bkey, bs.bkey_s, bs.bval, h->blist, (size_t)(2 * E),
                                         0, tbits, s)))
            goto rfail;
        hipLaunchKernelGGL(gb_offsets_kernel, dim3(nblk(nt_ub + 1)), dim3(256), 0, s, bs.bkey_s, 2 * E,
                           bs.cnt, nt_ub + 1, h->bptr);
        SLAM_HIP_TRY(hipGetLastError());
        // read back through pinned memory: the counts, then the distinct times
        const int64_t need = std::max<int64_t>(2, nt_ub);
        if (h->cnt_cap < need) {
            h->mem.release(h->cnt_host);
            h->cnt_cap = 0;
            GTRY(h->mem.alloc_pinned(&h->cnt_host, nullptr, (size_t)need, hipHostMallocDefault));
            h->cnt_cap = need;
        }
        SLAM_HIP_TRY(hipMemcpyAsync(h->cnt_host, bs.cnt, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        SLAM_HIP_TRY(hipStreamSynchronize(s));
        const int64_t cnt[2] = {h->cnt_host[0], h->cnt_host[1]};
        SLAM_HIP_TRY(hipMemcpyAsync(h->cnt_host, h->times, cnt[0] * sizeof(int64_t),
                                    hipMemcpyDeviceToHost, s));
        GTRY(finish_structure(h, E, cnt[0], cnt[1]));
        SLAM_HIP_TRY(hipStreamSynchronize(s));
        h->times_h.assign(h->cnt_host, h->cnt_host + cnt[0]);
        return SLAM_OK;
    }
rfail:
    return fail(SLAM_ERR_HIP, "graph structure build: rocPRIM call failed");
qfail:
    return fail(SLAM_ERR_HIP, "graph structure build: rocPRIM size query failed");
}

// the same arrays from a host pass (SLAM_GRAPH_HOST_BUILD=1; the tests compare the two)
int build_structure_host(slam_graph* h, const int64_t n_lm, const slam_graph_edge* ed_lm,
                         const int64_t n_od, const slam_graph_odom* od) {
    const int64_t E = n_lm + n_od;
    std::vector<slam_graph_edge> all;      // the concatenation (only with odometry edges)
    const slam_graph_edge* ed = ed_lm;
    if (n_od) {
        all.resize((size_t)E);
        if (n_lm) std::memcpy(all.data(), ed_lm, (size_t)n_lm * sizeof(slam_graph_edge));
        std::memcpy(all.data() + n_lm, od, (size_t)n_od * sizeof(slam_graph_odom));
        ed = all.data();
    }
    std::vector<int64_t> tl;
    tl.reserve(2 * E);
    for (int64_t e = 0; e < E; ++e) {
        tl.push_back(ed[e].time_bfr);
        tl.push_back(ed[e].time_aft);
    }
    std::sort(tl.begin(), tl.end());
    tl.erase(std::unique(tl.begin(), tl.end()), tl.end());
    const int64_t nt = (int64_t)tl.size();
    auto rank = [&](int64_t t) { return (int64_t)(std::lower_bound(tl.begin(), tl.end(), t) - tl.begin()); };
    std::vector<int64_t> rb(E), ra(E);
    std::vector<int64_t> keys;
    keys.reserve(4 * E + nt);
    for (int64_t i = 0; i < nt; ++i) keys.push_back(i * nt + i);
    for (int64_t e = 0; e < E; ++e) {
        rb[e] = rank(ed[e].time_bfr);
        ra[e] = rank(ed[e].time_aft);
        keys.push_back(rb[e] * nt + ra[e]);
        keys.push_back(ra[e] * nt + rb[e]);
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const int64_t ns = (int64_t)keys.size();
    auto slot = [&](int64_t r, int64_t c) {
        return (int64_t)(std::lower_bound(keys.begin(), keys.end(), r * nt + c) - keys.begin());
    };
    std::vector<int64_t> srow(ns), scol(ns), rptr(nt + 1, 0), dslot(nt);
    for (int64_t s = 0; s < ns; ++s) {
        srow[s] = keys[s] / nt;
        scol[s] = keys[s] % nt;
        rptr[srow[s] + 1]++;
        if (srow[s] == scol[s]) dslot[srow[s]] = s;
    }
    for (int64_t i = 0; i < nt; ++i) rptr[i + 1] += rptr[i];
    // accumulation plan, stable in edge order (updateEstPose :484-492)
    std::vector<int64_t> cnt(ns + 1, 0), sl(4 * E);
    for (int64_t e = 0; e < E; ++e) {
        sl[4 * e + 0] = slot(rb[e], rb[e]);
        sl[4 * e + 1] = slot(rb[e], ra[e]);
        sl[4 * e + 2] = slot(ra[e], rb[e]);
        sl[4 * e + 3] = slot(ra[e], ra[e]);
        for (int k = 0; k < 4; ++k) cnt[sl[4 * e + k] + 1]++;
    }
    for (int64_t s = 0; s < ns; ++s) cnt[s + 1] += cnt[s];
    std::vector<int64_t> cptr = cnt, clist(4 * E);
    for (int64_t c = 0; c < 4 * E; ++c) clist[cnt[sl[c]]++] = c;     // c = 4 e + part
    std::vector<int64_t> bc(nt + 1, 0), blist(2 * E);
    for (int64_t e = 0; e < E; ++e) {
        bc[rb[e] + 1]++;
        bc[ra[e] + 1]++;
    }
    for (int64_t i = 0; i < nt; ++i) bc[i + 1] += bc[i];
    std::vector<int64_t> bptr = bc;
    for (int64_t e = 0; e < E; ++e) {
        blist[bc[rb[e]]++] = 2 * e;
        blist[bc[ra[e]]++] = 2 * e + 1;
    }
    // device buffers (the same carve as the device build)
    GTRY(carve_edge_set(h, E, std::min<int64_t>(2 * E, h->T), 0, nullptr));
    h->times_h = tl;
    GTRY(finish_structure(h, E, nt, ns));
    SLAM_HIP_TRY(hipMemcpyAsync(h->edges, ed, E * sizeof(slam_graph_edge), hipMemcpyHostToDevice,
                                h->stream));
    GTRY(upload(h, h->times, tl));
    GTRY(upload(h, h->srow, srow));
    GTRY(upload(h, h->scol, scol));
    GTRY(upload(h, h->rptr, rptr));
    GTRY(upload(h, h->cptr, cptr));
    GTRY(upload(h, h->clist, clist));
    GTRY(upload(h, h->bptr, bptr));
    GTRY(upload(h, h->blist, blist));
    GTRY(upload(h, h->dslot, dslot));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int build_structure(slam_graph* h, int64_t n_lm, const slam_graph_edge* ed, int64_t n_od,
                    const slam_graph_odom* od) {
    const char* hb = std::getenv("SLAM_GRAPH_HOST_BUILD");
    if (hb && hb[0] == '1') return build_structure_host(h, n_lm, ed, n_od, od);
    return build_structure_device(h, n_lm, ed, n_od, od);
}

// slam_graph_set_edges / slam_graph_set_edges_odom after their pointer checks:
// every record is checked on the host before the handle changes; the edge set
// is the concatenation, landmark edges first.  E_lm is set only once the
// structure stands; a build that fails leaves the handle with no edge set.
int set_edge_set(slam_graph* h, int64_t n_edges, const slam_graph_edge* edges, int64_t n_odom,
                 const slam_graph_odom* odom, const std::string& entry) {
    for (int64_t e = 0; e < n_edges; ++e) {
        const slam_graph_edge& d = edges[e];
        SLAM_ARG_CHECK(d.pose_bfr >= 0 && d.pose_bfr < h->T && d.pose_aft >= 0 && d.pose_aft < h->T &&
                           d.time_bfr >= 0 && d.time_bfr < h->T && d.time_aft >= 0 &&
                           d.time_aft < h->T,
                       entry + ": pose / time index out of range");
    }
    for (int64_t e = 0; e < n_odom; ++e) {
        const slam_graph_odom& d = odom[e];
        SLAM_ARG_CHECK(d.pose_bfr >= 0 && d.pose_bfr < h->T && d.pose_aft >= 0 && d.pose_aft < h->T &&
                           d.time_bfr >= 0 && d.time_bfr < h->T && d.time_aft >= 0 &&
                           d.time_aft < h->T,
                       entry + ": pose / time index of an odometry edge out of range");
        SLAM_ARG_CHECK(d.time_bfr != d.time_aft, entry + ": odometry edge with time_bfr == time_aft");
        for (int k = 0; k < 3; ++k) {
            SLAM_ARG_CHECK(std::isfinite(d.rel[k]), entry + ": odometry rel is not finite");
            SLAM_ARG_CHECK(std::isfinite(d.sigma[k]) && d.sigma[k] > 0.0,
                           entry + ": odometry sigma must be finite and > 0");
        }
    }
    if (h->B) {
        // both poses and both times of an edge in one member's range (the times
        // index poses: graph_pose_update_kernel)
        auto one_member = [&](const int64_t tb, const int64_t pb, const int64_t ta, const int64_t pa) {
            const int64_t m = member_of(h, tb);
            const int64_t lo = h->pose_off[m], hi = h->pose_off[m + 1];
            return lo <= pb && pb < hi && lo <= ta && ta < hi && lo <= pa && pa < hi;
        };
        for (int64_t e = 0; e < n_edges; ++e)
            SLAM_ARG_CHECK(one_member(edges[e].time_bfr, edges[e].pose_bfr, edges[e].time_aft,
                                      edges[e].pose_aft),
                           entry + ": an edge whose poses and times are not in one member");
        for (int64_t e = 0; e < n_odom; ++e)
            SLAM_ARG_CHECK(one_member(odom[e].time_bfr, odom[e].pose_bfr, odom[e].time_aft,
                                      odom[e].pose_aft),
                           entry + ": an odometry edge whose poses and times are not in one member");
    }
    SLAM_HIP_TRY(hipSetDevice(h->device));
    h->assembled = false;
    h->marg_last_iters = 0;
    h->lin_kind = -1;
    int rc = SLAM_OK;
    if (n_edges + n_odom) rc = build_structure(h, n_edges, edges, n_odom, odom);
    if (!rc && h->B && n_edges + n_odom) rc = members_layout(h, n_edges, edges, n_odom, odom);
    if (rc || n_edges + n_odom == 0) {
        h->E = h->E_lm = h->nt = h->n_slots = 0;
        h->times_h.clear();
        return rc;
    }
    h->E_lm = n_edges;
    return SLAM_OK;
}

// the handle back in the plain form with no edge set (slam_graph_set_members,
// and slam_graph_set_poses on a handle with members)
void clear_members(slam_graph* h) {
    h->B = 0;
    h->pose_off.clear();
    h->members.clear();
    h->E = h->E_lm = h->nt = h->n_slots = 0;
    h->times_h.clear();
    h->assembled = false;
    h->marg_last_iters = 0;
    h->lin_kind = -1;
}

GraphConst gconst(const slam_graph_config& c) { return GraphConst{c.r_dist, c.r_dir, c.r_orient}; }

// the robust array's parts for E edges
struct RobustRows {
    double *lin, *eval, *part, *tot;
};

RobustRows robust_rows(const slam_graph* h) {
    const int64_t cap = h->rw_cap;
    return RobustRows{h->rw, h->rw + 2 * cap, h->rw + 4 * cap,
                      h->rw + 4 * cap + 4 * (int64_t)nblk(cap, kChi2Threads)};
}

int robust_reserve(slam_graph* h) {
    if (h->rw && h->E <= h->rw_cap) return SLAM_OK;
    h->robust.release(h->rw);
    h->rw_cap = 0;
    const int64_t cap = h->E + h->E / 4;
    GTRY(h->robust.alloc(&h->rw, (size_t)(4 * cap + 4 * (int64_t)nblk(cap, kChi2Threads) + 4)));
    h->rw_cap = cap;
    return SLAM_OK;
}

// the linearise launch of both sites (linearize_assemble, slam_graph_marginals)
// with the handle's robust kind; a none handle takes the unweighted
// instantiation and never allocates the rows.  A set without odometry edges
// launches the default instantiation over all E columns and nothing else; with
// them the landmark columns [0, E_lm) take the MIXED one (E is the stride) and
// graph_linearize_odom_kernel the tail [E_lm, E).
int launch_linearize(slam_graph* h) {
    const int32_t kind = h->robust_kind;
    const int64_t n_od = h->E - h->E_lm;
    double* rows = nullptr;
    if (kind != SLAM_GRAPH_ROBUST_NONE) {
        GTRY(robust_reserve(h));
        rows = robust_rows(h).lin;
    }
#define SLAM_LINEARIZE(K)                                                                          \
    if (n_od == 0)                                                                                 \
        hipLaunchKernelGGL(graph_linearize_kernel<K>, dim3(nblk(h->E)), dim3(256), 0, h->stream,   \
                           h->E, h->edges, h->poses, gconst(h->cfg), h->blocks, h->robust_param,   \
                           rows, (int64_t)0);                                                      \
    else if (h->E_lm)                                                                              \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(graph_linearize_kernel<K, true>), dim3(nblk(h->E_lm)),  \
                           dim3(256), 0, h->stream, h->E, h->edges, h->poses, gconst(h->cfg),      \
                           h->blocks, h->robust_param, rows, h->E_lm)
    switch (kind) {
        case SLAM_GRAPH_ROBUST_HUBER: SLAM_LINEARIZE(SLAM_GRAPH_ROBUST_HUBER); break;
        case SLAM_GRAPH_ROBUST_CAUCHY: SLAM_LINEARIZE(SLAM_GRAPH_ROBUST_CAUCHY); break;
        case SLAM_GRAPH_ROBUST_DCS: SLAM_LINEARIZE(SLAM_GRAPH_ROBUST_DCS); break;
        default: SLAM_LINEARIZE(SLAM_GRAPH_ROBUST_NONE); break;      // set_robust admits no other
    }
#undef SLAM_LINEARIZE
    if (n_od)
        hipLaunchKernelGGL(graph_linearize_odom_kernel, dim3(nblk(n_od)), dim3(256), 0, h->stream,
                           h->E_lm, h->E, h->edges, h->poses, h->blocks, rows);
    h->lin_kind = kind;
    // the preconditioner takes effect here, like the robust kind
    h->pc_kind = h->precond_kind;
    h->pc_seg = (h->pc_kind == SLAM_GRAPH_PRECOND_CHAIN) ? h->precond_seg : 1;
    h->pc_ready = false;
    return SLAM_OK;
}

// chi2_e, w_e of every edge at the current poses into `rows` ([2][E]) and the
// four totals into the robust array (graph_chi2_kernel, then its fold)
int launch_chi2(slam_graph* h, double* rows) {
    const RobustRows r = robust_rows(h);
    const unsigned nb = nblk(h->E, kChi2Threads);
    const bool mixed = h->E_lm < h->E;
#define SLAM_CHI2(K)                                                                               \
    if (!mixed)                                                                                    \
        hipLaunchKernelGGL(graph_chi2_kernel<K>, dim3(nb), dim3(kChi2Threads), 0, h->stream, h->E, \
                           h->edges, h->poses, gconst(h->cfg), h->robust_param, rows, r.part,      \
                           (int64_t)0);                                                            \
    else                                                                                           \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(graph_chi2_kernel<K, true>), dim3(nb),                  \
                           dim3(kChi2Threads), 0, h->stream, h->E, h->edges, h->poses,             \
                           gconst(h->cfg), h->robust_param, rows, r.part, h->E_lm)
    switch (h->robust_kind) {
        case SLAM_GRAPH_ROBUST_HUBER: SLAM_CHI2(SLAM_GRAPH_ROBUST_HUBER); break;
        case SLAM_GRAPH_ROBUST_CAUCHY: SLAM_CHI2(SLAM_GRAPH_ROBUST_CAUCHY); break;
        case SLAM_GRAPH_ROBUST_DCS: SLAM_CHI2(SLAM_GRAPH_ROBUST_DCS); break;
        default: SLAM_CHI2(SLAM_GRAPH_ROBUST_NONE); break;
    }
#undef SLAM_CHI2
    hipLaunchKernelGGL(graph_chi2_fold_kernel, dim3(1), dim3(kChi2FoldThreads), 0, h->stream,
                       (int64_t)nb, r.part, r.tot);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int linearize_assemble(slam_graph* h) {
    SLAM_HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    GTRY(launch_linearize(h));
    SLAM_HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    hipLaunchKernelGGL(graph_assemble_h_kernel, dim3(nblk(9 * h->n_slots)), dim3(256), 0,
                       h->stream, h->n_slots, h->E, h->cptr, h->clist, h->blocks, h->cfg.anchor,
                       h->val);
    hipLaunchKernelGGL(graph_assemble_b_kernel, dim3(nblk(3 * h->nt)), dim3(256), 0, h->stream,
                       h->nt, h->E, h->bptr, h->blist, h->blocks, h->b);
    SLAM_HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int dense_matrix(slam_graph* h, double* A) {
    const int64_t n = 3 * h->nt;
    SLAM_HIP_TRY(hipMemsetAsync(A, 0, n * n * sizeof(double), h->stream));
    hipLaunchKernelGGL(graph_dense_scatter_kernel, dim3(nblk(9 * h->n_slots)), dim3(256), 0,
                       h->stream, h->n_slots, h->srow, h->scol, h->val, n, A);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// dense path: LU of H and the reference's gate on it (updateEstPose :494-496)
int dense_factor_gate(slam_graph* h, double* det_out, double* cond_out, bool* pass) {
    const int64_t n = 3 * h->nt;
    GTRY(dense_matrix(h, h->A));
    SLAM_HIP_TRY(hipMemcpyAsync(h->LU, h->A, n * n * sizeof(double), hipMemcpyDeviceToDevice,
                                h->stream));
    hipLaunchKernelGGL(graph_symmetrize_kernel, dim3(nblk(n * n)), dim3(256), 0, h->stream, h->A, n,
                       h->S);
    hipLaunchKernelGGL(graph_lu_kernel, dim3(1), dim3(kGraphThreads), 0, h->stream, h->LU, (int)n,
                       h->piv, h->luout);
    hipLaunchKernelGGL(graph_lanczos_kernel, dim3(1), dim3(kGraphThreads), 0, h->stream, h->S,
                       (int)n, h->V, h->lan, h->lan + n, h->lan + 2 * n, h->luout + 3,
                       (uint64_t)0x5EEDULL);
    SLAM_HIP_TRY(hipGetLastError());
    double lo[5];
    SLAM_HIP_TRY(hipMemcpyAsync(lo, h->luout, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    // numpy det: sign * exp(logdet); a zero pivot gives 0 (getrf info > 0)
    const double det = (lo[2] != 0.0) ? 0.0 : lo[0] * std::exp(lo[1]);
    const double cond = (lo[4] > 0.0) ? lo[3] / lo[4] : std::numeric_limits<double>::infinity();
    *det_out = det;
    *cond_out = cond;
    *pass = (h->cfg.det_min < det) && (cond < h->cfg.cond_max);
    return SLAM_OK;
}

// dense path: det, cond, gate, delta (updateEstPose :494-502)
int solve_dense(slam_graph* h, double* stats, bool* solved) {
    const int64_t n = 3 * h->nt;
    GTRY(dense_factor_gate(h, &stats[2], &stats[3], solved));
    if (*solved)
        hipLaunchKernelGGL(graph_lu_solve_kernel, dim3(1), dim3(kGraphThreads), 0, h->stream,
                           h->LU, (int)n, h->piv, h->b, h->delta);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// the estimate's stall window (kCondWin; SLAM_GRAPH_COND_WIN 2..32 for A/B)
static int cond_win() {
    static const int w = [] {
        const char* e = std::getenv("SLAM_GRAPH_COND_WIN");
        const int v = e ? std::atoi(e) : 0;
        return (v >= 2 && v <= 32) ? v : kCondWin;
    }();
    return w;
}

// condition-number estimate (graph_kernels.inl: LOBPCG for the extreme
// eigenvalues) on h->cstream, enqueued in batches of `count` iterations
// starting at iteration k0 (k0 = 0: the start sequence first).
// The certificate mode's early decision of the estimate (CondState.etol): both
// sides moved less than 1e-3 (relative) over 8 iterations and the estimate
// clears cond_max by a factor 100 (status 5).  A Ritz ratio under-estimates
// cond, so the factor is the margin the VERDICT r4 asked for; with the
// tight test (1e-5 over 16, status 1) the gate keeps a factor 10.
constexpr double kCertEarlyTol = 1e-3, kCertEarlyMargin = 100.0, kCertConvMargin = 10.0;
constexpr int kCertEarlyWin = 8;

int cond_enqueue(slam_graph* h, int32_t k0, int32_t count) {
    const int64_t n = 3 * h->nt;
    const bool early = h->cfg.cond_mode == SLAM_GRAPH_COND_MARGIN;
    const unsigned nb = nblk(n, kPcgThreads);
    hipStream_t s = h->cstream;
    const double tol = h->cfg.cond_tol > 0.0 ? h->cfg.cond_tol : 1e-5;
    const int32_t mx = h->cfg.cond_max_iter > 0 ? h->cfg.cond_max_iter : 3000;
    int32_t k = k0;
    // merged (default): the SpMV launch's last workgroup folds and decides
    // the iteration (two launches per iteration); SLAM_GRAPH_COND_MERGED=0
    // keeps the separate one-workgroup fold launch (same totals, A/B)
    static const bool merged = [] {
        const char* e = std::getenv("SLAM_GRAPH_COND_MERGED");
        return !(e && e[0] == '0');
    }();
    if (merged) {
        if (k0 == 0) {
            hipLaunchKernelGGL(graph_cond_init_kernel, dim3(nblk(2 * n)), dim3(256), 0, s, n,
                               h->cond_warm ? 0 : 1, cond_win(), h->cx, h->cp, h->chp, h->cst,
                               early ? kCertEarlyTol : 0.0, kCertEarlyWin, kCertEarlyMargin);
            hipLaunchKernelGGL((graph_cond_spmv_kernel<true, true>), dim3(nb), dim3(kSpmvThreads), 0, s,
                               h->nt, h->rptr, h->scol, h->val, h->cx, h->chx, h->cw, h->cw2, h->chw,
                               h->cp, h->chp, h->cpart, h->cst, 0, tol, mx, h->cfg.cond_max);
            hipLaunchKernelGGL(graph_cond_update_kernel, dim3(nb), dim3(kPcgThreads), 0, s, n, 0,
                               h->minv, h->cx, h->chx, h->cw2, h->chw, h->cp, h->chp, h->cw,
                               h->cpart, h->cst);
            k = 1;
        }
        for (; k < k0 + count; ++k) {
            hipLaunchKernelGGL((graph_cond_spmv_kernel<false, true>), dim3(nb), dim3(kSpmvThreads), 0,
                               s, h->nt, h->rptr, h->scol, h->val, h->cx, h->chx, h->cw, h->cw2,
                               h->chw, h->cp, h->chp, h->cpart, h->cst, k, tol, mx, h->cfg.cond_max);
            hipLaunchKernelGGL(graph_cond_update_kernel, dim3(nb), dim3(kPcgThreads), 0, s, n, k,
                               h->minv, h->cx, h->chx, h->cw2, h->chw, h->cp, h->chp, h->cw,
                               h->cpart, h->cst);
        }
        SLAM_HIP_TRY(hipGetLastError());
        return SLAM_OK;
    }
    if (k0 == 0) {
        hipLaunchKernelGGL(graph_cond_init_kernel, dim3(nblk(2 * n)), dim3(256), 0, s, n,
                           h->cond_warm ? 0 : 1, cond_win(), h->cx, h->cp, h->chp, h->cst,
                           early ? kCertEarlyTol : 0.0, kCertEarlyWin, kCertEarlyMargin);
        hipLaunchKernelGGL(graph_cond_spmv_kernel<true>, dim3(nb), dim3(kSpmvThreads), 0, s, h->nt,
                           h->rptr, h->scol, h->val, h->cx, h->chx, h->cw, h->cw2, h->chw, h->cp,
                           h->chp, h->cpart, h->cst);
        hipLaunchKernelGGL(graph_cond_fold_kernel, dim3(1), dim3(kCondFoldThreads), 0, s,
                           (int64_t)nb, h->cpart, h->cst, 0, tol, mx, h->cfg.cond_max);
        hipLaunchKernelGGL(graph_cond_update_kernel, dim3(nb), dim3(kPcgThreads), 0, s, n, 0,
                           h->minv, h->cx, h->chx, h->cw2, h->chw, h->cp, h->chp, h->cw, h->cpart,
                           h->cst);
        k = 1;
    }
    for (; k < k0 + count; ++k) {
        hipLaunchKernelGGL(graph_cond_spmv_kernel<false>, dim3(nb), dim3(kSpmvThreads), 0, s, h->nt,
                           h->rptr, h->scol, h->val, h->cx, h->chx, h->cw, h->cw2, h->chw, h->cp,
                           h->chp, h->cpart, h->cst);
        hipLaunchKernelGGL(graph_cond_fold_kernel, dim3(1), dim3(kCondFoldThreads), 0, s,
                           (int64_t)nb, h->cpart, h->cst, k, tol, mx, h->cfg.cond_max);
        hipLaunchKernelGGL(graph_cond_update_kernel, dim3(nb), dim3(kPcgThreads), 0, s, n, k,
                           h->minv, h->cx, h->chx, h->cw2, h->chw, h->cp, h->chp, h->cw, h->cpart,
                           h->cst);
    }
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// ---- the gate's certificate (SLAM_GRAPH_COND_MARGIN; graph_kernels.inl)
// The certificate's sums on the second stream beside the PCG (after the
// block-Jacobi inverses): one lane per pose, one per block slot, one fold.
int cert_enqueue(slam_graph* h) {
    hipStream_t s = h->cstream;
    const unsigned nbp = nblk(h->nt, kCertThreads), nbs = nblk(h->n_slots, kCertThreads);
    hipLaunchKernelGGL(graph_cert_pose_kernel, dim3(nbp), dim3(kCertThreads), 0, s, h->nt, h->dslot,
                       h->val, h->minv, h->cert_part);
    hipLaunchKernelGGL(graph_cert_slot_kernel, dim3(nbs), dim3(kCertThreads), 0, s, h->n_slots,
                       h->srow, h->scol, h->val, h->minv, h->cert_part + 4 * (int64_t)nbp);
    hipLaunchKernelGGL(graph_cert_fold_kernel, dim3(1), dim3(kCertThreads), 0, s, (int64_t)nbp,
                       h->cert_part, (int64_t)nbs, h->cert_part + 4 * (int64_t)nbp, h->cert);
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipMemcpyAsync(h->cert_host, h->cert, sizeof(CertState), hipMemcpyDeviceToHost, s));
    return SLAM_OK;
}

// det(H) from the dense LU (n <= kGraphDenseMax): the certificate's fallback
int dense_det(slam_graph* h, double* det) {
    const int64_t n = 3 * h->nt;
    GTRY(dense_matrix(h, h->A));
    SLAM_HIP_TRY(hipMemcpyAsync(h->LU, h->A, n * n * sizeof(double), hipMemcpyDeviceToDevice,
                                h->stream));
    hipLaunchKernelGGL(graph_lu_kernel, dim3(1), dim3(kGraphThreads), 0, h->stream, h->LU, (int)n,
                       h->piv, h->luout);
    SLAM_HIP_TRY(hipGetLastError());
    double lo[3];
    SLAM_HIP_TRY(hipMemcpyAsync(lo, h->luout, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    *det = (lo[2] != 0.0) ? 0.0 : lo[0] * std::exp(lo[1]);
    return SLAM_OK;
}

// cond(H) by the dense path's Lanczos (n <= kGraphDenseMax): the certificate's fallback
int dense_cond(slam_graph* h, double* cond) {
    const int64_t n = 3 * h->nt;
    GTRY(dense_matrix(h, h->A));
    hipLaunchKernelGGL(graph_symmetrize_kernel, dim3(nblk(n * n)), dim3(256), 0, h->stream, h->A, n,
                       h->S);
    hipLaunchKernelGGL(graph_lanczos_kernel, dim3(1), dim3(kGraphThreads), 0, h->stream, h->S,
                       (int)n, h->V, h->lan, h->lan + n, h->lan + 2 * n, h->luout + 3,
                       (uint64_t)0x5EEDULL);
    SLAM_HIP_TRY(hipGetLastError());
    double lo[2];
    SLAM_HIP_TRY(hipMemcpyAsync(lo, h->luout + 3, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    *cond = (lo[1] > 0.0) ? lo[0] / lo[1] : std::numeric_limits<double>::infinity();
    return SLAM_OK;
}

// The gate (:494-496) in the estimate-with-margin mode (SLAM_GRAPH_COND_MARGIN,
// formerly named CERTIFY), from the LOBPCG estimate (cs, run beside the PCG
// with the early decision) and the log-det sums (ct).  Not a certificate: the
// estimate's Ritz value over-estimates lambda_min(H), so each half passes
// only with a margin against that error (VERDICT / ADVICE r5):
//  * cond: the Ritz ratio under-estimates cond; status 5 (the early stop)
//    passes with cond x 100 < cond_max, status 1 (tightly converged) with cond
//    x 10 < cond_max, and a converged estimate inside that band is decided by
//    the estimate itself (decision 5, as SLAM_GRAPH_COND_ESTIMATE does: the
//    reference applies such updates); status 2 / 4 rejects (cond >= cond_max,
//    or not positive definite, for certain); anything else is undecided;
//  * det: log det H in [log det M + c(a) (tr(P^2) - n), log det M] (Fischer
//    above; the quadratic bound of ln below, valid for any a <= lambda_min(P),
//    graph_kernels.inl), with a = lambda~min(H) / (F max tr M_i), F =
//    kGateDetMargin = 1000: the lower end stays a bound unless the Ritz value
//    over-estimates lambda_min(H) by more than F (lambda_min(P) >= lambda_min(H)
//    / lambda_max(M) >= lambda_min(H) / max tr M_i).  gate_info reports the
//    largest factor the decision tolerates (det_margin).  Passes above ln
//    det_min, rejects below the upper end (rigorous), undecided inside;
// an undecided half takes the dense path's own det / Lanczos cond when n <=
// kGraphDenseMax, otherwise the update is not solved and gate_info says
// "undecided" (a possible parity gap, not a rejection).
// SLAM_GRAPH_GATE_RITZ_SCALE=<f> (diagnostic, tests): the gate uses f x the
// estimate's lambda_min, emulating an estimate that over-estimates it by f.
constexpr double kGateDetMargin = 1000.0;

double gate_ritz_scale() {
    const char* e = std::getenv("SLAM_GRAPH_GATE_RITZ_SCALE");
    const double f = e ? std::atof(e) : 1.0;
    return f > 0.0 ? f : 1.0;
}

// the log-det lower end for lambda_min(P) >= a
double logdet_lower(const CertState& ct, const double a, const int64_t n) {
    const double c = (std::log(a) - a + 1.0) / ((a - 1.0) * (a - 1.0));
    return ct.logdet_m + c * std::max(0.0, ct.trp2 - (double)n);
}

int cert_gate(slam_graph* h, const CondState& cs, double* stats, bool* gate) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = 3 * h->nt;
    SLAM_HIP_TRY(hipStreamSynchronize(h->cstream));
    const CertState ct = *h->cert_host;
    const double lam0 = cs.lam[0] * gate_ritz_scale();
    double* g = h->gate_info;
    g[0] = 1.0;
    g[6] = lam0;
    g[7] = cs.lam[1];
    g[8] = ct.trp2;
    g[9] = (double)n;
    g[10] = cs.iter;
    // ---- cond (:495)
    const double inf = std::numeric_limits<double>::infinity();
    double cond = (cs.status == 4 || !(lam0 > 0.0)) ? inf : cs.lam[1] / lam0;
    int cond_dec;
    if ((cs.status == 5 && kCertEarlyMargin * cond < h->cfg.cond_max) ||
        (cs.status == 1 && kCertConvMargin * cond < h->cfg.cond_max))
        cond_dec = 1;
    else if (cs.status == 1 && cond < h->cfg.cond_max) cond_dec = 5;    // converged, inside the band
    else if (cs.status == 2 || cs.status == 4) cond_dec = 0;
    else cond_dec = -1;
    if (cond_dec < 0 && n <= kGraphDenseMax) {
        GTRY(dense_cond(h, &cond));
        cond_dec = cond < h->cfg.cond_max ? 3 : 2;
    }
    g[2] = cond_dec;
    g[5] = cond;
    g[13] = (cond > 0.0) ? h->cfg.cond_max / cond : inf;
    // ---- det (:494)
    const double ln_min = h->cfg.det_min > 0.0 ? std::log(h->cfg.det_min) : -inf;
    const double hi = ct.logdet_m;                 // Fischer: det H <= prod det M_i
    const bool have = ct.bad == 0 && lam0 > 0.0 && ct.trm_max > 0.0 && cs.status != 4;
    const double a1 = have ? lam0 / ct.trm_max : 0.0;     // a at margin 1
    double lo = -inf;
    if (have) lo = logdet_lower(ct, a1 / kGateDetMargin, n);
    // the largest margin F with the lower end still above ln det_min (lo falls as a does)
    double fmax = 0.0;
    if (have && logdet_lower(ct, a1, n) > ln_min) {
        double l = 0.0, u = 700.0;                 // ln F
        if (logdet_lower(ct, a1 * std::exp(-u), n) > ln_min) l = u;
        for (int it = 0; it < 60 && u - l > 1e-3; ++it) {
            const double m = 0.5 * (l + u);
            if (logdet_lower(ct, a1 * std::exp(-m), n) > ln_min) l = m;
            else u = m;
        }
        fmax = std::exp(l);
    }
    g[3] = lo;
    g[4] = hi;
    g[12] = fmax;
    int det_dec;
    double det;
    if (ct.bad == 0 && lo > ln_min) {
        det_dec = 1;                               // passed with the margin
        det = std::exp(lo);                        // det >= this unless the margin failed (inf past the double range, as numpy)
    } else if (ct.bad == 0 && hi < ln_min) {
        det_dec = 0;                               // rejected by the upper bound
        det = std::exp(hi);                        // det <= this
    } else if (n <= kGraphDenseMax) {
        GTRY(dense_det(h, &det));                  // the reference's own det (numpy's LU)
        det_dec = (h->cfg.det_min < det) ? 3 : 2;
    } else {
        det_dec = -1;
        det = std::numeric_limits<double>::quiet_NaN();
    }
    g[1] = det_dec;
    g[0] = (det_dec >= 2 || (cond_dec >= 2 && cond_dec <= 3)) ? 2.0 : 1.0;   // 2: a half took the dense path's value
    stats[2] = det;
    stats[3] = cond;
    *gate = (det_dec == 1 || det_dec == 3) && (cond_dec == 1 || cond_dec == 3 || cond_dec == 5);
    g[11] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SLAM_OK;
}

// The factors of the preconditioner in force on the assembled system: the
// block-Jacobi inverses always (the condition estimate and the gate use them),
// the chain factor beside them when it is in force.
int precond_factor(slam_graph* h) {
    hipLaunchKernelGGL(graph_block_inv_kernel, dim3(nblk(h->nt)), dim3(256), 0, h->stream, h->nt,
                       h->dslot, h->val, h->minv);
    if (h->pc_kind == SLAM_GRAPH_PRECOND_CHAIN) {
        SLAM_HIP_TRY(hipMemsetAsync(h->pc_cnt, 0, 2 * sizeof(int32_t), h->stream));
        const int64_t nseg = (h->nt + h->pc_seg - 1) / h->pc_seg;
        hipLaunchKernelGGL(graph_chain_factor_kernel, dim3(nblk(nseg, 64)), dim3(64), 0, h->stream,
                           h->nt, h->pc_seg, h->rptr, h->scol, h->dslot, h->val, h->fac, h->pc_cnt);
    }
    h->pc_ready = true;
    return SLAM_OK;
}

// PCG on H delta = -b with block-Jacobi, or with the chain preconditioner when
// slam_graph_set_precond put it in force (large trajectories): two launches per
// iteration, enqueued in chunks between host polls of the device state.  The
// gate's condition number (:495) is estimated on a second stream at the same
// time (cond_mode SLAM_GRAPH_COND_ESTIMATE); the solve is applied only if the
// gate passes, as the reference inverts H only then (:496-497).
int solve_pcg(slam_graph* h, double* stats, bool* solved, int32_t* iters) {
    const int64_t n = 3 * h->nt;
    const unsigned nb = nblk(n, kPcgThreads);
    const bool cert = (h->cfg.cond_mode == SLAM_GRAPH_COND_MARGIN);
    const bool est = (h->cfg.cond_mode == SLAM_GRAPH_COND_ESTIMATE) || cert;   // the estimate runs
    const bool chain = (h->pc_kind == SLAM_GRAPH_PRECOND_CHAIN);
    GTRY(precond_factor(h));
    if (est) {
        SLAM_HIP_TRY(hipEventRecord(h->cev[0], h->stream));
        SLAM_HIP_TRY(hipStreamWaitEvent(h->cstream, h->cev[0], 0));
        SLAM_HIP_TRY(hipEventRecord(h->cev[1], h->cstream));
    }
    if (cert) GTRY(cert_enqueue(h));
    if (chain)
        hipLaunchKernelGGL(graph_pcg_start_kernel<true>, dim3(nb), dim3(kPcgThreads), 0, h->stream, n,
                           h->minv, h->b, h->delta, h->r, h->z, h->part, h->fac, h->pc_seg,
                           h->pc_cnt);
    else
        hipLaunchKernelGGL(graph_pcg_start_kernel<false>, dim3(nb), dim3(kPcgThreads), 0, h->stream,
                           n, h->minv, h->b, h->delta, h->r, h->z, h->part, nullptr, 0, nullptr);
    SLAM_HIP_TRY(hipGetLastError());
    PcgState& s = *h->pcg_host;
    CondState& cs = *h->cond_host;
    s = PcgState{};
    cs = CondState{};
    // The first batch runs through the previous solve's iteration count (the
    // Gauss-Newton steps of one edge set converge in similar counts), so a
    // repeated solve usually needs a single host poll; then batches of 8.
    int32_t k_end = std::max<int32_t>(16, std::min<int32_t>(h->pcg_last_iters + 1, 1024));
    int32_t c_end = std::max<int32_t>(cond_win() + 1, std::min<int32_t>(h->cond_last_iters + 1, 1024));
    bool pcg_done = false, cond_done = !est, abandoned = false;
    int32_t k0 = 0, c0 = 0;
    while (!pcg_done || !cond_done) {
        // the two streams' launches interleaved in proportion to their batch
        // lengths, so the estimate starts with the solve instead of after the
        // host has enqueued the whole PCG batch (~1 ms of launch calls)
        const int32_t np = pcg_done ? 0 : k_end - k0;
        const int32_t nc = cond_done ? 0 : c_end - c0;
        for (int32_t ip = 0, ic = 0; ip < np || ic < nc;) {
            if (ic < nc && (ip >= np || (int64_t)ic * np <= (int64_t)ip * nc)) {
                GTRY(cond_enqueue(h, c0 + ic, 1));
                ++ic;
            } else {
                const int32_t k = k0 + ip;
                hipLaunchKernelGGL(graph_pcg_dir_spmv_kernel, dim3(nb), dim3(kSpmvThreads), 0,
                                   h->stream, h->nt, k, h->rptr, h->scol, h->val, h->z, h->p, h->q,
                                   h->part, h->st, h->cfg.pcg_tol, h->cfg.pcg_max_iter);
                if (chain)
                    hipLaunchKernelGGL(graph_pcg_step_kernel<true>, dim3(nb), dim3(kPcgThreads), 0,
                                       h->stream, n, k, h->minv, h->p, h->q, h->delta, h->r, h->z,
                                       h->part, h->st, h->fac, h->pc_seg);
                else
                    hipLaunchKernelGGL(graph_pcg_step_kernel<false>, dim3(nb), dim3(kPcgThreads), 0,
                                       h->stream, n, k, h->minv, h->p, h->q, h->delta, h->r, h->z,
                                       h->part, h->st, nullptr, 0);
                ++ip;
            }
        }
        SLAM_HIP_TRY(hipGetLastError());
        if (!pcg_done)
            SLAM_HIP_TRY(hipMemcpyAsync(h->pcg_host, h->st, sizeof(PcgState), hipMemcpyDeviceToHost,
                                        h->stream));
        if (!cond_done)
            SLAM_HIP_TRY(hipMemcpyAsync(h->cond_host, h->cst, sizeof(CondState), hipMemcpyDeviceToHost,
                                        h->cstream));
        if (!pcg_done) {
            SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
            pcg_done = s.done;
            k0 = k_end;
            k_end += 8;
        }
        if (!cond_done) {
            SLAM_HIP_TRY(hipStreamSynchronize(h->cstream));
            cond_done = cs.done;
            c0 = c_end;
            c_end += 16;
            // the gate rejects H for certain (cond >= cond_max, or not positive
            // definite): the reference does not solve (:496), neither do we
            if (cs.done && (cs.status == 2 || cs.status == 4) && !pcg_done) {
                pcg_done = true;
                abandoned = true;
            }
        }
    }
    *iters = s.iter;
    h->pcg_last_iters = (s.status == 1) ? s.iter : 0;
    const bool pcg_ok = (s.status == 1);
    stats[2] = std::numeric_limits<double>::quiet_NaN();     // det: not formed at this size
    stats[3] = std::numeric_limits<double>::quiet_NaN();
    bool gate = true;
    for (double& v : h->cond_info) v = 0.0;
    for (double& v : h->gate_info) v = 0.0;
    if (est) {
        SLAM_HIP_TRY(hipEventRecord(h->cev[2], h->cstream));
        SLAM_HIP_TRY(hipEventSynchronize(h->cev[2]));
        float ms = 0.f;
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->cev[1], h->cev[2]));
        const double cond = (cs.status == 4 || !(cs.lam[0] > 0.0))
                                ? std::numeric_limits<double>::infinity()
                                : cs.lam[1] / cs.lam[0];
        stats[3] = cond;
        // :496 -- only a converged estimate certifies cond < cond_max: Ritz
        // values lie inside [lambda_min, lambda_max], so an estimate stopped
        // at cond_max_iter (status 3) only bounds cond from below and cannot
        // pass the gate; status 2 / 4 reject for certain
        gate = (cs.status == 1) && cond < h->cfg.cond_max;
        h->cond_warm = (cs.status == 1 || cs.status == 3 || cs.status == 5);
        h->cond_last_iters = (cs.status == 1 || cs.status == 5) ? cs.iter : 0;
        h->cond_info[0] = cs.iter;
        h->cond_info[1] = cs.status;
        h->cond_info[2] = cs.lam[0];
        h->cond_info[3] = cs.lam[1];
        h->cond_info[4] = cs.iters_side[0];
        h->cond_info[5] = cs.iters_side[1];
        h->cond_info[6] = ms;
        if (cert && pcg_ok && !abandoned) GTRY(cert_gate(h, cs, stats, &gate));
    }
    *solved = pcg_ok && gate && !abandoned;
    h->pcg_failed = !pcg_ok && !abandoned;
    if (abandoned) {
        *iters = -1;
        h->pcg_last_iters = 0;
    }
    return SLAM_OK;
}

int do_update(slam_graph* h, double* stats) {
    stats[0] = stats[1] = stats[2] = stats[3] = 0.0;
    for (double& x : h->last) x = 0.0;
    h->pcg_failed = false;
    if (h->E == 0 || 3 * h->nt <= 3) return SLAM_OK;        // :469 (leng > 3)
    GTRY(linearize_assemble(h));
    h->assembled = true;
    const int64_t n = 3 * h->nt;
    const bool dense = (h->cfg.solver == SLAM_GRAPH_DENSE) ||
                       (h->cfg.solver == SLAM_GRAPH_AUTO && n <= kGraphDenseMax);
    if (dense && n > kGraphDenseMax)
        return fail(SLAM_ERR_ARG, "slam_graph_update: dense solver limited to 2048 unknowns");
    bool solved = false;
    int32_t iters = 0;
    if (dense) GTRY(solve_dense(h, stats, &solved));
    else GTRY(solve_pcg(h, stats, &solved, &iters));
    SLAM_HIP_TRY(hipEventRecord(h->ev[3], h->stream));
    if (solved) {
        hipLaunchKernelGGL(graph_pose_update_kernel, dim3(nblk(h->nt)), dim3(256), 0, h->stream,
                           h->nt, h->times, h->delta, h->poses, h->part);
        hipLaunchKernelGGL(graph_dsum_kernel, dim3(1), dim3(1024), 0, h->stream,
                           (int64_t)nblk(h->nt), h->part, h->dsum);
        SLAM_HIP_TRY(hipGetLastError());
        SLAM_HIP_TRY(hipMemcpyAsync(&stats[1], h->dsum, sizeof(double), hipMemcpyDeviceToHost,
                                    h->stream));
        stats[0] = 1.0;
    }
    SLAM_HIP_TRY(hipEventRecord(h->ev[4], h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    float ms;
    for (int k = 0; k < 4; ++k) {
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        h->last[k] = ms;
    }
    h->last[4] = iters;
    return SLAM_OK;
}

// ---- members (graph_members.inl)
// the linearise launches of launch_linearize over the members that are active
int launch_linearize_members(slam_graph* h) {
    const int32_t kind = h->robust_kind;
    const int64_t n_od = h->E - h->E_lm;
    double* rows = nullptr;
    if (kind != SLAM_GRAPH_ROBUST_NONE) {
        GTRY(robust_reserve(h));
        rows = robust_rows(h).lin;
    }
#define SLAM_LINEARIZE_MEMBERS(K)                                                                  \
    hipLaunchKernelGGL(graph_member_linearize_kernel<K>, dim3(nblk(h->E_lm)), dim3(256), 0,        \
                       h->stream, h->E_lm, h->E, h->edges, h->poses, gconst(h->cfg), h->blocks,    \
                       h->robust_param, rows, h->m_edge, h->m_active)
    if (h->E_lm) switch (kind) {
            case SLAM_GRAPH_ROBUST_HUBER: SLAM_LINEARIZE_MEMBERS(SLAM_GRAPH_ROBUST_HUBER); break;
            case SLAM_GRAPH_ROBUST_CAUCHY: SLAM_LINEARIZE_MEMBERS(SLAM_GRAPH_ROBUST_CAUCHY); break;
            case SLAM_GRAPH_ROBUST_DCS: SLAM_LINEARIZE_MEMBERS(SLAM_GRAPH_ROBUST_DCS); break;
            default: SLAM_LINEARIZE_MEMBERS(SLAM_GRAPH_ROBUST_NONE); break;
        }
#undef SLAM_LINEARIZE_MEMBERS
    if (n_od)
        hipLaunchKernelGGL(graph_member_linearize_odom_kernel, dim3(nblk(n_od)), dim3(256), 0,
                           h->stream, h->E_lm, h->E, h->edges, h->poses, h->blocks, rows, h->m_edge,
                           h->m_active);
    h->lin_kind = kind;
    h->pc_kind = h->precond_kind;                  // accepted, without effect (the dense path)
    h->pc_seg = (h->pc_kind == SLAM_GRAPH_PRECOND_CHAIN) ? h->precond_seg : 1;
    h->pc_ready = false;
    return SLAM_OK;
}

// One updateEstPose of every member with act[m] != 0, all members per launch;
// stats [B][4], zero rows for the others and for a member that is never solved.
// Two synchronisations: the members' LU / Lanczos results for the host's gate
// (formed as dense_factor_gate forms it), and the sums of delta^2.
int do_update_members(slam_graph* h, const std::vector<char>& act, double* stats) {
    const int64_t B = h->B;
    std::fill(stats, stats + 4 * B, 0.0);
    for (double& x : h->last) x = 0.0;
    h->pcg_failed = false;
    if (h->E == 0) return SLAM_OK;
    bool any = false;
    for (int64_t m = 0; m < B; ++m) {
        h->m_flags_host[m] = (act[m] && h->members[m].n > 0) ? 1 : 0;
        any = any || h->m_flags_host[m];
    }
    if (!any) return SLAM_OK;
    hipStream_t s = h->stream;
    const dim3 per_member((unsigned)B), split((unsigned)B, kMemberSplit), wg(kGraphThreads);
    SLAM_HIP_TRY(hipMemcpyAsync(h->m_active, h->m_flags_host, B * sizeof(int32_t),
                                hipMemcpyHostToDevice, s));
    SLAM_HIP_TRY(hipEventRecord(h->ev[0], s));
    GTRY(launch_linearize_members(h));
    SLAM_HIP_TRY(hipEventRecord(h->ev[1], s));
    hipLaunchKernelGGL(graph_member_assemble_h_kernel, dim3(nblk(9 * h->n_slots)), dim3(256), 0, s,
                       h->n_slots, h->E, h->cptr, h->clist, h->blocks, h->cfg.anchor, h->val,
                       h->m_slot, h->m_desc, h->dslot, h->m_active);
    hipLaunchKernelGGL(graph_member_assemble_b_kernel, dim3(nblk(3 * h->nt)), dim3(256), 0, s,
                       h->nt, h->E, h->bptr, h->blist, h->blocks, h->b, h->m_row, h->m_active);
    SLAM_HIP_TRY(hipEventRecord(h->ev[2], s));
    h->assembled = true;
    hipLaunchKernelGGL(graph_member_zero_kernel, split, wg, 0, s, h->m_desc, h->m_active, h->A);
    hipLaunchKernelGGL(graph_member_scatter_kernel, dim3(nblk(9 * h->n_slots)), dim3(256), 0, s,
                       h->n_slots, h->srow, h->scol, h->val, h->m_slot, h->m_desc, h->m_active, h->A);
    hipLaunchKernelGGL(graph_member_symmetrize_kernel, split, wg, 0, s, h->m_desc, h->m_active,
                       h->A, h->S, h->LU);
    hipLaunchKernelGGL(graph_member_lu_kernel, per_member, wg, 0, s, h->m_desc, h->m_active, h->LU,
                       h->piv, h->m_luout);
    hipLaunchKernelGGL(graph_member_lanczos_kernel, per_member, wg, 0, s, h->m_desc, h->m_active,
                       h->S, h->V, h->lan, h->m_luout, (uint64_t)0x5EEDULL);
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipMemcpyAsync(h->m_out_host, h->m_luout, kMemberOut * B * sizeof(double),
                                hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));
    int32_t* pass = h->m_flags_host + B;
    for (int64_t m = 0; m < B; ++m) {
        pass[m] = 0;
        if (!h->m_flags_host[m]) continue;
        // numpy det: sign * exp(logdet); a zero pivot gives 0 (getrf info > 0)
        const double* lo = h->m_out_host + kMemberOut * m;
        const double det = (lo[2] != 0.0) ? 0.0 : lo[0] * std::exp(lo[1]);
        const double cond = (lo[4] > 0.0) ? lo[3] / lo[4] : std::numeric_limits<double>::infinity();
        stats[4 * m + 2] = det;
        stats[4 * m + 3] = cond;
        pass[m] = ((h->cfg.det_min < det) && (cond < h->cfg.cond_max)) ? 1 : 0;
    }
    SLAM_HIP_TRY(hipMemcpyAsync(h->m_pass, pass, B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(graph_member_lu_solve_kernel, per_member, wg, 0, s, h->m_desc, h->m_active,
                       h->m_pass, h->LU, h->piv, h->b, h->delta);
    SLAM_HIP_TRY(hipEventRecord(h->ev[3], s));
    hipLaunchKernelGGL(graph_member_pose_update_kernel, per_member, dim3(1024), 0, s, h->m_desc,
                       h->m_active, h->m_pass, h->times, h->delta, h->poses, h->m_dsum);
    SLAM_HIP_TRY(hipGetLastError());
    double* dsum = h->m_out_host + kMemberOut * B;
    SLAM_HIP_TRY(hipMemcpyAsync(dsum, h->m_dsum, B * sizeof(double), hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipEventRecord(h->ev[4], s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));
    for (int64_t m = 0; m < B; ++m)
        if (pass[m]) {
            stats[4 * m] = 1.0;
            stats[4 * m + 1] = dsum[m];
        }
    float ms;
    for (int k = 0; k < 4; ++k) {
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        h->last[k] = ms;
    }
    return SLAM_OK;
}

// ---- slam_graph_marginals (graph_marginals.inl)
constexpr int kMargDefaultCols = 4;    // least time per column at config 5
constexpr int kMargWidths[] = {1, 2, 4, 8};
static_assert(kMargDefaultCols <= kMargMaxCols, "MargState holds the widest pass");

// the call's device buffers, carved from one grow-only allocation of h->marg
struct MargBuffers {
    double *minv, *x, *r, *z, *p, *q, *part, *tot, *cov;
    int64_t* qidx;
    MargState* st;
};

int marg_buffers(slam_graph* h, int64_t M, bool pcg, int cols, MargBuffers* mb) {
    const int64_t n = 3 * h->nt;
    const int64_t nv = pcg ? n * cols : 0;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c{pass ? h->marg_arena : nullptr};
        mb->cov = c.take<double>(M * M);
        mb->qidx = c.take<int64_t>(M);
        mb->st = c.take<MargState>(1);
        mb->minv = c.take<double>(pcg ? 9 * h->nt : 0);
        mb->x = c.take<double>(nv);
        mb->r = c.take<double>(nv);
        mb->z = c.take<double>(nv);
        mb->p = c.take<double>(nv);
        mb->q = c.take<double>(nv);
        mb->part = c.take<double>(pcg ? 3 * (int64_t)nblk(n, kPcgThreads) * cols : 0);
        mb->tot = c.take<double>(3 * kMargMaxCols);
        if (pass == 0 && c.off > h->marg_bytes) {
            h->marg.release(h->marg_arena);
            h->marg_bytes = 0;
            GTRY(h->marg.alloc(&h->marg_arena, c.off));
            h->marg_bytes = c.off;
        }
    }
    if (!h->marg_host) {
        GTRY(h->marg.alloc_pinned(&h->marg_host, nullptr, 1, hipHostMallocDefault));
        for (auto& e : h->marg_ev) GTRY(h->marg.event(&e));
    }
    return SLAM_OK;
}

template <int W>
void marg_start(slam_graph* h, const MargBuffers& mb, int64_t j0, int64_t M) {
    const int64_t n = 3 * h->nt;
    hipLaunchKernelGGL(graph_marg_start_kernel<W>, dim3(nblk(n, kPcgThreads)), dim3(kPcgThreads), 0,
                       h->stream, n, mb.minv, mb.qidx, j0, M, mb.x, mb.r, mb.z, mb.part, mb.st);
}

// redundant folds (default): two launches per iteration; fold_launch: the
// partials folded by a one-workgroup launch before each of them (four launches,
// the same bits; SLAM_GRAPH_MARG_FOLD=1, measured and not kept: DESIGN 8.2)
template <int W>
void marg_iterations(slam_graph* h, const MargBuffers& mb, int32_t k0, int32_t k1, bool fold_launch) {
    const int64_t n = 3 * h->nt;
    const unsigned nb = nblk(n, kPcgThreads);
    hipStream_t s = h->stream;
    for (int32_t k = k0; k < k1; ++k) {
        if (fold_launch) {
            hipLaunchKernelGGL((graph_marg_fold_kernel<kSpmvThreads, W, 2>), dim3(1), dim3(kSpmvThreads),
                               0, s, (int64_t)nb, mb.part, 1, mb.tot);
            hipLaunchKernelGGL((graph_marg_dir_spmm_kernel<W, true>), dim3(nb), dim3(kSpmvThreads), 0, s,
                               h->nt, k, h->rptr, h->scol, h->val, mb.z, mb.p, mb.q, mb.part, mb.tot,
                               mb.st, h->cfg.pcg_tol, h->cfg.pcg_max_iter);
            hipLaunchKernelGGL((graph_marg_fold_kernel<kPcgThreads, W, 1>), dim3(1), dim3(kPcgThreads),
                               0, s, (int64_t)nb, mb.part, 0, mb.tot);
            hipLaunchKernelGGL((graph_marg_step_kernel<W, true>), dim3(nb), dim3(kPcgThreads), 0, s, n,
                               k, mb.minv, mb.p, mb.q, mb.x, mb.r, mb.z, mb.part, mb.tot, mb.st);
        } else {
            hipLaunchKernelGGL((graph_marg_dir_spmm_kernel<W, false>), dim3(nb), dim3(kSpmvThreads), 0, s,
                               h->nt, k, h->rptr, h->scol, h->val, mb.z, mb.p, mb.q, mb.part, mb.tot,
                               mb.st, h->cfg.pcg_tol, h->cfg.pcg_max_iter);
            hipLaunchKernelGGL((graph_marg_step_kernel<W, false>), dim3(nb), dim3(kPcgThreads), 0, s, n,
                               k, mb.minv, mb.p, mb.q, mb.x, mb.r, mb.z, mb.part, mb.tot, mb.st);
        }
    }
}

#define MARG_DISPATCH(W, fn, ...)                 \
    switch (W) {                                  \
        case 1: fn<1>(__VA_ARGS__); break;        \
        case 2: fn<2>(__VA_ARGS__); break;        \
        case 4: fn<4>(__VA_ARGS__); break;        \
        default: fn<8>(__VA_ARGS__); break;       \
    }

// One pass of W columns (requests j0 .. j0 + W - 1, those past M padding) in the
// manner of solve_pcg: enqueue a batch of iterations, poll a pinned copy of the
// state.  The final state is left in *h->marg_host.
int marg_pass(slam_graph* h, const MargBuffers& mb, int W, int64_t j0, int64_t M) {
    MARG_DISPATCH(W, marg_start, h, mb, j0, M);
    const char* fe = std::getenv("SLAM_GRAPH_MARG_FOLD");
    const bool fold_launch = fe && fe[0] == '1';
    const MargState& s = *h->marg_host;
    int32_t k0 = 0;
    int32_t k1 = std::max<int32_t>(16, std::min<int32_t>(h->marg_last_iters + 1, 1024));
    for (;;) {
        MARG_DISPATCH(W, marg_iterations, h, mb, k0, k1, fold_launch);
        SLAM_HIP_TRY(hipGetLastError());
        SLAM_HIP_TRY(hipMemcpyAsync(h->marg_host, mb.st, sizeof(MargState), hipMemcpyDeviceToHost,
                                    h->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        if (s.done[0] || s.done[1]) break;
        k0 = k1;
        k1 += 16;
    }
    return SLAM_OK;
}

// the PCG path: passes of at most `cols` columns; a pass narrower than that runs
// at the smallest instantiated width that holds it (the bits do not depend on
// the width).  Stops at the first pass with a column that did not converge.
int marg_pcg(slam_graph* h, const MargBuffers& mb, int64_t M, int cols, double* info) {
    hipLaunchKernelGGL(graph_block_inv_kernel, dim3(nblk(h->nt)), dim3(256), 0, h->stream, h->nt,
                       h->dslot, h->val, mb.minv);
    bool ok = true;
    int32_t passes = 0, max_iter = 0;
    double worst = 0.0;
    for (int64_t j0 = 0; j0 < M && ok; j0 += cols) {
        int W = cols;
        for (int w : kMargWidths)
            if (w >= M - j0 && w < W) W = w;
        GTRY(marg_pass(h, mb, W, j0, M));
        ++passes;
        const MargState& s = *h->marg_host;
        int32_t pass_iter = 0;
        for (int c = 0; c < W && j0 + c < M; ++c) {
            ok = ok && s.status[c] == 1;
            pass_iter = std::max(pass_iter, s.iter[c]);
            const double rel = std::sqrt(s.rr[c] / s.rr0[c]);
            if (!(rel <= worst)) worst = rel;      // a NaN residual is the worst
        }
        max_iter = std::max(max_iter, pass_iter);
        h->marg_last_iters = ok ? pass_iter : 0;
        hipLaunchKernelGGL(graph_marg_extract_kernel, dim3(nblk(M * W)), dim3(256), 0, h->stream, M, W,
                           j0, mb.qidx, mb.x, mb.cov);
        SLAM_HIP_TRY(hipGetLastError());
    }
    info[0] = ok ? 1.0 : 0.0;
    info[1] = passes;
    info[2] = max_iter;
    info[3] = worst;
    return SLAM_OK;
}

// the dense path: the reference's gate on this H, then one workgroup per column
int marg_dense(slam_graph* h, const MargBuffers& mb, int64_t M, double* info) {
    double det, cond;
    bool pass = false;
    GTRY(dense_factor_gate(h, &det, &cond, &pass));
    if (pass) {
        hipLaunchKernelGGL(graph_marg_lu_cols_kernel, dim3((unsigned)M), dim3(kMargDenseThreads), 0,
                           h->stream, h->LU, (int)(3 * h->nt), h->piv, mb.qidx, M, mb.cov);
        SLAM_HIP_TRY(hipGetLastError());
    }
    info[0] = pass ? 1.0 : 0.0;
    info[1] = 1.0;
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_graph_create(const slam_graph_config* cfg, int device, slam_graph** out) {
    SLAM_ARG_CHECK(cfg && out, "slam_graph_create: NULL argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(SLAM_ERR_ARG, "slam_graph_create: no such HIP device");
    SLAM_HIP_TRY(hipSetDevice(device));
    HandlePtr<slam_graph, slam_graph_destroy> hp(new slam_graph());
    slam_graph* h = hp.get();
    h->cfg = *cfg;
    if (h->cfg.pcg_max_iter <= 0) h->cfg.pcg_max_iter = 10000;
    if (!(h->cfg.cond_tol > 0.0)) h->cfg.cond_tol = 1e-5;
    if (h->cfg.cond_max_iter <= 0) h->cfg.cond_max_iter = 3000;
    if (!(h->cfg.pcg_tol > 0.0)) h->cfg.pcg_tol = 1e-10;
    h->device = device;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking) != hipSuccess)
        return fail(SLAM_ERR_HIP, "slam_graph_create: stream creation failed");
    DeviceMem& m = h->mem;
    for (auto& e : h->ev)
        if (m.event(&e)) return fail(SLAM_ERR_HIP, "slam_graph_create: event creation failed");
    for (auto& e : h->cev)
        if (m.event(&e)) return fail(SLAM_ERR_HIP, "slam_graph_create: event creation failed");
    if (m.alloc_pinned(&h->pcg_host, nullptr, 1, hipHostMallocDefault) ||
        m.alloc_pinned(&h->cond_host, nullptr, 1, hipHostMallocDefault) ||
        m.alloc_pinned(&h->cert_host, nullptr, 1, hipHostMallocDefault))
        return fail(SLAM_ERR_HIP, "slam_graph_create: pinned state buffers");
    *out = hp.release();
    return SLAM_OK;
}

int slam_graph_destroy(slam_graph* h) {
    if (!h) return SLAM_OK;
    (void)hipSetDevice(h->device);
    for (hipStream_t s : {h->cstream, h->stream})
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    delete h;
    return SLAM_OK;
}

int slam_graph_set_poses(slam_graph* h, int64_t n_poses, const double* poses) {
    SLAM_ARG_CHECK(h && poses && n_poses >= 1, "slam_graph_set_poses: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (h->B) clear_members(h);                    // the members go, and their edge set with them
    if (n_poses != h->T) {
        h->map_set = false;                        // the observations index the poses that go
        h->mem.release(h->poses);
        h->T = 0;
        const int rc = h->mem.alloc(&h->poses, 3 * (size_t)n_poses);
        if (rc) return rc;
        h->T = n_poses;
    }
    SLAM_HIP_TRY(hipMemcpyAsync(h->poses, poses, 3 * n_poses * sizeof(double),
                                hipMemcpyHostToDevice, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_graph_get_poses(slam_graph* h, double* poses) {
    SLAM_ARG_CHECK(h && poses && h->poses, "slam_graph_get_poses: no poses");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    SLAM_HIP_TRY(hipMemcpyAsync(poses, h->poses, 3 * h->T * sizeof(double), hipMemcpyDeviceToHost,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_graph_set_edges(slam_graph* h, int64_t n_edges, const slam_graph_edge* edges) {
    SLAM_ARG_CHECK(h && n_edges >= 0 && (edges || n_edges == 0), "slam_graph_set_edges: bad arguments");
    SLAM_ARG_CHECK(h->poses, "slam_graph_set_edges: set the poses first");
    return set_edge_set(h, n_edges, edges, 0, nullptr, "slam_graph_set_edges");
}

int slam_graph_set_edges_odom(slam_graph* h, int64_t n_edges, const slam_graph_edge* edges,
                              int64_t n_odom, const slam_graph_odom* odom) {
    SLAM_ARG_CHECK(h, "slam_graph_set_edges_odom: NULL handle");
    SLAM_ARG_CHECK(n_edges >= 0 && n_odom >= 0, "slam_graph_set_edges_odom: negative count");
    SLAM_ARG_CHECK((edges || n_edges == 0) && (odom || n_odom == 0),
                   "slam_graph_set_edges_odom: NULL array with a positive count");
    SLAM_ARG_CHECK(h->poses, "slam_graph_set_edges_odom: set the poses first");
    return set_edge_set(h, n_edges, edges, n_odom, odom, "slam_graph_set_edges_odom");
}

int slam_graph_update(slam_graph* h, double* stats) {
    SLAM_ARG_CHECK(h && stats && h->poses, "slam_graph_update: bad arguments");
    SLAM_ARG_CHECK(h->B == 0, "slam_graph_update: the handle has members (slam_graph_update_members)");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    return do_update(h, stats);
}

int slam_graph_optimize(slam_graph* h, double delta_sum_th, int32_t max_iter, double* stats,
                        int32_t* n_iter) {
    SLAM_ARG_CHECK(h && h->poses && max_iter >= 1, "slam_graph_optimize: bad arguments");
    SLAM_ARG_CHECK(h->B == 0,
                   "slam_graph_optimize: the handle has members (slam_graph_optimize_members)");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int32_t it = 0;
    double s[4] = {0, 0, 0, 0};
    double dsum = delta_sum_th;
    while (delta_sum_th <= dsum && it < max_iter) {            // :692
        GTRY(do_update(h, s));
        if (stats) std::memcpy(stats + 4 * it, s, sizeof(s));
        dsum = s[1];
        ++it;
        // is_calc = 0 ends the loop as in the reference (:706-709: sum delta^2 = 0);
        // on the PCG path that is a solver failure, not a converged trajectory
        if (h->pcg_failed) {
            if (n_iter) *n_iter = it;
            return fail(SLAM_ERR_SOLVE, "slam_graph_optimize: PCG did not converge within "
                                        "pcg_max_iter iterations; poses left at the last "
                                        "converged Gauss-Newton step");
        }
    }
    if (n_iter) *n_iter = it;
    return SLAM_OK;
}

int slam_graph_set_members(slam_graph* h, int64_t n_members, const int64_t* pose_off) {
    SLAM_ARG_CHECK(h, "slam_graph_set_members: NULL handle");
    SLAM_ARG_CHECK(n_members >= 0 && (pose_off || n_members == 0),
                   "slam_graph_set_members: negative count, or NULL offsets with a positive count");
    if (n_members) {
        SLAM_ARG_CHECK(h->poses, "slam_graph_set_members: set the poses first");
        SLAM_ARG_CHECK(h->cfg.solver != SLAM_GRAPH_PCG,
                       "slam_graph_set_members: members take the dense path, the handle's solver is PCG");
        SLAM_ARG_CHECK(n_members <= h->T && pose_off[0] == 0 && pose_off[n_members] == h->T,
                       "slam_graph_set_members: the offsets must run from 0 to the pose count");
        for (int64_t m = 0; m < n_members; ++m) {
            SLAM_ARG_CHECK(pose_off[m] < pose_off[m + 1],
                           "slam_graph_set_members: the offsets must increase strictly");
            SLAM_ARG_CHECK(pose_off[m + 1] - pose_off[m] <= kGraphDenseMax / 3,
                           "slam_graph_set_members: a member is limited to 682 poses (2046 unknowns)");
        }
    }
    clear_members(h);
    if (n_members) h->map_set = false;             // no map of members
    h->B = n_members;
    if (n_members) h->pose_off.assign(pose_off, pose_off + n_members + 1);
    return SLAM_OK;
}

int slam_graph_update_members(slam_graph* h, double* stats) {
    SLAM_ARG_CHECK(h && stats, "slam_graph_update_members: NULL argument");
    SLAM_ARG_CHECK(h->B > 0 && h->poses,
                   "slam_graph_update_members: the handle has no members (slam_graph_set_members)");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    return do_update_members(h, std::vector<char>((size_t)h->B, 1), stats);
}

int slam_graph_optimize_members(slam_graph* h, double delta_sum_th, int32_t max_iter, double* stats,
                                int32_t* n_iter) {
    SLAM_ARG_CHECK(h && n_iter && max_iter >= 1, "slam_graph_optimize_members: bad arguments");
    SLAM_ARG_CHECK(h->B > 0 && h->poses,
                   "slam_graph_optimize_members: the handle has no members (slam_graph_set_members)");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const int64_t B = h->B;
    if (stats) std::fill(stats, stats + 4 * B * (int64_t)max_iter, 0.0);
    // every member runs the loop of slam_graph_optimize (:692) on its own sum
    const bool first = delta_sum_th <= delta_sum_th;           // false for a NaN threshold, as there
    std::vector<char> act((size_t)B, first ? 1 : 0);
    std::vector<int32_t> it((size_t)B, 0);
    std::vector<double> st((size_t)(4 * B));
    for (bool any = first; any;) {
        GTRY(do_update_members(h, act, st.data()));
        any = false;
        for (int64_t m = 0; m < B; ++m) {
            if (!act[m]) continue;
            if (stats) std::memcpy(stats + 4 * (m * max_iter + it[m]), &st[4 * m], 4 * sizeof(double));
            ++it[m];
            act[m] = (delta_sum_th <= st[4 * m + 1] && it[m] < max_iter) ? 1 : 0;
            any = any || act[m];
        }
    }
    std::copy(it.begin(), it.end(), n_iter);
    return SLAM_OK;
}

int slam_graph_get_system(slam_graph* h, int64_t* n_times, int64_t* times, double* H, double* b,
                          double* blocks) {
    SLAM_ARG_CHECK(h && n_times, "slam_graph_get_system: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    *n_times = h->nt;
    if (times) std::memcpy(times, h->times_h.data(), h->nt * sizeof(int64_t));
    const int64_t n = 3 * h->nt;
    DeviceMem union_h;             // with members h->A holds their matrices, not the union's
    if (H) {
        double* A = h->A;
        if (h->B) {
            SLAM_ARG_CHECK(n <= kGraphDenseMax, "slam_graph_get_system: dense H only up to 2048 unknowns");
            GTRY(union_h.alloc(&A, (size_t)(n * n)));
        }
        SLAM_ARG_CHECK(A, "slam_graph_get_system: dense H only up to 2048 unknowns");
        GTRY(dense_matrix(h, A));
        SLAM_HIP_TRY(hipMemcpyAsync(H, A, n * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if (b)
        SLAM_HIP_TRY(hipMemcpyAsync(b, h->b, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (blocks && h->E) {
        std::vector<double> t(42 * h->E);
        SLAM_HIP_TRY(hipMemcpyAsync(t.data(), h->blocks, t.size() * sizeof(double),
                                    hipMemcpyDeviceToHost, h->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        for (int64_t e = 0; e < h->E; ++e)
            for (int q = 0; q < 42; ++q) blocks[42 * e + q] = t[q * h->E + e];
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_graph_get_bsr(slam_graph* h, int64_t* n_slots, int64_t* rows, int64_t* cols,
                       double* vals) {
    SLAM_ARG_CHECK(h && n_slots, "slam_graph_get_bsr: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    *n_slots = h->n_slots;
    if (rows)
        SLAM_HIP_TRY(hipMemcpyAsync(rows, h->srow, h->n_slots * sizeof(int64_t),
                                    hipMemcpyDeviceToHost, h->stream));
    if (cols)
        SLAM_HIP_TRY(hipMemcpyAsync(cols, h->scol, h->n_slots * sizeof(int64_t),
                                    hipMemcpyDeviceToHost, h->stream));
    if (vals)
        SLAM_HIP_TRY(hipMemcpyAsync(vals, h->val, 9 * h->n_slots * sizeof(double),
                                    hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_graph_get_delta(slam_graph* h, double* delta) {
    SLAM_ARG_CHECK(h && delta, "slam_graph_get_delta: bad arguments");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (h->nt)
        SLAM_HIP_TRY(hipMemcpyAsync(delta, h->delta, 3 * h->nt * sizeof(double),
                                    hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_graph_timing(slam_graph* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_graph_timing: NULL argument");
    for (int k = 0; k < 5; ++k) out[k] = h->last[k];
    return SLAM_OK;
}

int slam_graph_cond_info(slam_graph* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_graph_cond_info: NULL argument");
    for (int k = 0; k < 7; ++k) out[k] = h->cond_info[k];
    return SLAM_OK;
}

int slam_graph_gate_info(slam_graph* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_graph_gate_info: NULL argument");
    for (int k = 0; k < kGateInfo; ++k) out[k] = h->gate_info[k];
    return SLAM_OK;
}

int slam_graph_set_marginal_cols(slam_graph* h, int32_t cols) {
    SLAM_ARG_CHECK(h, "slam_graph_set_marginal_cols: NULL handle");
    bool known = cols == 0;
    for (int w : kMargWidths) known = known || cols == w;
    SLAM_ARG_CHECK(known, "slam_graph_set_marginal_cols: cols must be 0, 1, 2, 4 or 8");
    h->marg_cols = cols;
    return SLAM_OK;
}

int slam_graph_marginals(slam_graph* h, int64_t m, const int64_t* times, int32_t relinearize,
                         double* cov, double* info) {
    SLAM_ARG_CHECK(h && times && cov && info && m >= 1, "slam_graph_marginals: bad arguments");
    SLAM_ARG_CHECK(h->poses, "slam_graph_marginals: set the poses first");
    SLAM_ARG_CHECK(h->B == 0, "slam_graph_marginals: not on a handle with members");
    SLAM_ARG_CHECK(m <= (int64_t)1 << 20, "slam_graph_marginals: too many times");
    const int64_t M = 3 * m;
    const int cols = h->marg_cols ? h->marg_cols : kMargDefaultCols;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 6; ++k) info[k] = 0.0;
    info[5] = cols;
    if (h->E == 0 || 3 * h->nt <= 3) {                      // :469 (leng > 3), as do_update
        std::fill(cov, cov + M * M, nan);
        return SLAM_OK;
    }
    // times -> unknowns; distinct and all of the edge set, before any launch
    std::vector<int64_t> qidx((size_t)M);
    {
        std::vector<int64_t> ranks((size_t)m);
        for (int64_t a = 0; a < m; ++a) {
            const auto it = std::lower_bound(h->times_h.begin(), h->times_h.end(), times[a]);
            SLAM_ARG_CHECK(it != h->times_h.end() && *it == times[a],
                           "slam_graph_marginals: a time that is not among the edge set's times");
            ranks[a] = it - h->times_h.begin();
            for (int q = 0; q < 3; ++q) qidx[3 * a + q] = 3 * ranks[a] + q;
        }
        std::sort(ranks.begin(), ranks.end());
        SLAM_ARG_CHECK(std::adjacent_find(ranks.begin(), ranks.end()) == ranks.end(),
                       "slam_graph_marginals: times must be distinct");
    }
    SLAM_ARG_CHECK(relinearize || h->assembled,
                   "slam_graph_marginals: relinearize = 0 before any system was assembled");
    const int64_t n = 3 * h->nt;
    const bool dense = (h->cfg.solver == SLAM_GRAPH_DENSE) ||
                       (h->cfg.solver == SLAM_GRAPH_AUTO && n <= kGraphDenseMax);
    SLAM_ARG_CHECK(!dense || n <= kGraphDenseMax,
                   "slam_graph_marginals: dense solver limited to 2048 unknowns");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    MargBuffers mb{};
    GTRY(marg_buffers(h, M, !dense, cols, &mb));
    hipStream_t s = h->stream;
    SLAM_HIP_TRY(hipEventRecord(h->marg_ev[0], s));
    if (relinearize) {
        GTRY(launch_linearize(h));      // the handle's robust kind: the weighted H
        hipLaunchKernelGGL(graph_assemble_h_kernel, dim3(nblk(9 * h->n_slots)), dim3(256), 0, s,
                           h->n_slots, h->E, h->cptr, h->clist, h->blocks, h->cfg.anchor, h->val);
        hipLaunchKernelGGL(graph_assemble_b_kernel, dim3(nblk(3 * h->nt)), dim3(256), 0, s, h->nt,
                           h->E, h->bptr, h->blist, h->blocks, h->b);
        SLAM_HIP_TRY(hipGetLastError());
        h->assembled = true;
    }
    SLAM_HIP_TRY(hipMemcpyAsync(mb.qidx, qidx.data(), M * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (dense) GTRY(marg_dense(h, mb, M, info));
    else GTRY(marg_pcg(h, mb, M, cols, info));
    SLAM_HIP_TRY(hipEventRecord(h->marg_ev[1], s));
    if (info[0] != 0.0)
        SLAM_HIP_TRY(hipMemcpyAsync(cov, mb.cov, M * M * sizeof(double), hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));      // qidx (host) is read by the upload until here
    if (info[0] == 0.0) std::fill(cov, cov + M * M, nan);
    float ms = 0.f;
    SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->marg_ev[0], h->marg_ev[1]));
    info[4] = ms;
    if (dense) info[5] = (double)M;
    return SLAM_OK;
}

int slam_graph_set_robust(slam_graph* h, int32_t kind, double param) {
    SLAM_ARG_CHECK(h, "slam_graph_set_robust: NULL handle");
    SLAM_ARG_CHECK(kind == SLAM_GRAPH_ROBUST_NONE || kind == SLAM_GRAPH_ROBUST_HUBER ||
                       kind == SLAM_GRAPH_ROBUST_CAUCHY || kind == SLAM_GRAPH_ROBUST_DCS,
                   "slam_graph_set_robust: unknown kind");
    SLAM_ARG_CHECK(std::isfinite(param), "slam_graph_set_robust: the parameter is not finite");
    SLAM_ARG_CHECK(kind == SLAM_GRAPH_ROBUST_NONE || param > 0.0,
                   "slam_graph_set_robust: the parameter of huber, cauchy and dcs must be > 0");
    h->robust_kind = kind;
    h->robust_param = param;
    return SLAM_OK;
}

int slam_graph_set_precond(slam_graph* h, int32_t kind, int32_t segment) {
    SLAM_ARG_CHECK(h, "slam_graph_set_precond: NULL handle");
    SLAM_ARG_CHECK(kind == SLAM_GRAPH_PRECOND_BLOCK_JACOBI || kind == SLAM_GRAPH_PRECOND_CHAIN,
                   "slam_graph_set_precond: unknown kind");
    if (kind == SLAM_GRAPH_PRECOND_CHAIN) {
        if (segment == 0) segment = kChainPoses;
        SLAM_ARG_CHECK(segment >= 1 && segment <= kChainPoses && (segment & (segment - 1)) == 0,
                       "slam_graph_set_precond: segment must be 0, 1, 2, 4, 8, 16, 32 or 64");
        h->precond_seg = segment;
    }
    h->precond_kind = kind;
    return SLAM_OK;
}

int slam_graph_precond_info(slam_graph* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_graph_precond_info: NULL argument");
    out[0] = h->pc_kind;
    out[1] = h->pc_seg;
    out[2] = out[3] = 0.0;
    if (h->pc_kind == SLAM_GRAPH_PRECOND_CHAIN && h->pc_ready && h->assembled) {
        SLAM_HIP_TRY(hipSetDevice(h->device));
        int32_t cnt[2];
        SLAM_HIP_TRY(hipMemcpyAsync(cnt, h->pc_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        out[2] = cnt[0];
        out[3] = cnt[1];
    }
    return SLAM_OK;
}

int slam_graph_apply_precond(slam_graph* h, const double* r, double* z) {
    SLAM_ARG_CHECK(h && r && z, "slam_graph_apply_precond: NULL argument");
    SLAM_ARG_CHECK(h->B == 0, "slam_graph_apply_precond: not on a handle with members");
    SLAM_ARG_CHECK(h->assembled && h->nt > 0,
                   "slam_graph_apply_precond: no system assembled since slam_graph_set_edges");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const int64_t n = 3 * h->nt;
    const unsigned nb = nblk(n, kPcgThreads);
    hipStream_t s = h->stream;
    if (!h->pc_ready) GTRY(precond_factor(h));
    // the PCG's own r and z are scratch between solves
    SLAM_HIP_TRY(hipMemcpyAsync(h->r, r, n * sizeof(double), hipMemcpyHostToDevice, s));
    if (h->pc_kind == SLAM_GRAPH_PRECOND_CHAIN)
        hipLaunchKernelGGL(graph_precond_apply_kernel<true>, dim3(nb), dim3(kPcgThreads), 0, s, n,
                           h->minv, h->fac, h->pc_seg, h->r, h->z);
    else
        hipLaunchKernelGGL(graph_precond_apply_kernel<false>, dim3(nb), dim3(kPcgThreads), 0, s, n,
                           h->minv, h->fac, h->pc_seg, h->r, h->z);
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipMemcpyAsync(z, h->z, n * sizeof(double), hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));
    return SLAM_OK;
}

int slam_graph_chi2(slam_graph* h, double* totals, double* chi2, double* weight) {
    SLAM_ARG_CHECK(h && totals, "slam_graph_chi2: NULL handle or totals");
    for (int k = 0; k < 4; ++k) totals[k] = 0.0;
    if (h->E == 0) return SLAM_OK;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    GTRY(robust_reserve(h));
    const RobustRows r = robust_rows(h);
    GTRY(launch_chi2(h, r.eval));
    hipStream_t s = h->stream;
    const size_t row = (size_t)h->E * sizeof(double);
    SLAM_HIP_TRY(hipMemcpyAsync(totals, r.tot, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (chi2) SLAM_HIP_TRY(hipMemcpyAsync(chi2, r.eval, row, hipMemcpyDeviceToHost, s));
    if (weight) SLAM_HIP_TRY(hipMemcpyAsync(weight, r.eval + h->E, row, hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));
    return SLAM_OK;
}

int slam_graph_get_edge_weights(slam_graph* h, double* chi2, double* weight) {
    SLAM_ARG_CHECK(h, "slam_graph_get_edge_weights: NULL handle");
    SLAM_ARG_CHECK(h->lin_kind >= 0,
                   "slam_graph_get_edge_weights: nothing linearised since slam_graph_set_edges");
    SLAM_ARG_CHECK(h->lin_kind != SLAM_GRAPH_ROBUST_NONE,
                   "slam_graph_get_edge_weights: the last linearisation ran with kind none and "
                   "stored no rows (every weight was 1; slam_graph_chi2 evaluates chi2)");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const RobustRows r = robust_rows(h);
    hipStream_t s = h->stream;
    const size_t row = (size_t)h->E * sizeof(double);
    if (chi2) SLAM_HIP_TRY(hipMemcpyAsync(chi2, r.lin, row, hipMemcpyDeviceToHost, s));
    if (weight) SLAM_HIP_TRY(hipMemcpyAsync(weight, r.lin + h->E, row, hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));
    return SLAM_OK;
}

int slam_graph_set_observations(slam_graph* h, int64_t n_halves, const slam_graph_half* halves,
                                int64_t n_landmarks) {
    SLAM_ARG_CHECK(h, "slam_graph_set_observations: NULL handle");
    SLAM_ARG_CHECK(n_halves >= 0 && n_landmarks >= 0, "slam_graph_set_observations: negative count");
    SLAM_ARG_CHECK(halves || n_halves == 0,
                   "slam_graph_set_observations: NULL array with a positive count");
    SLAM_ARG_CHECK(h->poses, "slam_graph_set_observations: set the poses first");
    SLAM_ARG_CHECK(h->B == 0, "slam_graph_set_observations: the handle has members (no map of members)");
    for (int64_t q = 0; q < n_halves; ++q) {
        const slam_graph_half& d = halves[q];
        SLAM_ARG_CHECK(d.pose >= 0 && d.pose < h->T,
                       "slam_graph_set_observations: pose index out of range");
        SLAM_ARG_CHECK(std::isfinite(d.obs[0]) && std::isfinite(d.obs[1]) && std::isfinite(d.obs[2]),
                       "slam_graph_set_observations: observation is not finite");
        SLAM_ARG_CHECK(d.obs[0] > 0.0, "slam_graph_set_observations: distance must be > 0");
    }
    h->map_set = false;
    if (n_halves == 0) return SLAM_OK;
    // stable grouping by landmark id (counting sort), as slam_graph_pair_halves
    // groups; each landmark's run cut into chunks counted from its first half-edge
    const int64_t NL = n_landmarks;
    std::vector<int64_t> lstart(NL + 1, 0), coff(NL + 1, 0);
    for (int64_t q = 0; q < n_halves; ++q) {
        const int64_t l = halves[q].landmark;
        if (l >= 0 && l < NL) lstart[l + 1]++;
    }
    h->map_count.assign(lstart.begin() + 1, lstart.end());
    for (int64_t l = 0; l < NL; ++l) {
        coff[l + 1] = coff[l] + (lstart[l + 1] + kMapChunk - 1) / kMapChunk;
        lstart[l + 1] += lstart[l];
    }
    const int64_t G = lstart[NL], NC = coff[NL];
    std::vector<int64_t> gpose(G), gsrc(G), clm(NC), cfirst(NC);
    std::vector<double> gobs(2 * G);
    {
        std::vector<int64_t> fill(lstart.begin(), lstart.end() - 1);
        for (int64_t q = 0; q < n_halves; ++q) {
            const int64_t l = halves[q].landmark;
            if (l < 0 || l >= NL) continue;
            const int64_t k = fill[l]++;
            gpose[k] = halves[q].pose;
            gsrc[k] = q;
            gobs[k] = halves[q].obs[0];
            gobs[G + k] = halves[q].obs[1];
        }
    }
    for (int64_t l = 0; l < NL; ++l)
        for (int64_t c = coff[l]; c < coff[l + 1]; ++c) {
            clm[c] = l;
            cfirst[c] = lstart[l] + (c - coff[l]) * kMapChunk;
        }
    const std::vector<double> nan_half(n_halves, std::numeric_limits<double>::quiet_NaN());
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (!h->map_ev[0])
        for (auto& e : h->map_ev) GTRY(h->map.event(&e));
    auto carve = [&](char* base) {
        Carver cv{base};
        h->map_gpose = cv.take<int64_t>(G);
        h->map_gsrc = cv.take<int64_t>(G);
        h->map_lstart = cv.take<int64_t>(NL + 1);
        h->map_coff = cv.take<int64_t>(NL + 1);
        h->map_clm = cv.take<int64_t>(NC);
        h->map_cfirst = cv.take<int64_t>(NC);
        h->map_gobs = cv.take<double>(2 * G);
        h->map_term = cv.take<double>(kMapTerms * G);
        h->map_part = cv.take<double>(kMapSums * NC);
        h->map_mean = cv.take<double>(2 * NL);
        h->map_cov = cv.take<double>(4 * NL);
        h->map_chi2 = cv.take<double>(NL);
        h->map_half = cv.take<double>(n_halves);
        return cv.off;
    };
    const size_t need = carve(nullptr);
    if (need > h->map_bytes) {
        h->map.release(h->map_arena);
        h->map_bytes = 0;
        GTRY(h->map.alloc(&h->map_arena, need + need / 4));
        h->map_bytes = need + need / 4;
    }
    carve(h->map_arena);
    GTRY(upload(h, h->map_gpose, gpose));
    GTRY(upload(h, h->map_gsrc, gsrc));
    GTRY(upload(h, h->map_lstart, lstart));
    GTRY(upload(h, h->map_coff, coff));
    GTRY(upload(h, h->map_clm, clm));
    GTRY(upload(h, h->map_cfirst, cfirst));
    GTRY(upload(h, h->map_gobs, gobs));
    GTRY(upload(h, h->map_half, nan_half));    // the ignored half-edges keep this NaN
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    h->map_n = n_halves;
    h->map_G = G;
    h->map_NL = NL;
    h->map_NC = NC;
    h->map_set = true;
    return SLAM_OK;
}

int slam_graph_landmarks(slam_graph* h, double* mean, double* cov, int64_t* count, double* chi2,
                         double* half_chi2) {
    SLAM_ARG_CHECK(h, "slam_graph_landmarks: NULL handle");
    SLAM_ARG_CHECK(h->map_set, "slam_graph_landmarks: no observations (slam_graph_set_observations)");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int64_t G = h->map_G, NL = h->map_NL, NC = h->map_NC;
    const bool want_chi2 = chi2 || half_chi2;
    int launches = 0;
    SLAM_HIP_TRY(hipEventRecord(h->map_ev[0], s));
    if (G) {
        hipLaunchKernelGGL(graph_map_contrib_kernel, dim3(nblk(G)), dim3(256), 0, s, G, h->map_gpose,
                           h->map_gobs, h->poses, gconst(h->cfg), h->map_term);
        ++launches;
    }
    SLAM_HIP_TRY(hipEventRecord(h->map_ev[1], s));
    if (G) {
        hipLaunchKernelGGL(graph_map_fold_kernel<false>, dim3((unsigned)NC), dim3(kMapChunk), 0, s, G,
                           NC, h->map_clm, h->map_cfirst, h->map_lstart, h->map_term, h->map_mean,
                           h->map_gsrc, h->map_part, h->map_half);
        ++launches;
    }
    SLAM_HIP_TRY(hipEventRecord(h->map_ev[2], s));
    if (NL) {
        hipLaunchKernelGGL(graph_map_finish_kernel<false>, dim3(nblk(NL, 64)), dim3(64), 0, s, NL, G, NC,
                           h->map_coff, h->map_lstart, h->map_part, h->map_term, h->map_mean,
                           h->map_cov, h->map_chi2);
        ++launches;
    }
    SLAM_HIP_TRY(hipEventRecord(h->map_ev[3], s));
    if (want_chi2 && G) {
        hipLaunchKernelGGL(graph_map_fold_kernel<true>, dim3((unsigned)NC), dim3(kMapChunk), 0, s, G,
                           NC, h->map_clm, h->map_cfirst, h->map_lstart, h->map_term, h->map_mean,
                           h->map_gsrc, h->map_part, h->map_half);
        ++launches;
    }
    SLAM_HIP_TRY(hipEventRecord(h->map_ev[4], s));
    if (want_chi2 && NL) {
        hipLaunchKernelGGL(graph_map_finish_kernel<true>, dim3(nblk(NL, 64)), dim3(64), 0, s, NL, G, NC,
                           h->map_coff, h->map_lstart, h->map_part, h->map_term, h->map_mean,
                           h->map_cov, h->map_chi2);
        ++launches;
    }
    SLAM_HIP_TRY(hipEventRecord(h->map_ev[5], s));
    SLAM_HIP_TRY(hipGetLastError());
    const size_t d = sizeof(double);
    if (mean && NL) SLAM_HIP_TRY(hipMemcpyAsync(mean, h->map_mean, 2 * NL * d, hipMemcpyDeviceToHost, s));
    if (cov && NL) SLAM_HIP_TRY(hipMemcpyAsync(cov, h->map_cov, 4 * NL * d, hipMemcpyDeviceToHost, s));
    if (chi2 && NL) SLAM_HIP_TRY(hipMemcpyAsync(chi2, h->map_chi2, NL * d, hipMemcpyDeviceToHost, s));
    if (half_chi2)
        SLAM_HIP_TRY(hipMemcpyAsync(half_chi2, h->map_half, h->map_n * d, hipMemcpyDeviceToHost, s));
    SLAM_HIP_TRY(hipStreamSynchronize(s));
    if (count) std::copy(h->map_count.begin(), h->map_count.end(), count);
    double total = 0.0;
    for (int k = 0; k < 5; ++k) {
        float ms = 0.f;
        SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->map_ev[k], h->map_ev[k + 1]));
        h->map_ms[k] = ms;
        total += ms;
    }
    h->map_last[0] = total;
    h->map_last[1] = launches;
    return SLAM_OK;
}

int slam_graph_map_timing(slam_graph* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_graph_map_timing: NULL argument");
    out[0] = h->map_last[0];
    out[1] = h->map_last[1];
    return SLAM_OK;
}

int slam_graph_map_kernel_timing(slam_graph* h, double* out) {
    SLAM_ARG_CHECK(h && out, "slam_graph_map_kernel_timing: NULL argument");
    for (int k = 0; k < 5; ++k) out[k] = h->map_ms[k];
    return SLAM_OK;
}

int slam_graph_pair_halves(int64_t n_halves, const slam_graph_half* halves, int64_t n_landmarks,
                           int device, int64_t* n_edges, slam_graph_edge* edges) {
    SLAM_ARG_CHECK(n_edges && n_halves >= 0 && n_landmarks >= 0 && (halves || n_halves == 0),
                   "slam_graph_pair_halves: bad arguments");
    // stable grouping by landmark id (counting sort), pair offsets per landmark
    std::vector<int64_t> lm_start(n_landmarks + 1, 0);
    for (int64_t q = 0; q < n_halves; ++q) {
        const int64_t l = halves[q].landmark;
        if (l >= 0 && l < n_landmarks) lm_start[l + 1]++;
    }
    std::vector<int64_t> pair_off(n_landmarks + 1, 0);
    for (int64_t l = 0; l < n_landmarks; ++l) {
        const int64_t m = lm_start[l + 1];
        pair_off[l + 1] = pair_off[l] + m * (m - 1) / 2;
        lm_start[l + 1] += lm_start[l];
    }
    const int64_t E = pair_off[n_landmarks];
    *n_edges = E;
    if (!edges || E == 0) return SLAM_OK;
    std::vector<slam_graph_half> grouped(lm_start[n_landmarks]);
    {
        std::vector<int64_t> fill(lm_start.begin(), lm_start.end() - 1);
        for (int64_t q = 0; q < n_halves; ++q) {
            const int64_t l = halves[q].landmark;
            if (l >= 0 && l < n_landmarks) grouped[fill[l]++] = halves[q];
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(SLAM_ERR_ARG, "slam_graph_pair_halves: no such HIP device");
    SLAM_HIP_TRY(hipSetDevice(device));
    int64_t *d_off = nullptr, *d_start = nullptr;
    slam_graph_half* d_half = nullptr;
    slam_graph_edge* d_edges = nullptr;
    DeviceMem mem;
    if (mem.alloc(&d_off, pair_off.size()) || mem.alloc(&d_start, lm_start.size()) ||
        mem.alloc(&d_half, grouped.size()) || mem.alloc(&d_edges, (size_t)E))
        return fail(SLAM_ERR_HIP, "slam_graph_pair_halves: device allocation failed");
    if (hipMemcpy(d_off, pair_off.data(), pair_off.size() * sizeof(int64_t), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(d_start, lm_start.data(), lm_start.size() * sizeof(int64_t), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(d_half, grouped.data(), grouped.size() * sizeof(slam_graph_half),
                  hipMemcpyHostToDevice) != hipSuccess)
        return fail(SLAM_ERR_HIP, "slam_graph_pair_halves: upload failed");
    hipLaunchKernelGGL(graph_pair_kernel, dim3(nblk(E)), dim3(256), 0, nullptr, E, n_landmarks, d_off,
                       d_start, d_half, d_edges);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(edges, d_edges, (size_t)E * sizeof(slam_graph_edge), hipMemcpyDeviceToHost) !=
            hipSuccess)
        return fail(SLAM_ERR_HIP, "slam_graph_pair_halves: kernel or download failed");
    return SLAM_OK;
}

int slam_graph_linearize_solve(const slam_graph_config* cfg, const slam_graph_edge* edges,
                               int64_t n_edges, double* poses, int64_t n_poses, double* stats,
                               int device) {
    SLAM_ARG_CHECK(poses && stats, "slam_graph_linearize_solve: NULL argument");
    slam_graph* h = nullptr;
    int rc = slam_graph_create(cfg, device, &h);
    if (rc) return rc;
    rc = slam_graph_set_poses(h, n_poses, poses);
    if (!rc) rc = slam_graph_set_edges(h, n_edges, edges);
    if (!rc) rc = slam_graph_update(h, stats);
    if (!rc) rc = slam_graph_get_poses(h, poses);
    slam_graph_destroy(h);
    return rc;
}

}  // extern "C"
