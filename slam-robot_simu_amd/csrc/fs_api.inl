// fs_api.inl -- C-ABI of FastSLAM 1.0, with known data association or with
// per-particle maximum-likelihood association, and of FastSLAM 2.0's proposal
// handles, with known ids or associating (include/slam_hip.h, slam_fs_*).  Included by pf_api.hip, as
// pf_dist_api.inl is: the poses, weights, exact cumsum, systematic resampling,
// predict and step end are the single handle's own (a slam_pf with zero
// landmarks); this file adds the per-particle maps, their update with its log
// weights, and their resampling gather (fastslam.inl), and the optional landmark
// evidence pass (fs_prune.hip).
#include "fastslam.inl"
#include "fs_prune.hpp"

struct slam_fs {
    slam_fs_config cfg;
    slam_pf* pf = nullptr;                 // the inner filter: destroyed with this handle
    DeviceMem mem;                         // everything else below
    int64_t n = 0, npad = 0;
    int32_t nl = 0;
    double* map[2] = {nullptr, nullptr};   // ping-pong halves, [NL][5][npad]
    int mcur = 0;
    double* L = nullptr;                   // [n] log weights of the step
    double* bmax = nullptr;                // [nb] block maxima, then the grid maximum at [nb]
    int32_t nb = 0;
    int32_t* seen_dev = nullptr;           // [NL]
    int32_t* list_dev = nullptr;           // [NL] the seen landmarks (gather)
    FsObs* obs_dev = nullptr;              // the staged step, or the loaded run
    int64_t obs_cap = 0;
    double* stage = nullptr;               // get / set maps staging
    int64_t stage_cap = 0;                 // doubles
    std::vector<int32_t> seen;             // host mirror
    std::vector<int32_t> list;
    std::vector<FsObs> obs_host;
    std::vector<int64_t> run_off;          // loaded run: record offsets per step, [steps + 1]
    hipEvent_t ev[4][2] = {};
    bool ran[4] = {false, false, false, false};
    // per-particle association (slam_fs_create_assoc); nl is then the capacity
    bool assoc = false;
    slam_fs_assoc_config acfg = {};
    int32_t* cnt[2] = {nullptr, nullptr};  // ping-pong halves of the counts, [npad]
    int ccur = 0;
    int32_t* stamp = nullptr;              // [cap][npad] update call that last matched the slot
    int32_t call = 0;                      // number of the last update call
    int32_t* bcnt = nullptr;               // [nb] block maxima of the counts
    int32_t* cmax_pin = nullptr;           // pinned, coherent: max cnt after the last update
    int32_t* cmax_pin_dev = nullptr;
    int32_t cmax = 0;                      // host bound on max cnt (exact after an update)
    int32_t* assoc_dev = nullptr;          // [assoc_cap][npad] the last update's choices
    int64_t assoc_cap = 0;
    int32_t assoc_k = 0;
    // FastSLAM 2.0 proposal (slam_fs_create_proposal)
    bool prop = false;
    slam_fs_proposal_config pcfg = {};
    FsPropQ propq = {};                    // Q = F^T F of cfg.pf.q_factor
    double* prop_rec = nullptr;            // [9][npad] mean and covariance before sampling (record)
    bool prop_ran = false;                 // a step has filled prop_rec and L
    // landmark evidence and removal (slam_fs_set_pruning); buffers from the first turning on
    bool prune = false;
    slam_fs_prune_config prcfg = {};
    int32_t* evd[2] = {nullptr, nullptr};  // ping-pong halves of the evidence, [cap][npad]
    int ecur = 0;
    int32_t* cnt0 = nullptr;               // [npad] the counts ahead of the update
    int32_t* removed = nullptr;            // [npad] the last pass's removals
};

namespace {

// One step's observation list against the argument rules (host only)
int fs_check_list(int32_t nl, const char* who, int32_t k, const int64_t* ids, const double* obs) {
    if (k < 0 || k > nl) return fail(SLAM_ERR_ARG, std::string(who) + ": need 0 <= k <= n_landmarks");
    if (k > 0 && (!ids || !obs)) return fail(SLAM_ERR_ARG, std::string(who) + ": NULL ids / obs");
    for (int32_t t = 0; t < k; ++t) {
        if (ids[t] < 0 || ids[t] >= nl)
            return fail(SLAM_ERR_ARG, std::string(who) + ": landmark id out of range");
        const double d = obs[3 * t], phi = obs[3 * t + 1], psi = obs[3 * t + 2];
        if (!(std::isfinite(d) && std::isfinite(phi) && std::isfinite(psi)))
            return fail(SLAM_ERR_ARG, std::string(who) + ": non-finite observation");
        if (!(d > 0.0)) return fail(SLAM_ERR_ARG, std::string(who) + ": observed range d <= 0");
    }
    std::vector<int64_t> s(ids, ids + k);
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end())
        return fail(SLAM_ERR_ARG, std::string(who) + ": duplicate landmark id within one step");
    return SLAM_OK;
}

// An associating handle's list: no ids, k bounded by SLAM_FS_ASSOC_MAX_OBS
int fs_check_list_assoc(const char* who, int32_t k, const int64_t* ids, const double* obs) {
    if (ids) return fail(SLAM_ERR_ARG, std::string(who) + ": ids must be NULL on an associating handle");
    if (k < 0 || k > SLAM_FS_ASSOC_MAX_OBS)
        return fail(SLAM_ERR_ARG, std::string(who) + ": need 0 <= k <= SLAM_FS_ASSOC_MAX_OBS");
    if (k > 0 && !obs) return fail(SLAM_ERR_ARG, std::string(who) + ": NULL obs");
    for (int32_t t = 0; t < k; ++t) {
        const double d = obs[3 * t], phi = obs[3 * t + 1], psi = obs[3 * t + 2];
        if (!(std::isfinite(d) && std::isfinite(phi) && std::isfinite(psi)))
            return fail(SLAM_ERR_ARG, std::string(who) + ": non-finite observation");
        if (!(d > 0.0)) return fail(SLAM_ERR_ARG, std::string(who) + ": observed range d <= 0");
    }
    return SLAM_OK;
}

int fs_check_obs(slam_fs* f, const char* who, int32_t k, const int64_t* ids, const double* obs) {
    if (f->assoc) return fs_check_list_assoc(who, k, ids, obs);
    return fs_check_list(f->nl, who, k, ids, obs);
}

// the particle-independent terms of one observation (scan_cov with the observed range)
FsObs fs_make_obs(const slam_fs* f, int64_t id, const double* o) {
    FsObs r;
    r.d = o[0];
    r.phi = o[1];
    r.psi = o[2];
    const double a = r.d * f->cfg.r_dist, b = r.d * std::sin(f->cfg.r_dir);
    r.r0 = a * a;
    r.r1 = b * b;
    r.rx = r.d * std::cos(r.phi);
    r.ry = r.d * std::sin(r.phi);
    r.vo = f->cfg.r_dir * f->cfg.r_dir + f->cfg.r_orient * f->cfg.r_orient;
    r.id = id;
    return r;
}

// grow-only buffer of the handle: release, allocate, then the capacity
template <typename T>
int fs_reserve(slam_fs* f, T*& p, int64_t& cap, int64_t want, size_t count) {
    if (want <= cap) return SLAM_OK;
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    f->mem.release(p);
    cap = 0;
    const int rc = f->mem.alloc(&p, count);
    if (rc) return rc;
    cap = want;
    return SLAM_OK;
}
int fs_reserve_obs(slam_fs* f, int64_t count) {
    return fs_reserve(f, f->obs_dev, f->obs_cap, count, (size_t)count);
}
int fs_reserve_assoc(slam_fs* f, int64_t k) {
    return fs_reserve(f, f->assoc_dev, f->assoc_cap, k, (size_t)k * (size_t)f->npad);
}
int fs_reserve_stage(slam_fs* f, int64_t doubles) {
    return fs_reserve(f, f->stage, f->stage_cap, doubles, (size_t)doubles);
}

void fs_tic(slam_fs* f, int k) {
    (void)hipEventRecord(f->ev[k][0], f->pf->stream);
    f->ran[k] = true;
}
void fs_toc(slam_fs* f, int k) { (void)hipEventRecord(f->ev[k][1], f->pf->stream); }

inline dim3 fs_grid(int64_t n, int64_t rows) {
    return dim3(grid_for(n, kFsThreads), (unsigned)std::max<int64_t>(1, std::min<int64_t>(rows, 65535)));
}

// __resampling (particle_filter.py:200-224) as slam_pf_resample enqueues it,
// then the maps of the seen landmarks through the same indices.  The clamp's
// status bit stays in the flags: the step end's record carries it (a
// stand-alone slam_fs_resample reads and clears it itself).
int fs_enqueue_resample(slam_fs* f, double u) {
    slam_pf* h = f->pf;
    int rc = stage_scan_offset(h, u);
    if (rc || (rc = launch_scans(h, 1, true)) || (rc = retire_scan_marks(h))) return rc;
    const double ofs = std::isnan(u) ? u : u * h->pc.np_recip;
    resample_search_kernel<<<grid_for(h->n, 256), 256, 0, h->stream>>>(
        h->n, h->c, h->idx, h->pc.rstep, ofs, h->pc.np_recip, h->cfg.seed, h->stepno, h->flags);
    const int src = h->cur, dst = 1 - h->cur;
    gather_kernel<<<grid_for(h->n, 256), 256, 0, h->stream>>>(
        h->n, h->idx, h->x[src], h->y[src], h->th[src], h->x[dst], h->y[dst], h->th[dst], h->w_un,
        h->pc.np_recip);
    SLAM_HIP_TRY(hipGetLastError());
    if ((rc = set_s_one(h))) return rc;
    h->cur = dst;
    if (f->assoc) {
        // the counts with the poses, and every row below a particle's own count
        fs_tic(f, 0);
        fs_assoc_gather_kernel<<<fs_grid(f->n, f->cmax), kFsThreads, 0, h->stream>>>(
            f->n, f->npad, h->idx, f->cmax, f->map[f->mcur], f->map[1 - f->mcur], f->cnt[f->ccur],
            f->cnt[1 - f->ccur]);
        if (f->prune) {
            // the evidence rows with the maps, by the source's counts
            fs_prune_gather_launch(h->stream, fs_grid(f->n, f->cmax), f->n, f->npad, h->idx, f->cmax,
                                   f->cnt[f->ccur], f->evd[f->ecur], f->evd[1 - f->ecur]);
            f->ecur = 1 - f->ecur;
        }
        SLAM_HIP_TRY(hipGetLastError());
        f->mcur = 1 - f->mcur;
        f->ccur = 1 - f->ccur;
        fs_toc(f, 0);
        h->resample_next = 0;
        return set_flag(h, kFlagResample, 0);
    }
    f->list.clear();
    for (int32_t j = 0; j < f->nl; ++j)
        if (f->seen[(size_t)j]) f->list.push_back(j);
    fs_tic(f, 0);
    if (!f->list.empty()) {
        SLAM_HIP_TRY(hipMemcpyAsync(f->list_dev, f->list.data(), f->list.size() * sizeof(int32_t),
                                    hipMemcpyHostToDevice, h->stream));
        fs_map_gather_kernel<<<fs_grid(f->n, (int64_t)f->list.size()), kFsThreads, 0, h->stream>>>(
            f->n, f->npad, h->idx, f->list_dev, (int32_t)f->list.size(), f->map[f->mcur],
            f->map[1 - f->mcur]);
        SLAM_HIP_TRY(hipGetLastError());
        f->mcur = 1 - f->mcur;
    }
    fs_toc(f, 0);
    h->resample_next = 0;
    return set_flag(h, kFlagResample, 0);
}

// A pruning handle: the counts as they stand ahead of the map update (the
// update kernels overwrite them in place; the pass needs cnt0 -- DESIGN 11f)
int fs_prune_note_counts(slam_fs* f) {
    if (!f->prune) return SLAM_OK;
    SLAM_HIP_TRY(hipMemcpyAsync(f->cnt0, f->cnt[f->ccur], sizeof(int32_t) * (size_t)f->npad,
                                hipMemcpyDeviceToDevice, f->pf->stream));
    return SLAM_OK;
}

// The evidence pass after the map update, then the largest count to the host's
// coherent word.  call: the update's number, -1 where no update ran (k = 0 on
// an "ml" handle: no stamp equals it).
int fs_enqueue_prune(slam_fs* f, int32_t call) {
    slam_pf* h = f->pf;
    const slam_fs_prune_config& pc = f->prcfg;
    const FsPrune P{pc.view_range * pc.view_range, pc.view_tan, pc.init, pc.hit, pc.miss,
                    pc.ev_max, pc.remove_below};
    const int c = h->cur;
    fs_prune_launch(h->stream, pc.use_angle != 0, f->nb, f->n, f->npad, h->x[c], h->y[c], h->th[c],
                    f->map[f->mcur], f->cnt[f->ccur], f->cnt0, f->stamp, call, f->nl, P,
                    f->evd[f->ecur], f->removed, f->bcnt, f->cmax_pin_dev);
    SLAM_HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// __predict (particle_filter.py:156-168): the single handle's fused launch
// with zero landmarks -- the weights pass through (w_un = w, s = 1)
int fs_enqueue_predict(slam_fs* f, const double* control, const double* noise) {
    slam_pf* h = f->pf;
    int rc;
    if ((rc = stage_inputs(h, control, nullptr, noise, std::nan("")))) return rc;
    if ((rc = set_flag(h, kFlagResample, 0))) return rc;
    fs_tic(f, 1);
    rc = launch_fused(h, h->cfg.motion, noise != nullptr);
    fs_toc(f, 1);
    if (rc || (rc = set_s_one(h))) return rc;
    h->stepno++;
    return SLAM_OK;
}

// A proposal handle's predict and map update in one launch (fs_proposal_kernel):
// the noise-free motion, the proposal over the step's k records, the sampled
// pose and the maps at it.  The counters move as in fs_enqueue_predict; the
// weights and the step end follow in fs_enqueue_update.
int fs_enqueue_proposal(slam_fs* f, const double* control, int32_t k, const FsObs* obs,
                        const double* noise) {
    slam_pf* h = f->pf;
    int rc;
    if ((rc = stage_inputs(h, control, nullptr, noise, std::nan("")))) return rc;
    const int src = h->cur, dst = 1 - h->cur;
    fs_tic(f, 1);
#define SLAM_FS_PROPOSAL(HN)                                                                     \
    fs_proposal_kernel<HN><<<f->nb, kFsThreads, 0, h->stream>>>(                                 \
        f->n, f->npad, h->x[src], h->y[src], h->th[src], h->x[dst], h->y[dst], h->th[dst],       \
        h->w_un, h->s_cur, h->pc.np_recip, f->map[f->mcur], k, obs, f->seen_dev,                 \
        f->cfg.use_orient, h->pc.dt, control[0], control[1], f->propq, h->noise,                 \
        (uint32_t)h->stepno, h->cfg.seed, f->prop_rec, f->L, f->bmax)
    if (noise) SLAM_FS_PROPOSAL(true); else SLAM_FS_PROPOSAL(false);
#undef SLAM_FS_PROPOSAL
    fs_toc(f, 1);
    SLAM_HIP_TRY(hipGetLastError());
    h->cur = dst;
    f->prop_ran = true;
    if ((rc = set_s_one(h))) return rc;
    h->stepno++;
    return SLAM_OK;
}

// fs_enqueue_proposal on a handle that also associates (fs_assoc_proposal_kernel):
// the choices always go to memory -- the kernel's second pass reads them back.
int fs_enqueue_assoc_proposal(slam_fs* f, const double* control, int32_t k, const FsObs* obs,
                              const double* noise) {
    slam_pf* h = f->pf;
    int rc;
    if ((rc = fs_reserve_assoc(f, k))) return rc;
    if ((rc = stage_inputs(h, control, nullptr, noise, std::nan("")))) return rc;
    if ((rc = fs_prune_note_counts(f))) return rc;
    const int src = h->cur, dst = 1 - h->cur;
    ++f->call;
    fs_tic(f, 1);
#define SLAM_FS_ASSOC_PROPOSAL(HN)                                                               \
    fs_assoc_proposal_kernel<HN><<<f->nb, kFsThreads, 0, h->stream>>>(                           \
        f->n, f->npad, h->x[src], h->y[src], h->th[src], h->x[dst], h->y[dst], h->th[dst],       \
        h->w_un, h->s_cur, h->pc.np_recip, f->map[f->mcur], f->cnt[f->ccur], f->stamp, f->call,  \
        f->nl, k, obs, f->cfg.use_orient, h->pc.dt, control[0], control[1], f->propq,            \
        f->acfg.log_p_new, h->noise, (uint32_t)h->stepno, h->cfg.seed, f->assoc_dev,             \
        f->prop_rec, f->L, f->bmax, f->bcnt)
    if (noise) SLAM_FS_ASSOC_PROPOSAL(true); else SLAM_FS_ASSOC_PROPOSAL(false);
#undef SLAM_FS_ASSOC_PROPOSAL
    fs_toc(f, 1);
    SLAM_HIP_TRY(hipGetLastError());
    h->cur = dst;
    f->prop_ran = true;
    if ((rc = set_s_one(h))) return rc;
    h->stepno++;
    return SLAM_OK;
}

// the per-particle map update with its log weights, the weights, then the
// single handle's step end on the current particles (its update stage with
// zero landmarks: the block partials of the new w_un, then the finalize)
int fs_enqueue_update(slam_fs* f, int32_t k, const FsObs* obs, int32_t resampled) {
    slam_pf* h = f->pf;
    int rc;
    fs_tic(f, 2);
    if (!f->prop && (rc = fs_prune_note_counts(f))) return rc;     // a proposal launch took its own
    if (k > 0 && f->assoc && f->prop) {
        // the proposal launch left L, the counts and their block maxima, and updated the maps
        fs_assoc_fold_kernel<<<1, kFsThreads, 0, h->stream>>>(f->bmax, f->bcnt, f->nb, f->bmax + f->nb,
                                                             f->cmax_pin_dev);
        fs_weight_kernel<<<f->nb, kFsThreads, 0, h->stream>>>(f->n, f->L, f->bmax + f->nb, h->w_un);
        SLAM_HIP_TRY(hipGetLastError());
    } else if (k > 0 && f->assoc) {
        const int c = h->cur;
        int32_t* rec = nullptr;
        if (f->acfg.record) {
            if ((rc = fs_reserve_assoc(f, k))) return rc;
            rec = f->assoc_dev;
        }
        ++f->call;
        fs_assoc_update_kernel<<<f->nb, kFsThreads, 0, h->stream>>>(
            f->n, f->npad, h->x[c], h->y[c], h->th[c], f->map[f->mcur], f->cnt[f->ccur], f->stamp,
            f->call, f->nl, k, obs, f->cfg.use_orient, f->acfg.log_p_new, rec, f->L, f->bmax, f->bcnt);
        fs_assoc_fold_kernel<<<1, kFsThreads, 0, h->stream>>>(f->bmax, f->bcnt, f->nb, f->bmax + f->nb,
                                                             f->cmax_pin_dev);
        fs_weight_kernel<<<f->nb, kFsThreads, 0, h->stream>>>(f->n, f->L, f->bmax + f->nb, h->w_un);
        SLAM_HIP_TRY(hipGetLastError());
    } else if (k > 0 && f->prop) {
        // the proposal launch left L and its block maxima, and updated the maps
        fs_max_fold_kernel<<<1, kFsThreads, 0, h->stream>>>(f->bmax, f->nb, f->bmax + f->nb);
        fs_weight_kernel<<<f->nb, kFsThreads, 0, h->stream>>>(f->n, f->L, f->bmax + f->nb, h->w_un);
        fs_mark_seen_kernel<<<grid_for(k, kFsThreads), kFsThreads, 0, h->stream>>>(k, obs, f->seen_dev);
        SLAM_HIP_TRY(hipGetLastError());
    } else if (k > 0) {
        const int c = h->cur;
        fs_update_kernel<<<f->nb, kFsThreads, 0, h->stream>>>(
            f->n, f->npad, h->x[c], h->y[c], h->th[c], f->map[f->mcur], k, obs, f->seen_dev,
            f->cfg.use_orient, f->L, f->bmax);
        fs_max_fold_kernel<<<1, kFsThreads, 0, h->stream>>>(f->bmax, f->nb, f->bmax + f->nb);
        fs_weight_kernel<<<f->nb, kFsThreads, 0, h->stream>>>(f->n, f->L, f->bmax + f->nb, h->w_un);
        fs_mark_seen_kernel<<<grid_for(k, kFsThreads), kFsThreads, 0, h->stream>>>(k, obs, f->seen_dev);
        SLAM_HIP_TRY(hipGetLastError());
    }
    if (f->assoc) f->assoc_k = k;
    // an empty scan is evidence too: the pass runs whatever k is
    if (f->prune && (rc = fs_enqueue_prune(f, k > 0 || f->prop ? f->call : -1))) return rc;
    fs_toc(f, 2);
    static const double ctl0[2] = {0.0, 0.0};
    SLAM_HIP_TRY(hipMemcpyAsync(h->ctl, ctl0, 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = set_ctr(h, 0)) || (rc = set_flag(h, kFlagResample, 0))) return rc;
    fs_tic(f, 3);
    if ((rc = launch_fused(h, kMotionNone, false)) || (rc = launch_reduce(h, resampled))) return rc;
    fs_toc(f, 3);
    return SLAM_OK;
}

// after the step's host read.  An associating handle has no filter-wide
// "seen": it takes the largest count, which the fold stored beside the record.
void fs_note_seen(slam_fs* f, int32_t k, const FsObs* obs) {
    if (f->assoc) {
        if (k > 0 || f->prune) f->cmax = *f->cmax_pin;     // a pruning pass folds on every step
        return;
    }
    for (int32_t t = 0; t < k; ++t) f->seen[(size_t)obs[t].id] = 1;
}

// one whole step from k records already on the device (host copies in host_obs)
int fs_step_records(slam_fs* f, const double* control, int32_t k, const FsObs* dev_obs,
                    const FsObs* host_obs, const double* noise, double u, slam_pf_result* res) {
    slam_pf* h = f->pf;
    h->prep_step = -1;
    for (int q = 0; q < 4; ++q) f->ran[q] = false;
    const int32_t resampling = h->resample_next;
    int rc;
    if (resampling && (rc = fs_enqueue_resample(f, u))) return rc;
    if ((rc = f->prop && f->assoc ? fs_enqueue_assoc_proposal(f, control, k, dev_obs, noise)
              : f->prop         ? fs_enqueue_proposal(f, control, k, dev_obs, noise)
                                : fs_enqueue_predict(f, control, noise)))
        return rc;
    if ((rc = fs_enqueue_update(f, k, dev_obs, resampling))) return rc;
    if (f->assoc) {
        rc = sync_results(h, 0, 1, res);    // the step's one host read, the largest count with it
        fs_note_seen(f, k, host_obs);
        return rc;
    }
    fs_note_seen(f, k, host_obs);
    return sync_results(h, 0, 1, res);      // the step's one host read
}

int fs_stage_step_obs(slam_fs* f, int32_t k, const int64_t* ids, const double* obs) {
    f->obs_host.resize((size_t)k);
    for (int32_t t = 0; t < k; ++t)
        f->obs_host[(size_t)t] = fs_make_obs(f, ids ? ids[t] : -1, obs + 3 * t);
    f->run_off.clear();                     // the device records no longer hold a loaded run
    if (k == 0) return SLAM_OK;
    int rc = fs_reserve_obs(f, k);
    if (rc) return rc;
    SLAM_HIP_TRY(hipMemcpyAsync(f->obs_dev, f->obs_host.data(), sizeof(FsObs) * (size_t)k,
                                hipMemcpyHostToDevice, f->pf->stream));
    return SLAM_OK;
}

// maps between the host layout and the device's, a slab of particles at a time
constexpr int64_t kFsStageDoubles = int64_t(1) << 22;      // 32 MiB

int fs_maps_io(slam_fs* f, bool to_device, double* mean, double* cov) {
    slam_pf* h = f->pf;
    const int64_t per = 3 * (int64_t)f->nl;
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>(f->n, kFsStageDoubles / per));
    int rc = fs_reserve_stage(f, slab * per);
    if (rc) return rc;
    for (int pass = 0; pass < 2; ++pass) {
        double* host = pass == 0 ? mean : cov;
        if (!host) continue;
        const int32_t comp0 = pass == 0 ? 0 : 2, ncomp = pass == 0 ? 2 : 3;
        for (int64_t p0 = 0; p0 < f->n; p0 += slab) {
            const int64_t cnt = std::min<int64_t>(slab, f->n - p0);
            const size_t bytes = sizeof(double) * (size_t)cnt * f->nl * ncomp;
            double* hp = host + (size_t)p0 * f->nl * ncomp;
            if (to_device) {
                SLAM_HIP_TRY(hipMemcpyAsync(f->stage, hp, bytes, hipMemcpyHostToDevice, h->stream));
                // the slab's particles are rows p0.. of the staged array
                fs_map_unpack_kernel<<<fs_grid(cnt, f->nl), kFsThreads, 0, h->stream>>>(
                    cnt, f->npad, f->nl, comp0, ncomp, f->stage, f->map[f->mcur] + p0);
            } else {
                if (f->assoc)
                    fs_assoc_pack_kernel<<<fs_grid(cnt, f->nl), kFsThreads, 0, h->stream>>>(
                        f->n, f->npad, f->nl, p0, cnt, comp0, ncomp, f->cnt[f->ccur],
                        f->map[f->mcur], f->stage);
                else
                    fs_map_pack_kernel<<<fs_grid(cnt, f->nl), kFsThreads, 0, h->stream>>>(
                        f->n, f->npad, f->nl, p0, cnt, comp0, ncomp, f->seen_dev, f->map[f->mcur],
                        f->stage);
                SLAM_HIP_TRY(hipMemcpyAsync(hp, f->stage, bytes, hipMemcpyDeviceToHost, h->stream));
            }
            SLAM_HIP_TRY(hipGetLastError());
            SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return SLAM_OK;
}

int fs_create_impl(const slam_fs_config* cfg, const slam_fs_assoc_config* acfg,
                   const slam_fs_proposal_config* pcfg, int64_t n_particles, int32_t n_landmarks,
                   int device, slam_fs** out);

}  // namespace

extern "C" {

int slam_fs_check_observations(int32_t n_landmarks, int32_t k, const int64_t* ids, const double* obs) {
    SLAM_ARG_CHECK(n_landmarks >= 1, "slam_fs_check_observations: need n_landmarks >= 1");
    return fs_check_list(n_landmarks, "slam_fs_check_observations", k, ids, obs);
}

int slam_fs_create(const slam_fs_config* cfg, int64_t n_particles, int32_t n_landmarks, int device,
                   slam_fs** out) {
    return fs_create_impl(cfg, nullptr, nullptr, n_particles, n_landmarks, device, out);
}

int slam_fs_create_assoc(const slam_fs_config* cfg, const slam_fs_assoc_config* acfg,
                         int64_t n_particles, int32_t max_landmarks, int device, slam_fs** out) {
    SLAM_ARG_CHECK(cfg && acfg && out, "slam_fs_create_assoc: NULL argument");
    *out = nullptr;
    SLAM_ARG_CHECK(n_particles >= 1 && n_particles <= (int64_t(1) << 24),
                   "slam_fs_create_assoc: need 1 <= n_particles <= 2^24");
    SLAM_ARG_CHECK(max_landmarks >= 1, "slam_fs_create_assoc: need max_landmarks >= 1");
    SLAM_ARG_CHECK(std::isfinite(acfg->log_p_new), "slam_fs_create_assoc: non-finite log_p_new");
    return fs_create_impl(cfg, acfg, nullptr, n_particles, max_landmarks, device, out);
}

int slam_fs_create_proposal(const slam_fs_config* cfg, const slam_fs_proposal_config* pcfg,
                            int64_t n_particles, int32_t n_landmarks, int device, slam_fs** out) {
    SLAM_ARG_CHECK(cfg, "slam_fs_create_proposal: NULL cfg");
    SLAM_ARG_CHECK(pcfg, "slam_fs_create_proposal: NULL pcfg");
    SLAM_ARG_CHECK(out, "slam_fs_create_proposal: NULL out");
    *out = nullptr;
    SLAM_ARG_CHECK(cfg->pf.motion == SLAM_MOTION_LINEAR,
                   "slam_fs_create_proposal: pf.motion must be SLAM_MOTION_LINEAR");
    return fs_create_impl(cfg, nullptr, pcfg, n_particles, n_landmarks, device, out);
}

int slam_fs_create_assoc_proposal(const slam_fs_config* cfg, const slam_fs_assoc_config* acfg,
                                  const slam_fs_proposal_config* pcfg, int64_t n_particles,
                                  int32_t max_landmarks, int device, slam_fs** out) {
    SLAM_ARG_CHECK(cfg, "slam_fs_create_assoc_proposal: NULL cfg");
    SLAM_ARG_CHECK(acfg, "slam_fs_create_assoc_proposal: NULL acfg");
    SLAM_ARG_CHECK(pcfg, "slam_fs_create_assoc_proposal: NULL pcfg");
    SLAM_ARG_CHECK(out, "slam_fs_create_assoc_proposal: NULL out");
    *out = nullptr;
    SLAM_ARG_CHECK(n_particles >= 1 && n_particles <= (int64_t(1) << 24),
                   "slam_fs_create_assoc_proposal: need 1 <= n_particles <= 2^24");
    SLAM_ARG_CHECK(max_landmarks >= 1, "slam_fs_create_assoc_proposal: need max_landmarks >= 1");
    SLAM_ARG_CHECK(std::isfinite(acfg->log_p_new),
                   "slam_fs_create_assoc_proposal: non-finite log_p_new");
    SLAM_ARG_CHECK(cfg->pf.motion == SLAM_MOTION_LINEAR,
                   "slam_fs_create_assoc_proposal: pf.motion must be SLAM_MOTION_LINEAR");
    return fs_create_impl(cfg, acfg, pcfg, n_particles, max_landmarks, device, out);
}

}  // extern "C"

namespace {

// the device side of fs_create_impl
int fs_create_buffers(slam_fs* f, const slam_fs_assoc_config* acfg,
                      const slam_fs_proposal_config* pcfg) {
    DeviceMem& m = f->mem;
    const hipStream_t st = f->pf->stream;
    const size_t nl = (size_t)f->nl, npad = (size_t)f->npad;
    const size_t map_count = (size_t)kFsComp * nl * npad;
    int rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = m.alloc(&f->map[k], map_count))) return rc;
        SLAM_HIP_TRY(hipMemsetAsync(f->map[k], 0, sizeof(double) * map_count, st));
    }
    if ((rc = m.alloc(&f->L, npad)) || (rc = m.alloc(&f->bmax, (size_t)f->nb + 1)) ||
        (rc = m.alloc(&f->seen_dev, nl)) || (rc = m.alloc(&f->list_dev, nl)))
        return rc;
    SLAM_HIP_TRY(hipMemsetAsync(f->seen_dev, 0, sizeof(int32_t) * nl, st));
    if (acfg) {
        f->assoc = true;
        f->acfg = *acfg;
        f->acfg.record = acfg->record ? 1 : 0;
        for (int k = 0; k < 2; ++k) {
            if ((rc = m.alloc(&f->cnt[k], npad))) return rc;
            SLAM_HIP_TRY(hipMemsetAsync(f->cnt[k], 0, sizeof(int32_t) * npad, st));
        }
        if ((rc = m.alloc(&f->stamp, npad * nl))) return rc;
        SLAM_HIP_TRY(hipMemsetAsync(f->stamp, 0, sizeof(int32_t) * npad * nl, st));
        if ((rc = m.alloc(&f->bcnt, (size_t)f->nb)) ||
            (rc = m.alloc_pinned(&f->cmax_pin, &f->cmax_pin_dev, 1,
                                 hipHostMallocMapped | hipHostMallocCoherent)))
            return rc;
        *f->cmax_pin = 0;
    }
    if (pcfg) {
        f->prop = true;
        f->pcfg.record = pcfg->record ? 1 : 0;
        const double* F = f->cfg.pf.q_factor;
        auto q = [F](int i, int j) { return (F[i] * F[j] + F[3 + i] * F[3 + j]) + F[6 + i] * F[6 + j]; };
        f->propq = FsPropQ{q(0, 0), q(0, 1), q(0, 2), q(1, 1), q(1, 2), q(2, 2)};
        if (f->pcfg.record && (rc = m.alloc(&f->prop_rec, 9 * npad))) return rc;
    }
    for (auto& pr : f->ev)
        for (auto& ev : pr)
            if ((rc = m.event(&ev))) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(st));
    return SLAM_OK;
}

// slam_fs_create, and slam_fs_create_assoc's second half (acfg != NULL)
int fs_create_impl(const slam_fs_config* cfg, const slam_fs_assoc_config* acfg,
                   const slam_fs_proposal_config* pcfg, int64_t n_particles, int32_t n_landmarks,
                   int device, slam_fs** out) {
    SLAM_ARG_CHECK(cfg && out, "slam_fs_create: NULL argument");
    *out = nullptr;
    SLAM_ARG_CHECK(n_particles >= 1 && n_particles <= (int64_t(1) << 24),
                   "slam_fs_create: need 1 <= n_particles <= 2^24");
    SLAM_ARG_CHECK(n_landmarks >= 1, "slam_fs_create: need n_landmarks >= 1");
    SLAM_ARG_CHECK(cfg->pf.motion == SLAM_MOTION_LINEAR || cfg->pf.motion == SLAM_MOTION_VELOCITY,
                   "slam_fs_create: bad motion model");
    SLAM_ARG_CHECK(cfg->r_dist > 0.0 && std::sin(cfg->r_dir) != 0.0 && std::isfinite(cfg->r_orient),
                   "slam_fs_create: need r_dist > 0, sin(r_dir) != 0, finite r_orient");
    slam_pf_config pc = cfg->pf;
    pc.r_cov[0] = pc.r_cov[3] = 1.0;        // ignored here: the single handle only checks it
    pc.r_cov[1] = pc.r_cov[2] = 0.0;
    pc.likelihood = SLAM_LIK_PRODUCT;       // zero landmarks: the factor is exactly 1
    slam_pf* pf = nullptr;
    int rc = create_impl(&pc, n_particles, n_particles, 0, 0, nullptr, device, &pf, false);
    if (rc) return rc;
    HandlePtr<slam_fs, slam_fs_destroy> fp(new slam_fs());
    slam_fs* f = fp.get();
    f->pf = pf;
    f->cfg = *cfg;
    f->cfg.use_orient = cfg->use_orient ? 1 : 0;
    f->n = n_particles;
    f->npad = (n_particles + kFsThreads - 1) / kFsThreads * kFsThreads;
    f->nl = n_landmarks;
    f->nb = (int32_t)(f->npad / kFsThreads);
    f->seen.assign((size_t)n_landmarks, 0);
    if ((rc = fs_create_buffers(f, acfg, pcfg)))
        return fail(rc, std::string("slam_fs_create: ") + slam_last_error());
    *out = fp.release();
    return SLAM_OK;
}

// the counts of the current half on the host (synchronises)
int fs_counts_host(slam_fs* f, std::vector<int32_t>& c) {
    c.resize((size_t)f->n);
    SLAM_HIP_TRY(hipMemcpyAsync(c.data(), f->cnt[f->ccur], sizeof(int32_t) * (size_t)f->n,
                                hipMemcpyDeviceToHost, f->pf->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    return SLAM_OK;
}

// every slot of the current evidence half at init (the slots at or above a
// particle's count are never read: a slot the update creates takes init)
int fs_evidence_init(slam_fs* f) {
    SLAM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)f->evd[f->ecur], f->prcfg.init,
                                   (size_t)f->nl * (size_t)f->npad, f->pf->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_fs_destroy(slam_fs* f) {
    if (!f) return SLAM_OK;
    if (f->pf) {
        (void)hipSetDevice(f->pf->device);
        (void)hipStreamSynchronize(f->pf->stream);
    }
    slam_pf_destroy(f->pf);
    delete f;
    return SLAM_OK;
}

int slam_fs_info(slam_fs* f, int64_t* n_particles, int32_t* n_landmarks, int32_t* n_seen) {
    SLAM_ARG_CHECK(f, "slam_fs_info: NULL handle");
    if (n_particles) *n_particles = f->n;
    if (n_landmarks) *n_landmarks = f->nl;
    if (n_seen && f->assoc) {
        SLAM_HIP_TRY(hipSetDevice(f->pf->device));
        std::vector<int32_t> c;
        int rc = fs_counts_host(f, c);
        if (rc) return rc;
        *n_seen = *std::max_element(c.begin(), c.end());
    } else if (n_seen) {
        *n_seen = (int32_t)std::count(f->seen.begin(), f->seen.end(), 1);
    }
    return SLAM_OK;
}

int slam_fs_set_state(slam_fs* f, const double* x, const double* y, const double* th,
                      const double* w) {
    SLAM_ARG_CHECK(f, "slam_fs_set_state: NULL handle");
    return slam_pf_set_state(f->pf, x, y, th, w);
}

int slam_fs_get_state(slam_fs* f, double* x, double* y, double* th, double* w) {
    SLAM_ARG_CHECK(f, "slam_fs_get_state: NULL handle");
    return slam_pf_get_state(f->pf, x, y, th, w);
}

int slam_fs_set_resample_next(slam_fs* f, int32_t on) {
    SLAM_ARG_CHECK(f, "slam_fs_set_resample_next: NULL handle");
    return slam_pf_set_resample_next(f->pf, on);
}

int slam_fs_set_maps(slam_fs* f, const int32_t* seen, const double* mean, const double* cov) {
    SLAM_ARG_CHECK(f, "slam_fs_set_maps: NULL handle");
    SLAM_ARG_CHECK((seen || f->assoc) && mean && cov, "slam_fs_set_maps: NULL argument");
    slam_pf* h = f->pf;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    // an associating handle ignores seen: every slot is taken, the counts say which hold
    if (f->assoc) return fs_maps_io(f, true, const_cast<double*>(mean), const_cast<double*>(cov));
    for (int32_t j = 0; j < f->nl; ++j) f->seen[(size_t)j] = seen[j] ? 1 : 0;
    SLAM_HIP_TRY(hipMemcpyAsync(f->seen_dev, f->seen.data(), sizeof(int32_t) * (size_t)f->nl,
                                hipMemcpyHostToDevice, h->stream));
    return fs_maps_io(f, true, const_cast<double*>(mean), const_cast<double*>(cov));
}

int slam_fs_get_maps(slam_fs* f, int32_t* seen, double* mean, double* cov) {
    SLAM_ARG_CHECK(f, "slam_fs_get_maps: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    if (seen && f->assoc) {
        std::vector<int32_t> c;
        int rc = fs_counts_host(f, c);
        if (rc) return rc;
        const int32_t cm = *std::max_element(c.begin(), c.end());
        for (int32_t j = 0; j < f->nl; ++j) seen[j] = j < cm;
    } else if (seen) {
        std::copy(f->seen.begin(), f->seen.end(), seen);
    }
    return fs_maps_io(f, false, mean, cov);
}

int slam_fs_get_map(slam_fs* f, int64_t particle, int32_t* seen, double* mean, double* cov) {
    SLAM_ARG_CHECK(f, "slam_fs_get_map: NULL handle");
    SLAM_ARG_CHECK(particle >= 0 && particle < f->n, "slam_fs_get_map: no such particle");
    slam_pf* h = f->pf;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if (seen && f->assoc) {
        int32_t cp = 0;
        SLAM_HIP_TRY(hipMemcpyAsync(&cp, f->cnt[f->ccur] + particle, sizeof(int32_t),
                                    hipMemcpyDeviceToHost, h->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        for (int32_t j = 0; j < f->nl; ++j) seen[j] = j < cp;
    } else if (seen) {
        std::copy(f->seen.begin(), f->seen.end(), seen);
    }
    int rc = fs_reserve_stage(f, 5 * (int64_t)f->nl);
    if (rc) return rc;
    for (int pass = 0; pass < 2; ++pass) {
        double* host = pass == 0 ? mean : cov;
        if (!host) continue;
        const int32_t comp0 = pass == 0 ? 0 : 2, ncomp = pass == 0 ? 2 : 3;
        double* st = f->stage + (pass == 0 ? 0 : 2 * (size_t)f->nl);
        if (f->assoc)
            fs_assoc_pack_kernel<<<fs_grid(1, f->nl), kFsThreads, 0, h->stream>>>(
                f->n, f->npad, f->nl, particle, 1, comp0, ncomp, f->cnt[f->ccur], f->map[f->mcur],
                st);
        else
            fs_map_pack_kernel<<<fs_grid(1, f->nl), kFsThreads, 0, h->stream>>>(
                f->n, f->npad, f->nl, particle, 1, comp0, ncomp, f->seen_dev, f->map[f->mcur], st);
        SLAM_HIP_TRY(hipGetLastError());
        SLAM_HIP_TRY(hipMemcpyAsync(host, st, sizeof(double) * (size_t)f->nl * ncomp,
                                    hipMemcpyDeviceToHost, h->stream));
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_fs_step(slam_fs* f, const double* control, int32_t k, const int64_t* ids, const double* obs,
                 const double* noise, double u_resample, slam_pf_result* res) {
    SLAM_ARG_CHECK(f && control, "slam_fs_step: NULL argument");
    int rc = fs_check_obs(f, "slam_fs_step", k, ids, obs);
    if (rc) return rc;
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    if ((rc = fs_stage_step_obs(f, k, ids, obs))) return rc;
    return fs_step_records(f, control, k, f->obs_dev, f->obs_host.data(), noise, u_resample, res);
}

int slam_fs_resample(slam_fs* f, double u_resample, int32_t force, int32_t* resampled) {
    SLAM_ARG_CHECK(f, "slam_fs_resample: NULL handle");
    slam_pf* h = f->pf;
    h->prep_step = -1;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const int32_t go = force ? 1 : h->resample_next;
    if (resampled) *resampled = go;
    if (!go) return SLAM_OK;
    int rc = fs_enqueue_resample(f, u_resample);
    if (rc) return rc;
    int32_t st = 0;
    SLAM_HIP_TRY(hipMemcpyAsync(&st, h->flags + kFlagStatus, 4, hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = set_flag(h, kFlagStatus, 0))) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    if (st & 1)
        return fail(SLAM_ERR_INDEX, "resample position beyond the last cumulative weight "
                                    "(IndexError in particle_filter.py:219)");
    return SLAM_OK;
}

int slam_fs_predict(slam_fs* f, const double* control, const double* noise) {
    SLAM_ARG_CHECK(f && control, "slam_fs_predict: NULL argument");
    SLAM_ARG_CHECK(!f->prop, "slam_fs_predict: a proposal handle needs the step's scan (slam_fs_step)");
    slam_pf* h = f->pf;
    h->prep_step = -1;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc = fs_enqueue_predict(f, control, noise);
    if (rc || (rc = set_flag(h, kFlagResample, h->resample_next))) return rc;
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_fs_update(slam_fs* f, int32_t k, const int64_t* ids, const double* obs,
                   slam_pf_result* res) {
    SLAM_ARG_CHECK(f, "slam_fs_update: NULL handle");
    SLAM_ARG_CHECK(!f->prop, "slam_fs_update: a proposal handle needs the step's control (slam_fs_step)");
    int rc = fs_check_obs(f, "slam_fs_update", k, ids, obs);
    if (rc) return rc;
    slam_pf* h = f->pf;
    h->prep_step = -1;
    SLAM_HIP_TRY(hipSetDevice(h->device));
    if ((rc = fs_stage_step_obs(f, k, ids, obs))) return rc;
    if ((rc = fs_enqueue_update(f, k, f->obs_dev, 0))) return rc;
    if (f->assoc) {
        rc = sync_results(h, 0, 1, res);
        fs_note_seen(f, k, f->obs_host.data());
        return rc;
    }
    fs_note_seen(f, k, f->obs_host.data());
    return sync_results(h, 0, 1, res);
}

int slam_fs_load_observations(slam_fs* f, int32_t n_steps, const int32_t* counts, const int64_t* ids,
                              const double* obs) {
    SLAM_ARG_CHECK(f, "slam_fs_load_observations: NULL handle");
    SLAM_ARG_CHECK(n_steps > 0 && counts, "slam_fs_load_observations: bad argument");
    std::vector<int64_t> off((size_t)n_steps + 1, 0);
    int rc;
    for (int32_t s = 0; s < n_steps; ++s) {
        const int64_t o = off[(size_t)s];
        if ((rc = fs_check_obs(f, "slam_fs_load_observations", counts[s], ids ? ids + o : nullptr,
                               obs ? obs + 3 * o : nullptr)))
            return rc;
        off[(size_t)s + 1] = o + counts[s];
    }
    const int64_t total = off[(size_t)n_steps];
    f->obs_host.resize((size_t)total);
    for (int64_t t = 0; t < total; ++t)
        f->obs_host[(size_t)t] = fs_make_obs(f, ids ? ids[t] : -1, obs + 3 * t);
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    f->run_off.clear();
    if (total > 0) {
        if ((rc = fs_reserve_obs(f, total))) return rc;
        SLAM_HIP_TRY(hipMemcpyAsync(f->obs_dev, f->obs_host.data(), sizeof(FsObs) * (size_t)total,
                                    hipMemcpyHostToDevice, f->pf->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    }
    f->run_off = std::move(off);
    return SLAM_OK;
}

int slam_fs_run(slam_fs* f, int32_t first_step, int32_t n_steps, const double* controls,
                slam_pf_result* results) {
    SLAM_ARG_CHECK(f && controls && n_steps > 0, "slam_fs_run: bad argument");
    SLAM_ARG_CHECK(first_step >= 0 && (size_t)first_step + (size_t)n_steps < f->run_off.size(),
                   "slam_fs_run: steps outside the loaded observations");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    for (int32_t s = 0; s < n_steps; ++s) {
        const int64_t o = f->run_off[(size_t)(first_step + s)];
        const int32_t k = (int32_t)(f->run_off[(size_t)(first_step + s) + 1] - o);
        const int rc = fs_step_records(f, controls + 2 * s, k, f->obs_dev + o, f->obs_host.data() + o,
                                       nullptr, std::nan(""), results ? results + s : nullptr);
        if (rc) return rc;
    }
    return SLAM_OK;
}

int slam_fs_set_counts(slam_fs* f, const int32_t* counts) {
    SLAM_ARG_CHECK(f && counts, "slam_fs_set_counts: NULL argument");
    SLAM_ARG_CHECK(f->assoc, "slam_fs_set_counts: not an associating handle");
    int32_t cm = 0;
    for (int64_t p = 0; p < f->n; ++p) {
        SLAM_ARG_CHECK(counts[p] >= 0 && counts[p] <= f->nl,
                       "slam_fs_set_counts: need 0 <= count <= max_landmarks");
        cm = std::max(cm, counts[p]);
    }
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    SLAM_HIP_TRY(hipMemcpyAsync(f->cnt[f->ccur], counts, sizeof(int32_t) * (size_t)f->n,
                                hipMemcpyHostToDevice, f->pf->stream));
    if (f->prune) {
        const int rc = fs_evidence_init(f);     // the slots that now hold start at init
        if (rc) return rc;
    }
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    f->cmax = cm;
    return SLAM_OK;
}

int slam_fs_check_prune_config(const slam_fs_prune_config* c) {
    SLAM_ARG_CHECK(c, "slam_fs_check_prune_config: NULL config");
    SLAM_ARG_CHECK(std::isfinite(c->view_range) && c->view_range > 0.0,
                   "slam_fs_check_prune_config: need a finite view_range > 0");
    SLAM_ARG_CHECK(!c->use_angle || !std::isnan(c->view_tan),
                   "slam_fs_check_prune_config: view_tan is NaN");
    SLAM_ARG_CHECK(c->hit >= 0 && c->miss >= 0, "slam_fs_check_prune_config: need hit, miss >= 0");
    SLAM_ARG_CHECK(c->ev_max >= c->init, "slam_fs_check_prune_config: need ev_max >= init");
    SLAM_ARG_CHECK(c->init >= c->remove_below,
                   "slam_fs_check_prune_config: need init >= remove_below");
    return SLAM_OK;
}

int slam_fs_set_pruning(slam_fs* f, const slam_fs_prune_config* c) {
    SLAM_ARG_CHECK(f, "slam_fs_set_pruning: NULL handle");
    SLAM_ARG_CHECK(f->assoc, "slam_fs_set_pruning: not an associating handle");
    if (!c) {
        f->prune = false;
        return SLAM_OK;
    }
    int rc = slam_fs_check_prune_config(c);
    if (rc) return rc;
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    if (!f->evd[0]) {
        const size_t rows = (size_t)f->nl * (size_t)f->npad;
        if ((rc = f->mem.alloc(&f->evd[0], rows)) || (rc = f->mem.alloc(&f->evd[1], rows)) ||
            (rc = f->mem.alloc(&f->cnt0, (size_t)f->npad)) ||
            (rc = f->mem.alloc(&f->removed, (size_t)f->npad))) {
            f->mem.release(f->evd[0]);
            f->mem.release(f->evd[1]);
            f->mem.release(f->cnt0);
            f->mem.release(f->removed);
            (void)hipGetLastError();
            return rc;
        }
    }
    const bool was = f->prune;
    f->prcfg = *c;
    f->prcfg.use_angle = c->use_angle ? 1 : 0;
    f->prune = true;
    if (!was) {
        // turned on: every live slot starts at init, nothing removed yet
        if ((rc = fs_evidence_init(f))) return rc;
        SLAM_HIP_TRY(hipMemsetAsync(f->removed, 0, sizeof(int32_t) * (size_t)f->npad, f->pf->stream));
        SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    }
    return SLAM_OK;
}

int slam_fs_set_evidence(slam_fs* f, const int32_t* ev) {
    SLAM_ARG_CHECK(f && ev, "slam_fs_set_evidence: NULL argument");
    SLAM_ARG_CHECK(f->prune, "slam_fs_set_evidence: pruning is off");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    const size_t npad = (size_t)f->npad, nl = (size_t)f->nl;
    std::vector<int32_t> rows(nl * npad, f->prcfg.init);
    for (size_t p = 0; p < (size_t)f->n; ++p)
        for (size_t j = 0; j < nl; ++j) rows[j * npad + p] = ev[p * nl + j];
    SLAM_HIP_TRY(hipMemcpyAsync(f->evd[f->ecur], rows.data(), sizeof(int32_t) * rows.size(),
                                hipMemcpyHostToDevice, f->pf->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    return SLAM_OK;
}

int slam_fs_get_evidence(slam_fs* f, int32_t* ev) {
    SLAM_ARG_CHECK(f && ev, "slam_fs_get_evidence: NULL argument");
    SLAM_ARG_CHECK(f->prune, "slam_fs_get_evidence: pruning is off");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    const size_t npad = (size_t)f->npad, nl = (size_t)f->nl;
    std::vector<int32_t> rows(nl * npad), c;
    SLAM_HIP_TRY(hipMemcpyAsync(rows.data(), f->evd[f->ecur], sizeof(int32_t) * rows.size(),
                                hipMemcpyDeviceToHost, f->pf->stream));
    const int rc = fs_counts_host(f, c);        // synchronises
    if (rc) return rc;
    for (size_t p = 0; p < (size_t)f->n; ++p)
        for (size_t j = 0; j < nl; ++j)
            ev[p * nl + j] = (int32_t)j < c[p] ? rows[j * npad + p] : 0;
    return SLAM_OK;
}

int slam_fs_get_removed(slam_fs* f, int32_t* removed) {
    SLAM_ARG_CHECK(f && removed, "slam_fs_get_removed: NULL argument");
    SLAM_ARG_CHECK(f->prune, "slam_fs_get_removed: pruning is off");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    SLAM_HIP_TRY(hipMemcpyAsync(removed, f->removed, sizeof(int32_t) * (size_t)f->n,
                                hipMemcpyDeviceToHost, f->pf->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    return SLAM_OK;
}

int slam_fs_get_counts(slam_fs* f, int32_t* counts) {
    SLAM_ARG_CHECK(f && counts, "slam_fs_get_counts: NULL argument");
    SLAM_ARG_CHECK(f->assoc, "slam_fs_get_counts: not an associating handle");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    SLAM_HIP_TRY(hipMemcpyAsync(counts, f->cnt[f->ccur], sizeof(int32_t) * (size_t)f->n,
                                hipMemcpyDeviceToHost, f->pf->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    return SLAM_OK;
}

int slam_fs_get_assoc(slam_fs* f, int32_t* out) {
    SLAM_ARG_CHECK(f && out, "slam_fs_get_assoc: NULL argument");
    SLAM_ARG_CHECK(f->assoc, "slam_fs_get_assoc: not an associating handle");
    // a proposal handle's kernel keeps the choices between its passes whatever record says
    SLAM_ARG_CHECK(f->acfg.record || f->prop,
                   "slam_fs_get_assoc: the handle does not record (record = 0)");
    if (f->assoc_k == 0) return SLAM_OK;
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    SLAM_HIP_TRY(hipMemcpy2DAsync(out, sizeof(int32_t) * (size_t)f->n, f->assoc_dev,
                                  sizeof(int32_t) * (size_t)f->npad, sizeof(int32_t) * (size_t)f->n,
                                  (size_t)f->assoc_k, hipMemcpyDeviceToHost, f->pf->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    return SLAM_OK;
}

int slam_fs_get_proposal(slam_fs* f, double* mean, double* cov, double* L) {
    SLAM_ARG_CHECK(f, "slam_fs_get_proposal: NULL handle");
    SLAM_ARG_CHECK(f->prop, "slam_fs_get_proposal: not a proposal handle");
    SLAM_ARG_CHECK(f->pcfg.record, "slam_fs_get_proposal: the handle does not record (record = 0)");
    SLAM_ARG_CHECK(f->prop_ran, "slam_fs_get_proposal: no step has run yet");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    const hipStream_t st = f->pf->stream;
    const size_t n = (size_t)f->n, npad = (size_t)f->npad;
    std::vector<double> rec;
    if (mean || cov) {
        rec.resize(9 * npad);
        SLAM_HIP_TRY(hipMemcpyAsync(rec.data(), f->prop_rec, sizeof(double) * 9 * npad,
                                    hipMemcpyDeviceToHost, st));
    }
    if (L) SLAM_HIP_TRY(hipMemcpyAsync(L, f->L, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    SLAM_HIP_TRY(hipStreamSynchronize(st));
    for (size_t p = 0; p < n && (mean || cov); ++p) {
        for (int c = 0; c < 3 && mean; ++c) mean[3 * p + c] = rec[(size_t)c * npad + p];
        for (int c = 0; c < 6 && cov; ++c) cov[6 * p + c] = rec[(size_t)(3 + c) * npad + p];
    }
    return SLAM_OK;
}

int slam_fs_timing(slam_fs* f, double* out) {
    SLAM_ARG_CHECK(f && out, "slam_fs_timing: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(f->pf->device));
    SLAM_HIP_TRY(hipStreamSynchronize(f->pf->stream));
    for (int k = 0; k < 4; ++k) {
        float ms = 0.f;
        if (f->ran[k]) SLAM_HIP_TRY(hipEventElapsedTime(&ms, f->ev[k][0], f->ev[k][1]));
        out[k] = ms;
    }
    return SLAM_OK;
}

}  // extern "C"
