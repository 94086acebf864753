// pf_batch_api.hip -- C-ABI of the particle-filter ensemble (include/slam_hip.h,
// "Particle-filter ensemble"): n_filters independent ParticleFilter instances
// (particle_filter.py:18-237) of n_particles <= 8192 each on one GPU, one
// workgroup per filter (pf_batch.inl).  A step or a run of any length is one
// launch; the records land in coherent pinned host memory.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "device_mem.hpp"
#include "pf_batch.inl"

using namespace slam;

struct slam_pfb {
    int device = 0;
    int32_t B = 0, n = 0, npad = 0, nl = 0;
    int32_t motion = 0, lik = 0;
    std::vector<slam_pf_config> cfgs;
    hipStream_t stream = nullptr;
    DeviceMem mem;
    double* x[2] = {nullptr, nullptr};
    double* y[2] = {nullptr, nullptr};
    double* th[2] = {nullptr, nullptr};
    int cur = 0;
    double *w_un = nullptr, *s_cur = nullptr;
    uint64_t* c = nullptr;
    PfbSpecial* spec = nullptr;
    int32_t* flags = nullptr;
    PfbFilter* filt = nullptr;
    double* lm = nullptr;
    int32_t *leaves = nullptr, *ops = nullptr;
    int32_t nleaves = 0, nops = 0;
    // one staged step (slam_pfb_step)
    double *ctl1 = nullptr, *z1 = nullptr, *noise = nullptr, *ofs = nullptr;
    int32_t *idx = nullptr, *istat = nullptr, *ispec = nullptr;
    // loaded batch (slam_pfb_load_observations / slam_pfb_run)
    double *ctl = nullptr, *z_all = nullptr;
    int32_t z_steps = 0, ctl_cap = 0;
    slam_pf_result* res_host = nullptr;     // pinned, coherent
    slam_pf_result* res_host_dev = nullptr;
    size_t res_cap = 0;
    uint32_t stepno = 0;
    double ess_band = 1e-9;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    int64_t last_launches = 0;
};

namespace {

// [B][n] host rows <-> [B][npad] device rows
int rows_to_device(slam_pfb* h, double* dst, const double* src) {
    SLAM_HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double) * h->npad, src, sizeof(double) * h->n,
                                  sizeof(double) * h->n, h->B, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}
int rows_to_host(slam_pfb* h, double* dst, const double* src) {
    SLAM_HIP_TRY(hipMemcpy2DAsync(dst, sizeof(double) * h->n, src, sizeof(double) * h->npad,
                                  sizeof(double) * h->n, h->B, hipMemcpyDeviceToHost, h->stream));
    return SLAM_OK;
}

int ensure_results(slam_pfb* h, size_t records) {
    if (records <= h->res_cap) return SLAM_OK;
    h->mem.release(h->res_host);
    h->res_cap = 0;
    const int rc = h->mem.alloc_pinned(&h->res_host, &h->res_host_dev, records,
                                       hipHostMallocMapped | hipHostMallocCoherent);
    if (rc) return rc;
    h->res_cap = records;
    return SLAM_OK;
}

PfbArgs make_args(slam_pfb* h) {
    PfbArgs a{};
    a.B = h->B;
    a.n = h->n;
    a.npad = h->npad;
    a.nl = h->nl;
    for (int k = 0; k < 2; ++k) {
        a.x[k] = h->x[k];
        a.y[k] = h->y[k];
        a.th[k] = h->th[k];
    }
    a.w_un = h->w_un;
    a.s_cur = h->s_cur;
    a.c = h->c;
    a.spec = h->spec;
    a.flags = h->flags;
    a.filt = h->filt;
    a.lm = h->lm;
    a.leaves = h->leaves;
    a.ops = h->ops;
    a.nleaves = h->nleaves;
    a.nops = h->nops;
    a.res = h->res_host_dev;
    a.stepno = h->stepno;
    a.cur = h->cur;
    a.ess_band = h->ess_band;
    return a;
}

// one launch: steps [a.first, a.first + a.nsteps) of every filter
int launch_run(slam_pfb* h, const PfbArgs& a, bool host_noise) {
    const size_t lds = h->nl <= kPfbLdsNl ? sizeof(double) * 4 * (size_t)h->nl : 0;
    const dim3 grid((unsigned)h->B), block(kPfbThreads);
    SLAM_HIP_TRY(hipEventRecord(h->ev0, h->stream));
#define SLAM_PFB(M, L, HN) pfb_run_kernel<M, L, HN><<<grid, block, lds, h->stream>>>(a)
    if (h->motion == SLAM_MOTION_LINEAR) {
        if (h->lik == SLAM_LIK_PRODUCT) {
            if (host_noise) SLAM_PFB(0, 0, true); else SLAM_PFB(0, 0, false);
        } else {
            if (host_noise) SLAM_PFB(0, 1, true); else SLAM_PFB(0, 1, false);
        }
    } else {
        if (h->lik == SLAM_LIK_PRODUCT) {
            if (host_noise) SLAM_PFB(1, 0, true); else SLAM_PFB(1, 0, false);
        } else {
            if (host_noise) SLAM_PFB(1, 1, true); else SLAM_PFB(1, 1, false);
        }
    }
#undef SLAM_PFB
    SLAM_HIP_TRY(hipGetLastError());
    SLAM_HIP_TRY(hipEventRecord(h->ev1, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    SLAM_HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->last_ms = ms;
    h->last_launches = 1;
    h->stepno += (uint32_t)a.nsteps;
    h->cur = (h->cur + a.nsteps) & 1;
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_pfb_create(const slam_pf_config* cfgs, int32_t n_filters, int32_t n_particles,
                    int32_t n_landmarks, const double* landmarks, int device, slam_pfb** out) {
    SLAM_ARG_CHECK(cfgs && out && landmarks, "slam_pfb_create: NULL argument");
    *out = nullptr;
    SLAM_ARG_CHECK(n_filters >= 1, "slam_pfb_create: n_filters < 1");
    SLAM_ARG_CHECK(n_particles >= 1 && n_particles <= kPfbMaxN,
                   "slam_pfb_create: n_particles outside 1..8192 (one np.sum buffer per filter)");
    SLAM_ARG_CHECK(n_landmarks >= 1, "slam_pfb_create: n_landmarks < 1");
    SLAM_ARG_CHECK(cfgs[0].motion == SLAM_MOTION_LINEAR || cfgs[0].motion == SLAM_MOTION_VELOCITY,
                   "slam_pfb_create: bad motion model");
    SLAM_ARG_CHECK(cfgs[0].likelihood == SLAM_LIK_PRODUCT || cfgs[0].likelihood == SLAM_LIK_LOGSUM,
                   "slam_pfb_create: bad likelihood mode");
    for (int32_t b = 1; b < n_filters; ++b)
        SLAM_ARG_CHECK(cfgs[b].motion == cfgs[0].motion && cfgs[b].likelihood == cfgs[0].likelihood &&
                           cfgs[b].dt == cfgs[0].dt,
                       "slam_pfb_create: motion, likelihood and dt must agree across the filters");
    std::vector<PfbFilter> filt((size_t)n_filters);
    for (int32_t b = 0; b < n_filters; ++b) {
        PfbFilter& f = filt[b];
        std::memset(&f, 0, sizeof f);
        // the landmark loop of the log-sum form (no per-step closed-form words here)
        const int rc = lik_const_from(cfgs[b].r_cov, n_landmarks, false, f.lc);
        if (rc) return rc;
        f.pc.dt = cfgs[b].dt;
        for (int k = 0; k < 6; ++k) f.pc.alphas[k] = cfgs[b].alphas[k];
        for (int k = 0; k < 9; ++k) f.pc.q[k] = cfgs[b].q_factor[k];
        f.pc.np_recip = 1.0 / (double)n_particles;           // particle_filter.py:32
        f.pc.rstep = 1.0 / (double)n_particles;              // :213 arange step
        f.pc.n_global = n_particles;
        f.pc.gbase = 0;
        f.seed = cfgs[b].seed;
        f.ess_th = cfgs[b].ess_threshold;
    }
    std::vector<int32_t> leaves, ops;
    if (n_particles >= 8) pairwise_sum_split(0, n_particles, leaves, ops);
    SLAM_ARG_CHECK(leaves.size() / 2 <= (size_t)kPfbMaxLeaves && ops.size() <= 2 * (size_t)kPfbMaxLeaves,
                   "slam_pfb_create: np.sum tree larger than the kernel's table");

    int ndev = 0;
    SLAM_HIP_TRY(hipGetDeviceCount(&ndev));
    SLAM_ARG_CHECK(device >= 0 && device < ndev, "slam_pfb_create: no such HIP device");
    SLAM_HIP_TRY(hipSetDevice(device));
    HandlePtr<slam_pfb, slam_pfb_destroy> hp(new slam_pfb());
    slam_pfb* h = hp.get();
    h->device = device;
    h->B = n_filters;
    h->n = n_particles;
    h->npad = (n_particles + kPfbTile - 1) / kPfbTile * kPfbTile;
    h->nl = n_landmarks;
    h->motion = cfgs[0].motion;
    h->lik = cfgs[0].likelihood;
    h->cfgs.assign(cfgs, cfgs + n_filters);
    h->nleaves = (int32_t)(leaves.size() / 2);
    h->nops = (int32_t)ops.size();
    const size_t B = (size_t)n_filters, n = (size_t)n_particles, npad = (size_t)h->npad;
    const size_t nl2 = 2 * (size_t)n_landmarks;
    SLAM_HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    DeviceMem& m = h->mem;
    int r;
    if ((r = m.event(&h->ev0)) || (r = m.event(&h->ev1))) return r;
    for (int k = 0; k < 2; ++k)
        if ((r = m.alloc(&h->x[k], B * npad)) || (r = m.alloc(&h->y[k], B * npad)) ||
            (r = m.alloc(&h->th[k], B * npad)))
            return r;
    if ((r = m.alloc(&h->w_un, B * npad)) || (r = m.alloc(&h->s_cur, B)) ||
        (r = m.alloc(&h->c, B * npad)) || (r = m.alloc(&h->spec, B * n)) ||
        (r = m.alloc(&h->flags, B)) || (r = m.alloc(&h->filt, B)) ||
        (r = m.alloc(&h->lm, B * nl2)) || (r = m.alloc(&h->leaves, leaves.size() + 2)) ||
        (r = m.alloc(&h->ops, ops.size() + 1)) || (r = m.alloc(&h->ctl1, 2 * B)) ||
        (r = m.alloc(&h->z1, B * nl2)) || (r = m.alloc(&h->noise, 3 * B * n)) ||
        (r = m.alloc(&h->ofs, B)) || (r = m.alloc(&h->idx, B * n)) ||
        (r = m.alloc(&h->istat, B)) || (r = m.alloc(&h->ispec, B)))
        return r;
    if ((r = ensure_results(h, B))) return r;
    // initial state: particle_filter.py:81-84 (pad slots: zero state, zero weight)
    std::vector<double> row(B * npad, 0.0);
    for (int q = 0; q < 3; ++q) {
        for (size_t b = 0; b < B; ++b)
            std::fill(row.begin() + b * npad, row.begin() + b * npad + n, cfgs[b].x0[q]);
        double* d0 = q == 0 ? h->x[0] : q == 1 ? h->y[0] : h->th[0];
        double* d1 = q == 0 ? h->x[1] : q == 1 ? h->y[1] : h->th[1];
        SLAM_HIP_TRY(hipMemcpy(d0, row.data(), sizeof(double) * B * npad, hipMemcpyHostToDevice));
        SLAM_HIP_TRY(hipMemcpy(d1, row.data(), sizeof(double) * B * npad, hipMemcpyHostToDevice));
    }
    std::fill(row.begin(), row.end(), 0.0);
    for (size_t b = 0; b < B; ++b)
        std::fill(row.begin() + b * npad, row.begin() + b * npad + n, 1.0 / (double)n_particles);
    SLAM_HIP_TRY(hipMemcpy(h->w_un, row.data(), sizeof(double) * B * npad, hipMemcpyHostToDevice));
    SLAM_HIP_TRY(hipMemset(h->c, 0, sizeof(uint64_t) * B * npad));
    std::vector<double> ones(B, 1.0);
    SLAM_HIP_TRY(hipMemcpy(h->s_cur, ones.data(), sizeof(double) * B, hipMemcpyHostToDevice));
    SLAM_HIP_TRY(hipMemset(h->flags, 0, sizeof(int32_t) * B));
    SLAM_HIP_TRY(hipMemcpy(h->filt, filt.data(), sizeof(PfbFilter) * B, hipMemcpyHostToDevice));
    SLAM_HIP_TRY(hipMemcpy(h->lm, landmarks, sizeof(double) * B * nl2, hipMemcpyHostToDevice));
    if (!leaves.empty()) {
        SLAM_HIP_TRY(hipMemcpy(h->leaves, leaves.data(), leaves.size() * 4, hipMemcpyHostToDevice));
        SLAM_HIP_TRY(hipMemcpy(h->ops, ops.data(), ops.size() * 4, hipMemcpyHostToDevice));
    }
    *out = hp.release();
    return SLAM_OK;
}

int slam_pfb_destroy(slam_pfb* h) {
    if (!h) return SLAM_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SLAM_OK;
}

int slam_pfb_info(slam_pfb* h, int32_t* n_filters, int32_t* n_particles, int32_t* n_landmarks) {
    SLAM_ARG_CHECK(h, "slam_pfb_info: NULL handle");
    if (n_filters) *n_filters = h->B;
    if (n_particles) *n_particles = h->n;
    if (n_landmarks) *n_landmarks = h->nl;
    return SLAM_OK;
}

int slam_pfb_set_state(slam_pfb* h, const double* x, const double* y, const double* th,
                       const double* w) {
    SLAM_ARG_CHECK(h, "slam_pfb_set_state: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const int c = h->cur;
    int rc;
    if (x && (rc = rows_to_device(h, h->x[c], x))) return rc;
    if (y && (rc = rows_to_device(h, h->y[c], y))) return rc;
    if (th && (rc = rows_to_device(h, h->th[c], th))) return rc;
    std::vector<double> ones;
    std::vector<int32_t> fl;
    if (w) {
        if ((rc = rows_to_device(h, h->w_un, w))) return rc;
        ones.assign((size_t)h->B, 1.0);
        fl.resize((size_t)h->B);
        // particle_filter.py:210-211: the resample decision from these weights
        for (int32_t b = 0; b < h->B; ++b) {
            double s2 = 0.0;
            const double* wb = w + (size_t)b * h->n;
            for (int32_t i = 0; i < h->n; ++i) s2 += wb[i] * wb[i];
            fl[b] = (1.0 / s2 < h->cfgs[b].ess_threshold) ? 1 : 0;
        }
        SLAM_HIP_TRY(hipMemcpyAsync(h->s_cur, ones.data(), sizeof(double) * h->B, hipMemcpyHostToDevice,
                                    h->stream));
        SLAM_HIP_TRY(hipMemcpyAsync(h->flags, fl.data(), sizeof(int32_t) * h->B, hipMemcpyHostToDevice,
                                    h->stream));
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_pfb_get_weights_raw(slam_pfb* h, double* w_un, double* s) {
    SLAM_ARG_CHECK(h, "slam_pfb_get_weights_raw: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (w_un && (rc = rows_to_host(h, w_un, h->w_un))) return rc;
    if (s)
        SLAM_HIP_TRY(hipMemcpyAsync(s, h->s_cur, sizeof(double) * h->B, hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_pfb_get_state(slam_pfb* h, double* x, double* y, double* th, double* w) {
    SLAM_ARG_CHECK(h, "slam_pfb_get_state: NULL handle");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const int c = h->cur;
    int rc;
    if (x && (rc = rows_to_host(h, x, h->x[c]))) return rc;
    if (y && (rc = rows_to_host(h, y, h->y[c]))) return rc;
    if (th && (rc = rows_to_host(h, th, h->th[c]))) return rc;
    std::vector<double> s;
    if (w) {
        s.resize((size_t)h->B);
        if ((rc = rows_to_host(h, w, h->w_un))) return rc;
        SLAM_HIP_TRY(hipMemcpyAsync(s.data(), h->s_cur, sizeof(double) * h->B, hipMemcpyDeviceToHost,
                                    h->stream));
    }
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    if (w) {
        // particle_filter.py:235-236: w = w_un / s (one IEEE division, as the
        // kernels form it), NaN -> 1/NP
        const double np_recip = 1.0 / (double)h->n;
        for (int32_t b = 0; b < h->B; ++b) {
            double* wb = w + (size_t)b * h->n;
            for (int32_t i = 0; i < h->n; ++i) {
                const double v = wb[i] / s[b];
                wb[i] = std::isnan(v) ? np_recip : v;
            }
        }
    }
    return SLAM_OK;
}

int slam_pfb_set_resample_next(slam_pfb* h, const int32_t* flags) {
    SLAM_ARG_CHECK(h && flags, "slam_pfb_set_resample_next: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    std::vector<int32_t> fl((size_t)h->B);
    SLAM_HIP_TRY(hipMemcpyAsync(fl.data(), h->flags, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    for (int32_t b = 0; b < h->B; ++b)
        if (flags[b] >= 0) fl[b] = flags[b] ? 1 : 0;
    SLAM_HIP_TRY(hipMemcpyAsync(h->flags, fl.data(), sizeof(int32_t) * h->B, hipMemcpyHostToDevice,
                                h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int slam_pfb_set_ess_band(slam_pfb* h, double band) {
    SLAM_ARG_CHECK(h && band >= 0.0, "slam_pfb_set_ess_band: bad argument");
    h->ess_band = band;
    return SLAM_OK;
}

int slam_pfb_step(slam_pfb* h, const double* control, const double* z, const double* noise,
                  const double* u_resample, slam_pf_result* res) {
    SLAM_ARG_CHECK(h && control && z, "slam_pfb_step: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    std::vector<double> ofs(B, std::numeric_limits<double>::quiet_NaN());
    if (u_resample)
        for (size_t b = 0; b < B; ++b)                       // particle_filter.py:214
            if (!std::isnan(u_resample[b])) ofs[b] = u_resample[b] * (1.0 / (double)h->n);
    SLAM_HIP_TRY(hipMemcpyAsync(h->ctl1, control, sizeof(double) * 2 * B, hipMemcpyHostToDevice, h->stream));
    SLAM_HIP_TRY(hipMemcpyAsync(h->z1, z, sizeof(double) * 2 * B * h->nl, hipMemcpyHostToDevice, h->stream));
    SLAM_HIP_TRY(hipMemcpyAsync(h->ofs, ofs.data(), sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    if (noise)
        SLAM_HIP_TRY(hipMemcpyAsync(h->noise, noise, sizeof(double) * 3 * B * h->n, hipMemcpyHostToDevice,
                                    h->stream));
    int rc = ensure_results(h, B);
    if (rc) return rc;
    PfbArgs a = make_args(h);
    a.ctl = h->ctl1;
    a.z = h->z1;
    a.noise = h->noise;
    a.ofs = h->ofs;
    a.first = 0;
    a.nsteps = 1;
    if ((rc = launch_run(h, a, noise != nullptr))) return rc;
    if (res) std::memcpy(res, h->res_host, sizeof(slam_pf_result) * B);
    return SLAM_OK;
}

int slam_pfb_load_observations(slam_pfb* h, int32_t n_steps, const double* z_all) {
    SLAM_ARG_CHECK(h && n_steps > 0 && z_all, "slam_pfb_load_observations: bad argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t per = 2 * (size_t)h->B * h->nl;
    if (n_steps > h->z_steps) {
        h->mem.release(h->z_all);
        h->z_steps = 0;
        const int rc = h->mem.alloc(&h->z_all, per * n_steps);
        if (rc) return rc;
    }
    SLAM_HIP_TRY(hipMemcpy(h->z_all, z_all, sizeof(double) * per * n_steps, hipMemcpyHostToDevice));
    h->z_steps = n_steps;
    return SLAM_OK;
}

int slam_pfb_run(slam_pfb* h, int32_t first_step, int32_t n_steps, const double* controls,
                 slam_pf_result* results) {
    SLAM_ARG_CHECK(h && controls && n_steps > 0, "slam_pfb_run: bad argument");
    SLAM_ARG_CHECK(first_step >= 0 && first_step + n_steps <= h->z_steps,
                   "slam_pfb_run: steps outside the loaded observations");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    int rc;
    if (n_steps > h->ctl_cap) {
        SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        h->mem.release(h->ctl);
        h->ctl_cap = 0;
        if ((rc = h->mem.alloc(&h->ctl, 2 * B * n_steps))) return rc;
        h->ctl_cap = n_steps;
    }
    if ((rc = ensure_results(h, B * n_steps))) return rc;
    SLAM_HIP_TRY(hipMemcpyAsync(h->ctl, controls, sizeof(double) * 2 * B * n_steps, hipMemcpyHostToDevice,
                                h->stream));
    PfbArgs a = make_args(h);
    a.ctl = h->ctl;
    a.z = h->z_all;
    a.noise = nullptr;
    a.ofs = nullptr;
    a.first = first_step;
    a.nsteps = n_steps;
    if ((rc = launch_run(h, a, false))) return rc;
    if (results) std::memcpy(results, h->res_host, sizeof(slam_pf_result) * B * n_steps);
    return SLAM_OK;
}

int slam_pfb_resample_indices(slam_pfb* h, const double* u_resample, int64_t* idx_out) {
    SLAM_ARG_CHECK(h && idx_out, "slam_pfb_resample_indices: NULL argument");
    SLAM_HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B, n = (size_t)h->n;
    std::vector<double> ofs(B, std::numeric_limits<double>::quiet_NaN());
    if (u_resample)
        for (size_t b = 0; b < B; ++b)
            if (!std::isnan(u_resample[b])) ofs[b] = u_resample[b] * (1.0 / (double)h->n);
    SLAM_HIP_TRY(hipMemcpyAsync(h->ofs, ofs.data(), sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    PfbArgs a = make_args(h);
    a.ofs = h->ofs;
    pfb_indices_kernel<<<dim3((unsigned)h->B), dim3(kPfbThreads), 0, h->stream>>>(a, h->idx, h->istat,
                                                                                   h->ispec);
    SLAM_HIP_TRY(hipGetLastError());
    std::vector<int32_t> idx(B * n), st(B);
    SLAM_HIP_TRY(hipMemcpyAsync(idx.data(), h->idx, sizeof(int32_t) * B * n, hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipMemcpyAsync(st.data(), h->istat, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
    SLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < B * n; ++i) idx_out[i] = idx[i];
    for (size_t b = 0; b < B; ++b)
        if (st[b] & 1)
            return fail(SLAM_ERR_INDEX, "slam_pfb_resample_indices: filter " + std::to_string(b) +
                                            ": resample position beyond the last cumulative weight "
                                            "(IndexError in particle_filter.py:219); clamped to NP-1");
    return SLAM_OK;
}

int slam_pfb_timing(slam_pfb* h, double* ms, int64_t* launches) {
    SLAM_ARG_CHECK(h && ms && launches, "slam_pfb_timing: NULL argument");
    *ms = h->last_ms;
    *launches = h->last_launches;
    return SLAM_OK;
}

}  // extern "C"
