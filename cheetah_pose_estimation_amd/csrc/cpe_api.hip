// cpe_api.hip -- C ABI (include/cpe.h) over the HIP kernels.  gfx950 only, no CPU fallback:
// every entry point fails with CPE_NO_DEVICE / CPE_HIP_ERROR when the GPU path is unavailable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include <algorithm>
#include <type_traits>

#include "cpe_kernels.hip"

static thread_local std::string g_err;
static cpe_status fail(cpe_status s, const std::string& m) { g_err = m; return s; }
#define HIPCHK(x)                                                                                         \
    do {                                                                                                  \
        hipError_t e_ = (x);                                                                              \
        if (e_ != hipSuccess) return fail(CPE_HIP_ERROR, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct cpe_handle {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    DevModel hm;                 // host copy
    DevModel* dm = nullptr;      // device copy
    // cpe_create_multi: host copies of all the handle's models (models[0] = hm; empty for cpe_create) -- dm holds them in this order
    std::vector<DevModel> models;
    cpe_options opts;
    // solver workspace (its device buffers are recorded in ws_bufs as they are allocated, see ws_alloc)
    size_t ws_frames = 0; int ws_B = 0;
    std::vector<void**> ws_bufs;
    double *qbuf = nullptr, *gbuf = nullptr, *Bbuf = nullptr, *costbuf = nullptr, *Lbuf = nullptr, *zbuf = nullptr,
           *gtbuf = nullptr, *dgbuf = nullptr, *cmax = nullptr, *mu = nullptr, *gambuf = nullptr;
    SeqState* st = nullptr;
    int* flag = nullptr;
    int* act = nullptr;          // [ws_B] sequences of the current launch window (written by k_build_act)
    int2* rseq = nullptr;        // [ws_B] (model, frames) of every sequence of a cpe_solve_ragged call
    int* n_act = nullptr;        // device word: entries of act in use
    int* poll_host = nullptr;    // pinned host memory: two snapshots of n_act, read without draining the stream
    hipEvent_t poll_ev[2] = {nullptr, nullptr};
    hipEvent_t order_ev = nullptr;   // cpe_stream_wait / cpe_stream_signal
    // per-kernel device time of the last cpe_solve (cpe_profile_enable / cpe_profile_get)
    bool prof = false;
    double prof_ms[CPE_PROFILE_SLOTS] = {0};
    int64_t prof_n[CPE_PROFILE_SLOTS] = {0};
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> prof_spans;
    cpe_eom_options* eom = nullptr;   // device copy of the last cpe_eom_rows options
    cpe_dyn_options* dyn = nullptr;   // device copy of the last cpe_eom_residual options
    // learned priors (config 3)
    DevPriors* pri = nullptr;    // device copy, nullptr without priors
    int gmm_k = 0, gmm_dim = 0, lr_window = 0;
    double* Hlr = nullptr;       // [2][F][pb][nu*nu] off-diagonal Gauss-Newton blocks of the autoregressive prior
    // physics-based model (cpe_solve_kinetic): device options and workspace
    DevKin* dk = nullptr; DevKin hk;  // dk: one entry per model (n_models); hk: host copy of entry 0
    std::vector<DevKin> hks;          // cpe_solve_kinetic_ragged: host copies of every entry
    size_t kws_frames = 0;
    std::vector<void**> kws_bufs;
    double *kmut = nullptr;       // multipliers of the torque boxes [F][2 CPE_MAX_MOTORS] (cpe_solve_kinetic_bounded)
    double *kmus = nullptr;       // multipliers of the box on the residual [F][2 CPE_MAX_NQ] (bound_eom_error)
    double *fbuf = nullptr, *kmu = nullptr, *Jbuf = nullptr, *Abuf = nullptr, *pieces = nullptr, *gTb = nullptr, *dstat = nullptr, *slackb = nullptr,
           *Tbuf = nullptr, *gk = nullptr, *Bk = nullptr, *Hk = nullptr;
    int* pmeta = nullptr;
    // 3D kinematic cost of the physics-based solve (cpe_solve_kinetic_tracked*): per-model tables, their host copies, x* of every frame
    DevTrack* dtrack = nullptr; std::vector<DevTrack> htrack;
    double* xtgt = nullptr; size_t xtgt_frames = 0;
    double* trackH = nullptr; size_t trackH_frames = 0;      // the full-weight form: 2 X^T W_n X of every frame (k_track_block)
    double* covG = nullptr; size_t covG_n = 0;     // cpe_covariance / cpe_band_inverse: the sweep's operands T^T T | G_1 .. G_pb of every column
    // cpe_rate_covariance: the handle's skeletons once more with the link centres as markers (centre-of-mass Jacobian), host and device, in
    // dm's order -- or why they could not be built; and the Jacobians of a call that does not ask for them
    std::vector<DevModel> cmodels; DevModel* dmc = nullptr; std::string com_err;
    double* rateJ = nullptr; size_t rateJ_n = 0;
    int pb = 3;                // half-bandwidth of the normal equations in frames (W with a window-W motion prior, W = 4..6)
};

struct DevBuf {
    double* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, sizeof(double) * (n ? n : 1)); }
};

// The device side of a host-pointer twin.  Every staged array is named once, with its element type and count: in() uploads it, out() remembers
// the download that fetch() enqueues.  The first HIP error sticks in `err` (checked once after the staging and once by fetch's caller) and makes
// the later calls do nothing; the memory is freed on destruction.
struct Staging {
    struct Download { void* host; const void* dev; size_t bytes; };
    hipStream_t stream;
    hipError_t err = hipSuccess;
    std::vector<void*> bufs;
    std::vector<Download> downloads;
    explicit Staging(hipStream_t s) : stream(s) {}
    Staging(const Staging&) = delete;
    ~Staging() { for (void* p : bufs) (void)hipFree(p); }
    template <class T> T* alloc(size_t n) {
        void* p = nullptr;
        if (err == hipSuccess && (err = hipMalloc(&p, sizeof(T) * (n ? n : 1))) == hipSuccess) bufs.push_back(p);
        return static_cast<T*>(p);
    }
    template <class T> T* in(const T* host, size_t n) {          // a null host pointer stays null
        T* d = host ? alloc<T>(n) : nullptr;
        if (d) err = hipMemcpyAsync(d, host, sizeof(T) * n, hipMemcpyHostToDevice, stream);
        return d;
    }
    // the device entry gets its buffer also where the caller does not want the array back (host null: nothing to download)
    template <class T> T* out(T* host, size_t n) {
        T* d = alloc<T>(n);
        if (d && host) downloads.push_back({host, d, sizeof(T) * n});
        return d;
    }
    template <class T> T* out_opt(T* host, size_t n) { return host ? out(host, n) : nullptr; }   // for outputs the device entry takes as null
    hipError_t fetch() {                                          // the downloads, then the one drain of the stream
        for (const Download& d : downloads)
            if (err == hipSuccess) err = hipMemcpyAsync(d.host, d.dev, d.bytes, hipMemcpyDeviceToHost, stream);
        return err == hipSuccess ? (err = hipStreamSynchronize(stream)) : err;
    }
};

// A workspace buffer is allocated through ws_alloc, which records the member's address: ws_free walks that record, so every buffer
// is named once.
template <class T>
static hipError_t ws_alloc(std::vector<void**>& rec, T*& p, size_t n) {
    rec.push_back(reinterpret_cast<void**>(&p));
    return hipMalloc(&p, sizeof(T) * n);
}
static void ws_free(std::vector<void**>& rec) {
    for (void** p : rec) { (void)hipFree(*p); *p = nullptr; }      // (hipFree of a null pointer does nothing)
    rec.clear();
}

static double host_rho0(double a, double b, double c) {
    // rho(0) of acinoset_misc.py:2001-2015
    auto sg = [](double t) { return 1.0 / (1.0 + std::exp(t)); };   // s(t, 0) = 1/(1+e^{t})
    const double sa = sg(a), sb = sg(b), sc = sg(c);
    const double cb = c - b, w = c / cb;
    return (sa - sb) * (-0.5 * a * a) + (sb - sc) * (a * b - 0.5 * a * a + 0.5 * a * cb * (1.0 - w * w)) +
           sc * (a * b - 0.5 * a * a + 0.5 * a * cb);
}

// The chain vectors of one marker (DevModel::chain_vec) from the root down: in the frame of link chain_link[i], where the next link of the chain
// attaches, and for the last link the marker's offset.  Linear in (attach, marker_off): given the derivatives of the two tables by a length
// scale, the same loop returns the derivatives of the chain vectors (cpe_scale_system).
static void chain_vectors(const int32_t* chain_link, int n, const double (*attach)[3], const double* marker_off, double (*vec)[3]) {
    for (int i = 0; i < n; i++) {
        const double* v = i == n - 1 ? marker_off : attach[chain_link[i + 1]];
        for (int d = 0; d < 3; d++) vec[i][d] = v[d];
    }
}

// gather = false: without the gather lists of H and g (a model that only serves the reduced marker columns, build_com_model)
static cpe_status build_model(const cpe_skeleton* s, const cpe_camera* cams, int C, const cpe_options* o, DevModel& m, bool gather = true) {
    memset(&m, 0, sizeof(m));
    if (s->n_links < 1 || s->n_links > CPE_MAX_LINKS || s->n_markers < 1 || s->n_markers > CPE_MAX_MARKERS ||
        s->n_joints < 0 || s->n_joints > CPE_MAX_JOINTS || s->n_bounds < 0 || s->n_bounds > CPE_MAX_BOUNDS ||
        C < 1 || C > CPE_MAX_CAMS)
        return fail(CPE_BAD_ARG, "skeleton / camera counts out of range");
    const int nl = s->n_links, nq = 3 + 3 * nl, L = s->n_markers;
    m.nl = nl; m.L = L; m.C = C; m.nq = nq; m.nj = s->n_joints; m.nb = s->n_bounds;
    m.h = o->h; m.ih2 = 1.0 / (o->h * o->h);
    m.loss_a = o->loss_a; m.loss_b = o->loss_b; m.loss_c = o->loss_c;
    m.bound_penalty = o->bound_penalty; m.curvature = o->curvature;
    m.rho0 = host_rho0(o->loss_a, o->loss_b, o->loss_c);
    if (!(o->h > 0)) return fail(CPE_BAD_ARG, "options.h must be > 0");
    double mt = 0;
    for (int i = 0; i < nl; i++) {
        if (s->parent[i] >= i) return fail(CPE_BAD_ARG, "links must be ordered parents first");
        m.parent[i] = s->parent[i];
        for (int d = 0; d < 3; d++) { m.attach[i][d] = s->attach[i][d]; m.com[i][d] = s->com[i][d]; }
        m.mass[i] = s->mass[i]; mt += s->mass[i];
    }
    m.inv_total_mass = mt > 0 ? 1.0 / mt : 0.0;
    for (int c = 0; c < C; c++) m.cam[c] = cams[c];

    // dependent / independent split
    for (int p = 0; p < nq; p++) { m.u_of_q[p] = -1; m.dep_of_q[p] = -1; }
    int ndep = 0;
    std::vector<int> joint_of_child(nl, -1);
    for (int j = 0; j < s->n_joints; j++) {
        const int p = s->joint_parent[j], c = s->joint_child[j], k = s->joint_kind[j];
        if (p < 0 || p >= nl || c <= p || c >= nl || joint_of_child[c] >= 0) return fail(CPE_BAD_ARG, "bad joint");
        m.joint_parent[j] = p; m.joint_child[j] = c; m.joint_kind[j] = k;
        joint_of_child[c] = j;
        m.joint_dep0[j] = ndep;
        m.dep_joint[ndep] = j;
        m.dep_of_q[3 + 3 * c] = ndep++;
        if (k == CPE_JOINT_REVOLUTE_Y) { m.dep_joint[ndep] = j; m.dep_of_q[3 + 3 * c + 2] = ndep++; }
        else if (k != CPE_JOINT_HOOKE_YZ) return fail(CPE_BAD_ARG, "unknown joint kind");
        if (ndep > CPE_MAX_DEP) return fail(CPE_BAD_ARG, "too many dependent angles");
    }
    m.ndep = ndep;
    int nu = 0;
    for (int p = 0; p < nq; p++)
        if (m.dep_of_q[p] < 0) { if (nu >= CPE_NX) return fail(CPE_BAD_ARG, "more than 28 independent dofs"); m.indep[nu] = p; m.u_of_q[p] = nu++; }
    m.nu = nu;
    if (nu != CPE_NX) return fail(CPE_BAD_ARG, "the solver is built for exactly 28 independent dofs");
    for (int p = 0; p < nq; p++)
        if (m.dep_of_q[p] >= 0 && s->motion_w[p] != 0.0) return fail(CPE_BAD_ARG, "motion weight on a dependent angle");
    for (int k = 0; k < nu; k++) {
        const int p = m.indep[k];
        m.motion_w_u[k] = s->motion_w[p];
        m.rel_sign_u[k] = s->rel_ref[p] < 0 ? 1.0 : s->rel_sign[p];
        m.rel_ref_u[k] = s->rel_ref[p] < 0 ? -1 : m.u_of_q[s->rel_ref[p]];
        if (s->rel_ref[p] >= 0 && m.rel_ref_u[k] < 0) return fail(CPE_BAD_ARG, "relative angle references a dependent dof");
    }
    // joint bodies and S column layout
    m.n_srow = 0;
    for (int r = 0; r < CPE_MAX_DEP; r++) m.srow[r] = -1;
    for (int j = 0; j < s->n_joints; j++) {
        const int p = m.joint_parent[j], c = m.joint_child[j], r = m.joint_dep0[j];
        if (m.joint_kind[j] == CPE_JOINT_REVOLUTE_Y) {
            int body = p;
            const int jp = joint_of_child[p];
            if (jp >= 0) {
                if (m.joint_kind[jp] != CPE_JOINT_REVOLUTE_Y) return fail(CPE_BAD_ARG, "revolute joint below a hooke joint is not supported");
                body = m.joint_body[jp];
            }
            m.joint_body[j] = body;
            for (int a = 0; a < 3; a++)
                if (m.u_of_q[3 + 3 * body + a] < 0) return fail(CPE_BAD_ARG, "revolute chain must hang off a link with independent angles");
            if (m.u_of_q[3 + 3 * c + 1] < 0) return fail(CPE_BAD_ARG, "theta of a revolute child must be independent");
            for (int rr = r; rr < r + 2; rr++) {
                m.scol_n[rr] = 4; m.dep_level[rr] = 0;
                for (int a = 0; a < 3; a++) m.scol[rr][a] = m.u_of_q[3 + 3 * body + a];
                m.scol[rr][3] = m.u_of_q[3 + 3 * c + 1];
            }
        } else {
            m.joint_body[j] = p;
            m.srow[r] = m.n_srow++;
            int n = 0;
            auto add = [&](int col, int kind, int ang, int chain) -> bool {
                for (int e = 0; e < n; e++)
                    if (m.scol[r][e] == col) { if (chain >= 0) m.hk_chain[r][e] = (int16_t)chain; else { m.hk_kind[r][e] = (int8_t)kind; m.hk_ang[r][e] = (int8_t)ang; } return true; }
                if (n >= CPE_MAX_SCOL) return false;
                m.scol[r][n] = col; m.hk_kind[r][n] = (int8_t)kind; m.hk_ang[r][n] = (int8_t)ang; m.hk_chain[r][n] = (int16_t)chain; n++;
                return true;
            };
            if (m.u_of_q[3 + 3 * c + 1] < 0 || m.u_of_q[3 + 3 * c + 2] < 0) return fail(CPE_BAD_ARG, "theta/psi of a hooke child must be independent");
            bool ok = add(m.u_of_q[3 + 3 * c + 1], 0, 1, -1) && add(m.u_of_q[3 + 3 * c + 2], 0, 2, -1);
            m.dep_level[r] = 0;
            for (int a = 0; a < 3 && ok; a++) {
                const int pq = 3 + 3 * p + a;
                if (m.u_of_q[pq] >= 0) ok = add(m.u_of_q[pq], 1, a, -1);
                else {
                    if (a != 0) return fail(CPE_BAD_ARG, "hooke parent with dependent theta/psi is not supported");
                    const int pr = m.dep_of_q[pq];
                    if (m.dep_level[pr] != 0 || m.joint_kind[m.dep_joint[pr]] != CPE_JOINT_HOOKE_YZ)
                        return fail(CPE_BAD_ARG, "hooke chains deeper than two are not supported");
                    m.dep_level[r] = 1;
                    for (int e = 0; e < m.scol_n[pr] && ok; e++) ok = add(m.scol[pr][e], 2, 0, m.srow[pr] * CPE_MAX_SCOL + e);
                }
            }
            if (!ok) return fail(CPE_BAD_ARG, "too many columns in a hooke row");
            m.scol_n[r] = n;
        }
    }
    // revolute (leg) links: R_c = R_body Ry(alpha_c)
    std::vector<int> rev_of_link(nl, -1);
    m.nrev = 0;
    for (int p = 0; p < nq; p++) m.euler_rev[p] = -1;
    for (int k = 0; k < nu; k++) { m.rev_of_u[k] = -1; m.ucoord_src[k] = m.indep[k]; m.bodyang_j[k] = -1; m.bodyang_legs_n[k] = 0; }
    for (int j = 0; j < s->n_joints; j++)
        if (m.joint_kind[j] == CPE_JOINT_REVOLUTE_Y) {
            const int r = m.nrev++, c = m.joint_child[j], Bk = m.joint_body[j];
            rev_of_link[c] = r;
            m.rev_child[r] = c; m.rev_body[r] = Bk; m.rev_u[r] = m.u_of_q[3 + 3 * c + 1];
            m.rev_of_u[m.rev_u[r]] = r; m.euler_rev[3 + 3 * c + 1] = r;
            for (int a = 0; a < 3; a++) {
                const int kb = m.u_of_q[3 + 3 * Bk + a];
                m.rev_body_u[r][a] = kb; m.bodyang_j[kb] = a;
                m.bodyang_legs[kb][m.bodyang_legs_n[kb]++] = r;
            }
        }
    m.ns = nq + m.nrev;
    for (int k = 0; k < nu; k++) {
        const int r = m.rev_of_u[k];
        m.ucost[k] = r < 0 ? m.indep[k] : ((3 + 3 * m.rev_body[r] + 1) | (nq + r + 1) << 8);      // trunk: its Euler angle; leg: theta_B + alpha_r
    }
    if (m.nrev > LM_MAX_REV) return fail(CPE_BAD_ARG, "more than 12 leg links");
    for (int k = 0; k < nu; k++) if (m.bodyang_legs_n[k] > LM_MAX_LEGS) return fail(CPE_BAD_ARG, "more than 6 leg links on one body");
    for (int r = 0; r < m.nrev; r++) m.ucoord_src[m.rev_u[r]] = nq + r;
    m.n_trunk = 0;
    for (int i = 0; i < nl; i++) { m.trunk_slot[i] = -1; if (rev_of_link[i] < 0) { m.trunk_slot[i] = m.n_trunk; m.trunk_link[m.n_trunk++] = i; } }
    // marker chains and Jacobian slots
    int S = 0, mct = 0, ss = 0, sv = 0;
    for (int l = 0; l < L; l++) {
        int chain[CPE_MAX_LINKS], n = 0, k = s->marker_link[l];
        if (k < 0 || k >= nl) return fail(CPE_BAD_ARG, "bad marker link");
        while (k >= 0) { chain[n++] = k; k = s->parent[k]; }
        if (n > CPE_MAX_CHAIN) return fail(CPE_BAD_ARG, "marker chain too long");
        m.chain_len[l] = n;
        for (int i = 0; i < n; i++) m.chain_link[l][i] = chain[n - 1 - i];
        chain_vectors(m.chain_link[l], n, s->attach, s->marker_off[l], m.chain_vec[l]);
        m.slot_off[l] = S;
        if (S + 3 + 3 * n > CPE_MAX_SLOTS) return fail(CPE_BAD_ARG, "too many Jacobian slots");
        for (int d = 0; d < 3; d++) { m.slot_marker[S] = l; m.slot_dof[S] = d; m.slot_cpos[S] = -1; m.slot_ang[S] = 0; S++; }
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) { m.slot_marker[S] = l; m.slot_dof[S] = 3 + 3 * m.chain_link[l][i] + a; m.slot_cpos[S] = i; m.slot_ang[S] = a; S++; }
        // ---- solver side: reduced columns of this marker.  Leg links are rotations of their body about its
        // y axis (R_c = R_B Ry(alpha_c)); everything the legs contribute is a body matrix times a body-frame
        // vector that depends on the alphas ("dynamic vectors").
        int nc = 0;
        auto col_index = [&](int col) -> int {
            for (int e = 0; e < nc; e++) if (m.mcol[l][e] == col) return e;
            if (nc >= CPE_MAX_MCOL) return -1;
            m.mcol[l][nc] = col; m.term_n[l][nc] = 0; return nc++;
        };
        auto add_term = [&](int col, int slot, int sidx) -> bool {
            const int e = col_index(col);
            if (e < 0 || m.term_n[l][e] >= CPE_MAX_TERMS) return false;
            m.term_slot[l][e][m.term_n[l][e]] = (int16_t)slot; m.term_s[l][e][m.term_n[l][e]] = (int16_t)sidx; m.term_n[l][e]++;
            return true;
        };
        auto new_slot = [&](int moff, int vdyn, const double* v) -> int {
            if (ss >= CPE_MAX_SLOTS) return -1;
            m.ss_moff[ss] = moff; m.ss_vdyn[ss] = vdyn;
            for (int d = 0; d < 3; d++) m.ss_vec[ss][d] = v ? v[d] : 0.0;
            return ss++;
        };
        bool ok = true;
        const double ex[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int d = 0; d < 3 && ok; d++) { const int sl = new_slot(-1, -1, ex[d]); ok = sl >= 0 && add_term(m.u_of_q[d], sl, -1); }
        int n_trunk_chain = 0;
        while (n_trunk_chain < n && rev_of_link[m.chain_link[l][n_trunk_chain]] < 0) n_trunk_chain++;
        m.pc_len[l] = n_trunk_chain; m.pw_id[l] = -1; m.pw_body[l] = 0;
        for (int i = 0; i < n_trunk_chain && ok; i++) {
            const int link = m.chain_link[l][i];
            m.pc_link[l][i] = link;
            for (int d = 0; d < 3; d++) m.pc_vec[l][i][d] = m.chain_vec[l][i][d];
            for (int a = 0; a < 3 && ok; a++) {
                const int sl = new_slot(9 * (4 * m.trunk_slot[link] + 1 + a), -1, m.chain_vec[l][i]);
                const int p = 3 + 3 * link + a;
                if (sl < 0) { ok = false; break; }
                if (m.u_of_q[p] >= 0) ok = add_term(m.u_of_q[p], sl, -1);
                else { const int r = m.dep_of_q[p]; for (int e = 0; e < m.scol_n[r] && ok; e++) ok = m.srow[r] >= 0 && add_term(m.scol[r][e], sl, m.srow[r] * CPE_MAX_SCOL + e); }
            }
        }
        if (n_trunk_chain < n && ok) {
            const int Bk = m.chain_link[l][n_trunk_chain - 1];
            const int nleg = n - n_trunk_chain;
            if (nleg > 3 || sv + 1 + nleg > CPE_MAX_SDYN) return fail(CPE_BAD_ARG, "leg chain too long");
            const int wid = sv++;
            m.sv_kind[wid] = 0; m.sv_cnt[wid] = nleg;
            for (int i = 0; i < nleg; i++) {
                const int link = m.chain_link[l][n_trunk_chain + i];
                if (rev_of_link[link] < 0 || m.rev_body[rev_of_link[link]] != Bk) return fail(CPE_BAD_ARG, "leg links must follow their body in the marker chain");
                m.sv_rev[wid][i] = rev_of_link[link];
                for (int d = 0; d < 3; d++) m.sv_vec[wid][i][d] = m.chain_vec[l][n_trunk_chain + i][d];
            }
            m.pw_id[l] = wid; m.pw_body[l] = Bk;
            for (int a = 0; a < 3 && ok; a++) {           // body angles act on the whole leg vector
                const int sl = new_slot(9 * (4 * m.trunk_slot[Bk] + 1 + a), wid, nullptr);
                ok = sl >= 0 && add_term(m.u_of_q[3 + 3 * Bk + a], sl, -1);
            }
            for (int i = 0; i < nleg && ok; i++) {        // alpha of each leg link
                const int did = sv++;
                m.sv_kind[did] = 1; m.sv_cnt[did] = 1; m.sv_rev[did][0] = m.sv_rev[wid][i];
                for (int d = 0; d < 3; d++) m.sv_vec[did][0][d] = m.sv_vec[wid][i][d];
                const int sl = new_slot(9 * (4 * m.trunk_slot[Bk]), did, nullptr);
                ok = sl >= 0 && add_term(m.rev_u[m.sv_rev[wid][i]], sl, -1);
            }
        }
        if (!ok) return fail(CPE_BAD_ARG, "marker depends on too many reduced dofs");
        m.mcol_n[l] = nc; m.mcol_off[l] = mct;
        for (int e = 0; e < nc; e++) { m.mc_marker[mct] = (int16_t)l; m.mc_j[mct] = (int16_t)e; mct++; }
    }
    m.ss_n = ss; m.sv_n = sv;
    m.slot_off[L] = S;
    // Row alignment: J is [C][S][2] doubles, so a camera row is 16 S bytes.  S = 270 (the reference's 24 markers) makes every
    // other row start 32 B off a 64-byte line and measured 9 % slower than S = 276; pad S to a multiple of 4 with slots
    // of marker 0 and a dof outside its chain (structurally zero: the kernel stores 0 there, as the dense Jacobian has).
    for (int d = s->n_links * 3 + 2; (S & 3) && d >= 3; d--) {
        bool in_chain = false;
        for (int i = 0; i < m.chain_len[0]; i++) in_chain |= (d - 3) / 3 == m.chain_link[0][i];
        if (in_chain) continue;
        if (S >= CPE_MAX_SLOTS) return fail(CPE_BAD_ARG, "too many Jacobian slots");
        m.slot_marker[S] = 0; m.slot_dof[S] = d; m.slot_cpos[S] = -2; m.slot_ang[S] = 0; S++;
    }
    m.S = S; m.mcol_off[L] = mct; m.mc_total = mct;
    if (S > 5 * WAVE) return fail(CPE_BAD_ARG, "more than 320 Jacobian slots");
    {   // flat term list of the reduced marker columns (see cpe_model.h)
        m.tl_n = 0;
        for (int l = 0; l < L; l++)
            for (int e = 0; e < m.mcol_n[l]; e++)
                for (int k = 0; k < m.term_n[l][e]; k++) {
                    if (m.tl_n >= CPE_MAX_TL) return fail(CPE_BAD_ARG, "too many marker-column terms");
                    const int sl = m.term_slot[l][e][k], si = m.term_s[l][e][k], item = m.mcol_off[l] + e;
                    if (item >= 1024 || si + 1 >= 1024 || m.ss_vdyn[sl] + 1 >= 1024) return fail(CPE_BAD_ARG, "marker-column term out of range");
                    auto& T = m.tl[m.tl_n++];
                    T.w0 = item | ((si + 1) << 10) | ((m.ss_vdyn[sl] + 1) << 20);
                    T.moff = m.ss_moff[sl];
                    for (int d = 0; d < 3; d++) T.v[d] = m.ss_vec[sl][d];
                }
    }
    if (gather) {   // gather lists for H and g (see cpe_model.h)
        const int nu_ = m.nu;
        std::vector<std::vector<uint32_t>> by_entry(nu_ * nu_);
        for (int l = 0; l < L; l++)
            for (int i = 0; i < m.mcol_n[l]; i++)
                for (int j = 0; j <= i; j++) {
                    int a = m.mcol[l][i], b = m.mcol[l][j];
                    if (a < b) std::swap(a, b);
                    by_entry[a * nu_ + b].push_back((uint32_t)(m.mcol_off[l] + i) | ((uint32_t)(m.mcol_off[l] + j) << 8) | ((uint32_t)l << 16));
                }
        std::vector<int> order;
        for (int e = 0; e < nu_ * nu_; e++) if (!by_entry[e].empty()) order.push_back(e);
        for (auto& w : m.h_covered) w = 0;
        for (int e : order) { const int a = e / nu_, b = e % nu_; for (int t : {a * nu_ + b, b * nu_ + a}) m.h_covered[t >> 5] |= 1u << (t & 31); }
        std::sort(order.begin(), order.end(), [&](int x, int y) { return by_entry[x].size() != by_entry[y].size() ? by_entry[x].size() > by_entry[y].size() : x < y; });
        int load[64] = {0};
        for (int e : order) {
            int best = 0;
            for (int ln = 1; ln < 64; ln++) if (load[ln] < load[best]) best = ln;
            if (load[best] + (int)by_entry[e].size() > CPE_MAX_HG) return fail(CPE_BAD_ARG, "normal-matrix gather list too long");
            const uint32_t ab = (uint32_t)(((e / nu_) << 5) | (e % nu_));
            for (size_t k = 0; k < by_entry[e].size(); k++) m.hg_code[load[best] + k][best] = by_entry[e][k] | (k == 0 ? 1u << 21 : 0u) | (ab << 22);
            load[best] += (int)by_entry[e].size();
        }
        m.hg_max = 0;
        for (int ln = 0; ln < 64; ln++) { m.hg_cnt[ln] = load[ln]; if (load[ln] > m.hg_max) m.hg_max = load[ln]; }
        for (int k = 0; k < nu_; k++) m.gg_cnt[k] = 0;
        for (int l = 0; l < L; l++)
            for (int i = 0; i < m.mcol_n[l]; i++) {
                const int a = m.mcol[l][i];
                if (m.gg_cnt[a] >= CPE_MAX_GG) return fail(CPE_BAD_ARG, "gradient gather list too long");
                m.gg_code[m.gg_cnt[a]++][a] = (uint16_t)((m.mcol_off[l] + i) | (l << 8));
            }
    }
    {   // per-lane tables of k_frame_normal with resolved indices (see cpe_model.h)
        m.hk_n = 0;
        for (int r = 0; r < m.ndep; r++) {
            const int j = m.dep_joint[r];
            if (m.joint_kind[j] != CPE_JOINT_HOOKE_YZ || m.srow[r] < 0) continue;
            for (int jc = 0; jc < m.scol_n[r]; jc++) {
                if (m.hk_n >= 64) return fail(CPE_BAD_ARG, "more than 64 entries in the hooke rows of S");
                const int ps = m.trunk_slot[m.joint_parent[j]], cs = m.trunk_slot[m.joint_child[j]];
                if (ps < 0 || cs < 0 || ps >= 64 || cs >= 64) return fail(CPE_BAD_ARG, "hooke joint between leg links");
                m.hk_w[m.hk_n][0] = ps | (cs << 6) | ((m.hk_kind[r][jc] & 3) << 12) | ((m.hk_ang[r][jc] & 3) << 14) | ((m.dep_level[r] & 1) << 16);
                m.hk_w[m.hk_n][1] = (m.hk_chain[r][jc] + 1) | ((m.srow[r] * CPE_MAX_SCOL + jc) << 16);
                m.hk_n++;
            }
        }
        m.hj_n = 0;
        for (int j = 0; j < s->n_joints; j++)
            if (m.joint_kind[j] == CPE_JOINT_HOOKE_YZ) {
                if (m.hj_n >= 64) return fail(CPE_BAD_ARG, "more than 64 hooke joints");
                m.fn_lane[m.hj_n++][0] = m.joint_parent[j] | (m.joint_child[j] << 8) | ((m.dep_of_q[3 + 3 * m.joint_parent[j]] >= 0 ? 1 : 0) << 16);
            }
        for (int t = 0; t < 4 * m.n_trunk && t < 64; t++) m.fn_lane[t][1] = m.trunk_link[t >> 2];     // (nrev <= 16 and sv_n <= 48 by the table sizes)
        for (int r = 0; r < m.nrev; r++) m.fn_lane[r][2] = m.rev_body[r] | (m.rev_child[r] << 8) | (m.trunk_slot[m.rev_body[r]] << 16);
        for (int t = 0; t < m.sv_n; t++) m.fn_lane[t][3] = m.sv_kind[t] | (m.sv_cnt[t] << 2) | (m.sv_rev[t][0] << 4) | (m.sv_rev[t][1] << 10) | (m.sv_rev[t][2] << 16);
        for (int l = 0; l < L; l++) {
            for (int i = 0; i < m.pc_len[l]; i++) m.pc_off[l][i] = 36 * m.trunk_slot[m.pc_link[l][i]];
            m.pw_off[l] = m.pw_id[l] >= 0 ? 36 * m.trunk_slot[m.pw_body[l]] : 0;
        }
    }
    for (int bnd = 0; bnd < s->n_bounds; bnd++) {
        const int a = s->bound_a[bnd], bb = s->bound_b[bnd];
        if (a < 0 || a >= nq || bb >= nq || m.u_of_q[a] < 0 || (bb >= 0 && m.u_of_q[bb] < 0))
            return fail(CPE_BAD_ARG, "bounds must act on independent dofs");
        m.bound_ua[bnd] = m.u_of_q[a]; m.bound_ub[bnd] = bb < 0 ? -1 : m.u_of_q[bb];
        m.bound_lo[bnd] = s->bound_lo[bnd]; m.bound_up[bnd] = s->bound_up[bnd];
        // (state index of the value, + 1 of the second addend or 0) for each side: a leg pitch is theta_B + alpha (ucost)
        const int ca = m.ucost[m.u_of_q[a]], cb = bb < 0 ? 0 : m.ucost[m.u_of_q[bb]];
        m.bnd_q[bnd] = (ca & 255) | (bb < 0 ? 0 : ((cb & 255) + 1) << 8) | ((ca >> 8) & 255) << 16 | (bb < 0 ? 0 : ((cb >> 8) & 255)) << 24;
    }
    return CPE_OK;
}

// The skeleton once more with its link centres as markers -- marker i = the centre of mass of link i -- so that the reduced marker columns of this
// model are d (link centre) / d u: the centre-of-mass Jacobian is their mass-weighted mean (k_point_jac).  Appends to `out`; a skeleton whose link
// centres do not fit the marker tables leaves the reason in `err` and `out` empty: only the centre-of-mass outputs of cpe_rate_covariance need it.
static void build_com_model(const cpe_skeleton* s, const cpe_camera* cams, int C, const cpe_options* o, std::vector<DevModel>& out, std::string& err) {
    if (!err.empty()) return;
    cpe_skeleton c = *s;
    c.n_markers = s->n_links;
    for (int i = 0; i < s->n_links && i < CPE_MAX_MARKERS; i++) {
        c.marker_link[i] = i;
        for (int d = 0; d < 3; d++) c.marker_off[i][d] = s->com[i][d];
    }
    const std::string keep = g_err;
    out.emplace_back();
    if (build_model(&c, cams, C, o, out.back(), false) != CPE_OK) { err = g_err; out.clear(); }
    g_err = keep;
}

// the plain variant of k_frame_normal (no Gaussian-mixture prior, no shutter delay) writes H straight to HBM and needs 6 KB less LDS per wave
template <bool RAGGED = false>
static auto frame_normal(bool plain) { return plain ? k_frame_normal<true, RAGGED> : k_frame_normal<false, RAGGED>; }
static size_t lds_fk(const DevModel& m) { return sizeof(double) * (m.nq + 6 * m.nl + 36 * m.nl + 3 * m.L + 23 * m.C); }
static size_t lds_normal(const DevModel& m, int gmm_k = 0, int gmm_dim = 0, bool shutter = false) {
    // g (and, unless the plain variant writes H straight to HBM, H | g) overlay the S rows, which are dead once Dp is built
    const bool plain = gmm_k == 0 && !shutter;
    size_t ov = CPE_MAX_SCOL * m.n_srow, hg = plain ? m.nu : m.nu * m.nu + m.nu;
    size_t camov = 6 * m.nl + 2 * m.nrev + 36 * m.n_trunk;   // sin / cos tables + trunk rotations, later the staged cameras (sizeof(cpe_camera) = 22 doubles each)
    if (camov < (size_t)22 * m.C) camov = (size_t)22 * m.C;
    size_t n = m.ns + camov + 3 * m.L + 3 * m.sv_n + GAM_STRIDE * m.nrev + (ov > hg ? ov : hg) +
               9 * m.L + 3 * m.mc_total;
    if (gmm_k > 0) n += CPE_NX + gmm_k * gmm_dim + CPE_MAX_GMM + CPE_NX;          // x | P_k (x - mu_k) | log p_k | gradient in x
    if (shutter) n += 15 * m.C + 6 * m.L + 6;          // shift | coefficients | rc | Mc per camera, M1 per marker, M2
    return sizeof(double) * n;
}
// k_frame_tracked (cpe_tracked.hip.inc): state | sin / cos | trunk rotations | Gamma | weighted residual | H | g, then the pose prior's scratch
template <bool RAGGED = false>
static auto frame_tracked(bool gmm, bool full = false) {
    if (full) return gmm ? k_frame_tracked<true, RAGGED, true> : k_frame_tracked<false, RAGGED, true>;
    return gmm ? k_frame_tracked<true, RAGGED> : k_frame_tracked<false, RAGGED>;
}
static size_t lds_tracked(const DevModel& m, int gmm_k, int gmm_dim) {
    size_t n = m.ns + 6 * m.nl + 2 * m.nrev + 36 * m.n_trunk + GAM_STRIDE * m.nrev + m.nu + m.nu * m.nu + m.nu;
    if (gmm_k > 0) n += CPE_NX + gmm_k * gmm_dim + CPE_MAX_GMM + CPE_NX;          // x | P_k (x - mu_k) | log p_k | gradient in x
    return sizeof(double) * n;
}
// the dynamic LDS a ragged launch needs: the most any of the handle's models needs
template <class Fn>
static size_t lds_all(const cpe_handle* h, Fn&& lds) {
    size_t n = lds(h->hm);
    for (const DevModel& m : h->models) n = std::max(n, lds(m));
    return n;
}
static size_t lds_normal_all(const cpe_handle* h) { return lds_all(h, [h](const DevModel& m) { return lds_normal(m, h->gmm_k, h->gmm_dim); }); }
// The dynamic LDS of a launch: with the ragged table rg what every model of the handle fits in (no shutter delay there), without it what the
// handle's first model needs
static size_t lds_fk(const cpe_handle* h, const RaggedArgs* rg) { return rg ? lds_all(h, [](const DevModel& m) { return lds_fk(m); }) : lds_fk(h->hm); }
static size_t lds_normal(const cpe_handle* h, const RaggedArgs* rg, bool shutter = false) {
    return rg ? lds_normal_all(h) : lds_normal(h->hm, h->gmm_k, h->gmm_dim, shutter);
}
static size_t lds_tracked(const cpe_handle* h, const RaggedArgs* rg) {
    return rg ? lds_all(h, [h](const DevModel& m) { return lds_tracked(m, h->gmm_k, h->gmm_dim); }) : lds_tracked(h->hm, h->gmm_k, h->gmm_dim);
}
static int n_models(const cpe_handle* h) { return h->models.empty() ? 1 : (int)h->models.size(); }
static int cams_max(const cpe_handle* h) {
    int c = h->hm.C;
    for (const DevModel& m : h->models) c = std::max(c, m.C);
    return c;
}

extern "C" {

const char* cpe_last_error(void) { return g_err.c_str(); }

void cpe_default_options(cpe_options* o) {
    o->h = 1.0 / 120.0; o->loss_a = 3.0; o->loss_b = 10.0; o->loss_c = 20.0; o->cost_scale = 1e-3;
    o->bound_penalty = 1e4; o->bound_tol = 1e-6; o->lambda0 = 1e-4; o->tol_step = 1e-8; o->tol_cost = 1e-9; o->max_iter = 200;
    o->curvature = 0; o->max_outer = 8; o->_pad = 0;
}

void cpe_destroy(cpe_handle* h);
// models: the models cpe_create_multi has built already (h->hm is models[0]), or null: build the one of (skel, cams, opts)
static cpe_status create_impl(cpe_handle* h, const cpe_skeleton* skel, const cpe_camera* cams, int32_t n_cams, const cpe_options* opts,
                              const cpe_priors* priors, bool use_pri, const std::vector<DevModel>* models = nullptr) {
    const int device = h->device;
    if (models) { h->models = *models; h->hm = h->models[0]; }
    else {
        if (cpe_status s = build_model(skel, cams, n_cams, opts, h->hm); s != CPE_OK) return s;
        build_com_model(skel, cams, n_cams, opts, h->cmodels, h->com_err);
    }
    HIPCHK(hipSetDevice(device));
    {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        // dynamic LDS above 64 KiB needs an explicit opt-in per kernel
        const void* ks[] = {(const void*)&k_resjac<true, 4, 3, 2>, (const void*)&k_resjac<false, 4, 3, 2>,
                            (const void*)&k_resjac<true, 4, 4, 2>, (const void*)&k_resjac<false, 4, 4, 2>,
                            (const void*)&k_dyn_eval<>, (const void*)&k_dyn_assemble<>, (const void*)&k_dyn_schur<>, (const void*)&k_dyn_jac<>,
                            (const void*)&k_dyn_eval<true>, (const void*)&k_dyn_assemble<true>, (const void*)&k_dyn_schur<true>, (const void*)&k_dyn_jac<true>,
                            (const void*)&k_force_cov<>, (const void*)&k_force_cov<true>, (const void*)&k_force_sample<>, (const void*)&k_force_sample<true>};
        for (const void* k : ks) {         // all of the CU's 160 KiB that the kernel's static LDS leaves (k_dyn_schur<*> holds a word of its own)
            hipFuncAttributes fa;
            HIPCHK(hipFuncGetAttributes(&fa, k));
            HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)fa.sharedSizeBytes));
        }
    }
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) HIPCHK(hipEventCreateWithFlags(&h->poll_ev[i], hipEventDisableTiming));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->poll_host), 2 * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipMalloc(&h->n_act, sizeof(int)));
    HIPCHK(hipMalloc(&h->dm, sizeof(DevModel) * n_models(h)));
    HIPCHK(hipMemcpy(h->dm, h->models.empty() ? &h->hm : h->models.data(), sizeof(DevModel) * n_models(h), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&h->flag, sizeof(int)));
    if (!h->cmodels.empty()) {
        HIPCHK(hipMalloc(&h->dmc, sizeof(DevModel) * h->cmodels.size()));
        HIPCHK(hipMemcpy(h->dmc, h->cmodels.data(), sizeof(DevModel) * h->cmodels.size(), hipMemcpyHostToDevice));
    }
    if (use_pri) {
        if (h->hm.nu != CPE_NX) return fail(CPE_BAD_ARG, "learned priors need the 28 relative angles of the reference's skeleton");
        if (priors->gmm_k > 0 && priors->gmm_dim > h->hm.nu) return fail(CPE_BAD_ARG, "pose prior dimension exceeds the number of relative angles");
        std::vector<DevPriors> hp(1);
        DevPriors& P = hp[0];
        memset(&P, 0, sizeof(P));
        P.p = *priors;
        const int W = priors->lr_window, nu = CPE_NX;
        if (W > 0) {
            // K_t[p][j]: lag blocks of slack = sum_t K_t x_{n-W+t} - b
            auto K = [&](int t, int p2, int j) -> double { return t == W ? (p2 == j ? 1.0 : 0.0) : -priors->lr_coef[p2][t * nu + j]; };
            for (int ta = 0; ta <= W; ta++)
                for (int tb = 0; tb <= ta; tb++)
                    for (int i = 0; i < nu; i++)
                        for (int j = 0; j < nu; j++) {
                            double a = 0.0;
                            for (int p2 = 0; p2 < nu; p2++) a += K(ta, p2, i) * priors->lr_w[p2] * K(tb, p2, j);
                            P.lr_PK[ta][tb][i * nu + j] = 2.0 * a;
                        }
            for (int k = 0; k <= W; k++)
                for (int ta = k; ta <= W; ta++)
                    for (int e = 0; e < nu * nu; e++) P.lr_HI[k][e] += P.lr_PK[ta][ta - k][e];
            for (int f = 0; f < W * nu; f++) {
                bool any = false;
                for (int p2 = 0; p2 < nu; p2++) { P.lr_coefT[f][p2] = priors->lr_coef[p2][f]; any = any || priors->lr_coef[p2][f] != 0.0; }
                if (any) P.lr_feat[P.lr_nf++] = (uint8_t)f;
            }
        }
        // X' = dx/du: x_k = sign_k (c_k - c_ref), c = the reduced coordinate itself or, for a leg link, theta_B + alpha_c (cost pitch)
        const DevModel& hm = h->hm;
        for (int i = 0; i < nu; i++)
            for (int side = 0; side < 2; side++) {
                const int kk = side == 0 ? i : hm.rel_ref_u[i];
                if (kk < 0) continue;
                const double sgn = side == 0 ? hm.rel_sign_u[i] : -hm.rel_sign_u[i];
                P.Xc[i][kk] += sgn;
                const int r = hm.rev_of_u[kk];
                if (r >= 0) P.Xc[i][hm.rev_body_u[r][1]] += sgn;
            }
        // out = X'^T A X' (A, out row-major nu x nu), fixed summation order
        auto to_u = [&](const double* A, double* out) {
            std::vector<double> T((size_t)nu * nu);
            for (int r2 = 0; r2 < nu; r2++)
                for (int j = 0; j < nu; j++) { double a = 0.0; for (int c = 0; c < nu; c++) a += A[r2 * nu + c] * P.Xc[c][j]; T[(size_t)r2 * nu + j] = a; }
            for (int i = 0; i < nu; i++)
                for (int j = 0; j < nu; j++) { double a = 0.0; for (int r2 = 0; r2 < nu; r2++) a += P.Xc[r2][i] * T[(size_t)r2 * nu + j]; out[i * nu + j] = a; }
        };
        if (W > 0) {
            for (int ta = 0; ta <= W; ta++) for (int tb = 0; tb <= ta; tb++) to_u(P.lr_PK[ta][tb], P.lr_PKu[ta][tb]);
            for (int k = 0; k <= W; k++) to_u(P.lr_HI[k], P.lr_HIu[k]);
        }
        if (priors->gmm_k > 0) {
            const int D = priors->gmm_dim, off = nu - D;
            std::vector<double> A((size_t)nu * nu);
            for (int k = 0; k < priors->gmm_k; k++) {
                std::fill(A.begin(), A.end(), 0.0);
                for (int i = 0; i < D; i++)
                    for (int j = 0; j < D; j++) { A[(size_t)(off + i) * nu + off + j] = priors->gmm_P[k][i][j]; P.gmm_PT[k][j][i] = priors->gmm_P[k][i][j]; }
                to_u(A.data(), P.gmm_Q[k]);
            }
        }
        HIPCHK(hipMalloc(&h->pri, sizeof(DevPriors)));
        HIPCHK(hipMemcpy(h->pri, &P, sizeof(DevPriors), hipMemcpyHostToDevice));
        h->gmm_k = priors->gmm_k; h->gmm_dim = priors->gmm_dim; h->lr_window = W;
        h->pb = W > 3 ? W : 3;
    }
    return CPE_OK;
}

static cpe_status check_priors(const cpe_priors* priors, bool* use_pri) {
    *use_pri = priors && (priors->gmm_k > 0 || priors->lr_window > 0);
    if (*use_pri) {
        if (priors->gmm_k < 0 || priors->gmm_k > CPE_MAX_GMM || priors->gmm_dim < 0 || priors->gmm_dim > CPE_NX || (priors->gmm_k > 0 && priors->gmm_dim < 1))
            return fail(CPE_BAD_ARG, "pose prior: component count / dimension out of range");
        if (priors->lr_window < 0 || priors->lr_window > CPE_MAX_WINDOW)
            return fail(CPE_BAD_ARG, "motion prior: window " + std::to_string(priors->lr_window) + " out of range (0 = off, 1.." + std::to_string(CPE_MAX_WINDOW) + ")");
    }
    return CPE_OK;
}

cpe_status cpe_create(const cpe_skeleton* skel, const cpe_camera* cams, int32_t n_cams, const cpe_options* opts,
                      const cpe_priors* priors, int32_t device, cpe_handle** out) {
    if (!skel || !cams || !opts || !out) return fail(CPE_BAD_ARG, "null argument");
    bool use_pri;
    if (cpe_status s = check_priors(priors, &use_pri); s != CPE_OK) return s;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(CPE_NO_DEVICE, "no HIP device: this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(CPE_BAD_ARG, "device index out of range");
    cpe_handle* h = new cpe_handle();
    h->device = device; h->opts = *opts;
    const cpe_status s = create_impl(h, skel, cams, n_cams, opts, priors, use_pri);
    if (s != CPE_OK) { cpe_destroy(h); return s; }      // releases whatever was allocated before the failure
    *out = h;
    return CPE_OK;
}

static void free_kws(cpe_handle* h) {
    ws_free(h->kws_bufs);
    h->kws_frames = 0;
}

static void free_ws(cpe_handle* h) {       // the kinetic workspace goes with it
    free_kws(h);
    ws_free(h->ws_bufs);
    h->ws_frames = 0; h->ws_B = 0;
}

// The fields two models of one cpe_create_multi handle must share (include/cpe.h): the skeleton's shape, the relative-angle convention the priors
// are built in, and the options the LM driver reads as launch parameters or applies on the host.  Returns the first field that differs, or null.
static const char* shape_mismatch(const cpe_skeleton& a, const cpe_skeleton& b, const cpe_options& oa, const cpe_options& ob) {
    auto same = [](const auto& x, const auto& y, int n) { return memcmp(&x, &y, sizeof(x[0]) * (size_t)n) == 0; };
    if (a.n_links != b.n_links) return "n_links";
    if (!same(a.parent, b.parent, a.n_links)) return "parent";
    if (a.n_markers != b.n_markers) return "n_markers";
    if (!same(a.marker_link, b.marker_link, a.n_markers)) return "marker_link";
    if (a.n_joints != b.n_joints) return "n_joints";
    if (!same(a.joint_parent, b.joint_parent, a.n_joints)) return "joint_parent";
    if (!same(a.joint_child, b.joint_child, a.n_joints)) return "joint_child";
    if (!same(a.joint_kind, b.joint_kind, a.n_joints)) return "joint_kind";
    if (a.n_bounds != b.n_bounds) return "n_bounds";
    if (!same(a.bound_a, b.bound_a, a.n_bounds)) return "bound_a";
    if (!same(a.bound_b, b.bound_b, a.n_bounds)) return "bound_b";
    const int nq = 3 + 3 * a.n_links;
    if (!same(a.rel_ref, b.rel_ref, nq)) return "rel_ref";
    if (!same(a.rel_sign, b.rel_sign, nq)) return "rel_sign";
    if (oa.lambda0 != ob.lambda0) return "lambda0";
    if (oa.tol_step != ob.tol_step) return "tol_step";
    if (oa.tol_cost != ob.tol_cost) return "tol_cost";
    if (oa.max_iter != ob.max_iter) return "max_iter";
    if (oa.max_outer != ob.max_outer) return "max_outer";
    if (oa.curvature != ob.curvature) return "curvature";
    if (oa.bound_tol != ob.bound_tol) return "bound_tol";
    if (oa.cost_scale != ob.cost_scale) return "cost_scale";
    return nullptr;
}

cpe_status cpe_create_multi(int32_t n_models, const cpe_skeleton* skels, const cpe_camera* cams, const int32_t* n_cams, const cpe_options* opts,
                            const cpe_priors* priors, int32_t device, cpe_handle** out) {
    if (!skels || !cams || !n_cams || !opts || !out) return fail(CPE_BAD_ARG, "null argument");
    if (n_models < 1) return fail(CPE_BAD_ARG, "n_models must be at least 1");
    bool use_pri;
    if (cpe_status s = check_priors(priors, &use_pri); s != CPE_OK) return s;
    // every refusal below comes before the device is opened
    std::vector<DevModel> models((size_t)n_models);
    for (int k = 0; k < n_models; k++) {
        if (cpe_status s = build_model(&skels[k], cams + (size_t)k * CPE_MAX_CAMS, n_cams[k], &opts[k], models[k]); s != CPE_OK)   // (checks the counts)
            return fail(s, std::string("cpe_create_multi: model ") + std::to_string(k) + ": " + g_err);
        if (k > 0)
            if (const char* field = shape_mismatch(skels[0], skels[k], opts[0], opts[k]))
                return fail(CPE_BAD_ARG, std::string("cpe_create_multi: model ") + std::to_string(k) + " differs from model 0 in " + field);
        if (k > 0 && (models[k].nu != models[0].nu || memcmp(models[k].indep, models[0].indep, sizeof(models[0].indep)) != 0))
            return fail(CPE_BAD_ARG, std::string("cpe_create_multi: model ") + std::to_string(k) + " differs from model 0 in its independent dofs");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(CPE_NO_DEVICE, "no HIP device: this library has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(CPE_BAD_ARG, "device index out of range");
    cpe_handle* h = new cpe_handle();
    h->device = device; h->opts = opts[0];
    for (int k = 0; k < n_models; k++) build_com_model(&skels[k], cams + (size_t)k * CPE_MAX_CAMS, n_cams[k], &opts[k], h->cmodels, h->com_err);
    const cpe_status s = create_impl(h, &skels[0], cams, n_cams[0], &opts[0], priors, use_pri, &models);
    if (s != CPE_OK) { cpe_destroy(h); return s; }
    *out = h;
    return CPE_OK;
}

void cpe_destroy(cpe_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    free_ws(h);
    if (h->dm) (void)hipFree(h->dm);
    if (h->flag) (void)hipFree(h->flag);
    if (h->pri) (void)hipFree(h->pri);
    if (h->eom) (void)hipFree(h->eom);
    if (h->dyn) (void)hipFree(h->dyn);
    if (h->dk) (void)hipFree(h->dk);
    if (h->dtrack) (void)hipFree(h->dtrack);
    if (h->trackH) (void)hipFree(h->trackH);
    if (h->xtgt) (void)hipFree(h->xtgt);
    if (h->covG) (void)hipFree(h->covG);
    if (h->dmc) (void)hipFree(h->dmc);
    if (h->rateJ) (void)hipFree(h->rateJ);
    if (h->n_act) (void)hipFree(h->n_act);
    if (h->poll_host) (void)hipHostFree(h->poll_host);
    for (int i = 0; i < 2; i++) if (h->poll_ev[i]) (void)hipEventDestroy(h->poll_ev[i]);
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    for (auto& sp : h->prof_spans) { (void)hipEventDestroy(sp.second.first); (void)hipEventDestroy(sp.second.second); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

void* cpe_stream(cpe_handle* h) { return h ? (void*)h->stream : nullptr; }
cpe_status cpe_synchronize(cpe_handle* h) {
    if (!h) return fail(CPE_BAD_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    return CPE_OK;
}

// ---- ordering against the caller's stream (e.g. torch's current stream) ---------------------------------------------
cpe_status cpe_stream_wait(cpe_handle* h, void* other) {
    if (!h) return fail(CPE_BAD_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->order_ev, (hipStream_t)other));
    HIPCHK(hipStreamWaitEvent(h->stream, h->order_ev, 0));
    return CPE_OK;
}
cpe_status cpe_stream_signal(cpe_handle* h, void* other) {
    if (!h) return fail(CPE_BAD_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->order_ev, h->stream));
    HIPCHK(hipStreamWaitEvent((hipStream_t)other, h->order_ev, 0));
    return CPE_OK;
}

// ---- per-kernel device time of cpe_solve ------------------------------------------------------------------------------
cpe_status cpe_profile_enable(cpe_handle* h, int32_t on) {
    if (!h) return fail(CPE_BAD_ARG, "null handle");
    h->prof = on != 0;
    for (int i = 0; i < CPE_PROFILE_SLOTS; i++) { h->prof_ms[i] = 0.0; h->prof_n[i] = 0; }
    return CPE_OK;
}
cpe_status cpe_profile_get(cpe_handle* h, double* ms, int64_t* launches) {
    if (!h || !ms || !launches) return fail(CPE_BAD_ARG, "null argument");
    for (int i = 0; i < CPE_PROFILE_SLOTS; i++) { ms[i] = h->prof_ms[i]; launches[i] = h->prof_n[i]; }
    return CPE_OK;
}
static void prof_begin(cpe_handle* h, int id) {
    if (!h->prof) return;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    (void)hipEventRecord(a, h->stream);
    h->prof_spans.push_back({id, {a, b}});
}
static void prof_end(cpe_handle* h) {
    if (!h->prof || h->prof_spans.empty()) return;
    (void)hipEventRecord(h->prof_spans.back().second.second, h->stream);
}
static void prof_collect(cpe_handle* h) {       // after the stream has been synchronised
    for (auto& sp : h->prof_spans) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, sp.second.first, sp.second.second) == hipSuccess) { h->prof_ms[sp.first] += ms; h->prof_n[sp.first]++; }
        (void)hipEventDestroy(sp.second.first); (void)hipEventDestroy(sp.second.second);
    }
    h->prof_spans.clear();
}

int32_t cpe_jacobian_slots(const cpe_handle* h) { return h ? h->hm.S : 0; }
cpe_status cpe_jacobian_layout(const cpe_handle* h, int32_t* slot_marker, int32_t* slot_dof) {
    if (!h || !slot_marker || !slot_dof) return fail(CPE_BAD_ARG, "null argument");
    for (int s = 0; s < h->hm.S; s++) { slot_marker[s] = h->hm.slot_marker[s]; slot_dof[s] = h->hm.slot_dof[s]; }
    return CPE_OK;
}
int32_t cpe_num_independent(const cpe_handle* h) { return h ? h->hm.nu : 0; }
cpe_status cpe_independent_dofs(const cpe_handle* h, int32_t* dofs) {
    if (!h || !dofs) return fail(CPE_BAD_ARG, "null argument");
    for (int k = 0; k < h->hm.nu; k++) dofs[k] = h->hm.indep[k];
    return CPE_OK;
}

// The size check of every entry point that takes a batch of B sequences of N frames: F = B N frames, at most one launch grid of them.
static cpe_status frames(int32_t B, int32_t N, size_t* F) {
    if (B < 0 || N < 0) return fail(CPE_BAD_ARG, "negative size");
    *F = (size_t)B * N;
    if (*F > 0x7fffffffULL) return fail(CPE_BAD_ARG, "too many frames for one launch");
    return CPE_OK;
}

cpe_status cpe_eval_resjac(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                           double* r, double* J, double* eps, double* cost) {
    if (!h || !q || !meas || !r || !J || !eps) return fail(CPE_BAD_ARG, "null argument");
    if (cost && !weight) return fail(CPE_BAD_ARG, "cost requested without weights");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    const DevModel& m = h->hm;
    if (m.C * m.L > RJ_MAXPASS * WAVE) return fail(CPE_BAD_ARG, "cpe_eval_resjac supports at most 256 (camera, marker) pairs");
    constexpr int NW = 4;                                   // waves (= frames in flight) per workgroup
    const size_t lds = sizeof(double) * (((rj_shared_doubles(m.C, m.L, m.S) + 1) & ~1) + (size_t)NW * rj_wave_doubles(m.C, m.L, m.nq, m.nl));
    int wg_per_cu = (int)((160 * 1024) / lds);
    if (wg_per_cu < 1) return fail(CPE_BAD_ARG, "model too large for the LDS of one workgroup");
    // 2 workgroups (8 waves) per CU: the kernel needs ~200 VGPRs; capping it at 168 for 3 waves/SIMD spills
    // and measures 25 % slower (profiles/r01_resjac_ablation.md)
    constexpr int variant = 2;
    if (wg_per_cu > variant) wg_per_cu = variant;
    long grid = (long)h->n_cu * wg_per_cu;
    const long need = (long)((F + NW - 1) / NW);
    if (grid > need) grid = need;
    const int npass = (m.C * m.L + WAVE - 1) / WAVE;
#define RJ_LAUNCH(COST, NP, OC) hipLaunchKernelGGL((k_resjac<COST, NW, NP, OC>), dim3((unsigned)grid), dim3(WAVE * NW), lds, h->stream, h->dm, N, (long)F, q, meas, weight, r, J, eps, cost)
    if (cost) { if (npass <= 3) RJ_LAUNCH(true, 3, 2); else RJ_LAUNCH(true, 4, 2); }
    else { if (npass <= 3) RJ_LAUNCH(false, 3, 2); else RJ_LAUNCH(false, 4, 2); }
#undef RJ_LAUNCH
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_project_joints(cpe_handle* h, int32_t B, int32_t N, double* q) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;                      // empty batch: q may be null
    if (!q) return fail(CPE_BAD_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemsetAsync(h->flag, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_project, dim3((unsigned)F), dim3(WAVE), sizeof(double) * (h->hm.nq + 6 * h->hm.nl), h->stream, h->dm, q, h->flag);
    HIPCHK(hipGetLastError());
    int fl = 0;
    HIPCHK(hipMemcpyAsync(&fl, h->flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return fl ? CPE_NUMERICAL : CPE_OK;
}

cpe_status cpe_grf_fit(cpe_handle* h, const cpe_grf_options* opt, int32_t B, int32_t N, const double* q, const double* dq,
                       const double* ddq, const int32_t* contact, double* grfz, double* grfxy, double* residual) {
    if (!h || !opt || !q || !dq || !ddq || !contact || !grfz || !grfxy) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (opt->n_feet < 1 || opt->n_feet > 4 || opt->iterations < 1 || !(opt->gravity > 0) || !(opt->force_max > 0) || !(opt->friction_ratio >= 0))
        return fail(CPE_BAD_ARG, "grf options out of range");
    for (int f = 0; f < opt->n_feet; f++)
        if (opt->foot_marker[f] < 0 || opt->foot_marker[f] >= h->hm.L) return fail(CPE_BAD_ARG, "foot marker index out of range");
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_grf, dim3((unsigned)((F + GRF_PACK - 1) / GRF_PACK)), dim3(WAVE), 0, h->stream, h->dm, *opt, F, q, dq, ddq, contact, grfz, grfxy, residual);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_eom_rows(cpe_handle* h, const cpe_eom_options* opt, int32_t B, int32_t N, const double* q, const double* dq,
                        const double* ddq, double* rows) {
    if (!h || !opt || !q || !dq || !ddq || !rows) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    if (!h->eom) HIPCHK(hipMalloc(&h->eom, sizeof(cpe_eom_options)));
    HIPCHK(hipMemcpyAsync(h->eom, opt, sizeof(cpe_eom_options), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_eom, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, h->eom, F, q, dq, ddq, rows);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_eom_residual(cpe_handle* h, const cpe_dyn_options* opt, int32_t B, int32_t N, const double* q, const double* dq,
                            const double* ddq, const double* tau, const double* lambda, const double* grf, double* residual) {
    if (!h || !opt || !q || !dq || !ddq || !residual) return fail(CPE_BAD_ARG, "null argument");
    if (opt->n_feet < 0 || opt->n_feet > 4 || opt->n_motors < 0 || opt->n_motors > 32) return fail(CPE_BAD_ARG, "dynamics options out of range");
    for (int f = 0; f < opt->n_feet; f++) if (opt->foot_marker[f] < 0 || opt->foot_marker[f] >= h->hm.L) return fail(CPE_BAD_ARG, "foot marker index out of range");
    for (int m = 0; m < opt->n_motors; m++)
        if (opt->motor_first[m] < 0 || opt->motor_first[m] >= h->hm.nl || opt->motor_second[m] < 0 || opt->motor_second[m] >= h->hm.nl ||
            opt->motor_axis[m] < 0 || opt->motor_axis[m] > 2) return fail(CPE_BAD_ARG, "motor definition out of range");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    cpe_status s = cpe_eom_rows(h, &opt->eom, B, N, q, dq, ddq, residual);
    if (s != CPE_OK) return s;
    if (F == 0 || (!tau && !lambda && !grf)) return CPE_OK;
    if (!h->dyn) HIPCHK(hipMalloc(&h->dyn, sizeof(cpe_dyn_options)));
    HIPCHK(hipMemcpyAsync(h->dyn, opt, sizeof(cpe_dyn_options), hipMemcpyHostToDevice, h->stream));
    int n_con = 0;
    for (int j = 0; j < h->hm.nj; j++) n_con += h->hm.joint_kind[j] == CPE_JOINT_REVOLUTE_Y ? 2 : 1;
    hipLaunchKernelGGL(k_dyn_forces, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, h->dyn, F, q, tau, lambda, grf, n_con, residual);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_forward_kinematics(cpe_handle* h, int32_t B, int32_t N, const double* q, double* positions, double* com) {
    if (!h || !q || !positions) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_fk, dim3((unsigned)F), dim3(WAVE), lds_fk(h->hm), h->stream, h->dm, q, positions, com);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_marker_velocities(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* dq, double* velocities) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    if (!q || !dq || !velocities) return fail(CPE_BAD_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t lds = sizeof(double) * (2 * h->hm.nq + 6 * h->hm.nl + 36 * h->hm.nl);
    hipLaunchKernelGGL(k_marker_vel, dim3((unsigned)F), dim3(WAVE), lds, h->stream, h->dm, q, dq, velocities);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_reproject(cpe_handle* h, int32_t B, int32_t N, const double* positions, double* uv) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    if (!positions || !uv) return fail(CPE_BAD_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_reproject, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, positions, uv);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

// ---- the detection report (include/cpe.h, cpe_detection_report; kernel in cpe_detection.hip.inc) ---------------------------------------------
// the refusals of both entries, in one place: everything that can be told from the arguments alone, then the handle.  F == 0 asks for nothing,
// so its arrays may be null (cpe_reproject's convention).
static cpe_status detection_args(const char* who, const cpe_handle* h, int32_t B, int32_t N, const double* positions, const double* cov_pos,
                                 const double* meas, const double* weight, const double* weight_fit, const double* uv, const double* cov_px,
                                 const double* uv_loo, const double* cov_loo, const double* d2, const double* leverage, size_t* F) {
    const std::string w = std::string(who) + ": ";
    if (B < 0 || N < 0) return fail(CPE_BAD_ARG, w + "negative size");
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return fail(s, w + g_err);
    if ((meas == nullptr) != (weight == nullptr)) return fail(CPE_BAD_ARG, w + "meas and weight are given together");
    if (weight_fit && !weight) return fail(CPE_BAD_ARG, w + "weight_fit without weight");
    if (!meas) {
        const char* name = uv_loo ? "uv_loo" : cov_loo ? "cov_loo" : d2 ? "d2" : leverage ? "leverage" : nullptr;
        if (name) return fail(CPE_BAD_ARG, w + name + " requested without measurements");
    }
    if (*F > 0) {
        const char* name = !positions ? "positions" : !cov_pos ? "cov_pos" : !uv ? "uv" : !cov_px ? "cov_px" : nullptr;
        if (name) return fail(CPE_BAD_ARG, w + name + " is null");
    }
    if (!h) return fail(CPE_BAD_ARG, w + "the handle is null");
    return CPE_OK;
}

cpe_status cpe_detection_report(cpe_handle* h, int32_t B, int32_t N, const double* positions, const double* cov_pos, const double* meas,
                                const double* weight, const double* weight_fit, double* uv, double* cov_px, double* uv_loo, double* cov_loo,
                                double* d2, double* leverage) {
    size_t F;
    if (cpe_status s = detection_args("cpe_detection_report", h, B, N, positions, cov_pos, meas, weight, weight_fit, uv, cov_px, uv_loo, cov_loo, d2,
                                      leverage, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    if (meas)
        hipLaunchKernelGGL(k_detection_report<true>, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, positions, cov_pos, meas, weight,
                           weight_fit ? weight_fit : weight, uv, cov_px, uv_loo, cov_loo, d2, leverage);
    else
        hipLaunchKernelGGL(k_detection_report<false>, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, positions, cov_pos, nullptr, nullptr,
                           nullptr, uv, cov_px, nullptr, nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_detection_report_host(cpe_handle* h, int32_t B, int32_t N, const double* positions, const double* cov_pos, const double* meas,
                                     const double* weight, const double* weight_fit, double* uv, double* cov_px, double* uv_loo, double* cov_loo,
                                     double* d2, double* leverage) {
    size_t F;
    if (cpe_status s = detection_args("cpe_detection_report_host", h, B, N, positions, cov_pos, meas, weight, weight_fit, uv, cov_px, uv_loo, cov_loo,
                                      d2, leverage, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t nL = F * (size_t)h->hm.L, nCL = F * (size_t)h->hm.C * h->hm.L;
    Staging st(h->stream);
    const double* dp = st.in(positions, 3 * nL);
    const double* dc = st.in(cov_pos, 9 * nL);
    const double* dz = st.in(meas, 2 * nCL);
    const double* dw = st.in(weight, nCL);
    const double* dwf = st.in(weight_fit, nCL);
    double* ouv = st.out(uv, 2 * nCL);
    double* ocp = st.out(cov_px, 3 * nCL);
    double* oul = st.out_opt(uv_loo, 2 * nCL);
    double* ocl = st.out_opt(cov_loo, 3 * nCL);
    double* od2 = st.out_opt(d2, nCL);
    double* olv = st.out_opt(leverage, nCL);
    HIPCHK(st.err);
    const cpe_status s = cpe_detection_report(h, B, N, dp, dc, dz, dw, dwf, ouv, ocp, oul, ocl, od2, olv);
    if (s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

cpe_status cpe_triangulate(cpe_handle* h, int32_t n, const int32_t* cam_a, const int32_t* cam_b, const double* uv_a, const double* uv_b,
                           double depth, double* xyz) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    if (n < 0) return fail(CPE_BAD_ARG, "negative size");
    if (n == 0) return CPE_OK;                      // empty input: the arrays may be null
    if (!cam_a || !cam_b || !uv_a || !uv_b || !xyz) return fail(CPE_BAD_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    // the camera indices select entries of the handle's camera table: check them on the host before any lane dereferences one
    std::vector<int32_t> ia(n), ib(n);
    HIPCHK(hipMemcpyAsync(ia.data(), cam_a, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ib.data(), cam_b, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++)
        if (ia[i] < 0 || ia[i] >= h->hm.C || ib[i] >= h->hm.C) return fail(CPE_BAD_ARG, "camera index out of range");
    hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->dm, n, cam_a, cam_b, uv_a, uv_b, depth, xyz);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_tensorise_dlc(cpe_handle* h, int32_t N, int32_t n_slots, int32_t slot, const double* table, int32_t rows, int32_t parts,
                             int32_t first_row, const int32_t* part_of_marker, const double* inv_sigma, double thresh, double* meas, double* weight) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    if (N < 0 || rows < 0 || parts <= 0) return fail(CPE_BAD_ARG, "bad size");
    if (n_slots <= 0 || slot < 0 || slot >= n_slots) return fail(CPE_BAD_ARG, "camera slot out of range");
    if (N == 0) return CPE_OK;
    if (!part_of_marker || !inv_sigma || !meas || !weight || (!table && rows > 0)) return fail(CPE_BAD_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    const long total = (long)N * h->hm.L;
    hipLaunchKernelGGL(k_tensorise_dlc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, N, h->hm.L, n_slots, slot, table, rows, parts,
                       first_row, part_of_marker, inv_sigma, thresh, meas, weight);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

static size_t n_mu(const DevModel& m, size_t F) { return F * (size_t)(m.nb > 0 ? m.nb : 1) * 2; }   // bound multipliers

static cpe_status ensure_ws(cpe_handle* h, int B, int N) {
    const size_t F = (size_t)B * N;
    if (F <= h->ws_frames && B <= h->ws_B) return CPE_OK;
    free_ws(h);
    const int nu = h->hm.nu;
    auto& w = h->ws_bufs;
    HIPCHK(ws_alloc(w, h->qbuf, 2 * F * h->hm.ns));
    HIPCHK(ws_alloc(w, h->gambuf, 2 * F * (size_t)(GAM_STRIDE * (h->hm.nrev > 0 ? h->hm.nrev : 1))));
    HIPCHK(ws_alloc(w, h->gbuf, 2 * F * nu));
    HIPCHK(ws_alloc(w, h->Bbuf, 2 * F * nu * nu));
    HIPCHK(ws_alloc(w, h->costbuf, 2 * F * COST_STRIDE));
    HIPCHK(ws_alloc(w, h->mu, n_mu(h->hm, F)));
    HIPCHK(ws_alloc(w, h->Lbuf, F * (h->pb + 1) * nu * nu + (size_t)B * lm_spill_doubles(h->pb)));     // + k_lm_step's window blocks past LDS
    HIPCHK(ws_alloc(w, h->zbuf, F * nu));
    HIPCHK(ws_alloc(w, h->gtbuf, F * nu));
    HIPCHK(ws_alloc(w, h->dgbuf, F * nu));
    HIPCHK(ws_alloc(w, h->cmax, F));
    HIPCHK(ws_alloc(w, h->st, B));
    HIPCHK(ws_alloc(w, h->act, B));
    HIPCHK(ws_alloc(w, h->rseq, B));
    if (h->lr_window > 0) HIPCHK(ws_alloc(w, h->Hlr, 2 * F * h->pb * nu * nu));
    h->ws_frames = F; h->ws_B = B;
    return CPE_OK;
}

// f(std::integral_constant<int, PB>{}) for the handle's half-bandwidth PB = 3..6: k_lm_step and k_lm_back are instantiated per PB
extern "C++" template <class Fn>
static void with_pb(int pb, Fn&& f) {
    switch (pb) {
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 6>{}); break;
    }
}

// f(std::true_type{}, *rg) with the ragged table of a call, f(std::false_type{}, RaggedArgs{}) without one (rg null): every kernel that has a
// ragged form takes the flag as its RAGGED template argument and the table as its last argument, and is launched from inside such an f
extern "C++" template <class Fn>
static void with_ragged(const RaggedArgs* rg, Fn&& f) {
    if (rg) f(std::true_type{}, *rg);
    else f(std::false_type{}, RaggedArgs{});
}

// Cold start of every sequence from Euler q (device pointer): state buffer 0 = (q, alpha), sequence states and bound multipliers zero.
// rg: the ragged table of cpe_solve_ragged (N = nmax), or null
static cpe_status state_reset(cpe_handle* h, int B, int N, const double* q, const RaggedArgs* rg = nullptr) {
    const size_t F = (size_t)B * N;
    // Euler q -> (q, alpha)
    with_ragged(rg, [&](auto r, RaggedArgs a) { hipLaunchKernelGGL(k_state_init<decltype(r)::value>, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, q, h->qbuf, a); });
    HIPCHK(hipMemsetAsync(h->st, 0, sizeof(SeqState) * B, h->stream));
    HIPCHK(hipMemsetAsync(h->mu, 0, sizeof(double) * n_mu(h->hm, F), h->stream));
    return CPE_OK;
}

cpe_status cpe_eval_normal(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                           double* g, double* Bm, double* cost, double* gam, double* q_out) {
    if (!h || !q || !meas || !weight || !g || !Bm || !cost) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    if ((s = state_reset(h, B, N, q)) != CPE_OK) return s;
    const DevModel& m = h->hm;
    hipLaunchKernelGGL(frame_normal<>(h->gmm_k == 0), dim3((unsigned)F), dim3(WAVE), lds_normal(h, nullptr), h->stream, h->dm, h->st, N, 1, F, h->qbuf, meas, weight,
                       h->gbuf, h->Bbuf, h->costbuf, h->mu, h->gambuf, h->pri, nullptr, nullptr, ShutterArgs{nullptr, nullptr, nullptr}, RaggedArgs{});
    HIPCHK(hipMemcpyAsync(g, h->gbuf, sizeof(double) * F * m.nu, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(Bm, h->Bbuf, sizeof(double) * F * m.nu * m.nu, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(k_gather_normal, dim3((unsigned)F), dim3(128), 0, h->stream, h->dm, F, h->qbuf, h->costbuf, h->gambuf, cost, gam, q_out);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

static LmParams lm_params(const cpe_handle* h, int B, int N) {
    LmParams prm;
    prm.tol_step = h->opts.tol_step; prm.tol_cost = h->opts.tol_cost; prm.lambda0 = h->opts.lambda0; prm.B = B; prm.N = N;
    prm.bound_tol = h->opts.bound_tol; prm.max_outer = h->opts.max_outer; prm.max_iter = h->opts.max_iter;
    return prm;
}

// One LM iteration of the sequences listed in `act` (device arrays; nullptr = all B), `first` = 1 in the first pass.  The grids are sized
// for `slots` sequences; workgroups past *n_act leave at once.
using LmIterate = std::function<void(int first, const int* act, const int* n_act, int slots)>;

// The one launch of k_build_act (one workgroup of 256 threads): lm_drive before every iteration, cpe_eval_active_list on its scratch arrays.
static void launch_build_act(hipStream_t stream, const SeqState* st, int B, int window, int* act, int* n_act) {
    hipLaunchKernelGGL(k_build_act, dim3(1), dim3(256), 0, stream, st, B, window, act, n_act);
}

// The LM loop of both models on the handle's workspace, from the first pass over every sequence to the last sequence's end.
// Active window: k_lm_step runs one workgroup per sequence and its duration is the sequential depth of ONE sequence,
// whatever the grid (3.3 ms for <= 256 workgroups, 4.4 ms for 512 = 2 per CU), so the launches are kept exactly full: before
// every iteration k_build_act lists the first `window` unfinished sequences ON THE DEVICE, so a sequence that converges hands
// its slot to the next waiting one at once and the host never waits for an iteration: it queues POLL iterations, then reads
// the PREVIOUS batch's snapshot of the list length (pinned memory + event) -- the stream stays at least one batch ahead and
// is never drained inside the loop.  The price is at most 2 POLL iterations of empty launches after the last sequence ends.
static cpe_status lm_drive(cpe_handle* h, int B, const LmIterate& iterate) {
    iterate(1, nullptr, nullptr, B);        // first evaluation and first step of every sequence
    HIPCHK(hipGetLastError());
    const int window = std::min(B, h->n_cu * (h->pb == 3 ? 2 : 1));          // k_lm_step: 2 workgroups per CU at PB = 3, 1 at PB = 4..6
    constexpr int POLL = 4;
    const long per_seq = (long)h->opts.max_iter + 2L * (h->opts.max_outer > 0 ? h->opts.max_outer : 0) + POLL;
    const long max_rounds = ((long)(B + window - 1) / window + 1) * per_seq;
    bool pending[2] = {false, false};
    int slot = 0;
    for (long it = 0; it < max_rounds; it += POLL) {
        for (int k = 0; k < POLL; k++) {
            prof_begin(h, 3);
            launch_build_act(h->stream, h->st, B, window, h->act, h->n_act);
            prof_end(h);
            iterate(0, h->act, h->n_act, window);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h->poll_host + slot, h->n_act, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipEventRecord(h->poll_ev[slot], h->stream));
        pending[slot] = true;
        const int prev = 1 - slot;
        if (pending[prev]) {
            HIPCHK(hipEventSynchronize(h->poll_ev[prev]));
            pending[prev] = false;
            if (h->poll_host[prev] == 0) break;          // no sequence was running when that list was built
        }
        slot = prev;
    }
    return CPE_OK;
}

// restart of an LM run from the current iterate (shutter-delay outer loop): every sequence runs again, its buffers stay
__global__ void k_reset_status(SeqState* __restrict__ st, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) { st[b].status = 0; st[b].al_pending = 0; }
}

// One iteration of the kinematic solve (the LmIterate of lm_run): k_frame_normal (+ k_lr_band) on the evaluated buffer, then k_lm_step and
// k_lm_back.  sh: shutter-delay buffers (all null = off); rg: the ragged table (N = nmax), or null.  Precondition: sh is all null whenever rg
// is given -- the ragged forms have no shutter delay (lm_run refuses the pair; the other callers pass one of the two as null).
// back = false (cpe_covariance): stop after k_lm_step -- the factor is in Lbuf and every factored sequence has back_pending = 1.
static void lm_iterate(cpe_handle* h, const LmParams& prm, int N, size_t Fw, size_t ldsn, const double* meas, const double* weight, ShutterArgs sh,
                       const RaggedArgs* rg, int first, const int* act, const int* n_act, int slots, bool back = true) {
    const bool lr = h->lr_window > 0;
    const unsigned gf = (unsigned)((size_t)slots * N);
    const double* hiu = lr ? reinterpret_cast<const double*>(reinterpret_cast<const char*>(h->pri) + offsetof(DevPriors, lr_HIu)) + CPE_NX * CPE_NX : nullptr;
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        prof_begin(h, 0);
        hipLaunchKernelGGL(frame_normal<R>(h->gmm_k == 0 && sh.tau == nullptr), dim3(gf), dim3(WAVE), ldsn, h->stream, h->dm, h->st, N, first, Fw, h->qbuf, meas, weight,
                           h->gbuf, h->Bbuf, h->costbuf, h->mu, h->gambuf, h->pri, act, n_act, sh, a);
        prof_end(h);
        if (lr) {
            prof_begin(h, 1);
            hipLaunchKernelGGL(k_lr_band<R>, dim3(gf), dim3(WAVE), 0, h->stream, h->dm, h->st, N, first, Fw, h->qbuf, h->gambuf, h->pri, h->pb, h->gbuf, h->Bbuf,
                               h->Hlr, h->costbuf, act, n_act, a);
            prof_end(h);
        }
        prof_begin(h, 2);
        with_pb(h->pb, [&](auto pbc) {
            hipLaunchKernelGGL((k_lm_step<decltype(pbc)::value, 0, R>), dim3(slots), dim3(LM_THREADS), 0, h->stream, h->dm, h->st, prm, first, h->qbuf, h->gbuf,
                               h->Bbuf, h->costbuf, h->Lbuf, h->zbuf, h->gtbuf, h->gambuf, h->Hlr, act, n_act, 2, sh.gx, h->dgbuf, hiu, h->lr_window, a);
        });
        prof_end(h);
        if (!back) return;
        prof_begin(h, 7);
        with_pb(h->pb, [&](auto pbc) {
            hipLaunchKernelGGL((k_lm_back<decltype(pbc)::value, R>), dim3(slots), dim3(2 * WAVE), 0, h->stream, h->dm, h->st, prm, h->qbuf, h->Lbuf, h->zbuf,
                               h->gtbuf, h->dgbuf, act, n_act, a);
        });
        prof_end(h);
    });
}

// The LM run of cpe_solve on the handle's workspace: cold start from q_init (device pointer) or, with q_init == nullptr, a restart from
// the current iterate of every sequence.  sh: shutter-delay buffers (all null = off).
// rg: the ragged table of cpe_solve_ragged (N = nmax; no shutter delay), or null.
static cpe_status lm_run(cpe_handle* h, int B, int N, const double* q_init, const double* meas, const double* weight, ShutterArgs sh,
                         const RaggedArgs* rg = nullptr) {
    if (rg && (sh.tau || sh.gx || sh.rcb)) return fail(CPE_BAD_ARG, "the ragged solve has no shutter delay");
    const size_t Fw = (size_t)B * N;   // buffers are laid out for exactly this call's F (strides use F)
    if (q_init) {
        const cpe_status s = state_reset(h, B, N, q_init, rg);
        if (s != CPE_OK) return s;
    } else hipLaunchKernelGGL(k_reset_status, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->st, B);
    const LmParams prm = lm_params(h, B, N);
    const size_t ldsn = lds_normal(h, rg, sh.tau != nullptr);
    return lm_drive(h, B, [&](int first, const int* act, const int* n_act, int slots) {
        lm_iterate(h, prm, N, Fw, ldsn, meas, weight, sh, rg, first, act, n_act, slots);
    });
}

// Outputs of a finished LM run: k_finalize (tau: the shutter delays, or null), then `more` (what else the caller enqueues there, or
// empty), then the sequence states and the max |joint equality| of every sequence are read back; the stream is drained.
// rg: the ragged table (N = nmax, tau null), or null.
static cpe_status lm_readback(cpe_handle* h, int B, int N, const double* meas, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                              const double* tau, const std::function<void()>& more, std::vector<SeqState>& hs, std::vector<double>& hc,
                              const RaggedArgs* rg = nullptr) {
    const size_t F = (size_t)B * N;
    HIPCHK(hipMemsetAsync(h->cmax, 0, sizeof(double) * B, h->stream));
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        hipLaunchKernelGGL(k_finalize<decltype(r)::value>, dim3((unsigned)F), dim3(WAVE), lds_fk(h, rg), h->stream, h->dm, h->st, N, F, h->qbuf, meas, q, dq, ddq,
                           positions, meas_err, reinterpret_cast<unsigned long long*>(h->cmax), tau, a);
    });
    if (more) more();
    HIPCHK(hipGetLastError());
    hs.resize(B);
    hc.resize(B);
    HIPCHK(hipMemcpyAsync(hs.data(), h->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(hc.data(), h->cmax, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    prof_collect(h);
    return CPE_OK;
}

// The cost terms each model reports (SeqState.terms).  The kinematic model: measurements, constant-acceleration model, pose prior,
// motion prior.  The physics-based model has no motion prior; its model cost is terms[4].
static void kinematic_costs(const SeqState& S, double scale, cpe_stats& o) {
    o.cost_meas = S.terms[0]; o.cost_model = S.terms[1]; o.cost_pose = S.terms[3]; o.cost_motion = S.terms[4];
    o.cost = scale * (S.terms[0] + S.terms[1] + S.terms[3] + S.terms[4]);
}
static void kinetic_costs(const SeqState& S, double scale, cpe_stats& o) {
    o.cost_meas = S.terms[0]; o.cost_model = S.terms[4]; o.cost_pose = S.terms[3]; o.cost_motion = 0.0;
    o.cost = scale * (S.terms[0] + S.terms[3] + S.terms[4]);
}

// Status of every sequence and, when `stats` is given, its cpe_stats (`iters_extra[b]` iterations of earlier runs added).  Returns the worst status.
static cpe_status seq_stats(const cpe_handle* h, int B, const std::vector<SeqState>& hs, const std::vector<double>& hc, const std::vector<int>* iters_extra,
                            void (*costs)(const SeqState&, double, cpe_stats&), cpe_stats* stats) {
    cpe_status worst = CPE_OK;
    for (int b = 0; b < B; b++) {
        const SeqState& S = hs[b];
        const cpe_status sb = S.status == 1 ? CPE_OK : ((S.status == 0 || S.status == 3) ? CPE_MAX_ITER : CPE_NUMERICAL);
        if (sb > worst) worst = sb;
        if (stats) {
            cpe_stats& o = stats[b];
            o.status = sb; o.iterations = S.iters + (iters_extra ? (*iters_extra)[b] : 0); o.lambda = S.lambda; o.max_constraint = hc[b];
            o.max_bound_violation = S.maxviol; o.outer = S.outer; o._pad = 0;
            costs(S, h->opts.cost_scale, o);
        }
    }
    return worst;
}

// outputs and statistics of a finished kinematic LM run; `iters_extra[b]` iterations of earlier runs are added
static cpe_status lm_finish(cpe_handle* h, int B, int N, const double* meas, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                            const double* tau, cpe_stats* stats, const std::vector<int>* iters_extra, const RaggedArgs* rg = nullptr) {
    std::vector<SeqState> hs;
    std::vector<double> hc;
    const cpe_status s = lm_readback(h, B, N, meas, q, dq, ddq, positions, meas_err, tau, nullptr, hs, hc, rg);
    if (s != CPE_OK) return s;
    return seq_stats(h, B, hs, hc, iters_extra, kinematic_costs, stats);
}

// The arguments of cpe_solve_ragged, checked before anything is launched: the (model, frames) table of the batch.
static cpe_status ragged_table(const cpe_handle* h, int B, int N_max, const int32_t* model, const int32_t* n_frames, std::vector<int2>& seq) {
    seq.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        if (model[b] < 0 || model[b] >= n_models(h))
            return fail(CPE_BAD_ARG, "cpe_solve_ragged: model index of sequence " + std::to_string(b) + " out of range");
        if (n_frames[b] < 1 || n_frames[b] > N_max)
            return fail(CPE_BAD_ARG, "cpe_solve_ragged: frame count of sequence " + std::to_string(b) + " outside 1..N_max");
        seq[(size_t)b] = make_int2(model[b], n_frames[b]);
    }
    return CPE_OK;
}

// The checked table on the device (h->rseq) and the kernels' view of it.  seq is pageable: the caller drains the stream before seq goes.
static cpe_status ragged_upload(cpe_handle* h, const std::vector<int2>& seq, int N_max, RaggedArgs& rg) {
    HIPCHK(hipMemcpyAsync(h->rseq, seq.data(), sizeof(int2) * seq.size(), hipMemcpyHostToDevice, h->stream));
    rg = RaggedArgs{h->rseq, N_max, cams_max(h)};
    return CPE_OK;
}

// cpe_solve (model == nullptr) and cpe_solve_ragged
static cpe_status solve_impl(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q_init, const double* meas,
                             const double* weight, double* q, double* dq, double* ddq, double* positions, double* meas_err, cpe_stats* stats) {
    if (!h || !q_init || !meas || !weight || !q) return fail(CPE_BAD_ARG, "null argument");
    if ((dq == nullptr) != (ddq == nullptr)) return fail(CPE_BAD_ARG, "dq and ddq must be given together");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    std::vector<int2> seq;
    if (model) { if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return s; }
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    RaggedArgs rgv;
    if (model && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;     // (seq outlives the stream: lm_finish drains it)
    const RaggedArgs* rg = model ? &rgv : nullptr;
    s = lm_run(h, B, N, q_init, meas, weight, ShutterArgs{nullptr, nullptr, nullptr}, rg);
    if (s != CPE_OK) return s;
    return lm_finish(h, B, N, meas, q, dq, ddq, positions, meas_err, nullptr, stats, nullptr, rg);
}

cpe_status cpe_solve(cpe_handle* h, int32_t B, int32_t N, const double* q_init, const double* meas, const double* weight,
                     double* q, double* dq, double* ddq, double* positions, double* meas_err, cpe_stats* stats) {
    return solve_impl(h, B, N, nullptr, nullptr, q_init, meas, weight, q, dq, ddq, positions, meas_err, stats);
}

cpe_status cpe_solve_ragged(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q_init,
                            const double* meas, const double* weight, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                            cpe_stats* stats) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    return solve_impl(h, B, N_max, model, n_frames, q_init, meas, weight, q, dq, ddq, positions, meas_err, stats);
}

// ---- shutter-delay estimation (include/cpe.h, cpe_solve_shutter) ------------------------------------------------------------------
// Anderson mixing (memory AA_MEM) of the delay iteration tau <- tau + step(tau): the plain iteration contracts slowly where all delays move
// together and the trajectory shifts in time to make up for it.  Host side, C - 1 unknowns per sequence.
namespace {
constexpr int AA_MEM = 4;
struct Anderson {
    int k = 0;
    double X[AA_MEM + 1][CPE_MAX_CAMS], F[AA_MEM + 1][CPE_MAX_CAMS], fn_prev = 0;
    void next(int n, const double* x, const double* f, double* xn) {
        double fn = 0;
        for (int i = 0; i < n; i++) fn += f[i] * f[i];
        if (k > 0 && fn > fn_prev) k = 0;                             // residual grew: drop the history
        fn_prev = fn;
        const int slot = k % (AA_MEM + 1);
        int mk = std::min(std::min(k, AA_MEM), n);
        for (int i = 0; i < n; i++) { X[slot][i] = x[i]; F[slot][i] = f[i]; xn[i] = x[i] + f[i]; }
        if (mk > 0) {
            double dX[AA_MEM][CPE_MAX_CAMS], dF[AA_MEM][CPE_MAX_CAMS], Mn[AA_MEM][AA_MEM], r[AA_MEM], tr = 0;
            for (int j = 0; j < mk; j++) {
                const int s1 = (k - j) % (AA_MEM + 1), s0 = (k - j - 1) % (AA_MEM + 1);
                for (int i = 0; i < n; i++) { dX[j][i] = X[s1][i] - X[s0][i]; dF[j][i] = F[s1][i] - F[s0][i]; }
            }
            for (int a = 0; a < mk; a++) {
                for (int b = 0; b < mk; b++) { double v = 0; for (int i = 0; i < n; i++) v += dF[a][i] * dF[b][i]; Mn[a][b] = v; }
                double v = 0; for (int i = 0; i < n; i++) v += dF[a][i] * f[i];
                r[a] = v; tr += Mn[a][a];
            }
            for (int a = 0; a < mk; a++) Mn[a][a] += 1e-10 * tr / mk + 1e-300;
            bool ok = true;
            for (int j = 0; j < mk && ok; j++) {
                double d = Mn[j][j];
                for (int t = 0; t < j; t++) d -= Mn[j][t] * Mn[j][t];
                if (!(d > 0)) { ok = false; break; }
                d = sqrt(d); Mn[j][j] = d;
                for (int i = j + 1; i < mk; i++) { double v = Mn[i][j]; for (int t = 0; t < j; t++) v -= Mn[i][t] * Mn[j][t]; Mn[i][j] = v / d; }
            }
            if (ok) {
                for (int i = 0; i < mk; i++) { double v = r[i]; for (int t = 0; t < i; t++) v -= Mn[i][t] * r[t]; r[i] = v / Mn[i][i]; }
                for (int i = mk - 1; i >= 0; i--) { double v = r[i]; for (int t = i + 1; t < mk; t++) v -= Mn[t][i] * r[t]; r[i] = v / Mn[i][i]; }
                for (int j = 0; j < mk; j++) for (int i = 0; i < n; i++) xn[i] -= r[j] * (dX[j][i] + dF[j][i]);
            }
        }
        k++;
    }
};
}  // namespace

cpe_status cpe_solve_shutter(cpe_handle* h, int32_t B, int32_t N, const double* q_init, const double* meas, const double* weight, double tau_bound,
                             int32_t max_rounds, double tol_tau, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                             double* tau_out, cpe_stats* stats, int32_t* rounds_out) {
    if (!h || !q_init || !meas || !weight || !q || !tau_out) return fail(CPE_BAD_ARG, "null argument");
    if ((dq == nullptr) != (ddq == nullptr)) return fail(CPE_BAD_ARG, "dq and ddq must be given together");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (max_rounds < 1 || !(tau_bound > 0) || !(tol_tau > 0)) return fail(CPE_BAD_ARG, "bad round count or tolerance");
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    const int C = h->hm.C;
    DevBuf gx, rcb, step;
    HIPCHK(gx.alloc(2 * F * 6)); HIPCHK(rcb.alloc(2 * F * C * 9)); HIPCHK(step.alloc((size_t)B * C));
    HIPCHK(hipMemsetAsync(tau_out, 0, sizeof(double) * B * C, h->stream));      // the first camera is the reference (tau = 0, acinoset_misc.py:274-275); the others start at 0
    ShutterArgs sh{tau_out, gx.p, rcb.p};
    std::vector<int> iters(B, 0);
    std::vector<SeqState> hs(B);
    std::vector<double> hstep((size_t)B * C), htau((size_t)B * C, 0.0);
    std::vector<Anderson> mix(B);
    std::vector<char> settled(B, 0);
    int round = 0;
    for (; round < max_rounds; round++) {
        s = lm_run(h, B, N, round == 0 ? q_init : nullptr, meas, weight, sh);
        if (s != CPE_OK) return s;
        hipLaunchKernelGGL(k_shutter_step, dim3(B), dim3(WAVE), 0, h->stream, h->dm, h->st, N, F, h->qbuf, rcb.p, tau_out, step.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs.data(), h->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(hstep.data(), step.p, sizeof(double) * B * C, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        bool all = true, moved = false;
        for (int b = 0; b < B; b++) {
            iters[b] += hs[b].iters;
            if (settled[b]) continue;                                 // its delays are a fixed point already (the trajectory solve above was a no-op restart)
            double worst = 0.0, tn[CPE_MAX_CAMS];
            for (int c = 1; c < C; c++) worst = std::max(worst, fabs(hstep[(size_t)b * C + c]));
            if (worst == 0.0 || hs[b].status == 2) { settled[b] = 1; continue; }   // nothing to move (N < 3), or a numerical failure: leave its delays alone
            mix[b].next(C, &htau[(size_t)b * C], &hstep[(size_t)b * C], tn);
            // the plain step underestimates the distance to the fixed point by the contraction factor (the trajectory has not followed
            // yet): the test is on the mixed update
            worst = 0.0;
            for (int c = 1; c < C; c++) {
                const double v = std::min(tau_bound, std::max(-tau_bound, tn[c]));
                worst = std::max(worst, fabs(v - htau[(size_t)b * C + c]));
                htau[(size_t)b * C + c] = v;
            }
            moved = true;
            if (worst < tol_tau) settled[b] = 1; else all = false;
        }
        if (moved) {
            HIPCHK(hipMemcpyAsync(tau_out, htau.data(), sizeof(double) * B * C, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));                  // htau is pageable: the copy has left the host buffer only now
        }
        if (all) { if (moved) round++; break; }
    }
    // one more solve at the final delays (they moved after the last one if max_rounds ran out; otherwise a restart that stops at once)
    s = lm_run(h, B, N, nullptr, meas, weight, sh);
    if (s != CPE_OK) return s;
    if (rounds_out) *rounds_out = round;
    return lm_finish(h, B, N, meas, q, dq, ddq, positions, meas_err, tau_out, stats, &iters);
}

// ---- physics-based trajectory model (include/cpe.h, cpe_solve_kinetic) -------------------------------------------------------------
void cpe_default_kinetic_options(cpe_kinetic_options* o, double fps, int32_t kinetic_dataset) {
    // o->dyn (inertias, feet, motors) is the caller's
    o->w_slack = 10e3; o->w_torque = 1.0; o->w_smooth = 0.1 / (fps * fps); o->friction = 0.8; o->force_max = 5.0; o->grfz_min = 0.01;
    o->foot_height_tol = kinetic_dataset ? 0.03 : 0.1; o->foot_height_min = 0.0; o->ground_height = 0.0; o->slip_max = 1.0; o->zvel_max = kinetic_dataset ? 1.0 : 0.0;
    o->slack_lo = -2.0; o->slack_hi = 2.0; o->kappa_slack = 1e6;
    o->reg_force = 1e-4; o->kappa_force = 1e5; o->kappa_height = 1e6; o->kappa_slip = 1e2; o->lm_force_damping = 10.0; o->lm_wall_damping = 10.0;
    o->inner_iterations = 30; o->_pad = 0;
}

// The kinetic tables K of model m under options opt (the batch's buffers grf_fix / tau_box / grf_box as given; the workspace is sized before this
// is called).  Host side only.
static cpe_status build_kin_entry(cpe_handle* h, const DevModel& m, const cpe_kinetic_options* opt, const double* grf_fix, const double* tau_box,
                                  const double* grf_box, DevKin& K) {
    memset(&K, 0, sizeof(K));
    K.o = *opt;
    const cpe_dyn_options& d = opt->dyn;
    if (d.n_feet < 1 || d.n_feet > 4 || d.n_motors < 0 || d.n_motors > CPE_MAX_MOTORS) return fail(CPE_BAD_ARG, "kinetic options: feet / motors out of range");
    for (int f = 0; f < d.n_feet; f++) if (d.foot_marker[f] < 0 || d.foot_marker[f] >= m.L) return fail(CPE_BAD_ARG, "foot marker index out of range");
    for (int k = 0; k < d.n_motors; k++)
        if (d.motor_first[k] < 0 || d.motor_first[k] >= m.nl || d.motor_second[k] < 0 || d.motor_second[k] >= m.nl || d.motor_axis[k] < 0 || d.motor_axis[k] > 2)
            return fail(CPE_BAD_ARG, "motor definition out of range");
    if (!(opt->w_slack > 0) || !(opt->kappa_force > 0) || !(opt->kappa_height > 0) || !(opt->kappa_slip > 0) || !(opt->reg_force > 0) ||
        !(d.eom.gravity > 0) || opt->inner_iterations < 1)
        return fail(CPE_BAD_ARG, "kinetic options: weights, penalties and gravity must be positive");
    for (int k = 0; k < m.nu; k++) if (m.motion_w_u[k] != 0.0) return fail(CPE_BAD_ARG, "the physics-based model replaces the constant-acceleration cost: motion_w must be zero");
    if (h->lr_window > 0) return fail(CPE_BAD_ARG, "the physics-based model does not use the autoregressive motion prior (acinoset_opt.py:905-921)");
    K.nm = d.n_motors; K.nf = d.n_feet; K.nc = 0;
    for (int j = 0; j < m.nj; j++)
        for (int t = (m.joint_kind[j] == CPE_JOINT_REVOLUTE_Y ? 0 : 1); t < 2; t++) { K.con_joint[K.nc] = j; K.con_axis[K.nc] = t == 0 ? 0 : 2; K.nc++; }
    K.nlat = K.nm + K.nc + 3 * K.nf;
    if (K.nlat > KIN_NA_MAX || K.nm + K.nc > 52) return fail(CPE_BAD_ARG, "more than 60 node forces");
    K.nrow = m.nq + 4 * K.nf + 3 * m.L;          // slack | foot heights | foot velocities (x, y, z) | second differences of the markers
    // the evaluation slots of k_dyn_eval are laid out for the reference's skeleton (KS_* in cpe_kinetic.hip.inc): anything larger is refused here,
    // not truncated there
    if (m.nq > KS_NQ || m.nl > KS_NL || m.L > KS_L || m.ns > KS_NS || m.nrev > 32 || K.nrow > KS_NROW || K.nrow > KIN_ROWS_MAX)
        return fail(CPE_BAD_ARG, "skeleton too large for the kinetic kernels (at most 54 coordinates, 17 links, 24 markers)");
    double mt = 0; for (int i = 0; i < m.nl; i++) mt += m.mass[i];
    K.Mg = mt * d.eom.gravity; K.h = m.h; K.ih = 1.0 / m.h;          // (m.h: the frame interval of the model's options)
    for (int i = 0; i < m.nl; i++) { uint32_t mask = 0; for (int j = 0; j < m.nl; j++) { int a = j; while (a >= 0 && a != i) a = m.parent[a]; if (a == i) mask |= 1u << j; } K.sub_mask[i] = mask; }
    K.grf_fix = grf_fix;
    K.grf_box = grf_box;
    K.tau_box = tau_box; K.mu_tau = h->kmut;            // (the workspace is sized before this is called)
    // ---- tables of the analytic Jacobian (k_dyn_jac): ancestry of the link pairs, moments of every subtree about its link's origin
    {
        const int nl = m.nl;
        auto is_anc = [&](int a, int i) { int j = m.parent[i]; while (j >= 0) { if (j == a) return true; j = m.parent[j]; } return false; };      // a strict ancestor of i
        auto toward = [&](int up, int down) { int j = down; while (m.parent[j] != up) j = m.parent[j]; return j; };                                 // child of `up` on the path to `down`
        K.nblk = 0;
        for (int i = 0; i < nl; i++) for (int k = 0; k < nl; k++) {
            int rel = 0, tw = 0;
            if (i == k) rel = 3;
            else if (is_anc(k, i)) { rel = 1; tw = toward(k, i); }
            else if (is_anc(i, k)) { rel = 2; tw = toward(i, k); }
            K.rel[i][k] = (int8_t)rel; K.toward[i][k] = (int8_t)tw; K.blk[i][k] = -1;
            if (rel) {
                if (K.nblk >= 96) return fail(CPE_BAD_ARG, "skeleton too deep for the kinetic kernels (more than 96 related link pairs)");
                K.blk[i][k] = (int16_t)K.nblk; K.blk_i[K.nblk] = (int8_t)i; K.blk_k[K.nblk] = (int8_t)k; K.nblk++;
            }
        }
        for (int bl = 0; bl < K.nblk; bl++) {
            const int i = K.blk_i[bl], k = K.blk_k[bl];
            K.blk_word[bl] = (uint32_t)i | ((uint32_t)k << 8) | ((uint32_t)(uint8_t)K.rel[i][k] << 16) | ((uint32_t)(uint8_t)K.toward[i][k] << 24);
            int nmo = 0, nco = 0;
            for (int mo = 0; mo < K.nm; mo++) {
                const int a1 = d.motor_first[mo], a2 = d.motor_second[mo];
                if (a1 == a2 || (i != a1 && i != a2) || (k != i && k != a1)) continue;
                if (nmo >= KJ_LMAX) return fail(CPE_BAD_ARG, "more motors on one link pair than the kinetic kernels are sized for");
                K.bm[bl][nmo++] = (uint8_t)mo;
            }
            for (int r = 0; r < K.nc; r++) {
                const int p = m.joint_parent[K.con_joint[r]], ch = m.joint_child[K.con_joint[r]];
                if (!((i == p || i == ch) && (k == p || k == ch))) continue;
                if (nco >= KJ_LMAX) return fail(CPE_BAD_ARG, "more joint equalities on one link pair than the kinetic kernels are sized for");
                K.bc[bl][nco++] = (uint8_t)r;
            }
            K.bm_n[bl] = (uint8_t)nmo; K.bc_n[bl] = (uint8_t)nco;
        }
        std::vector<double> msub(nl, 0.0);
        for (int i = 0; i < nl; i++) for (int j = 0; j < nl; j++) if (j == i || is_anc(i, j)) msub[i] += m.mass[j];
        K.mtot = mt;
        for (int i = 0; i < nl; i++) {
            for (int d = 0; d < 3; d++) K.s1[i][d] = m.mass[i] * m.com[i][d];
            for (int a = 0; a < 3; a++) for (int b2 = 0; b2 < 3; b2++) K.S2[i][3 * a + b2] = m.mass[i] * m.com[i][a] * m.com[i][b2];
            for (int c = 0; c < nl; c++) if (m.parent[c] == i) {
                for (int d = 0; d < 3; d++) K.s1[i][d] += msub[c] * m.attach[c][d];
                for (int a = 0; a < 3; a++) for (int b2 = 0; b2 < 3; b2++) K.S2[i][3 * a + b2] += msub[c] * m.attach[c][a] * m.attach[c][b2];
            }
            K.leg_of_link[i] = -1; K.hooke_of_link[i] = -1;
        }
        for (int r = 0; r < m.nrev; r++) K.leg_of_link[m.rev_child[r]] = (int8_t)r;
        K.nh = 0;
        for (int j = 0; j < m.nj; j++) if (m.joint_kind[j] == CPE_JOINT_HOOKE_YZ) {          // joints are stored parents first (cpe_model.h)
            if (K.nh >= 4) return fail(CPE_BAD_ARG, "more than four Hooke joints");
            K.hk_parent[K.nh] = (int8_t)m.joint_parent[j]; K.hk_child[K.nh] = (int8_t)m.joint_child[j]; K.hooke_of_link[m.joint_child[j]] = (int8_t)K.nh; K.nh++;
        }
    }
    for (int l = 0; l < m.L; l++) if (m.chain_len[l] > KJ_CHAIN) return fail(CPE_BAD_ARG, "skeleton too deep for the kinetic kernels (a marker more than 5 links from the root)");
    K.mu_slack = h->kmus; K.sbox = (opt->slack_hi < 1e9 || opt->slack_lo > -1e9) ? 1 : 0;
    if (K.sbox && (!(opt->kappa_slack > 0) || !(opt->slack_lo < opt->slack_hi))) return fail(CPE_BAD_ARG, "kinetic options: slack box needs lo < hi and a positive penalty");
    return CPE_OK;
}

// entry 0 of the device tables, from the handle's first model
static cpe_status build_kin(cpe_handle* h, const cpe_kinetic_options* opt, const double* grf_fix = nullptr, const double* tau_box = nullptr, const double* grf_box = nullptr) {
    if (cpe_status s = build_kin_entry(h, h->hm, opt, grf_fix, tau_box, grf_box, h->hk); s != CPE_OK) return s;
    if (!h->dk) HIPCHK(hipMalloc(&h->dk, sizeof(DevKin) * n_models(h)));
    HIPCHK(hipMemcpyAsync(h->dk, &h->hk, sizeof(DevKin), hipMemcpyHostToDevice, h->stream));
    return CPE_OK;
}

// every entry, model k under opts[k] (cpe_solve_kinetic_ragged, cpe_covariance_kinetic_ragged: `who`, for the reason of a refusal)
static cpe_status build_kin_all(cpe_handle* h, const cpe_kinetic_options* opts, const double* grf_fix, const double* tau_box, const double* grf_box,
                                const char* who = "cpe_solve_kinetic_ragged") {
    const int nmod = n_models(h);
    h->hks.resize((size_t)nmod);
    for (int k = 0; k < nmod; k++)
        if (cpe_status s = build_kin_entry(h, h->models.empty() ? h->hm : h->models[(size_t)k], &opts[k], grf_fix, tau_box, grf_box, h->hks[(size_t)k]); s != CPE_OK)
            return fail(s, std::string(who) + ": model " + std::to_string(k) + ": " + g_err);
    h->hk = h->hks[0];
    if (!h->dk) HIPCHK(hipMalloc(&h->dk, sizeof(DevKin) * nmod));
    HIPCHK(hipMemcpyAsync(h->dk, h->hks.data(), sizeof(DevKin) * nmod, hipMemcpyHostToDevice, h->stream));
    return CPE_OK;
}

// The kinetic option fields the models of one cpe_solve_kinetic_ragged call must share (include/cpe.h): they fix which node forces and rows every
// node has and the layout of stance, tau, grf and the force arrays.  Returns the first field that differs, or null.
static const char* kinetic_shape_mismatch(const cpe_kinetic_options& a, const cpe_kinetic_options& b) {
    const cpe_dyn_options &x = a.dyn, &y = b.dyn;
    auto same = [](const auto& u, const auto& v, int n) { return n <= 0 || memcmp(&u, &v, sizeof(u[0]) * (size_t)n) == 0; };
    if (x.n_feet != y.n_feet) return "dyn.n_feet";
    if (!same(x.foot_marker, y.foot_marker, std::min(x.n_feet, 4))) return "dyn.foot_marker";
    if (x.n_motors != y.n_motors) return "dyn.n_motors";
    const int nm = std::min(x.n_motors, CPE_MAX_MOTORS);
    if (!same(x.motor_first, y.motor_first, nm)) return "dyn.motor_first";
    if (!same(x.motor_second, y.motor_second, nm)) return "dyn.motor_second";
    if (!same(x.motor_axis, y.motor_axis, nm)) return "dyn.motor_axis";
    return nullptr;
}

static_assert(KE_R1 >= KS_NQ * KIN_LS && KE_R1 >= KIN_SLOT && KE_R2 >= 3 * KIN_SLOT, "regions of k_dyn_eval hold A, an evaluation slot / the three base slots");
static size_t lds_kin_eval() { return sizeof(double) * ((sizeof(KinShared) + 7) / 8 + (size_t)KE_R1 + KE_R2); }
static size_t lds_kin_assemble() { return sizeof(double) * ((size_t)KA_RC * KA_RS + (size_t)KS_NQ * KIN_LS + 2 * KS_NROW); }
static size_t lds_kin_schur() { return sizeof(double) * ((size_t)(KIN_NA_MAX + KIN_NC3) * KIN_MS + KIN_LS); }

static cpe_status ensure_kws(cpe_handle* h, int B, int N) {
    const size_t F = (size_t)B * N;
    if (F <= h->kws_frames) return CPE_OK;
    free_kws(h);
    const int BB = CPE_NX * CPE_NX;
    auto& w = h->kws_bufs;
    HIPCHK(ws_alloc(w, h->fbuf, 2 * F * KIN_LS));
    HIPCHK(ws_alloc(w, h->kmu, F * 4 * KIN_MU));
    HIPCHK(ws_alloc(w, h->kmut, F * 2 * CPE_MAX_MOTORS));
    HIPCHK(ws_alloc(w, h->kmus, F * 2 * CPE_MAX_NQ));
    HIPCHK(ws_alloc(w, h->Jbuf, F * KIN_JSTRIDE));
    HIPCHK(ws_alloc(w, h->Abuf, F * CPE_MAX_NQ * KIN_LS));
    HIPCHK(ws_alloc(w, h->pieces, 2 * F * KIN_PIECE));
    HIPCHK(ws_alloc(w, h->pmeta, 2 * F * (KIN_LS + 1)));
    HIPCHK(ws_alloc(w, h->gTb, 2 * (F + 2) * KIN_NC3));
    HIPCHK(ws_alloc(w, h->dstat, 2 * F * KIN_STAT));
    HIPCHK(ws_alloc(w, h->slackb, 2 * F * CPE_MAX_NQ));
    HIPCHK(ws_alloc(w, h->Tbuf, (F + 2) * 6 * BB));
    HIPCHK(ws_alloc(w, h->gk, F * CPE_NX));
    HIPCHK(ws_alloc(w, h->Bk, F * BB));
    HIPCHK(ws_alloc(w, h->Hk, F * 3 * BB));
    h->kws_frames = F;
    return CPE_OK;
}

// Cold start of the physics terms (after state_reset): node forces and their multipliers, those of the box on the residual and, with
// torque boxes, theirs.
static cpe_status kin_state_reset(cpe_handle* h, size_t F, bool torque_box) {
    HIPCHK(hipMemsetAsync(h->fbuf, 0, sizeof(double) * 2 * F * KIN_LS, h->stream));
    HIPCHK(hipMemsetAsync(h->kmu, 0, sizeof(double) * F * 4 * KIN_MU, h->stream));
    HIPCHK(hipMemsetAsync(h->kmus, 0, sizeof(double) * F * 2 * CPE_MAX_NQ, h->stream));
    if (torque_box) HIPCHK(hipMemsetAsync(h->kmut, 0, sizeof(double) * F * 2 * CPE_MAX_MOTORS, h->stream));
    return CPE_OK;
}

// one evaluation pass of the physics terms on the evaluated buffer (after k_frame_normal): rows, node forces, cost.
// rg: the ragged table (N = nmax), or null -- here and in the two functions below
static void launch_dyn_eval(cpe_handle* h, int N, int first, size_t Fw, const int32_t* stance, const int* act, const int* n_act, int slots, const RaggedArgs* rg) {
    const unsigned gf = (unsigned)((size_t)slots * N);
    prof_begin(h, 5);
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        hipLaunchKernelGGL(k_dyn_eval<decltype(r)::value>, dim3(gf), dim3(KIN_THREADS), lds_kin_eval(), h->stream, h->dm, h->dk, h->st, N, first, Fw, h->qbuf, stance,
                           h->fbuf, h->kmu, h->costbuf, h->Jbuf, h->Abuf, h->pieces, h->pmeta, h->dstat, h->slackb, act, n_act, a);
    });
    prof_end(h);
}
// Jacobian and second-order pieces of the CURRENT iterate -- after the accept step, and only for sequences whose iterate is new: a rejected trial
// costs its evaluation only (a quarter to a third of the iterations of a physics-based solve are rejections)
static void launch_dyn_pieces(cpe_handle* h, int N, int first, size_t Fw, const int* act, const int* n_act, int slots, const RaggedArgs* rg) {
    const unsigned gf = (unsigned)((size_t)slots * N);
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        prof_begin(h, 10);
        hipLaunchKernelGGL(k_dyn_jac<R>, dim3(gf), dim3(KJ_THREADS), sizeof(double) * KJ_DOUBLES, h->stream, h->dm, h->dk, h->st, N, first, Fw, h->qbuf, h->fbuf, h->Jbuf,
                           act, n_act, a);
        prof_end(h);
        prof_begin(h, 8);
        hipLaunchKernelGGL(k_dyn_assemble<R>, dim3(gf), dim3(KIN_THREADS), lds_kin_assemble(), h->stream, h->dm, h->dk, h->st, N, first, Fw, h->Jbuf, h->Abuf, h->pieces,
                           h->pmeta, h->gTb, act, n_act, a);
        prof_end(h);
    });
}

// One iteration of the physics-based solve: per-frame terms and physics terms of the evaluated buffer, accept / reject (new damping), elimination
// of the node forces at that damping for the CURRENT iterate, band system, factor + solve + next trial.
// xt: x* of every frame (the 3D kinematic cost, k_frame_tracked in place of k_frame_normal), or null (reprojections); tw: its full-weight
// form's per-frame arrays (W non-null), or nulls.
// back = false (cpe_covariance_kinetic): stop after k_lm_step<3, 2> -- the factor is in Lbuf and every factored sequence has back_pending = 1.
static void kin_iterate(cpe_handle* h, const LmParams& prm, int N, size_t Fw, size_t ldsn, const double* meas, const double* weight, const int32_t* stance,
                        const double* xt, const RaggedArgs* rg, int first, const int* act, const int* n_act, int slots, bool back = true,
                        TrackFull tw = TrackFull{}) {
    const unsigned gf = (unsigned)((size_t)slots * N);
    const bool plain = h->gmm_k == 0;
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        prof_begin(h, 0);
        if (xt) hipLaunchKernelGGL(frame_tracked<R>(!plain, tw.W != nullptr), dim3(gf), dim3(WAVE), ldsn, h->stream, h->dm, h->dtrack, h->st, N, first, Fw, h->qbuf, xt,
                                   h->gbuf, h->Bbuf, h->costbuf, h->mu, h->gambuf, h->pri, act, n_act, a, tw);
        else hipLaunchKernelGGL(frame_normal<R>(plain), dim3(gf), dim3(WAVE), ldsn, h->stream, h->dm, h->st, N, first, Fw, h->qbuf, meas, weight, h->gbuf, h->Bbuf,
                                h->costbuf, h->mu, h->gambuf, h->pri, act, n_act, ShutterArgs{nullptr, nullptr, nullptr}, a);
        prof_end(h);
        launch_dyn_eval(h, N, first, Fw, stance, act, n_act, slots, rg);
        prof_begin(h, 2);
        hipLaunchKernelGGL((k_lm_step<3, 1, R>), dim3(slots), dim3(LM_THREADS), 0, h->stream, h->dm, h->st, prm, first, h->qbuf, h->gbuf, h->Bbuf, h->costbuf,
                           h->Lbuf, h->zbuf, h->gtbuf, h->gambuf, nullptr, act, n_act, 2, nullptr, h->dgbuf, nullptr, 0, a);
        prof_end(h);
        launch_dyn_pieces(h, N, 0, Fw, act, n_act, slots, rg);      // (`which` = 0 also in the first pass: the accept step has just marked every sequence new)
        prof_begin(h, 9);
        hipLaunchKernelGGL(k_dyn_schur<R>, dim3(gf), dim3(KIN_THREADS), lds_kin_schur(), h->stream, h->dk, h->st, N, Fw, h->pieces, h->pmeta, h->fbuf, h->kmu, stance,
                           h->Tbuf, act, n_act, a);
        prof_end(h);
        prof_begin(h, 6);
        hipLaunchKernelGGL(k_dyn_gather<R>, dim3(gf), dim3(KIN_THREADS), 0, h->stream, h->st, N, Fw, h->gbuf, h->Bbuf, h->Tbuf, h->gTb, h->gk, h->Bk, h->Hk, act,
                           n_act, a);
        prof_end(h);
        prof_begin(h, 2);
        hipLaunchKernelGGL((k_lm_step<3, 2, R>), dim3(slots), dim3(LM_THREADS), 0, h->stream, h->dm, h->st, prm, first, h->qbuf, h->gk, h->Bk, h->costbuf,
                           h->Lbuf, h->zbuf, h->gtbuf, h->gambuf, h->Hk, act, n_act, 1, nullptr, h->dgbuf, nullptr, 0, a);
        prof_end(h);
        if (!back) return;
        prof_begin(h, 7);
        hipLaunchKernelGGL((k_lm_back<3, R>), dim3(slots), dim3(2 * WAVE), 0, h->stream, h->dm, h->st, prm, h->qbuf, h->Lbuf, h->zbuf, h->gtbuf, h->dgbuf, act, n_act, a);
        prof_end(h);
    });
}

// ---- 3D kinematic cost (cpe_solve_kinetic_tracked*) ----------------------------------------------------------------------
void cpe_default_track_weights(double w[CPE_NX]) {
    // acinoset_misc.py:531-589 (its 54 weights per relative Euler angle) restated on x, in link order: base x, y, z | base phi, theta, psi |
    // bodyF, neck: phi, theta, psi | tail0, tail1: theta, psi | leg pitches of UFL LFL HFL UFR LFR HFR UBL LBL UBR LBR HBL HBR (upper 5, lower 2,
    // hock 1).  Every roll and every leg yaw the reference weights 0; of those only bodyF phi and neck phi are entries of x.
    static const double t[CPE_NX] = {10, 10, 10, 5, 5, 5, 0, 5, 5, 0, 2, 2, 5, 5, 5, 5, 5, 2, 1, 5, 2, 1, 5, 2, 5, 2, 1, 1};
    for (int k = 0; k < CPE_NX; k++) w[k] = t[k];
}

// The tables of the tracked cost for every model of the handle: weights w (rows of CPE_NX; model k takes row min(k, rows - 1)), X^T and
// 2 X^T diag(w) X with X = dx/du of the cost view (the construction of DevPriors::Xc).  Refuses negative or non-finite weights.  w null (the
// full-weight form, which reads X^T only): weights zero.
static cpe_status build_track(cpe_handle* h, const double* w, int rows) {
    static const double zero[CPE_NX] = {};
    if (!w) { w = zero; rows = 1; }
    for (int i = 0; i < rows * CPE_NX; i++)
        if (!std::isfinite(w[i]) || w[i] < 0.0)
            return fail(CPE_BAD_ARG, "track_w: weights must be finite and non-negative (row " + std::to_string(i / CPE_NX) + ", entry " + std::to_string(i % CPE_NX) + ")");
    const int nmod = n_models(h);
    h->htrack.assign((size_t)nmod, DevTrack{});
    for (int k = 0; k < nmod; k++) {
        const DevModel& m = h->models.empty() ? h->hm : h->models[(size_t)k];
        const double* wk = w + (size_t)std::min(k, rows - 1) * CPE_NX;
        const int nu = m.nu;
        double X[CPE_NX][CPE_NX] = {};
        for (int i = 0; i < nu; i++)
            for (int side = 0; side < 2; side++) {
                const int kk = side == 0 ? i : m.rel_ref_u[i];
                if (kk < 0) continue;
                const double sgn = side == 0 ? m.rel_sign_u[i] : -m.rel_sign_u[i];
                X[i][kk] += sgn;
                const int r = m.rev_of_u[kk];
                if (r >= 0) X[i][m.rev_body_u[r][1]] += sgn;
            }
        DevTrack& T = h->htrack[(size_t)k];
        for (int i = 0; i < nu; i++) T.w[i] = wk[i];
        for (int i = 0; i < nu; i++)
            for (int j = 0; j < nu; j++) {
                T.Xt[j][i] = X[i][j];
                double a = 0.0;
                for (int p = 0; p < nu; p++) a += X[p][i] * wk[p] * X[p][j];
                T.H[i * nu + j] = 2.0 * a;
            }
    }
    if (!h->dtrack) HIPCHK(hipMalloc(&h->dtrack, sizeof(DevTrack) * nmod));
    HIPCHK(hipMemcpyAsync(h->dtrack, h->htrack.data(), sizeof(DevTrack) * nmod, hipMemcpyHostToDevice, h->stream));
    return CPE_OK;
}

// CPE_BAD_ARG unless every entry of the target's own frames (host pointer [B][N][nq]; lens: the sequences' frame counts, or null) is finite
static cpe_status check_target(const double* hq, int B, int N, int nq, const int32_t* lens) {
    for (int b = 0; b < B; b++)
        for (size_t i = 0; i < (size_t)(lens ? lens[b] : N) * nq; i++)
            if (!std::isfinite(hq[(size_t)b * N * nq + i]))
                return fail(CPE_BAD_ARG, "q_target: non-finite entry (sequence " + std::to_string(b) + ", frame " + std::to_string(i / nq) + ")");
    return CPE_OK;
}

// x* of every frame from the Euler target (device pointer [B][N][nq]) into h->xtgt.  Unless the caller has checked it on the host already
// (checked: the _host entries), the target is copied to the host and checked first (a non-finite entry is CPE_BAD_ARG, nothing launched).
// rg: the ragged table (N = nmax), or null; lens: the sequences' frame counts, or null.
static cpe_status track_target(cpe_handle* h, int B, int N, const double* q_target, const RaggedArgs* rg, const int32_t* lens, bool checked) {
    const size_t F = (size_t)B * N;
    const int nq = h->hm.nq;
    if (!checked) {
        std::vector<double> hq(F * nq);
        HIPCHK(hipMemcpyAsync(hq.data(), q_target, sizeof(double) * F * nq, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (cpe_status s = check_target(hq.data(), B, N, nq, lens); s != CPE_OK) return s;
    }
    if (F > h->xtgt_frames) {
        if (h->xtgt) (void)hipFree(h->xtgt);
        h->xtgt = nullptr; h->xtgt_frames = 0;
        HIPCHK(hipMalloc(&h->xtgt, sizeof(double) * F * CPE_NX));
        h->xtgt_frames = F;
    }
    with_ragged(rg, [&](auto r, RaggedArgs a) { hipLaunchKernelGGL(k_track_target<decltype(r)::value>, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dm, q_target, h->xtgt, a); });
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

// at most one of grf_fixed / tau_box / grf_box is given: refused under the entry's name `who`
static cpe_status one_force(const std::string& who, const double* grf_fixed, const double* tau_box, const double* grf_box) {
    if ((grf_fixed != nullptr) + (tau_box != nullptr) + (grf_box != nullptr) > 1) return fail(CPE_BAD_ARG, who + ": at most one of grf_fixed, tau_box, grf_box");
    return CPE_OK;
}

// what the tracked entries add to solve_kinetic_impl: weights (rows of CPE_NX) and the Euler target (device pointer)
// full (cpe_solve_kinetic_tracked_weighted*): W [B][N][28][28] (device pointer) in place of w
struct TrackIn { const double* w; int rows; const double* q_target; bool checked; bool full; const double* W; };   // checked: q_target checked on the host

// the per-frame blocks 2 X^T W X of the full-weight form into h->trackH (after build_track); rg: the ragged table (N = nmax), or null
static cpe_status track_blocks(cpe_handle* h, int B, int N, const double* W, const RaggedArgs* rg) {
    const size_t F = (size_t)B * N;
    if (F > h->trackH_frames) {
        if (h->trackH) (void)hipFree(h->trackH);
        h->trackH = nullptr; h->trackH_frames = 0;
        HIPCHK(hipMalloc(&h->trackH, sizeof(double) * F * CPE_NX * CPE_NX));
        h->trackH_frames = F;
    }
    with_ragged(rg, [&](auto r, RaggedArgs a) { hipLaunchKernelGGL(k_track_block<decltype(r)::value>, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dtrack, W, h->trackH, N, a); });
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

// CPE_BAD_ARG unless every W_n of the sequences' own frames (host pointer [B][N][28][28]; lens: the frame counts, or null) is finite and bit-symmetric
// with a non-negative diagonal.  (Positive semi-definiteness is not checked: the caller's contract.)
static cpe_status check_track_W(const double* W, int B, int N, const int32_t* lens) {
    constexpr size_t BB = (size_t)CPE_NX * CPE_NX;
    for (int b = 0; b < B; b++)
        for (int n = 0; n < (lens ? lens[b] : N); n++) {
            const double* w = W + ((size_t)b * N + n) * BB;
            const std::string where = " (sequence " + std::to_string(b) + ", frame " + std::to_string(n) + ")";
            for (int i = 0; i < CPE_NX; i++)
                for (int j = 0; j <= i; j++) {
                    if (!std::isfinite(w[i * CPE_NX + j]) || !std::isfinite(w[j * CPE_NX + i])) return fail(CPE_BAD_ARG, "track_W: non-finite entry" + where);
                    if (w[i * CPE_NX + j] != w[j * CPE_NX + i]) return fail(CPE_BAD_ARG, "track_W: not symmetric" + where);
                }
            for (int i = 0; i < CPE_NX; i++)
                if (w[i * CPE_NX + i] < 0.0) return fail(CPE_BAD_ARG, "track_W: negative diagonal entry" + where);
        }
    return CPE_OK;
}

// The physics-based solve of every entry point: cpe_solve_kinetic* (model == null: B sequences of N frames of the handle's first model, options
// opt[0]) and cpe_solve_kinetic_ragged (model / n_frames: host arrays of the batch, N = N_max, options opt[k] for model k).  At most one of
// grf_fixed / tau_box / grf_box is given (the entry points check it).  tr: the 3D kinematic cost in place of the reprojections (meas / weight
// may then be null together: meas_err is not written), or null.
static cpe_status solve_kinetic_impl(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames,
                                     const double* q_init, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                     const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                     double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats,
                                     const TrackIn* tr = nullptr) {
    if (!h || !opt || !q_init || !stance || !q) return fail(CPE_BAD_ARG, "null argument");
    if (!tr && (!meas || !weight)) return fail(CPE_BAD_ARG, "null argument");
    if (tr) {
        if (tr->full ? !tr->W : !tr->w) return fail(CPE_BAD_ARG, tr->full ? "track_W is null" : "track_w is null");
        if (!tr->q_target) return fail(CPE_BAD_ARG, "q_target is null");
        if (meas && !weight) return fail(CPE_BAD_ARG, "meas is given without weight");
        if (weight && !meas) return fail(CPE_BAD_ARG, "weight is given without meas");
        if (!meas) meas_err = nullptr;
    }
    if ((dq == nullptr) != (ddq == nullptr)) return fail(CPE_BAD_ARG, "dq and ddq must be given together");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const bool ragged = model != nullptr;
    std::vector<int2> seq;
    if (ragged) {           // every refusal of the batch comes before anything is launched
        if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return s;
        for (int k = 1; k < n_models(h); k++)
            if (const char* field = kinetic_shape_mismatch(opt[0], opt[k]))
                return fail(CPE_BAD_ARG, std::string("cpe_solve_kinetic_ragged: kinetic options of model ") + std::to_string(k) + " differ from model 0 in " + field);
    }
    if (h->pb != 3) return fail(CPE_BAD_ARG, "the physics-based model runs on the half-bandwidth-3 solver");
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    s = ensure_kws(h, B, N);
    if (s != CPE_OK) return s;
    s = ragged ? build_kin_all(h, opt, grf_fixed, tau_box, grf_box) : build_kin(h, opt, grf_fixed, tau_box, grf_box);
    if (s != CPE_OK) return s;
    if (tr && (s = build_track(h, tr->full ? nullptr : tr->w, tr->rows)) != CPE_OK) return s;
    const DevModel& m = h->hm;
    const size_t Fw = F;
    RaggedArgs rgv;
    if (ragged && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;     // (seq outlives the stream: drained below)
    const RaggedArgs* rg = ragged ? &rgv : nullptr;
    if (tr && (s = track_target(h, B, N, tr->q_target, rg, n_frames, tr->checked)) != CPE_OK) return s;
    if (tr && tr->full && (s = track_blocks(h, B, N, tr->W, rg)) != CPE_OK) return s;
    const TrackFull tw = tr && tr->full ? TrackFull{tr->W, h->trackH} : TrackFull{};
    if ((s = state_reset(h, B, N, q_init, rg)) != CPE_OK || (s = kin_state_reset(h, F, tau_box != nullptr)) != CPE_OK) return s;
    const LmParams prm = lm_params(h, B, N);
    const size_t ldsn = tr ? lds_tracked(h, rg) : lds_normal(h, rg);
    const double* xt = tr ? h->xtgt : nullptr;
    auto iterate = [&](int first, const int* act, const int* n_act, int slots) {
        kin_iterate(h, prm, N, Fw, ldsn, meas, weight, stance, xt, rg, first, act, n_act, slots, true, tw);
    };
    if ((s = lm_drive(h, B, iterate)) != CPE_OK) return s;
    std::vector<SeqState> hs;
    std::vector<double> hc;
    s = lm_readback(h, B, N, meas, q, dq, ddq, positions, meas_err, nullptr, [&] {
        with_ragged(rg, [&](auto r, RaggedArgs a) {
            hipLaunchKernelGGL(k_dyn_outputs<decltype(r)::value>, dim3((unsigned)F), dim3(64), 0, h->stream, h->dk, h->st, N, Fw, h->fbuf, h->Abuf, nullptr, tau, lambda, grf, a);
        });
    }, hs, hc, rg);
    if (s != CPE_OK) return s;
    auto len = [&](int b) { return ragged ? n_frames[b] : N; };          // the sequence's own frames
    // slack and the per-node statistics live in the buffer of each sequence's final iterate
    std::vector<double> hd(kstats ? 2 * F * KIN_STAT : 0);
    std::vector<int> hit(kstats ? 2 * F : 0);               // last word of every node's meta record: Newton iterations of its force solve
    if (kstats) {
        HIPCHK(hipMemcpyAsync(hd.data(), h->dstat, sizeof(double) * 2 * F * KIN_STAT, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpy2DAsync(hit.data(), sizeof(int), h->pmeta + KIN_LS, sizeof(int) * (KIN_LS + 1), sizeof(int), 2 * F, hipMemcpyDeviceToHost, h->stream));
    }
    if (slack) {
        if (ragged) HIPCHK(hipMemsetAsync(slack, 0, sizeof(double) * F * m.nq, h->stream));        // the padding rows
        for (int b = 0; b < B; b++)
            HIPCHK(hipMemcpy2DAsync(slack + (size_t)b * N * m.nq, sizeof(double) * m.nq, h->slackb + ((size_t)hs[b].cur * F + (size_t)b * N) * CPE_MAX_NQ,
                                    sizeof(double) * CPE_MAX_NQ, sizeof(double) * m.nq, len(b), hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (kstats)
        for (int b = 0; b < B; b++) {
            const SeqState& S = hs[b];
            cpe_kinetic_stats& k = kstats[b];
            memset(&k, 0, sizeof(k));
            for (int n = 0; n < len(b); n++) {
                const double* d = hd.data() + ((size_t)S.cur * F + (size_t)b * N + n) * KIN_STAT;
                k.cost_eom += d[0]; k.cost_torque += d[1]; k.cost_energy += d[3];
                k.max_slack = std::max(k.max_slack, d[5]); k.max_base_rows = std::max(k.max_base_rows, d[6]); k.max_violation = std::max(k.max_violation, d[7]);
                k.inner_max = std::max(k.inner_max, hit[(size_t)S.cur * F + (size_t)b * N + n]);
            }
        }
    return seq_stats(h, B, hs, hc, nullptr, kinetic_costs, stats);
}

cpe_status cpe_solve_kinetic(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                             const double* weight, const int32_t* stance, double* q, double* dq, double* ddq, double* positions,
                             double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats) {
    return cpe_solve_kinetic_fixed(h, opt, B, N, q_init, meas, weight, stance, nullptr, q, dq, ddq, positions, meas_err, tau, lambda, grf, slack, stats, kstats);
}
cpe_status cpe_solve_kinetic_fixed(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                                   const double* weight, const int32_t* stance, const double* grf_fixed, double* q, double* dq, double* ddq,
                                   double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                   cpe_kinetic_stats* kstats) {
    return solve_kinetic_impl(h, opt, B, N, nullptr, nullptr, q_init, meas, weight, stance, grf_fixed, nullptr, nullptr, q, dq, ddq, positions, meas_err, tau, lambda, grf, slack, stats, kstats);
}
cpe_status cpe_solve_kinetic_force_box(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                                       const double* weight, const int32_t* stance, const double* grf_box, double* q, double* dq, double* ddq,
                                       double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                       cpe_kinetic_stats* kstats) {
    if (!grf_box) return fail(CPE_BAD_ARG, "null argument");
    return solve_kinetic_impl(h, opt, B, N, nullptr, nullptr, q_init, meas, weight, stance, nullptr, nullptr, grf_box, q, dq, ddq, positions, meas_err, tau, lambda, grf, slack, stats, kstats);
}
cpe_status cpe_solve_kinetic_bounded(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                                     const double* weight, const int32_t* stance, const double* tau_box, double* q, double* dq, double* ddq,
                                     double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                     cpe_kinetic_stats* kstats) {
    if (!tau_box) return fail(CPE_BAD_ARG, "null argument");
    return solve_kinetic_impl(h, opt, B, N, nullptr, nullptr, q_init, meas, weight, stance, nullptr, tau_box, nullptr, q, dq, ddq, positions, meas_err, tau, lambda, grf, slack, stats, kstats);
}

cpe_status cpe_solve_kinetic_ragged(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames,
                                    const double* q_init, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                    const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                    double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats) {
    if (!h || !opts || !model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = one_force("cpe_solve_kinetic_ragged", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    return solve_kinetic_impl(h, opts, B, N_max, model, n_frames, q_init, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq, positions, meas_err,
                              tau, lambda, grf, slack, stats, kstats);
}

cpe_status cpe_solve_kinetic_tracked(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_w, int32_t B, int32_t N, const double* q_init,
                                     const double* q_target, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                     const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                     double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats) {
    if (cpe_status s = one_force("cpe_solve_kinetic_tracked", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    const TrackIn tr{track_w, 1, q_target, false};
    return solve_kinetic_impl(h, opt, B, N, nullptr, nullptr, q_init, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq, positions, meas_err,
                              tau, lambda, grf, slack, stats, kstats, &tr);
}

cpe_status cpe_solve_kinetic_tracked_ragged(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_w, int32_t B, int32_t N_max,
                                            const int32_t* model, const int32_t* n_frames, const double* q_init, const double* q_target, const double* meas,
                                            const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box,
                                            const double* grf_box, double* q, double* dq, double* ddq, double* positions, double* meas_err, double* tau,
                                            double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats) {
    if (!h || !opts || !model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = one_force("cpe_solve_kinetic_tracked_ragged", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    const TrackIn tr{track_w, n_models(h), q_target, false};
    return solve_kinetic_impl(h, opts, B, N_max, model, n_frames, q_init, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq, positions, meas_err,
                              tau, lambda, grf, slack, stats, kstats, &tr);
}

cpe_status cpe_solve_kinetic_tracked_weighted(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_W, int32_t B, int32_t N,
                                              const double* q_init, const double* q_target, const double* meas, const double* weight, const int32_t* stance,
                                              const double* grf_fixed, const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq,
                                              double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                              cpe_kinetic_stats* kstats) {
    if (cpe_status s = one_force("cpe_solve_kinetic_tracked_weighted", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    const TrackIn tr{nullptr, 1, q_target, false, true, track_W};
    return solve_kinetic_impl(h, opt, B, N, nullptr, nullptr, q_init, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq, positions, meas_err,
                              tau, lambda, grf, slack, stats, kstats, &tr);
}

cpe_status cpe_solve_kinetic_tracked_weighted_ragged(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_W, int32_t B, int32_t N_max,
                                                     const int32_t* model, const int32_t* n_frames, const double* q_init, const double* q_target,
                                                     const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                                     const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions,
                                                     double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                                     cpe_kinetic_stats* kstats) {
    if (!h || !opts || !model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = one_force("cpe_solve_kinetic_tracked_weighted_ragged", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    const TrackIn tr{nullptr, 1, q_target, false, true, track_W};
    return solve_kinetic_impl(h, opts, B, N_max, model, n_frames, q_init, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq, positions, meas_err,
                              tau, lambda, grf, slack, stats, kstats, &tr);
}

// W_n = (scale / 2) (X Sigma_nn X^T)^-1 of every frame (k_track_precision); model / n_frames: host arrays of a ragged batch (N = N_max), or null
cpe_status cpe_track_precision(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* cov_diag, double scale,
                               double* W) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    if (!cov_diag) return fail(CPE_BAD_ARG, "cov_diag is null");
    if (!W) return fail(CPE_BAD_ARG, "W is null");
    if (!std::isfinite(scale) || !(scale > 0.0)) return fail(CPE_BAD_ARG, "scale must be finite and > 0");
    if ((model == nullptr) != (n_frames == nullptr)) return fail(CPE_BAD_ARG, "model and n_frames are given together");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    std::vector<int2> seq;
    if (model)
        if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return s;
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK || (s = build_track(h, nullptr, 1)) != CPE_OK) return s;
    RaggedArgs rgv;
    if (model && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;
    Staging st(h->stream);
    int* bad = st.alloc<int>(F);
    HIPCHK(st.err);
    if (model) HIPCHK(hipMemsetAsync(bad, 0, sizeof(int) * F, h->stream));        // (padding frames are not visited)
    with_ragged(model ? &rgv : nullptr, [&](auto r, RaggedArgs a) {
        hipLaunchKernelGGL(k_track_precision<decltype(r)::value>, dim3((unsigned)F), dim3(WAVE), 0, h->stream, h->dtrack, cov_diag, scale, W, bad, N, a);
    });
    HIPCHK(hipGetLastError());
    std::vector<int> hbad(F);
    HIPCHK(hipMemcpyAsync(hbad.data(), bad, sizeof(int) * F, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t f = 0; f < F; f++)
        if (hbad[f])
            return fail(CPE_NUMERICAL, "cpe_track_precision: the covariance block of sequence " + std::to_string(f / (size_t)N) + ", frame " +
                                           std::to_string(f % (size_t)N) + " has no Cholesky factor (its W is zero)");
    return CPE_OK;
}

cpe_status cpe_track_precision_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* cov_diag,
                                    double scale, double* W) {
    if (!h) return fail(CPE_BAD_ARG, "null argument");
    if (!cov_diag) return fail(CPE_BAD_ARG, "cov_diag is null");
    if (!W) return fail(CPE_BAD_ARG, "W is null");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t BB = (size_t)CPE_NX * CPE_NX;
    Staging st(h->stream);
    const double* dc = st.in(cov_diag, F * BB);
    double* ow = st.out(W, F * BB);
    HIPCHK(st.err);
    if (model) HIPCHK(hipMemsetAsync(ow, 0, sizeof(double) * F * BB, h->stream));   // the padding frames
    const cpe_status s = cpe_track_precision(h, B, N, model, n_frames, dc, scale, ow);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

// cpe_eval_normal_tracked (track_w) and cpe_eval_normal_tracked_weighted (track_W, device [B][N][28][28]): exactly one of the two is given
static cpe_status eval_normal_tracked_impl(cpe_handle* h, const double* track_w, const double* track_W, int32_t B, int32_t N, const double* q,
                                           const double* q_target, double* g, double* Bm, double* cost, double* gam, double* q_out);

cpe_status cpe_eval_normal_tracked(cpe_handle* h, const double* track_w, int32_t B, int32_t N, const double* q, const double* q_target, double* g,
                                   double* Bm, double* cost, double* gam, double* q_out) {
    if (h && q && g && Bm && cost && !track_w) return fail(CPE_BAD_ARG, "track_w is null");
    return eval_normal_tracked_impl(h, track_w, nullptr, B, N, q, q_target, g, Bm, cost, gam, q_out);
}

cpe_status cpe_eval_normal_tracked_weighted(cpe_handle* h, const double* track_W, int32_t B, int32_t N, const double* q, const double* q_target, double* g,
                                            double* Bm, double* cost, double* gam, double* q_out) {
    if (h && q && g && Bm && cost && !track_W) return fail(CPE_BAD_ARG, "track_W is null");
    return eval_normal_tracked_impl(h, nullptr, track_W, B, N, q, q_target, g, Bm, cost, gam, q_out);
}

static cpe_status eval_normal_tracked_impl(cpe_handle* h, const double* track_w, const double* track_W, int32_t B, int32_t N, const double* q,
                                           const double* q_target, double* g, double* Bm, double* cost, double* gam, double* q_out) {
    if (!h || !q || !g || !Bm || !cost) return fail(CPE_BAD_ARG, "null argument");
    if (!q_target) return fail(CPE_BAD_ARG, "q_target is null");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    if ((s = build_track(h, track_w, 1)) != CPE_OK || (s = track_target(h, B, N, q_target, nullptr, nullptr, false)) != CPE_OK) return s;
    if (track_W && (s = track_blocks(h, B, N, track_W, nullptr)) != CPE_OK) return s;
    if ((s = state_reset(h, B, N, q)) != CPE_OK) return s;
    const DevModel& m = h->hm;
    hipLaunchKernelGGL(frame_tracked<>(h->gmm_k > 0, track_W != nullptr), dim3((unsigned)F), dim3(WAVE), lds_tracked(h, nullptr), h->stream, h->dm, h->dtrack, h->st,
                       N, 1, F, h->qbuf, h->xtgt, h->gbuf, h->Bbuf, h->costbuf, h->mu, h->gambuf, h->pri, nullptr, nullptr, RaggedArgs{},
                       track_W ? TrackFull{track_W, h->trackH} : TrackFull{});
    HIPCHK(hipMemcpyAsync(g, h->gbuf, sizeof(double) * F * m.nu, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(Bm, h->Bbuf, sizeof(double) * F * m.nu * m.nu, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(k_gather_normal, dim3((unsigned)F), dim3(128), 0, h->stream, h->dm, F, h->qbuf, h->costbuf, h->gambuf, cost, gam, q_out);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

// diagnostic building block (as cpe_eval_normal): one evaluation of the physics terms at Euler q, multipliers zero, forces from a cold start.
// Device pointers: f [B][N][64] node forces, stat [B][N][8], g [B][N][84], Huu [B][N][84][84], Hfu [B][N][64][84], Hff [B][N][64][64];
// meta int32 [B][N][65] = (number of free node forces, their indices).  (What ASL would hand IPOPT for the physics constraints of one node.)
cpe_status cpe_eval_kinetic_nodes(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                                  const int32_t* stance, double* f, double* stat, double* g, double* Huu, double* Hfu, double* Hff, int32_t* meta) {
    return cpe_eval_kinetic_system(h, opt, B, N, q, meas, weight, stance, nullptr, nullptr, nullptr, f, stat, g, Huu, Hfu, Hff, meta, nullptr, nullptr, nullptr);
}

// cpe_eval_kinetic_nodes with the variants of cpe_solve_kinetic_ragged (grf_fixed / tau_box / grf_box, at most one) and the band system that
// k_lm_step<3, 2> receives at the damping a solve starts with (opts.lambda0): gk [B][N][28], Bk [B][N][28][28], Hk [B][N][2][28][28] (blocks
// (m, m-1), (m, m-2)), made by k_dyn_schur and k_dyn_gather after the node pieces.
cpe_status cpe_eval_kinetic_system(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                                   const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double* f, double* stat,
                                   double* g, double* Huu, double* Hfu, double* Hff, int32_t* meta, double* gk, double* Bk, double* Hk) {
    if (!h || !opt || !q || !meas || !weight || !stance) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = one_force("cpe_eval_kinetic_system", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    if (h->pb != 3) return fail(CPE_BAD_ARG, "the physics-based model runs on the half-bandwidth-3 solver");
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);                     // the workspaces first: build_kin records pointers into them
    if (s != CPE_OK) return s;
    if ((s = ensure_kws(h, B, N)) != CPE_OK) return s;
    if ((s = build_kin(h, opt, grf_fixed, tau_box, grf_box)) != CPE_OK) return s;
    if ((s = state_reset(h, B, N, q)) != CPE_OK || (s = kin_state_reset(h, F, tau_box != nullptr)) != CPE_OK) return s;
    // the kernels write the pieces of nodes n >= 2 and their free forces only: the rest of what is copied out below is defined as zero here
    // (not left from an earlier call)
    HIPCHK(hipMemsetAsync(h->pieces, 0, sizeof(double) * F * KIN_PIECE, h->stream));
    HIPCHK(hipMemsetAsync(h->gTb, 0, sizeof(double) * F * KIN_NC3, h->stream));
    HIPCHK(hipMemsetAsync(h->dstat, 0, sizeof(double) * F * KIN_STAT, h->stream));
    const bool band = gk || Bk || Hk;
    std::vector<SeqState> hs;
    if (band) {          // state_reset has cleared every state (status 0, al_pending 0: k_dyn_schur / k_dyn_gather run); the damping is a solve's first
        hs.assign((size_t)B, SeqState{});
        for (SeqState& S : hs) S.lambda = h->opts.lambda0;
        HIPCHK(hipMemcpyAsync(h->st, hs.data(), sizeof(SeqState) * B, hipMemcpyHostToDevice, h->stream));
    }
    const DevModel& m = h->hm;
    hipLaunchKernelGGL(frame_normal<>(h->gmm_k == 0), dim3((unsigned)F), dim3(WAVE), lds_normal(h, nullptr), h->stream, h->dm, h->st, N, 1, F, h->qbuf, meas, weight,
                       h->gbuf, h->Bbuf, h->costbuf, h->mu, h->gambuf, h->pri, nullptr, nullptr, ShutterArgs{nullptr, nullptr, nullptr}, RaggedArgs{});
    launch_dyn_eval(h, N, 1, F, stance, nullptr, nullptr, B, nullptr);
    launch_dyn_pieces(h, N, 1, F, nullptr, nullptr, B, nullptr);
    if (band) {
        hipLaunchKernelGGL(k_dyn_schur<>, dim3((unsigned)F), dim3(KIN_THREADS), lds_kin_schur(), h->stream, h->dk, h->st, N, F, h->pieces, h->pmeta, h->fbuf, h->kmu,
                           stance, h->Tbuf, nullptr, nullptr, RaggedArgs{});
        hipLaunchKernelGGL(k_dyn_gather<>, dim3((unsigned)F), dim3(KIN_THREADS), 0, h->stream, h->st, N, F, h->gbuf, h->Bbuf, h->Tbuf, h->gTb, h->gk, h->Bk, h->Hk,
                           nullptr, nullptr, RaggedArgs{});
    }
    HIPCHK(hipGetLastError());
    if (f) HIPCHK(hipMemcpyAsync(f, h->fbuf, sizeof(double) * F * KIN_LS, hipMemcpyDeviceToDevice, h->stream));
    if (stat) HIPCHK(hipMemcpyAsync(stat, h->dstat, sizeof(double) * F * KIN_STAT, hipMemcpyDeviceToDevice, h->stream));
    if (g) HIPCHK(hipMemcpyAsync(g, h->gTb, sizeof(double) * F * KIN_NC3, hipMemcpyDeviceToDevice, h->stream));
    if (meta) HIPCHK(hipMemcpyAsync(meta, h->pmeta, sizeof(int) * F * (KIN_LS + 1), hipMemcpyDeviceToDevice, h->stream));
    const size_t w = sizeof(double), BB = (size_t)CPE_NX * CPE_NX;
    if (Huu) HIPCHK(hipMemcpy2DAsync(Huu, w * KIN_NC3 * KIN_NC3, h->pieces, w * KIN_PIECE, w * KIN_NC3 * KIN_NC3, F, hipMemcpyDeviceToDevice, h->stream));
    if (Hfu) HIPCHK(hipMemcpy2DAsync(Hfu, w * KIN_LS * KIN_NC3, h->pieces + KIN_NC3 * KIN_NC3, w * KIN_PIECE, w * KIN_LS * KIN_NC3, F, hipMemcpyDeviceToDevice, h->stream));
    if (Hff) HIPCHK(hipMemcpy2DAsync(Hff, w * KIN_LS * KIN_LS, h->pieces + KIN_NC3 * KIN_NC3 + KIN_LS * KIN_NC3, w * KIN_PIECE, w * KIN_LS * KIN_LS, F, hipMemcpyDeviceToDevice, h->stream));
    if (gk) HIPCHK(hipMemcpyAsync(gk, h->gk, w * F * CPE_NX, hipMemcpyDeviceToDevice, h->stream));
    if (Bk) HIPCHK(hipMemcpyAsync(Bk, h->Bk, w * F * BB, hipMemcpyDeviceToDevice, h->stream));
    if (Hk) HIPCHK(hipMemcpy2DAsync(Hk, w * 2 * BB, h->Hk, w * 3 * BB, w * 2 * BB, F, hipMemcpyDeviceToDevice, h->stream));     // (the third block is zero)
    if (band) HIPCHK(hipStreamSynchronize(h->stream));      // (hs is read by the copy above)
    return CPE_OK;
}

// The first pass of a solve from Euler q at damping lam, for the diagnostics below: cold start, what a sequence without a step leaves defined as
// zero, then the launches of lm_iterate (sh: the shutter-delay buffers, all null = off) or, with kopt, of kin_iterate.  The stream is drained; hs
// receives the sequence states, step[b] whether sequence b made a step, seq [B][8] (host) the cost terms, predicted decrease, max |delta| and status.
static cpe_status lm_first_pass(cpe_handle* h, const cpe_kinetic_options* kopt, int B, int N, const double* q, const double* meas, const double* weight,
                                const int32_t* stance, double lam, ShutterArgs sh, std::vector<SeqState>& hs, std::vector<char>& step, double* seq) {
    const size_t F = (size_t)B * N;
    cpe_status s = ensure_ws(h, B, N);                     // the workspaces first: build_kin records pointers into them
    if (s != CPE_OK) return s;
    if (kopt) {
        if ((s = ensure_kws(h, B, N)) != CPE_OK) return s;
        if ((s = build_kin(h, kopt)) != CPE_OK) return s;
    }
    if ((s = state_reset(h, B, N, q)) != CPE_OK) return s;
    if (kopt && (s = kin_state_reset(h, F, false)) != CPE_OK) return s;
    const DevModel& m = h->hm;
    const int ns = m.ns, RING = h->pb + 1;
    const size_t BB = (size_t)CPE_NX * CPE_NX, w = sizeof(double), LC = (size_t)RING * BB;
    // what a sequence without a step leaves is defined here, not left from an earlier call: g, dg, L and delta zero, trial = current
    HIPCHK(hipMemsetAsync(h->gtbuf, 0, w * F * CPE_NX, h->stream));
    HIPCHK(hipMemsetAsync(h->dgbuf, 0, w * F * CPE_NX, h->stream));
    HIPCHK(hipMemsetAsync(h->zbuf, 0, w * F * CPE_NX, h->stream));
    HIPCHK(hipMemsetAsync(h->Lbuf, 0, w * F * LC, h->stream));
    HIPCHK(hipMemcpyAsync(h->qbuf + F * ns, h->qbuf, w * F * ns, hipMemcpyDeviceToDevice, h->stream));
    LmParams prm = lm_params(h, B, N);
    prm.lambda0 = lam;                                     // the accept stage of the first pass sets S.lambda from it
    const size_t ldsn = lds_normal(h, nullptr, sh.tau != nullptr);
    if (kopt) kin_iterate(h, prm, N, F, ldsn, meas, weight, stance, nullptr, nullptr, 1, nullptr, nullptr, B);
    else lm_iterate(h, prm, N, F, ldsn, meas, weight, sh, nullptr, 1, nullptr, nullptr, B);
    HIPCHK(hipGetLastError());
    hs.resize((size_t)B);
    HIPCHK(hipMemcpyAsync(hs.data(), h->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    // a step was made where the evaluation is finite (status 0) and the factor exists: a failed factorisation multiplies the damping by 10
    step.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const SeqState& S = hs[b];
        step[b] = S.status == 0 && S.lambda == lam;
        double* o = seq + (size_t)b * 8;
        for (int t = 0; t < 5; t++) o[t] = S.terms[t];
        o[5] = S.pred; o[6] = S.maxstep; o[7] = step[b] ? CPE_OK : CPE_NUMERICAL;
        if (!step[b] && S.status == 0) {                   // partly written before the factorisation failed
            HIPCHK(hipMemsetAsync(h->gtbuf + (size_t)b * N * CPE_NX, 0, w * N * CPE_NX, h->stream));
            HIPCHK(hipMemsetAsync(h->dgbuf + (size_t)b * N * CPE_NX, 0, w * N * CPE_NX, h->stream));
            HIPCHK(hipMemsetAsync(h->zbuf + (size_t)b * N * CPE_NX, 0, w * N * CPE_NX, h->stream));
            HIPCHK(hipMemsetAsync(h->Lbuf + (size_t)b * N * LC, 0, w * N * LC, h->stream));
        }
    }
    return CPE_OK;
}

// Diagnostic (include/cpe.h): the first LM iteration of a solve from Euler q at damping lam -- the launches of the first pass of cpe_solve
// (lm_iterate) or, with kopt, of cpe_solve_kinetic (kin_iterate) -- and what k_lm_step / k_lm_back leave behind, in plain layouts.
cpe_status cpe_eval_lm_step(cpe_handle* h, const cpe_kinetic_options* kopt, int32_t B, int32_t N, const double* q, const double* meas,
                            const double* weight, const int32_t* stance, double lam, double* g, double* dg, double* L, double* delta, double* state,
                            double* seq) {
    if (!h || !q || !meas || !weight || !seq) return fail(CPE_BAD_ARG, "null argument");
    if ((kopt == nullptr) != (stance == nullptr)) return fail(CPE_BAD_ARG, "cpe_eval_lm_step: stance is given with the kinetic options, and only then");
    if (!(lam > 0.0) || !std::isfinite(lam)) return fail(CPE_BAD_ARG, "cpe_eval_lm_step: the damping must be positive and finite");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    if (kopt && h->pb != 3) return fail(CPE_BAD_ARG, "the physics-based model runs on the half-bandwidth-3 solver");
    HIPCHK(hipSetDevice(h->device));
    std::vector<SeqState> hs;
    std::vector<char> step;
    if (cpe_status s = lm_first_pass(h, kopt, B, N, q, meas, weight, stance, lam, ShutterArgs{nullptr, nullptr, nullptr}, hs, step, seq); s != CPE_OK) return s;
    const int ns = h->hm.ns;
    const size_t BB = (size_t)CPE_NX * CPE_NX, w = sizeof(double), LC = (size_t)(h->pb + 1) * BB;
    if (g) HIPCHK(hipMemcpyAsync(g, h->gtbuf, w * F * CPE_NX, hipMemcpyDeviceToDevice, h->stream));
    if (dg) HIPCHK(hipMemcpyAsync(dg, h->dgbuf, w * F * CPE_NX, hipMemcpyDeviceToDevice, h->stream));
    if (delta) HIPCHK(hipMemcpyAsync(delta, h->zbuf, w * F * CPE_NX, hipMemcpyDeviceToDevice, h->stream));
    if (state)
        for (int b = 0; b < B; b++)
            for (int t = 0; t < 2; t++) {                  // t = 0: the current buffer, 1: the trial
                const int buf = t == 0 ? hs[b].cur : 1 - hs[b].cur;
                HIPCHK(hipMemcpy2DAsync(state + ((size_t)b * N * 2 + t) * ns, w * 2 * ns, h->qbuf + ((size_t)buf * F + (size_t)b * N) * ns, w * ns, w * ns, N,
                                        hipMemcpyDeviceToDevice, h->stream));
            }
    if (L) {
        // Lbuf, column n: block 0 = L(n, n) with 1 / L[k][k] on its diagonal, block i = L(n + i, n), entries [row * 28 + col]; the plain form
        // has the true diagonal (the reciprocal of the stored one)
        std::vector<double> hl(F * LC);
        HIPCHK(hipMemcpyAsync(hl.data(), h->Lbuf, w * F * LC, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (size_t f = 0; f < F; f++)
            if (step[f / (size_t)N])
                for (int k = 0; k < CPE_NX; k++) { double& d = hl[f * LC + (size_t)k * (CPE_NX + 1)]; d = 1.0 / d; }
        HIPCHK(hipMemcpyAsync(L, hl.data(), w * F * LC, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));                // (hl is read by the copy above)
    return CPE_OK;
}

// Diagnostic (include/cpe.h): k_build_act alone, through lm_drive's launch statement, on a scratch state array that holds the given status words
// and zeros elsewhere.  act has ACT_GUARD entries past `window`, all filled with -1 first: what the kernel leaves of them is what the caller sees.
cpe_status cpe_eval_active_list(cpe_handle* h, int32_t B, int32_t window, const int32_t* status, int32_t* act, int32_t* n_act) {
    constexpr int ACT_GUARD = 64;
    if (!h) return fail(CPE_BAD_ARG, "cpe_eval_active_list: h is null");
    if (!status) return fail(CPE_BAD_ARG, "cpe_eval_active_list: status is null");
    if (!act) return fail(CPE_BAD_ARG, "cpe_eval_active_list: act is null");
    if (!n_act) return fail(CPE_BAD_ARG, "cpe_eval_active_list: n_act is null");
    if (B < 1) return fail(CPE_BAD_ARG, "cpe_eval_active_list: B = " + std::to_string(B) + " (at least 1)");
    if (window < 1) return fail(CPE_BAD_ARG, "cpe_eval_active_list: window = " + std::to_string(window) + " (at least 1)");
    if (window > 0x7fffffff - ACT_GUARD) return fail(CPE_BAD_ARG, "cpe_eval_active_list: window = " + std::to_string(window) + " is too large");
    HIPCHK(hipSetDevice(h->device));
    std::vector<SeqState> hs((size_t)B);
    memset(hs.data(), 0, sizeof(SeqState) * hs.size());
    for (int b = 0; b < B; b++) hs[b].status = status[b];
    const size_t n_out = (size_t)window + ACT_GUARD;
    Staging sg(h->stream);
    SeqState* dst = sg.in(hs.data(), hs.size());
    int32_t* dact = sg.out(act, n_out);
    int32_t* dn = sg.out(n_act, 1);
    if (sg.err != hipSuccess) return fail(CPE_HIP_ERROR, std::string("cpe_eval_active_list: ") + hipGetErrorString(sg.err));
    HIPCHK(hipMemsetAsync(dact, 0xff, sizeof(int32_t) * n_out, h->stream));          // every byte 0xff: -1 in every entry
    HIPCHK(hipMemsetAsync(dn, 0xff, sizeof(int32_t), h->stream));
    launch_build_act(h->stream, dst, B, window, dact, dn);
    HIPCHK(hipGetLastError());
    if (sg.fetch() != hipSuccess) return fail(CPE_HIP_ERROR, std::string("cpe_eval_active_list: ") + hipGetErrorString(sg.err));   // (drains the stream)
    return CPE_OK;
}

// Diagnostic (include/cpe.h): the first pass of a round of cpe_solve_shutter from Euler q at the delays tau and damping lam -- lm_iterate with the
// shutter-delay buffers, k_shutter_step, k_finalize(tau) -- and what they leave behind, in plain layouts.  The first pass does not move
// st[b].cur: k_shutter_step and k_finalize read the evaluated buffer, and the `cur` half of gx / rcb is what is copied out.
cpe_status cpe_eval_shutter_step(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, const double* tau,
                                 double lam, double* g, double* Bm, double* cost, double* gx, double* rcb, double* g_total, double* step,
                                 double* meas_err, double* seq) {
    if (!h || !q || !meas || !weight || !tau || !seq) return fail(CPE_BAD_ARG, "null argument");
    if (!(lam > 0.0) || !std::isfinite(lam)) return fail(CPE_BAD_ARG, "cpe_eval_shutter_step: the damping must be positive and finite");
    if (n_models(h) > 1) return fail(CPE_BAD_ARG, "cpe_eval_shutter_step: the shutter-delay path has no ragged form (a handle of several models)");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    const DevModel& m = h->hm;
    const int C = m.C, nu = m.nu;
    DevBuf dgx, drcb, dstep, dq;
    HIPCHK(dgx.alloc(2 * F * 6)); HIPCHK(drcb.alloc(2 * F * C * 9)); HIPCHK(dstep.alloc((size_t)B * C)); HIPCHK(dq.alloc(F * m.nq));
    std::vector<SeqState> hs;
    std::vector<char> made;
    if (cpe_status s = lm_first_pass(h, nullptr, B, N, q, meas, weight, nullptr, lam, ShutterArgs{tau, dgx.p, drcb.p}, hs, made, seq); s != CPE_OK) return s;
    hipLaunchKernelGGL(k_shutter_step, dim3(B), dim3(WAVE), 0, h->stream, h->dm, h->st, N, F, h->qbuf, drcb.p, tau, dstep.p);
    hipLaunchKernelGGL(k_finalize<>, dim3((unsigned)F), dim3(WAVE), lds_fk(m), h->stream, h->dm, h->st, N, F, h->qbuf, meas, dq.p, nullptr, nullptr, nullptr,
                       meas_err, nullptr, tau);
    HIPCHK(hipGetLastError());
    const size_t w = sizeof(double);
    for (int b = 0; b < B; b++) {                            // the per-frame buffers hold two iterates: [buffer][F][...]
        const size_t src = (size_t)hs[b].cur * F + (size_t)b * N, dst = (size_t)b * N;
        if (g) HIPCHK(hipMemcpyAsync(g + dst * nu, h->gbuf + src * nu, w * N * nu, hipMemcpyDeviceToDevice, h->stream));
        if (Bm) HIPCHK(hipMemcpyAsync(Bm + dst * nu * nu, h->Bbuf + src * nu * nu, w * N * nu * nu, hipMemcpyDeviceToDevice, h->stream));
        if (cost) HIPCHK(hipMemcpy2DAsync(cost + dst * 3, w * 3, h->costbuf + src * COST_STRIDE, w * COST_STRIDE, w * 3, N, hipMemcpyDeviceToDevice, h->stream));
        if (gx) HIPCHK(hipMemcpyAsync(gx + dst * 6, dgx.p + src * 6, w * N * 6, hipMemcpyDeviceToDevice, h->stream));
        if (rcb) HIPCHK(hipMemcpyAsync(rcb + dst * C * 9, drcb.p + src * C * 9, w * N * C * 9, hipMemcpyDeviceToDevice, h->stream));
    }
    if (g_total) HIPCHK(hipMemcpyAsync(g_total, h->gtbuf, w * F * CPE_NX, hipMemcpyDeviceToDevice, h->stream));
    if (step) HIPCHK(hipMemcpyAsync(step, dstep.p, w * B * C, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                // (the scratch buffers are freed on return)
    return CPE_OK;
}

// ---- posterior covariance of the kinematic estimate (include/cpe.h; kernels in cpe_covariance.hip.inc) --------------------------------------
// What every covariance entry refuses, before the device is touched: pb < 0 = the half-bandwidth is not known yet
static cpe_status cov_check(const char* who, int pb, double ridge) {
    if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(CPE_BAD_ARG, std::string(who) + ": ridge must be finite and >= 0");
    if (pb > 4)
        return fail(CPE_BAD_ARG, std::string(who) + ": half-bandwidth " + std::to_string(pb) + " (motion-prior window above 4) is not supported by the covariance sweep");
    return CPE_OK;
}

static cpe_status ensure_cov(cpe_handle* h, size_t F) {
    const size_t n = F * (size_t)(h->pb + 1) * CPE_NX * CPE_NX;
    if (n <= h->covG_n) return CPE_OK;
    if (h->covG) { HIPCHK(hipStreamSynchronize(h->stream)); (void)hipFree(h->covG); h->covG = nullptr; h->covG_n = 0; }
    HIPCHK(hipMalloc(&h->covG, sizeof(double) * n));
    h->covG_n = n;
    return CPE_OK;
}

// pre-pass + sweep over the factor columns Lsrc (recip: reciprocal diagonal, as in Lbuf); st: sequence states or null (all sequences)
static void cov_launch(cpe_handle* h, int B, int N, const SeqState* st, const double* Lsrc, int recip, double* cov_diag, double* cov_off,
                       const RaggedArgs* rg) {
    const unsigned gf = (unsigned)((size_t)B * N);
    auto go = [&](auto pbc) {
        with_ragged(rg, [&](auto r, RaggedArgs a) {
            constexpr int PB = decltype(pbc)::value;
            constexpr bool R = decltype(r)::value;
            hipLaunchKernelGGL((k_cov_prep<PB, R>), dim3(gf), dim3(WAVE), 0, h->stream, st, Lsrc, h->covG, N, recip, a);
            hipLaunchKernelGGL((k_lm_selinv<PB, R>), dim3(B), dim3(COV_THREADS), 0, h->stream, st, h->covG, cov_diag, cov_off, N, a);
        });
    };
    if (h->pb == 3) go(std::integral_constant<int, 3>{}); else go(std::integral_constant<int, 4>{});
}

// what the covariances of both models add after the sweep: the markers' position covariance (cov_pos, or null) and the factor columns in plain
// layout (L, or null)
static void cov_extras(cpe_handle* h, int N, size_t F, const double* cov_diag, double* cov_pos, double* L, const RaggedArgs* rg) {
    const size_t BB = (size_t)CPE_NX * CPE_NX;
    // (k_marker_cov's arrays are a subset of k_frame_normal's, plus Sigma(n,n) and one int per (marker, column) item; in both forms it is given
    // what the largest of the handle's models needs)
    const size_t ldsm = lds_normal_all(h) + sizeof(double) * BB + sizeof(int) * (size_t)(CPE_MAX_MARKERS * CPE_MAX_MCOL);
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        if (cov_pos) hipLaunchKernelGGL(k_marker_cov<R>, dim3((unsigned)F), dim3(WAVE), ldsm, h->stream, h->dm, h->st, N, F, h->qbuf, cov_diag, cov_pos, a);
        if (L) hipLaunchKernelGGL(k_cov_export<R>, dim3((unsigned)F), dim3(COV_THREADS), 0, h->stream, h->st, h->Lbuf, L, N, (int)((h->pb + 1) * BB), a);
    });
}

cpe_status cpe_covariance_supported(const cpe_priors* priors, double ridge) {
    bool use_pri;
    if (cpe_status s = check_priors(priors, &use_pri); s != CPE_OK) return s;
    const int pb = use_pri && priors->lr_window > 3 ? priors->lr_window : 3;
    if (cpe_status s = cov_check("cpe_covariance", pb, ridge); s != CPE_OK) return s;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(CPE_NO_DEVICE, "no HIP device: this library has no CPU fallback");
    return CPE_OK;
}

cpe_status cpe_band_inverse(cpe_handle* h, int32_t B, int32_t N, const double* L, double* cov_diag, double* cov_off) {
    if (!h || !L || !cov_diag) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = cov_check("cpe_band_inverse", h->pb, 0.0); s != CPE_OK) return s;
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    if (cpe_status s = ensure_cov(h, F); s != CPE_OK) return s;
    cov_launch(h, B, N, nullptr, L, 0, cov_diag, cov_off, nullptr);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

// cpe_covariance (model == nullptr) and cpe_covariance_ragged
static cpe_status covariance_impl(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q,
                                  const double* meas, const double* weight, double ridge, double* cov_diag, double* cov_off, double* cov_pos,
                                  double* L, cpe_status* status) {
    const char* who = model ? "cpe_covariance_ragged" : "cpe_covariance";
    if (cpe_status s = cov_check(who, -1, ridge); s != CPE_OK) return s;
    if (!h || !q || !meas || !weight || !cov_diag || !status || ((model == nullptr) != (n_frames == nullptr))) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = cov_check(who, h->pb, ridge); s != CPE_OK) return s;
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    std::vector<int2> seq;
    if (model) { if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return s; }
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    if ((s = ensure_cov(h, F)) != CPE_OK) return s;
    RaggedArgs rgv;
    if (model && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;     // (seq outlives the stream: it is drained below)
    const RaggedArgs* rg = model ? &rgv : nullptr;
    if ((s = state_reset(h, B, N, q, rg)) != CPE_OK) return s;
    const DevModel& m = h->hm;
    const size_t BB = (size_t)CPE_NX * CPE_NX, w = sizeof(double);
    // a sequence without a factor, and every frame past a sequence's own, has all outputs zero
    HIPCHK(hipMemsetAsync(cov_diag, 0, w * F * BB, h->stream));
    if (cov_off) HIPCHK(hipMemsetAsync(cov_off, 0, w * F * h->pb * BB, h->stream));
    if (cov_pos) HIPCHK(hipMemsetAsync(cov_pos, 0, w * F * m.L * 9, h->stream));
    // the launches of a solve's first pass up to the factor, multipliers zero, at damping ridge in place of opts.lambda0
    LmParams prm = lm_params(h, B, N);
    prm.lambda0 = ridge;
    lm_iterate(h, prm, N, F, lds_normal(h, rg), meas, weight, ShutterArgs{nullptr, nullptr, nullptr}, rg, 1, nullptr, nullptr, B, false);
    cov_launch(h, B, N, h->st, h->Lbuf, 1, cov_diag, cov_off, rg);
    cov_extras(h, N, F, cov_diag, cov_pos, L, rg);
    HIPCHK(hipGetLastError());
    std::vector<SeqState> hs((size_t)B);
    HIPCHK(hipMemcpyAsync(hs.data(), h->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    cpe_status worst = CPE_OK;
    for (int b = 0; b < B; b++) {
        status[b] = hs[b].status == 0 && hs[b].back_pending == 1 ? CPE_OK : CPE_NUMERICAL;
        if (status[b] > worst) worst = status[b];
    }
    return worst;
}

cpe_status cpe_covariance(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, double ridge,
                          double* cov_diag, double* cov_off, double* cov_pos, double* L, cpe_status* status) {
    return covariance_impl(h, B, N, nullptr, nullptr, q, meas, weight, ridge, cov_diag, cov_off, cov_pos, L, status);
}

cpe_status cpe_covariance_ragged(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q,
                                 const double* meas, const double* weight, double ridge, double* cov_diag, double* cov_off, double* cov_pos,
                                 double* L, cpe_status* status) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    return covariance_impl(h, B, N_max, model, n_frames, q, meas, weight, ridge, cov_diag, cov_off, cov_pos, L, status);
}

// host-pointer twins (stage through HBM)
static cpe_status covariance_host_impl(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q,
                                       const double* meas, const double* weight, double ridge, double* cov_diag, double* cov_off, double* cov_pos,
                                       double* L, cpe_status* status) {
    const char* who = model ? "cpe_covariance_ragged_host" : "cpe_covariance_host";
    if (cpe_status s = cov_check(who, -1, ridge); s != CPE_OK) return s;
    if (!h || !q || !meas || !weight || !cov_diag || !status) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = cov_check(who, h->pb, ridge); s != CPE_OK) return s;
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t nm = F * cams_max(h) * m.L, BB = (size_t)CPE_NX * CPE_NX;
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    double *od = st.out(cov_diag, F * BB), *oo = st.out_opt(cov_off, F * h->pb * BB), *op = st.out_opt(cov_pos, F * m.L * 9);
    double* ol = st.out_opt(L, F * (h->pb + 1) * BB);
    HIPCHK(st.err);
    const cpe_status s = covariance_impl(h, B, N, model, n_frames, dq, dmeas, dweight, ridge, od, oo, op, ol, status);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

cpe_status cpe_covariance_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, double ridge,
                               double* cov_diag, double* cov_off, double* cov_pos, double* L, cpe_status* status) {
    return covariance_host_impl(h, B, N, nullptr, nullptr, q, meas, weight, ridge, cov_diag, cov_off, cov_pos, L, status);
}

cpe_status cpe_covariance_ragged_host(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q,
                                      const double* meas, const double* weight, double ridge, double* cov_diag, double* cov_off, double* cov_pos,
                                      double* L, cpe_status* status) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    return covariance_host_impl(h, B, N_max, model, n_frames, q, meas, weight, ridge, cov_diag, cov_off, cov_pos, L, status);
}

// ---- columns of Sigma beyond the band (include/cpe.h, cpe_covariance_columns; k_cov_columns in cpe_covariance.hip.inc) -----------------------
// What both forms refuse, before the device is touched; fills F and the device's view of the call: tab = one (0, frames) pair per sequence -- zero
// frames for a sequence without an anchor, whose arrays are then not read -- followed by the B K anchors.
static cpe_status columns_check(const char* who, const cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, bool arrays, int32_t K,
                                const int32_t* anchors, size_t* F, std::vector<int>& tab) {
    const std::string w = std::string(who) + ": ";
    if (!h || !arrays || !anchors) return fail(CPE_BAD_ARG, w + "null argument (only n_frames may be null)");
    if (cpe_status s = cov_check(who, h->pb, 0.0); s != CPE_OK) return s;
    if (K < 1) return fail(CPE_BAD_ARG, w + "K must be at least 1");
    size_t FK;
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return fail(s, w + g_err);
    if (cpe_status s = frames((int32_t)*F, K, &FK); s != CPE_OK) return fail(s, w + g_err);
    tab.assign(2 * (size_t)B + (size_t)B * K, 0);
    for (int b = 0; b < B; b++) {
        const int nf = n_frames ? n_frames[b] : N;
        if (nf < 0 || nf > N) return fail(CPE_BAD_ARG, w + "frame count of sequence " + std::to_string(b) + " outside 0..N");
        bool any = false;
        for (int k = 0; k < K; k++) {
            const int a = anchors[(size_t)b * K + k];
            if (a < -1 || a >= nf)
                return fail(CPE_BAD_ARG, w + "anchor " + std::to_string(a) + " of sequence " + std::to_string(b) + " outside -1.." + std::to_string(nf - 1));
            tab[2 * (size_t)B + (size_t)b * K + k] = a;
            any = any || a >= 0;
        }
        tab[2 * (size_t)b + 1] = any ? nf : 0;
    }
    return CPE_OK;
}

// the device entry after its checks: d_tab = tab on the device
static cpe_status columns_launch(cpe_handle* h, int32_t B, int32_t N, size_t F, const int* d_tab, const double* L, const double* cov_diag,
                                 const double* cov_off, int32_t K, double* cols) {
    if (cpe_status s = ensure_cov(h, F); s != CPE_OK) return s;
    HIPCHK(hipMemsetAsync(cols, 0, sizeof(double) * F * K * CPE_NX * CPE_NX, h->stream));      // n > a, unused slots, past a sequence's frames
    const RaggedArgs rg{reinterpret_cast<const int2*>(d_tab), N, 0};
    const int* d_anchors = d_tab + 2 * (size_t)B;
    auto go = [&](auto pbc) {
        constexpr int PB = decltype(pbc)::value;
        hipLaunchKernelGGL((k_cov_prep<PB, true>), dim3((unsigned)F), dim3(WAVE), 0, h->stream, nullptr, L, h->covG, N, 0, rg);
        hipLaunchKernelGGL((k_cov_columns<PB>), dim3((unsigned)((size_t)B * K)), dim3(COV_THREADS), 0, h->stream, h->covG, cov_diag, cov_off, d_anchors, cols, N, K);
    };
    if (h->pb == 3) go(std::integral_constant<int, 3>{}); else go(std::integral_constant<int, 4>{});
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_covariance_columns(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, const double* L, const double* cov_diag,
                                  const double* cov_off, int32_t K, const int32_t* anchors, double* cols) {
    size_t F;
    std::vector<int> tab;
    if (cpe_status s = columns_check("cpe_covariance_columns", h, B, N, n_frames, L && cov_diag && cov_off && cols, K, anchors, &F, tab); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const int* d_tab = st.in(tab.data(), tab.size());
    HIPCHK(st.err);
    if (cpe_status s = columns_launch(h, B, N, F, d_tab, L, cov_diag, cov_off, K, cols); s != CPE_OK) return s;
    HIPCHK(hipStreamSynchronize(h->stream));                // (tab is pageable and the staged copy is freed on return)
    return CPE_OK;
}

cpe_status cpe_covariance_columns_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, const double* L, const double* cov_diag,
                                       const double* cov_off, int32_t K, const int32_t* anchors, double* cols) {
    size_t F;
    std::vector<int> tab;
    if (cpe_status s = columns_check("cpe_covariance_columns_host", h, B, N, n_frames, L && cov_diag && cov_off && cols, K, anchors, &F, tab); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t BB = (size_t)CPE_NX * CPE_NX;
    Staging st(h->stream);
    const int* d_tab = st.in(tab.data(), tab.size());
    const double *dl = st.in(L, F * (h->pb + 1) * BB), *dd = st.in(cov_diag, F * BB), *dof = st.in(cov_off, F * h->pb * BB);
    double* oc = st.out(cols, F * K * BB);
    HIPCHK(st.err);
    if (cpe_status s = columns_launch(h, B, N, F, d_tab, dl, dd, dof, K, oc); s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

// ---- draws from the posterior (include/cpe.h, cpe_band_sample / cpe_posterior_samples; kernels in cpe_sample.hip.inc) ------------------------
// What both forms of a sampling entry refuse about its sizes, before the device is touched and before anything that needs a handle: fills
// F = B N and FS = B N S, the sample frames (one launch grid of them at most).
static cpe_status sample_sizes(const std::string& w, int32_t B, int32_t N, int32_t S, size_t* F, size_t* FS) {
    if (S < 1) return fail(CPE_BAD_ARG, w + "S must be at least 1");
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return fail(s, w + g_err);
    if (cpe_status s = frames((int32_t)*F, S, FS); s != CPE_OK) return fail(s, w + g_err);
    return CPE_OK;
}

// cpe_band_sample's refusals, columns_check's where they apply; lens = the frame count of every sequence (n_frames, or N)
static cpe_status band_sample_check(const char* who, const cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, bool arrays, int32_t S, size_t* F,
                                    size_t* FS, std::vector<int>& lens) {
    const std::string w = std::string(who) + ": ";
    if (cpe_status s = sample_sizes(w, B, N, S, F, FS); s != CPE_OK) return s;
    lens.assign((size_t)B, N);
    for (int b = 0; n_frames && b < B; b++) {
        if (n_frames[b] < 0 || n_frames[b] > N) return fail(CPE_BAD_ARG, w + "frame count of sequence " + std::to_string(b) + " outside 0..N");
        lens[(size_t)b] = n_frames[b];
    }
    if (!h || !arrays) return fail(CPE_BAD_ARG, w + "null argument (only n_frames may be null)");
    return cov_check(who, h->pb, 0.0);
}

// the device entry after its checks: d_len = the frame counts on the device, or null (all N)
static cpe_status band_sample_launch(cpe_handle* h, int32_t B, int32_t N, size_t FS, const int* d_len, const double* L, int32_t S, const double* z,
                                     double* du) {
    HIPCHK(hipMemsetAsync(du, 0, sizeof(double) * FS * CPE_NX, h->stream));       // past a sequence's frames, and a sequence of no frames
    const unsigned grid = (unsigned)((size_t)B * ((S + WAVE - 1) / WAVE));
    if (h->pb == 3) hipLaunchKernelGGL((k_band_sample<3>), dim3(grid), dim3(2 * WAVE), 0, h->stream, L, z, du, d_len, N, S);
    else hipLaunchKernelGGL((k_band_sample<4>), dim3(grid), dim3(2 * WAVE), 0, h->stream, L, z, du, d_len, N, S);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_band_sample(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, const double* L, int32_t S, const double* z, double* du) {
    size_t F, FS;
    std::vector<int> lens;
    if (cpe_status s = band_sample_check("cpe_band_sample", h, B, N, n_frames, L && z && du, S, &F, &FS, lens); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const int* d_len = n_frames ? st.in(lens.data(), lens.size()) : nullptr;
    HIPCHK(st.err);
    if (cpe_status s = band_sample_launch(h, B, N, FS, d_len, L, S, z, du); s != CPE_OK) return s;
    if (n_frames) HIPCHK(hipStreamSynchronize(h->stream));          // (lens is pageable and the staged copy is freed on return)
    return CPE_OK;
}

cpe_status cpe_band_sample_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, const double* L, int32_t S, const double* z, double* du) {
    size_t F, FS;
    std::vector<int> lens;
    if (cpe_status s = band_sample_check("cpe_band_sample_host", h, B, N, n_frames, L && z && du, S, &F, &FS, lens); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const int* d_len = n_frames ? st.in(lens.data(), lens.size()) : nullptr;
    const double *dl = st.in(L, F * (h->pb + 1) * CPE_NX * CPE_NX), *dz = st.in(z, FS * CPE_NX);
    double* od = st.out(du, FS * CPE_NX);
    HIPCHK(st.err);
    if (cpe_status s = band_sample_launch(h, B, N, FS, d_len, dl, S, dz, od); s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

// cpe_posterior_samples' refusals; seq = the ragged table (model given), else empty
static cpe_status posterior_samples_check(const char* who, const cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames,
                                          bool arrays, int32_t S, size_t* F, size_t* FS, std::vector<int2>& seq) {
    const std::string w = std::string(who) + ": ";
    if (cpe_status s = sample_sizes(w, B, N, S, F, FS); s != CPE_OK) return s;
    if ((model == nullptr) != (n_frames == nullptr)) return fail(CPE_BAD_ARG, w + "model and n_frames are given together");
    if (!h || !arrays) return fail(CPE_BAD_ARG, w + "null argument (handle, q, du and q_s are required)");
    if (model) { if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return fail(s, w + g_err.substr(g_err.find(": ") + 2)); }
    return CPE_OK;
}

// the device entry after its checks.  The samples are B S sequences of N frames to k_finalize: their states in a scratch array of that shape, their
// sequence states zero (buffer 0), and -- ragged -- the table with every sequence's row S times.
static cpe_status posterior_samples_launch(cpe_handle* h, int32_t B, int32_t N, size_t FS, const std::vector<int2>& seq, const double* q,
                                           int32_t S, const double* du, double* q_s, double* positions_s) {
    const bool ragged = !seq.empty();
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    RaggedArgs rgv;
    if (ragged && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;
    if ((s = state_reset(h, B, N, q, ragged ? &rgv : nullptr)) != CPE_OK) return s;
    const size_t BS = (size_t)B * S;
    std::vector<int2> seqs;
    if (ragged) { seqs.resize(BS); for (size_t i = 0; i < BS; i++) seqs[i] = seq[i / (size_t)S]; }
    Staging st(h->stream);
    double* sstate = st.alloc<double>(FS * h->hm.ns);
    SeqState* sst = st.alloc<SeqState>(BS);
    const int2* d_seqs = ragged ? st.in(seqs.data(), seqs.size()) : nullptr;
    HIPCHK(st.err);
    HIPCHK(hipMemsetAsync(sst, 0, sizeof(SeqState) * BS, h->stream));
    if (ragged) HIPCHK(hipMemsetAsync(sstate, 0, sizeof(double) * FS * h->hm.ns, h->stream));      // (the padding frames: never read, kept defined)
    const RaggedArgs rgs{d_seqs, N, cams_max(h)};
    const RaggedArgs* rg = ragged ? &rgv : nullptr;
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        hipLaunchKernelGGL(k_sample_state<R>, dim3((unsigned)FS), dim3(WAVE), 0, h->stream, h->dm, h->qbuf, du, sstate, N, S, a);
        hipLaunchKernelGGL(k_finalize<R>, dim3((unsigned)FS), dim3(WAVE), lds_fk(h, rg), h->stream, h->dm, sst, N, FS, sstate, nullptr, q_s, nullptr, nullptr,
                           positions_s, nullptr, nullptr, nullptr, R ? rgs : a);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));                // (the scratch arrays are freed on return; seq and seqs are pageable)
    return CPE_OK;
}

cpe_status cpe_posterior_samples(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, int32_t S,
                                 const double* du, double* q_s, double* positions_s) {
    size_t F, FS;
    std::vector<int2> seq;
    if (cpe_status s = posterior_samples_check("cpe_posterior_samples", h, B, N, model, n_frames, q && du && q_s, S, &F, &FS, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    return posterior_samples_launch(h, B, N, FS, seq, q, S, du, q_s, positions_s);
}

cpe_status cpe_posterior_samples_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, int32_t S,
                                      const double* du, double* q_s, double* positions_s) {
    size_t F, FS;
    std::vector<int2> seq;
    if (cpe_status s = posterior_samples_check("cpe_posterior_samples_host", h, B, N, model, n_frames, q && du && q_s, S, &F, &FS, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dd = st.in(du, FS * CPE_NX);
    double *oq = st.out(q_s, FS * m.nq), *op = st.out_opt(positions_s, FS * m.L * 3);
    HIPCHK(st.err);
    if (cpe_status s = posterior_samples_launch(h, B, N, FS, seq, dq, S, dd, oq, op); s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

// ---- the reduced system of the segment-length calibration (include/cpe.h, cpe_scale_system; kernels in cpe_scale.hip.inc) -------------------
// dynamic LDS of k_scale_cross for model m and G scales (the carve of the kernel, in its order)
static size_t lds_scale(const DevModel& m, int G) {
    const size_t d = m.ns + 6 * m.nl + 2 * m.nrev + 36 * m.n_trunk + 3 * m.sv_n + CPE_MAX_SCOL * m.n_srow + 3 * m.mc_total + 3 * m.L + CAMW * m.C +
                     9 * m.L + 9 * m.nl + 2 * (size_t)(3 * m.L * G);
    return sizeof(double) * d + sizeof(int) * (size_t)(m.L * CPE_NX + m.mc_total);
}
// No model build_model accepts needs more than the 64 KB a launch may ask for without an attribute: the carve at every table's limit (leg links
// LM_MAX_REV, all links in the trunk, CPE_MAX_SDYN dynamic vectors, CPE_MAX_DEP hooke rows, CPE_MAX_MARKERS x CPE_MAX_MCOL marker columns,
// CPE_MAX_CAMS cameras, CPE_MAX_SCALES scales) is 57 304 B
static_assert(sizeof(double) * (CPE_MAX_NQ + LM_MAX_REV + 6 * CPE_MAX_LINKS + 2 * LM_MAX_REV + 36 * CPE_MAX_LINKS + 3 * CPE_MAX_SDYN + CPE_MAX_SCOL * CPE_MAX_DEP +
                                3 * CPE_MAX_MARKERS * CPE_MAX_MCOL + 3 * CPE_MAX_MARKERS + CAMW * CPE_MAX_CAMS + 9 * CPE_MAX_MARKERS + 9 * CPE_MAX_LINKS +
                                2 * 3 * CPE_MAX_MARKERS * CPE_MAX_SCALES) +
                  sizeof(int) * (CPE_MAX_MARKERS * CPE_NX + CPE_MAX_MARKERS * CPE_MAX_MCOL) <= 65536, "k_scale_cross: dynamic LDS within the default limit");

// k_scale_points (cpe_scale_cov.hip.inc) adds R_n [28][G] behind that carve, after an int of padding: 60 892 B at every limit
static size_t lds_scale_points(const DevModel& m, int G) { return lds_scale(m, G) + sizeof(int) + sizeof(double) * (size_t)(CPE_NX * G); }
static_assert(57304 + sizeof(int) + sizeof(double) * CPE_NX * CPE_MAX_SCALES <= 65536, "k_scale_points: dynamic LDS within the default limit");

// What both forms refuse, before the device is touched and in this order -- what needs no handle first: G outside 1..CPE_MAX_SCALES, a negative
// or non-finite ridge, negative sizes, model without n_frames or the reverse, a frame count outside 1..N, a null handle or array; then a
// half-bandwidth above 4 and a model index out of range.  Fills F and, for the ragged form, the table.
static cpe_status scale_check(const char* who, const cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, bool arrays,
                              double ridge, int32_t G, size_t* F, std::vector<int2>& seq) {
    const std::string w = std::string(who) + ": ";
    if (G < 1 || G > CPE_MAX_SCALES) return fail(CPE_BAD_ARG, w + "G = " + std::to_string(G) + " outside 1.." + std::to_string(CPE_MAX_SCALES));
    if (cpe_status s = cov_check(who, -1, ridge); s != CPE_OK) return s;
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return fail(s, w + g_err);
    if ((model == nullptr) != (n_frames == nullptr)) return fail(CPE_BAD_ARG, w + "model and n_frames are given together");
    for (int b = 0; n_frames && b < B; b++)
        if (n_frames[b] < 1 || n_frames[b] > N) return fail(CPE_BAD_ARG, w + "frame count of sequence " + std::to_string(b) + " outside 1..N");
    if (!h || !arrays) return fail(CPE_BAD_ARG, w + "null argument (only model and n_frames may be null)");
    if (cpe_status s = cov_check(who, h->pb, ridge); s != CPE_OK) return s;
    if (model) { if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return fail(s, w + g_err.substr(g_err.find(": ") + 2)); }
    return CPE_OK;
}

// the device entry after its checks: q .. cost are device pointers, d_attach / d_marker_off / status host.  cpe_scale_system: resp_u and resp_pos
// null.  cpe_scale_response: A, bvec, b_red and cost null (scratch here), resp_u given and resp_pos given or null; k_band_forward then leaves -Y_E as
// well, the factor goes to the plain layout (k_cov_export), k_band_sample solves L^T X = -Y_E for the G columns and k_scale_points forms resp_u and
// resp_pos.
static cpe_status scale_launch(cpe_handle* h, int32_t B, int32_t N, size_t F, const std::vector<int2>& seq, const double* q, const double* meas,
                               const double* weight, double ridge, int32_t G, const double* d_attach, const double* d_marker_off, double* A,
                               double* bvec, double* A_red, double* b_red, double* cost, cpe_status* status, double* resp_u = nullptr,
                               double* resp_pos = nullptr) {
    const bool ragged = !seq.empty();
    const int nm = n_models(h), L = h->hm.L, nl = h->hm.nl;
    size_t lds = 0;
    for (int k = 0; k < nm; k++) lds = std::max(lds, lds_scale(h->models.empty() ? h->hm : h->models[k], G));
    size_t lds_pts = 0;
    for (int k = 0; k < nm; k++) lds_pts = std::max(lds_pts, lds_scale_points(h->models.empty() ? h->hm : h->models[k], G));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    RaggedArgs rgv;
    if (ragged && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;
    const RaggedArgs* rg = ragged ? &rgv : nullptr;
    if ((s = state_reset(h, B, N, q, rg)) != CPE_OK) return s;
    // d chain_vec / d s_g of every model, by the loop that builds chain_vec
    const size_t per = (size_t)L * CPE_MAX_CHAIN * 3;
    std::vector<double> dcv((size_t)nm * G * per, 0.0);
    for (int k = 0; k < nm; k++) {
        const DevModel& m = h->models.empty() ? h->hm : h->models[k];
        for (int g = 0; g < G; g++) {
            const double(*att)[3] = reinterpret_cast<const double(*)[3]>(d_attach + ((size_t)k * G + g) * nl * 3);
            const double* off = d_marker_off + ((size_t)k * G + g) * L * 3;
            for (int l = 0; l < L; l++)
                chain_vectors(m.chain_link[l], m.chain_len[l], att, off + 3 * l, reinterpret_cast<double(*)[3]>(&dcv[((size_t)k * G + g) * per + (size_t)l * CPE_MAX_CHAIN * 3]));
        }
    }
    const int SC = scale_record(G);
    Staging sc(h->stream);
    const double* d_dcv = sc.in(dcv.data(), dcv.size());
    double* rec = sc.alloc<double>(F * SC);
    const size_t BB = (size_t)CPE_NX * CPE_NX, FG = F * (size_t)G * CPE_NX;
    double *Yneg = nullptr, *X = nullptr, *Lp = nullptr;
    int* d_len = nullptr;
    if (resp_u) {
        A = sc.alloc<double>((size_t)B * G * G); bvec = sc.alloc<double>((size_t)B * G); b_red = sc.alloc<double>((size_t)B * G); cost = sc.alloc<double>(B);
        Yneg = sc.alloc<double>(FG); X = sc.alloc<double>(FG); Lp = sc.alloc<double>(F * (h->pb + 1) * BB); d_len = sc.alloc<int>(B);
    }
    HIPCHK(sc.err);
    const size_t w = sizeof(double);
    // a sequence without a factor has all outputs zero
    if (resp_u) {
        HIPCHK(hipMemsetAsync(resp_u, 0, w * FG, h->stream));
        if (resp_pos) HIPCHK(hipMemsetAsync(resp_pos, 0, w * F * L * 3 * G, h->stream));
        HIPCHK(hipMemsetAsync(Yneg, 0, w * FG, h->stream));            // (the frames past a sequence's own: never read, kept defined)
    }
    HIPCHK(hipMemsetAsync(A, 0, w * B * G * G, h->stream));
    HIPCHK(hipMemsetAsync(A_red, 0, w * B * G * G, h->stream));
    HIPCHK(hipMemsetAsync(bvec, 0, w * B * G, h->stream));
    HIPCHK(hipMemsetAsync(b_red, 0, w * B * G, h->stream));
    HIPCHK(hipMemsetAsync(cost, 0, w * B, h->stream));
    // the first pass of cpe_covariance: the factor in Lbuf, the gradient in gtbuf
    LmParams prm = lm_params(h, B, N);
    prm.lambda0 = ridge;
    lm_iterate(h, prm, N, F, lds_normal(h, rg), meas, weight, ShutterArgs{nullptr, nullptr, nullptr}, rg, 1, nullptr, nullptr, B, false);
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        hipLaunchKernelGGL(k_scale_cross<R>, dim3((unsigned)F), dim3(WAVE), lds, h->stream, h->dm, h->st, N, F, h->qbuf, meas, weight, d_dcv, G, rec, a);
        if (h->pb == 3) hipLaunchKernelGGL((k_band_forward<3, R>), dim3(B), dim3(WAVE), 0, h->stream, h->st, h->Lbuf, h->gtbuf, h->costbuf, rec, N, F, G, A, bvec, A_red, b_red, cost, Yneg, a);
        else hipLaunchKernelGGL((k_band_forward<4, R>), dim3(B), dim3(WAVE), 0, h->stream, h->st, h->Lbuf, h->gtbuf, h->costbuf, rec, N, F, G, A, bvec, A_red, b_red, cost, Yneg, a);
        if (!resp_u) return;
        hipLaunchKernelGGL(k_response_lens<R>, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), 0, h->stream, h->st, B, N, d_len, a);
        hipLaunchKernelGGL(k_cov_export<R>, dim3((unsigned)F), dim3(COV_THREADS), 0, h->stream, h->st, h->Lbuf, Lp, N, (int)((h->pb + 1) * BB), a);
        // (X needs no zeroing: k_scale_points reads it only where k_band_sample wrote it)
        if (h->pb == 3) hipLaunchKernelGGL((k_band_sample<3>), dim3(B), dim3(2 * WAVE), 0, h->stream, Lp, Yneg, X, d_len, N, G);
        else hipLaunchKernelGGL((k_band_sample<4>), dim3(B), dim3(2 * WAVE), 0, h->stream, Lp, Yneg, X, d_len, N, G);
        hipLaunchKernelGGL(k_scale_points<R>, dim3((unsigned)F), dim3(WAVE), lds_pts, h->stream, h->dm, h->st, N, F, h->qbuf, d_dcv, G, X, resp_u, resp_pos, a);
    });
    HIPCHK(hipGetLastError());
    std::vector<SeqState> hs((size_t)B);
    HIPCHK(hipMemcpyAsync(hs.data(), h->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                // (the scratch arrays are freed on return; seq and dcv are pageable)
    cpe_status worst = CPE_OK;
    for (int b = 0; b < B; b++) {
        status[b] = hs[b].status == 0 && hs[b].back_pending == 1 ? CPE_OK : CPE_NUMERICAL;
        if (status[b] > worst) worst = status[b];
    }
    return worst;
}

cpe_status cpe_scale_system(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, const double* meas,
                            const double* weight, double ridge, int32_t G, const double* d_attach, const double* d_marker_off, double* A, double* b,
                            double* A_red, double* b_red, double* cost, cpe_status* status) {
    size_t F;
    std::vector<int2> seq;
    const bool arrays = q && meas && weight && d_attach && d_marker_off && A && b && A_red && b_red && cost && status;
    if (cpe_status s = scale_check("cpe_scale_system", h, B, N, model, n_frames, arrays, ridge, G, &F, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    return scale_launch(h, B, N, F, seq, q, meas, weight, ridge, G, d_attach, d_marker_off, A, b, A_red, b_red, cost, status);
}

cpe_status cpe_scale_system_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q,
                                 const double* meas, const double* weight, double ridge, int32_t G, const double* d_attach,
                                 const double* d_marker_off, double* A, double* b, double* A_red, double* b_red, double* cost, cpe_status* status) {
    size_t F;
    std::vector<int2> seq;
    const bool arrays = q && meas && weight && d_attach && d_marker_off && A && b && A_red && b_red && cost && status;
    if (cpe_status s = scale_check("cpe_scale_system_host", h, B, N, model, n_frames, arrays, ridge, G, &F, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t nmeas = F * cams_max(h) * m.L;
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nmeas * 2), *dweight = st.in(weight, nmeas);
    double *oA = st.out(A, (size_t)B * G * G), *ob = st.out(b, (size_t)B * G), *oAr = st.out(A_red, (size_t)B * G * G), *obr = st.out(b_red, (size_t)B * G),
           *oc = st.out(cost, (size_t)B);
    HIPCHK(st.err);
    const cpe_status s = scale_launch(h, B, N, F, seq, dq, dmeas, dweight, ridge, G, d_attach, d_marker_off, oA, ob, oAr, obr, oc, status);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

// ---- the pose covariance marginalised over the scales (include/cpe.h, cpe_scale_response / cpe_covariance_add_scales; kernels in
// cpe_scale_cov.hip.inc) ---------------------------------------------------------------------------------------------------------------------
cpe_status cpe_scale_response(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, const double* meas,
                              const double* weight, double ridge, int32_t G, const double* d_attach, const double* d_marker_off, double* A_red,
                              double* resp_u, double* resp_pos, cpe_status* status) {
    size_t F;
    std::vector<int2> seq;
    const bool arrays = q && meas && weight && d_attach && d_marker_off && A_red && resp_u && status;
    if (cpe_status s = scale_check("cpe_scale_response", h, B, N, model, n_frames, arrays, ridge, G, &F, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    return scale_launch(h, B, N, F, seq, q, meas, weight, ridge, G, d_attach, d_marker_off, nullptr, nullptr, A_red, nullptr, nullptr, status, resp_u, resp_pos);
}

cpe_status cpe_scale_response_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q,
                                   const double* meas, const double* weight, double ridge, int32_t G, const double* d_attach,
                                   const double* d_marker_off, double* A_red, double* resp_u, double* resp_pos, cpe_status* status) {
    size_t F;
    std::vector<int2> seq;
    const bool arrays = q && meas && weight && d_attach && d_marker_off && A_red && resp_u && status;
    if (cpe_status s = scale_check("cpe_scale_response_host", h, B, N, model, n_frames, arrays, ridge, G, &F, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t nmeas = F * cams_max(h) * m.L;
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nmeas * 2), *dweight = st.in(weight, nmeas);
    double *oAr = st.out(A_red, (size_t)B * G * G), *oru = st.out(resp_u, F * CPE_NX * G), *orp = st.out_opt(resp_pos, F * m.L * 3 * G);
    HIPCHK(st.err);
    const cpe_status s = scale_launch(h, B, N, F, seq, dq, dmeas, dweight, ridge, G, d_attach, d_marker_off, nullptr, nullptr, oAr, nullptr, nullptr, status, oru, orp);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

// What both forms of cpe_covariance_add_scales refuse, before the device is touched -- what needs no handle first: G outside 1..CPE_MAX_SCALES,
// negative sizes, a frame count outside 0..N, a null handle or array (n_frames may be null; cov_pos, resp_pos and cov_pos_m are null together);
// then a half-bandwidth above 4.  Fills F and lens = the frame count of every sequence.
static cpe_status add_scales_check(const char* who, const cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, int32_t G, bool arrays,
                                   int markers_given, size_t* F, std::vector<int>& lens) {
    const std::string w = std::string(who) + ": ";
    if (G < 1 || G > CPE_MAX_SCALES) return fail(CPE_BAD_ARG, w + "G = " + std::to_string(G) + " outside 1.." + std::to_string(CPE_MAX_SCALES));
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return fail(s, w + g_err);
    lens.assign((size_t)B, N);
    for (int b = 0; n_frames && b < B; b++) {
        if (n_frames[b] < 0 || n_frames[b] > N) return fail(CPE_BAD_ARG, w + "frame count of sequence " + std::to_string(b) + " outside 0..N");
        lens[(size_t)b] = n_frames[b];
    }
    if (!h || !arrays) return fail(CPE_BAD_ARG, w + "null argument (only n_frames and the three marker arrays may be null)");
    if (markers_given != 0 && markers_given != 3) return fail(CPE_BAD_ARG, w + "cov_pos, resp_pos and cov_pos_m are null together or given together");
    return cov_check(who, h->pb, 0.0);
}

// the device entry after its checks: d_len = the frame counts on the device, or null (all N)
static cpe_status add_scales_launch(cpe_handle* h, int32_t B, int32_t N, size_t F, const int* d_len, int32_t G, const double* cov_s, const double* resp_u,
                                    const double* resp_pos, const double* cov_diag, const double* cov_off, const double* cov_pos, double* cov_diag_m,
                                    double* cov_off_m, double* cov_pos_m) {
    const size_t BB = (size_t)CPE_NX * CPE_NX, w = sizeof(double);
    const int L = h->hm.L;
    // past a sequence's frames, and the blocks (n + i, n) with n + i past them
    HIPCHK(hipMemsetAsync(cov_diag_m, 0, w * F * BB, h->stream));
    HIPCHK(hipMemsetAsync(cov_off_m, 0, w * F * h->pb * BB, h->stream));
    if (cov_pos_m) HIPCHK(hipMemsetAsync(cov_pos_m, 0, w * F * L * 9, h->stream));
    hipLaunchKernelGGL(k_cov_add_scales, dim3((unsigned)F), dim3(WAVE), 0, h->stream, d_len, N, h->pb, G, L, cov_s, resp_u, resp_pos, cov_diag, cov_off, cov_pos,
                       cov_diag_m, cov_off_m, cov_pos_m);
    HIPCHK(hipGetLastError());
    return CPE_OK;
}

cpe_status cpe_covariance_add_scales(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, int32_t G, const double* cov_s, const double* resp_u,
                                     const double* resp_pos, const double* cov_diag, const double* cov_off, const double* cov_pos, double* cov_diag_m,
                                     double* cov_off_m, double* cov_pos_m) {
    size_t F;
    std::vector<int> lens;
    const bool arrays = cov_s && resp_u && cov_diag && cov_off && cov_diag_m && cov_off_m;
    const int mg = (resp_pos != nullptr) + (cov_pos != nullptr) + (cov_pos_m != nullptr);
    if (cpe_status s = add_scales_check("cpe_covariance_add_scales", h, B, N, n_frames, G, arrays, mg, &F, lens); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const int* d_len = n_frames ? st.in(lens.data(), lens.size()) : nullptr;
    HIPCHK(st.err);
    if (cpe_status s = add_scales_launch(h, B, N, F, d_len, G, cov_s, resp_u, resp_pos, cov_diag, cov_off, cov_pos, cov_diag_m, cov_off_m, cov_pos_m); s != CPE_OK)
        return s;
    if (n_frames) HIPCHK(hipStreamSynchronize(h->stream));          // (lens is pageable and the staged copy is freed on return)
    return CPE_OK;
}

cpe_status cpe_covariance_add_scales_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, int32_t G, const double* cov_s,
                                          const double* resp_u, const double* resp_pos, const double* cov_diag, const double* cov_off,
                                          const double* cov_pos, double* cov_diag_m, double* cov_off_m, double* cov_pos_m) {
    size_t F;
    std::vector<int> lens;
    const bool arrays = cov_s && resp_u && cov_diag && cov_off && cov_diag_m && cov_off_m;
    const int mg = (resp_pos != nullptr) + (cov_pos != nullptr) + (cov_pos_m != nullptr);
    if (cpe_status s = add_scales_check("cpe_covariance_add_scales_host", h, B, N, n_frames, G, arrays, mg, &F, lens); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t BB = (size_t)CPE_NX * CPE_NX, L = h->hm.L;
    Staging st(h->stream);
    const int* d_len = n_frames ? st.in(lens.data(), lens.size()) : nullptr;
    const double *dcs = st.in(cov_s, (size_t)B * G * G), *dru = st.in(resp_u, F * CPE_NX * G), *drp = st.in(resp_pos, F * L * 3 * G);
    const double *dcd = st.in(cov_diag, F * BB), *dco = st.in(cov_off, F * h->pb * BB), *dcp = st.in(cov_pos, F * L * 9);
    double *od = st.out(cov_diag_m, F * BB), *oo = st.out(cov_off_m, F * h->pb * BB), *op = st.out_opt(cov_pos_m, F * L * 9);
    HIPCHK(st.err);
    if (cpe_status s = add_scales_launch(h, B, N, F, d_len, G, dcs, dru, drp, dcd, dco, dcp, od, oo, op); s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

// ---- posterior covariance of the rates (include/cpe.h, cpe_rate_covariance; kernels in cpe_rate_cov.hip.inc) --------------------------------
// What both forms refuse, before the device is touched and in this order -- what needs no handle first: negative sizes, the ragged form's null
// model / n_frames, a null handle, q, cov_diag or cov_off, all outputs null; then a plain handle or a bad table for the ragged form, and a
// centre-of-mass output for a skeleton without a link-centre model.  Fills F and, for the ragged form, the table.
static cpe_status rate_cov_check(const char* who, bool ragged, const cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames,
                                 bool inputs, bool any_output, bool want_com, size_t* F, std::vector<int2>& seq) {
    const std::string w = std::string(who) + ": ";
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return fail(s, w + g_err);
    if (ragged && (!model || !n_frames)) return fail(CPE_BAD_ARG, w + "null model / n_frames");
    if (!h || !inputs) return fail(CPE_BAD_ARG, w + "null argument (handle, q, cov_diag and cov_off are required)");
    if (!any_output) return fail(CPE_BAD_ARG, w + "all outputs are null");
    if (ragged && h->models.empty()) return fail(CPE_BAD_ARG, w + "a plain handle has no ragged form (create it with cpe_create_multi)");
    if (ragged) { if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return fail(s, w + g_err.substr(g_err.find(": ") + 2)); }     // (its own name in place of cpe_solve_ragged's)
    if (want_com && h->cmodels.empty())
        return fail(CPE_BAD_ARG, w + "no centre-of-mass Jacobian for this skeleton (its link centres do not fit the marker tables: " + h->com_err + ")");
    return CPE_OK;
}

// cpe_rate_covariance (model == nullptr) and cpe_rate_covariance_ragged
static cpe_status rate_covariance_impl(const char* who, bool ragged, cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames,
                                       const double* q, const double* cov_diag, const double* cov_off, double* cov_du, double* cov_ddu,
                                       double* cov_vel, double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com) {
    const bool want_com = cov_com || cov_com_vel || jac_com, want_pos = cov_vel || jac_pos;
    size_t F;
    std::vector<int2> seq;
    if (cpe_status s = rate_cov_check(who, ragged, h, B, N, model, n_frames, q && cov_diag && cov_off, cov_du || cov_ddu || want_com || want_pos, want_com, &F, seq);
        s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    cpe_status s = ensure_ws(h, B, N);
    if (s != CPE_OK) return s;
    const DevModel& m = h->hm;
    const size_t BB = (size_t)CPE_NX * CPE_NX, PW = 3 * CPE_NX, wd = sizeof(double);
    // the Jacobians the caller does not take go to scratch of the handle
    const size_t need = (want_pos && !jac_pos ? F * m.L * PW : 0) + (want_com && !jac_com ? F * PW : 0);
    if (need > h->rateJ_n) {
        if (h->rateJ) { HIPCHK(hipStreamSynchronize(h->stream)); (void)hipFree(h->rateJ); h->rateJ = nullptr; h->rateJ_n = 0; }
        HIPCHK(hipMalloc(&h->rateJ, wd * need));
        h->rateJ_n = need;
    }
    double* jp = !want_pos ? nullptr : jac_pos ? jac_pos : h->rateJ;
    double* jc = !want_com ? nullptr : jac_com ? jac_com : h->rateJ + (want_pos && !jac_pos ? F * m.L * PW : 0);
    RaggedArgs rgv;
    if (ragged && (s = ragged_upload(h, seq, N, rgv)) != CPE_OK) return s;     // (seq outlives the stream: it is drained below)
    const RaggedArgs* rg = ragged ? &rgv : nullptr;
    if ((s = state_reset(h, B, N, q, rg)) != CPE_OK) return s;
    // everything that is defined as zero -- past a sequence's frames, row 0 of the velocities, the short sequences, the columns a point does not
    // depend on -- is zero from here; the kernels write the rest
    if (jp) HIPCHK(hipMemsetAsync(jp, 0, wd * F * m.L * PW, h->stream));
    if (jc) HIPCHK(hipMemsetAsync(jc, 0, wd * F * PW, h->stream));
    if (cov_du) HIPCHK(hipMemsetAsync(cov_du, 0, wd * F * BB, h->stream));
    if (cov_ddu) HIPCHK(hipMemsetAsync(cov_ddu, 0, wd * F * BB, h->stream));
    if (cov_vel) HIPCHK(hipMemsetAsync(cov_vel, 0, wd * F * m.L * 9, h->stream));
    if (cov_com) HIPCHK(hipMemsetAsync(cov_com, 0, wd * F * 9, h->stream));
    if (cov_com_vel) HIPCHK(hipMemsetAsync(cov_com_vel, 0, wd * F * 9, h->stream));
    const unsigned gf = (unsigned)F;
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        constexpr bool R = decltype(r)::value;
        if (jp || jc) hipLaunchKernelGGL(k_point_jac<R>, dim3(gf), dim3(WAVE), wd * PJ_LDS_DOUBLES, h->stream, h->dm, h->dmc, N, h->qbuf, jp, jc, a);
        if (cov_du || cov_ddu || cov_vel || cov_com || cov_com_vel) {
            const size_t lds = wd * (3 * BB + 2 * PW * m.L + 2 * PW);       // (at most 63168 bytes, CPE_MAX_MARKERS = 32)
            hipLaunchKernelGGL(k_rate_cov<R>, dim3(gf), dim3(WAVE), lds, h->stream, h->dm, N, h->pb, cov_diag, cov_off, jp, jc, cov_du, cov_ddu, cov_vel, cov_com,
                               cov_com_vel, a);
        }
    });
    HIPCHK(hipGetLastError());
    if (ragged) HIPCHK(hipStreamSynchronize(h->stream));
    return CPE_OK;
}

cpe_status cpe_rate_covariance(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* cov_diag, const double* cov_off, double* cov_du,
                               double* cov_ddu, double* cov_vel, double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com) {
    return rate_covariance_impl("cpe_rate_covariance", false, h, B, N, nullptr, nullptr, q, cov_diag, cov_off, cov_du, cov_ddu, cov_vel, cov_com, cov_com_vel,
                                jac_pos, jac_com);
}

cpe_status cpe_rate_covariance_ragged(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q,
                                      const double* cov_diag, const double* cov_off, double* cov_du, double* cov_ddu, double* cov_vel,
                                      double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com) {
    return rate_covariance_impl("cpe_rate_covariance_ragged", true, h, B, N_max, model, n_frames, q, cov_diag, cov_off, cov_du, cov_ddu, cov_vel, cov_com,
                                cov_com_vel, jac_pos, jac_com);
}

// host-pointer twins (stage through HBM); refused on the host pointers, before anything is staged
static cpe_status rate_covariance_host_impl(const char* who, bool ragged, cpe_handle* h, int32_t B, int32_t N, const int32_t* model,
                                            const int32_t* n_frames, const double* q, const double* cov_diag, const double* cov_off, double* cov_du,
                                            double* cov_ddu, double* cov_vel, double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com) {
    size_t F;
    std::vector<int2> seq;
    if (cpe_status s = rate_cov_check(who, ragged, h, B, N, model, n_frames, q && cov_diag && cov_off,
                                      cov_du || cov_ddu || cov_vel || cov_com || cov_com_vel || jac_pos || jac_com, cov_com || cov_com_vel || jac_com, &F, seq);
        s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t BB = (size_t)CPE_NX * CPE_NX, PW = 3 * CPE_NX;
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dd = st.in(cov_diag, F * BB), *dof = st.in(cov_off, F * h->pb * BB);
    double *odu = st.out_opt(cov_du, F * BB), *oddu = st.out_opt(cov_ddu, F * BB), *ov = st.out_opt(cov_vel, F * m.L * 9);
    double *oc = st.out_opt(cov_com, F * 9), *ocv = st.out_opt(cov_com_vel, F * 9), *ojp = st.out_opt(jac_pos, F * m.L * PW), *ojc = st.out_opt(jac_com, F * PW);
    HIPCHK(st.err);
    const cpe_status s = rate_covariance_impl(who, ragged, h, B, N, model, n_frames, dq, dd, dof, odu, oddu, ov, oc, ocv, ojp, ojc);
    if (s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return s;
}

cpe_status cpe_rate_covariance_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* cov_diag, const double* cov_off,
                                    double* cov_du, double* cov_ddu, double* cov_vel, double* cov_com, double* cov_com_vel, double* jac_pos,
                                    double* jac_com) {
    return rate_covariance_host_impl("cpe_rate_covariance_host", false, h, B, N, nullptr, nullptr, q, cov_diag, cov_off, cov_du, cov_ddu, cov_vel, cov_com,
                                     cov_com_vel, jac_pos, jac_com);
}

cpe_status cpe_rate_covariance_ragged_host(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q,
                                           const double* cov_diag, const double* cov_off, double* cov_du, double* cov_ddu, double* cov_vel,
                                           double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com) {
    return rate_covariance_host_impl("cpe_rate_covariance_ragged_host", true, h, B, N_max, model, n_frames, q, cov_diag, cov_off, cov_du, cov_ddu, cov_vel,
                                     cov_com, cov_com_vel, jac_pos, jac_com);
}

// ---- posterior covariance of the physics-based estimate (include/cpe.h, cpe_covariance_kinetic; kernel in cpe_force_cov.hip.inc) -------------
static cpe_status cov_kinetic_check(const char* who, const cpe_handle* h, const cpe_kinetic_options* opt, const int32_t* stance, const double* grf_fixed,
                                    const double* tau_box, const double* grf_box, double ridge) {
    if (cpe_status s = cov_check(who, -1, ridge); s != CPE_OK) return s;
    if (!opt) return fail(CPE_BAD_ARG, std::string(who) + ": null kinetic options");
    if (!stance) return fail(CPE_BAD_ARG, std::string(who) + ": null stance");
    if (cpe_status s = one_force(who, grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    if (h && h->pb != 3)
        return fail(CPE_BAD_ARG, std::string(who) + ": half-bandwidth " + std::to_string(h->pb) + ": the physics-based model runs on the half-bandwidth-3 solver");
    return CPE_OK;
}

// What the ragged pair refuses of its batch, before the device is touched: the (model, frames) table and kinetic options of different shape
static cpe_status cov_kinetic_batch(const char* who, const cpe_handle* h, const cpe_kinetic_options* opt, int B, int N_max, const int32_t* model,
                                    const int32_t* n_frames, std::vector<int2>& seq) {
    if (cpe_status s = ragged_table(h, B, N_max, model, n_frames, seq); s != CPE_OK) return s;
    for (int k = 1; k < n_models(h); k++)
        if (const char* field = kinetic_shape_mismatch(opt[0], opt[k]))
            return fail(CPE_BAD_ARG, std::string(who) + ": kinetic options of model " + std::to_string(k) + " differ from model 0 in " + field);
    return CPE_OK;
}

// What both forms of cpe_covariance_kinetic* refuse, in this order: cov_kinetic_check's, a null handle or array (`arrays`: the entry's required
// ones), the sizes, the ragged batch.  Fills F (0: nothing to do) and, for the ragged form, the table.  (force_samples_check runs the same pieces
// with its sample sizes ahead of what needs a handle.)
static cpe_status kin_cov_args(const char* who, const cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model,
                               const int32_t* n_frames, bool arrays, const int32_t* stance, const double* grf_fixed, const double* tau_box,
                               const double* grf_box, double ridge, size_t* F, std::vector<int2>& seq) {
    if (cpe_status s = cov_kinetic_check(who, h, opt, stance, grf_fixed, tau_box, grf_box, ridge); s != CPE_OK) return s;
    if (!h || !arrays) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = frames(B, N, F); s != CPE_OK) return s;
    if (*F == 0 || !model) return CPE_OK;
    return cov_kinetic_batch(who, h, opt, B, N, model, n_frames, seq);
}

// The first pass both entries run at Euler q: workspaces, model tables, cold-start state, one flag per sequence for the node kernel (kin_cov_setup),
// then the launches of the physics solve's first pass up to the band factor, multipliers zero, at damping ridge in place of opts.lambda0
// (kin_cov_pass); after the entry's own kernels, the status of every sequence (kin_cov_status).
struct KinCovPass {
    RaggedArgs rgv;
    const RaggedArgs* rg = nullptr;
    DevBuf bad_buf;
    int* bad = nullptr;                // [B]: a node's force matrix has no Cholesky factor
};
static cpe_status kin_cov_setup(const char* who, cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, size_t F, const std::vector<int2>& seq,
                                const double* q, const double* grf_fixed, const double* tau_box, const double* grf_box, KinCovPass& kp) {
    const bool ragged = !seq.empty();
    cpe_status s = ensure_ws(h, B, N);                     // the workspaces first: build_kin records pointers into them
    if (s != CPE_OK) return s;
    if ((s = ensure_kws(h, B, N)) != CPE_OK || (s = ensure_cov(h, F)) != CPE_OK) return s;
    if ((s = ragged ? build_kin_all(h, opt, grf_fixed, tau_box, grf_box, who) : build_kin(h, opt, grf_fixed, tau_box, grf_box)) != CPE_OK) return s;
    if (ragged && (s = ragged_upload(h, seq, N, kp.rgv)) != CPE_OK) return s;     // (seq outlives the stream: drained by kin_cov_status)
    kp.rg = ragged ? &kp.rgv : nullptr;
    if ((s = state_reset(h, B, N, q, kp.rg)) != CPE_OK || (s = kin_state_reset(h, F, tau_box != nullptr)) != CPE_OK) return s;
    HIPCHK(kp.bad_buf.alloc(((size_t)B + 1) / 2));
    kp.bad = reinterpret_cast<int*>(kp.bad_buf.p);
    HIPCHK(hipMemsetAsync(kp.bad, 0, sizeof(int) * B, h->stream));
    return CPE_OK;
}
static void kin_cov_pass(cpe_handle* h, int32_t B, int32_t N, size_t F, const double* meas, const double* weight, const int32_t* stance, double ridge,
                         const KinCovPass& kp) {
    LmParams prm = lm_params(h, B, N);
    prm.lambda0 = ridge;
    kin_iterate(h, prm, N, F, lds_normal(h, kp.rg), meas, weight, stance, nullptr, kp.rg, 1, nullptr, nullptr, B, false);
}
// drains the stream; status[b], the worst of them, and wipe[b] = the band of sequence b has a factor but one of its nodes has none: what the
// kernels wrote for it is to be cleared by the entry (a sequence without a band factor has been written by no kernel)
static cpe_status kin_cov_status(cpe_handle* h, int32_t B, const KinCovPass& kp, cpe_status* status, std::vector<char>& wipe, cpe_status* worst) {
    std::vector<SeqState> hs((size_t)B);
    std::vector<int> hbad((size_t)B);
    HIPCHK(hipMemcpyAsync(hs.data(), h->st, sizeof(SeqState) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(hbad.data(), kp.bad, sizeof(int) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    wipe.assign((size_t)B, 0);
    *worst = CPE_OK;
    for (int b = 0; b < B; b++) {
        const bool band_ok = hs[b].status == 0 && hs[b].back_pending == 1;
        status[b] = band_ok && !hbad[b] ? CPE_OK : CPE_NUMERICAL;
        if (status[b] > *worst) *worst = status[b];
        wipe[(size_t)b] = band_ok && hbad[b];
    }
    return CPE_OK;
}

// cpe_covariance_kinetic (model == null: B sequences of N frames of the handle's first model, options opt[0]) and cpe_covariance_kinetic_ragged
// (model / n_frames: host arrays of the batch, N = N_max, options opt[k] for model k)
static cpe_status covariance_kinetic_impl(const char* who, cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model,
                                          const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                          const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, double* cov_diag,
                                          double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L, cpe_status* status) {
    size_t F;
    std::vector<int2> seq;
    if (cpe_status s = kin_cov_args(who, h, opt, B, N, model, n_frames, q && meas && weight && cov_diag && status, stance, grf_fixed, tau_box, grf_box, ridge, &F, seq);
        s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    KinCovPass kp;
    if (cpe_status s = kin_cov_setup(who, h, opt, B, N, F, seq, q, grf_fixed, tau_box, grf_box, kp); s != CPE_OK) return s;
    const RaggedArgs* rg = kp.rg;
    const DevModel& m = h->hm;
    const size_t BB = (size_t)CPE_NX * CPE_NX, w = sizeof(double), LC = 4 * BB, FF = (size_t)KIN_LS * KIN_LS;
    // k_force_cov reads the off-diagonal blocks of the band whether the caller wants them or not
    DevBuf off_own;
    if (!cov_off) { HIPCHK(off_own.alloc(F * 3 * BB)); cov_off = off_own.p; }
    // a sequence without a factor has all outputs zero, and so have the nodes 0 and 1 in cov_f, f and meta and every frame past a sequence's own
    HIPCHK(hipMemsetAsync(cov_diag, 0, w * F * BB, h->stream));
    HIPCHK(hipMemsetAsync(cov_off, 0, w * F * 3 * BB, h->stream));
    if (cov_pos) HIPCHK(hipMemsetAsync(cov_pos, 0, w * F * m.L * 9, h->stream));
    if (cov_f) HIPCHK(hipMemsetAsync(cov_f, 0, w * F * FF, h->stream));
    if (f) HIPCHK(hipMemsetAsync(f, 0, w * F * KIN_LS, h->stream));
    if (meta) HIPCHK(hipMemsetAsync(meta, 0, sizeof(int32_t) * F * (KIN_LS + 1), h->stream));
    kin_cov_pass(h, B, N, F, meas, weight, stance, ridge, kp);
    cov_launch(h, B, N, h->st, h->Lbuf, 1, cov_diag, cov_off, rg);
    // (without cov_f the kernel still decides whether every node's force matrix has a factor: the status does not depend on what is asked for)
    with_ragged(rg, [&](auto r, RaggedArgs a) {
        hipLaunchKernelGGL(k_force_cov<decltype(r)::value>, dim3((unsigned)F), dim3(KIN_THREADS), sizeof(double) * FC_DOUBLES, h->stream, h->dk, h->st, N, F, h->pieces,
                           h->pmeta, h->fbuf, h->kmu, stance, cov_diag, cov_off, cov_f, f, meta, kp.bad, a);
    });
    cov_extras(h, N, F, cov_diag, cov_pos, L, rg);
    HIPCHK(hipGetLastError());
    std::vector<char> wipe;
    cpe_status worst;
    if (cpe_status s = kin_cov_status(h, B, kp, status, wipe, &worst); s != CPE_OK) return s;
    for (int b = 0; b < B; b++) {
        if (wipe[(size_t)b]) {                              // a node's force matrix has no factor: what the band kernels wrote goes too
            const size_t o = (size_t)b * N;
            HIPCHK(hipMemsetAsync(cov_diag + o * BB, 0, w * N * BB, h->stream));
            if (!off_own.p) HIPCHK(hipMemsetAsync(cov_off + o * 3 * BB, 0, w * N * 3 * BB, h->stream));
            if (cov_pos) HIPCHK(hipMemsetAsync(cov_pos + o * m.L * 9, 0, w * N * m.L * 9, h->stream));
            if (cov_f) HIPCHK(hipMemsetAsync(cov_f + o * FF, 0, w * N * FF, h->stream));
            if (f) HIPCHK(hipMemsetAsync(f + o * KIN_LS, 0, w * N * KIN_LS, h->stream));
            if (meta) HIPCHK(hipMemsetAsync(meta + o * (KIN_LS + 1), 0, sizeof(int32_t) * N * (KIN_LS + 1), h->stream));
            if (L) HIPCHK(hipMemsetAsync(L + o * LC, 0, w * N * LC, h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));                // (the buffers of this call are freed on return)
    return worst;
}

cpe_status cpe_covariance_kinetic(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                  const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                                  double ridge, double* cov_diag, double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L,
                                  cpe_status* status) {
    return covariance_kinetic_impl("cpe_covariance_kinetic", h, opt, B, N, nullptr, nullptr, q, meas, weight, stance, grf_fixed, tau_box, grf_box, ridge,
                                   cov_diag, cov_off, cov_pos, cov_f, f, meta, L, status);
}

cpe_status cpe_covariance_kinetic_ragged(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model,
                                         const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                         const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, double* cov_diag,
                                         double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L, cpe_status* status) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "cpe_covariance_kinetic_ragged: null model / n_frames");
    return covariance_kinetic_impl("cpe_covariance_kinetic_ragged", h, opts, B, N_max, model, n_frames, q, meas, weight, stance, grf_fixed, tau_box, grf_box,
                                   ridge, cov_diag, cov_off, cov_pos, cov_f, f, meta, L, status);
}

// host-pointer twins (stage through HBM): cpe_covariance_kinetic_host (model == null) and cpe_covariance_kinetic_ragged_host
static cpe_status covariance_kinetic_host_impl(const char* who, cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model,
                                               const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                               const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, double* cov_diag,
                                               double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L, cpe_status* status) {
    size_t F;
    std::vector<int2> seq;  // (refused here too: before anything is staged)
    if (cpe_status s = kin_cov_args(who, h, opt, B, N, model, n_frames, q && meas && weight && cov_diag && status, stance, grf_fixed, tau_box, grf_box, ridge, &F, seq);
        s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const int nf = opt->dyn.n_feet, nmot = opt->dyn.n_motors;
    const size_t nm = F * cams_max(h) * m.L, BB = (size_t)CPE_NX * CPE_NX, FF = (size_t)KIN_LS * KIN_LS;
    const double* var = grf_fixed ? grf_fixed : (tau_box ? tau_box : grf_box);
    const size_t nvar = grf_fixed ? F * nf * 3 : (tau_box ? F * nmot * 2 : (grf_box ? F * nf * 6 : 0));
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    const int32_t* dstance = st.in(stance, F * nf);
    const double* dvar = st.in(var, nvar);
    double *od = st.out(cov_diag, F * BB), *oo = st.out_opt(cov_off, F * 3 * BB), *op = st.out_opt(cov_pos, F * m.L * 9);
    double *oc = st.out_opt(cov_f, F * FF), *of = st.out_opt(f, F * KIN_LS), *ol = st.out_opt(L, F * 4 * BB);
    int32_t* ometa = st.out_opt(meta, F * (KIN_LS + 1));
    HIPCHK(st.err);
    const cpe_status s = covariance_kinetic_impl(model ? "cpe_covariance_kinetic_ragged" : "cpe_covariance_kinetic", h, opt, B, N, model, n_frames, dq, dmeas,
                                                 dweight, dstance, grf_fixed ? dvar : nullptr, tau_box ? dvar : nullptr, grf_box ? dvar : nullptr, ridge, od,
                                                 oo, op, oc, of, ometa, ol, status);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

cpe_status cpe_covariance_kinetic_host(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                       const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box,
                                       const double* grf_box, double ridge, double* cov_diag, double* cov_off, double* cov_pos, double* cov_f, double* f,
                                       int32_t* meta, double* L, cpe_status* status) {
    return covariance_kinetic_host_impl("cpe_covariance_kinetic_host", h, opt, B, N, nullptr, nullptr, q, meas, weight, stance, grf_fixed, tau_box, grf_box,
                                        ridge, cov_diag, cov_off, cov_pos, cov_f, f, meta, L, status);
}

cpe_status cpe_covariance_kinetic_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model,
                                              const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                              const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, double* cov_diag,
                                              double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L, cpe_status* status) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "cpe_covariance_kinetic_ragged_host: null model / n_frames");
    return covariance_kinetic_host_impl("cpe_covariance_kinetic_ragged_host", h, opts, B, N_max, model, n_frames, q, meas, weight, stance, grf_fixed, tau_box,
                                        grf_box, ridge, cov_diag, cov_off, cov_pos, cov_f, f, meta, L, status);
}

// ---- draws of the node forces of the physics-based estimate (include/cpe.h, cpe_force_samples; kernel in cpe_force_sample.hip.inc) -----------
// What both forms refuse, before the device is touched: cpe_covariance_kinetic's refusals, a null du or f_s, S < 1, too many sample frames.
// Fills F = B N, FS = B N S and, for the ragged form, the table.
static cpe_status force_samples_check(const char* who, const cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model,
                                      const int32_t* n_frames, bool arrays, const int32_t* stance, const double* grf_fixed, const double* tau_box,
                                      const double* grf_box, double ridge, int32_t S, const double* du, const double* f_s, size_t* F, size_t* FS,
                                      std::vector<int2>& seq) {
    if (cpe_status s = cov_kinetic_check(who, h, opt, stance, grf_fixed, tau_box, grf_box, ridge); s != CPE_OK) return s;
    if (!du || !f_s) return fail(CPE_BAD_ARG, std::string(who) + ": null du / f_s");
    if (cpe_status s = sample_sizes(std::string(who) + ": ", B, N, S, F, FS); s != CPE_OK) return s;
    if (!h || !arrays) return fail(CPE_BAD_ARG, "null argument");                  // (what needs a handle last)
    if (*F == 0 || !model) return CPE_OK;
    return cov_kinetic_batch(who, h, opt, B, N, model, n_frames, seq);
}

// cpe_force_samples (model == null) and cpe_force_samples_ragged: the first pass of covariance_kinetic_impl, then k_force_sample on its pieces
static cpe_status force_samples_impl(const char* who, cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model,
                                     const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                     const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, int32_t S, const double* du,
                                     const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status) {
    size_t F, FS;
    std::vector<int2> seq;
    if (cpe_status s = force_samples_check(who, h, opt, B, N, model, n_frames, q && meas && weight && status, stance, grf_fixed, tau_box, grf_box, ridge, S, du,
                                           f_s, &F, &FS, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    HIPCHK(hipSetDevice(h->device));
    KinCovPass kp;
    if (cpe_status s = kin_cov_setup(who, h, opt, B, N, F, seq, q, grf_fixed, tau_box, grf_box, kp); s != CPE_OK) return s;
    const size_t w = sizeof(double);
    // a sequence without a factor has all outputs zero, and so have the nodes 0 and 1 and every frame past a sequence's own
    HIPCHK(hipMemsetAsync(f_s, 0, w * FS * KIN_LS, h->stream));
    if (f) HIPCHK(hipMemsetAsync(f, 0, w * F * KIN_LS, h->stream));
    if (meta) HIPCHK(hipMemsetAsync(meta, 0, sizeof(int32_t) * F * (KIN_LS + 1), h->stream));
    kin_cov_pass(h, B, N, F, meas, weight, stance, ridge, kp);
    with_ragged(kp.rg, [&](auto r, RaggedArgs a) {
        hipLaunchKernelGGL(k_force_sample<decltype(r)::value>, dim3((unsigned)F), dim3(KIN_THREADS), sizeof(double) * FS_DOUBLES, h->stream, h->dk, h->st, N, F,
                           h->pieces, h->pmeta, h->fbuf, h->kmu, stance, S, du, zeta, f_s, f, meta, kp.bad, a);
    });
    HIPCHK(hipGetLastError());
    std::vector<char> wipe;
    cpe_status worst;
    if (cpe_status s = kin_cov_status(h, B, kp, status, wipe, &worst); s != CPE_OK) return s;
    for (int b = 0; b < B; b++) {
        if (wipe[(size_t)b]) {                              // a node's force matrix has no factor: what the other nodes wrote goes
            const size_t o = (size_t)b * N;
            HIPCHK(hipMemsetAsync(f_s + o * S * KIN_LS, 0, w * N * S * KIN_LS, h->stream));
            if (f) HIPCHK(hipMemsetAsync(f + o * KIN_LS, 0, w * N * KIN_LS, h->stream));
            if (meta) HIPCHK(hipMemsetAsync(meta + o * (KIN_LS + 1), 0, sizeof(int32_t) * N * (KIN_LS + 1), h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));                // (the buffers of this call are freed on return)
    return worst;
}

cpe_status cpe_force_samples(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                             const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, int32_t S,
                             const double* du, const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status) {
    return force_samples_impl("cpe_force_samples", h, opt, B, N, nullptr, nullptr, q, meas, weight, stance, grf_fixed, tau_box, grf_box, ridge, S, du, zeta, f_s,
                              f, meta, status);
}

cpe_status cpe_force_samples_ragged(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames,
                                    const double* q, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                    const double* tau_box, const double* grf_box, double ridge, int32_t S, const double* du, const double* zeta, double* f_s,
                                    double* f, int32_t* meta, cpe_status* status) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "cpe_force_samples_ragged: null model / n_frames");
    return force_samples_impl("cpe_force_samples_ragged", h, opts, B, N_max, model, n_frames, q, meas, weight, stance, grf_fixed, tau_box, grf_box, ridge, S, du,
                              zeta, f_s, f, meta, status);
}

// host-pointer twins (stage through HBM): cpe_force_samples_host (model == null) and cpe_force_samples_ragged_host
static cpe_status force_samples_host_impl(const char* who, cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const int32_t* model,
                                          const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                          const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, int32_t S, const double* du,
                                          const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status) {
    size_t F, FS;
    std::vector<int2> seq;  // (refused here too: before anything is staged)
    if (cpe_status s = force_samples_check(who, h, opt, B, N, model, n_frames, q && meas && weight && status, stance, grf_fixed, tau_box, grf_box, ridge, S, du,
                                           f_s, &F, &FS, seq); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const int nf = opt->dyn.n_feet, nmot = opt->dyn.n_motors;
    const size_t nm = F * cams_max(h) * m.L;
    const double* var = grf_fixed ? grf_fixed : (tau_box ? tau_box : grf_box);
    const size_t nvar = grf_fixed ? F * nf * 3 : (tau_box ? F * nmot * 2 : (grf_box ? F * nf * 6 : 0));
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    const int32_t* dstance = st.in(stance, F * nf);
    const double* dvar = st.in(var, nvar);
    const double *ddu = st.in(du, FS * CPE_NX), *dzeta = st.in(zeta, FS * KIN_LS);
    double *os = st.out(f_s, FS * KIN_LS), *of = st.out_opt(f, F * KIN_LS);
    int32_t* ometa = st.out_opt(meta, F * (KIN_LS + 1));
    HIPCHK(st.err);
    const cpe_status s = force_samples_impl(model ? "cpe_force_samples_ragged" : "cpe_force_samples", h, opt, B, N, model, n_frames, dq, dmeas, dweight, dstance,
                                            grf_fixed ? dvar : nullptr, tau_box ? dvar : nullptr, grf_box ? dvar : nullptr, ridge, S, ddu, dzeta, os, of, ometa,
                                            status);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

cpe_status cpe_force_samples_host(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                  const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                                  double ridge, int32_t S, const double* du, const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status) {
    return force_samples_host_impl("cpe_force_samples_host", h, opt, B, N, nullptr, nullptr, q, meas, weight, stance, grf_fixed, tau_box, grf_box, ridge, S, du,
                                   zeta, f_s, f, meta, status);
}

cpe_status cpe_force_samples_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model,
                                         const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                         const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, int32_t S, const double* du,
                                         const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "cpe_force_samples_ragged_host: null model / n_frames");
    return force_samples_host_impl("cpe_force_samples_ragged_host", h, opts, B, N_max, model, n_frames, q, meas, weight, stance, grf_fixed, tau_box, grf_box,
                                   ridge, S, du, zeta, f_s, f, meta, status);
}

#ifdef CPE_LM_STAMPS
// diagnostic build only: table sizes and LDS bytes of the per-frame kernels for a model (needs no GPU)
cpe_status cpe_debug_footprint(const cpe_skeleton* skel, const cpe_camera* cams, int32_t n_cams, const cpe_options* opts, int64_t* out16) {
    std::vector<DevModel> mv(1);
    cpe_status s = build_model(skel, cams, n_cams, opts, mv[0]);
    if (s != CPE_OK) return s;
    const DevModel& m = mv[0];
    const int64_t v[16] = {m.nq, m.ns, m.nu, m.ndep, m.nrev, m.S, m.ss_n, m.sv_n, m.mc_total, (int64_t)lds_normal(m), (int64_t)sizeof(DevModel), m.L, m.C, m.nl, m.nb, 0};
    for (int i = 0; i < 16; i++) out16[i] = v[i];
    return CPE_OK;
}
// diagnostic build only: the Jacobian of the rows of frame `frame` of the last cpe_eval_kinetic_nodes / solve, column-major [84][KIN_ROWS_MAX] + row gradient + row weight
cpe_status cpe_debug_kinetic_jacobian(cpe_handle* h, int64_t frame, double* out) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->Jbuf + (size_t)frame * KIN_JSTRIDE, sizeof(double) * KIN_JSTRIDE, hipMemcpyDeviceToHost));
    return CPE_OK;
}
cpe_status cpe_debug_fn_stamps(unsigned long long* out16) {
    HIPCHK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_fn_stamps), sizeof(unsigned long long) * 16));
    unsigned long long z[16] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_fn_stamps), z, sizeof(z)));
    return CPE_OK;
}
// diagnostic build only: per-phase shader-clock totals accumulated by block 0 of k_lm_step since the last call
cpe_status cpe_debug_lm_stamps(unsigned long long* out32) {
    HIPCHK(hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_lm_stamps), sizeof(unsigned long long) * 32));
    unsigned long long z[32] = {0};
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_lm_stamps), z, sizeof(z)));
    return CPE_OK;
}
#endif

// ---- host-pointer wrappers: stage through HBM (PCIe-inclusive; never the benchmarked path) -------------

cpe_status cpe_eval_resjac_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                                double* r, double* J, double* eps, double* cost) {
    if (!h || !q || !meas || !r || !J || !eps) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t nm = F * m.C * m.L;
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    double *dr = st.out(r, nm * 2), *dJ = st.out(J, F * m.C * m.S * 2), *deps = st.out(eps, F * m.nq);
    double* dcost = st.out_opt(weight ? cost : nullptr, F);       // the cost needs the weights
    HIPCHK(st.err);
    cpe_status s = cpe_eval_resjac(h, B, N, dq, dmeas, dweight, dr, dJ, deps, dcost);
    if (s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

// host-pointer twins of cpe_solve (model == null) and cpe_solve_ragged: stage through HBM
static cpe_status solve_host_impl(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q_init,
                                  const double* meas, const double* weight, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                  cpe_stats* stats) {
    if (!h || !q_init || !meas || !weight || !q) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    std::vector<int2> seq;
    if (model)
        if (cpe_status s = ragged_table(h, B, N, model, n_frames, seq); s != CPE_OK) return s;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t nm = F * (model ? cams_max(h) : m.C) * m.L;
    Staging st(h->stream);
    const double *di = st.in(q_init, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    double *oq = st.out(q, F * m.nq), *odq = st.out(dq, F * m.nq), *oddq = st.out(ddq, F * m.nq);
    double *op = st.out(positions, F * m.L * 3), *ome = st.out(meas_err, nm * 2);
    HIPCHK(st.err);
    cpe_status s = solve_impl(h, B, N, model, n_frames, di, dmeas, dweight, oq, odq, oddq, op, ome, stats);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

cpe_status cpe_solve_host(cpe_handle* h, int32_t B, int32_t N, const double* q_init, const double* meas, const double* weight,
                          double* q, double* dq, double* ddq, double* positions, double* meas_err, cpe_stats* stats) {
    return solve_host_impl(h, B, N, nullptr, nullptr, q_init, meas, weight, q, dq, ddq, positions, meas_err, stats);
}

cpe_status cpe_solve_ragged_host(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q_init,
                                 const double* meas, const double* weight, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                 cpe_stats* stats) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    return solve_host_impl(h, B, N_max, model, n_frames, q_init, meas, weight, q, dq, ddq, positions, meas_err, stats);
}

// host-pointer twin of cpe_eval_shutter_step: stage through HBM
cpe_status cpe_eval_shutter_step_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, const double* tau,
                                      double lam, double* g, double* Bm, double* cost, double* gx, double* rcb, double* g_total, double* step,
                                      double* meas_err, double* seq) {
    if (!h || !q || !meas || !weight || !tau || !seq) return fail(CPE_BAD_ARG, "null argument");
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    const DevModel& m = h->hm;
    HIPCHK(hipSetDevice(h->device));
    const size_t nm = F * m.C * m.L, BB = (size_t)CPE_NX * CPE_NX;
    Staging st(h->stream);
    const double *dq = st.in(q, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm), *dtau = st.in(tau, (size_t)B * m.C);
    double *og = st.out_opt(g, F * CPE_NX), *oB = st.out_opt(Bm, F * BB), *oc = st.out_opt(cost, F * 3), *ox = st.out_opt(gx, F * 6);
    double *orc = st.out_opt(rcb, F * m.C * 9), *ogt = st.out_opt(g_total, F * CPE_NX), *os = st.out_opt(step, (size_t)B * m.C);
    double* ome = st.out_opt(meas_err, nm * 2);
    HIPCHK(st.err);
    const cpe_status s = cpe_eval_shutter_step(h, B, N, dq, dmeas, dweight, dtau, lam, og, oB, oc, ox, orc, ogt, os, ome, seq);
    if (s != CPE_OK) return s;
    HIPCHK(st.fetch());
    return CPE_OK;
}

// joint equalities of a model: two rows per revolute joint, one per Hooke joint (the node forces lambda, build_kin_entry)
static int n_con(const DevModel& m) {
    int n = 0;
    for (int j = 0; j < m.nj; j++) n += m.joint_kind[j] == CPE_JOINT_REVOLUTE_Y ? 2 : 1;
    return n;
}

// What the physics-based solve twins size their staging by: the counts every model shares (refused here when out of range, and checked again by
// the solve) and the one optional force array (at most one of the three is given: the callers have checked) with its element count over F frames
struct ForceStage { size_t nf, nmo; const double* fx; size_t n_fx; };
static cpe_status force_stage(const cpe_dyn_options& d, size_t F, const double* grf_fixed, const double* tau_box, const double* grf_box, ForceStage& fs) {
    if (d.n_feet < 1 || d.n_feet > 4 || d.n_motors < 0 || d.n_motors > CPE_MAX_MOTORS) return fail(CPE_BAD_ARG, "kinetic options: feet / motors out of range");
    const size_t nf = (size_t)d.n_feet, nmo = (size_t)d.n_motors;
    fs = {nf, nmo, grf_fixed ? grf_fixed : (tau_box ? tau_box : grf_box), grf_fixed ? F * nf * 3 : (tau_box ? F * nmo * 2 : (grf_box ? F * nf * 6 : 0))};
    return CPE_OK;
}

cpe_status cpe_solve_kinetic_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames,
                                         const double* q_init, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                         const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                         double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats) {
    if (!h || !opts || !model || !n_frames || !q_init || !meas || !weight || !stance || !q) return fail(CPE_BAD_ARG, "null argument");
    if (cpe_status s = one_force("cpe_solve_kinetic_ragged", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    size_t F;
    if (cpe_status s = frames(B, N_max, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    ForceStage fs;
    if (cpe_status s = force_stage(opts[0].dyn, F, grf_fixed, tau_box, grf_box, fs); s != CPE_OK) return s;
    const DevModel& m = h->hm;
    const size_t nf = fs.nf, nmo = fs.nmo, nc = (size_t)n_con(m), nm = F * cams_max(h) * m.L;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const double *di = st.in(q_init, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    const int32_t* dstance = st.in(stance, F * nf);
    const double* dfx = st.in(fs.fx, fs.n_fx);
    double *oq = st.out(q, F * m.nq), *odq = st.out(dq, F * m.nq), *oddq = st.out(ddq, F * m.nq);
    double *op = st.out(positions, F * m.L * 3), *ome = st.out(meas_err, nm * 2);
    double *ot = st.out(tau, F * nmo), *ol = st.out(lambda, F * nc), *og = st.out(grf, F * nf * 5), *osl = st.out(slack, F * m.nq);
    HIPCHK(st.err);
    cpe_status s = cpe_solve_kinetic_ragged(h, opts, B, N_max, model, n_frames, di, dmeas, dweight, dstance, grf_fixed ? dfx : nullptr,
                                            tau_box ? dfx : nullptr, grf_box ? dfx : nullptr, oq, odq, oddq, op, ome, ot, ol, og, osl, stats, kstats);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

// host-pointer twins of cpe_solve_kinetic_tracked (model == null) and cpe_solve_kinetic_tracked_ragged: stage through HBM
// track_W non-null: the full-weight form ([B][N][28][28], host; checked here), track_w is then not read
static cpe_status kinetic_tracked_host(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_w, int32_t B, int32_t N, const int32_t* model,
                                       const int32_t* n_frames, const double* q_init, const double* q_target, const double* meas, const double* weight,
                                       const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double* q, double* dq,
                                       double* ddq, double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack,
                                       cpe_stats* stats, cpe_kinetic_stats* kstats, const double* track_W = nullptr, bool full = false) {
    if (!h || !opts || !q_init || !stance || !q) return fail(CPE_BAD_ARG, "null argument");
    if (full ? !track_W : !track_w) return fail(CPE_BAD_ARG, full ? "track_W is null" : "track_w is null");
    if (!q_target) return fail(CPE_BAD_ARG, "q_target is null");
    if (meas && !weight) return fail(CPE_BAD_ARG, "meas is given without weight");
    if (weight && !meas) return fail(CPE_BAD_ARG, "weight is given without meas");
    if (cpe_status s = one_force("cpe_solve_kinetic_tracked", grf_fixed, tau_box, grf_box); s != CPE_OK) return s;
    size_t F;
    if (cpe_status s = frames(B, N, &F); s != CPE_OK) return s;
    if (F == 0) return CPE_OK;
    ForceStage fs;
    if (cpe_status s = force_stage(opts[0].dyn, F, grf_fixed, tau_box, grf_box, fs); s != CPE_OK) return s;
    const DevModel& m = h->hm;
    if (cpe_status s = check_target(q_target, B, N, m.nq, n_frames); s != CPE_OK) return s;
    if (full)
        if (cpe_status s = check_track_W(track_W, B, N, n_frames); s != CPE_OK) return s;
    const size_t nf = fs.nf, nmo = fs.nmo, nc = (size_t)n_con(m), nm = F * (model ? cams_max(h) : m.C) * m.L;
    HIPCHK(hipSetDevice(h->device));
    Staging st(h->stream);
    const double *di = st.in(q_init, F * m.nq), *dt = st.in(q_target, F * m.nq), *dmeas = st.in(meas, nm * 2), *dweight = st.in(weight, nm);
    const double* dW = st.in(full ? track_W : nullptr, F * CPE_NX * CPE_NX);
    const int32_t* dstance = st.in(stance, F * nf);
    const double* dfx = st.in(fs.fx, fs.n_fx);
    double *oq = st.out(q, F * m.nq), *odq = st.out(dq, F * m.nq), *oddq = st.out(ddq, F * m.nq), *op = st.out(positions, F * m.L * 3);
    double* ome = meas ? st.out(meas_err, nm * 2) : nullptr;          // without measurements there are no reprojection errors
    double *ot = st.out(tau, F * nmo), *ol = st.out(lambda, F * nc), *og = st.out(grf, F * nf * 5), *osl = st.out(slack, F * m.nq);
    HIPCHK(st.err);
    // the target is checked here, on the host copy the caller handed in: the device entries' own copy back is skipped
    const TrackIn tr{track_w, model ? n_models(h) : 1, dt, true, full, dW};
    cpe_status s = solve_kinetic_impl(h, opts, B, N, model, n_frames, di, dmeas, dweight, dstance, grf_fixed ? dfx : nullptr, tau_box ? dfx : nullptr,
                                      grf_box ? dfx : nullptr, oq, odq, oddq, op, ome, ot, ol, og, osl, stats, kstats, &tr);
    if (s < 0) return s;
    HIPCHK(st.fetch());
    return s;
}

cpe_status cpe_solve_kinetic_tracked_host(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_w, int32_t B, int32_t N, const double* q_init,
                                          const double* q_target, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                          const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions,
                                          double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                          cpe_kinetic_stats* kstats) {
    return kinetic_tracked_host(h, opt, track_w, B, N, nullptr, nullptr, q_init, q_target, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq,
                                positions, meas_err, tau, lambda, grf, slack, stats, kstats);
}

cpe_status cpe_solve_kinetic_tracked_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_w, int32_t B, int32_t N_max,
                                                 const int32_t* model, const int32_t* n_frames, const double* q_init, const double* q_target,
                                                 const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                                 const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions,
                                                 double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                                 cpe_kinetic_stats* kstats) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    return kinetic_tracked_host(h, opts, track_w, B, N_max, model, n_frames, q_init, q_target, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq,
                                positions, meas_err, tau, lambda, grf, slack, stats, kstats);
}

cpe_status cpe_solve_kinetic_tracked_weighted_host(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_W, int32_t B, int32_t N,
                                                   const double* q_init, const double* q_target, const double* meas, const double* weight,
                                                   const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double* q,
                                                   double* dq, double* ddq, double* positions, double* meas_err, double* tau, double* lambda, double* grf,
                                                   double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats) {
    return kinetic_tracked_host(h, opt, nullptr, B, N, nullptr, nullptr, q_init, q_target, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq,
                                positions, meas_err, tau, lambda, grf, slack, stats, kstats, track_W, true);
}

cpe_status cpe_solve_kinetic_tracked_weighted_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_W, int32_t B, int32_t N_max,
                                                          const int32_t* model, const int32_t* n_frames, const double* q_init, const double* q_target,
                                                          const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                                          const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq,
                                                          double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack,
                                                          cpe_stats* stats, cpe_kinetic_stats* kstats) {
    if (!model || !n_frames) return fail(CPE_BAD_ARG, "null argument");
    return kinetic_tracked_host(h, opts, nullptr, B, N_max, model, n_frames, q_init, q_target, meas, weight, stance, grf_fixed, tau_box, grf_box, q, dq, ddq,
                                positions, meas_err, tau, lambda, grf, slack, stats, kstats, track_W, true);
}

}  // extern "C"
