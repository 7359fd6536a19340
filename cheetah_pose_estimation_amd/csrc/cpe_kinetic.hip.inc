// cpe_kinetic.hip.inc -- physics-based trajectory model (config 4 / SURVEY row a12), included by cpe_kernels.hip.
//
// Statement: include/cpe.h above cpe_solve_kinetic and DESIGN.md 2b; reference: estimate_kinetics (acinoset_opt.py:693-963),
// prescribe_contact_order (acinoset_misc.py:1140-1167), motion_smoothing_cost (:601-613), eom_slack_cost (:631-636).
//
// Per LM iteration, after k_frame_normal has made the Euler angles of every frame consistent:
//   k_dyn_eval      one workgroup per node n: residual vector rho(u_n, u_n-1, u_n-2; f) = [slack_eom | foot heights | foot velocities (x, y, z) |
//                   fps^2 second differences of the markers]; the node forces f = (tau, lambda, net foot forces) minimised out exactly
//                   (constraint forces and torques by one Cholesky, the foot forces by a semismooth Newton on <= 12 unknowns; the active sets of the
//                   torque boxes and of the box on the residual iterated around that elimination); cost; row gradients and weights
//   k_dyn_jac       (cpe_kinetic_jac.hip.inc) Jacobian of rho with respect to the 84 reduced coordinates of the three frames, in closed form
//   k_dyn_assemble  H_uu = J^T W J, H_fu = -A^T W J_e, gradient: the second-order pieces of the node (kept per buffer)
//   (k_lm_step<.., 1>: accept / reject, new damping)
//   k_dyn_schur     per node of the CURRENT iterate: H_uu - H_uf (H_ff + lambda diag H_ff)^-1 H_fu  (trust region in force space)
//   k_dyn_gather    per frame: band blocks and gradient of the whole objective, read by k_lm_step<.., 2>
// All sums have a fixed order: solves are reproducible bit for bit.

// diagnostic build only (-DCPE_LM_STAMPS): shader-clock totals of the phases of k_dyn_eval for node 5 of sequence 0, slots 9..15 of g_fn_stamps
#ifdef CPE_LM_STAMPS
#define KSTAMP(i) do { if (blockIdx.x == 5 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_fn_stamps[9 + (i)] += t_ - tk_last; tk_last = t_; } } while (0)
#else
#define KSTAMP(i) do { } while (0)
#endif
#define KIN_MU 19                 // multipliers per foot: 0-1 Fz lower / upper, 2-5 +-Fx, +-Fy <= fmax, 6-9 friction polyhedron, 10-11 |height|, 12-15 +-vx, +-vy, 16 flight height, 17-18 +-vz
#define KIN_LS 64                 // stride of a node-force vector (tau | lambda | (z, x, y) per foot), nlat <= 64
#define KIN_NC3 (3 * CPE_NX)      // reduced coordinates of the three frames of a node
#define KIN_ROWS_MAX (CPE_MAX_NQ + 16 + 3 * CPE_MAX_MARKERS)
#define KIN_THREADS 256
#define KIN_SLOT 1152             // doubles of LDS scratch per evaluation slot (two slots per wave)
#define KIN_NA_MAX 60              // node forces that can be unknowns at once (tau, lambda, three per stance foot)
#define KIN_MS (KIN_NA_MAX + 1)    // stride of the node's normal matrix in LDS (odd: its columns are read without bank conflicts)
#define KE_R1 (KIN_MS * KIN_MS + 576)   // LDS regions of k_dyn_eval in doubles (see there)
#define KE_R2 (KIN_NA_MAX * KIN_LS)
#define KIN_PIECE (KIN_NC3 * KIN_NC3 + KIN_LS * KIN_NC3 + KIN_LS * KIN_LS)      // doubles per node: H_uu | H_fu | H_ff
#define KIN_JSTRIDE (KIN_ROWS_MAX * KIN_NC3 + 2 * KIN_ROWS_MAX)                  // J | row gradient | row weight
#define KIN_POLE 0.1               // |cos theta| below which a link counts as next to the pole of its Euler chart (5.7 degrees)
#define KJ_LMAX 12                // motors / equality rows per link pair (8 / 6 on the cheetah)
#define KIN_STAT 8                // per-node record: eom, torque, reg, energy, al, max slack, max base row, max violation

struct DevKin {
    cpe_kinetic_options o;
    int32_t nm, nc, nf, nlat, nrow;
    double Mg, h, ih;
    uint32_t sub_mask[CPE_MAX_LINKS];                 // bit j set: link j lies in the subtree of link i (i itself included)
    int32_t con_joint[2 * CPE_MAX_JOINTS], con_axis[2 * CPE_MAX_JOINTS];      // constraint row -> joint, child axis (0 = x, 2 = z)
    const double* grf_fix;                            // prescribed net foot forces [F][nf][3] (z, x, y; body weights), or null: the forces of the stance feet are unknowns
    const double* grf_box;                            // boxes on the net foot forces [F][nf][3][2] = (lower, upper) of (z, x, y), or null (cpe_solve_kinetic_force_box)
    const double* tau_box;                            // torque boxes [F][nm][2] = (lower, upper), or null (cpe_solve_kinetic_bounded: the reference's module-level estimate_grf,
    double* mu_tau;                                   //   acinoset_opt.py:995-1003); their multipliers [F][nm][2] (lower side, upper side)
    double* mu_slack;                                 // multipliers of the box on the residual [F][CPE_MAX_NQ][2] (upper side, lower side): bound_eom_error
    int32_t sbox;                                     // the box [slack_lo, slack_hi] is on
    // ---- tables of k_dyn_jac (cpe_kinetic_jac.hip.inc), built on the host from the skeleton
    int8_t rel[CPE_MAX_LINKS][CPE_MAX_LINKS];         // (i, k): 0 unrelated, 1 k is a strict ancestor of i, 2 k is a strict descendant of i, 3 k == i
    int8_t toward[CPE_MAX_LINKS][CPE_MAX_LINKS];      // rel 1: the child of k on the path to i; rel 2: the child of i on the path to k
    int16_t blk[CPE_MAX_LINKS][CPE_MAX_LINKS];        // index of the related pair (i, k) in the block matrices, or -1
    int32_t nblk; int8_t blk_i[96], blk_k[96];
    uint32_t blk_word[96];                            // i | k << 8 | rel << 16 | (toward & 255) << 24 of the pair: one read instead of four, two of them behind the others
    uint8_t bm_n[96], bc_n[96], bm[96][KJ_LMAX], bc[96][KJ_LMAX];     // motors / joint-equality rows whose generalised force has a second derivative in the pair
    double s1[CPE_MAX_LINKS][3], S2[CPE_MAX_LINKS][9];        // first / second moments of the subtree of link i about its origin, in its frame
    double mtot;
    int8_t leg_of_link[CPE_MAX_LINKS];                // index of the revolute (leg) coordinate of a link, or -1
    int8_t hooke_of_link[CPE_MAX_LINKS];              // index among the Hooke children (parents first), or -1
    int32_t nh; int8_t hk_parent[4], hk_child[4];
};

// slot layout (offsets in doubles), sized for the reference's skeleton and checked against it by build_kin (cpe_api.hip): KS_NQ coordinates,
// KS_NL links, KS_L markers, KS_NS state words (Euler angles | leg angles), KS_NROW rows of the node's residual vector
#define KS_NQ 54
#define KS_NL 17
#define KS_L 24
#define KS_NS 71
#define KS_NROW 144
#define KS_E0 0
#define KS_E1 (KS_E0 + KS_NQ)
#define KS_E2 (KS_E1 + KS_NQ)
#define KS_DQ (KS_E2 + KS_NQ)
#define KS_DDQ (KS_DQ + KS_NQ)
#define KS_SC (KS_DDQ + KS_NQ)
#define KS_R (KS_SC + 6 * KS_NL)
#define KS_W (KS_R + 9 * KS_NL)
#define KS_AL (KS_W + 3 * KS_NL)
#define KS_FI (KS_AL + 3 * KS_NL)
#define KS_FS (KS_FI + 3 * KS_NL)
#define KS_ROWS (KS_FS + 3 * KS_NL)
#define KS_Q (KS_ROWS + KS_NQ)
#define KS_POS (KS_Q + KS_NQ)
#define KS_ST (KS_POS + 3 * KS_L)
#define KS_RHO (KS_ST + KS_NS)
static_assert(KS_SC == 270 && KS_R == 372 && KS_POS == 837 && KS_ST == 909 && KS_RHO == 980, "slot layout of the kinetic kernels");
static_assert(KS_RHO + KS_NROW <= KIN_SLOT, "an evaluation slot holds the whole residual vector");
static_assert(KS_NQ <= CPE_MAX_NQ && KS_NL <= CPE_MAX_LINKS && KS_L <= CPE_MAX_MARKERS, "slot layout inside the ABI limits");

struct KinShared {
    double st[3][KS_NS + 1];                       // states of frames n, n-1, n-2 (consistent Euler angles | leg angles)
    double f[KIN_LS];                              // node forces in use
    double fw[KIN_LS];                             // warm start (forces of the current iterate)
    double mu[4 * KIN_MU];
    double posb[3][3 * KS_L];                      // marker positions of the three frames at the base point
    double scb[6 * KS_NL], Rb[9 * KS_NL];      // sin / cos and rotations of frame n at the base point
    double r0[KS_NROW], rhob[KS_NROW], grow[KS_NROW], wrow[KS_NROW];
    double bv[KIN_LS];                             // A_a^T diag(omega) (r0 - c) of the round
    double red[16];
    int stance[4];
    int idx[KIN_LS], na;
    double tb[2 * CPE_MAX_MOTORS], mt[2 * CPE_MAX_MOTORS];      // torque boxes and their multipliers (entry 2 m + side)
    int tact[2 * CPE_MAX_MOTORS];                               // active set of the torque rows during the node solve
    double ms[2 * KS_NQ];                                  // multipliers of the slack box (2 p: upper side, 2 p + 1: lower side)
    double wsl[KS_NQ], csl[KS_NQ];                    // row weights omega_p = W_p / w and shifts c_p of the residual rows for the box's active set
    int sact[2 * KS_NQ];                                   // active set of the box during the node solve
};

__device__ __forceinline__ void kin_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void kin_matvec(const double* R, const double* v, double* o) {
    o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2]; o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2]; o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}
__device__ __forceinline__ double kin_al(double g, double m, double kp, double* p_out) {
    double t = m + kp * g; if (t < 0.0) t = 0.0; if (p_out) *p_out = t; return (t * t - m * m) / (2.0 * kp);
}
// linear inequality j (0..9) on the net force (Fz, Fx, Fy) of a stance foot: c . F - d <= 0
// bx: box of this foot's net force (z lo, z hi, x lo, x hi, y lo, y hi) replacing the constants of rows 0-5, or null (cpe_solve_kinetic_force_box)
__device__ __forceinline__ void kin_force_con(const cpe_kinetic_options& ko, int j, double* c3, double* d, const double* bx = nullptr) {
    c3[0] = c3[1] = c3[2] = 0.0;
    if (j == 0) { c3[0] = -1.0; *d = -ko.grfz_min; }
    else if (j == 1) { c3[0] = 1.0; *d = ko.force_max; }
    else if (j == 2) { c3[1] = 1.0; *d = ko.force_max; }
    else if (j == 3) { c3[1] = -1.0; *d = ko.force_max; }
    else if (j == 4) { c3[2] = 1.0; *d = ko.force_max; }
    else if (j == 5) { c3[2] = -1.0; *d = ko.force_max; }
    else { c3[0] = -ko.friction; c3[1] = (j - 6) < 2 ? 1.0 : -1.0; c3[2] = ((j - 6) & 1) ? -1.0 : 1.0; *d = 0.0; }
    if (bx && j < 6) *d = j == 0 ? -bx[0] : (j == 1 ? bx[1] : (j == 2 ? bx[3] : (j == 3 ? -bx[2] : (j == 4 ? bx[5] : -bx[4]))));      // -z <= -lo, z <= hi, x <= hi, -x <= -lo, y <= hi, -y <= -lo
}

// nearest equivalent ZYX triple of link i of q to that of ref (both LDS), written to out
__device__ __forceinline__ void kin_nearest_link(const double* ref, const double* q, double* out, int i) {
    const double TWO_PI = 6.283185307179586476925286766559, PI = 3.14159265358979323846264338327950288;
    const double* a = q + 3 + 3 * i; const double* r = ref + 3 + 3 * i;
    const double alt[3] = {a[0] + PI, PI - a[1], a[2] + PI};
    double c1[3], c2[3], d1 = 0.0, d2 = 0.0;
    for (int k = 0; k < 3; k++) {
        c1[k] = a[k] + TWO_PI * rint((r[k] - a[k]) / TWO_PI);
        c2[k] = alt[k] + TWO_PI * rint((r[k] - alt[k]) / TWO_PI);
        d1 += (c1[k] - r[k]) * (c1[k] - r[k]); d2 += (c2[k] - r[k]) * (c2[k] - r[k]);
    }
    double o[3];
    for (int k = 0; k < 3; k++) o[k] = d2 < d1 ? c2[k] : c1[k];
    // At the pole of the ZYX chart (cos theta = 0) the rotation depends on phi - sin(theta) psi only: the read-back (phi, psi) of a link next to the
    // pole is an arbitrary point of the line (phi + t, psi + sin(theta) t), and its difference to the neighbouring frame's angles fakes roll and yaw
    // rates of ~pi / 2 per frame that cancel in the rotation (cliffs of +24 ... +40 in the objective, measured).  Next to the pole the representative
    // is moved ALONG that line to the point nearest the reference: exact at the pole, blended out (C1) between |cos theta| = KIN_POLE / 2 and KIN_POLE.
    const double ct = fabs(cos(o[1]));
    if (ct < KIN_POLE) {
        const double sg = sin(o[1]) > 0.0 ? 1.0 : -1.0;
        const double t = 0.5 * ((r[0] - o[0]) + sg * (r[2] - o[2]));
        const double u = ct <= 0.5 * KIN_POLE ? 0.0 : (ct - 0.5 * KIN_POLE) / (0.5 * KIN_POLE), w = 1.0 - u * u * (3.0 - 2.0 * u);
        o[0] += w * t; o[2] += w * sg * t;
    }
    for (int k = 0; k < 3; k++) out[3 + 3 * i + k] = o[k];
}

// coefficient of the generalised force of coordinate p: Q_p = Mg * ( sum_m tau_m cm + sum_r lam_r cr + sum_k F_k . ck )  (body weights)
// sc, R: sin / cos and rotation of every link of frame n (LDS); D = d R_i / d a of p's own link i, angle a (registers; p >= 3)
__device__ __forceinline__ double kin_coef_motor(const DevKin* K, const double* sc, const double* R, int i, int a, int m) {
    const int a1 = K->o.dyn.motor_first[m], a2 = K->o.dyn.motor_second[m];
    if (a1 != i && a2 != i) return 0.0;
    const double sf = sc[6 * i], cf = sc[6 * i + 1], st = sc[6 * i + 2], ct = sc[6 * i + 3];
    const double c3[3][3] = {{1.0, 0.0, 0.0}, {0.0, cf, -sf}, {-st, sf * ct, cf * ct}};
    double wc[3]; kin_matvec(R + 9 * i, c3[a], wc);                     // d w_world / d q'_a of link i
    const int ax = K->o.dyn.motor_axis[m];
    const double* R1 = R + 9 * a1;
    const double t = R1[ax] * wc[0] + R1[3 + ax] * wc[1] + R1[6 + ax] * wc[2];
    return (a2 == i ? t : 0.0) - (a1 == i ? t : 0.0);
}
__device__ __forceinline__ double kin_coef_con(const DevModel* M, const DevKin* K, const double* R, const double* D, int i, int r) {
    const int j = K->con_joint[r], cc = K->con_axis[r];
    const int p = M->joint_parent[j], ch = M->joint_child[j];
    double d = 0.0;
    if (p == i) { const double* Rc = R + 9 * ch; d += D[1] * Rc[cc] + D[4] * Rc[3 + cc] + D[7] * Rc[6 + cc]; }
    if (ch == i) { const double* Rp = R + 9 * p; d += Rp[1] * D[cc] + Rp[4] * D[3 + cc] + Rp[7] * D[6 + cc]; }
    return d;
}
// derivative of the foot point of foot k with respect to coordinate p (3-vector; zero if p's link is not on the chain)
__device__ __forceinline__ void kin_coef_foot(const DevModel* M, const DevKin* K, const double* D, int p, int i, int k, double* out) {
    out[0] = out[1] = out[2] = 0.0;
    if (p < 3) { out[p] = 1.0; return; }
    const int l = K->o.dyn.foot_marker[k];
    for (int c = 0; c < M->chain_len[l]; c++)
        if (M->chain_link[l][c] == i) { kin_matvec(D, M->chain_vec[l][c], out); return; }
}

// One evaluation of the node's residual vector in a slot (32 lanes, l = lane in the slot) at the states of the three frames held in Sh->st.
//   The rows are evaluated at node forces f = 0: the residual is r0 - A f with A = d(generalised forces) / d f built by k_dyn_eval itself.
//   (Round 2 also moved one coordinate at a time through here: 168 central differences per node; the derivatives are k_dyn_jac's now.)
// Result: S[KS_RHO ...].  Also leaves sin / cos, R of frame n in S[KS_SC], S[KS_R].
__device__ __forceinline__ void kin_eval(const DevModel* __restrict__ M, const DevKin* __restrict__ K, KinShared* Sh, double* S, int l) {
    const int nq = M->nq, nl = M->nl, L = M->L, nf = K->nf;
    double* E0 = S + KS_E0; double* E1 = S + KS_E1; double* E2 = S + KS_E2;
    // ---- Euler angles of the three frames
    for (int t = l; t < nq; t += 32) {
        E0[t] = Sh->st[0][t];
        S[KS_Q + t] = Sh->st[1][t];                                  // raw neighbours (unwrapped below), parked in the Q / ROWS areas
        S[KS_ROWS + t] = Sh->st[2][t];
    }
    wave_lds_sync();
    if (l < 3) { E1[l] = S[KS_Q + l]; E2[l] = S[KS_ROWS + l]; }
    if (l < nl) kin_nearest_link(E0, S + KS_Q, E1, l);
    wave_lds_sync();
    if (l < nl) kin_nearest_link(E1, S + KS_ROWS, E2, l);
    wave_lds_sync();
    const double ih = K->ih;
    for (int t = l; t < nq; t += 32) { S[KS_DQ + t] = (E0[t] - E1[t]) * ih; S[KS_DDQ + t] = (E0[t] - 2.0 * E1[t] + E2[t]) * ih * ih; }
    // (sin / cos and the rotations of frame n are in this slot already: kin_positions of the same half-wave left them in S[KS_SC], S[KS_R]; so are the
    // marker positions, in Sh->posb[0])
    wave_lds_sync();
    // ---- rows of d/dt dL/dq' - dL/dq (k_eom's arithmetic, one lane per link)
    double Jw[3][3] = {{0}};
    if (l < nl) {
        const double* da = S + KS_DQ + 3 + 3 * l; const double* dda = S + KS_DDQ + 3 + 3 * l;
        const double sf = S[KS_SC + 6 * l], cf = S[KS_SC + 6 * l + 1], st = S[KS_SC + 6 * l + 2], ct = S[KS_SC + 6 * l + 3];
        const double c0[3] = {1.0, 0.0, 0.0}, c1[3] = {0.0, cf, -sf}, c2[3] = {-st, sf * ct, cf * ct};
        const double d1[3] = {0.0, -sf * da[0], -cf * da[0]};
        const double d2[3] = {-ct * da[1], cf * da[0] * ct - sf * st * da[1], -sf * da[0] * ct - cf * st * da[1]};
        for (int t = 0; t < 3; t++) {
            S[KS_W + 3 * l + t] = c0[t] * da[0] + c1[t] * da[1] + c2[t] * da[2];
            S[KS_AL + 3 * l + t] = c0[t] * dda[0] + c1[t] * dda[1] + c2[t] * dda[2] + d1[t] * da[1] + d2[t] * da[2];
            Jw[t][0] = c0[t]; Jw[t][1] = c1[t]; Jw[t][2] = c2[t];
        }
    }
    wave_lds_sync();
    double fi[3] = {0, 0, 0};
    if (l < nl) {
        double acc[3] = {S[KS_DDQ], S[KS_DDQ + 1], S[KS_DDQ + 2]};
        double terms[CPE_MAX_CHAIN][3];
        int nt = 0, j = l;
        while (M->parent[j] >= 0) {
            const int p = M->parent[j];
            grf_point_acc(S + KS_R + 9 * p, S + KS_W + 3 * p, S + KS_AL + 3 * p, M->attach[j], terms[nt]);
            nt++; j = p;
        }
        for (int t = nt - 1; t >= 0; t--) { acc[0] += terms[t][0]; acc[1] += terms[t][1]; acc[2] += terms[t][2]; }
        double ac[3];
        grf_point_acc(S + KS_R + 9 * l, S + KS_W + 3 * l, S + KS_AL + 3 * l, M->com[l], ac);
        const double m = M->mass[l];
        fi[0] = m * (acc[0] + ac[0]); fi[1] = m * (acc[1] + ac[1]); fi[2] = m * (acc[2] + ac[2] + K->o.dyn.eom.gravity);
        S[KS_FI + 3 * l] = fi[0]; S[KS_FI + 3 * l + 1] = fi[1]; S[KS_FI + 3 * l + 2] = fi[2];
    }
    wave_lds_sync();
    if (l < nl) {                 // subtree sums in link order (fixed order: reproducible)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        const uint32_t mask = K->sub_mask[l];
        for (int j = 0; j < nl; j++) if ((mask >> j) & 1u) { s0 += S[KS_FI + 3 * j]; s1 += S[KS_FI + 3 * j + 1]; s2 += S[KS_FI + 3 * j + 2]; }
        S[KS_FS + 3 * l] = s0; S[KS_FS + 3 * l + 1] = s1; S[KS_FS + 3 * l + 2] = s2;
    }
    wave_lds_sync();
    if (l < nl) {
        if (M->parent[l] < 0) { S[KS_ROWS] = S[KS_FS + 3 * l]; S[KS_ROWS + 1] = S[KS_FS + 3 * l + 1]; S[KS_ROWS + 2] = S[KS_FS + 3 * l + 2]; }
        const double* I = K->o.dyn.eom.link_inertia[l]; const double* w = S + KS_W + 3 * l; const double* al = S + KS_AL + 3 * l;
        const double Iw[3] = {I[0] * w[0], I[1] * w[1], I[2] * w[2]};
        double wIw[3]; kin_cross(w, Iw, wIw);
        const double tq[3] = {I[0] * al[0] + wIw[0], I[1] * al[1] + wIw[1], I[2] * al[2] + wIw[2]};
        for (int a2 = 0; a2 < 3; a2++) {
            double D[9], v[3];
            rot_kind(S + KS_SC + 6 * l, 1 + a2, D);
            kin_matvec(D, M->com[l], v);
            double e = fi[0] * v[0] + fi[1] * v[1] + fi[2] * v[2];
            for (int c = 0; c < nl; c++)
                if (M->parent[c] == l) { kin_matvec(D, M->attach[c], v); e += S[KS_FS + 3 * c] * v[0] + S[KS_FS + 3 * c + 1] * v[1] + S[KS_FS + 3 * c + 2] * v[2]; }
            e += tq[0] * Jw[0][a2] + tq[1] * Jw[1][a2] + tq[2] * Jw[2][a2];
            S[KS_ROWS + 3 + 3 * l + a2] = e;
        }
    }
    wave_lds_sync();
    // ---- foot velocity x, y, z: (d foot / d q) dq, lanes 0 .. nf-1
    double vfoot[3] = {0.0, 0.0, 0.0};
    if (l < nf) {
        const int mk = K->o.dyn.foot_marker[l];
        double v0 = S[KS_DQ], v1 = S[KS_DQ + 1], v2 = S[KS_DQ + 2];
        for (int c = 0; c < M->chain_len[mk]; c++) {
            const int lk = M->chain_link[mk][c];
            for (int a = 0; a < 3; a++) {
                double D[9], t[3];
                rot_kind(S + KS_SC + 6 * lk, 1 + a, D);
                kin_matvec(D, M->chain_vec[mk][c], t);
                const double w = S[KS_DQ + 3 + 3 * lk + a];
                v0 += t[0] * w; v1 += t[1] * w; v2 += t[2] * w;
            }
        }
        vfoot[0] = v0; vfoot[1] = v1; vfoot[2] = v2;
    }
    wave_lds_sync();
    // ---- the residual vector
    double* rho = S + KS_RHO;
    const double iMg = 1.0 / K->Mg;
    for (int p = l; p < nq; p += 32) rho[p] = S[KS_ROWS + p] * iMg;
    if (l < nf) {
        const int mk = K->o.dyn.foot_marker[l];
        const double z = Sh->posb[0][3 * mk + 2];
        rho[nq + l] = z - K->o.ground_height;
        rho[nq + nf + 3 * l] = vfoot[0]; rho[nq + nf + 3 * l + 1] = vfoot[1]; rho[nq + nf + 3 * l + 2] = vfoot[2];
    }
    const double c2 = ih * ih;
    for (int t = l; t < 3 * L; t += 32) {
        const double a0 = Sh->posb[0][t], a1 = Sh->posb[1][t], a2 = Sh->posb[2][t];
        rho[nq + 4 * nf + t] = c2 * (a0 - 2.0 * a1 + a2);
    }
    wave_lds_sync();
}

// positions of a frame from its Euler angles into out[3 L] (slot scratch used for sin / cos and R); 32 lanes
__device__ __forceinline__ void kin_positions(const DevModel* __restrict__ M, const double* E, double* S, double* out, int l) {
    const int nl = M->nl, L = M->L;
    for (int t = l; t < 3 * nl; t += 32) { double s_, c_; sincos(E[3 + t], &s_, &c_); S[KS_SC + 2 * t] = s_; S[KS_SC + 2 * t + 1] = c_; }
    wave_lds_sync();
    if (l < nl) rot_kind(S + KS_SC + 6 * l, 0, S + KS_R + 9 * l);
    wave_lds_sync();
    if (l < L) {
        double p0 = E[0], p1 = E[1], p2 = E[2];
        for (int c = 0; c < M->chain_len[l]; c++) {
            double t[3]; kin_matvec(S + KS_R + 9 * M->chain_link[l][c], M->chain_vec[l][c], t);
            p0 += t[0]; p1 += t[1]; p2 += t[2];
        }
        out[3 * l] = p0; out[3 * l + 1] = p1; out[3 * l + 2] = p2;
    }
    wave_lds_sync();
}

// The first npiv steps of a right-looking Cholesky of the n x n matrix H (lower triangle, leading dimension ld) by the whole workgroup, four pivots
// per step (two barriers per four pivots).  On return columns < npiv hold the factor (rows >= npiv: L_21 = H_21 L_11^-T), dg[j] = 1 / L_jj, and the
// trailing block the Schur complement H_22 - L_21 L_21^T -- columns < ncol only (ncol = npiv: just the factor and L_21).
// The TRAILING MATRIX LIVES IN REGISTERS: thread (ta, tc) of the 16 x 16 grid owns the entries (a, c) with a = ta mod 16, c = tc mod 16 (c <= a, c < ncol: up to
// 9 x 4 of them) for the whole factorisation.  Per panel
//   (0) the owners of the panel's four columns publish them to LDS;
//   (1) every thread factors the 4 x 4 pivot block in its registers (the same ten numbers from LDS, broadcast);
//   (2) one thread per row below the block: its four entries of the panel by forward substitution, back to LDS;
//   (3) rank-4 update of the owned entries from the panel values of their rows and columns (13 LDS reads of 16 B a panel where the update of the matrix in
//       LDS took ~216 of 8 B: stamps had that update at 70 % of the routine, the LDS pipe of the CU shared by eight waves).
// The arithmetic per entry is what it was (same expression, same order of the panels): results are bit-identical to the LDS-resident version.
#define KPC_CJ 4            // columns a thread owns: ncol <= 16 * KPC_CJ
static_assert(KIN_NA_MAX + KIN_NC3 <= 16 * 9 && KIN_NA_MAX + 1 <= 16 * KPC_CJ, "kin_partial_cholesky: ownership grid");
template <int KPC_RI /* rows a thread owns: n <= 16 * KPC_RI (k_dyn_schur: 9) */>
__device__ __forceinline__ bool kin_partial_cholesky(double* H, int n, int npiv, int ncol, int ld, double* dg, int tid, int* flag) {
    const int ta = tid >> 4, tc = tid & 15;
    double e[KPC_RI][KPC_CJ];
    const double* rowp[KPC_RI]; const double* colp[KPC_CJ]; bool colok[KPC_CJ];          // rows / columns of this thread in LDS (clamped into the matrix)
#pragma unroll
    for (int i = 0; i < KPC_RI; i++) { const int a = ta + 16 * i; rowp[i] = H + (a < n ? a : n - 1) * ld; }
#pragma unroll
    for (int j = 0; j < KPC_CJ; j++) { const int c = tc + 16 * j; colok[j] = c < ncol && c < n; colp[j] = H + (c < n ? c : n - 1) * ld; }
#pragma unroll
    for (int i = 0; i < KPC_RI; i++)
#pragma unroll
        for (int j = 0; j < KPC_CJ; j++) {
            const int a = ta + 16 * i, c = tc + 16 * j;
            const bool own = a < n && c < ncol && c <= a;
            e[i][j] = H[own ? a * ld + c : 0];
        }
    for (int j0 = 0; j0 < npiv; j0 += 4) {
        const int w = npiv - j0 < 4 ? npiv - j0 : 4;
        // (0) publish the panel's columns (their current values: every earlier panel has been applied)
        // (the four columns j0 .. j0 + 3 belong to the threads tc = j0 mod 16 .. + 3, all in their column slot j0 / 16: one uniform choice of the slot, then
        // nine predicated stores -- tested per slot and row this step was a third of the routine)
        {
            const int jp = j0 >> 4, cpub = tc + 16 * jp;
            const bool pub = cpub >= j0 && cpub < j0 + w;
#pragma unroll
            for (int j = 0; j < KPC_CJ; j++)
                if (j == jp) {
#pragma unroll
                    for (int i = 0; i < KPC_RI; i++) { const int a = ta + 16 * i; if (pub && a < n && cpub <= a) H[a * ld + cpub] = e[i][j]; }
                }
        }
        __syncthreads();
        double P[4][4], ip[4];
        bool bad = false;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = 0; q <= p; q++) P[p][q] = (p < w) ? H[(j0 + p) * ld + j0 + q] : (p == q ? 1.0 : 0.0);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            double d = P[p][p];
#pragma unroll
            for (int q = 0; q < p; q++) d -= P[p][q] * P[p][q];
            if (!(d > 0.0)) bad = true;
            // 1 / sqrt(d) from the hardware estimate and two Newton steps (full precision; a third of the dependent chain of sqrt + divide)
            double is = __builtin_amdgcn_rsq(d);
            is = is * (1.5 - 0.5 * d * is * is); is = is * (1.5 - 0.5 * d * is * is);
            const double sd = d * is;
            P[p][p] = sd; ip[p] = is;
#pragma unroll
            for (int r = p + 1; r < 4; r++) { double v = P[r][p]; 
#pragma unroll
                for (int q = 0; q < p; q++) v -= P[r][q] * P[p][q];
                P[r][p] = v * is; }
        }
        if (bad) { if (tid == 0) *flag = 1; __syncthreads(); return false; }      // uniform: every thread factors the same block
        for (int a = j0 + w + tid; a < n; a += KIN_THREADS) {
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = q < w ? H[a * ld + j0 + q] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
#pragma unroll
                for (int r = 0; r < q; r++) v[q] -= v[r] * P[q][r];
                v[q] *= ip[q];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) if (q < w) H[a * ld + j0 + q] = v[q];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int p = 0; p < 4; p++) if (p < w) { dg[j0 + p] = ip[p];
#pragma unroll
                for (int q = 0; q <= p; q++) H[(j0 + p) * ld + j0 + q] = P[p][q]; }
        }
        // (3) the owned entries right of the panel: e(a, c) -= sum_q L(a, j0 + q) L(c, j0 + q).  Branch-free: the panel values of a column that is finished
        // (c < j0 + w) or outside the matrix are taken as zero, so its entries -- and those of rows above the panel, whose columns are all finished -- are left
        // as they are; entries a thread does not own hold numbers that are never stored.  (The update is issue-bound: two workgroups a CU, two waves a SIMD.)
        const int r0 = j0 + w;
        double hq[KPC_CJ][4];
#pragma unroll
        for (int j = 0; j < KPC_CJ; j++) {
            const bool live = colok[j] && tc + 16 * j >= r0;
#pragma unroll
            for (int q = 0; q < 4; q++) { const double v = colp[j][j0 + q]; hq[j][q] = live && q < w ? v : 0.0; }
        }
#pragma unroll
        for (int i = 0; i < KPC_RI; i++) {
            double lq[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { const double v = rowp[i][j0 + q]; lq[q] = q < w ? v : 0.0; }
#pragma unroll
            for (int j = 0; j < KPC_CJ; j++) {
                double u = lq[0] * hq[j][0];                 // (past the panel's width both factors are exact zeros: those terms add +0)
                u += lq[1] * hq[j][1];
                u += lq[2] * hq[j][2];
                u += lq[3] * hq[j][3];
                e[i][j] -= u;
            }
        }
    }
    // the trailing block (columns npiv .. ncol - 1) back to LDS
#pragma unroll
    for (int j = 0; j < KPC_CJ; j++) {
        const int c = tc + 16 * j;
        if (c >= npiv && c < ncol) {
#pragma unroll
            for (int i = 0; i < KPC_RI; i++) { const int a = ta + 16 * i; if (a < n && c <= a) H[a * ld + c] = e[i][j]; }
        }
    }
    __syncthreads();
    if (tid == 0) *flag = 0;
    return true;
}
// (k_dyn_eval's matrix is 61 x 61 at most: there the version that keeps the matrix in LDS is the faster one -- 1.91 against 1.98 ms per 12 800 nodes)
// The first npiv steps of a right-looking Cholesky of the n x n matrix H (lower triangle, leading dimension ld) by the whole workgroup, four pivots
// per step (two barriers per four pivots).  On return columns < npiv hold the factor (rows >= npiv: L_21 = H_21 L_11^-T), dg[j] = 1 / L_jj, and the
// trailing block the Schur complement H_22 - L_21 L_21^T -- columns < ncol only (ncol = npiv: just the factor and L_21).
//   (1) every thread factors the 4 x 4 pivot block in its registers (the same ten numbers from LDS, broadcast);
//   (2) one thread per row below the block: its four entries of the panel by forward substitution;
//   (3) rank-4 update of the trailing block, threads 16 x 16 over (row, column); thread 0 stores the pivot block's factor meanwhile.
__device__ __forceinline__ bool kin_partial_cholesky_lds(double* H, int n, int npiv, int ncol, int ld, double* dg, int tid, int* flag) {
    const int ta = tid >> 4, tc = tid & 15;
    for (int j0 = 0; j0 < npiv; j0 += 4) {
        const int w = npiv - j0 < 4 ? npiv - j0 : 4;
        double P[4][4], ip[4];
        bool bad = false;
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int q = 0; q <= p; q++) P[p][q] = (p < w) ? H[(j0 + p) * ld + j0 + q] : (p == q ? 1.0 : 0.0);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            double d = P[p][p];
#pragma unroll
            for (int q = 0; q < p; q++) d -= P[p][q] * P[p][q];
            if (!(d > 0.0)) bad = true;
            // 1 / sqrt(d) from the hardware estimate and two Newton steps (full precision; a third of the dependent chain of sqrt + divide)
            double is = __builtin_amdgcn_rsq(d);
            is = is * (1.5 - 0.5 * d * is * is); is = is * (1.5 - 0.5 * d * is * is);
            const double sd = d * is;
            P[p][p] = sd; ip[p] = is;
#pragma unroll
            for (int r = p + 1; r < 4; r++) { double v = P[r][p]; 
#pragma unroll
                for (int q = 0; q < p; q++) v -= P[r][q] * P[p][q];
                P[r][p] = v * is; }
        }
        if (bad) { if (tid == 0) *flag = 1; __syncthreads(); return false; }      // uniform: every thread factors the same block
        for (int a = j0 + w + tid; a < n; a += KIN_THREADS) {
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = q < w ? H[a * ld + j0 + q] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
#pragma unroll
                for (int r = 0; r < q; r++) v[q] -= v[r] * P[q][r];
                v[q] *= ip[q];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) if (q < w) H[a * ld + j0 + q] = v[q];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int p = 0; p < 4; p++) if (p < w) { dg[j0 + p] = ip[p];
#pragma unroll
                for (int q = 0; q <= p; q++) H[(j0 + p) * ld + j0 + q] = P[p][q]; }
        }
        for (int a = j0 + w + ta; a < n; a += 16) {
            const double l0 = H[a * ld + j0], l1 = w > 1 ? H[a * ld + j0 + 1] : 0.0, l2 = w > 2 ? H[a * ld + j0 + 2] : 0.0, l3 = w > 3 ? H[a * ld + j0 + 3] : 0.0;
            const int ce = a < ncol ? a : ncol - 1;
            for (int c = j0 + w + tc; c <= ce; c += 16) {
                double u = l0 * H[c * ld + j0];
                if (w > 1) u += l1 * H[c * ld + j0 + 1];
                if (w > 2) u += l2 * H[c * ld + j0 + 2];
                if (w > 3) u += l3 * H[c * ld + j0 + 3];
                H[a * ld + c] -= u;
            }
        }
        __syncthreads();
    }
    if (tid == 0) *flag = 0;
    return true;
}
// --------------------------------------------------------------------------------------------------
// k_dyn_eval: one workgroup (256 threads) per frame of the launch; frames n < 2 only clear their outputs.
// dynamic LDS (78.7 KB: two workgroups per CU): KinShared | R1 | R2 with, in time order,
//   R2: three evaluation slots (base positions, base evaluations)   ->  G [na][KIN_LS] = A_a^T diag(omega) A_a, kept until H_ff is written
//   R1: A [nq][KIN_LS]  ->  M [(na + 1)][KIN_MS], the node's normal matrix with the right-hand side as its last row, + work  ->  the slot of the evaluation at f*
// (A is written to global memory for k_dyn_assemble anyway; a further active-set round reads it back)
// RAGGED (cpe_solve_kinetic_ragged): N = nmax; the sequence's model picks M and K, frames past its own length leave at once (as in every kernel below)
template <bool RAGGED = false>
__global__ __launch_bounds__(KIN_THREADS) void k_dyn_eval(const DevModel* __restrict__ M, const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N,
                                                          int which, size_t n_frames, const double* __restrict__ qbuf, const int32_t* __restrict__ stance,
                                                          double* __restrict__ fbuf, double* __restrict__ kmu, double* __restrict__ costbuf,
                                                          double* __restrict__ Jbuf, double* __restrict__ Abuf, double* __restrict__ pieces, int* __restrict__ pmeta,
                                                          double* __restrict__ dstat, double* __restrict__ slackbuf, const int* __restrict__ act,
                                                          const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    if (n_act && (int)(blockIdx.x / (unsigned)N) >= *n_act) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l = lane & 31;
    const int b = act ? act[blockIdx.x / (unsigned)N] : (int)(blockIdx.x / (unsigned)N), n = (int)(blockIdx.x % (unsigned)N);
    if constexpr (RAGGED) {
        const int2 rs = rg.seq[b];
        if (n >= rs.y) return;
        M += rs.x; K += rs.x;
    }
    const size_t f_ = (size_t)b * N + n;
    const SeqState Sq = st[b];
    if (Sq.status != 0) return;
    const int pend = Sq.al_pending;
    const int buf = (which || pend) ? Sq.cur : 1 - Sq.cur;
    const int nq = M->nq, ns = M->ns, nf = K->nf, nlat = K->nlat, nrow = K->nrow, nm = K->nm, nc = K->nc, L = M->L;
    const size_t fo = (size_t)buf * n_frames + f_;
    KinShared* Sh = reinterpret_cast<KinShared*>(smem);
    double* R1 = smem + (sizeof(KinShared) + 7) / 8;
    double* R2 = R1 + KE_R1;
    double* A = R1;
    double* ds = dstat + fo * KIN_STAT;
    double* cb = costbuf + fo * COST_STRIDE;
    if (n < 2) {
        if (tid < KIN_STAT) ds[tid] = 0.0;
        if (tid < KIN_LS) fbuf[fo * KIN_LS + tid] = 0.0;
        if (tid < nq) slackbuf[fo * CPE_MAX_NQ + tid] = 0.0;
        if (tid == 0) { pmeta[fo * (KIN_LS + 1)] = 0; pmeta[fo * (KIN_LS + 1) + KIN_LS] = 0; cb[5] = 0.0; }
        return;
    }
    const cpe_kinetic_options& ko = K->o;
#ifdef CPE_LM_STAMPS
    unsigned long long tk_last = __builtin_amdgcn_s_memtime();
#endif
    // ---- load: states of the three frames, warm start, multipliers, stance flags
    for (int t = tid; t < 3 * ns; t += KIN_THREADS) { const int fr = t / ns, p = t - fr * ns; Sh->st[fr][p] = qbuf[((size_t)buf * n_frames + f_ - fr) * ns + p]; }
    if (tid < KIN_LS) { Sh->fw[tid] = tid < nlat ? fbuf[((size_t)Sq.cur * n_frames + f_) * KIN_LS + tid] : 0.0; Sh->f[tid] = 0.0; }
    if (tid < nf * KIN_MU) Sh->mu[tid] = kmu[f_ * (4 * KIN_MU) + tid];
    if (tid < nf) Sh->stance[tid] = stance[f_ * nf + tid];
    const bool tbx = K->tau_box != nullptr;
    const double* gbx = K->grf_box ? K->grf_box + f_ * (size_t)(nf * 6) : nullptr;      // boxes on the foot forces of this node
    if (tbx && tid < 2 * nm) { Sh->tb[tid] = K->tau_box[f_ * (size_t)(2 * nm) + tid]; Sh->mt[tid] = K->mu_tau[f_ * (size_t)(2 * nm) + tid]; }
    const bool sbx = K->sbox != 0;
    if (tid < 2 * nq) Sh->ms[tid] = sbx ? K->mu_slack[f_ * (size_t)(2 * CPE_MAX_NQ) + tid] : 0.0;
    __syncthreads();
    // ---- base positions of the three frames (waves 0..2, slot 0 scratch of each)
    if (wave < 3 && half == 0) kin_positions(M, Sh->st[wave], R2 + wave * KIN_SLOT, Sh->posb[wave], l);
    if (wave == 0 && half == 0) {                            // sin / cos and rotations of frame n (kin_positions left them in the slot): what the columns of A need
        for (int t = l; t < 6 * M->nl; t += 32) Sh->scb[t] = R2[KS_SC + t];
        for (int t = l; t < 9 * M->nl; t += 32) Sh->Rb[t] = R2[KS_R + t];
    }
    __syncthreads();
    // ---- base evaluation (wave 0, half 0): r0 = the rows at node forces 0 -- a chain of one half-wave (22 % of this kernel) -- and BESIDE it, on waves 1 - 3,
    // A [nq][KIN_LS]: e = r0 - A f (12 % when it followed the evaluation on all four waves).  Thread -> (coordinate p, group of columns)
    if (wave == 0) {
        if (half == 0) {
            double* Sl = R2;
            kin_eval(M, K, Sh, Sl, l);
            for (int t = l; t < nrow; t += 32) Sh->r0[t] = Sl[KS_RHO + t];
        }
    } else {
        const int p = tid & 63, grp = (tid >> 6) - 1;
        if (p < nq) {
            const int i = p < 3 ? -1 : (p - 3) / 3, a = p < 3 ? 0 : (p - 3) - 3 * i;
            double D[9] = {0};
            if (i >= 0) rot_kind(Sh->scb + 6 * i, 1 + a, D);
            for (int c = grp; c < KIN_LS; c += 3) {
                double v = 0.0;
                if (c < nm) v = i >= 0 ? kin_coef_motor(K, Sh->scb, Sh->Rb, i, a, c) : 0.0;
                else if (c < nm + nc) v = i >= 0 ? kin_coef_con(M, K, Sh->Rb, D, i, c - nm) : 0.0;
                else if (c < nlat) { const int kf = (c - nm - nc) / 3, d = (c - nm - nc) - 3 * kf; double c3[3]; kin_coef_foot(M, K, D, p, i, kf, c3); v = d == 0 ? c3[2] : (d == 1 ? c3[0] : c3[1]); }
                A[p * KIN_LS + c] = v;
            }
        }
    }
    __syncthreads();
    // ---- multiplier update at the current iterate (pend): forces of its last evaluation (the warm start), geometry of the state -- the foot rows do not
    // depend on the forces; the box on the residual takes e = r0 - A f, below, once A exists
    if (pend) {
        if (tid < nf) {
            const int kf = tid;
            double* m = Sh->mu + kf * KIN_MU; const double* F = Sh->fw + nm + nc + 3 * kf; const double* rho = Sh->r0;
            if (Sh->stance[kf]) {
                if (!K->grf_fix) for (int j = 0; j < 10; j++) { double c3[3], d; kin_force_con(ko, j, c3, &d, gbx ? gbx + 6 * kf : nullptr); kin_al(c3[0] * F[0] + c3[1] * F[1] + c3[2] * F[2] - d, m[j], ko.kappa_force, &m[j]); }
                const double hh = rho[nq + kf];
                kin_al(hh - ko.foot_height_tol, m[10], ko.kappa_height, &m[10]); kin_al(-hh - ko.foot_height_tol, m[11], ko.kappa_height, &m[11]);
                if (ko.slip_max > 0.0) for (int d = 0; d < 2; d++) { const double v = rho[nq + nf + 3 * kf + d];
                    kin_al(v - ko.slip_max, m[12 + 2 * d], ko.kappa_slip, &m[12 + 2 * d]); kin_al(-v - ko.slip_max, m[13 + 2 * d], ko.kappa_slip, &m[13 + 2 * d]); }
                if (ko.zvel_max > 0.0) { const double v = rho[nq + nf + 3 * kf + 2];
                    kin_al(v - ko.zvel_max, m[17], ko.kappa_slip, &m[17]); kin_al(-v - ko.zvel_max, m[18], ko.kappa_slip, &m[18]); }
            } else if (ko.foot_height_min > -1e9) kin_al(ko.foot_height_min - rho[nq + kf], m[16], ko.kappa_height, &m[16]);
        }
        if (tbx && tid >= 64 && tid < 64 + nm) {
            const int m2 = tid - 64;
            kin_al(Sh->tb[2 * m2] - Sh->fw[m2], Sh->mt[2 * m2], ko.kappa_force, &Sh->mt[2 * m2]);
            kin_al(Sh->fw[m2] - Sh->tb[2 * m2 + 1], Sh->mt[2 * m2 + 1], ko.kappa_force, &Sh->mt[2 * m2 + 1]);
        }
    }
    __syncthreads();
    if (pend && tid < nf * KIN_MU) kmu[f_ * (4 * KIN_MU) + tid] = Sh->mu[tid];
    if (pend && tbx && tid < 2 * nm) K->mu_tau[f_ * (size_t)(2 * nm) + tid] = Sh->mt[tid];
    KSTAMP(0);
    for (int t = tid; t < nq * KIN_LS; t += KIN_THREADS) Abuf[f_ * (size_t)(CPE_MAX_NQ * KIN_LS) + t] = A[t];
    // prescribed foot forces (estimate_kinetics(joint_estimation=False), acinoset_opt.py:813-838: GRFz / GRFxy fixed to a given profile): they are
    // constants of the node -- e = (r0 - A_F F) - A_x x -- and the friction / positivity rows do not apply to them
    const bool fixedF = K->grf_fix != nullptr;
    if (fixedF) {
        if (tid < nq) {
            double s = 0.0;
            for (int kf = 0; kf < nf; kf++) if (Sh->stance[kf]) for (int d = 0; d < 3; d++) s += A[tid * KIN_LS + nm + nc + 3 * kf + d] * K->grf_fix[(f_ * nf + kf) * 3 + d];
            Sh->r0[tid] -= s;
        }
        __syncthreads();
    }
    KSTAMP(1);
    // ---- node forces: x = (tau, lambda) are unconstrained and enter quadratically: eliminated by one Cholesky (nx x nx);
    // the net forces F of the stance feet (nF = 3 per stance foot) by a semismooth Newton on the reduced convex piecewise quadratic
    const int nx = nm + nc;
    int nF = 0;
    if (tid == 0) {
        int na = 0;
        for (int m = 0; m < nx; m++) Sh->idx[na++] = m;
        if (!K->grf_fix) for (int kf = 0; kf < nf; kf++) if (Sh->stance[kf]) for (int d = 0; d < 3; d++) Sh->idx[na++] = nx + 3 * kf + d;
        Sh->na = na;
    }
    __syncthreads();
    const int na = Sh->na;
    nF = na - nx;
    double* G = R2;                                   // [nlat][KIN_LS]: A^T diag(omega) A over all columns (read through idx)
    double* Mx = R1;                                  // [na + 1][KIN_MS]: H = 2 w G + D over (x | F), last row the right-hand side; factored on its first nx pivots
    double* Wk = R1 + KIN_MS * KIN_MS;                // work: HF[12][12] | gF | Fv | 1 / diagonal of the factor [52] | the Newton's scratch [352]
    double* bv = Sh->bv; double* HF = Wk; double* gF = HF + 144; double* Fv = gF + 12; double* dg = Fv + 12; double* dF = dg + 52;
    const double w = ko.w_slack, kp = ko.kappa_force, ksl = ko.kappa_slack;
    // Torque boxes (cpe_solve_kinetic_bounded): augmented-Lagrangian rows on tau, piecewise quadratic in x.  Their ACTIVE SET is held fixed while x is
    // eliminated (curvature kappa on the diagonal, the constant of the gradient on the right-hand side) and re-read from the minimiser; the loop
    // ends when it repeats itself -- the semismooth Newton of the oracle, one full elimination per round (one round without boxes).
    int* chg = reinterpret_cast<int*>(Sh->red + 14);
    if (tbx && tid < 2 * nm) { const int m2 = tid >> 1; const double g = (tid & 1) ? Sh->fw[m2] - Sh->tb[tid] : Sh->tb[tid] - Sh->fw[m2]; Sh->tact[tid] = Sh->mt[tid] + kp * g > 0.0 ? 1 : 0; }
    // The box on the residual (bound_eom_error): augmented-Lagrangian rows on e = r0 - A f, piecewise quadratic in ALL node forces.  With its active set
    // held fixed, an active side of row p only changes the weight of that row (w -> w + kappa / 2 per active side) and shifts its target
    // (e_p -> e_p - c_p): the same elimination with G = A^T diag(omega) A, b = A^T diag(omega) (r0 - c).  The set is re-read from the minimiser and the
    // loop ends when it repeats itself (the oracle runs one semismooth Newton on all forces and rows at once).  Start: the set at the warm start.
    if (tid < nq) {
        int su = 0, sl_ = 0;
        if (sbx) {
            double e = Sh->r0[tid];
            for (int a = 0; a < na; a++) e -= A[tid * KIN_LS + Sh->idx[a]] * Sh->fw[Sh->idx[a]];
            if (pend) {                                   // multiplier update of the box at the current iterate, then back to global memory
                kin_al(e - ko.slack_hi, Sh->ms[2 * tid], ksl, &Sh->ms[2 * tid]); kin_al(ko.slack_lo - e, Sh->ms[2 * tid + 1], ksl, &Sh->ms[2 * tid + 1]);
                K->mu_slack[f_ * (size_t)(2 * CPE_MAX_NQ) + 2 * tid] = Sh->ms[2 * tid]; K->mu_slack[f_ * (size_t)(2 * CPE_MAX_NQ) + 2 * tid + 1] = Sh->ms[2 * tid + 1];
            }
            su = Sh->ms[2 * tid] + ksl * (e - ko.slack_hi) > 0.0; sl_ = Sh->ms[2 * tid + 1] + ksl * (ko.slack_lo - e) > 0.0;
        }
        Sh->sact[2 * tid] = su; Sh->sact[2 * tid + 1] = sl_;
    }
    __syncthreads();
    int iters = 0;
    for (int tround = 0;; tround++) {
    iters = 0;
    if (tid < nq) {
        const int su = Sh->sact[2 * tid], sl_ = Sh->sact[2 * tid + 1];
        const double om = 1.0 + (0.5 * ksl / w) * (double)(su + sl_);
        Sh->wsl[tid] = om;
        Sh->csl[tid] = (su + sl_) ? 0.5 * ksl * ((su ? ko.slack_hi - Sh->ms[2 * tid] / ksl : 0.0) + (sl_ ? ko.slack_lo + Sh->ms[2 * tid + 1] / ksl : 0.0)) / (w * om) : 0.0;
    }
    __syncthreads();
    // G over ALL columns of A (the columns of feet in the air cost a fifth more and are never read): 4 x 4 register tiles of the lower triangle,
    // 15 x 16 / 2 = 120 tiles on threads 0..119, two 16-byte LDS reads per 16 multiply-adds; b on threads 128..
    if (tid < 120) {
        int ta = 0, tb = tid; while (tb > ta) { tb -= ta + 1; ta++; }
        double c[4][4] = {{0}};
        for (int p = 0; p < nq; p++) {
            const double wp = Sh->wsl[p];
            const double2 x01 = *reinterpret_cast<const double2*>(A + p * KIN_LS + 4 * ta), x23 = *reinterpret_cast<const double2*>(A + p * KIN_LS + 4 * ta + 2);
            const double2 y01 = *reinterpret_cast<const double2*>(A + p * KIN_LS + 4 * tb), y23 = *reinterpret_cast<const double2*>(A + p * KIN_LS + 4 * tb + 2);
            const double x[4] = {x01.x, x01.y, x23.x, x23.y}, y[4] = {wp * y01.x, wp * y01.y, wp * y23.x, wp * y23.y};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) c[i][j] += x[i] * y[j];
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) { G[(4 * ta + i) * KIN_LS + 4 * tb + j] = c[i][j]; G[(4 * tb + j) * KIN_LS + 4 * ta + i] = c[i][j]; }
    } else if (tid >= 128 && tid < 128 + na) {
        const int a = tid - 128;
        double s = 0.0; for (int p = 0; p < nq; p++) s += A[p * KIN_LS + Sh->idx[a]] * Sh->wsl[p] * (Sh->r0[p] - Sh->csl[p]); bv[a] = s;
    }
    __syncthreads();              // A is dead from here: M takes its place
    KSTAMP(5);
    // M = [H_xx . | H_Fx H_FF | r^T 0] (lower triangle), H = 2 w G + 2 D (+ curvature of the active torque rows), r = 2 w b (+ their constants)
    for (int a = tid >> 4; a <= na; a += 16)
        for (int c = tid & 15; c <= a; c += 16) {
            double v;
            if (a < na) {
                v = 2.0 * w * G[Sh->idx[a] * KIN_LS + Sh->idx[c]] + (a == c ? 2.0 * (a < nm ? ko.w_torque : ko.reg_force) : 0.0);
                if (tbx && a == c && a < nm) v += kp * (double)(Sh->tact[2 * a] + Sh->tact[2 * a + 1]);
            } else if (c < na) {
                v = 2.0 * w * bv[c];
                // constant parts of the active torque rows' gradients: lower side -(m + kappa lo), upper side +(m - kappa hi), moved to the right-hand side
                if (tbx && c < nm) v += (Sh->tact[2 * c] ? Sh->mt[2 * c] + kp * Sh->tb[2 * c] : 0.0) - (Sh->tact[2 * c + 1] ? Sh->mt[2 * c + 1] - kp * Sh->tb[2 * c + 1] : 0.0);
            } else v = 0.0;
            Mx[a * KIN_MS + c] = v;
        }
    __syncthreads();
    int* flag = reinterpret_cast<int*>(Sh->red + 15);
    // nx elimination steps: rows nx.. of the factor are Y^T = H_Fx L^-T and y^T = r_x^T L^-T, the trailing block the reduced problem in F:
    //   Hessian_F = H_FF - Y^T Y (+ kappa sum c c^T of the active force rows);  gradient_F = -(r_F - Y^T y) + Hessian_F F + AL terms
    kin_partial_cholesky_lds(Mx, na + 1, nx, na + 1, KIN_MS, dg, tid, flag);
    KSTAMP(6);
    if (wave == 0) {
        // constant part of the reduced Hessian and gradient (lanes: entries)
        for (int t = lane; t < nF * nF; t += 64) { const int a = t / nF, c = t - a * nF; HF[a * 12 + c] = a >= c ? Mx[(nx + a) * KIN_MS + nx + c] : Mx[(nx + c) * KIN_MS + nx + a]; }
        if (lane < nF) { gF[lane] = -Mx[na * KIN_MS + nx + lane]; Fv[lane] = Sh->fw[Sh->idx[nx + lane]]; }
        wave_lds_sync();
        // The small Newton on F (nF = 3 per stance foot) by the whole wave: lanes = the 10 inequality rows per stance foot for the multiplier terms,
        // lanes = entries for gradient / Hessian / the in-place Cholesky / the two substitutions; every scalar of the control flow (objective, decrease,
        // step length) is the same in all lanes (butterfly sums).  Arrays in the LDS work area; LDS operations of one wave keep their order.
        if (nF > 0) {
            double* Fc = dF; double* gr = Fc + 12; double* dl = gr + 12; double* Ft = dl + 12; double* Hn = Ft + 12; double* PJ = Hn + 144; double* CC = PJ + 40;      // Hn [12][12], CC [40][3]
            const int nfs = nF / 3;
            const bool clane = lane < 10 * nfs;
            double c3[3] = {0.0, 0.0, 0.0}, dcon = 0.0, muj = 0.0; int a0 = 0;
            if (clane) {
                const int fs = lane / 10, jj = lane - 10 * fs, kf = (Sh->idx[nx + 3 * fs] - nx) / 3;
                kin_force_con(ko, jj, c3, &dcon, gbx ? gbx + 6 * kf : nullptr);
                muj = Sh->mu[kf * KIN_MU + jj]; a0 = 3 * fs;
                CC[3 * lane] = c3[0]; CC[3 * lane + 1] = c3[1]; CC[3 * lane + 2] = c3[2];
            }
            if (lane < nF) Fc[lane] = Fv[lane];
            wave_lds_sync();
            auto phi = [&](const double* Fq) {             // reduced objective up to a constant: 1/2 F^T HF F + gF^T F + AL(F)
                double part = 0.0;
                if (lane < nF) { double s = 0.0; for (int c = 0; c < nF; c++) s += HF[lane * 12 + c] * Fq[c]; part = Fq[lane] * (0.5 * s + gF[lane]); }
                if (clane) part += kin_al(c3[0] * Fq[a0] + c3[1] * Fq[a0 + 1] + c3[2] * Fq[a0 + 2] - dcon, muj, kp, nullptr);
                return wave_sum(part);
            };
            double ph = phi(Fc);
            for (; iters < ko.inner_iterations; iters++) {
                double pj = 0.0;
                if (clane) { kin_al(c3[0] * Fc[a0] + c3[1] * Fc[a0 + 1] + c3[2] * Fc[a0 + 2] - dcon, muj, kp, &pj); PJ[lane] = pj; }
                wave_lds_sync();
                if (lane < nF) {
                    double s = gF[lane]; for (int c = 0; c < nF; c++) s += HF[lane * 12 + c] * Fc[c];
                    const int fs = lane / 3, u = lane - 3 * fs;
                    for (int jj = 0; jj < 10; jj++) { const double p = PJ[10 * fs + jj]; if (p > 0.0) s += p * CC[3 * (10 * fs + jj) + u]; }
                    gr[lane] = s;
                }
                for (int t = lane; t < nF * nF; t += 64) {
                    const int a = t / nF, c = t - a * nF, fs = a / 3;
                    double v = HF[a * 12 + c];
                    if (c / 3 == fs) for (int jj = 0; jj < 10; jj++) if (PJ[10 * fs + jj] > 0.0) v += kp * CC[3 * (10 * fs + jj) + a - 3 * fs] * CC[3 * (10 * fs + jj) + c - 3 * fs];
                    Hn[a * 12 + c] = v;
                }
                wave_lds_sync();
                bool ok = true;
                for (int j = 0; j < nF; j++) {
                    const double d = Hn[j * 12 + j];
                    if (!(d > 0.0)) { ok = false; break; }                       // uniform
                    const double sd = sqrt(d);
                    if (lane == j) Hn[j * 12 + j] = sd; else if (lane > j && lane < nF) Hn[lane * 12 + j] /= sd;
                    wave_lds_sync();
                    const int m = nF - j - 1;
                    for (int t = lane; t < m * m; t += 64) { const int i = j + 1 + t / m, c = j + 1 + t % m; if (c <= i) Hn[i * 12 + c] -= Hn[i * 12 + j] * Hn[c * 12 + j]; }
                    wave_lds_sync();
                }
                if (!ok) break;
                if (lane < nF) dl[lane] = -gr[lane];
                wave_lds_sync();
                for (int j = 0; j < nF; j++) {               // L y = -gradient, column sweep
                    const double yj = dl[j] / Hn[j * 12 + j];
                    if (lane == j) dl[j] = yj; else if (lane > j && lane < nF) dl[lane] -= Hn[lane * 12 + j] * yj;
                    wave_lds_sync();
                }
                for (int j = nF - 1; j >= 0; j--) {           // L^T step = y
                    const double xj = dl[j] / Hn[j * 12 + j];
                    if (lane == j) dl[j] = xj; else if (lane < j) dl[lane] -= Hn[j * 12 + lane] * xj;
                    wave_lds_sync();
                }
                const double dec = wave_sum(lane < nF ? -gr[lane] * dl[lane] : 0.0);
                if (!(dec > 1e-22 * (1.0 + fabs(ph)))) break;
                double tt = 1.0, pt = ph;
                for (int ls = 0; ls < 40; ls++) {
                    if (lane < nF) Ft[lane] = Fc[lane] + tt * dl[lane];
                    wave_lds_sync();
                    pt = phi(Ft);
                    if (pt <= ph - 1e-4 * tt * dec || tt < 1e-9) break;
                    tt *= 0.5;
                }
                if (lane < nF) Fc[lane] = Ft[lane];
                wave_lds_sync();
                ph = pt;
            }
            if (lane < nF) Fv[lane] = Fc[lane];
        }
        wave_lds_sync();
        // x = Hxx^-1 (r_x - H_xF F) = L^-T (y - Y F): lane i holds entry i, back substitution over the rows of L (row i is contiguous: lanes k < i)
        double xv = 0.0;
        if (lane < nx) { xv = Mx[na * KIN_MS + lane]; for (int a = 0; a < nF; a++) xv -= Mx[(nx + a) * KIN_MS + lane] * Fv[a]; }
        for (int i = nx - 1; i >= 0; i--) {
            const double xi = __shfl(xv, i, WAVE) * dg[i];
            if (lane == i) xv = xi; else if (lane < i) xv -= Mx[i * KIN_MS + lane] * xi;
        }
        if (lane < KIN_LS) Sh->f[lane] = 0.0;
        wave_lds_sync();
        if (lane < nx) Sh->f[lane] = xv;
        if (lane < nF) Sh->f[Sh->idx[nx + lane]] = Fv[lane];
        if (fixedF && lane < 3 * nf && Sh->stance[lane / 3]) Sh->f[nx + lane] = K->grf_fix[f_ * nf * 3 + lane];
    }
    __syncthreads();
    KSTAMP(2);
    // ---- residual at the round's forces, e = r0 - A_a f (the other rows do not depend on the forces).  M is dead and A went to global memory before
    // the first round: read back, four groups of columns per row, partial sums added in a fixed order
    {
        const int p = tid & 63, gq = tid >> 6;
        double sacc = 0.0;
        if (p < nq) { const double* Ar = Abuf + f_ * (size_t)(CPE_MAX_NQ * KIN_LS) + p * KIN_LS; for (int a = gq; a < na; a += 4) { const int c = Sh->idx[a]; sacc += Ar[c] * Sh->f[c]; } }
        R1[gq * 64 + p] = sacc;
    }
    __syncthreads();
    if (tid < nrow) Sh->rhob[tid] = tid < nq ? Sh->r0[tid] - (((R1[tid] + R1[64 + tid]) + R1[128 + tid]) + R1[192 + tid]) : Sh->r0[tid];
    if (tid == 0) *chg = 0;
    __syncthreads();
    if (!tbx && !sbx) break;
    if (tbx && tid < 2 * nm) {
        const int m2 = tid >> 1; const double g = (tid & 1) ? Sh->f[m2] - Sh->tb[tid] : Sh->tb[tid] - Sh->f[m2];
        const int on = Sh->mt[tid] + kp * g > 0.0 ? 1 : 0;
        if (on != Sh->tact[tid]) { Sh->tact[tid] = on; atomicOr(chg, 1); }
    }
    if (sbx && tid < nq) {
        const double e = Sh->rhob[tid];                   // = r0 - A f
        const int su = Sh->ms[2 * tid] + ksl * (e - ko.slack_hi) > 0.0, sl_ = Sh->ms[2 * tid + 1] + ksl * (ko.slack_lo - e) > 0.0;
        if (su != Sh->sact[2 * tid] || sl_ != Sh->sact[2 * tid + 1]) { Sh->sact[2 * tid] = su; Sh->sact[2 * tid + 1] = sl_; atomicOr(chg, 1); }
    }
    __syncthreads();
    KSTAMP(3);
    if (!*chg || tround >= 11) break;
    for (int t = tid; t < nq * KIN_LS; t += KIN_THREADS) A[t] = Abuf[f_ * (size_t)(CPE_MAX_NQ * KIN_LS) + t];      // another round: A back from global memory
    __syncthreads();
    }
    KSTAMP(3);
    if (tid < KIN_LS) fbuf[fo * KIN_LS + tid] = Sh->f[tid];
    // ---- H_ff (not factored) at the minimiser, active columns compact: pieces [H_uu | H_fu | H_ff], meta [na | idx]
    double* pc = pieces + fo * (size_t)KIN_PIECE;
    double* pHff = pc + KIN_NC3 * KIN_NC3 + KIN_LS * KIN_NC3;
    // (waves 1 - 3; wave 0 works out the cost parts and the row gradients below at the same time: neither reads what the other writes)
    for (int t = tid - 64; t >= 0 && t < na * na; t += KIN_THREADS - 64) {
        const int a = t / na, c = t - a * na;
        double v = 2.0 * w * G[Sh->idx[a] * KIN_LS + Sh->idx[c]] + (a == c ? 2.0 * (a < nm ? ko.w_torque : ko.reg_force) : 0.0);
        if (tbx && a == c && a < nm) v += kp * (double)(Sh->tact[2 * a] + Sh->tact[2 * a + 1]);
        if (a >= nx && c >= nx && (a - nx) / 3 == (c - nx) / 3) {
            const int a0 = nx + 3 * ((a - nx) / 3), kf = (Sh->idx[a0] - nx) / 3;
            for (int j = 0; j < 10; j++) { double c3[3], d, p; kin_force_con(ko, j, c3, &d, gbx ? gbx + 6 * kf : nullptr);
                kin_al(c3[0] * Sh->f[Sh->idx[a0]] + c3[1] * Sh->f[Sh->idx[a0 + 1]] + c3[2] * Sh->f[Sh->idx[a0 + 2]] - d, Sh->mu[kf * KIN_MU + j], kp, &p);
                if (p > 0.0) v += kp * c3[a - a0] * c3[c - a0]; }
        }
        pHff[a * KIN_LS + c] = v;
    }
    if (tid <= na) pmeta[fo * (KIN_LS + 1) + tid] = tid == 0 ? na : Sh->idx[tid - 1];
    if (tid == 0) pmeta[fo * (KIN_LS + 1) + KIN_LS] = iters;       // Newton iterations of this node's force solve (thread 0 ran it; na <= 60: the last word is free)
    if (tid < nq) slackbuf[fo * CPE_MAX_NQ + tid] = Sh->rhob[tid];
    // ---- cost parts, row gradients and weights (psi_r = w_r rho_r^2 for the least-squares rows, augmented-Lagrangian terms for the inequality rows)
    if (wave == 0) {
        const double* rho = Sh->rhob;
        double eom = 0.0, en = 0.0, ms = 0.0, mb = 0.0;
        double alb = 0.0, vb = 0.0;                        // the box on the residual: multiplier terms, largest violation
        for (int p = lane; p < nq; p += 64) {
            const double r = rho[p]; eom += r * r; ms = fmax(ms, fabs(r)); if (p < 3) mb = fmax(mb, fabs(r));
            double gr_ = 2.0 * w * r, wr_ = 2.0 * w;
            if (sbx) {
                double pu, pl; const double gu = r - ko.slack_hi, gl = ko.slack_lo - r;
                alb += kin_al(gu, Sh->ms[2 * p], ksl, &pu); alb += kin_al(gl, Sh->ms[2 * p + 1], ksl, &pl);
                gr_ += pu - pl; wr_ += (pu > 0.0 ? ksl : 0.0) + (pl > 0.0 ? ksl : 0.0);
                vb = fmax(vb, fmax(gu, gl));
            }
            Sh->grow[p] = gr_; Sh->wrow[p] = wr_;
        }
        for (int t = lane; t < 3 * L; t += 64) { const int r = nq + 4 * nf + t; en += rho[r] * rho[r]; Sh->grow[r] = 2.0 * ko.w_smooth * rho[r]; Sh->wrow[r] = 2.0 * ko.w_smooth; }
        // fixed-order sums: lane-strided partials, then a butterfly (same on every run)
        eom = wave_sum(eom); en = wave_sum(en); ms = wave_max(ms); mb = wave_max(mb); alb = wave_sum(alb); vb = wave_max(vb);
        double tq = 0.0, rg = 0.0;
        for (int m = lane; m < nlat; m += 64) { const double v = Sh->f[m]; if (m < nm) tq += v * v; else rg += v * v; }
        tq = wave_sum(tq); rg = wave_sum(rg);
        double al = 0.0, viol = 0.0;
        if (lane < nf) {
            const int kf = lane;
            const double* m = Sh->mu + kf * KIN_MU; const double* F = Sh->f + nx + 3 * kf;
            const int rh = nq + kf;
            double gh = 0.0, wh = 0.0, gv[3] = {0, 0, 0}, wv[3] = {0, 0, 0}, p;
            if (Sh->stance[kf]) {
                if (!fixedF) for (int j = 0; j < 10; j++) { double c3[3], d; kin_force_con(ko, j, c3, &d, gbx ? gbx + 6 * kf : nullptr); const double g = c3[0] * F[0] + c3[1] * F[1] + c3[2] * F[2] - d; al += kin_al(g, m[j], kp, &p); viol = fmax(viol, g); }
                const double hh = rho[rh];
                al += kin_al(hh - ko.foot_height_tol, m[10], ko.kappa_height, &p); gh += p; wh += p > 0.0 ? ko.kappa_height : 0.0;
                al += kin_al(-hh - ko.foot_height_tol, m[11], ko.kappa_height, &p); gh -= p; wh += p > 0.0 ? ko.kappa_height : 0.0;
                viol = fmax(viol, fabs(hh) - ko.foot_height_tol);
                if (ko.slip_max > 0.0)
                    for (int d = 0; d < 2; d++) {
                        const double v = rho[nq + nf + 3 * kf + d];
                        al += kin_al(v - ko.slip_max, m[12 + 2 * d], ko.kappa_slip, &p); gv[d] += p; wv[d] += p > 0.0 ? ko.kappa_slip : 0.0;
                        al += kin_al(-v - ko.slip_max, m[13 + 2 * d], ko.kappa_slip, &p); gv[d] -= p; wv[d] += p > 0.0 ? ko.kappa_slip : 0.0;
                        viol = fmax(viol, (fabs(v) - ko.slip_max) * K->h);
                    }
                if (ko.zvel_max > 0.0) {                  // `foot_z_vel <= 1` of the kinetic dataset (acinoset_opt.py:807-810, :864-866)
                    const double v = rho[nq + nf + 3 * kf + 2];
                    al += kin_al(v - ko.zvel_max, m[17], ko.kappa_slip, &p); gv[2] += p; wv[2] += p > 0.0 ? ko.kappa_slip : 0.0;
                    al += kin_al(-v - ko.zvel_max, m[18], ko.kappa_slip, &p); gv[2] -= p; wv[2] += p > 0.0 ? ko.kappa_slip : 0.0;
                    viol = fmax(viol, (fabs(v) - ko.zvel_max) * K->h);
                }
            } else if (ko.foot_height_min > -1e9) {
                const double g = ko.foot_height_min - rho[rh];
                al += kin_al(g, m[16], ko.kappa_height, &p); gh -= p; wh += p > 0.0 ? ko.kappa_height : 0.0;
                viol = fmax(viol, g);
            }
            Sh->grow[rh] = gh; Sh->wrow[rh] = wh;
            for (int d = 0; d < 3; d++) { Sh->grow[nq + nf + 3 * kf + d] = gv[d]; Sh->wrow[nq + nf + 3 * kf + d] = wv[d]; }
        }
        // feet in index order
        double als = alb, vs = vb;
        for (int kf = 0; kf < nf; kf++) { als += __shfl(al, kf, WAVE); vs = fmax(vs, __shfl(viol, kf, WAVE)); }
        if (tbx) {                                          // torque rows: lane-strided partials, butterfly (fixed order)
            double alt = 0.0, vt = 0.0, p;
            for (int m2 = lane; m2 < nm; m2 += 64) {
                const double glo = Sh->tb[2 * m2] - Sh->f[m2], ghi = Sh->f[m2] - Sh->tb[2 * m2 + 1];
                alt += kin_al(glo, Sh->mt[2 * m2], kp, &p); alt += kin_al(ghi, Sh->mt[2 * m2 + 1], kp, &p);
                vt = fmax(vt, fmax(glo, ghi));
            }
            als += wave_sum(alt); vs = fmax(vs, wave_max(vt));
        }
        if (lane == 0) {
            ds[0] = eom; ds[1] = tq; ds[2] = rg; ds[3] = en; ds[4] = als; ds[5] = ms; ds[6] = mb; ds[7] = vs;
            cb[5] = ko.w_slack * eom + ko.w_torque * tq + ko.w_smooth * en;        // the reference's "motion prior + slack" part of the objective
            cb[1] += ko.reg_force * rg + als;                                        // regularisation + multiplier terms ride with the bound term
            cb[4] = fmax(cb[4], vs);
        }
    }
    __syncthreads();
    // d psi / d rho and the Gauss-Newton weights of the rows ride behind the Jacobian, which k_dyn_jac (cpe_kinetic_jac.hip.inc) writes in closed form
    double* Jg = Jbuf + f_ * (size_t)KIN_JSTRIDE;
    for (int t = tid; t < nrow; t += KIN_THREADS) { Jg[(size_t)KIN_ROWS_MAX * KIN_NC3 + t] = Sh->grow[t]; Jg[(size_t)KIN_ROWS_MAX * KIN_NC3 + KIN_ROWS_MAX + t] = Sh->wrow[t]; }
    KSTAMP(4);
    (void)iters;
}

// --------------------------------------------------------------------------------------------------
// k_dyn_assemble: second-order pieces of a node from J (global scratch) and A: H_uu = J^T W J, H_fu = -A_a^T W_e J_e, gradient J^T (d psi / d rho).
// One workgroup per node, 4 x 4 register tiles: a thread owns one tile of the lower triangle of H_uu (21 x 22 / 2 = 231 tiles) and keeps it in registers
// while the rows of J pass through LDS in two chunks of KA_RC rows (two 16-byte LDS reads per 16 multiply-adds); the 25 threads without a tile take the
// gradient; H_fu (its sum runs over the nq rows of the residual only: chunk 0) in tiles of 4 forces x 4 coordinates afterwards.
// dynamic LDS (79.5 KB: two workgroups per CU): J chunk [KA_RC][KA_RS] row-major | A_a [nq][KIN_LS] | d psi / d rho | row weights
#define KA_RC 72
#define KA_RS (KIN_NC3 + 2)        // even (16-byte rows), not a multiple of 8
static_assert(2 * KA_RC >= KS_NROW && KA_RC >= KS_NQ && KIN_NC3 % 4 == 0 && KIN_NC3 / 4 * (KIN_NC3 / 4 + 1) / 2 <= KIN_THREADS - KIN_NC3 / 4, "tiling of k_dyn_assemble");
template <bool RAGGED = false>
__global__ __launch_bounds__(KIN_THREADS, 2) void k_dyn_assemble(const DevModel* __restrict__ M, const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N,
                                                              int which, size_t n_frames, const double* __restrict__ Jbuf, const double* __restrict__ Abuf,
                                                              double* __restrict__ pieces, const int* __restrict__ pmeta, double* __restrict__ gT,
                                                              const int* __restrict__ act, const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    if (n_act && (int)(blockIdx.x / (unsigned)N) >= *n_act) return;
    const int tid = threadIdx.x;
    const int b = act ? act[blockIdx.x / (unsigned)N] : (int)(blockIdx.x / (unsigned)N), n = (int)(blockIdx.x % (unsigned)N);
    if constexpr (RAGGED) {
        const int2 rs = rg.seq[b];
        if (n >= rs.y) return;
        M += rs.x; K += rs.x;
    }
    const size_t f_ = (size_t)b * N + n;
    const SeqState Sq = st[b];
    if (Sq.status != 0 || (!which && (!Sq.fresh || Sq.al_pending))) return;      // after the accept step, current iterate, only when it is new (see k_dyn_jac)
    const int buf = Sq.cur;
    const size_t fo = (size_t)buf * n_frames + f_;
    double* g = gT + fo * KIN_NC3;
    if (n < 2) { if (tid < KIN_NC3) g[tid] = 0.0; return; }
    const int nq = M->nq, nrow = K->nrow;
    const int na = pmeta[fo * (KIN_LS + 1)];
    const int* idx = pmeta + fo * (KIN_LS + 1) + 1;
    double* J = smem;                                      // [KA_RC][KA_RS]
    double* Aa = J + KA_RC * KA_RS;                        // [nq][KIN_LS], active columns compact, zero beyond na
    double* grow = Aa + KS_NQ * KIN_LS; double* wrow = grow + KS_NROW;
    const double* Jg = Jbuf + f_ * (size_t)KIN_JSTRIDE;
    constexpr int NT = KIN_NC3 / 4, NTILE = NT * (NT + 1) / 2;
    // tile of this thread: (ta, tb), tb <= ta
    int ta = 0, tb = tid;
    if (tid < NTILE) { while (tb > ta) { tb -= ta + 1; ta++; } }
    const bool tile = tid < NTILE, gthr = tid >= NTILE && tid < NTILE + NT;
    const int gk = tid - NTILE;                            // gradient entries 4 gk .. 4 gk + 3
    double c[4][4] = {{0}}, gs[4] = {0, 0, 0, 0};
    // k_dyn_jac stores column-major [84][KIN_ROWS_MAX] (its lanes are rows): consecutive threads along a column, rows of 84 in LDS.  A thread's
    // KA_LD elements of a chunk are requested together (one memory latency per chunk, not one per element), the next chunk's before the arithmetic
    // of the current one.
    constexpr int KA_LD = (KIN_NC3 * KA_RC + KIN_THREADS - 1) / KIN_THREADS;
    double stage[KA_LD];
    auto request = [&](int r0) {
        const int nr = nrow - r0 < KA_RC ? nrow - r0 : KA_RC;
#pragma unroll
        for (int q = 0; q < KA_LD; q++) { const int t = tid + q * KIN_THREADS, a = t / KA_RC, r = t - a * KA_RC; stage[q] = (t < KIN_NC3 * KA_RC && r < nr) ? Jg[(size_t)a * KIN_ROWS_MAX + r0 + r] : 0.0; }
    };
    request(0);
    for (int t = tid; t < nrow; t += KIN_THREADS) { grow[t] = Jg[(size_t)KIN_ROWS_MAX * KIN_NC3 + t]; wrow[t] = Jg[(size_t)KIN_ROWS_MAX * KIN_NC3 + KIN_ROWS_MAX + t]; }
    for (int t = tid; t < nq * KIN_LS; t += KIN_THREADS) { const int p = t / KIN_LS, i = t - p * KIN_LS; Aa[t] = i < na ? Abuf[f_ * (size_t)(CPE_MAX_NQ * KIN_LS) + p * KIN_LS + idx[i]] : 0.0; }
    for (int r0 = 0; r0 < nrow; r0 += KA_RC) {
        const int nr = nrow - r0 < KA_RC ? nrow - r0 : KA_RC;
        if (r0) __syncthreads();                          // the chunk before is consumed
#pragma unroll
        for (int q = 0; q < KA_LD; q++) { const int t = tid + q * KIN_THREADS, a = t / KA_RC, r = t - a * KA_RC; if (t < KIN_NC3 * KA_RC) J[r * KA_RS + a] = stage[q]; }
        if (r0 + KA_RC < nrow) request(r0 + KA_RC);
        __syncthreads();
        if (tile) {
            const double* ja = J + 4 * ta; const double* jb = J + 4 * tb;
            for (int r = 0; r < nr; r++) {
                const double wr = wrow[r0 + r];
                if (wr == 0.0) continue;                   // uniform: an inequality row that is not active
                const double2 x01 = *reinterpret_cast<const double2*>(ja + r * KA_RS), x23 = *reinterpret_cast<const double2*>(ja + r * KA_RS + 2);
                const double2 y01 = *reinterpret_cast<const double2*>(jb + r * KA_RS), y23 = *reinterpret_cast<const double2*>(jb + r * KA_RS + 2);
                const double x[4] = {x01.x, x01.y, x23.x, x23.y}, y[4] = {wr * y01.x, wr * y01.y, wr * y23.x, wr * y23.y};
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) c[i][j] += x[i] * y[j];
            }
        } else if (gthr) {
            for (int r = 0; r < nr; r++) {
                const double gr = grow[r0 + r];
                const double2 x01 = *reinterpret_cast<const double2*>(J + r * KA_RS + 4 * gk), x23 = *reinterpret_cast<const double2*>(J + r * KA_RS + 4 * gk + 2);
                gs[0] += gr * x01.x; gs[1] += gr * x01.y; gs[2] += gr * x23.x; gs[3] += gr * x23.y;
            }
        }
        if (r0 == 0) {
            // H_fu[i][a] = -sum_p A_a[p][i] wrow[p] J[p][a] over the nq rows of the residual (wrow = 2 w, + kappa on an active side of the box)
            double* Hfu = pieces + fo * (size_t)KIN_PIECE + KIN_NC3 * KIN_NC3;
            const int ntc = (na + 3) >> 2;
            for (int t = tid; t < ntc * NT; t += KIN_THREADS) {
                const int tc = t / NT, tu = t - tc * NT;
                double h[4][4] = {{0}};
                for (int p = 0; p < nq; p++) {
                    const double wr = wrow[p];
                    const double2 a01 = *reinterpret_cast<const double2*>(Aa + p * KIN_LS + 4 * tc), a23 = *reinterpret_cast<const double2*>(Aa + p * KIN_LS + 4 * tc + 2);
                    const double2 y01 = *reinterpret_cast<const double2*>(J + p * KA_RS + 4 * tu), y23 = *reinterpret_cast<const double2*>(J + p * KA_RS + 4 * tu + 2);
                    const double x[4] = {a01.x, a01.y, a23.x, a23.y}, y[4] = {wr * y01.x, wr * y01.y, wr * y23.x, wr * y23.y};
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) h[i][j] += x[i] * y[j];
                }
#pragma unroll
                for (int i = 0; i < 4; i++) if (4 * tc + i < na) {
#pragma unroll
                    for (int j = 0; j < 4; j++) Hfu[(4 * tc + i) * KIN_NC3 + 4 * tu + j] = -h[i][j];
                }
            }
        }
    }
    double* Huu = pieces + fo * (size_t)KIN_PIECE;
    if (tile) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) { Huu[(4 * ta + i) * KIN_NC3 + 4 * tb + j] = c[i][j]; Huu[(4 * tb + j) * KIN_NC3 + 4 * ta + i] = c[i][j]; }
    } else if (gthr) {
#pragma unroll
        for (int i = 0; i < 4; i++) g[4 * gk + i] = gs[i];
    }
}


// The node's force matrix as the elimination takes it, with H_uf riding along (k_dyn_schur, k_force_cov), into Mx [na + 84][KIN_MS] by the whole
// workgroup: rows < na the damped H_ff (lower triangle) -- diagonal times 1 + lam_f, lam_f = lambda * lm_force_damping, plus the wall term -- and
// rows na + u the row u of H_uf.  f_: the node's frame, fo: its frame in the current buffer.  Ends with a barrier.
__device__ __forceinline__ void kin_force_matrix(const DevKin* __restrict__ K, const SeqState& Sq, size_t f_, size_t fo, int na, const double* __restrict__ Hfu,
                                                 const double* __restrict__ Hff, const double* __restrict__ fbuf, const double* __restrict__ kmu,
                                                 const int32_t* __restrict__ stance, double* Mx, int tid) {
    const double lamf = Sq.lambda * K->o.lm_force_damping;
    for (int a = tid >> 4; a < na; a += 16) for (int c = tid & 15; c <= a; c += 16) { const double v = Hff[a * KIN_LS + c]; Mx[a * KIN_MS + c] = a == c ? v + lamf * v : v; }
    for (int t = tid; t < na * KIN_NC3; t += KIN_THREADS) { const int a = t / KIN_NC3, u = t - a * KIN_NC3; Mx[(na + u) * KIN_MS + a] = Hfu[t]; }
    __syncthreads();
    // walls: Hessian of a log barrier on the INACTIVE force inequalities of the stance feet, lambda * kb * 2 w c c^T / gap^2 (one thread per foot block entry)
    if (K->o.lm_wall_damping > 0.0 && !K->grf_fix && tid < 9 * K->nf) {
        const int kf = tid / 9, u = (tid - 9 * kf) / 3, v = tid - 9 * kf - 3 * u, fo0 = K->nm + K->nc;
        if (stance[f_ * K->nf + kf]) {
            int a = fo0;
            for (int k2 = 0; k2 < kf; k2++) if (stance[f_ * K->nf + k2]) a += 3;
            const double* F = fbuf + fo * KIN_LS + fo0 + 3 * kf; const double* mu = kmu + f_ * (4 * KIN_MU) + kf * KIN_MU;
            double add = 0.0;
            for (int j = 0; j < 10; j++) {
                double c3[3], d; kin_force_con(K->o, j, c3, &d, K->grf_box ? K->grf_box + (f_ * K->nf + kf) * 6 : nullptr);
                const double g = c3[0] * F[0] + c3[1] * F[1] + c3[2] * F[2] - d;
                if (mu[j] + K->o.kappa_force * g > 0.0) continue;               // active: its curvature is in H_ff already
                const double gap = fmax(-g, 1e-3);
                add += Sq.lambda * K->o.lm_wall_damping * 2.0 * K->o.w_slack / (gap * gap) * c3[u] * c3[v];
            }
            if (v <= u) Mx[(a + u) * KIN_MS + a + v] += add;
        }
    }
    __syncthreads();
}

// --------------------------------------------------------------------------------------------------
// k_dyn_schur: per node of the CURRENT iterate, S = H_uu - H_uf (H_ff + lam_f diag H_ff)^-1 H_fu with lam_f = lambda * lm_force_damping
// (trust region in force space), written as the six lower 28 x 28 blocks [n,n] [n,n-1] [n,n-2] [n-1,n-1] [n-1,n-2] [n-2,n-2].
// dynamic LDS: H [na][KIN_LS] | Y [na][84]
template <bool RAGGED = false>
__global__ __launch_bounds__(KIN_THREADS) void k_dyn_schur(const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                           const double* __restrict__ pieces, const int* __restrict__ pmeta, const double* __restrict__ fbuf,
                                                           const double* __restrict__ kmu, const int32_t* __restrict__ stance, double* __restrict__ Tbuf,
                                                           const int* __restrict__ act, const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    __shared__ int flag;
    if (n_act && (int)(blockIdx.x / (unsigned)N) >= *n_act) return;
    const int tid = threadIdx.x;
    const int b = act ? act[blockIdx.x / (unsigned)N] : (int)(blockIdx.x / (unsigned)N), n = (int)(blockIdx.x % (unsigned)N);
    if constexpr (RAGGED) {
        const int2 rs = rg.seq[b];
        if (n >= rs.y) return;
        K += rs.x;
    }
    const size_t f_ = (size_t)b * N + n;
    const SeqState Sq = st[b];
    if (Sq.status != 0 || Sq.al_pending) return;
    double* T = Tbuf + f_ * (size_t)(6 * CPE_NX * CPE_NX);
    if (n < 2) return;                                       // no node: k_dyn_gather does not read T of frames 0, 1
    const size_t fo = (size_t)Sq.cur * n_frames + f_;
    const int na = pmeta[fo * (KIN_LS + 1)];
    const double* pc = pieces + fo * (size_t)KIN_PIECE;
    const double* Huu = pc; const double* Hfu = pc + KIN_NC3 * KIN_NC3; const double* Hff = Hfu + KIN_LS * KIN_NC3;
    // LDS: Mx [na + 84][KIN_MS]: rows < na the damped H_ff (lower triangle), rows na + u the row u of H_uf; after na elimination steps on the columns
    // < na those rows hold Y^T = H_uf L^-T and the blocks are H_uu - Y^T Y
    double* Mx = smem; double* dg = Mx + (KIN_NA_MAX + KIN_NC3) * KIN_MS;
    kin_force_matrix(K, Sq, f_, fo, na, Hfu, Hff, fbuf, kmu, stance, Mx, tid);
    // blocks: (fa, fb) with fb >= fa (frame n - fa is the ROW frame: later in time), element [i][j] = S[fa nu + i][fb nu + j]; 4 x 4 register tiles,
    // the diagonal blocks by their lower triangle and mirrored: 3 x 28 + 3 x 49 = 231 tiles, one per thread.  The tile of H_uu is requested before
    // the factorisation (its latency hides behind it).
    constexpr int TB = CPE_NX / 4, TD = TB * (TB + 1) / 2;
    static_assert(CPE_NX % 4 == 0 && 3 * TD + 3 * TB * TB <= KIN_THREADS, "tiling of k_dyn_schur");
    const bool tile = tid < 3 * TD + 3 * TB * TB;
    int blk = 0, ti = 0, tj = 0;
    if (tile) {
        if (tid < 3 * TD) { const int d = tid / TD; int r = tid - d * TD; ti = 0; while (r > ti) { r -= ti + 1; ti++; } tj = r; blk = d == 0 ? 0 : (d == 1 ? 3 : 5); }
        else { const int o = (tid - 3 * TD) / (TB * TB), r = (tid - 3 * TD) - o * TB * TB; ti = r / TB; tj = r - ti * TB; blk = o == 0 ? 1 : (o == 1 ? 2 : 4); }
    }
    const int fa = blk < 3 ? 0 : (blk < 5 ? 1 : 2), fb = blk < 3 ? blk : (blk < 5 ? blk - 2 : 2);
    const int ra = fa * CPE_NX + 4 * ti, rb = fb * CPE_NX + 4 * tj;
    double c[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) c[i][j] = tile ? Huu[(ra + i) * KIN_NC3 + rb + j] : 0.0;
    const bool ok = kin_partial_cholesky<9>(Mx, na + KIN_NC3, na, na, KIN_MS, dg, tid, &flag);
    if (tile) {
        if (ok) {
            const double* ya = Mx + (na + ra) * KIN_MS; const double* yb = Mx + (na + rb) * KIN_MS;
            for (int q2 = 0; q2 < na; q2++) {
                double x[4], y[4];
#pragma unroll
                for (int i = 0; i < 4; i++) { x[i] = ya[i * KIN_MS + q2]; y[i] = yb[i * KIN_MS + q2]; }
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) c[i][j] -= x[i] * y[j];
            }
        }
        double* Tb = T + blk * (CPE_NX * CPE_NX);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                Tb[(4 * ti + i) * CPE_NX + 4 * tj + j] = c[i][j];
                if (fa == fb && ti != tj) Tb[(4 * tj + j) * CPE_NX + 4 * ti + i] = c[i][j];
            }
    }
}


// --------------------------------------------------------------------------------------------------
// k_dyn_gather: band blocks and gradient of the whole objective for frame m of the current iterate (single-buffered, read by k_lm_step<PB, 2>):
//   Bk[m]    = B_meas[m] + T_m[n,n] + T_m+1[n-1,n-1] + T_m+2[n-2,n-2]
//   Hk[m][0] = block (m, m-1) = T_m[n,n-1] + T_m+1[n-1,n-2] ;  Hk[m][1] = block (m, m-2) = T_m[n,n-2] ;  Hk[m][2] = 0
//   gk[m]    = g_meas[m] + gT_m[0] + gT_m+1[1] + gT_m+2[2]
template <bool RAGGED = false>
__global__ __launch_bounds__(KIN_THREADS) void k_dyn_gather(const SeqState* __restrict__ st, int N, size_t n_frames, const double* __restrict__ gbuf,
                                                            const double* __restrict__ Bbuf, const double* __restrict__ Tbuf, const double* __restrict__ gT,
                                                            double* __restrict__ gk, double* __restrict__ Bk, double* __restrict__ Hk,
                                                            const int* __restrict__ act, const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{}) {
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, act, n_act, rg, fs)) return;
    const int tid = threadIdx.x;
    const int b = fs.b, m = fs.n, NL = fs.len;           // N: the buffers' frames per sequence, NL: this sequence's length (nodes m + 1, m + 2 inside it)
    const size_t f_ = (size_t)b * N + m;
    const SeqState Sq = st[b];
    if (Sq.status != 0 || Sq.al_pending) return;
    const size_t fo = (size_t)Sq.cur * n_frames + f_;
    constexpr int BB = CPE_NX * CPE_NX;
    const double* T0 = Tbuf + f_ * (size_t)(6 * BB); const double* T1 = T0 + 6 * BB; const double* T2 = T1 + 6 * BB;
    const bool h0 = m >= 2, h1 = m + 1 < NL && m + 1 >= 2, h2 = m + 2 < NL;
    for (int e = tid; e < BB; e += KIN_THREADS) {
        double v = Bbuf[fo * BB + e];
        if (h0) v += T0[e];
        if (h1) v += T1[3 * BB + e];
        if (h2) v += T2[5 * BB + e];
        Bk[f_ * BB + e] = v;
        double a = 0.0;
        if (h0) a += T0[1 * BB + e];
        if (h1) a += T1[4 * BB + e];
        Hk[(f_ * 3 + 0) * BB + e] = a;
        Hk[(f_ * 3 + 1) * BB + e] = h0 ? T0[2 * BB + e] : 0.0;
        Hk[(f_ * 3 + 2) * BB + e] = 0.0;
    }
    if (tid < CPE_NX) {
        double v = gbuf[fo * CPE_NX + tid];
        if (h0) v += gT[fo * KIN_NC3 + tid];
        if (h1) v += gT[(fo + 1) * KIN_NC3 + CPE_NX + tid];
        if (h2) v += gT[(fo + 2) * KIN_NC3 + 2 * CPE_NX + tid];
        gk[f_ * CPE_NX + tid] = v;
    }
}

// outputs of the physics-based solve: node forces of the final iterate as the reference stores them (tau, Fr, GRFz / GRFxy) and slack_eom
template <bool RAGGED = false>
__global__ void k_dyn_outputs(const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N, size_t n_frames, const double* __restrict__ fbuf,
                              const double* __restrict__ Abuf, const double* __restrict__ dummy, double* __restrict__ tau, double* __restrict__ lam,
                              double* __restrict__ grf, RaggedArgs rg = RaggedArgs{} /* RAGGED: frames past a sequence's own are written as zeros */) {
    const size_t f_ = blockIdx.x;
    FrameSlot fs;
    const bool own = frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs);
    K += fs.model;                                         // (the counts nm, nc, nf are the same in every model of the handle)
    const int b = fs.b, n = fs.n, t = threadIdx.x;
    const double* f = fbuf + ((size_t)st[b].cur * n_frames + f_) * KIN_LS;
    const bool on = n >= 2 && own;
    if (tau && t < K->nm) tau[f_ * K->nm + t] = on ? f[t] : 0.0;
    if (lam && t < K->nc) lam[f_ * K->nc + t] = on ? f[K->nm + t] : 0.0;
    if (grf && t < K->nf) {
        const double* F = f + K->nm + K->nc + 3 * t;
        double* o = grf + (f_ * K->nf + t) * 5;
        o[0] = on ? F[0] : 0.0;
        o[1] = on && F[1] > 0.0 ? F[1] : 0.0; o[2] = on && F[2] > 0.0 ? F[2] : 0.0;
        o[3] = on && F[1] < 0.0 ? -F[1] : 0.0; o[4] = on && F[2] < 0.0 ? -F[2] : 0.0;
    }
    (void)Abuf; (void)dummy;
}
