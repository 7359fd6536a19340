// cpe_kinetic_jac.hip.inc -- analytic Jacobian of the node rows of the physics-based model (included by cpe_kernels.hip after cpe_kinetic.hip.inc).
//
// k_dyn_jac: one workgroup per node n >= 2.  J [nrow][84] = d rho / d (u_n | u_n-1 | u_n-2) for the residual vector of cpe_kinetic.hip.inc
//   rho = [ e = rows(q0, q', q'') / Mg - A(q0) f | foot heights | foot velocities (d foot / d q) q' | fps^2 second differences of the markers ],
//   q0 = Q(u_n), a1 = nearest(q0, Q(u_n-1)), a2 = nearest(a1, Q(u_n-2)), q' = (q0 - a1) / h, q'' = (q0 - 2 a1 + a2) / h^2,
// in closed form (round 2 took 168 central differences of the whole evaluation).  What the reference gets from ASL's automatic differentiation of
// the Pyomo expression trees of make_pyomo_model(include_eom_slack=True) (acinoset_opt.py:510-514), here written out for the absolute-orientation
// chain:
//   * every point of the body is x + sum_k R_k(theta_k) v_k, so with B_k = d^2 R_k / dt^2 (a 3 x 3 matrix of link k's own angles, rates and
//     accelerations), the first moments s_i = sum_{j in subtree(i)} m_j v_ji and second moments S_i = sum m_j v_ji v_ji^T of every subtree about
//     its link's origin (constants), the rows are
//         row(i, a) = (d_a R_i s_i) . A_i + < (d_a R_i)^T B_i , S_i > + sum_{c child of i} (d_a R_i attach_c) . D_c + (I alpha + w x I w)_i . dw_i/dq'_a ,
//         A_i = x'' + g e_z + sum_{k ancestor of i} B_k v_k->i ,   D_c = sum_{k in subtree(c)} B_k s_k ,   row(x_d) = M (x'' + g e_z)_d + sum_k (B_k s_k)_d
//     and their derivatives with respect to (theta, theta', theta'') of link k touch row (i, a) only if k is an ancestor of i, a descendant, or i itself:
//     89 link pairs of the cheetah, 9 numbers each, per kind -- K (angles), C (rates), M (accelerations: the mass matrix);
//   * d B_k / d(theta'', theta', theta)_b = d_b R , 2 sum_a d_ab R theta'_a , sum_a d_ab R theta''_a + sum_ac d_abc R theta'_a theta'_c: derivatives of
//     R = Rz Ry Rx of any order are products of shifted elementary rotations;
//   * the rotational term of a link is a function of its own nine numbers: differentiated by forward-mode arithmetic (value + one tangent per lane);
//   * the generalised forces A(q0) f: second derivatives of foot points (same link only), of the joint equalities (parent / child), of the motor axes;
//   * the coordinate map Q(u) (DESIGN.md 2): leg link c = R_B Ry(alpha): d(Euler_c) / d(alpha, Euler_B) = Jw_c^-1 [ e_y | Ry(alpha)^T Jw_B ];
//     roll of a tail from its Hooke equality by implicit differentiation, chained through the parent's roll;
//   * nearest(): signs of the equivalent triple and, next to the pole of the chart, the 3 x 3 blocks of the shift along phi -+ psi = const.
// One column (frame, coordinate) = one direction (d q0, d q', d q'') per touched link (<= 9 links); a wave evaluates one column at a time, lanes = rows.
// All sums have a fixed order: bit-reproducible.  The CPU checker holds a dense restatement of the same derivatives and a numerical one (fourth-order differences) beside it.

#define KJ_THREADS 256
#define KJ_MAXB 96                 // related (ancestor / descendant / same) link pairs: 89 for the cheetah
#define KJ_NH 4                    // Hooke joints (2)
#define KJ_CHAIN 5                 // links on the path root -> marker that k_dyn_jac keeps in registers (paw: base, bodyF, thigh, calf, hock); build_kin refuses longer chains

struct KjD1 { double v, d; };      // value + one tangent
__device__ __forceinline__ KjD1 operator+(KjD1 a, KjD1 b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ KjD1 operator-(KjD1 a, KjD1 b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ KjD1 operator-(KjD1 a) { return {-a.v, -a.d}; }
__device__ __forceinline__ KjD1 operator*(KjD1 a, KjD1 b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ KjD1 operator*(double a, KjD1 b) { return {a * b.v, a * b.d}; }
__device__ __forceinline__ KjD1 kj_sin(KjD1 a) { double s, c; sincos(a.v, &s, &c); return {s, c * a.d}; }
__device__ __forceinline__ KjD1 kj_cos(KjD1 a) { double s, c; sincos(a.v, &s, &c); return {c, -s * a.d}; }

// (I alpha + w x I w) . dw/dq'_a for a = 0..2: body rates from the link's own Euler angles, rates and accelerations (k_eom's arithmetic on KjD1)
__device__ __forceinline__ void kj_rot_rows(const KjD1* th, const KjD1* dth, const KjD1* ddth, const double* I, KjD1* out) {
    const KjD1 sf = kj_sin(th[0]), cf = kj_cos(th[0]), st = kj_sin(th[1]), ct = kj_cos(th[1]);
    const KjD1 zero = {0.0, 0.0}, one = {1.0, 0.0};
    const KjD1 c0[3] = {one, zero, zero}, c1[3] = {zero, cf, -sf}, c2[3] = {-st, sf * ct, cf * ct};
    const KjD1 d1[3] = {zero, -(sf * dth[0]), -(cf * dth[0])};
    const KjD1 d2[3] = {-(ct * dth[1]), cf * dth[0] * ct - sf * st * dth[1], -(sf * dth[0] * ct) - cf * st * dth[1]};
    KjD1 w[3], al[3];
    for (int t = 0; t < 3; t++) {
        w[t] = c0[t] * dth[0] + c1[t] * dth[1] + c2[t] * dth[2];
        al[t] = c0[t] * ddth[0] + c1[t] * ddth[1] + c2[t] * ddth[2] + d1[t] * dth[1] + d2[t] * dth[2];
    }
    const KjD1 Iw[3] = {I[0] * w[0], I[1] * w[1], I[2] * w[2]};
    const KjD1 tq[3] = {I[0] * al[0] + (w[1] * Iw[2] - w[2] * Iw[1]), I[1] * al[1] + (w[2] * Iw[0] - w[0] * Iw[2]), I[2] * al[2] + (w[0] * Iw[1] - w[1] * Iw[0])};
    out[0] = tq[0] * c0[0] + tq[1] * c0[1] + tq[2] * c0[2];
    out[1] = tq[0] * c1[0] + tq[1] * c1[1] + tq[2] * c1[2];
    out[2] = tq[0] * c2[0] + tq[1] * c2[1] + tq[2] * c2[2];
}

// d^(n0 + n1 + n2) R / d phi^n0 d theta^n1 d psi^n2 of R = Rz(psi) Ry(theta) Rx(phi), row-major; sc = sin / cos of (phi, theta, psi)
__device__ __forceinline__ void kj_drot(const double* sc, int n0, int n1, int n2, double* M) {
    // n-th derivative of (sin, cos): (s, c), (c, -s), (-s, -c), (-c, s)
    auto ds = [](double s, double c, int n) { n &= 3; return n == 0 ? s : (n == 1 ? c : (n == 2 ? -s : -c)); };
    auto dc = [](double s, double c, int n) { n &= 3; return n == 0 ? c : (n == 1 ? -s : (n == 2 ? -c : s)); };
    const double sx = ds(sc[0], sc[1], n0), cx = dc(sc[0], sc[1], n0), sy = ds(sc[2], sc[3], n1), cy = dc(sc[2], sc[3], n1), sz = ds(sc[4], sc[5], n2), cz = dc(sc[4], sc[5], n2);
    const double o0 = n0 ? 0.0 : 1.0, o1 = n1 ? 0.0 : 1.0, o2 = n2 ? 0.0 : 1.0;
    const double a00 = cy * o0, a01 = sy * sx, a02 = sy * cx, a10 = 0.0, a11 = o1 * cx, a12 = -o1 * sx, a20 = -sy * o0, a21 = cy * sx, a22 = cy * cx;
    M[0] = cz * a00 - sz * a10; M[1] = cz * a01 - sz * a11; M[2] = cz * a02 - sz * a12;
    M[3] = sz * a00 + cz * a10; M[4] = sz * a01 + cz * a11; M[5] = sz * a02 + cz * a12;
    M[6] = o2 * a20;            M[7] = o2 * a21;            M[8] = o2 * a22;
}
// columns of the Euler-rate map Jw(phi, theta) = [c0 c1 c2] (body rates w = Jw theta') and their derivatives: (n0, n1) orders in phi, theta
__device__ __forceinline__ void kj_cvec(const double* sc, int a, int n0, int n1, double* c) {
    auto ds = [](double s, double cc, int n) { n &= 3; return n == 0 ? s : (n == 1 ? cc : (n == 2 ? -s : -cc)); };
    auto dc = [](double s, double cc, int n) { n &= 3; return n == 0 ? cc : (n == 1 ? -s : (n == 2 ? -cc : s)); };
    const double sf = ds(sc[0], sc[1], n0), cf = dc(sc[0], sc[1], n0), st = ds(sc[2], sc[3], n1), ct = dc(sc[2], sc[3], n1);
    if (a == 0) { c[0] = (n0 | n1) ? 0.0 : 1.0; c[1] = 0.0; c[2] = 0.0; }
    else if (a == 1) { c[0] = 0.0; c[1] = n1 ? 0.0 : cf; c[2] = n1 ? 0.0 : -sf; }
    else { c[0] = n0 ? 0.0 : -st; c[1] = sf * ct; c[2] = cf * ct; }
}
__device__ __forceinline__ int kj_pair(int a, int b) { const int lo = a < b ? a : b, hi = a < b ? b : a; return lo == 0 ? hi : (lo == 1 ? 2 + hi : 5); }      // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> 0..5
__device__ __forceinline__ double kj_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void kj_mv(const double* Mx, const double* v, double* o) { o[0] = Mx[0] * v[0] + Mx[1] * v[1] + Mx[2] * v[2]; o[1] = Mx[3] * v[0] + Mx[4] * v[1] + Mx[5] * v[2]; o[2] = Mx[6] * v[0] + Mx[7] * v[1] + Mx[8] * v[2]; }
__device__ __forceinline__ void kj_m3v(const double* B, const double* v, double* o) { kj_mv(B, v, o); }

// nearest equivalent triple of link angles a (3) to r (3) with the pole shift of kin_nearest_link, and the 3 x 3 blocks S = d out / d a, P = d out / d r
__device__ __forceinline__ void kj_nearest(const double* r, const double* a, double* out, double* S, double* P) {
    const double TWO_PI = 6.283185307179586476925286766559, PI = 3.14159265358979323846264338327950288;
    const double alt[3] = {a[0] + PI, PI - a[1], a[2] + PI};
    double c1[3], c2[3], d1 = 0.0, d2 = 0.0;
    for (int k = 0; k < 3; k++) {
        c1[k] = a[k] + TWO_PI * rint((r[k] - a[k]) / TWO_PI);
        c2[k] = alt[k] + TWO_PI * rint((r[k] - alt[k]) / TWO_PI);
        d1 += (c1[k] - r[k]) * (c1[k] - r[k]); d2 += (c2[k] - r[k]) * (c2[k] - r[k]);
    }
    const bool al = d2 < d1;
    double o[3];
    for (int k = 0; k < 3; k++) o[k] = al ? c2[k] : c1[k];
    const double sth = al ? -1.0 : 1.0;                       // d o_theta / d a_theta
    for (int k = 0; k < 9; k++) { S[k] = 0.0; P[k] = 0.0; }
    S[0] = 1.0; S[4] = sth; S[8] = 1.0;
    const double cth = cos(o[1]), ct = fabs(cth);
    if (ct < KIN_POLE) {
        const double sg = sin(o[1]) > 0.0 ? 1.0 : -1.0;
        const double t = 0.5 * ((r[0] - o[0]) + sg * (r[2] - o[2]));
        const bool blend = ct > 0.5 * KIN_POLE;
        const double u = blend ? (ct - 0.5 * KIN_POLE) / (0.5 * KIN_POLE) : 0.0, w = 1.0 - u * u * (3.0 - 2.0 * u);
        // d w / d theta = dw/du du/dct dct/dtheta, dct/dtheta = -sign(cos) sin
        const double dw = blend ? (-6.0 * u * (1.0 - u)) * (2.0 / KIN_POLE) * (-(cth > 0.0 ? 1.0 : -1.0) * sin(o[1])) : 0.0;
        // rows of d o' / d o : o0' = o0 + w t, o2' = o2 + w sg t
        const double Do[9] = {1.0 - 0.5 * w, t * dw, -0.5 * w * sg,   0.0, 1.0, 0.0,   -0.5 * w * sg, sg * t * dw, 1.0 - 0.5 * w};
        // S = Do . diag(1, sth, 1)
        for (int i = 0; i < 3; i++) { S[3 * i] = Do[3 * i]; S[3 * i + 1] = Do[3 * i + 1] * sth; S[3 * i + 2] = Do[3 * i + 2]; }
        P[0] = 0.5 * w; P[2] = 0.5 * w * sg; P[6] = 0.5 * w * sg; P[8] = 0.5 * w;
        o[0] += w * t; o[2] += w * sg * t;
    }
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
}

#if defined(CPE_LM_STAMPS) && defined(CPE_JAC_STAMPS)
#define JSTAMP(i) do { if (blockIdx.x == 5 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_fn_stamps[i] += t_ - tj_last; tj_last = t_; } } while (0)
#else
#define JSTAMP(i) do { } while (0)
#endif
// LDS layout of k_dyn_jac (offsets in doubles)
#define KJ_E 0                                   // [3][KS_NS] states
#define KJ_A1 (KJ_E + 3 * KS_NS)                 // [KS_NQ]
#define KJ_A2 (KJ_A1 + KS_NQ)
#define KJ_DQ (KJ_A2 + KS_NQ)
#define KJ_DDQ (KJ_DQ + KS_NQ)
#define KJ_SC (KJ_DDQ + KS_NQ)                   // [3][KS_NL][6]
#define KJ_R (KJ_SC + 18 * KS_NL)                // [KS_NL][9]              frame n
#define KJ_D1R (KJ_R + 9 * KS_NL)                // [3][KS_NL][3][9]
#define KJ_D2R (KJ_D1R + 81 * KS_NL)             // [KS_NL][6][9]           frame n
#define KJ_NB (KJ_D2R + 54 * KS_NL)              // [KS_NL][4][9]: S1, P1, S2, P2
#define KJ_B (KJ_NB + 36 * KS_NL)                // [KS_NL][9]
#define KJ_TBS (KJ_B + 9 * KS_NL)                // [KS_NL][9][3]           (dB_k / d local j) s_k
#define KJ_TBA (KJ_TBS + 27 * KS_NL)             // [KS_NL][9][3]           (dB_parent(c) / d local j) attach_c, indexed by the child c
#define KJ_SQ (KJ_TBA + 27 * KS_NL)              // [KS_NL][3][9]           self terms of row (i, a) with respect to local j of link i
#define KJ_AC (KJ_SQ + 27 * KS_NL)               // [KS_NL][3]  A_i
#define KJ_DS (KJ_AC + 3 * KS_NL)                // [KS_NL][3]  D_i = sum over the subtree of i of B_k s_k
#define KJ_BV (KJ_DS + 3 * KS_NL)                // [KS_NL][3]  B_i s_i
#define KJ_DRS (KJ_BV + 3 * KS_NL)               // [KS_NL][3][3]  d_a R_i s_i
#define KJ_DRA (KJ_DRS + 9 * KS_NL)              // [KS_NL][3][3]  d_a R_parent(c) attach_c, by child c
#define KJ_KF (KJ_DRA + 9 * KS_NL)               // [KJ_MAXB][9]   K / Mg - d(A f)/dq
#define KJ_CB (KJ_KF + 9 * KJ_MAXB)
#define KJ_MB (KJ_CB + 9 * KJ_MAXB)
#define KJ_GL (KJ_MB + 9 * KJ_MAXB)              // [3][CPE_MAX_JOINTS][12]  d Euler_c / d (alpha, Euler_B), row-major [3][4]
#define KJ_GP (KJ_GL + 36 * CPE_MAX_JOINTS)      // [3][KJ_NH][CPE_NX]       d phi_child / d u
#define KJ_F (KJ_GP + 3 * KJ_NH * CPE_NX)        // [KIN_LS]
#define KJ_TL (KJ_F + KIN_LS)                    // [4 waves][KS_NL][12]     direction of the wave's column: raw (3), d q0 (3), d q' (3), d q'' (3)
#define KJ_TT (KJ_TL + 4 * KS_NL * 12)           // [4 waves][12]            translation part: raw of frames 0, 1, 2 (3), d x' (3), d x'' (3), pad
#define KJ_DOUBLES (KJ_TT + 4 * 12)

template <bool RAGGED = false>
__global__ __launch_bounds__(KJ_THREADS) void k_dyn_jac(const DevModel* __restrict__ M, const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N, int which,
                                                         size_t n_frames, const double* __restrict__ qbuf, const double* __restrict__ fbuf, double* __restrict__ Jbuf,
                                                         const int* __restrict__ act, const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double sm[];
    if (n_act && (int)(blockIdx.x / (unsigned)N) >= *n_act) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = act ? act[blockIdx.x / (unsigned)N] : (int)(blockIdx.x / (unsigned)N), n = (int)(blockIdx.x % (unsigned)N);
    if constexpr (RAGGED) {                                  // (see k_dyn_eval)
        const int2 rs = rg.seq[b];
        if (n >= rs.y) return;
        M += rs.x; K += rs.x;
    }
    const size_t f_ = (size_t)b * N + n;
    const SeqState Sq = st[b];
    // runs AFTER the accept step, on the current iterate, and only when that iterate is new (a rejected trial leaves the pieces of the current
    // iterate standing; `which`: evaluation on request, cpe_eval_kinetic_nodes)
    if (Sq.status != 0 || n < 2 || (!which && (!Sq.fresh || Sq.al_pending))) return;
    const int buf = Sq.cur;
    const size_t fo = (size_t)buf * n_frames + f_;
    const int nq = M->nq, ns = M->ns, nl = M->nl, nf = K->nf, nm = K->nm, nc = K->nc, L = M->L, nrow = K->nrow, nu = M->nu;
    const double ih = K->ih, ih2 = K->ih * K->ih, iMg = 1.0 / K->Mg;
    double* E = sm + KJ_E;
#if defined(CPE_LM_STAMPS) && defined(CPE_JAC_STAMPS)
    unsigned long long tj_last = __builtin_amdgcn_s_memtime();
#endif
    // ---- states of the three frames, node forces
    for (int t = tid; t < 3 * ns; t += KJ_THREADS) { const int fr = t / ns, p = t - fr * ns; E[fr * KS_NS + p] = qbuf[((size_t)buf * n_frames + f_ - fr) * ns + p]; }
    if (tid < KIN_LS) sm[KJ_F + tid] = fbuf[fo * KIN_LS + tid];
    {   // lists of the force terms per link pair, bytes: counts of motors [KJ_MAXB] | of equality rows [KJ_MAXB] | motors [KJ_MAXB][KJ_LMAX] | rows [KJ_MAXB][KJ_LMAX];
        // parked in the column phase's direction buffers (free until then)
        unsigned char* lb = reinterpret_cast<unsigned char*>(sm + KJ_TL);
        for (int t = tid; t < KJ_MAXB; t += KJ_THREADS) { lb[t] = K->bm_n[t]; lb[KJ_MAXB + t] = K->bc_n[t]; }
        for (int t = tid; t < KJ_MAXB * KJ_LMAX; t += KJ_THREADS) { lb[2 * KJ_MAXB + t] = K->bm[t / KJ_LMAX][t % KJ_LMAX]; lb[2 * KJ_MAXB + KJ_MAXB * KJ_LMAX + t] = K->bc[t / KJ_LMAX][t % KJ_LMAX]; }
    }
    __syncthreads();
    // ---- sin / cos of every angle of the three frames
    for (int t = tid; t < 9 * nl; t += KJ_THREADS) { const int fr = t / (3 * nl), r = t - fr * 3 * nl; double s_, c_; sincos(E[fr * KS_NS + 3 + r], &s_, &c_); sm[KJ_SC + fr * 6 * KS_NL + 2 * r] = s_; sm[KJ_SC + fr * 6 * KS_NL + 2 * r + 1] = c_; }
    __syncthreads();
    // ---- rotations and their derivatives; nearest triples of frames n-1, n-2 with their blocks
    for (int t = tid; t < 9 * nl; t += KJ_THREADS) { const int fr = t / (3 * nl), r = t - fr * 3 * nl, i = r / 3, a = r - 3 * i; rot_kind(sm + KJ_SC + fr * 6 * KS_NL + 6 * i, 1 + a, sm + KJ_D1R + (fr * KS_NL + i) * 27 + 9 * a); }
    for (int t = tid; t < 6 * nl; t += KJ_THREADS) { const int i = t / 6, pr = t - 6 * i; const int a = pr < 3 ? 0 : (pr < 5 ? 1 : 2), c = pr < 3 ? pr : (pr < 5 ? pr - 2 : 2);
        kj_drot(sm + KJ_SC + 6 * i, (a == 0) + (c == 0), (a == 1) + (c == 1), (a == 2) + (c == 2), sm + KJ_D2R + i * 54 + 9 * pr); }
    if (tid < nl) rot_kind(sm + KJ_SC + 6 * tid, 0, sm + KJ_R + 9 * tid);
    if (tid >= 64 && tid < 64 + nl) {
        const int i = tid - 64;
        double* nb = sm + KJ_NB + i * 36;
        kj_nearest(E + 3 + 3 * i, E + KS_NS + 3 + 3 * i, sm + KJ_A1 + 3 + 3 * i, nb, nb + 9);                            // a1 = nearest(q0, q1): S1, P1
        kj_nearest(sm + KJ_A1 + 3 + 3 * i, E + 2 * KS_NS + 3 + 3 * i, sm + KJ_A2 + 3 + 3 * i, nb + 18, nb + 27);           // a2 = nearest(a1, q2): S2, P2
    }
    if (tid >= 128 && tid < 131) { sm[KJ_A1 + tid - 128] = E[KS_NS + tid - 128]; sm[KJ_A2 + tid - 128] = E[2 * KS_NS + tid - 128]; }
    __syncthreads();
    if (tid < nq) { sm[KJ_DQ + tid] = (E[tid] - sm[KJ_A1 + tid]) * ih; sm[KJ_DDQ + tid] = (E[tid] - 2.0 * sm[KJ_A1 + tid] + sm[KJ_A2 + tid]) * ih2; }
    __syncthreads();
    JSTAMP(0);
    // ---- per link and local variable j (0-2 angles, 3-5 rates, 6-8 accelerations): dB = d B / d local_j; its products with the link's moments
    for (int t = tid; t < 9 * nl; t += KJ_THREADS) {
        const int i = t / 9, j = t - 9 * i, ty = j / 3, bb = j - 3 * ty;
        const double* sc = sm + KJ_SC + 6 * i; const double* d1r = sm + KJ_D1R + i * 27; const double* d2r = sm + KJ_D2R + i * 54;
        const double* dq = sm + KJ_DQ + 3 + 3 * i; const double* ddq = sm + KJ_DDQ + 3 + 3 * i;
        double dB[9];
        if (ty == 2) for (int e = 0; e < 9; e++) dB[e] = d1r[9 * bb + e];
        else if (ty == 1) for (int e = 0; e < 9; e++) dB[e] = 2.0 * (d2r[9 * kj_pair(0, bb) + e] * dq[0] + d2r[9 * kj_pair(1, bb) + e] * dq[1] + d2r[9 * kj_pair(2, bb) + e] * dq[2]);
        else {
            for (int e = 0; e < 9; e++) dB[e] = d2r[9 * kj_pair(0, bb) + e] * ddq[0] + d2r[9 * kj_pair(1, bb) + e] * ddq[1] + d2r[9 * kj_pair(2, bb) + e] * ddq[2];
            for (int a = 0; a < 3; a++) for (int c = a; c < 3; c++) {
                double T3[9];
                kj_drot(sc, (a == 0) + (c == 0) + (bb == 0), (a == 1) + (c == 1) + (bb == 1), (a == 2) + (c == 2) + (bb == 2), T3);
                const double wgt = (a == c ? 1.0 : 2.0) * dq[a] * dq[c];
                for (int e = 0; e < 9; e++) dB[e] += wgt * T3[e];
            }
        }
        kj_mv(dB, K->s1[i], sm + KJ_TBS + (i * 9 + j) * 3);
        for (int c = 0; c < nl; c++) if (M->parent[c] == i) kj_mv(dB, M->attach[c], sm + KJ_TBA + (c * 9 + j) * 3);
        // self terms: < (d_a R_i)^T dB , S_i > + d rot_a / d local_j
        double Tm[9];
        const double* S2 = K->S2[i];
        for (int m = 0; m < 3; m++) for (int c = 0; c < 3; c++) Tm[3 * m + c] = dB[3 * m] * S2[c] + dB[3 * m + 1] * S2[3 + c] + dB[3 * m + 2] * S2[6 + c];
        KjD1 th[3], dth[3], ddth[3], ro[3];
        for (int a = 0; a < 3; a++) { th[a] = {E[3 + 3 * i + a], j == a ? 1.0 : 0.0}; dth[a] = {dq[a], j == 3 + a ? 1.0 : 0.0}; ddth[a] = {ddq[a], j == 6 + a ? 1.0 : 0.0}; }
        kj_rot_rows(th, dth, ddth, K->o.dyn.eom.link_inertia[i], ro);
        for (int a = 0; a < 3; a++) { double s = 0.0; for (int e = 0; e < 9; e++) s += d1r[9 * a + e] * Tm[e]; sm[KJ_SQ + (i * 3 + a) * 9 + j] = s + ro[a].d; }
        if (j == 0) {              // the value B_i, B_i s_i, d_a R_i s_i, d_a R_parent attach_i
            double Bv[9];
            for (int e = 0; e < 9; e++) {
                double s = d1r[e] * ddq[0] + d1r[9 + e] * ddq[1] + d1r[18 + e] * ddq[2];
                for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) s += d2r[9 * kj_pair(a, c) + e] * dq[a] * dq[c];
                Bv[e] = s; sm[KJ_B + 9 * i + e] = s;
            }
            kj_mv(Bv, K->s1[i], sm + KJ_BV + 3 * i);
            for (int a = 0; a < 3; a++) kj_mv(d1r + 9 * a, K->s1[i], sm + KJ_DRS + (i * 3 + a) * 3);
            const int p = M->parent[i];
            if (p >= 0) for (int a = 0; a < 3; a++) kj_mv(sm + KJ_D1R + p * 27 + 9 * a, M->attach[i], sm + KJ_DRA + (i * 3 + a) * 3);
        }
    }
    __syncthreads();
    JSTAMP(1);
    // ---- A_i (acceleration of the link's origin + g) and D_i (subtree sums, link order: fixed)
    if (tid < nl) {
        const int i = tid;
        double acc[3] = {sm[KJ_DDQ], sm[KJ_DDQ + 1], sm[KJ_DDQ + 2] + K->o.dyn.eom.gravity};
        double terms[CPE_MAX_CHAIN][3]; int nt = 0, j = i;
        while (M->parent[j] >= 0) { const int p = M->parent[j]; kj_mv(sm + KJ_B + 9 * p, M->attach[j], terms[nt]); nt++; j = p; }
        for (int t = nt - 1; t >= 0; t--) { acc[0] += terms[t][0]; acc[1] += terms[t][1]; acc[2] += terms[t][2]; }
        sm[KJ_AC + 3 * i] = acc[0]; sm[KJ_AC + 3 * i + 1] = acc[1]; sm[KJ_AC + 3 * i + 2] = acc[2];
        double s0 = 0.0, s1_ = 0.0, s2 = 0.0; const uint32_t mask = K->sub_mask[i];
        for (int k = 0; k < nl; k++) if ((mask >> k) & 1u) { s0 += sm[KJ_BV + 3 * k]; s1_ += sm[KJ_BV + 3 * k + 1]; s2 += sm[KJ_BV + 3 * k + 2]; }
        sm[KJ_DS + 3 * i] = s0; sm[KJ_DS + 3 * i + 1] = s1_; sm[KJ_DS + 3 * i + 2] = s2;
    }
    __syncthreads();
    JSTAMP(2);
    // ---- the three block matrices over the related link pairs: entry [a][b] = d row(i, a) / d (local b of kind ty of link k), in body weights
    const unsigned char* LB = reinterpret_cast<const unsigned char*>(sm + KJ_TL);
    // One thread per ENTRY (kind, pair, a, bb) -- 3 x 89 x 9 of the cheetah, the 801 entries of kind 0 (which carry the force terms) first: every
    // pass of the workgroup is evenly loaded, and a wave meets only the motors / joint equalities of the seven pairs its 64 entries belong to.
    const int nblk9 = 9 * K->nblk, n_ent = 3 * nblk9;
    // (the pair word of the NEXT pass is requested before this pass's arithmetic)
    unsigned wd_next = K->blk_word[tid < n_ent ? (tid % nblk9) / 9 : 0];
    for (int t = tid; t < n_ent; t += KJ_THREADS) {
        const int ty = t / nblk9, t9 = t - ty * nblk9, bl = t9 / 9, ab = t9 - 9 * bl, a = ab / 3, bb = ab - 3 * a;
        const unsigned wd = wd_next;
        { const int tn = t + KJ_THREADS; wd_next = K->blk_word[tn < n_ent ? (tn % nblk9) / 9 : 0]; }
        const int i = wd & 255u, k = (wd >> 8) & 255u, rel = (wd >> 16) & 255u, c = (int)(int8_t)(wd >> 24);
        const int j = 3 * ty + bb;
        double v;
        if (rel == 2) v = kj_dot3(sm + KJ_DRA + (c * 3 + a) * 3, sm + KJ_TBS + (k * 9 + j) * 3);            // k below i: (d_a R_i attach_c) . (dB_k s_k)
        else if (rel == 1) v = kj_dot3(sm + KJ_DRS + (i * 3 + a) * 3, sm + KJ_TBA + (c * 9 + j) * 3);       // k above i: (d_a R_i s_i) . (dB_k v_k->i)
        else {
            v = sm[KJ_SQ + (i * 3 + a) * 9 + j];
            if (ty == 0) {
                const double* d2 = sm + KJ_D2R + i * 54 + 9 * kj_pair(a, bb);
                double t3[3]; kj_mv(d2, K->s1[i], t3);
                v += kj_dot3(t3, sm + KJ_AC + 3 * i);
                const double* Bi = sm + KJ_B + 9 * i; const double* S2 = K->S2[i];
                for (int m = 0; m < 3; m++) for (int nn = 0; nn < 3; nn++) { const double bs = Bi[3 * m] * S2[nn] + Bi[3 * m + 1] * S2[3 + nn] + Bi[3 * m + 2] * S2[6 + nn]; v += d2[3 * m + nn] * bs; }
                for (int ch = 0; ch < nl; ch++) if (M->parent[ch] == i) { kj_mv(d2, M->attach[ch], t3); v += kj_dot3(t3, sm + KJ_DS + 3 * ch); }
            }
        }
        v *= iMg;
        if (ty == 0) {
            // minus d (A f) / d q: Q(i, a) = sum_m tau_m cm + sum_r lambda_r cr + sum_feet F . d foot / d q(i, a); derivative with respect to angle bb of link k.
            // The motor / constraint / foot tables are read once per item (uniform loads), the entry decides whether the item touches it.
            const double* F = sm + KJ_F;
            double g = 0.0;
            const double* Ri = sm + KJ_R + 9 * i;
            for (int qm = 0; qm < LB[bl]; qm++) {             // the motors of this pair (host list)
                const int m = LB[2 * KJ_MAXB + bl * KJ_LMAX + qm];
                const int a1 = K->o.dyn.motor_first[m], a2 = K->o.dyn.motor_second[m], ax = K->o.dyn.motor_axis[m];
                const double tau = F[m];
                if (tau == 0.0) continue;
                const double sgn = (i == a2 ? 1.0 : 0.0) - (i == a1 ? 1.0 : 0.0);
                if (sgn == 0.0) continue;
                const double* R1 = sm + KJ_R + 9 * a1;
                double ca[3], Rca[3]; kj_cvec(sm + KJ_SC + 6 * i, a, 0, 0, ca); kj_mv(Ri, ca, Rca);
                double tt = 0.0;
                if (k == i) {          // d / d angle bb of link i of (R_a1 e_ax) . (R_i c_a):  d_bb R_i c_a + R_i d_bb c_a
                    double dca[3], v1[3], v2[3] = {0.0, 0.0, 0.0};
                    kj_mv(sm + KJ_D1R + i * 27 + 9 * bb, ca, v1);
                    if (bb < 2) { kj_cvec(sm + KJ_SC + 6 * i, a, bb == 0, bb == 1, dca); kj_mv(Ri, dca, v2); }
                    tt += R1[ax] * (v1[0] + v2[0]) + R1[3 + ax] * (v1[1] + v2[1]) + R1[6 + ax] * (v1[2] + v2[2]);
                }
                if (k == a1) {         // through the motor axis R_a1 e_ax
                    const double* D1 = sm + KJ_D1R + a1 * 27 + 9 * bb;
                    tt += D1[ax] * Rca[0] + D1[3 + ax] * Rca[1] + D1[6 + ax] * Rca[2];
                }
                g += sgn * tau * tt;
            }
            for (int qc = 0; qc < LB[KJ_MAXB + bl]; qc++) {    // the joint equalities of this pair
                const int r = LB[2 * KJ_MAXB + KJ_MAXB * KJ_LMAX + bl * KJ_LMAX + qc];
                const int jn = K->con_joint[r], cc = K->con_axis[r], p = M->joint_parent[jn], ch = M->joint_child[jn];
                const double lam = F[nm + r];
                if (lam == 0.0) continue;
                const double* Rp = sm + KJ_R + 9 * p; const double* Rc = sm + KJ_R + 9 * ch;
                double tt;
                if (i == p && k == p) { const double* D2 = sm + KJ_D2R + p * 54 + 9 * kj_pair(a, bb); tt = D2[1] * Rc[cc] + D2[4] * Rc[3 + cc] + D2[7] * Rc[6 + cc]; }
                else if (i == p && k == ch) { const double* Da = sm + KJ_D1R + p * 27 + 9 * a; const double* Db = sm + KJ_D1R + ch * 27 + 9 * bb; tt = Da[1] * Db[cc] + Da[4] * Db[3 + cc] + Da[7] * Db[6 + cc]; }
                else if (i == ch && k == p) { const double* Db = sm + KJ_D1R + p * 27 + 9 * bb; const double* Da = sm + KJ_D1R + ch * 27 + 9 * a; tt = Db[1] * Da[cc] + Db[4] * Da[3 + cc] + Db[7] * Da[6 + cc]; }
                else { const double* D2 = sm + KJ_D2R + ch * 54 + 9 * kj_pair(a, bb); tt = Rp[1] * D2[cc] + Rp[4] * D2[3 + cc] + Rp[7] * D2[6 + cc]; }
                g += lam * tt;
            }
            if (i == k) for (int kf = 0; kf < nf; kf++) {
                const double* Ff = F + nm + nc + 3 * kf;
                const int l = K->o.dyn.foot_marker[kf];
                if (Ff[0] == 0.0 && Ff[1] == 0.0 && Ff[2] == 0.0) continue;
                for (int cpos = 0; cpos < M->chain_len[l]; cpos++) if (M->chain_link[l][cpos] == i) {
                    double t3[3]; kj_mv(sm + KJ_D2R + i * 54 + 9 * kj_pair(a, bb), M->chain_vec[l][cpos], t3);
                    g += Ff[1] * t3[0] + Ff[2] * t3[1] + Ff[0] * t3[2];                  // (z, x, y) . d^2 foot
                }
            }
            v -= g;
        }
        sm[(ty == 0 ? KJ_KF : (ty == 1 ? KJ_CB : KJ_MB)) + 9 * bl + 3 * a + bb] = v;
    }
    JSTAMP(3);
    // ---- the coordinate map: legs in closed form, roll of the Hooke children by implicit differentiation (parents first)
    for (int t = tid; t < 3 * M->nrev; t += KJ_THREADS) {
        const int fr = t / M->nrev, rv = t - fr * M->nrev, c = M->rev_child[rv], Bk = M->rev_body[rv];
        const double* scc = sm + KJ_SC + fr * 6 * KS_NL + 6 * c; const double* scB = sm + KJ_SC + fr * 6 * KS_NL + 6 * Bk;
        double sa, ca; sincos(E[fr * KS_NS + nq + rv], &sa, &ca);
        // M4 = [ e_y | Ry(alpha)^T Jw_B ] (3 x 4); Ry^T = [[ca, 0, -sa], [0, 1, 0], [sa, 0, ca]]
        double M4[12];
        M4[0] = 0.0; M4[4] = 1.0; M4[8] = 0.0;
        for (int jj = 0; jj < 3; jj++) { double cB[3]; kj_cvec(scB, jj, 0, 0, cB); M4[1 + jj] = ca * cB[0] - sa * cB[2]; M4[5 + jj] = cB[1]; M4[9 + jj] = sa * cB[0] + ca * cB[2]; }
        // Jw_c^-1 = [[1, sf tt, cf tt], [0, cf, -sf], [0, sf / ct, cf / ct]]
        const double sf = scc[0], cf = scc[1], stc = scc[2], ctc = scc[3], ict = ctc != 0.0 ? 1.0 / ctc : 0.0, tt = stc * ict;
        double* G = sm + KJ_GL + (fr * CPE_MAX_JOINTS + rv) * 12;
        for (int col = 0; col < 4; col++) {
            const double m0 = M4[col], m1 = M4[4 + col], m2 = M4[8 + col];
            G[col] = m0 + sf * tt * m1 + cf * tt * m2; G[4 + col] = cf * m1 - sf * m2; G[8 + col] = (sf * m1 + cf * m2) * ict;
        }
    }
    if (tid >= 192 && tid < 195) {
        const int fr = tid - 192;
        for (int hj = 0; hj < K->nh; hj++) {
            const int p = K->hk_parent[hj], c = K->hk_child[hj];
            const double* scp = sm + KJ_SC + fr * 6 * KS_NL + 6 * p; const double* scc = sm + KJ_SC + fr * 6 * KS_NL + 6 * c;
            double Rp[9], Rc[9], Dm[9];
            rot_kind(scp, 0, Rp); rot_kind(scc, 0, Rc);
            const double ay[3] = {Rp[1], Rp[4], Rp[7]}, zc[3] = {Rc[2], Rc[5], Rc[8]};
            rot_kind(scc, 1, Dm); const double gphi = ay[0] * Dm[2] + ay[1] * Dm[5] + ay[2] * Dm[8], ig = gphi != 0.0 ? -1.0 / gphi : 0.0;
            double own[2], par[3];
            for (int bb = 1; bb < 3; bb++) { rot_kind(scc, 1 + bb, Dm); own[bb - 1] = ig * (ay[0] * Dm[2] + ay[1] * Dm[5] + ay[2] * Dm[8]); }
            for (int bb = 0; bb < 3; bb++) { rot_kind(scp, 1 + bb, Dm); par[bb] = ig * (Dm[1] * zc[0] + Dm[4] * zc[1] + Dm[7] * zc[2]); }
            double* row = sm + KJ_GP + (fr * KJ_NH + hj) * CPE_NX;
            for (int k = 0; k < nu; k++) {
                double v = 0.0;
                if (M->u_of_q[3 + 3 * c + 1] == k) v += own[0];
                if (M->u_of_q[3 + 3 * c + 2] == k) v += own[1];
                for (int bb = 0; bb < 3; bb++) {
                    const int pq = 3 + 3 * p + bb;
                    if (M->u_of_q[pq] == k) v += par[bb];
                    else if (bb == 0 && K->hooke_of_link[p] >= 0) v += par[0] * sm[KJ_GP + (fr * KJ_NH + K->hooke_of_link[p]) * CPE_NX + k];      // the parent's roll is itself dependent
                }
                row[k] = v;
            }
        }
    }
    __syncthreads();
    JSTAMP(4);
    // ---- columns: wave w evaluates column a = fr * nu + k; lanes = rows
    double* Jg = Jbuf + f_ * (size_t)KIN_JSTRIDE;
    double* TL = sm + KJ_TL + wave * KS_NL * 12;
    double* TT = sm + KJ_TT + wave * 12;
    const double c2 = ih2;
    // Every lane owns the same rows in every column: row `lane` of the equations of motion (lane < nq) and the marker-type rows nq + lane and
    // nq + 64 + lane (foot heights, foot velocities, second differences).  What those rows need from the model tables -- the block indices of the
    // link pairs, the marker's chain of links and body-frame vectors -- is read ONCE into registers: the column loop below touches LDS only.
    int e_i = -1, e_a = 0, eblk[KS_NL];
#pragma unroll
    for (int kk = 0; kk < KS_NL; kk++) eblk[kk] = -1;
    if (lane >= 3 && lane < nq) {
        e_i = (lane - 3) / 3; e_a = (lane - 3) - 3 * e_i;
#pragma unroll
        for (int kk = 0; kk < KS_NL; kk++) eblk[kk] = kk < nl ? (int)K->blk[e_i][kk] : -1;
    }
    int mkind[2], md[2], mnch[2], mlink[2][KJ_CHAIN];          // kind 0 none, 2 foot height, 3 foot velocity, 4 second difference
    double mvec[2][KJ_CHAIN][3];
#pragma unroll
    for (int pz = 0; pz < 2; pz++) {
        const int r = nq + lane + 64 * pz;
        int l = 0; mkind[pz] = 0; md[pz] = 0; mnch[pz] = 0;
        if (r < nq + nf) { mkind[pz] = 2; l = K->o.dyn.foot_marker[r - nq]; md[pz] = 2; }
        else if (r < nq + 4 * nf) { const int kf = (r - nq - nf) / 3; mkind[pz] = 3; md[pz] = (r - nq - nf) - 3 * kf; l = K->o.dyn.foot_marker[kf]; }
        else if (r < nrow) { const int t = r - nq - 4 * nf; mkind[pz] = 4; l = t / 3; md[pz] = t - 3 * l; }
        if (mkind[pz]) mnch[pz] = M->chain_len[l];
#pragma unroll
        for (int cpos = 0; cpos < KJ_CHAIN; cpos++) {
            const bool on = mkind[pz] != 0 && cpos < mnch[pz];
            mlink[pz][cpos] = on ? M->chain_link[l][cpos] : 0;
            mvec[pz][cpos][0] = on ? M->chain_vec[l][cpos][0] : 0.0; mvec[pz][cpos][1] = on ? M->chain_vec[l][cpos][1] : 0.0; mvec[pz][cpos][2] = on ? M->chain_vec[l][cpos][2] : 0.0;
        }
    }
    const double mtot = K->mtot;
    // the same for the direction of a column: which reduced coordinates the three angles of link `lane` are, the leg / tail the link is, and per
    // reduced coordinate whether it is a leg angle / a base translation (bit masks) -- the column loop read these ~10 words from the model tables in
    // global memory per column, two of them behind another
    int c_uq0 = -1, c_uq1 = -1, c_uq2 = -1, c_rv = -1, c_ru = -1, c_rb0 = -1, c_rb1 = -1, c_rb2 = -1, c_hj = -1;
    if (lane < nl) {
        c_uq0 = M->u_of_q[3 + 3 * lane]; c_uq1 = M->u_of_q[3 + 3 * lane + 1]; c_uq2 = M->u_of_q[3 + 3 * lane + 2];
        c_rv = K->leg_of_link[lane]; c_hj = K->hooke_of_link[lane];
        if (c_rv >= 0) { c_ru = M->rev_u[c_rv]; c_rb0 = M->rev_body_u[c_rv][0]; c_rb1 = M->rev_body_u[c_rv][1]; c_rb2 = M->rev_body_u[c_rv][2]; }
    }
    const unsigned long long rev_mask = __ballot(lane < nu && M->rev_of_u[lane < nu ? lane : 0] >= 0);
    const unsigned long long trans_mask = __ballot(lane < 3 && M->rev_of_u[lane < 3 ? lane : 0] < 0 && M->u_of_q[lane < 3 ? lane : 0] == lane);
    JSTAMP(5);
    // Columns are handed out through a counter in LDS, the expensive ones first: the columns of the six trunk angles that carry legs (base, bodyF: reduced
    // coordinates 3 .. 8) touch seven links, the others one or none -- dealt round-robin, two waves got twice as many of those as the other two.
    // Every column is computed by one wave from the same inputs whoever takes it: the result does not depend on the order.
    int* s_next_col = reinterpret_cast<int*>(sm + KJ_TT + 9);        // (a pad word of the translation scratch: the kernel's LDS is full to the last 192 bytes)
    if (tid == 0) *s_next_col = 0;
    __syncthreads();
    for (;;) {
        int ticket = 0;
        if (lane == 0) ticket = atomicAdd(s_next_col, 1);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
        if (ticket >= KIN_NC3) break;
        const int kk_ = ticket / 3, fr = ticket - 3 * kk_;
        const int k = kk_ < 6 ? 3 + kk_ : (kk_ < 9 ? kk_ - 6 : kk_);
        const int col = fr * nu + k;
        // (1) the direction: per link raw = Gamma_fr[:, k] rows of the link; d a1, d a2 through the blocks; d q0, d q', d q''
        unsigned long long touched = 0ull;
        if (lane < nl) {
            const int i = lane;
            double r0 = 0.0, r1 = 0.0, r2 = 0.0;                       // raw = rows of Gamma_fr[:, k] that belong to link i
            if (!((rev_mask >> k) & 1ull)) {
                if (c_uq0 == k) r0 = 1.0;
                if (c_uq1 == k) r1 = 1.0;
                if (c_uq2 == k) r2 = 1.0;
            }
            const int rv = c_rv;
            if (rv >= 0) {
                const double* G = sm + KJ_GL + (fr * CPE_MAX_JOINTS + rv) * 12;
                int colg = -1;
                if (c_ru == k) colg = 0;
                if (c_rb0 == k) colg = 1;
                if (c_rb1 == k) colg = 2;
                if (c_rb2 == k) colg = 3;
                if (colg >= 0) { r0 = G[colg]; r1 = G[4 + colg]; r2 = G[8 + colg]; }
            }
            const int hj = c_hj;
            if (hj >= 0) r0 = sm[KJ_GP + (fr * KJ_NH + hj) * CPE_NX + k];
            const double* nb = sm + KJ_NB + i * 36;
            // d a1 = (fr == 0 ? P1 : fr == 1 ? S1 : 0) raw ; d a2 = (fr == 2 ? S2 raw : P2 d a1) ; d q0 = (fr == 0 ? raw : 0)
            const double* M1 = fr == 0 ? nb + 9 : nb;
            const double f1 = fr <= 1 ? 1.0 : 0.0, f0 = fr == 0 ? 1.0 : 0.0;
            const double a10 = f1 * (M1[0] * r0 + M1[1] * r1 + M1[2] * r2), a11 = f1 * (M1[3] * r0 + M1[4] * r1 + M1[5] * r2), a12 = f1 * (M1[6] * r0 + M1[7] * r1 + M1[8] * r2);
            const double* M2 = fr == 2 ? nb + 18 : nb + 27;
            const double x0 = fr == 2 ? r0 : a10, x1 = fr == 2 ? r1 : a11, x2 = fr == 2 ? r2 : a12;
            const double a20 = M2[0] * x0 + M2[1] * x1 + M2[2] * x2, a21 = M2[3] * x0 + M2[4] * x1 + M2[5] * x2, a22 = M2[6] * x0 + M2[7] * x1 + M2[8] * x2;
            double* o = TL + i * 12;
            o[0] = r0; o[1] = r1; o[2] = r2;
            o[3] = f0 * r0; o[4] = f0 * r1; o[5] = f0 * r2;
            o[6] = (f0 * r0 - a10) * ih; o[7] = (f0 * r1 - a11) * ih; o[8] = (f0 * r2 - a12) * ih;
            o[9] = (f0 * r0 - 2.0 * a10 + a20) * ih2; o[10] = (f0 * r1 - 2.0 * a11 + a21) * ih2; o[11] = (f0 * r2 - 2.0 * a12 + a22) * ih2;
            const bool any = r0 != 0.0 || r1 != 0.0 || r2 != 0.0;
            touched = __ballot(any);
        } else touched = __ballot(false);
        if (lane == 0) {
            for (int d = 0; d < 3; d++) {
                const double r0 = (fr == 0 && k == d) ? 1.0 : 0.0, r1 = (fr == 1 && k == d) ? 1.0 : 0.0, r2 = (fr == 2 && k == d) ? 1.0 : 0.0;
                TT[d] = r0 + r1 + r2;                                   // raw displacement of the base position of frame fr
                TT[3 + d] = (r0 - r1) * ih; TT[6 + d] = (r0 - 2.0 * r1 + r2) * ih2;
            }
        }
        touched = __builtin_amdgcn_readfirstlane((unsigned)(touched & 0xffffffffull)) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(touched >> 32)) << 32);
        wave_lds_sync();
        const bool trans = (trans_mask >> k) & 1ull;                                         // a base translation coordinate
        // (2) rows of the equations of motion: lane = row
        if (lane < nq) {
            double v = 0.0;
            if (lane < 3) {
                for (int kk = 0; kk < nl; kk++) if ((touched >> kk) & 1ull) {
                    const double* o = TL + kk * 12; const double* tb = sm + KJ_TBS + kk * 27;
                    if (fr == 0) for (int bb = 0; bb < 3; bb++) v += tb[3 * bb + lane] * o[3 + bb];                 // d q0 is zero for the columns of frames n-1, n-2
                    for (int bb = 0; bb < 3; bb++) v += tb[3 * (3 + bb) + lane] * o[6 + bb] + tb[3 * (6 + bb) + lane] * o[9 + bb];
                }
                v = (v + mtot * TT[6 + lane]) * iMg;
            } else {
#pragma unroll
                for (int kk = 0; kk < KS_NL; kk++) {
                    const int bl = eblk[kk];
                    if (bl < 0 || !((touched >> kk) & 1ull)) continue;
                    const double* o = TL + kk * 12;
                    const double* kf = sm + KJ_KF + 9 * bl + 3 * e_a; const double* cb = sm + KJ_CB + 9 * bl + 3 * e_a; const double* mb = sm + KJ_MB + 9 * bl + 3 * e_a;
                    if (fr == 0) v += kf[0] * o[3] + kf[1] * o[4] + kf[2] * o[5];
                    v += cb[0] * o[6] + cb[1] * o[7] + cb[2] * o[8] + mb[0] * o[9] + mb[1] * o[10] + mb[2] * o[11];
                }
                if (trans) { const double* ds = sm + KJ_DRS + (e_i * 3 + e_a) * 3; v += (ds[0] * TT[6] + ds[1] * TT[7] + ds[2] * TT[8]) * iMg; }
            }
            Jg[(size_t)col * KIN_ROWS_MAX + lane] = v;
        }
        // (3) marker-type rows nq + lane and nq + 64 + lane
#pragma unroll
        for (int pz = 0; pz < 2; pz++) {
            const int kind = mkind[pz], d = md[pz];
            if (kind == 0) continue;
            double v = 0.0;
            if (kind == 2) {                      // foot height: z of the foot point of frame n
                if (fr == 0) {
                    v = TT[2];
#pragma unroll
                    for (int cpos = 0; cpos < KJ_CHAIN; cpos++) { const int kk = mlink[pz][cpos]; if (cpos >= mnch[pz] || !((touched >> kk) & 1ull)) continue;
                        const double* o = TL + kk * 12;
                        for (int bb = 0; bb < 3; bb++) { const double* D = sm + KJ_D1R + kk * 27 + 9 * bb; v += (D[6] * mvec[pz][cpos][0] + D[7] * mvec[pz][cpos][1] + D[8] * mvec[pz][cpos][2]) * o[bb]; } }
                }
            } else if (kind == 3) {               // foot velocity (d foot / d q)(q0) q', component d
                v = TT[3 + d];
#pragma unroll
                for (int cpos = 0; cpos < KJ_CHAIN; cpos++) { const int kk = mlink[pz][cpos]; if (cpos >= mnch[pz] || !((touched >> kk) & 1ull)) continue;
                    const double* o = TL + kk * 12; const double* dqk = sm + KJ_DQ + 3 + 3 * kk;
                    for (int bb = 0; bb < 3; bb++) {
                        const double* D = sm + KJ_D1R + kk * 27 + 9 * bb;
                        v += (D[3 * d] * mvec[pz][cpos][0] + D[3 * d + 1] * mvec[pz][cpos][1] + D[3 * d + 2] * mvec[pz][cpos][2]) * o[6 + bb];                  // J d q'
                        if (fr == 0) for (int a = 0; a < 3; a++) { const double* D2 = sm + KJ_D2R + kk * 54 + 9 * kj_pair(a, bb);
                            v += (D2[3 * d] * mvec[pz][cpos][0] + D2[3 * d + 1] * mvec[pz][cpos][1] + D2[3 * d + 2] * mvec[pz][cpos][2]) * o[3 + a] * dqk[bb]; }      // (d J / d q0) q'
                    } }
            } else {                              // second difference of a marker, component d: positions use the RAW angles of their own frame
                double s_ = TT[d];
#pragma unroll
                for (int cpos = 0; cpos < KJ_CHAIN; cpos++) { const int kk = mlink[pz][cpos]; if (cpos >= mnch[pz] || !((touched >> kk) & 1ull)) continue;
                    const double* o = TL + kk * 12;
                    for (int bb = 0; bb < 3; bb++) { const double* D = sm + KJ_D1R + (fr * KS_NL + kk) * 27 + 9 * bb; s_ += (D[3 * d] * mvec[pz][cpos][0] + D[3 * d + 1] * mvec[pz][cpos][1] + D[3 * d + 2] * mvec[pz][cpos][2]) * o[bb]; } }
                v = c2 * (fr == 1 ? -2.0 : 1.0) * s_;
            }
            Jg[(size_t)col * KIN_ROWS_MAX + nq + lane + 64 * pz] = v;
        }
        wave_lds_sync();
    }
    JSTAMP(6);
}
