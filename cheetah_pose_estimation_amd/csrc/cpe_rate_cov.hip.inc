// cpe_rate_cov.hip.inc -- posterior covariance of the rates (include/cpe.h, cpe_rate_covariance; DESIGN.md 2 "What is propagated").
// A rate is a fixed linear stencil over at most three consecutive frames, rate = sum_i c_i u_{f_i}, so its covariance is
//     sum_i sum_j c_i c_j Sigma(f_i, f_j),
// every block inside the band cpe_band_inverse writes (cov_diag, cov_off: band_entry).  A point p(u) -- a marker, the
// centre of mass -- moves by P = d p / d u to first order: cov p = P Sigma(n,n) P^T, and the velocity (p(u_n) - p(u_{n-1})) / h has
//     (P_n S_nn P_n^T + P_{n-1} S_{n-1,n-1} P_{n-1}^T - P_n S_{n,n-1} P_{n-1}^T - (that)^T) / h^2.
// Two kernels, one wave per frame: k_point_jac (P of every marker and of the centre of mass, dense) and k_rate_cov (the five covariances).
// No atomics; every sum has a fixed order; every block is computed on its lower triangle and mirrored.

// LDS of k_point_jac in doubles, sized by the table limits (cpe.h, cpe_model.h) so that one size serves every model of a handle:
// state | sin / cos | leg sin / cos | trunk R, dR | dynamic vectors | S rows | Dp | first term of every item (int)
#define PJ_ITEMS (CPE_MAX_MARKERS * CPE_MAX_MCOL)
#define PJ_LDS_DOUBLES (CPE_MAX_NQ + CPE_MAX_JOINTS + 6 * CPE_MAX_LINKS + 2 * CPE_MAX_JOINTS + 36 * CPE_MAX_LINKS + 3 * CPE_MAX_SDYN + \
                        CPE_MAX_SCOL * CPE_MAX_DEP + 3 * PJ_ITEMS + PJ_ITEMS / 2)

// ---- Jacobians, one wave per frame.  M: the handle's models; Mc: the same skeletons with the link centres as markers (marker i = centre of mass
// of link i).  State: buffer 0 of the workspace as k_state_init wrote it.  jac_pos [F][L][3][28] and jac_com [F][3][28] arrive zeroed: only the
// columns a point depends on are written.  jac_com = sum_i m_i Dp_i / M, column by column, in link order (k_fk's centre of mass).
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_point_jac(const DevModel* __restrict__ M, const DevModel* __restrict__ Mc, int N,
                                                    const double* __restrict__ qbuf, double* __restrict__ jac_pos, double* __restrict__ jac_com,
                                                    RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs)) return;
    M += fs.model; Mc += fs.model;
    const size_t f = (size_t)fs.b * N + fs.n;
    const int nq = M->nq, nl = M->nl, L = M->L, nrev = M->nrev, ns = M->ns;
    double* sq = smem;
    double* sal = sq + nq;
    double* ssc = sq + (CPE_MAX_NQ + CPE_MAX_JOINTS);
    double* ssa = ssc + 6 * CPE_MAX_LINKS;
    double* sR = ssa + 2 * CPE_MAX_JOINTS;
    double* sdyn = sR + 36 * CPE_MAX_LINKS;
    double* sSv = sdyn + 3 * CPE_MAX_SDYN;
    double* sDp = sSv + CPE_MAX_SCOL * CPE_MAX_DEP;
    int* sBeg = reinterpret_cast<int*>(sDp + 3 * PJ_ITEMS);

    const int4 fw = *reinterpret_cast<const int4*>(M->fn_lane[lane]);
    const int hj_n = M->hj_n, hk_n = M->hk_n;
    const int2 hkw = *reinterpret_cast<const int2*>(M->hk_w[lane]);
    const double* stf = qbuf + f * ns;
    for (int t = lane; t < ns; t += WAVE) sq[t] = stf[t];
    wave_lds_sync();
    // ---- the state phases (cpe_kernels.hip), as k_marker_cov runs them; they read the joints only, which M and Mc share
    wave_state_sincos(M, sq, sal, ssc, ssa, nrev, lane);
    wave_lds_sync();
    wave_tail_roll(sq, ssc, hj_n, fw.x, lane);
    wave_trunk_rotations(M, ssc, sR, fw.y, lane);
    wave_lds_sync();
    wave_hooke_srows(sR, sSv, hk_n, hkw, lane);
    if (jac_pos) {
        wave_point_columns(M, ssa, sR, sSv, sdyn, sDp, sBeg, lane);
        double* o = jac_pos + f * (size_t)(L * 3 * NU);
        for (int t = lane; t < M->mc_total; t += WAVE) {
            const int l = M->mc_marker[t], col = M->mcol[l][M->mc_j[t]];
#pragma unroll
            for (int a = 0; a < 3; a++) o[(l * 3 + a) * NU + col] = sDp[3 * t + a];
        }
        wave_lds_sync();        // sdyn, sDp and sBeg are rewritten below
    }
    if (jac_com) {
        wave_point_columns(Mc, ssa, sR, sSv, sdyn, sDp, sBeg, lane);
        const double im = Mc->inv_total_mass;
        for (int t = lane; t < 3 * NU; t += WAVE) {
            const int a = t / NU, col = t - a * NU;
            double s = 0.0;
            for (int i = 0; i < nl; i++) {
                const int nc = Mc->mcol_n[i], off = Mc->mcol_off[i];
                for (int j = 0; j < nc; j++)
                    if (Mc->mcol[i][j] == col) s = fma(Mc->mass[i], sDp[3 * (off + j) + a], s);
            }
            jac_com[f * (size_t)(3 * NU) + t] = s * im;
        }
    }
}

// ---- stencils.  velocity row n of a sequence of NL frames: (u_n - u_{n-1}) / h; row 0 repeats k_finalize's gauge, (-2 u_0 + 3 u_1 - u_2) / h
// (NL >= 3), (u_1 - u_0) / h (NL == 2), nothing (NL == 1).  acceleration row n: (u_m - 2 u_{m-1} + u_{m-2}) / h^2 at m = max(n, 2), nothing
// for NL < 3.  The m frames are consecutive, f0 .. f0 + m - 1; a coefficient is k / h or k / (h h) with k a small integer.
struct RateStencil { int m; int f0; double c[3]; };
__device__ __forceinline__ RateStencil velocity_stencil(int NL, int n, double h) {
    RateStencil s;
    s.m = 0; s.f0 = 0; s.c[0] = s.c[1] = s.c[2] = 0.0;
    if (n >= 1) { s.m = 2; s.f0 = n - 1; s.c[0] = -1.0 / h; s.c[1] = 1.0 / h; }
    else if (NL >= 3) { s.m = 3; s.c[0] = -2.0 / h; s.c[1] = 3.0 / h; s.c[2] = -1.0 / h; }
    else if (NL == 2) { s.m = 2; s.c[0] = -1.0 / h; s.c[1] = 1.0 / h; }
    return s;
}
__device__ __forceinline__ RateStencil acceleration_stencil(int NL, int n, double h) {
    RateStencil s;
    s.m = 0; s.f0 = 0; s.c[0] = s.c[1] = s.c[2] = 0.0;
    if (NL >= 3) {
        const double h2 = h * h;
        s.m = 3; s.f0 = (n > 2 ? n : 2) - 2; s.c[0] = 1.0 / h2; s.c[1] = -2.0 / h2; s.c[2] = 1.0 / h2;
    }
    return s;
}

// out [28][28] = sum_i sum_j (c_i c_j) Sigma(f_i, f_j), i outer, j inner, straight from the band in HBM (band_entry; every entry is read once or
// twice).  Lower triangle, mirrored.
__device__ __forceinline__ void wave_stencil_cov(const RateStencil& s, const double* __restrict__ cd, const double* __restrict__ co, int pb,
                                                 double* __restrict__ out, int lane) {
    constexpr int BB = NU * NU;
    for (int e = lane; e < BB; e += WAVE) {
        const int a = e / NU, c = e - a * NU;
        if (c > a) continue;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)                          // (constant trip counts: the stencil stays in registers)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                if (i >= s.m || j >= s.m) continue;
                acc = fma(s.c[i] * s.c[j], band_entry(cd, co, pb, s.f0 + i, s.f0 + j, a, c), acc);
            }
        out[a * NU + c] = acc; out[c * NU + a] = acc;
    }
}

// x^T S y over the listed columns: sum_i x[ci] (sum_j S[ci][cj] y[cj]); cols == nullptr: all 28
__device__ __forceinline__ double quad_form(const double* S, const double* x, const double* y, const int32_t* __restrict__ cols, int nc) {
    double s = 0.0;
    for (int i = 0; i < nc; i++) {
        const int ci = cols ? cols[i] : i;
        double w = 0.0;
        for (int j = 0; j < nc; j++) { const int cj = cols ? cols[j] : j; w = fma(S[ci * NU + cj], y[cj], w); }
        s = fma(x[ci], w, s);
    }
    return s;
}

// ---- the five covariances of frame n, one wave per frame.  cov_diag, cov_off: the band (layout of cpe_band_inverse, half-bandwidth pb >= 2);
// jp [F][L][3][28], jc [F][3][28]: k_point_jac's Jacobians.  Every output may be null and arrives zeroed; what is defined as zero is not written.
// dynamic LDS: Sigma(n,n) | Sigma(n-1,n-1) | Sigma(n,n-1) | P_n | P_{n-1} | Pc_n | Pc_{n-1}   (3 * 784 + 2 * 84 L + 2 * 84 doubles)
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_rate_cov(const DevModel* __restrict__ M, int N, int pb, const double* __restrict__ cov_diag,
                                                   const double* __restrict__ cov_off, const double* __restrict__ jp, const double* __restrict__ jc,
                                                   double* __restrict__ cov_du, double* __restrict__ cov_ddu, double* __restrict__ cov_vel,
                                                   double* __restrict__ cov_com, double* __restrict__ cov_com_vel, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    constexpr int BB = NU * NU, PW = 3 * NU;
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs)) return;
    M += fs.model;
    const int n = fs.n, NL = fs.len, L = M->L;
    const double h = M->h;
    const size_t f0 = (size_t)fs.b * N, f = f0 + n;
    const double* cd = cov_diag + f0 * BB;
    const double* co = cov_off + f0 * (size_t)pb * BB;
    if (cov_du) wave_stencil_cov(velocity_stencil(NL, n, h), cd, co, pb, cov_du + f * BB, lane);
    if (cov_ddu) wave_stencil_cov(acceleration_stencil(NL, n, h), cd, co, pb, cov_ddu + f * BB, lane);
    if (!cov_vel && !cov_com && !cov_com_vel) return;          // uniform

    double* sA = smem;                 // Sigma(n,n)
    double* sB = sA + BB;              // Sigma(n-1,n-1)
    double* sX = sB + BB;              // Sigma(n,n-1)
    double* sP = sX + BB;              // P_n
    double* sQ = sP + PW * L;          // P_{n-1}
    double* sPc = sQ + PW * L;         // Pc_n
    double* sQc = sPc + PW;            // Pc_{n-1}
    const bool vel = n >= 1;           // uniform
    for (int t = lane; t < BB; t += WAVE) {
        const int r = t / NU, c = t - r * NU;
        sA[t] = band_entry(cd, co, pb, n, n, r, c);
        if (vel) { sB[t] = band_entry(cd, co, pb, n - 1, n - 1, r, c); sX[t] = band_entry(cd, co, pb, n, n - 1, r, c); }
    }
    if (cov_vel && vel)
        for (int t = lane; t < PW * L; t += WAVE) { sP[t] = jp[f * (size_t)(PW * L) + t]; sQ[t] = jp[(f - 1) * (size_t)(PW * L) + t]; }
    if (cov_com || cov_com_vel)
        for (int t = lane; t < PW; t += WAVE) { sPc[t] = jc[f * PW + t]; if (vel) sQc[t] = jc[(f - 1) * PW + t]; }
    wave_lds_sync();
    const double h2 = h * h;
    // lane = (point, entry of the lower triangle); the mirror is stored with it
    if (cov_vel && vel)
        for (int t = lane; t < 6 * L; t += WAVE) {
            const int l = t / 6;
            int a, c; lower_entry3(t - 6 * l, a, c);
            const int32_t* cols = M->mcol[l];
            const int nc = M->mcol_n[l];
            const double *Pa = sP + (l * 3 + a) * NU, *Pc = sP + (l * 3 + c) * NU, *Qa = sQ + (l * 3 + a) * NU, *Qc = sQ + (l * 3 + c) * NU;
            const double t1 = quad_form(sA, Pa, Pc, cols, nc), t2 = quad_form(sB, Qa, Qc, cols, nc);
            const double t3 = quad_form(sX, Pa, Qc, cols, nc), t4 = quad_form(sX, Pc, Qa, cols, nc);
            const double v = (t1 + t2 - t3 - t4) / h2;
            double* o = cov_vel + (f * (size_t)L + l) * 9;
            o[3 * a + c] = v; o[3 * c + a] = v;
        }
    if (lane < 6) {
        int a, c; lower_entry3(lane, a, c);
        const double *Pa = sPc + a * NU, *Pc = sPc + c * NU, *Qa = sQc + a * NU, *Qc = sQc + c * NU;
        if (cov_com || (cov_com_vel && vel)) {
            const double t1 = quad_form(sA, Pa, Pc, nullptr, NU);
            if (cov_com) { cov_com[f * 9 + 3 * a + c] = t1; cov_com[f * 9 + 3 * c + a] = t1; }
            if (cov_com_vel && vel) {
                const double t2 = quad_form(sB, Qa, Qc, nullptr, NU);
                const double t3 = quad_form(sX, Pa, Qc, nullptr, NU), t4 = quad_form(sX, Pc, Qa, nullptr, NU);
                const double v = (t1 + t2 - t3 - t4) / h2;
                cov_com_vel[f * 9 + 3 * a + c] = v; cov_com_vel[f * 9 + 3 * c + a] = v;
            }
        }
    }
}
