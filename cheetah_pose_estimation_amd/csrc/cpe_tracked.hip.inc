// cpe_tracked.hip.inc -- the 3D kinematic cost of the physics-based solve (included by cpe_kernels.hip after the solver and covariance kernels).
//
// estimate_kinetics(use_2d_reprojections=False) (acinoset_opt.py:908-913, acinoset_misc.py:531-590) replaces the reprojection cost by
//     T_n = sum_{p in x} w_p (x_p(u_n) - x*_{n,p})^2
// over the 28 relative angles x on the cost view (leg pitch = theta_B + alpha, DESIGN.md 2).  x = X u with a constant X of the model, so the
// gradient 2 X^T W (x - x*) and the block 2 X^T W X are exact and the block is a constant of (model, weights): DevTrack.  DESIGN.md 2b.
// The full-weight form (cpe_solve_kinetic_tracked_weighted*) tracks frame n with its own symmetric 28 x 28 matrix,
//     T_n = (x_n - x*_n)^T W_n (x_n - x*_n),
// W_n = (scale / 2) (X Sigma_nn X^T)^-1 from the kinematic posterior (k_track_precision), block 2 X^T W_n X once per solve (k_track_block).

// per model: weights, X^T and 2 X^T W X (built by the host, cpe_api.hip build_track)
struct DevTrack {
    double w[CPE_NX];
    double Xt[CPE_NX][CPE_NX];          // Xt[j][k] = d x_k / d u_j
    double H[CPE_NX * CPE_NX];          // 2 X^T diag(w) X, row-major
};

// the full-weight form's per-frame arrays: W [F][28][28] (the caller's) and the blocks 2 X^T W X [F][28 * 28] (k_track_block); null in the plain form
struct TrackFull { const double* W; const double* H; };

// W_n = (scale / 2) (X Sigma_nn X^T)^-1 of every frame from the u-space blocks cov_diag [F][28][28] of cpe_covariance: C = X Sigma X^T (lower
// triangle), its Cholesky factor in place, T = L^-1 and T^T T by the helpers of k_cov_prep (bit-symmetric).  A block without a factor -- a pivot
// that is not positive and finite -- gives W = 0 and bad[f] = 1 (else 0).  One wave per frame, every sum in a fixed order, no atomics; RAGGED:
// padding frames leave at once.
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_track_precision(const DevTrack* __restrict__ T, const double* __restrict__ cov_diag, double scale,
                                                         double* __restrict__ W, int* __restrict__ bad, int NS, RaggedArgs rg = RaggedArgs{}) {
    constexpr int BB = NU * NU;
    __shared__ double sA[BB];            // Sigma, then C and its factor
    __shared__ double sY[BB];            // Sigma X^T, then T
    __shared__ double sr[NU];
    __shared__ int sbad;
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(NS, nullptr, nullptr, rg, fs)) return;
    T += fs.model;
    const size_t f = blockIdx.x;
    const double* Sg = cov_diag + f * BB;
    double* Wo = W + f * BB;
    for (int t = lane; t < BB; t += WAVE) sA[t] = Sg[t];
    if (lane == 0) sbad = 0;
    wave_lds_sync();
    // Y[a][j] = sum_b Sigma[a][b] X[j][b]
    for (int t = lane; t < BB; t += WAVE) {
        const int a = t / NU, j = t - a * NU;
        double s = 0.0;
        for (int b = 0; b < NU; b++) s = fma(sA[a * NU + b], T->Xt[b][j], s);
        sY[t] = s;
    }
    wave_lds_sync();
    // C[i][j] = sum_a X[i][a] Y[a][j], j <= i (the upper triangle is never read)
    for (int t = lane; t < BB; t += WAVE) {
        const int i = t / NU, j = t - i * NU;
        if (j > i) continue;
        double s = 0.0;
        for (int a = 0; a < NU; a++) s = fma(T->Xt[a][i], sY[a * NU + j], s);
        sA[t] = s;
    }
    wave_lds_sync();
    // Cholesky, right-looking, in place: column k scaled by 1 / L[k][k], then the trailing lower triangle updated
    for (int k = 0; k < NU; k++) {
        const double d = sA[k * NU + k];
        if (!(d > 0.0) || isinf(d)) { if (lane == 0) sbad = 1; break; }        // uniform
        const double l = sqrt(d), il = 1.0 / l;
        wave_lds_sync();                                     // every lane has read the pivot
        if (lane == 0) { sA[k * NU + k] = l; sr[k] = il; }
        if (lane > k && lane < NU) sA[lane * NU + k] *= il;
        wave_lds_sync();
        const int m = NU - 1 - k;                            // trailing rows k+1 .. 27
        for (int e = lane; e < m * m; e += WAVE) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) sA[i * NU + j] = fma(-sA[i * NU + k], sA[j * NU + k], sA[i * NU + j]);
        }
        wave_lds_sync();
    }
    wave_lds_sync();
    if (sbad) {                                              // uniform
        for (int t = lane; t < BB; t += WAVE) Wo[t] = 0.0;
        if (lane == 0) bad[f] = 1;
        return;
    }
    if (lane == 0) bad[f] = 0;
    double t[NU];
    wave_tri_inverse(sA, sr, sY, t, lane);
    if (lane < 2 * NU) wave_ttt<true>(sY, t, Wo, 0.5 * scale, lane);
}

// H_n = 2 X^T W_n X of every frame, [F][28 * 28] row-major, from W [F][28][28]: the lower triangle is computed and mirrored, so the block is
// exactly symmetric.  Once per solve (the block is a constant of it); one wave per frame, fixed order, no atomics.
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_track_block(const DevTrack* __restrict__ T, const double* __restrict__ W, double* __restrict__ H, int NS,
                                                     RaggedArgs rg = RaggedArgs{}) {
    constexpr int BB = NU * NU;
    __shared__ double sW[BB];
    __shared__ double sY[BB];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(NS, nullptr, nullptr, rg, fs)) return;
    T += fs.model;
    const size_t f = blockIdx.x;
    for (int t = lane; t < BB; t += WAVE) sW[t] = W[f * BB + t];
    wave_lds_sync();
    // Y[p][j] = sum_q W[p][q] X[q][j]
    for (int t = lane; t < BB; t += WAVE) {
        const int p = t / NU, j = t - p * NU;
        double s = 0.0;
        for (int q = 0; q < NU; q++) s = fma(sW[p * NU + q], T->Xt[j][q], s);
        sY[t] = s;
    }
    wave_lds_sync();
    double* Ho = H + f * BB;
    for (int t = lane; t < BB; t += WAVE) {
        const int i = t / NU, j = t - i * NU;
        if (j > i) continue;
        double s = 0.0;
        for (int p = 0; p < NU; p++) s = fma(T->Xt[i][p], sY[p * NU + j], s);
        Ho[i * NU + j] = 2.0 * s; Ho[j * NU + i] = 2.0 * s;
    }
}

// x* of every frame from an Euler target q [F][nq]: the state (q, alpha = leg_alpha) of k_state_init, then the relative angles on the cost view.  One wave per frame; RAGGED: padding frames leave at once (nothing reads them).
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_track_target(const DevModel* __restrict__ M, const double* __restrict__ q, double* __restrict__ xt,
                                                      RaggedArgs rg = RaggedArgs{}) {
    __shared__ double ss[CPE_MAX_NQ + LM_MAX_REV];
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    FrameSlot s;
    if (!frame_slot_flat<RAGGED>(rg, s)) return;
    M += s.model;
    const int nq = M->nq;
    if (lane < nq) ss[lane] = q[f * nq + lane];
    if (lane < M->nrev) ss[nq + lane] = leg_alpha(q + f * nq + 3 + 3 * M->rev_body[lane], q + f * nq + 3 + 3 * M->rev_child[lane]);
    wave_lds_sync();
    if (lane < M->nu) {
        const int r = M->rel_ref_u[lane];
        xt[f * CPE_NX + lane] = M->rel_sign_u[lane] * (cost_coord(M, ss, lane) - (r >= 0 ? cost_coord(M, ss, r) : 0.0));
    }
}

// Per-frame normal equations of the tracked cost: k_frame_normal without its camera phase (no meas / weight read, no projection, no camera LDS).
// Kept: the state made consistent with the joint equalities (tails' roll, legs' Euler angles: the physics terms read them), Gamma, the
// angle-bound AL terms and the pose prior (GMM).  Added: T_n to g, to the diagonal block and to cost slot 0.  One wave per frame.
// dynamic LDS (doubles): q | al [ns] | sc[6 nl] | sa[2 nrev] | R[36 n_trunk] | gam[4 nrev] | res[nu] | H[nu nu] | g[nu] | GMM scratch
// FULLW: the full-weight form -- r = 2 W_n d with W_n read row by row from global memory (W_n is symmetric: lane p sums W[k][p] d[k] over the
// rows k, so every load is contiguous across the lanes), T_n = d . r / 2, the block from tw.H; the LDS is the plain form's.
template <bool GMM, bool RAGGED = false, bool FULLW = false>
__global__ __launch_bounds__(WAVE) void k_frame_tracked(const DevModel* __restrict__ M, const DevTrack* __restrict__ T, const SeqState* __restrict__ st,
                                                        int N, int which, size_t n_frames, double* __restrict__ qbuf, const double* __restrict__ xt,
                                                        double* __restrict__ gbuf, double* __restrict__ Bbuf, double* __restrict__ costbuf,
                                                        double* __restrict__ mu, double* __restrict__ gambuf, const DevPriors* __restrict__ pri,
                                                        const int* __restrict__ act, const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{},
                                                        TrackFull tw = TrackFull{}) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, act, n_act, rg, fs)) return;
    M += fs.model; T += fs.model;
    const int b = fs.b;
    const size_t f = (size_t)b * N + fs.n;
    const SeqState S = st[b];
    if (S.status != 0) return;
    const int pend = S.al_pending;                       // multiplier update: re-evaluate the CURRENT iterate
    const int buf = (which || pend) ? S.cur : 1 - S.cur;

    const int nq = M->nq, nl = M->nl, nu = M->nu, nrev = M->nrev, ns = M->ns;
    double* sq = smem;
    double* sal = sq + nq;
    double* ssc = sq + ns;
    double* ssa = ssc + 6 * nl;
    double* sR = ssa + 2 * nrev;                        // R, dR/dphi, dR/dtheta, dR/dpsi of the trunk links (what leg_euler reads)
    double* sgam = sR + 36 * M->n_trunk;
    double* sres = sgam + GAM_STRIDE * nrev;
    double* sH = sres + nu;
    double* sg = sH + nu * nu;
    const int4 fw = *reinterpret_cast<const int4*>(M->fn_lane[lane]);
    double* stf = qbuf + (size_t)buf * n_frames * ns + f * ns;
    for (int t = lane; t < ns; t += WAVE) sq[t] = stf[t];
    const double xtg = lane < nu ? xt[f * CPE_NX + lane] : 0.0;
    const int nbnd = M->nb;
    double2 pf_mu = make_double2(0.0, 0.0);
    if (nbnd > 0) pf_mu = reinterpret_cast<const double2*>(mu)[f * (size_t)nbnd + (lane < nbnd ? lane : nbnd - 1)];
    wave_lds_sync();
    // ---- the state phases (cpe_kernels.hip): no marker is read, so no leg vectors and no S rows
    wave_state_sincos(M, sq, sal, ssc, ssa, nrev, lane);
    wave_lds_sync();
    wave_tail_roll(sq, ssc, M->hj_n, fw.x, lane);
    wave_trunk_rotations(M, ssc, sR, fw.y, lane);
    wave_lds_sync();
    wave_leg_state(sq, ssc, ssa, sR, sgam, nrev, fw.z, lane);
    // ---- the tracked term: x on the cost view reads independent coordinates only (trunk Euler angles, alpha), none of those written above
    double ft = 0.0;
    if (lane < nu) {
        const int r = M->rel_ref_u[lane];
        const double d = M->rel_sign_u[lane] * (cost_coord(M, sq, lane) - (r >= 0 ? cost_coord(M, sq, r) : 0.0)) - xtg;
        if constexpr (FULLW) sres[lane] = d;
        else {
            const double w = T->w[lane];
            ft = w * d * d;
            sres[lane] = 2.0 * w * d;
        }
    }
    if constexpr (FULLW) {
        const double* Hn = tw.H + f * (size_t)(NU * NU);
        for (int t = lane; t < nu * nu; t += WAVE) sH[t] = Hn[t];
        wave_lds_sync();
        double r = 0.0;
        if (lane < nu) {
            const double* Wn = tw.W + f * (size_t)(NU * NU) + lane;
#pragma unroll 4
            for (int k = 0; k < nu; k++) r += Wn[k * NU] * sres[k];
            r *= 2.0;
            ft = 0.5 * sres[lane] * r;
        }
        wave_lds_sync();
        if (lane < nu) sres[lane] = r;
    } else {
        for (int t = lane; t < nu * nu; t += WAVE) sH[t] = T->H[t];
    }
    wave_lds_sync();
    if (lane < nq) stf[lane] = sq[lane];                  // Euler part of the state, consistent with the joint equalities
    if (lane < GAM_STRIDE * nrev) gambuf[((size_t)buf * n_frames + f) * (GAM_STRIDE * nrev) + lane] = sgam[lane];
    if (lane < nu) {                                      // g = X^T (2 w (x - x*)), fixed order
        double a = 0.0;
        for (int k = 0; k < nu; k++) a += T->Xt[lane][k] * sres[k];
        sg[lane] = a;
    }
    ft = wave_sum(ft);
    wave_lds_sync();

    // ---- angle bounds, augmented Lagrangian (as k_frame_normal)
    double fb = 0.0, vm = 0.0;
    if (lane < nbnd) {
        const int bq = M->bnd_q[lane];
        const double b_lo = M->bound_lo[lane], b_up = M->bound_up[lane];
        const double kp = M->bound_penalty;
        const double v = sq[bq & 255] + (((bq >> 16) & 255) ? sq[((bq >> 16) & 255) - 1] : 0.0)
                         - (((bq >> 8) & 255) ? sq[((bq >> 8) & 255) - 1] + (((bq >> 24) & 255) ? sq[((bq >> 24) & 255) - 1] : 0.0) : 0.0);
        double* mp = mu + (f * (size_t)nbnd + lane) * 2;
        double mu_up = pf_mu.x, mu_lo = pf_mu.y;
        const double du = v - b_up, dlo = b_lo - v;
        if (pend) {
            mu_up = fmax(0.0, mu_up + kp * du); mu_lo = fmax(0.0, mu_lo + kp * dlo);
            mp[0] = mu_up; mp[1] = mu_lo;
        }
        vm = fmax(0.0, fmax(du, dlo));
        const double pu = fmax(0.0, mu_up + kp * du), pl = fmax(0.0, mu_lo + kp * dlo);
        fb = (pu * pu - mu_up * mu_up + pl * pl - mu_lo * mu_lo) / (2.0 * kp);
        if (pu > 0.0 || pl > 0.0) {
            const double gv = pu - pl, hv = kp * ((pu > 0.0 ? 1.0 : 0.0) + (pl > 0.0 ? 1.0 : 0.0));
            const int ka = M->bound_ua[lane], kb = M->bound_ub[lane];
            int col[8]; double val[8]; int nz = 0;
            for (int side = 0; side < 2; side++) {
                const int k = side == 0 ? ka : kb;
                if (k < 0) continue;
                const double sgn = side == 0 ? 1.0 : -1.0;
                const int r = M->rev_of_u[k];
                if (r < 0) { col[nz] = k; val[nz++] = sgn; }
                else {
                    col[nz] = k; val[nz++] = sgn * sgam[GAM_STRIDE * r];
                    for (int a = 0; a < 3; a++) { col[nz] = M->rev_body_u[r][a]; val[nz++] = sgn * sgam[GAM_STRIDE * r + 1 + a]; }
                }
            }
            for (int i = 0; i < nz; i++) {
                atomicAdd(sg + col[i], gv * val[i]);
                for (int j = 0; j < nz; j++) atomicAdd(sH + col[i] * nu + col[j], hv * val[i] * val[j]);
            }
        }
    }
    fb = wave_sum(fb);
    vm = wave_max(vm);
    wave_lds_sync();

    // ---- Gaussian-mixture pose prior (as k_frame_normal: x = X' u, curvature sum_k gamma_k X'^T P_k X')
    double fpz = 0.0;
    if constexpr (GMM) {
        const int K = pri->p.gmm_k, D = pri->p.gmm_dim, off = nu - D;
        double* sxv = sg + nu;
        double* sv = sxv + CPE_NX;
        double* slp = sv + K * D;
        double* sgr = slp + CPE_MAX_GMM;
        if (lane < D) {
            const int k = off + lane, r = M->rel_ref_u[k];
            sxv[lane] = M->rel_sign_u[k] * (cost_coord(M, sq, k) - (r >= 0 ? cost_coord(M, sq, r) : 0.0));
        }
        wave_lds_sync();
        constexpr int CH = 8;
        for (int t = lane; t < K * D; t += WAVE) {
            const int k = t / D, i = t - k * D;
            double a = 0.0;
            for (int j0 = 0; j0 < D; j0 += CH) {
                double pq[CH], mq[CH];
#pragma unroll
                for (int u = 0; u < CH; u++) { const int j = j0 + u < D ? j0 + u : D - 1; pq[u] = pri->gmm_PT[k][j][i]; mq[u] = pri->p.gmm_mu[k][j]; }
#pragma unroll
                for (int u = 0; u < CH; u++) if (j0 + u < D) a += pq[u] * (sxv[j0 + u] - mq[u]);
            }
            sv[t] = a;
        }
        wave_lds_sync();
        if (lane < K) {
            double qf = 0.0;
            for (int i0 = 0; i0 < D; i0 += CH) {
                double mq[CH];
#pragma unroll
                for (int u = 0; u < CH; u++) mq[u] = pri->p.gmm_mu[lane][i0 + u < D ? i0 + u : D - 1];
#pragma unroll
                for (int u = 0; u < CH; u++) if (i0 + u < D) qf += sv[lane * D + i0 + u] * (sxv[i0 + u] - mq[u]);
            }
            slp[lane] = pri->p.gmm_logw[lane] - 0.5 * qf;
        }
        wave_lds_sync();
        double mx = -1e300, sum = 0.0;
        for (int k = 0; k < K; k++) mx = fmax(mx, slp[k]);
        for (int k = 0; k < K; k++) sum += exp(slp[k] - mx);
        const double dens = sum * exp(mx) + 1e-12;
        fpz = -log(dens);
        double resp[CPE_MAX_GMM];
#pragma unroll
        for (int k = 0; k < CPE_MAX_GMM; k++) resp[k] = k < K ? exp(slp[k]) / dens : 0.0;
        if (lane < D) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < CPE_MAX_GMM; k++) if (k < K) a += resp[k] * sv[k * D + lane];
            sgr[lane] = a;
        }
        wave_lds_sync();
        if (lane < nu) {
            double a = 0.0;
            for (int i0 = 0; i0 < D; i0 += CH) {
                double xq[CH];
#pragma unroll
                for (int u = 0; u < CH; u++) xq[u] = pri->Xc[off + (i0 + u < D ? i0 + u : D - 1)][lane];
#pragma unroll
                for (int u = 0; u < CH; u++) if (i0 + u < D) a += xq[u] * sgr[i0 + u];
            }
            sg[lane] += a;
        }
        for (int t0 = lane; t0 < nu * nu; t0 += 2 * WAVE) {
            const int t1 = t0 + WAVE;
            const bool h1 = t1 < nu * nu;
            const int t1c = h1 ? t1 : t0;
            double q0[CPE_MAX_GMM], q1[CPE_MAX_GMM];
#pragma unroll
            for (int k = 0; k < CPE_MAX_GMM; k++) { const int kc = k < K ? k : K - 1; q0[k] = pri->gmm_Q[kc][t0]; q1[k] = pri->gmm_Q[kc][t1c]; }
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int k = 0; k < CPE_MAX_GMM; k++) { a0 += resp[k] * q0[k]; a1 += resp[k] * q1[k]; }
            sH[t0] += a0;
            if (h1) sH[t1] += a1;
        }
        wave_lds_sync();
    }

    // ---- write out (k_frame_normal's cost record: slot 0 holds the tracked cost in place of the reprojection cost)
    const size_t fo = (size_t)buf * n_frames + f;
    double* Bo = Bbuf + fo * (nu * nu);
    for (int t = lane; t < nu * nu; t += WAVE) Bo[t] = sH[t];
    if (lane < nu) gbuf[fo * nu + lane] = sg[lane];
    if (lane == 0) {
        double* cb = costbuf + fo * COST_STRIDE;
        cb[0] = ft; cb[1] = fb; cb[2] = fpz; cb[3] = 0.0; cb[4] = vm; cb[5] = 0.0;
    }
}
