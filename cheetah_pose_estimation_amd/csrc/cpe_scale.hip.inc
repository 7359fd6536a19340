// cpe_scale.hip.inc -- the reduced system of the segment-length calibration (include/cpe.h, cpe_scale_system; DESIGN.md 2 "What is calibrated").
// Unknowns beside the poses u: one scale s_g per segment group, G <= CPE_MAX_SCALES.  Marker positions are linear in the chain vectors,
// p_l = x_base + sum_k R_{chain_link[l][k]} chain_vec[l][k], and the chain vectors are linear in the scales, so d p_l / d s_g =
// sum_k R_k dchain_vec[g][l][k] with constant dchain_vec (the host builds it from the skeleton's length derivatives).  Two kernels:
//   k_scale_cross   per frame: A_n = d2 J / ds ds, b_n = d J / ds, E_n = d2 J / du ds of the measurement cost (Gauss-Newton, k_frame_normal's weights)
//   k_band_forward  per sequence: Y = L^-1 [E | g] on the block-banded factor k_lm_step left, then A - Y^T Y and b - Y^T L^-1 g
// No atomics; every sum has a fixed order, and nothing depends on the batch.

#define SCALE_RHS (CPE_MAX_SCALES + 1)      // right-hand sides of the forward substitution: the G columns of E and the gradient g
#define SCALE_PARTS 3                       // lanes per right-hand side in the off-diagonal updates of k_band_forward (17 x 3 <= 64)

// doubles of one frame's record: A_n [G][G] | b_n [G] | E_n [28][G]
__host__ __device__ inline int scale_record(int G) { return G * G + G + NU * G; }

// entry e of the lower triangle of a square matrix, rows first: (g, h) with h <= g
__device__ __forceinline__ void lower_entry(int e, int& g, int& h) {
    g = 0;
    while ((g + 1) * (g + 2) / 2 <= e) g++;
    h = e - g * (g + 1) / 2;
}

// ---- per-frame pieces, one wave per frame.  State: the current buffer of the sequence as k_frame_normal left it (its Euler part is consistent with
// the joint equalities); the state phases and the reduced marker columns Dp as k_marker_cov builds them (cpe_kernels.hip, wave_point_columns),
// the positions by k_frame_normal's formula.  Then, per marker l, the sums over its cameras -- in camera order, by the marker's own lane --
//     M_l = sum_c kappa (m w)^2 G^T G  (3 x 3),    r_l = sum_c rho'(t) m w G^T  (3),      t = m w e, G = d pixel / d p
// with robust_loss' gradient weight and curvature weight kappa (opts.curvature) and project_point_staged's near-plane handling, exactly the terms
// k_frame_normal adds into its Mv.  Ds_l[g] = d p_l / d s_g from the full rotations of every link (the state's Euler angles), and
//     A_n[g][h] = sum_l Ds_lg . M_l Ds_lh      b_n[g] = sum_l Ds_lg . r_l      E_n[k][g] = sum_l Dp_lk . M_l Ds_lg
// summed over the markers in their order; an entry of A_n and its mirror are stored from one register.  A group no marker depends on has
// dchain_vec = 0: its rows and columns are sums of products with 0.0.
// dynamic LDS (doubles): state | sin / cos | leg sin / cos | trunk R, dR | dynamic vectors | S rows | Dp | positions | cameras | M_l, r_l
//                        | R of every link | Ds [L][G][3] | M Ds [L][G][3] | item of (marker, reduced column) (int) | first term of every item (int)
// dcv: dchain_vec of every model [model][G][L][CPE_MAX_CHAIN][3]
// The carve of a frame's dynamic LDS, in the order of the comment above, and what k_scale_cross and k_scale_points (cpe_scale_cov.hip.inc) share.
struct ScaleLds {
    double *sq, *sal, *ssc, *ssa, *sR, *sdyn, *sSv, *sDp, *spos, *scam, *sMv, *sRf, *sDs, *sMD;
    int *sIdx, *sBeg;
};
// The first half of a frame, one wave: the carve, the state and the cameras into LDS, the state phases, the reduced marker columns Dp, the rotation
// of every link and the item of every (marker, reduced column) (-1: the marker does not depend on that column).  stf: the frame's state.  Ends
// with a wave_lds_sync.
__device__ __forceinline__ void wave_scale_head(const DevModel* __restrict__ M, const double* __restrict__ stf, int G, double* smem, ScaleLds& s,
                                                int lane) {
    const int nq = M->nq, nl = M->nl, L = M->L, C = M->C, nrev = M->nrev, ns = M->ns, svn = M->sv_n, mct = M->mc_total;
    s.sq = smem;
    s.sal = s.sq + nq;
    s.ssc = s.sal + nrev;
    s.ssa = s.ssc + 6 * nl;
    s.sR = s.ssa + 2 * nrev;
    s.sdyn = s.sR + 36 * M->n_trunk;
    s.sSv = s.sdyn + 3 * svn;
    s.sDp = s.sSv + CPE_MAX_SCOL * M->n_srow;
    s.spos = s.sDp + 3 * mct;
    s.scam = s.spos + 3 * L;
    s.sMv = s.scam + CAMW * C;
    s.sRf = s.sMv + 9 * L;
    s.sDs = s.sRf + 9 * nl;
    s.sMD = s.sDs + 3 * L * G;
    s.sIdx = reinterpret_cast<int*>(s.sMD + 3 * L * G);
    s.sBeg = s.sIdx + L * NU;

    const int4 fw = *reinterpret_cast<const int4*>(M->fn_lane[lane]);
    const int hj_n = M->hj_n, hk_n = M->hk_n;
    const int2 hkw = *reinterpret_cast<const int2*>(M->hk_w[lane]);
    for (int t = lane; t < ns; t += WAVE) s.sq[t] = stf[t];
    const double* camw = reinterpret_cast<const double*>(M->cam);
    for (int t = lane; t < CAMW * C; t += WAVE) s.scam[t] = camw[t];
    for (int t = lane; t < L * NU; t += WAVE) s.sIdx[t] = -1;
    wave_lds_sync();
    // ---- the state phases (cpe_kernels.hip); the legs' Euler angles are not rebuilt: the state holds them
    wave_state_sincos(M, s.sq, s.sal, s.ssc, s.ssa, nrev, lane);
    wave_lds_sync();
    wave_tail_roll(s.sq, s.ssc, hj_n, fw.x, lane);
    wave_trunk_rotations(M, s.ssc, s.sR, fw.y, lane);
    wave_lds_sync();
    wave_hooke_srows(s.sR, s.sSv, hk_n, hkw, lane);
    wave_point_columns(M, s.ssa, s.sR, s.sSv, s.sdyn, s.sDp, s.sBeg, lane);
    // ---- the rotation of every link, the item of every (marker, reduced column)
    if (lane < nl) rot_kind(s.ssc + 6 * lane, 0, s.sRf + 9 * lane);
    for (int t = lane; t < mct; t += WAVE) { const int l = M->mc_marker[t]; s.sIdx[l * NU + M->mcol[l][M->mc_j[t]]] = t; }
    wave_lds_sync();
}
// Ds_l[g] = d p_l / d s_g = sum_k R_{chain_link[l][k]} dchain_vec[g][l][k], over the chain in its order; dv: the model's dchain_vec, sRf: wave_scale_head's
__device__ __forceinline__ void scale_point_derivative(const DevModel* __restrict__ M, const double* __restrict__ dv, const double* sRf, int l, int g,
                                                       double& d0, double& d1, double& d2) {
    const double* v = dv + ((size_t)g * M->L + l) * (CPE_MAX_CHAIN * 3);
    const int n = M->chain_len[l];
    d0 = 0.0; d1 = 0.0; d2 = 0.0;
    for (int k = 0; k < n; k++) {
        const double* R = sRf + 9 * M->chain_link[l][k];
        const double v0 = v[3 * k], v1 = v[3 * k + 1], v2 = v[3 * k + 2];
        d0 += R[0] * v0 + R[1] * v1 + R[2] * v2; d1 += R[3] * v0 + R[4] * v1 + R[5] * v2; d2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
    }
}

template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_scale_cross(const DevModel* __restrict__ M, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                      const double* __restrict__ qbuf, const double* __restrict__ meas,
                                                      const double* __restrict__ weight, const double* __restrict__ dcv, int G,
                                                      double* __restrict__ rec, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs)) return;
    M += fs.model;
    const int b = fs.b;
    if (!cov_seq_ok(st, b)) return;
    const size_t f = (size_t)b * N + fs.n;
    const int buf = st[b].cur;
    const int L = M->L, C = M->C, ns = M->ns;
    const double* dv = dcv + (size_t)fs.model * G * L * (CPE_MAX_CHAIN * 3);
    ScaleLds s;
    wave_scale_head(M, qbuf + (size_t)buf * n_frames * ns + f * ns, G, smem, s, lane);
    double *sq = s.sq, *sR = s.sR, *sdyn = s.sdyn, *sDp = s.sDp, *spos = s.spos, *scam = s.scam, *sMv = s.sMv, *sRf = s.sRf, *sDs = s.sDs, *sMD = s.sMD;
    int* sIdx = s.sIdx;
    // ---- marker positions (k_frame_normal's formula)
    if (lane < L) {
        double p0 = sq[0], p1 = sq[1], p2 = sq[2];
#pragma unroll
        for (int k = 0; k < CPE_MAX_CHAIN; k++) {          // entries past the chain's length: rotation 0 times a zero vector
            const double* R = sR + M->pc_off[lane][k];
            const double v0 = M->pc_vec[lane][k][0], v1 = M->pc_vec[lane][k][1], v2 = M->pc_vec[lane][k][2];
            p0 += R[0] * v0 + R[1] * v1 + R[2] * v2; p1 += R[3] * v0 + R[4] * v1 + R[5] * v2; p2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
        }
        const int wid = M->pw_id[lane];
        if (wid >= 0) {
            const double* R = sR + M->pw_off[lane];
            const double v0 = sdyn[3 * wid], v1 = sdyn[3 * wid + 1], v2 = sdyn[3 * wid + 2];
            p0 += R[0] * v0 + R[1] * v1 + R[2] * v2; p1 += R[3] * v0 + R[4] * v1 + R[5] * v2; p2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
        }
        spos[3 * lane] = p0; spos[3 * lane + 1] = p1; spos[3 * lane + 2] = p2;
    }
    wave_lds_sync();
    // ---- M_l and r_l: the marker's lane walks its cameras in order
    const size_t pair0 = f * (size_t)((RAGGED ? rg.cstride : C) * L);
    if (lane < L) {
        double m6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r3[3] = {0.0, 0.0, 0.0};
        const double px = spos[3 * lane], py = spos[3 * lane + 1], pz = spos[3 * lane + 2];
        for (int c = 0; c < C; c++) {
            const double w = scam[CAMW * c + 21] * weight[pair0 + (size_t)c * L + lane];
            const double2 z = reinterpret_cast<const double2*>(meas)[pair0 + (size_t)c * L + lane];
            if (w == 0.0) continue;
            double u, v, Gp[6];
            project_point_staged(scam, c, px, py, pz, u, v, Gp);
            const LossOut l0 = robust_loss(w * (u - z.x), M->loss_a, M->loss_b, M->loss_c, M->curvature, true);
            const LossOut l1 = robust_loss(w * (v - z.y), M->loss_a, M->loss_b, M->loss_c, M->curvature, true);
            const double g0 = l0.d1 * w, g1 = l1.d1 * w, c0 = l0.cw * w * w, c1 = l1.cw * w * w;
            m6[0] += c0 * Gp[0] * Gp[0] + c1 * Gp[3] * Gp[3]; m6[1] += c0 * Gp[0] * Gp[1] + c1 * Gp[3] * Gp[4]; m6[2] += c0 * Gp[0] * Gp[2] + c1 * Gp[3] * Gp[5];
            m6[3] += c0 * Gp[1] * Gp[1] + c1 * Gp[4] * Gp[4]; m6[4] += c0 * Gp[1] * Gp[2] + c1 * Gp[4] * Gp[5]; m6[5] += c0 * Gp[2] * Gp[2] + c1 * Gp[5] * Gp[5];
            r3[0] += g0 * Gp[0] + g1 * Gp[3]; r3[1] += g0 * Gp[1] + g1 * Gp[4]; r3[2] += g0 * Gp[2] + g1 * Gp[5];
        }
#pragma unroll
        for (int e = 0; e < 6; e++) sMv[9 * lane + e] = m6[e];
#pragma unroll
        for (int e = 0; e < 3; e++) sMv[9 * lane + 6 + e] = r3[e];
    }
    wave_lds_sync();
    // ---- Ds_l[g] and M_l Ds_l[g], one (marker, group) per lane and round
    for (int t = lane; t < L * G; t += WAVE) {
        const int l = t / G, g = t - l * G;
        double d0, d1, d2;
        scale_point_derivative(M, dv, sRf, l, g, d0, d1, d2);
        const double* Mv = sMv + 9 * l;
        sDs[3 * t] = d0; sDs[3 * t + 1] = d1; sDs[3 * t + 2] = d2;
        sMD[3 * t] = Mv[0] * d0 + Mv[1] * d1 + Mv[2] * d2;
        sMD[3 * t + 1] = Mv[1] * d0 + Mv[3] * d1 + Mv[4] * d2;
        sMD[3 * t + 2] = Mv[2] * d0 + Mv[4] * d1 + Mv[5] * d2;
    }
    wave_lds_sync();
    // ---- the frame's record
    double* o = rec + f * (size_t)scale_record(G);
    for (int e = lane; e < G * (G + 1) / 2; e += WAVE) {
        int g, h; lower_entry(e, g, h);
        double s = 0.0;
        for (int l = 0; l < L; l++) {
            const double* d = sDs + 3 * (l * G + g); const double* y = sMD + 3 * (l * G + h);
            s += d[0] * y[0] + d[1] * y[1] + d[2] * y[2];
        }
        o[g * G + h] = s; o[h * G + g] = s;
    }
    if (lane < G) {
        double s = 0.0;
        for (int l = 0; l < L; l++) {
            const double* d = sDs + 3 * (l * G + lane); const double* r = sMv + 9 * l + 6;
            s += d[0] * r[0] + d[1] * r[1] + d[2] * r[2];
        }
        o[G * G + lane] = s;
    }
    for (int t = lane; t < NU * G; t += WAVE) {
        const int k = t / G, g = t - k * G;
        double s = 0.0;
        for (int l = 0; l < L; l++) {
            const int it = sIdx[l * NU + k];
            if (it < 0) continue;
            const double* d = sDp + 3 * it; const double* y = sMD + 3 * (l * G + g);
            s += d[0] * y[0] + d[1] * y[1] + d[2] * y[2];
        }
        o[G * G + G + t] = s;
    }
}

// ---- L Y = [E | g] for G + 1 right-hand sides on the block-banded factor, oldest frame first -- the mirror image of k_band_sample's back
// substitution, on Lbuf as k_lm_step leaves it (column n: block 0 = L(n,n) with the reciprocals on its diagonal, block i = L(n+i,n)):
//     Y_n = L(n,n)^-1 t_n,     t_m = [E_m | g_m] - sum_{i=1..PB} L(m,m-i) Y_{m-i}
// column by column: once Y_n is known, the pending t of the frames n+1 .. n+PB (an LDS ring over the frame index mod PB) take their terms of
// column n, so t_m receives the columns m-PB .. m-1 in that order and every product sums over the block's columns in ascending order.  One
// wave per sequence.  The column (25-31 KB) is staged in LDS by all lanes and read back as broadcasts; right-hand side j belongs to lanes
// j + 17 p: part 0 solves the triangle (28 steps, registers), all SCALE_PARTS parts share the rows of the off-diagonal products.  The Gram
// products Y^T Y and Y^T (L^-1 g) and the sums of A_n, b_n and of the measurement cost grow frame by frame in the registers of the lane that
// stores them: entry (g, h) and its mirror come from one register, so A and A_red are exactly symmetric.
// A sequence without a factor is left alone (the caller zeroed its outputs); RAGGED: the sequence's own length.
// Yneg (or null): -Y_E = -L^-1 E, column g of frame n at [b][g][n][row] -- the right-hand sides from which k_band_sample's back substitution gives
// the response of the poses to the scales, R = -(H + ridge D)^-1 E (cpe_scale_response); storing it changes nothing of the other outputs.
template <int PB, bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_band_forward(const SeqState* __restrict__ st, const double* __restrict__ Lbuf, const double* __restrict__ gtbuf,
                                                       const double* __restrict__ costbuf, const double* __restrict__ rec, int NS, size_t n_frames,
                                                       int G, double* __restrict__ A, double* __restrict__ bv, double* __restrict__ A_red,
                                                       double* __restrict__ b_red, double* __restrict__ cost, double* __restrict__ Yneg,
                                                       RaggedArgs rg = RaggedArgs{}) {
    constexpr int RING = PB + 1, BB = NU * NU, COLD = RING * BB;
    static_assert(PB >= 3 && PB <= 4, "the half-bandwidths of the covariance entries");
    __shared__ double col[COLD];
    __shared__ double ring[PB * NU * SCALE_RHS];           // pending t of frame m: [m % PB][row][rhs]
    __shared__ double sY[NU * SCALE_RHS];                  // Y_n [row][rhs]
    const int lane = threadIdx.x, b = blockIdx.x;
    int N = NS;
    if constexpr (RAGGED) N = rg.seq[b].y;
    if (!cov_seq_ok(st, b)) return;                         // uniform
    const int buf = st[b].cur, R = G + 1, SC = scale_record(G);
    const int j = lane % SCALE_RHS, part = lane / SCALE_RHS;
    const bool live = j < R && part < SCALE_PARTS;
    const double* Lb = Lbuf + (size_t)b * NS * COLD;
    const double* gtb = gtbuf + (size_t)b * NS * NU;
    const double* cb = costbuf + ((size_t)buf * n_frames + (size_t)b * NS) * COST_STRIDE;
    const double* rb = rec + (size_t)b * NS * SC;
    // this lane's entries of the lower triangle of the (G + 1) x (G + 1) Gram matrix: rows g < G are Y^T Y, row G is (L^-1 g)^T Y
    constexpr int EPL = (SCALE_RHS * (SCALE_RHS + 1) / 2 + WAVE - 1) / WAVE;
    const int n_ent = R * (R + 1) / 2;
    int eg[EPL], eh[EPL];
    double gram[EPL], sum[EPL], cst = 0.0;
#pragma unroll
    for (int i = 0; i < EPL; i++) {
        const int e = lane + WAVE * i;
        eg[i] = eh[i] = 0; gram[i] = sum[i] = 0.0;
        if (e < n_ent) lower_entry(e, eg[i], eh[i]);
    }
    for (int t = lane; t < PB * NU * SCALE_RHS; t += WAVE) ring[t] = 0.0;
    for (int n = 0; n < N; n++) {
        const double* Lc = Lb + (size_t)n * COLD;
        for (int t = lane; t < COLD; t += WAVE) col[t] = Lc[t];
        wave_lds_sync();
        double* pend = ring + (n % PB) * (NU * SCALE_RHS);
        if (live && part == 0) {
            double t[NU];
#pragma unroll
            for (int k = 0; k < NU; k++) {
                const double rhs = j < G ? rb[(size_t)n * SC + G * G + G + k * G + j] : gtb[(size_t)n * NU + k];
                t[k] = rhs + pend[k * SCALE_RHS + j];
                pend[k * SCALE_RHS + j] = 0.0;               // the slot now belongs to frame n + PB
            }
#pragma unroll
            for (int m = 0; m < NU; m++) {
                const double y = t[m] * col[m * NU + m];
                t[m] = y;
#pragma unroll
                for (int a = m + 1; a < NU; a++) t[a] = fma(-col[a * NU + m], y, t[a]);
            }
#pragma unroll
            for (int k = 0; k < NU; k++) sY[k * SCALE_RHS + j] = t[k];
            if (Yneg && j < G) {                             // -Y_E as right-hand side j of k_band_sample: [b][j][n][row]
                double* yo = Yneg + (((size_t)b * G + j) * NS + n) * NU;
#pragma unroll
                for (int k = 0; k < NU; k++) yo[k] = -t[k];
            }
        }
        wave_lds_sync();
        if (live) {
            double y[NU];
#pragma unroll
            for (int k = 0; k < NU; k++) y[k] = sY[k * SCALE_RHS + j];
#pragma unroll
            for (int i = 1; i <= PB; i++) {
                if (n + i < N) {                             // uniform
                    const double* Li = col + i * BB;
                    double* pi = ring + ((n + i) % PB) * (NU * SCALE_RHS) + j;
                    for (int a = part; a < NU; a += SCALE_PARTS) {
                        double s = pi[a * SCALE_RHS];
#pragma unroll
                        for (int k = 0; k < NU; k++) s = fma(-Li[a * NU + k], y[k], s);
                        pi[a * SCALE_RHS] = s;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < EPL; i++) {
            if (lane + WAVE * i < n_ent) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < NU; k++) s = fma(sY[k * SCALE_RHS + eg[i]], sY[k * SCALE_RHS + eh[i]], s);
                gram[i] += s;
                if (eg[i] < G) sum[i] += rb[(size_t)n * SC + eg[i] * G + eh[i]];
                else if (eh[i] < G) sum[i] += rb[(size_t)n * SC + G * G + eh[i]];
            }
        }
        if (lane == WAVE - 1) cst += cb[(size_t)n * COST_STRIDE];
        wave_lds_sync();                                     // column n and Y_n are retired
    }
#pragma unroll
    for (int i = 0; i < EPL; i++) {
        if (lane + WAVE * i < n_ent) {
            const int g = eg[i], h = eh[i];
            if (g < G) {
                const double red = sum[i] - gram[i];
                A[((size_t)b * G + g) * G + h] = sum[i]; A[((size_t)b * G + h) * G + g] = sum[i];
                A_red[((size_t)b * G + g) * G + h] = red; A_red[((size_t)b * G + h) * G + g] = red;
            } else if (h < G) {
                bv[(size_t)b * G + h] = sum[i];
                b_red[(size_t)b * G + h] = sum[i] - gram[i];
            }
        }
    }
    if (lane == WAVE - 1) cost[b] = cst;
}
