// cpe_scale_cov.hip.inc -- the pose covariance marginalised over the fitted segment lengths (include/cpe.h, cpe_scale_response /
// cpe_covariance_add_scales; DESIGN.md 2 "What is marginalised").  The joint Gauss-Newton matrix over (u, s) is a block arrow: pose blocks
// H + ridge D, borders E = d2 J / du ds, corner A + P.  Its inverse has
//     R = du / ds = -(H + ridge D)^-1 E        cov(u) = Sigma + R cov_s R^T        cov(p_l) = P_l Sigma P_l^T + W_l cov_s W_l^T,  W_l = Ds_l + P_l R_n
// R comes from the factor: k_band_forward leaves -Y_E = -L^-1 E (cpe_scale.hip.inc) and k_band_sample solves L^T X = -Y_E for the G right-hand
// sides (cpe_sample.hip.inc).  Three kernels here:
//   k_response_lens   per sequence: the frame count k_band_sample is given -- 0 for a sequence without a factor
//   k_scale_points    per frame: R_n from the back substitution's layout into resp_u, and W = Ds + Dp R_n
//   k_cov_add_scales  per frame: the band blocks and the marker blocks plus their scale terms
// No atomics; every sum has a fixed order, and nothing depends on the batch.

template <bool RAGGED = false>
__global__ void k_response_lens(const SeqState* __restrict__ st, int B, int N, int* __restrict__ lens, RaggedArgs rg = RaggedArgs{}) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = N;
    if constexpr (RAGGED) n = rg.seq[b].y;
    lens[b] = cov_seq_ok(st, b) ? n : 0;
}

// ---- per frame, one wave: k_scale_cross's first half (wave_scale_head: state phases, Dp, link rotations, items), then
//     resp_u[n][k][g] = R_n[k][g]                             from X [b][g][n][k], k_band_sample's layout
//     resp_pos[n][l][a][g] = Ds_l[g][a] + sum_k Dp_lk[a] R_n[k][g]     over the marker's reduced columns k ascending
// one (marker, group) per lane and round.  resp_pos may be null.  A sequence without a factor and the frames past a sequence's own are left alone
// (the caller zeroed the outputs).  dynamic LDS: k_scale_cross's carve | R_n [28][G]
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_scale_points(const DevModel* __restrict__ M, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                       const double* __restrict__ qbuf, const double* __restrict__ dcv, int G,
                                                       const double* __restrict__ X, double* __restrict__ resp_u, double* __restrict__ resp_pos,
                                                       RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs)) return;
    M += fs.model;
    const int b = fs.b;
    if (!cov_seq_ok(st, b)) return;
    const size_t f = (size_t)b * N + fs.n;
    const int buf = st[b].cur;
    const int L = M->L, ns = M->ns;
    const double* dv = dcv + (size_t)fs.model * G * L * (CPE_MAX_CHAIN * 3);
    ScaleLds s;
    wave_scale_head(M, qbuf + (size_t)buf * n_frames * ns + f * ns, G, smem, s, lane);
    double* sRn = reinterpret_cast<double*>(s.sBeg + M->mc_total + (M->mc_total & 1));       // (8-byte aligned: L NU is even)
    for (int t = lane; t < NU * G; t += WAVE) {
        const int g = t / NU, k = t - g * NU;
        const double v = X[(((size_t)b * G + g) * N + fs.n) * NU + k];
        sRn[k * G + g] = v;
        resp_u[(f * NU + k) * G + g] = v;
    }
    wave_lds_sync();
    if (!resp_pos) return;                                    // uniform
    for (int t = lane; t < L * G; t += WAVE) {
        const int l = t / G, g = t - l * G;
        double w0, w1, w2;
        scale_point_derivative(M, dv, s.sRf, l, g, w0, w1, w2);
        for (int k = 0; k < NU; k++) {
            const int it = s.sIdx[l * NU + k];
            if (it < 0) continue;
            const double* d = s.sDp + 3 * it;
            const double r = sRn[k * G + g];
            w0 = fma(d[0], r, w0); w1 = fma(d[1], r, w1); w2 = fma(d[2], r, w2);
        }
        double* o = resp_pos + (f * (size_t)L + l) * 3 * G + g;
        o[0] = w0; o[G] = w1; o[2 * G] = w2;
    }
}

// ---- per frame n of sequence b, one wave:
//     cov_diag_m[n]      = cov_diag[n]      + R_n     cov_s R_n^T
//     cov_off_m[n][i-1]  = cov_off[n][i-1]  + R_{n+i} cov_s R_n^T        i = 1..pb, n + i < the sequence's frames
//     cov_pos_m[n][l]    = cov_pos[n][l]    + W_l     cov_s W_l^T
// in cpe_band_inverse's layout.  Staged in LDS with rows of GS = G | 1 doubles (an odd stride: consecutive rows fall on different banks): cov_s
// from its lower triangle, R_n .. R_{n+pb}, T = R_n cov_s, W and W cov_s.  T[c][g] = sum_h cov_s[g][h] R_n[c][h] over h ascending, and an
// entry [r][c] of a block = sum_g R_{n+i}[r][g] T[c][g] over g ascending; an entry of the diagonal block, and of a marker block, is computed in its
// lower triangle and stored with its mirror from one register.  n_frames: the frames of every sequence (device), or null = all NS; the frames
// past a sequence's own, and the blocks with n + i past them, are left alone (the caller zeroed the outputs).  The marker arrays are null together.
__global__ __launch_bounds__(WAVE) void k_cov_add_scales(const int* __restrict__ n_frames, int NS, int pb, int G, int L, const double* __restrict__ cov_s,
                                                         const double* __restrict__ resp_u, const double* __restrict__ resp_pos,
                                                         const double* __restrict__ cov_diag, const double* __restrict__ cov_off,
                                                         const double* __restrict__ cov_pos, double* __restrict__ cov_diag_m,
                                                         double* __restrict__ cov_off_m, double* __restrict__ cov_pos_m) {
    constexpr int GSM = CPE_MAX_SCALES + 1, BB = NU * NU;
    __shared__ double sC[CPE_MAX_SCALES * GSM];
    __shared__ double sRr[5 * NU * GSM];                      // R_{n+i}, i = 0..4
    __shared__ double sT[NU * GSM];
    __shared__ double sW[CPE_MAX_MARKERS * 3 * GSM];
    __shared__ double sTW[CPE_MAX_MARKERS * 3 * GSM];
    const int lane = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)NS), n = (int)(blockIdx.x % (unsigned)NS);
    const int NL = n_frames ? n_frames[b] : NS;
    if (n >= NL) return;                                      // uniform
    const int GS = G | 1;
    const size_t f = (size_t)b * NS + n;
    int nb = NL - n - 1;                                      // off-diagonal blocks inside the sequence
    if (nb > pb) nb = pb;
    for (int t = lane; t < G * G; t += WAVE) {
        const int g = t / G, h = t - g * G;
        sC[g * GS + h] = cov_s[(size_t)b * G * G + (g >= h ? g * G + h : h * G + g)];
    }
    for (int t = lane; t < (nb + 1) * NU * G; t += WAVE) {
        const int i = t / (NU * G), e = t - i * (NU * G), r = e / G, g = e - r * G;
        sRr[(i * NU + r) * GS + g] = resp_u[(f + i) * (size_t)(NU * G) + e];
    }
    if (cov_pos)
        for (int t = lane; t < 3 * L * G; t += WAVE) {
            const int r = t / G, g = t - r * G;
            sW[r * GS + g] = resp_pos[f * (size_t)(3 * L * G) + t];
        }
    wave_lds_sync();
    for (int t = lane; t < NU * G; t += WAVE) {
        const int c = t / G, g = t - c * G;
        double s = 0.0;
        for (int h = 0; h < G; h++) s = fma(sC[g * GS + h], sRr[c * GS + h], s);
        sT[c * GS + g] = s;
    }
    if (cov_pos)
        for (int t = lane; t < 3 * L * G; t += WAVE) {
            const int r = t / G, g = t - r * G;
            double s = 0.0;
            for (int h = 0; h < G; h++) s = fma(sC[g * GS + h], sW[r * GS + h], s);
            sTW[r * GS + g] = s;
        }
    wave_lds_sync();
    // ---- the diagonal block from its lower triangle
    for (int e = lane; e < BB; e += WAVE) {
        const int r = e / NU, c = e - r * NU;
        if (c > r) continue;
        double s = 0.0;
        for (int g = 0; g < G; g++) s = fma(sRr[r * GS + g], sT[c * GS + g], s);
        const double v = cov_diag[f * BB + e] + s;
        cov_diag_m[f * BB + r * NU + c] = v; cov_diag_m[f * BB + c * NU + r] = v;
    }
    // ---- the off-diagonal blocks (later frame n + i, earlier frame n)
    for (int i = 1; i <= nb; i++) {
        const double* Ri = sRr + i * NU * GS;
        const size_t o = (f * pb + (i - 1)) * BB;
        for (int e = lane; e < BB; e += WAVE) {
            const int r = e / NU, c = e - r * NU;
            double s = 0.0;
            for (int g = 0; g < G; g++) s = fma(Ri[r * GS + g], sT[c * GS + g], s);
            cov_off_m[o + e] = cov_off[o + e] + s;
        }
    }
    // ---- the marker blocks from their lower triangles
    if (cov_pos)
        for (int t = lane; t < 6 * L; t += WAVE) {
            const int l = t / 6;
            int a, c; lower_entry3(t - 6 * l, a, c);
            double s = 0.0;
            for (int g = 0; g < G; g++) s = fma(sW[(3 * l + a) * GS + g], sTW[(3 * l + c) * GS + g], s);
            const size_t o = (f * (size_t)L + l) * 9;
            const double v = cov_pos[o + 3 * a + c] + s;
            cov_pos_m[o + 3 * a + c] = v; cov_pos_m[o + 3 * c + a] = v;
        }
}
