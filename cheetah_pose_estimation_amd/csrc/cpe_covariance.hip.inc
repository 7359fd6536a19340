// cpe_covariance.hip.inc -- posterior covariance of the kinematic estimate (include/cpe.h, cpe_covariance; DESIGN.md 2 "What is inverted").
// Sigma = (H + ridge D)^-1 on its block band, by selected inversion (Takahashi recurrence) of the block Cholesky factor k_lm_step leaves in
// Lbuf.  With T_n = L(n,n)^-1 and G_k = L(n+k,n) T_n (k = 1..PB), columns n = N-1 .. 0:
//     Sigma(n+i,n) = - sum_k Sigma(n+i,n+k) G_k                       i = 1..PB   (Sigma(a,b) = Sigma(b,a)^T for a < b)
//     Sigma(n,n)   = T_n^T T_n - sum_k G_k^T Sigma(n+k,n)
// Every Sigma on the right lies inside the band.  Three kernels: k_cov_prep (frame-parallel: T, G, T^T T -- the whole factor is known up
// front, so the 28-step triangular inverse is not part of the serial chain), k_lm_selinv (the serial sweep, one workgroup per sequence)
// and k_marker_cov (3x3 covariance of every marker position).  No atomics; every sum has a fixed order.  A fourth, k_cov_columns at the end of the
// file, continues the recurrence past the band: whole columns Sigma(0..a, a) for the covariance between distant frames (cpe_covariance_columns).

#define COV_THREADS 256

// A sequence takes part when its evaluation was finite and k_lm_step factored its matrix (it then leaves back_pending = 1; the covariance
// entry does not run k_lm_back).  st == nullptr (cpe_band_inverse): every sequence does.
__device__ __forceinline__ bool cov_seq_ok(const SeqState* __restrict__ st, int b) {
    return st == nullptr || (st[b].status == 0 && st[b].back_pending == 1);
}

// ---- building blocks of the kernels of this file, of cpe_rate_cov.hip.inc and of cpe_force_cov.hip.inc

// One 4 x 4 register tile of a block product on the vector ALU (DESIGN.md 4 has the reason): acc[x][y] (+/-)= A[x * sx + m * sm] * B[m * sb + y]
// for m = m0 .. m1-1 in that order; the strides choose the orientation of A.  UNROLL: the unroll hint of the loop over m (0: none).
template <bool NEG>
__device__ __forceinline__ void tile4_step(double (&acc)[4][4], const double* A, int sx, const double* B) {
    double av[4], bv[4];
#pragma unroll
    for (int x = 0; x < 4; x++) av[x] = A[x * sx];
#pragma unroll
    for (int y = 0; y < 4; y++) bv[y] = B[y];
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = fma(NEG ? -av[x] : av[x], bv[y], acc[x][y]);
}
template <bool NEG, int UNROLL>
__device__ __forceinline__ void tile4_fma(double (&acc)[4][4], const double* A, int sx, int sm, const double* B, int sb, int m0, int m1) {
    if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
        for (int m = m0; m < m1; m++) tile4_step<NEG>(acc, A + m * sm, sx, B + m * sb);
    } else {
        for (int m = m0; m < m1; m++) tile4_step<NEG>(acc, A + m * sm, sx, B + m * sb);
    }
}
__device__ __forceinline__ void tile4_zero(double (&acc)[4][4]) {
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = 0.0;
}
__device__ __forceinline__ void tile4_store(const double (&acc)[4][4], double* O, int ld) {
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) O[x * ld + y] = acc[x][y];
}

// tile t of the lower triangle, rows first: (ti, tj) with tj <= ti
__device__ __forceinline__ void lower_tile(int t, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    tj = t - ti * (ti + 1) / 2;
}

// entry e = 0 .. 5 of the lower triangle of a 3 x 3 block, rows first: (a, c) with c <= a
__device__ __forceinline__ void lower_entry3(int e, int& a, int& c) {
    a = e < 1 ? 0 : (e < 3 ? 1 : 2);
    c = e - a * (a + 1) / 2;
}

// The band of Sigma as k_lm_selinv writes it, half-bandwidth pb: cov_diag block [f] = Sigma(f, f), cov_off block [f][k-1] = Sigma(f + k, f),
// k = 1 .. pb -- the block of (later frame, earlier frame); Sigma(a, b) = Sigma(b, a)^T for a < b.  Returns Sigma(fi, fj)[r][c], |fi - fj| <= pb:
// the stored block as it stands, or transposed where fi < fj.  cd / co: the sequence's cov_diag / cov_off; fi, fj: frames of that sequence.
__device__ __forceinline__ double band_entry(const double* __restrict__ cd, const double* __restrict__ co, int pb, int fi, int fj, int r, int c) {
    constexpr int BB = NU * NU;
    if (fi == fj) return cd[(size_t)fi * BB + r * NU + c];
    if (fi > fj) return co[((size_t)fj * pb + (fi - fj - 1)) * BB + r * NU + c];
    return co[((size_t)fi * pb + (fj - fi - 1)) * BB + c * NU + r];
}

// The operand blocks of one step of a serial sweep, CNT doubles (whole 28 x 28 blocks) from g: requested into registers a step ahead --
// unconditional loads at a clamped index -- and scattered into padded LDS blocks [blk][28][LDB] when their step begins.
template <int CNT>
__device__ __forceinline__ void cov_prefetch(double (&pf)[(CNT + COV_THREADS - 1) / COV_THREADS], const double* g, int tid) {
#pragma unroll
    for (int j = 0; j < (CNT + COV_THREADS - 1) / COV_THREADS; j++) { const int e = tid + COV_THREADS * j; pf[j] = g[e < CNT ? e : CNT - 1]; }
}
template <int CNT>
__device__ __forceinline__ void cov_stage(const double (&pf)[(CNT + COV_THREADS - 1) / COV_THREADS], double* Gs, int tid) {
    constexpr int BB = NU * NU;
#pragma unroll
    for (int j = 0; j < (CNT + COV_THREADS - 1) / COV_THREADS; j++) {
        const int e = tid + COV_THREADS * j;
        if (e < CNT) { const int blk = e / BB, r = (e - blk * BB) / NU, c = e % NU; Gs[blk * BLK + r * LDB + c] = pf[j]; }
    }
}

// Reduced columns Dp of the points of model X (its markers) at the state whose sin / cos, trunk rotations and S rows are in LDS: the dynamic
// vectors of X's leg chains, then the terms of one item (point, column) -- they sit next to each other in X->tl, in item order: a first pass marks
// where every item's terms begin -- summed in list order, one lane per item, so no LDS atomics are needed.  Ends with a wave_lds_sync.
__device__ __forceinline__ void wave_point_columns(const DevModel* __restrict__ X, const double* ssa, const double* sR, const double* sSv,
                                                   double* sdyn, double* sDp, int* sBeg, int lane) {
    const int svn = X->sv_n, mct = X->mc_total, ntl = X->tl_n;
    const int fww = X->fn_lane[lane][3];
    const int svl = lane < CPE_MAX_SDYN ? lane : 0;
    double svv[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) { svv[i][0] = X->sv_vec[svl][i][0]; svv[i][1] = X->sv_vec[svl][i][1]; svv[i][2] = X->sv_vec[svl][i][2]; }
    wave_leg_vectors(ssa, sdyn, svn, fww, svv, lane);
    for (int t = lane; t < mct; t += WAVE) sBeg[t] = ntl;
    wave_lds_sync();
    for (int e = lane; e < ntl; e += WAVE) {
        const int it = X->tl[e].w0 & 1023;
        if (e == 0 || (X->tl[e - 1].w0 & 1023) != it) sBeg[it] = e;
    }
    wave_lds_sync();
    for (int t = lane; t < mct; t += WAVE) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int e = sBeg[t]; e < ntl; e++) {
            const int w0 = X->tl[e].w0;
            if ((w0 & 1023) != t) break;
            const int si = ((w0 >> 10) & 1023) - 1, vd = ((w0 >> 20) & 1023) - 1, moff = X->tl[e].moff;
            const double v0 = vd < 0 ? X->tl[e].v[0] : sdyn[3 * vd], v1 = vd < 0 ? X->tl[e].v[1] : sdyn[3 * vd + 1], v2 = vd < 0 ? X->tl[e].v[2] : sdyn[3 * vd + 2];
            const double z = si < 0 ? 1.0 : sSv[si];
            double p0 = v0, p1 = v1, p2 = v2;
            if (moff >= 0) {
                const double* D = sR + moff;
                p0 = D[0] * v0 + D[1] * v1 + D[2] * v2; p1 = D[3] * v0 + D[4] * v1 + D[5] * v2; p2 = D[6] * v0 + D[7] * v1 + D[8] * v2;
            }
            s0 += z * p0; s1 += z * p1; s2 += z * p2;
        }
        sDp[3 * t] = s0; sDp[3 * t + 1] = s1; sDp[3 * t + 2] = s2;
    }
    wave_lds_sync();
}

// T = L^-1 of the lower-triangular block sL [28][28] (row-major; sr[k] = 1 / L[k][k]) by forward substitution, one column per lane: lanes 0..27
// and 28..55 both hold columns 0..27 in t (each half takes every second row of the products that follow), lanes 56..63 shadow columns 0..7 and
// store nothing.  T goes to sT, row-major; ends with a wave_lds_sync.
__device__ __forceinline__ void wave_tri_inverse(const double* sL, const double* sr, double* sT, double (&t)[NU], int lane) {
    const int c = lane % NU, hh = lane / NU;
#pragma unroll
    for (int i = 0; i < NU; i++) {
        double s = i == c ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) s = fma(-sL[i * NU + k], t[k], s);
        t[i] = s * sr[i];
    }
    if (hh == 0) {
#pragma unroll
        for (int k = 0; k < NU; k++) sT[k * NU + c] = t[k];
    }
    wave_lds_sync();
}
// (T^T T)[a][c] = sum_k T[k][a] T[k][c] after wave_tri_inverse, lanes 0..55: the same products in the same order for [a][c] and [c][a] --
// bit-symmetric.  O: the block [28][28], row-major; SCALED: every entry times `scale` (symmetric still).
template <bool SCALED>
__device__ __forceinline__ void wave_ttt(const double* sT, const double (&t)[NU], double* O, double scale, int lane) {
    const int c = lane % NU, hh = lane / NU;
    for (int a = hh; a < NU; a += 2) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NU; k++) s = fma(sT[k * NU + a], t[k], s);
        O[a * NU + c] = SCALED ? scale * s : s;
    }
}

// ---- pre-pass, one wave per frame.  Column n of the factor: block 0 = L(n,n), block i = L(n+i,n), [row * 28 + col].  `recip` != 0: the
// diagonal of block 0 holds 1 / L[k][k] (Lbuf as k_lm_step writes it), else L[k][k] itself (the plain layout of cpe_eval_lm_step).  Both
// forms go through the same arithmetic, r = 1 / d with d the true diagonal, so a factor exported by cpe_covariance and handed back to
// cpe_band_inverse gives the same bits.  Output column n of Gbuf, same shape: block 0 = T^T T, block i = G_i (zero where n + i >= N).
template <int PB, bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_cov_prep(const SeqState* __restrict__ st, const double* __restrict__ Lsrc, double* __restrict__ Gbuf,
                                                   int NS, int recip, RaggedArgs rg = RaggedArgs{}) {
    constexpr int RING = PB + 1, BB = NU * NU;
    __shared__ double sL[RING * BB];
    __shared__ double sT[BB];
    __shared__ double sr[NU];
    const int lane = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)NS), n = (int)(blockIdx.x % (unsigned)NS);
    int N = NS;
    if constexpr (RAGGED) N = rg.seq[b].y;
    if (n >= N || !cov_seq_ok(st, b)) return;                 // uniform
    const size_t col = ((size_t)b * NS + n) * (size_t)(RING * BB);
    const double* Lc = Lsrc + col;
    double* Gc = Gbuf + col;
    for (int t = lane; t < RING * BB; t += WAVE) sL[t] = Lc[t];
    wave_lds_sync();
    if (lane < NU) {
        const double x = sL[lane * NU + lane];
        const double d = recip ? 1.0 / x : x;
        sr[lane] = 1.0 / d;
    }
    wave_lds_sync();
    double t[NU];
    wave_tri_inverse(sL, sr, sT, t, lane);
    const int c = lane % NU, hh = lane / NU;
    if (hh < 2) {
        wave_ttt<false>(sT, t, Gc, 1.0, lane);
#pragma unroll
        for (int i = 1; i <= PB; i++) {
            const double* Li = sL + i * BB;
            const bool in = n + i < N;
            for (int r = hh; r < NU; r += 2) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < NU; k++) s = fma(Li[r * NU + k], t[k], s);
                Gc[i * BB + r * NU + c] = in ? s : 0.0;
            }
        }
    }
}

// ---- the serial sweep, one 256-thread workgroup per sequence, columns N-1 .. 0.  LDS: the window of Sigma as a ring over the frame index
// mod PB + 1 (blk_slot: PB (PB + 1) / 2 blocks of the frames n+1 .. n+PB plus the PB + 1 blocks of column n under construction -- 6 + 4 at
// PB = 3, 10 + 5 at PB = 4), the operands T^T T | G_1 .. G_PB of the column, and PB partial products of the diagonal block; blocks are
// [28][LDB] doubles as k_lm_step keeps them.  The operands of column n-1 are requested before column n is computed (cov_prefetch / cov_stage).
// Block products by tile4_fma: 49 PB tile jobs for the off-diagonal blocks, one per thread, each the whole sum over k and m in that order;
// then 28 PB jobs (lower_tile, k) for G_k^T Sigma(n+k,n), summed over k in order by the thread that stores the element and its mirror --
// Sigma(n,n) is exactly symmetric.
template <int PB, bool RAGGED = false>
__global__ __launch_bounds__(COV_THREADS, 1) void k_lm_selinv(const SeqState* __restrict__ st, const double* __restrict__ Gbuf,
                                                              double* __restrict__ cov_diag, double* __restrict__ cov_off, int NS,
                                                              RaggedArgs rg = RaggedArgs{}) {
    constexpr int RING = PB + 1, NW = RING * (RING + 1) / 2, BB = NU * NU, COLD = RING * BB;
    constexpr int TPB = (NU / 4) * (NU / 4);                 // 49 tiles of a block
    constexpr int LTT = (NU / 4) * (NU / 4 + 1) / 2;         // 28 tiles of its lower triangle
    static_assert(PB >= 3 && PB <= 4 && TPB * PB <= COV_THREADS && LTT * PB <= COV_THREADS, "one tile job per thread");
    __shared__ double Wn[NW * BLK];
    __shared__ double Gs[RING * BLK];
    __shared__ double Ps[PB * BLK];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    int N = NS;
    if constexpr (RAGGED) N = rg.seq[b].y;
    if (!cov_seq_ok(st, b)) return;                          // uniform: the outputs of such a sequence stay zero
    const double* Gb = Gbuf + (size_t)b * NS * COLD;
    double* cd = cov_diag + (size_t)b * NS * BB;
    double* co = cov_off ? cov_off + (size_t)b * NS * (size_t)(PB * BB) : nullptr;

    for (int t = tid; t < NW * BLK; t += COV_THREADS) Wn[t] = 0.0;      // frames past the end: Sigma = 0
    double pf[(COLD + COV_THREADS - 1) / COV_THREADS];
    auto fetch = [&](int n) { cov_prefetch<COLD>(pf, Gb + (size_t)n * COLD, tid); };
    fetch(N - 1);
    // this thread's jobs
    const int ja_i = 1 + tid / TPB, ja_t = tid % TPB, ja_r = 4 * (ja_t / (NU / 4)), ja_c = 4 * (ja_t % (NU / 4));
    const bool ja_on = tid < TPB * PB;
    const int jb_k = 1 + tid / LTT, jb_t = tid % LTT;
    int jb_tr, jb_tc; lower_tile(jb_t, jb_tr, jb_tc);
    const int jb_r = 4 * jb_tr, jb_c = 4 * jb_tc;
    const bool jb_on = tid < LTT * PB;

    for (int n = N - 1; n >= 0; n--) {
        cov_stage<COLD>(pf, Gs, tid);
        fetch(n > 0 ? n - 1 : 0);
        lds_barrier();
        // ---- off-diagonal blocks: Sigma(n+i,n) = - sum_k Sigma(n+i,n+k) G_k
        if (ja_on) {
            double acc[4][4];
            tile4_zero(acc);
#pragma unroll
            for (int k = 1; k <= PB; k++) {
                // Sigma(n+i,n+k) is stored as the block of (larger frame, smaller frame): read as it stands (k <= i) or transposed
                const bool tr = k > ja_i;
                const int hi = tr ? k : ja_i, lo = tr ? ja_i : k;
                const double* A = Wn + blk_slot<RING>(n + hi, n + lo) * BLK + ja_r * (tr ? 1 : LDB);
                const int sx = tr ? 1 : LDB, sm = tr ? LDB : 1;
                const double* G = Gs + k * BLK + ja_c;
                tile4_fma<true, 4>(acc, A, sx, sm, G, LDB, 0, NU);
            }
            tile4_store(acc, Wn + blk_slot<RING>(n + ja_i, n) * BLK + ja_r * LDB + ja_c, LDB);
            if (co) tile4_store(acc, co + ((size_t)n * PB + (ja_i - 1)) * BB + ja_r * NU + ja_c, NU);
        }
        lds_barrier();
        // ---- diagonal block, part k: G_k^T Sigma(n+k,n) on the tiles of the lower triangle
        if (jb_on) {
            double acc[4][4];
            tile4_zero(acc);
            const double* G = Gs + jb_k * BLK + jb_r;
            const double* S = Wn + blk_slot<RING>(n + jb_k, n) * BLK + jb_c;
            tile4_fma<false, 4>(acc, G, 1, LDB, S, LDB, 0, NU);
            tile4_store(acc, Ps + (jb_k - 1) * BLK + jb_r * LDB + jb_c, LDB);
        }
        lds_barrier();
        // ---- Sigma(n,n) = T^T T - (part 1 + part 2 + ...), from its lower triangle, mirrored
        {
            double* D = Wn + blk_slot<RING>(n, n) * BLK;
            double* Dg = cd + (size_t)n * BB;
            for (int e = tid; e < BB; e += COV_THREADS) {
                const int a = e / NU, c = e - a * NU;
                if (c <= a) {
                    double s = Ps[a * LDB + c];
#pragma unroll
                    for (int k = 1; k < PB; k++) s += Ps[k * BLK + a * LDB + c];
                    const double v = Gs[a * LDB + c] - s;
                    D[a * LDB + c] = v; D[c * LDB + a] = v;
                    Dg[a * NU + c] = v; Dg[c * NU + a] = v;
                }
            }
        }
        lds_barrier();          // the column is complete; Gs and Ps are free for the next one
    }
}

// ---- marker covariance, one wave per frame: cov_pos[l] = P_l Sigma(n,n) P_l^T with P_l = d p_l / d u, the reduced marker columns Dp of
// k_frame_normal (same tables, same state phases, same order of the terms: wave_point_columns).  State: the current buffer of the sequence, as
// k_frame_normal left it.
// dynamic LDS: state | sin / cos | leg sin / cos | trunk R, dR | dynamic vectors | S rows | Dp | Sigma(n,n) | first term of every item (int)
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_marker_cov(const DevModel* __restrict__ M, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                     const double* __restrict__ qbuf, const double* __restrict__ cov_diag,
                                                     double* __restrict__ cov_pos, RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs)) return;
    M += fs.model;
    const int b = fs.b;
    if (!cov_seq_ok(st, b)) return;
    const size_t f = (size_t)b * N + fs.n;
    const int buf = st[b].cur;
    const int nq = M->nq, nl = M->nl, L = M->L, nrev = M->nrev, ns = M->ns, svn = M->sv_n, mct = M->mc_total;
    double* sq = smem;
    double* sal = sq + nq;
    double* ssc = sal + nrev;
    double* ssa = ssc + 6 * nl;
    double* sR = ssa + 2 * nrev;
    double* sdyn = sR + 36 * M->n_trunk;
    double* sSv = sdyn + 3 * svn;
    double* sDp = sSv + CPE_MAX_SCOL * M->n_srow;
    double* sSig = sDp + 3 * mct;
    int* sBeg = reinterpret_cast<int*>(sSig + NU * NU);       // first term of every item of the flat list

    const int4 fw = *reinterpret_cast<const int4*>(M->fn_lane[lane]);
    const int hj_n = M->hj_n, hk_n = M->hk_n;
    const int2 hkw = *reinterpret_cast<const int2*>(M->hk_w[lane]);
    const double* stf = qbuf + (size_t)buf * n_frames * ns + f * ns;
    for (int t = lane; t < ns; t += WAVE) sq[t] = stf[t];
    for (int t = lane; t < NU * NU; t += WAVE) sSig[t] = cov_diag[f * (size_t)(NU * NU) + t];
    wave_lds_sync();
    // ---- the state phases (cpe_kernels.hip); the legs' Euler angles are not rebuilt: the state holds them
    wave_state_sincos(M, sq, sal, ssc, ssa, nrev, lane);
    wave_lds_sync();
    wave_tail_roll(sq, ssc, hj_n, fw.x, lane);
    wave_trunk_rotations(M, ssc, sR, fw.y, lane);
    wave_lds_sync();
    wave_hooke_srows(sR, sSv, hk_n, hkw, lane);
    wave_point_columns(M, ssa, sR, sSv, sdyn, sDp, sBeg, lane);
    // cov_pos[l][a][c] = sum_i sum_j Dp_i[a] Sigma[col_i][col_j] Dp_j[c] over the marker's columns; lane = (marker, entry of the lower
    // triangle), the mirror is stored with it
    for (int t = lane; t < 6 * L; t += WAVE) {
        const int l = t / 6;
        int a, c; lower_entry3(t - 6 * l, a, c);
        const int off = M->mcol_off[l], nc = M->mcol_n[l];
        double s = 0.0;
        for (int i = 0; i < nc; i++) {
            const int ci = M->mcol[l][i];
            double w = 0.0;
            for (int j = 0; j < nc; j++) w = fma(sSig[ci * NU + M->mcol[l][j]], sDp[3 * (off + j) + c], w);
            s = fma(sDp[3 * (off + i) + a], w, s);
        }
        double* o = cov_pos + (f * (size_t)L + l) * 9;
        o[3 * a + c] = s; o[3 * c + a] = s;
    }
}

// ---- the factor cpe_covariance used, in the plain layout of cpe_eval_lm_step (true diagonal); zero for a sequence without a factor and past
// a sequence's own frames.  One workgroup per frame.
template <bool RAGGED = false>
__global__ __launch_bounds__(COV_THREADS) void k_cov_export(const SeqState* __restrict__ st, const double* __restrict__ Lbuf, double* __restrict__ L,
                                                            int NS, int cold, RaggedArgs rg = RaggedArgs{}) {
    const int b = (int)(blockIdx.x / (unsigned)NS), n = (int)(blockIdx.x % (unsigned)NS);
    int N = NS;
    if constexpr (RAGGED) N = rg.seq[b].y;
    const bool ok = n < N && cov_seq_ok(st, b);
    const size_t col = (size_t)blockIdx.x * (size_t)cold;
    for (int t = threadIdx.x; t < cold; t += COV_THREADS) {
        double v = 0.0;
        if (ok) { v = Lbuf[col + t]; if (t < NU * NU && t / NU == t % NU) v = 1.0 / v; }
        L[col + t] = v;
    }
}

// ---- columns of Sigma beyond the band (include/cpe.h, cpe_covariance_columns; DESIGN.md 2 "What is spanned").  L^T Sigma = L^-1 is lower
// triangular, so above an anchor frame a the rows of L^T give
//     Sigma(n,a) = - sum_k G_k(n)^T Sigma(n+k,a)                      k = 1..PB,   n = a-PB-1 .. 0
// with k_cov_prep's G_k: the sweep's recurrence continued upward, seeded by the band blocks Sigma(a-i,a) = Sigma(a,a-i)^T.  One 256-thread workgroup
// per (sequence, anchor slot), the rows in series.  LDS: the last PB blocks of the column as a ring over the frame index mod PB, the operands
// G_1 .. G_PB of the row, and PB partial products; blocks are [28][LDB] doubles.  Operands and block products as in k_lm_selinv: 49 PB jobs
// (tile, k), one per thread, then the thread that stores an element sums its PB parts in the order of k.  No atomics; a column depends on nothing but its own sequence and anchor.  The rows n > a are not
// written (the caller zeroes the output); the rows a-PB .. a are copies of the band.
template <int PB>
__global__ __launch_bounds__(COV_THREADS, 1) void k_cov_columns(const double* __restrict__ Gbuf, const double* __restrict__ cov_diag,
                                                                const double* __restrict__ cov_off, const int* __restrict__ anchors,
                                                                double* __restrict__ cols, int NS, int K) {
    constexpr int RING = PB + 1, BB = NU * NU, COLD = RING * BB, GN = PB * BB;
    constexpr int TPB = (NU / 4) * (NU / 4);                 // 49 tiles of a block
    static_assert(PB >= 3 && PB <= 4 && TPB * PB <= COV_THREADS, "one tile job per thread");
    __shared__ double Xs[PB * BLK];
    __shared__ double Gs[PB * BLK];
    __shared__ double Ps[PB * BLK];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)K);
    const int a = anchors[blockIdx.x];
    if (a < 0 || a >= NS) return;                            // uniform: an unused slot stays zero
    const double* Gb = Gbuf + (size_t)b * NS * COLD;
    const double* cd = cov_diag + (size_t)b * NS * BB;
    const double* co = cov_off + (size_t)b * NS * (size_t)(PB * BB);
    double* out = cols + (size_t)blockIdx.x * NS * BB;

    // ---- the rows inside the band: Sigma(a,a), and Sigma(a-i,a) -- into the ring as well
    for (int e = tid; e < BB; e += COV_THREADS) out[(size_t)a * BB + e] = cd[(size_t)a * BB + e];
#pragma unroll
    for (int i = 1; i <= PB; i++) {
        const int n = a - i;
        if (n < 0) break;
        double* X = Xs + (n % PB) * BLK;
        for (int e = tid; e < BB; e += COV_THREADS) {
            const int r = e / NU, c = e - r * NU;
            const double v = band_entry(cd, co, PB, n, a, r, c);
            X[r * LDB + c] = v;
            out[(size_t)n * BB + e] = v;
        }
    }
    const int n0 = a - PB - 1;
    if (n0 < 0) return;                                      // uniform
    double pf[(GN + COV_THREADS - 1) / COV_THREADS];
    auto fetch = [&](int n) { cov_prefetch<GN>(pf, Gb + (size_t)n * COLD + BB, tid); };        // G_1 .. G_PB of row n
    fetch(n0);
    const int jk = tid / TPB, jt = tid % TPB, jr = 4 * (jt / (NU / 4)), jc = 4 * (jt % (NU / 4));
    const bool jon = tid < TPB * PB;

    for (int n = n0; n >= 0; n--) {
        cov_stage<GN>(pf, Gs, tid);
        fetch(n > 0 ? n - 1 : 0);
        lds_barrier();          // the operands of this row, and the block the row before it left in the ring
        // ---- part k: G_k^T Sigma(n+k,a)
        if (jon) {
            double acc[4][4];
            tile4_zero(acc);
            const double* G = Gs + jk * BLK + jr;
            const double* X = Xs + ((n + 1 + jk) % PB) * BLK + jc;
            tile4_fma<false, 4>(acc, G, 1, LDB, X, LDB, 0, NU);
            tile4_store(acc, Ps + jk * BLK + jr * LDB + jc, LDB);
        }
        lds_barrier();          // the parts are complete, and Sigma(n+PB,a) has been read for the last time: row n takes its place in the ring
        {
            double* X = Xs + (n % PB) * BLK;
            double* Og = out + (size_t)n * BB;
            for (int e = tid; e < BB; e += COV_THREADS) {
                const int r = e / NU, c = e - r * NU;
                double s = Ps[r * LDB + c];
#pragma unroll
                for (int k = 1; k < PB; k++) s += Ps[k * BLK + r * LDB + c];
                X[r * LDB + c] = -s;
                Og[e] = -s;
            }
        }
        // (no barrier here: the next row's operands go to Gs, which nobody reads any more, and its first barrier orders the ring)
    }
}
