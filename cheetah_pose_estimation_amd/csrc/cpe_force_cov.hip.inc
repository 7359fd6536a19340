// cpe_force_cov.hip.inc -- posterior covariance of the node forces of the physics-based estimate (include/cpe.h, cpe_covariance_kinetic;
// DESIGN.md 2b "What is inverted").  The band k_lm_step<3, 2> factors is the Schur complement of the joint Gauss-Newton matrix over
// (coordinates, node forces), so the force block of its inverse is local to the node:
//     cov_f(n) = M^-1 + S W S^T,   S = M^-1 H_fu
// with M the node's force matrix as k_dyn_schur eliminated it (kin_force_matrix) and W the 84 x 84 covariance of the coordinates of the frames
// (n, n-1, n-2), all of it inside the band k_lm_selinv returns.  With M = L L^T and Y = L^-1 H_fu (kin_partial_cholesky, H_uf riding along as in
// k_dyn_schur: the same factor, bit for bit)
//     cov_f = L^-T (I + Y W Y^T) L^-1.
// One 256-thread workgroup per node n >= 2.  No atomics; every sum has a fixed order; the result is stored from its lower triangle with the
// mirror, so it is exactly symmetric.
// dynamic LDS (141 KB: one workgroup per CU -- the kernel runs once per call, not per LM iteration):
//   Mx [na + 84][KIN_MS]   L (rows < na) | Y^T (rows na + u)                      ->  P = C L^-1 from row KIN_NA_MAX on, once Y is dead
//   dg [KIN_LS]            1 / L_jj
//   Zt [84][KIN_MS]        Z^T, Z = Y W                                           ->  L^-1 [na][KIN_MS]
//   Cs [KIN_NA_MAX][KIN_MS] a 28-row panel of W [28][84] (W is streamed by panel) ->  C = I + Z Y^T
#define FC_MX ((KIN_NA_MAX + KIN_NC3) * KIN_MS)
#define FC_ZT (KIN_NC3 * KIN_MS)
#define FC_CS (KIN_NA_MAX * KIN_MS)
#define FC_DOUBLES (FC_MX + KIN_LS + FC_ZT + FC_CS)
#define FC_TA (KIN_NA_MAX / 4)            // 4 x 4 tiles along the forces
#define FC_TV (KIN_NC3 / 4)               // ... along the coordinates
#define FC_PB 3                           // half-bandwidth of the band k_lm_step<3, 2> factors
static_assert(KIN_NA_MAX % 4 == 0 && KIN_NC3 % 4 == 0 && FC_TA * FC_TV <= 2 * KIN_THREADS && FC_TA * FC_TA <= KIN_THREADS, "tiling of k_force_cov");
static_assert(CPE_NX * KIN_NC3 <= FC_CS && KIN_NA_MAX * KIN_MS <= FC_ZT && KIN_NA_MAX <= KIN_LS, "LDS regions of k_force_cov");

// cov_diag / cov_off: the band of Sigma as k_lm_selinv wrote it (band_entry, half-bandwidth FC_PB).  cov_f [F][KIN_LS][KIN_LS], f_out
// [F][KIN_LS] and meta_out [F][KIN_LS + 1] (each may be null): the node's forces and (count, indices of its free forces, zeros, Newton iterations).
// bad [B]: set to 1 where a node's M has no Cholesky factor (the host clears that sequence's outputs).
// RAGGED (cpe_covariance_kinetic_ragged): N = rg.nmax; sequence b has its own frame count and its own entry of K, by the table rg.
template <bool RAGGED = false>
__global__ __launch_bounds__(KIN_THREADS, 1) void k_force_cov(const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                              const double* __restrict__ pieces, const int* __restrict__ pmeta,
                                                              const double* __restrict__ fbuf, const double* __restrict__ kmu,
                                                              const int32_t* __restrict__ stance, const double* __restrict__ cov_diag,
                                                              const double* __restrict__ cov_off, double* __restrict__ cov_f,
                                                              double* __restrict__ f_out, int32_t* __restrict__ meta_out, int* __restrict__ bad,
                                                              RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    __shared__ int flag;
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)N), n = (int)(blockIdx.x % (unsigned)N);
    if constexpr (RAGGED) {
        const int2 rs = rg.seq[b];
        if (n >= rs.y) return;                                // a frame past the sequence's own
        K += rs.x;
    }
    if (n < 2 || !cov_seq_ok(st, b)) return;                  // uniform; no node, or no factor of the band: the outputs stay zero
    const size_t f_ = (size_t)b * N + n;
    const SeqState Sq = st[b];
    const size_t fo = (size_t)Sq.cur * n_frames + f_;
    const int na = pmeta[fo * (KIN_LS + 1)];
    if (na < 0 || na > KIN_NA_MAX) return;                    // (k_dyn_eval never writes such a count)
    const double* pc = pieces + fo * (size_t)KIN_PIECE;
    const double* Hfu = pc + KIN_NC3 * KIN_NC3; const double* Hff = Hfu + KIN_LS * KIN_NC3;
    double* Mx = smem; double* dg = Mx + FC_MX; double* Zt = dg + KIN_LS; double* Cs = Zt + FC_ZT;

    if (f_out && tid < KIN_LS) f_out[f_ * KIN_LS + tid] = fbuf[fo * KIN_LS + tid];
    if (meta_out && tid <= KIN_LS) meta_out[f_ * (KIN_LS + 1) + tid] = tid <= na || tid == KIN_LS ? pmeta[fo * (KIN_LS + 1) + tid] : 0;
    // entries the factorisation does not write (the upper triangle of L, columns >= na of Y^T) are read as zeros by the tiles below
    for (int t = tid; t < FC_MX; t += KIN_THREADS) Mx[t] = 0.0;
    __syncthreads();
    kin_force_matrix(K, Sq, f_, fo, na, Hfu, Hff, fbuf, kmu, stance, Mx, tid);
    if (!kin_partial_cholesky<9>(Mx, na + KIN_NC3, na, na, KIN_MS, dg, tid, &flag)) {          // uniform
        if (tid == 0) bad[b] = 1;
        return;
    }
    if (!cov_f) return;                                       // (only the status was asked for)
    const int nta = (na + 3) >> 2;                            // tiles along the forces that hold an unknown
    const double* Yt = Mx + na * KIN_MS;                      // Y^T [u][a]

    // ---- Z = Y W, W streamed in three panels of 28 rows (the frame n - p); two tiles (4 forces x 4 coordinates) per thread, each the whole
    // sum over u = 0 .. 83 in that order
    double z[2][4][4];
    tile4_zero(z[0]); tile4_zero(z[1]);
    int za[2], zv[2]; bool zon[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int t = tid + KIN_THREADS * s;
        zon[s] = t < nta * FC_TV;
        za[s] = zon[s] ? 4 * (t / FC_TV) : 0; zv[s] = zon[s] ? 4 * (t % FC_TV) : 0;
    }
    const double* cd = cov_diag + (size_t)b * N * (CPE_NX * CPE_NX);                  // the sequence's band
    const double* co = cov_off + (size_t)b * N * (FC_PB * CPE_NX * CPE_NX);
    for (int p = 0; p < 3; p++) {
        // W[28 p + i][28 q + j] = Sigma(n - p, n - q)[i][j]
        for (int t = tid; t < CPE_NX * KIN_NC3; t += KIN_THREADS) {
            const int i = t / KIN_NC3, v = t - i * KIN_NC3, q = v / CPE_NX, j = v - q * CPE_NX;
            Cs[t] = band_entry(cd, co, FC_PB, n - p, n - q, i, j);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; s++)
            tile4_fma<false, 4>(z[s], Yt + (size_t)(CPE_NX * p) * KIN_MS + za[s], 1, KIN_MS, Cs + zv[s], KIN_NC3, 0, CPE_NX);
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < 2; s++)
        if (zon[s]) {
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) Zt[(zv[s] + j) * KIN_MS + za[s] + i] = z[s][i][j];
        }
    __syncthreads();

    // ---- C = I + Z Y^T on the tiles of the lower triangle, mirrored (rows and columns past na: zero)
    if (tid < nta * (nta + 1) / 2) {
        int ti, tj; lower_tile(tid, ti, tj);
        double c[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) c[i][j] = ti == tj && i == j && 4 * ti + i < na ? 1.0 : 0.0;
        tile4_fma<false, 4>(c, Zt + 4 * ti, 1, KIN_MS, Yt + 4 * tj, KIN_MS, 0, KIN_NC3);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ti != tj || j <= i) { Cs[(4 * ti + i) * KIN_MS + 4 * tj + j] = c[i][j]; Cs[(4 * tj + j) * KIN_MS + 4 * ti + i] = c[i][j]; }
    }
    __syncthreads();          // Z is dead: its area takes L^-1

    // ---- T = L^-1 by forward substitution, one column per thread (T[i][c], i = c .. na - 1; the rest of the area zero)
    double* Ti = Zt;
    for (int t = tid; t < KIN_NA_MAX * KIN_MS; t += KIN_THREADS) Ti[t] = 0.0;
    __syncthreads();
    if (tid < na) {
        const int c = tid;
        for (int i = c; i < na; i++) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; k++) s = fma(-Mx[i * KIN_MS + k], Ti[k * KIN_MS + c], s);
            Ti[i * KIN_MS + c] = s * dg[i];
        }
    }
    __syncthreads();          // Y is dead too: P goes behind the factor

    // ---- P = C T: one tile per thread, the sum over k from the tile's first column on (T[k][c] = 0 for k < c)
    double* Ps = Mx + KIN_NA_MAX * KIN_MS;
    if (tid < nta * nta) {
        const int ti = tid / nta, tj = tid - ti * nta;
        double c[4][4];
        tile4_zero(c);
        tile4_fma<false, 0>(c, Cs + (4 * ti) * KIN_MS, KIN_MS, 1, Ti + 4 * tj, KIN_MS, 4 * tj, na);
        tile4_store(c, Ps + (4 * ti) * KIN_MS + 4 * tj, KIN_MS);
    }
    __syncthreads();

    // ---- cov_f = T^T P on the tiles of the lower triangle (T[k][a] = 0 for k < a), stored with the mirror
    if (tid < nta * (nta + 1) / 2) {
        int ti, tj; lower_tile(tid, ti, tj);
        double c[4][4];
        tile4_zero(c);
        tile4_fma<false, 0>(c, Ti + 4 * ti, 1, KIN_MS, Ps + 4 * tj, KIN_MS, 4 * ti, na);
        double* O = cov_f + f_ * (size_t)(KIN_LS * KIN_LS);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int a = 4 * ti + i, e = 4 * tj + j;
                if (a < na && e < na && (ti != tj || j <= i)) { O[a * KIN_LS + e] = c[i][j]; O[e * KIN_LS + a] = c[i][j]; }
            }
    }
}
