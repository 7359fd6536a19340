// cpe_force_sample.hip.inc -- draws of the node forces of the physics-based estimate (include/cpe.h, cpe_force_samples; DESIGN.md 2b "What is
// sampled (forces)").  The band k_lm_step<3, 2> factors is the Schur complement of the joint Gauss-Newton matrix over (coordinates, node forces).
// Ordered as (forces of every node, coordinates) that joint matrix has the lower Cholesky factor
//     G = [[ blockdiag(C_n), 0 ], [ H_uf C_n^-T, L ]],        M_n = C_n C_n^T,  A = L L^T,
// so the back substitution G^T (df, du) = (zeta, z) with z, zeta ~ N(0, I) is a draw of the joint Laplace posterior: L^T du = z is k_band_sample's,
// and per node n >= 2
//     df_n = C_n^-T (zeta_n - Y_n w_n),        Y_n = C_n^-1 H_fu(n),   w_n = (du_n, du_{n-1}, du_{n-2})
// is this kernel's.  C_n and Y_n^T come out of kin_force_matrix + kin_partial_cholesky<9> exactly as in k_force_cov (the same factor, bit for bit).
// One 256-thread workgroup per node; the factor is formed once and serves all S samples in passes of FS_CHUNK = 256, THREAD = SAMPLE (as
// k_band_sample has lane = sample): the rows of Y^T and of C are wave-uniform LDS reads (broadcasts), t[] lives in registers under compile-time
// indices only (loops unrolled to KIN_NA_MAX under the uniform predicate a < na -- a runtime index would put it into scratch), so there is no
// cross-lane traffic and no barrier after the factor.  Order of every sum: t[a] = zeta[a], then t[a] = fma(-Y^T[u][a], w[u], t[a]) for
// u = 0 .. 83 ascending (u = 28 p + i: coordinate i of frame n - p); then C^T x = t from row na - 1 down: x[m] = t[m] dg[m],
// t[k] = fma(-C[m][k], x[m], t[k]) for k = m - 1 .. 0.  Nothing depends on the lane, the pass, S or the batch: a sample's forces are bit-equal
// whatever S, its slot and the batch.  No atomics.
// dynamic LDS (70.8 KB): Mx [KIN_NA_MAX + 84][KIN_MS] | dg [KIN_LS]; static: the node's forces, its index list and the mask of its unknowns.
#define FS_CHUNK KIN_THREADS              // samples per workgroup pass
#define FS_DOUBLES ((KIN_NA_MAX + KIN_NC3) * KIN_MS + KIN_LS)
static_assert(KIN_NC3 % 4 == 0, "k_force_sample reads w four at a time");

// du [B][S][N][28], zeta [B][S][N][KIN_LS] (compact order of the node's meta; entries past the count are not read; null = zeros: the conditional
// mean f - S w), f_s [B][S][N][KIN_LS] in f's layout: f + df on the node's unknowns, f elsewhere; it arrives zeroed (the nodes 0, 1, the frames
// past a sequence's own and a sequence without a band factor are not written).  f_out [F][KIN_LS], meta_out [F][KIN_LS + 1] (each may be null)
// and bad [B]: as in k_force_cov.
template <bool RAGGED = false>
__global__ __launch_bounds__(KIN_THREADS, 1) void k_force_sample(const DevKin* __restrict__ K, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                                 const double* __restrict__ pieces, const int* __restrict__ pmeta,
                                                                 const double* __restrict__ fbuf, const double* __restrict__ kmu,
                                                                 const int32_t* __restrict__ stance, int S, const double* __restrict__ du,
                                                                 const double* __restrict__ zeta, double* __restrict__ f_s,
                                                                 double* __restrict__ f_out, int32_t* __restrict__ meta_out, int* __restrict__ bad,
                                                                 RaggedArgs rg = RaggedArgs{}) {
    extern __shared__ double smem[];
    __shared__ int flag;
    __shared__ double fv[KIN_LS];
    __shared__ int idx[KIN_LS], unk[KIN_LS];
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
    double* Mx = smem; double* dg = Mx + (KIN_NA_MAX + KIN_NC3) * KIN_MS;

    if (tid < KIN_LS) {
        const double v = fbuf[fo * KIN_LS + tid];
        fv[tid] = v; unk[tid] = 0;
        idx[tid] = tid < na ? pmeta[fo * (KIN_LS + 1) + 1 + tid] & (KIN_LS - 1) : 0;      // (an index of the evaluation is below KIN_LS; masked: it addresses LDS and f_s)
        if (f_out) f_out[f_ * KIN_LS + tid] = v;
    }
    if (meta_out && tid <= KIN_LS) meta_out[f_ * (KIN_LS + 1) + tid] = tid <= na || tid == KIN_LS ? pmeta[fo * (KIN_LS + 1) + tid] : 0;
    // entries the factorisation does not write (the upper triangle of C, columns >= na of Y^T) are read as zeros below
    for (int t = tid; t < (KIN_NA_MAX + KIN_NC3) * KIN_MS; t += KIN_THREADS) Mx[t] = 0.0;
    __syncthreads();
    if (tid < na) unk[idx[tid]] = 1;
    kin_force_matrix(K, Sq, f_, fo, na, Hfu, Hff, fbuf, kmu, stance, Mx, tid);
    if (!kin_partial_cholesky<9>(Mx, na + KIN_NC3, na, na, KIN_MS, dg, tid, &flag)) {          // uniform
        if (tid == 0) bad[b] = 1;
        return;
    }
    const double* Yt = Mx + na * KIN_MS;                      // Y^T [u][a]

    for (int s = tid; s < S; s += FS_CHUNK) {                 // no barrier below: a thread past S in the last pass simply has no sample
        asm volatile("" ::: "memory");                        // (the LDS reads below stay in the pass: hoisted, the wave-uniform ones pile up in scalar registers)
        const size_t sf = ((size_t)b * S + s) * N + n;       // the sample's frame n
        const double* wp = du + sf * CPE_NX;                  // frame n - p: wp - p * CPE_NX
        double t[KIN_NA_MAX];
        if (zeta) {
            const double* zp = zeta + sf * KIN_LS;
#pragma unroll
            for (int a = 0; a < KIN_NA_MAX; a++) t[a] = a < na ? zp[a] : 0.0;
        } else {
#pragma unroll
            for (int a = 0; a < KIN_NA_MAX; a++) t[a] = 0.0;
        }
        // t -= Y w, four u at a time; the lane's next four w are requested before the products of these four
        double wn[4];
#pragma unroll
        for (int j = 0; j < 4; j++) wn[j] = wp[j];
        for (int u0 = 0; u0 < KIN_NC3; u0 += 4) {
            double wv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) wv[j] = wn[j];
            if (u0 + 4 < KIN_NC3) {
                const int u1 = u0 + 4, p = u1 / CPE_NX, i = u1 - p * CPE_NX;      // (CPE_NX % 4 == 0: the four stay in one frame)
#pragma unroll
                for (int j = 0; j < 4; j++) wn[j] = wp[i + j - p * CPE_NX];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double* row = Yt + (u0 + j) * KIN_MS;
#pragma unroll
                for (int a = 0; a < KIN_NA_MAX; a++) t[a] = fma(-row[a], wv[j], t[a]);          // (columns >= na of Y^T are zeros)
            }
        }
        // C^T x = t from row na - 1 down.  (The factor is read relative to a base the compiler does not know: with the absolute LDS addresses of
        // the ~1800 entries as constants it keeps them in scalar registers and spills a thousand of those; so they are immediate offsets.)
        int base = 0;
        asm volatile("" : "+v"(base));
        const double* Cb = Mx + base; const double* dgb = dg + base;
#pragma unroll
        for (int m = KIN_NA_MAX - 1; m >= 0; m--) {
            if (m < na) {                                     // uniform
                const double x = t[m] * dgb[m];
                t[m] = x;
                const double* row = Cb + m * KIN_MS;
#pragma unroll
                for (int k = m - 1; k >= 0; k--) t[k] = fma(-row[k], x, t[k]);
            }
        }
        // f_s = f + df through the node's indices; every entry of the row is written once
        double* out = f_s + sf * KIN_LS;
#pragma unroll
        for (int j = 0; j < KIN_LS; j++) if (!unk[j]) out[j] = fv[j];          // uniform
#pragma unroll
        for (int a = 0; a < KIN_NA_MAX; a++) if (a < na) out[idx[a]] = fv[idx[a]] + t[a];
    }
}
