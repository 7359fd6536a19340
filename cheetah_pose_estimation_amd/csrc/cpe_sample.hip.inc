// cpe_sample.hip.inc -- draws from the posterior of the kinematic estimate (include/cpe.h, cpe_band_sample / cpe_posterior_samples; DESIGN.md 2
// "What is sampled").  With z ~ N(0, I) the solution of L^T du = z has covariance L^-T L^-1 = Sigma -- the whole matrix, not only its band.
// Two kernels: k_band_sample, the banded back substitution with many right-hand sides per sequence, and k_sample_state, which adds a draw to the
// cold-start state and runs the state phases; k_finalize (cpe_solver.hip.inc) then turns that state into Euler q and marker positions.

// ---- L^T du = z for S right-hand sides per sequence, newest frame first:
//     du_n = L(n,n)^-T (z_n - sum_{i=1..PB} L(n+i,n)^T du_{n+i}),        blocks with n + i >= N are not used.
// k_lm_back does this for one right-hand side as a latency chain; here a factor column (25-31 KB) serves 64 samples.  One workgroup of two waves
// per (sequence, 64 samples).  Wave 1 only moves factor columns from HBM into a two-column LDS ring with LDS-DMA loads (as k_lm_back's loader),
// one column ahead of wave 0, and leaves the reciprocals of the column's diagonal (r = 1 / d, as k_cov_prep forms them) next to it.  Wave 0 owns
// the arithmetic, LANE = SAMPLE: the factor entries are wave-uniform LDS reads (broadcasts), du_n[28] lives in registers, du_{n+1..n+PB} in a
// lane-private LDS ring [PB][28][64] (consecutive lanes, consecutive words: no bank conflicts), so the products and the 28-step triangular solve
// are lane-local -- no cross-lane traffic at all.  Every sum has a fixed order (i, then the row of the block, ascending; the solve from row 27
// down) and nothing depends on the lane, the workgroup or the other samples: a sample's result is bit-equal whatever S, its slot and the batch.
// The lanes past S of the last workgroup shadow sample S - 1 and store nothing.  One barrier per column joins the two waves.
// n_frames: the length of every sequence (device), or null = all NS; a sequence of length 0 is not read.  du arrives zeroed: the frames past a
// sequence's own are not written.
template <int CNT>
__device__ __forceinline__ void band_row(double (&r)[CNT], const double* p) {      // CNT wave-uniform doubles from LDS
#pragma unroll
    for (int k = 0; k < CNT; k++) r[k] = p[k];
}
template <int PB>
__global__ __launch_bounds__(2 * WAVE) void k_band_sample(const double* __restrict__ L, const double* __restrict__ z, double* __restrict__ du,
                                                          const int* __restrict__ n_frames, int NS, int S) {
    constexpr int RING = PB + 1, BB = NU * NU, COLD = RING * BB;
    constexpr int COLB = COLD * 8, NCH = (COLB + 1023) / 1024;       // bytes per factor column, 1 KB LDS-DMA pieces per column
    static_assert(PB >= 3 && PB <= 4 && COLB % 16 == 0, "16-byte pieces; the LDS of both rings fits a CU");
    __shared__ __attribute__((aligned(16))) double col[2 * COLD];    // column n sits in slot n & 1
    __shared__ double dring[PB * NU * WAVE];                          // du of frame f: [f % PB][row][lane]
    __shared__ double srec[2 * NU];                                   // 1 / L(n,n)[k][k], [n & 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunks = (S + WAVE - 1) / WAVE;
    const int b = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int N = n_frames ? n_frames[b] : NS;
    if (N <= 0) return;                                               // uniform
    const double* Lb = L + (size_t)b * NS * COLD;

    if (wave == 1) {
        // ---- loader
        auto issue = [&](int n) {
            const char* g = reinterpret_cast<const char*>(Lb + (size_t)n * COLD) + lane * 16;
            double* dst = col + (n & 1) * COLD;
#pragma unroll
            for (int t = 0; t < NCH; t++)
                if (t * 1024 + lane * 16 < COLB)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + t * 1024),
                                                     (__attribute__((address_space(3))) void*)(dst + t * 128), 16, 0, 0);
        };
        // the column has landed (this wave's vmcnt covers its own LDS-DMA loads); its reciprocal diagonal, then the hand-over
        auto landed = [&](int n) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane < NU) srec[(n & 1) * NU + lane] = 1.0 / col[(n & 1) * COLD + lane * NU + lane];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        };
        issue(N - 1);
        landed(N - 1);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        for (int n = N - 1; n >= 0; n--) {
            // wave 0 works on column n; the other slot held column n + 1, which the barrier behind us has retired
            if (n >= 1) { issue(n - 1); landed(n - 1); }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        return;
    }

    // ---- wave 0: the arithmetic, lane = sample
    const int s_raw = chunk * WAVE + lane;
    const bool live = s_raw < S;
    const size_t base = ((size_t)b * S + (live ? s_raw : S - 1)) * NS * NU;
    const double* zs = z + base;
    double* ds = du + base;
    double zn[NU];                                                    // z of the next column, a column ahead
#pragma unroll
    for (int k = 0; k < NU; k++) zn[k] = zs[(size_t)(N - 1) * NU + k];
    lds_barrier();                                                    // column N - 1 and its reciprocals are in LDS
    for (int n = N - 1; n >= 0; n--) {
        double t[NU];
#pragma unroll
        for (int k = 0; k < NU; k++) t[k] = zn[k];
        {
            const size_t np = (size_t)(n > 0 ? n - 1 : 0) * NU;
#pragma unroll
            for (int k = 0; k < NU; k++) zn[k] = zs[np + k];
        }
        const double* Lc = col + (n & 1) * COLD;
        // t[k] -= sum_a L(n+i,n)[a][k] du_{n+i}[a], row by row.  The reads of row a + 1 (14 broadcasts of 16 bytes and the lane's own du: 15 LDS
        // operations, what lgkmcnt can count) are issued before the 28 multiply-adds of row a and land under them; the scheduling barriers keep the
        // compiler from sinking the reads to their uses, where three in flight would leave the wave waiting on LDS latency
#pragma unroll
        for (int i = 1; i <= PB; i++) {
            if (n + i < N) {                                          // uniform
                const double* Li = Lc + i * BB;
                const double* dv = dring + ((n + i) % PB) * (NU * WAVE) + lane;
                double ra[NU], rb[NU];
                double da = dv[0], db;
                band_row<NU>(ra, Li);
#pragma unroll
                for (int a = 0; a < NU; a += 2) {
                    band_row<NU>(rb, Li + (a + 1) * NU);
                    db = dv[(a + 1) * WAVE];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int k = 0; k < NU; k++) t[k] = fma(-ra[k], da, t[k]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (a + 2 < NU) { band_row<NU>(ra, Li + (a + 2) * NU); da = dv[(a + 2) * WAVE]; }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int k = 0; k < NU; k++) t[k] = fma(-rb[k], db, t[k]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // L(n,n)^T x = t from row 27 down: x[m] = t[m] r[m], then t[k] -= L(n,n)[m][k] x[m] for k < m (k from m - 1 down: the next row's pivot first)
        const double* rc = srec + (n & 1) * NU;
#pragma unroll
        for (int m = NU - 1; m >= 0; m--) {
            const double x = t[m] * rc[m];
            t[m] = x;
            const double* row = Lc + m * NU;
#pragma unroll
            for (int k = m - 1; k >= 0; k--) t[k] = fma(-row[k], x, t[k]);
        }
        double* dn = dring + (n % PB) * (NU * WAVE) + lane;           // takes the slot of du_{n+PB}, which no later column reads
#pragma unroll
        for (int k = 0; k < NU; k++) dn[k * WAVE] = t[k];
        if (live) {
#pragma unroll
            for (int k = 0; k < NU; k++) ds[(size_t)n * NU + k] = t[k];
        }
        lds_barrier();                                                // column n is retired; column n - 1 has landed
    }
}

// ---- the state of one sample frame, one wave per (sequence, sample, frame): the cold-start state of the frame (k_state_init's, in buffer 0 of the
// workspace) with du added to the entries ucoord_src names -- the update with which k_lm_back writes a trial iterate -- then the state phases
// k_frame_normal runs on such an iterate (cpe_kernels.hip; wave_leg_state), which make the Euler part consistent with the joint equalities.  The
// result goes to sstate [B S][N][ns], a state array of B S sequences that k_finalize reads as it reads the workspace's.
// RAGGED: rg.seq is the table of the B sequences; the frames past a sequence's own are left alone (k_finalize does not read them).
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_sample_state(const DevModel* __restrict__ M, const double* __restrict__ state0, const double* __restrict__ du,
                                                       double* __restrict__ sstate, int N, int S, RaggedArgs rg = RaggedArgs{}) {
    __shared__ double sq[CPE_MAX_NQ + CPE_MAX_JOINTS];               // q | alpha, contiguous as in the state
    __shared__ double ssc[6 * CPE_MAX_LINKS], ssa[2 * CPE_MAX_JOINTS], sR[36 * CPE_MAX_LINKS], sgam[GAM_STRIDE * CPE_MAX_JOINTS];
    const int lane = threadIdx.x;
    const unsigned i = blockIdx.x / (unsigned)N;                      // b S + s
    const int n = (int)(blockIdx.x % (unsigned)N), b = (int)(i / (unsigned)S);
    if constexpr (RAGGED) {
        const int2 rs = rg.seq[b];
        if (n >= rs.y) return;                                        // uniform
        M += rs.x;
    }
    const int nq = M->nq, nrev = M->nrev, ns = M->ns;
    const int4 fw = *reinterpret_cast<const int4*>(M->fn_lane[lane]);
    const double* src = state0 + ((size_t)b * N + n) * ns;
    for (int t = lane; t < ns; t += WAVE) sq[t] = src[t];
    const double d = du[(size_t)blockIdx.x * NU + (lane < NU ? lane : 0)];
    wave_lds_sync();
    if (lane < NU) sq[M->ucoord_src[lane]] += d;                      // (28 different entries)
    wave_lds_sync();
    wave_state_sincos(M, sq, sq + nq, ssc, ssa, nrev, lane);
    wave_lds_sync();
    wave_tail_roll(sq, ssc, M->hj_n, fw.x, lane);
    wave_trunk_rotations(M, ssc, sR, fw.y, lane);
    wave_lds_sync();
    wave_leg_state(sq, ssc, ssa, sR, sgam, nrev, fw.z, lane);
    wave_lds_sync();
    double* dst = sstate + (size_t)blockIdx.x * ns;
    for (int t = lane; t < ns; t += WAVE) dst[t] = sq[t];
}
