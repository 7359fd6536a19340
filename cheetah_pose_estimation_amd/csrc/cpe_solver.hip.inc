// cpe_solver.hip.inc -- solver kernels (included by cpe_kernels.hip).
//
// The NLP of the reference (acinoset_opt.py:589-617) in reduced coordinates u (the 28 independent dofs;
// the 26 dependent angles follow from the joint equalities in closed form):
//     min_u  sum_n [ sum_{c,l,d} rho(m_c w e) + bounds + pose prior ](u_n)  +  sum_{n>=3} sum_k w_k eps_{n,k}^2
// Levenberg-Marquardt with a block-banded Cholesky over the time axis (28x28 blocks, half-bandwidth 3
// = block-tridiagonal in 84x84 super-blocks).  DESIGN.md "Solver".

#define NU CPE_NX
// diagnostic build only (-DCPE_LM_STAMPS): per-phase shader-clock totals of block 0, read back with cpe_debug_lm_stamps
#ifdef CPE_LM_STAMPS
__device__ unsigned long long g_lm_stamps[32];     // 0..15: k_lm_step (thread 0 = factor wave, thread 64 = an update wave), 16..31: k_lm_back
__device__ unsigned long long g_fn_stamps[16];
#ifdef CPE_JAC_STAMPS      // slots 0..8 of g_fn_stamps go to k_dyn_jac's phases instead of k_frame_normal's
#define FSTAMP(i) do { (void)tf_last; } while (0)
#else
#define FSTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_fn_stamps[i] += t_ - tf_last; tf_last = t_; } } while (0)
#endif
#define STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_lm_stamps[i] += t_ - t_last; t_last = t_; } } while (0)
#define USTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == WAVE) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_lm_stamps[i] += t_ - tu_last; tu_last = t_; } } while (0)
#define BSTAMP(i) do { if (blockIdx.x == 0 && lane == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_lm_stamps[16 + (i)] += t_ - tb_last; tb_last = t_; } } while (0)
#define RSTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == WAVE && g_tu) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_lm_stamps[i] += t_ - *g_tu; *g_tu = t_; } } while (0)
#else
#define RSTAMP(i) do { } while (0)
#define USTAMP(i) do { } while (0)
#define BSTAMP(i) do { } while (0)
#define STAMP(i) do { } while (0)
#define FSTAMP(i) do { } while (0)
#endif
#define LDB 29                 // padded leading dimension of a 28x28 block in LDS (odd: conflict-free columns)
#define BLK (NU * LDB)
#define LM_THREADS 256
// Floor of the diagonal in the Marquardt scaling lambda * max(diag H, floor).  Sequences of fewer than 4 frames have no motion term (no third
// difference exists): a coordinate no measurement of its frame sees is tied to nothing, its diagonal is ~0 and scaling alone leaves it undamped (steps
// of 30 rad, creep to the iteration limit) -> floor 0.1 there, ~1e-5 of the diagonal of an observed coordinate.  From 4 frames on the motion term
// ties every coordinate to its neighbours and the floor would only slow the weakly observed directions next to the Euler pole (measured: 200
// instead of 38 iterations): 1e-12, the guard against an exact zero.  Same rule in the oracle (CPO_DIAG_FLOOR).
#define LM_DIAG_FLOOR(N) ((N) < 4 ? 0.1 : 1e-12)
#define LM_NU0 8.0               // first rejection multiplies lambda by 8, then 16, 32, ... (same constant in the oracle)
#define LM_MAX_REV 12           // leg links (revolute joints) the LM kernel is sized for
#define LM_MAX_LEGS 6           // leg links hanging on one body
#define LM_MAX_TERMS 256        // product terms of the motion model's block pattern (cheetah: ~210)
#define LM_MAX_GROUP 7          // terms of one element: the diagonal + one per leg link of the body (1 + LM_MAX_LEGS)

struct LmParams {
    double tol_step, tol_cost, lambda0, bound_tol;
    int32_t B, N, max_outer, max_iter;
};
// Ragged batch (cpe_solve_ragged, DESIGN.md 7): sequence b solves device model seq[b].x (an index into the handle's model array) over the
// first seq[b].y frames of the nmax its buffers are laid out for; meas / weight / meas_err carry cstride cameras per frame.  The kernels of the
// kinematic solve take it as a compile-time form (RAGGED = true, launched with the table); their plain forms never read it.
struct RaggedArgs { const int2* seq; int nmax; int cstride; };

// The slot of a per-frame workgroup: workgroup blockIdx.x of a launch over N frames per sequence works on frame n of sequence b -- frame
// f = b N + n of the buffers -- which solves device model `model` (an offset the caller adds to its per-model tables: M += s.model) over its
// first `len` frames.
struct FrameSlot { int b, n, model, len; };
// act / n_act: the sequences of this launch and how many of them are in use (a device word), or null = all.  False: the workgroup has nothing
// to do -- past the active list, or RAGGED and past the sequence's own length (the slot is filled all the same).  Plain form: model 0, len N,
// both compile-time.  The status of the sequence is the caller's to test.
template <bool RAGGED>
__device__ __forceinline__ bool frame_slot(int N, const int* __restrict__ act, const int* __restrict__ n_act, const RaggedArgs& rg, FrameSlot& s) {
    const unsigned i = blockIdx.x / (unsigned)N;
    if (n_act && (int)i >= *n_act) return false;
    s.b = act ? act[i] : (int)i;
    s.n = (int)(blockIdx.x % (unsigned)N);
    s.model = 0; s.len = N;
    if constexpr (RAGGED) {
        const int2 rs = rg.seq[s.b];
        s.model = rs.x; s.len = rs.y;
        if (s.n >= rs.y) return false;
    }
    return true;
}
// the same for a kernel over all frames that is not told N: the ragged form has it in rg.nmax, the plain form needs no slot (model 0)
template <bool RAGGED>
__device__ __forceinline__ bool frame_slot_flat(const RaggedArgs& rg, FrameSlot& s) {
    if constexpr (RAGGED) return frame_slot<true>(rg.nmax, nullptr, nullptr, rg, s);
    s = FrameSlot{0, 0, 0, 0};
    return true;
}

#define COST_STRIDE 8   // per-frame cost record: meas, bound(AL), pose, clamped, max bound violation, autoregressive prior

// --------------------------------------------------------------------------------------------------
// Reduced coordinates of the solver (DESIGN.md 2): trunk = independent Euler dofs; every leg link c is its
// body B rotated about B's y axis: R_c = R_B Ry(alpha_c).  One frame's state = Euler q (nq) | alpha (nrev).
#define GAM_STRIDE 4    // per leg link: d theta_c / d (alpha_c, phi_B, theta_B, psi_B)

// value of weighted coordinate k for the cost terms (DevModel::ucost): an Euler angle of the trunk, or theta_B + alpha for a leg link
__device__ __forceinline__ double cost_coord(const DevModel* __restrict__ M, const double* __restrict__ state, int k) {
    const int w = M->ucost[k];
    return state[w & 255] + ((w >> 8) ? state[(w >> 8) - 1] : 0.0);
}

// Euler angles (principal pitch) of leg link r from (R_B, alpha_r): the triple the STATE carries (forward kinematics of the outputs, the physics terms).
// The row Gamma_r it returns is d theta_c / d(...) of that triple; the cost terms do not use it any more (cost pitch: Gamma = (1, 0, 1, 0)).
// Body angular velocity per unit Euler rate of B (ZYX): phi: (1,0,0)  theta: (0,cphi,-sphi)  psi: (-sth, sphi cth, cphi cth);
// in the leg frame w' = Ry(alpha)^T w, and theta_c' = cos(phi_c) w'_y - sin(phi_c) w'_z.
__device__ __forceinline__ void leg_euler(const double* RB, const double* scB, double sa, double ca, double psi_ref,
                                          double* euler, double* gam) {
    // R_c = R_B Ry(alpha): columns 0 and 2 mix, column 1 is R_B's
    const double r00 = RB[0] * ca - RB[2] * sa, r10 = RB[3] * ca - RB[5] * sa, r20 = RB[6] * ca - RB[8] * sa;
    const double r21 = RB[7], r22 = RB[6] * sa + RB[8] * ca;
    double sth = -r20; sth = fmin(1.0, fmax(-1.0, sth));
    const double th = asin(sth), phi = atan2(r21, r22);
    double psi = atan2(r10, r00);
    psi += 6.283185307179586476925286766559 * rint((psi_ref - psi) / 6.283185307179586476925286766559);
    euler[0] = phi; euler[1] = th; euler[2] = psi;
    const double cth = sqrt(fmax(0.0, 1.0 - sth * sth));
    const double icth = cth > 1e-300 ? 1.0 / cth : 0.0;
    const double sphic = r21 * icth, cphic = r22 * icth;            // sin / cos of phi_c
    const double sfB = scB[0], cfB = scB[1], stB = scB[2], ctB = scB[3];
    gam[0] = cphic;                                                   // w' = e_y
    // phi_B: w = (1,0,0) -> w' = (ca, 0, sa)
    gam[1] = -sphic * sa;
    // theta_B: w = (0, cfB, -sfB) -> w' = (sa sfB, cfB, -ca sfB)
    gam[2] = cphic * cfB + sphic * ca * sfB;
    // psi_B: w = (-stB, sfB ctB, cfB ctB) -> w'_y = sfB ctB, w'_z = -sa stB + ca cfB ctB
    gam[3] = cphic * sfB * ctB - sphic * (ca * cfB * ctB - sa * stB);
}

// State phase (after the trunk rotations, cpe_kernels.hip): Euler triple of leg link `lane` -> sq, and its constant Gamma row of the cost
// pitch theta_B + alpha_c, d / d (alpha_c, phi_B, theta_B, psi_B) = (1, 0, 1, 0), -> sgam.  fwz = body | child << 8 | body's trunk slot << 16
__device__ __forceinline__ void wave_leg_state(double* sq, const double* ssc, const double* ssa, const double* sR, double* sgam, int nrev,
                                               int fwz, int lane) {
    if (lane < nrev) {
        const int Bk = fwz & 255, c = (fwz >> 8) & 255;
        double e[3];
        double gtrue[GAM_STRIDE];
        leg_euler(sR + 36 * (fwz >> 16), ssc + 6 * Bk, ssa[2 * lane], ssa[2 * lane + 1], sq[3 + 3 * Bk + 2], e, gtrue);
        sq[3 + 3 * c] = e[0]; sq[3 + 3 * c + 1] = e[1]; sq[3 + 3 * c + 2] = e[2];
        sgam[GAM_STRIDE * lane] = 1.0; sgam[GAM_STRIDE * lane + 1] = 0.0; sgam[GAM_STRIDE * lane + 2] = 1.0; sgam[GAM_STRIDE * lane + 3] = 0.0;
    }
}

// the inverse, for a state built from an Euler q: alpha = rotation of R_B^T R_c about y, from the Euler triples of the body and of the leg link
__device__ __forceinline__ double leg_alpha(const double* qb, const double* qc) {
    double scb[6], scc[6], RB[9], RC[9];
    for (int a = 0; a < 3; a++) { sincos(qb[a], &scb[2 * a], &scb[2 * a + 1]); sincos(qc[a], &scc[2 * a], &scc[2 * a + 1]); }
    rot_kind(scb, 0, RB); rot_kind(scc, 0, RC);
    const double m00 = RB[0] * RC[0] + RB[3] * RC[3] + RB[6] * RC[6], m02 = RB[0] * RC[2] + RB[3] * RC[5] + RB[6] * RC[8];
    return atan2(m02, m00);
}

// --------------------------------------------------------------------------------------------------
// initial state from an Euler q: alpha_r = leg_alpha.  One wave per frame.
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_state_init(const DevModel* __restrict__ M, const double* __restrict__ q, double* __restrict__ state,
                                                    RaggedArgs rg = RaggedArgs{}) {
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    FrameSlot s;
    if (!frame_slot_flat<RAGGED>(rg, s)) return;           // padding frames stay unset: nothing reads them
    M += s.model;
    const int nq = M->nq, ns = M->ns;
    if (lane < nq) state[f * ns + lane] = q[f * nq + lane];
    if (lane < M->nrev) state[f * ns + nq + lane] = leg_alpha(q + f * nq + 3 + 3 * M->rev_body[lane], q + f * nq + 3 + 3 * M->rev_child[lane]);
}

// --------------------------------------------------------------------------------------------------
// per-frame normal equations.  One wave per frame.
// dynamic LDS (doubles): q[nq] | al[nrev] | sc[6nl] | sa[2 nrev] | R[36nl] | pos[3L] | cam[23C] | dyn[3 sv_n] | gam[4 nrev]
//                        | dp[3 ss_n] | Sv[8 ndep] | Mv[9L] | Dp[3 mc_total] | H[nu nu] | g[nu]
// which = 1: evaluate buffer `cur` (first call), 0: evaluate the trial buffer 1-cur.
//
// Shutter delay (SURVEY 8f-4, acinoset_misc.py:179-183, :278-288): with sh.tau != null every camera c sees the markers displaced by
// v_n tau_c + a_n tau_c^2 (v, a = implicit-Euler velocity and acceleration of the base position, from node 2 on: q'_0, q''_0 are free in the
// reference, its first two nodes can absorb any shift).  P = p_l(u_n) + alpha_c x_n + beta_c x_n-1 + gamma_c x_n-2 with
// alpha = tau/h + tau^2/h^2, beta = -tau/h - 2 tau^2/h^2, gamma = tau^2/h^2.  The gradient is exact -- its parts that belong to the base
// position of frames n-1, n-2 go to sh.gx for k_lm_step to collect -- and so is the curvature inside the frame; the cross-frame curvature
// blocks are left out of the Gauss-Newton matrix (any positive semi-definite model is admissible for LM).  sh.rcb receives, per camera,
// sum_l G^T rho' w (3) and sum_l G^T cw G (6): what the delay update (k_shutter_step) needs.
// PLAIN (no Gaussian-mixture prior, no shutter delay): H never sits in LDS -- every lane stores its finished entries of the gather straight to
// HBM, the few bound terms follow as global atomics -- which takes 6 KB off the wave's LDS: 11 waves per CU instead of 8, and this kernel's time
// goes with 1 / occupancy (measured by padding its LDS: 8 waves 1.87 ms, 6 waves 2.32, 5 waves 3.19).
struct ShutterArgs { const double* tau; double* gx; double* rcb; };
template <bool PLAIN, bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_frame_normal(const DevModel* __restrict__ M, const SeqState* __restrict__ st,
                                                       int N, int which, size_t n_frames,
                                                       double* __restrict__ qbuf, const double* __restrict__ meas,
                                                       const double* __restrict__ weight, double* __restrict__ gbuf,
                                                       double* __restrict__ Bbuf, double* __restrict__ costbuf,
                                                       double* __restrict__ mu, double* __restrict__ gambuf,
                                                       const DevPriors* __restrict__ pri, const int* __restrict__ act /* sequences of this launch, or null = all */,
                                                       const int* __restrict__ n_act /* entries of act in use (device word written by k_build_act), or null */,
                                                       ShutterArgs sh = ShutterArgs{nullptr, nullptr, nullptr},
                                                       RaggedArgs rg = RaggedArgs{} /* RAGGED: N = nmax, no shutter delay */) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, act, n_act, rg, fs)) return;
    M += fs.model;
    const int b = fs.b;
    const size_t f = (size_t)b * N + fs.n;
    const SeqState S = st[b];
    if (S.status != 0) return;
    const int pend = S.al_pending;                       // multiplier update: re-evaluate the CURRENT iterate
    const int buf = (which || pend) ? S.cur : 1 - S.cur;

    const int nq = M->nq, nl = M->nl, L = M->L, C = M->C, nu = M->nu, ndep = M->ndep, mct = M->mc_total;
    const int nrev = M->nrev, ns = M->ns, ssn = M->ss_n, svn = M->sv_n;
    double* sq = smem;
    double* sal = sq + nq;
    double* ssc = sal + nrev;
    double* ssa = ssc + 6 * nl;
    double* sR = ssa + 2 * nrev;                        // R, dR/dphi, dR/dtheta, dR/dpsi of the TRUNK links (slot = trunk_slot[link])
    const int n_camov = 6 * nl + 2 * nrev + 36 * M->n_trunk;     // doubles from ssc to the end of sR: dead once Dp is built, the cameras move in (CAMW C doubles;
    double* spos = ssc + (n_camov > CAMW * C ? n_camov : CAMW * C);   // the host's lds_normal pads likewise when they need more)
    double* scam = ssc;
    double* sdyn = spos + 3 * L;
    double* sgam = sdyn + 3 * svn;
    double* sSv = sgam + GAM_STRIDE * nrev;
    const int n_ov = CPE_MAX_SCOL * M->n_srow, n_hg = PLAIN ? nu : nu * nu + nu;
    double* sMv = sSv + (n_ov > n_hg ? n_ov : n_hg);
    double* sDp = sMv + 9 * L;
    double* sH = sSv;                                    // H | g (PLAIN: g alone) overlay the S rows, which are dead once Dp is built
    double* sg = PLAIN ? sSv : sH + nu * nu;
    (void)ssn;

#ifdef CPE_LM_STAMPS
    unsigned long long tf_last = __builtin_amdgcn_s_memtime();
#endif
    const int4 fw = *reinterpret_cast<const int4*>(M->fn_lane[lane]);      // this lane's first-phase words (cpe_model.h): no table read below depends on another
    const int svl = lane < CPE_MAX_SDYN ? lane : 0;
    double svv[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) { svv[i][0] = M->sv_vec[svl][i][0]; svv[i][1] = M->sv_vec[svl][i][1]; svv[i][2] = M->sv_vec[svl][i][2]; }
    const int hj_n = M->hj_n;
    __builtin_amdgcn_s_setprio(2);                          // issue priority while the frame's short phases run (measured: 1.070 -> 1.057 ms; raised for the
    const int hk_n = M->hk_n;                                // pair phase instead 1.107, graded by phase 1.12): a wave gets its loads and its LDS round trips out early
    const int2 hkw = *reinterpret_cast<const int2*>(M->hk_w[lane]);      // this lane's hooke S item (64 table rows: the read is unconditional)
    double* stf = qbuf + (size_t)buf * n_frames * ns + f * ns;
    for (int t = lane; t < ns; t += WAVE) sq[t] = stf[t];  // q and alpha are contiguous in LDS too (sal = sq + nq); ns may exceed 64
    for (int t = lane; t < 9 * L; t += WAVE) sMv[t] = 0.0;
    wave_lds_sync();
    // ---- the state phases (cpe_kernels.hip)
    wave_state_sincos(M, sq, sal, ssc, ssa, nrev, lane);
    wave_lds_sync();
    wave_tail_roll(sq, ssc, hj_n, fw.x, lane);
    wave_trunk_rotations(M, ssc, sR, fw.y, lane);
    wave_lds_sync();
    wave_leg_state(sq, ssc, ssa, sR, sgam, nrev, fw.z, lane);
    wave_leg_vectors(ssa, sdyn, svn, fw.w, svv, lane);
    wave_lds_sync();
    if (lane < nq) stf[lane] = sq[lane];                  // Euler part of the state, consistent with the joint equalities
    if (lane < GAM_STRIDE * nrev) gambuf[((size_t)buf * n_frames + f) * (GAM_STRIDE * nrev) + lane] = sgam[lane];

    // this lane's marker chain (positions phase below), requested before the S rows are worked out: all reads unconditional and independent
    const int lm_ = lane < L ? lane : 0;
    int pco[CPE_MAX_CHAIN]; double pcv[CPE_MAX_CHAIN][3];
#pragma unroll
    for (int k = 0; k < CPE_MAX_CHAIN; k++) { pco[k] = M->pc_off[lm_][k]; pcv[k][0] = M->pc_vec[lm_][k][0]; pcv[k][1] = M->pc_vec[lm_][k][1]; pcv[k][2] = M->pc_vec[lm_][k][2]; }
    const int pwid = M->pw_id[lm_], pwo = M->pw_off[lm_];
    FSTAMP(0);
    wave_hooke_srows(sR, sSv, hk_n, hkw, lane);

    FSTAMP(1);
    // ---- marker positions: x + sum_trunk R_k v_k + R_B w(alpha)
    if (lane < L) {
        double p0 = sq[0], p1 = sq[1], p2 = sq[2];
#pragma unroll
        for (int k = 0; k < CPE_MAX_CHAIN; k++) {          // entries past the chain's length: rotation 0 times a zero vector
            const double* R = sR + pco[k];
            const double v0 = pcv[k][0], v1 = pcv[k][1], v2 = pcv[k][2];
            p0 += R[0] * v0 + R[1] * v1 + R[2] * v2; p1 += R[3] * v0 + R[4] * v1 + R[5] * v2; p2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
        }
        const int wid = pwid;
        if (wid >= 0) {
            const double* R = sR + pwo;
            const double v0 = sdyn[3 * wid], v1 = sdyn[3 * wid + 1], v2 = sdyn[3 * wid + 2];
            p0 += R[0] * v0 + R[1] * v1 + R[2] * v2; p1 += R[3] * v0 + R[4] * v1 + R[5] * v2; p2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
        }
        spos[3 * lane] = p0; spos[3 * lane + 1] = p1; spos[3 * lane + 2] = p2;
    }
    FSTAMP(2);
    // ---- reduced marker columns Dp[(marker, column)] = sum of its terms  z * Mat v : matrix = trunk R / dR or identity, v a constant or
    // dynamic (leg) vector, z = 1 or an entry of a hooke S row.  One term per lane per round from a flat list (32 bytes per term, read in
    // list order: no gathers, nothing staged per slot), summed into Dp with LDS adds -- the terms of one column sit next to each other.
    // measurements and weights of the first PAIR_PF rounds of the pair loop and the multipliers of the bounds: loaded here, used two phases on
    // (this kernel is a latency chain -- its time goes with 1 / occupancy -- so an HBM round trip taken in the shadow of other work is time gained)
    constexpr int PAIR_PF = 3;
    const size_t pair0 = f * (size_t)((RAGGED ? rg.cstride : C) * L);
    const int n_pairs = C * L;
    const int pt0 = lane < n_pairs ? lane : n_pairs - 1, pt1 = WAVE + lane < n_pairs ? WAVE + lane : n_pairs - 1,      // clamped: the loads
              pt2 = 2 * WAVE + lane < n_pairs ? 2 * WAVE + lane : n_pairs - 1;                                            // themselves are unconditional
    const double pf_w0 = weight[pair0 + pt0], pf_w1 = weight[pair0 + pt1], pf_w2 = weight[pair0 + pt2];
    const double2 pf_za = reinterpret_cast<const double2*>(meas)[pair0 + pt0], pf_zb = reinterpret_cast<const double2*>(meas)[pair0 + pt1],
                  pf_zc = reinterpret_cast<const double2*>(meas)[pair0 + pt2];
    const double* camw = reinterpret_cast<const double*>(M->cam);   // first three rounds of the camera table in registers now, to LDS after the Dp phase
    const int ncw = CAMW * C;
    const double pf_c0 = camw[lane < ncw ? lane : 0], pf_c1 = camw[WAVE + lane < ncw ? WAVE + lane : 0], pf_c2 = camw[2 * WAVE + lane < ncw ? 2 * WAVE + lane : 0];
    const int nbnd = M->nb;
    double2 pf_mu = make_double2(0.0, 0.0);
    if (nbnd > 0) pf_mu = reinterpret_cast<const double2*>(mu)[f * (size_t)nbnd + (lane < nbnd ? lane : nbnd - 1)];
    for (int t = lane; t < 3 * mct; t += WAVE) sDp[t] = 0.0;
    wave_lds_sync();
    {
        const int ntl = M->tl_n;
        // a round ahead: the 32 bytes of round k + 1 are requested before round k's arithmetic (reads past the list stay inside the table)
        int2 wn = *reinterpret_cast<const int2*>(&M->tl[lane].w0);
        double v0n = M->tl[lane].v[0], v1n = M->tl[lane].v[1], v2n = M->tl[lane].v[2];
        for (int e = lane; e < ntl; e += WAVE) {
            const int2 w = wn;
            const double v0c = v0n, v1c = v1n, v2c = v2n;
            {
                const int en = e + WAVE < CPE_MAX_TL ? e + WAVE : lane;
                wn = *reinterpret_cast<const int2*>(&M->tl[en].w0);
                v0n = M->tl[en].v[0]; v1n = M->tl[en].v[1]; v2n = M->tl[en].v[2];
            }
            const int item = w.x & 1023, si = ((w.x >> 10) & 1023) - 1, vd = ((w.x >> 20) & 1023) - 1, moff = w.y;
            // (every LDS read unconditional, at a clamped index)
            const double* dy = sdyn + 3 * (vd < 0 ? 0 : vd);
            const double y0 = dy[0], y1 = dy[1], y2 = dy[2];
            const double* D = sR + (moff < 0 ? 0 : moff);
            const double D0 = D[0], D1 = D[1], D2 = D[2], D3 = D[3], D4 = D[4], D5 = D[5], D6 = D[6], D7 = D[7], D8 = D[8];
            const double zz = sSv[si < 0 ? 0 : si];
            const double v0 = vd < 0 ? v0c : y0, v1 = vd < 0 ? v1c : y1, v2 = vd < 0 ? v2c : y2;
            const double z = si < 0 ? 1.0 : zz;
            const double p0 = moff < 0 ? v0 : D0 * v0 + D1 * v1 + D2 * v2;
            const double p1 = moff < 0 ? v1 : D3 * v0 + D4 * v1 + D5 * v2;
            const double p2 = moff < 0 ? v2 : D6 * v0 + D7 * v1 + D8 * v2;
            atomicAdd(sDp + 3 * item, z * p0); atomicAdd(sDp + 3 * item + 1, z * p1); atomicAdd(sDp + 3 * item + 2, z * p2);
        }
    }
    wave_lds_sync();
    if (lane < ncw) scam[lane] = pf_c0;                   // sin / cos tables and trunk rotations are dead: the cameras take their place
    if (WAVE + lane < ncw) scam[WAVE + lane] = pf_c1;
    if (2 * WAVE + lane < ncw) scam[2 * WAVE + lane] = pf_c2;
    for (int t = 3 * WAVE + lane; t < ncw; t += WAVE) scam[t] = camw[t];
    for (int t = lane; t < (PLAIN ? nu : nu * nu + nu); t += WAVE) sH[t] = 0.0;   // H | g (PLAIN: g) take over the space of the S rows
    const size_t fo = (size_t)buf * n_frames + f;
    double* Bo = Bbuf + fo * (nu * nu);
    if (PLAIN)                                            // structural zeros of H: no lane's gather list writes them
        for (int t = lane; t < nu * nu; t += WAVE) if (!((M->h_covered[t >> 5] >> (t & 31)) & 1u)) Bo[t] = 0.0;
    // shutter-delay scratch behind everything else: shift[C][3] | coef[C][3] (alpha, beta, gamma) | rc[C][3] | Mc[C][6] | M1[L][6] | M2[6]
    const int nloc = fs.n;
    const bool shut = sh.tau != nullptr && nloc >= 2;
    double* sSh = sDp + 3 * mct + ((pri && pri->p.gmm_k > 0) ? CPE_NX + pri->p.gmm_k * pri->p.gmm_dim + CPE_MAX_GMM + CPE_NX : 0);
    double* sCo = sSh + 3 * C; double* sRc = sCo + 3 * C; double* sMc = sRc + 3 * C; double* sM1 = sMc + 6 * C; double* sM2 = sM1 + 6 * L;
    if (sh.tau) {
        for (int t = lane; t < 6 * C + 3 * C + 6 * C + 6 * L + 6; t += WAVE) sSh[t] = 0.0;
        wave_lds_sync();
        if (shut && lane < C) {
            const double ta = sh.tau[(size_t)b * C + lane], ih = 1.0 / M->h;
            const double al = ta * ih + ta * ta * ih * ih, be = -ta * ih - 2.0 * ta * ta * ih * ih, ga = ta * ta * ih * ih;
            sCo[3 * lane] = al; sCo[3 * lane + 1] = be; sCo[3 * lane + 2] = ga;
            const double* s1 = stf - ns; const double* s2 = stf - 2 * ns;          // frames n-1, n-2 of the same buffer
            for (int d = 0; d < 3; d++) sSh[3 * lane + d] = al * sq[d] + be * s1[d] + ga * s2[d];
        }
        wave_lds_sync();
    }

    FSTAMP(3);
    // ---- every valid (camera, marker) pair: robust loss, 3x3 normal matrix and 3-gradient per marker
    double fc = 0.0;
    __builtin_amdgcn_s_setprio(0);
    for (int t = lane, rnd = 0; t < n_pairs; t += WAVE, rnd++) {
        const int c = t / L, l = t - c * L;
        double w_in; double2 z;
        if (rnd < PAIR_PF) {                                // (rnd is wave-uniform; with the loop unrolled these are plain register picks)
            w_in = rnd == 0 ? pf_w0 : (rnd == 1 ? pf_w1 : pf_w2);
            z.x = rnd == 0 ? pf_za.x : (rnd == 1 ? pf_zb.x : pf_zc.x);
            z.y = rnd == 0 ? pf_za.y : (rnd == 1 ? pf_zb.y : pf_zc.y);
        } else { w_in = weight[pair0 + t]; z = reinterpret_cast<const double2*>(meas)[pair0 + t]; }
        const double w = scam[CAMW * c + 21] * w_in;
        if (w == 0.0) { fc += 2.0 * M->rho0; continue; }   // the reference still adds rho(0) per coordinate
        double u, v, G[6];
        const double sx = sh.tau ? sSh[3 * c] : 0.0, sy = sh.tau ? sSh[3 * c + 1] : 0.0, sz = sh.tau ? sSh[3 * c + 2] : 0.0;
        project_point_staged(scam, c, spos[3 * l] + sx, spos[3 * l + 1] + sy, spos[3 * l + 2] + sz, u, v, G);
        const LossOut l0 = robust_loss(w * (u - z.x), M->loss_a, M->loss_b, M->loss_c, M->curvature, true);
        const LossOut l1 = robust_loss(w * (v - z.y), M->loss_a, M->loss_b, M->loss_c, M->curvature, true);
        fc += l0.rho + l1.rho;
        const double g0 = l0.d1 * w, g1 = l1.d1 * w, c0 = l0.cw * w * w, c1 = l1.cw * w * w;
        double* Mv = sMv + 9 * l;
        const double m6[6] = {c0 * G[0] * G[0] + c1 * G[3] * G[3], c0 * G[0] * G[1] + c1 * G[3] * G[4], c0 * G[0] * G[2] + c1 * G[3] * G[5],
                              c0 * G[1] * G[1] + c1 * G[4] * G[4], c0 * G[1] * G[2] + c1 * G[4] * G[5], c0 * G[2] * G[2] + c1 * G[5] * G[5]};
        const double r3[3] = {g0 * G[0] + g1 * G[3], g0 * G[1] + g1 * G[4], g0 * G[2] + g1 * G[5]};
#pragma unroll
        for (int e = 0; e < 6; e++) atomicAdd(Mv + e, m6[e]);
#pragma unroll
        for (int e = 0; e < 3; e++) atomicAdd(Mv + 6 + e, r3[e]);
        if (sh.tau) {
            const double al = sCo[3 * c];
#pragma unroll
            for (int e = 0; e < 6; e++) { atomicAdd(sMc + 6 * c + e, m6[e]); if (shut) { atomicAdd(sM1 + 6 * l + e, al * m6[e]); atomicAdd(sM2 + e, al * al * m6[e]); } }
#pragma unroll
            for (int e = 0; e < 3; e++) atomicAdd(sRc + 3 * c + e, r3[e]);
        }
    }
    unsigned nxt[8];                                      // first batch of the gather list below: requested before the reduction and the fence
#pragma unroll
    for (int u = 0; u < 8; u++) nxt[u] = M->hg_code[u][lane];
    const int bq = M->bnd_q[lane & (CPE_MAX_BOUNDS - 1)];
    const double b_lo = M->bound_lo[lane & (CPE_MAX_BOUNDS - 1)], b_up = M->bound_up[lane & (CPE_MAX_BOUNDS - 1)];      // this lane's bound (used after the gather)
    fc = wave_sum(fc);
    wave_lds_sync();

    FSTAMP(4);
    // ---- H = sum_l Dp_l^T M_l Dp_l, g = sum_l Dp_l^T v_l by gathering: every lane sums the contributions of its own
    // entries of the lower triangle in a register (balanced lists built on the host) and stores entry and mirror once
    {
        const int cnt = M->hg_cnt[lane], kmax = M->hg_max;
        double acc = 0.0;
        int tgt = -1;                                       // a * nu + b of the entry being summed
        // list words eight at a time (independent loads, one L2 round trip), a batch ahead of the branch-free arithmetic that uses them;
        // rows past the lane's own count are read too (the table has CPE_MAX_HG rows) and ignored
        for (int k0 = 0; k0 < kmax; k0 += 8) {
            unsigned codes[8];
#pragma unroll
            for (int u = 0; u < 8; u++) codes[u] = nxt[u];
            if (k0 + 8 < kmax) {
#pragma unroll
                for (int u = 0; u < 8; u++) nxt[u] = M->hg_code[k0 + 8 + u < CPE_MAX_HG ? k0 + 8 + u : CPE_MAX_HG - 1][lane];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const unsigned code = k0 + u < cnt ? codes[u] : 0u;
                const bool valid = k0 + u < cnt;
                const double* di = sDp + 3 * (code & 255);
                const double* dj = sDp + 3 * ((code >> 8) & 255);
                const double* Mv = sMv + 9 * ((code >> 16) & 31);
                const double a0 = Mv[0] * dj[0] + Mv[1] * dj[1] + Mv[2] * dj[2];
                const double a1 = Mv[1] * dj[0] + Mv[3] * dj[1] + Mv[4] * dj[2];
                const double a2 = Mv[2] * dj[0] + Mv[4] * dj[1] + Mv[5] * dj[2];
                const double term = di[0] * a0 + di[1] * a1 + di[2] * a2;
                if (valid && ((code >> 21) & 1)) {            // first contribution of a new entry: store the finished one
                    if (tgt >= 0) { const int ea = tgt >> 5, eb = tgt & 31; double* Hd = PLAIN ? Bo : sH; Hd[ea * nu + eb] = acc; Hd[eb * nu + ea] = acc; }
                    tgt = (int)(code >> 22);
                    acc = 0.0;
                }
                acc += valid ? term : 0.0;
            }
        }
        if (tgt >= 0) { const int ea = tgt >> 5, eb = tgt & 31; double* Hd = PLAIN ? Bo : sH; Hd[ea * nu + eb] = acc; Hd[eb * nu + ea] = acc; }
        if (lane < nu) {
            double ga = 0.0;
            const int gc_ = M->gg_cnt[lane];
            for (int k = 0; k < gc_; k++) {
                const int code = M->gg_code[k][lane];
                const double* di = sDp + 3 * (code & 255);
                const double* Mv = sMv + 9 * (code >> 8);
                ga += di[0] * Mv[6] + di[1] * Mv[7] + di[2] * Mv[8];
            }
            sg[lane] = ga;
        }
    }
    wave_lds_sync();
    if (sh.tau) {
        // d P / d u_n = Dp_l + alpha_c E (E picks the base position, reduced coordinates 0..2, and Dp_l E = I): inside the frame
        //   H += sum_l [ E^T M1_l Dp_l + Dp_l^T M1_l E ] + E^T M2 E,   g += E^T sum_c alpha_c rc_c
        // (the E^T M1_l Dp_l sum runs over ALL reduced columns of the marker, the base position included: together with its transpose and
        // M2 that is (1 + alpha)^2 on the xyz block).  Per (marker, reduced column) item: 3 x 2 LDS adds, in list order (one wave).
        if (shut) {
            for (int t = lane; t < mct; t += WAVE) {
                const int l = M->mc_marker[t], j = M->mcol[l][M->mc_j[t]];
                const double* m1 = sM1 + 6 * l; const double* d = sDp + 3 * t;
                const double y0 = m1[0] * d[0] + m1[1] * d[1] + m1[2] * d[2], y1 = m1[1] * d[0] + m1[3] * d[1] + m1[4] * d[2], y2 = m1[2] * d[0] + m1[4] * d[1] + m1[5] * d[2];
                atomicAdd(sH + 0 * nu + j, y0); atomicAdd(sH + 1 * nu + j, y1); atomicAdd(sH + 2 * nu + j, y2);
                atomicAdd(sH + j * nu + 0, y0); atomicAdd(sH + j * nu + 1, y1); atomicAdd(sH + j * nu + 2, y2);
            }
            if (lane < 9) { const int r = lane / 3, cc = lane - 3 * r; const int e = r <= cc ? (r == 0 ? cc : (r == 1 ? 2 + cc : 5)) : (cc == 0 ? r : (cc == 1 ? 2 + r : 5)); atomicAdd(sH + r * nu + cc, sM2[e]); }
            if (lane < 3) { double a = 0.0; for (int c = 0; c < C; c++) a += sCo[3 * c] * sRc[3 * c + lane]; atomicAdd(sg + lane, a); }
        }
        // parts of the gradient that belong to the base position of frames n-1 and n-2, and the per-camera sums for the delay update
        const size_t fo2 = (size_t)buf * n_frames + f;
        if (lane < 6) {
            double a = 0.0;
            if (shut) for (int c = 0; c < C; c++) a += sCo[3 * c + 1 + lane / 3] * sRc[3 * c + lane % 3];
            sh.gx[fo2 * 6 + lane] = a;
        }
        for (int t = lane; t < 9 * C; t += WAVE) { const int c = t / 9, e = t - 9 * c; sh.rcb[(fo2 * C + c) * 9 + e] = e < 3 ? sRc[3 * c + e] : sMc[6 * c + e - 3]; }
        wave_lds_sync();
    }

    FSTAMP(5);
    // ---- angle bounds (cheetah.py:306-352), augmented Lagrangian: per bound two multipliers (upper, lower side),
    // psi = (max(0, mu + kappa*viol)^2 - mu^2) / (2 kappa), linear in u
    double fb = 0.0, vm = 0.0;
    if (lane < nbnd) {
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
            // v = difference of two EULER angles; its gradient in the reduced coordinates is a difference of two
            // sparse rows: (k, 1) for a trunk angle, (alpha_c, phi_B, theta_B, psi_B) x Gamma_r for a leg pitch
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
            if (PLAIN) __builtin_amdgcn_s_waitcnt(0x0F70);       // the gather's stores of H have been acknowledged: the adds below come after them
            for (int i = 0; i < nz; i++) {
                atomicAdd(sg + col[i], gv * val[i]);
                for (int j = 0; j < nz; j++) atomicAdd((PLAIN ? Bo : sH) + col[i] * nu + col[j], hv * val[i] * val[j]);
            }
        }
    }
    fb = wave_sum(fb);
    vm = wave_max(vm);
    wave_lds_sync();

    FSTAMP(6);
    // ---- Gaussian-mixture pose prior on the relative angles x[nu-D:] (acinoset_misc.py:680-714):
    // f = -log(sum_k w_k N(x; mu_k, Sigma_k) + 1e-12), curvature sum_k gamma_k P_k (responsibility-weighted precisions).  x = X' u with the constant X' of
    // the cost pitch, so the curvature in the reduced coordinates is sum_k gamma_k (X'^T P_k X'): a mix of K constant matrices of the model (DevPriors::gmm_Q),
    // the gradient X'^T sum_k gamma_k P_k (x - mu_k).  (Round 2 chained a state-dependent X' through two dense products in LDS: 58 % of this kernel's time with
    // the prior on, and 13.7 KB of its LDS -- four waves per CU.)
    double fpz = 0.0;
    if (pri && pri->p.gmm_k > 0) {
        const int K = pri->p.gmm_k, D = pri->p.gmm_dim, off = nu - D;
        double* sxv = sDp + 3 * mct;                         // scratch of the prior: behind the regular layout
        double* sv = sxv + CPE_NX;
        double* slp = sv + K * D;
        double* sgr = slp + CPE_MAX_GMM;
        if (lane < D) {
            const int k = off + lane, r = M->rel_ref_u[k];
            sxv[lane] = M->rel_sign_u[k] * (cost_coord(M, sq, k) - (r >= 0 ? cost_coord(M, sq, r) : 0.0));
        }
        wave_lds_sync();
        // (the tables of the prior sit in L2: a loop that loads one word per step waits ~700 cycles per step, and this wave shares its SIMD with one or two
        // others only -- stamps: 64 % of the kernel's chain with the prior on.  Every loop below requests a chunk of eight words, at clamped indices, before
        // it uses the first; the sums keep their order)
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
        double resp[CPE_MAX_GMM];                           // responsibilities exp(log p_k) / density: the same in every lane, computed once
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
        // two rounds of entries at a time, all components requested together (resp[k] = 0 past the last component: those terms add +0)
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

    FSTAMP(7);
    // ---- write out
    if (!PLAIN) for (int t = lane; t < nu * nu; t += WAVE) Bo[t] = sH[t];
    if (lane < nu) gbuf[fo * nu + lane] = sg[lane];
    if (lane == 0) {
        double* cb = costbuf + fo * COST_STRIDE;
        cb[0] = fc; cb[1] = fb; cb[2] = fpz; cb[3] = 0.0; cb[4] = vm; cb[5] = 0.0;
    }
    FSTAMP(8);
}

// --------------------------------------------------------------------------------------------------
// Linear autoregressive motion prior (acinoset_misc.py:291-336), one wave per frame a, AFTER k_frame_normal wrote the
// Euler angles and Gamma rows of the evaluated buffer:  slack_n = x_n - b - sum_{t<W} coef_t x_{n-W+t}  (n >= W),
// cost sum_p w_p slack_{n,p}^2.  Adds the exact gradient to gbuf, the diagonal Gauss-Newton block to Bbuf, writes the
// blocks (a, a-1..a-nk) to Hlr and the cost of slack_a to the frame's cost record.  x-space blocks: see DevPriors.
// x = X' u with the constant X' of the cost pitch: the blocks in the reduced coordinates are constants of the model too (DevPriors::lr_PKu, lr_HIu) --
// this kernel only picks and sums them (rounds 2-3 rebuilt X' per frame and multiplied X_a^T H_x X_b out in LDS: 1.7 ms per 51 200 frames).
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_lr_band(const DevModel* __restrict__ M, const SeqState* __restrict__ st, int N, int which,
                                                  size_t n_frames, const double* __restrict__ qbuf, const double* __restrict__ gambuf,
                                                  const DevPriors* __restrict__ pri, int nk, double* __restrict__ gbuf, double* __restrict__ Bbuf,
                                                  double* __restrict__ Hlr, double* __restrict__ costbuf, const int* __restrict__ act,
                                                  const int* __restrict__ n_act, RaggedArgs rg = RaggedArgs{}) {
    FrameSlot fs;
    if (!frame_slot<RAGGED>(N, act, n_act, rg, fs)) return;
    __shared__ double sx[(2 * CPE_MAX_WINDOW + 1) * CPE_NX];
    __shared__ double ssl[(CPE_MAX_WINDOW + 1) * CPE_NX];
    __shared__ double sgx[CPE_NX];
    __shared__ double sgu[CPE_NX];
    const int lane = threadIdx.x;
    const int b = fs.b, a = fs.n, NL = fs.len;           // N: the buffers' frames per sequence, NL: this sequence's length
    const size_t f = (size_t)b * N + a;
    M += fs.model;
    const SeqState S = st[b];
    if (S.status != 0) return;
    const int buf = (which || S.al_pending) ? S.cur : 1 - S.cur;
    const int nu = M->nu, ns = M->ns, W = pri->p.lr_window;
    const double* qs = qbuf + ((size_t)buf * n_frames + (size_t)b * N) * ns;           // the sequence's states
    (void)gambuf;
    const size_t fo = (size_t)buf * n_frames + f;

    // x of frames a-W .. a+W
    for (int t = lane; t < (2 * W + 1) * nu; t += WAVE) {
        const int d = t / nu, k = t - d * nu, n = a - W + d;
        double v = 0.0;
        if (n >= 0 && n < NL) {
            const double* qn = qs + (size_t)n * ns;
            const int r = M->rel_ref_u[k];
            v = M->rel_sign_u[k] * (cost_coord(M, qn, k) - (r >= 0 ? cost_coord(M, qn, r) : 0.0));
        }
        sx[t] = v;
    }
    wave_lds_sync();
    // 2 w slack_n for n = a .. a+W (zero where the term does not exist)
    double fl = 0.0;
    for (int t = lane; t < (W + 1) * nu; t += WAVE) {
        const int d = t / nu, p = t - d * nu, n = a + d;
        double sl = 0.0;
        if (n >= W && n < NL) {
            sl = sx[(d + W) * nu + p] - pri->p.lr_b[p];
            // over the features the model uses (ascending: the same order of the same non-zero products as the dense double loop)
            const double* xs = sx + d * nu;
            for (int e = 0; e < pri->lr_nf; e++) { const int ft = pri->lr_feat[e]; sl -= pri->lr_coefT[ft][p] * xs[ft]; }
        }
        const double w = pri->p.lr_w[p];
        if (d == 0) fl += w * sl * sl;
        ssl[t] = 2.0 * w * sl;
    }
    fl = wave_sum(fl);
    wave_lds_sync();
    // x-space gradient at frame a: sum_n K_{a-n+W}^T (2 w slack_n)
    if (lane < nu) {
        double gacc = ssl[lane];                                             // n = a: K_W = I
        for (int d = 1; d <= W; d++) {                                       // n = a + d: lag block t = W - d
            const int tt = W - d;
            const double* sn = ssl + d * nu;
            for (int p = 0; p < nu; p++) gacc -= pri->p.lr_coef[p][tt * nu + lane] * sn[p];
        }
        sgx[lane] = gacc;
    }
    wave_lds_sync();
    if (lane < nu) { double gacc = 0.0; for (int r = 0; r < nu; r++) gacc += pri->Xc[r][lane] * sgx[r]; sgu[lane] = gacc; }
    wave_lds_sync();
    if (lane < nu) gbuf[fo * nu + lane] += sgu[lane];
    const bool row_interior = a >= W && a <= NL - W;          // every block of the row is the constant lr_HIu[k]: k_lm_step reads the table, not Hlr
    for (int k = 0; k <= nk && k <= a; k++) {
        if (k > 0 && row_interior) break;
        // block (a, a - k): sum over the lags ta of frame a with tb = ta - k, terms n = a - ta + W inside [W, N-1]
        const int ta_lo = k > a - NL + 1 + W ? k : a - NL + 1 + W, ta_hi = W < a ? W : a;
        const bool interior = ta_lo == k && ta_hi == W;
        for (int t = lane; t < nu * nu; t += WAVE) {
            double v = 0.0;
            if (interior) v = pri->lr_HIu[k][t];
            else for (int ta = ta_lo; ta <= ta_hi; ta++) v += pri->lr_PKu[ta][ta - k][t];
            if (k == 0) Bbuf[fo * (nu * nu) + t] += v;
            else Hlr[(fo * nk + (k - 1)) * (nu * nu) + t] = v;
        }
    }
    if (lane == 0) costbuf[fo * COST_STRIDE + 5] = fl;
}

// The launch window of cpe_solve: the first `window` sequences that are still running, in index order, and their count.
// One workgroup; ballot prefix sums, so the list (and with it every later launch) is the same on every run.
__global__ __launch_bounds__(256) void k_build_act(const SeqState* __restrict__ st, int B, int window, int* __restrict__ act, int* __restrict__ n_act) {
    __shared__ int wcnt[4];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (in an SGPR: branches on it are scalar)
#ifdef CPE_LM_STAMPS
    unsigned long long* g_tu = nullptr;
#endif
    if (tid == 0) base = 0;
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + tid;
        const bool run = b < B && st[b].status == 0;
        const unsigned long long m = __ballot(run);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; w++) off += wcnt[w];
        const int idx = off + __popcll(m & ((1ull << lane) - 1ull));
        if (run && idx < window) act[idx] = b;
        __syncthreads();
        if (tid == 0) base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
        if (base >= window) break;      // uniform
    }
    if (tid == 0) *n_act = base < window ? base : window;
}

// Shutter delays (acinoset_misc.py:182-183: one per camera, camera 1 fixed to 0, |tau| <= h): one damped Newton step per camera with the
// trajectory held fixed -- d/dtau_c = sum_n t_n . rc_nc, d2/dtau_c2 ~ sum_n t_n^T Mc_nc t_n with t_n = v_n + 2 a_n tau_c, rc / Mc from
// k_frame_normal at the current iterate.  One workgroup per sequence, one wave per camera round; fixed summation order.  step = the Newton steps (the host mixes and clamps them).
__global__ __launch_bounds__(WAVE) void k_shutter_step(const DevModel* __restrict__ M, const SeqState* __restrict__ st, int N, size_t n_frames,
                                                       const double* __restrict__ qbuf, const double* __restrict__ rcb,
                                                       const double* __restrict__ tau, double* __restrict__ step /* [B][C] */) {
    const int b = blockIdx.x, lane = threadIdx.x, C = M->C, ns = M->ns;
    const int cur = st[b].cur;
    const double* qs = qbuf + ((size_t)cur * n_frames + (size_t)b * N) * ns;
    const double ih = 1.0 / M->h;
    if (lane == 0) step[(size_t)b * C] = 0.0;
    for (int c = 1; c < C; c++) {
        const double ta = tau[(size_t)b * C + c];
        double g = 0.0, hh = 0.0;
        for (int n = 2 + lane; n < N; n += WAVE) {
            const double* r = rcb + (((size_t)cur * n_frames + (size_t)b * N + n) * C + c) * 9;
            double t3[3];
            for (int d = 0; d < 3; d++) {
                const double x0 = qs[(size_t)n * ns + d], x1 = qs[(size_t)(n - 1) * ns + d], x2 = qs[(size_t)(n - 2) * ns + d];
                t3[d] = (x0 - x1) * ih + 2.0 * ta * (x0 - 2.0 * x1 + x2) * ih * ih;
            }
            g += t3[0] * r[0] + t3[1] * r[1] + t3[2] * r[2];
            hh += t3[0] * (r[3] * t3[0] + r[4] * t3[1] + r[5] * t3[2]) + t3[1] * (r[4] * t3[0] + r[6] * t3[1] + r[7] * t3[2]) + t3[2] * (r[5] * t3[0] + r[7] * t3[1] + r[8] * t3[2]);
        }
        g = wave_sum(g); hh = wave_sum(hh);
        if (lane == 0) step[(size_t)b * C + c] = hh > 0.0 ? -g / hh : 0.0;
    }
}

// gathers cpe_eval_normal's outputs out of the solver workspace (buffer 0)
__global__ void k_gather_normal(const DevModel* __restrict__ M, size_t F, const double* __restrict__ qbuf, const double* __restrict__ costbuf,
                                const double* __restrict__ gambuf, double* __restrict__ cost, double* __restrict__ gam, double* __restrict__ q_out) {
    const size_t f = blockIdx.x;
    const int t = threadIdx.x, nq = M->nq, ns = M->ns, GS = GAM_STRIDE * M->nrev;
    if (t < 3) cost[3 * f + t] = costbuf[f * COST_STRIDE + t];
    if (gam && t < GS) gam[f * GS + t] = gambuf[f * GS + t];
    if (q_out && t < nq) q_out[f * nq + t] = qbuf[f * ns + t];
}

// --------------------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_f64(double v, int l) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}

// T = D3^T D3 of the constant-acceleration model: T[i][i-k], D3 rows n = 3..N-1 with stencil (-1,3,-3,1)
__device__ __forceinline__ double motion_T(int i, int k, int N) {
    const double c[4] = {-1.0, 3.0, -3.0, 1.0};
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 4; t++)
        if (t >= k && t <= i && t >= i + 4 - N) s += c[t] * c[t - k];
    return s;
}

// LDS slot of block (row frame r, col frame c), r >= c, r - c < RING (ring over frame index mod RING): the RING
// diagonal blocks first, then the pairs (lo, hi) of ring positions in row-major order
template <int RING>
__device__ __forceinline__ int blk_slot(int r, int c) {
    const int ri = r % RING, ci = c % RING;
    if (ri == ci) return ri;
    const int lo = ri < ci ? ri : ci, hi = ri < ci ? ci : ri;
    return RING + lo * RING - lo * (lo + 1) / 2 + (hi - lo - 1);
}

// 1/sqrt(x) in full fp64 precision from the hardware estimate + two Newton steps (x > 0, normal range)
__device__ __forceinline__ double rsqrt_f64(double x) {
    double y = __builtin_amdgcn_rsq(x);
    y = y * (1.5 - 0.5 * x * y * y);
    y = y * (1.5 - 0.5 * x * y * y);
    return y;
}

// 1/x in full fp64 precision from the hardware estimate + two Newton steps (x > 0, normal range)
__device__ __forceinline__ double rcp_f64(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = y * fma(-x, y, 2.0);
    y = y * fma(-x, y, 2.0);
    return y;
}

// Diagonal-block Cholesky + panel solve by ONE wave, rows in lanes: lanes 0..27 hold the rows of the 28x28 diagonal block A (lower
// triangle), the other lanes hold panel rows x (rows of the identity, the right-hand side).  Right-looking elimination: with c = column k
// of the current matrix and piv = c[k],
//     row[j] -= (row[k] / piv) * c[j]   (j > k),        row[k] *= 1/sqrt(piv)
// turns the A rows into L (A = L L^T) and every panel row into x L^-T -- the same update for both kinds of rows, so the triangular
// solve rides along with the factorisation.  A row of the identity comes out as the same row of L^-T: that is how k_lm_step obtains the
// inverse factor for its matrix-core panel product.
// BLOCKED by four columns: inside a group the four pivot steps touch only the group's own columns (c[j] = register a[k] of lane j,
// v_readlane: at most three products per step), and the chain from one pivot to the next is a reciprocal (estimate + two Newton steps),
// two products and the broadcast; the rest of the row then takes the group's four updates at once, the four column values of every
// later row j read as one LDS broadcast (28 x 4 doubles, written once per group).  7 LDS exchanges and ~1 300 instructions per sweep where
// the column-at-a-time form had 28 and ~2 400.  The square roots are taken once, for all 28 pivots at the same time (lane k keeps
// pivot k), after the last step.  Returns false if a pivot is not positive.
__device__ __forceinline__ bool wave_factor_panel(const double* src, double* dst /* or nullptr */, bool store_lower_only,
                                                  double* colbuf /* [28][4], private to the wave */, double* invd_out /* or nullptr */, int lane,
                                                  int ident = -1 /* >= 0: this lane's row is row `ident` of the identity (src unused) */) {
    static_assert(NU % 4 == 0, "groups of four columns");
    double a[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) a[j] = src[j];
    if (ident >= 0) {
#pragma unroll
        for (int j = 0; j < NU; j++) a[j] = j == ident ? 1.0 : 0.0;
    }
    bool ok = true;
    double mypiv = 1.0;
#pragma unroll
    for (int g = 0; g < NU / 4; g++) {
        const int k0 = 4 * g;
        double t[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int k = k0 + c;
            double piv = readlane_f64(a[k], k);
            if (!(piv > 0.0)) { ok = false; piv = 1.0; }
            if (lane == k) mypiv = piv;
            t[c] = a[k] * rcp_f64(piv);
#pragma unroll
            for (int c2 = c + 1; c2 < 4; c2++) a[k0 + c2] = fma(-t[c], readlane_f64(a[k], k0 + c2), a[k0 + c2]);
        }
        if (k0 + 4 < NU) {
            if (lane < NU) {
#pragma unroll
                for (int c = 0; c < 4; c++) colbuf[lane * 4 + c] = a[k0 + c];
            }
            wave_lds_sync();
            // four rows at a time: their 16 column values are requested together, then four independent chains of four products
#pragma unroll
            for (int jb = k0 + 4; jb < NU; jb += 4) {
                double cc[4][4];
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int c = 0; c < 4; c++) cc[q][c] = colbuf[(jb + q) * 4 + c];
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int q = 0; q < 4; q++) a[jb + q] = fma(-t[c], cc[q][c], a[jb + q]);
            }
            // keep this group's updates inside the group: otherwise the compiler sinks the FMAs towards their first use and keeps every
            // broadcast alive.  The empty asm makes each a[j] "used" here at no instruction cost.
#pragma unroll
            for (int j = k0 + 4; j < NU; j++) asm volatile("" : "+v"(a[j]));
            wave_lds_sync();
        }
    }
    const double isp = rsqrt_f64(mypiv);                 // lane k < 28: 1 / L[k][k]
#pragma unroll
    for (int k = 0; k < NU; k++) a[k] *= readlane_f64(isp, k);
    if (invd_out && lane < NU) invd_out[lane] = isp;
    if (dst) {
#pragma unroll
        for (int j = 0; j < NU; j++)
            if (!store_lower_only || j <= lane) dst[j] = a[j];
    }
    return ok;
}

// fp64 matrix-core tiles (v_mfma_f64_16x16x4_f64: D[16][16] += A[16][4] B[4][16]; lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and
// holds D[(l >> 4) + 4 r][l & 15], r = 0..3).  A 28 x 28 block in LDS ([28][LDB]) is covered by 2 x 2 tiles; rows / columns 28..31 of the
// second tile read whatever follows in LDS -- they only reach results that are never stored.
typedef double d4_t __attribute__((ext_vector_type(4)));
// rows row0 .. row0+15 of a block as the A operand of the 7 k-steps (or, the same values, as the B operand of the product with the
// block's transpose): [row0 + (l & 15)][4 s + (l >> 4)]
__device__ __forceinline__ void mfma_frag_rows(const double* blk, int row0, int lane, double (&f)[7]) {
    const double* p = blk + (row0 + (lane & 15)) * LDB + (lane >> 4);
#pragma unroll
    for (int s = 0; s < 7; s++) f[s] = p[4 * s];
}
// columns col0 .. col0+15 of a block as the B operand: [4 s + (l >> 4)][col0 + (l & 15)]
__device__ __forceinline__ void mfma_frag_cols(const double* blk, int col0, int lane, double (&f)[7]) {
    const double* p = blk + (lane >> 4) * LDB + col0 + (lane & 15);
#pragma unroll
    for (int s = 0; s < 7; s++) f[s] = p[4 * s * LDB];
}

// Window blocks of k_lm_step resident in LDS: the whole window up to PB = 5 (21 blocks, 136 KB).  From PB = 6 on the slots past these
// live in global memory (a per-sequence area behind the factor columns in Lbuf, L2-resident): win_blk maps a slot to its place.
#define LM_LDS_BLOCKS 21
// doubles of global memory per sequence for the window blocks of k_lm_step<PB> past LM_LDS_BLOCKS, with room for the tiles' over-read (the
// fragment of rows 16..31 of a block reads up to 115 doubles past its end; those rows only reach results that are never stored)
__host__ __device__ constexpr size_t lm_spill_doubles(int pb) {
    return (pb + 1) * (pb + 2) / 2 <= LM_LDS_BLOCKS ? 0 : (size_t)((pb + 1) * (pb + 2) / 2 - LM_LDS_BLOCKS) * BLK + 4 * LDB;
}
template <int RING>
__device__ __forceinline__ double* win_blk(double* W, double* Wg, int slot) {
    constexpr int NLDS = RING * (RING + 1) / 2 < LM_LDS_BLOCKS ? RING * (RING + 1) / 2 : LM_LDS_BLOCKS;
    if constexpr (RING * (RING + 1) / 2 <= LM_LDS_BLOCKS) { (void)Wg; return W + slot * BLK; }
    else return slot < NLDS ? W + slot * BLK : Wg + (slot - NLDS) * BLK;
}

// LDS slot of block (row frame r, col frame c) -- defined above (blk_slot).  CNT tiles (idx = g0 .. g0+CNT-1: block j = 1 + idx / 2, column
// half idx & 1) of the trailing update of half panel (i, tr): A_ij -= X_i X_j^T with CNT independent accumulators in flight (a dependent
// fp64 MFMA waits ~116 cycles, an independent one issues every ~64)
template <int RING, int CNT>
__device__ __forceinline__ void p2_tiles(double* W, int n, int i, int tr, int g0, const double (&xa)[7], int lane, double* Wg = nullptr) {
    constexpr int SPLIT = CNT <= 2 ? 2 : 1;            // one or two tiles: the 7 k-steps of a tile go to two accumulators (even / odd), four chains in flight
    double xb[CNT][7];
    d4_t acc[CNT][SPLIT];
#pragma unroll
    for (int q = 0; q < CNT; q++) {
        const int idx = g0 + q;
        mfma_frag_rows(win_blk<RING>(W, Wg, blk_slot<RING>(n + 1 + idx / 2, n)), 16 * (idx & 1), lane, xb[q]);
#pragma unroll
        for (int h = 0; h < SPLIT; h++) acc[q][h] = d4_t{0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll
    for (int s2 = 0; s2 < 7; s2++)
#pragma unroll
        for (int q = 0; q < CNT; q++) acc[q][s2 % SPLIT] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s2], xb[q][s2], acc[q][s2 % SPLIT], 0, 0, 0);
#pragma unroll
    for (int q = 0; q < CNT; q++) {
        const int idx = g0 + q, j = 1 + idx / 2, col = 16 * (idx & 1) + (lane & 15);
        double* Cd = win_blk<RING>(W, Wg, blk_slot<RING>(n + i, n + j));
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * tr + (lane >> 4) + 4 * r;
            const double v = SPLIT == 2 ? acc[q][0][r] + acc[q][SPLIT - 1][r] : acc[q][0][r];
            if (row < NU && col < NU) Cd[row * LDB + col] -= v;
        }
    }
}

// --------------------------------------------------------------------------------------------------
// One LM step per sequence: (1) accept / reject the pending trial, (2) assemble H = blockdiag(B_n) +
// motion band + lambda diag(H), factor it with a sliding-window block Cholesky in LDS, (3) solve,
// (4) write the next trial iterate.  One 256-thread workgroup per sequence.  PB = half-bandwidth in frames: 3 for the
// constant-acceleration model (2 workgroups per CU), W = 4..6 when the window-W autoregressive prior is on (1 per CU).  The window's
// (PB+1)(PB+2)/2 blocks sit in LDS up to PB = 5; from PB = 6 on the slots past LM_LDS_BLOCKS are in global memory (win_blk).
// MODE 0: the whole step.  The physics-based model puts kernels between the two halves (the elimination of the node forces needs the
// damping the accept step has just set): MODE 1 = accept / reject only, MODE 2 = assemble, factor, solve, trial only.
// hb = number of buffers of gbuf / Bbuf / Hlr: 2 (indexed by the current buffer) or 1 (already those of the current iterate).
template <int PB, int MODE = 0, bool RAGGED = false>
__global__ __launch_bounds__(LM_THREADS, PB == 3 ? 2 : 1) void k_lm_step(const DevModel* __restrict__ M, SeqState* __restrict__ st,
                                                        LmParams prm, int first, double* __restrict__ qbuf,
                                                        const double* __restrict__ gbuf, const double* __restrict__ Bbuf,
                                                        const double* __restrict__ costbuf, double* __restrict__ Lbuf,
                                                        double* __restrict__ zbuf, double* __restrict__ gtbuf,
                                                        const double* __restrict__ gambuf, const double* __restrict__ Hlr,
                                                        const int* __restrict__ act /* sequences of this launch, or null = all */,
                                                        const int* __restrict__ n_act /* entries of act in use, or null */, int hb = 2,
                                                        const double* __restrict__ gxbuf = nullptr /* shutter delay: cross-frame gradient parts [2][F][6], or null */,
                                                        double* __restrict__ dgbuf = nullptr /* [F][NU]: diagonal of H before damping, for k_lm_back */,
                                                        const double* __restrict__ HIu = nullptr /* motion prior: DevPriors::lr_HIu[1], the constant blocks of a frame away from the sequence ends */,
                                                        int lrW = 0 /* its window */, RaggedArgs rg = RaggedArgs{}) {
    if (n_act && (int)blockIdx.x >= *n_act) return;     // uniform: the whole workgroup leaves
    constexpr int RING = PB + 1;                       // frames in the sliding window
    constexpr int NBLK = RING * (RING + 1) / 2;        // lower-triangle blocks of the window
    constexpr int NRH = 2 * PB;                        // half panels (16 rows) below the diagonal block: (i, tr), i = 1..PB, index 2 (i - 1) + tr
    constexpr int NLDS = NBLK < LM_LDS_BLOCKS ? NBLK : LM_LDS_BLOCKS, NSPILL = NBLK - NLDS;     // window blocks in LDS / in global memory
    static_assert(PB >= 3 && PB <= 6, "the tile deal of P2 below is written for PB = 3..6");
    __shared__ double W[NLDS * BLK];
    __shared__ __attribute__((aligned(16))) double colbuf[NU * 4];     // the four columns of a pivot group, rows in order (factor sweep, wave 0 only)
    __shared__ double dummy_row[NU + 4];     // sink for idle lanes of the factor sweep
    __shared__ double Tm[BLK + 4 * LDB];     // L00^-T of the current diagonal block (upper triangular), padded for the tiles' rows 28..31
    __shared__ double smw[NU];               // 2/h^4 * motion weight per reduced dof
    __shared__ int sindep[NU];
    constexpr int RG = RING + 1;             // Gamma ring: one slot more than the window, the row being staged runs ahead of the row being stored
    __shared__ double gamw[RG * LM_MAX_REV * GAM_STRIDE];      // Gamma rows of the frames in the window (ring)
    __shared__ double marr[2 * NU];          // Euler-space motion gradient of the row being loaded ([m & 1])
    __shared__ double sgc[2 * NU];           // per-frame gradient of the row being loaded ([m & 1])
    __shared__ int s_cnt[4];                 // look-ahead counters (monotonic): 0 factor sweeps done, 1 rows staged, 2 priority parts of the update done (x3), 3 update-wave barrier
    __shared__ int mterm[LM_MAX_TERMS + LM_MAX_GROUP];      // product terms of the motion model's Gauss-Newton block (packed, see below)
    __shared__ int srev_of_u[NU], sja[NU], srev_u[LM_MAX_REV], srbu[LM_MAX_REV * 3], slegs_n[NU], slegs[NU * LM_MAX_LEGS];
    __shared__ int scoord_of_state[CPE_MAX_NQ + CPE_MAX_JOINTS];
    __shared__ double rw[RING * NU];
    __shared__ double invd[NU];
    __shared__ double red[16];
    __shared__ int s_int[4];
    __shared__ double s_dbl[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (in an SGPR: branches on it are scalar)
#ifdef CPE_LM_STAMPS
    unsigned long long* g_tu = nullptr;
#endif
    const int b = act ? act[blockIdx.x] : (int)blockIdx.x, NS = prm.N;       // NS: the buffers' frames per sequence
    int N = NS;                                                                // N: this sequence's length
    if constexpr (RAGGED) { const int2 rs = rg.seq[b]; M += rs.x; N = rs.y; }
    const int nq = M->ns;     // NOTE: nq is the STATE stride here (Euler q + leg angles)
    const int nrev = M->nrev, GS = GAM_STRIDE * nrev;
    const size_t n_frames = (size_t)prm.B * NS;
    SeqState S = st[b];
    if (S.status != 0) return;
#ifdef CPE_LM_STAMPS
    unsigned long long t_last = __builtin_amdgcn_s_memtime();
#endif

    if (MODE == 2) { if (S.al_pending) return; }
    // ---------------- (1) cost of the evaluated buffer, accept / reject
    if (MODE != 2) {
        const int mode = first ? 1 : (S.al_pending ? 2 : 0);     // 1/2: the CURRENT buffer was (re-)evaluated
        const int eb = mode ? S.cur : 1 - S.cur;
        const double* cb = costbuf + ((size_t)eb * n_frames + (size_t)b * NS) * COST_STRIDE;
        const double* qe = qbuf + (size_t)eb * n_frames * nq + (size_t)b * NS * nq;
        double acc[6] = {0, 0, 0, 0, 0, 0};   // meas, model, bound, pose, clamped, autoregressive prior
        double vmax = 0.0;
        for (int n = tid; n < N; n += LM_THREADS) {
            const double* c = cb + (size_t)n * COST_STRIDE;
            acc[0] += c[0]; acc[2] += c[1]; acc[3] += c[2]; acc[4] += c[3]; acc[5] += c[5]; vmax = fmax(vmax, c[4]);
        }
        for (int t = tid; t < N * NU; t += LM_THREADS) {
            const int n = t / NU, k = t - n * NU;
            const double wk = M->motion_w_u[k];
            if (n >= 3 && wk != 0.0) {
                const double* qf = qe + (size_t)n * nq;              // (cost pitch for the leg links: cost_coord)
                const double e = (cost_coord(M, qf, k) - 3.0 * cost_coord(M, qf - nq, k) + 3.0 * cost_coord(M, qf - 2 * nq, k) - cost_coord(M, qf - 3 * nq, k)) * M->ih2;
                acc[1] += wk * e * e;
            }
        }
        double tot[6];
        for (int v = 0; v < 6; v++) {
            double x = wave_sum(acc[v]);
            __syncthreads();
            if (lane == 0) red[wave] = x;
            __syncthreads();
            tot[v] = red[0] + red[1] + red[2] + red[3];
        }
        vmax = wave_max(vmax);
        __syncthreads();
        if (lane == 0) red[wave] = vmax;
        __syncthreads();
        vmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        if (tid == 0) {
            double total = tot[0] + tot[1] + tot[2] + tot[3] + tot[5];
            if (tot[4] > 0.0 || !isfinite(total)) total = INFINITY;
            bool inner_done = false;
            if (mode == 1) {
                S.cost_cur = total; S.lambda = prm.lambda0; S.nu = LM_NU0; S.iters = 0; S.rejects = 0; S.outer = 0; S.al_pending = 0; S.fresh = 1;
                S.maxviol = vmax;
                S.terms[0] = tot[0]; S.terms[1] = tot[1]; S.terms[2] = tot[2]; S.terms[3] = tot[3]; S.terms[4] = tot[5];
                if (!isfinite(total)) S.status = 2;
            } else if (mode == 2) {
                S.cost_cur = total; S.maxviol = vmax; S.al_pending = 0; S.nu = LM_NU0; S.fresh = 1;
                if (S.lambda > 1e-3) S.lambda = 1e-3;
                S.terms[0] = tot[0]; S.terms[1] = tot[1]; S.terms[2] = tot[2]; S.terms[3] = tot[3]; S.terms[4] = tot[5];
            } else {
                S.iters++;
                const double act = S.cost_cur - total;
                const double gain = S.pred > 0.0 ? act / S.pred : -1.0;
                if (isfinite(total) && act > 0.0 && gain > 1e-4) {
                    const double rel = act / (fabs(S.cost_cur) + 1e-30);
                    S.cur = 1 - S.cur; S.cost_cur = total; S.maxviol = vmax; S.fresh = 1;
                    S.terms[0] = tot[0]; S.terms[1] = tot[1]; S.terms[2] = tot[2]; S.terms[3] = tot[3]; S.terms[4] = tot[5];
                    const double t3 = 2.0 * gain - 1.0, fl = 1.0 - t3 * t3 * t3;
                    S.lambda *= fl > 1.0 / 3.0 ? fl : 1.0 / 3.0; S.nu = LM_NU0;
                    if (S.lambda < 1e-12) S.lambda = 1e-12;
                    if (S.maxstep < prm.tol_step || rel < prm.tol_cost) inner_done = true;
                } else {
                    S.lambda *= S.nu; S.nu *= 2.0; S.rejects++; S.fresh = 0;        // the pieces of the current iterate stand
                    if (S.maxstep < prm.tol_step * 1e-2 || S.lambda > 1e14) inner_done = true;
                }
            }
            if (inner_done) {
                if (S.maxviol > prm.bound_tol && S.outer < prm.max_outer) { S.outer++; S.al_pending = 1; }
                else S.status = 1;
            }
            if (S.status == 0 && !S.al_pending && S.iters >= prm.max_iter) S.status = 3;   // iteration limit
            st[b] = S;
            s_int[0] = S.cur; s_int[1] = S.status; s_int[3] = S.al_pending; s_dbl[0] = S.lambda;
        }
        __syncthreads();
        S.cur = s_int[0]; S.status = s_int[1]; S.lambda = s_dbl[0];
        if (S.status != 0 || s_int[3]) return;
    }
    if (MODE == 1) return;

    STAMP(0);
    // ---------------- (2) forward: sliding-window block Cholesky + forward substitution
    const int cur = S.cur;
    const double lam = S.lambda;
    const double* qc = qbuf + (size_t)cur * n_frames * nq + (size_t)b * NS * nq;
    const size_t hcur = hb == 2 ? (size_t)cur * n_frames : 0;
    const double* gc = gbuf + (hcur + (size_t)b * NS) * NU;
    const double* Bc = Bbuf + (hcur + (size_t)b * NS) * (NU * NU);
    double* Lb = Lbuf + (size_t)b * NS * RING * (NU * NU);
    double* Wg = nullptr;                                    // the window blocks past NLDS: this sequence's area behind the factor columns
    if constexpr (NSPILL > 0) Wg = Lbuf + n_frames * RING * (NU * NU) + (size_t)b * lm_spill_doubles(PB);
    double* zb = zbuf + (size_t)b * NS * NU;
    double* gtb = gtbuf + (size_t)b * NS * NU;
    double* dgb = dgbuf + (size_t)b * NS * NU;
    const double mscale = 2.0 * M->ih2 * M->ih2;

    if (tid < NU) {
        smw[tid] = mscale * M->motion_w_u[tid]; sindep[tid] = M->ucost[tid];
        srev_of_u[tid] = M->rev_of_u[tid]; sja[tid] = M->bodyang_j[tid]; slegs_n[tid] = M->bodyang_legs_n[tid];
        for (int i = 0; i < M->bodyang_legs_n[tid]; i++) slegs[tid * LM_MAX_LEGS + i] = M->bodyang_legs[tid][i];
    }
    if (tid < nrev) { srev_u[tid] = M->rev_u[tid]; for (int a = 0; a < 3; a++) srbu[3 * tid + a] = M->rev_body_u[tid][a]; }
    for (int t = tid; t < nq; t += LM_THREADS) scoord_of_state[t] = -1;
    __syncthreads();
    if (tid < NU) scoord_of_state[M->ucoord_src[tid]] = tid;
    const double* gamc = gambuf + ((size_t)cur * n_frames + (size_t)b * NS) * GS;
    const double* Hlc = Hlr ? Hlr + (hcur + (size_t)b * NS) * PB * (NU * NU) : nullptr;
    __syncthreads();

    // motion-model Gauss-Newton term of element (i, j) of block (frame a, frame b): sum_p Gamma_a[p][i] w_p Gamma_b[p][j]
    // over the weighted Euler dofs p (Gamma = d Euler / d coordinate: identity rows for the trunk, 4 entries per leg pitch)
    auto mot = [&](int i, int j, const double* Ga, const double* Gb) -> double {
        const int ri = srev_of_u[i], rj = srev_of_u[j];
        if (ri >= 0 && rj >= 0) return ri == rj ? Ga[GAM_STRIDE * ri] * smw[i] * Gb[GAM_STRIDE * ri] : 0.0;
        if (ri >= 0) { const int jb = sja[j]; return (jb >= 0 && srbu[3 * ri + jb] == j) ? Ga[GAM_STRIDE * ri] * smw[i] * Gb[GAM_STRIDE * ri + 1 + jb] : 0.0; }
        if (rj >= 0) { const int ja = sja[i]; return (ja >= 0 && srbu[3 * rj + ja] == i) ? Ga[GAM_STRIDE * rj + 1 + ja] * smw[j] * Gb[GAM_STRIDE * rj] : 0.0; }
        double v = i == j ? smw[i] : 0.0;
        const int ja = sja[i], jb = sja[j];
        if (ja >= 0 && jb >= 0)
            for (int e = 0; e < slegs_n[i]; e++) {
                const int r = slegs[i * LM_MAX_LEGS + e];
                if (srbu[3 * r + jb] == j) v += Ga[GAM_STRIDE * r + 1 + ja] * smw[srev_u[r]] * Gb[GAM_STRIDE * r + 1 + jb];
            }
        return v;
    };

    // The three update waves (threads ut = 0 .. 191) own the window rows: element t = ut + 192 j of every 28 x 28 block belongs to thread ut.
    // B_m (28x28, HBM) is fetched into registers one column ahead.
    constexpr int UT = LM_THREADS - WAVE, NPB = (NU * NU + UT - 1) / UT;
    const int ut = tid - WAVE;
    double pb[NPB], pbh = 0.0;                               // pbh: B_m at this thread's heavy element (below), if it has one
    int hcnt = 0, ht = 0;

    // Synchronisation of the look-ahead (LDS counters, polled): wave 0 and the update waves meet through s_cnt, never at s_barrier
    // (with window blocks in global memory the fences order those too)
    auto lds_release = [&]() {
        if constexpr (NSPILL > 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    };
    auto wait_ge = [&](int idx, int target) {
        while (__atomic_load_n(&s_cnt[idx], __ATOMIC_RELAXED) < target) __builtin_amdgcn_s_sleep(1);
        if constexpr (NSPILL > 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    };
    int sync_epoch = 0;
    auto sync3 = [&]() {                                  // barrier of the three update waves
        lds_release();
        if (lane == 0) atomicAdd(&s_cnt[3], 1);
        sync_epoch += 3;
        wait_ge(3, sync_epoch);
    };
    // The motion model's Gauss-Newton term Gamma_a^T W Gamma_b touches the same sparse set of elements in every block: the
    // diagonal, leg x its body's angles, and pairs of angles of one body.  It is flattened once per launch into ~210
    // product terms  w[wi] * Gamma_a[oa] * Gamma_b[ob]  (offset 63 = factor 1), packed oa<<10 | ob<<16 | wi<<22, the terms of one
    // element consecutive in the list; the element's OWNER thread keeps (first, count) in a register and sums them in list order
    // when it stores the element: no atomics, no pass over the window after the dense store, and a solve is reproducible bit for
    // bit (the order of the elements in the list does not enter any sum).
    // (Evaluating the pattern per element inside the frame loop made the compiler hoist dozens of LDS table addresses and spill them.)
    if (tid == 0) { s_int[0] = 0; s_int[1] = 0; }
    __syncthreads();
    // element classes: no term, ONE term (its code stays in a register of the owner, bit 28 set) or SEVERAL (the 18 pairs of angles of a body
    // with legs: bit 29; such an element is handed to a dedicated thread h = position in the heavy list, 8 list words each: codes, then count << 16 | t)
    constexpr int HEAVY_MAX = (LM_MAX_TERMS + LM_MAX_GROUP) / 8;
    // The elements are then DEALT AGAIN so that the ones with a term (about 210 of 784) sit in the first slots of every thread and the
    // rest -- a plain copy of B_m or a zero -- in the last ones, which take a short path: code words through a list in the (still
    // unused) window, terms from the front, the others from the back.
    int* elist = reinterpret_cast<int*>(W);                  // [NU * NU]
    if (tid == 0) { s_int[1] = 0; s_int[3] = 0; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPB; j++) {
        const int t = ut + UT * j;
        if (ut >= 0 && t < NU * NU) {
            const int a = t / NU, c = t - a * NU;
            const int ri = srev_of_u[a], rj = srev_of_u[c];
            int codes[LM_MAX_GROUP], cnt = 0;
            auto emit = [&](int oa, int ob, int wi) { if (cnt < LM_MAX_GROUP) codes[cnt++] = (oa << 10) | (ob << 16) | (wi << 22); };
            if (ri >= 0 && rj >= 0) { if (ri == rj) emit(GAM_STRIDE * ri, GAM_STRIDE * ri, a); }
            else if (ri >= 0) { const int jb = sja[c]; if (jb >= 0 && srbu[3 * ri + jb] == c) emit(GAM_STRIDE * ri, GAM_STRIDE * ri + 1 + jb, a); }
            else if (rj >= 0) { const int ja = sja[a]; if (ja >= 0 && srbu[3 * rj + ja] == a) emit(GAM_STRIDE * rj + 1 + ja, GAM_STRIDE * rj, c); }
            else {
                if (a == c) emit(63, 63, a);
                const int ja = sja[a], jb = sja[c];
                if (ja >= 0 && jb >= 0)
                    for (int e = 0; e < slegs_n[a]; e++) {
                        const int r = slegs[a * LM_MAX_LEGS + e];
                        if (srbu[3 * r + jb] == c) emit(GAM_STRIDE * r + 1 + ja, GAM_STRIDE * r + 1 + jb, srev_u[r]);
                    }
            }
            const int where = (a * LDB + c) | (a == c ? 1 << 30 : 0);     // bits 0-9: position in a block, bit 30: on the diagonal
            if (cnt == 0) elist[NU * NU - 1 - atomicAdd(&s_int[3], 1)] = where;
            else if (cnt == 1) elist[atomicAdd(&s_int[1], 1)] = where | codes[0] | (1 << 28);
            else {
                const int h = atomicAdd(&s_int[0], 1);       // (a list that would overflow fails the step below instead of dropping terms)
                if (h < HEAVY_MAX) {
                    for (int g = 0; g < LM_MAX_GROUP; g++) mterm[8 * h + g] = g < cnt ? codes[g] : 0;
                    mterm[8 * h + 7] = (cnt << 16) | t;          // (t < 1024)
                }
            }
        }
    }
    __syncthreads();
    const int n_term = s_int[1], n_plain = s_int[3];
    (void)n_plain;
    const int npa = (n_term + UT - 1) / UT;                  // slots j < npa of a thread may hold an element with a term (uniform)
    int my_code[NPB];                                        // bit 31: the slot is empty
    auto elem_of = [&](int code) -> int { const int off = code & 1023; return (off / LDB) * NU + off % LDB; };   // element index t from the place in a block
#pragma unroll
    for (int j = 0; j < NPB; j++) {
        const int i = ut + UT * j;
        int code = 1 << 31;
        if (ut >= 0) {
            if (i < n_term) code = elist[i];
            else if (i - n_term < n_plain) code = elist[NU * NU - 1 - (i - n_term)];
        }
        my_code[j] = code;
    }
    auto fetch_B = [&](int m) {                              // B_m (28x28, HBM) is fetched into registers one column ahead
#pragma unroll
        for (int j = 0; j < NPB; j++) if (my_code[j] >= 0) pb[j] = Bc[(size_t)m * (NU * NU) + elem_of(my_code[j])];
        if (hcnt > 0) pbh = Bc[(size_t)m * (NU * NU) + ht];
    };
    __syncthreads();
    const int n_heavy = s_int[0];
    const bool list_ok = n_heavy <= HEAVY_MAX && n_heavy <= WAVE;
    // the extra work of a row is dealt to different waves: heavy element h to thread h of the SECOND update wave, the gradient of coordinate k to
    // thread k of the THIRD (the first keeps the right-hand-side updates of P2)
    const int hsel = ut - WAVE, gsel = ut - 2 * WAVE;
    int hcode[LM_MAX_GROUP];                                 // this thread's heavy element (hcnt terms, element ht), if any
#pragma unroll
    for (int g = 0; g < LM_MAX_GROUP; g++) hcode[g] = 0;
    if (list_ok && hsel >= 0 && hsel < n_heavy) {
#pragma unroll
        for (int g = 0; g < LM_MAX_GROUP; g++) hcode[g] = mterm[8 * hsel + g];
        hcnt = mterm[8 * hsel + 7] >> 16; ht = mterm[8 * hsel + 7] & 0xffff;
    }
    // coordinate-space motion gradient of coordinate gsel (< 28): Gamma_m^T (Euler-space gradient) = own entry (x Gamma[r][0] for a leg) plus, for
    // an angle of a body with legs, one product per leg -- (offset in the Gamma row) | (Euler-space index) << 8, in registers
    int gl[LM_MAX_LEGS], gl_n = 0, gl_own = -1;              // gl_own: offset of the leg's own Gamma entry, or -1 (factor 1)
#pragma unroll
    for (int e = 0; e < LM_MAX_LEGS; e++) gl[e] = 0;
    if (gsel >= 0 && gsel < NU) {
        const int r = srev_of_u[gsel];
        if (r >= 0) gl_own = GAM_STRIDE * r;
        else {
            const int ja = sja[gsel];
            if (ja >= 0) {
                gl_n = slegs_n[gsel];
#pragma unroll
                for (int e = 0; e < LM_MAX_LEGS; e++)
                    if (e < gl_n) { const int rr = slegs[gsel * LM_MAX_LEGS + e]; gl[e] = (GAM_STRIDE * rr + 1 + ja) | (srev_u[rr] << 8); }
            }
        }
    }
    // Gamma rows, Euler-space motion gradient and per-frame gradient of frame m, staged into LDS by ONE wave ahead of
    // store_row (wave 3 is idle during the factor/panel sweep for PB = 3): no global-load latency inside store_row
    // (two halves: the global loads go out before wave 0's factor sweep, the values are used after it)
    double st_gam = 0.0, st_tu = 0.0, st_gv = 0.0;
    auto stage_load = [&](int m) {
        st_gam = lane < GS ? gamc[(size_t)m * GS + lane] : 0.0;
        if (lane < NU) {
            const int p = sindep[lane] & 255, p2 = (sindep[lane] >> 8) - 1;      // cost value of the coordinate: state[p] (+ state[p2]: theta_B + alpha)
            double tu = 0.0;
#pragma unroll
            for (int j = -3; j <= 3; j++) {
                const int mj = m + j;
                if (mj < 0 || mj >= N) continue;
                const double T = j <= 0 ? motion_T(m, -j, N) : motion_T(mj, j, N);
                tu += T * (qc[(size_t)mj * nq + p] + (p2 >= 0 ? qc[(size_t)mj * nq + p2] : 0.0));          // cost value of the weighted dof
            }
            st_tu = tu;
            double gv = gc[(size_t)m * NU + lane];
            if (gxbuf && lane < 3) {        // the residuals of frames m+1, m+2 also depend on this frame's base position (shutter delay)
                const double* gxc = gxbuf + ((size_t)cur * n_frames + (size_t)b * NS) * 6;
                if (m + 1 < N) gv += gxc[(size_t)(m + 1) * 6 + lane];
                if (m + 2 < N) gv += gxc[(size_t)(m + 2) * 6 + 3 + lane];
            }
            st_gv = gv;
        }
    };
    auto stage_store = [&](int m) {
        if (lane < GS) gamw[(m % RG) * GS + lane] = st_gam;
        if (lane < NU) { marr[(m & 1) * NU + lane] = smw[lane] * st_tu; sgc[(m & 1) * NU + lane] = st_gv; }
    };
    // stores the window row of frame m: blocks (m, m-PB..m) from pb, the motion term and the damping, and the rhs -g_total(m); stage_row(m)
    // came first.  Executed by the three update waves; every element is computed and stored by its owner, so there is no step in between
    // that the waves would have to wait for.
    auto store_row = [&](int m) {
        const double* Gm = gamw + (m % RG) * GS;
        // the same for every element: band factors of the motion model and the blocks' places in the window
        double Tk[4];
        int base[PB + 1];
#pragma unroll
        for (int k = 0; k <= 3; k++) Tk[k] = m - k >= 0 ? motion_T(m, k, N) : 0.0;
#pragma unroll
        for (int k = 0; k <= PB; k++) base[k] = blk_slot<RING>(m, m - k >= 0 ? m - k : m) * BLK;
        const double* Gk[4];
#pragma unroll
        for (int k = 0; k <= 3; k++) Gk[k] = gamw + ((m - k >= 0 ? m - k : m) % RG) * GS;
        // one element of the row: value of the diagonal block (with damping; the undamped diagonal goes to k_lm_back) and of the PB blocks left of
        // it.  Two copies of the code, chosen once per row: a conditional load of the prior's blocks inside the element would leave an
        // s_waitcnt vmcnt(0) at every merge point -- also when there is no prior -- and each would drain the factor stores of P1.
        const bool prior = Hlc != nullptr;
        // the prior's blocks of row m: away from the sequence ends (k_lr_band's `interior`, for every k) they are constants of the model, read from the
        // 25 KB table that stays in L2 instead of 25 KB of HBM per frame; k_lr_band writes Hlr for the other rows only
        const double* Hrow = prior ? ((HIu && m >= lrW && m <= N - lrW) ? HIu : Hlc + (size_t)m * PB * (NU * NU)) : nullptr;
        auto wput = [&](int bo, int off, double v) {                // an off-diagonal block of the row (the diagonal one is always in LDS)
            if constexpr (NSPILL == 0) W[bo + off] = v;
            else { if (bo < NLDS * BLK) W[bo + off] = v; else Wg[bo - NLDS * BLK + off] = v; }
        };
        auto put = [&](int t, int where, double bval, const double (&acc)[4]) {
            const int off = where & 1023;
            double v = bval + Tk[0] * acc[0];
            if (where & (1 << 30)) { dgb[(size_t)m * NU + off / (LDB + 1)] = v; v += lam * fmax(v, LM_DIAG_FLOOR(N)); }
            W[base[0] + off] = v;
            if (prior) {
#pragma unroll
                for (int k = 1; k <= PB; k++)
                    if (m - k >= 0) wput(base[k], off, Hrow[(k - 1) * (NU * NU) + t] + (k <= 3 ? Tk[k] * acc[k] : 0.0));
            } else {
#pragma unroll
                for (int k = 1; k <= PB; k++)
                    if (m - k >= 0) wput(base[k], off, k <= 3 ? Tk[k] * acc[k] : 0.0);
            }
        };
#pragma unroll
        for (int j = 0; j < NPB; j++) {
            int code = my_code[j];
            asm volatile("" : "+v"(code));                        // (what derives from the code word -- a dozen offsets and addresses per element -- is recomputed here, not kept in registers across the column loop)
            if (code >= 0) {
                const int t = prior ? elem_of(code) : 0;          // (only the prior's blocks are addressed by element index)
                if (j < npa) {
                    // (every LDS read unconditional, at a clamped index: a select around a read becomes a branch with its own wait)
                    const int oa = (code >> 10) & 63, ob = (code >> 16) & 63, wi = (code >> 22) & 31;
                    const int oac = oa == 63 ? 0 : oa, obc = ob == 63 ? 0 : ob;
                    const double sw = smw[wi], ga = Gm[oac];
                    double gb[4];
#pragma unroll
                    for (int k = 0; k <= 3; k++) gb[k] = Gk[k][obc];
                    const double wa = (code & (1 << 28)) ? sw * (oa == 63 ? 1.0 : ga) : 0.0;
                    double acc[4];
#pragma unroll
                    for (int k = 0; k <= 3; k++) acc[k] = wa * (ob == 63 ? 1.0 : gb[k]);
                    put(t, code, pb[j], acc);
                } else {
                    const double acc[4] = {0.0, 0.0, 0.0, 0.0};         // no term: B_m on the diagonal block, zero (or the prior) beside it
                    put(t, code, pb[j], acc);
                }
            }
        }
        RSTAMP(14);
        if (hcnt > 0) {
            // every operand of the up to 7 terms is requested before the first is used; the sum runs in list order
            double sw[LM_MAX_GROUP], ga[LM_MAX_GROUP], gb[LM_MAX_GROUP][4];
            int hc[LM_MAX_GROUP];
#pragma unroll
            for (int g = 0; g < LM_MAX_GROUP; g++) { hc[g] = hcode[g]; asm volatile("" : "+v"(hc[g])); }
#pragma unroll
            for (int g = 0; g < LM_MAX_GROUP; g++) {
                const int oa = (hc[g] >> 10) & 63, ob = (hc[g] >> 16) & 63, wi = (hc[g] >> 22) & 31;
                sw[g] = smw[wi]; ga[g] = Gm[oa == 63 ? 0 : oa];
#pragma unroll
                for (int k = 0; k <= 3; k++) gb[g][k] = Gk[k][ob == 63 ? 0 : ob];
            }
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int g = 0; g < LM_MAX_GROUP; g++) {
                const int oa = (hc[g] >> 10) & 63, ob = (hc[g] >> 16) & 63;
                const bool on = g < hcnt;                       // entries past the element's terms contribute exactly 0
                const double wa = on ? sw[g] * (oa == 63 ? 1.0 : ga[g]) : 0.0;
#pragma unroll
                for (int k = 0; k <= 3; k++) acc[k] += wa * (ob == 63 || !on ? 1.0 : gb[g][k]);
            }
            const int a = ht / NU, c = ht - a * NU;
            put(ht, (a * LDB + c) | (a == c ? 1 << 30 : 0), pbh, acc);
        }
        RSTAMP(15);
        if (gsel >= 0 && gsel < NU) {
            // coordinate-space gradient: Gamma_m^T (Euler-space gradient), all operands requested at once
            const double* mar = marr + (m & 1) * NU;
            const double own = mar[gsel], gown = Gm[gl_own >= 0 ? gl_own : 0];
            double lg[LM_MAX_LEGS], lm[LM_MAX_LEGS];
#pragma unroll
            for (int e = 0; e < LM_MAX_LEGS; e++) { lg[e] = Gm[gl[e] & 255]; lm[e] = mar[gl[e] >> 8]; }
            double gm = gl_own >= 0 ? gown * own : own;
#pragma unroll
            for (int e = 0; e < LM_MAX_LEGS; e++) gm += e < gl_n ? lg[e] * lm[e] : 0.0;
            const double gt = sgc[(m & 1) * NU + gsel] + gm;
            gtb[(size_t)m * NU + gsel] = gt;
            rw[(m % RING) * NU + gsel] = -gt;
        }
    };

    if (tid < 4) s_cnt[tid] = 0;
    if (tid == 0) s_int[2] = list_ok ? 0 : 1;
    for (int t = tid; t < BLK + 4 * LDB; t += LM_THREADS) Tm[t] = 0.0;
    __syncthreads();
    STAMP(1);

    // LOOK-AHEAD.  Per block column n the work is
    //   F(n)   factor sweep: right-looking Cholesky of D00 with the 28 rows of the identity and the right-hand side riding along as panel
    //          rows (wave_factor_panel): L00 (in place), T = L00^-T (Tm), z_n.  28 dependent pivot steps -- the one part that is a chain;
    //   P1(n)  X_i = A_i0 T for the PB blocks below, on the matrix cores (in place, and straight to HBM as column n of the factor);
    //   P2(n)  A_ij -= X_i X_j^T over the window's lower triangle, matrix cores; right-hand sides -= X_i z_n;
    //   R(n)   block row n + RING enters the window (store_row).
    // F(n+1) needs from column n only the three tiles of A_11 and the right-hand side of frame n+1: WAVE 0 runs the sweeps and, before each, that
    // small part of P2 itself (its SIMD's matrix pipe is otherwise idle); WAVES 1-3 run P1, the rest of P2 and R, and the sweep of the next
    // column overlaps the rest of the update of this one.  The two sides
    // meet through monotonic LDS counters (s_cnt), polled: [0] sweeps done, [1] rows staged by wave 0 (Gamma, gradients: stage_row),
    // [2] columns whose first block wave 0 has finished with, [3] the update waves' own barrier.
    // Tiles: a half panel (i, tr) = rows 16 tr .. of block i, index rh = 2 (i - 1) + tr.  P1: wave w takes half panels whole (both column
    // halves: 7 + 4 k-steps, T is upper triangular; read whole before it is overwritten).  P2: the tiles (j <= i, tc) of the half panels of blocks 2..PB are dealt
    // evenly (6 a wave for PB = 3), a half panel's A operand shared by its tiles, up to four accumulators in flight.
    if (s_int[2]) {
        // the motion model's term list does not fit: nothing to factor (uniform; the failure branch below takes over)
    } else if (wave == 0) {
        __builtin_amdgcn_s_setprio(3);                       // the factor wave carries the longer chain: it wins issue arbitration against whichever wave shares its SIMD
        for (int m = 0; m < RING && m < N; m++) {
            if (m >= 2) wait_ge(3, 3 * (m - 1));             // marr / sgc have two slots: row m-2 must have been stored
            stage_load(m); stage_store(m);
            lds_release();
            if (lane == 0) __atomic_store_n(&s_cnt[1], m + 1, __ATOMIC_RELAXED);
        }
        // rows 0 .. RING-1 are built by the update waves: [3] reaches 3 * min(RING, N) when the last of them is complete
        const int rows0 = N < RING ? N : RING;
        wait_ge(3, 3 * rows0);
        for (int n = 0; n < N; n++) {
            double* D00 = W + blk_slot<RING>(n, n) * BLK;
            if (n + RING < N) stage_load(n + RING);             // Gamma, motion gradient and per-frame gradient of the row that enters during column n: loads in flight during the sweep
            if (n >= 1) {
                // What this sweep needs from column n-1 -- A_11 -= X_1 X_1^T (three tiles) and rhs_1 -= X_1 z -- is done HERE, on this SIMD's
                // otherwise idle matrix pipe, as soon as the panel product of column n-1 is complete ([3] counts the update waves' barriers:
                // rows0 in the prologue, three per column, the first after P1).  The update waves keep their hands off block 1's tiles.
                wait_ge(3, 3 * (rows0 + 3 * (n - 1) + 1));
                STAMP(3);
                const double* X1 = win_blk<RING>(W, Wg, blk_slot<RING>(n, n - 1));
                if (lane < NU) {
                    const double* Li = X1 + lane * LDB;
                    const double* z = rw + ((n - 1) % RING) * NU;
                    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
                    for (int k = 0; k < NU; k += 2) { acc0 = fma(Li[k], z[k], acc0); acc1 = fma(Li[k + 1], z[k + 1], acc1); }
                    rw[(n % RING) * NU + lane] -= acc0 + acc1;
                }
                double xa[7];
                mfma_frag_rows(X1, 0, lane, xa);
                p2_tiles<RING, 1>(W, n - 1, 1, 0, 0, xa, lane, Wg);
                mfma_frag_rows(X1, 16, lane, xa);
                p2_tiles<RING, 2>(W, n - 1, 1, 1, 0, xa, lane, Wg);
                lds_release();
                if (lane == 0) __atomic_store_n(&s_cnt[2], n, __ATOMIC_RELAXED);     // X_1 of column n-1 is no longer read here: its slot may take the entering row
            }
            STAMP(6);
            const double* src;
            double* dst;
            int ident = -1;
            if (lane < NU) { src = D00 + lane * LDB; dst = D00 + lane * LDB; }
            else if (lane < 2 * NU) { ident = lane - NU; src = dummy_row; dst = Tm + ident * LDB; }
            else if (lane == 2 * NU) { src = rw + (n % RING) * NU; dst = rw + (n % RING) * NU; }
            else { src = dummy_row; dst = dummy_row; }
            const bool ok = wave_factor_panel(src, dst, lane < NU, colbuf, invd, lane, ident);
            if (!ok && lane == 0) s_int[2] = 1;
            lds_release();
            if (lane == 0) __atomic_store_n(&s_cnt[0], n + 1, __ATOMIC_RELAXED);
            STAMP(2);
            if (!ok) break;
            if (n + RING < N) {
                stage_store(n + RING);
                lds_release();
                if (lane == 0) __atomic_store_n(&s_cnt[1], n + RING + 1, __ATOMIC_RELAXED);
            }
            STAMP(1);
        }
    } else {
        for (int m = 0; m < RING && m < N; m++) { fetch_B(m); wait_ge(1, m + 1); store_row(m); sync3(); }
        constexpr int W3 = 3;
        const int uw = wave - 1;                                 // 0..2
#ifdef CPE_LM_STAMPS
        unsigned long long tu_last = __builtin_amdgcn_s_memtime();
        g_tu = &tu_last;
#endif
        for (int n = 0; n < N; n++) {
            double* D00 = W + blk_slot<RING>(n, n) * BLK;
            const int nb_i = N - 1 - n < PB ? N - 1 - n : PB;    // blocks below the diagonal in this column
            const int nrows = nb_i * NU;
            // P1's A operands do not depend on the sweep: they are read while it still runs
            constexpr int QN = (NRH + W3 - 1) / W3;                 // half panels per wave: 2 (PB = 3), 3 (PB = 4: 3, 3, 2)
            const int rh_lo = uw * QN, rh_n = rh_lo + QN <= NRH ? QN : NRH - rh_lo;
            double fa[QN][7];
#pragma unroll
            for (int q = 0; q < QN; q++) {
                const int rh = rh_lo + (q < rh_n ? q : 0);
                mfma_frag_rows(win_blk<RING>(W, Wg, blk_slot<RING>(n + 1 + rh / 2, n)), 16 * (rh & 1), lane, fa[q]);
            }
            wait_ge(0, n + 1);
            USTAMP(10);
            if (s_int[2]) break;                                 // uniform (the sweep failed)
            if (n + RING < N) fetch_B(n + RING);                 // in flight during the products
            double* Lcol = Lb + (size_t)n * RING * (NU * NU);
            // ---- P1: X_i = A_i0 T
            {
                double t1[7], t0[4];
                mfma_frag_cols(Tm, 16, lane, t1);
                {
                    const double* p = Tm + (lane >> 4) * LDB + (lane & 15);
#pragma unroll
                    for (int s2 = 0; s2 < 4; s2++) t0[s2] = p[4 * s2 * LDB];
                }
                d4_t acc[QN][2];
#pragma unroll
                for (int q = 0; q < QN; q++) { acc[q][0] = d4_t{0.0, 0.0, 0.0, 0.0}; acc[q][1] = d4_t{0.0, 0.0, 0.0, 0.0}; }
#pragma unroll
                for (int s2 = 0; s2 < 7; s2++)
#pragma unroll
                    for (int q = 0; q < QN; q++) {
                        acc[q][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[q][s2], t1[s2], acc[q][1], 0, 0, 0);
                        if (s2 < 4) acc[q][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[q][s2], t0[s2], acc[q][0], 0, 0, 0);   // T is upper triangular: rows 16.. of its left half are zero
                    }
                // X into the window first: wave 0 is waiting for exactly this (its A_11 tiles, then the next sweep) ...
#pragma unroll
                for (int q = 0; q < QN; q++) {
                    if (q < rh_n) {
                        const int rh = rh_lo + q, i = 1 + rh / 2;
                        double* Xi = win_blk<RING>(W, Wg, blk_slot<RING>(n + i, n));
#pragma unroll
                        for (int tc = 0; tc < 2; tc++) {
                            const int col = 16 * tc + (lane & 15);
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const int row = 16 * (rh & 1) + (lane >> 4) + 4 * r;
                                if (row < NU && col < NU) Xi[row * LDB + col] = i <= nb_i ? acc[q][tc][r] : 0.0;
                            }
                        }
                    }
                }
                USTAMP(4);
                sync3();
                // ... then column n of the factor to HBM, off that path: X from the accumulators, L00 with 1 / L[k][k] on its diagonal (block 0), z_n
#pragma unroll
                for (int q = 0; q < QN; q++) {
                    if (q < rh_n) {
                        const int rh = rh_lo + q, i = 1 + rh / 2;
#pragma unroll
                        for (int tc = 0; tc < 2; tc++) {
                            const int col = 16 * tc + (lane & 15);
#pragma unroll
                            for (int r = 0; r < 4; r++) {
                                const int row = 16 * (rh & 1) + (lane >> 4) + 4 * r;
                                if (row < NU && col < NU) Lcol[(size_t)i * (NU * NU) + row * NU + col] = i <= nb_i ? acc[q][tc][r] : 0.0;
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < NPB; j++) {
                    const int e = ut + UT * j;
                    if (e < NU * NU) {
                        const int a = e / NU, c = e - a * NU;
                        Lcol[e] = c < a ? D00[a * LDB + c] : (c == a ? invd[a] : 0.0);
                    }
                }
                if (ut < NU) zb[(size_t)n * NU + ut] = rw[(n % RING) * NU + ut];
            }
            USTAMP(9);
            // ---- P2: rhs_i -= X_i z, A_ij -= X_i X_j^T for the blocks below the first (block 1's rows are wave 0's)
            if (ut >= NU && ut < nrows) {
                const int i = 1 + ut / NU, a = ut - (i - 1) * NU;
                const double* Li = win_blk<RING>(W, Wg, blk_slot<RING>(n + i, n)) + a * LDB;
                const double* z = rw + (n % RING) * NU;
                double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
                for (int k = 0; k < NU; k += 2) { acc0 = fma(Li[k], z[k], acc0); acc1 = fma(Li[k + 1], z[k + 1], acc1); }
                rw[((n + i) % RING) * NU + a] -= acc0 + acc1;
            }
            // tiles of this wave: (half panel, first tile, tiles); half panel rh has rh + 1 tiles.  PB = 3 (18 tiles, 6 a wave): {rh5: 6},
            // {rh4: 5, rh2: tile 0}, {rh3: 4, rh2: tiles 1-2}; PB = 4 (33 tiles): {rh7: 8, rh2: 3}, {rh6: 7, rh3: 4}, {rh5: 6, rh4: 5};
            // PB = 5 (52): {rh9: 10, rh5: 6, rh2: tile 0}, {rh8: 9, rh6: 7, rh2: tiles 1-2}, {rh7: 8, rh4: 5, rh3: 4};
            // PB = 6 (75, 25 a wave): {rh11: 12, rh8: 9, rh3: 4}, {rh10: 11, rh7: 8, rh5: 6}, {rh9: 10, rh6: 7, rh4: 5, rh2: 3}
            constexpr int NMINE = PB <= 4 ? 2 : PB - 2;
            int m_rh[NMINE], m_lo[NMINE], m_n[NMINE];
            if constexpr (PB == 3) {
                m_rh[0] = 5 - uw; m_lo[0] = 0; m_n[0] = 6 - uw;
                m_rh[1] = uw == 0 ? -1 : 2; m_lo[1] = uw == 1 ? 0 : 1; m_n[1] = uw == 1 ? 1 : 2;
            } else if constexpr (PB == 4) {
                m_rh[0] = 7 - uw; m_lo[0] = 0; m_n[0] = 8 - uw;
                m_rh[1] = 2 + uw; m_lo[1] = 0; m_n[1] = 3 + uw;
            } else if constexpr (PB == 5) {
                m_rh[0] = 9 - uw; m_lo[0] = 0; m_n[0] = 10 - uw;
                m_rh[1] = uw == 0 ? 5 : (uw == 1 ? 6 : 4); m_lo[1] = 0; m_n[1] = m_rh[1] + 1;
                m_rh[2] = uw == 2 ? 3 : 2; m_lo[2] = uw == 1 ? 1 : 0; m_n[2] = uw == 0 ? 1 : (uw == 1 ? 2 : 4);
            } else {
                m_rh[0] = 11 - uw; m_lo[0] = 0; m_n[0] = 12 - uw;
                m_rh[1] = 8 - uw; m_lo[1] = 0; m_n[1] = 9 - uw;
                m_rh[2] = uw == 0 ? 3 : (uw == 1 ? 5 : 4); m_lo[2] = 0; m_n[2] = m_rh[2] + 1;
                m_rh[3] = uw == 2 ? 2 : -1; m_lo[3] = 0; m_n[3] = 3;
            }
#pragma unroll
            for (int pass = 0; pass < NMINE; pass++) {                   // (unrolled: the three small tables stay in registers)
                const int rh = m_rh[pass];
                if (rh < 0) continue;
                const int i = 1 + rh / 2, tr = rh & 1;
                if (i > nb_i) continue;                                  // uniform per wave
                double xa[7];
                mfma_frag_rows(win_blk<RING>(W, Wg, blk_slot<RING>(n + i, n)), 16 * tr, lane, xa);
                const int gend = m_lo[pass] + m_n[pass];                 // tiles (j, tc) of a half panel: j < i both column halves, j = i up to the diagonal tile
                for (int g = m_lo[pass]; g < gend;) {
                    const int left = gend - g, cnt = left >= 7 ? 4 : (left >= 5 ? 3 : left);    // 5 = 3 + 2, 6 = 3 + 3, 7 = 4 + 3, 8 = 4 + 4
                    if (cnt == 4) p2_tiles<RING, 4>(W, n, i, tr, g, xa, lane, Wg);
                    else if (cnt == 3) p2_tiles<RING, 3>(W, n, i, tr, g, xa, lane, Wg);
                    else if (cnt == 2) p2_tiles<RING, 2>(W, n, i, tr, g, xa, lane, Wg);
                    else p2_tiles<RING, 1>(W, n, i, tr, g, xa, lane, Wg);
                    g += cnt;
                }
            }
            USTAMP(5);
            // The prefetched B row is waited for HERE, while only loads are outstanding besides the factor stores of P1
            __builtin_amdgcn_s_waitcnt(0x0F70);
            USTAMP(15);
            sync3();
            USTAMP(7);
            if (n + RING < N) { wait_ge(1, n + RING + 1); wait_ge(2, n + 1 < N ? n + 1 : 0); USTAMP(12); store_row(n + RING); }
            USTAMP(11);
            sync3();
            USTAMP(13);
        }
    }

    __syncthreads();        // the factor columns and z written above are read back (by other threads) below
    if (s_int[2]) {
        // factorisation failed (matrix not positive definite at this damping): raise lambda, retry next call
        for (size_t t = tid; t < (size_t)N * nq; t += LM_THREADS)
            qbuf[(size_t)(1 - cur) * n_frames * nq + (size_t)b * NS * nq + t] = qc[t];
        if (tid == 0) { S = st[b]; S.lambda *= 10.0; S.pred = 0.0; S.maxstep = 1.0; S.back_pending = 0; st[b] = S; }
#ifdef CPE_LM_STAMPS
        if (tid == 0) atomicAdd(&g_lm_stamps[8], 1ull);       // factorisation failures over all workgroups
#endif
        return;
    }

    // (3) backward substitution, predicted reduction and trial iterate: k_lm_back, one wave per sequence
    if (tid == 0) st[b].back_pending = 1;
}

// --------------------------------------------------------------------------------------------------
// Second half of an LM step: backward substitution L^T delta = z (newest frame first) with the factor columns k_lm_step left in HBM, the
// predicted reduction and the trial iterate.  The work per block column is 25 KB of factor, 84 x 28 products and a 28-step substitution
// -- all latency, no parallelism across frames --, so it runs apart from k_lm_step's four-wave, 80 KB workgroups: TWO WAVES per
// sequence.  Wave 1 only moves factor columns from HBM into a three-column LDS ring with LDS-DMA loads (global_load_lds_dwordx4: no
// registers, nothing to wait for but its own vmcnt), two columns ahead of wave 0, which owns the arithmetic: lane k < 28 holds component
// k of delta_n; delta_{n+1..n+PB} sit in a small LDS ring and are read back as broadcasts.  One LDS barrier per column joins the two.
// From PB = 5 on a column is more than 31 1-KB pieces and two columns in flight would overrun vmcnt: the loader then waits for column
// n-1 before it issues column n-2 (still two columns ahead of wave 0, one in flight).
#define BACK_SLOTS 3
template <int PB, bool RAGGED = false>
__global__ __launch_bounds__(2 * WAVE) void k_lm_back(const DevModel* __restrict__ M, SeqState* __restrict__ st, LmParams prm, double* __restrict__ qbuf,
                                                      const double* __restrict__ Lbuf, double* __restrict__ zbuf, const double* __restrict__ gtbuf,
                                                      const double* __restrict__ dgbuf, const int* __restrict__ act, const int* __restrict__ n_act,
                                                      RaggedArgs rg = RaggedArgs{}) {
    if (n_act && (int)blockIdx.x >= *n_act) return;
    constexpr int RING = PB + 1, COLD = RING * NU * NU;
    constexpr int COLB = COLD * 8, NCH = (COLB + 1023) / 1024;       // bytes per factor column, 1 KB LDS-DMA pieces per column
    constexpr bool TWO = NCH < 32;                                    // two columns in flight fit vmcnt (6 bits)
    static_assert(NU % 4 == 0 && COLB % 16 == 0 && NCH < 64, "four accumulation chains; 16-byte pieces; a column in flight fits vmcnt");
    __shared__ __attribute__((aligned(16))) double ring[BACK_SLOTS * COLD];
    __shared__ __attribute__((aligned(16))) double dsh[PB * NU];
    __shared__ double far_part[2 * NU];                       // [n & 1]: sum over blocks 2..PB of column n, left by wave 1 one step ahead
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = act ? act[blockIdx.x] : (int)blockIdx.x, NS = prm.N;       // NS: the buffers' frames per sequence
    int N = NS;                                                                // N: this sequence's length
    if constexpr (RAGGED) { const int2 rs = rg.seq[b]; M += rs.x; N = rs.y; }
    const int ns = M->ns;
    const SeqState S = st[b];
    if (S.status != 0 || !S.back_pending) return;             // uniform
    const double* Lb = Lbuf + (size_t)b * NS * COLD;
    const int k = lane < NU ? lane : NU - 1;                  // idle lanes shadow lane 27 (reads stay in bounds, results unused)
    for (int t = threadIdx.x; t < PB * NU; t += 2 * WAVE) dsh[t] = 0.0;
    if (threadIdx.x < 2 * NU) far_part[threadIdx.x] = 0.0;    // column N-1 has no later frames

    if (wave == 1) {
        // ---- loader: column n goes to ring slot n % 3
        auto issue = [&](int n) {
            const char* g = reinterpret_cast<const char*>(Lb + (size_t)n * COLD) + lane * 16;
            double* dst = ring + (n % BACK_SLOTS) * COLD;
#pragma unroll
            for (int t = 0; t < NCH; t++)
                if (t * 1024 + lane * 16 < COLB)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g + t * 1024),
                                                     (__attribute__((address_space(3))) void*)(dst + t * 128), 16, 0, 0);
        };
#ifdef CPE_LM_STAMPS
        unsigned long long tb_last = __builtin_amdgcn_s_memtime();
#endif
        issue(N - 1);
        if (TWO && N > 1) issue(N - 2);
        // (raw barriers in this wave: a fenced one would wait for EVERY LDS-DMA load in flight, vmcnt(0), and the ring would never run ahead)
        if (TWO && N > 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(TWO ? NCH : 0) : "memory"); else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // column N-1 has landed (and this wave's share of the zeroing above)
        asm volatile("" ::: "memory");
        if (!TWO && N > 1) issue(N - 2);
        for (int n = N - 1; n >= 0; n--) {
            // wave 0 works on column n; column n+1's slot is free (the barrier that ended its step is behind us): column n-2 goes there
            if constexpr (!TWO) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                     // column n-1 has landed
                if (n >= 2) { issue(n - 2); BSTAMP(9); }
            } else if (n >= 2) { issue(n - 2); BSTAMP(9); asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TWO ? NCH : 0) : "memory"); }     // all but the newest column: n-1 has landed
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            BSTAMP(14);
            // the blocks 2..PB of column n-1 meet delta_{n+1..n+PB-1}, which are known already: their part of t is summed here, off
            // wave 0's chain (block i of column n-1 multiplies delta_{n-1+i})
            if (n >= 1) {
                const double* Lc = ring + ((n - 1) % BACK_SLOTS) * COLD + k;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
                for (int i = 2; i <= PB; i++) {
                    const double* dv = dsh + ((n - 1 + i) % PB) * NU;
                    const double* Li = Lc + i * (NU * NU);
#pragma unroll
                    for (int a = 0; a < NU; a += 4) {
                        a0 = fma(Li[a * NU], dv[a], a0);
                        a1 = fma(Li[(a + 1) * NU], dv[a + 1], a1);
                        a2 = fma(Li[(a + 2) * NU], dv[a + 2], a2);
                        a3 = fma(Li[(a + 3) * NU], dv[a + 3], a3);
                    }
                }
                if (lane < NU) far_part[((n - 1) & 1) * NU + lane] = (a0 + a1) + (a2 + a3);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            BSTAMP(15);
        }
        return;
    }

    // ---- wave 0: the arithmetic
    const size_t n_frames = (size_t)prm.B * NS;
    const int cur = S.cur;
    const double lam = S.lambda;
    double* zb = zbuf + (size_t)b * NS * NU;
    const double* gtb = gtbuf + (size_t)b * NS * NU;
    const double* dgb = dgbuf + (size_t)b * NS * NU;
    const double* qc = qbuf + ((size_t)cur * n_frames + (size_t)b * NS) * ns;
    double* qt = qbuf + ((size_t)(1 - cur) * n_frames + (size_t)b * NS) * ns;
    // state entry p moves with coordinate ck (or with none)
    int ck0 = -1, ck1 = -1;
    for (int c = 0; c < NU; c++) { const int p = M->ucoord_src[c]; if (p == lane) ck0 = c; if (p == lane + WAVE) ck1 = c; }
    double gtd = 0.0, dDd = 0.0, mx = 0.0;
    lds_barrier();
#ifdef CPE_LM_STAMPS
    unsigned long long tb_last = __builtin_amdgcn_s_memtime();
#endif
    // z, g, diag(H) and the state of the NEXT column are fetched one column ahead (an L2 round trip would otherwise sit on the chain)
    double z_n = zb[(size_t)(N - 1) * NU + k], gt_n = gtb[(size_t)(N - 1) * NU + k], dg_n = dgb[(size_t)(N - 1) * NU + k];
    double q0_n = lane < ns ? qc[(size_t)(N - 1) * ns + lane] : 0.0, q1_n = lane + WAVE < ns ? qc[(size_t)(N - 1) * ns + lane + WAVE] : 0.0;
    for (int n = N - 1; n >= 0; n--) {
        double tk = z_n;
        const double gt = gt_n, dgv = dg_n, q0 = q0_n, q1 = q1_n;
        {
            const int np = n > 0 ? n - 1 : 0;
            z_n = zb[(size_t)np * NU + k]; gt_n = gtb[(size_t)np * NU + k]; dg_n = dgb[(size_t)np * NU + k];
            q0_n = lane < ns ? qc[(size_t)np * ns + lane] : 0.0; q1_n = lane + WAVE < ns ? qc[(size_t)np * ns + lane + WAVE] : 0.0;
        }
        const double* Lc = ring + (n % BACK_SLOTS) * COLD + k;
        // t[k] = z_n[k] - sum_{i=1..PB} sum_a L_i0[a][k] delta_{n+i}[a]: block 1 (it needs delta_{n+1}, the newest) here in four chains, the
        // others from wave 1 (blocks past the end are zero in the factor)
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        {
            const double* dv = dsh + ((n + 1) % PB) * NU;
            const double* Li = Lc + NU * NU;
#pragma unroll
            for (int a = 0; a < NU; a += 4) {
                a0 = fma(Li[a * NU], dv[a], a0);
                a1 = fma(Li[(a + 1) * NU], dv[a + 1], a1);
                a2 = fma(Li[(a + 2) * NU], dv[a + 2], a2);
                a3 = fma(Li[(a + 3) * NU], dv[a + 3], a3);
            }
        }
        BSTAMP(6);
        // L00^T x = t, x[m] from m = 27 down, in the scaled variable w[k] = t[k] / L00[k][k]: with c[m] = L00[m][k] / L00[k][k] (column k of
        // L00 scaled by this lane's own pivot, off the chain; zero on and above the diagonal) a step is ONE broadcast and ONE fused
        // multiply-add for every lane: x[m] = w[m] once every m' > m has been applied, w[k] -= c[m] x[m] for k < m
        const double invk = Lc[k * NU];                          // 1 / L00[k][k] sits on the diagonal of the stored block
        double col[NU];
#pragma unroll
        for (int m2 = 0; m2 < NU; m2++) col[m2] = Lc[m2 * NU];     // (unconditional reads: a select around the read becomes 28 branches, each waiting for its own LDS round trip)
        const double ninv = -invk;
#pragma unroll
        for (int m2 = 0; m2 < NU; m2++) { const double c = col[m2] * ninv; col[m2] = lane == m2 ? 0.0 : c; }
        tk = (tk - far_part[(n & 1) * NU + k] - ((a0 + a1) + (a2 + a3))) * invk;
#pragma unroll
        for (int m2 = NU - 1; m2 > 0; m2--) tk = fma(col[m2], readlane_f64(tk, m2), tk);
        BSTAMP(7);
        if (lane < NU) {
            dsh[(n % PB) * NU + lane] = tk;                   // takes the slot of delta_{n+PB}, which no later column reads
            zb[(size_t)n * NU + lane] = tk;                   // delta overwrites z
            gtd += gt * tk;
            dDd += fmax(dgv, LM_DIAG_FLOOR(N)) * tk * tk;
            mx = fmax(mx, fabs(tk));
        }
        // trial iterate into the other buffer
        const double m0 = __shfl(tk, ck0 >= 0 ? ck0 : 0), m1 = __shfl(tk, ck1 >= 0 ? ck1 : 0);
        if (lane < ns) qt[(size_t)n * ns + lane] = q0 + (ck0 >= 0 ? m0 : 0.0);
        if (lane + WAVE < ns) qt[(size_t)n * ns + lane + WAVE] = q1 + (ck1 >= 0 ? m1 : 0.0);
        BSTAMP(12);
        lds_barrier();
        BSTAMP(13);
    }
    gtd = wave_sum(gtd); dDd = wave_sum(dDd); mx = wave_max(mx);
    if (lane == 0) {
        SeqState* Sp = st + b;
        Sp->pred = -0.5 * gtd + 0.5 * lam * dDd;
        Sp->maxstep = mx;
        Sp->back_pending = 0;
    }
}

// --------------------------------------------------------------------------------------------------
// Per-frame ground-reaction-force fit (acinoset_opt.py:176-270, SURVEY A.8; include/cpe.h).  One wave per frame:
// rows 0-5 of the equations of motion from (q, q', q'') by the projected Newton-Euler form (every link's centre-of-mass
// acceleration walks up its own chain, one lane per link), the 6 x 5 n_feet force matrix, then FISTA on
// |E - A y|^2 / 2 + eps |y|^2 / 2 with the exact projection onto {0 <= y <= fmax, sum_k x_k <= mu z} per foot (bisection
// on the multiplier of the friction constraint, lanes 0, 5, 10, 15).  Same arithmetic as cpo_grf_fit_frame.
// static LDS per wave: q, dq, ddq, sin/cos, R, w, alpha, dR_root, A, first vectors
__device__ __forceinline__ void grf_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void grf_point_acc(const double* R, const double* w, const double* al, const double* v, double* out) {
    double t1[3], t2[3], t3[3];
    grf_cross(w, v, t1); grf_cross(w, t1, t2); grf_cross(al, v, t3);
    t2[0] += t3[0]; t2[1] += t3[1]; t2[2] += t3[2];
    out[0] = R[0] * t2[0] + R[1] * t2[1] + R[2] * t2[2];
    out[1] = R[3] * t2[0] + R[4] * t2[1] + R[5] * t2[2];
    out[2] = R[6] * t2[0] + R[7] * t2[1] + R[8] * t2[2];
}
__device__ __forceinline__ double grf_clamp(double v, double hi) { return v < 0.0 ? 0.0 : (v > hi ? hi : v); }

#define GRF_PACK 3      // frames per wave in k_grf: 3 x (5 unknowns x 4 feet) = 60 of 64 lanes
__global__ __launch_bounds__(WAVE) void k_grf(const DevModel* __restrict__ M, cpe_grf_options o, size_t n_frames,
                                              const double* __restrict__ q, const double* __restrict__ dq,
                                              const double* __restrict__ ddq, const int32_t* __restrict__ contact,
                                              double* __restrict__ grfz, double* __restrict__ grfxy, double* __restrict__ residual) {
    __shared__ double sq[3][CPE_MAX_NQ];
    __shared__ double ssc[6 * CPE_MAX_LINKS], sR[9 * CPE_MAX_LINKS], sw[3 * CPE_MAX_LINKS], sal[3 * CPE_MAX_LINKS];
    __shared__ double sdR[27], sJw[9], sA[GRF_PACK][6 * 20], sE[GRF_PACK][6], sfirst[4][3];
    const int lane = threadIdx.x;
    const int nq = M->nq, nl = M->nl, nf = o.n_feet, nv = 5 * nf;
    for (int t = lane; t < GRF_PACK * 6 * 20; t += WAVE) (&sA[0][0])[t] = 0.0;
    if (lane < GRF_PACK * 6) (&sE[0][0])[lane] = 0.0;
    wave_lds_sync();
    // The iteration below keeps only nv <= 20 lanes busy per frame, so a wave fits GRF_PACK = 3 frames side by side: the
    // set-up (all 64 lanes on one frame) runs once per packed frame, then lanes [g nv, (g+1) nv) iterate on frame g.
    for (int g2 = 0; g2 < GRF_PACK; g2++) {
    const size_t f = (size_t)blockIdx.x * GRF_PACK + g2;
    if (f >= n_frames) break;
    if (lane < nq) { sq[0][lane] = q[f * nq + lane]; sq[1][lane] = dq[f * nq + lane]; sq[2][lane] = ddq[f * nq + lane]; }
    wave_lds_sync();
    wave_sincos(M, sq[0], ssc, lane);
    wave_lds_sync();
    int root = 0;
    for (int i = 0; i < nl; i++) if (M->parent[i] < 0) root = i;
    if (lane < nl) {
        rot_kind(ssc + 6 * lane, 0, sR + 9 * lane);
        const double* a = sq[0] + 3 + 3 * lane; const double* da = sq[1] + 3 + 3 * lane; const double* dda = sq[2] + 3 + 3 * lane;
        const double sf = ssc[6 * lane], cf = ssc[6 * lane + 1], st = ssc[6 * lane + 2], ct = ssc[6 * lane + 3];
        (void)a;
        const double c0[3] = {1.0, 0.0, 0.0}, c1[3] = {0.0, cf, -sf}, c2[3] = {-st, sf * ct, cf * ct};
        const double d1[3] = {0.0, -sf * da[0], -cf * da[0]};
        const double d2[3] = {-ct * da[1], cf * da[0] * ct - sf * st * da[1], -sf * da[0] * ct - cf * st * da[1]};
        for (int k = 0; k < 3; k++) {
            sw[3 * lane + k] = c0[k] * da[0] + c1[k] * da[1] + c2[k] * da[2];
            sal[3 * lane + k] = c0[k] * dda[0] + c1[k] * dda[1] + c2[k] * dda[2] + d1[k] * da[1] + d2[k] * da[2];
            if (lane == root) { sJw[3 * k] = c0[k]; sJw[3 * k + 1] = c1[k]; sJw[3 * k + 2] = c2[k]; }
        }
        if (lane == root) for (int a2 = 0; a2 < 3; a2++) rot_kind(ssc + 6 * lane, 1 + a2, sdR + 9 * a2);
    }
    wave_lds_sync();
    // centre-of-mass force of link `lane` and its contribution to the six rows
    double e6[6] = {0, 0, 0, 0, 0, 0};
    double mtot = 0.0;
    for (int i = 0; i < nl; i++) mtot += M->mass[i];
    if (lane < nl) {
        double acc[3] = {sq[2][0], sq[2][1], sq[2][2]}, first[3] = {M->com[lane][0], M->com[lane][1], M->com[lane][2]};
        // walk up the chain; the sum is formed root-first (as the oracle's recursion does) by collecting the terms
        double terms[CPE_MAX_CHAIN][3];
        int nt = 0, j = lane;
        while (M->parent[j] >= 0) {
            const int p = M->parent[j];
            grf_point_acc(sR + 9 * p, sw + 3 * p, sal + 3 * p, M->attach[j], terms[nt]);
            if (p == root) { first[0] = M->attach[j][0]; first[1] = M->attach[j][1]; first[2] = M->attach[j][2]; }
            nt++; j = p;
        }
        for (int t = nt - 1; t >= 0; t--) { acc[0] += terms[t][0]; acc[1] += terms[t][1]; acc[2] += terms[t][2]; }
        double ac[3];
        grf_point_acc(sR + 9 * lane, sw + 3 * lane, sal + 3 * lane, M->com[lane], ac);
        const double m = M->mass[lane];
        const double fx = m * (acc[0] + ac[0]), fy = m * (acc[1] + ac[1]), fz = m * (acc[2] + ac[2] + o.gravity);
        e6[0] = fx; e6[1] = fy; e6[2] = fz;
        for (int a2 = 0; a2 < 3; a2++) {
            const double* D = sdR + 9 * a2;
            const double v0 = D[0] * first[0] + D[1] * first[1] + D[2] * first[2];
            const double v1 = D[3] * first[0] + D[4] * first[1] + D[5] * first[2];
            const double v2 = D[6] * first[0] + D[7] * first[1] + D[8] * first[2];
            e6[3 + a2] = fx * v0 + fy * v1 + fz * v2;
        }
        if (lane == root) {
            const double* I = o.root_inertia; const double* w = sw + 3 * root; const double* al = sal + 3 * root;
            const double Iw[3] = {I[0] * w[0], I[1] * w[1], I[2] * w[2]};
            double wIw[3]; grf_cross(w, Iw, wIw);
            const double tq[3] = {I[0] * al[0] + wIw[0], I[1] * al[1] + wIw[1], I[2] * al[2] + wIw[2]};
            for (int a2 = 0; a2 < 3; a2++) e6[3 + a2] += tq[0] * sJw[a2] + tq[1] * sJw[3 + a2] + tq[2] * sJw[6 + a2];
        }
    }
    // the root-frame vector on the way to each foot = first entry of the marker's chain table
    if (lane < 3 * nf) sfirst[lane / 3][lane % 3] = M->chain_vec[o.foot_marker[lane / 3]][0][lane % 3];
    for (int k = 0; k < 6; k++) { const double x = wave_sum(e6[k]); if (lane == 0) sE[g2][k] = x / (mtot * o.gravity); }
    wave_lds_sync();
    // force matrix, column `lane`
    const double Dk[5][3] = {{0, 0, 1}, {1, 0, 0}, {0, 1, 0}, {-1, 0, 0}, {0, -1, 0}};
    if (lane < nv) {
        const int ft = lane / 5, k = lane - 5 * ft;
        for (int d = 0; d < 3; d++) sA[g2][d * nv + lane] = Dk[k][d];
        for (int a2 = 0; a2 < 3; a2++) {
            const double* D = sdR + 9 * a2; const double* fv = sfirst[ft];
            const double v0 = D[0] * fv[0] + D[1] * fv[1] + D[2] * fv[2];
            const double v1 = D[3] * fv[0] + D[4] * fv[1] + D[5] * fv[2];
            const double v2 = D[6] * fv[0] + D[7] * fv[1] + D[8] * fv[2];
            sA[g2][(3 + a2) * nv + lane] = v0 * Dk[k][0] + v1 * Dk[k][1] + v2 * Dk[k][2];
        }
    }
    wave_lds_sync();
    }       // packed frames
    // ---- packed iteration: lane -> (frame slot g, unknown c)
    const int g = lane / nv < GRF_PACK ? lane / nv : 0, c_ = lane - (lane / nv) * nv, gbase = g * nv;
    const size_t f = (size_t)blockIdx.x * GRF_PACK + g;
    const bool valid = lane < GRF_PACK * nv && f < n_frames;
    const int act = valid && contact[f * nf + c_ / 5] != 0;
    double Acol[6] = {0, 0, 0, 0, 0, 0};
    if (valid) for (int r = 0; r < 6; r++) Acol[r] = sA[g][r * nv + c_];
    double lsum = 0.0;
    if (act) for (int r = 0; r < 6; r++) lsum += Acol[r] * Acol[r];
    // L = eps + sum over the columns in contact, accumulated foot by foot and component by component like the oracle
    double Lc = o.regularisation;
    for (int c = 0; c < nv; c++) { const double x = __shfl(lsum, gbase + c, WAVE); Lc += x; }
    const int any = __any(act);
    double y = 0.0, v = 0.0;
    const double E0 = sE[g][0], E1 = sE[g][1], E2 = sE[g][2], E3 = sE[g][3], E4 = sE[g][4], E5 = sE[g][5];
    const double* Ag = sA[g];
    if (any)
        for (int it = 0; it < o.iterations; it++) {
            // r = E - A v : the sum over the columns in index order (matches the oracle bit for bit up to contraction)
            double r6[6] = {E0, E1, E2, E3, E4, E5};
            for (int c = 0; c < nv; c++) {
                const double vc = __shfl(v, gbase + c, WAVE);
#pragma unroll
                for (int r = 0; r < 6; r++) r6[r] -= Ag[r * nv + c] * vc;
            }
            double gr = o.regularisation * v;
#pragma unroll
            for (int r = 0; r < 6; r++) gr -= Acol[r] * r6[r];
            const double yprev = y;
            double y0 = act ? v - gr / Lc : 0.0;
            // projection of the foot's five numbers, every lane of the group of five redundantly
            const int base = lane - c_ % 5;
            double t5[5];
#pragma unroll
            for (int k = 0; k < 5; k++) t5[k] = __shfl(y0, (base + k) & 63, WAVE);
            double lam = 0.0;
            {
                const double mu = o.friction_ratio, fm = o.force_max;
                auto G = [&](double l) {
                    return grf_clamp(t5[1] - l, fm) + grf_clamp(t5[2] - l, fm) + grf_clamp(t5[3] - l, fm) + grf_clamp(t5[4] - l, fm) -
                           mu * grf_clamp(t5[0] + mu * l, fm);
                };
                if (G(0.0) > 0.0) {
                    double lo = 0.0, hi = t5[1];
                    for (int k = 2; k < 5; k++) if (t5[k] > hi) hi = t5[k];
                    for (int b2 = 0; b2 < 50; b2++) { const double mid = 0.5 * (lo + hi); if (G(mid) > 0.0) lo = mid; else hi = mid; }
                    lam = hi;
                }
            }
            const int k = c_ % 5;
            y = act ? grf_clamp(k == 0 ? y0 + o.friction_ratio * lam : y0 - lam, o.force_max) : 0.0;
            const double beta = (double)it / (double)(it + 3);
            v = y + beta * (y - yprev);
        }
    if (valid) {
        const int ft = c_ / 5, k = c_ - 5 * ft;
        if (k == 0) grfz[f * nf + ft] = y; else grfxy[(f * nf + ft) * 4 + (k - 1)] = y;
    }
    if (residual) {
        double r6[6] = {E0, E1, E2, E3, E4, E5};
        for (int c = 0; c < nv; c++) {
            const double yc = __shfl(y, gbase + c, WAVE);
            for (int r = 0; r < 6; r++) r6[r] -= Ag[r * nv + c] * yc;
        }
        // lane c_ of the frame stores row c_; one foot leaves only five lanes per frame, so lane 0 stores row 5 as well
        if (valid)
            for (int r = c_; r < 6; r += nv) {
                const double rr = r == 0 ? r6[0] : r == 1 ? r6[1] : r == 2 ? r6[2] : r == 3 ? r6[3] : r == 4 ? r6[4] : r6[5];
                residual[f * 6 + r] = rr;
            }
    }
}

// --------------------------------------------------------------------------------------------------
// All rows of the equations of motion (include/cpe.h, cpe_eom_rows; residual function of SURVEY row a12).  One wave per frame,
// one lane per link: body rates, centre-of-mass force f_i = m_i (P_i'' + g e_z) by walking up the chain, subtree sums of
// the forces with LDS atomics (every link adds its f to itself and its ancestors), then the three angle rows of the link.
__global__ __launch_bounds__(WAVE) void k_eom(const DevModel* __restrict__ M, const cpe_eom_options* __restrict__ o, size_t n_frames,
                                              const double* __restrict__ q, const double* __restrict__ dq,
                                              const double* __restrict__ ddq, double* __restrict__ rows) {
    __shared__ double sq[3][CPE_MAX_NQ];
    __shared__ double ssc[6 * CPE_MAX_LINKS], sR[9 * CPE_MAX_LINKS], sw[3 * CPE_MAX_LINKS], sal[3 * CPE_MAX_LINKS], sFs[3 * CPE_MAX_LINKS];
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    const int nq = M->nq, nl = M->nl;
    if (lane < nq) { sq[0][lane] = q[f * nq + lane]; sq[1][lane] = dq[f * nq + lane]; sq[2][lane] = ddq[f * nq + lane]; }
    if (lane < 3 * nl) sFs[lane] = 0.0;
    wave_lds_sync();
    wave_sincos(M, sq[0], ssc, lane);
    wave_lds_sync();
    double Jw[3][3] = {{0}};
    if (lane < nl) {
        rot_kind(ssc + 6 * lane, 0, sR + 9 * lane);
        const double* da = sq[1] + 3 + 3 * lane; const double* dda = sq[2] + 3 + 3 * lane;
        const double sf = ssc[6 * lane], cf = ssc[6 * lane + 1], st = ssc[6 * lane + 2], ct = ssc[6 * lane + 3];
        const double c0[3] = {1.0, 0.0, 0.0}, c1[3] = {0.0, cf, -sf}, c2[3] = {-st, sf * ct, cf * ct};
        const double d1[3] = {0.0, -sf * da[0], -cf * da[0]};
        const double d2[3] = {-ct * da[1], cf * da[0] * ct - sf * st * da[1], -sf * da[0] * ct - cf * st * da[1]};
        for (int k = 0; k < 3; k++) {
            sw[3 * lane + k] = c0[k] * da[0] + c1[k] * da[1] + c2[k] * da[2];
            sal[3 * lane + k] = c0[k] * dda[0] + c1[k] * dda[1] + c2[k] * dda[2] + d1[k] * da[1] + d2[k] * da[2];
            Jw[k][0] = c0[k]; Jw[k][1] = c1[k]; Jw[k][2] = c2[k];
        }
    }
    wave_lds_sync();
    double fi[3] = {0, 0, 0};
    if (lane < nl) {
        double acc[3] = {sq[2][0], sq[2][1], sq[2][2]};
        double terms[CPE_MAX_CHAIN][3];
        int nt = 0, j = lane;
        while (M->parent[j] >= 0) {
            const int p = M->parent[j];
            grf_point_acc(sR + 9 * p, sw + 3 * p, sal + 3 * p, M->attach[j], terms[nt]);
            nt++; j = p;
        }
        for (int t = nt - 1; t >= 0; t--) { acc[0] += terms[t][0]; acc[1] += terms[t][1]; acc[2] += terms[t][2]; }
        double ac[3];
        grf_point_acc(sR + 9 * lane, sw + 3 * lane, sal + 3 * lane, M->com[lane], ac);
        const double m = M->mass[lane];
        fi[0] = m * (acc[0] + ac[0]); fi[1] = m * (acc[1] + ac[1]); fi[2] = m * (acc[2] + ac[2] + o->gravity);
        for (j = lane; j >= 0; j = M->parent[j]) { atomicAdd(sFs + 3 * j, fi[0]); atomicAdd(sFs + 3 * j + 1, fi[1]); atomicAdd(sFs + 3 * j + 2, fi[2]); }
    }
    wave_lds_sync();
    if (lane < nl) {
        if (M->parent[lane] < 0) { rows[f * nq] = sFs[3 * lane]; rows[f * nq + 1] = sFs[3 * lane + 1]; rows[f * nq + 2] = sFs[3 * lane + 2]; }
        const double* I = o->link_inertia[lane]; const double* w = sw + 3 * lane; const double* al = sal + 3 * lane;
        const double Iw[3] = {I[0] * w[0], I[1] * w[1], I[2] * w[2]};
        double wIw[3]; grf_cross(w, Iw, wIw);
        const double tq[3] = {I[0] * al[0] + wIw[0], I[1] * al[1] + wIw[1], I[2] * al[2] + wIw[2]};
        for (int a2 = 0; a2 < 3; a2++) {
            double D[9];
            rot_kind(ssc + 6 * lane, 1 + a2, D);
            auto dot_dRv = [&](const double* F3, const double* v) {
                return F3[0] * (D[0] * v[0] + D[1] * v[1] + D[2] * v[2]) + F3[1] * (D[3] * v[0] + D[4] * v[1] + D[5] * v[2]) +
                       F3[2] * (D[6] * v[0] + D[7] * v[1] + D[8] * v[2]);
            };
            double e = dot_dRv(fi, M->com[lane]);
            for (int c = 0; c < nl; c++) if (M->parent[c] == lane) e += dot_dRv(sFs + 3 * c, M->attach[c]);
            e += tq[0] * Jw[0][a2] + tq[1] * Jw[1][a2] + tq[2] * Jw[2][a2];
            rows[f * nq + 3 + 3 * lane + a2] = e;
        }
    }
}

// --------------------------------------------------------------------------------------------------
// residual -= Q, the generalised forces of the physics-based model (include/cpe.h, cpe_eom_residual; same sums as
// cpo_dyn_forces).  One wave per frame, one lane per coordinate.
__global__ __launch_bounds__(WAVE) void k_dyn_forces(const DevModel* __restrict__ M, const cpe_dyn_options* __restrict__ o, size_t n_frames,
                                                     const double* __restrict__ q, const double* __restrict__ tau,
                                                     const double* __restrict__ lam, const double* __restrict__ grf,
                                                     int n_con, double* __restrict__ residual) {
    __shared__ double sq[CPE_MAX_NQ];
    __shared__ double ssc[6 * CPE_MAX_LINKS], sR[36 * CPE_MAX_LINKS];
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x;
    const int nq = M->nq, nl = M->nl;
    if (lane < nq) sq[lane] = q[f * nq + lane];
    wave_lds_sync();
    wave_sincos(M, sq, ssc, lane);
    wave_lds_sync();
    for (int t = lane; t < 4 * nl; t += WAVE) rot_kind(ssc + 6 * (t >> 2), t & 3, sR + 9 * t);     // R, dR/dphi, dR/dtheta, dR/dpsi per link
    wave_lds_sync();
    if (lane >= nq) return;
    double mtot = 0.0;
    for (int i = 0; i < nl; i++) mtot += M->mass[i];
    const double Mg = mtot * o->eom.gravity;
    const double Dk[5][3] = {{0, 0, 1}, {1, 0, 0}, {0, 1, 0}, {-1, 0, 0}, {0, -1, 0}};
    const int i = lane < 3 ? -1 : (lane - 3) / 3, a = lane < 3 ? 0 : (lane - 3) - 3 * i;
    double Q = 0.0;
    if (grf)
        for (int ft = 0; ft < o->n_feet; ft++) {
            const double* gf = grf + (f * o->n_feet + ft) * 5;
            double F[3] = {0, 0, 0};
            for (int k = 0; k < 5; k++) for (int d = 0; d < 3; d++) F[d] += Mg * gf[k] * Dk[k][d];
            if (lane < 3) { Q += F[lane]; continue; }
            const int l = o->foot_marker[ft];
            for (int k = 0; k < M->chain_len[l]; k++)
                if (M->chain_link[l][k] == i) {
                    const double* D = sR + 9 * (4 * i + 1 + a); const double* v = M->chain_vec[l][k];
                    Q += F[0] * (D[0] * v[0] + D[1] * v[1] + D[2] * v[2]) + F[1] * (D[3] * v[0] + D[4] * v[1] + D[5] * v[2]) +
                         F[2] * (D[6] * v[0] + D[7] * v[1] + D[8] * v[2]);
                }
        }
    if (tau && i >= 0) {
        // d w_world / d q'_a of link i = R_i times column a of the body-rate map
        const double sf = ssc[6 * i], cf = ssc[6 * i + 1], st = ssc[6 * i + 2], ct = ssc[6 * i + 3];
        const double c3[3][3] = {{1.0, 0.0, 0.0}, {0.0, cf, -sf}, {-st, sf * ct, cf * ct}};
        const double* R = sR + 36 * i;
        const double wc[3] = {R[0] * c3[a][0] + R[1] * c3[a][1] + R[2] * c3[a][2], R[3] * c3[a][0] + R[4] * c3[a][1] + R[5] * c3[a][2],
                              R[6] * c3[a][0] + R[7] * c3[a][1] + R[8] * c3[a][2]};
        for (int m = 0; m < o->n_motors; m++) {
            const int a1 = o->motor_first[m], a2 = o->motor_second[m];
            if (a1 != i && a2 != i) continue;
            const double* R1 = sR + 36 * a1; const int ax = o->motor_axis[m];
            const double t = Mg * tau[f * o->n_motors + m] * (R1[ax] * wc[0] + R1[3 + ax] * wc[1] + R1[6 + ax] * wc[2]);
            Q += (a2 == i ? t : 0.0) - (a1 == i ? t : 0.0);
        }
    }
    if (lam && i >= 0) {
        int row = 0;
        for (int j = 0; j < M->nj; j++) {
            const int p = M->joint_parent[j], ch = M->joint_child[j];
            const int first = M->joint_kind[j] == CPE_JOINT_REVOLUTE_Y ? 0 : 1;
            for (int t = first; t < 2; t++, row++) {
                if (p != i && ch != i) continue;
                const int cc = t == 0 ? 0 : 2;                       // child x axis, child z axis
                const double* Rp = sR + 36 * p; const double* Rc = sR + 36 * ch;
                double d = 0.0;
                if (p == i) { const double* Dp = sR + 9 * (4 * p + 1 + a); d += Dp[1] * Rc[cc] + Dp[4] * Rc[3 + cc] + Dp[7] * Rc[6 + cc]; }
                if (ch == i) { const double* Dc = sR + 9 * (4 * ch + 1 + a); d += Rp[1] * Dc[cc] + Rp[4] * Dc[3 + cc] + Rp[7] * Dc[6 + cc]; }
                Q += d * lam[f * n_con + row];
            }
        }
    }
    residual[f * nq + lane] -= Q;
}

// --------------------------------------------------------------------------------------------------
// solver outputs as CheetahEstimator.save writes them (acinoset_opt.py:289-361): q, dq, ddq (implicit
// Euler with the free-initial-state gauge ddq0 = ddq1 = ddq2), marker positions, meas_err.
// dynamic LDS: q[nq] | sc[6nl] | R[36nl] | pos[3L] | cam[23C]
template <bool RAGGED = false>
__global__ __launch_bounds__(WAVE) void k_finalize(const DevModel* __restrict__ M, const SeqState* __restrict__ st, int N,
                                                   size_t n_frames, const double* __restrict__ qbuf,
                                                   const double* __restrict__ meas, double* __restrict__ q,
                                                   double* __restrict__ dq, double* __restrict__ ddq,
                                                   double* __restrict__ positions, double* __restrict__ meas_err,
                                                   unsigned long long* __restrict__ cmax_seq /* [B] bit patterns of max |joint equality| */,
                                                   const double* __restrict__ tau = nullptr /* shutter delays [B][C], or null */,
                                                   RaggedArgs rg = RaggedArgs{} /* RAGGED: N = nmax; frames and cameras past a sequence's own are written as zeros */) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    FrameSlot fs;
    const bool own = frame_slot<RAGGED>(N, nullptr, nullptr, rg, fs);     // false: a frame past the sequence's own length
    M += fs.model;
    const int NL = fs.len;                               // N: the buffers' frames per sequence, NL: this sequence's length
    const int nq = M->nq, nl = M->nl, L = M->L, C = M->C;
    const int cst = RAGGED ? rg.cstride : C;             // cameras per frame of meas / meas_err
    double* sq = smem;
    double* ssc = sq + nq;
    double* sR = ssc + 6 * nl;
    double* spos = sR + 36 * nl;
    double* scam = spos + 3 * L;
    const size_t f = blockIdx.x;
    const int b = fs.b, n = fs.n;
    const int ns = M->ns;                                                                  // state stride (Euler q + leg angles)
    if (!own) {
        for (int t = lane; t < nq; t += WAVE) { q[f * nq + t] = 0.0; if (dq && ddq) { dq[f * nq + t] = 0.0; ddq[f * nq + t] = 0.0; } }
        if (positions) for (int t = lane; t < 3 * L; t += WAVE) positions[f * (size_t)(3 * L) + t] = 0.0;
        if (meas_err) for (int t = lane; t < 2 * cst * L; t += WAVE) meas_err[f * (size_t)(2 * cst * L) + t] = 0.0;
        return;
    }
    const double* qs = qbuf + (size_t)st[b].cur * n_frames * ns + (size_t)b * N * ns;   // sequence base
    if (lane < nq) {
        const double h = M->h;
        const double q0 = qs[(size_t)n * ns + lane];
        sq[lane] = q0;
        q[f * nq + lane] = q0;
        if (dq && ddq) {
            double v = 0.0, a = 0.0;
            if (NL >= 3) {
                const int m = n < 2 ? 2 : n;      // ddq0 = ddq1 = ddq2
                a = (qs[(size_t)m * ns + lane] - 2.0 * qs[(size_t)(m - 1) * ns + lane] + qs[(size_t)(m - 2) * ns + lane]) / (h * h);
            }
            if (n >= 1) v = (q0 - qs[(size_t)(n - 1) * ns + lane]) / h;
            else if (NL >= 2) v = (qs[(size_t)ns + lane] - q0) / h - h * a;   // dq0 = dq1 - h ddq1
            dq[f * nq + lane] = v; ddq[f * nq + lane] = a;
        }
    }
    for (int t = lane; t < 23 * C; t += WAVE) scam[t] = reinterpret_cast<const double*>(M->cam)[t];
    wave_lds_sync();
    wave_sincos(M, sq, ssc, lane);
    wave_lds_sync();
    for (int t = lane; t < nl; t += WAVE) rot_kind(ssc + 6 * t, 0, sR + 36 * t);
    wave_lds_sync();
    wave_markers(M, sq, sR, spos, lane);
    wave_lds_sync();
    if (cmax_seq) {
        // joint equalities of the returned Euler angles (cheetah.py:71-72,101,160-161): parent.y . child.x and parent.y . child.z
        // for a revolute joint, parent.y . child.z for a hooke joint; non-negative doubles order like their bit patterns
        double cv = 0.0;
        if (lane < M->nj) {
            const double* Rp = sR + 36 * M->joint_parent[lane]; const double* Rc = sR + 36 * M->joint_child[lane];
            const double yz = Rp[1] * Rc[2] + Rp[4] * Rc[5] + Rp[7] * Rc[8];
            cv = fabs(yz);
            if (M->joint_kind[lane] == CPE_JOINT_REVOLUTE_Y) cv = fmax(cv, fabs(Rp[1] * Rc[0] + Rp[4] * Rc[3] + Rp[7] * Rc[6]));
        }
        cv = wave_max(cv);
        if (lane == 0) atomicMax(cmax_seq + b, (unsigned long long)__double_as_longlong(cv));
    }
    if (positions) for (int t = lane; t < 3 * L; t += WAVE) positions[f * (size_t)(3 * L) + t] = spos[t];
    if (meas_err) {
        const cpe_camera* cams = reinterpret_cast<const cpe_camera*>(scam);
        const size_t pair0 = f * (size_t)(cst * L);
        for (int t = lane; t < C * L; t += WAVE) {
            const int c = t / L, l = t - c * L;
            double u, v, s3[3] = {0.0, 0.0, 0.0};
            if (tau && n >= 2) {            // displaced by v_n tau_c + a_n tau_c^2 (acinoset_misc.py:283-285), as in k_frame_normal
                const double ta = tau[(size_t)b * C + c], ih = 1.0 / M->h;
                const double al = ta * ih + ta * ta * ih * ih, be = -ta * ih - 2.0 * ta * ta * ih * ih, ga = ta * ta * ih * ih;
                for (int d = 0; d < 3; d++) s3[d] = al * qs[(size_t)n * ns + d] + be * qs[(size_t)(n - 1) * ns + d] + ga * qs[(size_t)(n - 2) * ns + d];
            }
            project_point(cams[c], spos[3 * l] + s3[0], spos[3 * l + 1] + s3[1], spos[3 * l + 2] + s3[2], u, v, nullptr);
            const double2 z = reinterpret_cast<const double2*>(meas)[pair0 + t];
            reinterpret_cast<double2*>(meas_err)[pair0 + t] = make_double2(u - z.x, v - z.y);
        }
        if (RAGGED) for (int t = C * L + lane; t < cst * L; t += WAVE) reinterpret_cast<double2*>(meas_err)[pair0 + t] = make_double2(0.0, 0.0);
    }
}
