// cpe_kernels.hip -- hand-written HIP kernels for gfx950 (MI355X): one 64-lane wavefront per frame.
//
//   k_resjac        metric 1: reprojection residual + sparse Jacobian + acceleration slack per frame
//   k_fk            marker positions + centre of mass
//   k_project       closed-form solve of the joint equalities for the dependent angles
//   k_frame_normal  solver: per-frame cost, reduced gradient g[28] and PSD block B[28x28]
//   k_lm_step       solver: one Levenberg-Marquardt step per sequence (block-banded Cholesky over time)
//   k_finalize      solver outputs (q, dq, ddq, positions, meas_err, cost terms)
//
// Data layout in HBM (all fp64, frame-major, so a wave's loads/stores of one frame are contiguous):
//   q[B][N][nq]  meas[B][N][C][L][2]  weight[B][N][C][L]  r[B][N][C][L][2]  J[B][N][C][S][2]  eps[B][N][nq]
// No MFMA: nothing here is a dense contraction larger than 28x28.
#include <hip/hip_runtime.h>

#include "cpe_device.h"

// --------------------------------------------------------------------------------------------------
// shared wave-level building blocks.  LDS arrays are private to the wave (one wave per workgroup).

// sincos of all link angles of the frame held in sq -> ssc[6*link + 2*ang + {0,1}]
__device__ __forceinline__ void wave_sincos(const DevModel* __restrict__ M, const double* sq, double* ssc, int lane) {
    if (lane < 3 * M->nl) {
        double s, c;
        sincos(sq[3 + lane], &s, &c);
        ssc[2 * lane] = s; ssc[2 * lane + 1] = c;
    }
}

// R and dR/d(phi,theta,psi) of every link -> sR[9*(4*link + kind)]
__device__ __forceinline__ void wave_rotations(const DevModel* __restrict__ M, const double* ssc, double* sR, int lane) {
    for (int t = lane; t < 4 * M->nl; t += WAVE) rot_kind(ssc + 6 * (t >> 2), t & 3, sR + 9 * t);
}

// marker positions p_l = x_base + sum_k R_k v_lk  (acinoset_misc.py:1581-1659)
__device__ __forceinline__ void wave_markers(const DevModel* __restrict__ M, const double* sq, const double* sR,
                                             double* spos, int lane) {
    if (lane < M->L) {
        double p0 = sq[0], p1 = sq[1], p2 = sq[2];
        const int n = M->chain_len[lane];
        for (int k = 0; k < n; k++) {
            const double* R = sR + 36 * M->chain_link[lane][k];
            const double v0 = M->chain_vec[lane][k][0], v1 = M->chain_vec[lane][k][1], v2 = M->chain_vec[lane][k][2];
            p0 += R[0] * v0 + R[1] * v1 + R[2] * v2;
            p1 += R[3] * v0 + R[4] * v1 + R[5] * v2;
            p2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
        }
        spos[3 * lane] = p0; spos[3 * lane + 1] = p1; spos[3 * lane + 2] = p2;
    }
}

// d p_marker / d q_dof for Jacobian slot s
__device__ __forceinline__ void slot_dp(const DevModel* __restrict__ M, const double* sR, int s, double& d0, double& d1, double& d2) {
    const int cpos = M->slot_cpos[s];
    if (cpos < 0) {
        const int ax = M->slot_dof[s];
        d0 = ax == 0 ? 1.0 : 0.0; d1 = ax == 1 ? 1.0 : 0.0; d2 = ax == 2 ? 1.0 : 0.0;
    } else {
        const int l = M->slot_marker[s];
        const double* D = sR + 9 * (4 * M->chain_link[l][cpos] + 1 + M->slot_ang[s]);
        const double v0 = M->chain_vec[l][cpos][0], v1 = M->chain_vec[l][cpos][1], v2 = M->chain_vec[l][cpos][2];
        d0 = D[0] * v0 + D[1] * v1 + D[2] * v2;
        d1 = D[3] * v0 + D[4] * v1 + D[5] * v2;
        d2 = D[6] * v0 + D[7] * v1 + D[8] * v2;
    }
}

// roll of a hooke child in closed form: the phi at which the child's z axis is normal to the parent's y axis a (rot_ycol of the parent), from
// the sin / cos of the child's theta (st, ct) and psi (sp, cp).  Returns phi and its sin / cos.  The callers form a themselves: with rot_ycol
// in here the compiler contracts num's sum from another term in k_frame_normal, and the state's last bit moves.
__device__ __forceinline__ void hooke_roll(const double* a, double st, double ct, double sp, double cp, double& phi, double& sphi, double& cphi) {
    const double num = a[0] * st * cp + a[1] * st * sp + a[2] * ct;
    const double den = a[1] * cp - a[0] * sp;
    const double hyp = sqrt(num * num + den * den);
    phi = atan2(num, den);
    sphi = num / hyp; cphi = den / hyp;
}

// closed-form solution of the joint equalities for the dependent angles (branch
// child.y = +parent.y reached from the reference's initial guess, acinoset_opt.py:574-583).
// Updates sq and ssc in place; returns non-zero in every lane if some revolute child sits in the gimbal
// band |cos(theta)| < |a_z| where the equalities have no solution.
__device__ __forceinline__ int wave_project_joints(const DevModel* __restrict__ M, double* sq, double* ssc, int lane, bool hooke_only = false) {
    int clamped = 0;
    double psi0 = 0.0;          // a revolute child's psi as the closed form gives it, before the whole turns towards its parent's psi
    bool rev = false;
    for (int level = 0; level < 2; level++) {
        if (lane < M->nj && !(hooke_only && M->joint_kind[lane] == CPE_JOINT_REVOLUTE_Y)) {
            const int kind = M->joint_kind[lane], p = M->joint_parent[lane], c = M->joint_child[lane];
            const bool lvl1 = kind == CPE_JOINT_HOOKE_YZ && M->dep_of_q[3 + 3 * p] >= 0;   // parent phi is itself dependent
            if ((level == 1) == lvl1) {
                double a[3];
                const double st = ssc[6 * c + 2], ct = ssc[6 * c + 3];
                if (kind == CPE_JOINT_REVOLUTE_Y) {
                    rot_ycol(ssc + 6 * M->joint_body[lane], a);
                    double sphi = a[2] / ct;
                    if (sphi > 1.0) { sphi = 1.0; clamped = 1; }
                    if (sphi < -1.0) { sphi = -1.0; clamped = 1; }
                    const double cphi = sqrt(fmax(0.0, 1.0 - sphi * sphi));
                    psi0 = atan2(a[1], a[0]) - atan2(cphi, sphi * st);
                    rev = true;
                    sq[3 + 3 * c] = asin(sphi);
                    ssc[6 * c] = sphi; ssc[6 * c + 1] = cphi;
                } else {
                    rot_ycol(ssc + 6 * p, a);
                    double phi, sphi, cphi;
                    hooke_roll(a, st, ct, ssc[6 * c + 4], ssc[6 * c + 5], phi, sphi, cphi);
                    sq[3 + 3 * c] = phi;
                    ssc[6 * c] = sphi; ssc[6 * c + 1] = cphi;
                }
            }
        }
        if (level == 0) {
            // whole turns of every revolute child's psi towards its parent's psi.  The parent may be a revolute child of this very pass
            // (hock -> calf -> thigh -> body) whose psi another lane is writing, so the turns are taken again until no psi moves: each
            // child then has seen its parent's final psi, as if the joints had been walked parents first (chain depth + 1 rounds).
            // Every round reads in all lanes before any lane writes.
            const int c = rev ? M->joint_child[lane] : 0, p = rev ? M->joint_parent[lane] : 0;
            for (int round = 0; round <= CPE_MAX_JOINTS; round++) {
                wave_lds_sync();
                double psi = 0.0;
                bool moved = false;
                if (rev) {
                    const double ref = sq[3 + 3 * p + 2];
                    psi = psi0 + 6.283185307179586476925286766559 * rint((ref - psi0) / 6.283185307179586476925286766559);
                    moved = psi != sq[3 + 3 * c + 2];
                }
                wave_lds_sync();
                if (moved) sq[3 + 3 * c + 2] = psi;
                if (!__any(moved)) break;
            }
            if (rev) {
                double s, co; sincos(sq[3 + 3 * c + 2], &s, &co);
                ssc[6 * c + 4] = s; ssc[6 * c + 5] = co;
            }
        }
        wave_lds_sync();
    }
    return __any(clamped);
}

// --------------------------------------------------------------------------------------------------
// State phases of the solver's per-frame kernels (k_frame_normal, k_frame_tracked, k_marker_cov): what each of them rebuilds from the state
// (q, alpha) before its own work, in this order.  The helpers read no model table: the caller loads its lane's packed words (DevModel::fn_lane
// = fw, hk_w, sv_vec; cpe_model.h) where its prefetches belong and passes them in.  (wave_leg_state, the legs' Euler angles, is in cpe_solver.hip.inc.)

// sin / cos of the state: the link angles -> ssc (wave_sincos), the leg angles alpha -> ssa[2 r + {0,1}]
__device__ __forceinline__ void wave_state_sincos(const DevModel* __restrict__ M, const double* sq, const double* sal, double* ssc, double* ssa,
                                                  int nrev, int lane) {
    wave_sincos(M, sq, ssc, lane);
    if (lane < nrev) { double s_, c_; sincos(sal[lane], &s_, &c_); ssa[2 * lane] = s_; ssa[2 * lane + 1] = c_; }
}

// hooke joints: phi of the tails in closed form, one joint per lane from its word fwx (parent | child << 8 | level << 16), level by level:
// a level-1 joint hangs on a link whose own roll is set at level 0
__device__ __forceinline__ void wave_tail_roll(double* sq, double* ssc, int hj_n, int fwx, int lane) {
    for (int level = 0; level < 2; level++) {
        if (lane < hj_n && ((fwx >> 16) & 1) == level) {
            const int p = fwx & 255, c = (fwx >> 8) & 255;
            double a[3], phi, sphi, cphi;
            rot_ycol(ssc + 6 * p, a);
            hooke_roll(a, ssc[6 * c + 2], ssc[6 * c + 3], ssc[6 * c + 4], ssc[6 * c + 5], phi, sphi, cphi);
            sq[3 + 3 * c] = phi;
            ssc[6 * c] = sphi; ssc[6 * c + 1] = cphi;
        }
        wave_lds_sync();
    }
}

// R and dR/d(phi,theta,psi) of the TRUNK links only (leg links are body rotations) -> sR[9 * (4 * trunk slot + kind)]; fwy = the trunk link
// of the lane's block
__device__ __forceinline__ void wave_trunk_rotations(const DevModel* __restrict__ M, const double* ssc, double* sR, int fwy, int lane) {
    if (lane < 4 * M->n_trunk) rot_kind(ssc + 6 * fwy, lane & 3, sR + 9 * lane);
    for (int t = WAVE + lane; t < 4 * M->n_trunk; t += WAVE) rot_kind(ssc + 6 * M->trunk_link[t >> 2], t & 3, sR + 9 * t);     // more than 16 trunk links
}

// dynamic body-frame vector `lane` of the leg markers -> sdyn[3 lane]: sum_i Ry(alpha_r_i) v_i, or dRy/dalpha(alpha_r_0) v_0, from the lane's
// word fww (kind | count << 2 | r_0..2 << 4, 10, 16) and its vectors svv
__device__ __forceinline__ void wave_leg_vectors(const double* ssa, double* sdyn, int svn, int fww, const double (&svv)[3][3], int lane) {
    if (lane < svn) {                                      // sv_n <= CPE_MAX_SDYN < 64
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        if ((fww & 3) == 0) {
            const int cnt = (fww >> 2) & 3;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const int r = (fww >> (4 + 6 * i)) & 63;
                const double sa = ssa[2 * r], ca = ssa[2 * r + 1];
                if (i < cnt) { d0 += ca * svv[i][0] + sa * svv[i][2]; d1 += svv[i][1]; d2 += -sa * svv[i][0] + ca * svv[i][2]; }
            }
        } else {
            const int r = (fww >> 4) & 63;
            const double sa = ssa[2 * r], ca = ssa[2 * r + 1];
            d0 = -sa * svv[0][0] + ca * svv[0][2]; d2 = -ca * svv[0][0] - sa * svv[0][2];
        }
        sdyn[3 * lane] = d0; sdyn[3 * lane + 1] = d1; sdyn[3 * lane + 2] = d2;
    }
}

// S rows of the hooke joints (tails): d phi_c / d(independent) -> sSv, level by level; one host-resolved item per lane, hkw (cpe_model.h).
// A level-1 item (the parent's own roll is dependent) adds d phi_c / d phi_parent times the parent's level-0 entry of that column.
__device__ __forceinline__ void wave_hooke_srows(const double* sR, double* sSv, int hk_n, int2 hkw, int lane) {
    for (int level = 0; level < 2; level++) {
        if (lane < hk_n && ((hkw.x >> 16) & 1) == level) {
            const double* Rp = sR + 36 * (hkw.x & 63); const double* Rc = sR + 36 * ((hkw.x >> 6) & 63);
            const double y0 = Rp[1], y1 = Rp[4], y2 = Rp[7];
            const double z0 = Rc[2], z1 = Rc[5], z2 = Rc[8];
            const double* Dcphi = Rc + 9;
            const double gphi = y0 * Dcphi[2] + y1 * Dcphi[5] + y2 * Dcphi[8];
            const int kind = (hkw.x >> 12) & 3, ang = (hkw.x >> 14) & 3;
            double direct = 0.0;
            if (kind == 0) { const double* D = Rc + 9 * (1 + ang); direct = y0 * D[2] + y1 * D[5] + y2 * D[8]; }
            else if (kind == 1) { const double* D = Rp + 9 * (1 + ang); direct = D[1] * z0 + D[4] * z1 + D[7] * z2; }
            double val = -direct / gphi;
            const int ch = (hkw.y & 0xFFFF) - 1;
            if (ch >= 0) {
                const double* Dpphi = Rp + 9;
                const double t0 = -(Dpphi[1] * z0 + Dpphi[4] * z1 + Dpphi[7] * z2) / gphi;
                val += t0 * sSv[ch];
            }
            sSv[hkw.y >> 16] = val;
        }
        wave_lds_sync();
    }
}

// --------------------------------------------------------------------------------------------------
// metric 1 kernel: residual + sparse Jacobian + acceleration slack.
//
// Persistent workgroups of NW waves; every wave owns one frame at a time and walks the frame list with a
// grid stride.  Read-only model tables (cameras, Jacobian-slot table, marker-chain table) are staged ONCE
// per workgroup in LDS, so the per-frame code has no dependent global loads; the next frame's q / meas /
// neighbour-q are prefetched into registers while the current frame computes and stores.
// Index arithmetic is kept off the vector pipe.  The wave number is read once as a scalar, so the frame index, n = f mod N (carried along:
// one division ahead of the loop, one add and conditional subtract per frame) and the frame's base addresses in q / meas / weight / r / J /
// eps / cost live in scalar registers; every load and store of the loop has the form scalar 64-bit base + 32-bit lane offset (+ immediate).
// What depends on the lane alone -- camera and marker of its pairs in each projection pass, the G offset of its Jacobian slots -- is worked
// out ahead of the loop.  The J loop issues the 15 G reads of a camera back to back, then the 30 multiply-adds, then the five stores, which
// alone are guarded.  None of this changes an operation on r, J or eps or its order (outputs bit-equal to the version before;
// profiles/r04_resjac_notes.md has the instruction counts and the timing).
// LDS (doubles): shared  cam[23C] | ident[10] | slot[4S] | chain[4*L*MAXCHAIN] | clen[(L+1)/2]
//                per wave A[max(6CL, nq+6nl+36nl)] | pos[3L(+1)]   with A = {q, sin/cos, R & dR} later overlaid by G
// Tables are structure-of-arrays so that consecutive lanes touch consecutive LDS words (no bank conflicts):
//   slot:  v0[S] v1[S] v2[S] (double) | doff[S] marker[S] (int32; doff = offset of the 3x3 dR in the wave's R block, <0: identity)
//   chain: v0[K][L] v1[K][L] v2[K][L] (double) | roff[K][L] (int32), K = CPE_MAX_CHAIN, marker index fastest
#define RJ_MAXPASS 4

// A wave-uniform address as the scalar base of the loads and stores built on it (global_load / global_store with an SGPR pair as base and a
// 32-bit VGPR offset).  The empty asm only hides the value's origin: otherwise the loop-invariant lane offset is folded into the kernel
// argument ahead of the loop and the per-frame part is added per lane, in 64-bit vector arithmetic.
// The pointer is cast to the global address space first, so that what comes out of the asm is still known to be global memory.
#define RJ_GLOBAL __attribute__((address_space(1)))
typedef double rj_v2d __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ RJ_GLOBAL T* rj_sbase(T* p) {
    RJ_GLOBAL T* g = (RJ_GLOBAL T*)p;
    asm("" : "+s"(g));
    return g;
}

__host__ __device__ inline int rj_shared_doubles(int C, int L, int S) {
    return 23 * C + 10 + 3 * S + (2 * S + 1) / 2 + 3 * L * CPE_MAX_CHAIN + (L * CPE_MAX_CHAIN + 1) / 2 + (L + 1) / 2;
}
__host__ __device__ inline int rj_wave_doubles(int C, int L, int nq, int nl) {
    const int a = 6 * C * L, b = nq + 6 * nl + 36 * nl;
    return ((a > b ? a : b) + 3 * L + 3) & ~1;
}

template <bool WANT_COST, int NW, int NPASS, int OCC>
__global__ __launch_bounds__(WAVE * NW, (OCC * NW) / 4) void k_resjac(const DevModel* __restrict__ M, int N, long F,
                                                      const double* __restrict__ q, const double* __restrict__ meas,
                                                      const double* __restrict__ weight, double* __restrict__ r,
                                                      double* __restrict__ J, double* __restrict__ eps,
                                                      double* __restrict__ cost) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    // the wave number is the same in all 64 lanes; saying so keeps the frame index, n = f % N and every per-frame base address in scalar registers
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nq = M->nq, nl = M->nl, L = M->L, C = M->C, S = M->S, CL = C * L;
    double* scam = smem;
    double* sident = scam + 23 * C;
    double* slv = sident + 10;                                              // slot vectors [3][S]
    int* sli = reinterpret_cast<int*>(slv + 3 * S);                         // doff[S], marker[S]
    double* chv = slv + 3 * S + (2 * S + 1) / 2;                            // chain vectors [3][K][L]
    int* chr = reinterpret_cast<int*>(chv + 3 * L * CPE_MAX_CHAIN);         // roff[K][L]
    int* sclen = reinterpret_cast<int*>(chv + 3 * L * CPE_MAX_CHAIN + (L * CPE_MAX_CHAIN + 1) / 2);
    double* wbase = smem + ((rj_shared_doubles(C, L, S) + 1) & ~1);
    const int nA = rj_wave_doubles(C, L, nq, nl) - ((3 * L + 3) & ~1) + 0;
    double* wv = wbase + wave * rj_wave_doubles(C, L, nq, nl);
    double* sq = wv;
    double* ssc = sq + nq;
    double* sR = ssc + 6 * nl;
    double* sG = wv;                       // overlays q / sincos / R once they are dead
    double* spos = wv + nA;

    // ---- stage the model tables (once per workgroup)
    for (int t = tid; t < 23 * C; t += WAVE * NW) scam[t] = reinterpret_cast<const double*>(M->cam)[t];
    if (tid < 9) sident[tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
    for (int s = tid; s < S; s += WAVE * NW) {
        const int l = M->slot_marker[s], cpos = M->slot_cpos[s];
        sli[S + s] = l;
        if (cpos < 0) {
            const int ax = cpos == -2 ? 3 : M->slot_dof[s];            // -2: alignment slot, structurally zero
            slv[s] = ax == 0 ? 1.0 : 0.0; slv[S + s] = ax == 1 ? 1.0 : 0.0; slv[2 * S + s] = ax == 2 ? 1.0 : 0.0; sli[s] = -1;
        } else {
            slv[s] = M->chain_vec[l][cpos][0]; slv[S + s] = M->chain_vec[l][cpos][1]; slv[2 * S + s] = M->chain_vec[l][cpos][2];
            sli[s] = 9 * (4 * M->chain_link[l][cpos] + 1 + M->slot_ang[s]);
        }
    }
    for (int t = tid; t < L * CPE_MAX_CHAIN; t += WAVE * NW) {
        const int k = t / L, l = t - k * L;
        const bool on = k < M->chain_len[l];
        chv[t] = on ? M->chain_vec[l][k][0] : 0.0;
        chv[L * CPE_MAX_CHAIN + t] = on ? M->chain_vec[l][k][1] : 0.0;
        chv[2 * L * CPE_MAX_CHAIN + t] = on ? M->chain_vec[l][k][2] : 0.0;
        chr[t] = on ? 36 * M->chain_link[l][k] : 0;
    }
    for (int t = tid; t < L; t += WAVE * NW) sclen[t] = M->chain_len[t];
    const double ih2 = M->ih2, la = M->loss_a, lb = M->loss_b, lc = M->loss_c;
    __syncthreads();

    const cpe_camera* cams = reinterpret_cast<const cpe_camera*>(scam);
    // what depends on the lane alone is worked out once: camera and marker of the lane's pair in every projection pass (an integer division
    // by the run-time L each), and the G offset 6 * marker of the lane's Jacobian slots (lanes past the last slot read marker 0 and store nothing)
    int pcam[NPASS], ppos[NPASS], gofs[5];
#pragma unroll
    for (int p = 0; p < NPASS; p++) {
        const int t = lane + WAVE * p;
        const int c = t < CL ? t / L : 0;
        pcam[p] = c; ppos[p] = t < CL ? 3 * (t - c * L) : 0;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const int s = lane + WAVE * i;
        gofs[i] = s < S ? 6 * sli[S + s] : 0;
    }
    // F < 2^31 (cpe_eval_resjac checks it) and the grid has at most ceil(F / NW) workgroups, so a frame index and its successor fit 32 bits
    // unsigned, and the 64-bit element offsets of a frame are each one 32 x 32 -> 64-bit scalar product
    const unsigned Fu = (unsigned)F, wstride = gridDim.x * NW;
    unsigned f = blockIdx.x * NW + wave;

    // One drain point per frame.  vmcnt counts loads and stores together and the two kinds may retire out of order with
    // respect to each other, so with stores in flight the only safe wait for a load is vmcnt(0) -- which drains every
    // outstanding store of the wave.  The first version waited for its measurements inside each projection pass and for
    // the next q at the frame end: 4 drains per frame, compute and the 26 KB of J stores never overlapped (compute-only
    // 1.86 ms + store-only 2.0 ms ~ 3.1 ms measured).  Now a frame issues all its loads at the top, computes everything
    // (projections and G included) without touching them, waits ONCE, and only then issues its 34 stores in one burst;
    // the burst drains while the next frame computes.
    const rj_v2d* meas2 = reinterpret_cast<const rj_v2d*>(meas);
    // n = f % N is carried along: one division here, then n += wstride % N with a conditional subtraction per frame (n, dn < N < 2^31: the sum fits 32 bits)
    unsigned n = (unsigned)(f % N);
    const unsigned dn = (unsigned)(wstride % N);
    const unsigned ulane = lane;        // per-lane offsets inside a frame fit 32 bits; the frame bases below are 64-bit scalars
    double qreg = 0.0;
    if (f < Fu && lane < nq) qreg = rj_sbase(q + (unsigned long)f * (unsigned)nq)[ulane];
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0) before the loop: its header then carries no pending load on either edge

    while (f < Fu) {
        // Two waves share a SIMD: the one in its dependent chain (rotations, chain walk, projections) goes first at issue, the one in its store
        // burst (independent G reads, products and stores) fills the gaps -- measured -3.0 % against equal priorities, the reverse +0.7 % (60 launches each, interleaved in one process)
        __builtin_amdgcn_s_setprio(2);
        if (lane < nq) sq[lane] = qreg;
        const unsigned fn = f + wstride;
        // element offsets of the frame in q / eps, in meas / weight / r (pairs) and in J (double2)
        const unsigned long fq = (unsigned long)f * (unsigned)nq, fcl = (unsigned long)f * (unsigned)CL, fj = (unsigned long)f * (unsigned)(C * S);
        const bool has_prev = n >= 3u;
        double qn = 0.0, qp1 = 0.0, qp2 = 0.0, qp3 = 0.0;
        rj_v2d mz[NPASS];
        double wz[NPASS];
        if (lane < nq) {
            if (fn < Fu) qn = rj_sbase(q + (unsigned long)fn * (unsigned)nq)[ulane];
            if (has_prev) { qp1 = rj_sbase(q + (fq - nq))[ulane]; qp2 = rj_sbase(q + (fq - 2 * nq))[ulane]; qp3 = rj_sbase(q + (fq - 3 * nq))[ulane]; }
        }
        RJ_GLOBAL const rj_v2d* measf = rj_sbase(meas2 + fcl);
        RJ_GLOBAL const double* weightf = WANT_COST ? rj_sbase(weight + fcl) : nullptr;
#pragma unroll
        for (int p = 0; p < NPASS; p++) {
            const int t = lane + WAVE * p;
            mz[p] = rj_v2d{0.0, 0.0}; wz[p] = 0.0;
            if (t < CL) { mz[p] = measf[ulane + WAVE * p]; if (WANT_COST) wz[p] = weightf[ulane + WAVE * p]; }
        }
        wave_lds_sync();
        if (lane < 3 * nl) {            // wave_sincos with the link count the kernel already holds
            double sn, cs;
            sincos(sq[3 + lane], &sn, &cs);
            ssc[2 * lane] = sn; ssc[2 * lane + 1] = cs;
        }
        wave_lds_sync();
        for (int t = lane; t < 4 * nl; t += WAVE) rot_kind(ssc + 6 * (t >> 2), t & 3, sR + 9 * t);
        wave_lds_sync();
        // marker positions from the LDS chain table.  Two lanes per marker (2 L <= 64): lane l takes the even chain elements
        // (and the base position), lane L + l the odd ones; the halves meet through one cross-lane read.  Halves the depth of
        // the dependent table-index -> rotation reads.
        {
            const int half = lane >= L ? 1 : 0, l = lane - half * L;
            double p0 = 0.0, p1 = 0.0, p2 = 0.0;
            if (lane < 2 * L) {
                if (!half) { p0 = sq[0]; p1 = sq[1]; p2 = sq[2]; }
                const int n = sclen[l];
                const int KL = L * CPE_MAX_CHAIN;
                for (int k = half; k < n; k += 2) {
                    const int t = k * L + l;
                    const double v0 = chv[t], v1 = chv[KL + t], v2 = chv[2 * KL + t];
                    const double* R = sR + chr[t];
                    p0 += R[0] * v0 + R[1] * v1 + R[2] * v2;
                    p1 += R[3] * v0 + R[4] * v1 + R[5] * v2;
                    p2 += R[6] * v0 + R[7] * v1 + R[8] * v2;
                }
            }
            const int partner = (lane + L) & (WAVE - 1);
            const double o0 = __shfl(p0, partner, WAVE), o1 = __shfl(p1, partner, WAVE), o2 = __shfl(p2, partner, WAVE);
            if (lane < L) { spos[3 * lane] = p0 + o0; spos[3 * lane + 1] = p1 + o1; spos[3 * lane + 2] = p2 + o2; }
        }
        // d p / d q of my Jacobian slots (slot s = lane + 64 i) stay in registers
        double dp0[5], dp1[5], dp2[5];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const int s = lane + WAVE * i;
            dp0[i] = dp1[i] = dp2[i] = 0.0;
            if (s < S) {
                const int doff = sli[s];
                const double v0 = slv[s], v1 = slv[S + s], v2 = slv[2 * S + s];
                const double* D = doff < 0 ? sident : sR + doff;
                dp0[i] = D[0] * v0 + D[1] * v1 + D[2] * v2;
                dp1[i] = D[3] * v0 + D[4] * v1 + D[5] * v2;
                dp2[i] = D[6] * v0 + D[7] * v1 + D[8] * v2;
            }
        }
        wave_lds_sync();        // R, sincos, q are dead from here: G may overlay them

        // project every (camera, marker) pair: (u, v) stay in registers, d(u,v)/dp goes to LDS; nothing is stored yet
        RJ_GLOBAL rj_v2d* rf = rj_sbase(reinterpret_cast<rj_v2d*>(r) + fcl);
        double fc = 0.0;
        double2 uv[NPASS];
#pragma unroll
        for (int p = 0; p < NPASS; p++) {
            __builtin_amdgcn_sched_barrier(0);      // keep the passes sequential: interleaving them costs ~40 VGPRs
            const int t = lane + WAVE * p;
            uv[p] = make_double2(0.0, 0.0);
            if (t < CL) {
                const double* pl = spos + ppos[p];
                double u, v, G[6];
                project_point(cams[pcam[p]], pl[0], pl[1], pl[2], u, v, G);      // (the staged form, 210 instead of 225 VGPRs, measured 0.8 % slower here: no occupancy step in reach)
                uv[p] = make_double2(u, v);
                double2* Gd = reinterpret_cast<double2*>(sG + 6 * t);
                Gd[0] = make_double2(G[0], G[1]); Gd[1] = make_double2(G[2], G[3]); Gd[2] = make_double2(G[4], G[5]);
            }
        }
        wave_lds_sync();
        // the frame's only wait on vector memory: this frame's loads have arrived, the previous frame's stores have drained
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_waitcnt(0x0F70);
        // the loaded values become usable HERE: without this the compiler hoists 3*qp1, 3*qp2 to the top of the frame and
        // waits for them there (which drains the previous frame's stores at once)
        asm volatile("" : "+v"(qp1), "+v"(qp2), "+v"(qp3), "+v"(qn));
#pragma unroll
        for (int p = 0; p < NPASS; p++) {
            const int t = lane + WAVE * p;
            if (t < CL) {
                const double e0 = uv[p].x - mz[p].x, e1 = uv[p].y - mz[p].y;
                rf[ulane + WAVE * p] = rj_v2d{e0, e1};
                if (WANT_COST) {
                    const double w = cams[pcam[p]].mult * wz[p];
                    fc += robust_loss(w * e0, la, lb, lc, 0, false).rho + robust_loss(w * e1, la, lb, lc, 0, false).rho;
                }
            }
        }
        // J[c][s][0..1] = G_{c,marker(s)} . dp_s : 16-byte streaming stores, consecutive lanes -> consecutive slots.  Per camera: the G reads
        // of all five slots first (unconditional: a lane without a slot reads marker 0), then the products, then the stores, which alone are
        // guarded -- full rounds of 64 slots by a scalar test, the tail round per lane.  The row base advances on the scalar side.
        const int nfull = S >> 6;
        for (int c = 0; c < C; c++) {
            const double* Gc = sG + 6 * c * L;
            RJ_GLOBAL rj_v2d* Jc = rj_sbase(reinterpret_cast<rj_v2d*>(J) + (fj + (unsigned)(c * S)));
            double2 g0[5], g1[5], g2[5];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                const double2* G = reinterpret_cast<const double2*>(Gc + gofs[i]);
                g0[i] = G[0]; g1[i] = G[1]; g2[i] = G[2];
            }
            rj_v2d val[5];
#pragma unroll
            for (int i = 0; i < 5; i++) {
                val[i].x = g0[i].x * dp0[i] + g0[i].y * dp1[i] + g1[i].x * dp2[i];
                val[i].y = g1[i].y * dp0[i] + g2[i].x * dp1[i] + g2[i].y * dp2[i];
                asm volatile("" : "+v"(val[i]));        // the products stay here, ahead of the guards: sunk into them, each would wait for its G reads on its own
            }
#pragma unroll
            for (int i = 0; i < 5; i++) {
                if (i < nfull || lane + WAVE * i < S) {
#ifdef CPE_RJ_NOSTORE       // diagnostic build only (profiles/r01_resjac_ablation.md): J computed, not stored -- the compute floor of the box
                    if (val[i].x == 1.2345e300) Jc[ulane + WAVE * i] = val[i];
#else
                    __builtin_nontemporal_store(val[i], &Jc[ulane + WAVE * i]);
#endif
                }
            }
        }
        if (WANT_COST) {
            fc = wave_sum(fc);
            if (lane == 0) cost[f] = fc;
        }
        // acceleration slack of the constant-acceleration model (free dq0/ddq0 => 0 for n < 3)
        if (lane < nq) {
            double e = 0.0;
            if (has_prev) e = (qreg - 3.0 * qp1 + 3.0 * qp2 - qp3) * ih2;
            rj_sbase(eps + fq)[ulane] = e;
        }
        qreg = qn;
        f = fn;
        n += dn;
        if (n >= (unsigned)N) n -= (unsigned)N;
        wave_lds_sync();        // G region is rewritten as q / sincos / R by the next frame
    }
}

// --------------------------------------------------------------------------------------------------
// forward kinematics: positions[F][L][3], com[F][3] (acinoset_misc.py:1581-1659, :722-742)
// dynamic LDS: q[nq] | sc[6 nl] | R[36 nl] | pos[3 L]
__global__ __launch_bounds__(WAVE) void k_fk(const DevModel* __restrict__ M, const double* __restrict__ q,
                                             double* __restrict__ positions, double* __restrict__ com) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    const int nq = M->nq, nl = M->nl, L = M->L;
    double* sq = smem;
    double* ssc = sq + nq;
    double* sR = ssc + 6 * nl;
    double* spos = sR + 36 * nl;
    const size_t f = blockIdx.x;
    if (lane < nq) sq[lane] = q[f * nq + lane];
    wave_lds_sync();
    wave_sincos(M, sq, ssc, lane);
    wave_lds_sync();
    for (int t = lane; t < nl; t += WAVE) rot_kind(ssc + 6 * t, 0, sR + 36 * t);
    wave_lds_sync();
    wave_markers(M, sq, sR, spos, lane);
    wave_lds_sync();
    for (int t = lane; t < 3 * L; t += WAVE) positions[f * (size_t)(3 * L) + t] = spos[t];
    if (com) {
        // link origins by walking up the chain (depth <= CPE_MAX_CHAIN), one lane per link
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        if (lane < nl) {
            const double* R = sR + 36 * lane;
            double p0 = R[0] * M->com[lane][0] + R[1] * M->com[lane][1] + R[2] * M->com[lane][2];
            double p1 = R[3] * M->com[lane][0] + R[4] * M->com[lane][1] + R[5] * M->com[lane][2];
            double p2 = R[6] * M->com[lane][0] + R[7] * M->com[lane][1] + R[8] * M->com[lane][2];
            int k = lane;
            while (M->parent[k] >= 0) {
                const int p = M->parent[k];
                const double* Rp = sR + 36 * p;
                p0 += Rp[0] * M->attach[k][0] + Rp[1] * M->attach[k][1] + Rp[2] * M->attach[k][2];
                p1 += Rp[3] * M->attach[k][0] + Rp[4] * M->attach[k][1] + Rp[5] * M->attach[k][2];
                p2 += Rp[6] * M->attach[k][0] + Rp[7] * M->attach[k][1] + Rp[8] * M->attach[k][2];
                k = p;
            }
            const double m = M->mass[lane];
            c0 = m * (p0 + sq[0]); c1 = m * (p1 + sq[1]); c2 = m * (p2 + sq[2]);
        }
        c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
        if (lane == 0) {
            com[3 * f] = c0 * M->inv_total_mass; com[3 * f + 1] = c1 * M->inv_total_mass; com[3 * f + 2] = c2 * M->inv_total_mass;
        }
    }
}

// --------------------------------------------------------------------------------------------------
// marker velocities v_l = (d p_l / d q) dq, the analytic foot velocity of the contact heuristic
// (`foot.Pb_I_vel` lambdified in acinoset_misc.py:347-360).  One lane per marker walks the marker's Jacobian slots.
// dynamic LDS: q[nq] | dq[nq] | sc[6 nl] | R[36 nl]
__global__ __launch_bounds__(WAVE) void k_marker_vel(const DevModel* __restrict__ M, const double* __restrict__ q,
                                                     const double* __restrict__ dq, double* __restrict__ vel) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    const int nq = M->nq, nl = M->nl, L = M->L;
    double* sq = smem;
    double* sdq = sq + nq;
    double* ssc = sdq + nq;
    double* sR = ssc + 6 * nl;
    const size_t f = blockIdx.x;
    if (lane < nq) { sq[lane] = q[f * nq + lane]; sdq[lane] = dq[f * nq + lane]; }
    wave_lds_sync();
    wave_sincos(M, sq, ssc, lane);
    wave_lds_sync();
    wave_rotations(M, ssc, sR, lane);
    wave_lds_sync();
    if (lane < L) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        for (int s = M->slot_off[lane]; s < M->slot_off[lane + 1]; s++) {
            double d0, d1, d2;
            slot_dp(M, sR, s, d0, d1, d2);
            const double w = sdq[M->slot_dof[s]];
            v0 += d0 * w; v1 += d1 * w; v2 += d2 * w;
        }
        double* o = vel + (f * (size_t)L + lane) * 3;
        o[0] = v0; o[1] = v1; o[2] = v2;
    }
}

// --------------------------------------------------------------------------------------------------
// reprojection of stored 3D marker positions into every camera, for the cam*_fte writers
// (acinoset_misc.py:1339-1407).  One lane per (camera, marker) pair; no LDS.
__global__ __launch_bounds__(WAVE) void k_reproject(const DevModel* __restrict__ M, const double* __restrict__ positions,
                                                    double* __restrict__ uv) {
    const int L = M->L, CL = M->C * L;
    const size_t f = blockIdx.x;
    const double* P = positions + f * (size_t)(3 * L);
    for (int t = threadIdx.x; t < CL; t += WAVE) {
        const int c = t / L, l = t - c * L;
        double u, v, G[6];
        project_point(M->cam[c], P[3 * l], P[3 * l + 1], P[3 * l + 2], u, v, G);
        reinterpret_cast<double2*>(uv)[f * (size_t)CL + t] = make_double2(u, v);
    }
}

// --------------------------------------------------------------------------------------------------
// initial-guess ingestion: undistort two detections and triangulate them linearly (triangulate_points[_fisheye],
// acinoset_misc.py:1432-1453: cv[.fisheye].undistortPoints + cv.triangulatePoints), one lane per point pair.
// cam_b < 0: back-projection of the first detection to `depth` along its ray (the monocular rule of the initial
// trajectory estimate).  Pure register code.
__device__ __forceinline__ void undistort_pixel(const cpe_camera& c, double u, double v, double& x, double& y) {
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    if (c.model == CPE_CAM_FISHEYE) {
        // theta_d = theta (1 + D0 theta^2 + .. + D3 theta^8) solved for theta by Newton, then (x, y) *= tan(theta) / theta_d
        const double rd = sqrt(x0 * x0 + y0 * y0);
        double th = rd;
        for (int it = 0; it < 20; it++) {
            const double t2 = th * th;
            const double f = th * (1.0 + t2 * (c.D[0] + t2 * (c.D[1] + t2 * (c.D[2] + t2 * c.D[3])))) - rd;
            const double df = 1.0 + t2 * (3.0 * c.D[0] + t2 * (5.0 * c.D[1] + t2 * (7.0 * c.D[2] + t2 * 9.0 * c.D[3])));
            th -= f / df;
        }
        const double sc = rd > 1e-12 ? tan(th) / rd : 1.0;
        x = x0 * sc; y = y0 * sc;
    } else {
        // radial polynomial inverted by the fixed-point iteration of cv.undistortPoints
        x = x0; y = y0;
        for (int it = 0; it < 20; it++) {
            const double r2 = x * x + y * y;
            const double g = 1.0 + r2 * (c.D[0] + r2 * (c.D[1] + r2 * c.D[2]));
            x = x0 / g; y = y0 / g;
        }
    }
}

__global__ __launch_bounds__(256) void k_triangulate(const DevModel* __restrict__ M, int n, const int* __restrict__ cam_a,
                                                     const int* __restrict__ cam_b, const double* __restrict__ uv_a,
                                                     const double* __restrict__ uv_b, double depth, double* __restrict__ xyz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cpe_camera& ca = M->cam[cam_a[i]];
    double xa, ya;
    undistort_pixel(ca, uv_a[2 * i], uv_a[2 * i + 1], xa, ya);
    double X[3];
    if (cam_b[i] < 0) {
        // X = R^T (depth (x, y, 1) - t)
        const double w[3] = {depth * xa - ca.t[0], depth * ya - ca.t[1], depth - ca.t[2]};
        for (int k = 0; k < 3; k++) X[k] = ca.R[k] * w[0] + ca.R[3 + k] * w[1] + ca.R[6 + k] * w[2];
    } else {
        const cpe_camera& cb = M->cam[cam_b[i]];
        double xb, yb;
        undistort_pixel(cb, uv_b[2 * i], uv_b[2 * i + 1], xb, yb);
        // rows of A: x P[2] - P[0], y P[2] - P[1] for both views, P = [R | t]; the solution is the right singular vector of
        // the smallest singular value.  One-sided (Hestenes) cyclic Jacobi on A itself: pairs of columns of A V are rotated until they are
        // orthogonal; the column of the smallest norm then belongs to the smallest singular value.  (Jacobi on A^T A squares the
        // condition number: at baseline / depth 1e-3 it lost three to four digits against the SVD, tests/test_gpu_ingest_output.py.)
        double A[4][4], V[4][4];
        for (int k = 0; k < 4; k++) {
            const double a0 = k < 3 ? ca.R[k] : ca.t[0], a1 = k < 3 ? ca.R[3 + k] : ca.t[1], a2 = k < 3 ? ca.R[6 + k] : ca.t[2];
            const double b0 = k < 3 ? cb.R[k] : cb.t[0], b1 = k < 3 ? cb.R[3 + k] : cb.t[1], b2 = k < 3 ? cb.R[6 + k] : cb.t[2];
            A[0][k] = xa * a2 - a0; A[1][k] = ya * a2 - a1; A[2][k] = xb * b2 - b0; A[3][k] = yb * b2 - b1;
        }
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) V[r][c] = r == c ? 1.0 : 0.0;
        for (int sweep = 0; sweep < 12; sweep++)
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int q = p + 1; q < 4; q++) {
                    double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) { al += A[k][p] * A[k][p]; be += A[k][q] * A[k][q]; ga += A[k][p] * A[k][q]; }
                    if (fabs(ga) < 1e-300) continue;
                    const double tau = (be - al) / (2.0 * ga);
                    const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
#pragma unroll
                    for (int k = 0; k < 4; k++) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq; }
#pragma unroll
                    for (int k = 0; k < 4; k++) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq; }
                }
        double nrm[4];
#pragma unroll
        for (int k = 0; k < 4; k++) nrm[k] = A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k] + A[3][k] * A[3][k];
        int m = 0;
#pragma unroll
        for (int k = 1; k < 4; k++) if (nrm[k] < nrm[m]) m = k;
        double h[4];
#pragma unroll
        for (int k = 0; k < 4; k++) h[k] = m == 0 ? V[k][0] : m == 1 ? V[k][1] : m == 2 ? V[k][2] : V[k][3];
        for (int k = 0; k < 3; k++) X[k] = h[k] / h[3];
    }
    xyz[3 * i] = X[0]; xyz[3 * i + 1] = X[1]; xyz[3 * i + 2] = X[2];
}

// --------------------------------------------------------------------------------------------------
// DeepLabCut table of one camera -> that camera's slice of meas[N][C][L][2] and weight[N][C][L]
// (init_measurements / init_meas_weights, acinoset_misc.py:211-256).  One lane per (frame, marker): a strided gather.
__global__ __launch_bounds__(256) void k_tensorise_dlc(int N, int L, int n_slots, int slot, const double* __restrict__ table, int rows,
                                                       int parts, int first_row, const int* __restrict__ part_of_marker,
                                                       const double* __restrict__ inv_sigma, double thresh,
                                                       double* __restrict__ meas, double* __restrict__ weight) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * L) return;
    const int n = (int)(i / L), l = (int)(i - (long)n * L);
    const long row = (long)first_row + n;
    double x = 0.0, y = 0.0, w = 0.0;
    const int part = part_of_marker[l];
    if (row >= 0 && row < rows && part >= 0 && part < parts) {
        const double* v = table + row * (long)(3 * parts) + 3 * part;
        const double vx = v[0], vy = v[1], lik = v[2];
        const bool finite = vx == vx && vy == vy && fabs(vx) != INFINITY && fabs(vy) != INFINITY;
        if (finite) { x = vx; y = vy; if (lik > thresh) w = inv_sigma[l]; }
    }
    const long o = ((long)n * n_slots + slot) * L + l;
    meas[2 * o] = x; meas[2 * o + 1] = y; weight[o] = w;
}

// --------------------------------------------------------------------------------------------------
// dependent-angle projection in place.  dynamic LDS: q[nq] | sc[6 nl]
__global__ __launch_bounds__(WAVE) void k_project(const DevModel* __restrict__ M, double* __restrict__ q,
                                                  int* __restrict__ clamped_flag) {
    extern __shared__ double smem[];
    const int lane = threadIdx.x;
    const int nq = M->nq;
    double* sq = smem;
    double* ssc = sq + nq;
    const size_t f = blockIdx.x;
    if (lane < nq) sq[lane] = q[f * nq + lane];
    wave_lds_sync();
    wave_sincos(M, sq, ssc, lane);
    wave_lds_sync();
    const int cl = wave_project_joints(M, sq, ssc, lane);
    if (lane < nq) q[f * nq + lane] = sq[lane];
    if (cl && lane == 0 && clamped_flag) atomicOr(clamped_flag, 1);
}

#include "cpe_solver.hip.inc"
#include "cpe_kinetic.hip.inc"
#include "cpe_kinetic_jac.hip.inc"
#include "cpe_covariance.hip.inc"
#include "cpe_tracked.hip.inc"
#include "cpe_rate_cov.hip.inc"
#include "cpe_force_cov.hip.inc"
#include "cpe_sample.hip.inc"
#include "cpe_force_sample.hip.inc"
#include "cpe_scale.hip.inc"
#include "cpe_scale_cov.hip.inc"
#include "cpe_detection.hip.inc"
