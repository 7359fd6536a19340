/*
 * cpe.h -- C ABI of the MI355X trajectory-optimisation back end for cheetah 3D pose.
 *
 * This is the drop-in boundary.  The reference (zicodasilva/cheetah_pose_estimation) has no FFI: its
 * seam is the hand-off of the Pyomo model to the IPOPT executable,
 *     pe.utils.default_solver(...).solve(robot.m)          acinoset_opt.py:611-617
 * plus the model-building calls around it (acinoset_opt.py:413-536, :539-635).  The entry points below
 * are what a ctypes binding placed at that seam binds.  Plain pointers and sizes,
 * caller-owned buffers, integer status codes, no torch types.
 *
 * Conventions:
 *   - q[54] = [x,y,z,phi,theta,psi]_base then [phi,theta,psi] of links 1..16, absolute ZYX Euler angles;
 *     link order base,bodyF,neck,tail0,tail1,UFL,LFL,HFL,UFR,LFR,HFR,UBL,LBL,UBR,LBR,HBL,HBR
 *     (cheetah.py:197-198).  DOF index of angle j of link i is 3 + 3*i + j.
 *   - all arrays are C-contiguous fp64, frames are the slowest index inside a sequence:
 *     q[B][N][nq], meas[B][N][C][L][2], weight[B][N][C][L].
 *   - "device" entry points take pointers into HBM (e.g. torch-ROCm tensor.data_ptr()); the *_host
 *     variants take host pointers and stage through HBM (PCIe-inclusive).
 */
#ifndef CPE_H
#define CPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPE_MAX_LINKS 20
#define CPE_MAX_MARKERS 32
#define CPE_MAX_CAMS 18      /* 6 cameras x 3: with pairwise pseudo-measurements (m.W = RangeSet(3), acinoset_misc.py:179) every camera
                              * appears three times with the same parameters and its own meas / weight slice */
#define CPE_MAX_JOINTS 16
#define CPE_MAX_BOUNDS 32
#define CPE_MAX_NQ (3 + 3 * CPE_MAX_LINKS)
#define CPE_MAX_GMM 8        /* mixture components of the pose prior */
#define CPE_NX 28            /* size of the reduced / relative-angle vector x (acinoset_misc.py:1699-1757) */
#define CPE_MAX_WINDOW 6     /* window of the linear motion prior (acinoset_opt.py:545): 1..6 (the grid search of run_dataset.py:814-915 also asks for 7) */

typedef int32_t cpe_status;
#define CPE_OK 0              /* converged                                             */
#define CPE_MAX_ITER 1        /* iteration limit reached (solution still written)      */
#define CPE_NUMERICAL 2       /* numerical failure (non-finite cost / factorisation)   */
#define CPE_BAD_ARG (-1)
#define CPE_NO_DEVICE (-2)    /* HIP runtime / GPU unavailable: there is NO CPU fallback */
#define CPE_HIP_ERROR (-3)

/* joint kinds (cheetah.py:71-72,101,160-161): the equalities live in the .robot `angle_constraints` */
#define CPE_JOINT_REVOLUTE_Y 0   /* (R_p e_y).(R_c e_x) = 0 and (R_p e_y).(R_c e_z) = 0 ; child phi,psi dependent */
#define CPE_JOINT_HOOKE_YZ 1     /* (R_p e_y).(R_c e_z) = 0                            ; child phi dependent     */

/* camera models (acinoset_misc.py:1663-1696) */
#define CPE_CAM_FISHEYE 0
#define CPE_CAM_PINHOLE 1

/*
 * Skeleton = absolute-orientation articulated chain.  Every point of the body is
 *     x_base + sum_{k on the path root->link} R_k(q) * v_k
 * origin_i = origin_parent(i) + R_parent(i) * attach[i]   (origin_base = q[0:3])
 * com_i    = origin_i + R_i * com[i]                      (Link3D.Pb_I)
 * marker_l = origin_link(l) + R_link(l) * marker_off[l]   (acinoset_misc.py:1586-1659)
 */
typedef struct cpe_skeleton {
    int32_t n_links;
    int32_t n_markers;
    int32_t n_joints;
    int32_t n_bounds;
    int32_t parent[CPE_MAX_LINKS];
    double attach[CPE_MAX_LINKS][3];
    double com[CPE_MAX_LINKS][3];
    double mass[CPE_MAX_LINKS];
    int32_t marker_link[CPE_MAX_MARKERS];
    double marker_off[CPE_MAX_MARKERS][3];
    int32_t joint_parent[CPE_MAX_JOINTS];
    int32_t joint_child[CPE_MAX_JOINTS];
    int32_t joint_kind[CPE_MAX_JOINTS];
    /* lo <= q[a] - q[b] <= up ; b < 0 means a plain bound on q[a]   (cheetah.py:306-352) */
    int32_t bound_a[CPE_MAX_BOUNDS];
    int32_t bound_b[CPE_MAX_BOUNDS];
    double bound_lo[CPE_MAX_BOUNDS];
    double bound_up[CPE_MAX_BOUNDS];
    /* constant-acceleration model weight 1/Q_p^2, 0 where Q_p = 0 (acinoset_misc.py:234,1852-1908) */
    double motion_w[CPE_MAX_NQ];
    /* relative angles (acinoset_misc.py:508-528): rel[p] = rel_sign[p] * (q[p] - q[rel_ref[p]]),
     * rel_ref[p] < 0 means rel[p] = q[p].  x (28) = rel restricted to the independent dofs. */
    int32_t rel_ref[CPE_MAX_NQ];
    double rel_sign[CPE_MAX_NQ];
} cpe_skeleton;

typedef struct cpe_camera {
    int32_t model;      /* CPE_CAM_FISHEYE | CPE_CAM_PINHOLE */
    int32_t _pad;
    double fx, fy, cx, cy;
    double D[4];        /* fisheye k1..k4 ; pinhole uses D[0..2] */
    double R[9];        /* row-major world->camera rotation */
    double t[3];
    double mult;        /* cam_uncertainty_multiplier (acinoset_misc.py:462-464) */
} cpe_camera;

/* learned priors of the monocular "data-driven" model (config 3) */
typedef struct cpe_priors {
    int32_t gmm_k;                                   /* 0 = pose prior off (acinoset_misc.py:680-714) */
    int32_t gmm_dim;                                 /* 22 = x[6:]                                    */
    double gmm_logw[CPE_MAX_GMM];                    /* log(w_k) - 0.5*logdet(2 pi Sigma_k)           */
    double gmm_mu[CPE_MAX_GMM][CPE_NX];
    double gmm_P[CPE_MAX_GMM][CPE_NX][CPE_NX];       /* precision matrices Sigma_k^-1                 */
    int32_t lr_window;                               /* 0 = motion prior off (acinoset_misc.py:291-336) */
    int32_t _pad;
    double lr_coef[CPE_NX][CPE_MAX_WINDOW * CPE_NX]; /* y = coef . [x_{n-w};...;x_{n-1}] + b, oldest first */
    double lr_b[CPE_NX];
    double lr_w[CPE_NX];                             /* 1/error_variance (0 if variance is 0)         */
} cpe_priors;

typedef struct cpe_options {
    double h;            /* 1/fps; implicit-Euler step of make_pyomo_model (acinoset_opt.py:508) */
    double loss_a, loss_b, loss_c;  /* redescending loss knots 3,10,20 (acinoset_misc.py:479-481) */
    double cost_scale;   /* 1e-3 (acinoset_opt.py:602); only scales the reported objective      */
    double bound_penalty;/* kappa of the augmented Lagrangian that enforces the 23 angle bounds   */
    double bound_tol;    /* bounds are met when the largest violation is below this (rad)         */
    double lambda0;      /* initial Levenberg-Marquardt damping (default 1e-4)                  */
    double tol_step;     /* converged when max |du| < tol_step                                  */
    double tol_cost;     /* ... or relative cost decrease < tol_cost (default 1e-9: within 0.01 mm RMSE of the 1e-12 solution;
                          * the reference runs IPOPT with Tol = 1e-3, acinoset_opt.py:611-617)   */
    int32_t max_iter;
    int32_t curvature;   /* 0: max(rho'', rho'(s)/s, 0) ; 1: max(rho''(s), 0)                     */
    int32_t max_outer;   /* multiplier updates of the augmented Lagrangian (0 = pure penalty)     */
    int32_t _pad;
} cpe_options;

typedef struct cpe_stats {
    int32_t status;      /* cpe_status of this sequence */
    int32_t iterations;  /* LM iterations (accepted + rejected) */
    double cost;         /* final objective, already multiplied by cost_scale */
    double cost_meas, cost_model, cost_pose, cost_motion;   /* estimator.costs (acinoset_opt.py:603-608) */
    double lambda;       /* final damping */
    double max_constraint; /* max |joint equality| at the solution */
    double max_bound_violation; /* largest violation of an angle bound at the solution (rad) */
    int32_t outer;       /* multiplier updates performed */
    int32_t _pad;
} cpe_stats;

typedef struct cpe_handle cpe_handle;

/* ---- life cycle -------------------------------------------------------------------------------- */
/* replaces init_trajectory()'s model construction (acinoset_opt.py:459-525). `priors` may be NULL. */
cpe_status cpe_create(const cpe_skeleton* skel, const cpe_camera* cams, int32_t n_cams,
                      const cpe_options* opts, const cpe_priors* priors, int32_t device,
                      cpe_handle** out);
/* frees everything cpe_create allocated (the reference drops its Pyomo model and calls gc.collect() between sequences,
 * run_dataset.py:1145-1231) */
void cpe_destroy(cpe_handle* h);
/* text of the last failure on this thread's most recent call (the reference raises Python exceptions, acinoset_opt.py:400-406) */
const char* cpe_last_error(void);
/* the values the reference hard-codes: loss knots (3, 10, 20) acinoset_misc.py:2001-2015, fps-derived h acinoset_opt.py:483-487 */
void cpe_default_options(cpe_options* o);
/* stream the handle launches on (hipStream_t as void*), for event timing by the caller */
void* cpe_stream(cpe_handle* h);
cpe_status cpe_synchronize(cpe_handle* h);
/* Synchronisation contract of the device-pointer entry points: they only ENQUEUE work on the handle's own (non-blocking) stream
 * and order nothing against any other stream.  A caller that produced the inputs on another stream (`other`, a hipStream_t as
 * void*; NULL = the legacy default stream; e.g. torch's current stream) calls cpe_stream_wait before the entry point, and
 * cpe_stream_signal after it when that stream will consume the outputs; or it calls cpe_synchronize.  (The reference is
 * synchronous: Pyomo blocks on the IPOPT subprocess, acinoset_opt.py:611-617.) */
cpe_status cpe_stream_wait(cpe_handle* h, void* other);     /* later launches of the handle wait for the work queued on `other` so far */
cpe_status cpe_stream_signal(cpe_handle* h, void* other);   /* `other` waits for the work the handle has queued so far */
/* per-kernel device time of cpe_solve / cpe_solve_kinetic, accumulated by HIP events on the handle's stream while enabled
 * (what the reference stores as processing_time_s is one wall time around .solve(), acinoset_opt.py:610-618).
 * slots: 0 k_frame_normal, 1 k_lr_band, 2 k_lm_step, 3 k_build_act, 4 k_finalize, 5 k_dyn_eval, 6 k_dyn_gather, 7 k_lm_back,
 *        8 k_dyn_assemble, 9 k_dyn_schur, 10 k_dyn_jac, 11 free */
#define CPE_PROFILE_SLOTS 12
cpe_status cpe_profile_enable(cpe_handle* h, int32_t on);                              /* also clears the totals */
cpe_status cpe_profile_get(cpe_handle* h, double* ms /*[12]*/, int64_t* launches /*[12]*/);

/* number of Jacobian slots: the structurally non-zero (marker, dof) pairs, sum_l (3 + 3*chain_len(l)), followed by 0-3
 * structurally ZERO pairs (marker 0, a dof outside its chain; the stored value is 0) that round the count up to a multiple of 4,
 * so that every camera row of J starts on a 64-byte line */
int32_t cpe_jacobian_slots(const cpe_handle* h);       /* (the non-zeros of d measurement_constraints / dq, acinoset_misc.py:278-288) */
/* slot -> (marker, dof) tables; caller provides int32[cpe_jacobian_slots] each */
cpe_status cpe_jacobian_layout(const cpe_handle* h, int32_t* slot_marker, int32_t* slot_dof);
/* the reduced coordinates x of get_relative_angles + get_relative_angle_mask (acinoset_misc.py:487-528, :1699-1757) */
int32_t cpe_num_independent(const cpe_handle* h);                      /* 28 */
cpe_status cpe_independent_dofs(const cpe_handle* h, int32_t* dofs);   /* q index of each reduced coordinate */

/* ---- metric 1: residual + Jacobian evaluation ------------------------------------------------------
 * One pass of acinoset_misc.py:269-288 (pose + measurement constraints) and :639-677 (acceleration
 * slack) over B*N frames; all pointers are DEVICE pointers.
 *   r     [B][N][C][L][2]      reprojection residual  proj(q) - meas   (= slack_meas / fte.pickle meas_err)
 *   J     [B][N][C][S][2]      d r / d q on the S structurally non-zero (marker,dof) slots
 *   eps   [B][N][nq]           acceleration slack ddq_n - ddq_{n-1} (0 for n < 3, free initial states)
 *   cost  [B][N]   (optional)  per-frame sum_c,l,d rho(mult*w*r)  (acinoset_misc.py:459-484), unscaled
 */
cpe_status cpe_eval_resjac(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas,
                           const double* weight, double* r, double* J, double* eps, double* cost);

/* ---- dependent-angle projection: closed-form solve of the 26 joint equalities for the 26 dependent
 * angles given the 28 independent ones (in place on q[B][N][nq], device pointer). */
/* (the `angle_constraints` of the .robot model, created by add_revolute_joint / add_hookes_joint, cheetah.py:71-72,101,160-161) */
cpe_status cpe_project_joints(cpe_handle* h, int32_t B, int32_t N, double* q);

/* ---- building block of the solver: per-frame terms in the reduced coordinates at the Euler
 * iterate q (leg angles are taken as rotations of their body about its y axis, tails re-projected).
 * Device pointers.  g [B][N][28]; Bm [B][N][28][28] (measurement + bound + pose-prior Gauss-Newton block);
 * cost [B][N][3] = {robust measurement cost, bound term, pose-prior term}; gam [B][N][nrev][4] = d (cost pitch of the leg link) / d(alpha, phi_B, theta_B, psi_B) = (1, 0, 1, 0) since round 3;
 * q_out [B][N][nq] = the consistent Euler angles.  gam and q_out may be NULL. */
/* (per frame, what ASL hands IPOPT for measurement_cost acinoset_misc.py:459-484, the angle bounds cheetah.py:306-352 and
 * gmm_pose_cost acinoset_misc.py:680-714: value, gradient and Hessian block) */
cpe_status cpe_eval_normal(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight,
                           double* g, double* Bm, double* cost, double* gam, double* q_out);

/* ---- metric 2: full-trajectory solve ---------------------------------------------------------------
 * replaces default_solver(...).solve(robot.m) for the kinematic model (acinoset_opt.py:589-617).
 * Device pointers.  q_init [B][N][nq] (dependent angles are re-projected), outputs as the reference
 * saves them (acinoset_opt.py:289-361):
 *   q,dq,ddq [B][N][nq] ; positions [B][N][L][3] ; meas_err [B][N][C][L][2] ; stats[B] (HOST pointer)
 * Leg links: q holds the principal ZYX triple of every link (|pitch| <= pi / 2; the same rotation has the triple (phi + pi, pi - theta, psi + pi), which
 * is the one the reference's variables are on while a limb is beyond the horizontal).  The three terms of the objective that act on a leg link's pitch
 * itself -- constant-acceleration cost (acinoset_misc.py:639-677), joint ranges (cheetah.py:306-352), learned priors (acinoset_misc.py:291-336, :680-714)
 * -- are evaluated on theta_body + alpha_link (the leg's angle about its body's y axis): the reference's variable for an unrolled trunk, smooth through
 * +-pi / 2 ("cost pitch").
 */
cpe_status cpe_solve(cpe_handle* h, int32_t B, int32_t N, const double* q_init, const double* meas,
                     const double* weight, double* q, double* dq, double* ddq, double* positions,
                     double* meas_err, cpe_stats* stats);

/* ---- shutter-delay estimation (`shutter_delay_estimation=True`, acinoset_misc.py:179-183, :274-288; run_dataset.py:1323) -----------
 * The reference adds one unknown delay tau_c per camera (camera 1 fixed to 0, |tau_c| <= h) and lets camera c see every marker displaced by
 * q'_base tau_c + q''_base tau_c^2 (implicit-Euler velocity and acceleration of the base position).  Solved here by block-coordinate descent on
 * the reference's objective: cpe_solve's LM with the delays fixed (exact gradient, including the parts that reach frames n-1 and n-2 through q',
 * q''; curvature inside the frame exact, cross-frame curvature blocks left out of the Gauss-Newton model), then one Newton step per delay with
 * the trajectory fixed; the sequence of delay vectors is accelerated by Anderson mixing (memory 4, host side, per sequence: the plain alternation
 * contracts slowly where all delays move together and the trajectory shifts in time), clamped to +-tau_bound; repeated until no delay moves by
 * more than tol_tau (<= max_rounds), then a last trajectory solve.
 * Deviation: the displacement acts from node 2 on (q'_0 and q''_0 are free variables of the reference's collocation: its first two nodes can
 * absorb any displacement).  Device pointers; tau [B][C] (output; tau[.][0] = 0); stats HOST; rounds (HOST, optional) = delay updates done. */
cpe_status cpe_solve_shutter(cpe_handle* h, int32_t B, int32_t N, const double* q_init, const double* meas, const double* weight, double tau_bound,
                             int32_t max_rounds, double tol_tau, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                             double* tau, cpe_stats* stats, int32_t* rounds);

/* host-pointer convenience wrappers of cpe_eval_resjac / cpe_solve above (same reference counterparts: acinoset_misc.py:269-288,
 * acinoset_opt.py:611-617); they stage through HBM, so their rates are PCIe-inclusive */
cpe_status cpe_eval_resjac_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas,
                                const double* weight, double* r, double* J, double* eps, double* cost);
cpe_status cpe_solve_host(cpe_handle* h, int32_t B, int32_t N, const double* q_init, const double* meas,
                          const double* weight, double* q, double* dq, double* ddq, double* positions,
                          double* meas_err, cpe_stats* stats);

/* ---- ragged batches: sequences of their own length, rig and skeleton in ONE solve -----------------------------------------
 * cpe_create_multi: one handle over n_models models, model k = (skels[k], cams[k * CPE_MAX_CAMS .. + n_cams[k]], opts[k]); one set of priors
 * for all of them.  The models must share their shape: n_links, parent, n_markers, marker_link, the joints (joint_parent / child / kind),
 * n_bounds with bound_a / bound_b, rel_ref / rel_sign and the independent dofs; and the options the solver reads per batch: lambda0, tol_step,
 * tol_cost, max_iter, max_outer, curvature, bound_tol, cost_scale.  Everything else may differ per model: h (frame rate), link geometry,
 * masses, marker offsets, bound limits, motion weights, cameras and their count, loss knots, bound_penalty.  A mismatch fails with
 * CPE_BAD_ARG and cpe_last_error() names the field and the model, before the device is opened.  Entry points without a model argument
 * (cpe_solve, cpe_eval_*, cpe_forward_kinematics, the shutter-delay and physics-based solves, ...) see model 0 of such a handle. */
cpe_status cpe_create_multi(int32_t n_models, const cpe_skeleton* skels /*[n_models]*/, const cpe_camera* cams /*[n_models][CPE_MAX_CAMS]*/,
                            const int32_t* n_cams /*[n_models]*/, const cpe_options* opts /*[n_models]*/, const cpe_priors* priors,
                            int32_t device, cpe_handle** out);
/* cpe_solve for B sequences of their own length and model, on any handle (a cpe_create handle has one model: ragged lengths only).
 * model[b] (index into the handle's models) and n_frames[b] (1 .. N_max) are HOST arrays; the others are laid out as cpe_solve's with
 * N = N_max frames per sequence and C_max cameras per frame (the largest camera count of the handle's models):
 *   q_init, q, dq, ddq [B][N_max][nq] ; meas [B][N_max][C_max][L][2] ; weight [B][N_max][C_max][L] ; positions [B][N_max][L][3] ;
 *   meas_err [B][N_max][C_max][L][2] ; stats[B] (HOST).
 * Sequence b reads only its frames n < n_frames[b] and cameras c < its model's count; every output past those is written as 0.0.  Each
 * sequence's outputs and stats are bit-equal to a cpe_solve of that sequence alone on a cpe_create handle of its own model.
 * Kinematic model only (no shutter delay).  Device pointers. */
cpe_status cpe_solve_ragged(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model /*[B] host*/, const int32_t* n_frames /*[B] host*/,
                            const double* q_init, const double* meas, const double* weight, double* q, double* dq, double* ddq,
                            double* positions, double* meas_err, cpe_stats* stats);
/* host-pointer twin of cpe_solve_ragged (stages through HBM) */
cpe_status cpe_solve_ragged_host(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames,
                                 const double* q_init, const double* meas, const double* weight, double* q, double* dq, double* ddq,
                                 double* positions, double* meas_err, cpe_stats* stats);

/* ---- per-frame ground-reaction-force fit (CheetahEstimator.estimate_grf, acinoset_opt.py:176-270).
 * Rows 0-5 (root x, y, z, phi, theta, psi) of d/dt dL/dq' - dL/dq for L = sum_i (m_i |P_i'|^2 / 2 + w_i^T I_i w_i / 2
 * - m_i g P_i,z) are balanced against B = sum_feet (d foot / dq)^T M g (GRFz e_z + sum_k D_k GRFxy_k),
 * D = [+x, +y, -x, -y], for the feet flagged in contact:  minimise |rows - B| subject to 0 <= GRF <= force_max and
 * friction_ratio * GRFz >= sum_k GRFxy_k per foot (acinoset_opt.py:183-192).  Forces are in body weights (M g).
 * The reference hands each frame to IPOPT; the least-squares problem is convex but not strictly (opposing friction
 * components, three or more feet), so IPOPT's answer is one point of a face of minimisers.  Here the Tikhonov term
 * `regularisation` singles out one minimiser (the minimum-norm point of that face in the limit) and a fixed `iterations`
 * count of FISTA with exact projections moves towards it, identically in oracle and HIP.  The fixed count does not reach
 * it: after the default 2000 iterations the objective (8.0e-10) and the net wrench, hence `residual` (1.5e-6), are
 * determined, while the split of the force over the null space of the force matrix is a feasible near-minimum-norm point
 * up to 1.35e-2 body weights from that minimiser (measured against a KKT-certified minimiser, DESIGN.md row a13,
 * tests/test_dynamics_compare.py).  Only the root link's inertia enters rows 0-5 (all other orientations are
 * independent coordinates). */
typedef struct cpe_grf_options {
    double root_inertia[3];   /* principal moments of the root link about its body axes (cheetah: cylinder along x)   */
    double friction_ratio;    /* 1.3 (acinoset_opt.py:190)                                                            */
    double force_max;         /* 5.0 (acinoset_opt.py:186-187)                                                        */
    double regularisation;    /* 1e-6                                                                                 */
    double gravity;           /* 9.81                                                                                 */
    int32_t n_feet;           /* <= 4                                                                                 */
    int32_t foot_marker[4];   /* marker sitting at hock.bottom of each foot (the paw markers), order = output order   */
    int32_t iterations;       /* FISTA iterations (2000)                                                              */
} cpe_grf_options;

/* q, dq, ddq [B][N][nq]; contact [B][N][n_feet] (0 / 1); grfz [B][N][n_feet]; grfxy [B][N][n_feet][4];
 * residual [B][N][6] = rows - B at the solution, in units of M g (may be NULL).  Device pointers. */
/* CheetahEstimator.estimate_grf, acinoset_opt.py:176-270 (one IPOPT launch per frame there) */
cpe_status cpe_grf_fit(cpe_handle* h, const cpe_grf_options* opt, int32_t B, int32_t N, const double* q, const double* dq,
                       const double* ddq, const int32_t* contact, double* grfz, double* grfxy, double* residual);

/* ---- all rows of the equations of motion (the residual function of the physics-based model, config 4 / SURVEY row a12:
 * `make_pyomo_model(include_eom_slack=True)`, acinoset_opt.py:510-514): rows [B][N][nq] = d/dt dL/dq' - dL/dq in N and N m for
 * L = sum_i (m_i |P_i'|^2 / 2 + w_i^T I_i w_i / 2 - m_i g P_i,z), evaluated from (q, q', q'') without forming M, C, G:
 * row of angle a of link i = f_i . (dR_i/da c_i) + sum over the children c of i  F_subtree(c) . (dR_i/da attach_c)
 *                            + (I_i alpha_i + w_i x I_i w_i) . dw_i/dq'_a,     f_j = m_j (P_j'' + g e_z).
 * What the reference balances these rows against (motor torques, the 26 joint constraint forces, contact forces, slack) is
 * cpe_dyn_forces / cpe_eom_residual below, and the solve with all of them as unknowns is cpe_solve_kinetic.  link_inertia:
 * principal moments of every link about its body axes.  Device pointers. */
typedef struct cpe_eom_options {
    double gravity;
    double link_inertia[CPE_MAX_LINKS][3];
} cpe_eom_options;
/* the lambdified equations of motion `eom_f` of the .robot model (acinoset_opt.py:120-161, :510-514) evaluated at (q, dq, ddq) */
cpe_status cpe_eom_rows(cpe_handle* h, const cpe_eom_options* opt, int32_t B, int32_t N, const double* q, const double* dq,
                        const double* ddq, double* rows);

/* ---- generalised forces of the physics-based model: what the rows above are balanced against,
 *   Q = B_grf + B_tau + (dc/dq)^T lambda,
 *   B_grf = sum_feet (d foot / dq)^T  M g (GRFz e_z + sum_k D_k GRFxy_k),  D = [+x, +y, -x, -y]   (forces in body weights)
 *   B_tau = sum_motors (J_w,second - J_w,first)^T  M g tau  R_first e_axis,  J_w,i = d w_i(world) / dq' = R_i dw_i(body)/dq'
 *   c     = the joint equalities in the order of cpe_skeleton.joint_* (two rows per revolute, one per hooke joint)
 * cpe_eom_residual returns rows - Q (the reference's slack_eom).  The pairing of the reference's motor names with
 * (first, second, axis) follows cheetah.py:70-165 and is supplied by the caller; against the reference's `.robot` pickles
 * this is "parity unpinned" -- the tests check virtual work instead (Q . q' = sum F . v_foot + sum T . (w_second - w_first)). */
typedef struct cpe_dyn_options {
    cpe_eom_options eom;
    int32_t n_feet, n_motors;
    int32_t foot_marker[4];
    int32_t motor_first[32], motor_second[32], motor_axis[32];      /* axis 0/1/2 = x/y/z of the FIRST link */
} cpe_dyn_options;
/* tau [B][N][n_motors], lambda [B][N][n_constraints], grf [B][N][n_feet][5] = (z, +x, +y, -x, -y) per foot; any may be NULL (= 0).
 * residual [B][N][nq].  Device pointers. */
/* `slack_eom` of make_pyomo_model(include_eom_slack=True) (acinoset_opt.py:510-514; cost misc.eom_slack_cost, acinoset_misc.py:631) */
cpe_status cpe_eom_residual(cpe_handle* h, const cpe_dyn_options* opt, int32_t B, int32_t N, const double* q, const double* dq,
                            const double* ddq, const double* tau, const double* lambda, const double* grf, double* residual);

/* ---- physics-based trajectory model (config 4: estimate_kinetics, acinoset_opt.py:693-963) -------------------
 * The reference adds to the kinematic NLP, per node: 22 joint torques tau, 26 joint constraint forces lambda (`Fr`), four feet x
 * (GRFz + 4 non-negative friction components), 54 slack_eom, and the equality
 *     rows(q, q', q'') = B_grf + B_tau + (dc/dq)^T lambda + slack            (forces in body weights M g, cpe_eom_residual above)
 * with the cost (acinoset_opt.py:905-921)
 *     1e-3 ( measurement + GMM pose + sum tau^2 + 0.1 fps^-2 sum (fps^2 (pose[n+2] - 2 pose[n+1] + pose[n]))^2 + 10e3 sum slack^2 )
 * -- no constant-acceleration term, no autoregressive prior -- and the contact schedule of prescribe_contact_order
 * (acinoset_misc.py:1140-1167) + the no-slip rule (acinoset_opt.py:783-806): outside stance the foot force is fixed to 0; in stance
 * GRFz >= grfz_min, |foot height| <= foot_height_tol, foot xy speed components <= slip_max; always 0 <= GRF <= force_max and
 * friction * GRFz >= sum_k GRFxy_k.
 *
 * Statement solved here: slack is eliminated (it IS the residual e_n of the equality), the per-node forces
 * f_n = (tau, lambda, net foot force (z, x, y) of every stance foot) enter e_n linearly and are minimised out exactly per node
 * (a convex piecewise-quadratic problem, semismooth Newton), and the trajectory is found by the same Levenberg-Marquardt /
 * block-banded Cholesky as cpe_solve on  V_n(u_n, u_n-1, u_n-2) = min_f [ w_slack |e_n|^2 + w_torque |tau|^2 + ... ]  (n >= 2: q'_0
 * and q''_0 are free in the implicit-Euler collocation, so nodes 0 and 1 carry no dynamics), whose Gauss-Newton blocks are the
 * Schur complements of the force unknowns.  The reference's four non-negative friction components enter only through their
 * differences; the cost-neutral face is resolved by x+ x- = 0 (the minimum-norm point), i.e. net forces with |Fx| + |Fy| <= mu Fz.
 * Inequalities: augmented Lagrangian (multipliers updated with the angle bounds'), including the box [slack_lo, slack_hi] on every
 * component of the residual (the reference's bound_eom_error): inside the node solve its active set is iterated to a fixed point around the
 * exact elimination, like the torque boxes'.  motion_w of the handle's skeleton must be all zero.
 * Versus the reference's `.robot` equations of motion this model is "parity unpinned" (SURVEY 8c-8): the pins are the numerical
 * Lagrangian and virtual work (tests/test_grf.py). */
#define CPE_MAX_MOTORS 32
#define CPE_KIN_MAXLAT (CPE_MAX_MOTORS + 2 * CPE_MAX_JOINTS + 12)    /* latent forces per node: tau | lambda | (z, x, y) per foot */
typedef struct cpe_kinetic_options {
    cpe_dyn_options dyn;      /* gravity, link inertias, feet (markers at the hock bottoms), motors                              */
    double w_slack;           /* 1e4 = `10e3 * slack_cost`            (acinoset_opt.py:921)                                      */
    double w_torque;          /* 1                                    (torque_squared_penalty, :915)                             */
    double w_smooth;          /* 0.1 / fps^2                          (:919-920), on |fps^2 * second difference of the markers|^2 */
    double friction;          /* 0.8                                  (:506)                                                     */
    double force_max;         /* 5                                    (:494-497)                                                 */
    double grfz_min;          /* 0.01                                 (acinoset_misc.py:1144)                                    */
    double foot_height_tol;   /* 0.1; 0.03 for the kinetic dataset    (acinoset_opt.py:780)                                      */
    double foot_height_min;   /* 0: lower bound of `foot_height` outside stance (variable bound inside the absent pe.foot: unpinned); <= -1e9 disables */
    double ground_height;     /* Foot3D.ground_plane_height           (:500)                                                     */
    double slip_max;          /* 1: `gamma <= 1` in stance            (:803-806); <= 0 disables                                  */
    double zvel_max;          /* 1 on the kinetic dataset, else off: `foot_z_vel <= 1` in stance (:807-810, :864-866), read as |vertical foot speed| <= zvel_max
                               * (the variable lives in the absent pe.foot: unpinned); <= 0 disables                             */
    double slack_lo, slack_hi;/* bound_eom_error: box on every slack_eom component, ENFORCED as augmented-Lagrangian rows on the residual:
                               * (-2, 2) run_dataset.py:984, :1211; (-0.1, 0.1) in the last stage of run_kinetic, :1136; lo <= -1e9 and hi >= 1e9: no box */
    double reg_force;         /* Tikhonov weight on lambda and the foot forces (1e-4): picks the minimum-norm point of a face the reference leaves open */
    double kappa_force, kappa_height, kappa_slip;     /* augmented-Lagrangian penalties (1e5, 1e6, 1e2; kappa_slip also serves zvel_max)  */
    double kappa_slack;       /* penalty of the slack box (1e6 = 100 w_slack)                                                    */
    double lm_force_damping;  /* the node forces are eliminated from (H_ff + lambda * lm_force_damping * diag(H_ff) + walls): the trust region
                               * also acts in FORCE space, where the walls of this problem (force bounds, friction polyhedron) are */
    double lm_wall_damping;   /* walls: + lambda * lm_wall_damping * 2 w_slack * sum over the INACTIVE force inequalities c c^T / gap^2
                               * (the Hessian of a log barrier, affine-scaling trust region): forces near a bound are held back in the model */
    int32_t inner_iterations; /* cap on the per-node Newton iterations for the forces (30)                                       */
    int32_t _pad;
} cpe_kinetic_options;

typedef struct cpe_kinetic_stats {
    double cost_torque;       /* sum tau^2                      estimator.costs["torque"]    (acinoset_opt.py:922-928)           */
    double cost_energy;       /* sum (fps^2 second difference)^2               ["energy"]                                        */
    double cost_eom;          /* sum slack^2                                   ["eom_error"]                                     */
    double max_slack;         /* largest |slack_eom| component (body weights), to hold against [slack_lo, slack_hi]              */
    double max_base_rows;     /* largest |rows 0-2 - forces| / (M g): the reference's stored solutions have <= 8e-5 */
    double max_violation;     /* largest violated force / height / slip inequality at the solution                               */
    int32_t inner_max;        /* largest Newton iteration count of a node in the last evaluation                                 */
    int32_t _pad;
} cpe_kinetic_stats;

/* the reference's values for a given frame rate and data set (kinetic_dataset: foot_height_tol 0.03, zvel_max 1) */
void cpe_default_kinetic_options(cpe_kinetic_options* o, double fps, int32_t kinetic_dataset);

/* Device pointers.  q_init [B][N][nq] = the kinematic solution (init_prev_kinematic_solution, acinoset_opt.py:739-777);
 * stance int32 [B][N][n_feet] (1 = the foot is inside a contact window of autogen-contact.json, :783-812);
 * outputs as cpe_solve plus tau [B][N][n_motors], lambda [B][N][n_constraints], grf [B][N][n_feet][5] = (z, +x, +y, -x, -y),
 * slack [B][N][nq] (all zero at nodes 0 and 1); stats / kstats [B] are HOST pointers (kstats may be NULL).
 * cpe_stats.cost_model carries w_torque * torque + w_smooth * energy + w_slack * eom (the reference's "motion prior + slack" part),
 * cpe_stats.cost the whole objective times cost_scale. */
cpe_status cpe_solve_kinetic(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                             const double* weight, const int32_t* stance, double* q, double* dq, double* ddq, double* positions,
                             double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                             cpe_kinetic_stats* kstats);

/* the same with PRESCRIBED foot forces (estimate_kinetics(joint_estimation=False, fix_grf=True), acinoset_opt.py:813-838: GRFz / GRFxy fixed to a
 * synthesised or previously fitted profile): grf_fixed [B][N][n_feet][3] = net force (z, x, y) of every foot in body weights, device pointer,
 * read where stance != 0 (elsewhere the force is zero as before).  The foot forces stop being unknowns of the node -- only torques and
 * joint constraint forces are eliminated -- and the friction / positivity rows drop out, as the reference removes its friction constraint for fixed
 * forces; the foot-height and no-slip rules of the stance frames stay.  grf_fixed == NULL is cpe_solve_kinetic. */
cpe_status cpe_solve_kinetic_fixed(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                                   const double* weight, const int32_t* stance, const double* grf_fixed, double* q, double* dq, double* ddq,
                                   double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                   cpe_kinetic_stats* kstats);

/* the same with every TORQUE BOXED: the reference's module-level estimate_grf (acinoset_opt.py:966-1048, called by run_dataset.py:1138 as the last
 * stage of the kinetic-dataset pipeline) re-solves the physics-based model from the previous solve with `Tc.bounds = bound_value(init_tau, 0.1)` (:995-1003),
 * the foot forces free where the measured force plates saw a contact and zero elsewhere.  tau_box [B][N][n_motors][2] = (lower, upper), device pointer.
 * The boxes are augmented-Lagrangian rows of the node (penalty kappa_force, multipliers updated with the others); inside the node solve their active
 * set is iterated to a fixed point around the exact elimination of torques and constraint forces.  `stance` carries the measured contact pattern. */
cpe_status cpe_solve_kinetic_bounded(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                                     const double* weight, const int32_t* stance, const double* tau_box, double* q, double* dq, double* ddq,
                                     double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                     cpe_kinetic_stats* kstats);

/* the same with the net force of every stance foot BOXED (estimate_kinetics(joint_estimation=False, fix_grf=False), acinoset_opt.py:838-850: `GRFz` and
 * the `GRFxy` sides unfixed within `bound_value(profile, 0.2)`): grf_box [B][N][n_feet][3][2] = (lower, upper) of the net (z, x, y) force in body
 * weights, device pointer, read where stance != 0.  The boxes replace the constants of the positivity / force_max rows of the foot; the friction
 * polyhedron stays, as in the reference (it removes that constraint only when the forces are fixed). */
cpe_status cpe_solve_kinetic_force_box(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q_init, const double* meas,
                                       const double* weight, const int32_t* stance, const double* grf_box, double* q, double* dq, double* ddq,
                                       double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                       cpe_kinetic_stats* kstats);

/* ---- ragged physics-based solve: cpe_solve_kinetic for B sequences of their own length and model in ONE solve, on any handle
 * (a cpe_create_multi handle; a cpe_create handle has one model: ragged lengths only).  opts[k] are the kinetic options of model k (one per model
 * of the handle); model[b] and n_frames[b] (1 .. N_max) are HOST arrays.  The three optional arrays select the variant of the whole batch: all
 * NULL = free foot forces (cpe_solve_kinetic), grf_fixed (cpe_solve_kinetic_fixed), tau_box (cpe_solve_kinetic_bounded) or grf_box
 * (cpe_solve_kinetic_force_box); more than one non-NULL is CPE_BAD_ARG.  Layout as cpe_solve_ragged's, N_max frames and C_max cameras:
 *   q_init, q, dq, ddq, slack [B][N_max][nq] ; meas, meas_err [B][N_max][C_max][L][2] ; weight [B][N_max][C_max][L] ; positions [B][N_max][L][3] ;
 *   stance [B][N_max][n_feet] ; grf_fixed [B][N_max][n_feet][3] ; tau_box [B][N_max][n_motors][2] ; grf_box [B][N_max][n_feet][3][2] ;
 *   tau [B][N_max][n_motors] ; lambda [B][N_max][n_constraints] ; grf [B][N_max][n_feet][5] ; stats, kstats [B] (HOST; kstats may be NULL).
 * Sequence b reads only its frames n < n_frames[b] and cameras c < its model's count; every output past those is written as 0.0.
 * Contract: each sequence's outputs, cpe_stats and cpe_kinetic_stats are BIT-EQUAL to those of the matching cpe_solve_kinetic* call of that
 * sequence alone, on a cpe_create handle of its own model, with its own opts[k] and the same optional array.
 * The kinetic options of all models must agree in the fields that fix the node's unknowns and rows and the arrays' layout: dyn.n_feet,
 * dyn.foot_marker, dyn.n_motors, dyn.motor_first / motor_second / motor_axis.  A mismatch fails with CPE_BAD_ARG before anything is launched
 * and cpe_last_error() names the field and the model.  Every other field may differ per model (inertias, gravity, weights, w_smooth per frame
 * rate, foot_height_tol, zvel_max, slip_max, the slack box, penalties, damping, inner_iterations).  As for cpe_solve_kinetic, motion_w of every
 * model's skeleton must be zero.  Device pointers. */
cpe_status cpe_solve_kinetic_ragged(cpe_handle* h, const cpe_kinetic_options* opts /*[n_models of h]*/, int32_t B, int32_t N_max,
                                    const int32_t* model /*[B] host*/, const int32_t* n_frames /*[B] host*/, const double* q_init, const double* meas,
                                    const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                                    double* q, double* dq, double* ddq, double* positions, double* meas_err, double* tau, double* lambda, double* grf,
                                    double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats);
/* host-pointer twin of cpe_solve_kinetic_ragged (stages through HBM) */
cpe_status cpe_solve_kinetic_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model,
                                         const int32_t* n_frames, const double* q_init, const double* meas, const double* weight, const int32_t* stance,
                                         const double* grf_fixed, const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq,
                                         double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                         cpe_kinetic_stats* kstats);

/* ---- physics-based solve with the 3D kinematic cost (estimate_kinetics(use_2d_reprojections=False), acinoset_opt.py:908-913):
 * inverse dynamics of a given trajectory.  The reprojection cost of every frame is replaced by
 *     T_n = sum_p w_p (x_p(u_n) - x*_{n,p})^2        (acinoset_misc.py:531-590, kinematic_cost)
 * over the CPE_NX relative angles x (base 6, then child-minus-parent angles; the leg pitch on the cost view theta_B + alpha), x* = the same
 * view of q_target [B][N][nq] (Euler; alpha from R_B^T R_c, so either triple of a link gives the same x*).  Everything else is the physics-based
 * model of cpe_solve_kinetic*: the pose prior of the handle, angle bounds, torque / smoothing / slack costs of `opt`, contact rules, the variant
 * chosen by grf_fixed / tau_box / grf_box (at most one non-NULL).  The reference's motion energy in this mode (1e-2 x torque) is expressed
 * through the options: w_smooth = 0, w_torque = 1 + 1e-3 fps^-2.  cpe_stats.cost_meas reports sum_n T_n.
 * track_w [CPE_NX] (ragged: [n_models of h][CPE_NX]), HOST: the weights, finite and >= 0 (cpe_default_track_weights gives the reference's).
 * meas, weight and meas_err may be NULL together (measurements are never read; with meas given, meas_err reports the reprojection errors of
 * the result).  Refused with CPE_BAD_ARG before anything is launched, cpe_last_error() naming the argument: NULL q_target or track_w, meas
 * without weight (or weight without meas), negative or non-finite weights, a non-finite entry of q_target within a sequence's own frames.
 * Layouts, outputs and the ragged contract as cpe_solve_kinetic / cpe_solve_kinetic_ragged; q_target takes q_init's layout. */
void cpe_default_track_weights(double w[CPE_NX]);
cpe_status cpe_solve_kinetic_tracked(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_w, int32_t B, int32_t N, const double* q_init,
                                     const double* q_target, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                     const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions, double* meas_err,
                                     double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats);
cpe_status cpe_solve_kinetic_tracked_host(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_w, int32_t B, int32_t N, const double* q_init,
                                          const double* q_target, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                          const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions,
                                          double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                          cpe_kinetic_stats* kstats);
cpe_status cpe_solve_kinetic_tracked_ragged(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_w, int32_t B, int32_t N_max,
                                            const int32_t* model /*[B] host*/, const int32_t* n_frames /*[B] host*/, const double* q_init,
                                            const double* q_target, const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                            const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions,
                                            double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                            cpe_kinetic_stats* kstats);
cpe_status cpe_solve_kinetic_tracked_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_w, int32_t B, int32_t N_max,
                                                 const int32_t* model, const int32_t* n_frames, const double* q_init, const double* q_target,
                                                 const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                                 const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq, double* positions,
                                                 double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                                 cpe_kinetic_stats* kstats);
/* diagnostic twin of cpe_eval_normal for the tracked per-frame terms (k_frame_tracked): T_n, angle bounds, pose prior at Euler q, multipliers
 * zero.  track_w [CPE_NX]; q, q_target [B][N][nq]; outputs as cpe_eval_normal's (device pointers). */
cpe_status cpe_eval_normal_tracked(cpe_handle* h, const double* track_w, int32_t B, int32_t N, const double* q, const double* q_target, double* g,
                                   double* Bm, double* cost, double* gam, double* q_out);

/* ---- the 3D kinematic cost with the kinematic posterior as its weights (estimate_kinetics(track_weights="posterior")).  Frame n
 * is tracked with its own symmetric matrix,
 *     T_n = (x_n - x*_n)^T W_n (x_n - x*_n),        W_n = (scale / 2) (X Sigma_nn X^T)^-1,        X = dx/du of the cost view,
 * the per-frame Laplace surrogate of the reprojection cost: Sigma_nn is the frame's block of cpe_covariance's cov_diag.  The marginal block
 * ignores the posterior's correlation between frames, so the motion model's information is counted in every frame it touched: `scale` is the
 * caller's handle on that.
 * cpe_track_precision: cov_diag, W [B][N][CPE_NX][CPE_NX] (device pointers; _host: host pointers), scale finite and > 0; model / n_frames [B]
 * (HOST) as cpe_solve_ragged's with N = N_max, or both NULL (B sequences of N frames of the first model).  W_n is bit-symmetric.  A block
 * without a Cholesky factor (a pivot that is not positive and finite) gets W_n = 0 and the call returns CPE_NUMERICAL, cpe_last_error() naming
 * the first such sequence and frame; the other frames are written.  Frames past a sequence's own are not written (_host: they come back zero).
 * NULL cov_diag or W, or a bad scale: CPE_BAD_ARG, cpe_last_error() naming the argument. */
cpe_status cpe_track_precision(cpe_handle* h, int32_t B, int32_t N, const int32_t* model /*[B] host or NULL*/, const int32_t* n_frames /*[B] host or NULL*/,
                               const double* cov_diag, double scale, double* W);
cpe_status cpe_track_precision_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* cov_diag,
                                    double scale, double* W);
/* cpe_solve_kinetic_tracked* with track_W [B][N][CPE_NX][CPE_NX] (x-space; a device pointer, a host pointer in the _host forms) in place of
 * track_w; every other argument, layout, output and the ragged contract are theirs, and cpe_stats.cost_meas reports sum_n T_n.  Every W_n must
 * be symmetric and positive semi-definite: positive semi-definiteness is the caller's contract and is not checked (an indefinite W_n gives an
 * indefinite Gauss-Newton block).  Refused with CPE_BAD_ARG before anything is launched, cpe_last_error() naming the argument: NULL track_W or
 * q_target, meas without weight (or weight without meas), a non-finite entry of q_target; and, in the _host forms only (the device forms do not
 * copy 6 KB per frame back), within a sequence's own frames a non-finite entry of track_W, a negative diagonal entry, or W[i][j] != W[j][i]. */
cpe_status cpe_solve_kinetic_tracked_weighted(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_W, int32_t B, int32_t N,
                                              const double* q_init, const double* q_target, const double* meas, const double* weight, const int32_t* stance,
                                              const double* grf_fixed, const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq,
                                              double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack, cpe_stats* stats,
                                              cpe_kinetic_stats* kstats);
cpe_status cpe_solve_kinetic_tracked_weighted_host(cpe_handle* h, const cpe_kinetic_options* opt, const double* track_W, int32_t B, int32_t N,
                                                   const double* q_init, const double* q_target, const double* meas, const double* weight,
                                                   const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double* q,
                                                   double* dq, double* ddq, double* positions, double* meas_err, double* tau, double* lambda, double* grf,
                                                   double* slack, cpe_stats* stats, cpe_kinetic_stats* kstats);
cpe_status cpe_solve_kinetic_tracked_weighted_ragged(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_W, int32_t B, int32_t N_max,
                                                     const int32_t* model /*[B] host*/, const int32_t* n_frames /*[B] host*/, const double* q_init,
                                                     const double* q_target, const double* meas, const double* weight, const int32_t* stance,
                                                     const double* grf_fixed, const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq,
                                                     double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack,
                                                     cpe_stats* stats, cpe_kinetic_stats* kstats);
cpe_status cpe_solve_kinetic_tracked_weighted_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, const double* track_W, int32_t B, int32_t N_max,
                                                          const int32_t* model, const int32_t* n_frames, const double* q_init, const double* q_target,
                                                          const double* meas, const double* weight, const int32_t* stance, const double* grf_fixed,
                                                          const double* tau_box, const double* grf_box, double* q, double* dq, double* ddq,
                                                          double* positions, double* meas_err, double* tau, double* lambda, double* grf, double* slack,
                                                          cpe_stats* stats, cpe_kinetic_stats* kstats);
/* cpe_eval_normal_tracked with track_W [B][N][CPE_NX][CPE_NX] (device pointer) in place of track_w */
cpe_status cpe_eval_normal_tracked_weighted(cpe_handle* h, const double* track_W, int32_t B, int32_t N, const double* q, const double* q_target, double* g,
                                            double* Bm, double* cost, double* gam, double* q_out);

/* diagnostic building block of cpe_solve_kinetic (as cpe_eval_normal is of cpe_solve): ONE evaluation of the physics terms of every node at
 * Euler q, multipliers zero, forces from a cold start -- what ASL hands IPOPT per node for the constraints of make_pyomo_model(include_eom_slack=True)
 * (acinoset_opt.py:510-514) after the node forces are minimised out.  Device pointers, each may be NULL: f [B][N][64] node forces (tau | lambda |
 * (z, x, y) per foot), stat [B][N][8] = (sum slack^2, sum tau^2, regularised norm, smoothing energy, multiplier terms, max |slack|, max |base rows|,
 * max violation), g [B][N][84] gradient with respect to the coordinates of frames n, n-1, n-2, Huu [B][N][84][84], Hfu [B][N][64][84], Hff [B][N][64][64]
 * (rows = free node forces in meta's order), meta int32 [B][N][65] = (count, indices). */
cpe_status cpe_eval_kinetic_nodes(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                  const double* weight, const int32_t* stance, double* f, double* stat, double* g, double* Huu, double* Hfu,
                                  double* Hff, int32_t* meta);
/* cpe_eval_kinetic_nodes with the variants of cpe_solve_kinetic_ragged -- grf_fixed [B][N][nf][3], tau_box [B][N][n_motors][2], grf_box
 * [B][N][nf][3][2], device pointers, at most one non-NULL (else CPE_BAD_ARG) -- and the band system of the physics-based solve that this
 * evaluation gives at the damping a solve starts with (opts.lambda0 of the handle), device pointers, each may be NULL: gk [B][N][28] gradient,
 * Bk [B][N][28][28] diagonal block, Hk [B][N][2][28][28] blocks (m, m-1) and (m, m-2) of frame m; the node forces enter the band through
 * their elimination at that damping (lm_force_damping, lm_wall_damping).  In both entries the per-node outputs of nodes 0 and 1, and the
 * entries past a node's free forces, are zero. */
cpe_status cpe_eval_kinetic_system(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                   const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                                   double* f, double* stat, double* g, double* Huu, double* Hfu, double* Hff, int32_t* meta, double* gk, double* Bk,
                                   double* Hk);
/* Diagnostic building block of both solves, for tests: exactly the first LM iteration of cpe_solve (kopt NULL, stance NULL) or of
 * cpe_solve_kinetic (kopt and stance given; free foot forces; the handle's half-bandwidth must be 3) from Euler q, at the damping lam > 0 in
 * place of opts.lambda0 -- the same launches as the solve's first pass: evaluation, band assembly, block Cholesky factor, forward and back
 * substitution, trial iterate.  In the physics-based model the node forces are eliminated at that damping too.  Outputs, device pointers
 * except seq, each may be NULL except seq (pb = the half-bandwidth in frames: 3, or the motion prior's window when that is larger):
 *   g [B][N][28]      total gradient of the objective in the reduced coordinates (per-frame terms, constant-acceleration model, motion prior,
 *                     eliminated physics terms)
 *   dg [B][N][28]     diagonal of the Gauss-Newton matrix H before damping; the damped matrix is H + lam diag(max(dg, floor)), floor 0.1
 *                     for N < 4, else 1e-12
 *   L [B][N][pb+1][28][28]  block [n][i] = block (n + i, n) of the lower Cholesky factor of the damped matrix, row-major, with its true
 *                     diagonal; zero where n + i >= N
 *   delta [B][N][28]  the step: (H + lam diag(...)) delta = -g
 *   state [B][N][2][ns]  the current state (Euler q made consistent, then the leg angles) and the trial state = current + delta at the slot
 *                     of every reduced coordinate
 *   seq [B][8]        HOST: cost terms of the evaluation (meas, model, bound, pose, motion -- the physics-based model reports its own cost
 *                     in the last), predicted decrease, max |delta|, status: CPE_OK where a step was made, CPE_NUMERICAL where the
 *                     evaluation is not finite or the damped matrix has no Cholesky factor -- that sequence has g, dg, L and delta zero
 *                     and its trial state is not defined. */
cpe_status cpe_eval_lm_step(cpe_handle* h, const cpe_kinetic_options* kopt, int32_t B, int32_t N, const double* q, const double* meas,
                            const double* weight, const int32_t* stance, double lam, double* g, double* dg, double* L, double* delta, double* state,
                            double* seq);
/* Diagnostic building block of the shutter-delay estimation, for tests: exactly the first pass of a round of cpe_solve_shutter from Euler q at
 * the delays tau [B][C] (device; tau[b][0] is the reference camera's and is read like the others) and the damping lam > 0 in place of
 * opts.lambda0 -- the same launches: the cold start, k_frame_normal in its shutter-delay branch (+ the motion prior's band), k_lm_step with the
 * collection of the cross-frame gradient parts, k_lm_back; then k_shutter_step and k_finalize with the delays, both at the evaluated iterate
 * (a first pass accepts nothing).  It stands for the reference's displaced view, acinoset_misc.py:179-183 and :278-288: camera c sees the
 * markers of frame n >= 2 at p + v_n tau_c + a_n tau_c^2, v and a the backward differences of the base position.  Outputs, device pointers
 * except seq, each may be NULL except seq:
 *   g [B][N][28], Bm [B][N][28][28], cost [B][N][3]   k_frame_normal's per-frame terms with the displacement (cpe_eval_normal's layouts); on a
 *                     handle with a motion prior g and Bm are read after that prior's band kernel has added its per-frame part
 *   gx [B][N][6]      the parts of frame n's measurement gradient that belong to the base positions of frames n-1 (0..2) and n-2 (3..5)
 *   rcb [B][N][C][9]  per camera: the gradient of the frame's measurement cost with respect to a displacement of that camera's markers (3), and the
 *                     upper triangle xx, xy, xz, yy, yz, zz of its Gauss-Newton matrix (6)
 *   g_total [B][N][28]  k_lm_step's total gradient, gx collected (cpe_eval_lm_step's g)
 *   step [B][C]       k_shutter_step's Newton step of every delay with the trajectory held fixed; step[b][0] = 0, and 0 for N < 3
 *   meas_err [B][N][C][L][2]  pixel minus measurement of the displaced view at the evaluated iterate (cpe_solve_shutter's meas_err)
 *   seq [B][8]        HOST, as cpe_eval_lm_step
 * CPE_BAD_ARG, the reason in cpe_last_error(): a null required argument, lam <= 0 or not finite, a handle of several models (cpe_create_multi:
 * the shutter-delay path has no ragged form).  The _host twin takes host pointers throughout and stages through HBM. */
cpe_status cpe_eval_shutter_step(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, const double* tau,
                                 double lam, double* g, double* Bm, double* cost, double* gx, double* rcb, double* g_total, double* step,
                                 double* meas_err, double* seq);
cpe_status cpe_eval_shutter_step_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, const double* tau,
                                      double lam, double* g, double* Bm, double* cost, double* gx, double* rcb, double* g_total, double* step,
                                      double* meas_err, double* seq);
/* Diagnostic building block of every solve, for tests: the launch window.  After its first pass a solve lists, before every iteration and on the
 * device, the first `window` sequences that are still running (k_build_act), and every kernel of the iteration works on that list.  This entry
 * runs that one launch, through the launch statement of the solves, on a scratch state array of B sequences whose status words are status[b]
 * (0 = running, anything else = finished) and whose other fields are zero.  HOST pointers.  Outputs:
 *   act [window + 64]  the indices of the first min(count, window) running sequences in ascending order; every entry after them, the 64 past
 *                     `window` included, reads -1 (the entry fills the array with -1 before the launch: the kernel writes nothing else)
 *   n_act              min(count, window), count = the number of running sequences
 * window > B is allowed (no solve passes it): the list is then every running sequence.  The entry allocates its own buffers, leaves the handle's
 * solver workspace alone and drains the stream before it returns.  CPE_BAD_ARG, with the argument's name in cpe_last_error(): a null h, status,
 * act or n_act; B < 1; window < 1. */
cpe_status cpe_eval_active_list(cpe_handle* h, int32_t B, int32_t window, const int32_t* status, int32_t* act, int32_t* n_act);

/* ---- posterior covariance of the kinematic estimate ("What is inverted").  The reference returns one trajectory and no measure
 * of how well the data determine it (IPOPT's reduced Hessian is never asked for, acinoset_opt.py:611-617).  Here
 *     Sigma = (H + ridge D)^-1      on its block band,
 * H = the Gauss-Newton matrix of cpe_solve's objective in the 28 reduced coordinates per frame (measurement, constant-acceleration, bound-penalty,
 * pose-prior and motion-prior terms) exactly as the first LM pass of cpe_solve assembles it at q, D = max(diag H, floor) with cpe_eval_lm_step's
 * floors.  Sigma comes from the block Cholesky factor of that pass by selected inversion (Takahashi recurrence); no dense inverse is formed.
 * Named deviations: (scale) the objective is taken as the negative log posterior as it stands, cost_scale plays no part; (bounds) multipliers are
 * zero: a bound violated at q contributes its penalty curvature, a bound that is met nothing -- the Laplace approximation of the unbounded posterior;
 * (robust loss) the curvature is the solver's PSD weight (opts.curvature), so redescended outliers carry no information; (coordinates) the reduced
 * ones: trunk entries are Euler angles or metres, leg entries the rotation about the body's y axis (cpe_independent_dofs names them).
 * cpe_covariance* take the kinematic objective (no shutter displacement); cpe_covariance_kinetic below the physics-based one.  Every covariance entry refuses with CPE_BAD_ARG, before the device
 * is touched and with the reason in cpe_last_error(): ridge < 0 or not finite; a handle whose half-bandwidth is above 4 (motion-prior windows 5, 6). */
/* the refusals above for a handle that cpe_create would build with `priors` (NULL = none), without a handle: CPE_BAD_ARG, else CPE_NO_DEVICE
 * where no GPU is visible, else CPE_OK */
cpe_status cpe_covariance_supported(const cpe_priors* priors, double ridge);
/* Building block: selected inverse of a block-banded Cholesky factor.  Device pointers.  L [B][N][pb+1][28][28] in cpe_eval_lm_step's layout
 * (block [n][i] = block (n + i, n) of the lower factor, row-major, true diagonal; blocks with n + i >= N are not read).  cov_diag [B][N][28][28] =
 * Sigma(n, n), exactly symmetric; cov_off [B][N][pb][28][28] (may be NULL): block [n][i-1] = Sigma(n + i, n), zero where n + i >= N. */
cpe_status cpe_band_inverse(cpe_handle* h, int32_t B, int32_t N, const double* L, double* cov_diag, double* cov_off);
/* Sigma at Euler q [B][N][nq]: the launches of a solve's first pass up to the factor (cold start, multipliers zero, as cpe_eval_lm_step) at damping
 * ridge >= 0, then the sweep.  Device pointers except status.  cov_diag, cov_off as above; cov_pos [B][N][L][3][3] (may be NULL) = P_l Sigma(n,n) P_l^T,
 * P_l = d marker_l / d u: the covariance of every marker position in metres^2; L (may be NULL) = the factor used, in cpe_band_inverse's layout (cov_diag
 * and cov_off are bit-equal to cpe_band_inverse of it).  status [B], HOST: CPE_OK, or CPE_NUMERICAL where the evaluation is not finite or the matrix
 * has no Cholesky factor at that ridge -- all outputs of such a sequence are zero; the damping is never raised silently.  Returns the worst status.
 * Results are reproducible bit for bit (no atomics in the sweep), and a sequence's outputs do not depend on its batch. */
cpe_status cpe_covariance(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, double ridge,
                          double* cov_diag, double* cov_off, double* cov_pos, double* L, cpe_status* status);
/* the same for sequences of their own length and model, in cpe_solve_ragged's layout (N_max frames, C_max cameras; model, n_frames HOST); every
 * output past a sequence's frames is 0.0 */
cpe_status cpe_covariance_ragged(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model /*[B] host*/, const int32_t* n_frames /*[B] host*/,
                                 const double* q, const double* meas, const double* weight, double ridge, double* cov_diag, double* cov_off,
                                 double* cov_pos, double* L, cpe_status* status);
/* host-pointer twins (stage through HBM) */
cpe_status cpe_covariance_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* meas, const double* weight, double ridge,
                               double* cov_diag, double* cov_off, double* cov_pos, double* L, cpe_status* status);
cpe_status cpe_covariance_ragged_host(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q,
                                      const double* meas, const double* weight, double ridge, double* cov_diag, double* cov_off, double* cov_pos,
                                      double* L, cpe_status* status);

/* ---- posterior covariance of the rates ("What is propagated"): how well the data determine velocities, accelerations and the
 * centre of mass, from a covariance band the entries above return.  A rate is a fixed linear stencil over at most three consecutive frames, so its
 * covariance needs Sigma(n,n), Sigma(n+1,n), Sigma(n+2,n) only -- all inside the band.  The entry does not care where Sigma came from
 * (cpe_covariance*, cpe_covariance_kinetic*, cpe_band_inverse, or a band of the caller's); values are not validated.
 * Device pointers.  q [B][N][nq]: Euler angles as cpe_covariance takes them (cold start of the state); cov_diag [B][N][28][28] and cov_off
 * [B][N][pb][28][28] (block [n][i-1] = Sigma(n+i, n), pb = the handle's half-bandwidth): cpe_band_inverse's layout.
 * With NL the sequence's length, h its model's time step and u_n the 28 reduced coordinates (the gauge of the solve's dq / ddq at the first frames):
 *   cov_du      [B][N][28][28]   covariance of the reduced velocity: row n >= 1 (u_n - u_{n-1}) / h; row 0 (-2 u_0 + 3 u_1 - u_2) / h if NL >= 3,
 *                                (u_1 - u_0) / h if NL == 2, zero if NL == 1
 *   cov_ddu     [B][N][28][28]   covariance of (u_m - 2 u_{m-1} + u_{m-2}) / h^2, m = max(n, 2); zero if NL < 3 (rows 0, 1, 2 are bit-equal)
 *   cov_vel     [B][N][L][3][3]  first-order covariance of the marker velocity (p_l(u_n) - p_l(u_{n-1})) / h:
 *                                (P_n S_nn P_n^T + P_{n-1} S_{n-1,n-1} P_{n-1}^T - P_n S_{n,n-1} P_{n-1}^T - (that)^T) / h^2; row 0 is zero
 *   cov_com     [B][N][3][3]     Pc_n S_nn Pc_n^T, the covariance of the centre of mass in metres^2
 *   cov_com_vel [B][N][3][3]     the velocity formula with Pc; row 0 is zero, row k + 1 belongs to the velocity between the frames k and k + 1
 *   jac_pos     [B][N][L][3][28] P_l = d p_l / d u, dense (exactly 0.0 in the columns a marker does not depend on): cpe_covariance's cov_pos is
 *                                P_l Sigma(n,n) P_l^T of these numbers
 *   jac_com     [B][N][3][28]    Pc = d com / d u, com as cpe_forward_kinematics returns it: the mass-weighted mean of the link centres' columns
 * Every output may be NULL, but not all of them.  Every block is symmetric bit for bit; every sum has a fixed order (no atomics): results are
 * reproducible bit for bit and a sequence's outputs do not depend on its batch.  All outputs are linear in Sigma: a sequence whose band is zero
 * (cpe_covariance found no factor) gets zero covariances.  du of a trunk coordinate is the rate of the Euler angle cpe_independent_dofs names, du of
 * a leg coordinate the rate of its rotation about the body's y axis.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): negative sizes; NULL h, q, cov_diag or cov_off; all
 * outputs NULL; a centre-of-mass output for a skeleton whose link centres do not fit the marker tables. */
cpe_status cpe_rate_covariance(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* cov_diag, const double* cov_off, double* cov_du,
                               double* cov_ddu, double* cov_vel, double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com);
/* the same for sequences of their own length and model, in cpe_covariance_ragged's layout (N_max frames; model, n_frames HOST): NL = n_frames[b], h
 * and the Jacobians those of model[b]; everything past a sequence's frames reads 0.0.  Also refused: NULL model or n_frames, a model index or frame
 * count out of range, a plain handle (cpe_create). */
cpe_status cpe_rate_covariance_ragged(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model /*[B] host*/, const int32_t* n_frames /*[B] host*/,
                                      const double* q, const double* cov_diag, const double* cov_off, double* cov_du, double* cov_ddu, double* cov_vel,
                                      double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com);
/* host-pointer twins (stage through HBM) */
cpe_status cpe_rate_covariance_host(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* cov_diag, const double* cov_off,
                                    double* cov_du, double* cov_ddu, double* cov_vel, double* cov_com, double* cov_com_vel, double* jac_pos,
                                    double* jac_com);
cpe_status cpe_rate_covariance_ragged_host(cpe_handle* h, int32_t B, int32_t N_max, const int32_t* model, const int32_t* n_frames, const double* q,
                                           const double* cov_diag, const double* cov_off, double* cov_du, double* cov_ddu, double* cov_vel,
                                           double* cov_com, double* cov_com_vel, double* jac_pos, double* jac_com);

/* ---- covariance between distant frames ("What is spanned"): the blocks Sigma(n, a) of a whole column above an anchor frame a, far
 * outside the band -- what the error bar of a displacement, a stride length or a mean speed between two frames needs.  L^T Sigma = L^-1 is lower
 * triangular, so the sweep's recurrence continues upward: Sigma(n, a) = - sum_{k=1..pb} G_k(n)^T Sigma(n+k, a), G_k(n) = L(n+k, n) L(n, n)^-1, for
 * n = a-pb-1 .. 0, seeded by the band blocks Sigma(a-i, a) = Sigma(a, a-i)^T -- the back substitution of L^T X = Y on the rows where Y = 0.
 * Device pointers except n_frames and anchors.  L [B][N][pb+1][28][28], cov_diag [B][N][28][28], cov_off [B][N][pb][28][28]: cpe_band_inverse's
 * layout, pb = the handle's half-bandwidth, from cpe_covariance*, cpe_covariance_kinetic*, cpe_band_inverse or the caller; values are not validated.
 * n_frames [B] HOST: the length of every sequence, or NULL = all N.  anchors [B][K] HOST: frame indices, -1 = unused slot.
 * cols [B][K][N][28][28]: block [b][k][n] = Sigma(n, a), a = anchors[b][k], for n <= a; the rows a-pb .. a are bit-copies of the band blocks
 * (transposed where needed); exactly 0.0 for n > a, for an unused slot and past a sequence's frames.  A sequence all of whose anchors are -1 is not
 * read at all: the way to skip a sequence for which cpe_covariance found no factor.  Every sum has a fixed order (no atomics): results are
 * reproducible bit for bit, and a column depends neither on the batch nor on the other anchors of the call.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): a NULL argument other than n_frames; K < 1; an anchor
 * outside [-1, n_frames[b]); a frame count outside [0, N]; a half-bandwidth above 4; negative sizes or more than 2^31 - 1 blocks (B N K). */
cpe_status cpe_covariance_columns(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames /*[B] host, or NULL*/, const double* L,
                                  const double* cov_diag, const double* cov_off, int32_t K, const int32_t* anchors /*[B][K] host*/, double* cols);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_covariance_columns_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, const double* L, const double* cov_diag,
                                       const double* cov_off, int32_t K, const int32_t* anchors, double* cols);

/* ---- draws from the posterior of the kinematic estimate ("What is sampled"): whole trajectories, for the error bar of any quantity a
 * caller computes from a trajectory -- also one that is no smooth function of a few neighbouring frames and has no Jacobian here (a joint-angle range
 * over a stride, the foot height at touch-down, a detected contact window).  With z ~ N(0, I) the solution of L^T du = z has covariance
 * L^-T L^-1 = Sigma: the full matrix, not only its band.
 * cpe_band_sample, the building block (pure linear algebra): for every sequence b and sample s, newest frame first (NL the sequence's length),
 *     du_n = L(n,n)^-T (z_n - sum_{i=1..pb} L(n+i,n)^T du_{n+i}),        n = NL-1 .. 0,   blocks with n + i >= NL are not used.
 * Device pointers except n_frames.  L [B][N][pb+1][28][28]: cpe_band_inverse's layout with the true diagonal, pb = the handle's half-bandwidth, from
 * cpe_covariance*, cpe_covariance_kinetic*, cpe_eval_lm_step or the caller; values are not validated.  z, du [B][S][N][28]: sample s of sequence b is
 * one contiguous trajectory.  n_frames [B] HOST: the length of every sequence, or NULL = all N.  du is exactly 0.0 past a sequence's frames; a
 * sequence with n_frames[b] == 0 is not read at all (neither L nor z): the way to skip a sequence for which cpe_covariance found no factor.  The
 * reciprocals of the diagonal are formed as the covariance sweep forms them (r = 1 / d).  Every sum has a fixed order (no atomics): results are
 * reproducible bit for bit, and the result of a sample depends neither on S, nor on its slot s, nor on the batch.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): S < 1; negative sizes or more than 2^31 - 1 sample frames
 * (B N S); a frame count outside [0, N]; a NULL argument other than n_frames; a half-bandwidth above 4. */
cpe_status cpe_band_sample(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames /*[B] host, or NULL*/, const double* L, int32_t S,
                           const double* z, double* du);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_band_sample_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, const double* L, int32_t S, const double* z, double* du);
/* cpe_posterior_samples: the poses of S draws.  Device pointers except model and n_frames.  q [B][N][nq]: the estimate, Euler angles as
 * cpe_covariance takes them; du [B][S][N][28]: cpe_band_sample's output (or any step in the reduced coordinates).  Sample s of sequence b is the
 * cold-start state of q (leg angles about the body's y axis, as every solve starts) with du added to the entries of the reduced coordinates --
 * exactly the update with which an LM step writes its trial iterate -- made consistent with the joint equalities and turned into Euler angles and
 * marker positions by the code of the solve's own outputs: q_s [B][S][N][nq] (required) satisfies the joint equalities as cpe_solve's q does, and
 * positions_s [B][S][N][L][3] (may be NULL) are its marker positions.  Angle bounds are not enforced (they are not part of the Laplace
 * approximation, see cpe_covariance).  All samples with du == 0 of a sequence come back with the same bits.
 * model, n_frames [B] HOST: both NULL, or both given = sequences of their own length and model in cpe_covariance_ragged's layout (N = N_max) on a
 * handle of cpe_create_multi; everything past a sequence's frames is then 0.0, and a sequence's samples are bit-equal to those of its own plain call.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): S < 1; negative sizes or more than 2^31 - 1 sample frames;
 * model without n_frames or the reverse; NULL h, q, du or q_s; a model index or frame count out of range. */
cpe_status cpe_posterior_samples(cpe_handle* h, int32_t B, int32_t N, const int32_t* model /*[B] host, or NULL*/, const int32_t* n_frames /*[B] host, or NULL*/,
                                 const double* q, int32_t S, const double* du, double* q_s, double* positions_s);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_posterior_samples_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, int32_t S,
                                      const double* du, double* q_s, double* positions_s);

/* ---- segment lengths as unknowns of the kinematic estimate ("What is calibrated").  One scale s_g per segment group, G groups,
 * multiplies the lengths of the group's links; marker positions are linear in the scales.  With J(s, u) the objective of cpe_solve,
 * cpe_scale_system returns, per sequence, the Gauss-Newton system of the scales with the poses eliminated (variable projection):
 *     A = d2 J / ds ds,   b = d J / ds,   E = d2 J / du ds     (the measurement terms: only they depend on the lengths; loss gradient weight and
 *                                                               PSD curvature weight of opts.curvature, as in the solve's own normal equations)
 *     A_red = A - E^T (H + ridge D)^-1 E,     b_red = b - E^T (H + ridge D)^-1 g
 * with H, D, g the matrix, damping diagonal and gradient of cpe_covariance: it runs that entry's first pass at Euler q [B][N][nq] to the factor
 * L L^T = H + ridge D, then Y = L^-1 [E | g] by forward substitution, A_red = A - Y^T Y and b_red = b - Y^T L^-1 g.  The Newton step of the
 * scales at re-adapted poses is -A_red^-1 b_red, and A_red^-1 is the covariance of the scales.
 * Device pointers: q, meas, weight (as cpe_covariance takes them) and the outputs A, A_red [B][G][G], b, b_red [B][G], cost [B] = the measurement
 * cost at q.  HOST: d_attach [M][G][n_links][3] and d_marker_off [M][G][n_markers][3], the derivatives of cpe_skeleton's `attach` and `marker_off`
 * by every scale for each of the handle's M models (1 for cpe_create); model, n_frames [B], both NULL or both given (cpe_covariance_ragged's
 * layout); status [B]: CPE_OK, or CPE_NUMERICAL where the matrix has no factor -- that sequence's outputs are all 0.0.  A and A_red are exactly
 * symmetric, a group no marker depends on has exactly zero rows and columns, every sum has a fixed order (no atomics): results are reproducible
 * bit for bit and a sequence's do not depend on the batch.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): G outside 1..CPE_MAX_SCALES; a negative or non-finite
 * ridge; negative sizes; model without n_frames or the reverse; a frame count outside 1..N; a NULL argument other than model and n_frames; a
 * half-bandwidth above 4; a model index out of range. */
#define CPE_MAX_SCALES 16
cpe_status cpe_scale_system(cpe_handle* h, int32_t B, int32_t N, const int32_t* model /*[B] host, or NULL*/, const int32_t* n_frames /*[B] host, or NULL*/,
                            const double* q, const double* meas, const double* weight, double ridge, int32_t G, const double* d_attach /*host*/,
                            const double* d_marker_off /*host*/, double* A, double* b, double* A_red, double* b_red, double* cost, cpe_status* status);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_scale_system_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, const double* meas,
                                 const double* weight, double ridge, int32_t G, const double* d_attach, const double* d_marker_off, double* A,
                                 double* b, double* A_red, double* b_red, double* cost, cpe_status* status);

/* ---- the pose covariance marginalised over the fitted scales ("What is marginalised").  cpe_covariance is the covariance of the
 * poses GIVEN the lengths.  Over (u, s) the joint Gauss-Newton matrix of one animal is a block arrow -- pose blocks H + ridge D, borders E, corner
 * sum A + P with P the prior precision of the scales -- and its inverse is, exactly,
 *     cov_s = (sum_b A_red,b + P)^-1     R_b = du_b / ds = -(H_b + ridge D_b)^-1 E_b     cov(u_b) = Sigma_b + R_b cov_s R_b^T     cov(u_b, s) = R_b cov_s
 * and, a marker position depending on the scales directly (Ds_l = d p_l / d s) and through the poses (P_l = d p_l / d u),
 *     W_l = Ds_l + P_l R_n     cov(p_l) = P_l Sigma(n,n) P_l^T + W_l cov_s W_l^T.
 * cpe_scale_response: arguments, statuses and refusals of cpe_scale_system.  A_red [B][G][G] is bit-equal to that entry's; resp_u [B][N][28][G] = R,
 * the response of the re-adapted poses to the scales; resp_pos [B][N][L][3][G] = W, how far a marker moves per unit of a scale once the poses have
 * re-adapted (may be NULL).  Layouts, ragged included, as cpe_covariance_ragged's cov_pos; everything is 0.0 past a sequence's frames and for a
 * sequence without a factor (CPE_NUMERICAL in status[b]).  It runs cpe_scale_system's launches, keeps Y_E = L^-1 E, solves L^T X = -Y_E for the G
 * columns (cpe_band_sample's kernel) and forms W per frame.  The named deviations of cpe_covariance and cpe_scale_system carry over. */
cpe_status cpe_scale_response(cpe_handle* h, int32_t B, int32_t N, const int32_t* model /*[B] host, or NULL*/, const int32_t* n_frames /*[B] host, or NULL*/,
                              const double* q, const double* meas, const double* weight, double ridge, int32_t G, const double* d_attach /*host*/,
                              const double* d_marker_off /*host*/, double* A_red, double* resp_u, double* resp_pos, cpe_status* status);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_scale_response_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* model, const int32_t* n_frames, const double* q, const double* meas,
                                   const double* weight, double ridge, int32_t G, const double* d_attach, const double* d_marker_off, double* A_red,
                                   double* resp_u, double* resp_pos, cpe_status* status);
/* cpe_covariance_add_scales: the band of cov(u) and the marker covariances with the scale terms added, blocks in cpe_band_inverse's layout:
 *     cov_diag_m[n] = cov_diag[n] + R_n cov_s R_n^T     cov_off_m[n][i-1] = cov_off[n][i-1] + R_{n+i} cov_s R_n^T     cov_pos_m[n][l] = cov_pos[n][l] + W_l cov_s W_l^T
 * Device pointers: cov_s [B][G][G] (only its lower triangle is read), resp_u, resp_pos (cpe_scale_response's), cov_diag, cov_off, cov_pos (a covariance
 * entry's) and the outputs, which must not overlap the inputs.  n_frames [B] HOST, or NULL = all N.  cov_pos, resp_pos and cov_pos_m are NULL together
 * or given together.  cov_diag_m and cov_pos_m are exactly symmetric; the outputs are 0.0 past a sequence's frames and where n + i is past them; a
 * sequence of 0 frames is not read.  Every sum runs over the scales in ascending order (no atomics) and a result depends on its own sequence alone.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): G outside 1..CPE_MAX_SCALES; negative sizes; a frame count
 * outside 0..N; a NULL argument other than those named; a half-bandwidth above 4. */
cpe_status cpe_covariance_add_scales(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames /*[B] host, or NULL*/, int32_t G, const double* cov_s,
                                     const double* resp_u, const double* resp_pos, const double* cov_diag, const double* cov_off, const double* cov_pos,
                                     double* cov_diag_m, double* cov_off_m, double* cov_pos_m);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_covariance_add_scales_host(cpe_handle* h, int32_t B, int32_t N, const int32_t* n_frames, int32_t G, const double* cov_s, const double* resp_u,
                                          const double* resp_pos, const double* cov_diag, const double* cov_off, const double* cov_pos, double* cov_diag_m,
                                          double* cov_off_m, double* cov_pos_m);

/* ---- posterior covariance of the physics-based estimate: coordinates, and the node forces (torques, joint constraint forces, net foot forces)
 * the solve infers ("What is inverted").  Runs the launches of the first pass of cpe_solve_kinetic at Euler q -- cold start, multipliers
 * zero, node forces minimised from a cold start, as cpe_eval_kinetic_system / cpe_eval_lm_step -- at damping `ridge` in place of opts.lambda0, up to
 * and including the band factor (no back substitution, no trial iterate).  Then
 *     Sigma = (H + ridge D)^-1      on its block band (pb = 3),
 * H = the reduced band of that pass (the Schur complement of the joint Gauss-Newton matrix over coordinates and node forces), D its Marquardt diagonal
 * with cpe_eval_lm_step's floors; and, because the band is that Schur complement, the Laplace covariance of the forces of node n is local and exact:
 *     cov_f(n) = M_n^-1 + S_n W_n S_n^T,   S_n = M_n^-1 H_fu(n),
 * W_n = the 84 x 84 covariance of the coordinates of the frames (n, n-1, n-2), all of it inside the band, M_n = the node's force matrix as the pass
 * eliminated it.  At ridge = 0 M_n is the plain H_ff of cpe_eval_kinetic_nodes.  At ridge > 0 the forces are eliminated at that damping too
 * (k_dyn_schur reads the sequence's lambda): M_n = H_ff + ridge lm_force_damping diag H_ff + the wall term ridge lm_wall_damping 2 w_slack c c^T / gap^2
 * of every inactive force inequality of a stance foot.
 * Named deviations: those of cpe_covariance (scale, bounds / multipliers zero, robust-loss curvature, reduced coordinates); a force whose inequality
 * row is active at the cold-start minimiser carries that row's penalty curvature in H_ff; a prescribed (grf_fixed) or absent (swing foot) force is not
 * an unknown and has no entry.
 * Device pointers except status.  grf_fixed / tau_box / grf_box: at most one non-NULL, as cpe_eval_kinetic_system.  cov_diag, cov_off, cov_pos, L,
 * status as cpe_covariance (cov_diag and cov_off are bit-equal to cpe_band_inverse of L).  cov_f [B][N][64][64]: the covariance of node n's free forces
 * in the compact order of meta[n] -- the row order of Hff in cpe_eval_kinetic_nodes -- exactly symmetric, zero past the count and for the nodes 0, 1.
 * f [B][N][64] and meta int32 [B][N][65] = (count na, the na indices into f's layout tau | lambda | (z, x, y) per foot, zeros, Newton iterations of the
 * node's force solve in the last word): those of the evaluation.  cov_off, cov_pos, cov_f, f, meta, L may be NULL.
 * status[b] is CPE_NUMERICAL, and every output of that sequence zero, where the evaluation is not finite or the band or any node's M_n has no Cholesky
 * factor; the damping is never raised silently.  Results are reproducible bit for bit (no atomics), and a sequence's outputs do not depend on its batch.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): ridge < 0 or not finite; a handle whose half-bandwidth is not 3
 * (motion-prior windows above 3); NULL opt or stance; more than one of grf_fixed, tau_box, grf_box.  Not built: the 3D kinematic cost (cpe_solve_kinetic_tracked*),
 * the shutter displacement. */
cpe_status cpe_covariance_kinetic(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                  const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                                  double ridge, double* cov_diag, double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L,
                                  cpe_status* status);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_covariance_kinetic_host(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                       const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box,
                                       const double* grf_box, double ridge, double* cov_diag, double* cov_off, double* cov_pos, double* cov_f, double* f,
                                       int32_t* meta, double* L, cpe_status* status);
/* The same for sequences of their own length, rig and model, in cpe_solve_kinetic_ragged's layout: a handle of cpe_create_multi, opts [n_models] (one
 * cpe_kinetic_options per model of the handle), model [B] and n_frames [B] HOST arrays, every per-frame array padded to N_max frames (meas / weight
 * to C_max cameras as well).  For every sequence b the rows [0, n_frames[b]) of cov_diag, cov_off, cov_pos, cov_f, f, meta and L, and status[b], are
 * bit-equal to cpe_covariance_kinetic of that sequence alone (B = 1, N = n_frames[b]) on a plain handle of its own model; rows past a sequence's
 * length read 0.  status[b] is CPE_NUMERICAL, and every output of that sequence zero (what the band kernels had written included), where its
 * evaluation is not finite or its band or one of its nodes' M_n has no Cholesky factor; such a sequence does not disturb a neighbour's bits.  Returns
 * the worst status.  cov_off == NULL works as in the plain entry.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): what cpe_covariance_kinetic refuses; NULL model or n_frames;
 * a model index or frame count out of range; kinetic options of a model that differ from model 0's in a field that fixes the layout of the node
 * forces (dyn.n_feet, dyn.foot_marker, dyn.n_motors, dyn.motor_first / _second / _axis: the field is named). */
cpe_status cpe_covariance_kinetic_ragged(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model /*[B] host*/,
                                         const int32_t* n_frames /*[B] host*/, const double* q, const double* meas, const double* weight,
                                         const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge,
                                         double* cov_diag, double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L,
                                         cpe_status* status);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_covariance_kinetic_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model,
                                              const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                              const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, double* cov_diag,
                                              double* cov_off, double* cov_pos, double* cov_f, double* f, int32_t* meta, double* L, cpe_status* status);

/* ---- draws of the node forces of the physics-based estimate ("What is sampled (forces)"): whole trajectories of torques, joint
 * constraint forces and net foot forces JOINTLY with the coordinates, for the error bar of any quantity computed from them -- the impulse of a stance,
 * a peak force and its frame, joint power and work, a duty factor from a force threshold -- which need the covariance between the forces of different
 * frames and between forces and coordinates, not only cov_f(n).  The band cpe_covariance_kinetic factors (A = L L^T) is the Schur complement of the
 * joint Gauss-Newton matrix over (coordinates, node forces).  Ordered as (forces of every node, coordinates) that joint matrix has the lower factor
 *     G = [[ blockdiag(C_n), 0 ], [ H_uf C_n^-T, L ]],        M_n = C_n C_n^T  (the node's force matrix as eliminated),
 * so G^T (df, du) = (zeta, z) with z, zeta ~ N(0, I) is a draw of the joint Laplace posterior:
 *     L^T du = z                                        (cpe_band_sample on the L cpe_covariance_kinetic returns)
 *     df_n = C_n^-T (zeta_n - Y_n w_n),   Y_n = C_n^-1 H_fu(n),   w_n = (du_n, du_{n-1}, du_{n-2}),   n >= 2      (this entry)
 * with cov(df_n) = M_n^-1 + S_n W_n S_n^T = cov_f(n) exactly, cov(df_n, du) = -S_n Sigma(w_n, .), and for n != m cov(df_n, df_m) =
 * S_n Sigma(w_n, w_m) S_m^T -- blocks of Sigma at any distance, which only sampling reaches without a dense inverse.
 * The entry is stateless: it runs the first pass of cpe_covariance_kinetic itself (cold start at Euler q, multipliers zero, damping `ridge`, up to and
 * including the band factor), then one kernel over the nodes.  That pass is deterministic: f, meta and status[b] are bit-equal to
 * cpe_covariance_kinetic's for the same inputs, and M_n is the matrix behind its cov_f.
 * Device pointers except status.  q, meas, weight, stance, grf_fixed / tau_box / grf_box, ridge: as cpe_covariance_kinetic.  du [B][S][N][28]:
 * cpe_band_sample's output, or any step in the reduced coordinates.  zeta [B][S][N][64]: standard normals in the compact order of meta[n]; entries past
 * the node's count are not read; NULL = zeros, which gives the conditional mean f - S_n w_n.  f_s [B][S][N][64], f's layout tau | lambda | (z, x, y)
 * per foot: f + df on the node's unknowns; a force that is no unknown of the node keeps f's value; the nodes 0, 1 and the frames past a sequence's
 * own are exactly 0.0.  f [B][N][64], meta int32 [B][N][65]: as cpe_covariance_kinetic, may be NULL.  status [B], HOST: CPE_NUMERICAL under
 * cpe_covariance_kinetic's conditions (the evaluation is not finite, or the band or a node's M_n has no Cholesky factor) -- all outputs of that
 * sequence are zero.  Returns the worst status.  Every sum has a fixed order (no atomics): a sample's forces are bit-equal whatever S, its slot s and
 * the batch.
 * Named deviations -- a draw is NOT: (linear) re-minimised: the forces are the linearisation about the evaluation, not the minimiser at the sampled
 * pose; (inequalities) feasible: the friction polyhedron, Fz >= 0.01 and the torque / force boxes are not enforced, a row active at the evaluation
 * contributes its penalty curvature, an inactive one nothing; (centre) centred on anything but the evaluation's f -- the cold-start evaluation at q
 * with multipliers zero, not a converged solve's forces; (ridge) as wide as the posterior at ridge > 0: M_n and the band are both damped, the draws
 * are narrower; plus those of cpe_covariance_kinetic.
 * Refused with CPE_BAD_ARG before the device is touched, the reason in cpe_last_error(): what cpe_covariance_kinetic refuses; S < 1; negative sizes
 * or more than 2^31 - 1 sample frames (B N S); NULL du or f_s. */
cpe_status cpe_force_samples(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                             const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                             double ridge, int32_t S, const double* du, const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_force_samples_host(cpe_handle* h, const cpe_kinetic_options* opt, int32_t B, int32_t N, const double* q, const double* meas,
                                  const double* weight, const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box,
                                  double ridge, int32_t S, const double* du, const double* zeta, double* f_s, double* f, int32_t* meta,
                                  cpe_status* status);
/* The same for sequences of their own length, rig and model, in cpe_covariance_kinetic_ragged's layout (du, zeta, f_s padded to N_max frames): every
 * sequence's rows are bit-equal to its own plain call, rows past its length read 0, and a sequence that is CPE_NUMERICAL does not disturb a
 * neighbour's bits.  Also refused: what cpe_covariance_kinetic_ragged refuses. */
cpe_status cpe_force_samples_ragged(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model /*[B] host*/,
                                    const int32_t* n_frames /*[B] host*/, const double* q, const double* meas, const double* weight,
                                    const int32_t* stance, const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge,
                                    int32_t S, const double* du, const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_force_samples_ragged_host(cpe_handle* h, const cpe_kinetic_options* opts, int32_t B, int32_t N_max, const int32_t* model,
                                         const int32_t* n_frames, const double* q, const double* meas, const double* weight, const int32_t* stance,
                                         const double* grf_fixed, const double* tau_box, const double* grf_box, double ridge, int32_t S,
                                         const double* du, const double* zeta, double* f_s, double* f, int32_t* meta, cpe_status* status);

/* forward kinematics only (get_pose_state / get_com, acinoset_misc.py:1581-1659, :722-742); device ptrs */
cpe_status cpe_forward_kinematics(cpe_handle* h, int32_t B, int32_t N, const double* q,
                                  double* positions /*[B][N][L][3]*/, double* com /*[B][N][3] or NULL*/);

/* marker velocities v_l = (d p_l / d q) dq (the lambdified `foot.Pb_I_vel` of the contact heuristic, acinoset_misc.py:347-360,
 * for every marker); device ptrs */
cpe_status cpe_marker_velocities(cpe_handle* h, int32_t B, int32_t N, const double* q, const double* dq,
                                 double* velocities /*[B][N][L][3]*/);

/* reprojection of 3D marker positions into every camera of the handle, for the cam*_fte.{h5,csv} writers
 * (acinoset_misc.py:1339-1407: cv.fisheye.projectPoints / pt3d_to_2d per camera); device ptrs */
cpe_status cpe_reproject(cpe_handle* h, int32_t B, int32_t N, const double* positions /*[B][N][L][3]*/,
                         double* uv /*[B][N][C][L][2]*/);

/* The detection report ("What is predicted in the image"): where in every camera's image every marker is, give or take how many
 * pixels, and -- with detections -- how far each detection is from what everything else predicts for it.  Per frame, camera c, marker l, with p
 * the marker's position, Sigma_p its 3 x 3 block of cpe_covariance's cov_pos, z the detection, w = cam[c].mult * weight (the solver's scale of the
 * residual) and w_f = cam[c].mult * weight_fit (the weight the detection had in the fit whose covariance Sigma_p is; weight_fit NULL = weight, 0 =
 * held out):
 *   uv, G       the projection and its 2 x 3 derivative by p; uv is bit-equal to cpe_reproject's
 *   cov_px      S = G Sigma_p G^T as (xx, xy, yy): the covariance of the predicted pixel, exact to first order
 *   l_d         the loss at w_f (uv_d - z_d), d = 0, 1 (the handle's knots and curvature mode); g_d = l_d' w_f and W = diag(kappa_d w_f^2) are the
 *               gradient and curvature terms this detection put into H;  a_d = sqrt(W_dd);  T = I - diag(a) S diag(a)
 *   leverage    W_00 S_00 + W_11 S_11 = tr(W S), the detection's share of the hat matrix's trace
 *   cov_loo     S_loo = S + S diag(a) T^-1 diag(a) S  (= S (I - W S)^-1, stored symmetric as (xx, xy, yy)): the detection taken out of the fit
 *   uv_loo      uv + S_loo g: one Gauss-Newton step about the estimate, exact for a quadratic objective
 *   d2          r^T (S_loo + sigma2 I)^-1 r with r = z - uv_loo and sigma2 = 1 / (w^2 kappa0), kappa0 the loss's curvature at its centre: chi-square
 *               with 2 degrees of freedom where the model holds
 * Where the smaller eigenvalue of T is not finite or not above 1e-9 the detection alone determines a direction: uv_loo, cov_loo and d2 are NaN,
 * leverage is still written.  w == 0 (no detection): uv_loo = uv and cov_loo = cov_px bit for bit, leverage 0, d2 NaN.  w_f == 0 < w (held out):
 * W = 0 and g = 0, so uv_loo = uv, cov_loo = cov_px and d2 = r^T (S + sigma2 I)^-1 r.  A redescended outlier has W = 0 too: it is out of the fit
 * already.  With a ridge in cov_pos the report is that of the damped posterior; multipliers are zero as in cpe_covariance.
 * Device pointers, enqueued on the handle's stream; no workspace, no atomics: reproducible bit for bit, and a sequence's outputs do not depend on
 * the batch it is in.  meas and weight come together or not at all; without them the call is the pixel-ellipse part alone and the four outputs
 * after cov_px must be NULL; with them each of the four may be NULL.  CPE_BAD_ARG with the argument named in cpe_last_error(), before the device is
 * touched: negative sizes; meas without weight or weight without meas; weight_fit without weight; uv_loo, cov_loo, d2 or leverage without
 * measurements; null positions, cov_pos, uv or cov_px (B N > 0); a null handle.  B = 0 or N = 0 returns CPE_OK and touches nothing. */
cpe_status cpe_detection_report(cpe_handle* h, int32_t B, int32_t N, const double* positions /*[B][N][L][3]*/, const double* cov_pos /*[B][N][L][3][3]*/,
                                const double* meas /*[B][N][C][L][2] or NULL*/, const double* weight /*[B][N][C][L] or NULL*/,
                                const double* weight_fit /*[B][N][C][L] or NULL = weight*/, double* uv /*[B][N][C][L][2]*/,
                                double* cov_px /*[B][N][C][L][3]*/, double* uv_loo /*[B][N][C][L][2]*/, double* cov_loo /*[B][N][C][L][3]*/,
                                double* d2 /*[B][N][C][L]*/, double* leverage /*[B][N][C][L]*/);
/* host-pointer twin (stages through HBM) */
cpe_status cpe_detection_report_host(cpe_handle* h, int32_t B, int32_t N, const double* positions, const double* cov_pos, const double* meas,
                                     const double* weight, const double* weight_fit, double* uv, double* cov_px, double* uv_loo, double* cov_loo,
                                     double* d2, double* leverage);

/* initial-guess ingestion: two-view linear triangulation of n detection pairs, i.e. triangulate_points[_fisheye]
 * (acinoset_misc.py:1432-1453: cv[.fisheye].undistortPoints of both pixels with the cameras' K and D, cv.triangulatePoints with
 * [R | t]).  cam_a / cam_b index the handle's cameras; cam_b[i] < 0 asks for the monocular rule instead: the first detection
 * back-projected to `depth` metres along its ray.  Device ptrs: cam_a, cam_b int32[n]; uv_a, uv_b [n][2]; xyz [n][3]. */
cpe_status cpe_triangulate(cpe_handle* h, int32_t n, const int32_t* cam_a, const int32_t* cam_b, const double* uv_a, const double* uv_b,
                           double depth, double* xyz);

/* measurement ingestion: the DeepLabCut table of ONE camera -> that camera's slice `slot` of meas [N][n_slots][L][2]
 * and weight [N][n_slots][L], as init_measurements / init_meas_weights fill the Pyomo params (acinoset_misc.py:211-256): frame n
 * reads table row first_row + n (first_row = start_frame - sync_offset of the camera), marker l reads body part part_of_marker[l];
 * weight = inv_sigma[l] if likelihood > thresh else 0.  Rows outside the table and non-finite coordinates give meas 0, weight 0.
 * table [rows][3*parts] = (x, y, likelihood) per body part; L is the handle's marker count.  Device ptrs. */
cpe_status cpe_tensorise_dlc(cpe_handle* h, int32_t N, int32_t n_slots, int32_t slot, const double* table, int32_t rows, int32_t parts,
                             int32_t first_row, const int32_t* part_of_marker, const double* inv_sigma, double thresh, double* meas, double* weight);

#ifdef __cplusplus
}
#endif
#endif /* CPE_H */
