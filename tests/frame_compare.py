"""Entry-by-entry comparison of cpe_eval_normal's outputs (k_frame_normal: g [28], Bm [28, 28], cost [3], q_out [nq] of every frame) with an
extended-precision reference that shares no derivative code with the oracle.  Helper of the tests, not a test module.

The reference (evaluate(), dtype np.longdouble).  Reduced coordinates u [28] of a frame from the oracle's consistent q (oracle.move_coordinate by
0.0: used only to make q consistent): the independent Euler dofs of the trunk and, in every leg's pitch slot, alpha = the angle of R_B^T R_c about y.
Pixels as a function of u: synth.legs_from_alpha + synth.project_dependents_numpy_hooke (q_of_u), synth.fk_numpy, synth.project_numpy.
J_u = d pixel / d u [C, L, 2, 28] by five-point central differences at h = 1e-3 and h / 2, extrapolated (16 D(h / 2) - D(h)) / 15.  The loss
rho, rho', rho'' and the curvature weight cw of both modes (include/cpe.h: mode 0 max(rho'', rho'(|s|) / |s|, 0), mode 1 max(rho'', 0)), the
bound penalty on the cost view (a leg's pitch is theta_B + alpha, so every bound is linear in u with the constant rows of cost_rows()) with
multipliers zero, and the Gaussian-mixture pose prior -log(sum_k w_k N(x; mu_k, Sigma_k) + 1e-12) on x = X u (synth.tracked_x_jacobian) with the
solver's curvature sum_k gamma_k P_k.

discrepancies(G, R): one number per key, the worst over the frames and entries of |HIP - reference| / scale; inf for any non-finite HIP value;
where a scale is exactly zero the compared value must be exactly zero:

  cost       the three cost terms           scale: the reference's own |value|
  g          reduced gradient               scale per entry: sum_i |rho'_i w_i J_u,ia| + the absolute bound and prior contributions (+ floor, below)
  Bm         Gauss-Newton block             scale sqrt(Bm_aa Bm_bb) of the reference (+ floor, below)
  sym        Bm - Bm^T                      Bm's scale, frames with an active bound or the prior (their terms are added to finished entries one by
                                            one: the global atomics of two bounds that meet in one entry may arrive in either order, the prior's
                                            constant matrices X^T P_k X come from the host as they are)
  sym_exact  Bm - Bm^T                      all other frames: 0 or inf (the gather of k_frame_normal stores every entry and its mirror from one
                                            register)
  q_out      consistent Euler q             absolute (rad, m), against the oracle's consistent q

The floor of the scales of g and Bm.  Beyond the last knot rho' and cw are differences of logistic switches that agree to within
exp(c - |s|), formed from terms of the size of a |s|: 1 - s_a, s_a - s_b, ... round at 1e-16 of the terms they stand between.  For |s| - c
between about 20 and 44 rho' lies between 1e-9 and 1e-19: np.longdouble still resolves it, double precision returns rounding noise or 0
(further out both give exactly 0).  A coordinate that only such residuals reach -- one paw marker, an outlier in every camera -- then has a
scale of 1e-15 by the rule above, against which no double-precision evaluation of the loss can be compared.  So FLOOR = 2^-10 of the same
sums with every term of rho' and rho'' taken absolutely (loss(): the switches' differences expanded) is added to both scales:
sum_i FLOOR |rho'|_abs,i |w_i J_u,ia| to g's, FLOOR sum_i cw_abs,i w_i^2 J_u,ia^2 under Bm's root.  2^-10: a few ulp of rounding of those terms
then read as a few 1e-13, the level of every other entry (measurement 2 with 2^-20: 3.8e-10 on such a coordinate of the loss cases, 1e-13
elsewhere).  On an entry that inliers reach the floor adds about a percent to the scale.

Conditions on the inputs (returned in R["conditions"], asserted by every case; they are not tolerances, they keep the comparison from hiding
a failure): no weighted pair has |z_cam| < resjac_compare.NEAR_Z ("near"; the cases zero such weights: clear_near()), no weighted residual has
|s| < 1e-9 ("small_s": the e > 1e-12 guard of cw), no bound lies within 1e-6 rad of its limit ("bound_margin": the active set is unambiguous),
and every camera holds at least MIN_CAMERA_INLIERS weighted residuals with |s| < loss_c ("camera_inliers", per camera: a camera that holds
only outliers adds nothing to g or Bm and a constant to the cost, so a kernel that misread its parameters would pass).

Tolerances.  TOL[key] = MARGIN (32) x the larger of two numbers measured ON THE CPU over the inputs of every case of
tests/test_gpu_frame_normal.py (case_inputs below); nothing of the kernel's output enters them:

  1  the spread of the float64 evaluation of this same numpy reference under a one-ulp change of every q (np.nextafter, random direction,
     4 draws): ulp_spread()
  2  the distance between that float64 evaluation and the np.longdouble one: extended_distance()

  In the float64 evaluation everything is float64 -- u from q, the pixels at u, residuals, loss, sums, bounds, prior -- except the difference
  quotient, which is formed in np.longdouble from the float64 u and rounded: evaluate(stencil=np.longdouble).  A quotient formed in float64
  measures its own cancellation (1e-13 px of rounding over h = 1e-3 is 1e-10 px / rad on every entry of J_u, 2e-10 to 8e-10 on g and Bm), which
  the kernel, differentiating analytically, does not have; tolerances of 1e-8 would have followed, above the oracle's own distance.

             measurement 1   measurement 2   TOL = 32 x the larger
  cost       1.20e-13        3.37e-14        3.85e-12
  g          3.39e-13        5.41e-13        1.73e-11
  Bm         2.36e-11        2.77e-12        7.56e-10
  q_out      3.55e-15        1.32e-15        1.14e-13

  cost: the narrow pinhole rig, as in resjac_compare.  Bm: 2.4e-11 is case "knots", every other case stays below 5e-13.  With a = 2 the loss
  has rho'(0+) = 0.03 > 0 (the switches do not close at 0), so mode 0's weight rho'(|s|) / |s| grows as 0.03 / |s| towards 0 and a residual of
  |s| ~ 1e-3 carries d cw / d s ~ 3e4: one ulp of q moves s by 6e-14 and that entry of Bm by 2e-11 of its scale.  The kernel shares this.

  (produced by `python -m tests.frame_compare` from the repository root, which prints the table; tests/test_frame_compare.py recomputes both and
  asserts that TOL / (1) lies in [16, 128] and (2) < TOL / 8)

The margin of 32 stands for what legitimately differs between kernel and reference on identical inputs: the device sincos, FMA contraction and
the kernel's summation order, as argued in resjac_compare.py.

The oracle's own distance from the extended reference (oracle.frame_normal, whose Z' = d Euler / d u is a central difference at h = 1e-6), worst
over the same inputs and both curvature modes, for the record:
  cost 1.5e-13, g 3.6e-10, Bm 1.2e-09, sym 3.0e-16 (q_out is the oracle's own): the finite-difference Z' shows in g and Bm, at a thousandth of
  the 2e-6 and a fortieth of the 5e-8 that the comparisons with the oracle allow themselves

The kernel's own worst values on an MI355X over every case of tests/test_gpu_frame_normal.py (its test_zz_report), for the record; they never fed TOL:
  cost 8.3e-14 (one camera), g 5.0e-13 (loss-c0), Bm 2.8e-12 (knots), sym 1.2e-16 (packaged prior, six cameras), sym_exact 0, q_out 8.9e-16
  (plain): each at the level of the two measurements, a factor 30 to 270 inside its tolerance
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resjac_compare as RC                                                         # noqa: E402
from cheetah_pose_estimation_amd import abi, priors, skeleton, synth               # noqa: E402

KEYS = ("cost", "g", "Bm", "sym", "sym_exact", "q_out")
MEASURED_KEYS = ("cost", "g", "Bm", "q_out")
NEAR_Z = RC.NEAR_Z
SMALL_S = 1e-9
BOUND_MARGIN = 1e-6
MIN_CAMERA_INLIERS = 40       # every camera of a case: at least this many weighted residuals with |s| < loss_c (outliers add nothing to g and Bm)
MARGIN = 32.0
FD_H = 1e-3
FLOOR = 2.0 ** -10            # share of the absolute sums of the loss's own terms that is added to the scales of g and Bm (module docstring)

# (measurement 1, measurement 2) per key, in the units above: CPU only, see the module docstring
MEASURED = dict(cost=(1.20e-13, 3.37e-14), g=(3.39e-13, 5.41e-13), Bm=(2.36e-11, 2.77e-12), q_out=(3.55e-15, 1.32e-15))
TOL = {k: MARGIN * max(v) for k, v in MEASURED.items()}
TOL["sym"] = TOL["Bm"]
TOL["sym_exact"] = 0.0


# ---- coordinates -----------------------------------------------------------------------------------------------------------------------
_TABLES = {}


def tables(sk):
    """(independent dofs [28], [(leg link, body link)], slot of every leg's alpha in u, slot of its body's pitch in u)"""
    key = bytes(sk)
    if key not in _TABLES:
        ind = [int(p) for p in skeleton.independent_dofs(sk)]
        lay = synth.leg_layout(sk)
        _TABLES[key] = (ind, lay, [ind.index(3 + 3 * c + 1) for c, _ in lay], [ind.index(3 + 3 * B + 1) for _, B in lay])
    return _TABLES[key]


def u_of_q(sk, q):
    """reduced coordinates u [..., 28] of a consistent Euler q [..., nq], in q's dtype"""
    ind, lay, leg_u, _ = tables(sk)
    u = q[..., ind].copy()
    for r, (c, B) in enumerate(lay):
        M = np.einsum("...ji,...jk->...ik", synth.rot_zyx(q[..., 3 + 3 * B:6 + 3 * B]), synth.rot_zyx(q[..., 3 + 3 * c:6 + 3 * c]))
        u[..., leg_u[r]] = np.arctan2(M[..., 0, 2], M[..., 0, 0])
    return u


def q_of_u(sk, u):
    """consistent Euler q [..., nq] of reduced coordinates u [..., 28], in u's dtype: R_c = R_B Ry(alpha) for the legs, the tails' roll from their
    hooke equality"""
    ind, _, leg_u, _ = tables(sk)
    q = np.zeros(u.shape[:-1] + (sk.nq,), dtype=u.dtype)
    q[..., ind] = u
    q = synth.legs_from_alpha(sk, q, u[..., leg_u])
    with np.errstate(invalid="ignore", divide="ignore"):
        q = synth.project_dependents_numpy_hooke(sk, q)
    assert q.dtype == u.dtype
    return q


def cost_rows(sk):
    """Cv [nq, 28]: row p = d (cost view of Euler angle p) / d u, for the independent p (a leg's pitch is theta_B + alpha); known [nq]"""
    ind, lay, leg_u, body_u = tables(sk)
    Cv = np.zeros((sk.nq, len(ind)))
    known = np.zeros(sk.nq, dtype=bool)
    for k, p in enumerate(ind):
        Cv[p, k] = 1.0
        known[p] = True
    for r, (c, _) in enumerate(lay):
        Cv[3 + 3 * c + 1, body_u[r]] += 1.0
    return Cv, known


def pixels(sk, cams, u):
    """(uv [..., C, L, 2], z_cam [..., C, L]) of reduced coordinates u [..., 28]"""
    pos = synth.fk_numpy(sk, q_of_u(sk, u))[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pr = [synth.project_numpy(cams[c], pos) for c in range(len(cams))]
    return np.stack([p[0] for p in pr], axis=-3), np.stack([p[1] for p in pr], axis=-2)


def pixel_jacobian(sk, cams, u, fd_h=FD_H):
    """J_u [F, C, L, 2, 28] of u [F, 28]: five-point quotients at fd_h and fd_h / 2, extrapolated"""
    dt = u.dtype.type
    F, nu = u.shape
    steps = np.array([k * s for s in (1.0, 0.5) for k in (-2, -1, 1, 2)], dtype=u.dtype) * dt(fd_h)            # [8]
    up = np.broadcast_to(u[:, None, None, :], (F, nu, 8, nu)).copy()
    for k in range(nu):
        up[:, k, :, k] += steps
    return np.moveaxis(stencil_quotient(pixels(sk, cams, up)[0], dt(fd_h)), 1, -1)                               # (f [F, nu, 8, C, L, 2])


def stencil_quotient(f, fd_h):
    """the extrapolated five-point quotient [F, n, ...] of f [F, n, 8, ...], the values at -2, -1, 1, 2 steps of fd_h and then of fd_h / 2"""
    # (differences first: a pixel that does not depend on the coordinate gives exactly 0)
    five = lambda a, hh: (8 * (a[:, :, 2] - a[:, :, 1]) - (a[:, :, 3] - a[:, :, 0])) / (12 * hh)
    return (16 * five(f[:, :, 4:], fd_h / 2) - five(f[:, :, :4], fd_h)) / 15


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def loss(s, a, b, c):
    """(rho, d rho / d s, d2 rho / d s2) of the redescending loss (acinoset_misc.py:2001-2015) in s's dtype: a blend of s^2 / 2, the line
    a |s| - a^2 / 2, the parabola that levels off at |s| = c and the constant K by three logistic switches of unit width at the knots"""
    e = np.abs(s)
    with np.errstate(over="ignore"):
        sg = [1 / (1 + np.exp(t - e)) for t in (a, b, c)]
    s1 = [v * (1 - v) for v in sg]
    s2 = [v * (1 - v) * (1 - 2 * v) for v in sg]
    cb = c - b
    base = a * b - a * a / 2
    pieces = (                                                                       # (value, first, second derivative in e) of every piece
        (e * e / 2, e, np.ones_like(e)),
        (a * e - a * a / 2, a * np.ones_like(e), np.zeros_like(e)),
        (base + (a * cb / 2) * (1 - ((c - e) / cb) ** 2), a * (c - e) / cb, -a / cb * np.ones_like(e)),
        (base + a * cb / 2 + np.zeros_like(e), np.zeros_like(e), np.zeros_like(e)))
    sw = ((1 - sg[0], -s1[0], -s2[0]), (sg[0] - sg[1], s1[0] - s1[1], s2[0] - s2[1]), (sg[1] - sg[2], s1[1] - s1[2], s2[1] - s2[2]),
          (sg[2], s1[2], s2[2]))
    rho = sum(w[0] * p[0] for w, p in zip(sw, pieces))
    d1 = sum(w[1] * p[0] + w[0] * p[1] for w, p in zip(sw, pieces))
    d2 = sum(w[2] * p[0] + 2 * w[1] * p[1] + w[0] * p[2] for w, p in zip(sw, pieces))
    # the same sums with every term taken absolutely, the switches' differences included (1 - s_a as 1 + s_a, ...): what rounds in a
    # double-precision evaluation, used by the floors of the scales of g and Bm only
    one = np.ones_like(e)
    ab = [(one + sg[0], s1[0], np.abs(s2[0])), (sg[0] + sg[1], s1[0] + s1[1], np.abs(s2[0]) + np.abs(s2[1])),
          (sg[1] + sg[2], s1[1] + s1[2], np.abs(s2[1]) + np.abs(s2[2])), (sg[2], s1[2], np.abs(s2[2]))]
    d1a = sum(w[1] * np.abs(p[0]) + w[0] * np.abs(p[1]) for w, p in zip(ab, pieces))
    d2a = sum(w[2] * np.abs(p[0]) + 2 * w[1] * np.abs(p[1]) + w[0] * np.abs(p[2]) for w, p in zip(ab, pieces))
    return rho, d1 * np.sign(s), d2, d1a, d2a


def curvature_weight(s, d1, d2, mode):
    """include/cpe.h: mode 0 max(rho'', rho'(|s|) / |s|, 0), mode 1 max(rho'', 0)"""
    cw = np.maximum(d2, 0)
    if mode == 0:
        e = np.abs(s)
        with np.errstate(invalid="ignore", divide="ignore"):
            cw = np.maximum(cw, np.where(e > 0, d1 * np.sign(s) / np.where(e > 0, e, 1), 0))
    return cw


# ---- the reference of a batch of frames ----------------------------------------------------------------------------------------------------
def _prior_arrays(pr, dt):
    K, D = pr.gmm_k, pr.gmm_dim
    P = np.array([[[pr.gmm_P[k][i][j] for j in range(D)] for i in range(D)] for k in range(K)], dtype=dt)
    mu = np.array([[pr.gmm_mu[k][i] for i in range(D)] for k in range(K)], dtype=dt)
    return P, mu, np.array(pr.gmm_logw[:K], dtype=dt)


def evaluate(sk, cams, opts, pr, qc, meas, weight, dtype=np.longdouble, fd_h=FD_H, stencil=None, view=None):
    """one frame's terms of F frames at consistent Euler qc [F, nq] (meas [F, C, L, 2], weight [F, C, L]), everything in `dtype`: dict(cost [F, 3],
    g, g_scale [F, 28], Bm [F, 28, 28], q [F, nq] = the numpy map's own consistent q, s [F, C, L, 2] weighted residuals (0 where w = 0), w, z,
    J [F, C, L, 2, 28], v / margin / active of the bounds, g_meas, g_prior).  view: None, or (pixels(u) -> (uv, z), jacobian(u, fd_h) -> [F, C,
    L, 2, >= 28]) of another view of the same frames (shutter_compare's displaced one) in place of pixels() and pixel_jacobian(): the first 28
    columns of its Jacobian are d / d u, all of them come back as Jx beside the loss weights gw, cw w^2 and their absolute forms"""
    dt = np.dtype(dtype).type
    C = len(cams)
    ind, _, _, _ = tables(sk)
    nu = len(ind)
    u = u_of_q(sk, np.asarray(qc).astype(dtype))
    pix, jac = view if view is not None else ((lambda u_: pixels(sk, cams, u_)), (lambda u_, h_: pixel_jacobian(sk, cams, u_, h_)))
    uv, z = pix(u)
    if stencil is None or np.dtype(stencil) == np.dtype(dtype):
        J = jac(u, fd_h)
    else:                                                                            # the stencil alone in another precision, from the same u
        J = jac(u.astype(stencil), fd_h).astype(dtype)
    w = np.array([cams[c].mult for c in range(C)], dtype=dtype)[None, :, None] * np.asarray(weight).astype(dtype)
    on = w != 0
    on2 = on[..., None]
    s = np.where(on2, w[..., None] * (np.where(on2, uv, 0) - np.asarray(meas).astype(dtype)), 0)
    Jx = np.where(on2[..., None], J, 0)
    J = Jx[..., :nu]
    a, b, c = dt(opts.loss_a), dt(opts.loss_b), dt(opts.loss_c)
    rho, d1, d2, d1a, d2a = loss(s, a, b, c)
    cw = np.where(on2, curvature_weight(s, d1, d2, int(opts.curvature)), 0)
    cwa = np.where(on2, curvature_weight(np.abs(s), d1a, d2a, int(opts.curvature)), 0)
    gw = np.where(on2, d1 * w[..., None], 0)
    cost = np.zeros((u.shape[0], 3), dtype=dtype)
    cost[:, 0] = rho.sum(axis=(1, 2, 3))                                             # (s = 0 where w = 0: 2 rho(0) per such pair)
    g_meas = np.einsum("fcld,fclda->fa", gw, J)
    g_scale = np.einsum("fcld,fclda->fa", np.abs(gw), np.abs(J))
    g_floor = np.einsum("fcld,fclda->fa", np.where(on2, d1a * np.abs(w[..., None]), 0), np.abs(J))
    B_floor = np.einsum("fcld,fclda->fa", cwa * w[..., None] ** 2, J * J)
    Bm = np.einsum("fclda,fcldb->fab", J * (cw * w[..., None] ** 2)[..., None], J)
    g = g_meas.copy()
    # angle bounds, multipliers zero: psi = (max(0, kappa (v - up))^2 + max(0, kappa (lo - v))^2) / (2 kappa), v linear in u
    Cv, known = cost_rows(sk)
    nb = sk.n_bounds
    kp = dt(opts.bound_penalty)
    v = np.zeros((u.shape[0], nb), dtype=dtype)
    margin = np.full((u.shape[0], max(nb, 1)), np.inf)
    active = np.zeros((u.shape[0], nb, 2), dtype=bool)
    for i in range(nb):
        ia, ib = sk.bound_a[i], sk.bound_b[i]
        assert known[ia] and (ib < 0 or known[ib]), "a bound on a dependent angle is not linear in u"
        dv = (Cv[ia] - (Cv[ib] if ib >= 0 else 0.0)).astype(dtype)
        v[:, i] = u @ dv
        up_, lo_ = dt(sk.bound_up[i]), dt(sk.bound_lo[i])
        pu, pl = np.maximum(kp * (v[:, i] - up_), 0), np.maximum(kp * (lo_ - v[:, i]), 0)
        margin[:, i] = np.minimum(np.abs(v[:, i] - up_), np.abs(lo_ - v[:, i])).astype(np.float64)
        active[:, i, 0], active[:, i, 1] = pu > 0, pl > 0
        cost[:, 1] += (pu * pu + pl * pl) / (2 * kp)
        g += (pu - pl)[:, None] * dv
        g_scale += (pu + pl)[:, None] * np.abs(dv)
        Bm += (kp * ((pu > 0).astype(dtype) + (pl > 0).astype(dtype)))[:, None, None] * np.outer(dv, dv)
    g_prior = np.zeros_like(g)
    if pr is not None and pr.gmm_k > 0:
        P, mu, logw = _prior_arrays(pr, dtype)
        D = pr.gmm_dim
        X = synth.tracked_x_jacobian(sk)[nu - D:].astype(dtype)                     # [D, 28]
        x = u @ X.T                                                                  # [F, D]
        dx = x[:, None, :] - mu[None]                                                # [F, K, D]
        Pd = np.einsum("kij,fkj->fki", P, dx)
        lp = logw[None] - np.einsum("fki,fki->fk", Pd, dx) / 2
        S = np.exp(lp).sum(axis=1) + dt(1e-12)
        cost[:, 2] = -np.log(S)
        gam = np.exp(lp) / S[:, None]
        g_prior = np.einsum("fk,fki->fi", gam, Pd) @ X
        g += g_prior
        g_scale += np.einsum("fk,fki->fi", gam, np.abs(np.einsum("kij,fkj->fki", np.abs(P), np.abs(dx)))) @ np.abs(X)
        Bm += np.einsum("ia,fij,jb->fab", X, np.einsum("fk,kij->fij", gam, P), X)
    return dict(cost=cost, g=g, g_scale=g_scale, Bm=Bm, q=q_of_u(sk, u), s=s, w=w, z=z, J=J, v=v, margin=margin, active=active,
                g_meas=g_meas, g_prior=g_prior, g_floor=g_floor, B_floor=B_floor, has_prior=pr is not None and pr.gmm_k > 0,
                u=u, uv=uv, Jx=Jx, gw=gw, gwa=np.where(on2, d1a * np.abs(w[..., None]), 0), cww=cw * w[..., None] ** 2, cwwa=cwa * w[..., None] ** 2)


def consistent_q(oracle, sk, q):
    """the oracle's consistent q of Euler q [F, nq] (the coordinate map alone: a coordinate moved by 0.0)"""
    return np.stack([oracle.move_coordinate(sk, q[f:f + 1], 0, 0, 0.0)[0] for f in range(q.shape[0])])


def make_reference(E, qc, opts):
    """the comparator's form of evaluate()'s result E; qc = the oracle's consistent q"""
    for k in ("cost", "g", "Bm"):
        if not np.all(np.isfinite(E[k])):
            raise ValueError("the reference itself is not finite: no case may be built on such inputs")
    diag = np.sqrt(np.einsum("faa->fa", E["Bm"]) + FLOOR * E["B_floor"])
    on = E["w"] != 0
    e = np.abs(E["s"][on]).astype(np.float64).ravel()                                # the weighted residuals, both coordinates
    knots = (0.0, opts.loss_a, opts.loss_b, opts.loss_c, np.inf)
    cond = dict(near=int((on & (np.abs(E["z"]) < NEAR_Z)).sum()), small_s=int((e < SMALL_S).sum()),
                bound_margin=float(E["margin"].min()), weighted=int(on.sum()),
                camera_inliers=tuple(int(v) for v in ((np.abs(E["s"]).astype(np.float64) < opts.loss_c) & on[..., None]).sum(axis=(0, 2, 3))),
                pieces=tuple(float(((e >= lo) & (e < hi)).mean()) if e.size else 0.0 for lo, hi in zip(knots[:-1], knots[1:])))
    exact = ~(E["active"].any(axis=(1, 2)) | E["has_prior"])
    return dict(E, q_out=np.asarray(qc), g_scale=E["g_scale"] + FLOOR * E["g_floor"], Bm_scale=diag[:, :, None] * diag[:, None, :], sym_exact=exact, conditions=cond)


def reference(oracle, sk, cams, opts, pr, q, meas, weight, dtype=np.longdouble):
    """the reference of F frames q [F, nq] (any Euler q; the kernel makes it consistent as the oracle does), meas [F, C, L, 2], weight [F, C, L]"""
    qc = consistent_q(oracle, sk, np.ascontiguousarray(q, dtype=np.float64))
    return make_reference(evaluate(sk, cams, opts, pr, qc, meas, weight, dtype), qc, opts)


def conditions_hold(R):
    c = R["conditions"]
    return c["near"] == 0 and c["small_s"] == 0 and c["bound_margin"] >= BOUND_MARGIN and min(c["camera_inliers"]) >= MIN_CAMERA_INLIERS


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def _ratio(G, Rv, scale):
    """worst |G - R| / scale; inf where G is not finite, or where the scale is zero and G != R"""
    G = np.asarray(G)
    if not np.all(np.isfinite(G)):
        return float("inf")
    d = np.abs(G - Rv)
    scale = np.broadcast_to(scale, d.shape)
    zero = scale == 0
    if np.any(d[zero] != 0):
        return float("inf")
    return float((d[~zero] / scale[~zero]).max(initial=0.0))


def discrepancies(G, R):
    """worst value of every key over the frames of R: G = dict(g [F, 28], Bm [F, 28, 28], cost [F, 3], q_out [F, nq] or None) of HIP"""
    out = dict(cost=_ratio(G["cost"], R["cost"], np.abs(R["cost"])), g=_ratio(G["g"], R["g"], R["g_scale"]),
               Bm=_ratio(G["Bm"], R["Bm"], R["Bm_scale"]))
    Bm = np.asarray(G["Bm"])
    asym = Bm - np.swapaxes(Bm, 1, 2)
    ex = R["sym_exact"]
    out["sym"] = _ratio(asym[~ex], 0.0, R["Bm_scale"][~ex])
    out["sym_exact"] = 0.0 if np.all(np.isfinite(Bm[ex])) and not np.any(asym[ex] != 0.0) else float("inf")
    if G.get("q_out") is not None:
        out["q_out"] = _ratio(G["q_out"], R["q_out"], 1.0)
    return out


def relative_difference(a, b, scale):
    """largest |a - b| / scale over the entries whose scale is not zero"""
    d, scale = np.abs(np.asarray(a) - np.asarray(b)), np.asarray(scale)
    return float((d[scale != 0] / scale[scale != 0]).max(initial=0.0))


def failures(d, tol=None):
    """the keys of a discrepancy dict beyond their tolerance"""
    tol = tol or TOL
    return {k: d[k] for k in KEYS if k in d and not d[k] <= tol[k]}


def merge(worst, d):
    for k in KEYS:
        if k in d:
            worst[k] = max(worst.get(k, 0.0), d[k])
    return worst


def outputs(E):
    """evaluate()'s numbers in cpe_eval_normal's layout and float64 (what a kernel would return)"""
    f = lambda a: np.asarray(a).astype(np.float64)
    return dict(g=f(E["g"]), Bm=f(E["Bm"]), cost=f(E["cost"]), q_out=f(E["q"]))


# ---- the two measurements the tolerances stand on (CPU) --------------------------------------------------------------------------------
def ulp_spread(sk, cams, opts, pr, qc, meas, weight, draws=4, seed=0):
    """measurement 1 of a batch of frames: the float64 evaluation at qc against itself at qc moved by one ulp in a random direction per entry"""
    E = evaluate(sk, cams, opts, pr, qc, meas, weight, np.float64, stencil=np.longdouble)
    R = make_reference(E, np.asarray(E["q"]), opts)
    rng = np.random.default_rng(seed)
    worst = {}
    for _ in range(draws):
        q1 = np.nextafter(qc, np.where(rng.random(qc.shape) < 0.5, -np.inf, np.inf))
        merge(worst, discrepancies(outputs(evaluate(sk, cams, opts, pr, q1, meas, weight, np.float64, stencil=np.longdouble)), R))
    return worst


def extended_distance(sk, cams, opts, pr, qc, meas, weight, R=None):
    """measurement 2 of a batch of frames: the float64 evaluation against the np.longdouble one (q_out: the two maps' consistent q)"""
    if R is None:
        R = make_reference(evaluate(sk, cams, opts, pr, qc, meas, weight, np.longdouble), qc, opts)
    R = dict(R, q_out=R["q"])
    return discrepancies(outputs(evaluate(sk, cams, opts, pr, qc, meas, weight, np.float64, stencil=np.longdouble)), R)


# ---- the inputs of the GPU cases (shared with the CPU test, which checks the conditions and re-measures the tolerances on them) -----------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRIOR_FILES = dict(packaged=None, k3_w2_dense="priors_k3_w2_dense.npz", k3_w5_dense="priors_k3_w5_dense.npz", k5_w6_lasso="priors_k5_w6_lasso.npz")
CAMERA_COUNTS = (1, 13, 14, 18)
CAMW = 22                                                                            # doubles of one camera in k_frame_normal's LDS
B, N = 2, 5
CASES = (("plain", "loss-c0", "loss-c1", "knots") + tuple(f"cams{c}" for c in CAMERA_COUNTS) + ("weights", "bounds")
         + tuple(f"prior-{p}-c{c}" for p in PRIOR_FILES for c in (1, 2, 6)))


def n_camov(sk):
    """doubles of k_frame_normal's LDS from the sin / cos table to the end of the trunk rotations, which the cameras later overlay
    (cpe_solver.hip.inc: 6 nl + 2 nrev + 36 n_trunk); the positions start at max(n_camov, CAMW C)"""
    legs = {c for c, _ in synth.leg_layout(sk)}
    return 6 * sk.n_links + 2 * len(legs) + 36 * (sk.n_links - len(legs))


def load_prior(name):
    return priors.load_priors() if PRIOR_FILES[name] is None else priors.load_priors(path=os.path.join(GOLDEN, PRIOR_FILES[name]))


def cyclic_cameras(n):
    """the six-camera rig repeated cyclically to n cameras, as the pairwise pseudo-measurements repeat it"""
    c6 = synth.make_cameras(6)
    return (abi.Camera * n)(*[c6[i % 6] for i in range(n)])


def clear_near(sk, cams, q, weight):
    """weight with every pair within NEAR_Z of its camera's plane set to 0 (at the float64 numpy map's positions of q)"""
    z = RC.depth(sk, cams, q)
    return np.where(np.abs(z) < 1.5 * NEAR_Z, 0.0, weight)


def truths(sk, n_frames, seed, fps=120.0, first=0):
    """frames first .. first + n_frames of the synthetic runs seed, seed + 1: q_true [2, n_frames, nq]"""
    return np.stack([synth.truth_trajectory(sk, first + n_frames, fps, np.random.default_rng(seed + b))[first:] for b in range(B)])


def observe(sk, cams, q_true, seed, kinetic_dataset=False, noise_px=2.0, outlier_frac=0.10, keep=0.5):
    """(meas [.., C, L, 2], weight [.., C, L]) of q_true [.., nq] as synth.make_batch draws them -- 2 px of noise, 10 % outliers anywhere in the
    image, half of the pairs dropped, weight 1 / sigma_l -- except that a pair counts as seen wherever the marker lies in front of the camera
    (beyond 2 NEAR_Z), on the image or off it.  The camera models are defined there too, and on no stretch of a run do all six cameras of the
    20 m rig have the animal ON their images: with make_batch's own rule four of them, and twelve of the 18 cyclic copies, would hold
    nothing but outliers, which add nothing to g or Bm"""
    rng = np.random.default_rng(seed)
    sigma = skeleton.measurement_sigma(sk.n_markers, kinetic_dataset)
    pos = synth.fk_numpy(sk, q_true)[0]
    meas, weight = [], []
    for c in range(len(cams)):
        uv, z = synth.project_numpy(cams[c], pos)
        uv = uv + rng.normal(0, noise_px, uv.shape)
        out = rng.random(z.shape) < outlier_frac
        uv[out] = np.stack([rng.uniform(0, synth.IMG_W, out.sum()), rng.uniform(0, synth.IMG_H, out.sum())], axis=-1)
        seen = (z > 2 * NEAR_Z) & (rng.random(z.shape) < keep)
        uv[~seen] = 0.0
        meas.append(uv)
        weight.append(np.where(seen, 1.0 / sigma, 0.0))
    return np.ascontiguousarray(np.stack(meas, axis=-3)), np.ascontiguousarray(np.stack(weight, axis=-2))


def plain_inputs(n_frames=6):
    """the pose of test_frame_normal_matches_oracle (tests/test_gpu_parity.py): phantom 25, six fisheye cameras, the truth of seed 41 + noise, a
    rolled base and four limbs swung far beyond 90 degrees; measurements by observe(), so that every camera holds inliers"""
    sk, cams = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6)
    qt = truths(sk, 6, 41)
    rng = np.random.default_rng(8)
    q = qt + rng.normal(0, 0.02, qt.shape)
    q[..., 3] += 0.25
    for lk in ("HFL", "LBR", "LFR", "UBL"):
        q[..., skeleton.dof(lk, 1)] += rng.uniform(1.2, 2.2)
    meas, weight = observe(sk, cams, qt, 4100)
    cut = lambda a: np.ascontiguousarray(a[:, :n_frames])
    return dict(sk=sk, cams=cams, opts=abi.default_options(), pr=None, q=cut(q), meas=cut(meas), weight=cut(clear_near(sk, cams, q, weight)))


def prior_inputs(prior="packaged", n_cams=1):
    """the pose of test_pose_prior_frame_term_matches_oracle (tests/test_gpu_parity.py): phantom 24 near the mixture's support (the truth of
    seed 43 + N(0, 0.01)); one camera (the third of the rig), two or six; measurements by observe()"""
    sk = skeleton.build_skeleton("phantom", 24)
    c6 = synth.make_cameras(6)
    cams = (abi.Camera * 1)(c6[2]) if n_cams == 1 else (synth.make_cameras(2) if n_cams == 2 else c6)
    qt = truths(sk, N, 43)
    q = qt + np.random.default_rng(3).normal(0, 0.01, qt.shape)
    q[..., 3] += 0.05
    meas, weight = observe(sk, cams, qt, 4700 + n_cams)
    return dict(sk=sk, cams=cams, opts=abi.default_options(), pr=load_prior(prior), q=q, meas=meas, weight=clear_near(sk, cams, q, weight))


def _noisy(sk, cams, seed, fps=120.0, kin=False, sd=0.02, first=0, n_frames=N):
    """frames first .. first + n_frames of two synthetic runs: q = the truth + N(0, sd), measurements by observe()"""
    qt = truths(sk, n_frames, seed, fps, first)
    q = qt + np.random.default_rng(seed + 1000).normal(0, sd, qt.shape)
    meas, weight = observe(sk, cams, qt, seed + 2000, kin)
    return q, meas, clear_near(sk, cams, q, weight)


def loss_inputs(curvature, n_frames=N, seed=4200):
    """phantom 25, six cameras, 2 x n_frames: every weighted residual placed in a piece of the loss drawn at random, |s| in (0.2, a), (a, b),
    (b, c) or (c, 2 c), 0.05 away from the knots; opts.curvature as given"""
    sk, cams, opts = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options()
    opts.curvature = curvature
    q, meas, weight = _noisy(sk, cams, seed, n_frames=n_frames)
    rng = np.random.default_rng(seed + 1)
    uv = pixels(sk, cams, u_of_q(sk, q))[0]                                          # at the consistent q the kernel evaluates
    knots = np.array([0.2, opts.loss_a, opts.loss_b, opts.loss_c, 2 * opts.loss_c])
    piece = rng.integers(0, 4, uv.shape)
    e = rng.uniform(knots[piece] + 0.05, knots[piece + 1] - 0.05) * rng.choice([-1.0, 1.0], uv.shape)
    on = weight > 0
    meas = np.where(on[..., None], uv - e / np.where(on, weight, 1.0)[..., None], meas)
    return dict(sk=sk, cams=cams, opts=opts, pr=None, q=q, meas=np.ascontiguousarray(meas), weight=np.ascontiguousarray(weight))


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """dict(sk, cams, opts, pr, q [2, 5, nq], meas [2, 5, C, L, 2], weight [2, 5, C, L]) of a case, plus what the case asserts about itself"""
    if name == "plain":
        return plain_inputs(N)
    if name.startswith("prior-"):
        _, p, c = name.split("-")
        return prior_inputs(p, int(c[1:]))
    sk, cams, opts = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options()
    extra = {}
    if name.startswith("loss-c"):
        return loss_inputs(int(name[-1]))
    if name == "knots":
        # the kinetic-dataset rig: four pinhole cameras with radial distortion and multipliers (1, 1, 0.6, 0.6), an `-02` skeleton, 200 fps
        from test_gpu_parity import _kinetic_setup
        sk, cams = _kinetic_setup()
        opts = abi.default_options(200.0)
        opts.loss_a, opts.loss_b, opts.loss_c = 2.0, 6.0, 15.0
        q, meas, weight = _noisy(sk, cams, 4300, fps=200.0, kin=True, first=100)     # (half a second into the run: on the images of all four cameras)
    elif name.startswith("cams"):
        cams = cyclic_cameras(int(name[4:]))
        q, meas, weight = _noisy(sk, cams, 4400 + int(name[4:]))
    elif name == "weights":
        q, meas, weight = _noisy(sk, cams, 4500)
        weight[0, 1] = 0.0; meas[0, 1] = 0.0                                         # a frame without any measurement
        seen = np.flatnonzero((weight[0, 2] > 0).sum(axis=0) >= 2)
        m = int(seen[0]); keep = int(np.flatnonzero(weight[0, 2, :, m] > 0)[0])
        for c in range(6):                                                           # a marker seen by exactly one camera
            if c != keep:
                weight[0, 2, c, m] = 0.0
        gap = np.random.default_rng(4501).random(weight[1].shape) < 0.3             # NaN gaps: weight 0 and measurement 0
        weight[1][gap] = 0.0; meas[1][gap] = 0.0
        extra = dict(zero_frame=(0, 1), single=(0, 2, m, keep), gaps=int(gap.sum()))
    elif name == "bounds":
        q, meas, weight = _noisy(sk, cams, 4600)
        nb = sk.n_bounds
        find = lambda a, ang, b: next(i for i in range(nb) if sk.bound_a[i] == skeleton.dof(a, ang) and
                                      sk.bound_b[i] == (-1 if b is None else skeleton.dof(b, ang)))
        TH, PH = skeleton.THETA, skeleton.PHI
        i_plain, i_diff, i_legs, i_body = find("base", PH, None), find("neck", TH, "bodyF"), find("UBL", TH, "LBL"), find("bodyF", TH, "UFL")
        q[0, 0, skeleton.dof("base", PH)] = sk.bound_up[i_plain] + 0.2                # a plain upper bound
        q[0, 1, skeleton.dof("base", PH)] = sk.bound_lo[i_plain] - 0.2                # a plain lower bound
        q[0, 2, skeleton.dof("neck", TH)] = q[0, 2, skeleton.dof("bodyF", TH)] + sk.bound_up[i_diff] + 0.2       # a difference of trunk angles
        q[0, 3, skeleton.dof("LBL", TH)] = q[0, 3, skeleton.dof("UBL", TH)] + 0.3     # thigh - calf below its lower limit 0: two leg pitches
        q[0, 4, skeleton.dof("UFL", TH)] = q[0, 4, skeleton.dof("bodyF", TH)] - sk.bound_lo[i_body] + 0.2        # body - thigh: trunk pitch and leg pitch
        weight = clear_near(sk, cams, q, weight)
        extra = dict(expect_active=((0, 0, i_plain, 0), (0, 1, i_plain, 1), (0, 2, i_diff, 0), (0, 3, i_legs, 1), (0, 4, i_body, 1)))
    else:
        raise KeyError(name)
    return dict(sk=sk, cams=cams, opts=opts, pr=None, q=q, meas=np.ascontiguousarray(meas), weight=np.ascontiguousarray(weight), **extra)


def flat(c):
    """(q [F, nq], meas [F, C, L, 2], weight [F, C, L]) of a case's [B, N, ...] inputs"""
    return tuple(np.ascontiguousarray(c[k].reshape((-1,) + c[k].shape[2:])) for k in ("q", "meas", "weight"))


@functools.lru_cache(maxsize=None)
def case_reference(oracle, name):
    """the np.longdouble reference of a case (computed once per process)"""
    c = case_inputs(name)
    return reference(oracle, c["sk"], c["cams"], c["opts"], c["pr"], *flat(c))


def with_curvature(opts, mode):
    o = abi.Options.from_buffer_copy(bytes(opts))
    o.curvature = mode
    return o


def oracle_outputs(oracle, sk, cams, opts, pr, q, meas, weight):
    """oracle.frame_normal of F frames in cpe_eval_normal's layout"""
    out = [oracle.frame_normal(sk, cams, opts, pr, q[f], meas[f], weight[f]) for f in range(q.shape[0])]
    return dict(g=np.stack([o[0] for o in out]), Bm=np.stack([o[1] for o in out]), cost=np.stack([o[2] for o in out]),
                q_out=np.stack([o[4] for o in out]))


def hip_outputs(h, q, meas, weight, want_gam=False):
    """cpe_eval_normal of handle h on q [B, N, nq], meas, weight: dict(g, Bm, cost, q_out[, gam]) with the frames flattened [B N, ...]"""
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    E = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    Bn, Nn = q.shape[:2]
    nu = abi.NX
    out = dict(g=E(Bn, Nn, nu), Bm=E(Bn, Nn, nu, nu), cost=E(Bn, Nn, 3), q_out=E(Bn, Nn, h.sk.nq))
    gam = E(Bn, Nn, len(synth.leg_layout(h.sk)), 4) if want_gam else None
    h.eval_normal(T(q), T(meas), T(weight), out["g"], out["Bm"], out["cost"], gam, out["q_out"])
    h.synchronize()
    res = {k: v.cpu().numpy().reshape((Bn * Nn,) + tuple(v.shape[2:])) for k, v in out.items()}
    if want_gam:
        res["gam"] = gam.cpu().numpy().reshape((Bn * Nn,) + tuple(gam.shape[2:]))
    return res


# ---- `python -m tests.frame_compare`: the tables of the module docstring ---------------------------------------------------------------
def measure(oracle, names=CASES, log=print):
    """(measurement 1, measurement 2, the oracle's distance) per key over the cases `names`"""
    m1, m2, mo = {}, {}, {}
    for i, name in enumerate(names):
        c = case_inputs(name)
        q, meas, weight = flat(c)
        R = case_reference(oracle, name)
        assert conditions_hold(R), (name, R["conditions"])
        a = ulp_spread(c["sk"], c["cams"], c["opts"], c["pr"], R["q_out"], meas, weight, seed=i)
        b = extended_distance(c["sk"], c["cams"], c["opts"], c["pr"], R["q_out"], meas, weight, R)
        o = {}
        for mode in (0, 1):
            op = with_curvature(c["opts"], mode)
            Rm = R if mode == c["opts"].curvature else reference(oracle, c["sk"], c["cams"], op, c["pr"], q, meas, weight)
            merge(o, discrepancies(oracle_outputs(oracle, c["sk"], c["cams"], op, c["pr"], q, meas, weight), Rm))
        log(f"{name:22s} (1) " + ", ".join(f"{k} {a[k]:.2e}" for k in MEASURED_KEYS) + " | (2) " + ", ".join(f"{k} {b[k]:.2e}" for k in MEASURED_KEYS)
            + " | oracle " + ", ".join(f"{k} {o[k]:.2e}" for k in KEYS))
        merge(m1, a); merge(m2, b); merge(mo, o)
    return m1, m2, mo


if __name__ == "__main__":
    from oracle import oracle as O
    O.lib()
    m1, m2, mo = measure(O)
    for k in MEASURED_KEYS:
        print(f"  {k:9s}  {m1[k]:.2e}        {m2[k]:.2e}        {MARGIN * max(m1[k], m2[k]):.2e}")
    print("  oracle: " + ", ".join(f"{k} {mo[k]:.2e}" for k in KEYS))
