"""Reference side of the rate-covariance tests (cpe_rate_covariance, include/cpe.h).  Helper, not a test module.  Pure numpy on top of
tests/cov_compare.py, oracle.move_coordinate and synth.fk_numpy.

A band is (diag [N][28][28] = Sigma(n, n), off [N][PB][28][28], off[n][i - 1] = Sigma(n + i, n)), cpe_band_inverse's layout.  A rate is a
stencil sum_i c_i u_{f_i} over at most three consecutive frames; its covariance is sum_i sum_j c_i c_j Sigma(f_i, f_j).  The coefficients are
k / h (velocity) and k / (h h) (acceleration), k a small integer -- one rounding each, the same numbers the kernel forms.

Round-off bound of an entry that is a recursive sum of n products of three factors: (n + 3) 2^-52 x (the same expression with every factor
replaced by its absolute value) -- `abs_bound` gives that expression, the tests multiply."""
import numpy as np

import cov_compare as CC

NX = CC.NX
EPS = CC.EPS


def stencils(NL, n, h):
    """(velocity, acceleration) rows n of a sequence of NL frames, each a list of (frame, coefficient), frames ascending, empty = zero.  Velocity:
    (u_n - u_{n-1}) / h; row 0 is the gauge of the solve's dq: (-2 u_0 + 3 u_1 - u_2) / h (NL >= 3), (u_1 - u_0) / h (NL == 2), nothing (NL == 1).
    Acceleration: (u_m - 2 u_{m-1} + u_{m-2}) / h^2 at m = max(n, 2); nothing for NL < 3."""
    if n >= 1:
        vel = [(n - 1, -1.0 / h), (n, 1.0 / h)]
    elif NL >= 3:
        vel = [(0, -2.0 / h), (1, 3.0 / h), (2, -1.0 / h)]
    elif NL == 2:
        vel = [(0, -1.0 / h), (1, 1.0 / h)]
    else:
        vel = []
    acc = []
    if NL >= 3:
        m, h2 = max(n, 2), h * h
        acc = [(m - 2, 1.0 / h2), (m - 1, -2.0 / h2), (m, 1.0 / h2)]
    return vel, acc


def block(diag, off, r, c):
    """Sigma(r, c) from the band"""
    if r == c:
        return diag[r]
    return off[c, r - c - 1] if r > c else off[r, c - r - 1].T


def _stencil_cov(st, diag, off, absolute=False, cross_sign=1.0):
    out = np.zeros((NX, NX))
    for i, (fi, ci) in enumerate(st):
        for j, (fj, cj) in enumerate(st):
            S, w = block(diag, off, fi, fj), ci * cj
            if absolute:
                S, w = np.abs(S), abs(w)
            elif i != j:
                w = cross_sign * w
            out = out + w * S
    return out


def rates_from_band(diag, off, h, absolute=False, cross_sign=1.0, gauge=True):
    """(cov_du, cov_ddu) [N][28][28] by the stencil formulas.  absolute: the bound expression (every factor by its absolute value).  The two
    deliberately wrong variants for the power tests: cross_sign = -1 flips the sign of the cross terms; gauge = False leaves row 0 of the velocity
    zero and gives the acceleration rows 0 and 1 no stencil."""
    N = diag.shape[0]
    du, ddu = np.zeros((N, NX, NX)), np.zeros((N, NX, NX))
    for n in range(N):
        vel, acc = stencils(N, n, h)
        if not gauge and n == 0:
            vel = []
        if not gauge and n < 2:
            acc = []
        du[n] = _stencil_cov(vel, diag, off, absolute, cross_sign)
        ddu[n] = _stencil_cov(acc, diag, off, absolute, cross_sign)
    return du, ddu


def difference_matrices(N, h):
    """(Dv, Da) [(N 28) x (N 28)]: the explicit difference operators, rows by `stencils`"""
    Dv, Da = np.zeros((N * NX, N * NX)), np.zeros((N * NX, N * NX))
    I = np.eye(NX)
    for n in range(N):
        vel, acc = stencils(N, n, h)
        for f, c in vel:
            Dv[n * NX:(n + 1) * NX, f * NX:(f + 1) * NX] += c * I
        for f, c in acc:
            Da[n * NX:(n + 1) * NX, f * NX:(f + 1) * NX] += c * I
    return Dv, Da


def rates_dense(S, h):
    """the independent route: the diagonal blocks of D S D^T for the dense inverse S and the explicit difference matrices"""
    N = S.shape[0] // NX
    Dv, Da = difference_matrices(N, h)
    Cv, Ca = Dv @ S @ Dv.T, Da @ S @ Da.T
    cut = lambda M: np.stack([M[n * NX:(n + 1) * NX, n * NX:(n + 1) * NX] for n in range(N)])
    return cut(Cv), cut(Ca)


def point_cov(P, diag, absolute=False):
    """P Sigma(n,n) P^T for P [N][..., 3, 28] (markers [N][L][3][28] or the centre of mass [N][3][28])"""
    if absolute:
        P, diag = np.abs(P), np.abs(diag)
    return np.einsum("n...ak,nkj,n...bj->n...ab", P, diag, P)


def point_vel_cov(P, diag, off, h, absolute=False):
    """first-order covariance of (p(u_n) - p(u_{n-1})) / h: (P_n S_nn P_n^T + P_{n-1} S_{n-1,n-1} P_{n-1}^T - P_n S_{n,n-1} P_{n-1}^T - (that)^T) / h^2;
    row 0 is zero.  P as in point_cov."""
    out = np.zeros(P.shape[:-1] + (3,))
    if P.shape[0] < 2:
        return out
    if absolute:
        P, diag, off = np.abs(P), np.abs(diag), np.abs(off)
    own = np.einsum("n...ak,nkj,n...bj->n...ab", P, diag, P)
    cross = np.einsum("n...ak,nkj,n...bj->n...ab", P[1:], off[:-1, 0], P[:-1])          # P_n Sigma(n, n-1) P_{n-1}^T
    crossT = np.swapaxes(cross, -1, -2)
    out[1:] = (own[1:] + own[:-1] + (cross + crossT if absolute else -cross - crossT)) / (h * h)
    return out


def abs_bound(kind, *args):
    """the bound expression of `kind` in ("rates", "point", "point_vel"): the same formula with every factor replaced by its absolute value"""
    if kind == "rates":
        return rates_from_band(*args, absolute=True)
    if kind == "point":
        return point_cov(*args, absolute=True)
    if kind == "point_vel":
        return point_vel_cov(*args, absolute=True)
    raise KeyError(kind)


def roundoff_tolerance(n_products, bound):
    """(n + 3) 2^-52 |expression|: a recursive sum of n three-factor products"""
    return (n_products + 3) * EPS * bound


def com_jacobians(oracle, sk, q, frames, step):
    """Pc [len(frames)][3][28] = d com / d u at the listed frames: central differences of synth.fk_numpy's centre of mass through
    oracle.move_coordinate, as cov_compare.marker_jacobians does for the markers"""
    from cheetah_pose_estimation_amd import synth
    out = []
    for n in frames:
        P = np.zeros((3, NX))
        for k in range(NX):
            cp = synth.fk_numpy(sk, oracle.move_coordinate(sk, q, n, k, +step)[n])[1]
            cm = synth.fk_numpy(sk, oracle.move_coordinate(sk, q, n, k, -step)[n])[1]
            P[:, k] = (cp - cm) / (2.0 * step)
        out.append(P)
    return np.stack(out)


def variance_ratio(du, diag, h):
    """h^2 var(du_n) / (var u_n + var u_{n-1}) [N-1][28], n >= 1: below 1 where consecutive frames are positively correlated"""
    v = np.diagonal(diag, axis1=1, axis2=2)
    return (h * h) * np.diagonal(du, axis1=1, axis2=2)[1:] / (v[1:] + v[:-1])


def bits_symmetric(a):
    """blocks [..., k, k] equal their transposes bit for bit"""
    a = np.ascontiguousarray(a)
    return a.tobytes() == np.ascontiguousarray(np.swapaxes(a, -1, -2)).tobytes()
