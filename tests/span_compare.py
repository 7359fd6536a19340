"""Reference side of the tests of the covariance between distant frames (cpe_covariance_columns, estimator.span_uncertainty).  Helper, not a
test module.

A column of Sigma = A^-1 above an anchor frame a: the blocks Sigma(n, a), n = 0 .. a, zero below (cpe_covariance_columns' layout, [N][28][28]
per anchor).  Two float64 routes to it, both numpy:
  dense        the blocks of the dense inverse (cov_compare.dense_inverse)
  recurrence   numpy's Cholesky factor in cpe_eval_lm_step's layout, cov_compare.takahashi for the band, then
               Sigma(n,a) = - sum_k G_k(n)^T Sigma(n+k,a), G_k(n) = L(n+k,n) L(n,n)^-1, n = a-PB-1 .. 0, seeded by the band blocks

Error unit of a column (`column_error`): |difference| / sqrt(Sigma(n,n)_ii Sigma(a,a)_jj) of the reference, worst over the column.
Error unit of a span covariance (`span_error`): |difference| / sqrt(T_ii T_jj), T = P_b S_bb P_b^T + P_a S_aa P_a^T of the reference -- the
independent-frames sum, so that the cancellation between strongly correlated frames (one camera) does not inflate the unit.
Tolerance of a GPU result on a matrix (`reference`, `span_reference`): 10 x max(r, 2^-52 x Jacobi-scaled condition number), r = the same measure
between the two routes above on that matrix -- cov_compare's rule: set by the reference alone, never by the GPU's numbers; the factor 10 covers
the summation order.

Worst values measured on an MI355X (tests/test_gpu_span_covariance.py::test_zz_report; the table is in DESIGN.md 4), error / its tolerance:
  random bands             columns 1.2e-12 / 1.2e-11 (N = 57, PB = 4); short sequences N = 1, 4, 5: 6.8e-14 / 6.8e-13; lengths 5, 12, 40 in one
                           call: 1.8e-12 / 1.8e-11
  the solver's own factor  N = 40, anchors 39, 20, 5, against the dense inverse of L L^T: 6 cameras 6.1e-11 / 7.9e-9 (ridge 0), 2.8e-11 / 4.8e-9
                           (ridge 1e-6); 1 camera + priors (PB = 4) 1.2e-7 / 1.9e-5 (ridge 0, scaled condition 8.5e9), 1.5e-10 / 1.2e-8 (ridge 1e-6)
  estimator, end to end    span covariance of the centre of mass 2.1e-12, of the markers 5.3e-12 / 1.5e-9
  the two numpy routes     4.6e-11 (6 cameras), 2.4e-10 (2 cameras), 1.2e-7 (1 camera) at ridge 0 on the CPU (tests/test_span_covariance_host.py)
"""
import numpy as np

import cov_compare as CC

NX = CC.NX
EPS = CC.EPS


# ---- columns ----------------------------------------------------------------------------------------------------------------------------------
def columns_from_factor(L, diag, off, anchors):
    """route `recurrence`: [K][N][28][28] from a factor in cpe_eval_lm_step's layout and the band (diag, off) of its inverse; an anchor of -1
    gives a zero column"""
    N, PB = L.shape[0], L.shape[1] - 1
    G = np.zeros((N, PB + 1, NX, NX))
    for n in range(N):
        T = np.linalg.inv(L[n, 0])
        for k in range(1, PB + 1):
            if n + k < N:
                G[n, k] = L[n, k] @ T
    cols = np.zeros((len(anchors), N, NX, NX))
    for s, a in enumerate(anchors):
        if a < 0:
            continue
        cols[s, a] = diag[a]
        for i in range(1, PB + 1):
            if a - i >= 0:
                cols[s, a - i] = off[a - i, i - 1].T
        for n in range(a - PB - 1, -1, -1):
            cols[s, n] = -sum(G[n, k].T @ cols[s, n + k] for k in range(1, PB + 1))
    return cols


def columns_dense(S, anchors):
    """route `dense`: the same blocks cut from the dense inverse S"""
    N = S.shape[0] // NX
    cols = np.zeros((len(anchors), N, NX, NX))
    for s, a in enumerate(anchors):
        for n in range(0, a + 1):
            cols[s, n] = S[n * NX:(n + 1) * NX, a * NX:(a + 1) * NX]
    return cols


def column_error(cols, ref_cols, ref_diag, anchors):
    """worst |difference| / sqrt(Sigma(n,n)_ii Sigma(a,a)_jj) over the columns (inf where something is not finite)"""
    if not np.all(np.isfinite(cols)):
        return float("inf")
    s = np.sqrt(np.diagonal(ref_diag, axis1=1, axis2=2))          # [N, 28]
    worst = 0.0
    for k, a in enumerate(anchors):
        if a >= 0:
            worst = max(worst, float((np.abs(cols[k] - ref_cols[k]) / (s[:, :, None] * s[a][None, None, :])).max()))
    return worst


def reference(Ad, Hk, anchors):
    """both routes on one matrix: dict(cols, diag, off = the dense route, S = the dense inverse, L = numpy's factor, r = the discrepancy between
    the routes, cond, tol = 10 max(r, 2^-52 cond))"""
    anchors = [int(a) for a in anchors]
    d1, o1, S = CC.dense_inverse(Ad, Hk)
    L = CC.cholesky_layout(Ad, Hk)
    d2, o2 = CC.takahashi(L)
    c1, c2 = columns_dense(S, anchors), columns_from_factor(L, d2, o2, anchors)
    r = column_error(c2, c1, d1, anchors)
    cond = CC.scaled_condition(Ad, Hk)
    return dict(cols=c1, diag=d1, off=o1, S=S, L=L, r=r, cond=cond, tol=10.0 * max(r, EPS * cond))


# ---- spans ------------------------------------------------------------------------------------------------------------------------------------
def span_cov_dense(S, P, a, b):
    """cov(p_b - p_a) = J S J^T with the stacked Jacobian J = [.. -P_a .. P_b ..], P [N, ..., 3, 28]; and T, the independent-frames sum"""
    blk = lambda r, c: S[r * NX:(r + 1) * NX, c * NX:(c + 1) * NX]
    T_ = lambda M: np.swapaxes(M, -1, -2)
    Pa, Pb = P[a], P[b]
    X = Pb @ blk(b, a) @ T_(Pa)
    T = Pb @ blk(b, b) @ T_(Pb) + Pa @ blk(a, a) @ T_(Pa)
    return T - X - T_(X), T


def span_error(cov, ref, T):
    """worst |difference| / sqrt(T_ii T_jj) over the blocks [..., 3, 3]"""
    if not np.all(np.isfinite(cov)):
        return float("inf")
    s = np.sqrt(np.diagonal(T, axis1=-2, axis2=-1))
    return float((np.abs(cov - ref) / (s[..., :, None] * s[..., None, :])).max())


def span_reference(Ad, Hk, P_com, P_pos, spans):
    """the span covariances of the centre of mass [S, 3, 3] and of every marker [S, L, 3, 3] by both routes: dict(com, pos = the dense route,
    T_com, T_pos = its independent-frames sums, r = the discrepancy between the routes in span_error's unit, cond, tol)"""
    R = reference(Ad, Hk, sorted({b for _, b in spans}))
    anchors = sorted({b for _, b in spans})
    d2, o2 = CC.takahashi(R["L"])
    c2 = columns_from_factor(R["L"], d2, o2, anchors)
    S2 = np.zeros_like(R["S"])                                    # the recurrence route's blocks, placed where span_cov_dense reads them
    N = Ad.shape[0]
    for n in range(N):
        S2[n * NX:(n + 1) * NX, n * NX:(n + 1) * NX] = d2[n]
    for k, b in enumerate(anchors):
        for n in range(b):
            S2[b * NX:(b + 1) * NX, n * NX:(n + 1) * NX] = c2[k, n].T
    out = dict(com=[], pos=[], T_com=[], T_pos=[])
    r = 0.0
    for a, b in spans:
        for key, P in (("com", P_com), ("pos", P_pos)):
            c, T = span_cov_dense(R["S"], P, a, b)
            r = max(r, span_error(span_cov_dense(S2, P, a, b)[0], c, T))
            out[key].append(c); out["T_" + key].append(T)
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(r=r, cond=R["cond"], tol=10.0 * max(r, EPS * R["cond"]))
    return out
