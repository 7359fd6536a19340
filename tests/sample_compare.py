"""Reference side of the posterior-sample tests (cpe_band_sample / cpe_posterior_samples, include/cpe.h).  Helper, not a test module.

The factor: L [N][PB + 1][28][28] in cpe_band_inverse's layout (block [n][i] = block (n + i, n) of the lower Cholesky factor, true diagonal), of
the matrix A = L L^T, Sigma = A^-1.  A draw: du with L^T du = z.  z and du are [S][N][28], one trajectory per sample.

Two float64 routes to du, both numpy:
  route 1   scipy.linalg.solve_triangular on the dense L^T
  route 2   the block recurrence the HIP kernel runs (du_n = L(n,n)^-T (z_n - sum_i L(n+i,n)^T du_{n+i}), newest frame first) in np.longdouble

Error unit (`scaled_error`): |du - ref| / (s_a ||z||_2), s_a = sqrt(Sigma_aa) from the dense inverse, ||z||_2 over the whole trajectory, worst
over entries and samples.  |du_a| = |e_a^T L^-T z| <= ||L^-1 e_a|| ||z|| = s_a ||z|| holds exactly, so the unit is scale-free across metres and
radians.  Tolerance of a GPU result on a matrix (`reference`): 10 x max(r, 2^-52 x cov_compare.scaled_condition), r = the same measure between the
two routes on that matrix: set by the reference alone, never by the GPU's numbers (cov_compare.tolerance's rule; the factor 10 covers the
different summation order).

Identity check: with z = the 28 N unit vectors, sum_s du_s du_s^T = L^-T L^-1 = Sigma.  Cut to the band it is compared with the band of the dense
inverse in cov_compare.scaled_error's unit; tolerance 10 x max(e_ref, 2^-52 cond), e_ref = the error of the same sum formed from route 1 (on the
CPU e_ref reaches 3.8e-13 at N = 40, above 2^-52 cond of the random bands: it has to be part of the bound).

Measured on the CPU on cov_compare.random_band, (N, PB) = (1, 3), (5, 3), (11, 4), (40, 4), (40, 3) (tests/test_posterior_samples_host.py):
r <= 2.3e-16, 2^-52 cond ~ 3e-14, max |du| / (s ||z||) <= 0.64.

Worst values measured on an MI355X (tests/test_gpu_posterior_samples.py::test_zz_report; the table is in DESIGN.md 4), error / its tolerance:
  random bands, PB 3 / 4   every N = 1 .. 2 PB + 3 and 57 at S = 65: 4.7e-16 / 2.6e-13; N = 200, S = 64: 8.2e-17 / 3.3e-13; N = 11 at S = 1, 63, 64,
                           65, 130: 2.8e-16 / 2.9e-13
  the solver's factors     N = 40, ridge 0 and 1e-6: 6 cameras 4.7e-15 / 7.9e-9 and 3.9e-15 / 4.8e-9, 2 cameras 6.8e-15 / 7.4e-8 and 4.9e-15 / 1.1e-8,
                           1 camera + priors (PB = 4, scaled condition 8.5e9 at ridge 0) 4.7e-14 / 1.9e-5 and 5.3e-15 / 1.2e-8
  identity, N = 6          against the dense inverse PB 3: 6.5e-14 / 6.5e-13, PB 4: 2.1e-14 / 2.4e-13; against cpe_band_inverse 1.5e-15 and 1.3e-15
  poses, 6 frames x 3      positions 8.9e-16 m, q through sin / cos 2.3e-15, joint equalities 4.3e-16; du = 0 against cpe_forward_kinematics 2.2e-16 m
"""
import numpy as np

import cov_compare as CC
import lm_compare as LC

NX = CC.NX
EPS = CC.EPS


def dense_factor(L):
    """the dense lower-triangular factor of the blocks L [N][PB + 1][28][28] (blocks with n + i >= N are not read)"""
    N, PB = L.shape[0], L.shape[1] - 1
    D = np.zeros((N * NX, N * NX))
    for n in range(N):
        for i in range(min(PB, N - 1 - n) + 1):
            D[(n + i) * NX:(n + i + 1) * NX, n * NX:(n + 1) * NX] = L[n, i]
    return D


def solve_dense(L, z):
    """route 1: du [S][N][28] with L^T du = z, LAPACK's triangular solve on the dense factor"""
    from scipy.linalg import solve_triangular
    S, N = z.shape[0], z.shape[1]
    x = solve_triangular(dense_factor(L).T, z.reshape(S, N * NX).T, lower=False)
    return np.ascontiguousarray(x.T).reshape(S, N, NX)


def solve_recurrence(L, z):
    """route 2: the block recurrence, newest frame first, in np.longdouble; rounded to float64 at the end"""
    N, PB = L.shape[0], L.shape[1] - 1
    Ll, zl = L.astype(np.longdouble), z.astype(np.longdouble)
    x = np.zeros((N, NX, z.shape[0]), np.longdouble)
    for n in range(N - 1, -1, -1):
        t = zl[:, n].T.copy()                               # [28][S]
        for i in range(1, PB + 1):
            if n + i < N:
                t -= Ll[n, i].T @ x[n + i]
        U = Ll[n, 0].T                                      # upper triangular
        for m in range(NX - 1, -1, -1):
            x[n, m] = (t[m] - U[m, m + 1:] @ x[n, m + 1:]) / U[m, m]
    return np.ascontiguousarray(np.transpose(x, (2, 0, 1))).astype(np.float64)


def scaled_error(du, ref, s, z):
    """worst |du - ref| / (s_a ||z||_2): du, ref, z [S][N][28], s [N][28] (inf where du is not finite)"""
    if not np.all(np.isfinite(du)):
        return float("inf")
    zn = np.linalg.norm(z.reshape(z.shape[0], -1), axis=1)
    return float((np.abs(du - ref) / (s[None] * zn[:, None, None])).max())


def unit_vectors(N):
    """z [28 N][N][28]: sample s is the unit vector e_s of the trajectory's 28 N coordinates"""
    return np.eye(N * NX).reshape(N * NX, N, NX)


def band_of_sum(du, PB):
    """(diag, off) = sum_s du_s du_s^T cut to the band, in the covariance layout of cov_compare"""
    X = du.reshape(du.shape[0], -1)
    return CC.cut_band(X.T @ X, PB)


def reference(L, z=None, identity=False):
    """both routes on the factor L for the right-hand sides z [S][N][28]: dict(Ad, Hk = the band of L L^T, diag, off = the band of its dense
    inverse, s [N][28] = sqrt of the inverse's diagonal, cond = scaled condition number; with z: du = route 1, r = the discrepancy of route 2, tol =
    10 max(r, 2^-52 cond); with identity: e_ref = the error of the identity sum formed from route 1, tol_identity = 10 max(e_ref, 2^-52 cond))"""
    N, PB = L.shape[0], L.shape[1] - 1
    Ad, Hk = LC.factor_product(L)
    diag, off, _ = CC.dense_inverse(Ad, Hk)
    s = np.sqrt(np.diagonal(diag, axis1=1, axis2=2))
    cond = CC.scaled_condition(Ad, Hk)
    out = dict(Ad=Ad, Hk=Hk, diag=diag, off=off, s=s, cond=cond, PB=PB)
    if z is not None:
        du = solve_dense(L, z)
        r = scaled_error(solve_recurrence(L, z), du, s, z)
        out.update(du=du, r=r, tol=10.0 * max(r, EPS * cond), bound=float((np.abs(du) / (s[None] * np.linalg.norm(z.reshape(z.shape[0], -1), axis=1)[:, None, None])).max()))
    if identity:
        e_ref = CC.scaled_error(*band_of_sum(solve_dense(L, unit_vectors(N)), PB), diag, off)
        out.update(e_ref=e_ref, tol_identity=10.0 * max(e_ref, EPS * cond))
    return out


def normals(seed, K, N):
    """the z of estimator.sample_normals: a function of (seed, K, N) alone"""
    return np.random.default_rng(seed).standard_normal((K, N, NX))


# ---- the retraction: a sample's pose from the estimate and du --------------------------------------------------------------------------------
def moved(oracle, sk, q, du):
    """q [N][nq] with du [N][28] added in the reduced coordinates: 28 successive oracle.move_coordinate calls per frame (the moves add to state
    entries, so they commute)"""
    out = np.array(q, dtype=np.float64, copy=True)
    for n in range(q.shape[0]):
        for k in range(NX):
            out = oracle.move_coordinate(sk, out, n, k, float(du[n, k]))
    return out
