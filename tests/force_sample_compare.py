"""Reference side of the tests of the node-force draws (cpe_force_samples, include/cpe.h; DESIGN.md 2b "What is sampled (forces)").  Helper, not a
test module; numpy and scipy only (no GPU).

A node n >= 2 has na free forces, H_fu [na][84] (columns: the coordinates of the frames n, n-1, n-2) and its force matrix M [na][na] = C C^T.
A draw:  df = C^-T (zeta - Y w),  Y = C^-1 H_fu,  w = (du_n, du_{n-1}, du_{n-2}) [84],  zeta [na].

Two float64 routes to df, both from (H_fu, M, w, zeta):
  route 1   scipy.linalg.cholesky + solve_triangular
  route 2   the same recurrence (Cholesky by columns, forward substitution for Y, back substitution for df) in np.longdouble

Error unit (`scaled_error`): |df_a - ref_a| / (sqrt(cov_f_aa) ||(zeta_n, z)||_2), z the whole trajectory's normals behind du (L^T du = z), cov_f
the reference's M^-1 + S W S^T.  Row a of [C^-T, -S P L^-T] (P picks the node's window) has squared norm cov_f_aa, so
|df_a| <= sqrt(cov_f_aa) ||(zeta_n, z)|| holds exactly and the unit is scale-free across torques, constraint forces and foot forces.
Tolerance of a GPU result (`reference`): kinetic_cov_compare's rule, 10 x max(r, 2^-52 x scaled condition of M), r = the same measure between the
two routes: set by the reference alone, never by GPU numbers; the factor 10 covers the different summation order, as in sample_compare.

Joint identity (`joint_samples`): with the unit vectors of (z, every node's zeta) as samples, sum_s x_s x_s^T over x = (du, df of all nodes) is the
inverse of kinetic_cov_compare.joint_matrix -- every block of it: Sigma, cov_f(n), force-coordinate, and force-force between different nodes.

Measured on the CPU (tests/test_force_samples_host.py), 12-frame gallop at the oracle's solution, ridge 0, 852 unit-vector samples: the joint
identity against the inverse of the joint matrix, worst entry per kind of block -- Sigma 3.0e-9, force-coordinate 9.7e-10, cov_f 2.8e-10, force-force
between different nodes 1.8e-10 against kinetic_cov_compare.reference's tolerance 1.4e-5 (2 cameras); 7.4e-9, 1.5e-9, 6.8e-10, 1.9e-10 against
5.1e-6 (6 cameras).  Largest force-force correlation between the nodes n and n + 1: 0.41 (2 cameras) and 0.46 (6 cameras); between n and n + 5:
0.039 and 0.043.  The two routes on node 6 with 7 random draws: r = 1.2e-14 / 1.0e-14 at a scaled condition of M of 2.2e2 (2^-52 x that: 4.9e-14,
which sets the tolerance 4.9e-13); largest |df_a| in the unit 0.14 (the exact inequality keeps it <= 1).

Identity with cov_f (the GPU test holds M^-1 from the zeta unit vectors and -S from the window unit steps, as M^-1 + S W S^T, against
cpe_covariance_kinetic's cov_f).  At ridge 0 its tolerance is kinetic_cov_compare.kernel_tolerance's on the HIP path's own H_fu / H_ff.  At ridge
1e-6 the library's M holds the wall term and is not available outside it, and 10 x 2^-52 x the scaled condition of M alone is below what float64
leaves of the identity in numpy itself (S W S^T and Y W Y^T have entries orders of magnitude above the result): so the tolerance there is
kinetic_cov_compare's rule, 10 x max(r, 2^-52 x cond), with r = `identity_error` at the node on the ORACLE's system at that ridge -- CPU numbers only.
The identity has two sides and r is the larger of both: the draws' side (route 1's draws in place of the kernel's, against the solve-based local
formula) and cov_f's side (the Cholesky-based local formula, k_force_cov's order of operations, against the solve-based one: kernel_tolerance's r,
which is what the ridge-0 bound is made of).  The oracle's M at ridge 1e-6 is H_ff + ridge lm_force_damping diag H_ff WITHOUT the wall term: r is the
rounding of the same formulas on a matrix of the same size and conditioning (scaled condition 75 - 1050 either way), not of the library's own M.
Measured in numpy per node (tests/test_force_samples_host.py::test_identity_in_numpy): "base" 1.8e-12 .. 6.0e-11 at ridge 0 and 3.9e-13 .. 1.4e-11
at ridge 1e-6; "boxed" 2.5e-12 .. 3.2e-11 and 1.5e-12 .. 3.5e-11 -- above 10 x 2^-52 x cond (1.7e-13 .. 2.3e-12) at 8 - 10 of the 10 nodes.

Worst values measured on an MI355X (tests/test_gpu_force_samples.py::test_zz_report; the table is in DESIGN.md 4), error / its tolerance:
  kernel, S = 65      base 2.9e-14 / 4.0e-13, six 1.3e-13 / 1.6e-12, flight 2.7e-14 / 4.0e-13, fixed 2.4e-14 / 4.0e-13, boxed 2.4e-14 / 3.0e-13,
                      fixed at ridge 1e-6 1.4e-14 / 2.9e-13
  identity, ridge 0   base 1.5e-10 / 1.8e-10, boxed 1.1e-11 / 4.5e-11 (k_force_cov's own error against its numpy r: the same figures as its kernel test)
  identity, ridge 1e-6  base 7.8e-12 / 9.5e-12, boxed 7.1e-12 / 1.2e-11 (the node with the largest error / tolerance)
  joint path, base    Sigma 3.5e-9, force-coordinate 8.2e-10, cov_f 1.0e-9, force-force between nodes 3.1e-10 / 2.0e-5
"""
import numpy as np

import cov_compare as CC
import kinetic_cov_compare as KV
import lm_compare as LC

NX = CC.NX
EPS = CC.EPS
CHUNK = 256            # samples per workgroup pass of k_force_sample (FS_CHUNK, csrc/cpe_force_sample.hip.inc)


def window_steps(du, n):
    """w [S][84] of node n from du [S][N][28]: the frames (n, n-1, n-2), H_fu's column order"""
    return np.concatenate([du[:, n - p] for p in range(3)], axis=1)


def df_scipy(Hfu, M, w, zeta):
    """route 1: df [S][na] from w [S][84], zeta [S][na]"""
    from scipy.linalg import cholesky, solve_triangular
    C = cholesky(M, lower=True)
    Y = solve_triangular(C, Hfu, lower=True)
    return np.ascontiguousarray(solve_triangular(C, zeta.T - Y @ w.T, lower=True, trans="T").T)


def df_recurrence(Hfu, M, w, zeta):
    """route 2: the same recurrence in np.longdouble; rounded to float64 at the end"""
    Ml, Hl, wl, zl = (np.asarray(a, dtype=np.longdouble) for a in (M, Hfu, w, zeta))
    na = M.shape[0]
    C = np.zeros((na, na), np.longdouble)
    for j in range(na):
        C[j, j] = np.sqrt(Ml[j, j] - C[j, :j] @ C[j, :j])
        C[j + 1:, j] = (Ml[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    Y = np.zeros(Hl.shape, np.longdouble)
    for i in range(na):
        Y[i] = (Hl[i] - C[i, :i] @ Y[:i]) / C[i, i]
    t = zl.T - Y @ wl.T
    x = np.zeros(t.shape, np.longdouble)
    for m in range(na - 1, -1, -1):
        x[m] = (t[m] - C[m + 1:, m] @ x[m + 1:]) / C[m, m]
    return np.ascontiguousarray(x.T).astype(np.float64)


def sample_norms(z, zeta_n=None):
    """||(zeta_n, z)||_2 per sample: z [S][N][28], zeta_n [S][na] or None (zeros)"""
    q = (z.reshape(z.shape[0], -1) ** 2).sum(axis=1)
    if zeta_n is not None:
        q = q + (zeta_n ** 2).sum(axis=1)
    return np.sqrt(q)


def scaled_error(df, ref, cov_f, norms):
    """worst |df - ref| / (sqrt(cov_f_aa) norm_s): df, ref [S][na], norms [S] (inf where df is not finite; a sample of norm 0 must agree exactly)"""
    if not np.all(np.isfinite(df)):
        return float("inf")
    s = np.sqrt(np.diag(cov_f))
    live = norms > 0.0
    if np.any(df[~live] != ref[~live]):
        return float("inf")
    if not live.any():
        return 0.0
    return float((np.abs(df[live] - ref[live]) / (s[None] * norms[live][:, None])).max())


def reference(Hfu, M, W, w, zeta, norms):
    """both routes on one node: dict(df = route 1, cov_f = M^-1 + S W S^T (the solve-based local formula), r = the discrepancy of route 2, cond = the
    scaled condition of M, tol = 10 max(r, 2^-52 cond), bound = the largest |df_a| / (sqrt(cov_f_aa) norm), which the exact inequality keeps <= 1)"""
    df = df_scipy(Hfu, M, w, zeta)
    cov_f = KV.local_formula(Hfu, M, W)
    r, cond = scaled_error(df_recurrence(Hfu, M, w, zeta), df, cov_f, norms), KV.scaled_condition(M)
    return dict(df=df, cov_f=cov_f, r=r, cond=cond, tol=10.0 * max(r, EPS * cond), bound=scaled_error(df, np.zeros_like(df), cov_f, norms))


def dense_sigma(L):
    """Sigma dense from a factor L [N][PB + 1][28][28] in cpe_band_inverse's layout: the dense inverse of L L^T"""
    return CC.dense_inverse(*LC.factor_product(L))[2]


def unit_samples(N, counts):
    """the unit vectors of (z, every node's zeta): z [S][N][28], zeta [S][N][64], S = 28 N + sum of counts; counts {n: na}.  Sample 28 N + k is the
    k-th free force in the order of the nodes, as kinetic_cov_compare.joint_matrix lays them out."""
    S = N * NX + sum(counts.values())
    z, zeta = np.zeros((S, N, NX)), np.zeros((S, N, 64))
    z[:N * NX] = np.eye(N * NX).reshape(N * NX, N, NX)
    s = N * NX
    for n in sorted(counts):
        for a in range(counts[n]):
            zeta[s, n, a] = 1.0
            s += 1
    return z, zeta


def joint_sum(du, df):
    """sum_s x_s x_s^T, x = (du [S][N][28], df {n: [S][na]} in the order of the nodes): joint_matrix's layout"""
    X = np.concatenate([du.reshape(du.shape[0], -1)] + [df[n] for n in sorted(df)], axis=1)
    return X.T @ X


def joint_samples(Ad, Hk, nodes):
    """the joint identity by the reference's own route 1: (sum_s x_s x_s^T, the offsets of the nodes in it)"""
    from scipy.linalg import solve_triangular
    N = Ad.shape[0]
    z, zeta = unit_samples(N, {n: nodes[n][0].shape[0] for n in nodes})
    Ld = np.linalg.cholesky(LC.dense(Ad, Hk))
    du = np.ascontiguousarray(solve_triangular(Ld.T, z.reshape(z.shape[0], -1).T, lower=False).T).reshape(z.shape)
    df = {n: df_scipy(Hfu, M, window_steps(du, n), zeta[:, n, :M.shape[0]]) for n, (Hfu, M) in nodes.items()}
    return joint_sum(du, df), KV.joint_matrix(Ad, Hk, nodes)[1]


def block_errors(X, ref, offs, nodes, N):
    """kinetic_cov_compare's scaled unit |difference| / sqrt(ref_aa ref_bb), worst entry per kind of block: dict(sigma, cov_f, force_coordinate,
    force_force = between different nodes)"""
    if not np.all(np.isfinite(X)):
        return dict(sigma=float("inf"), cov_f=float("inf"), force_coordinate=float("inf"), force_force=float("inf"))
    s = np.sqrt(np.diag(ref))
    E = np.abs(X - ref) / (s[:, None] * s[None, :])
    nu = N * NX
    kind = np.full(ref.shape[0], -1)
    for n, o in offs.items():
        kind[o:o + nodes[n][0].shape[0]] = n
    ff = E[nu:, nu:]
    same = kind[nu:, None] == kind[None, nu:]
    return dict(sigma=float(E[:nu, :nu].max()), force_coordinate=float(E[nu:, :nu].max()), cov_f=float(ff[same].max()),
                force_force=float(ff[~same].max()))


def cross_correlation(ref, offs, nodes, gap):
    """largest |correlation| between a force of node n and a force of node n + gap in the joint covariance ref"""
    s = np.sqrt(np.diag(ref))
    R = np.abs(ref) / (s[:, None] * s[None, :])
    worst = 0.0
    for n, o in offs.items():
        if n + gap in offs:
            p = offs[n + gap]
            worst = max(worst, float(R[o:o + nodes[n][0].shape[0], p:p + nodes[n + gap][0].shape[0]].max()))
    return worst


def identity_cov_f(Minv_rows, S_cols, W):
    """cov_f = sum df df^T + S W S^T from the draws of the identity test: Minv_rows [na][na] (row a: df of zeta = e_a, du = 0, i.e. C^-T e_a) and
    S_cols [84][na] (row u: df of du = the window unit step u, zeta = 0, i.e. -S[:, u]); symmetrised"""
    Sn = -S_cols.T
    C = Minv_rows.T @ Minv_rows + Sn @ W @ Sn.T
    return 0.5 * (C + C.T)


def identity_error(Hfu, M, W):
    """the identity of the GPU test run in numpy, both of its sides: (r, the scaled condition of M), r = the larger of
      the draws' side   M^-1 + S W S^T built from route 1's draws (in place of the kernel's) against the solve-based local formula, and
      cov_f's side      the Cholesky-based local formula -- the order of operations of k_force_cov, whose cov_f the identity is held against --
                        against the solve-based one (kinetic_cov_compare.kernel_tolerance's r)
    in kinetic_cov_compare's unit.  What float64 leaves of the identity on the CPU: S W S^T and Y W Y^T have entries orders of magnitude above the
    result."""
    na = M.shape[0]
    rows = df_scipy(Hfu, M, np.zeros((na, 84)), np.eye(na))
    cols = df_scipy(Hfu, M, np.eye(84), np.zeros((84, na)))
    ref, _, r_cov, cond = KV.kernel_tolerance(Hfu, M, W)
    return max(KV.scaled_difference(identity_cov_f(rows, cols, W), ref), r_cov), cond


def compact(f_s, f, meta, n):
    """df [S][na] of node n in the compact order of meta from f_s [S][N][64], f [N][64], meta [N][65]"""
    na = int(meta[n, 0])
    idx = np.asarray(meta[n, 1:1 + na], dtype=np.int64)
    return np.ascontiguousarray(f_s[:, n, idx] - f[n, idx][None])
