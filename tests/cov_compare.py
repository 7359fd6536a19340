"""Reference side of the posterior-covariance tests (cpe_covariance / cpe_band_inverse, include/cpe.h).  Helper, not a test module.

The matrix: A = H + ridge diag(max(diag H, floor)) as a symmetric block band in lm_compare's form -- diagonal blocks Ad [N][28][28] and the blocks
(m, m - k), k = 1..PB, Hk [N][PB][28][28].  The covariance Sigma = A^-1 is wanted on the same band: diag [N][28][28] = Sigma(n, n) and
off [N][PB][28][28], off[n][i - 1] = Sigma(n + i, n), zero where n + i >= N (cpe_band_inverse's layout).

Two float64 routes to it, both numpy:
  dense      np.linalg.inv of the dense matrix, cut to the band
  takahashi  dense Cholesky factor, put in the L layout of cpe_eval_lm_step, then the block recurrence the HIP sweep runs
             (G_k = L(n+k,n) L(n,n)^-1;  Sigma(n+i,n) = - sum_k Sigma(n+i,n+k) G_k;  Sigma(n,n) = L(n,n)^-T L(n,n)^-1 - sum_k G_k^T Sigma(n+k,n))

Error unit (`scaled_error`): |difference| / sqrt(Sigma_aa Sigma_bb) of the reference, worst over the band.  Residual unit (`residual`): entry (a, b)
of sum_k A(n,k) Sigma(k,n) - I over sqrt(A_aa Sigma_bb), worst over the band's columns -- oracle-free.  Tolerance of a GPU result on a matrix
(`tolerance`): 10 x max(r, 2^-52 x Jacobi-scaled condition number), r = the same measure between the two routes above on that matrix: it is set by
the reference alone, never by the GPU's numbers; the factor 10 covers the different summation order and the different route to L(n,n)^-1.

Worst values measured on an MI355X (tests/test_gpu_covariance.py::test_zz_report; the table is in DESIGN.md 4), error / its tolerance:
  oracle bands, N = 40    6 cameras 5.4e-11 / 4.8e-9, 2 cameras 1.4e-10 / 7.4e-8, 1 camera + priors (PB = 4) at ridge 0 1.7e-7 / 1.9e-5 (scaled
                          condition 8.5e9), at ridge 1e-6 1.2e-10 / 1.2e-8; residual at most 7.4e-12
  random bands            error 4.3e-13 / 4.3e-12 (PB = 4, N = 57), residual at most 2.1e-15
  the two numpy routes    4.7e-11 (6 cameras) and 2.4e-10 (2 cameras) at ridge 0 on the CPU (tests/test_covariance_host.py)
  full path, 6 cameras    factor key 2.7e-10; ||Sigma_o E||_2 7.0e-6; direct difference 3.5e-10, 2.5e-4 of its bound
  marker covariance       3.2e-10 of the block scale, 0.24 of its tolerance
"""
import numpy as np

import lm_compare as LC

NX = LC.NX
EPS = 2.0 ** -52
N_CASE = 40
DENSE_N = 60        # longest sequence that is treated with dense LAPACK routines (np.linalg.inv, every eigenvalue)

_CACHE = {}


# ---- the named cases: synthetic phantom sequences, N = 40, at the oracle's solution ----------------------------------------------
def case_setup(name):
    """(skeleton, cameras, priors, seed) of a named case"""
    from cheetah_pose_estimation_amd import abi, priors, skeleton, synth
    cams6 = synth.make_cameras(6)
    if name in ("six", "n3"):
        return skeleton.build_skeleton("phantom", 25), cams6, None, 11
    if name == "two":
        return skeleton.build_skeleton("phantom", 25), (abi.Camera * 2)(cams6[0], cams6[3]), None, 12
    if name == "mono":
        return skeleton.build_skeleton("phantom", 24), (abi.Camera * 1)(cams6[2]), priors.load_priors(), 13
    if name == "mono_noprior":
        return skeleton.build_skeleton("phantom", 24), (abi.Camera * 1)(cams6[2]), None, 13
    raise KeyError(name)


def oracle_case(oracle, name):
    """dict(sk, cams, opts, priors, q [N, nq] = the oracle's solution, meas, weight, Bk, Hk = the oracle's undamped band there, PB); computed once
    per session and shared -- callers must not modify it.  "n3" = the first 3 frames of "six" at its solution (no motion term)."""
    if name in _CACHE:
        return _CACHE[name]
    from cheetah_pose_estimation_amd import abi, synth
    sk, cams, pr, seed = case_setup(name)
    opts = abi.default_options()
    if name == "n3":
        six = oracle_case(oracle, "six")
        q, meas, weight = six["q"][:3].copy(), six["meas"][:3].copy(), six["weight"][:3].copy()
    else:
        d = synth.make_batch(sk, cams, B=1, N=N_CASE, seed=seed)
        meas, weight = d["meas"][0], d["weight"][0]
        q = oracle.solve(sk, cams, opts, pr, d["q_init"][0], meas, weight)["q"]
    PB = LC.solver_pb(pr)
    _, _, H, _, qc = oracle.objective(sk, cams, opts, pr, q, meas, weight, want_grad=True, want_H=True)
    Bk, Hk = LC._blocks_from_band(H, q.shape[0], PB)
    _CACHE[name] = dict(sk=sk, cams=cams, opts=opts, priors=pr, q=qc, meas=meas, weight=weight, Bk=Bk, Hk=Hk, PB=PB)
    return _CACHE[name]


def damped(Bk, ridge):
    """diagonal blocks of H + ridge diag(max(diag H, floor)) (the floor of cpe_eval_lm_step)"""
    N = Bk.shape[0]
    Ad = Bk.copy()
    idx = np.arange(NX)
    Ad[:, idx, idx] += ridge * np.maximum(np.diagonal(Bk, axis1=1, axis2=2), LC.diag_floor(N))
    return Ad


def random_band(N, PB, seed):
    """a random SPD block band: A = M M^T + I with M a random lower block band of half-bandwidth PB (so A's is PB too), rows scaled over four
    decades as the solver's coordinates are (metres against radians)"""
    rng = np.random.default_rng(seed)
    M = np.zeros((N * NX, N * NX))
    for n in range(N):
        for i in range(min(PB, N - 1 - n) + 1):
            blk = rng.normal(0.0, 1.0, (NX, NX))
            M[(n + i) * NX:(n + i + 1) * NX, n * NX:(n + 1) * NX] = np.tril(blk) + 3.0 * np.eye(NX) if i == 0 else 0.3 * blk
    s = 10.0 ** rng.uniform(-2.0, 2.0, N * NX)
    A = (M @ M.T + np.eye(N * NX)) * s[:, None] * s[None, :]
    return cut_band(A, PB, lower_first=True)


# ---- band <-> dense -------------------------------------------------------------------------------------------------------------------------
def cut_band(S, PB, lower_first=False):
    """the band of a dense symmetric matrix.  lower_first: lm_compare's form (Ad, Hk[m][k-1] = block (m, m - k)); else the covariance
    layout (diag, off[n][i-1] = block (n + i, n))"""
    N = S.shape[0] // NX
    blk = lambda r, c: S[r * NX:(r + 1) * NX, c * NX:(c + 1) * NX]
    diag = np.stack([blk(n, n) for n in range(N)])
    off = np.zeros((N, PB, NX, NX))
    for n in range(N):
        for i in range(1, PB + 1):
            if lower_first and n - i >= 0:
                off[n, i - 1] = blk(n, n - i)
            if not lower_first and n + i < N:
                off[n, i - 1] = blk(n + i, n)
    return diag, off


def dense_inverse(Ad, Hk):
    """route 1: (diag, off) of the dense inverse, and the dense inverse itself.  np.linalg.inv up to DENSE_N frames; for longer sequences (the
    random bands of 200 frames: 5 600 unknowns) every column of the inverse from LAPACK's banded solve of the identity, which keeps a test case
    within seconds"""
    N = Ad.shape[0]
    if N <= DENSE_N:
        S = np.linalg.inv(LC.dense(Ad, Hk))
    else:
        from scipy.linalg import solveh_banded
        S = solveh_banded(LC.to_lapack_lower(Ad, Hk), np.eye(N * NX), lower=True)
    S = 0.5 * (S + S.T)
    return cut_band(S, Hk.shape[1]) + (S,)


def cholesky_layout(Ad, Hk):
    """numpy's dense Cholesky factor of the band in cpe_eval_lm_step's L layout [N][PB + 1][28][28] (true diagonal); raises LinAlgError when
    the matrix is not positive definite"""
    N, PB = Ad.shape[0], Hk.shape[1]
    Lf = np.linalg.cholesky(LC.dense(Ad, Hk))
    L = np.zeros((N, PB + 1, NX, NX))
    for n in range(N):
        for i in range(min(PB, N - 1 - n) + 1):
            L[n, i] = Lf[(n + i) * NX:(n + i + 1) * NX, n * NX:(n + 1) * NX]
    return L


def takahashi(L):
    """route 2: the block recurrence on the factor's blocks.  Returns (diag, off)"""
    N, PB = L.shape[0], L.shape[1] - 1
    diag = np.zeros((N, NX, NX))
    off = np.zeros((N, PB, NX, NX))

    def sig(r, c):                      # Sigma(r, c) for frames inside the band and the sequence, already computed
        if r >= N or c >= N:
            return np.zeros((NX, NX))
        if r == c:
            return diag[r]
        return off[c, r - c - 1] if r > c else off[r, c - r - 1].T

    for n in range(N - 1, -1, -1):
        T = np.linalg.inv(L[n, 0])
        G = [None] + [L[n, k] @ T for k in range(1, PB + 1)]
        for i in range(1, PB + 1):
            if n + i < N:
                off[n, i - 1] = -sum(sig(n + i, n + k) @ G[k] for k in range(1, PB + 1))
        D = T.T @ T - sum(G[k].T @ sig(n + k, n) for k in range(1, PB + 1))
        diag[n] = 0.5 * (D + D.T)
    return diag, off


# ---- measures -------------------------------------------------------------------------------------------------------------------------------
def scaled_error(diag, off, ref_diag, ref_off):
    """worst |difference| / sqrt(Sigma_aa Sigma_bb) of the reference over the band (inf where something is not finite)"""
    N, PB = ref_off.shape[0], ref_off.shape[1]
    s = np.sqrt(np.diagonal(ref_diag, axis1=1, axis2=2))          # [N, 28]
    if not (np.all(np.isfinite(diag)) and np.all(np.isfinite(off))):
        return float("inf")
    worst = float((np.abs(diag - ref_diag) / (s[:, :, None] * s[:, None, :])).max())
    for i in range(1, PB + 1):
        if N - i > 0:
            e = np.abs(off[:N - i, i - 1] - ref_off[:N - i, i - 1]) / (s[i:, :, None] * s[:N - i, None, :])
            worst = max(worst, float(e.max()))
    return worst


def residual(Ad, Hk, diag, off):
    """worst entry of sum_k A(n,k) Sigma(k,n) - I over sqrt(A_aa Sigma_bb), n = 0..N-1 (k over the band of row n of A)"""
    N, PB = Ad.shape[0], Hk.shape[1]
    sa = np.sqrt(np.diagonal(Ad, axis1=1, axis2=2))
    ss = np.sqrt(np.diagonal(diag, axis1=1, axis2=2))
    worst = 0.0
    for n in range(N):
        R = Ad[n] @ diag[n] - np.eye(NX)
        for i in range(1, PB + 1):
            if n + i < N:
                R += Hk[n + i, i - 1].T @ off[n, i - 1]           # A(n, n+i) Sigma(n+i, n)
            if n - i >= 0:
                R += Hk[n, i - 1] @ off[n - i, i - 1].T           # A(n, n-i) Sigma(n-i, n)
        worst = max(worst, float((np.abs(R) / (sa[n][:, None] * ss[n][None, :])).max()))
    return worst


def scaled_condition(Ad, Hk):
    """condition number of the Jacobi-scaled matrix D^-1/2 A D^-1/2 from the extreme eigenvalues of the scaled band"""
    from scipy.linalg import eig_banded
    N, PB = Ad.shape[0], Hk.shape[1]
    d = 1.0 / np.sqrt(np.diagonal(Ad, axis1=1, axis2=2))
    As = Ad * d[:, :, None] * d[:, None, :]
    Hs = np.zeros_like(Hk)
    for k in range(1, min(PB, N - 1) + 1):
        Hs[k:, k - 1] = Hk[k:, k - 1] * d[k:, :, None] * d[:N - k, None, :]
    ab = LC.to_lapack_lower(As, Hs)
    n = N * NX
    if N <= DENSE_N:
        lo = eig_banded(ab, lower=True, eigvals_only=True, select="i", select_range=(0, 0))[0]
        hi = eig_banded(ab, lower=True, eigvals_only=True, select="i", select_range=(n - 1, n - 1))[0]
    else:           # long sequences: Lanczos on the band product, and on the banded solve for the smallest eigenvalue
        from scipy.linalg import cholesky_banded, cho_solve_banded
        from scipy.sparse.linalg import LinearOperator, eigsh
        mv = LinearOperator((n, n), matvec=lambda x: LC.band_matvec(As, Hs, np.asarray(x).reshape(N, NX)).ravel(), dtype=np.float64)
        cb = cholesky_banded(ab, lower=True)
        sv = LinearOperator((n, n), matvec=lambda x: cho_solve_banded((cb, True), np.asarray(x).ravel()), dtype=np.float64)
        hi = eigsh(mv, k=1, which="LA", return_eigenvectors=False)[0]
        lo = 1.0 / eigsh(sv, k=1, which="LA", return_eigenvectors=False)[0]
    return float(hi / lo) if lo > 0 else float("inf")


def reference(Ad, Hk, want_dense=False):
    """both routes on one matrix: dict(diag, off = the dense inverse's band, r_err, r_res = the discrepancy between the routes in the two
    measures, cond = scaled condition number, tol_err, tol_res = 10 max(r, 2^-52 cond), [S = the dense inverse])"""
    d1, o1, S = dense_inverse(Ad, Hk)
    d2, o2 = takahashi(cholesky_layout(Ad, Hk))
    r_err = scaled_error(d2, o2, d1, o1)
    r_res = max(residual(Ad, Hk, d1, o1), residual(Ad, Hk, d2, o2))
    cond = scaled_condition(Ad, Hk)
    out = dict(diag=d1, off=o1, r_err=r_err, r_res=r_res, cond=cond, tol_err=10.0 * max(r_err, EPS * cond), tol_res=10.0 * max(r_res, EPS * cond))
    if want_dense:
        out["S"] = S
    return out


def structure_failures(diag, off, tol):
    """what is wrong with the structure of a covariance band, as a list of strings: diagonal blocks bit-symmetric, positive diagonals, PSD to
    round-off (smallest eigenvalue of the Jacobi-scaled block >= -28 tol), zeros past the end"""
    bad = []
    N, PB = off.shape[0], off.shape[1]
    if not np.array_equal(diag.view(np.int64), np.swapaxes(diag, 1, 2).copy().view(np.int64)):
        bad.append("diagonal blocks not bit-symmetric")
    dd = np.diagonal(diag, axis1=1, axis2=2)
    if not np.all(dd > 0.0):
        bad.append("non-positive variance")
    else:
        s = 1.0 / np.sqrt(dd)
        ev = np.linalg.eigvalsh(diag * s[:, :, None] * s[:, None, :])
        if ev.min() < -NX * tol:
            bad.append(f"diagonal block not PSD: smallest scaled eigenvalue {ev.min():.2e}")
    for i in range(1, PB + 1):
        if off[max(N - i, 0):, i - 1].any():
            bad.append(f"non-zero past the end in off-diagonal block {i}")
    return bad


# ---- marker Jacobians by central differences ------------------------------------------------------------------------------------------------
def marker_jacobians(oracle, sk, q, frames, step):
    """P [len(frames)][L][3][28] = d p_l / d u at the listed frames: central differences of synth.fk_numpy through oracle.move_coordinate"""
    from cheetah_pose_estimation_amd import synth
    out = []
    for n in frames:
        P = np.zeros((sk.n_markers, 3, NX))
        for k in range(NX):
            pp = synth.fk_numpy(sk, oracle.move_coordinate(sk, q, n, k, +step)[n])[0]
            pm = synth.fk_numpy(sk, oracle.move_coordinate(sk, q, n, k, -step)[n])[0]
            P[:, :, k] = (pp - pm) / (2.0 * step)
        out.append(P)
    return np.stack(out)


def marker_covariance(P, diag_blocks):
    """P_l Sigma(n,n) P_l^T for P [F][L][3][28] and the matching diagonal blocks [F][28][28]"""
    return np.einsum("flak,fkj,flbj->flab", P, diag_blocks, P)


def line_of_sight_axes(cam, positions):
    """for marker positions [..., 3]: (a, t1, t2) = the world axis the camera's line of sight to the marker runs along (largest component of
    the unit vector from the camera centre to the marker) and the two other axes"""
    Rc = np.array(cam.R[:]).reshape(3, 3)
    centre = -Rc.T @ np.array(cam.t[:])
    ray = positions - centre
    a = np.argmax(np.abs(ray), axis=-1)
    return a, (a + 1) % 3, (a + 2) % 3


def depth_exceeds_transverse(cam, positions, positions_std):
    """bool [...]: the component of positions_std [..., 3] on the line-of-sight axis exceeds both other components"""
    a, t1, t2 = line_of_sight_axes(cam, positions)
    take = lambda ax: np.take_along_axis(positions_std, ax[..., None], axis=-1)[..., 0]
    return take(a) > np.maximum(take(t1), take(t2))
