"""Entry-by-entry comparison of the first LM iteration of a solve (cpe_eval_lm_step's outputs: gradient, diagonal, Cholesky factor, step,
predicted decrease, trial state) with a reference built from the oracle.  Helper of the tests, not a test module.

The reference system of one sequence, in blocks of the reduced coordinates (28 per frame), PB = the solver's half-bandwidth in frames:

  kinematic model    oracle.objective(want_grad, want_H): g and the lower band, kd = (max(3, W) + 1) 28 - 1, split into the diagonal
                     blocks Bk [N][28][28] and the blocks (m, m - k), k = 1..PB, Hk [N][PB][28][28]
  physics model      oracle.kinetic_system(lam): gk / Bk / Hk after the node forces are eliminated at the damping lam; the third
                     off-diagonal block is zero
  damping            A = H + lam diag(max(diag H, floor)), floor 0.1 for N < 4, else 1e-12 (both solvers)

Every key is one number per sequence, the worst over its entries of |HIP - reference| / scale:

  terms     the five cost terms, HIP's order (meas, model, bound, pose, motion or physics cost)      scale |R|
  g         total gradient                          scale sqrt(2 V D_aa), D = max(diag H, floor), V the objective
  dg        diagonal of H before damping            scale |H_aa|
  factor    L L^T against A over every block of the band, A's diagonal from HIP's dg      scale sqrt(A_ii A_jj)
  solve     backward error of HIP's own L, delta, g: |L L^T d + g| / (|L L^T| |d| + |g|)   (infinity norms; oracle-free)
  step      backward error of HIP's delta in A d = -g of the oracle
  delta     |d - d_ref| / |d_ref| against the oracle's step (scipy.linalg.solveh_banded), asserted only where cond(A) is known and small
  pred      |pred - pred_ref| / (|g|.|d| + |d|^T |H| |d| / 2), pred_ref = -g.d - d^T H d / 2 from the oracle's blocks (math.fsum)
  maxstep   max |d|, bit for bit (0 or inf)
  trial     trial - current = d at the state slot of every reduced coordinate, every other slot unchanged, bit for bit (0 or inf)

Where a scale is exactly zero the compared value must be exactly zero.  Structural zeros of the factor (blocks past the sequence end, the
upper triangle of its diagonal blocks) must be exactly zero and every pivot positive, or `factor` is inf.
"""
import math

import numpy as np

NX = 28
KEYS = ("terms", "g", "dg", "factor", "solve", "step", "delta", "pred", "maxstep", "trial")

# Tolerances of the GPU-vs-oracle comparison (tests/test_gpu_lm_step.py), per key, in the units above: about 10 x the worst value measured on
# an MI355X over every case of that module (printed by its test_zz_report).
# terms 1.3e-14, g 3.0e-10, dg 5.1e-9, factor 4.8e-9, solve 2.2e-16, step 1.5e-10, delta 1.4e-10 (where asserted), pred 4.0e-11.  g, dg, factor and
# step carry the per-frame kernel's rounding against the oracle's (the largest at N = 1000 with both priors); solve is HIP's own and sits at
# round-off.  maxstep and trial are exact.
TOL = dict(terms=1.5e-13, g=3e-9, dg=5e-8, factor=5e-8, solve=2e-15, step=1.5e-9, delta=1.5e-9, pred=4e-10, maxstep=0.0, trial=0.0)
# delta is compared with the oracle's step only where the damped matrix is this well conditioned (dense condition number, N <= COND_N)
COND_ASSERT, COND_N = 1e7, 40


def diag_floor(N):
    return 0.1 if N < 4 else 1e-12


def hip_terms_kinematic(terms):
    """the oracle's terms (meas, model, pose, motion, bound) in HIP's order (meas, model, bound, pose, motion)"""
    return np.array([terms[0], terms[1], terms[4], terms[2], terms[3]])


def _blocks_from_band(H, N, PB):
    """the lower band of the oracle (H[i, i - j] = A(i, j), j <= i) as Bk [N][28][28] (symmetric) and Hk [N][PB][28][28] (block (m, m - k))"""
    kd = H.shape[1] - 1
    Bk = np.zeros((N, NX, NX))
    Hk = np.zeros((N, PB, NX, NX))
    rows = H.reshape(N, NX, kd + 1)
    for a in range(NX):
        for c in range(a + 1):
            Bk[:, a, c] = Bk[:, c, a] = rows[:, a, a - c]
        for k in range(1, PB + 1):
            for c in range(NX):
                d = k * NX + a - c
                if d <= kd:
                    Hk[k:, k - 1, a, c] = rows[k:, a, d]
    return Bk, Hk


def reference(oracle, sk, cams, opts, priors, q, meas, weight, lam, PB, kopts=None, stance=None):
    """the oracle's system of one sequence at damping lam: dict g [N, 28], Bk, Hk [N, PB, 28, 28], Ad (damped diagonal blocks), D (the
    damping's diagonal), V, terms (HIP's order), delta (the oracle's step), q (the consistent Euler q)"""
    N = q.shape[0]
    if kopts is None:
        V, g, H, terms, qc = oracle.objective(sk, cams, opts, priors, q, meas, weight, want_grad=True, want_H=True)
        Bk, Hk = _blocks_from_band(H, N, PB)
        g = g.reshape(N, NX)
        terms = hip_terms_kinematic(terms)
    else:
        R = oracle.kinetic_system(sk, cams, opts, priors, kopts, q, meas, weight, stance, lam=lam)
        V, _, qc, t8, _ = oracle.kinetic_objective(sk, cams, opts, priors, kopts, q, meas, weight, stance, want_grad=False)
        g, Bk = R["gk"], R["Bk"]
        Hk = np.zeros((N, PB, NX, NX))
        Hk[:, :2] = R["Hk"]
        kin = kopts.w_torque * t8[4] + kopts.w_smooth * t8[5] + kopts.w_slack * t8[6]
        model = 0.0 if not any(sk.motion_w[p] for p in range(sk.nq)) else t8[1] - kin
        terms = np.array([t8[0], model, t8[3], t8[2], kin])
    dH = np.diagonal(Bk, axis1=1, axis2=2)
    D = np.maximum(dH, diag_floor(N))
    Ad = Bk.copy()
    idx = np.arange(NX)
    Ad[:, idx, idx] += lam * D
    R = dict(g=g, Bk=Bk, Hk=Hk, Ad=Ad, D=D, V=float(V), terms=terms, q=qc, lam=lam)
    R["delta"] = band_solve(Ad, Hk, -g)
    return R


# ---- band algebra in blocks ------------------------------------------------------------------------------------------------------------
def band_matvec(Ad, Hk, x):
    """A x for the symmetric block band (diagonal blocks Ad [N], blocks (m, m - k) Hk [N][PB]), x [N, 28]"""
    y = np.einsum("nab,nb->na", Ad, x)
    for k in range(1, Hk.shape[1] + 1):
        Hb = Hk[k:, k - 1]
        y[k:] += np.einsum("nab,nb->na", Hb, x[:-k])
        y[:-k] += np.einsum("nba,nb->na", Hb, x[k:])
    return y


def band_abs_rowsum(Ad, Hk):
    """row sums of |A| (the infinity norm is their maximum)"""
    s = np.abs(Ad).sum(axis=2)
    for k in range(1, Hk.shape[1] + 1):
        Hb = np.abs(Hk[k:, k - 1])
        s[k:] += Hb.sum(axis=2)
        s[:-k] += Hb.sum(axis=1)
    return s


def to_lapack_lower(Ad, Hk):
    """scipy.linalg.solveh_banded's lower form: ab[i - j, j] = A(i, j)"""
    N, PB = Ad.shape[0], Hk.shape[1]
    kd = (PB + 1) * NX - 1
    ab = np.zeros((kd + 1, N * NX))
    for a in range(NX):
        for c in range(a + 1):
            ab[a - c, c::NX][:N] = Ad[:, a, c]
        for k in range(1, PB + 1):
            for c in range(NX):
                d = k * NX + a - c
                if d <= kd and k < N:
                    ab[d, c::NX][:N - k] = Hk[k:, k - 1, a, c]
    return ab


def band_solve(Ad, Hk, rhs):
    from scipy.linalg import solveh_banded
    x = solveh_banded(to_lapack_lower(Ad, Hk), rhs.reshape(-1), lower=True)
    return x.reshape(rhs.shape)


def dense(Ad, Hk):
    N = Ad.shape[0]
    A = np.zeros((N * NX, N * NX))
    for m in range(N):
        A[m * NX:(m + 1) * NX, m * NX:(m + 1) * NX] = Ad[m]
        for k in range(1, Hk.shape[1] + 1):
            if m - k >= 0:
                A[m * NX:(m + 1) * NX, (m - k) * NX:(m - k + 1) * NX] = Hk[m, k - 1]
                A[(m - k) * NX:(m - k + 1) * NX, m * NX:(m + 1) * NX] = Hk[m, k - 1].T
    return A


def factor_product(L):
    """L L^T in blocks from the factor in cpe_eval_lm_step's form (L[n][i] = block (n + i, n)): diagonal blocks Md [N] and blocks (m, m - k)
    Mk [N][PB] (Mk[m][k - 1] = 0 for m < k)"""
    N, P1 = L.shape[0], L.shape[1]
    PB = P1 - 1
    Md = np.zeros((N, NX, NX))
    Mk = np.zeros((N, PB, NX, NX))
    for d in range(min(P1, N)):             # row frame m = j + d
        for k in range(d + 1):              # (m, m - k): sum over columns j of L(m, j) L(m - k, j)^T, j = m - d
            Lm = L[:N - d, d]               # L(j + d, j) for j = 0 .. N - 1 - d
            Lk = L[:N - d, d - k]           # L(j + d - k, j)
            P = np.einsum("jac,jbc->jab", Lm, Lk)
            if k == 0:
                Md[d:] += P
            else:
                Mk[d:, k - 1] += P
    return Md, Mk


def factor_apply(L, x):
    """L L^T x from the factor's blocks"""
    N, P1 = L.shape[0], L.shape[1]
    y = np.einsum("nca,nc->na", L[:, 0], x)                 # y = L^T x: y_n = sum_i L(n + i, n)^T x_{n + i}
    for i in range(1, min(P1, N)):
        y[:N - i] += np.einsum("nca,nc->na", L[:N - i, i], x[i:])
    z = np.einsum("nac,nc->na", L[:, 0], y)                 # z = L y: z_m = sum_i L(m, m - i) y_{m - i}
    for i in range(1, min(P1, N)):
        z[i:] += np.einsum("nac,nc->na", L[:N - i, i], y[:N - i])
    return z


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def _ratio(G, R, scale):
    """worst |G - R| / scale, inf where the scale is zero and G != R (or where G is not finite)"""
    G = np.asarray(G, dtype=np.float64)
    d = np.abs(G - R)
    if not np.all(np.isfinite(d)):
        return float("inf")
    scale = np.broadcast_to(scale, d.shape)
    zero = scale == 0.0
    if np.any(d[zero] != 0.0):
        return float("inf")
    return float((d[~zero] / scale[~zero]).max(initial=0.0))


def coordinate_slots(sk):
    """state slot of every reduced coordinate: the Euler angle of a trunk coordinate, nq + r for the rotation of leg link r"""
    from cheetah_pose_estimation_amd import abi, skeleton
    ind = [int(p) for p in skeleton.independent_dofs(sk)]
    assert len(ind) == NX
    slot = list(ind)
    r = 0
    for j in range(sk.n_joints):
        if sk.joint_kind[j] == abi.JOINT_REVOLUTE_Y:
            slot[ind.index(3 + 3 * sk.joint_child[j] + 1)] = sk.nq + r
            r += 1
    return np.array(slot)


def _backward_error(r, Anorm, dnorm, gnorm):
    den = Anorm * dnorm + gnorm
    return float(np.abs(r).max() / den) if den > 0 else (0.0 if not np.abs(r).any() else float("inf"))


def discrepancies(G, R, slots, cond=None):
    """worst value of every key for one sequence: G = cpe_eval_lm_step's outputs of it (g, dg, delta [N, 28], L [N, PB + 1, 28, 28], state
    [N, 2, ns], seq [8]), R = reference(...); cond: the dense condition number of A, if known"""
    N = R["g"].shape[0]
    out = {}
    out["terms"] = _ratio(G["seq"][:5], R["terms"], np.abs(R["terms"]))
    out["g"] = _ratio(G["g"], R["g"], np.sqrt(2.0 * max(R["V"], 0.0) * R["D"]))
    dH = np.diagonal(R["Bk"], axis1=1, axis2=2)
    out["dg"] = _ratio(G["dg"], dH, np.abs(dH))
    # factor: structure, pivots, then L L^T against A
    L = np.asarray(G["L"], dtype=np.float64)
    P1 = L.shape[1]
    ok = np.all(np.isfinite(L)) and np.all(np.diagonal(L[:, 0], axis1=1, axis2=2) > 0.0) and not np.triu(L[:, 0], 1).any()
    for i in range(1, P1):
        ok = ok and not L[max(N - i, 0):, i].any()
    if ok:
        # the matrix HIP factored has HIP's own diagonal, which `dg` holds against the oracle: L L^T is compared with the oracle's blocks with
        # that diagonal, damped here (so that the rounding of the per-frame kernel's diagonal does not set the level of this key)
        Md, Mk = factor_product(L)
        dgh = np.asarray(G["dg"], dtype=np.float64)
        Ah = R["Ad"].copy()
        idx = np.arange(NX)
        Ah[:, idx, idx] = dgh + R["lam"] * np.maximum(dgh, diag_floor(N))
        dA = np.diagonal(R["Ad"], axis1=1, axis2=2)                        # [N, 28], positive (damped with a floor)
        sd = np.sqrt(dA[:, :, None] * dA[:, None, :])
        sk = np.zeros_like(Mk)
        for k in range(1, min(P1, N)):
            sk[k:, k - 1] = np.sqrt(dA[k:, :, None] * dA[:N - k, None, :])
        out["factor"] = max(_ratio(Md, Ah, sd), _ratio(Mk, R["Hk"], sk))
    else:
        out["factor"] = float("inf")
    d, g = np.asarray(G["delta"], dtype=np.float64), np.asarray(G["g"], dtype=np.float64)
    dn, gn = np.abs(d).max(), np.abs(g).max()
    if ok:
        out["solve"] = _backward_error(factor_apply(L, d) + g, band_abs_rowsum(Md, Mk).max(), dn, gn)
    else:
        out["solve"] = float("inf")
    out["step"] = _backward_error(band_matvec(R["Ad"], R["Hk"], d) + R["g"], band_abs_rowsum(R["Ad"], R["Hk"]).max(), dn, np.abs(R["g"]).max())
    dr = R["delta"]
    out["delta"] = float(np.abs(d - dr).max() / np.abs(dr).max()) if np.abs(dr).max() > 0 else (0.0 if not d.any() else float("inf"))
    # predicted decrease from the oracle's (undamped) blocks
    Hd = band_matvec(R["Bk"], R["Hk"], d)
    Habs = band_matvec(np.abs(R["Bk"]), np.abs(R["Hk"]), np.abs(d))
    pr = -math.fsum((R["g"] * d).ravel()) - 0.5 * math.fsum((d * Hd).ravel())
    ps = math.fsum(np.abs(R["g"] * d).ravel()) + 0.5 * math.fsum((np.abs(d) * Habs).ravel())
    out["pred"] = _ratio(G["seq"][5], pr, ps)
    out["maxstep"] = 0.0 if G["seq"][6] == np.abs(d).max() else float("inf")
    # trial iterate: current + delta at the coordinates' slots, bit for bit; every other slot unchanged
    st = np.asarray(G["state"], dtype=np.float64)
    cur, tri = st[:, 0], st[:, 1]
    want = cur.copy()
    want[:, slots] = cur[:, slots] + d
    out["trial"] = 0.0 if np.array_equal(tri.view(np.int64), want.view(np.int64)) else float("inf")
    if cond is not None:
        out["cond"] = cond
    return out


def condition(R):
    """dense condition number of the damped matrix (N <= COND_N), else None"""
    N = R["g"].shape[0]
    return float(np.linalg.cond(dense(R["Ad"], R["Hk"]))) if N <= COND_N else None


def failures(d, tol=None, only=None):
    """the keys of a discrepancy dict beyond their tolerance (delta only where the condition number allows it); only: the keys to assert"""
    tol = tol or TOL
    keys = only or KEYS
    bad = {}
    for k in keys:
        if k == "delta" and not (d.get("cond") is not None and d["cond"] <= COND_ASSERT):
            continue
        if not d[k] <= tol[k]:
            bad[k] = d[k]
    return bad


# ---- a reference of the HIP outputs, built on the CPU (tests/test_lm_compare.py) -------------------------------------------------------
def reference_outputs(R, state_cur, slots):
    """what cpe_eval_lm_step should return for the reference R, computed with numpy: dense Cholesky of A (N small), its step, the predicted
    decrease of k_lm_back's formula and the trial state from the current state [N, ns]"""
    N, PB = R["g"].shape[0], R["Hk"].shape[1]
    A = dense(R["Ad"], R["Hk"])
    Lf = np.linalg.cholesky(A)
    L = np.zeros((N, PB + 1, NX, NX))
    for n in range(N):
        for i in range(PB + 1):
            if n + i < N:
                L[n, i] = Lf[(n + i) * NX:(n + i + 1) * NX, n * NX:(n + 1) * NX]
    d = np.linalg.solve(A, -R["g"].ravel()).reshape(N, NX)
    pred = -0.5 * float(R["g"].ravel() @ d.ravel()) + 0.5 * R["lam"] * float((R["D"] * d * d).sum())
    st = np.stack([state_cur, state_cur], axis=1).copy()
    st[:, 1, slots] = state_cur[:, slots] + d
    seq = np.concatenate([R["terms"], [pred, np.abs(d).max(), 0.0]])
    return dict(g=R["g"].copy(), dg=np.diagonal(R["Bk"], axis1=1, axis2=2).copy(), L=L, delta=d, state=st, seq=seq)


def truncated_prior(W):
    """the packaged motion prior cut to its last W lags (coefficients of x_{n-W} .. x_{n-1}; intercept and weights unchanged), pose prior off:
    a motion prior of window W < 4 that needs no fit"""
    from cheetah_pose_estimation_amd import abi, priors
    pr = priors.load_priors(pose=False)
    assert pr.lr_window == 4 and 1 <= W <= 4
    coef = np.array([[pr.lr_coef[p][j] for j in range(4 * NX)] for p in range(NX)])
    keep = coef[:, (4 - W) * NX:]
    pr.lr_window = W
    for p in range(NX):
        for j in range(abi.MAX_WINDOW * NX):
            pr.lr_coef[p][j] = keep[p, j] if j < W * NX else 0.0
    return pr


def solver_pb(priors):
    """half-bandwidth of the solver's band in frames for these priors (3, or a longer motion prior's window)"""
    return max(3, priors.lr_window) if priors is not None else 3
