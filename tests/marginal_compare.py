"""Reference side of the length-marginal tests (cpe_scale_response, cpe_covariance_add_scales, include/cpe.h; DESIGN.md 2 "What is marginalised").
Helper, not a test module.  Everything is built from what exists: scale_compare.case_inputs / frame_terms / band_with_frames give the dense damped
matrix Hd, the borders E_n and A; scale_compare.position_derivatives gives Ds = d p / d s at fixed poses; cov_compare.marker_jacobians gives
P = d p / d u (central differences at two steps h and 2 h, extrapolated: (4 P_h - P_2h) / 3).  With Pm = I / PRIOR_SIGMA^2, per sequence, two routes:

  dense   the inverse of the joint matrix K = [[Hd, E], [E^T, A + Pm]]: its (u, u) block is the marginal covariance, its (s, s) block cov_s, and
          R = du / ds = (u, s) (s, s)^-1 = -Hd^-1 E
  schur   scipy Cholesky of Hd: Sigma = Hd^-1, R = -Hd^-1 E, cov_s = (A - E^T Hd^-1 E + Pm)^-1, marginal = Sigma + R cov_s R^T

and for both W_l = Ds_l + P_l R_n, cov(p_l) = P_l Sigma(n,n) P_l^T + W_l cov_s W_l^T.  The two routes take P at different step pairs, so their
distance holds the difference quotient's own error.  A scale no marker depends on (E column and A_gg exactly zero) has R and W columns set to
exactly zero -- what the formulas give in exact arithmetic.

Units of discrepancies(G, R), worst over frames and entries, inf for a non-finite value, and where a unit is exactly zero the value must be equal:
  resp_u    sqrt(Sigma_kk(n) A_gg): a Cauchy-Schwarz bound of the entry (E^T Hd^-1 E <= A)
  resp_pos  |Ds| + sum_k |P_lak| x (resp_u's unit)
  band      cov_compare.scaled_error of cov_diag_m / cov_off_m against the reference marginal's own diagonal
  cov_pos   sqrt(ref_aa ref_bb) of the reference's marginal marker block
  sym       cov_diag_m and cov_pos_m against their transposes: 0 or inf

Tolerances, by scale_compare's rule: tolerance(case)[key] = MARGIN (32) x the larger of two numbers measured ON THE CPU on that case's inputs
(MEASURED below; `python -m tests.marginal_compare` prints it; tests/test_marginal_lengths_host.py re-measures two cases); nothing of the kernels'
output enters them:
  1  route schur on the float64 frame terms against route dense on the np.longdouble ones
  2  the float64 route dense at q against itself at q moved by one ulp per entry
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cov_compare as CC                                                            # noqa: E402
import frame_compare as FC                                                          # noqa: E402
import lm_compare as LC                                                             # noqa: E402
import scale_compare as SC                                                          # noqa: E402

NX = SC.NX
MARGIN = SC.MARGIN
PRIOR_SIGMA = 0.1
KEYS = ("resp_u", "resp_pos", "band", "cov_pos", "sym")
MEASURED_KEYS = ("resp_u", "resp_pos", "band", "cov_pos")
P_STEPS = dict(dense=(2e-3, 1e-3), schur=(1e-3, 5e-4))
CASES = ("plain", "n1", "n2", "ragged", "g1", "g16", "prior", "cams1", "batch3")

# per case and key the larger of (measurement 1, measurement 2): CPU only, see the module docstring (`python -m tests.marginal_compare` prints this)
MEASURED = {
    'plain': dict(resp_u=1.22e-11, resp_pos=7.57e-12, band=8.65e-11, cov_pos=5.38e-11),
    'n1': dict(resp_u=2.43e-14, resp_pos=5.21e-13, band=6.48e-14, cov_pos=4.21e-12),
    'n2': dict(resp_u=2.84e-12, resp_pos=2.83e-12, band=1.78e-10, cov_pos=2.39e-10),
    'ragged': dict(resp_u=6.00e-12, resp_pos=3.81e-12, band=2.66e-10, cov_pos=2.85e-10),
    'g1': dict(resp_u=3.40e-12, resp_pos=2.30e-12, band=2.85e-11, cov_pos=1.90e-11),
    'g16': dict(resp_u=1.12e-11, resp_pos=9.00e-12, band=7.05e-11, cov_pos=4.59e-11),
    'prior': dict(resp_u=6.14e-12, resp_pos=3.44e-12, band=6.32e-11, cov_pos=2.21e-11),
    'cams1': dict(resp_u=2.21e-11, resp_pos=1.21e-11, band=3.53e-10, cov_pos=3.67e-10),
    'batch3': dict(resp_u=3.98e-12, resp_pos=2.42e-12, band=3.77e-11, cov_pos=3.20e-11),
}


def tolerance(name):
    """TOL of a case: MARGIN x the reference's own spread on that case's inputs; sym is exact"""
    return dict({k: MARGIN * v for k, v in MEASURED[name].items()}, sym=0.0)


def marker_jacobians(oracle, sk, qc, steps):
    """P [N, L, 3, 28] at consistent q: cov_compare's central differences at the steps (2 h, h), extrapolated to fourth order"""
    frames = range(qc.shape[0])
    P2, P1 = (np.asarray(CC.marker_jacobians(oracle, sk, qc, frames, h)) for h in steps)
    return (4.0 * P1 - P2) / 3.0


def sequence_reference(oracle, sk, cams, opts, pr, q, meas, weight, d_attach, d_marker_off, ridge, T=None, route="dense"):
    """the reference of ONE sequence by `route` on the frame terms T (None: float64 with np.longdouble stencils, at q): dict(R [N, 28, G],
    W [N, L, 3, G], cov_s [G, G], A_red, diag / off = the band of the marginal covariance, cov_pos_m [N, L, 3, 3], sigma_diag / sigma_off / cov_pos =
    the same GIVEN the lengths, and the units u_unit, pos_unit)"""
    from scipy.linalg import cho_factor, cho_solve
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if T is None:
        T = SC.frame_terms(sk, cams, opts, pr, FC.consistent_q(oracle, sk, q), meas, weight, d_attach, d_marker_off, np.float64, np.longdouble)
    Hd, _, _ = SC.band_with_frames(oracle, sk, cams, opts, pr, q, meas, weight, ridge, T["E"])
    N, G = T["b_n"].shape
    n, PB = N * NX, LC.solver_pb(pr)
    Em, A = f64(T["E_n"]).reshape(n, G), f64(T["A_n"].sum(axis=0))
    A = 0.5 * (A + A.T)
    Pm = np.eye(G) / PRIOR_SIGMA ** 2
    qE = f64(T["E"]["q"])
    Ds = f64(SC.position_derivatives(sk, np.asarray(d_attach), np.asarray(d_marker_off), qE))
    Pj = marker_jacobians(oracle, sk, qE, P_STEPS[route])
    if route == "schur":
        c = cho_factor(Hd, lower=True)
        Sig, X = cho_solve(c, np.eye(n)), cho_solve(c, Em)
        R = -X
        Ar = A - Em.T @ X
        Ar = 0.5 * (Ar + Ar.T)
        cov_s = np.linalg.inv(Ar + Pm)
        Mg = Sig + R @ cov_s @ R.T
    else:
        Ki = np.linalg.inv(np.block([[Hd, Em], [Em.T, A + Pm]]))
        Mg, cov_s = Ki[:n, :n], 0.5 * (Ki[n:, n:] + Ki[n:, n:].T)
        R = Ki[:n, n:] @ np.linalg.inv(cov_s)
        Sig = np.linalg.inv(Hd)
        Ar = np.linalg.inv(cov_s) - Pm
    dead = ~Em.any(axis=0) & (np.diag(A) == 0.0) & ~Ds.any(axis=(0, 1, 2))
    R[:, dead] = 0.0
    R = R.reshape(N, NX, G)
    W = Ds + np.einsum("nlak,nkg->nlag", Pj, R)
    Sig, Mg = 0.5 * (Sig + Sig.T), 0.5 * (Mg + Mg.T)
    sd, so = CC.cut_band(Sig, PB)
    md, mo = CC.cut_band(Mg, PB)
    cp = CC.marker_covariance(Pj, sd)
    cpm = cp + np.einsum("nlag,gh,nlbh->nlab", W, cov_s, W)
    u_unit = np.sqrt(np.einsum("nkk->nk", sd)[:, :, None] * np.diag(A)[None, None, :])
    pos_unit = np.abs(Ds) + np.einsum("nlak,nkg->nlag", np.abs(Pj), u_unit)
    return dict(R=R, W=W, cov_s=cov_s, A_red=Ar, diag=md, off=mo, cov_pos_m=cpm, sigma_diag=sd, sigma_off=so, cov_pos=cp, u_unit=u_unit, pos_unit=pos_unit,
                q=qE)


def _per_sequence(c):
    return [(c["sk"][b], c["cams"][b], c["opts"], c["pr"], c["q"][b], c["meas"][b], c["weight"][b], c["d_attach"][b], c["d_marker_off"][b], c["ridge"])
            for b in range(len(c["q"]))]


@functools.lru_cache(maxsize=None)
def case_reference(oracle, name):
    """route dense on the np.longdouble frame terms of scale_compare.case_reference (shared with tests/test_gpu_scale_system.py): one dict per
    sequence -- callers must not modify it"""
    frames = SC.case_reference(oracle, name)["frames"]
    return [sequence_reference(oracle, *a, T=T) for a, T in zip(_per_sequence(SC.case_inputs(name)), frames)]


def outputs(R):
    """a reference's numbers under the kernels' names"""
    return dict(resp_u=[S["R"] for S in R], resp_pos=[S["W"] for S in R], cov_diag_m=[S["diag"] for S in R], cov_off_m=[S["off"] for S in R],
                cov_pos_m=[S["cov_pos_m"] for S in R])


def discrepancies(G, R):
    """worst value of every key: G = dict(resp_u, resp_pos, cov_diag_m, cov_off_m, cov_pos_m: one entry [N_b, ...] per sequence) of HIP,
    R = case_reference(...)"""
    out = {}
    worst = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), v))
    for b, S in enumerate(R):
        worst("resp_u", FC._ratio(G["resp_u"][b], S["R"], S["u_unit"]))
        worst("resp_pos", FC._ratio(G["resp_pos"][b], S["W"], S["pos_unit"]))
        worst("band", CC.scaled_error(np.asarray(G["cov_diag_m"][b]), np.asarray(G["cov_off_m"][b]), S["diag"], S["off"]))
        d = np.sqrt(np.einsum("nlaa->nla", S["cov_pos_m"]))
        worst("cov_pos", FC._ratio(G["cov_pos_m"][b], S["cov_pos_m"], d[..., :, None] * d[..., None, :]))
        cd, cp = np.asarray(G["cov_diag_m"][b]), np.asarray(G["cov_pos_m"][b])
        sym = np.array_equal(cd, np.swapaxes(cd, 1, 2)) and np.array_equal(cp, np.swapaxes(cp, 2, 3)) and np.all(np.isfinite(cd)) and np.all(np.isfinite(cp))
        worst("sym", 0.0 if sym else float("inf"))
    return out


def failures(d, tol):
    return {k: d[k] for k in KEYS if k in d and not d[k] <= tol[k]}


def measure_case(oracle, name, draws=2, seed=0):
    """(measurement 1, measurement 2) of a case, per key"""
    R = case_reference(oracle, name)
    seqs = _per_sequence(SC.case_inputs(name))
    m1 = discrepancies(outputs([sequence_reference(oracle, *a[:4], S["q"], *a[5:], route="schur") for a, S in zip(seqs, R)]), R)
    R64 = [sequence_reference(oracle, *a[:4], S["q"], *a[5:]) for a, S in zip(seqs, R)]
    rng = np.random.default_rng(seed)
    m2 = {}
    for _ in range(draws):
        moved = [np.nextafter(S["q"], np.where(rng.random(S["q"].shape) < 0.5, -np.inf, np.inf)) for S in R]
        SC._merge(m2, discrepancies(outputs([sequence_reference(oracle, *a[:4], q1, *a[5:]) for a, q1 in zip(seqs, moved)]), R64))
    return m1, m2


def widening(S):
    """(median, worst) of marginal over conditional standard deviation of ONE sequence's reference: (coordinates, marker positions)"""
    ru = np.sqrt(np.einsum("nkk->nk", S["diag"]) / np.einsum("nkk->nk", S["sigma_diag"]))
    rp = np.sqrt(np.einsum("nlaa->nla", S["cov_pos_m"]) / np.einsum("nlaa->nla", S["cov_pos"]))
    return (float(np.median(ru)), float(ru.max())), (float(np.median(rp)), float(rp.max()))


if __name__ == "__main__":
    from oracle import oracle as O
    O.lib()
    print("MEASURED = {")
    for name in CASES:
        m1, m2 = measure_case(O, name)
        print(f"    {name!r}: dict(" + ", ".join(f"{k}={max(m1[k], m2[k]):.2e}" for k in MEASURED_KEYS) + "),", flush=True)
    print("}")
