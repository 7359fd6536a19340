"""Posterior covariance of the physics-based estimate (cpe_covariance_kinetic, include/cpe.h), the part that needs no GPU: the two numpy routes
of tests/kinetic_cov_compare.py against each other on the CPU oracle's system, the inputs of the GPU tests (positive definite, or without a
factor where the GPU test wants that), the ordering in the damping, the refusals of the C ABI and the estimator's scatter of cov_f.  The HIP side
is tests/test_gpu_kinetic_covariance.py."""
import ctypes as C

import numpy as np
import pytest

import kinetic_cov_compare as KV
import lm_compare as LC
from cheetah_pose_estimation_amd import _lib, abi, skeleton


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_symbols_and_ctypes_mirror(lib):
    """the library exports the entry points and the ctypes mirror has their 20 arguments (fails without the feature)"""
    for name in ("cpe_covariance_kinetic", "cpe_covariance_kinetic_host"):
        assert name in abi.KINETIC_COVARIANCE_ENTRIES and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 20
    assert hasattr(_lib.Handle, "covariance_kinetic_host")


def test_refusals(lib):
    """bad ridge, null options, null stance, two variant pointers: CPE_BAD_ARG with the reason, before the device is opened (no handle is needed to
    get there); valid arguments get as far as the handle"""
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    dummy = (C.c_double * 4)()                     # never read: every call below is refused before its arrays are looked at
    p = C.addressof(dummy)
    for name in ("cpe_covariance_kinetic", "cpe_covariance_kinetic_host"):
        fn = getattr(lib, name)
        call = lambda opt, stance, var, ridge: fn(None, opt, 1, 4, None, None, None, stance, var[0], var[1], var[2], ridge, None, None, None, None,
                                                  None, None, None, None)
        none = (None, None, None)
        for ridge in (-1e-9, float("nan"), float("inf")):
            assert call(C.byref(ko), p, none, ridge) == abi.BAD_ARG
            assert b"ridge" in lib.cpe_last_error()
        assert call(None, p, none, 0.0) == abi.BAD_ARG
        assert b"options" in lib.cpe_last_error()
        assert call(C.byref(ko), None, none, 0.0) == abi.BAD_ARG
        assert b"stance" in lib.cpe_last_error()
        for var in ((p, p, None), (p, None, p), (None, p, p), (p, p, p)):
            assert call(C.byref(ko), p, var, 0.0) == abi.BAD_ARG
            assert b"at most one" in lib.cpe_last_error()
        assert call(C.byref(ko), p, (p, None, None), 1e-6) == abi.BAD_ARG          # (no handle)
        assert b"null" in lib.cpe_last_error()


@pytest.mark.parametrize("name", ["base", "six"])
def test_the_two_routes_agree(oracle, name):
    """joint route against local route on the oracle's system at its solution, ridge 0 and 1e-6: r stays below the cap 1e-4 (a broken helper does
    not pass) and the tolerance the GPU tests get from it is far below any error worth finding; the recorded values are in the helper's docstring"""
    c = KV.gallop_case(oracle, name)
    for ridge in (0.0, 1e-6):
        R, Ad, Hk, nodes = KV.oracle_system(oracle, c, ridge)
        ref = KV.reference(Ad, Hk, nodes)
        print(f"{name} ridge {ridge:g}: r {ref['r']:.1e} (forces {ref['r_f']:.1e}, coordinates {ref['r_u']:.1e}), scaled condition {ref['cond']:.1e}, "
              f"tolerance {ref['tol']:.1e}")
        assert ref["r"] < 1e-4 and ref["tol"] < 1e-3
        n = KV.FLIGHT_NODE
        std = np.sqrt(np.diag(ref["cov_f"][n]))
        assert np.all(std > 0.0) and np.all(np.isfinite(std))
        # the formula itself, by its two evaluations (what the kernel test's tolerance is made of): far tighter than the band allows
        Hfu, M = nodes[n]
        _, tol, r2, cond = KV.kernel_tolerance(Hfu, M, ref["S"][np.ix_(KV.window(n), KV.window(n))])
        print(f"{name} ridge {ridge:g} node {n}: local formula solve / Cholesky {r2:.1e}, scaled condition of M {cond:.1e}")
        assert tol < 1e-8


@pytest.mark.parametrize("name", KV.CASES)
def test_inputs_of_the_gpu_tests_are_positive_definite(oracle, name):
    """the band and every node's H_ff at ridge 0, on every case the GPU tests evaluate; the node counts the GPU tests rely on"""
    c = KV.gallop_case(oracle, name)
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, 0.0)
    ev = np.linalg.eigvalsh(LC.dense(Ad, Hk))
    ef = min(np.linalg.eigvalsh(M)[0] for _, M in nodes.values())
    print(f"{name}: smallest eigenvalue of the band {ev[0]:.3g} (largest {ev[-1]:.3g}), of H_ff {ef:.3g}; na {sorted(set(R['meta'][2:, 0]))}")
    assert ev[0] > 0.0 and ef > 0.0
    np.linalg.cholesky(LC.dense(Ad, Hk))
    na = R["meta"][2:, 0]
    if name == "base":
        assert set(na) == {51, 54}
    if name == "flight":
        assert na[KV.FLIGHT_NODE - 2] == 48 and set(na) == {48, 51, 54}
    if name == "fixed":
        assert set(na) == {48}
    if name == "boxed":
        base = KV.oracle_system(oracle, KV.gallop_case(oracle, "base"), 0.0)[0]
        assert not np.array_equal(R["Hff"], base["Hff"])                          # the boxes bind: their penalty curvature is in H_ff


@pytest.mark.parametrize("name", ["base", "six", "flight"])
def test_reduced_band_is_the_schur_complement(oracle, name):
    """what makes cov_f = M^-1 + S W S^T the force block of the joint inverse: the oracle's reduced band equals (per-frame band) + sum_n H_uu - H_uf
    H_ff^-1 H_fu, assembled here from oracle.objective and the node pieces.  Bound 1e-10: the two evaluations of H_uf H_ff^-1 H_fu differ by
    2^-52 x the scaled condition of H_ff (130 - 350) of that term, and the term is up to 1e3 of what is left of H_uu after it is subtracted"""
    d = KV.schur_band_difference(oracle, KV.gallop_case(oracle, name))
    print(f"{name}: reduced band against per-frame band + node Schur complements {d:.1e}")
    assert d < 1e-10


def test_two_frames_have_coordinates_without_curvature(oracle):
    """N = 2 has no node, and the 24-marker skeleton without a motion term leaves coordinates that no marker moves: exact zeros on the band's
    diagonal, an exactly zero pivot at ridge 0 (the GPU test of the edge lengths relies on it)"""
    c = dict(KV.gallop_case(oracle, "base"))
    for k in ("q", "meas", "weight", "stance"):
        c[k] = np.ascontiguousarray(c[k][:2])
    Ad = KV.oracle_system(oracle, c, 0.0)[1]
    assert np.all((np.diagonal(Ad, axis1=1, axis2=2) == 0.0).sum(axis=1) >= 1)


def test_input_without_a_factor(oracle):
    """the GPU test of the numerical status: the base case with every weight zero (no camera sees a marker).  Translations along x and y leave the
    physics terms unchanged, so the band is singular: its smallest eigenvalue is round-off of the largest.  (With three frames or more the physics
    terms give every coordinate curvature, so no input of that length has an exactly zero pivot; the pivot that fails is round-off.)"""
    c = dict(KV.gallop_case(oracle, "base"))
    c["weight"] = np.zeros_like(c["weight"])
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, 0.0)
    ev = np.linalg.eigvalsh(LC.dense(Ad, Hk))
    assert abs(ev[0]) < 1e-12 * ev[-1] and abs(ev[1]) < 1e-12 * ev[-1]
    assert min(np.linalg.eigvalsh(M)[0] for _, M in nodes.values()) > 0.0      # the node matrices are not what fails


def test_damping_lowers_the_force_covariance(oracle):
    """cov_f(ridge) <= cov_f(0) in the PSD order for a diagonal-only damping (the helper's own matrices: ridge D on the band's diagonal, ridge x
    lm_force_damping x diag H_ff on every node's), by the joint route"""
    c = KV.gallop_case(oracle, "base")
    R, Ad0, Hk, nodes0 = KV.oracle_system(oracle, c, 0.0)
    J0, offs = KV.joint_matrix(Ad0, Hk, nodes0)
    S0, cond = KV.scaled_inverse(J0)
    tol = 10.0 * KV.EPS * cond
    nu = Ad0.shape[0] * KV.NX
    for ridge in (1e-6, 1e-3):
        J = J0.copy()
        d = np.zeros(J.shape[0])
        d[:nu] = ridge * np.maximum(np.diag(J0)[:nu], LC.diag_floor(Ad0.shape[0]))
        d[nu:] = ridge * c["ko"].lm_force_damping * np.diag(J0)[nu:]
        J[np.diag_indices_from(J)] += d
        S1 = KV.scaled_inverse(J)[0]
        worst = min(KV.psd_gap(S0[o:o + nodes0[n][0].shape[0], o:o + nodes0[n][0].shape[0]], S1[o:o + nodes0[n][0].shape[0], o:o + nodes0[n][0].shape[0]])
                    for n, o in offs.items())
        print(f"ridge {ridge:g}: smallest scaled eigenvalue of cov_f(0) - cov_f(ridge) {worst:.2e} (tolerance {-tol:.1e})")
        assert worst >= -tol
        assert all(np.all(np.diag(S1)[o:o + 3] < np.diag(S0)[o:o + 3]) for o in offs.values())


def test_estimator_scatter_of_a_hand_made_node():
    """force_uncertainty: cov_f + meta -> tau_std / lambda_std / grf_std / tau_cov in f's layout, zeros where a force is not an unknown"""
    from cheetah_pose_estimation_amd.estimator import force_uncertainty
    nm, nc, nf = 3, 2, 2                                       # f = tau0 tau1 tau2 | lam0 lam1 | (z, x, y) foot 0 | (z, x, y) foot 1
    cov = np.zeros((3, 64, 64)); meta = np.zeros((3, 65), dtype=np.int32)
    idx = [0, 2, 3, 8, 9, 10]                                  # node 2: tau0, tau2, lam0, foot 1 (z, x, y); tau1, lam1 and foot 0 are not unknowns
    A = np.arange(1.0, 37.0).reshape(6, 6); A = A @ A.T + np.eye(6)
    cov[2, :6, :6] = A
    meta[2, 0] = 6; meta[2, 1:7] = idx; meta[2, 64] = 5         # (the last word is not an index)
    u = force_uncertainty(cov, meta, nm, nc, nf)
    assert u["tau_std"].shape == (3, 3) and u["lambda_std"].shape == (3, 2) and u["grf_std"].shape == (3, 2, 3) and u["tau_cov"].shape == (3, 3, 3)
    s = np.sqrt(np.diag(A))
    assert np.array_equal(u["tau_std"][2], [s[0], 0.0, s[1]])
    assert np.array_equal(u["lambda_std"][2], [s[2], 0.0])
    assert np.array_equal(u["grf_std"][2], [[0.0, 0.0, 0.0], [s[3], s[4], s[5]]])
    assert np.array_equal(u["tau_cov"][2], [[A[0, 0], 0.0, A[0, 1]], [0.0, 0.0, 0.0], [A[1, 0], 0.0, A[1, 1]]])
    assert not u["tau_std"][:2].any() and not u["grf_std"][:2].any() and not u["tau_cov"][:2].any()
