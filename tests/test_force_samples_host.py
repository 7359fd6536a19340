"""Draws of the node forces of the physics-based estimate (cpe_force_samples, include/cpe.h), the part that needs no GPU: the symbols and their
ctypes mirror, the refusals of the C ABI, the joint identity of the numpy reference of tests/force_sample_compare.py on the CPU oracle's system, the
estimator's refusals and its normals.  The HIP side is tests/test_gpu_force_samples.py."""
import ctypes as C

import numpy as np
import pytest

import force_sample_compare as FS
import kinetic_cov_compare as KV
from cheetah_pose_estimation_amd import _lib, abi, skeleton

PLAIN = ("cpe_force_samples", "cpe_force_samples_host")
RAGGED = ("cpe_force_samples_ragged", "cpe_force_samples_ragged_host")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_symbols_and_ctypes_mirror(lib):
    """the library exports the four entry points and the ctypes mirror has their 19 / 21 arguments (fails without the feature)"""
    for names, count in ((PLAIN, 19), (RAGGED, 21)):
        for name in names:
            assert name in abi.FORCE_SAMPLE_ENTRIES and name in abi.ENTRIES and hasattr(lib, name)
            assert len(getattr(lib, name).argtypes) == count
    for name in ("force_samples", "force_samples_host", "force_samples_ragged", "force_samples_ragged_host"):
        assert hasattr(_lib.Handle, name)


def test_refusals(lib):
    """a null handle, null options, null du / f_s, S = 0 and a negative ridge: CPE_BAD_ARG with the reason, before the device is opened (no handle
    is needed to get there)"""
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    dummy = (C.c_double * 4)()                     # never read: every call below is refused before its arrays are looked at
    p = C.addressof(dummy)
    seq = (C.c_int32 * 1)()
    tab = (C.c_int32 * 1)(0)
    for name in PLAIN + RAGGED:
        fn = getattr(lib, name)
        rag = (tab, tab) if name in RAGGED else ()

        def call(h, opt, ridge, S, du, f_s):
            return fn(h, opt, 1, 4, *rag, p, p, p, p, None, None, None, ridge, S, du, None, f_s, None, None, seq)
        for ridge in (-1e-9, float("nan")):
            assert call(None, C.byref(ko), ridge, 1, p, p) == abi.BAD_ARG
            assert b"ridge" in lib.cpe_last_error()
        assert call(None, None, 0.0, 1, p, p) == abi.BAD_ARG
        assert b"options" in lib.cpe_last_error()
        for du, f_s in ((None, p), (p, None)):
            assert call(None, C.byref(ko), 0.0, 1, du, f_s) == abi.BAD_ARG
            assert b"null du / f_s" in lib.cpe_last_error()
        for S in (0, -3):
            assert call(None, C.byref(ko), 0.0, S, p, p) == abi.BAD_ARG
            assert b"S must be at least 1" in lib.cpe_last_error()
        assert call(None, C.byref(ko), 0.0, 2 ** 31 - 1, p, p) == abi.BAD_ARG       # 4 (2^31 - 1) sample frames
        assert name.encode() in lib.cpe_last_error() and b"too many frames" in lib.cpe_last_error()
        assert call(None, C.byref(ko), 0.0, 1, p, p) == abi.BAD_ARG                 # (no handle)
        assert b"null argument" in lib.cpe_last_error()
        if name in RAGGED:
            assert fn(None, C.byref(ko), 1, 4, None, None, p, p, p, p, None, None, None, 0.0, 1, p, None, p, None, None, seq) == abi.BAD_ARG
            assert b"model / n_frames" in lib.cpe_last_error()


@pytest.mark.parametrize("name", ["base", "six"])
def test_joint_identity_of_the_reference(oracle, name):
    """the unit vectors of (z, every node's zeta) through the reference's route 1: sum_s x_s x_s^T over x = (du, df of all nodes) is the inverse of
    the joint matrix, block by block, in kinetic_cov_compare's unit within its tolerance; and the force blocks between different nodes -- what
    cov_f(n) alone does not give -- are far from negligible"""
    c = KV.gallop_case(oracle, name)
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, 0.0)
    ref = KV.reference(Ad, Hk, nodes)
    N = Ad.shape[0]
    X, offs = FS.joint_samples(Ad, Hk, nodes)
    assert X.shape[0] == N * FS.NX + sum(M.shape[0] for _, M in nodes.values())
    J, _ = KV.joint_matrix(Ad, Hk, nodes)
    Jinv, cond = KV.scaled_inverse(J)
    err = FS.block_errors(X, Jinv, offs, nodes, N)
    c1, c5 = FS.cross_correlation(Jinv, offs, nodes, 1), FS.cross_correlation(Jinv, offs, nodes, 5)
    print(f"{name}: {X.shape[0]} samples, joint identity " + ", ".join(f"{k} {v:.1e}" for k, v in err.items()) + f" (tolerance {ref['tol']:.1e}, scaled condition "
          f"{cond:.1e}); largest force-force correlation between nodes n, n + 1: {c1:.3f}, n, n + 5: {c5:.3f}")
    for k, v in err.items():
        assert v <= ref["tol"], (name, k, v, ref["tol"])
    # not negligible: orders of magnitude above what the comparison resolves, and a correlation anyone would see
    assert c1 > 0.1 and c1 > 1e3 * ref["tol"] and c5 > 1e3 * ref["tol"]
    # the two routes of the helper on a node, with random normals
    rng = np.random.default_rng(5)
    n = KV.FLIGHT_NODE
    Hfu, M = nodes[n]
    z = rng.standard_normal((7, N, FS.NX))
    from scipy.linalg import solve_triangular
    import lm_compare as LC
    du = solve_triangular(np.linalg.cholesky(LC.dense(Ad, Hk)).T, z.reshape(7, -1).T, lower=False).T.reshape(z.shape)
    zeta = rng.standard_normal((7, M.shape[0]))
    r = FS.reference(Hfu, M, ref["S"][np.ix_(KV.window(n), KV.window(n))], FS.window_steps(du, n), zeta, FS.sample_norms(z, zeta))
    print(f"{name} node {n}: routes agree to r {r['r']:.1e}, scaled condition of M {r['cond']:.1e}, tolerance {r['tol']:.1e}, largest |df| in the unit {r['bound']:.3f}")
    assert r["r"] < 1e-10 and r["tol"] < 1e-8 and 0.0 < r["bound"] <= 1.0


@pytest.mark.parametrize("name", ["base", "boxed"])
def test_identity_in_numpy(oracle, name):
    """the identity of the GPU test (M^-1 from the zeta unit vectors, -S from the window unit steps, M^-1 + S W S^T against the local formula) run in
    numpy on the oracle's system: what float64 leaves of it on the CPU.  At ridge 1e-6 it is above 10 x 2^-52 x the scaled condition of M at some
    node -- the bound the GPU test cannot use alone -- and it is the r of that test's tolerance"""
    c = KV.gallop_case(oracle, name)
    for ridge in (0.0, 1e-6):
        R, Ad, Hk, nodes = KV.oracle_system(oracle, c, ridge)
        S = KV.reference(Ad, Hk, nodes)["S"]
        vals = {n: FS.identity_error(*nodes[n], S[np.ix_(KV.window(n), KV.window(n))]) for n in nodes}
        worst = max(vals, key=lambda n: vals[n][0])
        over = sum(e > 10.0 * FS.EPS * cond for e, cond in vals.values())
        print(f"{name} ridge {ridge:g}: numpy identity error {min(e for e, _ in vals.values()):.1e} .. {vals[worst][0]:.1e} (node {worst}), "
              f"10 x 2^-52 x cond {10.0 * FS.EPS * min(c_ for _, c_ in vals.values()):.1e} .. {10.0 * FS.EPS * max(c_ for _, c_ in vals.values()):.1e}, above it at {over} of {len(vals)} nodes")
        assert vals[worst][0] < 1e-9                    # (a broken helper does not pass)
        assert over > 0


def test_estimator_refusals_without_a_gpu():
    """uncertainty_samples without uncertainty and a negative count: ValueError before anything is read (the estimator is never looked at); with
    use_2d_reprojections=False: NotImplementedError, as uncertainty alone"""
    from cheetah_pose_estimation_amd import estimator as E
    for fn in (E.estimate_kinetics, E.estimate_grf):
        with pytest.raises(ValueError, match="needs uncertainty=True"):
            fn(None, uncertainty_samples=3)
        with pytest.raises(ValueError, match=">= 0"):
            fn(None, uncertainty=True, uncertainty_samples=-1)
    for ragged in (False, True):
        with pytest.raises(ValueError, match="needs uncertainty=True"):
            E.estimate_kinetics_batch([None], ragged=ragged, uncertainty_samples=3)
        with pytest.raises(ValueError, match=">= 0"):
            E.estimate_kinetics_batch([None], ragged=ragged, uncertainty=True, uncertainty_samples=-2)
        with pytest.raises(NotImplementedError, match="use_2d_reprojections"):
            E.estimate_kinetics_batch([], ragged=ragged, uncertainty=True, uncertainty_samples=3, use_2d_reprojections=False)

    class Stub:
        class params:
            start_frame, end_frame = 0, 8
    with pytest.raises(NotImplementedError, match="use_2d_reprojections"):
        E.estimate_kinetics(Stub(), uncertainty=True, uncertainty_samples=3, use_2d_reprojections=False)
    assert set(E.SAMPLE_FIELDS) < set(E.KINETIC_SAMPLE_FIELDS)
    assert set(E.KINETIC_SAMPLE_FIELDS) - set(E.SAMPLE_FIELDS) == {"tau", "lam", "grf_net", "tau_mean", "lam_mean", "grf_net_mean"}


def test_force_normals():
    """sample_force_normals is a function of (seed, K, N) alone and a stream of its own: not sample_normals' numbers"""
    from cheetah_pose_estimation_amd import estimator as E
    a, b = E.sample_force_normals(3, 4, 9), E.sample_force_normals(3, 4, 9)
    assert a.shape == (4, 9, 64) and a.dtype == np.float64 and a.tobytes() == b.tobytes()
    assert np.array_equal(a, np.random.default_rng([3, 1]).standard_normal((4, 9, 64)))
    for other in (E.sample_force_normals(4, 4, 9), E.sample_force_normals(3, 4, 10)[:, :9]):
        assert not np.array_equal(a, other)
    z = E.sample_normals(3, 4, 9)
    assert z.tobytes() == np.random.default_rng(3).standard_normal((4, 9, 28)).tobytes()          # (unchanged: the du of a physics draw follows the kinematic rule)
    assert not np.array_equal(a[..., :28], z) and not np.array_equal(a.ravel()[:z.size], z.ravel())
    f = E.force_sample_fields(np.arange(2 * 3 * 64, dtype=np.float64).reshape(2, 3, 64), np.arange(3 * 64, dtype=np.float64).reshape(3, 64), 22, 26, 4)
    assert f["tau"].shape == (2, 3, 22) and f["lam"].shape == (2, 3, 26) and f["grf_net"].shape == (2, 3, 4, 3)
    assert f["tau_mean"].shape == (3, 22) and f["lam_mean"].shape == (3, 26) and f["grf_net_mean"].shape == (3, 4, 3)
    assert f["grf_net"][1, 2, 3, 2] == 64 * 5 + 22 + 26 + 11 and f["lam_mean"][2, 0] == 64 * 2 + 22
