"""Draws from the posterior, the parts that need no GPU: the four prototypes against the ctypes mirror and the exported symbols, the refusals,
the numpy reference (tests/sample_compare.py) by its two routes and its identity check, and the estimator's keywords."""
import ctypes as C

import numpy as np
import pytest

import cov_compare as CC
import sample_compare as SM
from test_covariance_host import _prototype
from cheetah_pose_estimation_amd import _lib, abi
from cheetah_pose_estimation_amd import estimator as E

BAND = ("h", "i", "i", "ip", "p", "i", "p", "p")
POSTERIOR = ("h", "i", "i", "ip", "ip", "p", "i", "p", "p", "p")
SHAPES = [(1, 3, 1), (5, 3, 2), (11, 4, 3), (40, 4, 4), (40, 3, 5)]           # (N, PB, seed)


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_signatures(lib):
    """the four prototypes of include/cpe.h against abi.SAMPLE_ENTRIES, the exported symbols and the wrappers (fails without the feature)"""
    assert abi.SAMPLE_ENTRIES == {"cpe_band_sample": BAND, "cpe_band_sample_host": BAND, "cpe_posterior_samples": POSTERIOR,
                                  "cpe_posterior_samples_host": POSTERIOR}
    for name, kinds in abi.SAMPLE_ENTRIES.items():
        fn = getattr(lib, name)                                   # AttributeError when the symbol is missing
        assert _prototype(name) == tuple(abi.ENTRIES[name]) == kinds, name
        assert list(fn.argtypes) == abi.argtypes(name), name
    for method in ("band_sample", "band_sample_host", "posterior_samples", "posterior_samples_host"):
        assert callable(getattr(_lib.Handle, method))


def test_refusals(lib):
    """CPE_BAD_ARG with the reason, before anything is dereferenced: S < 1, negative sizes, too many sample frames, a frame count outside 0..N,
    model without n_frames, a null handle"""
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    one, two, neg = (C.c_int32 * 1)(0), (C.c_int32 * 1)(2), (C.c_int32 * 1)(-1)

    def refused(name, args, reason):
        assert getattr(lib, name)(*args) == abi.BAD_ARG, (name, args)
        err = lib.cpe_last_error()
        assert name.encode() + b":" in err and reason in err, (name, err)

    for name in ("cpe_band_sample", "cpe_band_sample_host"):
        for S in (0, -3):
            refused(name, (None, 1, 1, None, p, S, p, p), b"S must be at least 1")
        refused(name, (None, -1, 1, None, p, 1, p, p), b"negative size")
        refused(name, (None, 1, -1, None, p, 1, p, p), b"negative size")
        refused(name, (None, 1 << 15, 1 << 15, None, p, 4, p, p), b"too many frames")
        refused(name, (None, 1, 1, two, p, 1, p, p), b"frame count of sequence 0 outside 0..N")
        refused(name, (None, 1, 1, neg, p, 1, p, p), b"frame count of sequence 0 outside 0..N")
        refused(name, (None, 1, 1, one, p, 1, p, p), b"null argument")
        refused(name, (None, 1, 1, None, p, 1, p, p), b"null argument")
    for name in ("cpe_posterior_samples", "cpe_posterior_samples_host"):
        refused(name, (None, 1, 1, None, None, p, 0, p, p, p), b"S must be at least 1")
        refused(name, (None, 1, -1, None, None, p, 1, p, p, p), b"negative size")
        refused(name, (None, 1 << 15, 1 << 15, None, None, p, 4, p, p, p), b"too many frames")
        refused(name, (None, 1, 1, one, None, p, 1, p, p, p), b"model and n_frames are given together")
        refused(name, (None, 1, 1, None, one, p, 1, p, p, p), b"model and n_frames are given together")
        refused(name, (None, 1, 1, None, None, p, 1, p, p, p), b"null argument")
        refused(name, (None, 1, 1, one, one, p, 1, p, p, None), b"null argument")


@pytest.mark.parametrize("N,PB,seed", SHAPES)
def test_routes_agree_and_the_identity_holds(N, PB, seed):
    """the triangular solve against the long-double recurrence in the helper's unit; |du_a| <= s_a ||z|| (the unit's own bound); the identity sum
    of route 1 against the dense inverse's band within 10 max(its own error, 2^-52 cond) -- trivially, which is the point: the numbers printed
    here are what the GPU's tolerance is made of"""
    L = CC.cholesky_layout(*CC.random_band(N, PB, seed))
    z = np.random.default_rng(seed).standard_normal((65, N, SM.NX))
    R = SM.reference(L, z, identity=True)
    print(f"N {N} PB {PB}: r {R['r']:.2e}, 2^-52 cond {SM.EPS * R['cond']:.2e}, max |du| / (s |z|) {R['bound']:.3f}, identity e_ref {R['e_ref']:.2e}")
    assert R["r"] <= 1e-15 and R["r"] <= R["tol"] / 10.0
    assert R["bound"] <= 1.0
    assert R["e_ref"] <= 1e-11 and R["tol_identity"] >= 10.0 * R["e_ref"]
    # the recurrence's own identity sum passes the bound set by route 1
    e2 = CC.scaled_error(*SM.band_of_sum(SM.solve_recurrence(L, SM.unit_vectors(N)), PB), R["diag"], R["off"])
    assert e2 <= R["tol_identity"], (e2, R["tol_identity"])
    # L^T du = z, directly
    D = SM.dense_factor(L)
    assert np.allclose(D.T @ R["du"].reshape(65, -1).T, z.reshape(65, -1).T, rtol=0, atol=1e-9 * np.abs(z).max())


def test_keywords():
    """uncertainty_samples without uncertainty=True, and a negative count: ValueError in both functions before an estimator attribute is read"""
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"estimator.{name} was read")
    for fn, arg in ((E.estimate_kinematics, Untouchable()), (E.estimate_kinematics_batch, [Untouchable()])):
        with pytest.raises(ValueError, match="uncertainty_samples needs uncertainty=True"):
            fn(arg, uncertainty_samples=3)
        for kw in (dict(), dict(uncertainty=True)):
            with pytest.raises(ValueError, match="uncertainty_samples must be >= 0"):
                fn(arg, uncertainty_samples=-1, **kw)
    with pytest.raises(ValueError, match="uncertainty_samples needs uncertainty=True"):
        E.estimate_kinematics_batch([Untouchable()], uncertainty_samples=3, ragged=True)
    assert E.SAMPLE_FIELDS == ("seed", "ridge", "du", "q", "x", "positions", "com_pos")
    assert not set(E.SAMPLE_FIELDS) & (set(E.RATE_FIELDS) | set(E.SPAN_FIELDS)) - {"ridge"}


def test_z_is_a_function_of_seed_count_and_length():
    """z = default_rng(seed).standard_normal((K, N, 28)) and nothing else: the same bits on every call, other bits for another seed, count or
    length; the helper's copy of the rule is the estimator's"""
    z = E.sample_normals(7, 4, 40)
    assert z.shape == (4, 40, 28) and z.dtype == np.float64
    assert z.tobytes() == np.random.default_rng(7).standard_normal((4, 40, 28)).tobytes() == E.sample_normals(7, 4, 40).tobytes() == SM.normals(7, 4, 40).tobytes()
    for other in ((8, 4, 40), (7, 4, 39)):                  # (a larger K continues the same stream: its first 4 samples are these)
        zo = E.sample_normals(*other)
        assert zo.shape == (other[1], other[2], 28) and not np.array_equal(zo[:, :39], z[:, :39])
    assert np.array_equal(E.sample_normals(7, 5, 40)[:4], z)
