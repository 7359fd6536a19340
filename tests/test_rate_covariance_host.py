"""Rate covariance, the parts that need no GPU: the numpy reference (tests/rate_compare.py) by two routes on the oracle's bands and on random
bands, the power of that comparison, the library's refusals, the prototypes against the ctypes mirror, and the estimator's keyword."""
import ctypes as C

import numpy as np
import pytest

import cov_compare as CC
import rate_compare as RC
from test_covariance_host import _prototype
from cheetah_pose_estimation_amd import _lib, abi

H = 1.0 / 120.0
N_TERMS = 9          # products summed into one entry of cov_du / cov_ddu: a three-frame stencil has 3 x 3 blocks


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def _bands(oracle):
    """(label, diag, off, dense inverse) of every band the comparison runs on"""
    for name in ("six", "mono"):
        c = CC.oracle_case(oracle, name)
        for ridge in (0.0, 1e-6):
            d, o, S = CC.dense_inverse(CC.damped(c["Bk"], ridge), c["Hk"])
            yield f"{name} ridge {ridge:g}", d, o, S
    for PB in (3, 4):
        for N in (1, 2, 3, 4, 9):
            d, o, S = CC.dense_inverse(*CC.random_band(N, PB, 31 * PB + N))
            yield f"random PB {PB} N {N}", d, o, S


def _misses(got, ref, bound):
    """entries of `got` outside the round-off bound around `ref`"""
    return int(np.count_nonzero(np.abs(got - ref) > RC.roundoff_tolerance(N_TERMS, bound)))


def test_band_route_equals_dense_route(oracle):
    """the stencil formulas on the band against D S D^T with the explicit (N 28) x (N 28) difference matrices, entry by entry, within
    (n + 3) 2^-52 |expression|; and the comparison has power: a flipped cross term and a missing frame-0 gauge both fail that bound"""
    worst = 0.0
    for label, d, o, S in _bands(oracle):
        N = d.shape[0]
        du, ddu = RC.rates_from_band(d, o, H)
        dv, dda = RC.rates_dense(S, H)
        bu, bdu = RC.abs_bound("rates", d, o, H)
        rel = max(float((np.abs(du - dv)[bu > 0] / bu[bu > 0]).max()) if N > 1 else 0.0, float((np.abs(ddu - dda)[bdu > 0] / bdu[bdu > 0]).max()) if N > 2 else 0.0)
        worst = max(worst, rel)
        print(f"{label}: band route against dense route {rel:.2e} of the bound expression (tolerance {(N_TERMS + 3) * RC.EPS:.2e})")
        assert _misses(du, dv, bu) == 0 and _misses(ddu, dda, bdu) == 0, label
        if N == 1:
            assert not du.any() and not ddu.any() and not dv.any() and not dda.any()
        if N == 2:
            assert not ddu.any() and not dda.any() and np.array_equal(du[0], du[1])
        if N >= 3:
            assert np.array_equal(ddu[0], ddu[2]) and np.array_equal(ddu[1], ddu[2])
        if N >= 2:
            fu, fdu = RC.rates_from_band(d, o, H, cross_sign=-1.0)
            assert _misses(fu, dv, bu) > 0, label
        if N >= 3:
            gu, gdu = RC.rates_from_band(d, o, H, gauge=False)
            assert _misses(gu, dv, bu) > 0 and _misses(gdu, dda, bdu) > 0 and _misses(fdu, dda, bdu) > 0, label
    print(f"worst over all bands: {worst:.2e}")


@pytest.mark.parametrize("name", ["six", "mono"])
def test_consecutive_frames_are_positively_correlated(oracle, name):
    """on the oracle's bands h^2 var(du_n) < var u_n + var u_{n-1} for every coordinate and n >= 1 (the cross term lowers the variance of a
    difference); with the sign of the cross term flipped the ratio is above 1 everywhere"""
    c = CC.oracle_case(oracle, name)
    for ridge in (0.0, 1e-6):
        d, o, _ = CC.dense_inverse(CC.damped(c["Bk"], ridge), c["Hk"])
        r = RC.variance_ratio(RC.rates_from_band(d, o, H)[0], d, H)
        f = RC.variance_ratio(RC.rates_from_band(d, o, H, cross_sign=-1.0)[0], d, H)
        print(f"{name} ridge {ridge:g}: h^2 var du / (var u_n + var u_n-1) at most {r.max():.3f}; flipped sign at least {f.min():.3f}")
        assert np.all(r > 0.0) and np.all(r < 1.0) and np.all(f > 1.0)


def test_point_formulas_agree_with_the_dense_route():
    """point_cov / point_vel_cov on a random band and random Jacobians against J S J^T with the stacked velocity Jacobian"""
    N, PB = 5, 3
    d, o, S = CC.dense_inverse(*CC.random_band(N, PB, 77))
    P = np.random.default_rng(5).normal(size=(N, 2, 3, 28))
    got, bound = RC.point_vel_cov(P, d, o, H), RC.abs_bound("point_vel", P, d, o, H)
    assert not got[0].any()
    for n in range(1, N):
        for l in range(2):
            J = np.zeros((3, N * 28))
            J[:, n * 28:(n + 1) * 28] = P[n, l] / H
            J[:, (n - 1) * 28:n * 28] = -P[n - 1, l] / H
            assert np.all(np.abs(got[n, l] - J @ S @ J.T) <= RC.roundoff_tolerance(4 * 28 * 28, bound[n, l]))
    assert np.all(np.abs(RC.point_cov(P, d)[2, 1] - P[2, 1] @ d[2] @ P[2, 1].T) <= RC.roundoff_tolerance(28 * 28, RC.abs_bound("point", P, d)[2, 1]))


def test_signatures(lib):
    """the four prototypes of include/cpe.h against abi.RATE_COVARIANCE_ENTRIES, the symbols and the wrappers (fails without the feature)"""
    assert set(abi.RATE_COVARIANCE_ENTRIES) == {"cpe_rate_covariance", "cpe_rate_covariance_host", "cpe_rate_covariance_ragged",
                                                "cpe_rate_covariance_ragged_host"}
    for name, kinds in abi.RATE_COVARIANCE_ENTRIES.items():
        fn = getattr(lib, name)                                   # AttributeError when the symbol is missing
        assert _prototype(name) == tuple(kinds), name
        assert abi.ENTRIES[name] == kinds and list(fn.argtypes) == abi.argtypes(name), name
    assert len(abi.RATE_COVARIANCE_OUTPUTS) == 7
    for method in ("rate_covariance", "rate_covariance_host", "rate_covariance_ragged_host"):
        assert callable(getattr(_lib.Handle, method))


def test_refusals(lib):
    """negative sizes, null required arguments, all outputs null, null model / n_frames: CPE_BAD_ARG with the reason, before a handle is looked at
    (the pointers below are never dereferenced: every refusal here precedes the first use of one)"""
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    one = (C.c_int32 * 1)(1)
    none7 = (None,) * 7
    plain = ("cpe_rate_covariance", "cpe_rate_covariance_host")
    ragged = ("cpe_rate_covariance_ragged", "cpe_rate_covariance_ragged_host")
    for name in plain + ragged:
        fn = getattr(lib, name)
        mid = (one, one) if name in ragged else ()
        for B, N in ((-1, 3), (1, -3)):
            assert fn(None, B, N, *mid, None, None, None, *none7) == abi.BAD_ARG
            assert b"negative size" in lib.cpe_last_error() and name.encode() + b":" in lib.cpe_last_error()
        for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):      # h, q, cov_diag, cov_off
            assert fn(args[0], 1, 1, *mid, *args[1:], p, *(None,) * 6) == abi.BAD_ARG
            assert b"null argument" in lib.cpe_last_error()
        assert fn(p, 1, 1, *mid, p, p, p, *none7) == abi.BAD_ARG
        assert b"all outputs are null" in lib.cpe_last_error()
    for name in ragged:
        fn = getattr(lib, name)
        for mid in ((None, one), (one, None)):
            assert fn(p, 1, 1, *mid, p, p, p, p, *(None,) * 6) == abi.BAD_ARG
            assert b"null model / n_frames" in lib.cpe_last_error()


def test_keyword_needs_uncertainty():
    """uncertainty_rates=True without uncertainty=True: ValueError in all five functions, before the estimator is looked at"""
    from cheetah_pose_estimation_amd import estimator as E
    for fn, arg in ((E.estimate_kinematics, None), (E.estimate_kinematics_batch, [None]), (E.estimate_kinetics, None),
                    (E.estimate_kinetics_batch, [None]), (E.estimate_grf, None)):
        with pytest.raises(ValueError, match="uncertainty_rates"):
            fn(arg, uncertainty_rates=True)
        with pytest.raises(ValueError, match="uncertainty_rates"):
            fn(arg, uncertainty=False, uncertainty_rates=True)


def test_speed_std_is_the_delta_method():
    from cheetah_pose_estimation_amd.estimator import speed_std_of
    v = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 2.0]])
    Cv = np.stack([np.diag([1.0, 4.0, 9.0])] * 3)
    assert np.allclose(speed_std_of(v, Cv), [np.sqrt(9.0 + 64.0) / 5.0, 0.0, 3.0], rtol=1e-15)
