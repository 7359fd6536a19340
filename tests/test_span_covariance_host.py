"""Covariance between distant frames, the parts that need no GPU: the numpy reference (tests/span_compare.py) by two routes on random bands and
on the oracle's bands, estimator.span_uncertainty against J S J^T, the stated condition of the monocular case, the prototypes against the ctypes
mirror, and the estimator's keyword."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import cov_compare as CC
import span_compare as SC
from test_covariance_host import _prototype
from cheetah_pose_estimation_amd import _lib, abi
from cheetah_pose_estimation_amd import estimator as E

NX = 28
H = 1.0 / 120.0


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def _anchors(N, PB):
    return sorted({N - 1, N // 2, PB + 1, PB, 0})


def _routes(label, Ad, Hk, PB):
    """the two routes on one matrix: their discrepancy against cov_compare's tolerance of that matrix (set by the band's own two routes)"""
    N = Ad.shape[0]
    R = SC.reference(Ad, Hk, _anchors(N, PB))
    tol = CC.reference(Ad, Hk)["tol_err"]
    print(f"{label}: columns, recurrence against dense inverse {R['r']:.2e} (scaled condition {R['cond']:.2e}, band tolerance {tol:.2e})")
    assert R["r"] <= tol, (label, R["r"], tol)
    return R


@pytest.mark.parametrize("N,PB", [(9, 3), (57, 4)])
def test_routes_agree_on_random_bands(N, PB):
    Ad, Hk = CC.random_band(N, PB, 500 + N)
    R = _routes(f"random N {N} PB {PB}", Ad, Hk, PB)
    # the layout: rows a-PB .. a are the band blocks, the rows below the anchor are zero
    for k, a in enumerate(_anchors(N, PB)):
        assert np.array_equal(R["cols"][k, a], R["diag"][a]) and not R["cols"][k, a + 1:].any()
        for i in range(1, min(PB, a) + 1):
            assert np.array_equal(R["cols"][k, a - i], R["off"][a - i, i - 1].T)


@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("name", ["six", "two", "mono"])
def test_routes_agree_on_the_oracles_bands(oracle, name, ridge):
    c = CC.oracle_case(oracle, name)
    _routes(f"{name} ridge {ridge:g}", CC.damped(c["Bk"], ridge), c["Hk"], c["PB"])


def _random_case(N=9, PB=3, L=2, seed=3):
    rng = np.random.default_rng(seed)
    d, o, S = CC.dense_inverse(*CC.random_band(N, PB, 70 + seed))
    spans = [(0, N - 1), (2, 5), (1, N - 1), (3, 4)]
    anchors = sorted({b for _, b in spans})
    return dict(N=N, d=d, S=S, spans=spans, anchors=anchors + [-1], cols=np.concatenate([SC.columns_dense(S, anchors), np.zeros((1, N, NX, NX))]),
                Pc=rng.normal(size=(N, 3, NX)), Pp=rng.normal(size=(N, L, 3, NX)), com=rng.normal(size=(N, 3)))


def test_span_uncertainty_is_J_S_Jt():
    """every covariance of span_uncertainty against J S J^T with the dense S and the stacked Jacobian J = [.. -P_a .. P_b ..], entry by entry
    within (4 x 28^2 + 3) 2^-52 of the sum of the absolute values of the products (the round-off of two sums of that length)"""
    c = _random_case()
    out = E.span_uncertainty(c["cols"], c["anchors"], c["d"], c["Pc"], c["Pp"], c["com"], c["spans"], H)
    assert set(out) == set(E.SPAN_FIELDS) and np.array_equal(out["span_frames"], np.array(c["spans"]))
    Sabs = np.abs(c["S"])
    for s, (a, b) in enumerate(c["spans"]):
        for P, got in [(c["Pc"], out["span_com_displacement_cov"][s])] + [(c["Pp"][:, l], out["span_positions_displacement_cov"][s, l]) for l in range(2)]:
            J = np.zeros((3, c["N"] * NX))
            J[:, b * NX:(b + 1) * NX] = P[b]
            J[:, a * NX:(a + 1) * NX] = -P[a]
            bound = (4 * NX * NX + 3) * 2.0 ** -52 * (np.abs(J) @ Sabs @ np.abs(J).T)
            assert np.all(np.abs(got - J @ c["S"] @ J.T) <= bound), (s, a, b)
            assert np.array_equal(got, got.T)
    sec = out["span_seconds"]
    assert np.array_equal(sec, np.array([(b - a) * H for a, b in c["spans"]]))
    assert np.array_equal(out["span_mean_velocity_cov"], out["span_com_displacement_cov"] / (sec ** 2)[:, None, None])


def test_span_fields_follow_from_each_other():
    """mean velocity = the mean of com_vel[first:last] to round-off; every _std = sqrt of its covariance's diagonal; distance and speed by the
    delta method of speed_std_of"""
    c = _random_case(seed=4)
    out = E.span_uncertainty(c["cols"], c["anchors"], c["d"], c["Pc"], c["Pp"], c["com"], c["spans"], H)
    com_vel = (c["com"][1:] - c["com"][:-1]) / H
    for s, (a, b) in enumerate(c["spans"]):
        # (a telescoping sum of b - a differences of numbers of size max |com| / h)
        atol = (b - a + 2) * 2.0 ** -52 * np.abs(c["com"]).max() / H
        assert np.all(np.abs(out["span_mean_velocity"][s] - com_vel[a:b].mean(axis=0)) <= atol)
        assert np.array_equal(out["span_com_displacement"][s], c["com"][b] - c["com"][a])
    for key in ("span_com_displacement", "span_mean_velocity", "span_positions_displacement"):
        assert np.array_equal(out[key + "_std"], np.sqrt(np.diagonal(out[key + "_cov"], axis1=-2, axis2=-1))), key
        assert np.all(out[key + "_std"] > 0.0)
    assert np.array_equal(out["span_distance"], np.linalg.norm(out["span_com_displacement"], axis=1))
    assert np.array_equal(out["span_distance_std"], E.speed_std_of(out["span_com_displacement"], out["span_com_displacement_cov"]))
    assert np.array_equal(out["span_mean_speed_std"], E.speed_std_of(out["span_mean_velocity"], out["span_mean_velocity_cov"]))
    assert np.allclose(out["span_mean_speed"], out["span_distance"] / out["span_seconds"], rtol=1e-15)
    assert np.allclose(out["span_mean_speed_std"], out["span_distance_std"] / out["span_seconds"], rtol=1e-12)
    empty = E.span_uncertainty(c["cols"], c["anchors"], c["d"], c["Pc"], c["Pp"], c["com"], [], H)
    assert set(empty) == set(E.SPAN_FIELDS) and all(v.shape[0] == 0 for v in empty.values())
    assert empty["span_positions_displacement_cov"].shape == (0, 2, 3, 3) and empty["span_frames"].shape == (0, 2)


def test_one_camera_knows_the_displacement_better_than_the_positions(oracle):
    """the stated condition of the feature: on "mono" at ridge 0, span (10, 30), base coordinates 0 and 1, the reference's variance of u_b - u_a
    is below half the sum of the two variances (0.20 and 0.06 of it); with six cameras the frames are nearly independent"""
    c = CC.oracle_case(oracle, "mono")
    _, _, S = CC.dense_inverse(CC.damped(c["Bk"], 0.0), c["Hk"])
    a, b = 10, 30
    for i in (0, 1):
        ia, ib = a * NX + i, b * NX + i
        ratio = (S[ib, ib] + S[ia, ia] - 2.0 * S[ib, ia]) / (S[ib, ib] + S[ia, ia])
        print(f"mono, span ({a}, {b}), base coordinate {i}: var(u_b - u_a) / (var u_b + var u_a) = {ratio:.3f}")
        assert 0.0 < ratio < 0.5
    # the same through span_uncertainty, with the unit Jacobian of the base position
    P = np.zeros((CC.N_CASE, 3, NX)); P[:, [0, 1, 2], [0, 1, 2]] = 1.0
    d = np.stack([S[n * NX:(n + 1) * NX, n * NX:(n + 1) * NX] for n in range(CC.N_CASE)])
    out = E.span_uncertainty(SC.columns_dense(S, [b]), [b], d, P, P[:, None], np.zeros((CC.N_CASE, 3)), [(a, b)], H)
    indep = np.sqrt(d[a].diagonal()[:2] + d[b].diagonal()[:2])
    assert np.all(out["span_com_displacement_std"][0, :2] < np.sqrt(0.5) * indep)


def test_signatures(lib):
    """the two prototypes of include/cpe.h against the ctypes mirror, the exported symbols and the wrappers (fails without the feature)"""
    assert tuple(abi.COLUMN_COVARIANCE_ENTRIES) == ("cpe_covariance_columns", "cpe_covariance_columns_host")
    assert not set(abi.COLUMN_COVARIANCE_ENTRIES) & set(abi.COVARIANCE_ENTRIES)
    for name in abi.COLUMN_COVARIANCE_ENTRIES:
        fn = getattr(lib, name)                                   # AttributeError when the symbol is missing
        assert _prototype(name) == tuple(abi.ENTRIES[name]) == ("h", "i", "i", "ip", "p", "p", "p", "i", "ip", "p"), name
        assert list(fn.argtypes) == abi.argtypes(name), name
    for method in ("covariance_columns", "covariance_columns_host"):
        assert callable(getattr(_lib.Handle, method))


def test_null_arguments_are_refused(lib):
    """a null handle: CPE_BAD_ARG with the reason, before anything is dereferenced"""
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    one = (C.c_int32 * 1)(0)
    for name in abi.COLUMN_COVARIANCE_ENTRIES:
        assert getattr(lib, name)(None, 1, 1, None, p, p, p, 1, one, p) == abi.BAD_ARG
        assert b"null argument" in lib.cpe_last_error() and name.encode() + b":" in lib.cpe_last_error()


def test_keyword():
    """uncertainty_spans without uncertainty=True: ValueError in all five functions, before the estimator is looked at; a bad pair: ValueError when
    the spans are resolved, before anything is prepared or solved"""
    for fn, arg in ((E.estimate_kinematics, None), (E.estimate_kinematics_batch, [None]), (E.estimate_kinetics, None),
                    (E.estimate_kinetics_batch, [None]), (E.estimate_grf, None)):
        for spans in (True, [(0, 5)]):
            with pytest.raises(ValueError, match="uncertainty_spans needs uncertainty=True"):
                fn(arg, uncertainty_spans=spans)
    assert E.resolve_spans(None, 10) is None
    assert E.resolve_spans(True, 10) == [(0, 9)] and E.resolve_spans(True, 2) == [(0, 1)] and E.resolve_spans(True, 1) == []
    assert E.resolve_spans([(0, -1), (2, 9), (-3, -2)], 10) == [(0, 9), (2, 9), (7, 8)]
    for bad in ([(5, 5)], [(6, 2)], [(0, 10)], [(-11, 3)], [(0, -10)], [(0, 1), (3,)], [4]):
        with pytest.raises(ValueError, match="uncertainty_spans"):
            E.resolve_spans(bad, 10)
    # through the public functions: the estimator's frame range is all that is read before the refusal
    stub = SimpleNamespace(params=SimpleNamespace(start_frame=4, end_frame=14), scene=None, skeleton=None)
    for fn, arg in ((E.estimate_kinematics, stub), (E.estimate_kinematics_batch, [stub]), (E.estimate_kinetics, stub), (E.estimate_kinetics_batch, [stub]),
                    (E.estimate_grf, stub)):
        for bad in ([(3, 3)], [(0, 10)]):
            with pytest.raises(ValueError, match="does not satisfy"):
                fn(arg, uncertainty=True, uncertainty_spans=bad)
