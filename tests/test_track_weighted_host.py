"""The 3D kinematic cost weighted by the kinematic posterior (estimate_kinetics(track_weights="posterior"); cpe_track_precision,
cpe_solve_kinetic_tracked_weighted*) without a GPU: the exported symbols, the numpy reference (tests/track_compare.py) against itself and against
the diagonal form's reference, the padding helper, the grouping of estimate_kinetics_batch and the estimator's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import track_compare as TC
from cheetah_pose_estimation_amd import _lib, abi, estimator as E, skeleton, synth
from test_gpu_tracked import _numpy_term


def _sk(animal="phantom"):
    return skeleton.without_motion_model(skeleton.build_skeleton(animal, 24))


def _spd_cov(rng, shape):
    """u-space covariance blocks with standard deviations over two decades"""
    A = rng.standard_normal(tuple(shape) + (28, 28)) / np.sqrt(28.0)
    S = A @ np.swapaxes(A, -1, -2) + 0.5 * np.eye(28)
    s = 10.0 ** rng.uniform(-3.0, -1.0, tuple(shape) + (28,))
    return s[..., :, None] * S * s[..., None, :]


def test_symbols_are_exported_and_a_null_handle_is_refused():
    lib = _lib.load()
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    W = np.zeros((1, 8, 28, 28))
    mo, nf = (C.c_int32 * 1)(0), (C.c_int32 * 1)(8)
    tail = [*([None] * 17), (abi.Stats * 1)(), (abi.KineticStats * 1)()]
    for name in ("cpe_solve_kinetic_tracked_weighted", "cpe_solve_kinetic_tracked_weighted_host"):
        assert getattr(lib, name)(None, C.byref(ko), W.ctypes.data, 1, 8, *tail) == abi.BAD_ARG, name
        assert b"null" in lib.cpe_last_error()
    for name in ("cpe_solve_kinetic_tracked_weighted_ragged", "cpe_solve_kinetic_tracked_weighted_ragged_host"):
        assert getattr(lib, name)(None, C.byref(ko), W.ctypes.data, 1, 8, mo, nf, *tail) == abi.BAD_ARG, name
    assert lib.cpe_eval_normal_tracked_weighted(None, W.ctypes.data, 1, 8, *([None] * 7)) == abi.BAD_ARG
    for name in ("cpe_track_precision", "cpe_track_precision_host"):
        assert getattr(lib, name)(None, 1, 8, None, None, W.ctypes.data, 1.0, W.ctypes.data) == abi.BAD_ARG, name
    for name in ("track_precision", "track_precision_host", "solve_kinetic_tracked_weighted", "solve_kinetic_tracked_weighted_host",
                 "solve_kinetic_tracked_weighted_ragged_host"):
        assert callable(getattr(_lib.Handle, name)), name


def test_reference_precision_inverts_the_x_space_covariance():
    """2 W C / scale = I for the numpy reference, at two scales, to the accuracy the blocks' condition allows"""
    sk = _sk()
    cov = _spd_cov(np.random.default_rng(1), (2, 5))
    C_x = TC.x_covariance(sk, cov)
    assert np.array_equal(C_x.shape, cov.shape) and np.abs(C_x - np.swapaxes(C_x, -1, -2)).max() <= 1e-15 * np.abs(C_x).max()
    for scale in (1.0, 37.5):
        W = TC.precision(sk, cov, scale)
        bound = 64 * np.finfo(float).eps * np.linalg.cond(C_x)
        assert (TC.precision_residual(W, C_x, scale) <= bound).all()
    assert np.allclose(TC.precision(sk, cov, 4.0), 4.0 * TC.precision(sk, cov, 1.0), rtol=1e-14, atol=0.0)


def test_reference_term_with_diagonal_weights_is_the_diagonal_forms():
    """W = diag(w): T_n, gradient and block of the numpy reference == _numpy_term of tests/test_gpu_tracked.py"""
    for animal in ("phantom", "jules"):
        sk = _sk(animal)
        rng = np.random.default_rng(3)
        q = synth.q_from_u(sk, 0.3 * rng.standard_normal((2, 4, abi.NX)))
        qt = synth.q_from_u(sk, 0.3 * rng.standard_normal((2, 4, abi.NX)))
        w = abi.default_track_weights() * (1.0 + rng.random(abi.NX))
        T0, g0, H0 = _numpy_term(sk, q, qt, w)
        T1, g1, H1 = TC.weighted_term(sk, q, qt, np.broadcast_to(np.diag(w), (2, 4, 28, 28)))
        assert np.abs(T1 - T0).max() <= 1e-13 * np.abs(T0).max()
        assert np.abs(g1 - g0).max() <= 1e-13 * np.abs(g0).max()
        assert np.abs(H1 - H0).max() <= 1e-13 * np.abs(H0).max()


def test_reference_gradient_equals_central_differences():
    """gradient 2 X^T W d against central differences of T over the reduced coordinates u, and the block against those of the gradient"""
    sk = _sk()
    rng = np.random.default_rng(7)
    W = TC.random_spd(rng, ())
    assert np.array_equal(W, W.T)
    u, ut = 0.3 * rng.standard_normal(abi.NX), 0.3 * rng.standard_normal(abi.NX)
    qt = synth.q_from_u(sk, ut)
    f = lambda v: TC.weighted_term(sk, synth.q_from_u(sk, v), qt, W)
    T, g, H = f(u)
    h = 1e-5
    gn, Hn = np.empty(abi.NX), np.empty((abi.NX, abi.NX))
    for j in range(abi.NX):
        e = np.zeros(abi.NX); e[j] = h
        (Tp, gp, _), (Tm, gm, _) = f(u + e), f(u - e)
        gn[j], Hn[:, j] = (Tp - Tm) / (2 * h), (gp - gm) / (2 * h)
    assert T > 0.0
    assert np.abs(gn - g).max() <= 1e-7 * max(1.0, np.abs(g).max())              # T is quadratic in u: central differences are exact up to rounding
    assert np.abs(Hn - H).max() <= 1e-7 * np.abs(H).max() and np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()


def test_pad_track_W_pads_like_the_other_inputs():
    rng = np.random.default_rng(5)
    lens = (7, 12, 3)
    Ws = [TC.random_spd(rng, (n,)) for n in lens]
    P = _lib.pad_track_W(Ws, lens)
    assert P.shape == (3, 12, 28, 28) and P.dtype == np.float64 and P.flags["C_CONTIGUOUS"]
    for b, n in enumerate(lens):
        assert np.array_equal(P[b, :n], Ws[b]) and not P[b, n:].any()
    assert np.array_equal(_lib.pad_track_W(Ws), P)
    with pytest.raises(ValueError, match="frames"):
        _lib.pad_track_W(Ws, (7, 11, 3))
    with pytest.raises(ValueError, match="track_W"):
        _lib.pad_track_W([np.zeros((4, 28, 27))])


def test_group_key_separates_the_weighted_mode():
    sk = _sk()
    opts = abi.default_options(120.0)
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    kt = E.kinetic_ragged_group_key(sk, opts, ko, None, "free", 0, tracked=True)
    kp = E.kinetic_ragged_group_key(sk, opts, ko, None, "free", 0, tracked=True, track_weights="posterior")
    k2 = E.kinetic_ragged_group_key(sk, opts, ko, None, "free", 0)
    assert len({kt, kp, k2}) == 3
    assert kt == E.kinetic_ragged_group_key(sk, opts, ko, None, "free", 0, tracked=True, track_weights="reference")     # existing calls compare as before
    assert kp == E.kinetic_ragged_group_key(_sk("jules"), abi.default_options(90.0), abi.default_kinetic_options(skeleton.dyn_options("jules"), 90.0),
                                            None, "free", 0, tracked=True, track_weights="posterior")


def test_estimator_refusals(tmp_path):
    """"posterior" needs use_2d_reprojections=False, an unknown string is refused the same way (both before the estimator is looked at), and a
    missing uncertainty.npz names its path and the call that writes it"""
    for entry in (E.estimate_kinetics, lambda est, **kw: E.estimate_kinetics_batch([est], **kw)):
        with pytest.raises(ValueError, match="use_2d_reprojections=False"):
            entry(None, use_2d_reprojections=True, track_weights="posterior")
        with pytest.raises(ValueError, match="track_weights"):
            entry(None, use_2d_reprojections=False, track_weights="covariance")
        with pytest.raises(ValueError, match="track_scale"):
            entry(None, use_2d_reprojections=False, track_weights="posterior", track_scale=0.0)
    pickle_path = os.path.join(str(tmp_path), "fte_kinematic", "fte.pickle")
    with pytest.raises(FileNotFoundError) as err:
        E.load_posterior_blocks(pickle_path, 5)
    assert os.path.join(str(tmp_path), "fte_kinematic", "uncertainty.npz") in str(err.value)
    assert "estimate_kinematics(uncertainty=True)" in str(err.value)
    os.makedirs(os.path.dirname(pickle_path))
    cov = _spd_cov(np.random.default_rng(2), (6,))
    np.savez(os.path.join(os.path.dirname(pickle_path), "uncertainty.npz"), cov_u=cov, ridge=0.0)
    assert np.array_equal(E.load_posterior_blocks(pickle_path, 5), cov[:5])
    with pytest.raises(ValueError, match="cov_u"):
        E.load_posterior_blocks(pickle_path, 7)
