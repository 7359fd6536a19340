"""Motion-prior windows of 5 and 6 frames without a GPU: priors.fit_priors fits them (the two fixtures), the ctypes mirror and the C header
agree on the window limit, the oracle reads the wider cpe_priors correctly (its motion term against a numpy statement of
acinoset_misc.py:291-336), and cpe_create takes windows 5 and 6 as far as opening the device while it still refuses 7 and negative windows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REF_TABLE = os.path.join(GOLDEN, "dataset_full_pose_28cols.csv.gz")
FIXTURES = {(3, 5, False): os.path.join(GOLDEN, "priors_k3_w5_dense.npz"), (5, 6, True): os.path.join(GOLDEN, "priors_k5_w6_lasso.npz")}


@pytest.mark.parametrize("k, w, sparse", sorted(FIXTURES))
def test_fit_priors_reproduces_the_fixture(tmp_path, k, w, sparse):
    """the fixtures are priors.fit_priors' own output: the same fit again gives every array number for number.  The one exception is the plain
    least-squares motion model: LAPACK's least-squares driver rounds with the thread count of the BLAS, and this fit's coefficients reach 112, so
    they (and the residual statistics that follow from them) are held to 1e-10 of their largest entry (measured: 9e-12 between 4 threads and all)."""
    pytest.importorskip("sklearn")
    pytest.importorskip("pandas")
    path = priors.fit_priors(k, w, sparse, dataset=REF_TABLE, cache_dir=str(tmp_path))
    assert os.path.basename(path) == os.path.basename(FIXTURES[(k, w, sparse)])
    a, b = np.load(path), np.load(FIXTURES[(k, w, sparse)])
    assert sorted(a.files) == sorted(b.files)
    for f in b.files:
        if not sparse and f in ("lr_coef", "lr_intercept", "lr_error_variance"):
            assert np.abs(a[f] - b[f]).max() <= 1e-10 * np.abs(b[f]).max(), f
        else:
            assert np.array_equal(a[f], b[f]), f
    assert int(a["lr_window"]) == w and a["lr_coef"].shape == (abi.NX, w * abi.NX) and a["gmm_means"].shape == (k, 22)
    if sparse:
        assert np.count_nonzero(a["lr_coef"]) < 0.5 * a["lr_coef"].size                # multi-task lasso: most lags dropped
    else:
        assert np.count_nonzero(a["lr_coef"]) > 0.9 * a["lr_coef"].size


def test_window_limit_of_the_header_and_the_mirror():
    with open(os.path.join(os.path.dirname(HERE), "include", "cpe.h")) as fh:
        m = re.search(r"^#define CPE_MAX_WINDOW\s+(\d+)", fh.read(), re.M)
    assert m is not None
    assert abi.MAX_WINDOW == int(m.group(1)) == 6
    assert C.sizeof(abi.Priors().lr_coef) == abi.NX * abi.MAX_WINDOW * abi.NX * 8


def test_fit_priors_still_refuses_window_7(tmp_path):
    with pytest.raises(NotImplementedError, match="window of 7 frames"):
        priors.fit_priors(5, 7, True, dataset=REF_TABLE, cache_dir=str(tmp_path))


@pytest.mark.parametrize("w", [5, 6])
def test_oracle_motion_term_at_windows_5_and_6(oracle, cams6, w):
    """the motion term of the oracle's objective at a random trajectory equals
    sum_{n >= W} sum_p w_p (x_n - b - coef [x_{n-W}; ...; x_{n-1}])_p^2, x the relative angles of the cost view"""
    path = FIXTURES[(3, 5, False)] if w == 5 else FIXTURES[(5, 6, True)]
    pr = priors.load_priors(path=path)
    assert pr.lr_window == w
    sk = skeleton.build_skeleton("phantom", 24)
    cam1 = (abi.Camera * 1)(cams6[2])
    N = 2 * w + 5
    d = synth.make_batch(sk, cam1, B=1, N=N, seed=17 + w, init_noise=0.05)
    q = d["q_init"][0] + np.random.default_rng(w).normal(0, 0.05, d["q_init"][0].shape)
    f, _, _, terms, qc = oracle.objective(sk, cam1, abi.default_options(), pr, q, d["meas"][0], d["weight"][0])
    x = np.array([oracle.relative_angles(sk, qq) for qq in synth.cost_view_numpy(sk, qc)])
    coef = np.array([[pr.lr_coef[p][j] for j in range(w * abi.NX)] for p in range(abi.NX)])
    b, wt = np.array(pr.lr_b[:abi.NX]), np.array(pr.lr_w[:abi.NX])
    assert not np.array([[pr.lr_coef[p][j] for j in range(w * abi.NX, abi.MAX_WINDOW * abi.NX)] for p in range(abi.NX)]).any()
    motion = sum((wt * (x[n] - (coef @ x[n - w:n].ravel() + b)) ** 2).sum() for n in range(w, N))
    assert motion > 0.0
    assert abs(terms[3] - motion) < 1e-9 * motion, (terms[3], motion)


def _create(lr_window):
    """cpe_create with the window-6 fixture's priors at the given lr_window; returns (status, message), destroys a handle it got"""
    lib = _lib.load()
    pr = priors.load_priors(path=FIXTURES[(5, 6, True)])
    pr.lr_window = lr_window
    sk = skeleton.build_skeleton("phantom", 24)
    cams = synth.make_cameras(1)
    opts = abi.default_options()
    h = C.c_void_p()
    st = lib.cpe_create(C.byref(sk), cams, len(cams), C.byref(opts), C.byref(pr), 0, C.byref(h))
    msg = lib.cpe_last_error().decode()
    if st == abi.OK:
        lib.cpe_destroy(h)
    return st, msg


@pytest.mark.parametrize("w", [5, 6])
def test_create_takes_windows_5_and_6(w):
    # valid priors get as far as opening the device: OK with a GPU, NO_DEVICE without one -- never BAD_ARG
    st, msg = _create(w)
    assert st in (abi.OK, abi.NO_DEVICE), msg


@pytest.mark.parametrize("w", [7, -1])
def test_create_refuses_windows_out_of_range(w):
    st, msg = _create(w)
    assert st == abi.BAD_ARG
    assert f"window {w} out of range" in msg, msg
