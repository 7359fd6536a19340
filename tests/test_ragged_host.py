"""Ragged batches without a GPU: cpe_create_multi refuses models of different shapes before it opens the device, and the estimator's ragged
grouping key puts the reference's four skeletons and both rigs into one group."""
import ctypes as C

import pytest

from cheetah_pose_estimation_amd import _lib, abi, estimator, priors, skeleton, synth

ANIMALS = (("phantom", False), ("jules", False), ("arabia-02", True), ("shiraz-02", True))


def _model(animal, kin):
    sk = skeleton.build_skeleton(animal, 24, kinetic_dataset=kin)
    return sk, synth.make_cameras(4 if kin else 6), abi.default_options(200.0 if kin else 120.0)


def _create_multi(models):
    """cpe_create_multi on the given (skeleton, cameras, options) models; returns (status, message), destroys a handle it got"""
    lib = _lib.load()
    n = len(models)
    sks = (abi.Skeleton * n)(*[m[0] for m in models])
    cams = (abi.Camera * (n * abi.MAX_CAMS))()
    for k, (_, cl, _) in enumerate(models):
        for c in range(len(cl)):
            cams[k * abi.MAX_CAMS + c] = cl[c]
    ncam = (C.c_int32 * n)(*[len(m[1]) for m in models])
    ops = (abi.Options * n)(*[m[2] for m in models])
    h = C.c_void_p()
    st = lib.cpe_create_multi(n, sks, cams, ncam, ops, None, 0, C.byref(h))
    msg = lib.cpe_last_error().decode()
    if st == abi.OK:
        lib.cpe_destroy(h)
    return st, msg


def test_four_skeletons_and_both_rigs_pass_the_shape_check():
    # valid models get as far as opening the device: OK with a GPU, NO_DEVICE without one -- never BAD_ARG
    st, msg = _create_multi([_model(a, k) for a, k in ANIMALS])
    assert st in (abi.OK, abi.NO_DEVICE), msg


@pytest.mark.parametrize("what, field", [("n_markers", "n_markers"), ("bound", "bound_b"), ("max_iter", "max_iter")])
def test_create_multi_refuses_a_shape_mismatch(what, field):
    models = [_model(a, k) for a, k in ANIMALS]
    sk, cams, opts = models[2]
    if what == "n_markers":
        sk = skeleton.build_skeleton("arabia-02", 25, kinetic_dataset=True)
    elif what == "bound":
        sk.bound_b[3] = sk.bound_b[3] + 3 if sk.bound_b[3] >= 0 else 3
    else:
        opts.max_iter = opts.max_iter + 1
    models[2] = (sk, cams, opts)
    st, msg = _create_multi(models)
    assert st == abi.BAD_ARG
    assert f"model 2 differs from model 0 in {field}" in msg, msg


def test_create_multi_refuses_bad_arguments():
    lib = _lib.load()
    h = C.c_void_p()
    sk, cams, opts = _model("phantom", False)
    assert lib.cpe_create_multi(0, C.byref(sk), cams, (C.c_int32 * 1)(6), C.byref(opts), None, 0, C.byref(h)) == abi.BAD_ARG
    assert lib.cpe_create_multi(1, None, cams, (C.c_int32 * 1)(6), C.byref(opts), None, 0, C.byref(h)) == abi.BAD_ARG
    cams18 = (abi.Camera * abi.MAX_CAMS)(*cams)
    assert lib.cpe_create_multi(1, C.byref(sk), cams18, (C.c_int32 * 1)(abi.MAX_CAMS + 1), C.byref(opts), None, 0, C.byref(h)) == abi.BAD_ARG
    assert "model 0" in lib.cpe_last_error().decode()


def test_solve_ragged_refuses_a_null_handle():
    lib = _lib.load()
    one = (C.c_int32 * 1)(1)
    assert lib.cpe_solve_ragged(None, 1, 1, one, one, None, None, None, None, None, None, None, None, None) == abi.BAD_ARG
    assert lib.cpe_solve_ragged_host(None, 1, 1, one, one, None, None, None, None, None, None, None, None, None) == abi.BAD_ARG


def test_ragged_group_key_joins_skeletons_and_rigs_and_separates_priors():
    keys = [estimator.ragged_group_key(sk, opts, None, 0) for sk, _, opts in (_model(a, k) for a, k in ANIMALS)]
    assert len(set(keys)) == 1
    sk, _, opts = _model("jules", False)
    pr = priors.load_priors()
    assert estimator.ragged_group_key(sk, opts, pr, 0) != keys[0]
    assert estimator.ragged_group_key(sk, opts, pr, 0) != estimator.ragged_group_key(sk, opts, priors.load_priors(motion=False), 0)
    assert estimator.ragged_group_key(sk, opts, None, 1) != keys[0]
    o2 = abi.default_options(120.0)
    o2.tol_cost = 1e-7
    assert estimator.ragged_group_key(sk, o2, None, 0) != keys[0]
    sk25 = skeleton.build_skeleton("jules", 25)
    assert estimator.ragged_group_key(sk25, opts, None, 0) != keys[0]
