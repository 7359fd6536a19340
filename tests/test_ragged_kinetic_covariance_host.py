"""Posterior covariance of batched and ragged physics-based solves (cpe_covariance_kinetic_ragged, include/cpe.h), the part that needs no GPU:
exported symbols and their ctypes mirror, the refusals of the C ABI that need no handle, the padding and unpadding of the _lib method, the inputs
of the GPU tests (positive definite at ridge 0, so that no bit-equality there compares zeros with zeros) and what estimate_kinetics_batch refuses
before any device work.  The HIP side is tests/test_gpu_ragged_kinetic_covariance.py."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

import kinetic_cov_compare as KV
import lm_compare as LC
import ragged_kinetic_cov_cases as RC
from cheetah_pose_estimation_amd import _lib, abi, estimator as E, skeleton

NAMES = ("cpe_covariance_kinetic_ragged", "cpe_covariance_kinetic_ragged_host")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_symbols_and_ctypes_mirror(lib):
    """the library exports both entries, the signature table names each once and gives them the plain pair's 20 arguments plus model, n_frames
    (fails without the feature)"""
    for name in NAMES:
        assert hasattr(lib, name) and name in abi.ENTRIES
        assert len(getattr(lib, name).argtypes) == 22
        plain = abi.ENTRIES[name.replace("_ragged", "")]
        assert abi.ENTRIES[name] == plain[:4] + ("ip", "ip") + plain[4:]
    assert set(abi.KINETIC_COVARIANCE_ENTRIES) == {"cpe_covariance_kinetic", "cpe_covariance_kinetic_host"}


def test_header_declares_both_entries():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpe.h")).read()
    for name in NAMES:
        assert f"cpe_status {name}(" in text


def test_lib_methods_and_estimator_arguments():
    """_lib.Handle has both methods; estimate_kinetics_batch takes uncertainty / uncertainty_ridge, off by default (fails without the feature)"""
    assert hasattr(_lib.Handle, "covariance_kinetic_ragged") and hasattr(_lib.Handle, "covariance_kinetic_ragged_host")
    p = inspect.signature(E.estimate_kinetics_batch).parameters
    assert p["uncertainty"].default is False and p["uncertainty_ridge"].default == 0.0


def test_refusals(lib):
    """bad ridge, null options, null stance, null model / n_frames, two variant pointers: CPE_BAD_ARG with the reason, before the device is opened
    (no handle is needed to get there); valid arguments get as far as the handle"""
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    dummy = (C.c_double * 4)()                     # never read: every call below is refused before its arrays are looked at
    p = C.addressof(dummy)
    mo, nf = (C.c_int32 * 1)(0), (C.c_int32 * 1)(4)
    none = (None, None, None)
    for name in NAMES:
        fn = getattr(lib, name)
        call = lambda opt, stance, var, ridge, model=mo, frames=nf: fn(None, opt, 1, 4, model, frames, None, None, None, stance, var[0], var[1], var[2],
                                                                       ridge, None, None, None, None, None, None, None, None)
        for ridge in (-1e-9, float("nan"), float("inf")):
            assert call(C.byref(ko), p, none, ridge) == abi.BAD_ARG
            assert b"ridge" in lib.cpe_last_error()
        assert call(None, p, none, 0.0) == abi.BAD_ARG
        assert b"options" in lib.cpe_last_error()
        assert call(C.byref(ko), None, none, 0.0) == abi.BAD_ARG
        assert b"stance" in lib.cpe_last_error()
        for model, frames in ((None, nf), (mo, None), (None, None)):
            assert call(C.byref(ko), p, none, 0.0, model, frames) == abi.BAD_ARG
            assert b"null model / n_frames" in lib.cpe_last_error() and name.encode() in lib.cpe_last_error()
        for var in ((p, p, None), (p, None, p), (None, p, p), (p, p, p)):
            assert call(C.byref(ko), p, var, 0.0) == abi.BAD_ARG
            assert b"at most one" in lib.cpe_last_error()
        assert call(C.byref(ko), p, (p, None, None), 1e-6) == abi.BAD_ARG          # (no handle)
        assert b"null" in lib.cpe_last_error()


# ---- padding and unpadding of the _lib method, on made-up arrays ------------------------------------------------------------------------------
def _seq(rng, N, C_, L=24, nq=54):
    return dict(q=rng.standard_normal((N, nq)), meas=rng.standard_normal((N, C_, L, 2)), weight=rng.random((N, C_, L)),
                stance=rng.integers(0, 2, (N, 4)).astype(np.int32), tau_box=rng.standard_normal((N, 22, 2)))


def _view(addr, shape, dtype=np.float64):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_int32 if dtype == np.int32 else C.c_double)), shape=(n,)).reshape(shape)


def _fake_handle(model_n_cams, seen):
    """a Handle without a device whose library records the arguments of cpe_covariance_kinetic_ragged_host and fills every output with
    1000 b + n (so that what comes back is what was padded, cut to each sequence's own frames)"""
    h = _lib.Handle.__new__(_lib.Handle)
    h._h = C.c_void_p()
    h.n_cams, h.model_n_cams, h.L, h.nq, h.pb = max(model_n_cams), list(model_n_cams), 24, 54, 3
    h.sk = skeleton.build_skeleton("phantom", 24)

    def entry(handle, ko, B, N, model, n_frames, q, meas, weight, stance, grf_fixed, tau_box, grf_box, ridge, cov_diag, cov_off, cov_pos, cov_f, f, meta,
              L, status):
        cm = h.n_cams
        seen.update(B=B, N=N, ridge=ridge, model=list(model)[:B], n_frames=list(n_frames)[:B], ko=[ko[k].ground_height for k in range(len(model_n_cams))],
                    q=_view(q, (B, N, 54)).copy(), meas=_view(meas, (B, N, cm, 24, 2)).copy(), weight=_view(weight, (B, N, cm, 24)).copy(),
                    stance=_view(stance, (B, N, 4), np.int32).copy(), grf_fixed=grf_fixed, grf_box=grf_box,
                    tau_box=None if tau_box is None else _view(tau_box, (B, N, 22, 2)).copy(), L=L)
        fill = (1000.0 * np.arange(B)[:, None] + np.arange(N)[None, :])
        for addr, tail, dt in ((cov_diag, (28, 28), np.float64), (cov_off, (3, 28, 28), np.float64), (cov_pos, (24, 3, 3), np.float64),
                               (cov_f, (64, 64), np.float64), (f, (64,), np.float64), (meta, (65,), np.int32), (L, (4, 28, 28), np.float64)):
            if addr is not None:
                v = _view(addr, (B, N) + tail, dt)
                v[...] = fill.reshape((B, N) + (1,) * len(tail))
        for b in range(B):
            status[b] = abi.NUMERICAL if b == 1 else abi.OK
        return abi.NUMERICAL
    h.lib = types.SimpleNamespace(cpe_covariance_kinetic_ragged_host=entry)
    return h


@pytest.mark.parametrize("want_L", [False, True])
def test_padding_and_unpadding_of_the_host_method(want_L):
    rng = np.random.default_rng(11)
    seen = {}
    h = _fake_handle((6, 4, 2), seen)
    seqs = [_seq(rng, n, c) for n, c in ((7, 2), (12, 4), (3, 6), (9, 4))]
    model_of = [2, 1, 0, 1]
    kos = []
    for k in range(3):                                         # told apart by a field that is free per model
        ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
        ko.ground_height = 0.25 * (k + 1)
        kos.append(ko)
    lists = lambda key: [s[key] for s in seqs]
    r = h.covariance_kinetic_ragged_host(lists("q"), lists("meas"), lists("weight"), lists("stance"), kos, model_of, 1e-6, tau_box=lists("tau_box"), want_L=want_L)
    # what the entry was given: N_max frames, C_max cameras, zero tails, the option array in model order
    assert (seen["B"], seen["N"], seen["ridge"]) == (4, 12, 1e-6)
    assert seen["model"] == model_of and seen["n_frames"] == [7, 12, 3, 9] and seen["ko"] == [0.25, 0.5, 0.75]
    assert seen["grf_fixed"] is None and seen["grf_box"] is None and (seen["L"] is not None) == want_L
    for b, s in enumerate(seqs):
        n, c = s["q"].shape[0], s["meas"].shape[1]
        assert np.array_equal(seen["q"][b, :n], s["q"]) and not seen["q"][b, n:].any()
        assert np.array_equal(seen["meas"][b, :n, :c], s["meas"]) and not seen["meas"][b, n:].any() and not seen["meas"][b, :, c:].any()
        assert np.array_equal(seen["weight"][b, :n, :c], s["weight"]) and not seen["weight"][b, n:].any() and not seen["weight"][b, :, c:].any()
        assert np.array_equal(seen["stance"][b, :n], s["stance"]) and not seen["stance"][b, n:].any()
        assert np.array_equal(seen["tau_box"][b, :n], s["tau_box"]) and not seen["tau_box"][b, n:].any()
    # what comes back: per-sequence lists cut to the sequence's own frames, the statuses, the padded arrays
    keys = RC.KEYS if want_L else RC.KEYS[:-1]
    assert set(r) == set(keys) | {"status", "seq_status", "padded"} and set(r["padded"]) == set(keys)
    assert r["status"] == abi.NUMERICAL and r["seq_status"] == [abi.OK, abi.NUMERICAL, abi.OK, abi.OK]
    tails = dict(cov_diag=(28, 28), cov_off=(3, 28, 28), cov_pos=(24, 3, 3), cov_f=(64, 64), f=(64,), meta=(65,), L=(4, 28, 28))
    for k in keys:
        assert r["padded"][k].shape == (4, 12) + tails[k] and len(r[k]) == 4
        for b, s in enumerate(seqs):
            n = s["q"].shape[0]
            assert r[k][b].shape == (n,) + tails[k] and r[k][b].flags["C_CONTIGUOUS"]
            assert r[k][b].dtype == (np.int32 if k == "meta" else np.float64)
            assert np.array_equal(r[k][b].reshape(n, -1)[:, 0], 1000 * b + np.arange(n))


def test_host_method_checks_its_lists_before_any_call():
    h = _fake_handle((6, 4), {})
    h.lib = None                                               # any call into the library would fail on this
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    rng = np.random.default_rng(1)
    a, b = _seq(rng, 9, 6), _seq(rng, 5, 4)
    args = lambda *s: ([x["q"] for x in s], [x["meas"] for x in s], [x["weight"] for x in s], [x["stance"] for x in s])
    with pytest.raises(ValueError, match="per sequence"):
        h.covariance_kinetic_ragged_host(*args(a, b), [ko, ko], [0])
    with pytest.raises(ValueError, match="at most one"):
        h.covariance_kinetic_ragged_host(*args(a, b), [ko, ko], [0, 1], grf_fixed=[np.zeros((9, 4, 3)), np.zeros((5, 4, 3))], tau_box=[a["tau_box"], b["tau_box"]])
    with pytest.raises(ValueError, match="one kinetic options struct per model"):
        h.covariance_kinetic_ragged_host(*args(a, b), [ko], [0, 1])
    with pytest.raises(ValueError, match="out of range"):
        h.covariance_kinetic_ragged_host(*args(a, b), [ko, ko], [0, 2])
    with pytest.raises(ValueError, match="shapes of its model"):
        h.covariance_kinetic_ragged_host(*args(a, b), [ko, ko], [1, 1])          # sequence 0 has 6 cameras, model 1 has 4
    with pytest.raises(ValueError, match="per sequence"):
        h.covariance_kinetic_ragged_host(*args(a, b), [ko, ko], [0, 1], tau_box=[a["tau_box"]])
    with pytest.raises(ValueError, match="at most one"):
        h.covariance_kinetic_ragged([ko, ko], [0, 1], [9, 5], None, None, None, None, 0.0, None, grf_fixed=object(), grf_box=object())


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------------------
def _smallest(oracle, c):
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, 0.0)
    A = LC.dense(Ad, Hk)
    np.linalg.cholesky(A)
    return np.linalg.eigvalsh(A)[0], min(np.linalg.eigvalsh(M)[0] for _, M in nodes.values()), sorted(set(int(n) for n in R["meta"][2:, 0]))


def test_inputs_of_the_gpu_tests_are_positive_definite(oracle):
    """the reduced band and every node's H_ff at ridge 0, by oracle.kinetic_system, for the four sequences of the batch and for the 7- and 5-frame
    cuts of "seed7"; the node counts the GPU tests rely on (arabia-02: flight nodes, na = 48)"""
    seqs = RC.sequences(oracle)
    assert [c["q"].shape[0] for c in seqs] == list(RC.SEQ_FRAMES)
    seed7 = KV.gallop_case(oracle, "seed7")
    cases = [("base", seqs[0], {51, 54}), ("six", seqs[1], {51, 54}), ("seed7[:9]", seqs[2], {51, 54}), ("seed7[:7]", RC.cut(seed7, 7), {51, 54}),
             ("seed7[:5]", RC.cut(seed7, 5), {51, 54}), ("arabia-02", seqs[3], {48, 51})]
    for name, c, counts in cases:
        eb, ef, na = _smallest(oracle, c)
        print(f"{name}: smallest eigenvalue of the reduced band {eb:.3g}, of any node's H_ff {ef:.3g}; na {na}")
        assert eb > 0.0 and ef > 0.0, name
        assert set(na) <= counts and (name != "arabia-02" or set(na) == counts), (name, na)


@pytest.mark.parametrize("variant", ["grf_fixed", "tau_box"])
def test_variant_inputs_of_the_gpu_tests_are_positive_definite(oracle, variant):
    """the same for the batch with per-sequence prescribed foot forces (no foot rows: na = motors + 26 = 48) and torque boxes"""
    for b, c in enumerate(RC.sequences(oracle)):
        v = RC.with_variant(c, variant)
        assert v["var"][variant].shape[0] == RC.SEQ_FRAMES[b]
        eb, ef, na = _smallest(oracle, v)
        print(f"sequence {b} {variant}: smallest eigenvalue of the reduced band {eb:.3g}, of any node's H_ff {ef:.3g}; na {na}")
        assert eb > 0.0 and ef > 0.0, (b, variant)
        assert variant != "grf_fixed" or na == [48]


def test_models_of_the_batch_can_share_a_handle(oracle):
    """the three models have one shape, one set of shared solver options and kinetic options of one shape: what cpe_create_multi and
    cpe_covariance_kinetic_ragged ask of them"""
    ms = RC.models(oracle)
    assert len({_lib.shape_signature(m["sk"]) for m in ms}) == 1
    assert len({_lib.shared_options_signature(m["opts"]) for m in ms}) == 1
    assert len({_lib.kinetic_shape_signature(m["ko"]) for m in ms}) == 1
    assert [len(m["cams"]) for m in ms] == [2, 6, 4]
    assert ms[2]["ko"].zvel_max != ms[0]["ko"].zvel_max and ms[2]["opts"].h != ms[0]["opts"].h


# ---- the estimator ------------------------------------------------------------------------------------------------------------------------------
def test_batch_refuses_the_3d_kinematic_cost_before_any_device_work():
    """estimate_kinetics_batch(uncertainty=True, use_2d_reprojections=False): NotImplementedError before an estimator is looked at"""
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"estimator.{name} was read")
    with pytest.raises(NotImplementedError, match="use_2d_reprojections"):
        E.estimate_kinetics_batch([Untouchable()], uncertainty=True, use_2d_reprojections=False)
    with pytest.raises(NotImplementedError, match="use_2d_reprojections"):
        E.estimate_kinetics_batch([Untouchable()], uncertainty=True, use_2d_reprojections=False, ragged=True)
