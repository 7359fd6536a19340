"""The ragged physics-based solve without a GPU: exported symbols, refusals before any device call, the pad / unpad helpers and the grouping
of estimate_kinetics_batch(ragged=True)."""
import ctypes as C

import numpy as np
import pytest

from cheetah_pose_estimation_amd import _lib, abi, estimator as E, skeleton, synth

ANIMALS = (("phantom", 120.0, False), ("jules", 90.0, False), ("arabia-02", 200.0, True), ("shiraz-02", 200.0, True))


def test_symbols_are_exported():
    lib = _lib.load()
    for sym in ("cpe_solve_kinetic_ragged", "cpe_solve_kinetic_ragged_host"):
        assert getattr(lib, sym) is not None


def test_null_handle_is_refused():
    lib = _lib.load()
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    mo, nf = (C.c_int32 * 1)(0), (C.c_int32 * 1)(8)
    for fn in (lib.cpe_solve_kinetic_ragged, lib.cpe_solve_kinetic_ragged_host):
        st = fn(None, C.byref(ko), 1, 8, mo, nf, *([None] * 16), (abi.Stats * 1)(), (abi.KineticStats * 1)())
        assert st == abi.BAD_ARG and b"null" in lib.cpe_last_error()


def _seq(rng, N, C_, L=24, nq=54, nm=22):
    return dict(q_init=rng.standard_normal((N, nq)), meas=rng.standard_normal((N, C_, L, 2)), weight=rng.random((N, C_, L)),
                stance=rng.integers(0, 2, (N, 4)).astype(np.int32), force=rng.standard_normal((N, nm, 2)))


def test_pad_unpad_round_trip_and_zero_fill():
    rng = np.random.default_rng(3)
    seqs = [_seq(rng, n, c) for n, c in ((7, 6), (12, 4), (3, 1))]
    p = _lib.pad_kinetic([s["q_init"] for s in seqs], [s["meas"] for s in seqs], [s["weight"] for s in seqs], [s["stance"] for s in seqs],
                         [s["force"] for s in seqs])
    assert p["lens"] == [7, 12, 3]
    assert p["q_init"].shape == (3, 12, 54) and p["meas"].shape == (3, 12, 6, 24, 2) and p["weight"].shape == (3, 12, 6, 24)
    assert p["stance"].shape == (3, 12, 4) and p["stance"].dtype == np.int32 and p["force"].shape == (3, 12, 22, 2)
    for b, s in enumerate(seqs):
        n, c = s["q_init"].shape[0], s["meas"].shape[1]
        assert np.array_equal(p["q_init"][b, :n], s["q_init"]) and not p["q_init"][b, n:].any()
        assert np.array_equal(p["meas"][b, :n, :c], s["meas"]) and not p["meas"][b, n:].any() and not p["meas"][b, :, c:].any()
        assert np.array_equal(p["weight"][b, :n, :c], s["weight"]) and not p["weight"][b, :, c:].any() and not p["weight"][b, n:].any()
        assert np.array_equal(p["stance"][b, :n], s["stance"]) and not p["stance"][b, n:].any()
        assert np.array_equal(p["force"][b, :n], s["force"]) and not p["force"][b, n:].any()
    assert _lib.pad_kinetic([s["q_init"] for s in seqs], [s["meas"] for s in seqs], [s["weight"] for s in seqs],
                            [s["stance"] for s in seqs])["force"] is None
    # outputs: padded [B, N_max, ...] -> the sequences' own frames and cameras
    padded = dict(q=p["q_init"], meas_err=p["meas"], tau=p["force"][..., 0])
    u = _lib.unpad_kinetic(padded, p["lens"], [6, 4, 1])
    assert set(u) == {"q", "meas_err", "tau"}
    for b, s in enumerate(seqs):
        assert np.array_equal(u["q"][b], s["q_init"]) and np.array_equal(u["meas_err"][b], s["meas"])
        assert np.array_equal(u["tau"][b], s["force"][..., 0]) and u["tau"][b].flags["C_CONTIGUOUS"]


def _key(animal, fps, kin, variant="free", pri=None, device=0, opts=None, ko=None):
    sk = skeleton.without_motion_model(skeleton.build_skeleton(animal, 24, kinetic_dataset=kin))
    opts = opts if opts is not None else abi.default_options(fps)
    ko = ko if ko is not None else abi.default_kinetic_options(skeleton.dyn_options(animal), fps, kin)
    return E.kinetic_ragged_group_key(sk, opts, ko, pri, variant, device)


def test_group_key_joins_skeletons_and_rigs_and_separates_the_rest():
    keys = {_key(a, fps, kin) for a, fps, kin in ANIMALS}
    assert len(keys) == 1                                                # four skeletons, 120 / 90 / 200 fps, both kinetic-option sets
    base = _key("phantom", 120.0, False)
    assert _key("phantom", 120.0, False, variant="fixed") != base
    assert _key("phantom", 120.0, False, variant="force_box") != _key("phantom", 120.0, False, variant="fixed")
    from cheetah_pose_estimation_amd import priors
    assert _key("phantom", 120.0, False, pri=priors.load_priors(pose=True, motion=False)) != base
    o = abi.default_options(120.0); o.max_iter = 77
    assert _key("phantom", 120.0, False, opts=o) != base
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0); ko.dyn.n_motors -= 1
    assert _key("phantom", 120.0, False, ko=ko) != base
    assert _key("phantom", 120.0, False, device=1) != base
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0); ko.slack_lo, ko.slack_hi, ko.inner_iterations = -0.1, 0.1, 12
    assert _key("phantom", 120.0, False, ko=ko) == base                  # free per model


def _fake_handle(model_n_cams=(6, 4)):
    """a Handle without a device: the argument checks of solve_kinetic_ragged_host run before anything touches it"""
    h = _lib.Handle.__new__(_lib.Handle)
    h._h = C.c_void_p()
    h.n_cams, h.model_n_cams, h.L, h.nq = max(model_n_cams), list(model_n_cams), 24, 54
    h.sk = skeleton.build_skeleton("phantom", 24)
    h.lib = None                                                         # any device call would fail on this
    return h


def test_host_argument_validation_raises_before_any_device_call():
    h = _fake_handle()
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    rng = np.random.default_rng(1)
    a, b = _seq(rng, 9, 6), _seq(rng, 5, 4)
    args = lambda *s: ([x["q_init"] for x in s], [x["meas"] for x in s], [x["weight"] for x in s], [x["stance"] for x in s])
    with pytest.raises(ValueError, match="per sequence"):
        h.solve_kinetic_ragged_host([ko, ko], [a["q_init"], b["q_init"]], [a["meas"]], [a["weight"], b["weight"]], [a["stance"], b["stance"]], [0, 1])
    with pytest.raises(ValueError, match="per sequence"):
        h.solve_kinetic_ragged_host([ko, ko], *args(a, b), [0])
    with pytest.raises(ValueError, match="at most one"):
        h.solve_kinetic_ragged_host([ko, ko], *args(a, b), [0, 1], grf_fixed=[np.zeros((9, 4, 3)), np.zeros((5, 4, 3))],
                                    tau_box=[a["force"], b["force"]])
    with pytest.raises(ValueError, match="one kinetic options struct per model"):
        h.solve_kinetic_ragged_host([ko], *args(a, b), [0, 1])
    with pytest.raises(ValueError, match="out of range"):
        h.solve_kinetic_ragged_host([ko, ko], *args(a, b), [0, 2])
    with pytest.raises(ValueError, match="shapes of its model"):
        h.solve_kinetic_ragged_host([ko, ko], *args(a, b), [1, 1])          # sequence 0 has 6 cameras, model 1 has 4
    with pytest.raises(ValueError, match="per sequence"):
        h.solve_kinetic_ragged_host([ko, ko], *args(a, b), [0, 1], tau_box=[a["force"]])
    with pytest.raises(ValueError, match="at most one"):
        h.solve_kinetic_ragged(
            [ko, ko], [0, 1], [9, 5], None, None, None, None, None, None, None, None, None, grf_fixed=object(), grf_box=object())


def test_kinetic_shape_signature_reads_the_shared_fields_only():
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    s = _lib.kinetic_shape_signature(ko)
    assert s[0] == 4 and s[2] == 22 and len(s[1]) == 4 and len(s[3]) == len(s[4]) == len(s[5]) == 22
    k2 = abi.default_kinetic_options(skeleton.dyn_options("arabia"), 200.0, True)
    assert _lib.kinetic_shape_signature(k2) == s
    k2.dyn.foot_marker[1] = 3
    assert _lib.kinetic_shape_signature(k2) != s
