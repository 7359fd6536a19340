"""The shutter-delay terms through cpe_eval_shutter_step, entry by entry against the extended-precision reference of tests/shutter_compare.py:
k_frame_normal's shutter branch (g, Bm, cost, gx, rcb), k_lm_step's collection of gx (g_total), k_shutter_step (step) and k_finalize with
delays (meas_err).  Every case is one call on two sequences (the long one on one), asserts the conditions on its inputs and that the path it
means to exercise is active, and records its worst value per key; test_zz_report prints the worst of the module."""
import numpy as np
import pytest

import frame_compare as FC
import shutter_compare as SC
from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth

pytestmark = pytest.mark.gpu

WORST = {}                                        # (case, key) -> worst value, printed at the end of the module


def _run(name, oracle, gpu_handle_factory):
    """HIP against the reference on a case of shutter_compare.CASES: (HIP's outputs, the reference, the inputs, the handle)"""
    c = SC.case_inputs(name)
    R = SC.case_reference(oracle, name)
    assert SC.conditions_hold(R), (name, R["conditions"])
    assert np.all(c["tau"][:, 0] == 0.0)                                             # the first camera is the reference
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["pr"])
    G = SC.hip_outputs(h, c)
    assert np.all(G["seq"][:, 7] == abi.OK), G["seq"]
    d = SC.discrepancies(G, R, c["keys"])
    print(f"{name}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items()))
    for k, v in d.items():
        WORST[(name, k)] = v
    assert not SC.failures(d), (name, SC.failures(d))
    return G, R, c, h


def _undisplaced(oracle, c):
    """frame_compare's own reference of a case's frames (no delays)"""
    q, meas, weight = FC.flat(c)
    return FC.reference(oracle, c["sk"], c["cams"], c["opts"], c["pr"], q, meas, weight)


def test_plain(oracle, gpu_handle_factory):
    """phantom 25, six fisheye cameras, no prior, N = 5: frames 0 and 1 of either sequence undisplaced, 2 to 4 displaced"""
    G, R, c, _ = _run("plain", oracle, gpu_handle_factory)
    N = c["q"].shape[1]
    n = np.arange(G["gx"].shape[0]) % N
    assert N == 5 and c["pr"] is None and not G["gx"][n < 2].any() and np.all(np.abs(G["gx"][n >= 2]).max(axis=1) > 0)
    assert np.all(G["step"][:, 0] == 0.0) and np.all(G["step"][:, 1:] != 0.0)


def test_zero_delays(oracle, gpu_handle_factory):
    """the same inputs at tau = 0: every key of k_frame_normal meets frame_compare's own reference and tolerances, gx is exactly 0"""
    G, R, c, _ = _run("zero", oracle, gpu_handle_factory)
    assert not c["tau"].any() and np.array_equal(c["q"], FC.case_inputs("plain")["q"])
    d = FC.discrepancies(dict(g=G["g"], Bm=G["Bm"], cost=G["cost"]), FC.case_reference(oracle, "plain"))
    assert not FC.failures(d), d
    assert not G["gx"].any() and np.all(np.isfinite(G["step"])) and np.all(G["step"][:, 0] == 0.0)


@pytest.mark.parametrize("N", SC.SHORT)
def test_short_sequences(N, oracle, gpu_handle_factory):
    """N = 1, 2: nothing is displaced -- gx and step exactly 0, rcb still filled, g / Bm / cost those of the undisplaced reference; N = 3: one
    displaced frame per sequence"""
    G, R, c, _ = _run(f"short{N}", oracle, gpu_handle_factory)
    assert c["q"].shape[:2] == (2, N) and np.all(G["rcb"][..., 3] > 0) and np.all(G["rcb"][..., :3] != 0)       # every camera of every frame
    if N < 3:
        assert not G["gx"].any() and not G["step"].any() and not R["conditions"]["displaced"]
        d = FC.discrepancies(dict(g=G["g"], Bm=G["Bm"], cost=G["cost"]), _undisplaced(oracle, c))
        assert not FC.failures(d), d
    else:
        assert not G["gx"][[0, 1, 3, 4]].any() and G["gx"][2].any() and G["gx"][5].any() and np.all(G["step"][:, 1:] != 0.0)


@pytest.mark.parametrize("Cn", SC.CAMERA_COUNTS)
def test_camera_counts(Cn, oracle, gpu_handle_factory):
    """C = 1: the single step is the exact zero and g carries no tau; 13 and 14 cameras lie on opposite sides of the switch of the kernel's LDS
    layout (the positions start at max(n_camov, CAMW C)), the shutter scratch behind it; 18 is CPE_MAX_CAMS"""
    G, R, c, _ = _run(f"cams{Cn}", oracle, gpu_handle_factory)
    assert len(c["cams"]) == Cn and FC.CAMW * 13 < FC.n_camov(c["sk"]) < FC.CAMW * 14 and max(SC.CAMERA_COUNTS) == abi.MAX_CAMS
    if Cn == 1:
        assert G["step"].shape == (2, 1) and not G["step"].any() and not G["gx"].any()
        d = FC.discrepancies(dict(g=G["g"], Bm=G["Bm"], cost=G["cost"]), _undisplaced(oracle, c))
        assert not FC.failures(d), d
    else:
        assert len(R["conditions"]["displaced_inliers"]) == Cn - 1 and np.all(G["step"][:, 1:] != 0.0)


@pytest.mark.parametrize("mode", [0, 1])
def test_pinhole_rig_with_multipliers(mode, oracle, gpu_handle_factory):
    """the kinetic-dataset rig -- four pinhole cameras with radial distortion and multipliers (1, 1, 0.6, 0.6), 200 fps -- with loss knots 2, 6, 15,
    in both curvature modes"""
    G, R, c, _ = _run(f"knots-c{mode}", oracle, gpu_handle_factory)
    assert (c["opts"].loss_a, c["opts"].loss_b, c["opts"].loss_c) == (2.0, 6.0, 15.0) and c["opts"].h == 1.0 / 200.0 and c["opts"].curvature == mode
    assert [cam.mult for cam in c["cams"]] == [1.0, 1.0, 0.6, 0.6] and all(cam.model == abi.CAM_PINHOLE for cam in c["cams"])


@pytest.mark.parametrize("name", SC.PRIOR_CASES)
def test_pose_prior(name, oracle, gpu_handle_factory):
    """phantom 24 with the packaged mixture and the golden K = 5 one, on 1 and 6 cameras: the shutter scratch sits behind the mixture's.  The
    handles are built WITHOUT a motion prior (shutter_compare.mixture_only), so g and Bm are k_frame_normal's own: k_lr_band does not run"""
    G, R, c, h = _run(name, oracle, gpu_handle_factory)
    assert c["pr"].gmm_k > 0 and c["pr"].lr_window == 0 and h.pb == 3 and len(c["cams"]) == int(name[-1])
    assert np.all(G["cost"][:, 2] != 0.0) and np.abs(R["g_prior"]).max() > 1.0


def test_motion_prior(oracle, gpu_handle_factory):
    """both packaged priors (window 4, half-bandwidth 4) at N = 9 on six cameras: k_lr_band runs between k_frame_normal and k_lm_step, gx is
    collected across the wider band.  g and Bm carry k_lr_band's part here and are not compared; g_total, gx, rcb, step and meas_err are"""
    G, R, c, h = _run("motion", oracle, gpu_handle_factory)
    assert c["pr"].lr_window == 4 and h.pb == 4 and c["q"].shape[:2] == (2, 9) and set(c["keys"]) == {"gx", "rcb", "step", "g_total", "meas_err"}
    assert G["seq"][:, 4].all()                                                      # the motion prior's cost term


def test_active_bounds(oracle, gpu_handle_factory):
    """frame_compare's "bounds" poses under delays: the bounds' atomics and the shutter terms' meet in the same H"""
    G, R, c, _ = _run("bounds", oracle, gpu_handle_factory)
    for b, n, i, side in FC.case_inputs("bounds")["expect_active"]:
        assert R["active"][b * 5 + n, i, side] and G["cost"][b * 5 + n, 1] > 0.0
    assert WORST[("bounds", "sym")] <= SC.TOL["sym"] and WORST[("bounds", "Bm")] <= SC.TOL["Bm"]


def test_long_sequence(oracle, gpu_handle_factory):
    """B = 1, N = 70: frames 66 to 69 are reached only by the second trip of k_shutter_step's frame loop, and leaving them out moves the
    reference's step by more than 100 tolerances"""
    G, R, c, _ = _run("long", oracle, gpu_handle_factory)
    assert c["q"].shape[:2] == (1, SC.LONG_N) and SC.LONG_N > 2 + 64
    W = SC.wrong_reference(oracle, "long", "frames from 66 on left out")
    assert SC.discrepancies(SC.outputs(W), R, ("step",))["step"] > 100 * SC.TOL["step"]


def _equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_batch_independence(gpu_handle_factory):
    """the two sequences of "plain" alone and together, bit-equal in every output: k_frame_normal reads frames n-1 and n-2 through the frame
    pointer, and a sequence must never see its neighbour's; the same call twice is bit-equal too"""
    c = SC.case_inputs("plain")
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["pr"])
    G1, G2 = SC.hip_outputs(h, c), SC.hip_outputs(h, c)
    assert all(np.isfinite(v).all() for v in G1.values()) and all(_equal(G1[k], G2[k]) for k in G1)
    N = c["q"].shape[1]
    for b in range(2):
        Gs = SC.hip_outputs(h, SC.cut(c, b))
        for k in G1:
            assert _equal(G1[k][b:b + 1] if k in ("step", "seq") else G1[k][b * N:(b + 1) * N], Gs[k]), (b, k)


def test_host_twin(gpu_handle_factory):
    """cpe_eval_shutter_step_host returns what the device entry returns, bit for bit"""
    c = SC.case_inputs("short3")
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["pr"])
    Gd, Gh = SC.hip_outputs(h, c), SC.hip_outputs(h, c, host=True)
    assert set(Gd) == set(Gh) and all(_equal(Gd[k], Gh[k]) for k in Gd)


def test_refusals(gpu_handle_factory):
    """CPE_BAD_ARG with the reason in cpe_last_error(), before anything is launched"""
    import torch
    sk, cams = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6)
    h = gpu_handle_factory(sk, cams)
    lib = h.lib
    p = torch.zeros(4096, dtype=torch.float64, device="cuda:0").data_ptr()
    seq = np.zeros(8)
    sp = seq.ctypes.data
    call = lambda hh, q=p, meas=p, weight=p, tau=p, lam=1e-2, s=sp, B=1, N=1: lib.cpe_eval_shutter_step(hh, B, N, q, meas, weight, tau, lam, *[None] * 8, s)
    for kw in (dict(q=None), dict(meas=None), dict(weight=None), dict(tau=None), dict(s=None)):
        assert call(h._h, **kw) == abi.BAD_ARG and b"null argument" in lib.cpe_last_error(), kw
    assert call(None) == abi.BAD_ARG and b"null argument" in lib.cpe_last_error()
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert call(h._h, lam=lam) == abi.BAD_ARG and b"damping must be positive" in lib.cpe_last_error(), lam
    for B, N in ((-2, 1), (1, -2)):
        assert call(h._h, B=B, N=N) == abi.BAD_ARG and b"negative size" in lib.cpe_last_error()
        assert lib.cpe_eval_shutter_step_host(h._h, B, N, sp, sp, sp, sp, 1e-2, *[None] * 8, sp) == abi.BAD_ARG and b"negative size" in lib.cpe_last_error()
    assert call(h._h, B=0, N=5) == abi.OK                                            # empty batch: nothing to touch
    assert lib.cpe_eval_shutter_step_host(h._h, 1, 1, None, sp, sp, sp, 1e-2, *[None] * 8, sp) == abi.BAD_ARG
    hm = _lib.Handle.multi([sk, sk], [cams, synth.make_cameras(2)])
    try:
        assert call(hm._h) == abi.BAD_ARG and b"no ragged form" in lib.cpe_last_error()
    finally:
        hm.close()
    with pytest.raises(_lib.CpeError):
        h.eval_shutter_step_host(np.zeros((1, 3, sk.nq)), np.zeros((1, 3, 6, 25, 2)), np.zeros((1, 3, 6, 25)), np.zeros((1, 5)), 1e-2)


def test_zz_report():
    """the worst value of every key over the cases of this module (recorded in shutter_compare's docstring; they never feed its tolerances)"""
    for k in SC.KEYS:
        vals = {c: v for (c, kk), v in WORST.items() if kk == k}
        if vals:
            c = max(vals, key=vals.get)
            print(f"worst {k}: {vals[c]:.2e} ({c}), tolerance {SC.TOL[k]:.2e}")
