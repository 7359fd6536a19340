"""k_frame_normal through cpe_eval_normal, entry by entry against the extended-precision reference of tests/frame_compare.py: both curvature
modes with residuals in every piece of the loss, other knots with pinhole cameras and camera multipliers, camera counts on both sides of the
switch of the kernel's LDS layout, degenerate weights, every kind of angle bound, the Gaussian-mixture prior (the non-PLAIN instantiation) and
the independence of a sequence from its batch.  Every case is 2 x 5 frames, asserts the conditions on its inputs and that the path it means to
exercise is active, and records its worst value per key; test_zz_report prints the worst of the module."""
import numpy as np
import pytest

import frame_compare as FC
from cheetah_pose_estimation_amd import abi, skeleton, synth

pytestmark = pytest.mark.gpu

WORST = {}                                        # (case, key) -> worst value, printed at the end of the module


def _run(name, oracle, gpu_handle_factory):
    """HIP against the reference on a case of frame_compare.CASES: (HIP's outputs, the reference, the inputs)"""
    c = FC.case_inputs(name)
    R = FC.case_reference(oracle, name)
    assert FC.conditions_hold(R), (name, R["conditions"])
    inl = R["conditions"]["camera_inliers"]                                          # every camera holds residuals below loss_c, not outliers alone
    assert len(inl) == len(c["cams"]) and min(inl) >= FC.MIN_CAMERA_INLIERS, (name, inl)
    assert c["q"].shape[:2] == (FC.B, FC.N)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["pr"])
    G = FC.hip_outputs(h, c["q"], c["meas"], c["weight"])
    d = FC.discrepancies(G, R)
    print(f"{name}: " + ", ".join(f"{k} {d[k]:.1e}" for k in FC.KEYS))
    for k in FC.KEYS:
        WORST[(name, k)] = d[k]
    assert not FC.failures(d), (name, FC.failures(d))
    return G, R, c


def _frame(b, n):
    return b * FC.N + n


def test_plain(oracle, gpu_handle_factory):
    """phantom 25, six fisheye cameras, a rolled base and limbs swung beyond 90 degrees of pitch (both cos(phi) branches)"""
    G, R, c = _run("plain", oracle, gpu_handle_factory)
    assert c["pr"] is None and (np.abs(R["q_out"][:, 3::3][:, 1:]) > np.pi / 2).any()


def test_loss_pieces_in_both_curvature_modes(oracle, gpu_handle_factory):
    """each of the four pieces of the loss holds at least 5 % of the weighted residuals; between the two modes g, cost and q_out are bit-equal
    and Bm is not"""
    out = {}
    for mode in (0, 1):
        G, R, c = _run(f"loss-c{mode}", oracle, gpu_handle_factory)
        assert c["opts"].curvature == mode and min(R["conditions"]["pieces"]) >= 0.05, R["conditions"]
        out[mode] = (G, R)
    (G0, R0), (G1, _) = out[0], out[1]
    for k in ("g", "cost", "q_out"):
        assert G0[k].tobytes() == G1[k].tobytes(), k
    assert FC.relative_difference(G0["Bm"], G1["Bm"], R0["Bm_scale"]) > 1e-3


def test_other_knots_pinhole_cameras_and_multipliers(oracle, gpu_handle_factory):
    """loss knots 2, 6, 15 on the kinetic-dataset rig: four pinhole cameras with radial distortion and multipliers (1, 1, 0.6, 0.6), an `-02`
    skeleton with its tighter bounds, 200 fps"""
    G, R, c = _run("knots", oracle, gpu_handle_factory)
    assert (c["opts"].loss_a, c["opts"].loss_b, c["opts"].loss_c) == (2.0, 6.0, 15.0) and c["opts"].h == 1.0 / 200.0
    assert [cam.mult for cam in c["cams"]] == [1.0, 1.0, 0.6, 0.6] and all(cam.model == abi.CAM_PINHOLE for cam in c["cams"])
    assert R["active"].any()                                                         # the tighter bounds bite


@pytest.mark.parametrize("C", FC.CAMERA_COUNTS)
def test_camera_counts_across_the_lds_switch(C, oracle, gpu_handle_factory):
    """the positions of k_frame_normal's LDS start at max(n_camov, CAMW C): 13 and 14 cameras lie on opposite sides, 18 is CPE_MAX_CAMS"""
    sk = FC.case_inputs(f"cams{C}")["sk"]
    assert FC.CAMW * 13 < FC.n_camov(sk) < FC.CAMW * 14 and max(FC.CAMERA_COUNTS) == abi.MAX_CAMS
    G, R, c = _run(f"cams{C}", oracle, gpu_handle_factory)
    assert len(c["cams"]) == C and len(R["conditions"]["camera_inliers"]) == C        # (_run asserts the inliers of every one of them)
    if C > 6:                                                                        # every copy of a camera has its own draw of noise and weights
        assert not np.array_equal(c["meas"][:, :, 0], c["meas"][:, :, 6]) and not np.array_equal(c["weight"][:, :, 0], c["weight"][:, :, 6])


def test_degenerate_weights(oracle, gpu_handle_factory):
    """a frame with every weight zero, a marker seen by exactly one camera, zero weights with zero measurements (NaN gaps)"""
    G, R, c = _run("weights", oracle, gpu_handle_factory)
    f = _frame(*c["zero_frame"])
    C, L = c["weight"].shape[2:]
    rho0 = FC.loss(np.zeros(1, dtype=np.longdouble), *(np.longdouble(x) for x in (c["opts"].loss_a, c["opts"].loss_b, c["opts"].loss_c)))[0][0]
    assert not c["weight"][c["zero_frame"]].any()
    assert abs(G["cost"][f, 0] - float(2 * C * L * rho0)) <= FC.TOL["cost"] * abs(float(2 * C * L * rho0))
    assert not R["g_meas"][f].any() and not R["active"][f].any()                     # nothing but the bounds could contribute, and none is active:
    assert not G["g"][f].any() and not G["Bm"][f].any()                              # exactly zero
    b, n, m, keep = c["single"]
    assert (c["weight"][b, n, :, m] > 0).sum() == 1 and c["weight"][b, n, keep, m] > 0
    gaps = (c["weight"][1] == 0) & ~c["meas"][1].any(axis=-1)
    assert gaps.sum() >= c["gaps"] > 100


def test_angle_bounds(oracle, gpu_handle_factory):
    """a plain upper bound, a plain lower bound, a difference of two trunk angles, a difference of two leg pitches and a trunk pitch against a
    leg pitch (the cost-pitch row theta_B + alpha), each violated in a frame of its own"""
    G, R, c = _run("bounds", oracle, gpu_handle_factory)
    sk = c["sk"]
    legs = {3 + 3 * cl + 1 for cl, _ in synth.leg_layout(sk)}
    kinds = set()
    for b, n, i, side in c["expect_active"]:
        f = _frame(b, n)
        assert R["active"][f, i, side] and G["cost"][f, 1] > 0.0, (b, n, i, side)
        kinds.add((sk.bound_b[i] >= 0, sk.bound_a[i] in legs, sk.bound_b[i] in legs, side))
    assert kinds == {(False, False, False, 0), (False, False, False, 1), (True, False, False, 0), (True, True, True, 1), (True, False, True, 1)}


@pytest.mark.parametrize("n_cams", [1, 2, 6])
@pytest.mark.parametrize("prior", list(FC.PRIOR_FILES))
def test_pose_prior(prior, n_cams, oracle, gpu_handle_factory):
    """the non-PLAIN instantiation: the packaged priors and the golden K = 3 and K = 5 mixtures, on 1, 2 and 6 cameras"""
    G, R, c = _run(f"prior-{prior}-c{n_cams}", oracle, gpu_handle_factory)
    assert c["pr"].gmm_k > 0 and len(c["cams"]) == n_cams
    assert np.all(G["cost"][:, 2] != 0.0)
    assert np.abs(R["g_prior"]).max() > 1.0                                          # the prior really moves g


def _equal(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_batch_independence(gpu_handle_factory):
    """the 37-sequence mixed batch of test_gpu_lm_step.test_large_mixed_batch cut to its frames 2 to 4 (the frame without measurements among them): every sequence bit-equal to its own B = 1 call,
    the same call twice bit-equal"""
    sk, cams = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6)
    h = gpu_handle_factory(sk, cams, abi.default_options())
    d = synth.make_batch(sk, cams, B=37, N=9, seed=61)
    rng = np.random.default_rng(62)
    q, me, we = d["q_init"].copy(), d["meas"], d["weight"].copy()
    q[::3] += rng.normal(0, 0.05, q[::3].shape)
    q[1::5, :, 3] += 0.4
    we[2::7, 4] = 0.0
    q, me, we = (np.ascontiguousarray(a[:, 2:5]) for a in (q, me, we))
    assert not we[2::7, 2].any() and we[2::7, 1].any()
    G1 = FC.hip_outputs(h, q, me, we)
    G2 = FC.hip_outputs(h, q, me, we)
    assert all(np.isfinite(v).all() for v in G1.values())
    assert all(_equal(G1[k], G2[k]) for k in G1)
    for b in range(37):
        Gs = FC.hip_outputs(h, q[b:b + 1], me[b:b + 1], we[b:b + 1])
        assert all(_equal(G1[k][3 * b:3 * b + 3], Gs[k]) for k in G1), b


def test_zz_report():
    """the worst value of every key over the cases of this module (recorded in frame_compare's docstring; they never feed its tolerances)"""
    for k in FC.KEYS:
        vals = {c: v for (c, kk), v in WORST.items() if kk == k}
        if vals:
            c = max(vals, key=vals.get)
            print(f"worst {k}: {vals[c]:.2e} ({c}), tolerance {FC.TOL[k]:.2e}")
