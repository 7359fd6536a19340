"""The reduced system of the length calibration on the GPU (cpe_scale_system, include/cpe.h: k_scale_cross, k_band_forward) entry by entry against
the np.longdouble reference of tests/scale_compare.py.  The cases are the smallest shapes at which the kernels can go wrong:

  plain        25 markers (the 25th has no length dependence), 6 cameras, 11 groups, N = 5: past the half-bandwidth, the ring of pending rows wraps
  n1, n2       N = 1 (A = A_n, b = b_n: the per-frame record itself; no off-diagonal block) and N = 2 (below the half-bandwidth)
  ragged       N_max 5, lengths 5 and 2, two models with different lengths, tables and camera counts (6 and 2: the batch's camera stride is not
               the second model's camera count; cpe_create_multi)
  cams1/18     one camera; 18 cameras (the camera table's 396 doubles in LDS, frame_compare.CAMERA_COUNTS' upper end)
  g1, g16      one group of all links; 16 groups = CPE_MAX_SCALES, one of them without a link: its rows and columns are exactly zero and
               A_red + P is still solvable
  zero_camera  one camera with all weights zero
  loss_c1      the other curvature mode; every case holds residuals beyond loss_c (10 % outliers anywhere on the image), which add nothing
  pinhole      the kinetic-dataset rig: four pinhole cameras, multipliers (1, 1, 0.6, 0.6), an `-02` skeleton
  prior        the packaged window-4 priors: half-bandwidth 4, the pose prior in H
  batch3       B = 3: bit-equal to three single calls, and a repeated call bit-equal to the first

Tolerances: scale_compare.tolerance(case), 32 x the reference's own spread on that case's inputs, measured on the CPU (its module docstring); the
GPU's worst values are printed by test_zz_report and never feed a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import scale_compare as SC
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

WORST = {}
HANDLES = {}


def _handle(name):
    """the handle of a case (one per module run) and the stacked derivative tables of its models"""
    c = SC.case_inputs(name)
    if name not in HANDLES:
        sks = [m[0] for m in c["models"]]
        if len(sks) == 1:
            h = _lib.Handle(sks[0], c["models"][0][3], c["opts"], c["pr"])
        else:
            h = _lib.Handle.multi(sks, [m[3] for m in c["models"]], [c["opts"]] * len(sks), c["pr"])
        HANDLES[name] = h
    da = np.stack([m[1] for m in c["models"]])
    dm = np.stack([m[2] for m in c["models"]])
    return c, HANDLES[name], da, dm


def _run(name):
    c, h, da, dm = _handle(name)
    if len(c["q"]) > 1 or len(c["models"]) > 1:
        same = len({q.shape[0] for q in c["q"]}) == 1 and len(c["models"]) == 1
        if same:
            return h.scale_system_host(np.stack(c["q"]), np.stack(c["meas"]), np.stack(c["weight"]), da, dm, c["ridge"])
        return h.scale_system_host(list(c["q"]), list(c["meas"]), list(c["weight"]), da, dm, c["ridge"], model_list=c["model"])
    return h.scale_system_host(c["q"][0][None], c["meas"][0][None], c["weight"][0][None], da, dm, c["ridge"])


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in HANDLES.values():
        h.close()
    HANDLES.clear()


@pytest.mark.parametrize("name", SC.CASES)
def test_scale_system_matches_the_reference(oracle, name):
    c = SC.case_inputs(name)
    R = SC.case_reference(oracle, name)
    out = _run(name)
    B = len(c["q"])
    assert out["status"] == abi.OK and out["seq_status"] == [abi.OK] * B
    G = {k: [out[k][b] for b in range(B)] for k in ("A", "b", "A_red", "b_red", "cost")}
    d = SC.discrepancies(G, R)
    print(name, ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    tol = SC.tolerance(name)
    for k, v in d.items():                                           # the worst share of its tolerance, for the record
        share = v / tol[k] if tol[k] > 0 else (0.0 if v == 0.0 else float("inf"))
        if share >= WORST.get(k, (0.0, 0.0, ""))[0]:
            WORST[k] = (share, v, name)
    assert not SC.failures(d, tol), (name, SC.failures(d, tol), tol)
    ng = len(c["groups"])
    P = np.eye(ng) / 0.1 ** 2
    for b in range(B):
        assert np.array_equal(out["A"][b], out["A"][b].T) and np.array_equal(out["A_red"][b], out["A_red"][b].T)
        step = np.linalg.solve(out["A_red"][b] + P, -(out["b_red"][b]))
        assert np.all(np.isfinite(step))
        for g, (_, links) in enumerate(c["groups"]):
            if not links:                                            # a group no marker depends on
                for k in ("A", "A_red"):
                    assert not out[k][b][g].any() and not out[k][b][:, g].any()
                assert out["b"][b][g] == 0.0 and out["b_red"][b][g] == 0.0 and step[g] == 0.0
    if name == "n1":                                                 # no pose can re-adapt along a direction the frame does not see: A_red <= A
        assert np.all(np.diag(out["A_red"][0]) <= np.diag(out["A"][0]))


def test_batch_and_repeat_are_bit_equal(oracle):
    """B = 3 against three single calls, the batch in another order, and the same call again: the same bits"""
    c, h, da, dm = _handle("batch3")
    q, me, we = np.stack(c["q"]), np.stack(c["meas"]), np.stack(c["weight"])
    keys = ("A", "b", "A_red", "b_red", "cost")
    full = h.scale_system_host(q, me, we, da, dm, c["ridge"])
    again = h.scale_system_host(q, me, we, da, dm, c["ridge"])
    back = h.scale_system_host(q[::-1].copy(), me[::-1].copy(), we[::-1].copy(), da, dm, c["ridge"])
    for k in keys:
        assert full[k].tobytes() == again[k].tobytes(), k
        assert np.ascontiguousarray(back[k][::-1]).tobytes() == full[k].tobytes(), k
    for b in range(3):
        one = h.scale_system_host(q[b:b + 1], me[b:b + 1], we[b:b + 1], da, dm, c["ridge"])
        for k in keys:
            assert one[k][0].tobytes() == full[k][b].tobytes(), (b, k)


def test_ragged_sequences_equal_their_plain_calls(oracle):
    """every sequence of the ragged pair against a plain call on a handle of its own model: the same bits"""
    c, h, da, dm = _handle("ragged")
    out = _run("ragged")
    for b, m in enumerate(c["model"]):
        sk, a, o, cams = c["models"][m]
        hb = _lib.Handle(sk, cams, c["opts"], c["pr"])
        try:
            one = hb.scale_system_host(c["q"][b][None], c["meas"][b][None], c["weight"][b][None], a, o, c["ridge"])
        finally:
            hb.close()
        for k in ("A", "b", "A_red", "b_red", "cost"):
            assert one[k][0].tobytes() == out[k][b].tobytes(), (b, k)


def test_sequence_without_a_factor(oracle):
    """cpe_covariance's rule: three frames without any measurement at ridge 0 (no motion term below four frames: H = 0) have no factor --
    CPE_NUMERICAL and all outputs zero, as that entry reports for the same input, and the batch neighbour keeps its bits; at ridge 1e-3 the
    sequence has a factor and a system of zeros"""
    c, h, da, dm = _handle("batch3")
    q, me, we = np.stack(c["q"])[:2, :3].copy(), np.stack(c["meas"])[:2, :3].copy(), np.stack(c["weight"])[:2, :3].copy()
    keys = ("A", "b", "A_red", "b_red", "cost")
    good = h.scale_system_host(q[:1], me[:1], we[:1], da, dm, 0.0)
    assert good["seq_status"] == [abi.OK]
    we[1] = 0.0; me[1] = 0.0
    out = h.scale_system_host(q, me, we, da, dm, 0.0)
    cov = h.covariance_host(q, me, we, 0.0)
    assert out["seq_status"] == cov["seq_status"] == [abi.OK, abi.NUMERICAL] and out["status"] == abi.NUMERICAL
    for k in keys:
        assert not np.asarray(out[k][1]).any() and out[k][0].tobytes() == good[k][0].tobytes(), k
    ok = h.scale_system_host(q, me, we, da, dm, 1e-3)
    assert ok["seq_status"] == [abi.OK] * 2 and not any(np.asarray(ok[k][1]).any() for k in keys[:4])
    assert np.isfinite(ok["cost"][1])                                 # (rho(0) per unseen coordinate, as the solve counts it)


def test_refusals_that_need_a_handle():
    """a half-bandwidth above 4 in cov_check's wording, a model index out of range and a null array: CPE_BAD_ARG, nothing launched and the
    outputs untouched (the refusals that need no handle: tests/test_length_scale_host.py)"""
    da, dm = skeleton.length_derivatives("phantom", 24)
    sk = skeleton.build_skeleton("phantom", 24)
    w5 = priors.load_priors(path=os.path.join(os.path.dirname(__file__), "golden", "priors_k3_w5_dense.npz"))
    h5 = _lib.Handle(sk, synth.make_cameras(2), abi.default_options(), w5)
    try:
        assert h5.pb == 5
        q, me, we = np.zeros((1, 6, h5.nq)), np.zeros((1, 6, 2, 24, 2)), np.zeros((1, 6, 2, 24))
        with pytest.raises(_lib.CpeError, match="cpe_scale_system_host: half-bandwidth 5 .* is not supported by the covariance sweep"):
            h5.scale_system_host(q, me, we, da, dm)
        import torch
        dev = torch.device("cuda", 0)
        T = lambda a: torch.tensor(a, device=dev)
        out = [torch.full(s, 7.0, dtype=torch.float64, device=dev) for s in ((1, 11, 11), (1, 11), (1, 11, 11), (1, 11), (1,))]
        with pytest.raises(_lib.CpeError, match="cpe_scale_system: half-bandwidth 5 .* is not supported by the covariance sweep"):
            h5.scale_system(T(q), T(me), T(we), da, dm, *out)
        assert all(bool((o == 7.0).all()) for o in out)
        with pytest.raises(ValueError, match="A_red is a contiguous float64 tensor of shape"):
            h5.scale_system(T(q), T(me), T(we), da, dm, out[0], out[1], out[1], out[3], out[4])
    finally:
        h5.close()
    c, h, tda, tdm = _handle("ragged")                               # a handle of two models
    q, me, we = np.zeros((1, 3, h.nq)), np.zeros((1, 3, h.n_cams, 24, 2)), np.zeros((1, 3, h.n_cams, 24))
    outs = [np.full(s, 7.0) for s in ((1, 11, 11), (1, 11), (1, 11, 11), (1, 11), (1,))]
    st = (C.c_int32 * 1)(5)
    ptr = lambda a: a.ctypes.data
    for model, reason in ((2, b"model index of sequence 0 out of range"), (-1, b"model index of sequence 0 out of range")):
        rc = h.lib.cpe_scale_system_host(h._h, 1, 3, (C.c_int32 * 1)(model), (C.c_int32 * 1)(3), ptr(q), ptr(me), ptr(we), 0.0, 11, ptr(tda), ptr(tdm),
                                         *[ptr(o) for o in outs], st)
        assert rc == abi.BAD_ARG and b"cpe_scale_system_host: " in h.lib.cpe_last_error() and reason in h.lib.cpe_last_error()
        assert all((o == 7.0).all() for o in outs) and st[0] == 5
    rc = h.lib.cpe_scale_system_host(h._h, 1, 3, None, None, ptr(q), ptr(me), ptr(we), 0.0, 11, ptr(tda), None, *[ptr(o) for o in outs], st)
    assert rc == abi.BAD_ARG and b"cpe_scale_system_host: null argument" in h.lib.cpe_last_error() and all((o == 7.0).all() for o in outs)
    with pytest.raises(ValueError, match="d_attach is \\[2, G, 17, 3\\]"):
        h.scale_system_host(q, me, we, tda[:1], tdm[:1])


def test_zz_report():
    """the GPU's worst value per key next to its tolerance (for the record; asserts nothing new)"""
    for k in SC.KEYS:
        if k in WORST:
            print(f"  {k:7s} worst share of its tolerance {WORST[k][0]:.3f} (value {WORST[k][1]:.2e}, case {WORST[k][2]})")
