"""estimate_kinematics_batch(estimate_lengths=True, uncertainty=True, uncertainty_lengths=True) on the GPU (DESIGN.md 2 "What is marginalised"):
the experiment of tests/scale_compare.py -- phantom with every segment group off by up to 8 %, two sequences of N = 16, six cameras, the case whose
calibration converges in 6 rounds.  The estimators are made in memory (no detection tables), so the initial guess the fronts would build from the
tables is handed to estimator._kin_prepare here.

Measured on an MI355X (printed by the test; nothing of it feeds a bound): marginal over conditional standard deviation, median / worst --
coordinates 1.012 / 1.40 and 1.011 / 1.52, marker positions 1.013 / 1.84 and 1.007 / 2.00 (the two sequences); the standard deviation of the scales
is up to 2.5e-2."""
import os

import numpy as np
import pytest

import scale_compare as SC
from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth
from cheetah_pose_estimation_amd import estimator as E

pytestmark = pytest.mark.gpu


def _estimators(data):
    sk = skeleton.build_skeleton("phantom", 24)
    cams = data["cams"]                                              # the scene's arrays, for the files est.save writes
    K = [np.array([[c.fx, 0.0, c.cx], [0.0, c.fy, c.cy], [0.0, 0.0, 1.0]]) for c in cams]
    D, R, t = [np.array(c.D[:4]) for c in cams], [np.array(c.R[:]).reshape(3, 3) for c in cams], [np.array(c.t[:]) for c in cams]
    out = []
    for b in range(data["meas"].shape[0]):
        N = data["meas"].shape[1]
        params = E.TrajectoryParams("", 0, N, N, 0.5, None, False, False, False, False)
        scene = E.Scene("", K, D, R, t, (synth.IMG_W, synth.IMG_H), 120.0, len(cams), None)
        out.append(E.CheetahEstimator("phantom", f"seq{b}", params, scene, abi.Skeleton.from_buffer_copy(bytes(sk)), data["cams"],
                                      np.ascontiguousarray(data["meas"][b]), np.ascontiguousarray(data["weight"][b]), 0.0, True))
    return out


def _run(monkeypatch, tmp_path, data, **kw):
    ests = _estimators(data)
    guess = {id(e): data["q_init"][b] for b, e in enumerate(ests)}
    prepare = E._kin_prepare
    monkeypatch.setattr(E, "_kin_prepare", lambda est, *a: prepare(est, *a[:6], guess[id(est)] if a[6] is None else a[6], *a[7:]))
    ok = E.estimate_kinematics_batch(ests, out_dir_prefix=str(tmp_path), estimate_lengths=True, uncertainty=True, **kw)
    assert ok == [True, True]
    files = [dict(np.load(os.path.join(str(tmp_path), f"seq{b}", "fte_kinematic", "uncertainty.npz"))) for b in range(len(ests))]
    return ests, files


def test_marginal_fields_of_a_calibrated_batch(monkeypatch, tmp_path):
    data = SC.experiment_data(2)
    plain, plain_files = _run(monkeypatch, tmp_path / "plain", data)
    ests, files = _run(monkeypatch, tmp_path / "marginal", data, uncertainty_lengths=True)
    G, N = len(skeleton.LENGTH_GROUPS), data["meas"].shape[1]
    for b, (e, f) in enumerate(zip(ests, files)):
        u = e.uncertainty
        # every field from before: the bits of the run without the keyword, in memory and in the file
        assert set(plain_files[b]) == set(f) - set(E.LENGTH_FIELDS) and set(E.LENGTH_FIELDS) <= set(f)
        for k, v in plain_files[b].items():
            assert v.tobytes() == f[k].tobytes() == np.asarray(u[k]).tobytes(), k
        for k in E.LENGTH_FIELDS:
            assert np.all(np.isfinite(u[k])) and np.asarray(u[k]).tobytes() == f[k].tobytes(), k
        assert u["cov_u_marginal"].shape == (N, 28, 28) and u["positions_cov_marginal"].shape == (N, 24, 3, 3) and u["scale_cov"].shape == (G, G)
        assert u["u_scale_response"].shape == (N, 28, G) and u["positions_scale_response"].shape == (N, 24, 3, G)
        assert np.all(u["u_std_marginal"] >= u["u_std"]) and np.all(u["positions_std_marginal"] >= u["positions_std"])
        assert np.array_equal(u["cov_u_marginal"], np.swapaxes(u["cov_u_marginal"], 1, 2))
    # scale_cov = inv(sum A_red + P) at the returned poses, the same for both sequences of the animal
    da, dm = skeleton.length_derivatives("phantom", 24)
    h = _lib.Handle(ests[0].skeleton, data["cams"], abi.default_options(120.0), None)
    try:
        sys_ = h.scale_system_host(np.stack([e.result["q"][0] for e in ests]), data["meas"], data["weight"], da, dm, 0.0)
    finally:
        h.close()
    assert sys_["seq_status"] == [abi.OK, abi.OK]
    cov_s = E.scale_covariance(list(sys_["A_red"]), ests[0].length_calibration["prior_sigma"])
    assert np.array_equal(cov_s, np.linalg.inv(sys_["A_red"][0] + sys_["A_red"][1] + np.eye(G) / 0.1 ** 2))
    for e in ests:
        u = e.uncertainty
        assert u["scale_cov"].tobytes() == cov_s.tobytes()
        # the marginal = the conditional + R scale_cov R^T from the stored responses.  Kernel and numpy sum the same G^2 products in different
        # orders: each is within (2 G + 2) eps of the exact value in units of the sum of the terms' magnitudes (the standard bound of a
        # float64 sum of products), so the two differ by at most twice that
        R, W = u["u_scale_response"], u["positions_scale_response"]
        mu = u["cov_u"] + np.einsum("nkg,gh,njh->nkj", R, cov_s, R)
        mp = u["positions_cov"] + np.einsum("nlag,gh,nlbh->nlab", W, cov_s, W)
        bound = 2 * (2 * G + 2) * 2.0 ** -52
        au = np.abs(u["cov_u"]) + np.einsum("nkg,gh,njh->nkj", np.abs(R), np.abs(cov_s), np.abs(R))
        ap = np.abs(u["positions_cov"]) + np.einsum("nlag,gh,nlbh->nlab", np.abs(W), np.abs(cov_s), np.abs(W))
        assert np.all(np.abs(mu - u["cov_u_marginal"]) <= bound * au) and np.all(np.abs(mp - u["positions_cov_marginal"]) <= bound * ap)
        su, sp = u["u_std_marginal"], u["positions_std_marginal"]
        ru, rp = su / u["u_std"], sp / u["positions_std"]
        print(f"{e.data_path}: marginal / conditional std, median / worst: coordinates {np.median(ru):.3f} / {ru.max():.2f}, "
              f"marker positions {np.median(rp):.3f} / {rp.max():.2f}; sigma of the scales up to {np.sqrt(np.diag(cov_s)).max():.2e}")
