"""The length calibration on the GPU (estimator.calibrate_lengths: batch pose solves + cpe_scale_system per round; DESIGN.md 2 "What is
calibrated") on the experiment of tests/scale_compare.py -- phantom with every segment group off by up to 8 %, N = 16 -- and end to end through
files.  What is asserted is what a joint minimiser of poses and lengths must satisfy, not closeness to the true lengths: the minimiser is biased
by the prior and by the constant-acceleration term.

Measured on an MI355X (printed by the tests; nothing of it feeds a bound):
  two sequences   6 rounds (the oracle-driven loop: 6), objective -1971.991198 against -1971.687770 at the truth, max |s - s_true| 1.6e-2,
                  max |s - s_oracle| 1.0e-12
  noisy           7 rounds, objective 8078.999770 against 8080.339512 at the truth, max |s - s_true| 3.2e-2
  one camera      30 rounds and NOT converged (steps still at the cap: the valley along scale-and-depth is flat but for the prior), objective
                  -50.94 against 8.17 at s = 1, max |s - 1| 0.252 = 2.5 sigma
  through files   from +-5 % to max |s - 1| 2.4e-3; standard deviation of the scales up to 1.9e-2"""
import json
import os
import sys

import numpy as np
import pytest

import scale_compare as SC
from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth
from cheetah_pose_estimation_amd import estimator as E

pytestmark = pytest.mark.gpu

G = len(skeleton.LENGTH_GROUPS)
S_TRUE = SC.EXPERIMENT_SCALE
SIGMA = 0.1


def _estimators(data, cam_idx=None):
    """one estimator per sequence of experiment_data's dict, on the NOMINAL skeleton, as init_trajectory would hand them over"""
    sk = skeleton.build_skeleton("phantom", 24)
    out = []
    for b in range(data["meas"].shape[0]):
        N = data["meas"].shape[1]
        params = E.TrajectoryParams("", 0, N, N, 0.5, None, False, False, False, False)
        scene = E.Scene("", None, None, None, None, (synth.IMG_W, synth.IMG_H), 120.0, len(data["cams"]), cam_idx)
        out.append(E.CheetahEstimator("phantom", "", params, scene, abi.Skeleton.from_buffer_copy(bytes(sk)), data["cams"],
                                      np.ascontiguousarray(data["meas"][b]), np.ascontiguousarray(data["weight"][b]), 0.0, True))
    return out


def _objective(data, s, sigma, q_init=None, priors=None):
    """the total objective the loop minimises at scales s with re-solved poses, by the GPU's own solve: sum of the solves' cost / cost_scale + prior"""
    opts = abi.default_options()
    h = _lib.Handle(skeleton.build_skeleton("phantom", 24, length_scale=s), data["cams"], opts, priors)
    try:
        res = h.solve_host(data["q_init"] if q_init is None else q_init, data["meas"], data["weight"])
    finally:
        h.close()
    assert all(st.status != abi.NUMERICAL for st in res["stats"])
    return sum(st.cost for st in res["stats"]) / opts.cost_scale + 0.5 * ((np.asarray(s) - 1.0) ** 2).sum() / sigma ** 2


def test_two_sequences_of_one_animal():
    """the CPU experiment with B = 2 sequences sharing their scales: converged within max_rounds; the objective at the result is not above the
    objective at the true lengths (slack 1e-6 |J|); the lengths end at most half as far from the truth as they started; and the scales agree
    with the oracle-driven loop's (tests/golden/length_calibration_oracle.npz, re-made by tests/test_length_scale_host.py) to 1e-4: both loops
    stop at a step below 1e-6, and with the slowest contraction measured, 0.97, each ends within 3.3e-5 of the fixed point"""
    data = SC.experiment_data(2)
    ests = _estimators(data)
    r = E.calibrate_lengths(ests, prior_sigma=SIGMA, q_init=list(data["q_init"]))
    J_true = _objective(data, S_TRUE, SIGMA)
    gold = np.load(SC.ORACLE_GOLDEN)
    err = np.abs(r["s"] - S_TRUE).max()
    print(f"rounds {r['rounds']} (oracle {int(gold['rounds'])}), objective {r['objective']:.6f} (at the truth {J_true:.6f}; oracle {float(gold['objective']):.6f}), "
          f"max |s - s_true| {err:.3e}, max |s - s_oracle| {np.abs(r['s'] - gold['s']).max():.3e}")
    assert r["converged"] and r["rounds"] <= 30
    assert r["objective"] <= J_true + 1e-6 * abs(J_true)
    assert err <= 0.5 * 7.9e-2
    assert np.abs(r["s"] - gold["s"]).max() <= 1e-4
    for e in ests:                                                   # what the call leaves on every estimator
        assert e.length_calibration == dict(converged=True, rounds=r["rounds"], prior_sigma=SIGMA, ridge=0.0, objective=r["objective"])
        assert np.array_equal(e.length_scale, r["s"]) and e.length_groups == skeleton.LENGTH_GROUPS
        assert np.array_equal(e.length_scale_cov, r["cov"]) and np.all(np.linalg.eigvalsh(r["cov"]) > 0)
        assert bytes(e.skeleton) == bytes(skeleton.build_skeleton("phantom", 24, length_scale=r["s"]))
    assert len(r["q"]) == 2 and r["q"][0].shape == data["q_init"][0].shape


def test_noisy_detections():
    """2 px of noise and 10 % outliers: the objective at the result is not above the objective at the true lengths"""
    data = SC.experiment_data(1, noisy=True)
    r = E.calibrate_lengths(_estimators(data), prior_sigma=SIGMA, q_init=list(data["q_init"]))
    J_true = _objective(data, S_TRUE, SIGMA)
    print(f"rounds {r['rounds']}, converged {r['converged']}, objective {r['objective']:.6f} (at the truth {J_true:.6f}), "
          f"max |s - s_true| {np.abs(r['s'] - S_TRUE).max():.3e}")
    assert r["objective"] <= J_true + 1e-6 * abs(J_true)


def test_one_camera_leans_on_the_prior():
    """one camera (with the packaged priors, as a monocular estimate runs): scale and depth are not separable, the prior sigma = 0.1 holds the
    scales -- |s - 1| <= 3 sigma -- and the total objective is not above its value at s = 1; without a prior the call is refused.  The loop
    does not converge within 30 rounds here (module docstring): that is what it warns of and records, which IS asserted, so that the day the
    loop converges on this case the record and this test are looked at again."""
    from cheetah_pose_estimation_amd import priors
    data = SC.experiment_data(1, n_cams=1)
    ests = _estimators(data, cam_idx=1)
    assert (data["weight"] > 0).sum() > 150                           # the camera sees the animal
    with pytest.raises(ValueError, match="scale and depth cannot be separated"):
        E.calibrate_lengths(ests, prior_sigma=None, monocular_constraints=True, q_init=list(data["q_init"]))
    with pytest.warns(RuntimeWarning, match="not converged after 30 rounds"):               # said aloud, and kept with the result
        r = E.calibrate_lengths(ests, prior_sigma=SIGMA, monocular_constraints=True, ridge=1e-6, q_init=list(data["q_init"]))
    assert not r["converged"] and ests[0].length_calibration == dict(converged=False, rounds=30, prior_sigma=SIGMA, ridge=1e-6, objective=r["objective"])
    J_one = _objective(data, np.ones(G), SIGMA, priors=priors.load_priors())
    print(f"rounds {r['rounds']}, converged {r['converged']}, objective {r['objective']:.6f} (at s = 1 {J_one:.6f}), max |s - 1| {np.abs(r['s'] - 1.0).max():.3e}")
    assert np.abs(r["s"] - 1.0).max() <= 3.0 * SIGMA
    assert r["objective"] <= J_one + 1e-6 * abs(J_one)


def test_through_files(tmp_path):
    """write_dataset -> init_trajectory -> estimate_kinematics(estimate_lengths=True, length_scale_init=...) from lengths off by 5 % on data of the
    nominal animal: fte.pickle and skeleton_scale.json are written, the scales end nearer to 1 than they started, the later stages' tables
    carry them; a run without the flag writes no json, leaves the estimator's skeleton alone and returns the bits of a direct solve of the same
    inputs (the default path adds nothing)"""
    sys.path.insert(0, os.path.dirname(__file__))
    from dataset_util import write_dataset
    init = lambda root: E.init_trajectory(root_dir=root, data_path="2019_03_07/synth/run", cheetah_name="phantom", kinetic_dataset=False,
                                          solver_path="/unused/ipopt", kinematic_model=True)
    roots = {k: str(tmp_path / k) for k in ("plain", "fit")}
    for root in roots.values():
        write_dataset(root, N=16, noise_px=0.5)
    plain = init(roots["plain"])
    nominal = bytes(plain.skeleton)
    assert E.estimate_kinematics(plain, solver_output=False)
    out_plain = os.path.join(roots["plain"], "2019_03_07/synth/run", "fte_kinematic")
    assert os.path.exists(os.path.join(out_plain, "fte.pickle")) and not os.path.exists(os.path.join(out_plain, "skeleton_scale.json"))
    assert plain.length_scale is None and bytes(plain.skeleton) == nominal
    q_init, opts, pri = E._kin_prepare(init(roots["plain"]), False, False, False, 5, 4, True, None, None)
    h = _lib.Handle(plain.skeleton, plain.cams, opts, pri)
    try:
        direct = h.solve_host(q_init[None], plain.meas[None], plain.weight[None])
    finally:
        h.close()
    stored = E.load_result_pickle(os.path.join(out_plain, "fte.pickle"))
    assert stored["q"].tobytes() == direct["q"][0].tobytes() and stored["positions"].tobytes() == direct["positions"][0].tobytes()

    s0 = 1.0 + 0.05 * np.where(np.arange(G) % 2 == 0, 1.0, -1.0)
    fit = init(roots["fit"])
    assert E.estimate_kinematics(fit, solver_output=False, estimate_lengths=True, length_scale_init=s0, length_ridge=1e-9)
    out_fit = os.path.join(roots["fit"], "2019_03_07/synth/run", "fte_kinematic")
    assert os.path.exists(os.path.join(out_fit, "fte.pickle"))
    js = json.load(open(os.path.join(out_fit, "skeleton_scale.json")))
    s = np.array(js["length_scale"])
    print(f"|s0 - 1| {np.abs(s0 - 1).max():.3f} -> max |s - 1| {np.abs(s - 1).max():.3e}, sigma of the scales {np.sqrt(np.diag(fit.length_scale_cov)).max():.3e}")
    assert np.array_equal(s, fit.length_scale) and [g[0] for g in js["groups"]] == [n for n, _ in skeleton.LENGTH_GROUPS]
    assert np.array(js["length_scale_cov"]).shape == (G, G)
    assert js["converged"] is True and js["rounds"] == fit.length_calibration["rounds"] >= 1 and js["prior_sigma"] == 0.1 and js["ridge"] == 1e-9
    assert np.abs(s - 1.0).max() < np.abs(s0 - 1.0).max() and np.linalg.norm(s - 1.0) < np.linalg.norm(s0 - 1.0)
    assert bytes(fit.skeleton) == bytes(skeleton.build_skeleton("phantom", 24, length_scale=s)) != nominal
    assert bytes(skeleton.dyn_options("phantom", **E._length_kw(fit))) == bytes(skeleton.dyn_options("phantom", length_scale=s))
    assert E._length_kw(plain) == {}
