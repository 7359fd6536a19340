"""The comparator of k_frame_normal (tests/frame_compare.py) on the CPU: its tolerances still stand on the two CPU measurements they were derived
from; every GPU case's inputs satisfy the conditions and exercise what the case is named for, by the reference alone; the oracle's per-frame
terms agree with the extended reference in BOTH curvature modes; the stencil of J_u agrees with the oracle's analytic Jacobian where Z' is the
identity; and planted faults are flagged.  CPU only."""
import numpy as np
import pytest

import frame_compare as FC
import resjac_compare as RC
from cheetah_pose_estimation_amd import abi, synth


@pytest.fixture(scope="module")
def measured(oracle):
    """(measurement 1, measurement 2, the oracle's distance from the extended reference in both curvature modes) over every GPU case's inputs"""
    return FC.measure(oracle, log=lambda s: print(s))


def test_tolerances_are_set_and_ordered():
    for k in FC.MEASURED_KEYS:
        assert FC.TOL[k] == FC.MARGIN * max(FC.MEASURED[k]) and 0.0 < FC.TOL[k] < 2e-8, k
    assert FC.TOL["sym"] == FC.TOL["Bm"] and FC.TOL["sym_exact"] == 0.0


def test_tolerances_stand_on_the_two_measurements(measured):
    m1, m2, _ = measured
    for k in FC.MEASURED_KEYS:
        print(f"{k}: (1) {m1[k]:.2e} (TOL / it = {FC.TOL[k] / m1[k]:.1f}), (2) {m2[k]:.2e}")
    for k in FC.MEASURED_KEYS:
        assert 16.0 <= FC.TOL[k] / m1[k] <= 128.0, (k, m1[k], FC.TOL[k])
        assert m2[k] < FC.TOL[k] / 8.0, (k, m2[k], FC.TOL[k])


def test_oracle_agrees_with_the_extended_reference_in_both_curvature_modes(measured):
    """at least as well as the GPU tests allow the oracle: 2e-6 on g and Bm, 1e-9 on cost (the first test of the oracle's mode 1)"""
    mo = measured[2]
    print("oracle: " + ", ".join(f"{k} {mo[k]:.2e}" for k in FC.KEYS))
    assert mo["g"] <= 2e-6 and mo["Bm"] <= 2e-6 and mo["sym"] <= 2e-6 and mo["cost"] <= 1e-9 and mo["q_out"] == 0.0


@pytest.mark.parametrize("name", FC.CASES)
def test_case_inputs(name, oracle):
    """the conditions on the inputs, the numpy map against the oracle's consistent q, and what the case is named for -- by the reference alone"""
    c, R = FC.case_inputs(name), FC.case_reference(oracle, name)
    cond = R["conditions"]
    assert c["q"].shape[:2] == (FC.B, FC.N) and FC.conditions_hold(R), cond
    assert cond["near"] == 0 and cond["small_s"] == 0 and cond["bound_margin"] >= FC.BOUND_MARGIN and cond["weighted"] > 0
    assert len(cond["camera_inliers"]) == len(c["cams"]) and min(cond["camera_inliers"]) >= FC.MIN_CAMERA_INLIERS, cond["camera_inliers"]
    assert np.abs(R["q"].astype(np.float64) - R["q_out"]).max() < 1e-12
    if name.startswith("loss"):
        assert min(cond["pieces"]) >= 0.05
    if name == "knots":
        assert R["active"].any()
    if name == "weights":
        f = c["zero_frame"][0] * FC.N + c["zero_frame"][1]
        assert not R["active"][f].any() and not R["g"][f].any() and not R["Bm"][f].any() and R["cost"][f, 0] != 0
    if name == "bounds":
        for b, n, i, side in c["expect_active"]:
            assert R["active"][b * FC.N + n, i, side] and R["cost"][b * FC.N + n, 1] > 0
    if name.startswith("prior"):
        assert np.all(R["cost"][:, 2] != 0) and np.abs(R["g_prior"]).max() > 1.0
    if name.startswith("cams"):
        assert FC.CAMW * 13 < FC.n_camov(c["sk"]) < FC.CAMW * 14


def test_curvature_modes_differ_in_the_reference(oracle):
    R0, R1 = FC.case_reference(oracle, "loss-c0"), FC.case_reference(oracle, "loss-c1")
    assert np.array_equal(R0["g"], R1["g"]) and np.array_equal(R0["cost"], R1["cost"])
    assert FC.relative_difference(R0["Bm"], R1["Bm"], R0["Bm_scale"]) > 1e-3


def test_stencil_against_the_analytic_jacobian_where_the_coordinate_map_is_the_identity(oracle):
    """J_u of the extrapolated stencil = (projection gradient) (oracle.markers_jac) on the coordinates whose column of Z' is a unit vector (base
    position, neck angles), in units of the row's largest entry, both rigs"""
    seen = 0
    for name in ("plain", "knots"):
        c, R = FC.case_inputs(name), FC.case_reference(oracle, name)
        q, meas, weight = FC.flat(c)
        ind = FC.tables(c["sk"])[0]
        for f in (0, 7):
            Z = oracle.frame_normal(c["sk"], c["cams"], c["opts"], None, q[f], meas[f], weight[f])[3]
            cols = [k for k in range(abi.NX) if np.count_nonzero(Z[:, k]) == 1]
            assert set(range(3)) <= set(cols) and len(cols) >= 6
            pos, dpos = oracle.markers_jac(c["sk"], R["q_out"][f])
            for cc in range(len(c["cams"])):
                for l in range(c["sk"].n_markers):
                    if R["w"][f, cc, l] == 0:
                        continue
                    G = oracle.project(c["cams"][cc], pos[l], want_G=True)[1]
                    Ja = G @ dpos[l][:, [ind[k] for k in cols]]
                    Js = R["J"][f, cc, l][:, cols].astype(np.float64)
                    assert np.abs(Js - Ja).max() <= 1e-11 * np.abs(R["J"][f, cc, l]).max().astype(np.float64)
                    seen += 1
    assert seen > 100


@pytest.fixture(scope="module")
def bounds_case(oracle):
    R = FC.case_reference(oracle, "bounds")
    G = FC.outputs(R)
    G["Bm"] = 0.5 * (G["Bm"] + np.swapaxes(G["Bm"], 1, 2))                            # (the einsum's two triangles differ in the last bit)
    return R, G


def test_outputs_of_the_reference_pass(bounds_case):
    R, G = bounds_case
    d = FC.discrepancies(dict(G, q_out=R["q_out"]), R)
    assert not FC.failures(d) and max(d[k] for k in ("cost", "g", "Bm", "sym", "q_out")) < 1e-15, d


@pytest.mark.parametrize("fault", ["g entry", "Bm entry", "Bm asymmetric", "Bm asymmetric, exact frame", "cost", "bound cost", "q_out", "nan"])
def test_planted_faults_are_flagged(fault, bounds_case):
    R, G0 = bounds_case
    G = {k: v.copy() for k, v in G0.items()}
    G["q_out"] = R["q_out"].copy()
    fa = int(np.flatnonzero(~R["sym_exact"])[0]); fe = int(np.flatnonzero(R["sym_exact"])[0])
    rel = 4.0 * FC.TOL["Bm"]
    if fault == "g entry":
        G["g"][3, 5] += rel * float(R["g_scale"][3, 5]); want = {"g"}
    elif fault == "Bm entry":
        G["Bm"][fa, 2, 7] += rel * float(R["Bm_scale"][fa, 2, 7]); G["Bm"][fa, 7, 2] = G["Bm"][fa, 2, 7]; want = {"Bm"}
    elif fault == "Bm asymmetric":
        G["Bm"][fa, 2, 7] += rel * float(R["Bm_scale"][fa, 2, 7]); want = {"Bm", "sym"}
    elif fault == "Bm asymmetric, exact frame":
        G["Bm"][fe, 2, 7] = np.nextafter(G["Bm"][fe, 2, 7], np.inf); want = {"sym_exact"}
    elif fault == "cost":
        G["cost"][4, 0] *= 1.0 + 4.0 * FC.TOL["cost"]; want = {"cost"}
    elif fault == "bound cost":
        G["cost"][fe, 1] = 1e-300; want = {"cost"}                                  # the reference's value is exactly zero there
    elif fault == "q_out":
        G["q_out"][6, 20] += 4.0 * FC.TOL["q_out"]; want = {"q_out"}
    else:
        G["g"][0, 0] = np.nan; want = {"g"}
    assert set(FC.failures(FC.discrepancies(G, R))) == want


@pytest.mark.parametrize("what", ["curvature mode", "camera multiplier", "bound penalty", "loss knots"])
def test_a_wrong_option_is_flagged(what, oracle):
    """the reference evaluated with one option wrong -- the other curvature mode, the multipliers dropped, model 0's penalty or knots -- fails
    the comparison with the right one by orders of magnitude"""
    name = {"curvature mode": "loss-c1", "camera multiplier": "knots", "bound penalty": "bounds", "loss knots": "knots"}[what]
    c, R = FC.case_inputs(name), FC.case_reference(oracle, name)
    opts, cams = abi.Options.from_buffer_copy(bytes(c["opts"])), c["cams"]
    if what == "curvature mode":
        opts.curvature = 0
    elif what == "camera multiplier":
        cams = (abi.Camera * len(cams))(*[abi.Camera.from_buffer_copy(bytes(cam)) for cam in cams])
        for cam in cams:
            cam.mult = 1.0
    elif what == "bound penalty":
        opts.bound_penalty = 3e3
    else:
        opts.loss_a, opts.loss_b, opts.loss_c = 3.0, 10.0, 20.0
    q, meas, weight = FC.flat(c)
    W = FC.outputs(FC.evaluate(c["sk"], cams, opts, c["pr"], R["q_out"], meas, weight, np.float64))
    bad = FC.failures(FC.discrepancies(W, dict(R, q_out=R["q"])))
    assert "Bm" in bad and bad["Bm"] > 1e4 * FC.TOL["Bm"], bad
    if what != "curvature mode":
        assert bad["g"] > 1e4 * FC.TOL["g"] and bad["cost"] > 1e4 * FC.TOL["cost"], bad


def test_near_and_small_residuals_are_counted(oracle):
    """the conditions do count what they are there to exclude"""
    c = FC.case_inputs("cams1")
    q, meas, weight = FC.flat(c)
    R = FC.case_reference(oracle, "cams1")
    on = np.argwhere(R["w"][0] != 0)[0]
    m2 = meas.copy()
    m2[0, on[0], on[1], 0] += float(R["s"][0, on[0], on[1], 0] / R["w"][0, on[0], on[1]])       # this residual becomes ~0
    R2 = FC.reference(oracle, c["sk"], c["cams"], c["opts"], None, q[:1], m2[:1], weight[:1])
    assert R2["conditions"]["small_s"] == 1 and not FC.conditions_hold(R2)
    z = RC.depth(c["sk"], c["cams"], q[:1])
    assert np.abs(z[weight[:1] > 0]).min() >= FC.NEAR_Z
