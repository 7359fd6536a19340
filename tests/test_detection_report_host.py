"""The detection report (cpe_detection_report, estimator.detection_report), the parts that need no GPU: the two prototypes against the ctypes
mirror, the exported symbols and the wrappers; every refusal through the library; the estimator's fields and keyword refusals; the numpy reference
(tests/detection_compare.py) against brute force on a linear-Gaussian problem, its calibration, its undefined rule and the power of the
comparison; and the CPU route of the experiment the GPU tests repeat (the oracle's solve and band, the reference's report)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cov_compare as CC
import detection_compare as DC
import ingest_compare as IC
from test_covariance_host import _prototype
from cheetah_pose_estimation_amd import _lib, abi, synth
from cheetah_pose_estimation_amd import estimator as E

DETECTION = ("h", "i", "i") + ("p",) * 11
QUAD = (1e6, 2e6, 3e6)              # knots out of reach: the loss is s^2 / 2, kappa = kappa0 = 1


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_signatures(lib):
    """the two prototypes of include/cpe.h against abi.DETECTION_ENTRIES, the exported symbols and the wrappers (fails without the feature)"""
    assert abi.DETECTION_ENTRIES == {"cpe_detection_report": DETECTION, "cpe_detection_report_host": DETECTION}
    for name, kinds in abi.DETECTION_ENTRIES.items():
        fn = getattr(lib, name)                                   # AttributeError when the symbol is missing
        assert _prototype(name) == tuple(abi.ENTRIES[name]) == kinds, name
        assert list(fn.argtypes) == abi.argtypes(name), name
    assert abi.DETECTION_OUTPUTS == DC.KEYS
    sig = inspect.signature(_lib.Handle.detection_report_host).parameters
    assert list(sig) == ["self", "positions", "cov_pos", "meas", "weight", "weight_fit"] and all(sig[k].default is None for k in list(sig)[3:])
    assert callable(_lib.Handle.detection_report)
    for table in ("COVARIANCE_ENTRIES", "SAMPLE_ENTRIES", "RATE_COVARIANCE_ENTRIES", "SCALE_ENTRIES", "SCALE_RESPONSE_ENTRIES"):
        assert not set(getattr(abi, table)) & set(abi.DETECTION_ENTRIES)


def test_refusals(lib):
    """CPE_BAD_ARG with the argument named, before a pointer is used and before the device is touched: every call here has a null handle, and the
    handle is looked at last"""
    buf = (C.c_double * 8)()
    p = C.addressof(buf)

    def call(name, B=1, N=1, positions=p, cov_pos=p, meas=p, weight=p, weight_fit=p, uv=p, cov_px=p, uv_loo=p, cov_loo=p, d2=p, leverage=p):
        st = getattr(lib, name)(None, B, N, positions, cov_pos, meas, weight, weight_fit, uv, cov_px, uv_loo, cov_loo, d2, leverage)
        return st, lib.cpe_last_error()

    def refused(name, reason, **kw):
        st, err = call(name, **kw)
        assert st == abi.BAD_ARG and name.encode() + b": " in err and reason in err, (name, kw, st, err)

    none = dict(meas=None, weight=None, weight_fit=None, uv_loo=None, cov_loo=None, d2=None, leverage=None)
    for name in abi.DETECTION_ENTRIES:
        refused(name, b"negative size", B=-1)
        refused(name, b"negative size", N=-1)
        refused(name, b"too many frames", B=1 << 15, N=1 << 16)
        for k in ("positions", "cov_pos", "uv", "cov_px"):
            refused(name, k.encode() + b" is null", **{k: None})
            refused(name, k.encode() + b" is null", **{**none, k: None})
        refused(name, b"meas and weight are given together", meas=None)
        refused(name, b"meas and weight are given together", weight=None, weight_fit=None)
        refused(name, b"weight_fit without weight", **{**none, "weight_fit": p})
        for k in ("uv_loo", "cov_loo", "d2", "leverage"):
            refused(name, k.encode() + b" requested without measurements", **{**none, k: p})
        refused(name, b"the handle is null")
        refused(name, b"the handle is null", **none)
        refused(name, b"the handle is null", weight_fit=None, uv_loo=None, d2=None)      # each of the four may be null on its own
        refused(name, b"the handle is null", B=0, **{**none, "positions": None, "uv": None})   # an empty call needs no arrays, but a handle


# ---- 2. the estimator's front ------------------------------------------------------------------------------------------------------------
def test_fields_and_keywords(tmp_path):
    assert E.DETECTION_FIELDS == ("uv", "uv_cov", "uv_std", "uv_loo", "uv_loo_cov", "residual", "residual_loo", "d2_loo", "leverage", "outlier",
                                  "held_out", "chi2", "p_outlier", "ridge", "n_detections", "dof_measurements", "log_score", "log_score_held_out")
    assert E.DETECTION_CSV_COLUMNS == ("x", "y", "x_std", "y_std", "xy_corr", "x_loo", "y_loo", "d2_loo", "leverage", "outlier", "held_out")
    sig = inspect.signature(E.detection_report).parameters
    assert list(sig)[:5] == ["estimator", "validate_with", "p_outlier", "out_dir_prefix", "write"]
    assert (sig["validate_with"].default, sig["p_outlier"].default, sig["out_dir_prefix"].default, sig["write"].default) == (None, 1e-3, None, True)
    assert E.CheetahEstimator.__dataclass_fields__["detections"].default is None

    def est(ppm=False, kinetic=None, result=None, uncertainty=None, cam_idx=None, frames=(10, 50)):
        params = E.TrajectoryParams(str(tmp_path), frames[0], frames[1], frames[1] - frames[0], 0.5, None, False, False, False, ppm)
        scene = E.Scene("", None, None, None, None, (2704, 1520), 120.0, 6, cam_idx)
        e = E.CheetahEstimator("phantom", "seq", params, scene, IC.model("phantom24"), synth.make_cameras(6), None, None, 1.0, True)
        e.kinetic, e.result, e.uncertainty = kinetic, result, uncertainty
        return e

    for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="p_outlier"):
            E.detection_report(est(), p_outlier=p)
    with pytest.raises(NotImplementedError, match="pairwise pseudo-measurements"):
        E.detection_report(est(ppm=True))
    with pytest.raises(NotImplementedError, match="pairwise pseudo-measurements"):
        E.detection_report(est(), validate_with=est(ppm=True))
    with pytest.raises(NotImplementedError, match="physics-stage"):
        E.detection_report(est(kinetic=dict(tau=None)))
    with pytest.raises(ValueError, match="no covariance"):
        E.detection_report(est(result=dict(positions=[np.zeros((40, 24, 3))])))
    with pytest.raises(ValueError, match="frames 10..49"):
        E.detection_report(est(cam_idx=2), validate_with=est(frames=(10, 49)))
    with pytest.raises(ValueError, match="multi-view"):
        E.detection_report(est(cam_idx=2), validate_with=est(cam_idx=1))
    with pytest.raises(FileNotFoundError, match="fte_kinematic.*fte.pickle"):
        E.detection_report(est())
    # kappa0 of the default knots, against the reference's carried derivatives
    k0 = float(DC.loss(np.zeros(1), DC.KNOTS, 0)[1][0])
    assert abs(E.loss_centre_curvature(*DC.KNOTS) - k0) < 1e-14 and 1.03 < k0 < 1.05
    assert E.loss_centre_curvature(*QUAD) == 1.0


# ---- 3. the reference: camera derivative, brute force, calibration, undefined rule, power -----------------------------------------------------
def test_camera_jacobian_against_central_differences():
    """the analytic G against a central difference of ingest_compare.project (longdouble, step 1e-7 m: truncation 1e-14 relative, rounding
    1e-19 / 1e-7 = 1e-12 of the pixel scale), at generic points of fisheye and pinhole cameras; tolerance 1e-8 of the largest entry of G"""
    cams = IC.reproject_cameras(6, 25)
    rng = np.random.default_rng(3)
    p = np.array([0.3, -0.5, 0.4]) + rng.uniform(-1.0, 1.0, (40, 3))
    worst = 0.0
    for c in range(6):
        uv, G = DC.project_with_jacobian(cams[c], p)
        assert IC.worst(uv, IC.project(cams[c], p)) <= 1e-12
        h = DC.LD(1e-7)
        for j in range(3):
            d = np.zeros(3, DC.LD); d[j] = h
            cd = (IC.project(cams[c], IC.ld(p) + d) - IC.project(cams[c], IC.ld(p) - d)) / (2 * h)
            worst = max(worst, IC.worst(G[..., j], cd, np.abs(G).max()))
    print(f"G against central differences: {worst:.2e} of its largest entry")
    assert worst <= 1e-8


def test_brute_force_on_a_linear_gaussian_problem():
    """28 unknowns, 48 two-row detections, four with a zero weight in one or both rows: S_loo against J_i (H - J_i^T W_i J_i)^-1 J_i^T and uv_loo
    against the actual refit without the detection, relative 1e-10; the symmetric form against S (I - W S)^-1; the sum of the leverages
    against tr(Sigma J^T W J)"""
    p = DC.linear_problem(48, 5)
    J, W, z = p["J"], p["W"], p["z"]
    uv = J @ p["xh"]
    S = J @ p["Sigma"] @ np.swapaxes(J, -1, -2)
    g = W * (uv - z)
    ul, Sl, lev, tmin, ok = DC.woodbury(uv, S, g, W, np.float64)
    assert ok.all() and tmin.min() > 0.05 and (W == 0).sum() == 5
    eS = eu = ef = 0.0
    for i in range(len(J)):
        u_ref, S_ref = DC.linear_loo(p, i)
        eS = max(eS, np.abs(Sl[i] - S_ref).max() / np.abs(S_ref).max())
        eu = max(eu, np.abs(ul[i] - u_ref).max() / np.abs(u_ref).max())
        form = S[i] @ np.linalg.inv(np.eye(2) - np.diag(W[i]) @ S[i])
        ef = max(ef, np.abs(Sl[i] - form).max() / np.abs(form).max())
    print(f"S_loo - dense inverse {eS:.2e}, uv_loo - refit {eu:.2e}, symmetric form - S (I - W S)^-1 {ef:.2e}")
    assert eS <= 1e-10 and eu <= 1e-10 and ef <= 1e-10
    H_meas = np.einsum("nda,nd,ndb->ab", J, W, J)
    assert abs(lev.sum() - np.trace(p["Sigma"] @ H_meas)) <= 1e-10 * lev.sum()


def test_calibration_of_d2():
    """2000 detections drawn from the model (seed 9; prior on 28 unknowns, both rows of a detection at one weight): the mean of d2 is within 0.2 of
    2 (a chi-square with 2 degrees of freedom; its mean over 2000 draws has standard deviation 0.045), and the naive r^T (S + sigma2 I)^-1 r of
    the raw residual is below it"""
    rng = np.random.default_rng([9, 1])                     # (its own stream: linear_problem draws J from seed 9's)
    p = DC.linear_problem(2000, 9, zero_rows=False)
    w = rng.uniform(0.5, 2.0, 2000)
    # rebuild the problem with one weight per detection (W = w^2 in both rows) and noise of that precision
    J = p["J"]
    z = J @ p["x"] + rng.normal(size=(2000, 2)) / w[:, None]
    W = np.repeat((w * w)[:, None], 2, axis=1)
    H = p["P0"] + np.einsum("nda,nd,ndb->ab", J, W, J)
    Sigma = np.linalg.inv(H)
    xh = Sigma @ np.einsum("nda,nd,nd->a", J, W, z)
    uv, S = J @ xh, J @ Sigma @ np.swapaxes(J, -1, -2)
    out = DC.leave_one_out(uv, S, z, w, w, QUAD, 0, np.float64)
    d2 = out["d2"]
    r = z - uv
    C = S + (1.0 / (w * w))[:, None, None] * np.eye(2)
    naive = np.einsum("na,nab,nb->n", r, np.linalg.inv(C), r)
    print(f"mean d2 {d2.mean():.4f}, mean of the raw-residual form {naive.mean():.4f}, leverage sum {out['leverage'].sum():.3f}")
    assert np.isfinite(d2).all() and abs(d2.mean() - 2.0) <= 0.2
    assert naive.mean() < d2.mean()
    assert abs(out["leverage"].sum() - np.trace(Sigma @ np.einsum("nda,nd,ndb->ab", J, W, J))) <= 1e-9 * 28


def test_undefined_rule():
    """the smaller eigenvalue of T at -0.5: NaN in uv_loo, cov_loo and d2; at 0.5: numbers; the leverage is finite in both"""
    S = np.array([[[1.0, 0.2], [0.2, 0.8]]] * 2)
    ev = np.linalg.eigvalsh(S[0])[-1]                       # T = I - w^2 S with the quadratic loss: smaller eigenvalue 1 - w^2 ev
    w = np.sqrt(np.array([1.5, 0.5]) / ev)
    uv, z = np.array([[100.0, 200.0]] * 2), np.array([[100.5, 199.0]] * 2)
    out = DC.leave_one_out(uv, S, z, w, w, QUAD, 0)
    assert np.allclose(np.asarray(out["tmin"], float), [-0.5, 0.5], atol=1e-12)
    assert np.isnan(out["uv_loo"][0]).all() and np.isnan(out["cov_loo"][0]).all() and np.isnan(out["d2"][0])
    assert np.isfinite(out["uv_loo"][1]).all() and np.isfinite(out["cov_loo"][1]).all() and np.isfinite(out["d2"][1])
    assert np.isfinite(out["leverage"]).all() and (out["leverage"] > 0).all()
    # no detection: copied; held out: the raw residual's distance
    o = DC.leave_one_out(uv, S, z, np.array([0.0, 1.0]), np.array([0.0, 0.0]), DC.KNOTS, 0, np.float64)
    assert np.array_equal(o["uv_loo"], uv) and np.array_equal(o["cov_loo"], S) and np.isnan(o["d2"][0]) and not o["leverage"].any()
    k0 = float(DC.loss(np.zeros(1), DC.KNOTS, 0, np.float64)[1][0])
    r = z[1] - uv[1]
    assert abs(o["d2"][1] - r @ np.linalg.inv(S[1] + np.eye(2) / k0) @ r) <= 1e-14


@pytest.mark.parametrize("variant,keys", [("sign", ("uv_loo", "d2")), ("kappa0", ("d2",)), ("w_for_wf", ("uv_loo", "cov_loo", "leverage"))])
def test_power_of_the_comparison(variant, keys):
    """a reference with the sign of S_loo g flipped, without kappa0, or with w where the statement has w_f (on a held-out detection) is further
    than 100 x the tolerance from the reference on at least one case, in every key the mistake touches"""
    hit = {k: 0.0 for k in keys}
    for case in DC.CASES[:6]:
        cams = DC.case_inputs(case)["cams"]
        tol = DC.tolerance(case)
        d = DC.distances(DC.case_reference(case, DC.LD, variant), DC.case_reference(case), cams)
        for k in keys:
            hit[k] = max(hit[k], d[k] / tol[k])
    print(variant, {k: f"{v:.1e} x tolerance" for k, v in hit.items()})
    assert all(v > 100.0 for v in hit.values())


def test_reference_float64_error_and_conditions():
    """every accuracy case satisfies the case conditions (asserted by case_reference) and holds every kind of detection; the worst distance
    between the float64 and the longdouble reference per key is printed (detection_compare's docstring records it)"""
    worst = {}
    for case in DC.CASES:
        c = DC.case_inputs(case)
        ref = DC.case_reference(case)
        for k, v in DC.distances(DC.case_reference(case, np.float64), ref, c["cams"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        und = np.isnan(np.asarray(ref["d2"], dtype=np.float64)) & (c["weight"] > 0)
        assert np.array_equal(und, c["kinds"]["undefined"])
        if case[0] != (1, 1):
            assert all(c["kinds"][k].any() for k in ("undefined", "held", "none", "half"))
            s = np.abs(np.asarray(ref["s"], dtype=np.float64))
            assert all(((s > lo) & (s < hi)).any() for lo, hi in DC.REGIMES)
            W0 = np.asarray(DC.loss(ref["s"], DC.KNOTS, c["mode"])[1], dtype=np.float64)
            assert ((W0[..., 0] == 0) != (W0[..., 1] == 0)).any() or c["mode"] == 0            # one coordinate's W exactly zero (mode 1, 10..20)
    print("float64 reference - longdouble reference, worst per key:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert set(worst) == set(DC.KEYS)


# ---- 4. the CPU route of the experiment on the project's own fit ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_fit(oracle):
    """the oracle's solve of detection_compare.fit_data, its undamped band inverted densely, the marker Jacobians by central differences, and
    the numpy reference's report at the solution"""
    d = DC.fit_data()
    sk, cams, opts = d["sk"], d["cams"], d["opts"]
    q = oracle.solve(sk, cams, opts, None, d["q_init"], d["meas"], d["weight"])["q"]
    _, _, H, _, qc = oracle.objective(sk, cams, opts, None, q, d["meas"], d["weight"], want_grad=True, want_H=True)
    Bk, Hk = CC.LC._blocks_from_band(H, q.shape[0], 3)
    diag = CC.dense_inverse(Bk, Hk)[0]
    P = CC.marker_jacobians(oracle, sk, qc, range(q.shape[0]), 1e-6)
    cov_pos = CC.marker_covariance(P, diag)
    pos = synth.fk_numpy(sk, qc)[0]
    rep = DC.reference(cams, DC.KNOTS, 0, pos[None], cov_pos[None], d["meas"][None], d["weight"][None], dtype=np.float64)
    return dict(q=qc, pos=pos, cov_pos=cov_pos, rep={k: np.asarray(v[0], dtype=np.float64) for k, v in rep.items()})


def test_planted_outliers_are_flagged_on_the_cpu_route(cpu_fit):
    """all 10 planted detections are flagged at p = 1e-3 and at most 1 % of the others (0.1 % expected under the model)"""
    d = DC.fit_data()
    flag = DC.flagged(cpu_fit["rep"]["d2"], d["weight"])
    others = (d["weight"] > 0) & ~d["mask"]
    print(f"seed {DC.FIT_SEED}: planted flagged {int(flag[d['mask']].sum())} / {DC.FIT_PLANTED}, others flagged {int(flag[others].sum())} / {int(others.sum())}; "
          f"d2 of the planted {np.sort(cpu_fit['rep']['d2'][d['mask']]).round(1)}; leverage sum {cpu_fit['rep']['leverage'].sum():.1f} of {28 * DC.FIT_N}")
    assert d["mask"].sum() == DC.FIT_PLANTED and flag[d["mask"]].all()
    assert flag[others].sum() <= 0.01 * others.sum()


def test_loo_against_the_oracles_refit(oracle, cpu_fit):
    """three inliers of largest leverage and one planted outlier: the detection's weight zeroed, the oracle re-solved from the solution, the
    marker reprojected -- against uv_loo, relative to |uv_loo - uv|.  First-order agreement: the figure is what detection_compare.REFIT_CPU
    records (the GPU test allows 4 x it)"""
    d = DC.fit_data()
    rep = cpu_fit["rep"]
    worst = 0.0
    for n, c, l in DC.refit_targets(rep["leverage"], d["mask"], d["weight"]):
        w = d["weight"].copy()
        w[n, c, l] = 0.0
        q2 = oracle.solve(d["sk"], d["cams"], d["opts"], None, cpu_fit["q"], d["meas"], w)["q"]
        uv2 = np.asarray(IC.project(d["cams"][c], synth.fk_numpy(d["sk"], q2[n])[0][l]), dtype=np.float64)
        move = np.linalg.norm(rep["uv_loo"][n, c, l] - rep["uv"][n, c, l])
        miss = np.linalg.norm(uv2 - rep["uv_loo"][n, c, l]) / move
        print(f"detection {(n, c, l)}: leverage {rep['leverage'][n, c, l]:.3f}, |uv_loo - uv| {move:.3e} px, refit - uv_loo {miss:.3f} of it")
        worst = max(worst, miss)
    print(f"worst {worst:.3f} (recorded REFIT_CPU {DC.REFIT_CPU})")
    assert worst <= DC.REFIT_CPU
