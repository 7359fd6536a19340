"""Covariance between distant frames on the GPU (cpe_covariance_columns, include/cpe.h; estimator.span_uncertainty and the uncertainty_spans
keyword) against the numpy references of tests/span_compare.py: the columns on random block bands and on the solver's own factor of the oracle
cases, the layout rules (band rows bit-equal, exact zeros), the batch rules, short and ragged sequences, the refusals, and the estimator through
files.

Error units and tolerances: span_compare's (10 x max(r, 2^-52 x scaled condition), r = the discrepancy between the helper's two float64 routes on
that matrix) -- measured on the reference, never on the GPU.  test_zz_report prints every measured value next to its tolerance."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

import cov_compare as CC
import lm_compare as LC
import span_compare as SC
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

REPORT = []                                      # (label, measure, value, tolerance)
NX = 28


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _pb_handle(factory, PB):
    """a handle of half-bandwidth PB (the band entries read nothing else of it)"""
    if PB == 3:
        return factory(skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options())
    return factory(skeleton.build_skeleton("phantom", 24), synth.make_cameras(2), abi.default_options(), priors.load_priors())


def _layout_failures(cols, diag, off, anchors):
    """what is wrong with the layout of one sequence's columns [K][N][28][28]: rows a-PB .. a bit-equal to the band, exact zeros elsewhere"""
    bad = []
    N, PB = off.shape[0], off.shape[1]
    for k, a in enumerate(anchors):
        if a < 0:
            if cols[k].any():
                bad.append(f"slot {k} (unused) is not zero")
            continue
        if cols[k, a + 1:].any():
            bad.append(f"anchor {a}: non-zero below the anchor")
        if not _bits(cols[k, a], diag[a]):
            bad.append(f"anchor {a}: row a is not Sigma(a,a)")
        for i in range(1, min(PB, a) + 1):
            if not _bits(cols[k, a - i], off[a - i, i - 1].T):
                bad.append(f"anchor {a}: row a-{i} is not the transposed band block")
    return bad


# ---- 1. random bands: cpe_band_inverse, then the columns -------------------------------------------------------------------------------
@pytest.mark.parametrize("N,PB", [(9, 3), (57, 4)])
def test_columns_on_random_bands(gpu_handle_factory, N, PB):
    h = _pb_handle(gpu_handle_factory, PB)
    assert h.pb == PB
    bands = [CC.random_band(N, PB, 2000 * PB + 10 * N + b) for b in range(2)]
    L = np.stack([CC.cholesky_layout(Ad, Hk) for Ad, Hk in bands])
    diag, off = h.band_inverse_host(L)
    anchors = [N - 1, N // 2, PB + 1, PB, 0, -1]
    A2 = np.array([anchors, anchors], dtype=np.int32)
    cols = h.covariance_columns_host(L, diag, off, A2)
    assert cols.shape == (2, len(anchors), N, NX, NX)
    for b, (Ad, Hk) in enumerate(bands):
        R = SC.reference(Ad, Hk, anchors[:-1])
        err = SC.column_error(cols[b, :-1], R["cols"], R["diag"], anchors[:-1])
        _note(f"random N {N} PB {PB} #{b}", "column error", err, R["tol"])
        assert err <= R["tol"], (b, err, R["tol"])
        bad = _layout_failures(cols[b], diag[b], off[b], anchors)
        assert not bad, (b, bad)
    assert _bits(h.covariance_columns_host(L, diag, off, A2), cols)                                    # a second run
    for b in range(2):                                                                                   # alone, and the other order in the batch
        assert _bits(h.covariance_columns_host(L[b:b + 1], diag[b:b + 1], off[b:b + 1], A2[:1])[0], cols[b]), b
    assert _bits(h.covariance_columns_host(L[::-1].copy(), diag[::-1].copy(), off[::-1].copy(), A2)[::-1], cols)
    for k, a in enumerate(anchors):                                                                      # one anchor per call, K = 1
        one = h.covariance_columns_host(L, diag, off, np.array([[a], [a]], dtype=np.int32))
        assert _bits(one[:, 0], cols[:, k]), a
    mixed = h.covariance_columns_host(L, diag, off, np.array([[0, N - 1], [-1, -1]], dtype=np.int32))    # a sequence without any anchor
    assert _bits(mixed[0, 1], cols[0, 0]) and _bits(mixed[0, 0], cols[0, 4]) and not mixed[1].any()


# ---- 2. short sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ["1", "PB+1", "PB+2"])
def test_columns_on_short_sequences(gpu_handle_factory, N):
    """one frame; the longest sequence without a row outside the band; the first with one"""
    PB = 3
    N = {"1": 1, "PB+1": PB + 1, "PB+2": PB + 2}[N]
    h = _pb_handle(gpu_handle_factory, PB)
    Ad, Hk = CC.random_band(N, PB, 3000 + N)
    L = CC.cholesky_layout(Ad, Hk)[None]
    diag, off = h.band_inverse_host(L)
    anchors = sorted({N - 1, N // 2, 0}, reverse=True)
    cols = h.covariance_columns_host(L, diag, off, [anchors])
    R = SC.reference(Ad, Hk, anchors)
    err = SC.column_error(cols[0], R["cols"], R["diag"], anchors)
    _note(f"short N {N}", "column error", err, R["tol"])
    assert err <= R["tol"]
    assert not _layout_failures(cols[0], diag[0], off[0], anchors)


# ---- 3. sequences of their own length in one call ---------------------------------------------------------------------------------------
def test_columns_with_n_frames(gpu_handle_factory):
    """lengths (5, 12, 40) in one call at N = 40: every sequence byte-equal to its own call, rows past its length zero; what lies past a
    sequence's frames in the inputs is NaN here, so it is not read"""
    PB, lens, Nm = 3, (5, 12, 40), 40
    h = _pb_handle(gpu_handle_factory, PB)
    own, Lp, dp, op = [], np.full((3, Nm, PB + 1, NX, NX), np.nan), np.full((3, Nm, NX, NX), np.nan), np.full((3, Nm, PB, NX, NX), np.nan)
    anchors = np.full((3, 3), -1, dtype=np.int32)
    for b, n in enumerate(lens):
        Ad, Hk = CC.random_band(n, PB, 4000 + n)
        L = CC.cholesky_layout(Ad, Hk)[None]
        diag, off = h.band_inverse_host(L)
        anchors[b] = [n - 1, n // 2, 0]
        own.append(h.covariance_columns_host(L, diag, off, anchors[b:b + 1])[0])
        Lp[b, :n], dp[b, :n], op[b, :n] = L[0], diag[0], off[0]
        R = SC.reference(Ad, Hk, anchors[b])
        err = SC.column_error(own[b], R["cols"], R["diag"], anchors[b])
        _note(f"n_frames {n}", "column error", err, R["tol"])
        assert err <= R["tol"]
    cols = h.covariance_columns_host(Lp, dp, op, anchors, n_frames=lens)
    for b, n in enumerate(lens):
        assert _bits(cols[b, :, :n], own[b]), b
        assert not cols[b, :, n:].any(), b
    # a sequence of zero frames takes no anchor
    cols0 = h.covariance_columns_host(Lp, dp, op, np.array([[-1], [11], [-1]], dtype=np.int32), n_frames=(0, 12, 40))
    assert not cols0[0].any() and not cols0[2].any() and _bits(cols0[1, 0, :12], own[1][0])


# ---- 4. the solver's own factor of the oracle cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("name", ["six", "mono"])
def test_columns_of_the_solvers_factor(oracle, gpu_handle_factory, name, ridge):
    """cpe_covariance's factor (existing code) -> columns for the anchors 39, 20, 5 against the numpy dense inverse of L L^T of that factor, within
    cov_compare.reference's tolerance of that matrix"""
    c = CC.oracle_case(oracle, name)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    out = h.covariance_host(c["q"][None], c["meas"][None], c["weight"][None], ridge, want_L=True)
    assert out["seq_status"] == [abi.OK]
    anchors = [39, 20, 5]
    cols = h.covariance_columns_host(out["L"], out["cov_diag"], out["cov_off"], [anchors])
    Md, Mk = LC.factor_product(out["L"][0])
    R = CC.reference(Md, Mk, want_dense=True)
    err = SC.column_error(cols[0], SC.columns_dense(R["S"], anchors), R["diag"], anchors)
    _note(f"solver's factor {name} ridge {ridge:g}", "column error", err, R["tol_err"])
    _note(f"solver's factor {name} ridge {ridge:g}", "scaled condition", R["cond"], np.inf)
    assert err <= R["tol_err"], (err, R["tol_err"])
    assert not _layout_failures(cols[0], out["cov_diag"][0], out["cov_off"][0], anchors)
    if name == "mono" and ridge == 0.0:
        # what the feature is for: frames 10 and 30 of the base position are strongly correlated with one camera
        s = np.sqrt(np.diagonal(out["cov_diag"][0], axis1=1, axis2=2))
        col30 = h.covariance_columns_host(out["L"], out["cov_diag"], out["cov_off"], [[30]])[0, 0]
        corr = [col30[10][i, i] / (s[10, i] * s[30, i]) for i in (0, 1)]
        _note("mono ridge 0", "correlation of base x between frames 10 and 30", corr[0], np.inf)
        assert min(corr) > 0.5


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_handle_factory):
    """an anchor equal to the sequence's frame count, K = 0, a null cols: CpeError with the reason; nothing is launched (the device pointers below
    are not device memory -- a launch would fault)"""
    h = _pb_handle(gpu_handle_factory, 3)
    N = 6
    L, d, o = np.zeros((1, N, 4, NX, NX)), np.zeros((1, N, NX, NX)), np.zeros((1, N, 3, NX, NX))
    with pytest.raises(_lib.CpeError, match=r"anchor 6 of sequence 0 outside -1\.\.5"):
        h.covariance_columns_host(L, d, o, [[N]])
    with pytest.raises(_lib.CpeError, match=r"anchor 4 of sequence 0 outside -1\.\.3"):
        h.covariance_columns_host(L, d, o, [[4]], n_frames=[4])
    with pytest.raises(_lib.CpeError, match="anchor -2"):
        h.covariance_columns_host(L, d, o, [[-2]])
    with pytest.raises(_lib.CpeError, match="frame count of sequence 0 outside 0..N"):
        h.covariance_columns_host(L, d, o, [[0]], n_frames=[N + 1])
    with pytest.raises(_lib.CpeError, match="K must be at least 1"):
        h.covariance_columns_host(L, d, o, np.zeros((1, 0), dtype=np.int32))
    fn, fh = h.lib.cpe_covariance_columns, h.lib.cpe_covariance_columns_host
    one = (C.c_int32 * 1)(0)
    p = L.ctypes.data                                     # a host address in the place of a device pointer: never dereferenced
    for f in (fn, fh):
        assert f(h._h, 1, N, None, p, p, p, 1, one, None) == abi.BAD_ARG and b"null argument" in h.lib.cpe_last_error()
        assert f(h._h, 1, N, None, None, p, p, 1, one, p) == abi.BAD_ARG and b"null argument" in h.lib.cpe_last_error()
        assert f(h._h, 1, N, None, p, p, p, 1, None, p) == abi.BAD_ARG and b"null argument" in h.lib.cpe_last_error()
        assert f(h._h, 1, N, None, p, p, p, 0, one, p) == abi.BAD_ARG and b"K must be" in h.lib.cpe_last_error()
        assert f(h._h, 1, N, None, p, p, p, 1, (C.c_int32 * 1)(N), p) == abi.BAD_ARG and b"anchor 6" in h.lib.cpe_last_error()
        assert f(h._h, -1, N, None, p, p, p, 1, one, p) == abi.BAD_ARG and b"negative size" in h.lib.cpe_last_error()
        assert f(h._h, 1 << 20, 1 << 10, None, p, p, p, 4, one, p) == abi.BAD_ARG and b"too many frames" in h.lib.cpe_last_error()
    # half-bandwidth above 4: cov_check's wording
    w5 = priors.load_priors(path=os.path.join(os.path.dirname(__file__), "golden", "priors_k3_w5_dense.npz"))
    h5 = gpu_handle_factory(skeleton.build_skeleton("phantom", 24), synth.make_cameras(2), abi.default_options(), w5)
    assert h5.pb == 5
    with pytest.raises(_lib.CpeError, match="half-bandwidth 5 .* is not supported by the covariance sweep"):
        h5.covariance_columns_host(np.zeros((1, N, 6, NX, NX)), d, np.zeros((1, N, 5, NX, NX)), [[0]])


# ---- 6. the estimator, through files -----------------------------------------------------------------------------------------------------
def _init(E, root, path, **kw):
    return E.init_trajectory(root_dir=root, data_path=path, cheetah_name="phantom", kinetic_dataset=False, solver_path="/unused/ipopt",
                             kinematic_model=True, **kw)


def _span_shapes(E, S, L=24):
    shapes = dict(span_frames=(S, 2), span_seconds=(S,), span_com_displacement=(S, 3), span_com_displacement_cov=(S, 3, 3),
                  span_com_displacement_std=(S, 3), span_distance=(S,), span_distance_std=(S,), span_mean_velocity=(S, 3),
                  span_mean_velocity_cov=(S, 3, 3), span_mean_velocity_std=(S, 3), span_mean_speed=(S,), span_mean_speed_std=(S,),
                  span_positions_displacement_cov=(S, L, 3, 3), span_positions_displacement_std=(S, L, 3))
    assert set(shapes) == set(E.SPAN_FIELDS)
    return shapes


TODAY = ("cov_u", "u_std", "positions_cov", "positions_std", "ridge")


def test_estimate_kinematics_writes_spans(tmp_path):
    """single call: every field of SPAN_FIELDS, the covariances against the numpy propagation from the dense inverse of the exported factor;
    ragged batch over three sequences of different length and rig: byte-equal fields; uncertainty_spans=None: today's keys only"""
    sys.path.insert(0, os.path.dirname(__file__))
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    SPANS = [(0, -1), (2, 9)]
    specs = [("2019_03_07/synth/run1", 24, 5, 6), ("2019_03_07/synth/run2", 17, 9, 6), ("2019_03_09/synth/run3", 30, 6, 4)]
    roots = {k: str(tmp_path / k) for k in ("unc", "single", "ragged")}
    ests = {}
    for k, root in roots.items():
        for path, N, seed, nc in specs:
            write_dataset(root, data_path=path, N=N, seed=seed, n_cams=nc)
        ests[k] = [_init(E, root, p) for p, _, _, _ in specs]
    assert E.estimate_kinematics(ests["unc"][0], solver_output=False, uncertainty=True)
    assert all(E.estimate_kinematics(e, solver_output=False, uncertainty=True, uncertainty_spans=SPANS) for e in ests["single"])
    assert E.estimate_kinematics_batch(ests["ragged"], ragged=True, uncertainty=True, uncertainty_spans=SPANS) == [True] * 3
    zu = np.load(os.path.join(roots["unc"], specs[0][0], "fte_kinematic", "uncertainty.npz"))
    assert sorted(zu.files) == sorted(TODAY) and sorted(ests["unc"][0].uncertainty) == sorted(TODAY)
    for k, (path, N, _, _) in enumerate(specs):
        za = np.load(os.path.join(roots["single"], path, "fte_kinematic", "uncertainty.npz"))
        zb = np.load(os.path.join(roots["ragged"], path, "fte_kinematic", "uncertainty.npz"))
        shapes = _span_shapes(E, len(SPANS))
        assert sorted(za.files) == sorted(TODAY + tuple(shapes)) == sorted(zb.files) == sorted(ests["single"][k].uncertainty)
        for key in za.files:
            assert _bits(za[key], zb[key]), (k, key)                                   # ragged=True matches the single call bit for bit
            assert _bits(za[key], np.asarray(ests["single"][k].uncertainty[key])) and _bits(zb[key], np.asarray(ests["ragged"][k].uncertainty[key])), (k, key)
        for key, shp in shapes.items():
            assert za[key].shape == shp, key
        if k == 0:
            assert all(_bits(za[key], zu[key]) for key in TODAY)                       # the spans change nothing of today's fields
        est = ests["single"][k]
        assert np.array_equal(za["span_frames"], [[0, N - 1], [2, 9]])
        assert np.all(za["span_com_displacement_std"] > 0.0) and np.all(za["span_positions_displacement_std"] > 0.0) and np.all(za["span_distance_std"] > 0.0)
        assert _bits(za["span_com_displacement"], est.com_pos[[N - 1, 9]] - est.com_pos[[0, 2]])
        assert np.allclose(za["span_mean_velocity"][0], est.com_vel.mean(axis=0), rtol=1e-10, atol=1e-12)
        # the reference: the same handle the estimator built, its exported factor, numpy from there on
        _, opts, pri = E._kin_prepare(est, False, False, False, 5, 4, True, None, None)
        h = _lib.Handle(est.skeleton, est.cams, opts, pri)
        try:
            cov = h.covariance_host(est.result["q"], est.meas[None], est.weight[None], 0.0, want_L=True)
            jac = h.rate_covariance_host(est.result["q"], cov["cov_diag"], cov["cov_off"], want=("jac_pos", "jac_com"))
        finally:
            h.close()
        assert _bits(cov["cov_diag"][0], za["cov_u"])
        Md, Mk = LC.factor_product(cov["L"][0])
        R = SC.span_reference(Md, Mk, jac["jac_com"][0], jac["jac_pos"][0], [(0, N - 1), (2, 9)])
        for key, ref, T in (("span_com_displacement_cov", R["com"], R["T_com"]), ("span_positions_displacement_cov", R["pos"], R["T_pos"])):
            err = SC.span_error(za[key], ref, T)
            _note(f"estimate_kinematics #{k}", f"{key} error", err, R["tol"])
            assert err <= R["tol"], (k, key, err, R["tol"])
        ratio = np.diagonal(za["span_com_displacement_cov"], axis1=1, axis2=2) / np.diagonal(R["T_com"], axis1=1, axis2=2)
        _note(f"estimate_kinematics #{k}", "largest var(displacement) / independent sum", float(ratio.max()), np.inf)
    with pytest.raises(ValueError, match="does not satisfy"):                          # before any solve: nothing is written
        E.estimate_kinematics(_init(E, roots["unc"], specs[1][0]), solver_output=False, uncertainty=True, uncertainty_spans=[(0, 17)])
    assert not os.path.exists(os.path.join(roots["unc"], specs[1][0], "fte_kinematic"))


KW = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True)


def test_estimate_kinetics_writes_spans(tmp_path):
    """estimate_kinetics at N = 16 with uncertainty_spans=True: the fields, byte-equal inside estimate_kinetics_batch"""
    sys.path.insert(0, os.path.dirname(__file__))
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    N, sets = 16, []
    for k, seed in enumerate((5, 7)):
        root = str(tmp_path / f"set{k}")
        info = write_dataset(root, data_path=f"2019_03_07/synth/run{k}", N=N, noise_px=0.5, gallop=True, seed=seed, n_cams=6)
        assert E.estimate_kinematics(_init(E, root, info["data_path"]), solver_output=False) is True
        sets.append((root, info["data_path"]))

    def fresh(prefix):
        out = []
        for root, dp in sets:
            shutil.copytree(os.path.join(root, dp, "fte_kinematic"), os.path.join(prefix, dp, "fte_kinematic"))
            out.append(E.init_trajectory(root, dp, "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True, bound_eom_error=(-2.0, 2.0),
                                         include_camera_constraints=True, kinematic_model=False))
        return out
    P = lambda name: str(tmp_path / ("out_" + name))
    single, batch = fresh(P("single")), fresh(P("batch"))
    assert E.estimate_kinetics(single[0], uncertainty=True, uncertainty_spans=True, out_dir_prefix=P("single"), **KW) is True
    assert E.estimate_kinetics_batch(batch, uncertainty=True, uncertainty_spans=True, out_dir_prefix=P("batch"), **KW) == [True, True]
    za = np.load(os.path.join(P("single"), sets[0][1], "fte_kinetic", "uncertainty.npz"))
    zb = np.load(os.path.join(P("batch"), sets[0][1], "fte_kinetic", "uncertainty.npz"))
    shapes = _span_shapes(E, 1)
    assert set(shapes) <= set(za.files) and sorted(za.files) == sorted(zb.files) and "_spans" not in za.files
    for key in za.files:
        assert _bits(za[key], zb[key]), key
    for key, shp in shapes.items():
        assert za[key].shape == shp, key
    assert np.array_equal(za["span_frames"], [[0, N - 1]]) and za["span_seconds"][0] == (N - 1) / single[0].scene.fps
    assert np.all(za["span_com_displacement_std"] > 0.0) and za["span_mean_speed_std"][0] > 0.0
    assert _bits(za["span_mean_speed"], za["span_distance"] / za["span_seconds"])


def test_zz_report():
    """every measured error next to the tolerance applied to it (inf = reported, not asserted)"""
    for label, measure, value, tol in REPORT:
        print(f"{label:40s} {measure:48s} {value:.3e}   tolerance {tol:.3e}")
    worst = {}
    for label, measure, value, tol in REPORT:
        if np.isfinite(tol):
            key = label.split(" #")[0].split(" N ")[0] + " | " + measure
            if key not in worst or value / tol > worst[key][0] / worst[key][1]:
                worst[key] = (value, tol, label)
    for key, (value, tol, label) in sorted(worst.items()):
        print(f"worst {key}: {value:.2e} of {tol:.2e} ({label})")
