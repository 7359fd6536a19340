"""Posterior covariance of the kinematic estimate on the GPU (cpe_band_inverse, cpe_covariance, include/cpe.h) against the numpy references of
tests/cov_compare.py: the selected-inversion sweep on the oracle's matrices and on random block bands, the full path from q through the solver's
own factor, the marker covariance, the batch rules, the sequences without a factor and the estimator through files.

Error unit: |difference| / sqrt(Sigma_aa Sigma_bb) of the reference, worst over the band; residual: entries of sum_k A(n,k) Sigma(k,n) - I over
sqrt(A_aa Sigma_bb).  Tolerance per matrix: 10 x max(r, 2^-52 x Jacobi-scaled condition number), r = the discrepancy between the helper's two
float64 routes on that matrix (cov_compare.reference) -- measured on the reference, never on the GPU.  test_zz_report prints every measured value
next to its tolerance."""
import os
import sys

import numpy as np
import pytest

import cov_compare as CC
import lm_compare as LC
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

REPORT = []                                      # (label, measure, value, tolerance)
RIDGE = 1e-6


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _pb_handle(factory, PB):
    """a handle of half-bandwidth PB (cpe_band_inverse reads nothing else of it)"""
    if PB == 3:
        return factory(skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options())
    return factory(skeleton.build_skeleton("phantom", 24), synth.make_cameras(2), abi.default_options(), priors.load_priors())


def _check_band(label, Ad, Hk, diag, off, R):
    err, res = CC.scaled_error(diag, off, R["diag"], R["off"]), CC.residual(Ad, Hk, diag, off)
    _note(label, "error", err, R["tol_err"])
    _note(label, "residual", res, R["tol_res"])
    bad = CC.structure_failures(diag, off, R["tol_err"])
    assert not bad, (label, bad)
    assert err <= R["tol_err"], (label, err, R["tol_err"])
    assert res <= R["tol_res"], (label, res, R["tol_res"])


# ---- 1. the sweep against the oracle's matrix and random bands, same input on both sides ------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, RIDGE])
@pytest.mark.parametrize("name", ["six", "two", "mono"])
def test_sweep_on_the_oracles_band(oracle, gpu_handle_factory, name, ridge):
    c = CC.oracle_case(oracle, name)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    assert h.pb == c["PB"] == (4 if name == "mono" else 3)
    Ad = CC.damped(c["Bk"], ridge)
    R = CC.reference(Ad, c["Hk"])
    L = CC.cholesky_layout(Ad, c["Hk"])
    diag, off = h.band_inverse_host(L[None])
    _note(f"{name} ridge {ridge:g}", "scaled condition", R["cond"], np.inf)
    _check_band(f"sweep {name} ridge {ridge:g}", Ad, c["Hk"], diag[0], off[0], R)


@pytest.mark.parametrize("PB", [3, 4])
@pytest.mark.parametrize("N", ["1", "2", "PB", "PB+1", "57", "200"])
def test_sweep_on_random_bands(gpu_handle_factory, PB, N):
    """random SPD block bands, two per call (more than one workgroup); the sequence lengths below, at and one past the window and two that wrap
    the ring many times"""
    N = {"PB": PB, "PB+1": PB + 1}.get(N) or int(N)
    h = _pb_handle(gpu_handle_factory, PB)
    assert h.pb == PB
    bands = [CC.random_band(N, PB, 1000 * PB + 10 * N + b) for b in range(2)]
    L = np.stack([CC.cholesky_layout(Ad, Hk) for Ad, Hk in bands])
    diag, off = h.band_inverse_host(L)
    for b, (Ad, Hk) in enumerate(bands[:1 if N == 200 else 2]):          # (one reference at 5 600 unknowns: seconds each)
        _check_band(f"random PB {PB} N {N} #{b}", Ad, Hk, diag[b], off[b], CC.reference(Ad, Hk))
    d2, o2 = h.band_inverse_host(L[::-1].copy())                          # the other order in the batch, and a second run: same bits
    assert _bits(d2[::-1], diag) and _bits(o2[::-1], off)


# ---- 2. the full path: q -> the solver's own factor -> Sigma ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six", "two", "mono"])
def test_full_path_chain(oracle, gpu_handle_factory, name):
    """L of cpe_covariance is bit-equal to cpe_eval_lm_step's at lam = ridge; Sigma is bit-equal to cpe_band_inverse of that L; L L^T against the
    oracle's band passes lm_compare's `factor` key at its existing tolerance.  This chain is the oracle comparison (a direct comparison of Sigma
    with the inverse of the oracle's band is ill-posed at round-off)."""
    c = CC.oracle_case(oracle, name)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    q, me, we = c["q"][None], c["meas"][None], c["weight"][None]
    out = h.covariance_host(q, me, we, RIDGE, want_L=True)
    assert out["status"] == abi.OK and out["seq_status"] == [abi.OK]
    G = h.eval_lm_step_host(q, me, we, RIDGE)
    assert G["seq"][0, 7] == abi.OK
    assert _bits(out["L"], G["L"])
    diag, off = h.band_inverse_host(out["L"])
    assert _bits(diag, out["cov_diag"]) and _bits(off, out["cov_off"])
    Rlm = LC.reference(oracle, c["sk"], c["cams"], c["opts"], c["priors"], c["q"], c["meas"], c["weight"], RIDGE, h.pb)
    d = LC.discrepancies({k: v[0] for k, v in G.items()}, Rlm, LC.coordinate_slots(c["sk"]))
    _note(f"full path {name}", "factor", d["factor"], LC.TOL["factor"])
    assert not LC.failures(d, only=("factor",)), d["factor"]
    bad = CC.structure_failures(out["cov_diag"][0], out["cov_off"][0], 1e-6)
    assert not bad, bad
    # ridge 0 (a damping cpe_eval_lm_step does not take): the same internal consistency
    o0 = h.covariance_host(q, me, we, 0.0, want_L=True)
    assert o0["seq_status"] == [abi.OK]
    d0, f0 = h.band_inverse_host(o0["L"])
    assert _bits(d0, o0["cov_diag"]) and _bits(f0, o0["cov_off"])
    assert not _bits(o0["cov_diag"], out["cov_diag"])


def test_full_path_direct_bound_six_cameras(oracle, gpu_handle_factory):
    """the one direct assertion: with E = L L^T - A_oracle, |Sigma_gpu - Sigma_oracle| <= 2 |Sigma_o| |E| |Sigma_o| entrywise plus the tolerance of
    the sweep, under the condition ||Sigma_o E||_2 < 0.1 (asserted: without it the first-order bound means nothing)"""
    c = CC.oracle_case(oracle, "six")
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    out = h.covariance_host(c["q"][None], c["meas"][None], c["weight"][None], RIDGE, want_L=True)
    assert out["seq_status"] == [abi.OK]
    Ad = CC.damped(c["Bk"], RIDGE)
    R = CC.reference(Ad, c["Hk"], want_dense=True)
    Md, Mk = LC.factor_product(out["L"][0])
    E = LC.dense(Md - Ad, Mk - c["Hk"])
    So = R["S"]
    cond1 = float(np.linalg.norm(So @ E, 2))
    _note("direct six", "||Sigma_o E||_2", cond1, 0.1)
    sa = np.sqrt(np.diag(LC.dense(Ad, c["Hk"])))
    _note("direct six", "|E| / sqrt(A_aa A_bb)", float((np.abs(E) / (sa[:, None] * sa[None, :])).max()), np.inf)
    assert cond1 < 0.1
    ss = np.sqrt(np.diag(So))
    bound = 2.0 * (np.abs(So) @ np.abs(E) @ np.abs(So)) + R["tol_err"] * ss[:, None] * ss[None, :]
    bd, bo = CC.cut_band(bound, h.pb)
    dd, do = np.abs(out["cov_diag"][0] - R["diag"]), np.abs(out["cov_off"][0] - R["off"])
    _note("direct six", "error", CC.scaled_error(out["cov_diag"][0], out["cov_off"][0], R["diag"], R["off"]), np.inf)
    _note("direct six", "worst |difference| / bound", max(float((dd / bd).max()), float((do[bo > 0] / bo[bo > 0]).max())), 1.0)
    assert np.all(dd <= bd) and np.all(do <= bo)


# ---- 3. marker covariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six", "mono"])
def test_marker_covariance(oracle, gpu_handle_factory, name):
    """cov_pos against P Sigma_gpu P^T, P by central differences (steps 1e-5 and 1e-6; tolerance 10 x their difference, per marker block);
    symmetric bit for bit and PSD to round-off"""
    c = CC.oracle_case(oracle, name)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    out = h.covariance_host(c["q"][None], c["meas"][None], c["weight"][None], 0.0)
    assert out["seq_status"] == [abi.OK]
    cp, N = out["cov_pos"][0], c["q"].shape[0]
    assert _bits(cp, np.swapaxes(cp, 2, 3))
    frames = range(N)
    r5 = CC.marker_covariance(CC.marker_jacobians(oracle, c["sk"], c["q"], frames, 1e-5), out["cov_diag"][0])
    r6 = CC.marker_covariance(CC.marker_jacobians(oracle, c["sk"], c["q"], frames, 1e-6), out["cov_diag"][0])
    tol = 10.0 * np.abs(r5 - r6).max(axis=(2, 3))                      # [N, L]
    err = np.abs(cp - r5).max(axis=(2, 3))
    scale = np.abs(r5).max(axis=(2, 3))
    _note(f"marker covariance {name}", "worst error / block scale", float((err / scale).max()), float((tol / scale).max()))
    _note(f"marker covariance {name}", "worst error / tolerance", float((err / tol).max()), 1.0)
    assert np.all(tol > 0.0) and np.all(err <= tol)
    ev = np.linalg.eigvalsh(cp)
    assert np.all(ev[..., 0] >= -tol) and np.all(ev[..., 2] > 0.0)
    if name == "mono":
        # what the feature is for: one camera determines depth worst.  positions_std on the world axis of the line of sight to the marker exceeds
        # both other components, mid-sequence, for every marker (cov_compare.depth_exceeds_transverse; true of the reference too, tested on the CPU)
        std = np.sqrt(np.diagonal(cp, axis1=2, axis2=3))
        pos = synth.fk_numpy(c["sk"], c["q"])[0]
        assert np.all(CC.depth_exceeds_transverse(c["cams"][0], pos[N // 2], std[N // 2]))
        _note("mono", "largest positions_std mid-sequence (m)", float(std[N // 2].max()), np.inf)


# ---- 4. batch rules ---------------------------------------------------------------------------------------------------------------------
COV_KEYS = ("cov_diag", "cov_off", "cov_pos", "L")
ANIMALS = (("phantom", False), ("jules", False), ("arabia-02", True), ("shiraz-02", True))


def test_batch_rules(gpu_handle_factory):
    """a sequence alone, inside a B = 5 batch and inside a ragged batch of mixed skeletons, rigs and lengths: bit-equal outputs; two runs bit-equal;
    zeros past a sequence's frames"""
    sk, cams, opts = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options()
    h = gpu_handle_factory(sk, cams, opts)
    d = synth.make_batch(sk, cams, B=5, N=23, seed=90)
    q, me, we = d["q_true"], d["meas"], d["weight"]
    a = h.covariance_host(q, me, we, RIDGE, want_L=True)
    b = h.covariance_host(q, me, we, RIDGE, want_L=True)
    assert a["seq_status"] == [abi.OK] * 5
    assert all(_bits(a[k], b[k]) for k in COV_KEYS)
    for s in (0, 3):
        one = h.covariance_host(q[s:s + 1], me[s:s + 1], we[s:s + 1], RIDGE, want_L=True)
        assert all(_bits(one[k][0], a[k][s]) for k in COV_KEYS), s
    models = []
    for k, (animal, kin) in enumerate(ANIMALS):
        models.append((skeleton.build_skeleton(animal, 24, kinetic_dataset=kin), synth.make_cameras(4 if kin else 6, seed=100 + k),
                       abi.default_options(200.0 if kin else 120.0), kin))
    seqs = []
    for s, N in enumerate([30, 36, 5, 44, 4, 33]):
        m = s % len(models)
        skm, cm, om, kin = models[m]
        dd = synth.make_batch(skm, cm, B=1, N=N, fps=1.0 / om.h, seed=140 + s, kinetic_dataset=kin)
        seqs.append((m, dd["q_true"][0], dd["meas"][0], dd["weight"][0]))
    hm = _lib.Handle.multi([m[0] for m in models], [m[1] for m in models], [m[2] for m in models])
    try:
        r = hm.covariance_ragged_host([s[1] for s in seqs], [s[2] for s in seqs], [s[3] for s in seqs], [s[0] for s in seqs], RIDGE, want_L=True)
        r2 = hm.covariance_ragged_host([s[1] for s in seqs], [s[2] for s in seqs], [s[3] for s in seqs], [s[0] for s in seqs], RIDGE, want_L=True)
    finally:
        hm.close()
    assert r["seq_status"] == [abi.OK] * len(seqs)
    for k in COV_KEYS:
        assert _bits(r["padded"][k], r2["padded"][k]), k
    for s, (m, qs, ms, ws) in enumerate(seqs):
        hs = gpu_handle_factory(models[m][0], models[m][1], models[m][2])
        one = hs.covariance_host(qs[None], ms[None], ws[None], RIDGE, want_L=True)
        for k in COV_KEYS:
            assert _bits(one[k][0], r[k][s]), (s, k)
            assert not r["padded"][k][s, qs.shape[0]:].any(), (s, k)


# ---- 5. sequences whose matrix has no Cholesky factor -------------------------------------------------------------------------------------
def test_numerical_status(oracle, gpu_handle_factory):
    """one camera without priors, and three frames at ridge 0 (zero diagonal entries: no motion term): CPE_NUMERICAL, every output zero, the batch
    neighbour unaffected; the three-frame case succeeds at ridge 1e-3"""
    c = CC.oracle_case(oracle, "mono_noprior")
    six = CC.oracle_case(oracle, "six")
    sk = c["sk"]
    d = synth.make_batch(sk, six["cams"], B=1, N=CC.N_CASE, seed=17)
    hm = _lib.Handle.multi([sk, sk], [c["cams"], six["cams"]], [c["opts"], c["opts"]])
    try:
        r = hm.covariance_ragged_host([c["q"], d["q_true"][0]], [c["meas"], d["meas"][0]], [c["weight"], d["weight"][0]], [0, 1], 0.0, want_L=True)
    finally:
        hm.close()
    assert r["seq_status"] == [abi.NUMERICAL, abi.OK] and r["status"] == abi.NUMERICAL
    assert not any(r[k][0].any() for k in COV_KEYS)
    alone = gpu_handle_factory(sk, six["cams"], c["opts"]).covariance_host(d["q_true"], d["meas"], d["weight"], 0.0, want_L=True)
    assert all(_bits(alone[k][0], r[k][1]) for k in COV_KEYS)
    n3 = CC.oracle_case(oracle, "n3")
    h = gpu_handle_factory(n3["sk"], n3["cams"], n3["opts"])
    q = np.stack([n3["q"], six["q"][5:8]]); me = np.stack([n3["meas"], six["meas"][5:8]]); we = np.stack([n3["weight"], six["weight"][5:8]])
    o = h.covariance_host(q, me, we, 0.0, want_L=True)
    assert o["seq_status"] == [abi.NUMERICAL] * 2 and not any(o[k].any() for k in COV_KEYS)
    o = h.covariance_host(q, me, we, 1e-3, want_L=True)
    assert o["seq_status"] == [abi.OK] * 2
    R = CC.reference(CC.damped(n3["Bk"], 1e-3), n3["Hk"])
    assert not CC.structure_failures(o["cov_diag"][0], o["cov_off"][0], R["tol_err"])
    # a three-frame sequence next to a long one in one ragged call: its failure leaves the neighbour's bits alone
    hm = _lib.Handle.multi([n3["sk"]], [n3["cams"]], [n3["opts"]])
    try:
        r = hm.covariance_ragged_host([n3["q"], six["q"]], [n3["meas"], six["meas"]], [n3["weight"], six["weight"]], [0, 0], 0.0)
    finally:
        hm.close()
    assert r["seq_status"] == [abi.NUMERICAL, abi.OK] and not r["cov_diag"][0].any() and not r["cov_pos"][0].any()
    one = h.covariance_host(six["q"][None], six["meas"][None], six["weight"][None], 0.0)
    assert _bits(one["cov_diag"][0], r["cov_diag"][1]) and _bits(one["cov_pos"][0], r["cov_pos"][1])


# ---- 6. the estimator, through files -----------------------------------------------------------------------------------------------------
def _init(E, root, path, **kw):
    return E.init_trajectory(root_dir=root, data_path=path, cheetah_name="phantom", kinetic_dataset=False, solver_path="/unused/ipopt",
                             kinematic_model=True, **kw)


def test_estimator_writes_uncertainty(tmp_path):
    sys.path.insert(0, os.path.dirname(__file__))
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    specs = [("2019_03_07/synth/run1", 24, 5, 6), ("2019_03_09/synth/run2", 30, 6, 4)]
    roots = {k: str(tmp_path / k) for k in ("plain", "single", "ragged")}
    for root in roots.values():
        for path, N, seed, nc in specs:
            write_dataset(root, data_path=path, N=N, seed=seed, n_cams=nc)
    ests = {k: [_init(E, root, p) for p, _, _, _ in specs] for k, root in roots.items()}
    assert all(E.estimate_kinematics(e, solver_output=False) for e in ests["plain"])
    assert all(E.estimate_kinematics(e, solver_output=False, uncertainty=True) for e in ests["single"])
    assert E.estimate_kinematics_batch(ests["ragged"], ragged=True, uncertainty=True, uncertainty_ridge=0.0) == [True, True]
    for k, (path, N, _, _) in enumerate(specs):
        dirs = {r: os.path.join(roots[r], path, "fte_kinematic") for r in roots}
        assert not os.path.exists(os.path.join(dirs["plain"], "uncertainty.npz")) and ests["plain"][k].uncertainty is None
        fa = E.load_result_pickle(os.path.join(dirs["plain"], "fte.pickle"))
        for r in ("single", "ragged"):
            fb = E.load_result_pickle(os.path.join(dirs[r], "fte.pickle"))
            assert fa.keys() == fb.keys()
            for key in fa:
                if isinstance(fa[key], np.ndarray):
                    assert _bits(fa[key], fb[key]), (r, key)
                elif key != "processing_time_s":
                    assert fa[key] == fb[key] or isinstance(fa[key], dict), (r, key)
            assert sorted(f for f in os.listdir(dirs[r]) if f != "uncertainty.npz") == sorted(os.listdir(dirs["plain"]))
        za, zb = np.load(os.path.join(dirs["single"], "uncertainty.npz")), np.load(os.path.join(dirs["ragged"], "uncertainty.npz"))
        shapes = dict(cov_u=(N, 28, 28), u_std=(N, 28), positions_cov=(N, 24, 3, 3), positions_std=(N, 24, 3), ridge=())
        assert sorted(za.files) == sorted(shapes)
        for key, shp in shapes.items():
            assert za[key].shape == shp, key
            assert _bits(za[key], zb[key]), key                             # ragged=True matches the single call bit for bit
            assert _bits(za[key], np.asarray(ests["single"][k].uncertainty[key])), key
        assert np.all(za["u_std"] > 0.0) and np.all(za["positions_std"] > 0.0) and float(za["ridge"]) == 0.0
    with pytest.raises(NotImplementedError, match="shutter"):
        E.estimate_kinematics(_init(E, roots["plain"], specs[0][0], shutter_delay_estimation=True), solver_output=False, uncertainty=True)


def test_zz_report():
    """every measured error next to the tolerance applied to it (inf = reported, not asserted)"""
    for label, measure, value, tol in REPORT:
        print(f"{label:40s} {measure:32s} {value:.3e}   tolerance {tol:.3e}")
    worst = {}
    for label, measure, value, tol in REPORT:
        if measure in ("error", "residual") and np.isfinite(tol):
            key = ("oracle bands" if label.startswith("sweep") else "random bands", measure)
            if key not in worst or value / tol > worst[key][0] / worst[key][1]:
                worst[key] = (value, tol, label)
    for (group, measure), (value, tol, label) in sorted(worst.items()):
        print(f"worst {measure} on {group}: {value:.2e} of {tol:.2e} ({label})")
