"""Posterior covariance of the physics-based estimate on the GPU (cpe_covariance_kinetic, include/cpe.h): the covariance of the coordinates on the
band and of every node's free forces (k_force_cov), against the numpy references of tests/kinetic_cov_compare.py.

Error unit: |difference| / sqrt(C_aa C_bb) of the reference, worst entry.  Two tolerances, both made of reference numbers only:
  kernel     per node, 10 x max(r, 2^-52 x scaled condition of H_ff), r = the difference between the solve-based and the Cholesky-based numpy
             evaluation of cov_f = M^-1 + S W S^T from the HIP path's OWN H_fu / H_ff / meta and the call's OWN Sigma -- isolates k_force_cov
  full path  10 x max(r, 2^-52 x scaled condition of the joint matrix), r = joint route against local route on the oracle's system
             (kinetic_cov_compare.reference)
The kernel tolerance is the issue's rule and its margin is thin: the kernel sums the 84 terms of Y W Y^T in sequence where BLAS sums in blocks, and
lands at 5 - 8 x r under the 10 x rule.  r is a property of the numpy build as well (BLAS blocking, FMA contraction): a failure here after a change of
either side by a factor below two is that margin, not a wrong kernel -- compare the error with the full-path tolerance before suspecting the kernel.
test_zz_report prints every measured value next to its tolerance.  Cases: kinetic_cov_compare.gallop_case (12 frames, computed once per session).

Measured on an MI355X (test_zz_report; the table is in DESIGN.md 4), error / tolerance: kernel 1.5e-10 / 1.8e-10 (2 cameras), 2.4e-10 / 5.3e-10 (a node
in flight), 1.1e-12 / 2.3e-12 (prescribed forces), 1.7e-11 / 7.3e-11 (binding torque boxes); full path Sigma 3.5e-9 and cov_f 1.0e-9 / 2.0e-5 (2 cameras, ridge 0), Sigma 1.1e-9 / 9.5e-7 (ridge
1e-6), 7.8e-9 and 7.1e-10 / 5.7e-6 and 9.9e-10 / 4.1e-6 (6 cameras); cov_pos 0.10 of its tolerance; cov_f(0) - cov_f(1e-3) has no negative eigenvalue."""
import os

import numpy as np
import pytest

import cov_compare as CC
import kinetic_cov_compare as KV
from cheetah_pose_estimation_amd import abi

pytestmark = pytest.mark.gpu

REPORT = []
KEYS = ("cov_diag", "cov_off", "cov_pos", "cov_f", "f", "meta", "L")
_RUNS = {}


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _var(c):
    return {k: v[None] for k, v in c["var"].items()}


def _run(oracle, factory, name, ridge):
    """(case, handle, the call's outputs for the case alone) -- one call per (case, ridge) and session"""
    c = KV.gallop_case(oracle, name)
    h = factory(c["sk"], c["cams"], c["opts"])
    if (name, ridge) not in _RUNS:
        out = h.covariance_kinetic_host(c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], c["ko"], ridge, want_L=True, **_var(c))
        assert out["status"] == abi.OK and out["seq_status"] == [abi.OK], (name, ridge)
        _RUNS[(name, ridge)] = out
    return c, h, _RUNS[(name, ridge)]


def _window_cov(diag, off, n):
    """W [84][84] of node n from the band the call returned: frames (n, n-1, n-2); off[f][k-1] = Sigma(f + k, f)"""
    W = np.zeros((84, 84))
    for a in range(3):
        for b in range(3):
            if a == b:
                blk = diag[n - a]
            elif a < b:
                blk = off[n - b, b - a - 1]                    # Sigma(n - a, n - b): rows in the later frame
            else:
                blk = off[n - a, a - b - 1].T
            W[28 * a:28 * a + 28, 28 * b:28 * b + 28] = blk
    return W


def _kernel_check(label, h, c, out):
    """cov_f of every node against the local formula from the HIP path's own pieces; returns (the counts na seen, the largest tolerance used)"""
    G = h.eval_kinetic_system_host(c["ko"], c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], band=False, **_var(c))
    nodes = KV.node_blocks({k: G[k][0] for k in ("Hfu", "Hff", "meta")})
    worst, tol_max, seen = (0.0, 1.0), 0.0, set()
    for n, (Hfu, M) in nodes.items():
        na = M.shape[0]
        seen.add(na)
        ref, tol, r, cond = KV.kernel_tolerance(Hfu, M, _window_cov(out["cov_diag"][0], out["cov_off"][0], n))
        err = KV.scaled_difference(out["cov_f"][0, n, :na, :na], ref)
        if err / tol >= worst[0] / worst[1]:
            worst = (err, tol)
        tol_max = max(tol_max, tol)
        assert err <= tol, (label, n, na, err, tol, r, cond)
    _note(label, "kernel error", *worst)
    return seen, tol_max


# ---- 1. the kernel, tightly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "flight", "boxed"])
def test_force_covariance_against_the_local_formula(oracle, gpu_handle_factory, name):
    """every node; "boxed": the tau_box variant (the boxes of the module-level estimate_grf)"""
    c, h, out = _run(oracle, gpu_handle_factory, name, 0.0)
    seen, _ = _kernel_check(f"kernel {name}", h, c, out)
    assert seen == ({48, 51, 54} if name == "flight" else {51, 54})


# ---- 2. the full path against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("name", ["base", "six"])
def test_full_path_against_the_oracle(oracle, gpu_handle_factory, name, ridge):
    """Sigma (ridge 0 and 1e-6) and cov_f (ridge 0) against the joint route built from oracle.kinetic_system(lam = ridge)"""
    c, h, out = _run(oracle, gpu_handle_factory, name, ridge)
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, ridge)
    ref = KV.reference(Ad, Hk, nodes)
    assert np.array_equal(out["meta"][0][:, 0], R["meta"][:, 0])
    eu = CC.scaled_error(out["cov_diag"][0], out["cov_off"][0], ref["diag"], ref["off"])
    _note(f"full path {name} ridge {ridge:g}", "Sigma error", eu, ref["tol"])
    ef = None
    if ridge == 0.0:
        ef = KV.force_error(out["cov_f"][0], ref["cov_f"])
        _note(f"full path {name} ridge {ridge:g}", "cov_f error", ef, ref["tol"])
    assert eu <= ref["tol"], (eu, ref["tol"])
    assert ef is None or ef <= ref["tol"], (ef, ref["tol"])


# ---- 3. structure ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "flight", "fixed"])
def test_structure(oracle, gpu_handle_factory, name):
    c, h, out = _run(oracle, gpu_handle_factory, name, 0.0)
    diag, off = h.band_inverse_host(out["L"])
    assert _bits(diag, out["cov_diag"]) and _bits(off, out["cov_off"])
    cf, meta = out["cov_f"][0], out["meta"][0]
    assert _bits(cf, np.swapaxes(cf, 1, 2))
    assert not cf[:2].any() and not out["f"][0][:2].any() and not meta[:2].any()
    G = h.eval_kinetic_system_host(c["ko"], c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], band=False, **_var(c))
    assert _bits(out["f"][0], G["f"][0])
    _, tol = _kernel_check(f"structure {name}", h, c, out)
    for n in range(2, cf.shape[0]):
        na = meta[n, 0]
        assert na == G["meta"][0][n, 0] and np.array_equal(meta[n, 1:1 + na], G["meta"][0][n, 1:1 + na]) and meta[n, 64] == G["meta"][0][n, 64]
        assert not meta[n, 1 + na:64].any()
        assert not cf[n, na:].any() and not cf[n, :, na:].any()
        C = cf[n, :na, :na]
        s = 1.0 / np.sqrt(np.diag(C))
        assert np.all(np.isfinite(s))
        assert np.linalg.eigvalsh(C * s[:, None] * s[None, :])[0] >= -tol
    assert not CC.structure_failures(out["cov_diag"][0], out["cov_off"][0], 1e-6)


# ---- 4. marker covariance ------------------------------------------------------------------------------------------------------------------------
def test_marker_covariance(oracle, gpu_handle_factory):
    """cov_pos against P Sigma_gpu P^T, P by central differences (steps 1e-5 and 1e-6; tolerance 10 x their difference per marker block), as the
    kinematic test"""
    c, h, out = _run(oracle, gpu_handle_factory, "base", 0.0)
    cp, N = out["cov_pos"][0], c["q"].shape[0]
    assert _bits(cp, np.swapaxes(cp, 2, 3))
    r5 = CC.marker_covariance(CC.marker_jacobians(oracle, c["sk"], c["q"], range(N), 1e-5), out["cov_diag"][0])
    r6 = CC.marker_covariance(CC.marker_jacobians(oracle, c["sk"], c["q"], range(N), 1e-6), out["cov_diag"][0])
    tol = 10.0 * np.abs(r5 - r6).max(axis=(2, 3))
    err = np.abs(cp - r5).max(axis=(2, 3))
    _note("marker covariance", "worst error / tolerance", float((err / tol).max()), 1.0)
    assert np.all(tol > 0.0) and np.all(err <= tol)


# ---- 5. edge lengths -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3])
def test_edge_lengths(oracle, gpu_handle_factory, N):
    """N = 2: no node -- cov_f zero, Sigma finite; N = 3: one node, whose window starts at the sequence's first frame.  (Three frames carry no
    smoothing term against which every coordinate is determined, so the damping is 1e-3 as in the kinematic test of short sequences.)"""
    c, h, _ = _run(oracle, gpu_handle_factory, "base", 0.0)
    cut = lambda a: np.ascontiguousarray(a[:N])[None]
    out = h.covariance_kinetic_host(cut(c["q"]), cut(c["meas"]), cut(c["weight"]), cut(c["stance"]), c["ko"], 1e-3, want_L=True)
    assert out["seq_status"] == [abi.OK]
    assert np.all(np.isfinite(out["cov_diag"])) and np.all(np.diagonal(out["cov_diag"][0], axis1=1, axis2=2) > 0.0)
    assert not out["cov_f"][0][:2].any()
    if N == 2:
        # at ridge 0 two frames have coordinates with exactly zero curvature (tests/test_kinetic_covariance_host.py): an exactly zero pivot
        o0 = h.covariance_kinetic_host(cut(c["q"]), cut(c["meas"]), cut(c["weight"]), cut(c["stance"]), c["ko"], 0.0, want_L=True)
        assert o0["seq_status"] == [abi.NUMERICAL] and not any(o0[k].any() for k in KEYS)
    if N == 3:
        na = out["meta"][0][2, 0]
        assert na in (51, 54)
        C = out["cov_f"][0][2]
        assert np.all(np.diag(C)[:na] > 0.0) and _bits(C, C.T) and not C[na:].any()
        diag, off = h.band_inverse_host(out["L"])
        assert _bits(diag, out["cov_diag"]) and _bits(off, out["cov_off"])


# ---- 6. batch ------------------------------------------------------------------------------------------------------------------------------------
def test_batch_rules(oracle, gpu_handle_factory):
    """B = 3 (three seeds): every sequence bit-equal to its own call; a repeated call bit-equal"""
    names = ("base", "seed7", "seed11")
    cs = [KV.gallop_case(oracle, n) for n in names]
    h = gpu_handle_factory(cs[0]["sk"], cs[0]["cams"], cs[0]["opts"])
    st = lambda k: np.stack([c[k] for c in cs])
    a = h.covariance_kinetic_host(st("q"), st("meas"), st("weight"), st("stance"), cs[0]["ko"], 0.0, want_L=True)
    b = h.covariance_kinetic_host(st("q"), st("meas"), st("weight"), st("stance"), cs[0]["ko"], 0.0, want_L=True)
    assert a["seq_status"] == [abi.OK] * 3
    assert all(_bits(a[k], b[k]) for k in KEYS)
    assert not _bits(a["cov_f"][0], a["cov_f"][1])
    for s, name in enumerate(names):
        one = _run(oracle, gpu_handle_factory, name, 0.0)[2]
        assert all(_bits(one[k][0], a[k][s]) for k in KEYS), name
    # the device-pointer entry gives the host-pointer twin's bits
    import torch
    dev = torch.device("cuda", 0)
    T = lambda x, dt=torch.float64: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    o = {k: torch.zeros(a[k].shape, dtype=torch.int32 if k == "meta" else torch.float64, device=dev) for k in KEYS}
    st_, seq = h.covariance_kinetic(cs[0]["ko"], T(st("q")), T(st("meas")), T(st("weight")), T(st("stance"), torch.int32), 0.0, **o)
    h.synchronize()
    assert st_ == abi.OK and seq == [abi.OK] * 3
    assert all(_bits(o[k].cpu().numpy(), a[k]) for k in KEYS)


# ---- 7. a sequence without a factor --------------------------------------------------------------------------------------------------------------
def test_numerical_status(oracle, gpu_handle_factory):
    """next to a good sequence: one no camera sees (every weight zero: the band is singular, tests/test_kinetic_covariance_host.py -- the pivot that
    fails is round-off, no input of three frames or more has an exactly zero one) and one whose evaluation is not finite (a NaN measurement with a
    positive weight, which does not depend on rounding): [CPE_NUMERICAL, CPE_NUMERICAL, CPE_OK], their outputs zero, the neighbour's bits those of
    its own call.  A handle of half-bandwidth 4 is refused."""
    c, h, alone = _run(oracle, gpu_handle_factory, "base", 0.0)
    three = lambda a: np.stack([a, a, a])
    w, me = three(c["weight"]), three(c["meas"])
    w[0] = 0.0
    l = int(np.argmax(w[1, 5, 0] > 0.0))
    me[1, 5, 0, l, 0] = np.nan
    r = h.covariance_kinetic_host(three(c["q"]), me, w, three(c["stance"]), c["ko"], 0.0, want_L=True)
    assert r["seq_status"] == [abi.NUMERICAL, abi.NUMERICAL, abi.OK] and r["status"] == abi.NUMERICAL
    assert not any(r[k][b].any() for k in KEYS for b in (0, 1))
    assert all(_bits(alone[k][0], r[k][2]) for k in KEYS)
    from cheetah_pose_estimation_amd import _lib, priors, skeleton
    h4 = gpu_handle_factory(skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24)), c["cams"], c["opts"], priors.load_priors())
    assert h4.pb == 4
    with pytest.raises(_lib.CpeError, match="half-bandwidth 4"):
        h4.covariance_kinetic_host(c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], c["ko"], 0.0)


# ---- 8. prescribed foot forces -------------------------------------------------------------------------------------------------------------------
def test_prescribed_forces(oracle, gpu_handle_factory):
    c, h, out = _run(oracle, gpu_handle_factory, "fixed", 0.0)
    nm, nc = c["ko"].dyn.n_motors, 26
    meta = out["meta"][0]
    assert np.all(meta[2:, 0] == nm + nc) and np.all(meta[2:, 1:1 + nm + nc] == np.arange(nm + nc))       # no foot rows
    seen, _ = _kernel_check("kernel fixed", h, c, out)
    assert seen == {48}
    free = _run(oracle, gpu_handle_factory, "base", 0.0)[2]
    assert not _bits(free["cov_f"][0][:, :48, :48], out["cov_f"][0][:, :48, :48])


# ---- 9. monotonic in the damping -----------------------------------------------------------------------------------------------------------------
def test_damping_lowers_the_force_covariance(oracle, gpu_handle_factory):
    c, h, o0 = _run(oracle, gpu_handle_factory, "base", 0.0)
    o1 = _run(oracle, gpu_handle_factory, "base", 1e-3)[2]
    _, tol = _kernel_check("kernel base (ridge 0)", h, c, o0)
    worst = 0.0
    for n in range(2, c["q"].shape[0]):
        na = o0["meta"][0][n, 0]
        assert na == o1["meta"][0][n, 0]
        worst = min(worst, KV.psd_gap(o0["cov_f"][0][n, :na, :na], o1["cov_f"][0][n, :na, :na]))
        assert np.all(np.diag(o1["cov_f"][0][n])[:na] < np.diag(o0["cov_f"][0][n])[:na])
    _note("monotonic", "most negative scaled eigenvalue of cov_f(0) - cov_f(1e-3)", -worst, tol)
    assert worst >= -tol


# ---- 10. the estimator, through files ------------------------------------------------------------------------------------------------------------
def test_estimator_writes_force_uncertainty(tmp_path):
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    N = 24
    ests, dirs = {}, {}
    for key in ("plain", "unc"):
        root = str(tmp_path / key)
        info = write_dataset(root, N=N, noise_px=0.5, gallop=True)
        est = E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
        assert E.estimate_kinematics(est, solver_output=False) is True
        ests[key] = E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True,
                                      bound_eom_error=(-2.0, 2.0), include_camera_constraints=True, kinematic_model=False)
        dirs[key] = os.path.join(root, info["data_path"], "fte_kinetic")
    kw = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True)
    assert E.estimate_kinetics(ests["plain"], **kw) is True
    assert E.estimate_kinetics(ests["unc"], uncertainty=True, **kw) is True
    assert ests["plain"].uncertainty is None and not os.path.exists(os.path.join(dirs["plain"], "uncertainty.npz"))
    fa, fb = E.load_result_pickle(os.path.join(dirs["plain"], "fte.pickle")), E.load_result_pickle(os.path.join(dirs["unc"], "fte.pickle"))
    assert fa.keys() == fb.keys()
    for key in fa:
        if isinstance(fa[key], np.ndarray):
            assert _bits(fa[key], fb[key]), key
        elif key == "tau":
            assert all(_bits(fa[key][m], fb[key][m]) for m in fa[key])
    assert sorted(f for f in os.listdir(dirs["unc"]) if f != "uncertainty.npz") == sorted(os.listdir(dirs["plain"]))
    z = np.load(os.path.join(dirs["unc"], "uncertainty.npz"))
    shapes = dict(cov_u=(N, 28, 28), u_std=(N, 28), positions_cov=(N, 24, 3, 3), positions_std=(N, 24, 3), ridge=(), tau_std=(N, 22),
                  lambda_std=(N, 26), grf_std=(N, 4, 3), tau_cov=(N, 22, 22))
    assert sorted(z.files) == sorted(shapes)
    for key, shp in shapes.items():
        assert z[key].shape == shp, key
        assert _bits(z[key], np.asarray(ests["unc"].uncertainty[key])), key
    assert np.all(z["tau_std"][2:] > 0.0) and np.all(z["lambda_std"][2:] > 0.0) and not z["tau_std"][:2].any()
    stance = ests["unc"].kinetic["stance"]
    assert np.array_equal(np.all(z["grf_std"] > 0.0, axis=-1)[2:], stance[2:] == 1) and np.array_equal(np.any(z["grf_std"] > 0.0, axis=-1)[2:], stance[2:] == 1)
    assert np.all(z["u_std"] > 0.0) and float(z["ridge"]) == 0.0
    # the module-level estimate_grf (torque boxes around the stored torques): same fields beside fte_grf/fte.pickle when the solve is ok
    import dataclasses
    est3 = E.init_trajectory(str(tmp_path / "unc"), info["data_path"], "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True,
                             bound_eom_error=(-2.0, 2.0), include_camera_constraints=True, kinematic_model=False)
    est3.params = dataclasses.replace(est3.params, kinetic_dataset=True)             # (only the flag is the kinetic set's, as tests/test_gpu_kinetic.py)
    ok3 = E.estimate_grf(est3, solver_output=False, uncertainty=True)
    npz = os.path.join(str(tmp_path / "unc"), info["data_path"], "fte_grf", "uncertainty.npz")
    assert os.path.exists(npz) == bool(ok3) and (est3.uncertainty is not None) == bool(ok3)
    print(f"estimate_grf(uncertainty=True): ok {ok3}")
    if ok3:
        z3 = np.load(npz)
        assert sorted(z3.files) == sorted(shapes) and all(z3[k].shape == shp for k, shp in shapes.items())
        assert np.all(z3["tau_std"][2:] > 0.0) and _bits(z3["tau_cov"], est3.uncertainty["tau_cov"])
    with pytest.raises(NotImplementedError, match="use_2d_reprojections"):
        E.estimate_kinetics(ests["unc"], uncertainty=True, use_2d_reprojections=False, **kw)


def test_zz_report():
    """every measured error next to the tolerance applied to it"""
    for label, measure, value, tol in REPORT:
        print(f"{label:40s} {measure:60s} {value:.3e}   tolerance {tol:.3e}")
