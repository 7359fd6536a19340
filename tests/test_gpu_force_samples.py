"""Draws of the node forces of the physics-based estimate on the GPU (cpe_force_samples, k_force_sample; include/cpe.h), against the numpy
references of tests/force_sample_compare.py and kinetic_cov_compare.py.

Error units and tolerances, all made of reference numbers only:
  kernel      per node, |df_a - ref_a| / (sqrt(cov_f_aa) ||(zeta_n, z)||), within 10 x max(r, 2^-52 x scaled condition of M), r = the two numpy
              routes against each other, from the HIP path's OWN H_fu / H_ff / meta and the call's OWN factor L -- isolates k_force_sample
  identity    M_n^-1 from the zeta unit vectors and -S_n from the window unit steps, put together with the W of the band cpe_covariance_kinetic
              returns: against that entry's cov_f in kinetic_cov_compare's unit, within kernel_tolerance's value (ridge 0) or, at ridge 1e-6,
              10 x max(r, 2^-52 x the scaled condition of (sum df df^T)^-1) with r = force_sample_compare.identity_error on the oracle's system
              (the rule and its reason: that helper's docstring)
  joint path  the unit vectors of (z, every node's zeta) through cpe_band_sample + cpe_force_samples: sum_s x_s x_s^T against the inverse of the
              joint matrix of the oracle's system, every block, within kinetic_cov_compare.reference's tolerance
test_zz_report prints every measured value next to its tolerance.  Cases: kinetic_cov_compare.gallop_case (12 frames, computed once per session)."""
import ctypes as C
import os

import numpy as np
import pytest

import force_sample_compare as FS
import kinetic_cov_compare as KV
import ragged_kinetic_cov_cases as RC
from cheetah_pose_estimation_amd import _lib, abi

pytestmark = pytest.mark.gpu

REPORT = []
_RUNS = {}
N = KV.N_CASE


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _var(c):
    return {k: v[None] for k, v in c["var"].items()}


def _args(c):
    return c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], c["ko"]


def _cov(oracle, factory, name, ridge):
    """(case, handle, cpe_covariance_kinetic's outputs for the case alone) -- one call per (case, ridge) and session"""
    c = KV.gallop_case(oracle, name)
    h = factory(c["sk"], c["cams"], c["opts"])
    if (name, ridge) not in _RUNS:
        out = h.covariance_kinetic_host(*_args(c), ridge, want_L=True, **_var(c))
        assert out["status"] == abi.OK and out["seq_status"] == [abi.OK], (name, ridge)
        _RUNS[(name, ridge)] = out
    return c, h, _RUNS[(name, ridge)]


def _samples(h, c, du, zeta, ridge):
    out = h.force_samples_host(*_args(c), du[None], None if zeta is None else zeta[None], ridge, **_var(c))
    assert out["status"] == abi.OK and out["seq_status"] == [abi.OK]
    return out


def _hip_nodes(h, c, lam_f=0.0):
    G = h.eval_kinetic_system_host(c["ko"], c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], band=False, **_var(c))
    return KV.node_blocks({k: G[k][0] for k in ("Hfu", "Hff", "meta")}, lam_f), G


def _window_cov(diag, off, n):
    """W [84][84] of node n from the band the covariance call returned (tests/test_gpu_kinetic_covariance.py's rule)"""
    W = np.zeros((84, 84))
    for a in range(3):
        for b in range(3):
            blk = diag[n - a] if a == b else (off[n - b, b - a - 1] if a < b else off[n - a, a - b - 1].T)
            W[28 * a:28 * a + 28, 28 * b:28 * b + 28] = blk
    return W


# ---- 1. the kernel, tightly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ridge", [("base", 0.0), ("six", 0.0), ("flight", 0.0), ("fixed", 0.0), ("boxed", 0.0), ("fixed", 1e-6)])
def test_kernel_against_the_reference(oracle, gpu_handle_factory, name, ridge):
    """S = 65, random z and zeta, du from cpe_band_sample on the call's own L: every node's f_s - f against the reference from the HIP path's own
    H_fu / H_ff / meta.  ("fixed" at ridge 1e-6: with prescribed forces there is no wall term, M = H_ff + ridge lm_force_damping diag H_ff.)"""
    c, h, cov = _cov(oracle, gpu_handle_factory, name, ridge)
    rng = np.random.default_rng(11)
    S = 65
    z, zeta = rng.standard_normal((S, N, 28)), rng.standard_normal((S, N, 64))
    du = h.band_sample_host(cov["L"], z[None])[0]
    out = _samples(h, c, du, zeta, ridge)
    nodes, _ = _hip_nodes(h, c, ridge * c["ko"].lm_force_damping)
    Sigma = FS.dense_sigma(cov["L"][0])
    seen, worst, bound = set(), (0.0, 1.0), 0.0
    for n, (Hfu, M) in nodes.items():
        na = M.shape[0]
        seen.add(na)
        assert out["meta"][0][n, 0] == na
        zn = zeta[:, n, :na]
        ref = FS.reference(Hfu, M, Sigma[np.ix_(KV.window(n), KV.window(n))], FS.window_steps(du, n), zn, FS.sample_norms(z, zn))
        err = FS.scaled_error(FS.compact(out["f_s"][0], out["f"][0], out["meta"][0], n), ref["df"], ref["cov_f"], FS.sample_norms(z, zn))
        if err / ref["tol"] >= worst[0] / worst[1]:
            worst = (err, ref["tol"])
        bound = max(bound, ref["bound"])
        assert err <= ref["tol"], (name, n, na, err, ref["tol"], ref["r"], ref["cond"])
    _note(f"kernel {name} ridge {ridge:g}", "df error", *worst)
    assert 0.0 < bound <= 1.0
    assert seen == {"flight": {48, 51, 54}, "fixed": {48}}.get(name, {51, 54})


# ---- 2. the library's two outputs against each other, any ridge -------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("name", ["base", "boxed"])
def test_identity_with_the_force_covariance(oracle, gpu_handle_factory, name, ridge):
    """zeta = e_a with du = 0 gives M_n^-1 = sum df df^T; du = the window unit steps with zeta = NULL gives -S_n column by column; M_n^-1 + S W S^T
    with W from the band cpe_covariance_kinetic returned is that entry's cov_f (at ridge 1e-6 M_n holds the wall term, which only the library
    has)"""
    c, h, cov = _cov(oracle, gpu_handle_factory, name, ridge)
    zeta = np.zeros((64, N, 64))
    zeta[np.arange(64), :, np.arange(64)] = 1.0
    a = _samples(h, c, np.zeros((64, N, 28)), zeta, ridge)
    b = _samples(h, c, np.eye(N * 28).reshape(N * 28, N, 28), None, ridge)
    nodes0, _ = _hip_nodes(h, c)
    if ridge > 0.0:
        # r of the tolerance: the same identity in numpy on the oracle's system at this ridge (force_sample_compare.identity_error; the oracle's M
        # has the diagonal damping but no wall term)
        R, Ad, Hk, onodes = KV.oracle_system(oracle, c, ridge)
        So = KV.reference(Ad, Hk, onodes)["S"]
        r_cpu = {n: FS.identity_error(*onodes[n], So[np.ix_(KV.window(n), KV.window(n))])[0] for n in onodes}
    worst = (0.0, 1.0)
    for n in range(2, N):
        na = int(cov["meta"][0][n, 0])
        X = FS.compact(a["f_s"][0], a["f"][0], a["meta"][0], n)[:na]          # row a: C^-T e_a
        Minv = X.T @ X
        Sn = -FS.compact(b["f_s"][0], b["f"][0], b["meta"][0], n)[KV.window(n)].T          # [na][84]
        W = _window_cov(cov["cov_diag"][0], cov["cov_off"][0], n)
        Cf = Minv + Sn @ W @ Sn.T
        ref = cov["cov_f"][0][n, :na, :na]
        tol = KV.kernel_tolerance(*nodes0[n], W)[1] if ridge == 0.0 else 10.0 * max(r_cpu[n], FS.EPS * KV.scaled_condition(np.linalg.inv(Minv)))
        err = KV.scaled_difference(0.5 * (Cf + Cf.T), ref)
        if err / tol >= worst[0] / worst[1]:
            worst = (err, tol)
        assert err <= tol, (name, ridge, n, err, tol)
    _note(f"identity {name} ridge {ridge:g}", "cov_f error", *worst)


# ---- 3. the full joint path against the oracle ----------------------------------------------------------------------------------------------
def test_joint_path_against_the_oracle(oracle, gpu_handle_factory):
    c, h, cov = _cov(oracle, gpu_handle_factory, "base", 0.0)
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, 0.0)
    ref = KV.reference(Ad, Hk, nodes)
    meta = cov["meta"][0]
    assert np.array_equal(meta[:, 0], R["meta"][:, 0]) and all(np.array_equal(meta[n, 1:1 + meta[n, 0]], R["meta"][n, 1:1 + meta[n, 0]]) for n in nodes)
    z, zeta = FS.unit_samples(N, {n: nodes[n][0].shape[0] for n in nodes})
    du = h.band_sample_host(cov["L"], z[None])[0]
    out = _samples(h, c, du, zeta, 0.0)
    X = FS.joint_sum(du, {n: FS.compact(out["f_s"][0], out["f"][0], out["meta"][0], n) for n in nodes})
    J, offs = KV.joint_matrix(Ad, Hk, nodes)
    err = FS.block_errors(X, KV.scaled_inverse(J)[0], offs, nodes, N)
    for k, v in err.items():
        _note(f"joint path base ({z.shape[0]} samples)", f"{k} error", v, ref["tol"])
    assert all(v <= ref["tol"] for v in err.values()), (err, ref["tol"])


# ---- 4. structure -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "flight", "fixed"])
def test_structure(oracle, gpu_handle_factory, name):
    c, h, cov = _cov(oracle, gpu_handle_factory, name, 0.0)
    rng = np.random.default_rng(3)
    S = 5
    z, zeta = rng.standard_normal((S, N, 28)), rng.standard_normal((S, N, 64))
    du = h.band_sample_host(cov["L"], z[None])[0]
    out = _samples(h, c, du, zeta, 0.0)
    assert _bits(out["f"], cov["f"]) and _bits(out["meta"], cov["meta"]) and out["seq_status"] == cov["seq_status"]
    fs, f, meta = out["f_s"][0], out["f"][0], out["meta"][0]
    assert not fs[:, :2].any()
    nm, nc = c["ko"].dyn.n_motors, 26
    for n in range(2, N):
        na = meta[n, 0]
        free = np.zeros(64, bool)
        free[meta[n, 1:1 + na]] = True
        assert all(_bits(fs[s, n, ~free], f[n, ~free]) for s in range(S))
        assert np.all(fs[:, n, free] != f[n, free][None])
        if name == "flight" and n == KV.FLIGHT_NODE:
            assert na == 48 and not fs[:, n, nm + nc:].any()
        if name == "fixed":
            assert all(_bits(fs[s, n, nm + nc:nm + nc + 12], c["var"]["grf_fixed"][n].ravel()) for s in range(S))
    zero = _samples(h, c, np.zeros((S, N, 28)), None, 0.0)
    assert all(_bits(zero["f_s"][0][s], f) for s in range(S))


# ---- 5. sample counts and slots -----------------------------------------------------------------------------------------------------------------
def test_sample_counts_slots_and_batch(oracle, gpu_handle_factory):
    """S = 1, C - 1, C, C + 1, 2 C + 2 (C = the kernel's samples per workgroup pass): a sample's bits depend neither on S, nor on its slot, nor on
    the batch; a repeated call is bit-equal"""
    names = ("base", "seed7", "seed11")
    cs = [KV.gallop_case(oracle, n) for n in names]
    h = gpu_handle_factory(cs[0]["sk"], cs[0]["cams"], cs[0]["opts"])
    st = lambda k: np.stack([c[k] for c in cs])
    Cn = FS.CHUNK
    Smax = 2 * Cn + 2
    rng = np.random.default_rng(17)
    du, zeta = 1e-3 * rng.standard_normal((3, Smax, N, 28)), rng.standard_normal((3, Smax, N, 64))
    call = lambda: h.force_samples_host(st("q"), st("meas"), st("weight"), st("stance"), cs[0]["ko"], du, zeta, 0.0)
    a, b = call(), call()
    assert a["seq_status"] == [abi.OK] * 3
    assert all(_bits(a[k], b[k]) for k in ("f_s", "f", "meta"))
    assert not _bits(a["f_s"][0], a["f_s"][1]) and not _bits(a["f_s"][0, 0], a["f_s"][0, 1])
    for b_, S in ((0, 1), (1, Cn - 1), (2, Cn), (0, Cn + 1), (1, Smax)):
        pick = np.arange(Smax)[::-1][:S]                                   # other slots, and another pass for most of them
        one = _samples(h, cs[b_], du[b_][pick], zeta[b_][pick], 0.0)
        assert _bits(one["f_s"][0], a["f_s"][b_][pick]), (b_, S)
        assert _bits(one["f"][0], a["f"][b_]) and _bits(one["meta"][0], a["meta"][b_])
    # the device-pointer entry gives the host-pointer twin's bits
    import torch
    dev = torch.device("cuda", 0)
    T = lambda x, dt=torch.float64: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    o = dict(f_s=torch.ones(a["f_s"].shape, dtype=torch.float64, device=dev), f=torch.ones(a["f"].shape, dtype=torch.float64, device=dev),
             meta=torch.ones(a["meta"].shape, dtype=torch.int32, device=dev))
    st_, seq = h.force_samples(cs[0]["ko"], T(st("q")), T(st("meas")), T(st("weight")), T(st("stance"), torch.int32), 0.0, T(du), zeta=T(zeta), **o)
    h.synchronize()
    assert st_ == abi.OK and seq == [abi.OK] * 3
    assert all(_bits(o[k].cpu().numpy(), a[k]) for k in o)


# ---- 6. edge lengths -----------------------------------------------------------------------------------------------------------------------------
def test_edge_lengths(oracle, gpu_handle_factory):
    """N = 2 at ridge 1e-3: no node, f_s all zero, status OK; N = 3: one node whose window starts at frame 0; N = 2 at ridge 0: CPE_NUMERICAL (two
    frames have coordinates with exactly zero curvature), all zero"""
    c, h, _ = _cov(oracle, gpu_handle_factory, "base", 0.0)
    rng = np.random.default_rng(23)
    for n_, ridge in ((2, 1e-3), (3, 1e-3), (2, 0.0)):
        cut = lambda a: np.ascontiguousarray(a[:n_])[None]
        du, zeta = 1e-3 * rng.standard_normal((1, 4, n_, 28)), rng.standard_normal((1, 4, n_, 64))
        args = (cut(c["q"]), cut(c["meas"]), cut(c["weight"]), cut(c["stance"]), c["ko"])
        out = h.force_samples_host(*args, du, zeta, ridge)
        cov = h.covariance_kinetic_host(*args, ridge)
        assert out["seq_status"] == cov["seq_status"] == ([abi.NUMERICAL] if ridge == 0.0 else [abi.OK])
        assert _bits(out["f"], cov["f"]) and _bits(out["meta"], cov["meta"])
        if n_ == 2:
            assert not out["f_s"].any() and not out["f"].any() and not out["meta"].any()
        else:
            na = out["meta"][0][2, 0]
            assert na in (51, 54) and not out["f_s"][0][:, :2].any()
            df = FS.compact(out["f_s"][0], out["f"][0], out["meta"][0], 2)
            assert np.all(np.isfinite(df)) and np.all(df != 0.0)
            # the window of node 2 starts at frame 0: a step of frame 0 alone moves the node's forces (zeta = NULL: the conditional mean -S w)
            d0 = np.zeros((1, 28, n_, 28))
            d0[0, np.arange(28), 0, np.arange(28)] = 1e-3
            m = h.force_samples_host(*args, d0, None, ridge)
            assert np.all(np.abs(FS.compact(m["f_s"][0], m["f"][0], m["meta"][0], 2)).max(axis=1) > 0.0)


# ---- 7. ragged ----------------------------------------------------------------------------------------------------------------------------------
def test_ragged(oracle, gpu_handle_factory):
    """lengths 12, 7 and 3 over two models: every sequence bit-equal to its plain call, rows past a length zero; a sequence made CPE_NUMERICAL by
    its inputs (a NaN measurement with a positive weight) leaves its neighbours' bits alone"""
    base, six = KV.gallop_case(oracle, "base"), KV.gallop_case(oracle, "six")
    seqs = [base, RC.cut(six, 7), RC.cut(KV.gallop_case(oracle, "seed7"), 3)]
    model_of, lens = [0, 1, 0], [12, 7, 3]
    ridge, S = 1e-3, 3                                  # (three frames need the damping: tests/test_gpu_kinetic_covariance.py::test_edge_lengths)
    rng = np.random.default_rng(29)
    du = [1e-3 * rng.standard_normal((S, n, 28)) for n in lens]
    zeta = [rng.standard_normal((S, n, 64)) for n in lens]
    h = _lib.Handle.multi([base["sk"], six["sk"]], [base["cams"], six["cams"]], [base["opts"], six["opts"]])
    try:
        kos = [base["ko"], six["ko"]]
        (q, me, we, stn), kw = RC.ragged_args(seqs, model_of)
        r = h.force_samples_ragged_host(q, me, we, stn, kos, du, zeta, ridge=ridge, **kw)
        assert r["seq_status"] == [abi.OK] * 3
        pad = r["padded"]
        for b, c in enumerate(seqs):
            hp = gpu_handle_factory(c["sk"], c["cams"], c["opts"])
            one = hp.force_samples_host(*_args(c), du[b][None], zeta[b][None], ridge)
            assert one["seq_status"] == [abi.OK]
            assert _bits(one["f_s"][0], r["f_s"][b]) and _bits(one["f"][0], r["f"][b]) and _bits(one["meta"][0], r["meta"][b]), b
            assert not pad["f_s"][b, :, lens[b]:].any() and not pad["f"][b, lens[b]:].any() and not pad["meta"][b, lens[b]:].any()
        me2 = [m.copy() for m in me]
        l = int(np.argmax(we[1][5, 0] > 0.0))
        me2[1][5, 0, l, 0] = np.nan
        r2 = h.force_samples_ragged_host(q, me2, we, stn, kos, du, zeta, ridge=ridge, **kw)
        assert r2["seq_status"] == [abi.OK, abi.NUMERICAL, abi.OK] and r2["status"] == abi.NUMERICAL
        assert not r2["padded"]["f_s"][1].any() and not r2["padded"]["f"][1].any() and not r2["padded"]["meta"][1].any()
        assert all(_bits(r2[k][b], r[k][b]) for k in ("f_s", "f", "meta") for b in (0, 2))
    finally:
        h.close()


# ---- 8. refusals that need a handle --------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_handle(oracle, gpu_handle_factory):
    c, h, _ = _cov(oracle, gpu_handle_factory, "base", 0.0)
    from cheetah_pose_estimation_amd import priors, skeleton
    du = np.zeros((1, 1, N, 28))
    h4 = gpu_handle_factory(skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24)), c["cams"], c["opts"], priors.load_priors())
    assert h4.pb == 4
    with pytest.raises(_lib.CpeError, match="half-bandwidth 4"):
        h4.force_samples_host(*_args(c), du)
    box = np.zeros((1, N, c["ko"].dyn.n_motors, 2))
    fixed = np.zeros((1, N, c["ko"].dyn.n_feet, 3))
    with pytest.raises(_lib.CpeError, match="at most one"):
        h.force_samples_host(*_args(c), du, tau_box=box, grf_fixed=fixed)
    # too many sample frames: refused before any array is read (the arrays are those of S = 1)
    q, me, we, stn = (np.ascontiguousarray(a) for a in _args(c)[:4])
    f_s, seq = np.zeros((1, 1, N, 64)), (C.c_int32 * 1)()
    S = (2 ** 31 - 1) // N + 1
    st = h.lib.cpe_force_samples_host(h._h, C.byref(c["ko"]), 1, N, q.ctypes.data, me.ctypes.data, we.ctypes.data, stn.ctypes.data, None, None, None, 0.0, S,
                                      du.ctypes.data, None, f_s.ctypes.data, None, None, seq)
    assert st == abi.BAD_ARG and b"too many frames" in h.lib.cpe_last_error()
    for S in (0, -1):
        st = h.lib.cpe_force_samples_host(h._h, C.byref(c["ko"]), 1, N, q.ctypes.data, me.ctypes.data, we.ctypes.data, stn.ctypes.data, None, None, None, 0.0,
                                          S, du.ctypes.data, None, f_s.ctypes.data, None, None, seq)
        assert st == abi.BAD_ARG and b"S must be at least 1" in h.lib.cpe_last_error()


# ---- 9. the estimator's torque-box path, whatever the solve says --------------------------------------------------------------------------------
def test_estimator_torque_box_samples(oracle, gpu_handle_factory):
    """what estimate_grf computes after its solve (estimator._kinetic_uncertainty with tau_box and samples), on case "boxed" in place of a solve's
    result: the sample fields are cpe_force_samples' for the same tau_box and the same normals, bit for bit.  (The end-to-end test below reaches
    this path only when estimate_grf's own solve is ok.)"""
    from types import SimpleNamespace
    from cheetah_pose_estimation_amd import estimator as E
    c, h, cov = _cov(oracle, gpu_handle_factory, "boxed", 0.0)
    K, seed = 3, 7
    nm, nf = c["ko"].dyn.n_motors, c["ko"].dyn.n_feet
    res = dict(q=c["q"][None], stats=[SimpleNamespace(status=abi.OK)], tau=np.zeros((1, N, nm)), lam=np.zeros((1, N, 26)), grf=np.zeros((1, N, nf, 5)))
    req = E.PosteriorRequest(ridge=0.0, samples=K, seed=seed)
    unc = E._kinetic_uncertainty(h, c["ko"], res, c["meas"], c["weight"], c["stance"], req, tau_box=c["var"]["tau_box"])
    assert unc.reason is None and unc.fields is not None and unc.samples is not None
    sm = unc.samples
    du = h.band_sample_host(cov["L"], E.sample_normals(seed, K, N)[None])[0]
    assert _bits(sm["du"], du)
    out = _samples(h, c, du, E.sample_force_normals(seed, K, N), 0.0)
    want = E.force_sample_fields(out["f_s"][0], out["f"][0], nm, 26, nf)
    assert sorted(want) == sorted(set(E.KINETIC_SAMPLE_FIELDS) - set(E.SAMPLE_FIELDS))
    assert all(_bits(sm[k], want[k]) for k in want)
    assert np.any(sm["tau"][:, 2:] != sm["tau_mean"][None, 2:]) and _bits(sm["tau_mean"], cov["f"][0][:, :nm])
    free = _samples(h, KV.gallop_case(oracle, "base"), du, E.sample_force_normals(seed, K, N), 0.0)
    assert not _bits(free["f_s"], out["f_s"])                       # (the boxes bind: not the bits of the call without them)


# ---- 10. the estimator, through files -----------------------------------------------------------------------------------------------------------
def test_estimator_writes_force_samples(tmp_path):
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    Ne, K = 24, 3
    root = str(tmp_path / "data")
    info = write_dataset(root, N=Ne, noise_px=0.5, gallop=True)
    est = E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
    assert E.estimate_kinematics(est, solver_output=False) is True
    fresh = lambda: E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True,
                                      bound_eom_error=(-2.0, 2.0), include_camera_constraints=True, kinematic_model=False)
    out = os.path.join(root, info["data_path"], "fte_kinetic")
    kw = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True)
    load = lambda name: {k: v.copy() for k, v in np.load(os.path.join(out, name)).items()}
    same = lambda a, b: sorted(a) == sorted(b) and all(_bits(a[k], b[k]) for k in a)

    e0 = fresh()
    assert E.estimate_kinetics(e0, uncertainty=True, **kw) is True
    assert e0.samples is None and not os.path.exists(os.path.join(out, "samples.npz"))
    unc0 = load("uncertainty.npz")
    e1 = fresh()
    assert E.estimate_kinetics(e1, uncertainty=True, uncertainty_samples=K, uncertainty_seed=7, **kw) is True
    # uncertainty.npz: every array byte for byte what the call without samples writes (the archive itself carries the time of writing)
    assert same(load("uncertainty.npz"), unc0)
    z = load("samples.npz")
    shapes = dict(seed=(), ridge=(), du=(K, Ne, 28), q=(K, Ne, 54), x=(K, Ne, 28), positions=(K, Ne, 24, 3), com_pos=(K, Ne, 3), tau=(K, Ne, 22),
                  lam=(K, Ne, 26), grf_net=(K, Ne, 4, 3), tau_mean=(Ne, 22), lam_mean=(Ne, 26), grf_net_mean=(Ne, 4, 3))
    assert sorted(z) == sorted(shapes) == sorted(E.KINETIC_SAMPLE_FIELDS)
    for key, shp in shapes.items():
        assert z[key].shape == shp, key
        assert _bits(z[key], np.asarray(e1.samples[key])), key
    assert int(z["seed"]) == 7 and float(z["ridge"]) == 0.0
    # |df_a| <= sqrt(cov_f_aa) ||(zeta_n, z)||: exact for the node's own normals and the whole trajectory's z
    zn, zt = E.sample_normals(7, K, Ne), E.sample_force_normals(7, K, Ne)
    dev = (z["tau"] - z["tau_mean"][None])[:, 2:] / unc0["tau_std"][None, 2:]
    assert np.all(np.isfinite(dev)) and np.any(dev != 0.0) and not (z["tau"] - z["tau_mean"][None])[:, :2].any()
    bound = np.sqrt((zn.reshape(K, -1) ** 2).sum(axis=1)[:, None] + (zt ** 2).sum(axis=2))[:, 2:]          # (all 64 normals of the node: not below its na)
    assert np.all(np.abs(dev) <= bound[:, :, None] * (1.0 + 1e-9))
    stance = e1.kinetic["stance"]
    assert not z["grf_net"][:, stance == 0].any()
    # batches of one give the bits of the single call
    for ragged in (False, True):
        eb = fresh()
        assert E.estimate_kinetics_batch([eb], uncertainty=True, uncertainty_samples=K, uncertainty_seed=7, ragged=ragged, **kw) == [True]
        assert same(load("samples.npz"), z) and same(load("uncertainty.npz"), unc0), ragged
        assert all(_bits(np.asarray(eb.samples[k]), z[k]) for k in z)
    # the module-level estimate_grf (torque boxes around the stored torques): the same fields beside fte_grf/uncertainty.npz when the solve is ok
    import dataclasses
    e3 = fresh()
    e3.params = dataclasses.replace(e3.params, kinetic_dataset=True)             # (only the flag is the kinetic set's, as tests/test_gpu_kinetic.py)
    ok3 = E.estimate_grf(e3, solver_output=False, uncertainty=True, uncertainty_samples=K, uncertainty_seed=7)
    npz = os.path.join(root, info["data_path"], "fte_grf", "samples.npz")
    assert os.path.exists(npz) == bool(ok3) and (e3.samples is not None) == bool(ok3)
    print(f"estimate_grf(uncertainty_samples={K}): ok {ok3}")
    if ok3:
        z3 = np.load(npz)
        assert sorted(z3.files) == sorted(shapes) and all(z3[k].shape == shp for k, shp in shapes.items())
        assert all(_bits(z3[k], np.asarray(e3.samples[k])) for k in shapes) and np.all(np.isfinite(z3["tau"]))
    with pytest.raises(NotImplementedError, match="use_2d_reprojections"):
        E.estimate_kinetics(fresh(), uncertainty=True, uncertainty_samples=K, use_2d_reprojections=False, **kw)


def test_zz_report():
    """every measured error next to the tolerance applied to it"""
    for label, measure, value, tol in REPORT:
        print(f"{label:40s} {measure:40s} {value:.3e}   tolerance {tol:.3e}")
