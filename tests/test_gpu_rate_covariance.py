"""Posterior covariance of the rates on the GPU (cpe_rate_covariance, include/cpe.h) against the numpy references of tests/rate_compare.py: the
linear outputs on exact random bands, the Jacobians against central differences, the combination to round-off on the GPU's own arrays, the
end-to-end velocity covariances against finite-difference Jacobians, the batch rules, the physics-based band and the estimator through files.

Round-off tolerance of an entry that sums n three-factor products: (n + 3) 2^-52 x the same expression with every factor replaced by its
absolute value (rate_compare.abs_bound) -- the textbook bound, no measured constant.  Finite-difference tolerance: 10 x the difference between
the results at steps 1e-5 and 1e-6, per block -- set by the reference alone.  test_zz_report prints every measured error next to its tolerance.

Worst values measured on an MI355X, error as a fraction of its tolerance (test_zz_report; the same figures are in DESIGN.md 4):
  random bands, PB 3 / 4        cov_du 0.15, cov_ddu 0.23
  Jacobians                     jac_pos 0.049, jac_com 0.021 (the tolerance is 2e-9 .. 6e-9 of the block scale)
  combination, own arrays       cov_vel 0.001, cov_com 0.028, cov_com_vel 0.003, cov_du 0.093, cov_ddu 0.036; against k_marker_cov's cov_pos 0.004
  physics-based band            cov_vel 0.001, cov_com 0.004, cov_com_vel 0.0003, cov_du 0.17, cov_ddu 0.13
  end to end                    cov_vel 0.16, cov_com_vel 0.018; h^2 var du / (var u_n + var u_n-1) at most 0.32"""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import cov_compare as CC
import rate_compare as RC
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

REPORT = []
RIDGE = 1e-6
NF = 9                                           # frames of the oracle cases that the Jacobian and combination tests use
OUT = abi.RATE_COVARIANCE_OUTPUTS
COVS = OUT[:5]
N_STENCIL, N_POINT, N_VEL = 9, 28 * 28, 4 * 28 * 28          # products summed into one entry of cov_du / cov_ddu, P S P^T, a velocity covariance
_RUNS = {}


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _within(label, measure, got, ref, tol):
    """got within tol of ref entry by entry; reports the worst error over its tolerance"""
    err = np.abs(got - ref)
    pos = tol > 0
    ratio = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    _note(label, measure + " (worst error / tolerance)", ratio, 1.0)
    assert np.all(err <= tol), (label, measure, ratio)


def _psd(label, cov, tol):
    """blocks [..., 3, 3] symmetric bit for bit and PSD to the entrywise tolerance"""
    assert RC.bits_symmetric(cov), label
    ev = np.linalg.eigvalsh(cov)[..., 0]
    assert np.all(ev >= -3.0 * tol.max(axis=(-1, -2))), (label, float(ev.min()))


def _pb_handle(factory, PB):
    """PB 3: six cameras, no priors; PB 4: one camera and the packaged priors (motion-prior window 4)"""
    if PB == 3:
        return factory(skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options())
    return factory(skeleton.build_skeleton("phantom", 24), synth.make_cameras(1), abi.default_options(), priors.load_priors())


def _random_sigma(N, PB, seed):
    """(diag, off) of the inverse of a random SPD band, cut to the band"""
    d, o, _ = CC.dense_inverse(*CC.random_band(N, PB, seed))
    return d, o


# ---- 1. linear outputs, exact input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("PB", [3, 4])
def test_linear_outputs_on_random_bands(gpu_handle_factory, PB):
    """cov_du and cov_ddu against the stencil formulas, entry by entry, B = 2, N in {1, 2, 3, 4, 9}; bit-symmetric; rows 0, 1, 2 of cov_ddu
    bit-equal; N = 1 and N = 2 give the defined zeros"""
    h = _pb_handle(gpu_handle_factory, PB)
    assert h.pb == PB
    q9 = synth.make_batch(h.sk, h.cams, B=2, N=9, seed=3)["q_true"]
    for N in (1, 2, 3, 4, 9):
        bands = [_random_sigma(N, PB, 500 * PB + 10 * N + b) for b in range(2)]
        diag, off = np.stack([b[0] for b in bands]), np.stack([b[1] for b in bands])
        out = h.rate_covariance_host(q9[:, :N], diag, off, want=("cov_du", "cov_ddu"))
        assert sorted(out) == ["cov_ddu", "cov_du"]
        for b in range(2):
            du, ddu = RC.rates_from_band(diag[b], off[b], h.opts.h)
            bu, bdu = RC.abs_bound("rates", diag[b], off[b], h.opts.h)
            _within(f"PB {PB} N {N} #{b}", "cov_du", out["cov_du"][b], du, RC.roundoff_tolerance(N_STENCIL, bu))
            _within(f"PB {PB} N {N} #{b}", "cov_ddu", out["cov_ddu"][b], ddu, RC.roundoff_tolerance(N_STENCIL, bdu))
        assert RC.bits_symmetric(out["cov_du"]) and RC.bits_symmetric(out["cov_ddu"])
        if N == 1:
            assert not out["cov_du"].any() and not out["cov_ddu"].any()
        elif N == 2:
            assert not out["cov_ddu"].any() and out["cov_du"].all() and _bits(out["cov_du"][:, 0], out["cov_du"][:, 1])
        else:
            assert _bits(out["cov_ddu"][:, 0], out["cov_ddu"][:, 2]) and _bits(out["cov_ddu"][:, 1], out["cov_ddu"][:, 2])
            assert out["cov_du"].all() and out["cov_ddu"].all()


# ---- the oracle cases, first NF frames: one covariance call and one rate call per case and session ----------------------------------------
def _case_run(oracle, factory, name):
    c = CC.oracle_case(oracle, name)
    h = factory(c["sk"], c["cams"], c["opts"], c["priors"])
    if name not in _RUNS:
        q, me, we = c["q"][None, :NF], c["meas"][None, :NF], c["weight"][None, :NF]
        cov = h.covariance_host(q, me, we, RIDGE)
        assert cov["seq_status"] == [abi.OK]
        rates = h.rate_covariance_host(q, cov["cov_diag"], cov["cov_off"])
        assert sorted(rates) == sorted(OUT)
        fd = {step: (CC.marker_jacobians(oracle, c["sk"], c["q"][:NF], range(NF), step), RC.com_jacobians(oracle, c["sk"], c["q"][:NF], range(NF), step))
              for step in (1e-5, 1e-6)}
        _RUNS[name] = dict(cov={k: cov[k][0] for k in ("cov_diag", "cov_off", "cov_pos")}, rates={k: v[0] for k, v in rates.items()}, fd=fd)
    return c, h, _RUNS[name]


# ---- 2. Jacobians ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six", "mono"])
def test_jacobians_against_central_differences(oracle, gpu_handle_factory, name):
    """jac_pos and jac_com against central differences at steps 1e-5 and 1e-6, tolerance 10 x their difference per block; a column a marker does
    not depend on is exactly 0.0"""
    c, h, run = _case_run(oracle, gpu_handle_factory, name)
    (p5, c5), (p6, c6) = run["fd"][1e-5], run["fd"][1e-6]
    jp, jc = run["rates"]["jac_pos"], run["rates"]["jac_com"]
    assert jp.shape == (NF, c["sk"].n_markers, 3, 28) and jc.shape == (NF, 3, 28)
    tol_p = 10.0 * np.abs(p5 - p6).max(axis=(2, 3), keepdims=True) * np.ones_like(p5)
    tol_c = 10.0 * np.abs(c5 - c6).max(axis=(1, 2), keepdims=True) * np.ones_like(c5)
    assert np.all(tol_p > 0.0) and np.all(tol_c > 0.0)
    _within(f"jacobians {name}", "jac_pos", jp, p5, tol_p)
    _within(f"jacobians {name}", "jac_com", jc, c5, tol_c)
    _note(f"jacobians {name}", "jac_pos tolerance / block scale", float((tol_p.max(axis=(2, 3)) / np.abs(p5).max(axis=(2, 3))).max()), np.inf)
    free = ~(p5.any(axis=(0, 2)) | p6.any(axis=(0, 2)))             # [L, 28]: the differences are exactly zero at every frame, in every component
    assert free.any() and not free.all()
    zeros = np.swapaxes(jp, 1, 2)[:, :, free]                       # [NF, 3, the free (marker, column) pairs]
    assert not zeros.any() and not np.signbit(zeros).any()


# ---- 3. the combination, exact to round-off ------------------------------------------------------------------------------------------------
def _combination(label, rates, cov, h_step):
    """the identities of the combination kernel on the GPU's own arrays: cov_vel, cov_com, cov_com_vel against the numpy formulas with jac_* and
    the band, within the round-off bound; symmetric bit for bit, PSD to that bound, row 0 of the velocities zero"""
    d, o, jp, jc = cov["cov_diag"], cov["cov_off"], rates["jac_pos"], rates["jac_com"]
    t_vel = RC.roundoff_tolerance(N_VEL, RC.abs_bound("point_vel", jp, d, o, h_step))
    t_com = RC.roundoff_tolerance(N_POINT, RC.abs_bound("point", jc, d))
    t_cv = RC.roundoff_tolerance(N_VEL, RC.abs_bound("point_vel", jc, d, o, h_step))
    _within(label, "cov_vel", rates["cov_vel"], RC.point_vel_cov(jp, d, o, h_step), t_vel)
    _within(label, "cov_com", rates["cov_com"], RC.point_cov(jc, d), t_com)
    _within(label, "cov_com_vel", rates["cov_com_vel"], RC.point_vel_cov(jc, d, o, h_step), t_cv)
    _psd(label, rates["cov_vel"], t_vel); _psd(label, rates["cov_com"], t_com); _psd(label, rates["cov_com_vel"], t_cv)
    assert not rates["cov_vel"][0].any() and not rates["cov_com_vel"][0].any()
    assert rates["cov_vel"][1:].all() and rates["cov_com"].all() and rates["cov_com_vel"][1:].all()
    # the new Jacobian against the tested k_marker_cov: jac_pos Sigma(n,n) jac_pos^T is the cov_pos the covariance entry returned
    _within(label, "jac_pos Sigma jac_pos^T = cov_pos", RC.point_cov(jp, d), cov["cov_pos"], RC.roundoff_tolerance(N_POINT, RC.abs_bound("point", jp, d)))
    assert RC.bits_symmetric(rates["cov_du"]) and RC.bits_symmetric(rates["cov_ddu"])
    du, ddu = RC.rates_from_band(d, o, h_step)
    bu, bdu = RC.abs_bound("rates", d, o, h_step)
    _within(label, "cov_du", rates["cov_du"], du, RC.roundoff_tolerance(N_STENCIL, bu))
    _within(label, "cov_ddu", rates["cov_ddu"], ddu, RC.roundoff_tolerance(N_STENCIL, bdu))


@pytest.mark.parametrize("name", ["six", "mono"])
def test_combination_to_roundoff(oracle, gpu_handle_factory, name):
    c, h, run = _case_run(oracle, gpu_handle_factory, name)
    _combination(f"combination {name}", run["rates"], run["cov"], c["opts"].h)


# ---- 4. end to end against finite differences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six", "mono"])
def test_velocity_covariances_against_finite_differences(oracle, gpu_handle_factory, name):
    """cov_vel and cov_com_vel against the numpy formulas with the finite-difference Jacobians: 10 x |step 1e-5 - step 1e-6| + the round-off
    bound; h^2 var(du) < var u_n + var u_{n-1} everywhere, as the CPU test shows of the reference"""
    c, h, run = _case_run(oracle, gpu_handle_factory, name)
    d, o, hs = run["cov"]["cov_diag"], run["cov"]["cov_off"], c["opts"].h
    for key, which in (("cov_vel", 0), ("cov_com_vel", 1)):
        r5, r6 = RC.point_vel_cov(run["fd"][1e-5][which], d, o, hs), RC.point_vel_cov(run["fd"][1e-6][which], d, o, hs)
        fd = 10.0 * np.abs(r5 - r6).max(axis=(-1, -2), keepdims=True) * np.ones_like(r5)
        tol = fd + RC.roundoff_tolerance(N_VEL, RC.abs_bound("point_vel", run["fd"][1e-5][which], d, o, hs))
        _within(f"end to end {name}", key, run["rates"][key], r5, tol)
        scale = np.abs(r5).max(axis=(-1, -2))[1:]
        _note(f"end to end {name}", key + ": |step 1e-5 - step 1e-6| / block scale", float((fd.max(axis=(-1, -2))[1:] / 10.0 / scale).max()), np.inf)
    ratio = RC.variance_ratio(run["rates"]["cov_du"], d, hs)
    _note(f"end to end {name}", "h^2 var du / (var u_n + var u_n-1)", float(ratio.max()), 1.0)
    assert np.all(ratio > 0.0) and np.all(ratio < 1.0)


# ---- 5. batch rules --------------------------------------------------------------------------------------------------------------------------
def _two_models():
    out = []
    for k, (animal, kin) in enumerate((("phantom", False), ("arabia-02", True))):
        out.append((skeleton.build_skeleton(animal, 24, kinetic_dataset=kin), synth.make_cameras(4 if kin else 6, seed=100 + k),
                    abi.default_options(200.0 if kin else 120.0), kin))
    return out


def test_batch_rules(gpu_handle_factory):
    """a sequence alone, inside B = 3 and inside a ragged batch of mixed skeleton, rig and length (two models, lengths 1, 2, 3, 9, 5): bit-equal
    outputs; two runs bit-equal; zeros past a sequence's frames; an all-zero Sigma gives zero covariances and leaves the neighbours' bits alone"""
    models = _two_models()
    lens, of = [1, 2, 3, 9, 5], [0, 1, 0, 1, 0]
    seqs = []
    for s, (N, m) in enumerate(zip(lens, of)):
        skm, cm, om, kin = models[m]
        q = synth.make_batch(skm, cm, B=1, N=9, fps=1.0 / om.h, seed=40 + s, kinetic_dataset=kin)["q_true"][0, :N]
        seqs.append((q,) + _random_sigma(N, 3, 900 + s))
    hm = _lib.Handle.multi([m[0] for m in models], [m[1] for m in models], [m[2] for m in models])
    try:
        r = hm.rate_covariance_ragged_host([s[0] for s in seqs], [s[1] for s in seqs], [s[2] for s in seqs], of)
        r2 = hm.rate_covariance_ragged_host([s[0] for s in seqs], [s[1] for s in seqs], [s[2] for s in seqs], of)
        # what a handle refuses: a model index or a frame count out of range (the plain handle is refused below)
        one = (C.c_int32 * 1)
        buf = np.zeros(9 * 4 * 28 * 28)
        for mo, nf, word in ((2, 3, b"model index"), (-1, 3, b"model index"), (0, 0, b"frame count"), (0, 4, b"frame count")):
            st = hm.lib.cpe_rate_covariance_ragged_host(hm._h, 1, 3, one(mo), one(nf), buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                                        buf.ctypes.data, None, None, None, None, None, None)
            assert st == abi.BAD_ARG and word in hm.lib.cpe_last_error() and b"cpe_rate_covariance_ragged_host" in hm.lib.cpe_last_error()
    finally:
        hm.close()
    assert sorted(k for k in r if k != "padded") == sorted(OUT)
    for k in OUT:
        assert _bits(r["padded"][k], r2["padded"][k]), k
    for s, (q, d, o) in enumerate(seqs):
        skm, cm, om, _ = models[of[s]]
        hs = gpu_handle_factory(skm, cm, om)
        one = hs.rate_covariance_host(q[None], d[None], o[None])
        for k in OUT:
            assert _bits(one[k][0], r[k][s]), (s, k)
            assert not r["padded"][k][s, lens[s]:].any(), (s, k)
        if lens[s] == 1:
            assert not any(one[k].any() for k in ("cov_du", "cov_ddu", "cov_vel", "cov_com_vel")) and one["cov_com"].all()
        if lens[s] == 2:
            assert not one["cov_ddu"].any() and one["cov_du"].all()
    # plain batch of three, and one of them without a factor (Sigma = 0)
    skm, cm, om, _ = models[0]
    h = gpu_handle_factory(skm, cm, om)
    q = synth.make_batch(skm, cm, B=3, N=9, seed=60)["q_true"]
    bands = [_random_sigma(9, 3, 950 + b) for b in range(3)]
    d, o = np.stack([b[0] for b in bands]), np.stack([b[1] for b in bands])
    a, b2 = h.rate_covariance_host(q, d, o), h.rate_covariance_host(q, d, o)
    assert all(_bits(a[k], b2[k]) for k in OUT)
    for s in (0, 2):
        one = h.rate_covariance_host(q[s:s + 1], d[s:s + 1], o[s:s + 1])
        assert all(_bits(one[k][0], a[k][s]) for k in OUT), s
    d0, o0 = d.copy(), o.copy()
    d0[1] = 0.0; o0[1] = 0.0
    z = h.rate_covariance_host(q, d0, o0)
    for k in OUT:
        assert _bits(z[k][0], a[k][0]) and _bits(z[k][2], a[k][2]), k
    assert not any(z[k][1].any() for k in COVS) and _bits(z["jac_pos"][1], a["jac_pos"][1]) and _bits(z["jac_com"][1], a["jac_com"][1])
    # a subset of the outputs gives the same bits as the full call (the Jacobians then live in the handle's scratch)
    part = h.rate_covariance_host(q, d, o, want=("cov_vel", "cov_com_vel"))
    assert sorted(part) == ["cov_com_vel", "cov_vel"] and _bits(part["cov_vel"], a["cov_vel"]) and _bits(part["cov_com_vel"], a["cov_com_vel"])
    # the ragged entries refuse a plain handle
    one = (C.c_int32 * 1)
    st = h.lib.cpe_rate_covariance_ragged_host(h._h, 1, 9, one(0), one(9), q.ctypes.data, d.ctypes.data, o.ctypes.data, d0.ctypes.data, None, None,
                                               None, None, None, None)
    assert st == abi.BAD_ARG and b"plain handle" in h.lib.cpe_last_error()


def test_device_pointer_entry_gives_the_host_twin_bits(gpu_handle_factory):
    """Handle.rate_covariance on torch tensors against rate_covariance_host"""
    import torch
    h = _pb_handle(gpu_handle_factory, 3)
    q = synth.make_batch(h.sk, h.cams, B=2, N=4, seed=8)["q_true"]
    bands = [_random_sigma(4, 3, 970 + b) for b in range(2)]
    d, o = np.stack([b[0] for b in bands]), np.stack([b[1] for b in bands])
    ref = h.rate_covariance_host(q, d, o)
    dev = {k: torch.full(v.shape, float("nan"), dtype=torch.float64, device="cuda") for k, v in ref.items()}
    h.rate_covariance(h._to_device(q), h._to_device(d), h._to_device(o), **dev)
    h.synchronize()
    for k in OUT:
        assert _bits(dev[k].cpu().numpy(), ref[k]), k


def test_kinetic_band(oracle, gpu_handle_factory):
    """the band of the physics-based covariance, N = 9: the identities of the combination hold on it"""
    import kinetic_cov_compare as KV
    c = KV.gallop_case(oracle, "base")
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"])
    cut = lambda a: np.ascontiguousarray(a[None, :NF])
    cov = h.covariance_kinetic_host(cut(c["q"]), cut(c["meas"]), cut(c["weight"]), cut(c["stance"]), c["ko"], 1e-3)
    assert cov["seq_status"] == [abi.OK]
    rates = h.rate_covariance_host(cut(c["q"]), cov["cov_diag"], cov["cov_off"])
    _combination("kinetic band", {k: v[0] for k, v in rates.items()}, {k: cov[k][0] for k in ("cov_diag", "cov_off", "cov_pos")}, c["opts"].h)


# ---- 6. the estimator, through files --------------------------------------------------------------------------------------------------------
TODAY = dict(cov_u=(28, 28), u_std=(28,), positions_cov=(24, 3, 3), positions_std=(24, 3))
KINETIC_TODAY = dict(TODAY, tau_std=(22,), lambda_std=(26,), grf_std=(4, 3), tau_cov=(22, 22))
RATES = dict(du_std=(28,), ddu_std=(28,), velocities_cov=(24, 3, 3), velocities_std=(24, 3), com_cov=(3, 3), com_std=(3,))
RATES_VEL = dict(com_vel_cov=(3, 3), com_vel_std=(3,), speed_std=())


def _check_files(E, N, d_rates, d_unc, d_off, est_rates, est_unc, today):
    """uncertainty.npz of a run with uncertainty_rates=True against the run with uncertainty=True alone and the run without: today's fields
    bit-equal plus exactly the new fields with their shapes; no other file changes"""
    z, zu = np.load(os.path.join(d_rates, "uncertainty.npz")), np.load(os.path.join(d_unc, "uncertainty.npz"))
    assert sorted(zu.files) == sorted(list(today) + ["ridge"]) and sorted(est_unc.uncertainty) == sorted(zu.files)
    assert sorted(z.files) == sorted(list(today) + ["ridge"] + list(RATES) + list(RATES_VEL)) == sorted(list(zu.files) + list(E.RATE_FIELDS))
    for key in zu.files:
        assert _bits(z[key], zu[key]), key
    for key, shp in RATES.items():
        assert z[key].shape == (N,) + shp, key
    for key, shp in RATES_VEL.items():
        assert z[key].shape == (N - 1,) + shp, key
    for key in z.files:
        assert _bits(z[key], np.asarray(est_rates.uncertainty[key])), key
    assert z["com_vel_std"].shape == est_rates.com_vel.shape
    assert np.all(z["du_std"] > 0.0) and np.all(z["ddu_std"] > 0.0) and np.all(z["com_std"] > 0.0) and np.all(z["com_vel_std"] > 0.0)
    assert np.all(z["velocities_std"][1:] > 0.0) and not z["velocities_std"][0].any() and np.all(z["speed_std"] > 0.0)
    assert _bits(z["speed_std"], E.speed_std_of(est_rates.com_vel, z["com_vel_cov"]))
    assert sorted(f for f in os.listdir(d_rates) if f != "uncertainty.npz") == sorted(os.listdir(d_off)) == sorted(f for f in os.listdir(d_unc) if f != "uncertainty.npz")
    assert "uncertainty.npz" not in os.listdir(d_off)
    return z


def _same_fields(za, zb, where):
    assert sorted(za.files) == sorted(zb.files), where
    for key in za.files:
        assert _bits(za[key], zb[key]), (where, key)


def test_estimate_kinematics_writes_rates(tmp_path):
    """single, plain batch and ragged batch: the fields above, and every sequence's fields inside a batch bit-equal to its own single call"""
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    specs = [("2019_03_07/synth/run1", 24, 5, 6), ("2019_03_07/synth/run2", 24, 9, 6), ("2019_03_09/synth/run3", 30, 6, 4)]
    roots = {k: str(tmp_path / k) for k in ("off", "unc", "single", "plain", "ragged")}
    ests = {}
    for k, root in roots.items():
        for path, N, seed, nc in specs:
            write_dataset(root, data_path=path, N=N, seed=seed, n_cams=nc)
        ests[k] = [E.init_trajectory(root_dir=root, data_path=p, cheetah_name="phantom", kinetic_dataset=False, solver_path="/unused/ipopt",
                                     kinematic_model=True) for p, _, _, _ in specs]
    assert all(E.estimate_kinematics(e, solver_output=False) for e in ests["off"])
    assert all(E.estimate_kinematics(e, solver_output=False, uncertainty=True) for e in ests["unc"])
    assert all(E.estimate_kinematics(e, solver_output=False, uncertainty=True, uncertainty_rates=True) for e in ests["single"])
    assert E.estimate_kinematics_batch(ests["plain"], uncertainty=True, uncertainty_rates=True) == [True] * 3
    assert E.estimate_kinematics_batch(ests["ragged"], ragged=True, uncertainty=True, uncertainty_rates=True) == [True] * 3
    for k, (path, N, _, _) in enumerate(specs):
        D = {r: os.path.join(roots[r], path, "fte_kinematic") for r in roots}
        z = _check_files(E, N, D["single"], D["unc"], D["off"], ests["single"][k], ests["unc"][k], TODAY)
        assert ests["off"][k].uncertainty is None
        for r in ("plain", "ragged"):
            _same_fields(z, np.load(os.path.join(D[r], "uncertainty.npz")), (r, k))
            assert all(_bits(np.asarray(ests[r][k].uncertainty[key]), z[key]) for key in z.files), (r, k)


KW = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True)
SETS = ((24, 6, 5), (18, 4, 7))                  # (frames, cameras, seed)


@pytest.fixture(scope="module")
def kinetic_sets(tmp_path_factory):
    """two sequences on disk with their kinematic results; fresh(prefix): physics-stage estimators whose outputs go under a prefix of their own"""
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    tmp = tmp_path_factory.mktemp("rate_kinetic")
    sets = []
    for k, (N, n_cams, seed) in enumerate(SETS):
        root = str(tmp / f"set{k}")
        info = write_dataset(root, data_path=f"2019_03_07/synth/run{k}", N=N, noise_px=0.5, gallop=True, seed=seed, n_cams=n_cams)
        est = E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
        assert E.estimate_kinematics(est, solver_output=False) is True
        sets.append((root, info["data_path"]))

    def fresh(prefix):
        ests = []
        for root, dp in sets:
            dst = os.path.join(prefix, dp, "fte_kinematic")
            if not os.path.exists(dst):
                shutil.copytree(os.path.join(root, dp, "fte_kinematic"), dst)
            ests.append(E.init_trajectory(root, dp, "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True, bound_eom_error=(-2.0, 2.0),
                                          include_camera_constraints=True, kinematic_model=False))
        return ests
    return str(tmp), sets, fresh


def test_estimate_kinetics_writes_rates(kinetic_sets):
    """estimate_kinetics alone, and estimate_kinetics_batch plain and ragged: the same rules as for the kinematic solve"""
    from cheetah_pose_estimation_amd import estimator as E
    tmp, sets, fresh = kinetic_sets
    P = lambda name: os.path.join(tmp, "out_" + name)
    runs = {name: fresh(P(name)) for name in ("off", "unc", "single", "plain", "ragged")}
    assert all(E.estimate_kinetics(e, out_dir_prefix=P("off"), **KW) is True for e in runs["off"])
    assert all(E.estimate_kinetics(e, uncertainty=True, out_dir_prefix=P("unc"), **KW) is True for e in runs["unc"])
    assert all(E.estimate_kinetics(e, uncertainty=True, uncertainty_rates=True, out_dir_prefix=P("single"), **KW) is True for e in runs["single"])
    for name, ragged in (("plain", False), ("ragged", True)):
        assert E.estimate_kinetics_batch(runs[name], ragged=ragged, uncertainty=True, uncertainty_rates=True, out_dir_prefix=P(name), **KW) == [True] * 2
    for k, (root, dp) in enumerate(sets):
        D = {name: os.path.join(P(name), dp, "fte_kinetic") for name in runs}
        z = _check_files(E, SETS[k][0], D["single"], D["unc"], D["off"], runs["single"][k], runs["unc"][k], KINETIC_TODAY)
        for name in ("plain", "ragged"):
            _same_fields(z, np.load(os.path.join(D[name], "uncertainty.npz")), (name, k))
            assert all(_bits(np.asarray(runs[name][k].uncertainty[key]), z[key]) for key in z.files), (name, k)


# ---- 7. report -----------------------------------------------------------------------------------------------------------------------------
def test_zz_report():
    """every measured error next to the tolerance applied to it (inf = reported, not asserted), and the worst ratio of every kind"""
    worst = {}
    for label, measure, value, tol in REPORT:
        print(f"{label:28s} {measure:62s} {value:.3e}   tolerance {tol:.3e}")
        if np.isfinite(tol):
            key = (label.split(" ")[0], measure.split(" (")[0])
            worst[key] = max(worst.get(key, 0.0), value / tol)
    for (group, measure), ratio in sorted(worst.items()):
        print(f"worst {group}: {measure}: {ratio:.3f} of its tolerance")
