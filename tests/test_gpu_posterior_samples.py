"""Draws from the posterior of the kinematic estimate on the GPU (cpe_band_sample, cpe_posterior_samples, include/cpe.h) against the numpy
references of tests/sample_compare.py: the banded back substitution on random bands and on the solver's own factors, its independence of the
slot, the sample count and the batch, ragged lengths, the identity sum_s du_s du_s^T = Sigma, the poses of the samples against the oracle's
coordinate moves, and the estimator through files.

Error unit: |du - ref| / (s_a ||z||_2), s_a = sqrt(Sigma_aa) of the dense inverse.  Tolerance per matrix: 10 x max(r, 2^-52 x Jacobi-scaled
condition number), r = the discrepancy between the helper's two float64 routes on that matrix (sample_compare.reference) -- measured on the
reference, never on the GPU.  test_zz_report prints every measured value next to its tolerance."""
import os
import sys

import numpy as np
import pytest

import cov_compare as CC
import sample_compare as SM
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

NX = SM.NX
REPORT = []                                      # (label, measure, value, tolerance)


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _pb_handle(factory, PB):
    """a handle of half-bandwidth PB (cpe_band_sample reads nothing else of it)"""
    if PB == 3:
        return factory(skeleton.build_skeleton("phantom", 25), synth.make_cameras(6), abi.default_options())
    return factory(skeleton.build_skeleton("phantom", 24), synth.make_cameras(2), abi.default_options(), priors.load_priors())


def _factor(N, PB, seed):
    return CC.cholesky_layout(*CC.random_band(N, PB, seed))


def _check_draws(label, L, z, du):
    R = SM.reference(L, z)
    err = SM.scaled_error(du, R["du"], R["s"], z)
    _note(label, "error", err, R["tol"])
    assert err <= R["tol"], (label, err, R["tol"])
    return R


# ---- 1. the back substitution against the reference ---------------------------------------------------------------------------------------
RANDOM_CASES = [(PB, N, 65) for PB in (3, 4) for N in list(range(1, 2 * PB + 4)) + [57]] + [(4, 200, 64)]


@pytest.mark.parametrize("PB,N,S", RANDOM_CASES)
def test_band_sample_on_random_bands(gpu_handle_factory, PB, N, S):
    """random SPD block bands, two different factors per call; every length from 1 to 2 PB + 3 (the ring of earlier frames unfilled, exactly
    filled and sliding), 57, and one of 200 frames"""
    h = _pb_handle(gpu_handle_factory, PB)
    assert h.pb == PB
    L = np.stack([_factor(N, PB, 2000 * PB + 10 * N + b) for b in range(2)])
    z = np.random.default_rng(N + PB).standard_normal((2, S, N, NX))
    du = h.band_sample_host(L, z)
    assert du.shape == z.shape
    for b in range(1 if N == 200 else 2):                                 # (one reference at 5 600 unknowns: seconds each)
        _check_draws(f"random PB {PB} N {N} #{b}", L[b], z[b], du[b])


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_band_sample_sample_counts(gpu_handle_factory, S):
    """N = 11 at every kind of sample count: one lane, a wave short of one, a full wave, one past it, two waves and a part"""
    for PB in (3, 4):
        h = _pb_handle(gpu_handle_factory, PB)
        L = _factor(11, PB, 77 + PB)[None]
        z = np.random.default_rng(S).standard_normal((1, S, 11, NX))
        _check_draws(f"random PB {PB} N 11 S {S}", L[0], z[0], h.band_sample_host(L, z)[0])


@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("name", ["six", "two", "mono"])
def test_band_sample_on_the_solvers_factors(oracle, gpu_handle_factory, name, ridge):
    """the factor cpe_covariance itself returns at the oracle's solution of the named cases ("mono": PB 4, scaled condition 8.5e9 at ridge 0);
    the reference solves with the same factor"""
    c = CC.oracle_case(oracle, name)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    assert h.pb == c["PB"] == (4 if name == "mono" else 3)
    out = h.covariance_host(c["q"][None], c["meas"][None], c["weight"][None], ridge, want_L=True)
    assert out["seq_status"] == [abi.OK]
    z = np.random.default_rng(5).standard_normal((1, 65, CC.N_CASE, NX))
    du = h.band_sample_host(out["L"], z)
    R = _check_draws(f"{name} ridge {ridge:g}", out["L"][0], z[0], du[0])
    _note(f"{name} ridge {ridge:g}", "scaled condition", R["cond"], np.inf)


# ---- 2. slot, count and batch independence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("PB", [3, 4])
def test_a_sample_does_not_depend_on_its_slot_or_its_batch(gpu_handle_factory, PB):
    h = _pb_handle(gpu_handle_factory, PB)
    N, S = 11, 130
    L = np.stack([_factor(N, PB, 31 + PB), _factor(N, PB, 32 + PB)])
    z = np.random.default_rng(PB).standard_normal((2, S, N, NX))
    du = h.band_sample_host(L, z)
    assert _bits(h.band_sample_host(L, z), du)                            # a second run
    for s in (0, 63, 64, 129):                                            # the same sample alone: S = 1, slot 0
        assert _bits(h.band_sample_host(L[:1], z[:1, s:s + 1]), du[:1, s:s + 1]), s
    for b in range(2):                                                    # a sequence alone: B = 1
        assert _bits(h.band_sample_host(L[b:b + 1], z[b:b + 1]), du[b:b + 1]), b
    assert _bits(h.band_sample_host(L[::-1].copy(), z[::-1].copy())[::-1], du)


@pytest.mark.parametrize("PB", [3, 4])
def test_ragged_lengths(gpu_handle_factory, PB):
    """n_frames = [11, 4, 0, 7] in N = 11: each sequence bit-equal to its own plain call, zeros past its end; the sequence of no frames is given
    NaN-filled L and z and returns zeros"""
    h = _pb_handle(gpu_handle_factory, PB)
    N, S, lens = 11, 65, [11, 4, 0, 7]
    L = np.full((4, N, PB + 1, NX, NX), np.nan)
    z = np.full((4, S, N, NX), np.nan)
    rng = np.random.default_rng(40 + PB)
    own = []
    for b, n in enumerate(lens):
        if n:
            Lb, zb = _factor(n, PB, 50 + b), rng.standard_normal((S, n, NX))
            L[b, :n], z[b, :, :n] = Lb, zb
            L[b, n:] = 0.0
            own.append(h.band_sample_host(Lb[None], zb[None])[0])
        else:
            own.append(None)
    du = h.band_sample_host(L, z, lens)
    for b, n in enumerate(lens):
        assert not du[b, :, n:].any() and np.all(np.isfinite(du[b]))
        if n:
            assert _bits(du[b, :, :n], own[b]), b
    # the blocks past a sequence's end are not used either: NaN there changes nothing
    L2 = L.copy()
    L2[1, 4:] = np.nan
    for n in range(4):
        L2[1, n, 4 - n:] = np.nan                                         # block (n + i, n) with n + i >= 4
    assert _bits(h.band_sample_host(L2, z, lens), du)


def test_refusals_that_need_a_handle(gpu_handle_factory):
    """a half-bandwidth above 4 in cov_check's wording, a null array and a model index out of range: CPE_BAD_ARG through the wrappers, nothing
    launched (the refusals that need no handle: tests/test_posterior_samples_host.py)"""
    w5 = priors.load_priors(path=os.path.join(os.path.dirname(__file__), "golden", "priors_k3_w5_dense.npz"))
    h5 = gpu_handle_factory(skeleton.build_skeleton("phantom", 24), synth.make_cameras(2), abi.default_options(), w5)
    assert h5.pb == 5
    with pytest.raises(_lib.CpeError, match="cpe_band_sample_host: half-bandwidth 5 .* is not supported by the covariance sweep"):
        h5.band_sample_host(np.zeros((1, 2, 6, NX, NX)), np.zeros((1, 1, 2, NX)))
    h = _pb_handle(gpu_handle_factory, 3)
    z = np.zeros((1, 1, 2, NX))
    assert h.lib.cpe_band_sample_host(h._h, 1, 2, None, None, 1, z.ctypes.data, z.ctypes.data) == abi.BAD_ARG
    assert b"cpe_band_sample_host: null argument" in h.lib.cpe_last_error()
    with pytest.raises(_lib.CpeError, match="cpe_posterior_samples_host: model index of sequence 0 out of range"):
        h.posterior_samples_host([np.zeros((2, h.nq))], [np.zeros((1, 2, NX))], [1])
    with pytest.raises(ValueError, match="half-bandwidth is 3"):
        h.band_sample_host(np.zeros((1, 2, 5, NX, NX)), z)


# ---- 3. the identity: the draws of the unit vectors sum to Sigma --------------------------------------------------------------------------
@pytest.mark.parametrize("PB", [3, 4])
def test_unit_vectors_sum_to_the_covariance(gpu_handle_factory, PB):
    """N = 6, S = 168 = every unit vector: sum_s du_s du_s^T cut to the band against the dense inverse (tolerance from the reference's own sum)
    and against cpe_band_inverse of the same factor (both within that tolerance of the inverse: twice it of each other)"""
    h = _pb_handle(gpu_handle_factory, PB)
    N = 6
    L = _factor(N, PB, 90 + PB)
    du = h.band_sample_host(L[None], SM.unit_vectors(N)[None])[0]
    assert du.shape == (N * NX, N, NX)
    R = SM.reference(L, identity=True)
    diag, off = SM.band_of_sum(du, PB)
    err = CC.scaled_error(diag, off, R["diag"], R["off"])
    _note(f"identity PB {PB}", "error against the dense inverse", err, R["tol_identity"])
    assert err <= R["tol_identity"]
    gd, go = h.band_inverse_host(L[None])
    err2 = CC.scaled_error(diag, off, gd[0], go[0])
    _note(f"identity PB {PB}", "error against cpe_band_inverse", err2, 2.0 * R["tol_identity"])
    assert err2 <= 2.0 * R["tol_identity"]
    # e_s hits frames <= its own only: du_s is zero in the frames after the unit vector's
    for s in (0, NX * 3 + 5, N * NX - 1):
        assert not du[s, s // NX + 1:].any() and du[s, s // NX].any()


# ---- 4. the poses of the samples ----------------------------------------------------------------------------------------------------------
def _pose_case(oracle, h):
    c = CC.oracle_case(oracle, "six")
    N, S = 6, 3
    q = np.ascontiguousarray(c["q"][:N])
    out = h.covariance_host(q[None], c["meas"][None, :N], c["weight"][None, :N], 1e-6, want_L=True)
    assert out["seq_status"] == [abi.OK]
    du = h.band_sample_host(out["L"], SM.normals(3, S, N)[None])
    return c, q, du


def test_posterior_samples_against_the_oracles_moves(oracle, gpu_handle_factory):
    """case "six" cut to 6 frames, 3 draws.  Reference: 28 oracle.move_coordinate calls per frame, synth.fk_numpy of the result.  positions to
    1e-10 m, q through the sin and cos of every angle to 1e-10 (free of 2 pi branches), the joint equalities of q_s below 1e-12.
    du = 0 against cpe_forward_kinematics(q): to 1e-13 m, NOT bit for bit -- observed on an MI355X: 2.2e-16 m (a leg link's Euler angles go through
    its leg angle and back)."""
    c = CC.oracle_case(oracle, "six")
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"], c["priors"])
    c, q, du = _pose_case(oracle, h)
    sk, S, N = c["sk"], du.shape[1], q.shape[0]
    assert np.abs(du).max() > 1e-4                                       # the draws move the pose by far more than the tolerances below
    ps = h.posterior_samples_host(q[None], du)
    assert ps["q"].shape == (1, S, N, sk.nq) and ps["positions"].shape == (1, S, N, sk.n_markers, 3)
    worst_p = worst_q = worst_c = 0.0
    for s in range(S):
        qr = SM.moved(oracle, sk, q, du[0, s])
        worst_p = max(worst_p, float(np.abs(ps["positions"][0, s] - synth.fk_numpy(sk, qr)[0]).max()))
        ang_g, ang_r = ps["q"][0, s][:, 3:], qr[:, 3:]
        worst_q = max(worst_q, float(np.abs(ps["q"][0, s][:, :3] - qr[:, :3]).max()), float(np.abs(np.sin(ang_g) - np.sin(ang_r)).max()),
                      float(np.abs(np.cos(ang_g) - np.cos(ang_r)).max()))
        worst_c = max(worst_c, max(float(np.abs(oracle.constraints(sk, ps["q"][0, s, n])).max()) for n in range(N)))
    _note("poses six", "positions against the oracle's moves (m)", worst_p, 1e-10)
    _note("poses six", "q through sin / cos", worst_q, 1e-10)
    _note("poses six", "joint equalities of q_s", worst_c, 1e-12)
    assert worst_p < 1e-10 and worst_q < 1e-10 and worst_c < 1e-12
    # positions are those of q_s, and without positions the same q_s
    assert _bits(h.posterior_samples_host(q[None], du, want_positions=False)["q"], ps["q"])
    # du = 0: the estimate itself, every sample the same bits
    z0 = h.posterior_samples_host(q[None], np.zeros_like(du))
    for s in range(1, S):
        assert _bits(z0["q"][0, s], z0["q"][0, 0]) and _bits(z0["positions"][0, s], z0["positions"][0, 0])
    import torch
    dev = torch.device("cuda", 0)
    pos = torch.empty((1, N, sk.n_markers, 3), dtype=torch.float64, device=dev)
    h.forward_kinematics(torch.tensor(q[None], device=dev), pos); h.synchronize()
    d0 = float(np.abs(z0["positions"][0, 0] - pos[0].cpu().numpy()).max())
    _note("poses six", "du = 0 against cpe_forward_kinematics (m)", d0, 1e-13)
    print("du = 0 against cpe_forward_kinematics:", "bit-equal" if d0 == 0.0 else f"{d0:.3e} m")
    assert d0 <= 1e-13
    # a mixed call: the zero sample next to others keeps its bits
    mixed = du.copy(); mixed[0, 1] = 0.0
    pm = h.posterior_samples_host(q[None], mixed)
    assert _bits(pm["q"][0, 1], z0["q"][0, 0]) and _bits(pm["q"][0, 0], ps["q"][0, 0]) and _bits(pm["positions"][0, 2], ps["positions"][0, 2])


def test_posterior_samples_ragged(oracle, gpu_handle_factory):
    """a Handle.multi of two skeletons, lengths [6, 4]: each sequence bit-equal to its plain call on a handle of its own model, zeros past its end"""
    c = CC.oracle_case(oracle, "six")
    sk2 = skeleton.build_skeleton("jules", 25)
    assert _lib.shape_signature(sk2) == _lib.shape_signature(c["sk"])
    hs = [gpu_handle_factory(c["sk"], c["cams"], c["opts"]), gpu_handle_factory(sk2, c["cams"], c["opts"])]
    _, q, du = _pose_case(oracle, hs[0])
    qs, dus = [q, np.ascontiguousarray(q[:4])], [du[0], np.ascontiguousarray(du[0][::-1, :4])]
    hm = _lib.Handle.multi([c["sk"], sk2], [c["cams"], c["cams"]], [c["opts"], c["opts"]])
    try:
        for models in ([0, 1], [1, 0]):
            out = hm.posterior_samples_host(qs, dus, models)
            for b in range(2):
                own = hs[models[b]].posterior_samples_host(qs[b][None], dus[b][None])
                assert _bits(out["q"][b], own["q"][0]) and _bits(out["positions"][b], own["positions"][0]), (models, b)
            assert not out["padded"]["q"][1, :, 4:].any() and not out["padded"]["positions"][1, :, 4:].any()
    finally:
        hm.close()
    a, b_ = hs[0].posterior_samples_host(qs[1][None], dus[1][None]), hs[1].posterior_samples_host(qs[1][None], dus[1][None])
    assert not _bits(a["positions"], b_["positions"])                   # the two skeletons do differ


# ---- 5. the estimator, through files ------------------------------------------------------------------------------------------------------
def _init(E, root, path, **kw):
    return E.init_trajectory(root_dir=root, data_path=path, cheetah_name="phantom", kinetic_dataset=False, solver_path="/unused/ipopt",
                             kinematic_model=True, **kw)


def test_estimator_writes_samples(tmp_path):
    sys.path.insert(0, os.path.dirname(__file__))
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    path, N, K = "2019_03_07/synth/run1", 40, 4
    roots = {k: str(tmp_path / k) for k in ("none", "single", "seed", "batch", "ragged")}
    for root in roots.values():
        write_dataset(root, data_path=path, N=N, seed=5, n_cams=6)
    ests = {k: _init(E, root, path) for k, root in roots.items()}
    kw = dict(solver_output=False, uncertainty=True, uncertainty_samples=K, uncertainty_seed=7)
    assert E.estimate_kinematics(ests["none"], solver_output=False, uncertainty=True)
    assert E.estimate_kinematics(ests["single"], **kw)
    assert E.estimate_kinematics(ests["seed"], **dict(kw, uncertainty_seed=8))
    assert E.estimate_kinematics_batch([ests["batch"]], **kw) == [True]
    assert E.estimate_kinematics_batch([ests["ragged"]], ragged=True, **kw) == [True]
    dirs = {r: os.path.join(roots[r], path, "fte_kinematic") for r in roots}
    read = lambda r, f: open(os.path.join(dirs[r], f), "rb").read()
    assert not os.path.exists(os.path.join(dirs["none"], "samples.npz")) and ests["none"].samples is None
    for r in ("single", "seed", "batch", "ragged"):
        assert read(r, "uncertainty.npz") == read("none", "uncertainty.npz"), r          # byte-equal to a run without samples
        assert sorted(os.listdir(dirs[r])) == sorted(os.listdir(dirs["none"]) + ["samples.npz"])
    za = np.load(os.path.join(dirs["single"], "samples.npz"))
    L_, nq = ests["single"].skeleton.n_markers, ests["single"].skeleton.nq
    shapes = dict(seed=(), ridge=(), du=(K, N, 28), q=(K, N, nq), x=(K, N, 28), positions=(K, N, L_, 3), com_pos=(K, N, 3))
    assert sorted(za.files) == sorted(E.SAMPLE_FIELDS) == sorted(shapes)
    for key, shp in shapes.items():
        assert za[key].shape == shp and np.all(np.isfinite(za[key])), key
        assert _bits(za[key], np.asarray(ests["single"].samples[key])), key
        for r in ("batch", "ragged"):
            assert _bits(np.load(os.path.join(dirs[r], "samples.npz"))[key], za[key]), (r, key)
    assert int(za["seed"]) == 7 and float(za["ridge"]) == 0.0
    zs = np.load(os.path.join(dirs["seed"], "samples.npz"))
    assert int(zs["seed"]) == 8 and not np.array_equal(zs["du"], za["du"])
    assert _bits(za["x"], ests["single"].relative_angles(za["q"]))
    # the draws scatter as the covariance says: every |du| within 6 standard deviations (4 x 40 x 28 normal draws)
    u_std = np.load(os.path.join(dirs["single"], "uncertainty.npz"))["u_std"]
    assert np.all(np.abs(za["du"]) < 6.0 * u_std[None]) and np.abs(za["du"] / u_std[None]).max() > 1.0
    # the antithetic pair +-du: the mean of the two poses' positions is off the estimate's positions by the second order only -- the
    # retraction is centred on the estimate and is no offset
    e = ests["single"]
    h = _lib.Handle(e.skeleton, e.cams, abi.default_options(e.scene.fps))
    try:
        q = e.result["q"]
        plus, minus = h.posterior_samples_host(q, za["du"][None]), h.posterior_samples_host(q, -za["du"][None])
        assert _bits(plus["positions"][0], za["positions"]) and _bits(plus["q"][0], za["q"])
        first = np.abs(plus["positions"][0] - e.result["positions"]).max()
        mean_off = np.abs(0.5 * (plus["positions"][0] + minus["positions"][0]) - e.result["positions"]).max()
        _note("estimator", "antithetic mean off the estimate (m)", mean_off, 0.5 * first)
        assert first > 0.0 and mean_off < 0.5 * first
    finally:
        h.close()


def test_zz_report():
    """every measured value next to its tolerance, and the worst of each kind"""
    assert REPORT, "run with the other tests of this module"
    print("\n== posterior samples, measured on this GPU ==")
    for label, measure, value, tol in REPORT:
        print(f"{label:32s} {measure:48s} {value:10.3e}   tolerance {tol:10.3e}")
    for kind in ("random", "six", "two", "mono", "identity"):
        rows = [(v, t, l) for l, m, v, t in REPORT if l.startswith(kind) and m.startswith("error")]
        if rows:
            v, t, l = max(rows, key=lambda r: r[0] / r[1])
            print(f"worst of '{kind}': {v:.3e} / {t:.3e} ({l})")
