"""Posterior covariance of batched and ragged physics-based solves on the GPU (cpe_covariance_kinetic_ragged, include/cpe.h; k_force_cov<true>): every
sequence of a ragged batch is BIT-equal to cpe_covariance_kinetic of that sequence alone on a plain handle of its own model, the padding reads 0, a
sequence without a factor leaves its neighbours' bits alone, and estimate_kinetics_batch(uncertainty=True) writes what estimate_kinetics writes.
The batch: tests/ragged_kinetic_cov_cases.py (four sequences, three models, 9 to 12 frames; positive definite at ridge 0, asserted on the CPU by
tests/test_ragged_kinetic_covariance_host.py).

Accuracy of the model that is not the handle's first (arabia-02, sequence 3), in the unit and by the two tolerances of
tests/test_gpu_kinetic_covariance.py, both made of reference numbers only: full path 10 x max(r, 2^-52 x scaled condition of the joint matrix),
kernel 10 x max(r, 2^-52 x scaled condition of H_ff) per node.  test_zz_report prints every measured value next to its tolerance.

Measured on an MI355X (test_zz_report), error / tolerance, sequence 3 at ridge 0: kernel (worst node) 1.6e-10 / 3.6e-10; full path Sigma
2.1e-7 / 7.3e-4, cov_f 9.0e-8 / 7.3e-4 (the reference's two routes disagree by 7.3e-5 on this input there, by 4.1e-5 with another numpy build: scaled condition of the joint matrix 2.4e10)."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import cov_compare as CC
import kinetic_cov_compare as KV
import ragged_kinetic_cov_cases as RC
from cheetah_pose_estimation_amd import _lib, abi

pytestmark = pytest.mark.gpu

KEYS = RC.KEYS
REPORT = []
_ALONE = {}


def _note(label, measure, value, tol):
    REPORT.append((label, measure, float(value), float(tol)))
    print(f"{label}: {measure} {value:.3e} (tolerance {tol:.3e})")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _alone(factory, c, ridge):
    """the plain entry on the case alone (B = 1) on a plain handle of its own model: one call per (case, ridge) and session, asserted CPE_OK"""
    key = (id(c), ridge)
    if key not in _ALONE:
        h = factory(c["sk"], c["cams"], c["opts"])
        out = h.covariance_kinetic_host(c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], c["ko"], ridge, want_L=True,
                                        **{k: v[None] for k, v in c["var"].items()})
        assert out["status"] == abi.OK and out["seq_status"] == [abi.OK], ridge
        assert all(out[k].any() for k in KEYS)
        _ALONE[key] = (c, out)                                  # (the case is kept: its id is the key)
    return _ALONE[key][1]


@pytest.fixture(scope="module")
def batch(oracle):
    """(the handle over the three models, their kinetic options in model order, the four sequences)"""
    ms = RC.models(oracle)
    h = _lib.Handle.multi([m["sk"] for m in ms], [m["cams"] for m in ms], [m["opts"] for m in ms])
    yield h, [m["ko"] for m in ms], RC.sequences(oracle)
    h.close()


def _ragged(h, kos, seqs, model_of, ridge, variant=None):
    args, kw = RC.ragged_args(seqs, model_of, variant)
    return h.covariance_kinetic_ragged_host(*args, kos, ridge=ridge, want_L=True, **kw)


def _assert_sequence(out, b, alone, what=""):
    for k in KEYS:
        assert _bits(out[k][b], alone[k][0]), (what, b, k)


def _assert_padding_zero(out, seqs):
    for b, c in enumerate(seqs):
        n = c["q"].shape[0]
        for k in KEYS:
            assert not out["padded"][k][b, n:].any(), (b, k)


# ---- 1. bit-equality -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
def test_every_sequence_is_bit_equal_to_its_own_call(oracle, gpu_handle_factory, batch, ridge):
    """four sequences, three models, lengths 12 / 12 / 9 / 10: every output of every sequence, byte for byte; the padding zero; in another order;
    twice"""
    h, kos, seqs = batch
    alone = [_alone(gpu_handle_factory, c, ridge) for c in seqs]
    out = _ragged(h, kos, seqs, RC.SEQ_MODEL, ridge)
    assert out["status"] == abi.OK and out["seq_status"] == [abi.OK] * 4
    assert [out["cov_f"][b].shape[0] for b in range(4)] == list(RC.SEQ_FRAMES)
    for b in range(4):
        _assert_sequence(out, b, alone[b], f"ridge {ridge:g}")
    _assert_padding_zero(out, seqs)
    assert not _bits(out["cov_f"][0][:9], out["cov_f"][2]) and not _bits(out["cov_f"][0][:10], out["cov_f"][3])
    again = _ragged(h, kos, seqs, RC.SEQ_MODEL, ridge)
    assert again["seq_status"] == [abi.OK] * 4 and all(_bits(out["padded"][k], again["padded"][k]) for k in KEYS)
    order = [3, 1, 0, 2]
    perm = _ragged(h, kos, [seqs[i] for i in order], [RC.SEQ_MODEL[i] for i in order], ridge)
    assert perm["seq_status"] == [abi.OK] * 4
    for b, i in enumerate(order):
        _assert_sequence(perm, b, alone[i], f"ridge {ridge:g}, order {order}")
    _assert_padding_zero(perm, [seqs[i] for i in order])


def test_device_pointer_entry_gives_the_host_twin_bits(batch):
    """cpe_covariance_kinetic_ragged on device tensors against the host twin; without cov_off (the entry's own buffer) the other outputs keep their
    bits"""
    import torch
    h, kos, seqs = batch
    ref = _ragged(h, kos, seqs, RC.SEQ_MODEL, 0.0)["padded"]
    p = _lib.pad_kinetic([c["q"] for c in seqs], [c["meas"] for c in seqs], [c["weight"] for c in seqs], [c["stance"] for c in seqs], n_cams_max=h.n_cams)
    dev = torch.device("cuda", 0)
    T = lambda x, dt=torch.float64: torch.tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    ins = (T(p["q_init"]), T(p["meas"]), T(p["weight"]), T(p["stance"], torch.int32))
    for without in ((), ("cov_off",)):
        o = {k: torch.full(ref[k].shape, 7, dtype=torch.int32 if k == "meta" else torch.float64, device=dev) for k in KEYS if k not in without}
        st, seq = h.covariance_kinetic_ragged(kos, RC.SEQ_MODEL, RC.SEQ_FRAMES, *ins, 0.0, **o)
        h.synchronize()
        assert st == abi.OK and seq == [abi.OK] * 4
        assert all(_bits(o[k].cpu().numpy(), ref[k]) for k in o), without


# ---- 2. accuracy of the model that is not the handle's first -----------------------------------------------------------------------------------------
def _window_cov(diag, off, n):
    """W [84][84] of node n from the band the call returned: frames (n, n-1, n-2); off[f][k-1] = Sigma(f + k, f)"""
    W = np.zeros((84, 84))
    for a in range(3):
        for b in range(3):
            blk = diag[n - a] if a == b else (off[n - b, b - a - 1] if a < b else off[n - a, a - b - 1].T)
            W[28 * a:28 * a + 28, 28 * b:28 * b + 28] = blk
    return W


def test_accuracy_of_the_arabia_sequence(oracle, gpu_handle_factory, batch):
    """sequence 3 (another skeleton, DevKin, kinetic options and length than the handle's first model) of the ragged call at ridge 0: Sigma and cov_f
    against the joint route on oracle.kinetic_system (kinetic_cov_compare.reference and its tolerance), and cov_f of every node against the local
    formula from the HIP path's own H_fu / H_ff / meta and the call's own Sigma (kinetic_cov_compare.kernel_tolerance)"""
    h, kos, seqs = batch
    c = seqs[3]
    out = _ragged(h, kos, seqs, RC.SEQ_MODEL, 0.0)
    assert out["seq_status"][3] == abi.OK
    diag, off, cf, meta = out["cov_diag"][3], out["cov_off"][3], out["cov_f"][3], out["meta"][3]
    R, Ad, Hk, nodes = KV.oracle_system(oracle, c, 0.0)
    ref = KV.reference(Ad, Hk, nodes)
    assert np.array_equal(meta[:, 0], R["meta"][:, 0]) and set(meta[2:, 0]) == {48, 51}
    eu = CC.scaled_error(diag, off, ref["diag"], ref["off"])
    ef = KV.force_error(cf, ref["cov_f"])
    _note("full path arabia-02 (ragged, sequence 3) ridge 0", "Sigma error", eu, ref["tol"])
    _note("full path arabia-02 (ragged, sequence 3) ridge 0", "cov_f error", ef, ref["tol"])
    # the kernel's formula per node, from the HIP path's own pieces on a plain handle of the model
    hp = gpu_handle_factory(c["sk"], c["cams"], c["opts"])
    G = hp.eval_kinetic_system_host(c["ko"], c["q"][None], c["meas"][None], c["weight"][None], c["stance"][None], band=False)
    worst, seen = (0.0, 1.0), set()
    fails = []
    for n, (Hfu, M) in KV.node_blocks({k: G[k][0] for k in ("Hfu", "Hff", "meta")}).items():
        na = M.shape[0]
        seen.add(na)
        kref, tol, r, cond = KV.kernel_tolerance(Hfu, M, _window_cov(diag, off, n))
        err = KV.scaled_difference(cf[n, :na, :na], kref)
        if err / tol >= worst[0] / worst[1]:
            worst = (err, tol)
        if not err <= tol:
            fails.append((n, na, err, tol, r, cond))
    _note("kernel arabia-02 (ragged, sequence 3)", "kernel error", *worst)
    assert eu <= ref["tol"], (eu, ref["tol"])
    assert ef <= ref["tol"], (ef, ref["tol"])
    assert not fails, fails
    assert seen == {48, 51}


# ---- 3. variants ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["grf_fixed", "tau_box"])
def test_variants_are_bit_equal_to_their_own_calls(oracle, gpu_handle_factory, batch, variant):
    """per-sequence grf_fixed (each solution's own net foot forces) and tau_box (bound_value(0.5 tau, 0.1)), padded to N_max by the host method"""
    h, kos, seqs = batch
    vs = [RC.with_variant(c, variant) for c in seqs]
    out = _ragged(h, kos, vs, RC.SEQ_MODEL, 0.0, variant)
    assert out["seq_status"] == [abi.OK] * 4
    for b, c in enumerate(vs):
        _assert_sequence(out, b, _alone(gpu_handle_factory, c, 0.0), variant)
        assert not _bits(out["cov_f"][b], _alone(gpu_handle_factory, seqs[b], 0.0)["cov_f"][0])      # (the variant is not the free problem)
    _assert_padding_zero(out, vs)
    if variant == "grf_fixed":
        for b, c in enumerate(vs):
            assert np.all(out["meta"][b][2:, 0] == c["ko"].dyn.n_motors + 26) and not out["meta"][b][:2].any()


# ---- 4. failure isolation -------------------------------------------------------------------------------------------------------------------------
def test_a_failed_sequence_does_not_disturb_its_neighbours(oracle, gpu_handle_factory, batch):
    """sequence 0 with every weight zero (the band is singular), sequence 2 with one NaN measurement under a positive weight (the evaluation is not
    finite): [NUMERICAL, OK, NUMERICAL, OK], the call returns CPE_NUMERICAL, every output of the failed ones zero -- what the band kernels had
    written included -- and the other two keep the bits of their own calls"""
    h, kos, seqs = batch
    bad = [dict(c) for c in seqs]
    bad[0]["weight"] = np.zeros_like(seqs[0]["weight"])
    me = seqs[2]["meas"].copy()
    l = int(np.argmax(seqs[2]["weight"][5, 0] > 0.0))
    assert seqs[2]["weight"][5, 0, l] > 0.0
    me[5, 0, l, 0] = np.nan
    bad[2]["meas"] = me
    out = _ragged(h, kos, bad, RC.SEQ_MODEL, 0.0)
    assert out["seq_status"] == [abi.NUMERICAL, abi.OK, abi.NUMERICAL, abi.OK] and out["status"] == abi.NUMERICAL
    for b in (0, 2):
        assert not any(out["padded"][k][b].any() for k in KEYS), b
    for b in (1, 3):
        _assert_sequence(out, b, _alone(gpu_handle_factory, seqs[b], 0.0), "beside failed sequences")
    _assert_padding_zero(out, bad)


# ---- 5. edge length ---------------------------------------------------------------------------------------------------------------------------------
def test_three_frames_beside_twelve(oracle, gpu_handle_factory, batch):
    """a member of 3 frames (one node, whose window starts at the sequence's first frame) beside one of 12, at ridge 1e-3 (three frames do not
    determine every coordinate at ridge 0; the damping of test_gpu_kinetic_covariance.py::test_edge_lengths)"""
    h, kos, seqs = batch
    short, long_ = RC.cut(seqs[0], 3), seqs[0]
    out = _ragged(h, kos, [short, long_], [0, 0], 1e-3)
    assert out["seq_status"] == [abi.OK, abi.OK] and out["status"] == abi.OK
    meta, cf = out["meta"][0], out["cov_f"][0]
    assert meta.shape[0] == 3 and cf.shape[0] == 3
    assert not meta[:2].any() and meta[2, 0] in (51, 54)          # one node
    assert not cf[:2].any()
    na = meta[2, 0]
    assert np.all(np.diag(cf[2])[:na] > 0.0) and _bits(cf[2], cf[2].T) and not cf[2][na:].any()
    _assert_padding_zero(out, [short, long_])
    _assert_sequence(out, 1, _alone(gpu_handle_factory, long_, 1e-3), "12 frames beside 3")
    _assert_sequence(out, 0, _alone(gpu_handle_factory, short, 1e-3), "3 frames beside 12")


# ---- 6. refusals on a handle ------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_handle(oracle, batch):
    from cheetah_pose_estimation_amd import priors, skeleton
    h, kos, seqs = batch
    bad = abi.KineticOptions(); C.memmove(C.byref(bad), C.byref(kos[2]), C.sizeof(abi.KineticOptions))
    bad.dyn.n_motors -= 1
    args, kw = RC.ragged_args(seqs, RC.SEQ_MODEL)
    with pytest.raises(_lib.CpeError, match=r"cpe_covariance_kinetic_ragged_host: kinetic options of model 2 differ from model 0 in dyn\.n_motors"):
        h.covariance_kinetic_ragged_host(*args, [kos[0], kos[1], bad], **kw)
    bad = abi.KineticOptions(); C.memmove(C.byref(bad), C.byref(kos[1]), C.sizeof(abi.KineticOptions))
    bad.dyn.motor_axis[3] = (bad.dyn.motor_axis[3] + 1) % 3
    with pytest.raises(_lib.CpeError, match=r"model 1 differ from model 0 in dyn\.motor_axis"):
        h.covariance_kinetic_ragged_host(*args, [kos[0], bad, kos[2]], **kw)
    c = seqs[0]
    h4 = _lib.Handle.multi([skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24))], [c["cams"]], [c["opts"]], priors.load_priors())
    try:
        assert h4.pb == 4
        with pytest.raises(_lib.CpeError, match="half-bandwidth 4"):
            h4.covariance_kinetic_ragged_host([c["q"]], [c["meas"]], [c["weight"]], [c["stance"]], [c["ko"]])
    finally:
        h4.close()


# ---- 7. the estimator, through files -------------------------------------------------------------------------------------------------------------------
UNC_FIELDS = ("cov_u", "u_std", "positions_cov", "positions_std", "ridge", "tau_std", "lambda_std", "grf_std", "tau_cov")
SETS = ((24, 6, 5), (24, 6, 6), (18, 4, 7), (24, 6, 8))        # (frames, cameras, seed): the 6-camera ones share a rig
BLIND = 3                                                      # the sequence whose weights test 7b zeroes; the batches of test 7a are the first three
KW = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True)


def _same_pickle(a, b, where=""):
    if isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            if k != "processing_time_s":
                _same_pickle(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert _bits(a, b), where
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same_pickle(x, y, f"{where}[{i}]")
    else:
        assert a == b, where


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """four sequences on disk with their kinematic results, and fresh(prefix, which): physics-stage estimators whose outputs (and whose copy of the
    kinematic result they start from) go under an output prefix of their own"""
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    tmp = tmp_path_factory.mktemp("ragged_kinetic_cov")
    sets = []
    for k, (N, n_cams, seed) in enumerate(SETS):
        root = str(tmp / f"set{k}")
        info = write_dataset(root, data_path=f"2019_03_07/synth/run{k}", N=N, noise_px=0.5, gallop=True, seed=seed, n_cams=n_cams)
        est = E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
        assert E.estimate_kinematics(est, solver_output=False) is True
        sets.append((root, info["data_path"]))

    def fresh(prefix, which=range(3)):
        ests = []
        for k in which:
            root, dp = sets[k]
            dst = os.path.join(prefix, dp, "fte_kinematic")
            if not os.path.exists(dst):
                shutil.copytree(os.path.join(root, dp, "fte_kinematic"), dst)
            ests.append(E.init_trajectory(root, dp, "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True, bound_eom_error=(-2.0, 2.0),
                                          include_camera_constraints=True, kinematic_model=False))
        return ests
    return str(tmp), sets, fresh


def _out_dir(prefix, dp):
    return os.path.join(prefix, dp, "fte_kinetic")


def test_estimator_batches_write_what_the_single_call_writes(datasets):
    """estimate_kinetics_batch(uncertainty=True), ragged=False (one group of two sequences sharing a rig and a length, one of one) and ragged=True (one
    group, two models): every sequence's uncertainty.npz and est.uncertainty bit-equal to those of its own estimate_kinetics(uncertainty=True); the
    arrays of fte.pickle those of the batch without uncertainty; no file more than uncertainty.npz; none without uncertainty"""
    from cheetah_pose_estimation_amd import estimator as E
    tmp, sets, fresh = datasets
    P = lambda name: os.path.join(tmp, "out_" + name)
    solo = fresh(P("solo"))
    assert all(E.estimate_kinetics(e, uncertainty=True, out_dir_prefix=P("solo"), **KW) is True for e in solo)
    runs = {}
    for name, ragged, unc in (("plain_off", False, False), ("plain", False, True), ("ragged_off", True, False), ("ragged", True, True)):
        ests = fresh(P(name))
        assert E.estimate_kinetics_batch(ests, ragged=ragged, uncertainty=unc, out_dir_prefix=P(name), **KW) == [True] * 3
        runs[name] = ests
    for k, (root, dp) in enumerate(sets[:3]):
        N = SETS[k][0]
        zs = np.load(os.path.join(_out_dir(P("solo"), dp), "uncertainty.npz"))
        assert sorted(zs.files) == sorted(UNC_FIELDS) and zs["cov_u"].shape == (N, 28, 28) and zs["tau_cov"].shape == (N, 22, 22)
        assert np.all(zs["tau_std"][2:] > 0.0) and np.all(zs["u_std"] > 0.0)
        for name in ("plain", "ragged"):
            d, off = _out_dir(P(name), dp), _out_dir(P(name + "_off"), dp)
            z = np.load(os.path.join(d, "uncertainty.npz"))
            assert sorted(z.files) == sorted(UNC_FIELDS)
            unc = runs[name][k].uncertainty
            assert sorted(unc) == sorted(UNC_FIELDS)
            for key in UNC_FIELDS:
                assert _bits(z[key], zs[key]), (name, k, key)
                assert _bits(np.asarray(unc[key]), np.asarray(solo[k].uncertainty[key])), (name, k, key)
            _same_pickle(E.load_result_pickle(os.path.join(d, "fte.pickle")), E.load_result_pickle(os.path.join(off, "fte.pickle")), f"{name}/{k}")
            assert sorted(f for f in os.listdir(d) if f != "uncertainty.npz") == sorted(os.listdir(off))
            assert "uncertainty.npz" not in os.listdir(off) and runs[name + "_off"][k].uncertainty is None


@pytest.mark.parametrize("ragged", [False, True])
def test_estimator_batch_finishes_every_sequence_before_it_raises(datasets, monkeypatch, ragged):
    """a fourth sequence that no camera sees (every weight zero) beside the three: its solve converges, its band is singular (the covariance status is
    CPE_NUMERICAL; its own estimate_kinetics(uncertainty=True) raises CpeError after its files).  In the batch the others' files are complete -- their
    uncertainty.npz bit-equal to the batch without that sequence -- its own solve's files are written, the group still makes ONE covariance call, and
    only then ONE CpeError names it, with the hint about uncertainty_ridge"""
    from cheetah_pose_estimation_amd import estimator as E
    tmp, sets, fresh = datasets
    prefix = os.path.join(tmp, "out_failed_ragged" if ragged else "out_failed_plain")
    method = "covariance_kinetic_ragged_host" if ragged else "covariance_kinetic_host"
    real = getattr(_lib.Handle, method)
    calls = []

    def counted(self, *a, **kw):
        r = real(self, *a, **kw)
        calls.append(list(r["seq_status"]))
        return r
    monkeypatch.setattr(_lib.Handle, method, counted)
    ests = fresh(prefix, range(4))
    ests[BLIND].weight[:] = 0.0
    with pytest.raises(_lib.CpeError, match=r"uncertainty_ridge.*\(no uncertainty for: phantom 2019_03_07/synth/run3\)$"):
        E.estimate_kinetics_batch(ests, ragged=ragged, uncertainty=True, out_dir_prefix=prefix, **KW)
    # ONE call per group: ragged, all four; else the three of the 6-camera rig with 24 frames, and the 4-camera one
    assert calls == ([[abi.OK, abi.OK, abi.OK, abi.NUMERICAL]] if ragged else [[abi.OK, abi.OK, abi.NUMERICAL], [abi.OK]])
    ref = os.path.join(tmp, "out_ragged" if ragged else "out_plain")
    for k, (root, dp) in enumerate(sets):
        d = _out_dir(prefix, dp)
        assert os.path.exists(os.path.join(d, "fte.pickle")) and ests[k].result["stats"][0].status == abi.OK
        if k == BLIND:
            assert ests[k].uncertainty is None and "uncertainty.npz" not in os.listdir(d)
        else:
            assert ests[k].uncertainty is not None
            z = np.load(os.path.join(d, "uncertainty.npz"))
            assert sorted(z.files) == sorted(UNC_FIELDS) and np.all(z["u_std"] > 0.0)
            if os.path.exists(os.path.join(_out_dir(ref, dp), "uncertainty.npz")):               # (written by the test above, when it has run)
                zr = np.load(os.path.join(_out_dir(ref, dp), "uncertainty.npz"))
                assert all(_bits(z[key], zr[key]) for key in UNC_FIELDS), k
    # alone, the same sequence raises after its own files
    solo = fresh(os.path.join(tmp, "out_failed_solo"), [BLIND])[0]
    solo.weight[:] = 0.0
    with pytest.raises(_lib.CpeError, match="uncertainty_ridge"):
        E.estimate_kinetics(solo, uncertainty=True, out_dir_prefix=os.path.join(tmp, "out_failed_solo"), **KW)
    assert os.path.exists(os.path.join(_out_dir(os.path.join(tmp, "out_failed_solo"), sets[BLIND][1]), "fte.pickle"))


def test_zz_report():
    """every measured error next to the tolerance applied to it"""
    for label, measure, value, tol in REPORT:
        print(f"{label:55s} {measure:15s} {value:.3e}   tolerance {tol:.3e}")
