"""cpe_solve_kinetic_ragged on the GPU: physics-based solves of sequences of their own length, rig, skeleton and kinetic options in one call.
Every sequence's outputs, cpe_stats and cpe_kinetic_stats are BIT-equal to a cpe_solve_kinetic* of that sequence alone on a handle of its own
model (include/cpe.h), and the padding reads 0.0.  max_iter is capped: bit-equality does not need convergence."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

# phantom 6 cameras / 120 fps, jules 6 cameras / 90 fps, the kinetic dataset's two cheetahs 4 cameras / 200 fps with its options
ANIMALS = (("phantom", 120.0, False), ("jules", 90.0, False), ("arabia-02", 200.0, True), ("shiraz-02", 200.0, True))
FIELDS = ("q", "dq", "ddq", "positions", "meas_err", "tau", "lam", "grf", "slack")
STATS = [f for f, _ in abi.Stats._fields_]
KSTATS = [f for f, _ in abi.KineticStats._fields_]
MAX_ITER = 150


def _models(n_cams=None, max_iter=MAX_ITER):
    out = []
    for k, (animal, fps, kin) in enumerate(ANIMALS):
        cams = synth.make_cameras(4 if kin else 6, seed=200 + k)
        if n_cams is not None:
            cams = (abi.Camera * n_cams)(*cams[:n_cams])
        sk = skeleton.without_motion_model(skeleton.build_skeleton(animal, 24, kinetic_dataset=kin))
        opts = abi.default_options(fps)
        opts.tol_cost, opts.max_iter = 1e-6, max_iter
        ko = abi.default_kinetic_options(skeleton.dyn_options(animal), fps, kin)
        if kin:
            assert ko.zvel_max == 1.0 and ko.foot_height_tol == 0.03
            ko.slack_lo, ko.slack_hi = -2.0, 2.0
        out.append(dict(sk=sk, cams=cams, opts=opts, ko=ko, fps=fps, kin=kin))
    return out


def _force(variant, N, stance, nm, seed):
    """a per-sequence force array of the variant (None for free forces)"""
    rng = np.random.default_rng(seed)
    if variant == "grf_fixed":
        f = np.zeros((N, 4, 3)); f[..., 0] = 0.5 * stance; f[..., 1] = 0.05 * stance * rng.standard_normal((N, 4))
        return f
    if variant == "tau_box":
        c = 0.1 * rng.standard_normal((N, nm))
        return np.stack([c - 0.3, c + 0.3], axis=-1)
    if variant == "grf_box":
        z = 0.5 * stance
        b = np.zeros((N, 4, 3, 2)); b[..., 0, 0], b[..., 0, 1] = 0.8 * z, 1.2 * z; b[..., 1:, 0], b[..., 1:, 1] = -0.1, 0.1
        return b
    return None


def _sequences(models, lengths, seed=60, variant=None, model_of=None):
    seqs = []
    for b, N in enumerate(lengths):
        m = b % len(models) if model_of is None else model_of[b]
        md = models[m]
        d = synth.make_gallop_batch(md["sk"], md["cams"], B=1, N=N, fps=md["fps"], seed=seed + b, kinetic_dataset=md["kin"], stance_frames=6)
        seqs.append(dict(m=m, q_init=d["q_init"][0], meas=d["meas"][0], weight=d["weight"][0], stance=d["stance"][0],
                         force=_force(variant, N, d["stance"][0], md["ko"].dyn.n_motors, seed + 1000 + b)))
    return seqs


def _alone(models, seqs, variant=None, pr=None):
    refs = []
    for s in seqs:
        md = models[s["m"]]
        h = _lib.Handle(md["sk"], md["cams"], md["opts"], pr)
        try:
            kw = {} if variant is None else {variant: s["force"][None]}
            refs.append(h.solve_kinetic_host(md["ko"], s["q_init"][None], s["meas"][None], s["weight"][None], s["stance"][None], **kw))
        finally:
            h.close()
    return refs


def _ragged(h, models, seqs, variant=None):
    kw = {} if variant is None else {variant: [s["force"] for s in seqs]}
    return h.solve_kinetic_ragged_host([md["ko"] for md in models], [s["q_init"] for s in seqs], [s["meas"] for s in seqs], [s["weight"] for s in seqs],
                                       [s["stance"] for s in seqs], [s["m"] for s in seqs], **kw)


def _multi(models, pr=None):
    return _lib.Handle.multi([md["sk"] for md in models], [md["cams"] for md in models], [md["opts"] for md in models], pr)


def _assert_bit_equal(out, b, ref, rb=0):
    for k in FIELDS:
        assert out[k][b].shape == ref[k][rb].shape, (b, k)
        assert out[k][b].tobytes() == ref[k][rb].tobytes(), (b, k, np.abs(out[k][b] - ref[k][rb]).max())
    s, r = out["stats"][b], ref["stats"][rb]
    for f in STATS:
        assert getattr(s, f) == getattr(r, f), (b, f, getattr(s, f), getattr(r, f))
    s, r = out["kstats"][b], ref["kstats"][rb]
    for f in KSTATS:
        assert getattr(s, f) == getattr(r, f), (b, f, getattr(s, f), getattr(r, f))


def _assert_padding_zero(out, seqs, models):
    P = out["padded"]
    for b, s in enumerate(seqs):
        n, c = s["q_init"].shape[0], len(models[s["m"]]["cams"])
        for k in FIELDS:
            assert not P[k][b, n:].any(), (b, k)
        assert not P["meas_err"][b, :n, c:].any(), b


def _check_batch(models, seqs, variant=None, pr=None):
    refs = _alone(models, seqs, variant, pr)
    h = _multi(models, pr)
    try:
        out = _ragged(h, models, seqs, variant)
    finally:
        h.close()
    for b in range(len(seqs)):
        _assert_bit_equal(out, b, refs[b])
    _assert_padding_zero(out, seqs, models)
    return out, refs


def test_mixed_batch_is_bit_equal_to_solo_solves():
    models = _models()
    lengths = [3, 11, 20, 27, 34, 41, 48, 15]                # every length different, from the shortest with a node (frame 2) up
    seqs = _sequences(models, lengths)
    out, refs = _check_batch(models, seqs)
    assert sum(r["stats"][0].iterations for r in refs) > 8 * 5              # real solves, not a cold exit
    assert {s["m"] for s in seqs} == {0, 1, 2, 3}


@pytest.mark.parametrize("variant", ["grf_fixed", "tau_box", "grf_box"])
def test_each_variant_is_bit_equal_to_solo_solves(variant):
    models = _models()
    seqs = _sequences(models, [22, 9, 37, 30, 16], seed=80, variant=variant)
    _check_batch(models, seqs, variant)


def test_monocular_with_pose_prior():
    models = _models(n_cams=1)
    pr = priors.load_priors(pose=True, motion=False)
    seqs = _sequences(models, [18, 25, 12, 31], seed=120)
    _check_batch(models, seqs, None, pr)


def test_plain_handle_ragged_lengths_in_any_order():
    models = _models()[:1]
    seqs = _sequences(models, [20, 9, 33], seed=140)
    refs = _alone(models, seqs)
    md = models[0]
    h = _lib.Handle(md["sk"], md["cams"], md["opts"])
    try:
        for order in ([0, 1, 2], [2, 0, 1]):
            out = _ragged(h, models, [seqs[i] for i in order])
            for b, i in enumerate(order):
                _assert_bit_equal(out, b, refs[i])
            _assert_padding_zero(out, [seqs[i] for i in order], models)
    finally:
        h.close()


def test_slot_reuse_matches_plain_batched_solves():
    """more sequences than the active window (2 per CU), so slots are handed on; the references are plain batched solves per (model, N)"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    models = _models(max_iter=30)
    per = (2 * n_cu) // 8 + 3                                 # sequences per (model, length) group: 8 groups together exceed the window
    groups = [(m, N) for m in range(4) for N in (5, 7)]
    seqs, refs = [], []
    for g, (m, N) in enumerate(groups):
        md = models[m]
        d = synth.make_gallop_batch(md["sk"], md["cams"], B=per, N=N, fps=md["fps"], seed=300 + 17 * g, kinetic_dataset=md["kin"], stance_frames=3)
        h = _lib.Handle(md["sk"], md["cams"], md["opts"])
        try:
            refs.append(h.solve_kinetic_host(md["ko"], d["q_init"], d["meas"], d["weight"], d["stance"]))
        finally:
            h.close()
        for b in range(per):
            seqs.append(dict(m=m, q_init=d["q_init"][b], meas=d["meas"][b], weight=d["weight"][b], stance=d["stance"][b], force=None, g=g, b=b))
    assert len(seqs) > 2 * n_cu
    perm = np.random.default_rng(7).permutation(len(seqs))     # interleave the groups
    seqs = [seqs[i] for i in perm]
    h = _multi(models)
    try:
        out = _ragged(h, models, seqs)
    finally:
        h.close()
    for b, s in enumerate(seqs):
        _assert_bit_equal(out, b, refs[s["g"]], s["b"])
    _assert_padding_zero(out, seqs, models)


def test_refusals():
    models = _models()
    seqs = _sequences(models, [8, 10], seed=160)
    h = _multi(models)
    try:
        kos = [md["ko"] for md in models]
        bad = abi.KineticOptions(); C.memmove(C.byref(bad), C.byref(kos[2]), C.sizeof(abi.KineticOptions))
        bad.dyn.n_motors -= 1
        with pytest.raises(_lib.CpeError, match=r"model 2.*dyn\.n_motors"):
            h.solve_kinetic_ragged_host(kos[:2] + [bad] + kos[3:], [s["q_init"] for s in seqs], [s["meas"] for s in seqs], [s["weight"] for s in seqs],
                                        [s["stance"] for s in seqs], [s["m"] for s in seqs])
        bad = abi.KineticOptions(); C.memmove(C.byref(bad), C.byref(kos[1]), C.sizeof(abi.KineticOptions))
        bad.dyn.motor_axis[3] = (bad.dyn.motor_axis[3] + 1) % 3
        with pytest.raises(_lib.CpeError, match=r"model 1.*dyn\.motor_axis"):
            h.solve_kinetic_ragged_host([kos[0], bad] + kos[2:], [s["q_init"] for s in seqs], [s["meas"] for s in seqs], [s["weight"] for s in seqs],
                                        [s["stance"] for s in seqs], [s["m"] for s in seqs])
        # the C entry point itself refuses two force arrays
        lib = _lib.load()
        B, N = 1, 8
        z = np.zeros(B * N * 4 * 6 * 24 * 4)
        st = np.zeros(B * N * 4, np.int32)
        ko = (abi.KineticOptions * 4)(*kos)
        mo, nf = (C.c_int32 * 1)(0), (C.c_int32 * 1)(N)
        stats, ks = (abi.Stats * 1)(), (abi.KineticStats * 1)()
        p = z.ctypes.data
        s = lib.cpe_solve_kinetic_ragged_host(h._h, ko, B, N, mo, nf, p, p, p, st.ctypes.data, p, p, None, *([np.zeros_like(z).ctypes.data] * 9), stats, ks)
        assert s == abi.BAD_ARG and b"at most one" in lib.cpe_last_error()
        # a skeleton with a motion model is refused, as by the plain path
        with pytest.raises(_lib.CpeError, match="motion_w"):
            hm = _lib.Handle.multi([skeleton.build_skeleton("phantom", 24)], [models[0]["cams"]], [models[0]["opts"]])
            try:
                s0 = seqs[0]
                hm.solve_kinetic_ragged_host([kos[0]], [s0["q_init"]], [s0["meas"]], [s0["weight"]], [s0["stance"]])
            finally:
                hm.close()
    finally:
        h.close()


def _load(path):
    from cheetah_pose_estimation_amd import estimator as E
    return E.load_result_pickle(path)


def _assert_same_output(a, b, where=""):
    if isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            if k != "processing_time_s":
                _assert_same_output(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), where
    else:
        assert a == b, where


def test_estimate_kinetics_batch_writes_what_estimate_kinetics_writes(tmp_path):
    """two sequences of different lengths through files (as test_estimate_kinetics_end_to_end_from_files builds them): estimate_kinetics on each,
    then estimate_kinetics_batch(ragged=True) and (ragged=False); every array of every fte.pickle is the same"""
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    ests = []
    for k, N in enumerate((36, 44)):
        root = str(tmp_path / f"set{k}")
        info = write_dataset(root, N=N, noise_px=0.5, gallop=True, seed=5 + k)
        est = E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
        assert E.estimate_kinematics(est, solver_output=False) is True
        ests.append((root, info))
    kw = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True)

    def fresh():
        return [E.init_trajectory(root, info["data_path"], "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True,
                                  bound_eom_error=(-2.0, 2.0), include_camera_constraints=True, kinematic_model=False) for root, info in ests]
    solo = [E.estimate_kinetics(e, out_fname="fte_solo", **kw) for e in fresh()]
    rag = E.estimate_kinetics_batch(fresh(), out_fname="fte_ragged", ragged=True, **kw)
    bat = E.estimate_kinetics_batch(fresh(), out_fname="fte_batched", ragged=False, **kw)
    assert solo == rag == bat and all(solo)
    for root, info in ests:
        d = os.path.join(root, info["data_path"], "fte_kinetic")
        a = _load(os.path.join(d, "fte_solo.pickle"))
        assert a["q"].shape[0] in (36, 44)
        _assert_same_output(a, _load(os.path.join(d, "fte_ragged.pickle")))
        _assert_same_output(a, _load(os.path.join(d, "fte_batched.pickle")))
