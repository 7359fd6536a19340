"""cpe_solve_ragged on the GPU: sequences of their own length, rig and skeleton in one solve.  Every sequence's outputs and statistics are BIT-equal
to a cpe_solve of that sequence alone on a handle of its own model (include/cpe.h), and the padding reads 0.0."""
import os
import sys

import numpy as np
import pytest

from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

# the reference's four skeletons: 6-camera AcinoSet rigs at 120 fps, 4-camera kinetic-dataset rigs at 200 fps; every model its own rig
ANIMALS = (("phantom", False), ("jules", False), ("arabia-02", True), ("shiraz-02", True))
FIELDS = ("q", "dq", "ddq", "positions", "meas_err")
STATS = ("status", "iterations", "outer", "cost", "cost_meas", "cost_model", "cost_pose", "cost_motion", "lam", "max_constraint",
         "max_bound_violation")


def _models(n_cams=None):
    out = []
    for k, (animal, kin) in enumerate(ANIMALS):
        cams = synth.make_cameras(4 if kin else 6, seed=100 + k)
        if n_cams is not None:
            cams = (abi.Camera * n_cams)(*cams[:n_cams])
        out.append((skeleton.build_skeleton(animal, 24, kinetic_dataset=kin), cams, abi.default_options(200.0 if kin else 120.0), kin))
    return out


def _sequences(models, lengths, seed=40):
    """one synthetic sequence per length; sequence b uses model b mod len(models)"""
    seqs = []
    for b, N in enumerate(lengths):
        m = b % len(models)
        sk, cams, opts, kin = models[m]
        d = synth.make_batch(sk, cams, B=1, N=N, fps=1.0 / opts.h, seed=seed + b, kinetic_dataset=kin)
        seqs.append((m, d["q_init"][0], d["meas"][0], d["weight"][0]))
    return seqs


def _alone(models, seqs, pr=None):
    refs = []
    for m, qi, me, we in seqs:
        sk, cams, opts, _ = models[m]
        h = _lib.Handle(sk, cams, opts, pr)
        try:
            refs.append(h.solve_host(qi[None], me[None], we[None]))
        finally:
            h.close()
    return refs


def _assert_bit_equal(out, b, ref):
    for k in FIELDS:
        assert out[k][b].shape == ref[k][0].shape, (b, k)
        assert out[k][b].tobytes() == ref[k][0].tobytes(), (b, k)
    s, r = out["stats"][b], ref["stats"][0]
    for f in STATS:
        assert getattr(s, f) == getattr(r, f), (b, f, getattr(s, f), getattr(r, f))


def _assert_padding_zero(out, seqs, models):
    P = out["padded"]
    for b, (m, qi, _, _) in enumerate(seqs):
        n, c = qi.shape[0], len(models[m][1])
        for k in ("q", "dq", "ddq", "positions", "meas_err"):
            assert not P[k][b, n:].any(), (b, k)
        assert not P["meas_err"][b, :n, c:].any(), b


def _ragged(models, seqs, pr=None):
    h = _lib.Handle.multi([m[0] for m in models], [m[1] for m in models], [m[2] for m in models], pr)
    try:
        return h.solve_ragged_host([s[1] for s in seqs], [s[2] for s in seqs], [s[3] for s in seqs], [s[0] for s in seqs])
    finally:
        h.close()


def test_mixed_batch_is_bit_equal_to_solo_solves():
    models = _models()
    seqs = _sequences(models, [30, 36, 41, 44, 49, 52, 57, 33])
    out = _ragged(models, seqs)
    refs = _alone(models, seqs)
    for b in range(len(seqs)):
        _assert_bit_equal(out, b, refs[b])
    _assert_padding_zero(out, seqs, models)
    assert all(s.status == abi.OK for s in out["stats"])


@pytest.mark.parametrize("which", ["both-w4", "both-k3-w2-dense"])
def test_priors_batch_is_bit_equal_to_solo_solves(which):
    # learned priors on one camera per model: k_lm_step<4> with the window-4 motion prior, k_lm_step<3> + the LR band with the golden k3 / w2 set
    if which == "both-w4":
        pr = priors.load_priors()
        assert pr.lr_window == 4
    else:
        pr = priors.load_priors(path=os.path.join(os.path.dirname(__file__), "golden", "priors_k3_w2_dense.npz"))
        assert pr.gmm_k == 3 and pr.lr_window == 2
    models = _models(n_cams=1)
    seqs = _sequences(models, [30, 36, 41, 44, 49, 52, 57, 33], seed=60)
    out = _ragged(models, seqs, pr)
    refs = _alone(models, seqs, pr)
    for b in range(len(seqs)):
        _assert_bit_equal(out, b, refs[b])
    _assert_padding_zero(out, seqs, models)


def test_per_model_options_reach_the_kernels(oracle):
    """three models of one shape that differ in loss knots, bound_penalty and camera multipliers (include/cpe.h: these may differ per model), with
    outliers and a start outside an angle range: every sequence bit-equal to its solo solve on a handle of its own model, and a model-1
    sequence solved with model 0's options ends elsewhere"""
    sk = skeleton.build_skeleton("phantom", 24)
    models = []
    for knots, kappa, mult in (((3.0, 10.0, 20.0), 1e4, (1.0,) * 6), ((2.0, 6.0, 15.0), 3e3, (1.0, 1.0, 0.6, 0.6, 1.0, 0.8)),
                               ((1e6, 2e6, 3e6), 1e4, (0.9,) * 6)):
        cams = synth.make_cameras(6, seed=100)
        for c in range(6):
            cams[c].mult = mult[c]
        opts = abi.default_options()
        opts.loss_a, opts.loss_b, opts.loss_c = knots
        opts.bound_penalty = kappa
        models.append((sk, cams, opts, False))
    seqs = []
    for b, (m, n) in enumerate(((0, 9), (1, 7), (2, 9), (1, 5), (0, 8))):
        d = synth.make_batch(sk, models[m][1], B=1, N=n, seed=80 + b)                 # (10 % of the measurements are outliers)
        seqs.append((m, d["q_init"][0].copy(), d["meas"][0], d["weight"][0]))
    i_roll = next(i for i in range(sk.n_bounds) if sk.bound_a[i] == skeleton.dof("base", skeleton.PHI) and sk.bound_b[i] < 0)
    seqs[1][1][:, skeleton.dof("base", skeleton.PHI)] = sk.bound_up[i_roll] + 0.3     # the start of a model-1 sequence violates a bound
    m1, q1, me1, we1 = seqs[1]
    assert oracle.objective(sk, models[1][1], models[1][2], None, q1, me1, we1)[3][4] > 0.0
    assert len(seqs) == 5 and max(s[1].shape[0] for s in seqs) == 9
    out = _ragged(models, seqs)
    refs = _alone(models, seqs)
    for b in range(len(seqs)):
        _assert_bit_equal(out, b, refs[b])
    _assert_padding_zero(out, seqs, models)
    wrong = _alone(models, [(0, q1, me1, we1)])[0]                                    # the same sequence with model 0's knots, penalty and multipliers
    own, other = refs[1]["stats"][0].cost, wrong["stats"][0].cost
    assert out["stats"][1].cost == own and own != other and out["stats"][1].cost != other
    assert refs[1]["q"][0].tobytes() != wrong["q"][0].tobytes()


def test_short_sequences_next_to_a_long_one():
    # the degenerate band cases (no motion term below 4 frames, partial windows below 8) in one batch with N = 57
    models = _models()
    seqs = _sequences(models, [1, 2, 3, 4, 5, 9, 57], seed=7)
    out = _ragged(models, seqs)
    refs = _alone(models, seqs)
    for b in range(len(seqs)):
        _assert_bit_equal(out, b, refs[b])
    _assert_padding_zero(out, seqs, models)


def test_plain_handle_equal_lengths_and_permutation():
    # a cpe_create handle takes ragged calls too (one model): with equal lengths the call is cpe_solve's, and permuting the sequences permutes the outputs
    sk = skeleton.build_skeleton("phantom", 24)
    cams = synth.make_cameras(6)
    h = _lib.Handle(sk, cams, abi.default_options())
    try:
        d = synth.make_batch(sk, cams, B=5, N=30, seed=11)
        full = h.solve_host(d["q_init"], d["meas"], d["weight"])
        out = h.solve_ragged_host(list(d["q_init"]), list(d["meas"]), list(d["weight"]))
        for k in FIELDS:
            assert np.stack(out[k]).tobytes() == full[k].tobytes(), k
        for b in range(5):
            for f in STATS:
                assert getattr(out["stats"][b], f) == getattr(full["stats"][b], f), (b, f)
        perm = [3, 0, 4, 1, 2]
        outp = h.solve_ragged_host([d["q_init"][p] for p in perm], [d["meas"][p] for p in perm], [d["weight"][p] for p in perm])
        for i, p in enumerate(perm):
            for k in FIELDS:
                assert outp[k][i].tobytes() == out[k][p].tobytes(), (i, k)
            for f in STATS:
                assert getattr(outp["stats"][i], f) == getattr(out["stats"][p], f), (i, f)
    finally:
        h.close()


def _tree(root):
    """every file under root -> bytes (result pickles as their loaded dictionaries without the wall-clock field)"""
    from cheetah_pose_estimation_amd import estimator as E
    files = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            rel = os.path.relpath(p, root)
            if f.endswith(".pickle"):
                r = E.load_result_pickle(p)
                r.pop("processing_time_s", None)
                files[rel] = r
            else:
                with open(p, "rb") as fh:
                    files[rel] = fh.read()
    return files


def test_estimator_ragged_matches_grouped_batches(tmp_path):
    sys.path.insert(0, os.path.dirname(__file__))
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    specs = [("2019_03_07/synth/run1", 24, 5, 6), ("2019_03_09/synth/run2", 30, 6, 4), ("2019_03_07/synth/run3", 33, 7, 6),
             ("2019_03_09/synth/run4", 27, 8, 4)]
    roots = {k: str(tmp_path / k) for k in ("grouped", "ragged")}
    for root in roots.values():
        for path, N, seed, nc in specs:
            write_dataset(root, data_path=path, N=N, seed=seed, n_cams=nc)
    ests = {k: [E.init_trajectory(root_dir=root, data_path=p, cheetah_name="phantom", kinetic_dataset=False, solver_path="/unused/ipopt",
                                  kinematic_model=True) for p, _, _, _ in specs] for k, root in roots.items()}
    oks_g = E.estimate_kinematics_batch(ests["grouped"])
    oks_r = E.estimate_kinematics_batch(ests["ragged"], ragged=True)
    assert oks_g == oks_r == [True] * len(specs)
    for a, b in zip(ests["grouped"], ests["ragged"]):
        for k in FIELDS:
            assert a.result[k].tobytes() == b.result[k].tobytes(), k
        assert a.costs == b.costs
        assert a.com_pos.tobytes() == b.com_pos.tobytes()
    ta, tb = _tree(roots["grouped"]), _tree(roots["ragged"])
    assert ta.keys() == tb.keys()
    written = [k for k in ta if "fte_kinematic" in k]
    assert len(written) >= len(specs)
    for k in ta:
        if isinstance(ta[k], dict):
            assert ta[k].keys() == tb[k].keys(), k
            for key in ta[k]:
                x, y = ta[k][key], tb[k][key]
                assert (np.asarray(x).tobytes() == np.asarray(y).tobytes()) if isinstance(x, np.ndarray) else x == y, (k, key)
        else:
            assert ta[k] == tb[k], k
