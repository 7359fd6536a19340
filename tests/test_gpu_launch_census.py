"""The launch census of a solve: the plain and the ragged form of one batch enqueue the same kernels the same number of times.  The same
B = 2 full-length sequences go through a plain handle (cpe_solve*_host) and through a cpe_create_multi handle of that one model
(cpe_solve*_ragged_host) with the per-kernel profile on: the profile slots and their launch counts agree (counts only, never milliseconds) and the
outputs are byte-equal.  The host's iteration functions (lm_iterate, kin_iterate in cpe_api.hip) have one body for both forms; this pins that a
launch is neither dropped nor doubled in one of them."""
import numpy as np
import pytest

from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

KINEMATIC = ("q", "dq", "ddq", "positions", "meas_err")


def _census(h, solve):
    h.profile(True)
    out = solve(h)
    return out, {k: n for k, (_, n) in h.profile_totals().items()}


def _compare(plain, multi, solve_plain, solve_ragged, fields, expect):
    try:
        full, n_plain = _census(plain, solve_plain)
        out, n_ragged = _census(multi, solve_ragged)
    finally:
        plain.close()
        multi.close()
    print("launches, plain: ", n_plain)
    print("launches, ragged:", n_ragged)
    assert set(expect) <= set(n_plain), (expect, n_plain)          # the case runs the kernels it is meant to
    assert all(n > 0 for n in n_plain.values())
    assert n_plain == n_ragged
    for k in fields:
        assert np.stack(out[k]).tobytes() == full[k].tobytes(), k
    assert [s.iterations for s in out["stats"]] == [s.iterations for s in full["stats"]]


@pytest.mark.parametrize("motion_prior", [False, True])
def test_kinematic_solve_census(motion_prior):
    # without priors: k_frame_normal, k_lm_step<3>, k_lm_back<3>; with the window-4 motion prior k_lr_band and the PB = 4 instantiations
    pr = priors.load_priors(pose=False, motion=True) if motion_prior else None
    assert pr is None or (pr.lr_window == 4 and pr.gmm_k == 0)
    sk, cams, opts = skeleton.build_skeleton("phantom", 24), synth.make_cameras(6), abi.default_options()
    d = synth.make_batch(sk, cams, B=2, N=12, seed=21)
    expect = ("k_frame_normal", "k_lm_step", "k_build_act", "k_lm_back") + (("k_lr_band",) if motion_prior else ())
    _compare(_lib.Handle(sk, cams, opts, pr), _lib.Handle.multi([sk], [cams], [opts], pr),
             lambda h: h.solve_host(d["q_init"], d["meas"], d["weight"]),
             lambda h: h.solve_ragged_host(list(d["q_init"]), list(d["meas"]), list(d["weight"])), KINEMATIC, expect)


def test_kinetic_solve_census():
    # nodes n < 2 only clear: N = 16 gives every physics kernel nodes to work on
    sk, cams, opts = skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24)), synth.make_cameras(6), abi.default_options()
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0, False)
    d = synth.make_gallop_batch(sk, cams, B=2, N=16, fps=120.0, seed=22, stance_frames=6)
    expect = ("k_frame_normal", "k_lm_step", "k_build_act", "k_dyn_eval", "k_dyn_gather", "k_lm_back", "k_dyn_assemble", "k_dyn_schur", "k_dyn_jac")
    _compare(_lib.Handle(sk, cams, opts), _lib.Handle.multi([sk], [cams], [opts]),
             lambda h: h.solve_kinetic_host(ko, d["q_init"], d["meas"], d["weight"], d["stance"]),
             lambda h: h.solve_kinetic_ragged_host([ko], list(d["q_init"]), list(d["meas"]), list(d["weight"]), list(d["stance"])),
             _lib.KINETIC_OUTPUTS, expect)
