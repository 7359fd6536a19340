"""One evaluation of the physics terms, entry by entry: the HIP node kernels (k_dyn_eval, k_dyn_jac, k_dyn_assemble) and the elimination of
the node forces into the band system (k_dyn_schur, k_dyn_gather) through cpe_eval_kinetic_system, against the oracle's kinetic_system, with
the per-entry scales of tests/kinetic_compare.py.  Every variant of the node forces, every model, the edges of the sequence, three dampings.
Each case asserts that the rows it means to exercise are active and prints the worst scaled discrepancy per key."""
import numpy as np
import pytest

import kinetic_compare as KC
from cheetah_pose_estimation_amd import abi, skeleton, synth

pytestmark = pytest.mark.gpu

LAMBDAS = (1e-4, 1e-1, 10.0)
WORST = {}                                        # (case, key) -> worst scaled discrepancy, printed at the end of the module


def _phantom(n_cams):
    sk = skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24))
    cams = synth.make_cameras(n_cams)
    return sk, cams, abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)


def _with_lambda0(opts, lam):
    import ctypes
    o = type(opts)()
    ctypes.pointer(o)[0] = opts
    o.lambda0 = lam
    return o


def _compare(oracle, h, sk, cams, opts, ko, q, meas, weight, stance, label, priors=None, var=None, tol=None, active=None):
    """HIP vs oracle on every output of cpe_eval_kinetic_system for a batch (var: {name: [B, ...] array}, at most one); active(R, b, ko):
    asserts on the oracle's outputs of sequence b that the case's rows are active.  Returns the worst discrepancy per key."""
    var = var or {}
    G = h.eval_kinetic_system_host(ko, q, meas, weight, stance, **var)
    worst = {}
    for b in range(q.shape[0]):
        vb = {k: v[b] for k, v in var.items()}
        R = oracle.kinetic_system(sk, cams, opts, priors, ko, q[b], meas[b], weight[b], stance[b], lam=opts.lambda0, **vb)
        V = oracle.kinetic_objective(sk, cams, opts, priors, ko, q[b], meas[b], weight[b], stance[b], want_grad=False, **vb)[0]
        if active is not None:
            active(R, b, ko)
        Gb = {k: v[b] for k, v in G.items()}
        d = KC.discrepancies(Gb, R, sk, ko, V)
        assert d["meta"] == 0.0, (label, b, "meta")
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{label}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items() if k != "meta"))
    for k, v in worst.items():
        WORST[(label, k)] = v
    tol = tol or KC.TOL
    bad = {k: v for k, v in worst.items() if k != "meta" and not v <= tol[k]}
    assert not bad, (label, bad)
    return worst


def _rule_active(oracle, sk, cams, opts, ko, q, meas, weight, stance, off, var=None):
    """the rule moves the multiplier terms (stat column 4) of the oracle's evaluation: the options `off` switch it off"""
    var = var or {}
    a = oracle.kinetic_system(sk, cams, opts, None, ko, q, meas, weight, stance, **var)["stat"][:, 4]
    b = oracle.kinetic_system(sk, cams, opts, None, KC.with_options(ko, **off), q, meas, weight, stance, **var)["stat"][:, 4]
    return bool(np.any(a != b))


def _gallop(sk, cams, B=2, N=12, seed=4321, **kw):
    return synth.make_gallop_batch(sk, cams, B=B, N=N, seed=seed, init_noise=kw.pop("init_noise", 0.002), **kw)


def _free_variants(oracle, sk, cams, opts, ko, d):
    """the variant arrays of every sequence, from the oracle's free evaluation of it"""
    vs = [KC.variants(oracle.kinetic_system(sk, cams, opts, None, ko, d["q_init"][b], d["meas"][b], d["weight"][b], d["stance"][b]), sk, ko)
          for b in range(d["q_init"].shape[0])]
    return {k: np.stack([v[k] for v in vs]) for k in vs[0]}


VARIANTS = ("free", "grf_fixed", "tau_box", "grf_box", "slack_box", "zvel_max", "slip_max", "foot_height_min")


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_variants_match_oracle(oracle, gpu_handle_factory, variant, lam):
    """phantom, 2 cameras, 2 x 12 frames: the free forces, prescribed forces, torque boxes, force boxes, and each inequality rule binding"""
    sk, cams, ko = _phantom(2)
    opts = _with_lambda0(abi.default_options(120.0), lam)
    d = _gallop(sk, cams)
    q, me, we, st = d["q_init"], d["meas"], d["weight"], d["stance"]
    h = gpu_handle_factory(sk, cams, opts)
    nm, nc = ko.dyn.n_motors, KC.n_constraint_forces(sk)
    var, active = None, None
    if variant in ("grf_fixed", "tau_box", "grf_box"):
        var = {variant: _free_variants(oracle, sk, cams, opts, ko, d)[variant]}
    if variant == "free":
        def active(R, b, k):
            assert st[b][2:].any() and (R["meta"][2:, 0] > nm + nc).any()                  # stance feet carry free forces
            assert _rule_active(oracle, sk, cams, opts, ko, q[b], me[b], we[b], st[b], dict(kappa_force=2 * ko.kappa_force))
    elif variant == "grf_fixed":
        def active(R, b, k):
            on = st[b][2:] == 1
            assert on.any() and (R["meta"][2:, 0] == nm + nc).all()                         # no foot force is free
            F = R["f"][2:, nm + nc:nm + nc + 12].reshape(-1, 4, 3)
            assert np.array_equal(F[on], var["grf_fixed"][b][2:][on])
    elif variant == "tau_box":
        def active(R, b, k):
            tb, tau = var["tau_box"][b][2:], R["f"][2:, :nm]
            assert np.any((tau < tb[..., 0]) | (tau > tb[..., 1]))
    elif variant == "grf_box":
        def active(R, b, k):
            gb, F = var["grf_box"][b][2:], R["f"][2:, nm + nc:nm + nc + 12].reshape(-1, 4, 3)
            assert np.any(((F < gb[..., 0]) | (F > gb[..., 1]))[st[b][2:] == 1])
    elif variant == "slack_box":
        s0 = min(oracle.kinetic_system(sk, cams, opts, None, ko, q[b], me[b], we[b], st[b])["stat"][2:, 5].min() for b in range(2))
        ko = KC.with_options(ko, slack_lo=-0.3 * s0, slack_hi=0.3 * s0)
        def active(R, b, k):
            assert _rule_active(oracle, sk, cams, opts, k, q[b], me[b], we[b], st[b], dict(slack_lo=-1e10, slack_hi=1e10))
    elif variant == "zvel_max":
        ko = KC.with_options(ko, zvel_max=0.05, slip_max=0.0)
        def active(R, b, k):
            assert _rule_active(oracle, sk, cams, opts, k, q[b], me[b], we[b], st[b], dict(zvel_max=0.0))
    elif variant == "slip_max":
        ko = KC.with_options(ko, slip_max=0.02)
        def active(R, b, k):
            assert _rule_active(oracle, sk, cams, opts, k, q[b], me[b], we[b], st[b], dict(slip_max=0.0))
    elif variant == "foot_height_min":
        q = q.copy(); q[..., 2] -= 0.08                                                    # the whole animal 8 cm lower: swing paws below ground
        def active(R, b, k):
            assert _rule_active(oracle, sk, cams, opts, k, q[b], me[b], we[b], st[b], dict(foot_height_min=-1e10))
    _compare(oracle, h, sk, cams, opts, ko, q, me, we, st, f"{variant} lambda0 {lam:g}", var=var, active=active)


def test_models_match_oracle(oracle, gpu_handle_factory):
    """phantom with 6 cameras, jules at 90 fps, the kinetic-dataset configuration (arabia, pinhole rig, 200 fps), and one camera with the
    Gaussian-mixture pose prior (the per-frame kernel that is not the plain one feeds Bk)"""
    from cheetah_pose_estimation_amd import priors
    from test_gpu_parity import _kinetic_setup
    sk, cams, ko = _phantom(6)
    opts = abi.default_options(120.0)
    d = _gallop(sk, cams)
    _compare(oracle, gpu_handle_factory(sk, cams, opts), sk, cams, opts, ko, d["q_init"], d["meas"], d["weight"], d["stance"], "phantom 6 cameras")
    skj = skeleton.without_motion_model(skeleton.build_skeleton("jules", 24))
    koj = abi.default_kinetic_options(skeleton.dyn_options("jules"), 90.0)
    optj = abi.default_options(90.0)
    d = _gallop(skj, cams, fps=90.0)
    _compare(oracle, gpu_handle_factory(skj, cams, optj), skj, cams, optj, koj, d["q_init"], d["meas"], d["weight"], d["stance"], "jules 90 fps")
    sk0, pcams = _kinetic_setup()
    ska = skeleton.without_motion_model(sk0)
    koa = abi.default_kinetic_options(skeleton.dyn_options("arabia"), 200.0, True)
    opta = abi.default_options(200.0)
    d = synth.make_gallop_batch(ska, pcams, B=2, N=12, fps=200.0, seed=99, kinetic_dataset=True, stance_frames=20, x0=4.5, speed=6.0, init_noise=0.002)

    def zvel_on(R, b, k):
        assert k.zvel_max == 1.0 and d["stance"][b][2:].any()
    _compare(oracle, gpu_handle_factory(ska, pcams, opta), ska, pcams, opta, koa, d["q_init"], d["meas"], d["weight"], d["stance"], "arabia kinetic dataset",
             active=zvel_on)
    pr = priors.load_priors(motion=False)
    cam1 = (abi.Camera * 1)(cams[2])
    d = _gallop(sk, cam1)
    hp = gpu_handle_factory(sk, cam1, opts, pr)
    q, me, we, st = d["q_init"], d["meas"], d["weight"], d["stance"]

    def prior_on(R, b, k):                                                     # the prior is in the oracle's per-frame blocks
        R0 = oracle.kinetic_system(sk, cam1, opts, None, k, q[b], me[b], we[b], st[b])
        assert not np.array_equal(R0["Bk"], R["Bk"])
    _compare(oracle, hp, sk, cam1, opts, ko, q, me, we, st, "monocular pose prior", priors=pr, active=prior_on)


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
def test_short_sequences_match_oracle(oracle, gpu_handle_factory, N):
    """N = 1, 2: no node (the physics outputs are zero, Bk / gk the per-frame terms); N = 3, 4, 5: the edge flags of k_dyn_gather"""
    sk, cams, ko = _phantom(2)
    opts = _with_lambda0(abi.default_options(120.0), 1e-1)
    d = _gallop(sk, cams, N=12)
    sl = slice(4, 4 + N)                                                       # frames 6.. have feet in stance
    q, me, we, st = (np.ascontiguousarray(d[k][:, sl]) for k in ("q_init", "meas", "weight", "stance"))

    def active(R, b, k):
        if N < 3:
            assert not R["Huu"].any() and not R["f"].any() and not R["Hk"][:, 1].any()
        else:
            assert R["Huu"][2:].any() and np.abs(R["Hk"][2:, 1]).max() > 0
    _compare(oracle, gpu_handle_factory(sk, cams, opts), sk, cams, opts, ko, q, me, we, st, f"N = {N}", active=active)


def test_edges_match_oracle(oracle, gpu_handle_factory):
    """a link frame near the pole of its Euler chart; every foot in stance; no foot in stance; touchdown exactly at node 2; B = 1"""
    from test_kinetic_oracle import _near_pole_sequence
    sk, cams, ko = _phantom(2)
    opts = _with_lambda0(abi.default_options(120.0), 1e-1)
    h = gpu_handle_factory(sk, cams, opts)
    d = _gallop(sk, cams, N=10)
    q, me, we, st = d["q_init"].copy(), d["meas"], d["weight"], d["stance"].copy()
    q[1] = _near_pole_sequence(oracle, sk, {"q_init": q[1:2]})
    _compare(oracle, h, sk, cams, opts, ko, q, me, we, st, "near pole")
    nm, nc = ko.dyn.n_motors, KC.n_constraint_forces(sk)
    # every foot in stance, paws in the air included: with the default 30 Newton iterations one node's force solve stops at the cap in the
    # oracle (its forces still move with more iterations), and two solvers stopped early need not agree; with 100 both converge.  The force
    # Hessian of that node has condition 4.8e6 (1e3 - 1e4 elsewhere), and the rounding of the solve grows with it: measured on an MI355X,
    # f 3.3e-10, stat 7.8e-11, Huu 3.5e-10, Hfu 1.8e-10, Hk 6.5e-11 -- hence 10 x that here, asserted together with the conditioning
    ko_all = KC.with_options(ko, inner_iterations=100)
    conds = []

    def all_feet(R, b, k):
        assert (R["meta"][2:, 0] == nm + nc + 12).all()
        more = oracle.kinetic_system(sk, cams, opts, None, KC.with_options(k, inner_iterations=1000), q[b], me[b], we[b], np.ones_like(st[b]), lam=opts.lambda0)
        assert np.array_equal(more["f"], R["f"])                               # converged: more iterations change nothing
        conds.extend(np.linalg.cond(R["Hff"][n, :R["meta"][n, 0], :R["meta"][n, 0]]) for n in range(2, len(R["f"])))
    tol = dict(KC.TOL, f=4e-9, stat=1e-9, Huu=4e-9, Hfu=2e-9, Hk=7e-10)
    _compare(oracle, h, sk, cams, opts, ko_all, q, me, we, np.ones_like(st), "all feet in stance", active=all_feet, tol=tol)
    assert max(conds) > 1e6
    _compare(oracle, h, sk, cams, opts, ko, q, me, we, np.zeros_like(st), "no foot in stance",
             active=lambda R, b, k: (R["meta"][2:, 0] == nm + nc).all() or pytest.fail("no foot"))
    td = np.zeros_like(st); td[:, 2:, 0] = 1; td[:, 2:, 3] = 1                 # two feet touch down at node 2 (the first node)
    _compare(oracle, h, sk, cams, opts, ko, q, me, we, td, "touchdown at node 2",
             active=lambda R, b, k: (R["meta"][2, 0] == nm + nc + 6 and R["meta"][:2, 0] == 0).all() or pytest.fail("touchdown"))
    _compare(oracle, h, sk, cams, opts, ko, q[:1], me[:1], we[:1], st[:1], "B = 1")


def test_large_batch_matches_oracle(oracle, gpu_handle_factory):
    """37 sequences of 9 frames in one launch"""
    sk, cams, ko = _phantom(2)
    opts = _with_lambda0(abi.default_options(120.0), 1e-1)
    d = _gallop(sk, cams, B=37, N=9, seed=77)
    _compare(oracle, gpu_handle_factory(sk, cams, opts), sk, cams, opts, ko, d["q_init"], d["meas"], d["weight"], d["stance"], "37 x 9",
             active=lambda R, b, k: None)


def test_zz_report():
    """the worst scaled discrepancy of every case and key of this module (the numbers the tolerances of kinetic_compare.TOL stand on)"""
    keys = KC.NODE_KEYS + KC.BAND_KEYS
    for k in keys:
        vals = {c: v for (c, kk), v in WORST.items() if kk == k}
        if vals:
            c = max(vals, key=vals.get)
            print(f"worst {k}: {vals[c]:.2e} ({c})")
