"""The first LM iteration of a solve, entry by entry: the band assembly, block Cholesky factor and forward substitution of k_lm_step and the back
substitution, predicted decrease and trial iterate of k_lm_back, through cpe_eval_lm_step, against the oracle's system (tests/lm_compare.py).
Short sequences, both sides of the motion prior's constant-block switch, windows 1 to 4, long sequences that wrap every LDS ring, a large mixed
batch, the edges of the per-frame blocks, the physics-based model and a sequence that fails inside a batch.  Each case asserts that the path it
means to exercise is active and records its worst value per key; test_zz_report prints the worst of the module."""
import numpy as np
import pytest

import lm_compare as LC
from cheetah_pose_estimation_amd import abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

WORST = {}                                        # (case, key) -> worst value, printed at the end of the module
OUT_KEYS = ("g", "dg", "L", "delta", "state", "seq")


def _compare(oracle, h, sk, cams, opts, pr, q, meas, weight, lam, label, kopts=None, stance=None, G=None):
    """HIP vs oracle on every output of cpe_eval_lm_step for a batch; returns HIP's outputs"""
    if G is None:
        G = h.eval_lm_step_host(q, meas, weight, lam, kopts, stance)
    slots = LC.coordinate_slots(sk)
    worst, bad = {}, {}
    for b in range(q.shape[0]):
        assert G["seq"][b, 7] == abi.OK, (label, b, "no step")
        R = LC.reference(oracle, sk, cams, opts, pr, q[b], meas[b], weight[b], lam, h.pb, kopts, None if stance is None else stance[b])
        d = LC.discrepancies({k: v[b] for k, v in G.items()}, R, slots, LC.condition(R))
        for k in LC.KEYS:
            if k == "delta" and not (d.get("cond") is not None and d["cond"] <= LC.COND_ASSERT):
                continue
            worst[k] = max(worst.get(k, 0.0), d[k])
        if d.get("cond") is not None:
            worst["cond"] = max(worst.get("cond", 0.0), d["cond"])
        bad.update({(b, k): v for k, v in LC.failures(d).items()})
    print(f"{label}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        WORST[(label, k)] = v
    assert not bad, (label, bad)
    return G


def _phantom25(n_cams=6):
    return skeleton.build_skeleton("phantom", 25), synth.make_cameras(n_cams)


def _frames(d, lo, N):
    return tuple(np.ascontiguousarray(d[k][:, lo:lo + N]) for k in ("q_init", "meas", "weight"))


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8, 9, 12])
def test_short_sequences_without_prior(oracle, gpu_handle_factory, N):
    """k_lm_step<3, 0> with the plain per-frame kernel: N < RING = 4 (the window never fills), the damping floor 0.1 below 4 frames, 1e-12 from 4"""
    sk, cams = _phantom25()
    opts = abi.default_options()
    h = gpu_handle_factory(sk, cams, opts)
    assert h.pb == 3
    q, me, we = _frames(synth.make_batch(sk, cams, B=2, N=12, seed=21), 0, N)
    for lam in (1e-12, 1e-4, 1e-1, 1e3):
        G = _compare(oracle, h, sk, cams, opts, None, q, me, we, lam, f"no prior N = {N} lambda {lam:g}")
        # the damping of k_lm_back's prediction uses the floor of this length: pred = -g.d / 2 + lam sum max(dg, floor) d^2 / 2
        fl = LC.diag_floor(N)
        for b in range(2):
            g, d = G["g"][b], G["delta"][b]
            p = -0.5 * float((g * d).sum()) + 0.5 * lam * float((np.maximum(G["dg"][b], fl) * d * d).sum())
            assert abs(p - G["seq"][b, 5]) <= 1e-9 * abs(p)


def _lr_rows(N, W):
    """rows of the band whose off-diagonal blocks k_lm_step reads from the constant table lr_HIu, and the others (read from Hlr)"""
    rows = np.arange(N)
    table = (rows >= W) & (rows <= N - W)
    return rows[table], rows[~table]


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13])
def test_packaged_priors(oracle, gpu_handle_factory, N):
    """k_lm_step<4, 0>, the Gaussian-mixture per-frame kernel and both sources of the prior's off-diagonal blocks (lr_HIu away from the ends,
    Hlr written by k_lr_band near them)"""
    sk, cams = skeleton.build_skeleton("phantom", 24), synth.make_cameras(2)
    pr = priors.load_priors()
    opts = abi.default_options()
    h = gpu_handle_factory(sk, cams, opts, pr)
    assert h.pb == 4 and pr.gmm_k > 0
    table, near = _lr_rows(N, 4)
    assert len(near) > 0 and (len(table) > 0) == (N >= 8)
    q, me, we = _frames(synth.make_batch(sk, cams, B=2, N=13, seed=31), 0, N)
    for lam in (1e-4, 1e-1):
        _compare(oracle, h, sk, cams, opts, pr, q, me, we, lam, f"window-4 priors N = {N} lambda {lam:g}")


@pytest.mark.parametrize("W", [1, 2, 3])
def test_prior_windows_below_the_band(oracle, gpu_handle_factory, W):
    """PB = 3 with a motion prior narrower than the constant-acceleration band: lr_HIu[k] for W < k <= 3 must add nothing, and both row kinds
    occur from N = 2 W on.  The window-W prior is the packaged one cut to its last W lags (lm_compare.truncated_prior)."""
    sk, cams = skeleton.build_skeleton("phantom", 24), synth.make_cameras(2)
    pr = LC.truncated_prior(W)
    opts = abi.default_options()
    h = gpu_handle_factory(sk, cams, opts, pr)
    assert h.pb == 3
    d = synth.make_batch(sk, cams, B=2, N=2 * W + 3, seed=41 + W)
    seen_table = False
    for N in range(1, 2 * W + 4):
        table, near = _lr_rows(N, W)
        seen_table |= len(table) > 0 and len(near) > 0
        q, me, we = _frames(d, 0, N)
        _compare(oracle, h, sk, cams, opts, pr, q, me, we, 1e-1, f"window {W} N = {N}")
    assert seen_table


def test_long_sequences(oracle, gpu_handle_factory):
    """N = 300 (B = 3) and N = 1000 (B = 1, window-4 priors: PB = 4): the window ring, the Gamma ring and the three-slot ring of k_lm_back wrap
    many times"""
    sk, cams = _phantom25()
    opts = abi.default_options()
    d = synth.make_batch(sk, cams, B=3, N=300, seed=51)
    _compare(oracle, gpu_handle_factory(sk, cams, opts), sk, cams, opts, None, d["q_init"], d["meas"], d["weight"], 1e-4, "N = 300, B = 3")
    sk24, cam2 = skeleton.build_skeleton("phantom", 24), synth.make_cameras(2)
    pr = priors.load_priors()
    d = synth.make_batch(sk24, cam2, B=1, N=1000, seed=52)
    h = gpu_handle_factory(sk24, cam2, opts, pr)
    assert h.pb == 4
    _compare(oracle, h, sk24, cam2, opts, pr, d["q_init"], d["meas"], d["weight"], 1e-4, "N = 1000, window-4 priors")


def _equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def test_large_mixed_batch(oracle, gpu_handle_factory):
    """37 x 9, mixed content (noise levels, a frame without measurements, rolled trunks): every sequence bit-equal to its own B = 1 call, the
    same call twice bit-equal, and every sequence against the oracle"""
    sk, cams = _phantom25()
    opts = abi.default_options()
    h = gpu_handle_factory(sk, cams, opts)
    d = synth.make_batch(sk, cams, B=37, N=9, seed=61)
    rng = np.random.default_rng(62)
    q, me, we = d["q_init"].copy(), d["meas"], d["weight"].copy()
    q[::3] += rng.normal(0, 0.05, q[::3].shape)
    q[1::5, :, 3] += 0.4
    we[2::7, 4] = 0.0
    G1 = h.eval_lm_step_host(q, me, we, 1e-2)
    G2 = h.eval_lm_step_host(q, me, we, 1e-2)
    assert all(_equal(G1[k], G2[k]) for k in OUT_KEYS)
    for b in range(37):
        Gs = h.eval_lm_step_host(q[b:b + 1], me[b:b + 1], we[b:b + 1], 1e-2)
        assert all(_equal(G1[k][b:b + 1], Gs[k]) for k in OUT_KEYS), b
    _compare(oracle, h, sk, cams, opts, None, q, me, we, 1e-2, "37 x 9", G=G1)


def test_edges_of_the_frame_blocks(oracle, gpu_handle_factory):
    """limbs pitched beyond 90 degrees under a rolled trunk; one frame with every weight zero; q outside an angle range (the bound term on);
    one camera; jules; 8 cameras -- ill-conditioned systems among them, where delta is compared only as far as the conditioning allows"""
    sk, cams = _phantom25()
    opts = abi.default_options()
    h = gpu_handle_factory(sk, cams, opts)
    d = synth.make_batch(sk, cams, B=2, N=8, seed=71)
    rng = np.random.default_rng(8)
    q = d["q_true"] + rng.normal(0, 0.02, d["q_true"].shape)
    q[..., 3] += 0.25
    for lk in ("HFL", "LBR", "LFR", "UBL"):
        q[..., skeleton.dof(lk, 1)] += rng.uniform(1.2, 2.2)
    Rq = oracle.objective(sk, cams, opts, None, q[0], d["meas"][0], d["weight"][0])[4]
    assert (np.abs(Rq[:, 3::3][:, 1:]) > np.pi / 2).any()                          # some |phi_c| > 90 degrees: the other branch of the pitch
    for lam in (1e-4, 1e-1):
        _compare(oracle, h, sk, cams, opts, None, q, d["meas"], d["weight"], lam, f"limbs beyond 90 degrees lambda {lam:g}")
    we = d["weight"].copy(); we[:, 3] = 0.0
    _compare(oracle, h, sk, cams, opts, None, d["q_init"], d["meas"], we, 1e-1, "a frame without measurements")
    qb = d["q_init"].copy()
    b0 = next(i for i in range(sk.n_bounds) if sk.bound_b[i] < 0)
    qb[..., sk.bound_a[b0]] = sk.bound_up[b0] + 0.3
    terms = oracle.objective(sk, cams, opts, None, qb[0], d["meas"][0], d["weight"][0])[3]
    assert terms[4] > 0.0                                                             # the bound term
    _compare(oracle, h, sk, cams, opts, None, qb, d["meas"], d["weight"], 1e-1, "q outside an angle range")
    cam1 = (abi.Camera * 1)(cams[2])
    d1 = synth.make_batch(sk, cam1, B=2, N=8, seed=72)
    _compare(oracle, gpu_handle_factory(sk, cam1, opts), sk, cam1, opts, None, d1["q_init"], d1["meas"], d1["weight"], 1e-1, "one camera")
    skj = skeleton.build_skeleton("jules", 24)
    dj = synth.make_batch(skj, cams, B=2, N=8, seed=73)
    _compare(oracle, gpu_handle_factory(skj, cams, opts), skj, cams, opts, None, dj["q_init"], dj["meas"], dj["weight"], 1e-1, "jules")
    cam8 = synth.make_cameras(8)
    d8 = synth.make_batch(sk, cam8, B=2, N=8, seed=74)
    _compare(oracle, gpu_handle_factory(sk, cam8, opts), sk, cam8, opts, None, d8["q_init"], d8["meas"], d8["weight"], 1e-1, "8 cameras")


@pytest.mark.parametrize("lam", [1e-4, 1e-1, 10.0])
def test_physics_model(oracle, gpu_handle_factory, lam):
    """k_lm_step<3, 1> (accept, damping), the elimination of the node forces at that damping, then k_lm_step<3, 2> and k_lm_back<3> on the
    eliminated band: phantom 24 without the constant-acceleration model, 2 cameras, 12 frames, free foot forces"""
    sk = skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24))
    cams = synth.make_cameras(2)
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    opts = abi.default_options(120.0)
    d = synth.make_gallop_batch(sk, cams, B=2, N=12, seed=4321, init_noise=0.002)
    st = d["stance"]
    assert st[:, 2:].any()                                                          # feet in stance: free foot forces in the eliminated band
    h = gpu_handle_factory(sk, cams, opts)
    G = _compare(oracle, h, sk, cams, opts, None, d["q_init"], d["meas"], d["weight"], lam, f"physics model lambda {lam:g}", kopts=ko, stance=st)
    assert np.all(G["seq"][:, 4] > 0.0) and not G["seq"][:, 1].any()               # the physics cost, no constant-acceleration model


def test_curvature_mode_1(oracle, gpu_handle_factory):
    """opts.curvature = 1 (the curvature weight max(rho'', 0)) on both sides, with residuals in all four pieces of the loss: the band, its
    factor and the step differ from mode 0's wherever rho'' < rho' / s"""
    import frame_compare as FC
    c = FC.loss_inputs(1, n_frames=8)
    sk, cams, opts = c["sk"], c["cams"], c["opts"]
    assert opts.curvature == 1
    pieces = FC.reference(oracle, sk, cams, opts, None, *FC.flat(c))["conditions"]["pieces"]
    assert min(pieces) >= 0.05, pieces
    h = gpu_handle_factory(sk, cams, opts)
    G1 = _compare(oracle, h, sk, cams, opts, None, c["q"], c["meas"], c["weight"], 1e-1, "curvature 1")
    G0 = gpu_handle_factory(sk, cams, FC.with_curvature(opts, 0)).eval_lm_step_host(c["q"], c["meas"], c["weight"], 1e-1)
    assert _equal(G0["g"], G1["g"]) and not _equal(G0["L"], G1["L"])                # the option reaches the kernel


def test_failed_sequence_inside_a_batch(oracle, gpu_handle_factory):
    """a NaN in q of one sequence: status CPE_NUMERICAL and no step for it; its neighbours bit-equal to their own B = 1 calls"""
    sk, cams = _phantom25()
    opts = abi.default_options()
    h = gpu_handle_factory(sk, cams, opts)
    d = synth.make_batch(sk, cams, B=3, N=9, seed=81)
    q = d["q_init"].copy()
    q[1, 5, 7] = np.nan
    G = h.eval_lm_step_host(q, d["meas"], d["weight"], 1e-1)
    assert G["seq"][1, 7] == abi.NUMERICAL
    assert not G["delta"][1].any() and not G["L"][1].any() and not G["g"][1].any()
    for b in (0, 2):
        Gs = h.eval_lm_step_host(q[b:b + 1], d["meas"][b:b + 1], d["weight"][b:b + 1], 1e-1)
        assert all(_equal(G[k][b:b + 1], Gs[k]) for k in OUT_KEYS), b
        assert G["seq"][b, 7] == abi.OK


def test_zz_report():
    """the worst value of every key over the cases of this module (the numbers the tolerances of lm_compare.TOL stand on)"""
    for k in LC.KEYS + ("cond",):
        vals = {c: v for (c, kk), v in WORST.items() if kk == k}
        if vals:
            c = max(vals, key=vals.get)
            print(f"worst {k}: {vals[c]:.2e} ({c})")
