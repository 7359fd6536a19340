"""The 3D kinematic cost weighted by the kinematic posterior on the GPU (cpe_track_precision, cpe_solve_kinetic_tracked_weighted*,
estimate_kinetics(track_weights="posterior")): the per-frame term entry by entry against numpy, the precision kernel on real
posterior blocks, optimality against the oracle's objective, the ragged contract, the refusals and the flow through files."""
import ctypes as C
import os

import numpy as np
import pytest

import track_compare as TC
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth
from test_gpu_tracked import FIELDS, KSTATS, STATS, _consistent_target, _eval, _gallop, _model

pytestmark = pytest.mark.gpu


def _dev(h):
    import torch
    return torch.device("cuda", h.device)


def _eval_W(h, q, qt, W):
    """eval_normal_tracked(track_W=W): g [B, N, 28], Bm [B, N, 28, 28], cost [B, N, 3]"""
    import torch
    dev = _dev(h)
    B, N = q.shape[:2]
    T = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    g = torch.empty((B, N, 28), dtype=torch.float64, device=dev); Bm = torch.empty((B, N, 28, 28), dtype=torch.float64, device=dev)
    cost = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
    h.eval_normal_tracked(T(q), T(qt), g, Bm, cost, track_W=T(W))
    h.synchronize()
    return g.cpu().numpy(), Bm.cpu().numpy(), cost.cpu().numpy()


def _synthetic_cov(rng, shape, lo=-2.0, hi=0.0):
    """u-space covariance blocks [*shape, 28, 28]: a well-conditioned correlation pattern, standard deviations 10^lo .. 10^hi across coordinates"""
    A = rng.standard_normal(tuple(shape) + (28, 28)) / np.sqrt(28.0)
    S = A @ np.swapaxes(A, -1, -2) + 0.5 * np.eye(28)
    S = 0.5 * (S + np.swapaxes(S, -1, -2))
    s = 10.0 ** rng.uniform(lo, hi, tuple(shape) + (28,))
    return s[..., :, None] * S * s[..., None, :]


@pytest.mark.parametrize("case", ["phantom", "jules", "mono_prior"])
def test_weighted_term_entry_by_entry(case):
    """eval(W) - eval(0) == numpy's gradient and block of T_n = d^T W_n d to 1e-12 of their scale with a different SPD W_n per frame, cost[0] ==
    T_n, the other cost slots bit-equal; with W_n = diag(w) the outputs are those of eval_normal_tracked(w)"""
    animal = "jules" if case == "jules" else "phantom"
    md = _model(animal, 120.0, n_cams=1 if case == "mono_prior" else 6)
    pr = priors.load_priors(pose=True, motion=False) if case == "mono_prior" else None
    d = synth.make_gallop_batch(md["sk"], md["cams"], B=2, N=8, fps=120.0, seed=17)
    rng = np.random.default_rng(9)
    q = d["q_true"] + rng.normal(0, 0.05, d["q_true"].shape)
    for lk in ("HFL", "UBR"):
        q[..., skeleton.dof(lk, 1)] += 1.6                                        # limbs beyond the horizontal
    qt = d["q_true"]
    w = abi.default_track_weights() * (1.0 + rng.random(abi.NX))
    W = TC.random_spd(rng, (2, 8))
    assert np.abs(W[0, 0] - W[1, 3]).max() > 1.0
    h = _lib.Handle(md["sk"], md["cams"], md["opts"], pr)
    try:
        g1, B1, c1 = _eval_W(h, q, qt, W)
        g0, B0, c0 = _eval_W(h, q, qt, np.zeros_like(W))
        gd, Bd, cd = _eval_W(h, q, qt, np.ascontiguousarray(np.broadcast_to(np.diag(w), W.shape)))
        gw, Bw, cw = _eval(h, q, qt, w)
    finally:
        h.close()
    Tn, gT, HT = TC.weighted_term(md["sk"], q, qt, W)
    sg, sB, sT = max(1.0, np.abs(gT).max()), max(1.0, np.abs(HT).max()), max(1.0, np.abs(Tn).max())
    print(f"weighted term {case}: |g - numpy| {np.abs((g1 - g0) - gT).max():.2e} of {sg:.2e}, |B - numpy| {np.abs((B1 - B0) - HT).max():.2e} of {sB:.2e}, "
          f"|T - numpy| {np.abs(c1[..., 0] - Tn).max():.2e} of {sT:.2e}")
    assert np.abs((g1 - g0) - gT).max() < 1e-12 * sg
    assert np.abs((B1 - B0) - HT).max() < 1e-12 * sB
    assert np.abs(c1[..., 0] - Tn).max() < 1e-12 * sT and np.all(c0[..., 0] == 0.0)
    assert np.array_equal(c1[..., 1:], c0[..., 1:])                             # bounds and pose prior do not see the weights
    if pr is not None:
        assert np.abs(c1[..., 2]).min() > 0.0
    # the diagonal form through the full-weight path
    swg, swB, swT = max(1.0, np.abs(gw).max()), max(1.0, np.abs(Bw).max()), max(1.0, np.abs(cw[..., 0]).max())
    assert np.abs(gd - gw).max() < 1e-12 * swg and np.abs(Bd - Bw).max() < 1e-12 * swB and np.abs(cd[..., 0] - cw[..., 0]).max() < 1e-12 * swT
    assert np.array_equal(cd[..., 1:], cw[..., 1:])


@pytest.fixture(scope="module")
def posterior_blocks():
    """cov_diag [1, 12, 28, 28] of two real kinematic solves at N = 12: six cameras, and one camera with the packaged priors (ill-conditioned)"""
    out = {}
    for name, n_cams, pr in (("six", 6, None), ("mono", 1, priors.load_priors())):
        sk = skeleton.build_skeleton("phantom", 24)
        cams = (abi.Camera * n_cams)(*synth.make_cameras(6, seed=200)[:n_cams])
        d = synth.make_gallop_batch(sk, cams, B=1, N=12, fps=120.0, seed=23)
        h = _lib.Handle(sk, cams, abi.default_options(120.0), pr)
        try:
            sol = h.solve_host(d["q_init"], d["meas"], d["weight"])
            cov = h.covariance_host(sol["q"], d["meas"], d["weight"], 0.0, want_off=False, want_pos=False)
        finally:
            h.close()
        assert cov["status"] == abi.OK, name
        out[name] = dict(sk=sk, cams=cams, pri=pr, cov=cov["cov_diag"])
    return out


@pytest.mark.parametrize("name", ["six", "mono"])
def test_precision_kernel_on_real_posterior_blocks(posterior_blocks, name):
    """per frame max |2 W C / scale - I| <= 8 x that of np.linalg.inv on the block + 1e-13; W bit-symmetric; no frame skipped"""
    c = posterior_blocks[name]
    scale = 2.5
    h = _lib.Handle(c["sk"], c["cams"], abi.default_options(120.0), c["pri"])
    try:
        W = h.track_precision_host(c["cov"], scale)
    finally:
        h.close()
    Cx = TC.x_covariance(c["sk"], c["cov"])
    ref = TC.precision_residual(TC.precision(c["sk"], c["cov"], scale), Cx, scale)
    got = TC.precision_residual(W, Cx, scale)
    print(f"precision {name}: cond {np.linalg.cond(Cx).max():.2e}, residual HIP {got.max():.2e}, numpy inverse {ref.max():.2e}, "
          f"worst ratio {(got / np.maximum(ref, 1e-300)).max():.2f}")
    assert W.shape == c["cov"].shape and np.isfinite(W).all()
    assert np.array_equal(W, np.swapaxes(W, -1, -2))
    assert (np.abs(W).max(axis=(-2, -1)) > 0.0).all()                          # every frame was written
    assert (got <= 8.0 * ref + 1e-13).all()


def test_precision_kernel_flags_a_block_without_a_factor(posterior_blocks):
    """B = 2: a negated block and a NaN block each give CPE_NUMERICAL naming the sequence and the frame; the block's W is zero, the others are
    those of the clean call"""
    c = posterior_blocks["six"]
    cov = np.concatenate([c["cov"], c["cov"]], axis=0)
    h = _lib.Handle(c["sk"], c["cams"], abi.default_options(120.0))
    try:
        clean = h.track_precision_host(cov, 1.0)
        for (b, n), fill in (((1, 3), "negated"), ((0, 10), "nan")):
            bad = cov.copy()
            bad[b, n] = -bad[b, n] if fill == "negated" else np.nan
            W = np.full_like(bad, 7.0)
            st = h.lib.cpe_track_precision_host(h._h, 2, 12, None, None, bad.ctypes.data, 1.0, W.ctypes.data)
            msg = h.lib.cpe_last_error().decode()
            assert st == abi.NUMERICAL and f"sequence {b}, frame {n}" in msg, (fill, st, msg)
            assert not W[b, n].any()
            keep = np.ones((2, 12), bool); keep[b, n] = False
            assert np.array_equal(W[keep], clean[keep])
            with pytest.raises(_lib.CpeError, match=f"sequence {b}, frame {n}"):
                h.track_precision_host(bad, 1.0)
    finally:
        h.close()


def test_precision_kernel_ragged_equals_solo_and_leaves_the_padding(posterior_blocks):
    """lengths (12, 7): the ragged call == the solo calls bit for bit, and nothing is written past a sequence's end (device form, on a sentinel)"""
    import torch
    c = posterior_blocks["mono"]
    covs = [c["cov"][0], c["cov"][0, 2:9]]
    h = _lib.Handle(c["sk"], c["cams"], abi.default_options(120.0), c["pri"])
    try:
        solo = [h.track_precision_host(cv[None], 1.5)[0] for cv in covs]
        both = h.track_precision_host(covs, 1.5)
        dev = _dev(h)
        cd = torch.tensor(_lib.pad_track_W(covs), device=dev)
        cd[1, 7:] = float("nan")                                                # the padding is not read either
        Wd = torch.full((2, 12, 28, 28), -3.0, dtype=torch.float64, device=dev)
        h.track_precision(cd, Wd, 1.5, model=[0, 0], n_frames=[12, 7])
        h.synchronize()
        Wd = Wd.cpu().numpy()
    finally:
        h.close()
    for b, n in enumerate((12, 7)):
        assert both[b].shape == (n, 28, 28)
        assert np.array_equal(both[b], solo[b]) and np.array_equal(Wd[b, :n], solo[b]), b
    assert np.all(Wd[1, 7:] == -3.0)


# measured on one MI355X, started at the target as the existing test starts: max |g| 152.9 at the solution, 8.632e3 at the start (the target itself:
# the tracked term vanishes there, the physics terms do not), ratio 1.77e-2, 199 iterations; HIP's cost 4.010303393818491 against oracle + T
# 4.010303393818535.  Each bound is twice the measured value.
G_BOUND = 306.0
RATIO_BOUND = 3.6e-2


@pytest.fixture(scope="module")
def consistent():
    return _consistent_target()


def test_weighted_solution_is_a_minimiser_of_the_oracles_objective(oracle, consistent):
    """prescribed foot forces, max_outer = 0, W_n = track_precision of synthetic SPD blocks (standard deviations over two decades): HIP's cost
    == the oracle's objective (weight = 0) + numpy's T to 1e-10; the oracle-plus-numpy gradient at the solution is far below its value at the
    start; 100 W tracks the target more closely"""
    md, d, sol, fx = consistent
    tgt = sol["q"]
    N = tgt.shape[1]
    opts = abi.default_options(120.0)
    opts.tol_cost, opts.max_iter, opts.max_outer = 1e-6, 600, 0
    cov = _synthetic_cov(np.random.default_rng(77), (1, N))
    # started where the existing test starts (the target itself) the tracked term and its gradient vanish at the start; the physics terms do not
    h = _lib.Handle(md["sk"], md["cams"], opts)
    try:
        W = h.track_precision_host(cov, 1.0)
        r = h.solve_kinetic_tracked_weighted_host(md["ko"], W, tgt, tgt, d["stance"], grf_fixed=fx)
        r100 = h.solve_kinetic_tracked_weighted_host(md["ko"], 100.0 * W, tgt, tgt, d["stance"], grf_fixed=fx)
    finally:
        h.close()
    st = r["stats"][0]
    assert np.array_equal(W, np.swapaxes(W, -1, -2))
    assert st.status == abi.OK and st.outer == 0
    zero = np.zeros_like(d["weight"][0])

    def total(q):
        f, g, qc, terms, _ = oracle.kinetic_objective(md["sk"], md["cams"], opts, None, md["ko"], q, d["meas"][0], zero, d["stance"][0], grf_fixed=fx[0])
        Tn, gT, _ = TC.weighted_term(md["sk"], qc, tgt[0], W[0])
        # the reported cost leaves out the angle bounds' penalty (terms[3]) in both implementations; the gradient is that of everything minimised
        return f - terms[0] - terms[3] + float(Tn.sum()), g + gT, float(Tn.sum())

    f_s, g_s, T_s = total(r["q"][0])
    f_0, g_0, _ = total(tgt[0])
    ratio = np.abs(g_s).max() / np.abs(g_0).max()
    dist = lambda res: float(((synth.tracked_x(md["sk"], res["q"][0]) - synth.tracked_x(md["sk"], tgt[0])) ** 2).sum())
    print(f"weighted optimality: max |g| at the solution {np.abs(g_s).max():.3e}, at the start {np.abs(g_0).max():.3e}, ratio {ratio:.2e}; "
          f"{st.iterations} iterations; cost HIP {st.cost / opts.cost_scale!r} oracle + T {f_s!r}; cost_meas {st.cost_meas!r} T {T_s!r}; "
          f"sum |x - x*|^2 {dist(r):.4e} with W, {dist(r100):.4e} with 100 W ({r100['stats'][0].iterations} iterations, status {r100['stats'][0].status})")
    assert abs(st.cost / opts.cost_scale - f_s) <= 1e-10 * abs(f_s)
    assert f_s < f_0
    assert np.abs(g_s).max() < G_BOUND and ratio < RATIO_BOUND
    assert dist(r100) < dist(r)


def test_ragged_weighted_is_bit_equal_to_solo_solves():
    """phantom with 6 cameras and arabia-02 with 4, lengths (12, 19, 15), max_iter 20: one cpe_solve_kinetic_tracked_weighted_ragged_host == each
    sequence alone, bit for bit, in every field and stat; the padding is zero"""
    models = [_model("phantom", 120.0, False, n_cams=6, max_iter=20, seed=200), _model("arabia-02", 200.0, True, n_cams=4, max_iter=20, seed=201)]
    lens, of = (12, 19, 15), (0, 1, 0)
    rng = np.random.default_rng(41)
    seqs = []
    for b, N in enumerate(lens):
        dd = _gallop(models[of[b]], N, seed=70 + b)
        W = TC.precision(models[of[b]]["sk"], _synthetic_cov(rng, (N,)), 1.0)
        seqs.append(dict(m=of[b], q_init=dd["q_init"][0], q_target=dd["q_true"][0], meas=dd["meas"][0], weight=dd["weight"][0], stance=dd["stance"][0],
                         W=0.5 * (W + np.swapaxes(W, -1, -2))))
    h = _lib.Handle.multi([md["sk"] for md in models], [md["cams"] for md in models], [md["opts"] for md in models])
    try:
        out = h.solve_kinetic_tracked_weighted_ragged_host([md["ko"] for md in models], [s["W"] for s in seqs], [s["q_init"] for s in seqs],
                                                           [s["q_target"] for s in seqs], [s["stance"] for s in seqs], [s["meas"] for s in seqs],
                                                           [s["weight"] for s in seqs], [s["m"] for s in seqs])
    finally:
        h.close()
    for b, s in enumerate(seqs):
        md = models[s["m"]]
        h1 = _lib.Handle(md["sk"], md["cams"], md["opts"])
        try:
            ref = h1.solve_kinetic_tracked_weighted_host(md["ko"], s["W"][None], s["q_init"][None], s["q_target"][None], s["stance"][None],
                                                         s["meas"][None], s["weight"][None])
        finally:
            h1.close()
        assert ref["stats"][0].iterations > 0 and ref["stats"][0].cost_meas > 0.0
        for k in FIELDS + ("meas_err",):
            assert np.array_equal(out[k][b], ref[k][0]), (b, k)
        for f in STATS:
            assert getattr(out["stats"][b], f) == getattr(ref["stats"][0], f), (b, f)
        for f in KSTATS:
            assert getattr(out["kstats"][b], f) == getattr(ref["kstats"][0], f), (b, f)
    for k in FIELDS:
        for b, N in enumerate(lens):
            assert not out["padded"][k][b, N:].any(), (k, b)


def test_refusals_name_the_argument():
    md = _model(max_iter=5)
    d = _gallop(md, 12, seed=3)
    W = TC.random_spd(np.random.default_rng(1), (1, 12))
    h = _lib.Handle(md["sk"], md["cams"], md["opts"])
    try:
        solve = lambda **kw: h.solve_kinetic_tracked_weighted_host(md["ko"], kw.pop("W", W), d["q_init"], kw.pop("qt", d["q_true"]), d["stance"], **kw)
        with pytest.raises(_lib.CpeError, match="track_W is null"):
            solve(W=None)
        qt = d["q_true"].copy(); qt[0, 5, 7] = np.nan
        with pytest.raises(_lib.CpeError, match="q_target"):
            solve(qt=qt)
        for what, (i, j, v) in (("non-finite", (3, 4, np.inf)), ("non-finite", (4, 3, np.nan)), ("negative diagonal", (6, 6, -1e-3)), ("not symmetric", (2, 9, 0.5))):
            Wb = W.copy(); Wb[0, 7, i, j] = v
            with pytest.raises(_lib.CpeError, match=f"track_W: {what}.*sequence 0, frame 7"):
                solve(W=Wb)
        lib = h.lib
        qi = np.ascontiguousarray(d["q_init"]); st = np.ascontiguousarray(d["stance"], dtype=np.int32); me = np.ascontiguousarray(d["meas"])
        we = np.ascontiguousarray(d["weight"])
        out = np.empty_like(qi)
        tail = [st.ctypes.data, None, None, None, out.ctypes.data, *([None] * 8), (abi.Stats * 1)(), (abi.KineticStats * 1)()]
        head = [h._h, C.byref(md["ko"]), W.ctypes.data, 1, 12, qi.ctypes.data]
        s = lib.cpe_solve_kinetic_tracked_weighted_host(*head, None, None, None, *tail)
        assert s == abi.BAD_ARG and b"q_target" in lib.cpe_last_error()
        s = lib.cpe_solve_kinetic_tracked_weighted_host(*head, qi.ctypes.data, me.ctypes.data, None, *tail)
        assert s == abi.BAD_ARG and b"meas" in lib.cpe_last_error() and b"weight" in lib.cpe_last_error()
        s = lib.cpe_solve_kinetic_tracked_weighted_host(*head, qi.ctypes.data, None, we.ctypes.data, *tail)
        assert s == abi.BAD_ARG and b"meas" in lib.cpe_last_error() and b"weight" in lib.cpe_last_error()
        # a sequence's padding is not looked at: garbage past its own frames passes the host form's checks
        Wp = _lib.pad_track_W([W[0, :9]]); Wp = np.concatenate([Wp, np.full((1, 3, 28, 28), np.nan)], axis=1)
        mo, nf = (C.c_int32 * 1)(0), (C.c_int32 * 1)(9)
        s = lib.cpe_solve_kinetic_tracked_weighted_ragged_host(h._h, C.byref(md["ko"]), Wp.ctypes.data, 1, 12, mo, nf, qi.ctypes.data, qi.ctypes.data, None, None,
                                                               *tail)
        assert s in (abi.OK, abi.MAX_ITER), lib.cpe_last_error()
        # the device entries: NULL track_W, and the target copied back and checked before anything is launched
        import torch
        dev = _dev(h)
        T = lambda a, dt=np.float64: torch.tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
        E = lambda *s_: torch.empty(s_, dtype=torch.float64, device=dev)
        outs = lambda: (E(1, 12, 54), E(1, 12, 54), E(1, 12, 54), E(1, 12, 24, 3))
        with pytest.raises(_lib.CpeError, match="track_W is null"):
            h.solve_kinetic_tracked_weighted(md["ko"], None, T(d["q_init"]), T(d["q_true"]), T(d["stance"], np.int32), *outs())
        with pytest.raises(_lib.CpeError, match="q_target"):
            h.solve_kinetic_tracked_weighted(md["ko"], T(W), T(d["q_init"]), T(qt), T(d["stance"], np.int32), *outs())
        g, Bm, cost = E(1, 12, 28), E(1, 12, 28, 28), E(1, 12, 3)
        s = lib.cpe_eval_normal_tracked_weighted(h._h, None, 1, 12, T(d["q_init"]).data_ptr(), T(d["q_true"]).data_ptr(), g.data_ptr(), Bm.data_ptr(),
                                                 cost.data_ptr(), None, None)
        assert s == abi.BAD_ARG and b"track_W is null" in lib.cpe_last_error()
        # cpe_track_precision
        cov = _synthetic_cov(np.random.default_rng(2), (1, 12))
        for args, name in (((None, 1.0, W.ctypes.data), "cov_diag"), ((cov.ctypes.data, 1.0, None), "W is null"), ((cov.ctypes.data, 0.0, W.ctypes.data), "scale"),
                           ((cov.ctypes.data, -1.0, W.ctypes.data), "scale"), ((cov.ctypes.data, float("nan"), W.ctypes.data), "scale"),
                           ((cov.ctypes.data, float("inf"), W.ctypes.data), "scale")):
            s = lib.cpe_track_precision_host(h._h, 1, 12, None, None, *args)
            assert s == abi.BAD_ARG and name.encode() in lib.cpe_last_error(), (name, s, lib.cpe_last_error())
    finally:
        h.close()


def test_estimate_kinetics_with_posterior_weights_end_to_end(tmp_path):
    """write_dataset -> estimate_kinematics(uncertainty=True) -> estimate_kinetics(use_2d_reprojections=False, track_weights="posterior"), through
    files; the ragged batch entry writes the same numbers; the default arguments still write what track_weights="reference" writes"""
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    info = write_dataset(str(tmp_path), N=48, noise_px=0.5, gallop=True)
    est = E.init_trajectory(str(tmp_path), info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
    assert E.estimate_kinematics(est, solver_output=False, uncertainty=True) is True
    kin_dir = os.path.join(str(tmp_path), info["data_path"], "fte_kinematic")
    cov_u = np.load(os.path.join(kin_dir, "uncertainty.npz"))["cov_u"]
    kin = E.load_result_pickle(os.path.join(kin_dir, "fte.pickle"))
    mk = lambda: E.init_trajectory(str(tmp_path), info["data_path"], "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True,
                                   bound_eom_error=(-2.0, 2.0), include_camera_constraints=True, kinematic_model=False)
    kw = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True, use_2d_reprojections=False)
    scale = 0.25
    est2 = mk()
    ok = E.estimate_kinetics(est2, track_weights="posterior", track_scale=scale, out_fname="fte_post", **kw)
    st = est2.result["stats"][0]
    print(f"posterior end to end: status {st.status}, {st.iterations} iterations / {st.outer} updates, costs {est2.costs}")
    assert ok is True
    out_dir = os.path.join(str(tmp_path), info["data_path"], "fte_kinetic")
    d = E.load_result_pickle(os.path.join(out_dir, "fte_post.pickle"))
    assert d["q"].shape == (48, 54)
    W = TC.precision(est2.skeleton, cov_u[:48], scale)
    Tn, _, _ = TC.weighted_term(est2.skeleton, d["q"], kin["q"][:48], W)
    print(f"posterior end to end: measurement {est2.costs['measurement']!r}, numpy sum d^T W d {Tn.sum()!r}")
    assert abs(est2.costs["measurement"] - Tn.sum()) <= 1e-9 * max(1.0, Tn.sum())
    # the batch entry, ragged: the same numbers
    est3 = mk()
    assert E.estimate_kinetics_batch([est3], out_fname="fte_post_batch", ragged=True, track_weights="posterior", track_scale=scale, **kw) == [True]
    d3 = E.load_result_pickle(os.path.join(out_dir, "fte_post_batch.pickle"))
    for k in ("q", "dq", "ddq", "positions", "meas_err"):
        assert np.array_equal(np.asarray(d3[k]), np.asarray(d[k])), k
    for k in d["tau"]:
        assert np.array_equal(d3["tau"][k], d["tau"][k]), k
    assert est3.costs == est2.costs
    # the batch entry, plain (one group of one sequence): every array of the pickle
    est6 = mk()
    assert E.estimate_kinetics_batch([est6], out_fname="fte_post_plain_batch", ragged=False, track_weights="posterior", track_scale=scale, **kw) == [True]
    d6 = E.load_result_pickle(os.path.join(out_dir, "fte_post_plain_batch.pickle"))
    assert set(d6) == set(d) and {"q", "dq", "ddq", "positions", "meas_err", "x", "dx", "ddx", "com_pos", "com_vel", "tau"} <= set(d)
    for k, v in d.items():
        if isinstance(v, (np.ndarray, list)):
            assert np.array_equal(np.asarray(d6[k]), np.asarray(v)), k
    assert set(d6["tau"]) == set(d["tau"])
    for k in d["tau"]:
        assert np.array_equal(d6["tau"][k], d["tau"][k]), k
    assert est6.costs == est2.costs
    # default arguments: the reference's weights, as before
    est4, est5 = mk(), mk()
    assert E.estimate_kinetics(est4, out_fname="fte_default", **kw) is True
    assert E.estimate_kinetics(est5, out_fname="fte_reference", track_weights="reference", **kw) is True
    d4, d5 = E.load_result_pickle(os.path.join(out_dir, "fte_default.pickle")), E.load_result_pickle(os.path.join(out_dir, "fte_reference.pickle"))
    for k in ("q", "dq", "ddq", "positions", "meas_err"):
        assert np.array_equal(np.asarray(d4[k]), np.asarray(d5[k])), k
    assert est4.costs == est5.costs and est4.costs != est2.costs
    assert not np.array_equal(np.asarray(d4["q"]), np.asarray(d["q"]))
