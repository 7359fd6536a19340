"""The physics-based solve with the 3D kinematic cost (estimate_kinetics(use_2d_reprojections=False); cpe_solve_kinetic_tracked*) on
the GPU: the per-frame term entry by entry against numpy, measurements never read, refusals, all four variants on a target the dynamics can
follow, optimality against the oracle's objective, the ragged contract and the flow through files."""
import os

import numpy as np
import pytest

from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

ANIMALS = (("phantom", 120.0, False), ("jules", 90.0, False), ("arabia-02", 200.0, True), ("shiraz-02", 200.0, True))
FIELDS = ("q", "dq", "ddq", "positions", "tau", "lam", "grf", "slack")
STATS = [f for f, _ in abi.Stats._fields_]
KSTATS = [f for f, _ in abi.KineticStats._fields_]


def _model(animal="phantom", fps=120.0, kin=False, n_cams=6, max_iter=600, seed=200):
    cams = synth.make_cameras(6, seed=seed)
    cams = (abi.Camera * n_cams)(*cams[:n_cams])
    sk = skeleton.without_motion_model(skeleton.build_skeleton(animal, 24, kinetic_dataset=kin))
    opts = abi.default_options(fps)
    opts.tol_cost, opts.max_iter = 1e-6, max_iter
    ko = abi.default_kinetic_options(skeleton.dyn_options(animal), fps, kin)
    ko.w_torque, ko.w_smooth = 1.0 + 1e-3 / fps ** 2, 0.0                          # the motion energy of this mode (acinoset_opt.py:913, :919)
    return dict(sk=sk, cams=cams, opts=opts, ko=ko, fps=fps, kin=kin)


def _gallop(md, N, seed):
    return synth.make_gallop_batch(md["sk"], md["cams"], B=1, N=N, fps=md["fps"], seed=seed, kinetic_dataset=md["kin"], stance_frames=6)


def _numpy_term(sk, q, q_target, w):
    """T_n, its gradient 2 X^T W (x - x*) and block 2 X^T W X per frame"""
    X = synth.tracked_x_jacobian(sk)
    r = synth.tracked_x(sk, q) - synth.tracked_x(sk, q_target)
    return (w * r * r).sum(-1), 2.0 * (w * r) @ X, 2.0 * X.T @ (w[:, None] * X)


def _eval(h, q, qt, w):
    import torch
    dev = torch.device("cuda", h.device)
    B, N = q.shape[:2]
    T = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    g = torch.empty((B, N, 28), dtype=torch.float64, device=dev); Bm = torch.empty((B, N, 28, 28), dtype=torch.float64, device=dev)
    cost = torch.empty((B, N, 3), dtype=torch.float64, device=dev)
    h.eval_normal_tracked(T(q), T(qt), g, Bm, cost, track_w=w)
    h.synchronize()
    return g.cpu().numpy(), Bm.cpu().numpy(), cost.cpu().numpy()


def _other_triple(sk, q):
    """the same pose with every leg link's Euler triple (phi, theta, psi) -> (phi + pi, pi - theta, psi + pi)"""
    q = q.copy()
    for c, _ in synth.leg_layout(sk):
        q[..., 3 + 3 * c] += np.pi; q[..., 3 + 3 * c + 1] = np.pi - q[..., 3 + 3 * c + 1]; q[..., 3 + 3 * c + 2] += np.pi
    return q


@pytest.mark.parametrize("case", ["phantom", "jules", "mono_prior"])
def test_tracked_term_entry_by_entry(case):
    """eval_normal_tracked(w) - eval_normal_tracked(0) == numpy's gradient and block of T_n to 1e-12 of their scale, cost[0] == T_n; the target given
    in the other Euler triple of its leg links gives the same terms"""
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
    h = _lib.Handle(md["sk"], md["cams"], md["opts"], pr)
    try:
        g1, B1, c1 = _eval(h, q, qt, w)
        g0, B0, c0 = _eval(h, q, qt, np.zeros(abi.NX))
        g2, B2, c2 = _eval(h, q, _other_triple(md["sk"], qt), w)
    finally:
        h.close()
    # the state the kernel evaluates is q made consistent with the joint equalities: the term reads independent coordinates only
    Tn, gT, HT = _numpy_term(md["sk"], q, qt, w)
    sg, sB = max(1.0, np.abs(gT).max()), max(1.0, np.abs(HT).max())
    assert np.abs((g1 - g0) - gT).max() < 1e-12 * sg
    assert np.abs((B1 - B0) - HT[None, None]).max() < 1e-12 * sB
    assert np.abs(c1[..., 0] - Tn).max() < 1e-12 * max(1.0, np.abs(Tn).max()) and np.all(c0[..., 0] == 0.0)
    assert np.array_equal(c1[..., 1:], c0[..., 1:])                             # bounds and pose prior do not see the weights
    if pr is not None:
        assert np.abs(c1[..., 2]).min() > 0.0
    assert np.abs(g2 - g1).max() < 1e-12 * sg and np.abs(B2 - B1).max() == 0.0 and np.abs(c2 - c1).max() < 1e-12 * max(1.0, np.abs(Tn).max())


def test_measurements_are_never_read():
    """meas = weight = NULL and NaN-filled meas / weight give bit-equal solves"""
    md = _model(max_iter=60)
    d = _gallop(md, 24, seed=31)
    h = _lib.Handle(md["sk"], md["cams"], md["opts"])
    try:
        a = h.solve_kinetic_tracked_host(md["ko"], d["q_init"], d["q_true"], d["stance"])
        nan = np.full_like(d["meas"], np.nan)
        b = h.solve_kinetic_tracked_host(md["ko"], d["q_init"], d["q_true"], d["stance"], nan, np.full_like(d["weight"], np.nan))
    finally:
        h.close()
    assert a["meas_err"] is None and b["meas_err"] is not None
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k
    for f in STATS:
        assert getattr(a["stats"][0], f) == getattr(b["stats"][0], f), f
    for f in KSTATS:
        assert getattr(a["kstats"][0], f) == getattr(b["kstats"][0], f), f


def test_refusals_name_the_argument():
    md = _model(max_iter=5)
    d = _gallop(md, 12, seed=3)
    h = _lib.Handle(md["sk"], md["cams"], md["opts"])
    try:
        qt = d["q_true"].copy(); qt[0, 5, 7] = np.nan
        with pytest.raises(_lib.CpeError, match="q_target"):
            h.solve_kinetic_tracked_host(md["ko"], d["q_init"], qt, d["stance"])
        w = abi.default_track_weights(); w[4] = -1.0
        with pytest.raises(_lib.CpeError, match="track_w"):
            h.solve_kinetic_tracked_host(md["ko"], d["q_init"], d["q_true"], d["stance"], track_w=w)
        w[4] = np.inf
        with pytest.raises(_lib.CpeError, match="track_w"):
            h.solve_kinetic_tracked_host(md["ko"], d["q_init"], d["q_true"], d["stance"], track_w=w)
        import ctypes as C
        lib = h.lib
        ws = abi.default_track_weights()
        qi = np.ascontiguousarray(d["q_init"]); st = np.ascontiguousarray(d["stance"], dtype=np.int32); me = np.ascontiguousarray(d["meas"])
        out = np.empty_like(qi)
        s = lib.cpe_solve_kinetic_tracked_host(h._h, C.byref(md["ko"]), ws.ctypes.data, 1, 12, qi.ctypes.data, None, None, None, st.ctypes.data, None,
                                               None, None, out.ctypes.data, *([None] * 8), (abi.Stats * 1)(), (abi.KineticStats * 1)())
        assert s == abi.BAD_ARG and b"q_target" in lib.cpe_last_error()
        s = lib.cpe_solve_kinetic_tracked_host(h._h, C.byref(md["ko"]), ws.ctypes.data, 1, 12, qi.ctypes.data, qi.ctypes.data, me.ctypes.data, None,
                                               st.ctypes.data, None, None, None, out.ctypes.data, *([None] * 8), (abi.Stats * 1)(), (abi.KineticStats * 1)())
        assert s == abi.BAD_ARG and b"meas" in lib.cpe_last_error() and b"weight" in lib.cpe_last_error()
        # the device entry checks the target too (copied back to the host before anything is launched)
        import torch
        dev = torch.device("cuda", h.device)
        T = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
        E = lambda *s_: torch.empty(s_, dtype=torch.float64, device=dev)
        with pytest.raises(_lib.CpeError, match="q_target"):
            h.solve_kinetic_tracked(md["ko"], T(d["q_init"]), T(qt), T(d["stance"].astype(np.int32)), E(1, 12, 54), E(1, 12, 54), E(1, 12, 54),
                                    E(1, 12, 24, 3))
    finally:
        h.close()


def _consistent_target(N=30, seed=4321):
    """a target the dynamics can follow: the reprojection-based physics solve of a synthetic gallop (free forces), warm-started from its kinematic
    estimate as the reference's flow is (|slack| < 5e-3 body weights).  Returns (model, gallop, that solution, its net foot forces [1, N, 4, 3])."""
    md = _model(max_iter=600)
    d = _gallop(md, N, seed)
    hk = _lib.Handle(skeleton.build_skeleton("phantom", 24), md["cams"], abi.default_options(120.0))
    try:
        kin = hk.solve_host(d["q_init"], d["meas"], d["weight"])
    finally:
        hk.close()
    h = _lib.Handle(md["sk"], md["cams"], md["opts"])
    try:
        sol = h.solve_kinetic_host(abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0), kin["q"], d["meas"], d["weight"], d["stance"])
    finally:
        h.close()
    assert sol["stats"][0].status == abi.OK and np.abs(sol["slack"]).max() < 1e-2
    g = sol["grf"]
    return md, d, sol, np.stack([g[..., 0], g[..., 1] - g[..., 3], g[..., 2] - g[..., 4]], axis=-1)


# about twice what one MI355X measured, started at the target as the reference starts (init_q = the target): the largest distance of a weighted
# relative angle from the target (rad; base position in m) free 0.097, prescribed 0.149, torque boxes 0.062, force boxes 0.101; |slack| <= 3.7e-4
BOUND = {"free": 0.2, "grf_fixed": 0.3, "tau_box": 0.12, "grf_box": 0.2}


def test_every_variant_tracks_a_consistent_target():
    """free, prescribed-force, torque-box and force-box variants, started at the target: every weighted relative angle stays near it and the
    dynamics stay met; every variant converges"""
    md, d, sol, fx = _consistent_target()
    tgt, tau = sol["q"], sol["tau"]
    gb = np.sort(np.stack([0.8 * fx, 1.2 * fx], -1), -1)
    gb[..., 1:, 0] -= 0.02; gb[..., 1:, 1] += 0.02
    variants = {"free": {}, "grf_fixed": dict(grf_fixed=fx), "tau_box": dict(tau_box=np.sort(np.stack([0.9 * tau, 1.1 * tau], -1), -1)),
                "grf_box": dict(grf_box=gb)}
    w = abi.default_track_weights()
    xt = synth.tracked_x(md["sk"], tgt[0])
    h = _lib.Handle(md["sk"], md["cams"], md["opts"])
    try:
        for name, kw in variants.items():
            r = h.solve_kinetic_tracked_host(md["ko"], tgt, tgt, d["stance"], **kw)
            st = r["stats"][0]
            dist = np.abs(synth.tracked_x(md["sk"], r["q"][0]) - xt)[:, w > 0].max()
            slack = np.abs(r["slack"]).max()
            print(f"tracked {name}: status {st.status}, {st.iterations} iterations / {st.outer} updates, max |x - x*| {dist:.3e}, max |slack| {slack:.2e}")
            assert st.status == abi.OK, name
            assert dist < BOUND[name] and slack < 1e-3, name
    finally:
        h.close()


# measured on one MI355X: max |g| 61.2 at the solution, 8.63e3 at the start (the target itself), ratio 7.1e-3 -- the solve stops on the relative
# decrease 1e-6 of this stiff objective, about two orders of magnitude down
G_BOUND = 600.0


def test_tracked_solution_is_a_minimiser_of_the_oracles_objective(oracle):
    """prescribed foot forces, no multiplier update (max_outer = 0: the oracle's objective at zero multipliers is then the one HIP minimised):
    at HIP's solution the oracle's gradient (weight = 0: no reprojections) plus numpy's gradient of T is orders of magnitude below its value
    at the start (about 1 / 140), and HIP's cost is the oracle's plus T"""
    md, d, sol, fx = _consistent_target()
    tgt = sol["q"]
    opts = abi.default_options(120.0)
    opts.tol_cost, opts.max_iter, opts.max_outer = 1e-6, 600, 0
    h = _lib.Handle(md["sk"], md["cams"], opts)
    try:
        r = h.solve_kinetic_tracked_host(md["ko"], tgt, tgt, d["stance"], grf_fixed=fx)
    finally:
        h.close()
    st = r["stats"][0]
    assert st.status == abi.OK and st.outer == 0
    w = abi.default_track_weights()
    X = synth.tracked_x_jacobian(md["sk"])
    zero = np.zeros_like(d["weight"][0])

    def total(q):
        f, g, qc, terms, _ = oracle.kinetic_objective(md["sk"], md["cams"], opts, None, md["ko"], q, d["meas"][0], zero, d["stance"][0], grf_fixed=fx[0])
        res = synth.tracked_x(md["sk"], qc) - synth.tracked_x(md["sk"], tgt[0])
        T = float((w * res * res).sum())
        # the reported cost leaves out the angle bounds' penalty (terms[3]) in both implementations; the gradient is that of everything minimised
        return f - terms[0] - terms[3] + T, g + 2.0 * (w * res) @ X

    f_s, g_s = total(r["q"][0])
    f_0, g_0 = total(tgt[0])
    ratio = np.abs(g_s).max() / np.abs(g_0).max()
    print(f"optimality: max |g| at the solution {np.abs(g_s).max():.3e}, at the start {np.abs(g_0).max():.3e}, ratio {ratio:.2e}; "
          f"{st.iterations} iterations; cost HIP {st.cost / opts.cost_scale!r} oracle + T {f_s!r}")
    assert np.abs(g_s).max() < G_BOUND and ratio < 2e-2
    assert abs(st.cost / opts.cost_scale - f_s) <= 1e-10 * abs(f_s)
    assert f_s < f_0


def test_ragged_tracked_is_bit_equal_to_solo_solves():
    """four skeletons, both rigs, N = 30 ... 58: one cpe_solve_kinetic_tracked_ragged == each sequence alone, bit for bit"""
    models = []
    for k, (animal, fps, kin) in enumerate(ANIMALS):
        md = _model(animal, fps, kin, n_cams=4 if kin else 6, max_iter=40, seed=200 + k)
        models.append(md)
    lens = (30, 41, 58, 36, 47)
    seqs = []
    for b, N in enumerate(lens):
        m = b % len(models)
        d = _gallop(models[m], N, seed=70 + b)
        seqs.append(dict(m=m, q_init=d["q_init"][0], q_target=d["q_true"][0], meas=d["meas"][0], weight=d["weight"][0], stance=d["stance"][0]))
    h = _lib.Handle.multi([md["sk"] for md in models], [md["cams"] for md in models], [md["opts"] for md in models])
    try:
        out = h.solve_kinetic_tracked_ragged_host([md["ko"] for md in models], [s["q_init"] for s in seqs], [s["q_target"] for s in seqs],
                                                  [s["stance"] for s in seqs], [s["meas"] for s in seqs], [s["weight"] for s in seqs],
                                                  [s["m"] for s in seqs])
    finally:
        h.close()
    for b, s in enumerate(seqs):
        md = models[s["m"]]
        h1 = _lib.Handle(md["sk"], md["cams"], md["opts"])
        try:
            ref = h1.solve_kinetic_tracked_host(md["ko"], s["q_init"][None], s["q_target"][None], s["stance"][None], s["meas"][None], s["weight"][None])
        finally:
            h1.close()
        for k in FIELDS + ("meas_err",):
            assert np.array_equal(out[k][b], ref[k][0]), (b, k)
        for f in STATS:
            assert getattr(out["stats"][b], f) == getattr(ref["stats"][0], f), (b, f)
        for f in KSTATS:
            assert getattr(out["kstats"][b], f) == getattr(ref["kstats"][0], f), (b, f)
    assert not out["padded"]["q"][0, lens[0]:].any()


def test_estimate_kinetics_without_2d_reprojections_end_to_end(tmp_path):
    """write_dataset -> estimate_kinematics -> estimate_kinetics(use_2d_reprojections=False): inverse dynamics of the stored kinematic solution,
    through files; the batch entry (ragged) writes the same numbers"""
    from cheetah_pose_estimation_amd import estimator as E
    from dataset_util import write_dataset
    info = write_dataset(str(tmp_path), N=48, noise_px=0.5, gallop=True)
    est = E.init_trajectory(str(tmp_path), info["data_path"], "phantom", False, solver_path="/unused/ipopt", kinematic_model=True)
    assert E.estimate_kinematics(est, solver_output=False) is True
    mk = lambda: E.init_trajectory(str(tmp_path), info["data_path"], "phantom", False, solver_path="/unused/ipopt", enable_eom_slack=True,
                                   bound_eom_error=(-2.0, 2.0), include_camera_constraints=True, kinematic_model=False)
    est2 = mk()
    kin = E.load_result_pickle(os.path.join(str(tmp_path), info["data_path"], "fte_kinematic", "fte.pickle"))
    fps = est2.scene.fps
    p = E._kinetic_prepare(est2, False, False, True, False, True, True, True, False, False, False, None, None, None)
    assert p["tracked"] and np.array_equal(p["q_target"], kin["q"][:48]) and p["ko"].w_smooth == 0.0 and p["ko"].w_torque == 1.0 + 1e-3 / fps ** 2
    p0 = E._kinetic_prepare(est2, False, False, True, False, True, True, True, False, False, True, None, None, None)
    assert p0["ko"].w_smooth == 0.0 and p0["ko"].w_torque == 0.0
    assert not E._kinetic_prepare(est2, False, True, True, False, True, True, True, False, False, False, None, None, None)["tracked"]
    kw = dict(init_torques=False, init_prev_kinematic_solution=True, solver_output=False, auto=False, joint_estimation=True, use_2d_reprojections=False)
    ok = E.estimate_kinetics(est2, **kw)
    st = est2.result["stats"][0]
    print(f"tracked end to end: status {st.status}, {st.iterations} iterations / {st.outer} updates, costs {est2.costs}")
    assert ok is True
    out_dir = os.path.join(str(tmp_path), info["data_path"], "fte_kinetic")
    d = E.load_result_pickle(os.path.join(out_dir, "fte.pickle"))
    assert d["q"].shape == (48, 54) and len(d["tau"]) == 16
    Tn, _, _ = _numpy_term(est2.skeleton, d["q"], kin["q"][:48], abi.default_track_weights())
    assert abs(est2.costs["measurement"] - Tn.sum()) <= 1e-9 * max(1.0, Tn.sum())
    assert est2.costs["energy"] == 1e-2 * est2.costs["torque"] and est2.costs["torque"] > 0.0
    # the batch entry, ragged: the same numbers
    est3 = mk()
    assert E.estimate_kinetics_batch([est3], out_fname="fte_batch", ragged=True, **kw) == [True]
    d3 = E.load_result_pickle(os.path.join(out_dir, "fte_batch.pickle"))
    for k in ("q", "dq", "ddq", "positions", "meas_err"):
        assert np.array_equal(np.asarray(d3[k]), np.asarray(d[k])), k
    for k in d["tau"]:
        assert np.array_equal(d3["tau"][k], d["tau"][k]), k
    assert est3.costs == est2.costs
    # the batch entry, plain (one group of one sequence): every array of the pickle
    est4 = mk()
    assert E.estimate_kinetics_batch([est4], out_fname="fte_plain_batch", ragged=False, **kw) == [True]
    d4 = E.load_result_pickle(os.path.join(out_dir, "fte_plain_batch.pickle"))
    assert set(d4) == set(d) and {"q", "dq", "ddq", "positions", "meas_err", "x", "dx", "ddx", "com_pos", "com_vel", "tau"} <= set(d)
    for k, v in d.items():
        if isinstance(v, (np.ndarray, list)):
            assert np.array_equal(np.asarray(d4[k]), np.asarray(v)), k
    assert set(d4["tau"]) == set(d["tau"])
    for k in d["tau"]:
        assert np.array_equal(d4["tau"][k], d["tau"][k]), k
    assert est4.costs == est2.costs
