"""Reference side of the length-calibration tests (cpe_scale_system, include/cpe.h; DESIGN.md 2 "What is calibrated").  Helper, not a test module.

The unknowns beside the poses: one scale s_g per segment group.  Marker positions are linear in the scales, so Ds = d p / d s_g =
p(s + e_g) - p(s) exactly: two forward kinematics (synth.fk_numpy) at the same consistent q, the second on a skeleton whose `attach` and
`marker_off` are moved by the derivative tables (skeleton.length_derivatives; tests/test_length_scale_host.py holds the tables against
build_skeleton(length_scale=)).  Jp = d pixel / d p [F, C, L, 2, 3] by frame_compare's extrapolated five-point quotient on synth.project_numpy,
Js = Jp Ds.  Pixels, loss, gradient weight gw = rho' m w, curvature weight cww = kappa (m w)^2 and Ju = d pixel / d u come from
frame_compare.evaluate (np.longdouble).  Per frame
    A_n = sum cww Js^T Js [G, G]      b_n = sum gw Js [G]      E_n = sum cww Ju^T Js [28, G]
and per sequence A = sum A_n, b = sum b_n, A_red = A - E^T Hd^-1 E, b_red = b - E^T Hd^-1 g with Hd = H + ridge diag(max(diag H, floor)) DENSE
(scipy Cholesky, float64).  H and g: the oracle's band and gradient (oracle.objective) with the oracle's own per-frame blocks
(oracle.frame_normal, whose d Euler / d u is a difference quotient) taken out and frame_compare's extended ones put in; what stays of the
oracle is the motion model and the motion prior, which are constant matrices.

Units of discrepancies(G, R), worst over frames / sequences and entries, inf for a non-finite value, and where a scale is exactly zero the
value must be exactly zero (a group no marker depends on):
  A, A_red        sqrt(S_gg S_hh), S = the diagonal of the reference's A + FLOOR x the same sum with frame_compare's absolute loss terms
  b               sum |gw| |Js| (+ FLOOR x the absolute form)
  b_red           b's scale + |E|^T |Hd^-1 g| (what is summed to form it)
  sym             A - A^T and A_red - A_red^T: 0 or inf
  cost            the reference's |value|

Tolerances.  tolerance(case)[key] = MARGIN (32, frame_compare's) x the larger of two numbers measured ON THE CPU on the inputs of THAT case of
tests/test_gpu_scale_system.py (MEASURED below; `python -m tests.scale_compare` prints it; tests/test_length_scale_host.py re-measures two cases
and holds them against it); nothing of the kernel's output enters them:
  1  the float64 evaluation of this reference at q against itself at q moved by one ulp per entry (frame_compare.ulp_spread's rule), which for
     A_red and b_red includes the dense solve's sensitivity; plus, for those two, the Cholesky route against numpy's LU solve on the same matrix
  2  the float64 evaluation against the np.longdouble one
Per case because the cases differ by two decades: A_red and b_red spread by 1.1e-11 and 1.1e-10 on the pinhole rig (four narrow cameras on one
side pair: the depth directions of H are weak and one ulp of q shows in Hd^-1) and by at most 7e-12 and 1.8e-12 on every other case; one
tolerance for all would be fifty times too wide on twelve of the thirteen.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_compare as FC                                                          # noqa: E402
import lm_compare as LC                                                             # noqa: E402
from cheetah_pose_estimation_amd import abi, priors, skeleton, synth               # noqa: E402

NX = abi.NX
MARGIN = FC.MARGIN
FLOOR = FC.FLOOR
KEYS = ("A", "b", "A_red", "b_red", "sym", "cost")
MEASURED_KEYS = ("A", "b", "A_red", "b_red", "cost")

# per case and key the larger of (measurement 1, measurement 2): CPU only, see the module docstring (`python -m tests.scale_compare` prints this)
MEASURED = {
    'plain': dict(A=3.83e-15, b=8.46e-15, A_red=1.72e-12, b_red=4.88e-13, cost=6.06e-16),
    'n1': dict(A=3.93e-14, b=5.82e-14, A_red=2.38e-15, b_red=3.92e-15, cost=4.48e-16),
    'n2': dict(A=4.94e-15, b=7.89e-15, A_red=2.53e-14, b_red=6.16e-15, cost=1.68e-15),
    'ragged': dict(A=2.70e-15, b=2.84e-14, A_red=1.68e-12, b_red=3.26e-13, cost=3.70e-15),
    'cams1': dict(A=1.20e-14, b=3.67e-14, A_red=6.95e-12, b_red=1.75e-12, cost=9.52e-16),
    'cams18': dict(A=1.17e-15, b=4.82e-15, A_red=4.03e-13, b_red=1.50e-13, cost=7.67e-16),
    'g1': dict(A=1.07e-15, b=7.31e-15, A_red=1.14e-12, b_red=1.03e-12, cost=4.77e-16),
    'g16': dict(A=1.93e-15, b=1.13e-14, A_red=1.82e-12, b_red=9.21e-13, cost=4.13e-16),
    'zero_camera': dict(A=3.01e-15, b=1.03e-14, A_red=2.61e-12, b_red=1.37e-12, cost=2.91e-16),
    'loss_c1': dict(A=1.02e-14, b=1.60e-14, A_red=6.53e-13, b_red=5.27e-13, cost=5.09e-16),
    'pinhole': dict(A=3.30e-15, b=4.50e-14, A_red=1.14e-11, b_red=1.05e-10, cost=2.90e-16),
    'prior': dict(A=1.49e-15, b=2.24e-14, A_red=9.09e-13, b_red=1.79e-12, cost=3.69e-16),
    'batch3': dict(A=3.18e-15, b=1.54e-14, A_red=9.92e-13, b_red=5.07e-13, cost=1.68e-15),
}



def tolerance(name):
    """TOL of a case: MARGIN x the reference's own spread on that case's inputs; sym is exact"""
    return dict({k: MARGIN * v for k, v in MEASURED[name].items()}, sym=0.0)


# the groups of the GPU cases: the packaged eleven; one scale for the whole animal; sixteen = the trunk links, the two sides of every thigh and
# calf on their own, the hocks in pairs, and one group without a link (no marker depends on it)
G1 = (("all", tuple(skeleton.LINKS)),)
G16 = (tuple(skeleton.LENGTH_GROUPS[:5]) + tuple((n, (n,)) for n in ("UFL", "UFR", "LFL", "LFR", "UBL", "UBR", "LBL", "LBR"))
       + (("front_hock", ("HFL", "HFR")), ("back_hock", ("HBL", "HBR")), ("none", ())))
GROUPS = {1: G1, 11: skeleton.LENGTH_GROUPS, 16: G16}


def shifted(sk, d_attach, d_marker_off):
    """copy of skeleton sk with `attach` and `marker_off` moved by one group's derivative tables: the skeleton at s + e_g"""
    out = abi.Skeleton.from_buffer_copy(bytes(sk))
    for i in range(sk.n_links):
        for d in range(3):
            out.attach[i][d] = sk.attach[i][d] + d_attach[i][d]
    for l in range(sk.n_markers):
        for d in range(3):
            out.marker_off[l][d] = sk.marker_off[l][d] + d_marker_off[l][d]
    return out


def position_derivatives(sk, d_attach, d_marker_off, q):
    """Ds [F, L, 3, G] = p(s + e_g) - p(s) at consistent Euler q [F, nq], in q's dtype"""
    p0 = synth.fk_numpy(sk, q)[0]
    return np.stack([synth.fk_numpy(shifted(sk, d_attach[g], d_marker_off[g]), q)[0] - p0 for g in range(d_attach.shape[0])], axis=-1)


def projection_jacobian(cams, pos, fd_h=FC.FD_H):
    """Jp [F, C, L, 2, 3] = d pixel / d position at pos [F, L, 3]: frame_compare's extrapolated five-point quotient"""
    dt = pos.dtype.type
    steps = np.array([k * s for s in (1.0, 0.5) for k in (-2, -1, 1, 2)], dtype=pos.dtype) * dt(fd_h)
    F, L = pos.shape[:2]
    pp = np.broadcast_to(pos[:, None, None], (F, 3, 8, L, 3)).copy()
    for a in range(3):
        pp[:, a, :, :, a] += steps[:, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        uv = np.stack([synth.project_numpy(cams[c], pp)[0] for c in range(len(cams))], axis=3)            # [F, 3, 8, C, L, 2]
    return np.moveaxis(FC.stencil_quotient(uv, dt(fd_h)), 1, -1)


def frame_terms(sk, cams, opts, pr, qc, meas, weight, d_attach, d_marker_off, dtype=np.longdouble, stencil=None):
    """the per-frame pieces at consistent Euler qc [F, nq]: dict(A_n [F, G, G], b_n [F, G], E_n [F, 28, G], their scales, cost [F], E = the
    frame_compare.evaluate result they are built on), everything in `dtype` (stencil: the precision of the difference quotients alone)"""
    E = FC.evaluate(sk, cams, opts, pr, qc, meas, weight, dtype, stencil=stencil)
    q = E["q"]
    Ds = position_derivatives(sk, np.asarray(d_attach), np.asarray(d_marker_off), q)
    pos = synth.fk_numpy(sk, q)[0]
    sd = dtype if stencil is None else stencil
    Jp = projection_jacobian(cams, pos.astype(sd)).astype(dtype)
    on = (E["w"] != 0)[..., None, None]
    Js = np.where(on, np.einsum("fclda,flag->fcldg", Jp, Ds), 0)
    cww, gw, Ju = E["cww"], E["gw"], E["J"]
    out = dict(A_n=np.einsum("fcldg,fcldh->fgh", Js * cww[..., None], Js), b_n=np.einsum("fcld,fcldg->fg", gw, Js),
               E_n=np.einsum("fcldk,fcldg->fkg", Ju * cww[..., None], Js), cost=E["cost"][:, 0], E=E)
    S = np.einsum("faa->fa", out["A_n"]) + FLOOR * np.einsum("fcld,fcldg->fg", E["cwwa"], Js * Js)
    Bd = np.einsum("fcld,fcldk->fk", cww, Ju * Ju) + FLOOR * np.einsum("fcld,fcldk->fk", E["cwwa"], Ju * Ju)
    out.update(S=S, A_n_scale=np.sqrt(S[:, :, None] * S[:, None, :]), E_n_scale=np.sqrt(Bd[:, :, None] * S[:, None, :]),
               b_n_scale=np.einsum("fcld,fcldg->fg", np.abs(gw), np.abs(Js)) + FLOOR * np.einsum("fcld,fcldg->fg", E["gwa"], np.abs(Js)))
    return out


def band_with_frames(oracle, sk, cams, opts, pr, q, meas, weight, ridge, E):
    """(Hd dense [N 28, N 28], g [N 28], consistent q) of one sequence at damping ridge: the oracle's band and gradient with its per-frame blocks
    replaced by those of frame_compare.evaluate's result E (float64 from here on)"""
    N = q.shape[0]
    PB = LC.solver_pb(pr)
    _, g0, H, _, qc = oracle.objective(sk, cams, opts, pr, q, meas, weight, want_grad=True, want_H=True)
    R = dict(zip(("Bk", "Hk"), LC._blocks_from_band(H, N, PB)), g=g0.reshape(N, NX), q=qc)
    fo = [oracle.frame_normal(sk, cams, opts, pr, q[n], meas[n], weight[n]) for n in range(N)]
    Bk = R["Bk"] - np.stack([o[1] for o in fo]) + np.asarray(E["Bm"], dtype=np.float64)
    Bk = 0.5 * (Bk + np.swapaxes(Bk, 1, 2))
    g = R["g"] - np.stack([o[0] for o in fo]) + np.asarray(E["g"], dtype=np.float64)
    Ad = Bk.copy()
    idx = np.arange(NX)
    Ad[:, idx, idx] += ridge * np.maximum(np.diagonal(Bk, axis1=1, axis2=2), LC.diag_floor(N))
    return LC.dense(Ad, R["Hk"]), g.reshape(-1), R["q"]


def reduce_system(T, Hd, g, route="cholesky"):
    """the per-sequence outputs from frame_terms' result T of ONE sequence and its dense damped matrix: dict(A, b, A_red, b_red, cost, scales)"""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    N, G = T["b_n"].shape
    Em = f64(T["E_n"]).reshape(N * NX, G)
    rhs = np.concatenate([Em, g[:, None]], axis=1)
    if route == "cholesky":
        from scipy.linalg import cho_factor, cho_solve
        X = cho_solve(cho_factor(Hd, lower=True), rhs)
    else:
        X = np.linalg.solve(Hd, rhs)
    A, b = f64(T["A_n"].sum(axis=0)), f64(T["b_n"].sum(axis=0))
    Ar = A - Em.T @ X[:, :G]
    S = f64(T["S"].sum(axis=0))
    return dict(A=A, b=b, A_red=0.5 * (Ar + Ar.T), b_red=b - Em.T @ X[:, G], cost=float(f64(T["cost"]).sum()),
                A_scale=np.sqrt(S[:, None] * S[None, :]), b_scale=f64(T["b_n_scale"].sum(axis=0)),
                b_red_scale=f64(T["b_n_scale"].sum(axis=0)) + np.abs(Em).T @ np.abs(X[:, G]))


def reference(oracle, sk, cams, opts, pr, q_list, meas_list, weight_list, d_attach, d_marker_off, ridge, dtype=np.longdouble, stencil=None,
              route="cholesky"):
    """the reference of a batch of sequences (lists of q [N_b, nq], meas [N_b, C, L, 2], weight [N_b, C, L]): dict of per-sequence lists A, b,
    A_red, b_red, cost and their scales (seq), and frames = frame_terms' result of every sequence.  sk, d_attach, d_marker_off: one for all, or a
    list with every sequence's own (a ragged batch over several models); cams: one rig, or a python list of every sequence's rig"""
    out = dict(frames=[], seq=[])
    each = lambda v, b: v[b] if isinstance(v, (list, tuple)) else v
    for b, (q, meas, weight) in enumerate(zip(q_list, meas_list, weight_list)):
        skb, da, dm = each(sk, b), each(d_attach, b), each(d_marker_off, b)
        cb = cams[b] if isinstance(cams, list) else cams
        q = np.ascontiguousarray(q, dtype=np.float64)
        qc = FC.consistent_q(oracle, skb, q)
        T = frame_terms(skb, cb, opts, pr, qc, meas, weight, da, dm, dtype, stencil)
        Hd, g, _ = band_with_frames(oracle, skb, cb, opts, pr, q, meas, weight, ridge, T["E"])
        out["frames"].append(T)
        out["seq"].append(reduce_system(T, Hd, g, route))
    return out


def discrepancies(G, R):
    """worst value of every key: G = dict(A, b, A_red, b_red, cost: one entry per sequence) of HIP, R = reference(...).  (The per-frame record
    A_n, b_n, E_n is not an output of cpe_scale_system: a sequence of one frame has A = A_n and b = b_n, and E_n enters A_red and b_red.)"""
    out = {}
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    worst = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), v))
    for bq, (T, S) in enumerate(zip(R["frames"], R["seq"])):
        worst("A", FC._ratio(G["A"][bq], S["A"], S["A_scale"]))
        worst("b", FC._ratio(G["b"][bq], S["b"], S["b_scale"]))
        worst("A_red", FC._ratio(G["A_red"][bq], S["A_red"], S["A_scale"]))
        worst("b_red", FC._ratio(G["b_red"][bq], S["b_red"], S["b_red_scale"]))
        worst("cost", FC._ratio(np.asarray(G["cost"][bq]), S["cost"], abs(S["cost"])))
        asym = max(np.abs(np.asarray(G[k][bq]) - np.asarray(G[k][bq]).T).max() for k in ("A", "A_red"))
        worst("sym", 0.0 if asym == 0.0 and np.all(np.isfinite(G["A_red"][bq])) else float("inf"))
    return out


def failures(d, tol):
    return {k: d[k] for k in KEYS if k in d and not d[k] <= tol[k]}


def outputs(R):
    """a reference's numbers in the kernel's layout and float64"""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    return {k: [f64(S[k]) for S in R["seq"]] for k in ("A", "b", "A_red", "b_red", "cost")}


# ---- the inputs of the GPU cases (shared with the CPU test, which re-measures the tolerances on them) -----------------------------------------
def _pinhole_setup():
    from test_gpu_parity import _kinetic_setup
    return _kinetic_setup()


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """dict(opts, pr, groups, ridge; sk, cams, d_attach, d_marker_off, q, meas, weight = lists with one entry per sequence; models = the
    (sk, d_attach, d_marker_off, cams) of the handle's models, model = the model of every sequence) of a case.  The poses are
    the truth of a synthetic run + N(0, 0.02), the measurements frame_compare.observe's (every camera holds inliers), on a skeleton whose groups are
    scaled by 1 + U(-0.08, 0.08): the state in which the calibration calls the entry."""
    n_markers, n_cams, G, lens, prior, curvature, ridge, rig = dict(
        plain=(25, 6, 11, (5,), None, 0, 0.0, "fisheye"),
        n1=(24, 6, 11, (1,), None, 0, 1e-6, "fisheye"),
        n2=(24, 6, 11, (2,), None, 0, 1e-6, "fisheye"),
        ragged=(24, 6, 11, (5, 2), None, 0, 1e-6, "fisheye"),
        cams1=(24, 1, 11, (5,), None, 0, 1e-6, "fisheye"),
        cams18=(25, 18, 11, (5,), None, 0, 0.0, "fisheye"),
        g1=(24, 6, 1, (5,), None, 0, 0.0, "fisheye"),
        g16=(25, 6, 16, (5,), None, 0, 0.0, "fisheye"),
        zero_camera=(25, 6, 11, (5,), None, 0, 0.0, "fisheye"),
        loss_c1=(25, 6, 11, (5,), None, 1, 0.0, "fisheye"),
        pinhole=(24, 4, 11, (5,), None, 0, 0.0, "pinhole"),
        prior=(24, 2, 11, (5,), "packaged", 0, 1e-6, "fisheye"),
        batch3=(25, 6, 11, (5, 5, 5), None, 0, 0.0, "fisheye"))[name]
    groups = GROUPS[G]
    seed = 5000 + sorted(("plain", "n1", "n2", "ragged", "cams1", "cams18", "g1", "g16", "zero_camera", "loss_c1", "pinhole", "prior", "batch3")).index(name)
    scale = 1.0 + np.random.default_rng(seed).uniform(-0.08, 0.08, G)
    opts, fps, kin, first = abi.default_options(), 120.0, False, 0
    if rig == "pinhole":
        # the kinetic-dataset rig: four pinhole cameras with radial distortion and multipliers (1, 1, 0.6, 0.6), an `-02` skeleton, 200 fps,
        # half a second into the run (on the images of all four cameras), as frame_compare's case "knots"
        cams = _pinhole_setup()[1]
        opts, fps, kin, first = abi.default_options(200.0), 200.0, True, 100
        sk = skeleton.build_skeleton("arabia-02", n_markers, kinetic_dataset=True, length_scale=scale, groups=groups)
        d_attach, d_marker_off = skeleton.length_derivatives("arabia-02", n_markers, groups)
    else:
        sk = skeleton.build_skeleton("phantom", n_markers, length_scale=scale, groups=groups)
        d_attach, d_marker_off = skeleton.length_derivatives("phantom", n_markers, groups)
        cams = (abi.Camera * 1)(synth.make_cameras(6)[2]) if n_cams == 1 else (synth.make_cameras(n_cams) if n_cams in (2, 6) else FC.cyclic_cameras(n_cams))
    opts.curvature = curvature
    pr = None if prior is None else FC.load_prior(prior)
    # the ragged pair: its second sequence belongs to a second model -- another animal's lengths and tables, and a rig of two cameras beside the
    # first model's six, so that the batch's camera stride is not the model's camera count
    models = [(sk, d_attach, d_marker_off, cams)]
    if name == "ragged":
        s2 = 1.0 + np.random.default_rng(seed + 1).uniform(-0.08, 0.08, G)
        models.append((skeleton.build_skeleton("jules", n_markers, length_scale=s2, groups=groups),) + skeleton.length_derivatives("jules", n_markers, groups)
                      + (synth.make_cameras(2),))
    model = [min(b, len(models) - 1) for b in range(len(lens))]
    qs, ms, ws = [], [], []
    for b, n in enumerate(lens):
        sk, cams = models[model[b]][0], models[model[b]][3]
        qt = synth.truth_trajectory(sk, first + n, fps, np.random.default_rng(seed + 10 + b))[first:]
        q = qt + np.random.default_rng(seed + 20 + b).normal(0, 0.02 if prior is None else 0.01, qt.shape)
        meas, weight = FC.observe(sk, cams, qt, seed + 30 + b, kin)
        weight = FC.clear_near(sk, cams, q, weight)
        if name == "zero_camera":
            weight[:, 3] = 0.0; meas[:, 3] = 0.0
        qs.append(q); ms.append(np.ascontiguousarray(meas)); ws.append(np.ascontiguousarray(weight))
    per = lambda i: [models[m][i] for m in model]
    return dict(sk=per(0), cams=per(3), opts=opts, pr=pr, groups=groups, scale=scale, d_attach=per(1), d_marker_off=per(2), q=qs, meas=ms, weight=ws,
                ridge=ridge, models=models, model=model)


CASES = ("plain", "n1", "n2", "ragged", "cams1", "cams18", "g1", "g16", "zero_camera", "loss_c1", "pinhole", "prior", "batch3")


@functools.lru_cache(maxsize=None)
def case_reference(oracle, name):
    c = case_inputs(name)
    return reference(oracle, c["sk"], c["cams"], c["opts"], c["pr"], c["q"], c["meas"], c["weight"], c["d_attach"], c["d_marker_off"], c["ridge"])


def _merge(worst, d):
    for k, v in d.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return worst


def measure_case(oracle, name, draws=2, seed=0):
    """(measurement 1, measurement 2) of a case, per key"""
    c = case_inputs(name)
    args = (c["sk"], c["cams"], c["opts"], c["pr"])
    tabs = (c["d_attach"], c["d_marker_off"], c["ridge"])
    R = case_reference(oracle, name)
    qc = [np.asarray(T["E"]["q"], dtype=np.float64) for T in R["frames"]]
    R64 = reference(oracle, *args, qc, c["meas"], c["weight"], *tabs, dtype=np.float64, stencil=np.longdouble)
    m2 = discrepancies(outputs(R64), R)
    m1 = discrepancies(outputs(reference(oracle, *args, qc, c["meas"], c["weight"], *tabs, dtype=np.float64, stencil=np.longdouble, route="lu")), R64)
    rng = np.random.default_rng(seed)
    for _ in range(draws):
        q1 = [np.nextafter(q, np.where(rng.random(q.shape) < 0.5, -np.inf, np.inf)) for q in qc]
        _merge(m1, discrepancies(outputs(reference(oracle, *args, q1, c["meas"], c["weight"], *tabs, dtype=np.float64, stencil=np.longdouble)), R64))
    return m1, m2


# ---- the calibration experiment ("What is calibrated"): shared by the CPU loop test and the GPU calibration test ----------------
EXPERIMENT_SCALE = 1.0 + np.random.default_rng(7).uniform(-0.08, 0.08, len(skeleton.LENGTH_GROUPS))
ORACLE_GOLDEN = os.path.join(FC.GOLDEN, "length_calibration_oracle.npz")


def experiment_data(B=1, noisy=False, n_cams=6):
    """phantom with every group off by EXPERIMENT_SCALE (up to 8 %), synth.make_cameras(6) (n_cams = 1: its second camera, which has the animal on
    its image in these frames -- as the first has, and none of the other four), B sequences of N = 16
    from synth.make_batch: clean detections, or 2 px of noise and 10 % outliers.  dict(sk_true, cams, q_init, meas, weight [B, ...])"""
    sk_true = skeleton.build_skeleton("phantom", 24, length_scale=EXPERIMENT_SCALE)
    c6 = synth.make_cameras(6)
    cams = c6 if n_cams == 6 else (abi.Camera * 1)(c6[1])
    d = synth.make_batch(sk_true, cams, B, N=16, **({} if noisy else dict(noise_px=0.0, outlier_frac=0.0)))
    return dict(sk_true=sk_true, cams=cams, q_init=d["q_init"], meas=d["meas"], weight=d["weight"])


def oracle_calibration(oracle, data, prior_sigma=0.1, tol=1e-6, max_rounds=30):
    """estimator.calibrate_loop driven by oracle.solve and this module's reduced system over the sequences of experiment_data's dict, from s = 1:
    (the loop's result, J_true = the total objective at the true lengths with re-solved poses)"""
    from cheetah_pose_estimation_amd import estimator as E
    opts = abi.default_options()
    da, dm = skeleton.length_derivatives("phantom", 24)
    build = lambda s: skeleton.build_skeleton("phantom", 24, length_scale=s)
    B = data["meas"].shape[0]

    def solve(s, state):
        sk = build(s)
        rs = [oracle.solve(sk, data["cams"], opts, None, data["q_init"][b] if state is None else state[b], data["meas"][b], data["weight"][b]) for b in range(B)]
        return sum(r["stats"].cost for r in rs) / opts.cost_scale, [r["q"] for r in rs]

    def system(s, state):
        R = reference(oracle, build(s), data["cams"], opts, None, state, list(data["meas"]), list(data["weight"]), da, dm, 0.0, dtype=np.float64,
                      stencil=np.longdouble)["seq"]
        return sum(S["A_red"] for S in R), sum(S["b_red"] for S in R)

    r = E.calibrate_loop(solve, system, len(skeleton.LENGTH_GROUPS), prior_sigma, None, tol, max_rounds)
    J_true = solve(EXPERIMENT_SCALE, None)[0] + 0.5 * ((EXPERIMENT_SCALE - 1.0) ** 2).sum() / prior_sigma ** 2
    return r, J_true


if __name__ == "__main__":
    from oracle import oracle as O
    O.lib()
    print("MEASURED = {")
    for name in CASES:
        m1, m2 = measure_case(O, name)
        print(f"    {name!r}: dict(" + ", ".join(f"{k}={max(m1[k], m2[k]):.2e}" for k in MEASURED_KEYS) + "),", flush=True)
    print("}")
