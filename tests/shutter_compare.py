"""Entry-by-entry comparison of cpe_eval_shutter_step's outputs -- the shutter-delay branch of k_frame_normal (g, Bm, cost, gx, rcb), k_lm_step's
collection of gx (g_total), k_shutter_step (step) and k_finalize with delays (meas_err) -- with an extended-precision reference that shares no
derivative code with the oracle or the kernel.  Helper of the tests, not a test module; built on the pieces of tests/frame_compare.py.

The model is one function.  Camera c sees marker l of frame n at

    proj_c( p_l(u_n) + s_c + [n >= 2] (alpha_c x_n + beta_c x_n-1 + gamma_c x_n-2) ),

x = the base position (reduced coordinates 0..2), alpha = tau/h + tau^2/h^2, beta = -tau/h - 2 tau^2/h^2, gamma = tau^2/h^2, s_c a free 3-vector
evaluated at 0, n the index inside the frame's own sequence.  make_view() differences it with frame_compare's extrapolated five-point stencil
with respect to 37 columns -- u_n (28), x_n-1 (3), x_n-2 (3), s (3); the groups "u", "x", "s" are selectable, the columns of a group that was
left out are zero and the keys that need them are not compared -- and frame_compare.evaluate() turns the first 28 into g, Bm and cost with its own
loss, bounds and prior.  From the same Jacobian and loss weights (gw = rho' w, cw w^2):

  cost, g, Bm, sym   as in frame_compare, same scales; sym over every frame (the shutter terms arrive by LDS atomics: no frame is exact)
  gx [6]             sum gw J[28:34]; exactly 0 for n < 2               scale sum |gw| |J| + FLOOR of the same sum with the loss's terms absolute
  rcb [c][0:3]       sum_l gw J_s over camera c's pairs                 scale: the absolute sum + floor, per camera
  rcb [c][3:9]       upper triangle of sum_l J_s^T cw w^2 J_s           scale sqrt(M_aa M_bb), floor under the root
  step [c]           -G_c / H_c, G_c = sum_{n >= 2} t_n . rc_nc, H_c = sum t_n^T Mc_nc t_n, t_n = v_n + 2 a_n tau_c (backward differences of x);
                     step[0] = 0 exactly; 0 where H_c = 0            scale (sum_n sum_d |t_nd| |rc_nd|_abs) / H_c
  g_total            g_total_plain + (g_shutter - g_plain) + gx[m+1][0:3] + gx[m+2][3:6] (the last two on coordinates 0..2, where they exist):
                     g_total_plain = the oracle's total gradient at tau = 0 (oracle.objective: the motion model and the motion prior do not
                     depend on tau), the bracket and gx this module's        scale: the absolute sums of the parts + |g_total_plain|
  meas_err           the displaced pixel minus meas, at every pair more than 2 NEAR_Z in front of its camera        scale: absolute, pixels

Sums over frames (step) are math.fsum in the float64 evaluation and np.longdouble sums in the extended one.

Conditions (R["conditions"], asserted by every case; they are not tolerances): frame_compare.conditions_hold on the displaced residuals, and
where a case displaces anything (N >= 3, more than one camera, a non-zero delay): every camera c >= 1 has H_c > 0 and at least 40 weighted inlier
residuals in its frames n >= 2; |x_n - x_n-1| / h > 1 m/s in every displaced frame; max |tau| >= 0.3 h with delays of both signs; the displaced
pixels of the delayed cameras differ from the undisplaced ones by more than 1 px in the median (a kernel that ignored tau fails every key).

Tolerances, by frame_compare's rule: TOL[key] = MARGIN (32) x the larger of two numbers measured ON THE CPU over the inputs of every case of
tests/test_gpu_shutter_terms.py (CASES below); nothing of the kernel's output enters them:

  1  the spread of the float64 evaluation of this reference (stencil in np.longdouble, as in frame_compare) under a one-ulp change of every q,
     4 draws; for g_total the oracle is evaluated at the moved q too, so its finite-difference Z' (h = 1e-6) is part of the spread
  2  the distance between the float64 evaluation and the np.longdouble one

             measurement 1   measurement 2   TOL = 32 x the larger
  cost       1.20e-13        3.37e-14        3.85e-12
  g          5.68e-13        6.40e-13        2.05e-11
  Bm         1.63e-11        6.36e-12        5.22e-10
  gx         1.74e-13        5.71e-14        5.56e-12
  rcb        3.08e-11        1.20e-11        9.86e-10
  step       2.29e-12        8.85e-13        7.33e-11
  g_total    5.80e-11        3.37e-11        1.86e-09
  meas_err   1.82e-12        1.31e-12        5.82e-11

  cost, g and Bm land at frame_compare's values (3.85e-12, 1.73e-11, 7.56e-10).  Bm, rcb (its Mc entries) and step are set by case "knots-c0"; every
  other case stays below 2.4e-13 on Bm, 5.6e-13 on rcb and 6.1e-14 on step.  It is frame_compare's "knots" effect: with a = 2 the loss has
  rho'(0+) > 0, mode 0's weight rho'(|s|) / |s| grows as 0.03 / |s| towards 0, and one ulp of q moves the weight of a residual of |s| ~ 1e-3 by
  1e-11 of itself; Mc is a sum of such weights over one camera's 60 pairs, H_c inherits it and step = -G_c / H_c with it.  The kernel shares this.
  g_total: the oracle's Z' is a central difference at h = 1e-6, whose rounding noise (1e-16 / 1e-6) one ulp of q shows in full; the oracle's
  truncation error, 3.6e-10 of g's scale by frame_compare's record, is of the same order in g_total's wider scale

  (produced by `python -m tests.shutter_compare` from the repository root; tests/test_shutter_compare.py recomputes both and asserts that
  TOL / (1) lies in [16, 128] and (2) < TOL / 8)

The margin of 32 stands for what legitimately differs between kernel and reference on identical inputs -- the device sincos, FMA contraction, the
kernel's summation order and the order in which its LDS atomics arrive -- as argued in resjac_compare.py.

The oracle against this reference (oracle.objective_shutter, CPU only), worst over the cases with all column groups (ORACLE below):
  d f / d tau_c against G_c 5.3e-14 (step's scale times H_c), its gradient against g_total 5.2e-11 (short3; the plain parts of both are the
  oracle's own, so this is the distance of its shutter terms: frame_compare records 3.6e-10 for the whole per-frame g), its objective against the
  plain objective + the difference of the summed measurement costs 2.7e-16 of the objective.  tests/test_shutter_compare.py asserts each at 10 x
  the value recorded here.

The kernels' own worst values on an MI355X over every case of tests/test_gpu_shutter_terms.py (its test_zz_report), for the record; they never fed TOL:
  cost 8.3e-14 (cams1), g 3.4e-13 (bounds), Bm 2.3e-12 (knots-c0), sym 9.2e-17 (prior-packaged-c1), gx 5.9e-14 (motion), rcb 4.3e-12 (knots-c0),
  step 3.2e-13 (knots-c0), g_total 1.4e-10 (the same in nearly every case: the rounding of the oracle's Z' quotient on a coordinate whose gradient
  is the motion model's), meas_err 1.0e-12 px (prior-packaged-c1): each a factor 13 to 230 inside its tolerance
"""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import frame_compare as FC                                                          # noqa: E402
from cheetah_pose_estimation_amd import abi, skeleton, synth                       # noqa: E402

KEYS = ("cost", "g", "Bm", "sym", "gx", "rcb", "step", "g_total", "meas_err")
MEASURED_KEYS = ("cost", "g", "Bm", "gx", "rcb", "step", "g_total", "meas_err")
FRAME_KEYS = ("cost", "g", "Bm", "sym")                                              # need the columns of u; frame_compare computes them
NU = abi.NX
GROUPS = dict(u=range(0, NU), x=range(NU, NU + 6), s=range(NU + 6, NU + 9))
NCOL = NU + 9
ALL = ("u", "x", "s")
MARGIN, FLOOR, NEAR_Z = FC.MARGIN, FC.FLOOR, FC.NEAR_Z
MIN_SPEED = 1.0                # m/s of the base in every displaced frame
MIN_TAU = 0.3                  # max |tau| / h of a case
MIN_SHIFT_PX = 1.0             # median displacement of the delayed cameras' pixels
LAM = 1e-2                     # damping of the first pass (none of the compared outputs depends on it)

# (measurement 1, measurement 2) per key: CPU only, see the module docstring
MEASURED = dict(cost=(1.20e-13, 3.37e-14), g=(5.68e-13, 6.40e-13), Bm=(1.63e-11, 6.36e-12), gx=(1.74e-13, 5.71e-14), rcb=(3.08e-11, 1.20e-11),
                step=(2.29e-12, 8.85e-13), g_total=(5.80e-11, 3.37e-11), meas_err=(1.82e-12, 1.31e-12))
TOL = {k: MARGIN * max(v) for k, v in MEASURED.items()}
TOL["sym"] = TOL["Bm"]
# the oracle's distance from this reference, worst over the cases with all column groups (gt: d f / d tau_c against G_c in step's scale times
# H_c; g: its total gradient against g_total; f: its objective against the plain objective + the difference of the summed measurement costs)
ORACLE = dict(gt=5.30e-14, g=5.23e-11, f=2.68e-16)


# ---- the displaced view ----------------------------------------------------------------------------------------------------------------
def coefficients(tau, h, wrong=()):
    r = tau / h
    al, be, ga = r + r * r, -r - 2 * r * r, r * r
    if "alpha without its square" in wrong:
        al = r
    if "beta and gamma exchanged" in wrong:
        be, ga = ga, be
    return al, be, ga


def make_view(sk, cams, opts, tau, N, groups=ALL, wrong=()):
    """frame_compare.evaluate's `view` of B sequences of N frames (flattened, F = B N) under the delays tau [B, C]: (pixels, jacobian), plus
    parts(u) -> (displaced [F], x_n-1, x_n-2 [F, 3], alpha, beta, gamma [F, C], the last three zero where nothing is displaced)"""
    C, L = len(cams), sk.n_markers
    cols = [k for g in ALL if g in groups for k in GROUPS[g]]
    assert FC.tables(sk)[0][:3] == [0, 1, 2]                                         # the base position is reduced coordinates 0..2

    def parts(u):
        F = u.shape[0]
        assert F == tau.shape[0] * N
        n = np.arange(F) % N
        disp = np.arange(F) >= 2 if "the neighbour's frames" in wrong else n >= 2    # (wrong: frames 0, 1 of sequence 1 see sequence 0's last two)
        x = u[:, :3]
        x1, x2 = np.where(disp[:, None], np.roll(x, 1, axis=0), 0), np.where(disp[:, None], np.roll(x, 2, axis=0), 0)
        co = coefficients(np.repeat(np.asarray(tau).astype(u.dtype), N, axis=0), u.dtype.type(opts.h), wrong)
        return (disp, x1, x2) + tuple(np.where(disp[:, None], a, 0) for a in co)

    def shift(x, x1, x2, al, be, ga):
        """[..., C, 3] of x.. [..., 3] and al.. [..., C] (zero where nothing is displaced: exactly no shift there)"""
        return al[..., None] * x[..., None, :] + be[..., None] * x1[..., None, :] + ga[..., None] * x2[..., None, :]

    def project(pos, sh):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            pr = [synth.project_numpy(cams[c], pos + sh[..., c, None, :]) for c in range(C)]
        return np.stack([p[0] for p in pr], axis=-3), np.stack([p[1] for p in pr], axis=-2)

    def pixels(u):
        _, x1, x2, al, be, ga = parts(u)
        return project(synth.fk_numpy(sk, FC.q_of_u(sk, u))[0], shift(u[:, :3], x1, x2, al, be, ga))

    def jacobian(u, fd_h):
        dt = u.dtype.type
        F = u.shape[0]
        steps = np.array([k * s for s in (1.0, 0.5) for k in (-2, -1, 1, 2)], dtype=u.dtype) * dt(fd_h)
        _, x1, x2, al, be, ga = parts(u)
        e = lambda a: a[:, None, None]
        out = np.zeros((F, C, L, 2, NCOL), dtype=u.dtype)
        ucols, ocols = [k for k in cols if k < NU], [k for k in cols if k >= NU]
        if ucols:                                                                    # the frame's own coordinates: alpha x_n moves with them
            up = np.broadcast_to(e(u), (F, len(ucols), 8, NU)).copy()
            for i, k in enumerate(ucols):
                up[:, i, :, k] += steps
            f = project(synth.fk_numpy(sk, FC.q_of_u(sk, up))[0], shift(up[..., :3], e(x1), e(x2), e(al), e(be), e(ga)))[0]
            out[..., ucols] = np.moveaxis(FC.stencil_quotient(f, dt(fd_h)), 1, -1)
        if ocols:                                                                    # x_n-1, x_n-2 and s: the markers stay, the shift moves
            v = [np.broadcast_to(e(a), (F, len(ocols), 8, 3)).copy() for a in (x1, x2, np.zeros_like(x1))]
            for i, k in enumerate(ocols):
                v[(k - NU) // 3][:, i, :, (k - NU) % 3] += steps
            pos = synth.fk_numpy(sk, FC.q_of_u(sk, u))[0]
            f = project(e(pos), shift(e(u[:, :3]), v[0], v[1], e(al), e(be), e(ga)) + v[2][..., None, :])[0]
            out[..., ocols] = np.moveaxis(FC.stencil_quotient(f, dt(fd_h)), 1, -1)
        return out

    return pixels, jacobian, parts


def _fsum(a, dtype):
    """sum of every entry: math.fsum in float64, the np.longdouble sum otherwise"""
    return dtype(math.fsum(np.asarray(a, dtype=np.float64).ravel())) if np.dtype(dtype) == np.float64 else np.asarray(a).sum()


def newton_step(x, tau, h, rc, rc_abs, Mc, wrong=()):
    """(step, scale, H [B, C]) of base positions x [B, N, 3], delays tau [B, C], rc, rc_abs [B, N, C, 3], Mc [B, N, C, 3, 3]"""
    dt = x.dtype.type
    B, N = x.shape[:2]
    Cn = tau.shape[1]
    step, scale, H = (np.zeros((B, Cn), dtype=x.dtype) for _ in range(3))
    stop = min(N, 66) if "frames from 66 on left out" in wrong else N
    if stop < 3:
        return step, scale, H
    v = (x[:, 2:] - x[:, 1:-1]) / dt(h)
    a = (x[:, 2:] - 2 * x[:, 1:-1] + x[:, :-2]) / (dt(h) * dt(h))
    fac = 1 if "t without the factor 2" in wrong else 2
    t = (v[:, :, None, :] + fac * a[:, :, None, :] * tau.astype(x.dtype)[:, None, :, None])[:, :stop - 2]       # [B, stop - 2, C, 3]
    Gt, At = t * rc[:, 2:stop], np.abs(t) * rc_abs[:, 2:stop]
    Ht = np.einsum("snci,sncij,sncj->snc", t, Mc[:, 2:stop], t)
    for b in range(B):
        for c in range(1, Cn):
            G, A = _fsum(Gt[b, :, c], dt), _fsum(At[b, :, c], dt)
            H[b, c] = _fsum(Ht[b, :, c], dt)
            if H[b, c] > 0:
                step[b, c], scale[b, c] = -G / H[b, c], A / H[b, c]
    return step, scale, H


def evaluate(sk, cams, opts, pr, qc, meas, weight, tau, dtype=np.longdouble, groups=ALL, stencil=None, wrong=()):
    """the terms of B sequences at consistent Euler qc [B, N, nq] (meas [B, N, C, L, 2], weight [B, N, C, L]) under the delays tau [B, C], everything
    in `dtype`: frame_compare.evaluate's dict of the flattened frames (displaced view) plus gx, gx_scale [F, 6], rcb, rcb_scale [F, C, 9], step,
    step_scale, H [B, C], meas_err [F, C, L, 2], me_valid [F, C, L], x [B, N, 3], al [F, C].  wrong: deliberate errors (tests of the comparison's
    sensitivity)"""
    B, N = qc.shape[:2]
    C = len(cams)
    fl = lambda a: np.ascontiguousarray(np.asarray(a).reshape((-1,) + np.asarray(a).shape[2:]))
    tau = np.asarray(tau, dtype=np.float64)
    assert tau.shape == (B, C)
    pix, jac, parts = make_view(sk, cams, opts, tau, N, groups, wrong)
    E = FC.evaluate(sk, cams, opts, pr, fl(qc), fl(meas), fl(weight), dtype, stencil=stencil, view=(pix, jac))
    Jx, gw, gwa, cww, cwwa = E["Jx"], E["gw"], E["gwa"], E["cww"], E["cwwa"]
    al = parts(E["u"])[3]
    Jn, Js = Jx[..., NU:NU + 6], Jx[..., NU + 6:]
    gx = np.einsum("fcld,fclda->fa", gw, Jn)
    gx_scale = np.einsum("fcld,fclda->fa", np.abs(gw), np.abs(Jn)) + FLOOR * np.einsum("fcld,fclda->fa", gwa, np.abs(Jn))
    rc = np.einsum("fcld,fclda->fca", gw, Js)
    rc_abs = np.einsum("fcld,fclda->fca", np.abs(gw), np.abs(Js)) + FLOOR * np.einsum("fcld,fclda->fca", gwa, np.abs(Js))
    Mc = np.einsum("fclda,fcldb->fcab", Js * cww[..., None], Js)
    md = np.sqrt(np.einsum("fcaa->fca", Mc) + FLOOR * np.einsum("fcld,fclda->fca", cwwa, Js * Js))
    Mc_scale = md[..., :, None] * md[..., None, :]
    if "the previous camera's Mc" in wrong:
        Mc = np.roll(Mc, 1, axis=1)
    if "u" in groups and ("M2 weighted by alpha" in wrong or "E^T M1 Dp without its transpose" in wrong):
        # d pixel / d u_n = Jfix + alpha_c J_s E^T (E picks coordinates 0..2): J^T W J = Jfix^T W Jfix + T1 + T1^T + T2 with
        # T1 = E sum_c alpha_c J_s^T W Jfix (rows 0..2), T2 = E sum_c alpha_c^2 J_s^T W J_s E^T
        A = np.einsum("fclda,fcldb->fcab", Js * cww[..., None], Jx[..., :NU])        # J_s^T W J [F, C, 3, 28]
        A[..., :3] -= al[..., None, None] * Mc                                      # J_s^T W Jfix
        T1 = np.einsum("fc,fcab->fab", al, A)
        Bm = E["Bm"].copy()
        if "M2 weighted by alpha" in wrong:
            Bm[:, :3, :3] += np.einsum("fc,fcab->fab", al - al * al, Mc)
        else:
            Bm[:, :, :3] -= np.swapaxes(T1, 1, 2)
        E = dict(E, Bm=Bm)
    iu = np.triu_indices(3)
    rcb = np.concatenate([rc, Mc[..., iu[0], iu[1]]], axis=-1)
    rcb_scale = np.concatenate([rc_abs, Mc_scale[..., iu[0], iu[1]]], axis=-1)
    x = E["u"][:, :3].reshape(B, N, 3)
    r4 = lambda a: a.reshape((B, N) + a.shape[1:])
    step, step_scale, H = newton_step(x, tau, opts.h, r4(rc), r4(rc_abs), r4(Mc), wrong)
    me = E["uv"] - fl(meas).astype(dtype)
    valid = np.asarray(E["z"] > 2 * NEAR_Z) & np.all(np.isfinite(E["uv"]), axis=-1)
    return dict(E, gx=gx, gx_scale=gx_scale, rcb=rcb, rcb_scale=rcb_scale, step=step, step_scale=step_scale, H=H, meas_err=np.where(valid[..., None], me, 0),
                me_valid=valid, x=x, al=al, tau=tau, groups=tuple(groups), shape=(B, N))


def make_reference(E, qc, sk, cams, opts):
    """the comparator's form of evaluate()'s result (frame_compare.make_reference + the conditions of the displaced frames)"""
    B, N = E["shape"]
    R = FC.make_reference(E, qc.reshape(B * N, -1), opts)
    R["sym_exact"] = np.zeros(B * N, dtype=bool)                                     # the shutter terms arrive by atomics in every frame
    tau, h = E["tau"], opts.h
    n = np.arange(B * N) % N
    dis = n >= 2
    cond = dict(R["conditions"], displaced=bool(N >= 3 and len(cams) > 1 and np.any(tau != 0)))
    if cond["displaced"]:
        on = E["w"] != 0
        s = np.abs(E["s"]).astype(np.float64)
        cond["displaced_inliers"] = tuple(int(v) for v in ((s[dis] < opts.loss_c) & on[dis][..., None]).sum(axis=(0, 2, 3))[1:])
        cond["H_min"] = float(E["H"][:, 1:].min())
        x = E["x"].astype(np.float64)
        cond["speed_min"] = float((np.linalg.norm(x[:, 2:] - x[:, 1:-1], axis=-1) / h).min())
        cond["tau_max"] = float(np.abs(tau).max() / h)
        cond["tau_signs"] = (bool((tau > 0).any()), bool((tau < 0).any()))
        uv0 = FC.pixels(sk, cams, E["u"])[0]
        delayed = np.repeat(tau != 0, N, axis=0)[:, :, None] & on & dis[:, None, None]
        d = np.linalg.norm((E["uv"] - uv0).astype(np.float64), axis=-1)
        cond["shift_px"] = float(np.median(d[delayed]))
    R["conditions"] = cond
    return R


def conditions_hold(R):
    c = R["conditions"]
    ok = FC.conditions_hold(R)
    if c["displaced"]:
        ok = (ok and min(c["displaced_inliers"]) >= FC.MIN_CAMERA_INLIERS and c["H_min"] > 0 and c["speed_min"] > MIN_SPEED and c["tau_max"] >= MIN_TAU
              and all(c["tau_signs"]) and c["shift_px"] > MIN_SHIFT_PX)
    return bool(ok)


def collect(gx, N, wrong=()):
    """[F, 3]: what frame m's base position receives from frames m+1 (gx[0:3]) and m+2 (gx[3:6]) of its own sequence"""
    g4 = np.asarray(gx).reshape((-1, N, 6))
    a, b = (g4[..., 3:], g4[..., :3]) if "gx rows exchanged" in wrong else (g4[..., :3], g4[..., 3:])
    out = np.zeros(g4.shape[:2] + (3,), dtype=g4.dtype)
    out[:, :-1] += a[:, 1:]
    out[:, :-2] += b[:, 2:]
    return out.reshape(-1, 3)


def total_gradient(oracle, c, R, Rp, q, wrong=()):
    """(g_total, its scale) [F, 28] of case inputs c at Euler q [B, N, nq]: the oracle's total gradient at tau = 0 + this module's shutter parts
    (R: the displaced reference, Rp: frame_compare.evaluate of the same frames without delays and without prior)"""
    B, N = R["shape"]
    gp = np.concatenate([oracle.objective(c["sk"], c["cams"], c["opts"], c["pr"], q[b], c["meas"][b], c["weight"][b], want_grad=True)[1].reshape(N, NU)
                         for b in range(B)])
    g = gp.astype(R["g"].dtype) + (R["g_meas"] - Rp["g_meas"])
    scale = np.abs(gp) + R["g_scale"] + Rp["g_scale"] + FLOOR * Rp["g_floor"]
    g[:, :3] += collect(R["gx"], N, wrong)
    scale[:, :3] += collect(R["gx_scale"], N)
    return g, scale


def reference(oracle, c, dtype=np.longdouble, q=None, stencil=None, wrong=(), total=None):
    """the reference of case inputs c (case_inputs): consistent q by the oracle, evaluate(), make_reference(), and (total, by default where the
    case has the columns of u) g_total.  q: other Euler q in place of c["q"]"""
    q = np.ascontiguousarray(c["q"] if q is None else q, dtype=np.float64)
    B, N = q.shape[:2]
    qc = FC.consistent_q(oracle, c["sk"], q.reshape(B * N, -1)).reshape(q.shape)
    E = evaluate(c["sk"], c["cams"], c["opts"], c["pr"], qc, c["meas"], c["weight"], c["tau"], dtype, c["groups"], stencil, wrong)
    R = make_reference(E, qc, c["sk"], c["cams"], c["opts"])
    if total is None:
        total = "u" in c["groups"]
    if total:
        fl = lambda a: np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))
        Ep = FC.evaluate(c["sk"], c["cams"], c["opts"], None, fl(qc), fl(c["meas"]), fl(c["weight"]), dtype, stencil=stencil)
        R["g_total"], R["g_total_scale"] = total_gradient(oracle, c, R, Ep, qc, wrong)      # (the oracle at the consistent q: what every evaluation shares)
    return R


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def discrepancies(G, R, keys=KEYS):
    """worst value of the keys `keys` over the frames of R: G = cpe_eval_shutter_step's outputs with the frames flattened (outputs(), hip_outputs())"""
    out = {}
    if any(k in keys for k in FRAME_KEYS):
        assert "u" in R["groups"]
        d = FC.discrepancies(dict(g=G["g"], Bm=G["Bm"], cost=G["cost"]), R)
        out.update({k: d[k] for k in FRAME_KEYS if k in keys})
    for k in ("gx", "rcb", "step", "g_total"):
        if k in keys:
            out[k] = FC._ratio(G[k], R[k], R[k + "_scale"])
    if "meas_err" in keys:
        v = R["me_valid"]
        out["meas_err"] = FC._ratio(np.asarray(G["meas_err"])[v], R["meas_err"][v], 1.0)
    return out


def failures(d, tol=None):
    tol = tol or TOL
    return {k: d[k] for k in KEYS if k in d and not d[k] <= tol[k]}


def merge(worst, d):
    for k in KEYS:
        if k in d:
            worst[k] = max(worst.get(k, 0.0), d[k])
    return worst


def outputs(R):
    """a reference's numbers in cpe_eval_shutter_step's layouts (frames flattened) and float64: what a kernel would return"""
    return {k: np.asarray(R[k]).astype(np.float64) for k in ("g", "Bm", "cost", "gx", "rcb", "step", "g_total", "meas_err") if k in R}


def hip_outputs(h, c, lam=LAM, host=False):
    """cpe_eval_shutter_step of handle h on case inputs c: its outputs with the frames flattened [B N, ...] (step [B, C], seq [B, 8])"""
    if host:
        G = h.eval_shutter_step_host(c["q"], c["meas"], c["weight"], c["tau"], lam)
    else:
        import torch
        dev = torch.device("cuda", 0)
        T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
        Bn, Nn = c["q"].shape[:2]
        out = {k: torch.full(s, float("nan"), dtype=torch.float64, device=dev) for k, s in h._shutter_step_shapes(Bn, Nn).items()}
        seq = np.full((Bn, 8), np.nan)
        h.eval_shutter_step(T(c["q"]), T(c["meas"]), T(c["weight"]), T(c["tau"]), lam, seq, **out)
        h.synchronize()
        G = {k: v.cpu().numpy() for k, v in out.items()}
        G["seq"] = seq
    return {k: (v if k in ("step", "seq") else v.reshape((-1,) + v.shape[2:])) for k, v in G.items()}


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------------
CAMERA_COUNTS = (1, 2, 13, 14, 18)
PRIOR_CASES = tuple(f"prior-{p}-c{n}" for p in ("packaged", "k5_w6_lasso") for n in (1, 6))
SHORT = (1, 2, 3)
CASES = (("plain",) + tuple(f"short{n}" for n in SHORT) + tuple(f"cams{n}" for n in CAMERA_COUNTS) + ("knots-c0", "knots-c1") + PRIOR_CASES
         + ("motion", "bounds", "long", "zero"))
LONG_N = 70
TAU_SEEDS = dict(cams2=7101)   # the seed of a case's delays where 7000 + its place in CASES does not meet the conditions (two cameras: one delay per sequence, of either sign)


def draw_tau(seed, B, C, h):
    """delays in +-0.6 h, one set per sequence, the first camera the reference"""
    tau = np.random.default_rng(seed).uniform(-0.6 * h, 0.6 * h, (B, C))
    tau[:, 0] = 0.0
    return tau


def mixture_only(pr):
    """a copy of priors pr without its motion prior"""
    p = abi.Priors.from_buffer_copy(bytes(pr))
    p.lr_window = 0
    return p


def _noisy(sk, cams, seed, n_frames, B=2, fps=120.0, sd=0.02, keep=0.5):
    qt = FC.truths(sk, n_frames, seed, fps)[:B]
    q = qt + np.random.default_rng(seed + 1000).normal(0, sd, qt.shape)
    meas, weight = FC.observe(sk, cams, qt, seed + 2000, keep=keep)
    return q, meas, FC.clear_near(sk, cams, q, weight)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """dict(sk, cams, opts, pr, q [B, N, nq], meas, weight, tau [B, C], groups, keys) of a case"""
    groups, keys = ALL, KEYS
    if name in ("plain", "zero"):
        c = FC.case_inputs("plain")
    elif name.startswith("short"):                                                   # every pair kept: two frames still give each camera its 40 inliers
        sk, cams = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6)
        q, meas, weight = _noisy(sk, cams, 5100, int(name[5:]), keep=1.0)
        c = dict(sk=sk, cams=cams, opts=abi.default_options(), pr=None, q=q, meas=meas, weight=weight)
    elif name == "cams2":
        sk, cams = skeleton.build_skeleton("phantom", 25), FC.cyclic_cameras(2)
        q, meas, weight = FC._noisy(sk, cams, 4402)
        c = dict(sk=sk, cams=cams, opts=abi.default_options(), pr=None, q=q, meas=meas, weight=weight)
    elif name.startswith("cams") or name == "bounds":
        c = FC.case_inputs(name)
    elif name.startswith("knots-c"):
        c = FC.case_inputs("knots")
        c = dict(c, opts=FC.with_curvature(c["opts"], int(name[-1])))
    elif name.startswith("prior-"):                                                  # the mixture alone: g and Bm are not touched by k_lr_band
        _, p, n = name.split("-")
        c = FC.prior_inputs(p, int(n[1:]))
        c = dict(c, pr=mixture_only(c["pr"]))
    elif name == "motion":                                                           # both packaged priors: window 4, half-bandwidth 4
        sk, cams = skeleton.build_skeleton("phantom", 24), synth.make_cameras(6)
        qt = FC.truths(sk, 9, 43)
        q = qt + np.random.default_rng(5).normal(0, 0.01, qt.shape)
        q[..., 3] += 0.05
        meas, weight = FC.observe(sk, cams, qt, 4790)
        c = dict(sk=sk, cams=cams, opts=abi.default_options(), pr=FC.load_prior("packaged"), q=q, meas=meas, weight=FC.clear_near(sk, cams, q, weight))
        keys = ("gx", "rcb", "step", "g_total", "meas_err")
    elif name == "long":
        sk, cams = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6)
        q, meas, weight = _noisy(sk, cams, 5200, LONG_N, B=1)
        c = dict(sk=sk, cams=cams, opts=abi.default_options(), pr=None, q=q, meas=meas, weight=weight)
        groups, keys = ("x", "s"), ("gx", "rcb", "step", "meas_err")
    else:
        raise KeyError(name)
    c = {k: c[k] for k in ("sk", "cams", "opts", "pr", "q", "meas", "weight")}
    Bn, Cn = c["q"].shape[0], len(c["cams"])
    seed = TAU_SEEDS.get(name, 7000 + (CASES.index(name) if name in CASES else 0))
    tau = np.zeros((Bn, Cn)) if name == "zero" else draw_tau(seed, Bn, Cn, c["opts"].h)
    return dict(c, tau=tau, groups=groups, keys=keys, name=name)


@functools.lru_cache(maxsize=None)
def case_reference(oracle, name):
    """the np.longdouble reference of a case (computed once per process)"""
    return reference(oracle, case_inputs(name))


@functools.lru_cache(maxsize=None)
def wrong_reference(oracle, name, *wrong):
    """the reference of a case evaluated with deliberate errors (evaluate()'s `wrong`)"""
    return reference(oracle, case_inputs(name), wrong=tuple(wrong))


def cut(c, b):
    """sequence b of case inputs c alone"""
    return dict(c, **{k: np.ascontiguousarray(c[k][b:b + 1]) for k in ("q", "meas", "weight", "tau")})


# ---- the two measurements the tolerances stand on, and the oracle's distance (CPU) ------------------------------------------------------
def ulp_spread(oracle, c, R, draws=4, seed=0):
    """measurement 1 of a case: the float64 evaluation at the consistent q against itself at that q moved by one ulp in a random direction"""
    B, N = R["shape"]
    qc = R["q_out"].reshape(B, N, -1)
    R0 = reference(oracle, c, np.float64, q=qc, stencil=np.longdouble)
    rng = np.random.default_rng(seed)
    worst = {}
    for _ in range(draws):
        q1 = np.nextafter(qc, np.where(rng.random(qc.shape) < 0.5, -np.inf, np.inf))
        merge(worst, discrepancies(outputs(reference(oracle, c, np.float64, q=q1, stencil=np.longdouble)), R0, c["keys"]))
    return worst


def extended_distance(oracle, c, R):
    """measurement 2 of a case: the float64 evaluation against the np.longdouble one"""
    B, N = R["shape"]
    return discrepancies(outputs(reference(oracle, c, np.float64, q=R["q_out"].reshape(B, N, -1), stencil=np.longdouble)), R, c["keys"])


def oracle_distance(oracle, c, R):
    """oracle.objective_shutter against the reference R of a case with the columns of u, per sequence: dict(gt, g, f) in the units of ORACLE"""
    B, N = R["shape"]
    out = dict(gt=0.0, g=0.0, f=0.0)
    fl = lambda a: np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))
    Ep = FC.evaluate(c["sk"], c["cams"], c["opts"], None, fl(R["q_out"].reshape(c["q"].shape)), fl(c["meas"]), fl(c["weight"]))
    for b in range(B):
        a = (c["sk"], c["cams"], c["opts"], c["pr"], c["q"][b], c["meas"][b], c["weight"][b])
        f, g, gt, _ = oracle.objective_shutter(*a, c["tau"][b], want_grad=True)
        f0 = oracle.objective(*a)[0]
        sl = slice(b * N, (b + 1) * N)
        # d f / d tau_c = G_c = -step_c H_c, in step's scale times H_c
        Gc, Sc = -R["step"][b] * R["H"][b], R["step_scale"][b] * R["H"][b]
        out["gt"] = max(out["gt"], FC._ratio(gt[1:], Gc[1:], Sc[1:]))
        out["g"] = max(out["g"], FC._ratio(g.reshape(N, NU), R["g_total"][sl], R["g_total_scale"][sl]))
        df = (R["cost"][sl, 0] - Ep["cost"][sl, 0]).sum()
        out["f"] = max(out["f"], float(abs(f - (f0 + df)) / abs(f)))
    return out


def measure(oracle, names=CASES, log=print):
    """(measurement 1, measurement 2, the oracle's distance) per key over the cases `names`"""
    m1, m2, mo = {}, {}, {}
    for i, name in enumerate(names):
        c, R = case_inputs(name), case_reference(oracle, name)
        assert conditions_hold(R), (name, R["conditions"])
        a, b = ulp_spread(oracle, c, R, seed=i), extended_distance(oracle, c, R)
        o = oracle_distance(oracle, c, R) if "g_total" in R else {}
        log(f"{name:22s} (1) " + ", ".join(f"{k} {v:.2e}" for k, v in a.items()) + " | (2) " + ", ".join(f"{k} {v:.2e}" for k, v in b.items())
            + " | oracle " + ", ".join(f"{k} {v:.2e}" for k, v in o.items()))
        merge(m1, a); merge(m2, b)
        for k, v in o.items():
            mo[k] = max(mo.get(k, 0.0), v)
    return m1, m2, mo


if __name__ == "__main__":
    from oracle import oracle as O
    O.lib()
    m1, m2, mo = measure(O)
    for k in MEASURED_KEYS:
        print(f"  {k:9s}  {m1[k]:.2e}        {m2[k]:.2e}        {MARGIN * max(m1[k], m2[k]):.2e}")
    print("  oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in mo.items()))
