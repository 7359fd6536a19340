"""Independent reference of the detection report (include/cpe.h, cpe_detection_report; DESIGN.md 2 "What is predicted in the image"), for
tests/test_detection_report_host.py (CPU) and tests/test_gpu_detection_report.py (GPU).

The statement is evaluated in numpy at one dtype, `np.longdouble` (the reference) or `np.float64` (its own rounding error: the tolerances).  It
shares nothing with the HIP code.  The loss and its first and second derivative come from carrying (value, first, second derivative) triples
through the loss's definition -- a sum of sigmoid switches times polynomial pieces --, not from expanded formulas; the camera's 2 x 3 derivative
is written from g(r) = distortion factor, d(a g)/da = g + a^2 g'/r, and is held against a central difference of ingest_compare.project in
tests/test_detection_report_host.py.  The package is used for inputs only (camera structs, synthetic points).

Tolerances (tolerance()): per case and output key 16 x the distance between the float64 and the longdouble evaluation of this reference on that
very case, with a floor of 64 eps, both in units of the entry's scale: |uv| + fx for pixels, max(S_xx, S_yy) for covariances, max(1, |x|) for
d2 and leverage.  One order over the reference's own float64 error is what the rounding of this length of 2 x 2 algebra in another order of
operations (fused multiply-adds on the GPU) justifies.  Recorded values below never feed a tolerance.

Conditions on every accuracy case (check_conditions): the smaller eigenvalue of T is >= 0.05 or <= -1e-3, so that the undefined rule (> 1e-9) is
never decided by rounding, and no coordinate's scaled residual w_f r sits within 1e-3 of a knot of the loss.

Recorded (printed by the tests; `python -m pytest -s`):
  worst distance float64 reference - longdouble reference over the GPU cases, in units of the scale:
      uv 3.7e-16, cov_px 1.0e-14, uv_loo 3.1e-15, cov_loo 3.1e-13, d2 1.9e-12, leverage 1.8e-13   (CPU, test_detection_report_host.py)
  worst distance GPU (MI355X) - longdouble reference over the same cases (test_gpu_detection_report.py::test_zz_report):
      uv 6.1e-16, cov_px 4.9e-15, uv_loo 3.1e-15, cov_loo 3.1e-13, d2 8.9e-13, leverage 1.9e-13; at most 0.096 of a case's tolerance
      (profiles/r13_detection_report_notes.md has the table)
  brute force on the linear-Gaussian problem (28 unknowns, 48 detections): S_loo against the dense inverse 8.0e-16, uv_loo against the refit
      9.9e-15, the symmetric form against S (I - W S)^-1 5.6e-16; mean of d2 over 2000 detections from the model 1.955 (raw-residual form 1.928)
  leave-one-out against an actual re-solve without the detection, relative to |uv_loo - uv| (REFIT_CPU; the oracle's solve on the CPU and
      solve_host on the GPU give the same figures): 0.022, 0.119, 0.006 on the three inliers of largest leverage, 0.195 on a planted outlier
  the project's own fit at FIT_SEED = 21 (the first seed tried): 10 of 10 planted detections flagged, 0 of the 1002 others, on both routes
"""
import functools

import numpy as np

import ingest_compare as IC
from cheetah_pose_estimation_amd import abi

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
KEYS = ("uv", "cov_px", "uv_loo", "cov_loo", "d2", "leverage")
MARGIN, FLOOR = 16.0, 64.0 * EPS
T_MIN = 1e-9                  # the statement's rule: defined where the smaller eigenvalue of T is finite and above this
KNOTS = (3.0, 10.0, 20.0)
# what the leave-one-out prediction missed the oracle's actual re-solve by, relative to |uv_loo - uv|, measured on the CPU by
# test_detection_report_host.py::test_loo_against_the_oracles_refit: 0.195, rounded up (the GPU test allows 4 x this)
REFIT_CPU = 0.2


# ---------------------------------------------------------------------------------------------------- the loss, by carried derivatives
class Jet:
    """(value, first, second derivative) of a function of one variable, entry by entry"""

    def __init__(self, v, d=0, dd=0):
        self.v, self.d, self.dd = v, d + 0 * v, dd + 0 * v

    @staticmethod
    def lift(x):
        return x if isinstance(x, Jet) else Jet(x)

    def __add__(self, o):
        o = Jet.lift(o)
        return Jet(self.v + o.v, self.d + o.d, self.dd + o.dd)

    __radd__ = __add__

    def __neg__(self):
        return Jet(-self.v, -self.d, -self.dd)

    def __sub__(self, o):
        return self + (-Jet.lift(o))

    def __rsub__(self, o):
        return Jet.lift(o) + (-self)

    def __mul__(self, o):
        o = Jet.lift(o)
        return Jet(self.v * o.v, self.d * o.v + self.v * o.d, self.dd * o.v + 2 * self.d * o.d + self.v * o.dd)

    __rmul__ = __mul__

    def sigmoid(self):
        """1 / (1 + exp(-x)): s' = s (1 - s), s'' = s (1 - s) (1 - 2 s)"""
        with np.errstate(over="ignore"):
            s = 1 / (1 + np.exp(-self.v))
        s1, s2 = s * (1 - s), s * (1 - s) * (1 - 2 * s)
        return Jet(s, s1 * self.d, s2 * self.d * self.d + s1 * self.dd)


def loss(s, knots, mode, dtype=LD):
    """the redescending loss at the scaled residual s: (rho'(s), kappa(s)) with kappa the PSD curvature weight of the solver -- mode 0:
    max(rho'', rho'(|s|) / |s|, 0), mode 1: max(rho'', 0).  rho(e), e = |s|, is quadratic below a, linear to b, a falling parabola to c and
    constant beyond, the pieces blended by sigmoid switches at the knots."""
    a, b, c = (dtype(k) for k in knots)
    s = np.asarray(s, dtype=dtype)
    e = Jet(np.abs(s), dtype(1), dtype(0))
    on = lambda k: (e - k).sigmoid()
    half = dtype(1) / 2
    quad = half * (e * e)
    line = a * e - a * a * half
    u = (c - e) * (1 / (c - b))
    para = (a * b - a * a * half) + (a * (c - b) * half) * (1 - u * u)
    flat = a * b - a * a * half + a * (c - b) * half
    rho = (1 - on(a)) * quad + (on(a) - on(b)) * line + (on(b) - on(c)) * para + on(c) * flat
    d1 = np.sign(s) * rho.d
    kap = np.maximum(rho.dd, 0)
    if mode == 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            sec = np.where((e.v > 1e-12) & (rho.d > 0), rho.d / np.where(e.v > 0, e.v, 1), 0)
        kap = np.maximum(kap, sec)
    return d1, kap


# ---------------------------------------------------------------------------------------------------- the camera and its derivative
def project_with_jacobian(cam, p, dtype=LD):
    """uv [..., 2] and G = d uv / d p [..., 2, 3] of one camera at points p [..., 3].  With X = R p + t, (a, b) = (X0, X1) / X2, r = |(a, b)| and the
    distortion factor g(r), uv = f (a, b) g + c, so d(a g)/d(a, b) = (g + a^2 k, a b k) with k = g'(r) / r (0 at r = 0) and d(a, b)/dp = (R_0 - a
    R_2, R_1 - b R_2) / X2.  Fisheye: g = theta P(theta) / (r + 1e-12), theta = atan r; pinhole: g = 1 + D0 r^2 + D1 r^4 + D2 r^6."""
    R = np.array(cam.R[:], dtype=dtype).reshape(3, 3)
    t, D = np.array(cam.t[:], dtype=dtype), np.array(cam.D[:], dtype=dtype)
    f, c = np.array([cam.fx, cam.fy], dtype=dtype), np.array([cam.cx, cam.cy], dtype=dtype)
    p = np.asarray(p, dtype=dtype)
    X = p @ R.T + t
    with np.errstate(all="ignore"):
        ab = X[..., :2] / X[..., 2:3]
        r2 = (ab * ab).sum(-1)
        r = np.sqrt(r2)
        if cam.model == abi.CAM_FISHEYE:
            th = np.arctan(r)
            P = 1 + D[0] * th**2 + D[1] * th**4 + D[2] * th**6 + D[3] * th**8
            dthP = 1 + 3 * D[0] * th**2 + 5 * D[1] * th**4 + 7 * D[2] * th**6 + 9 * D[3] * th**8        # d(theta P)/d theta
            den = r + dtype(1e-12)
            g = th * P / den
            dg = dthP / (1 + r2) / den - th * P / (den * den)
        else:
            g = 1 + D[0] * r2 + D[1] * r2**2 + D[2] * r2**3
            dg = r * (2 * D[0] + 4 * D[1] * r2 + 6 * D[2] * r2**2)
        k = np.where(r > 0, dg / np.where(r > 0, r, 1), 0)
        uv = f * ab * g[..., None] + c
        dab = (R[:2][None] - ab[..., :, None] * R[2]) / X[..., 2:3, None]                                 # [..., 2, 3]
        Kd = g[..., None, None] * np.eye(2, dtype=dtype) + k[..., None, None] * ab[..., :, None] * ab[..., None, :]
        G = f[:, None] * (Kd @ dab)
    return uv, G


def sym3(S):
    """[..., 2, 2] -> (xx, xy, yy)"""
    return np.stack([S[..., 0, 0], S[..., 0, 1], S[..., 1, 1]], axis=-1)


def full2(s3):
    """(xx, xy, yy) -> [..., 2, 2]"""
    return np.asarray(s3)[..., [0, 1, 1, 2]].reshape(np.shape(s3)[:-1] + (2, 2))


# ---------------------------------------------------------------------------------------------------- the 2 x 2 algebra of the statement
def woodbury(uv, S, g, W, dtype=LD, sign=1):
    """one detection's term (gradient g [..., 2], curvature diag(W [..., 2])) taken out of a fit whose pixel covariance is S [..., 2, 2]:
    (uv_loo, S_loo, leverage, smaller eigenvalue of T, defined) with T = I - diag(a) S diag(a), a = sqrt(W), S_loo = S + S diag(a) T^-1 diag(a) S
    (symmetric; = S (I - W S)^-1) and uv_loo = uv + S_loo g"""
    uv, S, g, W = (np.asarray(x, dtype=dtype) for x in (uv, S, g, W))
    a = np.sqrt(W)
    I = np.eye(2, dtype=dtype)
    T = I - a[..., :, None] * S * a[..., None, :]
    lev = W[..., 0] * S[..., 0, 0] + W[..., 1] * S[..., 1, 1]
    hd = (T[..., 0, 0] - T[..., 1, 1]) / 2
    tmin = (T[..., 0, 0] + T[..., 1, 1]) / 2 - np.sqrt(hd * hd + T[..., 0, 1] * T[..., 0, 1])
    ok = np.isfinite(tmin) & (tmin > T_MIN)
    with np.errstate(all="ignore"):
        Ti = _inv2(np.where(ok[..., None, None], T, I))
        Sa = S * a[..., None, :]
        Sl = S + Sa @ Ti @ np.swapaxes(Sa, -1, -2)
        Sl = (Sl + np.swapaxes(Sl, -1, -2)) / 2
        ul = uv + sign * (Sl @ g[..., None])[..., 0]
    return ul, Sl, lev, tmin, ok


def leave_one_out(uv, S, z, w, wf, knots, mode, dtype=LD, variant=None):
    """the statement from (uv [..., 2], S [..., 2, 2]) on: dict(uv_loo, cov_loo [..., 2, 2], d2, leverage, tmin, s) for detections z with the
    solver's weights w and the fit's weights wf (camera multiplier included).  variant (the power checks of the host tests): "sign" flips
    S_loo g, "kappa0" drops kappa0 from sigma2, "w_for_wf" uses w where the statement says w_f."""
    uv, S, z = (np.asarray(x, dtype=dtype) for x in (uv, S, z))
    w, wf = np.asarray(w, dtype=dtype), np.asarray(wf, dtype=dtype)
    if variant == "w_for_wf":
        wf = w
    s = wf[..., None] * (uv - z)
    d1, kap = loss(s, knots, mode, dtype)
    g = d1 * wf[..., None]
    W = kap * (wf * wf)[..., None]
    I = np.eye(2, dtype=dtype)
    ul, Sl, lev, tmin, ok = woodbury(uv, S, g, W, dtype, -1 if variant == "sign" else 1)
    with np.errstate(all="ignore"):
        kappa0 = loss(np.zeros(1, dtype=dtype), knots, mode, dtype)[1][0]
        sigma2 = 1 / (w * w * (1 if variant == "kappa0" else kappa0))
        r = z - ul
        Cm = Sl + sigma2[..., None, None] * I
        d2 = (r[..., None, :] @ _inv2(Cm) @ r[..., :, None])[..., 0, 0]
    nan = dtype(np.nan)
    seen = w != 0
    und = seen & ~ok
    ul = np.where(und[..., None], nan, np.where(seen[..., None], ul, uv))
    Sl = np.where(und[..., None, None], nan, np.where(seen[..., None, None], Sl, S))
    d2 = np.where(seen & ok, d2, nan)
    lev = np.where(seen, lev, 0)
    return dict(uv_loo=ul, cov_loo=Sl, d2=d2, leverage=lev, tmin=np.where(seen, tmin, 1), s=np.where(seen[..., None], s, 0))


def _inv2(M):
    """inverse of [..., 2, 2] by the adjugate, at M's dtype (numpy's inv has no longdouble)"""
    det = M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 1, 0]
    adj = np.stack([np.stack([M[..., 1, 1], -M[..., 0, 1]], -1), np.stack([-M[..., 1, 0], M[..., 0, 0]], -1)], -2)
    return adj / det[..., None, None]


def reference(cams, knots, mode, positions, cov_pos, meas=None, weight=None, weight_fit=None, dtype=LD, variant=None):
    """the whole statement: positions [B, N, L, 3], cov_pos [B, N, L, 3, 3], meas [B, N, C, L, 2], weight / weight_fit [B, N, C, L] -> dict of
    KEYS in the C ABI's layouts (cov_px, cov_loo as (xx, xy, yy)) plus tmin and s [B, N, C, L(, 2)] for check_conditions"""
    pos, Sp = np.asarray(positions, dtype=dtype), np.asarray(cov_pos, dtype=dtype)
    uv, S = [], []
    for c in range(len(cams)):
        u, G = project_with_jacobian(cams[c], pos, dtype)
        uv.append(u)
        S.append(G @ Sp @ np.swapaxes(G, -1, -2))
    uv, S = np.stack(uv, axis=2), np.stack(S, axis=2)
    out = dict(uv=uv, cov_px=sym3(S))
    if meas is None:
        return out
    mult = np.array([cams[c].mult for c in range(len(cams))], dtype=dtype)[None, None, :, None]
    w = mult * np.asarray(weight, dtype=dtype)
    wf = w if weight_fit is None else mult * np.asarray(weight_fit, dtype=dtype)
    loo = leave_one_out(uv, S, meas, w, wf, knots, mode, dtype, variant)
    loo["cov_loo"] = sym3(loo["cov_loo"])
    out.update(loo)
    return out


# ---------------------------------------------------------------------------------------------------- distances and tolerances
def scales(ref, cams):
    """the scale of every entry of every key: |uv| + fx for pixels, max(S_xx, S_yy) for covariances, max(1, |x|) for d2 and leverage"""
    fx = np.array([cams[c].fx for c in range(len(cams))])[None, None, :, None, None]
    uv = np.asarray(ref["uv"], dtype=np.float64)
    S = np.asarray(ref["cov_px"], dtype=np.float64)
    sc = dict(uv=np.abs(uv) + fx, cov_px=np.maximum(S[..., 0], S[..., 2])[..., None] * np.ones(3))
    if "uv_loo" in ref:
        Sl = np.asarray(ref["cov_loo"], dtype=np.float64)
        sc.update(uv_loo=np.abs(np.nan_to_num(np.asarray(ref["uv_loo"], dtype=np.float64))) + fx,
                  cov_loo=np.nan_to_num(np.maximum(Sl[..., 0], Sl[..., 2]), nan=1.0)[..., None] * np.ones(3),
                  d2=np.maximum(1.0, np.abs(np.nan_to_num(np.asarray(ref["d2"], dtype=np.float64)))),
                  leverage=np.maximum(1.0, np.abs(np.asarray(ref["leverage"], dtype=np.float64))))
    return sc


def distances(got, ref, cams):
    """{key: largest |got - ref| / scale}; the NaN patterns must agree exactly (asserted)"""
    sc = scales(ref, cams)
    out = {}
    for k in KEYS:
        if k not in ref or k not in got:
            continue
        a, b = np.asarray(got[k], dtype=LD), np.asarray(ref[k], dtype=LD)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{k}: NaN pattern differs"
        diff = np.abs(a - b)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(diff == 0, 0, diff / sc[k])                  # (S = 0 on a fisheye camera's optical axis: equal, at any scale)
        out[k] = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
    return out


def tolerance(case):
    """{key: max(16 x |float64 reference - longdouble reference|, 64 eps)} of the case, in units of the scale"""
    ref, r64 = case_reference(case), case_reference(case, np.float64)
    return {k: max(MARGIN * v, FLOOR) for k, v in distances(r64, ref, case_inputs(case)["cams"]).items()}


def check_conditions(ref, knots):
    tmin, s = np.asarray(ref["tmin"], dtype=np.float64), np.abs(np.asarray(ref["s"], dtype=np.float64))
    assert np.all((tmin >= 0.05) | (tmin <= -1e-3)), "a case's T has its smaller eigenvalue where rounding decides the undefined rule"
    for k in knots:
        assert np.all(np.abs(s - k) >= 1e-3), "a scaled residual sits on a knot of the loss"


# ---------------------------------------------------------------------------------------------------- the cases of both test files
CONFIGS = ((1, 24), (3, 25), (18, 25))                       # (C, L): C L = 24 (less than a wave), 75 (a second, partial trip), 450 (CPE_MAX_CAMS)
CASES = tuple((shape, cl, mode) for cl in CONFIGS for shape in IC.SHAPES for mode in (0, 1))
REGIMES = ((0.1, 2.8), (3.2, 9.5), (10.5, 19.5), (21.0, 40.0))            # |w_f r| below 3, 3..10, 10..20, beyond 20


def edge_points():
    """the points in front of ingest_compare's axis cameras: on the optical axis, at r = 1e-12 .. 1e-3 in both image directions, out to theta = 1.4"""
    edge = []
    for r in IC.AXIS_RADII:
        edge += [(3 * r, -1.0, 0.0), (0.0, -1.0, -3 * r)]
    for th in IC.WIDE_THETA:
        edge += [(3 * np.tan(th), -1.0, 0.0), (-3 * np.tan(th) * 0.6, -1.0, 3 * np.tan(th) * 0.8)]
    return np.array(edge)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """the inputs of one accuracy case: cameras (fisheye and pinhole alternating, the first two the axis cameras), points around the rig's centre
    with the edge points in the first and the last frame, random SPD cov_pos with standard deviations 1 mm .. 0.3 m, and detections placed from
    the float64 reference's own uv and S: the weight from a target t = w^2 tr S (0.05 .. 0.8, so that T >= 0.2; 3 .. 6 with a small residual on
    every 13th pair: undefined), each coordinate's scaled residual in one of the loss's four regimes, every 11th pair without a detection, another
    11th held out (weight_fit 0) and another fitted at half its weight"""
    (B, N), (C, L), mode = case
    rng = np.random.default_rng(1000 * C + 100 * B + N + 7 * mode)
    cams = IC.reproject_cameras(C, L)
    pos = np.array([0.3, -0.5, 0.4]) + rng.uniform(-1.0, 1.0, (B, N, L, 3))
    edge = edge_points()
    pos[0, 0, :len(edge)] = edge
    pos[-1, -1, :len(edge)] = edge
    Q = np.linalg.qr(rng.normal(size=(B, N, L, 3, 3)))[0]
    sd = 10.0 ** rng.uniform(-3.0, np.log10(0.3), (B, N, L, 3))
    cov = Q @ (sd[..., None] ** 2 * np.swapaxes(Q, -1, -2))
    cov = 0.5 * (cov + np.swapaxes(cov, -1, -2))
    base = reference(cams, KNOTS, mode, pos, cov, dtype=np.float64)
    uv, S = np.asarray(base["uv"]), np.asarray(base["cov_px"])
    t = np.arange(C * L).reshape(C, L)[None, None] + np.arange(B * N).reshape(B, N, 1, 1)        # a running pair number that shifts with the frame
    tau = rng.uniform(0.05, 0.8, (B, N, C, L))
    undefined = t % 13 == 7
    tau = np.where(undefined, rng.uniform(3.0, 6.0, tau.shape), tau)
    mult = np.array([cams[c].mult for c in range(C)])[None, None, :, None]
    trS = S[..., 0] + S[..., 2]
    w = np.sqrt(tau / np.where(trS > 0, trS, 1.0))
    w = np.where(trS > 0, w, 0.01)                                                   # (S = 0 on the optical axis of a fisheye camera: G = 0 there)
    half, held, none = t % 11 == 7, (t % 11 == 5) & ~undefined, (t % 11 == 3) & ~undefined
    wf = np.where(half & ~undefined, 0.5 * w, w)
    reg = np.stack([t % 4, (t // 4) % 4], axis=-1)
    lo, hi = np.array(REGIMES)[reg, 0], np.array(REGIMES)[reg, 1]
    s = rng.uniform(lo, hi) * rng.choice([-1.0, 1.0], reg.shape)
    s = np.where(undefined[..., None], rng.uniform(-0.9, 0.9, s.shape), s)
    meas = uv - s / wf[..., None]
    weight, weight_fit = w / mult, np.where(held, 0.0, wf / mult)
    weight = np.where(none, 0.0, weight)
    weight_fit = np.where(none, 0.0, weight_fit)
    return dict(cams=cams, mode=mode, positions=pos, cov_pos=cov, meas=np.ascontiguousarray(meas), weight=np.ascontiguousarray(weight),
                weight_fit=np.ascontiguousarray(weight_fit), kinds=dict(undefined=undefined & ~none, held=held & ~none, none=none, half=half))


@functools.lru_cache(maxsize=None)
def case_reference(case, dtype=LD, variant=None):
    """the reference of a case (computed once, shared, read-only); the longdouble one asserts the case conditions"""
    c = case_inputs(case)
    ref = reference(c["cams"], KNOTS, c["mode"], c["positions"], c["cov_pos"], c["meas"], c["weight"], c["weight_fit"], dtype, variant)
    if dtype is LD and variant is None:
        check_conditions(ref, KNOTS)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def options(mode):
    o = abi.default_options()
    o.loss_a, o.loss_b, o.loss_c = KNOTS
    o.curvature = mode
    return o


# ---------------------------------------------------------------------------------------------------- the project's own fit
FIT_SEED = 21                # the first seed tried: the CPU route (test_detection_report_host.py) flags the 10 planted detections and none of the others
FIT_N, FIT_SHIFT, FIT_PLANTED, P_OUTLIER = 40, 30.0, 10, 1e-3
CHI2 = -2.0 * np.log(P_OUTLIER)


@functools.lru_cache(maxsize=None)
def fit_data():
    """phantom with 25 markers, six cameras, N = 40, noise 1 px, no synthetic outliers; 10 detections shifted by 30 px in a random image direction.
    The 10 are drawn (fixed seed) among the seen detections of markers whose sigma is at most 5 px: the shift is then at least 6 standard
    deviations of the detection model against a threshold of sqrt(chi2) = 3.7, which leaves room for the prediction's own variance; on the
    widest markers (7 px) 30 px is 4.2 standard deviations and no outlier at p = 1e-3.  Returns dict(sk, cams, opts, q_init, meas, weight,
    planted [10, 3] = (frame, camera, marker), mask [N, C, L])."""
    from cheetah_pose_estimation_amd import skeleton, synth
    sk, cams = skeleton.build_skeleton("phantom", 25), synth.make_cameras(6)
    d = synth.make_batch(sk, cams, B=1, N=FIT_N, seed=FIT_SEED, noise_px=1.0, outlier_frac=0.0)
    meas, weight = d["meas"][0].copy(), d["weight"][0].copy()
    rng = np.random.default_rng(FIT_SEED)
    sigma = skeleton.measurement_sigma(25)
    cand = np.argwhere((weight > 0) & (sigma[None, None, :] <= 5.0))
    planted = cand[rng.choice(len(cand), FIT_PLANTED, replace=False)]
    phi = rng.uniform(0, 2 * np.pi, FIT_PLANTED)
    mask = np.zeros(weight.shape, bool)
    for (n, c, l), a in zip(planted, phi):
        meas[n, c, l] += FIT_SHIFT * np.array([np.cos(a), np.sin(a)])
        mask[n, c, l] = True
    return dict(sk=sk, cams=cams, opts=options(0), q_init=d["q_init"][0], meas=np.ascontiguousarray(meas), weight=weight, planted=planted, mask=mask)


def flagged(d2, weight):
    return (weight > 0) & np.isfinite(d2) & (np.nan_to_num(np.asarray(d2, dtype=np.float64)) > CHI2)


def refit_targets(leverage, mask, weight):
    """the detections whose leave-one-out prediction is held against an actual re-solve: the three inliers of largest leverage and the first
    planted outlier, as (frame, camera, marker)"""
    lev = np.where(mask | (weight <= 0), -1.0, np.asarray(leverage, dtype=np.float64))
    top = np.argsort(lev, axis=None)[::-1][:3]
    return [tuple(int(i) for i in np.unravel_index(t, lev.shape)) for t in top] + [tuple(int(i) for i in np.argwhere(mask)[0])]


# ---------------------------------------------------------------------------------------------------- the linear-Gaussian problem
def linear_problem(n_det, seed, n_x=28, zero_rows=True, noise=True):
    """a random linear-Gaussian problem: x ~ N(0, P0^-1), detection i observes z_i = J_i x + e_i (J_i [2, n_x]) with precision diag(W_i) (some W_i
    with a zero in one or both rows).  Returns J [n, 2, n_x], W [n, 2], z [n, 2], P0, the estimate xh, H and Sigma = H^-1."""
    rng = np.random.default_rng(seed)
    J = rng.normal(size=(n_det, 2, n_x))
    W = rng.uniform(0.2, 3.0, (n_det, 2))
    if zero_rows:
        W[3, 0] = 0.0; W[7, 1] = 0.0; W[11] = 0.0; W[19, 0] = 0.0
    A = rng.normal(size=(n_x, n_x))
    P0 = A @ A.T / n_x + 0.5 * np.eye(n_x)
    x = np.linalg.solve(np.linalg.cholesky(P0).T, rng.normal(size=n_x))
    with np.errstate(divide="ignore"):
        e = np.where(W > 0, rng.normal(size=(n_det, 2)) / np.sqrt(np.where(W > 0, W, 1.0)), 0.0) if noise else 0.0
    z = J @ x + e
    H = P0 + np.einsum("nda,nd,ndb->ab", J, W, J)
    xh = np.linalg.solve(H, np.einsum("nda,nd,nd->a", J, W, z))
    return dict(J=J, W=W, z=z, P0=P0, xh=xh, H=H, Sigma=np.linalg.inv(H), x=x)


def linear_loo(p, i):
    """detection i left out, by brute force: the dense inverse of H - J_i^T W_i J_i and the actual refit; returns (J_i x_loo, J_i Sigma_loo J_i^T)"""
    J, W, z = p["J"], p["W"], p["z"]
    Hi = p["H"] - J[i].T @ (W[i][:, None] * J[i])
    keep = np.arange(len(J)) != i
    xl = np.linalg.solve(Hi, np.einsum("nda,nd,nd->a", J[keep], W[keep], z[keep]))
    return J[i] @ xl, J[i] @ np.linalg.inv(Hi) @ J[i].T
