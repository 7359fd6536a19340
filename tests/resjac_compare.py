"""Row-by-row comparison of cpe_eval_resjac's outputs (k_resjac: r [N, C, L, 2], J in slot layout [N, C, S, 2], eps [N, nq], cost [N] or None)
with oracle.eval_resjac on the same bits of input.  Helper of the tests, not a test module.

Every key is one number per sequence, the worst over its entries of |HIP - oracle| / scale; inf for any non-finite HIP value:

  J_row   every real slot of a (frame, camera, marker) row; the oracle's dense J gathered into slots with skeleton.jacobian_layout
          scale: max |J_oracle| over that row (2 x nq entries), times max(1, NEAR_Z / |z_cam|)
  J_pad   the alignment slots (0-3 pairs after the last real slot): exactly 0.0, or inf
  r       residual                     scale max(|r_oracle + meas|, 1) per entry (the projected pixel)
  eps     acceleration slack           scale (|q_n| + 3 |q_n-1| + 3 |q_n-2| + |q_n-3|) / h^2 per entry; frames 0..2: exactly 0.0, or inf
  cost    per-frame robust cost        scale |cost_oracle|; exactly zero where that is zero

Rows near a camera's plane.  The projection of a marker close to z_cam = 0 is ill conditioned and the synthetic runs do pass there.  The oracle's
own one-ulp spread of a row grows as 1 / |z_cam| and no faster (tests/test_resjac_compare.py asserts that law on the benchmark-shape inputs), so
no row is left out: a row's tolerance is TOL["J_row"] max(1, NEAR_Z / |z_cam|), z_cam = the camera-frame depth synth.project_numpy(...)[1] at
synth.fk_numpy(q).  So that the loosening cannot hide a failure, the comparator returns the share of rows with |z_cam| < NEAR_Z ("near") and
every case asserts it is at most NEAR_SHARE_MAX = 0.5 %.

Tolerances.  TOL[key] = MARGIN (32) x the larger of two numbers measured ON THE CPU, over the inputs of the cases of tests/test_gpu_resjac.py
(case_inputs below); nothing of the kernel's output enters them:

  1  the oracle's spread under a one-ulp change of every q (np.nextafter, random direction, 4 draws): ulp_spread(), over every sequence of the
     cases "bench" (77 x 200, fisheye) and "kinetic" (42 x 200, pinhole)
  2  the oracle's distance from an extended-precision reference: synth.fk_numpy + synth.project_numpy in np.longdouble, J from five-point
     central differences with h = 1e-3 and h / 2, extrapolated ((16 D(h / 2) - D(h)) / 15), the loss and the slack in np.longdouble:
     extended_reference(), over 2 sequences x 60 frames of each of the two rigs.  (At h = 1e-6 the quotient's own rounding, 1e-11, hides the
     oracle's.  The plain five-point quotient at h = 1e-3 is good enough for the fisheye rig, 2.8e-14, but not for the pinhole rig, whose
     sixth-order radial polynomial leaves it a truncation error of 2.3e-12 that falls 16-fold at h / 2: the stencil's, not the oracle's.
     Extrapolated, the distance is 4e-15 there.)

            measurement 1   measurement 2   TOL = 32 x the larger
  J_row     6.19e-14        1.17e-14        1.98e-12
  r         1.71e-12        3.24e-13        5.47e-11
  eps       6.63e-16        3.29e-16        2.12e-14
  cost      7.19e-12        1.28e-14        2.30e-10

  r: the oracle's spread is 2.5e-12 px whatever the pixel (the principal point, ~1350 px, enters last), so the worst entry in units of its own
  pixel is one that projects to |u| <= 1 px.  cost: 8.1e-14 on the fisheye rig; the 7.2e-12 is a frame of the narrow pinhole rig with few
  markers in view, whose small cost is the square of a difference of two large pixels.

  (produced by `python -m tests.resjac_compare` from the repository root, which prints the table; tests/test_resjac_compare.py recomputes both and asserts that TOL / (1)
  lies in [16, 128] and (2) < TOL / 8)

The margin of 32 stands for what legitimately differs between the two sides on identical inputs: the device sincos (1-2 ulp), FMA contraction
and the two-lane split of the marker chain sum, each of which acts like a few one-ulp perturbations of an intermediate.

The kernel's own worst values on an MI355X over every case of tests/test_gpu_resjac.py (its test_zz_report), for the record; they never fed TOL:
  J_row 6.4e-14 (77 x 200), J_pad 0, r 1.4e-12 (8191 x 1), eps 5.3e-16 (kinetic rig), cost 6.1e-12 (two cameras): each at the level of
  measurement 1, a factor 9 to 40 inside its tolerance
"""
import functools

import numpy as np

from cheetah_pose_estimation_amd import abi, skeleton, synth

KEYS = ("J_row", "J_pad", "r", "eps", "cost")
NEAR_Z = 0.25                 # metres of camera-frame depth below which a row's tolerance grows as 1 / |z_cam|
NEAR_SHARE_MAX = 0.005        # every case: at most this share of its rows may be that near
MARGIN = 32.0

# (measurement 1, measurement 2) per key, in the units above: CPU only, see the module docstring
MEASURED = dict(J_row=(6.19e-14, 1.17e-14), r=(1.71e-12, 3.24e-13), eps=(6.63e-16, 3.29e-16), cost=(7.19e-12, 1.28e-14))
TOL = {k: MARGIN * max(v) for k, v in MEASURED.items()}
TOL["J_pad"] = 0.0


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
_LAYOUTS = {}


def layout(sk):
    """(slot_marker [S], slot_dof [S], number of real slots, first slot of every marker [L]); the slots from the real count on are alignment"""
    key = (sk.n_markers, sk.n_links, tuple(sk.marker_link[l] for l in range(sk.n_markers)), tuple(sk.parent[k] for k in range(sk.n_links)))
    if key not in _LAYOUTS:
        sm, sd = skeleton.jacobian_layout(sk)
        n_real = 0
        for l in range(sk.n_markers):
            k, n = sk.marker_link[l], 3
            while k >= 0:
                n += 3
                k = sk.parent[k]
            n_real += n
        assert n_real <= len(sm) < n_real + 4 and np.all(np.diff(sm[:n_real]) >= 0)
        first = np.searchsorted(sm[:n_real], np.arange(sk.n_markers))       # first slot of every marker (slots are marker-major)
        _LAYOUTS[key] = (sm, sd, n_real, first)
    return _LAYOUTS[key]


def to_slots(sk, Jdense):
    """dense J [N, C, L, 2, nq] -> slot layout [N, C, S, 2], alignment slots 0.0"""
    sm, sd, n_real, _ = layout(sk)
    J = np.ascontiguousarray(np.moveaxis(Jdense[:, :, sm, :, sd], 0, 2))
    J[:, :, n_real:] = 0.0
    return J


def depth(sk, cams, q):
    """camera-frame depth z_cam [N, C, L] of every marker"""
    pos = synth.fk_numpy(sk, q)[0]
    return np.stack([synth.project_numpy(cams[c], pos)[1] for c in range(len(cams))], axis=-2)


# ---- the reference of one sequence ----------------------------------------------------------------------------------------------------
def make_reference(sk, cams, h, q, meas, r, Jdense, eps, cost):
    """the reference of one sequence from (r, dense J, eps, cost) of it, in the comparator's form"""
    for a in (r, Jdense, eps, cost):
        if not np.all(np.isfinite(a)):
            raise ValueError("the reference itself is not finite: no case may be built on such inputs")
    ql = np.abs(q)
    es = np.zeros_like(ql)
    if q.shape[0] > 3:
        es[3:] = (ql[3:] + 3 * ql[2:-1] + 3 * ql[1:-2] + ql[:-3]) / (h * h)
    return dict(r=r, J=to_slots(sk, Jdense), rowmax=np.abs(Jdense).max(axis=(-1, -2)), eps=eps, eps_scale=es, cost=cost,
                z=depth(sk, cams, np.asarray(q, dtype=np.float64)), uv=np.abs(r + meas), sk=sk)


def reference(oracle, sk, cams, opts, q, meas, weight, frames_are_sequences=False):
    """oracle.eval_resjac of one sequence q [N, nq], meas [N, C, L, 2], weight [N, C, L].  frames_are_sequences: the N frames are N sequences of
    one frame each (r, J and cost are per-frame quantities; eps is zero by the rule of the first three frames)"""
    ro, Jo, eo, co = oracle.eval_resjac(sk, cams, opts, q, meas, weight)
    R = make_reference(sk, cams, opts.h, q, meas, ro, Jo, eo, co)
    if frames_are_sequences:
        R["eps"] = np.zeros_like(eo)
        R["eps_scale"] = np.zeros_like(eo)
    return R


def oracle_outputs(R):
    """the reference's own numbers in cpe_eval_resjac's layout (what a faultless kernel would return)"""
    return dict(r=R["r"].copy(), J=R["J"].copy(), eps=R["eps"].copy(), cost=R["cost"].copy())


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def _ratio(G, R, scale):
    """worst |G - R| / scale; inf where G is not finite, or where the scale is zero and G != R"""
    G = np.asarray(G)
    if not np.all(np.isfinite(G)):
        return float("inf")
    d = np.abs(G - R)
    scale = np.broadcast_to(scale, d.shape)
    zero = scale == 0.0
    if np.any(d[zero] != 0.0):
        return float("inf")
    return float((d[~zero] / scale[~zero]).max(initial=0.0))


def row_errors(G_J, R):
    """[N, C, L]: worst |J_HIP - J_oracle| over the real slots of every row, in units of the row's max |J_oracle| (no depth factor)"""
    _, _, n_real, first = layout(R["sk"])
    d = np.abs(np.asarray(G_J)[:, :, :n_real] - R["J"][:, :, :n_real]).max(axis=-1)          # [N, C, n_real]
    return np.maximum.reduceat(d, first, axis=2) / R["rowmax"]


def discrepancies(G, R):
    """worst value of every key for one sequence: G = dict(r, J, eps, cost or None) of HIP, R = reference(...); plus "near" = share of rows with
    |z_cam| < NEAR_Z and "rows" = the number of rows"""
    _, _, n_real, _ = layout(R["sk"])
    out = {}
    GJ = np.asarray(G["J"])
    if not np.all(np.isfinite(GJ)):
        out["J_row"] = float("inf")
    else:
        with np.errstate(divide="ignore"):
            fac = np.maximum(1.0, NEAR_Z / np.abs(R["z"]))
        if np.any(R["rowmax"] == 0.0):
            raise ValueError("a row of the reference is all zero")
        out["J_row"] = float((row_errors(GJ, R) / fac).max(initial=0.0))
    pad = GJ[:, :, n_real:]
    out["J_pad"] = 0.0 if not np.any(pad != 0.0) and not np.any(np.isnan(pad)) else float("inf")
    out["r"] = _ratio(G["r"], R["r"], np.maximum(R["uv"], 1.0))
    out["eps"] = _ratio(G["eps"], R["eps"], R["eps_scale"])
    if G.get("cost") is not None:
        out["cost"] = _ratio(G["cost"], R["cost"], np.abs(R["cost"]))
    out["near"] = float((np.abs(R["z"]) < NEAR_Z).mean())
    out["rows"] = int(R["z"].size)
    return out


def failures(d, tol=None):
    """the keys of a discrepancy dict beyond their tolerance"""
    tol = tol or TOL
    return {k: d[k] for k in KEYS if k in d and not d[k] <= tol[k]}


def merge(worst, d):
    """fold one sequence's discrepancies into the running worst of a case ("near" becomes the share over all rows seen)"""
    for k in KEYS:
        if k in d:
            worst[k] = max(worst.get(k, 0.0), d[k])
    n0, n1 = worst.get("rows", 0), d["rows"]
    worst["near"] = (worst.get("near", 0.0) * n0 + d["near"] * n1) / (n0 + n1)
    worst["rows"] = n0 + n1
    return worst


# ---- the two measurements the tolerances stand on (CPU) --------------------------------------------------------------------------------
def ulp_spread(oracle, sk, cams, opts, q, meas, weight, draws=4, seed=0, rows=False):
    """measurement 1 of one sequence: the worst of every key between the oracle at q and the oracle at q moved by one ulp in a random direction per
    entry, `draws` times.  rows: also the per-row J spread [N, C, L] (units of the row's max |J|, no depth factor) and |z_cam|"""
    R = reference(oracle, sk, cams, opts, q, meas, weight)
    rng = np.random.default_rng(seed)
    worst, spread = {}, np.zeros(R["z"].shape)
    for _ in range(draws):
        q1 = np.nextafter(q, np.where(rng.random(q.shape) < 0.5, -np.inf, np.inf))
        ro, Jo, eo, co = oracle.eval_resjac(sk, cams, opts, q1, meas, weight)
        G = dict(r=ro, J=to_slots(sk, Jo), eps=eo, cost=co)
        merge(worst, discrepancies(G, R))
        if rows:
            spread = np.maximum(spread, row_errors(G["J"], R))
    return (worst, spread, np.abs(R["z"])) if rows else worst


def _loss_ld(err, a, b, c):
    """the redescending loss of oracle/cpe_oracle.c (cpo_loss, value only) in np.longdouble"""
    e = np.abs(err)
    sig = lambda t: 1 / (1 + np.exp(-(e - t)))
    sa, sb, sc = sig(a), sig(b), sig(c)
    lin = a * e - a * a / 2
    cb = c - b
    u = (c - e) / cb
    k = a * b - a * a / 2 + (a * cb / 2) * (1 - u * u)
    K = a * b - a * a / 2 + a * cb / 2
    return (1 - sa) / 2 * e * e + (sa - sb) * lin + (sb - sc) * k + sc * K


def extended_reference(sk, cams, opts, q, meas, weight, fd_h=1e-3):
    """measurement 2's reference of one sequence, everything in np.longdouble: (r, dense J, eps, cost)"""
    ld = np.longdouble
    ql, ml, wl = q.astype(ld), meas.astype(ld), weight.astype(ld)
    C = len(cams)

    def uv(qq):
        pos = synth.fk_numpy(sk, qq)[0]
        return np.stack([synth.project_numpy(cams[c], pos)[0] for c in range(C)], axis=-3)            # [N, C, L, 2]
    u0 = uv(ql)
    assert u0.dtype == ld
    r = u0 - ml
    J = np.zeros(r.shape + (sk.nq,), dtype=ld)

    def five_point(p, hh):
        f = []
        for k in (-2, -1, 1, 2):
            qq = ql.copy()
            qq[:, p] += k * hh
            f.append(uv(qq))
        return (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * hh)
    hh = ld(fd_h)
    for p in range(sk.nq):
        J[..., p] = (16 * five_point(p, hh / 2) - five_point(p, hh)) / 15
    mult = np.array([cams[c].mult for c in range(C)], dtype=ld)
    we = (mult[None, :, None] * wl)[..., None] * r
    cost = _loss_ld(we, ld(opts.loss_a), ld(opts.loss_b), ld(opts.loss_c)).sum(axis=(1, 2, 3))
    eps = np.zeros_like(ql)
    h = ld(opts.h)
    eps[3:] = (ql[3:] - 3 * ql[2:-1] + 3 * ql[1:-2] - ql[:-3]) / (h * h)
    return r, J, eps, cost


def extended_distance(oracle, sk, cams, opts, q, meas, weight):
    """measurement 2 of one sequence: the oracle's worst distance from extended_reference, per key"""
    r, J, eps, cost = extended_reference(sk, cams, opts, q, meas, weight)
    R = make_reference(sk, cams, np.longdouble(opts.h), q.astype(np.longdouble), meas.astype(np.longdouble), r, J, eps, cost)
    ro, Jo, eo, co = oracle.eval_resjac(sk, cams, opts, q, meas, weight)
    return discrepancies(dict(r=ro, J=to_slots(sk, Jo), eps=eo, cost=co), R)


# ---- the inputs of the GPU cases (shared with the CPU test, which checks the share of near rows and re-measures the tolerances on them) ----
STRIDE_FRAMES = 2048          # frames of one grid stride of k_resjac on 256 compute units (4 waves x 2 workgroups x 256)
CASES = {
    # name: (rig, B, N, first seed)
    "bench": ("phantom25", 77, 200, 9100),
    "tail7": ("phantom25", 1201, 7, 9400),
    "tail1": ("phantom25", 8191, 1, 9450),
    "tail3": ("phantom25", 2731, 3, 9500),
    "tail4": ("phantom25", 2049, 4, 9550),
    "cam8": ("cam8", 42, 200, 9300),
    "cam1": ("cam1", 42, 200, 9600),
    "cam2": ("cam2", 42, 200, 9650),
    "phantom24": ("phantom24", 42, 200, 9700),
    "jules": ("jules", 42, 200, 9750),
    "kinetic": ("kinetic", 42, 200, 9200),
    "stress": ("phantom25", 42, 200, 9800),
    "large": ("phantom25", 16, 200, 9900),
}


@functools.lru_cache(maxsize=None)
def rig(name):
    """(skeleton, cameras, options, fps, kinetic_dataset) of a rig of the cases"""
    if name == "kinetic":
        from test_gpu_parity import _kinetic_setup
        sk, cams = _kinetic_setup()
        return sk, cams, abi.default_options(200.0), 200.0, True
    sk = skeleton.build_skeleton("jules" if name == "jules" else "phantom", 25 if name in ("phantom25", "cam8", "cam1", "cam2") else 24)
    # (two cameras: the default seed puts 0.76 % of the rows within NEAR_Z of a camera plane, seed 10 puts 0.3 % there)
    cams = synth.make_cameras(2, seed=10) if name == "cam2" else synth.make_cameras({"cam8": 8, "cam1": 1}.get(name, 6))
    return sk, cams, abi.default_options(), 120.0, False


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """dict(sk, cams, opts, q [B, N, nq], meas [B, N, C, L, 2], weight [B, N, C, L]) of a case: synth.make_batch of 200-frame runs, sequence b from
    seed + b, q = q_true + N(0, 0.05) from default_rng(5); sequences shorter than 200 frames are consecutive pieces of such runs (all distinct)"""
    rg, B, N, seed = CASES[name]
    sk, cams, opts, fps, kin = rig(rg)
    runs = -(-B * N // 200)
    d = synth.make_batch(sk, cams, B=runs, N=200, fps=fps, seed=seed, kinetic_dataset=kin, wide_limbs=(name == "stress"))
    q = d["q_true"] + np.random.default_rng(5).normal(0, 0.05, d["q_true"].shape)
    cut = lambda a: np.ascontiguousarray(a.reshape((runs * 200,) + a.shape[2:])[:B * N].reshape((B, N) + a.shape[2:]))
    q, meas, weight = cut(q), cut(d["meas"]), cut(d["weight"])
    if name == "stress":
        _stress(sk, q, meas, weight)
    return dict(sk=sk, cams=cams, opts=opts, q=q, meas=meas, weight=weight)


ZERO_FRAME = 17               # "stress": the frame of sequences 2, 5, 8, ... with every weight and measurement zero


def _stress(sk, q, meas, weight):
    """inputs that stress the per-frame code, in place: weights x 100 (w r beyond loss_c) on sequences 0, 3, ..., x 0.01 (inside loss_a) on
    1, 4, ...; one frame without any measurement on 2, 5, ...; the limbs of make_batch(wide_limbs=True) (rolled trunk, calves and hocks beyond
    the horizontal), four of them swung further on every fourth sequence as in test_frame_normal_matches_oracle"""
    weight[0::3] *= 100.0
    weight[1::3] *= 0.01
    weight[2::3, ZERO_FRAME] = 0.0
    meas[2::3, ZERO_FRAME] = 0.0
    rng = np.random.default_rng(8)
    q[0::4, :, 3] += 0.25
    for lk in ("HFL", "LBR", "LFR", "UBL"):
        q[0::4, :, skeleton.dof(lk, 1)] += rng.uniform(1.2, 2.2)


# ---- `python -m tests.resjac_compare`: the table of the module docstring -------------------------------------------------------------
def measure(oracle, names=("bench", "kinetic"), ext_sequences=2, ext_frames=60, log=print):
    """(measurement 1, measurement 2) per key over the cases `names`, and the share of near rows of measurement 1's inputs"""
    m1, m2 = {}, {}
    for name in names:
        c = case_inputs(name)
        for b in range(c["q"].shape[0]):
            merge(m1, ulp_spread(oracle, c["sk"], c["cams"], c["opts"], c["q"][b], c["meas"][b], c["weight"][b], seed=b))
        for b in range(ext_sequences):
            merge(m2, extended_distance(oracle, c["sk"], c["cams"], c["opts"], c["q"][b, :ext_frames], c["meas"][b, :ext_frames], c["weight"][b, :ext_frames]))
        log(f"{name}: (1) " + ", ".join(f"{k} {m1[k]:.2e}" for k in KEYS) + " | (2) " + ", ".join(f"{k} {m2[k]:.2e}" for k in KEYS))
    return m1, m2


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))                  # (the kinetic rig comes from tests/test_gpu_parity.py)
    from oracle import oracle as O
    O.lib()
    m1, m2 = measure(O)
    for k in ("J_row", "r", "eps", "cost"):
        print(f"  {k:8s}  {m1[k]:.2e}   {m2[k]:.2e}   TOL {MARGIN * max(m1[k], m2[k]):.2e}")
