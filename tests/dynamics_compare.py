"""Independent references for the inverse-dynamics kernels (k_eom, k_dyn_forces, k_grf behind cpe_eom_rows, cpe_eom_residual and cpe_grf_fit).
Helper of tests/test_dynamics_compare.py (CPU) and tests/test_gpu_dynamics.py (GPU), not a test module.  Everything here is built from the
skeleton tables and the option structs; none of the oracle's derivative or force code is used.

Equations of motion (eom_rows).  L(q, q') = sum_i m_i |P_i'|^2 / 2 + w_i^T I_i w_i / 2 - m_i g P_i,z in torch float64 on the CPU: P' by
torch.autograd.functional.jvp of the centre-of-mass map, w from the link's Euler angles (the body-rate map of tests/test_grf.py::_omega_body),
rows = (d2L/dq'dq') q'' + (d2L/dq'dq) q' - dL/dq from `hessian` and `jacobian` of L.  No Newton-Euler recursion, no subtree sums, no dR/da tables.

Generalised forces (force_tables, gen_forces), entry by entry from autograd Jacobians:
  feet    Q = sum_f (d p_foot / dq)^T  M g (z e_z + sum_k D_k xy_k)
  motors  Q_a = sum_m M g tau_m R_first[:, axis] . d(w_second - w_first)_world / dq'_a,   w_world = R w_body
  joints  Q = (dc/dq)^T lambda, c from the rotation matrices in the row order of skeleton.constraint_rows: parent y . child x and
          parent y . child z for a revolute joint, parent y . child z for a Hooke joint

Force fit (FitProblem): A [6, 5 n_feet] = foot Jacobians of the six root coordinates times D_k, E = rows 0-5 / (M g) with the root's inertia
from cpe_grf_options; minimise |E - A y|^2 / 2 + eps |y|^2 / 2 over {0 <= y <= fmax, sum_k xy_k <= mu z per foot}, feet out of contact fixed
at zero.  project(): the exact projection (the multiplier of the friction row is the root of a piecewise linear function, found on its
breakpoints).  kkt_residual(y) = |y - Proj(y - grad f(y) / L)|_inf L in np.longdouble: zero exactly at the minimiser, whatever route led there.
minimiser(): primal active-set method with a dense np.longdouble solve; what makes it a reference is its certificate (<= CERT = 1e-14, asserted
by every caller), not the route.  fista(n, dtype): the documented iteration (L = eps + sum of the squared norms of the
contact columns, beta = it / (it + 3), zero start), written from that description; one_step(): its first iterate in closed form, Proj(A^T E / L).

Inputs of the GPU tests live here too (eom_cases, force_map_case, grf_pool, ...), so that the CPU test can hold the references against the
oracle on exactly those inputs.

Measured on the CPU (tests/test_dynamics_compare.py recomputes, prints and asserts them):

  reference vs oracle, worst over every input of the GPU tests, in units of the scale (rows, forces: max(M g, largest |reference entry| of the
  frame); E, A: max(1, largest |entry|)); the condition is < 1e-12 (REF_ORACLE):
      rows 3.6e-16   feet 3.1e-16   motors 4.4e-16   joints 1.4e-18   E 5.2e-16   A 5.6e-17
  (joints: lambda is in N m, not in body weights, so a unit of it is 3e-3 of the scale M g)

  float64 vs np.longdouble evaluation of fista() over every case of grf_cases() (FISTA_F64_LD): worst force component 1.28e-13, worst residual
  entry 2.20e-15.  32 x 1.28e-13 = 4.1e-12 is below the project's 1e-8, so TOL_FIT = 1e-8 stands.

  truncation (TRUNCATION): fista(2000, longdouble) against minimiser() on the committed stance frames (cases "phantom-2000", 16 frames, and
  "acinoset-2000", 6 frames; contacts drawn with p = 0.6): worst force component 1.35e-2 body weights, worst residual entry 1.52e-6, worst
  objective gap 7.96e-10.  DESIGN.md (row a13) and include/cpe.h carry these figures.

The kernels' own worst values on an MI355X are recorded in tests/test_gpu_dynamics.py.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cheetah_pose_estimation_amd import abi, skeleton, synth               # noqa: E402

REF_ORACLE = 1e-12          # condition on the references: distance to the oracle in units of the scale
TOL_ROWS = 1e-10            # rows and generalised forces, kernel vs reference, in units of scale = max(M g, largest |reference row| of the frame)
CERT = 1e-14                # certificate a minimiser must reach
DK = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0.0]])      # (z, +x, +y, -x, -y)
LD = np.longdouble


# ---- skeletons and options -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name):
    """(skeleton, cpe_eom_options, cpe_dyn_options, cpe_grf_options) of "phantom", "acinoset" (the heaviest) and "phantom-kinetic" """
    animal = name.split("-")[0]
    sk = skeleton.build_skeleton(animal, 24, kinetic_dataset=name.endswith("-kinetic"))
    return sk, skeleton.eom_options(animal), skeleton.dyn_options(animal), skeleton.grf_options(animal)


MODELS = ("phantom", "acinoset", "phantom-kinetic")


def total_mass(sk):
    return float(sum(sk.mass[:sk.n_links]))


def n_constraints(sk):
    return len(skeleton.constraint_rows(sk))


# ---- kinematics in torch ---------------------------------------------------------------------------------------------------------------
# Every point is q[:3] + sum over the links j on its chain of R_j v_j: the vectors v (attach point of the next link of the chain, or the point's
# own offset on its last link) are a constant table [points, links, 3] built from the skeleton, so the whole map is one batched product and the
# autograd graph stays a few dozen nodes deep whatever the number of links.
def _rot_all(ang):
    """ang [n, 3] = (phi, theta, psi) -> R [n, 3, 3] = Rz(psi) Ry(theta) Rx(phi)"""
    sf, cf, st, ct, sp, cp = (torch.sin(ang[:, 0]), torch.cos(ang[:, 0]), torch.sin(ang[:, 1]), torch.cos(ang[:, 1]),
                              torch.sin(ang[:, 2]), torch.cos(ang[:, 2]))
    return torch.stack([torch.stack([cp * ct, sf * st * cp - sp * cf, sf * sp + st * cf * cp], -1),
                        torch.stack([sp * ct, sf * sp * st + cf * cp, -sf * cp + sp * st * cf], -1),
                        torch.stack([-st, sf * ct, cf * ct], -1)], 1)


@functools.lru_cache(maxsize=None)
def _chain_table(sk_bytes, kind):
    sk = abi.Skeleton.from_buffer_copy(sk_bytes)
    if kind == "com":
        pts = [(i, [float(x) for x in sk.com[i][:]]) for i in range(sk.n_links)]
    else:
        pts = [(int(sk.marker_link[l]), [float(x) for x in sk.marker_off[l][:]]) for l in range(sk.n_markers)]
    V = np.zeros((len(pts), sk.n_links, 3))
    for k, (link, off) in enumerate(pts):
        V[k, link] = off
        j = link
        while sk.parent[j] >= 0:
            V[k, sk.parent[j]] += [float(x) for x in sk.attach[j][:]]
            j = sk.parent[j]
    return torch.tensor(V)


def _rotations(sk, q):
    return _rot_all(q[3:3 + 3 * sk.n_links].reshape(sk.n_links, 3))


def _coms(sk, q):
    return q[:3] + torch.einsum("jab,ijb->ia", _rotations(sk, q), _chain_table(bytes(sk), "com"))


def _marker_points(sk, q):
    return q[:3] + torch.einsum("jab,ijb->ia", _rotations(sk, q), _chain_table(bytes(sk), "marker"))


def _omega_body(a, da):
    """body rates [n, 3] from the Euler angles a and their rates da [n, 3]"""
    sf, cf, st, ct = torch.sin(a[:, 0]), torch.cos(a[:, 0]), torch.sin(a[:, 1]), torch.cos(a[:, 1])
    return torch.stack([da[:, 0] - st * da[:, 2], cf * da[:, 1] + sf * ct * da[:, 2], -sf * da[:, 1] + cf * ct * da[:, 2]], -1)


def lagrangian(sk, inertia, gravity, q, dq, translational=True, rotational=True):
    """L(q, q'); inertia [n_links][3] principal moments about the body axes"""
    nl = sk.n_links
    L = torch.zeros((), dtype=torch.float64)
    if translational:
        m = torch.tensor([float(sk.mass[i]) for i in range(nl)], dtype=torch.float64)
        P, V = torch.autograd.functional.jvp(lambda x: _coms(sk, x), (q,), (dq,), create_graph=True)
        L = L + 0.5 * (m * (V * V).sum(1)).sum() - gravity * (m * P[:, 2]).sum()
    if rotational:
        w = _omega_body(q[3:3 + 3 * nl].reshape(nl, 3), dq[3:3 + 3 * nl].reshape(nl, 3))
        L = L + 0.5 * (torch.tensor(inertia, dtype=torch.float64)[:nl] * w * w).sum()
    return L


def _rows(sk, inertia, gravity, q, dq, ddq, **parts):
    nq = sk.nq
    z = torch.tensor(np.concatenate([q, dq]), dtype=torch.float64)
    f = lambda x: lagrangian(sk, inertia, gravity, x[:nq], x[nq:], **parts)
    H = torch.autograd.functional.hessian(f, z, vectorize=True)
    g = torch.autograd.functional.jacobian(f, z)
    a, v = torch.tensor(ddq, dtype=torch.float64), torch.tensor(dq, dtype=torch.float64)
    return (H[nq:, nq:] @ a + H[nq:, :nq] @ v - g[:nq]).numpy()


_ROWS = {}


def eom_rows(sk, eopt, q, dq, ddq, gravity=None, root_inertia=None):
    """all nq rows of d/dt dL/dq' - dL/dq of one frame (N, N m); cached per input (a reference is computed once and shared)"""
    g = float(eopt.gravity) if gravity is None else float(gravity)
    inertia = [[float(eopt.link_inertia[i][k]) for k in range(3)] for i in range(sk.n_links)]
    if root_inertia is not None:
        root = [i for i in range(sk.n_links) if sk.parent[i] < 0][0]
        inertia[root] = [float(x) for x in root_inertia]
    q, dq, ddq = (np.ascontiguousarray(x, dtype=np.float64) for x in (q, dq, ddq))
    key = (bytes(sk), g, repr(inertia), q.tobytes(), dq.tobytes(), ddq.tobytes())
    if key not in _ROWS:
        _ROWS[key] = _rows(sk, inertia, g, q, dq, ddq)
    return _ROWS[key].copy()


def rotational_rows_autograd(sk, eopt, q, dq, ddq):
    """the rows of the rotational energy alone"""
    inertia = [[float(eopt.link_inertia[i][k]) for k in range(3)] for i in range(sk.n_links)]
    return _rows(sk, inertia, 0.0, np.asarray(q, float), np.asarray(dq, float), np.asarray(ddq, float), translational=False)


def rotational_rows_closed_form(sk, eopt, q, dq, ddq, drop_gyroscopic=False):
    """the same rows in closed form, (I alpha + w x I w) . dw/dq'_a per link with alpha = d/dt of the body rate: numpy, for the planted-error
    check of tests/test_dynamics_compare.py (drop_gyroscopic leaves w x I w out)"""
    out = np.zeros(sk.nq)
    for i in range(sk.n_links):
        a, da, dda = (np.asarray(x, float)[3 + 3 * i:6 + 3 * i] for x in (q, dq, ddq))
        sf, cf, st, ct = np.sin(a[0]), np.cos(a[0]), np.sin(a[1]), np.cos(a[1])
        Jw = np.array([[1.0, 0.0, -st], [0.0, cf, sf * ct], [0.0, -sf, cf * ct]])                       # w = Jw a'
        dJw = np.array([[0.0, 0.0, -ct * da[1]], [0.0, -sf * da[0], cf * ct * da[0] - sf * st * da[1]],
                        [0.0, -cf * da[0], -sf * ct * da[0] - cf * st * da[1]]])                          # d/dt Jw
        w, al = Jw @ da, Jw @ dda + dJw @ da
        I = np.array([float(eopt.link_inertia[i][k]) for k in range(3)])
        t = I * al + (0.0 if drop_gyroscopic else np.cross(w, I * w))
        out[3 + 3 * i:6 + 3 * i] = Jw.T @ t
    return out


# ---- generalised forces ----------------------------------------------------------------------------------------------------------------
def constraint_defs(sk):
    """(parent, child, child axis) of every joint-equality row: the order of skeleton.constraint_rows, x then z for a revolute joint"""
    rows, out, r = skeleton.constraint_rows(sk), [], 0
    for j in range(sk.n_joints):
        axes = (0, 2) if sk.joint_kind[j] == abi.JOINT_REVOLUTE_Y else (2,)
        for ax in axes:
            assert rows[r] == (sk.joint_parent[j], sk.joint_child[j])
            out.append((int(rows[r][0]), int(rows[r][1]), ax)); r += 1
    assert r == len(rows)
    return out


_TABLES = {}


def force_tables(sk, q, defs=None):
    """autograd Jacobians at q: Jm [n_markers, 3, nq] = d marker / dq, W [n_links, 3, nq] = d w_world / dq', R [n_links, 3, 3],
    Cq [n_constraints, nq] = dc/dq"""
    q = np.ascontiguousarray(q, dtype=np.float64)
    defs = tuple(constraint_defs(sk) if defs is None else defs)
    key = (bytes(sk), q.tobytes(), defs)
    if key in _TABLES:
        return _TABLES[key]
    qt = torch.tensor(q)
    jac = torch.autograd.functional.jacobian
    nl = sk.n_links
    Jm = jac(lambda x: _marker_points(sk, x), qt).numpy()
    R = _rotations(sk, qt)

    def w_world(v):
        return torch.einsum("iab,ib->ia", R, _omega_body(qt[3:3 + 3 * nl].reshape(nl, 3), v[3:3 + 3 * nl].reshape(nl, 3)))
    W = jac(w_world, torch.zeros(sk.nq, dtype=torch.float64)).numpy()
    ip, ic, ia = (torch.tensor([d[k] for d in defs]) for k in range(3))

    def cons(x):
        Rx = _rotations(sk, x)
        return (Rx[ip][:, :, 1] * Rx[ic][torch.arange(len(defs)), :, ia]).sum(1)
    Cq = jac(cons, qt).numpy()
    _TABLES[key] = dict(Jm=Jm, W=W, R=R.numpy(), Cq=Cq)
    return _TABLES[key]


def gen_forces(sk, dopt, q, tau=None, lam=None, grf=None, D=DK, defs=None):
    """the three families of generalised forces [nq] each (N, N m) for tau [n_motors], lam [n_constraints], grf [n_feet, 5] in body weights"""
    T = force_tables(sk, q, defs)
    Mg = total_mass(sk) * float(dopt.eom.gravity)
    out = dict(feet=np.zeros(sk.nq), motors=np.zeros(sk.nq), joints=np.zeros(sk.nq))
    if grf is not None:
        for f in range(dopt.n_feet):
            out["feet"] += T["Jm"][dopt.foot_marker[f]].T @ (Mg * (np.asarray(grf[f], float) @ D))
    if tau is not None:
        for m in range(dopt.n_motors):
            a1, a2, ax = dopt.motor_first[m], dopt.motor_second[m], dopt.motor_axis[m]
            out["motors"] += Mg * float(tau[m]) * (T["R"][a1][:, ax] @ (T["W"][a2] - T["W"][a1]))
    if lam is not None:
        out["joints"] = T["Cq"].T @ np.asarray(lam, float)
    return out


def row_scale(Mg, ref):
    """scale of one frame's rows: max(M g, largest |reference entry|)"""
    return max(Mg, float(np.abs(ref).max()))


def distance(got, ref, Mg):
    """worst |got - ref| / row_scale over frames: got, ref [..., n]; inf for a non-finite value"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    if not np.isfinite(got).all():
        return np.inf
    sc = np.maximum(Mg, np.abs(ref).max(-1, keepdims=True))
    return float((np.abs(got - ref) / sc).max())


# ---- the force-fit problem -------------------------------------------------------------------------------------------------------------
def fit_terms(sk, gopt, eopt, q, dq, ddq):
    """E [6] (body weights) and A [6, 5 n_feet] of one frame"""
    rows = eom_rows(sk, eopt, q, dq, ddq, gravity=gopt.gravity, root_inertia=gopt.root_inertia[:])
    E = rows[:6] / (total_mass(sk) * float(gopt.gravity))
    Jm = force_tables(sk, q)["Jm"]
    A = np.zeros((6, 5 * gopt.n_feet))
    for f in range(gopt.n_feet):
        A[:, 5 * f:5 * f + 5] = Jm[gopt.foot_marker[f]][:, :6].T @ DK.T
    return E, A


def project(t, mu, fmax):
    """exact projection of t [..., 5] onto {0 <= y <= fmax, sum_k y_k <= mu y_0} per foot, in t's dtype.  y = clamp(t - l a) with
    a = (-mu, 1, 1, 1, 1) and the smallest l >= 0 at which G(l) = sum_k clamp(t_k - l) - mu clamp(t_0 + mu l) <= 0; G is piecewise linear and
    non-increasing, so l lies between two neighbouring breakpoints (where one clamp opens or closes) and follows by linear interpolation."""
    dt = t.dtype.type
    mu, fmax = dt(mu), dt(fmax)
    z, x = t[..., :1], t[..., 1:]
    bp = [np.zeros_like(z), x, x - fmax]
    if mu > 0:
        bp += [-z / mu, (fmax - z) / mu]
    bp = np.sort(np.maximum(np.concatenate(bp, -1), 0), -1)                                    # [..., nb], bp[..., 0] = 0
    G = lambda l: np.clip(x[..., :, None] - l[..., None, :], 0, fmax).sum(-2) - mu * np.clip(z + mu * l, 0, fmax)
    g = G(bp)
    assert (g[..., -1] <= 0).all()
    first = np.argmax(g <= 0, -1)[..., None]                                                   # first breakpoint with G <= 0
    prev = np.maximum(first - 1, 0)
    lo, hi = np.take_along_axis(bp, prev, -1), np.take_along_axis(bp, first, -1)
    glo, ghi = np.take_along_axis(g, prev, -1), np.take_along_axis(g, first, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        l = np.where(first == 0, 0, lo + (hi - lo) * glo / (glo - ghi))
    return np.concatenate([np.clip(z + mu * l, 0, fmax), np.clip(x - l, 0, fmax)], -1)


def _solve(M, b):
    """dense Gaussian elimination with partial pivoting in M's dtype (numpy's solvers do not take np.longdouble)"""
    M, b = M.copy(), b.copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]; b[[k, p]] = b[[p, k]]
        m = M[k + 1:, k] / M[k, k]
        M[k + 1:, k:] -= m[:, None] * M[k, k:][None, :]; b[k + 1:] -= m * b[k]
    x = np.zeros_like(b)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - M[k, k + 1:] @ x[k + 1:]) / M[k, k]
    return x


class FitProblem:
    """the fits of F frames: A [F, 6, 5 nf], E [F, 6], contact [F, nf]; friction ratio mu, cap fmax, Tikhonov weight eps from cpe_grf_options.
    Forces y are [F, nf, 5] = (z, +x, +y, -x, -y) per foot in body weights."""

    def __init__(self, A, E, contact, gopt):
        self.A, self.E = np.asarray(A, float), np.asarray(E, float)
        self.F, self.nf = self.A.shape[0], self.A.shape[2] // 5
        self.contact = np.asarray(contact).astype(bool).reshape(self.F, self.nf)
        self.mu, self.fmax, self.eps = float(gopt.friction_ratio), float(gopt.force_max), float(gopt.regularisation)
        self.mask = np.repeat(self.contact, 5, axis=1)

    def _terms(self, dtype):
        A = self.A.astype(dtype) * self.mask.astype(dtype)[:, None, :]
        return A, self.E.astype(dtype), dtype(self.eps), dtype(self.eps) + (A * A).sum((1, 2))

    def _flat(self, y, dtype):
        return np.asarray(y, dtype).reshape(self.F, 5 * self.nf)

    def residual(self, y, dtype=LD):
        """E - A y [F, 6]"""
        A, E, _, _ = self._terms(dtype)
        return E - np.einsum("frc,fc->fr", A, self._flat(y, dtype))

    def objective(self, y, dtype=LD):
        y = self._flat(y, dtype)
        r = self.residual(y, dtype)
        return (r * r).sum(1) / 2 + dtype(self.eps) * (y * y).sum(1) / 2

    def gradient(self, y, dtype=LD):
        A, E, eps, _ = self._terms(dtype)
        y = self._flat(y, dtype)
        return eps * y - np.einsum("frc,fr->fc", A, E - np.einsum("frc,fc->fr", A, y))

    def _proj(self, t):
        return project(t.reshape(self.F, self.nf, 5), self.mu, self.fmax).reshape(self.F, -1) * self.mask.astype(t.dtype)

    def feasible(self, y, slack=0.0):
        y = np.asarray(y).reshape(self.F, self.nf, 5)
        return bool((y >= 0).all() and (y <= self.fmax).all() and (y[..., 1:].sum(-1) <= self.mu * y[..., 0] + slack).all()
                    and not y[~self.contact].any())

    def kkt_residual(self, y):
        """per frame [F]"""
        L = self._terms(LD)[3]
        y = self._flat(y, LD)
        return (np.abs(y - self._proj(y - self.gradient(y, LD) / L[:, None])).max(1) * L).astype(float)

    def one_step(self, dtype=np.float64):
        A, E, _, L = self._terms(dtype)
        return self._proj(np.einsum("frc,fr->fc", A, E) / L[:, None]).reshape(self.F, self.nf, 5)

    def fista(self, n_iter, dtype=np.float64):
        A, E, eps, L = self._terms(dtype)
        y = np.zeros((self.F, 5 * self.nf), dtype=dtype); v = y.copy()
        for it in range(n_iter):
            g = eps * v - np.einsum("frc,fr->fc", A, E - np.einsum("frc,fc->fr", A, v))
            yn = self._proj(v - g / L[:, None])
            v = yn + (dtype(it) / dtype(it + 3)) * (yn - y)
            y = yn
        return y.reshape(self.F, self.nf, 5)

    def minimiser(self):
        """[F, nf, 5] np.longdouble; asserts the certificate of every frame"""
        y = np.stack([self._minimiser(f) for f in range(self.F)])
        cert = self.kkt_residual(y)
        assert (cert <= CERT).all(), f"active-set minimiser: certificate {cert.max():.2e}"
        return y

    def _minimiser(self, fr):
        """primal active-set method (Nocedal and Wright, algorithm 16.3) on the feet in contact of frame fr, np.longdouble"""
        feet = [f for f in range(self.nf) if self.contact[fr, f]]
        y = np.zeros((self.nf, 5), dtype=LD)
        if not feet:
            return y
        n = 5 * len(feet)
        cols = np.concatenate([np.arange(5 * f, 5 * f + 5) for f in feet])
        A = self.A[fr].astype(LD)[:, cols]; E = self.E[fr].astype(LD)
        H = A.T @ A + LD(self.eps) * np.eye(n, dtype=LD); c = A.T @ E
        # constraints G x <= h: -x <= 0, x <= fmax, sum_k x_k - mu x_0 <= 0
        fric = np.zeros((len(feet), n), dtype=LD)
        for i in range(len(feet)):
            fric[i, 5 * i] = -LD(self.mu); fric[i, 5 * i + 1:5 * i + 5] = 1
        G = np.concatenate([-np.eye(n, dtype=LD), np.eye(n, dtype=LD), fric])
        h = np.concatenate([np.zeros(n, LD), np.full(n, LD(self.fmax)), np.zeros(len(feet), LD)])
        # start strictly inside (mu > 0): no constraint active, nothing degenerate.  mu = 0 leaves only x_k = 0: those bounds stay in the working
        # set for good and the friction rows (then implied) are left out.
        x = np.zeros(n, dtype=LD); W = []; keep = set()
        if self.mu > 0:
            z0 = LD(min(self.fmax, 1.0)) / 2
            for i in range(len(feet)):
                x[5 * i] = z0; x[5 * i + 1:5 * i + 5] = LD(self.mu) * z0 / 8
        else:
            x[0::5] = LD(self.fmax) / 2
            W = [i for i in range(n) if i % 5]; keep = set(W)
            G, h = G[:2 * n], h[:2 * n]
        for _ in range(100 * n):
            g = H @ x - c
            k = len(W)
            K = np.zeros((n + k, n + k), dtype=LD); K[:n, :n] = H
            K[:n, n:] = G[W].T; K[n:, :n] = G[W]
            sol = _solve(K, np.concatenate([-g, np.zeros(k, LD)]))
            p, lam = sol[:n], sol[n:]                           # x + p minimises on the working set's face
            Gp, room = G @ p, h - G @ x
            # the first constraint met on the way; a row that depends on the working set (a degenerate vertex: more than five of a foot's six rows)
            # has G p = 0 up to rounding and cannot block
            alpha, block = LD(1), None
            cand = sorted((max(room[i], LD(0)) / Gp[i], i) for i in range(len(h)) if i not in W and Gp[i] > 0 and room[i] < Gp[i])
            Gf = G.astype(float)
            for a, i in cand:
                if np.linalg.matrix_rank(Gf[W + [i]]) == k + 1:
                    alpha, block = a, i
                    break
            x = x + alpha * p
            if block is not None:
                W.append(block)
                continue
            free = [j for j in range(k) if W[j] not in keep]
            if not free or min(lam[j] for j in free) >= -LD(1e-16):
                break
            W.pop(min(free, key=lambda j: lam[j]))
        else:
            raise AssertionError("active-set method did not terminate")
        for i in W:                                              # a bound of the final working set holds exactly
            if i < 2 * n:
                x[i % n] = 0 if i < n else LD(self.fmax)
        y.reshape(-1)[cols] = np.clip(x, 0, LD(self.fmax))
        return y


# ---- inputs of the GPU tests -----------------------------------------------------------------------------------------------------------
H_FRAME = 1.0 / 120.0
LOW_GRAVITY = 3.7           # the second gravity of the options-lifetime test


def _differences(q):
    """backward differences of a trajectory q [N, nq] (the first frames repeat the first available value)"""
    dq = np.zeros_like(q); ddq = np.zeros_like(q)
    dq[1:] = (q[1:] - q[:-1]) / H_FRAME; dq[0] = dq[1]
    ddq[2:] = (q[2:] - 2 * q[1:-1] + q[:-2]) / H_FRAME ** 2; ddq[:2] = ddq[2]
    return dq, ddq


@functools.lru_cache(maxsize=None)
def gallop(name, n_frames=20, seed=17):
    sk = model(name)[0]
    q = synth.make_batch(sk, synth.make_cameras(1), B=1, N=n_frames, seed=seed)["q_true"][0]
    dq, ddq = _differences(q)
    return q, dq, ddq


LEG_LINK = 6                # "LFL": the link whose pitch is put next to pi / 2


@functools.lru_cache(maxsize=None)
def eom_cases(name):
    """q, dq, ddq [7, nq].  Frames 0-2: the velocity terms dominate (angles uniform in +-1.2, q' ~ N(0, 5), q'' ~ N(0, 50)); 3: the same with a leg
    link's theta within 1e-3 of pi / 2; 4: at rest (q' = q'' = 0); 5, 6: gallop frames.  B x N = 1 x 1 is frame 0, (2, 3) is frames 1-6."""
    sk = model(name)[0]
    rng = np.random.default_rng(1000 + MODELS.index(name))
    q = rng.uniform(-1.2, 1.2, (7, sk.nq)); dq = rng.normal(0, 5, (7, sk.nq)); ddq = rng.normal(0, 50, (7, sk.nq))
    q[3, 3 + 3 * LEG_LINK + 1] = np.pi / 2 - 7e-4
    dq[4] = 0; ddq[4] = 0
    g = gallop(name)
    for k, n in ((5, 6), (6, 13)):
        q[k], dq[k], ddq[k] = g[0][n], g[1][n], g[2][n]
    return q, dq, ddq


@functools.lru_cache(maxsize=None)
def force_map_case(name="phantom"):
    """one q and 68 frames of unit inputs: one-hot tau (22 frames), one-hot lambda (26), one-hot grf (20)"""
    sk, _, dopt, _ = model(name)
    q = eom_cases(name)[0][1]
    nm, nc, nf = dopt.n_motors, n_constraints(sk), dopt.n_feet
    F = nm + nc + 5 * nf
    tau = np.zeros((F, nm)); lam = np.zeros((F, nc)); grf = np.zeros((F, nf, 5))
    tau[np.arange(nm), np.arange(nm)] = 1
    lam[nm + np.arange(nc), np.arange(nc)] = 1
    grf.reshape(F, -1)[nm + nc + np.arange(5 * nf), np.arange(5 * nf)] = 1
    return q, tau, lam, grf


def force_inputs(name, n_frames, n_motors, n_feet, seed=2):
    sk = model(name)[0]
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.5, (n_frames, n_motors)), rng.normal(0, 0.5, (n_frames, n_constraints(sk))), rng.uniform(0, 2, (n_frames, n_feet, 5))


def dyn_variant(name, n_feet=None, reverse_feet=False, n_motors=None):
    """cpe_dyn_options with fewer feet (optionally in reversed order) and 0, 1 or 32 motors (32: the valid ones repeated)"""
    base = model(name)[2]
    o = abi.DynOptions.from_buffer_copy(base)
    if n_feet is not None:
        fm = list(base.foot_marker[:4])[::-1] if reverse_feet else list(base.foot_marker[:4])
        o.n_feet = n_feet
        for i in range(4):
            o.foot_marker[i] = fm[i] if i < n_feet else 0
    if n_motors is not None:
        o.n_motors = n_motors
        for i in range(32):
            j = i % base.n_motors
            o.motor_first[i], o.motor_second[i], o.motor_axis[i] = base.motor_first[j], base.motor_second[j], base.motor_axis[j]
    return o


def grf_variant(name, n_feet=4, reverse_feet=False, **fields):
    base = model(name)[3]
    o = abi.GrfOptions.from_buffer_copy(base)
    fm = list(base.foot_marker[:4])[::-1] if reverse_feet else list(base.foot_marker[:4])
    o.n_feet = n_feet
    for i in range(4):
        o.foot_marker[i] = fm[i] if i < n_feet else 0
    for k, v in fields.items():
        setattr(o, k, v)
    return o


@functools.lru_cache(maxsize=None)
def grf_pool(name):
    """16 gallop frames (q, dq, ddq [16, nq])"""
    q, dq, ddq = gallop(name)
    return q[3:19].copy(), dq[3:19].copy(), ddq[3:19].copy()


def contact_draw(n_frames, n_feet, seed=4, p=0.6):
    return (np.random.default_rng(seed).random((n_frames, n_feet)) < p).astype(np.int32)


def all_patterns():
    """the 16 contact patterns of four feet, frame n = bits of n"""
    return np.array([[(n >> f) & 1 for f in range(4)] for n in range(16)], dtype=np.int32)


def fit_problem(name, gopt, q, dq, ddq, contact):
    sk, eopt, _, _ = model(name)
    terms = [fit_terms(sk, gopt, eopt, q[n], dq[n], ddq[n]) for n in range(len(q))]
    return FitProblem(np.stack([t[1] for t in terms]), np.stack([t[0] for t in terms]), contact, gopt)


USES = ((True, True, True), (False, False, True), (True, False, False), (False, True, False))      # (tau, lambda, grf): together, each alone


@functools.lru_cache(maxsize=None)
def dyn_cases():
    """every input of the k_dyn_forces tests of tests/test_gpu_dynamics.py except the unit-input map (force_map_case): key -> dict(model, dopt,
    idx = frames of eom_cases, shape (B, N), tau, lam, grf (arrays or None))"""
    cases = {}

    def add(key, name, dopt, idx, shape, use, seed):
        tau, lam, grf = force_inputs(name, len(idx), dopt.n_motors, dopt.n_feet, seed)
        cases[key] = dict(model=name, dopt=dopt, idx=list(idx), shape=shape, tau=tau if use[0] else None, lam=lam if use[1] else None,
                          grf=grf if use[2] else None)

    for name in MODELS:
        add(f"{name}-1x1", name, model(name)[2], [0], (1, 1), USES[0], 3)
        for k, use in enumerate(USES):
            add(f"{name}-2x3-{'tlg'[0] * use[0]}{'l' * use[1]}{'g' * use[2]}", name, model(name)[2], range(1, 7), (2, 3), use, 4 + k)
    for nf in (0, 1, 3):
        add(f"feet-{nf}", "phantom", dyn_variant("phantom", n_feet=nf, reverse_feet=True), range(1, 7), (2, 3), USES[0], 10 + nf)
    for nm in (0, 1, 32):
        add(f"motors-{nm}", "phantom", dyn_variant("phantom", n_motors=nm), range(1, 7), (2, 3), USES[0], 20 + nm)
    return cases


def dyn_reference(case):
    """rows - Q [F, nq] of a case of dyn_cases(), and the rows alone"""
    sk, _, _, _ = model(case["model"])
    q, dq, ddq = (x[case["idx"]] for x in eom_cases(case["model"]))
    rows = np.stack([eom_rows(sk, case["dopt"].eom, q[n], dq[n], ddq[n]) for n in range(len(q))])
    Q = np.zeros_like(rows)
    for n in range(len(q)):
        Q[n] = sum(gen_forces(sk, case["dopt"], q[n], None if case["tau"] is None else case["tau"][n], None if case["lam"] is None else case["lam"][n],
                              None if case["grf"] is None else case["grf"][n]).values())
    return rows - Q, rows


def gravity_torques(sk, gravity, q):
    """dV/dq [nq] of V = sum_i m_i g P_i,z: what the rows are at rest"""
    m = torch.tensor([float(sk.mass[i]) for i in range(sk.n_links)], dtype=torch.float64)
    return torch.autograd.functional.jacobian(lambda x: gravity * (m * _coms(sk, x)[:, 2]).sum(), torch.tensor(np.asarray(q, float))).numpy()


SHORT = 200                 # FISTA iterations of the cases that are about shapes, packing and contact patterns


@functools.lru_cache(maxsize=None)
def grf_cases():
    """name -> dict(model, gopt, q, dq, ddq [F, nq], contact [F, nf], shape (B, N)): every input of the force-fit tests of tests/test_gpu_dynamics.py"""
    cases = {}

    def add(key, name, gopt, F, contact, shape=None):
        q, dq, ddq = (x[:F] for x in grf_pool(name))
        cases[key] = dict(model=name, gopt=gopt, q=q, dq=dq, ddq=ddq, contact=np.ascontiguousarray(contact, dtype=np.int32), shape=shape or (1, F))

    for (B, N) in ((1, 1), (1, 2), (2, 2), (1, 5), (1, 7), (2, 3)):                                  # 1, 2, 4, 5, 7 and 6 frames: packs of three and tails
        c = contact_draw(B * N, 4, seed=10 + B * N); c[0, 1] = 1
        add(f"frames-{B}x{N}", "phantom", grf_variant("phantom", iterations=SHORT), B * N, c, (B, N))
    for nf in (1, 2, 3, 4):                                                                       # nv = 5, 10, 15, 20; three feet in reversed order
        c = contact_draw(7, nf, seed=20 + nf); c[1] = 1; c[2] = 0
        add(f"feet-{nf}", "phantom", grf_variant("phantom", n_feet=nf, reverse_feet=nf == 3, iterations=SHORT), 7, c)
    add("patterns", "phantom", grf_variant("phantom", iterations=SHORT), 16, all_patterns())
    add("flight-packs", "phantom", grf_variant("phantom", iterations=SHORT), 6, [[0] * 4, [1] * 4] + [[0] * 4] * 4)
    c7 = contact_draw(7, 4, seed=30); c7[3] = 1
    for it in (1, 2):
        add(f"iterations-{it}", "phantom", grf_variant("phantom", iterations=it), 7, c7)
    add("phantom-2000", "phantom", grf_variant("phantom", iterations=2000), 16, contact_draw(16, 4))
    add("acinoset-2000", "acinoset", grf_variant("acinoset", iterations=2000), 6, contact_draw(6, 4, seed=5))
    add("cap", "phantom", grf_variant("phantom", iterations=2000, force_max=0.3), 16, contact_draw(16, 4))
    add("no-friction", "phantom", grf_variant("phantom", iterations=2000, friction_ratio=0.0), 16, contact_draw(16, 4))
    return cases


TRUNCATION_CASES = ("phantom-2000", "acinoset-2000")
BINDING_CASES = ("phantom-2000", "cap", "no-friction")              # default mu = 1.3, force_max = 0.3, friction_ratio = 0


@functools.lru_cache(maxsize=None)
def case_problem(key):
    c = grf_cases()[key]
    return fit_problem(c["model"], c["gopt"], c["q"], c["dq"], c["ddq"], c["contact"])


@functools.lru_cache(maxsize=None)
def case_fista(key, extended=False):
    """the reference's FISTA with the case's own iteration count [F, nf, 5]"""
    return case_problem(key).fista(int(grf_cases()[key]["gopt"].iterations), LD if extended else np.float64)


@functools.lru_cache(maxsize=None)
def case_minimiser(key):
    return case_problem(key).minimiser()


def binding_share(key):
    """share of the case's contact frames (at least one foot down) in which the case's constraint is active at the certified minimiser: a foot on its
    friction cone with a force on it ("phantom-2000"), a component at force_max ("cap"); for "no-friction" a foot that carries friction at mu = 1.3"""
    P, y = case_problem(key), case_minimiser(key)
    if key == "cap":
        hit = (np.abs(y - P.fmax) < 1e-12).any(-1)
    elif key == "no-friction":
        assert not y[..., 1:].any()
        hit = case_minimiser("phantom-2000")[..., 1:].sum(-1) > 1e-6
    else:
        hit = (np.abs(y[..., 1:].sum(-1) - P.mu * y[..., 0]) < 1e-12) & (y[..., 0] > 1e-6)
    frames = P.contact.any(1)
    return float((hit & P.contact).any(1)[frames].mean())


# the float64-vs-longdouble distance of fista() and the truncation distance: recomputed and asserted by tests/test_dynamics_compare.py
# (test_fista_float64_distance, test_truncation_distance_is_the_recorded_one)
FISTA_F64_LD = dict(force=1.28e-13, residual=2.20e-15)
TRUNCATION = dict(force=1.35e-2, residual=1.52e-6, objective=7.96e-10)
TOL_FIT = 1e-8
