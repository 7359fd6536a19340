"""k_eom, k_dyn_forces and k_grf (cpe_eom_rows, cpe_eom_residual, cpe_grf_fit) entry by entry against the independent references of
tests/dynamics_compare.py: autograd equations of motion, autograd force Jacobians, and a plain numpy FISTA with an exact projection plus a
certified minimiser.  tests/test_dynamics_compare.py holds those references against the oracle on the same inputs (CPU).

Tolerances (none of them comes from the kernels' output):
  rows, generalised forces   1e-10 x max(M g, largest |reference row| of the frame): the figure the project asserts for these kernels (DC.TOL_ROWS)
  force fit vs fista(n)      max(1e-8, 32 x 1.28e-13) = 1e-8: 1.28e-13 is the float64-vs-longdouble distance of the reference's own FISTA on these inputs
                             (DC.TOL_FIT; the rule of tests/frame_compare.py)
  E of a flight frame        1e-10 x max(1, largest |E|): the row tolerance in body weights
  objective, residual after 2 000 iterations vs the certified minimiser: twice the recorded truncation distance (DC.TRUNCATION)

The kernels' worst observed values on an MI355X (printed after the module's tests with -s; they never fed a tolerance):
  k_eom rows 1.0e-15 of the scale; k_dyn_forces residual 1.0e-15; unit-input map 2.6e-16
  k_grf vs fista(n): forces 1.9e-13, residual 3.9e-15; E of flight frames 1.9e-16; vs the oracle (2 000 iterations) 1.3e-13
  2 000 iterations vs the certified minimiser: objective gap 8.0e-10, residual 1.5e-6 (the truncation distance itself, as on the CPU)

What the file found: with n_feet = 1 k_grf left residual[5] of every frame unwritten (five lanes per frame, six rows; case "feet-1").
"""
import numpy as np
import pytest

import dynamics_compare as DC
from cheetah_pose_estimation_amd import abi, synth

pytestmark = pytest.mark.gpu

WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    return float(value)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """after the module's tests: the worst value of every comparison that ran (shown with -s)"""
    yield
    if WORST:
        print("\nworst observed: " + "; ".join(f"{k} {v:.1e}" for k, v in WORST.items()))


_HANDLES = {}


def _handle(factory, name):
    if name not in _HANDLES:
        _HANDLES[name] = factory(DC.model(name)[0], synth.make_cameras(1))
    return _HANDLES[name]


def _dev(a, shape=None, dtype=None):
    import torch
    t = torch.tensor(np.ascontiguousarray(a, dtype=dtype or np.float64), device=torch.device("cuda", 0))
    return t if shape is None else t.reshape(shape).contiguous()


def _frames(name, idx, shape):
    q, dq, ddq = (x[list(idx)] for x in DC.eom_cases(name))
    nq = q.shape[1]
    return q, dq, ddq, tuple(_dev(x, shape + (nq,)) for x in (q, dq, ddq))


def _eom_rows(h, eopt, dev, shape):
    import torch
    rows = torch.full(shape + (dev[0].shape[-1],), float("nan"), dtype=torch.float64, device=dev[0].device)
    h.eom_rows(eopt, *dev, rows)
    h.synchronize()
    return rows.cpu().numpy().reshape(-1, rows.shape[-1])


# ---- k_eom ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 3)])
@pytest.mark.parametrize("name", DC.MODELS)
def test_eom_rows_match_the_autograd_lagrangian(name, shape, gpu_handle_factory):
    """every row of every frame: high rates (velocity terms dominate), a leg link's theta next to pi / 2, rest, gallop"""
    sk, eopt, _, _ = DC.model(name)
    Mg = DC.total_mass(sk) * eopt.gravity
    idx = [0] if shape == (1, 1) else range(1, 7)
    q, dq, ddq, dev = _frames(name, idx, shape)
    got = _eom_rows(_handle(gpu_handle_factory, name), eopt, dev, shape)
    ref = np.stack([DC.eom_rows(sk, eopt, q[n], dq[n], ddq[n]) for n in range(len(q))])
    d = _note("k_eom rows", DC.distance(got, ref, Mg))
    print(f"\nk_eom {name} {shape}: {d:.2e}")
    assert d < DC.TOL_ROWS
    if shape == (2, 3):                                                         # frame 4 of the cases is at rest: index 3 here
        assert not dq[3].any() and not ddq[3].any()
        assert np.abs(got[3, :3] - [0, 0, Mg]).max() < DC.TOL_ROWS * Mg
        assert np.abs(got[3] - DC.gravity_torques(sk, eopt.gravity, q[3])).max() < DC.TOL_ROWS * Mg


def test_eom_options_belong_to_their_call(gpu_handle_factory):
    """cpe_eom_rows keeps a device copy of the caller's options: two calls in a row with different gravity, without synchronising in between and behind
    a launch that keeps the stream busy, and a struct overwritten right after its call returns -- each output matches the options of its own call"""
    import torch
    name = "phantom"
    sk, eopt, _, _ = DC.model(name)
    h = _handle(gpu_handle_factory, name)
    q, dq, ddq, dev = _frames(name, range(1, 7), (2, 3))
    low = abi.EomOptions.from_buffer_copy(eopt); low.gravity = DC.LOW_GRAVITY
    mine = abi.EomOptions.from_buffer_copy(eopt)
    big = tuple(x.reshape(1, 6, -1).repeat(4096, 1, 1).contiguous() for x in dev)      # 24 576 frames ahead of the calls under test
    out = [torch.full(x, float("nan"), dtype=torch.float64, device=dev[0].device) for x in ((4096, 6, sk.nq), (2, 3, sk.nq), (2, 3, sk.nq), (2, 3, sk.nq))]
    h.synchronize()
    h.eom_rows(eopt, *big, out[0])
    h.eom_rows(eopt, *dev, out[1])
    h.eom_rows(low, *dev, out[2])
    h.eom_rows(mine, *dev, out[3])
    mine.gravity = 1.0
    for i in range(sk.n_links):
        mine.link_inertia[i][0] = 0.0
    h.synchronize()
    ref = {g: np.stack([DC.eom_rows(sk, eopt, q[n], dq[n], ddq[n], gravity=g) for n in range(6)]) for g in (eopt.gravity, DC.LOW_GRAVITY)}
    assert DC.distance(ref[eopt.gravity], ref[DC.LOW_GRAVITY], 1.0) > 1e-3         # the two gravities are told apart
    for k, g in ((1, eopt.gravity), (2, DC.LOW_GRAVITY), (3, eopt.gravity)):
        assert DC.distance(out[k].cpu().numpy().reshape(6, -1), ref[g], DC.total_mass(sk) * g) < DC.TOL_ROWS, k
    first = out[0].cpu().numpy()
    for b in (0, 2047, 4095):
        assert DC.distance(first[b], ref[eopt.gravity], DC.total_mass(sk) * eopt.gravity) < DC.TOL_ROWS


# ---- k_dyn_forces --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(DC.dyn_cases()))
def test_eom_residual_matches_the_autograd_forces(key, gpu_handle_factory):
    """rows - Q for tau, lambda and grf together and each alone, 1 x 1 and 2 x 3 frames, three skeletons; 0, 1 and 3 feet in reversed order; 0, 1 and 32 motors"""
    import torch
    c = DC.dyn_cases()[key]
    sk, dopt, shape = DC.model(c["model"])[0], c["dopt"], c["shape"]
    Mg = DC.total_mass(sk) * dopt.eom.gravity
    _, _, _, dev = _frames(c["model"], c["idx"], shape)
    arg = [None if c[k] is None or c[k].size == 0 else _dev(c[k], shape + c[k].shape[1:]) for k in ("tau", "lam", "grf")]
    res = torch.full(shape + (sk.nq,), float("nan"), dtype=torch.float64, device=dev[0].device)
    h = _handle(gpu_handle_factory, c["model"])
    h.eom_residual(dopt, *dev, *arg, res)
    h.synchronize()
    ref, rows = DC.dyn_reference(c)
    got = res.cpu().numpy().reshape(ref.shape)
    scale = np.maximum(Mg, np.abs(rows).max(-1, keepdims=True))
    d = _note("k_dyn_forces residual", np.inf if not np.isfinite(got).all() else (np.abs(got - ref) / scale).max())
    print(f"\nk_dyn_forces {key}: {d:.2e}")
    assert d < DC.TOL_ROWS
    assert np.abs(ref - rows).max() > 1e-3 * Mg or not any(a is not None for a in arg)      # the forces are visible in the residual


def test_unit_inputs_give_every_column_of_the_force_map(gpu_handle_factory):
    """one batch of 68 frames at one q (at rest, so that M g is the scale): one-hot tau (22), one-hot lambda (26), one-hot grf (20).  Every column of Q:
    each motor's sign and axis, the running constraint-row counter (two rows per revolute joint, one per Hooke joint), each D_k of each foot"""
    import torch
    sk, _, dopt, _ = DC.model("phantom")
    Mg = DC.total_mass(sk) * dopt.eom.gravity
    q, tau, lam, grf = DC.force_map_case()
    F = len(tau)
    assert F == 68 and DC.n_constraints(sk) == 26
    qd = _dev(np.repeat(q[None], F, 0), (4, 17, sk.nq)); zero = torch.zeros_like(qd)
    res = torch.full((4, 17, sk.nq), float("nan"), dtype=torch.float64, device=qd.device)
    h = _handle(gpu_handle_factory, "phantom")
    h.eom_residual(dopt, qd, zero, zero, _dev(tau, (4, 17, 22)), _dev(lam, (4, 17, 26)), _dev(grf, (4, 17, 4, 5)), res)
    h.synchronize()
    got = res.cpu().numpy().reshape(F, sk.nq)
    rows = DC.eom_rows(sk, dopt.eom, q, 0 * q, 0 * q)
    worst = 0.0
    for f in range(F):
        Q = sum(DC.gen_forces(sk, dopt, q, tau[f], lam[f], grf[f]).values())
        assert np.abs(Q).max() > 1e-3                                          # no column of the map is empty
        d = DC.distance(rows - got[f], Q, Mg)
        assert d < DC.TOL_ROWS, (f, d)
        worst = max(worst, d)
    print(f"\nforce map: {_note('unit-input map', worst):.2e}")


# ---- k_grf ---------------------------------------------------------------------------------------------------------------------------------
PAD = 3                     # frames of sentinel behind every output


def _fit(h, c, with_residual=True):
    """forces [F, nf, 5] and residual [F, 6] (or None) of a case through Handle.grf_fit; the outputs are allocated PAD frames longer than needed and
    filled with NaN: the extra frames must come back untouched and every real frame written"""
    import torch
    (B, N), gopt = c["shape"], c["gopt"]
    F, nf, nq = B * N, gopt.n_feet, c["q"].shape[1]
    dev = torch.device("cuda", 0)
    buf = [torch.full(((F + PAD) * w,), float("nan"), dtype=torch.float64, device=dev) for w in (nf, 4 * nf, 6)]
    gz, gxy, res = buf[0][:F * nf].view(B, N, nf), buf[1][:F * nf * 4].view(B, N, nf, 4), buf[2][:F * 6].view(B, N, 6)
    h.grf_fit(gopt, _dev(c["q"], (B, N, nq)), _dev(c["dq"], (B, N, nq)), _dev(c["ddq"], (B, N, nq)), _dev(c["contact"], (B, N, nf), np.int32),
              gz, gxy, res if with_residual else None)
    h.synchronize()
    host = [b.cpu().numpy() for b in buf]
    for k, (b, w) in enumerate(zip(host, (nf, 4 * nf, 6))):
        assert np.isnan(b[F * w:]).all(), "wrote behind the last frame"
        if k < 2 or with_residual:
            assert np.isfinite(b[:F * w]).all(), "left an entry of a real frame unwritten"
        else:
            assert np.isnan(b).all()
    y = np.concatenate([host[0][:F * nf].reshape(F, nf, 1), host[1][:F * nf * 4].reshape(F, nf, 4)], -1)
    return y, host[2][:F * 6].reshape(F, 6) if with_residual else None


@pytest.mark.parametrize("key", list(DC.grf_cases()))
def test_grf_fit_matches_the_plain_fista(key, oracle, gpu_handle_factory):
    """every case of dynamics_compare.grf_cases(): 1, 2, 4, 5, 7 and 6 frames (tail packs), 1-4 feet, all 16 contact patterns, flight packs,
    1, 2 and 2 000 iterations on two skeletons, the cap and the friction cone binding, no friction at all"""
    c = DC.grf_cases()[key]
    P, gopt = DC.case_problem(key), c["gopt"]
    y, res = _fit(_handle(gpu_handle_factory, c["model"]), c)
    # feasibility outright
    assert (y >= 0).all() and (y <= gopt.force_max).all() and (y[..., 1:].sum(-1) <= gopt.friction_ratio * y[..., 0] + 1e-12).all()
    assert not y[~P.contact].any()
    # flight frames: exactly zero forces, and the residual is E -- the only place the kernel's six rows are visible
    flight = ~P.contact.any(1)
    assert not y[flight].any()
    if flight.any():
        dE = (np.abs(res[flight] - P.E[flight]) / np.maximum(1.0, np.abs(P.E[flight]).max(1, keepdims=True))).max()
        print(f"\nk_grf {key}: E of {int(flight.sum())} flight frames {_note('k_grf flight E', dE):.2e}")
        assert dE < DC.TOL_ROWS
    # the same iteration count in plain numpy
    ref = DC.case_fista(key)
    dy, dr = np.abs(y - ref).max(), np.abs(res - P.residual(ref, np.float64)).max()
    print(f"\nk_grf {key}: forces {_note('k_grf forces vs fista', dy):.2e}, residual {_note('k_grf residual vs fista', dr):.2e}")
    assert dy < DC.TOL_FIT and dr < DC.TOL_FIT
    if key in DC.BINDING_CASES:                                                # the case's constraint is active at the certified minimiser
        assert DC.binding_share(key) >= 1 / 3
    if key == "iterations-1":
        assert np.abs(y - P.one_step()).max() < DC.TOL_FIT and y.any()
    if key == "no-friction":
        assert not y[..., 1:].any() and y[..., 0].max() > 0.1
    if key == "cap":
        assert (y == gopt.force_max).any()
    if int(gopt.iterations) == 2000:                                           # against the oracle as before
        sk = DC.model(c["model"])[0]
        oz, oxy, ores = oracle.grf_fit(sk, gopt, c["q"], c["dq"], c["ddq"], c["contact"])
        do = max(np.abs(oz - y[..., 0]).max(), np.abs(oxy - y[..., 1:]).max(), np.abs(ores - res).max())
        print(f"k_grf {key}: vs oracle {_note('k_grf vs oracle', do):.2e}")
        assert do < 1e-8
    if key in DC.TRUNCATION_CASES:                                             # the documented deviation: the objective and the net wrench are there
        ym = DC.case_minimiser(key)
        gap = float((P.objective(y) - P.objective(ym)).max())
        dres = float(np.abs(res - P.residual(ym)).max())
        print(f"k_grf {key}: objective gap {_note('objective gap to the minimiser', gap):.2e}, residual {_note('residual vs the minimiser', dres):.2e}")
        assert -1e-15 <= gap <= 2 * DC.TRUNCATION["objective"] and dres <= 2 * DC.TRUNCATION["residual"]


def test_grf_fit_without_a_residual_buffer(gpu_handle_factory):
    """residual = NULL skips the last store and nothing else: the forces are the same bit for bit"""
    for key in ("feet-3", "frames-1x5", "patterns"):
        c = DC.grf_cases()[key]
        h = _handle(gpu_handle_factory, c["model"])
        y, _ = _fit(h, c)
        y0, none = _fit(h, c, with_residual=False)
        assert none is None and np.array_equal(y, y0) and y.any()
