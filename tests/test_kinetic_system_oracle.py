"""The oracle's band system of the physics-based model (oracle.kinetic_system, the reference side of cpe_eval_kinetic_system) and the
comparator the GPU tests use (tests/kinetic_compare.py).  No GPU here: the HIP side is tests/test_gpu_kinetic_nodes.py."""
import numpy as np
import pytest

import kinetic_compare as KC
from test_kinetic_oracle import _problem

NU = 28
MUTATIONS = (("w_smooth", 1.01), ("w_torque", 1.001), ("kappa_force", 1.01), ("kappa_height", 1.01), ("kappa_slip", 1.01),
             ("kappa_slack", 1.01), ("lm_force_damping", 1.01), ("lm_wall_damping", 1.01))


def _band_blocks(band, N):
    """diagonal and the two sub-diagonal 28 x 28 blocks of cpo_kinetic_objective's band (row i holds AB(i, i - c) in column c)"""
    AB = lambda i, j: band[i, i - j]
    Bk = np.array([[[AB(m * NU + max(i, j), m * NU + min(i, j)) for j in range(NU)] for i in range(NU)] for m in range(N)])
    Hk = np.zeros((N, 2, NU, NU))
    for m in range(N):
        for t in range(2):
            if m >= t + 1:
                Hk[m, t] = [[AB(m * NU + i, (m - 1 - t) * NU + j) for j in range(NU)] for i in range(NU)]
    return Bk, Hk


def _sensitive_problem():
    """phantom, 2 cameras, 10 frames, two feet in stance; slip_max 0.02 and a slack box of +-0.01 so that those rows bind"""
    sk, cams, opts, ko, d = _problem(10)
    ko = KC.with_options(ko, slip_max=0.02, slack_lo=-0.01, slack_hi=0.01)
    return sk, cams, opts, ko, d["q_init"][0], d["meas"][0], d["weight"][0], d["stance"][0]


def test_comparator_flags_a_one_percent_change_of_every_term(oracle):
    """each cost weight, penalty and damping factor scaled by 1.01 (w_torque by 1.001) moves the oracle's own outputs by at least 100 x the
    tolerance the GPU comparison uses, on data where that row family is active"""
    sk, cams, opts, ko, q, me, we, st = _sensitive_problem()
    assert st[2:].sum() > 0
    lam = 0.1
    ev = lambda k: oracle.kinetic_system(sk, cams, opts, None, k, q, me, we, st, lam=lam)
    R = ev(ko)
    V = oracle.kinetic_objective(sk, cams, opts, None, ko, q, me, we, st, want_grad=False)[0]
    for field in ("kappa_force", "kappa_height", "kappa_slip", "kappa_slack"):
        assert KC.multiplier_terms_move(ev, ko, field), field                # the rows this penalty weighs are active
    assert R["stat"][2:, 3].min() > 0 and R["stat"][2:, 1].min() > 0         # smoothing energy and torques in every node
    for field, fac in MUTATIONS:
        M = ev(KC.with_options(ko, **{field: getattr(ko, field) * fac}))
        d = KC.discrepancies(M, R, sk, ko, V)
        signal = max(v / KC.TOL[k] for k, v in d.items() if k != "meta")
        print(f"{field} x {fac}: " + ", ".join(f"{k} {v:.1e}" for k, v in d.items() if k != "meta") + f"  -> {signal:.1e} x tolerance")
        assert signal >= 100.0, (field, d)
    for field in ("lm_force_damping", "lm_wall_damping"):                     # the damping terms act on the band only
        M = ev(KC.with_options(ko, **{field: getattr(ko, field) * 1.01}))
        assert all(np.array_equal(M[k], R[k]) for k in KC.NODE_KEYS) and not np.array_equal(M["Bk"], R["Bk"])


def test_comparator_scales_and_structural_zeros(oracle):
    """the comparator itself: identical outputs give 0, a change in a structural zero is infinite, a change of one entry by 1e-6 of its scale
    reads as 1e-6, meta is compared exactly"""
    sk, cams, opts, ko, q, me, we, st = _sensitive_problem()
    R = oracle.kinetic_system(sk, cams, opts, None, ko, q, me, we, st, lam=0.1)
    V = 1.0
    assert all(v == 0.0 for v in KC.discrepancies(R, R, sk, ko, V).values())
    S = KC.scales(R, sk, ko, V)
    G = {k: v.copy() for k, v in R.items()}
    G["Huu"][5, 3, 7] += 1e-6 * S["Huu"][5, 3, 7]
    assert abs(KC.discrepancies(G, R, sk, ko, V)["Huu"] - 1e-6) < 1e-12
    G = {k: v.copy() for k, v in R.items()}
    G["Huu"][0, 0, 0] = 1e-300                                                # node 0 has no dynamics: its pieces are zero
    assert KC.discrepancies(G, R, sk, ko, V)["Huu"] == float("inf")
    G = {k: v.copy() for k, v in R.items()}
    G["Hk"][0, 0, 1, 1] = 1e-300                                              # frame 0 has no block (0, -1)
    assert KC.discrepancies(G, R, sk, ko, V)["Hk"] == float("inf")
    G = {k: v.copy() for k, v in R.items()}
    G["meta"][4, 1] += 1
    assert KC.discrepancies(G, R, sk, ko, V)["meta"] == float("inf")


def test_system_node_outputs_equal_kinetic_nodes(oracle):
    """kinetic_system without a variant gives kinetic_nodes' per-node outputs bit for bit (kinetic_nodes is a thin wrapper over it)"""
    sk, cams, opts, ko, d = _problem(9)
    q, st = d["q_init"][0], d["stance"][0]
    A = oracle.kinetic_nodes(sk, cams, opts, ko, q, st)
    S = oracle.kinetic_system(sk, cams, opts, None, ko, q, d["meas"][0], d["weight"][0], st, lam=0.1)
    for k in KC.NODE_KEYS + ("meta",):
        assert np.array_equal(A[k], S[k]), k


@pytest.mark.parametrize("N", [1, 2, 7])
def test_band_at_zero_damping_equals_the_objective_band(oracle, N):
    """at lam = 0 and without a variant, the band system is cpo_kinetic_objective's gradient and band matrix bit for bit; N = 1, 2 have no
    node, and their blocks are the per-frame terms alone"""
    sk, cams, opts, ko, d = _problem(max(N, 3))
    q, me, we, st = d["q_init"][0][:N], d["meas"][0][:N], d["weight"][0][:N], d["stance"][0][:N]
    S = oracle.kinetic_system(sk, cams, opts, None, ko, q, me, we, st, lam=0.0)
    _, g, _, _, band = oracle.kinetic_objective(sk, cams, opts, None, ko, q, me, we, st, want_band=True)
    Bk, Hk = _band_blocks(band, N)
    assert np.array_equal(S["gk"], g) and np.array_equal(S["Bk"], Bk) and np.array_equal(S["Hk"], Hk)
    assert np.array_equal(S["Bk"], np.swapaxes(S["Bk"], 1, 2))
    if N < 3:
        assert not S["f"].any() and not S["Huu"].any() and not S["Hk"][:, 1].any()


@pytest.mark.parametrize("variant", ["free", "grf_fixed", "tau_box", "grf_box"])
def test_band_gradient_of_the_projected_objective_per_variant(oracle, variant):
    """for each variant, the band gradient is the gradient of the projected objective (the node forces minimised out, envelope theorem):
    central differences of cpo_kinetic_objective_variant agree with it, as in test_gradient_of_the_projected_objective"""
    sk, cams, opts, ko, d = _problem(6)
    q, me, we, st = d["q_init"][0], d["meas"][0], d["weight"][0], d["stance"][0]
    R0 = oracle.kinetic_system(sk, cams, opts, None, ko, q, me, we, st)
    var = {} if variant == "free" else {variant: KC.variants(R0, sk, ko)[variant]}
    S = oracle.kinetic_system(sk, cams, opts, None, ko, q, me, we, st, lam=1.0, **var)
    f0, g, qc, terms, _ = oracle.kinetic_objective(sk, cams, opts, None, ko, q, me, we, st, **var)
    assert np.array_equal(S["gk"], g) and terms[6] > 0                          # (the gradient does not depend on the damping)
    if variant == "tau_box":
        tb = var["tau_box"][2:]
        tau = S["f"][2:, :ko.dyn.n_motors]
        assert np.any((tau < tb[..., 0]) | (tau > tb[..., 1]))                  # the boxes bind
    if variant == "grf_box":
        nm, nc = ko.dyn.n_motors, KC.n_constraint_forces(sk)
        F = S["f"][2:, nm + nc:nm + nc + 12].reshape(-1, 4, 3)
        on = st[2:] == 1
        gb = var["grf_box"][2:]
        assert np.any(((F < gb[..., 0]) | (F > gb[..., 1]))[on])
    if variant == "grf_fixed":
        assert (S["meta"][2:, 0] == ko.dyn.n_motors + KC.n_constraint_forces(sk)).all()
    eps, worst = 1e-6, 0.0
    rng = np.random.default_rng(1)
    for n, k in zip(rng.integers(0, 6, 30), rng.integers(0, 28, 30)):
        fa = oracle.kinetic_objective(sk, cams, opts, None, ko, oracle.move_coordinate(sk, qc, n, k, eps), me, we, st, want_grad=False, **var)[0]
        fb = oracle.kinetic_objective(sk, cams, opts, None, ko, oracle.move_coordinate(sk, qc, n, k, -eps), me, we, st, want_grad=False, **var)[0]
        fd = (fa - fb) / (2 * eps)
        worst = max(worst, abs(fd - g[n, k]) / max(1.0, abs(fd)))
    print(f"{variant}: worst relative difference {worst:.1e}")
    assert worst < 5e-4, worst
