"""The references of tests/dynamics_compare.py held against the oracle on every input of tests/test_gpu_dynamics.py, the teeth of the comparison,
and the truncation distance of the force fit as a documented deviation.  CPU only.

Reference vs oracle (test_references_match_the_oracle; the condition is 1e-12 of the scale, on the references, not a tolerance for a kernel),
measured:
    rows 3.6e-16   feet 3.1e-16   motors 4.4e-16   joints 1.4e-18   E 5.2e-16   A 5.6e-17

float64 vs np.longdouble evaluation of the reference's own FISTA on the inputs of the GPU force-fit tests (test_fista_float64_distance), measured:
    forces 1.28e-13   residual 2.20e-15      32 x 1.28e-13 = 4.1e-12 < 1e-8: the GPU tolerance is the project's 1e-8

Truncation: fista(2000, longdouble) vs the certified minimiser on the committed stance frames (test_truncation_distance_is_the_recorded_one), measured:
    forces 1.35e-2 body weights   residual 1.52e-6   objective 7.96e-10
"""
import numpy as np
import pytest

import dynamics_compare as DC
from cheetah_pose_estimation_amd import abi

LD = np.longdouble


def test_references_match_the_oracle(oracle):
    worst = dict(rows=0.0, feet=0.0, motors=0.0, joints=0.0, E=0.0, A=0.0)
    for name in DC.MODELS:
        sk, eopt, dopt, _ = DC.model(name)
        Mg = DC.total_mass(sk) * eopt.gravity
        q, dq, ddq = DC.eom_cases(name)
        for n in range(len(q)):
            worst["rows"] = max(worst["rows"], DC.distance(oracle.eom_rows(sk, eopt, q[n], dq[n], ddq[n]), DC.eom_rows(sk, eopt, q[n], dq[n], ddq[n]), Mg))
    # the second gravity of the options-lifetime test
    sk, eopt, _, _ = DC.model("phantom")
    low = abi.EomOptions.from_buffer_copy(eopt); low.gravity = DC.LOW_GRAVITY
    q, dq, ddq = DC.eom_cases("phantom")
    for n in range(1, 7):
        worst["rows"] = max(worst["rows"], DC.distance(oracle.eom_rows(sk, low, q[n], dq[n], ddq[n]), DC.eom_rows(sk, low, q[n], dq[n], ddq[n]),
                                                     DC.total_mass(sk) * DC.LOW_GRAVITY))
    # the force families of every case, one at a time
    for key, c in DC.dyn_cases().items():
        sk, dopt = DC.model(c["model"])[0], c["dopt"]
        Mg = DC.total_mass(sk) * dopt.eom.gravity
        qs = DC.eom_cases(c["model"])[0][c["idx"]]
        for n in range(len(qs)):
            tau, lam, grf = (None if c[k] is None else c[k][n] for k in ("tau", "lam", "grf"))
            ref = DC.gen_forces(sk, dopt, qs[n], tau, lam, grf)
            for fam, kw in (("feet", dict(grf=grf)), ("motors", dict(tau=tau)), ("joints", dict(lam=lam))):
                if next(iter(kw.values())) is not None and next(iter(kw.values())).size:
                    worst[fam] = max(worst[fam], DC.distance(oracle.dyn_forces(sk, dopt, qs[n], **kw), ref[fam], Mg))
    # the unit-input map, column by column
    sk, _, dopt, _ = DC.model("phantom")
    Mg = DC.total_mass(sk) * dopt.eom.gravity
    q, tau, lam, grf = DC.force_map_case()
    for f in range(len(tau)):
        ref = DC.gen_forces(sk, dopt, q, tau[f], lam[f], grf[f])
        for fam, kw in (("feet", dict(grf=grf[f])), ("motors", dict(tau=tau[f])), ("joints", dict(lam=lam[f]))):
            worst[fam] = max(worst[fam], DC.distance(oracle.dyn_forces(sk, dopt, q, **kw), ref[fam], Mg))
    # E and A of every force-fit case
    for key, c in DC.grf_cases().items():
        sk, P = DC.model(c["model"])[0], DC.case_problem(key)
        for n in range(P.F):
            E, A = oracle.grf_terms(sk, c["gopt"], c["q"][n], c["dq"][n], c["ddq"][n])
            worst["E"] = max(worst["E"], float(np.abs(E - P.E[n]).max() / max(1.0, np.abs(E).max())))
            worst["A"] = max(worst["A"], float(np.abs(A - P.A[n]).max() / max(1.0, np.abs(A).max())))
    print("\nreference vs oracle: " + "   ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert 0 < v < DC.REF_ORACLE, (k, v)                # (exactly 0 would mean that nothing was compared)


def test_rest_frame_is_gravity_alone():
    """q' = q'' = 0: rows 0-2 are (0, 0, M g) and the angle rows are the gravity torques dV/dq"""
    for name in DC.MODELS:
        sk, eopt, _, _ = DC.model(name)
        q, dq, ddq = DC.eom_cases(name)
        assert not dq[4].any() and not ddq[4].any()
        rows = DC.eom_rows(sk, eopt, q[4], dq[4], ddq[4])
        Mg = DC.total_mass(sk) * eopt.gravity
        assert np.abs(rows[:3] - [0, 0, Mg]).max() < 1e-13 * Mg
        assert np.abs(rows - DC.gravity_torques(sk, eopt.gravity, q[4])).max() < 1e-13 * Mg and np.abs(rows[3:]).max() > 1e-3 * Mg


def test_inputs_are_where_the_kernels_can_go_wrong():
    for name in DC.MODELS:
        sk, eopt, _, _ = DC.model(name)
        q, dq, ddq = DC.eom_cases(name)
        assert abs(q[3, 3 + 3 * DC.LEG_LINK + 1] - np.pi / 2) < 1e-3
        # the velocity terms dominate on frames 0-3: the gyroscopic term alone is far above the tolerance, and the rows are above M g
        Mg = DC.total_mass(sk) * eopt.gravity
        for n in range(4):
            gyro = DC.rotational_rows_closed_form(sk, eopt, q[n], dq[n], ddq[n]) - DC.rotational_rows_closed_form(sk, eopt, q[n], dq[n], ddq[n], True)
            assert np.abs(gyro).max() > 1e-3 * Mg and np.abs(DC.eom_rows(sk, eopt, q[n], dq[n], ddq[n])).max() > Mg
    cases = DC.grf_cases()
    assert sorted(c["q"].shape[0] for k, c in cases.items() if k.startswith("frames-")) == [1, 2, 4, 5, 6, 7]
    assert sorted(c["gopt"].n_feet for k, c in cases.items() if k.startswith("feet-")) == [1, 2, 3, 4]
    pat = cases["patterns"]["contact"]
    assert len({tuple(r) for r in pat.tolist()}) == 16
    packs = cases["flight-packs"]["contact"]
    assert packs[1].all() and not packs[[0, 2, 3, 4, 5]].any()
    assert pat[:3].any(1).tolist() == [False, True, True]                         # a pack of three whose frames disagree about contact


def test_projection_is_exact_idempotent_and_feasible():
    rng = np.random.default_rng(5)
    for mu, fmax in ((1.3, 5.0), (1.3, 0.3), (0.0, 5.0), (0.4, 1.0)):
        t = rng.normal(0, 2, (400, 5)).astype(LD)
        t[:50, 0] = rng.uniform(0, fmax, 50); t[:50, 1:] = LD(mu) * t[:50, :1] * rng.uniform(0, 0.25, (50, 4))    # feasible already
        t[50:60, 1:] = 0
        y = DC.project(t, mu, fmax)
        assert (y >= 0).all() and (y <= fmax).all() and (y[:, 1:].sum(1) <= LD(mu) * y[:, 0] + LD(1e-18)).all()
        assert np.abs(DC.project(y, mu, fmax) - y).max() <= 1e-18
        inside = (t >= 0).all(1) & (t <= fmax).all(1) & (t[:, 1:].sum(1) <= LD(mu) * t[:, 0])
        assert inside.any() and np.array_equal(y[inside], t[inside])
        # nearest point: no feasible point of a random cloud around y is closer to t
        for _ in range(20):
            z = DC.project(y + rng.normal(0, 0.05, y.shape).astype(LD), mu, fmax)
            assert (((z - t) ** 2).sum(1) >= ((y - t) ** 2).sum(1) - LD(1e-17)).all()
        # float64 agrees with the extended evaluation
        assert np.abs(DC.project(t.astype(np.float64), mu, fmax) - y).max() < 1e-14


@pytest.mark.parametrize("key", DC.BINDING_CASES + ("acinoset-2000", "patterns", "feet-1", "feet-3"))
def test_certificate_accepts_the_minimiser_and_rejects_its_neighbours(key):
    P, y = DC.case_problem(key), DC.case_minimiser(key)
    cert = P.kkt_residual(y)
    assert (cert <= DC.CERT).all() and P.feasible(y, 1e-17)
    frames = np.flatnonzero(P.contact.any(1))
    assert len(frames)
    for f in frames:
        foot = int(np.flatnonzero(P.contact[f])[0])
        for comp, shift in ((0, 1e-9), (0, -1e-9), (1, 1e-9)):
            if key == "no-friction" and comp:
                continue                                                        # Proj returns every xy to 0 there: only z can be off
            y2 = y.copy(); y2[f, foot, comp] += LD(shift)
            if comp == 0 and not (1e-6 < y[f, foot, 0] < P.fmax - 1e-6):
                continue                                                        # on a bound the shifted point projects back
            assert P.kkt_residual(y2)[f] > 1e-11, (key, f, comp, shift)
    # no feasible neighbour has a lower objective
    rng = np.random.default_rng(3)
    f0 = P.objective(y)
    for _ in range(20):
        z = P._proj((y + rng.normal(0, 1e-3, y.shape).astype(LD)).reshape(P.F, -1))
        assert (P.objective(z) >= f0 - LD(1e-18)).all()
    # the first iterate in closed form is the first iterate
    assert np.array_equal(P.one_step(), P.fista(1))


def test_binding_cases_bind():
    for key in DC.BINDING_CASES:
        share = DC.binding_share(key)
        print(f"\n{key}: constraint active in {share:.2f} of the contact frames")
        assert share >= 1 / 3, (key, share)


def test_comparison_notices_planted_errors(oracle):
    """a copy of the reference's own formulas with one error each, measured by the same distance() at the GPU tolerance"""
    sk, eopt, dopt, _ = DC.model("phantom")
    Mg = DC.total_mass(sk) * eopt.gravity
    q, dq, ddq = DC.eom_cases("phantom")
    # w x I w dropped: the closed form of the rotational rows equals the autograd rows of the rotational energy, and stops doing so without it
    for n in (0, 5):                                                            # a high-rate frame and a gallop frame
        rot = DC.rotational_rows_autograd(sk, eopt, q[n], dq[n], ddq[n])
        rows = DC.eom_rows(sk, eopt, q[n], dq[n], ddq[n])
        good = rows - rot + DC.rotational_rows_closed_form(sk, eopt, q[n], dq[n], ddq[n])
        bad = rows - rot + DC.rotational_rows_closed_form(sk, eopt, q[n], dq[n], ddq[n], drop_gyroscopic=True)
        assert DC.distance(good, rows, Mg) < DC.REF_ORACLE and DC.distance(bad, rows, Mg) > 100 * DC.TOL_ROWS
    # one D_k sign flipped: caught by the unit-input map, in the columns of that component only
    qm, tau, lam, grf = DC.force_map_case()
    D = DC.DK.copy(); D[3] = -D[3]
    hit = []
    for f in range(len(grf)):
        ref = DC.gen_forces(sk, dopt, qm, grf=grf[f])["feet"]
        if DC.distance(DC.gen_forces(sk, dopt, qm, grf=grf[f], D=D)["feet"], ref, Mg) > 100 * DC.TOL_ROWS:
            hit.append(f)
    assert hit == [22 + 26 + 5 * ft + 3 for ft in range(4)]
    # one constraint row shifted by one: row 8 built from the joint of row 9
    defs = DC.constraint_defs(sk)
    bad = list(defs); bad[8] = defs[9]
    hit = []
    for f in range(22, 48):
        ref = DC.gen_forces(sk, dopt, qm, lam=lam[f])["joints"]
        if DC.distance(DC.gen_forces(sk, dopt, qm, lam=lam[f], defs=bad)["joints"], ref, Mg) > 100 * DC.TOL_ROWS:
            hit.append(f - 22)
    assert hit == [8]
    # ... which a virtual-work scalar with lambda = const would not see, but every single entry does; the oracle agrees with the unshifted rows
    assert DC.distance(oracle.dyn_forces(sk, dopt, qm, lam=lam[30]), DC.gen_forces(sk, dopt, qm, lam=lam[30])["joints"], Mg) < DC.REF_ORACLE


def test_fista_float64_distance():
    """what fixes the GPU tolerance of the force fit: 32 x the distance between the float64 and the np.longdouble evaluation of the reference's own
    FISTA on the inputs of the GPU tests, or the project's 1e-8, whichever is larger.  Measured: forces 1.28e-13, residual 2.20e-15."""
    worst = dict(force=0.0, residual=0.0)
    for key in DC.grf_cases():
        P = DC.case_problem(key)
        a, b = DC.case_fista(key), DC.case_fista(key, True)
        worst["force"] = max(worst["force"], float(np.abs(a - b).max()))
        worst["residual"] = max(worst["residual"], float(np.abs(P.residual(a, np.float64) - P.residual(b)).max()))
    print(f"\nFISTA float64 vs longdouble: forces {worst['force']:.2e}, residual {worst['residual']:.2e}")
    for k, v in worst.items():
        assert v <= 2 * DC.FISTA_F64_LD[k], (k, v)
        assert DC.TOL_FIT == max(1e-8, 32 * DC.FISTA_F64_LD[k])


def test_truncation_distance_is_the_recorded_one():
    """Deviation: 2 000 FISTA iterations do not reach the minimum-norm minimiser.  L / eps is about 2e7, so the net wrench and
    the objective converge while the split of the force over the null space of A (14 dimensions with four feet down) is still moving.  Distance
    from fista(2000, longdouble) to the certified minimiser on the committed stance frames (16 phantom and 6 acinoset gallop frames, contacts drawn
    with p = 0.6), measured: forces 1.35e-2 body weights, residual 1.52e-6, objective 7.96e-10.  Each is held to twice its recorded value: the margin
    stands for another contact draw, not for arithmetic.  Each must also reach half its recorded value, so that DESIGN.md and cpe.h cannot go on
    quoting figures that no longer hold: a change that improves the iteration re-records DC.TRUNCATION and those two texts."""
    worst = dict(force=0.0, residual=0.0, objective=0.0)
    for key in DC.TRUNCATION_CASES:
        P, y, ym = DC.case_problem(key), DC.case_fista(key, True), DC.case_minimiser(key)
        assert int(DC.grf_cases()[key]["gopt"].iterations) == 2000 and (P.kkt_residual(ym) <= DC.CERT).all()
        worst["force"] = max(worst["force"], float(np.abs(y - ym).max()))
        worst["residual"] = max(worst["residual"], float(np.abs(P.residual(y) - P.residual(ym)).max()))
        gap = P.objective(y) - P.objective(ym)
        assert (gap >= -LD(1e-18)).all()                                        # the minimiser is the minimiser
        worst["objective"] = max(worst["objective"], float(gap.max()))
    print("\ntruncation after 2 000 iterations: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 2 * DC.TRUNCATION[k], (k, v)
        assert v >= DC.TRUNCATION[k] / 2, (k, v)                                 # and the record is not stale
