"""The launch window of every solve on the GPU (lm_drive and k_build_act, DESIGN.md "The launch window"): the active list against numpy, and
solves of more sequences than the window has slots against the same sequences solved in small chunks, bit for bit (the batching contract of
DESIGN.md 7 held past the window), in every form that goes through lm_drive.

The launch model the driver tests hold (tests/window_compare.py): k_build_act lists a sequence that ends OK or at the iteration limit in
exactly `iterations + outer` launches (listed_launches: read from k_lm_step -- one launch per judged trial, the last of which also writes the
final status, and one launch per multiplier update that re-evaluates and makes a trial without judging one), and lm_drive leaves
launches_after(r) launches after the first pass when the last sequence ends in windowed iteration r.  need = iterations + 2 * outer + 1, the
shape of lm_drive's per_seq, bounds that count from above by outer + 1; for a sequence solved alone
    K_solo - 3 POLL <= need <= K_solo                       (while outer <= 4)
and for a batch K <= greedy_rounds(need, window) + 3 POLL, where a driver that hands no slot over takes lockstep_rounds(need, window)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import test_gpu_ragged as RG
import test_gpu_ragged_kinetic as RK
import track_compare as TC
import window_compare as WC
from cheetah_pose_estimation_amd import _lib, abi, priors, synth
from test_gpu_track_weighted import _synthetic_cov
from test_gpu_tracked import _model as _tracked_model
from test_shutter import TRUE as SHUTTER_TRUE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POLL = WC.POLL


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_same(out, ref, fields, stats, kstats=()):
    """every sequence of `out` bit-equal to the same sequence of `ref`: arrays of `fields`, then the cpe_stats / cpe_kinetic_stats members"""
    B = len(ref["stats"])
    assert len(out["stats"]) == B
    for k in fields:
        assert out[k].shape == ref[k].shape, k
        if out[k].tobytes() != ref[k].tobytes():
            bad = [b for b in range(B) if out[k][b].tobytes() != ref[k][b].tobytes()]
            raise AssertionError((k, len(bad), bad[:8], float(np.abs(out[k][bad[0]] - ref[k][bad[0]]).max())))
    for key, names in (("stats", stats), ("kstats", kstats)):
        for f in names:
            a, r = [getattr(s, f) for s in out[key]], [getattr(s, f) for s in ref[key]]
            bad = [b for b in range(B) if a[b] != r[b]]
            assert not bad, (key, f, len(bad), [(b, a[b], r[b]) for b in bad[:8]])


# ---- 3. k_build_act against numpy ------------------------------------------------------------------------------------------------------
def test_active_list_matches_numpy(sk24, cams6, gpu_handle_factory):
    """every (B, window, pattern) of window_compare.active_list_cases / patterns through cpe_eval_active_list: the list length, the list, and
    -1 in every entry behind it up to window + 64"""
    h = gpu_handle_factory(sk24, cams6)
    t0, n = time.perf_counter(), 0
    for B, window in WC.active_list_cases():
        for name, status in WC.patterns(B, window, seed=11).items():
            want, n_want = WC.active_list(status, window)
            act, n_act = h.eval_active_list(status, window)
            assert act.shape == (window + WC.ACT_GUARD,) and act.dtype == np.int32
            assert n_act == n_want == min(int((status == 0).sum()), window), (B, window, name, n_act, n_want)
            assert np.array_equal(act[:n_act], want), (B, window, name)
            assert (act[n_act:] == -1).all(), (B, window, name, np.flatnonzero(act[n_act:] != -1)[:8] + n_act)
            n += 1
    print(f"k_build_act: {n} cases in {time.perf_counter() - t0:.2f} s")
    assert n >= 300


def test_active_list_refusals(sk24, cams6, gpu_handle_factory):
    h = gpu_handle_factory(sk24, cams6)
    with pytest.raises(_lib.CpeError, match="window"):
        h.eval_active_list(np.zeros(4, np.int32), 0)
    with pytest.raises(_lib.CpeError, match="B = 0"):
        h.eval_active_list(np.zeros(0, np.int32), 4)
    lib, st = h.lib, (C.c_int32 * 4)()
    for args, name in (((4, 2, None, st, st), b"status"), ((4, 2, st, None, st), b"act"), ((4, 2, st, st, None), b"n_act")):
        assert lib.cpe_eval_active_list(h._h, *args) == abi.BAD_ARG and name + b" is null" in lib.cpe_last_error()
    # a solve on the same handle afterwards is untouched by the entry's scratch arrays
    d = synth.make_batch(sk24, cams6, B=2, N=6, seed=3)
    a = h.solve_host(d["q_init"], d["meas"], d["weight"])
    h.eval_active_list(np.zeros(700, np.int32), 512)
    b = h.solve_host(d["q_init"], d["meas"], d["weight"])
    assert a["q"].tobytes() == b["q"].tobytes() and [s.iterations for s in a["stats"]] == [s.iterations for s in b["stats"]]


# ---- 4 a, b. the plain kinematic solve at PB = 3 -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(sk25, cams6, n_cu):
    """two windows + 5 sequences of N = 9 (synth.make_batch, seed 7000): the chunked reference, and the whole batch in one solve with the launch
    profile on"""
    window = 2 * n_cu
    B = 2 * window + 5
    d = synth.make_batch(sk25, cams6, B=B, N=9, seed=7000)
    arrays = (d["q_init"], d["meas"], d["weight"])
    t0 = time.perf_counter()
    href = _lib.Handle(sk25, cams6, abi.default_options())
    try:
        ref = WC.chunked(href.solve_host, arrays, 128)
    finally:
        href.close()
    t1 = time.perf_counter()
    h = _lib.Handle(sk25, cams6, abi.default_options())
    try:
        assert h.pb == 3
        h.profile(True)
        out = h.solve_host(*arrays)
        K = h.profile_totals()["k_build_act"][1]
    finally:
        h.close()
    print(f"plain solve past the window: B = {B}, window = {window}; chunked reference {t1 - t0:.2f} s, one solve {time.perf_counter() - t1:.2f} s, "
          f"K = {K}")
    return dict(d=d, arrays=arrays, window=window, B=B, ref=ref, out=out, K=K)


def test_plain_solve_past_the_window(plain, oracle, sk25, cams6):
    ref, out, window = plain["ref"], plain["out"], plain["window"]
    its = np.array([s.iterations for s in ref["stats"]])
    outer = np.array([s.outer for s in ref["stats"]])
    print(f"reference: {len(set(its.tolist()))} distinct iteration counts {its.min()} .. {its.max()}, {int((outer > 0).sum())} sequences with a "
          f"multiplier update, {int((outer[window:] > 0).sum())} of them past the window")
    assert len(set(its.tolist())) >= 10                                       # the slots are handed over at many different times
    assert (outer[window:] > 0).any()                                         # a multiplier pass runs in a handed-over slot
    assert all(s.status == abi.OK for s in ref["stats"])
    _assert_same(out, ref, RG.FIELDS, RG.STATS)
    # against the oracle past the window, at the bars of test_kinetic_dataset_configuration_matches_oracle
    d, opts = plain["d"], abi.default_options()
    picks = WC.oracle_picks(oracle, sk25, cams6, opts, d, window)
    assert len(picks) == 8
    for b, r in picks:
        st, rs = out["stats"][b], r["stats"]
        rmse = float(np.sqrt(((out["positions"][b] - r["positions"]) ** 2).sum(-1).mean()))
        print(f"sequence {b}: HIP {st.iterations} iterations, {st.outer} updates, oracle {rs.iterations}, {rs.outer}; cost {st.cost:.9g} / {rs.cost:.9g}; "
              f"markers {rmse:.2e} m")
        assert st.status == rs.status and st.outer == rs.outer and abs(st.iterations - rs.iterations) <= 2, b
        assert abs(st.cost - rs.cost) < 1e-6 * abs(rs.cost) and rmse < 1e-5, b


def test_slots_are_handed_over(plain, sk25, cams6):
    """counts only: the launches of k_build_act of the big solve stay within the greedy schedule of the launch model, which a driver that waits
    for a whole window cannot meet on this batch; the model itself is first held against four sequences solved alone"""
    ref, window, K = plain["ref"], plain["window"], plain["K"]
    need, listed = WC.need(ref["stats"]), WC.listed_launches(ref["stats"])
    outer = np.array([s.outer for s in ref["stats"]])
    past = np.arange(window, plain["B"])
    solo = [int(past[np.argmax(outer[past] > 0)]), int(past[np.argmax(outer[past] == 0)]), int(past[np.argmax(need[past])]),
            int(past[np.argmin(need[past])])]
    h = _lib.Handle(sk25, cams6, abi.default_options())
    try:
        for b in solo:
            h.profile(True)
            one = h.solve_host(*[a[b:b + 1] for a in plain["arrays"]])
            K_solo = h.profile_totals()["k_build_act"][1]
            s = one["stats"][0]
            print(f"sequence {b} alone: {s.iterations} iterations, {s.outer} updates, need {need[b]}, listed {listed[b]}, K_solo {K_solo}")
            assert (s.iterations, s.outer) == (ref["stats"][b].iterations, ref["stats"][b].outer)
            assert K_solo - 3 * POLL <= need[b] <= K_solo, (b, K_solo, need[b])
            assert K_solo == WC.launches_after(listed[b]), (b, K_solo, listed[b])
    finally:
        h.close()
    greedy, lockstep = WC.greedy_rounds(need, window), WC.lockstep_rounds(need, window)
    exact = WC.greedy_rounds(listed, window)
    print(f"K = {K}; greedy_rounds(need) = {greedy}, lockstep_rounds(need) = {lockstep}; greedy_rounds(listed) = {exact} -> {WC.launches_after(exact)}")
    assert lockstep >= greedy + 6 * POLL                                      # the batch tells the two drivers apart
    assert K <= greedy + 3 * POLL
    assert K == WC.launches_after(exact)                                      # and every launch is kept full: the schedule is the greedy one exactly


# ---- 4 c. the driver's exit ----------------------------------------------------------------------------------------------------------------
def test_every_sequence_runs_to_max_iter(plain, sk25, cams6):
    """max_iter = 3 with both tolerances 0 (no step is small enough to stop on): three windows' worth of sequences all end MAX_ITER after exactly
    3 iterations -- none is left behind when the list runs empty, none gets a fourth"""
    opts = abi.default_options()
    opts.max_iter, opts.tol_step, opts.tol_cost = 3, 0.0, 0.0
    assert opts.max_outer == abi.default_options().max_outer == 8
    t0 = time.perf_counter()
    ref = out = None
    for big in (False, True):
        h = _lib.Handle(sk25, cams6, opts)
        try:
            if big:
                h.profile(True)
                out = h.solve_host(*plain["arrays"])
                K = h.profile_totals()["k_build_act"][1]
            else:
                ref = WC.chunked(h.solve_host, plain["arrays"], 128)
        finally:
            h.close()
    assert all(s.status == abi.MAX_ITER and s.iterations == 3 for s in ref["stats"])
    _assert_same(out, ref, RG.FIELDS, RG.STATS)
    assert all(s.status == abi.MAX_ITER and s.iterations == 3 for s in out["stats"]) and len(out["stats"]) == plain["B"] >= 2 * plain["window"] + 1
    rounds = WC.greedy_rounds(WC.listed_launches(ref["stats"]), plain["window"])
    print(f"max_iter = 3: K = {K}, {rounds} windowed iterations; {time.perf_counter() - t0:.2f} s")
    assert K == WC.launches_after(rounds)


# ---- 4 d. motion-prior windows: one slot per CU, and at W = 6 the spill area behind Lbuf -------------------------------------------------
@pytest.mark.parametrize("W", [4, 6])
def test_priors_solve_past_the_window(W, sk24, cams6, n_cu):
    pr = priors.load_priors() if W == 4 else priors.load_priors(path=os.path.join(GOLDEN, "priors_k5_w6_lasso.npz"))
    assert pr.lr_window == W
    cam1 = (abi.Camera * 1)(cams6[2])
    B, N = n_cu + 13, 2 * W + 3
    d = synth.make_batch(sk24, cam1, B=B, N=N, seed=7100 + W)
    arrays = (d["q_init"], d["meas"], d["weight"])
    t0 = time.perf_counter()
    ref = out = None
    for big in (False, True):
        h = _lib.Handle(sk24, cam1, abi.default_options(), pr)
        try:
            assert h.pb == W
            if big:
                out = h.solve_host(*arrays)
            else:
                ref = WC.chunked(h.solve_host, arrays, 128)
        finally:
            h.close()
    its = np.array([s.iterations for s in ref["stats"]])
    print(f"window-{W} priors past {n_cu} slots: B = {B}, N = {N}, iterations {its.min()} .. {its.max()} ({its[n_cu:].tolist()} past the window); "
          f"{time.perf_counter() - t0:.2f} s")
    assert (its[n_cu:] > 1).any()
    _assert_same(out, ref, RG.FIELDS, RG.STATS)


# ---- 4 e. the kinematic ragged form ------------------------------------------------------------------------------------------------------------
def test_ragged_solve_past_the_window(n_cu):
    models = RG._models()
    per = (2 * (2 * n_cu)) // 8 + 3                                           # 8 groups: two windows (rounded down to whole groups) + 24 sequences
    lens = (7, 9, 12, 10)
    groups = [(g % 4, lens[(g + g // 4) % 4]) for g in range(8)]
    assert len(set(groups)) == 8
    t0 = time.perf_counter()
    seqs, refs = [], []
    for g, (m, N) in enumerate(groups):
        sk, cams, opts, kin = models[m]
        d = synth.make_batch(sk, cams, B=per, N=N, fps=1.0 / opts.h, seed=7200 + 17 * g, kinetic_dataset=kin)
        h = _lib.Handle(sk, cams, opts)
        try:
            refs.append(WC.chunked(h.solve_host, (d["q_init"], d["meas"], d["weight"]), 128))
        finally:
            h.close()
        seqs += [(m, d["q_init"][b], d["meas"][b], d["weight"][b], g, b) for b in range(per)]
    assert len(seqs) == (2 * (2 * n_cu)) // 8 * 8 + 24 > 2 * (2 * n_cu)
    perm = np.random.default_rng(7).permutation(len(seqs))                    # interleave the groups
    seqs = [seqs[i] for i in perm]
    t1 = time.perf_counter()
    out = RG._ragged(models, seqs)
    print(f"ragged past the window: {len(seqs)} sequences; references {t1 - t0:.2f} s, one ragged solve {time.perf_counter() - t1:.2f} s")
    for i, (m, _, _, _, g, b) in enumerate(seqs):
        ref = refs[g]
        for k in RG.FIELDS:
            assert out[k][i].shape == ref[k][b].shape and out[k][i].tobytes() == ref[k][b].tobytes(), (i, g, b, k)
        for f in RG.STATS:
            assert getattr(out["stats"][i], f) == getattr(ref["stats"][b], f), (i, g, b, f)
    RG._assert_padding_zero(out, [s[:4] for s in seqs], models)
    assert sum(s.iterations > 1 for s in out["stats"][2 * n_cu:]) > len(seqs) // 4


# ---- 4 f. the physics-based forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["kinetic", "tracked", "tracked_weighted"])
def test_kinetic_solve_past_the_window(form, n_cu):
    md = RK._models(max_iter=30)[0] if form == "kinetic" else _tracked_model("phantom", 120.0, max_iter=30)
    assert md["opts"].max_iter == 30 and len(md["cams"]) == 6
    B, N, ko = 2 * n_cu + 9, 7, md["ko"]
    d = synth.make_gallop_batch(md["sk"], md["cams"], B=B, N=N, fps=120.0, seed=7300, stance_frames=3)
    qi, qt, me, we, stn = d["q_init"], d["q_true"], d["meas"], d["weight"], d["stance"]
    if form == "kinetic":
        arrays = (qi, me, we, stn)
        solve = lambda h: (lambda qi, me, we, stn: h.solve_kinetic_host(ko, qi, me, we, stn))
    elif form == "tracked":
        arrays = (qi, qt, me, we, stn)
        solve = lambda h: (lambda qi, qt, me, we, stn: h.solve_kinetic_tracked_host(ko, qi, qt, stn, me, we))
    else:
        Wt = TC.precision(md["sk"], _synthetic_cov(np.random.default_rng(41), (B, N)), 1.0)
        arrays = (np.ascontiguousarray(0.5 * (Wt + np.swapaxes(Wt, -1, -2))), qi, qt, me, we, stn)
        solve = lambda h: (lambda Wt, qi, qt, me, we, stn: h.solve_kinetic_tracked_weighted_host(ko, Wt, qi, qt, stn, me, we))
    t0 = time.perf_counter()
    ref = out = None
    for big in (False, True):
        h = _lib.Handle(md["sk"], md["cams"], md["opts"])
        try:
            if big:
                out = solve(h)(*arrays)
            else:
                ref = WC.chunked(solve(h), arrays, 64)
        finally:
            h.close()
    its = np.array([s.iterations for s in ref["stats"]])
    print(f"{form} past the window: B = {B}, iterations {its.min()} .. {its.max()}, {len(set(its.tolist()))} distinct; {time.perf_counter() - t0:.2f} s")
    assert (its[2 * n_cu:] > 1).any() and its.sum() > 5 * B                   # real solves, also in the handed-over slots
    _assert_same(out, ref, RK.FIELDS, RK.STATS, RK.KSTATS)


# ---- 4 g. shutter-delay rounds: restarts of more sequences than one block of k_reset_status, more than one window ------------------------------
def test_shutter_solve_past_the_window(sk25, n_cu):
    cams = synth.make_cameras(6, track=5.0)
    opts = abi.default_options()
    P, N, rounds = 8, 12, 3
    d = synth.make_batch(sk25, cams, P, N=N, seed=77, noise_px=1.0, outlier_frac=0.05, shutter_delay=SHUTTER_TRUE)
    rep = (2 * n_cu) // 8 + 2
    B = P * rep
    assert B > 2 * n_cu and B > 256
    t0 = time.perf_counter()
    h = _lib.Handle(sk25, cams, opts)
    try:
        ref = h.solve_shutter_host(d["q_init"], d["meas"], d["weight"], opts.h, rounds, 1e-5)
        out = h.solve_shutter_host(*[np.tile(d[k], (rep,) + (1,) * (d[k].ndim - 1)) for k in ("q_init", "meas", "weight")], opts.h, rounds, 1e-5)
    finally:
        h.close()
    print(f"shutter past the window: B = {B}, rounds {ref['rounds']} / {out['rounds']}, iterations {[s.iterations for s in ref['stats']]}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert ref["rounds"] >= 1 and np.abs(ref["tau"][:, 1:]).min() > 0.0       # the delays moved: the later rounds are restarts
    assert out["rounds"] == ref["rounds"]
    for k in range(B):
        for f in ("q", "tau", "positions"):
            assert out[f][k].tobytes() == ref[f][k % P].tobytes(), (k, f, float(np.abs(out[f][k] - ref[f][k % P]).max()))
        assert out["stats"][k].iterations == ref["stats"][k % P].iterations, k
