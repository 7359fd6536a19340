"""The launch-window helpers (tests/window_compare.py) against plain loops and hand-worked cases, the new entry's place in the C ABI, and the
input conditions of tests/test_gpu_launch_window.py that the oracle alone decides.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import window_compare as WC
from cheetah_pose_estimation_amd import _lib, abi, synth
from test_covariance_host import _prototype

N_CU = 256                      # the MI355X's compute units: the window of the conditions below is the one the GPU tests meet there


def _loop_list(status, window):
    out = []
    for b, s in enumerate(status):
        if s == 0 and len(out) < window:
            out.append(b)
    return out


def test_active_list_matches_a_plain_loop_on_every_pattern():
    cases = WC.active_list_cases()
    assert len(cases) >= 90 and {B for B, _ in cases} == set(WC.ACT_B)
    assert all((B, B) in cases and (B, B + 5) in cases for B in WC.ACT_B) and max(w - B for B, w in cases) == 5
    seen, n = set(), 0
    for B, window in cases:
        for name, status in WC.patterns(B, window, seed=11).items():
            assert status.shape == (B,) and status.dtype == np.int32, (B, window, name)
            act, n_act = WC.active_list(status, window)
            want = _loop_list(status.tolist(), window)
            assert act.tolist() == want and n_act == len(want) == min(int((status == 0).sum()), window), (B, window, name)
            seen.add(name)
            n += 1
    assert seen == {"all running", "none running", "only the first", "only the last", "alternating", "random 0.05", "random 0.5", "random 0.95",
                    "mixed finished words", "break after the first chunk", "wave and chunk borders"}
    assert n >= 300


def test_patterns_are_what_their_names_say():
    P = WC.patterns(1000, 64, seed=11)
    assert (P["all running"] == 0).all() and (P["none running"] != 0).all()
    assert np.flatnonzero(P["only the first"] == 0).tolist() == [0] and np.flatnonzero(P["only the last"] == 0).tolist() == [999]
    assert np.flatnonzero(P["alternating"] == 0).tolist() == list(range(0, 1000, 2))
    for dens in (0.05, 0.5, 0.95):
        assert abs((P[f"random {dens}"] == 0).mean() - dens) < 0.06
    m = P["mixed finished words"]
    assert set(np.unique(m)) == {0, *WC.FINISHED} and 0.2 < (m == 0).mean() < 0.6
    brk = P["break after the first chunk"]
    assert int((brk[:256] == 0).sum()) == 64 and int((brk[256:] == 0).sum()) > 0            # exactly `window` in the first chunk, more behind
    assert np.flatnonzero(P["wave and chunk borders"] == 0).tolist() == list(WC.BORDERS)
    assert np.flatnonzero(WC.patterns(257, 2, seed=11)["wave and chunk borders"] == 0).tolist() == [63, 64, 255, 256]
    assert "wave and chunk borders" not in WC.patterns(63, 2, seed=11) and "break after the first chunk" not in WC.patterns(256, 2, seed=11)
    assert "break after the first chunk" not in WC.patterns(1000, 256, seed=11)
    # the same seed gives the same words, another seed others
    assert all(np.array_equal(a, b) for a, b in zip(P.values(), WC.patterns(1000, 64, seed=11).values()))
    assert not np.array_equal(P["random 0.5"], WC.patterns(1000, 64, seed=12)["random 0.5"])


def test_round_counts_on_hand_worked_cases():
    """Three sequences, need = (3, 1, 2), window = 2.
    greedy:   round 1 runs 0, 1 -> (2, 0, 2); round 2 runs 0, 2 -> (1, 0, 1); round 3 runs 0, 2 -> (0, 0, 0): 3 rounds.
    lockstep: window {0, 1} runs max(3, 1) = 3 rounds, then window {2} runs 2: 5 rounds."""
    assert WC.greedy_rounds([3, 1, 2], 2) == 3 and WC.lockstep_rounds([3, 1, 2], 2) == 5
    # window 1: one sequence at a time either way
    assert WC.greedy_rounds([3, 1, 2], 1) == 6 == WC.lockstep_rounds([3, 1, 2], 1)
    # (5, 1, 1, 1), window 2: greedy 5 (sequence 0 never leaves, the others pass through the second slot); lockstep 5 + 1
    assert WC.greedy_rounds([5, 1, 1, 1], 2) == 5 and WC.lockstep_rounds([5, 1, 1, 1], 2) == 6
    # a long sequence at the end cannot start early: (1, 1, 4), window 2 -> round 1: 0, 1; rounds 2..5: 2
    assert WC.greedy_rounds([1, 1, 4], 2) == 5 and WC.lockstep_rounds([1, 1, 4], 2) == 5
    assert WC.greedy_rounds([0, 0], 3) == 0 == WC.lockstep_rounds([0, 0], 3)
    rng = np.random.default_rng(5)
    for B, window in ((1, 1), (7, 7), (7, 12), (40, 64)):                              # window >= B: the slowest sequence
        need = rng.integers(0, 30, B)
        assert WC.greedy_rounds(need, window) == WC.lockstep_rounds(need, window) == need.max()
    for B, window, k in ((10, 3, 4), (9, 3, 2), (1029, 512, 7), (5, 1, 3)):             # all equal: whole windows, one after the other
        want = -(-B // window) * k
        assert WC.greedy_rounds([k] * B, window) == WC.lockstep_rounds([k] * B, window) == want
    for _ in range(20):                                                                 # never more rounds with hand-over, never fewer than the work
        B, window = int(rng.integers(1, 60)), int(rng.integers(1, 20))
        need = rng.integers(0, 25, B)
        g = WC.greedy_rounds(need, window)
        assert max(int(need.max()), -(-int(need.sum()) // window)) <= g <= WC.lockstep_rounds(need, window)


def test_launch_models():
    S = lambda it, outer: abi.Stats(iterations=it, outer=outer)
    stats = [S(8, 0), S(129, 2), S(3, 0)]
    assert WC.need(stats).tolist() == [9, 134, 4] and WC.listed_launches(stats).tolist() == [8, 131, 3]
    # the last sequence ends in windowed iteration r: launch r + 1 builds the empty list, the batch that holds it is read one batch later
    # (r = 3: launch 4, the last of batch 1, lists nothing, and batch 1's snapshot is read once batch 2 is queued; r = 4: launch 5 is in batch 2)
    assert [WC.launches_after(r) for r in (0, 1, 2, 3, 4, 7, 8)] == [8, 8, 8, 8, 12, 12, 16]
    for r in range(0, 50):
        assert r + 1 + WC.POLL <= WC.launches_after(r) <= r + 2 * WC.POLL and WC.launches_after(r) % WC.POLL == 0


def test_chunked_concatenates_in_index_order():
    calls = []

    def solve(a, b):
        calls.append(len(a))
        return dict(status=0, q=a * 2.0, none=None, stats=[int(x) for x in b], rounds=1)
    a, b = np.arange(10.0).reshape(5, 2), np.arange(5)
    out = WC.chunked(solve, (a, b), 2)
    assert calls == [2, 2, 1] and set(out) == {"q", "none", "stats"}
    assert np.array_equal(out["q"], a * 2.0) and out["none"] is None and out["stats"] == [0, 1, 2, 3, 4]
    assert WC.chunked(solve, (a, b), 128)["stats"] == [0, 1, 2, 3, 4] and calls[-1] == 5


def test_entry_is_declared_exported_and_wrapped():
    _lib.build_library()
    lib = _lib.load()
    kinds = ("h", "i", "i", "ip", "ip", "ip")
    assert _prototype("cpe_eval_active_list") == kinds == tuple(abi.ENTRIES["cpe_eval_active_list"])
    assert list(lib.cpe_eval_active_list.argtypes) == abi.argtypes("cpe_eval_active_list")
    assert callable(_lib.Handle.eval_active_list)
    # the refusals that need no device: a null handle is named before anything is touched
    st = (C.c_int32 * 4)()
    assert lib.cpe_eval_active_list(None, 4, 2, st, st, st) == abi.BAD_ARG and b"h is null" in lib.cpe_last_error()


def test_plain_solve_inputs_hold_for_the_oracle(oracle, sk25, cams6):
    """synth.make_batch(seed=7000), N = 9, B = 2 windows + 5 at PB = 3: within the first 64 sequences past the window the oracle ends 8 with OK
    in fewer than 60 iterations (the parity check of test_plain_solve_past_the_window uses exactly these), and among them are both a sequence
    with and one without a multiplier update"""
    window = 2 * N_CU
    B = 2 * window + 5
    d = synth.make_batch(sk25, cams6, B=B, N=9, seed=7000)
    picks = WC.oracle_picks(oracle, sk25, cams6, abi.default_options(), d, window)
    assert len(picks) == 8
    assert all(window <= b < window + 64 and r["stats"].status == abi.OK and r["stats"].iterations < 60 for b, r in picks)
    outers = {r["stats"].outer > 0 for _, r in picks}
    print("oracle picks:", [(b, r["stats"].iterations, r["stats"].outer) for b, r in picks])
    assert outers == {False, True}
