"""Reference side of the launch-window tests (k_build_act and lm_drive in cpe_api.hip; cpe_eval_active_list, include/cpe.h).  Helper, not a
test module, and nothing here needs a GPU.

  active_list      what k_build_act must write: the first `window` running sequences in index order, and how many
  greedy_rounds    launches of a driver that refills the window before every iteration (lm_drive's contract)
  lockstep_rounds  launches of a driver that hands no slot over: every window of sequences runs until its slowest member ends
  need, listed_launches   the launch models of one sequence: how often k_build_act lists it, from above and exactly
  launches_after   lm_drive's launches of k_build_act when the last sequence ends in a given windowed iteration
  chunked          a host-form solve over a batch in index chunks, outputs and statistics concatenated: the reference of every
                   past-the-window comparison, each chunk far below the window
  patterns         the status words of the k_build_act cases, from a seed
  oracle_picks     the sequences of a batch past the window that the oracle solves quickly, for the parity check there"""
import numpy as np

POLL = 4                      # lm_drive queues this many iterations between two reads of the list length
ACT_GUARD = 64                # entries of cpe_eval_active_list's act past `window`
ACT_B = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 2051)
ACT_WINDOWS = (1, 2, 63, 64, 65, 255, 256, 257, 512)          # and B, B + 5 of every case (active_list_cases)
BORDERS = (63, 64, 255, 256, 511, 512)                        # last lane of a wave / first of the next, last thread of a chunk / first of the next
FINISHED = (1, 2, -1, 7)                                      # any word but 0 is "not running"


def active_list(status, window):
    """(indices of the first `window` sequences with status 0 in ascending order, their number)"""
    act = np.flatnonzero(np.asarray(status) == 0)[:window]
    return act.astype(np.int32), int(act.shape[0])


def greedy_rounds(need, window):
    """Rounds until no sequence has work left when, every round, the first `window` sequences (by index) that still have work do one unit of
    it: need[b] = units of sequence b.  Simulated round by round."""
    left = np.array(need, dtype=np.int64)
    assert left.ndim == 1 and (left >= 0).all() and window >= 1
    rounds = 0
    while True:
        run = np.flatnonzero(left > 0)[:window]
        if run.size == 0:
            return rounds
        left[run] -= 1
        rounds += 1


def lockstep_rounds(need, window):
    """The same work without hand-over: consecutive index windows one after the other, each for as long as its slowest sequence"""
    need = np.asarray(need, dtype=np.int64)
    assert need.ndim == 1 and (need >= 0).all() and window >= 1
    return int(sum(int(need[i:i + window].max()) for i in range(0, need.shape[0], window)))


def need(stats):
    """The launch model of the driver tests, from a sequence's final cpe_stats: iterations + 2 * outer + 1 windowed iterations, the shape of
    lm_drive's per_seq.  It is an upper bound of listed_launches, by outer + 1."""
    return np.array([s.iterations + 2 * s.outer + 1 for s in stats], dtype=np.int64)


def listed_launches(stats):
    """How often k_build_act lists a sequence that ends OK or at the iteration limit, read from k_lm_step: iterations + outer.  The first pass
    (all B sequences, before the list exists) evaluates and makes the first trial.  After it, every launch that lists the sequence either judges
    a trial (iterations + 1; the launch that judges the last one also writes the final status) or, one launch after a converged inner loop
    met a violated bound and armed the update (outer + 1, al_pending), re-evaluates the current iterate with the new multipliers and makes a
    trial without judging one."""
    return np.array([s.iterations + s.outer for s in stats], dtype=np.int64)


def launches_after(rounds):
    """k_build_act launches of lm_drive when the last sequence ends in windowed iteration `rounds` (>= 0; 0 = all ended in the first pass):
    launch rounds + 1 is the first to build an empty list; the snapshot of the list length is taken after every POLL launches, so batch
    j = ceil((rounds + 1) / POLL) is the first whose snapshot is 0, and the host reads it after it has queued batch j + 1."""
    return POLL * (-(-(rounds + 1) // POLL) + 1)


def chunked(solve, arrays, chunk):
    """solve(*[a[i:i + chunk] for a in arrays]) over the batch in index order, concatenated: numpy outputs along the sequence axis, `stats` /
    `kstats` lists appended; an output that is None in every chunk stays None.  `status` (one word per call) is dropped."""
    B = len(arrays[0])
    assert chunk >= 1 and all(len(a) == B for a in arrays)
    parts = [solve(*[a[i:i + chunk] for a in arrays]) for i in range(0, B, chunk)]
    out = {}
    for k in parts[0]:
        vals = [p[k] for p in parts]
        if k in ("status", "rounds"):
            continue
        if isinstance(vals[0], np.ndarray):
            out[k] = np.concatenate(vals, axis=0)
        elif vals[0] is None:
            assert all(v is None for v in vals), k
            out[k] = None
        else:
            out[k] = [s for v in vals for s in v]
    return out


def patterns(B, window, seed):
    """{name: status [B] int32} of the k_build_act cases for one (B, window); 0 = running.  Patterns that need an index the batch does not
    have are left out (the border pattern keeps the borders below B, and is left out when there is none)."""
    rng = np.random.default_rng([seed, B, window])
    done = lambda n: rng.choice(FINISHED, size=n).astype(np.int32)
    P = {"all running": np.zeros(B, np.int32), "none running": np.ones(B, np.int32)}
    first = np.ones(B, np.int32); first[0] = 0
    last = np.ones(B, np.int32); last[B - 1] = 0
    alt = np.ones(B, np.int32); alt[::2] = 0
    P.update({"only the first": first, "only the last": last, "alternating": alt})
    for dens in (0.05, 0.5, 0.95):
        P[f"random {dens}"] = (rng.random(B) >= dens).astype(np.int32)
    mixed = done(B); mixed[rng.random(B) < 0.4] = 0
    P["mixed finished words"] = mixed
    # exactly `window` running sequences inside the first 256-thread chunk and more behind it: the kernel leaves its loop after that chunk
    if window < 256 and B > 256:
        brk = done(B)
        brk[np.sort(rng.choice(256, size=window, replace=False))] = 0
        brk[256 + rng.choice(B - 256, size=max(1, (B - 256) // 3), replace=False)] = 0
        P["break after the first chunk"] = brk
    at = [i for i in BORDERS if i < B]
    if at:
        bd = done(B); bd[at] = 0
        P["wave and chunk borders"] = bd
    return P


def active_list_cases():
    """[(B, window)]: every B of ACT_B with the windows of ACT_WINDOWS up to B + 5, and B, B + 5 themselves"""
    return [(B, w) for B in ACT_B for w in sorted(set(ACT_WINDOWS + (B, B + 5))) if w <= B + 5]


def oracle_picks(O, sk, cams, opts, d, window, count=8, limit=64, below=60, ok=0):
    """The first `count` sequences of the batch d (synth.make_batch's dict) at index >= window that oracle.solve ends with status `ok` in
    fewer than `below` iterations, looking at no more than `limit` candidates: [(index, the oracle's result)]"""
    picks = []
    for b in range(window, min(window + limit, d["q_init"].shape[0])):
        ref = O.solve(sk, cams, opts, None, d["q_init"][b], d["meas"][b], d["weight"][b])
        if ref["stats"].status == ok and ref["stats"].iterations < below:
            picks.append((b, ref))
            if len(picks) == count:
                break
    return picks
