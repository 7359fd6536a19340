"""Developer tool (not part of the product or the tests): times ONE cpe_covariance_kinetic_ragged_host call over 15 mixed sequences next to the same
15 sequences through cpe_covariance_kinetic_host one by one (B = 1, a plain handle per model, created beforehand) on the same build.  The mix has
the shape of DESIGN.md section 7's: arabia-02 / shiraz-02 with the kinetic dataset's skeleton and options at 200 fps under 4 cameras, phantom, jules,
arabia-02 and shiraz-02 at 120 / 90 fps under 6 cameras -- six models -- and N = 30 .. 58.  Every output is asked for, ridge 1e-6, evaluated at the
generator's q_init (the cost of the call does not depend on where it is evaluated).  Both are timed warm, `--reps` times, host arrays in and out (the
staging is part of both).  Prints one JSON line: median and min / max of both in milliseconds, their ratio, the longest member alone, and the
statuses.  The numbers quoted in DESIGN.md section 7.

    python tools/time_kinetic_cov_ragged.py [--reps R]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

MODELS = (("arabia-02", 200.0, True, 4), ("shiraz-02", 200.0, True, 4), ("phantom", 120.0, False, 6), ("jules", 90.0, False, 6),
          ("arabia-02", 120.0, False, 6), ("shiraz-02", 120.0, False, 6))
LENGTHS = (30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58)


def main():
    from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    models = []
    for k, (animal, fps, kin, n_cams) in enumerate(MODELS):
        sk = skeleton.without_motion_model(skeleton.build_skeleton(animal, 24, kinetic_dataset=kin))
        ko = abi.default_kinetic_options(skeleton.dyn_options(animal), fps, kin)
        if kin:
            ko.slack_lo, ko.slack_hi = -2.0, 2.0
        models.append(dict(sk=sk, cams=synth.make_cameras(n_cams, seed=200 + k), opts=abi.default_options(fps), ko=ko, fps=fps, kin=kin))
    seqs = []
    for b, N in enumerate(LENGTHS):
        m = b % len(models)
        md = models[m]
        d = synth.make_gallop_batch(md["sk"], md["cams"], B=1, N=N, fps=md["fps"], seed=60 + b, kinetic_dataset=md["kin"], stance_frames=6)
        seqs.append(dict(m=m, q=d["q_init"][0], meas=d["meas"][0], weight=d["weight"][0], stance=d["stance"][0]))
    ridge = 1e-6

    def timed(fn, reps):
        fn()                                               # warm-up (workspace allocation, code objects)
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            out.append(1e3 * (time.perf_counter() - t0))
        return sorted(out)

    h = _lib.Handle.multi([md["sk"] for md in models], [md["cams"] for md in models], [md["opts"] for md in models])
    lists = lambda k: [s[k] for s in seqs]
    status = {}

    def ragged():
        r = h.covariance_kinetic_ragged_host(lists("q"), lists("meas"), lists("weight"), lists("stance"), [md["ko"] for md in models], lists("m"), ridge,
                                             want_L=True)
        status["ragged"] = r["seq_status"]
    ragged_ms = timed(ragged, args.reps)
    h.close()

    plain = [_lib.Handle(md["sk"], md["cams"], md["opts"]) for md in models]

    def one(s):
        r = plain[s["m"]].covariance_kinetic_host(s["q"][None], s["meas"][None], s["weight"][None], s["stance"][None], models[s["m"]]["ko"], ridge, want_L=True)
        return r["seq_status"][0]

    def one_by_one():
        status["one_by_one"] = [one(s) for s in seqs]
    serial_ms = timed(one_by_one, args.reps)
    longest_ms = timed(lambda: one(seqs[-1]), args.reps)
    for p in plain:
        p.close()
    med = statistics.median
    row = lambda v: dict(median=round(med(v), 2), min=round(v[0], 2), max=round(v[-1], 2))
    print(json.dumps(dict(sequences=len(seqs), models=len(models), frames=[LENGTHS[0], LENGTHS[-1]], reps=args.reps, ragged_ms=row(ragged_ms),
                          one_by_one_ms=row(serial_ms), longest_member_alone_ms=row(longest_ms), speedup=round(med(serial_ms) / med(ragged_ms), 2),
                          same_status=status["ragged"] == status["one_by_one"], sequences_without_factor=sum(s != abi.OK for s in status["ragged"]))),
          flush=True)


if __name__ == "__main__":
    main()
