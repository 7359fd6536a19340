#!/usr/bin/env python3
"""Developer tool: k_resjac of two builds of the library on THIS box, interleaved in one process.

    python tools/ab_resjac_builds.py A.so B.so [--rounds 4] [--launches 40] [--preheat 1.5] [--json OUT]

Both libraries are loaded side by side, each with a handle of its own on the benchmark's shape (2048 x 200 frames, 6 cameras, 25 markers).  After
`--preheat` seconds of untimed launches (both builds in turn) come `--rounds` alternations A, B, A, B, ..., each run `--launches` launches timed
one by one with HIP events on the handle's stream.  Both builds read the same inputs and write the same output buffers.  Printed: the mean (and median) milliseconds per launch of every run, the mean ratio B / A, and
whether the ranges overlap -- B counts as faster only if its slowest run beats A's fastest.  The outputs of the two builds are also compared bit
for bit (r, J, eps as int64).  Run-to-run spread of one build is about 3 % and boxes differ by 8 %, so numbers from separate processes or boxes
do not compare.  Run a pair in both orders (A B, then B A): what is left of a difference after the swap belongs to the builds."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, torch
from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a"); ap.add_argument("lib_b")
    ap.add_argument("--rounds", type=int, default=4); ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--preheat", type=float, default=1.5); ap.add_argument("--json")
    a = ap.parse_args()
    if a.rounds < 4 or a.launches < 40:
        sys.exit("at least 4 alternations of 40 launches")
    sk = skeleton.build_skeleton("phantom", 25); cams = synth.make_cameras(6)
    d = synth.make_batch(sk, cams, B=16, N=200, seed=1)
    dev = torch.device("cuda", 0)
    T = {k: torch.tensor(d[k], device=dev).repeat((128,) + (1,) * (d[k].ndim - 1)).contiguous() for k in ("q_true", "meas", "weight")}
    B, N = T["q_true"].shape[:2]
    H = {}
    for name, path in (("A", a.lib_a), ("B", a.lib_b)):
        _lib.LIB_PATH = os.path.abspath(path); _lib._LIB = None
        H[name] = _lib.Handle(sk, cams, abi.default_options())
    h = H["A"]
    # ONE set of output buffers for both builds: the same kernel writing to another 11 GB allocation has measured up to 7 % apart on one box
    out = (torch.empty((B, N, 6, 25, 2), dtype=torch.float64, device=dev), torch.empty((B, N, 6, h.S, 2), dtype=torch.float64, device=dev),
           torch.empty((B, N, h.nq), dtype=torch.float64, device=dev))
    launch = lambda k: H[k].eval_resjac(T["q_true"], T["meas"], T["weight"], *out)
    launch("A"); H["A"].synchronize()
    ref = [x.clone() for x in out]              # A's outputs, for the bit comparison with B's at the end
    for x in out:
        x.fill_(float("nan"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.preheat:
        for k in ("A", "B"):
            for _ in range(10):
                launch(k)
            H[k].synchronize()
    runs = {"A": [], "B": []}
    for _ in range(a.rounds):
        for k in ("A", "B"):
            with torch.cuda.stream(torch.cuda.ExternalStream(H[k].stream, device=dev)):      # events and launches on the handle's own stream
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
                for e0, e1 in ev:
                    e0.record(); launch(k); e1.record()
                H[k].synchronize()
                ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
            runs[k].append((float(ms.mean()), float(np.median(ms))))
    launch("B"); H["B"].synchronize()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(x.view(torch.int64), y.view(torch.int64))) for x, y in zip(ref, out))
    mean = {k: float(np.mean([m for m, _ in v])) for k, v in runs.items()}
    res = dict(lib_a=a.lib_a, lib_b=a.lib_b, launches=a.launches, runs_ms={k: [round(m, 4) for m, _ in v] for k, v in runs.items()},
               medians_ms={k: [round(m, 4) for _, m in v] for k, v in runs.items()}, mean_ms={k: round(v, 4) for k, v in mean.items()},
               ratio_b_over_a=round(mean["B"] / mean["A"], 4), b_slowest_below_a_fastest=max(m for m, _ in runs["B"]) < min(m for m, _ in runs["A"]),
               outputs_bit_equal=same)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f)
    for h in H.values():
        h.close()


if __name__ == "__main__":
    main()
