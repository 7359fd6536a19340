"""Developer tool (not part of the product or the tests): times cpe_force_samples -- the first pass of cpe_covariance_kinetic plus k_force_sample,
which factors every node's force matrix once and draws S samples from it -- next to cpe_covariance_kinetic (every output asked for) and
cpe_band_sample on that call's factor, at config 4's shape: phantom, six cameras, gallop, free foot forces, device tensors (no PCIe).  Two shapes by
default, (B, N, S) = (1, 200, 256) and (16, 200, 64).  Every call is timed warm, `--reps` times, host clock around a call that ends in a synchronise.
Prints one JSON line per shape: median and min / max in milliseconds.  No threshold; the numbers quoted in profiles/r10_force_sample_notes.md and
DESIGN.md section 4.

    python tools/time_force_samples.py [--shapes B,N,S ...] [--reps R] [--ridge RIDGE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    import torch
    from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["1,200,256", "16,200,64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ridge", type=float, default=1e-6)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sk = skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24))
    cams = synth.make_cameras(6)
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    for shape in args.shapes:
        B, N, S = (int(v) for v in shape.split(","))
        d = synth.make_gallop_batch(sk, cams, B=min(B, 8), N=N, seed=4321)
        rep = lambda a: np.ascontiguousarray(np.concatenate([a] * (B // min(B, 8) + 1))[:B])
        T = {k: torch.tensor(rep(d[k]), device=dev) for k in ("q_init", "meas", "weight")}
        T["stance"] = torch.tensor(rep(d["stance"]).astype(np.int32), device=dev)
        h = _lib.Handle(sk, cams, abi.default_options(120.0))
        o = dict(cov_diag=E(B, N, 28, 28), cov_off=E(B, N, 3, 28, 28), cov_pos=E(B, N, 24, 3, 3), cov_f=E(B, N, 64, 64), f=E(B, N, 64),
                 meta=torch.empty((B, N, 65), dtype=torch.int32, device=dev), L=E(B, N, 4, 28, 28))
        gen = torch.Generator(device=dev).manual_seed(1)
        z = torch.randn((B, S, N, 28), dtype=torch.float64, device=dev, generator=gen)
        zeta = torch.randn((B, S, N, 64), dtype=torch.float64, device=dev, generator=gen)
        du, f_s = E(B, S, N, 28), E(B, S, N, 64)
        status = {}

        def timed(fn):
            fn()                                               # warm-up (workspace allocation, code objects)
            out = []
            for _ in range(args.reps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                out.append(1e3 * (time.perf_counter() - t0))
            out.sort()
            return dict(median=round(statistics.median(out), 3), min=round(out[0], 3), max=round(out[-1], 3))

        def cov():
            status["covariance"] = h.covariance_kinetic(ko, T["q_init"], T["meas"], T["weight"], T["stance"], args.ridge, **o)
            h.synchronize()

        def band():
            h.band_sample(o["L"], z, du)
            h.synchronize()

        def force():
            status["samples"] = h.force_samples(ko, T["q_init"], T["meas"], T["weight"], T["stance"], args.ridge, du, f_s, zeta=zeta)
            h.synchronize()
        ms = dict(covariance_kinetic_ms=timed(cov), band_sample_ms=timed(band), force_samples_ms=timed(force))
        print(json.dumps(dict(B=B, N=N, S=S, ridge=args.ridge, reps=args.reps, **ms,
                              sequences_without_factor=sum(s != abi.OK for s in status["samples"][1]),
                              same_status=status["samples"][1] == status["covariance"][1], finite=bool(torch.isfinite(f_s).all()))), flush=True)
        h.close()
        del T, o, z, zeta, du, f_s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
