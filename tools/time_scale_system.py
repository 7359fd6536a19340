"""Developer tool (not part of the product or the tests): times cpe_scale_system -- the reduced system of the length calibration -- beside
cpe_covariance on the same handle and batch: phantom, six cameras, N frames, the 11 segment groups, at the synthetic truth with damping --ridge.
Both entries run the same first pass up to the band factor; cpe_covariance then sweeps the band (diagonal and off-diagonal blocks, no marker
covariance), cpe_scale_system runs k_scale_cross and k_band_forward.  Device pointers, a host clock around a call that ends in a synchronise,
one warm-up call, then the median of five.  Prints one JSON line per batch size.  No threshold; the numbers quoted in DESIGN.md section 4.

    python tools/time_scale_system.py [--batches 256,16] [--N 200] [--ridge 1e-6]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    import torch
    from cheetah_pose_estimation_amd import _lib, abi, skeleton, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,16")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--ridge", type=float, default=1e-6)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N = args.N
    sk, cams = skeleton.build_skeleton("phantom", 24), synth.make_cameras(6)
    da, dm = skeleton.length_derivatives("phantom", 24)
    G = da.shape[0]
    d = synth.make_batch(sk, cams, B=8, N=N, seed=1234)
    h = _lib.Handle(sk, cams, abi.default_options(120.0))
    E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)

    def median_ms(call):
        call(); h.synchronize()                                        # warm-up: code objects, workspaces
        ts = []
        for _ in range(5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()
            h.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts)), float(min(ts)), float(max(ts))

    for B in [int(b) for b in args.batches.split(",")]:
        rep = lambda a: np.ascontiguousarray(np.concatenate([a] * (B // 8 + 1))[:B])
        q, me, we = (torch.tensor(rep(d[k]), device=dev) for k in ("q_true", "meas", "weight"))
        cd, co = E(B, N, 28, 28), E(B, N, h.pb, 28, 28)
        A, Ar, b, br, cost = E(B, G, G), E(B, G, G), E(B, G), E(B, G), E(B)
        seq = [None]

        def scale():
            seq[0] = h.scale_system(q, me, we, da, dm, A, b, Ar, br, cost, args.ridge)[1]
        cov = median_ms(lambda: h.covariance(q, me, we, args.ridge, cd, cov_off=co))
        sc = median_ms(scale)
        print(json.dumps(dict(B=B, N=N, cameras=6, groups=G, ridge=args.ridge, sequences_with_factor=int(sum(s == abi.OK for s in seq[0])),
                              covariance_ms=dict(median=round(cov[0], 3), min=round(cov[1], 3), max=round(cov[2], 3)),
                              scale_system_ms=dict(median=round(sc[0], 3), min=round(sc[1], 3), max=round(sc[2], 3)))), flush=True)
        del q, me, we, cd, co
        torch.cuda.empty_cache()
    h.close()


if __name__ == "__main__":
    main()
