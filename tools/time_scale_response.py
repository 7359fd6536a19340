"""Developer tool (not part of the product or the tests): times the two entries of the length-marginal covariance -- cpe_scale_response and
cpe_covariance_add_scales -- beside cpe_covariance (with the marker covariance, as uncertainty=True calls it) and cpe_scale_system on the same
handle and batch: phantom, six cameras, N frames, the 11 segment groups, at the synthetic truth with damping --ridge.  cpe_scale_response runs
cpe_scale_system's launches, then the export of the factor, the back substitution for the G columns and k_scale_points; cpe_covariance_add_scales
is one kernel over the frames.  Device pointers, a host clock around a call that ends in a synchronise, one warm-up call, then the median of five.
Prints one JSON line per batch size, with the share of an uncertainty=True call (covariance + the new step) that the new step is.  No threshold.

    python tools/time_scale_response.py [--batches 256,16] [--N 200] [--ridge 1e-6]"""
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
    G, L = da.shape[0], 24
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
        return dict(median=round(float(np.median(ts)), 3), min=round(float(min(ts)), 3), max=round(float(max(ts)), 3))

    for B in [int(b) for b in args.batches.split(",")]:
        rep = lambda a: np.ascontiguousarray(np.concatenate([a] * (B // 8 + 1))[:B])
        q, me, we = (torch.tensor(rep(d[k]), device=dev) for k in ("q_true", "meas", "weight"))
        cd, co, cp = E(B, N, 28, 28), E(B, N, h.pb, 28, 28), E(B, N, L, 3, 3)
        cdm, com, cpm = E(B, N, 28, 28), E(B, N, h.pb, 28, 28), E(B, N, L, 3, 3)
        A, Ar, b, br, cost = E(B, G, G), E(B, G, G), E(B, G), E(B, G), E(B)
        ru, rp = E(B, N, 28, G), E(B, N, L, 3, G)
        cs = torch.tensor(np.broadcast_to(np.eye(G) * 1e-4, (B, G, G)).copy(), device=dev)
        seq = [None]

        def response():
            seq[0] = h.scale_response(q, me, we, da, dm, Ar, ru, rp, args.ridge)[1]
        cov = median_ms(lambda: h.covariance(q, me, we, args.ridge, cd, cov_off=co, cov_pos=cp))
        sc = median_ms(lambda: h.scale_system(q, me, we, da, dm, A, b, Ar, br, cost, args.ridge))
        rs = median_ms(response)
        ad = median_ms(lambda: h.covariance_add_scales(cs, ru, rp, cd, co, cp, cdm, com, cpm))
        new = rs["median"] + ad["median"]
        print(json.dumps(dict(B=B, N=N, cameras=6, groups=G, ridge=args.ridge, sequences_with_factor=int(sum(s == abi.OK for s in seq[0])),
                              covariance_ms=cov, scale_system_ms=sc, scale_response_ms=rs, add_scales_ms=ad,
                              new_step_share=round(new / (new + cov["median"]), 3))), flush=True)
        del q, me, we, cd, co, cp, cdm, com, cpm, ru, rp
        torch.cuda.empty_cache()
    h.close()


if __name__ == "__main__":
    main()
