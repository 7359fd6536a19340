"""Developer tool (not part of the product or the tests): times cpe_band_sample -- the banded back substitution with many right-hand sides -- next
to the two kernels that read the same factor: the covariance sweep (cpe_band_inverse: k_cov_prep + k_lm_selinv) and the back substitution of one
LM step (k_lm_back inside cpe_eval_lm_step: ONE right-hand side per sequence).  Two shapes: phantom with six cameras (half-bandwidth 3) and config 3,
one camera + the packaged priors (half-bandwidth 4); B sequences of N frames, S samples each.  The factor is cpe_covariance's at the synthetic
truth with damping --ridge.  Prints one JSON line per shape with host-clock milliseconds (best of three around calls that end in a synchronise);
under `rocprofv3 --kernel-trace --stats` the per-kernel times of the same calls are in the trace.  No threshold; the numbers quoted in
profiles/r09_band_sample_notes.md and DESIGN.md section 4.

    python tools/time_samples.py [--B B] [--N N] [--S S] [--ridge R]"""
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
    from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--ridge", type=float, default=1e-6)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, N, S = args.B, args.N, args.S
    cams6 = synth.make_cameras(6)
    shapes = (("6 cameras", skeleton.build_skeleton("phantom", 25), cams6, None),
              ("config 3: 1 camera + priors", skeleton.build_skeleton("phantom", 24), (abi.Camera * 1)(cams6[2]), priors.load_priors()))
    for label, sk, cams, pr in shapes:
        d = synth.make_batch(sk, cams, B=B, N=N, seed=1234)
        q, me, we = (torch.tensor(np.ascontiguousarray(d[k]), device=dev) for k in ("q_true", "meas", "weight"))
        h = _lib.Handle(sk, cams, abi.default_options(120.0), pr)
        E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        cd, co, Lf = E(B, N, 28, 28), E(B, N, h.pb, 28, 28), E(B, N, h.pb + 1, 28, 28)
        _, seq = h.covariance(q, me, we, args.ridge, cd, cov_off=co, L=Lf); h.synchronize()
        z = torch.randn((B, S, N, 28), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        du, q_s, pos_s = E(B, S, N, 28), E(B, S, N, sk.nq), E(B, S, N, sk.n_markers, 3)
        seq8 = np.zeros((B, 8))

        def timed(call):
            call(); h.synchronize()                                                                  # warm-up: code objects, workspaces
            best = None
            for _ in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                call()
                h.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                best = dt if best is None else min(best, dt)
            return round(best, 3)

        ms_sample = timed(lambda: h.band_sample(Lf, z, du))
        ms_sweep = timed(lambda: h.band_inverse(Lf, cd, co))
        ms_lm = timed(lambda: h._call(h.lib.cpe_eval_lm_step, "cpe_eval_lm_step", None, B, N, q.data_ptr(), me.data_ptr(), we.data_ptr(), None,
                                      args.ridge, None, None, None, None, None, seq8.ctypes.data))
        ms_pose = timed(lambda: h.posterior_samples(q, du, q_s, pos_s))
        print(json.dumps(dict(shape=label, B=B, N=N, S=S, half_bandwidth=h.pb, ridge=args.ridge, sequences_with_factor=int(sum(s == abi.OK for s in seq)),
                              finite=bool(torch.isfinite(du).all()), band_sample_ms=ms_sample, band_inverse_ms=ms_sweep, lm_iteration_ms=ms_lm,
                              posterior_samples_ms=ms_pose, band_sample_us_per_sample_column=round(1e3 * ms_sample / (B * S * N), 5))), flush=True)
        h.close()
        del q, me, we, cd, co, Lf, z, du, q_s, pos_s
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
