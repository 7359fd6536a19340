"""Developer tool (not part of the product or the tests): times cpe_covariance -- the posterior covariance of the kinematic estimate -- next to one
LM iteration of the same handle, at the two shapes the benchmark solves: phantom, six cameras, N = 200, B = 512 (half-bandwidth 3), and config 3,
one camera + the packaged priors, N = 200, B = 2048 (half-bandwidth 4).  The covariance is taken at the synthetic truth with damping --ridge; the LM
iteration is cpe_eval_lm_step on the same batch at the same damping.  Prints one JSON line per shape: milliseconds of cpe_covariance with every
output (best of three, host clock around a call that ends in a synchronise), the same without the marker covariance and with the diagonal
blocks only, the sequences with a factor, and the milliseconds of the LM iteration.  With --columns K also cpe_covariance_columns on that
covariance's factor and band, K anchors per sequence spread from the last frame down (device pointers, timed the same way).  With --rates also
cpe_rate_covariance with all seven outputs on the band just computed (k_point_jac and k_rate_cov; device pointers, timed the same way).  No
threshold; the numbers quoted in DESIGN.md sections 4 and 6.

    python tools/time_covariance.py [--batch6 B] [--batch1 B] [--N N] [--ridge R] [--columns K] [--rates]"""
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
    ap.add_argument("--batch6", type=int, default=512, help="sequences of the six-camera shape")
    ap.add_argument("--batch1", type=int, default=2048, help="sequences of the config-3 shape")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--ridge", type=float, default=1e-6)
    ap.add_argument("--columns", type=int, default=0, help="also time cpe_covariance_columns with this many anchors per sequence")
    ap.add_argument("--rates", action="store_true", help="also time cpe_rate_covariance with all seven outputs")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    N = args.N
    cams6 = synth.make_cameras(6)
    shapes = (("6 cameras", skeleton.build_skeleton("phantom", 25), cams6, None, args.batch6),
              ("config 3: 1 camera + priors", skeleton.build_skeleton("phantom", 24), (abi.Camera * 1)(cams6[2]), priors.load_priors(), args.batch1))
    for label, sk, cams, pr, B in shapes:
        opts = abi.default_options(120.0)
        d = synth.make_batch(sk, cams, B=8, N=N, seed=1234)
        rep = lambda a: np.ascontiguousarray(np.concatenate([a] * (B // 8 + 1))[:B])
        q, me, we = (torch.tensor(rep(d[k]), device=dev) for k in ("q_true", "meas", "weight"))
        h = _lib.Handle(sk, cams, opts, pr)
        E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        cd, co, cp = E(B, N, 28, 28), E(B, N, h.pb, 28, 28), E(B, N, sk.n_markers, 3, 3)

        def timed(**kw):
            best, seq = None, None
            for _ in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, seq = h.covariance(q, me, we, args.ridge, cd, **kw)
                h.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            return 1e3 * best, seq

        h.covariance(q, me, we, args.ridge, cd, cov_off=co, cov_pos=cp); h.synchronize()          # warm-up: code objects, workspaces
        ms_all, seq = timed(cov_off=co, cov_pos=cp)
        ms_nopos, _ = timed(cov_off=co)
        ms_diag, _ = timed()
        # one LM iteration of the same handle over the same batch: cpe_eval_lm_step (evaluation, band, factor, back substitution, trial iterate)
        # with no output but the per-sequence record, timed the same way
        seq8 = np.zeros((B, 8))
        lam = args.ridge if args.ridge > 0.0 else 1e-6
        ms_lm = None
        for _ in range(4):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            h._call(h.lib.cpe_eval_lm_step, "cpe_eval_lm_step", None, B, N, q.data_ptr(), me.data_ptr(), we.data_ptr(), None, lam, None, None, None,
                    None, None, seq8.ctypes.data)
            h.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            ms_lm = dt if ms_lm is None else min(ms_lm, dt)
        extra = {}
        if args.columns > 0:
            K = args.columns
            Lf, cols = E(B, N, h.pb + 1, 28, 28), E(B, K, N, 28, 28)
            h.covariance(q, me, we, args.ridge, cd, cov_off=co, L=Lf); h.synchronize()
            anchors = np.tile(np.array([N - 1 - (k * N) // K for k in range(K)], dtype=np.int32), (B, 1))
            ms_cols = None
            for _ in range(4):                                                                       # (the first call is the warm-up)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                h.covariance_columns(Lf, cd, co, anchors, cols)
                h.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                ms_cols = dt if ms_cols is None else min(ms_cols, dt)
            extra = dict(column_anchors=anchors[0].tolist(), columns_ms=round(ms_cols, 3))
            del Lf, cols
        if args.rates:
            L = sk.n_markers
            h.covariance(q, me, we, args.ridge, cd, cov_off=co); h.synchronize()                     # the band the rates are taken on
            outs = dict(cov_du=E(B, N, 28, 28), cov_ddu=E(B, N, 28, 28), cov_vel=E(B, N, L, 3, 3), cov_com=E(B, N, 3, 3), cov_com_vel=E(B, N, 3, 3),
                        jac_pos=E(B, N, L, 3, 28), jac_com=E(B, N, 3, 28))
            ms_rates = None
            for _ in range(4):                                                                       # (the first call is the warm-up)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                h.rate_covariance(q, cd, co, **outs)
                h.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                ms_rates = dt if ms_rates is None else min(ms_rates, dt)
            extra.update(rates_ms=round(ms_rates, 3))
            del outs
        print(json.dumps(dict(shape=label, B=B, N=N, half_bandwidth=h.pb, ridge=args.ridge, sequences_with_factor=int(sum(s == abi.OK for s in seq)),
                              covariance_ms=round(ms_all, 3), without_cov_pos_ms=round(ms_nopos, 3), diagonal_only_ms=round(ms_diag, 3),
                              lm_iteration_ms=round(ms_lm, 3), **extra)), flush=True)
        h.close()
        del q, me, we, cd, co, cp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
