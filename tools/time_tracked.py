"""Developer tool (not part of the product or the tests): times the physics-based solve at config 4's shape -- phantom, six cameras, gallop, N = 200,
B sequences, free foot forces -- with the 2D reprojection cost (cpe_solve_kinetic) and with the 3D kinematic cost (cpe_solve_kinetic_tracked,
estimate_kinetics(use_2d_reprojections=False)) and with its full-weight form (cpe_solve_kinetic_tracked_weighted, track_weights="posterior":
W from one cpe_track_precision call on synthetic covariance blocks, standard deviations over two decades), from the same start, the tracked
solves' target being the start itself.  Prints one JSON line per
mode: solves/s of the timed solve and the per-kernel milliseconds per launch of the handle's HIP-event profile of the untimed warm-up solve (slot
k_frame_normal holds k_frame_tracked in the tracked mode).  The numbers quoted in DESIGN.md section 4.

    python tools/time_tracked.py [--batch B] [--max-iter K]"""
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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--max-iter", type=int, default=60, help="LM iterations per solve (capped: both modes run the same count)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, N = args.batch, args.N
    sk = skeleton.without_motion_model(skeleton.build_skeleton("phantom", 24))
    cams = synth.make_cameras(6)
    opts = abi.default_options(120.0)
    opts.tol_cost, opts.tol_step, opts.max_iter = 0.0, 0.0, args.max_iter          # every sequence runs max_iter iterations in both modes
    d = synth.make_gallop_batch(sk, cams, B=8, N=N, seed=4321)
    rep = lambda a: np.ascontiguousarray(np.concatenate([a] * (B // 8 + 1))[:B])
    T = {k: torch.tensor(rep(d[k]), device=dev) for k in ("q_init", "meas", "weight")}
    T["stance"] = torch.tensor(rep(d["stance"]).astype(np.int32), device=dev)
    nm, nf = 22, 4
    h = _lib.Handle(sk, cams, opts)
    nc = h.n_constraint_rows()
    E = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    out = dict(q=E(B, N, 54), dq=E(B, N, 54), ddq=E(B, N, 54), positions=E(B, N, 24, 3), meas_err=E(B, N, 6, 24, 2), tau=E(B, N, nm),
               lam=E(B, N, nc), grf=E(B, N, nf, 5), slack=E(B, N, 54))
    ko = abi.default_kinetic_options(skeleton.dyn_options("phantom"), 120.0)
    rng = np.random.default_rng(7)
    A = rng.standard_normal((8, N, 28, 28)) / np.sqrt(28.0)
    s = 10.0 ** rng.uniform(-2.0, 0.0, (8, N, 28))
    S = A @ np.swapaxes(A, -1, -2) + 0.5 * np.eye(28)
    cov = torch.tensor(rep(s[..., :, None] * (0.5 * (S + np.swapaxes(S, -1, -2))) * s[..., None, :]), device=dev)
    W = E(B, N, 28, 28)
    h.track_precision(cov, W)
    for mode in ("2d", "tracked", "weighted"):
        if mode != "2d":
            ko.w_torque, ko.w_smooth = 1.0 + 1e-3 / 120.0 ** 2, 0.0
        run = (lambda: h.solve_kinetic(ko, T["q_init"], T["meas"], T["weight"], T["stance"], out["q"], out["dq"], out["ddq"], out["positions"],
                                       out["meas_err"], out["tau"], out["lam"], out["grf"], out["slack"])) if mode == "2d" else \
              (lambda: h.solve_kinetic_tracked(ko, T["q_init"], T["q_init"], T["stance"], out["q"], out["dq"], out["ddq"], out["positions"],
                                               tau=out["tau"], lam=out["lam"], grf=out["grf"], slack=out["slack"])) if mode == "tracked" else \
              (lambda: h.solve_kinetic_tracked_weighted(ko, W, T["q_init"], T["q_init"], T["stance"], out["q"], out["dq"], out["ddq"], out["positions"],
                                                        tau=out["tau"], lam=out["lam"], grf=out["grf"], slack=out["slack"]))
        h.profile(True)
        run(); h.synchronize()
        prof = h.profile_totals()
        h.profile(False)
        t0 = time.perf_counter()
        st, stats, _ = run(); h.synchronize()
        dt = time.perf_counter() - t0
        its = [s.iterations for s in stats]
        print(json.dumps(dict(mode=mode, B=B, N=N, iterations=[min(its), max(its)], seconds=round(dt, 4), solves_per_s=round(B / dt, 2),
                              ms_per_launch={k: round(ms / max(n, 1), 4) for k, (ms, n) in prof.items()})), flush=True)
    h.close()


if __name__ == "__main__":
    main()
