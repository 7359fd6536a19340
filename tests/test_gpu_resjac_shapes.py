"""k_resjac against the oracle at the smallest shapes where the structure of its frame loop can go wrong (tests/resjac_compare.py: the
comparator, TOL and the NEAR_SHARE_MAX cap, unchanged; the fenced runs of tests/test_gpu_resjac.py):

  slots23   L = 23, 6 cameras, 3 x 5     S = 256: exactly four full rounds of 64 Jacobian slots and no tail round; 15 frames, so the last
                                         workgroup has an idle wave
  slots5    L = 5, 3 cameras, 2 x 9      S = 52: no full round; one projection pass; an odd camera count
  slots1    L = 1, 1 camera, 4 x 6       S = 12
  slots16   L = 16, 7 cameras, 2 x 40    S = 188: two full rounds and a tail of 60; 112 (camera, marker) pairs, two projection passes
  wrap2051  L = 25, 6 cameras, 1 x 2051  N is above the grid stride of 2048 frames on 256 compute units: the carried n = f mod N advances by
                                         less than N and wraps on a wave's second frame (the tail* cases of test_gpu_resjac.py have strides above N)

Inputs as resjac_compare.case_inputs builds them: synth.make_batch runs of 200 frames (seed + run), q = q_true + N(0, 0.05) from default_rng(5),
cut into the case's sequences.  Share of rows nearer than NEAR_Z to a camera plane, measured on the CPU for these seeds: 0 for the four small
cases, 0.16 % for wrap2051 -- inside the 0.5 % cap, which _compare asserts again.  Every case runs with the cost; slots16 also without it, bit
for bit equal in r, J and eps."""
import functools

import numpy as np
import pytest

import resjac_compare as RC
import test_gpu_resjac as TG
from cheetah_pose_estimation_amd import abi, skeleton, synth

pytestmark = pytest.mark.gpu

# name: (markers, cameras, B, N, first seed, expected slots S)
SHAPES = {
    "slots23": (23, 6, 3, 5, 9910, 256),
    "slots5": (5, 3, 2, 9, 9920, 52),
    "slots1": (1, 1, 4, 6, 9930, 12),
    "slots16": (16, 7, 2, 40, 9940, 188),
    "wrap2051": (25, 6, 1, 2051, 9950, 276),
}


@functools.lru_cache(maxsize=None)
def shape_inputs(name):
    """dict(sk, cams, opts, q [B, N, nq], meas [B, N, C, L, 2], weight [B, N, C, L]) of a case"""
    L, C, B, N, seed, _ = SHAPES[name]
    sk, cams, opts = skeleton.build_skeleton("phantom", L), synth.make_cameras(C), abi.default_options()
    runs = -(-B * N // 200)
    d = synth.make_batch(sk, cams, B=runs, N=200, fps=120.0, seed=seed)
    q = d["q_true"] + np.random.default_rng(5).normal(0, 0.05, d["q_true"].shape)
    cut = lambda a: np.ascontiguousarray(a.reshape((runs * 200,) + a.shape[2:])[:B * N].reshape((B, N) + a.shape[2:]))
    return dict(sk=sk, cams=cams, opts=opts, q=cut(q), meas=cut(d["meas"]), weight=cut(d["weight"]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape(oracle, gpu_handle_factory, name):
    L, C, B, N, _, S = SHAPES[name]
    c = shape_inputs(name)
    h = gpu_handle_factory(c["sk"], c["cams"], c["opts"])
    assert (h.S, h.L, h.n_cams) == (S, L, C)
    F = B * N
    if name == "slots23":
        assert S % 64 == 0 and F % 4 != 0                              # full rounds only; idle waves in the last workgroup
    if name == "slots16":
        assert S // 64 == 2 and S % 64 == 60 and 64 < C * L <= 128     # a tail round; two projection passes
    if name == "wrap2051":
        ws = TG._wstride(F)
        assert ws < N < 2 * ws, (ws, N)                                 # n advances by ws < N and wraps on the second frame of a wave
    G = TG._run(h, c["q"], c["meas"], c["weight"], want_cost=True)
    if name == "slots16":
        G0 = TG._run(h, c["q"], c["meas"], c["weight"], want_cost=False)
        assert G0["cost"] is None and all(TG._same(G[k], G0[k]) for k in ("r", "J", "eps"))
    w = TG._compare(oracle, c, TG._host(G), name)
    assert "cost" in w
