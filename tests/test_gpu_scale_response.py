"""The response of the poses to the segment-length scales and the covariance marginalised over them on the GPU (cpe_scale_response,
cpe_covariance_add_scales, include/cpe.h: k_band_forward's Y_E, k_band_sample, k_scale_points, k_cov_add_scales) entry by entry against the reference
of tests/marginal_compare.py.  All cases are scale_compare's, at the smallest shapes where the kernels can go wrong:

  plain        N = 5, past the half-bandwidth; the 25th marker has no length dependence (Ds = 0, W = P R)
  n1, n2       no off-diagonal block; fewer frames than the half-bandwidth
  ragged       lengths 5 and 2, two models, camera stride different from the second model's camera count
  g1, g16      one group; 16 = CPE_MAX_SCALES with a group without a link: its columns of resp_u and resp_pos are exactly zero and the marginal does
               not change with its variance
  prior        half-bandwidth 4
  cams1        one camera
  batch3       B = 3: bit-equal to three single calls, to itself reversed and to a repeat

cov_s = the reference's (A_red + I / 0.01)^-1, handed to both sides.  Tolerances: marginal_compare.tolerance(case), measured on the CPU; the GPU's
worst values are printed by test_zz_report and never feed a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import marginal_compare as MC
import scale_compare as SC
from cheetah_pose_estimation_amd import _lib, abi, priors, skeleton, synth

pytestmark = pytest.mark.gpu

WORST = {}
HANDLES = {}
RUNS = {}
OUT = ("cov_diag", "cov_off", "cov_pos")


def _handle(name):
    """the handle of a case (one per module run) and the stacked derivative tables of its models"""
    c = SC.case_inputs(name)
    if name not in HANDLES:
        sks = [m[0] for m in c["models"]]
        if len(sks) == 1:
            h = _lib.Handle(sks[0], c["models"][0][3], c["opts"], c["pr"])
        else:
            h = _lib.Handle.multi(sks, [m[3] for m in c["models"]], [c["opts"]] * len(sks), c["pr"])
        HANDLES[name] = h
    return c, HANDLES[name], np.stack([m[1] for m in c["models"]]), np.stack([m[2] for m in c["models"]])


def _chain(h, c, da, dm, q, me, we, cov_s, model=None):
    """covariance -> scale_response -> add_scales over sequences given as lists; cov_s: one [G, G] per sequence.  Returns the padded arrays
    (resp_u, resp_pos, the band GIVEN the lengths, the marginal one), A_red, the statuses and the lengths"""
    lens = [len(a) for a in q]
    if model is None:
        Q, M, W = np.stack(q), np.stack(me), np.stack(we)
        cov = h.covariance_host(Q, M, W, c["ridge"])
        rs = h.scale_response_host(Q, M, W, da, dm, c["ridge"])
        nf, pad, rp = None, cov, rs
    else:
        cov = h.covariance_ragged_host(list(q), list(me), list(we), model, c["ridge"])
        rs = h.scale_response_host(list(q), list(me), list(we), da, dm, c["ridge"], model_list=model)
        nf, pad, rp = lens, cov["padded"], rs["padded"]
    m = h.covariance_add_scales_host(np.stack(cov_s), rp["resp_u"], rp["resp_pos"], pad["cov_diag"], pad["cov_off"], pad["cov_pos"], nf)
    return dict(resp_u=rp["resp_u"], resp_pos=rp["resp_pos"], A_red=rs["A_red"], cond={k: pad[k] for k in OUT}, marg=m, lens=lens,
                seq_status=rs["seq_status"], cov_status=cov["seq_status"])


def _run(oracle, name):
    if name not in RUNS:
        c, h, da, dm = _handle(name)
        R = MC.case_reference(oracle, name)
        ragged = len(c["models"]) > 1
        RUNS[name] = _chain(h, c, da, dm, c["q"], c["meas"], c["weight"], [S["cov_s"] for S in R], c["model"] if ragged else None)
    return RUNS[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in HANDLES.values():
        h.close()
    HANDLES.clear()
    RUNS.clear()


@pytest.mark.parametrize("name", MC.CASES)
def test_response_and_marginal_match_the_reference(oracle, name):
    c, h, da, dm = _handle(name)
    R = MC.case_reference(oracle, name)
    out = _run(oracle, name)
    B, lens = len(c["q"]), out["lens"]
    assert out["seq_status"] == out["cov_status"] == [abi.OK] * B
    cut = lambda a: [a[b, :n] for b, n in enumerate(lens)]
    G = dict(resp_u=cut(out["resp_u"]), resp_pos=cut(out["resp_pos"]), cov_diag_m=cut(out["marg"]["cov_diag"]), cov_off_m=cut(out["marg"]["cov_off"]),
             cov_pos_m=cut(out["marg"]["cov_pos"]))
    d = MC.discrepancies(G, R)
    print(name, ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    tol = MC.tolerance(name)
    for k, v in d.items():                                           # the worst share of its tolerance, for the record
        share = v / tol[k] if tol[k] > 0 else (0.0 if v == 0.0 else float("inf"))
        if share >= WORST.get(k, (0.0, 0.0, ""))[0]:
            WORST[k] = (share, v, name)
    assert not MC.failures(d, tol), (name, MC.failures(d, tol), tol)
    # A_red: cpe_scale_system's bits
    if len(c["models"]) > 1:
        sys_ = h.scale_system_host(list(c["q"]), list(c["meas"]), list(c["weight"]), da, dm, c["ridge"], model_list=c["model"])
    else:
        sys_ = h.scale_system_host(np.stack(c["q"]), np.stack(c["meas"]), np.stack(c["weight"]), da, dm, c["ridge"])
    assert sys_["A_red"].tobytes() == out["A_red"].tobytes()
    # zero past a sequence's frames, and the blocks (n + i, n) with n + i past them
    pb = h.pb
    for b, n in enumerate(lens):
        for a in (out["resp_u"], out["resp_pos"], out["marg"]["cov_diag"], out["marg"]["cov_off"], out["marg"]["cov_pos"]):
            assert not a[b, n:].any()
        for f in range(n):
            for i in range(1, pb + 1):
                assert (f + i < n) == bool(out["marg"]["cov_off"][b, f, i - 1].any())
    # the marginal variances are at or above the conditional ones
    assert np.all(np.einsum("bnkk->bnk", out["marg"]["cov_diag"]) >= np.einsum("bnkk->bnk", out["cond"]["cov_diag"]))
    assert np.all(np.einsum("bnlaa->bnla", out["marg"]["cov_pos"]) >= np.einsum("bnlaa->bnla", out["cond"]["cov_pos"]))
    # a group no marker depends on: exactly zero columns
    for g, (_, links) in enumerate(c["groups"]):
        if not links:
            assert not out["resp_u"][..., g].any() and not out["resp_pos"][..., g].any()


def test_zero_scale_covariance_returns_the_band(oracle):
    """cov_s = 0: the marginal band and marker blocks are the input's bits"""
    c, h, da, dm = _handle("plain")
    out = _run(oracle, "plain")
    G = len(c["groups"])
    m = h.covariance_add_scales_host(np.zeros((1, G, G)), out["resp_u"], out["resp_pos"], *[out["cond"][k] for k in OUT])
    for k in OUT:
        assert m[k].tobytes() == out["cond"][k].tobytes(), k
    # without the marker arrays the band is the same
    mb = h.covariance_add_scales_host(np.stack([S["cov_s"] for S in MC.case_reference(oracle, "plain")]), out["resp_u"], None, out["cond"]["cov_diag"],
                                      out["cond"]["cov_off"], None)
    assert mb["cov_pos"] is None and all(mb[k].tobytes() == out["marg"][k].tobytes() for k in OUT[:2])


def test_only_the_lower_triangle_of_cov_s_is_read_and_a_linkless_group_changes_nothing(oracle):
    c, h, da, dm = _handle("g16")
    out = _run(oracle, "g16")
    cs = MC.case_reference(oracle, "g16")[0]["cov_s"].copy()
    args = (out["resp_u"], out["resp_pos"]) + tuple(out["cond"][k] for k in OUT)
    upper = cs.copy()
    upper[np.triu_indices(16, 1)] = 7.0
    g = [i for i, (_, links) in enumerate(c["groups"]) if not links][0]
    wide = cs.copy()
    wide[g, g] *= 100.0
    for other in (upper, wide):
        m = h.covariance_add_scales_host(other[None], *args)
        for k in OUT:
            assert m[k].tobytes() == out["marg"][k].tobytes(), k


def test_batch_reverse_and_repeat_are_bit_equal(oracle):
    c, h, da, dm = _handle("batch3")
    full = _run(oracle, "batch3")
    cs = [S["cov_s"] for S in MC.case_reference(oracle, "batch3")]
    again = _chain(h, c, da, dm, c["q"], c["meas"], c["weight"], cs)
    back = _chain(h, c, da, dm, c["q"][::-1], c["meas"][::-1], c["weight"][::-1], cs[::-1])
    flat = lambda r: [r["resp_u"], r["resp_pos"], r["A_red"]] + [r["marg"][k] for k in OUT]
    for x, y, z in zip(flat(full), flat(again), flat(back)):
        assert x.tobytes() == y.tobytes() and x.tobytes() == np.ascontiguousarray(z[::-1]).tobytes()
    for b in range(3):
        one = _chain(h, c, da, dm, c["q"][b:b + 1], c["meas"][b:b + 1], c["weight"][b:b + 1], cs[b:b + 1])
        for x, y in zip(flat(full), flat(one)):
            assert x[b].tobytes() == y[0].tobytes(), b


def test_ragged_sequences_equal_their_plain_calls(oracle):
    c, h, da, dm = _handle("ragged")
    out = _run(oracle, "ragged")
    R = MC.case_reference(oracle, "ragged")
    flat = lambda r: [r["resp_u"], r["resp_pos"], r["A_red"]] + [r["marg"][k] for k in OUT]
    for b, m in enumerate(c["model"]):
        sk, a, o, cams = c["models"][m]
        hb = _lib.Handle(sk, cams, c["opts"], c["pr"])
        try:
            one = _chain(hb, c, a, o, [c["q"][b]], [c["meas"][b]], [c["weight"][b]], [R[b]["cov_s"]])
        finally:
            hb.close()
        n = out["lens"][b]
        for x, y in zip(flat(out), flat(one)):
            xb = x[b] if x.ndim == 3 else x[b, :n]
            assert np.ascontiguousarray(xb).tobytes() == y[0].tobytes(), b


def test_sequence_without_a_factor_and_of_no_frames(oracle):
    """cpe_scale_system's rule: CPE_NUMERICAL and all outputs zero, the neighbour keeps its bits; add_scales with a frame count of 0 reads nothing of
    that sequence (its inputs are NaN) and writes zeros"""
    c, h, da, dm = _handle("batch3")
    q, me, we = np.stack(c["q"])[:2, :3].copy(), np.stack(c["meas"])[:2, :3].copy(), np.stack(c["weight"])[:2, :3].copy()
    good = h.scale_response_host(q[:1], me[:1], we[:1], da, dm, 0.0)
    we[1] = 0.0; me[1] = 0.0
    out = h.scale_response_host(q, me, we, da, dm, 0.0)
    assert out["seq_status"] == [abi.OK, abi.NUMERICAL] and out["status"] == abi.NUMERICAL
    for k in ("A_red", "resp_u", "resp_pos"):
        assert not out[k][1].any() and out[k][0].tobytes() == good[k][0].tobytes(), k
    cov = h.covariance_host(q, me, we, 0.0)
    G = len(c["groups"])
    cs = np.stack([np.eye(G) * 1e-4] * 2)
    bad = lambda a: np.where(np.arange(2).reshape((2,) + (1,) * (a.ndim - 1)) == 1, np.nan, a)
    m = h.covariance_add_scales_host(bad(cs), bad(out["resp_u"]), bad(out["resp_pos"]), *[bad(cov[k]) for k in OUT], n_frames=[3, 0])
    ref = h.covariance_add_scales_host(cs[:1], out["resp_u"][:1], out["resp_pos"][:1], *[cov[k][:1] for k in OUT])
    for k in OUT:
        assert not m[k][1].any() and m[k][0].tobytes() == ref[k][0].tobytes(), k


def test_refusals():
    """every refusal of the two entries: CPE_BAD_ARG with the reason, the outputs untouched"""
    da, dm = skeleton.length_derivatives("phantom", 24)
    sk = skeleton.build_skeleton("phantom", 24)
    w5 = priors.load_priors(path=os.path.join(os.path.dirname(__file__), "golden", "priors_k3_w5_dense.npz"))
    h5 = _lib.Handle(sk, synth.make_cameras(2), abi.default_options(), w5)
    try:
        q, me, we = np.zeros((1, 6, h5.nq)), np.zeros((1, 6, 2, 24, 2)), np.zeros((1, 6, 2, 24))
        with pytest.raises(_lib.CpeError, match="cpe_scale_response_host: half-bandwidth 5 .* is not supported by the covariance sweep"):
            h5.scale_response_host(q, me, we, da, dm)
        with pytest.raises(_lib.CpeError, match="cpe_covariance_add_scales_host: half-bandwidth 5 .* is not supported by the covariance sweep"):
            h5.covariance_add_scales_host(np.zeros((1, 11, 11)), np.zeros((1, 6, 28, 11)), None, np.zeros((1, 6, 28, 28)), np.zeros((1, 6, 5, 28, 28)), None)
    finally:
        h5.close()
    h = _lib.Handle(sk, synth.make_cameras(2), abi.default_options(), None)
    try:
        lib, ptr = h.lib, (lambda a: None if a is None else a.ctypes.data)
        q, me, we = np.zeros((1, 3, h.nq)), np.zeros((1, 3, 2, 24, 2)), np.zeros((1, 3, 2, 24))
        outs = dict(A_red=np.full((1, 11, 11), 7.0), resp_u=np.full((1, 3, 28, 11), 7.0), resp_pos=np.full((1, 3, 24, 3, 11), 7.0))
        st = (C.c_int32 * 1)(5)
        i32 = lambda v: (C.c_int32 * 1)(v)

        def response(reason, B=1, N=3, model=None, n_frames=None, ridge=0.0, G=11, handle=h._h, **null):
            a = dict(q=q, meas=me, weight=we, d_attach=da, d_marker_off=dm, **outs)
            a.update(null)
            rc = lib.cpe_scale_response_host(handle, B, N, model, n_frames, ptr(a["q"]), ptr(a["meas"]), ptr(a["weight"]), ridge, G, ptr(a["d_attach"]),
                                             ptr(a["d_marker_off"]), ptr(a["A_red"]), ptr(a["resp_u"]), ptr(a["resp_pos"]), st)
            assert rc == abi.BAD_ARG and b"cpe_scale_response_host: " in lib.cpe_last_error() and reason in lib.cpe_last_error(), lib.cpe_last_error()
            assert all((o == 7.0).all() for o in outs.values()) and st[0] == 5

        response(b"G = 0 outside 1..16", G=0)
        response(b"G = 17 outside 1..16", G=17)
        response(b"ridge must be finite and >= 0", ridge=-1.0)
        response(b"ridge must be finite and >= 0", ridge=float("nan"))
        response(b"negative", B=-1)
        response(b"model and n_frames are given together", model=i32(0))
        response(b"frame count of sequence 0 outside 1..N", model=i32(0), n_frames=i32(0))
        response(b"frame count of sequence 0 outside 1..N", model=i32(0), n_frames=i32(4))
        response(b"model index of sequence 0 out of range", model=i32(1), n_frames=i32(3))
        response(b"null argument", handle=None)
        for k in ("q", "meas", "weight", "d_attach", "d_marker_off", "A_red", "resp_u"):
            response(b"null argument", **{k: None})

        pb, L = h.pb, 24
        ins = dict(cov_s=np.zeros((1, 11, 11)), resp_u=np.zeros((1, 3, 28, 11)), resp_pos=np.zeros((1, 3, L, 3, 11)), cov_diag=np.zeros((1, 3, 28, 28)),
                   cov_off=np.zeros((1, 3, pb, 28, 28)), cov_pos=np.zeros((1, 3, L, 3, 3)))
        mo = dict(cov_diag_m=np.full((1, 3, 28, 28), 7.0), cov_off_m=np.full((1, 3, pb, 28, 28), 7.0), cov_pos_m=np.full((1, 3, L, 3, 3), 7.0))

        def add(reason, B=1, N=3, n_frames=None, G=11, handle=h._h, **null):
            a = dict(ins, **mo)
            a.update(null)
            rc = lib.cpe_covariance_add_scales_host(handle, B, N, n_frames, G, *[ptr(a[k]) for k in list(ins) + list(mo)])
            assert rc == abi.BAD_ARG and b"cpe_covariance_add_scales_host: " in lib.cpe_last_error() and reason in lib.cpe_last_error(), lib.cpe_last_error()
            assert all((o == 7.0).all() for o in mo.values())

        add(b"G = 0 outside 1..16", G=0)
        add(b"G = 17 outside 1..16", G=17)
        add(b"negative", N=-1)
        add(b"frame count of sequence 0 outside 0..N", n_frames=i32(-1))
        add(b"frame count of sequence 0 outside 0..N", n_frames=i32(4))
        add(b"null argument", handle=None)
        for k in ("cov_s", "resp_u", "cov_diag", "cov_off", "cov_diag_m", "cov_off_m"):
            add(b"null argument", **{k: None})
        for k in ("resp_pos", "cov_pos", "cov_pos_m"):
            add(b"null together or given together", **{k: None})
    finally:
        h.close()


def test_zz_report():
    """the GPU's worst value per key next to its tolerance (for the record; asserts nothing new)"""
    for k in MC.KEYS:
        if k in WORST:
            print(f"  {k:8s} worst share of its tolerance {WORST[k][0]:.3f} (value {WORST[k][1]:.2e}, case {WORST[k][2]})")
