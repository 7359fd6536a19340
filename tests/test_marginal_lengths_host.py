"""The covariance marginalised over the fitted segment lengths without a device (DESIGN.md 2 "What is marginalised"): the reference's own spread
behind the tolerances of tests/test_gpu_scale_response.py, what the statement implies for the reference, the keyword's refusals, the C ABI's
argument lists, and the two calls estimator._posterior adds -- with a stub handle that records them, as tests/test_posterior_chain_host.py does."""
import ctypes as C
import inspect

import numpy as np
import pytest

import marginal_compare as MC
from cheetah_pose_estimation_amd import _lib, abi, estimator as E

NQ, NL, PB, G, RIDGE = 54, 24, 3, 11, 0.25
LENS = {False: (5, 5, 5), True: (5, 3, 4)}
OF = [1, 0, 1]
ANIMAL = [("a", False), ("b", False), ("a", False)]              # sequences 0 and 2 share their scales
SIGMA = [0.1, None, 0.1]
STATUS = [abi.OK, abi.OK, abi.NUMERICAL]                          # sequence 2 has no factor: it does not enter its animal's sum
TAILS = dict(cov_diag=(28, 28), cov_off=(PB, 28, 28), cov_pos=(NL, 3, 3), resp_u=(28, G), resp_pos=(NL, 3, G))


@pytest.mark.parametrize("name", ["n1", "plain"])
def test_tolerances_are_the_references_own_spread(oracle, name):
    """both measurements of marginal_compare's table re-made on two cases (the tightest and a typical one): within what is recorded for the
    case, which is what its tolerance is 32 times of; every case has its record"""
    m1, m2 = MC.measure_case(oracle, name, draws=1)
    print(name, {k: f"{m1[k]:.2e} / {m2[k]:.2e}" for k in MC.MEASURED_KEYS})
    tol = MC.tolerance(name)
    for k in MC.MEASURED_KEYS:
        assert tol[k] == MC.MARGIN * MC.MEASURED[name][k] > 0.0
        assert max(m1[k], m2[k]) <= 2.0 * MC.MEASURED[name][k], (k, m1[k], m2[k])          # (fewer draws than the table's: the same order)
    assert tol["sym"] == 0.0 and set(MC.MEASURED) == set(MC.CASES) and set(tol) == set(MC.KEYS)


def test_marginal_is_at_or_above_the_conditional(oracle):
    """the reference of case "plain": the marginal variances of coordinates and marker positions are not below the conditional ones, cov_s is
    (A_red + P)^-1, and the 25th marker -- no length dependence of its own -- still moves with the scales through the poses"""
    S = MC.case_reference(oracle, "plain")[0]
    assert np.all(np.einsum("nkk->nk", S["diag"]) >= np.einsum("nkk->nk", S["sigma_diag"]))
    assert np.all(np.einsum("nlaa->nla", S["cov_pos_m"]) >= np.einsum("nlaa->nla", S["cov_pos"]))
    Gn = S["cov_s"].shape[0]
    assert np.allclose(S["cov_s"] @ (S["A_red"] + np.eye(Gn) / MC.PRIOR_SIGMA ** 2), np.eye(Gn), atol=1e-9)
    assert np.abs(S["W"][:, 24]).max() > 0.0
    (mu, wu), (mp, wp) = MC.widening(S)
    print(f"plain: marginal / conditional std, median / worst: coordinates {mu:.3f} / {wu:.2f}, marker positions {mp:.3f} / {wp:.2f}")
    assert 1.0 <= mu <= wu and 1.0 <= mp <= wp


def test_keyword_and_its_refusals():
    """uncertainty_lengths sits before estimate_lengths on both fronts, defaults to False, and is refused before anything is looked at: without
    uncertainty=True, without estimate_lengths=True, and for a group whose estimators carry no fitted lengths"""
    for fn in (E.estimate_kinematics, E.estimate_kinematics_batch):
        p = inspect.signature(fn).parameters
        assert p["uncertainty_lengths"].default is False and list(p).index("uncertainty_lengths") == list(p).index("estimate_lengths") - 1
    assert "uncertainty_lengths" not in inspect.signature(E.estimate_kinetics).parameters
    assert list(inspect.signature(E.posterior_request).parameters)[-2:] == ["uncertainty_lengths", "estimate_lengths"]
    assert E.posterior_request(True, 0.5, False, None, 0, 0) == E.PosteriorRequest(0.5) and not E.PosteriorRequest(0.5).lengths
    assert E.posterior_request(True, 0.5, False, None, 0, 0, True, True) == E.PosteriorRequest(0.5, lengths=True)
    assert not E.PosteriorRequest(lengths=True).want_L
    for fn, first in ((E.estimate_kinematics, None), (E.estimate_kinematics_batch, [None])):
        with pytest.raises(ValueError, match="uncertainty_lengths=True needs uncertainty=True"):
            fn(first, estimate_lengths=True, uncertainty_lengths=True)
        with pytest.raises(ValueError, match="uncertainty_lengths=True needs estimate_lengths=True"):
            fn(first, uncertainty=True, uncertainty_lengths=True)
    bare = type("Est", (), dict(length_scale=None, length_calibration=None))()
    with pytest.raises(ValueError, match="has no fitted lengths"):
        E._length_group([bare], None)
    assert E.LENGTH_FIELDS == ("cov_u_marginal", "u_std_marginal", "positions_cov_marginal", "positions_std_marginal", "scale_cov", "u_scale_response",
                               "positions_scale_response")


def test_argument_lists_and_wrappers():
    """the four prototypes against abi.SCALE_RESPONSE_ENTRIES, the exported symbols and the wrappers (fails without the feature)"""
    _lib.build_library()
    lib = _lib.load()
    resp = ("h", "i", "i", "ip", "ip", "p", "p", "p", "d", "i", "p", "p", "p", "p", "p", "ip")
    add = ("h", "i", "i", "ip", "i") + ("p",) * 9
    assert abi.SCALE_RESPONSE_ENTRIES == {"cpe_scale_response": resp, "cpe_scale_response_host": resp, "cpe_covariance_add_scales": add,
                                          "cpe_covariance_add_scales_host": add}
    for name in abi.SCALE_RESPONSE_ENTRIES:
        assert abi.ENTRIES[name] == abi.SCALE_RESPONSE_ENTRIES[name] and list(getattr(lib, name).argtypes) == abi.argtypes(name)
    for m in ("scale_response", "scale_response_host", "covariance_add_scales", "covariance_add_scales_host"):
        assert callable(getattr(_lib.Handle, m))
    # the refusals that need no handle
    z = (C.c_double * 8)()
    p = C.cast(z, C.c_void_p)
    st = (C.c_int32 * 1)()
    for g in (0, 17):
        assert lib.cpe_scale_response_host(None, 1, 3, None, None, p, p, p, 0.0, g, p, p, p, p, p, st) == abi.BAD_ARG
        assert b"cpe_scale_response_host: G = " in lib.cpe_last_error()
        assert lib.cpe_covariance_add_scales(None, 1, 3, None, g, p, p, p, p, p, p, p, p, p) == abi.BAD_ARG
        assert b"cpe_covariance_add_scales: G = " in lib.cpe_last_error()
    assert lib.cpe_covariance_add_scales_host(None, 1, 3, (C.c_int32 * 1)(4), 2, p, p, p, p, p, p, p, p, p) == abi.BAD_ARG
    assert b"frame count of sequence 0 outside 0..N" in lib.cpe_last_error()
    assert lib.cpe_covariance_add_scales_host(None, 1, 3, None, 2, p, p, p, p, p, p, p, p, p) == abi.BAD_ARG and b"null argument" in lib.cpe_last_error()


class StubHandle:
    """records (name, args, kwargs) of every method called on it; the three methods of the chain return what _lib.Handle's return, in shape"""

    def __init__(self, lens, ragged):
        self.calls, self.lens, self.ragged, self.rng, self.A_red = [], lens, ragged, np.random.default_rng(3), None

    def _arrays(self, keys):
        B, Nm = len(self.lens), max(self.lens)
        padded = {k: self.rng.standard_normal((B, Nm) + TAILS[k]) for k in keys}
        if not self.ragged:
            return padded
        return dict({k: [np.ascontiguousarray(v[b, :n]) for b, n in enumerate(self.lens)] for k, v in padded.items()}, padded=padded)

    def __getattr__(self, name):
        def method(*a, **kw):
            self.calls.append((name, a, kw))
            B = len(self.lens)
            if name == "covariance_add_scales_host":
                return {k: self.rng.standard_normal(np.shape(a[3 + i])) for i, k in enumerate(("cov_diag", "cov_off", "cov_pos"))}
            if name == "scale_response_host":
                out = self._arrays(("resp_u", "resp_pos"))
                M = self.rng.standard_normal((B, G, G))
                self.A_red = np.einsum("bij,bkj->bik", M, M)
                out.update(A_red=self.A_red, status=abi.NUMERICAL, seq_status=list(STATUS), lens=list(self.lens))
                return out
            if name.startswith("covariance"):
                out = self._arrays(("cov_diag", "cov_off", "cov_pos"))
                for d in (out, out.get("padded", {})):
                    d["L"] = None
                out.update(status=abi.NUMERICAL, seq_status=list(STATUS))
                return out
            raise AssertionError(f"unexpected handle method {name}")
        return method


@pytest.mark.parametrize("ragged", [False, True])
def test_the_two_calls_of_the_length_step(ragged):
    lens = LENS[ragged]
    rng = np.random.default_rng(5)
    per = lambda *tail: [rng.standard_normal((n,) + tail) for n in lens]
    form = (lambda v: v) if ragged else np.stack
    q, meas, weight = form(per(NQ)), form(per(6, NL, 2)), form(per(6, NL))
    M = 2 if ragged else 1
    lg = dict(d_attach=rng.standard_normal((M, G, 17, 3)), d_marker_off=rng.standard_normal((M, G, NL, 3)), animal=ANIMAL, prior_sigma=SIGMA)
    of = OF if ragged else None
    # ---- nothing is called without the keyword
    h0 = StubHandle(lens, ragged)
    cov0 = E._posterior(h0, E.PosteriorRequest(ridge=RIDGE), None, q, E._Group((meas, weight), of, None, lg))
    assert [c[0] for c in h0.calls] == ["covariance_ragged_host" if ragged else "covariance_host"] and "lengths" not in cov0
    # ---- with it: the covariance call, then the two new ones, in that order
    h = StubHandle(lens, ragged)
    cov = E._posterior(h, E.PosteriorRequest(ridge=RIDGE, lengths=True), None, q, E._Group((meas, weight), of, None, lg))
    assert [c[0] for c in h.calls] == ["covariance_ragged_host" if ragged else "covariance_host", "scale_response_host", "covariance_add_scales_host"]
    _, a, kw = h.calls[1]
    assert a[0] is q and a[1] is meas and a[2] is weight and a[3] is lg["d_attach"] and a[4] is lg["d_marker_off"] and a[5] == RIDGE and len(a) == 6
    assert kw == (dict(model_list=OF) if ragged else {})
    src = cov["padded"] if ragged else cov
    _, a, kw = h.calls[2]
    cov_s, resp_u, resp_pos, cd, co, cp, n_frames = a
    assert kw == {} and cd is src["cov_diag"] and co is src["cov_off"] and cp is src["cov_pos"] and n_frames == (list(lens) if ragged else None)
    lgo = cov["lengths"]
    assert resp_u is lgo["resp_u"] and resp_pos is lgo["resp_pos"] and resp_u.shape == (3, max(lens), 28, G) and cov_s is lgo["cov_s"]
    # ---- cov_s: per animal, over its sequences that have a factor, in list order, with that animal's prior
    A_red = h.A_red
    assert np.array_equal(cov_s[0], np.linalg.inv(A_red[0] + np.eye(G) / 0.1 ** 2)) and np.array_equal(cov_s[2], cov_s[0])       # (2 has no factor)
    assert np.array_equal(cov_s[1], np.linalg.inv(A_red[1])) and cov_s.shape == (3, G, G)
    assert np.array_equal(cov_s[0], E.scale_covariance([A_red[0]], 0.1))
    # ---- what a sequence's est.uncertainty gains; none without a factor
    with np.errstate(invalid="ignore"):                               # (the stub's blocks are random: no square root of their diagonals)
        u = E._uncertainty_of(cov, 1, RIDGE)
    n = lens[1]
    assert set(E.LENGTH_FIELDS) <= set(u) and u["cov_u_marginal"].shape == (n, 28, 28) and u["positions_scale_response"].shape == (n, NL, 3, G)
    assert np.array_equal(u["cov_u_marginal"], lgo["cov_diag"][1, :n]) and np.array_equal(u["scale_cov"], cov_s[1])
    assert np.array_equal(u["cov_u"], cov["cov_diag"][1]) and E._uncertainty_of(cov, 2, RIDGE) is None


def test_scale_covariance_sums_in_list_order():
    rng = np.random.default_rng(1)
    A = [np.diag(rng.uniform(1.0, 2.0, 3)) * 10.0 ** k for k in (0, 8, -8)]
    assert np.array_equal(E.scale_covariance(A, 0.5), np.linalg.inv(((A[0] + A[1]) + A[2]) + np.eye(3) / 0.25))
    assert np.array_equal(E.scale_covariance(A[:1], None), np.linalg.inv(A[0]))
