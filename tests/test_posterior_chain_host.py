"""The posterior chain of the estimator (estimator._posterior: covariance -> rates and point Jacobians -> columns -> band samples -> posterior samples
-> force samples) without a device: a stub handle records every method with its arguments and returns arrays of the right shapes.  B = 2
sequences, the second one without a factor (seq_status NUMERICAL), lengths (5, 5) plain and (5, 3) ragged, K = 2 draws.  The expected calls are
written out below, not derived from the chain: they are what every way of calling an estimate (single, plain batch, ragged batch; kinematic and
physics-based) must hand the library for a sequence's files to be bit-equal between them."""
import numpy as np
import pytest

from cheetah_pose_estimation_amd import abi, estimator as E

NQ, NL, PB, K, SEED, RIDGE = 54, 24, 3, 2, 11, 0.25
LENS = {False: (5, 5), True: (5, 3)}
OF = [1, 0]                                                    # the model of every sequence of the ragged group
SPANS = {False: [[(0, 4), (1, 3), (2, 4)], [(0, 2)]], True: [[(0, 4), (1, 3), (2, 4)], [(0, 2)]]}
REQUESTS = dict(cov=dict(), rates=dict(rates=True), spans=dict(spans=True), samples=dict(samples=K, seed=SEED),
                all=dict(rates=True, spans=True, samples=K, seed=SEED))
RATE_WANT = ("cov_du", "cov_ddu", "cov_vel", "cov_com", "cov_com_vel")
TAILS = dict(cov_diag=(28, 28), cov_off=(PB, 28, 28), cov_pos=(NL, 3, 3), L=(PB + 1, 28, 28), cov_f=(64, 64), f=(64,), meta=(65,),
             cov_du=(28, 28), cov_ddu=(28, 28), cov_vel=(NL, 3, 3), cov_com=(3, 3), cov_com_vel=(3, 3), jac_pos=(NL, 3, 28), jac_com=(3, 28))

# the ordered handle methods of every case: (physics, ragged) -> request -> names
_kin = lambda form: dict(cov=["covariance" + form], rates=["covariance" + form, "rate_covariance" + form],
                         spans=["covariance" + form, "rate_covariance" + form, "covariance_columns_host"],
                         samples=["covariance" + form, "band_sample_host", "posterior_samples_host"],
                         all=["covariance" + form, "rate_covariance" + form, "covariance_columns_host", "band_sample_host", "posterior_samples_host"])
EXPECTED = {(False, False): _kin("_host"), (False, True): _kin("_ragged_host")}
for _ragged, _form in ((False, "_host"), (True, "_ragged_host")):
    EXPECTED[(True, _ragged)] = {k: ["covariance_kinetic" + _form] + v[1:] + (["force_samples" + _form] if k in ("samples", "all") else [])
                                 for k, v in _kin(_form).items()}
assert EXPECTED[(True, True)]["all"] == ["covariance_kinetic_ragged_host", "rate_covariance_ragged_host", "covariance_columns_host", "band_sample_host",
                                         "posterior_samples_host", "force_samples_ragged_host"]


class StubHandle:
    """records (name, args, kwargs) of every method called on it; every *_host method returns what _lib.Handle's returns, in shape"""

    def __init__(self, lens, ragged):
        self.calls, self.lens, self.ragged, self.rng = [], lens, ragged, np.random.default_rng(3)

    def _arrays(self, keys, lead=()):
        B, Nm = len(self.lens), max(self.lens)
        padded = {k: self.rng.standard_normal((B,) + lead + (Nm,) + TAILS[k]) for k in keys}
        if not self.ragged:
            return padded
        cut = lambda v: [np.ascontiguousarray(v[b, :n]) for b, n in enumerate(self.lens)]
        return dict({k: cut(v) for k, v in padded.items()}, padded=padded)

    def __getattr__(self, name):
        def method(*a, **kw):
            self.calls.append((name, a, kw))
            B, Nm = len(self.lens), max(self.lens)
            if name.startswith("covariance_columns"):
                return self.rng.standard_normal((B, np.shape(a[3])[1], Nm, 28, 28))
            if name.startswith("covariance"):
                keys = ("cov_diag", "cov_off", "cov_pos") + (("L",) if kw["want_L"] else ()) + (("cov_f", "f", "meta") if "kinetic" in name else ())
                out = self._arrays(keys)
                for d in (out, out.get("padded", {})):
                    d.setdefault("L", None)
                out.update(status=abi.NUMERICAL, seq_status=[abi.OK, abi.NUMERICAL])
                return out
            if name.startswith("rate_covariance"):
                return self._arrays(kw["want"])
            if name == "band_sample_host":
                return self.rng.standard_normal((B, K, Nm, 28))
            if name == "posterior_samples_host":
                n = lambda b: self.lens[b]
                if self.ragged:
                    return dict(q=[np.zeros((K, n(b), NQ)) for b in range(B)], positions=[np.zeros((K, n(b), NL, 3)) for b in range(B)])
                return dict(q=np.zeros((B, K, Nm, NQ)), positions=np.zeros((B, K, Nm, NL, 3)))
            if name.startswith("force_samples"):
                out = dict(f_s=self.rng.standard_normal((B, K, Nm, 64)), f=self.rng.standard_normal((B, Nm, 64)))
                return dict(padded=out) if self.ragged else out
            raise AssertionError(f"unexpected handle method {name}")
        return method


def _group(physics, ragged, lens):
    """(q, the group description, the covariance call's own arguments after q) of B = 2 sequences"""
    rng = np.random.default_rng(5)
    per = lambda *tail: [rng.standard_normal((n,) + tail) for n in lens]
    form = (lambda v: v) if ragged else np.stack
    q, meas, weight = form(per(NQ)), form(per(6, NL, 2)), form(per(6, NL))
    if not physics:
        return q, E._Group((meas, weight), OF if ragged else None), (meas, weight)
    stance = form([np.ones((n, 4), np.int32) for n in lens])
    ko = [object(), object()] if ragged else object()
    force = dict(tau_box=form(per(22, 2)))
    return q, E._Group((meas, weight, stance, ko), OF if ragged else None, force), (meas, weight, stance, ko)


def _same(a, b):
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a is b or (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and np.array_equal(a, b))


@pytest.mark.parametrize("which", list(REQUESTS))
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("physics", [False, True])
def test_calls_and_arguments(physics, ragged, which):
    lens = LENS[ragged]
    req = E.PosteriorRequest(ridge=RIDGE, **REQUESTS[which])
    spans = SPANS[ragged] if req.spans is not None else None
    h = StubHandle(lens, ragged)
    q, group, args = _group(physics, ragged, lens)
    cov = E._posterior(h, req, spans, q, group)
    models = (OF,) if ragged else ()
    # ---- the calls, in order -------------------------------------------------------------------------------------------------------------------
    assert [c[0] for c in h.calls] == EXPECTED[(physics, ragged)][which]
    calls = {c[0]: c for c in h.calls}
    # ---- the covariance call: its arguments, and want_L exactly when spans or samples are asked for -------------------------------------------
    _, a, kw = h.calls[0]
    assert len(a) == 1 + len(args) + len(models) + 1 and a[0] is q and all(x is y for x, y in zip(a[1:], args + models)) and a[-1] == RIDGE
    assert kw.pop("want_L") is req.want_L is (which in ("spans", "samples", "all"))
    assert set(kw) == ({"tau_box"} if physics else set()) and all(kw[k] is group.force[k] for k in kw)
    # ---- the rate call: want, and the covariance call's own band -----------------------------------------------------------------------------
    rate = calls.get("rate_covariance_ragged_host" if ragged else "rate_covariance_host")
    if which in ("rates", "spans", "all"):
        want = (RATE_WANT if req.rates else ()) + (("jac_pos", "jac_com") if spans is not None else ())
        assert rate[2] == dict(want=want) and E._RATE_WANT == RATE_WANT
        assert rate[1][0] is q and rate[1][1] is cov["cov_diag"] and rate[1][2] is cov["cov_off"] and rate[1][3:] == models
        assert ("rates" in cov) == req.rates and (not req.rates or set(cov["rates"]) - {"padded"} == set(want))
    else:
        assert rate is None and "rates" not in cov
    src = cov["padded"] if ragged else cov
    # ---- the columns call: no anchor for the sequence without a factor ----------------------------------------------------------------------
    if spans is not None:
        L, cd, co, anchors, n_frames = calls["covariance_columns_host"][1]
        assert L is src["L"] and L is not None and cd is src["cov_diag"] and co is src["cov_off"]
        assert anchors.dtype == np.int32 and anchors.tolist() == [[3, 4], [-1, -1]]
        assert n_frames == (list(lens) if ragged else None)
        assert cov["spans"]["spans"] is spans and cov["spans"]["anchors"] is anchors
    else:
        assert "covariance_columns_host" not in calls and "spans" not in cov
    # ---- the draws -----------------------------------------------------------------------------------------------------------------------------
    if req.samples:
        L, z, counts = calls["band_sample_host"][1]
        assert L is src["L"] and L is not None and counts == [5, 0]
        assert z.shape == (2, K, max(lens), abi.NX)
        for b, n in enumerate(lens):
            assert np.array_equal(z[b, :, :n], E.sample_normals(SEED, K, n)) and not z[b, :, n:].any()
        du = cov["samples"]["du"]
        ps = calls["posterior_samples_host"][1]
        if ragged:
            assert _same(ps[0], list(q)) and ps[2] == OF and all(np.array_equal(ps[1][b], du[b, :, :n]) for b, n in enumerate(lens))
        else:
            assert ps[0] is q and ps[1] is du and len(ps) == 2
        assert cov["samples"]["lens"] == list(lens) and cov["samples"]["seed"] == SEED
        fs = calls.get("force_samples_ragged_host" if ragged else "force_samples_host")
        if physics:
            a, kw = fs[1], fs[2]
            # the covariance call's own q / meas / weight / stance / options, then du, zeta, (models,) ridge, and its variant array
            assert a[0] is q and all(x is y for x, y in zip(a[1:5], args)) and a[-1] == RIDGE and a[7:-1] == models
            assert set(kw) == {"tau_box"} and kw["tau_box"] is group.force["tau_box"]
            zeta = a[6]
            for b, n in enumerate(lens):
                zb, db = (zeta[b], a[5][b]) if ragged else (zeta[b, :, :n], a[5][b, :, :n])
                assert np.array_equal(zb, E.sample_force_normals(SEED, K, n)) and np.array_equal(db, du[b, :, :n])
                assert ragged or not zeta[b, :, n:].any()
            assert cov["samples"]["f_s"].shape == (2, K, max(lens), 64) and cov["samples"]["f"].shape == (2, max(lens), 64)
        else:
            assert fs is None and "f_s" not in cov["samples"]
    else:
        assert "band_sample_host" not in calls and "samples" not in cov


def test_request_from_the_public_keywords():
    """posterior_request: None for uncertainty=False; the refusals in their order, with their messages; want_L; spans_for = resolve_spans"""
    assert E.posterior_request(False, 0.0, False, None, 0, 0) is None
    r = E.posterior_request(True, 0.5, True, [(0, -1)], 3, 9)
    assert r == E.PosteriorRequest(0.5, True, [(0, -1)], 3, 9) and r.want_L and r.spans_for(6) == [(0, 5)] == E.resolve_spans([(0, -1)], 6)
    for kw, want_L in ((dict(), False), (dict(rates=True), False), (dict(spans=True), True), (dict(samples=1), True)):
        assert E.PosteriorRequest(**kw).want_L is want_L
    with pytest.raises(ValueError, match="uncertainty_samples must be >= 0, not -1"):
        E.posterior_request(False, 0.0, True, True, -1, 0)
    with pytest.raises(ValueError, match="uncertainty_samples needs uncertainty=True"):
        E.posterior_request(False, 0.0, True, True, 2, 0)
    with pytest.raises(ValueError, match="uncertainty_rates=True needs uncertainty=True"):
        E.posterior_request(False, 0.0, True, True, 0, 0)
    with pytest.raises(ValueError, match="uncertainty_spans needs uncertainty=True"):
        E.posterior_request(False, 0.0, False, True, 0, 0)
    with pytest.raises(Exception):
        r.ridge = 1.0                                              # frozen
