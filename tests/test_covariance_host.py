"""Posterior covariance, the parts that need no GPU: the library's new symbols and their ctypes mirror, the refusals, the numpy reference
(tests/cov_compare.py) against itself on the oracle's band, and the inputs of the GPU's CPE_NUMERICAL test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cov_compare as CC
import lm_compare as LC
from cheetah_pose_estimation_amd import _lib, abi, priors

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "cpe.h")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def _prototypes():
    """{name: [argument declarations]} of every function declared in include/cpe.h"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\b(?:cpe_status|int32_t|void\*?|const char\*)\s+(cpe_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [" ".join(a.split()) for a in args.split(",") if a.split() and a.split() != ["void"]] for name, args in found}


def _prototype(name):
    """argument kinds of a prototype in include/cpe.h, in abi.COVARIANCE_ENTRIES' letters"""
    protos = _prototypes()
    assert name in protos, f"{name} is not declared in include/cpe.h"
    kinds = []
    for a in protos[name]:
        if "cpe_handle*" in a:
            kinds.append("h")
        elif "cpe_priors*" in a:
            kinds.append("pr")
        elif "double*" in a:
            kinds.append("p")
        elif "int32_t*" in a or "cpe_status*" in a:
            kinds.append("ip")
        elif a.startswith("int32_t "):
            kinds.append("i")
        elif a.startswith("double "):
            kinds.append("d")
        else:
            raise AssertionError((name, a))
    return tuple(kinds)


STRUCTS = {"cpe_skeleton": abi.Skeleton, "cpe_camera": abi.Camera, "cpe_options": abi.Options, "cpe_priors": abi.Priors, "cpe_stats": abi.Stats,
           "cpe_grf_options": abi.GrfOptions, "cpe_eom_options": abi.EomOptions, "cpe_dyn_options": abi.DynOptions,
           "cpe_kinetic_options": abi.KineticOptions, "cpe_kinetic_stats": abi.KineticStats}
SCALARS = {"int32_t": C.c_int32, "cpe_status": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def _ctypes_of(decl):
    """the ctypes types that may stand for one declared argument: a scalar is its own type; a pointer to a struct is a pointer to the struct's
    mirror; a pointer to numbers is a typed pointer or, where device memory may stand behind it, c_void_p; a handle or a stream is c_void_p"""
    m = re.fullmatch(r"(?:const )?(\w+)(\*{0,2}) \w+(\[\w*\])?", decl)
    assert m, decl
    base, stars = m.group(1), len(m.group(2)) + (1 if m.group(3) else 0)
    if base == "cpe_handle":
        return {1: [C.c_void_p], 2: [C.POINTER(C.c_void_p)]}[stars]
    if base == "void":
        assert stars == 1, decl
        return [C.c_void_p]
    if base in STRUCTS:
        assert stars == 1, decl
        return [C.POINTER(STRUCTS[base])]
    return [SCALARS[base]] if stars == 0 else [C.POINTER(SCALARS[base]), C.c_void_p]


def test_every_prototype_has_its_argument_list(lib):
    """abi.ENTRIES names every function include/cpe.h declares and nothing else, and the argtypes _lib.load() sets from it have every prototype's
    length and, argument by argument, its kind: a miscounted list fails here instead of handing C shifted arguments"""
    protos = _prototypes()
    assert len(protos) >= 56 and set(protos) == set(abi.ENTRIES)
    for name, decls in protos.items():
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None and len(argtypes) == len(decls), (name, len(argtypes or ()), len(decls))
        assert list(argtypes) == abi.argtypes(name), name
        for i, (t, decl) in enumerate(zip(argtypes, decls)):
            assert t in _ctypes_of(decl), (name, i, decl, t)
    assert lib.cpe_last_error.restype is C.c_char_p and lib.cpe_stream.restype is C.c_void_p


def test_symbols_and_ctypes_mirror(lib):
    """the library exports the covariance entry points and the ctypes mirror has their argument lists (fails without the feature)"""
    assert set(abi.COVARIANCE_ENTRIES) == {"cpe_covariance_supported", "cpe_band_inverse", "cpe_covariance", "cpe_covariance_host",
                                           "cpe_covariance_ragged", "cpe_covariance_ragged_host"}
    for name, kinds in abi.COVARIANCE_ENTRIES.items():
        fn = getattr(lib, name)                                   # AttributeError when the symbol is missing
        assert _prototype(name) == tuple(kinds), name
        assert list(fn.argtypes) == abi.covariance_argtypes(name), name
    for method in ("band_inverse", "covariance", "covariance_host", "covariance_ragged_host"):
        assert callable(getattr(_lib.Handle, method))
    assert C.sizeof(C.c_int32) == 4                               # cpe_status is int32_t: the status array of the mirror


def test_refusals(lib):
    """negative or non-finite ridge, and a motion prior of window 5 (half-bandwidth 5): CPE_BAD_ARG with the reason, before the device is opened;
    valid arguments get as far as the device"""
    for ridge in (-1e-9, float("nan"), float("inf")):
        assert lib.cpe_covariance_supported(None, ridge) == abi.BAD_ARG
        assert b"ridge" in lib.cpe_last_error()
        for name in ("cpe_covariance", "cpe_covariance_host"):
            assert getattr(lib, name)(None, 1, 4, None, None, None, ridge, None, None, None, None, None) == abi.BAD_ARG
            assert b"ridge" in lib.cpe_last_error()
        for name in ("cpe_covariance_ragged", "cpe_covariance_ragged_host"):
            one = (C.c_int32 * 1)(0)
            assert getattr(lib, name)(None, 1, 4, one, one, None, None, None, ridge, None, None, None, None, None) == abi.BAD_ARG
            assert b"ridge" in lib.cpe_last_error()
        with pytest.raises(_lib.CpeError, match="ridge"):
            _lib.covariance_supported(None, ridge)
    w5 = priors.load_priors(path=os.path.join(GOLDEN, "priors_k3_w5_dense.npz"))
    assert w5.lr_window == 5 and LC.solver_pb(w5) == 5 > abi.COVARIANCE_MAX_PB
    assert lib.cpe_covariance_supported(C.byref(w5), 0.0) == abi.BAD_ARG
    assert b"half-bandwidth 5" in lib.cpe_last_error()
    with pytest.raises(_lib.CpeError, match="half-bandwidth 5"):
        _lib.covariance_supported(w5, 1e-6)
    for pr in (None, priors.load_priors()):                        # none, and the packaged window-4 priors
        for ridge in (0.0, 1e-6):
            assert _lib.covariance_supported(pr, ridge) in (abi.OK, abi.NO_DEVICE)
    assert lib.cpe_covariance(None, 1, 4, None, None, None, 0.0, None, None, None, None, None) == abi.BAD_ARG     # (no handle)
    assert b"null" in lib.cpe_last_error()


# measured on the oracle's band at its own solution, ridge 0: 4.7e-11 and 2.4e-10 between the two routes; the bound leaves a
# factor 10 for another BLAS
ROUTES = {"six": 5e-10, "two": 2.5e-9}


@pytest.mark.parametrize("name", ["six", "two"])
def test_block_takahashi_equals_the_dense_inverse(oracle, name):
    c = CC.oracle_case(oracle, name)
    for ridge in (0.0, 1e-6):
        Ad = CC.damped(c["Bk"], ridge)
        R = CC.reference(Ad, c["Hk"])
        print(f"{name} ridge {ridge:g}: routes differ by {R['r_err']:.2e}, residual {R['r_res']:.2e}, scaled condition {R['cond']:.2e}, "
              f"tolerances {R['tol_err']:.2e} / {R['tol_res']:.2e}")
        assert R["r_err"] <= ROUTES[name]
        assert R["tol_err"] >= 10.0 * CC.EPS * R["cond"] and R["tol_res"] >= 10.0 * R["r_res"]
        L = CC.cholesky_layout(Ad, c["Hk"])
        d2, o2 = CC.takahashi(L)
        assert not CC.structure_failures(d2, o2, R["tol_err"])
        # the layout helpers agree with lm_compare's: L L^T gives the band back
        Md, Mk = LC.factor_product(L)
        sa = np.sqrt(np.diagonal(Ad, axis1=1, axis2=2))
        assert np.abs((Md - Ad) / (sa[:, :, None] * sa[:, None, :])).max() < 1e-12


def test_helper_on_random_bands():
    for PB, N in ((3, 1), (3, 4), (4, 2), (4, 9)):
        Ad, Hk = CC.random_band(N, PB, 7 * PB + N)
        R = CC.reference(Ad, Hk)
        assert R["r_err"] < 1e-11 and R["r_res"] < 1e-11 and 1.0 <= R["cond"] < 1e4
        assert not Hk[:1].any() and (N <= PB or Hk[PB, PB - 1].any())


def test_inputs_of_the_numerical_cases(oracle):
    """one camera without priors, and three frames at ridge 0, have no Cholesky factor; three frames at ridge 1e-3 have one"""
    c = CC.oracle_case(oracle, "mono_noprior")
    with pytest.raises(np.linalg.LinAlgError):
        CC.cholesky_layout(CC.damped(c["Bk"], 0.0), c["Hk"])
    n3 = CC.oracle_case(oracle, "n3")
    assert n3["q"].shape[0] == 3 and (np.diagonal(n3["Bk"], axis1=1, axis2=2) == 0.0).any()      # zero diagonal entries: no motion term
    with pytest.raises(np.linalg.LinAlgError):
        CC.cholesky_layout(CC.damped(n3["Bk"], 0.0), n3["Hk"])
    CC.cholesky_layout(CC.damped(n3["Bk"], 1e-3), n3["Hk"])
    mono = CC.oracle_case(oracle, "mono")
    assert mono["PB"] == 4
    CC.cholesky_layout(CC.damped(mono["Bk"], 0.0), mono["Hk"])


def test_monocular_depth_is_the_uncertain_direction(oracle):
    """the property the GPU test asserts of cov_pos, on the reference: mid-sequence, positions_std on the world axis of the line of sight exceeds
    both other components for every marker; the base's largest standard deviation there is decimetres"""
    from cheetah_pose_estimation_amd import synth
    c = CC.oracle_case(oracle, "mono")
    R = CC.reference(CC.damped(c["Bk"], 0.0), c["Hk"])
    n = c["q"].shape[0] // 2
    P = CC.marker_jacobians(oracle, c["sk"], c["q"], [n], 1e-6)
    std = np.sqrt(np.diagonal(CC.marker_covariance(P, R["diag"][[n]]), axis1=2, axis2=3))[0]
    pos = synth.fk_numpy(c["sk"], c["q"])[0][n]
    assert np.all(CC.depth_exceeds_transverse(c["cams"][0], pos, std))
    assert 0.1 < np.sqrt(np.diag(R["diag"][n])[:3]).max() < 1.0
