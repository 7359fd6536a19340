"""Loader + thin ctypes binding of libcpe.so (the HIP / C-ABI product library, include/cpe.h).

There is NO CPU fallback: if the library is missing, or no MI355X is visible, every call fails loudly.
Torch is used only as plumbing for device memory (tensor.data_ptr()).
"""
import ctypes as C
import os
import subprocess
from typing import Optional

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcpe.so")
_CSRC = os.path.join(_HERE, "csrc")
_LIB = None
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)


class CpeError(RuntimeError):
    pass


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into libcpe.so (in-tree).  hipcc cross-compiles without a GPU."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC)] + [os.path.join(_HERE, "..", "include", "cpe.h")]
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", LIB_PATH,
           os.path.join(_CSRC, "cpe_api.hip")]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise CpeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the solve path)")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7; it must be resident before
    # libcpe.so resolves the same soname, otherwise two runtimes fight over the device.
    import torch  # noqa: F401
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        C.CDLL(tl, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_PATH)
    for name in abi.ENTRIES:
        getattr(lib, name).argtypes = abi.argtypes(name)
    lib.cpe_last_error.restype = C.c_char_p
    lib.cpe_stream.restype = C.c_void_p
    lib.cpe_default_kinetic_options.restype = lib.cpe_default_track_weights.restype = None
    _LIB = lib
    return lib


def _check(status: int, what: str, allow=(abi.OK,)):
    if status not in allow:
        raise CpeError(f"{what} failed with status {status}: {load().cpe_last_error().decode()}")
    return status


def covariance_supported(priors: Optional[abi.Priors], ridge: float) -> int:
    """cpe_covariance_supported: what the covariance entries refuse, without a handle.  Returns the status (abi.OK, abi.NO_DEVICE where no GPU
    is visible); raises CpeError with the library's reason on abi.BAD_ARG (negative or non-finite ridge, motion-prior window above 4)."""
    st = load().cpe_covariance_supported(C.byref(priors) if priors is not None else None, float(ridge))
    return _check(st, "cpe_covariance_supported", allow=(abi.OK, abi.NO_DEVICE))


def shape_signature(sk: abi.Skeleton) -> bytes:
    """The part of a skeleton that models of one cpe_create_multi handle must share (include/cpe.h): link tree, markers' links, joints, bound pairs
    and the relative-angle convention.  Link geometry, masses, marker offsets, bound limits and motion weights may differ."""
    nl, L, nj, nb = sk.n_links, sk.n_markers, sk.n_joints, sk.n_bounds
    nq = 3 + 3 * nl
    parts = [np.array([nl, L, nj, nb], np.int32), np.ctypeslib.as_array(sk.parent)[:nl], np.ctypeslib.as_array(sk.marker_link)[:L],
             np.ctypeslib.as_array(sk.joint_parent)[:nj], np.ctypeslib.as_array(sk.joint_child)[:nj], np.ctypeslib.as_array(sk.joint_kind)[:nj],
             np.ctypeslib.as_array(sk.bound_a)[:nb], np.ctypeslib.as_array(sk.bound_b)[:nb], np.ctypeslib.as_array(sk.rel_ref)[:nq],
             np.ctypeslib.as_array(sk.rel_sign)[:nq]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


SHARED_OPTIONS = ("lambda0", "tol_step", "tol_cost", "max_iter", "max_outer", "curvature", "bound_tol", "cost_scale")


def shared_options_signature(opts: abi.Options) -> tuple:
    """The options the models of one cpe_create_multi handle must share (the LM driver reads them per batch)"""
    return tuple(getattr(opts, k) for k in SHARED_OPTIONS)


def kinetic_shape_signature(ko: abi.KineticOptions) -> tuple:
    """The kinetic option fields the models of one cpe_solve_kinetic_ragged call must share (include/cpe.h): feet, their markers, motors and
    their link pairs and axes.  Every other field may differ per model."""
    d = ko.dyn
    nf, nm = int(d.n_feet), int(d.n_motors)
    return (nf, tuple(d.foot_marker[:max(min(nf, 4), 0)]), nm, tuple(d.motor_first[:max(nm, 0)]), tuple(d.motor_second[:max(nm, 0)]),
            tuple(d.motor_axis[:max(nm, 0)]))


def _pad(arrs, n_max: int, tail) -> np.ndarray:
    """per-sequence arrays [N_b, *shape_b] -> [B, n_max, *tail], zero-filled past each sequence's own frames (and, on every axis, its own extent)"""
    out = np.zeros((len(arrs), n_max) + tuple(tail), dtype=np.result_type(*[np.asarray(a).dtype for a in arrs]) if arrs else np.float64)
    for b, a in enumerate(arrs):
        a = np.asarray(a)
        out[(b,) + tuple(slice(0, k) for k in a.shape)] = a
    return out


KINETIC_INPUTS = ("q_init", "meas", "weight", "stance", "force")
KINETIC_OUTPUTS = ("q", "dq", "ddq", "positions", "meas_err", "tau", "lam", "grf", "slack")
FORCE_VARIANTS = ("grf_fixed", "tau_box", "grf_box")
CAMS = "cameras"     # in a per-frame shape: the camera count -- of the sequence's model where shapes are checked, the handle's largest where arrays are padded


def _force_variant(who: str, grf_fixed, tau_box, grf_box, message: Optional[str] = None):
    """(name, array) of the one force array given -- the variant of a physics-based solve -- or (None, None); more than one is a ValueError"""
    given = [(k, a) for k, a in zip(FORCE_VARIANTS, (grf_fixed, tau_box, grf_box)) if a is not None]
    if len(given) > 1:
        raise ValueError(message or f"{who}: at most one of grf_fixed, tau_box, grf_box")
    return given[0] if given else (None, None)


def pad_kinetic(q_init_list, meas_list=None, weight_list=None, stance_list=None, force_list=None, n_cams_max: Optional[int] = None,
                q_target_list=None) -> dict:
    """The inputs of cpe_solve_kinetic_ragged_host from per-sequence arrays: q_init [N_b, nq], meas [N_b, C_b, L, 2], weight [N_b, C_b, L],
    stance [N_b, n_feet], force (grf_fixed / tau_box / grf_box of the sequence, or None) -> zero-padded [B, N_max, ...] arrays (C_max cameras,
    n_cams_max or the largest C_b).  An absent list gives None; q_target [N_b, nq] is padded as q_init is and listed only when given.  Pure numpy."""
    lens = [int(np.shape(q)[0]) for q in q_init_list]
    nmax = max(lens) if lens else 0

    def pad(arrs, tail=None, dtype=np.float64):
        return None if arrs is None else _pad([np.asarray(a, dtype) for a in arrs], nmax, np.shape(arrs[0])[1:] if tail is None else tail)
    out = dict(lens=lens, q_init=pad(q_init_list), meas=None, weight=None, stance=pad(stance_list, dtype=np.int32), force=pad(force_list))
    if meas_list is not None:
        cm = n_cams_max if n_cams_max is not None else max(int(np.shape(m)[1]) for m in meas_list)
        L = int(np.shape(meas_list[0])[2])
        out.update(meas=pad(meas_list, (cm, L, 2)), weight=pad(weight_list, (cm, L)))
    if q_target_list is not None:
        out["q_target"] = pad(q_target_list, np.shape(q_init_list[0])[1:])
    return out


def pad_kinetic_tracked(q_init_list, q_target_list, stance_list, meas_list=None, weight_list=None, force_list=None,
                        n_cams_max: Optional[int] = None) -> dict:
    """pad_kinetic for cpe_solve_kinetic_tracked_ragged_host: q_target [N_b, nq] is padded as q_init is; meas / weight may be None together (then
    the result's meas and weight are None).  Pure numpy."""
    if (meas_list is None) != (weight_list is None):
        raise ValueError("pad_kinetic_tracked: meas and weight are given together or not at all")
    if [int(np.shape(t)[0]) for t in q_target_list] != [int(np.shape(q)[0]) for q in q_init_list]:
        raise ValueError("pad_kinetic_tracked: every q_target has its q_init's frames")
    return pad_kinetic(q_init_list, meas_list, weight_list, stance_list, force_list, n_cams_max, q_target_list)


def pad_track_W(track_W_list, lens=None) -> np.ndarray:
    """The track_W of cpe_solve_kinetic_tracked_weighted_ragged_host from per-sequence arrays [N_b, NX, NX]: zero-padded [B, N_max, NX, NX] float64
    (lens: the frame counts they must have, e.g. pad_kinetic_tracked's; None = their own).  Pure numpy."""
    arrs = [np.asarray(w, dtype=np.float64) for w in track_W_list]
    if any(w.ndim != 3 or w.shape[1:] != (abi.NX, abi.NX) for w in arrs):
        raise ValueError(f"pad_track_W: every track_W is [N_b, {abi.NX}, {abi.NX}]")
    if lens is not None and [w.shape[0] for w in arrs] != [int(n) for n in lens]:
        raise ValueError("pad_track_W: every track_W has its q_init's frames")
    return _pad(arrs, max([w.shape[0] for w in arrs], default=0), (abi.NX, abi.NX))


def track_weights(track_w, rows: int) -> np.ndarray:
    """[rows, NX] float64 weights of the 3D kinematic cost: None = the reference's (abi.default_track_weights) for every row, one NX vector =
    the same for every row, or one row per model"""
    w = abi.default_track_weights() if track_w is None else np.asarray(track_w, dtype=np.float64)
    if w.ndim == 1:
        w = np.broadcast_to(w, (rows, w.shape[0]))
    if w.shape != (rows, abi.NX):
        raise ValueError(f"track weights: expected {abi.NX} entries per model ({rows} models), got shape {w.shape}")
    return np.ascontiguousarray(w, dtype=np.float64)


def unpad_kinetic(padded: dict, lens, n_cams) -> dict:
    """The per-sequence outputs of a padded ragged result: every array of `padded` [B, N_max, ...] -> list of [N_b, ...] (meas_err also cut to
    the sequence's n_cams[b] cameras); an output that is None stays None.  Pure numpy."""
    cut = lambda k, a, b: a[b, :lens[b], :n_cams[b]] if k == "meas_err" else a[b, :lens[b]]
    return {k: None if a is None else [np.ascontiguousarray(cut(k, a, b)) for b in range(len(lens))] for k, a in padded.items()}


def _ptr(t):
    """device pointer of a torch tensor / host pointer of a numpy array / None"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.dtype == np.float64 and t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    assert t.is_contiguous() and ((t.dtype.is_floating_point and t.element_size() == 8) or str(t.dtype) == "torch.int32")
    return t.data_ptr()


def _force_slots(variant, array) -> list:
    """the grf_fixed, tau_box, grf_box pointer arguments of an entry: `array` in its variant's place, null in the others"""
    return [_ptr(array) if variant == k else None for k in FORCE_VARIANTS]


def _f64(a, optional: bool = False):
    """a as a C-contiguous float64 array; optional: None stays None (an argument the entry may take as null)"""
    return None if optional and a is None else np.ascontiguousarray(a, dtype=np.float64)


def _int32s(B: int, values=()):
    """the c_int32 array of a call over B sequences: their model indices or frame counts, or (no values) room for their statuses"""
    return (C.c_int32 * max(B, 1))(*[int(v) for v in values])


class Handle:
    """One solver instance = one skeleton + one camera rig + options, bound to one GPU and one HIP stream.
    Stands where the reference builds its Pyomo model (acinoset_opt.py:459-525)."""

    def __init__(self, sk: abi.Skeleton, cams, opts: abi.Options = None, priors: abi.Priors = None, device: int = 0):
        self.lib = load()
        opts = opts if opts is not None else abi.default_options()
        self._h = C.c_void_p()
        st = self.lib.cpe_create(C.byref(sk), cams, len(cams), C.byref(opts), C.byref(priors) if priors is not None else None, device,
                                 C.byref(self._h))
        self._created(st, "cpe_create", sk, cams, opts, [len(cams)], priors, device)

    @classmethod
    def multi(cls, skels, cams_list, opts_list=None, priors: abi.Priors = None, device: int = 0) -> "Handle":
        """One handle over several models of the same shape (cpe_create_multi): model k = (skels[k], cams_list[k], opts_list[k]).  Its
        solve_ragged_host solves sequences of any of them, each with its own length, in one call."""
        n = len(skels)
        if n < 1 or len(cams_list) != n or (opts_list is not None and len(opts_list) != n):
            raise ValueError("Handle.multi: one camera list and one options struct per skeleton")
        opts_list = list(opts_list) if opts_list is not None else [abi.default_options() for _ in range(n)]
        sks = (abi.Skeleton * n)(*skels)
        cams = (abi.Camera * (n * abi.MAX_CAMS))()
        for k, cl in enumerate(cams_list):
            for c, cam in enumerate(cl):
                cams[k * abi.MAX_CAMS + c] = cam
        ncam = (C.c_int32 * n)(*[len(cl) for cl in cams_list])
        ops = (abi.Options * n)(*opts_list)
        self = cls.__new__(cls)
        self.lib = load()
        self._h = C.c_void_p()
        st = self.lib.cpe_create_multi(n, sks, cams, ncam, ops, C.byref(priors) if priors is not None else None, device, C.byref(self._h))
        self._created(st, "cpe_create_multi", skels[0], cams_list[0], opts_list[0], list(ncam), priors, device)
        return self

    def _created(self, st, what, sk, cams, opts, model_n_cams, priors, device):
        """the tail of both constructors: refuse a failed create, then what the methods read -- the first model's skeleton, cameras and options,
        the camera count of every model and the largest of them"""
        if st == abi.NO_DEVICE:
            raise CpeError("no HIP device visible: the solve path has no CPU fallback (" + self.lib.cpe_last_error().decode() + ")")
        _check(st, what)
        self.sk, self.cams, self.opts = sk, cams, opts
        self.model_n_cams, self.n_cams = model_n_cams, max(model_n_cams)
        self.device = device
        self.pb = max(3, priors.lr_window) if priors is not None else 3     # half-bandwidth of the solver's band in frames
        self.S = self.lib.cpe_jacobian_slots(self._h)
        self.nu = self.lib.cpe_num_independent(self._h)
        self.nq, self.L = sk.nq, sk.n_markers

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.cpe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return self.lib.cpe_stream(self._h)

    def synchronize(self):
        _check(self.lib.cpe_synchronize(self._h), "cpe_synchronize")

    # The device-pointer entry points enqueue on the handle's own stream (include/cpe.h, "Synchronisation contract").  Torch
    # tensors are produced and consumed on torch's current stream, so every device-pointer method below brackets its call:
    # the handle first waits for what torch has queued, and torch's stream afterwards waits for what the handle has queued.
    def _torch_stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _enter(self):
        _check(self.lib.cpe_stream_wait(self._h, self._torch_stream()), "cpe_stream_wait")

    def _leave(self):
        _check(self.lib.cpe_stream_signal(self._h, self._torch_stream()), "cpe_stream_signal")

    def _call(self, fn, what, *args, allow=(abi.OK,)):
        """fn(handle, *args) bracketed by _enter / _leave (also when it fails); returns its status, raises unless it is in `allow`"""
        self._enter()
        try:
            st = fn(self._h, *args)
        finally:
            self._leave()
        return _check(st, what, allow)

    # staging of numpy arrays for the *_host methods
    def _to_device(self, a, dtype=np.float64):
        import torch
        return torch.tensor(np.ascontiguousarray(a, dtype=dtype), device=torch.device("cuda", self.device))

    def _empty(self, *shape):
        import torch
        return torch.empty(shape, dtype=torch.float64, device=torch.device("cuda", self.device))

    PROFILE_SLOTS = ("k_frame_normal", "k_lr_band", "k_lm_step", "k_build_act", "k_finalize", "k_dyn_eval", "k_dyn_gather", "k_lm_back",
                     "k_dyn_assemble", "k_dyn_schur", "k_dyn_jac", "_free11")

    def profile(self, on: bool):
        _check(self.lib.cpe_profile_enable(self._h, 1 if on else 0), "cpe_profile_enable")

    def profile_totals(self):
        """{kernel: (milliseconds, launches)} accumulated by the solves since profile(True)"""
        ms = (C.c_double * len(self.PROFILE_SLOTS))(); n = (C.c_int64 * len(self.PROFILE_SLOTS))()
        _check(self.lib.cpe_profile_get(self._h, ms, n), "cpe_profile_get")
        return {k: (ms[i], int(n[i])) for i, k in enumerate(self.PROFILE_SLOTS) if n[i]}

    def jacobian_layout(self):
        sm = np.empty(self.S, dtype=np.int32); sd = np.empty(self.S, dtype=np.int32)
        _check(self.lib.cpe_jacobian_layout(self._h, sm.ctypes.data_as(ip), sd.ctypes.data_as(ip)), "cpe_jacobian_layout")
        return sm, sd

    def independent_dofs(self):
        d = np.empty(self.nu, dtype=np.int32)
        _check(self.lib.cpe_independent_dofs(self._h, d.ctypes.data_as(ip)), "cpe_independent_dofs")
        return d

    # ---- device-pointer entry points (torch-ROCm tensors on self.device) -------------------------------
    def eval_resjac(self, q, meas, weight, r, J, eps, cost=None):
        self._call(self.lib.cpe_eval_resjac, "cpe_eval_resjac", q.shape[0], q.shape[1], _ptr(q), _ptr(meas), _ptr(weight), _ptr(r), _ptr(J),
                   _ptr(eps), _ptr(cost))

    def project_joints(self, q):
        return self._call(self.lib.cpe_project_joints, "cpe_project_joints", q.shape[0], q.shape[1], _ptr(q), allow=(abi.OK, abi.NUMERICAL))

    def forward_kinematics(self, q, positions, com=None):
        self._call(self.lib.cpe_forward_kinematics, "cpe_forward_kinematics", q.shape[0], q.shape[1], _ptr(q), _ptr(positions), _ptr(com))

    def marker_velocities(self, q, dq, velocities):
        """v_l = (d p_l / d q) dq for every marker (device tensors; velocities [B, N, L, 3])"""
        self._call(self.lib.cpe_marker_velocities, "cpe_marker_velocities", q.shape[0], q.shape[1], _ptr(q), _ptr(dq), _ptr(velocities))

    def reproject(self, positions, uv):
        """stored 3D markers -> pixels in every camera (device tensors; uv [B, N, C, L, 2])"""
        self._call(self.lib.cpe_reproject, "cpe_reproject", positions.shape[0], positions.shape[1], _ptr(positions), _ptr(uv))

    def reproject_host(self, positions):
        """numpy [B, N, L, 3] -> numpy [B, N, C, L, 2] (staged through HBM with torch)"""
        pd = self._to_device(positions)
        uv = self._empty(pd.shape[0], pd.shape[1], self.n_cams, self.L, 2)
        self.reproject(pd, uv)
        self.synchronize()
        return uv.cpu().numpy()

    def detection_report(self, positions, cov_pos, uv, cov_px, meas=None, weight=None, weight_fit=None, uv_loo=None, cov_loo=None, d2=None,
                         leverage=None):
        """cpe_detection_report on device tensors: positions [B, N, L, 3], cov_pos [B, N, L, 3, 3] (covariance()'s) -> uv [B, N, C, L, 2], cov_px
        [B, N, C, L, 3] = (xx, xy, yy); with meas [B, N, C, L, 2] and weight [B, N, C, L] (weight_fit: the weights of the fit, None = weight) also
        uv_loo, cov_loo, d2 [B, N, C, L], leverage, each of which may be None"""
        self._call(self.lib.cpe_detection_report, "cpe_detection_report", positions.shape[0], positions.shape[1], _ptr(positions), _ptr(cov_pos),
                   _ptr(meas), _ptr(weight), _ptr(weight_fit), _ptr(uv), _ptr(cov_px), _ptr(uv_loo), _ptr(cov_loo), _ptr(d2), _ptr(leverage))

    def detection_report_host(self, positions, cov_pos, meas=None, weight=None, weight_fit=None):
        """cpe_detection_report_host: numpy in, dict of numpy arrays out -- uv, cov_px [B, N, C, L, 2, 2] and, with meas and weight, uv_loo, cov_loo
        [.., 2, 2], d2, leverage"""
        positions, cov_pos = _f64(positions), _f64(cov_pos)
        meas, weight, weight_fit = _f64(meas, True), _f64(weight, True), _f64(weight_fit, True)
        B, N = positions.shape[:2]
        pair = (B, N, self.n_cams, self.L)
        raw = dict(uv=np.empty(pair + (2,)), cov_px=np.empty(pair + (3,)))
        if meas is not None or weight is not None:
            raw.update(uv_loo=np.empty(pair + (2,)), cov_loo=np.empty(pair + (3,)), d2=np.empty(pair), leverage=np.empty(pair))
        _check(self.lib.cpe_detection_report_host(self._h, B, N, _ptr(positions), _ptr(cov_pos), _ptr(meas), _ptr(weight), _ptr(weight_fit),
                                                  *[_ptr(raw.get(k)) for k in abi.DETECTION_OUTPUTS]), "cpe_detection_report_host")
        for k in ("cov_px", "cov_loo"):
            if k in raw:
                raw[k] = raw[k][..., [0, 1, 1, 2]].reshape(pair + (2, 2))
        return raw

    def triangulate_host(self, cam_a, cam_b, uv_a, uv_b, depth=3.0):
        """n detection pairs -> xyz [n, 3] (cpe_triangulate; cam_b < 0: back-projection of uv_a to `depth`); numpy in / out"""
        ca, cb = self._to_device(cam_a, np.int32), self._to_device(cam_b, np.int32)
        ua = self._to_device(np.reshape(uv_a, (-1, 2)))
        ub = self._to_device(np.reshape(uv_b, (-1, 2)))
        n = int(ca.shape[0])
        if not (cb.shape[0] == n and ua.shape[0] == n and ub.shape[0] == n):
            raise CpeError("triangulate_host: array lengths differ")
        xyz = self._empty(n, 3)
        self._call(self.lib.cpe_triangulate, "cpe_triangulate", n, _ptr(ca), _ptr(cb), _ptr(ua), _ptr(ub), float(depth), _ptr(xyz))
        self.synchronize()
        return xyz.cpu().numpy()

    def tensorise_dlc_host(self, tables, first_rows, part_of_marker, inv_sigma, thresh, N):
        """per-camera DLC tables (numpy [rows, 3*parts]) -> meas [N, C, L, 2], weight [N, C, L] (numpy) through cpe_tensorise_dlc"""
        Cn = len(tables)
        meas, weight = self._empty(N, Cn, self.L, 2), self._empty(N, Cn, self.L)
        pm, isg = self._to_device(part_of_marker, np.int32), self._to_device(inv_sigma)
        if pm.shape[0] != self.L or isg.shape[0] != self.L:
            raise CpeError("tensorise_dlc_host: one body part and one sigma per marker of the handle")
        for c, tab in enumerate(tables):
            t = self._to_device(tab)
            if t.dim() != 2 or t.shape[1] % 3:
                raise CpeError("tensorise_dlc_host: a DLC table has 3 columns per body part")
            self._call(self.lib.cpe_tensorise_dlc, "cpe_tensorise_dlc", N, Cn, c, _ptr(t), int(t.shape[0]), int(t.shape[1] // 3), int(first_rows[c]),
                       _ptr(pm), _ptr(isg), float(thresh), _ptr(meas), _ptr(weight))
            self.synchronize()                      # `t` must outlive the launch
        return meas.cpu().numpy(), weight.cpu().numpy()

    def kinematics_host(self, q, dq):
        """numpy in, numpy out (staged through HBM with torch): positions [B, N, L, 3], marker velocities [B, N, L, 3]"""
        qd, dqd = self._to_device(q), self._to_device(dq)
        B, N = qd.shape[0], qd.shape[1]
        pos, vel = self._empty(B, N, self.L, 3), self._empty(B, N, self.L, 3)
        self.forward_kinematics(qd, pos, None)
        self.marker_velocities(qd, dqd, vel)
        self.synchronize()
        return pos.cpu().numpy(), vel.cpu().numpy()

    def eval_normal(self, q, meas, weight, g, Bm, cost, gam=None, q_out=None):
        self._call(self.lib.cpe_eval_normal, "cpe_eval_normal", q.shape[0], q.shape[1], _ptr(q), _ptr(meas), _ptr(weight), _ptr(g), _ptr(Bm),
                   _ptr(cost), _ptr(gam), _ptr(q_out))

    def solve(self, q_init, meas, weight, q, dq, ddq, positions, meas_err):
        B, N = q_init.shape[0], q_init.shape[1]
        stats = (abi.Stats * max(B, 1))()
        st = self._call(self.lib.cpe_solve, "cpe_solve", B, N, _ptr(q_init), _ptr(meas), _ptr(weight), _ptr(q), _ptr(dq), _ptr(ddq),
                        _ptr(positions), _ptr(meas_err), stats, allow=(abi.OK, abi.MAX_ITER, abi.NUMERICAL))
        return st, list(stats)[:B]

    def solve_ragged(self, model, n_frames, q_init, meas, weight, q, dq, ddq, positions, meas_err):
        """cpe_solve_ragged on device tensors laid out for N_max = q_init.shape[1] frames and C_max cameras; model / n_frames: int sequences
        (one per sequence).  Returns (status, [Stats])."""
        B, N = q_init.shape[0], q_init.shape[1]
        stats = (abi.Stats * max(B, 1))()
        mo, nf = _int32s(B, model), _int32s(B, n_frames)
        st = self._call(self.lib.cpe_solve_ragged, "cpe_solve_ragged", B, N, mo, nf, _ptr(q_init), _ptr(meas), _ptr(weight), _ptr(q), _ptr(dq),
                        _ptr(ddq), _ptr(positions), _ptr(meas_err), stats, allow=(abi.OK, abi.MAX_ITER, abi.NUMERICAL))
        return st, list(stats)[:B]

    def solve_shutter(self, q_init, meas, weight, tau_bound, q, dq, ddq, positions, meas_err, tau, max_rounds=8, tol_tau=1e-6):
        """trajectory + per-camera shutter delays (acinoset_misc.py:283-285); device tensors, tau [B, C]"""
        B, N = q_init.shape[0], q_init.shape[1]
        stats = (abi.Stats * max(B, 1))()
        rounds = C.c_int32(0)
        st = self._call(self.lib.cpe_solve_shutter, "cpe_solve_shutter", B, N, _ptr(q_init), _ptr(meas), _ptr(weight), float(tau_bound),
                        int(max_rounds), float(tol_tau), _ptr(q), _ptr(dq), _ptr(ddq), _ptr(positions), _ptr(meas_err), _ptr(tau), stats,
                        C.byref(rounds), allow=(abi.OK, abi.MAX_ITER, abi.NUMERICAL))
        return st, list(stats)[:B], rounds.value

    def solve_shutter_host(self, q_init, meas, weight, tau_bound, max_rounds=8, tol_tau=1e-6):
        """numpy in, numpy out (staged through HBM with torch)"""
        E = self._empty
        qi, me, we = self._to_device(q_init), self._to_device(meas), self._to_device(weight)
        B, N, nq = qi.shape
        q, dq, ddq = E(B, N, nq), E(B, N, nq), E(B, N, nq)
        pos, err, tau = E(B, N, self.L, 3), E(B, N, self.n_cams, self.L, 2), E(B, self.n_cams)
        st, stats, rounds = self.solve_shutter(qi, me, we, tau_bound, q, dq, ddq, pos, err, tau, max_rounds, tol_tau)
        self.synchronize()
        return dict(status=st, q=q.cpu().numpy(), dq=dq.cpu().numpy(), ddq=ddq.cpu().numpy(), positions=pos.cpu().numpy(),
                    meas_err=err.cpu().numpy(), tau=tau.cpu().numpy(), stats=stats, rounds=rounds)

    def eom_rows(self, eopt, q, dq, ddq, rows):
        """all rows of d/dt dL/dq' - dL/dq (device tensors [B, N, nq])"""
        self._call(self.lib.cpe_eom_rows, "cpe_eom_rows", C.byref(eopt), q.shape[0], q.shape[1], _ptr(q), _ptr(dq), _ptr(ddq), _ptr(rows))

    def eom_residual(self, dopt, q, dq, ddq, tau, lam, grf, residual):
        """rows of the equations of motion minus the generalised forces (device tensors; tau / lam / grf may be None)"""
        self._call(self.lib.cpe_eom_residual, "cpe_eom_residual", C.byref(dopt), q.shape[0], q.shape[1], _ptr(q), _ptr(dq), _ptr(ddq), _ptr(tau),
                   _ptr(lam), _ptr(grf), _ptr(residual))

    def grf_fit(self, gopt, q, dq, ddq, contact, grfz, grfxy, residual=None):
        """per-frame ground-reaction-force fit (device tensors); contact int32 [B, N, n_feet]"""
        self._call(self.lib.cpe_grf_fit, "cpe_grf_fit", C.byref(gopt), q.shape[0], q.shape[1], _ptr(q), _ptr(dq), _ptr(ddq), _ptr(contact),
                   _ptr(grfz), _ptr(grfxy), _ptr(residual))

    def grf_fit_host(self, gopt, q, dq, ddq, contact):
        """numpy in, numpy out (staged through HBM with torch): grfz [B, N, nf], grfxy [B, N, nf, 4], residual [B, N, 6]"""
        qd, dqd, ddqd, cd = self._to_device(q), self._to_device(dq), self._to_device(ddq), self._to_device(contact, np.int32)
        B, N, nf = qd.shape[0], qd.shape[1], gopt.n_feet
        gz, gxy, res = self._empty(B, N, nf), self._empty(B, N, nf, 4), self._empty(B, N, 6)
        self.grf_fit(gopt, qd, dqd, ddqd, cd, gz, gxy, res)
        self.synchronize()
        return gz.cpu().numpy(), gxy.cpu().numpy(), res.cpu().numpy()

    # ---- physics-based trajectory model (config 4) -------------------------------------------------------
    def solve_kinetic(self, kopts, q_init, meas, weight, stance, q, dq, ddq, positions, meas_err, tau=None, lam=None, grf=None, slack=None, grf_fixed=None, tau_box=None, grf_box=None):
        """device tensors (stance int32 [B, N, n_feet]; at most one of: grf_fixed [B, N, n_feet, 3] = prescribed net foot forces, tau_box [B, N, n_motors, 2] =
        (lower, upper) bound of every torque, grf_box [B, N, n_feet, 3, 2] = (lower, upper) of the net (z, x, y) foot forces); returns (status, [Stats], [KineticStats])"""
        variant, force = _force_variant("solve_kinetic", grf_fixed, tau_box, grf_box,
                                        "prescribed foot forces, torque boxes and force boxes are separate entry points")
        entry = {"tau_box": "cpe_solve_kinetic_bounded", "grf_box": "cpe_solve_kinetic_force_box"}.get(variant, "cpe_solve_kinetic_fixed")
        return self._solve_kinetic_entry(entry, C.byref(kopts), (), (), [q_init, meas, weight], stance, [_ptr(force)],
                                         [q, dq, ddq, positions, meas_err, tau, lam, grf, slack], what="cpe_solve_kinetic")

    def _solve_kinetic_entry(self, entry, ko, track, ragged, arrays, stance, forces, outputs, what=None):
        """The one argument list of the physics-based solves, whatever the entry (all ten wrappers end here): ko (the kinetic options by
        reference, or the array of a ragged entry), track (nothing, or for the 3D kinematic cost the one array track_w / track_W: held here, so
        that it outlives the call), B, N, ragged (model, n_frames, or nothing), arrays (q_init, [q_target], meas, weight), stance, forces (the
        entry's force slots, as pointers), the nine outputs in KINETIC_OUTPUTS' order, stats.  A *_host entry takes host pointers and is called
        directly; any other takes device tensors and goes through _call (stream bracketing; `what` names it in an error, default the entry).
        Returns (status, [Stats], [KineticStats]); raises CpeError unless the status is OK, MAX_ITER or NUMERICAL."""
        host = entry.endswith("_host")
        B, N = arrays[0].shape[0], arrays[0].shape[1]
        stats = (abi.Stats * max(B, 1))(); ks = (abi.KineticStats * max(B, 1))()
        args = [ko, *[_ptr(t) for t in track], B, N, *ragged, *[_ptr(a) for a in arrays], stance.ctypes.data if host else _ptr(stance), *forces,
                *[_ptr(a) for a in outputs], stats, ks]
        fn, allow = getattr(self.lib, entry), (abi.OK, abi.MAX_ITER, abi.NUMERICAL)
        st = _check(fn(self._h, *args), entry, allow) if host else self._call(fn, what or entry, *args, allow=allow)
        return st, list(stats)[:B], list(ks)[:B]

    def n_constraint_rows(self):
        return sum(2 if self.sk.joint_kind[j] == abi.JOINT_REVOLUTE_Y else 1 for j in range(self.sk.n_joints))

    def solve_kinetic_host(self, kopts, q_init, meas, weight, stance, grf_fixed=None, tau_box=None, grf_box=None):
        """numpy in, numpy out (staged through HBM with torch)"""
        T = self._to_device
        qi, me, we, stn = T(q_init), T(meas), T(weight), T(stance, np.int32)
        gfx, tbx, gbx = (None if a is None else T(a) for a in (grf_fixed, tau_box, grf_box))
        B, N = qi.shape[0], qi.shape[1]
        out = self._solve_outputs(B, N, kopts, alloc=lambda shape: self._empty(*shape))
        st, stats, ks = self.solve_kinetic(kopts, qi, me, we, stn, *[out[k] for k in KINETIC_OUTPUTS], grf_fixed=gfx, tau_box=tbx, grf_box=gbx)
        self.synchronize()
        return dict(status=st, **{k: t.cpu().numpy() for k, t in out.items()}, stats=stats, kstats=ks)

    def _solve_outputs(self, B, N, kopts=None, meas_err=True, alloc=np.empty) -> dict:
        """The outputs of a solve, [B, N, ...] each, unwritten, keyed as KINETIC_OUTPUTS: the kinematic solve's five, and with kinetic options the
        physics-based solve's nine; meas_err is None where it is not wanted"""
        nq, L = self.nq, self.L
        tails = dict(q=(nq,), dq=(nq,), ddq=(nq,), positions=(L, 3), meas_err=(self.n_cams, L, 2))
        if kopts is not None:
            tails.update(tau=(kopts.dyn.n_motors,), lam=(self.n_constraint_rows(),), grf=(kopts.dyn.n_feet, 5), slack=(nq,))
        return {k: alloc((B, N) + t) if meas_err or k != "meas_err" else None for k, t in tails.items()}

    def _kinetic_options_array(self, kopts_list):
        n = len(self.model_n_cams)
        kl = list(kopts_list)
        if len(kl) != n:
            raise ValueError(f"solve_kinetic_ragged: one kinetic options struct per model of the handle ({n}), got {len(kl)}")
        return (abi.KineticOptions * n)(*kl)

    def solve_kinetic_ragged(self, kopts_list, model, n_frames, q_init, meas, weight, stance, q, dq, ddq, positions, meas_err, tau=None, lam=None,
                             grf=None, slack=None, grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_solve_kinetic_ragged on device tensors laid out for N_max = q_init.shape[1] frames and C_max cameras; kopts_list: one
        KineticOptions per model of the handle; model / n_frames: int sequences (one per sequence); at most one of grf_fixed / tau_box / grf_box
        (the variant of the whole batch).  Returns (status, [Stats], [KineticStats])."""
        forces = _force_slots(*_force_variant("solve_kinetic_ragged", grf_fixed, tau_box, grf_box))
        ko = self._kinetic_options_array(kopts_list)
        B = q_init.shape[0]
        if len(model) != B or len(n_frames) != B:
            raise ValueError("solve_kinetic_ragged: one model index and one frame count per sequence")
        return self._solve_kinetic_entry("cpe_solve_kinetic_ragged", ko, (), [_int32s(B, model), _int32s(B, n_frames)], [q_init, meas, weight], stance, forces,
                                         [q, dq, ddq, positions, meas_err, tau, lam, grf, slack])

    def solve_kinetic_ragged_host(self, kopts_list, q_init_list, meas_list, weight_list, stance_list, model_list=None, grf_fixed=None, tau_box=None,
                                  grf_box=None):
        """cpe_solve_kinetic_ragged_host over sequences of their own length and model: per sequence q_init [N_b, nq], meas [N_b, C_m, L, 2],
        weight [N_b, C_m, L], stance [N_b, n_feet] (C_m = the camera count of its model, model_list[b]; None = model 0 for all); at most one of
        grf_fixed / tau_box / grf_box, each a list of one array per sequence ([N_b, n_feet, 3] / [N_b, n_motors, 2] / [N_b, n_feet, 3, 2]).
        Pads, solves, unpads: returns dict(status, q, dq, ddq, positions, meas_err, tau, lam, grf, slack = lists of per-sequence arrays, stats,
        kstats = lists, padded = the padded outputs)."""
        return self._solve_kinetic_ragged_host("cpe_solve_kinetic_ragged_host", "one q_init, meas, weight, stance, model (and force array)", kopts_list,
                                               model_list, (grf_fixed, tau_box, grf_box), q_init=q_init_list, meas=meas_list, weight=weight_list,
                                               stance=stance_list)

    def _solve_kinetic_host_entry(self, entry, kopts, ko, track, ragged, p, variant):
        """What every pointer-host form of the physics-based solve ends with.  p: its converted (ragged: padded) inputs under pad_kinetic's names,
        a q_target only for the 3D kinematic cost; kopts: the options that size the outputs; ko, track, ragged: as _solve_kinetic_entry takes them.
        Allocates the outputs (no meas_err without meas) and calls.  Returns them, [B, N, ...] each, and dict(status, stats, kstats)."""
        B, N = p["q_init"].shape[:2]
        out = self._solve_outputs(B, N, kopts, meas_err=p["meas"] is not None)
        st, stats, ks = self._solve_kinetic_entry(entry, ko, track, ragged, [p[k] for k in ("q_init", "q_target", "meas", "weight") if k in p], p["stance"],
                                                  _force_slots(variant, p["force"]), [out[k] for k in KINETIC_OUTPUTS])
        return out, dict(status=st, stats=stats, kstats=ks)

    def _solve_kinetic_ragged_host(self, entry, each, kopts_list, model_list, forces, track=None, **lists):
        """The three ragged pointer-host forms: force variant, _ragged_batch's checks and padding of `lists` (each: how its error names them), the
        entry, unpadding.  track(p): the track_w / track_W array of an entry of the 3D kinematic cost, made from the padded batch p."""
        who = entry[len("cpe_"):]
        variant, force = _force_variant(who, *forces)
        p = self._ragged_batch(who, each, model_list, kopts_list, variant, **lists, force=force)
        ko, track = self._kinetic_options_array(kopts_list), [] if track is None else [track(p)]
        out, tail = self._solve_kinetic_host_entry(entry, kopts_list[0], ko, track, [p["model_arr"], p["len_arr"]], p, variant)
        res = unpad_kinetic(out, p["lens"], p["cams"])
        res.update(tail, padded=out)
        return res

    def _ragged_batch(self, who, each, model_list, kopts_list=None, variant=None, **lists) -> dict:
        """The checks and the padding that every ragged *_host method starts with.  lists: the per-sequence arrays under pad_kinetic's names
        (q_init gives the lengths; None = absent); each: how the error names them; kopts_list / variant: the kinetic options of the models and
        the name of the force array, for the physics-based solves.  Raises ValueError, in this order, for: not one array per sequence, not one
        kinetic options struct per model, a model index out of range, a sequence without the shapes of its model.  Returns pad_kinetic's dict
        (pad_kinetic_tracked's with a q_target) plus models, cams (the camera count of every sequence) and the c_int32 arrays model_arr,
        len_arr."""
        B = len(lists["q_init"])
        models = [0] * B if model_list is None else [int(m) for m in model_list]
        ncams = self.model_n_cams
        # weight is looked at with meas only: alone, it is for pad_kinetic_tracked to refuse
        seen = {k: v for k, v in lists.items() if v is not None and (k != "weight" or lists.get("meas") is not None)}
        if any(len(v) != B for v in seen.values()) or len(models) != B or ("meas" in seen and "weight" not in seen):
            raise ValueError(f"{who}: {each} per sequence")
        if kopts_list is not None and len(kopts_list) != len(ncams):
            raise ValueError(f"{who}: one kinetic options struct per model of the handle ({len(ncams)}), got {len(kopts_list)}")
        if any(m < 0 or m >= len(ncams) for m in models):
            raise ValueError(f"{who}: model index out of range")
        nq, L = self.nq, self.L
        tails = dict(q_init=(nq,), q_target=(nq,), meas=(CAMS, L, 2), weight=(CAMS, L))
        if kopts_list is not None:
            nf, nm = int(kopts_list[0].dyn.n_feet), int(kopts_list[0].dyn.n_motors)
            tails.update(stance=(nf,), force=dict(grf_fixed=(nf, 3), tau_box=(nm, 2), grf_box=(nf, 3, 2)).get(variant))
        for b in range(B):
            n, c = int(np.shape(lists["q_init"][b])[0]), ncams[models[b]]
            if any(np.shape(v[b]) != (n,) + tuple(c if t == CAMS else t for t in tails[k]) for k, v in seen.items()):
                raise ValueError(f"{who}: sequence {b} does not have the shapes of its model ({n} frames, {c} cameras)")
        pad = pad_kinetic_tracked if "q_target" in lists else pad_kinetic
        p = pad(n_cams_max=self.n_cams, **{k + "_list": v for k, v in lists.items()})
        p.update(models=models, cams=[ncams[m] for m in models], model_arr=_int32s(B, models), len_arr=_int32s(B, p["lens"]))
        return p

    # ---- physics-based solve with the 3D kinematic cost (estimate_kinetics(use_2d_reprojections=False); include/cpe.h) ----------------------
    def solve_kinetic_tracked(self, kopts, q_init, q_target, stance, q, dq, ddq, positions, meas=None, weight=None, meas_err=None, tau=None, lam=None,
                              grf=None, slack=None, grf_fixed=None, tau_box=None, grf_box=None, track_w=None):
        """cpe_solve_kinetic_tracked on device tensors (q_target [B, N, nq]; meas / weight may be None together, meas_err is then not written);
        track_w: None (the reference's weights) or NX numbers (host).  Returns (status, [Stats], [KineticStats])"""
        forces = _force_slots(*_force_variant("solve_kinetic_tracked", grf_fixed, tau_box, grf_box))
        return self._solve_kinetic_entry("cpe_solve_kinetic_tracked", C.byref(kopts), [track_weights(track_w, 1)], (),
                                         [q_init, q_target, meas, weight], stance, forces, [q, dq, ddq, positions, meas_err, tau, lam, grf, slack])

    def _solve_kinetic_tracked_host(self, entry, kopts, track, q_init, q_target, stance, meas, weight, forces):
        """The two plain pointer-host forms of the 3D kinematic cost: force variant, meas and weight together, conversion, q_target's shape, then
        track(p) -> the entry's track_w / track_W array with its own checks made, the entry, solve_kinetic_host's dict.  A null q_init fails
        here; a null q_target goes to the library, which refuses it."""
        who = entry[len("cpe_"):]
        variant, force = _force_variant(who, *forces)
        if (meas is None) != (weight is None):
            raise ValueError(f"{who}: meas and weight are given together or not at all")
        p = {k: _f64(a, optional=True) for k, a in (("q_init", q_init), ("q_target", q_target), ("meas", meas), ("weight", weight), ("force", force))}
        p["stance"] = np.ascontiguousarray(stance, dtype=np.int32)
        if p["q_target"] is not None and p["q_target"].shape != p["q_init"].shape:
            raise ValueError(f"{who}: q_target has q_init's shape")
        out, tail = self._solve_kinetic_host_entry(entry, kopts, C.byref(kopts), [track(p)], (), p, variant)
        out.update(tail)
        return out

    def solve_kinetic_tracked_host(self, kopts, q_init, q_target, stance, meas=None, weight=None, grf_fixed=None, tau_box=None, grf_box=None,
                                   track_w=None):
        """cpe_solve_kinetic_tracked_host: numpy in, numpy out -- solve_kinetic_host's dict (meas_err None when meas is None)"""
        return self._solve_kinetic_tracked_host("cpe_solve_kinetic_tracked_host", kopts, lambda p: track_weights(track_w, 1), q_init, q_target, stance,
                                                meas, weight, (grf_fixed, tau_box, grf_box))

    def solve_kinetic_tracked_ragged_host(self, kopts_list, q_init_list, q_target_list, stance_list, meas_list=None, weight_list=None, model_list=None,
                                          grf_fixed=None, tau_box=None, grf_box=None, track_w=None):
        """cpe_solve_kinetic_tracked_ragged_host over sequences of their own length and model (solve_kinetic_ragged_host's arguments and result,
        plus q_target [N_b, nq] per sequence; meas_list / weight_list may be None together, meas_err is then None); track_w: None, NX numbers
        for every model, or [n_models, NX]"""
        return self._solve_kinetic_ragged_host("cpe_solve_kinetic_tracked_ragged_host", "one q_init, q_target, stance, model (and meas, weight, force array)",
                                               kopts_list, model_list, (grf_fixed, tau_box, grf_box), lambda p: track_weights(track_w, len(self.model_n_cams)),
                                               q_init=q_init_list, q_target=q_target_list, stance=stance_list, meas=meas_list, weight=weight_list)

    # ---- the 3D kinematic cost with the kinematic posterior as its weights (estimate_kinetics(track_weights="posterior"); include/cpe.h) --------
    def track_precision(self, cov_diag, W, scale=1.0, model=None, n_frames=None):
        """cpe_track_precision on device tensors: W [B, N, NX, NX] = (scale / 2) (X Sigma X^T)^-1 of every frame's block of cov_diag [B, N, NX, NX];
        model / n_frames: int sequences of a ragged batch (frames past a sequence's own are not written), or None.  A block without a Cholesky
        factor raises CpeError naming the sequence and the frame (its W is zero, the others are written)."""
        B, N = cov_diag.shape[0], cov_diag.shape[1]
        if (model is None) != (n_frames is None):
            raise ValueError("track_precision: model and n_frames are given together or not at all")
        mo = nf = None
        if model is not None:
            if len(model) != B or len(n_frames) != B:
                raise ValueError("track_precision: one model index and one frame count per sequence")
            mo, nf = _int32s(B, model), _int32s(B, n_frames)
        self._call(self.lib.cpe_track_precision, "cpe_track_precision", B, N, mo, nf, _ptr(cov_diag), float(scale), _ptr(W))

    def track_precision_host(self, cov_diag, scale=1.0, model_list=None):
        """cpe_track_precision_host: cov_diag [B, N, NX, NX] numpy -> W [B, N, NX, NX]; or, for sequences of their own length (and model,
        model_list; None = model 0), a list of [N_b, NX, NX] -> a list of W [N_b, NX, NX] from ONE call.  Raises CpeError as track_precision."""
        ragged = isinstance(cov_diag, (list, tuple))
        if ragged:
            lens = [int(np.shape(c)[0]) for c in cov_diag]
            models = [0] * len(lens) if model_list is None else [int(m) for m in model_list]
            if len(models) != len(lens):
                raise ValueError("track_precision_host: one model index per sequence")
            cd = pad_track_W(cov_diag)
            mo, nf = _int32s(len(lens), models), _int32s(len(lens), lens)
        else:
            cd = _f64(cov_diag)
            if cd.ndim != 4 or cd.shape[2:] != (abi.NX, abi.NX):
                raise ValueError(f"track_precision_host: cov_diag is [B, N, {abi.NX}, {abi.NX}]")
            mo = nf = None
        W = np.zeros_like(cd)
        st = self.lib.cpe_track_precision_host(self._h, cd.shape[0], cd.shape[1], mo, nf, _ptr(cd), float(scale), _ptr(W))
        _check(st, "cpe_track_precision_host")
        return [np.ascontiguousarray(W[b, :n]) for b, n in enumerate(lens)] if ragged else W

    def solve_kinetic_tracked_weighted(self, kopts, track_W, q_init, q_target, stance, q, dq, ddq, positions, meas=None, weight=None, meas_err=None,
                                       tau=None, lam=None, grf=None, slack=None, grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_solve_kinetic_tracked_weighted on device tensors: solve_kinetic_tracked with track_W [B, N, NX, NX] (symmetric, positive
        semi-definite: the caller's contract) in place of track_w.  Returns (status, [Stats], [KineticStats])"""
        forces = _force_slots(*_force_variant("solve_kinetic_tracked_weighted", grf_fixed, tau_box, grf_box))
        return self._solve_kinetic_entry("cpe_solve_kinetic_tracked_weighted", C.byref(kopts), [track_W], (), [q_init, q_target, meas, weight], stance,
                                         forces, [q, dq, ddq, positions, meas_err, tau, lam, grf, slack])

    def solve_kinetic_tracked_weighted_host(self, kopts, track_W, q_init, q_target, stance, meas=None, weight=None, grf_fixed=None, tau_box=None,
                                            grf_box=None):
        """cpe_solve_kinetic_tracked_weighted_host: numpy in, numpy out -- solve_kinetic_tracked_host's arguments and dict with track_W
        [B, N, NX, NX] in place of track_w"""
        who = "solve_kinetic_tracked_weighted_host"

        def track(p):
            W = _f64(track_W, optional=True)
            if W is not None and W.shape != p["q_init"].shape[:2] + (abi.NX, abi.NX):
                raise ValueError(f"{who}: track_W is [B, N, {abi.NX}, {abi.NX}]")
            return W
        return self._solve_kinetic_tracked_host("cpe_" + who, kopts, track, q_init, q_target, stance, meas, weight,
                                                (grf_fixed, tau_box, grf_box))

    def solve_kinetic_tracked_weighted_ragged_host(self, kopts_list, track_W_list, q_init_list, q_target_list, stance_list, meas_list=None,
                                                   weight_list=None, model_list=None, grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_solve_kinetic_tracked_weighted_ragged_host: solve_kinetic_tracked_ragged_host's arguments and result with one track_W
        [N_b, NX, NX] per sequence in place of track_w"""
        who, each = "solve_kinetic_tracked_weighted_ragged_host", "one q_init, q_target, track_W, stance, model (and meas, weight, force array)"

        def track(p):                                   # after _ragged_batch: the count, then the frames of every track_W
            if len(track_W_list) != len(p["lens"]):
                raise ValueError(f"{who}: {each} per sequence")
            return pad_track_W(track_W_list, p["lens"])
        return self._solve_kinetic_ragged_host("cpe_" + who, each, kopts_list, model_list, (grf_fixed, tau_box, grf_box),
                                               track, q_init=q_init_list, q_target=q_target_list, stance=stance_list, meas=meas_list, weight=weight_list)

    def eval_normal_tracked(self, q, q_target, g, Bm, cost, track_w=None, gam=None, q_out=None, track_W=None):
        """cpe_eval_normal_tracked on device tensors: the per-frame terms of the tracked solve (T_n, bounds, pose prior) at Euler q; track_W
        [B, N, NX, NX] (device tensor): the full-weight form instead (cpe_eval_normal_tracked_weighted; not together with track_w)"""
        if track_W is not None:
            if track_w is not None:
                raise ValueError("eval_normal_tracked: track_w or track_W, not both")
            self._call(self.lib.cpe_eval_normal_tracked_weighted, "cpe_eval_normal_tracked_weighted", _ptr(track_W), q.shape[0], q.shape[1], _ptr(q),
                       _ptr(q_target), _ptr(g), _ptr(Bm), _ptr(cost), _ptr(gam), _ptr(q_out))
            return
        w = track_weights(track_w, 1)
        self._call(self.lib.cpe_eval_normal_tracked, "cpe_eval_normal_tracked", w.ctypes.data, q.shape[0], q.shape[1], _ptr(q), _ptr(q_target), _ptr(g),
                   _ptr(Bm), _ptr(cost), _ptr(gam), _ptr(q_out))

    def eval_kinetic_nodes_host(self, kopts, q, meas, weight, stance):
        """one evaluation of the physics terms per node (cpe_eval_kinetic_nodes); numpy in, dict of numpy arrays out"""
        return self.eval_kinetic_system_host(kopts, q, meas, weight, stance, band=False)

    def eval_kinetic_system_host(self, kopts, q, meas, weight, stance, grf_fixed=None, tau_box=None, grf_box=None, band=True):
        """cpe_eval_kinetic_system: the per-node outputs of eval_kinetic_nodes_host and (band) the band system at the handle's lambda0 --
        gk [B, N, 28], Bk [B, N, 28, 28], Hk [B, N, 2, 28, 28]; grf_fixed / tau_box / grf_box (at most one) in solve_kinetic_host's layouts"""
        import torch
        T, E = self._to_device, self._empty
        qd, me, we, stn = T(q), T(meas), T(weight), T(stance, np.int32)
        var = [None if a is None else T(a) for a in (grf_fixed, tau_box, grf_box)]
        B, N = qd.shape[0], qd.shape[1]
        out = dict(f=E(B, N, 64), stat=E(B, N, 8), g=E(B, N, 84), Huu=E(B, N, 84, 84), Hfu=E(B, N, 64, 84), Hff=E(B, N, 64, 64))
        if band:
            out.update(gk=E(B, N, 28), Bk=E(B, N, 28, 28), Hk=E(B, N, 2, 28, 28))
        meta = torch.empty((B, N, 65), dtype=torch.int32, device=qd.device)
        self._call(self.lib.cpe_eval_kinetic_system, "cpe_eval_kinetic_system", C.byref(kopts), B, N, _ptr(qd), _ptr(me), _ptr(we), _ptr(stn),
                   *[_ptr(v) for v in var], _ptr(out["f"]), _ptr(out["stat"]), _ptr(out["g"]), _ptr(out["Huu"]), _ptr(out["Hfu"]), _ptr(out["Hff"]),
                   _ptr(meta), _ptr(out.get("gk")), _ptr(out.get("Bk")), _ptr(out.get("Hk")))
        self.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res["meta"] = meta.cpu().numpy()
        return res

    def eval_lm_step_host(self, q, meas, weight, lam, kopts=None, stance=None):
        """cpe_eval_lm_step: the first LM iteration of a solve from Euler q at damping lam -- the kinematic model, or with kopts and stance the
        physics-based one.  numpy in, dict of numpy arrays out: g, dg, delta [B, N, 28], L [B, N, pb + 1, 28, 28] (block [n][i] = block
        (n + i, n) of the lower Cholesky factor), state [B, N, 2, ns] (current, trial), seq [B, 8] (cost terms meas, model, bound, pose, motion;
        pred, maxstep, status)"""
        import torch
        T, E = self._to_device, self._empty
        qd, me, we = T(q), T(meas), T(weight)
        stn = None if stance is None else T(stance, np.int32)
        B, N = qd.shape[0], qd.shape[1]
        ns = self.nq + sum(1 for j in range(self.sk.n_joints) if self.sk.joint_kind[j] == abi.JOINT_REVOLUTE_Y)
        out = dict(g=E(B, N, 28), dg=E(B, N, 28), L=E(B, N, self.pb + 1, 28, 28), delta=E(B, N, 28), state=E(B, N, 2, ns))
        seq = np.zeros((B, 8))
        self._call(self.lib.cpe_eval_lm_step, "cpe_eval_lm_step", C.byref(kopts) if kopts is not None else None, B, N, _ptr(qd), _ptr(me), _ptr(we),
                   _ptr(stn), float(lam), _ptr(out["g"]), _ptr(out["dg"]), _ptr(out["L"]), _ptr(out["delta"]), _ptr(out["state"]), _ptr(seq))
        self.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res["seq"] = seq
        return res

    SHUTTER_STEP_OUTPUTS = ("g", "Bm", "cost", "gx", "rcb", "g_total", "step", "meas_err")

    def _shutter_step_shapes(self, B, N):
        Cn, L = self.n_cams, self.L
        return dict(g=(B, N, 28), Bm=(B, N, 28, 28), cost=(B, N, 3), gx=(B, N, 6), rcb=(B, N, Cn, 9), g_total=(B, N, 28), step=(B, Cn),
                    meas_err=(B, N, Cn, L, 2))

    def eval_shutter_step(self, q, meas, weight, tau, lam, seq, **out):
        """cpe_eval_shutter_step on device tensors (tau [B, C]; seq: numpy [B, 8]); out: any of SHUTTER_STEP_OUTPUTS, the others are not asked for"""
        assert set(out) <= set(self.SHUTTER_STEP_OUTPUTS)
        self._call(self.lib.cpe_eval_shutter_step, "cpe_eval_shutter_step", q.shape[0], q.shape[1], _ptr(q), _ptr(meas), _ptr(weight), _ptr(tau),
                   float(lam), *[_ptr(out.get(k)) for k in self.SHUTTER_STEP_OUTPUTS], _ptr(seq))

    def eval_shutter_step_host(self, q, meas, weight, tau, lam):
        """cpe_eval_shutter_step_host: the first pass of a round of the shutter-delay estimation from Euler q at the delays tau [B, C] and damping
        lam.  numpy in, dict of numpy arrays out: g, g_total [B, N, 28], Bm [B, N, 28, 28], cost [B, N, 3], gx [B, N, 6], rcb [B, N, C, 9],
        step [B, C], meas_err [B, N, C, L, 2], seq [B, 8] (as eval_lm_step_host)"""
        q, meas, weight, tau = _f64(q), _f64(meas), _f64(weight), _f64(tau)
        B, N = q.shape[:2]
        if tau.shape != (B, self.n_cams):
            raise CpeError("eval_shutter_step_host: one delay per sequence and camera")
        out = {k: np.full(s, np.nan) for k, s in self._shutter_step_shapes(B, N).items()}
        seq = np.zeros((B, 8))
        _check(self.lib.cpe_eval_shutter_step_host(self._h, B, N, _ptr(q), _ptr(meas), _ptr(weight), _ptr(tau), float(lam),
                                                   *[_ptr(out[k]) for k in self.SHUTTER_STEP_OUTPUTS], _ptr(seq)), "cpe_eval_shutter_step_host")
        out["seq"] = seq
        return out

    def eval_active_list(self, status, window):
        """cpe_eval_active_list: k_build_act on B = len(status) sequences with these status words (0 = running) -> (act, n_act): act is the
        whole int32 array of window + 64 entries as the kernel left it (-1 where it wrote nothing), n_act the length of the list"""
        st = np.ascontiguousarray(status, dtype=np.int32)
        if st.ndim != 1:
            raise ValueError("eval_active_list: status is one word per sequence")
        window = int(window)
        act = np.zeros(max(window, 0) + 64, dtype=np.int32)
        n_act = C.c_int32(0)
        _check(self.lib.cpe_eval_active_list(self._h, st.shape[0], window, st.ctypes.data_as(ip), act.ctypes.data_as(ip), C.byref(n_act)),
               "cpe_eval_active_list")
        return act, n_act.value

    # ---- posterior covariance of the kinematic estimate (include/cpe.h, cpe_covariance) -----------------------------------------------
    def band_inverse(self, L, cov_diag, cov_off=None):
        """cpe_band_inverse on device tensors: L [B, N, pb + 1, 28, 28] (eval_lm_step_host's layout) -> cov_diag [B, N, 28, 28], cov_off
        [B, N, pb, 28, 28] (block [n][i-1] = Sigma(n + i, n)) or None"""
        self._call(self.lib.cpe_band_inverse, "cpe_band_inverse", L.shape[0], L.shape[1], _ptr(L), _ptr(cov_diag), _ptr(cov_off))

    def band_inverse_host(self, L):
        """numpy in, numpy out (staged through HBM with torch): (cov_diag, cov_off)"""
        Ld = self._to_device(L)
        B, N = Ld.shape[0], Ld.shape[1]
        cd, co = self._empty(B, N, 28, 28), self._empty(B, N, self.pb, 28, 28)
        self.band_inverse(Ld, cd, co)
        self.synchronize()
        return cd.cpu().numpy(), co.cpu().numpy()

    def covariance(self, q, meas, weight, ridge, cov_diag, cov_off=None, cov_pos=None, L=None):
        """cpe_covariance on device tensors: Sigma = (H + ridge D)^-1 at Euler q [B, N, nq] on its block band; cov_diag [B, N, 28, 28], cov_off
        [B, N, pb, 28, 28], cov_pos [B, N, L, 3, 3], L [B, N, pb + 1, 28, 28] (each of the last three may be None).  Returns (status, [status of
        every sequence]): abi.OK, or abi.NUMERICAL where the matrix has no Cholesky factor (that sequence's outputs are zero)."""
        B, N = q.shape[0], q.shape[1]
        seq = _int32s(B)
        st = self._call(self.lib.cpe_covariance, "cpe_covariance", B, N, _ptr(q), _ptr(meas), _ptr(weight), float(ridge), _ptr(cov_diag), _ptr(cov_off),
                        _ptr(cov_pos), _ptr(L), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def _covariance_outputs(self, B, N, want_off, want_pos, want_L):
        E = np.empty
        return dict(cov_diag=E((B, N, 28, 28)), cov_off=E((B, N, self.pb, 28, 28)) if want_off else None,
                    cov_pos=E((B, N, self.L, 3, 3)) if want_pos else None, L=E((B, N, self.pb + 1, 28, 28)) if want_L else None)

    def covariance_host(self, q, meas, weight, ridge=0.0, want_off=True, want_pos=True, want_L=False):
        """cpe_covariance_host: numpy in, dict of numpy arrays out (cov_diag, cov_off, cov_pos, L as in covariance(); status, seq_status)"""
        q, meas, weight = _f64(q), _f64(meas), _f64(weight)
        B, N = q.shape[:2]
        out = self._covariance_outputs(B, N, want_off, want_pos, want_L)
        seq = _int32s(B)
        st = self.lib.cpe_covariance_host(self._h, B, N, _ptr(q), _ptr(meas), _ptr(weight), float(ridge), _ptr(out["cov_diag"]), _ptr(out["cov_off"]),
                                          _ptr(out["cov_pos"]), _ptr(out["L"]), seq)
        _check(st, "cpe_covariance_host", allow=(abi.OK, abi.NUMERICAL))
        out.update(status=st, seq_status=list(seq)[:B])
        return out

    def covariance_ragged_host(self, q_list, meas_list, weight_list, model_list=None, ridge=0.0, want_off=True, want_pos=True, want_L=False):
        """cpe_covariance_ragged_host over sequences of their own length and model (solve_ragged_host's arguments): pads, runs, unpads.  Returns
        dict(cov_diag, cov_off, cov_pos, L = lists of per-sequence arrays [N_b, ...] or None, status, seq_status, padded = the padded outputs)."""
        p = self._ragged_batch("covariance_ragged_host", "one q, meas, weight and model", model_list, q_init=q_list, meas=meas_list, weight=weight_list)
        B, Nm = p["q_init"].shape[:2]
        out = self._covariance_outputs(B, Nm, want_off, want_pos, want_L)
        seq = _int32s(B)
        st = self.lib.cpe_covariance_ragged_host(self._h, B, Nm, p["model_arr"], p["len_arr"], _ptr(p["q_init"]), _ptr(p["meas"]), _ptr(p["weight"]),
                                                 float(ridge), _ptr(out["cov_diag"]), _ptr(out["cov_off"]), _ptr(out["cov_pos"]), _ptr(out["L"]), seq)
        _check(st, "cpe_covariance_ragged_host", allow=(abi.OK, abi.NUMERICAL))
        res = unpad_kinetic(out, p["lens"], p["cams"])
        res.update(status=st, seq_status=list(seq)[:B], padded=out)
        return res

    # ---- covariance between distant frames (include/cpe.h, cpe_covariance_columns) ---------------------------------------------------------
    def _column_args(self, who, shape, anchors, n_frames):
        """B, N, K and the host arrays (anchors [B, K], n_frames [B] or None) of a columns call, from the shape of L"""
        B, N = int(shape[0]), int(shape[1])
        an = np.ascontiguousarray(anchors, dtype=np.int32)
        if an.ndim != 2 or an.shape[0] != B:
            raise ValueError(f"{who}: anchors must be [B, K] with one row per sequence")
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        if nf is not None and nf.shape != (B,):
            raise ValueError(f"{who}: one frame count per sequence")
        return B, N, an.shape[1], an, nf, an.ctypes.data_as(ip), None if nf is None else nf.ctypes.data_as(ip)

    def covariance_columns(self, L, cov_diag, cov_off, anchors, cols, n_frames=None):
        """cpe_covariance_columns on device tensors: L [B, N, pb + 1, 28, 28], cov_diag [B, N, 28, 28], cov_off [B, N, pb, 28, 28] (a covariance
        entry's factor and band); anchors [B, K] and n_frames [B] (or None = all N) on the host -> cols [B, K, N, 28, 28]: block [b, k, n] =
        Sigma(n, anchors[b, k]) for n <= the anchor, zero elsewhere and for an anchor of -1"""
        B, N, K, _an, _nf, pa, pn = self._column_args("covariance_columns", L.shape, anchors, n_frames)
        self._call(self.lib.cpe_covariance_columns, "cpe_covariance_columns", B, N, pn, _ptr(L), _ptr(cov_diag), _ptr(cov_off), K, pa, _ptr(cols))

    def covariance_columns_host(self, L, cov_diag, cov_off, anchors, n_frames=None):
        """cpe_covariance_columns_host: numpy in, cols [B, K, N, 28, 28] out"""
        L, cov_diag, cov_off = _f64(L), _f64(cov_diag), _f64(cov_off)
        B, N, K, _an, _nf, pa, pn = self._column_args("covariance_columns_host", L.shape, anchors, n_frames)
        if L.shape != (B, N, self.pb + 1, 28, 28) or cov_diag.shape != (B, N, 28, 28) or cov_off.shape != (B, N, self.pb, 28, 28):
            raise ValueError(f"covariance_columns_host: L / cov_diag / cov_off do not have the shapes of the handle's half-bandwidth {self.pb}")
        cols = np.empty((B, K, N, 28, 28))
        _check(self.lib.cpe_covariance_columns_host(self._h, B, N, pn, _ptr(L), _ptr(cov_diag), _ptr(cov_off), K, pa, _ptr(cols)),
               "cpe_covariance_columns_host")
        return cols

    # ---- draws from the posterior (include/cpe.h, cpe_band_sample / cpe_posterior_samples) -------------------------------------------------
    def _sample_args(self, who, L_shape, z_shape, n_frames):
        """B, N, S and the host array n_frames [B] (or None = all N) of a band_sample call, from the shapes of L and z"""
        B, N = int(L_shape[0]), int(L_shape[1])
        if tuple(L_shape) != (B, N, self.pb + 1, 28, 28) or len(z_shape) != 4 or (z_shape[0], z_shape[2], z_shape[3]) != (B, N, 28):
            raise ValueError(f"{who}: L is [B, N, {self.pb + 1}, 28, 28] (the handle's half-bandwidth is {self.pb}) and z [B, S, N, 28]")
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        if nf is not None and nf.shape != (B,):
            raise ValueError(f"{who}: one frame count per sequence")
        return B, N, int(z_shape[1]), nf, None if nf is None else nf.ctypes.data_as(ip)

    def band_sample(self, L, z, du, n_frames=None):
        """cpe_band_sample on device tensors: L [B, N, pb + 1, 28, 28] (a covariance entry's factor), z [B, S, N, 28] -> du [B, S, N, 28], the
        solutions of L^T du = z: with z ~ N(0, I) draws from N(0, Sigma).  n_frames [B] on the host (or None = all N): du is zero past a
        sequence's frames, and a sequence of 0 frames is not read"""
        B, N, S, _nf, pn = self._sample_args("band_sample", L.shape, z.shape, n_frames)
        self._call(self.lib.cpe_band_sample, "cpe_band_sample", B, N, pn, _ptr(L), S, _ptr(z), _ptr(du))

    def band_sample_host(self, L, z, n_frames=None):
        """cpe_band_sample_host: numpy in, du [B, S, N, 28] out"""
        L, z = _f64(L), _f64(z)
        B, N, S, _nf, pn = self._sample_args("band_sample_host", L.shape, z.shape, n_frames)
        du = np.empty((B, S, N, 28))
        _check(self.lib.cpe_band_sample_host(self._h, B, N, pn, _ptr(L), S, _ptr(z), _ptr(du)), "cpe_band_sample_host")
        return du

    def posterior_samples(self, q, du, q_s, positions_s=None, model=None, n_frames=None):
        """cpe_posterior_samples on device tensors: q [B, N, nq] (the estimate), du [B, S, N, 28] (band_sample's) -> q_s [B, S, N, nq], the poses
        of the samples (they satisfy the joint equalities), and positions_s [B, S, N, L, 3] (or None).  model / n_frames: int sequences of a
        ragged batch (everything past a sequence's frames is zero), or None"""
        B, N, S = q.shape[0], q.shape[1], du.shape[1]
        if (model is None) != (n_frames is None):
            raise ValueError("posterior_samples: model and n_frames are given together or not at all")
        mo = nf = None
        if model is not None:
            if len(model) != B or len(n_frames) != B:
                raise ValueError("posterior_samples: one model index and one frame count per sequence")
            mo, nf = _int32s(B, model), _int32s(B, n_frames)
        self._call(self.lib.cpe_posterior_samples, "cpe_posterior_samples", B, N, mo, nf, _ptr(q), S, _ptr(du), _ptr(q_s), _ptr(positions_s))

    def posterior_samples_host(self, q, du, model_list=None, want_positions=True):
        """cpe_posterior_samples_host: q [B, N, nq], du [B, S, N, 28] numpy -> dict(q [B, S, N, nq], positions [B, S, N, L, 3] or None); or, for
        sequences of their own length (and model, model_list; None = model 0), lists of q [N_b, nq] and du [S, N_b, 28] -> lists of
        [S, N_b, ...] from ONE call"""
        ragged = isinstance(q, (list, tuple))
        if ragged:
            lens = [int(np.shape(a)[0]) for a in q]
            B, Nm = len(lens), max(lens) if lens else 0
            models = [0] * B if model_list is None else [int(m) for m in model_list]
            S = int(np.shape(du[0])[0]) if B else 1
            if len(du) != B or len(models) != B or any(np.shape(du[b]) != (S, lens[b], 28) or np.shape(q[b]) != (lens[b], self.nq) for b in range(B)):
                raise ValueError("posterior_samples_host: one q [N_b, nq], du [S, N_b, 28] and model per sequence, the same S for all")
            qp = _f64(_pad(q, Nm, (self.nq,)))
            dp_ = np.zeros((B, S, Nm, 28))
            for b in range(B):
                dp_[b, :, :lens[b]] = du[b]
            mo, nf = _int32s(B, models), _int32s(B, lens)
        else:
            qp, dp_ = _f64(q), _f64(du)
            if qp.ndim != 3 or dp_.ndim != 4 or (dp_.shape[0], dp_.shape[2], dp_.shape[3]) != (qp.shape[0], qp.shape[1], 28) or qp.shape[2] != self.nq:
                raise ValueError("posterior_samples_host: q is [B, N, nq] and du [B, S, N, 28]")
            B, Nm, S = qp.shape[0], qp.shape[1], dp_.shape[1]
            mo = nf = None
        q_s = np.empty((B, S, Nm, self.nq))
        pos = np.empty((B, S, Nm, self.L, 3)) if want_positions else None
        _check(self.lib.cpe_posterior_samples_host(self._h, B, Nm, mo, nf, _ptr(qp), S, _ptr(dp_), _ptr(q_s), _ptr(pos)), "cpe_posterior_samples_host")
        if not ragged:
            return dict(q=q_s, positions=pos)
        cut = lambda a: None if a is None else [np.ascontiguousarray(a[b, :, :n]) for b, n in enumerate(lens)]
        return dict(q=cut(q_s), positions=cut(pos), padded=dict(q=q_s, positions=pos))

    # ---- the reduced system of the length calibration (include/cpe.h, cpe_scale_system) ---------------------------------------------------
    def _scale_tables(self, who, d_attach, d_marker_off):
        """G and the host tables d_attach [M, G, n_links, 3], d_marker_off [M, G, n_markers, 3] (M = the handle's models; a table of one model
        may come without the leading axis)"""
        da, dm = _f64(d_attach), _f64(d_marker_off)
        M = len(self.model_n_cams)
        if da.ndim == 3 and dm.ndim == 3 and M == 1:
            da, dm = da[None], dm[None]
        G = da.shape[1] if da.ndim == 4 else -1
        if da.shape != (M, G, self.sk.n_links, 3) or dm.shape != (M, G, self.L, 3):
            raise ValueError(f"{who}: d_attach is [{M}, G, {self.sk.n_links}, 3] and d_marker_off [{M}, G, {self.L}, 3]")
        return G, np.ascontiguousarray(da), np.ascontiguousarray(dm)

    def scale_system(self, q, meas, weight, d_attach, d_marker_off, A, b, A_red, b_red, cost, ridge=0.0, model=None, n_frames=None):
        """cpe_scale_system on device tensors: the Gauss-Newton system of G segment-length scales at Euler q [B, N, nq], poses eliminated through
        the band factor of (H + ridge D).  d_attach, d_marker_off: numpy (skeleton.length_derivatives).  A, A_red [B, G, G], b, b_red [B, G],
        cost [B] device tensors.  Returns (status, [status of every sequence]) as covariance() does."""
        B, N = q.shape[0], q.shape[1]
        G, da, dm = self._scale_tables("scale_system", d_attach, d_marker_off)
        if (model is None) != (n_frames is None):
            raise ValueError("scale_system: model and n_frames are given together or not at all")
        mo = nf = None
        if model is not None:
            if len(model) != B or len(n_frames) != B:
                raise ValueError("scale_system: one model index and one frame count per sequence")
            mo, nf = _int32s(B, model), _int32s(B, n_frames)
        for name, t, shape in (("A", A, (B, G, G)), ("b", b, (B, G)), ("A_red", A_red, (B, G, G)), ("b_red", b_red, (B, G)), ("cost", cost, (B,))):
            if t is None or tuple(t.shape) != shape or t.element_size() != 8 or not t.dtype.is_floating_point or not t.is_contiguous():
                raise ValueError(f"scale_system: {name} is a contiguous float64 tensor of shape {shape}")
        seq = _int32s(B)
        st = self._call(self.lib.cpe_scale_system, "cpe_scale_system", B, N, mo, nf, _ptr(q), _ptr(meas), _ptr(weight), float(ridge), G, _ptr(da),
                        _ptr(dm), _ptr(A), _ptr(b), _ptr(A_red), _ptr(b_red), _ptr(cost), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def scale_system_host(self, q, meas, weight, d_attach, d_marker_off, ridge=0.0, model_list=None):
        """cpe_scale_system_host: q [B, N, nq], meas, weight numpy -> dict(A, A_red [B, G, G], b, b_red [B, G], cost [B], status, seq_status); or,
        for sequences of their own length and model (lists, as covariance_ragged_host takes them; model_list None = model 0), ONE ragged call"""
        if isinstance(q, (list, tuple)):
            p = self._ragged_batch("scale_system_host", "one q, meas, weight and model", model_list, q_init=q, meas=meas, weight=weight)
            qp, mp, wp, mo, nf = p["q_init"], p["meas"], p["weight"], p["model_arr"], p["len_arr"]
        else:
            qp, mp, wp, mo, nf = _f64(q), _f64(meas), _f64(weight), None, None
        B, N = qp.shape[:2]
        G, da, dm = self._scale_tables("scale_system_host", d_attach, d_marker_off)
        out = dict(A=np.empty((B, G, G)), b=np.empty((B, G)), A_red=np.empty((B, G, G)), b_red=np.empty((B, G)), cost=np.empty(B))
        seq = _int32s(B)
        st = self.lib.cpe_scale_system_host(self._h, B, N, mo, nf, _ptr(qp), _ptr(mp), _ptr(wp), float(ridge), G, _ptr(da), _ptr(dm), _ptr(out["A"]),
                                            _ptr(out["b"]), _ptr(out["A_red"]), _ptr(out["b_red"]), _ptr(out["cost"]), seq)
        _check(st, "cpe_scale_system_host", allow=(abi.OK, abi.NUMERICAL))
        out.update(status=st, seq_status=list(seq)[:B])
        return out

    # ---- the pose covariance marginalised over the scales (include/cpe.h, cpe_scale_response / cpe_covariance_add_scales) ------------------
    def scale_response(self, q, meas, weight, d_attach, d_marker_off, A_red, resp_u, resp_pos=None, ridge=0.0, model=None, n_frames=None):
        """cpe_scale_response on device tensors: scale_system's inputs -> A_red [B, G, G] (scale_system's, bit for bit), resp_u [B, N, 28, G] =
        du / ds of the re-adapted poses, resp_pos [B, N, L, 3, G] = d p / d s in total (or None).  Returns (status, [status of every sequence])."""
        B, N = q.shape[0], q.shape[1]
        G, da, dm = self._scale_tables("scale_response", d_attach, d_marker_off)
        if (model is None) != (n_frames is None):
            raise ValueError("scale_response: model and n_frames are given together or not at all")
        mo = nf = None
        if model is not None:
            if len(model) != B or len(n_frames) != B:
                raise ValueError("scale_response: one model index and one frame count per sequence")
            mo, nf = _int32s(B, model), _int32s(B, n_frames)
        for name, t, shape in (("A_red", A_red, (B, G, G)), ("resp_u", resp_u, (B, N, 28, G)), ("resp_pos", resp_pos, (B, N, self.L, 3, G))):
            if name == "resp_pos" and t is None:
                continue
            if t is None or tuple(t.shape) != shape or t.element_size() != 8 or not t.dtype.is_floating_point or not t.is_contiguous():
                raise ValueError(f"scale_response: {name} is a contiguous float64 tensor of shape {shape}")
        seq = _int32s(B)
        st = self._call(self.lib.cpe_scale_response, "cpe_scale_response", B, N, mo, nf, _ptr(q), _ptr(meas), _ptr(weight), float(ridge), G, _ptr(da),
                        _ptr(dm), _ptr(A_red), _ptr(resp_u), _ptr(resp_pos), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def scale_response_host(self, q, meas, weight, d_attach, d_marker_off, ridge=0.0, model_list=None, want_pos=True):
        """cpe_scale_response_host: q [B, N, nq], meas, weight numpy -> dict(A_red [B, G, G], resp_u [B, N, 28, G], resp_pos [B, N, L, 3, G] or
        None, status, seq_status); or, for sequences of their own length and model (lists, as scale_system_host takes them), ONE ragged call:
        resp_u and resp_pos are then lists of [N_b, ...] and `padded` holds the padded arrays and `lens` the lengths"""
        ragged = isinstance(q, (list, tuple))
        if ragged:
            p = self._ragged_batch("scale_response_host", "one q, meas, weight and model", model_list, q_init=q, meas=meas, weight=weight)
            qp, mp, wp, mo, nf = p["q_init"], p["meas"], p["weight"], p["model_arr"], p["len_arr"]
        else:
            qp, mp, wp, mo, nf = _f64(q), _f64(meas), _f64(weight), None, None
        B, N = qp.shape[:2]
        G, da, dm = self._scale_tables("scale_response_host", d_attach, d_marker_off)
        out = dict(A_red=np.empty((B, G, G)), resp_u=np.empty((B, N, 28, G)), resp_pos=np.empty((B, N, self.L, 3, G)) if want_pos else None)
        seq = _int32s(B)
        st = self.lib.cpe_scale_response_host(self._h, B, N, mo, nf, _ptr(qp), _ptr(mp), _ptr(wp), float(ridge), G, _ptr(da), _ptr(dm),
                                              _ptr(out["A_red"]), _ptr(out["resp_u"]), _ptr(out["resp_pos"]), seq)
        _check(st, "cpe_scale_response_host", allow=(abi.OK, abi.NUMERICAL))
        if ragged:
            pad = dict(resp_u=out["resp_u"], resp_pos=out["resp_pos"])
            out.update(unpad_kinetic(pad, p["lens"], p["cams"]), padded=pad, lens=list(p["lens"]))
        out.update(status=st, seq_status=list(seq)[:B])
        return out

    def _add_scales_args(self, who, cov_s, resp_u, n_frames):
        """B, N, G and the host array n_frames [B] (or None = all N) of an add_scales call, from the shapes of resp_u and cov_s"""
        if len(resp_u.shape) != 4 or resp_u.shape[2] != 28 or tuple(cov_s.shape) != (resp_u.shape[0], resp_u.shape[3], resp_u.shape[3]):
            raise ValueError(f"{who}: resp_u is [B, N, 28, G] and cov_s [B, G, G]")
        B, N, G = int(resp_u.shape[0]), int(resp_u.shape[1]), int(resp_u.shape[3])
        nf = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        if nf is not None and nf.shape != (B,):
            raise ValueError(f"{who}: one frame count per sequence")
        return B, N, G, nf, None if nf is None else nf.ctypes.data_as(ip)

    def covariance_add_scales(self, cov_s, resp_u, resp_pos, cov_diag, cov_off, cov_pos, cov_diag_m, cov_off_m, cov_pos_m, n_frames=None):
        """cpe_covariance_add_scales on device tensors: cov_s [B, G, G], scale_response's resp_u and resp_pos, a covariance entry's cov_diag,
        cov_off and cov_pos -> the same three with the scale terms added (resp_pos, cov_pos and cov_pos_m: all three or None).  n_frames [B] on
        the host (or None = all N)"""
        B, N, G, _nf, pn = self._add_scales_args("covariance_add_scales", cov_s, resp_u, n_frames)
        self._call(self.lib.cpe_covariance_add_scales, "cpe_covariance_add_scales", B, N, pn, G, _ptr(cov_s), _ptr(resp_u), _ptr(resp_pos), _ptr(cov_diag),
                   _ptr(cov_off), _ptr(cov_pos), _ptr(cov_diag_m), _ptr(cov_off_m), _ptr(cov_pos_m))

    def covariance_add_scales_host(self, cov_s, resp_u, resp_pos, cov_diag, cov_off, cov_pos, n_frames=None):
        """cpe_covariance_add_scales_host: numpy in (padded arrays [B, N, ...]; resp_pos and cov_pos both None or both given), dict(cov_diag,
        cov_off, cov_pos or None) out: the marginal band and marker covariances"""
        cov_s, resp_u, cov_diag, cov_off = _f64(cov_s), _f64(resp_u), _f64(cov_diag), _f64(cov_off)
        resp_pos, cov_pos = _f64(resp_pos, True), _f64(cov_pos, True)
        B, N, G, _nf, pn = self._add_scales_args("covariance_add_scales_host", cov_s, resp_u, n_frames)
        if cov_diag.shape != (B, N, 28, 28) or cov_off.shape != (B, N, self.pb, 28, 28):
            raise ValueError(f"covariance_add_scales_host: cov_diag / cov_off do not have the shapes of the handle's half-bandwidth {self.pb}")
        if (resp_pos is None) != (cov_pos is None) or (cov_pos is not None and (cov_pos.shape != (B, N, self.L, 3, 3) or resp_pos.shape != (B, N, self.L, 3, G))):
            raise ValueError("covariance_add_scales_host: resp_pos [B, N, L, 3, G] and cov_pos [B, N, L, 3, 3] are given together or not at all")
        out = dict(cov_diag=np.empty_like(cov_diag), cov_off=np.empty_like(cov_off), cov_pos=None if cov_pos is None else np.empty_like(cov_pos))
        _check(self.lib.cpe_covariance_add_scales_host(self._h, B, N, pn, G, _ptr(cov_s), _ptr(resp_u), _ptr(resp_pos), _ptr(cov_diag), _ptr(cov_off),
                                                       _ptr(cov_pos), _ptr(out["cov_diag"]), _ptr(out["cov_off"]), _ptr(out["cov_pos"])),
               "cpe_covariance_add_scales_host")
        return out

    # ---- posterior covariance of the rates (include/cpe.h, cpe_rate_covariance) -----------------------------------------------------------
    def rate_covariance(self, q, cov_diag, cov_off, cov_du=None, cov_ddu=None, cov_vel=None, cov_com=None, cov_com_vel=None, jac_pos=None,
                        jac_com=None):
        """cpe_rate_covariance on device tensors: q [B, N, nq], cov_diag [B, N, 28, 28], cov_off [B, N, pb, 28, 28] (a covariance entry's band) ->
        cov_du, cov_ddu [B, N, 28, 28], cov_vel [B, N, L, 3, 3], cov_com, cov_com_vel [B, N, 3, 3], jac_pos [B, N, L, 3, 28], jac_com [B, N, 3, 28];
        each may be None, not all"""
        self._call(self.lib.cpe_rate_covariance, "cpe_rate_covariance", q.shape[0], q.shape[1], _ptr(q), _ptr(cov_diag), _ptr(cov_off), _ptr(cov_du),
                   _ptr(cov_ddu), _ptr(cov_vel), _ptr(cov_com), _ptr(cov_com_vel), _ptr(jac_pos), _ptr(jac_com))

    def _rate_outputs(self, B, N, want):
        shapes = dict(cov_du=(28, 28), cov_ddu=(28, 28), cov_vel=(self.L, 3, 3), cov_com=(3, 3), cov_com_vel=(3, 3), jac_pos=(self.L, 3, 28),
                      jac_com=(3, 28))
        unknown = set(want) - set(shapes)
        if unknown:
            raise ValueError(f"rate covariance: unknown outputs {sorted(unknown)}")
        return {k: np.empty((B, N) + shapes[k]) if k in want else None for k in abi.RATE_COVARIANCE_OUTPUTS}

    def rate_covariance_host(self, q, cov_diag, cov_off, want=abi.RATE_COVARIANCE_OUTPUTS):
        """cpe_rate_covariance_host: numpy in, dict of numpy arrays out (the outputs named in `want`, shapes as in rate_covariance())"""
        q, cov_diag, cov_off = _f64(q), _f64(cov_diag), _f64(cov_off)
        B, N = q.shape[:2]
        if cov_diag.shape != (B, N, 28, 28) or cov_off.shape != (B, N, self.pb, 28, 28):
            raise ValueError(f"rate_covariance_host: cov_diag / cov_off do not have the shapes of q and the handle's half-bandwidth {self.pb}")
        out = self._rate_outputs(B, N, want)
        st = self.lib.cpe_rate_covariance_host(self._h, B, N, _ptr(q), _ptr(cov_diag), _ptr(cov_off), *[_ptr(out[k]) for k in abi.RATE_COVARIANCE_OUTPUTS])
        _check(st, "cpe_rate_covariance_host")
        return {k: v for k, v in out.items() if v is not None}

    def rate_covariance_ragged_host(self, q_list, cov_diag_list, cov_off_list, model_list=None, want=abi.RATE_COVARIANCE_OUTPUTS):
        """cpe_rate_covariance_ragged_host over sequences of their own length and model (covariance_ragged_host's q_list and model_list, and its
        per-sequence cov_diag / cov_off): pads, runs, unpads.  Returns dict(the outputs named in `want` = lists of per-sequence arrays [N_b, ...],
        padded = the padded outputs)."""
        B = len(q_list)
        models = [0] * B if model_list is None else [int(m) for m in model_list]
        if len(cov_diag_list) != B or len(cov_off_list) != B or len(models) != B:
            raise ValueError("rate_covariance_ragged_host: one q, cov_diag, cov_off and model per sequence")
        if any(m < 0 or m >= len(self.model_n_cams) for m in models):
            raise ValueError("rate_covariance_ragged_host: model index out of range")
        lens = [int(np.shape(a)[0]) for a in q_list]
        for b in range(B):
            if np.shape(q_list[b]) != (lens[b], self.nq) or np.shape(cov_diag_list[b]) != (lens[b], 28, 28) or \
                    np.shape(cov_off_list[b]) != (lens[b], self.pb, 28, 28):
                raise ValueError(f"rate_covariance_ragged_host: sequence {b} does not have the shapes of its {lens[b]} frames")
        Nm = max(lens) if lens else 0
        q, cd, co = _f64(_pad(q_list, Nm, (self.nq,))), _f64(_pad(cov_diag_list, Nm, (28, 28))), _f64(_pad(cov_off_list, Nm, (self.pb, 28, 28)))
        out = self._rate_outputs(B, Nm, want)
        mo, nf = _int32s(B, models), _int32s(B, lens)
        st = self.lib.cpe_rate_covariance_ragged_host(self._h, B, Nm, mo, nf, _ptr(q), _ptr(cd), _ptr(co),
                                                      *[_ptr(out[k]) for k in abi.RATE_COVARIANCE_OUTPUTS])
        _check(st, "cpe_rate_covariance_ragged_host")
        out = {k: v for k, v in out.items() if v is not None}
        res = unpad_kinetic(out, lens, None)
        res.update(padded=out)
        return res

    # ---- posterior covariance of the physics-based estimate (include/cpe.h, cpe_covariance_kinetic) ------------------------------------
    def covariance_kinetic(self, kopt, q, meas, weight, stance, ridge, cov_diag, cov_off=None, cov_pos=None, cov_f=None, f=None, meta=None, L=None,
                           grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_covariance_kinetic on device tensors (stance, meta int32; the outputs as in covariance_kinetic_host, each but cov_diag may be None).
        Returns (status, [status of every sequence])."""
        B, N = q.shape[0], q.shape[1]
        seq = _int32s(B)
        st = self._call(self.lib.cpe_covariance_kinetic, "cpe_covariance_kinetic", C.byref(kopt) if kopt is not None else None, B, N, _ptr(q),
                        _ptr(meas), _ptr(weight), _ptr(stance), _ptr(grf_fixed), _ptr(tau_box), _ptr(grf_box), float(ridge), _ptr(cov_diag),
                        _ptr(cov_off), _ptr(cov_pos), _ptr(cov_f), _ptr(f), _ptr(meta), _ptr(L), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def covariance_kinetic_host(self, q, meas, weight, stance, kopt, ridge=0.0, grf_fixed=None, tau_box=None, grf_box=None, want_L=False):
        """cpe_covariance_kinetic_host: numpy in, dict of numpy arrays out -- cov_diag [B, N, 28, 28], cov_off [B, N, 3, 28, 28], cov_pos
        [B, N, L, 3, 3] as covariance_host; cov_f [B, N, 64, 64] the covariance of every node's free forces in the compact order of meta
        [B, N, 65] = (count, indices into f's layout tau | lambda | (z, x, y) per foot, ...), f [B, N, 64]; L with want_L; status, seq_status.
        grf_fixed / tau_box / grf_box (at most one) in solve_kinetic_host's layouts."""
        q, meas, weight, grf_fixed, tau_box, grf_box = (_f64(a, optional=True) for a in (q, meas, weight, grf_fixed, tau_box, grf_box))
        stance = None if stance is None else np.ascontiguousarray(stance, dtype=np.int32)
        B, N = q.shape[:2]
        out = self._covariance_outputs(B, N, True, True, want_L)
        out.update(cov_f=np.empty((B, N, 64, 64)), f=np.empty((B, N, 64)), meta=np.empty((B, N, 65), dtype=np.int32))
        seq = _int32s(B)
        st = self.lib.cpe_covariance_kinetic_host(self._h, C.byref(kopt) if kopt is not None else None, B, N, _ptr(q), _ptr(meas), _ptr(weight),
                                                  None if stance is None else stance.ctypes.data, _ptr(grf_fixed), _ptr(tau_box), _ptr(grf_box),
                                                  float(ridge), _ptr(out["cov_diag"]), _ptr(out["cov_off"]), _ptr(out["cov_pos"]), _ptr(out["cov_f"]),
                                                  _ptr(out["f"]), out["meta"].ctypes.data,
                                                  _ptr(out["L"]), seq)
        _check(st, "cpe_covariance_kinetic_host", allow=(abi.OK, abi.NUMERICAL))
        if not want_L:
            del out["L"]
        out.update(status=st, seq_status=list(seq)[:B])
        return out

    def covariance_kinetic_ragged(self, kopts_list, model, n_frames, q, meas, weight, stance, ridge, cov_diag, cov_off=None, cov_pos=None, cov_f=None,
                                  f=None, meta=None, L=None, grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_covariance_kinetic_ragged on device tensors laid out for N_max = q.shape[1] frames and C_max cameras, as solve_kinetic_ragged takes
        them; kopts_list: one KineticOptions per model of the handle; model / n_frames: int sequences (one per sequence).  The outputs as in
        covariance_kinetic, zero past every sequence's own frames.  Returns (status, [status of every sequence])."""
        _force_variant("covariance_kinetic_ragged", grf_fixed, tau_box, grf_box)
        ko = self._kinetic_options_array(kopts_list)
        B, N = q.shape[0], q.shape[1]
        if len(model) != B or len(n_frames) != B:
            raise ValueError("covariance_kinetic_ragged: one model index and one frame count per sequence")
        seq = _int32s(B)
        mo, nf = _int32s(B, model), _int32s(B, n_frames)
        st = self._call(self.lib.cpe_covariance_kinetic_ragged, "cpe_covariance_kinetic_ragged", ko, B, N, mo, nf, _ptr(q), _ptr(meas), _ptr(weight),
                        _ptr(stance), _ptr(grf_fixed), _ptr(tau_box), _ptr(grf_box), float(ridge), _ptr(cov_diag), _ptr(cov_off), _ptr(cov_pos),
                        _ptr(cov_f), _ptr(f), _ptr(meta), _ptr(L), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def covariance_kinetic_ragged_host(self, q_list, meas_list, weight_list, stance_list, kopts_list, model_list=None, ridge=0.0, grf_fixed=None,
                                       tau_box=None, grf_box=None, want_L=False):
        """cpe_covariance_kinetic_ragged_host over sequences of their own length and model (solve_kinetic_ragged_host's arguments: kopts_list one
        KineticOptions per model of the handle; grf_fixed / tau_box / grf_box, at most one, a list of one array per sequence): pads, runs, unpads.
        Returns dict(cov_diag, cov_off, cov_pos, cov_f, f, meta (L with want_L) = lists of per-sequence arrays [N_b, ...] as in
        covariance_kinetic_host, status, seq_status, padded = the padded outputs)."""
        who = "covariance_kinetic_ragged_host"
        variant, force = _force_variant(who, grf_fixed, tau_box, grf_box)
        p = self._ragged_batch(who, "one q, meas, weight, stance, model (and force array)", model_list, kopts_list, variant,
                               q_init=q_list, meas=meas_list, weight=weight_list, stance=stance_list, force=force)
        B, Nm = p["q_init"].shape[:2]
        out = self._covariance_outputs(B, Nm, True, True, want_L)
        out.update(cov_f=np.empty((B, Nm, 64, 64)), f=np.empty((B, Nm, 64)), meta=np.empty((B, Nm, 65), dtype=np.int32))
        if not want_L:
            del out["L"]
        seq = _int32s(B)
        ko = self._kinetic_options_array(kopts_list)
        st = self.lib.cpe_covariance_kinetic_ragged_host(self._h, ko, B, Nm, p["model_arr"], p["len_arr"], _ptr(p["q_init"]), _ptr(p["meas"]),
                                                         _ptr(p["weight"]), p["stance"].ctypes.data, *_force_slots(variant, p["force"]), float(ridge),
                                                         _ptr(out["cov_diag"]), _ptr(out["cov_off"]), _ptr(out["cov_pos"]), _ptr(out["cov_f"]),
                                                         _ptr(out["f"]), out["meta"].ctypes.data, _ptr(out.get("L")), seq)
        _check(st, "cpe_covariance_kinetic_ragged_host", allow=(abi.OK, abi.NUMERICAL))
        res = unpad_kinetic(out, p["lens"], p["cams"])
        res.update(status=st, seq_status=list(seq)[:B], padded=out)
        return res

    # ---- draws of the node forces of the physics-based estimate (include/cpe.h, cpe_force_samples) -----------------------------------------
    def force_samples(self, kopt, q, meas, weight, stance, ridge, du, f_s, zeta=None, f=None, meta=None, grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_force_samples on device tensors: du [B, S, N, 28] (band_sample's on the factor covariance_kinetic returns, or any step), zeta
        [B, S, N, 64] (standard normals in the compact order of meta; None = zeros: the conditional mean) -> f_s [B, S, N, 64] in f's layout
        tau | lambda | (z, x, y) per foot; f [B, N, 64], meta int32 [B, N, 65] as covariance_kinetic (each may be None).
        Returns (status, [status of every sequence])."""
        B, N, S = q.shape[0], q.shape[1], du.shape[1]
        seq = _int32s(B)
        st = self._call(self.lib.cpe_force_samples, "cpe_force_samples", C.byref(kopt) if kopt is not None else None, B, N, _ptr(q), _ptr(meas),
                        _ptr(weight), _ptr(stance), _ptr(grf_fixed), _ptr(tau_box), _ptr(grf_box), float(ridge), S, _ptr(du), _ptr(zeta), _ptr(f_s),
                        _ptr(f), _ptr(meta), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def force_samples_host(self, q, meas, weight, stance, kopt, du, zeta=None, ridge=0.0, grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_force_samples_host: numpy in (du [B, S, N, 28], zeta [B, S, N, 64] or None), dict of numpy arrays out -- f_s [B, S, N, 64], f
        [B, N, 64], meta [B, N, 65] (as covariance_kinetic_host's), status, seq_status"""
        q, meas, weight, grf_fixed, tau_box, grf_box, zeta = (_f64(a, optional=True) for a in (q, meas, weight, grf_fixed, tau_box, grf_box, zeta))
        stance = None if stance is None else np.ascontiguousarray(stance, dtype=np.int32)
        du = _f64(du)
        B, N = q.shape[:2]
        if du.ndim != 4 or (du.shape[0], du.shape[2], du.shape[3]) != (B, N, 28) or (zeta is not None and zeta.shape != du.shape[:3] + (64,)):
            raise ValueError("force_samples_host: du is [B, S, N, 28] and zeta [B, S, N, 64] (or None)")
        S = du.shape[1]
        out = dict(f_s=np.empty((B, S, N, 64)), f=np.empty((B, N, 64)), meta=np.empty((B, N, 65), dtype=np.int32))
        seq = _int32s(B)
        st = self.lib.cpe_force_samples_host(self._h, C.byref(kopt) if kopt is not None else None, B, N, _ptr(q), _ptr(meas), _ptr(weight),
                                             None if stance is None else stance.ctypes.data, _ptr(grf_fixed), _ptr(tau_box), _ptr(grf_box),
                                             float(ridge), S, _ptr(du), _ptr(zeta), _ptr(out["f_s"]), _ptr(out["f"]), out["meta"].ctypes.data, seq)
        _check(st, "cpe_force_samples_host", allow=(abi.OK, abi.NUMERICAL))
        out.update(status=st, seq_status=list(seq)[:B])
        return out

    def force_samples_ragged(self, kopts_list, model, n_frames, q, meas, weight, stance, ridge, du, f_s, zeta=None, f=None, meta=None, grf_fixed=None,
                             tau_box=None, grf_box=None):
        """cpe_force_samples_ragged on device tensors laid out for N_max = q.shape[1] frames and C_max cameras, as covariance_kinetic_ragged takes
        them; the outputs as in force_samples, zero past every sequence's own frames.  Returns (status, [status of every sequence])."""
        _force_variant("force_samples_ragged", grf_fixed, tau_box, grf_box)
        ko = self._kinetic_options_array(kopts_list)
        B, N, S = q.shape[0], q.shape[1], du.shape[1]
        if len(model) != B or len(n_frames) != B:
            raise ValueError("force_samples_ragged: one model index and one frame count per sequence")
        seq = _int32s(B)
        mo, nf = _int32s(B, model), _int32s(B, n_frames)
        st = self._call(self.lib.cpe_force_samples_ragged, "cpe_force_samples_ragged", ko, B, N, mo, nf, _ptr(q), _ptr(meas), _ptr(weight),
                        _ptr(stance), _ptr(grf_fixed), _ptr(tau_box), _ptr(grf_box), float(ridge), S, _ptr(du), _ptr(zeta), _ptr(f_s), _ptr(f),
                        _ptr(meta), seq, allow=(abi.OK, abi.NUMERICAL))
        return st, list(seq)[:B]

    def force_samples_ragged_host(self, q_list, meas_list, weight_list, stance_list, kopts_list, du_list, zeta_list=None, model_list=None, ridge=0.0,
                                  grf_fixed=None, tau_box=None, grf_box=None):
        """cpe_force_samples_ragged_host over sequences of their own length and model (covariance_kinetic_ragged_host's arguments, then du_list:
        one [S, N_b, 28] per sequence, the same S for all, and zeta_list: one [S, N_b, 64] per sequence, or None): pads, runs, unpads.  Returns
        dict(f_s = list of [S, N_b, 64], f, meta = lists of [N_b, ...], status, seq_status, padded = the padded outputs)."""
        who = "force_samples_ragged_host"
        variant, force = _force_variant(who, grf_fixed, tau_box, grf_box)
        p = self._ragged_batch(who, "one q, meas, weight, stance, model (and force array)", model_list, kopts_list, variant,
                               q_init=q_list, meas=meas_list, weight=weight_list, stance=stance_list, force=force)
        B, Nm = p["q_init"].shape[:2]
        lens = p["lens"]
        S = int(np.shape(du_list[0])[0]) if B else 1
        if len(du_list) != B or any(np.shape(du_list[b]) != (S, lens[b], 28) for b in range(B)) or \
                (zeta_list is not None and (len(zeta_list) != B or any(np.shape(zeta_list[b]) != (S, lens[b], 64) for b in range(B)))):
            raise ValueError(f"{who}: one du [S, N_b, 28] (and zeta [S, N_b, 64]) per sequence, the same S for all")
        du = np.zeros((B, S, Nm, 28))
        zeta = None if zeta_list is None else np.zeros((B, S, Nm, 64))
        for b in range(B):
            du[b, :, :lens[b]] = du_list[b]
            if zeta is not None:
                zeta[b, :, :lens[b]] = zeta_list[b]
        out = dict(f_s=np.empty((B, S, Nm, 64)), f=np.empty((B, Nm, 64)), meta=np.empty((B, Nm, 65), dtype=np.int32))
        seq = _int32s(B)
        ko = self._kinetic_options_array(kopts_list)
        st = self.lib.cpe_force_samples_ragged_host(self._h, ko, B, Nm, p["model_arr"], p["len_arr"], _ptr(p["q_init"]), _ptr(p["meas"]),
                                                    _ptr(p["weight"]), p["stance"].ctypes.data, *_force_slots(variant, p["force"]), float(ridge), S,
                                                    _ptr(du), _ptr(zeta), _ptr(out["f_s"]), _ptr(out["f"]), out["meta"].ctypes.data, seq)
        _check(st, who, allow=(abi.OK, abi.NUMERICAL))
        res = unpad_kinetic(dict(f=out["f"], meta=out["meta"]), lens, p["cams"])
        res.update(f_s=[np.ascontiguousarray(out["f_s"][b, :, :n]) for b, n in enumerate(lens)], status=st, seq_status=list(seq)[:B], padded=out)
        return res

    # ---- host-pointer conveniences (numpy in, numpy out; PCIe-inclusive) -------------------------------
    def eval_resjac_host(self, q, meas, weight, want_cost=True):
        q, meas, weight = _f64(q), _f64(meas), _f64(weight)
        B, N = q.shape[:2]
        r = np.empty((B, N, self.n_cams, self.L, 2)); J = np.empty((B, N, self.n_cams, self.S, 2))
        eps = np.empty((B, N, self.nq)); cost = np.empty((B, N)) if want_cost else None
        _check(self.lib.cpe_eval_resjac_host(self._h, B, N, _ptr(q), _ptr(meas), _ptr(weight), _ptr(r), _ptr(J), _ptr(eps), _ptr(cost)),
               "cpe_eval_resjac_host")
        return r, J, eps, cost

    def solve_host(self, q_init, meas, weight):
        q_init, meas, weight = _f64(q_init), _f64(meas), _f64(weight)
        B, N = q_init.shape[:2]
        out = self._solve_outputs(B, N)
        stats = (abi.Stats * max(B, 1))()
        st = self.lib.cpe_solve_host(self._h, B, N, _ptr(q_init), _ptr(meas), _ptr(weight), *[_ptr(a) for a in out.values()], stats)
        _check(st, "cpe_solve_host", allow=(abi.OK, abi.MAX_ITER, abi.NUMERICAL))
        return dict(status=st, **out, stats=list(stats)[:B])

    def solve_ragged_host(self, q_init_list, meas_list, weight_list, model_list=None):
        """cpe_solve_ragged_host over sequences of their own length and model: q_init [N_b, nq], meas [N_b, C_m, L, 2], weight [N_b, C_m, L]
        per sequence (C_m = the camera count of its model, model_list[b]; None = model 0 for all).  Pads, solves, unpads: returns dict(status,
        q, dq, ddq, positions, meas_err = lists of per-sequence arrays of the sequence's own shapes, stats = list of Stats)."""
        p = self._ragged_batch("solve_ragged_host", "one q_init, meas, weight and model", model_list, q_init=q_init_list, meas=meas_list,
                               weight=weight_list)
        B, Nm = p["q_init"].shape[:2]
        out = self._solve_outputs(B, Nm)
        stats = (abi.Stats * max(B, 1))()
        st = self.lib.cpe_solve_ragged_host(self._h, B, Nm, p["model_arr"], p["len_arr"], _ptr(p["q_init"]), _ptr(p["meas"]), _ptr(p["weight"]),
                                            *[_ptr(a) for a in out.values()], stats)
        _check(st, "cpe_solve_ragged_host", allow=(abi.OK, abi.MAX_ITER, abi.NUMERICAL))
        return dict(status=st, **unpad_kinetic(out, p["lens"], p["cams"]), stats=list(stats)[:B], padded=out)
