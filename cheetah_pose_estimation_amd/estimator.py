"""Host-side mirror of the reference's estimator API (layer L3, acinoset_opt.py) on top of the HIP back end.

Same entry points, argument meaning and return convention as the reference so that its drivers
(`run_dataset.py:1143-1231` etc., `tests.ipynb`) call in unchanged:

    est = init_trajectory(root_dir, data_path, cheetah_name, kinetic_dataset, solver_path, ...)   # acinoset_opt.py:413-430
    ok  = estimate_kinematics(est, ...)                                                            # acinoset_opt.py:539-547

and the on-disk contract is kept: `fte.pickle` (keys of acinoset_opt.py:330-361) and `cam{i}_fte.csv` in
DeepLabCut layout (acinoset_misc.py:1346-1407).  Where the reference builds a Pyomo model and spawns IPOPT
(acinoset_opt.py:508-525, :611-617) this module fills dense tensors and calls `cpe_solve` through the C ABI.
Everything numerical on the solve path runs on the GPU; numpy here only moves data in and out of files.
"""
import json
import os
import pickle
from dataclasses import dataclass, field
from glob import glob
from time import time
from typing import Sequence, Dict, List, Optional, Tuple

import numpy as np

from . import _lib, abi, skeleton


class _ArrayOnlyUnpickler(pickle.Unpickler):
    """`fte.pickle` reader that executes nothing from the file: only the globals a dict of numpy arrays / floats needs are
    resolvable; anything else (a `fte.pickle` may come from an untrusted tree laid out like the reference's data) raises."""
    _ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"fte.pickle: global {module}.{name} is not allowed (arrays, numbers, str, dict, list only)")


def load_result_pickle(path: str) -> dict:
    """read back a result file written by CheetahEstimator.save (plain dict of arrays and numbers)"""
    with open(path, "rb") as fh:
        return _ArrayOnlyUnpickler(fh).load()


# ---- data classes mirroring acinoset_misc.py:40-73 ---------------------------------------------------
@dataclass
class TrajectoryParams:
    data_dir: str
    start_frame: int
    end_frame: int
    total_length: int
    dlc_thresh: float
    sync_offset: Optional[List[Dict]]
    hand_labeled_data: bool
    kinetic_dataset: bool
    enable_shutter_delay_estimation: bool
    enable_ppms: bool


@dataclass
class Scene:
    scene_fpath: str
    k_arr: np.ndarray
    d_arr: np.ndarray
    r_arr: np.ndarray
    t_arr: np.ndarray
    cam_res: Tuple[int, int]
    fps: float
    n_cams: int
    cam_idx: Optional[int]


# ---- file formats ---------------------------------------------------------------------------------------
def load_scene(fpath: str):
    """`*_cam_scene_sba.json` (acinoset_misc.py:1496-1516)."""
    with open(fpath, "r", encoding="utf-8") as f:
        data = json.load(f)
    cams = data["cameras"]
    arr = lambda k: np.array([c[k] for c in cams], dtype=np.float64)
    return arr("k"), arr("d"), arr("r"), arr("t"), tuple(data["camera_resolution"])


def find_scene_file(dir_path: str, scene_fname: Optional[str] = None):
    """walk up from the sequence directory to `extrinsic_calib/` (acinoset_misc.py:1519-1544)."""
    if scene_fname is None:
        n_cams = len(glob(os.path.join(dir_path, "cam[1-9].mp4")))
        scene_fname = f"{n_cams}_cam_scene_sba.json" if n_cams else "[1-9]_cam_scene*.json"
    d = dir_path
    while d and d != os.path.sep:
        files = sorted(f for f in glob(os.path.join(d, "extrinsic_calib", scene_fname)) if "before_corrections" not in f)
        if files:
            k, dd, r, t, res = load_scene(files[-1])
            return k, dd, r, t, res, int(os.path.basename(files[-1])[0]), files[-1]
        nd = os.path.dirname(d)
        if nd == d:
            break
        d = nd
    raise FileNotFoundError(os.path.join("extrinsic_calib", scene_fname))


def load_dlc_table(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """One DeepLabCut file -> (frame index [F], values [F, 75]) with columns (x, y, likelihood) x 25 body parts.
    `.h5` needs PyTables (as in the reference, acinoset_misc.py:206); the `.csv` twin DeepLabCut writes beside
    it (3 header rows: scorer / bodyparts / coords) is read without it."""
    if path.endswith(".h5"):
        import pandas as pd
        df = pd.read_hdf(path)
        return np.asarray(df.index), df.to_numpy(dtype=np.float64)
    rows = np.genfromtxt(path, delimiter=",", skip_header=3)
    return rows[:, 0].astype(np.int64), rows[:, 1:].astype(np.float64)


def load_hand_labeled_table(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """One hand-labelled file (`dlc_hand_labeled/cam?.h5`, acinoset_misc.py:1545-1552) in the layout of `load_dlc_table`: (frame index [F], values
    [F, 75]).  The file holds (x, y) per body part and is indexed by image names (`.../img012.png`): the reference numbers its rows from the
    digits [3:6] of the first name to those of the last.  Likelihood 1 for a labelled point; a point without a label (NaN) gets likelihood 0 --
    DEVIATION: the reference compares with `== np.nan` (acinoset_misc.py:221, :247), which is never true, so its NLP would be handed the NaN.
    `.h5` needs PyTables; the `.csv` twin DeepLabCut writes beside it (`CollectedData_*.csv`: header rows scorer / bodyparts / coords, one or
    three leading name columns) is read without it."""
    if path.endswith(".h5"):
        import pandas as pd
        df = pd.read_hdf(path)
        names = [ix[-1] if isinstance(ix, tuple) else str(ix) for ix in df.index]
        xy = df.to_numpy(dtype=np.float64)
    else:
        import csv
        with open(path, "r", encoding="utf-8", newline="") as f:
            rows = list(csv.reader(f))
        coords = rows[2]
        first = next(i for i, c in enumerate(coords) if c.strip() in ("x", "y"))
        body = [r for r in rows[3:] if r]
        names = [r[first - 1] for r in body]
        xy = np.array([[float(v) if v.strip() not in ("", "nan", "NaN") else np.nan for v in r[first:]] for r in body], dtype=np.float64)
    base = lambda nm: os.path.basename(str(nm).replace("\\", "/"))
    start, end = int(base(names[0])[3:6]), int(base(names[-1])[3:6])
    assert end - start + 1 == xy.shape[0], f"{path}: {xy.shape[0]} rows for frames {start}..{end}"
    n_parts = xy.shape[1] // 2
    vals = np.zeros((xy.shape[0], 3 * n_parts))
    vals[:, 0::3], vals[:, 1::3] = xy[:, 0::2], xy[:, 1::2]
    ok = np.isfinite(xy[:, 0::2]) & np.isfinite(xy[:, 1::2])
    vals[:, 2::3] = ok
    vals[:, 0::3][~ok] = 0.0; vals[:, 1::3][~ok] = 0.0
    return np.arange(start, end + 1, dtype=np.int64), vals


def dlc_paths(dlc_dir: str) -> List[str]:
    h5 = sorted(glob(os.path.join(dlc_dir, "*.h5")))
    try:
        import tables  # noqa: F401
        if h5:
            return h5
    except Exception:
        pass
    csv = sorted(glob(os.path.join(dlc_dir, "*.csv")))
    return csv if csv else h5


def build_measurements(tables, start_frame: int, end_frame: int, sync_offset, n_cams: int, dlc_thresh: float,
                       kinetic_dataset: bool, cam_idx: Optional[int] = None, device: int = 0):
    """meas[N,C,24,2] and meas_err_weight[N,C,24] exactly as `init_measurements` / `init_meas_weights` fill the
    Pyomo params (acinoset_misc.py:211-256): row (n + start_frame - sync_offset[c]) of camera c, DLC column of
    each marker (`get_dlc_marker_indices`), weight 1/R_pw[0][l] if likelihood > dlc_thresh else 0.  The gather runs on
    the GPU (cpe_tensorise_dlc), one launch per camera table."""
    off = [0] * n_cams
    if sync_offset is not None:
        for o in sync_offset:
            off[o["cam"]] = o["frame"]
    N = end_frame - start_frame
    cams = list(range(n_cams)) if cam_idx is None else [cam_idx]
    sigma = skeleton.measurement_sigma(24, kinetic_dataset)
    col = [skeleton.DLC_INDEX[m] for m in skeleton.MARKERS]
    from .synth import make_cameras
    h = _lib.Handle(skeleton.build_skeleton("phantom", 24), make_cameras(1), device=device)        # only the marker count is used
    try:
        return h.tensorise_dlc_host([tables[c][1] for c in cams], [start_frame - off[c] for c in cams], col, 1.0 / sigma, dlc_thresh, N)
    finally:
        h.close()


def load_pairwise_table(path: str):
    """pairwise predictions of ONE camera (`dlc_pw/cam?DLC_....pickle`, acinoset_misc.py:202-205): per table row the DLC pose row [75] and the
    pairwise offsets `pws` [1, 25, 25, 2] (offset from body part a to body part b).  Accepted here: an `.npz` with arrays `pose [rows, 75]`,
    `pws [rows, 25, 25, 2]`, or the reference's pickle read with the arrays-only unpickler (a list of {"pose", "pws"} records)."""
    if path.endswith(".npz"):
        z = np.load(path, allow_pickle=False)
        return np.asarray(z["pose"], dtype=np.float64), np.asarray(z["pws"], dtype=np.float64)
    recs = load_result_pickle(path)
    pose = np.array([np.asarray(r["pose"], dtype=np.float64).ravel() for r in recs])
    pws = np.array([np.asarray(r["pws"], dtype=np.float64).reshape(25, 25, 2) for r in recs])
    return pose, pws


def build_pairwise_measurements(pw_tables, start_frame: int, end_frame: int, sync_offset, n_cams: int, dlc_thresh: float, kinetic_dataset: bool,
                                cam_idx: Optional[int] = None):
    """meas[N, 2, C, 24, 2] and weight[N, 2, C, 24] of the two pairwise pseudo-measurements w = 2, 3 as `init_measurements` / `init_meas_weights`
    fill them (acinoset_misc.py:211-256): marker l is predicted from body part b = pair_dict[marker][w - 2] as pose[b] + pws[b, dlc index of the
    marker]; weight 1 / R_pw[w - 1][l] if the likelihood of b exceeds the threshold.  Host gather over a few thousand numbers."""
    off = [0] * n_cams
    if sync_offset is not None:
        for o in sync_offset:
            off[o["cam"]] = o["frame"]
    N = end_frame - start_frame
    cams = list(range(n_cams)) if cam_idx is None else [cam_idx]
    meas = np.zeros((N, 2, len(cams), 24, 2)); weight = np.zeros((N, 2, len(cams), 24))
    own = np.array([skeleton.DLC_INDEX[m] for m in skeleton.MARKERS])
    for w in (0, 1):
        sig = skeleton.pairwise_sigma(w + 1, kinetic_dataset)
        src = np.array([skeleton.PAIRWISE[m][w] for m in skeleton.MARKERS])
        for ci, c in enumerate(cams):
            pose, pws = pw_tables[c]
            rows = np.arange(N) + start_frame - off[c]
            ok = (rows >= 0) & (rows < pose.shape[0])
            r = np.clip(rows, 0, pose.shape[0] - 1)
            xy = np.stack([pose[r][:, 0::3][:, src] + pws[r][:, src, own, 0], pose[r][:, 1::3][:, src] + pws[r][:, src, own, 1]], axis=-1)
            lik = pose[r][:, 2::3][:, src]
            good = ok[:, None] & np.isfinite(xy).all(-1)
            meas[:, w, ci] = np.where(good[..., None], xy, 0.0)
            weight[:, w, ci] = np.where(good & (lik > dlc_thresh), 1.0 / sig[None, :], 0.0)
    return meas, weight


def scene_cameras(scene: Scene, kinetic_dataset: bool, hand_labeled: bool = False):
    """abi.Camera array from the scene; multipliers [1,1,.6,.6] for the kinetic dataset (acinoset_misc.py:462-464) -- not with hand-labelled
    points, whose squared loss has no multiplier (:471-474)."""
    idx = list(range(scene.n_cams)) if scene.cam_idx is None else [scene.cam_idx]
    cams = (abi.Camera * len(idx))()
    mult = [1.0, 1.0, 0.6, 0.6] if kinetic_dataset and not hand_labeled else [1.0] * 6
    for j, c in enumerate(idx):
        cam = cams[j]
        cam.model = abi.CAM_PINHOLE if kinetic_dataset else abi.CAM_FISHEYE
        K = scene.k_arr[c]
        cam.fx, cam.fy, cam.cx, cam.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        D = np.asarray(scene.d_arr[c]).ravel()
        for i in range(min(4, len(D))):
            cam.D[i] = D[i]
        for i in range(9):
            cam.R[i] = np.asarray(scene.r_arr[c]).reshape(-1)[i]
        for i in range(3):
            cam.t[i] = np.asarray(scene.t_arr[c]).reshape(-1)[i]
        cam.mult = mult[c] if c < len(mult) else 1.0
    return cams


# ---- initial guess (acinoset_misc.py:381-456) ------------------------------------------------------------------------
def create_trajectory_estimate(tables, params: TrajectoryParams, scene: Scene, base_length: float, device: int = 0):
    """x, y, z, psi initial estimate from the `spine` marker (acinoset_misc.py:381-456): pairwise triangulation
    over the camera ring (multi-view) or back-projection to 3 m depth (monocular) -- both on the GPU, cpe_triangulate --
    then the per-frame mean over the pairs, a cubic / linear smoothing spline, heading from finite differences (+pi: the
    skeleton's head points along -x)."""
    from scipy.interpolate import UnivariateSpline
    kin = params.kinetic_dataset
    col = skeleton.DLC_INDEX["spine"]
    off = [0] * scene.n_cams
    if params.sync_offset is not None:
        for o in params.sync_offset:
            off[o["cam"]] = o["frame"]
    obs = {}
    for c in range(scene.n_cams):
        idx, vals = tables[c]
        ok = vals[:, 3 * col + 2] > params.dlc_thresh
        obs[c] = {int(f) + off[c]: vals[i, 3 * col:3 * col + 2] for i, f in enumerate(idx) if ok[i]}
    # one flat list of (frame, camera a, camera b, pixel a, pixel b) records for a single launch
    rec_f, rec_a, rec_b, rec_ua, rec_ub = [], [], [], [], []
    if scene.cam_idx is None:
        ncam = 2 if kin else scene.n_cams                       # kinetic dataset: near-side cameras only (:399-401)
        for a, b in [(i % ncam, (i + 1) % ncam) for i in range(ncam)]:
            for f in sorted(set(obs[a]) & set(obs[b])):
                rec_f.append(f); rec_a.append(a); rec_b.append(b); rec_ua.append(obs[a][f]); rec_ub.append(obs[b][f])
    else:
        c = scene.cam_idx
        for f in sorted(obs[c]):
            rec_f.append(f); rec_a.append(c); rec_b.append(-1); rec_ua.append(obs[c][f]); rec_ub.append(obs[c][f])
    if not rec_f:
        raise ValueError("no usable spine detections for the initial trajectory estimate")
    f32 = lambda a: np.array(a, dtype=np.float32).astype(np.float64)          # the reference hands float32 pixels to OpenCV (:1467-1468)
    all_cams = scene_cameras(Scene(scene.scene_fpath, scene.k_arr, scene.d_arr, scene.r_arr, scene.t_arr, scene.cam_res,
                                   scene.fps, scene.n_cams, None), kin)
    h = _lib.Handle(skeleton.build_skeleton("phantom", 24), all_cams, device=device)      # only the camera table is used
    try:
        X = h.triangulate_host(rec_a, rec_b, f32(rec_ua), f32(rec_ub), depth=3.0)
    finally:
        h.close()
    rec_f = np.array(rec_f)
    frames = np.unique(rec_f)
    xyz = np.array([X[rec_f == f].mean(axis=0) for f in frames])             # groupby(frame).mean() (:1491)
    xyz[:, 0] += base_length / 2.0                                   # :424
    k = 1 if kin else 3
    fr = np.arange(params.end_frame)
    est = [np.asarray(UnivariateSpline(frames, xyz[:, d], k=k)(fr)) for d in range(3)]
    psi = np.arctan2(np.diff(est[1]) * scene.fps, np.diff(est[0]) * scene.fps)
    psi = np.pi + np.append(psi, psi[-1])
    return est[0], est[1], est[2], psi


# ---- estimator object ---------------------------------------------------------------------------------------
@dataclass
class CheetahEstimator:
    """Counterpart of acinoset_opt.CheetahEstimator (acinoset_opt.py:21-70): holds the problem tensors instead
    of a Pyomo model."""
    name: str
    data_path: str
    params: TrajectoryParams
    scene: Scene
    skeleton: abi.Skeleton
    cams: object
    meas: np.ndarray                 # [N, C, 24, 2]
    weight: np.ndarray               # [N, C, 24]
    scale_forces_by: float
    kinematic_model: bool
    tables: object = None
    device: int = 0
    opt_time_s: float = 0.0
    shutter_delay: Optional[np.ndarray] = None   # [C] seconds, set by estimate_kinematics when enable_shutter_delay_estimation
    synthesised_grf: Optional[dict] = None       # {foot: GRFz per frame}: the profile estimate_kinetics(joint_estimation=False) prescribed (acinoset_opt.py:823)
    costs: Dict[str, float] = field(default_factory=dict)
    result: Optional[dict] = None
    com_pos: Optional[np.ndarray] = None
    com_vel: Optional[np.ndarray] = None
    enable_eom_slack: bool = True
    bound_eom_error: Optional[Tuple[float, float]] = None
    kinetic: Optional[dict] = None          # node forces of the last estimate_kinetics (tau, lam, grf, slack, stance)
    # estimate_kinematics(uncertainty=True): dict(cov_u [N, 28, 28], u_std [N, 28], positions_cov [N, L, 3, 3], positions_std [N, L, 3], ridge) --
    # the marginal posterior covariance of every frame's reduced coordinates and marker positions (cpe_covariance); None where it does not exist
    # estimate_kinetics / estimate_grf(uncertainty=True): the same fields from cpe_covariance_kinetic plus tau_std [N, n_motors], lambda_std [N, 26],
    # grf_std [N, 4, 3] (net z, x, y per foot) and tau_cov [N, n_motors, n_motors]; 0.0 where a force is not an unknown of that node
    # uncertainty_rates=True adds RATE_FIELDS (cpe_rate_covariance): du_std, ddu_std [N, 28], velocities_cov / _std [N, L, 3(, 3)], com_cov / _std
    # [N, 3(, 3)], and, aligned with com_vel, com_vel_cov / _std [N-1, 3(, 3)] and speed_std [N-1]
    # uncertainty_spans adds SPAN_FIELDS (cpe_covariance_columns, span_uncertainty): per span (first, last) the centre of mass's displacement, distance,
    # mean velocity and mean speed with covariances / standard deviations, and span_positions_displacement_cov / _std [S, L, 3(, 3)]
    # uncertainty_lengths adds LENGTH_FIELDS (cpe_scale_response, cpe_covariance_add_scales): the covariance marginalised over the fitted lengths
    uncertainty: Optional[dict] = None
    # estimate_kinematics(uncertainty=True, uncertainty_samples=K): SAMPLE_FIELDS, K trajectories drawn from the posterior (cpe_band_sample,
    # cpe_posterior_samples): du [K, N, 28], q [K, N, nq], x [K, N, 28], positions [K, N, L, 3], com_pos [K, N, 3], seed, ridge; None where not
    # asked for or where the covariance has no factor
    samples: Optional[dict] = None
    # calibrate_lengths / estimate_kinematics(estimate_lengths=True): the scale of every segment group of length_groups (skeleton.LENGTH_GROUPS'
    # form), the covariance of the scales (the inverse of the reduced system + prior), and the model name the skeleton was built from; None: the
    # parameter file's lengths.  The later stages build their inertia and mass tables with these scales.
    length_scale: Optional[np.ndarray] = None
    length_scale_cov: Optional[np.ndarray] = None
    length_groups: Optional[tuple] = None
    # how that fit ended: dict(converged, rounds, prior_sigma, ridge, objective).  converged False: the loop stopped at max_rounds or found no
    # descent step; the scales are then the last iterate, not a minimiser (a warning is issued, and skeleton_scale.json says so)
    length_calibration: Optional[dict] = None
    # detection_report: DETECTION_FIELDS, every marker's predicted pixel in every camera with its covariance, the leave-one-out prediction of every
    # detection and its chi-square distance (cpe_detection_report); None until asked for
    detections: Optional[dict] = None

    def get_objective_cost(self) -> float:
        return float(self.result["stats"][0].cost) if self.result else float("nan")

    def relative_angles(self, q: np.ndarray) -> np.ndarray:
        """x (28) of acinoset_misc.py:508-528 + mask :1699-1757, linear in q"""
        sk = self.skeleton
        ind = skeleton.independent_dofs(sk)
        ref = np.array(sk.rel_ref[:sk.nq]); sgn = np.array(sk.rel_sign[:sk.nq])
        rel = np.where(ref < 0, q, sgn * (q - q[..., np.maximum(ref, 0)]))
        return rel[..., ind]

    def estimate_grf(self, plot: bool = False, monocular: bool = False, out_dir_prefix: Optional[str] = None,
                     contacts: Optional[dict] = None):
        """Per-frame ground-reaction-force fit, same signature and return value as CheetahEstimator.estimate_grf
        (acinoset_opt.py:176-270): reads the kinematic result `fte_kinematic[_<cam>]/fte.pickle` and the contact windows of
        `grf/autogen-contact.json` (written by the reference's determine_contacts; may be passed as `contacts` instead),
        fits the forces of the feet in contact on the GPU (cpe_grf_fit) and returns ({foot: [GRFz per frame]},
        {foot: [[4 friction components] per frame]}) in body weights."""
        params, scene, sk = self.params, self.scene, self.skeleton
        data_dir = params.data_dir if out_dir_prefix is None else os.path.join(out_dir_prefix, self.data_path)
        sub = "fte_kinematic" if not monocular else f"fte_kinematic_{scene.cam_idx}"
        fte = load_result_pickle(os.path.join(data_dir, sub, "fte.pickle"))       # restricted unpickler: arrays and numbers only
        if contacts is None:
            with open(os.path.join(data_dir, "grf", "autogen-contact.json"), "r", encoding="utf-8") as fh:
                contacts = json.load(fh)
        start_frame, end_frame = contacts["start_frame"], contacts["end_frame"]
        N = end_frame - start_frame
        feet = [f"{name}_foot" for name in skeleton.FEET]
        flags = np.zeros((N, len(feet)), np.int32)
        for i, f in enumerate(feet):
            for seq in (contacts["contacts"].get(f) or []):           # [first, last, foot index, "leading"|"trailing"] (acinoset_misc.py:812)
                a, b = int(seq[0]), int(seq[1])
                lo, hi = max(a - start_frame, 0), min(b - start_frame, N)
                if hi > lo:
                    flags[lo:hi, i] = 1
        gopt = skeleton.grf_options(self.name, **_length_kw(self))            # load_params falls back to the generic animal
        h = _lib.Handle(sk, self.cams, device=self.device)
        try:
            gz, gxy, res = h.grf_fit_host(gopt, fte["q"][None, :N], fte["dq"][None, :N], fte["ddq"][None, :N], flags[None])
        finally:
            h.close()
        self.grf_residual = res[0]
        grfz_est = {f: [float(v) for v in gz[0, :, i]] for i, f in enumerate(feet)}
        grfxy_est = {f: [[float(v) for v in row] for row in gxy[0, :, i]] for i, f in enumerate(feet)}
        return grfz_est, grfxy_est

    def folded_meas_err(self) -> np.ndarray:
        """slack_meas as the reference stores it, [N, C, 24, 2, W] (acinoset_opt.py:325): the solver's camera axis is [w * C + c] with PPM"""
        me = self.result["meas_err"][0]
        W = 3 if self.params.enable_ppms else 1
        C1 = me.shape[1] // W
        return np.ascontiguousarray(np.stack([me[:, w * C1:(w + 1) * C1] for w in range(W)], axis=-1))

    def robot_data(self) -> dict:
        """`cheetah.pickle` of a physics-based run: the layout `System3D.save_data_to_file` gives the reference's files (SURVEY 8b:
        name, description, nfe, ncp, hm, hm0, links: [{name, is_base, mass, length, radius, q, dq, ddq, Fr, nodes}]): per link the
        collocation variables, the joint constraint forces the link takes part in, and its nodes -- a motor (`Tc`) or a foot (`GRFz`,
        `GRFxy`, `foot_height`).  The library that defines the exact field shapes is absent (physical_education): unpinned."""
        sk, res, kin = self.skeleton, self.result, self.kinetic
        q, dq, ddq = res["q"][0], res["dq"][0], res["ddq"][0]
        N = q.shape[0]
        p = skeleton.load_params(self.name, **_length_kw(self))
        groups = dict(skeleton.motor_groups())
        links = []
        for i, name in enumerate(skeleton.LINKS):
            lp = skeleton._link_param(p, name)
            sl = slice(0, 6) if i == 0 else slice(3 + 3 * i, 6 + 3 * i)
            rows = [r for r, (par, ch) in enumerate(skeleton.constraint_rows(sk)) if i in (par, ch)]
            nodes = []
            for mname, cols in groups.items():
                if mname.startswith(name + "_"):
                    nodes.append(dict(name=mname, Tc=kin["tau"][:, cols]))
            if name in skeleton.FEET:
                k = skeleton.FEET.index(name)
                mk = skeleton.MARKERS.index(skeleton.FOOT_MARKERS[k])
                nodes.append(dict(name=f"{name}_foot", GRFz=kin["grf"][:, k, 0], GRFxy=kin["grf"][:, k, 1:5],
                                  foot_height=res["positions"][0][:, mk, 2] - kin["ground_height"], stance=kin["stance"][:, k]))
            links.append(dict(name=name, is_base=i == 0, meta=[], mass=lp["mass"], length=lp["length"], radius=lp["radius"],
                              q=q[:, sl], dq=dq[:, sl], ddq=ddq[:, sl], Fr=kin["lam"][:, rows], nodes=nodes))
        h = 1.0 / self.scene.fps
        return dict(name=f"cheetah-{self.name}", description="Auto Save", repr="cheetah_pose_estimation_amd physics-based estimate",
                    nfe=N, ncp=1, hm=np.full(N, h), hm0=h, slack_eom=kin["slack"], links=links)

    def save(self, out_dir: str, fname: str = "fte", out_dir_prefix: Optional[str] = None):
        """fte.pickle + cam*_fte.csv, acinoset_opt.py:278-373."""
        res, params, scene = self.result, self.params, self.scene
        if out_dir_prefix:
            out_dir = os.path.join(out_dir_prefix, self.data_path, out_dir or "fte")
        else:
            out_dir = os.path.join(params.data_dir, out_dir or "fte")
        os.makedirs(out_dir, exist_ok=True)
        q, dq, ddq = res["q"][0], res["dq"][0], res["ddq"][0]
        tau = {}
        if self.kinetic is not None:                                # {motor name: [N, components]} (acinoset_opt.py:317-324)
            for name, cols in skeleton.motor_groups():
                tau[name] = np.ascontiguousarray(self.kinetic["tau"][:, cols])
        output = dict(positions=res["positions"][0], x=self.relative_angles(q), dx=self.relative_angles(dq),
                      ddx=self.relative_angles(ddq), q=q, dq=dq, ddq=ddq, com_pos=self.com_pos, com_vel=self.com_vel,
                      tau=tau, meas_err=self.folded_meas_err(), obj_cost=self.get_objective_cost(),
                      processing_time_s=self.opt_time_s, start_frame=params.start_frame)
        with open(os.path.join(out_dir, f"{fname}.pickle"), "wb") as f:
            pickle.dump(output, f)
        if not self.kinematic_model and self.kinetic is not None:
            with open(os.path.join(out_dir, "cheetah.pickle"), "wb") as f:      # robot.save_data_to_file (acinoset_opt.py:372-373)
                pickle.dump(self.robot_data(), f)
        off = [0] * scene.n_cams
        if params.sync_offset is not None:
            for o in params.sync_offset:
                off[o["cam"]] = o["frame"]
        all_cams = scene_cameras(Scene(scene.scene_fpath, scene.k_arr, scene.d_arr, scene.r_arr, scene.t_arr, scene.cam_res,
                                       scene.fps, scene.n_cams, None), params.kinetic_dataset)
        pos = res["positions"][0]
        hw = _lib.Handle(self.skeleton, all_cams, device=self.device)          # every camera of the scene, also for monocular runs
        try:
            delays = self.shutter_delay
            if delays is None:
                uv_all = hw.reproject_host(pos[None])[0]                       # [N, C, 24, 2] on the GPU (cpe_reproject)
            else:
                # positions_arr[c] = markers + q'_base tau_c + q''_base tau_c^2 (acinoset_opt.py:342-352), from node 2 on as the solve models it
                shift = np.zeros((scene.n_cams,) + pos.shape)
                for c in range(scene.n_cams):
                    d3 = dq[:, 0:3] * delays[c] + ddq[:, 0:3] * delays[c] ** 2
                    d3[:2] = 0.0
                    shift[c] = pos + d3[:, None, :]
                uv_c = hw.reproject_host(shift)                                # [C, N, C, 24, 2]: camera c reads its own displaced copy
                uv_all = np.stack([uv_c[c, :, c] for c in range(scene.n_cams)], axis=1)
        finally:
            hw.close()
        for i in range(scene.n_cams):
            uv = uv_all[:, i].copy()
            bad = (uv > np.array(scene.cam_res)) | (uv < 0)
            uv[bad.any(-1)] = np.nan                                # acinoset_misc.py:1385-1386
            n_frames = pos.shape[0]
            path = os.path.join(out_dir, f"cam{i + 1}_{fname}.csv")
            with open(path, "w") as f:                              # DLC MultiIndex layout (:1373-1399)
                f.write("bodyparts," + ",".join(f"{m},{m},{m}" for m in skeleton.MARKERS) + "\n")
                f.write("coords," + ",".join("x,y,likelihood" for _ in skeleton.MARKERS) + "\n")
                for n in range(n_frames):
                    row = ",".join((("" if np.isnan(uv[n, l, 0]) else repr(float(uv[n, l, 0]))) + "," +
                                    ("" if np.isnan(uv[n, l, 1]) else repr(float(uv[n, l, 1]))) + ",") for l in range(24))
                    f.write(f"{params.start_frame - off[i] + n},{row}\n")
        return out_dir


def init_trajectory(root_dir: str, data_path: str, cheetah_name: str, kinetic_dataset: bool, solver_path: Optional[str] = None,
                    start_frame: int = -1, end_frame: int = -1, dlc_thresh: float = 0.5,
                    include_camera_constraints: bool = True, enable_eom_slack: bool = True, kinematic_model: bool = False,
                    monocular_enable: bool = False, override_monocular_cam: Optional[int] = None,
                    disable_contact_lcp: bool = True, bound_eom_error: Optional[Tuple[float, float]] = None,
                    shutter_delay_estimation: bool = False, enable_ppm: bool = False, hand_labeled_data: bool = False,
                    device: int = 0) -> CheetahEstimator:
    """Same signature and meaning as acinoset_opt.init_trajectory (acinoset_opt.py:413-536).  `solver_path`
    (the IPOPT binary of the reference) is accepted and ignored."""
    if hand_labeled_data and enable_ppm:
        raise NotImplementedError("hand-labelled points together with pairwise predictions (there are none for hand labels)")
    if shutter_delay_estimation and enable_ppm and not monocular_enable:
        raise NotImplementedError("shutter delays together with pairwise predictions: the three measurement slices of a camera would share one delay")
    if cheetah_name not in ("jules", "phantom", "shiraz", "arabia"):
        cheetah_name = "acinoset"                                   # acinoset_opt.py:455-456
    model_name = f"{cheetah_name}-02" if kinetic_dataset else cheetah_name
    data_dir = os.path.join(root_dir, data_path)
    cam_idx, sync_offset = None, None
    if start_frame < 0 or end_frame < 0:
        with open(os.path.join(data_dir, "metadata.json"), "r", encoding="utf-8") as f:
            md = json.load(f)
        start_frame, end_frame, sync_offset = md["start_frame"], md["end_frame"], md["cam_sync"]
        cam_idx = md["monocular_cam"] if monocular_enable else None
        cam_idx = cam_idx if override_monocular_cam is None else override_monocular_cam
    total_length = end_frame - start_frame
    dlc_dir = os.path.join(data_dir, "dlc_hand_labeled" if hand_labeled_data else "dlc")          # acinoset_opt.py:479
    assert os.path.exists(dlc_dir), dlc_dir
    k_arr, d_arr, r_arr, t_arr, cam_res, n_cams, scene_fpath = find_scene_file(data_dir)
    fps = 200.0
    if not kinetic_dataset and "2019" in data_path:
        fps = 120.0
    elif not kinetic_dataset and "2017" in data_path:
        fps = 90.0                                                   # acinoset_opt.py:483-487
    d_arr = d_arr.reshape((n_cams, -1))
    params = TrajectoryParams(data_dir, start_frame, end_frame, total_length, dlc_thresh, sync_offset, hand_labeled_data,
                              kinetic_dataset, shutter_delay_estimation, enable_ppm)
    scene = Scene(scene_fpath, k_arr, d_arr, r_arr, t_arr, cam_res, fps, n_cams, cam_idx)
    paths = dlc_paths(dlc_dir)
    assert n_cams == len(paths), f"# of dlc files != # of cams in {scene_fpath}"
    sk = skeleton.build_skeleton(model_name, 24, kinetic_dataset)
    if hand_labeled_data:
        # acinoset_misc.py:217-222, :243-246, :471-474: rows by POSITION n + start_frame of the labelled table, no camera offsets, every labelled point at
        # weight 1 / R, squared loss (w r)^2.  The kernels evaluate rho(w r) with rho(e) = e^2 / 2 below the first knot: the knots go out of reach
        # (_kin_prepare) and the weights carry a factor sqrt(2).
        tables = [load_hand_labeled_table(p) for p in paths]
        pos = [(np.arange(len(t[0]), dtype=np.int64), t[1]) for t in tables]
        meas, weight = build_measurements(pos, start_frame, end_frame, None, n_cams, 0.5, kinetic_dataset, cam_idx, device=device)
        weight = weight * np.sqrt(2.0)
    else:
        tables = [load_dlc_table(p) for p in paths]
        meas, weight = build_measurements(tables, start_frame, end_frame, sync_offset, n_cams, dlc_thresh, kinetic_dataset, cam_idx, device=device)
    cams = scene_cameras(scene, kinetic_dataset, hand_labeled_data)
    if enable_ppm:
        # m.W = RangeSet(3) (acinoset_misc.py:179): the SAME projected marker is compared with three detections -- its own and two pairwise
        # predictions --, each with its own weight.  For the kernels that is every camera three times with identical parameters: cameras
        # [w * C + c], measurement slices [N, w * C + c, 24, ...]; CheetahEstimator.save folds the residuals back to [N, C, 24, 2, 3].
        pw_paths = sorted(glob(os.path.join(dlc_dir + "_pw", "*.npz"))) or sorted(glob(os.path.join(dlc_dir + "_pw", "*.pickle")))
        assert n_cams == len(pw_paths), f"# of pairwise files != # of cams in {scene_fpath}"
        pm, pw = build_pairwise_measurements([load_pairwise_table(p) for p in pw_paths], start_frame, end_frame, sync_offset, n_cams, dlc_thresh,
                                             kinetic_dataset, cam_idx)
        C1 = len(cams)
        meas = np.ascontiguousarray(np.concatenate([meas] + [pm[:, w] for w in range(2)], axis=1))
        weight = np.ascontiguousarray(np.concatenate([weight] + [pw[:, w] for w in range(2)], axis=1))
        cams3 = (abi.Camera * (3 * C1))()
        for w in range(3):
            for c in range(C1):
                cams3[w * C1 + c] = cams[c]
        cams = cams3
    total_mass = sum(sk.mass[i] for i in range(sk.n_links))
    return CheetahEstimator(cheetah_name, data_path, params, scene, sk, cams, meas, weight,
                            total_mass * 9.81, kinematic_model, tables, device, enable_eom_slack=enable_eom_slack, bound_eom_error=bound_eom_error)


def _kin_prepare(est: CheetahEstimator, monocular_constraints: bool, disable_pose_prior: bool, disable_motion_prior: bool,
                 pose_model_num_components: int, motion_model_window_size: int, motion_model_sparse_solution: bool,
                 q_init: Optional[np.ndarray], options: Optional[abi.Options]):
    """what estimate_kinematics sets up before the solver call (acinoset_opt.py:565-608): priors, initial guess, options"""
    params, scene, sk = est.params, est.scene, est.skeleton
    pri = None
    if monocular_constraints and scene.cam_idx is not None and not (disable_pose_prior and disable_motion_prior):
        # acinoset_opt.py:593-600.  The fitted numbers of the defaults ship as package data (tools/fit_priors.py re-runs the reference's recipe:
        # 5-component GMM, window-4 multi-task lasso); another size -- the grid search of run_dataset.py:814-915 -- is fitted here as the reference
        # does at run time (priors.fit_priors: up to 8 components, windows up to 6 frames) and cached.
        from . import priors as _priors
        default = (disable_pose_prior or pose_model_num_components == 5) and \
            (disable_motion_prior or (motion_model_window_size == 4 and motion_model_sparse_solution))
        if default:
            pri = _priors.load_priors(pose=not disable_pose_prior, motion=not disable_motion_prior)
        else:
            path = _priors.fit_priors(5 if disable_pose_prior else pose_model_num_components, 4 if disable_motion_prior else motion_model_window_size,
                                      True if disable_motion_prior else motion_model_sparse_solution)
            pri = _priors.load_priors(pose=not disable_pose_prior, motion=not disable_motion_prior, path=path)
    N = params.end_frame - params.start_frame
    if q_init is None:
        base_len = 2.0 * abs(sk.marker_off[5][0])
        x, y, z, psi = create_trajectory_estimate(est.tables, params, scene, base_len, device=est.device)
        q_init = np.zeros((N, sk.nq))                               # acinoset_opt.py:574-583
        sl = slice(params.start_frame, params.start_frame + N)
        q_init[:, 0], q_init[:, 1], q_init[:, 2] = x[sl], y[sl], z[sl]
        for i in range(sk.n_links):
            q_init[:, 3 + 3 * i + 2] = psi[sl]
    opts = options if options is not None else abi.default_options(scene.fps)
    opts.h = 1.0 / scene.fps
    if params.hand_labeled_data:
        opts.loss_a, opts.loss_b, opts.loss_c = 1e6, 2e6, 3e6          # squared loss: no residual reaches the first knot (init_trajectory)
    return q_init, opts, pri


SPAN_FIELDS = ("span_frames", "span_seconds", "span_com_displacement", "span_com_displacement_cov", "span_com_displacement_std", "span_distance",
               "span_distance_std", "span_mean_velocity", "span_mean_velocity_cov", "span_mean_velocity_std", "span_mean_speed", "span_mean_speed_std",
               "span_positions_displacement_cov", "span_positions_displacement_std")
RATE_FIELDS = ("du_std", "ddu_std", "velocities_cov", "velocities_std", "com_cov", "com_std", "com_vel_cov", "com_vel_std", "speed_std")
_RATE_WANT = ("cov_du", "cov_ddu", "cov_vel", "cov_com", "cov_com_vel")


SAMPLE_FIELDS = ("seed", "ridge", "du", "q", "x", "positions", "com_pos")
# uncertainty_lengths=True: the covariance marginalised over the fitted segment lengths ("What is marginalised") -- the diagonal blocks
# and marker blocks of cov_u / positions_cov with the scale terms added and their standard deviations, scale_cov [G, G] = the covariance of the scales
# that was used, u_scale_response [N, 28, G] = du / ds of the re-adapted poses and positions_scale_response [N, L, 3, G] = d p / d s in total
LENGTH_FIELDS = ("cov_u_marginal", "u_std_marginal", "positions_cov_marginal", "positions_std_marginal", "scale_cov", "u_scale_response",
                 "positions_scale_response")


@dataclass(frozen=True)
class PosteriorRequest:
    """what the uncertainty keywords of ONE public call ask of the posterior (posterior_request makes it; None stands for uncertainty=False):
    the damping, whether the rates are propagated, uncertainty_spans as given, the number of draws and their seed, and whether the covariance is
    also marginalised over the fitted segment lengths.  Rates, spans and samples stay conditional on the lengths."""
    ridge: float = 0.0
    rates: bool = False
    spans: object = None
    samples: int = 0
    seed: int = 0
    lengths: bool = False

    @property
    def want_L(self) -> bool:
        """spans and samples read the covariance call's factor"""
        return self.spans is not None or self.samples > 0

    def spans_for(self, n_frames: int):
        return resolve_spans(self.spans, n_frames)


def posterior_request(uncertainty: bool, uncertainty_ridge: float, uncertainty_rates: bool, uncertainty_spans, uncertainty_samples: int,
                      uncertainty_seed: int, uncertainty_lengths: bool = False, estimate_lengths: bool = False) -> Optional[PosteriorRequest]:
    """the public keywords -> the request, or None for uncertainty=False.  Samples, rates and spans propagate the covariance uncertainty=True
    computes: alone each is refused, as is a negative sample count, before anything is looked at.  uncertainty_lengths adds the scale terms to
    that covariance and needs the lengths fitted in the same call (estimate_lengths); rates, spans and samples stay conditional on the lengths."""
    if uncertainty_samples < 0:
        raise ValueError(f"uncertainty_samples must be >= 0, not {uncertainty_samples}")
    if uncertainty_samples and not uncertainty:
        raise ValueError("uncertainty_samples needs uncertainty=True: the samples are drawn from the covariance that keyword computes")
    if uncertainty_rates and not uncertainty:
        raise ValueError("uncertainty_rates=True needs uncertainty=True: the rates are propagated from the covariance that keyword computes")
    if uncertainty_spans is not None and not uncertainty:
        raise ValueError("uncertainty_spans needs uncertainty=True: the spans are propagated from the covariance that keyword computes")
    if uncertainty_lengths and not uncertainty:
        raise ValueError("uncertainty_lengths=True needs uncertainty=True: the scale terms are added to the covariance that keyword computes")
    if uncertainty_lengths and not estimate_lengths:
        raise ValueError("uncertainty_lengths=True needs estimate_lengths=True: the covariance is marginalised over the lengths the same call fits")
    if not uncertainty:
        return None
    return PosteriorRequest(uncertainty_ridge, bool(uncertainty_rates), uncertainty_spans, int(uncertainty_samples), uncertainty_seed,
                            bool(uncertainty_lengths))


def _spans_of(req: Optional[PosteriorRequest], ests) -> Optional[list]:
    """the resolved spans of every estimator, or None where none are asked for (a bad pair raises here: before any solve)"""
    if req is None or req.spans is None:
        return None
    return [req.spans_for(e.params.end_frame - e.params.start_frame) for e in ests]


def sample_normals(seed: int, K: int, N: int) -> np.ndarray:
    """z [K, N, 28] of K samples of a sequence of N frames: a function of (seed, K, N) alone, so a sequence's samples do not depend on the call
    (single, batch, ragged batch) that draws them"""
    return np.random.default_rng(seed).standard_normal((K, N, abi.NX))


# estimate_kinetics / estimate_grf(uncertainty=True, uncertainty_samples=K): SAMPLE_FIELDS plus the node forces of every draw (cpe_force_samples)
# in the layouts of tau_std, lambda_std and grf_std -- tau [K, N, n_motors], lam [K, N, n_con], grf_net [K, N, n_feet, 3] (z, x, y) -- and the
# forces the draws are centred on, tau_mean, lam_mean, grf_net_mean: those of the covariance call's evaluation (cold start at the stored q,
# multipliers zero), not the solve's own
KINETIC_SAMPLE_FIELDS = SAMPLE_FIELDS + ("tau", "lam", "grf_net", "tau_mean", "lam_mean", "grf_net_mean")


def sample_force_normals(seed: int, K: int, N: int) -> np.ndarray:
    """zeta [K, N, 64] of K samples of the node forces of a sequence of N frames: a function of (seed, K, N) alone, as sample_normals, and a
    stream of its own (z stays sample_normals(seed, K, N): the du of a physics draw follows the kinematic rule)"""
    return np.random.default_rng([seed, 1]).standard_normal((K, N, 64))


def force_sample_fields(f_s: np.ndarray, f: np.ndarray, n_motors: int, n_con: int, n_feet: int) -> dict:
    """f_s [K, N, 64] and f [N, 64] of cpe_force_samples in the layout tau | lambda | (z, x, y) per foot -> the force fields of
    KINETIC_SAMPLE_FIELDS"""
    a, b = n_motors, n_motors + n_con
    cut = lambda v: (np.ascontiguousarray(v[..., :a]), np.ascontiguousarray(v[..., a:b]),
                     np.ascontiguousarray(v[..., b:b + 3 * n_feet].reshape(v.shape[:-1] + (n_feet, 3))))
    (tau, lam, grf), (tau_m, lam_m, grf_m) = cut(f_s), cut(f)
    return dict(tau=tau, lam=lam, grf_net=grf, tau_mean=tau_m, lam_mean=lam_m, grf_net_mean=grf_m)


@dataclass
class _Group:
    """how the library is called for the sequences of one group, after q: `args` = the covariance call's own arguments (meas, weight; physics:
    meas, weight, stance, kinetic options).  of = None: the plain form (one model, arrays stacked to [B, N, ...], the *_host methods); of = the
    model of every sequence on a Handle.multi: the ragged form (lists of per-sequence arrays, the *_ragged_host methods).  force = None: a
    kinematic group; else the physics variant arrays (grf_fixed / tau_box / grf_box, at most one) that the covariance call and the force-sample
    call share.  lengths = None, or what the length step of a kinematic group needs (_length_group): d_attach [M, G, n_links, 3] and d_marker_off
    [M, G, n_markers, 3] = the derivative tables of every model of the handle, animal = what names the animal of every sequence (sequences of one
    animal share their scales), prior_sigma = the calibration's prior of every sequence (None: none)."""
    args: tuple
    of: Optional[list] = None
    force: Optional[dict] = None
    lengths: Optional[dict] = None


def _gather(arrays, ragged: bool):
    """the per-sequence arrays of a group in its form: a list (ragged) or stacked (plain); None where the group has none"""
    return None if arrays[0] is None else (list(arrays) if ragged else np.stack(arrays))


def scale_covariance(A_red, prior_sigma: Optional[float]) -> np.ndarray:
    """cov_s = (sum A_red + P)^-1 over the reduced matrices of one animal's sequences, summed in list order; P = I / prior_sigma^2 (None: 0)"""
    S = np.array(A_red[0], dtype=np.float64)
    for A in A_red[1:]:
        S = S + A
    if prior_sigma is not None:
        S = S + np.eye(S.shape[0]) / float(prior_sigma) ** 2
    return np.linalg.inv(S)


def _length_group(seqs, of) -> dict:
    """_Group.lengths of the estimators `seqs` of one group (of: the model of every sequence, or None = one model): raises ValueError for an
    estimator without fitted lengths"""
    if any(getattr(e, "length_scale", None) is None or not e.length_calibration for e in seqs):
        raise ValueError("uncertainty_lengths=True: an estimator of the group has no fitted lengths (calibrate_lengths did not run on it)")
    reps = [0] if of is None else [of.index(k) for k in range(max(of) + 1)]
    tabs = [skeleton.length_derivatives(f"{e.name}-02" if e.params.kinetic_dataset else e.name, e.skeleton.n_markers, e.length_groups)
            for e in (seqs[i] for i in reps)]
    return dict(d_attach=np.stack([t[0] for t in tabs]), d_marker_off=np.stack([t[1] for t in tabs]),
                animal=[(e.name, e.params.kinetic_dataset) for e in seqs], prior_sigma=[e.length_calibration["prior_sigma"] for e in seqs])


def _posterior(h, req: PosteriorRequest, spans: Optional[list], q, group: _Group) -> dict:
    """THE posterior chain of every estimate, on the handle h that solved the group, at its stored q:
      1. ONE covariance call (cpe_covariance / cpe_covariance_kinetic, plain or ragged) with the factor where spans or samples read it;
      2. req.rates or spans: ONE cpe_rate_covariance call with that call's cov_diag and cov_off -> "rates", and the point Jacobians of the spans;
      3. spans (the resolved spans of every sequence): ONE cpe_covariance_columns call above the distinct last frames of every sequence's spans
         -- no anchor for a sequence without a factor -> "spans";
      4. req.samples = K > 0: ONE cpe_band_sample call on the covariance call's own factor (no second factorisation; a sequence without a factor
         takes no part: frame count 0) with z = sample_normals(seed, K, n) per sequence at its own length, ONE cpe_posterior_samples call at the
         same q and, for a physics group, ONE cpe_force_samples call with the covariance call's own arguments and
         zeta = sample_force_normals(seed, K, n) -> "samples";
      5. req.lengths (kinematic groups only; group.lengths), after the covariance call and at the same ridge: ONE cpe_scale_response call over
         the group, cov_s = scale_covariance of the A_red of every animal's sequences that have a factor (in list order, with the calibration's
         prior), ONE cpe_covariance_add_scales call on the covariance call's own band -> "lengths".  Steps 2 - 4 read the covariance GIVEN the
         lengths, whatever req.lengths.
    Returns the covariance call's dict with those additions; _uncertainty_of / _kinetic_uncertainty_of / _samples_of cut a sequence out of it."""
    ragged = group.of is not None
    models = (group.of,) if ragged else ()
    form = "_ragged_host" if ragged else "_host"
    a, force = (q,) + tuple(group.args), group.force or {}
    cov = getattr(h, ("covariance" if group.force is None else "covariance_kinetic") + form)(*a, *models, req.ridge, want_L=req.want_L, **force)
    src = cov["padded"] if ragged else cov
    B, Nm = src["cov_diag"].shape[:2]
    lens = [len(c) for c in cov["cov_diag"]] if ragged else [Nm] * B
    factor = [s == abi.OK for s in cov["seq_status"]]
    if req.lengths and group.force is None:
        lg = group.lengths
        rs = h.scale_response_host(*a, lg["d_attach"], lg["d_marker_off"], req.ridge, **(dict(model_list=group.of) if ragged else {}))
        rp = rs["padded"] if ragged else rs
        cov_s = np.zeros((B,) + rs["A_red"].shape[1:])
        for key in dict.fromkeys(lg["animal"]):
            idx = [b for b in range(B) if lg["animal"][b] == key]
            have = [rs["A_red"][b] for b in idx if rs["seq_status"][b] == abi.OK]
            if have:
                cov_s[idx] = scale_covariance(have, lg["prior_sigma"][idx[0]])
        m = h.covariance_add_scales_host(cov_s, rp["resp_u"], rp["resp_pos"], src["cov_diag"], src["cov_off"], src["cov_pos"], lens if ragged else None)
        cov["lengths"] = dict(cov_diag=m["cov_diag"], cov_pos=m["cov_pos"], cov_s=cov_s, resp_u=rp["resp_u"], resp_pos=rp["resp_pos"], lens=lens,
                              seq_status=rs["seq_status"])
    want = (_RATE_WANT if req.rates else ()) + (("jac_pos", "jac_com") if spans is not None else ())
    if want:
        r = getattr(h, "rate_covariance" + form)(q, cov["cov_diag"], cov["cov_off"], *models, want=want)
        if req.rates:
            cov["rates"] = r
    if spans is not None:
        lasts = [sorted({b for _, b in sp}) if factor[k] else [] for k, sp in enumerate(spans)]
        anchors = np.full((len(spans), max(1, max(len(l) for l in lasts))), -1, dtype=np.int32)
        for k, l in enumerate(lasts):
            anchors[k, :len(l)] = l
        cols = h.covariance_columns_host(src["L"], src["cov_diag"], src["cov_off"], anchors, lens if ragged else None)
        cov["spans"] = dict(columns=cols, anchors=anchors, spans=spans, jac_pos=r["jac_pos"], jac_com=r["jac_com"])
    K = req.samples
    if K > 0:
        z = np.zeros((B, K, Nm, abi.NX))
        for b, n in enumerate(lens):
            z[b, :, :n] = sample_normals(req.seed, K, n)
        du = h.band_sample_host(src["L"], z, [n if factor[b] else 0 for b, n in enumerate(lens)])
        cuts = lambda v: [np.ascontiguousarray(v[b, :, :n]) for b, n in enumerate(lens)]
        ps = h.posterior_samples_host(list(q), cuts(du), group.of) if ragged else h.posterior_samples_host(q, du)
        cov["samples"] = dict(du=du, lens=lens, q=ps["q"], positions=ps["positions"], seed=int(req.seed))
        if group.force is not None:
            zeta = np.zeros((B, K, Nm, 64))
            for b, n in enumerate(lens):
                zeta[b, :, :n] = sample_force_normals(req.seed, K, n)
            if ragged:
                fs = h.force_samples_ragged_host(*a, cuts(du), cuts(zeta), group.of, req.ridge, **force)["padded"]
            else:
                fs = h.force_samples_host(*a, du, zeta, req.ridge, **force)
            cov["samples"].update(f_s=fs["f_s"], f=fs["f"])
    return cov


def _samples_of(cov: Optional[dict], b: int, ridge: float) -> Optional[dict]:
    """the sample fields of sequence b that the library computed (du, q, positions; seed, ridge), or None: not asked for, or no factor"""
    if cov is None or "samples" not in cov or cov["seq_status"][b] != abi.OK:
        return None
    sm = cov["samples"]
    return dict(seed=np.int64(sm["seed"]), ridge=float(ridge), du=np.ascontiguousarray(sm["du"][b, :, :sm["lens"][b]]),
                q=np.ascontiguousarray(sm["q"][b]), positions=np.ascontiguousarray(sm["positions"][b]))


def _com_of(h, est, q: np.ndarray) -> np.ndarray:
    """the centre of mass [B, N, 3] at the poses q [B, N, nq] (cpe_forward_kinematics; h: a handle of the sequence's model)"""
    import torch
    dev = torch.device("cuda", est.device)
    pos = torch.empty(q.shape[:2] + (est.skeleton.n_markers, 3), dtype=torch.float64, device=dev)
    com = torch.empty(q.shape[:2] + (3,), dtype=torch.float64, device=dev)
    h.forward_kinematics(torch.tensor(q, device=dev), pos, com); h.synchronize()
    return com.cpu().numpy()


def _store_com(est, h, q: np.ndarray) -> None:
    """est.com_pos and est.com_vel of the ONE sequence q [1, N, nq] (acinoset_misc.py:742)"""
    est.com_pos = _com_of(h, est, q)[0]
    est.com_vel = (est.com_pos[1:] - est.com_pos[:-1]) * est.scene.fps


def _complete_samples(est, h, samples: Optional[dict]) -> Optional[dict]:
    """the sample fields of this sequence with those computed from q (h: a handle of its model): x and com_pos; None stays None"""
    if samples is None or "x" in samples:
        return samples
    return dict(samples, x=est.relative_angles(samples["q"]), com_pos=_com_of(h, est, samples["q"]))


def _store_samples(est, h, samples: Optional[dict], out_dir: str, fields=SAMPLE_FIELDS) -> None:
    """est.samples = `fields` of this sequence (h: a handle of its model, or None for samples _complete_samples has seen) and samples.npz beside
    uncertainty.npz; None: no samples, no file"""
    est.samples = None
    if samples is None:
        return
    est.samples = _complete_samples(est, h, samples)
    assert set(est.samples) == set(fields)
    np.savez(os.path.join(out_dir, "samples.npz"), **est.samples)


def resolve_spans(uncertainty_spans, n_frames: int) -> Optional[List[Tuple[int, int]]]:
    """the (first, last) frame pairs of a sequence of n_frames frames that uncertainty_spans asks for: None -> None; True -> the whole sequence,
    (0, n_frames - 1), and no span at all for a one-frame sequence; else pairs relative to the sequence's first frame, negative values counting
    from its end, each with 0 <= first < last <= n_frames - 1 (ValueError otherwise)"""
    if uncertainty_spans is None:
        return None
    if uncertainty_spans is True:
        return [(0, n_frames - 1)] if n_frames >= 2 else []
    out = []
    for pair in uncertainty_spans:
        try:
            first, last = (int(v) for v in pair)
        except (TypeError, ValueError):
            raise ValueError(f"uncertainty_spans: {pair!r} is not a (first, last) pair of frames") from None
        a, b = (first + n_frames if first < 0 else first), (last + n_frames if last < 0 else last)
        if not 0 <= a < b <= n_frames - 1:
            raise ValueError(f"uncertainty_spans: ({first}, {last}) does not satisfy 0 <= first < last <= {n_frames - 1} in a sequence of {n_frames} frames")
        out.append((a, b))
    return out


def span_uncertainty(columns: np.ndarray, anchors, cov_diag: np.ndarray, jac_com: np.ndarray, jac_pos: np.ndarray, com_pos: np.ndarray, spans,
                     h: float) -> dict:
    """SPAN_FIELDS of one sequence: the displacement between two distant frames with its first-order covariance ("What is spanned").
    columns [K, N, 28, 28] with columns[k][n] = Sigma(n, anchors[k]) for n <= anchors[k] (cpe_covariance_columns; every span's last frame is among
    the anchors), cov_diag [N, 28, 28] = Sigma(n, n), jac_com [N, 3, 28] and jac_pos [N, L, 3, 28] (cpe_rate_covariance), com_pos [N, 3], spans =
    resolved (first, last) pairs, h = the time step in seconds.  For a span (a, b) and a point with Jacobians P_a, P_b:
        cov(p_b - p_a) = P_b S_bb P_b^T + P_a S_aa P_a^T - P_b S(b,a) P_a^T - (that)^T
    Pure numpy; S = 0 spans give arrays of leading size 0."""
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    S, L = spans.shape[0], jac_pos.shape[1]
    slot = {int(a): k for k, a in enumerate(np.asarray(anchors).ravel()) if a >= 0}
    T = lambda M: np.swapaxes(M, -1, -2)
    std = lambda c: np.sqrt(np.maximum(np.diagonal(c, axis1=-2, axis2=-1), 0.0))

    def displacement_cov(P, a, b):                           # P [N, ..., 3, 28]
        Pa, Pb = P[a], P[b]
        X = Pb @ T(columns[slot[b]][a]) @ T(Pa)              # P_b S(b,a) P_a^T, S(b,a) = S(a,b)^T
        C = Pb @ cov_diag[b] @ T(Pb) + Pa @ cov_diag[a] @ T(Pa) - X - T(X)
        return 0.5 * (C + T(C))

    seconds = (spans[:, 1] - spans[:, 0]) * float(h)
    disp = com_pos[spans[:, 1]] - com_pos[spans[:, 0]]
    dcov, pcov = np.zeros((S, 3, 3)), np.zeros((S, L, 3, 3))
    for s, (a, b) in enumerate(spans):
        dcov[s], pcov[s] = displacement_cov(jac_com, a, b), displacement_cov(jac_pos, a, b)
    vel, vcov = disp / seconds[:, None], dcov / (seconds ** 2)[:, None, None]
    dist = np.sqrt(np.einsum("si,si->s", disp, disp))
    return dict(span_frames=spans, span_seconds=seconds, span_com_displacement=disp, span_com_displacement_cov=dcov, span_com_displacement_std=std(dcov),
                span_distance=dist, span_distance_std=speed_std_of(disp, dcov), span_mean_velocity=vel, span_mean_velocity_cov=vcov,
                span_mean_velocity_std=std(vcov), span_mean_speed=dist / seconds, span_mean_speed_std=speed_std_of(vel, vcov),
                span_positions_displacement_cov=pcov, span_positions_displacement_std=std(pcov))


def _rate_fields(rates: dict, b: int) -> dict:
    """the rate fields of est.uncertainty of sequence b, all but speed_std (which needs the centre-of-mass velocity: speed_std_of).  com_vel_cov
    row k is the library's row k + 1: the velocity between the frames k and k + 1, as com_vel[k]."""
    std = lambda c, a, b_: np.sqrt(np.diagonal(c, axis1=a, axis2=b_))
    du, ddu, vel = (np.ascontiguousarray(rates[k][b]) for k in ("cov_du", "cov_ddu", "cov_vel"))
    com, cv = np.ascontiguousarray(rates["cov_com"][b]), np.ascontiguousarray(rates["cov_com_vel"][b][1:])
    return dict(du_std=std(du, 1, 2), ddu_std=std(ddu, 1, 2), velocities_cov=vel, velocities_std=std(vel, 2, 3), com_cov=com, com_std=std(com, 1, 2),
                com_vel_cov=cv, com_vel_std=std(cv, 1, 2))


def speed_std_of(com_vel: np.ndarray, com_vel_cov: np.ndarray) -> np.ndarray:
    """standard deviation of the speed |com_vel| by the delta method: sqrt(v^T C v) / |v|, and 0 where |v| = 0"""
    v = np.asarray(com_vel, dtype=np.float64)
    var = np.einsum("ni,nij,nj->n", v, com_vel_cov, v)
    norm = np.sqrt(np.einsum("ni,ni->n", v, v))
    out = np.zeros(v.shape[0])
    nz = norm > 0
    out[nz] = np.sqrt(np.maximum(var[nz], 0.0)) / norm[nz]
    return out


def _add_speed_std(est) -> None:
    """est.uncertainty["speed_std"] once est.com_vel is known (uncertainty_rates=True; nothing otherwise), and SPAN_FIELDS once est.com_pos is
    (uncertainty_spans: from what _uncertainty_of left under "_spans", which goes)"""
    if est.uncertainty is not None and "com_vel_cov" in est.uncertainty:
        est.uncertainty["speed_std"] = speed_std_of(est.com_vel, est.uncertainty["com_vel_cov"])
    sp = None if est.uncertainty is None else est.uncertainty.pop("_spans", None)
    if sp is not None:
        est.uncertainty.update(span_uncertainty(sp["columns"], sp["anchors"], est.uncertainty["cov_u"], sp["jac_com"], sp["jac_pos"], est.com_pos,
                                                sp["spans"], 1.0 / est.scene.fps))


def _uncertainty_of(cov: dict, b: int, ridge: float) -> Optional[dict]:
    """est.uncertainty of sequence b from a covariance_host / covariance_ragged_host result (None where the matrix has no Cholesky factor); with
    the rate fields where _posterior added the rate covariances"""
    if cov["seq_status"][b] != abi.OK:
        return None
    cu, cp = np.ascontiguousarray(cov["cov_diag"][b]), np.ascontiguousarray(cov["cov_pos"][b])
    unc = dict(cov_u=cu, u_std=np.sqrt(np.diagonal(cu, axis1=1, axis2=2)), positions_cov=cp, positions_std=np.sqrt(np.diagonal(cp, axis1=2, axis2=3)),
               ridge=float(ridge))
    if "rates" in cov:
        unc.update(_rate_fields(cov["rates"], b))
    if "lengths" in cov:                            # LENGTH_FIELDS
        lg = cov["lengths"]
        n = lg["lens"][b]
        cm, pm = np.ascontiguousarray(lg["cov_diag"][b, :n]), np.ascontiguousarray(lg["cov_pos"][b, :n])
        unc.update(cov_u_marginal=cm, u_std_marginal=np.sqrt(np.diagonal(cm, axis1=1, axis2=2)), positions_cov_marginal=pm,
                   positions_std_marginal=np.sqrt(np.diagonal(pm, axis1=2, axis2=3)), scale_cov=lg["cov_s"][b].copy(),
                   u_scale_response=np.ascontiguousarray(lg["resp_u"][b, :n]), positions_scale_response=np.ascontiguousarray(lg["resp_pos"][b, :n]))
    if "spans" in cov:                              # (SPAN_FIELDS need the centre of mass: _add_speed_std)
        sp = cov["spans"]
        unc["_spans"] = dict(columns=sp["columns"][b], anchors=sp["anchors"][b], spans=sp["spans"][b], jac_pos=np.ascontiguousarray(sp["jac_pos"][b]),
                             jac_com=np.ascontiguousarray(sp["jac_com"][b]))
    return unc


def _check_uncertainty(est: CheetahEstimator, pri: Optional[abi.Priors], ridge: float) -> None:
    """uncertainty=True: what is refused before anything is solved"""
    if est.params.enable_shutter_delay_estimation and est.scene.cam_idx is None:
        raise NotImplementedError("uncertainty together with shutter-delay estimation: the covariance is that of the kinematic objective without the "
                                  "shutter displacement (cpe_covariance); the delays would be treated as known")
    _lib.covariance_supported(pri, ridge)          # raises with the library's reason: negative ridge, motion-prior window above 4


def force_uncertainty(cov_f: np.ndarray, meta: np.ndarray, n_motors: int, n_con: int, n_feet: int) -> dict:
    """cov_f [N, 64, 64] and meta [N, 65] of cpe_covariance_kinetic -> standard deviations in the layout of the node forces f = tau | lambda |
    (z, x, y) per foot: tau_std [N, n_motors], lambda_std [N, n_con], grf_std [N, n_feet, 3], and tau_cov [N, n_motors, n_motors].  meta[n] = (count,
    the indices into f of the node's free forces, in cov_f's order); an entry is 0.0 where a force is not an unknown of the node."""
    N, nlat = cov_f.shape[0], n_motors + n_con + 3 * n_feet
    std = np.zeros((N, nlat))
    tau_cov = np.zeros((N, n_motors, n_motors))
    for n in range(N):
        na = int(meta[n, 0])
        idx = np.asarray(meta[n, 1:1 + na], dtype=np.int64)
        std[n, idx] = np.sqrt(np.diagonal(cov_f[n])[:na])
        t = np.nonzero(idx < n_motors)[0]
        tau_cov[n][np.ix_(idx[t], idx[t])] = cov_f[n][np.ix_(t, t)]
    return dict(tau_std=np.ascontiguousarray(std[:, :n_motors]), lambda_std=np.ascontiguousarray(std[:, n_motors:n_motors + n_con]),
                grf_std=np.ascontiguousarray(std[:, n_motors + n_con:].reshape(N, n_feet, 3)), tau_cov=tau_cov)


@dataclass
class KineticUncertainty:
    """what estimate_kinetics / estimate_grf(uncertainty=True) computed after the solver call: the fields of est.uncertainty, or why there are none
    (both None: the solve did not converge, nothing was asked of the library)"""
    fields: Optional[dict] = None
    reason: Optional[str] = None
    samples: Optional[dict] = None          # uncertainty_samples: KINETIC_SAMPLE_FIELDS of the sequence but x and com_pos (_complete_samples)


def _no_factor_reason(ridge: float, names: Optional[Sequence[str]] = None) -> str:
    """why a physics-based estimate has no uncertainty (names: the estimators of a batch it holds for)"""
    who = "" if names is None else f" (no uncertainty for: {', '.join(names)})"
    return (f"uncertainty: the evaluation at the solution is not finite, or the reduced band or a node's force matrix has no "
            f"Cholesky factor at ridge {ridge:g} (the data leave a coordinate or a force undetermined; a positive "
            f"uncertainty_ridge regularises it){who}")


def _kinetic_uncertainty_of(cov: dict, b: int, ridge: float, res: dict) -> KineticUncertainty:
    """sequence b of a covariance_kinetic_host / covariance_kinetic_ragged_host result; res: the solve's result of that ONE sequence"""
    if cov["seq_status"][b] != abi.OK:
        return KineticUncertainty(reason=_no_factor_reason(ridge))
    unc = _uncertainty_of(cov, b, ridge)
    counts = res["tau"].shape[-1], res["lam"].shape[-1], res["grf"].shape[-2]
    unc.update(force_uncertainty(cov["cov_f"][b], cov["meta"][b], *counts))
    sm = _samples_of(cov, b, ridge)
    if sm is not None:
        n = cov["samples"]["lens"][b]
        sm.update(force_sample_fields(cov["samples"]["f_s"][b, :, :n], cov["samples"]["f"][b, :n], *counts))
    return KineticUncertainty(fields=unc, samples=sm)


def _kinetic_options_of(preps, of):
    """the kinetic options of a group in its form: those of its one model (plain), or of the first sequence of every model (ragged)"""
    return preps[0]["ko"] if of is None else [preps[of.index(k)]["ko"] for k in range(max(of) + 1)]


def _batch_kinetic_uncertainty(h, req: Optional[PosteriorRequest], spans: Optional[list], res: dict, preps, meas, weight,
                               of=None) -> Dict[int, KineticUncertainty]:
    """uncertainty of every sequence of a solved physics group, keyed by its place b in the group (empty: not asked for): ONE posterior chain
    (_posterior) over the places whose solve converged, with the solve's own stance, options and variant arrays; the others get
    KineticUncertainty(): nothing is asked of the library for them.  preps: per sequence a dict with stance, ko and at most one of grf_fixed /
    tau_box / grf_box (a _kinetic_prepare dict); meas, weight, spans (or None): per sequence; of: as in _kinetic_solve."""
    if req is None:
        return {}
    unc = {b: KineticUncertainty() for b in range(len(preps))}
    conv = [b for b in unc if res["stats"][b].status == abi.OK]
    if conv:
        pick = lambda v: _gather([v[b] for b in conv], of is not None)
        force = {k: pick([p[k] for p in preps]) for k in ("grf_fixed", "tau_box", "grf_box") if preps[0].get(k) is not None}
        group = _Group((pick(meas), pick(weight), pick([p["stance"] for p in preps]), _kinetic_options_of(preps, of)),
                       None if of is None else [of[b] for b in conv], force)
        cov = _posterior(h, req, None if spans is None else [spans[b] for b in conv], pick(res["q"]), group)
        for k, b in enumerate(conv):
            unc[b] = _kinetic_uncertainty_of(cov, k, req.ridge, _sequence_of(res, b))
    return unc


def _kinetic_uncertainty(h, ko: abi.KineticOptions, res: dict, meas: np.ndarray, weight: np.ndarray, stance: np.ndarray, req: PosteriorRequest,
                         spans=None, **force) -> KineticUncertainty:
    """the group of one, from arrays: the posterior at the solution res["q"] of ONE physics-based solve with its stance, options and variant
    array (force: grf_fixed, tau_box or grf_box of that sequence); spans: its resolved spans"""
    return _batch_kinetic_uncertainty(h, req, None if spans is None else [spans], res, [dict(stance=stance, ko=ko, **force)], [meas], [weight])[0]


def _store_kinetic_uncertainty(est: CheetahEstimator, unc: Optional[KineticUncertainty], ok: bool, out_dir: Optional[str],
                               no_factor: Optional[list] = None, h=None) -> None:
    """after the solve's own files (unc None: not asked for, nothing changes): est.uncertainty and, for a solve that is `ok`, uncertainty.npz beside
    fte.pickle -- or the library's reason raised (no_factor, a list: the estimator is appended to it instead, for the batch to raise once at its end).
    unc.samples (uncertainty_samples): est.samples and samples.npz beside it; h: a handle of the sequence's model, or None where _complete_samples
    has seen them."""
    if unc is None:
        return
    est.uncertainty = None
    est.samples = None
    if not ok:
        return
    if unc.reason is not None:
        if no_factor is None:
            raise _lib.CpeError(unc.reason)
        no_factor.append(est)
        return
    if unc.fields is not None:
        est.uncertainty = unc.fields
        _add_speed_std(est)
        np.savez(os.path.join(out_dir, "uncertainty.npz"), **est.uncertainty)
        _store_samples(est, h, unc.samples, out_dir, KINETIC_SAMPLE_FIELDS)


def _kin_finish(est: CheetahEstimator, h, res: dict, seconds: float, solver_output: bool, monocular_constraints: bool,
                out_dir_prefix: Optional[str], uncertainty: Optional[Tuple[Optional[dict], float]] = None, samples: Optional[dict] = None) -> bool:
    """what estimate_kinematics does after the solver call (acinoset_opt.py:619-634): centre of mass, costs, files.  `res` holds ONE sequence.
    uncertainty: None (not asked for), or (est.uncertainty of this sequence or None, ridge): stored, and written as uncertainty.npz beside fte.pickle.
    samples: what _samples_of returned for this sequence (uncertainty_samples; None: none): completed, stored and written as samples.npz."""
    est.samples = None
    params, scene = est.params, est.scene
    est.opt_time_s = seconds
    _store_com(est, h, res["q"])
    st = res["stats"][0]
    est.result = res
    est.costs = {"measurement": st.cost_meas, "model": st.cost_model, "pose": st.cost_pose, "motion": st.cost_motion}
    if solver_output:
        print(f"Total cost: {st.cost}\n-- measurement: {st.cost_meas}\n-- model: {st.cost_model}\n-- pose: {st.cost_pose}\n-- motion: {st.cost_motion}\n"
              f"status {st.status}, {st.iterations} LM iterations, {est.opt_time_s:.3f} s")
        if est.shutter_delay is not None:
            print("Shutter delay estimation:", [float(v) for v in est.shutter_delay])           # acinoset_opt.py:397-398
    ok = st.status == abi.OK
    if ok:
        fname = f"fte_kinematic{'_gt' if params.hand_labeled_data else ''}"
        fname = fname if scene.cam_idx is None or monocular_constraints else "fte_kinematic_orig"
        fname = fname if scene.cam_idx is None else f"{fname}_{scene.cam_idx}"    # acinoset_opt.py:626-628
        out_dir = est.save(fname, out_dir_prefix=out_dir_prefix)
        if est.length_scale is not None:
            write_skeleton_scale(est, out_dir)
        if uncertainty is not None:
            est.uncertainty = uncertainty[0]
            if est.uncertainty is None:
                print(f"uncertainty: none for {est.name}: the Gauss-Newton matrix has no Cholesky factor at ridge {uncertainty[1]:g} "
                      "(the data leave a coordinate undetermined; a positive uncertainty_ridge regularises it)")
            else:
                _add_speed_std(est)
                np.savez(os.path.join(out_dir, "uncertainty.npz"), **est.uncertainty)
                _store_samples(est, h, samples, out_dir)
    elif uncertainty is not None:
        est.uncertainty = None
    return ok


def _length_kw(est) -> dict:
    """the length_scale / groups keywords of skeleton.load_params, grf_options, eom_options, dyn_options for an estimator: empty (today's tables)
    unless its lengths were calibrated"""
    ls = getattr(est, "length_scale", None)
    return {} if ls is None else dict(length_scale=ls, groups=est.length_groups)


LENGTH_STEP_CAP = 0.05          # largest change of a scale in one round
LENGTH_HALVINGS = 8             # how often a step is halved while the total objective rises


def calibrate_loop(solve, system, n_groups: int, prior_sigma: Optional[float] = 0.1, s0=None, tol: float = 1e-6, max_rounds: int = 30,
                   log=None) -> dict:
    """The length calibration over two callables ("What is calibrated"), the same loop for the GPU and for a CPU reference:
        solve(s, state)  -> (J, state')   the pose solves at scales s, warm-started from `state` (None: cold); J = the objective they reached,
                                          summed over the sequences (solver cost / cost_scale)
        system(s, state) -> (A_red, b_red) summed over the sequences: the Gauss-Newton system of the scales with the poses eliminated, at state
    Minimises T(s) = J(s, q*(s)) + |s - 1|^2 / (2 sigma^2) (prior_sigma None: no prior) by reduced Gauss-Newton steps
    ds = -(A_red + P)^-1 (b_red + P (s - 1)), P = I / sigma^2, each capped at LENGTH_STEP_CAP per scale and halved while T rises; stops when
    max |ds| < tol.  Returns dict(s, cov = (A_red + P)^-1 at the last system, objective = T, rounds, converged, state, history = [(T, max |ds|)])."""
    G = int(n_groups)
    s = np.ones(G) if s0 is None else np.array(s0, dtype=np.float64)
    if s.shape != (G,):
        raise ValueError(f"calibrate_loop: one initial scale per group ({G})")
    P = np.zeros((G, G)) if prior_sigma is None else np.eye(G) / float(prior_sigma) ** 2
    total = lambda J, sv: float(J) + 0.5 * float((sv - 1.0) @ P @ (sv - 1.0))
    J, state = solve(s, None)
    T = total(J, s)
    history, converged, rounds, cov = [], False, 0, None
    for rounds in range(1, max_rounds + 1):
        A_red, b_red = system(s, state)
        Hs = np.asarray(A_red, dtype=np.float64) + P
        cov = np.linalg.inv(Hs)
        ds = -np.linalg.solve(Hs, np.asarray(b_red, dtype=np.float64) + P @ (s - 1.0))
        big = np.abs(ds).max()
        if big > LENGTH_STEP_CAP:
            ds *= LENGTH_STEP_CAP / big
        history.append((T, float(np.abs(ds).max())))
        if log:
            log(f"length calibration round {rounds}: objective {T:.9g}, max |ds| {np.abs(ds).max():.3e}")
        if np.abs(ds).max() < tol:
            converged = True
            break
        for _ in range(LENGTH_HALVINGS + 1):
            J_try, state_try = solve(s + ds, state)
            T_try = total(J_try, s + ds)
            if T_try <= T:
                break
            ds = 0.5 * ds
        else:                                                # no step along ds lowers the objective: s is as good as this model gets
            converged = np.abs(ds).max() < tol
            break
        s, state, T = s + ds, state_try, T_try
    return dict(s=s, cov=cov, objective=T, rounds=rounds, converged=converged, state=state, history=history)


def calibrate_lengths(estimators: Sequence[CheetahEstimator], groups=skeleton.LENGTH_GROUPS, prior_sigma: Optional[float] = 0.1,
                      length_scale_init=None, tol: float = 1e-6, max_rounds: int = 30, monocular_constraints: bool = False,
                      disable_pose_prior: bool = False, disable_motion_prior: bool = False, options: Optional[abi.Options] = None,
                      ridge: float = 0.0, q_init: Optional[Sequence[np.ndarray]] = None, solver_output: bool = False,
                      pose_model_num_components: int = 5, motion_model_window_size: int = 4, motion_model_sparse_solution: bool = True) -> dict:
    """Fit the segment lengths of ONE animal to the data of its sequences: one scale per group of `groups` (skeleton.LENGTH_GROUPS' form), shared by
    all estimators (they must name the same animal and dataset kind).  calibrate_loop with, per round, one ragged batch pose solve on the
    skeleton build_skeleton(length_scale=s) -- warm-started from the previous round's poses -- and one cpe_scale_system call (damping `ridge`);
    A_red and b_red are summed in list order.  prior_sigma: standard deviation of the Gaussian prior s ~ N(1, sigma^2) on every scale, a
    modelling default for the individual variation of limb lengths (None: no prior -- refused for one camera, where scale and depth cannot be
    told apart, unless a sequence of the animal has more cameras).  q_init: the first round's initial poses per estimator (None: the
    reference's initial guess).  pose_model_num_components, motion_model_window_size, motion_model_sparse_solution: the priors of a monocular
    run, as estimate_kinematics takes them.
    Sets est.length_scale, est.length_scale_cov, est.length_groups, est.length_calibration (converged, rounds, prior_sigma, ridge, objective) and
    replaces est.skeleton on every estimator; returns calibrate_loop's dict with `q` = the last poses per estimator.  A loop that did not
    converge (max_rounds reached, or no descent step) leaves its last iterate all the same, says so in length_calibration and warns."""
    ests = list(estimators)
    if not ests:
        raise ValueError("calibrate_lengths: no estimator")
    _check_lengths(ests, prior_sigma)
    e0 = ests[0]
    if any(e.name != e0.name or e.params.kinetic_dataset != e0.params.kinetic_dataset or e.device != e0.device for e in ests):
        raise ValueError("calibrate_lengths: the estimators of one call share the animal, the dataset kind and the device")
    if prior_sigma is not None and not prior_sigma > 0:
        raise ValueError("calibrate_lengths: prior_sigma must be positive")
    groups = tuple((str(n), tuple(l)) for n, l in groups)
    G = len(groups)
    if not 1 <= G <= abi.MAX_SCALES:
        raise ValueError(f"calibrate_lengths: 1..{abi.MAX_SCALES} groups")
    model_name = f"{e0.name}-02" if e0.params.kinetic_dataset else e0.name
    n_markers = e0.skeleton.n_markers
    d_attach, d_marker_off = skeleton.length_derivatives(model_name, n_markers, groups)
    prep = [_kin_prepare(e, monocular_constraints, disable_pose_prior, disable_motion_prior, pose_model_num_components, motion_model_window_size,
                         motion_model_sparse_solution, None if q_init is None else q_init[i],
                         None if options is None else _struct_copy(options)) for i, e in enumerate(ests)]
    pri = prep[0][2]
    if len({ragged_group_key(e.skeleton, p[1], p[2], e.device) for e, p in zip(ests, prep)}) != 1:
        raise ValueError("calibrate_lengths: the sequences of one call go through one ragged batch: same priors and batch-level solver options")
    cost_scale = prep[0][1].cost_scale
    # one model per distinct (rig, options); the skeleton of every model is this round's
    of, reps = _models_of(b"".join(_struct_bytes(e.cams[c]) for c in range(len(e.cams))) + _struct_bytes(p[1]) for e, p in zip(ests, prep))
    meas, weight = [e.meas for e in ests], [e.weight for e in ests]
    tabs = (np.broadcast_to(d_attach, (len(reps),) + d_attach.shape), np.broadcast_to(d_marker_off, (len(reps),) + d_marker_off.shape))
    build = lambda s: skeleton.build_skeleton(model_name, n_markers, e0.params.kinetic_dataset, length_scale=s, groups=groups)

    def handle(s):
        sk = build(s)
        return _lib.Handle.multi([sk] * len(reps), [ests[i].cams for i in reps], [prep[i][1] for i in reps], pri, device=e0.device)

    def solve(s, state):
        h = handle(s)
        try:
            res = h.solve_ragged_host([p[0] for p in prep] if state is None else state, meas, weight, of)
        finally:
            h.close()
        if any(st.status == abi.NUMERICAL for st in res["stats"]):
            raise _lib.CpeError("calibrate_lengths: a pose solve failed numerically")
        return sum(st.cost for st in res["stats"]) / cost_scale, res["q"]

    def system(s, state):
        h = handle(s)
        try:
            out = h.scale_system_host(state, meas, weight, tabs[0], tabs[1], ridge, model_list=of)
        finally:
            h.close()
        if out["status"] != abi.OK:
            raise _lib.CpeError(f"calibrate_lengths: the Gauss-Newton matrix of the poses has no Cholesky factor at ridge {ridge:g} "
                                "(the data leave a coordinate undetermined; a positive ridge regularises it)")
        return out["A_red"].sum(axis=0), out["b_red"].sum(axis=0)

    r = calibrate_loop(solve, system, G, prior_sigma, length_scale_init, tol, max_rounds, log=print if solver_output else None)
    sk = build(r["s"])
    if not r["converged"]:
        import warnings
        warnings.warn(f"calibrate_lengths ({e0.name}): not converged after {r['rounds']} rounds (last step {r['history'][-1][1]:.2e}, tolerance "
                      f"{tol:g}); the scales are the last iterate, up to {np.abs(r['s'] - 1.0).max():.3f} from 1", RuntimeWarning, stacklevel=2)
    how = dict(converged=bool(r["converged"]), rounds=int(r["rounds"]), prior_sigma=None if prior_sigma is None else float(prior_sigma),
               ridge=float(ridge), objective=float(r["objective"]))
    for e in ests:
        e.length_scale, e.length_scale_cov, e.length_groups, e.length_calibration = r["s"].copy(), r["cov"].copy(), groups, dict(how)
        e.skeleton = abi.Skeleton.from_buffer_copy(bytes(sk))
    r["q"] = r.pop("state")
    return r


def write_skeleton_scale(est: CheetahEstimator, out_dir: str) -> str:
    """skeleton_scale.json beside fte.pickle: the groups, their scales, the covariance of the scales and how the fit ended (converged, rounds,
    prior_sigma, ridge, objective)"""
    path = os.path.join(out_dir, "skeleton_scale.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(dict(animal=est.name, groups=[[n, list(l)] for n, l in est.length_groups], length_scale=[float(v) for v in est.length_scale],
                       length_scale_cov=[[float(v) for v in row] for row in est.length_scale_cov], **(est.length_calibration or {})), f, indent=1)
    return path


def _check_lengths(ests, prior_sigma) -> None:
    """what a length calibration over the estimators of ONE animal refuses (calibrate_lengths, and the fronts before anything else is looked at):
    shutter-delay estimation, and no prior when every sequence has one camera -- scale and depth cannot be separated there"""
    if any(e.params.enable_shutter_delay_estimation and e.scene.cam_idx is None for e in ests):
        raise NotImplementedError("length calibration together with shutter-delay estimation")
    if prior_sigma is None and all(e.scene.cam_idx is not None for e in ests):
        raise ValueError("length calibration with one camera needs a prior (length_prior_sigma): scale and depth cannot be separated")


def _animals(ests) -> Dict[tuple, List[int]]:
    """the estimators of every animal (name, dataset kind), which share their scales: {key: indices}"""
    out: Dict[tuple, List[int]] = {}
    for i, est in enumerate(ests):
        out.setdefault((est.name, est.params.kinetic_dataset), []).append(i)
    return out


def estimate_kinematics(estimator: CheetahEstimator, solver_output: bool = True, monocular_constraints: bool = False,
                        disable_pose_prior: bool = False, disable_motion_prior: bool = False,
                        pose_model_num_components: int = 5, motion_model_window_size: int = 4,
                        motion_model_sparse_solution: bool = True, out_dir_prefix: Optional[str] = None,
                        q_init: Optional[np.ndarray] = None, options: Optional[abi.Options] = None, uncertainty: bool = False,
                        uncertainty_ridge: float = 0.0, uncertainty_rates: bool = False, uncertainty_spans=None, uncertainty_samples: int = 0,
                        uncertainty_seed: int = 0, uncertainty_lengths: bool = False, estimate_lengths: bool = False, length_prior_sigma: Optional[float] = 0.1,
                        length_scale_init=None, length_ridge: float = 0.0) -> bool:
    """Same signature as acinoset_opt.estimate_kinematics (acinoset_opt.py:539-547) plus optional
    keyword arguments.  Returns True when the solve converged (IPOPT `ok`+`optimal` in the reference).
    uncertainty=True: after a converged solve the posterior covariance of the estimate (cpe_covariance at the stored q, damping
    uncertainty_ridge) goes to est.uncertainty and to uncertainty.npz beside fte.pickle; the return value stays that of the solve.
    uncertainty_rates=True (with uncertainty=True): also how well the rates are determined (cpe_rate_covariance on that covariance): du_std, ddu_std
    [N, 28], velocities_cov / _std [N, L, 3(, 3)], com_cov / _std [N, 3(, 3)], com_vel_cov / _std [N-1, 3(, 3)] and speed_std [N-1], both aligned
    with com_vel (RATE_FIELDS; DESIGN.md 2, "What is propagated").
    uncertainty_spans (with uncertainty=True): True = the whole sequence, or (first, last) frame pairs relative to the sequence's first frame,
    negative values counting from its end (resolve_spans).  For every span the displacement of the centre of mass, the distance, the mean velocity
    and the mean speed with their first-order covariances and standard deviations, and the covariance of every marker's displacement (SPAN_FIELDS,
    span_uncertainty; DESIGN.md 2, "What is spanned"), from the covariance between the two frames (cpe_covariance_columns).
    uncertainty_samples=K > 0 (with uncertainty=True): K whole trajectories drawn from that posterior ("What is sampled"), for the
    error bar of any quantity computed from a trajectory: du = L^-T z with z = sample_normals(uncertainty_seed, K, N) and the covariance call's own
    factor L (cpe_band_sample), then the poses (cpe_posterior_samples).  They go to est.samples and to samples.npz beside uncertainty.npz
    (SAMPLE_FIELDS: seed, ridge, du [K, N, 28], q [K, N, nq], x = relative_angles(q), positions [K, N, L, 3], com_pos [K, N, 3]); est.uncertainty
    and uncertainty.npz do not change.  Without a factor: est.samples = None and no file.
    estimate_lengths=True: the segment lengths are fitted first (calibrate_lengths: one scale per group of skeleton.LENGTH_GROUPS, prior
    s ~ N(1, length_prior_sigma^2), start length_scale_init or 1); the estimate is then made on the fitted skeleton, est.length_scale and
    est.length_scale_cov hold the scales and their covariance, est.length_calibration how the fit ended (converged, rounds, prior_sigma, ridge,
    objective), and skeleton_scale.json beside fte.pickle holds all of it.  A fit that did not converge warns and is marked there; its scales
    are still used.  length_ridge: the damping of the poses' matrix in cpe_scale_system (a monocular run may need 1e-6 for a factor).  The
    calibration's pose solves use this call's priors and options.  One camera needs a prior (length_prior_sigma=None: ValueError); together
    with shutter-delay estimation: NotImplementedError.  uncertainty=True stays the covariance of the poses GIVEN the lengths.
    uncertainty_lengths=True (with uncertainty=True and estimate_lengths=True; else ValueError): est.uncertainty and uncertainty.npz gain
    LENGTH_FIELDS, the covariance marginalised over the fitted lengths ("What is marginalised": cpe_scale_response and
    cpe_covariance_add_scales at uncertainty_ridge, cov_s from this sequence's A_red and the calibration's prior); every other field keeps its bits.
    The rates, spans and samples stay conditional on the lengths."""
    req = posterior_request(uncertainty, uncertainty_ridge, uncertainty_rates, uncertainty_spans, uncertainty_samples, uncertainty_seed,
                            uncertainty_lengths, estimate_lengths)
    if estimate_lengths:
        _check_lengths([estimator], length_prior_sigma)
    est, params, scene = estimator, estimator.params, estimator.scene
    if estimate_lengths:
        cal = calibrate_lengths([est], prior_sigma=length_prior_sigma, length_scale_init=length_scale_init, monocular_constraints=monocular_constraints,
                                disable_pose_prior=disable_pose_prior, disable_motion_prior=disable_motion_prior, options=options, ridge=length_ridge,
                                q_init=None if q_init is None else [q_init], solver_output=solver_output,
                                pose_model_num_components=pose_model_num_components, motion_model_window_size=motion_model_window_size,
                                motion_model_sparse_solution=motion_model_sparse_solution)
        q_init = cal["q"][0]
    spans = _spans_of(req, [est])
    q_init, opts, pri = _kin_prepare(est, monocular_constraints, disable_pose_prior, disable_motion_prior, pose_model_num_components,
                                     motion_model_window_size, motion_model_sparse_solution, q_init, options)
    if req is not None:
        _check_uncertainty(est, pri, req.ridge)
    finish = (solver_output, monocular_constraints, out_dir_prefix)
    if params.enable_shutter_delay_estimation and scene.cam_idx is None:            # (never with uncertainty: _check_uncertainty)
        h = _lib.Handle(est.skeleton, est.cams, opts, pri, device=est.device)
        try:
            t0 = time()
            # m.shutter_delay, bounds +-hm0, camera 1 fixed (acinoset_misc.py:182-183, 273-275)
            res = h.solve_shutter_host(q_init[None], est.meas[None], est.weight[None], opts.h, max_rounds=20, tol_tau=1e-5)
            est.shutter_delay = res["tau"][0]
            return _kin_finish(est, h, res, time() - t0, *finish)
        finally:
            h.close()
    out = [None]
    _solve_kinematic_group([est], [0], {0: (q_init, opts, pri)}, out, False, req, spans, finish, single=True)
    return out[0]


def _struct_bytes(x) -> bytes:
    """the bytes of a ctypes struct"""
    return bytes(x)


def _struct_copy(x):
    """a ctypes struct of the same type with the same bytes"""
    return type(x).from_buffer_copy(x)


def ragged_group_key(sk: abi.Skeleton, opts: abi.Options, pri: Optional[abi.Priors], device: int) -> tuple:
    """What sequences must share to go through one cpe_solve_ragged call (Handle.multi): the skeleton's shape, the solver options the LM driver
    reads per batch, the priors and the device.  Rig, length, frame rate and the skeleton's numbers may differ."""
    return (_lib.shape_signature(sk), _lib.shared_options_signature(opts), None if pri is None else _struct_bytes(pri), device)


def estimate_kinematics_batch(estimators: Sequence[CheetahEstimator], solver_output: bool = False, monocular_constraints: bool = False,
                              disable_pose_prior: bool = False, disable_motion_prior: bool = False, out_dir_prefix: Optional[str] = None,
                              options: Optional[abi.Options] = None, ragged: bool = False, uncertainty: bool = False,
                              uncertainty_ridge: float = 0.0, uncertainty_rates: bool = False, uncertainty_spans=None, uncertainty_samples: int = 0,
                              uncertainty_seed: int = 0, uncertainty_lengths: bool = False, estimate_lengths: bool = False, length_prior_sigma: Optional[float] = 0.1,
                              length_scale_init=None, length_ridge: float = 0.0) -> List[bool]:
    """estimate_kinematics for MANY sequences at once: the loop of run_dataset.py:1145-1196 (`for seq in dataset: init_trajectory; estimate_kinematics`)
    as batched launches.  Sequences that share a skeleton, a camera rig, a length and a frame rate go through ONE solver handle and ONE cpe_solve
    call (B = the group's size: the GPU solves thousands of sequences per second batched, one at a time it is latency-bound at 7 - 30 ms each);
    every sequence then gets its own centre of mass, costs and files exactly as estimate_kinematics writes them.  All estimators must live on the
    same device; shutter-delay estimation is per sequence (cpe_solve_shutter) and goes through estimate_kinematics.  Returns one bool per
    estimator, in order.
    ragged=True: sequences need only share the skeleton's shape, the batch-level solver options, the priors and the device (ragged_group_key);
    each group is ONE cpe_solve_ragged call over a Handle.multi of its distinct (skeleton, rig, options) models, whatever the lengths.  Every
    sequence's results are bit-equal to those of ragged=False.
    uncertainty=True: as in estimate_kinematics, one cpe_covariance (ragged: cpe_covariance_ragged) call per group on the group's handle; every
    sequence's est.uncertainty and uncertainty.npz are bit-equal to those of its own estimate_kinematics call.  uncertainty_rates=True: as in
    estimate_kinematics, one cpe_rate_covariance (ragged: cpe_rate_covariance_ragged) call after each covariance call, with the same bit-equality.
    uncertainty_spans: as in estimate_kinematics, resolved for every sequence; one cpe_covariance_columns call per group, same bit-equality.
    uncertainty_samples, uncertainty_seed: as in estimate_kinematics, every sequence with the z of its own call (sample_normals); one cpe_band_sample
    and one cpe_posterior_samples call per group, same bit-equality of est.samples and samples.npz.
    estimate_lengths, length_prior_sigma, length_scale_init, length_ridge: as in estimate_kinematics; the estimators of one animal (name and dataset kind) share
    their scales: one calibrate_lengths call per animal over all its sequences, before the solves.
    uncertainty_lengths: as in estimate_kinematics; per group one cpe_scale_response and one cpe_covariance_add_scales call, and cov_s of an animal
    from the A_red of its sequences IN THAT GROUP (a plain batch splits an animal's sequences by length and rig; ragged=True keeps them together).
    Rates, spans and samples stay conditional on the lengths."""
    req = posterior_request(uncertainty, uncertainty_ridge, uncertainty_rates, uncertainty_spans, uncertainty_samples, uncertainty_seed,
                            uncertainty_lengths, estimate_lengths)
    ests = list(estimators)
    cal_q: Dict[int, np.ndarray] = {}
    if estimate_lengths:
        animals = _animals(ests)
        for idx in animals.values():                                                 # (every refusal before the first solve)
            _check_lengths([ests[i] for i in idx], length_prior_sigma)
        for idx in animals.values():
            cal = calibrate_lengths([ests[i] for i in idx], prior_sigma=length_prior_sigma, length_scale_init=length_scale_init,
                                    monocular_constraints=monocular_constraints, disable_pose_prior=disable_pose_prior,
                                    disable_motion_prior=disable_motion_prior, options=options, ridge=length_ridge, solver_output=solver_output)
            cal_q.update({i: cal["q"][b] for b, i in enumerate(idx)})
    spans = _spans_of(req, ests)
    out: List[Optional[bool]] = [None] * len(ests)
    groups: Dict[tuple, List[int]] = {}
    prepared = {}
    for i, est in enumerate(ests):
        if est.params.enable_shutter_delay_estimation and est.scene.cam_idx is None:
            out[i] = estimate_kinematics(est, solver_output, monocular_constraints, disable_pose_prior, disable_motion_prior, out_dir_prefix=out_dir_prefix, options=options,
                                         uncertainty=uncertainty, uncertainty_ridge=uncertainty_ridge, uncertainty_rates=uncertainty_rates,
                                         uncertainty_spans=uncertainty_spans, uncertainty_samples=uncertainty_samples, uncertainty_seed=uncertainty_seed)
            continue
        q_init, opts, pri = _kin_prepare(est, monocular_constraints, disable_pose_prior, disable_motion_prior, 5, 4, True, cal_q.get(i),
                                         None if options is None else _struct_copy(options))
        prepared[i] = (q_init, opts, pri)
        if req is not None:
            _check_uncertainty(est, pri, req.ridge)
        if ragged:
            key = ragged_group_key(est.skeleton, opts, pri, est.device)
        else:
            key = (_struct_bytes(est.skeleton), b"".join(_struct_bytes(est.cams[c]) for c in range(len(est.cams))), q_init.shape[0], _struct_bytes(opts),
                   None if pri is None else _struct_bytes(pri), est.device)
        groups.setdefault(key, []).append(i)
    for idx in groups.values():
        _solve_kinematic_group(ests, idx, prepared, out, ragged, req, spans, (solver_output, monocular_constraints, out_dir_prefix))
    return [bool(v) for v in out]


def _model_bytes(est: CheetahEstimator, opts: abi.Options) -> bytes:
    return _struct_bytes(est.skeleton) + b"".join(_struct_bytes(est.cams[c]) for c in range(len(est.cams))) + _struct_bytes(opts)


def _models_of(keys) -> Tuple[List[int], List[int]]:
    """model de-duplication of a group: (of = the model of every sequence, numbered in order of first appearance; the place of every model's
    first sequence) from what tells the sequences' models apart"""
    models: Dict[bytes, int] = {}
    of = [models.setdefault(k, len(models)) for k in keys]
    return of, [of.index(k) for k in range(len(models))]


class _GroupHandles:
    """The handles of one group in its form.  models: (skeleton, cameras, options) of every sequence; keys: what tells their models apart.
    Plain (keys None): `solve` is ONE handle of the first sequence's model and serves every sequence's forward kinematics as well; `of` is None.
    Ragged: `solve` is a Handle.multi over the distinct models, `of` the model of every sequence, and fk(b) a plain handle of sequence b's model
    (forward kinematics of that skeleton), made when first asked for and kept per model."""

    def __init__(self, models, pri, device: int, keys=None):
        self.of, self._fk = None, {}
        if keys is None:
            self.solve = _lib.Handle(*models[0], pri, device=device)
        else:
            self.of, reps = _models_of(keys)
            self._models, self._device = [models[b] for b in reps], device
            self.solve = _lib.Handle.multi(*(list(v) for v in zip(*self._models)), pri, device=device)

    def fk(self, b: int):
        if self.of is None:
            return self.solve
        k = self.of[b]
        if k not in self._fk:
            self._fk[k] = _lib.Handle(*self._models[k], None, device=self._device)
        return self._fk[k]

    def close(self) -> None:
        for h in [self.solve] + list(self._fk.values()):
            h.close()


def _sequence_of(res: dict, b: int) -> dict:
    """sequence b of a batched solve's result (plain: arrays [B, N, ...]; ragged: lists of per-sequence arrays) as the result of ONE sequence"""
    one = {k: (res[k][b][None] if isinstance(res[k], list) else res[k][b:b + 1]) for k in _lib.KINETIC_OUTPUTS if k in res}
    one.update({k: [res[k][b]] for k in ("stats", "kstats") if k in res}, status=res["stats"][b].status)
    return one


def _solve_kinematic_group(ests, idx, prepared, out, ragged: bool, req: Optional[PosteriorRequest], spans: Optional[list], finish: tuple,
                           single: bool = False) -> None:
    """estimate_kinematics (single: the group of one) and estimate_kinematics_batch for one group, plain (one model and length: ONE cpe_solve call
    with B = the group's size) or ragged (one model per distinct (skeleton, rig, options): ONE cpe_solve_ragged call): the solve, with req the
    posterior chain on the same handle at the stored q, then every sequence's centre of mass, costs and files through _kin_finish(..., *finish).
    spans: the resolved spans of ALL estimators, or None."""
    seqs = [ests[i] for i in idx]
    a = tuple(_gather(v, ragged) for v in ([prepared[i][0] for i in idx], [e.meas for e in seqs], [e.weight for e in seqs]))
    hs = _GroupHandles([(e.skeleton, e.cams, prepared[i][1]) for e, i in zip(seqs, idx)], prepared[idx[0]][2], seqs[0].device,
                       [_model_bytes(e, prepared[i][1]) for e, i in zip(seqs, idx)] if ragged else None)
    try:
        t0 = time()
        res = hs.solve.solve_ragged_host(*a, hs.of) if ragged else hs.solve.solve_host(*a)
        dt = (time() - t0) / len(idx)                                                # processing_time_s of a sequence: its share of the batched solve
        cov = None
        # THE asymmetry of the kinematic stage, kept as it is: a single call asks nothing of the library after a solve that did not converge; a
        # batch asks for its whole group and discards what such a sequence does not need
        if req is not None and not (single and res["stats"][0].status != abi.OK):
            cov = _posterior(hs.solve, req, None if spans is None else [spans[i] for i in idx], res["q"],
                             _Group(a[1:], hs.of, None, _length_group(seqs, hs.of) if req.lengths else None))
        for b, i in enumerate(idx):
            ests[i].shutter_delay = None
            unc = None if req is None else (None if cov is None else _uncertainty_of(cov, b, req.ridge), req.ridge)
            out[i] = _kin_finish(ests[i], hs.fk(b), _sequence_of(res, b), dt, *finish, uncertainty=unc,
                                 samples=None if cov is None else _samples_of(cov, b, req.ridge))
    finally:
        hs.close()


def _dataset_worker(rank: int, n_ranks: int, device: int, jobs: List[dict], estimate_kwargs: dict, queue) -> None:
    """one process of run_kinematics_dataset: builds the estimators of its shard on its GPU and solves them batched"""
    from . import sharding
    try:
        mine = [int(i) for i in sharding.shard_indices(len(jobs), rank, n_ranks)]
        ests = [init_trajectory(device=device, **jobs[i]) for i in mine]
        oks = estimate_kinematics_batch(ests, **estimate_kwargs)
        queue.put((rank, mine, oks, None))
    except Exception as exc:                                                          # the parent re-raises
        import traceback
        queue.put((rank, [], [], f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


def run_kinematics_dataset(jobs: Sequence[dict], devices: Sequence[int] = (0,), **estimate_kwargs) -> List[bool]:
    """A whole data set of sequences across the GPUs of one node (BASELINE config 5; the reference loops over them one by one on the CPU,
    run_dataset.py:1143-1231).  jobs: one dictionary of init_trajectory keyword arguments per sequence (root_dir, data_path, cheetah_name,
    kinetic_dataset, kinematic_model=True, ...).  Sequence i goes to rank i mod G (sharding.shard_indices: independent sequences, no collective on
    the solve path); every rank is a FRESH process started before it touches its GPU (spawn, not fork), builds its estimators with init_trajectory
    (DLC tables -> measurement tensors on its GPU), solves them with estimate_kinematics_batch and writes each sequence's files.  Returns one bool
    per job, in order.  devices may name one GPU several times (rehearsal of the multi-rank path on a one-GPU box)."""
    jobs = [dict(j) for j in jobs]
    G = len(devices)
    if G == 1:
        ests = [init_trajectory(device=devices[0], **j) for j in jobs]
        return estimate_kinematics_batch(ests, **estimate_kwargs)
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    procs = [ctx.Process(target=_dataset_worker, args=(r, G, int(devices[r]), jobs, estimate_kwargs, queue)) for r in range(G)]
    for p_ in procs:
        p_.start()
    results, errors = [None] * len(jobs), []
    for _ in range(G):
        rank, mine, oks, err = queue.get()
        if err:
            errors.append(f"rank {rank}: {err}")
        for i, ok in zip(mine, oks):
            results[i] = bool(ok)
    for p_ in procs:
        p_.join()
    if errors:
        raise RuntimeError("run_kinematics_dataset: " + " | ".join(errors))
    return results


def determine_contacts(estimator: CheetahEstimator, monocular: bool = False, verbose: bool = True,
                       out_dir_prefix: Optional[str] = None):
    """Contact windows from the kinematic reconstruction + template forces, acinoset_opt.py:636-692: reads
    `fte_kinematic[_<cam>]/fte.pickle` (written by `CheetahEstimator.save`), evaluates foot heights and analytic foot
    velocities on the GPU (cpe_forward_kinematics, cpe_marker_velocities), applies the height / zero-velocity / stance-time
    heuristic (contacts.contact_detection) and writes `grf/autogen-contact.json`, `grf/autogen-contact-02.json` and the two
    synthetic force tables.  Returns (contacts, contacts_height_only) -- the reference prints them and returns None."""
    from . import contacts as ct
    params, scene, sk = estimator.params, estimator.scene, estimator.skeleton
    data_dir = params.data_dir if out_dir_prefix is None else os.path.join(out_dir_prefix, estimator.data_path)
    sub = "fte_kinematic" if not monocular else f"fte_kinematic_{scene.cam_idx}"
    fte = load_result_pickle(os.path.join(data_dir, sub, "fte.pickle"))           # restricted unpickler: arrays and numbers only
    estimator.com_vel, estimator.com_pos = fte["com_vel"], fte["com_pos"]
    h = _lib.Handle(sk, estimator.cams, device=estimator.device)
    try:
        pos, vel = h.kinematics_host(fte["q"][None], fte["dq"][None])
    finally:
        h.close()
    feet_idx = [skeleton.MARKERS.index(m) for m in skeleton.FOOT_MARKERS]
    names = [f"{f}_foot" for f in skeleton.FEET]
    speed = float(np.mean(np.linalg.norm(estimator.com_vel, axis=1)))
    contacts, by_height = ct.contact_detection(pos[0][:, feet_idx, 2], vel[0][:, feet_idx, 2], names, params.start_frame, speed, scene.fps)
    if verbose:
        print("Height, velocity, stance time heuristic:")
        print(contacts)
        print("Height:")
        print(by_height)
    grf_dir = os.path.join(data_dir, "grf")
    n_frames = pos.shape[1]
    ct.write_contacts(grf_dir, params.start_frame, n_frames, contacts, by_height)
    direction = 1.0 if float(np.mean(estimator.com_vel, axis=0)[0]) < 0 else -1.0
    for cname, oname in (("autogen-contact.json", "data_synth"), ("autogen-contact-02.json", "data_synth_02")):
        with open(os.path.join(grf_dir, cname), "r", encoding="utf-8") as fh:
            cj = json.load(fh)
        ct.write_synth_grf(os.path.join(grf_dir, f"{oname}.csv"), ct.synth_grf(cj, names, speed, direction))
    return contacts, by_height


DETECTION_FIELDS = ("uv", "uv_cov", "uv_std", "uv_loo", "uv_loo_cov", "residual", "residual_loo", "d2_loo", "leverage", "outlier", "held_out", "chi2",
                    "p_outlier", "ridge", "n_detections", "dof_measurements", "log_score", "log_score_held_out")
DETECTION_CSV_COLUMNS = ("x", "y", "x_std", "y_std", "xy_corr", "x_loo", "y_loo", "d2_loo", "leverage", "outlier", "held_out")


def loss_centre_curvature(a: float, b: float, c: float) -> float:
    """kappa0 = rho''(0) of the redescending loss with knots a < b < c (acinoset_misc.py:2001-2015): the loss is the Gaussian of variance 1 / kappa0 at
    its centre (1.0392 with the default knots 3, 10, 20: the switch at a = 3 is not quite off at the centre)"""
    with np.errstate(over="ignore"):                                        # (knots out of reach: exp overflows to a switch that is off)
        sa, sb, sc = (1.0 / (1.0 + np.exp(k)) for k in (a, b, c))           # the three sigmoid switches at e = 0
    d1 = lambda x: x * (1.0 - x)
    d2 = lambda x: x * (1.0 - x) * (1.0 - 2.0 * x)
    cb = c - b
    lin, kq, K = -0.5 * a * a, a * b - 0.5 * a * a + 0.5 * a * cb * (1.0 - (c / cb) ** 2), a * b - 0.5 * a * a + 0.5 * a * cb
    k1, k2 = a * c / cb, -a / cb
    return max(0.0, float((1.0 - sa) + (d2(sa) - d2(sb)) * lin + 2.0 * (d1(sa) - d1(sb)) * a + (d2(sb) - d2(sc)) * kq + 2.0 * (d1(sb) - d1(sc)) * k1
                          + (sb - sc) * k2 + d2(sc) * K))


def _kinematic_dir(est: CheetahEstimator, out_dir_prefix: Optional[str]) -> str:
    """the directory _kin_finish saved the kinematic estimate to: the one of its names (with or without monocular constraints) whose fte.pickle is the
    newest; FileNotFoundError naming the first where there is none"""
    params, scene = est.params, est.scene
    data_dir = params.data_dir if out_dir_prefix is None else os.path.join(out_dir_prefix, est.data_path)
    base = f"fte_kinematic{'_gt' if params.hand_labeled_data else ''}"
    names = [base] if scene.cam_idx is None else [f"{base}_{scene.cam_idx}", f"{base}_orig_{scene.cam_idx}"]
    found = [d for d in (os.path.join(data_dir, n) for n in names) if os.path.exists(os.path.join(d, "fte.pickle"))]
    if not found:
        raise FileNotFoundError(os.path.join(data_dir, names[0], "fte.pickle"))
    return max(found, key=lambda d: os.path.getmtime(os.path.join(d, "fte.pickle")))


def detection_fields(raw: dict, meas: np.ndarray, weight: np.ndarray, weight_fit: np.ndarray, mult: np.ndarray, kappa0: float, p_outlier: float,
                     ridge: float, held_out_cams: np.ndarray) -> dict:
    """DETECTION_FIELDS of one sequence from Handle.detection_report_host's arrays [N, C, L, ..]: the residuals, the outlier flags at the exact
    chi-square quantile -2 ln(p_outlier), and the sums -- the detections counted, the degrees of freedom they buy (the hat matrix's trace) and the
    leave-one-out log predictive score -log(2 pi) - log det(S_loo + sigma2 I) / 2 - d2 / 2, over the fitted and over the held-out detections"""
    w = mult[None, :, None] * weight
    seen = w > 0.0
    d2 = raw["d2"]
    chi2 = -2.0 * np.log(p_outlier)
    held = np.broadcast_to(held_out_cams[None, :, None], weight.shape).copy()
    fitted = seen & (mult[None, :, None] * weight_fit > 0.0) & ~held
    defined = seen & np.isfinite(d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        C = raw["cov_loo"] + (1.0 / (w * w * kappa0))[..., None, None] * np.eye(2)
        dens = -np.log(2.0 * np.pi) - 0.5 * np.log(C[..., 0, 0] * C[..., 1, 1] - C[..., 0, 1] * C[..., 1, 0]) - 0.5 * d2
    nan2 = np.where(seen[..., None], 0.0, np.nan)
    return dict(uv=raw["uv"], uv_cov=raw["cov_px"], uv_std=np.sqrt(np.diagonal(raw["cov_px"], axis1=-2, axis2=-1)), uv_loo=raw["uv_loo"],
                uv_loo_cov=raw["cov_loo"], residual=meas - raw["uv"] + nan2, residual_loo=meas - raw["uv_loo"] + nan2, d2_loo=d2,
                leverage=raw["leverage"], outlier=defined & (d2 > chi2), held_out=held, chi2=float(chi2), p_outlier=float(p_outlier), ridge=float(ridge),
                n_detections=int(defined.sum()), dof_measurements=float(raw["leverage"][fitted].sum()),
                log_score=float(dens[defined & fitted].sum()), log_score_held_out=float(dens[defined & held].sum()))


def write_detection_csv(path: str, det: dict, c: int, start_frame: int) -> None:
    """one camera's rows of the report: a plain header, then one row per frame and marker (DETECTION_CSV_COLUMNS; numbers as repr, flags as 0 / 1)"""
    S = det["uv_cov"][:, c]
    std = det["uv_std"][:, c]
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = S[..., 0, 1] / (std[..., 0] * std[..., 1])
    cols = [det["uv"][:, c, :, 0], det["uv"][:, c, :, 1], std[..., 0], std[..., 1], corr, det["uv_loo"][:, c, :, 0], det["uv_loo"][:, c, :, 1],
            det["d2_loo"][:, c], det["leverage"][:, c]]
    flags = [det["outlier"][:, c], det["held_out"][:, c]]
    N, L = cols[0].shape
    names = [skeleton.MARKERS[l] if l < len(skeleton.MARKERS) else f"marker{l}" for l in range(L)]
    with open(path, "w") as f:
        f.write("frame,marker," + ",".join(DETECTION_CSV_COLUMNS) + "\n")
        for n in range(N):
            for l in range(L):
                f.write(f"{start_frame + n},{names[l]}," + ",".join(repr(float(a[n, l])) for a in cols) + "," +
                        ",".join(str(int(a[n, l])) for a in flags) + "\n")


def detection_report(estimator: CheetahEstimator, validate_with: Optional[CheetahEstimator] = None, p_outlier: float = 1e-3,
                     out_dir_prefix: Optional[str] = None, write: bool = True, options: Optional[abi.Options] = None) -> dict:
    """Where in every camera's image every marker is, give or take how many pixels, and which detections disagree with everything else the estimate
    knows ("What is predicted in the image"; cpe_detection_report).  Runs after estimate_kinematics(uncertainty=True) or
    estimate_kinematics_batch, as determine_contacts does: the positions and their CONDITIONAL covariance (positions_cov, never the _marginal one:
    the leave-one-out identity needs the covariance of the fit the detections were in) come from the estimator where it holds them, else from
    fte.pickle and uncertainty.npz in the directory `save` wrote (FileNotFoundError names the missing file).  Returns DETECTION_FIELDS, keeps them
    as est.detections and, with write=True, writes detections.npz beside uncertainty.npz and one cam{c+1}_detections.csv per camera, numbered as the
    scene's cameras are; cam*_fte.csv, fte.pickle and uncertainty.npz are not touched.
    validate_with: a second estimator of the same sequence initialised multi-view (same frame range and skeleton, else ValueError).  Its cameras,
    meas and weight span the report; the cameras outside `estimator`'s fit are held out (weight_fit = 0), so with a monocular `estimator` this is
    the cross-validation of the one-camera posterior: log_score_held_out is its predictive score on the cameras it did not see.
    outlier = d2_loo > chi2 = -2 ln(p_outlier), the exact upper quantile of a chi-square with 2 degrees of freedom.
    options: the options the estimate was made with where they were not the defaults (the loss's knots and curvature mode enter the report).
    NotImplementedError: pairwise pseudo-measurements (the three slices of a camera are not independent detections) and a physics-stage result."""
    est = estimator
    if not (0.0 < p_outlier < 1.0):
        raise ValueError(f"p_outlier must lie inside (0, 1), got {p_outlier!r}")
    for e, who in ((est, "estimator"), (validate_with, "validate_with")):
        if e is not None and e.params.enable_ppms:
            raise NotImplementedError(f"detection_report: {who} was built with pairwise pseudo-measurements; the three slices of a camera are not "
                                      "independent detections, and leaving one slice out does not leave the detection out")
    if est.kinetic is not None:
        raise NotImplementedError("detection_report: the estimator holds a physics-stage result; the report is that of the kinematic estimate "
                                  "(the force unknowns are out of scope)")
    params, scene = est.params, est.scene
    if validate_with is not None:
        v = validate_with
        if v.scene.cam_idx is not None:
            raise ValueError("detection_report: validate_with must be initialised multi-view")
        if (v.params.start_frame, v.params.end_frame) != (params.start_frame, params.end_frame):
            raise ValueError(f"detection_report: validate_with covers frames {v.params.start_frame}..{v.params.end_frame}, the estimator "
                             f"{params.start_frame}..{params.end_frame}")
        if _struct_bytes(v.skeleton) != _struct_bytes(est.skeleton):
            raise ValueError("detection_report: validate_with has a different skeleton")
    # the estimate: from the estimator where set, otherwise from the files of its save
    out_dir = None
    if est.result is not None and est.uncertainty is None:
        raise ValueError("detection_report: the estimate has no covariance (est.uncertainty is None: not asked for, or the Gauss-Newton matrix had no "
                         "Cholesky factor); run estimate_kinematics(uncertainty=True)")
    if est.result is not None:
        pos, unc = est.result["positions"][0], est.uncertainty
    else:
        out_dir = _kinematic_dir(est, out_dir_prefix)
        pos = load_result_pickle(os.path.join(out_dir, "fte.pickle"))["positions"]
        if not os.path.exists(os.path.join(out_dir, "uncertainty.npz")):
            raise FileNotFoundError(os.path.join(out_dir, "uncertainty.npz"))
        with np.load(os.path.join(out_dir, "uncertainty.npz")) as z:
            unc = dict(positions_cov=z["positions_cov"], ridge=float(z["ridge"]))
    if "tau_std" in unc:
        raise NotImplementedError("detection_report: the covariance is that of a physics-stage result (out of scope)")
    if write and out_dir is None:
        out_dir = _kinematic_dir(est, out_dir_prefix)
    # the cameras, detections and weights the report spans, and the weights the fit used
    own = list(range(scene.n_cams)) if scene.cam_idx is None else [scene.cam_idx]
    if validate_with is None:
        cams, cam_ids, meas, weight, weight_fit = est.cams, own, est.meas, est.weight, est.weight
    else:
        cams, cam_ids, meas, weight = v.cams, list(range(v.scene.n_cams)), v.meas, v.weight
        weight_fit = np.zeros_like(weight)
        for j, c in enumerate(own):
            weight_fit[:, c] = est.weight[:, j]
    held_cams = np.array([c not in own for c in cam_ids])
    opts = options if options is not None else abi.default_options(scene.fps)
    if options is None and params.hand_labeled_data:
        opts.loss_a, opts.loss_b, opts.loss_c = 1e6, 2e6, 3e6          # (_kin_prepare)
    h = _lib.Handle(est.skeleton, cams, opts, device=est.device)
    try:
        raw = h.detection_report_host(pos[None], unc["positions_cov"][None], meas[None], weight[None], weight_fit[None])
    finally:
        h.close()
    raw = {k: a[0] for k, a in raw.items()}
    mult = np.array([cams[j].mult for j in range(len(cams))])
    det = detection_fields(raw, np.asarray(meas, dtype=np.float64), np.asarray(weight, dtype=np.float64), np.asarray(weight_fit, dtype=np.float64), mult,
                           loss_centre_curvature(opts.loss_a, opts.loss_b, opts.loss_c), p_outlier, float(unc["ridge"]), held_cams)
    assert tuple(det) == DETECTION_FIELDS
    est.detections = det
    if write:
        np.savez(os.path.join(out_dir, "detections.npz"), **det)
        off = [0] * scene.n_cams
        if params.sync_offset is not None:
            for o in params.sync_offset:
                off[o["cam"]] = o["frame"]
        for j, c in enumerate(cam_ids):                              # rows numbered as cam{c+1}_fte.csv's are (save)
            write_detection_csv(os.path.join(out_dir, f"cam{c + 1}_detections.csv"), det, j, params.start_frame - off[c])
    return det


def stance_from_contacts(contact_json: dict, n_frames: int) -> np.ndarray:
    """contact windows [first, last, foot, label] of `autogen-contact.json` / metadata.json -> stance[N, 4] in skeleton.FEET order: node
    first - start_frame ... last - start_frame INCLUSIVE with start_frame = the CONTACT FILE's own (`contact_times` of acinoset_opt.py:787-798:
    `(f_contact[0] - start_frame) + 1` in Pyomo's one-based finite elements)"""
    start = contact_json["start_frame"]
    st = np.zeros((n_frames, len(skeleton.FEET)), np.int32)
    for k, foot in enumerate(skeleton.FEET):
        for win in (contact_json["contacts"].get(f"{foot}_foot") or []):
            a, b = int(win[0]) - start, int(win[1]) - start
            st[max(a, 0):max(min(b + 1, n_frames), 0), k] = 1
    return st


def load_force_table(path_csv: str) -> Dict[int, np.ndarray]:
    """`grf/data_synth.csv` (or a `grf/data.csv` twin of the measured force plates): {force plate: array [rows, 3] = (Fx, Fy, Fz)} in file order --
    the table the reference reads with `pd.read_hdf(...).query("force_plate == k")` (acinoset_misc.py:960, :981)"""
    rows = np.genfromtxt(path_csv, delimiter=",", skip_header=1)
    rows = rows.reshape(-1, 5)
    return {int(k): rows[rows[:, 0] == k][:, 2:5] for k in np.unique(rows[:, 0])}


def resample_force_plate(x: np.ndarray, up: int = 2, down: int = 35, dc_samples: int = 500) -> np.ndarray:
    """One channel of the measured force plates (`grf/data.h5`, 3.5 kHz) on the 200 Hz frame grid, as `get_grf_profile(synthetic_data=False)` prepares
    it for the kinetic dataset (acinoset_misc.py:985-1000): the mean of the first `dc_samples` samples is removed (`remove_dc_offset(x, 500)`, :717-719),
    then `scipy.signal.resample_poly(x, up=2, down=35)`: zero-stuffing by 2, the default Kaiser-windowed (beta 5) low-pass FIR of half-length
    10 max(up, down) with cut-off 1 / max(up, down) and gain `up`, decimation by 35, output length ceil(2 len / 35)."""
    from scipy import signal
    x = np.asarray(x, dtype=np.float64)
    return signal.resample_poly(x - np.mean(x[:dc_samples], axis=0), up=up, down=down, axis=0)


def grf_profile(plates: Dict[int, np.ndarray], contact_json: dict, n_frames: int, absolute_rows: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """`misc.get_grf_profile` on per-frame tables (acinoset_misc.py:946-1026): grfz [N, 4] and grfxy [N, 4, 4] (friction-polygon sides +x, +y, -x,
    -y) in skeleton.FEET order.  As there: only the FIRST contact of a foot (it "assumes a single stride"), frames 0 .. N-2
    (`for fe in range(1, nfe)`), and of the horizontal force only the LARGEST positive polygon component is kept.  Row convention: a synthetic table
    (`data_synth`) starts at the contact file's start frame -- frame n reads row n (`Fz[fe - 1]`, :1003-1006); the resampled MEASURED plates of the
    kinetic dataset start with the recording -- frame n reads row start_frame + n (`Fz[start_frame + fe - 1]`, :1007-1010): `absolute_rows=True`."""
    start = contact_json["start_frame"]
    gz = np.zeros((n_frames, len(skeleton.FEET))); gxy = np.zeros((n_frames, len(skeleton.FEET), 4))
    for k, foot in enumerate(skeleton.FEET):
        rec = contact_json["contacts"].get(f"{foot}_foot")
        if not rec:
            continue
        first, last, plate = int(rec[0][0]), int(rec[0][1]), int(rec[0][2]) - 1
        F = plates.get(plate)
        if F is None:
            continue
        for n in range(n_frames - 1):
            row = start + n if absolute_rows else n
            if first <= start + n <= last and 0 <= row < len(F):
                fx, fy, fz = F[row]
                gz[n, k] = fz
                comps = np.array([fx, fy, -fx, -fy])
                i = int(np.argmax(comps))
                if comps[i] > 0:
                    gxy[n, k, i] = comps[i]
    return gz, gxy


def load_measured_plates(grf_dir: str, direction: float, scale_forces_by: float) -> Optional[Dict[int, np.ndarray]]:
    """CSV twins of the reference's `grf/data.h5` (PyTables is absent; columns force_plate, sample, Fx, Fy, Fz as `load_force_table` reads them):
    `data.csv` = one row per video frame from the start of the recording, already resampled and in body weights; `data_3500hz.csv` = the raw 3.5 kHz
    samples in newtons, resampled here exactly as the reference does (`measured_force_plates`).  None if neither exists."""
    per_frame = os.path.join(grf_dir, "data.csv")
    if os.path.exists(per_frame):
        return load_force_table(per_frame)
    raw = os.path.join(grf_dir, "data_3500hz.csv")
    if os.path.exists(raw):
        return measured_force_plates(load_force_table(raw), direction, scale_forces_by)
    return None


def measured_force_plates(raw: Dict[int, np.ndarray], direction: float, scale_forces_by: float) -> Dict[int, np.ndarray]:
    """raw {plate: [samples, 3] = (Fx, Fy, Fz) at 3.5 kHz, newtons} -> the per-frame table `grf_profile(..., absolute_rows=True)` reads: every channel
    resampled by 2 / 35 after its DC offset is removed, Fx and Fy times the running direction, all times `scale_forces_by` = 1 / (M g)
    (acinoset_misc.py:985-1000)"""
    out = {}
    for k, F in raw.items():
        F = np.asarray(F, dtype=np.float64)
        out[k] = np.stack([direction * resample_force_plate(F[:, 0]) * scale_forces_by, direction * resample_force_plate(F[:, 1]) * scale_forces_by,
                           resample_force_plate(F[:, 2]) * scale_forces_by], axis=1)
    return out


def estimate_kinetics(estimator: CheetahEstimator, init_torques: bool = True, auto: bool = True, use_2d_reprojections: bool = True,
                      solver_output: bool = True, init_prev_kinematic_solution: bool = True, synthesised_grf: bool = False,
                      no_slip: bool = True, joint_estimation: bool = False, fix_grf: bool = True, ground_constraint: bool = False,
                      disable_pose_prior: bool = False, disable_motion_prior: bool = False, plot: bool = False, out_fname: str = "fte",
                      out_dir_prefix: Optional[str] = None, options: Optional[abi.Options] = None,
                      kinetic_options: Optional[abi.KineticOptions] = None, uncertainty: bool = False, uncertainty_ridge: float = 0.0,
                      uncertainty_rates: bool = False, uncertainty_spans=None, track_weights: str = "reference", track_scale: float = 1.0,
                      uncertainty_samples: int = 0, uncertainty_seed: int = 0) -> bool:
    """Same signature and meaning as acinoset_opt.estimate_kinetics (acinoset_opt.py:693-708) for the branch its drivers run for the
    physics-based reconstruction (`joint_estimation=True`, run_dataset.py:1198-1229): torques, joint constraint forces, ground-reaction
    forces and the trajectory are estimated together, warm-started from the kinematic solution on disk, with the contact windows of
    `grf/autogen-contact.json` (auto) or `metadata.json`; and for the branch of the kinetic-dataset driver (`joint_estimation=False`,
    `fix_grf=True`, run_dataset.py:1092-1140; acinoset_opt.py:813-866): the ground-reaction forces are PRESCRIBED -- the synthesised profile of
    `grf/data_synth.csv` (`synthesised_grf=True`) or the per-frame fit of `CheetahEstimator.estimate_grf` -- the feet are held near the ground
    (`ground_constraint`) and still (`no_slip`) while their force is positive, and torques, constraint forces and the trajectory are estimated
    (cpe_solve_kinetic_fixed).  With `fix_grf=False` the same profile only BOXES the forces (acinoset_opt.py:838-850: `GRFz` and every `GRFxy` side
    within `bound_value(profile, 0.2)`; cpe_solve_kinetic_force_box): net z in [0.8, 1.2] x profile, net x / y from the boxes of the two opposite
    polygon sides (a side is non-negative), friction polyhedron kept; feet outside the profile's contact carry no force (the reference would let
    them take up to 0.2 body weights: its box around zero).  The whole NLP runs on the GPU.  `init_torques` has no effect here: the torques are
    minimised out exactly at every evaluation, so they need no starting value.
    uncertainty=True: after a successful solve the posterior covariance of the estimate AND of its node forces (cpe_covariance_kinetic at the stored
    q with the solve's stance, options and force profile, damping uncertainty_ridge) goes to est.uncertainty and to uncertainty.npz beside fte.pickle:
    estimate_kinematics' fields plus tau_std, lambda_std, grf_std, tau_cov (force_uncertainty).  A sequence without a factor raises CpeError after the
    solve's own files are written.  Not with use_2d_reprojections=False (the covariance of the 3D kinematic cost is not built).
    uncertainty_rates=True (with uncertainty=True): the rate fields of estimate_kinematics (RATE_FIELDS), from that covariance.
    uncertainty_spans (with uncertainty=True): the span fields of estimate_kinematics (SPAN_FIELDS), from that covariance.
    uncertainty_samples=K > 0 (with uncertainty=True): K draws from the JOINT posterior of coordinates and node forces ("What is
    sampled (forces)"), for the error bar of anything computed from forces of several frames or from forces and poses -- an impulse, a peak force,
    joint power.  du = L^-T z as in estimate_kinematics (z = sample_normals(uncertainty_seed, K, N), the covariance call's own factor), the poses,
    then ONE cpe_force_samples call with zeta = sample_force_normals(uncertainty_seed, K, N).  est.samples and samples.npz beside uncertainty.npz
    hold KINETIC_SAMPLE_FIELDS: estimate_kinematics' fields plus tau [K, N, n_motors], lam [K, N, n_con], grf_net [K, N, n_feet, 3] (z, x, y) and
    tau_mean, lam_mean, grf_net_mean, the forces the draws are centred on -- the covariance call's cold-start evaluation at the stored q with
    multipliers zero, not fte.pickle's forces.  est.uncertainty and uncertainty.npz do not change.
    track_weights (use_2d_reprojections=False): "reference" = the reference's 28 constants; "posterior" = frame n is tracked with its own matrix
    W_n = (track_scale / 2) (X Sigma_nn X^T)^-1 from cov_u of the uncertainty.npz that estimate_kinematics(uncertainty=True) wrote beside the
    kinematic result (one cpe_track_precision call, then cpe_solve_kinetic_tracked_weighted; DESIGN.md 2b has the approximation and what
    track_scale is for).  "posterior" with use_2d_reprojections=True, or any other string, is a ValueError."""
    req = posterior_request(uncertainty, uncertainty_ridge, uncertainty_rates, uncertainty_spans, uncertainty_samples, uncertainty_seed)
    _check_track_weights(track_weights, track_scale, use_2d_reprojections)
    spans = _spans_of(req, [estimator])
    _check_tracked_uncertainty(req, use_2d_reprojections)
    prep = _kinetic_prepare(estimator, auto, use_2d_reprojections, init_prev_kinematic_solution, synthesised_grf, no_slip, joint_estimation, fix_grf,
                            ground_constraint, disable_pose_prior, disable_motion_prior, out_dir_prefix, options, kinetic_options,
                            track_weights=track_weights, track_scale=track_scale)
    if req is not None:
        _lib.covariance_supported(prep["pri"], req.ridge)                  # raises with the library's reason (negative or non-finite ridge)
    out = [None]
    _solve_kinetic_group([estimator], [0], {0: prep}, out, False, req, spans, (solver_output, out_fname, out_dir_prefix))      # the plain group of one
    return out[0]


def _check_tracked_uncertainty(req: Optional[PosteriorRequest], use_2d_reprojections: bool) -> None:
    """what the physics-based stage refuses of uncertainty=True before anything is prepared"""
    if req is not None and not use_2d_reprojections:
        raise NotImplementedError("uncertainty together with use_2d_reprojections=False: cpe_covariance_kinetic takes the reprojection cost; the covariance "
                                  "of the 3D kinematic cost (cpe_solve_kinetic_tracked) is not built")


def kinematic_result_path(data_dir: str, cam_idx: Optional[int], init_prev_kinematic_solution: bool) -> str:
    """the kinematic result estimate_kinetics starts from, and with use_2d_reprojections=False also tracks (init_q, acinoset_opt.py:739-744):
    fte_kinematic_<cam>/fte.pickle for a monocular estimator with init_prev_kinematic_solution, else fte_kinematic/fte.pickle"""
    mono = cam_idx is not None and init_prev_kinematic_solution
    return os.path.join(data_dir, f"fte_kinematic_{cam_idx}" if mono else "fte_kinematic", "fte.pickle")


TRACK_WEIGHTS = ("reference", "posterior")


def _check_track_weights(track_weights: str, track_scale: float, use_2d_reprojections: bool) -> None:
    """what the track_weights / track_scale keywords refuse, before anything is looked at"""
    if track_weights not in TRACK_WEIGHTS:
        raise ValueError(f"track_weights={track_weights!r}: expected one of {TRACK_WEIGHTS}")
    if track_weights == "posterior" and use_2d_reprojections:
        raise ValueError('track_weights="posterior" weights the 3D kinematic cost: it requires use_2d_reprojections=False')
    if not (np.isfinite(track_scale) and track_scale > 0.0):
        raise ValueError(f"track_scale={track_scale!r}: expected a finite number > 0")


def load_posterior_blocks(kinematic_pickle: str, n_frames: int) -> np.ndarray:
    """cov_u [n_frames, 28, 28] of the uncertainty.npz beside a kinematic result: the blocks track_weights="posterior" turns into weights"""
    path = os.path.join(os.path.dirname(kinematic_pickle), "uncertainty.npz")
    if not os.path.exists(path):
        raise FileNotFoundError(f'{path}: track_weights="posterior" reads the posterior covariance of the kinematic estimate; '
                                "estimate_kinematics(uncertainty=True) writes it beside its fte.pickle")
    with np.load(path) as z:
        cov_u = np.ascontiguousarray(z["cov_u"], dtype=np.float64)
    if cov_u.ndim != 3 or cov_u.shape[1:] != (abi.NX, abi.NX) or cov_u.shape[0] < n_frames:
        raise ValueError(f"{path}: cov_u has shape {cov_u.shape}, expected [at least {n_frames}, {abi.NX}, {abi.NX}]")
    return np.ascontiguousarray(cov_u[:n_frames])


def tracked_motion_options(ko: abi.KineticOptions, fps: float) -> abi.KineticOptions:
    """the motion energy of the 3D kinematic cost (acinoset_opt.py:913, :919-920): 1e-2 x torque in place of the marker smoothing, weighted
    0.1 fps^-2 -> w_torque = 1 + 1e-3 fps^-2, w_smooth = 0 (in place; returns ko)"""
    ko.w_torque, ko.w_smooth = 1.0 + 1e-3 / (fps * fps), 0.0
    return ko


def _kinetic_prepare(est: CheetahEstimator, auto: bool, use_2d_reprojections: bool, init_prev_kinematic_solution: bool, synthesised_grf: bool,
                     no_slip: bool, joint_estimation: bool, fix_grf: bool, ground_constraint: bool, disable_pose_prior: bool, disable_motion_prior: bool,
                     out_dir_prefix: Optional[str], options: Optional[abi.Options], kinetic_options: Optional[abi.KineticOptions],
                     track_weights: str = "reference", track_scale: float = 1.0) -> dict:
    """what estimate_kinetics sets up before the solver call: initial guess, contacts, stance, the force profile or its boxes, options, priors;
    with track_weights="posterior" also cov_u [N, 28, 28] of the kinematic estimate (weighted = True)"""
    params, scene, sk = est.params, est.scene, est.skeleton
    if est.kinematic_model:
        raise AssertionError("Dynamic model of the cheetah is required.")          # the reference asserts hasattr(model, 'eom_f')
    if not est.enable_eom_slack:
        raise NotImplementedError("enable_eom_slack=False (hard equations of motion, no slack cost, acinoset_opt.py:914): the slack IS the residual of this "
                                  "solver's least-squares model; no driver of the reference switches it off")
    if params.enable_shutter_delay_estimation and scene.cam_idx is None:
        raise NotImplementedError("shutter delays are estimated by estimate_kinematics only (cpe_solve_shutter); not inside the physics-based model")
    data_dir = params.data_dir if out_dir_prefix is None else os.path.join(out_dir_prefix, est.data_path)
    kin_path = kinematic_result_path(data_dir, scene.cam_idx, init_prev_kinematic_solution)
    fte = load_result_pickle(kin_path)
    est.com_vel, est.com_pos = fte["com_vel"], fte["com_pos"]
    N = params.end_frame - params.start_frame
    if init_prev_kinematic_solution:
        q_init = np.ascontiguousarray(fte["q"][:N], dtype=np.float64)                # acinoset_opt.py:768-777
    else:
        base_len = 2.0 * abs(sk.marker_off[5][0])
        x, y, z, psi = create_trajectory_estimate(est.tables, params, scene, base_len, device=est.device)
        q_init = np.zeros((N, sk.nq)); sl = slice(params.start_frame, params.start_frame + N)
        q_init[:, 0], q_init[:, 1], q_init[:, 2] = x[sl], y[sl], z[sl]
        for i in range(sk.n_links):
            q_init[:, 3 + 3 * i + 2] = psi[sl]
    with open(os.path.join(data_dir, "grf", "autogen-contact.json") if auto else os.path.join(params.data_dir, "metadata.json"), "r", encoding="utf-8") as fh:
        contact_json = json.load(fh)
    grf_fixed = None
    grf_box = None
    if joint_estimation:
        stance = stance_from_contacts(contact_json, N)
    else:
        if synthesised_grf:                                                          # acinoset_opt.py:814-820
            measured = (not auto) and params.kinetic_dataset                         # the resampled plates are indexed by absolute frame (acinoset_misc.py:1007-1010)
            if auto:
                table = os.path.join(data_dir, "grf", "data_synth.csv")
                plates = load_force_table(table) if os.path.exists(table) else None
            else:
                table = os.path.join(params.data_dir, "grf", "data.csv")
                direction = 1.0 if float(np.mean(est.com_vel, axis=0)[0]) < 0 else -1.0      # acinoset_opt.py:817
                plates = load_measured_plates(os.path.join(params.data_dir, "grf"), direction, 1.0 / est.scale_forces_by)
            if plates is None:
                raise FileNotFoundError(f"{table}: the force table of the prescribed-force branch (determine_contacts writes grf/data_synth.csv; the measured "
                                        "force plates ship as grf/data.h5 in the reference, which needs PyTables -- provide a CSV twin, data.csv or data_3500hz.csv)")
            gz, gxy = grf_profile(plates, contact_json, N, absolute_rows=measured)
        else:                                                                        # :821-822: the per-frame fit
            gzd, gxyd = est.estimate_grf(monocular=True, plot=False, out_dir_prefix=out_dir_prefix)
            gz = np.zeros((N, 4)); gxy = np.zeros((N, 4, 4))
            for k, foot in enumerate(skeleton.FEET):
                v = np.asarray(gzd[f"{foot}_foot"], dtype=np.float64); w = np.asarray(gxyd[f"{foot}_foot"], dtype=np.float64).reshape(-1, 4)
                gz[:min(N, len(v)), k] = v[:N]; gxy[:min(N, len(w)), k] = w[:N]
        est.synthesised_grf = {f"{foot}_foot": [float(v) for v in gz[:, k]] for k, foot in enumerate(skeleton.FEET)}
        stance = (gz > 0).astype(np.int32)                                           # height / no-slip rules where a force acts (:832-835, :853-864)
        grf_fixed = np.ascontiguousarray(np.stack([gz, gxy[..., 0] - gxy[..., 2], gxy[..., 1] - gxy[..., 3]], axis=-1))
        if not fix_grf:
            bz = bound_value(gz, 0.2)                                                  # [N, 4, 2]
            bs = np.maximum(bound_value(gxy, 0.2), 0.0)                                # [N, 4, 4 sides, 2]; a polygon side is >= 0
            grf_box = np.zeros((N, 4, 3, 2))
            grf_box[:, :, 0] = bz
            grf_box[:, :, 1, 0] = bs[:, :, 0, 0] - bs[:, :, 2, 1]; grf_box[:, :, 1, 1] = bs[:, :, 0, 1] - bs[:, :, 2, 0]      # x = (+x side) - (-x side)
            grf_box[:, :, 2, 0] = bs[:, :, 1, 0] - bs[:, :, 3, 1]; grf_box[:, :, 2, 1] = bs[:, :, 1, 1] - bs[:, :, 3, 0]
            grf_fixed = None
    pri = None
    if not disable_pose_prior and scene.cam_idx is not None:                         # acinoset_opt.py:916-917
        from . import priors as _priors
        pri = _priors.load_priors(pose=True, motion=False)
    opts = options if options is not None else abi.default_options(scene.fps)
    if params.hand_labeled_data:
        opts.loss_a, opts.loss_b, opts.loss_c = 1e6, 2e6, 3e6          # squared loss of hand-labelled points (init_trajectory)
    opts.h = 1.0 / scene.fps
    if options is None:
        opts.tol_cost, opts.max_iter = 1e-6, 1500          # the physics term is stiff: see DESIGN.md 2b (the reference stops IPOPT at Tol = 1e-3; a monocular start with a missed contact window has taken 1 200 iterations)
    ko = kinetic_options if kinetic_options is not None else abi.default_kinetic_options(skeleton.dyn_options(est.name, **_length_kw(est)), scene.fps, params.kinetic_dataset)
    if not no_slip and not joint_estimation:
        ko.slip_max = 0.0                                                            # `no_slip` guards the rules of the prescribed-force branch only (acinoset_opt.py:855-866);
        ko.zvel_max = 0.0                                                            # the joint-estimation branch always has them (:803-810)
    if not joint_estimation and not ground_constraint:
        ko.foot_height_tol = 1e9                                                     # the feet are not tied to the ground (:832)
    q_target = None
    if not use_2d_reprojections:                                                     # the 3D kinematic cost (acinoset_opt.py:911-913): the target is
        q_target = np.ascontiguousarray(fte["q"][:N], dtype=np.float64)              # init_q, the stored kinematic solution (:739-744)
        tracked_motion_options(ko, scene.fps)
    weighted = q_target is not None and track_weights == "posterior"
    cov_u = load_posterior_blocks(kin_path, N) if weighted else None
    if disable_motion_prior:
        ko.w_torque, ko.w_smooth = 0.0, 0.0                                          # acinoset_opt.py:918-920
    if est.bound_eom_error is not None:
        ko.slack_lo, ko.slack_hi = float(est.bound_eom_error[0]), float(est.bound_eom_error[1])      # make_pyomo_model(bound_eom_error=...), acinoset_opt.py:510-514
    skk = skeleton.without_motion_model(sk)              # the physics-based cost has no constant-acceleration term (acinoset_opt.py:905-921)
    variant = "fixed" if grf_fixed is not None else ("force_box" if grf_box is not None else "free")
    return dict(q_init=q_init, stance=stance, grf_fixed=grf_fixed, grf_box=grf_box, pri=pri, opts=opts, ko=ko, skeleton=skk, N=N, variant=variant,
                q_target=q_target, tracked=q_target is not None, weighted=weighted, cov_u=cov_u, track_scale=float(track_scale))


def _kinetic_finish(est: CheetahEstimator, h, res: dict, seconds: float, prep: dict, solver_output: bool, out_fname: str,
                    out_dir_prefix: Optional[str], uncertainty: Optional[KineticUncertainty] = None, no_factor: Optional[list] = None) -> bool:
    """what estimate_kinetics does after the solver call: centre of mass, costs, `ok`, files.  `res` holds ONE sequence; h: a handle of its model.
    uncertainty: what _kinetic_uncertainty returned, or None (not asked for); stored after the solve's own files (_store_kinetic_uncertainty, which
    no_factor goes to)."""
    params, scene = est.params, est.scene
    q_init, stance, ko = prep["q_init"], prep["stance"], prep["ko"]
    est.opt_time_s = seconds
    _store_com(est, h, res["q"])
    st, ks = res["stats"][0], res["kstats"][0]
    est.result = res
    est.kinetic = dict(tau=res["tau"][0], lam=res["lam"][0], grf=res["grf"][0], slack=res["slack"][0], stance=stance, ground_height=ko.ground_height)
    est.costs = {"measurement": st.cost_meas, "pose": st.cost_pose, "energy": ks.cost_energy, "eom_error": ks.cost_eom, "torque": ks.cost_torque}
    if prep.get("tracked"):                                                          # measurement = the kinematic cost, energy = 1e-2 torque (acinoset_opt.py:912-913)
        est.costs["energy"] = 1e-2 * ks.cost_torque
    base_err = float(np.sqrt(np.mean((q_init[:, :6] - res["q"][0][:, :6]) ** 2)))
    rel_err = float(np.sqrt(np.mean((q_init[:, 6:] - res["q"][0][:, 6:]) ** 2)))
    if solver_output:
        print(f"Total cost: {st.cost}\n-- measurement: {st.cost_meas}\n-- pose: {st.cost_pose}\n-- energy: {ks.cost_energy}\n-- eom_error: {ks.cost_eom}\n"
              f"-- torque: {ks.cost_torque}\nstatus {st.status}, {st.iterations} LM iterations, {st.outer} multiplier updates, {est.opt_time_s:.3f} s\n"
              f"max |slack_eom| {ks.max_slack:.3e} (box [{ko.slack_lo}, {ko.slack_hi}]), max |rows 0-2| / Mg {ks.max_base_rows:.3e}, max violated inequality {ks.max_violation:.3e}\n"
              f"RMSE base: {base_err:.4f}\nRMSE links: {rel_err:.4f}")
    ok = st.status == abi.OK and bool((res["slack"][0] >= ko.slack_lo - 1e-4).all() and (res["slack"][0] <= ko.slack_hi + 1e-4).all())
    out_dir = None
    if scene.cam_idx is not None or ok:                                              # acinoset_opt.py:948-954
        dname = f"fte_kinetic{'_gt' if params.hand_labeled_data else ''}"
        dname = dname if scene.cam_idx is None else f"{dname}_{scene.cam_idx}"
        out_dir = est.save(dname, fname=out_fname, out_dir_prefix=out_dir_prefix)
    _store_kinetic_uncertainty(est, uncertainty, ok, out_dir, no_factor, h)
    return ok


def _kinetic_solve(h, preps, ests, of=None) -> dict:
    """THE solver call of estimate_kinetics and estimate_kinetics_batch, in the mode the sequences were prepared for: 2D reprojections, the 3D
    kinematic cost (tracked) or its full-weight form (weighted: one cpe_track_precision call first).  preps / ests: the _kinetic_prepare dict
    and the estimator of every sequence, all of one mode and variant.  of = None: a plain batch on a handle of their one model (one length; the
    arrays are stacked to [B, N, ...]).  of = the model index of every sequence on a Handle.multi: a ragged batch (lists of per-sequence arrays;
    the kinetic options of model k are those of its first sequence).  Returns the result of the *_host / *_ragged_host method."""
    p0 = preps[0]
    gather = lambda v: _gather(v, of is not None)
    a = {k: gather([p[k] for p in preps]) for k in ("q_init", "q_target", "stance", "cov_u", "grf_fixed", "grf_box")}
    meas, weight = gather([e.meas for e in ests]), gather([e.weight for e in ests])
    ko, (form, kw) = _kinetic_options_of(preps, of), ("_host", {}) if of is None else ("_ragged_host", dict(model_list=of))
    force = dict(grf_fixed=a["grf_fixed"], grf_box=a["grf_box"])
    if p0["weighted"]:
        W = h.track_precision_host(a["cov_u"], p0["track_scale"], **kw)
        return getattr(h, "solve_kinetic_tracked_weighted" + form)(ko, W, a["q_init"], a["q_target"], a["stance"], meas, weight, **kw, **force)
    if p0["tracked"]:
        return getattr(h, "solve_kinetic_tracked" + form)(ko, a["q_init"], a["q_target"], a["stance"], meas, weight, **kw, **force)
    return getattr(h, "solve_kinetic" + form)(ko, a["q_init"], meas, weight, a["stance"], **kw, **force)


def kinetic_ragged_group_key(sk: abi.Skeleton, opts: abi.Options, ko: abi.KineticOptions, pri: Optional[abi.Priors], variant: str, device: int,
                             tracked: bool = False, track_weights: str = "reference") -> tuple:
    """What sequences must share to go through one cpe_solve_kinetic_ragged call (Handle.multi): the skeleton's shape, the solver options the LM
    driver reads per batch, the kinetic option fields that fix every node's unknowns and rows (_lib.kinetic_shape_signature), the priors, the
    variant (free, prescribed or boxed foot forces), the device and the mode (2D reprojections, or the 3D kinematic cost: tracked = True,
    cpe_solve_kinetic_tracked_ragged; with track_weights = "posterior" its full-weight form, cpe_solve_kinetic_tracked_weighted_ragged).  Rig,
    length, frame rate, masses and the other kinetic options may differ."""
    mode = "2d" if not tracked else ("tracked" if track_weights == "reference" else "tracked-" + track_weights)
    return (_lib.shape_signature(sk), _lib.shared_options_signature(opts), _lib.kinetic_shape_signature(ko), None if pri is None else _struct_bytes(pri),
            variant, device, mode)


def _kinetic_model_bytes(est: CheetahEstimator, prep: dict) -> bytes:
    return _model_bytes(est, prep["opts"]) + _struct_bytes(prep["skeleton"]) + _struct_bytes(prep["ko"])


def estimate_kinetics_batch(estimators: Sequence[CheetahEstimator], init_torques: bool = True, auto: bool = True, use_2d_reprojections: bool = True,
                            solver_output: bool = False, init_prev_kinematic_solution: bool = True, synthesised_grf: bool = False,
                            no_slip: bool = True, joint_estimation: bool = False, fix_grf: bool = True, ground_constraint: bool = False,
                            disable_pose_prior: bool = False, disable_motion_prior: bool = False, plot: bool = False, out_fname: str = "fte",
                            out_dir_prefix: Optional[str] = None, options: Optional[abi.Options] = None,
                            kinetic_options: Optional[abi.KineticOptions] = None, ragged: bool = False, uncertainty: bool = False,
                            uncertainty_ridge: float = 0.0, uncertainty_rates: bool = False, uncertainty_spans=None,
                            track_weights: str = "reference", track_scale: float = 1.0, uncertainty_samples: int = 0,
                            uncertainty_seed: int = 0) -> List[bool]:
    """estimate_kinetics for MANY sequences at once, with its keyword arguments (applied to every sequence).  Each sequence is prepared as
    estimate_kinetics prepares it (the per-frame force fit of the fix_grf=True, synthesised_grf=False branch included, one sequence at a time),
    then solved in a batch, then gets its centre of mass, costs and files exactly as estimate_kinetics writes them; only processing_time_s (its
    share of the batched solve) differs.  All estimators must live on the same device.  Returns one bool per estimator, in order.
    ragged=False: sequences with the same skeleton, rig, length, options, kinetic options, priors, variant and device share ONE solve_kinetic_host
    call.  ragged=True: they need only share kinetic_ragged_group_key; each group is ONE cpe_solve_kinetic_ragged call over a Handle.multi of its
    distinct (skeleton, rig, options, kinetic options) models, whatever the lengths.  Every sequence's results are bit-equal either way.
    uncertainty=True: as in estimate_kinetics, from ONE covariance call per group on the group's handle over its converged sequences
    (covariance_kinetic_host; ragged: covariance_kinetic_ragged_host); every sequence's est.uncertainty and uncertainty.npz are bit-equal to those of
    its own estimate_kinetics call.  A sequence without a factor does not stop the batch: every sequence is finished and stored first, then ONE
    CpeError names all of them.  uncertainty_rates=True: as in estimate_kinetics, one rate call after each covariance call, same bit-equality.
    uncertainty_spans: as in estimate_kinetics, resolved for every sequence; one cpe_covariance_columns call per group, same bit-equality.
    uncertainty_samples, uncertainty_seed: as in estimate_kinetics, every sequence with the z and zeta of its own call; one cpe_band_sample, one
    cpe_posterior_samples and one cpe_force_samples (ragged: cpe_force_samples_ragged) call per group, same bit-equality of est.samples and
    samples.npz.
    track_weights / track_scale: as in estimate_kinetics; "posterior" makes ONE cpe_track_precision call per group on the group's handle."""
    req = posterior_request(uncertainty, uncertainty_ridge, uncertainty_rates, uncertainty_spans, uncertainty_samples, uncertainty_seed)
    _check_track_weights(track_weights, track_scale, use_2d_reprojections)
    _check_tracked_uncertainty(req, use_2d_reprojections)
    ests = list(estimators)
    spans = _spans_of(req, ests)
    out: List[Optional[bool]] = [None] * len(ests)
    groups: Dict[tuple, List[int]] = {}
    prepared = {}
    for i, est in enumerate(ests):
        p = _kinetic_prepare(est, auto, use_2d_reprojections, init_prev_kinematic_solution, synthesised_grf, no_slip, joint_estimation, fix_grf,
                             ground_constraint, disable_pose_prior, disable_motion_prior, out_dir_prefix,
                             None if options is None else _struct_copy(options), None if kinetic_options is None else _struct_copy(kinetic_options),
                             track_weights=track_weights, track_scale=track_scale)
        prepared[i] = p
        if ragged:
            key = kinetic_ragged_group_key(p["skeleton"], p["opts"], p["ko"], p["pri"], p["variant"], est.device, tracked=p["tracked"],
                                           track_weights=track_weights)
        else:
            key = (_kinetic_model_bytes(est, p), p["N"], None if p["pri"] is None else _struct_bytes(p["pri"]), p["variant"], est.device, p["tracked"],
                   p["weighted"])
        groups.setdefault(key, []).append(i)
    if req is not None:                              # what is refused, before anything is solved
        for idx in groups.values():
            _lib.covariance_supported(prepared[idx[0]]["pri"], req.ridge)
    no_factor: List[CheetahEstimator] = []
    for idx in groups.values():
        _solve_kinetic_group(ests, idx, prepared, out, ragged, req, spans, (solver_output, out_fname, out_dir_prefix), no_factor)
    if no_factor:
        raise _lib.CpeError(_no_factor_reason(req.ridge, [f"{e.name} {e.data_path}" for e in no_factor]))
    return [bool(v) for v in out]


def _solve_kinetic_group(ests, idx, prepared, out, ragged: bool, req: Optional[PosteriorRequest], spans: Optional[list], finish: tuple,
                         no_factor: Optional[list] = None) -> None:
    """estimate_kinetics (the group of one) and estimate_kinetics_batch for one group, plain (one model and length: ONE solve call with B = the
    group's size) or ragged (one model per distinct (skeleton, rig, options, kinetic options): ONE ragged solve call): _kinetic_solve, with req
    ONE posterior chain on the same handle over the converged sequences (_batch_kinetic_uncertainty), then every sequence's centre of mass,
    costs and files through _kinetic_finish(..., *finish, its uncertainty, no_factor).  spans: the resolved spans of ALL estimators, or None."""
    seqs, preps = [ests[i] for i in idx], [prepared[i] for i in idx]
    hs = _GroupHandles([(p["skeleton"], e.cams, p["opts"]) for e, p in zip(seqs, preps)], preps[0]["pri"], seqs[0].device,
                       [_kinetic_model_bytes(e, p) for e, p in zip(seqs, preps)] if ragged else None)
    try:
        t0 = time()
        res = _kinetic_solve(hs.solve, preps, seqs, hs.of)
        dt = (time() - t0) / len(idx)                                                # processing_time_s of a sequence: its share of the batched solve
        unc = _batch_kinetic_uncertainty(hs.solve, req, None if spans is None else [spans[i] for i in idx], res, preps, [e.meas for e in seqs],
                                         [e.weight for e in seqs], hs.of)
        for b, i in enumerate(idx):
            out[i] = _kinetic_finish(ests[i], hs.fk(b), _sequence_of(res, b), dt, preps[b], *finish, unc.get(b), no_factor)
    finally:
        hs.close()


def bound_value(val, slack_percentage: float) -> np.ndarray:
    """`misc.bound_value` (acinoset_misc.py:84-90), vectorised: [..., 2] = (lower, upper) -- within `slack_percentage` of the value on its own
    side of zero, (-slack, +slack) for a value of exactly zero"""
    v = np.asarray(val, dtype=np.float64)
    lo = np.where(v > 0, (1 - slack_percentage) * v, np.where(v < 0, (1 + slack_percentage) * v, -slack_percentage))
    hi = np.where(v > 0, (1 + slack_percentage) * v, np.where(v < 0, (1 - slack_percentage) * v, slack_percentage))
    return np.stack([lo, hi], axis=-1)


def estimate_grf(estimator: CheetahEstimator, solver_output: bool = True, out_dir_prefix: Optional[str] = None,
                 options: Optional[abi.Options] = None, kinetic_options: Optional[abi.KineticOptions] = None, uncertainty: bool = False,
                 uncertainty_ridge: float = 0.0, uncertainty_rates: bool = False, uncertainty_spans=None, uncertainty_samples: int = 0,
                 uncertainty_seed: int = 0) -> bool:
    """Same signature and meaning as the module-level acinoset_opt.estimate_grf (acinoset_opt.py:966-1048), the last stage of the kinetic-dataset
    pipeline (run_dataset.py:1125-1138): the physics-based model is solved again from the stored `fte_kinetic/fte.pickle` -- trajectory as the
    starting point, every torque within 10 % of its stored value (`Tc.bounds = bound_value(init_tau, 0.1)`, :995-1003) -- with the ground-reaction
    forces FREE where the measured force plates saw the foot on the ground and zero elsewhere (:1005-1017), the feet within 3 cm of the ground
    during those contacts, no pose prior, cost = measurement + torque + 0.1 fps^-2 smoothing + 10e3 slack (:1019-1026).  Runs on the GPU
    (cpe_solve_kinetic_bounded); writes `fte_grf/`.
    Contact pattern: the reference takes the non-zero entries of `get_grf_profile(..., synthetic_data=False)`, i.e. the frames of each foot's FIRST
    window in `metadata.json` (frames 0 .. N-2) at which the resampled plate signal is non-zero; with a per-frame CSV twin `grf/data.csv` of that
    table (the reference ships `grf/data.h5` at 3.5 kHz, which needs PyTables and a resampling step that are not reproduced here) the same rule is
    applied to it, otherwise the window alone decides (a loaded plate never reads exactly zero).
    uncertainty=True: as in estimate_kinetics, with the torque boxes of this solve; uncertainty.npz goes beside fte_grf/fte.pickle.
    uncertainty_rates=True (with uncertainty=True): the rate fields of estimate_kinematics (RATE_FIELDS), from that covariance.
    uncertainty_spans (with uncertainty=True): the span fields of estimate_kinematics (SPAN_FIELDS), from that covariance.
    uncertainty_samples, uncertainty_seed (with uncertainty=True): as in estimate_kinetics (KINETIC_SAMPLE_FIELDS), with the torque boxes of this
    solve; samples.npz goes beside uncertainty.npz."""
    req = posterior_request(uncertainty, uncertainty_ridge, uncertainty_rates, uncertainty_spans, uncertainty_samples, uncertainty_seed)
    est, params, scene, sk = estimator, estimator.params, estimator.scene, estimator.skeleton
    spans = None if req is None else req.spans_for(params.end_frame - params.start_frame)
    assert params.kinetic_dataset, "Cannot determine GRF on a dataset other than the kinetic dataset from Penny Hudson and Co."
    if est.kinematic_model:
        raise AssertionError("Dynamic model of the cheetah is required.")
    data_dir = params.data_dir if out_dir_prefix is None else os.path.join(out_dir_prefix, est.data_path)
    fte = load_result_pickle(os.path.join(data_dir, "fte_kinetic", "fte.pickle"))
    N = params.end_frame - params.start_frame
    q_init = np.ascontiguousarray(fte["q"][:N], dtype=np.float64)
    groups = skeleton.motor_groups()
    nm = sum(len(cols) for _, cols in groups)
    init_tau = np.zeros((N, nm))
    for name, cols in groups:                                                       # {motor name: [N, components]} as save() and the reference write it
        init_tau[:, cols] = np.asarray(fte["tau"][name], dtype=np.float64)[:N]
    tau_box = bound_value(init_tau, 0.1)
    with open(os.path.join(params.data_dir, "metadata.json"), "r", encoding="utf-8") as fh:
        contact_json = json.load(fh)
    direction = 1.0 if float(np.mean(np.asarray(fte["com_vel"]), axis=0)[0]) < 0 else -1.0
    plates = load_measured_plates(os.path.join(params.data_dir, "grf"), direction, 1.0 / est.scale_forces_by)
    if plates is not None:
        gz, _ = grf_profile(plates, contact_json, N, absolute_rows=True)                # measured plates: row = absolute frame
        stance = (gz != 0).astype(np.int32)
    else:
        stance = np.zeros((N, len(skeleton.FEET)), np.int32)
        for k, foot in enumerate(skeleton.FEET):
            rec = contact_json["contacts"].get(f"{foot}_foot")
            if rec:
                a, b = int(rec[0][0]) - contact_json["start_frame"], int(rec[0][1]) - contact_json["start_frame"]
                stance[max(a, 0):max(min(b + 1, N - 1), 0), k] = 1                   # first window only, frames 0 .. N-2 (acinoset_misc.py:954, :1003)
    opts = options if options is not None else abi.default_options(scene.fps)
    if params.hand_labeled_data:
        opts.loss_a, opts.loss_b, opts.loss_c = 1e6, 2e6, 3e6          # squared loss of hand-labelled points (init_trajectory)
    opts.h = 1.0 / scene.fps
    if options is None:
        opts.tol_cost, opts.max_iter = 1e-6, 1500
    ko = kinetic_options if kinetic_options is not None else abi.default_kinetic_options(skeleton.dyn_options(est.name, **_length_kw(est)), scene.fps, True)
    if kinetic_options is None:
        ko.foot_height_tol = 0.03                                                    # foot_height in [-0.03, 0.03] during a contact (:1010-1012)
        ko.slip_max = 0.0                                                            # this NLP has no no-slip rule (estimate_kinetics adds it to ITS model)
        ko.zvel_max = 0.0                                                            # ... and no `foot_z_vel <= 1` rule either (acinoset_opt.py:1004-1017)
    if est.bound_eom_error is not None:
        ko.slack_lo, ko.slack_hi = float(est.bound_eom_error[0]), float(est.bound_eom_error[1])      # make_pyomo_model(bound_eom_error=...), acinoset_opt.py:510-514
    skk = skeleton.without_motion_model(sk)
    if req is not None:
        _lib.covariance_supported(None, req.ridge)                         # raises with the library's reason (negative or non-finite ridge)
    h = _lib.Handle(skk, est.cams, opts, None, device=est.device)
    unc = None
    try:
        t0 = time()
        res = h.solve_kinetic_host(ko, q_init[None], est.meas[None], est.weight[None], stance[None], tau_box=tau_box[None])
        est.opt_time_s = time() - t0
        if req is not None:
            unc = _kinetic_uncertainty(h, ko, res, est.meas, est.weight, stance, req, spans, tau_box=tau_box)
            unc.samples = _complete_samples(est, h, unc.samples)
        _store_com(est, h, res["q"])
    finally:
        h.close()
    st, ks = res["stats"][0], res["kstats"][0]
    est.result = res
    est.kinetic = dict(tau=res["tau"][0], lam=res["lam"][0], grf=res["grf"][0], slack=res["slack"][0], stance=stance, ground_height=ko.ground_height,
                       tau_box=tau_box)
    est.costs = {"measurement": st.cost_meas, "energy": ks.cost_energy, "eom_error": ks.cost_eom, "torque": ks.cost_torque}
    base_err = float(np.sqrt(np.mean((q_init[:, :6] - res["q"][0][:, :6]) ** 2)))
    rel_err = float(np.sqrt(np.mean((q_init[:, 6:] - res["q"][0][:, 6:]) ** 2)))
    if solver_output:
        print(f"Total cost: {st.cost}\n-- measurement: {st.cost_meas}\n-- energy: {ks.cost_energy}\n-- eom_error: {ks.cost_eom}\n-- torque: {ks.cost_torque}\n"
              f"status {st.status}, {st.iterations} LM iterations, {st.outer} multiplier updates, {est.opt_time_s:.3f} s\n"
              f"max |slack_eom| {ks.max_slack:.3e} (box [{ko.slack_lo}, {ko.slack_hi}]), max violated inequality {ks.max_violation:.3e}\n"
              f"RMSE base: {base_err:.4f}\nRMSE links: {rel_err:.4f}")
    ok = st.status == abi.OK and bool((res["slack"][0] >= ko.slack_lo - 1e-4).all() and (res["slack"][0] <= ko.slack_hi + 1e-4).all())
    out_dir = None
    if ok:
        out_dir = est.save("fte_grf", fname="fte", out_dir_prefix=out_dir_prefix)    # acinoset_opt.py:1045-1046
    _store_kinetic_uncertainty(est, unc, ok, out_dir)
    return ok
