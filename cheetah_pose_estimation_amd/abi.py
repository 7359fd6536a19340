"""ctypes mirror of include/cpe.h (the C ABI).  Pure data definitions: no compute lives here."""
import ctypes as C

MAX_LINKS = 20
MAX_MARKERS = 32
MAX_CAMS = 18
MAX_JOINTS = 16
MAX_BOUNDS = 32
MAX_NQ = 3 + 3 * MAX_LINKS
MAX_GMM = 8
NX = 28
MAX_WINDOW = 6

OK, MAX_ITER, NUMERICAL, BAD_ARG, NO_DEVICE, HIP_ERROR = 0, 1, 2, -1, -2, -3
JOINT_REVOLUTE_Y, JOINT_HOOKE_YZ = 0, 1
CAM_FISHEYE, CAM_PINHOLE = 0, 1

d3 = C.c_double * 3


class Skeleton(C.Structure):
    _fields_ = [
        ("n_links", C.c_int32), ("n_markers", C.c_int32), ("n_joints", C.c_int32), ("n_bounds", C.c_int32),
        ("parent", C.c_int32 * MAX_LINKS),
        ("attach", d3 * MAX_LINKS),
        ("com", d3 * MAX_LINKS),
        ("mass", C.c_double * MAX_LINKS),
        ("marker_link", C.c_int32 * MAX_MARKERS),
        ("marker_off", d3 * MAX_MARKERS),
        ("joint_parent", C.c_int32 * MAX_JOINTS),
        ("joint_child", C.c_int32 * MAX_JOINTS),
        ("joint_kind", C.c_int32 * MAX_JOINTS),
        ("bound_a", C.c_int32 * MAX_BOUNDS),
        ("bound_b", C.c_int32 * MAX_BOUNDS),
        ("bound_lo", C.c_double * MAX_BOUNDS),
        ("bound_up", C.c_double * MAX_BOUNDS),
        ("motion_w", C.c_double * MAX_NQ),
        ("rel_ref", C.c_int32 * MAX_NQ),
        ("rel_sign", C.c_double * MAX_NQ),
    ]

    @property
    def nq(self):
        return 3 + 3 * self.n_links


class Camera(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("_pad", C.c_int32),
        ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("D", C.c_double * 4), ("R", C.c_double * 9), ("t", C.c_double * 3), ("mult", C.c_double),
    ]


class Priors(C.Structure):
    _fields_ = [
        ("gmm_k", C.c_int32), ("gmm_dim", C.c_int32),
        ("gmm_logw", C.c_double * MAX_GMM),
        ("gmm_mu", (C.c_double * NX) * MAX_GMM),
        ("gmm_P", ((C.c_double * NX) * NX) * MAX_GMM),
        ("lr_window", C.c_int32), ("_pad", C.c_int32),
        ("lr_coef", (C.c_double * (MAX_WINDOW * NX)) * NX),
        ("lr_b", C.c_double * NX),
        ("lr_w", C.c_double * NX),
    ]


class Options(C.Structure):
    _fields_ = [
        ("h", C.c_double), ("loss_a", C.c_double), ("loss_b", C.c_double), ("loss_c", C.c_double),
        ("cost_scale", C.c_double), ("bound_penalty", C.c_double), ("bound_tol", C.c_double), ("lambda0", C.c_double),
        ("tol_step", C.c_double), ("tol_cost", C.c_double),
        ("max_iter", C.c_int32), ("curvature", C.c_int32), ("max_outer", C.c_int32), ("_pad", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("iterations", C.c_int32),
        ("cost", C.c_double), ("cost_meas", C.c_double), ("cost_model", C.c_double),
        ("cost_pose", C.c_double), ("cost_motion", C.c_double),
        ("lam", C.c_double), ("max_constraint", C.c_double), ("max_bound_violation", C.c_double),
        ("outer", C.c_int32), ("_pad", C.c_int32),
    ]


class GrfOptions(C.Structure):
    """mirror of cpe_grf_options (include/cpe.h)"""
    _fields_ = [
        ("root_inertia", C.c_double * 3), ("friction_ratio", C.c_double), ("force_max", C.c_double),
        ("regularisation", C.c_double), ("gravity", C.c_double),
        ("n_feet", C.c_int32), ("foot_marker", C.c_int32 * 4), ("iterations", C.c_int32),
    ]


class EomOptions(C.Structure):
    """mirror of cpe_eom_options (include/cpe.h)"""
    _fields_ = [("gravity", C.c_double), ("link_inertia", d3 * MAX_LINKS)]


class DynOptions(C.Structure):
    """mirror of cpe_dyn_options (include/cpe.h)"""
    _fields_ = [("eom", EomOptions), ("n_feet", C.c_int32), ("n_motors", C.c_int32), ("foot_marker", C.c_int32 * 4),
                ("motor_first", C.c_int32 * 32), ("motor_second", C.c_int32 * 32), ("motor_axis", C.c_int32 * 32)]


class KineticOptions(C.Structure):
    """mirror of cpe_kinetic_options (include/cpe.h): the physics-based trajectory model of estimate_kinetics"""
    _fields_ = [("dyn", DynOptions), ("w_slack", C.c_double), ("w_torque", C.c_double), ("w_smooth", C.c_double), ("friction", C.c_double),
                ("force_max", C.c_double), ("grfz_min", C.c_double), ("foot_height_tol", C.c_double), ("foot_height_min", C.c_double),
                ("ground_height", C.c_double), ("slip_max", C.c_double), ("zvel_max", C.c_double), ("slack_lo", C.c_double), ("slack_hi", C.c_double),
                ("reg_force", C.c_double), ("kappa_force", C.c_double), ("kappa_height", C.c_double), ("kappa_slip", C.c_double), ("kappa_slack", C.c_double),

                ("lm_force_damping", C.c_double), ("lm_wall_damping", C.c_double), ("inner_iterations", C.c_int32), ("_pad", C.c_int32)]


class KineticStats(C.Structure):
    """mirror of cpe_kinetic_stats (include/cpe.h)"""
    _fields_ = [("cost_torque", C.c_double), ("cost_energy", C.c_double), ("cost_eom", C.c_double), ("max_slack", C.c_double),
                ("max_base_rows", C.c_double), ("max_violation", C.c_double), ("inner_max", C.c_int32), ("_pad", C.c_int32)]


def default_kinetic_options(dyn: DynOptions, fps: float = 120.0, kinetic_dataset: bool = False) -> KineticOptions:
    """the reference's values (acinoset_opt.py:494-506, :780, :905-921; acinoset_misc.py:1140-1167; run_dataset.py:984); same numbers as
    cpe_default_kinetic_options() in csrc/cpe_api.hip"""
    o = KineticOptions()
    C.memmove(C.byref(o.dyn), C.byref(dyn), C.sizeof(DynOptions))
    o.w_slack, o.w_torque, o.w_smooth = 10e3, 1.0, 0.1 / (fps * fps)
    o.friction, o.force_max, o.grfz_min = 0.8, 5.0, 0.01
    o.foot_height_tol = 0.03 if kinetic_dataset else 0.1
    o.foot_height_min, o.ground_height, o.slip_max = 0.0, 0.0, 1.0
    o.zvel_max = 1.0 if kinetic_dataset else 0.0       # `foot_z_vel <= 1` is a rule of the kinetic dataset only (acinoset_opt.py:807-810)
    o.slack_lo, o.slack_hi = -2.0, 2.0                 # bound_eom_error of run_dataset.py:984
    o.reg_force, o.kappa_force, o.kappa_height, o.kappa_slip, o.kappa_slack = 1e-4, 1e5, 1e6, 1e2, 1e6
    o.lm_force_damping, o.lm_wall_damping = 10.0, 10.0
    o.inner_iterations = 30
    return o


def default_track_weights():
    """the weights of the 3D kinematic cost on x (NX entries, link order; acinoset_misc.py:531-589 restated: base x, y, z 10, base angles 5,
    bodyF / neck / tails theta and psi 5 / 2 / 5, leg pitches upper 5, lower 2, hock 1, every roll 0); same numbers as
    cpe_default_track_weights() in csrc/cpe_api.hip"""
    import numpy as np
    return np.array([10, 10, 10, 5, 5, 5, 0, 5, 5, 0, 2, 2, 5, 5, 5, 5, 5, 2, 1, 5, 2, 1, 5, 2, 5, 2, 1, 1], dtype=np.float64)


def default_options(fps: float = 120.0) -> Options:
    """Same defaults as cpe_default_options() in csrc/cpe_api.cpp."""
    o = Options()
    o.h = 1.0 / fps
    o.loss_a, o.loss_b, o.loss_c = 3.0, 10.0, 20.0   # acinoset_misc.py:479-481
    o.cost_scale = 1e-3                              # acinoset_opt.py:602
    o.bound_penalty = 1e4
    o.bound_tol = 1e-6
    o.max_outer = 8
    o.lambda0 = 1e-4
    o.tol_step = 1e-8
    o.tol_cost = 1e-9
    o.max_iter = 200
    o.curvature = 0
    return o


# ---- argument lists of every entry point of include/cpe.h, mirrored for _lib.load() (tests/test_covariance_host.py holds them against the
# header's prototypes).  "h" handle, "i" int32, "d" double, "p" pointer to double (or to int32 on the device, or a stream), "ip" / "dp" / "lp"
# pointer to int32 / double / int64 (host), "hp" pointer to a handle, and a pointer to a struct: "sk" Skeleton, "cam" Camera, "op" Options, "pr"
# Priors, "st" Stats, "go" GrfOptions, "eo" EomOptions, "do" DynOptions, "ko" KineticOptions, "ks" KineticStats
_BN = ("h", "i", "i")                      # handle, B, N
_RAGGED = ("ip", "ip")                     # model, n_frames
_SOLVE = ("p",) * 8                        # q_init, meas, weight | q, dq, ddq, positions, meas_err
_KIN_BN = ("h", "ko", "i", "i")            # handle, kinetic options, B, N
_KIN_IN = ("p",) * 4                       # q_init, meas, weight, stance
_KIN_FORCES = ("p",) * 3                   # grf_fixed, tau_box, grf_box
_KIN_OUT = ("p",) * 9 + ("st", "ks")       # q, dq, ddq, positions, meas_err, tau, lambda, grf, slack | stats, kstats
_TRACKED_BN = ("h", "ko", "p", "i", "i")   # handle, kinetic options, track_w, B, N
_TRACKED_IN = ("p",) * 5                   # q_init, q_target, meas, weight, stance
_COV = ("p", "p", "p", "d", "p", "p", "p", "p", "ip")      # q, meas, weight | ridge | cov_diag, cov_off, cov_pos, L | status
COVARIANCE_ENTRIES = {
    "cpe_covariance_supported": ("pr", "d"),
    "cpe_band_inverse": _BN + ("p", "p", "p"),
    "cpe_covariance": _BN + _COV,
    "cpe_covariance_host": _BN + _COV,
    "cpe_covariance_ragged": _BN + _RAGGED + _COV,
    "cpe_covariance_ragged_host": _BN + _RAGGED + _COV,
}
# the physics-based twin (cpe_covariance_kinetic): h, ko, B, N | q, meas, weight, stance, grf_fixed, tau_box, grf_box | ridge | cov_diag, cov_off,
# cov_pos, cov_f, f, meta, L | status
_KIN_COV = ("p",) * 7 + ("d",) + ("p",) * 7 + ("ip",)
KINETIC_COVARIANCE_ENTRIES = {
    "cpe_covariance_kinetic": _KIN_BN + _KIN_COV,
    "cpe_covariance_kinetic_host": _KIN_BN + _KIN_COV,
}
# its ragged pair: ko an array of one KineticOptions per model, N = N_max, then model, n_frames
KINETIC_COVARIANCE_RAGGED_ENTRIES = {
    "cpe_covariance_kinetic_ragged": _KIN_BN + _RAGGED + _KIN_COV,
    "cpe_covariance_kinetic_ragged_host": _KIN_BN + _RAGGED + _KIN_COV,
}
# the rates (cpe_rate_covariance): h, B, N (| model, n_frames) | q, cov_diag, cov_off | cov_du, cov_ddu, cov_vel, cov_com, cov_com_vel, jac_pos, jac_com
_RATE_COV = ("p",) * 10
RATE_COVARIANCE_ENTRIES = {
    "cpe_rate_covariance": _BN + _RATE_COV,
    "cpe_rate_covariance_host": _BN + _RATE_COV,
    "cpe_rate_covariance_ragged": _BN + _RAGGED + _RATE_COV,
    "cpe_rate_covariance_ragged_host": _BN + _RAGGED + _RATE_COV,
}
RATE_COVARIANCE_OUTPUTS = ("cov_du", "cov_ddu", "cov_vel", "cov_com", "cov_com_vel", "jac_pos", "jac_com")      # in the order of the arguments
# the columns beyond the band (cpe_covariance_columns): h, B, N | n_frames | L, cov_diag, cov_off | K, anchors | cols
_COLUMNS = _BN + ("ip", "p", "p", "p", "i", "ip", "p")
COLUMN_COVARIANCE_ENTRIES = ("cpe_covariance_columns", "cpe_covariance_columns_host")
# draws from the posterior (cpe_band_sample: h, B, N | n_frames | L | S | z | du; cpe_posterior_samples: h, B, N | model, n_frames | q | S | du |
# q_s, positions_s)
_BAND_SAMPLE = _BN + ("ip", "p", "i", "p", "p")
_POSTERIOR_SAMPLES = _BN + _RAGGED + ("p", "i", "p", "p", "p")
SAMPLE_ENTRIES = {
    "cpe_band_sample": _BAND_SAMPLE,
    "cpe_band_sample_host": _BAND_SAMPLE,
    "cpe_posterior_samples": _POSTERIOR_SAMPLES,
    "cpe_posterior_samples_host": _POSTERIOR_SAMPLES,
}
# draws of the node forces (cpe_force_samples): h, ko, B, N (| model, n_frames) | q, meas, weight, stance, grf_fixed, tau_box, grf_box | ridge | S |
# du, zeta | f_s, f, meta | status
_FORCE_SAMPLES = ("p",) * 7 + ("d", "i") + ("p",) * 5 + ("ip",)
FORCE_SAMPLE_ENTRIES = {
    "cpe_force_samples": _KIN_BN + _FORCE_SAMPLES,
    "cpe_force_samples_host": _KIN_BN + _FORCE_SAMPLES,
    "cpe_force_samples_ragged": _KIN_BN + _RAGGED + _FORCE_SAMPLES,
    "cpe_force_samples_ragged_host": _KIN_BN + _RAGGED + _FORCE_SAMPLES,
}
# the reduced system of the length calibration (cpe_scale_system): h, B, N | model, n_frames | q, meas, weight | ridge | G | d_attach, d_marker_off
# (host) | A, b, A_red, b_red, cost | status
MAX_SCALES = 16
_SCALE_SYSTEM = _BN + _RAGGED + ("p", "p", "p", "d", "i", "p", "p") + ("p",) * 5 + ("ip",)
SCALE_ENTRIES = {
    "cpe_scale_system": _SCALE_SYSTEM,
    "cpe_scale_system_host": _SCALE_SYSTEM,
}
# the pose covariance marginalised over the scales (cpe_scale_response: cpe_scale_system's inputs | A_red, resp_u, resp_pos | status;
# cpe_covariance_add_scales: h, B, N | n_frames | G | cov_s, resp_u, resp_pos | cov_diag, cov_off, cov_pos | cov_diag_m, cov_off_m, cov_pos_m)
_SCALE_RESPONSE = _BN + _RAGGED + ("p", "p", "p", "d", "i", "p", "p") + ("p",) * 3 + ("ip",)
_ADD_SCALES = _BN + ("ip", "i") + ("p",) * 9
SCALE_RESPONSE_ENTRIES = {
    "cpe_scale_response": _SCALE_RESPONSE,
    "cpe_scale_response_host": _SCALE_RESPONSE,
    "cpe_covariance_add_scales": _ADD_SCALES,
    "cpe_covariance_add_scales_host": _ADD_SCALES,
}
# the detection report (cpe_detection_report): h, B, N | positions, cov_pos | meas, weight, weight_fit | uv, cov_px | uv_loo, cov_loo, d2, leverage
_DETECTION = _BN + ("p",) * 11
DETECTION_ENTRIES = {
    "cpe_detection_report": _DETECTION,
    "cpe_detection_report_host": _DETECTION,
}
DETECTION_OUTPUTS = ("uv", "cov_px", "uv_loo", "cov_loo", "d2", "leverage")        # in the order of the arguments
COVARIANCE_MAX_PB = 4        # largest half-bandwidth (frames) the covariance sweep supports: motion-prior windows 5 and 6 are refused
ENTRIES = {
    "cpe_create": ("sk", "cam", "i", "op", "pr", "i", "hp"),
    "cpe_create_multi": ("i", "sk", "cam", "ip", "op", "pr", "i", "hp"),
    "cpe_destroy": ("h",),
    "cpe_last_error": (),
    "cpe_default_options": ("op",),
    "cpe_stream": ("h",),
    "cpe_synchronize": ("h",),
    "cpe_stream_wait": ("h", "p"),
    "cpe_stream_signal": ("h", "p"),
    "cpe_profile_enable": ("h", "i"),
    "cpe_profile_get": ("h", "dp", "lp"),
    "cpe_jacobian_slots": ("h",),
    "cpe_jacobian_layout": ("h", "ip", "ip"),
    "cpe_num_independent": ("h",),
    "cpe_independent_dofs": ("h", "ip"),
    "cpe_eval_resjac": _BN + ("p",) * 7,                       # q, meas, weight | r, J, eps, cost
    "cpe_eval_resjac_host": _BN + ("p",) * 7,
    "cpe_project_joints": _BN + ("p",),
    "cpe_forward_kinematics": _BN + ("p", "p", "p"),
    "cpe_marker_velocities": _BN + ("p", "p", "p"),
    "cpe_reproject": _BN + ("p", "p"),
    "cpe_triangulate": ("h", "i", "p", "p", "p", "p", "d", "p"),
    # N, n_slots, slot, table, rows, parts, first_row | part_of_marker, inv_sigma, thresh | meas, weight
    "cpe_tensorise_dlc": ("h", "i", "i", "i", "p", "i", "i", "i", "p", "p", "d", "p", "p"),
    "cpe_eval_normal": _BN + ("p",) * 8,                       # q, meas, weight | g, Bm, cost, gam, q_out
    "cpe_solve": _BN + _SOLVE + ("st",),
    "cpe_solve_host": _BN + _SOLVE + ("st",),
    "cpe_solve_ragged": _BN + _RAGGED + _SOLVE + ("st",),
    "cpe_solve_ragged_host": _BN + _RAGGED + _SOLVE + ("st",),
    # q_init, meas, weight | tau_bound, max_rounds, tol_tau | q, dq, ddq, positions, meas_err, tau | stats, rounds
    "cpe_solve_shutter": _BN + ("p", "p", "p", "d", "i", "d") + ("p",) * 6 + ("st", "ip"),
    "cpe_grf_fit": ("h", "go", "i", "i") + ("p",) * 7,          # q, dq, ddq, contact | grfz, grfxy, residual
    "cpe_eom_rows": ("h", "eo", "i", "i") + ("p",) * 4,         # q, dq, ddq | rows
    "cpe_eom_residual": ("h", "do", "i", "i") + ("p",) * 7,     # q, dq, ddq, tau, lambda, grf | residual
    "cpe_default_kinetic_options": ("ko", "d", "i"),
    "cpe_solve_kinetic": _KIN_BN + _KIN_IN + _KIN_OUT,
    "cpe_solve_kinetic_fixed": _KIN_BN + _KIN_IN + ("p",) + _KIN_OUT,
    "cpe_solve_kinetic_bounded": _KIN_BN + _KIN_IN + ("p",) + _KIN_OUT,
    "cpe_solve_kinetic_force_box": _KIN_BN + _KIN_IN + ("p",) + _KIN_OUT,
    "cpe_solve_kinetic_ragged": _KIN_BN + _RAGGED + _KIN_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_ragged_host": _KIN_BN + _RAGGED + _KIN_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_default_track_weights": ("p",),
    "cpe_solve_kinetic_tracked": _TRACKED_BN + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_tracked_host": _TRACKED_BN + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_tracked_ragged": _TRACKED_BN + _RAGGED + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_tracked_ragged_host": _TRACKED_BN + _RAGGED + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_eval_normal_tracked": ("h", "p", "i", "i") + ("p",) * 7,      # track_w | B, N | q, q_target | g, Bm, cost, gam, q_out
    # the full-weight form: track_W [B, N, NX, NX] in track_w's place; cpe_track_precision: B, N | model, n_frames | cov_diag | scale | W
    "cpe_track_precision": _BN + _RAGGED + ("p", "d", "p"),
    "cpe_track_precision_host": _BN + _RAGGED + ("p", "d", "p"),
    "cpe_solve_kinetic_tracked_weighted": _TRACKED_BN + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_tracked_weighted_host": _TRACKED_BN + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_tracked_weighted_ragged": _TRACKED_BN + _RAGGED + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_solve_kinetic_tracked_weighted_ragged_host": _TRACKED_BN + _RAGGED + _TRACKED_IN + _KIN_FORCES + _KIN_OUT,
    "cpe_eval_normal_tracked_weighted": ("h", "p", "i", "i") + ("p",) * 7,
    "cpe_eval_kinetic_nodes": _KIN_BN + _KIN_IN + ("p",) * 7,          # f, stat, g, Huu, Hfu, Hff, meta
    "cpe_eval_kinetic_system": _KIN_BN + _KIN_IN + _KIN_FORCES + ("p",) * 10,     # the same, then gk, Bk, Hk
    "cpe_eval_lm_step": _KIN_BN + _KIN_IN + ("d",) + ("p",) * 6,       # lam | g, dg, L, delta, state, seq
    # q, meas, weight, tau | lam | g, Bm, cost, gx, rcb, g_total, step, meas_err, seq
    "cpe_eval_shutter_step": _BN + ("p",) * 4 + ("d",) + ("p",) * 9,
    "cpe_eval_shutter_step_host": _BN + ("p",) * 4 + ("d",) + ("p",) * 9,
    "cpe_eval_active_list": ("h", "i", "i", "ip", "ip", "ip"),         # B, window | status | act, n_act (host)
    **COVARIANCE_ENTRIES, **KINETIC_COVARIANCE_ENTRIES, **KINETIC_COVARIANCE_RAGGED_ENTRIES, **RATE_COVARIANCE_ENTRIES,
    **{name: _COLUMNS for name in COLUMN_COVARIANCE_ENTRIES}, **SAMPLE_ENTRIES, **FORCE_SAMPLE_ENTRIES,
    **SCALE_ENTRIES, **SCALE_RESPONSE_ENTRIES, **DETECTION_ENTRIES,
}


def argtypes(name: str) -> list:
    """ctypes argument list of an entry point"""
    ptr = C.POINTER
    kinds = {"h": C.c_void_p, "i": C.c_int32, "d": C.c_double, "p": C.c_void_p, "ip": ptr(C.c_int32), "dp": ptr(C.c_double), "lp": ptr(C.c_int64),
             "hp": ptr(C.c_void_p), "sk": ptr(Skeleton), "cam": ptr(Camera), "op": ptr(Options), "pr": ptr(Priors), "st": ptr(Stats),
             "go": ptr(GrfOptions), "eo": ptr(EomOptions), "do": ptr(DynOptions), "ko": ptr(KineticOptions), "ks": ptr(KineticStats)}
    return [kinds[k] for k in ENTRIES[name]]


covariance_argtypes = argtypes
