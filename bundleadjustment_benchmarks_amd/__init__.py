"""Thin ctypes binding of libba_mi355x.so (include/ba_mi355x.h) for the parity tests and bench.py.

The product is the C-ABI library + the Bundle_Adjustment_{QRKit,QRChol,Cholesky,...,IterSchur} executables (csrc/main.c); this
module adds nothing to the data path.  It fails loudly when the HIP library is missing -- there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libba_mi355x.so")

QRKIT, QRCHOL, CHOLESKY, MOREQR, QRSPQR = 0, 1, 2, 3, 4
ITERSCHUR = 5  # no reference counterpart: the reduced camera system by PCG, never formed (include/ba_mi355x.h)
F64, F32 = 0, 1
KIND_NAMES = {QRKIT: "QRKIT", QRCHOL: "QRCHOL", CHOLESKY: "CHOLESKY", MOREQR: "MOREQR", QRSPQR: "QRSPQR", ITERSCHUR: "ITERSCHUR"}
STATUS = {-2: "NotStarted", -1: "Running", 0: "Success", 1: "ExceededLambdaMax", 2: "TooManyFunctionEvaluation",
          3: "MaxItersReached"}

# ba_solver_set_constant: bit q of a camera's mask word = camera parameter q (the camera block of GET_JC / GET_DX / GET_GRAD)
FIX_T, FIX_OMEGA, FIX_POSE, FIX_INTRINSICS, FIX_CAMERA = 0x007, 0x038, 0x03F, 0x1C0, 0x1FF

# ba_solver_set_loss: rho(s) of the weighted squared reprojection error s (include/ba_mi355x.h); a new solver is (LOSS_REFERENCE, 0.5)
LOSS_REFERENCE, LOSS_TRIVIAL, LOSS_HUBER, LOSS_CAUCHY = 0, 1, 2, 3

# ba_solver_set_preconditioner (ITERSCHUR): block Jacobi, or block Jacobi + the cross blocks of a spanning forest of the constraints,
# or + the blocks S_ab of a maximum-weight spanning forest of the co-visibility graph (Problem.covisibility)
PRECOND_BLOCK_JACOBI, PRECOND_CONSTRAINT_FOREST, PRECOND_VISIBILITY_FOREST = 0, 1, 3  # (2 is no kind: refused as before)

# ba_solver_set_damping: lambda I (the reference's, a new solver's) or Marquardt's lambda diag(J'J), clamped (CHOLESKY, ITERSCHUR)
DAMP_IDENTITY, DAMP_MARQUARDT = 0, 1

(GET_RESIDUALS, GET_JC, GET_JP, GET_GRAD, GET_S, GET_RHS, GET_DX, GET_CAMS, GET_POINTS, GET_CAMS_TEST,
 GET_POINTS_TEST) = range(11)

EXPORTS = [
    "ba_status_string", "ba_error_string", "ba_problem_load_bal", "ba_problem_create", "ba_problem_synthetic",
    "ba_problem_save_bal", "ba_problem_free", "ba_problem_dims", "ba_problem_get", "ba_lm_params_default",
    "ba_solver_create", "ba_solver_free", "ba_solver_set_allreduce", "ba_solver_set_stream", "ba_solver_shard",
    "ba_minimize", "ba_solver_linearize", "ba_solver_try_step", "ba_solver_accept", "ba_solver_stats", "ba_solver_get",
    "ba_solver_keep_intermediates", "ba_solver_set_state", "ba_solver_timing", "ba_solver_time_phase", "ba_device_info",
    "ba_version", "ba_shard_plan", "ba_problem_save_cache", "ba_problem_load_cache", "ba_solver_selftest",
    "ba_comm_unique_id", "ba_comm_id_via_file", "ba_comm_id_file_done", "ba_solver_comm_init", "ba_solver_recoveries",
    "ba_solver_set_pcg", "ba_solver_pcg_stats", "ba_solver_device_bytes", "ba_solver_set_constant", "ba_problem_gauge_mask",
    "ba_solver_covariance_compute", "ba_solver_covariance_get", "ba_solver_covariance_timing", "ba_solver_covariance_pcg",
    "ba_solver_set_loss", "ba_solver_set_obs_weights",
    "ba_solver_set_point_priors", "ba_solver_set_centre_priors", "ba_solver_set_intrinsics_priors", "ba_solver_prior_energy",
    "ba_solver_set_relative_poses", "ba_solver_relative_pose_energy",
    "ba_solver_set_preconditioner", "ba_solver_preconditioner_info", "ba_relpose_forest_plan", "ba_problem_covisibility",
    "ba_intrinsics_group_plan", "ba_solver_set_shared_intrinsics", "ba_solver_shared_intrinsics_info",
    "ba_solver_set_damping", "ba_solver_get_damping",
    "ba_solver_set_pcg_model_tol", "ba_solver_pcg_stop_stats",
    "ba_dogleg_coefficients", "ba_solver_dogleg_prepare", "ba_solver_try_dogleg", "ba_dogleg_params_default", "ba_minimize_dogleg",
    "ba_triangulate_params_default", "ba_solver_triangulate_points", "ba_triangulate_point",
    "ba_solver_set_obs_active", "ba_solver_get_obs_active", "ba_filter_params_default", "ba_solver_filter_observations", "ba_filter_track",
]
# ba_triangulate_status (include/ba_mi355x.h)
TRI_REPLACED, TRI_FEW_VIEWS, TRI_LOW_ANGLE, TRI_DEGENERATE, TRI_BEHIND, TRI_REPROJ, TRI_NOT_BETTER, TRI_FIXED = range(8)
TRI_NAMES = ("REPLACED", "FEW_VIEWS", "LOW_ANGLE", "DEGENERATE", "BEHIND", "REPROJ", "NOT_BETTER", "FIXED")
# ba_obs_status, ba_filter_point_status (include/ba_mi355x.h)
OBS_KEPT, OBS_WAS_OFF, OBS_BEHIND, OBS_NONFINITE, OBS_REPROJ, OBS_POINT = range(6)
OBS_NAMES = ("KEPT", "WAS_OFF", "BEHIND", "NONFINITE", "REPROJ", "POINT")
FPT_KEPT, FPT_SHORT, FPT_LOW_ANGLE = range(3)
FPT_NAMES = ("KEPT", "SHORT", "LOW_ANGLE")
ERR_ARG, ERR_NOMEM, ERR_SINGULAR = 4, 6, 8


class LMParams(C.Structure):
    _fields_ = [("lambda_min", C.c_double), ("lambda_max", C.c_double), ("lambda_decrease", C.c_double),
                ("lambda_increase_base", C.c_double), ("lambda_init", C.c_double), ("tol_fun", C.c_double),
                ("max_iter", C.c_int), ("max_fun_ev", C.c_int), ("max_trials", C.c_int), ("verbose", C.c_int)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("trials", C.c_int), ("fun_evals", C.c_int),
                ("energy", C.c_double), ("lambda_", C.c_double), ("seconds", C.c_double), ("schur_ms", C.c_double),
                ("linearize_ms", C.c_double)]


class Timing(C.Structure):
    _fields_ = [("linearize_ms", C.c_double), ("eliminate_ms", C.c_double), ("schur_ms", C.c_double),
                ("factor_ms", C.c_double), ("backsub_ms", C.c_double), ("test_eval_ms", C.c_double),
                ("comm_ms", C.c_double), ("trial_ms", C.c_double), ("n_linearize", C.c_longlong), ("n_trials", C.c_longlong),
                ("n_graph_trials", C.c_longlong)]


class PCGStats(C.Structure):
    _fields_ = [("solves", C.c_longlong), ("total_iters", C.c_longlong), ("last_iters", C.c_int), ("last_converged", C.c_int),
                ("last_rel_residual", C.c_double)]


class PCGStopStats(C.Structure):
    _fields_ = [("by_residual", C.c_longlong), ("by_model", C.c_longlong), ("at_cap", C.c_longlong), ("last_rule", C.c_int),
                ("last_zeta", C.c_double), ("last_model", C.c_double)]


class CovPCGStats(C.Structure):
    _fields_ = [("columns", C.c_longlong), ("batches", C.c_longlong), ("total_iters", C.c_longlong), ("max_iters", C.c_int),
                ("unconverged", C.c_int), ("worst_rel_residual", C.c_double), ("ms", C.c_double)]


class DoglegInfo(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("mu", "g2", "q", "gn2", "g_dot_gn", "alpha", "energy_gn", "rho_scale_gn")]


class DoglegParams(C.Structure):
    """ba_dogleg_params: the radius is in the units of the step (BA_GET_DX); defaults from ba_dogleg_params_default."""
    _fields_ = [("radius_init", C.c_double), ("radius_min", C.c_double), ("radius_max", C.c_double), ("mu_rel", C.c_double),
                ("mu_rel_max", C.c_double), ("tol_fun", C.c_double), ("max_iter", C.c_int), ("max_fun_ev", C.c_int),
                ("max_trials", C.c_int), ("verbose", C.c_int)]

    @classmethod
    def default(cls):
        p = cls()
        lib().ba_dogleg_params_default(C.byref(p))
        return p


class TriangulateParams(C.Structure):
    _fields_ = [("min_angle_deg", C.c_double), ("max_reproj_px", C.c_double), ("refine_iters", C.c_int), ("only_if_better", C.c_int)]

    @classmethod
    def default(cls):
        p = cls()
        lib().ba_triangulate_params_default(C.byref(p))
        return p


class TriangulateStats(C.Structure):
    _fields_ = [("asked", C.c_longlong), ("by_status", C.c_longlong * 8), ("cost_before", C.c_double), ("cost_after", C.c_double),
                ("ms", C.c_double)]


class FilterParams(C.Structure):
    _fields_ = [("max_reproj_px", C.c_double), ("min_angle_deg", C.c_double), ("min_track", C.c_int), ("require_front", C.c_int)]

    @classmethod
    def default(cls):
        p = cls()
        lib().ba_filter_params_default(C.byref(p))
        return p


class FilterStats(C.Structure):
    _fields_ = [("active_before", C.c_longlong), ("active_after", C.c_longlong), ("by_status", C.c_longlong * 6),
                ("points_short", C.c_longlong), ("points_low_angle", C.c_longlong), ("err_sum_before", C.c_double),
                ("err_sum_after", C.c_double), ("ms", C.c_double)]


def _filter_params(max_reproj_px, min_angle_deg, min_track, require_front):
    fp = FilterParams.default()
    if max_reproj_px is not None:
        fp.max_reproj_px = float(max_reproj_px)
    if min_angle_deg is not None:
        fp.min_angle_deg = float(min_angle_deg)
    if min_track is not None:
        fp.min_track = int(min_track)
    if require_front is not None:
        fp.require_front = int(bool(require_front))
    return fp


def _tri_params(min_angle_deg, max_reproj_px, refine_iters, only_if_better):
    tp = TriangulateParams.default()
    if min_angle_deg is not None:
        tp.min_angle_deg = float(min_angle_deg)
    if max_reproj_px is not None:
        tp.max_reproj_px = float(max_reproj_px)
    if refine_iters is not None:
        tp.refine_iters = int(refine_iters)
    tp.only_if_better = int(bool(only_if_better))
    return tp


TRIAL_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p)


class BAError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        RuntimeError.__init__(self, "%s failed: %s (code %d)" % (where, error_string(code), code))


def build(force=False):
    """Compile the HIP library and the executables for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", src, "all"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `make -C %s` (hipcc, gfx950); there is no CPU fallback"
                              % (LIB_PATH, os.path.join(_HERE, "csrc")))
        L = C.CDLL(LIB_PATH)
        L.ba_status_string.restype = C.c_char_p
        L.ba_error_string.restype = C.c_char_p
        L.ba_version.restype = C.c_char_p
        L.ba_problem_free.restype = None
        L.ba_solver_free.restype = None
        L.ba_lm_params_default.restype = None
        L.ba_problem_free.argtypes = [C.c_void_p]
        L.ba_solver_free.argtypes = [C.c_void_p]
        L.ba_problem_synthetic.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_void_p]
        L.ba_solver_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ba_solver_try_step.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_linearize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_accept.argtypes = [C.c_void_p]
        L.ba_solver_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.ba_solver_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_keep_intermediates.argtypes = [C.c_void_p, C.c_int]
        L.ba_solver_set_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_shard.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.ba_minimize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ba_solver_time_phase.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.ba_solver_selftest.argtypes = [C.c_void_p, C.c_int]
        L.ba_comm_unique_id.argtypes = [C.c_void_p]
        L.ba_comm_id_via_file.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        L.ba_solver_comm_init.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_comm_id_file_done.argtypes = [C.c_char_p, C.c_int]
        L.ba_solver_recoveries.argtypes = [C.c_void_p]
        L.ba_solver_set_pcg.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.ba_solver_pcg_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ba_solver_set_pcg_model_tol.argtypes = [C.c_void_p, C.c_double]
        L.ba_solver_pcg_stop_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.ba_solver_set_damping.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
        L.ba_solver_get_damping.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_dogleg_coefficients.argtypes = [C.c_double] * 6 + [C.c_void_p] * 4
        L.ba_solver_dogleg_prepare.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.ba_solver_try_dogleg.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 4
        L.ba_dogleg_params_default.restype = None
        L.ba_dogleg_params_default.argtypes = [C.c_void_p]
        L.ba_minimize_dogleg.argtypes = [C.c_void_p] * 5
        L.ba_triangulate_params_default.restype = None
        L.ba_triangulate_params_default.argtypes = [C.c_void_p]
        L.ba_solver_triangulate_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.ba_triangulate_point.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_double] + [C.c_void_p] * 7
        L.ba_solver_set_obs_active.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_get_obs_active.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_filter_params_default.restype = None
        L.ba_filter_params_default.argtypes = [C.c_void_p]
        L.ba_solver_filter_observations.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.ba_filter_track.argtypes = [C.c_int] + [C.c_void_p] * 9
        L.ba_solver_device_bytes.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_set_constant.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_problem_gauge_mask.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ba_solver_covariance_compute.argtypes = [C.c_void_p, C.c_double]
        L.ba_solver_covariance_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.ba_solver_covariance_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_covariance_pcg.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        L.ba_solver_set_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.ba_solver_set_obs_weights.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_set_point_priors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_set_centre_priors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_set_intrinsics_priors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_solver_prior_energy.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_set_relative_poses.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.ba_solver_relative_pose_energy.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_set_preconditioner.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ba_solver_preconditioner_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_relpose_forest_plan.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.ba_problem_covisibility.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ba_intrinsics_group_plan.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.ba_solver_set_shared_intrinsics.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_solver_shared_intrinsics_info.argtypes = [C.c_void_p, C.c_void_p]
        L.ba_problem_dims.argtypes = [C.c_void_p] + [C.c_void_p] * 3
        L.ba_problem_get.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.ba_problem_load_bal.argtypes = [C.c_char_p, C.c_void_p]
        L.ba_problem_save_bal.argtypes = [C.c_void_p, C.c_char_p]
        L.ba_problem_create.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.ba_device_info.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ba_shard_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ba_problem_save_cache.argtypes = [C.c_void_p, C.c_char_p]
        L.ba_problem_load_cache.argtypes = [C.c_char_p, C.c_void_p]
        _lib = L
    return _lib


def error_string(code):
    return lib().ba_error_string(code).decode()


def status_string(status):
    return lib().ba_status_string(status).decode()


def _chk(rc, where):
    if rc != 0:
        raise BAError(rc, where)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Problem:
    """ba_problem handle: the BAL problem as the reference's loader reads it (bundle_adjustment_large.cpp:59-107)."""

    def __init__(self, handle):
        self._h = handle
        N, M, K = C.c_int(), C.c_int(), C.c_int()
        _chk(lib().ba_problem_dims(self._h, C.byref(N), C.byref(M), C.byref(K)), "ba_problem_dims")
        self.N, self.M, self.K = N.value, M.value, K.value

    @classmethod
    def load_bal(cls, path):
        h = C.c_void_p()
        _chk(lib().ba_problem_load_bal(str(path).encode(), C.byref(h)), "ba_problem_load_bal(%s)" % path)
        return cls(h)

    @classmethod
    def synthetic(cls, N, M, K, seed):
        h = C.c_void_p()
        _chk(lib().ba_problem_synthetic(N, M, K, seed, C.byref(h)), "ba_problem_synthetic")
        return cls(h)

    @classmethod
    def from_arrays(cls, N, M, K, cam_idx, pt_idx, meas, cams9, pts):
        cam_idx = np.ascontiguousarray(cam_idx, np.int32)
        pt_idx = np.ascontiguousarray(pt_idx, np.int32)
        meas = np.ascontiguousarray(meas, np.float64)
        cams9 = np.ascontiguousarray(cams9, np.float64)
        pts = np.ascontiguousarray(pts, np.float64)
        h = C.c_void_p()
        _chk(lib().ba_problem_create(N, M, K, _p(cam_idx), _p(pt_idx), _p(meas), _p(cams9), _p(pts), C.byref(h)),
             "ba_problem_create")
        return cls(h)

    def arrays(self):
        cam_idx = np.empty(self.K, np.int32)
        pt_idx = np.empty(self.K, np.int32)
        meas = np.empty(2 * self.K)
        cams9 = np.empty(9 * self.N)
        pts = np.empty(3 * self.M)
        _chk(lib().ba_problem_get(self._h, _p(cam_idx), _p(pt_idx), _p(meas), _p(cams9), _p(pts)), "ba_problem_get")
        return dict(cam_idx=cam_idx, pt_idx=pt_idx, meas=meas, cams9=cams9, pts=pts)

    def shard_plan(self, rank, world):
        out = (C.c_longlong * 8)()
        _chk(lib().ba_shard_plan(self._h, rank, world, out), "ba_shard_plan")
        keys = ("p0", "p1", "o0", "o1", "entries", "chunks", "pairs", "was_sorted")
        return dict(zip(keys, [int(v) for v in out]))

    def covisibility(self, track_max=0):
        """ba_problem_covisibility (host only): (pairs [n, 2] with a < b, weight [n]) -- the camera pairs that share points and how many,
        ordered by (weight descending, a, b).  A point seen by more than track_max cameras (0: the library's default) counts only for
        the pairs adjacent in ascending camera index."""
        n = C.c_longlong(0)
        _chk(lib().ba_problem_covisibility(self._h, int(track_max), C.byref(n), None, None), "ba_problem_covisibility")
        pairs, weight = np.zeros((n.value, 2), np.int32), np.zeros(n.value, np.int32)
        _chk(lib().ba_problem_covisibility(self._h, int(track_max), C.byref(n), _p(pairs), _p(weight)), "ba_problem_covisibility")
        return pairs, weight

    @classmethod
    def load_cache(cls, path):
        h = C.c_void_p()
        _chk(lib().ba_problem_load_cache(str(path).encode(), C.byref(h)), "ba_problem_load_cache(%s)" % path)
        return cls(h)

    def save_cache(self, path):
        _chk(lib().ba_problem_save_cache(self._h, str(path).encode()), "ba_problem_save_cache")

    def save_bal(self, path):
        _chk(lib().ba_problem_save_bal(self._h, str(path).encode()), "ba_problem_save_bal")

    @property
    def D(self):
        return 9 * self.N

    def gauge_mask(self, ref_cam=0):
        """uint16[N] camera mask that fixes the similarity gauge: FIX_POSE on ref_cam + one component of T of the camera farthest
        from it (ba_problem_gauge_mask)."""
        m = np.zeros(self.N, np.uint16)
        _chk(lib().ba_problem_gauge_mask(self._h, int(ref_cam), _p(m)), "ba_problem_gauge_mask")
        return m

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ba_problem_free(self._h)
            self._h = None


class Solver:
    """ba_solver handle: device-resident LM state of one shard."""

    def __init__(self, problem, kind=CHOLESKY, scalar=F64, device=-1, shard_rank=0, shard_world=1):
        self.problem = problem
        self.kind, self.scalar = kind, scalar
        h = C.c_void_p()
        _chk(lib().ba_solver_create(problem._h, kind, scalar, device, shard_rank, shard_world, C.byref(h)),
             "ba_solver_create")
        self._h = h
        v = [C.c_int() for _ in range(4)]
        _chk(lib().ba_solver_shard(self._h, *[C.byref(x) for x in v]), "ba_solver_shard")
        self.p0, self.p1, self.o0, self.o1 = [x.value for x in v]
        self.Ml, self.Kl = self.p1 - self.p0, self.o1 - self.o0
        self._cb_keep = None

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ba_solver_free(self._h)
            self._h = None

    # -- seam -------------------------------------------------------------------------------------------
    def linearize(self, want_diag_max=True):
        e, d = C.c_double(), C.c_double()
        _chk(lib().ba_solver_linearize(self._h, C.byref(e), C.byref(d) if want_diag_max else None), "ba_solver_linearize")
        return e.value, d.value

    def try_step(self, lam):
        e, r, n = C.c_double(), C.c_double(), C.c_double()
        _chk(lib().ba_solver_try_step(self._h, float(lam), C.byref(e), C.byref(r), C.byref(n)), "ba_solver_try_step")
        return e.value, r.value, n.value

    def accept(self):
        _chk(lib().ba_solver_accept(self._h), "ba_solver_accept")

    def stats(self):
        out = np.empty(4)
        _chk(lib().ba_solver_stats(self._h, _p(out)), "ba_solver_stats")
        return dict(mean_err=out[0], inlier_mean_err=out[1], n_inliers=int(out[2]), objective=out[3])

    def keep_intermediates(self, on=True):
        _chk(lib().ba_solver_keep_intermediates(self._h, int(on)), "ba_solver_keep_intermediates")

    def get(self, what):
        N, D, Ml, Kl = self.problem.N, self.problem.D, self.Ml, self.Kl
        n = {GET_RESIDUALS: 2 * Kl, GET_JC: 18 * Kl, GET_JP: 6 * Kl, GET_GRAD: 3 * Ml + D, GET_S: D * D, GET_RHS: D,
             GET_DX: 3 * Ml + D, GET_CAMS: 15 * N, GET_POINTS: 3 * Ml, GET_CAMS_TEST: 15 * N, GET_POINTS_TEST: 3 * Ml}[what]
        out = np.empty(n)
        _chk(lib().ba_solver_get(self._h, what, _p(out), n), "ba_solver_get(%d)" % what)
        if what == GET_S:
            return out.reshape(D, D).T
        return out

    def set_state(self, cam15=None, pts=None):
        cam15 = None if cam15 is None else np.ascontiguousarray(cam15, np.float64)
        pts = None if pts is None else np.ascontiguousarray(pts, np.float64)
        _chk(lib().ba_solver_set_state(self._h, _p(cam15), _p(pts)), "ba_solver_set_state")

    def minimize(self, max_trials=0, verbose=False, trace=True, **lm_over):
        lm = LMParams()
        lib().ba_lm_params_default(C.byref(lm))
        lm.max_trials, lm.verbose = int(max_trials), int(verbose)
        for k, v in lm_over.items():
            setattr(lm, k, v)
        rows = []
        cb = TRIAL_CB(lambda user, it, acc, f, rho, lam, el: rows.append((it, acc, f, rho, lam, el))) if trace else None
        res = Result()
        _chk(lib().ba_minimize(self._h, C.byref(lm), cb, None, C.byref(res)), "ba_minimize")
        return dict(status=res.status, iterations=res.iterations, trials=res.trials, fun_evals=res.fun_evals,
                    energy=res.energy, lam=res.lambda_, seconds=res.seconds, schur_ms=res.schur_ms,
                    linearize_ms=res.linearize_ms, trace=np.array(rows).reshape(-1, 6))

    # -- Powell's dogleg (CHOLESKY, one shard; include/ba_mi355x.h) ------------------------------------------
    def dogleg_prepare(self, mu):
        """The Gauss-Newton step (H + mu I) dx_gn = g of the linearisation in place -- try_step(mu)'s, bit for bit -- kept on the device,
        and the fp64 scalars of the dogleg: dict(mu, g2, q, gn2, g_dot_gn, alpha, energy_gn, rho_scale_gn)."""
        info = DoglegInfo()
        _chk(lib().ba_solver_dogleg_prepare(self._h, float(mu), C.byref(info)), "ba_solver_dogleg_prepare")
        return {k: getattr(info, k) for k, _ in DoglegInfo._fields_}

    def try_dogleg(self, radius):
        """The dogleg step of the prepared linearisation for this radius (inf is legal): (e_test, pred, dx_norm, branch), branch 0
        Gauss-Newton, 1 scaled gradient, 2 interpolated.  get(GET_DX) returns the step; accept() takes it."""
        e, pr, n, b = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        _chk(lib().ba_solver_try_dogleg(self._h, float(radius), C.byref(e), C.byref(pr), C.byref(n), C.byref(b)), "ba_solver_try_dogleg")
        return e.value, pr.value, n.value, b.value

    def minimize_dogleg(self, max_trials=0, verbose=False, trace=True, **over):
        """ba_minimize_dogleg with DoglegParams' defaults and `over` on top: (result dict as minimize()'s without the trace, with
        `radius` for the final radius; trace [rows, 6]: iter, accepted, f, rho, radius of the trial, elapsed)."""
        dp = DoglegParams.default()
        dp.max_trials, dp.verbose = int(max_trials), int(verbose)
        for k, v in over.items():
            if not hasattr(dp, k):
                raise TypeError("DoglegParams has no field %r" % k)
            setattr(dp, k, v)
        rows = []
        cb = TRIAL_CB(lambda user, it, acc, f, rho, rad, el: rows.append((it, acc, f, rho, rad, el))) if trace else None
        res = Result()
        _chk(lib().ba_minimize_dogleg(self._h, C.byref(dp), cb, None, C.byref(res)), "ba_minimize_dogleg")
        out = dict(status=res.status, iterations=res.iterations, trials=res.trials, fun_evals=res.fun_evals, energy=res.energy,
                   radius=res.lambda_, seconds=res.seconds, schur_ms=res.schur_ms, linearize_ms=res.linearize_ms)
        return out, np.array(rows).reshape(-1, 6)

    # -- triangulation (every kind, one shard; include/ba_mi355x.h) ---------------------------------------------
    def triangulate_points(self, points=None, min_angle_deg=None, max_reproj_px=None, refine_iters=None, only_if_better=True):
        """ba_solver_triangulate_points on the resident state for `points` (problem numbering; None = all): (stats dict with asked,
        by_status [8], cost_before, cost_after, ms; status uint8 per asked point, TRI_*).  None keeps a default of
        ba_triangulate_params_default.  A linearize() comes next."""
        tp = _tri_params(min_angle_deg, max_reproj_px, refine_iters, only_if_better)
        ids = None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1)
        n = self.problem.M if ids is None else len(ids)
        status = np.zeros(max(n, 1), np.uint8)
        ts = TriangulateStats()
        _chk(lib().ba_solver_triangulate_points(self._h, C.byref(tp), 0 if ids is None else n, None if ids is None else _p(ids), _p(status),
                                                C.byref(ts)), "ba_solver_triangulate_points")
        return (dict(asked=ts.asked, by_status=np.array(list(ts.by_status), np.int64), cost_before=ts.cost_before,
                     cost_after=ts.cost_after, ms=ts.ms), status[:n])

    # -- the active mask and the filter (CHOLESKY and ITERSCHUR, one shard; include/ba_mi355x.h) -----------------
    def set_obs_active(self, active=None):
        """ba_solver_set_obs_active: K bools / bytes of the problem in the order of the input file (None: all active).  An inactive
        observation is exactly 0 in e and J from the next linearize() / minimize() on."""
        if active is not None:
            active = np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
            if active.shape != (self.problem.K,):
                raise ValueError("active must have shape (%d,), got %s" % (self.problem.K, active.shape))
        _chk(lib().ba_solver_set_obs_active(self._h, _p(active)), "ba_solver_set_obs_active")

    def get_obs_active(self):
        """ba_solver_get_obs_active: the mask as K bools in file order."""
        a = np.zeros(max(self.problem.K, 1), np.uint8)
        n = C.c_longlong()
        _chk(lib().ba_solver_get_obs_active(self._h, _p(a), C.byref(n)), "ba_solver_get_obs_active")
        a = a[:self.problem.K].astype(bool)
        assert int(a.sum()) == n.value
        return a

    def filter_observations(self, apply=True, max_reproj_px=None, min_angle_deg=None, min_track=None, require_front=None):
        """ba_solver_filter_observations on the resident state: (stats dict with active_before, active_after, by_status [6],
        points_short, points_low_angle, err_sum_before, err_sum_after, ms; obs_status uint8 [K] in file order, OBS_*; pt_status uint8
        [M], FPT_*; err_px float64 [K] in file order).  None keeps a default of ba_filter_params_default.  With apply every observation
        that is not OBS_KEPT becomes inactive; a linearize() comes next if one was."""
        fp = _filter_params(max_reproj_px, min_angle_deg, min_track, require_front)
        K, M = self.problem.K, self.problem.M
        ost, pst, err = np.zeros(max(K, 1), np.uint8), np.zeros(max(M, 1), np.uint8), np.zeros(max(K, 1))
        fs = FilterStats()
        _chk(lib().ba_solver_filter_observations(self._h, C.byref(fp), int(bool(apply)), _p(ost), _p(pst), _p(err), C.byref(fs)),
             "ba_solver_filter_observations")
        st = {k: getattr(fs, k) for k, _ in FilterStats._fields_ if k != "by_status"}
        st["by_status"] = np.array(list(fs.by_status), np.int64)
        return st, ost[:K], pst[:M], err[:K]

    def timing(self, reset=False):
        t = Timing()
        _chk(lib().ba_solver_timing(self._h, C.byref(t), int(reset)), "ba_solver_timing")
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def time_phase(self, phase, reps, lam):
        ms = C.c_double()
        _chk(lib().ba_solver_time_phase(self._h, phase, reps, float(lam), C.byref(ms)), "ba_solver_time_phase")
        return ms.value

    def recoveries(self):
        """Trials ba_minimize repeated through the launch-per-step factorisation after a hand-off time-out."""
        return int(lib().ba_solver_recoveries(self._h))

    def set_pcg(self, max_iter, rel_tol):
        """ITERSCHUR: at most max_iter PCG iterations per trial, stop at |r| <= rel_tol |rhs|."""
        _chk(lib().ba_solver_set_pcg(self._h, int(max_iter), float(rel_tol)), "ba_solver_set_pcg")

    def set_pcg_model_tol(self, eta):
        """ITERSCHUR: 0 < eta < 1 also stops a trial's PCG at iteration k >= 1 when zeta_k = k (s_k - s_{k-1}) / s_k < eta, with
        s_k = x_k'(rhs + r_k) twice the model decrease of the iterate (truncated Newton; Ceres' eta = 0.1).  eta = 0 (a new solver's): off."""
        _chk(lib().ba_solver_set_pcg_model_tol(self._h, float(eta)), "ba_solver_set_pcg_model_tol")

    def set_damping(self, kind, diag_min=0.0, diag_max=0.0):
        """DAMP_IDENTITY (a new solver's: lambda I) or DAMP_MARQUARDT: a trial solves (J'J + lambda D) dx = -J'e with
        D_ii = min(max((J'J)_ii, diag_min), diag_max); 0 = the library's defaults (1e-6, 1e32).  lambda is then dimensionless and
        minimize() starts from LMParams.lambda_init.  CHOLESKY and ITERSCHUR, one shard; takes effect at the next try_step() / minimize()."""
        _chk(lib().ba_solver_set_damping(self._h, int(kind), float(diag_min), float(diag_max)), "ba_solver_set_damping")

    def damping(self):
        """(kind, diag_min, diag_max) in force."""
        k, lo, hi = C.c_int(), C.c_double(), C.c_double()
        _chk(lib().ba_solver_get_damping(self._h, C.byref(k), C.byref(lo), C.byref(hi)), "ba_solver_get_damping")
        return int(k.value), float(lo.value), float(hi.value)

    def set_preconditioner(self, kind, max_tree=0):
        """ITERSCHUR: PRECOND_BLOCK_JACOBI (a new solver's), PRECOND_CONSTRAINT_FOREST or PRECOND_VISIBILITY_FOREST with at most max_tree
        cameras per tree (0: the library's default for that kind)."""
        _chk(lib().ba_solver_set_preconditioner(self._h, int(kind), int(max_tree)), "ba_solver_set_preconditioner")

    def preconditioner_info(self):
        """dict(kind, max_tree, trees, kept, dropped, largest_tree, fallback_trees): the forest in force and the trees of the last solve
        that fell back to block Jacobi."""
        out, fb = np.zeros(6, np.int64), C.c_int(0)
        _chk(lib().ba_solver_preconditioner_info(self._h, _p(out), C.byref(fb)), "ba_solver_preconditioner_info")
        d = dict(zip(("kind", "max_tree", "trees", "kept", "dropped", "largest_tree"), (int(v) for v in out)))
        d["fallback_trees"] = int(fb.value)
        return d

    def set_shared_intrinsics(self, group_of=None):
        """ITERSCHUR: the cameras with one label >= 0 in group_of (N ints; < 0: a camera of its own) solve for one f, k1, k2 from the next
        try_step() / minimize() on.  Their f, k1, k2 must be bit-equal in the resident state (set_state) and their FIX_INTRINSICS bits the
        same.  None, all negative or no label used twice: no groups."""
        if group_of is not None:
            group_of = np.asarray(group_of)
            if group_of.shape != (self.problem.N,) or group_of.dtype.kind not in "iu":
                raise ValueError("group_of must be an integer array of shape (%d,), got %s %s" % (self.problem.N, group_of.dtype, group_of.shape))
            if group_of.size and (group_of.min() < -2 ** 31 or group_of.max() >= 2 ** 31):
                raise ValueError("group_of: a label does not fit a C int")
            group_of = np.ascontiguousarray(group_of, np.int32)
        _chk(lib().ba_solver_set_shared_intrinsics(self._h, _p(group_of)), "ba_solver_set_shared_intrinsics")

    def shared_intrinsics_info(self):
        """dict(groups, grouped, largest_group, chunks) of the groups in force."""
        out = np.zeros(4, np.int64)
        _chk(lib().ba_solver_shared_intrinsics_info(self._h, _p(out)), "ba_solver_shared_intrinsics_info")
        return dict(zip(("groups", "grouped", "largest_group", "chunks"), (int(v) for v in out)))

    def set_constant(self, cam_mask=None, pt_fixed=None):
        """Hold parameters constant from the next linearize() / minimize() on: cam_mask uint16[N] (FIX_* bits), pt_fixed bool / uint8[M]
        of the problem (None: nothing of that kind; both None or all zero: the unmasked solver)."""
        N, M = self.problem.N, self.problem.M
        if cam_mask is not None:
            cam_mask = np.asarray(cam_mask)
            if cam_mask.shape != (N,) or cam_mask.dtype != np.uint16:
                raise ValueError("cam_mask must be a uint16 array of shape (%d,), got %s %s" % (N, cam_mask.dtype, cam_mask.shape))
            cam_mask = np.ascontiguousarray(cam_mask)
        if pt_fixed is not None:
            pt_fixed = np.asarray(pt_fixed)
            if pt_fixed.shape != (M,) or pt_fixed.dtype not in (np.bool_, np.uint8):
                raise ValueError("pt_fixed must be a bool or uint8 array of shape (%d,), got %s %s" % (M, pt_fixed.dtype, pt_fixed.shape))
            pt_fixed = np.ascontiguousarray(pt_fixed.astype(np.uint8))
        _chk(lib().ba_solver_set_constant(self._h, _p(cam_mask), _p(pt_fixed)), "ba_solver_set_constant")

    def set_loss(self, kind, scale=0.5):
        """Loss of the measurement model from the next linearize() / minimize() on: LOSS_REFERENCE (scale = tau; the default is tau = 0.5),
        LOSS_TRIVIAL (scale ignored), LOSS_HUBER (scale = delta), LOSS_CAUCHY (scale = c)."""
        _chk(lib().ba_solver_set_loss(self._h, int(kind), float(scale)), "ba_solver_set_loss")

    def set_obs_weights(self, w=None):
        """Per-observation weights w_o > 0 of the residual r_o = w_o (projection - measurement), e.g. 1 / sigma_o: K of the problem, in
        the order of the input file (None: no weights).  Takes effect at the next linearize() / minimize()."""
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            if w.shape != (self.problem.K,):
                raise ValueError("w must have shape (%d,), got %s" % (self.problem.K, w.shape))
        _chk(lib().ba_solver_set_obs_weights(self._h, _p(w)), "ba_solver_set_obs_weights")

    @staticmethod
    def _prior_arrays(ids, x0, sqrt_info, sigma):
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        n = len(ids)
        x0 = np.ascontiguousarray(np.asarray(x0, np.float64).reshape(n, 3))
        if (sqrt_info is None) == (sigma is None):
            raise ValueError("give sqrt_info or sigma, one of them")
        if sqrt_info is None:
            sg = np.broadcast_to(np.asarray(sigma, np.float64), (n, 3))
            L = np.zeros((n, 3, 3))
            for q in range(3):
                L[:, q, q] = 1.0 / sg[:, q]
        else:
            L = np.asarray(sqrt_info, np.float64).reshape(n, 3, 3)
        return n, ids, x0, np.ascontiguousarray(L)

    def set_point_priors(self, ids, x0, sqrt_info=None, sigma=None):
        """Gaussian priors e = L (X - x0) on the points `ids` of the problem from the next linearize() / minimize() on: sqrt_info (n, 3, 3)
        is L, or sigma (a scalar or (n, 3)) gives L = diag(1 / sigma).  An empty list removes them (CHOLESKY, ITERSCHUR; one shard)."""
        n, ids, x0, L = self._prior_arrays(ids, x0, sqrt_info, sigma)
        _chk(lib().ba_solver_set_point_priors(self._h, n, _p(ids), _p(x0), _p(L)), "ba_solver_set_point_priors")

    def set_centre_priors(self, ids, c0, sqrt_info=None, sigma=None):
        """Gaussian priors e = L (C - c0) on the centres C = -R^T T of the cameras `ids` (e.g. GNSS positions); arguments as set_point_priors."""
        n, ids, c0, L = self._prior_arrays(ids, c0, sqrt_info, sigma)
        _chk(lib().ba_solver_set_centre_priors(self._h, n, _p(ids), _p(c0), _p(L)), "ba_solver_set_centre_priors")

    def set_intrinsics_priors(self, ids, x0, sigma):
        """Priors e_q = (x_q - x0_q) / sigma_q on (f, k1, k2) of the cameras `ids`, in the units of get(GET_CAMS)[:, 12:15]; sigma is a
        scalar or (n, 3), and sigma_q = inf leaves parameter q without a row."""
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        n = len(ids)
        x0 = np.ascontiguousarray(np.asarray(x0, np.float64).reshape(n, 3))
        w = np.ascontiguousarray(1.0 / np.broadcast_to(np.asarray(sigma, np.float64), (n, 3)))
        _chk(lib().ba_solver_set_intrinsics_priors(self._h, n, _p(ids), _p(x0), _p(w)), "ba_solver_set_intrinsics_priors")

    def prior_energy(self):
        """Energies (sum of e^2) of the point, centre and intrinsics priors at x of the last linearize()."""
        out = np.empty(3)
        _chk(lib().ba_solver_prior_energy(self._h, _p(out)), "ba_solver_prior_energy")
        return out

    def set_relative_poses(self, pairs, R0, t0, sqrt_info_rot=None, sqrt_info_trans=None, sigma_rot=None, sigma_trans=None):
        """Relative-pose constraints e_t = L_t (t_ab - t0), e_r = L_r Log(R_ab R0^T) between the camera pairs (a, b) of `pairs` (n, 2), with
        R_ab = R_b R_a^T, t_ab = T_b - R_ab T_a, from the next linearize() / minimize() on.  R0 (n, 3, 3), t0 (n, 3); per kind either
        sqrt_info_* (n, 3, 3) = L or sigma_* (a scalar or (n, 3): L = diag(1 / sigma), radians / the units of T); neither: no rows of that
        kind.  An empty list removes the constraints (CHOLESKY, ITERSCHUR; one shard)."""
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        n = len(pairs)
        R0 = np.ascontiguousarray(np.asarray(R0, np.float64).reshape(n, 3, 3))
        t0 = np.ascontiguousarray(np.asarray(t0, np.float64).reshape(n, 3))

        def info(L, sigma, what):
            if L is not None and sigma is not None:
                raise ValueError("give sqrt_info_%s or sigma_%s, not both" % (what, what))
            out = np.zeros((n, 3, 3))
            if L is not None:
                out[:] = np.asarray(L, np.float64).reshape(n, 3, 3)
            elif sigma is not None:
                sg = np.broadcast_to(np.asarray(sigma, np.float64), (n, 3))
                for q in range(3):
                    out[:, q, q] = 1.0 / sg[:, q]
            return np.ascontiguousarray(out)
        Lr, Lt = info(sqrt_info_rot, sigma_rot, "rot"), info(sqrt_info_trans, sigma_trans, "trans")
        _chk(lib().ba_solver_set_relative_poses(self._h, n, _p(pairs), _p(R0), _p(t0), _p(Lr), _p(Lt)), "ba_solver_set_relative_poses")

    def relative_pose_energy(self):
        """(sum |e_r|^2, sum |e_t|^2) of the relative-pose constraints at x of the last linearize()."""
        out = np.empty(2)
        _chk(lib().ba_solver_relative_pose_energy(self._h, _p(out)), "ba_solver_relative_pose_energy")
        return out

    def pcg_stats(self, reset=False):
        """ITERSCHUR: solves and iterations counted on the device; the last solve's iterations, convergence and |rhs - S dx_c| / |rhs|."""
        st = PCGStats()
        _chk(lib().ba_solver_pcg_stats(self._h, C.byref(st), int(reset)), "ba_solver_pcg_stats")
        return {k: getattr(st, k) for k, _ in PCGStats._fields_}

    def pcg_stop_stats(self, reset=False):
        """ITERSCHUR with set_pcg_model_tol(eta > 0): solves ended by the residual rule, by the model rule and at the cap; the last
        solve's rule (0 cap, 1 residual, 2 model), zeta_k and s_k at its final iterate."""
        st = PCGStopStats()
        _chk(lib().ba_solver_pcg_stop_stats(self._h, C.byref(st), int(reset)), "ba_solver_pcg_stop_stats")
        return {k: getattr(st, k) for k, _ in PCGStopStats._fields_}

    def covariance(self, lam=0.0, cam_pairs=None, cams=None, points=None, compute=True):
        """Covariance blocks of the estimate at the last linearize(): Sigma = (J'J + lam I)^-1 on the free parameters, 0 for fixed ones
        (ba_solver_covariance_compute / _get; CHOLESKY and QRCHOL, F64, one shard).  cam_pairs: (n, 2) camera pairs -> (n, 9, 9);
        cams=[a, ...] is shorthand for the diagonal pairs (a, a); points: point ids of the problem -> (m, 3, 3).  Returns
        (camera blocks, point blocks), an empty array for a list not given.  compute=False reads further blocks of the last result.
        Raises BAError: code ERR_SINGULAR when J'J + lam I is not positive definite on the free parameters."""
        if cam_pairs is not None and cams is not None:
            raise ValueError("give cam_pairs or cams, not both")
        if cams is not None:
            cams = np.asarray(cams, np.int32).reshape(-1)
            cam_pairs = np.stack([cams, cams], axis=1)
        pairs = np.zeros((0, 2), np.int32) if cam_pairs is None else np.ascontiguousarray(cam_pairs, np.int32).reshape(-1, 2)
        pts = np.zeros(0, np.int32) if points is None else np.ascontiguousarray(points, np.int32).reshape(-1)
        if compute:
            _chk(lib().ba_solver_covariance_compute(self._h, float(lam)), "ba_solver_covariance_compute")
        cc = np.empty((len(pairs), 9, 9))
        pc = np.empty((len(pts), 3, 3))
        _chk(lib().ba_solver_covariance_get(self._h, len(pairs), _p(pairs), _p(cc), len(pts), _p(pts), _p(pc)), "ba_solver_covariance_get")
        return cc, pc

    def covariance_pcg(self, lam=0.0, cam_pairs=None, cams=None, points=None, max_iter=0, rel_tol=0.0):
        """ITERSCHUR: covariance blocks without forming S, by a PCG on nine right-hand sides at a time (ba_solver_covariance_pcg; F64,
        one shard).  The arguments of covariance(); max_iter = 0 / rel_tol = 0 take the values of set_pcg.  Returns (camera blocks,
        point blocks, stats): stats["unconverged"] counts the columns that ended at max_iter (no error: look at it), and
        stats["worst_rel_residual"] is the largest |b - S x| / |b| of a column.  Raises BAError: code ERR_SINGULAR when a point block or a
        camera's diagonal block is not positive definite, or a search direction has p'Sp <= 0."""
        if cam_pairs is not None and cams is not None:
            raise ValueError("give cam_pairs or cams, not both")
        if cams is not None:
            cams = np.asarray(cams, np.int32).reshape(-1)
            cam_pairs = np.stack([cams, cams], axis=1)
        pairs = np.zeros((0, 2), np.int32) if cam_pairs is None else np.ascontiguousarray(cam_pairs, np.int32).reshape(-1, 2)
        pts = np.zeros(0, np.int32) if points is None else np.ascontiguousarray(points, np.int32).reshape(-1)
        cc = np.empty((len(pairs), 9, 9))
        pc = np.empty((len(pts), 3, 3))
        st = CovPCGStats()
        _chk(lib().ba_solver_covariance_pcg(self._h, float(lam), int(max_iter), float(rel_tol), len(pairs), _p(pairs), _p(cc), len(pts), _p(pts),
                                            _p(pc), C.byref(st)), "ba_solver_covariance_pcg")
        return cc, pc, {k: getattr(st, k) for k, _ in CovPCGStats._fields_}

    def covariance_timing(self):
        """Device ms: (assembly, factorisation, inverse) of the last covariance compute, the point kernel of the last read of points."""
        out = np.empty(4)
        _chk(lib().ba_solver_covariance_timing(self._h, _p(out)), "ba_solver_covariance_timing")
        return tuple(float(v) for v in out)

    def device_bytes(self):
        """Sum of the handle's device allocations."""
        n = C.c_size_t()
        _chk(lib().ba_solver_device_bytes(self._h, C.byref(n)), "ba_solver_device_bytes")
        return n.value

    def selftest(self, which):
        """Returns the library's return code (not raised): the failure paths are what this hook exists to show."""
        return int(lib().ba_solver_selftest(self._h, int(which)))

    # -- multi-GPU plumbing -------------------------------------------------------------------------------
    def set_stream(self, raw_stream):
        _chk(lib().ba_solver_set_stream(self._h, C.c_void_p(raw_stream)), "ba_solver_set_stream")

    def comm_init(self, comm_id):
        """RCCL inside the library: comm_id = the 128 bytes of comm_unique_id() from shard rank 0; collective over the shard group."""
        buf = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        _chk(lib().ba_solver_comm_init(self._h, buf), "ba_solver_comm_init")

    def set_allreduce(self, pyfunc):
        """pyfunc(dev_ptr:int, count:int, scalar:int, op:int, stream:int) -> int (0 = ok)."""
        def tramp(user, buf, count, scalar, op, stream):
            try:
                return int(pyfunc(buf or 0, count, scalar, op, stream or 0))
            except Exception as exc:  # never unwind through C
                import sys
                print("allreduce callback raised: %r" % (exc,), file=sys.stderr)
                return 1
        self._cb_keep = ALLREDUCE_FN(tramp)
        _chk(lib().ba_solver_set_allreduce(self._h, C.cast(self._cb_keep, C.c_void_p), None), "ba_solver_set_allreduce")


COMM_ID_BYTES = 128


def forest_plan(N, pairs, max_tree):
    """ba_relpose_forest_plan (host only): dict(parent [N], via [N], order [N], kept [n] bool) of the spanning forest that
    PRECOND_CONSTRAINT_FOREST builds from the constraint list `pairs` ([n, 2]) with at most max_tree cameras per tree."""
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    n = len(pairs)
    parent, via, order = (np.zeros(max(int(N), 0), np.int32) for _ in range(3))
    kept = np.zeros(n, np.uint8)
    _chk(lib().ba_relpose_forest_plan(int(N), n, _p(pairs), int(max_tree), _p(parent), _p(via), _p(order), _p(kept)), "ba_relpose_forest_plan")
    return dict(parent=parent, via=via, order=order, kept=kept.astype(bool))


def intrinsics_group_plan(N, group_of, chunk=256):
    """ba_intrinsics_group_plan (host only): dict(group_ptr [g + 1], members, chunk_ptr [c + 1], chunk_group [c]) of the groups that
    Solver.set_shared_intrinsics builds from the labels group_of ([N]; < 0: no group) with at most `chunk` members per chunk."""
    if group_of is not None:
        group_of = np.asarray(group_of)
        if int(N) >= 0 and (group_of.shape != (int(N),) or (group_of.size and group_of.dtype.kind not in "iu")):  # (N < 0: refused unread)
            raise ValueError("group_of must be an integer array of shape (%d,), got %s %s" % (int(N), group_of.dtype, group_of.shape))
        if group_of.size and (group_of.min() < -2 ** 31 or group_of.max() >= 2 ** 31):
            raise ValueError("group_of: a label does not fit a C int")
        group_of = np.ascontiguousarray(group_of.reshape(-1), np.int32)
    ng, nc = C.c_int(0), C.c_int(0)
    _chk(lib().ba_intrinsics_group_plan(int(N), _p(group_of), int(chunk), C.byref(ng), None, None, C.byref(nc), None, None),
         "ba_intrinsics_group_plan")
    n = max(int(N), 0)
    group_ptr, members = np.zeros(ng.value + 1, np.int32), np.zeros(n, np.int32)
    chunk_ptr, chunk_group = np.zeros(nc.value + 1, np.int32), np.zeros(nc.value, np.int32)
    _chk(lib().ba_intrinsics_group_plan(int(N), _p(group_of), int(chunk), C.byref(ng), _p(group_ptr), _p(members), C.byref(nc), _p(chunk_ptr),
                                        _p(chunk_group)), "ba_intrinsics_group_plan")
    return dict(group_ptr=group_ptr, members=members[:group_ptr[-1]].copy(), chunk_ptr=chunk_ptr, chunk_group=chunk_group)


def dogleg_coefficients(g2, q, gn2, g_dot_gn, mu, radius):
    """ba_dogleg_coefficients (host only): (a, c, branch, pred) of the dogleg step dx = a g + c dx_gn for this radius from the scalars
    of Solver.dogleg_prepare.  Raises BAError (ERR_ARG) for what the library refuses."""
    a, c, pr, b = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    _chk(lib().ba_dogleg_coefficients(float(g2), float(q), float(gn2), float(g_dot_gn), float(mu), float(radius), C.byref(a), C.byref(c),
                                      C.byref(b), C.byref(pr)), "ba_dogleg_coefficients")
    return a.value, c.value, b.value, pr.value


def triangulate_point(cam15, meas, x_old, w=None, loss_kind=LOSS_REFERENCE, loss_scale=0.5, min_angle_deg=None, max_reproj_px=None,
                      refine_iters=None, only_if_better=True):
    """ba_triangulate_point (host only): the per-point rule on one track.  cam15 [t, 15] (rows of GET_CAMS, one per observation),
    meas [t, 2], w [t] or None: dict(x, status, cost_old, cost_new, angle_deg).  Raises BAError (ERR_ARG) for what the library refuses."""
    cam15 = np.ascontiguousarray(cam15, np.float64).reshape(-1, 15)
    t = len(cam15)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 2)
    x_old = np.ascontiguousarray(x_old, np.float64).reshape(3)
    if len(meas) != t or (w is not None and np.size(w) != t):
        raise ValueError("cam15, meas and w disagree on the track length")
    ww = None if w is None else np.ascontiguousarray(w, np.float64).reshape(-1)
    tp = _tri_params(min_angle_deg, max_reproj_px, refine_iters, only_if_better)
    x = np.zeros(3)
    st, c0, c1, ang = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    _chk(lib().ba_triangulate_point(t, _p(cam15) if t else None, _p(meas) if t else None, None if ww is None or not t else _p(ww),
                                    int(loss_kind), float(loss_scale), C.byref(tp), _p(x_old), _p(x), C.byref(st), C.byref(c0), C.byref(c1),
                                    C.byref(ang)), "ba_triangulate_point")
    return dict(x=x, status=st.value, cost_old=c0.value, cost_new=c1.value, angle_deg=ang.value)


def filter_track(cam15, meas, X, active=None, max_reproj_px=None, min_angle_deg=None, min_track=None, require_front=None):
    """ba_filter_track (host only): the filter's per-point rule on one track.  cam15 [t, 15] (rows of GET_CAMS, one per observation),
    meas [t, 2], active [t] or None: dict(obs_status uint8 [t], pt_status, err_px [t], angle_deg).  Raises BAError (ERR_ARG) for what
    the library refuses."""
    cam15 = np.ascontiguousarray(cam15, np.float64).reshape(-1, 15)
    t = len(cam15)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 2)
    X = np.ascontiguousarray(X, np.float64).reshape(3)
    if len(meas) != t or (active is not None and np.size(active) != t):
        raise ValueError("cam15, meas and active disagree on the track length")
    act = None if active is None else np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, np.uint8)
    fp = _filter_params(max_reproj_px, min_angle_deg, min_track, require_front)
    ost, err = np.zeros(max(t, 1), np.uint8), np.zeros(max(t, 1))
    ps, ang = C.c_int(), C.c_double()
    _chk(lib().ba_filter_track(t, _p(cam15) if t else None, _p(meas) if t else None, None if act is None or not t else _p(act), _p(X),
                               C.byref(fp), _p(ost), C.byref(ps), _p(err), C.byref(ang)), "ba_filter_track")
    return dict(obs_status=ost[:t], pt_status=ps.value, err_px=err[:t], angle_deg=ang.value)


def relative_pose(cam15, a, b):
    """(R_ab, t_ab) = (R_b R_a^T, T_b - R_ab T_a) of cameras a and b of a state as Solver.get(GET_CAMS) returns it (host only): the
    pose of a's frame seen from b's, x_b = R_ab x_a + t_ab -- what Solver.set_relative_poses constrains."""
    c = np.asarray(cam15, np.float64).reshape(-1, 15)
    Ra, Rb = c[a, :9].reshape(3, 3), c[b, :9].reshape(3, 3)
    Rab = Rb @ Ra.T
    return Rab, c[b, 9:12] - Rab @ c[a, 9:12]


def comm_unique_id():
    """ncclGetUniqueId through the library (call on shard rank 0, carry the bytes to the other ranks)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _chk(lib().ba_comm_unique_id(buf), "ba_comm_unique_id")
    return buf.raw


def device_info(device=-1):
    name = C.create_string_buffer(256)
    cus = C.c_int()
    _chk(lib().ba_device_info(device, name, 256, C.byref(cus)), "ba_device_info")
    return name.value.decode(), cus.value
