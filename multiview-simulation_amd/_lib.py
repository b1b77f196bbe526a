"""ctypes binding of libmvsim.so (include/mvsim.h).  No CPU fallback: if the HIP library is
missing or no gfx950 device is usable, every compute entry point raises."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmvsim.so")

MVSIM_OK, MVSIM_EINVAL, MVSIM_ENOMEM, MVSIM_EHIP, MVSIM_EFFT, MVSIM_ERCCL, MVSIM_ENODEV = 0, -1, -2, -3, -4, -5, -6
UNIQUE_ID_BYTES = 128


class MvsimError(RuntimeError):
    """HIP / rocFFT / RCCL failure inside libmvsim (Java side: RuntimeException)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"libmvsim status {status}: {message}")
        self.status = status


class MvsimNoDeviceError(MvsimError):
    pass


class ViewParams(C.Structure):
    _fields_ = [
        ("axis", C.c_int32), ("degrees", C.c_int32), ("delta", C.c_double), ("min_value", C.c_float),
        ("target_average", C.c_float), ("inc", C.c_int32), ("snr", C.c_float), ("seed", C.c_uint64),
        ("stream", C.c_uint32), ("conv_method", C.c_int32),
    ]


class BcastOp(C.Structure):
    _fields_ = [("stage", C.c_int32), ("kind", C.c_int32), ("peer", C.c_int32), ("pad", C.c_int32), ("first", C.c_int64), ("count", C.c_int64)]


class ViewOutputs(C.Structure):
    _fields_ = [("rot", C.c_void_p), ("att", C.c_void_p), ("con", C.c_void_p), ("acq", C.c_void_p)]


class IterationOutputs(C.Structure):
    _fields_ = [("iso", C.c_void_p), ("view", C.c_void_p), ("view_weights", C.c_void_p), ("view_psf", C.c_void_p)]


class Sphere(C.Structure):
    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("cz", C.c_int32), ("radius", C.c_int32), ("value", C.c_float)]


class RaySteps(C.Structure):
    """mvsim_ray_steps: host arrays the step list of refract3d is written to."""
    _fields_ = [("capacity", C.c_int64), ("n", C.c_int64), ("xyz", C.POINTER(C.c_double)), ("value", C.POINTER(C.c_float)),
                ("moves", C.POINTER(C.c_int32))]


class TraceParams(C.Structure):
    """mvsim_trace_params: the settings of mvsim_trace_rays."""
    _fields_ = [("n_a", C.c_double), ("n_b", C.c_double), ("ev_threshold", C.c_double), ("max_moves", C.c_int64),
                ("total_reflection", C.c_int32), ("normalize_dirs", C.c_int32), ("constant_value", C.c_double), ("sigma", C.c_double * 3),
                ("normalized", C.c_int32)]


MVSIM_TRACE_KEEP, MVSIM_TRACE_REFLECT = 0, 1


class Perlin(C.Structure):
    """mvsim_perlin: a Perlin field (host tables)."""
    _fields_ = [("scales", C.c_double * 3), ("loop_extents", C.c_int32 * 3), ("n_vectors", C.c_int32), ("gradients", C.POINTER(C.c_double)),
                ("permutation", C.POINTER(C.c_int32)), ("threshold", C.c_double)]


class SphereSet(C.Structure):
    """mvsim_sphere_set: spheres in list order (host arrays)."""
    _fields_ = [("n", C.c_int64), ("centres", C.POINTER(C.c_double)), ("radii", C.POINTER(C.c_double)), ("values", C.POINTER(C.c_float)),
                ("background", C.c_float)]


class Density(C.Structure):
    """mvsim_density: what mvsim_rejection_sample samples against."""
    _fields_ = [("kind", C.c_int32), ("perlin", C.POINTER(Perlin)), ("spheres", C.POINTER(SphereSet))]


class IntervalJob(C.Structure):
    """mvsim_interval_job: extractSlices over the interval [min, max] (inclusive, x first) of a DEVICE volume."""
    _fields_ = [("in_", C.c_void_p), ("dim", C.c_int64 * 3), ("min", C.c_int64 * 3), ("max", C.c_int64 * 3), ("inc", C.c_int32),
                ("snr", C.c_float), ("seed", C.c_uint64), ("stream", C.c_uint32)]


class DeconParams(C.Structure):
    """mvsim_decon_params: the settings of mvsim_deconvolve (mvsim_decon_params_default fills them)."""
    _fields_ = [("iterations", C.c_int32), ("method", C.c_int32), ("init_from_psi", C.c_int32), ("init_value", C.c_float),
                ("min_value", C.c_float), ("eps", C.c_float), ("lambda_", C.c_double)]


class DeconStat(C.Structure):
    """mvsim_decon_stat: what one update step reports."""
    _fields_ = [("sum_psi", C.c_double), ("max_change", C.c_float), ("n_floored", C.c_int64)]

    def as_dict(self):
        return {"sum_psi": float(self.sum_psi), "max_change": float(self.max_change), "n_floored": int(self.n_floored)}


class DogParams(C.Structure):
    """mvsim_dog_params: the settings of the bead detector (mvsim_dog_params_default fills them)."""
    _fields_ = [("sigma1", C.c_double * 3), ("sigma2", C.c_double * 3), ("threshold", C.c_float), ("max_moves", C.c_int32)]


class Peak(C.Structure):
    """mvsim_peak: one localised detection."""
    _fields_ = [("pos", C.c_double * 3), ("value", C.c_float), ("flags", C.c_int32), ("voxel", C.c_int64)]


class MatchParams(C.Structure):
    """mvsim_match_params: the settings of the bead registration (mvsim_match_params_default fills them)."""
    _fields_ = [("ratio", C.c_double), ("max_epsilon", C.c_double), ("min_inlier_ratio", C.c_double), ("seed", C.c_int64),
                ("redundancy", C.c_int32), ("hypotheses", C.c_int32), ("max_refits", C.c_int32), ("min_inliers", C.c_int32)]


class Match(C.Structure):
    """mvsim_match: one candidate correspondence."""
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("v_best", C.c_double), ("v_second", C.c_double)]


class Registration(C.Structure):
    """mvsim_registration: what the RANSAC and refit stage reports."""
    _fields_ = [("m", C.c_double * 12), ("mean_error", C.c_double), ("max_error", C.c_double), ("n_a", C.c_int64), ("n_b", C.c_int64),
                ("n_candidates", C.c_int64), ("n_inliers", C.c_int64), ("best_hypothesis", C.c_int64), ("refits", C.c_int32),
                ("flags", C.c_int32)]


class FuseParams(C.Structure):
    """mvsim_fuse_params: the settings of the view fusion (mvsim_fuse_params_default fills them)."""
    _fields_ = [("blend", C.c_double * 3), ("background", C.c_float), ("src_type", C.c_int32)]


class FuseView(C.Structure):
    """mvsim_fuse_view: one view of a fusion -- its voxels, its extents and its matrix view -> output frame (host, or 12 doubles in
    device memory)."""
    _fields_ = [("src", C.c_void_p), ("dim", C.c_int64 * 3), ("m_dev", C.c_void_p), ("m", C.c_double * 12)]


class PsfParams(C.Structure):
    """mvsim_psf_params: the settings of the PSF extraction (mvsim_psf_params_default fills them)."""
    _fields_ = [("kdim", C.c_int64 * 3), ("min_separation", C.c_double * 3), ("src_type", C.c_int32), ("subtract_min", C.c_int32),
                ("normalize", C.c_int32), ("pad", C.c_int32)]


class PsfResult(C.Structure):
    """mvsim_psf_result: what the PSF extraction reports beside the PSF."""
    _fields_ = [("minimum", C.c_double), ("sum", C.c_double), ("n_listed", C.c_int64), ("n_used", C.c_int64), ("n_nonfinite", C.c_int64),
                ("n_masked", C.c_int64), ("n_outside", C.c_int64), ("n_crowded", C.c_int64), ("flags", C.c_int32), ("pad", C.c_int32)]


MVSIM_MAX_VIEWS = 32
MVSIM_PSF_MAX_POINTS, MVSIM_PSF_MAX_DIM, MVSIM_PSF_CHUNK = 65536, 63, 256
MVSIM_PSF_USED, MVSIM_PSF_NONFINITE, MVSIM_PSF_MASKED, MVSIM_PSF_OUTSIDE, MVSIM_PSF_CROWDED = 0, 1, 2, 3, 4
MVSIM_PSF_SINGULAR, MVSIM_PSF_NO_BEADS, MVSIM_PSF_FLAT = 1, 2, 4
MVSIM_FUSE_SINGULAR = 1
MVSIM_REG_MAX_POINTS, MVSIM_REG_FIT_CHUNK = 65536, 256
MVSIM_REG_FEW_CANDIDATES, MVSIM_REG_NO_MODEL, MVSIM_REG_CAPPED, MVSIM_REG_FEW_INLIERS = 1, 2, 4, 8
MVSIM_SRC_F32, MVSIM_SRC_U16 = 0, 1
MVSIM_DOG_MAX_TAPS = 63
MVSIM_PEAK_SINGULAR, MVSIM_PEAK_FROZEN, MVSIM_PEAK_CAPPED, MVSIM_PEAK_OUTSIDE = 1, 2, 4, 8


class Timings(C.Structure):
    _fields_ = [(n, C.c_float) for n in
                ("rotate_ms", "attenuate_ms", "psf_ms", "convolve_ms", "adjust_ms", "extract_ms", "total_ms",
                 "pass_a_ms", "pass_b_ms", "pass_c_ms", "pass_d_ms", "pass_e_ms")]

    def as_dict(self):
        return {n: float(getattr(self, n)) for n, _ in self._fields_}


_i64p = C.POINTER(C.c_int64)
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)

# name -> (restype, argtypes).  Must list every symbol declared in include/mvsim.h.
SIGNATURES = {
    "mvsim_version": (C.c_char_p, []),
    "mvsim_last_error": (C.c_char_p, []),
    "mvsim_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mvsim_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "mvsim_destroy": (C.c_int, [_vp]),
    "mvsim_set_stream": (C.c_int, [_vp, _vp]),
    "mvsim_synchronize": (C.c_int, [_vp]),
    "mvsim_join": (C.c_int, [_vp]),
    "mvsim_set_option": (C.c_int, [_vp, C.c_char_p, C.c_char_p]),
    "mvsim_release_caches": (C.c_int, [_vp]),
    "mvsim_dev_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "mvsim_dev_free": (C.c_int, [_vp, _vp]),
    "mvsim_upload": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "mvsim_dev_memset": (C.c_int, [_vp, _vp, C.c_int, C.c_size_t]),
    "mvsim_host_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mvsim_host_free": (C.c_int, [_vp, _vp]),
    "mvsim_download": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "mvsim_axis_rotation": (C.c_int, [_i64p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "mvsim_extract_nz": (C.c_int64, [C.c_int64, C.c_int]),
    "mvsim_isotropic_nz": (C.c_int64, [C.c_int64, C.c_int]),
    "mvsim_poisson_mul": (C.c_double, [C.c_double]),
    "mvsim_rotate_around_axis": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_int, _vp]),
    "mvsim_attenuate3d": (C.c_int, [_vp, _vp, _i64p, C.c_double, _vp]),
    "mvsim_norm_image": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvsim_convolve": (C.c_int, [_vp, _vp, _i64p, _vp, _i64p, C.c_int, _vp]),
    "mvsim_adjust_image": (C.c_int, [_vp, _vp, C.c_int64, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "mvsim_extract_slices": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_float, C.c_uint64, C.c_uint32, _vp]),
    "mvsim_poisson_process": (C.c_int, [_vp, _vp, C.c_int64, C.c_double, C.c_uint64, C.c_uint32, C.c_uint64]),
    "mvsim_make_isotropic": (C.c_int, [_vp, _vp, _i64p, C.c_int, _vp]),
    "mvsim_compute_weight_image": (C.c_int, [_vp, _i64p, _vp]),
    "mvsim_rotate_around_axis_dev": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_int, _vp]),
    "mvsim_attenuate3d_dev": (C.c_int, [_vp, _vp, _i64p, C.c_double, _vp]),
    "mvsim_convolve_dev": (C.c_int, [_vp, _vp, _i64p, _vp, _i64p, C.c_int, _vp]),
    "mvsim_adjust_image_dev": (C.c_int, [_vp, _vp, C.c_int64, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "mvsim_extract_slices_dev": (C.c_int, [_vp, _vp, _i64p, C.c_int, C.c_float, C.c_uint64, C.c_uint32, _vp]),
    "mvsim_make_isotropic_dev": (C.c_int, [_vp, _vp, _i64p, C.c_int, _vp]),
    "mvsim_interval_out_dim": (C.c_int, [C.POINTER(IntervalJob), _i64p]),
    "mvsim_extract_intervals_dev": (C.c_int, [_vp, C.POINTER(IntervalJob), C.c_int, C.POINTER(_vp)]),
    "mvsim_extract_intervals": (C.c_int, [_vp, C.POINTER(IntervalJob), C.c_int, C.POINTER(_vp)]),
    "mvsim_tile_interval": (C.c_int, [_i64p, _dp, C.c_int, _i64p, _i64p, _i64p]),
    "mvsim_draw_spheres": (C.c_int, [_vp, _vp, _i64p, C.c_double, C.c_double, C.c_int, C.c_int,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "mvsim_draw_spheres_dev": (C.c_int, [_vp, _vp, _i64p, C.c_double, C.c_double, C.c_int, C.c_int,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "mvsim_downsample2x": (C.c_int, [_vp, _vp, _i64p, _vp]),
    "mvsim_downsample2x_dev": (C.c_int, [_vp, _vp, _i64p, _vp]),
    "mvsim_compute_weight_image_dev": (C.c_int, [_vp, _i64p, _vp]),
    "mvsim_sum_views_dev": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int64, _vp]),
    "mvsim_normalize_weights_dev": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int64, _vp, C.c_float]),
    "mvsim_normalize_weights": (C.c_int, [_vp, C.POINTER(_vp), C.c_int, C.c_int64, C.c_float]),
    "mvsim_view_params_default": (None, [C.POINTER(ViewParams)]),
    "mvsim_simulate_view_dev": (C.c_int, [_vp, _vp, _i64p, _vp, _i64p, C.POINTER(ViewParams),
                                          C.POINTER(ViewOutputs), C.POINTER(C.c_double)]),
    "mvsim_get_plane_stats": (C.c_int, [_vp, _i64p]),
    "mvsim_get_tail_path": (C.c_int, [_vp, _i64p]),
    "mvsim_get_psf_cache_stats": (C.c_int, [_vp, _i64p]),
    "mvsim_get_queue_stats": (C.c_int, [_vp, _i64p]),
    "mvsim_get_transfer_stats": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mvsim_simulate_views_dev": (C.c_int, [_vp, _vp, _i64p, C.POINTER(_vp), _i64p, C.POINTER(ViewParams),
                                           C.POINTER(ViewOutputs), C.c_int]),
    "mvsim_simulate_views": (C.c_int, [_vp, _vp, _i64p, C.POINTER(_vp), _i64p, C.POINTER(ViewParams), C.POINTER(_vp), C.c_int]),
    "mvsim_simulate_iteration_dev": (C.c_int, [_vp, _vp, _i64p, _vp, _i64p, C.POINTER(ViewParams), C.c_int,
                                               C.POINTER(ViewOutputs), C.POINTER(IterationOutputs)]),
    "mvsim_simulate_view": (C.c_int, [_vp, _vp, _i64p, _vp, _i64p, C.POINTER(ViewParams),
                                      C.POINTER(ViewOutputs), C.POINTER(C.c_double)]),
    "mvsim_splat_spheres": (C.c_int, [_vp, _vp, _i64p, _vp, C.c_int64]),
    "mvsim_splat_spheres_dev": (C.c_int, [_vp, _vp, _i64p, _vp, C.c_int64]),
    "mvsim_simulate_view_async": (C.c_int, [_vp, _vp, C.c_uint64, _i64p, _vp, _i64p, C.POINTER(ViewParams),
                                            C.POINTER(ViewOutputs), C.POINTER(C.c_int64)]),
    "mvsim_wait": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_double)]),
    "mvsim_simulate_view_zslabs": (C.c_int, [_vp, C.POINTER(_vp), _i64p, C.c_int, _i64p, _vp, _i64p, C.POINTER(ViewParams),
                                             C.POINTER(_vp), _i64p, C.c_int, C.POINTER(C.c_double)]),
    "mvsim_fft_geometry": (C.c_int, [_i64p, _i64p, _i64p]),
    "mvsim_zpass_geometry": (C.c_int, [_i64p, _i64p, C.c_int, _i64p]),
    "mvsim_rotate_around_axis_zslabs": (C.c_int, [_vp, C.POINTER(_vp), _i64p, C.c_int, _i64p, C.c_int, C.c_int, C.POINTER(_vp), _i64p, C.c_int]),
    "mvsim_attenuate3d_zslabs": (C.c_int, [_vp, C.POINTER(_vp), _i64p, C.c_int, _i64p, C.c_double, C.POINTER(_vp), _i64p, C.c_int]),
    "mvsim_convolve_zslabs": (C.c_int, [_vp, C.POINTER(_vp), _i64p, C.c_int, _i64p, _vp, _i64p, C.c_int, C.POINTER(_vp), _i64p, C.c_int]),
    "mvsim_extract_slices_zslabs": (C.c_int, [_vp, C.POINTER(_vp), _i64p, C.c_int, _i64p, C.c_int, C.c_float, C.c_uint64, C.c_uint32,
                                              C.POINTER(_vp), _i64p, C.c_int]),
    "mvsim_stencil_geometry": (C.c_int, [_i64p, _i64p]),
    "mvsim_extract_path": (C.c_int, [_i64p, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, _i64p]),
    "mvsim_fused_tail_geometry": (C.c_int, [_vp, _i64p, _i64p, C.c_int, C.c_int, _i64p]),
    "mvsim_get_extract_path": (C.c_int, [_vp, _i64p]),
    "mvsim_enable_timing": (C.c_int, [_vp, C.c_int]),
    "mvsim_get_timings": (C.c_int, [_vp, C.POINTER(Timings)]),
    "mvsim_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "mvsim_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]),
    "mvsim_comm_library_info": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "mvsim_comm_broadcast_volume": (C.c_int, [_vp, _vp, C.c_int64, C.c_int]),
    "mvsim_comm_broadcast_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, _vp, C.c_int, C.POINTER(C.c_int)]),
    "mvsim_comm_register_volume": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvsim_comm_unregister_volume": (C.c_int, [_vp, _vp]),
    "mvsim_comm_allreduce_sum": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvsim_comm_allreduce_sum_f64": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "mvsim_slab_range": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mvsim_view_slab_convolve_dev": (C.c_int, [_vp, _vp, _i64p, _vp, _i64p, _vp, C.c_int64, C.c_int64,
                                               C.POINTER(C.c_double)]),
    "mvsim_view_slab_finish_dev": (C.c_int, [_vp, _i64p, _vp, C.c_int64, C.c_int64, C.c_double, _vp,
                                             C.POINTER(C.c_int64)]),
    "mvsim_view_slab_dev": (C.c_int, [_vp, _vp, _vp, _i64p, _vp, _i64p, _vp, C.c_int64, C.c_int64, _vp, C.POINTER(C.c_int64)]),
    "mvsim_comm_allreduce_sum_f64_dev": (C.c_int, [_vp, _vp, _vp]),
    "mvsim_host_copy": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "mvsim_comm_destroy": (C.c_int, [_vp]),
    "mvsim_group_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(_vp)]),
    "mvsim_group_destroy": (C.c_int, [_vp]),
    "mvsim_group_size": (C.c_int, [_vp]),
    "mvsim_group_ctx": (_vp, [_vp, C.c_int]),
    "mvsim_group_broadcast_volume": (C.c_int, [_vp, _vp, _i64p]),
    "mvsim_group_simulate_views": (C.c_int, [_vp, C.POINTER(_vp), _i64p, C.POINTER(ViewParams), C.c_int, C.POINTER(_vp)]),
    "mvsim_shard_views": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "mvsim_beads_random_points": (C.c_int, [C.POINTER(C.c_uint64), C.c_int64, _i64p, _i64p, C.POINTER(C.c_double)]),
    "mvsim_render_beads": (C.c_int, [_vp, C.POINTER(C.c_double), _i64p, C.c_int64, C.POINTER(C.c_double), C.c_int, _i64p, _i64p,
                                     C.POINTER(C.c_double), C.POINTER(_vp), C.POINTER(_vp)]),
    "mvsim_render_beads_dev": (C.c_int, [_vp, C.POINTER(C.c_double), _i64p, C.c_int64, C.POINTER(C.c_double), C.c_int, _i64p, _i64p,
                                         C.POINTER(C.c_double), C.POINTER(_vp), C.POINTER(_vp)]),
    "mvsim_beads_normalize": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvsim_beads_normalize_dev": (C.c_int, [_vp, _vp, C.c_int64]),
    "mvsim_perlin_init": (C.c_int, [C.POINTER(C.c_uint64), C.c_int32, _dp, C.POINTER(C.c_int32), _dp]),
    "mvsim_perlin_at": (C.c_int, [_vp, C.POINTER(Perlin), _vp, C.c_int64, _vp]),
    "mvsim_perlin_at_dev": (C.c_int, [_vp, C.POINTER(Perlin), _vp, C.c_int64, _vp]),
    "mvsim_perlin_raster": (C.c_int, [_vp, C.POINTER(Perlin), _i64p, _i64p, _vp]),
    "mvsim_perlin_raster_dev": (C.c_int, [_vp, C.POINTER(Perlin), _i64p, _i64p, _vp]),
    "mvsim_spheres_at": (C.c_int, [_vp, C.POINTER(SphereSet), _vp, C.c_int64, _vp]),
    "mvsim_spheres_at_dev": (C.c_int, [_vp, C.POINTER(SphereSet), _vp, C.c_int64, _vp]),
    "mvsim_spheres_raster": (C.c_int, [_vp, C.POINTER(SphereSet), _i64p, _i64p, C.c_int, _vp]),
    "mvsim_spheres_raster_dev": (C.c_int, [_vp, C.POINTER(SphereSet), _i64p, _i64p, C.c_int, _vp]),
    "mvsim_rejection_sample": (C.c_int, [_vp, C.POINTER(C.c_uint64), _dp, _dp, C.c_int64, C.POINTER(Density), C.c_int64, _dp,
                                         C.POINTER(C.c_int64)]),
    "mvsim_lightsheet_fit": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, _dp]),
    "mvsim_hessian_at": (C.c_int, [_vp, _vp, _i64p, _dp, C.c_int64, _dp, _dp, _dp]),
    "mvsim_hessian_at_dev": (C.c_int, [_vp, _vp, _i64p, _dp, C.c_int64, _dp, _dp, _dp]),
    "mvsim_hessian_images": (C.c_int, [_vp, _vp, _i64p, _vp, _vp]),
    "mvsim_hessian_images_dev": (C.c_int, [_vp, _vp, _i64p, _vp, _vp]),
    "mvsim_refract3d_ray_starts": (C.c_int, [_vp, C.POINTER(C.c_uint64), _i64p, C.c_int, C.c_int, _dp, C.c_int64, _dp, _dp]),
    "mvsim_camera_ray_starts": (C.c_int, [_vp, C.POINTER(C.c_uint64), _i64p, C.c_int, _dp]),
    "mvsim_refract3d": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int64,
                                  C.POINTER(C.c_uint64), _vp, _vp, C.POINTER(RaySteps)]),
    "mvsim_refract3d_dev": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int64,
                                      C.POINTER(C.c_uint64), _vp, _vp, C.POINTER(RaySteps)]),
    "mvsim_trace_params_default": (C.c_int, [_i64p, C.POINTER(TraceParams)]),
    "mvsim_trace_rays": (C.c_int, [_vp, _vp, _vp, _i64p, _dp, _dp, C.POINTER(C.c_float), C.c_int64, C.POINTER(TraceParams), _vp, _vp,
                                   C.POINTER(RaySteps), _dp, _dp, C.POINTER(C.c_int64)]),
    "mvsim_trace_rays_dev": (C.c_int, [_vp, _vp, _vp, _i64p, _dp, _dp, C.POINTER(C.c_float), C.c_int64, C.POINTER(TraceParams), _vp, _vp,
                                       C.POINTER(RaySteps), _dp, _dp, C.POINTER(C.c_int64)]),
    "mvsim_sandbox_ray_starts": (C.c_int, [_vp, C.POINTER(C.c_uint64), _i64p, C.c_int, C.c_int, C.c_int64, _dp, _dp]),
    "mvsim_grid_ray_starts": (C.c_int, [_vp, _i64p, C.c_int, C.c_int, C.c_int64, _dp, _dp, C.POINTER(C.c_int64)]),
    "mvsim_draw_simple_image": (C.c_int, [_vp, _vp, _i64p, C.c_float, C.c_float]),
    "mvsim_draw_simple_image_dev": (C.c_int, [_vp, _vp, _i64p, C.c_float, C.c_float]),
    "mvsim_hessian_plane": (C.c_int, [_vp, _vp, _i64p, C.c_int, _vp, _vp]),
    "mvsim_hessian_plane_dev": (C.c_int, [_vp, _vp, _i64p, C.c_int, _vp, _vp]),
    "mvsim_volume_inject": (C.c_int, [_vp, _vp, _vp, _i64p, _dp, _dp, _dp, C.c_int64, C.c_int]),
    "mvsim_volume_inject_dev": (C.c_int, [_vp, _vp, _vp, _i64p, _dp, _dp, _dp, C.c_int64, C.c_int]),
    "mvsim_volume_inject_info": (C.c_int, [_dp, C.POINTER(C.c_int32), _dp, C.POINTER(C.c_int32)]),
    "mvsim_volume_normalize": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp]),
    "mvsim_volume_normalize_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp]),
    "mvsim_volume_project": (C.c_int, [_vp, _vp, _vp, _i64p, _vp]),
    "mvsim_volume_project_dev": (C.c_int, [_vp, _vp, _vp, _i64p, _vp]),
    "mvsim_project_to_camera": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int, C.c_int, C.POINTER(C.c_uint64), _vp]),
    "mvsim_project_to_camera_dev": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int, C.c_int, C.POINTER(C.c_uint64), _vp]),
    "mvsim_ri_noise": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_uint64)]),
    "mvsim_ri_noise_dev": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_uint64)]),
    "mvsim_multi_spheres": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "mvsim_multi_spheres_dev": (C.c_int, [_vp, _vp, _vp, _i64p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "mvsim_sphere_walk_geometry": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "mvsim_decon_params_default": (None, [C.POINTER(DeconParams)]),
    "mvsim_decon_flip_psf": (C.c_int, [_vp, _i64p, _vp, _i64p]),
    "mvsim_decon_geometry": (C.c_int, [_i64p]),
    "mvsim_decon_ratio_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_float, _vp]),
    "mvsim_decon_update_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_float, C.c_double, C.POINTER(DeconStat)]),
    "mvsim_deconvolve_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i64p, C.c_int, _i64p,
                                       C.POINTER(DeconParams), _vp, C.POINTER(DeconStat)]),
    "mvsim_deconvolve": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i64p, C.c_int, _i64p,
                                   C.POINTER(DeconParams), _vp, C.POINTER(DeconStat)]),
    "mvsim_dog_params_default": (None, [C.POINTER(DogParams)]),
    "mvsim_dog_taps": (C.c_int, [C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "mvsim_dog_geometry": (C.c_int, [_i64p]),
    "mvsim_dog_dev": (C.c_int, [_vp, _vp, C.c_int, _i64p, C.POINTER(DogParams), _vp]),
    "mvsim_find_peaks_dev": (C.c_int, [_vp, _vp, _i64p, C.c_float, C.c_int64, _vp, _vp]),
    "mvsim_localise_peaks_dev": (C.c_int, [_vp, _vp, _i64p, _vp, _vp, C.c_int64, C.c_int, _vp]),
    "mvsim_detect_beads_dev": (C.c_int, [_vp, _vp, C.c_int, _i64p, C.POINTER(DogParams), C.c_int64, _vp, _vp]),
    "mvsim_detect_beads": (C.c_int, [_vp, _vp, C.c_int, _i64p, C.POINTER(DogParams), C.c_int64, _vp, _vp]),
    "mvsim_match_params_default": (None, [C.POINTER(MatchParams)]),
    "mvsim_match_geometry": (C.c_int, [C.c_int64, C.c_int64, C.c_int, _i64p]),
    "mvsim_descriptor_subsets": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "mvsim_fit_affine": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "mvsim_knn_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int, _vp, _vp]),
    "mvsim_bead_descriptors_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]),
    "mvsim_match_descriptors_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int64, C.c_int, C.c_double, C.c_int64, _vp, _vp]),
    "mvsim_ransac_affine_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, C.c_int64,
                                          C.POINTER(MatchParams), _vp, _vp]),
    "mvsim_register_beads_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(MatchParams),
                                           _vp, _vp, _vp]),
    "mvsim_register_beads": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int64, C.POINTER(MatchParams), _vp, _vp, _vp]),
    "mvsim_fuse_params_default": (None, [C.POINTER(FuseParams)]),
    "mvsim_fuse_invert": (C.c_int, [_dp, _dp, C.POINTER(C.c_int)]),
    "mvsim_fusion_bounds": (C.c_int, [_dp, _i64p, C.c_int, C.c_int, _i64p, _i64p]),
    "mvsim_fusion_psf_matrix": (C.c_int, [_dp, _i64p, _i64p, _dp]),
    "mvsim_fusion_geometry": (C.c_int, [_i64p]),
    "mvsim_fuse_views_dev": (C.c_int, [_vp, C.POINTER(FuseView), C.c_int, _i64p, _i64p, C.POINTER(FuseParams), _vp, _vp, _vp]),
    "mvsim_align_views_dev": (C.c_int, [_vp, C.POINTER(FuseView), C.c_int, _i64p, _i64p, C.POINTER(FuseParams), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mvsim_fuse_views": (C.c_int, [_vp, C.POINTER(FuseView), C.c_int, _i64p, _i64p, C.POINTER(FuseParams), _vp, _vp, _vp]),
    "mvsim_align_views": (C.c_int, [_vp, C.POINTER(FuseView), C.c_int, _i64p, _i64p, C.POINTER(FuseParams), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mvsim_psf_params_default": (None, [C.POINTER(PsfParams)]),
    "mvsim_psf_offsets": (C.c_int, [_vp, _i64p, _vp, C.POINTER(C.c_int)]),
    "mvsim_psf_select": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _i64p, C.POINTER(PsfParams), _vp, C.POINTER(PsfResult)]),
    "mvsim_psf_finish": (C.c_int, [_vp, C.POINTER(PsfParams), _vp, C.POINTER(PsfResult)]),
    "mvsim_psf_geometry": (C.c_int, [_i64p]),
    "mvsim_psf_select_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _i64p, C.POINTER(PsfParams), _vp, _vp]),
    "mvsim_psf_gather_dev": (C.c_int, [_vp, _vp, _i64p, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, C.POINTER(PsfParams), _vp]),
    "mvsim_psf_finish_dev": (C.c_int, [_vp, _vp, C.POINTER(PsfParams), _vp, _vp]),
    "mvsim_psf_use_from_matches_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, C.c_int, C.c_int64, _vp]),
    "mvsim_extract_psf_dev": (C.c_int, [_vp, _vp, _i64p, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, C.POINTER(PsfParams), _vp, _vp, _vp]),
    "mvsim_extract_psf": (C.c_int, [_vp, _vp, _i64p, _vp, C.c_int64, C.c_int64, _vp, _vp, C.POINTER(PsfParams), _vp, C.POINTER(PsfResult), _vp]),
}

_lib = None


def load():
    """Load libmvsim.so (built in-tree by ``build.py``).  Raises ImportError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError => the .so does not match include/mvsim.h
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    if status == MVSIM_OK:
        return
    msg = (load().mvsim_last_error() or b"").decode("utf-8", "replace")
    if status == MVSIM_EINVAL:
        raise ValueError(msg)             # Java side: IllegalArgumentException
    if status == MVSIM_ENOMEM:
        raise MemoryError(msg)            # Java side: OutOfMemoryError
    if status == MVSIM_ENODEV:
        raise MvsimNoDeviceError(status, msg)
    raise MvsimError(status, msg)
