"""ctypes binding of libphysicl_hip.so (include/physicl_hip.h) -- the only way Python reaches the GPU.

There is no CPU fallback: if the library is missing, or a call fails, this module raises.
"""
import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int32, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libphysicl_hip.so")

# enums of include/physicl_hip.h
R0, R1, R2, V0, V1, V2, DR0, DR1, DR2, DV0, DV1, DV2, E, NFIELDS = range(14)
FIELD_GROUPS = {"r": (R0, R1, R2), "v": (V0, V1, V2), "dr": (DR0, DR1, DR2), "dv": (DV0, DV1, DV2)}
SCATTER_WAVELENGTH, SCATTER_VARIABLE_N, FUSED_LAZY, SCATTER_PY_DV = 1, 2, 4, 8
RNG_INPUT, RNG_PHILOX = 0, 1
PHASE_ISOTROPIC, PHASE_DELETE = 0, 1
KIND_OBJECT, KIND_PHOTON = 0, 1
DTYPE_F64, DTYPE_F32 = 0, 1
_NP_DTYPE = {DTYPE_F64: np.float64, DTYPE_F32: np.float32}
CNT_N, CNT_XP, CNT_YP, CNT_ZP, CNT_PLANE0 = 0, 1, 2, 3, 4
MAX_PLANES = 12
SRC_ANGULAR = {"beam": 0, "isotropic": 1, "cone": 2, "lambertian": 3}       # PCL_SRC_BEAM ...
SRC_SPATIAL = {"point": 0, "disc": 1, "gaussian": 2}                         # PCL_SRC_POINT ...
GRID_COORDS = {"x": 0, "y": 1, "z": 2, "r": 3}                               # PCL_GRID_X ... PCL_GRID_RADIUS
GRID_MAX_AXES, GRID_MAX_BINS, GRID_MAX_CELLS = 3, 1024, 1 << 20
SHELL_MAX_SHELLS, SHELL_MAX_BINS, SHELL_MAX_CELLS = 16, 1024, 8192              # PCL_SHELL_MAX_SHELLS ...
DETECTOR_MAX_PIXELS, DETECTOR_MAX_BANDS, DETECTOR_MAX_CELLS = 1024, 1024, 1 << 20      # PCL_DETECTOR_MAX_PIXELS ...
SURFACE_MODES = {"lambertian": 0, "specular": 1}                             # PCL_SURFACE_LAMBERTIAN, PCL_SURFACE_SPECULAR
ABSORB_MAX_LAYERS, ABSORB_MAX_BINS, ABSORB_MAX_CELLS = 64, 1024, 12288           # PCL_ABSORB_MAX_LAYERS ...
PHASE_FUNCTIONS = {"isotropic": 0, "hg": 1, "rayleigh": 2}                   # PCL_PHASE_ISOTROPIC, PCL_PHASE_HG, PCL_PHASE_RAYLEIGH
PHASE_TABLE = 3                                                              # PCL_PHASE_TABLE: a law of pcl_step_phase_layered only
LPHASE_MAX_LAWS, LPHASE_MAX_LAYERS, LPHASE_MAX_NODES, LPHASE_MAX_TOTAL_NODES = 8, 64, 1024, 2048       # PCL_LPHASE_MAX_LAWS ...
RECYCLE_MAX_BINS = 1024                                                      # PCL_RECYCLE_MAX_BINS: bins of a RecycleStep's spectrum
PATH_ABSORB_MAX_LAYERS, PATH_ABSORB_MAX_BANDS, PATH_ABSORB_MAX_CELLS = 64, 1024, 4096          # PCL_PATH_ABSORB_MAX_LAYERS ...
REEMIT_MAX_LAYERS, REEMIT_MAX_BINS, REEMIT_MAX_TOTAL_BINS = 64, 1024, 2048                      # PCL_REEMIT_MAX_LAYERS ...
SPECTRAL_MAX_BANDS = 1024                                                    # PCL_SPECTRAL_MAX_BANDS: bands of a SpectralSurfaceStep
SCATTER_LAYERED_MAX_LAYERS, SCATTER_LAYERED_MAX_BANDS, SCATTER_LAYERED_MAX_CELLS = 64, 1024, 4096       # PCL_SCATTER_LAYERED_MAX_LAYERS ...
SCATTER_GRID_MAX_BANDS, SCATTER_GRID_MAX_CELLS = 1024, 1 << 20                # PCL_SCATTER_GRID_MAX_BANDS, PCL_SCATTER_GRID_MAX_CELLS
PHASE_GRID_MAX_MIXTURES, PHASE_GRID_MAX_CELLS, PHASE_GRID_ALONE, PHASE_GRID_LDS_BYTES = 64, 1 << 20, 255, 65536   # PCL_PHASE_GRID_MAX_MIXTURES ...
ABSORB_GRID_MAX_BANDS, ABSORB_GRID_MAX_CELLS, ABSORB_GRID_LDS_CELLS, ABSORB_GRID_LDS_BYTES = 1024, 1 << 20, 4096, 65536   # PCL_ABSORB_GRID_MAX_BANDS ...
PLANE_FLUX_AXES = {"x": 0, "y": 1, "z": 2}                                   # the normal; (u, v) are the remaining two in x, y, z order
PLANE_FLUX_MAX_LEVELS, PLANE_FLUX_MAX_BINS, PLANE_FLUX_MAX_BANDS, PLANE_FLUX_MAX_CELLS = 16, 1024, 1024, 1 << 20   # PCL_PLANE_FLUX_MAX_LEVELS ...
PLANE_FLUX_LDS_CELLS, PLANE_FLUX_LDS_BYTES = 4096, 65536                     # PCL_PLANE_FLUX_LDS_CELLS, PCL_PLANE_FLUX_LDS_BYTES
WALL_MODES = {None: 0, "periodic": 1, "mirror": 2, "open": 3}               # PCL_WALL_NONE, PCL_WALL_PERIODIC, PCL_WALL_MIRROR, PCL_WALL_OPEN
REEMIT_LAWS = {"isotropic": 0, "lambertian": 1}                              # the flags of pcl_step_reemit_parked's lambertian_host
PROF_NEWTON, PROF_SCATTER, PROF_DELETE_MASK, PROF_COMPACT, PROF_COUNTERS, PROF_FUSED, PROF_MULTI, PROF_ONEPASS, \
    PROF_DELETE_AHEAD = range(9)
PROF_NAMES = {PROF_NEWTON: "k_newton", PROF_SCATTER: "k_scatter", PROF_DELETE_MASK: "k_delete_mask",
              PROF_COMPACT: "k_compact", PROF_COUNTERS: "k_counters", PROF_FUSED: "k_fused", PROF_MULTI: "k_multi",
              PROF_ONEPASS: "k_delete_onepass", PROF_DELETE_AHEAD: "k_delete_ahead"}
ERR_NAMES = {-1: "PCL_ERR_HIP", -2: "PCL_ERR_ARG", -3: "PCL_ERR_STATE", -4: "PCL_ERR_RTC", -5: "PCL_ERR_EXPR",
             -6: "PCL_ERR_NOMEM"}


class HipError(RuntimeError):
    """A libphysicl_hip call returned a negative code; message is pcl_last_error()."""

    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "PCL_ERR"), code, msg))
        self.code = code


class ExpressionError(HipError, ValueError):
    """variable_n_fn was rejected (validator or hipRTC compile)."""


_dp = POINTER(c_double)
_vp = c_void_p

# name -> argtypes ; restype is always int except pcl_last_error
_PROTOTYPES = {
    "pcl_abi_version": [],
    "pcl_device_count": [POINTER(c_int)],
    "pcl_set_knob": [c_char_p, c_char_p],
    "pcl_comm_unique_id": [_vp],
    "pcl_comm_create": [_vp, c_char_p, c_int, c_int, POINTER(_vp)],
    "pcl_comm_allreduce_sum_i64": [_vp, _vp, c_int],
    "pcl_comm_info": [_vp, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int64)],
    "pcl_comm_destroy": [_vp],
    "pcl_store_last_multi_work": [_vp, POINTER(c_int64), POINTER(c_int64), POINTER(c_int), POINTER(c_int64)],
    "pcl_store_last_multi_clock": [_vp, POINTER(c_double)],
    "pcl_store_last_mixed_rows": [_vp, POINTER(c_int)],
    "pcl_store_ahead_clock": [_vp, POINTER(c_double)],
    "pcl_store_last_multi_hist": [_vp, _vp],
    "pcl_store_ahead_stats": [_vp, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)],
    "pcl_store_ahead_work": [_vp, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)],
    "pcl_store_alloc_info": [_vp, POINTER(c_int), POINTER(c_double), c_int, POINTER(c_double)],
    "pcl_ctx_set_rtc_background": [_vp, c_int],
    "pcl_ctx_rtc_wait": [_vp, POINTER(c_int)],
    "pcl_pool_trim": [POINTER(c_int64)],
    "pcl_pool_bytes": [POINTER(c_int64)],
    "pcl_pool_info": [POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int)],
    "pcl_ctx_create": [c_int, _vp, POINTER(_vp)],
    "pcl_ctx_destroy": [_vp],
    "pcl_ctx_sync": [_vp],
    "pcl_ctx_stream": [_vp, POINTER(_vp)],
    "pcl_ctx_device_info": [_vp, c_char_p, c_int, POINTER(c_int64), POINTER(c_int), POINTER(c_int)],
    "pcl_ctx_device_pci": [_vp, c_char_p, c_int],
    "pcl_ctx_mem_info": [_vp, POINTER(c_int64), POINTER(c_int64)],
    "pcl_dev_alloc": [_vp, c_int64, POINTER(_vp)],
    "pcl_dev_free": [_vp, _vp],
    "pcl_h2d": [_vp, _vp, _vp, c_int64],
    "pcl_d2h": [_vp, _vp, _vp, c_int64],
    "pcl_dev_memset": [_vp, _vp, c_int, c_int64],
    "pcl_prof_enable": [_vp, c_int],
    "pcl_prof_read": [_vp, c_int, POINTER(c_int64), POINTER(c_double), POINTER(c_double), POINTER(c_double)],
    "pcl_timer_start": [_vp],
    "pcl_timer_stop": [_vp, POINTER(c_double)],
    "pcl_k_light_scatter_step_del": [_vp, _vp, _vp, _vp, _vp, c_double, c_double, _vp, c_int64],
    "pcl_k_scatter_delete_test": [_vp, _vp, _vp, _vp, _vp, c_double, c_double, _vp, c_int64],
    "pcl_k_light_scatter_step_sphere": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, c_double, c_double, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, c_int64, c_int, c_double, c_double, c_char_p],
    "pcl_k_compact_indices": [_vp, _vp, c_int64, _vp, POINTER(c_int64)],
    "pcl_expr_validate": [c_char_p],
    "pcl_user_kernel_build": [_vp, c_char_p, c_char_p, c_char_p, POINTER(_vp)],
    "pcl_user_kernel_launch": [_vp, _vp, c_int64, _vp, c_int64],
    "pcl_user_kernel_free": [_vp, _vp],
    "pcl_store_alloc": [_vp, c_int64],
    "pcl_store_alloc_dtype": [_vp, c_int64, c_int],
    "pcl_store_dtype": [_vp, POINTER(c_int)],
    "pcl_store_free": [_vp],
    "pcl_store_capacity": [_vp, POINTER(c_int64)],
    "pcl_store_count": [_vp, POINTER(c_int64)],
    "pcl_store_set_count": [_vp, c_int64, c_int64],
    "pcl_store_slots": [_vp, POINTER(c_int64), POINTER(c_int)],
    "pcl_store_reserve_compaction": [_vp],
    "pcl_store_upload": [_vp, c_int, _vp, c_int64, c_int64],
    "pcl_store_download": [_vp, c_int, _vp, c_int64, c_int64],
    "pcl_store_upload_ids": [_vp, _vp, c_int64, c_int64],
    "pcl_store_download_ids": [_vp, _vp, c_int64, c_int64],
    "pcl_store_upload_kind": [_vp, _vp, c_int64, c_int64],
    "pcl_store_download_kind": [_vp, _vp, c_int64, c_int64],
    "pcl_store_field_ptr": [_vp, c_int, POINTER(_vp)],
    "pcl_store_layout": [_vp, POINTER(c_int64), POINTER(c_int64)],
    "pcl_store_upload_rand": [_vp, c_int, _vp, c_int64],
    "pcl_store_upload_rand3": [_vp, _vp, c_int64, c_int64],
    "pcl_store_fill_photons": [_vp, c_int64, c_int64, c_double, c_double, c_double, c_uint64],
    "pcl_store_fill_photons_table": [_vp, c_int64, c_int64, c_double, _vp, _vp, c_int, c_uint64],
    "pcl_store_apply_source": [_vp, _vp, c_double, c_uint64],
    "pcl_step_newton": [_vp, c_double],
    "pcl_step_scatter_isotropic": [_vp, c_double, c_double, c_int, c_double, c_double, c_char_p, c_int, c_uint64,
                                   c_uint32, POINTER(c_int64)],
    "pcl_step_fused_delete_multi": [_vp, c_double, c_int, c_double, c_double, c_uint64, c_uint32, _vp, c_int, _vp],
    "pcl_step_scatter_pcoll": [_vp, c_double, c_double, c_int, c_double, c_double, _vp],
    "pcl_step_delete_flags": [_vp, _vp, POINTER(c_int64), POINTER(c_int64)],
    "pcl_step_plane_energies": [_vp, _vp, _vp, c_int64, POINTER(c_int64)],
    "pcl_store_is_uniform": [_vp, POINTER(c_int)],
    "pcl_step_fused_multi": [_vp, c_double, c_int, c_double, c_double, c_int, c_double, c_double, c_char_p, c_uint64,
                             c_uint32, _vp, c_int, _vp],
    "pcl_step_fused": [_vp, c_double, c_int, c_double, c_double, c_int, c_double, c_double, c_char_p, c_int, c_uint64,
                       c_uint32, _vp, c_int, _vp],
    "pcl_step_mixed_multi": [_vp, c_double, c_int, c_int, _vp, c_double, c_double, c_int, c_double, c_double, c_char_p,
                             c_double, c_double, c_uint64, c_uint32, _vp, c_int, _vp],
    "pcl_store_trace_ahead": [_vp, _vp, c_int, c_double, c_int, c_int, _vp, c_int, c_double, c_double, c_int, c_double, c_double,
                              c_char_p, c_double, c_double, c_uint64, c_uint32, _vp],
    "pcl_store_trace_read": [_vp, _vp, c_int64],
    "pcl_step_fused_read": [_vp, c_int, _vp],
    "pcl_store_last_scatter_hits": [_vp, POINTER(c_int64)],
    "pcl_step_scatter_delete": [_vp, c_double, c_double, c_int, c_uint64, c_uint32, POINTER(c_int64),
                                POINTER(c_int64)],
    "pcl_step_fused_delete": [_vp, c_double, c_double, c_double, c_int, c_int, c_uint64, c_uint32, _vp, c_int, _vp],
    "pcl_store_last_delete_flags": [_vp, _vp, c_int64],
    "pcl_step_counters": [_vp, _vp, c_int, _vp],
    "pcl_step_plane_spectra": [_vp, _vp, c_int, _vp, c_int, _vp, _vp],
    "pcl_step_position_grid": [_vp, c_int, _vp, _vp, _vp, _vp, _vp],
    "pcl_step_shell_crossings": [_vp, c_int, _vp, _vp, _vp, c_int, _vp, c_int, _vp, _vp, _vp],
    "pcl_step_detector_image": [_vp, _vp, _vp, c_double, _vp, c_int, _vp, c_int, _vp, c_int, _vp, _vp],
    "pcl_step_surface_reflect": [_vp, c_double, _vp, c_double, c_int, c_double, c_uint64, c_uint32, _vp],
    "pcl_step_phase_redirect": [_vp, c_int, c_double, c_double, c_uint64, c_uint32, _vp],
    "pcl_step_absorb_scattered": [_vp, c_int, _vp, _vp, _vp, c_int, _vp, c_uint64, c_uint32, _vp, _vp],
    "pcl_step_phase_layered": [_vp, c_int, _vp, _vp, _vp, _vp, _vp, c_int, _vp, _vp, _vp, c_double, c_uint64, c_uint32, _vp],
    "pcl_step_recycle_spent": [_vp, _vp, c_double, c_int, c_double, _vp, c_int, _vp, _vp, c_uint64, c_uint32, _vp],
    "pcl_step_absorb_path": [_vp, c_int, c_int, _vp, _vp, _vp, _vp, c_uint64, c_uint32, _vp, _vp],
    "pcl_step_reemit_parked": [_vp, c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_double, c_uint64, c_uint32, _vp],
    "pcl_step_refract_surface": [_vp, c_double, _vp, c_double, c_double, c_int, c_double, c_uint64, c_uint32, _vp],
    "pcl_step_ground_spectral": [_vp, c_double, _vp, c_int, _vp, _vp, _vp, c_double, c_uint64, c_uint32, _vp, _vp],
    "pcl_step_scatter_layered": [_vp, c_int, c_int, _vp, _vp, _vp, _vp, c_int, c_double, c_uint64, c_uint32, _vp, _vp],
    "pcl_step_scatter_grid": [_vp, c_int, _vp, _vp, _vp, _vp, c_int, _vp, _vp, c_int, c_double, c_uint64, c_uint32, _vp, _vp],
    "pcl_step_box_walls": [_vp, _vp, _vp, _vp, _vp],
    "pcl_step_phase_grid": [_vp, c_int, _vp, _vp, _vp, _vp, _vp, c_int, _vp, c_int, _vp, _vp, _vp, _vp, _vp, c_int, c_double, c_uint64, c_uint32, _vp],
    "pcl_step_absorb_grid": [_vp, c_int, _vp, _vp, _vp, _vp, c_int, _vp, _vp, _vp, c_uint64, c_uint32, _vp, _vp],
    # device groups: several GPUs from one process (the C-level counterpart of physicl_amd.multidev.MultiDevice)
    "pcl_group_create": [c_int, POINTER(c_int), POINTER(_vp)],
    "pcl_group_destroy": [_vp],
    "pcl_group_size": [_vp, POINTER(c_int)],
    "pcl_group_ctx": [_vp, c_int, POINTER(_vp)],
    "pcl_group_shard": [_vp, c_int64, c_int, POINTER(c_int64), POINTER(c_int64)],
    "pcl_group_store_alloc": [_vp, c_int64, c_int],
    "pcl_group_store_dtype": [_vp, POINTER(c_int)],
    "pcl_group_fill_photons": [_vp, c_int64, c_int64, c_double, c_double, c_double, c_uint64],
    "pcl_group_count": [_vp, POINTER(c_int64)],
    "pcl_group_sync": [_vp],
    "pcl_group_reserve_compaction": [_vp],
    "pcl_group_step_fused": [_vp, c_double, c_int, c_double, c_double, c_int, c_double, c_double, c_char_p, c_int, c_uint64,
                             c_uint32, _vp, c_int, _vp],
    "pcl_group_step_fused_delete": [_vp, c_double, c_double, c_double, c_int, c_int, c_uint64, c_uint32, _vp, c_int, _vp],
    "pcl_group_step_fused_multi": [_vp, c_double, c_int, c_double, c_double, c_int, c_double, c_double, c_char_p, c_uint64,
                                   c_uint32, _vp, c_int, _vp],
    "pcl_group_step_fused_delete_multi": [_vp, c_double, c_int, c_double, c_double, c_uint64, c_uint32, _vp, c_int, _vp],
    "pcl_group_step_mixed_multi": [_vp, c_double, c_int, c_int, _vp, c_double, c_double, c_int, c_double, c_double, c_char_p,
                                   c_double, c_double, c_uint64, c_uint32, _vp, c_int, _vp],
    "pcl_group_download": [_vp, c_int, _vp, c_int64, c_int64],
    "pcl_group_download_ids": [_vp, _vp, c_int64, c_int64],
    "pcl_group_step_plane_spectra": [_vp, _vp, c_int, _vp, c_int, _vp, _vp],
    "pcl_group_apply_source": [_vp, _vp, c_double, c_uint64],
    "pcl_group_step_position_grid": [_vp, c_int, _vp, _vp, _vp, _vp, _vp],
    "pcl_group_step_shell_crossings": [_vp, c_int, _vp, _vp, _vp, c_int, _vp, c_int, _vp, _vp, _vp],
    "pcl_group_step_detector_image": [_vp, _vp, _vp, c_double, _vp, c_int, _vp, c_int, _vp, c_int, _vp, _vp],
    "pcl_group_step_surface_reflect": [_vp, c_double, _vp, c_double, c_int, c_double, c_uint64, c_uint32, _vp],
    "pcl_group_step_phase_redirect": [_vp, c_int, c_double, c_double, c_uint64, c_uint32, _vp],
    "pcl_group_step_absorb_scattered": [_vp, c_int, _vp, _vp, _vp, c_int, _vp, c_uint64, c_uint32, _vp, _vp],
    "pcl_group_step_phase_layered": [_vp, c_int, _vp, _vp, _vp, _vp, _vp, c_int, _vp, _vp, _vp, c_double, c_uint64, c_uint32, _vp],
    "pcl_group_step_recycle_spent": [_vp, _vp, c_double, c_int, c_double, _vp, c_int, _vp, _vp, c_uint64, c_uint32, _vp],
    "pcl_group_step_absorb_path": [_vp, c_int, c_int, _vp, _vp, _vp, _vp, c_uint64, c_uint32, _vp, _vp],
    "pcl_group_step_reemit_parked": [_vp, c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_double, c_uint64, c_uint32, _vp],
    "pcl_group_step_refract_surface": [_vp, c_double, _vp, c_double, c_double, c_int, c_double, c_uint64, c_uint32, _vp],
    "pcl_group_step_ground_spectral": [_vp, c_double, _vp, c_int, _vp, _vp, _vp, c_double, c_uint64, c_uint32, _vp, _vp],
    "pcl_group_step_scatter_layered": [_vp, c_int, c_int, _vp, _vp, _vp, _vp, c_int, c_double, c_uint64, c_uint32, _vp, _vp],
    "pcl_group_step_scatter_grid": [_vp, c_int, _vp, _vp, _vp, _vp, c_int, _vp, _vp, c_int, c_double, c_uint64, c_uint32, _vp, _vp],
    "pcl_group_step_box_walls": [_vp, _vp, _vp, _vp, _vp],
    "pcl_group_step_phase_grid": [_vp, c_int, _vp, _vp, _vp, _vp, _vp, c_int, _vp, c_int, _vp, _vp, _vp, _vp, _vp, c_int, c_double, c_uint64,
                                  c_uint32, _vp],
    "pcl_group_step_absorb_grid": [_vp, c_int, _vp, _vp, _vp, _vp, c_int, _vp, _vp, _vp, c_uint64, c_uint32, _vp, _vp],
    "pcl_step_plane_flux": [_vp, c_int, c_int, _vp, _vp, c_int, _vp, c_int, _vp, c_int, _vp, _vp],
    "pcl_group_step_plane_flux": [_vp, c_int, c_int, _vp, _vp, c_int, _vp, c_int, _vp, c_int, _vp, _vp],
}
EXPORTS = sorted(list(_PROTOTYPES) + ["pcl_last_error"])

_lib = None


def load():
    """dlopen libphysicl_hip.so (built by ``python -m physicl_amd.build``).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "physicl_amd: %s is missing -- build it with `python -m physicl_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = c_int
    lib.pcl_last_error.argtypes = []
    lib.pcl_last_error.restype = c_char_p
    if lib.pcl_abi_version() != 1:
        raise ImportError("libphysicl_hip ABI version %d, expected 1" % lib.pcl_abi_version())
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = (_lib.pcl_last_error() or b"").decode("utf-8", "replace")
        raise (ExpressionError if rc in (-4, -5) else HipError)(rc, msg)


def set_knob(name, value=None):
    """An A/B switch of the library (pcl_set_knob): ``value`` = its text, None = back to the environment variable."""
    check(load().pcl_set_knob(name.encode(), None if value is None else str(value).encode()))


def device_count():
    n = c_int(0)
    rc = load().pcl_device_count(byref(n))
    return n.value if rc == 0 else 0


def pool_bytes():
    """Bytes of freed device blocks the library keeps for the next store of this process (PCL_POOL_GB bounds it)."""
    n = c_int64(0)
    check(load().pcl_pool_bytes(byref(n)))
    return n.value


def pool_info():
    """{'idle_blocks', 'idle_handles', 'parked_va', 'remaps_avoided', 'vmm_on'} (pcl_pool_info)."""
    a, b, c, d, e = c_int64(0), c_int64(0), c_int64(0), c_int64(0), c_int(0)
    check(load().pcl_pool_info(byref(a), byref(b), byref(c), byref(d), byref(e)))
    return {"idle_blocks": a.value, "idle_handles": b.value, "parked_va": c.value, "remaps_avoided": d.value, "vmm_on": bool(e.value)}


def pool_trim():
    """Hand every idle block back to the driver; returns the bytes released."""
    n = c_int64(0)
    check(load().pcl_pool_trim(byref(n)))
    return n.value


def validate_expr(expr):
    lib = load()
    rc = lib.pcl_expr_validate(expr.encode())
    if rc != 0:
        raise ExpressionError(rc, lib.pcl_last_error().decode())


def _host(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(c_void_p)


# ---------------------------------------------------------------- what every fused step takes and answers
# A counter row, one per light step per pass: int64 [N, sign x 3, planes ..., hits | removed].  This is the one layout; the
# host layer (physicl_amd/core.py) reads rows through _split_rows and knows no column numbers of its own.
_EVENT = -1               # the last column; CNT_N .. CNT_PLANE0 above name the others
_PHASES = {"iso": PHASE_ISOTROPIC, "delete": PHASE_DELETE}


def _split_rows(rows):
    """(N, sign x 3, planes, hits | removed) of one counter row or of a block of them: views of ``rows``."""
    return rows[..., CNT_N], rows[..., CNT_XP:CNT_PLANE0], rows[..., CNT_PLANE0:_EVENT], rows[..., _EVENT]


def _row_dict(row, event):
    """A counter row in its dict form (arrays of its own); ``event`` names the last column ("hits" / "removed")."""
    n, sign, planes, last = _split_rows(row)
    return {"N": int(n), "sign": sign.copy(), "planes": planes.copy(), event: int(last)}


def _planes(planes, off=False):
    """Measure planes -> (the float64 array the caller keeps alive over the call, its address or None, n_planes).  A ready
    array (C-contiguous, 2-D, float64: a loop hands the same one over every body) is taken as it is; no planes are a NULL
    pointer; ``None`` means "counters off" (n_planes = -1) where the entry point has that (``off``)."""
    if planes is None and off:
        return None, None, -1
    if type(planes) is np.ndarray and planes.dtype == np.float64 and planes.ndim == 2 and planes.flags.c_contiguous:
        pl = planes
    else:
        pl = np.ascontiguousarray(np.asarray(planes, dtype=np.float64).reshape(-1, 3))
    return pl, (pl.ctypes.data if len(pl) else None), len(pl)


def _spectra(entry, handle, planes, edges):
    """One call of pcl_step_plane_spectra / pcl_group_step_plane_spectra: (counts int64[P], hist int64[P, B])."""
    pl, pp, npl = _planes(planes)
    ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    n_bins = len(ed) - 1
    counts, hist = np.zeros(npl, dtype=np.int64), np.zeros((npl, max(n_bins, 0)), dtype=np.int64)
    check(entry(handle, pp, npl, ed.ctypes.data, n_bins, counts.ctypes.data, hist.ctypes.data))
    return counts, hist


def _grid(entry, handle, axes, edges, center=None):
    """One call of pcl_step_position_grid / pcl_group_step_position_grid: the int64 grid of shape (bins of axis 0, ...).
    ``axes``: "x", "y", "z", "r" (or the header's numbers), ``edges``: one sequence of edges per axis."""
    coords = np.array([GRID_COORDS.get(a, a) for a in axes], dtype=np.int32)
    per_axis = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
    if len(per_axis) != len(coords):
        raise ValueError("one sequence of edges per axis: %d axes, %d sequences" % (len(coords), len(per_axis)))
    n_bins = np.array([len(e) - 1 for e in per_axis], dtype=np.int32)
    ed = np.ascontiguousarray(np.concatenate(per_axis)) if per_axis else np.zeros(0)
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    out = np.zeros([max(int(b), 0) for b in n_bins], dtype=np.int64)
    check(entry(handle, len(coords), coords.ctypes.data, n_bins.ctypes.data, ed.ctypes.data, None if ce is None else ce.ctypes.data,
                out.ctypes.data))
    return out


def _shells(entry, handle, radii, center=None, E_edges=None, mu_edges=None):
    """One call of pcl_step_shell_crossings / pcl_group_step_shell_crossings: (counts int64[2, S], E_hist int64[2, S, B_E] or
    None, mu_hist int64[2, S, B_mu] or None) -- [0]: outward, [1]: inward.  The edges go over as given: the library makes
    R*R and the signed squares of the direction edges."""
    ra = np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    S = len(ra)
    counts = np.zeros((2, S), dtype=np.int64)
    edges, hists = [], []
    for e in (E_edges, mu_edges):
        ed = None if e is None else np.ascontiguousarray(e, dtype=np.float64).reshape(-1)
        edges.append(ed)
        hists.append(None if ed is None else np.zeros((2, S, max(len(ed) - 1, 0)), dtype=np.int64))
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    nb = lambda e: 0 if e is None else len(e) - 1                                                              # noqa: E731
    check(entry(handle, S, ra.ctypes.data, ptr(ce), ptr(edges[0]), nb(edges[0]), ptr(edges[1]), nb(edges[1]), counts.ctypes.data,
                ptr(hists[0]), ptr(hists[1])))
    return counts, hists[0], hists[1]


def _detector(entry, handle, position, frame, radius, x_edges, y_edges, E_edges=None):
    """One call of pcl_step_detector_image / pcl_group_step_detector_image: (counts int64[2] = [through, seen], image
    int64[max(bands, 1), ny, nx]).  ``frame``: e1, e2, n as nine numbers ((3, 3), a row each); the edges go over as given."""
    po = np.ascontiguousarray(position, dtype=np.float64).reshape(3)
    fr = np.ascontiguousarray(frame, dtype=np.float64).reshape(9)
    xe, ye = (np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in (x_edges, y_edges))
    ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    nx, ny, nE = len(xe) - 1, len(ye) - 1, 0 if ee is None else len(ee) - 1
    counts = np.zeros(2, dtype=np.int64)
    image = np.zeros((max(nE, 1), max(ny, 0), max(nx, 0)), dtype=np.int64)
    check(entry(handle, po.ctypes.data, fr.ctypes.data, float(radius), xe.ctypes.data, nx, ye.ctypes.data, ny,
                None if ee is None else ee.ctypes.data, nE, counts.ctypes.data, image.ctypes.data))
    return counts, image


def _surface(entry, handle, radius, center, albedo, mode, c, seed, n_pass):
    """One call of pcl_step_surface_reflect / pcl_group_step_surface_reflect: (reflected, absorbed) of this call.  ``mode``:
    "lambertian", "specular" or the header's numbers; ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2, dtype=np.int64)
    check(entry(handle, float(radius), None if ce is None else ce.ctypes.data, float(albedo), int(SURFACE_MODES.get(mode, mode)),
                float(c), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data))
    return int(counts[0]), int(counts[1])


def _phase(entry, handle, phase, g, c, seed, n_pass):
    """One call of pcl_step_phase_redirect / pcl_group_step_phase_redirect: the photons re-directed by this call.  ``phase``:
    "isotropic", "hg", "rayleigh" or the header's numbers; ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    count = np.zeros(1, dtype=np.int64)
    check(entry(handle, int(PHASE_FUNCTIONS.get(phase, phase)), float(g), float(c), int(seed) & 0xFFFFFFFFFFFFFFFF,
                int(n_pass) & 0xFFFFFFFF, count.ctypes.data))
    return int(count[0])


def _absorb(entry, handle, omega0, edges, center, E_edges, seed, n_pass):
    """One call of pcl_step_absorb_scattered / pcl_group_step_absorb_scattered: (interacted, absorbed, absorbed_by_layer int64[L'],
    E_hist int64[L', B_E] or None).  ``omega0``: one number with ``edges=None``, else one per layer; the edges go over as given
    (the library squares them); ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    om = np.ascontiguousarray(omega0, dtype=np.float64).reshape(-1)
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    L = 0 if ed is None else len(ed) - 1
    rows = max(L, 1)
    if len(om) != rows:
        raise ValueError("omega0 holds %d values for %d layers" % (len(om), rows))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    Ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    nE = 0 if Ee is None else len(Ee) - 1
    counts = np.zeros(2 + rows, dtype=np.int64)
    hist = None if Ee is None else np.zeros((rows, max(nE, 0)), dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, L, om.ctypes.data, ptr(ed), ptr(ce), nE, ptr(Ee), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF,
                counts.ctypes.data, ptr(hist)))
    return int(counts[0]), int(counts[1]), counts[2:].copy(), hist


def _law_arrays(laws):
    """(kinds int32[M], g float64[M], n_bins int32[M], mu, F) of a sequence of ``(kind, g, mu, F)`` laws as pcl_step_phase_layered and
    pcl_step_phase_grid take them: the tables' nodes and cumulative values one behind the other (None without a table)."""
    kinds = np.array([int(PHASE_TABLE if k == "table" else PHASE_FUNCTIONS.get(k, k)) for k, _, _, _ in laws], dtype=np.int32)
    g = np.array([float(x) for _, x, _, _ in laws], dtype=np.float64)
    tabs = [(np.ascontiguousarray(m, dtype=np.float64).reshape(-1), np.ascontiguousarray(f, dtype=np.float64).reshape(-1))
            for _, _, m, f in laws if m is not None]
    if any(len(m) != len(f) for m, f in tabs):
        raise ValueError("a table's mu and F must hold the same number of nodes")
    n_bins = np.zeros(len(laws), dtype=np.int32)
    n_bins[[j for j, law in enumerate(laws) if law[2] is not None]] = [len(m) - 1 for m, _ in tabs]
    mu = np.concatenate([m for m, _ in tabs]) if tabs else None
    F = np.concatenate([f for _, f in tabs]) if tabs else None
    return kinds, g, n_bins, mu, F


def _phase_layered(entry, handle, laws, cum, edges, center, c, seed, n_pass):
    """One call of pcl_step_phase_layered / pcl_group_step_phase_layered: (scattered, redirected, by_layer int64[L'], by_law
    int64[M]).  ``laws``: a sequence of ``(kind, g, mu, F)`` -- kind "isotropic", "hg", "rayleigh", "table" or the header's numbers,
    ``mu`` and ``F`` the K + 1 nodes and cumulative values of a table (None otherwise); ``cum``: the cumulative weights, one row
    of M per layer; the edges go over as given (the library squares them, and makes the tables' slopes); ``n_pass``: the caller's
    own pass counter (a Philox counter word)."""
    M = len(laws)
    kinds, g, n_bins, mu, F = _law_arrays(laws)
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    L = 0 if ed is None else len(ed) - 1
    rows = max(L, 1)
    cu = np.ascontiguousarray(cum, dtype=np.float64).reshape(-1)
    if len(cu) != rows * M:
        raise ValueError("cum holds %d values for %d layers of %d laws" % (len(cu), rows, M))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2 + rows + M, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, M, kinds.ctypes.data, g.ctypes.data, n_bins.ctypes.data, ptr(mu), ptr(F), L, cu.ctypes.data, ptr(ed), ptr(ce),
                float(c), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data))
    return int(counts[0]), int(counts[1]), counts[2:2 + rows].copy(), counts[2 + rows:].copy()


class SourceStruct(ctypes.Structure):
    """``pcl_source`` of include/physicl_hip.h."""
    _fields_ = [("origin", c_double * 3), ("e1", c_double * 3), ("e2", c_double * 3), ("d", c_double * 3),
                ("angular", c_int), ("spatial", c_int), ("cos_half_angle", c_double), ("radius", c_double)]


def _source_struct(src):
    """``pcl_source`` of a light.PhotonSource, or of anything with its attributes (origin, e1, e2, d: three numbers each;
    angular, spatial: names or the header's numbers; cos_half_angle, radius)."""
    vec = lambda a: (c_double * 3)(*[float(x) for x in a])                                                     # noqa: E731
    return SourceStruct(vec(src.origin), vec(src.e1), vec(src.e2), vec(src.d), int(SRC_ANGULAR.get(src.angular, src.angular)),
                        int(SRC_SPATIAL.get(src.spatial, src.spatial)), float(src.cos_half_angle), float(src.radius))


def _source(entry, handle, src, c, seed):
    """One call of pcl_store_apply_source / pcl_group_apply_source.  ``src``: what ``_source_struct`` takes."""
    st = _source_struct(src)
    check(entry(handle, ctypes.addressof(st), float(c), int(seed)))


def _recycle(entry, handle, src, c, at_rest, top, center, spectrum, seed, n_pass):
    """One call of pcl_step_recycle_spent / pcl_group_step_recycle_spent: (at_rest, escaped) of this call.  ``src``: what
    ``_source_struct`` takes; ``top``: None or a radius about ``center``; ``spectrum``: None or ``(grid, cdf)``; ``n_pass``: the
    caller's own pass counter (a Philox counter word)."""
    st = _source_struct(src)
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    grid = cdf = None
    if spectrum is not None:
        grid, cdf = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in spectrum)
        if len(grid) != len(cdf):
            raise ValueError("spectrum: grid and cdf must hold the same number of values")
    counts = np.zeros(2, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, ctypes.addressof(st), float(c), int(bool(at_rest)), 0.0 if top is None else float(top), ptr(ce),
                0 if cdf is None else len(cdf), ptr(cdf), ptr(grid), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF,
                counts.ctypes.data))
    return int(counts[0]), int(counts[1])


def _absorb_path(entry, handle, p, edges, center, E_edges, seed, n_pass):
    """One call of pcl_step_absorb_path / pcl_group_step_absorb_path: (exposed, absorbed, absorbed_by_cell int64[L', B']).  ``p``: the
    probability of absorption per pass, L' = max(layers, 1) rows of B' = max(bands, 1) values (any shape of that size); the edges go
    over as given (the library squares the radii); ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    pr = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    Ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    L, B = (0 if e is None else len(e) - 1 for e in (ed, Ee))
    rows, cols = max(L, 1), max(B, 1)
    if len(pr) != rows * cols:
        raise ValueError("p holds %d values for %d layers of %d bands" % (len(pr), rows, cols))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2, dtype=np.int64)
    cells = np.zeros((rows, cols), dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, L, B, pr.ctypes.data, ptr(ed), ptr(ce), ptr(Ee), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF,
                counts.ctypes.data, cells.ctypes.data))
    return int(counts[0]), int(counts[1]), cells


def _reemit(entry, handle, eta, angular, tables, edges, center, c, seed, n_pass):
    """One call of pcl_step_reemit_parked / pcl_group_step_reemit_parked: (parked, reemitted, by_layer int64[L']).  ``eta`` and
    ``angular`` ("isotropic", "lambertian" or the header's flags): one value, or one per layer of ``edges``; ``tables``: None, or per
    layer None or ``(grid, cdf)``; the edges go over as given (the library squares them); ``n_pass``: the caller's own pass counter (a
    Philox counter word)."""
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    L = 0 if ed is None else len(ed) - 1
    rows = max(L, 1)
    et = np.asarray(eta, dtype=np.float64).reshape(-1)
    et = np.ascontiguousarray(np.repeat(et, rows) if len(et) == 1 else et)
    laws = [angular] * rows if isinstance(angular, (str, int, np.integer)) else list(angular)
    tabs = [None] * rows if tables is None else list(tables)
    if not len(et) == len(laws) == len(tabs) == rows:
        raise ValueError("eta, angular and tables hold %d, %d and %d values for %d layers" % (len(et), len(laws), len(tabs), rows))
    lam = np.array([int(REEMIT_LAWS.get(a, a)) for a in laws], dtype=np.int32)
    tabs = [None if t is None else tuple(np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in t) for t in tabs]
    if any(t is not None and len(t[0]) != len(t[1]) for t in tabs):
        raise ValueError("a table's grid and cdf must hold the same number of values")
    off = np.concatenate([[0], np.cumsum([0 if t is None else len(t[1]) for t in tabs])]).astype(np.int32)
    grid = np.concatenate([t[0] for t in tabs if t is not None]) if off[-1] else None
    cdf = np.concatenate([t[1] for t in tabs if t is not None]) if off[-1] else None
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2 + rows, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, L, ptr(ed), ptr(ce), et.ctypes.data, lam.ctypes.data, off.ctypes.data, ptr(cdf), ptr(grid), float(c),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data))
    return int(counts[0]), int(counts[1]), counts[2:].copy()


def _refract(entry, handle, radius, center, n_inside, n_outside, fresnel, c, seed, n_pass):
    """One call of pcl_step_refract_surface / pcl_group_step_refract_surface: int64[6] -- in refracted, in reflected, out refracted,
    out reflected, out total, overshot -- of this call.  ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(6, dtype=np.int64)
    check(entry(handle, float(radius), None if ce is None else ce.ctypes.data, float(n_inside), float(n_outside), int(bool(fresnel)),
                float(c), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data))
    return counts


def _ground_spectral(entry, handle, radius, center, E_edges, albedo, specular, c, seed, n_pass):
    """One call of pcl_step_ground_spectral / pcl_group_step_ground_spectral: (counts int64[4] -- reflected, absorbed, mirrored,
    out_of_band --, reflected_by_band int64[B], absorbed_by_band int64[B]) of this call.  ``albedo``: one value per band of ``E_edges``;
    ``specular``: one value for every band, or one per band; ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    Ee = np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    B = len(Ee) - 1
    al = np.ascontiguousarray(albedo, dtype=np.float64).reshape(-1)
    sp = np.asarray(specular, dtype=np.float64).reshape(-1)
    sp = np.ascontiguousarray(np.repeat(sp, B) if len(sp) == 1 else sp)
    if not len(al) == len(sp) == B:
        raise ValueError("albedo and specular hold %d and %d values for %d bands" % (len(al), len(sp), B))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(4, dtype=np.int64)
    bands = np.zeros((2, max(B, 1)), dtype=np.int64)
    check(entry(handle, float(radius), None if ce is None else ce.ctypes.data, B, Ee.ctypes.data, al.ctypes.data, sp.ctypes.data, float(c),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data, bands.ctypes.data))
    return counts, bands[0].copy(), bands[1].copy()


def _scatter_layered(entry, handle, p, edges, center, E_edges, first, c, seed, n_pass):
    """One call of pcl_step_scatter_layered / pcl_group_step_scatter_layered: (exposed, scattered, scattered_by_cell int64[L', B']).
    ``p``: the probability of scattering per pass, L' = max(layers, 1) rows of B' = max(bands, 1) values (any shape of that size); the
    edges go over as given (the library squares the radii); ``first``: the pass's first scatterer (a miss gets dv = 0) or not (a miss
    is not written); ``n_pass``: the caller's own pass counter (a Philox counter word)."""
    pr = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    Ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    L, B = (0 if e is None else len(e) - 1 for e in (ed, Ee))
    rows, cols = max(L, 1), max(B, 1)
    if len(pr) != rows * cols:
        raise ValueError("p holds %d values for %d layers of %d bands" % (len(pr), rows, cols))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2, dtype=np.int64)
    cells = np.zeros((rows, cols), dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, L, B, pr.ctypes.data, ptr(ed), ptr(ce), ptr(Ee), int(bool(first)), float(c), int(seed) & 0xFFFFFFFFFFFFFFFF,
                int(n_pass) & 0xFFFFFFFF, counts.ctypes.data, cells.ctypes.data))
    return int(counts[0]), int(counts[1]), cells


def _scatter_grid(entry, handle, p, axes, edges, center, E_edges, first, c, seed, n_pass):
    """One call of pcl_step_scatter_grid / pcl_group_step_scatter_grid: (exposed, scattered, scattered_by_cell int64 of the grid's shape,
    with a last dimension of B bands if ``E_edges`` is given).  ``p``: the probability of scattering per pass, one value per cell (and
    band), row-major in the order of ``axes`` (any shape of that size); ``axes``, ``edges``, ``center``: as for ``_grid`` (the library
    squares the edges of a radius axis); ``first``: the pass's first scatterer (a miss gets dv = 0) or not (a miss is not written);
    ``n_pass``: the caller's own pass counter (a Philox counter word).  The table goes up and the tallies come back with every call."""
    coords = np.array([GRID_COORDS.get(a, a) for a in axes], dtype=np.int32)
    per_axis = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
    if len(per_axis) != len(coords):
        raise ValueError("one sequence of edges per axis: %d axes, %d sequences" % (len(coords), len(per_axis)))
    n_bins = np.array([len(e) - 1 for e in per_axis], dtype=np.int32)
    ed = np.ascontiguousarray(np.concatenate(per_axis)) if per_axis else np.zeros(0)
    Ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    B = 0 if Ee is None else len(Ee) - 1
    shape = [max(int(b), 0) for b in n_bins] + ([B] if Ee is not None else [])
    pr = np.ascontiguousarray(p, dtype=np.float64).reshape(-1)
    if len(pr) != int(np.prod(shape)):
        raise ValueError("p holds %d values for a grid of shape %r" % (len(pr), tuple(shape)))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2, dtype=np.int64)
    cells = np.zeros(shape, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, len(coords), coords.ctypes.data, n_bins.ctypes.data, ed.ctypes.data, ptr(ce), B, ptr(Ee), pr.ctypes.data,
                int(bool(first)), float(c), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data, cells.ctypes.data))
    return int(counts[0]), int(counts[1]), cells


def _box_walls(entry, handle, modes, lo, hi):
    """One call of pcl_step_box_walls / pcl_group_step_box_walls: int64[8] -- moving, multi, crossed[3][2] (axis-major: below, above) --
    of this call.  ``modes``: three of ``WALL_MODES``' keys or values, for x, y, z; ``lo``, ``hi``: three numbers each (those of an axis
    without a wall are not read)."""
    md = np.array([WALL_MODES.get(m, m) if m is None or isinstance(m, str) else m for m in modes], dtype=np.int32).reshape(3)
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(3)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(3)
    counts = np.zeros(8, dtype=np.int64)
    check(entry(handle, md.ctypes.data, lo.ctypes.data, hi.ctypes.data, counts.ctypes.data))
    return counts


def phase_grid_lds_bytes(n_mixtures, n_laws, n_edges, n_nodes):
    """The LDS a pcl_step_phase_grid call asks for, by the header's formula: K mixtures of M laws, E edges over all axes, T nodes over
    all tables.  At most ``PHASE_GRID_LDS_BYTES``."""
    K, M = int(n_mixtures), int(n_laws)
    return 8 * (K * M + int(n_edges) + M + 3 * int(n_nodes) + (3 * M + 1) // 2) + 4 * (2 + K + M)


def _phase_grid(entry, handle, laws, cum, axes, edges, center, mixture, outside, c, seed, n_pass):
    """One call of pcl_step_phase_grid / pcl_group_step_phase_grid: (scattered, redirected, by_mixture int64[K], by_law int64[M]).
    ``laws``: as for ``_phase_layered``; ``cum``: the cumulative weights, one row of M per mixture; ``axes``, ``edges``, ``center``: as
    for ``_grid`` (the library squares the edges of a radius axis); ``mixture``: one integer per cell, row-major in the order of
    ``axes`` (any shape of that size) -- a row of ``cum``, or -1 (``PHASE_GRID_ALONE`` as the byte that goes over) for a cell whose
    photons are left alone; ``outside``: the row of a scattered photon in no cell, None for none; ``n_pass``: the caller's own pass
    counter (a Philox counter word).  The map goes up with every call, one byte a cell."""
    M = len(laws)
    kinds, g, n_tab, mu, F = _law_arrays(laws)
    cu = np.ascontiguousarray(cum, dtype=np.float64).reshape(-1)
    if M < 1 or len(cu) % M or not len(cu):
        raise ValueError("cum holds %d values for mixtures of %d laws" % (len(cu), M))
    K = len(cu) // M
    coords = np.array([GRID_COORDS.get(a, a) for a in axes], dtype=np.int32)
    per_axis = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
    if len(per_axis) != len(coords):
        raise ValueError("one sequence of edges per axis: %d axes, %d sequences" % (len(coords), len(per_axis)))
    n_bins = np.array([len(e) - 1 for e in per_axis], dtype=np.int32)
    ed = np.ascontiguousarray(np.concatenate(per_axis)) if per_axis else np.zeros(0)
    mx = np.asarray(mixture).reshape(-1)
    if len(mx) != int(np.prod([max(int(b), 0) for b in n_bins])):
        raise ValueError("mixture holds %d values for a grid of shape %r" % (len(mx), tuple(int(b) for b in n_bins)))
    if not np.all((mx >= -1) & (mx < PHASE_GRID_ALONE)):
        raise ValueError("mixture must hold rows of cum or -1")
    mp = np.ascontiguousarray(np.where(mx < 0, PHASE_GRID_ALONE, mx), dtype=np.uint8)
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(2 + K + M, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, M, kinds.ctypes.data, g.ctypes.data, n_tab.ctypes.data, ptr(mu), ptr(F), K, cu.ctypes.data, len(coords),
                coords.ctypes.data, n_bins.ctypes.data, ed.ctypes.data, ptr(ce), mp.ctypes.data, -1 if outside is None else int(outside),
                float(c), int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data))
    return int(counts[0]), int(counts[1]), counts[2:2 + K].copy(), counts[2 + K:].copy()


def absorb_grid_lds_bytes(n_tables, n_edges, n_cells):
    """The LDS the LDS form of a pcl_step_absorb_grid call asks for, by the header's formula: t tables (1 or 2), E edges over all axes
    and the bands, C cells of the grid times bands."""
    return 8 * int(n_edges) + 8 * int(n_tables) * int(n_cells) + 4 * (4 + int(n_cells))


def absorb_grid_lds_form(n_tables, n_edges, n_cells):
    """Whether a pcl_step_absorb_grid call keeps its tables and tallies in LDS (the header's bound) or in device memory."""
    return n_cells <= ABSORB_GRID_LDS_CELLS and absorb_grid_lds_bytes(n_tables, n_edges, n_cells) <= ABSORB_GRID_LDS_BYTES


def _absorb_grid(entry, handle, p, omega0, axes, edges, center, E_edges, seed, n_pass):
    """One call of pcl_step_absorb_grid / pcl_group_step_absorb_grid: (counts int64[4] -- exposed, interacted, absorbed along the path,
    absorbed at the interaction --, absorbed_by_cell int64 of the grid's shape, with a last dimension of B bands if ``E_edges`` is
    given).  ``p``: the probability of absorption along the path per pass, ``omega0``: the single-scattering albedo, each None or one
    value per cell (and band), row-major in the order of ``axes`` (any shape of that size), not both None; ``axes``, ``edges``,
    ``center``: as for ``_grid`` (the library squares the edges of a radius axis); ``n_pass``: the caller's own pass counter (a Philox
    counter word).  The tables go up and the tallies come back with every call."""
    coords = np.array([GRID_COORDS.get(a, a) for a in axes], dtype=np.int32)
    per_axis = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
    if len(per_axis) != len(coords):
        raise ValueError("one sequence of edges per axis: %d axes, %d sequences" % (len(coords), len(per_axis)))
    n_bins = np.array([len(e) - 1 for e in per_axis], dtype=np.int32)
    ed = np.ascontiguousarray(np.concatenate(per_axis)) if per_axis else np.zeros(0)
    Ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    B = 0 if Ee is None else len(Ee) - 1
    shape = [max(int(b), 0) for b in n_bins] + ([B] if Ee is not None else [])
    tabs = [None if t is None else np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in (p, omega0)]
    if tabs[0] is None and tabs[1] is None:
        raise ValueError("p and omega0 are both None: an absorption needs one of them")
    for name, t in zip(("p", "omega0"), tabs):
        if t is not None and len(t) != int(np.prod(shape)):
            raise ValueError("%s holds %d values for a grid of shape %r" % (name, len(t), tuple(shape)))
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    counts = np.zeros(4, dtype=np.int64)
    cells = np.zeros(shape, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                                                       # noqa: E731
    check(entry(handle, len(coords), coords.ctypes.data, n_bins.ctypes.data, ed.ctypes.data, ptr(ce), B, ptr(Ee), ptr(tabs[0]), ptr(tabs[1]),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pass) & 0xFFFFFFFF, counts.ctypes.data, cells.ctypes.data))
    return counts, cells


def plane_flux_lds_bytes(n_levels, n_u, n_v, n_bands, n_cells):
    """The LDS the LDS form of a pcl_step_plane_flux call asks for, by the header's formula: S levels, n_u x n_v columns, B bands (0:
    none) and C = 2 S max(B, 1) n_u n_v cells."""
    S, B = int(n_levels), int(n_bands)
    return 8 * (S + int(n_u) + 1 + int(n_v) + 1 + (B + 1 if B else 0)) + 4 * (2 * S + int(n_cells))


def plane_flux_lds_form(n_levels, n_u, n_v, n_bands):
    """Whether a pcl_step_plane_flux call keeps its maps in LDS (the header's bound) or adds to them in device memory."""
    cells = 2 * int(n_levels) * max(int(n_bands), 1) * int(n_u) * int(n_v)
    return cells <= PLANE_FLUX_LDS_CELLS and plane_flux_lds_bytes(n_levels, n_u, n_v, n_bands, cells) <= PLANE_FLUX_LDS_BYTES


def _plane_flux(entry, handle, axis, levels, edges, E_edges=None):
    """One call of pcl_step_plane_flux / pcl_group_step_plane_flux: (counts int64[2, S] -- [0]: up, [1]: down --, maps int64[2, S,
    max(bands, 1), n_u, n_v]).  ``axis``: "x", "y", "z" (or the header's numbers), the normal; ``edges``: the bin edges of the two
    transverse axes, (u, v); the levels and the edges go over as given."""
    lv = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    per_axis = [np.ascontiguousarray(e, dtype=np.float64).reshape(-1) for e in edges]
    if len(per_axis) != 2:
        raise ValueError("two sequences of edges, for u and for v: got %d" % len(per_axis))
    ue, ve = per_axis
    ee = None if E_edges is None else np.ascontiguousarray(E_edges, dtype=np.float64).reshape(-1)
    S, nu, nv, nE = len(lv), len(ue) - 1, len(ve) - 1, 0 if ee is None else len(ee) - 1
    counts = np.zeros((2, S), dtype=np.int64)
    maps = np.zeros((2, S, max(nE, 1), max(nu, 0), max(nv, 0)), dtype=np.int64)
    check(entry(handle, int(PLANE_FLUX_AXES.get(axis, axis)), S, lv.ctypes.data, ue.ctypes.data, nu, ve.ctypes.data, nv,
                None if ee is None else ee.ctypes.data, nE, counts.ctypes.data, maps.ctypes.data))
    return counts, maps


def _scatter(sc, required=False, lazy=False, empty_expr=b""):
    """The scatter constants of a dict, in ABI order: A, n, flags, c, h, n_expr.  Missing keys are zeros, but A and n raise
    KeyError where the entry point has no "no scatter" form (``required``).  ``empty_expr``: what an empty expression goes
    over as (see DeviceGroup)."""
    A, n = (sc["A"], sc["n"]) if required else (sc.get("A", 0.0), sc.get("n", 0.0))
    expr = sc.get("n_expr")
    return (float(A), float(n), int(sc.get("flags", 0)) | (FUSED_LAZY if lazy else 0), float(sc.get("c", 0.0)),
            float(sc.get("h", 0.0)), None if expr is None else expr.encode() if expr else empty_expr)


def _phase_kinds(phases):
    return np.array([_PHASES[p] for p in phases], dtype=np.int32)


def _rows_out(n_rows, n_planes):
    return np.zeros((n_rows, 5 + max(n_planes, 0)), dtype=np.int64)


class DeviceArray:
    """Raw device allocation for Level-1 callers (what cl_array.to_device / cl_array.empty gave)."""

    def __init__(self, dev, n, dtype):
        self.dev, self.n, self.dtype = dev, int(n), np.dtype(dtype)
        p = c_void_p()
        check(dev.lib.pcl_dev_alloc(dev.ctx, self.n * self.dtype.itemsize, byref(p)))
        self.ptr = p

    @classmethod
    def from_host(cls, dev, arr, dtype=np.float64):
        arr, hp = _host(arr, dtype)
        self = cls(dev, arr.size, dtype)
        check(dev.lib.pcl_h2d(dev.ctx, self.ptr, hp, arr.nbytes))
        return self

    def fill_bytes(self, value):
        check(self.dev.lib.pcl_dev_memset(self.dev.ctx, self.ptr, value, self.n * self.dtype.itemsize))

    def get(self):
        out = np.empty(self.n, dtype=self.dtype)
        check(self.dev.lib.pcl_d2h(self.dev.ctx, out.ctypes.data_as(c_void_p), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr is not None and self.dev.ctx:
            check(self.dev.lib.pcl_dev_free(self.dev.ctx, self.ptr))
        self.ptr = None


_CTYPES = {"double": c_double, "int": c_int32, "float": ctypes.c_float, "long": c_int64}


class UserKernel:
    """A hipRTC-compiled user kernel (``pcl_user_kernel_*``): the device side of ``CLProgram``."""

    def __init__(self, dev, name, params, body):
        self.dev, self.name, self.params = dev, name, list(params)
        decl = ", ".join("%s %s%s" % (ct, "*" if ptr else "", nm) for ct, nm, ptr in self.params)
        h = c_void_p()
        rc = dev.lib.pcl_user_kernel_build(dev.ctx, name.encode(), decl.encode(), body.encode(), byref(h))
        if rc != 0:
            raise HipError(rc, dev.lib.pcl_last_error().decode("utf-8", "replace"))
        self.handle = h
        fields = [("a%d" % i, c_void_p if ptr else _CTYPES[ct]) for i, (ct, nm, ptr) in enumerate(self.params)]
        self._argtype = type("pcl_args_" + name, (ctypes.Structure,), {"_fields_": fields})

    def __call__(self, n, *args):
        assert len(args) == len(self.params), "kernel %s takes %d arguments" % (self.name, len(self.params))
        packed = self._argtype()
        for i, ((ct, nm, ptr), a) in enumerate(zip(self.params, args)):
            setattr(packed, "a%d" % i, a.ptr if ptr else _CTYPES[ct](a).value)
        check(self.dev.lib.pcl_user_kernel_launch(self.dev.ctx, self.handle, int(n), byref(packed), ctypes.sizeof(packed)))

    def free(self):
        if self.handle is not None and self.dev.ctx:
            self.dev.lib.pcl_user_kernel_free(self.dev.ctx, self.handle)
        self.handle = None


class Device:
    """One HIP context (device + stream) and, optionally, one resident particle store."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        ctx = c_void_p()
        check(self.lib.pcl_ctx_create(int(device), c_void_p(stream) if stream else None, byref(ctx)))
        self.ctx = ctx
        self.device = int(device)

    # ---------------------------------------------------------------- lifecycle
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.pcl_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_rtc_background(self, on=True):
        """Built-in variable_n_fn shapes start on the ahead-of-time kernels while hipRTC compiles (pcl_ctx_set_rtc_background)."""
        check(self.lib.pcl_ctx_set_rtc_background(self.ctx, 1 if on else 0))

    def rtc_wait(self):
        """Block until every specialisation still compiling in the background is in place; returns how many were pending."""
        n = c_int(0)
        check(self.lib.pcl_ctx_rtc_wait(self.ctx, byref(n)))
        return n.value

    def sync(self):
        check(self.lib.pcl_ctx_sync(self.ctx))

    def info(self):
        name = ctypes.create_string_buffer(256)
        hbm, cu, wf = c_int64(), c_int(), c_int()
        check(self.lib.pcl_ctx_device_info(self.ctx, name, 256, byref(hbm), byref(cu), byref(wf)))
        pci = ctypes.create_string_buffer(64)
        check(self.lib.pcl_ctx_device_pci(self.ctx, pci, 64))
        return {"name": name.value.decode(), "hbm_bytes": hbm.value, "compute_units": cu.value,
                "wavefront": wf.value, "device": self.device, "pci_bus_id": pci.value.decode()}

    def mem_info(self):
        """(free, total) bytes of the device as the driver reports them (idle pool blocks count as used)."""
        f, t = c_int64(), c_int64()
        check(self.lib.pcl_ctx_mem_info(self.ctx, byref(f), byref(t)))
        return f.value, t.value

    def timer_start(self):
        check(self.lib.pcl_timer_start(self.ctx))

    def timer_stop(self):
        ms = c_double()
        check(self.lib.pcl_timer_stop(self.ctx, byref(ms)))
        return ms.value

    def prof_enable(self, on=True):
        check(self.lib.pcl_prof_enable(self.ctx, 1 if on else 0))

    def prof_read(self, kernel_id):
        n, tot, mn, mx = c_int64(), c_double(), c_double(), c_double()
        check(self.lib.pcl_prof_read(self.ctx, kernel_id, byref(n), byref(tot), byref(mn), byref(mx)))
        return {"launches": n.value, "total_ms": tot.value, "min_ms": mn.value, "max_ms": mx.value,
                "avg_ms": tot.value / n.value if n.value else 0.0}

    # ---------------------------------------------------------------- Level 1 (reference-ABI kernels)
    def array(self, host, dtype=np.float64):
        return DeviceArray.from_host(self, host, dtype)

    def empty(self, n, dtype=np.float64):
        return DeviceArray(self, n, dtype)

    def k_light_scatter_step_del(self, dx, dy, dz, rand, n, A, result, N):
        check(self.lib.pcl_k_light_scatter_step_del(self.ctx, dx.ptr, dy.ptr, dz.ptr, rand.ptr, n, A, result.ptr, N))

    def k_scatter_delete_test(self, d0, d1, d2, rand, A, n, res, N):
        check(self.lib.pcl_k_scatter_delete_test(self.ctx, d0.ptr, d1.ptr, d2.ptr, rand.ptr, A, n, res.ptr, N))

    def k_light_scatter_step_sphere(self, d0, d1, d2, rtheta, rphi, rand, A, n, E, r, res0, res1, res2, N, flags, c, h,
                                    n_expr=None):
        nul = c_void_p()
        r = r or (None, None, None)
        check(self.lib.pcl_k_light_scatter_step_sphere(
            self.ctx, d0.ptr, d1.ptr, d2.ptr, rtheta.ptr, rphi.ptr, rand.ptr, A, n, E.ptr if E is not None else nul,
            *[x.ptr if x is not None else nul for x in r], res0.ptr, res1.ptr, res2.ptr, N, flags, c, h,
            n_expr.encode() if n_expr is not None else None))

    def k_compact_indices(self, flags, N, idx_out):
        keep = c_int64()
        check(self.lib.pcl_k_compact_indices(self.ctx, flags.ptr, N, idx_out.ptr, byref(keep)))
        return keep.value

    def user_kernel(self, name, params, body):
        """Compile a kernel body (OpenCL-C dialect) with hipRTC.  params: [(ctype, name, is_pointer), ...]."""
        return UserKernel(self, name, params, body)

    # ---------------------------------------------------------------- Level 2 (resident store)
    def store_alloc(self, capacity, dtype="f64"):
        """dtype 'f64' (the reference's precision, default) or 'f32' (precision sweep)."""
        code = {"f64": DTYPE_F64, "f32": DTYPE_F32, np.float64: DTYPE_F64, np.float32: DTYPE_F32}[dtype]
        check(self.lib.pcl_store_alloc_dtype(self.ctx, int(capacity), code))

    @property
    def np_dtype(self):
        d = c_int()
        check(self.lib.pcl_store_dtype(self.ctx, byref(d)))
        return _NP_DTYPE[d.value]

    def store_free(self):
        check(self.lib.pcl_store_free(self.ctx))

    @property
    def capacity(self):
        v = c_int64()
        check(self.lib.pcl_store_capacity(self.ctx, byref(v)))
        return v.value

    @property
    def count(self):
        v = c_int64()
        check(self.lib.pcl_store_count(self.ctx, byref(v)))
        return v.value

    @property
    def slots(self):
        """Slots the store spans: the count when it is dense, more while the delete path keeps removed photons' slots
        behind its alive mask (pcl_store_slots)."""
        v = c_int64()
        check(self.lib.pcl_store_slots(self.ctx, byref(v), None))
        return v.value

    def last_multi_work(self):
        """(dense passes, wave-steps, photons per wave, wave-steps on exp's saturation shortcut or -1) of the last
        step_fused_multi launch (pcl_store_last_multi_work)."""
        a, b, c, e = c_int64(), c_int64(), c_int(), c_int64()
        check(self.lib.pcl_store_last_multi_work(self.ctx, byref(a), byref(b), byref(c), byref(e)))
        return a.value, b.value, c.value, e.value

    def last_multi_clock(self):
        """GHz the chip held under the last step_fused_multi launch (pcl_store_last_multi_clock); 0.0 before any."""
        g = c_double()
        check(self.lib.pcl_store_last_multi_clock(self.ctx, byref(g)))
        return g.value

    def last_mixed_rows(self):
        """Rows of 64 particles per wave and trip in the last step_mixed_multi launch (pcl_store_last_mixed_rows): 2 or 3."""
        g = c_int()
        check(self.lib.pcl_store_last_mixed_rows(self.ctx, byref(g)))
        return g.value

    def ahead_clock(self):
        """GHz the chip held under this context's k_delete_ahead_live launches (pcl_store_ahead_clock); 0.0 before any."""
        g = c_double()
        check(self.lib.pcl_store_ahead_clock(self.ctx, byref(g)))
        return g.value

    def last_multi_hist(self):
        """Hits queued per wave and step in the last step_fused_multi launch, 129 bins (debug builds: pcl_store_last_multi_hist)."""
        out = np.zeros(129, dtype=np.int64)
        check(self.lib.pcl_store_last_multi_hist(self.ctx, out.ctypes.data))
        return out

    def ahead_stats(self):
        """(launches, bodies answered, launches not used up) of the delete bodies worked out ahead (pcl_store_ahead_stats)."""
        a, b, c = c_int64(), c_int64(), c_int64()
        check(self.lib.pcl_store_ahead_stats(self.ctx, byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    def ahead_work(self):
        """(groups of 128 slots loaded with a first pass of two bodies, ... of one body, rounds deciding two bodies, rounds
        deciding one) summed over the k_delete_ahead_live launches of this context, as the kernel tallied them
        (pcl_store_ahead_work)."""
        a, b, c, d = c_int64(), c_int64(), c_int64(), c_int64()
        check(self.lib.pcl_store_ahead_work(self.ctx, byref(a), byref(b), byref(c), byref(d)))
        return a.value, b.value, c.value, d.value

    def reserve_compaction(self):
        """Allocate the second slab, id arrays and mask scratch of the delete path now (pcl_store_reserve_compaction)."""
        check(self.lib.pcl_store_reserve_compaction(self.ctx))

    def set_count(self, count, id_base=0):
        check(self.lib.pcl_store_set_count(self.ctx, int(count), int(id_base)))

    def upload(self, field, host, offset=0):
        a, hp = _host(host, self.np_dtype)                 # rounded to the store's precision on the host
        check(self.lib.pcl_store_upload(self.ctx, field, hp, offset, a.size))

    def download(self, field, n=None, offset=0):
        """Field values in the store's own dtype (float64 or float32 array)."""
        n = self.count - offset if n is None else n
        out = np.empty(n, dtype=self.np_dtype)
        check(self.lib.pcl_store_download(self.ctx, field, out.ctypes.data_as(c_void_p), offset, n))
        return out

    def upload_ids(self, host, offset=0):
        a, hp = _host(host, np.int64)
        check(self.lib.pcl_store_upload_ids(self.ctx, hp, offset, a.size))

    def download_ids(self, n=None, offset=0):
        n = self.count - offset if n is None else n
        out = np.empty(n, dtype=np.int64)
        check(self.lib.pcl_store_download_ids(self.ctx, out.ctypes.data_as(c_void_p), offset, n))
        return out

    def upload_kind(self, host, offset=0):
        a, hp = _host(host, np.uint8)
        check(self.lib.pcl_store_upload_kind(self.ctx, hp, offset, a.size))

    def download_kind(self, n=None, offset=0):
        n = self.count - offset if n is None else n
        out = np.empty(n, dtype=np.uint8)
        check(self.lib.pcl_store_download_kind(self.ctx, out.ctypes.data_as(c_void_p), offset, n))
        return out

    def field_ptr(self, field):
        p = c_void_p()
        check(self.lib.pcl_store_field_ptr(self.ctx, field, byref(p)))
        return p.value

    def alloc_info(self):
        """How the store's slab was chosen: {'candidates_GBps': [...], 'chosen_GBps': x} (empty list: no selection)."""
        n, chosen = c_int(0), c_double(0.0)
        rates = (c_double * 8)()
        check(self.lib.pcl_store_alloc_info(self.ctx, byref(n), rates, 8, byref(chosen)))
        return {"candidates_GBps": [round(rates[k], 1) for k in range(n.value)], "chosen_GBps": round(chosen.value, 1)}

    def layout(self):
        """(tile_len, tile_stride) in elements: element i of a row is at row0[(i // T) * stride + i % T]."""
        t, ts = c_int64(), c_int64()
        check(self.lib.pcl_store_layout(self.ctx, byref(t), byref(ts)))
        return t.value, ts.value

    def upload_rand(self, which, host):
        a, hp = _host(host, self.np_dtype)
        check(self.lib.pcl_store_upload_rand(self.ctx, which, hp, a.size))

    RAND3_CHUNK = 1 << 20

    def upload_rand3(self, u3, offset=0):
        """Rows [offset, offset + len(u3)) of the reference's per-photon draws (rtheta-, rphi-, rand-uniform): ``u3`` is
        what ``np.random.random((n, 3))`` returns, at most RAND3_CHUNK rows per call, chunks in particle order from 0."""
        a = np.ascontiguousarray(u3, dtype=np.float64).reshape(-1, 3)
        check(self.lib.pcl_store_upload_rand3(self.ctx, a.ctypes.data, int(offset), len(a)))

    def fill_photons(self, n, id_base, c, e_min, e_max, seed):
        check(self.lib.pcl_store_fill_photons(self.ctx, int(n), int(id_base), c, e_min, e_max, int(seed)))

    def fill_photons_table(self, n, id_base, c, cdf, grid, seed):
        cdf, cp = _host(cdf, np.float64)
        grid, gp = _host(grid, np.float64)
        assert cdf.shape == grid.shape
        check(self.lib.pcl_store_fill_photons_table(self.ctx, int(n), int(id_base), c, cp, gp, len(cdf), int(seed)))

    def apply_source(self, src, c, seed):
        """Positions and velocities of a ``light.PhotonSource`` for the photons ``fill_photons`` / ``fill_photons_table`` has
        just created (pcl_store_apply_source; ``seed`` = the fill's: the draws are keyed by it and the photon's id)."""
        _source(self.lib.pcl_store_apply_source, self.ctx, src, c, seed)

    def upload_state(self, state):
        """state: dict with 'r','v','dr','dv' -> (n,3) or 3 arrays, 'E' -> (n,).  Sets count = n."""
        n = len(np.asarray(state["E"]))
        self.set_count(n, int(state.get("id_base", 0)))
        for g, fids in FIELD_GROUPS.items():
            a = state.get(g)
            for k, fid in enumerate(fids):
                col = np.zeros(n) if a is None else (np.asarray(a)[:, k] if np.ndim(a) == 2 else a[k])
                self.upload(fid, col)
        self.upload(E, state["E"])
        if state.get("id") is not None:
            self.upload_ids(state["id"])
        if state.get("kind") is not None:
            self.upload_kind(state["kind"])

    def download_state(self):
        n = self.count
        out = {g: [self.download(fid, n) for fid in fids] for g, fids in FIELD_GROUPS.items()}
        out["E"] = self.download(E, n)
        out["id"] = self.download_ids(n)
        return out

    def step_newton(self, dt):
        check(self.lib.pcl_step_newton(self.ctx, float(dt)))

    def step_scatter_isotropic(self, A, n, flags, c, h, n_expr=None, rng_mode=RNG_PHILOX, seed=0, step=0,
                               want_hits=True):
        hits = c_int64()
        check(self.lib.pcl_step_scatter_isotropic(
            self.ctx, float(A), float(n), int(flags), float(c), float(h),
            n_expr.encode() if n_expr is not None else None, int(rng_mode), int(seed), int(step) & 0xFFFFFFFF,
            byref(hits) if want_hits else None))
        return hits.value if want_hits else None

    def scatter_pcoll(self, A, n, flags, c, h):
        """Collision probability of every particle (constant n; ``flags`` & SCATTER_WAVELENGTH adds the wavelength
        term), as the scatter kernels compute it: input of the host-side RNG replay of the reference's CPU paths."""
        out = np.empty(self.count, dtype=self.np_dtype)
        check(self.lib.pcl_step_scatter_pcoll(self.ctx, float(A), float(n), int(flags), float(c), float(h),
                                              out.ctypes.data_as(c_void_p)))
        return out

    def step_delete_flags(self, flags):
        """Remove the particles whose flag is 1 (stable compaction of the whole state).  Returns (alive, removed)."""
        f = np.ascontiguousarray(flags, dtype=np.int32)
        if f.size != self.count:
            raise ValueError("one flag per particle: got %d for %d" % (f.size, self.count))
        alive, removed = c_int64(), c_int64()
        check(self.lib.pcl_step_delete_flags(self.ctx, f.ctypes.data_as(c_void_p), byref(alive), byref(removed)))
        return alive.value, removed.value

    def step_fused(self, dt, scatter=None, planes=None, sync=True, lazy=False):
        """One pass: Newton, then ScatterIsotropic if ``scatter`` (dict: A, n, flags, c, h, n_expr, rng_mode,
        seed, step), then counters if ``planes`` is not None (sequence of [x,y,z] rows, may be empty).
        Returns {'N','sign','planes','hits'} when counters are on and sync, else None."""
        sc = scatter or {}
        pl, pp, npl = _planes(planes, off=True)
        out = _rows_out(1, npl)[0] if sync and npl >= 0 else None
        check(self.lib.pcl_step_fused(
            self.ctx, float(dt), 1 if scatter else 0, *_scatter(sc, lazy=lazy), int(sc.get("rng_mode", RNG_PHILOX)),
            int(sc.get("seed", 0)), int(sc.get("step", 0)) & 0xFFFFFFFF, pp, npl, None if out is None else out.ctypes.data))
        return None if out is None else _row_dict(out, "hits")

    def is_uniform(self):
        """All photons with implicit ids: eligible for step_fused_multi."""
        u = c_int()
        check(self.lib.pcl_store_is_uniform(self.ctx, byref(u)))
        return bool(u.value)

    def step_fused_multi(self, dt, k_steps, scatter, planes=(), sync=True, raw=False):
        """``k_steps`` consecutive lazy fused steps (Newton + ScatterIsotropic + sign / plane counters, device RNG,
        launch indices scatter['step'] .. +k_steps-1) in one pass over the store.  Returns a list of k_steps dicts like
        step_fused's (or None if not sync)."""
        sc = scatter
        pl, pp, npl = _planes(planes)
        out = _rows_out(k_steps, npl) if sync else None
        check(self.lib.pcl_step_fused_multi(
            self.ctx, float(dt), int(k_steps), *_scatter(sc, required=True), int(sc.get("seed", 0)),
            int(sc.get("step", 0)) & 0xFFFFFFFF, pp, npl, out.ctypes.data if sync else None))
        if out is None or raw:    # raw: (k_steps, 5 + n_planes) int64, [N, sign x 3, planes ..., hits] per step
            return out
        return [_row_dict(o, "hits") for o in out]

    def step_mixed_multi(self, dt, k_passes, phases, scatter=None, delete=None, planes=(), seed=0, step=0, raw=False):
        """``k_passes`` passes of a loop whose body holds the phases ``phases`` -- a sequence of "iso" / "delete", at
        most one of each -- every phase being Newton + the light step + the counters of the measure steps behind it;
        one pass over the store and (with a delete phase) one compaction.  ``scatter``: dict A, n, flags, c, h, n_expr
        (kernel constants) of the isotropic phase; ``delete``: (A, n) of the delete phase.  Device RNG; phase j of
        pass p uses launch index ``step + p * len(phases) + j``.  Returns one dict per phase, in order:
        {'phase', 'N' (alive after it), 'sign', 'planes', 'hits' | 'removed'}."""
        kinds = _phase_kinds(phases)
        A_d, n_d = delete if delete is not None else (0.0, 0.0)
        pl, pp, npl = _planes(planes)
        out = _rows_out(k_passes * len(kinds), npl)
        check(self.lib.pcl_step_mixed_multi(
            self.ctx, float(dt), int(k_passes), len(kinds), kinds.ctypes.data, *_scatter(scatter or {}), float(A_d), float(n_d),
            int(seed), int(step) & 0xFFFFFFFF, pp, npl, out.ctypes.data))
        if raw:                   # (k_passes * len(phases), 5 + n_planes) int64: [N, sign x 3, planes ..., hits | removed]
            return out
        return [dict(phase=ph, **_row_dict(o, "hits" if ph == "iso" else "removed"))
                for o, ph in zip(out, list(phases) * int(k_passes))]

    def trace_ahead(self, ids, dt, k_passes, phases, record_phase=0, scatter=None, delete=None, seed=0, step=0, defer=False):
        """Where the particles with the (ascending) ids ``ids`` will be when a trace step behind phase ``record_phase`` runs
        in each of the next ``k_passes`` passes of a loop with the phases ``phases`` ("iso" / "delete"; arguments as
        step_mixed_multi's) -- worked out from the store as it stands, which is NOT changed (pcl_store_trace_ahead): call it
        with the arguments of the K-pass launch, before that launch.  Returns (k_passes, len(ids), 4) float64:
        r0, r1, r2, moved (dv != 0); NaN rows where the particle is not in the store at that point.
        ``defer=True``: the kernel is only enqueued and a function is returned that hands the rows out -- call it behind the
        K-pass launch (same stream, in order: the rows are there when the launch's own counter rows are, no extra wait)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        kinds = _phase_kinds(phases)
        A_d, n_d = delete if delete is not None else (0.0, 0.0)
        out = np.empty((int(k_passes), len(ids), 4), dtype=np.float64)
        check(self.lib.pcl_store_trace_ahead(
            self.ctx, ids.ctypes.data_as(c_void_p), len(ids), float(dt), int(k_passes), len(kinds), kinds.ctypes.data,
            int(record_phase), *_scatter(scatter or {}), float(A_d), float(n_d), int(seed), int(step) & 0xFFFFFFFF,
            None if (defer and out.size) else out.ctypes.data_as(c_void_p)))
        if not defer:
            return out

        def read():
            if out.size:
                check(self.lib.pcl_store_trace_read(self.ctx, out.ctypes.data_as(c_void_p), out.size))
            return out
        return read

    def step_fused_read(self, n_planes=0):
        """Counters of the last ``step_fused(..., sync=False)``: same dict as the synchronous call."""
        out = _rows_out(1, n_planes)[0]
        check(self.lib.pcl_step_fused_read(self.ctx, n_planes, out.ctypes.data))
        return _row_dict(out, "hits")

    def last_scatter_hits(self):
        h = c_int64()
        check(self.lib.pcl_store_last_scatter_hits(self.ctx, byref(h)))
        return h.value

    def step_scatter_delete(self, A, n, rng_mode=RNG_PHILOX, seed=0, step=0):
        alive, removed = c_int64(), c_int64()
        check(self.lib.pcl_step_scatter_delete(self.ctx, float(A), float(n), int(rng_mode), int(seed),
                                               int(step) & 0xFFFFFFFF, byref(alive), byref(removed)))
        return alive.value, removed.value

    def step_fused_delete(self, dt, A, n, rng_mode=RNG_PHILOX, seed=0, step=0, planes=None, lazy=False):
        """Newton + ScatterDelete (+ counters on the survivors if ``planes`` is not None) as one pipeline.
        Returns {'N' (alive), 'removed', 'sign', 'planes'}."""
        # (the host-latency path of the delete-until-empty run, one call per loop body: plain addresses instead of c_void_p
        #  objects, no call of check() unless something failed, and views of ``out`` -- this call's own array -- not copies,
        #  cut here: _row_dict's two calls and ``...`` indexing cost this call a tenth of its host time)
        pl, pp, npl = _planes(planes, off=True)
        out = np.zeros(5 + max(npl, 0), dtype=np.int64)
        rc = self.lib.pcl_step_fused_delete(self.ctx, float(dt), float(A), float(n), FUSED_LAZY if lazy else 0,
                                            int(rng_mode), int(seed), int(step) & 0xFFFFFFFF, pp, npl, out.ctypes.data)
        if rc != 0:
            check(rc)
        return {"N": int(out[CNT_N]), "sign": out[CNT_XP:CNT_PLANE0], "planes": out[CNT_PLANE0:_EVENT], "removed": int(out[_EVENT])}

    def step_fused_delete_multi(self, dt, k_steps, A, n, seed=0, step=0, planes=None, raw=False):
        """``k_steps`` delete loop bodies (Newton + ScatterDelete + counters on the survivors) in one pass and one
        compaction.  Returns a list of k_steps dicts {'N','removed','sign','planes'}."""
        pl, pp, npl = _planes(planes, off=True)
        out = _rows_out(k_steps, npl)
        check(self.lib.pcl_step_fused_delete_multi(self.ctx, float(dt), int(k_steps), float(A), float(n), int(seed),
                                                   int(step) & 0xFFFFFFFF, pp, npl, out.ctypes.data))
        if raw:                   # (k_steps, 5 + n_planes) int64: [N, sign x 3, planes ..., removed] per body
            return out
        return [_row_dict(o, "removed") for o in out]

    def last_delete_flags(self, n):
        out = np.empty(n, dtype=np.int32)
        check(self.lib.pcl_store_last_delete_flags(self.ctx, out.ctypes.data_as(c_void_p), n))
        return out

    def plane_energies(self, plane, n_hint=None):
        """Energies of the photons that crossed ``plane`` ([x, y, z] with NaN in the free coordinates) in the last
        move, in particle order (ScatterMeasureStep(measure_E=True)).  ``n_hint``: the crossing count if the caller
        already has it from step_counters (sizes the host buffer)."""
        pl = np.ascontiguousarray(np.asarray(plane, dtype=np.float64).reshape(3))
        n = c_int64()
        cap = self.count if n_hint is None else min(int(n_hint), self.count)
        out = np.empty(max(cap, 1), dtype=self.np_dtype)
        check(self.lib.pcl_step_plane_energies(self.ctx, pl.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p), cap, byref(n)))
        if n.value > cap:
            raise HipError(-2, "plane_energies: %d photons crossed, n_hint was %d" % (n.value, cap))
        return out[:n.value].copy()

    def step_counters(self, planes=()):
        pl, pp, npl = _planes(planes)
        out = np.zeros(CNT_PLANE0 + npl, dtype=np.int64)      # [N, sign x 3, planes ...]: no light step, no last column
        check(self.lib.pcl_step_counters(self.ctx, pp, npl, out.ctypes.data))
        return out

    def plane_spectra(self, planes, edges):
        """Per plane the number of particles that crossed it in the last move and the histogram of the crossing photons'
        energies over the bin ``edges`` (len(edges) - 1 bins, counted as ``numpy.histogram(E, bins=edges)`` does), for all
        planes in one sweep of the store: (counts int64[P], hist int64[P, B]).  ScatterMeasureStep(measure_E=True, E_bins=...)."""
        return _spectra(self.lib.pcl_step_plane_spectra, self.ctx, planes, edges)

    def position_grid(self, axes, edges, center=None):
        """Where the particles of the store are: the int64 histogram of their positions over the ``axes`` ("x", "y", "z",
        or "r", the distance from ``center``; one to three, each once), ``edges[a]`` the bin edges of axis a -- shape (bins of
        axis 0, ...), counted as ``numpy.histogramdd`` counts (a radius axis compares the squared distance with the squared
        edges), every particle of the store, in one sweep (pcl_step_position_grid).  PositionGridMeasureStep."""
        return _grid(self.lib.pcl_step_position_grid, self.ctx, axes, edges, center)

    def shell_crossings(self, radii, center=None, E_edges=None, mu_edges=None):
        """What crossed the spheres of ``radii`` about ``center`` (None: the origin) in the last move, every particle of the
        store, in one sweep (pcl_step_shell_crossings): ``(counts int64[2, S], E_hist int64[2, S, B_E] | None, mu_hist
        int64[2, S, B_mu] | None)``, index 0 outward, 1 inward.  ``E_edges``: bin edges of the crossing photons' energies;
        ``mu_edges``: of the cosine between the move and the outward normal.  ShellCrossingMeasureStep."""
        return _shells(self.lib.pcl_step_shell_crossings, self.ctx, radii, center, E_edges, mu_edges)

    def detector_image(self, position, frame, radius, x_edges, y_edges, E_edges=None):
        """What went through the disc of ``radius`` about ``position`` from the front in the last move, every particle of the
        store, in one sweep (pcl_step_detector_image): ``(counts int64[2] = [through, seen], image int64[max(bands, 1), ny,
        nx])``.  ``frame``: the orthonormal e1, e2, n (n from the detector into the scene); ``x_edges``, ``y_edges``: pixel edges
        in the tangent plane (the direction a photon came from, e1 and e2 over n); ``E_edges``: bands.  DetectorMeasureStep."""
        return _detector(self.lib.pcl_step_detector_image, self.ctx, position, frame, radius, x_edges, y_edges, E_edges)

    def surface_reflect(self, radius, center=None, albedo=1.0, mode="lambertian", c=0.0, seed=0, n_pass=0):
        """The photons whose last move took them into the sphere of ``radius`` about ``center`` (None: the origin) are put
        back, in one sweep (pcl_step_surface_reflect): reflected at the hit point (``mode``: "lambertian" or "specular") with
        speed ``c``, or -- with probability 1 - ``albedo`` -- left there at rest.  ``(reflected, absorbed)``.  SurfaceReflectStep."""
        return _surface(self.lib.pcl_step_surface_reflect, self.ctx, radius, center, albedo, mode, c, seed, n_pass)

    def phase_redirect(self, phase, g=0.0, c=0.0, seed=0, n_pass=0):
        """The photons the scatter step of this pass has hit (``dv != 0``) get a direction drawn from the phase function
        ``phase`` ("isotropic", "hg" with the mean cosine ``g``, "rayleigh") about the direction they had before the scatter, with
        speed ``c``, in one sweep (pcl_step_phase_redirect).  The number re-directed.  PhaseFunctionStep."""
        return _phase(self.lib.pcl_step_phase_redirect, self.ctx, phase, g, c, seed, n_pass)

    def absorb_scattered(self, omega0, edges=None, center=None, E_edges=None, seed=0, n_pass=0):
        """Absorb, with probability ``1 - omega0`` of the layer it stands in, each photon the scatter step of this pass has hit
        (dv != 0): it is left at rest where it is (v = 0, dv = 0), in one sweep (pcl_step_absorb_scattered).  ``(interacted,
        absorbed, absorbed_by_layer int64[L'], E_hist int64[L', B_E] | None)``.  AbsorptionStep."""
        return _absorb(self.lib.pcl_step_absorb_scattered, self.ctx, omega0, edges, center, E_edges, seed, n_pass)

    def phase_layered(self, laws, cum, edges=None, center=None, c=0.0, seed=0, n_pass=0):
        """The photons the scatter step of this pass has hit get a direction about the one they had before, drawn from a law
        that the radial layer they stand in chooses: ``laws`` are ``(kind, g, mu, F)``, row ``b`` of ``cum`` the cumulative
        weights of the laws in layer ``b`` (pcl_step_phase_layered).  ``(scattered, redirected, by_layer int64[L'], by_law
        int64[M])``.  LayeredPhaseStep."""
        return _phase_layered(self.lib.pcl_step_phase_layered, self.ctx, laws, cum, edges, center, c, seed, n_pass)

    def recycle_spent(self, src, c, at_rest=True, top=None, center=None, spectrum=None, seed=0, n_pass=0):
        """The photons at rest (``at_rest``) and those beyond the sphere of ``top`` about ``center`` (None: no top, the origin) are
        re-emitted by the ``light.PhotonSource`` ``src`` with speed ``c``, in one sweep (pcl_step_recycle_spent): new r and v, dr =
        dv = 0, and -- with ``spectrum=(grid, cdf)`` -- a new E; ids and kinds stay.  ``(at_rest, escaped)``.  RecycleStep."""
        return _recycle(self.lib.pcl_step_recycle_spent, self.ctx, src, c, at_rest, top, center, spectrum, seed, n_pass)

    def absorb_path(self, p, edges=None, center=None, E_edges=None, seed=0, n_pass=0):
        """Every moving photon is absorbed with the probability ``p`` of the radial layer (``edges`` about ``center``) it stands in
        and the band (``E_edges``) its energy falls in -- ``p``: max(L, 1) rows of max(B, 1) values --, and is left at rest where it is
        (v = 0, dv = 0), in one sweep (pcl_step_absorb_path).  ``(exposed, absorbed, absorbed_by_cell int64[L', B'])``.
        PathAbsorptionStep."""
        return _absorb_path(self.lib.pcl_step_absorb_path, self.ctx, p, edges, center, E_edges, seed, n_pass)

    def reemit_parked(self, c, eta=1.0, angular="isotropic", tables=None, edges=None, center=None, seed=0, n_pass=0):
        """The photons of the resident store that are parked at rest in a radial layer of ``edges`` about ``center`` (``None``: one
        layer everywhere) re-emitted from where they are with speed ``c``, each with the probability ``eta`` of its layer: a new
        direction -- isotropic, or "lambertian" about the local vertical --, dr = dv = 0 and, where the layer has a table ``(grid,
        cdf)``, a new E, in one sweep (pcl_step_reemit_parked).  ``(parked, reemitted, by_layer int64[L'])``.  light._reemit_parked
        restates the sweep with numpy."""
        return _reemit(self.lib.pcl_step_reemit_parked, self.ctx, eta, angular, tables, edges, center, c, seed, n_pass)

    def refract_surface(self, radius, n_inside, n_outside=1.0, center=None, fresnel=True, c=0.0, seed=0, n_pass=0):
        """The photons of the resident store whose last move crossed the sphere of ``radius`` about ``center``, in either direction,
        refracted into the medium beyond (``n_inside`` within the sphere, ``n_outside`` around it) or reflected -- with Fresnel's
        probability if ``fresnel``, and always beyond the critical angle -- at speed ``c``, with the rest of the move flown along the
        new direction, in one sweep (pcl_step_refract_surface).  int64[6]: in refracted, in reflected, out refracted, out reflected,
        out total, overshot.  light._refract_surface restates the sweep with numpy."""
        return _refract(self.lib.pcl_step_refract_surface, self.ctx, radius, center, n_inside, n_outside, fresnel, c, seed, n_pass)

    def ground_spectral(self, radius, E_edges, albedo, specular=0.0, center=None, c=0.0, seed=0, n_pass=0):
        """The photons of the resident store whose last move took them into the sphere of ``radius`` about ``center`` put back as
        ``Device.surface_reflect`` puts them, with the albedo and the mirrored share of the band their energy falls in (``E_edges``:
        B + 1 edges, ``albedo``: B values, ``specular``: one value or B), in one sweep (pcl_step_ground_spectral); a hit photon in no
        band is absorbed.  ``(counts int64[4]: reflected, absorbed, mirrored, out_of_band; reflected_by_band int64[B];
        absorbed_by_band int64[B])``.  light._spectral_bounce restates the sweep with numpy."""
        return _ground_spectral(self.lib.pcl_step_ground_spectral, self.ctx, radius, center, E_edges, albedo, specular, c, seed, n_pass)

    def scatter_layered(self, p, edges=None, center=None, E_edges=None, first=True, c=0.0, seed=0, n_pass=0):
        """Scattering by layer and band: every moving photon with a layer and a band scatters with the probability ``p[layer][band]``
        into a direction uniform on the sphere, ``dv = v' - v_old``; with ``first`` every other photon gets ``dv = 0``, without it
        nothing else is written -- one sweep (pcl_step_scatter_layered).  ``(exposed, scattered, scattered_by_cell int64[L', B'])``.
        ``n_pass``: the caller's own pass counter (a Philox counter word)."""
        return _scatter_layered(self.lib.pcl_step_scatter_layered, self.ctx, p, edges, center, E_edges, first, c, seed, n_pass)

    def scatter_grid(self, p, axes, edges, center=None, E_edges=None, first=True, c=0.0, seed=0, n_pass=0):
        """Scattering on a grid of cells: every moving photon with a cell of the grid over ``axes`` (``position_grid``'s cells) and a
        band of ``E_edges`` scatters with the probability ``p[cell][band]`` into a direction uniform on the sphere, ``dv = v' - v_old``;
        with ``first`` every other photon gets ``dv = 0``, without it nothing else is written -- one sweep (pcl_step_scatter_grid).
        ``(exposed, scattered, scattered_by_cell int64 of the grid's shape (+ bands))``.  ``n_pass``: the caller's own pass counter."""
        return _scatter_grid(self.lib.pcl_step_scatter_grid, self.ctx, p, axes, edges, center, E_edges, first, c, seed, n_pass)

    def phase_grid(self, laws, cum, axes, edges, center=None, mixture=None, outside=None, c=0.0, seed=0, n_pass=0):
        """The phase functions by grid cell: the photons the scatter step of this pass has hit get a direction drawn about their old
        one from a law chosen by the mixture of their cell -- ``mixture[cell]``, a row of the cumulative weights ``cum``, -1: left
        alone; ``outside``: the row of a photon in no cell, None: left alone; ``mixture=None``: row 0 everywhere
        (pcl_step_phase_grid).  ``(scattered, redirected, by_mixture int64[K], by_law int64[M])`` of this call."""
        if mixture is None:
            mixture = np.zeros([len(np.reshape(e, -1)) - 1 for e in edges], dtype=np.int64)
        return _phase_grid(self.lib.pcl_step_phase_grid, self.ctx, laws, cum, axes, edges, center, mixture, outside, c, seed, n_pass)

    def absorb_grid(self, p, omega0, axes, edges, center=None, E_edges=None, seed=0, n_pass=0):
        """Absorption on a grid of cells, both kinds in one sweep: every moving photon with a cell of the grid over ``axes``
        (``position_grid``'s cells) and a band of ``E_edges`` is absorbed along the path with the probability ``p[cell][band]``, and,
        if it was scattered in this pass (``dv != 0``) and is still under way, at the interaction with ``1 - omega0[cell][band]``; an
        absorbed photon is parked (``v = dv = 0``), nobody else is written (pcl_step_absorb_grid).  Either table may be None, not both.
        ``(counts int64[4]: exposed, interacted, absorbed along the path, absorbed at the interaction; absorbed_by_cell int64 of the
        grid's shape (+ bands))``.  ``n_pass``: the caller's own pass counter."""
        return _absorb_grid(self.lib.pcl_step_absorb_grid, self.ctx, p, omega0, axes, edges, center, E_edges, seed, n_pass)

    def plane_flux(self, axis, levels, edges, E_edges=None):
        """What passed through the planes ``axis = levels[s]`` in the last move, by direction and by the column of ``edges`` (the
        two transverse axes' bin edges) in which the straight move met the plane -- and by band of ``E_edges`` --, in one read-only
        sweep (pcl_step_plane_flux): ``(counts int64[2, S] = [up, down], maps int64[2, S, max(bands, 1), n_u, n_v])``."""
        return _plane_flux(self.lib.pcl_step_plane_flux, self.ctx, axis, levels, edges, E_edges)

    def box_walls(self, modes, lo, hi):
        """The walls of the box ``[lo, hi]``, per axis ``"periodic"``, ``"mirror"``, ``"open"`` or None: every moving photon outside on
        an axis with a wall is handed back in through the other side, folded back at the wall (an odd number of bounces turns ``v``,
        ``dv`` and ``dr`` of the axis round) or, through an open wall, parked at rest -- one deterministic sweep (pcl_step_box_walls).
        int64[8]: moving, multi, crossed[3][2].  light._box_walls restates the sweep with numpy, bit for bit."""
        return _box_walls(self.lib.pcl_step_box_walls, self.ctx, modes, lo, hi)


class DeviceGroup:
    """``pcl_group_*``: several contexts in one process, sharded by global index, behind the C ABI (the shim owns the
    contexts and one worker thread per context, fans every step out and sums the counter rows).  The Python host layer
    uses physicl_amd.multidev.MultiDevice, which does the same over ``Device`` objects; this class binds the C-level
    form a non-Python host would use, for tests and scripts."""

    def __init__(self, devices):
        self.lib = load()
        ids = (c_int * len(devices))(*[int(d) for d in devices])
        g = c_void_p()
        check(self.lib.pcl_group_create(len(devices), ids, byref(g)))
        self.g, self.n = g, len(devices)

    def close(self):
        if getattr(self, "g", None):
            self.lib.pcl_group_destroy(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, n_global, i):
        lo, hi = c_int64(), c_int64()
        check(self.lib.pcl_group_shard(self.g, int(n_global), int(i), byref(lo), byref(hi)))
        return lo.value, hi.value

    def store_alloc(self, capacity, dtype="f64"):
        check(self.lib.pcl_group_store_alloc(self.g, int(capacity), DTYPE_F64 if dtype == "f64" else DTYPE_F32))

    def fill_photons(self, n, id_base, c, e_min, e_max, seed):
        check(self.lib.pcl_group_fill_photons(self.g, int(n), int(id_base), c, e_min, e_max, int(seed)))

    def apply_source(self, src, c, seed):
        """``Device.apply_source`` on every context of the group (pcl_group_apply_source)."""
        _source(self.lib.pcl_group_apply_source, self.g, src, c, seed)

    @property
    def count(self):
        v = c_int64()
        check(self.lib.pcl_group_count(self.g, byref(v)))
        return v.value

    def sync(self):
        check(self.lib.pcl_group_sync(self.g))

    # The step methods answer with the raw rows ([N, sign x 3, planes ..., hits | removed], summed over the contexts).
    # One difference to Device is kept: an EMPTY n_expr goes over as NULL here, as "" there.  With SCATTER_VARIABLE_N set
    # the library refuses both with PCL_ERR_EXPR but words the message differently ("is NULL" / "is empty or longer ...").
    def step_fused_multi(self, dt, k_steps, sc, planes=()):
        pl, pp, npl = _planes(planes)
        out = _rows_out(k_steps, npl)
        check(self.lib.pcl_group_step_fused_multi(self.g, float(dt), int(k_steps), *_scatter(sc, required=True, empty_expr=None),
                                                  int(sc.get("seed", 0)), int(sc.get("step", 0)) & 0xFFFFFFFF, pp, npl, out.ctypes.data))
        return out

    def step_fused_delete(self, dt, A, n, seed, step, planes=(), lazy=True):
        pl, pp, npl = _planes(planes)
        out = np.zeros(5 + npl, dtype=np.int64)
        check(self.lib.pcl_group_step_fused_delete(self.g, float(dt), float(A), float(n), FUSED_LAZY if lazy else 0, RNG_PHILOX, int(seed),
                                                   int(step) & 0xFFFFFFFF, pp, npl, out.ctypes.data))
        return out

    def step_fused_delete_multi(self, dt, k_steps, A, n, seed, step, planes=()):
        pl, pp, npl = _planes(planes)
        out = _rows_out(k_steps, npl)
        check(self.lib.pcl_group_step_fused_delete_multi(self.g, float(dt), int(k_steps), float(A), float(n), int(seed), int(step) & 0xFFFFFFFF,
                                                         pp, npl, out.ctypes.data))
        return out

    def step_mixed_multi(self, dt, k_passes, phases, sc, delete, seed, step, planes=()):
        kinds = _phase_kinds(phases)
        pl, pp, npl = _planes(planes)
        out = _rows_out(k_passes * len(kinds), npl)
        check(self.lib.pcl_group_step_mixed_multi(self.g, float(dt), int(k_passes), len(kinds), kinds.ctypes.data,
                                                  *_scatter(sc, empty_expr=None), float(delete[0]), float(delete[1]), int(seed),
                                                  int(step) & 0xFFFFFFFF, pp, npl, out.ctypes.data))
        return out

    def plane_spectra(self, planes, edges):
        """``Device.plane_spectra`` summed over the group's contexts (pcl_group_step_plane_spectra)."""
        return _spectra(self.lib.pcl_group_step_plane_spectra, self.g, planes, edges)

    def position_grid(self, axes, edges, center=None):
        """``Device.position_grid`` summed over the group's contexts (pcl_group_step_position_grid)."""
        return _grid(self.lib.pcl_group_step_position_grid, self.g, axes, edges, center)

    def shell_crossings(self, radii, center=None, E_edges=None, mu_edges=None):
        """``Device.shell_crossings`` summed over the group's contexts (pcl_group_step_shell_crossings)."""
        return _shells(self.lib.pcl_group_step_shell_crossings, self.g, radii, center, E_edges, mu_edges)

    def detector_image(self, position, frame, radius, x_edges, y_edges, E_edges=None):
        """``Device.detector_image`` summed over the group's contexts (pcl_group_step_detector_image)."""
        return _detector(self.lib.pcl_group_step_detector_image, self.g, position, frame, radius, x_edges, y_edges, E_edges)

    def surface_reflect(self, radius, center=None, albedo=1.0, mode="lambertian", c=0.0, seed=0, n_pass=0):
        """``Device.surface_reflect`` on every context of the group, the counts summed (pcl_group_step_surface_reflect)."""
        return _surface(self.lib.pcl_group_step_surface_reflect, self.g, radius, center, albedo, mode, c, seed, n_pass)

    def phase_redirect(self, phase, g=0.0, c=0.0, seed=0, n_pass=0):
        """``Device.phase_redirect`` on every context of the group, the counts summed (pcl_group_step_phase_redirect)."""
        return _phase(self.lib.pcl_group_step_phase_redirect, self.g, phase, g, c, seed, n_pass)

    def absorb_scattered(self, omega0, edges=None, center=None, E_edges=None, seed=0, n_pass=0):
        """``Device.absorb_scattered`` on every context of the group, the tallies summed (pcl_group_step_absorb_scattered)."""
        return _absorb(self.lib.pcl_group_step_absorb_scattered, self.g, omega0, edges, center, E_edges, seed, n_pass)

    def phase_layered(self, laws, cum, edges=None, center=None, c=0.0, seed=0, n_pass=0):
        """``Device.phase_layered`` on every context of the group, the tallies summed (pcl_group_step_phase_layered)."""
        return _phase_layered(self.lib.pcl_group_step_phase_layered, self.g, laws, cum, edges, center, c, seed, n_pass)

    def recycle_spent(self, src, c, at_rest=True, top=None, center=None, spectrum=None, seed=0, n_pass=0):
        """``Device.recycle_spent`` on every context of the group, the counts summed (pcl_group_step_recycle_spent)."""
        return _recycle(self.lib.pcl_group_step_recycle_spent, self.g, src, c, at_rest, top, center, spectrum, seed, n_pass)

    def absorb_path(self, p, edges=None, center=None, E_edges=None, seed=0, n_pass=0):
        """``Device.absorb_path`` on every context of the group, the tallies summed (pcl_group_step_absorb_path)."""
        return _absorb_path(self.lib.pcl_group_step_absorb_path, self.g, p, edges, center, E_edges, seed, n_pass)

    def reemit_parked(self, c, eta=1.0, angular="isotropic", tables=None, edges=None, center=None, seed=0, n_pass=0):
        """``Device.reemit_parked`` on every context of the group, the counts summed (pcl_group_step_reemit_parked)."""
        return _reemit(self.lib.pcl_group_step_reemit_parked, self.g, eta, angular, tables, edges, center, c, seed, n_pass)

    def refract_surface(self, radius, n_inside, n_outside=1.0, center=None, fresnel=True, c=0.0, seed=0, n_pass=0):
        """``Device.refract_surface`` on every context of the group, the counts summed (pcl_group_step_refract_surface)."""
        return _refract(self.lib.pcl_group_step_refract_surface, self.g, radius, center, n_inside, n_outside, fresnel, c, seed, n_pass)

    def ground_spectral(self, radius, E_edges, albedo, specular=0.0, center=None, c=0.0, seed=0, n_pass=0):
        """``Device.ground_spectral`` on every context of the group, the tallies summed (pcl_group_step_ground_spectral)."""
        return _ground_spectral(self.lib.pcl_group_step_ground_spectral, self.g, radius, center, E_edges, albedo, specular, c, seed, n_pass)

    def scatter_layered(self, p, edges=None, center=None, E_edges=None, first=True, c=0.0, seed=0, n_pass=0):
        """``Device.scatter_layered`` on every context of the group, the tallies summed (pcl_group_step_scatter_layered)."""
        return _scatter_layered(self.lib.pcl_group_step_scatter_layered, self.g, p, edges, center, E_edges, first, c, seed, n_pass)

    def scatter_grid(self, p, axes, edges, center=None, E_edges=None, first=True, c=0.0, seed=0, n_pass=0):
        """``Device.scatter_grid`` on every context of the group, the tallies summed (pcl_group_step_scatter_grid)."""
        return _scatter_grid(self.lib.pcl_group_step_scatter_grid, self.g, p, axes, edges, center, E_edges, first, c, seed, n_pass)

    def phase_grid(self, laws, cum, axes, edges, center=None, mixture=None, outside=None, c=0.0, seed=0, n_pass=0):
        """``Device.phase_grid`` on every context of the group, the tallies summed (pcl_group_step_phase_grid)."""
        if mixture is None:
            mixture = np.zeros([len(np.reshape(e, -1)) - 1 for e in edges], dtype=np.int64)
        return _phase_grid(self.lib.pcl_group_step_phase_grid, self.g, laws, cum, axes, edges, center, mixture, outside, c, seed, n_pass)

    def plane_flux(self, axis, levels, edges, E_edges=None):
        """``Device.plane_flux`` summed over the group's contexts (pcl_group_step_plane_flux)."""
        return _plane_flux(self.lib.pcl_group_step_plane_flux, self.g, axis, levels, edges, E_edges)

    def absorb_grid(self, p, omega0, axes, edges, center=None, E_edges=None, seed=0, n_pass=0):
        """``Device.absorb_grid`` on every context of the group, the tallies summed (pcl_group_step_absorb_grid)."""
        return _absorb_grid(self.lib.pcl_group_step_absorb_grid, self.g, p, omega0, axes, edges, center, E_edges, seed, n_pass)

    def box_walls(self, modes, lo, hi):
        """``Device.box_walls`` on every context of the group, the counts summed (pcl_group_step_box_walls)."""
        return _box_walls(self.lib.pcl_group_step_box_walls, self.g, modes, lo, hi)

    def download(self, field, n=None, offset=0, dtype=None):
        n = self.count - offset if n is None else n
        if dtype is None:                         # the store's own element type (pcl_group_store_dtype)
            d = c_int()
            check(self.lib.pcl_group_store_dtype(self.g, byref(d)))
            dtype = np.float32 if d.value == DTYPE_F32 else np.float64
        out = np.empty(n, dtype=dtype)
        check(self.lib.pcl_group_download(self.g, int(field), out.ctypes.data, int(offset), int(n)))
        return out

    def download_ids(self, n=None, offset=0):
        n = self.count - offset if n is None else n
        out = np.empty(n, dtype=np.int64)
        check(self.lib.pcl_group_download_ids(self.g, out.ctypes.data, int(offset), int(n)))
        return out
