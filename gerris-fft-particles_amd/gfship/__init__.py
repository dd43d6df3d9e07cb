"""gfship -- host-side mirror of the libgfship C ABI (include/gfship.h).

Thin ctypes layer used by tests/, bench.py and __graft_entry__.py: object names follow the
reference (domain, variables, GfsMultilevelParams).  There is no CPU fallback: loading fails
loudly when the HIP library is missing, and creating a domain fails without a device.
"""
import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("GFSHIP_LIB", os.path.join(_PKG, "lib", "libgfship.so"))

SIDE_PERIODIC, SIDE_BOUNDARY, SIDE_EXTERNAL = 0, 1, 2
BC_SYMMETRY, BC_DIRICHLET, BC_NEUMANN = 0, 1, 2
SCHEME_GODUNOV, SCHEME_NONE = 0, 1
RELAX_EXACT, RELAX_REDBLACK, RELAX_EXACT_HYPERPLANE, RELAX_EXACT_PER_SWEEP = 0, 1, 2, 3


class GfshipError(RuntimeError):
    pass


class Norm(C.Structure):
    _fields_ = [("bias", C.c_double), ("first", C.c_double), ("second", C.c_double),
                ("infty", C.c_double), ("w", C.c_double)]


class MultilevelParams(C.Structure):
    """GfsMultilevelParams (src/poisson.h:39-52)."""
    _fields_ = [("tolerance", C.c_double), ("nrelax", C.c_uint), ("erelax", C.c_uint),
                ("minlevel", C.c_uint), ("nitermax", C.c_uint), ("nitermin", C.c_uint),
                ("dimension", C.c_uint), ("niter", C.c_uint), ("depth", C.c_uint),
                ("weighted", C.c_int), ("function", C.c_int),
                ("beta", C.c_double), ("omega", C.c_double),
                ("residual_before", Norm), ("residual", Norm)]


class AdvectionParams(C.Structure):
    """The fields of GfsAdvectionParams used on this path (src/advection.h:50-69)."""
    _fields_ = [("cfl", C.c_double), ("dt", C.c_double), ("gradient", C.c_int), ("gc", C.c_int)]


_lib = None

# every symbol include/gfship.h declares: name -> (restype, argtypes)
_vp, _i, _d, _u = C.c_void_p, C.c_int, C.c_double, C.c_uint
_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int)
SIGNATURES = {
    "gfship_last_error": (C.c_char_p, []),
    "gfship_version": (_i, []),
    "gfship_device_count": (_i, []),
    "gfship_domain_create": (_i, [C.POINTER(_vp), _i, _i, _pi, _i]),
    "gfship_domain_destroy": (None, [_vp]),
    "gfship_domain_set_relax_mode": (_i, [_vp, _i]),
    "gfship_domain_synchronize": (_i, [_vp]),
    "gfship_domain_stream": (_vp, [_vp]),
    "gfship_field_alloc": (_i, [_vp, _i]),
    "gfship_field_free": (_i, [_vp, _i]),
    "gfship_field_set_bc": (_i, [_vp, _i, _i, _i, _pd]),
    "gfship_field_upload": (_i, [_vp, _i, _i, _pd]),
    "gfship_field_download": (_i, [_vp, _i, _i, _pd]),
    "gfship_field_fill": (_i, [_vp, _i, _i, _d]),
    "gfship_field_device_ptr": (_vp, [_vp, _i, _i, _pi, _pi]),
    "gfship_bc": (_i, [_vp, _i, _i, _i]),
    "gfship_homogeneous_bc": (_i, [_vp, _i, _i, _i]),
    "gfship_multilevel_params_init": (None, [C.POINTER(MultilevelParams), _i]),
    "gfship_poisson_coefficients": (_i, [_vp]),
    "gfship_poisson_coefficients_alpha": (_i, [_vp, _pi]),
    "gfship_poisson_weights": (_i, [_vp, _i, _pi]),
    "gfship_relax": (_i, [_vp, _u, _i, _d, _i, _i, _i]),
    "gfship_residual": (_i, [_vp, _u, _i, _i, _i, _i, _i]),
    "gfship_norm_residual": (_i, [_vp, _d, _i, C.POINTER(Norm)]),
    "gfship_norm_variable": (_i, [_vp, _i, C.POINTER(Norm)]),
    "gfship_poisson_cycle": (_i, [_vp, C.POINTER(MultilevelParams), _i, _i, _i, _i]),
    "gfship_poisson_solve": (_i, [_vp, C.POINTER(MultilevelParams), _i, _i, _i, _i, _d]),
    "gfship_diffusion_coefficients": (_i, [_vp, _d, _d, _i, _d]),
    "gfship_diffusion_coefficients_faces": (_i, [_vp, _pi, _d, _i, _i, _d]),
    "gfship_diffusion_rhs": (_i, [_vp, _i, _i, _i, _d]),
    "gfship_diffusion_residual": (_i, [_vp, _i, _i, _i, _i]),
    "gfship_diffusion_cycle": (_i, [_vp, _u, _u, _u, _i, _i, _i, _i]),
    "gfship_diffusion": (_i, [_vp, C.POINTER(MultilevelParams), _i, _i, _i]),
    "gfship_time_relax": (_i, [_vp, _u, _i, _i, _i, _i, _i, _pd]),
    "gfship_time_relax_loop": (_i, [_vp, _i, _i, _i, _i, _u, _i, _pd, _pi]),
    "gfship_time_relax_loop_inclusive": (_i, [_vp, _i, _i, _i, _i, _u, _i, _pd, _pi, _pd]),
    "gfship_sim_create": (_i, [C.POINTER(_vp), _vp]),
    "gfship_sim_destroy": (None, [_vp]),
    "gfship_sim_variable": (_i, [_vp, _i, _i]),
    "gfship_sim_projection_params": (C.POINTER(MultilevelParams), [_vp]),
    "gfship_sim_approx_projection_params": (C.POINTER(MultilevelParams), [_vp]),
    "gfship_sim_advection_params": (C.POINTER(AdvectionParams), [_vp]),
    "gfship_sim_set_time": (_i, [_vp, _d, _d]),
    "gfship_sim_set_next_event": (_i, [_vp, _vp, _vp]),
    "gfship_sim_time": (_d, [_vp]),
    "gfship_sim_iter": (_u, [_vp]),
    "gfship_sim_add_tracer": (_i, [_vp]),
    "gfship_sim_set_viscosity": (_i, [_vp, _i, _d]),
    "gfship_sim_set_viscosity_faces": (_i, [_vp, _i, _pi]),
    "gfship_sim_set_alpha_cell": (_i, [_vp, _i]),
    "gfship_sim_set_viscosity_cell": (_i, [_vp, _i]),
    "gfship_variable_mac_source": (_i, [_vp, _i, _i]),
    "gfship_sim_set_alpha": (_i, [_vp, _pi]),
    "gfship_sim_set_source": (_i, [_vp, _i, _d]),
    "gfship_sim_diffusion_params": (C.POINTER(MultilevelParams), [_vp, _i]),
    "gfship_sim_start": (_i, [_vp]),
    "gfship_sim_step": (_i, [_vp]),
    "gfship_sim_advection_step": (_i, [_vp]),
    "gfship_sim_set_tracer_gradient": (_i, [_vp, _i, _i]),
    "gfship_sim_set_tracer_scheme": (_i, [_vp, _i, _i]),
    "gfship_sim_set_tracer_diffusion": (_i, [_vp, _i, _d]),
    "gfship_sim_tracer_diffusion_params": (C.POINTER(MultilevelParams), [_vp, _i]),
    "gfship_sim_tracer_diffusion_path": (_i, [_vp, _i]),
    "gfship_sim_tracer_diffusion_counts": (_i, [_vp, C.POINTER(C.c_ulonglong)]),
    "gfship_sim_gradients_unstored": (_i, [_vp, C.POINTER(C.c_ulonglong)]),
    "gfship_predicted_face_velocities": (_i, [_vp]),
    "gfship_mac_projection": (_i, [_vp, C.POINTER(MultilevelParams), _d, _i, _pi]),
    "gfship_approximate_projection": (_i, [_vp, C.POINTER(MultilevelParams), _d, _i, _pi]),
    "gfship_centered_velocity_advection": (_i, [_vp, _pi, _pi]),
    "gfship_correct_centered_velocities": (_i, [_vp, _pi, _d]),
    "gfship_sim_advance_time": (_i, [_vp]),
    "gfship_tracer_advection": (_i, [_vp, _i, _d]),
    "gfship_domain_cfl": (_i, [_vp, _pd]),
    "gfship_set_timestep": (_i, [_vp]),
    "gfship_coarse_init": (_i, [_vp]),
    "gfship_divergence_norm": (_i, [_vp, C.POINTER(Norm)]),
    "gfship_sim_download_un": (_i, [_vp, _i, _pd]),
    "gfship_domain_set_overlap": (_i, [_vp, _i]),
    "gfship_domain_set_exchange": (_i, [_vp, _vp, _vp]),
    "gfship_domain_set_reduce": (_i, [_vp, _vp, _vp]),
    "gfship_domain_set_gather": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(C.c_int)]),
    "gfship_domain_path_counts": (_i, [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "gfship_domain_kernel_counts": (_i, [_vp, C.POINTER(C.c_ulonglong), _i]),
    "gfship_sim_restart": (_i, [_vp, _d, _u]),
    "gfship_snapshot_tree_bytes": (C.c_size_t, [_vp, _i]),
    "gfship_snapshot_tree_write": (_i, [_vp, _i, _pi, _vp, C.c_size_t]),
    "gfship_snapshot_tree_read": (_i, [_vp, _i, _pi, _vp, C.c_size_t]),
    "gfship_comm_available": (_i, []),
    "gfship_comm_unique_id": (_i, [_vp]),
    "gfship_domain_comm_init": (_i, [_vp, _vp, _i, _i, _pi]),
    "gfship_domain_comm_size": (_i, [_vp]),
    "gfship_domain_comm_stats": (_i, [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "gfship_domain_comm_destroy": (_i, [_vp]),
    "gfship_halo_pack": (_i, [_vp, _vp, _i, _i, _vp]),
    "gfship_halo_unpack": (_i, [_vp, _vp, _i, _i, _vp]),
    "gfship_halo_pack_sides": (_i, [_vp, _vp, _i, _i, _pi, C.POINTER(_vp)]),
    "gfship_halo_unpack_sides": (_i, [_vp, _vp, _i, _i, _pi, C.POINTER(_vp)]),
    "gfship_field_interpolate": (_i, [_vp, _i, _i, _pd, _pd, C.POINTER(C.c_ubyte)]),
    "gfship_particles_create": (_i, [C.POINTER(_vp), _vp, _i, _pd, C.POINTER(C.c_uint)]),
    "gfship_particles_destroy": (None, [_vp]),
    "gfship_particle_list_event": (_i, [_vp]),
    "gfship_particles_count": (_i, [_vp]),
    "gfship_particles_set_migrate": (_i, [_vp, _vp, _vp]),
    "gfship_particles_slots": (_i, [_vp]),
    "gfship_particles_record_size": (_i, [_vp]),
    "gfship_particles_sort": (_i, [_vp]),
    "gfship_particles_set_sort_interval": (_i, [_vp, _i]),
    "gfship_particles_download": (_i, [_vp, _pd, C.POINTER(C.c_uint)]),
    "gfship_particles_download_old": (_i, [_vp, _pd]),
    "gfship_energy_spectra_bins": (_i, [_vp]),
    "gfship_energy_spectra": (_i, [_vp, _i, C.POINTER(_i), _pd, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    "gfship_init_spectra": (_i, [_vp, _vp, C.POINTER(_i)]),
    "gfship_output_spectra_side": (_i, [_vp]),
    "gfship_output_spectra": (_i, [_vp, _i, _pd, C.POINTER(C.c_double)]),
    "gfship_output_spectra_plane": (_i, [_vp, _i, _i, _d, _pd, _pd]),
    "gfship_turbulent_viscosity": (_i, [_vp, C.POINTER(_i), C.c_double, _i, _i]),
    "gfship_particles_set_particulate": (_i, [_vp, _pd, _pd, _pd]),
    "gfship_particles_set_forces": (_i, [_vp, _i, C.POINTER(_i), _pd]),
    "gfship_particles_set_force_coefficient": (_i, [_vp, _i, C.c_char_p]),
    "gfship_particles_download_particulate": (_i, [_vp, _pd, _pd, _pd]),
    "gfship_particulate_field": (_i, [_vp, _i]),
    "gfship_particles_forces_on_fluid": (_i, [_vp]),
    "gfship_particles_set_kernel": (_i, [_vp, C.c_double, C.c_char_p]),
    "gfship_source_particulate_event": (_i, [_vp, C.POINTER(_i)]),
    "gfship_particles_spread_forces": (_i, [_vp, C.POINTER(_i)]),
    "gfship_sim_set_source_fields": (_i, [_vp, C.POINTER(_i)]),
    "gfship_particles_time_spreading": (_i, [_vp, C.POINTER(_i), _pd]),
    "gfship_particulate_source_create": (_i, [C.POINTER(_vp), _vp, _i, C.c_char_p, _i, C.POINTER(C.c_char_p),
                                              C.POINTER(_i)]),
    "gfship_particulate_source_set_fields": (_i, [_vp, _i, C.POINTER(_i), _i]),
    "gfship_particulate_source_event": (_i, [_vp]),
    "gfship_particulate_source_time_event": (_i, [_vp, _pd]),
    "gfship_particulate_source_destroy": (None, [_vp]),
    "gfship_particles_download_volume": (_i, [_vp, _pd]),
    "gfship_feed_particle_create": (_i, [C.POINTER(_vp), _vp, C.c_char_p, C.c_char_p, _i, C.POINTER(C.c_char_p),
                                         C.POINTER(_i)]),
    "gfship_feed_particle_event": (_i, [_vp, _i, _pd]),
    "gfship_feed_particle_destroy": (None, [_vp]),
    "gfship_particles_set_idlast": (_i, [_vp, _i]),
    "gfship_particles_idlast": (_i, [_vp]),
    "gfship_tree_create": (_i, [C.POINTER(_vp), _i, C.c_void_p, _vp, _i]),
    "gfship_tree_create_sides": (_i, [C.POINTER(_vp), _i, C.c_void_p, _vp, _pi, _i]),
    "gfship_tree_set_bc": (_i, [_vp, _i, _i]),
    "gfship_tree_poisson_solve": (_i, [_vp, C.POINTER(MultilevelParams), _d]),
    "gfship_tree_destroy": (None, [_vp]),
    "gfship_tree_depth": (_i, [_vp]),
    "gfship_tree_dim": (_i, [_vp]),
    "gfship_tree_flags": (_i, [_vp, _i, C.POINTER(C.c_ubyte)]),
    "gfship_tree_upload": (_i, [_vp, _i, _i, _pd]),
    "gfship_tree_download": (_i, [_vp, _i, _i, _pd]),
    "gfship_tree_projection_params": (C.POINTER(MultilevelParams), [_vp, _i]),
    "gfship_tree_set_time": (_i, [_vp, _d, _d]),
    "gfship_tree_set_next_event": (_i, [_vp, _vp, _vp]),
    "gfship_tree_time": (_d, [_vp]),
    "gfship_tree_dt": (_d, [_vp]),
    "gfship_tree_iter": (_u, [_vp]),
    "gfship_tree_add_tracer": (_i, [_vp, _i]),
    "gfship_tree_set_bc_u": (_i, [_vp, _i, _i, _i]),
    "gfship_tree_set_viscosity": (_i, [_vp, _i, _d]),
    "gfship_tree_set_source": (_i, [_vp, _i, _d]),
    "gfship_tree_diffusion_params": (C.POINTER(MultilevelParams), [_vp, _i]),
    "gfship_tree_start": (_i, [_vp]),
    "gfship_tree_step": (_i, [_vp]),
    "gfship_tree_snapshot_bytes": (C.c_size_t, [_vp, _i]),
    "gfship_tree_snapshot_write": (_i, [_vp, _i, _pi, _vp, C.c_size_t]),
    "gfship_tree_snapshot_read": (_i, [_vp, _i, _pi, _vp, C.c_size_t]),
    "gfship_tree_restart": (_i, [_vp, _d, _u]),
    "gfship_tree_sweep_levels": (_i, [_vp, _i, _pi, _pi]),
    "gfship_tree_divergence": (_i, [_vp]),
    "gfship_tree_host_check": (_i, [_i, C.c_void_p, _vp, _pi, _u, C.POINTER(C.c_longlong)]),
    "gfship_tree_host_check_diffusion": (_i, [_i, C.c_void_p, _vp, _pi, _u, _d, C.POINTER(C.c_longlong)]),
    "gfship_tree_host_plan_digest": (_i, [_i, C.c_void_p, _vp, _pi, _u, C.POINTER(C.c_ulonglong)]),
    "gfship_tree_interpolate": (_i, [_vp, _i, _i, _pd, _pd, C.POINTER(C.c_ubyte)]),
    "gfship_tree_sampler_stats": (_i, [_vp, C.POINTER(C.c_longlong)]),
    "gfship_particles_create_tree": (_i, [C.POINTER(_vp), _vp, _i, _pd, C.POINTER(C.c_uint)]),
    "gfship_particulates_create_tree": (_i, [C.POINTER(_vp), _vp, _i, _pd, C.POINTER(C.c_uint), _pd, _pd, _pd]),
    "gfship_tree_particulate_field": (_i, [_vp, _i]),
    "gfship_tree_particles_forces_on_fluid": (_i, [_vp]),
    "gfship_tree_particles_set_kernel": (_i, [_vp, C.c_double, C.c_char_p]),
    "gfship_tree_particles_spread_forces": (_i, [_vp]),
    "gfship_tree_source_particulate_event": (_i, [_vp]),
    "gfship_tree_set_source_fields": (_i, [_vp, _i]),
    "gfship_tree_mac_source": (_i, [_vp, _i, _i]),
    "gfship_tree_particulate_source_create": (_i, [C.POINTER(_vp), _vp, _i, C.c_char_p, _i, C.POINTER(C.c_char_p),
                                                   C.POINTER(_i)]),
    "gfship_tree_particulate_source_set_fields": (_i, [_vp, _i, C.POINTER(_i), _i]),
    "gfship_tree_feed_particle_create": (_i, [C.POINTER(_vp), _vp, C.c_char_p, C.c_char_p, _i,
                                              C.POINTER(C.c_char_p), C.POINTER(_i)]),
    "gfship_tree_particles_set_idlast": (_i, [_vp, _i]),
    "gfship_tree_particles_idlast": (_i, [_vp]),
    "gfship_tag_droplets": (_i, [_vp, _i, _i, C.POINTER(C.c_uint)]),
    "gfship_tag_droplets_time": (_i, [_vp, _i, _i, _i, _pd]),
    "gfship_remove_droplets": (_i, [_vp, _i, _i, _i, C.c_double]),
    "gfship_droplet_to_particle_create": (_i, [C.POINTER(_vp), _vp, _i, _i, C.c_double, C.c_double, C.c_char_p, _i,
                                               C.POINTER(C.c_char_p), C.POINTER(_i)]),
    "gfship_droplet_to_particle_event": (_i, [_vp, C.POINTER(C.c_uint)]),
    "gfship_droplet_to_particle_destroy": (None, [_vp]),
    "gfship_tree_tag_droplets": (_i, [_vp, _i, C.POINTER(C.c_uint)]),
    "gfship_tree_tag_droplets_time": (_i, [_vp, _i, _i, _pd]),
    "gfship_tree_remove_droplets": (_i, [_vp, _i, _i, _i, C.c_double]),
    "gfship_tree_droplet_to_particle_create": (_i, [C.POINTER(_vp), _vp, _i, _i, C.c_double, C.c_double, C.c_char_p,
                                                    _i, C.POINTER(C.c_char_p), C.POINTER(_i)]),
    "gfship_tree_host_tag_droplets": (_i, [_i, C.c_void_p, _vp, _pi, C.c_longlong, _pd, C.c_longlong,
                                           C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_longlong)]),
}


UNIQUE_ID_BYTES = 128

# the families of gfship_domain_kernel_counts, in the order of the GFSHIP_KC_* constants of gfship.h
KERNEL_COUNT_NAMES = (
    "PREDICT_SWEEP", "PREDICT_SWEEP_MPI", "PREDICT_TILED", "PREDICT_TILED_MPI", "PREDICT_GENERAL",
    "ADVECT3_SWEEP2", "ADVECT3_SWEEP2_MPI", "ADVECT3_SWEEP1", "ADVECT3_TILED", "ADVECT3_TILED_MPI",
    "ADVECT1_TILED_VELOCITY", "ADVECT1_TILED_TRACER", "ADVECT_GENERAL", "CORRECTION_FUSED",
    "CORRECTION_DECLINED", "DIVERGENCE_FUSED", "DIVERGENCE_DECLINED", "DIVERGENCE_SEPARATE",
    "PROJECT_PAIRS", "PROJECT_SCALAR", "RESIDUAL_PAIRS", "RESIDUAL_SCALAR", "RN_BLOCKS_LIMIT",
    "RN_BLOCKS_MAX", "ROWS2D", "HYPERPLANES_2D", "DIFFUSION_PIPELINED", "DIFFUSION_HYPERPLANES",
    "WEIGHTED_PIPELINED", "WEIGHTED_HYPERPLANES", "PROLONGATION_FUSED", "PROLONGATION_DECLINED",
    "RESTRICTION_FUSED", "RESTRICTION_DECLINED", "PROLONG_PACK_NEW", "PROLONG_PACK_OLD",
    "ARM_AHEAD", "ARM_AHEAD_DECLINED", "ARM_INLINE", "PATCH_LOOP_KERNEL_ARMS",
    "PATCH_LOOP_HOST_ARMS", "XCD_SCOPE_ON", "XCD_SCOPE_OFF", "XCD_NEAR_MODE", "XCD_PLACE_ON",
    "XCD_PLACE_OFF", "COARSE_CYCLES", "COARSE_THREADS", "COARSE_END_BY_LEVEL",
    "DIFFUSION_FACES_PIPELINED", "DIFFUSION_FACES_HYPERPLANES",
)
# ... of which these hold a value (a limit, a thread count, a mode) instead of a tally
KERNEL_COUNT_VALUES = ("RN_BLOCKS_LIMIT", "RN_BLOCKS_MAX", "XCD_NEAR_MODE", "COARSE_THREADS")


def comm_available():
    """RCCL can be opened on this rank (gfship_comm_available); raises otherwise"""
    _check(lib().gfship_comm_available())


def comm_unique_id():
    """ncclGetUniqueId through the library (gfship_comm_unique_id): bytes for Domain.comm_init"""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _check(lib().gfship_comm_unique_id(buf))
    return buf.raw


def lib():
    """Load libgfship.so; raises if it was not built (no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GfshipError("%s not found: run __graft_entry__.build() "
                              "(gerris-fft-particles_amd/csrc/build.sh)" % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64
        # and loads them by unversioned names, so if libgfship pulled in /opt/rocm's copy first a
        # later `import torch` would start a second HSA runtime that finds no GPU.  Loading torch
        # first makes libgfship's NEEDED libamdhip64.so.7 resolve to the already loaded runtime.
        # (A C host that never loads torch uses /opt/rocm's runtime directly.)
        if "torch" not in sys.modules and os.environ.get("GFSHIP_NO_TORCH") is None:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)   # AttributeError if the library lacks a declared symbol
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise GfshipError("gfship error %d: %s" % (rc, lib().gfship_last_error().decode()))
    return rc


class Variable:
    """A GfsVariable living on the device (all levels)."""

    def __init__(self, dom, component=-1):
        self.dom = dom
        self.h = _check(lib().gfship_field_alloc(dom.ptr, component))

    def _shape(self, level):
        return ((1 << level) + 2,) * self.dom.dim

    def upload(self, a, level=None):
        level = self.dom.depth if level is None else level
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == self._shape(level), (a.shape, self._shape(level))
        _check(lib().gfship_field_upload(self.dom.ptr, self.h, level, a.ctypes.data_as(_pd)))

    def download(self, level=None):
        level = self.dom.depth if level is None else level
        a = np.empty(self._shape(level), dtype=np.float64)
        _check(lib().gfship_field_download(self.dom.ptr, self.h, level, a.ctypes.data_as(_pd)))
        return a

    def fill(self, value, level=None):
        level = self.dom.depth if level is None else level
        _check(lib().gfship_field_fill(self.dom.ptr, self.h, level, value))

    def set_bc(self, d, kind, val=None):
        if val is not None:
            val = np.ascontiguousarray(val, dtype=np.float64).ravel()
            p = val.ctypes.data_as(_pd)
        else:
            p = None
        _check(lib().gfship_field_set_bc(self.dom.ptr, self.h, d, kind, p))

    def free(self):
        if self.h is not None and self.dom.ptr:
            lib().gfship_field_free(self.dom.ptr, self.h)
            self.h = None


class Domain:
    """One uniform GfsBox on one GPU."""

    def __init__(self, dim, depth, side=None, device=0):
        self.dim, self.depth = dim, depth
        s = (C.c_int * 6)(*(side if side is not None else [SIDE_BOUNDARY] * 6))
        p = _vp()
        _check(lib().gfship_domain_create(C.byref(p), dim, depth, s, device))
        self.ptr = p

    def variable(self, component=-1):
        return Variable(self, component)

    def params(self):
        par = MultilevelParams()
        lib().gfship_multilevel_params_init(C.byref(par), self.dim)
        return par

    def comm_init(self, unique_id, rank, nranks, lattice):
        """in-library RCCL transport: this box is rank `rank` of a periodic lattice of boxes, one
        per GPU (gfship_domain_comm_init); unique_id = comm_unique_id() of one rank"""
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        _check(lib().gfship_domain_comm_init(self.ptr, buf, rank, nranks, (C.c_int * 3)(*lattice)))

    def comm_size(self):
        return _check(lib().gfship_domain_comm_size(self.ptr))

    def comm_stats(self):
        m, b = C.c_ulonglong(), C.c_ulonglong()
        _check(lib().gfship_domain_comm_stats(self.ptr, C.byref(m), C.byref(b)))
        return int(m.value), int(b.value)

    def path_counts(self):
        """(coarse ends of V-cycles computed for the whole lattice, tiled Godunov launches with MPI sides)"""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        _check(lib().gfship_domain_path_counts(self.ptr, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kernel_counts(self):
        """{family: tally} of gfship_domain_kernel_counts: which branch of every switchable dispatch has
        run on this domain (KERNEL_COUNT_NAMES; the families of KERNEL_COUNT_VALUES hold a value)"""
        n = len(KERNEL_COUNT_NAMES)
        a = (C.c_ulonglong * n)()
        _check(lib().gfship_domain_kernel_counts(self.ptr, a, n))
        return {name: int(a[k]) for k, name in enumerate(KERNEL_COUNT_NAMES)}

    def snapshot_tree(self, variables):
        """the binary cell data of a GfsBox (gfship_snapshot_tree_write) as bytes"""
        n = len(variables)
        h = (C.c_int * n)(*[v.h for v in variables])
        size = lib().gfship_snapshot_tree_bytes(self.ptr, n)
        buf = C.create_string_buffer(size)
        _check(lib().gfship_snapshot_tree_write(self.ptr, n, h, buf, size))
        return buf.raw

    def snapshot_tree_read(self, variables, data):
        n = len(variables)
        h = (C.c_int * n)(*[v.h for v in variables])
        buf = C.create_string_buffer(bytes(data), len(data))
        _check(lib().gfship_snapshot_tree_read(self.ptr, n, h, buf, len(data)))

    def set_overlap(self, overlap):
        _check(lib().gfship_domain_set_overlap(self.ptr, int(overlap)))

    def set_relax_mode(self, mode):
        _check(lib().gfship_domain_set_relax_mode(self.ptr, mode))

    def synchronize(self):
        _check(lib().gfship_domain_synchronize(self.ptr))

    def bc(self, v, v1=None, level=None):
        level = self.depth if level is None else level
        _check(lib().gfship_bc(self.ptr, v.h, (v1 or v).h, level))

    def tag_droplets(self, c, tag):
        """gfs_domain_tag_droplets: the leaves of `tag' get the index (1 ..) of their droplet of c, 0 outside;
        returns the number of droplets"""
        n = C.c_uint(0)
        _check(lib().gfship_tag_droplets(self.ptr, c.h, tag.h, C.byref(n)))
        return int(n.value)

    def time_tag_droplets(self, c, tag, reps=10):
        """tag_droplets, measured between two events after a warm-up call: milliseconds per call"""
        ms = C.c_double(0.)
        _check(lib().gfship_tag_droplets_time(self.ptr, c.h, tag.h, int(reps), C.byref(ms)))
        return float(ms.value)

    def remove_droplets(self, c, v, min, val=0.):
        """gfs_domain_remove_droplets: v = val in the droplets of c smaller than min cells (min < 0: all but the
        -min largest)"""
        _check(lib().gfship_remove_droplets(self.ptr, c.h, v.h, int(min), float(val)))

    def homogeneous_bc(self, ov, v, level=None):
        level = self.depth if level is None else level
        _check(lib().gfship_homogeneous_bc(self.ptr, ov.h, v.h, level))

    def poisson_coefficients(self):
        _check(lib().gfship_poisson_coefficients(self.ptr))

    def poisson_coefficients_alpha(self, alpha):
        """alpha: dim Variables holding the face values of the GfsFunction alpha"""
        h = (C.c_int * 3)(*([v.h for v in alpha] + [-1] * (3 - len(alpha))))
        _check(lib().gfship_poisson_coefficients_alpha(self.ptr, h))

    def poisson_weight(self, d, level=None):
        """f[d].v of the cells of a level (host array with ghosts)"""
        w = C.c_int()
        _check(lib().gfship_poisson_weights(self.ptr, d, C.byref(w)))
        v = Variable.__new__(Variable)
        v.dom, v.h = self, w.value
        a = v.download(level)
        v.h = None
        return a

    def relax(self, u, rhs, dia, level=None, omega=1., d=None):
        level = self.depth if level is None else level
        _check(lib().gfship_relax(self.ptr, d or self.dim, level, omega, u.h, rhs.h, dia.h))

    def residual(self, u, rhs, dia, res, level=None, d=None):
        level = self.depth if level is None else level
        _check(lib().gfship_residual(self.ptr, d or self.dim, level, u.h, rhs.h, dia.h, res.h))

    def norm_residual(self, res, dt=1.):
        n = Norm()
        _check(lib().gfship_norm_residual(self.ptr, dt, res.h, C.byref(n)))
        return n

    def norm_variable(self, v):
        n = Norm()
        _check(lib().gfship_norm_variable(self.ptr, v.h, C.byref(n)))
        return n

    def poisson_cycle(self, par, u, rhs, dia, res):
        _check(lib().gfship_poisson_cycle(self.ptr, C.byref(par), u.h, rhs.h, dia.h, res.h))

    def poisson_solve(self, par, lhs, rhs, res, dia, dt=1.):
        _check(lib().gfship_poisson_solve(self.ptr, C.byref(par), lhs.h, rhs.h, res.h, dia.h, dt))

    def diffusion_coefficients(self, D, dt, rhoc, beta=1.):
        _check(lib().gfship_diffusion_coefficients(self.ptr, D, dt, rhoc.h, beta))

    def diffusion_coefficients_faces(self, D, dt, rhoc, alpha_cell=None, beta=1.):
        """D: dim Variables holding the diffusion coefficient at the leaf faces (the layout of
        poisson_coefficients_alpha); alpha_cell: a Variable holding alpha on every level, or None"""
        h = (C.c_int * 3)(*([v.h for v in D] + [-1] * (3 - len(D))))
        _check(lib().gfship_diffusion_coefficients_faces(self.ptr, h, dt, rhoc.h,
                                                         -1 if alpha_cell is None else alpha_cell.h, beta))

    def diffusion_rhs(self, v, rhs, rhoc, beta=1.):
        _check(lib().gfship_diffusion_rhs(self.ptr, v.h, rhs.h, rhoc.h, beta))

    def diffusion_residual(self, u, rhs, rhoc, res):
        _check(lib().gfship_diffusion_residual(self.ptr, u.h, rhs.h, rhoc.h, res.h))

    def diffusion_cycle(self, levelmin, nrelax, u, rhs, rhoc, res):
        _check(lib().gfship_diffusion_cycle(self.ptr, levelmin, self.depth, nrelax,
                                            u.h, rhs.h, rhoc.h, res.h))

    def diffusion(self, par, v, rhs, rhoc):
        _check(lib().gfship_diffusion(self.ptr, C.byref(par), v.h, rhs.h, rhoc.h))

    def time_relax_loop(self, u, rhs, dia, nrelax=4, level=None, reps=5):
        """(ms per relax loop of the sweep kernels alone, fused?)"""
        level = self.depth if level is None else level
        ms, fused = C.c_double(), C.c_int()
        _check(lib().gfship_time_relax_loop(self.ptr, level, u.h, rhs.h, dia.h, nrelax, reps,
                                            C.byref(ms), C.byref(fused)))
        return ms.value, bool(fused.value)

    def time_relax_loop_inclusive(self, u, rhs, dia, nrelax=4, level=None, reps=5):
        """(ms of the sweep kernels alone, fused?, ms of the whole loop as a V-cycle pays for it)"""
        level = self.depth if level is None else level
        ms, fused, incl = C.c_double(), C.c_int(), C.c_double()
        _check(lib().gfship_time_relax_loop_inclusive(self.ptr, level, u.h, rhs.h, dia.h, nrelax, reps,
                                                      C.byref(ms), C.byref(fused), C.byref(incl)))
        return ms.value, bool(fused.value), incl.value

    def energy_spectra(self, comps):
        """GfsOutputEnergySpectra of the variables comps (U, V[, W]): (k, Ek, Etot) as the reference
        prints them (modules/fft.c:1340-1348)"""
        nk = _check(lib().gfship_energy_spectra_bins(self.ptr))
        Ek = np.empty(nk)
        etot, dk = C.c_double(), C.c_double()
        h = (_i * len(comps))(*[c.h for c in comps])
        _check(lib().gfship_energy_spectra(self.ptr, len(comps), h, Ek.ctypes.data_as(_pd),
                                           C.byref(etot), C.byref(dk)))
        i = np.arange(1, nk)
        return dk.value * np.sqrt(i.astype(float)), Ek[1:].copy(), etot.value

    def output_spectra(self, v):
        """GfsOutputSpectra of variable v on the whole 3-D domain: (F, kstep) with F the complex
        array [ix][iy][iz <= N/2] of the r2c DFT of (v - <v>)/ntot (modules/fft.c:1101-1160)"""
        N = _check(lib().gfship_output_spectra_side(self.ptr))
        out = np.empty((N, N, N // 2 + 1), dtype=np.complex128)
        ks = C.c_double()
        _check(lib().gfship_output_spectra(self.ptr, v.h, out.ctypes.data_as(_pd), C.byref(ks)))
        return out, ks.value

    def output_spectra_plane(self, v, normal, pos):
        """GfsOutputSpectra of a plane of the 3-D box (realdim == 2): (F, kstep), F[ia][ib] the full N x N
        2-D DFT of the cell values on the plane minus their mean over their number, ia / ib the first /
        second in-plane coordinate (what fftw_plan_dft_r2c_3d (N, N, 1) leaves: modules/fft.c:795-820)"""
        N = _check(lib().gfship_output_spectra_side(self.ptr))
        out = np.empty((N, N), dtype=np.complex128)
        ks = C.c_double()
        _check(lib().gfship_output_spectra_plane(self.ptr, v.h, int(normal), float(pos),
                                                 out.ctypes.data_as(_pd), C.byref(ks)))
        return out, ks.value

    def turbulent_viscosity(self, u, Cs, out, model=1):
        """GfsVariableTurbulentViscosity (modules/turbulence.c:953-1105): model 1 Smagorinsky, 0 sigma"""
        h = (_i * 3)(*([c.h for c in u] + [u[-1].h] * (3 - len(u))))
        _check(lib().gfship_turbulent_viscosity(self.ptr, h, float(Cs), int(model), out.h))

    def init_spectra(self, par, fields):
        """GfsInitSpectra (modules/turbulence.c): par = dict with the keywords of the .gfs object
        (x0 y0 z0 L E alpha epsilon c1 c2 c3 ReL kmax seed level)"""
        p = InitSpectraParams()
        for k, v in par.items():
            setattr(p, k, v)
        h = (_i * 3)(*[f.h for f in fields])
        _check(lib().gfship_init_spectra(self.ptr, C.byref(p), h))

    def interpolate(self, v, points):
        """GfsOutputLocation sampling: (values, inside) of variable v at points (np x 3)"""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        inside = np.empty(len(pts), dtype=np.uint8)
        _check(lib().gfship_field_interpolate(self.ptr, v.h, len(pts), pts.ctypes.data_as(_pd),
                                              out.ctypes.data_as(_pd),
                                              inside.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out, inside.astype(bool)

    def time_relax(self, u, rhs, dia, level=None, reps=10, d=None):
        level = self.depth if level is None else level
        ms = C.c_double()
        _check(lib().gfship_time_relax(self.ptr, d or self.dim, level, u.h, rhs.h, dia.h, reps,
                                       C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.ptr:
            lib().gfship_domain_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class _SimVariable(Variable):
    """A variable owned by a Simulation (P, Pmac, U, ...)."""

    def __init__(self, dom, handle):
        self.dom, self.h = dom, handle

    def free(self):
        pass


class Simulation:
    """GfsSimulation on one box: the simulation_run loop (src/simulation.c:432-557)."""
    VAR_P, VAR_PMAC, VAR_U, VAR_G, VAR_GMAC, VAR_TRACER, VAR_UN = range(7)

    def __init__(self, dom):
        self.dom = dom
        p = _vp()
        _check(lib().gfship_sim_create(C.byref(p), dom.ptr))
        self.ptr = p
        self.end = 1.7976931348623157e308
        L = lib()
        dim = dom.dim
        self.p = self._var(self.VAR_P)
        self.pmac = self._var(self.VAR_PMAC)
        self.u = [self._var(self.VAR_U, c) for c in range(dim)]
        self._g = None
        self.gmac = [self._var(self.VAR_GMAC, c) for c in range(dim)]
        self.projection_params = L.gfship_sim_projection_params(self.ptr).contents
        self.approx_projection_params = L.gfship_sim_approx_projection_params(self.ptr).contents
        self.advection_params = L.gfship_sim_advection_params(self.ptr).contents

    def _var(self, which, c=0):
        return _SimVariable(self.dom, _check(lib().gfship_sim_variable(self.ptr, which, c)))

    @property
    def g(self):
        """the centred pressure gradient: the handles are fetched on first use, and from then on the time
        step stores g (a simulation whose g nobody asks for leaves it unstored between steps)"""
        if self._g is None:
            self._g = [self._var(self.VAR_G, c) for c in range(self.dom.dim)]
        return self._g

    def set_source(self, c, g):
        """GfsSource {} U/V/W g: constant intensity"""
        _check(lib().gfship_sim_set_source(self.ptr, c, float(g)))

    def set_alpha(self, alpha):
        """GfsPhysicalParams { alpha }: dim Variables of face values (None: alpha = NULL)"""
        if alpha is None:
            _check(lib().gfship_sim_set_alpha(self.ptr, None))
            return
        h = (C.c_int * 3)(*([v.h for v in alpha] + [-1] * (3 - len(alpha))))
        _check(lib().gfship_sim_set_alpha(self.ptr, h))

    def set_viscosity(self, c, nu):
        """SourceDiffusion {} U|V|W nu"""
        _check(lib().gfship_sim_set_viscosity(self.ptr, c, nu))

    def set_viscosity_faces(self, c, D):
        """SourceDiffusion {} U|V|W f(x,y,z,t): dim Variables of face values (None removes it)"""
        if D is None:
            _check(lib().gfship_sim_set_viscosity_faces(self.ptr, c, None))
            return
        h = (C.c_int * 3)(*([v.h for v in D] + [-1] * (3 - len(D))))
        _check(lib().gfship_sim_set_viscosity_faces(self.ptr, c, h))

    def set_source_fields(self, F):
        """the velocity source of GfsSourceParticulate: dim Variables read as centred and MAC source of
        U, V, W (None removes it)"""
        if F is None:
            _check(lib().gfship_sim_set_source_fields(self.ptr, None))
            return
        h = (C.c_int * 3)(*([v.h for v in F] + [-1] * (3 - len(F))))
        _check(lib().gfship_sim_set_source_fields(self.ptr, h))

    def set_alpha_cell(self, alpha_cell):
        """alpha at the cell centres of every level: a Variable (None removes it)"""
        _check(lib().gfship_sim_set_alpha_cell(self.ptr, -1 if alpha_cell is None else alpha_cell.h))

    def set_viscosity_cell(self, mu):
        """the viscosity of U at the centres of the leaf cells, read by particle forces: a Variable (None
        removes it)"""
        _check(lib().gfship_sim_set_viscosity_cell(self.ptr, -1 if mu is None else mu.h))

    def variable_mac_source(self, c, out):
        """gfs_variable_mac_source of velocity component c into the Variable out"""
        _check(lib().gfship_variable_mac_source(self.ptr, c, out.h))

    def diffusion_params(self, c):
        return lib().gfship_sim_diffusion_params(self.ptr, c).contents

    def add_tracer(self, gradient=None):
        """GfsVariableTracer; gradient 0 = gfs_center_gradient, 1 = van Leer (the default)"""
        t = _check(lib().gfship_sim_add_tracer(self.ptr))
        if gradient is not None:
            _check(lib().gfship_sim_set_tracer_gradient(self.ptr, t, gradient))
        v = self._var(self.VAR_TRACER, t)
        v.tracer_index = t
        return v

    @staticmethod
    def _tracer(t):
        """the index of a tracer: the Variable add_tracer returned, or the index itself"""
        return t if isinstance(t, int) else t.tracer_index

    def set_tracer_diffusion(self, t, D):
        """SourceDiffusion T D on a tracer (0. removes it)"""
        _check(lib().gfship_sim_set_tracer_diffusion(self.ptr, self._tracer(t), float(D)))

    def tracer_diffusion_params(self, t):
        """the GfsMultilevelParams of the diffusion of a tracer (tolerance 1e-6, beta 1)"""
        p = lib().gfship_sim_tracer_diffusion_params(self.ptr, self._tracer(t))
        if not p:
            raise GfshipError("no tracer %r" % (t,))
        return p.contents

    def set_tracer_scheme(self, t, scheme):
        """VariableTracer T { scheme = godunov | none }: SCHEME_GODUNOV, SCHEME_NONE"""
        _check(lib().gfship_sim_set_tracer_scheme(self.ptr, self._tracer(t), scheme))

    def tracer_diffusion_path(self, fused):
        """1: the start of a tracer's diffusion solve in one pass where it applies (the default), 0: composed"""
        _check(lib().gfship_sim_tracer_diffusion_path(self.ptr, int(fused)))

    def tracer_diffusion_counts(self):
        """(fused, composed): the solves each path has started"""
        c = (C.c_ulonglong * 2)()
        _check(lib().gfship_sim_tracer_diffusion_counts(self.ptr, c))
        return int(c[0]), int(c[1])

    def mac_velocity(self, c):
        """MAC velocity of the + face of every cell along c (GFSHIP_VAR_UN)"""
        return self._var(self.VAR_UN, c)

    def gradients_unstored(self):
        """how many projections of step() have left their centred gradient unstored so far"""
        c = C.c_ulonglong()
        _check(lib().gfship_sim_gradients_unstored(self.ptr, C.byref(c)))
        return int(c.value)

    def advection_step(self):
        """loop body of advection_run (GfsAdvection) with the MAC velocities as they are"""
        _check(lib().gfship_sim_advection_step(self.ptr))

    def set_time(self, end=1.7976931348623157e308, dtmax=1.7976931348623157e308):
        self.end = end
        _check(lib().gfship_sim_set_time(self.ptr, end, dtmax))

    @property
    def t(self):
        return lib().gfship_sim_time(self.ptr)

    @property
    def i(self):
        return lib().gfship_sim_iter(self.ptr)

    @property
    def dt(self):
        return self.advection_params.dt

    def restart(self, t, i):
        _check(lib().gfship_sim_restart(self.ptr, t, i))

    def start(self):
        _check(lib().gfship_sim_start(self.ptr))

    def step(self):
        _check(lib().gfship_sim_step(self.ptr))

    def predicted_face_velocities(self):
        _check(lib().gfship_predicted_face_velocities(self.ptr))

    def cfl(self):
        v = C.c_double()
        _check(lib().gfship_domain_cfl(self.ptr, C.byref(v)))
        return v.value

    def divergence_norm(self):
        n = Norm()
        _check(lib().gfship_divergence_norm(self.ptr, C.byref(n)))
        return n

    def tracer_advection(self, t, dt):
        _check(lib().gfship_tracer_advection(self.ptr, t.h, dt))

    @staticmethod
    def _handles(v):
        return (C.c_int * 3)(*([f.h for f in v] + [-1] * (3 - len(v))))

    def mac_projection(self, par, dt, p, g):
        """gfs_mac_projection on the MAC velocities as they are; par: one of the parameter structs"""
        _check(lib().gfship_mac_projection(self.ptr, C.byref(par), dt, p.h, self._handles(g)))

    def approximate_projection(self, par, dt, p, g):
        _check(lib().gfship_approximate_projection(self.ptr, C.byref(par), dt, p.h, self._handles(g)))

    def centered_velocity_advection(self, gmac, g=None):
        _check(lib().gfship_centered_velocity_advection(self.ptr, self._handles(gmac),
                                                        self._handles(g) if g is not None else None))

    def correct_centered_velocities(self, g, dt):
        _check(lib().gfship_correct_centered_velocities(self.ptr, self._handles(g), dt))

    def set_timestep(self):
        _check(lib().gfship_set_timestep(self.ptr))

    def coarse_init(self):
        _check(lib().gfship_coarse_init(self.ptr))

    def advance_time(self):
        """t = tnext, i++ (the end of the loop body of simulation_run)"""
        _check(lib().gfship_sim_advance_time(self.ptr))

    NEXT_EVENT_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_double, C.c_uint)

    def set_next_event(self, fn):
        """fn (t, i) -> the tnext the host's events give (None: no events)"""
        self._next_event = None if fn is None else self.NEXT_EVENT_FN(lambda ctx, t, i: float(fn(t, i)))
        _check(lib().gfship_sim_set_next_event(
            self.ptr, None if fn is None else C.cast(self._next_event, C.c_void_p), None))

    def un(self, c):
        n = (1 << self.dom.depth) + 2
        a = np.empty((n,) * self.dom.dim)
        _check(lib().gfship_sim_download_un(self.ptr, c, a.ctypes.data_as(_pd)))
        return a

    def destroy(self):
        if self.ptr:
            lib().gfship_sim_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if self.dom.ptr:
                self.destroy()
        except Exception:
            pass


FORCE_INERTIAL, FORCE_ADDEDMASS, FORCE_LIFT, FORCE_DRAG, FORCE_BUOY = 1, 2, 3, 4, 5


class InitSpectraParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("x0", "y0", "z0", "L", "E", "alpha", "epsilon", "c1", "c2",
                                           "c3", "ReL", "kmax", "seed")] + [("level", C.c_int)]


class ParticleList:
    """GfsParticleList of GfsParticle tracers on the device; sim: a Simulation, or a Tree (tracers, or with
    particulate = (vel, mass, volume) a list of GfsParticulate: Tree.particulates)."""

    def __init__(self, sim, pos, ids, particulate=None):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        assert len(pos) == len(ids)
        self.sim, self.n0 = sim, len(ids)
        p = _vp()
        if particulate is not None:
            assert isinstance(sim, Tree)
            vel = np.ascontiguousarray(particulate[0], dtype=np.float64).reshape(-1, 3)
            mass = np.ascontiguousarray(particulate[1], dtype=np.float64)
            volume = np.ascontiguousarray(particulate[2], dtype=np.float64)
            assert len(vel) == len(mass) == len(volume) == len(ids)
            _check(lib().gfship_particulates_create_tree(
                C.byref(p), sim.ptr, len(ids), pos.ctypes.data_as(_pd), ids.ctypes.data_as(C.POINTER(C.c_uint)),
                vel.ctypes.data_as(_pd), mass.ctypes.data_as(_pd), volume.ctypes.data_as(_pd)))
            self.ptr = p
            return
        create = lib().gfship_particles_create_tree if isinstance(sim, Tree) else lib().gfship_particles_create
        _check(create(C.byref(p), sim.ptr, len(ids), pos.ctypes.data_as(_pd),
                      ids.ctypes.data_as(C.POINTER(C.c_uint))))
        self.ptr = p

    def event(self):
        _check(lib().gfship_particle_list_event(self.ptr))

    def sort(self):
        _check(lib().gfship_particles_sort(self.ptr))

    def set_sort_interval(self, every):
        _check(lib().gfship_particles_set_sort_interval(self.ptr, every))

    def count(self):
        return _check(lib().gfship_particles_count(self.ptr))

    def download(self):
        m = max(_check(lib().gfship_particles_slots(self.ptr)), 1)
        pos = np.empty((m, 3))
        ids = np.empty(m, dtype=np.uint32)
        k = _check(lib().gfship_particles_download(self.ptr, pos.ctypes.data_as(_pd),
                                                   ids.ctypes.data_as(C.POINTER(C.c_uint))))
        return pos[:k].copy(), ids[:k].copy()

    def download_old(self):
        """pos_old of the particles on the list, in the order of download()"""
        m = max(_check(lib().gfship_particles_slots(self.ptr)), 1)
        old = np.empty((m, 3))
        k = _check(lib().gfship_particles_download_old(self.ptr, old.ctypes.data_as(_pd)))
        return old[:k].copy()

    # GfsParticulate: velocity, mass, volume and the list's forces (FORCE_* in application order)
    def set_particulate(self, vel, mass, volume):
        vel = np.ascontiguousarray(vel, dtype=np.float64).reshape(-1, 3)
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        volume = np.ascontiguousarray(volume, dtype=np.float64)
        _check(lib().gfship_particles_set_particulate(self.ptr, vel.ctypes.data_as(_pd),
                                                      mass.ctypes.data_as(_pd),
                                                      volume.ctypes.data_as(_pd)))

    def set_forces(self, kinds, gravity=(0., 0., 0.)):
        k = (_i * len(kinds))(*kinds)
        g = (C.c_double * 3)(*gravity)
        _check(lib().gfship_particles_set_forces(self.ptr, len(kinds), k, g))

    def set_force_coefficient(self, force, function):
        """the GfsFunction (C text of Rep, Urelp, Vrelp, Wrelp, Pdia, t) of force number `force' of the
        list: compiled for the device with hipRTC"""
        _check(lib().gfship_particles_set_force_coefficient(self.ptr, int(force), function.encode()))

    def particulate_state(self):
        """(vel, mass, force) of the particles on the list, in list order"""
        m = max(_check(lib().gfship_particles_slots(self.ptr)), 1)
        vel, mass, force = np.empty((m, 3)), np.empty(m), np.empty((m, 3))
        k = _check(lib().gfship_particles_download_particulate(
            self.ptr, vel.ctypes.data_as(_pd), mass.ctypes.data_as(_pd), force.ctypes.data_as(_pd)))
        return vel[:k].copy(), mass[:k].copy(), force[:k].copy()

    # two-way coupling: GfsParticulateField and the event of GfsSourceParticulate
    def particulate_field(self, v):
        """v = the volume fraction of the particles of the list (GfsParticulateField)"""
        _check(lib().gfship_particulate_field(self.ptr, v.h))

    def forces_on_fluid(self):
        """the stored force of every particle = its forces but buoyancy, times its volume"""
        _check(lib().gfship_particles_forces_on_fluid(self.ptr))

    def set_kernel(self, rkernel, function=None):
        """rkernel (a length) and kernel (C text of x, y, z, t; a number; None = 0) of GfsSourceParticulate"""
        _check(lib().gfship_particles_set_kernel(
            self.ptr, float(rkernel), None if function is None else str(function).encode()))

    def _fields3(self, F):
        h = [f.h for f in F] + [-1] * (3 - len(F))
        return (_i * 3)(*h)

    def spread_forces(self, F):
        """F[c] = minus the stored forces spread around the particles with the kernel"""
        _check(lib().gfship_particles_spread_forces(self.ptr, self._fields3(F)))

    def time_spreading(self, F):
        """spread_forces, measured: (ms of pass 1, ms of pass 2, record slots per particle, particles per
        chunk, bytes of the record arrays)"""
        info = (C.c_double * 5)()
        _check(lib().gfship_particles_time_spreading(self.ptr, self._fields3(F), info))
        return float(info[0]), float(info[1]), int(info[2]), int(info[3]), int(info[4])

    def source_particulate_event(self, F):
        """forces_on_fluid, then spread_forces"""
        _check(lib().gfship_source_particulate_event(self.ptr, self._fields3(F)))

    def volumes(self):
        """the volume of the particles on the list, in list order"""
        m = max(_check(lib().gfship_particles_slots(self.ptr)), 1)
        vol = np.empty(m)
        k = _check(lib().gfship_particles_download_volume(self.ptr, vol.ctypes.data_as(_pd)))
        return vol[:k].copy()

    @property
    def idlast(self):
        """idlast of the GfsParticleList: the id the last particle a FeedParticle added took (lists of a box)"""
        return _check(lib().gfship_particles_idlast(self.ptr))

    @idlast.setter
    def idlast(self, value):
        _check(lib().gfship_particles_set_idlast(self.ptr, int(value)))

    def destroy(self):
        if self.ptr:
            lib().gfship_particles_destroy(self.ptr)
            self.ptr = None


SOURCE_VOLUME, SOURCE_MASS = 0, 1


class ParticulateSource:
    """GfsSourceParticulateVol (kind = SOURCE_VOLUME) or GfsSourceParticulateMass (SOURCE_MASS) on a list of
    particulates of a uniform box.  function: C text of Rad, Urelp, Vrelp, Wrelp (3-D), x, y, z, t and of the
    names of `variables' (a dict name -> Variable), a number, or None (the constant 0)."""

    def __init__(self, plist, kind, function=None, variables=None):
        variables = dict(variables or {})
        names = (C.c_char_p * max(len(variables), 1))(*[k.encode() for k in variables])
        fields = (_i * max(len(variables), 1))(*[v.h for v in variables.values()])
        p = _vp()
        _check(lib().gfship_particulate_source_create(
            C.byref(p), plist.ptr, int(kind), None if function is None else str(function).encode(),
            len(variables), names, fields))
        self.ptr, self.plist = p, plist

    def set_fields(self, rad=None, urel=(), deposit=None):
        """the Variables Rad, (Urelp, Vrelp[, Wrelp]) and the deposit variable; None: not written"""
        u = [v.h if v is not None else -1 for v in urel] + [-1] * (3 - len(urel))
        _check(lib().gfship_particulate_source_set_fields(
            self.ptr, -1 if rad is None else rad.h, (_i * 3)(*u), -1 if deposit is None else deposit.h))

    def event(self):
        _check(lib().gfship_particulate_source_event(self.ptr))

    def time_event(self):
        """event, measured: (ms of the passes per particle, ms of the sort and the pass per cell)"""
        info = (C.c_double * 2)()
        _check(lib().gfship_particulate_source_time_event(self.ptr, info))
        return float(info[0]), float(info[1])

    def destroy(self):
        if self.ptr:
            lib().gfship_particulate_source_destroy(self.ptr)
            self.ptr = None


class FeedParticle:
    """GfsFeedParticle on a list of particulates of a uniform box.  mass, volume: C text of x, y, z, t and of the
    names of `variables' (a dict name -> Variable), a number, or None (the constant 0: nothing is fed without a
    mass).  Close it before its list."""

    def __init__(self, plist, mass=None, volume=None, variables={}):
        variables = dict(variables or {})
        names = (C.c_char_p * max(len(variables), 1))(*[k.encode() for k in variables])
        fields = (_i * max(len(variables), 1))(*[v.h for v in variables.values()])
        p = _vp()
        _check(lib().gfship_feed_particle_create(
            C.byref(p), plist.ptr, None if mass is None else str(mass).encode(),
            None if volume is None else str(volume).encode(), len(variables), names, fields))
        self.ptr, self.plist = p, plist

    def event(self, pos):
        """the candidates pos, an (np, 3) array, in order: those with a cell and a mass join the end of the list"""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        _check(lib().gfship_feed_particle_event(self.ptr, len(pos), pos.ctypes.data_as(_pd)))

    def close(self):
        if self.ptr:
            lib().gfship_feed_particle_destroy(self.ptr)
            self.ptr = None


class DropletToParticle:
    """GfsDropletToParticle on a list of particulates of a uniform box: the droplets of the Variable c (or of
    `function': C text of x, y, z, t and of the names of `variables', a number, or the name of one of them) smaller
    than min cells become particulates, and c = reset there.  Close it before its list."""

    def __init__(self, plist, c, min=20, reset=0., density=1., function=None, variables=None):
        variables = dict(variables or {})
        names = (C.c_char_p * max(len(variables), 1))(*[k.encode() for k in variables])
        fields = (_i * max(len(variables), 1))(*[v.h for v in variables.values()])
        p = _vp()
        _check(lib().gfship_droplet_to_particle_create(
            C.byref(p), plist.ptr, c.h, int(min), float(reset), float(density),
            None if function is None else str(function).encode(), len(variables), names, fields))
        self.ptr, self.plist = p, plist

    def event(self):
        """one event; returns (droplets, the min used, particles made, cells reset)"""
        info = (C.c_uint * 4)()
        _check(lib().gfship_droplet_to_particle_event(self.ptr, info))
        return tuple(int(v) for v in info)

    def close(self):
        if self.ptr:
            lib().gfship_droplet_to_particle_destroy(self.ptr)
            self.ptr = None


class TreeParticulateSource(ParticulateSource):
    """GfsSourceParticulateVol (kind = SOURCE_VOLUME) or GfsSourceParticulateMass (SOURCE_MASS) on a list of
    Tree.particulates.  function: as for ParticulateSource; variables: a dict name -> Tree.* number, read at the leaf
    of the particle.  event, time_event and destroy are those of ParticulateSource.  Destroy it before its list."""

    def __init__(self, tree, plist, kind, function=None, variables=None):
        variables = dict(variables or {})
        names = (C.c_char_p * max(len(variables), 1))(*[k.encode() for k in variables])
        numbers = (_i * max(len(variables), 1))(*[int(v) for v in variables.values()])
        p = _vp()
        _check(lib().gfship_tree_particulate_source_create(
            C.byref(p), plist.ptr, int(kind), None if function is None else str(function).encode(),
            len(variables), names, numbers))
        self.ptr, self.plist, self.tree, self.kind = p, plist, tree, int(kind)

    def set_fields(self, rad=None, urel=(), deposit=None):
        """Tree.RAD, (Tree.URELP, Tree.VRELP[, Tree.WRELP]) and Tree.VOLSRC (a volume source) or Tree.DMDT (a mass
        source); None: not written"""
        u = [-1 if v is None else int(v) for v in urel] + [-1] * (3 - len(urel))
        _check(lib().gfship_tree_particulate_source_set_fields(
            self.ptr, -1 if rad is None else int(rad), (_i * 3)(*u), -1 if deposit is None else int(deposit)))


class TreeFeedParticle(FeedParticle):
    """GfsFeedParticle on a list of Tree.particulates.  mass, volume: as for FeedParticle; variables: a dict name ->
    Tree.* number, read at the leaf of the candidate.  event and close are those of FeedParticle.  Close it before its
    list."""

    def __init__(self, tree, plist, mass=None, volume=None, variables=None):
        variables = dict(variables or {})
        names = (C.c_char_p * max(len(variables), 1))(*[k.encode() for k in variables])
        numbers = (_i * max(len(variables), 1))(*[int(v) for v in variables.values()])
        p = _vp()
        _check(lib().gfship_tree_feed_particle_create(
            C.byref(p), plist.ptr, None if mass is None else str(mass).encode(),
            None if volume is None else str(volume).encode(), len(variables), names, numbers))
        self.ptr, self.plist, self.tree = p, plist, tree


class TreeDropletToParticle(DropletToParticle):
    """GfsDropletToParticle on a list of Tree.particulates: the droplets of the variable c (a Tree.* number), or of
    `function' -- as for DropletToParticle; variables: a dict name -> Tree.* number -- smaller than min leaves become
    particulates, and c = reset on their leaves.  A function that is no variable is evaluated at every cell of every
    level.  event and close are those of DropletToParticle.  Close it before its list."""

    def __init__(self, tree, plist, c, min=20, reset=0., density=1., function=None, variables=None):
        variables = dict(variables or {})
        names = (C.c_char_p * max(len(variables), 1))(*[k.encode() for k in variables])
        numbers = (_i * max(len(variables), 1))(*[int(v) for v in variables.values()])
        p = _vp()
        _check(lib().gfship_tree_droplet_to_particle_create(
            C.byref(p), plist.ptr, int(c), int(min), float(reset), float(density),
            None if function is None else str(function).encode(), len(variables), names, numbers))
        self.ptr, self.plist, self.tree = p, plist, tree


REFINE_FN = C.CFUNCTYPE(C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p)


def tree_host_check(refine, dim=2, sides=None, nrelax=4):
    """gfship_tree_host_check: the plans of a tree validated on the host (no device needed);
    returns (cell updates, levels sweep after sweep, levels of the loop plans, differing values)"""
    if dim == 2:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y)))
    else:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y, z)))
    arr = (C.c_int * 6)(*(list(sides) + [0] * 6)[:6]) if sides is not None else None
    stats = (C.c_longlong * 4)()
    _check(lib().gfship_tree_host_check(dim, C.cast(cb, C.c_void_p), None, arr, nrelax, stats))
    return tuple(stats)


def tree_host_check_diffusion(refine, w, dim=3, sides=None, nrelax=4):
    """gfship_tree_host_check_diffusion: the diffusion relax plans of a tree with the face coefficients of
    the weight w validated on the host; returns (cell updates, levels of the loop plans, faces whose
    coefficient is not w, differing values, flow hazards, levels without a flow plan)"""
    if dim == 2:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y)))
    else:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y, z)))
    arr = (C.c_int * 6)(*(list(sides) + [0] * 6)[:6]) if sides is not None else None
    stats = (C.c_longlong * 6)()
    _check(lib().gfship_tree_host_check_diffusion(dim, C.cast(cb, C.c_void_p), None, arr, nrelax, float(w), stats))
    return tuple(stats)


def tree_host_plan_digest(refine, dim=2, sides=None, nrelax=4):
    """gfship_tree_host_plan_digest: FNV-1a-64 digests of (topology, sweep plans, loop plans, flow plans, face sets)
    as a device tree of these arguments would upload them (no device needed)"""
    if dim == 2:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y)))
    else:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y, z)))
    arr = (C.c_int * 6)(*(list(sides) + [0] * 6)[:6]) if sides is not None else None
    out = (C.c_ulonglong * 5)()
    _check(lib().gfship_tree_host_plan_digest(dim, C.cast(cb, C.c_void_p), None, arr, nrelax, out))
    return tuple(out)


def tree_host_tag_droplets(refine, levels, nleaves, dim=2, sides=None):
    """gfship_tree_host_tag_droplets: the droplet plan of a tree and the closed form of gfs_domain_tag_droplets on
    it, on the host (no device needed).  levels: the mask, one array with ghosts per level; nleaves: the number of
    interior leaves.  Returns (the tag of every leaf in traversal order, the number of droplets, (contacts, contacts
    with a gate, periodic pairs))"""
    if dim == 2:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y)))
    else:
        cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y, z)))
    arr = (C.c_int * 6)(*(list(sides) + [0] * 6)[:6]) if sides is not None else None
    c = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in levels]))
    tags = np.zeros(int(nleaves), dtype=np.uint32)
    n = C.c_uint(0)
    counts = (C.c_longlong * 3)()
    _check(lib().gfship_tree_host_tag_droplets(dim, C.cast(cb, C.c_void_p), None, arr, c.size, c.ctypes.data_as(_pd),
                                               tags.size, tags.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(n),
                                               counts))
    return tags, int(n.value), tuple(counts)


class Tree:
    """gfship_tree: a GfsSimulation on one periodic box refined by a GfsRefine function (coarse-fine
    stencils; quadtree or octree).  refine (x, y) or refine (x, y, z) -> level wanted there."""
    P, PMAC, U, V, GX, GY, GMACX, GMACY, UN0, UN1, UN2, UN3, W, GZ, GMACZ, UN4, UN5, DIV, BCVAL, RES, T0, T1, BCU, BCV, BCW = range(25)
    UPREV, VPREV, WPREV = 25, 26, 27      # Un, Vn, Wn: once a list of particulates has a force with a coefficient
    VF, FX, FY, FZ = 28, 29, 30, 31       # GfsParticulateField, GfsSourceParticulate: once a call has needed them
    # Rad, Urelp, Vrelp, Wrelp, volsource, dmdtvariable of GfsSourceParticulateVol / ...Mass: in the same way
    RAD, URELP, VRELP, WRELP, VOLSRC, DMDT = 32, 33, 34, 35, 36, 37
    TAG = 38                              # the tags of tag_droplets: once a call has needed them

    def __init__(self, refine, dim=2, device=0, sides=None):
        self.dim = dim
        if dim == 2:
            self._cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y)))
        else:
            self._cb = REFINE_FN(lambda x, y, z, ctx: float(refine(x, y, z)))
        p = _vp()
        if sides is None:
            _check(lib().gfship_tree_create(C.byref(p), dim, C.cast(self._cb, C.c_void_p), None, device))
        else:
            arr = (C.c_int * 6)(*(list(sides) + [0] * 6)[:6])
            _check(lib().gfship_tree_create_sides(C.byref(p), dim, C.cast(self._cb, C.c_void_p), None, arr,
                                                  device))
        self.ptr = p
        self.depth = lib().gfship_tree_depth(p)
        self.projection_params = lib().gfship_tree_projection_params(p, 0).contents
        self.approx_projection_params = lib().gfship_tree_projection_params(p, 1).contents

    def flags(self, level):
        r = (1 << level) + 2
        a = np.zeros((r,) * self.dim, dtype=np.uint8)
        _check(lib().gfship_tree_flags(self.ptr, level, a.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return a

    def centres(self, level):
        n = 1 << level
        c = -0.5 + (np.arange(n + 2) - 0.5) / n
        if self.dim == 2:
            return np.meshgrid(c, c, indexing="xy")
        z, y, x = np.meshgrid(c, c, c, indexing="ij")
        return x, y, z

    def upload(self, var, level, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == ((1 << level) + 2,) * self.dim
        _check(lib().gfship_tree_upload(self.ptr, var, level, a.ctypes.data_as(_pd)))

    def download(self, var, level):
        r = (1 << level) + 2
        a = np.empty((r,) * self.dim)
        _check(lib().gfship_tree_download(self.ptr, var, level, a.ctypes.data_as(_pd)))
        return a

    def set_time(self, end, cfl):
        _check(lib().gfship_tree_set_time(self.ptr, end, cfl))

    def set_bc_u(self, c, d, kind, values=None):
        """condition of velocity component c on side d; values: per level, the arrays of the values at the
        ghost cells (the oracle's gt_bc_values_u layout), uploaded to BCU + c"""
        _check(lib().gfship_tree_set_bc_u(self.ptr, c, d, kind))
        if values is not None:
            for l, a in enumerate(values):
                self.upload(Tree.BCU + c, l, a)

    def set_viscosity(self, c, nu):
        _check(lib().gfship_tree_set_viscosity(self.ptr, c, nu))

    def set_source(self, c, g):
        _check(lib().gfship_tree_set_source(self.ptr, c, g))

    def diffusion_params(self, c):
        return lib().gfship_tree_diffusion_params(self.ptr, c).contents

    def add_tracer(self, gradient=1):
        """GfsVariableTracer [{ gradient = }] (0 centred, 1 van Leer): the variable index (T0, T1)"""
        return _check(lib().gfship_tree_add_tracer(self.ptr, gradient))

    def start(self):
        _check(lib().gfship_tree_start(self.ptr))

    def step(self):
        _check(lib().gfship_tree_step(self.ptr))

    def snapshot(self, variables):
        """the binary cell data of the GfsBox (gfship_tree_snapshot_write) for the variables (Tree.P ...) as bytes"""
        n = len(variables)
        h = (C.c_int * n)(*variables)
        size = lib().gfship_tree_snapshot_bytes(self.ptr, n)
        if size == 0:
            _check(-1)
        buf = C.create_string_buffer(size)
        _check(lib().gfship_tree_snapshot_write(self.ptr, n, h, buf, size))
        return buf.raw

    def snapshot_read(self, variables, data):
        n = len(variables)
        h = (C.c_int * n)(*variables)
        buf = C.create_string_buffer(bytes(data), len(data))
        _check(lib().gfship_tree_snapshot_read(self.ptr, n, h, buf, len(data)))

    def restart(self, t, i):
        """GfsTime { t = i = } of a simulation file: start() then takes the branch time.i > 0"""
        _check(lib().gfship_tree_restart(self.ptr, t, i))

    def set_bc(self, d, kind):
        _check(lib().gfship_tree_set_bc(self.ptr, d, kind))

    def poisson_solve(self, par, dt=1.):
        """gfs_poisson_solve: guess in P, right-hand side in DIV, residual left in RES"""
        _check(lib().gfship_tree_poisson_solve(self.ptr, C.byref(par), dt))

    def divergence(self, level):
        """the derived variable Divergence of the leaves of a level (gfs_divergence)"""
        _check(lib().gfship_tree_divergence(self.ptr))
        return self.download(self.DIV, level)

    def sweep_levels(self, level):
        a, b = C.c_int(), C.c_int()
        _check(lib().gfship_tree_sweep_levels(self.ptr, level, C.byref(a), C.byref(b)))
        return a.value, b.value

    def interpolate(self, var, points):
        """GfsOutputLocation: the variable (Tree.U ...) at points (N, 3) -> (values, inside)"""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        out = np.empty(len(pts))
        inside = np.empty(len(pts), dtype=np.uint8)
        _check(lib().gfship_tree_interpolate(self.ptr, var, len(pts), pts.ctypes.data_as(_pd),
                                             out.ctypes.data_as(_pd),
                                             inside.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out, inside.astype(bool)

    def particles(self, pos, ids):
        """a GfsParticleList of GfsParticle tracers on this tree (destroy it before the tree)"""
        return ParticleList(self, pos, ids)

    def particulates(self, pos, ids, vel, mass, volume):
        """a GfsParticleList of GfsParticulate on this tree: set_forces, set_force_coefficient, particulate_state
        and event work on it as on the uniform box (destroy it before the tree)"""
        return ParticleList(self, pos, ids, particulate=(vel, mass, volume))

    # two-way coupling: GfsParticulateField and GfsSourceParticulate on a list of Tree.particulates
    def particulate_field(self, pl):
        """Tree.VF = the volume fraction of the particles of the list (GfsParticulateField)"""
        _check(lib().gfship_tree_particulate_field(pl.ptr, Tree.VF))

    def forces_on_fluid(self, pl):
        """the stored force of every particle = its forces but buoyancy, times its volume"""
        _check(lib().gfship_tree_particles_forces_on_fluid(pl.ptr))

    def set_kernel(self, pl, rkernel, function=None):
        """rkernel (a length) and kernel (C text of x, y, z, t; a number; None = 0) of GfsSourceParticulate"""
        _check(lib().gfship_tree_particles_set_kernel(
            pl.ptr, float(rkernel), None if function is None else str(function).encode()))

    def spread_forces(self, pl):
        """Tree.FX ... = minus the stored forces spread around the particles with the kernel"""
        _check(lib().gfship_tree_particles_spread_forces(pl.ptr))

    def source_particulate_event(self, pl):
        """forces_on_fluid, then spread_forces"""
        _check(lib().gfship_tree_source_particulate_event(pl.ptr))

    # idlast of a list of this tree, tracers or particulates (ParticleList.idlast is the call of a box)
    def idlast(self, pl):
        """idlast of the GfsParticleList: the id the last particle a TreeFeedParticle added took"""
        return _check(lib().gfship_tree_particles_idlast(pl.ptr))

    def set_idlast(self, pl, value):
        _check(lib().gfship_tree_particles_set_idlast(pl.ptr, int(value)))

    def tag_droplets(self, c):
        """gfs_domain_tag_droplets: the leaves of Tree.TAG get the index (1 ..) of their droplet of the variable c, 0
        outside; returns the number of droplets"""
        n = C.c_uint(0)
        _check(lib().gfship_tree_tag_droplets(self.ptr, int(c), C.byref(n)))
        return int(n.value)

    def time_tag_droplets(self, c, reps=10):
        """tag_droplets, measured between two events after a warm-up call: milliseconds per call"""
        ms = C.c_double(0.)
        _check(lib().gfship_tree_tag_droplets_time(self.ptr, int(c), int(reps), C.byref(ms)))
        return ms.value

    def remove_droplets(self, c, v, min, val=0.):
        """gfs_domain_remove_droplets: v = val on the leaves of the droplets of c smaller than min leaves (min < 0: all
        but the -min largest)"""
        _check(lib().gfship_tree_remove_droplets(self.ptr, int(c), int(v), int(min), float(val)))

    def set_source_fields(self, on=True):
        """U, V(, W) take the velocity source of Tree.FX ... (GfsSourceParticulate in the time step)"""
        _check(lib().gfship_tree_set_source_fields(self.ptr, 1 if on else 0))

    def mac_source(self, c, var_out):
        """gfs_variable_mac_source of component c on the leaves, without the constant of set_source, into
        Tree.RES or Tree.DIV"""
        _check(lib().gfship_tree_mac_source(self.ptr, int(c), int(var_out)))

    def sampler_stats(self):
        """the corner interpolators of the sampler: (corners of leaves, corners that read the table, table
        entries, bytes on the device, cells of the longest interpolator)"""
        stats = (C.c_longlong * 5)()
        _check(lib().gfship_tree_sampler_stats(self.ptr, stats))
        return tuple(stats)

    t = property(lambda self: lib().gfship_tree_time(self.ptr))
    dt = property(lambda self: lib().gfship_tree_dt(self.ptr))
    i = property(lambda self: lib().gfship_tree_iter(self.ptr))

    def destroy(self):
        if self.ptr:
            lib().gfship_tree_destroy(self.ptr)
            self.ptr = None


TREE_TAG = Tree.TAG      # GFSHIP_TREE_TAG
