"""ctypes binding of libpixie_hip.so (declared in include/pixie_hip.h).

There is no CPU fallback: if the shared library is missing or a call fails, the caller gets an
exception.  Torch is used only for device memory (tensor.data_ptr()) and the current stream.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpixie_hip.so")
DIAG_LIB_PATH = os.path.join(_HERE, "libpixie_hip_diag.so")   # the -DPIXIE_DIAG build of the same sources (tests, profilers)


class PixieHipError(RuntimeError):
    pass


class BCDesc(C.Structure):
    """struct pixie_bc_desc"""
    _fields_ = [("type", C.c_int32), ("surface_type", C.c_int32), ("reset", C.c_int32), ("pad_", C.c_int32),
                ("point", C.c_double * 3), ("size", C.c_double * 3), ("velocity", C.c_double * 3),
                ("normal", C.c_double * 3), ("start_time", C.c_double), ("end_time", C.c_double),
                ("friction", C.c_double)]


class PModDesc(C.Structure):
    """struct pixie_pmod_desc"""
    _fields_ = [("type", C.c_int32), ("pad_", C.c_int32),
                ("point", C.c_double * 3), ("size", C.c_double * 3), ("force", C.c_double * 3),
                ("velocity", C.c_double * 3), ("normal", C.c_double * 3), ("h1", C.c_double * 3),
                ("h2", C.c_double * 3), ("half_height", C.c_double), ("radius", C.c_double),
                ("rotation_scale", C.c_double), ("translation_scale", C.c_double),
                ("start_time", C.c_double), ("end_time", C.c_double)]


class ConvDesc(C.Structure):
    """struct pixie_conv_desc"""
    _fields_ = [("d_in0", C.c_void_p), ("c0", C.c_int32),
                ("d_in1", C.c_void_p), ("c1", C.c_int32),
                ("in_d", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32),
                ("upsample", C.c_int32), ("stride", C.c_int32), ("ksize", C.c_int32),
                ("d_pro_a", C.c_void_p), ("d_pro_b", C.c_void_p),
                ("d_gamma", C.c_void_p), ("d_beta", C.c_void_p),
                ("act", C.c_int32),
                ("d_w", C.c_void_p), ("d_bias", C.c_void_p),
                ("c_out", C.c_int32),
                ("d_residual", C.c_void_p), ("d_out", C.c_void_p),
                ("d_w16", C.c_void_p), ("d_in_amax0", C.c_void_p), ("d_in_amax1", C.c_void_p),
                ("in_bound", C.c_float),
                ("d_out_stats", C.c_void_p), ("d_out_amax", C.c_void_p),
                ("d_workspace", C.c_void_p),
                ("out_d", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("d_skip_in0", C.c_void_p), ("skip_c0", C.c_int32),
                ("d_skip_in1", C.c_void_p), ("skip_c1", C.c_int32),
                ("d_skip_w16", C.c_void_p), ("d_skip_bias", C.c_void_p),
                ("d_skip_amax0", C.c_void_p), ("d_skip_amax1", C.c_void_p),
                ("w16_subpixel", C.c_int32)]


class UNetConfigC(C.Structure):
    """struct pixie_unet_config"""
    _fields_ = [("feature_channels", C.c_int32), ("cond_dim", C.c_int32), ("model_channels", C.c_int32), ("num_res_blocks", C.c_int32),
                ("n_channel_mult", C.c_int32), ("channel_mult", C.c_int32 * 8),
                ("n_attention_resolutions", C.c_int32), ("attention_resolutions", C.c_int32 * 8),
                ("grid_size", C.c_int32), ("out_channels", C.c_int32), ("precision", C.c_int32)]


class BatchSched(C.Structure):
    """struct pixie_batch_sched"""
    _fields_ = [("dt", C.c_double), ("steps_per_chunk", C.c_int32), ("n_chunks", C.c_int32), ("n_out", C.c_int32), ("pad_", C.c_int32),
                ("shift", C.c_double * 3), ("scale", C.c_double), ("mean", C.c_double * 3), ("inv_rotation", C.c_double * 9),
                ("d_pos", C.c_void_p), ("d_cov", C.c_void_p)]


class BatchSplatOut(C.Structure):
    """struct pixie_batch_splat_out"""
    _fields_ = [("d_log_scale", C.c_void_p), ("d_quat", C.c_void_p)]


class FieldDesc(C.Structure):
    """struct pixie_field_desc"""
    _fields_ = [("d_pred", C.c_void_p), ("d_mask", C.c_void_p),
                ("d_axis_x", C.c_void_p), ("d_axis_y", C.c_void_p), ("d_axis_z", C.c_void_p),
                ("n_classes", C.c_int32), ("d", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("min_spacing", C.c_double),
                ("density_min", C.c_double), ("density_max", C.c_double), ("E_min", C.c_double), ("E_max", C.c_double),
                ("nu_min", C.c_double), ("nu_max", C.c_double)]


class OccupancyDesc(C.Structure):
    """struct pixie_occupancy_desc"""
    _fields_ = [("d_alphas", C.c_void_p), ("d_rgb", C.c_void_p),
                ("d_axis_x", C.c_void_p), ("d_axis_y", C.c_void_p), ("d_axis_z", C.c_void_p), ("d_stats", C.c_void_p),
                ("dtype", C.c_int32), ("d", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("run_filters", C.c_int32), ("nb_neighbors", C.c_int32), ("min_points", C.c_int32), ("keep", C.c_int32),
                ("voxel_size", C.c_double), ("lattice_spacing", C.c_double),
                ("alpha_threshold", C.c_double), ("gray_threshold", C.c_double), ("std_ratio", C.c_double),
                ("eps_multiplier", C.c_double)]


PART_SEG_COUNTS = 40   # PIXIE_PART_SEG_COUNTS


class PartSegDesc(C.Structure):
    """struct pixie_part_seg_desc"""
    _fields_ = [("d_features", C.c_void_p), ("d_mask", C.c_void_p), ("d_queries", C.c_void_p), ("d_props", C.c_void_p),
                ("d", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("channels", C.c_int32), ("n_parts", C.c_int32),
                ("vote_k", C.c_int32), ("temperature", C.c_float), ("background_id", C.c_float)]


HASHMLP_MAX_LEVELS, HASHMLP_MAX_LAYERS, HASHMLP_MAX_INPUT, HASHMLP_MAX_OUTPUT = 16, 5, 160, 1024   # PIXIE_HASHMLP_*


class HashGridLevel(C.Structure):
    """struct pixie_hashgrid_level"""
    _fields_ = [("scale", C.c_float), ("shift", C.c_float), ("res", C.c_uint32), ("size", C.c_uint32), ("offset", C.c_uint32),
                ("dense", C.c_uint32)]


class HashMlpDesc(C.Structure):
    """struct pixie_hashmlp_desc"""
    _fields_ = [("n_levels", C.c_int32), ("features_per_level", C.c_int32), ("n_frequencies", C.c_int32), ("n_extra", C.c_int32),
                ("n_hidden", C.c_int32), ("out_dim", C.c_int32), ("out_activation", C.c_int32), ("pad_", C.c_int32),
                ("level", HashGridLevel * HASHMLP_MAX_LEVELS),
                ("d_table", C.c_void_p), ("table_rows", C.c_int64),
                ("d_weight", C.c_void_p * HASHMLP_MAX_LAYERS), ("d_bias", C.c_void_p * HASHMLP_MAX_LAYERS)]


class HashMlpGrads(C.Structure):
    """struct pixie_hashmlp_grads"""
    _fields_ = [("d_table", C.c_void_p), ("d_weight", C.c_void_p * HASHMLP_MAX_LAYERS), ("d_bias", C.c_void_p * HASHMLP_MAX_LAYERS),
                ("d_extra", C.c_void_p)]


DENSITY_FIELD_WIDTH, DENSITY_FIELD_MAX_LAYERS, DENSITY_FIELD_MAX_INPUT = 16, 3, 64   # PIXIE_DENSITY_FIELD_*


class DensityFieldDesc(C.Structure):
    """struct pixie_density_field_desc"""
    _fields_ = [("n_levels", C.c_int32), ("features_per_level", C.c_int32), ("n_hidden", C.c_int32), ("hidden_width", C.c_int32),
                ("contraction", C.c_int32), ("average_init_density", C.c_float),
                ("level", HashGridLevel * HASHMLP_MAX_LEVELS),
                ("d_table", C.c_void_p), ("table_rows", C.c_int64),
                ("d_weight", C.c_void_p * DENSITY_FIELD_MAX_LAYERS), ("d_bias", C.c_void_p * DENSITY_FIELD_MAX_LAYERS),
                ("d_world_to_nerf", C.c_void_p), ("aabb", C.c_float * 6)]


class DensityFieldGrads(C.Structure):
    """struct pixie_density_field_grads"""
    _fields_ = [("d_table", C.c_void_p), ("d_weight", C.c_void_p * DENSITY_FIELD_MAX_LAYERS), ("d_bias", C.c_void_p * DENSITY_FIELD_MAX_LAYERS)]


RAY_MAX_SAMPLES, RAY_MAX_FEATURE_SAMPLES, RAY_MAX_CHANNELS, RAY_MAX_RAYS = 1024, 256, 2048, 1 << 24   # csrc/ray_render_math.h


class RayDesc(C.Structure):
    """struct pixie_ray_desc"""
    _fields_ = [("n_rays", C.c_int64), ("n_samples", C.c_int32), ("n_channels", C.c_int32), ("background", C.c_int32), ("bg", C.c_float * 3)]


class RayInputs(C.Structure):
    """struct pixie_ray_inputs"""
    _fields_ = [("d_densities", C.c_void_p), ("d_deltas", C.c_void_p), ("d_weights", C.c_void_p), ("d_starts", C.c_void_p),
                ("d_ends", C.c_void_p), ("d_rgb", C.c_void_p), ("d_features", C.c_void_p)]


class RayOutputs(C.Structure):
    """struct pixie_ray_outputs"""
    _fields_ = [("d_weights", C.c_void_p), ("d_accumulation", C.c_void_p), ("d_expected_depth", C.c_void_p), ("d_median_depth", C.c_void_p),
                ("d_rgb", C.c_void_p), ("d_feature", C.c_void_p)]


class RayUpstream(C.Structure):
    """struct pixie_ray_upstream"""
    _fields_ = [("d_weights", C.c_void_p), ("d_accumulation", C.c_void_p), ("d_expected_depth", C.c_void_p), ("d_rgb", C.c_void_p),
                ("d_feature", C.c_void_p)]


class RayGrads(C.Structure):
    """struct pixie_ray_grads"""
    _fields_ = [("d_densities", C.c_void_p), ("d_weights", C.c_void_p), ("d_rgb", C.c_void_p), ("d_features", C.c_void_p)]


RAY_SAMPLE_MAX_SAMPLES, RAY_SAMPLE_MAX_LEVELS = 1024, 8   # csrc/ray_sample_math.h


class RaySampleDesc(C.Structure):
    """struct pixie_ray_sample_desc"""
    _fields_ = [("n_rays", C.c_int64), ("n_samples", C.c_int32), ("n_existing", C.c_int32), ("spacing", C.c_int32), ("jitter_stride", C.c_int32),
                ("include_original", C.c_int32), ("histogram_padding", C.c_float), ("eps", C.c_float), ("anneal", C.c_float),
                ("u_scale", C.c_float), ("u_offset", C.c_float)]


class RaySampleInputs(C.Structure):
    """struct pixie_ray_sample_inputs"""
    _fields_ = [(name, C.c_void_p) for name in ("d_nears", "d_fars", "d_origins", "d_directions", "d_table", "d_jitter", "d_existing_bins",
                                                "d_weights", "d_s_near", "d_s_far")]


class RaySampleOutputs(C.Structure):
    """struct pixie_ray_sample_outputs"""
    _fields_ = [(name, C.c_void_p) for name in ("d_bins", "d_starts", "d_ends", "d_deltas", "d_positions", "d_s_near", "d_s_far")]


class RayInterlevelDesc(C.Structure):
    """struct pixie_ray_interlevel_desc"""
    _fields_ = [("n_rays", C.c_int64), ("n_fine", C.c_int32), ("n_levels", C.c_int32), ("n_proposal", C.c_int32 * RAY_SAMPLE_MAX_LEVELS),
                ("per_sample", C.c_int32)]


class RayInterlevelInputs(C.Structure):
    """struct pixie_ray_interlevel_inputs"""
    _fields_ = [("d_fine_edges", C.c_void_p), ("d_fine_weights", C.c_void_p), ("d_edges", C.c_void_p * RAY_SAMPLE_MAX_LEVELS),
                ("d_weights", C.c_void_p * RAY_SAMPLE_MAX_LEVELS)]


class RayInterlevelGrads(C.Structure):
    """struct pixie_ray_interlevel_grads"""
    _fields_ = [("d_weights", C.c_void_p * RAY_SAMPLE_MAX_LEVELS)]


class RayDistortionDesc(C.Structure):
    """struct pixie_ray_distortion_desc"""
    _fields_ = [("n_rays", C.c_int64), ("n_samples", C.c_int32), ("per_ray", C.c_int32)]


class FieldVoxelizeDesc(C.Structure):
    """struct pixie_field_voxelize_desc"""
    _fields_ = [("density", HashMlpDesc), ("color", HashMlpDesc), ("feature", HashMlpDesc),
                ("d_axis_x", C.c_void_p), ("d_axis_y", C.c_void_p), ("d_axis_z", C.c_void_p),
                ("min_bounds", C.c_double * 3), ("voxel_size", C.c_double),
                ("d", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("contraction", C.c_int32), ("alpha_weighted", C.c_int32),
                ("average_init_density", C.c_float), ("world_to_nerf", C.c_float * 12), ("aabb", C.c_float * 6)]


class RasterDesc(C.Structure):
    """struct pixie_raster_desc"""
    _fields_ = [("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("viewmatrix", C.c_float * 16), ("projmatrix", C.c_float * 16), ("bg", C.c_float * 3), ("pad_", C.c_int32),
                ("d_means", C.c_void_p), ("d_cov3d", C.c_void_p), ("d_scales", C.c_void_p), ("d_rotations", C.c_void_p),
                ("d_colors", C.c_void_p), ("d_opacity", C.c_void_p),
                ("d_out_color", C.c_void_p), ("d_radii", C.c_void_p), ("d_final_T", C.c_void_p), ("d_n_contrib", C.c_void_p),
                ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class RasterBackwardDesc(C.Structure):
    """struct pixie_raster_backward_desc"""
    _fields_ = [("forward", RasterDesc), ("instances", C.c_int64),
                ("d_shs", C.c_void_p), ("sh_k", C.c_int32), ("sh_degree", C.c_int32), ("campos", C.c_float * 3), ("pad_", C.c_int32),
                ("d_dL_dcolor", C.c_void_p),
                ("d_dL_dmeans3D", C.c_void_p), ("d_dL_dmeans2D", C.c_void_p), ("d_dL_dopacity", C.c_void_p), ("d_dL_dcolors", C.c_void_p),
                ("d_dL_dshs", C.c_void_p), ("d_dL_dcov3D", C.c_void_p), ("d_dL_dscales", C.c_void_p), ("d_dL_drotations", C.c_void_p),
                ("d_grad_workspace", C.c_void_p), ("grad_workspace_bytes", C.c_int64)]


class RasterView(C.Structure):
    """struct pixie_raster_view"""
    _fields_ = [("viewmatrix", C.c_float * 16), ("projmatrix", C.c_float * 16), ("campos", C.c_float * 3),
                ("tanfovx", C.c_float), ("tanfovy", C.c_float)]


class RasterBatchDesc(C.Structure):
    """struct pixie_raster_batch_desc"""
    _fields_ = [("views", C.c_int32), ("n_dyn", C.c_int32), ("n_static", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("sh_degree", C.c_int32), ("k_coeffs", C.c_int32), ("scale_modifier", C.c_float), ("bg", C.c_float * 3), ("pad_", C.c_int32),
                ("view", C.POINTER(RasterView)),
                ("d_means", C.c_void_p), ("d_cov3d", C.c_void_p), ("means_view_stride", C.c_int64), ("cov3d_view_stride", C.c_int64),
                ("d_static_means", C.c_void_p), ("d_static_cov3d", C.c_void_p), ("d_opacity", C.c_void_p),
                ("d_colors", C.c_void_p), ("colors_view_stride", C.c_int64), ("d_shs", C.c_void_p),
                ("d_out_color", C.c_void_p), ("d_out_rgb8", C.c_void_p), ("d_radii", C.c_void_p), ("d_final_T", C.c_void_p),
                ("d_n_contrib", C.c_void_p),
                ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("max_instances", C.c_int64)]


class IngestDesc(C.Structure):
    """struct pixie_ingest_desc"""
    _fields_ = [("n", C.c_int64), ("n_attr", C.c_int32), ("sh_degree", C.c_int32), ("n_rotations", C.c_int32), ("has_sim_area", C.c_int32),
                ("rotations", C.c_float * 72), ("sim_area", C.c_float * 6), ("opacity_threshold", C.c_float), ("z_shift", C.c_float),
                ("d_block", C.c_void_p), ("columns", C.POINTER(C.c_int32)),
                ("d_pos", C.c_void_p), ("d_cov", C.c_void_p), ("d_opacity", C.c_void_p), ("d_shs", C.c_void_p),
                ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class GsAdamGroup(C.Structure):
    """struct pixie_gs_adam_group"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("count", C.c_int64), ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float)]


class GsAdamDesc(C.Structure):
    """struct pixie_gs_adam_desc"""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("n_groups", C.c_int32), ("pad_", C.c_int32),
                ("group", GsAdamGroup * 8)]


class GsDensifyDesc(C.Structure):
    """struct pixie_gs_densify_desc"""
    _fields_ = [("n", C.c_int64), ("n_rest", C.c_int32), ("has_max_screen_size", C.c_int32),
                ("max_grad", C.c_double), ("min_opacity", C.c_double), ("extent", C.c_double), ("percent_dense", C.c_double),
                ("d_xyz_gradient_accum", C.c_void_p), ("d_denom", C.c_void_p),
                ("d_param", C.c_void_p * 6), ("d_exp_avg", C.c_void_p * 6), ("d_exp_avg_sq", C.c_void_p * 6),
                ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class GsDensifyOuts(C.Structure):
    """struct pixie_gs_densify_outs"""
    _fields_ = [("n_out", C.c_int64), ("n_split", C.c_int64), ("d_noise", C.c_void_p),
                ("d_param", C.c_void_p * 6), ("d_exp_avg", C.c_void_p * 6), ("d_exp_avg_sq", C.c_void_p * 6),
                ("d_source_index", C.c_void_p), ("d_xyz_gradient_accum", C.c_void_p), ("d_denom", C.c_void_p),
                ("d_max_radii2D", C.c_void_p)]


# pixie_gs_densify_plan / _emit's return codes besides 0 and 1 (include/pixie_hip.h)
GS_DENSIFY_BAD_MAX_GRAD, GS_DENSIFY_TOO_MANY_ROWS, GS_DENSIFY_EMPTY = 2, 3, 4


# pixie_scene_ingest's return codes besides 0 and 1 (include/pixie_hip.h)
INGEST_NO_SELECTION, INGEST_ZERO_EXTENT, INGEST_TOO_MANY_ROTATIONS, INGEST_TOO_MANY_ROWS = 2, 3, 4, 5


# every symbol include/pixie_hip.h declares: name -> (restype, argtypes)
_VP, _I, _I64, _D, _S = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_char_p
_D3 = C.POINTER(C.c_double)
SIGNATURES = {
    "pixie_last_error": (C.c_char_p, []),
    "pixie_build_arch": (C.c_char_p, []),
    "pixie_mpm_create": (_I, [C.POINTER(_VP), _I, _I, _D]),
    "pixie_mpm_destroy": (_I, [_VP]),
    "pixie_mpm_regrid": (_I, [_VP, _I, _D, _VP]),
    "pixie_mpm_set_field": (_I, [_VP, _S, _VP, _I64, _VP]),
    "pixie_mpm_get_field": (_I, [_VP, _S, _VP, _I64, _VP]),
    "pixie_mpm_fill_field": (_I, [_VP, _S, _D, _VP]),
    "pixie_mpm_set_scalar": (_I, [_VP, _S, _D]),
    "pixie_mpm_get_scalar": (_I, [_VP, _S, C.POINTER(_D)]),
    "pixie_mpm_update_mass": (_I, [_VP, _VP]),
    "pixie_mpm_finalize_mu_lam": (_I, [_VP, _I, _VP]),
    "pixie_mpm_apply_additional_params": (_I, [_VP, _D3, _D3, _D, _D, _D, _I, _VP]),
    "pixie_mpm_apply_additional_params_batch": (_I, [_VP, _I64, _VP, _VP, _VP, _VP]),
    "pixie_mpm_add_bc": (_I, [_VP, C.POINTER(BCDesc)]),
    "pixie_mpm_add_particle_modifier": (_I, [_VP, C.POINTER(PModDesc), _VP]),
    "pixie_mpm_step": (_I, [_VP, _D, _I, _VP]),
    "pixie_mpm_export_cov": (_I, [_VP, _VP, _VP]),
    "pixie_mpm_export_R": (_I, [_VP, _VP, _VP]),
    "pixie_mpm_export_frame": (_I, [_VP, _I, _D3, _D, _D3, C.POINTER(C.c_double), _VP, _VP, _VP]),
    "pixie_mpm_out_of_bounds": (_I, [_VP, C.POINTER(_I64), _VP]),
    "pixie_mpm_batch_create": (_I, [C.POINTER(_VP), C.POINTER(_VP), _I]),
    "pixie_mpm_batch_step": (_I, [_VP, _D, _I, _VP]),
    "pixie_mpm_batch_run": (_I, [_VP, C.POINTER(BatchSched), _I, _VP]),
    "pixie_mpm_batch_run_splats": (_I, [_VP, C.POINTER(BatchSched), C.POINTER(BatchSplatOut), _I, _VP]),
    "pixie_splat_from_cov": (_I, [_VP, _I64, _VP, _VP, _VP]),
    "pixie_mpm_export_frame_splats": (_I, [_VP, _I, _D3, _D, _D3, C.POINTER(C.c_double), _VP, _VP, _VP, _VP, _VP]),
    "pixie_mpm_batch_destroy": (_I, [_VP]),
    "pixie_pack_fields": (_I, [_VP, _VP, _I64, _I64, _VP, _I64, _VP]),
    "pixie_conv_cout_padded": (_I, [_I]),
    "pixie_conv_pack_weights": (_I, [_VP, _VP, _I, _I, _I, _VP]),
    "pixie_conv_packed16_bytes": (_I64, [_I, _I, _I]),
    "pixie_conv_pack_weights_f16x2": (_I, [_VP, _VP, _I, _I, _I, _VP]),
    "pixie_conv_subpixel_bytes": (_I64, [_I, _I]),
    "pixie_conv_pack_weights_subpixel": (_I, [_VP, _VP, _I, _I, _VP]),
    "pixie_conv3d_forward": (_I, [C.POINTER(ConvDesc), _VP]),
    "pixie_conv_stats_floats": (_I64, [C.POINTER(ConvDesc)]),
    "pixie_conv_workspace_bytes": (_I64, [C.POINTER(ConvDesc)]),
    "pixie_stats_finalize": (_I, [_VP, C.POINTER(ConvDesc), _VP, _VP]),
    "pixie_stats_norm_finalize": (_I, [_VP, C.POINTER(ConvDesc), _VP, _VP, C.POINTER(ConvDesc), _VP, _I, _I64, _I, _I, _D, _VP, _VP, _VP, _VP, _VP]),
    "pixie_channel_stats": (_I, [_VP, _I, _I64, _VP, _VP, _VP]),
    "pixie_tensor_amax": (_I, [_VP, _I64, _VP, _VP]),
    "pixie_channel_sums": (_I, [_VP, _I, _I64, _VP, _VP]),
    "pixie_norm_finalize": (_I, [_VP, _I, _I64, _I, _I, _D, _VP, _VP, _VP, _VP, _VP]),
    "pixie_attention_forward": (_I, [_VP, _VP, _I, _I, _VP]),
    "pixie_channel_affine": (_I, [_VP, _VP, _VP, _VP, _I, _I64, _VP]),
    "pixie_projector_conv0": (_I, [_VP, _I64, _I, _I, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), _I, _VP]),
    "pixie_conv_skip_foldable": (_I, [C.POINTER(ConvDesc)]),
    "pixie_unet_create": (_I, [C.POINTER(_VP), C.POINTER(UNetConfigC)]),
    "pixie_unet_destroy": (_I, [_VP]),
    "pixie_unet_param_count": (_I, [_VP]),
    "pixie_unet_param_info": (_I, [_VP, _I, C.POINTER(_S), C.POINTER(_I64), C.POINTER(C.c_int32), C.POINTER(_I64)]),
    "pixie_unet_set_param": (_I, [_VP, _S, _VP, _I64]),
    "pixie_unet_workspace_bytes": (_I64, [_VP, _I, _I, _I]),
    "pixie_unet_set_option": (_I, [_VP, _S, _I]),
    "pixie_unet_forward": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _I64, _VP]),
    "pixie_unet_forward_pair": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _I64, _VP, _I64, _VP, _VP]),
    "pixie_combine_class_ids": (_I, [_VP, _I, _VP, _I64, _VP, _VP]),
    "pixie_combine_predictions": (_I, [_VP, _I, _VP, _I64, _VP, _VP, _VP]),
    "pixie_voxel_grid_to_ncdhw": (_I, [_VP, _I, _I, _I, _I, _VP, _VP]),
    "pixie_unscale_prediction": (_I, [_VP, _I, _I64, _D, _D, _D, _D, _D, _D, _VP, _VP]),
    "pixie_field_points_scratch_bytes": (_I64, [C.POINTER(FieldDesc)]),
    "pixie_field_points": (_I, [C.POINTER(FieldDesc), _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pixie_fill_densify": (_I, [_VP, _VP, _VP, _I, _I, _D, _VP, _VP, _VP]),
    "pixie_fill_dense_cells": (_I, [_VP, _VP, _I, _D, _D, _I, _VP, _I64, _VP, C.c_uint32, _VP]),
    "pixie_fill_internal_cells": (_I, [_VP, _VP, _I, _D, _I, _I, _I, _D, _VP, _I64, _VP, C.c_uint32, _VP]),
    "pixie_particle_volume": (_I, [_VP, _I, _I, _D, _VP, _VP, _VP]),
    "pixie_nearest_particle": (_I, [_VP, _I, _VP, _I, _VP, _VP]),
    "pixie_dbscan_roots": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, C.POINTER(_D), _D, _D, _I, _VP, _VP, _VP, _VP]),
    "pixie_raster_workspace_bytes": (_I64, [_I, _I, _I, _I64]),
    "pixie_raster_forward": (_I, [C.POINTER(RasterDesc), C.POINTER(_I64), _VP]),
    "pixie_raster_backward_workspace_bytes": (_I64, [_I, _I, _I, _I64]),
    "pixie_raster_backward": (_I, [C.POINTER(RasterBackwardDesc), _VP]),
    "pixie_sh_to_rgb": (_I, [_VP, _I64, _I, _I, _VP, C.POINTER(C.c_float), _VP, _I64, _VP, _VP]),
    "pixie_raster_batch_workspace_bytes": (_I64, [_I, _I, _I, _I, _I64]),
    "pixie_raster_forward_batch": (_I, [C.POINTER(RasterBatchDesc), C.POINTER(_I64), C.POINTER(C.c_int32), _VP]),
    "pixie_scene_ingest_workspace_bytes": (_I64, [_I64]),
    "pixie_scene_ingest": (_I, [C.POINTER(IngestDesc), C.POINTER(_I64), C.POINTER(C.c_float), C.POINTER(C.c_float), _VP]),
    "pixie_field_to_particles": (_I, [C.POINTER(FieldDesc), _VP, _I, _I, _D, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pixie_knn_mean_dist2_scratch_bytes": (_I64, [_I64]),
    "pixie_knn_mean_dist2": (_I, [_VP, _I64, _VP, _I64, _VP, _VP]),
    "pixie_photometric_workspace_bytes": (_I64, [_I, _I, _I, _I, _I]),
    "pixie_photometric_forward": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _I64, _I, _VP, _VP, _VP]),
    "pixie_photometric_backward": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP]),
    "pixie_gs_adam_step": (_I, [C.POINTER(GsAdamDesc), _VP]),
    "pixie_gs_densify_stats": (_I, [_VP, _VP, _I64, _VP, _VP, _VP, _VP]),
    "pixie_gs_densify_workspace_bytes": (_I64, [_I64]),
    "pixie_gs_densify_plan": (_I, [C.POINTER(GsDensifyDesc), C.POINTER(_I64), C.POINTER(_I64), _VP]),
    "pixie_gs_densify_emit": (_I, [C.POINTER(GsDensifyDesc), C.POINTER(GsDensifyOuts), _VP]),
    "pixie_occupancy_scratch_bytes": (_I64, [C.POINTER(OccupancyDesc), _I]),
    "pixie_occupancy_mask": (_I, [C.POINTER(OccupancyDesc), _VP, _VP, _VP, _VP, _VP]),
    "pixie_part_seg_scratch_bytes": (_I64, [C.POINTER(PartSegDesc)]),
    "pixie_part_segmentation": (_I, [C.POINTER(PartSegDesc), _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "pixie_part_material_grid": (_I, [_VP, _VP, _I, _I64, C.c_float, _VP, _VP]),
    "pixie_hashmlp_forward": (_I, [C.POINTER(HashMlpDesc), _VP, _VP, _I64, _VP, _VP]),
    "pixie_hashmlp_train_bytes": (_I, [C.POINTER(HashMlpDesc), _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "pixie_hashmlp_forward_saved": (_I, [C.POINTER(HashMlpDesc), _VP, _VP, _I64, _VP, _VP, _VP]),
    "pixie_hashmlp_backward": (_I, [C.POINTER(HashMlpDesc), _VP, _VP, _I64, _VP, _VP, _VP, C.POINTER(HashMlpGrads), _VP, _VP]),
    "pixie_density_field_train_bytes": (_I, [C.POINTER(DensityFieldDesc), _I64, C.POINTER(_I64), C.POINTER(_I64)]),
    "pixie_density_field_forward": (_I, [C.POINTER(DensityFieldDesc), _VP, _I64, _VP, _VP, _VP]),
    "pixie_density_field_backward": (_I, [C.POINTER(DensityFieldDesc), _VP, _I64, _VP, C.POINTER(DensityFieldGrads), _VP, _VP]),
    "pixie_ray_composite_bytes": (_I, [C.POINTER(RayDesc), C.POINTER(_I64)]),
    "pixie_ray_composite_forward": (_I, [C.POINTER(RayDesc), C.POINTER(RayInputs), C.POINTER(RayOutputs), _VP]),
    "pixie_ray_composite_backward": (_I, [C.POINTER(RayDesc), C.POINTER(RayInputs), C.POINTER(RayUpstream), C.POINTER(RayGrads), _VP, _VP]),
    "pixie_ray_sample_spaced": (_I, [C.POINTER(RaySampleDesc), C.POINTER(RaySampleInputs), C.POINTER(RaySampleOutputs), _VP]),
    "pixie_ray_sample_pdf": (_I, [C.POINTER(RaySampleDesc), C.POINTER(RaySampleInputs), C.POINTER(RaySampleOutputs), _VP]),
    "pixie_ray_interlevel_bytes": (_I, [C.POINTER(RayInterlevelDesc), C.POINTER(_I64)]),
    "pixie_ray_interlevel_forward": (_I, [C.POINTER(RayInterlevelDesc), C.POINTER(RayInterlevelInputs), _VP, _VP, _VP, _VP]),
    "pixie_ray_interlevel_backward": (_I, [C.POINTER(RayInterlevelDesc), C.POINTER(RayInterlevelInputs), _VP, C.POINTER(RayInterlevelGrads), _VP]),
    "pixie_ray_distortion_bytes": (_I, [C.POINTER(RayDistortionDesc), C.POINTER(_I64)]),
    "pixie_ray_distortion_forward": (_I, [C.POINTER(RayDistortionDesc), _VP, _VP, _VP, _VP, _VP]),
    "pixie_ray_distortion_backward": (_I, [C.POINTER(RayDistortionDesc), _VP, _VP, _VP, _VP, _VP]),
    "pixie_field_voxelize": (_I, [C.POINTER(FieldVoxelizeDesc), _VP, _VP, _VP, _VP, _VP, _VP]),
    "pixie_field_query_points": (_I, [C.POINTER(FieldVoxelizeDesc), _VP, _I64, _D, _VP, _VP, _VP, _VP, _VP]),
}

# entry points that exist only in the PIXIE_DIAG build (include/pixie_hip.h, last section)
DIAG_SIGNATURES = {
    "pixie_mpm_phase": (_I, [_VP, _I, _D, _VP]),
    "pixie_mpm_kernel_times": (_I, [_VP, C.POINTER(_D), C.POINTER(_D), C.POINTER(_I64)]),
    "pixie_conv_kernel_variant": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),     # (None, flag): the pair / 4-wave launch-form switch
    "pixie_conv_tile_geometry": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int32)]),   # (desc, None): the launch form's LDS bytes, 0 = 4-wave
    "pixie_conv_stats_layout": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int64)]),
}

_libs = {}


def load(diag: bool = False):
    """dlopen libpixie_hip.so -- or, diag=True, libpixie_hip_diag.so, the same sources built with -DPIXIE_DIAG, which adds the
    diagnostic entry points -- and type every entry point; raises if absent.  The two are independent libraries: a handle
    belongs to the one that created it."""
    if diag in _libs:
        return _libs[diag]
    path = DIAG_LIB_PATH if diag else LIB_PATH
    if not os.path.exists(path):
        raise PixieHipError(
            f"{path} not found: build it with `python -m pixie_amd.build` (hipcc, gfx950). "
            "pixie_amd has no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  The process must have ONE HIP runtime -- streams and
    # device pointers cross the C ABI in both directions -- so torch's copy has to be in the process before ours is resolved
    # (same SONAME: the loader then binds libpixie_hip.so to it).  Loaded the other way round, the system ROCm runtime and
    # torch's coexist and the first hipMalloc / launch on a torch stream fails.
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in list(SIGNATURES.items()) + (list(DIAG_SIGNATURES.items()) if diag else []):
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _libs[diag] = lib
    return lib


def check(rc: int, what: str = "", lib=None):
    if rc != 0:
        msg = (lib or load()).pixie_last_error()
        raise PixieHipError(f"{what}: {msg.decode() if msg else 'unknown error'}")


def current_stream_ptr():
    """hipStream_t of torch's current stream as a void pointer (value 0 / None = the default stream).  The raw getter is ~5x
    cheaper than building a torch.cuda.Stream object, which matters for callers that ask once per substep (the deferred
    p2g2p of the MPM shim: 1000 calls per frame)."""
    import torch
    try:
        return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))
    except AttributeError:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])
