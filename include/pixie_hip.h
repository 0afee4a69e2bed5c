/*
 * include/pixie_hip.h -- C ABI of libpixie_hip.so, the MI355X (gfx950) implementation of
 * Pixie's material_mode=neural inference hot path.
 *
 * The reference (vlongle/pixie) has no FFI/plugin layer for this path: its stages are Python
 * classes calling torch ops and NVIDIA-Warp kernels in-process.  This
 * header is therefore the boundary a maintainer would bind from the reference's Python with
 * ctypes (INTEGRATION.md shows the stubs); each entry point cites the reference call it
 * replaces.  Paths are relative to the reference root:
 *   WG = third_party/Wavelet-Generation,  PG = third_party/PhysGaussian.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, scalars.  No torch / HIP types in signatures;
 *     `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - every pointer named d_* is DEVICE memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()); the library never frees it.  Handles own their internal device state.
 *   - all launches are asynchronous on `stream`; nothing here synchronises the device
 *     unless documented.
 *   - return value 0 = success; non-zero = failure, message via pixie_last_error().
 *   - thread-compatible per handle; pixie_last_error() is thread-local.
 */
#ifndef PIXIE_HIP_H
#define PIXIE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* pixie_last_error(void);
/* Library/version probe: returns the gfx arch string the kernels were compiled for. */
const char* pixie_build_arch(void);
/* (No process-wide switches: every option lives on a handle -- pixie_unet_set_option, pixie_mpm_set_scalar.) */

/* ======================================================================================
 * (B) MLS-MPM solver -- replaces PG/mpm_solver_warp/mpm_solver_warp.py: MPM_Simulator_WARP
 * ====================================================================================== */
typedef struct pixie_mpm pixie_mpm;

/* MPM_Simulator_WARP.__init__/initialize (mpm_solver_warp.py:48-180): allocates particle and
 * grid state for n_particles and an n_grid^3 grid over [0,grid_lim]^3; v=0, C=0, F_trial=I. */
int pixie_mpm_create(pixie_mpm** out, int n_particles, int n_grid, double grid_lim);
int pixie_mpm_destroy(pixie_mpm* h);
/* set_parameters_dict with a new n_grid / grid_lim after the particles were loaded (mpm_solver_warp.py:315-342): the
 * reference re-allocates grid_m / grid_v_in / grid_v_out and recomputes dx, inv_dx; particle state, model scalars,
 * boundary conditions, particle modifiers and the time are untouched.  Same here, in place.  Synchronises `stream`. */
int pixie_mpm_regrid(pixie_mpm* h, int n_grid, double grid_lim, void* stream);

/* Field import/export in the reference's AoS layouts (warp_utils.py:42-74):
 *   "x","v": float[n][3]; "F","F_trial","C","stress": float[n][9] row-major;
 *   "vol","mass","density","E","nu","mu","lam","bulk","yield_stress": float[n];
 *   "material","selection": int32[n]; "init_cov","cov": float[n][6];
 *   grids (export only): "grid_m": float[ng^3], "grid_v_in","grid_v_out": float[ng^3][3].
 * Replaces import_particle_*_from_torch / export_particle_*_to_torch
 * (mpm_solver_warp.py:659-741) and wp.from_torch assignments such as gs_simulation.py:528.
 * `count` is the number of scalars in the caller's buffer (checked). */
int pixie_mpm_set_field(pixie_mpm* h, const char* name, const void* d_src, int64_t count, void* stream);
int pixie_mpm_get_field(pixie_mpm* h, const char* name, void* d_dst, int64_t count, void* stream);
/* set_value_to_{float,int}_array (warp_utils.py:222-230) as used by set_parameters_dict. */
int pixie_mpm_fill_field(pixie_mpm* h, const char* name, double value, void* stream);

/* Scalars of MPMModelStruct set by set_parameters_dict (mpm_solver_warp.py:386-433):
 * "rpic_damping","grid_v_damping_scale","hardening","xi","softening","plastic_viscosity",
 * "friction_angle","gx","gy","gz","time".
 * No reference counterpart: "compensated_x" (0, the default = the reference's float32 `x += dt v`, mpm_utils.py:447; 1 = the
 * rounding error of that sum is carried in three more words per particle and fed into the next increment, so the stored x is the
 * float32 rounding of the accumulated position: displacement error vs float64 4-8x smaller in quiet scenes, +5 % per substep),
 * "scatter_bits" (0 = by the particle-mass contrast, 32, 64), "occupancy", "item_cap" (0 = automatic: decided at every re-binning from
 * that binning's block histogram, with hysteresis; get_scalar "item_cap" returns the capacity in force), "wide", "sparse_tiles",
 * "grid_rb", "resort_interval", "xcd_order" (1, the default: the block kernel's workgroups take the block-ordered work list in
 * contiguous runs per XCD -- same bits, 2.6 % faster; 0: round-robin) (kernel variants, see csrc/mpm.hip).
 * "profile" / "trace": diagnostic switches of the PIXIE_DIAG build (libpixie_hip_diag.so); the product library accepts 0 (a no-op)
 * and refuses any other value. */
int pixie_mpm_set_scalar(pixie_mpm* h, const char* key, double value);
int pixie_mpm_get_scalar(pixie_mpm* h, const char* key, double* value);

/* get_float_array_product(density, vol, mass) (mpm_solver_warp.py:416-425). */
int pixie_mpm_update_mass(pixie_mpm* h, void* stream);
/* finalize_mu_lam / compute_bulk (mpm_solver_warp.py:465-471, 505-511; mpm_utils.py:282-293). */
int pixie_mpm_finalize_mu_lam(pixie_mpm* h, int with_bulk, void* stream);
/* apply_additional_params (mpm_utils.py:591-610): box-select E, nu, density, material. */
int pixie_mpm_apply_additional_params(pixie_mpm* h, const double point[3], const double size[3], double E,
                                      double nu, double density, int material, void* stream);
/* The same for a LIST of boxes in one launch, with the result of applying them one after the other in list order (a particle
 * inside several boxes keeps the LAST one's values).  material_field.py:343-363 uploads the material field as one 1 mm box
 * per particle -- N launches of N threads in the reference; here one launch.  Device arrays: d_boxes[n_boxes][6] =
 * (point.xyz, size.xyz) float32, d_params[n_boxes][3] = (E, nu, density) float32, d_material[n_boxes] int32. */
int pixie_mpm_apply_additional_params_batch(pixie_mpm* h, int64_t n_boxes, const float* d_boxes, const float* d_params,
                                            const int32_t* d_material, void* stream);

/* Grid boundary conditions, applied in registration order after the grid update. */
enum { PIXIE_BC_SURFACE = 0, PIXIE_BC_CUBOID = 1, PIXIE_BC_BBOX = 2 };
typedef struct pixie_bc_desc {
    int32_t type;          /* PIXIE_BC_* */
    int32_t surface_type;  /* surface collider: 0 sticky, 1 slip, 11 cut, 2 other (mpm_solver_warp.py:770-779) */
    int32_t reset;         /* cuboid (mpm_solver_warp.py:895-897) */
    int32_t pad_;
    double point[3], size[3], velocity[3], normal[3];
    double start_time, end_time, friction;
} pixie_bc_desc;
/* add_surface_collider (:749-843), set_velocity_on_cuboid (:853-908), add_bounding_box (:910-977). */
int pixie_mpm_add_bc(pixie_mpm* h, const pixie_bc_desc* bc);

/* Pre-P2G particle modifiers; masks are fixed at registration from the current positions. */
enum { PIXIE_PM_IMPULSE = 0, PIXIE_PM_TRANSLATION = 1, PIXIE_PM_ROTATION = 2 };
typedef struct pixie_pmod_desc {
    int32_t type; /* PIXIE_PM_* */
    int32_t pad_;
    double point[3], size[3];          /* box selection (mpm_utils.py:613-642) */
    double force[3];                   /* impulse: v += force/mass*dt (mpm_solver_warp.py:1015-1027) */
    double velocity[3];                /* translation pin (:1061-1073) */
    double normal[3], h1[3], h2[3];    /* rotation cylinder axes, prepared as :1092-1117 */
    double half_height, radius, rotation_scale, translation_scale;
    double start_time, end_time;
} pixie_pmod_desc;
/* add_impulse_on_particles (:982-1029), enforce_particle_velocity_translation (:1031-1075),
 * enforce_particle_velocity_rotation (:1080-1181). */
int pixie_mpm_add_particle_modifier(pixie_mpm* h, const pixie_pmod_desc* pm, void* stream);

/* p2g2p (mpm_solver_warp.py:514-637), n_substeps times with the same dt; advances h->time. */
int pixie_mpm_step(pixie_mpm* h, double dt, int n_substeps, void* stream);

/* Several independent scenes stepped together (no reference counterpart): every substep of every scene in ONE block-kernel
 * launch and ONE grid-kernel launch (one per kernel variant when the scenes differ in work-item capacity or scatter mode),
 * instead of two launches per scene.
 *   pixie_mpm_batch_create: 1 ... 32 distinct handles (kMaxBatch).  The batch owns its device tables and staging buffers, not
 *     the scenes: every handle must outlive the batch.
 *   pixie_mpm_batch_step: advances every scene by n_substeps substeps of dt on `stream`; each scene ends in exactly the bits
 *     pixie_mpm_step(h, dt, n_substeps, stream) gives it alone.  Each handle's state is re-read at the start of every call, so
 *     regrid / set_field / set_scalar / add_bc between calls are picked up.  n_substeps == 0 is a no-op.  Successive calls on
 *     different streams must be ordered by the caller, as for pixie_mpm_step.
 *   pixie_mpm_batch_run: per-scene time steps, substep counts and frame exports.  per_scene[s] (n_scenes == the batch's scene
 *     count) is scene s's frame loop, and scene s ends -- in its state and in every exported frame -- in exactly the bits of
 *       for (f = 0; f < n_chunks; ++f) {
 *           if (n_out > 0) pixie_mpm_export_frame(h, n_out, shift, scale, mean, inv_rotation,
 *                                                 d_pos + f * n_out * 3, d_cov ? d_cov + f * n_out * 6 : NULL, stream);
 *           pixie_mpm_step(h, dt, steps_per_chunk, stream);
 *       }
 *     (a ragged run is n_chunks = 1, n_out = 0; steps_per_chunk * n_chunks == 0 leaves the scene untouched).  Substep j of every
 *     scene is global step j of the call: one grid-kernel launch per global step covers every scene that still has substeps, so
 *     a call issues max_s(steps_per_chunk * n_chunks) grid launches; the exports of the scenes that start a frame at the same
 *     global step are one launch.  Chunk boundaries are kept as given (each is a pixie_mpm_step call of the solo loop).  The
 *     tables are built and uploaded in windows of 1024 global steps, so a call may be arbitrarily long.  Asynchronous on `stream`
 *     apart from the synchronisations a re-binning does.  Also refused: dt <= 0 or not finite, negative counts, n_scenes not the
 *     batch's scene count, n_out < 0 or > the scene's particle count, n_out > 0 with a null d_pos or a zero scale.
 *     pixie_mpm_batch_step(b, dt, n, stream) is the same call with every scene at (dt, n, 1 chunk, no export).
 * All three refuse -- with a pixie_last_error message, before anything is launched or changed -- a null or repeated handle, an
 * empty or too long list, a scene with a phase-API P2G pending, with `trace` set, with more than 16 boundary conditions or with
 * more than 8 particle modifiers (the cases pixie_mpm_step serves with extra launches). */
typedef struct pixie_mpm_batch pixie_mpm_batch;
typedef struct pixie_batch_sched {
    double dt;                         /* > 0 */
    int32_t steps_per_chunk;           /* substeps per frame (>= 0) */
    int32_t n_chunks;                  /* frames (>= 0) */
    int32_t n_out;                     /* particles exported per frame (caller order); 0: no export */
    int32_t pad_;
    double shift[3], scale, mean[3];   /* the export transform of pixie_mpm_export_frame */
    double inv_rotation[9];
    float* d_pos;                      /* [n_chunks][n_out][3] */
    float* d_cov;                      /* [n_chunks][n_out][6] or NULL */
} pixie_batch_sched;
int pixie_mpm_batch_create(pixie_mpm_batch** out, pixie_mpm* const* handles, int n_handles);
int pixie_mpm_batch_step(pixie_mpm_batch* b, double dt, int n_substeps, void* stream);
int pixie_mpm_batch_run(pixie_mpm_batch* b, const pixie_batch_sched* per_scene, int n_scenes, void* stream);
/* pixie_mpm_batch_run with 3DGS splats: a scene s with splats[s] set exports, per frame, (pos, cov) and the log-scales and
 * quaternions of pixie_mpm_export_frame_splats, bit for bit as that call in its solo loop.  At an export step the scenes without
 * splats keep pixie_mpm_batch_run's export launch and those with splats share a second one.  splats == NULL, or every entry
 * {NULL, NULL}: exactly pixie_mpm_batch_run's launches.  Refused before anything runs: only one of the two pointers set, splats
 * with n_out == 0 or with a null d_cov. */
typedef struct pixie_batch_splat_out {
    float* d_log_scale;                /* [n_chunks][n_out][3] or NULL */
    float* d_quat;                     /* [n_chunks][n_out][4] (wxyz) or NULL */
} pixie_batch_splat_out;
int pixie_mpm_batch_run_splats(pixie_mpm_batch* b, const pixie_batch_sched* per_scene, const pixie_batch_splat_out* splats /* [n_scenes] or NULL */,
                               int n_scenes, void* stream);
int pixie_mpm_batch_destroy(pixie_mpm_batch* b);

/* compute_cov_from_F (mpm_utils.py:529-553) and compute_R_from_F (:556-580) as used by
 * export_particle_cov_to_torch / export_particle_R_to_torch (mpm_solver_warp.py:702-741). */
int pixie_mpm_export_cov(pixie_mpm* h, float* d_cov /* [n][6] */, void* stream);
int pixie_mpm_export_R(pixie_mpm* h, float* d_R /* [n][9] */, void* stream);
/* Per-frame export for the rasteriser (PG/gs_simulation.py:591-600 with PG/utils/transformation_utils.py:19-20,108-130):
 * positions and covariances of the first n_out particles (caller order) back in the original scene frame,
 *   pos = ((x - shift) / scale + mean) @ M,   cov = M^T (F_trial init_cov F_trial^T / scale^2) M
 * where shift = (1, 1, 1 + z_shift) (undoshift2center111), scale / mean come from transform2origin and
 * M = R_k ... R_1 is the product apply_inverse_rotations walks (row-major 3x3).  d_cov may be NULL.  One launch. */
int pixie_mpm_export_frame(pixie_mpm* h, int n_out, const double shift[3], double scale, const double mean[3],
                           const double inv_rotation[9], float* d_pos /* [n_out][3] */, float* d_cov /* [n_out][6] or NULL */,
                           void* stream);
/* 3DGS splat parameters of a covariance (cov3D_to_log_scales_and_quats, PG/gs_simulation.py:253-288): per row of d_cov
 * (s11, s12, s13, s22, s23, s33), the eigenvalues in descending order as log_scale = 0.5 log(max(lambda, 1e-12)) and the
 * eigenvector matrix R (columns) as a unit quaternion (w, x, y, z), w >= 0.  R's signs are fixed: columns 0 and 1 have their
 * largest-magnitude component positive, column 2 = col0 x col1 (right-handed).  Double-precision Jacobi inside.  n == 0 is a
 * no-op; n < 0 and null pointers are refused.  One launch. */
int pixie_splat_from_cov(const float* d_cov /* [n][6] */, int64_t n, float* d_log_scale /* [n][3] */, float* d_quat /* [n][4] wxyz */,
                         void* stream);
/* pixie_mpm_export_frame with the splats of the exported covariances (the per-frame PLY of PG/gs_simulation.py:290-322) in the same
 * launch: d_log_scale / d_quat are the bits pixie_splat_from_cov gives for d_cov.  Every output is required. */
int pixie_mpm_export_frame_splats(pixie_mpm* h, int n_out, const double shift[3], double scale, const double mean[3],
                                  const double inv_rotation[9], float* d_pos /* [n_out][3] */, float* d_cov /* [n_out][6] */,
                                  float* d_log_scale /* [n_out][3] */, float* d_quat /* [n_out][4] */, void* stream);
/* Particles whose 3x3x3 stencil left the grid (undefined behaviour in the reference).  Here such a particle is frozen
 * (selection <- 2: it neither moves nor scatters mass again) and counted ONCE; slow-path particles that drifted out of
 * every active block between two re-binnings are dropped from that substep's P2G and counted too.  Synchronises
 * `stream`.  pixie_mpm_get_scalar("lost_particles_seen") returns the same count as of the last re-binning without
 * synchronising (the Python shim warns when it becomes non-zero). */
int pixie_mpm_out_of_bounds(pixie_mpm* h, int64_t* count, void* stream);

/* ======================================================================================
 * (A) 3D U-Net operators -- replace the torch ops under WG/models/module/diffusion_network.py
 *     (MyUNetModel :712-935, MyResBlock :639-710, FeatureProjector :534-589, AttentionBlock
 *     :192-242, Upsample/Downsample :51-97).  Activations are NCDHW float32, batch 1.
 * ====================================================================================== */

/* Prologue applied to every input element before the convolution (i.e. the normalisation +
 * activation that precede each conv in the reference graph), fused into the tile load:
 *   t = x * a[c] + b[c]                       (a,b: per-channel, from pixie_norm_finalize)
 *   t = t * gamma[d,h,w] + beta[d,h,w]        (if d_gamma != NULL: spatial LayerNorm affine)
 *   t = act(t):  0 none, 1 LeakyReLU(0.02), 2 SiLU
 * Zero padding applies to the activated tensor, as in the reference. */
typedef struct pixie_conv_desc {
    /* input: channel-concatenation of up to two tensors (th.cat([h, skip]), :932) */
    const float* d_in0; int32_t c0;
    const float* d_in1; int32_t c1;           /* d_in1 may be NULL (c1 = 0) */
    int32_t in_d, in_h, in_w;                 /* spatial size of the stored input tensors */
    int32_t upsample;                         /* 1: nearest x2 before the conv (Upsample :67-72) */
    int32_t stride;                           /* 1, or 2 (Downsample :89-91) */
    int32_t ksize;                            /* 3 (padding 1) or 1 (padding 0) */
    /* prologue */
    const float* d_pro_a; const float* d_pro_b;   /* [c0+c1] or NULL = identity */
    const float* d_gamma; const float* d_beta;    /* [D][H][W] of the conv-input grid, or NULL */
    int32_t act;
    /* weights, repacked by pixie_conv_pack_weights: [k^3][c_in][c_out_padded] */
    const float* d_w; const float* d_bias;        /* bias [c_out] or NULL */
    int32_t c_out;
    /* epilogue: out = conv + bias (+ residual) */
    const float* d_residual;                      /* [c_out][OD][OH][OW] or NULL; may alias d_out */
    float* d_out;                                 /* [c_out][OD][OH][OW] */
    /* f16x3 path (conv3d_f16x3.hip): used instead of d_w when d_w16 != NULL.  Requires stride 1, c0 % 8 == 0 and
     * (c0+c1) % 16 == 0.  The kernel scales the (prologue-transformed) input by a power of two chosen from
     * a bound on its magnitude so that it sits just below the fp16 range before the hi/lo split:
     *   - raw inputs (no prologue): d_in_amax0/1 point at the tensors' |x|max as float bits
     *     (pixie_channel_stats / pixie_tensor_amax keep them on the device -- no host sync);
     *   - normalised inputs: in_bound is a host-side bound on |prologue(x)| (sqrt(N)*max|gamma|+max|beta|). */
    const void* d_w16;                            /* from pixie_conv_pack_weights_f16x2, or NULL */
    const uint32_t* d_in_amax0; const uint32_t* d_in_amax1;
    float in_bound;
    /* f16x3 path only, optional: statistics of the OUTPUT taken in the epilogue (what the next layer's LayerNorm /
     * GroupNorm and the next f16x3 conv's scaling need), instead of a separate pass over the tensor:
     *   d_out_stats: pixie_conv_stats_floats(desc) floats of partial sums (per tile in fp32; a split-K launch: per segment
     *   of its reduce in fp64, so 8-byte aligned), finalised into the double[2*c_out] layout of pixie_channel_sums by
     *   pixie_stats_finalize or pixie_stats_norm_finalize; d_out_amax: |out|max (float bits), atomicMax'ed (caller zeroes). */
    float* d_out_stats;
    uint32_t* d_out_amax;
    /* f16x3 path only, optional: pixie_conv_workspace_bytes(desc) bytes of device scratch.  With it, layers whose output
     * is too small to fill the chip (the 16^3 / 32^3 levels) split their channel chunks over up to 8 workgroup slices
     * (deterministic: partial outputs are added in a fixed order); the reduce over the slices then takes d_out_stats. */
    void* d_workspace;
    /* Output extent, 0 = the natural size ((in * (upsample ? 2 : 1) + 2 pad - ksize) / stride + 1).  A smaller value crops
     * the trailing planes / rows / columns: the odd-grid crop h[..., :-1] that MyUNetModel.forward applies to an
     * up-sampled tensor before concatenating it with an odd-sized skip tensor (diffusion_network.py:925-930), done by not
     * computing the cropped voxels (d_out, d_residual and the output statistics all have the cropped extent). */
    int32_t out_d, out_h, out_w;
    /* f16x3 path only, optional: the residual block's 1x1x1 skip convolution (MyResBlock.skip_connection,
     * diffusion_network.py:691,705) folded into this launch:  out = conv(prologue(in)) + bias + skip_conv(skip_in) + skip_bias.
     * skip_in is the channel concatenation of up to two RAW tensors with the spatial size of the output; d_skip_w16 comes from
     * pixie_conv_pack_weights_f16x2(w_skip, ., c_out, skip_c0 + skip_c1, 1), d_skip_amax0/1 are the tensors' |x|max slots.
     * The skip tensor is then never written or read.  Only where pixie_conv_skip_foldable() says so (stride 1, no upsample,
     * no split-K); d_residual may still be given as well. */
    const float* d_skip_in0; int32_t skip_c0;
    const float* d_skip_in1; int32_t skip_c1;
    const void* d_skip_w16; const float* d_skip_bias;
    const uint32_t* d_skip_amax0; const uint32_t* d_skip_amax1;
    /* f16x3 path only: 1 = d_w16 comes from pixie_conv_pack_weights_subpixel and the launch is the sub-pixel form of a 3^3
     * convolution behind a nearest x2 upsampling (upsample = 1, ksize = 3, stride = 1; no folded skip): per output parity a
     * 2x2x2 convolution over the stored tensor with pre-summed weights, 8 taps instead of 27.  Same prologue, crop,
     * residual, statistics and split-K as the 27-tap form; results differ from it only by the summation order.  The
     * size queries above follow this field.  The prologue runs on the stored tensor before the upsampling, so d_gamma / d_beta,
     * refused with upsample = 1 otherwise, are allowed here and are [in_d][in_h][in_w]. */
    int32_t w16_subpixel;
} pixie_conv_desc;

/* Repack an nn.Conv3d / nn.Conv1d weight (c_out, c_in, k,k,k) into the kernel's
 * [tap][c_in][c_out_padded] layout; c_out_padded = pixie_conv_cout_padded(c_out). */
int pixie_conv_cout_padded(int c_out);
int pixie_conv_pack_weights(const float* d_w_oidhw, float* d_w_packed, int c_out, int c_in, int ksize, void* stream);
/* The same weight, split into fp16 hi/lo halves (w*s = hi + lo, s a power of two chosen on the device from
 * |w|max) and swizzled for the f16 MFMA A operand; d_packed needs pixie_conv_packed16_bytes() bytes. */
int64_t pixie_conv_packed16_bytes(int c_out, int c_in, int ksize);
int pixie_conv_pack_weights_f16x2(const float* d_w_oidhw, void* d_packed, int c_out, int c_in, int ksize, void* stream);
/* Sub-pixel packing of a 3^3 weight (c_out, c_in, 3,3,3) for pixie_conv_desc.w16_subpixel: the taps that read the same stored
 * voxel after a nearest x2 upsampling are summed in fp32 per output parity, then scaled by |summed w|max and split as above,
 * [parity 8][tap 8][c_in/8][c_out_padded].  pixie_conv_subpixel_bytes is 0 where the path does not apply (c_in % 16 != 0). */
int64_t pixie_conv_subpixel_bytes(int c_out, int c_in);
int pixie_conv_pack_weights_subpixel(const float* d_w_oidhw, void* d_packed, int c_out, int c_in, void* stream);
/* F.conv3d / nn.Conv3d forward: exact-fp32 MFMA path (d_w), or the f16x3 split path (d_w16). */
int pixie_conv3d_forward(const pixie_conv_desc* desc, void* stream);
/* Epilogue statistics of the f16x3 path: buffer size in floats for desc->d_out_stats (0: layer not on that path), and
 * the reduction of that buffer to d_sums[2*c] = (sum, sum of squares) in float64. */
int64_t pixie_conv_stats_floats(const pixie_conv_desc* desc);
int64_t pixie_conv_workspace_bytes(const pixie_conv_desc* desc);
int pixie_stats_finalize(const float* d_stats, const pixie_conv_desc* desc, double* d_sums, void* stream);
/* pixie_stats_finalize and pixie_norm_finalize (below) in one launch, over the channel concatenation of up to two tensors:
 * part 0 has desc0->c_out channels, part 1 (optional) c1.  A part given with its d_stats/desc has its partials added into
 * its d_sums (written); a part with d_stats NULL has final d_sums already (read).  d_a / d_b get c_out + c1 entries. */
int pixie_stats_norm_finalize(const float* d_stats0, const pixie_conv_desc* desc0, double* d_sums0, const float* d_stats1,
                              const pixie_conv_desc* desc1, double* d_sums1, int c1, int64_t spatial, int mode, int groups,
                              double eps, const float* d_weight, const float* d_bias, float* d_a, float* d_b, void* stream);
/* 1 if this descriptor's launch (its shape fields, d_w16 and d_workspace as they will be passed) can take a folded skip
 * convolution with skip_c0 + skip_c1 input channels; the skip pointers themselves need not be set yet. */
int pixie_conv_skip_foldable(const pixie_conv_desc* desc);

/* Per-channel sum and sum of squares over the spatial extent: d_sums[2*c] (float64). */
int pixie_channel_sums(const float* d_x, int channels, int64_t spatial, double* d_sums, void* stream);
/* Same, and additionally atomicMax's the tensor's |x|max (as float bits) into *d_amax (caller zeroes it). */
int pixie_channel_stats(const float* d_x, int channels, int64_t spatial, double* d_sums, uint32_t* d_amax, void* stream);
/* |x|max of `count` floats, atomicMax'ed (as float bits) into *d_slot (caller zeroes it). */
int pixie_tensor_amax(const float* d_x, int64_t count, uint32_t* d_slot, void* stream);
/* Turn channel sums into the prologue's (a,b):
 *  mode 0: LayerNorm([D,H,W]) statistics per channel (biased var, eps): a = rstd, b = -mean*rstd
 *          (affine gamma/beta are spatial and applied in the conv prologue);
 *  mode 1: GroupNorm(groups, channels): a = rstd_g*weight[c], b = bias[c] - mean_g*rstd_g*weight[c]. */
int pixie_norm_finalize(const double* d_sums, int channels, int64_t spatial, int mode, int groups, double eps,
                        const float* d_weight, const float* d_bias, float* d_a, float* d_b, void* stream);

/* QKVAttention (diffusion_network.py:218-242), single head: qkv [3C][T] -> out [C][T],
 * softmax over keys of (q*s)^T(k*s), s = C^-1/4, streamed (no T x T buffer). */
int pixie_attention_forward(const float* d_qkv, float* d_out, int channels, int tokens, void* stream);

/* y = x*a[c] + b[c] materialised (GroupNorm output feeding a non-conv consumer). */
int pixie_channel_affine(const float* d_x, const float* d_a, const float* d_b, float* d_y, int channels,
                         int64_t spatial, void* stream);

/* The voxel-grid loader of the reference's dataset item (WG/data_utils/my_data.py:160-224; features are written as
 * (D,H,W,C) float16 by pixie/voxel/voxelize.py:86,111): .astype(float32) + permute to (C,D,H,W), on the device. */
int pixie_voxel_grid_to_ncdhw(const void* d_feat_dhwc_f16, int d, int h, int w, int channels, float* d_out_cdhw, void* stream);

/* FeatureProjector.net[0] -- Conv3d(C, c_out, 1) + bias (diffusion_network.py:556-560) -- of one or two networks applied
 * to the voxel grid as the reference stores it: (voxels, C) float16, channels last (pixie/voxel/voxelize.py:86,111; what
 * WG/data_utils/my_data.py:160-224 converts to float32 and permutes first).  One launch reads the grid once and writes
 * d_out[n] = (c_out, voxels) float32 for each network n.  d_w16[n] comes from pixie_conv_pack_weights_f16x2(w, ., c_out,
 * C, 1): the inputs are exact fp16 numbers, so only the weights are split (two f16 MFMAs per product, fp32 accumulate).
 * Requires C % 16 == 0 and n_networks * padded(c_out) in {64, 128, 256} (the reference shapes: c_out = 128, one or two
 * networks); other shapes go through pixie_voxel_grid_to_ncdhw + pixie_conv3d_forward. */
int pixie_projector_conv0(const void* d_feat_dhwc_f16, int64_t voxels, int channels, int n_networks, const void* const* d_w16,
                          const float* const* d_bias, float* const* d_out, int c_out, void* stream);

/* The field exchange between ranks (the reference writes a 44 B/voxel (11, D, D, D) float file per scene and has no
 * exchange): n_scenes x (3, V) float32 continuous channels + n_scenes x V int32 class ids -> the 13 B/voxel wire buffer
 * [3 n V float32 | n V uint8 | zero pad to a multiple of 16 B] that ONE all-gather moves (pixie_amd/distributed.py).  One launch. */
int pixie_pack_fields(const float* d_cont, const int32_t* d_seg_pred, int64_t n_scenes, int64_t spatial, void* d_wire, int64_t wire_bytes,
                      void* stream);

/* process_batch/save_predictions (WG/trainer/inference_combined.py:124-126,186-195):
 * combined[0:3] = cont_pred; combined[3+k] = (argmax_c logits == k), ties -> lowest index. */
int pixie_combine_predictions(const float* d_logits, int num_classes, const float* d_cont, int64_t spatial,
                              float* d_combined, int32_t* d_argmax /* may be NULL */, void* stream);

/* save_predictions given class ids (WG/trainer/inference_combined.py:173-199): combined[0:3] = cont_pred,
 * combined[3 + k] = (seg_pred == k) for k < num_classes (an id outside [0, num_classes) leaves every class channel 0). */
int pixie_combine_class_ids(const int32_t* d_seg_pred, int num_classes, const float* d_cont, int64_t spatial, float* d_combined,
                            void* stream);

/* --------------------------------------------------------------------------------------
 * (A') One network as a handle -- what the reference does with an nn.Module: construction (MyUNetModel.__init__,
 *      diffusion_network.py:712-873, FeatureProjector :534-589, behind SegmentationUNet / RegressionUNet,
 *      trainer/training_discrete.py:50-88, trainer/training_continuous_mse.py:48-89), load_state_dict and
 *      forward (:875-935) -- so that a scene costs ONE foreign call per network instead of ~400 operator calls.
 *      The launch sequence equals pixie_amd/unet.py: UNetRunner.forward (bit-identical results); it allocates
 *      nothing and never synchronises once the weights are packed, i.e. it can be captured into a HIP graph.
 * -------------------------------------------------------------------------------------- */
typedef struct pixie_unet pixie_unet;
typedef struct pixie_unet_config {          /* the constructor arguments of the two wrappers */
    int32_t feature_channels, cond_dim, model_channels, num_res_blocks;
    int32_t n_channel_mult; int32_t channel_mult[8];
    int32_t n_attention_resolutions; int32_t attention_resolutions[8];
    int32_t grid_size;                      /* D = H = W of the feature grid (the LayerNorm([D,H,W]) parameters have this shape) */
    int32_t out_channels;                   /* num_classes (segmentation) or 3 (regression) */
    int32_t precision;                      /* 0: f16x3 convolutions where the shapes allow (default path), 1: exact fp32 MFMA everywhere */
} pixie_unet_config;

int pixie_unet_create(pixie_unet** out, const pixie_unet_config* cfg);
int pixie_unet_destroy(pixie_unet* h);
/* The state_dict: keys in the reference's registration order (a reference checkpoint loads key by key). */
int pixie_unet_param_count(const pixie_unet* h);
int pixie_unet_param_info(const pixie_unet* h, int index, const char** key, int64_t* numel, int32_t* ndim, int64_t shape[5]);
/* Point parameter `key` at `numel` float32 values in device memory.  The memory stays the caller's and must outlive the
 * handle's use of it; call again after changing the values (conv weights are re-packed, normalisation bounds re-taken, on
 * the next forward).  An unknown key or a wrong size is an error, as with load_state_dict(strict=True). */
int pixie_unet_set_param(pixie_unet* h, const char* key, const float* d_values, int64_t numel);
/* Bytes of device scratch one forward pass over a (d, h, w) grid needs (all activations, statistics and split-K buffers). */
int64_t pixie_unet_workspace_bytes(pixie_unet* h, int d, int hh, int w);
/* forward: d_feat (feature_channels, d, h, w) float32 -> d_out (out_channels, d, h, w) float32, all launches on `stream`.
 * d_proj0 (optional, hidden-128 projector only): the output of projector.net[0] computed elsewhere (pixie_projector_conv0 on
 * the channels-last grid); d_feat may then be NULL.  The first call after pixie_unet_set_param packs weights (hipMalloc) and
 * synchronises the stream once to read the normalisation bounds; later calls are launch-only. */
int pixie_unet_forward(pixie_unet* h, const float* d_feat, const float* d_proj0, int d, int hh, int w, float* d_out,
                       void* d_workspace, int64_t workspace_bytes, void* stream);
/* Two networks over ONE input on one stream: the outputs of pixie_unet_forward(h0, d_feat, NULL, ..., d_out0, ...) and of the same
 * call for h1, bit for bit, from one interleaved sequence of launches.  Both plans are walked into launch lists
 * (csrc/launch_list.h), then launched as: h0's full-resolution encoder section, h1's, the levels below full resolution of both
 * zipped -- two launches at the same position that run the same kernel on the same grid go out as one launch of that kernel's
 * grouped form (the split-K reduces, the statistics finalisers and the conv instantiations of conv16_group_kernel()'s table in
 * csrc/conv3d_f16x3.hip have one) --, h0's decoder section, h1's.  h1 takes over the
 * input statistics h0's pass computes.  Networks that differ in shape or precision only group less.  Both workspaces are in use
 * at once: each at least pixie_unet_workspace_bytes of its network, distinct.  No d_proj0 route; the handles' "graph" option
 * does not apply (the sequence is capturable by the caller).  launch_counts (optional): the launches of the two single passes,
 * the launches issued, how many of those are grouped, and how many of the grouped ones are convolutions (launches with dynamic
 * LDS).  PIXIE_UNET_PAIR_GROUP=0 in the environment: zipped, nothing grouped. */
int pixie_unet_forward_pair(pixie_unet* h0, pixie_unet* h1, const float* d_feat, int d, int hh, int w, float* d_out0, float* d_out1,
                            void* d_workspace0, int64_t workspace0_bytes, void* d_workspace1, int64_t workspace1_bytes, void* stream,
                            int32_t launch_counts[4]);
/* Options.  "graph" = 1: pixie_unet_forward records its launch sequence the first time it sees a combination of
 * (d_feat, d_proj0, d_out, d_workspace) pointers and replays it as ONE hipGraphLaunch on later calls with the same pointers
 * (a caller that keeps its buffers; up to 4 combinations are kept; pixie_unet_set_param invalidates them).  Needs a
 * non-default stream.  Same kernels, same arguments: bit-identical output. */
int pixie_unet_set_option(pixie_unet* h, const char* key, int value);

/* ======================================================================================
 * (C) Field -> particle transfer between the two halves: replaces the PLY round trip
 *     pixie/voxel/map_pred_to_coords.py:41-75,192-252 (unscale_prediction + masked voxel point list) and
 *     PG/material_field.py:228-300 perform_knn_smoothing (sklearn K-NN + a Python loop over every particle;
 *     MaterialProperties.assign_from_neighbors :52-78, .get_defaults :38-50).
 * ====================================================================================== */
typedef struct pixie_field_desc {
    const float* d_pred;        /* network output (3 + n_classes, D, H, W): cont channels in [-1,1] units, class scores / one-hot */
    const uint8_t* d_mask;      /* (D, H, W) occupancy, > 0 = a material point (clip_features_mask) */
    const float* d_axis_x; const float* d_axis_y; const float* d_axis_z;  /* voxel coordinates: float32(np.linspace(min, max, D)) per axis */
    int32_t n_classes, d, h, w;
    double min_spacing;         /* smallest lattice spacing of the three axes */
    double density_min, density_max, E_min, E_max, nu_min, nu_max;  /* normalization_stats/normalization_ranges.yaml */
} pixie_field_desc;
/* For each of the n particles (d_pos: float[n][3] in the field's coordinate frame) the k (<= 16) nearest material points;
 * continuous properties = mean (or inverse-distance weighted mean) of the un-scaled neighbours, material id / part label =
 * mode (ties: first in distance order; weighted: largest vote, ties to the smallest id), d_nearest = distance to the nearest
 * point.  Particles whose nearest point is farther than nn_distance_threshold get the defaults (mean over all material
 * points, default_material, default_part_label).  d_scratch: 64 bytes of device memory; after the call it holds
 * double[5] = sums of (density, E, nu, conf) over the material points and their count, then uint64 = number of too-far
 * particles.  Asynchronous on `stream`. */
int pixie_field_to_particles(const pixie_field_desc* field, const float* d_pos, int n, int k, double nn_distance_threshold,
                             int weighted, int default_material, int default_part_label, float* d_density, float* d_E,
                             float* d_nu, int32_t* d_material, int32_t* d_part_label, float* d_conf, float* d_nearest,
                             void* d_scratch, void* stream);

/* unscale_prediction (pixie/voxel/map_pred_to_coords.py:41-75): d_out[(channels, spatial)] = d_pred with channels 0..2
 * clipped to [-1, 1] and mapped back to physical units -- density and E through 10^(log-range), nu linearly, with the
 * ranges of normalization_stats/normalization_ranges.yaml; the class channels (3..) are copied.  float32 arithmetic,
 * as numpy does on the float32 array.  d_out may alias d_pred. */
int pixie_unscale_prediction(const float* d_pred, int channels, int64_t spatial, double density_min, double density_max,
                             double E_min, double E_max, double nu_min, double nu_max, float* d_out, void* stream);
/* The masked voxel point list map_pred_to_ply writes to its PLY (map_pred_to_coords.py:192-252): for every voxel with
 * mask > 0, in C order of the grid, its coordinates (the float32 lattice axes of `field`), un-scaled density / E / nu,
 * material id (argmax of the class channels, first maximum; a single class channel is the id itself, :122-126) and
 * confidence (the winning class score; 1 for a single channel).  *d_count (device int64) receives the number of points;
 * at most `capacity` records are written (call with capacity 0 to only count).  d_scratch needs
 * pixie_field_points_scratch_bytes(field) bytes.  Stable compaction, three launches, asynchronous on `stream`. */
int64_t pixie_field_points_scratch_bytes(const pixie_field_desc* field);
int pixie_field_points(const pixie_field_desc* field, int64_t capacity, float* d_xyz /* [n][3] */, float* d_density, float* d_E,
                       float* d_nu, int32_t* d_material, float* d_conf, int64_t* d_count, void* d_scratch, void* stream);

/* Density clustering of the "stationary" particles -- sklearn.cluster.DBSCAN(eps, min_samples).fit_predict at
 * PhysGaussian/material_field.py:405-406 -- up to the numbering: d_root[i] (ORIGINAL order) = the lowest original index among
 * the core points of point i's cluster (core points: their component; border points: the smallest such root among the core
 * points within eps), or -1 for noise.  Clusters numbered by ascending root are DBSCAN's labels.  The caller bins the points:
 * d_pos_sorted [n][3] sorted by cell id ((cx * ny + cy) * nz + cz of floor((p - lo) / cell_size), clamped), d_orig_index[s] the
 * original index of sorted point s, d_cell_start[nx*ny*nz + 1] the first sorted index of every cell; cell_size >= eps.
 * d_core_scratch / d_parent_scratch: n int32 each.  Distances in float64 on the float32 coordinates.  Three launches. */
int pixie_dbscan_roots(const float* d_pos_sorted, const int32_t* d_orig_index, const int32_t* d_cell_start, int n, int nx, int ny, int nz,
                       const double lo[3], double cell_size, double eps, int min_samples, int32_t* d_core_scratch,
                       int32_t* d_parent_scratch, int32_t* d_root, void* stream);

/* ======================================================================================
 * (D) Particle pre-pass of the MPM program: replaces the Taichi kernels of
 *     PG/particle_filling/filling.py that gs_simulation.py:442-482 runs before the solver is created.
 * ====================================================================================== */
/* densify_grids + compute_density (filling.py:13-92): for each of n Gaussians (d_pos [n][3], d_opacity [n], d_cov6 [n][6] =
 * xx,xy,xz,yy,yz,zz) count it in its cell (d_grid_count[grid_n^3] += 1) and splat opacity * mean_corners exp(-d^T C^-1 d / 2)
 * onto every cell within ceil(sqrt(max eigenvalue) / grid_dx) cells (d_grid_density[grid_n^3], accumulated; caller zeroes
 * both grids).  Particles outside the grid are not counted (the reference indexes unchecked). */
int pixie_fill_densify(const float* d_pos, const float* d_opacity, const float* d_cov6, int n, int grid_n, double grid_dx,
                       int32_t* d_grid_count, float* d_grid_density, void* stream);
/* fill_dense_grids (filling.py:95-121): every cell with density > density_thres and fewer than max_particles_per_cell
 * particles is topped up: new points at (cell + u) * grid_dx, u uniform in [0,1)^3 from a counter-based hash of (seed, cell,
 * k) -- ti.random() in the reference -- appended at d_new_particles[*d_counter ...]; *d_counter (device uint64) advances even
 * past max_samples (nothing is written there), so the caller can detect the overflow the reference would write through. */
int pixie_fill_dense_cells(int32_t* d_grid_count, const float* d_grid_density, int grid_n, double grid_dx, double density_thres,
                           int max_particles_per_cell, float* d_new_particles /* [max_samples][3] */, int64_t max_samples,
                           uint64_t* d_counter, uint32_t seed, void* stream);
/* internal_filling with collision_search / collision_times (filling.py:124-244): an EMPTY cell whose rays in all six axis
 * directions except exclude_dir (0:+x 1:-x 2:+y 3:-y 4:+z 5:-z) meet a cell with density > threshold, and whose ray along
 * ray_cast_dir crosses the surface an odd number of times, is filled with max_particles_per_cell points. */
int pixie_fill_internal_cells(int32_t* d_grid_count, const float* d_grid_density, int grid_n, double grid_dx, int max_particles_per_cell,
                              int exclude_dir, int ray_cast_dir, double threshold, float* d_new_particles, int64_t max_samples,
                              uint64_t* d_counter, uint32_t seed, void* stream);
/* get_particle_volume (filling.py:247-288): d_vol[p] = grid_dx^3 / (particles in p's cell).  d_grid_count_scratch:
 * grid_n^3 int32 of scratch (zeroed here). */
int pixie_particle_volume(const float* d_pos, int n, int grid_n, double grid_dx, int32_t* d_grid_count_scratch, float* d_vol, void* stream);
/* get_attr_from_closest (filling.py:383-403): d_nearest[i] = index of the original particle closest to new particle i
 * (first minimum in index order; brute force through LDS tiles). */
int pixie_nearest_particle(const float* d_pos, int n, const float* d_new_pos, int n_new, int32_t* d_nearest, void* stream);

/* ======================================================================================
 * (D) Forward 3D Gaussian splatting rasteriser -- the per-frame render of PG/gs_simulation.py:610-619
 *     (diff_gaussian_rasterization.GaussianRasterizer, forward only) and PG/utils/render_utils.py:113-130 (convert_SH).
 * ====================================================================================== */
/* One render.  viewmatrix / projmatrix are the 16 floats of the reference's world_view_transform / full_proj_transform tensors in
 * memory order (row-vector convention: p_view = [p, 1] . V).  The covariance is either d_cov3d ([n][6] upper triangle) or is built
 * from scale_modifier * d_scales ([n][3]) and d_rotations ([n][4], wxyz, used un-normalised); exactly one of the two forms.
 * d_colors is [n][3], d_opacity [n].  Outputs: d_out_color [3][height][width], d_radii [n] (0 = culled); d_final_T
 * [height][width] (transmittance left) and d_n_contrib [height][width] (position in the pixel's tile list of the last Gaussian
 * that contributed) where not NULL.  d_workspace: 16-byte aligned device memory of workspace_bytes bytes. */
typedef struct pixie_raster_desc {
    int32_t n, width, height;
    float tanfovx, tanfovy, scale_modifier;
    float viewmatrix[16], projmatrix[16], bg[3];
    int32_t pad_;
    const float* d_means;              /* [n][3] */
    const float* d_cov3d;              /* [n][6] or NULL */
    const float* d_scales;             /* [n][3] or NULL */
    const float* d_rotations;          /* [n][4] or NULL */
    const float* d_colors;             /* [n][3] */
    const float* d_opacity;            /* [n] */
    float* d_out_color;
    int32_t* d_radii;
    float* d_final_T;                  /* or NULL */
    int32_t* d_n_contrib;              /* or NULL */
    void* d_workspace;
    int64_t workspace_bytes;
} pixie_raster_desc;
/* Bytes of workspace a render of n Gaussians at width x height needs when the Gaussians touch max_instances tiles in total
 * (an instance = one Gaussian in one 16x16 tile).  -1 on error. */
int64_t pixie_raster_workspace_bytes(int n, int width, int height, int64_t max_instances);
/* Projects every Gaussian and counts the instances, synchronises `stream` ONCE to read that count (*instances_out, where not
 * NULL), then -- asynchronously -- duplicates, sorts by (tile, depth; equal keys keep index order, so the image is reproducible bit
 * for bit), and blends every pixel front to back: alpha = min(0.99, opacity exp(power)), skipped below 1/255, the pixel stops
 * when T (1 - alpha) < 1e-4, out = C + T bg.  A workspace that is too small for the count returns non-zero before anything is
 * rendered: d_radii is written, the image outputs are untouched, and pixie_last_error() and *instances_out give the count needed.
 * n == 0 or zero instances: the background. */
int pixie_raster_forward(const pixie_raster_desc* desc, int64_t* instances_out, void* stream);
/* convert_SH: d_out[i] = max(SH_degree(d_shs[i]; dir_i) + 0.5, 0) with dir_i = normalise(d_pos[i] - campos), for i < n_rot first
 * rotated by the row-major 3x3 d_rot[i].  d_shs is [n][k_coeffs][3], k_coeffs >= (degree + 1)^2, degree 0..3.  One launch. */
int pixie_sh_to_rgb(const float* d_shs, int64_t n, int k_coeffs, int degree, const float* d_pos /* [n][3] */, const float campos[3],
                    const float* d_rot /* [n_rot][9] or NULL */, int64_t n_rot, float* d_out /* [n][3] */, void* stream);

/* A frame sequence in one call: `views` renders of the same n = n_dyn + n_static Gaussians at one image size.  Each view has its
 * own camera (a host array of pixie_raster_view); width, height, bg and scale_modifier are shared (scale_modifier is carried for
 * symmetry with pixie_raster_desc: the batch takes precomputed covariances only, which it does not scale).
 * Geometry comes in two segments.  The dynamic one differs per view: d_means [views][n_dyn][3] and d_cov3d [views][n_dyn][6], view
 * v starting means_view_stride / cov3d_view_stride ELEMENTS after view v - 1 (a slice of a larger (F, N, .) tensor needs no copy; 0
 * shares one set among all views).  The static tail, d_static_means [n_static][3] and d_static_cov3d [n_static][6], is the same in
 * every view and is indexed after the dynamic Gaussians (the unselected Gaussians of PG/gs_simulation.py:602-606 without the
 * per-frame concatenation).  d_opacity is [n].  Exactly one colour source: d_colors ([n][3] per view, colors_view_stride elements
 * apart, 0 = shared), or d_shs [n][k_coeffs][3] evaluated at sh_degree along normalise(mean - campos of the view) inside the
 * projection kernel, as pixie_sh_to_rgb does without a rotation.
 * Outputs, each NULL or given, at least one of the two images: d_out_color [views][3][height][width]; d_out_rgb8
 * [views][height][width][3] = rintf(fminf(fmaxf(255 c, 0), 255)) of the same pixel; d_radii [views][n]; d_final_T and d_n_contrib
 * [views][height][width].  d_workspace: 16-byte aligned, workspace_bytes >= pixie_raster_batch_workspace_bytes(n, views, width,
 * height, max_instances); max_instances is the instance capacity one sort may use. */
typedef struct pixie_raster_view {
    float viewmatrix[16], projmatrix[16], campos[3];
    float tanfovx, tanfovy;
} pixie_raster_view;
typedef struct pixie_raster_batch_desc {
    int32_t views, n_dyn, n_static, width, height;
    int32_t sh_degree, k_coeffs;       /* read with d_shs only */
    float scale_modifier;
    float bg[3];
    int32_t pad_;
    const pixie_raster_view* view;     /* HOST array [views] */
    const float* d_means;              /* [views][n_dyn][3] */
    const float* d_cov3d;              /* [views][n_dyn][6] */
    int64_t means_view_stride, cov3d_view_stride;
    const float* d_static_means;       /* [n_static][3] */
    const float* d_static_cov3d;       /* [n_static][6] */
    const float* d_opacity;            /* [n] */
    const float* d_colors;             /* [views or 1][n][3], or NULL */
    int64_t colors_view_stride;
    const float* d_shs;                /* [n][k_coeffs][3], or NULL */
    float* d_out_color;                /* or NULL */
    uint8_t* d_out_rgb8;               /* or NULL */
    int32_t* d_radii;                  /* or NULL */
    float* d_final_T;                  /* or NULL */
    int32_t* d_n_contrib;              /* or NULL */
    void* d_workspace;
    int64_t workspace_bytes;
    int64_t max_instances;
} pixie_raster_batch_desc;
/* Bytes of workspace for a batch of `views` renders of n Gaussians: the part sized by views * n, plus the sort storage of the
 * largest group of views, max_instances instances.  -1 on error. */
int64_t pixie_raster_batch_workspace_bytes(int n, int views, int width, int height, int64_t max_instances);
/* Projects all views * n Gaussian-views in one launch, scans their tile counts in one scan, synchronises `stream` ONCE to read the
 * views + 1 offsets at the view boundaries (instances_out[v], where not NULL, is view v's instance count; a batch with n == 0
 * synchronises never), then partitions the views greedily into groups of consecutive views whose instances fit max_instances
 * (*groups_out, where not NULL) and -- asynchronously, per group -- duplicates with keys ((view in group * tiles + tile) << 32 |
 * depth bits), sorts once, finds the (view, tile) ranges and renders on a (tiles_x, tiles_y, views in group) grid.  Within a
 * (view, tile) run the instances are in (depth, index) order as in pixie_raster_forward, and the blend is the same code, so every
 * image has the bits that call gives for that view.  If one view alone exceeds max_instances the call returns non-zero: d_radii and
 * instances_out are written, no image output is touched, and pixie_last_error() names the view and the count it needs. */
int pixie_raster_forward_batch(const pixie_raster_batch_desc* desc, int64_t* instances_out, int32_t* groups_out, void* stream);

/* ======================================================================================
 * (D') Backward pass of the rasteriser: the gradient of one pixie_raster_forward render with respect to its inputs.
 * ====================================================================================== */
/* The gradient is the exact derivative of the forward as section (D) defines it, with every discrete decision held fixed: culling,
 * radius, tile rectangle, order, the power > 0 / 1/255 / 1e-4 rules, and min(0.99, .), the 1.3 tanfov clamp of the projection and the
 * max(., 0) of the colour each taking the branch they took.  Camera matrices get no gradient.
 * `forward` is the descriptor of the forward call as it was passed, with d_final_T and d_n_contrib given, its outputs (d_out_color,
 * d_radii, d_n_contrib) as that call wrote them and its workspace untouched since; `instances` is the count that call returned.
 * With d_shs ([n][sh_k][3]) the colours forward.d_colors are taken to be pixie_sh_to_rgb(d_shs, sh_degree, d_means, campos) without
 * a rotation, and the colour gradient is carried on to d_dL_dshs and, through the view direction, to d_dL_dmeans3D.
 * d_dL_dcolor is [3][height][width].  Outputs, each NULL (not computed) or given: d_dL_dmeans3D [n][3]; d_dL_dmeans2D [n][3] =
 * (dL/dpx 0.5 width, dL/dpy 0.5 height, 0) for the pixel centre (px, py), the convention of diff_gaussian_rasterization;
 * d_dL_dopacity [n]; d_dL_dcolors [n][3]; d_dL_dshs [n][sh_k][3] (needs d_shs); d_dL_dcov3D [n][6], one value per upper-triangle
 * entry, when the forward took d_cov3d, or d_dL_dscales [n][3] and d_dL_drotations [n][4] when it took the pair.  Culled Gaussians
 * (radius 0) get exact zeros.  d_grad_workspace: 16-byte aligned, grad_workspace_bytes >= pixie_raster_backward_workspace_bytes. */
typedef struct pixie_raster_backward_desc {
    pixie_raster_desc forward;
    int64_t instances;
    const float* d_shs;                /* [n][sh_k][3], or NULL */
    int32_t sh_k, sh_degree;           /* read with d_shs only */
    float campos[3];                   /* read with d_shs only */
    int32_t pad_;
    const float* d_dL_dcolor;          /* [3][height][width] */
    float* d_dL_dmeans3D;
    float* d_dL_dmeans2D;
    float* d_dL_dopacity;
    float* d_dL_dcolors;
    float* d_dL_dshs;
    float* d_dL_dcov3D;
    float* d_dL_dscales;
    float* d_dL_drotations;
    void* d_grad_workspace;
    int64_t grad_workspace_bytes;
} pixie_raster_backward_desc;
/* Bytes of the gradient workspace: nine floats per instance (one slot per Gaussian and tile of its rectangle).  -1 on error. */
int64_t pixie_raster_backward_workspace_bytes(int n, int width, int height, int64_t instances);
/* Asynchronous on `stream`, no synchronise.  Zeroes the per-instance buffer, walks every tile front to back up to its largest
 * n_contrib, reducing each Gaussian's nine partials (centre 2, conic 3, opacity 1, colour 3) over the tile in a fixed order into its
 * slot, then sums each Gaussian's slots sequentially and applies the per-Gaussian chain.  No floating-point atomics: the gradients
 * are bit-identical from run to run.  n == 0 or zero instances zeroes the outputs and launches nothing else; with every output NULL
 * the call checks its arguments and does nothing. */
int pixie_raster_backward(const pixie_raster_backward_desc* desc, void* stream);

/* ======================================================================================
 * (E) Scene ingest -- PG/gs_simulation.py:403-438: everything between GaussianModel.load_ply and fill_particles.
 * ====================================================================================== */
/* d_block is the body of the checkpoint PLY as it lies in the file: [n][n_attr] float32, row-major, 16-byte aligned, n_attr <= 254.
 * `columns` is a HOST table of 11 + 3 K entries, K = (sh_degree + 1)^2, naming the column of x, y, z, opacity, scale_0..2,
 * rot_0..3, f_dc_0..2, f_rest_0..3(K-1)-1, in that order; every entry lies in [0, n_attr).  `rotations` holds n_rotations (<= 8)
 * row-major 3x3 matrices applied in order (p @ R^T, R S R^T); sim_area = (x0, x1, y0, y1, z0, z1) on the rotated position, strict,
 * read when has_sim_area.  A Gaussian is dropped unless sigmoid(opacity) > opacity_threshold, selected if inside sim_area (or there
 * is none), unselected otherwise.
 * Outputs, n rows of room each: selected Gaussians, in file order, fill rows [0, n_sel); unselected ones, in file order, rows
 * [n_sel, n_sel + n_unsel).  d_pos [.][3]: selected = ((rotated - mean) * scale + 1) + (0, 0, z_shift), unselected = the file's
 * x y z.  d_cov [.][6] (00 01 02 11 12 22): the covariance of exp(scale) and the normalised quaternion; selected rows rotated and
 * times scale^2.  d_opacity [.][1]: sigmoid.  d_shs [.][K][3]: the file's f_dc | f_rest columns, (channel, coefficient) ->
 * (coefficient, channel).  mean = (min + max) / 2 and scale = 1 / max(max - min) over the selected rotated positions, float32. */
typedef struct pixie_ingest_desc {
    int64_t n;
    int32_t n_attr, sh_degree, n_rotations, has_sim_area;
    float rotations[72];
    float sim_area[6];
    float opacity_threshold, z_shift;
    const float* d_block;
    const int32_t* columns;            /* HOST array [11 + 3 K] */
    float* d_pos;
    float* d_cov;
    float* d_opacity;
    float* d_shs;
    void* d_workspace;
    int64_t workspace_bytes;
} pixie_ingest_desc;
/* What pixie_scene_ingest returns besides 0 and 1 (any other error): each leaves pixie_last_error() set and the outputs unwritten. */
enum {
    PIXIE_INGEST_NO_SELECTION = 2,       /* no Gaussian passes the opacity filter inside sim_area */
    PIXIE_INGEST_ZERO_EXTENT = 3,        /* max(max - min) == 0, one selected Gaussian included: 1 / 0 is no scale */
    PIXIE_INGEST_TOO_MANY_ROTATIONS = 4, /* n_rotations > 8 */
    PIXIE_INGEST_TOO_MANY_ROWS = 5       /* n > 2^31 - 2 */
};
/* Bytes of 16-byte aligned device workspace for n Gaussians (two 8-byte words per Gaussian and the scan's storage).  -1 on error. */
int64_t pixie_scene_ingest_workspace_bytes(int64_t n);
/* Classifies every Gaussian, bounds the selected ones, scans, synchronises `stream` ONCE to read counts_out (selected, unselected,
 * dropped), scale_out and mean_out (each NULL or given), then -- asynchronously, in one launch -- writes the four outputs.  On
 * PIXIE_INGEST_NO_SELECTION and PIXIE_INGEST_ZERO_EXTENT the counts are written and nothing is launched after the synchronise.
 * Deterministic: the same input gives the same bits. */
int pixie_scene_ingest(const pixie_ingest_desc* desc, int64_t counts_out[3], float scale_out[1], float mean_out[3], void* stream);

/* ---- 3DGS training natives: what gaussian-splatting/train.py needs beside its rasteriser ---- */

/* distCUDA2 of simple-knn (scene/gaussian_model.py:20, :134): d_out[i] = ((b0 + b1) + b2) / 3 with b0 <= b1 <= b2 the three
 * smallest ((dx dx + dy dy) + dz dz) over all OTHER points j != i (by index: a coincident point counts at distance 0), float32,
 * no fused multiply-add.  A missing neighbour counts as FLT_MAX, as in the reference: one or two points give +inf, three give
 * FLT_MAX / 3.  The search is exact, so the result is bit-equal to a float32 brute force in that expression order, bit-identical
 * from run to run and independent of the order of the rows.  The coordinates must be finite; a NaN gives unspecified values for
 * the affected points and nothing worse.  d_points [n][3], d_out [n]: caller-owned device memory; d_scratch: 16-byte aligned,
 * pixie_knn_mean_dist2_scratch_bytes(n) bytes (-1 for n outside [0, 2^24]).  n above 2^24 and a scratch buffer that is too small
 * are refused before anything is launched; n = 0 launches nothing.  Asynchronous on `stream`. */
int64_t pixie_knn_mean_dist2_scratch_bytes(int64_t n);
int pixie_knn_mean_dist2(const float* d_points, int64_t n, void* d_scratch, int64_t scratch_bytes, float* d_out, void* stream);

/* l1_loss and ssim of utils/loss_utils.py (window 11, sigma 1.5, zero padding 5, one window per channel, C1 = 1e-4, C2 = 9e-4) of
 * d_img against d_gt, both [b][c][h][w] float32, as per-image means d_out_l1[b] and d_out_ssim[b]: one fused launch and a
 * one-workgroup-per-image finalise, no floating-point atomics (bit-identical from run to run), no synchronise.  The window is
 * applied separably.  With with_grad != 0 the forward also leaves three planes in the workspace, from which
 * pixie_photometric_backward writes d_grad_img = sum over the image's two means of g * d mean / d d_img in one launch
 * (d_g_l1[b], d_g_ssim[b]: the upstream gradients of the means; sign(0) = 0 in the L1 term).  d_workspace: 16-byte aligned,
 * pixie_photometric_workspace_bytes(...) bytes for the same sizes and with_grad (-1 on error), untouched between the forward and
 * its backward.  h, w <= 32768 and b * c <= 65535. */
int64_t pixie_photometric_workspace_bytes(int b, int c, int h, int w, int with_grad);
int pixie_photometric_forward(const float* d_img, const float* d_gt, int b, int c, int h, int w, void* d_workspace,
                              int64_t workspace_bytes, int with_grad, float* d_out_l1, float* d_out_ssim, void* stream);
int pixie_photometric_backward(const float* d_img, const float* d_gt, int b, int c, int h, int w, const void* d_workspace,
                               const float* d_g_l1, const float* d_g_ssim, float* d_grad_img, void* stream);

/* ---- 3DGS training natives: what train.py does with the gradients (optimiser step, densification) ---- */

/* torch.optim.Adam (no weight decay, no amsgrad, not maximize) over up to 8 one-tensor groups in ONE launch.  Per element, in
 * float32 and in this order (no fused multiply-add), the scalars rounded from double: m = m + (1 - beta1) (g - m); v = v beta2 + ((1 - beta2) g) g;
 * p = p - step_size (m / (sqrt(v) / bias_correction2_sqrt + eps)).  The caller computes step_size = lr / (1 - beta1^t) and
 * bias_correction2_sqrt = sqrt(1 - beta2^t) in double and rounds once.  param, exp_avg and exp_avg_sq are updated in place; all
 * four arrays hold `count` floats of caller-owned device memory.  count == 0 is legal (its pointers are not read).  Every element
 * is updated (dense semantics).  No atomics, no synchronise: bit-identical from run to run. */
typedef struct pixie_gs_adam_group {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;
    float step_size, bias_correction2_sqrt;
} pixie_gs_adam_group;
typedef struct pixie_gs_adam_desc {
    double beta1, beta2, eps;          /* as Python holds them: 1 - beta is taken in double and rounded once, as torch does */
    int32_t n_groups;                  /* 0..8 */
    int32_t pad_;
    pixie_gs_adam_group group[8];
} pixie_gs_adam_desc;
int pixie_gs_adam_step(const pixie_gs_adam_desc* desc, void* stream);

/* train.py:114-116 in one launch, no synchronise: for every i < n with d_radii[i] > 0, d_max_radii2D[i] = max(d_max_radii2D[i],
 * d_radii[i]); d_xyz_gradient_accum[i] += sqrt(gx gx + gy gy) of d_viewspace_grad [n][3]; d_denom[i] += 1. */
int pixie_gs_densify_stats(const int32_t* d_radii, const float* d_viewspace_grad, int64_t n, float* d_max_radii2D,
                           float* d_xyz_gradient_accum, float* d_denom, void* stream);

/* scene/gaussian_model.py:densify_and_prune (:393-405) as plan + emit.  Fields are indexed xyz 0, f_dc 1, f_rest 2, opacity 3,
 * scaling 4, rotation 5; a row of them holds 3, 3, n_rest, 1, 3, 4 floats (n_rest = 3 ((sh_degree + 1)^2 - 1), 0 allowed).
 * A Gaussian with g = accum / denom (NaN -> 0) >= max_grad is cloned if max(exp(scaling)) <= float(percent_dense * extent) and
 * split in two otherwise.  Every row of the result -- originals, clones, children on their new scaling -- is then pruned if
 * sigmoid(opacity) < min_opacity or, with has_max_screen_size, max(exp(scaling)) > float(0.1 * extent).  (The reference's third
 * term, max_radii2D > max_screen_size, reads an array that densification_postfix has just zeroed: it never fires and is not
 * evaluated.)  Output rows, each group in source order: surviving originals that were not split, surviving clones, surviving first
 * children, surviving second children.  d_exp_avg / d_exp_avg_sq entries may be NULL (no optimiser state yet: zeros). */
typedef struct pixie_gs_densify_desc {
    int64_t n;
    int32_t n_rest, has_max_screen_size;
    double max_grad, min_opacity, extent, percent_dense;
    const float* d_xyz_gradient_accum;     /* [n] */
    const float* d_denom;                  /* [n] */
    const float* d_param[6];
    const float* d_exp_avg[6];
    const float* d_exp_avg_sq[6];
    void* d_workspace;                     /* 16-byte aligned, pixie_gs_densify_workspace_bytes(n) bytes, kept from plan to emit */
    int64_t workspace_bytes;
} pixie_gs_densify_desc;
/* n_out rows of room in every output; d_noise: standard-normal [2 n_split][3], row copy * n_split + (rank among the split). */
typedef struct pixie_gs_densify_outs {
    int64_t n_out, n_split;                /* as pixie_gs_densify_plan reported them */
    const float* d_noise;
    float* d_param[6];
    float* d_exp_avg[6];
    float* d_exp_avg_sq[6];
    int32_t* d_source_index;               /* [n_out]: the input row each output row came from */
    float* d_xyz_gradient_accum;           /* [n_out], zero-filled, as d_denom and d_max_radii2D */
    float* d_denom;
    float* d_max_radii2D;
} pixie_gs_densify_outs;
enum {
    PIXIE_GS_DENSIFY_BAD_MAX_GRAD = 2,     /* max_grad <= 0 (or NaN): the reference would split its own clones */
    PIXIE_GS_DENSIFY_TOO_MANY_ROWS = 3,    /* n > 2^31 - 2 */
    PIXIE_GS_DENSIFY_EMPTY = 4             /* n == 0 */
};
int64_t pixie_gs_densify_workspace_bytes(int64_t n);
/* Classifies, scans and synchronises `stream` ONCE.  counts_out = (surviving originals, clones kept, split children kept, rows the
 * final prune removed); their first three sum to the output's row count.  n_split_out = Gaussians split (kept or not): the caller
 * draws 2 n_split rows of noise and allocates the outputs between this call and pixie_gs_densify_emit. */
int pixie_gs_densify_plan(const pixie_gs_densify_desc* desc, int64_t counts_out[4], int64_t n_split_out[1], void* stream);
/* One launch, asynchronous.  Survivors keep their moments, new rows get zeros; clones are bit copies; children copy rotation, f_dc,
 * f_rest and opacity and get scaling = log(exp(scaling) / 1.6), xyz = R(q / |q|) (exp(scaling) * z) + xyz.  outs->n_out and
 * outs->n_split bound every write and every noise read: a wrong value loses rows, it cannot write outside the outputs. */
int pixie_gs_densify_emit(const pixie_gs_densify_desc* desc, const pixie_gs_densify_outs* outs, void* stream);

/* ======================================================================================
 * (E) Occupancy mask -- the stage between the voxel files and the networks: pixie/voxel/voxelize.py:188-263
 *     _create_occupancy_mask (and the same filters in compute_occupancy_point_cloud :331-400, with
 *     f3rm_robot/optimize.py:44-89 remove_floating_clusters).  Open3D's remove_statistical_outlier and cluster_dbscan
 *     are restated on the voxel lattice from their published algorithm.
 * ====================================================================================== */
typedef struct pixie_occupancy_desc {
    const void* d_alphas;       /* (D, H, W) densities, float16 or float32 (a trailing axis of 1 is the same memory) */
    const void* d_rgb;          /* (D, H, W, 3) colours, same dtype */
    const float* d_axis_x; const float* d_axis_y; const float* d_axis_z;  /* voxel coordinates, D / H / W float32 each, as pixie_field_desc;
                                   the three spacings must agree up to rounding (the reference: arange(min, max, voxel_size) per axis) */
    double* d_stats;            /* NULL or device double[3]: cloud_mean, std, cloud_mean + std_ratio std of stage B */
    int32_t dtype;              /* 0 = float16, 1 = float32 */
    int32_t d, h, w;            /* the grid need not be cubic */
    int32_t run_filters;        /* 0: stage A alone (voxelize.py:252-253) */
    int32_t nb_neighbors;       /* stage B, >= 1 */
    int32_t min_points;         /* stage C, >= 1 */
    int32_t keep;               /* stage C: 0 = every voxel of a cluster (voxelize.py:250), 1 = the largest cluster, first maximum;
                                   everything if there is no cluster (optimize.py:44-89) */
    double voxel_size;          /* eps = voxel_size * eps_multiplier, the product taken in double */
    double lattice_spacing;     /* spacing of the axes (need not equal voxel_size: compute_occupancy_point_cloud clusters a
                                   linspace lattice with eps = 5 * 0.01); sizes the index neighbourhood that is searched, nothing else */
    double alpha_threshold, gray_threshold;  /* rounded to float32 before the comparison, as torch compares a float32 tensor with a scalar */
    double std_ratio;
    double eps_multiplier;      /* > 0; eps / lattice_spacing < 30 */
} pixie_occupancy_desc;
/* Stage A: a voxel is a candidate iff float32(alpha) > alpha_threshold and ((r + g) + b) / 3 > gray_threshold in float32.
 * Stage B (Open3D RemoveStatisticalOutliers): m_i = mean Euclidean distance of candidate i to its k' = min(nb_neighbors, M)
 * nearest candidates, itself included at distance 0, in float64 on the float32 coordinates; the nearest are whole shells of
 * integer squared offset, ties inside the last shell in a fixed order.  cloud_mean = sum m_i / M and std = sqrt(sum (m_i -
 * cloud_mean)^2 / (M - 1)) by two fixed-order float64 reductions; voxel i survives iff m_i > 0 && m_i < cloud_mean + std_ratio std
 * (M = 1 and M = 2 keep nothing; M = 0 gives an empty mask and is no error).
 * Stage C (Open3D ClusterDBSCAN on the survivors): neighbours are the survivors with ((dx dx + dy dy) + dz dz) < eps eps in float64
 * on differences of the float32 coordinates -- STRICT, unlike the closed ball of pixie_dbscan_roots; a voxel is core when its open
 * ball holds >= min_points survivors, itself included; clusters are the components of the core voxels, numbered by ascending
 * lowest core index in C order; a border voxel joins the lowest-numbered cluster with a core voxel in reach; the rest is noise.
 * d_mask [D][H][W] receives 0 / 1.  d_mean_dist: NULL or [D][H][W] doubles, m_i for candidates and NaN elsewhere (not written when
 * run_filters == 0, nor is d_stats).  d_counts: device int64[8] = candidates after the density threshold, after the gray
 * threshold (M), after stage B, after stage C (= voxels set in d_mask), voxels that left stage B's fast path, number of clusters,
 * two reserved zeros.  d_scratch: 16-byte aligned, pixie_occupancy_scratch_bytes(desc, with_mean_dist) bytes (-1 on a bad descriptor;
 * only d, h, w are read); with_mean_dist != 0 says that the call will be given a d_mean_dist, which saves the 8 D H W bytes of the call's own.  Null pointers, nb_neighbors < 1, min_points < 1, eps_multiplier <= 0, a dimension < 1 and more than 2^31 voxels are
 * refused before any launch.  No stream synchronise, no host read-back, no floating-point atomics: asynchronous on `stream` and
 * bit-identical from run to run. */
int64_t pixie_occupancy_scratch_bytes(const pixie_occupancy_desc* desc, int with_mean_dist);
int pixie_occupancy_mask(const pixie_occupancy_desc* desc, uint8_t* d_mask, double* d_mean_dist, int64_t* d_counts, void* d_scratch,
                         void* stream);

/* ======================================================================================
 * (F) Language-query part segmentation -- material_mode=vlm, pixie/voxel/segmentation.py: run_clip and
 *     clip_part_segmentation (:98-168), local_post_process_segmentation (:190-226, sklearn KDTree + scipy.stats.mode in
 *     a Python loop) and the material grid of save_segmented_point_cloud (:429-452).
 * ====================================================================================== */
#define PIXIE_PART_SEG_COUNTS 40
typedef struct pixie_part_seg_desc {
    const void* d_features;     /* (D, H, W, C) float16, the layout voxelize.py writes; 16-byte aligned */
    const uint8_t* d_mask;      /* (D, H, W), != 0 = a masked voxel */
    const float* d_queries;     /* (K, C) float32 text embeddings, not normalised */
    const float* d_props;       /* NULL or (K, 4) float32: density, E, nu, material_id per part */
    int32_t d, h, w;            /* the grid need not be cubic */
    int32_t channels;           /* C: a multiple of 8, <= 2048 */
    int32_t n_parts;            /* K: 1 .. 32, and K C 4 <= 96 KB (the queries are staged in LDS) */
    int32_t vote_k;             /* 0: no vote; 1 .. 255: neighbours of the k-nearest-neighbour vote */
    float temperature;          /* softmax temperature T > 0 (the reference: 0.1) */
    float background_id;        /* material id of the rows outside the mask (the reference: 7) */
} pixie_part_seg_desc;
/* Stage A, every masked voxel: sim_j = <f, q_j> / (|f| |q_j|) in float32 on the widened row, d_labels = argmax_j sim_j (first
 * maximum), d_scores = 1 / sum_j exp((sim_j - sim_max) / T), i.e. softmax(sim / T)[label]; a row of zero norm gets label 0 and
 * score NaN.  Outside the mask d_labels = -1 and d_scores = NaN.  d_counts: device int64[PIXIE_PART_SEG_COUNTS] = voxels per part
 * (stage A labels, 32 slots), masked voxels, voxels that left the vote's fast path, reserved zeros.
 * Stage B (vote_k > 0), every masked voxel: d_voted [D][H][W] = the most frequent stage-A label among its k' = min(vote_k, masked
 * voxels) nearest masked voxels, itself included, neighbours ordered by (integer squared index offset, C-order index), equal
 * counts to the smallest label; -1 outside the mask.  d_voted must be NULL iff vote_k == 0.
 * d_material (iff d_props): [D][H][W][4] float32, d_props[label] (the voted label if stage B ran) on the mask and
 * [0, 0, 0, background_id] elsewhere; 16-byte aligned.
 * d_scratch: 16-byte aligned, pixie_part_seg_scratch_bytes(desc) bytes (-1 on a bad descriptor; the pointers are not read).
 * Shapes outside the limits above are refused before any launch.  No stream synchronise, no host read-back, no floating-point
 * atomics: asynchronous on `stream` and bit-identical from run to run. */
int64_t pixie_part_seg_scratch_bytes(const pixie_part_seg_desc* desc);
int pixie_part_segmentation(const pixie_part_seg_desc* desc, int8_t* d_labels, float* d_scores, int8_t* d_voted, float* d_material,
                            int64_t* d_counts, void* d_scratch, void* stream);
/* The material fill alone, for labels that exist already: labels outside [0, n_parts) give the background row. */
int pixie_part_material_grid(const int8_t* d_labels, const float* d_props, int n_parts, int64_t n_voxels, float background_id,
                             float* d_material, void* stream);

/* ======================================================================================
 * (G) NeRF feature-field query -- pixie/voxel/voxelize.py: extract_clip_voxel_grid (:17-141) through
 *     f3rm_robot/field_adapter.py (:28-72): multiresolution hash grids (+ frequency block, + extra input columns) feeding
 *     64-wide ReLU MLPs, the networks the reference evaluates with tiny-cuda-nn.
 * ====================================================================================== */
#define PIXIE_HASHMLP_MAX_LEVELS 16
#define PIXIE_HASHMLP_MAX_LAYERS 5      /* up to 4 hidden layers + the output layer */
#define PIXIE_HASHMLP_MAX_INPUT 160     /* widest input row: levels * features + 6 * frequencies + extra columns */
#define PIXIE_HASHMLP_MAX_OUTPUT 1024
/* One level of a grid.  For a unit-cube position p: q = p * scale + shift (float32, unfused), c0 = floor(q), w = q - c0, corners
 * c0 + {0,1}^3 with trilinear weights from w; corner (x, y, z) reads table row
 *   (dense ? x + y res + z res^2 : x ^ y 2654435761 ^ z 805459861) [uint32] % size + offset. */
typedef struct pixie_hashgrid_level {
    float scale, shift;
    uint32_t res, size, offset, dense;
} pixie_hashgrid_level;
typedef struct pixie_hashmlp_desc {
    int32_t n_levels;              /* 0 .. 16 (0: the input row is the extra columns alone) */
    int32_t features_per_level;    /* 2, 4 or 8 */
    int32_t n_frequencies;         /* 0 = no frequency block, else 1 .. 8: 6 n columns after the grid columns, tiny-cuda-nn's order:
                                    * column j has dim j / (2 n), octave (j / 2) % n, value sin(2^octave pi x + (j % 2) pi / 2) */
    int32_t n_extra;               /* float32 input columns appended last, read from d_extra */
    int32_t n_hidden;              /* 1 .. 4 hidden layers, each 64 wide, ReLU */
    int32_t out_dim;               /* 1 .. 1024 */
    int32_t out_activation;        /* 0 none, 1 sigmoid, 2 exp */
    int32_t pad_;
    pixie_hashgrid_level level[PIXIE_HASHMLP_MAX_LEVELS];
    const float* d_table;          /* (table_rows, features_per_level) float32, 16-byte aligned */
    int64_t table_rows;            /* every level's offset + size <= table_rows */
    const float* d_weight[PIXIE_HASHMLP_MAX_LAYERS];   /* layer i of n_hidden + 1: (out_i, in_i) row-major float32 */
    const float* d_bias[PIXIE_HASHMLP_MAX_LAYERS];     /* NULL (no bias) or (out_i) float32 */
} pixie_hashmlp_desc;
/* d_out (n, out_dim) float32 = act(MLP(row)) with row = [grid columns | frequency columns | d_extra (n, n_extra)] of the unit-cube
 * positions d_positions (n, 3) float32 (NULL allowed iff n_levels == 0 and n_frequencies == 0; d_extra NULL iff n_extra == 0).
 * float32 throughout, the layers on the float32 matrix instructions; the input row and the hidden activations stay on chip.
 * Anything outside the limits above (or an input row wider than PIXIE_HASHMLP_MAX_INPUT) is refused before any launch.
 * Asynchronous on `stream`, bit-identical from run to run. */
int pixie_hashmlp_forward(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, float* d_out,
                          void* stream);

/* ---- training: the same network with gradients (pixie_amd/csrc/field_query_backward.hip) ----
 * pixie_hashmlp_forward_saved is pixie_hashmlp_forward (the same bits in d_out) and also fills d_saved with what the backward reads,
 * channel-major float32: the input row [in_dim][n], then the post-ReLU activations of hidden layer k as [64][n], k = 0.. n_hidden - 1:
 *     saved_bytes = 4 n (in_dim + 64 n_hidden),  in_dim = n_levels features_per_level + 6 n_frequencies + n_extra.
 * pixie_hashmlp_backward takes the forward's inputs, its d_out, d_saved and d_dout = dL/d_out (n, out_dim) and WRITES (does not
 * accumulate) every gradient whose pointer is not NULL.  Positions get no gradient.  d_scratch, 256-byte aligned, of scratch_bytes:
 *     [0, 256)     header: uint32 bits of M = max |dX_grid|, int32 shift s the call used, int32 state (0 scattered, 1 M == 0, 2 M not finite)
 *     then, each rounded up to 256 bytes: dZ of the hidden layers 4 (64 n_hidden n) | dX of the grid columns 4 (n_levels F n) |
 *     weight-gradient slab partials 4 max_layers(slabs (out in + out)) | the table's accumulators 8 table_rows F,
 *     slabs(layer) = clamp(1024 / (ceil(out / 64) ceil(in / 64)), 1, min(ceil(n / 64), 256)).
 * The table gradient is a 64-bit fixed-point integer scatter (csrc/hashgrid_grad_math.h): bit-identical from run to run and under any
 * permutation of the points; weight and bias gradients sum fixed slabs of points in slab order: bit-identical from run to run.
 * M == 0 gives a zero table gradient; M not finite (an Inf or NaN in d_dout) fills the WHOLE table gradient with NaN.
 * Refusals are the forward's, and n > 2^24.  Asynchronous on `stream`: no synchronise, no host read-back. */
typedef struct pixie_hashmlp_grads {      /* any pointer may be NULL: that gradient is not computed */
    float* d_table;                        /* (table_rows, F) */
    float* d_weight[PIXIE_HASHMLP_MAX_LAYERS];
    float* d_bias[PIXIE_HASHMLP_MAX_LAYERS];
    float* d_extra;                        /* (n, n_extra) */
} pixie_hashmlp_grads;
int pixie_hashmlp_train_bytes(const pixie_hashmlp_desc* desc, int64_t n, int64_t* saved_bytes, int64_t* scratch_bytes);
int pixie_hashmlp_forward_saved(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, float* d_out,
                                void* d_saved, void* stream);
int pixie_hashmlp_backward(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, const float* d_out,
                           const void* d_saved, const float* d_dout, const pixie_hashmlp_grads* grads, void* d_scratch, void* stream);

/* ---- proposal density field: hash grid -> 16-wide MLP -> trunc_exp, fused (pixie_amd/csrc/density_field.hip) ----
 * nerfstudio's HashMLPDensityField.get_density (fields/density_fields.py:94-117), from nerf-frame sample positions to densities, in
 * one launch; what ProposalNetworkSampler calls once per proposal level.  Per point, float32, unfused up to the cell (hashgrid_math.h):
 *     p = world_to_nerf x (if given);  contraction ? L-infinity contraction then (p + 2) / 4 : (p - aabb_lo) / (aabb_hi - aabb_lo)
 *     selector = all of 0 < p < 1;  the grid sees p * selector;  per level the trilinear blend of 8 table rows
 *     z_j = fmaf chain over the inputs in index order from b_j (or 0), ReLU, hidden width exactly 16, n_hidden hidden layers
 *     density = average_init_density * exp(h) * selector
 * A point whose selector is 0 (on or outside a face, p exactly 0, any NaN coordinate) gets density exactly 0, contributes nothing to any
 * gradient and issues no table atomic; its d_raw is the network's output at p = 0. */
#define PIXIE_DENSITY_FIELD_WIDTH 16
#define PIXIE_DENSITY_FIELD_MAX_LAYERS 3     /* up to 2 hidden layers + the output layer */
#define PIXIE_DENSITY_FIELD_MAX_INPUT 64     /* n_levels * features_per_level */
typedef struct pixie_density_field_desc {
    int32_t n_levels;              /* 1 .. 16 */
    int32_t features_per_level;    /* 2, 4 or 8 */
    int32_t n_hidden;              /* 0 (one linear layer: the reference's use_linear), 1 or 2 */
    int32_t hidden_width;          /* must be 16 */
    int32_t contraction;           /* 1: L-infinity scene contraction, then (p + 2) / 4;  0: the aabb */
    float average_init_density;
    pixie_hashgrid_level level[PIXIE_HASHMLP_MAX_LEVELS];
    const float* d_table;          /* (table_rows, features_per_level) float32, 16-byte aligned */
    int64_t table_rows;
    const float* d_weight[PIXIE_DENSITY_FIELD_MAX_LAYERS];   /* layer i of n_hidden + 1: (out_i, in_i) row-major float32 */
    const float* d_bias[PIXIE_DENSITY_FIELD_MAX_LAYERS];     /* NULL (no bias) or (out_i) float32 */
    const float* d_world_to_nerf;  /* NULL (identity) or 12 float32 on the device: 3 x 4 row-major */
    float aabb[6];                 /* lo[3], hi[3]; read when contraction == 0, hi > lo */
} pixie_density_field_desc;
typedef struct pixie_density_field_grads {   /* any pointer may be NULL: that gradient is not wanted */
    float* d_table;                           /* (table_rows, F) */
    float* d_weight[PIXIE_DENSITY_FIELD_MAX_LAYERS];
    float* d_bias[PIXIE_DENSITY_FIELD_MAX_LAYERS];
} pixie_density_field_grads;
/* saved_bytes is 0: the backward recomputes the forward from the positions.  scratch_bytes, for a 256-byte aligned d_scratch:
 *     [0, 256)     header: uint32 bits of M = max |dX_grid|, int32 shift s, int32 state (0 scattered, 1 M == 0, 2 M not finite)
 *     then, each rounded up to 256 bytes: masked unit positions 4 (3 n) | dX of the grid columns 4 (in_dim n) |
 *     slab partials 4 slabs params | the table's accumulators 8 table_rows F,
 *     slabs = clamp(ceil(n / 256), 1, 1024), params = every weight and bias of the network (csrc/density_field_math.h). */
int pixie_density_field_train_bytes(const pixie_density_field_desc* desc, int64_t n, int64_t* saved_bytes, int64_t* scratch_bytes);
/* d_positions (n, 3) float32 -> d_density (n) float32 and, unless NULL, d_raw (n) = h.  One launch; nothing is saved for the backward.
 * Bit-identical from run to run, for a point alone or inside a batch, and under a permutation of the points. */
int pixie_density_field_forward(const pixie_density_field_desc* desc, const float* d_positions, int64_t n, float* d_density, float* d_raw,
                                void* stream);
/* d_ddensity (n) = dL/d density.  WRITES (does not accumulate) every gradient whose pointer is not NULL; positions get no gradient.
 * The table gradient is the 64-bit fixed-point scatter of csrc/hashgrid_grad_math.h: bit-identical from run to run and under a
 * permutation; a non-finite dX makes the WHOLE table gradient NaN.  Weight and bias gradients: one partial per slab, summed in slab
 * order: bit-identical from run to run.  No floating-point atomics.  Refusals: the limits above, n > 2^24.  Asynchronous on `stream`. */
int pixie_density_field_backward(const pixie_density_field_desc* desc, const float* d_positions, int64_t n, const float* d_ddensity,
                                 const pixie_density_field_grads* grads, void* d_scratch, void* stream);

typedef struct pixie_field_voxelize_desc {
    pixie_hashmlp_desc density;    /* out_dim = 1 + G <= 63, out_activation 0: column 0 the log density, columns 1.. the geometry
                                    * features (nerfacto_field.py:203-232) */
    pixie_hashmlp_desc color;      /* n_levels 0, n_frequencies 0, n_extra = G, out_dim 3, sigmoid: the colour head with the constant
                                    * direction and appearance inputs folded into its first bias by the caller */
    pixie_hashmlp_desc feature;    /* out_dim C, out_activation 0 (f3rm/feature_field.py:94-113) */
    const float* d_axis_x;         /* all three NULL, or the voxel coordinates themselves: (D), (H), (W) float32 device arrays.  The */
    const float* d_axis_y;         /* reference's lattice is torch.arange(min, max, voxel_size) evaluated on the CPU, whose vectorised */
    const float* d_axis_z;         /* loop rounds differently from the formula below (and with the CPU's vector width) */
    double min_bounds[3];          /* without axes voxel (i, j, k) sits at float32(min_bounds + (i, j, k) * voxel_size) computed in double */
    double voxel_size;             /* also the delta of alpha = 1 - exp(-density * float32(voxel_size)) */
    int32_t d, h, w;
    int32_t contraction;           /* 1: L-infinity scene contraction, then (p + 2) / 4;  0: (p - aabb_lo) / (aabb_hi - aabb_lo) */
    int32_t alpha_weighted;        /* 1: features are multiplied by the float32 alpha before rounding to float16 */
    float average_init_density;
    float world_to_nerf[12];       /* 3 x 4 row-major: n_r = ((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3] */
    float aabb[6];                 /* lo[3], hi[3]; read when contraction == 0 */
} pixie_field_voxelize_desc;
/* d_features (D, H, W, C) float16, d_alpha (D, H, W, 1) float16, d_rgb (D, H, W, 3) float16, d_density NULL or (D, H, W) float32;
 * d_scratch (D, H, W) float32, which holds the float32 alpha afterwards.  The density net sees p * selector, selector = all of
 * 0 < p < 1, and density = average_init_density * exp(h_0) * selector; the feature net sees p itself.  Every float16 output is the
 * float32 value rounded to nearest even.  Two launches, no stream synchronise, no host read-back, no floating-point atomics:
 * asynchronous on `stream` and bit-identical from run to run. */
int pixie_field_voxelize(const pixie_field_voxelize_desc* vdesc, void* d_features, void* d_alpha, void* d_rgb, float* d_density,
                         float* d_scratch, void* stream);
/* The same kernels on n world points d_world (n, 3) float32 in place of the lattice (min_bounds, voxel_size, d, h, w and
 * alpha_weighted are not read), with float32 outputs, FeatureFieldAdapter's surface: d_features (n, C) the raw feature net output,
 * d_alpha (n) = 1 - exp(-density * float32(delta)), d_rgb (n, 3), d_density (n).  Any output may be NULL and is then not computed.
 * A point gets the bits the lattice call gives a voxel at the same float32 position, before the rounding to float16. */
int pixie_field_query_points(const pixie_field_voxelize_desc* vdesc, const float* d_world, int64_t n, double delta, float* d_features,
                             float* d_alpha, float* d_rgb, float* d_density, void* stream);

/* ---- differentiable ray compositing (pixie_amd/csrc/ray_render.hip) ----
 * What lies between a NeRF's per-sample outputs and its loss: RaySamples.get_weights, RGBRenderer.combine_rgb, AccumulationRenderer,
 * DepthRenderer (median and expected) and f3rm's FeatureRenderer, for unpacked samples, forward and backward.  All arrays are
 * float32, contiguous, on the device; R = n_rays, S = n_samples, C = n_channels.
 *     x_i = delta_i density_i,  w_i = nan_to_num((1 - exp(-x_i)) exp(-sum_{j<i} x_j)),  A = sum w_i,  m_i = (start_i + end_i) / 2
 *     rgb = sum w_i rgb_i + bg (1 - A),  expected depth = sum w_i m_i / (A + 1e-10) (NOT clipped: the clip is global over the batch
 *     and the caller's),  median depth = m_j for the first j whose running sum of w reaches 0.5 (S - 1 if none),  feature_c = sum w_i f_ic
 * Two modes.  Densities given (d_densities and d_deltas set, inputs.d_weights NULL in the forward): the weights are computed and
 * written to outputs.d_weights, which is required.  Weights given (d_densities NULL, inputs.d_weights set): the renderers alone;
 * outputs.d_weights must be NULL.  Any other output pointer may be NULL and is then not computed; an output needs its inputs
 * (depths: starts and ends; rgb: d_rgb; feature: d_features).
 * Limits: 1 <= R <= 2^24, 1 <= S <= 1024, C a multiple of 4 in [0, 2048], S <= 256 when C > 0; feature arrays 16-byte aligned.
 * Anything else is refused with a non-zero return before any launch.  Every sum has one fixed order: bit-identical from run to run,
 * under a permutation of the rays and for any R.  No floating-point atomics.  Asynchronous on `stream`: no synchronise, no host
 * read-back. */
typedef struct pixie_ray_desc {
    int64_t n_rays;
    int32_t n_samples;
    int32_t n_channels;            /* 0: no features */
    int32_t background;            /* 0 none ("random": nothing is added), 1 the constant bg, 2 the ray's last sample's rgb */
    float bg[3];
} pixie_ray_desc;
typedef struct pixie_ray_inputs {
    const float* d_densities;      /* (R, S) or NULL */
    const float* d_deltas;         /* (R, S), with d_densities */
    const float* d_weights;        /* (R, S): the given weights; in the backward of the density mode, the forward's outputs.d_weights */
    const float* d_starts;         /* (R, S) or NULL, with d_ends */
    const float* d_ends;
    const float* d_rgb;            /* (R, S, 3) or NULL */
    const float* d_features;       /* (R, S, C) or NULL */
} pixie_ray_inputs;
typedef struct pixie_ray_outputs {
    float* d_weights;              /* (R, S) */
    float* d_accumulation;         /* (R) */
    float* d_expected_depth;       /* (R) */
    float* d_median_depth;         /* (R) */
    float* d_rgb;                  /* (R, 3) */
    float* d_feature;              /* (R, C) */
} pixie_ray_outputs;
/* dL/d(output), same shapes; NULL = that output has no gradient.  The median depth has none. */
typedef struct pixie_ray_upstream {
    const float* d_weights;        /* density mode only: the weights are an output there */
    const float* d_accumulation;
    const float* d_expected_depth;
    const float* d_rgb;
    const float* d_feature;
} pixie_ray_upstream;
/* gradients, WRITTEN (not accumulated); NULL = not wanted.  Deltas, starts and ends get none. */
typedef struct pixie_ray_grads {
    float* d_densities;            /* (R, S) density mode */
    float* d_weights;              /* (R, S) weights mode */
    float* d_rgb;                  /* (R, S, 3); needs upstream.d_rgb */
    float* d_features;             /* (R, S, C); needs upstream.d_feature */
} pixie_ray_grads;
/* The backward forms g_i = dL/dw_i as the sum, in this order, of the terms of the weights output, the feature (its partial dot
 * products per 256-channel chunk, in chunk order), the accumulation, the expected depth and the rgb, each term one float32; in the
 * weights mode that is d_weights.  In the density mode g_i is zeroed where nan_to_num replaced the weight, and
 *     d_density_k = delta_k (g_k exp(-x_k) exp(-P_k) - sum_{i>k} g_i w_i),
 * finite wherever the upstream gradients are: a NaN density gives zeros from its sample onward, not NaN.
 * d_scratch: scratch_bytes = 4 R ceil(C / 256) S, read and written only when upstream.d_feature is set and d_densities or d_weights
 * is wanted; may be NULL otherwise. */
int pixie_ray_composite_bytes(const pixie_ray_desc* desc, int64_t* scratch_bytes);
int pixie_ray_composite_forward(const pixie_ray_desc* desc, const pixie_ray_inputs* inputs, const pixie_ray_outputs* outputs, void* stream);
int pixie_ray_composite_backward(const pixie_ray_desc* desc, const pixie_ray_inputs* inputs, const pixie_ray_upstream* upstream,
                                 const pixie_ray_grads* grads, void* d_scratch, void* stream);

/* ---- proposal sampling and its losses (pixie_amd/csrc/ray_sample.hip) ----
 * nerfstudio's SpacedSampler family and PDFSampler.generate_ray_samples with Frustums.get_positions, and interlevel_loss /
 * distortion_loss forward and backward.  All arrays are float32, contiguous, on the device; R = n_rays.  The samplers have no
 * gradient (the reference detaches the bins); the losses are differentiable in the weights alone.  Random numbers and the linspace
 * tables are inputs.  Limits: 1 <= R <= 2^24, at most 1024 existing and 1024 produced samples per ray (with include_original:
 * n_samples + n_existing + 1 <= 1024), at most 8 proposal levels.  Anything else is refused with a non-zero return before any
 * launch.  Every sum has one fixed order: bit-identical from run to run, under a permutation of the rays and for any R.  No
 * floating-point atomics.  Asynchronous on `stream`: no synchronise, no host read-back. */
typedef struct pixie_ray_sample_desc {
    int64_t n_rays;
    int32_t n_samples;             /* spaced: the samples produced; pdf: num_samples, so n_samples + 1 new bins */
    int32_t n_existing;            /* pdf: samples of the existing level; spaced: ignored */
    int32_t spacing;               /* 0 uniform, 1 linear in disparity, 2 sqrt, 3 log, 4 uniform / linear-disparity piecewise;
                                      pdf only: -1 = a foreign spacing function, the spacing bins are the only output */
    int32_t jitter_stride;         /* 0: no jitter (eval mode), 1: one per ray (single_jitter), n_samples + 1: one per bin */
    int32_t include_original;      /* pdf: merge the existing bins into the new ones */
    float histogram_padding;       /* pdf */
    float eps;                     /* pdf: the weight an empty ray is padded to */
    float anneal;                  /* pdf: weights are raised to this power (float(pow(double))); 1 skips it */
    float u_scale;                 /* pdf: u_k = table_k + jitter * u_scale (torch on the device: float32(1) / (n_samples + 1)) */
    float u_offset;                /* pdf without jitter: u_k = table_k + u_offset (float32(1 / (2 (n_samples + 1)))) */
} pixie_ray_sample_desc;
typedef struct pixie_ray_sample_inputs {
    const float* d_nears;          /* (R) spaced */
    const float* d_fars;           /* (R) spaced */
    const float* d_origins;        /* (R, 3) or NULL: only for positions */
    const float* d_directions;     /* (R, 3) */
    const float* d_table;          /* spaced: linspace(0, 1, n_samples + 1); pdf: linspace(0, 1 - 1 / (n_samples + 1), n_samples + 1) */
    const float* d_jitter;         /* (R, jitter_stride) uniform in [0, 1), or NULL */
    const float* d_existing_bins;  /* pdf: (R, n_existing + 1) spacing bins, non-decreasing */
    const float* d_weights;        /* pdf: (R, n_existing) */
    const float* d_s_near;         /* pdf: (R) spacing_fn(near), the spaced call's output; NULL with a foreign spacing */
    const float* d_s_far;
} pixie_ray_sample_inputs;
/* M = n_samples (spaced, pdf) or n_samples + n_existing + 1 (pdf with include_original).  NULL = not wanted. */
typedef struct pixie_ray_sample_outputs {
    float* d_bins;                 /* (R, M + 1) spacing bins */
    float* d_starts;               /* (R, M) euclidean */
    float* d_ends;                 /* (R, M) */
    float* d_deltas;               /* (R, M) ends - starts */
    float* d_positions;            /* (R, M, 3) origins + directions * (starts + ends) / 2 */
    float* d_s_near;               /* (R) spaced only */
    float* d_s_far;
} pixie_ray_sample_outputs;
int pixie_ray_sample_spaced(const pixie_ray_sample_desc* desc, const pixie_ray_sample_inputs* inputs, const pixie_ray_sample_outputs* outputs,
                            void* stream);
/* A NaN weight makes the ray's cdf all zero: every new bin lands on the ray's last existing edge. */
int pixie_ray_sample_pdf(const pixie_ray_sample_desc* desc, const pixie_ray_sample_inputs* inputs, const pixie_ray_sample_outputs* outputs,
                         void* stream);

#define PIXIE_RAY_MAX_LEVELS 8
/* loss = sum over levels of mean over (R, n_fine) of clip(w - w_outer, 0)^2 / (w + 1e-7); d_loss: one float */
typedef struct pixie_ray_interlevel_desc {
    int64_t n_rays;
    int32_t n_fine;                                /* samples of the last level, whose edges and weights bound the others */
    int32_t n_levels;                              /* proposal levels, 1 .. 8 */
    int32_t n_proposal[PIXIE_RAY_MAX_LEVELS];      /* samples per proposal level */
    int32_t per_sample;                            /* 1: lossfun_outer itself, one level: the forward writes the (R, n_fine) terms and
                                                      no mean, the backward's d_upstream is (R, n_fine) */
} pixie_ray_interlevel_desc;
typedef struct pixie_ray_interlevel_inputs {
    const float* d_fine_edges;                     /* (R, n_fine + 1) spacing bins */
    const float* d_fine_weights;                   /* (R, n_fine) */
    const float* d_edges[PIXIE_RAY_MAX_LEVELS];    /* (R, n_proposal[l] + 1) */
    const float* d_weights[PIXIE_RAY_MAX_LEVELS];  /* (R, n_proposal[l]) */
} pixie_ray_interlevel_inputs;
typedef struct pixie_ray_interlevel_grads {
    float* d_weights[PIXIE_RAY_MAX_LEVELS];        /* (R, n_proposal[l]), WRITTEN; NULL = not wanted */
} pixie_ray_interlevel_grads;
int pixie_ray_interlevel_bytes(const pixie_ray_interlevel_desc* desc, int64_t* scratch_bytes);   /* 4 R n_levels: one float per ray and level */
int pixie_ray_interlevel_forward(const pixie_ray_interlevel_desc* desc, const pixie_ray_interlevel_inputs* inputs, float* d_loss,
                                 float* d_per_sample, void* d_scratch, void* stream);
/* d_upstream: dL/d loss, one float on the device.  The fine level gets no gradient. */
int pixie_ray_interlevel_backward(const pixie_ray_interlevel_desc* desc, const pixie_ray_interlevel_inputs* inputs, const float* d_upstream,
                                  const pixie_ray_interlevel_grads* grads, void* stream);

/* loss = mean over rays of sum_i w_i sum_j w_j |u_i - u_j| + sum_i w_i^2 (t_{i+1} - t_i) / 3, u the interval mid-points; the double
 * sum is direct, S^2 terms per ray from LDS: no (R, S, S) array exists.  d_edges (R, S + 1), d_weights and d_grad_weights (R, S). */
typedef struct pixie_ray_distortion_desc {
    int64_t n_rays;
    int32_t n_samples;
    int32_t per_ray;               /* backward: 1 = d_upstream is (R), the gradient of lossfun_distortion's per-ray values */
} pixie_ray_distortion_desc;
int pixie_ray_distortion_bytes(const pixie_ray_distortion_desc* desc, int64_t* scratch_bytes);   /* 4 R */
/* d_scratch receives the per-ray values (lossfun_distortion); d_loss their mean, or NULL */
int pixie_ray_distortion_forward(const pixie_ray_distortion_desc* desc, const float* d_edges, const float* d_weights, float* d_loss,
                                 void* d_scratch, void* stream);
int pixie_ray_distortion_backward(const pixie_ray_distortion_desc* desc, const float* d_edges, const float* d_weights, const float* d_upstream,
                                  float* d_grad_weights, void* stream);

/* ======================================================================================
 * Diagnostic entry points -- NOT part of the drop-in ABI.  They exist only in the -DPIXIE_DIAG build of the same sources,
 * libpixie_hip_diag.so, which the parity tests (per-phase comparison with the oracle) and the profilers (per-launch timings)
 * load; the production library libpixie_hip.so exports none of them and carries no trace buffer.
 * ====================================================================================== */
#ifdef PIXIE_DIAG
/* One phase of a substep, for per-kernel parity tests: 0 = pre-P2G modifiers + stress + P2G,
 * 1 = grid update + damping + BCs (+ host `modify`), 2 = G2P.  Does not advance time. */
int pixie_mpm_phase(pixie_mpm* h, int phase, double dt, void* stream);

/* Average duration in ms of the fused particle kernel / grid kernel over the launches since the
 * last call, measured with HIP events on `stream` (enable with set_scalar "profile"=1). */
int pixie_mpm_kernel_times(pixie_mpm* h, double* particle_ms, double* grid_ms, int64_t* n_launches);

/* Which kernel instantiation pixie_conv3d_forward picks for this descriptor: ksize*100 + MB*10 + NB of
 * conv3d_f16x3_kernel<ksize,MB,NB> -- with a folded skip convolution: of conv3d_f16x3_skip_kernel<ksize,MB,NB,...>, the same
 * number -- (and its split-K factor in *slices), 9324 = conv3d_f16x3_c64_fullres_kernel (the <3,2,4>
 * code under its own symbol for the 64 -> 64 full-resolution 3^3 layers), 0 = the exact-fp32 kernel.  For profilers that
 * want to group per-launch timings by kernel name, as rocprofv3 does; no reference counterpart.
 * The number does not say which launch form runs it: unsplit NB = 4 plans with an even number of 64-channel blocks and no folded skip
 * are launched in pair form (conv3d_f16x3_pair_kernel<ksize,4>: 512 threads over one tile and 128 output channels, same results bit
 * for bit).
 * desc == NULL is the switch between the two forms, for tests and timings that need both from one build: *slices = 1 makes every
 * following launch of this process keep the 4-wave kernels, *slices = 0 gives the choice back to the launcher, any other value (or
 * slices == NULL) changes nothing; returns the setting before the call.  The product library has no such switch. */
int pixie_conv_kernel_variant(const pixie_conv_desc* desc, int* slices);

/* The tiling pixie_conv3d_forward launches this descriptor with, from the launchers' own selection code (a pure host function of
 * the descriptor; no device needed): out = TX, TY, TZ (tile extents in output voxels; sub-pixel launches: in STORED voxels, each
 * tile being four (z, y)-parity workgroups), tiles_x, tiles_y, tiles_z, epi_lds (1 = the launch reserves LDS for the transposing
 * epilogue), slices (split-K factor), MB, NB.  With desc->d_w16 set it describes the f16x3 launch, otherwise the exact-fp32
 * launch of the same tiled body.  Returns 1 for descriptors that take neither (the first-generation exact kernel).  For tests that
 * must know which kernel variant and tile geometry a shape exercises.
 * out == NULL asks for the launch form instead, from the launcher's own decision (a pure function of the plan and of whether a
 * folded skip rides along): returns the dynamic LDS bytes of the pair-form launch, or 0 where the descriptor keeps the 4-wave
 * kernel (always 0 while the switch of pixie_conv_kernel_variant is set). */
int pixie_conv_tile_geometry(const pixie_conv_desc* desc, int32_t out[10]);
/* Where this descriptor's launch leaves the partial statistics of desc->d_out_stats, from the code pixie_stats_finalize and
 * pixie_stats_norm_finalize read them with (a pure host function of the descriptor): out = n (partials per channel), cstride,
 * tstride (partial t of channel c is the (sum, sum of squares) pair number c * cstride + t * tstride), f64 (1: float64 pairs, one
 * per segment of the split-K reduce, [c_out][n][2]; 0: float32 pairs, one per tile of the conv epilogue, [n][c_out padded][2]),
 * segment (voxels of one channel per reduce segment, the last one may be shorter; 0 for tile partials), c_out padded.
 * Returns 1 for descriptors off the f16x3 path.  For tests that must know which statistics code a shape exercises. */
int pixie_conv_stats_layout(const pixie_conv_desc* desc, int64_t out[6]);
#endif /* PIXIE_DIAG */

#ifdef __cplusplus
}
#endif
#endif /* PIXIE_HIP_H */
