"""ctypes binding of libnerftex_hip.so (C ABI: include/nerftex_hip.h).

This is plumbing: device memory, streams and autograd come from PyTorch-ROCm, every kernel comes from
the hand-written HIP library.  There is NO fallback: if the library is missing or a GPU op is invoked
without it, importing / calling fails loudly (a CPU or eager-PyTorch substitute would void parity).

    from nerftex_hip import lib, ptr, stream, check
    check(lib.nerftex_packbits(ptr(grid), N, thresh, ptr(bitfield), stream()))
"""
import ctypes as C
import os

from ._build import CSRC, LIB_PATH, PKG_ROOT  # noqa: F401

F32, F16 = 0, 1
LAYOUT_LBC, LAYOUT_BLC = 0, 1
LAYOUT_GRAD_OVERWRITE = 0x100  # backward: grad_embeddings is uninitialised and gets overwritten
LOSS_MSE, LOSS_L1, LOSS_HUBER = 0, 1, 2  # nerftex_step_loss_desc.kind


def rows_auto(n_rays, slots_per_ray):
    """NERFTEX_ROWS_AUTO(N, F): the n_step / rows_per_unit code that makes the kernels derive n_step from the alive count on the device."""
    assert 0 < n_rays < (1 << 24) and 0 < slots_per_ray <= 127
    return 0x80000000 | (int(slots_per_ray) << 24) | int(n_rays)


from ._build import build  # noqa: E402,F401


_u32, _f32, _i, _vp, _sz = C.c_uint32, C.c_float, C.c_int, C.c_void_p, C.c_size_t
_u64, _f64 = C.c_uint64, C.c_double

# name -> argument ctypes, in the order of include/nerftex_hip.h
_SIGNATURES = {
    "nerftex_field_forward": [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_amp": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_grid_encode_backward_amp": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _i, _vp, _vp, _u32, _i, _i, _i, _f32, _f32, _vp, _vp],
    "nerftex_field_density": [_vp, _vp, _u32, _vp, _vp],
    "nerftex_grid_encode_backward_phase": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _i, _i, _i, _f32, _f32, _i, _u32, _u32, _vp],
    "nerftex_release_workspaces": [],
    "nerftex_workspace_capture_set": [_i],
    "nerftex_field_forward_rows": [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp],
    "nerftex_grid_encode_forward_rows": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _i, _i, _i, _f32, _f32, _vp, _u32, _vp],
    "nerftex_field_mid_forward": [_vp, _vp, _u32, _vp, _vp, _vp],
    "nerftex_curved_pack_inputs": [_vp, _vp, _u32, _vp, _vp],
    "nerftex_curved_mid_forward": [_vp, _vp, _vp, _u32, _f32, _i, _vp, _vp, _vp],
    "nerftex_curved_out_forward": [_vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp],
    "nerftex_curved_field_infer": [_vp, _vp],
    "nerftex_curved_light_infer": [_vp, _vp],
    "nerftex_planar_lookup": [_vp, _vp, _u32, _u32, _u32, _f32, _f32, _f32, _f32, _f32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _vp],
    "nerftex_curved_import_infer": [_vp, _vp],
    "nerftex_planar_light_lookup": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _f32, _f32, _f32, _f32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp],
    "nerftex_curved_light_import_infer": [_vp, _vp],
    "nerftex_shape_lookup": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _u32, _f32, _f32, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp],
    "nerftex_curved_shape_infer": [_vp, _vp],
    "nerftex_vertex_lookup": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _f32, _vp, _u32, _vp, _u32, _vp, _f32, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp],
    "nerftex_curved_unhash_infer": [_vp, _vp],
    "nerftex_shape_light_lookup": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _f32, _f32, _f32,
                                   _f32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_curved_light_shape_infer": [_vp, _vp],
    "nerftex_patch_front": [_vp, _vp],
    "nerftex_patch_lookup": [_vp, _vp, _vp, _vp, _u32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_patch_light_lookup": [_vp, _vp, _vp, _vp, _vp, _u32, _f32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_curved_patch_infer": [_vp, _vp],
    "nerftex_curved_light_patch_infer": [_vp, _vp],
    "nerftex_curved_light_infer_relit": [_vp, _vp, _vp],
    "nerftex_curved_light_import_infer_relit": [_vp, _vp, _vp],
    "nerftex_curved_light_shape_infer_relit": [_vp, _vp, _vp],
    "nerftex_curved_light_patch_infer_relit": [_vp, _vp, _vp],
    "nerftex_sh_light_forward": [_vp, _vp],
    "nerftex_sh_light_backward": [_vp, _vp],
    "nerftex_sh_light_probe_forward": [_vp, _vp],
    "nerftex_envmap_fit": [_vp, _vp],
    "nerftex_envmap_vis_fit": [_vp, _vp],
    "nerftex_field_mid_backward": [_vp, _vp, _vp, _u32, _vp, _vp],
    "nerftex_field_out_forward": [_vp, _u32, _vp, _vp],
    "nerftex_field_out_backward": [_vp, _vp, _u32, _vp, _vp],
    "nerftex_render_tail_forward": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_render_tail_backward": [_vp, _vp, _f32, _vp, _vp, _f32, _u32, _vp, _vp, _vp],
    "nerftex_composite_tail_backward": [_vp, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp],
    "nerftex_adam_half_step": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _f64, _f64, _f64, _f64, _vp, _vp, _vp],
    "nerftex_amp_check_half": [_i, _vp, _vp, _vp, _vp],
    "nerftex_adam_half_step_amp": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _f64, _f64, _i, _vp],
    "nerftex_amp_update": [_vp, _vp, _vp, _vp, _f64, _f64, _i, _vp],
    "nerftex_adam_mixed_step": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _f32, _f64, _f64, _f64, _f64, _vp, _vp, _vp],
    "nerftex_adam_mixed_step_amp": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _f64, _f64, _i, _vp],
    "nerftex_amp_check_mixed": [_i, _vp, _vp, _u32, _vp, _vp],
    "nerftex_adam_mixed_step_amp_db": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _f64, _f64, _i,
                                       _vp, _vp, _vp, _vp, _u64, _vp],
    "nerftex_adam_mixed_step_amp_sched": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _f64, _vp, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _f64, _f64, _i,
                                          _vp],
    "nerftex_adam_mixed_step_amp_db_sched": [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _f64, _vp, _f64, _f64, _f64, _vp, _vp, _vp, _vp,
                                             _f64, _f64, _i, _vp, _vp, _vp, _vp, _u64, _vp],
    "nerftex_lr_schedule_publish": [_vp, _vp, _vp, _u32, _vp],
    "nerftex_ema_update": [_vp, _i, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_live": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_live_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_live_consume": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_live_consume_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_live_deferred": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_backward_live_deferred_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_step_trailer_run": [_vp, _vp],
    "nerftex_grid_encode_backward_adam_trailer": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _i, _i, _i, _f32, _f32, _vp, _vp, _vp, _vp],
    "nerftex_composite_step": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_render_tail_forward_live": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "nerftex_composite_tail_backward_live": [_vp, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp],
    "nerftex_render_tail_forward_ex": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp],
    "nerftex_render_tail_backward_ex": [_vp, _vp, _f32, _vp, _vp, _f32, _u32, _vp, _vp, _vp, _vp],
    "nerftex_composite_tail_backward_ex": [_vp, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp],
    "nerftex_composite_step_ex": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp],
    # the four _ex entries with a nerftex_step_pixels_desc (StepPixelsDesc) before the stream
    "nerftex_render_tail_forward_px": [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp],
    "nerftex_render_tail_backward_px": [_vp, _vp, _f32, _vp, _vp, _f32, _u32, _vp, _vp, _vp, _vp, _vp],
    "nerftex_composite_tail_backward_px": [_vp, _vp, _f32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_composite_step_px": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp],
    "nerftex_grid_encode_backward_adam": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _i, _i, _i, _f32, _f32, _vp, _vp, _vp],
    "nerftex_field_forward_bf16": [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_field_density_bf16": [_vp, _vp, _u32, _vp, _vp],
    "nerftex_field_forward_rows_bf16": [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _vp],
    "nerftex_field_backward_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_table_adam_step": [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _vp],
    "nerftex_tune_set": [C.c_char_p, C.c_long],
    "nerftex_profile_enable": [_i],
    "nerftex_profile_reset": [],
    "nerftex_profile_report": [C.c_char_p, _sz],
    "nerftex_grid_encode_forward": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _i, _vp, _u32, _i, _i, _i, _vp],
    "nerftex_grid_encode_backward": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _i, _vp, _vp, _u32, _i, _i, _i, _vp],
    "nerftex_grid_register_offsets": [_vp, _u32, _vp],
    "nerftex_deferred_error": [],
    "nerftex_grid_cluster_scratch_bytes": [_vp, C.POINTER(_sz)],
    "nerftex_grid_cluster_loss": [_vp, _vp],
    "nerftex_grid_encode_forward_affine": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _i, _vp, _u32, _i, _i, _i, _f32, _f32, _vp],
    "nerftex_grid_encode_backward_affine": [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _f32, _u32, _i, _vp, _vp, _u32, _i, _i, _i, _f32, _f32, _vp],
    "nerftex_sh_encode_forward": [_vp, _vp, _u32, _u32, _u32, _i, _vp, _vp],
    "nerftex_sh_encode_backward": [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp],
    "nerftex_near_far_from_aabb": [_vp, _vp, _vp, _u32, _f32, _vp, _vp, _vp],
    "nerftex_polar_from_ray": [_vp, _vp, _f32, _u32, _vp, _vp],
    "nerftex_morton3D": [_vp, _u32, _vp, _vp],
    "nerftex_morton3D_invert": [_vp, _u32, _vp, _vp],
    "nerftex_packbits": [_vp, _u32, _f32, _vp, _vp],
    "nerftex_march_rays_train": [_vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "nerftex_march_rays_train_fresh": [_vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "nerftex_march_rays_train_differentiable": [_vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "nerftex_composite_rays_train_forward": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp],
    "nerftex_composite_rays_train_backward": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp],
    "nerftex_march_rays": [_u32, _u32, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "nerftex_composite_rays": [_u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_compact_rays": [_u32, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_march_rays_dev": [_u32, _vp, _u32, _vp, _vp, _vp, _vp, _f32, _f32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
    "nerftex_composite_rays_dev": [_u32, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_compact_rays_dev": [_u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_compact_rays_budget_dev": [_u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp],
    "nerftex_compact_rays_budget_mirror_dev": [_u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp],
    "nerftex_occupancy_sample_full": [_vp, _u32, _u32, _f32, _vp, _u64, _vp],
    "nerftex_occupancy_sample_partial": [_vp, _u32, _u32, _f32, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp],
    "nerftex_occupancy_sample_partial_ordered": [_vp, _u32, _u32, _f32, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _vp],
    "nerftex_occupancy_update": [_vp, _vp, _vp, _u32, _u32, _u32, _f32, _i, _f32, _vp, _vp, _vp],
    "nerftex_ffmlp_forward": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp],
    "nerftex_ffmlp_inference": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp],
    "nerftex_ffmlp_backward": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _i, _vp, _vp, _vp, _vp],
    "nerftex_ffmlp_forward_bf16": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp],
    "nerftex_ffmlp_inference_bf16": [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp],
    "nerftex_ffmlp_backward_bf16": [_vp, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _i, _vp, _vp, _vp, _vp],
    "nerftex_ffmlp_allocate_splitk": [_sz],
    "nerftex_ffmlp_free_splitk": [],
    "nerftex_create_raytracer": [_vp, _u32, _vp, _u32, C.POINTER(_vp)],
    "nerftex_destroy_raytracer": [_vp],
    "nerftex_curved_project": [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _f32, _f32, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nerftex_knn_create": [_vp, _u32, C.POINTER(_vp)],
    "nerftex_knn_destroy": [_vp],
    "nerftex_knn_query": [_vp, _vp, _u32, _u32, _vp, _vp, _vp],
    "nerftex_synth_create": [_vp, C.POINTER(_vp)],
    "nerftex_synth_resolve": [_vp, _u32, _vp, _vp, _u32, _u32, _vp],
    "nerftex_synth_finish": [_vp, _vp],
    "nerftex_synth_result": [_vp, _vp],
    "nerftex_synth_read": [_vp, _u32, _vp, _sz, _vp],
    "nerftex_synth_destroy": [_vp],
    "nerftex_debug_workspace": [C.c_int, _vp, C.POINTER(_vp), C.POINTER(C.c_size_t)],
    "nerftex_raytracer_trace": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _vp],
}
class LrSchedule(C.Structure):
    """nerftex_lr_schedule of include/nerftex_hip.h, field for field."""
    _fields_ = [("factor", _vp), ("n", _u32), ("iter", _vp)]


class EmaDesc(C.Structure):
    """nerftex_ema_desc of include/nerftex_hip.h, field for field."""
    _fields_ = [("decay", _f64), ("num_updates", _vp), ("ticket", _vp), ("live", _vp), ("advance", _i)]


# the launch shape of nerftex_ema_update (csrc/trainstep.hip: kEmaThreads, kEmaVec, kEmaBlocksPerCu, kEmaUnroll, kMaxTensors)
EMA_THREADS, EMA_VEC, EMA_BLOCKS_PER_CU, EMA_UNROLL, EMA_MAX_TENSORS = 512, 4, 2, 4, 8


class TableAdam(C.Structure):
    """nerftex_table_adam of include/nerftex_hip.h, field for field (sched: address of a LrSchedule, or None)."""
    _fields_ = [("param", _vp * 2), ("exp_avg", _vp * 2), ("exp_avg_sq", _vp * 2), ("param_half", _vp), ("live", _vp), ("step", _vp),
                ("grad_scale", _vp), ("found_inf", _vp), ("lr", _f64), ("beta1", _f64), ("beta2", _f64), ("eps", _f64), ("sched", _vp)]


class StepTrailer(C.Structure):
    """nerftex_step_trailer of include/nerftex_hip.h: opaque, filled by nerftex_field_backward_live_deferred."""
    _fields_ = [("opaque", C.c_uint64 * 16)]


class GridClusterDesc(C.Structure):
    """nerftex_grid_cluster_desc of include/nerftex_hip.h, field for field."""
    _fields_ = [("table", _vp), ("offsets", _vp), ("C", _u32), ("L", _u32), ("K", _u32), ("max_level_rows", _u32), ("centres", _vp), ("alpha", _f32),
                ("weight", _f32), ("level", _vp), ("grad_scale", _vp), ("loss", _vp), ("grad_table", _vp), ("grad_centres", _vp), ("scratch", _vp),
                ("scratch_bytes", _sz)]


class StepLoss(C.Structure):
    """nerftex_step_loss of include/nerftex_hip.h, field for field."""
    _fields_ = [("err", _vp), ("n_rays", _u32), ("loss_mul", _f32), ("scale", _vp), ("loss", _vp), ("scaled_loss", _vp)]


class StepLossDesc(C.Structure):
    """nerftex_step_loss_desc of include/nerftex_hip.h, field for field: the criterion of a step, its per-ray loss and the error map."""
    _fields_ = [("kind", _u32), ("param", _f32), ("ray_loss", _vp), ("error_map", _vp), ("error_inds", _vp), ("error_cells", _u64), ("keep", _f32),
                ("take", _f32)]


class StepPixelsDesc(C.Structure):
    """nerftex_step_pixels_desc of include/nerftex_hip.h, field for field: a training step's per-ray background and RGBA pixels."""
    _fields_ = [("bg_rays", _vp), ("rgba", _vp), ("target_out", _vp)]


class CurvedInferDesc(C.Structure):
    """nerftex_curved_infer_desc of include/nerftex_hip.h, field for field: the curved field's no-grad forward as one device-count call."""
    # (knn down to in_mul: the members nerftex_curved_light_infer_desc begins with, too)
    _prefix = [("knn", _vp), ("tracer", _vp), ("xyz", _vp), ("dirs", _vp), ("B", _u32), ("n_verts", _u32), ("mesh_vertices", _vp), ("vertex_normals", _vp),
               ("tbn", _vp), ("K", _u32), ("n_freqs", _u32), ("dir_vec_wdist", _f32), ("h_threshold", _f32), ("table", _vp), ("offsets", _vp), ("D", _u32),
               ("C", _u32), ("L", _u32), ("S", _f32), ("H", _u32), ("gridtype", _u32), ("align_corners", _i), ("in_add", _f32), ("in_mul", _f32)]
    _fields_ = _prefix + [("sigma_weights", _vp), ("sigma_in", _u32), ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32),
                ("color_weights", _vp), ("color_in", _u32), ("color_hidden", _u32), ("color_layers", _u32), ("color_out", _u32), ("fc_weight", _f32),
                ("eval", _i), ("sigma", _vp), ("rgbs", _vp), ("units_dev", _vp), ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


PLANAR_MULTIPLY, PLANAR_DIVIDE = 0, 1  # NERFTEX_PLANAR_*: nerftex_planar_lookup's mode


class CurvedImportInferDesc(C.Structure):
    """nerftex_curved_import_infer_desc of include/nerftex_hip.h, field for field: the curved field's no-grad forward over an imported planar map."""
    _fields_ = [("xyz", _vp), ("dirs", _vp), ("B", _u32), ("map", _vp), ("map_h", _u32), ("map_w", _u32), ("n_features", _u32), ("mode", _u32),
                ("plane_scale0", _f32), ("plane_scale1", _f32), ("height_scale0", _f32), ("height_scale1", _f32), ("sdf_offset", _f32), ("h_threshold", _f32),
                ("n_freqs", _u32), ("sigma_weights", _vp), ("sigma_in", _u32), ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32),
                ("color_weights", _vp), ("color_in", _u32), ("color_hidden", _u32), ("color_layers", _u32), ("color_out", _u32), ("fc_weight", _f32),
                ("eval", _i), ("sigma", _vp), ("rgbs", _vp), ("units_dev", _vp), ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


class CurvedShapeInferDesc(C.Structure):
    """nerftex_curved_shape_infer_desc of include/nerftex_hip.h, field for field: the curved field's no-grad forward over an imported map on a new mesh."""
    _fields_ = [("knn", _vp), ("tracer", _vp), ("xyz", _vp), ("dirs", _vp), ("B", _u32), ("n_verts", _u32), ("mesh_vertices", _vp), ("vertex_normals", _vp),
                ("face_uv", _vp), ("n_faces", _u32), ("K", _u32), ("map", _vp), ("map_h", _u32), ("map_w", _u32), ("n_features", _u32), ("sdf_scale", _f32),
                ("sdf_offset", _f32), ("uv_rate", _f32), ("h_threshold", _f32), ("n_freqs", _u32), ("sigma_weights", _vp), ("sigma_in", _u32),
                ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32), ("color_weights", _vp), ("color_in", _u32), ("color_hidden", _u32),
                ("color_layers", _u32), ("color_out", _u32), ("fc_weight", _f32), ("eval", _i), ("sigma", _vp), ("rgbs", _vp), ("units_dev", _vp),
                ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


class CurvedUnhashInferDesc(C.Structure):
    """nerftex_curved_unhash_infer_desc of include/nerftex_hip.h, field for field: the curved field's no-grad forward over features baked onto the vertices of
    a fine mesh."""
    _fields_ = [("knn", _vp), ("tracer", _vp), ("xyz", _vp), ("dirs", _vp), ("B", _u32), ("n_verts", _u32), ("mesh_vertices", _vp), ("vertex_normals", _vp),
                ("K", _u32), ("dir_vec_wdist", _f32), ("fine_vertices", _vp), ("n_fine_verts", _u32), ("face_vertices", _vp), ("n_faces", _u32),
                ("vertex_features", _vp), ("n_features", _u32), ("sdf_scale", _f32), ("sdf_offset", _f32), ("h_threshold", _f32), ("n_freqs", _u32),
                ("sigma_weights", _vp), ("sigma_in", _u32), ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32), ("color_weights", _vp),
                ("color_in", _u32), ("color_hidden", _u32), ("color_layers", _u32), ("color_out", _u32), ("fc_weight", _f32), ("eval", _i), ("sigma", _vp),
                ("rgbs", _vp), ("units_dev", _vp), ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


LIGHT_VISUAL = {"Full": 0, "Specular": 1, "Diffuse": 2, "Albedo": 3}  # NERFTEX_LIGHT_VISUAL_*
NORMAL_NET_WEIGHTS, NORMAL_NET_BIASES = 1312, 66  # NERFTEX_NORMAL_NET_*


class CurvedLightInferDesc(C.Structure):
    """nerftex_curved_light_infer_desc of include/nerftex_hip.h, field for field: the SH-lit curved field's no-grad forward as one device-count call."""
    _fields_ = CurvedInferDesc._prefix + [("normal_table", _vp), ("normal_offsets", _vp), ("normal_C", _u32), ("normal_L", _u32), ("normal_S", _f32),
                ("normal_H", _u32), ("normal_gridtype", _u32), ("normal_align_corners", _i), ("normal_in_add", _f32), ("normal_in_mul", _f32),
                ("sigma_weights", _vp), ("sigma_in", _u32), ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32), ("normal_weights", _vp),
                ("normal_biases", _vp), ("normal_hidden", _u32), ("normal_layers", _u32), ("brdf_weights", _vp), ("brdf_in", _u32), ("brdf_hidden", _u32),
                ("brdf_layers", _u32), ("brdf_out", _u32), ("env_shs", _vp), ("n_sh", _u32), ("n_color", _u32), ("gamma", _f32), ("flags", _u32),
                ("visual_mode", _u32), ("fc_weight", _f32), ("eval", _i), ("sigma", _vp), ("rgbs", _vp), ("shading_normal", _vp), ("units_dev", _vp),
                ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


FRAME_MAP_STRIDE = 12  # NERFTEX_FRAME_MAP_STRIDE: floats per texel of the frame map and per row of the inverted patch frames


class CurvedLightImportInferDesc(C.Structure):
    """nerftex_curved_light_import_infer_desc of include/nerftex_hip.h, field for field: the SH-lit curved field's no-grad forward over imported maps."""
    _fields_ = [("xyz", _vp), ("dirs", _vp), ("B", _u32), ("map", _vp), ("phi_map", _vp), ("frame_map", _vp), ("sample_tbn_inv", _vp), ("map_h", _u32),
                ("map_w", _u32), ("n_features", _u32), ("n_phi", _u32), ("n_patches", _u32), ("mode", _u32), ("plane_scale0", _f32), ("plane_scale1", _f32),
                ("height_scale0", _f32), ("height_scale1", _f32), ("sdf_offset", _f32), ("h_threshold", _f32), ("n_freqs", _u32), ("sigma_weights", _vp),
                ("sigma_in", _u32), ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32), ("normal_weights", _vp), ("normal_biases", _vp),
                ("normal_hidden", _u32), ("normal_layers", _u32), ("brdf_weights", _vp), ("brdf_in", _u32), ("brdf_hidden", _u32), ("brdf_layers", _u32),
                ("brdf_out", _u32), ("env_shs", _vp), ("n_sh", _u32), ("n_color", _u32), ("gamma", _f32), ("flags", _u32), ("visual_mode", _u32),
                ("fc_weight", _f32), ("eval", _i), ("sigma", _vp), ("rgbs", _vp), ("shading_normal", _vp), ("units_dev", _vp), ("rows_per_unit", _u32),
                ("scratch", _vp), ("scratch_bytes", _sz)]


class CurvedLightShapeInferDesc(C.Structure):
    """nerftex_curved_light_shape_infer_desc of include/nerftex_hip.h, field for field: the SH-lit curved field's no-grad forward over imported maps on a
    new mesh."""
    _fields_ = [("knn", _vp), ("tracer", _vp), ("xyz", _vp), ("dirs", _vp), ("B", _u32), ("n_verts", _u32), ("mesh_vertices", _vp), ("vertex_normals", _vp),
                ("face_uv", _vp), ("face_tbn", _vp), ("n_faces", _u32), ("n_tbn_faces", _u32), ("K", _u32), ("map", _vp), ("phi_map", _vp), ("frame_map", _vp),
                ("sample_tbn_inv", _vp), ("map_h", _u32), ("map_w", _u32), ("n_features", _u32), ("n_phi", _u32), ("n_patches", _u32), ("sdf_scale", _f32),
                ("sdf_offset", _f32), ("uv_rate", _f32), ("h_threshold", _f32), ("n_freqs", _u32), ("sigma_weights", _vp), ("sigma_in", _u32),
                ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32), ("normal_weights", _vp), ("normal_biases", _vp), ("normal_hidden", _u32),
                ("normal_layers", _u32), ("brdf_weights", _vp), ("brdf_in", _u32), ("brdf_hidden", _u32), ("brdf_layers", _u32), ("brdf_out", _u32),
                ("env_shs", _vp), ("n_sh", _u32), ("n_color", _u32), ("gamma", _f32), ("flags", _u32), ("visual_mode", _u32), ("fc_weight", _f32), ("eval", _i),
                ("sigma", _vp), ("rgbs", _vp), ("shading_normal", _vp), ("units_dev", _vp), ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


class PatchFrontDesc(C.Structure):
    """nerftex_patch_front_desc of include/nerftex_hip.h, field for field: the front of the patch export for a chunk of candidates."""
    _fields_ = [("tracer", _vp), ("scan", _vp), ("frames", _vp), ("calibration", _vp), ("B", _u32), ("S", _u32), ("max_scan_dist", _f32),
                ("max_patch_num", _u32), ("origins", _vp), ("intersections", _vp), ("rays", _vp), ("stats", _vp), ("verdict", _vp), ("slot", _vp),
                ("count", _vp)]


PATCH_GEOM_STRIDE, PATCH_LIT_STRIDE = 8, 20  # NERFTEX_PATCH_*_STRIDE: floats per point of an imported patch's geom and lit records


class CurvedPatchInferDesc(C.Structure):
    """nerftex_curved_patch_infer_desc of include/nerftex_hip.h, field for field: the curved field's no-grad forward over an imported feature patch."""
    _fields_ = [("knn", _vp), ("xyz", _vp), ("dirs", _vp), ("B", _u32), ("n_points", _u32), ("geom", _vp), ("features", _vp), ("n_features", _u32),
                ("h_threshold", _f32), ("n_freqs", _u32), ("sigma_weights", _vp), ("sigma_in", _u32), ("sigma_hidden", _u32), ("sigma_layers", _u32),
                ("sigma_out", _u32), ("color_weights", _vp), ("color_in", _u32), ("color_hidden", _u32), ("color_layers", _u32), ("color_out", _u32),
                ("fc_weight", _f32), ("eval", _i), ("sigma", _vp), ("rgbs", _vp), ("units_dev", _vp), ("rows_per_unit", _u32), ("scratch", _vp),
                ("scratch_bytes", _sz)]


class CurvedLightPatchInferDesc(C.Structure):
    """nerftex_curved_light_patch_infer_desc of include/nerftex_hip.h, field for field: the SH-lit curved field's no-grad forward over an imported
    feature patch."""
    _fields_ = [("knn", _vp), ("xyz", _vp), ("dirs", _vp), ("B", _u32), ("n_points", _u32), ("geom", _vp), ("features", _vp), ("lit", _vp),
                ("n_features", _u32), ("n_phi", _u32), ("h_threshold", _f32), ("n_freqs", _u32), ("sigma_weights", _vp), ("sigma_in", _u32),
                ("sigma_hidden", _u32), ("sigma_layers", _u32), ("sigma_out", _u32), ("normal_weights", _vp), ("normal_biases", _vp), ("normal_hidden", _u32),
                ("normal_layers", _u32), ("brdf_weights", _vp), ("brdf_in", _u32), ("brdf_hidden", _u32), ("brdf_layers", _u32), ("brdf_out", _u32),
                ("env_shs", _vp), ("n_sh", _u32), ("n_color", _u32), ("gamma", _f32), ("flags", _u32), ("visual_mode", _u32), ("fc_weight", _f32), ("eval", _i),
                ("sigma", _vp), ("rgbs", _vp), ("shading_normal", _vp), ("units_dev", _vp), ("rows_per_unit", _u32), ("scratch", _vp), ("scratch_bytes", _sz)]


PATCH_ACCEPTED, PATCH_BELOW, PATCH_NAN, PATCH_FAR, PATCH_MISSED, PATCH_NOT_NEEDED = 0, 1, 2, 3, 4, 5  # the verdict codes of nerftex_patch_front (1: the host's)

SH_LIGHT_SPECULAR = 1  # nerftex_sh_light_desc.flags


class SHLightDesc(C.Structure):
    """nerftex_sh_light_desc of include/nerftex_hip.h, field for field: the SH light head's forward and backward."""
    _fields_ = [("brdf", _vp), ("brdf_stride", _u32), ("normals", _vp), ("dirs", _vp), ("env_shs", _vp), ("n_sh", _u32), ("n_color", _u32), ("mask", _vp),
                ("B", _u32), ("gamma", _f32), ("flags", _u32), ("color", _vp), ("specular", _vp), ("diffuse", _vp), ("albedo", _vp), ("grad_color", _vp),
                ("grad_brdf", _vp), ("grad_env_shs", _vp), ("scratch", _vp), ("scratch_bytes", _sz)]


SH_LIGHT_MAX_PROBES = 256  # nerftex_sh_light_probe_desc.K


class SHLightProbeDesc(C.Structure):
    """nerftex_sh_light_probe_desc of include/nerftex_hip.h, field for field: the head under per-probe imported lighting (forward only)."""
    _fields_ = [("brdf", _vp), ("brdf_stride", _u32), ("normals", _vp), ("dirs", _vp), ("normals_secondary", _vp), ("probes", _vp), ("probe_shs", _vp),
                ("K", _u32), ("mask", _vp), ("B", _u32), ("gamma", _f32), ("flags", _u32), ("color", _vp), ("specular", _vp), ("diffuse", _vp), ("albedo", _vp)]


class RelightDesc(C.Structure):
    """nerftex_relight_desc of include/nerftex_hip.h, field for field: per-probe lighting and the lighting rotation of the four _relit entries."""
    _fields_ = [("probes", _vp), ("probe_shs", _vp), ("K", _u32), ("rotation", _vp)]


class EnvmapFitDesc(C.Structure):
    """nerftex_envmap_fit_desc of include/nerftex_hip.h, field for field: SH lighting fitted to an environment map."""
    _fields_ = [("envmap", _vp), ("phi", _vp), ("theta", _vp), ("H", _u32), ("W", _u32), ("n_sh", _u32), ("max_steps", _u32), ("min_steps", _u32),
                ("lr", _f64), ("min_loss", _f64), ("env_shs", _vp), ("steps_run", _vp), ("final_loss", _vp), ("scratch", _vp), ("scratch_bytes", _sz)]


class EnvmapVisFitDesc(C.Structure):
    """nerftex_envmap_vis_fit_desc of include/nerftex_hip.h, field for field: the per-probe visibility lighting of an imported map."""
    _fields_ = [("env_shs", _vp), ("n_sh", _u32), ("lobes", _vp), ("K", _u32), ("rounds", _u32), ("batch", _u32), ("lr", _f64), ("seed", _u64),
                ("points", _vp), ("points_out", _vp), ("tables", _vp)]


# texture synthesis (nerftex_synth_*): status codes, modes, log layout and the arrays nerftex_synth_read copies
ERR_INVALID, ERR_HIP, ERR_EXHAUSTED = 1, 2, 3
SYNTH_CUT, SYNTH_BLEND, SYNTH_LOG_STRIDE = 0, 1, 36
SYNTH_CANVAS, SYNTH_CANVAS_ID, SYNTH_ID_MAP, SYNTH_LOG_IDS, SYNTH_LOG_DIST, SYNTH_TBN_IDS, SYNTH_TBN, SYNTH_TOTAL_ID = range(8)


class SynthDesc(C.Structure):
    """nerftex_synth_desc of include/nerftex_hip.h, field for field: what a texture synthesis is made of."""
    _fields_ = [("patches", _vp), ("sample_tbn", _vp), ("picked_vertices", _vp), ("P", _u32), ("S", _u32), ("C", _u32), ("match_dim", _u32),
                ("patch_size", _u32), ("overlap_size", _u32), ("output_h", _u32), ("output_w", _u32), ("mirror_hor", _u32), ("mirror_vert", _u32),
                ("attenuation", _u32), ("max_patch_res", _u32), ("mode", _u32), ("quilt", _u32), ("close_threshold", _f64), ("patch_length", _f64)]


class SynthView(C.Structure):
    """nerftex_synth_view of include/nerftex_hip.h, field for field: the device arrays of a synthesis and their sizes."""
    _fields_ = [("canvas", _vp), ("canvas_id", _vp), ("id_map", _vp), ("log_ids", _vp), ("log_dist", _vp), ("sample_tbn_ids", _vp), ("sample_tbn", _vp),
                ("total_id", _vp), ("side", _u32), ("cells_per_side", _u32), ("examples", _u32), ("channels", _u32), ("block", _u32), ("strip_floats", _u32),
                ("slices", _u32), ("n_total", _u32)]


EXPORTS = ["nerftex_last_error", "nerftex_version", "nerftex_tune_get", "nerftex_workspace_slots_touched", "nerftex_curved_field_infer_scratch_bytes",
           "nerftex_curved_light_infer_scratch_bytes", "nerftex_curved_import_infer_scratch_bytes", "nerftex_curved_shape_infer_scratch_bytes",
           "nerftex_curved_light_import_infer_scratch_bytes", "nerftex_curved_light_shape_infer_scratch_bytes", "nerftex_curved_patch_infer_scratch_bytes",
           "nerftex_curved_light_patch_infer_scratch_bytes", "nerftex_curved_unhash_infer_scratch_bytes", "nerftex_sh_light_scratch_bytes", "nerftex_envmap_fit_scratch_bytes"] + list(_SIGNATURES)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(needs hipcc; cross-compiles for gfx950 without a GPU). There is no CPU / eager fallback."
        )
    lib = C.CDLL(LIB_PATH)
    lib.nerftex_last_error.restype = C.c_char_p
    lib.nerftex_version.restype = C.c_char_p
    lib.nerftex_tune_get.argtypes = [C.c_char_p]
    lib.nerftex_tune_get.restype = C.c_long
    lib.nerftex_workspace_slots_touched.argtypes = []
    lib.nerftex_workspace_slots_touched.restype = C.c_uint
    lib.nerftex_curved_field_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_field_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_light_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_light_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_import_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_import_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_shape_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_shape_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_light_import_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_light_import_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_light_shape_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_light_shape_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_patch_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_patch_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_light_patch_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_light_patch_infer_scratch_bytes.restype = _sz
    lib.nerftex_curved_unhash_infer_scratch_bytes.argtypes = [_u32]
    lib.nerftex_curved_unhash_infer_scratch_bytes.restype = _sz
    lib.nerftex_sh_light_scratch_bytes.argtypes = [_u32]
    lib.nerftex_sh_light_scratch_bytes.restype = _sz
    lib.nerftex_envmap_fit_scratch_bytes.argtypes = [_u32, _u32]
    lib.nerftex_envmap_fit_scratch_bytes.restype = _sz
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == a symbol the header declares is not exported
        fn.argtypes = args
        fn.restype = C.c_int
    return lib


lib = _load()


def check(rc):
    """Raise RuntimeError with the library's message (mirrors the reference's TORCH_CHECK / runtime_error texts)."""
    if rc != 0:
        msg = lib.nerftex_last_error().decode() or f"nerftex_hip call failed with status {rc}"
        raise RuntimeError(msg)


class tune:
    """Set tuning knobs / A-B switches of the kernels (include/nerftex_hip.h: nerftex_tune_set); usable as a context manager:
    `with tune(grid_bwd=1): ...` restores the previous values on exit."""

    def __init__(self, **knobs):
        self._old = {k: lib.nerftex_tune_get(k.encode()) for k in knobs}
        for k, v in knobs.items():
            check(lib.nerftex_tune_set(k.encode(), int(v)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for k, v in self._old.items():
            check(lib.nerftex_tune_set(k.encode(), v))
        return False


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream():
    """torch's current HIP stream as the void* the C ABI expects (the raw handle: `torch.cuda.current_stream()` builds a Stream object,
    ~11 us a call, seven calls per eager training step)."""
    import torch

    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")


def require_contiguous(t, name):
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous tensor")


# ---- optional per-op device timing (bench.py turns it on to measure the roofline kernel live) ----
class _Timer:
    def __init__(self):
        self.enabled = False
        self.only = None  # optional set of op names to time (keeps the event overhead off everything else)
        self.records = {}

    def start(self, name):
        if not self.enabled or (self.only is not None and name not in self.only):
            return None
        import torch

        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        return (name, a, b)

    def stop(self, tok):
        if tok is None:
            return
        name, a, b = tok
        b.record()
        self.records.setdefault(name, []).append((a, b))

    def summary(self, reset=True):
        import torch

        torch.cuda.synchronize()
        out = {k: [a.elapsed_time(b) for a, b in v] for k, v in self.records.items()}
        if reset:
            self.records = {}
        return out


timer = _Timer()


def kernel_profile(enable=None, reset=False):
    """Per-kernel device timing of the library itself (hipEvent pairs on the launch stream).  kernel_profile(True) starts,
    kernel_profile() returns {"kernel": {"calls", "avg_us", "total_us"}} so far, kernel_profile(False) stops."""
    import json

    if reset:
        check(lib.nerftex_profile_reset())
    if enable is not None:
        check(lib.nerftex_profile_enable(int(enable)))  # 0 off, 1 / True every kernel, 2 hash-grid kernels only
        return None
    buf = C.create_string_buffer(1 << 16)
    check(lib.nerftex_profile_report(buf, len(buf)))
    return json.loads(buf.value.decode() or "{}")
