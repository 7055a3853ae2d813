"""ctypes binding of libunet_hip.so (include/unet_hip.h) — the only way the host reaches the GPU path.

There is deliberately no CPU fallback: if the shared library is missing or a tensor is not on a
HIP device, the call raises.  torch is used for device memory and streams only.
"""
import ctypes as C
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("UNET_SO") or os.path.join(_HERE, "libunet_hip.so")
_lib = None

N_PARAMS = 46
MAX_CLASSES = 16        # UNET_MAX_CLASSES

vp = C.c_void_p
_SIGS = {
    "unet_last_error": (C.c_char_p, []),
    "unet_abi_version": (C.c_int, []),
    "unet_set_math": (C.c_int, [C.c_int]),
    "unet_get_math": (C.c_int, []),
    "unet_set_lds_dma": (C.c_int, [C.c_int]),
    "unet_set_grad_scale": (C.c_int, [vp, C.c_float]),
    "unet_set_overlap": (C.c_int, [C.c_int]),
    "unet_dp_unique_id": (C.c_int, [vp]),
    "unet_dp_init": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "unet_dp_destroy": (C.c_int, [vp]),
    "unet_dp_world": (C.c_int, [vp]),
    "unet_dp_rccl_version": (C.c_int, []),
    "unet_dp_allreduce": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "unet_dp_broadcast": (C.c_int, [vp, vp, C.c_size_t, C.c_int, vp]),
    "unet_dp_join": (C.c_int, [vp, vp]),
    "unet_create": (C.c_int, [C.POINTER(vp), vp]),
    "unet_create_classes": (C.c_int, [C.POINTER(vp), vp, C.c_int]),
    "unet_n_classes": (C.c_int, [vp]),
    "unet_destroy": (C.c_int, [vp]),
    "unet_output_size": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "unet_param_count": (C.c_int, [vp, C.c_int, C.POINTER(C.c_size_t)]),
    "unet_workspace_bytes": (C.c_size_t, [vp, C.c_int, C.c_int, C.c_int]),
    "unet_forward": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, vp]),
    "unet_forward_dropout": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_float, C.c_ulonglong, C.c_ulonglong, vp]),
    "unet_dropout_mask": (C.c_int, [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_size_t, C.c_size_t, C.c_float, vp, vp]),
    "unet_backward": (C.c_int, [vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "unet_backward_stages": (C.c_int, []),
    "unet_backward_stage": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_size_t, vp]),
    "unet_backward_stage_params": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int]),
    "unet_backward_input": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp]),
    "unet_flops": (C.c_double, [vp, C.c_int, C.c_int, C.c_int]),
    "unet_activation_bytes": (C.c_int, [vp]),
    "unet_debug_buffer": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "unet_profile_enable": (C.c_int, [C.c_int]),
    "unet_profile_select": (C.c_int, [C.c_uint]),
    "unet_profile_reset": (C.c_int, []),
    "unet_profile_read": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "unet_profile_dump": (C.c_int, [C.c_char_p]),
    "unet_bce_scratch_bytes": (C.c_size_t, [C.c_size_t]),
    "unet_bce_logits": (C.c_int, [vp, vp, vp, C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int,
                                  vp, vp, C.c_float, vp, vp]),
    "unet_bce_step_scratch_bytes": (C.c_size_t, [C.c_size_t]),
    "unet_bce_step": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, vp, vp, C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int,
                                vp, vp, C.c_float, vp, vp, vp]),
    "unet_onehot2": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "unet_argmax2": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, vp, C.c_int, C.c_int, C.c_int, vp]),
    "unet_softmax_ce_scratch_bytes": (C.c_size_t, [C.c_size_t]),
    "unet_softmax_ce_step": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, C.c_int, vp, vp, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int,
                                       C.c_int, vp, vp, C.c_float, vp, vp, vp, vp]),
    "unet_dice_scratch_bytes": (C.c_size_t, [C.c_int] * 4),
    "unet_dice_step": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, C.c_int, vp, vp, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int,
                                 C.c_float, C.c_float, C.c_float, C.c_int, vp, vp, vp, C.c_float, vp, vp, vp, vp]),
    "unet_argmaxk": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "unet_sgd_momentum": (C.c_int, [vp, vp, vp, C.POINTER(C.c_size_t), C.c_int, C.c_float, C.c_float, C.c_int, vp]),
    "unet_adam_step": (C.c_int, [vp, vp, vp, vp, C.POINTER(C.c_size_t), C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                 C.c_int, C.c_long, vp, vp]),
    "unet_grad_sumsq_partials": (C.c_size_t, [C.POINTER(C.c_size_t), C.c_int]),
    "unet_grad_sumsq": (C.c_int, [vp, C.POINTER(C.c_size_t), C.c_int, vp, C.c_size_t, vp]),
    "unet_grad_norm_finish": (C.c_int, [vp, C.c_size_t, C.c_float, vp, vp]),
    "unet_grads_scale": (C.c_int, [vp, C.POINTER(C.c_size_t), C.c_int, vp, vp]),
    "unet_minmax": (C.c_int, [vp, C.c_int, C.c_size_t, vp, vp]),
    "unet_mirror_pad": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_tile_gather": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long,
                                   C.c_int, vp, vp]),
    "unet_tile_stitch": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int,
                                   vp, vp, vp]),
    "unet_tile_stitch_k": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int,
                                     C.c_int, vp, vp, vp]),
    "unet_tile_gather_view": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_long, C.c_int, vp, vp]),
    "unet_tile_stitch_view": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_eval_masks": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]),
    "unet_eval_confusion": (C.c_int, [vp, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp]),
    "unet_class_balance": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_weighted_map_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_weighted_map": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    "unet_label_components_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_label_components": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_label_components_conn_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_label_components_conn": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_clean_mask_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_clean_mask": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int,
                                  vp, vp, vp, vp, vp]),
    "unet_cell_sums_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "unet_cell_sums": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unet_remap_labels": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_longlong, vp, vp, vp]),
    "unet_cell_hulls_scratch_bytes": (C.c_size_t, [C.c_longlong]),
    "unet_cell_hulls": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_longlong, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unet_cell_contacts_scratch_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "unet_cell_contacts": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp]),
    "unet_mask_boundary": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "unet_surface_sums_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_surface_sums": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                    C.c_longlong, C.POINTER(C.c_int), C.c_int, vp, vp, vp, vp, vp]),
    "unet_instance_overlap_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_size_t]),
    "unet_instance_overlap": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]),
    "unet_partition_pairs_scratch_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "unet_partition_pairs": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp]),
    "unet_link_frames_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_size_t]),
    "unet_link_frames": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp, vp, vp]),
    "unet_aogm_counts_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_aogm_counts": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unet_grow_labels_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_grow_labels": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_longlong, vp, vp, vp]),
    "unet_warp_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_warp_init": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, vp, vp, vp, vp]),
    "unet_warp_sweeps": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_warp_finish": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_geodesic_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_geodesic_init": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_geodesic_sweeps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, vp, C.c_int, vp, vp]),
    "unet_geodesic_sweeps_conn": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_geodesic_finish": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, vp, vp, vp, vp, vp, vp]),
    "unet_flood_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_flood_init": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_flood_sweeps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, vp, C.c_int, vp, vp]),
    "unet_flood_sweeps_conn": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_flood_assign": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_flood_assign_conn": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_flood_finish": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "unet_distance_map_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_distance_map": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_reconstruct_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_reconstruct_init": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_reconstruct_sweeps": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_reconstruct_sweeps_conn": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
    "unet_reconstruct_finish": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_shape_heights": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_shape_lower": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "unet_shape_maxima": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "unet_carve_borders":(C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "unet_crop_counts_scratch_bytes": (C.c_size_t, [C.c_int] * 5),
    "unet_crop_counts": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "unet_gaussian_filter": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_float, vp, vp, vp]),
    "unet_warp_bilinear": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "unet_rotate_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "unet_reflect_rotate_crop": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, vp, vp, vp]),
    "unet_elastic_grid": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_double, vp, vp]),
    "unet_elastic_grid_sample": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_normalise01": (C.c_int, [vp, C.c_int, C.c_size_t, vp, vp]),
    "unet_grey_scratch_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "unet_grey_vary": (C.c_int, [vp, vp, C.c_int, C.c_size_t, C.c_longlong, C.POINTER(C.c_double), vp, C.c_ulonglong, C.c_ulonglong,
                                 C.c_int, vp, vp]),
    "unet_grey_normals": (C.c_int, [C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_size_t, C.c_size_t, vp, vp]),
    "unet_conv3x3_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "unet_conv3x3_fwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                   vp, vp, C.c_int, C.c_int, vp, vp, vp]),
    "unet_conv3x3_bwd_scratch_bytes": (C.c_size_t, [C.c_int] * 5),
    "unet_conv3x3_bwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                   vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "unet_maxpool2_fwd": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "unet_maxpool2_bwd": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "unet_dropout_pool_fwd": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_ulonglong, C.c_ulonglong, C.c_int, vp]),
    "unet_dropout_bwd": (C.c_int, [vp, C.c_size_t, C.c_float, vp]),
    "unet_upconv2_scratch_bytes": (C.c_size_t, [C.c_int] * 5),
    "unet_upconv2_fwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp]),
    "unet_upconv2_bwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "unet_head1x1_fwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_head1x1_bwd_scratch_bytes": (C.c_size_t, [C.c_int] * 4),
    "unet_head1x1_bwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "unet_head1xk_fwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "unet_head1xk_bwd_scratch_bytes": (C.c_size_t, [C.c_int] * 5),
    "unet_head1xk_bwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "unet_conv1ch_fwd": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp]),
    "unet_conv1ch_bwd_scratch_bytes": (C.c_size_t, [C.c_int] * 3),
    "unet_conv1ch_bwd": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "unet_conv1ch_dgrad": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
}
EXPORTS = tuple(_SIGS.keys())


class UnetConfig(C.Structure):
    _fields_ = [("base_ch", C.c_int), ("device", C.c_int), ("math", C.c_int)]


def build(force=False):
    """Compile libunet_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force and os.path.exists(_SO):
        os.remove(_SO)
    subprocess.check_call(["make", "-s", "-C", csrc, "-j4"])
    return _SO


def lib():
    """Load the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(
                "libunet_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C dl-unet_amd/csrc`. There is no CPU fallback for the HIP path." % _SO)
        L = C.CDLL(_SO)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().unet_last_error().decode("utf-8", "replace")
        raise RuntimeError("%s failed (rc=%d): %s" % (what or "libunet_hip", rc, msg))


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL). Refuses host tensors loudly."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("the HIP path needs tensors on a HIP device (got %s); there is no CPU fallback" % t.device)
    return C.c_void_p(t.data_ptr())


def stream(device=None):
    """The current HIP stream of `device` (default: the current device) as a void*."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def run(name, device, *args):
    """lib().<name>(*args, stream): `device` is made current for the call (everything the library keeps per device —
    zero page, kernel attributes — is keyed on the current device) and the work goes to that device's current stream."""
    with torch.cuda.device(device):
        check(getattr(lib(), name)(*args, stream(device)), name)


def scratch(name, device, *dims):
    """The uint8 scratch tensor an entry point asks for: lib().<name>_scratch_bytes(*dims) bytes on `device`."""
    return torch.empty(getattr(lib(), name + "_scratch_bytes")(*dims), dtype=torch.uint8, device=device)


def ptr_table(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        if not t.is_cuda:
            raise RuntimeError("parameter %d is on %s; move the module to a HIP device" % (i, t.device))
        arr[i] = t.data_ptr()
    return arr


class Handle:
    """RAII wrapper of unet_handle (one per device / module)."""

    def __init__(self, base_ch=64, device=0, math=-1, n_classes=2):
        """math: arithmetic mode of this handle (include/unet_hip.h unet_set_math codes); -1 follows unet_set_math.
        n_classes: output channels of the head, 2 (unet_create, the reference's net) .. MAX_CLASSES (unet_create_classes)."""
        self._h = C.c_void_p()
        cfg = UnetConfig(base_ch, device, math)
        if n_classes == 2:
            check(lib().unet_create(C.byref(self._h), C.byref(cfg)), "unet_create")
        else:
            check(lib().unet_create_classes(C.byref(self._h), C.byref(cfg), int(n_classes)), "unet_create_classes")
        self.base_ch = base_ch
        self.device = device
        self.math = math
        self.n_classes = n_classes

    def __del__(self):
        try:
            if self._h:
                lib().unet_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def h(self):
        return self._h

    def workspace_bytes(self, B, S, training):
        n = lib().unet_workspace_bytes(self._h, B, S, int(training))
        if n == 0:
            check(-1, "unet_workspace_bytes")
        return n

    def buffer_view(self, ws, B, S, training, name):
        """NHWC [B,e,e,C] float32 view of a named plan buffer inside workspace tensor `ws` (debug/tests)."""
        off, e, c = C.c_size_t(), C.c_int(), C.c_int()
        check(lib().unet_debug_buffer(self._h, B, S, int(training), name.encode(), C.byref(off), C.byref(e), C.byref(c)),
              "unet_debug_buffer")
        n = B * e.value * e.value * c.value
        eb = 4 if name == "xin" else lib().unet_activation_bytes(self._h)          # bf16 tensors in arithmetic mode 2
        return ws[off.value:off.value + eb * n].view(torch.bfloat16 if eb == 2 else torch.float32).view(B, e.value, e.value, c.value)

    def flops(self, B, S, backward):
        return lib().unet_flops(self._h, B, S, int(backward))
