"""CPU: an inventory of include/oneshotdet_hip.h — every declared osd_* function either names a test that calls it (directly or
through its `ops` wrapper) or is listed, with a reason, as a function that launches nothing.  A new entry point without a row
fails here; so does a row whose function left the header or whose test no longer exists.  The entries of NAMED are held to more:
the test's body names the function, and the `ops` wrapper that reaches it is itself called on the GPU."""
import os
import re

from abi_utils import declared

TESTS = os.path.dirname(os.path.abspath(__file__))


K, T, S = "test_gpu_kernels.py", "test_gpu_train.py", "test_gpu_support_kernels.py"
PR, BH, BT = "test_gpu_proposals.py", "test_gpu_box_head.py", "test_gpu_box_train.py"
EV, TR, G1, FL, QA = "test_gpu_evaluation.py", "test_gpu_transforms.py", "test_gpu_groupnorm_onepass.py", "test_gpu_fcos_loss_modes.py", \
    "test_gpu_query_avgpool.py"
NS = "test_gpu_box_neg_support.py"
SO, CS, GA, PB = "test_gpu_solver.py", "test_gpu_class_sweep.py", "test_gpu_gallery.py", "test_gpu_pred_bwd.py"
_QP = (K, "test_query_pool_levels_equals_the_per_level_launches")
_PRED = (K, "test_prediction_conv_data_gradient_as_a_gemm_over_the_gathered_dy")

# function -> (test file, test function) that runs it on the GPU and checks what it computed
COVERED = {
    "osd_conv_algo_count": (S, "test_conv_algo_count_bounds_the_selectable_algorithms"),
    "osd_conv2d_fwd": (K, "test_conv2d_bias_matches_torch"),
    "osd_conv2d_fwd_grouped": (K, "test_conv2d_grouped_equals_per_level_launches"),
    "osd_conv2d_fwd_multi": (K, "test_conv2d_multi_own_weights_strides_and_topdown_add"),
    "osd_conv2d_fwd_multi_gn": (T, "test_groupnorm_forward_statistics_gathered_by_the_tower_conv"),
    "osd_pack_conv_weight": (K, "test_conv2d_bias_matches_torch"),
    "osd_pack_conv_weight_ex": (S, "test_single_conv_packers_are_one_multiplication_and_one_rounding"),
    "osd_pack_multi": (S, "test_pack_multi_every_path_is_exact_and_equals_the_single_conv_packer"),
    "osd_pack_stem_weight": (K, "test_stem_conv_and_maxpool"),
    "osd_pack_image": (TR, "test_collate_writes_the_padded_batch_and_the_stem_input"),
    "osd_nhwc_to_nchw_f32": (S, "test_layout_changes_are_a_rounding_and_a_copy"),
    "osd_nchw_f32_to_nhwc": (S, "test_layout_changes_are_a_rounding_and_a_copy"),
    "osd_maxpool3x3s2_fwd": (K, "test_stem_conv_and_maxpool"),
    "osd_groupnorm_stats": (K, "test_groupnorm_relu"),
    "osd_groupnorm_finalize": (K, "test_groupnorm_relu"),
    "osd_groupnorm_relu_apply": (K, "test_groupnorm_relu"),
    "osd_roialign_fwd": (K, "test_roi_align_reference_vectors"),
    "osd_shot_mean": (K, "test_shot_mean"),
    "osd_query_pool_levels": _QP,
    "osd_query_pool_levels_bwd": _QP,
    "osd_query_avgpool_levels": (QA, "test_forward_kernel_matches_torch_bitwise_reproducible_and_batch_invariant"),
    "osd_query_avgpool_levels_bwd": (QA, "test_backward_kernel_closed_form_and_bf16_cast"),
    "osd_correlate_fwd": (K, "test_correlate_matches_broadcast_multiply"),
    "osd_correlate_levels": (K, "test_correlate_levels_forward_and_query_gradient"),
    "osd_correlate_bwd_query": (K, "test_correlate_levels_forward_and_query_gradient"),
    "osd_correlate_bwd_query_levels": (K, "test_correlate_levels_forward_and_query_gradient"),
    "osd_fcos_score_decode": (S, "test_fcos_score_decode_two_levels_into_one_buffer"),
    "osd_fcos_score_decode_sizes": (S, "test_fcos_score_decode_two_levels_into_one_buffer"),
    "osd_level_topk": (S, "test_level_topk_keeps_the_topn_by_key_then_index"),
    "osd_rank_sort_gather": (PR, "test_rank_sort_gather_against_a_plain_sort"),
    "osd_nms_sorted": (PR, "test_proposals_sort_nms_equals_the_two_call_pipeline"),
    "osd_nms": (PR, "test_osd_nms_single_entry_matches_the_oracle_for_any_scores"),
    "osd_proposals_sort_nms": (PR, "test_proposals_sort_nms_equals_the_two_call_pipeline"),
    "osd_proposals_sort_nms_hint": (PR, "test_proposal_depth_feedback_tracks_a_deepening_scan"),
    "osd_sigmoid_focal_fwd": (K, "test_sigmoid_focal_loss_fwd_bwd"),
    "osd_sigmoid_focal_bwd": (K, "test_sigmoid_focal_loss_fwd_bwd"),
    "osd_pack_conv_weight_dgrad": (S, "test_single_conv_packers_are_one_multiplication_and_one_rounding"),
    "osd_conv2d_wgrad": (T, "test_conv_wgrad_batched_equals_one_launch_per_conv"),
    "osd_conv2d_wgrad_grouped": (T, "test_prediction_conv_wgrad_levels_read_once_kernel"),
    "osd_conv2d_wgrad_pred": (T, "test_prediction_conv_wgrad_levels_read_once_kernel"),
    "osd_pred_dy_gather": _PRED,
    "osd_pred_dgrad_pack": _PRED,
    "osd_conv2d_wgrad_pred_gathered": _PRED,
    "osd_conv2d_wgrad_batched": (T, "test_conv_wgrad_batched_equals_one_launch_per_conv"),
    "osd_conv2d_wgrad_multi": (T, "test_conv_wgrad_multi_mixes_shared_and_own_weights"),
    "osd_conv2d_wgrad_mixed": (T, "test_conv_wgrad_mixed_geometries_in_one_launch"),
    "osd_unpack_wgrad": (S, "test_unpack_wgrad_writes_and_accumulates_exactly"),
    "osd_bias_grad": (S, "test_bias_grad_accumulates_the_column_sums"),
    "osd_conv2d_dgrad_naive": (S, "test_conv2d_dgrad_naive_masks_then_adds"),
    "osd_scatter2x": (S, "test_scatter2x_adds_then_masks"),
    "osd_add_mask": (S, "test_add_mask_every_operand_combination_in_place_and_past_the_grid"),
    "osd_upsample2x_bwd": (S, "test_upsample2x_bwd_sums_the_2x2_block"),
    "osd_roialign_bwd": _QP,
    "osd_shot_mean_bwd": _QP,
    "osd_cast_f32": _QP,
    "osd_grad_wire_cast": (T, "test_gradient_buckets_cover_the_flat_buffer_and_overlapped_exchange_runs"),
    "osd_sgd_momentum_multi": (S, "test_sgd_momentum_multi_matches_the_float64_update"),
    "osd_sgd_momentum_pack_multi": (S, "test_sgd_momentum_pack_multi_update_packed_weights_and_consumed_gradients"),
    "osd_groupnorm_relu_fwd_levels": (S, "test_plain_groupnorm_level_entries_are_the_fused_entries_with_no_fused_level"),
    "osd_groupnorm_relu_bwd_levels": (S, "test_plain_groupnorm_level_entries_are_the_fused_entries_with_no_fused_level"),
    "osd_groupnorm_relu_fwd_levels_fused": (T, "test_groupnorm_forward_statistics_gathered_by_the_tower_conv"),
    "osd_groupnorm_relu_bwd_levels_fused": (T, "test_groupnorm_backward_statistics_gathered_by_the_data_gradient_conv"),
    "osd_groupnorm_relu_bwd_levels_convbias": (T, "test_groupnorm_backward_also_gives_the_producing_convs_bias_gradient"),
    "osd_groupnorm_relu_fwd_levels_onepass": (G1, "test_onepass_groupnorm_hands_maps_too_large_for_one_resident_job_to_the_two_launch_kernels"),
    "osd_groupnorm_relu_bwd_levels_onepass": (G1, "test_onepass_groupnorm_backward_on_the_same_statistics_is_the_two_launch_backward"),
    "osd_fcos_loss_level": (FL, "test_old_entries_are_the_new_ones_in_the_default_mode"),
    "osd_fcos_loss_levels": (FL, "test_old_entries_are_the_new_ones_in_the_default_mode"),
    "osd_fcos_loss_level_opt": (FL, "test_losses_and_gradients_match_the_reference"),
    "osd_fcos_loss_levels_opt": (FL, "test_losses_and_gradients_match_the_reference"),
    "osd_fcos_loss_finalize": (FL, "test_losses_and_gradients_match_the_reference"),
    "osd_fcos_loss_finalize_scales": (S, "test_fcos_loss_finalize_scales_is_finalize_plus_the_scale_gradient"),
    "osd_roi_pool_levels": (BH, "test_roi_pool_levels_matches_oracle"),
    "osd_groupnorm_act_rois": (BH, "test_groupnorm_leaky_rois_matches_aten"),
    "osd_box_decode": (BH, "test_box_decode_matches_oracle"),
    "osd_append_gt_boxes": (PR, "test_append_gt_boxes_matches_reference_vectors"),
    "osd_box_match_sample": (BT, "test_match_sample_equals_the_reference_fixture"),
    "osd_box_loss": (BT, "test_box_loss_values_and_gradient"),
    "osd_groupnorm_act_rois_bwd": (BT, "test_groupnorm_leakyrelu_rois_backward"),
    "osd_rois_sum": (BT, "test_groupnorm_leakyrelu_rois_backward"),
    "osd_roi_pool_levels_bwd": (BT, "test_roi_pool_levels_backward_matches_oracle_autograd"),
    "osd_voc_match": (EV, "test_voc_match_flags_equal_the_oracle_per_image"),
    "osd_voc_curves": (EV, "test_voc_ap_equals_the_reference_fixture"),
    "osd_voc_ap": (EV, "test_voc_ap_from_curve_lists_long_classes_and_missing_curves"),
    "osd_coco_match": (EV, "test_coco_match_flags_equal_the_oracle_per_pair_and_edge_cases"),
    "osd_image_transform": (TR, "test_random_sizes_against_the_oracle"),
    "osd_image_transform_batch": (TR, "test_batched_chain_equals_the_per_image_one_for_mixed_batches"),
    "osd_box_loss_neg_support": (NS, "test_c_entry_with_padded_strides_null_gradients_bad_labels_and_error_codes"),
    "osd_solver_set": (SO, "test_solver_set_writes_its_eight_bytes_and_bad_blocks_are_refused"),
    "osd_sgd_momentum_multi_dev": (SO, "test_dev_entries_match_the_by_value_entries_bit_for_bit"),
    "osd_sgd_momentum_pack_multi_dev": (SO, "test_dev_entries_match_the_by_value_entries_bit_for_bit"),
    "osd_correlate_levels_sweep": (CS, "test_sweep_correlation_is_the_per_pair_launch_on_replicated_maps_bit_for_bit"),
    "osd_roi_pool_levels_sweep": (CS, "test_sweep_roi_pooling_is_the_per_pair_launch_on_replicated_maps_bit_for_bit"),
    "osd_correlate_levels_gallery": (GA, "test_gallery_correlation_is_the_sweep_launch_on_gathered_vectors_bit_for_bit"),
    "osd_groupnorm_act_rois_gallery": (GA, "test_gallery_groupnorm_is_the_existing_entry_on_a_gathered_addend_bit_for_bit"),
    "osd_conv2d_pred_bwd": (PB, "test_unsupported_shapes_return_the_documented_codes"),
    "osd_pred_bwd_workspace_bytes": (PB, "test_unsupported_shapes_return_the_documented_codes"),
}

_LOSS = "test_loss_kernel_matches_the_reference_fixture"
# function -> (what the body of its COVERED test must contain, the `ops` wrapper that reaches it, what the wrapper's body must contain,
#              the test of the same file that calls the wrapper (None: anywhere in the file), what that test must contain)
NAMED = {
    "osd_box_loss_neg_support": ('"osd_box_loss_neg_support"', "box_loss_neg_support", '"osd_box_loss_neg_support"', _LOSS,
                                 ("ops.box_loss_neg_support(", "grad_stride=")),
    "osd_solver_set": ('"osd_solver_set"', "solver_set", '"osd_solver_set"', None, ("ops.solver_set(",)),
    "osd_sgd_momentum_multi_dev": ('"osd_sgd_momentum_multi_dev"', "sgd_momentum_multi_dev", '"osd_sgd_momentum_multi_dev"', None,
                                   ("ops.sgd_momentum_multi_dev(",)),
    "osd_sgd_momentum_pack_multi_dev": ('"osd_sgd_momentum_pack_multi_dev"', "sgd_momentum_pack_multi_dev",
                                        '"osd_sgd_momentum_pack_multi_dev"', None, ("ops.sgd_momentum_pack_multi_dev(",)),
    # called through the bound library (lib.<name>(...)), not by name through _lib.call
    "osd_conv2d_pred_bwd": ("osd_conv2d_pred_bwd", "pred_bwd_fused", '"osd_conv2d_pred_bwd"', None, ("o.pred_bwd_fused(",)),
    "osd_pred_bwd_workspace_bytes": ("osd_pred_bwd_workspace_bytes", "pred_bwd_fused", "osd_pred_bwd_workspace_bytes(", None,
                                     ("o.pred_bwd_fused(",)),
}

# functions that launch no kernel of their own to compare with a reference
NO_LAUNCH = {
    "osd_last_error_string": "returns the calling thread's last error message",
    "osd_abi_version": "returns a constant (checked on the CPU by test_abi.py)",
    "osd_class_sweep_group": "returns a constant (checked against its #define on the CPU by test_abi.py)",
    "osd_query_avgpool_workspace_bytes": "host-side size query",
    "osd_nms_workspace_bytes": "host-side size query (value pinned by test_abi.py)",
    "osd_nms_single_workspace_bytes": "host-side size query",
    "osd_proposals_workspace_bytes": "host-side size query",
    "osd_conv2d_wgrad_pred_workspace_bytes": "host-side size query",
    "osd_groupnorm_onepass_workspace_bytes": "host-side size query",
    "osd_groupnorm_onepass_sync_bytes": "host-side size query",
    "osd_image_transform_workspace_bytes": "host-side size query",
    "osd_groupnorm_onepass_selftest_timeout": "diagnostic entry that runs the one-pass kernel's failure path; it has no result to compare",
}


def test_every_exported_function_names_a_test_or_a_reason():
    names = set(declared())
    listed = set(COVERED) | set(NO_LAUNCH)
    assert not (set(COVERED) & set(NO_LAUNCH))
    assert names - listed == set(), "entry points without a test: add one and a row to COVERED"
    assert listed - names == set(), "rows for functions the header no longer declares"
    assert all(reason.strip() for reason in NO_LAUNCH.values())
    sources = {}
    for name, (fname, test) in sorted(COVERED.items()):
        if fname not in sources:
            sources[fname] = open(os.path.join(TESTS, fname)).read()
        assert re.search(r"^def %s\(" % re.escape(test), sources[fname], flags=re.M), "%s: %s has no %s" % (name, fname, test)


def body(src, test):
    m = re.search(r"^def %s\(.*?(?=^def |^@pytest|\Z)" % re.escape(test), src, flags=re.S | re.M)
    assert m, test
    return m.group(0)


def test_named_entries_are_called_by_their_test_and_through_their_ops_wrapper():
    assert set(NAMED) <= set(COVERED)
    ops_src = open(os.path.join(os.path.dirname(TESTS), "oneshotdet_amd", "ops.py")).read()
    for fn, (needle, wrapper, wrapper_needle, through, also) in NAMED.items():
        fname, test = COVERED[fn]
        src = open(os.path.join(TESTS, fname)).read()
        assert "pytestmark = pytest.mark.gpu" in src, fname
        assert needle in body(src, test), (fn, test)
        wbody = re.search(r"^def %s\(.*?(?=^def |\Z)" % wrapper, ops_src, flags=re.S | re.M).group(0)
        assert wrapper_needle in wbody, (fn, wrapper)
        where = body(src, through) if through else src
        for word in also:
            assert word in where, (fn, through, word)
