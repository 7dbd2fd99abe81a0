"""ctypes binding of libt2s_hip.so (the C ABI declared in include/t2s_hip.h).

The product path has NO fallback: if the library is missing or an entry point
fails, a ``T2SError`` is raised.  PyTorch is used only for device memory and
streams; every pointer handed to the library is ``tensor.data_ptr()``.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("T2S_LIB_PATH") or os.path.join(HERE, "libt2s_hip.so")      # (override: diagnostic builds)

c_int, c_float, c_vp, c_long = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_long
c_double = ctypes.c_double

# name -> argtypes (every function returns int unless listed in _RESTYPE)
SIGNATURES = {
    "t2s_abi_version": [],
    "t2s_operand_format": [],
    "t2s_sizeof_taco_decoder": [],
    "t2s_sizeof_taco_bptt": [],
    "t2s_error_string": [c_int],
    "t2s_last_hip_error": [],
    "t2s_plane_rows": [c_int, c_int],
    "t2s_padded_rows": [c_int],
    "t2s_pack_conv_weight": [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                             c_vp, c_vp, c_vp, c_int, c_vp],
    "t2s_pack_conv_weight_table": [c_vp, c_int, c_long, c_vp],
    "t2s_weightnorm_small": [c_vp, c_vp, c_int, c_int, c_vp, c_vp],
    "t2s_wg_upsample_squeeze": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_vp, c_vp, c_vp],
    "t2s_wg_audio_squeeze": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_wg_convinv": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_small_logdet_inv": [c_vp, c_int, c_float, c_vp, c_vp, c_vp],
    "t2s_small_logdet_inv_batch": [c_vp, c_int, c_float, c_vp],
    "t2s_small_logdet_inv_batch_host": [c_vp, c_int, c_float, c_vp],
    "t2s_wg_start": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp],
    "t2s_wg_in_cond_gate": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int,
                            c_int, c_int, c_int, c_int, c_vp],
    "t2s_wg_res_skip": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                        c_int, c_int, c_vp],
    "t2s_wg_endfold_weights": [c_vp, c_int, c_int, c_vp],
    "t2s_wg_in_cond_gate_fold": [c_vp] * 11 + [c_int] * 10 + [c_vp],
    "t2s_wg_start_window": [c_vp, c_vp, c_vp] + [c_int] * 8 + [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp],
    "t2s_wg_startfold_weights": [c_vp] * 4 + [c_int] * 5 + [c_vp, c_vp, c_vp],
    "t2s_wg_in_win_gate_fold": [c_vp] * 11 + [c_int] * 9 + [c_vp],
    "t2s_wg_gate_fold_slots": [c_int, c_int, c_int],
    "t2s_wg_gate_tile_rows": [c_int, c_int, c_int],
    "t2s_wg_upsample_basis": [c_vp, c_vp] + [c_int] * 6 + [c_vp, c_vp, c_vp],
    "t2s_wg_compose_cond": [c_vp, c_vp] + [c_int] * 4 + [c_long, c_vp, c_vp, c_vp, c_vp],
    "t2s_wg_melwin_planes": [c_vp] + [c_int] * 5 + [c_vp, c_vp, c_vp],
    "t2s_wg_in_melwin_gate_fold": [c_vp] * 13 + [c_int] * 12 + [c_vp],
    "t2s_wg_res_only": [c_vp] * 7 + [c_int] * 7 + [c_vp],
    "t2s_wg_res_only_start": [c_vp] * 8 + [c_int] * 3 + [c_vp, c_vp] + [c_int] * 6 + [c_vp],
    "t2s_wg_flow_boundary": [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp] + [c_int] * 10 + [c_vp, c_vp, c_vp],
    "t2s_wg_start_ragged": [c_vp, c_vp, c_vp] + [c_int] * 8 + [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp],
    "t2s_wg_res_only_ragged": [c_vp] * 7 + [c_int] * 7 + [c_vp, c_vp],
    "t2s_wg_res_only_start_ragged": [c_vp] * 8 + [c_int] * 3 + [c_vp, c_vp] + [c_int] * 6 + [c_vp, c_vp],
    "t2s_wg_flow_boundary_ragged": [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp] + [c_int] * 10 + [c_vp, c_vp, c_vp, c_vp],
    "t2s_wg_end_fold_affine": [c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_wg_end_affine": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                          c_int, c_vp],
    "t2s_conv_bias_act": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                          c_int, c_int, c_int, c_int, c_vp],
    "t2s_gemv": [c_vp, c_int, c_int, c_vp, c_int, c_int, c_vp, c_int, c_long, c_vp, c_int, c_long, c_vp, c_int, c_long,
                 c_vp, c_vp, c_vp, c_long, c_long, c_int, c_int, c_int, c_vp, c_long, c_float, c_vp],
    "t2s_transpose": [c_vp, c_vp, c_int, c_int, c_vp],
    "t2s_embed_planes": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp],
    "t2s_f32_to_planes": [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp],
    "t2s_taco_parse_output": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp],
    "t2s_zero_plane_rows": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_zero_rows_f32": [c_vp, c_vp, c_int, c_int, c_int, c_vp],
    "t2s_bn_fold": [c_vp, c_vp, c_vp, c_vp, c_vp, c_float, c_int, c_vp, c_vp, c_vp],
    "t2s_bn_train": [c_vp, c_vp, c_vp, c_float, c_int, c_vp, c_float, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                     c_vp, c_vp, c_vp],
    "t2s_taco_encoder_lstm": [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp],
    "t2s_taco_encoder_lstm_bwd": [c_vp] * 9 + [c_int] * 4 + [c_vp],
    "t2s_taco_encoder_lstm_split": [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, ctypes.c_uint, c_vp],
    "t2s_taco_lstm_xbuf_bytes": [c_int],
    "t2s_taco_encoder_lstm_bwd_split": [c_vp] * 9 + [c_int] * 4 + [c_vp, ctypes.c_uint, c_vp],
    "t2s_rows_to_planes": [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp],
    "t2s_embedding_grad": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "t2s_bn_running_update": [c_vp, c_vp, c_vp, c_vp, c_vp, c_float, ctypes.c_longlong, c_int, c_vp],
    "t2s_zero_fill": [c_vp, ctypes.c_size_t, c_vp],
    "t2s_wg_bwd_pair8_ok": [c_int, c_int, c_int],
    "t2s_taco_attention": [c_vp] * 14 + [c_int] * 7 + [c_vp],
    "t2s_bernoulli_mask": [c_vp, ctypes.c_size_t, ctypes.c_ulonglong, ctypes.c_ulonglong, c_float, c_vp],
    "t2s_taco_decode_steps": [c_vp, c_int, c_int, c_vp],
    "t2s_taco_decode_plan": [c_vp, c_int, c_int, c_vp],
    "t2s_taco_decode_steps_w16": [c_vp, c_vp, c_int, c_int, c_vp],
    "t2s_taco_decode_plan_w16": [c_vp, c_vp, c_int, c_int, c_vp, c_vp],
    "t2s_taco_stop_check": [c_vp, c_int, c_int, c_int, c_int, c_int, c_float, c_vp, c_vp],
    "t2s_rows_to_tm": [c_vp, c_long, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp],
    "t2s_rows_to_tm_batched": [c_vp, c_long, c_long, c_int, c_int, c_int, c_int, c_vp, c_vp, c_long, c_int, c_int, c_int, c_vp],
    "t2s_lstm_cell_bwd": [c_vp, c_long, c_vp, c_long, c_vp, c_long, c_vp, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                          c_vp],
    "t2s_relu_drop_bwd": [c_vp, c_vp, c_float, ctypes.c_size_t, c_vp, c_vp],
    "t2s_taco_att_bwd": [c_vp, c_vp],
    "t2s_taco_bptt_steps": [c_vp, c_int, c_int, c_vp],
    "t2s_bn_bwd": [c_vp, c_vp, c_vp],
    "t2s_waveglow_loss": [c_vp, ctypes.c_size_t, c_vp, c_vp, c_int, c_vp, c_float, c_vp, c_vp, c_vp, c_vp],
    "t2s_taco_loss": [c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp, c_vp, ctypes.c_size_t, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "t2s_stft_transform": [c_vp, c_int, c_int, c_vp, c_int, c_int, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_long, c_vp],
    "t2s_mel_from_mag": [c_vp, c_long, c_int, c_int, c_vp, c_int, c_float, c_vp, c_vp],
    "t2s_stft_inverse": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_long, c_vp, c_float, c_vp, c_float, c_vp, c_vp, c_vp,
                         c_vp],
    "t2s_stft_transform_ragged": [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_long, c_vp, c_vp, c_vp, c_vp, c_long,
                                  c_vp],
    "t2s_mel_from_mag_ragged": [c_vp, c_long, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_float, c_vp, c_vp],
    "t2s_stft_inverse_ragged": [c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_long, c_vp, c_float, c_vp, c_float, c_vp,
                                c_vp, c_vp, c_vp],
    "t2s_pcm16": [c_vp, c_int, c_int, c_int, c_long, c_vp, c_vp, c_vp],
    "t2s_pcm16_gather": [c_vp, c_long, c_vp, c_int, c_int, c_float, c_vp, c_long, c_vp],
    "t2s_gate_targets": [c_vp, c_int, c_int, c_vp, c_vp],
    "t2s_resample_tile": [],
    "t2s_resample_table": [c_vp, c_int, c_long, c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_int, c_long, c_long, c_vp, c_vp],
    "t2s_resample_batch": [c_vp, c_int, c_int, c_int, c_long, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_long, c_vp, c_vp],
    "t2s_trim_tile": [],
    "t2s_trim_energy": [c_vp, c_int, c_long, c_vp, c_int, c_int, c_int, c_int, c_long, c_vp, c_long, c_vp, c_vp],
    "t2s_trim_bounds": [c_vp, c_int, c_int, c_long, c_int, c_int, c_int, c_long, c_vp, c_long, c_vp, c_double, c_int, c_double,
                        c_double, c_vp, c_vp],
    "t2s_trim_gather": [c_vp, c_int, c_long, c_vp, c_int, c_vp, c_vp, c_double, c_double, c_vp, c_int, c_long, c_long, c_vp, c_vp],
    "t2s_loud_tile": [],
    "t2s_loud_segment": [],
    "t2s_loud_scratch": [c_int, c_long],
    "t2s_loud_measure": [c_vp, c_int, c_long, c_vp, c_int, c_long, c_int, c_vp, c_vp, c_long, c_double, c_double, c_double, c_vp, c_vp,
                         c_vp],
    "t2s_loud_apply": [c_vp, c_int, c_long, c_vp, c_int, c_vp, c_vp, c_int, c_long, c_long, c_vp, c_vp],
    "t2s_limit_tile": [],
    "t2s_limit_max_lookahead": [],
    "t2s_limit_max_half_width": [],
    "t2s_limit_scratch": [c_int, c_long],
    "t2s_limit_measure": [c_vp, c_int, c_long, c_vp, c_int, c_long, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_double, c_vp, c_long,
                          c_vp, c_vp, c_vp],
    "t2s_limit_apply": [c_vp, c_int, c_long, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int, c_double, c_vp, c_vp, c_int, c_long,
                        c_long, c_vp, c_vp],
    "t2s_resample_window_carry": [c_int, c_int],
    "t2s_resample_window_end": [c_long, c_long, c_int, c_int, c_int, c_int],
    "t2s_resample_window": [c_vp, c_vp, c_vp, c_int, c_int, c_long, c_long, c_long, c_long, c_int, c_vp, c_int, c_int, c_int, c_vp, c_long,
                            c_long, c_vp],
    "t2s_limit_window_carry": [c_int, c_int],
    "t2s_limit_window_end": [c_long, c_long, c_int, c_int, c_int],
    "t2s_limit_window": [c_vp, c_vp, c_vp, c_int, c_int, c_long, c_long, c_long, c_long, c_int, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_int,
                         c_double, c_vp, c_long, c_long, c_vp, c_vp],
    "t2s_g711": [c_vp, c_long, c_int, c_vp, c_vp],
    "t2s_sos_tile": [],
    "t2s_sos_segment": [],
    "t2s_sos_max_sections": [],
    "t2s_sos_table_doubles": [],
    "t2s_sos_scratch": [c_int, c_long, c_int],
    "t2s_sos_filter": [c_vp, c_int, c_long, c_vp, c_int, c_long, c_vp, c_vp, c_int, c_vp, c_long, c_vp, c_int, c_long, c_long, c_vp, c_vp],
    "t2s_sos_window_carry": [c_int],
    "t2s_sos_window": [c_vp, c_vp, c_vp, c_int, c_int, c_long, c_long, c_long, c_vp, c_vp, c_int, c_vp, c_long, c_vp, c_long, c_vp, c_vp],
    "t2s_join_tile": [],
    "t2s_join_offsets": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_long, c_vp, c_vp, c_vp],
    "t2s_join_gather": [c_vp, c_int, c_int, c_int, c_long, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_long, c_vp],
    "t2s_align_rows": [c_vp, c_int, c_int, c_int, c_int, c_long, c_long, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "t2s_align_stats": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_double, c_vp, c_vp,
                        c_vp, c_vp, c_vp],
    "t2s_warp_block": [],
    "t2s_warp_map": [c_vp, c_int, c_int, c_long, c_vp, c_vp, c_long, c_vp, c_long, c_vp, c_int, c_double, c_double, c_int, c_vp, c_vp,
                     c_vp, c_vp],
    "t2s_warp_gather": [c_vp, c_int, c_int, c_int, c_int, c_long, c_long, c_vp, c_vp, c_vp, c_vp, c_int, c_vp],
    "t2s_warp_spans": [c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_long, c_long, c_long, c_vp, c_vp, c_vp],
    "t2s_align_window_state": [],
    "t2s_align_window": [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_long, c_long, c_vp, c_int, c_int, c_int, c_int, c_int,
                         c_double, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    "t2s_warp_window_map": [c_int, c_int, c_int, c_int, c_long, c_vp, c_vp, c_long, c_vp, c_int, c_vp, c_vp, c_vp],
    "t2s_warp_window_gather": [c_vp, c_int, c_int, c_int, c_int, c_int, c_long, c_long, c_vp, c_long, c_long, c_vp, c_vp],
    "t2s_bernoulli_mask_keyed": [c_vp, c_int, c_int, c_int, c_vp, c_float, c_vp],
    "t2s_noise_tile": [],
    "t2s_wg_noise_keyed": [c_vp, c_int, c_int, c_long, c_vp, c_float, c_vp, c_vp],
    "t2s_wg_noise_keyed_at": [c_vp, c_int, c_int, c_long, c_long, c_vp, c_vp, c_float, c_vp, c_vp],
    "t2s_wg_audio_window": [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_long, c_long, c_vp],
    "t2s_sum_axis0":[c_vp, c_int, c_int, c_vp, c_vp],
    "t2s_add3": [c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp, c_vp],
    "t2s_scale_by_scalar": [c_vp, ctypes.c_size_t, c_vp, c_float, c_vp, c_vp],
    "t2s_planes_to_f32": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp],
    "t2s_wg_in_cond_gate_train": [c_vp] * 13 + [c_int] * 9 + [c_vp],
    "t2s_wg_res_skip_train": [c_vp] * 10 + [c_int] * 8 + [c_vp],
    "t2s_wg_bwd_gate_dgrad": [c_vp] * 11 + [c_int] + [c_vp] * 2 + [c_int] * 8 + [c_vp],
    "t2s_wg_in_cond_gate_fold_train": [c_vp] * 11 + [c_int] + [c_vp] * 2 + [c_int] * 10 + [c_vp],
    "t2s_wg_res_only_train": [c_vp] * 5 + [c_int] + [c_vp] * 4 + [c_int] * 7 + [c_vp],
    "t2s_wg_skip_sum": [c_vp] * 5 + [c_int] * 2 + [c_vp] + [c_int] * 6 + [c_vp],
    "t2s_conv_accumulate": [c_vp] * 5 + [c_int] + [c_vp] * 2 + [c_int] * 11 + [c_vp],
    "t2s_wgrad_gemm": [c_vp] * 6 + [c_int] * 9 + [c_vp],
    "t2s_wgrad_gemm_flat": [c_vp] * 6 + [c_int] * 9 + [c_vp],
    "t2s_wgrad_cl": [c_vp, c_int, c_vp, c_int, c_vp] + [c_int] * 8 + [c_vp],
    "t2s_plane_transpose": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_vp],
    "t2s_tm_ones_row": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_pack_transposed": [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp],
    "t2s_weightnorm_scale": [c_vp, c_vp, c_int, c_int, c_vp, c_vp],
    "t2s_wn_backward": [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp,
                        c_vp, c_int, c_vp],
    "t2s_wg_affine_backward": [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_small_wgrad_scratch": [c_int, c_int],
    "t2s_small_wgrad": [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                        c_int, c_vp],
    "t2s_rows_sum": [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "t2s_wg_start_dgrad": [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp],
    "t2s_wg_convinv_wgrad": [c_vp, c_vp, c_vp, c_vp, c_float, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp],
    "t2s_wg_upsample_wgrad": [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                              c_vp],
    "t2s_adam_table": [c_vp, c_int, c_long, c_float, c_float, c_float, c_float, c_int, c_float, c_float, c_vp],
    "t2s_grad_norm_partials": [],
    "t2s_grad_norm_table": [c_vp, c_int, c_long, c_float, c_float, c_vp, c_vp, c_vp],
    "t2s_grad_scale_table": [c_vp, c_int, c_long, c_vp, c_vp],
    "t2s_adam_table_clip": [c_vp, c_int, c_long, c_float, c_float, c_float, c_float, c_int, c_float, c_float, c_vp, c_int, c_vp],
}
# fp16 vocoder planes (WaveGlow.infer for .half() models): every _h16 entry point takes its partner's argument list
for _n in ("t2s_pack_conv_weight_table", "t2s_wg_endfold_weights", "t2s_wg_upsample_squeeze", "t2s_wg_start",
           "t2s_wg_in_cond_gate_fold", "t2s_wg_res_only"):
    SIGNATURES[_n + "_h16"] = list(SIGNATURES[_n])
# ... and the fp16 chain of infer_batch: the _h16 partner's argument list with `const int* lengths` in front of `stream`
for _n in ("t2s_wg_start", "t2s_wg_in_cond_gate_fold", "t2s_wg_res_only"):
    SIGNATURES[_n + "_h16_ragged"] = SIGNATURES[_n + "_h16"][:-1] + [c_vp, c_vp]
del _n
_RESTYPE = {"t2s_error_string": ctypes.c_char_p, "t2s_last_hip_error": ctypes.c_char_p,
            "t2s_small_wgrad_scratch": ctypes.c_long, "t2s_taco_lstm_xbuf_bytes": ctypes.c_long, "t2s_loud_scratch": ctypes.c_long,
            "t2s_limit_scratch": ctypes.c_long, "t2s_resample_window_end": ctypes.c_long, "t2s_limit_window_end": ctypes.c_long,
            "t2s_sos_scratch": ctypes.c_long}


class T2SError(RuntimeError):
    pass


class TacoW16(ctypes.Structure):
    """Mirror of ``t2s_taco_w16`` (include/t2s_hip.h): the decoder's four LSTM matrices as IEEE binary16."""
    _fields_ = [(n, c_vp) for n in ("att_w_ih", "att_w_hh", "dec_w_ih", "dec_w_hh")]


_lib = None


def load():
    """Load the shared library (once).  Raises T2SError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise T2SError(
            "libt2s_hip.so not found at %s - build it with `python -m text2speech_amd.build` "
            "(there is no CPU fallback on the product path)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    diagnostic = bool(os.environ.get("T2S_LIB_PATH"))
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            if diagnostic:
                # a diagnostic build (explicit T2S_LIB_PATH) may predate the newest entry points: it loads, and CALLING a missing
                # one raises (`call` below).  The shipped library must export every declared symbol.
                continue
            raise T2SError("libt2s_hip.so does not export %s" % name) from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, c_int)
    _lib = lib
    return lib


def ptr(t):
    """Device (or host) pointer of a tensor, None -> NULL."""
    if t is None:
        return None
    return c_vp(t.data_ptr())


HOST_TIMES = {}     # T2S_HOST_TIMING=1: seconds the host spent inside each entry point (enqueue cost; diagnostic)
_HOST_TIMING = bool(os.environ.get("T2S_HOST_TIMING"))


def call(name, *args):
    """Call an int-returning entry point; raise on a non-zero code."""
    lib = load()
    if _HOST_TIMING:
        import time
        t0 = time.perf_counter()
        rc = getattr(lib, name)(*args)
        c = HOST_TIMES.setdefault(name, [0, 0.0])
        c[0] += 1
        c[1] += time.perf_counter() - t0
    else:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise T2SError("%s does not export %s (a diagnostic build older than the entry point?)" % (LIB_PATH, name)) from e
        rc = fn(*args)
    if rc != 0:
        msg = lib.t2s_error_string(rc).decode()
        hip = lib.t2s_last_hip_error().decode()
        raise T2SError("%s failed: %s%s" % (name, msg, (" (" + hip + ")") if hip and rc == -2 else ""))
    return rc


def operand_format():
    """0: split-bf16 planes (the shipped library); 1: split-fp16 planes (diagnostic build, T2S_LIB_PATH=build/f16x3/...)."""
    return load().t2s_operand_format()


def plane_rows(L, halo):
    return load().t2s_plane_rows(L, halo)


def padded_rows(rows):
    return load().t2s_padded_rows(rows)


def current_stream():
    import torch
    return c_vp(torch.cuda.current_stream().cuda_stream)


_orders = None         # every live StreamOrder (a weakref.WeakSet, made with the first one)


class StreamOrder:
    """Program order per object across streams (point 3).  The object remembers the stream of its last
    call; a call that arrives on another stream makes that stream wait on the device for the last one before its first launch or
    cache read.  On one stream it is a comparison: nothing is recorded and nothing is launched.

    Parameters are shared between objects: an optimizer (``writer=True``) rewrites in place what the engines pack from.  So a
    writer's call also waits for the latest call of every other object, and every object's call for the latest call of every
    writer - once per such call, and only where the two streams differ.  Two engines never wait for each other: a Tacotron and a
    WaveGlow on streams of their own stay independent."""
    __slots__ = ("last", "calls", "seen", "writer", "switched", "__weakref__")

    def __init__(self, writer=False):
        import weakref
        global _orders
        if _orders is None:
            _orders = weakref.WeakSet()
        self.last = None
        self.calls = 0
        self.seen = weakref.WeakKeyDictionary()     # other object -> the count of its calls this one is ordered behind
        self.writer = bool(writer)
        self.switched = False       # whether the latest enter() came on another stream than the call before it
        _orders.add(self)

    def __deepcopy__(self, memo):
        return StreamOrder(self.writer)     # a copied engine or optimizer has made no call yet

    def enter(self, device=None):
        """The caller's current stream, ordered behind the object's last call and behind the writers of what it reads."""
        import torch
        cur = torch.cuda.current_stream(device)
        last = self.last
        self.switched = last is not None and last != cur
        if self.switched:
            cur.wait_stream(last)
        self.last = cur
        self.calls += 1
        for o in _orders:
            if o is self or not (o.writer or self.writer) or o.last is None or self.seen.get(o) == o.calls:
                continue
            if o.last != cur:
                cur.wait_stream(o.last)
            self.seen[o] = o.calls
        return cur


def record_stream(obj, stream, _seen=None):
    """tensor.record_stream(stream) for every device tensor reachable through dicts, lists, tuples and plain objects: a resident
    buffer that was allocated on one stream and is now used on another must not be handed out again by the caching allocator,
    once it is dropped, before that other stream has finished with it.  Called where a StreamOrder saw the stream change, never on
    the single-stream path."""
    import torch
    seen = set() if _seen is None else _seen
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if torch.is_tensor(obj):
        if obj.is_cuda:
            obj.record_stream(stream)
    elif isinstance(obj, dict):
        for v in obj.values():
            record_stream(v, stream, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            record_stream(v, stream, seen)
    elif hasattr(obj, "__dict__") and not isinstance(obj, (torch.nn.Module, torch.cuda.Stream, torch.cuda.Event, type)):
        record_stream(vars(obj), stream, seen)
