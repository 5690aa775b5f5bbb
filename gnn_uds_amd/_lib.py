"""ctypes binding of libuds_hip.so (the C ABI in include/uds_hip.h) for PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the stream; every computation below is a
hand-written HIP kernel reached through the C ABI.  There is NO fallback: if the library is
missing or a tensor is not a contiguous fp32 CUDA(HIP) tensor the call raises.
"""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must be imported first: its libamdhip64.so.7 is the runtime we bind to)

_HERE = os.path.dirname(os.path.abspath(__file__))
# UDS_LIB_PATH: a differently built copy of the same library (kernel experiments: tools/variant_bench.py)
LIB_PATH = os.environ.get('UDS_LIB_PATH') or os.path.join(_HERE, 'libuds_hip.so')

ABI_VERSION = 23
FLAG_EXACT_FP32, FLAG_REQUIRE_FUSED = 1, 2
PRECISION_FLAGS = {'bf16x3': 0, 'fp32': FLAG_EXACT_FP32}

ACT = {None: 0, 'linear': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3, 'hard_sigmoid': 4}
_KIND = {'GRU': 0, 'LSTM': 1}           # the `kind` argument of the recurrent entries

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_ptr = ctypes.c_void_p

# name -> (restype, argtypes): every symbol include/uds_hip.h declares
SYMBOLS = {
    'uds_abi_version': (_c_int, []),
    'uds_last_error': (ctypes.c_char_p, []),
    'uds_csr_create': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_ptr)]),
    'uds_csr_destroy': (_c_int, [_c_ptr]),
    'uds_csr_shape': (_c_int, [_c_ptr, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64),
                               ctypes.POINTER(ctypes.c_int32)]),
    'uds_csr_row_order': (_c_int, [_c_ptr, _c_ptr]),
    'uds_dense_act': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_int, _c_ptr, _c_ptr,
                               _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_dense_route': (_c_int, [_c_i64, _c_i64, _c_i64, _c_int, _c_i64, _c_i64, _c_int, _c_ptr]),
    'uds_csr_spmm': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_int, _c_ptr, _c_ptr]),
    'uds_conv1d_causal': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr,
                                   _c_ptr]),
    'uds_dense_cumsum_heads': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr, _c_ptr, _c_ptr]),
    'uds_recurrent_fused': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_recurrent_fused_supported': (_c_int, [_c_i64, _c_int]),
    'uds_recurrent_forward': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_attn_sum_pool': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr]),
    'uds_attn_sum_pool_pair': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr]),
    'uds_attn_sum_pool_backward': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr,
                                            _c_ptr, _c_ptr]),
    'uds_dropout': (_c_int, [_c_ptr, _c_i64, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, _c_ptr, _c_ptr]),
    'uds_adam_workspace_floats': (_c_i64, [_c_ptr, _c_i64]),
    'uds_adam_step': (_c_int, [_c_ptr, _c_i64, _c_ptr] + [ctypes.c_double] * 5 + [_c_ptr, _c_ptr, _c_i64, _c_ptr]),
    'uds_window_batch': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int] + [_c_ptr] * 7),
    'uds_window_draw': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, ctypes.c_uint64, _c_ptr, _c_ptr, _c_ptr]),
    'uds_mpc_objective': (_c_int, [_c_ptr, _c_ptr] + [_c_i64] * 5 + [_c_ptr] * 6),
    'uds_mpc_objective_backward': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_ptr] + [_c_i64] * 4 + [_c_ptr] * 6),
    'uds_ce_draw': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, ctypes.c_uint64, _c_ptr, _c_ptr, _c_ptr]),
    'uds_ce_update': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, ctypes.c_double, ctypes.c_double] + [_c_ptr] * 6),
    'uds_recurrent_forward_train': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr]),
    'uds_recurrent_backward': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr]),
    'uds_recurrent_bwd_packed_bytes': (_c_i64, [_c_i64, _c_int]),
    'uds_recurrent_pack_bwd': (_c_int, [_c_ptr, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_recurrent_backward_h': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr,
                                          _c_ptr]),
    'uds_rowgemm_packed_bytes': (_c_i64, [_c_i64, _c_i64]),
    'uds_rowgemm_pack': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr]),
    'uds_gat_aggregate_masked': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_gat_aggregate_coef': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_diffusion_forward': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_diffusion_backward_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_diffusion_backward': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64,
                                        _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_diffusion_forward_m': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_diffusion_backward_m_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_diffusion_backward_m': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64,
                                          _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_halo_pack': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr]),
    'uds_halo_unpack': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr]),
    'uds_halo_pack_all': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_i64,
                                   _c_ptr, _c_ptr]),
    'uds_halo_unpack_all': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr,
                                     _c_i64, _c_ptr]),
    'uds_halo_pack_clear_all': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr,
                                         _c_i64, _c_ptr, _c_ptr]),
    'uds_halo_accumulate_all': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr,
                                         _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr]),
    'uds_remainder_packed_bytes': (_c_i64, [_c_i64, _c_i64]),
    'uds_remainder_pack': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr]),
    'uds_remainder_workspace_bytes': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_remainder_forward_dense': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_int, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr]),
    'uds_remainder_forward': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr]),
    'uds_remainder_snapshot_plan': (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64, _c_ptr]),
    'uds_remainder_snapshot': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_int, _c_i64, _c_i64, _c_ptr, _c_ptr]),
    'uds_remainder_snapshot_pair': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr,
                                             _c_ptr, _c_i64, _c_int, _c_i64, _c_i64, _c_ptr]),
    'uds_rowgemm_forward': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_rowgemm_forward_pair': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64,
                                          _c_i64, _c_i64, _c_int, _c_ptr]),
    'uds_rowgemm_forward_cat': (_c_int, [_c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int,
                                         _c_ptr, _c_i64, _c_i64, _c_ptr]),
    'uds_dense_cumsum': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr, _c_ptr]),
    'uds_conv_stack_plan': (_c_int, [_c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr]),
    'uds_conv_stack_forward': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr]),
    'uds_cumsum_act': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_flow_balance': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_gat_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64]),
    'uds_gat_forward': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64,
                                 _c_int, _c_ptr, _c_ptr, _c_ptr]),
    'uds_gat_aggregate': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_gat_backward': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_ptr,
                                  _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_gat_backward_coef': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_ptr,
                                       _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_gat_aggregate_ex': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr]),
    'uds_gat_backward_ex': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64,
                                     _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_gat_backward_act_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_gat_backward_act': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr,
                                      _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr]),
    'uds_gat_aggregate_heads': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_ptr,
                                         _c_ptr, _c_ptr]),
    'uds_gat_backward_heads': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64,
                                        _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_csr_sddmm': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_ptr, _c_ptr]),
    'uds_wgrad_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_int]),
    'uds_wgrad': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_wgrad_wide_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_int]),
    'uds_wgrad_wide': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_node_edge_wgrad_plan': (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64, _c_ptr]),
    'uds_node_edge_wgrad_workspace_bytes': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_node_edge_wgrad': (_c_int, [_c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_network_create': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, ctypes.POINTER(_c_ptr)]),
    'uds_network_destroy': (_c_int, [_c_ptr]),
    'uds_network_prepare': (_c_int, [_c_ptr, _c_i64, _c_i64]),
    'uds_network_plan_info': (_c_int, [_c_ptr, _c_ptr]),
    'uds_network_fused_launches': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_ptr]),
    'uds_fused_chunk': (_c_int, [_c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    'uds_tile_plan_create': (_c_int, [_c_ptr] * 8 + [_c_i64, _c_i64] + [ctypes.c_int32] * 4 + [ctypes.POINTER(_c_ptr)]),
    'uds_tile_plan_destroy': (_c_int, [_c_ptr]),
    'uds_tile_plan_sizes': (_c_int, [_c_ptr, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _c_ptr]),
    'uds_tile_plan_copy': (_c_int, [_c_ptr, _c_ptr, _c_ptr]),
    'uds_tile_plan_refine_counts': (_c_int, [_c_ptr, _c_ptr]),
    'uds_tile_plan_blocks': (_c_int, [_c_ptr, _c_ptr, ctypes.POINTER(_c_i64)]),
    'uds_roll_update': (_c_int, [_c_ptr] * 7 + [_c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_predict_tail': (_c_int, [_c_ptr] * 9 + [_c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr]),
    'uds_predict_tail_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_predict_tail_backward': (_c_int, [_c_ptr] * 9 + [_c_i64, _c_i64] + [_c_ptr] * 8),
    'uds_fit_tail': (_c_int, [_c_ptr] * 15 + [_c_i64, _c_i64, _c_i64, _c_int] + [_c_ptr] * 5),
    'uds_fit_tail_workspace_floats': (_c_i64, [_c_i64, _c_i64, _c_i64, _c_i64]),
    'uds_fit_tail_backward': (_c_int, [_c_ptr] * 15 + [_c_i64, _c_i64, _c_i64, _c_int] + [_c_ptr] * 7),
    'uds_spatial_workspace_floats': (_c_i64, [_c_ptr, _c_i64, _c_i64, _c_i64]),
    'uds_spatial_packed_bytes': (_c_i64, []),
    'uds_spatial_pack_weights': (_c_int, [_c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_ptr, _c_ptr]),
    'uds_spatial_layer_forward': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64, _c_i64, _c_i64, _c_int,
                                           _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_spatial_layer_forward_rem': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr, _c_i64, _c_i64, _c_i64, _c_int, _c_int,
                                      _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'uds_spatial_layer_forward_split': (_c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_i64,
                                                 _c_i64, _c_i64, _c_int, _c_int, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
}


class SpatialParams(ctypes.Structure):
    """uds_spatial_params_t"""
    _fields_ = [(n, _c_ptr) for n in ('xe_k', 'xe_b', 'ex_k', 'ex_b', 'ne_n_val', 'ne_e_val',
                                      'gx_k', 'gx_as', 'gx_an', 'gx_b', 'ge_k', 'ge_as', 'ge_an', 'ge_b', 'packed')]


class AdamTensor(ctypes.Structure):
    """uds_adam_tensor_t"""
    _fields_ = [('p', _c_ptr), ('g', _c_ptr), ('m', _c_ptr), ('v', _c_ptr), ('numel', _c_i64)]


class WindowSeries(ctypes.Structure):
    """uds_window_series_t"""
    _fields_ = [(n, _c_ptr) for n in ('states', 'flood', 'edge_states', 'settings', 'tide')] + [(n, _c_i64) for n in ('Ttot', 'N', 'E', 'n_act')]


class WindowNorm(ctypes.Structure):
    """uds_window_norm_t"""
    _fields_ = [(n, _c_ptr) for n in ('span_x', 'min_x', 'span_b', 'min_b', 'span_y', 'min_y', 'span_e', 'min_e')]


class UdsError(RuntimeError):
    pass


_lib = None


def load():
    """dlopen libuds_hip.so (built by `python -m gnn_uds_amd.build` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s is missing: the HIP engine is not built (run `python -m gnn_uds_amd.build`); '
                          'gnn_uds_amd has no CPU fallback' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.uds_abi_version() != ABI_VERSION:
        raise ImportError('libuds_hip.so ABI %d, binding expects %d' % (lib.uds_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        msg = load().uds_last_error()
        raise UdsError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else '?'))


def _dev(t, name, allow_none=False):
    """Device pointer of a contiguous fp32 HIP tensor (the C ABI takes plain pointers)."""
    if t is None:
        if allow_none:
            return None
        raise UdsError('%s is required' % name)
    if not isinstance(t, torch.Tensor):
        raise UdsError('%s must be a torch.Tensor, got %r' % (name, type(t)))
    if not t.is_cuda:
        raise UdsError('%s is on %s: gnn_uds_amd runs on the MI355X only and has no CPU fallback' % (name, t.device))
    if t.dtype != torch.float32:
        raise UdsError('%s must be float32, got %s' % (name, t.dtype))
    if not t.is_contiguous():
        raise UdsError('%s must be contiguous' % name)
    _same_device(t.device.index, name)
    return t.data_ptr()


def _current_device():
    if not torch.cuda.is_available():
        raise UdsError('no HIP device is visible: gnn_uds_amd runs on the MI355X only and has no CPU fallback')
    return torch.cuda.current_device()


def _same_device(index, what):
    """Kernels are enqueued on the CURRENT device's stream and handles allocate on the current device: an operand or a
    handle that lives on another GPU would be reached as peer traffic at best, fault at worst -- refuse it."""
    cur = _current_device()
    if index is not None and index != cur:
        raise UdsError('%s lives on cuda:%d but the current device is cuda:%d: call torch.cuda.set_device(%d) (one process per GPU) '
                       'or wrap the call in `with torch.cuda.device(%d):`' % (what, index, cur, index, index))


def _dev_i32(t, name):
    """Device pointer of a contiguous int32 HIP tensor (index lists of the backward kernels)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
        raise UdsError('%s must be a contiguous int32 HIP tensor' % name)
    _same_device(t.device.index, name)
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nothing_to_launch(t, name, result):
    """`result` for a call whose output is empty: no launch (an empty tensor has no device pointer), but the operand `t`
    is still checked."""
    _dev(t, name)
    return result


def _out(out, shape, like, name):
    """The caller's output tensor (checked: shape, fp32, contiguous, same device) or a new one."""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    if tuple(out.shape) != tuple(shape) or out.device != like.device:
        raise UdsError('%s must be %r on %s, got %r on %s' % (name, tuple(shape), like.device, tuple(out.shape), out.device))
    _dev(out, name)
    return out


class CsrHandle:
    """uds_csr_t: a CSR pattern resident on the device, plus its degree-sorted row schedule."""

    def __init__(self, csr):
        lib = load()
        self.n_rows, self.n_cols, self.nnz = int(csr.n_rows), int(csr.n_cols), int(csr.nnz)
        rowptr = np.ascontiguousarray(csr.rowptr, dtype=np.int32)
        col = np.ascontiguousarray(csr.col, dtype=np.int32)
        h = _c_ptr()
        self.device = _current_device()                  # uds_csr_create allocates on the current device
        _check(lib.uds_csr_create(rowptr.ctypes.data, col.ctypes.data, self.n_rows, self.n_cols, self.nnz,
                                  ctypes.byref(h)), 'uds_csr_create')
        self._h = h
        self._rowptr, self._col = rowptr, col
        self._t = None

    def transposed(self, device):
        """(handle of the transposed pattern, perm_t): perm_t[p] (int32 device tensor) = position in THIS pattern's
        row-major order of entry p of the transposed pattern.  Integer bookkeeping for the backward kernels, built once."""
        if self._t is None:
            rows = np.repeat(np.arange(self.n_rows, dtype=np.int64), np.diff(self._rowptr.astype(np.int64)))
            cols = self._col.astype(np.int64)
            order = np.lexsort((rows, cols))                  # by column, then row: the transpose in row-major order
            t_rowptr = np.zeros(self.n_cols + 1, dtype=np.int64)
            np.add.at(t_rowptr, cols + 1, 1)
            t_rowptr = np.cumsum(t_rowptr)

            class _T:      # what CsrHandle.__init__ reads
                pass
            t = _T()
            t.n_rows, t.n_cols, t.nnz = self.n_cols, self.n_rows, self.nnz
            t.rowptr, t.col = t_rowptr.astype(np.int32), rows[order].astype(np.int32)
            self._t = (CsrHandle(t), order.astype(np.int32))
        h, perm = self._t
        if not isinstance(perm, torch.Tensor) or perm.device != torch.device(device):
            perm = torch.as_tensor(np.asarray(perm.cpu() if isinstance(perm, torch.Tensor) else perm), dtype=torch.int32,
                                   device=device)
            self._t = (h, perm)
        return h, perm

    @property
    def ptr(self):
        _same_device(self.device, 'this CSR handle')
        return self._h

    def row_order(self):
        out = np.empty(self.n_rows, dtype=np.int32)
        _check(load().uds_csr_row_order(self._h, out.ctypes.data), 'uds_csr_row_order')
        return out

    def max_degree(self):
        md = ctypes.c_int32()
        _check(load().uds_csr_shape(self._h, None, None, None, ctypes.byref(md)), 'uds_csr_shape')
        return md.value

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h is not None and _lib is not None:
            _lib.uds_csr_destroy(h)


class NetworkHandle:
    """uds_network_t over a gnn_uds_amd.graph.DrainageGraph."""

    def __init__(self, graph):
        lib = load()
        self.graph = graph
        self.adj = CsrHandle(graph.adj)
        self.edge_adj = CsrHandle(graph.edge_adj)
        self.inc_n = CsrHandle(graph.inc_n)
        self.inc_e = CsrHandle(graph.inc_e)
        h = _c_ptr()
        self.device = _current_device()                  # tile plans are uploaded to the current device
        _check(lib.uds_network_create(self.adj.ptr, self.edge_adj.ptr, self.inc_n.ptr, self.inc_e.ptr, ctypes.byref(h)),
               'uds_network_create')
        self._h = h
        self._prepared = {(64, 64)}
        self._bits = None

    @property
    def ptr(self):
        _same_device(self.device, 'this network handle')
        return self._h

    def prepare(self, fx, fe):
        """Build the tile plans a layer with input widths (fx, fe) needs (no-op for 64/64 and once built)."""
        key = (int(fx), int(fe))
        if key not in self._prepared:
            _check(load().uds_network_prepare(self.ptr, key[0], key[1]), 'uds_network_prepare')
            self._prepared.add(key)
            self._bits = None

    def fused_bits(self, fx, fe):
        """prepare(fx, fe), then plan_info()['fused'] (include/uds_hip.h: uds_network_plan_info): read again only after a
        prepare that built a plan, so a layer's forward asks without a library call."""
        self.prepare(fx, fe)
        if self._bits is None:
            self._bits = self.plan_info()['fused']
        return self._bits

    def plan_info(self):
        """Tile plan of the fused kernel: dict(fused, node_tiles, link_tiles, p_cap, q_cap, meta_cap, lds_bytes, ...)."""
        info = np.zeros(8, dtype=np.int32)
        _check(load().uds_network_plan_info(self._h, info.ctypes.data), 'uds_network_plan_info')
        keys = ('fused', 'node_tiles', 'link_tiles', 'p_cap', 'q_cap', 'meta_cap', 'lds_bytes', 't_code')
        out = dict(zip(keys, (int(v) for v in info)))
        out['t_node'], out['t_link'] = out['t_code'] // 1000, out['t_code'] % 1000
        return out

    def fused_launches(self, fx, fe, d):
        """prepare(fx, fe), then the launches a fused forward of a layer (fx, fe, d) makes on this network
        (include/uds_hip.h: uds_network_fused_launches): a list of 0, 1 or 2 dict(kernel, fp, fs, side_mask, n_tiles), kernel one
        of FUSED_KERNELS; fused_chunk(S, n_tiles) is the chunk length of such a launch over S snapshots."""
        self.prepare(fx, fe)
        info = np.zeros(11, dtype=np.int32)
        _check(load().uds_network_fused_launches(self._h, int(fx), int(fe), int(d), info.ctypes.data), 'uds_network_fused_launches')
        return [dict(kernel=FUSED_KERNELS[int(k)], fp=int(fp), fs=int(fs), side_mask=int(m), n_tiles=int(t))
                for k, fp, fs, m, t in info[1:1 + 5 * int(info[0])].reshape(-1, 5)]

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h is not None and _lib is not None:
            _lib.uds_network_destroy(h)


FUSED_KERNELS = {1: 'k_fused_ws', 2: 'k_fused_tile', 3: 'k_fused_cs'}      # UDS_KERNEL_* of include/uds_hip.h


def fused_chunk(S, working_tiles):
    """Snapshots per workgroup of a fused spatial launch of S snapshots over working_tiles tiles (host only, no device needed)."""
    c = _c_i64()
    _check(load().uds_fused_chunk(int(S), int(working_tiles), ctypes.byref(c)), 'uds_fused_chunk')
    return c.value


def tile_plan(graph, t_node=48, t_link=48, p_limit=0, q_limit=0, blocks=False):
    """Host-only tile plan of a DrainageGraph (no GPU needed): returns (hdr (T,8) int32, pool int32, caps).
    hdr columns: n_own, n_prim, n_sec, n_inc, n_adj, pool_off, side, meta_len (csrc/tile_plan.hpp).
    caps: p_cap, q_cap, meta_cap and refine = what the refinement of the tiles did (fill / move / dissolve counts).
    blocks=True adds caps['blocks']: the (T, stride) int32 tile blocks the fused d = 64 kernel fetches (fixed-width index
    lists; include/uds_hip.h: uds_tile_plan_blocks), or None when a tile exceeds the byte-wide local indices."""
    lib = load()
    arrs = []
    for c in (graph.adj, graph.edge_adj, graph.inc_n, graph.inc_e):
        arrs += [np.ascontiguousarray(c.rowptr, dtype=np.int32), np.ascontiguousarray(c.col, dtype=np.int32)]
    h = _c_ptr()
    _check(lib.uds_tile_plan_create(*[a.ctypes.data for a in arrs], graph.n_node, graph.n_edge, t_node, t_link,
                                    p_limit, q_limit, ctypes.byref(h)), 'uds_tile_plan_create')
    try:
        nt, pl = _c_i64(), _c_i64()
        caps = np.zeros(3, dtype=np.int32)
        _check(lib.uds_tile_plan_sizes(h, ctypes.byref(nt), ctypes.byref(pl), caps.ctypes.data), 'uds_tile_plan_sizes')
        hdr = np.zeros((nt.value, 8), dtype=np.int32)
        pool = np.zeros(pl.value, dtype=np.int32)
        _check(lib.uds_tile_plan_copy(h, hdr.ctypes.data, pool.ctypes.data), 'uds_tile_plan_copy')
        refine = np.zeros(3, dtype=np.int64)
        _check(lib.uds_tile_plan_refine_counts(h, refine.ctypes.data), 'uds_tile_plan_refine_counts')
        blk = None
        if blocks:
            stride = _c_i64()
            if lib.uds_tile_plan_blocks(h, None, ctypes.byref(stride)) == 0:
                blk = np.zeros((nt.value, stride.value), dtype=np.int32)
                _check(lib.uds_tile_plan_blocks(h, blk.ctypes.data, ctypes.byref(stride)), 'uds_tile_plan_blocks')
    finally:
        lib.uds_tile_plan_destroy(h)
    out = dict(p_cap=int(caps[0]), q_cap=int(caps[1]), meta_cap=int(caps[2]),
               refine=dict(fill=int(refine[0]), move=int(refine[1]), dissolve=int(refine[2])))
    if blocks:
        out['blocks'] = blk
    return hdr, pool, out


DENSE_KERNELS = {0: 'tiled', 1: 'embed'}      # kernel 0 / 1 of uds_dense_route: k_dense_act<CG> / k_embed_act<F>


def dense_route(fa, f_out, rows, fb=0, taps=0, attn=False, aligned=True):
    """uds_dense_route (host only, no device needed): what uds_dense_act (taps = 0) or uds_conv1d_causal (taps > 0, rows = B T R)
    launches for a shape.  aligned: W and bias are 16-byte aligned.  dict(kernel = 'tiled' or 'embed', param = CG or F,
    rows_per_wg (tiled, else 0), workgroups, stride = the embed kernel's grid stride in lanes (tiled: 0))."""
    info = (ctypes.c_int32 * 5)()
    _check(load().uds_dense_route(int(fa), int(fb), int(taps), int(bool(attn)), int(f_out), int(rows), int(bool(aligned)), info),
           'uds_dense_route')
    return dict(kernel=DENSE_KERNELS[int(info[0])], param=int(info[1]), rows_per_wg=int(info[2]), workgroups=int(info[3]),
                stride=int(info[4]))


def dense_act(xa, kernel, bias=None, act='linear', xb=None, attn=None, out=None, s_out=None):
    """act([xa | xb] @ kernel + bias) on the last axis.  attn=(a_self, a_nbr) also returns the
    GAT attention scalars of the pre-activation rows.  out / s_out=(s_self, s_nbr): the caller's result tensors."""
    lib = load()
    fa = xa.shape[-1]
    fb = 0 if xb is None else xb.shape[-1]
    rows = xa.numel() // fa
    fo = kernel.shape[-1]
    if kernel.shape[0] != fa + fb:
        raise UdsError('kernel has %d input features, inputs give %d' % (kernel.shape[0], fa + fb))
    if xb is not None and xb.shape[:-1] != xa.shape[:-1]:
        raise UdsError('xa %r and xb %r disagree on leading dims' % (tuple(xa.shape), tuple(xb.shape)))
    out = _out(out, xa.shape[:-1] + (fo,), xa, 'out')
    s_self = s_nbr = None
    if attn is not None:
        s_self = _out(s_out[0] if s_out else None, xa.shape[:-1], xa, 's_self')
        s_nbr = _out(s_out[1] if s_out else None, xa.shape[:-1], xa, 's_nbr')
    elif s_out is not None:
        raise UdsError('dense_act: s_out is given without attn')
    if rows == 0:
        return _nothing_to_launch(xa, 'xa', (out, s_self, s_nbr) if attn is not None else out)
    _check(lib.uds_dense_act(_dev(xa, 'xa'), fa, _dev(xb, 'xb', True), fb, rows, _dev(kernel, 'kernel'),
                             _dev(bias, 'bias', True), fo, ACT[act],
                             _dev(attn[0], 'a_self') if attn else None, _dev(attn[1], 'a_nbr') if attn else None,
                             _dev(out, 'out'), _dev(s_self, 's_self', True), _dev(s_nbr, 's_nbr', True), _stream()),
           'uds_dense_act')
    return (out, s_self, s_nbr) if attn is not None else out


def conv1d_causal(x, kernel, bias=None, dilation=1, act='linear', out=None):
    """keras Conv1D(padding='causal', dilation_rate) along axis 1 of x (B,T,R,F), no transposes; kernel (taps,F,H).
    out: the caller's result tensor."""
    lib = load()
    if x.dim() != 4 or kernel.dim() != 3 or kernel.shape[1] != x.shape[-1]:
        raise UdsError('conv1d_causal: x %r / kernel %r' % (tuple(x.shape), tuple(kernel.shape)))
    B, T, R, F = x.shape
    taps, _, H = kernel.shape
    out = _out(out, (B, T, R, H), x, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_conv1d_causal(_dev(x, 'x'), B, T, R, F, _dev(kernel, 'kernel'), _dev(bias, 'bias', True), taps, dilation, H,
                                 ACT[act], _dev(out, 'out'), _stream()), 'uds_conv1d_causal')
    return out


def recurrent_fused_supported(F, kind):
    """Input forms uds_recurrent_fused takes: F = 64 / 128 input rows (W + U must fit the LDS), F = 0 = given projection."""
    return bool(load().uds_recurrent_fused_supported(int(F), _KIND[kind]))


def recurrent_pack(kernel, recurrent_kernel):
    """MFMA fragments of a GRU / LSTM layer with 64 units: the G 64-column slices of `kernel` (F, G*64) -- none when kernel is
    None (the input projection is computed separately) --, then of `recurrent_kernel` (64, G*64)."""
    G = recurrent_kernel.shape[1] // 64
    if tuple(recurrent_kernel.shape) != (64, G * 64) or G not in (3, 4) or (kernel is not None and kernel.shape[1] != G * 64):
        raise UdsError('recurrent_pack: kernel %r / recurrent kernel %r (F x G*64 and 64 x G*64 with G = 3 or 4)'
                       % (None if kernel is None else tuple(kernel.shape), tuple(recurrent_kernel.shape)))
    mats = [recurrent_kernel] if kernel is None else [kernel, recurrent_kernel]
    return torch.cat([rowgemm_pack(m[:, 64 * g:64 * (g + 1)].contiguous()) for m in mats for g in range(G)]).contiguous()


def recurrent_fused(x, packed, b_in, b_rec, kind, projected=False):
    """Hidden states (B, T, R, 64) of a GRU / LSTM layer with 64 units in one launch (uds_recurrent_fused).  projected=True:
    x is the input projection (B, T, R, G*64) incl. its bias."""
    lib = load()
    B, T, R, F = x.shape
    out = torch.empty((B, T, R, 64), device=x.device, dtype=torch.float32)
    if out.numel():
        _check(lib.uds_recurrent_fused(_dev(x, 'x'), 0 if projected else F, packed.data_ptr(), _dev(b_in, 'b_in', True), _dev(b_rec, 'b_rec', True),
                                       B, T, R, _KIND[kind], _dev(out, 'out'), _stream()), 'uds_recurrent_fused')
    return out


def attn_sum_pool(x, attn_kernel):
    """GlobalAttnSumPool: x (B, R, F), attn_kernel (F,) or (F, 1) -> (B, F) (uds_attn_sum_pool)."""
    lib = load()
    B, R, F = x.shape
    k = attn_kernel.reshape(-1).contiguous()
    if k.numel() != F:
        raise UdsError('attn_sum_pool: x %r, attn_kernel %r' % (tuple(x.shape), tuple(attn_kernel.shape)))
    out = torch.empty((B, F), device=x.device, dtype=torch.float32)
    if B:
        _check(lib.uds_attn_sum_pool(_dev(x, 'x'), _dev(k, 'attn_kernel'), B, R, F, _dev(out, 'out'), _stream()), 'uds_attn_sum_pool')
    return out


def _pool_pair_shapes(what, x, e, attn_kernel):
    if x.dim() != 3 or (e is not None and (e.dim() != 3 or e.shape[0] != x.shape[0] or e.shape[2] != x.shape[2])) or attn_kernel.numel() != x.shape[2]:
        raise UdsError('%s: x %r, e %r, attn_kernel %r' % (what, tuple(x.shape), None if e is None else tuple(e.shape), tuple(attn_kernel.shape)))
    if e is not None and e.shape[1] == 0:
        e = None
    return x.shape[0], x.shape[1], 0 if e is None else e.shape[1], x.shape[2], e, attn_kernel.reshape(-1).contiguous()


def attn_sum_pool_pair(x, e, attn_kernel, want_stat=False):
    """GlobalAttnSumPool over the rows of x (B, Rx, F) followed by those of e (B, Re, F) or None, without the concatenation
    (uds_attn_sum_pool_pair): out (B, F), bit for bit attn_sum_pool of the stacked tensor.  want_stat: also stat (B, 2), the
    running maximum and the sum of exponentials of every sample, which attn_sum_pool_backward takes."""
    lib = load()
    B, Rx, Re, F, e, k = _pool_pair_shapes('attn_sum_pool_pair', x, e, attn_kernel)
    out = torch.empty((B, F), device=x.device, dtype=torch.float32)
    stat = torch.empty((B, 2), device=x.device, dtype=torch.float32) if want_stat else None
    if B:
        _check(lib.uds_attn_sum_pool_pair(_dev(x, 'x'), Rx, _dev(e, 'e', True), Re, _dev(k, 'attn_kernel'), B, F, _dev(out, 'out'),
                                          _dev(stat, 'stat', True), _stream()), 'uds_attn_sum_pool_pair')
    return (out, stat) if want_stat else out


def attn_sum_pool_backward(x, e, attn_kernel, out, stat, grad, want_dx=True, want_de=True, want_dk=True, dx=None, de=None, dk=None, dk_ws=None):
    """(dx, de, dk) of attn_sum_pool_pair from its saved `out` and `stat` for the upstream gradient grad (B, F)
    (uds_attn_sum_pool_backward): dx like x, de like e, dk (F,); None for a gradient that is not wanted (and de when e is None).
    dx / de / dk / dk_ws (B, F): the caller's tensors instead of new ones."""
    lib = load()
    B, Rx, Re, F, e, k = _pool_pair_shapes('attn_sum_pool_backward', x, e, attn_kernel)
    if tuple(out.shape) != (B, F) or tuple(stat.shape) != (B, 2) or tuple(grad.shape) != (B, F):
        raise UdsError('attn_sum_pool_backward: out %r, stat %r, grad %r for B=%d, F=%d' % (tuple(out.shape), tuple(stat.shape), tuple(grad.shape), B, F))
    dx = _out(dx, (B, Rx, F), x, 'dx') if want_dx else None
    de = _out(de, (B, Re, F), x, 'de') if want_de and e is not None else None
    dk = _out(dk, (F,), x, 'dk') if want_dk else None
    dk_ws = _out(dk_ws, (B, F), x, 'dk_ws') if want_dk else None
    if dx is not None or de is not None or dk is not None:
        _check(lib.uds_attn_sum_pool_backward(_dev(x, 'x'), Rx, _dev(e, 'e', True), Re, _dev(k, 'attn_kernel'), _dev(out, 'out'), _dev(stat, 'stat'),
                                              _dev(grad, 'grad'), B, F, _dev(dx, 'dx', True), _dev(de, 'de', True), _dev(dk_ws, 'dk_ws', True),
                                              _dev(dk, 'dk', True), _stream()), 'uds_attn_sum_pool_backward')
    return dx, de, dk


def dropout(x, rate, seed, offset):
    """keras Dropout in training mode on a contiguous fp32 device tensor (uds_dropout): kept elements scaled by 1 / (1 - rate);
    the mask depends on (seed, offset + flat index) only."""
    lib = load()
    x = x.contiguous()
    out = torch.empty_like(x)
    if out.numel():
        _check(lib.uds_dropout(_dev(x, 'x'), x.numel(), float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                               _dev(out, 'out'), _stream()), 'uds_dropout')
    return out


def _recurrent_forward(xp, recurrent_kernel, recurrent_bias, kind, train):
    """(h, c) through uds_recurrent_forward_train (c: the LSTM's cell states, None for the GRU) or, train False, (h, None)
    through uds_recurrent_forward."""
    lib = load()
    B, T, R, GH = xp.shape
    G = {'GRU': 3, 'LSTM': 4}[kind]
    H = GH // G
    if GH != G * H or tuple(recurrent_kernel.shape) != (H, GH):
        raise UdsError('recurrent_forward: xp %r, recurrent kernel %r for a %s' % (tuple(xp.shape), tuple(recurrent_kernel.shape), kind))
    out = torch.empty((B, T, R, H), device=xp.device, dtype=torch.float32)
    c = torch.empty_like(out) if train and kind == 'LSTM' else None
    if out.numel():
        entry = 'uds_recurrent_forward_train' if train else 'uds_recurrent_forward'
        _check(getattr(lib, entry)(_dev(xp, 'xp'), _dev(recurrent_kernel, 'recurrent_kernel'), _dev(recurrent_bias, 'recurrent_bias', True),
                                   B, T, R, H, _KIND[kind], _dev(out, 'out'), *([_dev(c, 'c', True)] if train else []), _stream()), entry)
    return out, c


def recurrent_forward_train(xp, recurrent_kernel, recurrent_bias, kind):
    """(h, c): hidden states (B, T, R, H) as recurrent_forward, plus the LSTM's cell states (None for the GRU) -- what
    recurrent_backward needs from the forward pass."""
    return _recurrent_forward(xp, recurrent_kernel, recurrent_bias, kind, True)


RECURRENT_TRAIN_WIDTHS = tuple(range(16, 129, 16))      # units the back-propagation-through-time kernels are built for


def recurrent_bwd_route(units):
    """Which C entry back-propagates a GRU / LSTM layer of `units` units: 64 is uds_recurrent_backward (the kernel the 64-unit
    emulator has always trained on), every other multiple of 16 from 16 to 128 uds_recurrent_backward_h; None: not built."""
    if units == 64:
        return 'uds_recurrent_backward'
    return 'uds_recurrent_backward_h' if units in RECURRENT_TRAIN_WIDTHS else None


def recurrent_bwd_packed_bytes(units, G):
    """Bytes of the packed image of an (units, G*units) recurrent kernel: U_g and U_g^T for every gate, each ceil(units / 32)
    k-steps x units / 16 feature blocks of a bf16 hi and a lo fragment (64 lanes x 16 bytes); 0: width not built.  The host
    restatement of uds_recurrent_bwd_packed_bytes."""
    if units not in RECURRENT_TRAIN_WIDTHS or G not in (3, 4):
        return 0
    return 2 * G * ((units + 31) // 32) * (units // 16) * 2 * 64 * 16


def recurrent_pack_bwd(recurrent_kernel):
    """MFMA fragments for recurrent_backward: the G H x H slices of U, then of U_g^T, H = the layer's units (a multiple of 16
    from 16 to 128).  64 units: the uds_rowgemm_pack image uds_recurrent_backward takes; other widths: uds_recurrent_pack_bwd."""
    H = recurrent_kernel.shape[0]
    G = recurrent_kernel.shape[1] // max(H, 1)
    route = recurrent_bwd_route(H)
    if recurrent_kernel.dim() != 2 or tuple(recurrent_kernel.shape) != (H, G * H) or G not in (3, 4) or route is None:
        raise UdsError('recurrent_pack_bwd: recurrent kernel %r (H x G*H with G = 3 or 4 and H one of %r)'
                       % (tuple(recurrent_kernel.shape), RECURRENT_TRAIN_WIDTHS))
    if route == 'uds_recurrent_backward':
        sl = [recurrent_kernel[:, 64 * g:64 * (g + 1)] for g in range(G)]
        return torch.cat([rowgemm_pack(m.contiguous()) for m in sl] + [rowgemm_pack(m.t().contiguous()) for m in sl]).contiguous()
    lib = load()
    nbytes = lib.uds_recurrent_bwd_packed_bytes(H, G - 3)
    if nbytes != recurrent_bwd_packed_bytes(H, G):
        raise UdsError('recurrent_pack_bwd: the library packs %d bytes for %d units, the binding expects %d' % (nbytes, H, recurrent_bwd_packed_bytes(H, G)))
    out = torch.empty(nbytes // 4, device=recurrent_kernel.device, dtype=torch.float32)
    _check(lib.uds_recurrent_pack_bwd(_dev(recurrent_kernel.contiguous(), 'recurrent_kernel'), H, G - 3, out.data_ptr(), _stream()),
           'uds_recurrent_pack_bwd')
    return out


def recurrent_backward(xp, packed, recurrent_bias, h, c, gh, kind):
    """(dxp (B, T, R, G*H), darec (G, B, T, R, H)) of a GRU / LSTM layer of H units (a multiple of 16 from 16 to 128): back-
    propagation through time in one launch.  64 units run uds_recurrent_backward, other widths uds_recurrent_backward_h."""
    lib = load()
    B, T, R, GH = xp.shape
    G = {'GRU': 3, 'LSTM': 4}[kind]
    H = h.shape[-1]
    route = recurrent_bwd_route(H)
    if GH != G * H or tuple(h.shape) != (B, T, R, H) or tuple(gh.shape) != (B, T, R, H) or route is None:
        raise UdsError('recurrent_backward: xp %r, h %r, gh %r for a %s of one of %r units'
                       % (tuple(xp.shape), tuple(h.shape), tuple(gh.shape), kind, RECURRENT_TRAIN_WIDTHS))
    if packed.numel() * 4 != recurrent_bwd_packed_bytes(H, G):
        raise UdsError('recurrent_backward: packed image of %d bytes, %d units need %d' % (packed.numel() * 4, H, recurrent_bwd_packed_bytes(H, G)))
    dxp = torch.empty_like(xp)
    darec = torch.empty((G, B, T, R, H), device=xp.device, dtype=torch.float32)
    if dxp.numel():
        width = [] if route == 'uds_recurrent_backward' else [H]      # the 64-unit entry takes no width
        _check(getattr(lib, route)(_dev(xp, 'xp'), packed.data_ptr(), _dev(recurrent_bias, 'recurrent_bias', True), _dev(h, 'h'),
                                   _dev(c, 'c', True), _dev(gh, 'gh'), B, T, R, *width, _KIND[kind], _dev(dxp, 'dxp'), _dev(darec, 'darec'),
                                   _stream()), route)
    return dxp, darec


def recurrent_forward(xp, recurrent_kernel, recurrent_bias, kind):
    """Hidden states (B, T, R, H) of a GRU (kind 'GRU') or LSTM from the input projections xp (B, T, R, G*H)."""
    return _recurrent_forward(xp, recurrent_kernel, recurrent_bias, kind, False)[0]


def rowgemm_supported(k_total, f_in, f_out):
    """Shapes the matrix-core row GEMM takes: input width a multiple of 32, at most 64 outputs, and the packed weights
    (K/32 * ceil(f_out/16) * 2 KiB) next to at least 32 KiB of per-wave DMA rings and the store tiles inside the 160 KiB LDS."""
    mb = 1 if f_out <= 16 else 2 if f_out <= 32 else 4
    return (f_in % 32 == 0 and k_total % 32 == 0 and 0 < f_out <= 64
            and (k_total // 32) * mb * 2048 + 256 + 8 * 2 * 2048 + 8 * 16 * (36 if mb >= 2 else 20) * 4 <= 160 * 1024)


def rowgemm_pack(kernel2d):
    """Pre-split a (K, f_out) kernel into bf16 hi/lo MFMA fragments (once per parameter update)."""
    lib = load()
    K, fo = kernel2d.shape
    nbytes = lib.uds_rowgemm_packed_bytes(K, fo)
    if nbytes <= 0:
        raise UdsError('rowgemm_pack: unsupported shape %r' % ((K, fo),))
    out = torch.empty(nbytes // 4, device=kernel2d.device, dtype=torch.float32)
    _check(lib.uds_rowgemm_pack(_dev(kernel2d, 'kernel'), K, fo, out.data_ptr(), _stream()), 'uds_rowgemm_pack')
    return out


def diffusion_forward(csr, vals, c0, r, tot, act='tanh'):
    """out[s, i, q] = act(c0[q] tot[s] + sum_p vals[p, q] r[s, col[p]]): DiffusionConv on the CSR support (uds_diffusion_forward)."""
    lib = load()
    S, C = r.shape[0], vals.shape[1]
    if tuple(vals.shape) != (csr.nnz, C) or tuple(c0.shape) != (C,) or tuple(r.shape) != (S, csr.n_cols) or tuple(tot.shape) != (S,):
        raise UdsError('diffusion_forward: vals %r c0 %r r %r tot %r for a %d x %d pattern with %d entries'
                       % (tuple(vals.shape), tuple(c0.shape), tuple(r.shape), tuple(tot.shape), csr.n_rows, csr.n_cols, csr.nnz))
    out = torch.empty((S, csr.n_rows, C), device=r.device, dtype=torch.float32)
    if out.numel():
        _check(lib.uds_diffusion_forward(csr.ptr, _dev(vals, 'vals'), _dev(c0, 'c0'), _dev(r, 'r'), _dev(tot, 'tot'), S, C, ACT[act],
                                         _dev(out, 'out'), _stream()), 'uds_diffusion_forward')
    return out


def diffusion_backward(csr, a, vals, c0, r, tot, y, gy, K1, act='tanh'):
    """(dr (S, n_cols), dtheta (C, K1)) of diffusion_forward's out = y given dL/dout = gy: dr folds in the tot term, dtheta is
    the gradient of the (C, K1) coefficient kernel; `a` (nnz,) = the filter's values on the support (uds_diffusion_backward)."""
    lib = load()
    S, C = r.shape[0], vals.shape[1]
    if (tuple(vals.shape) != (csr.nnz, C) or tuple(a.shape) != (csr.nnz,) or tuple(c0.shape) != (C,) or tuple(r.shape) != (S, csr.n_cols)
            or tuple(tot.shape) != (S,) or tuple(y.shape) != (S, csr.n_rows, C) or tuple(gy.shape) != (S, csr.n_rows, C)):
        raise UdsError('diffusion_backward: a %r vals %r c0 %r r %r tot %r y %r gy %r for a %d x %d pattern with %d entries'
                       % (tuple(a.shape), tuple(vals.shape), tuple(c0.shape), tuple(r.shape), tuple(tot.shape), tuple(y.shape),
                          tuple(gy.shape), csr.n_rows, csr.n_cols, csr.nnz))
    nws = lib.uds_diffusion_backward_workspace_floats(csr.n_rows, S, C, K1)
    if nws < 0:
        raise UdsError('diffusion_backward: C=%d K1=%d not taken (C %% 4 == 0, C <= 256, 1 <= K1 <= 16)' % (C, K1))
    ht, perm = csr.transposed(r.device)
    ws = torch.empty(max(int(nws), 4), device=r.device, dtype=torch.float32)
    dr = torch.empty((S, csr.n_cols), device=r.device, dtype=torch.float32)
    dtheta = torch.empty((C, K1), device=r.device, dtype=torch.float32)
    _check(lib.uds_diffusion_backward(csr.ptr, ht.ptr, _dev_i32(perm, 'perm_t'), _dev(a, 'a'), _dev(vals, 'vals'), _dev(c0, 'c0'),
                                      _dev(r, 'r'), _dev(tot, 'tot'), _dev(y, 'y'), _dev(gy, 'gy'), S, C, K1, ACT[act], ws.data_ptr(),
                                      _dev(dr, 'dr'), _dev(dtheta, 'dtheta'), _stream()), 'uds_diffusion_backward')
    return dr, dtheta


def diffusion_forward_m(csr, a, theta, r, tot, act='tanh', out=None):
    """diffusion_forward without the (nnz, C) table: out[s, i, q] = act(sum_m theta[q][K - m] M_m[s, i]), M_0 = tot[s],
    M_m = sum_p a[p]^m r[s, col[p]] over row i; `a` (nnz,) the filter's support values, theta (C, K1) the layer's kernel
    (uds_diffusion_forward_m).  out: a contiguous (S, n_rows, C) tensor to write into."""
    lib = load()
    S, (C, K1) = r.shape[0], theta.shape
    if tuple(a.shape) != (csr.nnz,) or tuple(r.shape) != (S, csr.n_cols) or tuple(tot.shape) != (S,):
        raise UdsError('diffusion_forward_m: a %r theta %r r %r tot %r for a %d x %d pattern with %d entries'
                       % (tuple(a.shape), tuple(theta.shape), tuple(r.shape), tuple(tot.shape), csr.n_rows, csr.n_cols, csr.nnz))
    if out is None:
        out = torch.empty((S, csr.n_rows, C), device=r.device, dtype=torch.float32)
    elif tuple(out.shape) != (S, csr.n_rows, C):
        raise UdsError('diffusion_forward_m: out %r, expected %r' % (tuple(out.shape), (S, csr.n_rows, C)))
    _check(lib.uds_diffusion_forward_m(csr.ptr, _dev(a, 'a'), _dev(theta, 'theta'), _dev(r, 'r'), _dev(tot, 'tot'), S, C, K1, ACT[act],
                                       _dev(out, 'out'), _stream()), 'uds_diffusion_forward_m')
    return out


def diffusion_backward_m(csr, a, theta, r, tot, y, gy, act='tanh', out=None, workspace=None):
    """(dr (S, n_cols), dtheta (C, K1)) of diffusion_forward_m's out = y given dL/dout = gy (uds_diffusion_backward_m).
    out: (dr, dtheta) tensors to write into; workspace: at least uds_diffusion_backward_m_workspace_floats floats."""
    lib = load()
    S, (C, K1) = r.shape[0], theta.shape
    if (tuple(a.shape) != (csr.nnz,) or tuple(r.shape) != (S, csr.n_cols) or tuple(tot.shape) != (S,)
            or tuple(y.shape) != (S, csr.n_rows, C) or tuple(gy.shape) != (S, csr.n_rows, C)):
        raise UdsError('diffusion_backward_m: a %r theta %r r %r tot %r y %r gy %r for a %d x %d pattern with %d entries'
                       % (tuple(a.shape), tuple(theta.shape), tuple(r.shape), tuple(tot.shape), tuple(y.shape), tuple(gy.shape),
                          csr.n_rows, csr.n_cols, csr.nnz))
    nws = lib.uds_diffusion_backward_m_workspace_floats(csr.n_rows, S, C, K1)
    if nws < 0:
        raise UdsError('diffusion_backward_m: C=%d K1=%d not taken (C %% 4 == 0, C <= 256, 1 <= K1 <= 16)' % (C, K1))
    ht, perm = csr.transposed(r.device)
    ws = torch.empty(max(int(nws), 4), device=r.device, dtype=torch.float32) if workspace is None else workspace
    if ws.numel() < nws:
        raise UdsError('diffusion_backward_m: workspace of %d floats, needs %d' % (ws.numel(), nws))
    if out is None:
        dr = torch.empty((S, csr.n_cols), device=r.device, dtype=torch.float32)
        dtheta = torch.empty((C, K1), device=r.device, dtype=torch.float32)
    else:
        dr, dtheta = out
        if tuple(dr.shape) != (S, csr.n_cols) or tuple(dtheta.shape) != (C, K1):
            raise UdsError('diffusion_backward_m: out %r / %r, expected %r / %r' % (tuple(dr.shape), tuple(dtheta.shape), (S, csr.n_cols), (C, K1)))
    _check(lib.uds_diffusion_backward_m(csr.ptr, ht.ptr, _dev_i32(perm, 'perm_t'), _dev(a, 'a'), _dev(theta, 'theta'), _dev(r, 'r'),
                                        _dev(tot, 'tot'), _dev(y, 'y'), _dev(gy, 'gy'), S, C, K1, ACT[act], ws.data_ptr(),
                                        _dev(dr, 'dr'), _dev(dtheta, 'dtheta'), _stream()), 'uds_diffusion_backward_m')
    return dr, dtheta


def halo_pack(x, e, idx_x, idx_e):
    """One message buffer (S, nx + ne, F) = [x[:, idx_x] | e[:, idx_e]] (int32 device index tensors): one launch per peer."""
    lib = load()
    S, n_x, F = x.shape
    n_e = e.shape[1]
    nx, ne = int(idx_x.numel()), int(idx_e.numel())
    buf = torch.empty((S, nx + ne, F), device=x.device, dtype=torch.float32)
    if buf.numel():
        _check(lib.uds_halo_pack(_dev(x, 'x'), n_x, _dev(e, 'e'), n_e, S, F, _dev_i32(idx_x, 'idx_x') if nx else None, nx,
                                 _dev_i32(idx_e, 'idx_e') if ne else None, ne, _dev(buf, 'buf'), _stream()), 'uds_halo_pack')
    return buf


def halo_unpack(buf, x, e, idx_x, idx_e):
    """x[:, idx_x], e[:, idx_e] = the two parts of a received message buffer (in place)."""
    lib = load()
    S, n_x, F = x.shape
    nx, ne = int(idx_x.numel()), int(idx_e.numel())
    if tuple(buf.shape) != (S, nx + ne, F):
        raise UdsError('halo_unpack: buffer %r for %d + %d rows of %r' % (tuple(buf.shape), nx, ne, tuple(x.shape)))
    if buf.numel():
        _check(lib.uds_halo_unpack(_dev(buf, 'buf'), S, F, _dev_i32(idx_x, 'idx_x') if nx else None, nx,
                                   _dev_i32(idx_e, 'idx_e') if ne else None, ne, _dev(x, 'x'), n_x, _dev(e, 'e'), e.shape[1], _stream()),
               'uds_halo_unpack')


def _halo_all_args(x, e, idx_x, idx_e, off_x, off_e, what):
    if x.dim() != 3 or e.dim() != 3 or x.shape[0] != e.shape[0] or x.shape[2] != e.shape[2]:
        raise UdsError('%s: x %r and e %r must be (S, rows, F) with the same S and F' % (what, tuple(x.shape), tuple(e.shape)))
    P = int(off_x.numel()) - 1
    if P < 1 or int(off_e.numel()) != P + 1:
        raise UdsError('%s: off_x / off_e need P + 1 >= 2 entries each, got %d / %d' % (what, off_x.numel(), off_e.numel()))
    return P, int(idx_x.numel()), int(idx_e.numel())


def _halo_pack_all(entry, x, e, idx_x, idx_e, off_x, off_e):
    """uds_halo_pack_all or uds_halo_pack_clear_all: the same arguments, the same buffer."""
    lib = load()
    P, nx, ne = _halo_all_args(x, e, idx_x, idx_e, off_x, off_e, entry[4:])
    S, n_x, F = x.shape
    buf = torch.empty(S * (nx + ne) * F, device=x.device, dtype=torch.float32)
    if buf.numel():
        _check(getattr(lib, entry)(_dev(x, 'x') if nx else None, n_x, _dev(e, 'e') if ne else None, e.shape[1], S, F,
                                   _dev_i32(idx_x, 'idx_x') if nx else None, nx, _dev_i32(idx_e, 'idx_e') if ne else None, ne,
                                   _dev_i32(off_x, 'off_x'), _dev_i32(off_e, 'off_e'), P, _dev(buf, 'buf'), _stream()), entry)
    return buf


def halo_pack_all(x, e, idx_x, idx_e, off_x, off_e):
    """The messages of all P peers, ONE launch (uds_halo_pack_all): a flat buffer in which peer q's message is the (S, nx_q + ne_q, F)
    block [x[:, idx_x[off_x[q]:off_x[q+1]]] | e[:, idx_e[off_e[q]:off_e[q+1]]]] at element offset S F (off_x[q] + off_e[q]).
    idx_* / off_* are int32 device tensors (off_*: P + 1 offsets); any F >= 1."""
    return _halo_pack_all('uds_halo_pack_all', x, e, idx_x, idx_e, off_x, off_e)


def halo_unpack_all(buf, x, e, idx_x, idx_e, off_x, off_e):
    """The inverse of halo_pack_all: every peer's block of `buf` scattered into its rows of x / e (in place), ONE launch."""
    lib = load()
    P, nx, ne = _halo_all_args(x, e, idx_x, idx_e, off_x, off_e, 'halo_unpack_all')
    S, n_x, F = x.shape
    if buf.numel() != S * (nx + ne) * F:
        raise UdsError('halo_unpack_all: buffer of %d floats for %d + %d rows of %r' % (buf.numel(), nx, ne, tuple(x.shape)))
    if buf.numel():
        _check(lib.uds_halo_unpack_all(_dev(buf, 'buf'), S, F, _dev_i32(idx_x, 'idx_x') if nx else None, nx,
                                       _dev_i32(idx_e, 'idx_e') if ne else None, ne, _dev_i32(off_x, 'off_x'), _dev_i32(off_e, 'off_e'), P,
                                       _dev(x, 'x') if nx else None, n_x, _dev(e, 'e') if ne else None, e.shape[1], _stream()),
               'uds_halo_unpack_all')


def halo_pack_clear_all(x, e, idx_x, idx_e, off_x, off_e):
    """halo_pack_all, and every row it reads is then zeroed in x / e (in place), ONE launch (uds_halo_pack_clear_all): the
    first half of the exchange's adjoint.  The rows listed across all peers must be distinct."""
    return _halo_pack_all('uds_halo_pack_clear_all', x, e, idx_x, idx_e, off_x, off_e)


def halo_accumulate_all(buf, x, e, off_x, off_e, tgt_x, tgt_e, ptr, src):
    """x[:, tgt_x[t]] (then e[:, tgt_e[t - tx]]) += the message rows src[ptr[t]:ptr[t+1]] of `buf` (laid out by off_x / off_e
    as halo_pack_all lays it out; rows numbered across peers), added in the listed order after the current value; in place,
    ONE launch, no atomics (uds_halo_accumulate_all).  int32 device index tensors; any F >= 1."""
    lib = load()
    P, tx, te = _halo_all_args(x, e, tgt_x, tgt_e, off_x, off_e, 'halo_accumulate_all')
    S, n_x, F = x.shape
    n_src = int(src.numel())
    if int(ptr.numel()) != tx + te + 1:
        raise UdsError('halo_accumulate_all: ptr has %d entries for %d + %d targets' % (ptr.numel(), tx, te))
    if S and tx + te:
        _check(lib.uds_halo_accumulate_all(_dev(buf, 'buf') if n_src else None, S, F, _dev_i32(off_x, 'off_x'), _dev_i32(off_e, 'off_e'), P,
                                           _dev_i32(tgt_x, 'tgt_x') if tx else None, tx, _dev_i32(tgt_e, 'tgt_e') if te else None, te,
                                           _dev_i32(ptr, 'ptr'), _dev_i32(src, 'src') if n_src else None, n_src,
                                           _dev(x, 'x') if tx else None, n_x, _dev(e, 'e') if te else None, e.shape[1], _stream()),
               'uds_halo_accumulate_all')


def remainder_pack(rest):
    """Pre-split the dense off-support part `rest` (R, M) of a trained NodeEdge into bf16 hi/lo planes (once per update)."""
    lib = load()
    if rest.dim() != 2 or rest.numel() == 0:
        raise UdsError('remainder_pack: rest %r' % (tuple(rest.shape),))
    R, M = rest.shape
    out = torch.empty(lib.uds_remainder_packed_bytes(R, M) // 4, device=rest.device, dtype=torch.float32)
    _check(lib.uds_remainder_pack(_dev(rest, 'rest'), R, M, out.data_ptr(), _stream()), 'uds_remainder_pack')
    return out


def _remainder_forward(entry, packed, shape, t, name, h=None, dense=None):
    """uds_remainder_forward on t = x (..., M, h), or uds_remainder_forward_dense on t = e (..., M, F) with dense =
    (packed_w, bias, act) and the output width h."""
    lib = load()
    R, M = shape
    if t.dim() < 2 or t.shape[-2] != M:
        raise UdsError('%s: %s %r against rest (%d, %d)' % (entry[4:], name, tuple(t.shape), R, M))
    F = t.shape[-1]
    h = F if dense is None else h
    S = t.numel() // (M * F) if M * F else 0
    out = torch.empty(tuple(t.shape[:-2]) + (R, h), device=t.device, dtype=torch.float32)
    if S == 0:
        return _nothing_to_launch(t, name, out)
    ws = torch.empty(lib.uds_remainder_workspace_bytes(R, M, S, h) // 4, device=t.device, dtype=torch.float32)
    _check(getattr(lib, entry)(packed.data_ptr(), R, M, _dev(t, name),
                               *([] if dense is None else [F, dense[0].data_ptr(), _dev(dense[1], 'bias', True), ACT[dense[2]]]),
                               S, h, ws.data_ptr(), _dev(out, 'out'), _stream()), entry)
    return out


def remainder_forward(packed, shape, x):
    """out[..., r, :] = sum_m rest[r, m] x[..., m, :] on the matrix cores (split-bf16): `packed` = remainder_pack(rest),
    shape = rest.shape, x (..., M, h) with h % 4 == 0, h <= 64."""
    return _remainder_forward('uds_remainder_forward', packed, shape, x, 'x')


def remainder_forward_dense(packed, shape, e, packed_w, bias, act, h):
    """rest @ act(e W + b) without the fp32 x_e in between (uds_remainder_forward_dense): e (..., M, F) with F 64 or 128, packed_w =
    rowgemm_pack(W (F, h)), h 32 or 64 -> (..., R, h)."""
    return _remainder_forward('uds_remainder_forward_dense', packed, shape, e, 'e', h, (packed_w, bias, act))


def remainder_snapshot_plan(R, M, F, h):
    """uds_remainder_snapshot_plan (host only): dict(G = snapshots per workgroup, 0 when the shape is refused; lds = LDS bytes;
    row_blocks = 16-row blocks of `rest` per wave pass)."""
    info = (ctypes.c_int32 * 4)()
    _check(load().uds_remainder_snapshot_plan(int(R), int(M), int(F), int(h), info), 'uds_remainder_snapshot_plan')
    return dict(G=int(info[0]), lds=int(info[1]), row_blocks=int(info[2]))


def _snapshot_side(entry, side):
    """Checks of one argument group (packed, shape, e, packed_w, bias, act, h) -> (S, F, the ABI's per-side arguments, out)."""
    packed, shape, e, packed_w, bias, act, h = side
    R, M = shape
    if e.dim() < 2 or e.shape[-2] != M:
        raise UdsError('%s: e %r against rest (%d, %d)' % (entry[4:], tuple(e.shape), R, M))
    F = e.shape[-1]
    S = e.numel() // (M * F) if M * F else 0
    out = torch.empty(tuple(e.shape[:-2]) + (R, h), device=e.device, dtype=torch.float32)
    if S == 0:
        _nothing_to_launch(e, 'e', out)
        return S, F, None, out
    return S, F, [packed.data_ptr(), R, M, _dev(e, 'e'), packed_w.data_ptr(), _dev(bias, 'bias', True), _dev(out, 'out')], out


def remainder_snapshot(packed, shape, e, packed_w, bias, act, h):
    """rest @ act(e W + b) in one launch with x_e kept in LDS (uds_remainder_snapshot): the operands of remainder_forward_dense, no
    workspace; shapes remainder_snapshot_plan accepts.  e (..., M, F) -> (..., R, h)."""
    entry = 'uds_remainder_snapshot'
    S, F, args, out = _snapshot_side(entry, (packed, shape, e, packed_w, bias, act, h))
    if S == 0:
        return out
    _check(load().uds_remainder_snapshot(args[0], args[1], args[2], args[3], F, args[4], args[5], ACT[act], S, h, args[6], _stream()), entry)
    return out


def remainder_snapshot_pair(side0, side1):
    """Two remainder_snapshot problems -- the node side and the link side of one layer: argument tuples (packed, shape, e, packed_w,
    bias, act, h) that share F, h, act and the snapshot count -- in ONE launch (uds_remainder_snapshot_pair).  A side given as None
    is skipped (its result is None); both None is an error."""
    entry = 'uds_remainder_snapshot_pair'
    if side0 is None and side1 is None:
        raise UdsError('remainder_snapshot_pair: both sides are None')
    got = [None if sd is None else _snapshot_side(entry, sd) for sd in (side0, side1)]
    live = [(sd, g) for sd, g in zip((side0, side1), got) if sd is not None]
    (first, (S, F, _, _)) = live[0]
    for sd, g in live[1:]:
        if g[0] != S or g[1] != F or sd[5] != first[5] or sd[6] != first[6]:
            raise UdsError('remainder_snapshot_pair: the sides must share S, F, act and h: (%d, %d, %r, %d) against (%d, %d, %r, %d)'
                           % (S, F, first[5], first[6], g[0], g[1], sd[5], sd[6]))
    outs = tuple(None if g is None else g[3] for g in got)
    if S == 0:
        return outs
    none = [None, 0, 0, None, None, None, None]
    a0, a1 = (none if g is None else g[2] for g in got)
    _check(load().uds_remainder_snapshot_pair(*a0, *a1, F, ACT[first[5]], S, first[6], _stream()), entry)
    return outs


def rowgemm_forward(x, packed, bias, f_out, act='linear', taps=1, dilation=1, out=None):
    """Matrix-core Dense (taps=1, any leading dims) or causal Conv1D (x (B,T,R,F), taps = kernel size).  out: the result's
    tensor, allocated when None."""
    lib = load()
    F = x.shape[-1]
    if taps == 1:
        B, T, R = 1, 1, x.numel() // F
        out_shape = tuple(x.shape[:-1]) + (f_out,)
    else:
        if x.dim() != 4:
            raise UdsError('conv needs x (B,T,R,F), got %r' % (tuple(x.shape),))
        B, T, R = x.shape[:3]
        out_shape = (B, T, R, f_out)
    out = _out(out, out_shape, x, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_rowgemm_forward(_dev(x, 'x'), B, T, R, F, packed.data_ptr(), _dev(bias, 'bias', True), taps, dilation, f_out,
                                   ACT[act], _dev(out, 'out'), _stream()), 'uds_rowgemm_forward')
    return out


def rowgemm_forward_pair(x0, packed0, bias0, x1, packed1, bias1, f_out, act='linear', taps=1, dilation=1, out=None):
    """Two causal Conv1D / Dense problems of one layer shape -- x0 (B,T,R0,F), x1 (B,T,R1,F) -- in one launch when both are small
    (uds_rowgemm_forward_pair).  Returns (out0, out1): the tensors of out = (out0, out1) when given, else new ones."""
    lib = load()
    B, T, R0, F = x0.shape
    R1 = x1.shape[2]
    if tuple(x1.shape) != (B, T, R1, F):
        raise UdsError('rowgemm_forward_pair: x0 %r and x1 %r differ in more than the row count' % (tuple(x0.shape), tuple(x1.shape)))
    out0 = _out(None if out is None else out[0], (B, T, R0, f_out), x0, 'out0')
    out1 = _out(None if out is None else out[1], (B, T, R1, f_out), x0, 'out1')
    if out0.numel() and out1.numel():
        _check(lib.uds_rowgemm_forward_pair(_dev(x0, 'x0'), R0, packed0.data_ptr(), _dev(bias0, 'bias0', True), _dev(out0, 'out0'), _dev(x1, 'x1'), R1,
                                            packed1.data_ptr(), _dev(bias1, 'bias1', True), _dev(out1, 'out1'), B, T, F, taps, dilation, f_out,
                                            ACT[act], _stream()), 'uds_rowgemm_forward_pair')
    return out0, out1


def rowgemm_cat(x, x2, packed, bias, f_out, act='linear', out=None, col0=0):
    """Matrix-core Dense on rows [x | x2] (x2 None: x alone) written to columns [col0, col0 + f_out) of `out`
    (..., ldo) -- allocated (..., f_out) when None.  No concatenation copies (uds_rowgemm_forward_cat)."""
    lib = load()
    F1 = x.shape[-1]
    F2 = 0 if x2 is None else x2.shape[-1]
    rows = x.numel() // F1
    if x2 is not None and x2.numel() // F2 != rows:
        raise UdsError('rowgemm_cat: x %r and x2 %r have different row counts' % (tuple(x.shape), tuple(x2.shape)))
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (f_out,), device=x.device, dtype=torch.float32)
    ldo = out.shape[-1]
    if out.numel() // ldo != rows:
        raise UdsError('rowgemm_cat: out %r does not have %d rows' % (tuple(out.shape), rows))
    if rows == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_rowgemm_forward_cat(_dev(x, 'x'), F1, _dev(x2, 'x2', True), F2, 1, 1, rows, packed.data_ptr(), _dev(bias, 'bias', True),
                                       1, 1, f_out, ACT[act], _dev(out, 'out'), ldo, col0, _stream()), 'uds_rowgemm_forward_cat')
    return out


def dense_cumsum(x, packed, bias=None, res=None, act='linear', out=None):
    """act(cumsum over axis 1 of (x @ kernel + bias) + res): x (B,T,R,64), kernel (64,64) packed by rowgemm_pack,
    res (B,1,R,64) -- Dense + prefix sum + residual + activation in one kernel (uds_dense_cumsum).  out: the result's tensor,
    allocated when None."""
    lib = load()
    B, T, R, F = x.shape
    if F != 64:
        raise UdsError('dense_cumsum: 64 -> 64 only, got %d inputs' % F)
    if res is not None and tuple(res.shape) != (B, 1, R, 64):
        raise UdsError('dense_cumsum: res must be %r, got %r' % ((B, 1, R, 64), tuple(res.shape)))
    out = _out(out, (B, T, R, 64), x, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_dense_cumsum(_dev(x, 'x'), B, T, R, packed.data_ptr(), _dev(bias, 'bias', True), _dev(res, 'res', True), ACT[act],
                                _dev(out, 'out'), _stream()), 'uds_dense_cumsum')
    return out


class _Heads(ctypes.Structure):
    _fields_ = [('a_packed', ctypes.c_void_p), ('a_bias', ctypes.c_void_p), ('h_packed', ctypes.c_void_p * 5), ('h_bias', ctypes.c_void_p * 5),
                ('f_packed', ctypes.c_void_p), ('f_bias', ctypes.c_void_p), ('n_a', ctypes.c_int32), ('act_a', ctypes.c_int32),
                ('n_hidden', ctypes.c_int32), ('act_h', ctypes.c_int32), ('act_f', ctypes.c_int32)]


def dense_cumsum_heads(x, packed, bias, res, act, head_a, hidden=(), head_f=None, out=None):
    """uds_dense_cumsum_heads: act(cumsum_t(x @ kernel + bias) + res) consumed by its heads without being written.
    head_a = (packed (64, n_a), bias, n_a, activation); hidden = [(packed, bias), ...] the Dense(32) layers of the second
    head with their common activation in hidden_act = head_f[3]; head_f = (packed (32, 1), bias, activation, hidden activation).
    Returns (B, T, R, n_a + (1 if hidden else 0)): `out` when given, else a new tensor."""
    lib = load()
    B, T, R, F = x.shape
    if F != 64:
        raise UdsError('dense_cumsum_heads: 64 -> 64 only, got %d inputs' % F)
    if res is not None and tuple(res.shape) != (B, 1, R, 64):
        raise UdsError('dense_cumsum_heads: res must be %r, got %r' % ((B, 1, R, 64), tuple(res.shape)))
    hd = _Heads()
    keep = [head_a[0], head_a[1]]
    hd.a_packed, hd.a_bias, hd.n_a, hd.act_a = head_a[0].data_ptr(), _dev(head_a[1], 'a_bias', True), int(head_a[2]), ACT[head_a[3]]
    hd.n_hidden = len(hidden)
    for i, (pk, bs) in enumerate(hidden):
        hd.h_packed[i], hd.h_bias[i] = pk.data_ptr(), _dev(bs, 'h_bias', True)
        keep += [pk, bs]
    if hidden:
        hd.f_packed, hd.f_bias, hd.act_f, hd.act_h = head_f[0].data_ptr(), _dev(head_f[1], 'f_bias', True), ACT[head_f[2]], ACT[head_f[3]]
        keep += [head_f[0], head_f[1]]
    out = _out(out, (B, T, R, hd.n_a + (1 if hidden else 0)), x, 'out')
    if out.numel():
        _check(lib.uds_dense_cumsum_heads(_dev(x, 'x'), B, T, R, packed.data_ptr(), _dev(bias, 'bias', True), _dev(res, 'res', True), ACT[act],
                                          ctypes.byref(hd), _dev(out, 'out'), _stream()), 'uds_dense_cumsum_heads')
    return out


class _ConvStack(ctypes.Structure):
    """uds_conv_stack_t"""
    _fields_ = [('packed', ctypes.c_void_p * 3), ('bias', ctypes.c_void_p * 3), ('n_layers', ctypes.c_int32), ('act', ctypes.c_int32)]


def conv_stack_plan(B, T, R, L):
    """(n_seg, seg_len, halo): the time segmentation conv_stack_forward uses for n_seg = 0 (uds_conv_stack_plan, host only)."""
    n_seg, seg_len, halo = _c_i64(), _c_i64(), _c_i64()
    _check(load().uds_conv_stack_plan(B, T, R, L, ctypes.byref(n_seg), ctypes.byref(seg_len), ctypes.byref(halo)), 'uds_conv_stack_plan')
    return n_seg.value, seg_len.value, halo.value


def conv_stack_forward(x, layers, act='linear', n_seg=0, out=None):
    """A stack of len(layers) (2 or 3) causal Conv1D(64 -> 64, kernel 3) layers with dilations 1, 2[, 4] and one activation in ONE
    launch (uds_conv_stack_forward): x (B,T,R,64), layers = [(packed, bias), ...] with packed = rowgemm_pack of the layer's
    (192, 64) kernel and bias (64,) or None.  Bit-identical to the layers run one by one on the streaming-Conv1D route.  n_seg = 0:
    the planner's time segmentation, else that many segments.  out: the result's tensor, allocated when None."""
    lib = load()
    if x.dim() != 4 or x.shape[-1] != 64:
        raise UdsError('conv_stack_forward: needs x (B,T,R,64), got %r' % (tuple(x.shape),))
    B, T, R = x.shape[:3]
    st = _ConvStack()
    st.n_layers, st.act = len(layers), ACT[act]
    for i, (pk, bs) in enumerate(layers[:3]):
        st.packed[i], st.bias[i] = pk.data_ptr(), _dev(bs, 'bias', True)
    out = _out(out, (B, T, R, 64), x, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_conv_stack_forward(_dev(x, 'x'), B, T, R, ctypes.byref(st), int(n_seg), _dev(out, 'out'), _stream()),
           'uds_conv_stack_forward')
    return out


def cumsum_act(x, res=None, act='linear', out=None):
    """act(cumsum over axis 1 of x (B,T,R,F) + res (B,1,R,F)).  out: the caller's result tensor."""
    lib = load()
    B, T, R, F = x.shape
    if res is not None and tuple(res.shape) != (B, 1, R, F):
        raise UdsError('cumsum_act: res must be %r, got %r' % ((B, 1, R, F), tuple(res.shape)))
    out = _out(out, x.shape, x, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_cumsum_act(_dev(x, 'x'), _dev(res, 'res', True), B, T, R, F, ACT[act], _dev(out, 'out'), _stream()),
           'uds_cumsum_act')
    return out


ADAM_SPAN, ADAM_TABLE = 4096, 64      # elements per workgroup and tensors per launch of uds_adam_step (csrc/kernels_optim.hpp)


def adam_workspace_floats(numels):
    """Floats of workspace uds_adam_step needs for tensors of these sizes (one double per workgroup)."""
    arr = (_c_i64 * len(numels))(*[int(n) for n in numels])
    need = int(load().uds_adam_workspace_floats(arr, len(numels)))
    if need < 0:
        raise UdsError('uds_adam_workspace_floats: bad sizes %r' % (list(numels),))
    return need


def adam_step(ps, gs, ms, vs, state, workspace, loss=None, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None):
    """One Keras-Adam step with per-variable clipnorm on lists of contiguous fp32 device tensors (include/uds_hip.h:
    uds_adam_step), in place on ps, ms, vs.  state: int32[4] device tensor ([0] step count, [1] status of this call), zero
    before the first step; workspace: fp32 device tensor of adam_workspace_floats(...) elements whose storage is 8-byte
    aligned; loss: a 0-d / 1-element fp32 device tensor or None.  No allocation, copy or synchronisation: capture-safe."""
    if not (len(ps) == len(gs) == len(ms) == len(vs)):
        raise UdsError('adam_step: %d parameters, %d gradients, %d / %d moments' % (len(ps), len(gs), len(ms), len(vs)))
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.int32 or state.numel() != 4 or not state.is_contiguous():
        raise UdsError('state must be a contiguous int32 HIP tensor of 4 elements')
    _same_device(state.device.index, 'state')
    table = (AdamTensor * max(len(ps), 1))()
    for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
        if not (tuple(g.shape) == tuple(p.shape) == tuple(m.shape) == tuple(v.shape)):
            raise UdsError('adam_step: tensor %d: parameter %r, gradient %r, moments %r / %r' % (i, tuple(p.shape), tuple(g.shape), tuple(m.shape),
                                                                                                 tuple(v.shape)))
        if p.numel() == 0:
            for t, name in ((p, 'p'), (g, 'g'), (m, 'm'), (v, 'v')):
                _nothing_to_launch(t, '%s[%d]' % (name, i), None)
            continue
        table[i] = AdamTensor(_dev(p, 'p[%d]' % i), _dev(g, 'g[%d]' % i), _dev(m, 'm[%d]' % i), _dev(v, 'v[%d]' % i), p.numel())
    if loss is not None and loss.numel() != 1:
        raise UdsError('loss must hold one element, got %r' % (tuple(loss.shape),))
    _check(load().uds_adam_step(table, len(ps), _dev(loss, 'loss', True), float(lr), float(beta_1), float(beta_2), float(epsilon),
                                0.0 if clipnorm is None else float(clipnorm), state.data_ptr(), _dev(workspace, 'workspace'), workspace.numel(),
                                _stream()), 'uds_adam_step')


WINDOW_DRAW_MAX = 4096                # starts per uds_window_draw call (csrc/kernels_data.hpp)


def _dev_i64(t, name):
    """Device pointer of a contiguous int64 HIP tensor (the 64-bit prefix sums and the draw count of uds_window_draw)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous():
        raise UdsError('%s must be a contiguous int64 HIP tensor' % name)
    _same_device(t.device.index, name)
    return t.data_ptr()


def window_batch(states, flood, edge_states, settings, tide, starts, seq_in, t_out, if_flood, norms=None, out=None):
    """(x, a, b, y, ex, ey) of the B sliding windows at `starts` (int32 device tensor) of the time-major device series, in ONE
    launch (uds_window_batch; include/uds_hip.h gives the channels).  norms: None (raw) or {'x' | 'b' | 'y' | 'e': (span, min)}
    device tensors of the output's channel count ('e': 4).  `a` is None without settings.  A start outside the series fills its
    window with NaN.  out: the six tensors of an earlier call (a: None without settings) to fill again."""
    what = 'window_batch'
    if not (isinstance(states, torch.Tensor) and states.dim() == 3 and states.shape[2] == 4):
        raise UdsError('%s: states must be (Ttot, N, 4)' % what)
    Ttot, N = states.shape[:2]
    if not (isinstance(edge_states, torch.Tensor) and edge_states.dim() == 3 and edge_states.shape[0] == Ttot and edge_states.shape[2] == 4):
        raise UdsError('%s: edge_states must be (%d, E, 4)' % (what, Ttot))
    E = edge_states.shape[1]
    for name, t in (('flood', flood), ('tide', tide)):
        if not (name == 'tide' and t is None) and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (Ttot, N)):
            raise UdsError('%s: %s must be (%d, %d)' % (what, name, Ttot, N))
    if settings is not None and (settings.dim() != 2 or settings.shape[0] != Ttot or settings.shape[1] < 1):
        raise UdsError('%s: settings must be (%d, n_act >= 1)' % (what, Ttot))
    n_act = 0 if settings is None else settings.shape[1]
    if starts.dim() != 1:
        raise UdsError('%s: starts must be one-dimensional' % what)
    B, cx, cb = starts.shape[0], 5 if if_flood else 4, 1 if tide is None else 2
    shapes = ((B, seq_in, N, cx), (B, t_out, n_act), (B, t_out, N, cb), (B, t_out, N, cx), (B, seq_in, E, 4), (B, t_out, E, 3))
    out = [None] * 6 if out is None else list(out)
    for i, name in enumerate(('x', 'a', 'b', 'y', 'ex', 'ey')):
        out[i] = None if name == 'a' and settings is None else _out(out[i], shapes[i], states, name)
    series = WindowSeries(_dev(states, 'states'), _dev(flood, 'flood'), _dev(edge_states, 'edge_states'), _dev(settings, 'settings', True),
                          _dev(tide, 'tide', True), Ttot, N, E, n_act)
    norm = None
    if norms is not None:
        norm = WindowNorm()
        for item, c, rows in (('x', cx, N), ('b', cb, N), ('y', cx, N), ('e', 4, E)):
            if norms.get(item) is not None:
                for part, t in zip(('span', 'min'), norms[item]):
                    if tuple(t.shape) != (rows, c):
                        raise UdsError('%s: norm %r %s must be (%d, %d), got %r' % (what, item, part, rows, c, tuple(t.shape)))
                    setattr(norm, '%s_%s' % (part, item), _dev(t, 'norm %s %s' % (item, part)))
    if B == 0:
        return tuple(out)
    _check(load().uds_window_batch(ctypes.byref(series), None if norm is None else ctypes.byref(norm), _dev_i32(starts, 'starts'), B,
                                   int(seq_in), int(t_out), int(bool(if_flood)), *[None if t is None else t.data_ptr() for t in out], _stream()),
           'uds_window_batch')
    return tuple(out)


def window_draw(table, cum, seed, count, B, out=None):
    """B window starts (int32 device tensor) drawn from `table` (W int32 starts) with the inclusive 64-bit prefix sums `cum` of
    their integer weights (uds_window_draw): draw i uses the stream index count + i (Philox4x32-10, key = seed); afterwards
    count (one int64 device element) is count + B.  Device only; nothing is read back."""
    if not isinstance(table, torch.Tensor) or not isinstance(cum, torch.Tensor) or table.dim() != 1 or tuple(cum.shape) != tuple(table.shape):
        raise UdsError('window_draw: table and cum must be one-dimensional tensors of one length')
    if not isinstance(count, torch.Tensor) or count.numel() != 1:
        raise UdsError('window_draw: count must be one int64 device element')
    if out is None:
        _dev_i32(table, 'table')
        out = torch.empty(int(B), device=table.device, dtype=torch.int32)
    elif tuple(out.shape) != (int(B),):
        raise UdsError('window_draw: out must be (%d,), got %r' % (int(B), tuple(out.shape)))
    _check(load().uds_window_draw(_dev_i32(table, 'table'), _dev_i64(cum, 'cum'), table.shape[0], int(B),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, _dev_i64(count, 'count'), _dev_i32(out, 'out'), _stream()),
           'uds_window_draw')
    return out


CE_MAX = 1024                         # candidates and variables of a cross-entropy call (csrc/kernels_mpc.hpp)


def _mpc_objective_operands(what, preds, q_in0, w_flood, w_out, w_smooth, gamma):
    """Shapes of the objective operands -> (pop, T, N, C, q0_stride)."""
    if not isinstance(preds, torch.Tensor) or preds.dim() != 4:
        raise UdsError('%s: preds must be (pop, T, N, C)' % what)
    pop, T, N, C = preds.shape
    if tuple(q_in0.shape) not in ((N,), (pop, N)):
        raise UdsError('%s: q_in0 must be (%d,) or (%d, %d), got %r' % (what, N, pop, N, tuple(q_in0.shape)))
    for name, w in (('w_flood', w_flood), ('w_out', w_out), ('w_smooth', w_smooth)):
        if w is not None and tuple(w.shape) != (N,):
            raise UdsError('%s: %s must be (%d,), got %r' % (what, name, N, tuple(w.shape)))
    if gamma is not None and tuple(gamma.shape) != (T,):
        raise UdsError('%s: gamma must be (%d,), got %r' % (what, T, tuple(gamma.shape)))
    return pop, T, N, C, (N if q_in0.dim() == 2 else 0)


def mpc_objective(preds, q_in0, w_flood=None, w_out=None, w_smooth=None, gamma=None, out=None):
    """The scenario objective (pop,) of pop predicted horizons preds (pop, T, N, C) (uds_mpc_objective; include/uds_hip.h gives
    the definition): q_in0 (N,) shared or (pop, N), dense per-node weights (N,) or None, gamma (T,) or None."""
    what = 'mpc_objective'
    pop, T, N, C, q0 = _mpc_objective_operands(what, preds, q_in0, w_flood, w_out, w_smooth, gamma)
    out = _out(out, (pop,), preds, 'out')
    if pop == 0:
        return _nothing_to_launch(q_in0, 'q_in0', out)
    _check(load().uds_mpc_objective(_dev(preds, 'preds'), _dev(q_in0, 'q_in0'), q0, pop, T, N, C, _dev(w_flood, 'w_flood', True),
                                    _dev(w_out, 'w_out', True), _dev(w_smooth, 'w_smooth', True), _dev(gamma, 'gamma', True), _dev(out, 'out'),
                                    _stream()), 'uds_mpc_objective')
    return out


def mpc_objective_backward(preds, q_in0, g, w_flood=None, w_out=None, w_smooth=None, gamma=None, out=None):
    """d_preds (pop, T, N, C) of sum_p g[p] * mpc_objective(...)[p] (uds_mpc_objective_backward): every element written."""
    what = 'mpc_objective_backward'
    pop, T, N, C, q0 = _mpc_objective_operands(what, preds, q_in0, w_flood, w_out, w_smooth, gamma)
    if tuple(g.shape) != (pop,):
        raise UdsError('%s: g must be (%d,), got %r' % (what, pop, tuple(g.shape)))
    out = _out(out, preds.shape, preds, 'out')
    if pop == 0:
        return _nothing_to_launch(q_in0, 'q_in0', out)
    _check(load().uds_mpc_objective_backward(_dev(preds, 'preds'), _dev(q_in0, 'q_in0'), q0, _dev(g, 'g'), pop, T, N, C, _dev(w_flood, 'w_flood', True),
                                             _dev(w_out, 'w_out', True), _dev(w_smooth, 'w_smooth', True), _dev(gamma, 'gamma', True),
                                             _dev(out, 'out'), _stream()), 'uds_mpc_objective_backward')
    return out


def ce_draw(mean, std, seed, count, pop, out=None):
    """pop candidates (pop, n_var) from N(mean, std) clipped to [0, 1] (uds_ce_draw): candidate i uses the stream index count + i
    (Philox4x32-10, key = seed, counter (index, variable)); afterwards count (one int64 device element) is count + pop.  Device
    only; nothing is read back."""
    if not isinstance(mean, torch.Tensor) or not isinstance(std, torch.Tensor) or mean.dim() != 1 or tuple(std.shape) != tuple(mean.shape):
        raise UdsError('ce_draw: mean and std must be one-dimensional tensors of one length')
    if not isinstance(count, torch.Tensor) or count.numel() != 1:
        raise UdsError('ce_draw: count must be one int64 device element')
    out = _out(out, (int(pop), mean.shape[0]), mean, 'out')
    _check(load().uds_ce_draw(_dev(mean, 'mean'), _dev(std, 'std'), mean.shape[0], int(pop), int(seed) & 0xFFFFFFFFFFFFFFFF, _dev_i64(count, 'count'),
                              _dev(out, 'out'), _stream()), 'uds_ce_draw')
    return out


def ce_update(y, obj, n_elite, smooth, std_min, mean, std, best_y, best_obj, status):
    """One cross-entropy update in place on mean, std (n_var,), best_y (n_var,), best_obj (1,) and status (int32, [0] raised when
    no candidate is finite) from the candidates y (pop, n_var) and their objectives obj (pop,) (uds_ce_update).  Device only;
    nothing is read back."""
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise UdsError('ce_update: y must be (pop, n_var)')
    pop, n_var = y.shape
    for name, t, shape in (('obj', obj, (pop,)), ('mean', mean, (n_var,)), ('std', std, (n_var,)), ('best_y', best_y, (n_var,))):
        if tuple(t.shape) != shape:
            raise UdsError('ce_update: %s must be %r, got %r' % (name, shape, tuple(t.shape)))
    if best_obj.numel() != 1 or status.numel() < 1:
        raise UdsError('ce_update: best_obj must hold one element and status at least one')
    _check(load().uds_ce_update(_dev(y, 'y'), _dev(obj, 'obj'), pop, n_var, int(n_elite), float(smooth), float(std_min), _dev(mean, 'mean'),
                                _dev(std, 'std'), _dev(best_y, 'best_y'), _dev(best_obj, 'best_obj'), _dev_i32(status, 'status'), _stream()),
           'uds_ce_update')


def flow_balance(handle, sign, flow, scale_in, scale_out):
    """Link -> node flow balance (emulator.py:717-724): flow (S,E) -> q_in, q_out (S,N)."""
    lib = load()
    if flow.dim() != 2 or flow.shape[1] != handle.n_cols:
        raise UdsError('flow must be (S,%d), got %r' % (handle.n_cols, tuple(flow.shape)))
    S = flow.shape[0]
    q_in = torch.empty((S, handle.n_rows), device=flow.device, dtype=torch.float32)
    q_out = torch.empty_like(q_in)
    if q_in.numel() == 0:
        return q_in, q_out
    _check(lib.uds_flow_balance(handle.ptr, _dev(sign, 'sign'), _dev(flow, 'flow'), S, _dev(scale_in, 'scale_in'),
                                _dev(scale_out, 'scale_out'), _dev(q_in, 'q_in'), _dev(q_out, 'q_out'), _stream()),
           'uds_flow_balance')
    return q_in, q_out


def roll_update(handle, sign, span_e, mini_e, scale_in, scale_out, y, ey, b, x, ex, flood, preds=None):
    """The post-forward part of one autoregressive chunk (include/uds_hip.h: uds_roll_update): returns preds (B,so,N,cy+2)
    (the tensor `preds` when given, else a new one) and shifts the state windows x (B,T,N,cy+3), ex (B,T,E,ce+1) IN PLACE,
    feeding the prediction back."""
    lib = load()
    B, so, N, cy = y.shape
    ce, T = ey.shape[-1], x.shape[1]
    if (tuple(ey.shape[:3]) != (B, so, handle.n_cols) or tuple(b.shape) != (B, so, N, 1) or tuple(x.shape) != (B, T, N, cy + 3) or
            tuple(ex.shape) != (B, T, handle.n_cols, ce + 1) or N != handle.n_rows):
        raise UdsError('roll_update: inconsistent shapes y %r ey %r b %r x %r ex %r' % tuple(tuple(t.shape) for t in (y, ey, b, x, ex)))
    if not (x.is_contiguous() and ex.is_contiguous()):
        raise UdsError('roll_update: the state windows are updated in place and must be contiguous')
    preds = _out(preds, (B, so, N, cy + 2), y, 'preds')
    _check(lib.uds_roll_update(handle.ptr, _dev(sign, 'sign'), _dev(span_e, 'span_e'), _dev(mini_e, 'mini_e'), _dev(scale_in, 'scale_in'),
                               _dev(scale_out, 'scale_out'), _dev(y.contiguous(), 'y'), cy, _dev(ey.contiguous(), 'ey'), ce, _dev(b.contiguous(), 'b'),
                               B, so, T, int(bool(flood)), _dev(x, 'x'), _dev(ex, 'ex'), _dev(preds, 'preds'), _stream()), 'uds_roll_update')
    return preds


class TailParams(ctypes.Structure):
    """uds_tail_t"""
    SIZES = ('N', 'E', 'cy', 'ce', 'n_act', 'b_channels')
    SWITCHES = ('edge_fusion', 'tide', 'has_offset', 'act', 'pump_override', 'any_pump', 'if_flood')
    FLOAT_TABLES = ('is_outfall', 'hmin', 'hmax', 'area_eps', 'ps', 'pump_in', 'pump_out', 'ny_in', 'ny_out', 'scale_in', 'scale_out',
                    'span_y', 'mini_y', 'offset', 'pump', 'pump_mask', 'pump_den', 'ehmax', 'from_ok', 'span_e', 'mini_e', 'link_sign')
    INT_TABLES = ('from_node', 'act_link', 'act_in', 'act_out', 'link_node', 'al_ptr', 'al_idx', 'ai_ptr', 'ai_idx', 'ao_ptr', 'ao_idx')
    _fields_ = ([(n, ctypes.c_int32) for n in SIZES + SWITCHES] + [('depth_gate', ctypes.c_float), ('epsilon', ctypes.c_float)] +
                [(n, _c_ptr) for n in ('is_outfall', 'hmin', 'hmax', 'area_eps', 'ps', 'pump_in', 'pump_out', 'ny_in', 'ny_out', 'scale_in',
                                       'scale_out', 'span_y', 'mini_y', 'offset', 'pump', 'pump_mask', 'pump_den', 'ehmax', 'from_ok',
                                       'span_e', 'mini_e', 'from_node', 'act_link', 'act_in', 'act_out', 'link_node', 'link_sign',
                                       'al_ptr', 'al_idx', 'ai_ptr', 'ai_idx', 'ao_ptr', 'ao_idx')])


class TailSpec:
    """The constants of one model's predict tail on one device: `tables` name -> device tensor (fp32, or int32 for
    TailParams.INT_TABLES; the tensors are kept alive here), `scalars` the sizes and switches.  struct(depth_gate, pump_override)
    fills a uds_tail_t for one mode."""

    def __init__(self, tables, **scalars):
        self.tables, self.scalars = dict(tables), dict(scalars)
        for n in TailParams.FLOAT_TABLES:
            _dev(self.tables[n], n)
        for n in TailParams.INT_TABLES:
            _dev_i32(self.tables[n], n)

    def struct(self, depth_gate, pump_override):
        p = TailParams()
        for n in TailParams.SIZES + TailParams.SWITCHES:
            if n != 'pump_override':
                setattr(p, n, int(self.scalars[n]))
        p.pump_override, p.depth_gate, p.epsilon = int(bool(pump_override)), float(depth_gate), float(self.scalars['epsilon'])
        for n in TailParams.FLOAT_TABLES + TailParams.INT_TABLES:
            t = self.tables[n]
            setattr(p, n, t.data_ptr() if t.numel() else None)
        return p


def _tail_operands(handle, spec, y, ey, a, b_norm, runoff, h0):
    s = spec.scalars
    B, T = y.shape[:2]
    N, E = s['N'], s['E']
    want = dict(y=(B, T, N, s['cy']), ey=(B, T, E, s['ce']), b_norm=(B, T, N, s['b_channels']), runoff=(B, T, N), h0=(B, N))
    if s['act']:
        want['a'] = (B, T, s['n_act'])
    got = dict(y=y, ey=ey, a=a, b_norm=b_norm, runoff=runoff, h0=h0)
    for name, shape in want.items():
        if got[name] is None or tuple(got[name].shape) != shape:
            raise UdsError('predict_tail: %s must be %r, got %r' % (name, shape, None if got[name] is None else tuple(got[name].shape)))
    if handle.n_rows != N or handle.n_cols != E:
        raise UdsError('predict_tail: the incidence pattern is %d x %d, the model has %d nodes and %d links' % (handle.n_rows, handle.n_cols, N, E))
    return B, T


def predict_tail(handle, sign, spec, y, ey, a, b_norm, runoff, h0, depth_gate=0.0, pump_override=False, out_y=None, out_ey=None):
    """Everything after the network forward of Emulator.predict_tf / predict (include/uds_hip.h: uds_predict_tail): returns
    out_y (B,T,N,4 or 5) and out_ey (B,T,E,ce).  spec: a TailSpec."""
    lib = load()
    B, T = _tail_operands(handle, spec, y, ey, a, b_norm, runoff, h0)
    s = spec.scalars
    out_y = _out(out_y, (B, T, s['N'], 4 + int(bool(s['if_flood']))), y, 'out_y')
    out_ey = _out(out_ey, (B, T, s['E'], s['ce']), y, 'out_ey')
    if out_y.numel() == 0:
        return out_y, out_ey
    p = spec.struct(depth_gate, pump_override)
    _check(lib.uds_predict_tail(handle.ptr, _dev(sign, 'sign'), ctypes.addressof(p), _dev(y, 'y'), _dev(ey, 'ey'), _dev(a, 'a', not s['act']),
                                _dev(b_norm, 'b_norm'), _dev(runoff, 'runoff'), _dev(h0, 'h0'), B, T, _dev(out_y, 'out_y'), _dev(out_ey, 'out_ey'),
                                _stream()), 'uds_predict_tail')
    return out_y, out_ey


def predict_tail_backward(handle, sign, spec, y, ey, a, b_norm, runoff, h0, g_out_y, g_out_ey, depth_gate=0.0, pump_override=False):
    """Reverse mode of predict_tail: (dy, dey, da or None, dh0) for the upstream gradients of both outputs."""
    lib = load()
    B, T = _tail_operands(handle, spec, y, ey, a, b_norm, runoff, h0)
    s = spec.scalars
    if tuple(g_out_y.shape) != (B, T, s['N'], 4 + int(bool(s['if_flood']))) or tuple(g_out_ey.shape) != tuple(ey.shape):
        raise UdsError('predict_tail_backward: gradients %r / %r do not have the shapes of the outputs' % (tuple(g_out_y.shape), tuple(g_out_ey.shape)))
    dy, dey, dh0 = torch.empty_like(y), torch.empty_like(ey), torch.empty_like(h0)
    da = torch.empty_like(a) if s['act'] else None
    if dy.numel() == 0:
        return dy, dey, da, dh0
    ws = torch.empty(int(lib.uds_predict_tail_workspace_floats(s['N'], s['E'], B, T)), device=y.device, dtype=torch.float32)
    p = spec.struct(depth_gate, pump_override)
    _check(lib.uds_predict_tail_backward(handle.ptr, _dev(sign, 'sign'), ctypes.addressof(p), _dev(y, 'y'), _dev(ey, 'ey'), _dev(a, 'a', not s['act']),
                                         _dev(b_norm, 'b_norm'), _dev(runoff, 'runoff'), _dev(h0, 'h0'), B, T, _dev(g_out_y, 'g_out_y'),
                                         _dev(g_out_ey, 'g_out_ey'), _dev(dy, 'dy'), _dev(dey, 'dey'), _dev(da, 'da', not s['act']), _dev(dh0, 'dh0'),
                                         _dev(ws, 'workspace'), _stream()), 'uds_predict_tail_backward')
    return dy, dey, da, dh0


def _fit_tail_operands(what, handle, spec, y, ey, a, b_norm, y_true, ey_true, lw):
    """The checks uds_fit_tail and uds_fit_tail_backward share -> (B, T, cyt, balance, the ABI's leading arguments).  lw: the loss
    operands, nwei (N, 3 + balance) / poswei (N) / ewei (E) and, with balance, qw_den / span_b / mini_b (N)."""
    s = spec.scalars
    if y is None or y.dim() != 4:
        raise UdsError('%s: y must be (B, T, N, cy)' % what)
    B, T = y.shape[:2]
    N, E = s['N'], s['E']
    balance = int(bool(lw.get('balance')))
    cyt = int(y_true.shape[-1]) if isinstance(y_true, torch.Tensor) and y_true.dim() == 4 else 0
    want = dict(y=(B, T, N, s['cy']), ey=(B, T, E, s['ce']), b_norm=(B, T, N, s['b_channels']), y_true=(B, T, N, cyt), ey_true=(B, T, E, s['ce']),
                nwei=(N, 3 + balance), poswei=(N,), ewei=(E,))
    if s['act']:
        want['a'] = (B, T, s['n_act'])
    if balance:
        want.update(qw_den=(N,), span_b=(N,), mini_b=(N,))
    got = dict(y=y, ey=ey, a=a, b_norm=b_norm, y_true=y_true, ey_true=ey_true, **{k: lw.get(k) for k in ('nwei', 'poswei', 'ewei', 'qw_den', 'span_b', 'mini_b')})
    for name, shape in want.items():
        if not isinstance(got[name], torch.Tensor) or tuple(got[name].shape) != shape:
            raise UdsError('%s: %s must be %r, got %r' % (what, name, shape, tuple(got[name].shape) if isinstance(got[name], torch.Tensor) else got[name]))
        if got[name].dtype != torch.float32:
            raise UdsError('%s: %s must be float32, got %s' % (what, name, got[name].dtype))
    if cyt < 3:
        raise UdsError('%s: y_true needs at least 3 channels, got %d' % (what, cyt))
    if handle.n_rows != N or handle.n_cols != E:
        raise UdsError('%s: the incidence pattern is %d x %d, the model has %d nodes and %d links' % (what, handle.n_rows, handle.n_cols, N, E))
    opt = lambda k: _dev(lw[k], k) if balance else None
    return B, T, cyt, balance, lambda p: (
        handle.ptr, _dev(lw['sign'], 'sign'), ctypes.addressof(p), _dev(y, 'y'), _dev(ey, 'ey'), _dev(a, 'a') if s['act'] else None,
        _dev(b_norm, 'b_norm'), _dev(y_true, 'y_true'), _dev(ey_true, 'ey_true'), _dev(lw['nwei'], 'nwei'), _dev(lw['poswei'], 'poswei'),
        _dev(lw['ewei'], 'ewei'), opt('qw_den'), opt('span_b'), opt('mini_b'), B, T, cyt, balance)


def fit_tail(handle, spec, y, ey, a, b_norm, y_true, ey_true, lw, pump_override=False, out_y=None, out_ey=None):
    """Everything after the network forward of Emulator.fit_eval (include/uds_hip.h: uds_fit_tail): returns out_y (B,T,N,3 or 4) and
    out_ey (B,T,E,ce), what post_proc_tf returns, and loss_sums (3,) = the node / flood / edge loss sums before the division by the
    sample count.  spec: a TailSpec; lw: the loss operands plus 'sign', the incidence values (see _fit_tail_operands)."""
    lib = load()
    B, T, cyt, balance, lead = _fit_tail_operands('fit_tail', handle, spec, y, ey, a, b_norm, y_true, ey_true, lw)
    s = spec.scalars
    out_y = _out(out_y, (B, T, s['N'], 3 + int(bool(s['if_flood']))), y, 'out_y')
    out_ey = _out(out_ey, (B, T, s['E'], s['ce']), y, 'out_ey')
    if out_y.numel() == 0:
        return out_y, out_ey, torch.zeros(3, device=y.device, dtype=torch.float32)
    sums = torch.empty(3, device=y.device, dtype=torch.float32)
    ws = torch.empty(int(lib.uds_fit_tail_workspace_floats(s['N'], s['E'], B, T)), device=y.device, dtype=torch.float32)
    p = spec.struct(0.0, pump_override)
    _check(lib.uds_fit_tail(*lead(p), _dev(out_y, 'out_y'), _dev(out_ey, 'out_ey'), _dev(sums, 'loss_sums'), _dev(ws, 'workspace'), _stream()),
           'uds_fit_tail')
    return out_y, out_ey, sums


def fit_tail_backward(handle, spec, y, ey, a, b_norm, y_true, ey_true, lw, g_loss, g_out_y=None, g_out_ey=None, pump_override=False):
    """Reverse mode of fit_tail: (dy, dey) for g_loss (3,) on the device and the optional gradients arriving at out_y / out_ey."""
    lib = load()
    B, T, cyt, balance, lead = _fit_tail_operands('fit_tail_backward', handle, spec, y, ey, a, b_norm, y_true, ey_true, lw)
    s = spec.scalars
    if not isinstance(g_loss, torch.Tensor) or tuple(g_loss.shape) != (3,):
        raise UdsError('fit_tail_backward: g_loss must be (3,), got %r' % (tuple(g_loss.shape) if isinstance(g_loss, torch.Tensor) else g_loss,))
    if ((g_out_y is not None and tuple(g_out_y.shape) != (B, T, s['N'], 3 + int(bool(s['if_flood'])))) or
            (g_out_ey is not None and tuple(g_out_ey.shape) != tuple(ey.shape))):
        raise UdsError('fit_tail_backward: the gradients of out_y / out_ey do not have the shapes of the outputs')
    dy, dey = torch.empty_like(y), torch.empty_like(ey)
    if dy.numel() == 0:
        return dy, dey
    ws = torch.empty(int(lib.uds_fit_tail_workspace_floats(s['N'], s['E'], B, T)), device=y.device, dtype=torch.float32)
    p = spec.struct(0.0, pump_override)
    _check(lib.uds_fit_tail_backward(*lead(p), _dev(g_loss, 'g_loss'), _dev(g_out_y, 'g_out_y', True), _dev(g_out_ey, 'g_out_ey', True),
                                     _dev(dy, 'dy'), _dev(dey, 'dey'), _dev(ws, 'workspace'), _stream()), 'uds_fit_tail_backward')
    return dy, dey


def csr_spmm(handle, val, x, bias=None, act='linear', out=None):
    """out[s,r,:] = act(sum_p val[p] x[s,col[p],:] + bias); x:(S,n_cols,F) -> (S,n_rows,F).  out: the caller's result tensor."""
    lib = load()
    if x.dim() != 3 or x.shape[1] != handle.n_cols:
        raise UdsError('x must be (S,%d,F), got %r' % (handle.n_cols, tuple(x.shape)))
    if val is not None and val.numel() != handle.nnz:
        raise UdsError('val has %d entries, pattern has %d' % (val.numel(), handle.nnz))
    S, _, F = x.shape
    out = _out(out, (S, handle.n_rows, F), x, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(x, 'x', out)
    _check(lib.uds_csr_spmm(handle.ptr, _dev(val, 'val', True), _dev(x, 'x'), S, F, _dev(bias, 'bias', True), ACT[act],
                            _dev(out, 'out'), _stream()), 'uds_csr_spmm')
    return out


def gat_forward(handle, xa, kernel, a_self, a_nbr, bias=None, act='relu', xb=None, return_workspace=False, out=None, workspace=None):
    """Single-head GATConv over a CSR pattern with self loops; xa:(S,n,fa) [| xb:(S,n,fb)] -> (S,n,d).
    return_workspace=True also returns (hx (S,n,d), s_self (S,n), s_nbr (S,n)) -- views of the workspace, for the
    backward pass.  out / workspace (uds_gat_workspace_floats(n, S, d) floats): the caller's tensors."""
    lib = load()
    if xa.dim() != 3 or xa.shape[1] != handle.n_rows:
        raise UdsError('x must be (S,%d,F), got %r' % (handle.n_rows, tuple(xa.shape)))
    S, n, fa = xa.shape
    fb = 0 if xb is None else xb.shape[-1]
    d = kernel.shape[-1]
    if kernel.numel() != (fa + fb) * d:
        raise UdsError('kernel %r does not match %d input features' % (tuple(kernel.shape), fa + fb))
    out = _out(out, (S, n, d), xa, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(xa, 'xa', out)
    ws = _out(workspace, (lib.uds_gat_workspace_floats(n, S, d),), xa, 'workspace')
    _check(lib.uds_gat_forward(handle.ptr, _dev(xa, 'xa'), fa, _dev(xb, 'xb', True), fb, S, _dev(kernel, 'kernel'),
                               _dev(a_self, 'a_self'), _dev(a_nbr, 'a_nbr'), _dev(bias, 'bias', True), d, ACT[act],
                               _dev(ws, 'workspace'), _dev(out, 'out'), _stream()), 'uds_gat_forward')
    if return_workspace:
        m = S * n
        return out, (ws[:m * d].view(S, n, d), ws[m * d:m * d + m].view(S, n), ws[m * d + m:m * d + 2 * m].view(S, n))
    return out


def _gat_aggregate(entry, handle, hx, s_self, s_nbr, bias, act, extra, out):
    """One of the four single-head aggregate entries; extra: its (tensor, name, optional) operands between bias and S."""
    S, _, d = hx.shape
    out = _out(out, hx.shape, hx, 'out')
    if out.numel() == 0:
        return _nothing_to_launch(hx, 'hx', out)
    _check(getattr(load(), entry)(handle.ptr, _dev(hx, 'hx'), _dev(s_self, 's_self'), _dev(s_nbr, 's_nbr'), _dev(bias, 'bias', True),
                                  *[_dev(*op) for op in extra], S, d, ACT[act], _dev(out, 'out'), _stream()), entry)
    return out


def gat_aggregate(handle, hx, s_self, s_nbr, bias=None, act='relu', edge_mask=None, coef=None, out=None):
    """Attention softmax + neighbour sum of a GATConv from precomputed hx (S,n,d), s_self / s_nbr (S,n); out: the caller's result tensor.
    edge_mask (S, nnz): per-snapshot 0/1 over the pattern's entries (`use_adj`; the diagonal always takes part).
    coef (S, nnz): multiplier of the normalised coefficients (Spektral's attention dropout in training, uds_gat_aggregate_coef)."""
    S, n, d = hx.shape
    rows_ok = n == handle.n_rows and tuple(s_self.shape) == (S, n) and tuple(s_nbr.shape) == (S, n)
    if coef is not None:
        if edge_mask is not None:
            raise UdsError('gat_aggregate: edge_mask and coef together are not built')
        if tuple(coef.shape) != (S, handle.nnz) or not rows_ok:
            raise UdsError('gat_aggregate: coef %r / hx %r for %d snapshots of a %d-row, %d-entry pattern' %
                           (tuple(coef.shape), tuple(hx.shape), S, handle.n_rows, handle.nnz))
        return _gat_aggregate('uds_gat_aggregate_coef', handle, hx, s_self, s_nbr, bias, act, [(coef, 'coef')], out)
    if edge_mask is not None:
        if tuple(edge_mask.shape) != (S, handle.nnz):
            raise UdsError('gat_aggregate: edge_mask %r for %d snapshots of a %d-entry pattern' % (tuple(edge_mask.shape), S, handle.nnz))
        if not rows_ok:
            raise UdsError('gat_aggregate: hx %r does not match a %d-row pattern' % (tuple(hx.shape), handle.n_rows))
        return _gat_aggregate('uds_gat_aggregate_masked', handle, hx, s_self, s_nbr, bias, act, [(edge_mask, 'edge_mask')], out)
    if not rows_ok:
        raise UdsError('gat_aggregate: hx %r, s_self %r, s_nbr %r do not match a %d-row pattern' %
                       (tuple(hx.shape), tuple(s_self.shape), tuple(s_nbr.shape), handle.n_rows))
    return _gat_aggregate('uds_gat_aggregate', handle, hx, s_self, s_nbr, bias, act, [], out)


def _gat_backward_outputs(grad, out):
    """(d_hx, ds_self, ds_nbr): the caller's tensors (checked) or new ones."""
    S, n, _ = grad.shape
    o = out if out is not None else (None, None, None)
    return _out(o[0], grad.shape, grad, 'd_hx'), _out(o[1], (S, n), grad, 'ds_self'), _out(o[2], (S, n), grad, 'ds_nbr')


def _gat_backward(entry, handle, handle_t, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, extra, out, workspace):
    """uds_gat_backward_coef or uds_gat_backward_ex; extra: its (tensor, name, optional) operands between a_nbr and S."""
    S, n, d = grad.shape
    d_hx, ds_self, ds_nbr = _gat_backward_outputs(grad, out)
    if grad.numel() == 0:
        return _nothing_to_launch(grad, 'grad', (d_hx, ds_self, ds_nbr))
    ws = _out(workspace, (2, S, max(handle.nnz, 1)), grad, 'workspace')      # alpha and de per pattern entry
    _check(getattr(load(), entry)(handle.ptr, handle_t.ptr, _dev_i32(perm_t, 'perm_t'), _dev(grad, 'grad'), _dev(hx, 'hx'),
                                  _dev(s_self, 's_self'), _dev(s_nbr, 's_nbr'), _dev(a_self, 'a_self'), _dev(a_nbr, 'a_nbr'),
                                  *[_dev(*op) for op in extra], S, d, _dev(ws[0], 'alpha_ws'), _dev(ws[1], 'de_ws'), _dev(d_hx, 'd_hx'),
                                  _dev(ds_self, 'ds_self'), _dev(ds_nbr, 'ds_nbr'), _stream()), entry)
    return d_hx, ds_self, ds_nbr


def gat_backward(handle, handle_t, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, coef=None, out=None, workspace=None):
    """Reverse mode of the attention / aggregation part of gat_forward (uds_gat_backward): grad = dL/d(pre-activation)
    (S,n,d) -> d_hx (S,n,d), ds_self (S,n), ds_nbr (S,n).  coef: the attention-dropout multiplier of the forward pass, if any.
    out: the caller's (d_hx, ds_self, ds_nbr); workspace: the caller's (2, S, max(nnz, 1)) alpha / de scratch."""
    return _gat_backward('uds_gat_backward_coef', handle, handle_t, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, [(coef, 'coef', True)],
                         out, workspace)


def _check_entry_operand(name, t, S, handle):
    if t is not None and tuple(t.shape) != (S, handle.nnz):
        raise UdsError('%s %r for %d snapshots of a %d-entry pattern' % (name, tuple(t.shape), S, handle.nnz))


def gat_aggregate_ex(handle, hx, s_self, s_nbr, bias=None, act='relu', edge_mask=None, coef=None, out=None):
    """gat_aggregate with an optional per-snapshot edge_mask (S, nnz) AND an optional attention-dropout coef (S, nnz) on the
    grouped kernels (uds_gat_aggregate_ex): the training path of `use_adj` GAT layers.  A masked entry leaves the softmax; the
    diagonal always takes part.  With edge_mask = all ones and coef None the result is bitwise that of gat_aggregate."""
    S, n, d = hx.shape
    if n != handle.n_rows or tuple(s_self.shape) != (S, n) or tuple(s_nbr.shape) != (S, n):
        raise UdsError('gat_aggregate_ex: hx %r, s_self %r, s_nbr %r do not match a %d-row pattern' %
                       (tuple(hx.shape), tuple(s_self.shape), tuple(s_nbr.shape), handle.n_rows))
    _check_entry_operand('gat_aggregate_ex: edge_mask', edge_mask, S, handle)
    _check_entry_operand('gat_aggregate_ex: coef', coef, S, handle)
    return _gat_aggregate('uds_gat_aggregate_ex', handle, hx, s_self, s_nbr, bias, act, [(edge_mask, 'edge_mask', True), (coef, 'coef', True)], out)


def gat_backward_ex(handle, handle_t, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, edge_mask=None, coef=None, out=None, workspace=None):
    """Reverse mode of gat_aggregate_ex (uds_gat_backward_ex): outputs, out and workspace as gat_backward.  A masked entry
    contributes nothing."""
    S, n, d = grad.shape
    if n != handle.n_rows or tuple(hx.shape) != (S, n, d) or tuple(s_self.shape) != (S, n) or tuple(s_nbr.shape) != (S, n):
        raise UdsError('gat_backward_ex: grad %r, hx %r, s_self %r, s_nbr %r do not match a %d-row pattern' %
                       (tuple(grad.shape), tuple(hx.shape), tuple(s_self.shape), tuple(s_nbr.shape), handle.n_rows))
    _check_entry_operand('gat_backward_ex: edge_mask', edge_mask, S, handle)
    _check_entry_operand('gat_backward_ex: coef', coef, S, handle)
    return _gat_backward('uds_gat_backward_ex', handle, handle_t, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr,
                         [(edge_mask, 'edge_mask', True), (coef, 'coef', True)], out, workspace)


def gat_backward_act_workspace_floats(S, n, nnz, d):
    """Floats of workspace gat_backward_act needs: alpha, de, g and the partials of db / da (host-only, no device)."""
    return load().uds_gat_backward_act_workspace_floats(S, n, nnz, d)


def gat_backward_act(handle, handle_t, perm_t, out, gout, act, hx, s_self, s_nbr, a_self, a_nbr, edge_mask=None, coef=None, want_db=True,
                     want_da=True, outputs=None, workspace=None):
    """The reverse mode of a single-head GAT layer after its projection as one operator (uds_gat_backward_act): out (S,n,d) is
    the layer's output, gout = dL/dout, act its activation.  Returns (d_hx, ds_self, ds_nbr, db, da): the first three bitwise
    those of gat_backward[_ex] on act_grad(out, gout, act), db (d,) the bias gradient and da (2,d) the gradients of the
    attention kernels (a_self, a_nbr), each None when not wanted.  outputs: the caller's (d_hx, ds_self, ds_nbr, db, da);
    workspace: the caller's flat tensor of gat_backward_act_workspace_floats(S, n, nnz, d) floats or more."""
    if not isinstance(out, torch.Tensor) or not isinstance(gout, torch.Tensor) or out.dim() != 3 or tuple(gout.shape) != tuple(out.shape):
        raise UdsError('gat_backward_act: out and gout must be (S,n,d) tensors of one shape')
    if act not in ACT:
        raise UdsError('gat_backward_act: unknown activation %r' % (act,))
    S, n, d = out.shape
    if n != handle.n_rows or tuple(hx.shape) != (S, n, d) or tuple(s_self.shape) != (S, n) or tuple(s_nbr.shape) != (S, n):
        raise UdsError('gat_backward_act: out %r, hx %r, s_self %r, s_nbr %r do not match a %d-row pattern' %
                       (tuple(out.shape), tuple(hx.shape), tuple(s_self.shape), tuple(s_nbr.shape), handle.n_rows))
    if a_self.numel() != d or a_nbr.numel() != d:
        raise UdsError('gat_backward_act: a_self %r / a_nbr %r, expected %d values' % (tuple(a_self.shape), tuple(a_nbr.shape), d))
    _check_entry_operand('gat_backward_act: edge_mask', edge_mask, S, handle)
    _check_entry_operand('gat_backward_act: coef', coef, S, handle)
    o = outputs if outputs is not None else (None,) * 5
    d_hx, ds_self, ds_nbr = _gat_backward_outputs(gout, o[:3])
    db = _out(o[3], (d,), gout, 'db') if want_db else None
    da = _out(o[4], (2, d), gout, 'da') if want_da else None
    need = gat_backward_act_workspace_floats(S, n, handle.nnz, d)
    if workspace is None:
        workspace = torch.empty(max(need, 4), device=gout.device, dtype=torch.float32)
    elif not isinstance(workspace, torch.Tensor) or workspace.dim() != 1 or workspace.numel() < need:
        raise UdsError('gat_backward_act: workspace must be a flat tensor of at least %d floats' % need)
    if gout.numel() == 0:
        _dev(gout, 'gout')
        for t in (db, da):
            if t is not None:
                t.zero_()
        return d_hx, ds_self, ds_nbr, db, da
    _check(load().uds_gat_backward_act(handle.ptr, handle_t.ptr, _dev_i32(perm_t, 'perm_t'), _dev(out, 'out'), _dev(gout, 'gout'), ACT[act],
                                       _dev(hx, 'hx'), _dev(s_self, 's_self'), _dev(s_nbr, 's_nbr'), _dev(a_self, 'a_self'),
                                       _dev(a_nbr, 'a_nbr'), _dev(edge_mask, 'edge_mask', True), _dev(coef, 'coef', True), S, d,
                                       _dev(d_hx, 'd_hx'), _dev(ds_self, 'ds_self'), _dev(ds_nbr, 'ds_nbr'), _dev(db, 'db', True),
                                       _dev(da, 'da', True), _dev(workspace, 'workspace'), workspace.numel(), _stream()),
           'uds_gat_backward_act')
    return d_hx, ds_self, ds_nbr, db, da


def _check_heads_operands(name, handle, hx, s_self, s_nbr, edge_mask, coef):
    """(S, n, H, C) of a multi-head call: hx (S,n,H*C), scores (S,n,H), edge_mask (S,nnz), coef (S,H,nnz)."""
    if hx.dim() != 3 or s_self.dim() != 3 or tuple(s_nbr.shape) != tuple(s_self.shape):
        raise UdsError('%s: hx %r must be (S,n,H*C) and s_self %r, s_nbr %r (S,n,H)' %
                       (name, tuple(hx.shape), tuple(s_self.shape), tuple(s_nbr.shape)))
    S, n, width = hx.shape
    H = s_self.shape[-1]
    if n != handle.n_rows or tuple(s_self.shape) != (S, n, H) or H < 1 or width % H:
        raise UdsError('%s: hx %r, s_self %r, s_nbr %r do not match a %d-row pattern' %
                       (name, tuple(hx.shape), tuple(s_self.shape), tuple(s_nbr.shape), handle.n_rows))
    _check_entry_operand('%s: edge_mask' % name, edge_mask, S, handle)
    if coef is not None and tuple(coef.shape) != (S, H, handle.nnz):
        raise UdsError('%s: coef %r for %d snapshots and %d heads of a %d-entry pattern' % (name, tuple(coef.shape), S, H, handle.nnz))
    return S, n, H, width // H


def gat_aggregate_heads(handle, hx, s_self, s_nbr, bias=None, act='relu', concat=True, edge_mask=None, coef=None, out=None,
                        alpha_out=None):
    """Multi-head attention softmax + neighbour sum (uds_gat_aggregate_heads): hx (S,n,H*C) head-major, s_self / s_nbr (S,n,H),
    edge_mask (S,nnz) shared by the heads, coef (S,H,nnz) per head.  concat: out (S,n,H*C) with bias (H*C,); otherwise the mean
    over the heads, out (S,n,C) with bias (C,).  alpha_out: True or the caller's (S,H,nnz) tensor -- the coefficients the
    aggregation used (alpha * coef, 0 for a masked entry); the call then returns (out, alpha_out)."""
    lib = load()
    S, n, H, C = _check_heads_operands('gat_aggregate_heads', handle, hx, s_self, s_nbr, edge_mask, coef)
    width = H * C if concat else C
    if bias is not None and tuple(bias.shape) != (width,):
        raise UdsError('gat_aggregate_heads: bias %r, expected (%d,)' % (tuple(bias.shape), width))
    out = _out(out, (S, n, width), hx, 'out')
    alpha = None if alpha_out is None or alpha_out is False else _out(None if alpha_out is True else alpha_out, (S, H, handle.nnz), hx, 'alpha_out')
    if out.numel() == 0:
        _dev(hx, 'hx')
    else:
        _check(lib.uds_gat_aggregate_heads(handle.ptr, _dev(hx, 'hx'), _dev(s_self, 's_self'), _dev(s_nbr, 's_nbr'), _dev(bias, 'bias', True),
                                           _dev(edge_mask, 'edge_mask', True), _dev(coef, 'coef', True), S, H, C, int(bool(concat)), ACT[act],
                                           _dev(out, 'out'), _dev(alpha, 'alpha_out', True), _stream()), 'uds_gat_aggregate_heads')
    return out if alpha is None else (out, alpha)


def gat_backward_heads(handle, handle_t, perm_t, grad, hx, s_self, s_nbr, a_self, a_nbr, concat=True, edge_mask=None, coef=None, out=None,
                       workspace=None):
    """Reverse mode of gat_aggregate_heads (uds_gat_backward_heads): grad = dL/d(pre-activation), (S,n,H*C) or, for the mean,
    (S,n,C) -> d_hx (S,n,H*C), ds_self (S,n,H), ds_nbr (S,n,H).  a_self / a_nbr (H*C,) head-major.  out: the caller's
    (d_hx, ds_self, ds_nbr); workspace: the caller's (2, S, H, max(nnz, 1)) alpha / de scratch."""
    lib = load()
    S, n, H, C = _check_heads_operands('gat_backward_heads', handle, hx, s_self, s_nbr, edge_mask, coef)
    if tuple(grad.shape) != (S, n, H * C if concat else C):
        raise UdsError('gat_backward_heads: grad %r for hx %r, %d heads, concat=%r' % (tuple(grad.shape), tuple(hx.shape), H, bool(concat)))
    if a_self.numel() != H * C or a_nbr.numel() != H * C:
        raise UdsError('gat_backward_heads: a_self %r / a_nbr %r, expected %d values' % (tuple(a_self.shape), tuple(a_nbr.shape), H * C))
    o = out if out is not None else (None, None, None)
    d_hx, ds_self, ds_nbr = _out(o[0], hx.shape, grad, 'd_hx'), _out(o[1], (S, n, H), grad, 'ds_self'), _out(o[2], (S, n, H), grad, 'ds_nbr')
    if grad.numel() == 0:
        return _nothing_to_launch(grad, 'grad', (d_hx, ds_self, ds_nbr))
    ws = _out(workspace, (2, S, H, max(handle.nnz, 1)), grad, 'workspace')      # alpha and de per head and pattern entry
    _check(lib.uds_gat_backward_heads(handle.ptr, handle_t.ptr, _dev_i32(perm_t, 'perm_t'), _dev(grad, 'grad'), _dev(hx, 'hx'),
                                      _dev(s_self, 's_self'), _dev(s_nbr, 's_nbr'), _dev(a_self, 'a_self'), _dev(a_nbr, 'a_nbr'),
                                      _dev(edge_mask, 'edge_mask', True), _dev(coef, 'coef', True), S, H, C, int(bool(concat)),
                                      _dev(ws[0], 'alpha_ws'), _dev(ws[1], 'de_ws'), _dev(d_hx, 'd_hx'), _dev(ds_self, 'ds_self'),
                                      _dev(ds_nbr, 'ds_nbr'), _stream()), 'uds_gat_backward_heads')
    return d_hx, ds_self, ds_nbr


def wgrad_supported(F, H, with_bias=True):
    return load().uds_wgrad_workspace_floats(128, F, H, int(with_bias)) > 0


def wgrad(a, g, shift=0, with_bias=True):
    """d_kernel (F,H) [, d_bias (H)] of out = a @ kernel (+ bias): sums over all rows of a (B,T,R,F)^T g (B,T,R,H), for a
    causal Conv1D tap with the input `shift` time steps back.  Matrix cores, split-bf16, deterministic."""
    lib = load()
    B, T, R, F = a.shape
    H = g.shape[-1]
    if tuple(g.shape[:-1]) != (B, T, R):
        raise UdsError('wgrad: a %r and g %r disagree' % (tuple(a.shape), tuple(g.shape)))
    n_ws = lib.uds_wgrad_workspace_floats(max(B * T * R, 1), F, H, int(with_bias))
    if n_ws <= 0:
        raise UdsError('wgrad: F=%d / H=%d not supported' % (F, H))
    dk = torch.empty((F, H), device=a.device, dtype=torch.float32)
    db = torch.empty(H, device=a.device, dtype=torch.float32) if with_bias else None
    ws = torch.empty(n_ws, device=a.device, dtype=torch.float32)
    _check(lib.uds_wgrad(_dev(a, 'a'), _dev(g, 'g'), B, T, R, F, H, shift, int(with_bias), _dev(ws, 'workspace'), _dev(dk, 'd_kernel'),
                         _dev(db, 'd_bias', True), _stream()), 'uds_wgrad')
    return dk, db


def wgrad_wide_supported(F, H, with_bias=True):
    return load().uds_wgrad_wide_workspace_floats(128, F, H, int(with_bias)) > 0


def wgrad_wide(a, g, shift=0, with_bias=True):
    """wgrad for outputs up to 256 (+ the bias row) x 256 (uds_wgrad_wide): the output cut into blocks, one per wave of a
    workgroup, a and g read from memory once.  Same arithmetic, deterministic."""
    lib = load()
    B, T, R, F = a.shape
    H = g.shape[-1]
    if tuple(g.shape[:-1]) != (B, T, R):
        raise UdsError('wgrad_wide: a %r and g %r disagree' % (tuple(a.shape), tuple(g.shape)))
    n_ws = lib.uds_wgrad_wide_workspace_floats(max(B * T * R, 1), F, H, int(with_bias))
    if n_ws <= 0:
        raise UdsError('wgrad_wide: F=%d / H=%d not supported' % (F, H))
    dk = torch.empty((F, H), device=a.device, dtype=torch.float32)
    db = torch.empty(H, device=a.device, dtype=torch.float32) if with_bias else None
    ws = torch.empty(n_ws, device=a.device, dtype=torch.float32)
    _check(lib.uds_wgrad_wide(_dev(a, 'a'), _dev(g, 'g'), B, T, R, F, H, shift, int(with_bias), _dev(ws, 'workspace'), _dev(dk, 'd_kernel'),
                              _dev(db, 'd_bias', True), _stream()), 'uds_wgrad_wide')
    return dk, db


def node_edge_wgrad_plan(R, M, S, h):
    """uds_node_edge_wgrad_plan (host only): dict(ksteps = k-steps of 32 per snapshot, the instantiation, 0 when the shape is
    refused; pieces = pieces of the reduction over S; spp = snapshots per piece; padded = h is no multiple of 32)."""
    info = (ctypes.c_int32 * 4)()
    _check(load().uds_node_edge_wgrad_plan(int(R), int(M), int(S), int(h), info), 'uds_node_edge_wgrad_plan')
    return dict(ksteps=int(info[0]), pieces=int(info[1]), spp=int(info[2]), padded=bool(info[3]))


def node_edge_wgrad_supported(h):
    return load().uds_node_edge_wgrad_workspace_bytes(1, 1, 1, int(h)) > 0


def node_edge_wgrad(g, x, inci=None):
    """(d_bias, d_weight) of a dense-parameter NodeEdge (uds_node_edge_wgrad): d_bias[r, m] = sum_{s, k} g[s, r, k] x[s, m, k] for
    g (S, R, h), x (S, M, h) in their own layouts, d_weight = d_bias * inci (None without inci).  Matrix cores, split-bf16,
    deterministic."""
    lib = load()
    if g.dim() != 3 or x.dim() != 3 or g.shape[0] != x.shape[0] or g.shape[2] != x.shape[2]:
        raise UdsError('node_edge_wgrad: g %r and x %r disagree' % (tuple(g.shape), tuple(x.shape)))
    S, R, h = g.shape
    M = x.shape[1]
    if inci is not None and tuple(inci.shape) != (R, M):
        raise UdsError('node_edge_wgrad: inci %r against (%d, %d)' % (tuple(inci.shape), R, M))
    if lib.uds_node_edge_wgrad_workspace_bytes(R, M, 1, h) <= 0:
        raise UdsError('node_edge_wgrad: R=%d, M=%d, h=%d not supported' % (R, M, h))
    db = torch.empty((R, M), device=g.device, dtype=torch.float32)
    dw = torch.empty((R, M), device=g.device, dtype=torch.float32) if inci is not None else None
    ws = torch.empty(max(lib.uds_node_edge_wgrad_workspace_bytes(R, M, S, h) // 4, 1), device=g.device, dtype=torch.float32)
    _check(lib.uds_node_edge_wgrad(_dev(g, 'g') if S else None, _dev(x, 'x') if S else None, S, R, M, h, _dev(inci, 'inci', True),
                                   _dev(ws, 'workspace'), _dev(db, 'd_bias'), _dev(dw, 'd_weight', True), _stream()), 'uds_node_edge_wgrad')
    return db, dw


def csr_sddmm(handle, a, b, out=None):
    """out[k] = sum_s <a[s,row(k),:], b[s,col(k),:]> per pattern entry; a:(S,n_rows,F), b:(S,n_cols,F) -> (nnz,).
    out: the caller's result tensor (zeroed here where the kernel does not run)."""
    lib = load()
    if a.dim() != 3 or b.dim() != 3 or a.shape[1] != handle.n_rows or b.shape[1] != handle.n_cols or a.shape[0] != b.shape[0] \
            or a.shape[2] != b.shape[2]:
        raise UdsError('sddmm: a must be (S,%d,F) and b (S,%d,F), got %r, %r' % (handle.n_rows, handle.n_cols, tuple(a.shape),
                                                                               tuple(b.shape)))
    if out is None:
        out = torch.zeros(handle.nnz, device=a.device, dtype=torch.float32)
    else:
        out = _out(out, (handle.nnz,), a, 'out')
    if handle.nnz == 0 or a.numel() == 0:
        _dev(a, 'a')
        return out.zero_() if out.numel() else out
    _check(lib.uds_csr_sddmm(handle.ptr, _dev(a, 'a'), _dev(b, 'b'), a.shape[0], a.shape[2], _dev(out, 'out'), _stream()),
           'uds_csr_sddmm')
    return out


def _spatial_params(p):
    sp = SpatialParams()
    for name, _ in SpatialParams._fields_:
        if name == 'packed':
            t = p.get('packed')
            sp.packed = None if t is None else t.data_ptr()
        else:
            setattr(sp, name, _dev(p[name], name, allow_none=name.endswith('_b')))
    return sp


def spatial_pack_weights(p, fx, fe, h, d):
    """Pre-split the four kernels of a spatial layer into the fused kernel's bf16 hi/lo MFMA fragments (done once per
    parameter update instead of in every forward call).  Returns the device buffer to pass as p['packed']."""
    lib = load()
    out = torch.empty(lib.uds_spatial_packed_bytes() // 4, device=p['xe_k'].device, dtype=torch.float32)
    q = dict(p)
    q['packed'] = None
    _check(lib.uds_spatial_pack_weights(ctypes.byref(_spatial_params(q)), fx, fe, h, d, out.data_ptr(), _stream()),
           'uds_spatial_pack_weights')
    return out


def spatial_layer_forward(net, p, x, e, h, d, act='relu', flags=0, xb=None, eb=None, rem_x=None, rem_e=None):
    """One spatial-block loop body (`emulator.py:225-230`).  p: dict of the 14 tensors of
    uds_spatial_params_t.  x:(S,N,fx), e:(S,E,fe) -> (S,N,d), (S,E,d).  flags: FLAG_* of the C ABI.
    xb (S,N,32) / eb (S,E,32): extra columns appended to a 64-wide x / e without materialising the concatenation
    (uds_spatial_layer_forward_split; fused kernel only).
    rem_x (S,N,h) / rem_e (S,E,h): the dense remainder of a trained NodeEdge, added to the aggregates inside the d = 128 fused
    kernel (uds_spatial_layer_forward_rem; fused kernel only)."""
    lib = load()
    S, N, fx = x.shape
    _, E, fe = e.shape
    if e.shape[0] != S or N != net.graph.n_node or E != net.graph.n_edge:
        raise UdsError('x %r / e %r do not match the network (N=%d, E=%d)' % (tuple(x.shape), tuple(e.shape),
                                                                            net.graph.n_node, net.graph.n_edge))
    if S == 0:
        return _nothing_to_launch(x, 'x', (torch.empty((0, N, d), device=x.device, dtype=torch.float32),
                                           torch.empty((0, E, d), device=x.device, dtype=torch.float32)))
    sp = _spatial_params(p)
    ws = torch.empty(lib.uds_spatial_workspace_floats(net.ptr, S, h, d), device=x.device, dtype=torch.float32)
    out_x = torch.empty((S, N, d), device=x.device, dtype=torch.float32)
    out_e = torch.empty((S, E, d), device=x.device, dtype=torch.float32)
    if rem_x is not None or rem_e is not None:
        if xb is not None or eb is not None or rem_x is None or rem_e is None:
            raise UdsError('rem_x and rem_e come together, without xb / eb')
        if tuple(rem_x.shape) != (S, N, h) or tuple(rem_e.shape) != (S, E, h):
            raise UdsError('rem_x %r / rem_e %r must be %r / %r' % (tuple(rem_x.shape), tuple(rem_e.shape), (S, N, h), (S, E, h)))
        _check(lib.uds_spatial_layer_forward_rem(net.ptr, ctypes.byref(sp), _dev(x, 'x'), fx, _dev(e, 'e'), fe, _dev(rem_x, 'rem_x'),
                                                 _dev(rem_e, 'rem_e'), S, h, d, ACT[act], int(flags), _dev(ws, 'workspace'),
                                                 _dev(out_x, 'out_x'), _dev(out_e, 'out_e'), _stream()), 'uds_spatial_layer_forward_rem')
        return out_x, out_e
    if xb is not None or eb is not None:
        for t, ref, name in ((xb, x, 'xb'), (eb, e, 'eb')):
            if t is not None and tuple(t.shape[:2]) != tuple(ref.shape[:2]):
                raise UdsError('%s %r does not match %r' % (name, tuple(t.shape), tuple(ref.shape)))
        _check(lib.uds_spatial_layer_forward_split(net.ptr, ctypes.byref(sp), _dev(x, 'x'), fx, _dev(xb, 'xb', True),
                                                   0 if xb is None else xb.shape[-1], _dev(e, 'e'), fe, _dev(eb, 'eb', True),
                                                   0 if eb is None else eb.shape[-1], S, h, d, ACT[act], int(flags),
                                                   _dev(ws, 'workspace'), _dev(out_x, 'out_x'), _dev(out_e, 'out_e'), _stream()),
               'uds_spatial_layer_forward_split')
        return out_x, out_e
    _check(lib.uds_spatial_layer_forward(net.ptr, ctypes.byref(sp), _dev(x, 'x'), fx, _dev(e, 'e'), fe, S, h, d, ACT[act],
                                         int(flags), _dev(ws, 'workspace'), _dev(out_x, 'out_x'), _dev(out_e, 'out_e'), _stream()),
           'uds_spatial_layer_forward')
    return out_x, out_e
