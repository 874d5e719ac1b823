"""ctypes binding of libptb_hip.so (the C ABI declared in include/ptb_hip.h).

There is deliberately NO fallback behind this binding: if the shared library is missing, or a tensor that reaches an entry point
is not on the MI355X, the call fails loudly.  (Host tensors never reach it: the public functions route them -- by their device, and
by nothing else -- to the separate torch-op modules ``inference/_host.py`` / ``losses/_host.py``, like the device-agnostic
reference.)  PyTorch is used only for device memory, the current HIP stream and autograd glue.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTB_HIP_LIB: load another build of the library (A/B experiments, an integrator's own build location)
LIB_PATH = os.environ.get("PTB_HIP_LIB") or os.path.join(_HERE, "lib", "libptb_hip.so")

# view codes (bit0 transpose, bit1 flip source rows, bit2 flip source cols) -- include/ptb_hip.h
IDENT, TRANSPOSE, FLIPUD, ROT90_CW, FLIPLR, ROT90_CCW, ROT180, ANTITRANSPOSE = range(8)

RED_SUM, RED_MEAN, RED_GMEAN, RED_HMEAN, RED_HARMONIC1P, RED_LOGODD, RED_LOG1P = range(7)
F32, F16, BF16 = range(3)   # PTB_F32 / PTB_F16 / PTB_BF16: element type of the model outputs a `_t` entry point reads
DTYPE_CODES = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
# PTB_CROP_*: output kinds of ptb_volume_merge_crop (0..5) and ptb_merge_crop (0..3), by (argmax, requested dtype) -> (kind, output dtype)
CROP_F32, CROP_U8, CROP_ARGMAX_U8, CROP_ARGMAX_I64, CROP_F16, CROP_BF16 = range(6)
CROP_KINDS = {(False, torch.float32): (CROP_F32, torch.float32), (False, torch.uint8): (CROP_U8, torch.uint8),
              (False, torch.float16): (CROP_F16, torch.float16), (False, torch.bfloat16): (CROP_BF16, torch.bfloat16),
              (True, torch.uint8): (CROP_ARGMAX_U8, torch.uint8), (True, torch.int64): (CROP_ARGMAX_I64, torch.int64),
              (True, torch.float32): (CROP_ARGMAX_I64, torch.int64)}
U8, I16, U16 = 3, 4, 5      # PTB_U8 / PTB_I16 / PTB_U16: further volume element types of ptb_volume_split
VOLUME_DTYPE_CODES = {torch.uint8: U8, torch.int16: I16, torch.uint16: U16, torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32}
IMAGE_DTYPE_CODES = {torch.uint8: U8, torch.uint16: U16, torch.int16: I16}   # image element types of ptb_split_tiles
# PTB_BORDER_*: OpenCV's border codes (cv2.BORDER_CONSTANT .. cv2.BORDER_REFLECT_101)
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = range(5)
ROUND_SRC = 0x100           # PTB_ROUND_SRC, or-ed into a dtype code: round the reduced value to the (half) source type before blending
SRC_CHANNELS_LAST = 0x200   # PTB_SRC_CHANNELS_LAST, or-ed into a dtype code: the batch is [V*B, th, tw, C] memory (a model in torch.channels_last)
DTYPE_MASK = 0xFF           # the PTB_F32 / PTB_F16 / PTB_BF16 part of a dtype code that carries flags
LAYOUT_DENSE, LAYOUT_CHANNELS_LAST, LAYOUT_OTHER = range(3)
ACT_NONE, ACT_SIGMOID, ACT_SOFTMAX = range(3)   # PTB_ACT_*: the activation fused into the 2-D / 3-D de-augmentation and tile merges
ACT_CODES = {None: ACT_NONE, "sigmoid": ACT_SIGMOID, "softmax": ACT_SOFTMAX}
ACT_MAX_SOFTMAX_CHANNELS = 16

EFRESH = -5
PTB_EHELD = -6
PTB_EUNSUPPORTED = -2
_ERR = {-1: "invalid argument", -2: "unsupported configuration", -3: "HIP launch failed", -4: "tile rectangle outside the accumulator",
        -5: "a cell straddles written and never-written accumulator blocks (zero-fill the accumulators, then call without the first-touch bitmap)",
        -6: "the batch overlaps memory of an earlier batch that a later launch still reads",
        -7: "the relaxation did not converge within max_sweeps sweeps"}
PTB_ENOTCONVERGED = -7

_c_int = ctypes.c_int
_c_f = ctypes.c_float
_c_d = ctypes.c_double
_c_i64 = ctypes.c_int64
_vp = ctypes.c_void_p
_i64p = ctypes.POINTER(ctypes.c_int64)
_ip = ctypes.POINTER(ctypes.c_int)
_fp = ctypes.POINTER(ctypes.c_float)
_vpp = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); must list every symbol of include/ptb_hip.h (checked by tests/test_abi.py)
SIGNATURES = {
    "ptb_version": (_c_int, []),
    "ptb_last_hip_error": (ctypes.c_char_p, []),
    "ptb_set_tunable": (_c_int, [_c_int, _c_int]),
    "ptb_read_probe": (_c_int, [_vp, _c_i64, _vp, _vp]),
    "ptb_read_probe_multi": (_c_i64, [_vpp, _i64p, _c_int, _vp, _c_int, _vp]),
    "ptb_sums_finalize": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _vp]),
    "ptb_tile_accumulate": (_c_int, [_vp, _vp, _vp, _vp, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    "ptb_deaug_reduce_t": (_c_int, [_vp, _c_int, _vp, _c_int, _ip, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_deaug_accumulate_t": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _ip, _c_int, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    "ptb_accumulate_planned": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _ip, _c_int, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                        _vp, _c_int, _vp, _vp, _vp]),
    "ptb_accumulate_planned2": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _ip, _c_int, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                                         _vp, _c_int, _vp, _vp, _c_int, _vp]),
    "ptb_merge_div_masked": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    "ptb_norm_accumulate": (_c_int, [_vp, _vp, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    "ptb_debug_plan": (_c_int, [_i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _ip, _c_int]),
    "ptb_merge_div": (_c_int, [_vp, _vp, _vp, _c_int, _c_i64, _vp]),
    "ptb_merge_band": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _vp, _c_int, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_band_plan_create": (_c_i64, [_i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _i64p, _c_int, _vpp]),
    "ptb_band_plan_upload": (_c_int, [_vp, _vp, _vp]),
    "ptb_band_plan_info": (_c_int, [_vp, _ip, _ip, _i64p, _i64p, _i64p]),
    "ptb_band_plan_pairs": (_c_int, [_vp, _c_int, _ip, _ip]),
    "ptb_band_plan_reset": (_c_int, [_vp]),
    "ptb_band_plan_state": (_c_int, [_vp, _ip, _ip]),
    "ptb_band_plan_submit": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _c_int, _c_int, _ip, _c_int, _vp, _vp, _vp, _vp]),
    "ptb_band_plan_submit_next": (_c_int, [_vp, _vp, _c_int, _vp]),
    "ptb_band_plan_destroy": (None, [_vp]),
    "ptb_rccl_available": (_c_int, []),
    "ptb_rccl_unique_id": (_c_int, [_vp]),
    "ptb_rccl_comm_init": (_c_int, [_vp, _c_int, _c_int, _vpp]),
    "ptb_rccl_comm_destroy": (_c_int, [_vp]),
    "ptb_halo_exchange": (_c_int, [_vp, _c_int, _vpp, _i64p, _ip, _c_int, _vpp, _i64p, _ip, _vp]),
    "ptb_band_plan_create2": (_c_i64, [_i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _i64p, _c_int, _i64p, _c_int, _vpp]),
    "ptb_band_plan_create3": (_c_i64, [_i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _i64p, _c_int, _i64p, _c_int, _c_int,
                                       _vpp]),
    "ptb_band_plan_rows_launched": (_c_int, [_vp, _c_int, _c_int]),
    "ptb_halo_pack": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _c_int, _vp, _vp]),
    "ptb_band_plan_finish_rank": (_c_int, [_vp, _vp, _vp, _c_int, _i64p, _vpp, _c_int, _i64p, _vp]),
    "ptb_band_plan_submit_rank": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _c_int, _c_int, _ip, _c_int, _vp, _vp, _vp, _c_int, _i64p, _vpp, _ip, _vp,
                                           _ip, _vp]),
    "ptb_rect_add": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_i64, _c_i64, _vp]),
    "ptb_merge_div_ex": (_c_int, [_vp, _vp, _vp, _c_int, _c_i64, _c_i64, _c_i64, _vp, _c_i64, _c_i64, _vp]),
    "ptb_deaug_reduce": (_c_int, [_vp, _vp, _c_int, _ip, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_deaug_reduce_bwd": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _ip, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_view_transform": (_c_int, [_vp, _vp, _c_int, _ip, _c_int, _c_f, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_view_permute": (_c_int, [_vp, _vp, _c_int, _ip, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _vp]),
    "ptb_resize_bilinear": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_ms_deaug_reduce": (_c_int, [_vp, _ip, _ip, _c_int, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_ms_deaug_reduce_strip": (_c_int, [_vp, _ip, _ip, _ip, _ip, _c_int, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_resize_bilinear_bwd": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_ms_deaug_reduce_bwd": (_c_int, [_vp, _ip, _ip, _c_int, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_resize_bicubic": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_bitempered_rows": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_int, _c_f, _c_f, _c_f, _c_int, _c_int, _vp]),
    "ptb_stack_reduce": (_c_int, [_vp, _c_int, _c_i64, _c_int, _c_d, _vp, _vp]),
    "ptb_stack_reduce_bwd": (_c_int, [_vp, _vp, _vp, _c_int, _c_i64, _c_int, _c_d, _vp, _vp]),
    "ptb_resize_nearest": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_resize_nearest_exact": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_resize_area": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_ms_flip_deaug_reduce_strip": (_c_int, [_vp, _ip, _ip, _ip, _ip, _c_int, _c_int, _ip, _c_int, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_ms_flip_deaug_reduce": (_c_int, [_vp, _ip, _ip, _c_int, _c_int, _ip, _c_int, _vp, _c_i64, _c_int, _c_int, _c_int, _c_int, _vp]),
    "ptb_seg_loss_fwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_f, _c_f, _c_f, _c_i64, _c_f, _vp]),
    "ptb_focal_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_f, _c_i64, _c_f, _vp]),
    "ptb_focal_softmax_fwd": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_f, _c_i64, _c_f, _vp]),
    "ptb_focal_softmax_bwd": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_f, _c_i64, _c_f, _vp]),
    "ptb_seg_stats_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_i64, _c_f, _vp]),
    "ptb_region_workspace_bytes": (_c_i64, [_c_int]),
    "ptb_region_loss_fwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_f, _c_f, _c_f, _c_i64, _c_f, _c_f, _c_f, _c_f, _c_f,
                                     _c_f, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "ptb_region_epilogue": (_c_int, [_vp, _c_int, _c_int, _c_f, _c_f, _c_f, _c_f, _c_f, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "ptb_seg_fused_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_f, _c_f, _c_f, _c_i64, _c_f, _vp]),
    "ptb_softmax_focal_fwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_i64, _vp]),
    "ptb_softmax_focal_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_i64, _vp]),
    "ptb_lovasz_temp_bytes": (_c_i64, [_c_i64, _c_int]),
    "ptb_lovasz_fwd": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _c_f] + [_vp] * 9 + [_c_i64, _vp]),
    "ptb_lovasz_fwd_keys": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _c_f] + [_vp] * 6 + [_c_i64, _vp]),
    "ptb_lovasz_fwd_binned": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _c_f] + [_vp] * 9 + [_c_i64, _vp]),
    "ptb_lovasz_bwd_binned": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _c_f, _c_int, _vp]),
    "ptb_lovasz_bwd_binned2": (_c_int, [_vp] * 8 + [_c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _c_f, _c_int, _vp]),
    "ptb_lovasz_reduce": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp]),
    "ptb_lovasz_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_int, _c_i64, _c_f, _vp]),
    "ptb_deaug_accumulate": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _ip, _c_int, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    "ptb_split_tiles_u8": (_c_int, [_vp, _c_int, _c_int, _c_int, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _ip, _fp, _fp, _c_int, _vp, _vp]),
    "ptb_split_tiles": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _ip, _fp, _fp, _c_int, _c_f,
                                 _c_int, _vp, _vp]),
    "ptb_pointwise_loss_fwd": (_c_int, [_c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_f, _c_f, _vp]),
    "ptb_pointwise_loss_apply": (_c_int, [_c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_i64, _c_int, _c_f, _c_f, _c_f, _c_f, _vp]),
    "ptb_bitempered_binary_fwd": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_f, _c_f, _c_f, _c_int, _c_int, _c_f, _vp]),
    "ptb_bitempered_binary_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_f, _c_f, _c_f, _c_int, _c_int, _c_f, _vp]),
    "ptb_soft_ce_fwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_f, _c_int, _c_i64, _vp]),
    "ptb_soft_ce_bwd": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_f, _c_int, _c_i64, _vp]),
    "ptb_volume_accumulate": (_c_int, [_vp, _vp, _vp, _vp, _i64p, _i64p, _i64p] + [_c_int] * 8 + [_vp]),
    "ptb_ensemble_reduce": (_c_int, [_vpp, _c_int, _c_int, _c_int, _c_f, _c_int, _c_int, _c_i64, _vp, _vp]),
    "ptb_merge_crop": (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    "ptb_volume_split": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _i64p, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _fp, _fp, _c_f,
                                  _c_int, _vp, _vp]),
    "ptb_volume_merge_crop": (_c_int, [_vp, _vp] + [_c_int] * 12 + [_vp, _vp]),
    "ptb_volume_resize_trilinear": (_c_int, [_vp] + [_c_int] * 10 + [_vp, _vp]),
    "ptb_volume_mirror": (_c_int, [_vp, _c_int, _vp, _c_int, _ip] + [_c_int] * 6 + [_vp]),
    "ptb_volume_mirror_reduce": (_c_int, [_vp, _c_int, _vp, _c_int, _ip] + [_c_int] * 6 + [_vp]),
    "ptb_volume_mirror_accumulate": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _ip, _c_int, _i64p, _i64p, _i64p] + [_c_int] * 8 + [_vp]),
    "ptb_volume_split_mirror": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _i64p, _i64p, _i64p, _c_int, _c_int, _c_int, _c_int, _fp, _fp,
                                         _c_f, _c_int, _ip, _c_int, _vp, _vp]),
    "ptb_volume_plan_create": (_c_i64, [_i64p, _i64p, _i64p] + [_c_int] * 8 + [_i64p, _c_int, _c_int, _vpp]),
    "ptb_volume_plan_items": (_c_i64, [_vp, _i64p, _c_i64]),
    "ptb_volume_plan_info": (_c_int, [_vp, _ip, _ip, _i64p, _i64p, _i64p, _ip, _ip]),
    "ptb_volume_plan_upload": (_c_int, [_vp, _vp, _vp]),
    "ptb_volume_plan_reset": (_c_int, [_vp]),
    "ptb_volume_plan_state": (_c_int, [_vp, _ip, _ip]),
    "ptb_volume_plan_submit": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _c_int, _c_int, _ip, _c_int, _vp, _vp, _vp]),
    "ptb_volume_plan_destroy": (None, [_vp]),
    "ptb_volume_mirror_reduce_act": (_c_int, [_vp, _c_int, _vp, _c_int, _ip] + [_c_int] * 7 + [_c_f, _vp]),
    "ptb_volume_mirror_accumulate_act": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _ip, _c_int, _i64p, _i64p, _i64p] + [_c_int] * 9 + [_c_f, _vp]),
    "ptb_deaug_reduce_act": (_c_int, [_vp, _c_int, _vp, _c_int, _ip] + [_c_int] * 6 + [_c_f, _vp]),
    "ptb_deaug_accumulate_act": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _ip, _c_int, _i64p, _i64p] + [_c_int] * 6 + [_vp, _c_int, _c_int, _c_f, _vp]),
    "ptb_band_plan_submit_act": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _c_int, _c_int, _ip, _c_int, _vp, _vp, _vp, _c_int, _c_f, _vp]),
    "ptb_volume_plan_submit_act": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _c_int, _c_int, _ip, _c_int, _vp, _vp, _c_int, _c_f, _vp]),
    "ptb_rle_workspace_bytes": (_c_i64, [_c_int, _c_int, _c_int, _c_int]),
    "ptb_rle_count": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _i64p, _c_int, _vp, _c_i64, _vp]),
    "ptb_rle_write": (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _i64p, _c_int, _vp, _c_i64, _vp, _c_i64, _vp]),
    "ptb_rle_decode_workspace_bytes": (_c_i64, [_c_int, _c_int]),
    "ptb_rle_decode": (_c_int, [_vp, _c_i64, _c_int, _c_int, _vp, _vp, _c_i64, _vp]),
    "ptb_confusion_plan": (_c_int, [_c_int, _ip, _ip]),
    "ptb_confusion_labels": (_c_int, [_vp, _c_int, _vp, _c_int, _c_i64, _c_i64, _c_int, _c_int, _c_i64, _vp, _vp, _vp]),
    "ptb_confusion_logits": (_c_int, [_vp, _c_int, _c_i64, _c_int, _c_i64, _c_f, _vp, _c_int, _c_int, _c_int, _c_i64, _vp, _vp, _vp]),
    "ptb_cc_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _ip, _i64p, _i64p, _ip, _i64p, _i64p]),
    "ptb_cc_label": (_c_int, [_vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_i64, _vp, _vp, _vp, _c_i64, _vp]),
    "ptb_cc_remove_small": (_c_int, [_vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp]),
    "ptb_cc_stats": (_c_int, [_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "ptb_edt_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _i64p]),
    "ptb_edt": (_c_int, [_vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, ctypes.POINTER(_c_d), _c_int, _vp, _c_int, _vp, _c_i64, _vp]),
    "ptb_nearest_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _i64p]),
    "ptb_nearest": (_c_int, [_vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, ctypes.POINTER(_c_d), _c_int, _vp, _vp, _vp, _vp, _c_d,
                             _vp, _c_i64, _vp]),
    "ptb_watershed_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _i64p]),
    "ptb_watershed": (_c_int, [_vp, _c_int, _vp, _c_int, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _ip,
                               _vp, _c_i64, _vp]),
    "ptb_reconstruct_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _i64p]),
    "ptb_reconstruct": (_c_int, [_vp, _vp, _c_int, _vp, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_f, _c_f, _c_int, _vp, _ip, _vp, _c_i64,
                                 _vp]),
    "ptb_thin_rule": (ctypes.c_uint32, [_c_int, _c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]),
    "ptb_thin_steps": (_c_int, []),
    "ptb_skeleton_plan": (_c_int, [_c_i64, _c_i64, _c_i64, _i64p]),
    "ptb_skeleton": (_c_int, [_vp, _c_int, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, _c_int, _c_i64, _vp, _ip, _vp, _c_i64, _vp]),
    "ptb_centerline_dice_plan": (_c_int, [_c_i64, _c_i64, _c_i64, _c_int, _i64p]),
    "ptb_centerline_dice": (_c_int, [_vp, _c_int, _vp, _c_int, _c_i64, _c_i64, _c_i64, _i64p, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _ip, _vp, _c_i64, _vp]),
    "ptb_surface_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, _ip, _i64p, _i64p, _ip]),
    "ptb_surface_metrics": (_c_int, [_vp, _c_int, _vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, _i64p, _c_int, _c_int, _c_int, ctypes.POINTER(_c_d), _c_d,
                                     ctypes.POINTER(_c_d), _c_int] + [_vp] * 8 + [_vp, _c_i64, _vp]),
    "ptb_inst_plan": (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_i64, _i64p, _i64p, _i64p, _i64p]),
    "ptb_inst_overlaps": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp]),
    "ptb_inst_match": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_d), _c_int, _vp, _c_int, _vp, _c_int, _c_i64, _vp, _c_i64,
                                _vp, _c_i64, _vp]),
    "ptb_dloss_plan": (_c_int, [_c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_i64, _i64p, _i64p, _i64p, _i64p]),
    "ptb_dloss_masks": (_c_int, [_vp, _vp, _vp, _ip, _vp, _c_int, _c_int, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_i64, _c_f, _vp, _vp]),
    "ptb_dloss_fwd": (_c_int, [_c_int, _vp, _vp, _vp, _ip, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_i64, _c_f, _c_f,
                               _c_int, _vp, _c_i64, _vp, _vp, _vp, _vp]),
    "ptb_dloss_bwd": (_c_int, [_c_int, _vp, _vp, _vp, _ip, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_i64, _c_int, _c_int, _c_i64, _c_f, _c_f,
                               _c_int, _vp, _vp, _vp]),
    "ptb_hardce_workspace_bytes": (_c_i64, [_c_int, _c_int, _c_int, _c_i64, _c_int]),
    "ptb_hardce_fwd": (_c_int, [_vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _c_i64, _c_f, _c_int, _c_int, _c_d, _c_f, _c_i64] + [_vp] * 2 + [_c_i64]
                       + [_vp] * 7),
    "ptb_hardce_bwd": (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_int, _c_i64, _c_int, _vp, _vp, _vp, _vp]),
}

_lib = None
_lock = threading.Lock()
fresh_fallbacks = 0  # times a first-touch bitmap could not be honoured (diagnostics)
calls = 0  # number of native entry-point invocations (tests assert the HIP path really ran)


def load():
    """Load libptb_hip.so (built by ``__graft_entry__.build()``); raises ImportError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} is missing: build the HIP extension first "
                    "(python -c 'import __graft_entry__ as g; g.build()'). There is no non-HIP fallback."
                )
            lib = ctypes.CDLL(LIB_PATH)  # torch (imported above) has already loaded libamdhip64.so.7
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc, what):
    if rc == 0:
        return
    msg = _ERR.get(rc, f"error {rc}")
    if rc == -3:
        msg += ": " + load().ptb_last_hip_error().decode()
    if rc == -2:
        raise NotImplementedError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg}")


def batch_layout(t):
    """How a 4-D model output lies in memory: ``LAYOUT_DENSE`` (``[N, C, H, W]`` contiguous: what every kernel reads), ``LAYOUT_CHANNELS_LAST``
    (not that, but contiguous in ``torch.channels_last`` -- element ``(n, c, i, j)`` at ``((n * H + i) * W + j) * C + c``; read where it lies with
    ``SRC_CHANNELS_LAST``) or ``LAYOUT_OTHER`` (any other strides, tensors that are not 4-D: copied first).  With ``C == 1`` or a 1 x 1 plane
    the two formats coincide and the tensor counts as dense."""
    if t.is_contiguous():
        return LAYOUT_DENSE
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return LAYOUT_CHANNELS_LAST
    return LAYOUT_OTHER


def dense_or_channels_last(t):
    """The batch can be handed to the kernels as it is (see ``batch_layout``)."""
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


def volume_layout(t):
    """``batch_layout`` for a 5-D model output: ``LAYOUT_DENSE`` (``[N, C, D, H, W]`` contiguous), ``LAYOUT_CHANNELS_LAST`` (not that, but
    contiguous in ``torch.channels_last_3d`` -- element ``(n, c, z, y, x)`` at ``(((n * D + z) * H + y) * W + x) * C + c``; read where it lies
    with ``SRC_CHANNELS_LAST``) or ``LAYOUT_OTHER`` (any other strides, tensors that are not 5-D: copied first).  With ``C == 1`` or a
    1 x 1 x 1 volume the two formats coincide and the tensor counts as dense."""
    if t.dim() != 5:
        return LAYOUT_OTHER
    if t.is_contiguous():
        return LAYOUT_DENSE
    if t.is_contiguous(memory_format=torch.channels_last_3d):
        return LAYOUT_CHANNELS_LAST
    return LAYOUT_OTHER


def layout_flag(t):
    """``SRC_CHANNELS_LAST`` for a channels-last batch, 0 for a dense one."""
    return 0 if t.is_contiguous() else SRC_CHANNELS_LAST


def require_device(t, what):
    """The native path runs on the GPU only; a CPU tensor that gets this far (entry points without a host form: split_device, the
    sharded mergers' deferred plan, the strip kernels) is refused instead of silently computed elsewhere."""
    if not t.is_cuda:
        raise RuntimeError(
            f"{what}: tensor is on '{t.device}', but pytorch_toolbelt_amd runs its hot path as HIP kernels on the "
            "MI355X only (no CPU fallback). Move the tensor to a 'cuda' device."
        )


# raw_stream(index): the current HIP stream of device ``index`` as an integer handle (torch's raw query, called as it is: 0.3 us
# instead of 4 us for a Stream object); the one lookup of it in the package
raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda index: torch.cuda.current_stream(index).cuda_stream)


def stream_ptr(device):
    """The current HIP stream of ``device`` as a ``void*``."""
    idx = device.index
    return _vp(raw_stream(idx if idx is not None else torch.cuda.current_device()))


class on_device:
    """Make ``device`` current for the duration of a launch (kernels launch on the HIP current device)."""

    __slots__ = ("dev", "prev")

    def __init__(self, device):
        self.dev = device.index if device.index is not None else torch.cuda.current_device()
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.dev:
            self.prev = cur
            torch.cuda.set_device(self.dev)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


def int_array(values):
    return (ctypes.c_int * len(values))(*values)


def i64_array(values):
    return (ctypes.c_int64 * len(values))(*values)


def bump():
    global calls
    calls += 1


def ptr(t):
    """``t.data_ptr()``, or None (a NULL pointer) for an optional tensor that is absent."""
    return t.data_ptr() if t is not None else None


def launch(name, device, *args, what=None, count=True, raw=False):
    """Call the stream-taking entry point ``name`` on ``device``'s current stream: ``device`` is made current for the call and its
    stream handle is appended to ``args``.  ``count`` adds the call to ``calls`` whatever it returns (``count="ok"``: only when the
    code is not negative -- an entry point that declines a configuration has launched nothing, and its caller takes another one).
    The code goes through ``check(rc, what or name)``; with ``raw`` it is returned instead, for callers it steers."""
    global calls
    if count is not True and count is not False and count != "ok":
        raise ValueError(f"launch({name}): count must be True, False or 'ok', got {count!r}")
    fn = getattr(load(), name)
    with on_device(device):
        rc = fn(*args, stream_ptr(device))
    if count is True or (count == "ok" and rc >= 0):
        calls += 1
    if raw:
        return rc
    check(rc, what or name)
