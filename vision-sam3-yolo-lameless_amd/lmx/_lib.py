"""ctypes loader for liblmx.so (built in-tree by ``csrc/Makefile`` / ``__graft_entry__.build``).

Fails loudly: a missing library is an ImportError, a failed call raises ``LmxError`` with the C side's message.
Nothing here (or anywhere in the package) falls back to a CPU path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LMX_LIB: development builds only (csrc/Makefile `dbg`); the product loads the in-tree liblmx.so
LIB_PATH = os.environ.get("LMX_LIB") or os.path.join(_HERE, "liblmx.so")


class LmxError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_void_p), ("res", C.c_void_p),
        ("C", C.c_void_p),
        ("lda", C.c_int64), ("ldc", C.c_int64), ("ldr", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("act", C.c_int32), ("out_dtype", C.c_int32), ("a_mode", C.c_int32),
        ("H", C.c_int32), ("W_", C.c_int32), ("Cin", C.c_int32), ("conv_stride", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32), ("res_rows", C.c_int32), ("a_rep", C.c_int32), ("split_k", C.c_int32), ("split_stride", C.c_int64),
        ("ln_out", C.c_void_p), ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ld_ln", C.c_int64), ("ln_eps", C.c_float),
    ]


class DinoInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("arch", "hidden", "heads", "layers", "tokens", "image", "patch", "gated", "recipe_kind", "max_batch")]


class YoloInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("scale", "nc", "imgsz", "kpt_k", "kpt_ndim", "plans", "max_batch")]


class SamInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("encoder", "hidden", "heads", "layers", "mlp", "window", "patch", "image", "plans", "max_batch")]


class FusedInfo(C.Structure):  # lmx_fused_info_t
    _fields_ = [("yolo", YoloInfo), ("sam", SamInfo), ("dino", DinoInfo)] + [(n, C.c_int32) for n in ("hidden", "max_det", "max_frames", "sam_chunk",
                                                                                                        "sam_lanes", "max_streams")]


class HieraConfig(C.Structure):  # lmx_hiera_config_t
    MAX_STAGES, MAX_GLOBAL, MAX_BLOCKS = 8, 32, 256
    _fields_ = [("hidden", C.c_int32), ("n_stages", C.c_int32), ("blocks", C.c_int32 * 8), ("dims", C.c_int32 * 8), ("heads", C.c_int32 * 8),
                ("windows", C.c_int32 * 8), ("n_global", C.c_int32), ("global_blocks", C.c_int32 * 32), ("pos_bkg", C.c_int32 * 2),
                ("q_pool_stages", C.c_int32), ("fpn_dim", C.c_int32), ("n_top_down", C.c_int32), ("fpn_top_down", C.c_int32 * 8),
                ("image", C.c_int32), ("eps", C.c_double)]


class HieraBlock(C.Structure):  # lmx_hiera_block_t: lmx.sam.BlockPlan's fields in its order
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "Hf", "Ho", "Wo", "Hfo", "join", "attn", "ln1", "shortcut", "query", "window", "ln_out", "mlp",
                                         "emit_ln1", "stage_end", "keep", "x16", "join_out", "clone")]


class RecordField(C.Structure):  # lmx_record_field_t
    _fields_ = [("src", C.c_void_p), ("row_bytes", C.c_int64), ("offset", C.c_int64), ("map", C.c_int32), ("n_src", C.c_int32)]


class RecordFieldLayout(C.Structure):  # lmx_record_field_layout_t
    _fields_ = [("name", C.c_char * 16), ("dtype", C.c_int32), ("ndim", C.c_int32), ("shape", C.c_int64 * 2), ("offset", C.c_int64),
                ("nbytes", C.c_int64)]


class RecordLayout(C.Structure):  # lmx_record_layout_t
    MAX_FIELDS, MAX_MAPS = 16, 4
    _fields_ = [("n_fields", C.c_int32), ("reserved", C.c_int32), ("stride", C.c_int64), ("fields", RecordFieldLayout * 16)]


class YuvFrames(C.Structure):  # lmx_yuv_frames_t
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("pitch_y", C.c_int64), ("pitch_c", C.c_int64), ("stride_y", C.c_int64),
                ("stride_c", C.c_int64), ("layout", C.c_int32), ("matrix", C.c_int32)]


class YuvOut(C.Structure):  # lmx_yuv_out_t: lmx_yuv_frames_t with writable planes
    _fields_ = YuvFrames._fields_


class Rect(C.Structure):  # lmx_rect_t
    _fields_ = [(n, C.c_int32) for n in ("x", "y", "w", "h")]


class TleapLocomotion(C.Structure):  # lmx_tleap_locomotion_t: bit i of `present` is field i
    KEYS = ("back_arch_mean", "back_arch_std", "back_arch_score", "head_bob_magnitude", "head_bob_frequency", "head_bob_score",
            "stride_fl_mean", "stride_fl_std", "stride_fr_mean", "stride_fr_std", "stride_rl_mean", "stride_rl_std", "stride_rr_mean",
            "stride_rr_std", "front_leg_asymmetry", "rear_leg_asymmetry", "lameness_score")
    _fields_ = [(k, C.c_double) for k in KEYS] + [("present", C.c_uint32), ("reserved", C.c_uint32)]


class TcnWeights(C.Structure):  # lmx_tcn_weights_t: device pointers for lmx_k_tcn_forward, host pointers for lmx_h_tcn_forward
    MAX_BLOCKS = 8
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "n_blocks", "k", "head")] + [
        ("channels", C.c_int32 * 8), ("conv_w", (C.c_void_p * 2) * 8), ("conv_b", (C.c_void_p * 2) * 8), ("res_w", C.c_void_p * 8),
        ("res_b", C.c_void_p * 8), ("fc1_w", C.c_void_p), ("fc1_b", C.c_void_p), ("fc2_w", C.c_void_p), ("fc2_b", C.c_void_p)]


class TcnInfo(C.Structure):  # lmx_tcn_info_t
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "n_blocks", "k", "head", "receptive_field", "max_clips", "max_samples")] + [
        ("channels", C.c_int32 * 8), ("p", C.c_double)]


class XfmWeights(C.Structure):  # lmx_xfm_weights_t: device pointers for lmx_k_xfm_forward, host pointers for lmx_h_xfm_forward
    MAX_LAYERS = 8
    LAYER_FIELDS = ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_g", "ln2_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "d_model", "n_heads", "n_layers", "ff", "head", "max_len", "reserved")] + [
        (n, C.c_void_p) for n in ("in_w", "in_b", "pe")] + [(n, C.c_void_p * 8) for n in LAYER_FIELDS] + [
        (n, C.c_void_p) for n in ("lnf_g", "lnf_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class XfmInfo(C.Structure):  # lmx_xfm_info_t
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "d_model", "n_heads", "n_layers", "ff", "head", "max_len", "max_clips", "max_samples",
                                         "reserved")] + [("p", C.c_double)]


class GfmWeights(C.Structure):  # lmx_gfm_weights_t: device pointers for lmx_k_gfm_forward, host pointers for lmx_h_gfm_forward
    MAX_LAYERS = 8
    HEAD_FIELDS = ("in_w", "in_b", "in_g", "in_beta", "deg_in", "deg_out", "time_w", "time_b", "div_term", "spd", "e1_w", "e1_b", "e2_w", "e2_b")
    LAYER_FIELDS = ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_g", "ln2_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b", "vn", "vqkv_w",
                    "vqkv_b", "vout_w", "vout_b")
    TAIL_FIELDS = ("vu1_w", "vu1_b", "vu2_w", "vu2_b", "vu_g", "vu_beta", "lnf_g", "lnf_b", "pool1_w", "pool1_b", "pool2_w", "pool2_b", "comb_w",
                   "comb_b", "comb_g", "comb_beta", "ph1_w", "ph1_b", "ph2_w", "ph2_b", "ph3_w", "ph3_b", "nh1_w", "nh1_b", "nh2_w", "nh2_b")
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "d_model", "n_heads", "n_layers", "ff", "edge_dim", "max_degree", "max_spd")] + [
        (n, C.c_void_p) for n in HEAD_FIELDS] + [(n, C.c_void_p * 8) for n in LAYER_FIELDS] + [(n, C.c_void_p) for n in TAIL_FIELDS]


class GfmGraphs(C.Structure):  # lmx_gfm_graphs_t: the two offset arrays on the host, the rest where the forward runs
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_void_p) for n in (
        "node_off_host", "edge_off_host", "x", "timestamps", "has_time", "deg_in", "deg_out", "idx", "win", "edge_attr", "target")]


class GfmInfo(C.Structure):  # lmx_gfm_info_t
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "d_model", "n_heads", "n_layers", "ff", "edge_dim", "max_degree", "max_spd", "max_nodes",
                                         "max_graphs", "max_nodes_total", "max_samples")] + [("p", C.c_double)]


class GnnWeights(C.Structure):  # lmx_gnn_weights_t: device pointers for lmx_k_gnn_forward, host pointers for lmx_h_gnn_forward
    MAX_LAYERS = 4
    HEAD_FIELDS = ("in_w", "in_b", "lap1_w", "lap1_b", "lap2_w", "lap2_b", "lap_g", "lap_beta", "rw1_w", "rw1_b", "rw2_w", "rw2_b", "rw_g", "rw_beta",
                   "ee1_w", "ee1_b", "ee2_w", "ee2_b", "ee_g", "ee_beta")
    LAYER_FIELDS = ("ln1_g", "ln1_b", "abde_w", "abde_b", "c_w", "c_b", "eu1_w", "eu1_b", "eu2_w", "eu2_b", "bne_g", "bne_b", "bne_mean", "bne_var",
                    "bnn_g", "bnn_b", "bnn_mean", "bnn_var", "ln2_g", "ln2_b", "qkv_w", "qkv_b", "out_w", "out_b", "lna_g", "lna_b", "ln3_g", "ln3_b",
                    "ff1_w", "ff1_b", "ff2_w", "ff2_b")
    TAIL_FIELDS = ("lnf_g", "lnf_b", "nh1_w", "nh1_b", "nh2_w", "nh2_b", "na1_w", "na1_b", "na2_w", "na2_b", "cl1_w", "cl1_b", "cl2_w", "cl2_b",
                   "cl3_w", "cl3_b")
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "d_model", "n_heads", "n_layers", "pe_dim", "ff", "edge_dim", "reserved")] + [
        (n, C.c_void_p) for n in HEAD_FIELDS] + [(n, C.c_void_p * 4) for n in LAYER_FIELDS] + [(n, C.c_void_p) for n in TAIL_FIELDS]


class GnnGraphs(C.Structure):  # lmx_gnn_graphs_t: the two offset arrays on the host, the rest where the forward runs
    _fields_ = [("n", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_void_p) for n in (
        "node_off_host", "edge_off_host", "x", "lap", "rw", "edge_src", "edge_dst", "edge_attr", "csr_ptr", "csr_edge", "deg")]


class GnnInfo(C.Structure):  # lmx_gnn_info_t
    _fields_ = [(n, C.c_int32) for n in ("input_dim", "d_model", "n_heads", "n_layers", "pe_dim", "ff", "edge_dim", "max_nodes", "max_edges",
                                         "max_graphs", "max_nodes_total", "max_edges_total", "max_samples", "reserved")] + [("p", C.c_double)]


class TensorRow(C.Structure):  # lmx_tensor_row_t: one row of a model's weight table (lmx_h_<model>_tensors)
    _fields_ = [("name", C.c_char * 48), ("rank", C.c_int32), ("shape", C.c_int32 * 4), ("reserved", C.c_int32), ("pointer_at", C.c_int64)]


class LetterboxGeo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sh", "sw", "rh", "rw", "top", "left", "oh", "ow")] + [(n, C.c_double) for n in ("gain", "pad_x", "pad_y")]


class AttnDesc(C.Structure):
    _fields_ = [
        ("Q", C.c_void_p), ("K", C.c_void_p), ("V", C.c_void_p), ("O", C.c_void_p),
        ("ldq", C.c_int64), ("ldk", C.c_int64), ("ldv", C.c_int64), ("ldo", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32), ("hd", C.c_int32),
        ("scale", C.c_float), ("mode", C.c_int32),
        ("Gh", C.c_int32), ("Gw", C.c_int32), ("ws", C.c_int32), ("q_stride", C.c_int32),
        ("pad_k", C.c_void_p), ("pad_v", C.c_void_p),
        ("rel", C.c_void_p), ("rel_S", C.c_int32),
    ]


# name -> (restype, argtypes); must list every symbol include/lmx.h declares (tests/test_abi.py checks both ways)
_VP, _I, _I64, _F, _D = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
SIGNATURES = {
    "lmx_version": (_I, []),
    "lmx_last_error": (C.c_char_p, []),
    "lmx_device_count": (_I, []),
    "lmx_k_gemm": (_I, [C.POINTER(GemmDesc), _VP]),
    "lmx_dbg_set_gemm2_variant": (None, [_I]),
    "lmx_h_gemm_route": (_I, [C.POINTER(GemmDesc), C.c_char_p, _I]),
    "lmx_h_attn_route": (_I, [C.POINTER(AttnDesc), C.c_char_p, _I]),
    "lmx_h_layernorm_route": (_I, [_I, _I, _I, _I, _I, C.c_char_p, _I]),
    "lmx_k_pose_gather": (_I, [_VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _F, _F, _F, _F, _F, _VP, _VP]),
    "lmx_k_pack_bits": (_I, [_VP, _I64, _I, _VP, _VP]),
    "lmx_k_pack_records": (_I, [C.POINTER(RecordField), _I, C.POINTER(_VP), _I, _I64, _I64, _I64, _VP, _VP]),
    "lmx_h_record_layout": (_I, [_I, _I, _I, _I, _I, C.POINTER(RecordLayout)]),
    "lmx_h_stream_plan": (_I, [_I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int32)]),
    "lmx_h_row_map": (_I, [_I, C.POINTER(C.c_int32), _I, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lmx_k_ln_mlp": (_I, [_VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _I64, _I, _F, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_k_hiera_attn8": (_I, [_VP, _VP, _I64, _VP, _VP, _F, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _F, _VP]),
    "lmx_k_hiera_attn4": (_I, [_VP, _VP, _I64, _VP, _VP, _I, _I, _I, _I, _I, _F, _VP]),
    "lmx_k_hiera_attn_pool": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _F, _VP]),
    "lmx_k_ln_mlp_img": (_I, [_VP, _I64, _VP, _VP, _I64, _I, _F, _VP, _VP, _VP]),
    "lmx_k_layernorm": (_I, [_VP, _I, _I64, _VP, _VP, _VP, _I, _I64, _I, _I, _F, _I, _VP]),
    "lmx_k_attention": (_I, [C.POINTER(AttnDesc), _VP]),
    "lmx_k_relpos_tables": (_I, [C.POINTER(AttnDesc), _VP, _VP, _I, _VP, _VP]),
    "lmx_k_rope": (_I, [_VP, _I64, _I, _I, _I, _I, _I, _VP, _VP, _VP]),
    "lmx_k_pil_resize_h": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _I, _I, _VP]),
    "lmx_k_pil_resize_v": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _I, _VP]),
    "lmx_k_patchify_norm": (_I, [_VP, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _I64, _VP, _VP]),
    "lmx_k_float_resize_patchify": (_I, [_VP, _VP, _I, _I, _I, _I, _I, _I, _I64, _VP, _VP, _I, _VP, _VP, _I, _I, _F, _VP, _I, _VP]),
    "lmx_k_yuv420_to_bgr": (_I, [C.POINTER(YuvFrames), _I, _I, _I, _VP, _VP]),
    "lmx_h_yuv420_to_bgr": (_I, [C.POINTER(YuvFrames), _I, _I, _I, _VP]),
    "lmx_k_yuv420_to_bgr_roi": (_I, [C.POINTER(YuvFrames), _I, _I, _I, C.POINTER(Rect), _VP, _VP]),
    "lmx_h_yuv420_to_bgr_roi": (_I, [C.POINTER(YuvFrames), _I, _I, _I, C.POINTER(Rect), _VP]),
    "lmx_k_bgr_to_yuv420": (_I, [_VP, _I64, _I64, _I, _I, _I, C.POINTER(YuvOut), _VP]),
    "lmx_h_bgr_to_yuv420": (_I, [_VP, _I64, _I64, _I, _I, _I, C.POINTER(YuvOut)]),
    "lmx_h_crop_box": (_I, [C.POINTER(C.c_float), _I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "lmx_frame_quality_workspace_bytes": (_I64, [_I, _I, _I]),
    "lmx_k_frame_quality": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP]),
    "lmx_h_frame_quality": (_I, [_VP, _I, _I, _I, _VP]),
    "lmx_k_assemble_tokens": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "lmx_k_token_mean": (_I, [_VP, _I, _VP, _I, _I, _I, _VP]),
    "lmx_k_swiglu": (_I, [_VP, _I64, _VP, _I64, _I, _I, _VP]),
    "lmx_nms_workspace_bytes": (_I64, [_I, _I]),
    "lmx_k_nms": (_I, [_VP, _I, _I, _I, _F, _D, _I, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_k_letterbox": (_I, [_VP, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _I, _VP]),
    "lmx_k_stem_conv": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "lmx_k_split3": (_I, [_VP, _I64, _I, _VP, _I64, _VP, _I64, _I64, _I, _I, _I, _I64, _VP]),
    "lmx_k_maxpool5_x3": (_I, [_VP, _I64, _VP, _I64, _I, _I, _I, _I, _VP]),
    "lmx_k_stem_conv_x3": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "lmx_k_attention_f32": (_I, [_VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _I, _I, _I, _I, _I, _F, _VP]),
    "lmx_k_hyper_mask_f32": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "lmx_k_maxpool5": (_I, [_VP, _I64, _VP, _I64, _I, _I, _I, _I, _VP]),
    "lmx_k_upsample2": (_I, [_VP, _I64, _VP, _I64, _I, _I, _I, _I, _VP]),
    "lmx_k_detect_decode": (_I, [_VP, _I64, _VP, _I, _I, _I, _I, _F, _I, _I, _VP]),
    "lmx_k_scale_boxes": (_I, [_VP, _I, _F, _F, _F, _F, _F, _VP]),
    "lmx_k_im2col_u8": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I64, _VP]),
    "lmx_k_maxpool2": (_I, [_VP, _I64, _VP, _I64, _I, _I, _I, _I, _I, _VP]),
    "lmx_k_cast_f32_f16": (_I, [_VP, _I64, _VP, _I64, _I64, _I, _VP]),
    "lmx_h_hiera_band": (_I, [C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _I, _I, C.POINTER(C.c_int)]),
    "lmx_h_hiera_bands": (_I, [C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _I, _I, C.POINTER(C.c_int)]),
    "lmx_k_band_join": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP]),
    "lmx_h_hiera_blocks": (_I, [C.POINTER(HieraConfig), C.POINTER(C.c_int)]),
    "lmx_h_hiera_plan_rows": (_I, [C.POINTER(HieraConfig), _I, C.POINTER(C.c_int), _I, C.POINTER(HieraBlock)]),
    "lmx_h_hiera_plan": (_I, [C.POINTER(HieraConfig), _I, _I, _I, _I, C.POINTER(HieraBlock), C.POINTER(C.c_int)]),
    "lmx_k_add_bcast":(_I, [_VP, _I, _I64, _VP, _I64, _I, _VP, _I, _I64, _I64, _I, _VP]),
    "lmx_h_mask_features": (_I, [_VP, _I, _I, _VP]),
    "lmx_h_iou_matrix": (_I, [_VP, _I, _VP, _I, _VP]),
    "lmx_h_assign": (_I, [_VP, _I, _I, _VP, _VP]),
    "lmx_contour_workspace_bytes": (_I64, [_I, _I, _I]),
    "lmx_k_contour_features": (_I, [_VP, _I, _I, _I, _VP, _VP, _VP]),
    "lmx_k_prompt_box": (_I, [_VP, _I64, _VP, _I, _D, _D, _F, _VP, _VP, _I, _VP]),
    "lmx_k_hyper_mask": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP]),
    "lmx_k_mask_post": (_I, [_VP, _I, _I, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "lmx_k_prompt_points": (_I, [_VP, _VP, _I, _VP, _I64, _VP, _I, _D, _D, _F, _VP, _VP, _VP, _VP, _I, _VP]),
    "lmx_k_mask_embed": (_I, [_VP, _VP, _I, _I64, _VP, _VP, _I64, _I, _I, _VP]),
    "lmx_k_hyper_mask_multi": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "lmx_k_hyper_mask_multi_f32": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _VP]),
    "lmx_k_mask_logits": (_I, [_VP, _I, _I, _I, _I, _I, _I, _I, _VP, _VP]),
    "lmx_k_mask_score": (_I, [_VP, _I, _I, _I, _I, _I, _I, _I, _D, _D, _VP, _VP, _VP]),
    "lmx_k_nms_boxes": (_I, [_VP, _I64, _VP, _VP, _I, _D, _VP, _VP, _VP, _VP]),
    "lmx_h_pil_tables": (_I, [_I, _I, _I, _VP, _VP, _I64, C.POINTER(C.c_int)]),
    "lmx_h_aa_tables": (_I, [_I, _I, _I, _VP, _VP, _I64, C.POINTER(C.c_int)]),
    "lmx_h_identity_table": (_I, [_I, _VP, _VP]),
    "lmx_h_segment_cols": (_I, [_VP, _I, _I]),
    "lmx_dino_image_check_host": (_I, [C.c_char_p, C.POINTER(DinoInfo)]),
    "lmx_dino_open_host": (_I, [C.c_char_p, _I, C.POINTER(_VP)]),
    "lmx_dino_close": (None, [_VP]),
    "lmx_dino_info": (_I, [_VP, C.POINTER(DinoInfo)]),
    "lmx_dino_prepare": (_I, [_VP, _I, _I]),
    "lmx_dino_embed": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP]),
    "lmx_dino_embed_host": (_I, [_VP, _VP, _I, _I, _I, _I, _VP]),
    "lmx_h_letterbox_geometry": (_I, [_I, _I, _I, _I, _I, C.POINTER(LetterboxGeo)]),
    "lmx_h_letterbox_tables": (_I, [_I, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "lmx_h_conv_split_k": (_I, [_I64, _I, _I, _I]),
    "lmx_yolo_image_check_host": (_I, [C.c_char_p, C.POINTER(YoloInfo)]),
    "lmx_yolo_open_host": (_I, [C.c_char_p, _I, C.POINTER(_VP)]),
    "lmx_yolo_close": (None, [_VP]),
    "lmx_yolo_info": (_I, [_VP, C.POINTER(YoloInfo)]),
    "lmx_yolo_class_name": (C.c_char_p, [_VP, _I]),
    "lmx_yolo_prepare": (_I, [_VP, _I, _I, _I]),
    "lmx_yolo_anchors": (_I, [_VP, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lmx_yolo_predict": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP]),
    "lmx_yolo_detect": (_I, [_VP, _VP, _I, _I, _I, _I, _F, _D, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_yolo_detect_host": (_I, [_VP, _VP, _I, _I, _I, _I, _F, _D, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_sam_image_check_host": (_I, [C.c_char_p, C.POINTER(SamInfo)]),
    "lmx_sam_open_host": (_I, [C.c_char_p, _I, C.POINTER(_VP)]),
    "lmx_sam_close": (None, [_VP]),
    "lmx_sam_info": (_I, [_VP, C.POINTER(SamInfo)]),
    "lmx_sam_resized": (_I, [_VP, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lmx_sam_prepare": (_I, [_VP, _I, _I, _I]),
    "lmx_sam_encode": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP]),
    "lmx_sam_decode": (_I, [_VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_sam_segment": (_I, [_VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_sam_segment_host": (_I, [_VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_fused_open_host": (_I, [C.c_char_p, C.c_char_p, C.c_char_p, _I, _I, _I, _I, C.POINTER(_VP)]),
    "lmx_fused_close": (None, [_VP]),
    "lmx_fused_info": (_I, [_VP, C.POINTER(FusedInfo)]),
    "lmx_fused_layout": (_I, [_VP, _I, _I, _I, C.POINTER(RecordLayout)]),
    "lmx_fused_prepare": (_I, [_VP, _I, _I, _I]),
    "lmx_fused_schedule": (_I, [_VP, _I, C.POINTER(C.c_int32), _I, C.POINTER(C.c_int32), _I]),
    "lmx_fused_step": (_I, [_VP, _VP, _I, _I, _I, _I, _F, _VP, _I64, _VP]),
    "lmx_fused_step_host": (_I, [_VP, _VP, _I, _I, _I, _I, _F, _VP, _I64]),
    "lmx_fused_step_yuv": (_I, [_VP, C.POINTER(YuvFrames), _I, _I, _I, _I, _F, _VP, _I64, _VP]),
    "lmx_fused_step_yuv_roi": (_I, [_VP, C.POINTER(YuvFrames), _I, _I, _I, C.POINTER(Rect), _I, _F, _VP, _I64, _VP]),
    "lmx_fused_step_yuv_host": (_I, [_VP, _VP, _I, _I, _I, _I, _I, _I, _F, _VP, _I64]),
    "lmx_h_tcn_keep_bits": (_I, [C.c_uint64, _I, _I, _I, _I64, _D, _VP]),
    "lmx_tcn_workspace_bytes": (_I64, [_I]),
    "lmx_k_tcn_forward": (_I, [C.POINTER(TcnWeights), _VP, _VP, _I, _I, _I, _D, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_tcn_forward": (_I, [C.POINTER(TcnWeights), _VP, _VP, _I, _I, _I, _D, _VP, _VP, _VP]),
    "lmx_h_tcn_features": (_I, [_VP, _VP, _VP, _I, _I, _VP]),
    "lmx_tcn_image_check_host": (_I, [C.c_char_p, C.POINTER(TcnInfo)]),
    "lmx_tcn_open_host": (_I, [C.c_char_p, _I, _I, C.POINTER(_VP)]),
    "lmx_tcn_close": (None, [_VP]),
    "lmx_tcn_info": (_I, [_VP, C.POINTER(TcnInfo)]),
    "lmx_tcn_score": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP]),
    "lmx_tcn_score_host": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP]),
    "lmx_xfm_workspace_bytes": (_I64, [_I]),
    "lmx_k_xfm_forward": (_I, [C.POINTER(XfmWeights), _VP, _VP, _VP, _I, _I, _I, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_xfm_forward": (_I, [C.POINTER(XfmWeights), _VP, _VP, _VP, _I, _I, _I, _D, _VP, _VP, _VP, _VP]),
    "lmx_h_xfm_mask": (_I, [_VP, _VP, _VP, _I, _I, _VP]),
    "lmx_xfm_image_check_host": (_I, [C.c_char_p, C.POINTER(XfmInfo)]),
    "lmx_xfm_open_host": (_I, [C.c_char_p, _I, _I, C.POINTER(_VP)]),
    "lmx_xfm_close": (None, [_VP]),
    "lmx_xfm_info": (_I, [_VP, C.POINTER(XfmInfo)]),
    "lmx_xfm_score": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP]),
    "lmx_xfm_score_host": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP]),
    "lmx_tleap_workspace_bytes": (_I64, [_I, _I]),
    "lmx_k_tleap_series": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_tleap_series": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "lmx_h_tleap_locomotion": (_I, [_VP, _I, C.POINTER(C.c_char_p), C.POINTER(TleapLocomotion)]),
    "lmx_h_gfm_graph": (_I, [_VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_gfm_workspace_bytes": (_I64, [_I, _I64, _I]),
    "lmx_k_gfm_forward": (_I, [C.POINTER(GfmWeights), C.POINTER(GfmGraphs), _VP, _I, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_gfm_forward": (_I, [C.POINTER(GfmWeights), C.POINTER(GfmGraphs), _VP, _I, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_gfm_image_check_host": (_I, [C.c_char_p, C.POINTER(GfmInfo)]),
    "lmx_gfm_open_host": (_I, [C.c_char_p, _I, _I, _I, C.POINTER(_VP)]),
    "lmx_gfm_close": (None, [_VP]),
    "lmx_gfm_info": (_I, [_VP, C.POINTER(GfmInfo)]),
    "lmx_gfm_score": (_I, [_VP, C.POINTER(GfmGraphs), _VP, _I, _VP, _VP, _VP, _VP, _VP]),
    "lmx_gfm_score_host": (_I, [_VP, C.POINTER(GfmGraphs), _VP, _I, _VP, _VP, _VP, _VP]),
    "lmx_h_gnn_graph": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_gnn_laplacian": (_I, [_VP, _I, _I, _VP, _VP]),
    "lmx_gnn_workspace_bytes": (_I64, [_I, _I, _I, _I, _I, _I]),
    "lmx_k_gnn_forward": (_I, [C.POINTER(GnnWeights), C.POINTER(GnnGraphs), _VP, _I, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_gnn_forward": (_I, [C.POINTER(GnnWeights), C.POINTER(GnnGraphs), _VP, _I, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_gnn_image_check_host": (_I, [C.c_char_p, C.POINTER(GnnInfo)]),
    "lmx_gnn_open_host": (_I, [C.c_char_p, _I, _I, _I, _I, C.POINTER(_VP)]),
    "lmx_gnn_close": (None, [_VP]),
    "lmx_gnn_info": (_I, [_VP, C.POINTER(GnnInfo)]),
    "lmx_gnn_score": (_I, [_VP, C.POINTER(GnnGraphs), _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lmx_gnn_score_host": (_I, [_VP, C.POINTER(GnnGraphs), _VP, _I, _VP, _VP, _VP, _VP, _VP]),
    "lmx_h_tcn_tensors": (_I, [C.c_char_p, C.POINTER(TcnWeights), C.POINTER(TensorRow), _I, C.POINTER(_I)]),
    "lmx_h_xfm_tensors": (_I, [C.c_char_p, C.POINTER(XfmWeights), C.POINTER(TensorRow), _I, C.POINTER(_I)]),
    "lmx_h_gfm_tensors": (_I, [C.c_char_p, C.POINTER(GfmWeights), C.POINTER(TensorRow), _I, C.POINTER(_I)]),
    "lmx_h_gnn_tensors": (_I, [C.c_char_p, C.POINTER(GnnWeights), C.POINTER(TensorRow), _I, C.POINTER(_I)]),
    "lmx_h_cosine_topk_workspace": (_I64, [_I64, _I, _I]),
    "lmx_h_cosine_topk_geometry": (_I, [_I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "lmx_k_cosine_topk": (_I, [_VP, _I64, _I, _I64, _VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "lmx_h_cosine_topk": (_I, [_VP, _I64, _I, _I64, _VP, _I, _VP, _I, _VP, _VP]),
    "lmx_k_unit_rows": (_I, [_VP, _I, _I64, _I, _VP, _I64, _VP]),
    "lmx_h_unit_rows": (_I, [_VP, _I, _I64, _I, _VP, _I64]),
    "lmx_vstore_open": (_I, [_I, _I64, C.POINTER(_VP)]),
    "lmx_vstore_close": (None, [_VP]),
    "lmx_vstore_count": (_I64, [_VP]),
    "lmx_vstore_gallery": (_I, [_VP, C.POINTER(_VP), C.POINTER(_I64)]),
    "lmx_vstore_put_host": (_I, [_VP, _I64, _VP, _I]),
    "lmx_vstore_append": (_I, [_VP, _VP, _I, _I64]),
    "lmx_vstore_get_host": (_I, [_VP, _I64, _VP]),
    "lmx_vstore_read_host": (_I, [_VP, _I64, _I64, _VP]),
    "lmx_vstore_restore_host": (_I, [_VP, _VP, _I64]),
    "lmx_vstore_search": (_I, [_VP, _VP, _I, _I, _VP, _I, _VP, _VP, _VP]),
    "lmx_vstore_search_host": (_I, [_VP, _VP, _I, _I, _VP, _I, _VP, _VP]),
}

_lib = None


def load():
    """Load liblmx.so and bind every declared symbol.  Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  lmx has no CPU fallback.")
    # torch first: the library's libamdhip64.so.7 then binds to the HIP runtime torch already loaded, the one that owns the
    # tensors and streams it is handed.  Loaded first, it pulls in ROCm's own HIP + HSA runtime beside the one torch ships,
    # and its first launch fails with "no ROCm-capable device is detected" (build() then smoke() in one process did so).
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH, mode=os.RTLD_NOW)  # resolve every symbol now: a broken build fails here, not mid-run
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().lmx_last_error().decode("utf-8", "replace")
        raise LmxError(f"{what} failed (rc={rc}): {msg}")
