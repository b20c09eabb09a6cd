"""ctypes binding of librefid_hip.so (the C ABI declared in include/refid_hip.h).

There is NO fallback: if the shared library is missing or an entry point fails, the
caller gets an exception.  Build it with ``python -m refid_amd.build``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librefid_hip.so")


class RefidHipError(RuntimeError):
    pass


class PwExtras(C.Structure):
    _fields_ = [
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_eps", C.c_float), ("ln_out", C.c_void_p),
        ("ld_ln_out", C.c_int),
        ("pool", C.c_void_p), ("pool_parts", C.c_int), ("inv_hw", C.c_float), ("hw", C.c_int), ("se_c", C.c_int),
        ("se_w1", C.c_void_p), ("se_b1", C.c_void_p), ("se_w2", C.c_void_p), ("se_b2", C.c_void_p),
        ("se_m", C.c_void_p), ("se_z1", C.c_void_p), ("se_s", C.c_void_p),
        ("xs_out", C.c_void_p), ("ld_xs_out", C.c_int),
        ("res2", C.c_void_p), ("ld_res2", C.c_int),
        ("out2", C.c_void_p), ("ld_out2", C.c_int),
    ]


class ConvDesc(C.Structure):
    _fields_ = [
        ("in_a", C.c_void_p), ("in_b", C.c_void_p),
        ("ld_a", C.c_int), ("ld_b", C.c_int),
        ("c_a", C.c_int), ("c_b", C.c_int),
        ("w_packed", C.c_void_p), ("bias", C.c_void_p),
        ("out", C.c_void_p), ("ld_out", C.c_int),
        ("res", C.c_void_p), ("ld_res", C.c_int),
        ("mask", C.c_void_p), ("ld_mask", C.c_int),
        ("n", C.c_int), ("h", C.c_int), ("w", C.c_int),
        ("ho", C.c_int), ("wo", C.c_int),
        ("cout", C.c_int), ("cout_pad", C.c_int), ("co_base", C.c_int),
        ("kh", C.c_int), ("kw", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
        ("mode", C.c_int),
        ("slope_pre", C.c_float), ("slope_post", C.c_float), ("slope_mask", C.c_float),
        ("algo", C.c_int),
        ("split_k", C.c_int), ("wino_tile", C.c_int),
        ("pw", C.POINTER(PwExtras)),
        ("mfma_terms", C.c_int),
        ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
        ("add2", C.c_void_p), ("ld_add2", C.c_int), ("out2", C.c_void_p), ("ld_out2", C.c_int),
        ("mask_mode", C.c_int),
    ]


WGRAD_MAX_GROUPS = 24    # == REFID_WGRAD_MAX_GROUPS in include/refid_hip.h


class WgradDesc(C.Structure):
    _fields_ = [
        ("g", C.c_void_p), ("ld_g", C.c_int), ("c_o", C.c_int),
        ("in_a", C.c_void_p), ("in_b", C.c_void_p),
        ("ld_a", C.c_int), ("ld_b", C.c_int),
        ("c_a", C.c_int), ("c_b", C.c_int),
        ("dw", C.c_void_p), ("db", C.c_void_p), ("slabs", C.c_void_p),
        ("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("ho", C.c_int), ("wo", C.c_int),
        ("kh", C.c_int), ("kw", C.c_int), ("stride", C.c_int), ("pad", C.c_int),
        ("i_base", C.c_int), ("i_total", C.c_int), ("o_real", C.c_int), ("algo", C.c_int),
        ("phase", C.c_int),
        ("groups", C.c_int),
        ("g_more", C.c_void_p * (WGRAD_MAX_GROUPS - 1)), ("in_a_more", C.c_void_p * (WGRAD_MAX_GROUPS - 1)),
        ("in_b_more", C.c_void_p * (WGRAD_MAX_GROUPS - 1)),
    ]


class SampleDesc(C.Structure):
    """refid_sample_desc: one sample of a raw batch (refid_amd.data.DeviceBatchAssembler fills the table)."""
    _fields_ = [
        ("events", C.c_void_p), ("n_events", C.c_longlong),
        ("first_stamp", C.c_float), ("last_stamp", C.c_float),
        ("height", C.c_int), ("width", C.c_int),
        ("frames", C.c_void_p), ("frame_stride", C.c_longlong), ("row_pitch", C.c_int),
        ("y0", C.c_int), ("x0", C.c_int),
        ("top", C.c_int), ("left", C.c_int),
        ("hflip", C.c_int), ("vflip", C.c_int), ("rot90", C.c_int),
    ]


class AssembleDesc(C.Structure):
    _fields_ = [
        ("samples_host", C.c_void_p), ("samples_dev", C.c_void_p),
        ("batch", C.c_int),
        ("m", C.c_int), ("n", C.c_int), ("layout", C.c_int),
        ("crop_h", C.c_int), ("crop_w", C.c_int),
        ("scratch", C.c_void_p),
        ("lq", C.c_void_p), ("voxel", C.c_void_p), ("gt", C.c_void_p),
    ]


class SingleDesc(C.Structure):
    """refid_single_desc: the single-image layout (lq, plain-bin voxel with voxel_norm, gt)."""
    _fields_ = [
        ("samples_host", C.c_void_p), ("samples_dev", C.c_void_p),
        ("batch", C.c_int),
        ("bins", C.c_int),
        ("crop_h", C.c_int), ("crop_w", C.c_int),
        ("norm", C.c_int),
        ("scratch", C.c_void_p),
        ("parts", C.c_void_p),
        ("lq", C.c_void_p), ("voxel", C.c_void_p), ("gt", C.c_void_p),
    ]


class SeqPair(C.Structure):
    """refid_seq_pair: one frame pair of a resident sequence (refid_amd.sequence.SequenceAssembler fills the table)."""
    _fields_ = [
        ("left", C.c_int), ("right", C.c_int),
        ("row0", C.c_longlong), ("row1", C.c_longlong),
        ("first_stamp", C.c_float), ("last_stamp", C.c_float),
    ]


class SeqDesc(C.Structure):
    _fields_ = [
        ("events", C.c_void_p), ("n_events", C.c_longlong),
        ("frames", C.c_void_p), ("n_frames", C.c_int),
        ("frame_stride", C.c_longlong), ("row_pitch", C.c_int), ("height", C.c_int), ("width", C.c_int), ("bgr", C.c_int),
        ("pairs_host", C.c_void_p), ("pairs_dev", C.c_void_p), ("n_pairs", C.c_int),
        ("m", C.c_int), ("n", C.c_int), ("layout", C.c_int),
        ("out_h", C.c_int), ("out_w", C.c_int),
        ("scratch", C.c_void_p),
        ("lq", C.c_void_p), ("voxel", C.c_void_p),
    ]


class SeqSingleDesc(C.Structure):
    """refid_seq_single_desc: single-image items (blurry frame + exposure window) of a resident sequence."""
    _fields_ = [
        ("events", C.c_void_p), ("n_events", C.c_longlong),
        ("frames", C.c_void_p), ("n_frames", C.c_int),
        ("frame_stride", C.c_longlong), ("row_pitch", C.c_int), ("height", C.c_int), ("width", C.c_int), ("bgr", C.c_int),
        ("items_host", C.c_void_p), ("items_dev", C.c_void_p), ("n_items", C.c_int),
        ("bins", C.c_int), ("norm", C.c_int),
        ("out_h", C.c_int), ("out_w", C.c_int),
        ("scratch", C.c_void_p),
        ("parts", C.c_void_p),
        ("lq", C.c_void_p), ("voxel", C.c_void_p),
    ]


class PngUnfilterDesc(C.Structure):
    """refid_png_unfilter_desc: the inflate output of n_frames PNGs of one size -> uint8 (n_frames, height, width, 3)."""
    _fields_ = [
        ("rows", C.c_void_p), ("frames", C.c_void_p), ("bands", C.c_void_p),
        ("n_bands", C.c_int32), ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
    ]


class PngFilterDesc(C.Structure):
    """refid_png_filter_desc: uint8 (n_frames, height, width, 3) -> the filtered rows deflate takes, filter byte first."""
    _fields_ = [
        ("frames", C.c_void_p), ("rows", C.c_void_p), ("costs", C.c_void_p),
        ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("mode", C.c_int32),
    ]


class PngDeflateDesc(C.Structure):
    """refid_png_deflate_desc: n_streams runs of filtered rows -> one zlib stream each (Huffman codes per block)."""
    _fields_ = [
        ("src", C.c_void_p), ("out", C.c_void_p), ("lens", C.c_void_p), ("work", C.c_void_p),
        ("n_streams", C.c_int32), ("stream_bytes", C.c_int32), ("block_bytes", C.c_int32), ("out_pitch", C.c_int32),
    ]


class JpegDesc(C.Structure):
    """refid_jpeg_desc: uint8 RGB frames (n_frames, height, width, 3) -> one baseline JFIF file each, for Motion-JPEG."""
    _fields_ = [
        ("frames", C.c_void_p), ("out", C.c_void_p), ("lens", C.c_void_p), ("work", C.c_void_p),
        ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("quality", C.c_int32), ("subsampling", C.c_int32),
        ("restart_mcus", C.c_int32), ("out_pitch", C.c_int32),
    ]


class JpegInfo(C.Structure):
    """refid_jpeg_info: what refid_jpeg_probe reads from a file's header and refid_jpeg_entropy_decode expects of it."""
    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32), ("components", C.c_int32), ("sampling", C.c_int32),
        ("blocks", C.c_int32 * 3), ("total_blocks", C.c_int32), ("restart_interval", C.c_int32),
    ]


class JpegDecodeDesc(C.Structure):
    """refid_jpeg_decode_desc: the coefficients and tables of n_frames JPEG files of one geometry -> uint8 (n_frames, height, width, 3)."""
    _fields_ = [
        ("coefs", C.c_void_p), ("quant", C.c_void_p), ("frames", C.c_void_p), ("work", C.c_void_p),
        ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("sampling", C.c_int32),
    ]


class EventSimDesc(C.Structure):
    """refid_event_sim_desc: uint8 frames + stamps -> event rows [t, x, y, p] by the ESIM model; ``stage`` names the launch."""
    _fields_ = [
        ("frames", C.c_void_p), ("stamps_host", C.c_void_p), ("stamps_dev", C.c_void_p), ("lut", C.c_void_p),
        ("c_pos_map", C.c_void_p), ("c_neg_map", C.c_void_p), ("state", C.c_void_p), ("counts", C.c_void_p), ("totals", C.c_void_p),
        ("ends", C.c_void_p), ("rows", C.c_void_p), ("keys", C.c_void_p), ("perm", C.c_void_p), ("sorted", C.c_void_p),
        ("n_rows", C.c_int64),
        ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("bgr", C.c_int32),
        ("c_pos", C.c_int32), ("c_neg", C.c_int32), ("c_min", C.c_int32), ("lut_min", C.c_int32), ("lut_max", C.c_int32),
        ("stage", C.c_int32),
    ]


class BlurSynthDesc(C.Structure):
    """refid_blur_synth_desc: uint8 frames + windows [first, count] -> one averaged uint8 frame per window (csrc/blur_synth.hip)."""
    _fields_ = [
        ("frames", C.c_void_p), ("windows_host", C.c_void_p), ("windows", C.c_void_p), ("to_linear_host", C.c_void_p),
        ("to_linear", C.c_void_p), ("out", C.c_void_p),
        ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("n_windows", C.c_int32), ("max_groups", C.c_int32),
    ]


class EdiDesc(C.Structure):
    """refid_edi_desc: key frames + the stream packed by pixel + items -> latent uint8 frames at instants (csrc/edi.hip)."""
    _fields_ = [
        ("frames", C.c_void_p), ("ev_t", C.c_void_p), ("ev_p", C.c_void_p), ("seg", C.c_void_p), ("items_host", C.c_void_p),
        ("items", C.c_void_p), ("bounds_host", C.c_void_p), ("bounds", C.c_void_p), ("samples_host", C.c_void_p), ("samples", C.c_void_p),
        ("instants_host", C.c_void_p), ("instants", C.c_void_p), ("tables", C.c_void_p), ("out", C.c_void_p), ("clamped", C.c_void_p),
        ("eps255", C.c_double), ("n_events", C.c_int64),
        ("n_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("n_items", C.c_int32), ("n_instants", C.c_int32),
        ("m", C.c_int32), ("exposure", C.c_int32), ("c_pos", C.c_int32), ("c_neg", C.c_int32),
    ]


LAYOUT_BLUR, LAYOUT_SHARP = 0, 1                # == REFID_LAYOUT_* in include/refid_hip.h
ASSEMBLE_ZERO, ASSEMBLE_SCATTER, ASSEMBLE_FINISH, ASSEMBLE_FRAMES, ASSEMBLE_ALL = 1, 2, 4, 8, 15
ASSEMBLE_STATS = 16                              # refid_assemble_single only: voxel_norm's statistics, between scatter and finish

VAL_TAIL_BGR = 1         # == REFID_VAL_TAIL_BGR in include/refid_hip.h
NIQE_BGR = 1             # == REFID_NIQE_BGR in include/refid_hip.h
SCORE_BGR = 1            # == REFID_SCORE_BGR in include/refid_hip.h
PNG_MAX_ROW_BYTES = 32760    # == REFID_PNG_MAX_ROW_BYTES in include/refid_hip.h
PNG_FILTER_ADAPTIVE = 5      # == REFID_PNG_FILTER_ADAPTIVE in include/refid_hip.h
PNG_FILTER_MAX_WIDTH = 11184810    # == REFID_PNG_FILTER_MAX_WIDTH in include/refid_hip.h
PNG_DEFLATE_BLOCK = 32768          # == REFID_PNG_DEFLATE_BLOCK in include/refid_hip.h
PNG_DEFLATE_MAX_BLOCK = 65535      # == REFID_PNG_DEFLATE_MAX_BLOCK in include/refid_hip.h
PNG_DEFLATE_RECORD = 1088          # == REFID_PNG_DEFLATE_RECORD in include/refid_hip.h
JPEG_444, JPEG_420 = 0, 1          # == REFID_JPEG_444 / REFID_JPEG_420 in include/refid_hip.h
JPEG_HEADER_BYTES = 625            # == REFID_JPEG_HEADER_BYTES in include/refid_hip.h
JPEG_BLOCK_BITS = 1660             # == REFID_JPEG_BLOCK_BITS in include/refid_hip.h
JPEG_DEC_GREY, JPEG_DEC_444, JPEG_DEC_422, JPEG_DEC_420 = 0, 1, 2, 3    # == REFID_JPEG_DEC_* in include/refid_hip.h
EVENT_SIM_RESET, EVENT_SIM_COUNT, EVENT_SIM_EMIT, EVENT_SIM_GATHER = 1, 2, 4, 8    # == REFID_EVENT_SIM_* in include/refid_hip.h
EVENT_SIM_CAP = 255                # == REFID_EVENT_SIM_CAP in include/refid_hip.h
EVENT_SIM_MAX_FRAMES = 512         # == REFID_EVENT_SIM_MAX_FRAMES in include/refid_hip.h
EVENT_SIM_MAX_PIXELS = 1 << 25     # == REFID_EVENT_SIM_MAX_PIXELS in include/refid_hip.h
EVENT_SIM_FLAG_OVERFLOW, EVENT_SIM_FLAG_SLOTS = 1, 2    # == REFID_EVENT_SIM_FLAG_* in include/refid_hip.h
BLUR_MAX_COUNT = 64                # == REFID_BLUR_MAX_COUNT in include/refid_hip.h
EDI_SAMPLES, EDI_CONTINUOUS = 0, 1 # == REFID_EDI_SAMPLES / REFID_EDI_CONTINUOUS in include/refid_hip.h
EDI_THREADS = 256                  # == REFID_EDI_THREADS in include/refid_hip.h
EDI_CLAMP = 32                     # == REFID_EDI_CLAMP in include/refid_hip.h
EDI_TABLE = 577                    # == REFID_EDI_TABLE in include/refid_hip.h
EDI_MAX_INSTANTS = 256             # == REFID_EDI_MAX_INSTANTS in include/refid_hip.h
EDI_MAX_ITEMS = 65535              # == REFID_EDI_MAX_ITEMS in include/refid_hip.h
EDI_MAX_PIXELS = 1 << 25           # == REFID_EDI_MAX_PIXELS in include/refid_hip.h
EDI_MAX_THRESHOLD = 1 << 20        # == REFID_EDI_MAX_THRESHOLD in include/refid_hip.h
ABI_VERSION = 9          # == REFID_ABI_VERSION in include/refid_hip.h
_lib = None

# The weight-packing family: (size function, its one-by-one entry points, the geometry arguments both take, in the C order)
_PACK_FAMILY = (
    ("refid_packed_weight_floats", ("refid_pack_conv_weights", "refid_pack_conv_weights_scaled", "refid_pack_conv_weights_bf16"),
     "role o i kh kw kc bn"),
    ("refid_packed_weight_split_bytes", ("refid_pack_conv_weights_split",), "role o i kh kw bn planes"),
    ("refid_packed_weight_split_f16_bytes", ("refid_pack_conv_weights_split_f16",), "role o i kh kw bn"),
    ("refid_packed_weight_wino6_bytes", ("refid_pack_conv_weights_wino6",), "role o i bn"),
    ("refid_packed_weight_wino3h_bytes", ("refid_pack_conv_weights_wino3h",), "role o i bn"),
    ("refid_packed_weight_wino1h_bytes", ("refid_pack_conv_weights_wino1h",), "role o i bn"),
)
PACK_GEO = {}            # C symbol -> names of its geometry arguments (filled when the library is bound)


def lib():
    """The loaded library; raises RefidHipError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RefidHipError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU/eager fallback). "
            "Run `python -m refid_amd.build`.")
    import torch  # noqa: F401  first: the library then binds the HIP runtime torch ships.  Loaded before torch it pulls in the
    #                             system's, torch brings its own, and of two runtimes in one process the second finds no device
    L = C.CDLL(LIB_PATH)
    L.refid_last_error.restype = C.c_char_p
    L.refid_abi_version.restype = C.c_int
    L.refid_device_cu_count.restype = C.c_int
    L.refid_conv2d.argtypes = [C.POINTER(ConvDesc), C.c_void_p]
    L.refid_conv_workspace_bytes.argtypes = [C.POINTER(ConvDesc)]
    L.refid_conv_workspace_bytes.restype = C.c_size_t
    L.refid_conv_kc.argtypes = [C.c_int] * 4
    L.refid_conv_bn.argtypes = [C.c_int] * 5
    L.refid_conv_tile_name.argtypes = [C.c_int] * 5
    L.refid_conv_tile_name.restype = C.c_char_p
    L.refid_wgrad_workspace_bytes.argtypes = [C.POINTER(WgradDesc)]
    L.refid_wgrad_workspace_bytes.restype = C.c_size_t
    L.refid_conv2d_wgrad.argtypes = [C.POINTER(WgradDesc), C.c_void_p]
    L.refid_wgrad_finish_flush.argtypes = [C.c_void_p]
    L.refid_rows_sum_defer.argtypes = [C.c_int]
    L.refid_rows_sum_flush.argtypes = [C.c_void_p]
    L.refid_nchw_to_nhwc.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    L.refid_nchw_tsum_to_nhwc.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p] + [C.c_int] * 5 + \
        [C.c_void_p]
    L.refid_nhwc_to_nchw.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong] + [C.c_int] * 4 + [C.c_void_p]
    L.refid_nchw_to_nhwc_tb.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    L.refid_nhwc_to_nchw_tb.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_longlong] + [C.c_int] * 5 + [C.c_void_p]
    L.refid_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    L.refid_sum_n.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
    L.refid_act_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_longlong, C.c_void_p]
    _bind_extra(L)
    if L.refid_abi_version() != ABI_VERSION:
        raise RefidHipError("librefid_hip.so ABI version mismatch")
    _lib = L
    return L


def _bind_extra(L):
    """EGACA / train-step entry points (a stale .so without them fails loudly here)."""
    vp, i, f, ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong
    for size, entries, geo in _PACK_FAMILY:
        PACK_GEO[size] = geo = tuple(geo.split())
        getattr(L, size).argtypes, getattr(L, size).restype = [i] * len(geo), C.c_size_t
        for e in entries:                                   # (w, [oscale,] packed, geometry..., stream)
            PACK_GEO[e] = geo
            getattr(L, e).argtypes = [vp] * (2 if e == "refid_pack_conv_weights" else 3) + [i] * len(geo) + [vp]
    L.refid_pack_batch_prepass.argtypes = [vp, i, vp]
    L.refid_mul_vec.argtypes = [vp, vp, vp, i, vp]
    L.refid_pack_entry_bytes.restype = C.c_size_t
    L.refid_pack_entry_bytes.argtypes = []
    L.refid_pack_entry_fill.argtypes = [vp, i, vp, vp, vp, i, i, i, i, i, i, i, i, i]
    L.refid_pack_batch.argtypes = [vp, i, i, vp]
    L.refid_pack_table_check.argtypes = [vp, i]
    L.refid_fold_back.argtypes = [vp] * 8 + [i, i, vp]
    L.refid_layernorm2d_fwd.argtypes = [vp, i, vp, vp, vp, i, ll, i, f, vp]
    L.refid_layernorm2d_bwd.argtypes = [vp, i, vp, i, vp, vp, i, vp, i, vp, vp, vp, ll, i, f, vp]
    L.refid_layernorm2d_bwd_parts.argtypes = [ll, i]
    L.refid_colsum_parts.argtypes = [ll, i]
    L.refid_egaca_gs_reduce_parts.argtypes = [i, i]
    L.refid_dwconv3x3_gelu_fwd.argtypes = [vp, i, vp, vp, vp, vp, vp, i, i, i, i, vp]
    L.refid_dwconv3x3_bwd.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, vp]
    L.refid_dwconv3x3_bwd_parts.argtypes = [i, i, i]
    L.refid_se_fwd.argtypes = [vp, i, f, vp, vp, vp, vp, vp, vp, vp, i, i, vp]
    L.refid_dwconv_pool_parts.argtypes = [i, i, i]
    L.refid_se_bwd.argtypes = [vp] * 12 + [i, i, vp]
    L.refid_scale_cat.argtypes = [vp, vp, vp, vp, i, i, i, vp]
    L.refid_egaca_gs_reduce.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp]
    L.refid_egaca_bwd_elem.argtypes = [vp, vp, vp, f, vp, vp, vp, i, i, i, i, vp]
    L.refid_gelu_fwd.argtypes = [vp, vp, ll, vp]
    L.refid_gelu_bwd.argtypes = [vp, vp, vp, ll, vp]
    L.refid_colsum.argtypes = [vp, i, vp, vp, ll, i, vp]
    L.refid_charbonnier_parts.argtypes = [ll]
    L.refid_charbonnier.argtypes = [vp, vp, vp, vp, vp, ll, f, f, vp]
    L.refid_grad_sqnorm.argtypes = [vp, vp, ll, vp]
    L.refid_psnr_loss_parts.argtypes = [i, ll]
    L.refid_psnr_loss.argtypes = [vp, vp, vp, vp, vp, vp, i, ll, f, vp]
    L.refid_clip_adamw.argtypes = [vp, vp, vp, vp, vp, f, f, f, f, f, f, f, i, ll, vp]
    L.refid_clip_adamw_dev.argtypes = [vp, vp, vp, vp, vp, f, f, vp, f, f, f, f, ll, vp]
    d = C.c_double
    L.refid_events_to_voxel.argtypes = [vp, vp, vp, vp, ll, i, i, i, d, d, vp, vp]
    L.refid_sqerr_u8_parts.argtypes = [i, ll]
    L.refid_sqerr_u8.argtypes = [vp, vp, i, ll, vp, vp, vp]
    L.refid_ssim3d_u8_parts.argtypes = [i, i, i]
    L.refid_ssim3d_u8.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    L.refid_val_tail_parts.argtypes = [i, i, i]
    L.refid_val_tail_parts.restype = ll
    L.refid_val_tail.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp]
    L.refid_tile_add.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, vp]
    L.refid_tile_normalize.argtypes = [vp, vp, i, i, i, vp]
    L.refid_hin_parts.argtypes = [i]
    L.refid_hin_lrelu_fwd.argtypes = [vp, i, vp, vp, vp, i, vp, vp, i, i, i, i, f, f, vp]
    L.refid_hin_lrelu_bwd.argtypes = [vp, i, vp, i, vp, i, vp, vp, vp, i, vp, vp, vp, vp, i, i, i, i, f, vp]
    L.refid_fac_fwd.argtypes = [vp, i, vp, i, vp, i, ll, i, vp]
    L.refid_fac_bwd.argtypes = [vp, i, vp, i, vp, i, vp, i, vp, i, ll, i, vp]
    L.refid_assemble_bins.argtypes = [i, i, i]
    L.refid_assemble_batch.argtypes = [C.POINTER(AssembleDesc), i, vp]
    L.refid_seq_assemble.argtypes = [C.POINTER(SeqDesc), i, vp]
    L.refid_voxel_norm_parts.argtypes = [i, ll]
    L.refid_voxel_norm_parts.restype = ll
    L.refid_voxel_norm.argtypes = [vp, vp, i, ll, vp, vp]
    L.refid_single_bins.argtypes = [i]
    L.refid_assemble_single.argtypes = [C.POINTER(SingleDesc), i, vp]
    L.refid_seq_assemble_single.argtypes = [C.POINTER(SeqSingleDesc), i, vp]
    L.refid_niqe_moments_parts.argtypes = [i, i, i]
    L.refid_niqe_moments_parts.restype = ll
    L.refid_niqe_moments.argtypes = [vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp]
    L.refid_png_unfilter.argtypes = [C.POINTER(PngUnfilterDesc), vp]
    L.refid_png_filter.argtypes = [C.POINTER(PngFilterDesc), vp]
    L.refid_png_deflate_bound.argtypes = [C.c_int32, C.c_int32]
    L.refid_png_deflate_bound.restype = C.c_size_t
    L.refid_png_deflate_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.refid_png_deflate_work_bytes.restype = C.c_size_t
    L.refid_png_deflate.argtypes = [C.POINTER(PngDeflateDesc), vp]
    L.refid_jpeg_encode.argtypes = [C.POINTER(JpegDesc), vp]
    L.refid_jpeg_header_bytes.argtypes = []
    L.refid_jpeg_header_bytes.restype = C.c_size_t
    L.refid_jpeg_bound.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.refid_jpeg_bound.restype = C.c_size_t
    L.refid_jpeg_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.refid_jpeg_work_bytes.restype = C.c_size_t
    L.refid_jpeg_probe.argtypes = [vp, C.c_size_t, C.POINTER(JpegInfo)]
    L.refid_jpeg_entropy_decode.argtypes = [vp, C.c_size_t, C.POINTER(JpegInfo), vp, vp]
    L.refid_jpeg_decode.argtypes = [C.POINTER(JpegDecodeDesc), vp]
    L.refid_jpeg_decode_work_bytes.argtypes = [C.c_int32] * 4
    L.refid_jpeg_decode_work_bytes.restype = C.c_size_t
    L.refid_jpeg_decode_blocks.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)]
    L.refid_jpeg_decode_blocks.restype = C.c_int32
    L.refid_event_sim.argtypes = [C.POINTER(EventSimDesc), vp]
    L.refid_event_sim_min_threshold.argtypes = [C.c_int32, C.c_int32]
    L.refid_event_sim_min_threshold.restype = C.c_int32
    L.refid_blur_synth.argtypes = [C.POINTER(BlurSynthDesc), vp]
    L.refid_edi.argtypes = [C.POINTER(EdiDesc), vp]
    L.refid_score_u8_parts.argtypes = [i, i, i, i]
    L.refid_score_u8_parts.restype = ll
    L.refid_score_u8.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]


def check(rc, what):
    if rc != 0:
        msg = lib().refid_last_error().decode("utf-8", "replace")
        raise RefidHipError(f"{what} failed (rc={rc}): {msg}")
