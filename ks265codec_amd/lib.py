"""ctypes binding of include/ks265_hip.h.  Device buffers are torch CUDA(HIP) tensors; only their
data_ptr() crosses the C ABI."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libks265hip.so")

# descriptor layouts of include/ks265_hip.h
BLK = np.dtype([("a_off", "<i4"), ("b_off", "<i4"), ("w", "<i4"), ("h", "<i4")])
BLK3 = np.dtype([("a_off", "<i4"), ("b_off", "<i4", 3), ("w", "<i4"), ("h", "<i4")])
EDGE = np.dtype([("pix_off", "<i4"), ("beta", "<i2"), ("tc", "<i2"), ("length", "<i2"), ("dir", "u1"), ("flags", "u1")])
SAO_RECT = np.dtype([("org_off", "<i4"), ("rec_off", "<i4"), ("w", "<i4"), ("h", "<i4")])
INTRA_BLK = np.dtype([("ref_off", "<i4"), ("dst_off", "<i4"), ("dst_stride", "<i2"), ("mode", "u1"), ("log2", "u1"), ("edge_filter", "u1"), ("rsv", "u1", (3,))])
INTRA_REF = np.dtype([("src_off", "<i4"), ("dst_off", "<i4"), ("size", "<i4"), ("strong_enabled", "<i4")])
PU = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("mvpx", "<i2"), ("mvpy", "<i2"), ("cost", "<u4"), ("dist", "<u4")])
CU8 = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("mv1x", "<i2"), ("mv1y", "<i2"), ("log2_cu", "u1"), ("cbf", "u1"), ("pred_mode", "u1"), ("inter_dir", "u1")])
PU_B = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("mv1x", "<i2"), ("mv1y", "<i2"), ("cost", "<u4"), ("inter_dir", "<u4")])
RDOQ_TU = np.dtype([("off", "<i4"), ("tab", "<i4"), ("dq", "<i4"), ("last_pos", "<i4"), ("lam", "<i8"), ("lam_sdh", "<i8"), ("log2", "i1"), ("scan_idx", "i1"), ("comp", "i1"), ("per", "i1"),
                    ("tu5", "i1"), ("flag_a4c0", "i1"), ("sdh", "i1"), ("rsv", "i1")])      # ks265_rdoq_tu
SAO_PARAM = np.dtype([("type", "i1"), ("band", "i1"), ("offset", "i1", 4), ("rsv", "i1", 2)])      # rsv of a CTU's luma record: [SAO_MERGE_LEFT], [SAO_MERGE_UP] (sao=3)
SAO_MERGE_LEFT, SAO_MERGE_UP = 0, 1


class FrameCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "qp", "lambda_q4", "me_range", "me_method", "subme", "deblock", "sao",
                                          "beta_offset_div2", "tc_offset_div2", "bframes", "refs", "me_hex_thr", "sdh", "pre_search", "merge", "bi_refine", "decimate", "rdo", "intra_inter", "propagate", "sub_satd", "sub_thr", "sub_flat", "sub_cap", "sub_cap_step", "sub_diag_fast", "part", "tu_inter", "skip_rd")]


class FrameGeom(C.Structure):
    _fields_ = [("pad_y", C.c_int32), ("pad_c", C.c_int32), ("stride_y", C.c_int32), ("stride_c", C.c_int32),
                ("rows_y", C.c_int32), ("rows_c", C.c_int32), ("bytes_y", C.c_int64), ("bytes_c", C.c_int64),
                ("ctu_cols", C.c_int32), ("ctu_rows", C.c_int32), ("pu_per_ctu", C.c_int32), ("bytes_pu", C.c_int64),
                ("bytes_cu8", C.c_int64), ("bytes_sao", C.c_int64)]


class Pic(C.Structure):
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p)]


class RoiDesc(C.Structure):                   # ks265_roi_desc
    _fields_ = [("type", C.c_int32), ("log2_block", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32), ("data", C.c_void_p), ("pitch", C.c_int32)]


ROI_INT8, ROI_FLOAT32 = 0, 1


class AnField(C.Structure):                   # ks265_an_field
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_int32), ("plane", C.c_int64)]


class AnalysisDesc(C.Structure):              # ks265_analysis_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("mv", AnField), ("ref", AnField), ("cu", AnField), ("qp", AnField), ("sse", AnField)]


ANALYSIS_FIELDS = ("mv", "ref", "cu", "qp", "sse")


def analysis_shapes(width: int, height: int) -> dict:
    """field -> (torch dtype name, shape) of a width x height picture's analysis (include/ks265_hip.h)"""
    w8, h8, cc, cr = (width + 7) // 8, (height + 7) // 8, (width + 63) // 64, (height + 63) // 64
    return {"mv": ("int16", (2, h8, w8, 2)), "ref": ("int8", (2, h8, w8)), "cu": ("uint8", (5, h8, w8)), "qp": ("int8", (cr, cc)), "sse": ("int32", (3, h8, w8))}


class InDesc(C.Structure):                    # ks265_in_desc
    _fields_ = [("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("plane", C.c_void_p * 3), ("pitch", C.c_int32 * 3),
                ("pixel_step", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


class DenoiseCfg(C.Structure):                # ks265_denoise_cfg
    _fields_ = [("thr", C.c_int32), ("weight", C.c_int32)]


class EnhanceCfg(C.Structure):                # ks265_enhance_cfg
    _fields_ = [("edge_gain", C.c_int32), ("edge_core", C.c_int32), ("edge_limit", C.c_int32), ("edge_over", C.c_int32), ("color_gain", C.c_int32)]


class HdrCfg(C.Structure):                    # ks265_hdr_cfg
    _fields_ = [("gain", C.c_int32), ("iters", C.c_int32), ("slope", C.c_int32), ("radius", C.c_int32 * 3)]

    @classmethod
    def of(cls, cfg):
        """cfg: (gain, iters, slope, (radius ...)) as tests/hdr_ref.py params() gives it"""
        gain, iters, slope, radius = cfg
        return cls(int(gain), int(iters), int(slope), (C.c_int32 * 3)(*[int(r) for r in tuple(radius)[:3]]))


class OverlayDesc(C.Structure):               # ks265_overlay_desc
    _fields_ = [("rgb", InDesc), ("alpha", C.c_void_p), ("x", C.c_int32), ("y", C.c_int32), ("opacity", C.c_int32)]


OVERLAY_MAX = 8


class TonemapCfg(C.Structure):                # ks265_tonemap_cfg
    _fields_ = [("transfer", C.c_int32), ("curve", C.c_int32), ("full_range", C.c_int32), ("peak_nits", C.c_double), ("white_nits", C.c_double)]


TONEMAP_PQ = 16                                           # H.273's transfer code of SMPTE ST 2084
TONEMAP_CURVES = {"bt2390": 0, "reinhard": 1, "clip": 2}

IN_I420, IN_NV12, IN_RGB = 0, 1, 2
IN_RGB_F16, IN_RGB_BF16, IN_RGB_F32 = 16, 17, 18          # RGB as float samples in [0, 1]: plane, pixel_step and pitch stay in bytes
RGB_ELEM_SIZE = {IN_RGB: 1, IN_RGB_F16: 2, IN_RGB_BF16: 2, IN_RGB_F32: 4}
YUV_PLANAR, YUV_SEMI, YUV_YUYV, YUV_UYVY = 0, 1, 2, 3     # KS265_IN_YUV's layout
YUV_420, YUV_422, YUV_444 = 0, 1, 2                       # and its subsampling


def in_yuv(layout: int, sub: int, depth: int = 8, msb: int = 0) -> int:
    """KS265_IN_YUV(layout, sub, depth, msb): 8- to 16-bit YUV in 4:2:0 / 4:2:2 / 4:4:4 (depth > 8: two-byte elements, msb = the sample is their top bits)"""
    return 0x1000 | layout << 8 | sub << 6 | int(bool(msb)) << 5 | depth


IN_I422, IN_I444, IN_NV16, IN_NV24, IN_YUYV, IN_UYVY = in_yuv(0, 1), in_yuv(0, 2), in_yuv(1, 1), in_yuv(1, 2), in_yuv(2, 1), in_yuv(3, 1)
IN_I010, IN_I210, IN_I410 = in_yuv(0, 0, 10), in_yuv(0, 1, 10), in_yuv(0, 2, 10)
IN_P010, IN_P012, IN_P016, IN_P210, IN_P410 = in_yuv(1, 0, 10, 1), in_yuv(1, 0, 12, 1), in_yuv(1, 0, 16, 1), in_yuv(1, 1, 10, 1), in_yuv(1, 2, 10, 1)
IN_Y210, IN_Y216 = in_yuv(2, 1, 10, 1), in_yuv(2, 1, 16, 1)


class Ks265Error(RuntimeError):
    pass


_lib = None

# every symbol include/ks265_hip.h declares (checked by tests/test_abi.py against the header text)
EXPORTS = [
    "ks265_create", "ks265_create_prio", "ks265_destroy", "ks265_set_stream", "ks265_synchronize", "ks265_take_device_error", "ks265_last_error", "ks265_version",
    "ks265_timer_start", "ks265_timer_stop_ms", "ks265_marker", "ks265_debug_set",
    "ks265_dev_malloc", "ks265_dev_free", "ks265_host_malloc", "ks265_host_free", "ks265_memcpy_h2d_async", "ks265_memcpy_d2h_async", "ks265_memcpy_d2d_async", "ks265_copy_out_async", "ks265_memset_async",
    "ks265_event_create", "ks265_event_record", "ks265_event_wait", "ks265_event_query", "ks265_stream_wait_event", "ks265_event_destroy",
    "ks265_sad_batch", "ks265_sad4_batch", "ks265_sad3_batch", "ks265_sad4blk_8x8_batch", "ks265_sse_batch", "ks265_had_batch",
    "ks265_residual_batch", "ks265_fwd_transform_batch", "ks265_quant_batch", "ks265_sign_hiding_batch", "ks265_rdoq_batch", "ks265_dequant_batch", "ks265_dequant_rect_batch", "ks265_inv_transform_batch",
    "ks265_edge_filter_luma_batch", "ks265_edge_filter_chroma_batch", "ks265_interp_rect",
    "ks265_sao_apply_bo_rect", "ks265_sao_apply_eo_rect", "ks265_sao_stats_batch", "ks265_intra_pred_batch", "ks265_intra_filter_ref_batch",
    "ks265_downsample_rect", "ks265_downsample_from_host", "ks265_weight_bi_sad_batch", "ks265_ac_energy_batch", "ks265_ac_energy_map",
    "ks265_frame_reset_prediction", "ks265_frame_records_layout", "ks265_frame_pack_records", "ks265_frame_compact_layout", "ks265_frame_pack_compact", "ks265_frame_pack_compact_on", "ks265_frame_adapt_quant", "ks265_aq_ctu_map", "ks265_cutree_propagate", "ks265_calc_frame_cost", "ks265_calc_frame_cost_workspace", "ks265_cutree_finish", "ks265_host_register", "ks265_memcpy_h2d_sync", "ks265_host_unregister", "ks265_pad_plane", "ks265_fill_u16", "ks265_qoff_ctu_map", "ks265_frame_set_records_fence", "ks265_load_i420_on", "ks265_sse_picture_on", "ks265_copy_out_compact_async", "ks265_copy_out_compact_dma_async", "ks265_frame_geometry", "ks265_frame_create", "ks265_frame_destroy", "ks265_frame_set_qp", "ks265_frame_set_picture_tools", "ks265_frame_set_picture_skip", "ks265_frame_set_qp_map", "ks265_frame_set_rdoq", "ks265_pad_picture",
    "ks265_load_i420", "ks265_store_i420", "ks265_presearch", "ks265_me_integer", "ks265_me_propagate", "ks265_me_subpel", "ks265_cu_decide_part", "ks265_cu_decide_part_b", "ks265_merge_pass", "ks265_skip_pass", "ks265_cu_decide",
    "ks265_cu_flat_intra", "ks265_intra_decide", "ks265_intra_decide_ex", "ks265_lookahead_reduce", "ks265_lookahead_picture", "ks265_lookahead_inter", "ks265_intra_reconstruct", "ks265_reconstruct", "ks265_reconstruct_b", "ks265_bi_decide", "ks265_bi_refine_chosen", "ks265_bi_full_batch", "ks265_capture_begin", "ks265_capture_end", "ks265_graph_launch", "ks265_graph_destroy", "ks265_frame_p_state", "ks265_frame_p_advance", "ks265_frame_p_restore", "ks265_cu_decide_b", "ks265_deblock", "ks265_sao",
    "ks265_encode_picture", "ks265_encode_picture_b", "ks265_encode_picture_mref", "ks265_encode_picture_b_mref", "ks265_ref_pick", "ks265_ref_decide", "ks265_reconstruct_mref",
    "ks265_intra_candidates", "ks265_cu_decide_ii", "ks265_cu_decide_b_ii", "ks265_intra_inter_reconstruct", "ks265_frame_set_profiling", "ks265_frame_stage_ms", "ks265_frame_me_int_ms", "ks265_frame_levels", "ks265_frame_pu", "ks265_frame_cu8", "ks265_frame_ibest", "ks265_frame_sao", "ks265_sse_picture",
    "ks265_input_validate", "ks265_input_convert", "ks265_wait_external", "ks265_external_wait_event",
    "ks265_output_validate", "ks265_output_convert",
    "ks265_ssim_picture", "ks265_ssim_picture_on",
    "ks265_picture_hash", "ks265_picture_hash_on",
    "ks265_roi_validate", "ks265_roi_reduce", "ks265_roi_ctu_map",
    "ks265_scale_plan_create", "ks265_scale_plan_destroy", "ks265_input_scale_validate", "ks265_input_scale",
    "ks265_analysis_layout", "ks265_analysis_bytes", "ks265_analysis_pack", "ks265_analysis_pack_on", "ks265_analysis_validate", "ks265_analysis_export",
    "ks265_input_pad_validate", "ks265_input_pad", "ks265_output_crop", "ks265_sse_window",
    "ks265_input_denoise_validate", "ks265_input_denoise",
    "ks265_input_enhance_validate", "ks265_input_enhance",
    "ks265_input_hdr_validate", "ks265_input_hdr_work_bytes", "ks265_input_hdr",
    "ks265_input_overlay_validate", "ks265_input_overlay",
    "ks265_tonemap_plan_create", "ks265_tonemap_plan_destroy", "ks265_tonemap_plan_tables", "ks265_input_tonemap_validate", "ks265_input_tonemap",
]


def load_library() -> C.CDLL:
    """Load libks265hip.so; fail loudly if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Ks265Error(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
        _lib = C.CDLL(LIB_PATH)
        _lib.ks265_last_error.restype = C.c_char_p
        _lib.ks265_version.restype = C.c_char_p
        for n in ("ks265_frame_levels", "ks265_frame_pu", "ks265_frame_cu8", "ks265_frame_ibest", "ks265_frame_sao"):
            if hasattr(_lib, n):
                getattr(_lib, n).restype = C.c_void_p
    return _lib


def _p(t) -> C.c_void_p:
    """device pointer of a torch tensor (or None)"""
    return C.c_void_p(0 if t is None else t.data_ptr())


class KsContext:
    """Owns a ks265_ctx bound to torch's current HIP stream on `device` (own_stream: the non-blocking stream ks265_create made stays - a second stream beside torch's,
    ordered against it with events as the encoder host orders its streams)."""

    def __init__(self, device: int = 0, own_stream: bool = False):
        import torch

        self.lib = load_library()
        if not torch.cuda.is_available():
            raise Ks265Error("no HIP device visible: the ks265 pixel path has no CPU fallback")
        self.torch = torch
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        self._chk(self.lib.ks265_create(C.byref(h), C.c_int(device)), None)
        self.h = h
        torch.cuda.set_device(device)
        if not own_stream:
            self._chk(self.lib.ks265_set_stream(self.h, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))

    def _chk(self, rc: int, h="self"):
        if rc != 0:
            msg = self.lib.ks265_last_error(self.h).decode() if h == "self" and getattr(self, "h", None) else ""
            raise Ks265Error(f"ks265 call failed rc={rc} {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.ks265_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def dev(self, arr: np.ndarray):
        """host numpy (any dtype incl. structured) -> device byte-exact tensor of the same dtype family"""
        t = self.torch
        a = np.ascontiguousarray(arr)
        raw = t.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.device)
        return raw

    def zeros(self, nbytes: int):
        return self.torch.zeros(int(nbytes), dtype=self.torch.uint8, device=self.device)

    def host(self, t, dtype, shape=None) -> np.ndarray:
        a = t.cpu().numpy().view(dtype)
        return a.reshape(shape) if shape is not None else a

    def sync(self):
        self._chk(self.lib.ks265_synchronize(self.h))

    def debug_set(self, what: int, value: int):
        self._chk(self.lib.ks265_debug_set(self.h, C.c_int(what), C.c_int(value)))

    def marker(self, ident: int = 0):
        self._chk(self.lib.ks265_marker(self.h, C.c_int(ident)))

    # ---- events and pinned memory (hosts that order several contexts' streams)
    def event_create(self) -> C.c_void_p:
        ev = C.c_void_p()
        self._chk(self.lib.ks265_event_create(self.h, C.byref(ev)))
        return ev

    def event_record(self, ev):
        self._chk(self.lib.ks265_event_record(self.h, ev))

    def stream_wait_event(self, ev):
        """everything enqueued on this context's stream from here on waits for `ev` (recorded on another context's stream)"""
        self._chk(self.lib.ks265_stream_wait_event(self.h, ev))

    def event_destroy(self, ev):
        self._chk(self.lib.ks265_event_destroy(self.h, ev))

    def host_malloc(self, nbytes: int) -> "tuple[C.c_void_p, np.ndarray]":
        """pinned, device-mapped host memory of the library: (pointer for ks265_host_free / the copy-outs, uint8 view of it)"""
        hp = C.c_void_p()
        self._chk(self.lib.ks265_host_malloc(self.h, C.byref(hp), C.c_size_t(nbytes)))
        return hp, np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(hp.value))

    def host_free(self, hp):
        self._chk(self.lib.ks265_host_free(self.h, hp))

    # ---- section 2: batched operator tables (names follow the reference tables)
    def _dist(self, fn, a, sa, b, sb, blks: np.ndarray, k: int) -> np.ndarray:
        n = len(blks)
        out = self.zeros(4 * n * k)
        self._chk(fn(self.h, _p(a), C.c_int(sa), _p(b), C.c_int(sb), _p(self.dev(blks)), C.c_int(n), _p(out)))
        return self.host(out, np.uint32, (n, k) if k > 1 else (n,))

    def sad(self, a, sa, b, sb, blks): return self._dist(self.lib.ks265_sad_batch, a, sa, b, sb, blks, 1)
    def sse(self, a, sa, b, sb, blks): return self._dist(self.lib.ks265_sse_batch, a, sa, b, sb, blks, 1)
    def had(self, a, sa, b, sb, blks): return self._dist(self.lib.ks265_had_batch, a, sa, b, sb, blks, 1)
    def sad4(self, a, sa, b, sb, blks): return self._dist(self.lib.ks265_sad4_batch, a, sa, b, sb, blks, 4)
    def sad3(self, a, sa, b, sb, blks): return self._dist(self.lib.ks265_sad3_batch, a, sa, b, sb, blks, 3)
    def sad4blk_8x8(self, a, sa, b, sb, blks): return self._dist(self.lib.ks265_sad4blk_8x8_batch, a, sa, b, sb, blks, 4)

    def residual(self, org, so, pred, sp, blks: np.ndarray) -> np.ndarray:
        total = int((blks["w"].astype(np.int64) ** 2).sum())
        out = self.zeros(2 * total)
        self._chk(self.lib.ks265_residual_batch(self.h, _p(org), C.c_int(so), _p(pred), C.c_int(sp), _p(self.dev(blks)), C.c_int(len(blks)), _p(out)))
        return self.host(out, np.int16)

    def fwd_transform(self, idx: int, src: np.ndarray) -> np.ndarray:
        nblk = src.shape[0]
        d, out = self.dev(src.astype(np.int16)), self.zeros(src.size * 2)
        self._chk(self.lib.ks265_fwd_transform_batch(self.h, C.c_int(idx), _p(d), _p(out), C.c_int(nblk)))
        return self.host(out, np.int16, src.shape)

    def inv_transform(self, idx: int, coef: np.ndarray, pred: np.ndarray) -> np.ndarray:
        nblk = coef.shape[0]
        dc, dp, out = self.dev(coef.astype(np.int16)), self.dev(pred.astype(np.uint8)), self.zeros(pred.size)
        self._chk(self.lib.ks265_inv_transform_batch(self.h, C.c_int(idx), _p(dc), _p(dp), _p(out), C.c_int(nblk)))
        return self.host(out, np.uint8, pred.shape)

    def quant(self, n: int, coef: np.ndarray, scale: int, off: int, qbits: int):
        nblk = coef.shape[0]
        dc = self.dev(coef.astype(np.int16))
        lvl, du, nz = self.zeros(coef.size * 2), self.zeros(coef.size * 2), self.zeros(4 * nblk)
        self._chk(self.lib.ks265_quant_batch(self.h, C.c_int(n), _p(dc), _p(lvl), _p(du), _p(nz), C.c_int(scale), C.c_int(off), C.c_int(qbits), C.c_int(nblk)))
        return self.host(lvl, np.int16, coef.shape), self.host(du, np.int16, coef.shape), self.host(nz, np.int32)

    def sign_hiding(self, n: int, scan_idx: int, lvl: np.ndarray, coef: np.ndarray, delta_u: np.ndarray) -> np.ndarray:
        dl, dc, du = self.dev(lvl.astype(np.int16)), self.dev(coef.astype(np.int16)), self.dev(delta_u.astype(np.int16))
        self._chk(self.lib.ks265_sign_hiding_batch(self.h, C.c_int(n), C.c_int(scan_idx), _p(dl), _p(dc), _p(du), C.c_int(lvl.shape[0])))
        return self.host(dl, np.int16, lvl.shape)

    def rdoq(self, tus: np.ndarray, lvl: np.ndarray, coef: np.ndarray, tables: np.ndarray, sigmask: np.ndarray):
        """ks265_rdoq_batch (rdoQuant enc@0x4aac50): tus = RDOQ_TU records; lvl / coef flat int16; tables [ntab, 180] int32; sigmask [n, 64] uint16.
        Returns (levels, sigmask, out [n, 2] = (non-zero levels, last scan position), hidden [n])"""
        n = len(tus)
        dl, dc, dt, dm = self.dev(lvl.astype(np.int16)), self.dev(coef.astype(np.int16)), self.dev(np.ascontiguousarray(tables, np.int32)), self.dev(np.ascontiguousarray(sigmask, np.uint16))
        out, hid = self.zeros(8 * n), self.zeros(8 * n)
        self._chk(self.lib.ks265_rdoq_batch(self.h, _p(self.dev(tus)), C.c_int(n), _p(dl), _p(dc), _p(dt), _p(dm), _p(out), _p(hid)))
        return self.host(dl, np.int16), self.host(dm, np.uint16, (n, 64)), self.host(out, np.int32, (n, 2)), self.host(hid, np.uint64)

    def dequant(self, n: int, lvl: np.ndarray, scale: int, add: int, shift: int) -> np.ndarray:
        nblk = lvl.shape[0]
        dl, out = self.dev(lvl.astype(np.int16)), self.zeros(lvl.size * 2)
        self._chk(self.lib.ks265_dequant_batch(self.h, C.c_int(n), _p(dl), _p(out), C.c_int(scale), C.c_int(add), C.c_int(shift), C.c_int(nblk)))
        return self.host(out, np.int16, lvl.shape)

    def dequant_rect(self, n: int, lvl: np.ndarray, coef_init: np.ndarray, scale: int, add: int, shift: int, last_x: int, last_y: int) -> np.ndarray:
        dl, out = self.dev(lvl.astype(np.int16)), self.dev(coef_init.astype(np.int16))
        self._chk(self.lib.ks265_dequant_rect_batch(self.h, C.c_int(n), C.c_int(n), _p(dl), _p(out), C.c_int(scale), C.c_int(add), C.c_int(shift),
                                                    C.c_int(last_x), C.c_int(last_y), C.c_int(lvl.shape[0])))
        return self.host(out, np.int16, lvl.shape)

    def edge_filter(self, plane, stride: int, edges: np.ndarray, chroma: bool = False):
        fn = self.lib.ks265_edge_filter_chroma_batch if chroma else self.lib.ks265_edge_filter_luma_batch
        self._chk(fn(self.h, _p(plane), C.c_int(stride), _p(self.dev(edges)), C.c_int(len(edges))))

    def interp_rect(self, kind: int, dst, ds: int, src, src_byte_off: int, ss: int, w: int, h: int, frac: int):
        self._chk(self.lib.ks265_interp_rect(self.h, C.c_int(kind), _p(dst), C.c_int(ds), C.c_void_p(src.data_ptr() + src_byte_off),
                                             C.c_int(ss), C.c_int(w), C.c_int(h), C.c_int(frac)))

    def sao_apply_bo(self, offsets: np.ndarray, rec, stride: int, h: int, w: int, band: int):
        o = (C.c_int8 * 4)(*[int(x) for x in offsets])
        self._chk(self.lib.ks265_sao_apply_bo_rect(self.h, o, _p(rec), C.c_int(stride), C.c_int(h), C.c_int(w), C.c_int(band)))

    def sao_apply_eo(self, cls: int, offsets: np.ndarray, src, dst, byte_off: int, stride: int, h: int, w: int):
        o = (C.c_int8 * 5)(*[int(x) for x in offsets])
        self._chk(self.lib.ks265_sao_apply_eo_rect(self.h, C.c_int(cls), o, C.c_void_p(src.data_ptr() + byte_off),
                                                   C.c_void_p(dst.data_ptr() + byte_off), C.c_int(stride), C.c_int(h), C.c_int(w)))

    def sao_stats(self, org, os_: int, rec, rs: int, rects: np.ndarray, row_step: int) -> np.ndarray:
        out = self.zeros(4 * 96 * len(rects))
        self._chk(self.lib.ks265_sao_stats_batch(self.h, _p(org), C.c_int(os_), _p(rec), C.c_int(rs), _p(self.dev(rects)), C.c_int(len(rects)),
                                                 C.c_int(row_step), _p(out)))
        return self.host(out, np.int32, (len(rects), 96))

    def downsample(self, src, ss: int, w: int, h: int, ds: int):
        dst = self.zeros(ds * h)
        self._chk(self.lib.ks265_downsample_rect(self.h, _p(src), C.c_int(ss), _p(dst), C.c_int(ds), C.c_int(w), C.c_int(h)))
        return self.host(dst, np.uint8, (h, ds))

    def downsample_from_host(self, src: np.ndarray, ss: int, w: int, h: int, ds: int):
        """the same with the source in pinned host memory of the library (ks265_host_malloc): the kernel reads it over PCIe"""
        hp = C.c_void_p()
        self._chk(self.lib.ks265_host_malloc(self.h, C.byref(hp), C.c_size_t(src.size)))
        try:
            C.memmove(hp, src.ctypes.data, src.size)
            dst = self.zeros(ds * h)
            self._chk(self.lib.ks265_downsample_from_host(self.h, hp, C.c_int(ss), _p(dst), C.c_int(ds), C.c_int(w), C.c_int(h)))
            self.sync()
            return self.host(dst, np.uint8, (h, ds))
        finally:
            self._chk(self.lib.ks265_host_free(self.h, hp))

    def weight_bi_sad(self, org, so: int, r0, s0: int, r1, s1: int, blks: np.ndarray) -> np.ndarray:
        out = self.zeros(4 * len(blks))
        self._chk(self.lib.ks265_weight_bi_sad_batch(self.h, _p(org), C.c_int(so), _p(r0), C.c_int(s0), _p(r1), C.c_int(s1), _p(self.dev(blks)), C.c_int(len(blks)), _p(out)))
        return self.host(out, np.uint32)

    def bi_full(self, use_had: int, org, so: int, ref, sr: int, blks: np.ndarray, mvcost: np.ndarray) -> np.ndarray:
        out = self.zeros(8 * len(blks))
        d_blks, d_mvc = self.dev(blks), self.dev(np.ascontiguousarray(mvcost, np.uint16))      # both alive across the call (a temporary's block would be reused)
        self._chk(self.lib.ks265_bi_full_batch(self.h, C.c_int(int(use_had)), _p(org), C.c_int(so), _p(ref), C.c_int(sr), _p(d_blks), _p(d_mvc), C.c_int(len(blks)), _p(out)))
        return self.host(out, np.uint32, (len(blks), 2))

    def ac_energy(self, src, stride: int, log2: int, offs: np.ndarray) -> np.ndarray:
        out = self.zeros(4 * len(offs))
        self._chk(self.lib.ks265_ac_energy_batch(self.h, _p(src), C.c_int(stride), C.c_int(log2), _p(self.dev(np.asarray(offs, np.int32))), C.c_int(len(offs)), _p(out)))
        return self.host(out, np.uint32)

    def ac_energy_map(self, plane, stride: int, w: int, h: int, log2: int) -> np.ndarray:
        n = (w >> log2) * (h >> log2)
        out = self.zeros(4 * n)
        self._chk(self.lib.ks265_ac_energy_map(self.h, _p(plane), C.c_int(stride), C.c_int(w), C.c_int(h), C.c_int(log2), _p(out)))
        return self.host(out, np.uint32, (h >> log2, w >> log2))

    def frame_adapt_quant(self, y, stride_y: int, u, v, stride_c: int, nx: int, ny: int, strength: float, count: int | None = None):
        """calcFrameAdaptQuant enc@0x4653c0: (QP offsets float64 [ny, nx], inverse qscale factors uint16 [ny, nx]) of a picture's 16x16 blocks; y / u / v: device planes"""
        n = nx * ny
        off, inv, scal = self.zeros(8 * n), self.zeros(2 * n), self.zeros(16)
        self._chk(self.lib.ks265_frame_adapt_quant(self.h, _p(y), C.c_int(stride_y), _p(u), _p(v), C.c_int(stride_c), C.c_int(nx), C.c_int(ny), C.c_int(count or n), C.c_double(strength),
                                                   _p(off), _p(inv), _p(scal)))
        return self.host(off, np.float64, (ny, nx)), self.host(inv, np.uint16, (ny, nx))

    def cutree_propagate(self, lg: int, nx: int, ny: int, intra, invq, own, inter, bits, mv0, mv1, ref0, ref1, acc):
        """cuTreePropagate enc@0x47d460 on device arrays (ref0 / ref1 updated in place; acc: 2 * nx * ny zeroed uint64, left zero)"""
        self._chk(self.lib.ks265_cutree_propagate(self.h, C.c_int(lg), C.c_int(nx), C.c_int(ny), _p(intra), _p(invq), _p(own), _p(inter), _p(bits), _p(mv0), _p(mv1), _p(ref0), _p(ref1), _p(acc)))

    def calc_frame_cost(self, prm: "CfcParams", cur, ref0, ref1, arr: dict, sums: np.ndarray):
        """calcFrameCost enc@0x4a7410 on device data.  cur / ref0 / ref1: (tensor, byte offset of sample (0, 0)) or None; arr: device tensors intra (u16), imode (u8), invq (u16),
        inter (u16), bits (u8), mv0 / c0 / mv1 / c1 (i32) - updated in place; sums: 11 int32 (ks265_cfc_sums) in, the updated words out"""
        at = lambda t: C.c_void_p(t[0].data_ptr() + int(t[1])) if t is not None else None
        self.lib.ks265_calc_frame_cost_workspace.restype = C.c_size_t
        ws = self.zeros(int(self.lib.ks265_calc_frame_cost_workspace(C.c_int(prm.nx), C.c_int(prm.ny))))
        ds = self.dev(np.ascontiguousarray(sums, np.int32))
        g = lambda k: _p(arr[k]) if arr.get(k) is not None else None
        self._chk(self.lib.ks265_calc_frame_cost(self.h, C.byref(prm), at(cur), at(ref0), at(ref1), g("intra"), g("imode"), g("invq"), g("inter"), g("bits"), g("mv0"), g("c0"), g("mv1"), g("c1"),
                                                 _p(ds), _p(ws)))
        return self.host(ds, np.int32)

    def cutree_finish(self, cnt: int, intra, invq, prop, aq_off, dbl: int, out):
        """the cuTree finish (enc@0x480964..0x480a54) on device arrays; out (float64) updated in place"""
        self._chk(self.lib.ks265_cutree_finish(self.h, C.c_int(cnt), _p(intra), _p(invq), _p(prop), _p(aq_off), C.c_int(dbl), _p(out)))

    # ---- ROI quantiser offset maps (include/ks265_hip.h ks265_roi_*)
    def roi_desc(self, m, log2_block: int) -> RoiDesc:
        """descriptor of a 2-D int8 / float32 device tensor with unit column stride (any row stride)"""
        t = self.torch
        if m.dim() != 2 or m.dtype not in (t.int8, t.float32) or (m.shape[1] > 1 and m.stride(1) != 1):
            raise Ks265Error("a ROI map is a 2-D int8 or float32 tensor with unit column stride")
        return RoiDesc(ROI_INT8 if m.dtype == t.int8 else ROI_FLOAT32, log2_block, m.shape[1], m.shape[0], m.data_ptr(), m.stride(0) * m.element_size())

    def roi_validate(self, desc: RoiDesc) -> int:
        """the library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_roi_validate(self.h, C.byref(desc)))

    def roi_reduce(self, m, log2_block: int, width: int, height: int, out=None):
        """one int32 per CTU, the CTU's mean offset in 1/256 QP (device tensor, raster order); out: an int32 device tensor of ceil(width / 64) * ceil(height / 64) words"""
        n = ((width + 63) // 64) * ((height + 63) // 64)
        if out is None:
            out = self.torch.empty(n, dtype=self.torch.int32, device=self.device)
        self._chk(self.lib.ks265_roi_reduce(self.h, C.byref(self.roi_desc(m, log2_block)), C.c_int(width), C.c_int(height), _p(out)))
        return out

    def roi_ctu_map(self, records, base, nx: int, ny: int, blocks_per_ctu_side: int, ctu_cols: int, ctu_rows: int, base_qp: int, lo: int, hi: int) -> np.ndarray:
        """one QP per CTU (int8, raster) from the records (int32 device tensor or None) and the block offsets (float64 device tensor or None)"""
        out = self.zeros(ctu_cols * ctu_rows)
        self._chk(self.lib.ks265_roi_ctu_map(self.h, _p(records) if records is not None else None, _p(base) if base is not None else None, C.c_int(nx), C.c_int(ny),
                                             C.c_int(blocks_per_ctu_side), C.c_int(ctu_cols), C.c_int(ctu_rows), C.c_int(base_qp), C.c_int(lo), C.c_int(hi), _p(out)))
        return self.host(out, np.int8)

    # ---- analysis out (include/ks265_hip.h ks265_analysis_*)
    def analysis_desc(self, width: int, height: int, **fields) -> AnalysisDesc:
        """descriptor of the given device tensors (mv=, ref=, cu=, qp=, sse=; a field left out is not wanted): each of the field's dtype and shape (analysis_shapes), its
        innermost dimension(s) dense, rows and planes at any stride"""
        t = self.torch
        d = AnalysisDesc(width, height)
        shapes = analysis_shapes(width, height)
        for name, x in fields.items():
            if x is None:
                continue
            dt, shape = shapes[name]
            dense = x.stride(-1) == 1 and (name != "mv" or x.stride(-2) == 2)
            if x.dtype != getattr(t, dt) or tuple(x.shape) != shape or not dense:
                raise Ks265Error(f"analysis field {name}: a {dt} tensor of shape {shape} with dense rows")
            es = x.element_size()
            if name == "qp":
                setattr(d, name, AnField(x.data_ptr(), x.stride(0) * es, 0))
            else:
                setattr(d, name, AnField(x.data_ptr(), x.stride(1) * es, x.stride(0) * es))
        return d

    def analysis_validate(self, desc: AnalysisDesc) -> int:
        """the library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_analysis_validate(self.h, C.byref(desc)))

    def analysis_export(self, block, desc: AnalysisDesc) -> None:
        """one launch on the context's stream: the wanted fields of a packed block (KsFrame.analysis_pack) into the descriptor's arrays"""
        self._chk(self.lib.ks265_analysis_export(self.h, _p(block), C.byref(desc)))

    def analysis_tensors(self, block, width: int, height: int, fields=ANALYSIS_FIELDS) -> dict:
        """fresh device tensors of the wanted fields, filled from a packed block on the context's stream"""
        t = self.torch
        out = {n: t.empty(analysis_shapes(width, height)[n][1], dtype=getattr(t, analysis_shapes(width, height)[n][0]), device=self.device) for n in fields}
        self.analysis_export(block, self.analysis_desc(width, height, **out))
        return out

    # ---- device input of another size (include/ks265_hip.h ks265_scale_plan_*, ks265_input_scale)
    def scale_plan(self, src_w: int, src_h: int, dst_w: int, dst_h: int, filter: int = 1) -> C.c_void_p:
        """a plan (the tables in device memory) for src -> dst, filter 0 triangle / 1 Catmull-Rom; scale_plan_destroy frees it"""
        plan = C.c_void_p()
        self._chk(self.lib.ks265_scale_plan_create(self.h, C.c_int(src_w), C.c_int(src_h), C.c_int(dst_w), C.c_int(dst_h), C.c_int(filter), C.byref(plan)))
        return plan

    def scale_plan_destroy(self, plan: C.c_void_p) -> None:
        self._chk(self.lib.ks265_scale_plan_destroy(self.h, plan))

    def input_scale(self, plan: C.c_void_p, desc, dst, scratch=None) -> None:
        """desc: a ks265_in_desc (ctypes structure) of the source at the plan's source size; dst: uint8 device tensor of dst_w * dst_h * 3 / 2 bytes; scratch: for RGB and KS265_IN_YUV sources"""
        self._chk(self.lib.ks265_input_scale(self.h, plan, C.byref(desc), _p(scratch), _p(dst)))

    # ---- the temporal denoiser on the way in (include/ks265_hip.h ks265_input_denoise; tests/denoise_ref.py is its specification)
    def input_denoise_validate(self, thr: int, weight: int, width: int, height: int) -> int:
        """the library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_input_denoise_validate(self.h, C.byref(DenoiseCfg(thr, weight)), C.c_int(width), C.c_int(height)))

    def input_denoise_rc(self, thr: int, weight: int, width: int, height: int, pic, hist_in, hist_out, blocks=None) -> int:
        """one launch on the context's stream: `pic` (uint8 device tensor, packed I420 of width x height) filtered in place against hist_in (None: no history), the same
        bytes into hist_out; blocks: an int32 device tensor of 2 * ceil(width / 16) * ceil(height / 16) words or None.  The library's return code"""
        ptr = lambda x: C.c_void_p(x) if isinstance(x, int) else _p(x)
        return int(self.lib.ks265_input_denoise(self.h, C.byref(DenoiseCfg(thr, weight)), C.c_int(width), C.c_int(height), ptr(pic), ptr(hist_in), ptr(hist_out), ptr(blocks)))

    def input_denoise(self, thr: int, weight: int, width: int, height: int, pic, hist_in, hist_out, blocks=None) -> None:
        self._chk(self.input_denoise_rc(thr, weight, width, height, pic, hist_in, hist_out, blocks))

    # ---- edge and colour enhancement on the way in (include/ks265_hip.h ks265_input_enhance; tests/enhance_ref.py is its specification)
    def input_enhance_validate(self, cfg, width: int, height: int) -> int:
        """cfg: (edge_gain, edge_core, edge_limit, edge_over, color_gain).  The library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_input_enhance_validate(self.h, C.byref(EnhanceCfg(*cfg)), C.c_int(width), C.c_int(height)))

    def input_enhance_rc(self, cfg, width: int, height: int, luma_src, pic) -> int:
        """one launch on the context's stream: the luma of `pic` (uint8 device tensor, packed I420 of width x height) written from luma_src (a copy of the plane that does not
        overlap pic; None when edge_gain is 0), its chroma mapped in place.  The library's return code"""
        ptr = lambda x: C.c_void_p(x) if isinstance(x, int) else _p(x)
        return int(self.lib.ks265_input_enhance(self.h, C.byref(EnhanceCfg(*cfg)), C.c_int(width), C.c_int(height), ptr(luma_src), ptr(pic)))

    def input_enhance(self, cfg, width: int, height: int, luma_src, pic) -> None:
        self._chk(self.input_enhance_rc(cfg, width, height, luma_src, pic))

    # ---- local contrast on the way in (include/ks265_hip.h ks265_input_hdr; tests/hdr_ref.py is its specification)
    def input_hdr_validate(self, cfg, width: int, height: int) -> int:
        """cfg: (gain, iters, slope, (radius ...)).  The library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_input_hdr_validate(self.h, C.byref(HdrCfg.of(cfg)), C.c_int(width), C.c_int(height)))

    def input_hdr_work_bytes(self, width: int, height: int) -> int:
        self.lib.ks265_input_hdr_work_bytes.restype = C.c_size_t
        return int(self.lib.ks265_input_hdr_work_bytes(C.c_int(width), C.c_int(height)))

    def input_hdr_rc(self, cfg, width: int, height: int, pic, work, work_bytes=None) -> int:
        """2 x iters launches on the context's stream: the luma of `pic` (uint8 device tensor, packed I420 of width x height) filtered in place, `work` (a device tensor of
        input_hdr_work_bytes bytes, or an address) as the passes' buffer.  The library's return code"""
        ptr = lambda x: C.c_void_p(x) if isinstance(x, int) else _p(x)
        if work_bytes is None:
            work_bytes = work.numel() * work.element_size()
        return int(self.lib.ks265_input_hdr(self.h, C.byref(HdrCfg.of(cfg)), C.c_int(width), C.c_int(height), ptr(pic), ptr(work), C.c_size_t(work_bytes)))

    def input_hdr(self, cfg, width: int, height: int, pic, work) -> None:
        self._chk(self.input_hdr_rc(cfg, width, height, pic, work))

    # ---- overlays on the way in (include/ks265_hip.h ks265_input_overlay; tests/overlay_ref.py is its specification)
    @staticmethod
    def overlay_descs(overlays):
        """overlays: a sequence of (fmt, w, h, (R, G, B addresses), alpha address or None, pitch, pixel_step, x, y, opacity, matrix, full_range), everything in bytes; the
        array of ks265_overlay_desc"""
        arr = (OverlayDesc * max(1, len(overlays)))()
        for d, (fmt, w, h, planes, alpha, pitch, step, x, y, opacity, matrix, full_range) in zip(arr, overlays):
            d.rgb = InDesc(int(fmt), int(w), int(h), (C.c_void_p * 3)(*[int(q) for q in planes]), (C.c_int32 * 3)(int(pitch), 0, 0), int(step), int(matrix), int(bool(full_range)))
            d.alpha, d.x, d.y, d.opacity = (int(alpha) if alpha else None), int(x), int(y), int(opacity)
        return arr

    def input_overlay_validate(self, overlays, coded_w: int, coded_h: int, win_w=None, win_h=None, n=None) -> int:
        """The library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_input_overlay_validate(self.h, self.overlay_descs(overlays), C.c_int(len(overlays) if n is None else n), C.c_int(coded_w), C.c_int(coded_h),
                                                         C.c_int(coded_w if win_w is None else win_w), C.c_int(coded_h if win_h is None else win_h)))

    def input_overlay_rc(self, overlays, coded_w: int, coded_h: int, pic, win_w=None, win_h=None, n=None) -> int:
        """one launch on the context's stream: the overlays blended in the order of the sequence onto `pic` (uint8 device tensor or an address, packed I420 of coded_w x
        coded_h), clipped to the window.  The library's return code"""
        ptr = lambda x: C.c_void_p(x) if isinstance(x, int) else _p(x)
        return int(self.lib.ks265_input_overlay(self.h, self.overlay_descs(overlays), C.c_int(len(overlays) if n is None else n), C.c_int(coded_w), C.c_int(coded_h),
                                                C.c_int(coded_w if win_w is None else win_w), C.c_int(coded_h if win_h is None else win_h), ptr(pic)))

    def input_overlay(self, overlays, coded_w: int, coded_h: int, pic, win_w=None, win_h=None) -> None:
        self._chk(self.input_overlay_rc(overlays, coded_w, coded_h, pic, win_w, win_h))

    # ---- tone mapping on the way in (include/ks265_hip.h ks265_input_tonemap; tests/tonemap_ref.py is its specification)
    def tonemap_plan_create_rc(self, curve: int = 0, peak: float = 1000.0, white: float = 203.0, full_range: bool = False, transfer: int = TONEMAP_PQ):
        """(the library's return code, the plan or None): the tables of one configuration in device memory"""
        plan = C.c_void_p()
        rc = int(self.lib.ks265_tonemap_plan_create(self.h, C.byref(TonemapCfg(int(transfer), int(curve), int(full_range), float(peak), float(white))), C.byref(plan)))
        return rc, (plan if rc == 0 else None)

    def tonemap_plan_create(self, curve: int = 0, peak: float = 1000.0, white: float = 203.0, full_range: bool = False):
        rc, plan = self.tonemap_plan_create_rc(curve, peak, white, full_range)
        self._chk(rc)
        return plan

    def tonemap_plan_destroy(self, plan) -> None:
        self._chk(self.lib.ks265_tonemap_plan_destroy(self.h, plan))

    def tonemap_plan_tables(self, plan, where: int) -> None:
        """a measuring aid: the kernel gathers from global memory (0) or from LDS (1, what a new plan does); the bytes are the same"""
        self._chk(self.lib.ks265_tonemap_plan_tables(plan, C.c_int(where)))

    def input_tonemap_validate(self, plan, desc: InDesc) -> int:
        """The library's return code (0, KS265_POINTER -3, KS265_NOTSUPPORTED -4): nothing is enqueued"""
        return int(self.lib.ks265_input_tonemap_validate(self.h, plan, C.byref(desc)))

    def input_tonemap_rc(self, plan, desc: InDesc, dst) -> int:
        """one launch on the context's stream: the HDR10 picture `desc` describes into the packed I420 picture at `dst` (uint8 device tensor or an address)"""
        return int(self.lib.ks265_input_tonemap(self.h, plan, C.byref(desc), C.c_void_p(dst) if isinstance(dst, int) else _p(dst)))

    def input_tonemap(self, plan, desc: InDesc, dst) -> None:
        self._chk(self.input_tonemap_rc(plan, desc, dst))

    def intra_pred(self, ref, dst, blks: np.ndarray):
        """g_IntraPredFunction: predict every described block from dev `ref` into dev `dst` (in place)"""
        self._chk(self.lib.ks265_intra_pred_batch(self.h, _p(ref), _p(dst), _p(self.dev(blks)), C.c_int(len(blks))))

    def intra_filter_ref(self, src, dst, refs: np.ndarray):
        self._chk(self.lib.ks265_intra_filter_ref_batch(self.h, _p(src), _p(dst), _p(self.dev(refs)), C.c_int(len(refs))))


class CfcParams(C.Structure):                 # ks265_cfc_params (include/ks265_hip.h)
    _fields_ = [*[(n, C.c_int32) for n in ("w", "h", "nx", "ny", "cnt", "stride", "d0", "d1", "flag", "slice_type", "merange", "lg", "zero_thr", "fast_intra", "scenecut", "preset", "p8",
                                             "aq", "b_intra", "f3a8", "f36c", "f538", "f3b4")], ("do_list", C.c_int32 * 2), ("intra_done", C.c_int32), ("lambda_tab", C.c_uint16 * 52)]


class DevPic:
    """A padded YUV 4:2:0 picture in HBM (three torch byte tensors)."""

    def __init__(self, ks: "KsContext", geom: FrameGeom):
        self.y, self.u, self.v = ks.zeros(geom.bytes_y), ks.zeros(geom.bytes_c), ks.zeros(geom.bytes_c)

    def c(self) -> Pic:
        return Pic(self.y.data_ptr(), self.u.data_ptr(), self.v.data_ptr())


class KsFrame:
    """Whole-frame stages of include/ks265_hip.h section 3 (one picture size, one stream)."""

    def __init__(self, ks: KsContext, width: int, height: int, qp: int, lambda_q4: int, me_range: int = 64, subme: int = 1,
                 deblock: int = 1, sao: int = 1, me_method: int = 0, bframes: int = 0, refs: int = 1, me_hex_thr: int = 0, sdh: int = 0, pre_search: int = 0, merge: int = 0, bi_refine: int = 0, decimate: int = 0, rdo: int = 0, intra_inter: int = 0, propagate: int = 0,
                 sub_satd: int = 0, sub_thr: int = 24, sub_flat: int = 8, sub_cap: int = 0, sub_cap_step: int = 0, sub_diag_fast: int = 0, part: int = 0, tu_inter: int = 0, skip_rd: int = 0):     # the sub-pel knobs of -preset slow (synth.SUBME_PRESET)
        self.ks, self.lib = ks, ks.lib
        self.cfg = FrameCfg(width, height, qp, lambda_q4, me_range, me_method, subme, deblock, sao, 0, 0, bframes, refs, me_hex_thr, sdh, pre_search, merge, bi_refine, decimate, rdo, intra_inter, propagate, sub_satd, sub_thr, sub_flat, sub_cap, sub_cap_step, sub_diag_fast, part, tu_inter, skip_rd)
        self.geom = FrameGeom()
        ks._chk(self.lib.ks265_frame_geometry(C.byref(self.cfg), C.byref(self.geom)))
        h = C.c_void_p()
        ks._chk(self.lib.ks265_frame_create(ks.h, C.byref(self.cfg), C.byref(h)))
        self.h = h
        self.width, self.height = width, height
        self.nctu = self.geom.ctu_cols * self.geom.ctu_rows

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ks265_frame_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_pic(self) -> DevPic:
        return DevPic(self.ks, self.geom)

    def set_qp(self, qp: int, lambda_q4: int):
        self.cfg.qp, self.cfg.lambda_q4 = qp, lambda_q4
        self.ks._chk(self.lib.ks265_frame_set_qp(self.h, C.c_int(qp), C.c_int(lambda_q4)))

    def set_picture_tools(self, intra_inter: int = -1, bi_refine: int = -1, sao: int = -1, me_method: int = -1):
        """tools of the pictures coded from here on (-1 = as created, else 0 or the created value; a frame made with sao=3 also takes sao=2): ks265_frame_set_picture_tools"""
        self.ks._chk(self.lib.ks265_frame_set_picture_tools(self.h, C.c_int(intra_inter), C.c_int(bi_refine), C.c_int(sao), C.c_int(me_method)))

    def set_picture_skip(self, skip_rd: int = -1):
        """the skip pass of the pictures coded from here on (-1 = as created, else 0 .. the created skip_rd): ks265_frame_set_picture_skip"""
        self.ks._chk(self.lib.ks265_frame_set_picture_skip(self.h, C.c_int(skip_rd)))

    def set_qp_map(self, dev_map):
        """one QP per CTU (device int8 array, raster; None = off) for the pictures coded from here on; the caller keeps the array alive"""
        self._qp_map = dev_map
        self.ks._chk(self.lib.ks265_frame_set_qp_map(self.h, _p(dev_map) if dev_map is not None else None))

    def set_rdoq(self, tables: "np.ndarray | None", lam: "np.ndarray | None" = None, lam_sdh: "np.ndarray | None" = None):
        """cfg.rdoq (-rdoq 1): the reference's rdoQuant for the luma transform blocks of inter CUs from the next picture on - tables int32 [4][2][180] (estBitRdoq), the two lambdas
        int64 [52] by QP; None = back to the default seam.  The copies are enqueued: the arrays are kept alive here"""
        if tables is None:
            self.ks._chk(self.lib.ks265_frame_set_rdoq(self.h, None, None, None)); return
        self._rq = (np.ascontiguousarray(tables, np.int32), np.ascontiguousarray(lam, np.int64), np.ascontiguousarray(lam_sdh if lam_sdh is not None else lam, np.int64))
        assert self._rq[0].size == 1440 and self._rq[1].size == 52 and self._rq[2].size == 52
        self.ks._chk(self.lib.ks265_frame_set_rdoq(self.h, *(a.ctypes.data_as(C.c_void_p) for a in self._rq)))
        self.ks.sync()

    def load_i420(self, dev_i420, pic: DevPic):
        self.ks._chk(self.lib.ks265_load_i420(self.h, _p(dev_i420), pic.c()))

    def store_i420(self, pic: DevPic):
        out = self.ks.zeros(self.width * self.height * 3 // 2)
        self.ks._chk(self.lib.ks265_store_i420(self.h, pic.c(), _p(out)))
        return out

    def pad(self, pic: DevPic):
        self.ks._chk(self.lib.ks265_pad_picture(self.h, pic.c()))

    def presearch(self, src: DevPic, ref: DevPic) -> np.ndarray:
        """stage A0: the pre-search vector field, [ceil(H/16), ceil(W/16), 2] int16 (integer pel), and the CTUs' window offsets [rows, cols, 2]"""
        nbx, nby = (self.cfg.width + 15) // 16, (self.cfg.height + 15) // 16
        out, off = self.ks.zeros(nbx * nby * 4), self.ks.zeros(self.geom.ctu_cols * self.geom.ctu_rows * 4)
        self.ks._chk(self.lib.ks265_presearch(self.h, src.c(), ref.c(), _p(out), _p(off)))
        return self.ks.host(out, np.int16, (nby, nbx, 2)), self.ks.host(off, np.int16, (self.geom.ctu_rows, self.geom.ctu_cols, 2))

    def me_integer(self, src: DevPic, ref: DevPic, prev_pu, pu):
        self.ks._chk(self.lib.ks265_me_integer(self.h, src.c(), ref.c(), _p(prev_pu), _p(pu)))

    def me_propagate(self, src: DevPic, ref: DevPic, pu_in, pu_out):
        self.ks._chk(self.lib.ks265_me_propagate(self.h, src.c(), ref.c(), _p(pu_in), _p(pu_out)))

    def me_subpel(self, src: DevPic, ref: DevPic, pu):
        self.ks._chk(self.lib.ks265_me_subpel(self.h, src.c(), ref.c(), _p(pu)))

    def intra_decide(self, src: DevPic, cu8):
        self.ks._chk(self.lib.ks265_intra_decide(self.h, src.c(), _p(cu8)))

    def lookahead_picture(self, cur: DevPic, ref: DevPic) -> np.ndarray:
        """low-resolution frame cost: returns [sum intra, sum inter, sum min, blocks | intra-cheaper << 32] (this frame object = half size)"""
        nctu = self.geom.ctu_cols * self.geom.ctu_rows
        ws, out = self.ks.zeros(4 * 85 * nctu), self.ks.zeros(32)
        self.ks._chk(self.lib.ks265_lookahead_picture(self.h, cur.c(), ref.c(), _p(ws), _p(out)))
        self._la_ws = ws
        return self.ks.host(out, np.uint64)

    def lookahead_inter(self, cur: DevPic, ref: DevPic) -> np.ndarray:
        """cur against another reference, with the intra costs of the lookahead_picture call before (same cur)"""
        out = self.ks.zeros(32)
        self.ks._chk(self.lib.ks265_lookahead_inter(self.h, cur.c(), ref.c(), _p(self._la_ws), _p(out)))
        return self.ks.host(out, np.uint64)

    def intra_reconstruct(self, src: DevPic, cu8, lvl, recon: DevPic):
        self.ks._chk(self.lib.ks265_intra_reconstruct(self.h, src.c(), _p(cu8), _p(lvl[0]), _p(lvl[1]), _p(lvl[2]), recon.c()))

    def cu_decide(self, pu, cu8):
        self.ks._chk(self.lib.ks265_cu_decide(self.h, _p(pu), _p(cu8)))

    def cu_flat_intra(self, cu8):
        self.ks._chk(self.lib.ks265_cu_flat_intra(self.h, _p(cu8)))

    def reconstruct(self, src: DevPic, ref: DevPic, cu8, lvl, recon: DevPic):
        self.ks._chk(self.lib.ks265_reconstruct(self.h, src.c(), ref.c(), _p(cu8), _p(lvl[0]), _p(lvl[1]), _p(lvl[2]), recon.c()))

    def reconstruct_b(self, src: DevPic, ref0: DevPic, ref1: DevPic, cu8, lvl, recon: DevPic):
        self.ks._chk(self.lib.ks265_reconstruct_b(self.h, src.c(), ref0.c(), ref1.c(), _p(cu8), _p(lvl[0]), _p(lvl[1]), _p(lvl[2]), recon.c()))

    def skip_pass(self, src: DevPic, ref0: DevPic, ref1: "DevPic | None", cu8, lvl, recon: DevPic):
        """stage D2 after reconstruct[_b]: cu8 / lvl / recon updated in place (ref1 None: a P picture)"""
        self.ks._chk(self.lib.ks265_skip_pass(self.h, src.c(), ref0.c(), ref1.c() if ref1 is not None else Pic(None, None, None), _p(cu8), _p(lvl[0]), _p(lvl[1]), _p(lvl[2]), recon.c()))

    def bi_decide(self, src: DevPic, ref0: DevPic, ref1: DevPic, pu0, pu1, pub):
        self.ks._chk(self.lib.ks265_bi_decide(self.h, src.c(), ref0.c(), ref1.c(), _p(pu0), _p(pu1), _p(pub)))

    def bi_refine_chosen(self, src: DevPic, ref0: DevPic, ref1: DevPic, pu0, pu1, pub, cu8):
        self.ks._chk(self.lib.ks265_bi_refine_chosen(self.h, src.c(), ref0.c(), ref1.c(), _p(pu0), _p(pu1), _p(pub), _p(cu8)))

    def cu_decide_b(self, pub, cu8):
        self.ks._chk(self.lib.ks265_cu_decide_b(self.h, _p(pub), _p(cu8)))

    # ---- the decision stages of the encoder's tool set, one call each (stage tests; ks265_encode_picture* runs them itself)
    def intra_candidates(self, src: DevPic, records, best):
        """records: the picture's ks265_pu or ks265_pu_b records (the gate reads their costs); best: nctu x 85 uint32, cost << 6 | mode, all ones = no candidate"""
        self.ks._chk(self.lib.ks265_intra_candidates(self.h, src.c(), _p(records), _p(best)))

    def cu_decide_ii(self, pu, ibest, cu8):
        self.ks._chk(self.lib.ks265_cu_decide_ii(self.h, _p(pu), _p(ibest), _p(cu8)))

    def cu_decide_b_ii(self, pub, ibest, cu8):
        self.ks._chk(self.lib.ks265_cu_decide_b_ii(self.h, _p(pub), _p(ibest), _p(cu8)))

    def cu_decide_part(self, src: DevPic, ref: DevPic, pu, ibest, cu8):
        """needs KsFrame(part=1)"""
        self.ks._chk(self.lib.ks265_cu_decide_part(self.h, src.c(), ref.c(), _p(pu), _p(ibest), _p(cu8)))

    def cu_decide_part_b(self, src: DevPic, ref0: DevPic, ref1: DevPic, pu0, pu1, pub, ibest, cu8):
        self.ks._chk(self.lib.ks265_cu_decide_part_b(self.h, src.c(), ref0.c(), ref1.c(), _p(pu0), _p(pu1), _p(pub), _p(ibest), _p(cu8)))

    def merge_pass(self, src: DevPic, ref0: DevPic, ref1: "DevPic | None", pu, pub, cu_in, cu_out):
        """stage C2: pu for a P picture (ref1 None), pub for a B picture (the other None); cu_in and cu_out differ"""
        self.ks._chk(self.lib.ks265_merge_pass(self.h, src.c(), ref0.c(), ref1.c() if ref1 is not None else Pic(None, None, None), _p(pu), _p(pub), _p(cu_in), _p(cu_out)))

    def intra_inter_reconstruct(self, src: DevPic, cu8, lvl, recon: DevPic):
        """the intra CUs of a P / B picture, after reconstruct[_b / _mref] (and the skip pass): cu8 / lvl / recon updated in place"""
        self.ks._chk(self.lib.ks265_intra_inter_reconstruct(self.h, src.c(), _p(cu8), _p(lvl[0]), _p(lvl[1]), _p(lvl[2]), recon.c()))

    def ref_pick(self, pus: list, out, idx):
        """one list's per-PU choice: out (may be pus[0]) = the winner's record with the index bits in its cost, idx = its picture, one byte per record"""
        arr = (C.c_void_p * len(pus))(*[p.data_ptr() for p in pus])
        self.ks._chk(self.lib.ks265_ref_pick(self.h, C.c_int(len(pus)), arr, _p(out), _p(idx)))

    def intra_decide_ex(self, src: DevPic, cu8, cost):
        """ks265_intra_decide with the pre-selection costs (nctu x 85 uint32, PU indexing; None = not wanted)"""
        self.ks._chk(self.lib.ks265_intra_decide_ex(self.h, src.c(), _p(cu8), _p(cost)))

    def lookahead_reduce(self, intra_cost, pu) -> np.ndarray:
        """[sum intra, sum inter, sum min, blocks | intra-cheaper << 32] over the 8x8 blocks (intra_cost None: the search's sums alone)"""
        out = self.ks.zeros(32)
        self.ks._chk(self.lib.ks265_lookahead_reduce(self.h, _p(intra_cost), _p(pu), _p(out)))
        return self.ks.host(out, np.uint64)

    def encode_picture_mref(self, src: DevPic, refs: list, out: DevPic):
        """P picture searching len(refs) list-0 pictures (nearest first); needs KsFrame(refs >= len(refs))"""
        arr = (Pic * len(refs))(*[r.c() for r in refs])
        self.ks._chk(self.lib.ks265_encode_picture_mref(self.h, src.c(), arr, C.c_int(len(refs)), out.c()))

    def encode_picture_b_mref(self, src: DevPic, refs0: list, refs1: list, out: DevPic):
        """B picture with several pictures per list (refs0: before it, nearest first; refs1: after it, nearest first); needs KsFrame(refs >= both lengths, bframes > 0)"""
        a0, a1 = (Pic * len(refs0))(*[r.c() for r in refs0]), (Pic * len(refs1))(*[r.c() for r in refs1])
        self.ks._chk(self.lib.ks265_encode_picture_b_mref(self.h, src.c(), a0, C.c_int(len(refs0)), a1, C.c_int(len(refs1)), out.c()))

    def ref_decide(self, pus: list, pub):
        arr = (C.c_void_p * len(pus))(*[p.data_ptr() for p in pus])
        self.ks._chk(self.lib.ks265_ref_decide(self.h, C.c_int(len(pus)), arr, _p(pub)))

    def reconstruct_mref(self, src: DevPic, refs: list, cu8, lvl, recon: DevPic):
        ra = (Pic * len(refs))(*[r.c() for r in refs])
        self.ks._chk(self.lib.ks265_reconstruct_mref(self.h, src.c(), C.c_int(len(refs)), ra, _p(cu8), _p(lvl[0]), _p(lvl[1]), _p(lvl[2]), recon.c()))

    def encode_picture_b(self, src: DevPic, ref0: DevPic, ref1: DevPic, recon_out: DevPic):
        self.ks._chk(self.lib.ks265_encode_picture_b(self.h, src.c(), ref0.c(), ref1.c(), recon_out.c()))

    def deblock(self, cu8, recon: DevPic):
        self.ks._chk(self.lib.ks265_deblock(self.h, _p(cu8), recon.c()))

    def sao(self, src: DevPic, deb: DevPic, sao, dst: DevPic):
        self.ks._chk(self.lib.ks265_sao(self.h, src.c(), deb.c(), _p(sao), dst.c()))

    def encode_picture(self, src: DevPic, ref: DevPic, is_key: bool, recon_out: DevPic):
        self.ks._chk(self.lib.ks265_encode_picture(self.h, src.c(), ref.c(), C.c_int(1 if is_key else 0), recon_out.c()))

    STAGES = ("me_integer", "me_subpel", "intra_candidates", "cu_decide", "reconstruct", "intra_pass", "deblock", "sao")

    def set_profiling(self, on: bool):
        self.ks._chk(self.lib.ks265_frame_set_profiling(self.h, C.c_int(1 if on else 0)))

    def me_int_ms(self) -> float:
        """duration of the last me_int_kernel launch alone (profiling on)"""
        v = C.c_float(-1.0)
        self.ks._chk(self.lib.ks265_frame_me_int_ms(self.h, C.byref(v)))
        return float(v.value)

    def stage_ms(self) -> dict:
        ms = (C.c_float * 8)()
        self.ks._chk(self.lib.ks265_frame_stage_ms(self.h, ms))
        return {n: float(ms[i]) for i, n in enumerate(self.STAGES)}

    def sse_picture(self, a: DevPic, b: DevPic) -> np.ndarray:
        out = self.ks.zeros(24)
        self.ks._chk(self.lib.ks265_sse_picture(self.h, a.c(), b.c(), _p(out)))
        return self.ks.host(out, np.uint64)

    def ssim_picture(self, a: DevPic, b: DevPic, with_sse: bool = True):
        """(sse[3] uint64 or None, ssim[3] int64): per plane the SSE and the sum over the plane's whole 8x8 windows of llrint(ssim * 2^30), from one launch"""
        sse = self.ks.zeros(24) if with_sse else None
        out = self.ks.zeros(24)
        self.ks._chk(self.lib.ks265_ssim_picture(self.h, a.c(), b.c(), _p(sse), _p(out)))
        return (self.ks.host(sse, np.uint64) if with_sse else None), self.ks.host(out, np.int64)

    def analysis_bytes(self) -> int:
        self.lib.ks265_analysis_bytes.restype = C.c_size_t
        return int(self.lib.ks265_analysis_bytes(self.h))

    def analysis_layout(self) -> list:
        """byte offsets of the packed block's mv, ref, cu, sse and qp segments, then its size"""
        off = (C.c_size_t * 6)()
        self.ks._chk(self.lib.ks265_analysis_layout(C.c_int(self.width), C.c_int(self.height), off))
        return [int(x) for x in off]

    def analysis_pack(self, src: DevPic, recon: DevPic, picture_qp: int, deltas=((0, 0, 0, 0), (0, 0, 0, 0)), qp_map=None, cu8=None, block=None, on: "KsContext | None" = None):
        """one launch: the packed analysis block of the picture whose CU map is cu8 (device tensor; None = the frame's own) - deltas[L][i] = POC delta of list L's picture i,
        qp_map = int8 device tensor of one QP per CTU or None; returns the block (a uint8 device tensor of analysis_bytes())"""
        if block is None:
            block = self.ks.torch.empty(self.analysis_bytes(), dtype=self.ks.torch.uint8, device=self.ks.device)
        d = (C.c_int8 * 4 * 2)(*[(C.c_int8 * 4)(*[int(x) for x in row]) for row in deltas])
        args = (src.c(), recon.c(), _p(cu8), _p(qp_map), C.c_int(picture_qp), d, _p(block))
        if on is None:
            self.ks._chk(self.lib.ks265_analysis_pack(self.h, *args))
        else:
            on._chk(self.lib.ks265_analysis_pack_on(on.h, self.h, *args))
        return block

    def picture_hash(self, p: DevPic, on: "KsContext | None" = None):
        """uint32[6]: picture_crc of Y, Cb, Cr, then picture_checksum of Y, Cb, Cr (H.265 D.3.19) of the picture inside its padding, from one launch (on: another context's stream)"""
        out = self.ks.zeros(24)
        if on is None:
            self.ks._chk(self.lib.ks265_picture_hash(self.h, p.c(), _p(out)))
        else:
            self.ks._chk(self.lib.ks265_picture_hash_on(on.h, self.h, p.c(), _p(out)))
            on.sync()
        return self.ks.host(out, np.uint32)

    # internal workspace views (device pointers wrapped as ctypes addresses)
    def ws_ptr(self, name: str, comp: int = 0) -> int:
        fn = getattr(self.lib, "ks265_frame_" + name)
        return fn(self.h, C.c_int(comp)) if name == "levels" else fn(self.h)

    def ws_write(self, name: str, data: np.ndarray, comp: int = 0, offset: int = 0):
        """put the bytes of `data` into an internal workspace buffer, `offset` bytes from its start (ks265_memcpy_h2d_sync: on the device when the call returns)"""
        a = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        self.ks.sync()
        self.ks._chk(self.lib.ks265_memcpy_h2d_sync(self.ks.h, C.c_void_p(self.ws_ptr(name, comp) + int(offset)), C.c_void_p(a.ctypes.data), C.c_size_t(a.size)))

    # ---- the picture's records as one block (include/ks265_hip.h: ks265_frame_records_layout, ks265_frame_compact_layout)
    def records_layout(self) -> list:
        off = (C.c_size_t * 7)()
        self.ks._chk(self.lib.ks265_frame_records_layout(self.h, off))
        return [int(x) for x in off]

    def compact_layout(self) -> list:
        off = (C.c_size_t * 8)()
        self.ks._chk(self.lib.ks265_frame_compact_layout(self.h, off))
        return [int(x) for x in off]

    def pack_records(self, dst, extra64=None):
        """dst: device byte tensor of records_layout()[6] bytes; extra64: device tensor of 64 bytes or None"""
        self.ks._chk(self.lib.ks265_frame_pack_records(self.h, _p(dst), _p(extra64) if extra64 is not None else None))

    def pack_compact(self, dst, extra64=None, on: "KsContext | None" = None):
        """dst: device byte tensor of compact_layout()[7] bytes whose header was zero when it was allocated; on: another context's stream (the caller orders it)"""
        ex = _p(extra64) if extra64 is not None else None
        if on is None:
            self.ks._chk(self.lib.ks265_frame_pack_compact(self.h, _p(dst), ex))
        else:
            on._chk(self.lib.ks265_frame_pack_compact_on(on.h, self.h, _p(dst), ex))

    def copy_out_compact(self, ctx: KsContext, pinned, block, data_bytes: "int | None" = None):
        """a compact block to pinned memory (KsContext.host_malloc) on ctx's stream: by the copy kernel alone, or (data_bytes given) the copy engine for the fixed part and
        the first data_bytes of the data area + the kernel for what lies beyond"""
        if data_bytes is None:
            ctx._chk(self.lib.ks265_copy_out_compact_async(ctx.h, self.h, pinned, _p(block)))
        else:
            ctx._chk(self.lib.ks265_copy_out_compact_dma_async(ctx.h, self.h, pinned, _p(block), C.c_size_t(int(data_bytes))))

    def ws_read(self, name: str, nbytes: int, comp: int = 0) -> np.ndarray:
        """copy `nbytes` of an internal workspace buffer to the host"""
        t = self.ks.torch
        out = t.empty(nbytes, dtype=t.uint8, device=self.ks.device)
        src = self.ws_ptr(name, comp)
        hip = C.CDLL("libamdhip64.so")
        self.ks.sync()
        rc = hip.hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(src), C.c_size_t(nbytes), C.c_int(3))  # device to device
        if rc != 0:
            raise Ks265Error(f"hipMemcpy rc={rc}")
        return out.cpu().numpy()
