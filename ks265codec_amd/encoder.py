"""Encoder for torch users: pictures that are GPU tensors already go into the encoder without leaving the device (include/ks265_enc.h ks265_enc_encode_device_frame).

    enc = Encoder(3840, 2160, preset="slow", qp=27, iper=128)
    for frame in frames:                          # CUDA/HIP tensors: (H, W, 3 / 4) RGB(A) / BGR(A) or (3, H, W) planar RGB as uint8, or as float16 / bfloat16 /
        out += enc.encode(frame, format="rgba")   # float32 with values in [0, 1]; (H * 3 / 2, W) I420 / NV12 as uint8
    out += enc.flush()
    enc.close()

A float tensor is read where it lies, once, by one kernel (KS265_IN_RGB_F16 / _BF16 / _F32 of include/ks265_enc.h; tests/yuv_float_ref.py is the specification): [0, 1] is the
full 8-bit range, values outside are clamped, NaN counts 0.  A float32 picture u8 / 255 writes the stream of the uint8 picture u8; the 16-bit types land within one code of it.

YUV of more bits or more chroma (KS265_IN_YUV of include/ks265_enc.h; tests/yuv_hibit_ref.py is the specification) goes in as its planes, each a 2-D tensor with its own row
stride: enc.encode((y, uv), "nv12", depth=10) is a decoder's P010 surface, (y, u, v) with "i420" | "i422" | "i444", (y, uv) with "nv12" | "nv16" | "nv24", one (H, 2W) tensor with
"yuyv" | "uyvy"; uint8 planes are 8-bit, int16 / uint16 planes need depth=9..16 and msb= (the sample in the top bits of its word: the default for semi-planar and packed; in the
low bits: the default for planar).  One kernel reads the picture once: luma rounded to 8 bits, chroma filtered at full depth and rounded once, no dither, the range passes through.

The encoder reads each tensor in the order of torch's current stream and makes that stream wait until it has: the caller may overwrite the tensor with further work on the
same stream as soon as encode() returns, with no host synchronisation.  Parameters are QY265ConfigParse names (qp, crf, rc, iper, bframes, lookahead, latency, ...);
gpb=0|1 is the process default of that name (ks265_enc_set_default: anchors that search two or more past anchors as B slices over them), set before this handle opens.
hash=2|3 writes a decoded picture hash SEI message (CRC / checksum, computed on the device) behind every picture of THIS handle; the bytes come out of encode() / flush() with the
picture's.

recon="rgb"|"bgr"|"rgba"|"bgra"|"rgb_planar"|"nv12"|"i420" (with recon_matrix=, recon_full_range=) keeps the reconstruction of every picture of THIS handle fetchable on the
device (`devrecon`, include/ks265_enc.h): after every encode() / flush(), enc.recon() returns [(poc, tensor), ...] - the pictures a decoder of the stream will show, as fresh
uint8 tensors in that format, filled in the order of torch's current stream with no host synchronisation.  They must be fetched before the next encode(): the encoder takes
the pictures back then.  recon_dtype=torch.float16|torch.bfloat16|torch.float32 (RGB formats only; default torch.uint8) returns them as float tensors instead: every sample is
the uint8 reconstruction's byte / 255, correctly rounded - recon * 255 is the uint8 picture.

roi=True lets THIS handle take a map of quantiser offsets with every picture (`roi`, include/ks265_enc.h): encode(tensor, format, roi=MAP, roi_block=16) with MAP a 2-D int8 or
float32 array of QP offsets (positive = coarser), one element per roi_block x roi_block luma samples (1, 2, 4 .. 64), ceil(H / roi_block) x ceil(W / roi_block) elements, unit
column stride - a CUDA tensor, read in the order of torch's current stream like the picture (it may be overwritten on that stream as soon as encode() returns), or a NumPy array
in host memory (read before encode() returns).

scale="bicubic"|"bilinear" (with scale_from=(W, H), the largest source; default 8 times the encoder's size, at most 8192 x 8192) lets THIS handle take tensors of other sizes
(`ks265_enc_enable_device_scale`, include/ks265_enc.h): encode() scales them to the encoder's size on the GPU, in the order of torch's current stream like any other picture -
Catmull-Rom or a triangle, both widened when shrinking, exact integer arithmetic (tests/yuv_scale_ref.py is the specification).  Source width a multiple of 8, height even, each
ratio at most 8 either way.  One tensor may feed a ladder of handles of different sizes in one loop; a roi= map refers to the encoder's size.

analysis=True keeps what the encoder DECIDED about every picture of THIS handle fetchable on the device (`analysis`, include/ks265_enc.h): after every encode() / flush(),
enc.analysis() returns [{"poc", "slice_type", "mv", "ref", "cu", "qp", "sse"}, ...] for the pictures that call handed out, in coding order - fresh tensors filled on torch's
current stream with no host synchronisation: mv int16 (2, H/8, W/8, 2) quarter-sample vectors per list, ref int8 (2, H/8, W/8) display-index deltas (negative = past, 0 = list
unused or intra), cu uint8 (5, H/8, W/8) kind / log2 size / partition / cbf / intra mode, qp int8 (ceil(H/64), ceil(W/64)) the QP each CTU was coded with, sse int32
(3, H/8, W/8) the squared error each 8x8 block was left with.  A block's displacement per picture, in samples: flow = mv / 4 / ref (where ref != 0).

Any EVEN width and height opens (Encoder(854, 480), Encoder(960, 540)): a size that is no multiple of 8 is coded at the next multiple of 8 with a conformance window, the
picture padded on the GPU by replicating its last column and row (tests/picture_window_ref.py is the specification).  On such a handle encode() takes uint8 "i420" and "nv12"
tensors of the SOURCE shape only (every other format, and scale=, raises ValueError); recon() returns W x H pictures in every format and dtype; quality() counts the window;
a roi= map describes the source picture; analysis() describes the CODED picture - ceil(H / 8) x ceil(W / 8) blocks, block errors with the padding in them.

denoise=1|2|3 (gentle, medium, aggressive) and recur=V (the blend weight in 1/32, 0 .. 30) switch on the temporal denoiser of THIS handle (`vpp_denoise` / `vpp_recur_filter`,
include/ks265_enc.h; tests/denoise_ref.py is the specification): every picture, whatever its format, is filtered on the GPU against the previous filtered picture - motion
compensated, per 16x16 block - as the last step on its way in, in the order of torch's current stream.  The encoder, recon(), analysis() and quality() see the filtered
picture: PSNR is against it, not against the tensor handed in.

edge=1|2|3 and color=1|2|3 (gentle, medium, aggressive) switch on the enhancement of THIS handle (`vpp_edge` / `vpp_color`, include/ks265_enc.h; tests/enhance_ref.py is the
specification): an unsharp mask with coring and halo control on the luma and a saturation boost on the chroma, one stateless GPU step behind the denoiser and in front of the
encoder, for every format and for scale= (Encoder(w, h, edge=1) behind a shrinking scale= is the ladder's mild sharpening).  The levels are untuned choices; the encoder,
recon(), analysis() and quality() see the enhanced picture, so PSNR is against it.

hdr=True switches on the local-contrast filter of THIS handle (`vpp_hdr`, include/ks265_enc.h; tests/hdr_ref.py is the specification): the luma's base layer from 2 or 3
iterations of an edge-preserving smoother (the domain transform, exact in integers) and the detail above it amplified - contrast at large scale without halos at strong
edges - as a stateless GPU step between the denoiser and the enhancement, for every format and for scale=.  hdr_strength=S (0 .. 5: the detail's gain), hdr_iter=2|3,
hdr_sigma_s=V (0 .. 100: the spatial scale in samples), hdr_sigma_r=V (0 .. 100: the range scale in per cent of the 8-bit range); one left out or 0 takes the default 1.0 / 3 /
20 / 15.  The defaults are untuned choices; chroma is not touched; PSNR is against the filtered picture.

tonemap="bt2390"|"reinhard"|"clip" makes THIS handle tone-map HDR10 planes (`ks265_enc_enable_tonemap`, include/ks265_enc.h; tests/tonemap_ref.py is the specification):
enc.encode((y, uv), "nv12", depth=10) - a decoder's P010 surface in PQ and BT.2020 - and every other 4:2:0 picture of 10 to 16 bits, "i420" or "nv12", comes out as BT.709 SDR
in limited range from the one kernel that reads it, where it would otherwise only be rounded to 8 bits.  tonemap_peak=1000.0 (100 .. 10000 nits: the light that still fits),
tonemap_white=203.0 (80 .. 1000: the light of SDR white), tonemap_full_range=False (of the source).  The gain is taken on the largest of R, G, B, so hue is preserved; with
scale= the picture is mapped at its own size and scaled as SDR.  Planes of more than 8 bits in 4:2:2 or 4:4:4 raise EncoderError on such a handle: nothing is passed through
unmapped; uint8 planes and RGB tensors go in as before.  HLG is not built.

enc.set_overlay(slot, tensor, x=0, y=0, opacity=1.0, format="rgba") blends a GPU tensor of RGB plus alpha onto every picture from the next encode() on (`ks265_enc_set_overlay`,
include/ks265_enc.h; tests/overlay_ref.py is the specification): a logo, captions, a timestamp, a picture in picture.  Eight slots, later slots on top; x, y even, any sign, in the
encoder's picture, the part outside is clipped.  The tensor is read in place inside every encode(), in the order of torch's stream current at the set call: rewrite it on that
stream as soon as encode() returns and the next picture carries the new caption.  It is blended behind the filters above - they never see it - and in front of everything else:
recon(), analysis() and quality() see the overlaid picture.  enc.set_overlay(slot, None) clears the slot."""
from __future__ import annotations

import ctypes as C
import os

from . import stream as _stream

IN_I420, IN_NV12, IN_RGB = 0, 1, 2
IN_RGB_F16, IN_RGB_BF16, IN_RGB_F32 = 16, 17, 18              # RGB as float samples in [0, 1]; pointers, pixel step and pitch stay in bytes
MATRIX_BT709, MATRIX_BT601 = 0, 1
QY_OK, QY_FAIL, QY_OUTOFMEMORY, QY_POINTER, QY_NOTSUPPORTED = 0, -0x7FFFFFFF, -0x7FFFFFFE, -0x7FFFFFFD, -0x7FFFFFFC
# format name -> (code, byte offsets of R, G, B inside a pixel of an HWC tensor)
_FORMATS = {"i420": (IN_I420, None), "nv12": (IN_NV12, None), "rgb": (IN_RGB, (0, 1, 2)), "bgr": (IN_RGB, (2, 1, 0)),
            "rgba": (IN_RGB, (0, 1, 2)), "bgra": (IN_RGB, (2, 1, 0)), "rgb_planar": (IN_RGB, None)}
# YUV given as its planes: format name -> (layout, subsampling) of KS265_IN_YUV
_YUV_FORMATS = {"i420": (0, 0), "i422": (0, 1), "i444": (0, 2), "nv12": (1, 0), "nv16": (1, 1), "nv24": (1, 2), "yuyv": (2, 1), "uyvy": (3, 1)}
_CONFIG_BYTES = 4096                                          # more than sizeof(QY265EncConfig): the library writes only its own layout


class Nal(C.Structure):
    _fields_ = [("naltype", C.c_int), ("tid", C.c_int), ("iSize", C.c_int), ("pts", C.c_longlong), ("pPayload", C.POINTER(C.c_ubyte))]


class Picture(C.Structure):
    _fields_ = [("iSliceType", C.c_int), ("poc", C.c_int), ("pts", C.c_longlong), ("dts", C.c_longlong), ("yuv", C.c_void_p)]


class DevPicture(C.Structure):
    """ks265_dev_picture of include/ks265_enc.h"""
    _fields_ = [("format", C.c_int), ("device", C.c_int), ("plane", C.c_void_p * 3), ("pitch", C.c_int * 3), ("pixel_step", C.c_int),
                ("matrix", C.c_int), ("full_range", C.c_int), ("stream", C.c_void_p), ("pts", C.c_longlong)]


class AnField(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_int), ("plane", C.c_longlong)]


class DevAnalysis(C.Structure):
    """ks265_dev_analysis of include/ks265_enc.h"""
    _fields_ = [("device", C.c_int), ("stream", C.c_void_p), ("mv", AnField), ("ref", AnField), ("cu", AnField), ("qp", AnField), ("sse", AnField)]


class Overlay(C.Structure):
    """ks265_overlay of include/ks265_enc.h"""
    _fields_ = [("rgb", DevPicture), ("width", C.c_int), ("height", C.c_int), ("alpha", C.c_void_p), ("x", C.c_int), ("y", C.c_int), ("opacity", C.c_int), ("flags", C.c_int)]


OV_FORCED_ONLY, OV_SLOTS = 1, 8
# overlay format name -> (planar, element of R, G, B, alpha or None)
_OVERLAY_FORMATS = {"rgba": (False, 0, 1, 2, 3), "bgra": (False, 2, 1, 0, 3), "rgb": (False, 0, 1, 2, None), "bgr": (False, 2, 1, 0, None),
                    "rgb_planar": (True, 0, 1, 2, None), "rgba_planar": (True, 0, 1, 2, 3)}


class Tonemap(C.Structure):
    """ks265_tonemap of include/ks265_enc.h"""
    _fields_ = [("transfer", C.c_int), ("curve", C.c_int), ("full_range", C.c_int), ("peak_nits", C.c_double), ("white_nits", C.c_double)]


_TONEMAP_CURVES = {"bt2390": 0, "reinhard": 1, "clip": 2}
TONEMAP_PQ = 16                                                # H.273's transfer code of SMPTE ST 2084


class Roi(C.Structure):
    """ks265_roi of include/ks265_enc.h"""
    _fields_ = [("type", C.c_int), ("log2_block", C.c_int), ("device", C.c_int), ("data", C.c_void_p), ("pitch", C.c_int), ("stream", C.c_void_p)]


ROI_INT8, ROI_FLOAT32 = 0, 1
_SCALE_FILTERS = {"bilinear": 0, "bicubic": 1}                 # KS_SCALE_TRIANGLE, KS_SCALE_CATMULL_ROM


class Quality(C.Structure):
    """ks265_enc_quality of include/ks265_enc.h"""
    _fields_ = [("frames", C.c_long), ("have_sse", C.c_int), ("have_ssim", C.c_int), ("sse", C.c_double * 3), ("ssim", C.c_double * 3), ("last_poc", C.c_int),
                ("last_sse", C.c_double * 3), ("last_ssim", C.c_double * 3)]


class EncoderError(RuntimeError):
    def __init__(self, what: str, rc: int):
        super().__init__(f"{what}: 0x{rc & 0xFFFFFFFF:08X}")
        self.rc = rc


_lib = None


def library() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = C.CDLL(_stream.build())
        _lib.QY265EncoderOpen.restype = C.c_void_p
        _lib.QY265EncoderOpen.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        for n in ("QY265EncoderClose", "ks265_enc_enable_device_input", "QY265EncoderDelayedFrames"):
            getattr(_lib, n).argtypes = [C.c_void_p]
        _lib.QY265EncoderEncodeFrame.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Nal)), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
        _lib.ks265_enc_get_quality.argtypes = [C.c_void_p, C.POINTER(Quality)]
        _lib.ks265_enc_encode_device_frame.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Nal)), C.POINTER(C.c_int), C.POINTER(DevPicture), C.c_void_p]
        _lib.ks265_enc_device_recon_pending.argtypes = [C.c_void_p]
        _lib.ks265_enc_get_device_recon.argtypes = [C.c_void_p, C.POINTER(DevPicture), C.c_void_p]
        _lib.ks265_enc_set_next_roi.argtypes = [C.c_void_p, C.POINTER(Roi)]
        _lib.ks265_enc_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(Overlay)]
        _lib.ks265_enc_device_analysis_pending.argtypes = [C.c_void_p]
        _lib.ks265_enc_get_device_analysis.argtypes = [C.c_void_p, C.POINTER(DevAnalysis), C.c_void_p]
        _lib.ks265_enc_enable_device_scale.argtypes = [C.c_void_p, C.c_int, C.c_int]
        _lib.ks265_enc_enable_tonemap.argtypes = [C.c_void_p, C.POINTER(Tonemap)]
        _lib.ks265_enc_encode_device_frame_scaled.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Nal)), C.POINTER(C.c_int), C.POINTER(DevPicture), C.c_int, C.c_int, C.c_int, C.c_void_p]
    return _lib


def _rgb_code(dtype) -> int:
    """the format code of an RGB tensor's dtype"""
    import torch
    return {torch.uint8: IN_RGB, torch.float16: IN_RGB_F16, torch.bfloat16: IN_RGB_BF16, torch.float32: IN_RGB_F32}[dtype]


def _describe_yuv(t, format: str, depth, msb) -> DevPicture:
    """the ks265_dev_picture of a YUV picture given as its planes - (y, u, v), (y, uv), or the one (H, 2W) tensor of a packed format - with KS265_IN_YUV's code"""
    import torch
    layout, sub = _YUV_FORMATS[format]
    planes = [t] if isinstance(t, torch.Tensor) else list(t)
    want = 3 if layout == 0 else 2 if layout == 1 else 1
    if len(planes) != want:
        raise ValueError(f"{format}: {('(y, u, v)', '(y, uv)', 'one (H, 2W) tensor')[min(layout, 2)]}")
    words = (torch.int16,) + ((torch.uint16,) if hasattr(torch, "uint16") else ())
    for x in planes:
        if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dim() != 2 or x.dtype != planes[0].dtype or x.device != planes[0].device or (x.shape[1] > 1 and x.stride(1) != 1):
            raise ValueError(f"{format}: 2-D GPU tensors of one dtype on one device, each with unit column stride")
    if planes[0].dtype == torch.uint8:
        if depth not in (None, 8) or msb:
            raise ValueError(f"{format}: uint8 planes are depth 8 (no msb=)")
        depth, msb = 8, False
    elif planes[0].dtype in words:
        if depth is None or not 9 <= int(depth) <= 16:
            raise ValueError(f"{format}: int16 / uint16 planes need depth=9..16")
        depth, msb = int(depth), (layout != 0) if msb is None else bool(msb)
    else:
        raise ValueError(f"{format}: uint8, int16 or uint16 planes")
    H, W = planes[0].shape[0], planes[0].shape[1] // (2 if layout >= 2 else 1)
    cw, ch = (W if sub == 2 else W // 2), (H // 2 if sub == 0 else H)
    shapes = [(H, W), (ch, cw), (ch, cw)] if layout == 0 else [(H, W), (ch, 2 * cw)] if layout == 1 else [(H, 2 * W)]
    if W % 2 or H % 2 or [tuple(x.shape) for x in planes] != shapes:
        raise ValueError(f"{format}: planes of a {W}x{H} picture are {shapes}")
    es = planes[0].element_size()
    p = DevPicture()
    p.format = (IN_I420, IN_NV12)[layout] if depth == 8 and sub == 0 else 0x1000 | layout << 8 | sub << 6 | int(msb) << 5 | depth
    p.device = planes[0].device.index if planes[0].device.index is not None else torch.cuda.current_device()
    for k, x in enumerate(planes):
        if x.stride(0) < x.shape[1]:
            raise ValueError(f"{format}: a row stride below the row")
        p.plane[k], p.pitch[k] = x.data_ptr(), x.stride(0) * es
    p.stream = torch.cuda.current_stream(planes[0].device).cuda_stream
    return p


def picture_size(t, format: str) -> tuple:
    """(height, width) of the picture describe(t, format) describes"""
    import torch
    if not isinstance(t, torch.Tensor):
        return (t[0].shape[0], t[0].shape[1])
    if format in ("yuyv", "uyvy"):
        return (t.shape[0], t.shape[1] // 2)
    if format in ("i420", "nv12"):
        return (t.shape[0] * 2 // 3, t.shape[1])
    return (t.shape[1], t.shape[2]) if format == "rgb_planar" else (t.shape[0], t.shape[1])


def describe(t, format: str, matrix: int = MATRIX_BT709, full_range: bool = False, depth=None, msb=None) -> DevPicture:
    """the ks265_dev_picture of a GPU tensor (no copy: its storage, its strides): uint8, or for the RGB formats float16 / bfloat16 / float32 in [0, 1]; ValueError for a layout the
    encoder cannot read in place.  YUV beyond 8-bit 4:2:0 (KS265_IN_YUV of include/ks265_enc.h; tests/yuv_hibit_ref.py is the specification) comes as its planes: format "i420" |
    "i422" | "i444" with a sequence (y, u, v), "nv12" | "nv16" | "nv24" with (y, uv), "yuyv" | "uyvy" with one (H, 2W) tensor - 2-D tensors with their own row strides and unit
    column stride, on one device, all read on torch's current stream.  uint8 planes are depth 8; int16 / uint16 planes need depth=9..16 and say with msb= whether the sample is
    the top bits of its word (the default for semi-planar and packed: P010, Y210) or the low bits (the default for planar: yuv420p10le).  The range that goes in comes out."""
    import torch
    if format in _YUV_FORMATS and (not isinstance(t, torch.Tensor) or format not in ("i420", "nv12")):
        return _describe_yuv(t, format, depth, msb)
    if depth is not None or msb is not None:
        raise ValueError("depth= / msb=: for YUV pictures given as their planes")
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.float16, torch.bfloat16, torch.float32) or t.device.type != "cuda":
        raise ValueError("a uint8, float16, bfloat16 or float32 tensor on the GPU")
    if format not in _FORMATS:
        raise ValueError(f"format: one of {sorted(_FORMATS)}")
    code, offs = _FORMATS[format]
    if code != IN_RGB and t.dtype != torch.uint8:
        raise ValueError(f"{format}: a uint8 tensor (float samples are RGB only)")
    p = DevPicture()
    p.format, p.device = _rgb_code(t.dtype) if code == IN_RGB else code, t.device.index if t.device.index is not None else torch.cuda.current_device()
    p.matrix, p.full_range = matrix, int(bool(full_range))
    base, es = t.data_ptr(), t.element_size()                   # strides are in elements, the descriptor in bytes
    if code == IN_RGB and format == "rgb_planar":
        if t.dim() != 3 or t.shape[0] != 3 or t.stride(2) != 1 or t.stride(1) < t.shape[2]:
            raise ValueError("rgb_planar: a (3, H, W) tensor with unit column stride")
        for k in range(3):
            p.plane[k] = base + k * t.stride(0) * es
        p.pitch[0], p.pixel_step = t.stride(1) * es, es
    elif code == IN_RGB:
        n = 4 if format.endswith("a") else 3
        if t.dim() != 3 or t.shape[2] != n or t.stride(2) != 1 or t.stride(1) < n:
            raise ValueError(f"{format}: an (H, W, {n}) tensor with contiguous pixels")
        for k in range(3):
            p.plane[k] = base + offs[k] * es
        p.pitch[0], p.pixel_step = t.stride(0) * es, t.stride(1) * es
    else:                                                       # (H * 3 / 2, W): Y rows, then the chroma rows
        if t.dim() != 2 or t.shape[0] % 3 or t.stride(1) != 1:
            raise ValueError(f"{format}: an (H * 3 / 2, W) tensor with unit column stride")
        H, W, rs = t.shape[0] * 2 // 3, t.shape[1], t.stride(0)
        p.plane[0], p.pitch[0] = base, rs
        if code == IN_NV12:
            p.plane[1], p.pitch[1] = base + H * rs, rs
        else:                                                   # I420 in a 2-D tensor: each chroma row of the tensor holds two rows of U (then of V) of W / 2
            if rs != W:
                raise ValueError("i420: a (H * 3 / 2, W) tensor must be contiguous (its chroma rows hold two plane rows each); pass a padded picture as nv12 or through the C API")
            p.plane[1], p.plane[2] = base + H * W, base + H * W + H * W // 4
            p.pitch[1] = p.pitch[2] = W // 2
    p.stream = torch.cuda.current_stream(t.device).cuda_stream
    return p


def describe_overlay(t, format: str = "rgba", x: int = 0, y: int = 0, opacity: float = 1.0, matrix: int = MATRIX_BT709, full_range: bool = False, forced_only: bool = False) -> Overlay:
    """the ks265_overlay of a GPU tensor (no copy: its storage, its strides; read on torch's current stream): (H, W, 3 | 4) for "rgb" | "bgr" | "rgba" | "bgra" - in a
    four-element pixel without alpha the fourth element is ignored - or (3 | 4, H, W) for "rgb_planar" | "rgba_planar"; uint8, or float16 / bfloat16 / float32 in [0, 1].  One
    row stride and one column stride serve all channels, so a tensor's own strides always do.  opacity 0 .. 1 (in 1/256)"""
    import torch
    if format not in _OVERLAY_FORMATS:
        raise ValueError(f"format: one of {sorted(_OVERLAY_FORMATS)}")
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.float16, torch.bfloat16, torch.float32) or t.device.type != "cuda" or t.dim() != 3:
        raise ValueError("an overlay is a 3-D uint8, float16, bfloat16 or float32 tensor on the GPU")
    planar, r, g, b, a = _OVERLAY_FORMATS[format]
    need = 1 + max(r, g, b, a or 0)
    if planar:
        if t.shape[0] != need:
            raise ValueError(f"{format}: a ({need}, H, W) tensor")
        h, w, row, col, chan = t.shape[1], t.shape[2], t.stride(1), t.stride(2), t.stride(0)
    else:
        if t.shape[2] < need or t.shape[2] > 4:
            raise ValueError(f"{format}: an (H, W, {need}{' | 4' if need == 3 else ''}) tensor")
        h, w, row, col, chan = t.shape[0], t.shape[1], t.stride(0), t.stride(1), t.stride(2)
    if min(row, col, chan) < 1 or row < w * col:
        raise ValueError(f"{format}: positive strides, rows that do not overlap")
    if not 0.0 <= float(opacity) <= 1.0:
        raise ValueError("opacity: 0 .. 1")
    es, base = t.element_size(), t.data_ptr()
    o = Overlay()
    o.rgb.format, o.rgb.device = _rgb_code(t.dtype), t.device.index if t.device.index is not None else torch.cuda.current_device()
    for k, c in enumerate((r, g, b)):
        o.rgb.plane[k] = base + c * chan * es
    o.rgb.pitch[0], o.rgb.pixel_step, o.rgb.matrix, o.rgb.full_range = row * es, col * es, matrix, int(bool(full_range))
    o.rgb.stream = torch.cuda.current_stream(t.device).cuda_stream
    o.width, o.height, o.alpha = w, h, (base + a * chan * es if a is not None else None)
    o.x, o.y, o.opacity, o.flags = int(x), int(y), int(round(float(opacity) * 256)), OV_FORCED_ONLY if forced_only else 0
    return o


def describe_roi(m, block: int = 16) -> Roi:
    """the ks265_roi of a 2-D int8 / float32 map with unit column stride: a GPU tensor (no copy; read on torch's current stream) or a NumPy array in host memory"""
    import numpy as np
    if block not in (1, 2, 4, 8, 16, 32, 64):
        raise ValueError("roi_block: 1, 2, 4, 8, 16, 32 or 64")
    r = Roi()
    r.log2_block = block.bit_length() - 1
    if isinstance(m, np.ndarray):
        if m.ndim != 2 or m.dtype not in (np.int8, np.float32) or (m.shape[1] > 1 and m.strides[1] != m.itemsize) or m.strides[0] < m.shape[1] * m.itemsize:
            raise ValueError("roi: a 2-D int8 or float32 array with unit column stride")
        r.type, r.device, r.data, r.pitch = ROI_INT8 if m.dtype == np.int8 else ROI_FLOAT32, -1, m.ctypes.data, m.strides[0]
        return r
    import torch
    if not isinstance(m, torch.Tensor) or m.device.type != "cuda" or m.dim() != 2 or m.dtype not in (torch.int8, torch.float32) or (m.shape[1] > 1 and m.stride(1) != 1) or m.stride(0) < m.shape[1]:
        raise ValueError("roi: a 2-D int8 or float32 GPU tensor (or NumPy array) with unit column stride")
    r.type, r.device = ROI_INT8 if m.dtype == torch.int8 else ROI_FLOAT32, m.device.index if m.device.index is not None else torch.cuda.current_device()
    r.data, r.pitch, r.stream = m.data_ptr(), m.stride(0) * m.element_size(), torch.cuda.current_stream(m.device).cuda_stream
    return r


class Encoder:
    """one encoder handle with device input enabled; encode() returns the bytes of the NAL units that call produced (the encoder's output lags its input)"""

    def __init__(self, width: int, height: int, preset: str = "slow", **params):
        self.lib, self.width, self.height = library(), width, height
        self._cfg = (C.c_uint8 * _CONFIG_BYTES)()
        if self.lib.QY265ConfigDefaultPreset(self._cfg, preset.encode(), None, str(params.pop("latency", "default")).encode()) != 0:
            raise ValueError(f"preset {preset!r}")
        gpb = params.pop("gpb", None)                           # no QY265EncConfig field: a process default (None leaves it as it is)
        if gpb is not None and self.lib.ks265_enc_set_default(b"gpb", C.c_int(int(gpb))) != 0:
            raise ValueError(f"parameter gpb={gpb!r}: bad value")
        hash_ = params.pop("hash", None)                        # `hash` (ks265_enc.h): for this handle alone - the process default goes back to off once the handle is open
        if hash_ is not None and self.lib.ks265_enc_set_default(b"hash", C.c_int(int(hash_))) != 0:
            raise ValueError(f"parameter hash={hash_!r}: bad value (0, 2 = CRC, 3 = checksum)")
        self._recon = params.pop("recon", None)                 # `devrecon` (ks265_enc.h) for this handle alone, like `hash`; the format recon() fills its tensors in
        self._recon_matrix, self._recon_full = int(params.pop("recon_matrix", MATRIX_BT709)), bool(params.pop("recon_full_range", False))
        self._recon_dtype = params.pop("recon_dtype", None)    # the dtype of recon()'s tensors: None = torch.uint8; float16 / bfloat16 / float32 for the RGB formats
        if self._recon is not None and self._recon not in _FORMATS:
            raise ValueError(f"recon: one of {sorted(_FORMATS)}")
        if self._recon_dtype is not None:
            import torch
            if self._recon_dtype not in (torch.uint8, torch.float16, torch.bfloat16, torch.float32):
                raise ValueError("recon_dtype: torch.uint8, torch.float16, torch.bfloat16 or torch.float32")
            if self._recon_dtype != torch.uint8 and (self._recon is None or _FORMATS[self._recon][0] != IN_RGB):
                raise ValueError("recon_dtype: a float dtype needs an RGB format in recon=")
        if self._recon is not None and self.lib.ks265_enc_set_default(b"devrecon", C.c_int(1)) != 0:
            raise ValueError("parameter recon: the library has no devrecon switch")
        self._roi = bool(params.pop("roi", False))              # `roi` (ks265_enc.h) for this handle alone, like `hash`
        if self._roi and self.lib.ks265_enc_set_default(b"roi", C.c_int(1)) != 0:
            raise ValueError("parameter roi: the library has no roi switch")
        self._analysis = bool(params.pop("analysis", False))    # `analysis` (ks265_enc.h) for this handle alone, like `hash`
        if self._analysis and self.lib.ks265_enc_set_default(b"analysis", C.c_int(1)) != 0:
            raise ValueError("parameter analysis: the library has no analysis switch")
        self._scale = params.pop("scale", None)                 # ks265_enc_enable_device_scale for this handle: the filter encode() scales tensors of other sizes with
        scale_from = params.pop("scale_from", None)
        if self._scale is not None and self._scale not in _SCALE_FILTERS:
            raise ValueError(f"scale: one of {sorted(_SCALE_FILTERS)}")
        if scale_from is not None and self._scale is None:
            raise ValueError("scale_from: needs scale=")
        self._ragged = bool(width % 8 or height % 8)            # coded at the next multiple of 8 with a conformance window (ks265_enc.h)
        tonemap = params.pop("tonemap", None)                   # ks265_enc_enable_tonemap for this handle: HDR10 planes of 10 to 16 bits come out as BT.709 SDR
        tm_peak, tm_white, tm_full = params.pop("tonemap_peak", 1000.0), params.pop("tonemap_white", 203.0), params.pop("tonemap_full_range", False)
        if tonemap is not None and tonemap not in _TONEMAP_CURVES:
            raise ValueError(f"tonemap: one of {sorted(_TONEMAP_CURVES)}")
        if tonemap is None and (tm_peak, tm_white, bool(tm_full)) != (1000.0, 203.0, False):
            raise ValueError("tonemap_peak / tonemap_white / tonemap_full_range: need tonemap=")
        if tonemap is not None and self._ragged:
            raise ValueError(f"tonemap=: a {width}x{height} encoder (no multiple of 8) takes 8-bit i420 and nv12 pictures only")
        if tonemap is not None and not (100.0 <= float(tm_peak) <= 10000.0 and 80.0 <= float(tm_white) <= 1000.0 and float(tm_white) <= float(tm_peak)):
            raise ValueError("tonemap_peak: 100 .. 10000 nits; tonemap_white: 80 .. 1000 nits and at most the peak")
        if self._ragged and self._scale is not None:
            raise ValueError(f"scale=: the scaler writes sizes that are multiples of 8, not {width}x{height}")
        for k, v in (("wdt", width), ("hgt", height), *params.items()):
            rc = self.lib.QY265ConfigParse(self._cfg, str(k).replace("_", "-").encode(), str(int(v) if isinstance(v, bool) else v).encode())   # keyword form of the names with a dash: sao_ref=2 -> "sao-ref"; hdr=True -> "1"
            if rc != 0:
                raise ValueError(f"parameter {k}={v!r}: {'unknown name' if rc == -1 else 'bad value'}")
        err = C.c_int(0)
        self.h = self.lib.QY265EncoderOpen(self._cfg, C.byref(err))
        if hash_ is not None:
            self.lib.ks265_enc_set_default(b"hash", C.c_int(0))
        if self._recon is not None:
            self.lib.ks265_enc_set_default(b"devrecon", C.c_int(0))
        if self._roi:
            self.lib.ks265_enc_set_default(b"roi", C.c_int(0))
        if self._analysis:
            self.lib.ks265_enc_set_default(b"analysis", C.c_int(0))
        if not self.h:
            raise EncoderError("QY265EncoderOpen", err.value)
        rc = self.lib.ks265_enc_enable_device_input(self.h)
        if rc != QY_OK:
            self.lib.QY265EncoderClose(self.h)
            self.h = None
            raise EncoderError("ks265_enc_enable_device_input", rc)
        if self._scale is not None:
            mw, mh = scale_from if scale_from is not None else (min(8192, 8 * width), min(8192, 8 * height))
            rc = self.lib.ks265_enc_enable_device_scale(self.h, int(mw), int(mh))
            if rc != QY_OK:
                self.lib.QY265EncoderClose(self.h)
                self.h = None
                raise EncoderError(f"ks265_enc_enable_device_scale({mw}, {mh})", rc)
        if tonemap is not None:
            rc = self.lib.ks265_enc_enable_tonemap(self.h, C.byref(Tonemap(TONEMAP_PQ, _TONEMAP_CURVES[tonemap], int(bool(tm_full)), float(tm_peak), float(tm_white))))
            if rc != QY_OK:
                self.lib.QY265EncoderClose(self.h)
                self.h = None
                raise EncoderError(f"ks265_enc_enable_tonemap({tonemap}, peak {tm_peak}, white {tm_white}): tone mapping is unavailable on this handle (see the log)", rc)
        self._nal, self._nn, self._out, self._pts = C.POINTER(Nal)(), C.c_int(0), Picture(), 0
        self._flushed, self._held, self._next_display = [], {}, 0  # recon(): what flush() fetched call by call; order="display": early pictures by poc, the next index to return
        if self._recon is not None:                             # refused at open (a device library without the way back, lanes on several GPUs, KS265_GRAPH)?  Nothing is pending: QY_FAIL if on
            probe = DevPicture()
            probe.device = int(os.environ.get("KS265_DEVICE", "0"))
            if self.lib.ks265_enc_get_device_recon(self.h, C.byref(probe), None) == QY_NOTSUPPORTED:
                self.close()
                raise EncoderError("recon=: device reconstruction is unavailable on this handle (see the log)", QY_NOTSUPPORTED)
        self._flushed_an = []                                   # analysis(): what flush() fetched call by call
        self._overlays = {}                                     # set_overlay(): slot -> the tensor, kept alive while the encoder reads it
        if self._analysis:                                      # refused at open?  Nothing is pending: QY_FAIL if the switch is on
            probe = DevAnalysis()
            probe.device = int(os.environ.get("KS265_DEVICE", "0"))
            if self.lib.ks265_enc_get_device_analysis(self.h, C.byref(probe), None) == QY_NOTSUPPORTED:
                self.close()
                raise EncoderError("analysis=: the analysis is unavailable on this handle (see the log)", QY_NOTSUPPORTED)

    def _take(self) -> bytes:
        return b"".join(C.string_at(self._nal[i].pPayload, self._nal[i].iSize) for i in range(self._nn.value) if self._nal[i].iSize > 0)

    def encode(self, tensor, format: str = "rgba", matrix: int = MATRIX_BT709, full_range: bool = False, roi=None, roi_block: int = 16, depth=None, msb=None) -> bytes:
        """one picture in: a tensor, or the planes of a YUV picture with depth= / msb= (describe)"""
        if self.h is None:
            raise RuntimeError("encoder closed")
        pic = describe(tensor, format, matrix, full_range, depth, msb)
        if self._ragged and pic.format not in (IN_I420, IN_NV12):
            raise ValueError(f"format {format!r}: a {self.width}x{self.height} encoder (no multiple of 8) takes 8-bit i420 and nv12 pictures only")
        if roi is not None:
            if not self._roi:
                raise RuntimeError("Encoder(..., roi=True) switches the ROI maps on")
            rd = describe_roi(roi, roi_block)
            b = 1 << rd.log2_block
            if tuple(roi.shape) != ((self.height + b - 1) // b, (self.width + b - 1) // b):
                raise ValueError(f"roi {tuple(roi.shape)}: a {self.width}x{self.height} picture in blocks of {b} is {((self.height + b - 1) // b, (self.width + b - 1) // b)}")
        shape = picture_size(tensor, format)
        if shape != (self.height, self.width) and self._scale is None:
            raise ValueError(f"picture {shape[1]}x{shape[0]}, encoder {self.width}x{self.height}")
        if roi is not None:                                     # (behind every check of the picture: a refused picture leaves nothing pending)
            rc = self.lib.ks265_enc_set_next_roi(self.h, C.byref(rd))
            if rc != QY_OK:
                raise EncoderError("ks265_enc_set_next_roi", rc)
        pic.pts, self._pts = self._pts, self._pts + 1
        scaled = shape != (self.height, self.width)
        if scaled:                                              # scale=: scaled into the input slot on the GPU (a refused size: QY_NOTSUPPORTED, nothing enqueued)
            rc = self.lib.ks265_enc_encode_device_frame_scaled(self.h, C.byref(self._nal), C.byref(self._nn), C.byref(pic), shape[1], shape[0], _SCALE_FILTERS[self._scale],
                                                               C.addressof(self._out))
        else:
            rc = self.lib.ks265_enc_encode_device_frame(self.h, C.byref(self._nal), C.byref(self._nn), C.byref(pic), C.addressof(self._out))
        if rc != QY_OK:
            if roi is not None:
                self.lib.ks265_enc_set_next_roi(self.h, None)       # a picture refused before it was handed in has not taken its map: withdrawn
            raise EncoderError(f"ks265_enc_encode_device_frame_scaled: picture {shape[1]}x{shape[0]}, encoder {self.width}x{self.height}" if scaled else "ks265_enc_encode_device_frame", rc)
        return self._take()

    def set_overlay(self, slot: int, tensor, x: int = 0, y: int = 0, opacity: float = 1.0, format: str = "rgba", matrix: int = MATRIX_BT709, full_range: bool = False,
                    forced_only: bool = False) -> None:
        """slot 0 .. 7 blends `tensor` (describe_overlay) onto every picture from the next encode() on, its top-left corner at (x, y) of the encoder's picture; None clears
        the slot.  The tensor is read in place inside every encode() in the order of torch's stream current NOW: rewrite it there as soon as an encode() has returned.
        forced_only: KS265_OV_FORCED_ONLY - drawn for host pictures handed in with bForceLogo alone, so never for encode()'s tensors.  A refused overlay (ValueError for what
        this module can see, EncoderError for the library's codes) leaves the slot as it was"""
        if self.h is None:
            raise RuntimeError("encoder closed")
        if tensor is None:
            rc = self.lib.ks265_enc_set_overlay(self.h, int(slot), None)
        else:
            rc = self.lib.ks265_enc_set_overlay(self.h, int(slot), C.byref(describe_overlay(tensor, format, x, y, opacity, matrix, full_range, forced_only)))
        if rc != QY_OK:
            raise EncoderError(f"ks265_enc_set_overlay(slot {slot})", rc)
        # (the tensor it replaces may go: every read of it was enqueued inside an encode() that put the tensor's stream behind that read before it returned)
        self._overlays.pop(int(slot), None)
        if tensor is not None:
            self._overlays[int(slot)] = tensor

    def flush(self) -> bytes:
        out = bytearray()
        self._flushed += self._fetch()                          # (what the last encode() handed out and nobody fetched yet: the first flush call takes it back)
        self._flushed_an += self._fetch_analysis()
        while self.h is not None and self.lib.QY265EncoderDelayedFrames(self.h):
            rc = self.lib.QY265EncoderEncodeFrame(self.h, C.byref(self._nal), C.byref(self._nn), None, C.addressof(self._out), 0)
            if rc != QY_OK:
                raise EncoderError("QY265EncoderEncodeFrame (flush)", rc)
            out += self._take()
            self._flushed += self._fetch()                      # every call of the loop takes the previous call's reconstructions back: they are fetched here, for the next recon()
            self._flushed_an += self._fetch_analysis()
        return bytes(out)

    def _fetch(self) -> list:
        """every pending reconstruction (ks265_enc_get_device_recon), oldest first, each into a fresh tensor on torch's current stream"""
        if self._recon is None or self.h is None:
            return []
        import torch
        W, H, out = self.width, self.height, []
        shape = {"rgb": (H, W, 3), "bgr": (H, W, 3), "rgba": (H, W, 4), "bgra": (H, W, 4), "rgb_planar": (3, H, W), "nv12": (H * 3 // 2, W), "i420": (H * 3 // 2, W)}[self._recon]
        info = Picture()
        while self.lib.ks265_enc_device_recon_pending(self.h) > 0:
            t = torch.empty(shape, dtype=self._recon_dtype or torch.uint8, device="cuda")
            rc = self.lib.ks265_enc_get_device_recon(self.h, C.byref(describe(t, self._recon, self._recon_matrix, self._recon_full)), C.addressof(info))
            if rc != QY_OK:
                raise EncoderError("ks265_enc_get_device_recon", rc)
            out.append((info.poc, t))
        return out

    def recon(self, order: str = "coding") -> list:
        """[(poc, tensor), ...]: the reconstructions of the pictures the last encode() / flush() handed out (poc = display index in the stream), in the format of recon=.
        order="coding": as the NAL units came.  order="display": early pictures are kept back - only the run of consecutive display indices that continues what earlier calls
        returned comes out, the rest with later calls (after flush(): everything)."""
        if self._recon is None:
            raise RuntimeError("Encoder(..., recon=FORMAT) switches the reconstructions on")
        if order not in ("coding", "display"):
            raise ValueError('order: "coding" or "display"')
        pics, self._flushed = self._flushed + self._fetch(), []
        if order == "coding":
            return pics
        self._held.update(pics)
        out = []
        while self._next_display in self._held:
            out.append((self._next_display, self._held.pop(self._next_display)))
            self._next_display += 1
        return out

    def _fetch_analysis(self) -> list:
        """every pending analysis (ks265_enc_get_device_analysis), oldest first, each into fresh tensors on torch's current stream"""
        if not self._analysis or self.h is None:
            return []
        import torch
        w8, h8, cc, cr = (self.width + 7) // 8, (self.height + 7) // 8, (self.width + 63) // 64, (self.height + 63) // 64   # (the coded picture's blocks)
        shapes = {"mv": (torch.int16, (2, h8, w8, 2)), "ref": (torch.int8, (2, h8, w8)), "cu": (torch.uint8, (5, h8, w8)), "qp": (torch.int8, (cr, cc)), "sse": (torch.int32, (3, h8, w8))}
        info, out = Picture(), []
        while self.lib.ks265_enc_device_analysis_pending(self.h) > 0:
            a = {n: torch.empty(shape, dtype=dt, device="cuda") for n, (dt, shape) in shapes.items()}
            d = DevAnalysis()
            d.device, d.stream = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream
            for n, t in a.items():
                es = t.element_size()
                setattr(d, n, AnField(t.data_ptr(), t.stride(0) * es, 0) if n == "qp" else AnField(t.data_ptr(), t.stride(1) * es, t.stride(0) * es))
            rc = self.lib.ks265_enc_get_device_analysis(self.h, C.byref(d), C.addressof(info))
            if rc != QY_OK:
                raise EncoderError("ks265_enc_get_device_analysis", rc)
            out.append({"poc": info.poc, "slice_type": info.iSliceType, **a})
        return out

    def analysis(self) -> list:
        """[{"poc", "slice_type", "mv", "ref", "cu", "qp", "sse"}, ...]: what the encoder decided about the pictures the last encode() / flush() handed out, in coding order
        (poc = display index in the stream; slice_type 2 = I, 1 = P, 0 = B); the arrays as the module's header describes them"""
        if not self._analysis:
            raise RuntimeError("Encoder(..., analysis=True) switches the analysis on")
        out, self._flushed_an = self._flushed_an + self._fetch_analysis(), []
        return out

    def quality(self) -> dict:
        """quality figures of the pictures handed out so far (ks265_enc_get_quality): `frames`; `sse` = summed squared error per plane (psnr=1, else None); `ssim` = per plane the
        mean over the pictures of the reference's `-ssim` figure (ssim=1, else None); `last` = display index, SSE and SSIM of the picture accounted last; `psnr` = per plane
        the PSNR over all pictures from those sums (None without psnr=1 or before the first picture; 99.0 for a zero sum, as the encoder's own lines print).  A size that is no
        multiple of 8: SSE and PSNR count the width x height window, SSIM the coded picture"""
        if self.h is None:
            raise RuntimeError("encoder closed")
        q = Quality()
        rc = self.lib.ks265_enc_get_quality(self.h, C.byref(q))
        if rc != QY_OK:
            raise EncoderError("ks265_enc_get_quality", rc)
        n = max(1, q.frames)
        import math
        npx = [self.width * self.height, self.width * self.height // 4, self.width * self.height // 4]
        psnr = [10.0 * math.log10(255.0 * 255.0 * npx[k] * q.frames / q.sse[k]) if q.sse[k] > 0 else 99.0 for k in range(3)] if q.have_sse and q.frames else None
        return {"frames": q.frames, "psnr": psnr, "sse": list(q.sse) if q.have_sse else None, "ssim": [v / n for v in q.ssim] if q.have_ssim else None,
                "last": {"poc": q.last_poc, "sse": list(q.last_sse) if q.have_sse else None, "ssim": list(q.last_ssim) if q.have_ssim else None}}

    def close(self) -> None:
        if self.h is not None:
            self.lib.QY265EncoderClose(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
