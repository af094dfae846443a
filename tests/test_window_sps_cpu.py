"""CPU: the conformance window of ks265_write_sps (ks265_stream_cfg.crop_right / crop_bottom): the three sizes the reference's encoder was run on give its SPS values,
no window gives the bytes the writer always wrote, and anything but 0, 2, 4, 6 is refused."""
from __future__ import annotations

import ctypes as C

import pytest

import ks265codec_amd.stream as S
import picture_window_ref as pw
import window_sps as ws
from slice_headers import nal_units, parse_sps as parse_sps_without_window

KS265_NOTSUPPORTED = -4


class OldStreamCfg(C.Structure):              # ks265_stream_cfg before the window: what a caller compiled against the old header zero-extends to
    _fields_ = [(n, C.c_int32) for n in ("width", "height", "fps_num", "fps_den", "sao", "deblock", "beta_offset_div2", "tc_offset_div2",
                                          "max_dec_pic_buffering", "max_num_reorder", "log2_max_poc_lsb", "sdh", "wpp", "list_mod", "cu_qp_delta", "tu_inter")]


def _cfg(w, h, cr=0, cb=0, **kw):
    c = S.StreamCfg(w, h, 0, 0, 1, 1, 0, 0, 3, 1, 16, 1, 1, 0, 0, 0)
    c.crop_right, c.crop_bottom = cr, cb
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _write(f, cfg) -> "bytes | int":
    out = (C.c_uint8 * 256)()
    n = f(C.byref(cfg), out, C.c_size_t(256))
    return bytes(out[:n]) if n >= 0 else n


@pytest.mark.parametrize("w,h,cw,ch,crop,window", [(854, 480, 856, 480, (2, 0), (0, 1, 0, 0)), (960, 540, 960, 544, (0, 4), (0, 0, 0, 2)),
                                                   (250, 130, 256, 136, (6, 6), (0, 3, 0, 3))])
def test_the_reference_s_windows(w, h, cw, ch, crop, window):
    assert pw.coded_size(w, h) == (cw, ch) and pw.conf_window(w, h) == window
    sps = _write(S.lib().ks265_write_sps, _cfg(cw, ch, *crop))
    (t, rbsp), = list(nal_units(sps))
    assert t == ws.NAL_SPS
    got = ws.parse_sps(rbsp)
    assert (got["width"], got["height"]) == (cw, ch) and got["flag"] == 1 and got["window"] == window
    assert ws.output_size(got) == (w, h)
    assert (got["dpb"], got["reorder"], got["sao"], got["poc_bits"]) == (3, 1, 1, 16)          # what follows the window is read where it is
    # every other NAL unit is that of a configuration without a window
    for f in (S.lib().ks265_write_vps, S.lib().ks265_write_pps):
        assert _write(f, _cfg(cw, ch, *crop)) == _write(f, _cfg(cw, ch))


def test_no_window_is_the_old_sps():
    l = S.lib()
    for w, h in ((856, 480), (416, 240), (64, 64)):
        new = _write(l.ks265_write_sps, _cfg(w, h, 0, 0))
        # the same configuration without the two fields, in front of zeroed memory (a structure of the old layout that a caller zero-initialised)
        raw = (C.c_uint8 * (C.sizeof(OldStreamCfg) + 8))()
        old = OldStreamCfg.from_buffer(raw)
        for n, _ in OldStreamCfg._fields_:
            setattr(old, n, getattr(_cfg(w, h), n))
        out = (C.c_uint8 * 256)()
        n = l.ks265_write_sps(C.byref(old), out, C.c_size_t(256))
        assert n > 0 and bytes(out[:n]) == new
        (t, rbsp), = list(nal_units(new))
        assert parse_sps_without_window(rbsp)["width"] == w                                     # the existing reader (it asserts conformance_window_flag = 0)
        assert ws.parse_sps(rbsp)["flag"] == 0 and ws.parse_sps(rbsp)["window"] == (0, 0, 0, 0)
    # the writer's bytes for this configuration at 416x240, recorded before the fields existed
    assert _write(l.ks265_write_sps, _cfg(416, 240)).hex() == "000000014201010160000003009000000300000300b7a00d080f1636d6493292"
    assert _write(l.ks265_write_sps, _cfg(416, 240, 2, 0)) != _write(l.ks265_write_sps, _cfg(416, 240))


@pytest.mark.parametrize("cr,cb", [(1, 0), (0, 3), (8, 0), (0, 8), (-2, 0), (0, -2), (7, 7), (16, 0), (2, -4), (1 << 30, 0)])
def test_other_crops_are_refused(cr, cb):
    l = S.lib()
    assert _write(l.ks265_write_sps, _cfg(256, 136, cr, cb)) == KS265_NOTSUPPORTED
    assert l.ks265_slice_scratch_bytes(C.byref(_cfg(256, 136, 6, 6))) == l.ks265_slice_scratch_bytes(C.byref(_cfg(256, 136)))


@pytest.mark.parametrize("cr,cb", [(0, 0), (2, 0), (4, 2), (6, 6), (0, 6)])
def test_every_even_crop_below_8_is_written(cr, cb):
    got = ws.parse_sps(next(iter(nal_units(_write(S.lib().ks265_write_sps, _cfg(256, 136, cr, cb)))))[1])
    assert got["window"] == (0, cr // 2, 0, cb // 2) and got["flag"] == int(bool(cr or cb))
