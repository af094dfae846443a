"""CPU: the specification of the decoded picture hash (tests/picture_hash_ref.py) against the standard's loops, and the SEI writer (ks265_write_picture_hash_sei) byte for byte.
  * crc_bitserial is the catalogued CRC-16/SPI-FUJITSU (AUG-CCITT): its published check value pins it;
  * the fast forms equal the loops on planes small enough for the loops, among them one wider and one taller than 256 samples (the masks' `>> 8` terms);
  * the writer: exact bytes, emulation prevention, refusal of every hash_type but 1 and 2; sei_hashes reads back what the writer wrote."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import picture_hash_ref as ph

SHAPES = [(4, 4), (8, 8), (36, 20), (100, 68), (264, 2), (2, 264)]          # (width, height)


def test_published_check_value():
    assert ph.crc_bitserial(b"123456789") == 0xE5CC


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fast_forms_against_the_loops(shape):
    w, h = shape
    p = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    assert ph.crc(p) == ph.crc_bitserial(p)
    assert ph.checksum(p) == ph.checksum_scalar(p)


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_flat_planes(shape, value):
    w, h = shape
    p = np.full((h, w), value, np.uint8)
    assert ph.crc(p) == ph.crc_bitserial(p)
    assert ph.checksum(p) == ph.checksum_scalar(p)


def _one_picture_stream() -> bytes:
    """parameter sets of the writer + the header of an IDR slice (first slice, PPS 0, I, both SAO flags, slice_qp_delta 0), which is all sei_hashes reads of a picture"""
    from ks265codec_amd import stream
    return stream.StreamWriter(64, 64).headers() + bytes.fromhex("00000001" "2601" "afc0")


def _sei(hash_type, values):
    from ks265codec_amd import stream
    return stream.picture_hash_sei(hash_type, values)


def test_writer_exact_bytes():
    assert _sei(1, [0x1234, 0xABCD, 0x00FF]) == bytes.fromhex("00000001" "5001" "84" "07" "01" "1234" "abcd" "00ff" "80")
    assert _sei(2, [0x01020304, 0xA0B0C0D0, 0x55667788]) == bytes.fromhex("00000001" "5001" "84" "0d" "02" "01020304" "a0b0c0d0" "55667788" "80")
    assert _sei(2, [0, 0x300, 1]) == bytes.fromhex("00000001" "5001" "84" "0d" "02" "0000" "03" "0000" "03" "0000" "03" "0300" "00" "03" "0000" "03" "01" "80")


@pytest.mark.parametrize("hash_type", [1, 2])
@pytest.mark.parametrize("values", [[0, 0, 0], [0x300, 0x300, 0x300], [0, 0x300, 0], [0x00010000 >> 8, 0, 0x300]])
def test_values_that_need_emulation_prevention_round_trip(hash_type, values):
    from ks265codec_amd import stream
    nal = _sei(hash_type, values)
    if hash_type == 2:
        assert b"\x00\x00\x03" in nal[4:], "00 00 00 / 00 00 03 inside the payload are escaped"
    assert nal.count(b"\x00\x00\x01") == 1 and b"\x00\x00\x00" not in nal[4:]
    head = _one_picture_stream()
    pics, stripped = ph.sei_hashes(head + nal)
    assert stripped == head and len(pics) == 1 and pics[0]["hashes"] == [(hash_type, values)]
    assert stream.NAL_SUFFIX_SEI == 40


@pytest.mark.parametrize("hash_type", [0, 3, -1, 4])
def test_other_hash_types_are_refused(hash_type):
    from ks265codec_amd import stream
    out, v = (C.c_uint8 * 64)(), (C.c_uint32 * 3)(1, 2, 3)
    assert stream.lib().ks265_write_picture_hash_sei(C.c_int(hash_type), v, out, C.c_size_t(64)) == -4          # KS265_NOTSUPPORTED
    assert bytes(out) == bytes(64)
    with pytest.raises(RuntimeError):
        stream.picture_hash_sei(hash_type, [1, 2, 3])


def test_writer_checks_its_buffer():
    from ks265codec_amd import stream
    out, v = (C.c_uint8 * 64)(), (C.c_uint32 * 3)(0, 0, 0)
    assert stream.lib().ks265_write_picture_hash_sei(C.c_int(2), v, out, C.c_size_t(20)) < 0                    # 22 bytes + 4 escapes do not fit
