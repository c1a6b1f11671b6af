"""Decoding at 1/2, 1/4 and 1/8 scale on the GPU:
mij_decoder_reconstruct_scaled and what reads its result, against the numpy
model (scaled_model.py), which tests/test_scaled_model.py pins to
libjpeg-turbo.  No test here needs Pillow."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import decode_cases as DC
import foreign_cases as FC
import mijpeg
import oracle as O
import ppm
import recipes
import scaled_cases as SC
import scaled_model as SM

pytestmark = pytest.mark.gpu

PKG = os.path.dirname(mijpeg.LIB_PATH)
_LEGACY = {"16x16": lambda: recipes.noise(16, 16, 11), "48x32": lambda: recipes.noise(32, 48, 21),
           "496x272": lambda: recipes.config3_frame(0, 272, 496)}


@functools.lru_cache(maxsize=None)
def _legacy(name):
    """a three-scan stream from mijpeg.encode with the ORACLE's coefficients
    of the same frame (decode_cases.Case, as tests/test_pixels.py has them)"""
    bgr = _LEGACY[name]()
    Y, Cb, Cr, _, jpg = O.cref_stages(bgr, 50)
    assert mijpeg.encode(bgr, 50) == jpg
    return DC.Case(name, jpg, Y, Cb, Cr, bgr.shape[1], bgr.shape[0])


def _legacy_model(name, denom):
    c = _legacy(name)
    return SM.scaled_legacy(*c.coefs, *c.dqt, c.w, c.h, denom)


def _check(d, i, s, order, denom):
    """layout, every plane and the pixels of frame i against the model s"""
    assert d.scaled_layout(i, denom)["raw"] == s.layout
    for c, want in enumerate(s.planes):
        got = d.plane(i, c)
        assert got.shape == want.shape and (got == want).all(), ("plane", c, int((got != want).sum()))
    want = s.pixels(order)
    got = d.pixels(i)
    assert got.shape == want.shape and (got == want).all(), int((got != want).any(-1).sum())
    ptr, pitch = d.device_pixels(i)
    assert pitch == (3 * s.ow + 15) // 16 * 16 and ptr % 16 == 0


@pytest.mark.parametrize("denom", SC.DENOMS)
def test_every_fixture_in_one_mixed_decode(denom):
    """all accepted fixtures in one call: the 8450 luma blocks of 1040x520
    cross the DC tile, rst1 / rstrow segment the DCs, 17x9, 35x21 and 5x8 end
    their block rows in partial strips, 3x8 and 4x8 replicate their chroma"""
    d = mijpeg.Decoder(1040, 528, len(FC.NAMES))
    try:
        d.decode([FC.jpg(n) for n in FC.NAMES])
        for order in ("rgb", "bgr"):
            d.reconstruct(order, scale=denom)
            for i, n in enumerate(FC.NAMES):
                _check(d, i, SC.model(n, denom), order, denom)
    finally:
        d.close()


@pytest.mark.parametrize("denom", SC.DENOMS)
def test_legacy_streams_mixed_with_foreign_files(denom):
    """the encoder's own three-scan streams (raster DC rule) between files
    of the other kind, against the model on the ORACLE's coefficients"""
    order = [("L", "16x16"), ("F", "420_35x21"), ("L", "496x272"), ("F", "422_35x21"), ("L", "48x32"),
             ("F", "grey_35x21")]
    d = mijpeg.Decoder(496, 272, len(order))
    try:
        d.decode([_legacy(n).jpg if k == "L" else FC.jpg(n) for k, n in order])
        d.reconstruct("rgb", scale=denom)
        for i, (k, n) in enumerate(order):
            _check(d, i, _legacy_model(n, denom) if k == "L" else SC.model(n, denom), "rgb", denom)
    finally:
        d.close()


def test_scale_one_and_full_scaled_full():
    names = ["420_35x21", "422_35x21", "444_17x9"]
    legacy = _legacy("16x16")
    d = mijpeg.Decoder(48, 32, len(names) + 1)
    try:
        d.decode([FC.jpg(n) for n in names] + [legacy.jpg])
        d.reconstruct("rgb")
        full = [d.pixels(i).copy() for i in range(len(names) + 1)]
        planes = [d.plane(0, c).copy() for c in range(3)]
        assert all((full[i] == FC.model(n).rgb).all() for i, n in enumerate(names))
        assert d.lib.mij_decoder_reconstruct_scaled(d.h_, 1, 1) == 0  # denom 1 is mij_decoder_reconstruct
        assert all((d.pixels(i) == full[i]).all() for i in range(len(full)))
        d.reconstruct("rgb", scale=1)
        assert all((d.pixels(i) == full[i]).all() for i in range(len(full)))
        assert all((d.plane(0, c) == planes[c]).all() for c in range(3))
        assert all((a == b).all() for a, b in zip(d.planes(3), legacy.planes))
        d.reconstruct("rgb", scale=4)
        for i, n in enumerate(names):
            _check(d, i, SC.model(n, 4), "rgb", 4)
        _check(d, 3, _legacy_model("16x16", 4), "rgb", 4)
        with pytest.raises(mijpeg.MijError, match="scale"):
            d.planes(3)
        assert d.lib.mij_last_error() == 1  # MIJ_EINVAL
        d.reconstruct("rgb")
        assert all((d.pixels(i) == full[i]).all() for i in range(len(full)))
        assert all((d.plane(0, c) == planes[c]).all() for c in range(3))
        assert all((a == b).all() for a, b in zip(d.planes(3), legacy.planes))
    finally:
        d.close()


def test_transcode_and_transform_are_neither_needed_nor_disturbed():
    names = ["420_70x37_rstrow", "444_40x24"]
    d = mijpeg.Decoder(80, 48, 2)
    try:
        d.decode([FC.jpg(n) for n in names])
        d.transcode(1)
        tc = [d.transcoded(i) for i in range(2)]
        d.reconstruct("rgb", scale=2)  # after a transcode
        assert [d.transcoded(i) for i in range(2)] == tc
        for i, n in enumerate(names):
            _check(d, i, SC.model(n, 2), "rgb", 2)
        d.transform("rot90", trim=True)  # after a scaled reconstruct
        xf = [d.transcoded(i) for i in range(2)]
        for i, n in enumerate(names):
            _check(d, i, SC.model(n, 2), "rgb", 2)
        d.decode([FC.jpg(n) for n in names])
        d.reconstruct("bgr", scale=8)  # before them
        d.transform("rot90", trim=True)
        assert [d.transcoded(i) for i in range(2)] == xf
        d.transcode(1)
        assert [d.transcoded(i) for i in range(2)] == tc
        for i, n in enumerate(names):
            _check(d, i, SC.model(n, 8), "bgr", 8)
    finally:
        d.close()


def test_arena_grows_from_small_frames_to_larger_ones():
    d = mijpeg.Decoder(96, 80, 2)
    try:
        d.decode([FC.jpg("420_5x5")])
        d.reconstruct("rgb", scale=2)  # the first reconstruct of this decoder is a scaled one
        _check(d, 0, SC.model("420_5x5", 2), "rgb", 2)
        d.decode([FC.jpg("444_40x24"), FC.jpg("420_96x80_noise_q95")])
        with pytest.raises(mijpeg.MijError, match="reconstruct"):
            d.pixels(0)  # the newer decode: the old pixels are no longer served
        d.reconstruct("bgr", scale=4)
        _check(d, 0, SC.model("444_40x24", 4), "bgr", 4)
        _check(d, 1, SC.model("420_96x80_noise_q95", 4), "bgr", 4)
        d.decode([_legacy("48x32").jpg])  # and the legacy buffers' first use
        d.reconstruct("rgb", scale=2)
        _check(d, 0, _legacy_model("48x32", 2), "rgb", 2)
    finally:
        d.close()


def test_pixels_with_a_larger_pitch_and_short_caps():
    s = SC.model("420_35x21", 2)
    d = mijpeg.Decoder(48, 32, 1)
    try:
        d.decode([FC.jpg("420_35x21")])
        d.reconstruct("rgb", scale=2)
        pitch = 3 * s.ow + 7
        flat = np.full(s.oh * pitch, 0xA5, np.uint8)
        d.pixels(0, pitch=pitch, out=flat)
        rows = flat.reshape(s.oh, pitch)
        assert (rows[:, :3 * s.ow] == s.rgb.reshape(s.oh, -1)).all() and (rows[:, 3 * s.ow:] == 0xA5).all()
        lib = d.lib
        need = 3 * s.ow * s.oh
        out = np.zeros(need, np.uint8)
        assert lib.mij_decoder_pixels(d.h_, 0, out.ctypes.data, need - 1, 0) == 4  # MIJ_ENOSPC: the scaled size counts
        assert str(need).encode() in lib.mij_last_message()
        assert lib.mij_decoder_pixels(d.h_, 0, out.ctypes.data, need, 0) == 0
        assert (out == s.rgb.ravel()).all()
        pl = np.zeros(s.planes[0].size, np.uint8)
        assert lib.mij_decoder_plane(d.h_, 0, 0, pl.ctypes.data, pl.size - 1) == 4
        assert lib.mij_decoder_plane(d.h_, 0, 0, pl.ctypes.data, pl.size) == 0
        lay = np.zeros(18, np.int32)
        assert lib.mij_decoder_scaled_layout(d.h_, 0, 2, lay.ctypes.data, 17) == 4
        assert lib.mij_decoder_scaled_layout(d.h_, 0, 2, lay.ctypes.data, 18) == 0 and lay.tolist() == s.layout
    finally:
        d.close()


def test_refusals():
    lib = mijpeg.load()
    d = mijpeg.Decoder(48, 32, 1)
    try:
        d.decode([FC.jpg("420_35x21")])
        d.reconstruct("rgb")
        full = d.pixels(0).copy()
        for denom in (0, 3, 16):
            assert lib.mij_decoder_reconstruct_scaled(d.h_, 1, denom) == 1, denom  # MIJ_EINVAL
            assert b"scale" in lib.mij_last_message()
            lay = np.zeros(18, np.int32)
            assert lib.mij_decoder_scaled_layout(d.h_, 0, denom, lay.ctypes.data, 18) == 1
        assert lib.mij_decoder_reconstruct_scaled(d.h_, 2, 4) == 1 and b"order" in lib.mij_last_message()
        assert (d.pixels(0) == full).all()  # a refused call leaves the last result in place
        with pytest.raises(mijpeg.MijError, match="scale"):
            mijpeg.decode(FC.jpg("420_35x21"), "rgb", scale=3)
    finally:
        d.close()
    jpg = np.frombuffer(FC.jpg("420_35x21"), np.uint8)
    probe = np.zeros(1, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    assert lib.mij_decode_scaled(jpg.ctypes.data, jpg.size, 1, 4, probe.ctypes.data, 0, C.byref(w), C.byref(h)) == 4
    assert (w.value, h.value) == (9, 6)
    bad = np.frombuffer(FC.jpg("reject_progressive"), np.uint8)
    out = np.zeros(3 * 16 * 16, np.uint8)
    assert lib.mij_decode_scaled(bad.ctypes.data, bad.size, 1, 2, out.ctypes.data, out.size, None, None) == 8  # MIJ_EJPEG
    assert b"baseline" in lib.mij_last_message().lower()


@pytest.mark.parametrize("denom", SC.DENOMS)
def test_one_call_decode(denom):
    for n in ("422_35x21", "grey_35x21", "420_1x1"):
        s = SC.model(n, denom)
        assert (mijpeg.decode(FC.jpg(n), "rgb", scale=denom) == s.rgb).all(), n
        assert (mijpeg.decode(FC.jpg(n), scale=denom) == s.bgr).all(), n
    assert (mijpeg.decode(FC.jpg("422_35x21"), "rgb", scale=1) == FC.model("422_35x21").rgb).all()


def test_thumbnail_of_a_stored_jpeg_never_leaves_the_device():
    s = SC.model("420_96x80_noise_q95", 4)
    d = mijpeg.Decoder(96, 80, 1)
    b = mijpeg.Batch(32, 32, 1, 50)
    try:
        d.decode([FC.jpg("420_96x80_noise_q95")])
        d.reconstruct("bgr", scale=4)
        ptr, pitch = d.device_pixels(0)
        b.set_stream(d.stream_ptr())  # the encode runs behind the reconstruct
        b.pad_input(ptr, 0, pitch, [(s.ow, s.oh)])
        b.encode_interleaved(1, 0)
        assert b.output(0) == mijpeg.encode_any(s.bgr, "bgr", 50, 0)
    finally:
        b.close()
        d.close()


def test_host_tool_scale_option(tmp_path):
    """host/decode_jpg -scale 1/4 writes the model's pixels as a PPM"""
    s = SC.model("420_70x37_rstrow", 4)
    out = str(tmp_path / "out.ppm")
    subprocess.run([os.path.join(PKG, "host", "decode_jpg"), "-scale", "1/4",
                    os.path.join(FC.DIR, "420_70x37_rstrow.jpg"), out], check=True, timeout=120)
    with open(out, "rb") as f:  # 18x10: the project's own PPM readers take multiples of 16 only
        assert f.read() == ppm.ppm_bytes(s.rgb)
