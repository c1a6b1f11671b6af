"""Decode to pixels on the GPU (DESIGN.md "Decode to pixels"): k_dec_dc,
k_dec_idct and k_dec_colour against the numpy model (decode_model.py) applied
to the ORACLE's coefficients of the same frame -- never against the
library's own coefficients or pixels.  test_decode_model.py ties the model
to libjpeg and to the committed digests."""
import os
import subprocess

import numpy as np
import pytest

import decode_cases as DC
import mijpeg
import oracle as O

pytestmark = pytest.mark.gpu

PKG = os.path.dirname(mijpeg.LIB_PATH)


def check_frame(d, i, c, order):
    """planes and pixels of decoded frame i against case c's model output"""
    assert d.info(i)[:2] == (c.w, c.h)
    for got, want, what in zip(d.planes(i), c.planes, "Y Cb Cr".split()):
        assert got.shape == want.shape
        assert (got == want).all(), (c.name, what, int((got != want).sum()))
    want = c.rgb if order == "rgb" else c.bgr
    got = d.pixels(i)
    assert got.shape == want.shape
    assert (got == want).all(), (c.name, order, int((got != want).sum()))


def decode_and_check(names, max_w, max_h):
    cases = [DC.case(n) for n in names]
    d = mijpeg.Decoder(max_w, max_h, len(cases))
    try:
        d.decode([c.jpg for c in cases])
        for order in ("rgb", "bgr"):
            d.reconstruct(order)
            for i, c in enumerate(cases):
                check_frame(d, i, c, order)
    finally:
        d.close()


@pytest.mark.parametrize("name", ["noise_16x16_q50",      # one MCU: every upsampling edge is a replicated edge
                                  "noise_16x48_q50", "noise_48x16_q50",
                                  "sample_64x64",          # the committed reference stream
                                  "config3_496x272_q50"])  # 31 MCUs wide: no power-of-two tile divides it
def test_edge_shapes(name):
    c = DC.case(name)
    if name in DC.LIBJPEG_CASES:  # what is compared with is what libjpeg gives
        assert c.digests() == DC.committed_digests()[name]
    decode_and_check([name], c.w, c.h)


@pytest.mark.parametrize("quality", [10, 50, 90, 100])
def test_content(quality):
    """checkerboards at Q = 100 included: the expected values come from the
    coefficients, not from libjpeg (which misreads that stream's last block)"""
    decode_and_check([f"{r}_q{quality}" for r in ("noise", "gradients", "checkerboards", "near_gray")], 256, 128)


def test_mixed_sizes_in_one_decode():
    """16x16, 256x128 and 64x64 frames in the slots of a 256x128 decoder:
    each exact, so no halo is read across a frame's or a plane's edge"""
    decode_and_check(["noise_16x16_q50", "gradients_q90", "sample_64x64"], 256, 128)


def test_long_dc_prefix():
    """1920x1280: 38,400 luma blocks = five tiles of k_dec_dc (the last one
    short), 9,600 chroma blocks = two, their bases from k_dec_dcbase"""
    decode_and_check(["config3_1920x1280_q50"], 1920, 1280)


def test_pixels_with_padded_pitch():
    c = DC.case("noise_48x16_q50")
    pitch = 3 * c.w + 13
    d = mijpeg.Decoder(c.w, c.h, 1)
    try:
        d.decode([c.jpg])
        d.reconstruct("rgb")
        buf = np.full(c.h * pitch, 0xA5, np.uint8)
        d.pixels(0, pitch=pitch, out=buf)
        rows = buf.reshape(c.h, pitch)
        assert (rows[:, :3 * c.w].reshape(c.h, c.w, 3) == c.rgb).all()
        assert (rows[:, 3 * c.w:] == 0xA5).all()
        # the last row needs only its 3*w bytes
        tight = np.full((c.h - 1) * pitch + 3 * c.w, 0xA5, np.uint8)
        d.pixels(0, pitch=pitch, out=tight)
        assert (tight[-3 * c.w:].reshape(c.w, 3) == c.rgb[-1]).all()
    finally:
        d.close()


def test_error_paths():
    lib = mijpeg.load()
    c, c2 = DC.case("sample_64x64"), DC.case("noise_16x16_q50")
    out = np.zeros(3 * 64 * 64, np.uint8)
    d = mijpeg.Decoder(64, 64, 1)
    try:
        assert lib.mij_decoder_reconstruct(d.h_, 0) == 1  # MIJ_EINVAL: nothing decoded yet
        assert b"no decoded frames" in lib.mij_last_message()
        d.decode([c.jpg])
        assert lib.mij_decoder_pixels(d.h_, 0, out.ctypes.data, out.size, 0) == 1  # before reconstruct
        assert b"reconstruct" in lib.mij_last_message()
        assert lib.mij_decoder_planes(d.h_, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data) == 1
        assert not lib.mij_decoder_device_pixels(d.h_, 0, None) and lib.mij_last_error() == 1
        assert lib.mij_decoder_reconstruct(d.h_, 2) == 1 and b"order" in lib.mij_last_message()
        d.reconstruct("rgb")
        assert lib.mij_decoder_pixels(d.h_, 0, out.ctypes.data, out.size - 1, 0) == 4  # MIJ_ENOSPC
        assert b"12288" in lib.mij_last_message()
        assert lib.mij_decoder_pixels(d.h_, 1, out.ctypes.data, out.size, 0) == 1      # frame
        assert lib.mij_decoder_pixels(d.h_, 0, out.ctypes.data, out.size, 3 * 64 - 1) == 1  # pitch
        assert b"pitch" in lib.mij_last_message()
        assert (d.pixels(0) == c.rgb).all()
        d.decode([c2.jpg])  # a newer decode: the old pixels are no longer served
        assert lib.mij_decoder_pixels(d.h_, 0, out.ctypes.data, out.size, 0) == 1
        assert not lib.mij_decoder_device_pixels(d.h_, 0, None)
        with pytest.raises(mijpeg.MijError):
            d.reconstruct_ms()
        d.reconstruct("rgb")
        assert (d.pixels(0) == c2.rgb).all()
    finally:
        d.close()


def test_transcode_on_the_device():
    """Q = 90 stream -> BGR pixels in device memory -> mij_batch_set_input ->
    Q = 50 stream, equal to the oracle's encode of the model's pixels"""
    c = DC.case("gradients_q90")
    want = O.cref_encode(c.bgr, 50)
    d = mijpeg.Decoder(c.w, c.h, 1)
    b = mijpeg.Batch(c.w, c.h, 1, 50)
    try:
        d.decode([c.jpg])
        d.reconstruct("bgr")
        ptr, pitch = d.device_pixels(0)
        assert pitch == 3 * c.w and ptr % 16 == 0
        d.reconstruct_ms()  # waits: the batch encodes on a stream of its own
        b.set_input(ptr, pitch * c.h, pitch)
        b.encode(1)
        assert b.output(0) == want
    finally:
        b.close()  # the batch first: its input is the decoder's memory
        d.close()


def test_reconstruct_is_deterministic():
    cases = [DC.case("noise_q100"), DC.case("config3_496x272_q50")]
    d = mijpeg.Decoder(496, 272, 2)
    try:
        d.decode([c.jpg for c in cases])
        for rep in range(5):
            d.reconstruct("bgr")
            for i, c in enumerate(cases):
                assert (d.pixels(i) == c.bgr).all(), (rep, c.name)
            ms = d.reconstruct_ms()
            assert len(ms) == 2 and all(t > 0 for t in ms)
    finally:
        d.close()


def test_one_call_decode():
    c = DC.case("near_gray_q50")
    d = mijpeg.Decoder(c.w, c.h, 1)
    try:
        d.decode([c.jpg])
        d.reconstruct("bgr")
        via_decoder = d.pixels(0)
    finally:
        d.close()
    assert (via_decoder == c.bgr).all()
    assert (mijpeg.decode(c.jpg) == via_decoder).all()
    assert (mijpeg.decode(c.jpg, order="rgb") == c.rgb).all()


def test_host_tool(tmp_path):
    """host/decode_jpg on the committed 64x64 stream: a PPM mij_ppm_read accepts, the model's pixels"""
    c = DC.case("sample_64x64")
    out = str(tmp_path / "out.ppm")
    subprocess.run([os.path.join(PKG, "host", "decode_jpg"), os.path.join(DC.recipes.GOLDEN, "sample_64x64.jpg"), out],
                   check=True, timeout=120)
    assert mijpeg.ppm_header(out)[:2] == (64, 64)
    assert (mijpeg.ppm_read(out) == c.rgb).all()
    assert (mijpeg.ppm_read(out, to_bgr=True) == c.bgr).all()
