"""Lossless transcoding on the GPU: the kernels' bytes are
the numpy model's (transcode_model.py, pinned to foreign_model.py and Pillow
by test_transcode_model.py) and, with no model involved, the interleaved
encoder's own for the same frame at the new restart interval.  Equality of
bytes everywhere, no tolerance.  The shapes are the smallest at which each
part can go wrong: every sampling, one MCU, more than one workgroup of blocks,
more than 256 MCUs across, more than 256 MCU rows and intervals, more than one
stuffing chunk, frames of different kinds in one call."""
import ctypes as C
import re

import numpy as np
import pytest

import foreign_cases as FC
import interleave_model as IM
import mijpeg
import transcode_model as TM

pytestmark = pytest.mark.gpu

ACCEPTED = [n for n in FC.NAMES if not n.startswith("reject")]
SMALL = [n for n in ACCEPTED if "1040" not in n]

_enc = {}


def enc_any(f, q, rr):
    """mijpeg.encode_any(f, "bgr", q, rr), once per case"""
    key = (f.shape, f.tobytes(), q, rr)
    if key not in _enc:
        _enc[key] = mijpeg.encode_any(f, "bgr", q, rr)
    return _enc[key]


def same(got: bytes, want: bytes):
    assert len(got) == len(want), (len(got), len(want))
    assert got == want


# 1. every accepted small fixture: greyscale, 4:4:4, 4:2:2, 4:2:0, from 1x1, sources with Ri 0, 1 and a row
@pytest.mark.parametrize("rr", [0, 1, 2])
@pytest.mark.parametrize("name", SMALL)
def test_fixture_is_the_model(name, rr):
    same(mijpeg.transcode(FC.jpg(name), rr), TM.model(FC.jpg(name), rr))


# 2. 12 870 blocks: 51 workgroups; the second source's interval of 260 MCUs is re-segmented
@pytest.mark.parametrize("rr", [0, 3])
@pytest.mark.parametrize("name", ["420_1040x520_q30", "420_1040x520_q30_rst4"])
def test_many_workgroups(name, rr):
    same(mijpeg.transcode(FC.jpg(name), rr), TM.model(FC.jpg(name), rr))


# 3. against the encoder, no model involved
@pytest.mark.parametrize("w,h,q,kind", [(1, 1, 50, "photo"), (17, 9, 50, "photo"), (35, 21, 50, "photo"),
                                        (48, 32, 100, "noise")])
def test_interleaved_streams_change_their_interval(w, h, q, kind):
    f = IM.frame(w, h, kind=kind)
    for a in (0, 1):
        for b in (0, 1, 2):
            same(mijpeg.transcode(enc_any(f, q, a), b), enc_any(f, q, b))


# 4. the loops' second trips: 257 MCUs across, ~23 stuffing chunks and many 0xFF bytes; 257 MCU rows and
# intervals, RSTn wrapping 32 times
def test_wide_noise_frame():
    f = IM.frame(4112, 16, kind="noise")
    got = mijpeg.transcode(enc_any(f, 100, 0), 1)
    same(got, enc_any(f, 100, 1))
    assert len(got) > 5 * 4096 and got.count(b"\xff\x00") > 50


@pytest.mark.parametrize("b", [1, 0])
def test_tall_frame(b):
    f = IM.frame(16, 4112, kind="photo")
    got = mijpeg.transcode(enc_any(f, 50, 0), b)
    same(got, enc_any(f, 50, b))
    if b:
        assert sum(got.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) >= 256


# 5. the encoder's three-scan streams become its interleaved file
@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (320, 240)])
def test_legacy_streams(w, h, q):
    f = IM.frame(w, h, seed=q)
    legacy = mijpeg.encode(f, q)
    assert legacy.count(b"\xff\xda") >= 3
    for b in (0, 1):
        same(mijpeg.transcode(legacy, b), enc_any(f, q, b))


# 6. frames of every kind in one call; reconstruct after it and, in a second decoder, before it
def test_mixed_call_beside_reconstruct():
    leg = mijpeg.encode(IM.frame(48, 32, seed=5), 50)
    streams = [FC.jpg("grey_35x21"), FC.jpg("444_17x9"), FC.jpg("422_35x21"), FC.jpg("420_70x37_rst1"), leg,
               FC.jpg("420_96x80_noise_q95")]
    single = [mijpeg.transcode(s, 1) for s in streams]
    pixels = [mijpeg.decode(s) for s in streams]
    for first in ("transcode", "reconstruct"):
        d = mijpeg.Decoder(96, 80, len(streams))
        try:
            d.decode(streams)
            if first == "reconstruct":
                d.reconstruct("bgr")
            d.transcode(1)
            for i, want in enumerate(single):
                same(d.transcoded(i), want)
            assert d.transcode_ms() > 0
            if first == "transcode":
                d.reconstruct("bgr")
            for i, want in enumerate(pixels):
                assert (d.pixels(i) == want).all(), (first, i)
            for i, want in enumerate(single):  # (still served after the reconstruct)
                same(d.transcoded(i), want)
            ptr, n = d.device_transcoded(2)
            assert ptr and n == len(single[2])
        finally:
            d.close()


# 7. round trip on the device: the transcoded stream decodes to the source's planes and pixels
@pytest.mark.parametrize("name", SMALL)
def test_round_trip(name):
    src = FC.jpg(name)
    out = mijpeg.transcode(src, 1)
    assert (mijpeg.decode(out) == mijpeg.decode(src)).all()
    d = mijpeg.Decoder(96, 80, 2)
    try:
        d.decode([src, out])
        la, lb = d.layout(0), d.layout(1)
        assert la["raw"][:7] == lb["raw"][:7] and la["comps"] == lb["comps"]
        assert lb["ri"] == lb["mcus_x"]
        for c in range(la["ncomp"]):
            assert (d.component(0, c) == d.component(1, c)).all(), c
    finally:
        d.close()


# 8. state and errors
def _code(e) -> int:
    """the MIJ_* code of a MijError ("what: text (code): message")"""
    return int(re.search(r" \((\d+)\): ", str(e.value)).group(1))


def test_state_and_errors():
    lib = mijpeg.load()
    src = FC.jpg("420_35x21")
    d = mijpeg.Decoder(96, 80, 2)
    try:
        with pytest.raises(mijpeg.MijError, match="no decoded frames") as e:
            d.transcode(0)
        assert _code(e) == 1
        d.decode([src])
        with pytest.raises(mijpeg.MijError, match="transcode") as e:
            d.transcoded(0)
        assert _code(e) == 1
        with pytest.raises(mijpeg.MijError) as e:
            d.device_transcoded(0)
        assert _code(e) == 1
        for rr in (-1, 65536):
            with pytest.raises(mijpeg.MijError, match="frame 0") as e:
                d.transcode(rr)
            assert _code(e) == 1
        d.transcode(0)
        want = mijpeg.transcode(src, 0)
        same(d.transcoded(0), want)
        with pytest.raises(mijpeg.MijError) as e:
            d.transcoded(1)
        assert _code(e) == 1
        # a short buffer: MIJ_ENOSPC and the exact length
        n = C.c_size_t(0)
        buf = np.zeros(len(want), np.uint8)
        assert lib.mij_decoder_transcoded(d.h_, 0, buf.ctypes.data, len(want) - 1, C.byref(n)) == 4
        assert n.value == len(want) and not buf.any()
        assert lib.mij_decoder_transcoded(d.h_, 0, buf.ctypes.data, len(want), C.byref(n)) == 0
        assert buf.tobytes() == want
        d.decode([src])  # a newer decode: the old streams are no longer served
        with pytest.raises(mijpeg.MijError, match="transcode") as e:
            d.transcoded(0)
        assert _code(e) == 1
        with pytest.raises(mijpeg.MijError) as e:
            d.transcode_ms()
        assert _code(e) == 1
    finally:
        d.close()
    # one call, host to host: cap 0 asks for the size
    jb = np.frombuffer(src, np.uint8)
    n = C.c_size_t(0)
    assert lib.mij_transcode(jb.ctypes.data, jb.size, 0, None, 0, C.byref(n)) == 4
    assert n.value == len(want)
    for rr in (-1, 65536):
        with pytest.raises(mijpeg.MijError) as e:
            mijpeg.transcode(src, rr)
        assert _code(e) == 1


def test_refused_streams_keep_the_decoders_word():
    for name, (jpg, word) in sorted(FC.rejects().items()):
        with pytest.raises(mijpeg.MijError, match="(?i)" + word) as e:
            mijpeg.transcode(jpg, 0)
        assert _code(e) == 8, name  # MIJ_EJPEG
