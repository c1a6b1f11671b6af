"""Lossless transforms on the GPU: k_xf_blocks in front of the
transcoding stages gives the numpy model's bytes (transform_model.py, pinned
to the float IDCT and Pillow by test_transform_model.py) or, with no model
involved, satisfies the algebra of the operations and equals the encoder's
own stream of the cropped frame.  Equality of bytes and integers everywhere,
no tolerance.  The shapes are the smallest at which each part can go wrong:
every sampling, one block, a partial MCU trimmed away, more than one workgroup
of blocks, a grid one MCU wide or one MCU high and more than 256 long, frames
of different kinds in one call."""
import re

import numpy as np
import pytest

import foreign_cases as FC
import foreign_model as FM
import interleave_model as IM
import mijpeg
import transcode_model as TM
import transform_model as XM
from transform_model import app1, spliced

pytestmark = pytest.mark.gpu

ACCEPTED = [n for n in FC.NAMES if not n.startswith("reject")]
SMALL = [n for n in ACCEPTED if "1040" not in n]


def same(got: bytes, want: bytes):
    assert len(got) == len(want), (len(got), len(want))
    assert got == want


def _code(e) -> int:
    """the MIJ_* code of a MijError ("what: text (code): message")"""
    return int(re.search(r" \((\d+)\): ", str(e.value)).group(1))


def is_the_model(jpg, op, trim=False, crop=None, rr=0):
    """bytes == model, or both refuse"""
    try:
        want = XM.model(jpg, op, trim, crop, rr)
    except XM.Refused:
        with pytest.raises(mijpeg.MijError) as e:
            mijpeg.transform(jpg, op, trim, crop, rr)
        assert _code(e) == 1  # MIJ_EINVAL
        return None
    got = mijpeg.transform(jpg, op, trim, crop, rr)
    same(got, want)
    return got


# 1. every accepted small fixture: 1x1, greyscale, 4:4:4, 4:2:2 (not transposed), 4:2:0, sources with Ri 0, 1, a row
@pytest.mark.parametrize("rr", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_fixture_is_the_model(name, rr):
    done = 0
    for op in XM.OPS:
        done += is_the_model(FC.jpg(name), op, True, None, rr) is not None
    assert done >= 2


# 2. more than one workgroup of blocks, and a real partial MCU row trimmed away: 520 -> 512, 65 x 32 MCUs
@pytest.mark.parametrize("rr", [0, 3])
@pytest.mark.parametrize("name", ["420_1040x520_q30", "420_1040x520_q30_rst4"])
def test_many_workgroups(name, rr):
    for op in ("rot90", "transverse"):
        got = is_the_model(FC.jpg(name), op, True, None, rr)
        assert FM.geometry(FM.parse(got))["mcus_x"] == 32 and FM.geometry(FM.parse(got))["mcus_y"] == 65


# 3. the later stages' second loop trips on the NEW geometry: 257 MCU rows and intervals out of one row, and back
def test_wide_frame_stood_on_end():
    src = mijpeg.encode_any(IM.frame(4112, 16, kind="noise"), "bgr", 100, 0)
    up = is_the_model(src, "rot90", False, None, 1)
    G = FM.geometry(FM.parse(up))
    assert (G["mcus_x"], G["mcus_y"], G["ri"]) == (1, 257, 1)
    same(mijpeg.transform(up, "rot270"), mijpeg.transcode(src, 0))


def test_tall_frame_laid_down():
    src = mijpeg.encode_any(IM.frame(16, 4112, kind="photo"), "bgr", 50, 0)
    flat = is_the_model(src, "rot270", False, None, 1)
    G = FM.geometry(FM.parse(flat))
    assert (G["mcus_x"], G["mcus_y"], G["ri"]) == (257, 1, 257)
    same(mijpeg.transform(flat, "rot90"), mijpeg.transcode(src, 0))


# 4. the algebra of the operations, no model involved
def _streams():
    return [("any 48x32", mijpeg.encode_any(IM.frame(48, 32, seed=1), "bgr", 50, 0)),
            ("any 64x48", mijpeg.encode_any(IM.frame(64, 48, seed=2), "bgr", 90, 1)),
            ("legacy 48x32", mijpeg.encode(IM.frame(48, 32, seed=3), 50))]


def test_identities():
    for what, j in _streams():
        plain = mijpeg.transcode(j, 0)
        for op in ("flip_h", "flip_v", "rot180", "transpose", "transverse"):
            once = mijpeg.transform(j, op)
            assert once != plain, (what, op)
            same(mijpeg.transform(once, op), plain)
        r = j
        for _ in range(4):
            r = mijpeg.transform(r, "rot90")
        same(r, plain)
        same(mijpeg.transform(mijpeg.transform(j, "transpose"), "flip_h"), mijpeg.transform(j, "rot90"))
        same(mijpeg.transform(j, "none"), plain)
        same(mijpeg.transform(j, "none", restart_rows=2), mijpeg.transcode(j, 2))
    f = IM.frame(48, 32, seed=3)
    same(mijpeg.transform(mijpeg.encode(f, 50), "none"), mijpeg.encode_any(f, "bgr", 50, 0))


# 5. crop: against the encoder (sides that are multiples of 16: the blocks are the same pixels), and the model
def test_crop():
    f = IM.frame(64, 48, seed=4)
    j = mijpeg.encode_any(f, "bgr", 50, 0)
    for rr in (0, 1):
        same(mijpeg.transform(j, "none", crop=(16, 16, 32, 32), restart_rows=rr),
             mijpeg.encode_any(np.ascontiguousarray(f[16:48, 16:48]), "bgr", 50, rr))
    src = FC.jpg("420_70x37_rst1")
    cut = is_the_model(src, "none", False, (16, 0, 19, 21))
    assert FM.parse(cut)["w"] == 19 and FM.parse(cut)["h"] == 21
    turned = is_the_model(src, "rot180", True, (16, 0, 19, 21))
    assert FM.parse(turned)["w"] == 16 and FM.parse(turned)["h"] == 16
    assert is_the_model(src, "rot180", False, (16, 0, 19, 21)) is None  # refused by both


# 6. frames of every kind in one call, beside transcode and reconstruct
def test_mixed_batch():
    leg = mijpeg.encode(IM.frame(48, 32, seed=5), 50)
    streams = [leg, FC.jpg("grey_35x21"), FC.jpg("444_17x9"), FC.jpg("420_96x80_noise_q95")]
    single = [mijpeg.transform(s, "rot90", True, None, 1) for s in streams]
    plain = [mijpeg.transcode(s, 0) for s in streams]
    pixels = [mijpeg.decode(s) for s in streams]
    d = mijpeg.Decoder(96, 80, 5)
    try:
        d.decode(streams)
        d.reconstruct("bgr")
        for i, want in enumerate(pixels):
            assert (d.pixels(i) == want).all(), i
        d.transform("rot90", True, None, 1)
        for i, want in enumerate(single):
            same(d.transcoded(i), want)
        assert d.transcode_ms() > 0
        ptr, n = d.device_transcoded(3)
        assert ptr and n == len(single[3])
        d.transcode(0)  # the decoded planes are as they were
        for i, want in enumerate(plain):
            same(d.transcoded(i), want)
        d.transform("none")
        for i, want in enumerate(plain):
            same(d.transcoded(i), want)
        d.reconstruct("bgr")
        for i, want in enumerate(pixels):
            assert (d.pixels(i) == want).all(), i
        d.decode(streams)  # a newer decode: the old streams are no longer served
        with pytest.raises(mijpeg.MijError, match="transform") as e:
            d.transcoded(0)
        assert _code(e) == 1
        # one refused frame refuses the call, before any device work: nothing is served afterwards either
        d.decode(streams + [FC.jpg("422_35x21")])
        with pytest.raises(mijpeg.MijError, match="frame 4.*sampling") as e:
            d.transform("rot90", True)
        assert _code(e) == 1
        with pytest.raises(mijpeg.MijError) as e:
            d.transcoded(0)
        assert _code(e) == 1
        d.transform("flip_h", True)  # 4:2:2 may be mirrored
        same(d.transcoded(4), XM.model(FC.jpg("422_35x21"), "flip_h", True))
    finally:
        d.close()


# 7. round trip through the library's own decoder: the model's pixels of the model's stream
@pytest.mark.parametrize("name", ["420_35x21", "444_40x24", "grey_8x8"])
def test_round_trip(name):
    for op in XM.OPS:
        got = mijpeg.decode(mijpeg.transform(FC.jpg(name), op, trim=True), "rgb")
        want = FM.decoded(XM.model(FC.jpg(name), op, True)).rgb
        assert got.shape == want.shape and (got == want).all(), op


# 8. by EXIF orientation
def test_auto():
    j = FC.jpg("444_40x24")
    tagged = spliced("444_40x24", app1("MM", 6))
    same(mijpeg.transform(tagged, "auto"), mijpeg.transform(j, "rot90"))
    assert mijpeg.exif_orientation(mijpeg.transform(tagged, "auto")) == 1  # the APP1 is not carried over
    same(mijpeg.transform(j, "auto"), mijpeg.transcode(j, 0))
    with pytest.raises(mijpeg.MijError):
        mijpeg.transform(j, "sideways")


def test_host_tool(tmp_path):
    """host/transcode_jpg -rotate 90 -trim: the library's bytes"""
    import os
    import subprocess
    src = os.path.join(FC.DIR, "420_35x21.jpg")
    out = str(tmp_path / "out.jpg")
    exe = os.path.join(os.path.dirname(mijpeg.LIB_PATH), "host", "transcode_jpg")
    subprocess.run([exe, "-rotate", "90", "-trim", src, out], check=True, timeout=120)
    with open(out, "rb") as f:
        same(f.read(), XM.model(FC.jpg("420_35x21"), "rot90", True))
    subprocess.run([exe, "-crop", "16x16+16+0", "-flip", "h", src, out, "1"], check=True, timeout=120)
    with open(out, "rb") as f:
        same(f.read(), XM.model(FC.jpg("420_35x21"), "flip_h", False, (16, 0, 16, 16), 1))
