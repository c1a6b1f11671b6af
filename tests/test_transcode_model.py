"""Lossless transcoding without a GPU: the numpy model
(transcode_model.py) pinned to independent code.  The plain Python decoder
(foreign_model.py) must read back the source's coefficient planes, identical
and in the same layout, with the requested restart interval; Pillow's
libjpeg-turbo must give the source's pixels; a second transcode changes
nothing; and fed an interleaved stream of the encoder's (interleave_model.py)
the model gives the encoder's stream at the new restart interval, so the
header rules coincide with mij_encode_any's.  The GPU side is
tests/test_transcode_gpu.py."""
import io

import numpy as np
import pytest

import foreign_cases as FC
import foreign_model as FM
import interleave_model as IM
import oracle as O
import transcode_model as TM

ACCEPTED = [n for n in FC.NAMES if not n.startswith("reject")]
CASES = [(n, rr) for n in ACCEPTED for rr in (0, 1)]
ENC = [(1, 1, 50, "photo"), (17, 9, 50, "photo"), (35, 21, 50, "photo"), (48, 32, 100, "noise")]


def enc_frame(w, h, q, kind):
    return IM.frame(w, h, seed=q, kind=kind)


@pytest.mark.parametrize("name,rr", CASES)
def test_same_coefficients_new_intervals(name, rr):
    src = FC.model(name)
    out = TM.model(FC.jpg(name), rr)
    d = FM.decoded(out)
    G = d.G
    assert d.layout[:7] == src.layout[:7] and d.layout[8:] == src.layout[8:]  # all but the restart interval
    assert G["ri"] == rr * G["mcus_x"]
    for c in range(G["ncomp"]):
        assert d.coefs[c].shape == src.coefs[c].shape
        assert (d.coefs[c] == src.coefs[c]).all(), c
        assert (d.dqt[c] == src.dqt[c]).all(), c
    assert out.count(b"\xff\xda") == 1
    sel, data = FM.parse(out)["scan"]
    assert out.endswith(data + b"\xff\xd9")
    assert out.count(b"\xff\xdd\x00\x04") == (1 if rr else 0)
    marks = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert marks == [0xD0 + i % 8 for i in range(G["mcus_y"] - 1 if rr else 0)]
    # component entries verbatim
    assert FM.parse(out)["comps"] == FM.parse(FC.jpg(name))["comps"]


@pytest.mark.parametrize("name,rr", CASES)
def test_libjpeg_sees_the_sources_pixels(name, rr):
    try:
        from PIL import Image, features
    except ImportError:
        pytest.skip("Pillow not installed")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo")
    a = Image.open(io.BytesIO(FC.jpg(name)))
    b = Image.open(io.BytesIO(TM.model(FC.jpg(name), rr)))
    assert a.size == b.size and a.mode == b.mode
    assert (np.asarray(a) == np.asarray(b)).all()


@pytest.mark.parametrize("name,rr", CASES)
def test_second_transcode_is_the_identity(name, rr):
    out = TM.model(FC.jpg(name), rr)
    assert TM.model(out, rr) == out


SIZES = {"420_35x21": (903, 592), "444_24x24_noise_q100": (2978, 1988), "420_96x80_noise_q95": (9584, 8096),
         "420_1040x520_q30": (10239, 4720), "420_1040x520_q30_rst4": (10260, 4720), "420_33x17_opt": (554, 554)}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_recorded_sizes(name):
    """source -> transcoded bytes without restarts, as DESIGN.md §4h lists them
    (the last was already optimised by libjpeg: nothing left to gain)"""
    assert (len(FC.jpg(name)), len(TM.model(FC.jpg(name), 0))) == SIZES[name]
    if "1040" in name:  # 33 MCU rows: DRI + 32 markers + the intervals' pad bits
        assert len(TM.model(FC.jpg(name), 1)) == 4805


@pytest.mark.parametrize("w,h,q,kind", ENC)
def test_coincides_with_the_interleaved_encoder(w, h, q, kind):
    f = enc_frame(w, h, q, kind)
    for a in (0, 1):
        for b in (0, 1, 2):
            assert TM.model(IM.model(f, q, a).jpg, b) == IM.model(f, q, b).jpg, (a, b)


def test_greyscale_writes_two_dhts_and_one_dqt():
    names = [n for n in ACCEPTED if n.startswith("grey")]
    assert names
    for name in names:
        out = TM.model(FC.jpg(name), 1)
        head = out[:out.index(b"\xff\xda")]
        assert head.count(b"\xff\xc4") == 2 and head.count(b"\xff\xdb\x00\x43") == 1, name
        assert out[out.index(b"\xff\xda") + 2:][:8] == bytes([0x00, 0x08, 0x01, FM.parse(out)["comps"][0][0], 0x00,
                                                            0x00, 0x3F, 0x00])


@pytest.mark.parametrize("w,h", [(16, 16), (48, 32)])
def test_legacy_three_scan_frames_become_the_encoders_interleaved_file(w, h):
    for q in (50, 90):
        f = IM.frame(w, h, seed=q)
        legacy = O.cref_encode(f, q)
        assert legacy.count(b"\xff\xda") >= 3  # (the source really is the three-scan shape)
        for b in (0, 1):
            assert TM.model_legacy(f, q, b) == IM.model(f, q, b).jpg, (q, b)


def test_restart_rows_out_of_range():
    with pytest.raises(ValueError):
        TM.model(FC.jpg(ACCEPTED[0]), -1)
    with pytest.raises(ValueError):
        TM.model(FC.jpg(ACCEPTED[0]), 65536)
