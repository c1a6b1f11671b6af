"""The interleaved output format without a GPU: the numpy
model of the stream (interleave_model.py) pinned to independent code -- the
plain Python baseline decoder (foreign_model.py) must read back the oracle's
coefficients of the padded frame, at the true size, with the requested restart
interval, ending exactly on EOI; and Pillow's libjpeg-turbo must open the
stream at the true size with the decoder model's pixels.  The GPU side is
tests/test_interleave_gpu.py."""
import io

import numpy as np
import pytest

import foreign_model as FM
import interleave_model as IM

SIZES = [(1, 1), (16, 16), (17, 9), (35, 21)]
CASES = [(w, h, q, rr) for (w, h) in SIZES for q in (50, 100) for rr in (0, 1)]


def case_model(w, h, q, rr):
    return IM.model(IM.frame(w, h, seed=q), q, rr)


@pytest.mark.parametrize("w,h,q,rr", CASES)
def test_stream_decodes_to_the_oracles_coefficients(w, h, q, rr):
    m = case_model(w, h, q, rr)
    d = FM.decoded(m.jpg)
    mw, mh = -(-w // 16), -(-h // 16)
    assert (d.w, d.h) == (w, h)
    G = d.G
    assert [c[:2] for c in G["comps"]] == [(2, 2), (1, 1), (1, 1)]  # 4:2:0
    assert (G["mcus_x"], G["mcus_y"]) == (mw, mh)
    assert G["ri"] == rr * mw and G["interleaved"] == 1
    for c in range(3):
        assert d.coefs[c].shape == m.planes[c].shape
        assert (d.coefs[c] == m.planes[c]).all(), c
    # one SOS, and the parser's scan ends exactly on EOI
    assert m.jpg.count(b"\xff\xda") == 1
    sel, data = FM.parse(m.jpg)["scan"]
    assert m.jpg.endswith(data + b"\xff\xd9")
    assert m.jpg.count(b"\xff\xdd\x00\x04") == (1 if rr else 0)
    # restart markers: one after every interval but the last, numbered mod 8
    marks = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert marks == [0xD0 + i % 8 for i in range(mh - 1 if rr else 0)]


@pytest.mark.parametrize("w,h,q,rr", CASES)
def test_stream_opens_in_libjpeg(w, h, q, rr):
    try:
        from PIL import Image, features
    except ImportError:
        pytest.skip("Pillow not installed")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo")
    m = case_model(w, h, q, rr)
    im = Image.open(io.BytesIO(m.jpg))
    assert im.size == (w, h)
    ref = np.asarray(im.convert("RGB"))
    assert (ref == FM.decoded(m.jpg).rgb).all()


def test_padding_rule():
    f = IM.frame(17, 9)
    p = IM.pad16(f)
    assert p.shape == (16, 32, 3)
    assert (p[:9, :17] == f).all()
    assert (p[:9, 17:] == f[:, 16:17]).all()       # last column replicated
    assert (p[9:] == p[8:9]).all()                 # then the last row
    assert IM.pad16(IM.frame(32, 16)).shape == (16, 32, 3)


def test_only_the_luma_dc_counts_differ_from_the_three_scan_form():
    """tables item of the format: AC counts and the chroma DC counts are those
    of the oracle's three-scan tables on the padded frame (no restarts)"""
    import oracle as O
    f = IM.frame(35, 21, seed=3)
    m = IM.model(f, 50, 0)
    _, _, _, tabs, _ = O.cref_stages(IM.pad16(f), 50)
    for t in (1, 2, 3):
        assert list(m.tables[t].sym_code_len) == list(tabs[t].sym_code_len)
        assert list(m.tables[t].sym_code) == list(tabs[t].sym_code)
