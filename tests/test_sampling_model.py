"""Encoding at a chosen chroma sampling without a GPU: the
numpy model (sampling_model.py) pinned to the oracle by identities that need
no new C code --

  4:4:4  the 2x2 mean of four equal truncated samples is the sample, so the
         model's Cb / Cr planes of a frame are the oracle's 4:2:0 chroma
         planes of the frame with every pixel doubled in both directions;
         its Y plane is the oracle's of the frame itself
  4:2:2  (a + b + a + b) / 4 == (a + b) / 2 in integers, so its chroma planes
         are the oracle's of the frame with every row doubled
  grey   its Y plane is the 4:4:4 Y plane

-- then the streams: 4:2:0 is interleave_model's bytes, the plain Python
decoder (foreign_model.py) reads every stream back with the expected layout
and the coefficients that went in, and Pillow's libjpeg-turbo decodes them to
the decoder model's pixels.  The GPU side is tests/test_sampling_gpu.py."""
import io

import numpy as np
import pytest

import foreign_model as FM
import interleave_model as IM
import sampling_cases as SC
import sampling_model as SM

QUALITIES = (10, 50, 90, 100)


def double(f, rows=True, cols=True):
    if rows:
        f = np.repeat(f, 2, 0)
    if cols:
        f = np.repeat(f, 2, 1)
    return f


def oracle_luma(frame, q, bw, bh):
    """the oracle's Y blocks of the frame padded to 16, cut to the top-left bw x bh blocks"""
    h16, w16 = IM.pad16(frame).shape[:2]
    Y = IM.planes(frame, q)[0].reshape(h16 // 8, w16 // 8, 64)
    return Y[:bh, :bw].reshape(-1, 64)


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("w,h", [(32, 16), (21, 11)])
def test_444_planes_are_the_oracles(w, h, q):
    f = SC.photo(w, h, seed=q)
    Y, Cb, Cr = SM.planes(f, q, "444")
    G = SM.grid(w, h, "444")
    _, _, _, bw, bh = G["comps"][0]
    assert (Y == oracle_luma(f, q, bw, bh)).all()
    ref = IM.planes(double(SM.pad_mcu(f, "444")), q)  # 16 * bw x 16 * bh: no further padding
    assert Cb.shape == ref[1].shape == (bw * bh, 64)
    assert (Cb == ref[1]).all() and (Cr == ref[2]).all()


@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("w,h", [(32, 16), (21, 11)])
def test_422_planes_are_the_oracles(w, h, q):
    f = SC.photo(w, h, seed=q)
    Y, Cb, Cr = SM.planes(f, q, "422")
    G = SM.grid(w, h, "422")
    assert (Y == oracle_luma(f, q, G["comps"][0][3], G["comps"][0][4])).all()
    ref = IM.planes(double(SM.pad_mcu(f, "422"), cols=False), q)  # 16 mcus_x x 16 mcus_y
    assert Cb.shape == ref[1].shape == (G["comps"][1][3] * G["comps"][1][4], 64)
    assert (Cb == ref[1]).all() and (Cr == ref[2]).all()


@pytest.mark.parametrize("q", QUALITIES)
def test_grey_plane_is_the_444_luma(q):
    f = SC.photo(21, 11, seed=q)
    (Y,) = SM.planes(f, q, "gray")
    assert (Y == SM.planes(f, q, "444")[0]).all()


def test_padding_and_grids():
    f = SC.photo(21, 11)
    assert SM.pad_mcu(f, "444").shape == SM.pad_mcu(f, "gray").shape == (16, 24, 3)
    assert SM.pad_mcu(f, "422").shape == (16, 32, 3)
    p = SM.pad_mcu(f, "422")
    assert (p[:11, :21] == f).all() and (p[:11, 21:] == f[:, 20:21]).all() and (p[11:] == p[10:11]).all()
    assert SM.grid(21, 11, "422")["comps"] == [(2, 1, 0, 4, 2), (1, 1, 1, 2, 2), (1, 1, 1, 2, 2)]
    assert SM.grid(21, 11, "444")["comps"] == [(1, 1, 0, 3, 2), (1, 1, 1, 3, 2), (1, 1, 1, 3, 2)]
    assert SM.grid(21, 11, "gray")["comps"] == [(1, 1, 0, 3, 2)]
    # the slots the batch pads to multiples of 16 hold every sampling's extension
    for s in ("422", "444", "gray"):
        ph, pw = SM.pad_mcu(f, s).shape[:2]
        assert (IM.pad16(f)[:ph, :pw] == SM.pad_mcu(f, s)).all()


@pytest.mark.parametrize("q,rr", [(50, 0), (90, 2)])
def test_420_is_the_interleaved_model(q, rr):
    f = SC.photo(35, 21, seed=q)
    m = SM.model(f, q, rr, "420")
    assert m.jpg == IM.model(f, q, rr).jpg
    assert m.layout == FM.decoded(m.jpg).layout


STREAMS = [(w, h, q, rr, s) for (w, h) in ((1, 1), (17, 9), (35, 21)) for (q, rr) in ((50, 0), (100, 1))
           for s in ("422", "444", "gray")]


@pytest.mark.parametrize("w,h,q,rr,s", STREAMS)
def test_stream_decodes_to_the_models_coefficients(w, h, q, rr, s):
    m = SM.model(SC.photo(w, h, seed=q), q, rr, s)
    d = FM.decoded(m.jpg)
    assert (d.w, d.h) == (w, h)
    assert d.layout == m.layout
    assert d.G["ri"] == rr * m.G["mcus_x"]
    for c in range(m.G["ncomp"]):
        assert d.coefs[c].shape == m.planes[c].shape
        assert (d.coefs[c] == m.planes[c]).all(), c
    assert m.jpg.count(b"\xff\xda") == 1
    sel, data = FM.parse(m.jpg)["scan"]
    assert m.jpg.endswith(data + b"\xff\xd9")
    # greyscale: one DQT, two DHT, one component in SOS
    assert m.jpg.count(b"\xff\xdb\x00\x43") == (1 if s == "gray" else 2)
    assert len(sel) == (1 if s == "gray" else 3)
    marks = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert marks == [0xD0 + i % 8 for i in range(m.G["mcus_y"] - 1 if rr else 0)]


@pytest.mark.parametrize("w,h,q,rr,s", STREAMS)
def test_stream_opens_in_libjpeg(w, h, q, rr, s):
    try:
        from PIL import Image, features
    except ImportError:
        pytest.skip("Pillow not installed")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo")
    m = SM.model(SC.photo(w, h, seed=q), q, rr, s)
    im = Image.open(io.BytesIO(m.jpg))
    assert im.size == (w, h)
    assert im.mode == ("L" if s == "gray" else "RGB")
    ref = np.asarray(im.convert("RGB"))
    assert (ref == FM.decoded(m.jpg).rgb).all()


def test_exception_frame_shows_a_missed_exception():
    """the reference's truncated samples of the exception frame differ from
    the floor of the exact value in every channel: a front end that computed
    the colour exactly (or in another order) would not match the model on it"""
    f = SC.exception_frame()
    got = SM.samples(f, "444")
    exact = SC.exact_floor_ycc(f)
    for c in range(3):
        assert (got[c].astype(np.int64) != exact[c]).any(), c
        assert (got[c].astype(np.int64) - exact[c]).min() >= -1 and (got[c].astype(np.int64) <= exact[c]).all()
    # ... and the difference reaches the coefficients at Q = 100 (DC of a flat patch)
    P = SM.planes(f, 100, "444")
    for c in range(3):
        flat = ((exact[c][::8, ::8].astype(np.int64) - 128) * 8).reshape(-1)  # exact DC of a flat block at q = 1
        assert (P[c][:, 0] != flat).any(), c
