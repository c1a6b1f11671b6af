"""Encoding as libjpeg does, on the GPU: for every case the
batch's layout, every component plane (which tells a front-end error from an
entropy-coder error) and the stream's bytes are the numpy model's
(ijg_model.py, pinned to Pillow's libjpeg-turbo and to a manifest by
test_ijg_model.py); the streams decode with mijpeg.decode to the pixels the
plain Python decoder gives for them.  The shapes are the smallest at which
each part can go wrong."""
import io
import os
import subprocess

import numpy as np
import pytest

import foreign_cases as FC
import foreign_model as FM
import ijg_cases as IC
import ijg_model as J
import interleave_model as IM
import mijpeg
import ppm
import resize_model as RM
import sampling_model as SM
import scaled_cases as SC

pytestmark = pytest.mark.gpu

PKG = os.path.dirname(mijpeg.LIB_PATH)
# k_ijg_fdct's tile is 128 x 16 pixels: two tiles across and three down, with
# a right dummy column (25 real luma blocks of 26) and a bottom dummy row (5
# real luma block rows of 6 at 4:2:0) in the last tiles
TILE_FRAME = (200, 40)
# (1, 1) and (8, 8); (5, 5): right and bottom dummies together; (17, 9): a
# right dummy; (40, 24): a bottom dummy row and the sample-row replication;
# (3, 8): chroma two samples wide and four rows high; (33, 31)
SIZES = [(1, 1), (8, 8), (5, 5), (17, 9), (40, 24), (3, 8), (33, 31), TILE_FRAME]


def r16(v):
    return (v + 15) & ~15


def check(b, i, frame_bgr, q, rr, s, decode=True):
    m = J.model(frame_bgr, q, rr, s)
    assert b.sampled_layout(i)["raw"] == m.layout
    for c in range(m.G["ncomp"]):
        got_c = b.sampled_component(i, c)
        assert got_c.shape == m.planes[c].shape
        bad = np.argwhere(got_c != m.planes[c])
        assert bad.size == 0, (s, c, len(bad), bad[:4].tolist())
    got = b.output(i)
    assert len(got) == len(m.jpg), (len(got), len(m.jpg))
    assert got == m.jpg
    if decode:
        px = mijpeg.decode(got, "rgb")
        assert px.shape == frame_bgr.shape
        assert (px == FM.decoded(m.jpg).rgb).all()
    return got


@pytest.mark.parametrize("q", [50, 95])
@pytest.mark.parametrize("s", IC.SAMPLINGS)
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_restarts_orders(w, h, s, q):
    f = IC.frame("photo", w, h, seed=q)
    rgb = np.ascontiguousarray(f[..., ::-1])
    b = mijpeg.Batch(r16(w), r16(h), 1, q)
    try:
        for order in ("bgr", "rgb"):
            b.set_rgb(order == "rgb")
            b.upload_any(rgb if order == "rgb" else f, 0)
            for rr in (0, 1, 3):
                b.encode_libjpeg(1, s, rr)
                check(b, 0, f, q, rr, s, decode=order == "bgr")
    finally:
        b.close()


@pytest.mark.parametrize("s", IC.SAMPLINGS)
def test_extremes(s):
    """flat 0 (DC -1024 at Q = 100), flat 255 and the period-1 checkerboard (the largest AC), at Q = 100 and Q = 1"""
    for name, f, q in IC.special_group(s):
        b = mijpeg.Batch(16, 16, 1, q)
        try:
            b.upload_any(f, 0)
            b.encode_libjpeg(1, s, 0)
            check(b, 0, f, q, 0, s)
        finally:
            b.close()


def test_mixed_sizes_and_the_other_front_end_on_the_same_batch():
    """frames of four sizes in one call; then the same batch through
    encode_sampled and back: the buffers are shared, the results do not leak
    into each other, sampled_layout follows the last call"""
    sizes = [(1, 1), (40, 24), TILE_FRAME, (33, 31)]
    frames = [IC.frame("photo", w, h, seed=i) for i, (w, h) in enumerate(sizes)]
    b = mijpeg.Batch(208, 48, 4, 50)
    try:
        for i, f in enumerate(frames):
            b.upload_any(f, i)
        for s, rr in (("420", 1), ("444", 0)):
            b.encode_libjpeg(4, s, rr)
            lens = b.lengths(4)
            for i, f in enumerate(frames):
                assert lens[i] == len(J.model(f, 50, rr, s).jpg)
                check(b, i, f, 50, rr, s, decode=False)
        b.encode_sampled(4, "422", 2)
        for i, f in enumerate(frames):
            m = SM.model(f, 50, 2, "422")
            assert b.sampled_layout(i)["raw"] == m.layout
            assert (b.sampled_component(i, 1) == m.planes[1]).all()
            assert b.output(i) == m.jpg
        b.encode_libjpeg(3, "422", 2)
        for i in range(3):
            check(b, i, frames[i], 50, 2, "422", decode=False)
        b.encode_libjpeg(2, "gray", 0)  # fewer frames than before: nothing stale
        for i in range(2):
            check(b, i, frames[i], 50, 0, "gray", decode=False)
    finally:
        b.close()


def test_the_other_encoders_are_untouched():
    """encode_interleaved and encode_sampled on the same batch give, after an encode_libjpeg, the bytes they gave before"""
    f = IC.frame("photo", 100, 75, seed=3)
    b = mijpeg.Batch(112, 80, 1, 50)
    try:
        b.upload_any(f, 0)
        before = {}
        b.encode_interleaved(1, 2)
        before["il"] = b.output(0)
        for s in ("420", "444", "gray"):
            b.encode_sampled(1, s, 1)
            before[s] = b.output(0)
        assert before["il"] == IM.model(f, 50, 2).jpg and before["444"] == SM.model(f, 50, 1, "444").jpg
        for s in IC.SAMPLINGS:
            b.encode_libjpeg(1, s, 1)
            check(b, 0, f, 50, 1, s, decode=False)
            b.encode_interleaved(1, 2)
            assert b.output(0) == before["il"]
            for t in ("420", "444", "gray"):
                b.encode_sampled(1, t, 1)
                assert b.output(0) == before[t], (s, t)
            assert b.sampled_layout(0)["raw"] == SM.model(f, 50, 1, "gray").layout
    finally:
        b.close()


def test_one_call_and_errors():
    f = IC.frame("photo", 35, 21, seed=8)
    for s in IC.SAMPLINGS:
        assert mijpeg.encode_libjpeg(f, "bgr", 75, 1, s) == J.model(f, 75, 1, s).jpg
    assert mijpeg.encode_libjpeg(np.ascontiguousarray(f[..., ::-1]), "rgb", 30, 0, "420") == J.model(f, 30, 0, "420").jpg
    lib = mijpeg.load()
    b = mijpeg.Batch(48, 32, 2, 50)
    try:
        with pytest.raises(mijpeg.MijError, match="encode_libjpeg: slot 0 holds no padded input"):
            b.encode_libjpeg(1, "420", 0)
        b.upload_any(f, 0)
        with pytest.raises(mijpeg.MijError, match="slot 1 holds no padded input"):
            b.encode_libjpeg(2, "420", 0)
        assert lib.mij_batch_encode_libjpeg(b.h_, 1, 4, 0) == 1 and "sampling 4" in lib.mij_last_message().decode()
        assert lib.mij_batch_encode_libjpeg(b.h_, 1, 0, -1) == 1
        assert lib.mij_batch_encode_libjpeg(b.h_, 0, 0, 0) == 1
        assert lib.mij_batch_encode_libjpeg(b.h_, 1, 2, 13108) == 1 and "over 65535" in lib.mij_last_message().decode()
        b.set_rgb(True)
        assert lib.mij_batch_encode_libjpeg(b.h_, 1, 0, 0) == 1 and "set_rgb changed" in lib.mij_last_message().decode()
    finally:
        b.close()


THUMBS = [(name, size, f, s) for name in ("420_70x37_rst1", "420_1040x520_q30") for size in ((20, 17), (130, 65))
          for f in ("bicubic", "box") for s in ("420", "444")]


def thumb_source(name, size):
    m = FC.model(name)
    denom = mijpeg.thumbnail_denom(m.w, m.h, *size)
    return denom, np.ascontiguousarray(SC.model(name, denom).bgr if denom > 1 else m.rgb[..., ::-1])


@pytest.mark.parametrize("name,size,f,s", THUMBS)
def test_thumbnail(name, size, f, s):
    """mij_thumbnail_libjpeg is ijg_model of resize_model of the scaled model
    decode; where Pillow is installed, its coefficients are those of
    Image.open -> draft -> resize -> save(quality, subsampling, optimize)"""
    q = 75
    denom, px = thumb_source(name, size)
    want = J.model(RM.resize(px, size, f), q, 0, s).jpg
    got = mijpeg.thumbnail(FC.jpg(name), size, f, q, arithmetic="libjpeg", sampling=s)
    assert got == want
    if IC.have_pillow():
        from PIL import Image
        im = Image.open(io.BytesIO(FC.jpg(name)))
        im.draft("RGB", size)
        assert im.size == px.shape[1::-1]
        buf = io.BytesIO()
        im.resize(size, getattr(Image, f.upper())).save(buf, "JPEG", quality=q, subsampling=IC.PIL_SUBSAMPLING[s],
                                                         optimize=True)
        P, R = FM.parse(got), FM.parse(buf.getvalue())
        assert FM.layout_list(FM.geometry(P)) == FM.layout_list(FM.geometry(R))
        assert all((P["dqt"][t] == R["dqt"][t]).all() for t in (0, 1))
        for a, b in zip(FM.coefficients(P, FM.geometry(P)), FM.coefficients(R, FM.geometry(R))):
            assert (a == b).all()


def test_command_line(tmp_path):
    """host/encode_ppm --libjpeg and host/thumbnail_jpg --libjpeg write the bytes the Python calls give"""
    f = IC.frame("photo", 35, 21, seed=8)
    src = tmp_path / "in.ppm"
    src.write_bytes(ppm.ppm_bytes(np.ascontiguousarray(f[..., ::-1])))
    exe = os.path.join(PKG, "host", "encode_ppm")
    for extra, s in ((["--libjpeg", "--sampling", "422"], "422"), (["--libjpeg"], "420")):
        dst = tmp_path / f"out_{s}.jpg"
        r = subprocess.run([exe, str(src), str(dst), "90"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert dst.read_bytes() == mijpeg.encode_libjpeg(f, "bgr", 90, 0, s)
    name, size = "420_70x37_rst1", (20, 17)
    out = tmp_path / "thumb.jpg"
    subprocess.run([os.path.join(PKG, "host", "thumbnail_jpg"), "-filter", "box", "-quality", "60", "--libjpeg",
                    "--sampling", "444", f"{size[0]}x{size[1]}", os.path.join(FC.DIR, name + ".jpg"), str(out)],
                   check=True, timeout=120)
    assert out.read_bytes() == mijpeg.thumbnail(FC.jpg(name), size, "box", 60, arithmetic="libjpeg", sampling="444")
