"""4:4:0 files and transposed 4:2:2 ones on the GPU: a decoder
with MIJ_ACCEPT_440 against the numpy model (s440_model.py, pinned to Pillow
and jpegtran by tests/test_s440_model.py), through decode, every scale,
progressive input, both transcoders, the transforms and the loader.  Every
comparison is equality; no test here needs Pillow."""
import io
import os

import numpy as np
import pytest

import foreign_cases as FC
import mijpeg
import recipes
import resize_model as RM
import s440_cases as SC
import s440_model as SM
import tensor_model as TM
import transform_model as XM

pytestmark = pytest.mark.gpu

BOTH = mijpeg.ACCEPT_440 | mijpeg.ACCEPT_PROGRESSIVE


def _check_frame(d, i, m):
    assert d.layout(i)["raw"] == m.layout
    assert d.info(i)[:2] == (m.w, m.h)
    for c in range(m.G["ncomp"]):
        assert (d.component(i, c) == m.coefs[c]).all(), ("coefficients", c)


def _check_pixels(d, i, s, order):
    """s: the model at the scale of the last reconstruct (a Decoded serves full size)"""
    for c in range(len(s.planes)):
        assert (d.plane(i, c) == s.planes[c]).all(), ("plane", c)
    got, want = d.pixels(i), s.pixels(order)
    assert got.shape == want.shape and (got == want).all(), int((got != want).any(-1).sum())


def _legacy():
    with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
        return f.read()


def _mixed():
    """every baseline 4:4:0 fixture with a 4:2:0, a 4:2:2, a greyscale and a legacy three-scan stream among them"""
    items = [(n, SC.jpg(n)) for n in SC.BASELINE]
    items[2:2] = [("420_70x37_rstrow", FC.jpg("420_70x37_rstrow")), ("422_35x21", FC.jpg("422_35x21"))]
    items += [("grey_35x21", FC.jpg("grey_35x21")), ("legacy", _legacy())]
    return items


@pytest.fixture(scope="module")
def dec():
    d = mijpeg.Decoder(528, 1040, 16, accept440=True)
    yield d
    d.close()


# ---- 1. opt-in ---------------------------------------------------------------------------
def test_opt_in():
    f440, f422, f420 = SC.jpg("440_21x35"), SC.jpg("422_35x21"), FC.jpg("420_35x21")
    m = SC.model("440_21x35")
    d = mijpeg.Decoder(48, 48, 2)
    try:
        def refused():
            with pytest.raises(mijpeg.MijError, match=r"stream 1: luma sampling 1x2 \(only 1x1, 2x1, 2x2\)$"):
                d.decode([f420, f440])
            d.decode([f422])
            with pytest.raises(mijpeg.MijError, match="frame 0: ROT90 of a component with sampling 2x1"):
                d.transform("rot90", trim=True)
        refused()
        d.accept(mijpeg.ACCEPT_440)
        d.decode([f420, f440])
        _check_frame(d, 1, m)
        d.reconstruct("rgb")
        _check_pixels(d, 1, m, "rgb")
        d.decode([f422])
        d.transform("rot90", trim=True)
        assert d.transcoded(0) == SM.model(f422, "rot90", True)
        with pytest.raises(mijpeg.MijError, match="SOF 0xC2 is not baseline"):
            d.decode([SC.jpg("p440_21x35")])
        d.accept(0)
        refused()
        d.decode([f420])
        _check_frame(d, 0, FC.model("420_35x21"))
        with pytest.raises(mijpeg.MijError, match="unknown bits"):
            d.accept(2)
        with pytest.raises(mijpeg.MijError, match="unknown bits"):
            d.accept(8 | mijpeg.ACCEPT_440)
        d.accept(BOTH)
        d.decode([SC.jpg("p440_21x35"), f440])
        _check_frame(d, 0, SC.model("p440_21x35"))
        _check_frame(d, 1, m)
        # 4:1:1 (luma 4x1), luma 2x4 and chroma 1x2 stay refused; the message names what is admitted now
        for src in (f440, SC.jpg("p440_21x35")):
            with pytest.raises(mijpeg.MijError, match=r"luma sampling 4x1 \(only 1x1, 2x1, 2x2, 1x2\)"):
                d.decode([SC.with_luma_hv(src, 0x41)])
            with pytest.raises(mijpeg.MijError, match=r"luma sampling 2x4 \(only 1x1, 2x1, 2x2, 1x2\)"):
                d.decode([SC.with_luma_hv(src, 0x24)])
        i = f440.find(b"\xff\xc0") + 4 + 6 + 1 + 3
        with pytest.raises(mijpeg.MijError, match=r"chroma sampling 1x2 / 1x1 \(only 1x1\)"):
            d.decode([f440[:i] + b"\x12" + f440[i + 1:]])
        d.decode([f440])
        _check_frame(d, 0, m)
    finally:
        d.close()
    # the keyword of the one-shot calls routes through such a decoder; off by default
    with pytest.raises(mijpeg.MijError, match="luma sampling 1x2"):
        mijpeg.decode(f440, "rgb")
    assert (mijpeg.decode(f440, "rgb", accept440=True) == m.rgb).all()
    assert (mijpeg.decode(f440, "bgr", scale=4, accept440=True) == SC.scaled("440_21x35", 4).bgr).all()
    assert (mijpeg.decode(SC.jpg("p440_21x35"), "rgb", progressive=True, accept440=True) == m.rgb).all()
    assert mijpeg.transcode(f440, 1, accept440=True) == SM.model(f440, restart_rows=1)


# ---- 2. decode ---------------------------------------------------------------------------
def _model_of(name, jpg):
    return None if name == "legacy" else SM.decoded(jpg)


@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "reversed"])
def test_decode_mixed_call(dec, reverse):
    items = _mixed()[::-1] if reverse else _mixed()
    dec.decode([j for _, j in items])
    gold = np.load(os.path.join(recipes.GOLDEN, "sample_64x64.coefs.npz"))
    for i, (name, jpg) in enumerate(items):
        if name == "legacy":
            for got, k in zip(dec.coefs(i), ("Y", "Cb", "Cr")):
                assert (got.ravel() == gold[k].ravel()).all(), k
        else:
            _check_frame(dec, i, _model_of(name, jpg))
    for order in ("rgb", "bgr"):
        dec.reconstruct(order)
        for i, (name, jpg) in enumerate(items):
            if name != "legacy":
                _check_pixels(dec, i, _model_of(name, jpg), order)


# ---- 3. scales ---------------------------------------------------------------------------
def test_scales_mixed_call(dec):
    items = [it for it in _mixed() if it[0] != "legacy"]
    dec.decode([j for _, j in items])
    for scale in (2, 4, 8, 1, 4, 1):  # and full -> scaled -> full
        dec.reconstruct("rgb", scale)
        for i, (name, jpg) in enumerate(items):
            s = SM.scaled(jpg, scale)
            if scale > 1:
                assert dec.scaled_layout(i, scale)["raw"] == s.layout, (name, scale)
            _check_pixels(dec, i, s, "rgb")
    dec.reconstruct("bgr", 2)
    for i, (name, jpg) in enumerate(items):
        _check_pixels(dec, i, SM.scaled(jpg, 2), "bgr")
    # the full-size layout of a 4:4:0 frame through the scaled call: S = 8 everywhere
    at = [n for n, _ in items].index("440_21x35")
    assert dec.scaled_layout(at, 1)["raw"] == SC.scaled("440_21x35", 1).layout


# ---- 4. progressive in ---------------------------------------------------------------------
@pytest.mark.parametrize("mapping", [0, 1])
def test_progressive_files_equal_their_baseline_twins(mapping):
    names = sorted(SC.PROGRESSIVE)
    d = mijpeg.Decoder(48, 80, 4, progressive=True, accept440=True)
    try:
        assert d.lib.mij_test_prog_mapping(d.h_, mapping) == 1
        d.decode([SC.jpg(n) for n in names] + [SC.jpg(SC.PROGRESSIVE[n]) for n in names])
        for i, n in enumerate(names):
            _check_frame(d, i, SC.model(n))
            scans = SC.model(n).P["scans"]
            assert d.scan_info(i) == {"progressive": True, "nscans": len(scans), "levels": max(e["level"] for e in scans)}
            for c in range(3):
                assert (d.component(i, c) == d.component(i + len(names), c)).all(), (n, c)
        for scale in (1, 2, 4, 8):
            d.reconstruct("rgb", scale)
            for i, n in enumerate(names):
                _check_pixels(d, i, SC.scaled(n, scale), "rgb")
                for c in range(3):
                    assert (d.plane(i, c) == d.plane(i + len(names), c)).all(), (n, scale, c)
                assert (d.pixels(i) == d.pixels(i + len(names))).all(), (n, scale)
        d.transcode(1)
        for i in range(len(names)):
            assert d.transcoded(i) == d.transcoded(i + len(names))
    finally:
        d.close()


# ---- 5. transcode --------------------------------------------------------------------------
@pytest.mark.parametrize("output", ["baseline", "progressive"])
@pytest.mark.parametrize("restart_rows", [0, 1])
def test_transcode_every_fixture(dec, output, restart_rows):
    names = SC.NAMES
    dec.accept(BOTH)
    dec.output(output)
    try:
        dec.decode([SC.jpg(n) for n in names])
        dec.transcode(restart_rows)
        outs = [dec.transcoded(i) for i in range(len(names))]
        for n, out in zip(names, outs):
            assert out == SM.model(SC.jpg(n), restart_rows=restart_rows, output=output), n
            sof = out.find(b"\xff\xc2" if output == "progressive" else b"\xff\xc0")
            assert out[sof + 9:sof + 19] == bytes([3, 1, 0x12, out[sof + 12], 2, 0x11, out[sof + 15], 3, 0x11, out[sof + 18]]), n
        # back in: the source's planes
        dec.decode(outs)
        for i, n in enumerate(names):
            m = SC.model(n)
            for c in range(3):
                assert (dec.component(i, c) == m.coefs[c]).all(), (n, c)
            lay = dec.layout(i)["raw"]
            assert lay[:7] == m.layout[:7] and lay[9:] == m.layout[9:], n
            assert lay[7] == (0 if output == "progressive" else restart_rows * m.layout[5]), n
    finally:
        dec.output("baseline")
        dec.accept(mijpeg.ACCEPT_440)
    try:
        from PIL import Image
    except ImportError:
        return
    for n, out in zip(names, outs):
        assert (np.asarray(Image.open(io.BytesIO(out)).convert("RGB")) == SC.model(n).rgb).all(), n


# ---- 6. transform --------------------------------------------------------------------------
XF_FILES = ["422_48x32", "422_35x21", "440_21x35", "440_37x70_rstrow", "440_520x1040_q30"]


@pytest.mark.parametrize("trim", [False, True], ids=["perfect", "trim"])
def test_every_operation(dec, trim):
    files = [SC.jpg(n) for n in XF_FILES]
    dec.decode(files)
    for op in XM.OPS:
        want = []
        for j in files:
            try:
                want.append(SM.model(j, op, trim, None, 1))
            except XM.Refused:
                want.append(None)
        if any(w is None for w in want):  # one refused frame refuses the call
            assert not trim, op
            with pytest.raises(mijpeg.MijError, match=rf"frame {[w is None for w in want].index(True)}: "):
                dec.transform(op, trim, None, 1)
            # ... and each frame that the model keeps is written alone
            d1 = mijpeg.Decoder(528, 1040, 1, accept440=True)
            try:
                for n, j, w in zip(XF_FILES, files, want):
                    d1.decode([j])
                    if w is None:
                        with pytest.raises(mijpeg.MijError, match="frame 0: "):
                            d1.transform(op, trim, None, 1)
                    else:
                        d1.transform(op, trim, None, 1)
                        assert d1.transcoded(0) == w, (n, op)
            finally:
                d1.close()
            continue
        dec.transform(op, trim, None, 1)
        for i, (n, w) in enumerate(zip(XF_FILES, want)):
            assert dec.transcoded(i) == w, (n, op, trim)


def test_transposition_maps_422_and_440(dec):
    f422, f440 = SC.jpg("422_35x21"), SC.jpg("440_21x35")
    dec.decode([f422, f440, SC.jpg("422_48x32")])
    dec.transform("transpose")
    outs = [dec.transcoded(i) for i in range(3)]
    # a transposed 4:4:0 is what the existing path writes for the equivalent 4:2:2 planes
    assert outs[1] == mijpeg.transcode(f422)
    assert outs[0] == mijpeg.transcode(f440, accept440=True)
    dec.decode(outs)
    assert dec.layout(0)["raw"][:5] == [21, 35, 3, 1, 2] and dec.layout(0)["comps"][0][:2] == (1, 2)
    assert dec.layout(1)["raw"][:5] == [35, 21, 3, 2, 1] and dec.layout(1)["comps"][0][:2] == (2, 1)
    assert dec.layout(2)["raw"][:7] == [32, 48, 3, 1, 2, 4, 3]
    dec.reconstruct("rgb")
    _check_pixels(dec, 0, SC.model("440_21x35"), "rgb")
    # four quarter turns through 4:4:0 and back, progressive output included
    turned = SC.jpg("422_48x32")
    for k in range(4):
        turned = mijpeg.transform(turned, "rot90", accept440=True, output="progressive" if k == 1 else "baseline",
                                  progressive=k == 2)
    assert turned == mijpeg.transcode(SC.jpg("422_48x32"))


def test_crop_on_the_8x16_grid(dec):
    j = SC.jpg("440_37x70_rstrow")
    dec.decode([j])
    for crop, op in (((8, 16, 29, 54), "none"), ((16, 32, 16, 32), "rot270"), ((0, 48, 37, 22), "flip_v")):
        dec.transform(op, True, crop, 1)
        assert dec.transcoded(0) == SM.model(j, op, True, crop, 1), (crop, op)
    with pytest.raises(mijpeg.MijError, match=r"crop offset \+8\+8 is not aligned to the 8x16 MCU"):
        dec.transform("none", False, (8, 8, 8, 8))


def test_auto_turns_a_portrait_422_upright():
    src = SC.jpg("422_48x32")
    spliced = src[:2] + XM.app1("II", 6) + src[2:]
    assert mijpeg.exif_orientation(spliced) == 6
    with pytest.raises(mijpeg.MijError, match="sampling 2x1"):
        mijpeg.transform(spliced, "auto")
    got = mijpeg.transform(spliced, "auto", accept440=True)
    assert got == mijpeg.transform(src, "rot90", accept440=True) == SM.model(src, "rot90")
    d = mijpeg.Decoder(48, 48, 1, accept440=True)
    try:
        d.decode([spliced])
        d.transform(mijpeg.orientation_op(mijpeg.exif_orientation(spliced)), trim=True)
        assert d.transcoded(0) == got
        d.decode([got])
        assert d.layout(0)["raw"][:5] == [32, 48, 3, 1, 2]
        for scale in (1, 2, 4, 8):
            d.reconstruct("rgb", scale)
            _check_pixels(d, 0, SM.scaled(got, scale), "rgb")
    finally:
        d.close()


# ---- 7. loader, thumbnail ----------------------------------------------------------------------
def test_loader_mixed_kinds():
    names = ("440_37x70_rstrow", "422_35x21", "p440_37x70_rstrow", "440_520x1040_q30")
    files = [SC.jpg(n) for n in names]
    sizes = [(SC.model(n).w, SC.model(n).h) if n != "422_35x21" else (35, 21) for n in names]
    crops = ((3, 5, 30, 61), (1, 3, 33, 17), (3, 5, 30, 61), (101, 53, 401, 801))
    mirror = (1, 0, 1, 1)
    l = mijpeg.Loader(528, 1040, 4, progressive=True, accept440=True)
    try:
        for scale in (0, 2):
            got = l.load(files, (32, 32), crops=crops, mirror=mirror, scale=scale)
            d = l.denom()
            assert d == (scale or TM.denom(sizes, crops, 32, 32))
            frames = []
            for j, (W, H), crop in zip(files, sizes, crops):
                px = SM.scaled(j, d).rgb
                x0, y0, x1, y1 = TM.rect(crop, W, H, d)
                frames.append(RM.resize(np.ascontiguousarray(px[y0:y1, x0:x1]), (32, 32), "bilinear"))
            ref = TM.tensorize(frames, mirror)
            assert got.shape == (4, 3, 32, 32) and got.dtype == np.float16
            assert got.tobytes() == ref.tobytes(), scale
            assert got[0].tobytes() == got[2].tobytes()  # the progressive twin
        l.accept(mijpeg.ACCEPT_PROGRESSIVE)
        with pytest.raises(mijpeg.MijError, match="luma sampling 1x2"):
            l.load(files, (32, 32))
        with pytest.raises(mijpeg.MijError, match="unknown bits"):
            l.accept(2)
    finally:
        l.close()


def test_thumbnail_keyword():
    j = SC.jpg("440_40x48_noise_q95")
    with pytest.raises(mijpeg.MijError, match="luma sampling 1x2"):
        mijpeg.thumbnail(j, (9, 11))
    small = RM.resize(SC.scaled("440_40x48_noise_q95", 4).bgr, (9, 11), "bicubic")
    assert mijpeg.thumbnail_denom(40, 48, 9, 11) == 4
    assert mijpeg.thumbnail(j, (9, 11), accept440=True) == mijpeg.encode_any(small, "bgr", 75)
    assert (mijpeg.thumbnail(j, (9, 11), "bicubic", 80, "libjpeg", "422", accept440=True) ==
            mijpeg.encode_libjpeg(small, "bgr", 80, sampling="422"))


# ---- 8. refusal hygiene ----------------------------------------------------------------------
def test_a_refused_frame_leaves_nothing_served(dec):
    good, m = SC.jpg("440_21x35"), SC.model("440_21x35")
    dec.decode([good])
    for bad in (SC.with_luma_hv(good, 0x41), good[:len(good) // 2], SC.jpg("p440_21x35")):
        with pytest.raises(mijpeg.MijError):
            dec.decode([good, bad])
        for call in (lambda: dec.layout(0), lambda: dec.reconstruct("rgb"), lambda: dec.transcode(),
                     lambda: dec.transform("rot90")):
            with pytest.raises(mijpeg.MijError):
                call()
    dec.decode([good])
    _check_frame(dec, 0, m)
    dec.reconstruct("rgb")
    _check_pixels(dec, 0, m, "rgb")
    dec.transform("rot90", trim=True)
    assert dec.transcoded(0) == SM.model(good, "rot90", True)


def test_host_tools_440_option(tmp_path):
    """host/decode_jpg --440 (full size and -scale 1/2), transcode_jpg --440 -rotate 90 of a 4:2:2 file,
    thumbnail_jpg --440; without the option each refuses"""
    import subprocess

    import ppm
    host = os.path.join(os.path.dirname(mijpeg.LIB_PATH), "host")
    src, m = os.path.join(SC.DIR, "440_37x70_rstrow.jpg"), SC.model("440_37x70_rstrow")
    out = str(tmp_path / "out.ppm")
    subprocess.run([os.path.join(host, "decode_jpg"), "--440", src, out], check=True, timeout=120)
    with open(out, "rb") as f:
        assert f.read() == ppm.ppm_bytes(m.rgb)
    subprocess.run([os.path.join(host, "decode_jpg"), "--440", "-scale", "1/2", src, out], check=True, timeout=120)
    with open(out, "rb") as f:
        assert f.read() == ppm.ppm_bytes(SC.scaled("440_37x70_rstrow", 2).rgb)
    r = subprocess.run([os.path.join(host, "decode_jpg"), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "luma sampling 1x2" in r.stderr
    jpg, s422 = str(tmp_path / "out.jpg"), os.path.join(SC.DIR, "422_48x32.jpg")
    subprocess.run([os.path.join(host, "transcode_jpg"), "--440", "-rotate", "90", s422, jpg, "1"], check=True, timeout=120)
    with open(jpg, "rb") as f:
        assert f.read() == SM.model(SC.jpg("422_48x32"), "rot90", restart_rows=1)
    r = subprocess.run([os.path.join(host, "transcode_jpg"), "-rotate", "90", s422, jpg], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "sampling 2x1" in r.stderr
    subprocess.run([os.path.join(host, "thumbnail_jpg"), "--440", "9x17", src, jpg], check=True, timeout=120)
    with open(jpg, "rb") as f:
        assert f.read() == mijpeg.thumbnail(SC.jpg("440_37x70_rstrow"), (9, 17), accept440=True)
    r = subprocess.run([os.path.join(host, "thumbnail_jpg"), "9x17", src, jpg], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "luma sampling 1x2" in r.stderr
