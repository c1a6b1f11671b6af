"""The numpy model of the lossless transforms (transform_model.py, DESIGN.md
§4i) pinned to independent code, on the CPU: the float IDCT of every
transformed plane is the geometrically transformed float IDCT of the source
plane; algebraic identities on the model's bytes; Pillow opens the outputs;
the shared mapping header csrc/mij_xform.h, compiled for the host, gives the
model's permutation.  And what the library decides without a device: EXIF
orientation and every refusal of mij_transform."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import decode_model as M
import foreign_cases as FC
import mijpeg
import transcode_model as TM
import transform_model as XM
from transform_model import app1, spliced

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(mijpeg.LIB_PATH)
ACCEPTED = [n for n in FC.NAMES if not n.startswith("reject")]
SMALL = [n for n in ACCEPTED if "1040" not in n]

# numpy's own geometry, by name: rot90 is clockwise
GEOMETRY = {"none": lambda a: a, "flip_h": np.fliplr, "flip_v": np.flipud, "transpose": lambda a: a.T,
            "transverse": lambda a: np.rot90(a, 2).T, "rot90": lambda a: np.rot90(a, -1),
            "rot180": lambda a: np.rot90(a, 2), "rot270": lambda a: np.rot90(a, 1)}

# the orthonormal DCT-II matrix: samples = A.T @ coefficients @ A
_k = np.arange(8)
A = np.sqrt(2 / 8) * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)
A[0] /= np.sqrt(2)


def float_idct(blocks, q):
    """(bh, bw, 64) zigzag coefficients, 64 zigzag quantisers -> (8 bh, 8 bw) float samples"""
    bh, bw = blocks.shape[:2]
    nat = np.zeros(blocks.shape, np.float64)
    nat[:, :, M.ZZ] = blocks * np.asarray(q, np.float64)
    px = np.einsum("vy,rcvu,ux->rcyx", A, nat.reshape(bh, bw, 8, 8), A)
    return px.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def expect_refusal(name, op):
    """with TRIM and no crop: a 4:2:2 file under transposition, and a mirrored dimension under one MCU"""
    P, G, _ = XM.source(FC.jpg(name))
    t, fh, fv = XM.PARTS[op]
    if t and any(c[0] != c[1] for c in G["comps"]):
        return True
    mir_h, mir_v = (fv, fh) if t else (fh, fv)
    return bool((mir_h and P["w"] < 8 * G["hmax"]) or (mir_v and P["h"] < 8 * G["vmax"]))


@pytest.mark.parametrize("name", SMALL)
def test_float_idct_of_the_transformed_planes(name):
    jpg = FC.jpg(name)
    P, G, planes = XM.source(jpg)
    mw, mh = 8 * G["hmax"], 8 * G["vmax"]
    done = 0
    for op in XM.OPS:
        if expect_refusal(name, op):
            with pytest.raises(XM.Refused):
                XM.parts(jpg, op, True)
            continue
        w, h, comps, hv, dqt, out = XM.parts(jpg, op, True)
        x, y, kw, kh = XM.kept(P["w"], P["h"], mw, mh, op, True)
        assert (x, y) == (0, 0) and (w, h) == ((kh, kw) if XM.PARTS[op][0] else (kw, kh))
        mx, my = -(-w // (8 * max(a for a, _ in hv))), -(-h // (8 * max(b for _, b in hv)))
        for c, (a, b) in enumerate(hv):
            sa, sb = G["comps"][c][0], G["comps"][c][1]
            src = planes[c].reshape(G["mcus_y"] * sb, G["mcus_x"] * sa, 64)
            src = src[:-(-kh // mh) * sb, :-(-kw // mw) * sa]  # the trimmed source plane
            want = GEOMETRY[op](float_idct(src, P["dqt"][comps[c][2]]))
            got = float_idct(out[c].reshape(my * b, mx * a, 64), dqt[comps[c][2]])
            assert got.shape == want.shape, (op, c)
            worst = float(np.abs(got - want).max())
            assert worst <= 1e-9, (op, c, worst)  # measured 2.3e-13; a wrong sign or index shows as >= 1
        done += 1
    assert done >= 2  # none and transpose at the least, or none and the flips for 4:2:2


def test_identities_on_the_models_bytes():
    j = FC.jpg("444_40x24")
    plain = TM.model(j, 0)
    assert XM.model(j, "none") == plain
    assert XM.model(XM.model(j, "flip_h"), "flip_h") == plain
    r = j
    for _ in range(4):
        r = XM.model(r, "rot90")
    assert r == plain
    assert XM.model(XM.model(j, "rot90"), "rot270") == plain
    assert XM.model(XM.model(j, "transpose"), "flip_h") == XM.model(j, "rot90")  # flip_h o transpose
    assert XM.model(j, "none", restart_rows=1) == TM.model(j, 1)


def test_pillow_opens_every_output():
    Image = pytest.importorskip("PIL.Image")
    for name in SMALL:
        jpg = FC.jpg(name)
        for op in XM.OPS:
            if expect_refusal(name, op):
                continue
            w, h = XM.parts(jpg, op, True)[:2]
            im = Image.open(io.BytesIO(XM.model(jpg, op, True, None, 1)))
            im.load()
            assert im.size == (w, h), (name, op)
    # whole-MCU 4:4:4: libjpeg's pixels of the flipped file are its flipped pixels of the source
    j = FC.jpg("444_24x24_noise_q100")
    src = np.asarray(Image.open(io.BytesIO(j)).convert("RGB"))
    for op in ("flip_h", "flip_v", "rot180"):
        got = np.asarray(Image.open(io.BytesIO(XM.model(j, op))).convert("RGB"))
        assert (got == np.stack([GEOMETRY[op](src[:, :, k]) for k in range(3)], -1)).all(), op


# ---- the shared mapping header on the host -----------------------------------------
@pytest.fixture(scope="module")
def xform_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xform_check") / "xform_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "xform_check.cpp")])
    return exe


# source plane (blocks across, down), the kept part's offset and size in blocks
@pytest.mark.parametrize("sbw,sbh,ox,oy,kw,kh,ops", [
    (1, 1, 0, 0, 1, 1, XM.OPS),            # one block
    (6, 4, 2, 2, 4, 2, XM.OPS),            # the 2x2 component of 3 x 2 MCUs, cropped by one MCU each way
    (3, 2, 1, 1, 2, 1, XM.OPS),            # its 1x1 components
    (6, 2, 2, 0, 4, 2, XM.OPS[:3] + XM.OPS[6:7]),  # a 2x1 component: not transposed
])
def test_mapping_header_equals_model(xform_check, sbw, sbh, ox, oy, kw, kh, ops):
    for op in ops:
        t = XM.PARTS[op][0]
        dbw, dbh = (kh, kw) if t else (kw, kh)
        out = subprocess.check_output([xform_check] + [str(v) for v in (sbw, ox, oy, dbw, dbh, XM.OPS.index(op))])
        got = np.array(out.split(), np.int64).reshape(-1, 64, 3)
        want = XM.mapping(sbw, sbh, ox, oy, kw, kh, op)
        assert got.shape == want.shape and (got == want).all(), op
        assert (got[:, 0, 1:] == [0, 1]).all()  # the DC stays the DC and keeps its sign


# ---- EXIF orientation (host only) ----------------------------------------------------
def test_exif_orientation():
    assert mijpeg.exif_orientation(FC.jpg("420_35x21")) == 1  # none
    for order in ("II", "MM"):
        for n in range(1, 9):
            assert mijpeg.exif_orientation(spliced("420_35x21", app1(order, n))) == n, (order, n)
        assert mijpeg.exif_orientation(spliced("420_35x21", app1(order, 0))) == 1
        assert mijpeg.exif_orientation(spliced("420_35x21", app1(order, 9))) == 1
        assert mijpeg.exif_orientation(spliced("420_35x21", app1(order, 6, tag=0x0113))) == 1
        # truncated: the segment ends inside the entry / inside the TIFF header
        for cut in (5, 8, 14, 20):
            assert mijpeg.exif_orientation(spliced("420_35x21", app1(order, 6, cut=cut))) == 1, (order, cut)
        # IFD0 announced past the segment's end
        for ifd in (22, 26, 0x1000, 0xFFFFFFF0):
            assert mijpeg.exif_orientation(spliced("420_35x21", app1(order, 6, ifd=ifd))) == 1, (order, ifd)
    # a segment that runs past the file
    seg = app1("II", 6)
    assert mijpeg.exif_orientation(b"\xff\xd8" + seg[:-3]) == 1
    assert mijpeg.exif_orientation(b"") == 1 and mijpeg.exif_orientation(b"\xff\xd8\xff") == 1
    # an APP1 of another kind in front does not hide it
    other = b"\xff\xe1\x00\x08http:/"
    assert mijpeg.exif_orientation(spliced("444_17x9", other + app1("MM", 8))) == 8
    want = ["none", "flip_h", "rot180", "flip_v", "transpose", "rot90", "transverse", "rot270"]
    assert [mijpeg.orientation_op(n) for n in range(1, 9)] == want
    assert mijpeg.orientation_op(0) == mijpeg.orientation_op(9) == mijpeg.orientation_op(-1) == "none"


# ---- refusals: decided from the markers, no device -------------------------------------
def refused(name, op, flags=0, crop=None, rr=0):
    lib = mijpeg.load()
    j = np.frombuffer(FC.jpg(name), np.uint8)
    n = C.c_size_t(0)
    area = C.byref(mijpeg.Area(*crop)) if crop else None
    rc = lib.mij_transform(j.ctypes.data, j.size, op, flags, area, rr, None, 0, C.byref(n))
    return rc, lib.mij_last_message().decode()


def test_refusals_need_no_device():
    FLIP_H, ROT90, TRIM = 1, 5, 1
    rc, msg = refused("420_35x21", FLIP_H)
    assert rc == 1 and "frame 0" in msg and "width 35" in msg
    rc, msg = refused("422_35x21", ROT90, TRIM)
    assert rc == 1 and "frame 0" in msg and "sampling 2x1" in msg
    rc, msg = refused("420_1x1", FLIP_H, TRIM)
    assert rc == 1 and "nothing left" in msg
    rc, msg = refused("420_35x21", 0, 0, (8, 0, 16, 16))
    assert rc == 1 and "aligned" in msg
    rc, msg = refused("420_35x21", 0, 0, (0, 16, 16, 6))  # 16 + 6 > 21
    assert rc == 1 and "outside" in msg
    rc, msg = refused("420_35x21", 0, 0, (16, 0, 0, 5))
    assert rc == 1 and "empty" in msg
    rc, msg = refused("420_35x21", 8)
    assert rc == 1 and "operation 8" in msg
    rc, msg = refused("420_35x21", -1)
    assert rc == 1 and "operation" in msg
    rc, msg = refused("420_35x21", 0, 2)
    assert rc == 1 and "flag" in msg
    rc, msg = refused("420_35x21", 0, 0, None, -1)
    assert rc == 1 and "restart" in msg
    rc, msg = refused("420_35x21", 3, 0, None, 32768)  # 32768 rows x 2 MCUs of the transposed grid
    assert rc == 1 and "restart" in msg and "65536" in msg
    # the model refuses the same
    for args in (("flip_h",), ("flip_h", True)):
        with pytest.raises(XM.Refused):
            XM.parts(FC.jpg("420_1x1"), *args)
    with pytest.raises(XM.Refused):
        XM.parts(FC.jpg("422_35x21"), "rot90", True)
    with pytest.raises(XM.Refused):
        XM.parts(FC.jpg("420_35x21"), "none", False, (8, 0, 16, 16))


def test_host_tool_compiles(tmp_path):
    """host/transcode_jpg.c with its transform options against the public
    header, warning-free, and linked (nothing is run: no GPU here)"""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"),
                           os.path.join(PKG, "host", "transcode_jpg.c"), "-L", PKG, "-lmijpeg",
                           "-o", str(tmp_path / "transcode_jpg")])
