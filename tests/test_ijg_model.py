"""Encoding as libjpeg does, without a GPU: the numpy model
(ijg_model.py) against Pillow's libjpeg-turbo where it is installed -- the
DQTs, every coefficient of every plane (dummy blocks included) of Pillow's
own save(quality, subsampling, optimize=True), and the pixels Pillow decodes
from the model's stream -- and always against the digests of
tests/golden/ijg/manifest.json, which scripts/gen_ijg_golden.py writes only
when Pillow agreed; the C++ the kernel runs (csrc/mij_ijg_math.h) on the
host through ijg_check.cpp; the refusals of the new calls that need no
device.  The GPU side is tests/test_ijg_gpu.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import foreign_cases as FC
import foreign_model as FM
import ijg_cases as IC
import ijg_model as J
import mijpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "jpeg-encoder-decoder_amd")
GROUPS = IC.groups()


@pytest.fixture(scope="module")
def ijg_manifest():
    with open(os.path.join(REPO, "tests", "golden", "ijg", "manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("key", sorted(GROUPS))
def test_model_equals_pillow(key):
    if not IC.have_pillow():
        pytest.skip("Pillow with libjpeg-turbo not installed")
    s, cases = GROUPS[key]
    for name, f, q in cases:
        bad = IC.agrees_with_pillow(f, q, s)
        assert bad is None, (key, name, bad)


@pytest.mark.parametrize("key", sorted(GROUPS))
def test_model_equals_manifest(key, ijg_manifest):
    s, cases = GROUPS[key]
    assert IC.digests(s, cases) == ijg_manifest[key]


def test_manifest_is_whole(ijg_manifest):
    assert sorted(ijg_manifest) == sorted(GROUPS)


def test_extremes():
    """flat 0 puts -1024 into the DC at Q = 100, and nothing goes past 1024 in magnitude"""
    for s in IC.SAMPLINGS:
        for name, f, q in IC.special_group(s):
            m = J.model(f, q, 0, s)
            for p in m.planes:
                assert np.abs(p).max() <= 1024
            if name == "flat0_q100":
                assert (m.planes[0][:, 0] == -1024).all()
            if name == "checker_q100":
                assert np.abs(m.planes[0][:, 1:]).max() > 800  # (7, 7): about 837


def test_stream_reads_back():
    """the plain Python decoder reads the model's stream back to the layout, tables and planes that went in"""
    for s in IC.SAMPLINGS:
        m = J.model(IC.frame("photo", 40, 24, seed=3), 75, 1, s)
        d = FM.decoded(m.jpg)
        assert d.layout == m.layout
        for c in range(m.G["ncomp"]):
            assert (d.dqt[c] == m.dqt[c]).all()
            assert (d.coefs[c] == m.planes[c]).all()


def test_bottom_edge_rule():
    """40 x 24 at 4:2:0: chroma rows 12..15 of the second chroma block row are
    chroma row 11 again, not the downsample of pixel row 23 with itself"""
    f = IC.frame("noise", 40, 24, seed=1)
    cb = J.samples(f, "420")[1]
    assert cb.shape == (16, 24)
    assert (cb[12:] == cb[11:12]).all()
    # ... and the luma dummy row carries DCs only
    Y = J.planes(f, 75, "420")[0].reshape(4, 6, 64)
    assert (Y[3, :, 1:] == 0).all() and (Y[3, 0::2, 0] == Y[2, 1::2, 0]).all() and (Y[3, 1::2, 0] == Y[2, 1::2, 0]).all()
    assert (Y[:3, 5, 1:] == 0).all() and (Y[:3, 5, 0] == Y[:3, 4, 0]).all()


@pytest.fixture(scope="module")
def ijg_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ijg_check") / "ijg_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "ijg_check.cpp")])
    return exe


def test_kernel_arithmetic_on_the_host(ijg_check, tmp_path):
    """csrc/mij_ijg_math.h (what k_ijg_fdct calls), compiled for the host:
    colour, downsamplers, quantiser and table scaling exhaustively, the DCT
    and quantiser on the model's blocks, every intermediate inside int32"""
    blocks = []
    cases = [(IC.frame(k, 16, 16), q) for k in IC.SPECIAL for q in (100, 1)] + \
            [(IC.frame(k, 35, 21, seed=q), q) for k in IC.KINDS for q in IC.QUALITIES]
    rng = np.random.default_rng(5)
    ext = rng.choice(np.array([0, 255], np.uint8), (24, 24, 3))  # 0 / 255 in every pattern a seed gives
    cases.append((ext, 100))
    for f, q in cases:
        tabs = J.quality_tables(q)
        for c, s in enumerate(J.samples(f, "444")):
            b = J.blocks_of(s)
            want = J.quantise(J.fdct(b).reshape(-1, 64), tabs[1 if c else 0])
            for i in range(len(b)):
                blocks.append(np.concatenate([b[i].reshape(64), tabs[1 if c else 0], want[i]]))
    src = tmp_path / "in.bin"
    with open(src, "wb") as fh:
        for q in range(1, 101):
            lq, cq = J.quality_tables(q)
            fh.write(np.concatenate([lq, cq]).astype(np.int32).tobytes())
        fh.write(np.array([len(blocks)], np.int32).tobytes())
        fh.write(np.stack(blocks).astype(np.int32).tobytes())
    r = subprocess.run([ijg_check, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    peak = int(r.stdout.split()[1])
    assert 0 < peak < 3 << 29  # DESIGN.md §4n's bound, 1.5 * 2^30


def test_tables_call():
    for q in (1, 25, 50, 75, 100):
        assert mijpeg.libjpeg_tables(q).tobytes() == J.dqt_bytes(q)
    lib = mijpeg.load()
    out = np.zeros(128, np.uint8)
    for q in (0, 101, -3):
        assert lib.mij_libjpeg_tables(q, out.ctypes.data) == 1 and "quality" in lib.mij_last_message().decode()
    assert lib.mij_libjpeg_tables(50, None) == 1


def _encode_rc(w, h, order, q, s, rr, cap, stride=None):
    lib = mijpeg.load()
    px = np.zeros((max(h, 1), max(w, 1), 3), np.uint8)
    out = np.zeros(16, np.uint8)
    n = C.c_size_t(0)
    rc = lib.mij_encode_libjpeg(px.ctypes.data, w if stride is None else stride, w, h, order, q, s, rr,
                                out.ctypes.data, cap, C.byref(n))
    return rc, n.value, lib.mij_last_message().decode()


def test_encode_refusals_come_before_any_device_work():
    for s in range(4):
        name = ("420", "422", "444", "gray")[s]
        rc, n, msg = _encode_rc(35, 21, 0, 75, s, 2, 0)
        assert rc == 4 and n == mijpeg.max_jpg_bytes_sampled(35, 21, name, 2) and str(n) in msg  # MIJ_ENOSPC
    for s in (-1, 4):
        rc, _, msg = _encode_rc(35, 21, 0, 75, s, 0, 0)
        assert rc == 1 and "sampling" in msg
    for w, h in ((0, 21), (35, 0), (65536, 21), (35, 65536)):
        rc, _, msg = _encode_rc(w, h, 0, 75, 2, 0, 0)
        assert rc == 1 and "1..65535" in msg
    for q in (0, 101):
        rc, _, msg = _encode_rc(35, 21, 0, q, 2, 0, 0)
        assert rc == 1 and "quality" in msg
    assert _encode_rc(35, 21, 2, 75, 2, 0, 0)[0] == 1
    assert _encode_rc(35, 21, 0, 75, 2, -1, 0)[0] == 1
    rc, _, msg = _encode_rc(35, 21, 0, 75, 2, 13108, 0)  # Ri = 13108 * 5 > 65535
    assert rc == 1 and "over 65535" in msg
    with pytest.raises(ValueError, match="sampling"):
        mijpeg.encode_libjpeg(np.zeros((4, 4, 3), np.uint8), sampling="411")


def _thumbnail_rc(jpg, ow, oh, f, q, s, cap):
    lib = mijpeg.load()
    buf = np.frombuffer(jpg, np.uint8)
    out = np.zeros(16, np.uint8)
    n = C.c_size_t(0)
    rc = lib.mij_thumbnail_libjpeg(buf.ctypes.data, buf.size, ow, oh, f, q, s, out.ctypes.data, cap, C.byref(n))
    return rc, n.value, lib.mij_last_message().decode()


def test_thumbnail_refusals_come_before_any_device_work():
    jpg = FC.jpg("420_96x80_noise_q95")
    for s, name in enumerate(("420", "422", "444", "gray")):
        rc, n, msg = _thumbnail_rc(jpg, 20, 17, 2, 75, s, 0)
        assert rc == 4 and n == mijpeg.max_jpg_bytes_sampled(20, 17, name, 0) and str(n) in msg
    assert _thumbnail_rc(jpg, 20, 17, 5, 75, 0, 0)[0] == 1
    rc, _, msg = _thumbnail_rc(jpg, 0, 17, 2, 75, 0, 0)
    assert rc == 1 and "1..65535" in msg
    rc, _, msg = _thumbnail_rc(jpg, 20, 17, 2, 0, 0, 0)
    assert rc == 1 and "quality" in msg
    for s in (-1, 4):
        rc, _, msg = _thumbnail_rc(jpg, 20, 17, 2, 75, s, 0)
        assert rc == 1 and "sampling" in msg
    # what mij_decode refuses, with its message
    rc, _, msg = _thumbnail_rc(FC.jpg("reject_progressive"), 20, 17, 2, 75, 0, 0)
    assert rc == 8 and "baseline" in msg.lower(), (rc, msg)  # MIJ_EJPEG
    with pytest.raises(mijpeg.MijError, match="baseline"):
        mijpeg.thumbnail(FC.jpg("reject_progressive"), (20, 17), arithmetic="libjpeg", sampling="444")
    # the reference's arithmetic writes 4:2:0 only
    for s in ("422", "444", "gray"):
        with pytest.raises(ValueError, match="libjpeg"):
            mijpeg.thumbnail(jpg, (20, 17), sampling=s)
    with pytest.raises(ValueError):
        mijpeg.thumbnail(jpg, (20, 17), sampling="411", arithmetic="libjpeg")
