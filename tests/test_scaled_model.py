"""Decoding at 1/2, 1/4 and 1/8 scale without a GPU.

The chain: Pillow's libjpeg-turbo draft decode == the numpy model
(scaled_model.py) == the committed digests (tests/golden/scaled_pixels.json,
for machines without Pillow) == the kernels' own arithmetic
(csrc/mij_pixels.h) run on the host.  The GPU side is
tests/test_scaled_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foreign_cases as FC
import foreign_model as F
import mijpeg
import scaled_cases as SC
import scaled_model as SM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "jpeg-encoder-decoder_amd")

# a file of each layout whose size is not whole MCUs: compared with Pillow at every scale or the test fails
ODD = ("grey_35x21", "444_17x9", "422_35x21", "420_35x21")


def test_model_equals_libjpeg():
    """every committed fixture and 15 files made here, at 1/2, 1/4, 1/8, where
    Pillow took the requested scale"""
    Image = SC.pillow()
    if Image is None:
        pytest.skip("Pillow with libjpeg-turbo not installed")
    files = [(n, FC.jpg(n)) for n in FC.NAMES]
    files += [(n, SC.generated_jpg(Image, w, h, ss)) for n, w, h, ss in SC.GENERATED]
    assert len(files) == 35
    compared, skipped = set(), 0
    for name, jpg in files:
        m = F.decoded(jpg)
        for denom in SC.DENOMS:
            ref = SC.pillow_draft(Image, jpg, denom)
            if ref is None:
                skipped += 1
                continue
            s = SM.scaled(m, denom)
            assert ref.shape == s.rgb.shape, (name, denom, ref.shape, s.rgb.shape)
            assert (ref == s.rgb).all(), (name, denom, int((ref != s.rgb).any(-1).sum()))
            compared.add((name, denom))
    assert 4 * skipped <= 3 * len(files), skipped
    for name in ODD:
        for denom in SC.DENOMS:
            assert (name, denom) in compared, (name, denom)


@pytest.mark.parametrize("name", FC.NAMES)
def test_model_equals_committed_digests(name):
    want = SC.committed_digests()[name]
    for denom in SC.DENOMS:
        s = SC.model(name, denom)
        assert SC.digests(s) == want[str(denom)], denom
        assert (s.bgr == s.rgb[..., ::-1]).all()
        m = FC.model(name)
        assert (s.ow, s.oh) == (-(-m.w // denom), -(-m.h // denom))


def test_geometry_is_what_the_layouts_call_for():
    """IDCT sizes, what is left of upsampling, and the switch points"""
    for denom, s in ((2, 4), (4, 2), (8, 1)):
        assert [c[0] for c in SC.model("grey_35x21", denom).comps] == [s]
        assert [c[0] for c in SC.model("444_17x9", denom).comps] == [s] * 3
        assert [c[0] for c in SC.model("422_35x21", denom).comps] == [s] * 3
        assert [c[0] for c in SC.model("420_35x21", denom).comps] == [s, 2 * s, 2 * s]  # chroma scaled up in the IDCT
        assert SC.model("420_35x21", denom).mode == SM.PIX_444
        assert SC.model("444_17x9", denom).mode == SM.PIX_444 and SC.model("grey_35x21", denom).mode == SM.PIX_GREY
    # 4:2:2: fancy upsampling only for a chroma width > 2 and an IDCT size > 1
    assert [SC.model("422_35x21", d).mode for d in SC.DENOMS] == [SM.PIX_H2V1, SM.PIX_H2V1, SM.PIX_H2V1_REP]
    assert SC.model("422_5x8", 2).comps[1][1] == 2 and SC.model("422_5x8", 2).mode == SM.PIX_H2V1_REP
    assert SC.model("422_35x21", 4).comps[1][1:3] == (5, 6) and SC.model("422_35x21", 4).layout[:3] == [9, 6, 3]
    # planes: rows 8 bytes apart at least, S * blocks across rounded up
    assert SC.model("444_17x9", 4).comps[0] == (2, 5, 3, 8, 4)
    assert SC.model("420_1040x520_q30", 8).comps[0] == (1, 130, 65, 136, 66)


def test_eighth_scale_is_the_dc_alone():
    m = FC.model("grey_35x21")
    s = SC.model("grey_35x21", 8)
    bw, bh = m.G["comps"][0][3:5]
    dc = m.coefs[0].astype(np.int64)[:, 0] * int(m.dqt[0][0])
    want = np.clip(((dc + 4) >> 3) + 128, 0, 255).reshape(bh, bw)
    assert (s.planes[0][:, :bw] == want).all() and (s.planes[0][:, bw:] == 0).all()
    assert len(np.unique(want)) > 4


@pytest.mark.parametrize("name", FC.NAMES)
def test_integer_idcts_stay_within_one_of_the_float_idct(name):
    """the ISO 10918-2 style bound DESIGN.md §4e uses for the 8x8 IDCT, on
    the 4x4 and 2x2 forms: no sample further than 1 from the float64 result"""
    m = FC.model(name)
    seen = set()
    for denom in SC.DENOMS:
        for (S, *_), cf, q in zip(SC.model(name, denom).comps, m.coefs, m.dqt):
            if S in (4, 2):
                err = np.abs(SM.idct_blocks(cf, q, S).astype(np.float64) - SM.idct_float(cf, q, S)).max()
                assert err <= 1.0, (denom, S, err)
                seen.add(S)
    assert seen == {4, 2}


@pytest.fixture(scope="module")
def scaled_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scaled_check") / "scaled_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "scaled_check.cpp")])
    return exe


@pytest.mark.parametrize("name", FC.SMALL)
def test_kernel_arithmetic_on_the_host_equals_model(name, scaled_check, tmp_path):
    """scaled_geometry, the block IDCTs of every size and colour_tile_any on
    the scaled planes (what k_dec_idct<S> and k_dec_colour call), compiled for the host"""
    m = FC.model(name)
    for denom in SC.DENOMS:
        s = SC.model(name, denom)
        src, dst = tmp_path / f"in{denom}.bin", tmp_path / f"out{denom}.bin"
        with open(src, "wb") as f:
            f.write(np.array([m.w, m.h, m.G["ncomp"], denom], np.int32).tobytes())
            for c, comp in enumerate(m.G["comps"]):
                f.write(np.array([comp[0], comp[1], comp[3], comp[4]], np.int32).tobytes())
                f.write(m.dqt[c].astype(np.int32).tobytes())
            for a in m.coefs:
                f.write(np.ascontiguousarray(a, np.int16).tobytes())
        subprocess.check_call([scaled_check, str(src), str(dst)])
        got = np.fromfile(dst, np.uint8)
        nl = 4 * len(s.layout)
        assert got[:nl].view(np.int32).tolist() == s.layout, denom
        planes = np.concatenate([p.ravel() for p in s.planes])
        n = planes.size
        assert (got[nl:nl + n] == planes).all(), denom
        px = 3 * s.ow * s.oh
        assert got.size == nl + n + 2 * px
        assert (got[nl + n:nl + n + px] == s.rgb.ravel()).all(), (name, denom)
        assert (got[nl + n + px:] == s.bgr.ravel()).all(), (name, denom)


def _decode_scaled(jpg: bytes, denom: int, cap: int = 0):
    lib = mijpeg.load()
    buf = np.frombuffer(jpg, np.uint8)
    probe = np.zeros(1, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    rc = lib.mij_decode_scaled(buf.ctypes.data, buf.size, 1, denom, probe.ctypes.data, cap, C.byref(w), C.byref(h))
    return rc, w.value, h.value, lib.mij_last_message().decode()


@pytest.mark.parametrize("name", FC.NAMES)
def test_decode_scaled_reports_the_scaled_size_without_a_device(name):
    for denom in SC.DENOMS:
        s = SC.model(name, denom)
        rc, w, h, msg = _decode_scaled(FC.jpg(name), denom)
        assert (rc, w, h) == (4, s.ow, s.oh) and str(3 * s.ow * s.oh) in msg, (rc, msg)  # MIJ_ENOSPC


def test_decode_scaled_refusals_without_a_device():
    for denom in (0, 3, 16, -2):
        rc, _, _, msg = _decode_scaled(FC.jpg("420_35x21"), denom)
        assert rc == 1 and "scale" in msg, (denom, rc, msg)  # MIJ_EINVAL
    rc, _, _, msg = _decode_scaled(FC.jpg("reject_progressive"), 4)
    assert rc == 8 and "baseline" in msg.lower(), (rc, msg)  # MIJ_EJPEG
