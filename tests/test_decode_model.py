"""The decoder's pixel path without a GPU (DESIGN.md "Decode to pixels").

The chain: libjpeg (Pillow's libjpeg-turbo) == the numpy model
(decode_model.py) on the oracle's coefficients == the committed digests
(tests/golden/decode_pixels.json, for machines without Pillow) == the
kernels' own arithmetic (csrc/mij_pixels.h) run on the host; and the model
stays within 1 of the float64 IDCT, ISO/IEC 10918-2's accuracy bound.  The
GPU side of the chain is tests/test_pixels.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decode_cases as DC
import decode_model as M
import mijpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "jpeg-encoder-decoder_amd")


# checkerboards_q100 is left out on purpose: that stream ends its luma scan
# with an unstuffed FF, which libjpeg takes for marker fill (DESIGN.md
# "Decode to pixels", the unstuffed-FF caveat); test_pixels.py covers it
# against the coefficients
@pytest.mark.parametrize("name", DC.LIBJPEG_CASES)
def test_model_equals_libjpeg(name):
    c = DC.case(name)
    ref = DC.libjpeg_pixels(c.jpg)
    if ref is None:
        pytest.skip("Pillow with libjpeg-turbo not installed")
    rgb, y = ref
    assert (y == c.planes[0]).all(), int((y != c.planes[0]).sum())
    assert (rgb == c.rgb).all(), int((rgb != c.rgb).sum())


@pytest.mark.parametrize("name", DC.LIBJPEG_CASES)
def test_model_equals_committed_digests(name):
    assert DC.case(name).digests() == DC.committed_digests()[name]


def test_digest_file_lists_exactly_the_libjpeg_cases():
    assert sorted(DC.committed_digests()) == sorted(DC.LIBJPEG_CASES)


def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    c = np.cos((2 * n + 1) * k * np.pi / 16) / 2
    c[0] /= np.sqrt(2)
    return c  # c[k, n]: forward DCT is c @ x @ c.T


@pytest.mark.parametrize("name", DC.LIBJPEG_CASES)
def test_model_within_one_of_float64_idct(name):
    """ISO/IEC 10918-2: no sample further than 1 from the ideal IDCT"""
    c = DC.case(name)
    cm = _dct_matrix()
    for comp, (coefs, plane) in enumerate(zip(c.coefs, c.planes)):
        d = M.dequant(coefs, c.dqt[comp != 0]).astype(np.float64)
        x = np.einsum("ki,bkl,lj->bij", cm, d, cm)
        h, w = plane.shape
        ideal = np.clip(np.rint(x + 128), 0, 255).reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w)
        worst = int(np.abs(ideal - plane.astype(np.int64)).max())
        assert worst <= 1, (comp, worst)


@pytest.fixture(scope="module")
def pixels_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pixels_check") / "pixels_check")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "pixels_check.cpp")])
    return exe


@pytest.mark.parametrize("name", ["noise_16x16_q50", "noise_16x48_q50", "noise_48x16_q50", "sample_64x64",
                                  "checkerboards_q100", "noise_q100", "near_gray_q10", "config3_496x272_q50"])
def test_kernel_arithmetic_on_the_host_equals_model(name, pixels_check, tmp_path):
    """csrc/mij_pixels.h (what k_dec_idct and k_dec_colour call), compiled
    for the host and driven tile by tile as the kernels drive it"""
    c = DC.case(name)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([c.w, c.h], np.int32).tobytes())
        for q in c.dqt:
            f.write(q.astype(np.int32).tobytes())
        for a in c.coefs:
            f.write(np.ascontiguousarray(a, np.int16).tobytes())
    subprocess.check_call([pixels_check, str(src), str(dst)])
    got = np.fromfile(dst, np.uint8)
    n = c.w * c.h
    assert (got[:n * 3 // 2] == np.concatenate([p.ravel() for p in c.planes])).all()
    assert (got[n * 3 // 2:n * 9 // 2] == c.rgb.ravel()).all()
    assert (got[n * 9 // 2:] == c.bgr.ravel()).all()


def test_decode_validates_before_device_use():
    lib = mijpeg.load()
    jpg = np.frombuffer(DC.case("sample_64x64").jpg, np.uint8)
    out = np.zeros(64 * 64 * 3, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    assert lib.mij_decode(jpg.ctypes.data, jpg.size, 0, None, out.size, C.byref(w), C.byref(h)) == 1  # MIJ_EINVAL
    assert b"NULL" in lib.mij_last_message()
    for order in (-1, 2):
        assert lib.mij_decode(jpg.ctypes.data, jpg.size, order, out.ctypes.data, out.size, None, None) == 1
        assert lib.mij_last_error() == 1 and b"order" in lib.mij_last_message()
    # the size is reported, and a short cap refused, from the headers alone
    assert lib.mij_decode(jpg.ctypes.data, jpg.size, 1, out.ctypes.data, out.size - 1, C.byref(w), C.byref(h)) == 4
    assert (w.value, h.value) == (64, 64) and b"12288" in lib.mij_last_message()
    assert lib.mij_decoder_reconstruct(None, 0) == 1 and lib.mij_decoder_pixels(None, 0, out.ctypes.data, 1, 0) == 1
    with pytest.raises(mijpeg.MijError):
        mijpeg.decode(DC.case("sample_64x64").jpg, order="gbr")


def test_decode_host_tool_compiles(tmp_path):
    """host/decode_jpg.c against the public header, warning-free, and linked
    (nothing is run: no GPU here)"""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"),
                           os.path.join(PKG, "host", "decode_jpg.c"), "-L", PKG, "-lmijpeg",
                           "-o", str(tmp_path / "decode_jpg")])
    subprocess.check_call(["make", "-s", "-C", PKG, "host/decode_jpg"])
    assert os.access(os.path.join(PKG, "host", "decode_jpg"), os.X_OK)
