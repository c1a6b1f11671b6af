"""CPU tests of the sampled encoder's interface (DESIGN.md §4k,
include/mijpeg.h): the header declares it, the binding exports it, the size
bound follows its rules, and every refusal -- and the cap-0 size query --
comes back before any device work (this machine has no GPU to touch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mijpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "mijpeg.h")
NAMES = ["mij_max_jpg_bytes_sampled", "mij_batch_encode_sampled", "mij_batch_sampled_component",
         "mij_batch_sampled_layout", "mij_encode_sampled"]
S420, S422, S444, GRAY = 0, 1, 2, 3
EINVAL, ENOSPC = 1, 4


def test_header_and_binding_name_the_interface():
    src = open(HEADER).read()
    norm = re.sub(r"\s+", " ", src)
    assert "enum { MIJ_SAMP_420 = 0, MIJ_SAMP_422 = 1, MIJ_SAMP_444 = 2, MIJ_SAMP_GRAY = 3 };" in norm
    assert "size_t mij_max_jpg_bytes_sampled(int w, int h, int sampling, int restart_rows);" in norm
    assert "int mij_batch_encode_sampled(mij_batch *b, int nframes, int sampling, int restart_rows);" in norm
    assert "int mij_batch_sampled_component(mij_batch *b, int frame, int comp, int16_t *dst, size_t cap);" in norm
    assert "int mij_batch_sampled_layout(mij_batch *b, int frame, int *out, int n);" in norm
    assert ("int mij_encode_sampled(const uint8_t *px, int stride_px, int w, int h, int order, int quality, "
            "int sampling, int restart_rows, uint8_t *out, size_t cap, size_t *out_len);") in norm
    lib = mijpeg.load()
    for n in NAMES:
        assert hasattr(lib, n) and n in mijpeg.EXPORTS, n
    assert mijpeg.SAMPLINGS == {"420": S420, "422": S422, "444": S444, "gray": GRAY}
    for m in ("encode_sampled", "sampled_component", "sampled_layout"):
        assert callable(getattr(mijpeg.Batch, m))
    import inspect
    sig = inspect.signature(mijpeg.encode_any)
    assert list(sig.parameters) == ["frame", "order", "quality", "restart_rows", "sampling"]
    assert sig.parameters["sampling"].default == "420"
    # the capacity hook of the GPU tests is not public
    assert "mij_test_" not in src and hasattr(lib, "mij_test_sampled_out_cap")


SIZES = [(1, 1), (7, 9), (16, 16), (100, 75), (3837, 2157), (65535, 65535)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("rr", [0, 1, 3])
def test_bound_equals_any_for_420(w, h, rr):
    assert mijpeg.max_jpg_bytes_sampled(w, h, "420", rr) == mijpeg.max_jpg_bytes_any(w, h, rr)


def blocks(w, h, s):
    hmax, vmax = {S420: (2, 2), S422: (2, 1), S444: (1, 1), GRAY: (1, 1)}[s]
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return mx * my * (hmax * vmax + (0 if s == GRAY else 2)), mx, my


@pytest.mark.parametrize("w,h", SIZES[:-1] + [(4096, 65535)])
@pytest.mark.parametrize("rr", [0, 1, 3])
def test_bound_is_the_per_block_worst_case(w, h, rr):
    """the existing per-block worst case (mij_max_jpg_bytes: 434 bytes a block
    + 4096, rounded to 256) times the sampling's blocks, the DRI segment, two
    bytes per restart marker"""
    f = mijpeg.load().mij_max_jpg_bytes_sampled
    per64 = mijpeg.max_jpg_bytes(64, 64)  # 96 blocks
    assert per64 == -(-(96 * 434 + 4096) // 256) * 256
    for s in (S422, S444, GRAY):
        nb, mx, my = blocks(w, h, s)
        markers = (-(-my // rr) - 1) if rr else 0
        assert f(w, h, s, rr) == -(-(nb * 434 + 4096) // 256) * 256 + 2 * markers + (6 if rr else 0)


@pytest.mark.parametrize("w,h", [(16, 16), (64, 48), (1920, 1088), (3840, 2160)])
@pytest.mark.parametrize("rr", [0, 1, 3])
def test_bound_grows_with_the_sampling(w, h, rr):
    """grey <= 4:2:0 <= 4:2:2 <= 4:4:4 where the four MCU grids cover the same
    pixels (sides multiples of 16): the blocks are 1 : 1.5 : 2 : 3.  (A frame
    of 1..8 rows pads to 16 rows at 4:2:0 only, which can cost 4:2:0 more
    blocks than 4:2:2 or 4:4:4.)"""
    f = mijpeg.load().mij_max_jpg_bytes_sampled
    v = [f(w, h, s, rr) for s in (GRAY, S420, S422, S444)]
    assert 0 < v[0] <= v[1] <= v[2] <= v[3], v


def test_bound_refuses_bad_arguments():
    f = mijpeg.load().mij_max_jpg_bytes_sampled
    for s in (S420, S422, S444, GRAY):
        assert f(0, 16, s, 0) == f(16, 0, s, 0) == f(65536, 16, s, 0) == f(16, 65536, s, 0) == 0
        assert f(16, 16, s, -1) == 0
    assert f(16, 16, 4, 0) == f(16, 16, -1, 0) == 0
    # Ri = r * ceil(w / (8 Hmax)) over 65535
    assert f(65535, 16, S444, 8) == 0 and f(65535, 16, S444, 7) > 0      # 8192 MCUs across
    assert f(65535, 16, GRAY, 8) == 0
    assert f(65535, 16, S422, 16) == 0 and f(65535, 16, S422, 15) > 0    # 4096 MCUs across
    assert f(65535, 16, S420, 16) == 0


def call(w, h, s, rr=0, order=0, q=50, cap=0):
    lib = mijpeg.load()
    n = C.c_size_t(12345)
    rc = lib.mij_encode_sampled(None, w, w, h, order, q, s, rr, None, cap, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("s", [S420, S422, S444, GRAY])
def test_cap_zero_asks_for_the_size_without_a_device(s):
    for (w, h, rr) in ((1, 1, 0), (100, 75, 2), (3837, 2157, 1)):
        rc, n = call(w, h, s, rr)
        assert rc == ENOSPC and n == mijpeg.load().mij_max_jpg_bytes_sampled(w, h, s, rr) > 0
        assert mijpeg.load().mij_last_error() == ENOSPC


def test_refusals_come_before_any_device_work():
    for s in (4, -1):
        assert call(16, 16, s)[0] == EINVAL
    for s in (S422, S444, GRAY):
        assert call(0, 16, s)[0] == EINVAL and call(16, 0, s)[0] == EINVAL
        assert call(65536, 16, s)[0] == EINVAL and call(16, 65536, s)[0] == EINVAL
        assert call(16, 16, s, rr=-1)[0] == EINVAL
        assert call(16, 16, s, order=2)[0] == EINVAL and call(16, 16, s, order=-1)[0] == EINVAL
        assert call(16, 16, s, q=0)[0] == EINVAL and call(16, 16, s, q=101)[0] == EINVAL
        assert call(65535, 16, s, rr=16)[0] == EINVAL
        assert mijpeg.load().mij_last_error() == EINVAL
        assert b"mij_encode_sampled" in mijpeg.load().mij_last_message()
    # enough room, no pixels: still refused before a device is looked for
    lib = mijpeg.load()
    out = np.zeros(lib.mij_max_jpg_bytes_sampled(16, 16, S444, 0), np.uint8)
    n = C.c_size_t(0)
    assert lib.mij_encode_sampled(None, 16, 16, 16, 0, 50, S444, 0, out.ctypes.data, out.size, C.byref(n)) == EINVAL


def test_python_refuses_an_unknown_sampling():
    with pytest.raises(ValueError):
        mijpeg.encode_any(np.zeros((8, 8, 3), np.uint8), sampling="411")
    with pytest.raises(ValueError):
        mijpeg.max_jpg_bytes_sampled(8, 8, "440")
