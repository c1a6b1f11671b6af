"""Encoding at a chosen chroma sampling on the GPU: for every
case the batch's layout, every component plane (which tells a front-end error
from an entropy-coder error) and the stream's bytes are the numpy model's
(sampling_model.py, pinned to the oracle, foreign_model.py and Pillow by
test_sampling_model.py); the streams decode with mijpeg.decode to the pixels
the plain Python decoder gives for them.  The shapes are the smallest at
which each part can go wrong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foreign_model as FM
import interleave_model as IM
import mijpeg
import ppm
import sampling_cases as SC
import sampling_model as SM

pytestmark = pytest.mark.gpu

NEW = ("422", "444", "gray")
# k_samp_dct's tile is 128 x 16 pixels (SAMP_TW x SAMP_TH, csrc/mij_sampled.h):
# two tiles across with 72 of the second one's 128 columns, three down with
# one block row of the last one's two at 4:4:4, 4:2:2 and greyscale
TILE_FRAME = (200, 40)
SIZES = [(1, 1), (7, 9), (8, 8), (9, 8), (15, 17), (16, 16), (17, 15), (33, 31), (100, 75), TILE_FRAME]


def r16(v):
    return (v + 15) & ~15


def check(b, i, frame_bgr, q, rr, s, decode=True):
    m = SM.model(frame_bgr, q, rr, s)
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


@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("s", NEW)
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_restarts_orders(w, h, s, q):
    f = SC.photo(w, h, seed=q)
    rgb = np.ascontiguousarray(f[..., ::-1])
    b = mijpeg.Batch(r16(w), r16(h), 1, q)
    try:
        for order in ("bgr", "rgb"):
            b.set_rgb(order == "rgb")
            b.upload_any(rgb if order == "rgb" else f, 0)
            for rr in (0, 1, 3):
                b.encode_sampled(1, s, rr)
                check(b, 0, f, q, rr, s, decode=order == "bgr")
    finally:
        b.close()


def test_mixed_sizes_then_other_samplings_on_the_same_batch():
    """frames of four sizes in one call; then the same batch at the other
    samplings in a row (the buffers grow from greyscale to 4:4:4 and are
    reused going back), restarts changing with them"""
    sizes = [(1, 1), (100, 75), TILE_FRAME, (33, 31)]
    frames = [SC.photo(w, h, seed=i) for i, (w, h) in enumerate(sizes)]
    b = mijpeg.Batch(208, 80, 4, 50)
    try:
        for i, f in enumerate(frames):
            b.upload_any(f, i)
        for s, rr in (("gray", 1), ("444", 0), ("422", 2), ("444", 1), ("gray", 0)):
            b.encode_sampled(4, s, rr)
            lens = b.lengths(4)
            for i, f in enumerate(frames):
                assert lens[i] == len(SM.model(f, 50, rr, s).jpg)
                check(b, i, f, 50, rr, s, decode=False)
        # fewer frames than before: nothing stale
        b.encode_sampled(2, "422", 0)
        for i in range(2):
            check(b, i, frames[i], 50, 0, "422", decode=False)
    finally:
        b.close()


@pytest.mark.parametrize("rr", [0, 2])
def test_420_is_encode_interleaved(rr):
    f = SC.photo(100, 75, seed=3)
    b = mijpeg.Batch(112, 80, 1, 50)
    try:
        b.upload_any(f, 0)
        b.encode_interleaved(1, rr)
        want = b.output(0)
        b.encode_sampled(1, "444", rr)  # another path in between
        b.encode_sampled(1, "420", rr)
        assert b.output(0) == want == IM.model(f, 50, rr).jpg
        check(b, 0, f, 50, rr, "420")
    finally:
        b.close()
    assert mijpeg.encode_any(f, "bgr", 50, rr, sampling="420") == want


@pytest.mark.parametrize("s", NEW)
def test_exceptions_and_ties(s):
    """colours whose FP64 conversion lands one below the exact integer (Q =
    100 shows every sample in the DC), flat greys 0..255, checkerboards and
    0/255 extremes, and blocks synthesised onto quantisation boundaries"""
    cases = [(SC.exception_frame(), 100), (SC.grey_levels(), 100), (SC.grey_levels(), 50),
             (SC.checker_frame(), 100), (SC.checker_frame(), 50)] + \
            [(SC.boundary_frame(seed), q) for seed in (5, 6) for q in (100, 90, 50)]
    for f, q in cases:
        h, w = f.shape[:2]
        b = mijpeg.Batch(r16(w), r16(h), 1, q)
        try:
            b.upload_any(f, 0)
            b.encode_sampled(1, s, 0)
            check(b, 0, f, q, 0, s)
        finally:
            b.close()


def test_capacity_grows_with_the_sampling():
    """noise at Q = 100, 4:4:4, a restart every MCU row: twice the blocks of
    4:2:0 on a batch whose output capacity was sized for 4:2:0 before"""
    f = SC.noise(64, 64, seed=1)
    m = SM.model(f, 100, 1, "444")
    assert len(m.jpg) <= mijpeg.max_jpg_bytes_sampled(64, 64, "444", 1)
    b = mijpeg.Batch(64, 64, 1, 100)
    try:
        b.upload_any(f, 0)
        b.encode_interleaved(1, 1)
        assert b.output(0) == IM.model(f, 100, 1).jpg
        assert len(m.jpg) > len(b.output(0))
        b.encode_sampled(1, "444", 1)
        got = check(b, 0, f, 100, 1, "444")
        assert got.endswith(b"\xff\xd9") and got.count(b"\xff\x00") > 20
        # the model's stream is (or is not) past what a 4:2:0 frame of this size may need: recorded, not required
        print("444 stream", len(got), "bytes; 4:2:0 bound", mijpeg.max_jpg_bytes_any(64, 64, 1))
    finally:
        b.close()


@pytest.mark.parametrize("s,w,h,q,rr", [("444", 100, 75, 90, 3), ("422", 33, 31, 50, 1), ("gray", 200, 40, 50, 0),
                                        ("444", 7, 9, 50, 1)])
def test_round_trip_through_the_decoder_and_the_transcoder(s, w, h, q, rr):
    f = SC.photo(w, h, seed=q)
    got = mijpeg.encode_any(f, "bgr", q, rr, sampling=s)
    m = SM.model(f, q, rr, s)
    assert got == m.jpg
    b = mijpeg.Batch(r16(w), r16(h), 1, q)
    d = mijpeg.Decoder(r16(w), r16(h), 1)
    try:
        b.upload_any(f, 0)
        b.encode_sampled(1, s, rr)
        d.decode([got])
        assert d.layout(0)["raw"] == b.sampled_layout(0)["raw"]
        for c in range(m.G["ncomp"]):
            assert (d.component(0, c) == b.sampled_component(0, c)).all(), c
    finally:
        d.close()
        b.close()
    # the same coefficients give the same coder: transcoding to r restart rows
    # is encoding with r
    for r in (0, 1, 2):
        assert mijpeg.transcode(got, restart_rows=r) == SM.model(f, q, r, s).jpg


def test_errors():
    lib = mijpeg.load()

    def msg():
        return lib.mij_last_message().decode()

    frames = [SC.photo(33, 31, seed=i) for i in range(3)]
    b = mijpeg.Batch(48, 32, 3, 50)
    try:
        with pytest.raises(mijpeg.MijError, match="holds no padded input"):
            b.encode_sampled(1, "444", 0)
        b.upload_any(frames[0], 0)
        with pytest.raises(mijpeg.MijError, match="slot 1 holds no padded input"):
            b.encode_sampled(2, "422", 0)
        assert lib.mij_batch_encode_sampled(b.h_, 1, 4, 0) == 1 and "sampling 4" in msg()
        assert lib.mij_batch_encode_sampled(b.h_, 1, 2, -1) == 1
        assert lib.mij_batch_encode_sampled(b.h_, 0, 2, 0) == 1
        # Ri = restart_rows * ceil(w / 8) = 13108 * 5 > 65535
        assert lib.mij_batch_encode_sampled(b.h_, 1, 2, 13108) == 1 and "over 65535" in msg()
        out = np.zeros(24, np.int32)
        assert lib.mij_batch_sampled_layout(b.h_, 0, out.ctypes.data, 24) == 1 and "no mij_batch_encode_sampled" in msg()
        # set_rgb flipped after padding
        b.set_rgb(True)
        assert lib.mij_batch_encode_sampled(b.h_, 1, 2, 0) == 1 and "set_rgb changed" in msg()
        b.set_rgb(False)
        # one frame with too small an output capacity fails alone
        for i, f in enumerate(frames):
            b.upload_any(f, i)
        small = lib.mij_test_sampled_out_cap  # test-only (csrc/mij_testing.h), bound by name
        small.argtypes, small.restype = [C.c_void_p, C.c_int, C.c_longlong], C.c_int
        assert small(None, 0, 64) == -2 and small(b.h_, 3, 64) == -2 and small(b.h_, 0, -1) == -2
        assert small(b.h_, 1, 1500) == 0
        b.encode_sampled(3, "444", 1)
        lens = b.lengths(3)
        assert lens[1] == 0 and lens[0] > 0 and lens[2] > 0
        with pytest.raises(mijpeg.MijError, match=r"\(4\)"):
            b.output(1)
        for i in (0, 2):
            check(b, i, frames[i], 50, 1, "444", decode=False)
        # the hook is consumed: the next encode gives every frame
        b.encode_sampled(3, "444", 1)
        for i in range(3):
            check(b, i, frames[i], 50, 1, "444", decode=False)
        assert lib.mij_batch_sampled_layout(b.h_, 3, out.ctypes.data, 24) == 1
        assert lib.mij_batch_sampled_layout(b.h_, 0, out.ctypes.data, 23) == 4
        assert lib.mij_batch_sampled_component(b.h_, 0, 3, out.ctypes.data, 1 << 20) == 1
        assert lib.mij_batch_sampled_component(b.h_, 0, 0, out.ctypes.data, 63) == 4
    finally:
        b.close()


def test_command_line(tmp_path):
    """host/encode_ppm --sampling: any PPM size through mij_encode_sampled"""
    exe = os.path.join(os.path.dirname(mijpeg.LIB_PATH), "host", "encode_ppm")
    f = SC.photo(35, 21, seed=8)
    src = tmp_path / "in.ppm"
    src.write_bytes(ppm.ppm_bytes(np.ascontiguousarray(f[..., ::-1])))
    for s in ("444", "gray"):
        dst = tmp_path / f"out_{s}.jpg"
        r = subprocess.run([exe, str(src), str(dst), "90", "--sampling", s], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert dst.read_bytes() == SM.model(f, 90, 0, s).jpg
    r = subprocess.run([exe, str(src), str(tmp_path / "x.jpg"), "--sampling", "411"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0
