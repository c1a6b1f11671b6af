"""The pixels-to-tensor stage on the GPU: k_tensorize through
mij_tensorizer_* against the numpy model (tensor_model.py), which
tests/test_tensor_model.py pins to torch.  Every comparison is equality of
bytes."""
import numpy as np
import pytest

import mijpeg
import tensor_cases as TC
import tensor_model as TM

pytestmark = pytest.mark.gpu

AWKWARD = ((0.5, 0.25, 0.125), (1 / 3, 0.7, 2.0))  # three different channels, so a swapped or shifted channel shows
MIRROR = [0, 1, 1]
# 1 and 5: lines shorter than a 16-byte piece; 67: odd, heads and tails at every alignment; the last: a second
# workgroup across, holding 3 pixels
WIDTHS = (1, 5, 67, TC.TZ_SEG + 3)
# 1 and 3: less than a tile; the last: a second workgroup down, holding 3 rows
HEIGHTS = (1, 3, TC.TZ_ROWS + 3)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_dtype_layout_and_swap_into_both_destinations(w, h):
    """three frames at byte offsets 0, 1 and 3 with pitches 3w, 3w + 5 and
    3w + 16, mirror flags 0, 1, 1; into the tensorizer's own buffer, and into a
    caller's 16-aligned buffer whose bytes behind the tensor stay as they were"""
    frames = [TC.frame(w, h, s) for s in range(3)]
    arena, images, dst = TC.place(frames, dst_bytes=mijpeg.tensor_bytes(3, w, h, "float32"))
    assert [im[0] % 4 for im in images] == [0, 1, 3] and [im[1] - 3 * w for im in images] == [0, 5, 16]
    t = mijpeg.Tensorizer(3)
    try:
        for dtype in TM.DTYPES:  # by element size, so the bytes behind a tensor were never inside an earlier one
            need = mijpeg.tensor_bytes(3, w, h, dtype)
            for layout in TM.LAYOUTS:
                for swap in (0, 1):
                    want = TM.tensorize(frames, MIRROR, dtype, layout, swap, *AWKWARD)
                    assert want.nbytes == need
                    kw = dict(mirror=MIRROR, dtype=dtype, layout=layout, swap=swap, mean=AWKWARD[0], std=AWKWARD[1])
                    t.run(images, **kw)
                    got = t.result()
                    assert got.shape == want.shape and got.dtype == want.dtype
                    assert (bits(got) == bits(want)).all(), (dtype, layout, swap, int((bits(got) != bits(want)).sum()))
                    assert t.device()[1] == need and t.device()[0] % 16 == 0
                    t.run(images, dst_ptr=arena.ptr + dst, cap=need, **kw)
                    assert t.ms() >= 0  # waits: the arena is read back on another stream
                    back = arena.read(dst, need + 64)
                    assert (back[:need] == bits(want)).all(), (dtype, layout, swap, "caller's buffer")
                    assert (back[need:] == TC.FILL).all(), (dtype, layout, swap, "bytes behind the tensor")
                    assert (bits(t.result()) == bits(want)).all()  # the owned result is still served
        assert t.ms() >= 0
    finally:
        t.close()
        arena.close()


def test_no_mirror_flags_and_the_defaults():
    """mirror NULL; ImageNet's mean and std into float16 NCHW, the binding's defaults"""
    frames = [TC.frame(67, 3, s) for s in range(2)]
    arena, images, _ = TC.place(frames)
    t = mijpeg.Tensorizer(2)
    try:
        t.run(images)
        assert (bits(t.result()) == bits(TM.tensorize(frames))).all()
    finally:
        t.close()
        arena.close()


def test_the_owned_buffer_grows_and_the_first_call_still_works():
    small = [TC.frame(5, 3, s) for s in range(2)]
    large = [TC.frame(300, 40, s) for s in range(3)]
    a_s, im_s, _ = TC.place(small)
    a_l, im_l, _ = TC.place(large)
    t = mijpeg.Tensorizer(3)
    try:
        for _ in range(2):
            t.run(im_s, mirror=[1, 0], dtype="float32")
            assert (bits(t.result()) == bits(TM.tensorize(small, [1, 0], "float32"))).all()
            t.run(im_l, mirror=[0, 1, 0], dtype="float32", layout="nhwc")
            assert (bits(t.result()) == bits(TM.tensorize(large, [0, 1, 0], "float32", "nhwc"))).all()
    finally:
        t.close()
        a_s.close()
        a_l.close()


def test_a_refused_call_leaves_the_previous_owned_result_readable():
    frames = [TC.frame(67, 3, s) for s in range(2)]
    arena, images, dst = TC.place(frames, dst_bytes=4096)
    t = mijpeg.Tensorizer(2)
    lib = t.lib
    try:
        with pytest.raises(mijpeg.MijError, match="no mij_tensorizer_run"):
            t.device()
        assert lib.mij_last_error() == 1  # MIJ_EINVAL
        with pytest.raises(mijpeg.MijError, match="no mij_tensorizer_run"):
            t.ms()
        t.run(images, dtype="bfloat16", layout="nhwc")
        want = TM.tensorize(frames, None, "bfloat16", "nhwc")
        assert (bits(t.result()) == bits(want)).all()
        a, pitch, w, h = images[0]
        bad = [(dict(dtype=4), "dtype 4"), (dict(layout=2), "layout 2"), (dict(swap=2), "swap 2"),
               (dict(mean=(0.0, float("inf"), 0.0)), r"mean\[1\]"), (dict(std=(1.0, 1.0, 0.0)), r"std\[2\]"),
               (dict(images=[images[0], (images[1][0], images[1][1], w, h + 1)]), "frame 1: src is"),
               (dict(images=[(a, pitch, 65536, h)]), "frame 0: src is"), (dict(images=[(a, 3 * w - 1, w, h)]), "src.pitch"),
               (dict(images=[images[0], (0, pitch, w, h)]), "frame 1: src.px"), (dict(images=images * 2), "n 4"),
               (dict(images=[]), "n 0"), (dict(dst_ptr=arena.ptr + dst + 8, cap=1 << 20), "16-byte")]
        for kw, word in bad:
            kw = {"images": images, **kw}
            with pytest.raises(mijpeg.MijError, match=word):
                t.run(kw.pop("images"), **kw)
            assert lib.mij_last_error() == 1
            assert (bits(t.result()) == bits(want)).all()
        with pytest.raises(mijpeg.MijError, match=str(want.nbytes * 2)):
            t.run(images, dtype="float32", dst_ptr=arena.ptr + dst, cap=want.nbytes * 2 - 1)
        assert lib.mij_last_error() == 4  # MIJ_ENOSPC
        assert (arena.read(dst, 64) == TC.FILL).all()
        assert (bits(t.result()) == bits(want)).all()
        out = np.zeros(want.nbytes, np.uint8)
        assert lib.mij_tensorizer_read(t.h_, out.ctypes.data, want.nbytes - 1) == 4
        assert str(want.nbytes).encode() in lib.mij_last_message()
        # a caller's buffer does not disturb the owned result either
        t.run(images, dtype="uint8", dst_ptr=arena.ptr + dst, cap=4096)
        t.ms()  # waits: the arena is read back on another stream
        assert (arena.read(dst, 2 * 67 * 3 * 3) == bits(TM.tensorize(frames, None, "uint8"))).all()
        assert (bits(t.result()) == bits(want)).all()
    finally:
        t.close()
        arena.close()


def test_streams():
    frames = [TC.frame(5, 3, 0)]
    arena, images, _ = TC.place(frames)
    t, r = mijpeg.Tensorizer(1), mijpeg.Resizer(1)
    try:
        own = t.stream_ptr()
        t.set_stream(r.stream_ptr())
        assert t.stream_ptr() == r.stream_ptr() != own
        t.run(images, dtype="uint8")
        assert (bits(t.result()) == bits(TM.tensorize(frames, None, "uint8"))).all()
        t.set_stream(0)
        assert t.stream_ptr() == own
    finally:
        t.close()
        r.close()
        arena.close()
