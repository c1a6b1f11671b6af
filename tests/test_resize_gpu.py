"""The resampler on the GPU: k_rs_h / k_rs_v through
mij_resizer_*, mij_resize and mij_thumbnail against the numpy model
(resize_model.py), which tests/test_resize_model.py pins to Pillow.  No test
here needs Pillow."""
import os
import subprocess

import numpy as np
import pytest

import foreign_cases as FC
import mijpeg
import resize_cases as RC
import resize_model as RM
import scaled_cases as SC

pytestmark = pytest.mark.gpu

PKG = os.path.dirname(mijpeg.LIB_PATH)
CHAIN = ("420_96x80_noise_q95", (20, 17), "bicubic", 75)


def device_bytes(host: np.ndarray):
    """(owner, device address) of a copy of host's bytes: a detector's frame
    buffer serves as plain device memory (no second HIP runtime in the process)"""
    pitch = 4096
    rows = (-(-host.size // pitch) + 3) & ~3
    buf = np.zeros((max(rows, 16), pitch), np.uint8)
    buf.reshape(-1)[:host.size] = host
    det = mijpeg.Detector(16, max(rows, 16))
    return det, det.upload(buf, pitch)


def device_frames(frames, lead=0, gap=0):
    """the frames packed one after the other, `lead` bytes in and `gap` bytes
    apart: (owner, [(address, pitch, w, h)])"""
    at, offs = lead, []
    for f in frames:
        offs.append(at)
        at += f.size + gap
    host = np.full(at + 64, 0x5A, np.uint8)
    for f, o in zip(frames, offs):
        host[o:o + f.size] = f.ravel()
    det, ptr = device_bytes(host)
    return det, [(ptr + o, 3 * f.shape[1], f.shape[1], f.shape[0]) for f, o in zip(frames, offs)]


def check(r, i, want):
    got = r.pixels(i)
    assert got.shape == want.shape and (got == want).all(), (i, int((got != want).any(-1).sum()))
    ptr, pitch = r.device_pixels(i)
    assert pitch == (3 * want.shape[1] + 15) // 16 * 16 and ptr % 16 == 0


@pytest.mark.parametrize("f", RC.FILTERS)
def test_every_case_in_one_call(f):
    """the eleven pairs as eleven frames of one call: both passes, either one
    skipped, up and down, 1 x 1 on either side, the widest window (480 -> 7:
    weights read from the table, not from LDS), more than one tile across
    (100, 80) with a partial last one"""
    det, images = device_frames([RC.frame(p[0], p[1]) for p in RC.PAIRS])
    r = mijpeg.Resizer(len(RC.PAIRS))
    try:
        r.resize(images, [p[2:] for p in RC.PAIRS], f)
        for i, p in enumerate(RC.PAIRS):
            check(r, i, RC.model((p, f)))
        h_ms, v_ms = r.ms()
        assert h_ms >= 0 and v_ms >= 0
    finally:
        r.close()
        det.close()


def test_skipped_passes_and_a_copy_among_resized_frames():
    src = RC.frame(37, 29)
    sizes = [(16, 16), (37, 10), (37, 29), (80, 29), (37, 29), (1, 1)]
    det, images = device_frames([src] * len(sizes), lead=1, gap=3)
    r = mijpeg.Resizer(8)
    try:
        for f in ("bilinear", "box"):
            r.resize(images, sizes, f)
            for i, s in enumerate(sizes):
                check(r, i, RM.resize(src, s, f))
        assert (r.pixels(2) == src).all()  # both sizes equal: a copy
    finally:
        r.close()
        det.close()


@pytest.mark.parametrize("f", RC.FILTERS)
def test_windows_wider_than_the_staged_piece(f):
    """2500 source pixels under one tile: k_rs_h stages them in three pieces
    and a lane's window spans them, its weights read from the table; 1100 ->
    72 crosses a piece inside a window with the weights in LDS (ksize 63)"""
    a, b = RC.frame(2500, 5), RC.frame(1100, 6)
    det, images = device_frames([a, b], lead=3)
    r = mijpeg.Resizer(2)
    try:
        r.resize(images, [(3, 5), (72, 4)], f)
        check(r, 0, RM.resize(a, (3, 5), f))
        check(r, 1, RM.resize(b, (72, 4), f))
    finally:
        r.close()
        det.close()


@pytest.mark.parametrize("f", RC.FILTERS)
def test_interior_rectangle_at_an_odd_offset_and_pitch(f):
    """crop, then resize: a 37 x 29 rectangle inside a 101 x 67 image whose
    rows are 305 bytes apart, so the rows start at every alignment"""
    big = RC.frame(101, 67)
    pitch = 3 * 101 + 2
    host = np.full((67, pitch), 0xC3, np.uint8)
    host[:, :303] = big.reshape(67, -1)
    det, base = device_bytes(np.concatenate([np.zeros(1, np.uint8), host.ravel()]))
    x, y, w, h = 7, 5, 37, 29
    ptr = base + 1 + y * pitch + 3 * x
    assert ptr % 2 == 1 and pitch % 2 == 1
    crop = np.ascontiguousarray(big[y:y + h, x:x + w])
    sizes = [(16, 16), (37, 10), (80, 29), (37, 29), (64, 48)]
    r = mijpeg.Resizer(len(sizes))
    try:
        r.resize([(ptr, pitch, w, h)] * len(sizes), sizes, f)
        for i, s in enumerate(sizes):
            check(r, i, RM.resize(crop, s, f))
    finally:
        r.close()
        det.close()


@pytest.mark.parametrize("f", ("box", "bicubic"))
def test_tall_frames_whose_workgroups_take_several_row_groups(f):
    """k_rs_h gives a workgroup 1 to 8 groups of 4 rows, by the frame's height:
    1030 rows make 8 with a last workgroup of 6 rows, 300 rows 2, 515 rows 4"""
    frames = [RC.frame(40, 1030), RC.frame(23, 300), RC.frame(9, 515)]
    sizes = [(20, 1030), (70, 300), (5, 64)]
    det, images = device_frames(frames, lead=1)
    r = mijpeg.Resizer(3)
    try:
        r.resize(images, sizes, f)
        for i, s in enumerate(sizes):
            check(r, i, RM.resize(frames[i], s, f))
    finally:
        r.close()
        det.close()


def test_buffers_grow_and_the_first_call_still_works():
    small = [RC.frame(5, 3), RC.frame(2, 2)]
    large = [RC.frame(480, 270), RC.frame(240, 135)]
    det_s, im_s = device_frames(small)
    det_l, im_l = device_frames(large)
    r = mijpeg.Resizer(2)
    try:
        for _ in range(2):
            r.resize(im_s, [(1, 1), (3, 3)], "bicubic")
            check(r, 0, RC.model(((5, 3, 1, 1), "bicubic")))
            check(r, 1, RC.model(((2, 2, 3, 3), "bicubic")))
            r.resize(im_l, [(7, 3), (300, 200)], "bicubic")
            check(r, 0, RC.model(((480, 270, 7, 3), "bicubic")))
            check(r, 1, RM.resize(large[1], (300, 200), "bicubic"))
    finally:
        r.close()
        det_s.close()
        det_l.close()


def test_a_refused_call_leaves_the_previous_result_served():
    src = RC.frame(37, 29)
    det, images = device_frames([src])
    r = mijpeg.Resizer(1)
    lib = r.lib
    try:
        with pytest.raises(mijpeg.MijError, match="no mij_resizer_resize"):
            r.pixels(0)  # a pixels call before a resize
        assert lib.mij_last_error() == 1  # MIJ_EINVAL
        r.resize(images, [(16, 16)], "bicubic")
        want = RC.model(((37, 29, 16, 16), "bicubic"))
        check(r, 0, want)
        a, pitch, w, h = images[0]
        bad = [((images, [(16, 16)], 3), "filter"), ((images, [(0, 16)], 2), "frame 0: out_wh"),
               (([(a, pitch, w, 65536)], [(16, 16)], 2), "frame 0: src"), (([(0, pitch, w, h)], [(16, 16)], 2), "src.px"),
               (([(a, 3 * w - 1, w, h)], [(16, 16)], 2), "src.pitch"), ((images * 2, [(16, 16)] * 2, 2), "n 2")]
        for (im, sizes, f), word in bad:
            with pytest.raises(mijpeg.MijError, match=word):
                r.resize(im, sizes, f)
            assert lib.mij_last_error() == 1
            check(r, 0, want)
        out = np.zeros(want.size, np.uint8)
        assert lib.mij_resizer_pixels(r.h_, 0, out.ctypes.data, want.size - 1, 0) == 4  # MIJ_ENOSPC
        assert str(want.size).encode() in lib.mij_last_message()
        assert lib.mij_resizer_pixels(r.h_, 1, out.ctypes.data, want.size, 0) == 1
    finally:
        r.close()
        det.close()


def test_one_call_resize():
    for case in (((37, 29, 16, 16), "bicubic"), ((64, 48, 100, 75), "bilinear"), ((1, 1, 5, 7), "box")):
        (w, h, ow, oh), f = case
        assert (mijpeg.resize(RC.frame(w, h), (ow, oh), f) == RC.model(case)).all(), RC.case_id(case)
    wide = np.ascontiguousarray(RC.frame(64, 48)[:, :37])  # rows of a wider array: made contiguous by the wrapper
    assert (mijpeg.resize(RC.frame(64, 48)[:, :37], (16, 16)) == RM.resize(wide, (16, 16), "bicubic")).all()


def chain_model():
    name, size, f, q = CHAIN
    m = FC.model(name)
    denom = mijpeg.thumbnail_denom(m.w, m.h, *size)
    assert denom == 4
    s = SC.model(name, denom)
    assert (s.ow, s.oh) == (24, 20)
    return denom, s, mijpeg.encode_any(RM.resize(s.bgr, size, f), "bgr", q)


def test_device_chain_decode_resize_encode():
    """Decoder.reconstruct(scale) -> Resizer on the decoder's stream ->
    Batch.pad_input / encode_interleaved: the pixels never leave the device,
    and mijpeg.thumbnail is the same chain in one call"""
    name, size, f, q = CHAIN
    denom, s, want = chain_model()
    d = mijpeg.Decoder(96, 80, 1)
    r = mijpeg.Resizer(1)
    b = mijpeg.Batch(32, 32, 1, q)
    try:
        d.decode([FC.jpg(name)])
        d.reconstruct("bgr", scale=denom)
        ptr, pitch = d.device_pixels(0)
        r.set_stream(d.stream_ptr())
        assert r.stream_ptr() == d.stream_ptr()
        r.resize([(ptr, pitch, s.ow, s.oh)], [size], f)
        rptr, rpitch = r.device_pixels(0)
        b.set_stream(d.stream_ptr())
        b.pad_input(rptr, 0, rpitch, [size])
        b.encode_interleaved(1, 0)
        assert b.output(0) == want
        assert (r.pixels(0) == RM.resize(s.bgr, size, f)).all()
        b.set_stream(0)
        r.set_stream(0)
        assert r.stream_ptr() != d.stream_ptr()
    finally:
        b.close()
        r.close()
        d.close()
    assert mijpeg.thumbnail(FC.jpg(name), size, f, q) == want
    assert mijpeg.decode(want).shape == (size[1], size[0], 3)


def test_thumbnail_at_other_scales_and_filters():
    """denominator 1 (an enlargement) and 8, the other filters"""
    name = "420_96x80_noise_q95"
    for size, f, denom in (((120, 100), "bilinear", 1), ((12, 10), "box", 8), ((48, 40), "bicubic", 2)):
        assert mijpeg.thumbnail_denom(96, 80, *size) == denom
        px = SC.model(name, denom).bgr if denom > 1 else FC.model(name).rgb[..., ::-1]
        want = mijpeg.encode_any(RM.resize(np.ascontiguousarray(px), size, f), "bgr", 60)
        assert mijpeg.thumbnail(FC.jpg(name), size, f, 60) == want, (size, f)


def test_host_tool(tmp_path):
    name, size, f, q = CHAIN
    _, _, want = chain_model()
    out = str(tmp_path / "thumb.jpg")
    subprocess.run([os.path.join(PKG, "host", "thumbnail_jpg"), "-filter", f, "-quality", str(q), f"{size[0]}x{size[1]}",
                    os.path.join(FC.DIR, name + ".jpg"), out], check=True, timeout=120)
    with open(out, "rb") as fh:
        assert fh.read() == want
