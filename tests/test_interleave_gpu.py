"""The interleaved output format on the GPU: for every case
the kernels' bytes are the numpy model's (interleave_model.py, pinned to
foreign_model.py and Pillow by test_interleave_model.py), and they decode with
mijpeg.decode to the pixels the plain Python decoder gives for them.  The
shapes are the smallest at which each part can go wrong."""
import ctypes as C

import numpy as np
import pytest

import foreign_model as FM
import interleave_model as IM
import mijpeg

pytestmark = pytest.mark.gpu


def r16(v):
    return (v + 15) & ~15


def check_stream(got: bytes, frame_bgr, q, rr):
    want = IM.model(frame_bgr, q, rr).jpg
    assert len(got) == len(want), (len(got), len(want))
    assert got == want
    px = mijpeg.decode(got, "rgb")
    assert px.shape == frame_bgr.shape
    assert (px == FM.decoded(got).rgb).all()


def device_bytes(host: np.ndarray):
    """(owner, device address) of a copy of host's bytes: a detector's frame
    buffer serves as plain device memory (no second HIP runtime in the process)"""
    pitch = 4096
    rows = (-(-host.size // pitch) + 3) & ~3
    buf = np.zeros((max(rows, 16), pitch), np.uint8)
    buf.reshape(-1)[:host.size] = host
    det = mijpeg.Detector(16, max(rows, 16))
    return det, det.upload(buf, pitch)


def encode_one(frame, q=50, rr=0, rgb=False):
    h, w = frame.shape[:2]
    b = mijpeg.Batch(r16(w), r16(h), 1, q)
    try:
        b.set_rgb(rgb)
        b.upload_any(frame, 0)
        b.encode_interleaved(1, rr)
        return b.output(0)
    finally:
        b.close()


# one MCU with both pads; exact multiples; right pad only, bottom pad only;
# across K1's 128-pixel tile
@pytest.mark.parametrize("w,h", [(1, 1), (15, 15), (16, 16), (64, 48), (17, 16), (16, 17), (129, 33), (250, 130)])
def test_sizes(w, h):
    f = IM.frame(w, h)
    check_stream(encode_one(f), f, 50, 0)


def test_exact_multiple_planes_are_the_plain_paths():
    f = IM.frame(64, 48)
    a = mijpeg.Batch(64, 48, 1, 50)
    a.upload_any(f, 0)
    a.encode_interleaved(1, 0)
    got = a.coefs(0, diffed=False)
    a.close()
    p = mijpeg.Batch(64, 48, 1, 50)
    p.upload(f)
    p.dct(1)
    plain = p.coefs(0, diffed=False)
    p.close()
    want = IM.model(f, 50, 0).planes
    for c in range(3):
        assert (got[c] == plain[c]).all(), c
        assert (got[c].reshape(-1, 64) == want[c]).all(), c


# ten intervals (markers wrap past RST7); a short last interval; none
@pytest.mark.parametrize("rr", [1, 3, 0])
def test_restart_intervals(rr):
    f = IM.frame(40, 150)
    got = encode_one(f, 50, rr)
    check_stream(got, f, 50, rr)
    if rr == 1:
        assert got.count(b"\xff\xd7") >= 1 and FM.decoded(got).G["ri"] == 3


@pytest.mark.parametrize("rr", [0, 1])
def test_flat_frame(rr):
    f = IM.frame(33, 20, kind="flat")  # every block DC + EOB
    check_stream(encode_one(f, 50, rr), f, 50, rr)


@pytest.mark.parametrize("rr", [0, 1])
def test_noise_at_q100(rr):
    f = IM.frame(250, 130, kind="noise")  # long codes, ZRL, many stuffed bytes
    got = encode_one(f, 100, rr)
    check_stream(got, f, 100, rr)
    assert got.count(b"\xff\x00") > 50


@pytest.mark.parametrize("seed,ends", [(12, (b"\xff\x00\xff\xd1", b"\xff\x00\xff\xd9")),
                                       (86, (b"\xff\x00\xff\xd0", b"\xff\x00\xff\xd9"))])
def test_stuffed_pad_byte(seed, ends):
    """intervals, and the scan, whose padded last byte is 0xFF: stuffed before the marker"""
    f = IM.frame(16, 48, seed=seed, kind="noise")
    want = IM.model(f, 100, 1).jpg
    assert all(e in want for e in ends) and want.endswith(ends[1])
    check_stream(encode_one(f, 100, 1), f, 100, 1)


def tables_equal(got, want):
    return all(list(g.sym_code_len) == list(w.sym_code_len) and list(g.sym_code) == list(w.sym_code) and
               list(g.code_len_freq[1:17]) == list(w.code_len_freq[1:17]) for g, w in zip(got, want))


def test_mixed_sizes_then_reuse():
    sizes = [(1, 1), (129, 33), (250, 130), (64, 48)]
    frames = [IM.frame(w, h, seed=i) for i, (w, h) in enumerate(sizes)]
    # device frames at an odd byte offset, odd pitch, odd frame stride
    pitch, fs, off = 3 * 250 + 7, (3 * 250 + 7) * 130 + 3, 5
    host = np.zeros(off + 4 * fs, np.uint8)
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        rows = host[off + i * fs:off + i * fs + h * pitch].reshape(h, pitch)
        rows[:, :3 * w] = f.reshape(h, 3 * w)
    det, ptr = device_bytes(host)
    assert (ptr + off) % 2 == 1 and pitch % 2 == 1 and fs % 2 == 1
    b = mijpeg.Batch(256, 144, 4, 50)
    b.pad_input(ptr + off, fs, pitch, sizes)
    b.encode_interleaved(4, 1)
    lens = b.lengths(4)
    for i, f in enumerate(frames):
        m = IM.model(f, 50, 1)
        got = b.output(i)
        assert lens[i] == len(m.jpg)
        check_stream(got, f, 50, 1)
        assert tables_equal(b.tables(i), m.tables)
    # the same batch, fewer and smaller frames, no restarts: nothing stale
    small = [IM.frame(17, 9, seed=9), IM.frame(40, 20, seed=10)]
    for i, f in enumerate(small):
        b.upload_any(f, i)
    b.encode_interleaved(2, 0)
    lens = b.lengths(2)
    for i, f in enumerate(small):
        m = IM.model(f, 50, 0)
        assert lens[i] == len(m.jpg)
        check_stream(b.output(i), f, 50, 0)
        assert tables_equal(b.tables(i), m.tables)
    # slots 2 and 3 still hold their frames
    b.encode_interleaved(4, 0)
    check_stream(b.output(2), frames[2], 50, 0)
    check_stream(b.output(0), small[0], 50, 0)
    b.close()
    det.close()


def test_channel_orders():
    f = IM.frame(129, 33, seed=4)
    rgb = np.ascontiguousarray(f[..., ::-1])
    check_stream(encode_one(rgb, 50, 1, rgb=True), f, 50, 1)
    check_stream(mijpeg.encode_any(rgb, "rgb", 50, 1), f, 50, 1)
    check_stream(mijpeg.encode_any(f, "bgr", 50, 0), f, 50, 0)
    # R, G, B frames from a device pointer at an odd offset with an odd pitch
    pitch = 3 * 129 + 2
    host = np.zeros(1 + 33 * pitch, np.uint8)
    host[1:].reshape(33, pitch)[:, :3 * 129] = rgb.reshape(33, 3 * 129)
    det, ptr = device_bytes(host)
    b = mijpeg.Batch(144, 48, 2, 50)
    for on in (True, False):
        b.set_rgb(on)
        b.pad_input(ptr + 1, 0, pitch, [(129, 33)])
        b.encode_interleaved(1, 0)
        check_stream(b.output(0), f if on else rgb, 50, 0)
    b.close()
    det.close()


def test_errors():
    lib = mijpeg.load()

    def msg():
        return lib.mij_last_message().decode()

    b = mijpeg.Batch(64, 48, 2, 50)
    # no padded input yet; and a plain upload forgets it
    with pytest.raises(mijpeg.MijError, match="holds no padded input"):
        b.encode_interleaved(1, 0)
    b.upload_any(IM.frame(20, 20), 0)
    with pytest.raises(mijpeg.MijError, match="slot 1 holds no padded input"):
        b.encode_interleaved(2, 0)
    b.upload(np.zeros((48, 64, 3), np.uint8), 0)
    assert lib.mij_batch_encode_interleaved(b.h_, 1, 0) == 1 and "holds no padded input" in msg()
    # Ri = restart_rows * ceil(w / 16) > 65535
    b.upload_any(IM.frame(20, 20), 0)
    assert lib.mij_batch_encode_interleaved(b.h_, 1, 32768) == 1 and "over 65535" in msg()
    assert lib.mij_batch_encode_interleaved(b.h_, 1, 32767) == 0
    assert b.output(0) == IM.model(IM.frame(20, 20), 50, 32767).jpg
    assert mijpeg.max_jpg_bytes_any(20, 20, 32768) == 0
    # w or h of 0, or beyond the canvas
    det, ptr = device_bytes(np.zeros(64 * 64 * 3, np.uint8))
    for w, h in [(0, 5), (5, 0), (65, 48), (64, 49)]:
        wh = np.array([w, h], np.int32)
        assert lib.mij_batch_pad_input(b.h_, ptr, 0, 64 * 3, wh.ctypes.data, 1) == 1
        assert f"frame 0 is {w}x{h}" in msg()
    px = np.zeros((64, 64, 3), np.uint8)
    assert lib.mij_batch_upload_any(b.h_, px.ctypes.data, 64, 65, 48, 0) == 1 and "frame 0 is 65x48" in msg()
    b.close()
    det.close()
    # mij_encode_any: cap 0 asks for the bound, before any device work
    n = C.c_size_t(0)
    assert lib.mij_encode_any(None, 35, 35, 21, 0, 50, 1, None, 0, C.byref(n)) == 4
    assert n.value == mijpeg.max_jpg_bytes_any(35, 21, 1) == mijpeg.max_jpg_bytes(48, 32) + 2 * 1 + 6
    assert f"need {n.value} bytes" in msg()
    assert lib.mij_encode_any(None, 0, 0, 21, 0, 50, 0, None, 0, C.byref(n)) == 1 and "frame 0x21" in msg()


def test_two_encodes_give_the_models_bytes():
    f = IM.frame(129, 33, seed=5)
    want = IM.model(f, 50, 1).jpg
    b = mijpeg.Batch(144, 48, 1, 50)
    b.upload_any(f, 0)
    for _ in range(2):
        b.encode_interleaved(1, 1)
        assert b.output(0) == want
    # and the three-scan path of the same batch is unharmed by it
    g = IM.pad16(f)
    b.upload(g)
    b.encode(1)
    import oracle as O
    assert b.output(0) == O.cref_encode(g)
    b.close()


# more than 256 MCU rows / intervals / MCUs per row: the second round of every
# per-frame prefix sum (few pixels: one MCU wide or high)
@pytest.mark.parametrize("w,h,rr", [(16, 4112, 1), (10, 4100, 0), (4112, 16, 1)])
def test_more_than_256_rows_or_columns(w, h, rr):
    f = IM.frame(w, h, seed=2)
    got = encode_one(f, 50, rr)
    assert got == IM.model(f, 50, rr).jpg
    assert mijpeg.decode(got, "rgb").shape == (h, w, 3)


def test_more_than_256_stuffing_chunks():
    """entropy data beyond 256 chunks of 4096 bytes (the second round of the
    chunk offsets, several chunks per workgroup): the GPU decoder, independent
    code, must read back the planes K1 left (the model is too slow here)"""
    f = IM.frame(1401, 803, kind="noise")
    b = mijpeg.Batch(1408, 816, 1, 100)
    b.upload_any(f, 0)
    b.encode_interleaved(1, 2)
    got = b.output(0)
    planes = b.coefs(0, diffed=False)
    b.close()
    assert len(got) > 300 * 4096 and got[-2:] == b"\xff\xd9"
    d = mijpeg.Decoder(1408, 816, 1)
    d.decode([got])
    lay = d.layout(0)
    assert (lay["w"], lay["h"], lay["ri"], lay["interleaved"]) == (1401, 803, 2 * 88, 1)
    for c in range(3):
        assert (d.component(0, c) == planes[c].reshape(-1, 64)).all(), c
    d.close()


# a restart interval whose first entropy byte is the first byte of a 4096-byte
# stuffing chunk: that chunk writes its marker (seeds found with the model)
@pytest.mark.parametrize("seed", [0, 5, 45])
def test_interval_begins_on_a_chunk_boundary(seed):
    f = IM.frame(16, 4112, seed=seed)
    m = IM.model(f, 50, 1)
    assert 4096 in m.interval_starts[1:] and m.interval_starts[-1] > 4096
    got = encode_one(f, 50, 1)
    assert got == m.jpg
    # onto an output buffer that held other bytes before: nothing is left over
    b = mijpeg.Batch(16, 4112, 1, 50)
    b.upload_any(IM.frame(16, 4112, kind="noise"), 0)
    b.encode_interleaved(1, 0)
    b.upload_any(f, 0)
    b.encode_interleaved(1, 1)
    got = b.output(0)
    b.close()
    check_stream(got, f, 50, 1)


def test_upload_any_leaves_no_stale_region_sizes():
    """a former region batch, plain again, then one slot padded: the other
    slots are canvas frames for the three-scan path, not the old regions"""
    import oracle as O
    frames = np.stack([IM.frame(64, 48, seed=20), IM.frame(64, 48, seed=21)])
    b = mijpeg.Batch(64, 48, 2, 50)
    b.set_frame_dims([(16, 16), (32, 16)])
    b.set_frame_dims(None)
    b.upload(frames)
    small = IM.frame(20, 20, seed=22)
    b.upload_any(small, 1)
    b.encode(1)
    assert b.output(0) == O.cref_encode(frames[0])
    b.upload_any(frames[0], 0)
    b.encode_interleaved(2, 0)
    check_stream(b.output(0), frames[0], 50, 0)
    check_stream(b.output(1), small, 50, 0)
    b.close()
