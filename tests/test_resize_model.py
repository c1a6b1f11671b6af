"""The resampler without a GPU.

The chain: Pillow's Image.resize == the numpy model (resize_model.py) == the
committed digests (tests/golden/resize/manifest.json, for machines without
Pillow) == the library's own arithmetic (csrc/mij_resize.h) run on the host.
The host-only helpers against their committed Pillow tables, and the refusals
that come before any device work.  The GPU side is tests/test_resize_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foreign_cases as FC
import mijpeg
import resize_cases as RC
import resize_model as RM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "jpeg-encoder-decoder_amd")
IDS = [RC.case_id(c) for c in RC.CASES]


def test_the_cases_are_the_eleven_pairs_with_every_filter():
    assert len(RC.PAIRS) == 11 and len(RC.CASES) == 33 and len(set(IDS)) == 33
    assert sorted(RC.manifest()["cases"]) == sorted(IDS)
    # the inputs hold both extremes next to each other and the gradients in between
    px = RC.frame(37, 29)
    assert px.min() == 0 and px.max() == 255 and len(np.unique(px)) > 64


def test_model_equals_pillow():
    Image = RC.pillow()
    if Image is None:
        pytest.skip("Pillow not installed")
    for case in RC.CASES:
        (w, h, ow, oh), f = case
        ref = RC.pillow_resize(Image, RC.frame(w, h), (ow, oh), f)
        got = RC.model(case)
        assert ref.shape == got.shape and (ref == got).all(), (RC.case_id(case), int((ref != got).sum()))


@pytest.mark.parametrize("case", RC.CASES, ids=IDS)
def test_model_equals_committed_digests(case):
    assert RC.digest(RC.model(case)) == RC.manifest()["cases"][RC.case_id(case)]


def test_bicubic_reaches_both_clips():
    """the negative lobes push sums under 0 and over 255 << 22 next to the hard
    edges: without the clip the case's bytes would differ"""
    b, w = RM.axis_table(37, 80, "bicubic")
    src = RC.frame(37, 29).astype(np.int64)[14, :, 0]  # a row through the checkerboard
    acc = np.array([(w[i, :n] * src[x0:x0 + n]).sum() + (1 << 21) for i, (x0, n) in enumerate(b)]) >> 22
    assert acc.min() < 0 and acc.max() > 255


def test_accumulator_bound():
    """255 * sum |weight| + (1 << 21) stays inside int32: far
    inside on these tables, and the library checks every table it builds"""
    worst = 0
    for n_in, n_out in [(p[0], p[2]) for p in RC.PAIRS] + [(p[1], p[3]) for p in RC.PAIRS] + [(180, 167), (4000, 3)]:
        for f in RC.FILTERS:
            _, w = RM.axis_table(n_in, n_out, f)
            worst = max(worst, int(np.abs(w.astype(np.int64)).sum(1).max()))
    assert 255 * worst + (1 << 21) < 2 ** 31
    assert (1 << 22) <= worst < 1.3 * (1 << 22)  # 180 -> 167 BICUBIC: 1.2688, the largest of a sweep of 160000 pairs


@pytest.fixture(scope="module")
def resize_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resize_check") / "resize_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + os.path.join(PKG, "csrc"), "-o",
                           exe, os.path.join(REPO, "tests", "resize_check.cpp")])
    return exe


@pytest.mark.parametrize("case", RC.CASES, ids=IDS)
def test_library_arithmetic_on_the_host_equals_model(case, resize_check, tmp_path):
    """rs_build_axis' tables and rs_tap / rs_clip over them (what the library
    uploads and k_rs_h / k_rs_v run), compiled for the host"""
    (w, h, ow, oh), f = case
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([w, h, ow, oh, RC.FILTERS.index(f)], np.int32).tobytes())
        fh.write(RC.frame(w, h).tobytes())
    subprocess.check_call([resize_check, str(src), str(dst)])
    got = np.fromfile(dst, np.uint8)
    want = RC.model(case)
    assert (got[:want.size] == want.ravel()).all()
    tabs = got[want.size:-8].view(np.int32)
    at = 0
    for n_in, n_out in ((w, ow), (h, oh)):
        if n_in == n_out:
            continue
        b, wt = RM.axis_table(n_in, n_out, f)
        assert wt.shape[1] == RM.ksize(n_in, n_out, f)
        assert (tabs[at:at + b.size] == b.ravel()).all()
        at += b.size
        assert (tabs[at:at + wt.size] == wt.ravel()).all()
        at += wt.size
    assert at == tabs.size


def test_thumbnail_denom_is_pillows_draft_rule():
    rows = RC.manifest()["draft"]
    assert [240, 135, 120, 67, 2] in rows and [240, 135, 30, 16, 8] in rows and len(rows) >= 19
    for w, h, ow, oh, denom in rows:
        assert mijpeg.thumbnail_denom(w, h, ow, oh) == denom, (w, h, ow, oh)
    assert mijpeg.thumbnail_denom(0, 5, 1, 1) == 1 and mijpeg.thumbnail_denom(5, 5, 0, 1) == 1


def test_fit_size_is_pillows_thumbnail_size():
    rows = RC.manifest()["fit"]
    assert len(rows) >= 26
    for w, h, bw, bh, fw, fh in rows:
        assert mijpeg.fit_size(w, h, bw, bh) == (fw, fh), (w, h, bw, bh)
    with pytest.raises(mijpeg.MijError):
        mijpeg.fit_size(10, 10, 0, 5)


def _resize_rc(w, h, ow, oh, f, cap, px=True, stride=None):
    lib = mijpeg.load()
    src = np.zeros((max(h, 1), max(w, 1), 3), np.uint8)
    out = np.zeros(16, np.uint8)
    rc = lib.mij_resize(src.ctypes.data if px else None, w if stride is None else stride, w, h, ow, oh, f,
                        out.ctypes.data, cap)
    return rc, lib.mij_last_message().decode()


def test_resize_refusals_come_before_any_device_work():
    rc, msg = _resize_rc(37, 29, 16, 16, 2, 0)
    assert rc == 4 and str(3 * 16 * 16) in msg  # MIJ_ENOSPC: cap 0 asks for the size
    rc, msg = _resize_rc(37, 29, 16, 16, 2, 3 * 16 * 16 - 1)
    assert rc == 4
    for f in (-1, 3, 7):
        rc, msg = _resize_rc(37, 29, 16, 16, f, 0)
        assert rc == 1 and "filter" in msg, (f, msg)  # MIJ_EINVAL
    for w, h, ow, oh in ((0, 29, 16, 16), (37, 65536, 16, 16), (37, 29, 0, 16), (37, 29, 16, 65536), (37, 29, -4, 16)):
        rc, msg = _resize_rc(w, h, ow, oh, 2, 0)
        assert rc == 1 and "1..65535" in msg, (w, h, ow, oh, msg)
    lib = mijpeg.load()
    wh = (C.c_int * 2)(16, 16)
    im = mijpeg.Image(16, 111, 37, 29)
    assert lib.mij_resizer_resize(None, C.byref(im), wh, 1, 2) == 1 and b"null resizer" in lib.mij_last_message()
    out = np.zeros(16, np.uint8)
    assert lib.mij_resizer_pixels(None, 0, out.ctypes.data, 16, 0) == 1
    assert not lib.mij_resizer_device_pixels(None, 0, None) and lib.mij_last_error() == 1
    assert not lib.mij_resizer_create(0, 0) and lib.mij_last_error() == 1 and b"max_frames" in lib.mij_last_message()


def _thumbnail_rc(jpg, ow, oh, f, q, cap):
    lib = mijpeg.load()
    buf = np.frombuffer(jpg, np.uint8)
    out = np.zeros(16, np.uint8)
    n = C.c_size_t(0)
    rc = lib.mij_thumbnail(buf.ctypes.data, buf.size, ow, oh, f, q, out.ctypes.data, cap, C.byref(n))
    return rc, n.value, lib.mij_last_message().decode()


def test_thumbnail_refusals_come_before_any_device_work():
    jpg = FC.jpg("420_96x80_noise_q95")
    rc, n, msg = _thumbnail_rc(jpg, 20, 17, 2, 75, 0)
    assert rc == 4 and n == mijpeg.max_jpg_bytes_any(20, 17, 0) and str(n) in msg  # MIJ_ENOSPC with the bound
    assert _thumbnail_rc(jpg, 20, 17, 5, 75, 0)[0] == 1 and "filter" in mijpeg.load().mij_last_message().decode()
    rc, _, msg = _thumbnail_rc(jpg, 0, 17, 2, 75, 0)
    assert rc == 1 and "1..65535" in msg
    rc, _, msg = _thumbnail_rc(jpg, 20, 17, 2, 0, 0)
    assert rc == 1 and "quality" in msg
    # what mij_decode refuses, with its message
    rc, _, msg = _thumbnail_rc(FC.jpg("reject_progressive"), 20, 17, 2, 75, 0)
    assert rc == 8 and "baseline" in msg.lower(), (rc, msg)  # MIJ_EJPEG
    with pytest.raises(mijpeg.MijError, match="baseline"):
        mijpeg.thumbnail(FC.jpg("reject_progressive"), (20, 17))
    with pytest.raises(mijpeg.MijError, match="filter"):
        mijpeg.resize(np.zeros((4, 4, 3), np.uint8), (2, 2), "lanczos")
