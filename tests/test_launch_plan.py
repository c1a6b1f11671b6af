"""The launch plans of large batches, asserted and pinned to the oracle.

run_entropy / ent_args (csrc/mij_api.hip) choose the entropy stages' launch
sequence from the frame count, the quality and the geometry:

  frames      segment DCs + tables                          emit / seams
  1 .. 15     k_segdc_actab<dc_last>, no k_tables launch    192 slots, seams fixed in k_emit_scan
  16 .. 42    the same                                      192 slots, k_seam_fix
  43 .. 64    the same                                      48 slots
  65 ..       k_segdc_actab, then k_tables for the DC       48 slots
              tables only (two per frame)

and the pack groups' sizes (32 << ls segments) from the quality, lowered
while the batch has fewer than 1024 groups.  Every test here reads the plan
the encode stored (Batch.last_plan, csrc/mij_testing.h) and asserts the path
it claims before it trusts its bytes, so a threshold that moves fails the
test that named it.  Every output is compared byte for byte with
O.cref_encode (oracle/cpu_ref.c, pinned to the compiled reference by
tests/test_oracle.py).

The slots cycle 7 distinct contents, a period coprime with every group,
window and threshold size, so a wrong per-frame offset lands on another
content's bytes.  The default shape, 496x272: 62 luma block columns (the
last 128-px tile of a row holds 14 of 16), 136 luma and 68 chroma segments
(the last 32-segment pack group of a scan holds 8 and 4), 272 segments (two
segment-DC workgroups per frame), and a noise frame of several 8 KB emit
chunks."""
import functools

import numpy as np
import pytest

import mijpeg
import oracle as O
import recipes

pytestmark = pytest.mark.gpu

W, H = 496, 272
EMIT_CH = 8192  # csrc/mij_internal.h
NOISE = 1  # index of the noise frame in contents()


@functools.lru_cache(maxsize=None)
def contents(h=H, w=W):
    flat = np.empty((h, w, 3), np.uint8)
    flat[:] = (31, 170, 222)
    return (recipes.config3_frame(0, h, w), recipes.noise(h, w, 901), recipes.config3_frame(1, h, w),
            recipes.near_gray(h, w, 5), recipes.config3_frame(2, h, w), flat, recipes.config3_frame(3, h, w))


@functools.lru_cache(maxsize=None)
def wanted(q=50, h=H, w=W):
    """the oracle's stream of each distinct content, computed once"""
    return tuple(O.cref_encode(f, q) for f in contents(h, w))


def slots(n, h=H, w=W):
    c = contents(h, w)
    return np.stack([c[i % 7] for i in range(n)])


def first_diff(a, b):
    m = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:m], np.uint8) != np.frombuffer(b[:m], np.uint8))[0]
    return int(d[0]) if d.size else m


def check_outputs(b, n, want, what=""):
    assert len(b.lengths(n)) == n
    for i in range(n):
        got, ref = b.output(i), want[i % 7]
        assert got == ref, (f"{what}: slot {i} of {n} (content {i % 7}): {len(got)} vs {len(ref)} bytes, "
                            f"first difference at byte {first_diff(got, ref)}; plan {b.last_plan()}")


def assert_plan(b, **fields):
    p = b.last_plan()
    assert {k: p[k] for k in fields} == fields, p
    return p


# the plan of each frame-count range (module docstring)
def range_plan(n):
    if n >= 65:
        return dict(dc_last=0, actab=1, tables=2, segdc=2, emit_slots=48, seam_in_scan=0)
    if n >= 43:
        return dict(dc_last=1, actab=1, tables=0, segdc=2, emit_slots=48, seam_in_scan=0)
    if n >= 16:
        return dict(dc_last=1, actab=1, tables=0, segdc=2, emit_slots=192, seam_in_scan=0)
    return dict(dc_last=1, actab=1, tables=0, segdc=2, emit_slots=192, seam_in_scan=1)


@pytest.fixture(scope="module")
def batch96():
    b = mijpeg.Batch(W, H, 96)
    b.upload(slots(96))
    yield b
    b.close()


def test_plan_record_geometry():
    """The shape's numbers as the module docstring states them."""
    b = mijpeg.Batch(W, H, 1)
    g = b.geometry()
    b.close()
    assert g["nseg"] == 272 and g["tiles_per_frame"] == 4 * (H // 16)
    assert len(wanted()[NOISE]) > 4 * EMIT_CH


def test_frame_counts_across_every_threshold(batch96):
    """96, 64, 65, 16, 96, 15, 65, 1, 96 frames in turn on one batch: both
    sides of the dc_last limit (64 / 65), of the k_seam_fix launch (15 / 16)
    and of the 48-slot emit, each reached from above and from below, so each
    plan runs on the state the others leave (zeroed counts, pack state,
    dcx arrival counters).  The histogram fill is skipped exactly when the
    encode before left at least as many frames zeroed."""
    b, want = batch96, wanted()
    b.set_option("emit_slots", 0)
    b.encode(96)  # (a known state whichever test used the batch before)
    prev = 96
    for n in (96, 64, 65, 16, 96, 15, 65, 1, 96):
        b.encode(n)
        p = assert_plan(b, nframes=n, f0=0, entropy_calls=1, seam=1, ff_pack=1, k1_mode=2,
                        hist_fill_skipped=int(n <= prev), **range_plan(n))
        assert (p["pack_ls_luma"], p["pack_ls_chroma"]) == (0, 0)  # (fewer than 1024 groups)
        check_outputs(b, n, want, f"encode({n}) after encode({prev})")
        prev = n


def test_emit_slots_that_loop(batch96):
    """Fewer emit workgroups per frame than the noise frame has chunks: each
    workgroup writes several chunks in turn, as it does at 3840x2160 with 48
    slots (chunks of EMIT_CH scan bytes before stuffing; the stream's other
    bytes -- headers, tables, stuffed zeros -- stay below the 1 KB + the
    FF 00 pairs subtracted here)."""
    b, want = batch96, wanted()
    nslots = 2
    jpg = want[NOISE]
    chunks_at_least = (len(jpg) - jpg.count(b"\xff\x00") - 1024) // EMIT_CH
    assert chunks_at_least >= 2 * nslots, chunks_at_least
    b.set_option("emit_slots", nslots)
    try:
        b.encode(96)
        assert_plan(b, nframes=96, emit_slots=nslots, dc_last=0, tables=2, seam_in_scan=0)
        check_outputs(b, 96, want, "emit_slots 2")
    finally:
        b.set_option("emit_slots", 0)


@pytest.mark.parametrize("mode", ["q90", "split", "keep_coefs", "rgb"])
def test_above_64_frames_other_pipelines(mode):
    """72 frames, twice (the second encode skips the fills), through the
    pipelines that share run_entropy with the fused Q=50 one."""
    n, q = 72, 90 if mode == "q90" else 50
    want = wanted(q)
    frames = slots(n)
    b = mijpeg.Batch(W, H, n, q, keep_coefs=mode == "keep_coefs")
    try:
        if mode == "split":
            b.set_split(True)
        if mode == "rgb":
            b.set_rgb(True)
            frames = np.ascontiguousarray(frames[..., ::-1])
        b.upload(frames)
        for rep in range(2):
            b.encode(n)
            common = dict(nframes=n, f0=0, entropy_calls=1, dc_last=0, emit_slots=48, seam=1, ff_pack=1,
                          seam_in_scan=0, hist_fill_skipped=rep)
            if mode == "split":  # K1 wrote the segment-first DCs: no k_segdc_actab, all four tables
                assert_plan(b, actab=0, tables=4, segdc=0, k1_mode=6, pack_wide=0, **common)
            else:
                assert_plan(b, actab=1, tables=2, segdc=2, k1_mode=3 if mode == "keep_coefs" else 2,
                            pack_wide=int(mode == "q90"), **common)
            check_outputs(b, n, want, f"{mode} encode {rep}")
        if mode == "q90":
            assert b.replays() > 0
        if mode == "keep_coefs":
            for i in (0, NOISE, n - 1):
                Y, Cb, Cr, _, jpg = O.cref_stages(frames[i], q)
                assert jpg == want[i % 7]
                y, cb, cr = b.coefs(i, diffed=True)
                assert (y == Y).all() and (cb == Cb).all() and (cr == Cr).all(), i
    finally:
        b.close()


def test_overlapped_sub_batches_above_and_below_the_limit():
    """140 frames in 2 sub-batches of 70 (the DC-only tables launch with
    f0 > 0, on the second stream), then in 3 of 47, 47 and 46 (dc_last with
    f0 > 0), then whole again."""
    n, want = 140, wanted()
    b = mijpeg.Batch(W, H, n)
    try:
        b.upload(slots(n))
        b.set_overlap(2)
        b.encode(n)
        assert_plan(b, entropy_calls=2, nframes=70, f0=70, dc_last=0, actab=1, tables=2, emit_slots=48,
                    seam_in_scan=0, hist_fill_skipped=0, k1_mode=2)
        check_outputs(b, n, want, "overlap 2")
        b.set_overlap(3)
        b.encode(n)
        assert_plan(b, entropy_calls=3, nframes=46, f0=94, dc_last=1, actab=1, tables=0, emit_slots=48,
                    seam_in_scan=0, hist_fill_skipped=0, k1_mode=2)
        check_outputs(b, n, want, "overlap 3")
        b.set_overlap(1)
        b.encode(n)
        assert_plan(b, entropy_calls=1, nframes=n, f0=0, dc_last=0, tables=2, hist_fill_skipped=0)
        check_outputs(b, n, want, "whole after overlap")
    finally:
        b.close()


BW, BH, BN = 144, 2064, 256


@pytest.fixture(scope="module")
def bench_plan_frames():
    return slots(BN, BH, BW)


@pytest.mark.parametrize("q,ls", [(50, (2, 3)), (90, (1, 3))])
def test_benchmark_plan_by_automatic_selection(bench_plan_frames, q, ls):
    """What the 256 x 3840x2160 benchmark launches, with no option set, at the
    smallest shape whose host arithmetic selects it: 256 frames of 144x2064
    have 516 luma segments (5 groups of 128, the last of 4; 9 of 64 at Q=90)
    and 258 chroma segments (2 groups of 256, the last of 2), so the batch
    has 1024 groups or more of either kind and keeps the quality's group
    sizes -- luma and chroma groups of different sizes, which no option-less
    small batch reaches.  The last tile of a row holds 2 luma block columns
    and 1 chroma block column."""
    want = wanted(q, BH, BW)
    b = mijpeg.Batch(BW, BH, BN, q)
    try:
        b.upload(bench_plan_frames)
        b.encode(BN)
        assert_plan(b, nframes=BN, f0=0, entropy_calls=1, pack_ls_luma=ls[0], pack_ls_chroma=ls[1],
                    emit_slots=48, dc_last=0, actab=1, tables=2, segdc=2, seam=1, ff_pack=1, seam_in_scan=0,
                    pack_wide=int(q >= 85), k1_mode=2)
        for i in range(BN):
            got, ref = b.output(i), want[i % 7]
            assert got == ref, (f"q{q} slot {i} (content {i % 7}): {len(got)} vs {len(ref)} bytes, first "
                                f"difference at byte {first_diff(got, ref)}")
    finally:
        b.close()
