"""DC-only chroma segments without a token stream.

Where K1's all-AC-zero test passes for a chroma N-tile, a plain frame batch
stores no tokens for its Cb and Cr segments: seg_ntok carries the count with
bit 31 set, and the packing builds "DC difference, EOB" per block from the raw
DC plane.  Every case asserts the plan's dc_only field, then which segments
kept a stream -- Batch.token_count counts stored tokens only, so it must equal
the oracle's token total of the segments expected to keep one -- then the
bytes against O.cref_encode."""
import functools

import numpy as np
import pytest

import mijpeg
import oracle as O
import recipes

pytestmark = pytest.mark.gpu

W, H = 272, 64  # three tile columns, the last with one MCU; 12 chroma segments per plane: one pack group


@functools.lru_cache(maxsize=None)
def grey(w=W, h=H, seed=3):
    """grey texture: the chroma planes are flat but for the colour truncation's +-1"""
    v = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    return np.repeat(v[..., None], 3, axis=2)


@functools.lru_cache(maxsize=None)
def patched(w=W, h=H):
    """the same with one saturated textured MCU: the chroma N-tile of tile
    (row 1, column 0) fails the all-AC-zero test between flagged neighbours"""
    f = grey(w, h).copy()
    c = np.random.default_rng(9).integers(0, 2, (16, 16, 3), dtype=np.uint8) * 255
    f[16:32, 48:64] = c
    return f


def block_tokens(P):
    """tokens per block of a zigzag plane: DC, the nonzero ACs, EOB unless position 63 is set"""
    B = P.reshape(-1, 64)
    return 1 + (B[:, 1:] != 0).sum(1) + (B[:, 63] == 0)


def stored_tokens(frame, q, flagging):
    """the oracle's count of the tokens that keep a stream: all of luma, and
    of chroma the segments (8 blocks of an MCU row inside one 128-px tile, Cb
    and Cr together as K1 tests them) with any nonzero AC -- every chroma
    segment when K1's test is off"""
    Y, Cb, Cr = O.cref_stages(frame, q)[:3]
    h, w = frame.shape[:2]
    n = int(block_tokens(Y).sum())
    tb, tr = block_tokens(Cb).reshape(h // 16, w // 16), block_tokens(Cr).reshape(h // 16, w // 16)
    ab = (Cb.reshape(-1, 64)[:, 1:] != 0).any(1).reshape(h // 16, w // 16)
    ar = (Cr.reshape(-1, 64)[:, 1:] != 0).any(1).reshape(h // 16, w // 16)
    flagged = 0
    for x0 in range(0, w // 16, 8):
        for r in range(h // 16):
            keep = not flagging or ab[r, x0:x0 + 8].any() or ar[r, x0:x0 + 8].any()
            if keep:
                n += int(tb[r, x0:x0 + 8].sum() + tr[r, x0:x0 + 8].sum())
            else:
                flagged += 2
    return n, flagged


def run(frames, q, overlap=0, split=False):
    n, h, w = frames.shape[:3]
    b = mijpeg.Batch(w, h, n, q)
    try:
        if overlap:
            b.set_overlap(overlap)
        if split:
            b.set_split(True)
        b.upload(frames)
        b.encode(n)
        return [b.output(i) for i in range(n)], b.last_plan(), b.token_count(n)
    finally:
        b.close()


def check(frames, q, flagging, want_flagged=None, **kw):
    got, plan, ntok = run(frames, q, **kw)
    assert plan["dc_only"] == int(flagging), plan
    want = [stored_tokens(f, q, flagging) for f in frames]
    if want_flagged is not None:
        assert [w[1] for w in want] == want_flagged
    assert ntok == sum(w[0] for w in want), (ntok, want)
    for i, g in enumerate(got):
        ref = O.cref_encode(frames[i], q)
        assert g == ref, f"frame {i}: {len(g)} vs {len(ref)} bytes"
    return plan


def test_grey_frame_every_chroma_segment_flagged():
    check(grey()[None], 50, True, want_flagged=[24])


def test_one_unflagged_tile_among_flagged_neighbours():
    check(patched()[None], 50, True, want_flagged=[22])


def test_single_mcu_tile_odd_block_count():
    """144x32: the second tile column holds one MCU, so its chroma segments
    have one block -- two tokens and two LB_NOTOK slots"""
    check(grey(144, 32, 5)[None], 50, True, want_flagged=[8])


def test_q90_flags_nothing():
    """the all-AC-zero test is off above Q=75 and the host leaves dc_only off
    at the wide pack window's qualities: every segment keeps its stream"""
    check(np.stack([grey(), patched()]), 90, False)


def test_overlapped_sub_batches():
    frames = np.stack([(grey(), patched(), recipes.noise(H, W, 50 + i), grey(W, H, 20 + i))[i % 4] for i in range(17)])
    plan = check(frames, 50, True, overlap=2)
    assert plan["entropy_calls"] == 2 and plan["f0"] == 9, plan


def test_split_pipeline_is_off():
    frames = np.stack([grey(), patched()])
    got, plan, _ = run(frames, 50, split=True)
    assert plan["dc_only"] == 0 and plan["k1_mode"] == 6, plan
    for i, g in enumerate(got):
        assert g == O.cref_encode(frames[i], 50), i


def test_region_batch_is_off():
    frame = patched()
    regions = [(0, 0, W, H), (16, 0, 144, 32), (32, 16, 48, 48), (128, 32, 144, 32)]
    got = mijpeg.encode_regions(frame, regions, 50)
    plan = mijpeg.regions_last_plan()
    assert plan["dc_only"] == 0, plan
    for r, g in zip(regions, got):
        assert g == O.cref_encode(frame, 50, r), r
