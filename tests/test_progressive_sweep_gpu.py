"""The sweep of random scan scripts on the GPU (DESIGN.md §4p,
tests/progressive_sweep.py): the decoder must return the planes each stream
was written from, in calls of 16 frames that mix samplings, kinds of content,
scripts, level counts and sizes, under both lane mappings, and everything
downstream of the arena (pixels, reduced IDCTs, both transcoders) must agree
with its model on content no photograph gives.  Equality of bytes everywhere,
no tolerance.  tests/test_progressive_sweep_model.py runs the same streams
through the models and the shared routine on the CPU; no mutated stream comes
here, and no test here needs Pillow."""
import os

import numpy as np
import pytest

import foreign_cases as FC
import mijpeg
import progressive_model as PM
import progressive_sweep as S
import progwrite_cases as WC
import progwrite_model as W
import recipes
import scaled_model as SM

pytestmark = pytest.mark.gpu

CASES = S.cases()
CALLS = [CASES[i::6] for i in range(6)]  # 16 frames each, neighbours of the list in different calls
# one case of every sampling x kind, then the named ones without the 1x1 frames
PAIRS = [CASES[4 * i + 1] for i in range(20)]
SUBSET = PAIRS + CASES[84:]


def _decoder(n):
    return mijpeg.Decoder(112, 80, n, progressive=True)


def _check_frame(d, i, case):
    m = PM.decoded(case.stream)
    assert d.layout(i)["raw"] == m.layout, case
    w, h, dqt = d.info(i)
    assert (w, h) == (case.w, case.h), case
    assert (dqt[:64] == m.dqt[0]).all() and (dqt[64:] == m.dqt[1 if case.G["ncomp"] > 1 else 0]).all(), case
    assert d.scan_info(i) == {"progressive": True, "nscans": len(case.script), "levels": case.levels}, case
    for c, want in enumerate(case.coefs):
        got = d.component(i, c)
        assert got.shape == want.shape and (got == want).all(), (case, c, int((got != want).any(1).sum()))


def test_the_lists_are_what_the_tests_assume():
    assert len(CASES) == 96 and all(len(call) == 16 for call in CALLS)
    assert {(c.sampling, c.kind) for c in PAIRS} == {(s, k) for s in S.SAMPLINGS for k in S.KINDS}
    assert len(SUBSET) == 32 and len({c.name for c in SUBSET}) == 32
    for call in CALLS:
        assert len({c.sampling for c in call}) == 4 and len({c.kind for c in call}) >= 4
        assert len({c.levels for c in call}) >= 2 and len({len(c.script) for c in call}) >= 8
    # a level of some call holds more than one workgroup of units under the one-unit-per-lane mapping, and its
    # last workgroup is not full (the units of a level: every restart interval of every scan of that level)
    tails = []
    for call in CALLS:
        per = {}
        for c in call:
            for lv, (comps, _, _, _, _, ri) in zip(S.levels(c.script), c.script):
                per[lv] = per.get(lv, 0) + (-(-S.scan_mcus(c.G, comps) // ri) if ri else 1)
        tails += [n for n in per.values() if n > 64 and n % 64]
    assert tails


@pytest.mark.parametrize("mapping", [0, 1])
@pytest.mark.parametrize("call", range(6))
def test_decode_returns_the_planes(call, mapping):
    """... and again on the same object with the frames in reverse order: nothing of the first call's arena, units
    or tables may show"""
    frames = CALLS[call]
    d = _decoder(16)
    try:
        assert d.lib.mij_test_prog_mapping(d.h_, mapping) == 1
        for order in (frames, frames[::-1]):
            d.decode([c.stream for c in order])
            assert d.passes() == 0  # self-synchronising passes only
            for i, c in enumerate(order):
                _check_frame(d, i, c)
    finally:
        d.close()


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0)])
def test_mixed_with_baseline(order):
    """sweep frames between a legacy three-scan stream and a baseline file, in both orders of arrival"""
    with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
        legacy = f.read()
    gold = np.load(os.path.join(recipes.GOLDEN, "sample_64x64.coefs.npz"))
    sweep = [S.by_name(n) for n in ("rst1_420_small_100x70", "al3_chain_444_dense_35x21", "grey_h2v2_dense_100x70",
                                    "dc_swing_422_sparse_70x37")]
    items = [("legacy", legacy, None)] + [("sweep", c.stream, c) for c in sweep]
    items.append(("base", FC.jpg("420_70x37_rstrow"), FC.model("420_70x37_rstrow")))
    items = [items[i] for i in order]
    d = _decoder(len(items))
    try:
        d.decode([s for _, s, _ in items])
        d.reconstruct("rgb")
        for i, (kind, _, m) in enumerate(items):
            if kind == "legacy":
                for got, k in zip(d.coefs(i), ("Y", "Cb", "Cr")):
                    assert (got.ravel() == gold[k].ravel()).all(), k
                assert d.scan_info(i) == {"progressive": False, "nscans": 3, "levels": 1}
            elif kind == "base":
                assert d.scan_info(i) == {"progressive": False, "nscans": 1, "levels": 1}
                for c in range(3):
                    assert (d.component(i, c) == m.coefs[c]).all(), c
                assert (d.pixels(i) == m.rgb).all()
            else:
                _check_frame(d, i, m)
                assert (d.pixels(i) == PM.decoded(m.stream).rgb).all(), m
        assert d.passes() > 0
    finally:
        d.close()


@pytest.mark.parametrize("call", range(6))
def test_pixels_are_the_models(call):
    """dense included: out there the model's plain clamp is the definition"""
    frames = CALLS[call]
    d = _decoder(16)
    try:
        d.decode([c.stream for c in frames])
        for order in ("rgb", "bgr"):
            d.reconstruct(order)
            for i, case in enumerate(frames):
                m = PM.decoded(case.stream)
                for c in range(m.G["ncomp"]):
                    assert (d.plane(i, c) == m.planes[c]).all(), (case, "plane", c)
                got, want = d.pixels(i), m.pixels(order)
                assert got.shape == want.shape and (got == want).all(), (case, order, int((got != want).any(-1).sum()))
    finally:
        d.close()


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_scaled_pixels_are_the_models(scale):
    d = _decoder(len(PAIRS))
    try:
        d.decode([c.stream for c in PAIRS])
        d.reconstruct("rgb", scale=scale)
        for i, case in enumerate(PAIRS):
            got, want = d.pixels(i), SM.scaled(PM.decoded(case.stream), scale).pixels("rgb")
            assert got.shape == want.shape and (got == want).all(), (case, int((got != want).any(-1).sum()))
    finally:
        d.close()


def _decoded_planes(streams, progressive):
    out = []
    for k in range(0, len(streams), 16):
        d = mijpeg.Decoder(112, 80, 16, progressive=progressive)
        try:
            part = streams[k:k + 16]
            d.decode(part)
            for i in range(len(part)):
                out.append([d.component(i, c) for c in range(d.layout(i)["ncomp"])])
        finally:
            d.close()
    return out


@pytest.mark.parametrize("rr", [0, 1])
def test_out_again_as_a_progressive_file(rr):
    """k_pw_* on all-nonzero blocks, ZRL chains and all-zero frames: the model's bytes, and they decode to the
    planes wherever a progressive file of libjpeg's script carries them"""
    outs = []
    for case in SUBSET:
        got = mijpeg.transcode(case.stream, rr, progressive=True, output="progressive")
        want = W.model(case.stream, rr)
        assert len(got) == len(want) and got == want, case
        outs.append(got)
    for case, planes in zip(SUBSET, _decoded_planes(outs, True)):
        for c, src in enumerate(case.coefs):
            want, got = WC.coded_inside(src, planes[c], case.G, c)
            assert (want[0] == got[0]).all() and (want[1] == got[1]).all(), (case, c)


def test_out_again_as_a_baseline_file():
    outs = [mijpeg.transcode(case.stream, progressive=True) for case in SUBSET]
    for case, planes in zip(SUBSET, _decoded_planes(outs, False)):
        for c, src in enumerate(case.coefs):
            assert planes[c].shape == src.shape and (planes[c] == src).all(), (case, c)
