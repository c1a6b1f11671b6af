"""The baseline sweep on the GPU (DESIGN.md §4f "The sweep",
tests/baseline_sweep.py): k_dec_sync, k_dec_scan and k_dec_write, in both
their forms, must return the planes each stream was written from -- under
crafted Huffman tables, restart intervals of every kind and both stream
shapes, in calls of 16 frames that mix them -- and everything downstream of
the arena (pixels, reduced IDCTs, both transcoders, transforms) must agree
with its model on the same truth.  Then the DC range of the transcoder
(DESIGN.md §4h): what leaves it is a file that decodes to the source's
planes, or nothing.  Equality of bytes everywhere, no tolerance; no mutated
stream comes here, and no test here needs Pillow.
tests/test_baseline_sweep_model.py holds the census of what these streams put
in front of the decoder, and runs them through the models on the CPU."""
import numpy as np
import pytest

import baseline_sweep as B
import foreign_model as FM
import mijpeg
import progressive_sweep as S
import progwrite_model as W
import scaled_model as SM
import transcode_model as TM
import transform_model as XM

pytestmark = pytest.mark.gpu

CASES = B.cases()
CALLS = [CASES[i::3] for i in range(3)]  # 16 frames each, neighbours of the list in different calls
IL = [c for c in CASES if c.shape == "interleaved"]
TS = [c for c in CASES if c.shape == "three_scan"]
# one case of every sampling x kind, and three of the encoder's shape
PAIRS = [next(c for c in IL if (c.sampling, c.kind) == (s, k)) for s in S.SAMPLINGS for k in S.KINDS] + TS[::3]
# twelve interleaved frames for the progressive writer and the transforms: the named ones, one more of every
# sampling that is at least 21 pixels either way, and one under the "edge" tables
_NAMED = [c for c in IL if c.name.split("_")[0] in ("aligned", "rst1", "every", "dc", "fib", "ff")]
_ROOMY = [c for c in IL if c not in _NAMED and min(c.w, c.h) >= 21]
SUBSET = _NAMED + [next(c for c in _ROOMY if c.sampling == s) for s in S.SAMPLINGS]
SUBSET.append(next(c for c in _ROOMY if c.tables == "edge" and c not in SUBSET))


def _decoder(n):
    return mijpeg.Decoder(144, 144, n)


def _check_frame(d, i, case):
    assert d.layout(i)["raw"] == FM.layout_list(case.G), case
    w, h, dqt = d.info(i)
    assert (w, h) == (case.w, case.h), case
    assert (dqt[:64] == np.asarray(case.dqt[0])).all() and (dqt[64:] == np.asarray(case.dqt[1])).all(), case
    three = case.shape == "three_scan"
    assert d.scan_info(i) == {"progressive": False, "nscans": 3 if three else 1, "levels": 1}, case
    if three:
        for c, (got, want) in enumerate(zip(d.coefs(i), case.diffed())):
            assert got.shape == want.shape and (got == want).all(), (case, c, int((got != want).sum()))
    else:
        for c, want in enumerate(case.coefs):
            got = d.component(i, c)
            assert got.shape == want.shape and (got == want).all(), (case, c, int((got != want).any(1).sum()))


def test_the_lists_are_what_the_tests_assume():
    assert len(CASES) == 48 and all(len(call) == 16 for call in CALLS)
    assert len(SUBSET) == 12 and len({c.name for c in SUBSET}) == 12 and len(_NAMED) == 7
    assert len(PAIRS) == 23 and {c.sampling for c in SUBSET} == set(S.SAMPLINGS)
    for call in CALLS:
        assert len({c.sampling for c in call}) == 4 and len({c.kind for c in call}) == 5
        assert {c.tables for c in call} == set(B.TABLES) and len({c.ri for c in call}) >= 4
        # the two shapes alternate in arrival order (the host stages one-block-MCU scans first): three three-scan
        # frames, each between interleaved ones
        shape = [c.shape == "three_scan" for c in call]
        assert sum(shape) == 3 and not shape[0] and not shape[-1]
        assert all(not (a and b) for a, b in zip(shape, shape[1:]))
        assert sum(1 for a, b in zip(shape, shape[1:]) if a != b) == 6
    # some call holds more than one workgroup of chunks (256) in its interleaved scans
    chunks = [sum(-(-iv["nbits"] // B.CHUNK) for c in call if c.shape == "interleaved" for iv in c.bitmap["intervals"])
              for call in CALLS]
    assert max(chunks) > 256 and all(n % 256 for n in chunks)


@pytest.mark.parametrize("call", range(3))
def test_decode_returns_the_planes(call):
    """... and again on the same object with the frames in reverse order: nothing of the first call's arena,
    intervals or tables may show"""
    frames = CALLS[call]
    d = _decoder(16)
    try:
        for order in (frames, frames[::-1]):
            d.decode([c.stream for c in order])
            for i, c in enumerate(order):
                _check_frame(d, i, c)
    finally:
        d.close()


@pytest.mark.parametrize("call", range(3))
def test_pixels_are_the_models(call):
    """dense included: out there the model's plain clamp is the definition.  A three-scan frame's
    model is foreign_model on its interleaved twin: the same planes, and pixels are a function of the planes"""
    frames = CALLS[call]
    d = _decoder(16)
    try:
        d.decode([c.stream for c in frames])
        for order in ("rgb", "bgr"):
            d.reconstruct(order)
            for i, case in enumerate(frames):
                got, want = d.pixels(i), FM.decoded(case.twin).pixels(order)
                assert got.shape == want.shape and (got == want).all(), (case, order, int((got != want).any(-1).sum()))
    finally:
        d.close()


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_scaled_pixels_are_the_models(scale):
    """scaled_model on the truth planes (for a three-scan frame what scaled_legacy builds from the differences)"""
    d = _decoder(len(PAIRS))
    try:
        d.decode([c.stream for c in PAIRS])
        d.reconstruct("rgb", scale=scale)
        for i, case in enumerate(PAIRS):
            comps = [(hs, vs, bw, bh) for hs, vs, _, bw, bh in case.G["comps"]]
            dqt = [case.dqt[1 if c else 0] for c in range(len(comps))]
            want = SM.Scaled(case.w, case.h, comps, case.coefs, dqt, scale).pixels("rgb")
            got = d.pixels(i)
            assert got.shape == want.shape and (got == want).all(), (case, int((got != want).any(-1).sum()))
    finally:
        d.close()


def _decoded_planes(streams, progressive=False):
    out = []
    for k in range(0, len(streams), 16):
        d = mijpeg.Decoder(144, 144, 16, progressive=progressive)
        try:
            part = streams[k:k + 16]
            d.decode(part)
            for i in range(len(part)):
                out.append([d.component(i, c) for c in range(d.layout(i)["ncomp"])])
        finally:
            d.close()
    return out


@pytest.mark.parametrize("rr", [0, 1, 2])
def test_transcode_is_the_models_bytes(rr):
    """transcode_model.build of the truth planes, for both shapes (a three-scan stream's is model_legacy's path: the
    same build), whatever interval the source had; and the result decodes on the GPU back to the planes"""
    outs = []
    for case in CASES:
        comps, hv = case.sof
        want = TM.build(case.w, case.h, comps, hv, case.dqt_by_id, case.wide, rr)
        got = mijpeg.transcode(case.stream, rr)
        assert len(got) == len(want) and got == want, case
        outs.append(got)
    for case, planes in zip(CASES, _decoded_planes(outs)):
        for c, want in enumerate(case.coefs):
            assert planes[c].shape == want.shape and (planes[c] == want).all(), (case, c)


@pytest.mark.parametrize("rr", [0, 1])
def test_out_as_a_progressive_file(rr):
    for case in SUBSET:
        got = mijpeg.transcode(case.stream, rr, output="progressive")
        want = W.model(case.stream, rr)
        assert len(got) == len(want) and got == want, case


@pytest.mark.parametrize("op", ["flip_h", "rot90"])
def test_transforms_are_the_models_bytes(op):
    """with trim; where the model refuses (4:2:2 under a quarter turn, a frame narrower than an MCU), so must the
    library"""
    served = 0
    for case in SUBSET:
        try:
            want = XM.model(case.stream, op, trim=True, restart_rows=1)
        except XM.Refused:
            with pytest.raises(mijpeg.MijError):
                mijpeg.transform(case.stream, op, trim=True, restart_rows=1)
            continue
        got = mijpeg.transform(case.stream, op, trim=True, restart_rows=1)
        assert len(got) == len(want) and got == want, case
        served += 1
    assert served >= 9


# ---- the DC range ---------------------------------------------------------------
def _quarter_of_dc_only(dc):
    """the 16 x 16 pixels of an 8 x 8-block greyscale frame of DC-only blocks under an all-ones DQT at 1/4 scale, by
    §4e's wrap rule: jpeg_idct_2x2 with every sum modulo 2^32, converted back for the arithmetic shifts.  Beyond
    |DC| = 16384 the row pass's (DC * 4) << 15 leaves int32, where scaled_model's int64 is not the definition"""
    def wrap(x):
        return ((x + (1 << 31)) % (1 << 32)) - (1 << 31)
    dc = np.asarray(dc, np.int64)
    col = wrap((dc << 15) + (1 << 12)) >> 13
    px = np.clip((wrap((col << 15) + (1 << 19)) >> 20) + 128, 0, 255).astype(np.uint8)
    y = np.repeat(np.repeat(px.reshape(8, 8), 2, 0), 2, 1)
    return np.repeat(y[:, :, None], 3, 2)


def test_dc_range():
    """(a) a ramp to +-30000, (b) neighbours at +30000 and -30000, (c) sums that leave int16, twice (a): decode
    returns the planes (the sums modulo 2^16), the pixels are the model's of those planes at every scale, and a
    transcode is the model's bytes wherever every difference of the new scan has a category of at most 15 and is
    refused for that frame alone wherever one has 16: (b) always, (c) unless an interval starts where it wraps"""
    a, b, c = B.dc_range_cases()
    frames = [a, b, c, a]
    # the wrap-aware quarter-scale rule is scaled_model's wherever nothing wraps
    tame = np.zeros((64, 64), np.int16)
    tame[:, 0] = np.arange(-16384, 16384, 512)
    assert (_quarter_of_dc_only(tame[:, 0]) == SM.Scaled(64, 64, [(1, 1, 8, 8)], [tame], [a.dqt[0]], 4).pixels("rgb")).all()
    d = mijpeg.Decoder(64, 64, 4)
    try:
        d.decode([x.stream for x in frames])
        for i, case in enumerate(frames):
            _check_frame(d, i, case)
        for scale in (1, 2, 4, 8):
            d.reconstruct("rgb", scale=scale)
            for i, case in enumerate(frames):
                if scale == 1:
                    want = FM.decoded(case.stream).rgb
                elif scale == 4:
                    want = _quarter_of_dc_only(case.coefs[0][:, 0])
                else:
                    want = SM.Scaled(64, 64, [(1, 1, 8, 8)], case.coefs, [case.dqt[0]], scale).pixels("rgb")
                assert (d.pixels(i) == want).all(), (case, scale)
        served = {}
        for rr, refused in ((0, (1, 2)), (1, (1,)), (2, (1,))):
            d.transcode(rr)
            for i, case in enumerate(frames):
                if i in refused:
                    for read in (d.transcoded, d.device_transcoded):
                        with pytest.raises(mijpeg.MijError, match=rf" {i}: a DC difference of category 16"):
                            read(i)
                else:
                    got = d.transcoded(i)
                    assert got == TM.model(case.stream, rr), (case, rr)
                    served[(case.name, rr)] = (case, got)
        assert sorted(served) == [(a.name, 0), (a.name, 1), (a.name, 2), (c.name, 1), (c.name, 2)]
    finally:
        d.close()
    pairs = list(served.values())
    for (case, _), planes in zip(pairs, _decoded_planes([s for _, s in pairs])):
        assert (planes[0] == case.coefs[0]).all(), case
    # the one-shot call fails as a whole; a transform is the same coder
    for call in (lambda: mijpeg.transcode(b.stream, 0), lambda: mijpeg.transcode(c.stream, 0),
                 lambda: mijpeg.transform(b.stream, "flip_h")):
        with pytest.raises(mijpeg.MijError, match="a DC difference of category 16"):
            call()
    # a progressive file's first DC scan codes the DCs halved: its differences never need more than category 15
    got = mijpeg.transcode(b.stream, 0, output="progressive")
    assert got == W.model(b.stream, 0)
    (planes,) = _decoded_planes([got], progressive=True)
    assert (planes[0] == b.coefs[0]).all()
