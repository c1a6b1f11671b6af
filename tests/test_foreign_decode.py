"""Ordinary baseline JPEG files on the GPU (DESIGN.md "Decoding ordinary
baseline files"): every committed foreign fixture through
mij_decoder_decode / _reconstruct against the plain Python decoder
(foreign_model.py), which tests/test_foreign_model.py pins to libjpeg-turbo.
No test here needs Pillow."""
import os

import numpy as np
import pytest

import decode_cases as DC
import foreign_cases as FC
import mijpeg
import oracle as O
import recipes
import scaled_model as SM

pytestmark = pytest.mark.gpu


def _check_frame(d, i, m):
    assert d.layout(i)["raw"] == m.layout
    assert d.info(i)[:2] == (m.w, m.h)
    for c in range(m.G["ncomp"]):
        assert (d.component(i, c) == m.coefs[c]).all(), ("coefficients", c)


def _check_pixels(d, i, m, order):
    for c in range(m.G["ncomp"]):
        assert (d.plane(i, c) == m.planes[c]).all(), ("plane", c)
    want = m.pixels(order)
    got = d.pixels(i)
    assert got.shape == want.shape and (got == want).all(), int((got != want).any(-1).sum())
    pitch = 3 * m.w + 7
    flat = np.full(m.h * pitch, 0xA5, np.uint8)
    d.pixels(i, pitch=pitch, out=flat)
    rows = flat.reshape(m.h, pitch)
    assert (rows[:, :3 * m.w] == want.reshape(m.h, -1)).all() and (rows[:, 3 * m.w:] == 0xA5).all()


@pytest.mark.parametrize("name", FC.NAMES)
def test_fixture_decodes_as_the_model(name):
    m = FC.model(name)
    d = mijpeg.Decoder((m.w + 15) // 16 * 16, (m.h + 15) // 16 * 16, 1)
    try:
        d.decode([FC.jpg(name)])
        _check_frame(d, 0, m)
        for order in ("rgb", "bgr"):
            d.reconstruct(order)
            _check_pixels(d, 0, m, order)
        ptr, pitch = d.device_pixels(0)
        assert pitch == (3 * m.w + 15) // 16 * 16 and ptr % 16 == 0
        tq = [c[2] for c in m.G["comps"]]
        dqt = d.info(0)[2]
        assert (dqt[:64] == m.dqt[0]).all() and (dqt[64:] == m.dqt[1 if len(tq) > 1 else 0]).all()
    finally:
        d.close()
    assert (mijpeg.decode(FC.jpg(name), "rgb") == m.rgb).all()
    assert (mijpeg.decode(FC.jpg(name)) == m.bgr).all()


MIXED = ["grey_35x21", "sample_64x64", "420_5x5", "444_40x24", "422_35x21", "420_70x37_rst1", "444_17x9",
         "420_70x37_rstrow", "420_96x80_noise_q95", "420_1x1"]


def test_mixed_batch_in_one_call():
    """a legacy stream between frames of every other layout, larger slots
    after smaller ones; the frames' pixels lie back to back on the device, so
    a store past one frame's slot would show in its neighbour"""
    with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
        legacy = f.read()
    streams = [legacy if n == "sample_64x64" else FC.jpg(n) for n in MIXED]
    gold = np.load(os.path.join(recipes.GOLDEN, "sample_64x64.coefs.npz"))
    d = mijpeg.Decoder(96, 80, len(MIXED))
    alone = mijpeg.Decoder(64, 64, 1)
    try:
        alone.decode([legacy])
        alone.reconstruct("rgb")
        d.decode(streams)
        d.reconstruct("rgb")
        li = MIXED.index("sample_64x64")
        for got, want in zip(d.coefs(li), alone.coefs(0)):
            assert (got == want).all()
        for got, k in zip(d.coefs(li), ("Y", "Cb", "Cr")):
            assert (got.ravel() == gold[k].ravel()).all(), k
        for got, want in zip(d.planes(li), alone.planes(0)):
            assert (got == want).all()
        assert (d.pixels(li) == alone.pixels(0)).all()
        lay = d.layout(li)
        assert lay["interleaved"] == 0 and lay["comps"] == [(2, 2, 0, 8, 8), (1, 1, 1, 4, 4), (1, 1, 1, 4, 4)]
        # the legacy frame through the new calls: absolute DCs are the running sum of coefs()' differences
        Y = alone.coefs(0)[0].reshape(-1, 64).astype(np.int64)
        Y[:, 0] = np.cumsum(Y[:, 0])
        assert (d.component(li, 0) == Y).all()
        assert (d.plane(li, 0) == alone.planes(0)[0]).all()
        for i, n in enumerate(MIXED):
            if i == li:
                continue
            m = FC.model(n)
            _check_frame(d, i, m)
            _check_pixels(d, i, m, "rgb")
            with pytest.raises(mijpeg.MijError, match="component"):
                d.coefs(i)
            with pytest.raises(mijpeg.MijError, match="mij_decoder_plane"):
                d.planes(i)
    finally:
        d.close()
        alone.close()


def test_memory_grows_on_first_foreign_stream():
    with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
        legacy = f.read()
    m = FC.model("444_40x24")
    big = FC.model("420_96x80_noise_q95")
    d = mijpeg.Decoder(96, 80, 2)
    try:
        d.decode([legacy])
        d.reconstruct("rgb")
        first = d.pixels(0).copy()
        c0 = [a.copy() for a in d.coefs(0)]
        d.decode([FC.jpg("444_40x24")])
        with pytest.raises(mijpeg.MijError, match="reconstruct"):
            d.pixels(0)  # the newer decode: the old pixels are no longer served
        d.reconstruct("rgb")
        _check_frame(d, 0, m)
        _check_pixels(d, 0, m, "rgb")
        d.decode([FC.jpg("444_40x24"), FC.jpg("420_96x80_noise_q95")])  # the arena grows again
        d.reconstruct("bgr")
        _check_pixels(d, 0, m, "bgr")
        _check_frame(d, 1, big)
        _check_pixels(d, 1, big, "bgr")
        d.decode([legacy])
        d.reconstruct("rgb")
        assert (d.pixels(0) == first).all()
        assert all((a == b).all() for a, b in zip(d.coefs(0), c0))
    finally:
        d.close()


def test_device_pitch_and_neighbours():
    """rows 3*w rounded up to 16 apart; odd-width frames back to back in one
    call: a store past a row's pitch or past a frame's last row would land in
    the next frame's pixels"""
    names = ["420_35x21", "422_5x8", "grey_35x21", "444_17x9", "420_33x17_opt", "422_3x8"]
    d = mijpeg.Decoder(48, 32, len(names))
    try:
        d.decode([FC.jpg(n) for n in names])
        d.reconstruct("rgb")
        addr = []
        for i, n in enumerate(names):
            m = FC.model(n)
            ptr, pitch = d.device_pixels(i)
            assert pitch == (3 * m.w + 15) // 16 * 16 and ptr % 16 == 0
            addr.append((ptr, pitch * m.h))
        for (p0, n0), (p1, _) in zip(addr, addr[1:]):
            assert p1 == p0 + n0  # no gap: each frame's slot ends where the next begins
        for i, n in enumerate(names):
            assert (d.pixels(i) == FC.model(n).rgb).all(), n
    finally:
        d.close()


def test_repeated_decodes_are_identical():
    names = ["420_96x80_noise_q95", "444_24x24_noise_q100"]
    d = mijpeg.Decoder(96, 80, 2)
    try:
        passes = set()
        for _ in range(20):
            d.decode([FC.jpg(n) for n in names])
            passes.add(d.passes())
            d.reconstruct("rgb")
            for i, n in enumerate(names):
                assert (d.pixels(i) == FC.model(n).rgb).all(), n
        assert len(passes) == 1
    finally:
        d.close()


def _legacy_48x32():
    bgr = recipes.noise(32, 48, 21)
    Y, Cb, Cr, _, jpg = O.cref_stages(bgr, 50)
    return DC.Case("noise_48x32_q50", jpg, Y, Cb, Cr, 48, 32)


def test_every_frame_in_one_arena():
    """the encoder's three-scan streams and ordinary files share one set of
    buffers: every frame's pixels begin where the previous frame's end, and a
    three-scan frame reads the same there as in a decoder of its own"""
    legacy = {0: DC.case("noise_16x16_q50"), 2: _legacy_48x32(), 4: DC.case("sample_64x64")}
    foreign = {1: "420_35x21", 3: "grey_35x21"}
    streams = [legacy[i].jpg if i in legacy else FC.jpg(foreign[i]) for i in range(5)]
    size = lambda i: (legacy[i].w, legacy[i].h) if i in legacy else (FC.model(foreign[i]).w, FC.model(foreign[i]).h)
    d = mijpeg.Decoder(64, 64, 5)
    try:
        d.decode(streams)
        d.reconstruct("rgb")
        end = None
        for i in range(5):
            w, h = size(i)
            ptr, pitch = d.device_pixels(i)
            assert pitch == (3 * w + 15) // 16 * 16
            assert end is None or ptr == end, i
            end = ptr + pitch * h
        for i in range(5):
            if i in foreign:
                m = FC.model(foreign[i])
                _check_frame(d, i, m)
                _check_pixels(d, i, m, "rgb")
                with pytest.raises(mijpeg.MijError, match="not of the encoder's layout.*mij_decoder_component"):
                    d.coefs(i)
                with pytest.raises(mijpeg.MijError, match="not of the encoder's layout.*mij_decoder_plane"):
                    d.planes(i)
                continue
            c = legacy[i]
            assert (d.pixels(i) == c.rgb).all(), i
            alone = mijpeg.Decoder(c.w, c.h, 1)
            try:
                alone.decode([c.jpg])
                alone.reconstruct("rgb")
                for got, want, model in zip(d.coefs(i), alone.coefs(0), c.coefs):
                    assert (got == want).all() and (got.ravel() == np.asarray(model).ravel()).all(), i
                for got, want, model in zip(d.planes(i), alone.planes(0), c.planes):
                    assert (got == want).all() and (got == model).all(), i
                assert (d.pixels(i) == alone.pixels(0)).all(), i
            finally:
                alone.close()
        d.reconstruct("rgb", scale=2)
        for i in range(5):
            if i in foreign:
                s = SM.scaled(FC.model(foreign[i]), 2)
            else:
                c = legacy[i]
                s = SM.scaled_legacy(*c.coefs, *c.dqt, c.w, c.h, 2)
            got, want = d.pixels(i), s.pixels("rgb")
            assert got.shape == want.shape and (got == want).all(), i
    finally:
        d.close()


def test_corrupt_one_component_scan_in_a_mixed_call():
    """the first of a three-scan stream's scans cut short, behind an ordinary
    file in the same call: the call fails naming that stream, and the decoder
    goes on working"""
    with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
        jpg = f.read()
    bad = jpg[:330] + jpg[-2:]
    good, m = FC.jpg("420_35x21"), FC.model("420_35x21")
    d = mijpeg.Decoder(64, 64, 2)
    try:
        with pytest.raises(mijpeg.MijError, match="(?i)corrupt") as e:
            d.decode([good, bad])
        assert "stream 1" in str(e.value), str(e.value)
        d.decode([good])
        d.reconstruct("rgb")
        _check_frame(d, 0, m)
        assert (d.pixels(0) == m.rgb).all()
    finally:
        d.close()


def test_refusals_leave_the_decoder_usable():
    """invalid input ends in MIJ_EJPEG with a message; nothing else happens"""
    good, m = FC.jpg("420_35x21"), FC.model("420_35x21")
    cases = dict(FC.rejects())
    # cut inside the scan but closed with an EOI: the headers are sound, the entropy data is short
    plain = FC.jpg("420_96x80_noise_q95")
    cases["short_scan"] = (plain[:len(plain) // 2] + b"\xff\xd9", "corrupt")
    d = mijpeg.Decoder(96, 80, 2)
    try:
        for name, (jpg, word) in sorted(cases.items()):
            with pytest.raises(mijpeg.MijError, match="(?i)" + word) as e:
                d.decode([good, jpg])
            assert "stream 1" in str(e.value), (name, str(e.value))
            with pytest.raises(mijpeg.MijError):
                d.reconstruct("rgb")  # no decoded frames
        d.decode([good])
        d.reconstruct("rgb")
        assert (d.pixels(0) == m.rgb).all()
    finally:
        d.close()
