"""Progressive JPEG files on the GPU: every committed
progressive fixture through a decoder with MIJ_ACCEPT_PROGRESSIVE against the
plain Python model (progressive_model.py, pinned to Pillow and to the
fixtures' baseline twins by tests/test_progressive_model.py), and on through
everything that starts from the coefficient arena.  No test here needs
Pillow."""
import os
import re

import numpy as np
import pytest

import foreign_cases as FC
import mijpeg
import progressive_cases as PC
import recipes
import scaled_model as SM

pytestmark = pytest.mark.gpu


def _dec(m, n=1):
    return mijpeg.Decoder((m.w + 15) // 16 * 16, (m.h + 15) // 16 * 16, n, progressive=True)


def _check_frame(d, i, m):
    assert d.layout(i)["raw"] == m.layout
    assert d.info(i)[:2] == (m.w, m.h)
    for c in range(m.G["ncomp"]):
        assert (d.component(i, c) == m.coefs[c]).all(), ("coefficients", c)


def _check_pixels(d, i, m, order):
    for c in range(m.G["ncomp"]):
        assert (d.plane(i, c) == m.planes[c]).all(), ("plane", c)
    got, want = d.pixels(i), m.pixels(order)
    assert got.shape == want.shape and (got == want).all(), int((got != want).any(-1).sum())


@pytest.mark.parametrize("name", PC.NAMES)
def test_fixture_decodes_as_the_model(name):
    m, e = PC.model(name), PC.MANIFEST["files"][name]
    d = _dec(m)
    try:
        d.decode([PC.jpg(name)])
        _check_frame(d, 0, m)
        assert d.scan_info(0) == {"progressive": True, "nscans": e["nscans"], "levels": e["levels"]}
        assert d.passes() == 0  # self-synchronising passes only
        for order in ("rgb", "bgr"):
            d.reconstruct(order)
            _check_pixels(d, 0, m, order)
        dqt = d.info(0)[2]
        assert (dqt[:64] == m.dqt[0]).all() and (dqt[64:] == m.dqt[1 if m.G["ncomp"] > 1 else 0]).all()
        for scale in (2, 4, 8):
            d.reconstruct("rgb", scale=scale)
            got, want = d.pixels(0), SM.scaled(m, scale).pixels("rgb")
            assert got.shape == want.shape and (got == want).all(), scale
    finally:
        d.close()
    assert (mijpeg.decode(PC.jpg(name), "rgb", progressive=True) == m.rgb).all()


def test_pillow_colour_files_take_ten_scans_in_three_levels():
    m = PC.model("p420_35x21")
    d = _dec(m)
    try:
        d.decode([PC.jpg("p420_35x21")])
        assert d.scan_info(0) == {"progressive": True, "nscans": 10, "levels": 3}
        d.decode([FC.jpg("420_35x21")])
        assert d.scan_info(0) == {"progressive": False, "nscans": 1, "levels": 1}
    finally:
        d.close()


@pytest.mark.parametrize("mapping", [0, 1])
def test_lane_mappings_agree(mapping):
    """one unit per lane and one unit per wave (the default) leave the same planes"""
    names = ["p420_70x37_rst1", "p420_96x80_noise_q95", "m420_35x21_split", "pgrey_35x21"]
    d = mijpeg.Decoder(96, 80, len(names), progressive=True)
    try:
        assert d.lib.mij_test_prog_mapping(d.h_, mapping) == 1
        d.decode([PC.jpg(n) for n in names])
        for i, n in enumerate(names):
            _check_frame(d, i, PC.model(n))
        assert d.lib.mij_test_prog_mapping(d.h_, 1) == mapping and d.lib.mij_test_prog_mapping(d.h_, 2) == -2
    finally:
        d.close()


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0)])
def test_mixed_call(order):
    """a legacy three-scan stream, a baseline file and two progressive files in one call, in both orders of arrival"""
    with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
        legacy = f.read()
    items = [("legacy", legacy, None), ("base", FC.jpg("420_70x37_rstrow"), FC.model("420_70x37_rstrow")),
             ("prog", PC.jpg("p422_35x21"), PC.model("p422_35x21")),
             ("prog", PC.jpg("m420_35x21_split"), PC.model("m420_35x21_split"))]
    items = [items[i] for i in order]
    gold = np.load(os.path.join(recipes.GOLDEN, "sample_64x64.coefs.npz"))
    d = mijpeg.Decoder(80, 64, 4, progressive=True)
    try:
        d.decode([s for _, s, _ in items])
        d.reconstruct("rgb")
        for i, (kind, _, m) in enumerate(items):
            assert d.scan_info(i)["progressive"] == (kind == "prog")
            if kind == "legacy":
                for got, k in zip(d.coefs(i), ("Y", "Cb", "Cr")):
                    assert (got.ravel() == gold[k].ravel()).all(), k
                assert d.scan_info(i) == {"progressive": False, "nscans": 3, "levels": 1}
            else:
                _check_frame(d, i, m)
                _check_pixels(d, i, m, "rgb")
        assert d.passes() > 0
    finally:
        d.close()


def test_transcode_and_transform_equal_the_baseline_twins():
    """progressive in, optimised baseline out: byte for byte what the baseline twin gives"""
    m = PC.model("p420_35x21")
    d = _dec(m, 2)
    try:
        d.decode([PC.jpg("p420_35x21"), FC.jpg("420_35x21")])
        d.transcode()
        assert d.transcoded(0) == d.transcoded(1)
        d.transform("rot90", trim=True)
        assert d.transcoded(0) == d.transcoded(1)
    finally:
        d.close()
    assert mijpeg.transcode(PC.jpg("p420_35x21"), progressive=True) == mijpeg.transcode(FC.jpg("420_35x21"))
    assert (mijpeg.transform(PC.jpg("p420_35x21"), "rot90", trim=True, progressive=True) ==
            mijpeg.transform(FC.jpg("420_35x21"), "rot90", trim=True))


def test_loader_gives_the_twins_tensor():
    files = [PC.jpg("p420_96x80_noise_q95"), FC.jpg("420_96x80_noise_q95")]
    l = mijpeg.Loader(96, 80, 2, progressive=True)
    try:
        t = l.load(files, (40, 32), crops=((5, 3, 80, 70), (5, 3, 80, 70)), mirror=(1, 1))
        assert t.shape == (2, 3, 32, 40) and t[0].tobytes() == t[1].tobytes()
        l.accept(0)
        with pytest.raises(mijpeg.MijError, match="baseline"):
            l.load(files, (40, 32))
    finally:
        l.close()


def test_opt_in_and_refusals_leave_the_decoder_usable():
    """without the bit the same object refuses as ever; with it every illegal script is refused with its reason,
    before any device work, and the decoder goes on working"""
    good, m = PC.jpg("p420_35x21"), PC.model("p420_35x21")
    d = mijpeg.Decoder(48, 32, 2)
    try:
        with pytest.raises(mijpeg.MijError, match="stream 1: SOF 0xC2 is not baseline"):
            d.decode([FC.jpg("420_35x21"), good])
        with pytest.raises(mijpeg.MijError, match="unknown bits"):
            d.accept(2)
        d.accept(mijpeg.ACCEPT_PROGRESSIVE)
        for name, (stream, text) in sorted(PC.refusals().items()):
            with pytest.raises(mijpeg.MijError, match=re.escape("stream 1" + text if text[0] == ":" else "stream 1 " + text)):
                d.decode([good, stream])
            with pytest.raises(mijpeg.MijError):
                d.reconstruct("rgb")  # no decoded frames
        d.decode([good])
        d.reconstruct("rgb")
        _check_frame(d, 0, m)
        assert (d.pixels(0) == m.rgb).all()
        d.accept(0)
        with pytest.raises(mijpeg.MijError, match="SOF 0xC2 is not baseline"):
            d.decode([good])
    finally:
        d.close()


def test_corrupt_streams_end_in_a_status():
    """a refinement scan cut short and an end-of-band run past its scan (progressive_cases.corrupt(): the bytes that
    tests/test_progressive_model.py runs through the same decode routine on the CPU under the sanitizers, with
    the same scan and code expected): MIJ_EJPEG with the status, and the decoder still works"""
    p, m = PC.jpg("p420_35x21"), PC.model("p420_35x21")
    d = _dec(m, 2)
    try:
        for at, (stream, scan, code) in enumerate(PC.corrupt().values()):
            streams = [p, p]
            streams[at] = stream
            with pytest.raises(mijpeg.MijError, match=rf"stream {at} scan {scan}: corrupt entropy data \({code}\)"):
                d.decode(streams)
            with pytest.raises(mijpeg.MijError):
                d.layout(0)  # no decoded frames
        d.decode([p])
        _check_frame(d, 0, m)
    finally:
        d.close()


def test_repeated_decodes_are_identical():
    names = ["p420_96x80_noise_q95", "p420_70x37_rst1", "pgrey_35x21"]
    d = mijpeg.Decoder(96, 80, 3, progressive=True)
    try:
        arenas = []
        for _ in range(2):
            d.decode([PC.jpg(n) for n in names])
            arenas.append([d.component(i, c).copy() for i, n in enumerate(names) for c in range(PC.model(n).G["ncomp"])])
        assert all((a == b).all() for a, b in zip(*arenas))
        for i, n in enumerate(names):
            _check_frame(d, i, PC.model(n))
    finally:
        d.close()


def test_host_tools_progressive_option(tmp_path):
    """host/decode_jpg --progressive (full size and -scale 1/2) writes the model's pixels as a PPM; without the
    option it refuses the file; host/transcode_jpg --progressive writes the baseline twin's transcode"""
    import subprocess

    import ppm
    host = os.path.join(os.path.dirname(mijpeg.LIB_PATH), "host")
    src, m = os.path.join(PC.DIR, "p420_70x37_rstrow.jpg"), PC.model("p420_70x37_rstrow")
    out = str(tmp_path / "out.ppm")
    subprocess.run([os.path.join(host, "decode_jpg"), "--progressive", src, out], check=True, timeout=120)
    with open(out, "rb") as f:
        assert f.read() == ppm.ppm_bytes(m.rgb)
    subprocess.run([os.path.join(host, "decode_jpg"), "--progressive", "-scale", "1/2", src, out], check=True, timeout=120)
    with open(out, "rb") as f:
        assert f.read() == ppm.ppm_bytes(SM.scaled(m, 2).rgb)
    r = subprocess.run([os.path.join(host, "decode_jpg"), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not baseline" in r.stderr
    jpg = str(tmp_path / "out.jpg")
    subprocess.run([os.path.join(host, "transcode_jpg"), "--progressive", src, jpg, "1"], check=True, timeout=120)
    with open(jpg, "rb") as f:
        assert f.read() == mijpeg.transcode(FC.jpg("420_70x37_rstrow"), 1)
    r = subprocess.run([os.path.join(host, "transcode_jpg"), src, jpg], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not baseline" in r.stderr
