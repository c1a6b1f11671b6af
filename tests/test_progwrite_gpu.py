"""Progressive output on the GPU: the kernels' bytes are the
model's (tests/progwrite_model.py, pinned to Pillow's bytes and to the shared
per-block routines by tests/test_progwrite_model.py).  Equality of bytes
everywhere, no tolerance.  The inputs are the small fixtures: every sampling,
1x1, partial MCUs, baseline and progressive sources, the two files that cut an
EOB run at its limits (more than 937 buffered correction bits; 0x7FFF blocks,
which is also 129 workgroups of blocks and 516 steps of the run stage)."""
import os
import re
import subprocess

import numpy as np
import pytest

import mijpeg
import progressive_model as PM
import progwrite_cases as WC
import progwrite_model as W

pytestmark = pytest.mark.gpu


def same(got: bytes, want: bytes):
    assert len(got) == len(want), (len(got), len(want))
    assert got == want


def is_prog(name: str) -> bool:
    return name in WC.PILLOW or name in WC.LIMITS


# 1. baseline and progressive sources, restart_rows 0, 1, 2
@pytest.mark.parametrize("rr", [0, 1, 2])
@pytest.mark.parametrize("name", WC.BASELINE + WC.TWINS)
def test_fixture_is_the_model(name, rr):
    src = WC.jpg(name)
    same(mijpeg.transcode(src, rr, progressive=is_prog(name), output="progressive"), W.model(src, rr))


# 2. the limits of a run; a photograph of 12 870 blocks (51 workgroups, runs carried over many steps of the run stage)
@pytest.mark.parametrize("name,rr", [("corr_limit", 0), ("corr_limit", 3), ("run_limit", 0), ("420_1040x520_q30", 0),
                                     ("p420_1040x520_q30", 3)])
def test_run_limits(name, rr):
    src = WC.jpg(name)
    same(mijpeg.transcode(src, rr, progressive=True, output="progressive"), W.model(src, rr))


# 3. transforms: the model applied to the coefficients the baseline transform of the same call reports
@pytest.mark.parametrize("name,op,trim,crop,rr", [("420_70x37_rstrow", "rot90", True, None, 1),
                                                  ("420_96x80_noise_q95", "none", False, (16, 16, 50, 37), 0),
                                                  ("444_17x9", "rot90", True, None, 0)])
def test_transforms(name, op, trim, crop, rr):
    d = mijpeg.Decoder(96, 80, 1)
    try:
        d.decode([WC.jpg(name)])
        d.transform(op, trim, crop, rr)
        base = d.transcoded(0)
        d.output("progressive")
        d.transform(op, trim, crop, rr)
        same(d.transcoded(0), W.model(base, rr))
        d.output("baseline")  # sticky until changed: then today's bytes again
        d.transform(op, trim, crop, rr)
        same(d.transcoded(0), base)
    finally:
        d.close()


# 4. round trip on the device
@pytest.mark.parametrize("name", WC.BASELINE + ["pgrey_35x21", "corr_limit"])
def test_round_trip(name):
    src = WC.jpg(name)
    out = mijpeg.transcode(src, 1, progressive=is_prog(name), output="progressive")
    d = mijpeg.Decoder(256, 80, 2, progressive=True)
    try:
        d.decode([src, out])
        la, lb = d.layout(0), d.layout(1)
        assert la["raw"][:7] == lb["raw"][:7] and la["comps"] == lb["comps"]
        info = d.scan_info(1)
        assert info["progressive"] and info["nscans"] == (10 if la["ncomp"] == 3 else 6)
        G = W.geometry(la["w"], la["h"], [c[:2] for c in la["comps"]])
        for c in range(la["ncomp"]):
            want, got = WC.coded_inside(d.component(0, c), d.component(1, c), G, c)
            assert (want[0] == got[0]).all() and (want[1] == got[1]).all(), c
        d.reconstruct("rgb")
        assert (d.pixels(0) == d.pixels(1)).all()
    finally:
        d.close()


# 5. frames of different samplings and sizes in one call; baseline again afterwards
def test_mixed_call_and_back_to_baseline():
    names = ["grey_35x21", "p444_17x9", "422_35x21", "p420_70x37_rstrow", "420_96x80_noise_q95", "420_1x1"]
    streams = [WC.jpg(n) for n in names]
    d = mijpeg.Decoder(96, 80, len(streams), progressive=True)
    try:
        d.decode(streams)
        d.output("progressive")
        d.transcode(1)
        for i, s in enumerate(streams):
            same(d.transcoded(i), W.model(s, 1))
        assert d.transcode_ms() > 0
        ptr, n = d.device_transcoded(2)
        assert ptr and n == len(W.model(streams[2], 1))
        d.output("baseline")
        d.transcode(1)
        for i, s in enumerate(streams):
            same(d.transcoded(i), mijpeg.transcode(s, 1, progressive=True))
    finally:
        d.close()


# 6. refusals, before any device work
def _code(e) -> int:
    return int(re.search(r" \((\d+)\): ", str(e.value)).group(1))


def test_refusals():
    src = WC.jpg("420_35x21")  # 3 MCUs across, 5 luma blocks: 13108 rows fit the DC scans' DRI, not the luma scans'
    for rr in (-1, 13108):
        with pytest.raises(mijpeg.MijError, match="frame 0") as e:
            mijpeg.transcode(src, rr, output="progressive")
        assert _code(e) == 1
    assert len(mijpeg.transcode(src, 13108)) > 0  # (the baseline scan's interval is in the frame's MCUs)
    d = mijpeg.Decoder(96, 80, 2)
    try:
        d.decode([WC.jpg("444_17x9"), src])
        d.output("progressive")
        with pytest.raises(mijpeg.MijError, match="frame 1") as e:
            d.transcode(13108)
        assert _code(e) == 1
        with pytest.raises(mijpeg.MijError, match="output"):
            d.output("lossless")
        assert d.lib.mij_decoder_output(d.h_, 2) == 1
    finally:
        d.close()
    with pytest.raises(mijpeg.MijError):  # progressive= still says what comes in
        mijpeg.transcode(WC.jpg("p420_35x21"), 0, output="progressive")


# 7. the one-shot C call and the command-line tool
def test_one_shot_and_command_line(tmp_path):
    import ctypes as C
    lib = mijpeg.load()
    for name in ("420_70x37_rstrow", "p420_35x21"):
        src = WC.jpg(name)
        want = W.model(src, 1)
        jb = np.frombuffer(src, np.uint8)
        n = C.c_size_t(0)
        assert lib.mij_transcode_progressive(jb.ctypes.data, jb.size, 1, None, 0, C.byref(n)) == 4
        assert n.value == len(want)
        buf = np.zeros(n.value, np.uint8)
        assert lib.mij_transcode_progressive(jb.ctypes.data, jb.size, 1, buf.ctypes.data, buf.size, C.byref(n)) == 0
        same(buf.tobytes(), want)
    tool = os.path.join(os.path.dirname(mijpeg.__file__), "host", "transcode_jpg")
    src, dst = tmp_path / "in.jpg", tmp_path / "out.jpg"
    src.write_bytes(WC.jpg("420_70x37_rstrow"))
    subprocess.run([tool, "--write-progressive", str(src), str(dst), "1"], check=True, timeout=120, capture_output=True)
    same(dst.read_bytes(), mijpeg.transcode(WC.jpg("420_70x37_rstrow"), 1, output="progressive"))
