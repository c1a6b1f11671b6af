"""The progressive decoder without a GPU: the plain Python
model against the committed digests (and against Pillow where installed),
the scan-script refusals' wording, and the decode routine the kernel runs
per lane (csrc/mij_progressive.h), compiled for the host with the address
and undefined-behaviour sanitizers as a program of its own
(tests/progressive_check.cpp): every fixture against the model's
coefficients, then cut, overrun and bit-flipped streams, which must end in a
status code with nothing read or written out of bounds."""
import hashlib
import io
import re

import numpy as np
import pytest

import foreign_cases as FC
import progressive_cases as PC
import progressive_model as PM


def _sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.mark.parametrize("name", PC.NAMES)
def test_model_matches_the_manifest(name):
    e, m = PC.MANIFEST["files"][name], PC.model(name)
    assert _sha(PC.jpg(name)) == e["sha256"]
    assert (m.w, m.h, m.nscans, m.levels) == (e["w"], e["h"], e["nscans"], e["levels"])
    assert [list(s) for s in m.script] == e["script"]
    assert _sha(m.rgb.tobytes()) == e["rgb_sha256"]
    assert _sha(b"".join(c.tobytes() for c in m.coefs)) == e["coef_sha256"]
    if name.startswith("p") and name != "pgrey_35x21":
        assert (m.nscans, m.levels) == (10, 3)  # Pillow's script for colour files


@pytest.mark.parametrize("name", PC.NAMES)
def test_model_matches_the_baseline_twin(name):
    """same pixels; same coefficients on every block inside the components' own grids, no AC outside them"""
    m, t = PC.model(name), FC.model(PC.twin(name))
    assert m.layout == [*t.layout[:7], 0, 1, *t.layout[9:]]
    assert (m.rgb == t.rgb).all() and (m.bgr == t.bgr).all()
    for c in range(m.G["ncomp"]):
        ins = PM.inside(m.G, c)
        assert (m.coefs[c][ins] == t.coefs[c][ins]).all(), c
        out = np.setdiff1d(np.arange(len(m.coefs[c])), ins)
        assert not m.coefs[c][out][:, 1:].any(), c


def test_grids_are_narrower_than_the_padded_planes():
    """35x21 at 4:2:0: luma scans cover 5x3 blocks of a 6x4 plane"""
    G = PC.model("p420_35x21").G
    assert PM.grids(G) == [(5, 3), (3, 2), (3, 2)] and [c[3:] for c in G["comps"]] == [(6, 4), (3, 2), (3, 2)]


@pytest.mark.parametrize("name", PC.NAMES)
def test_model_matches_pillow(name):
    Image = pytest.importorskip("PIL.Image")
    px = np.asarray(Image.open(io.BytesIO(PC.jpg(name))).convert("RGB"))
    assert (PC.model(name).rgb == px).all()
    twin = np.asarray(Image.open(io.BytesIO(FC.jpg(PC.twin(name)))).convert("RGB"))
    assert (px == twin).all()


def test_encoder_round_trip_with_restart_intervals():
    """the model's encoder under a script with a restart interval in every scan, decoded by the model"""
    G, coefs, dqt = PC._twin_planes("420_35x21")
    script = [([0, 1, 2], 0, 0, 2), ([0], 1, 63, 4), ([1], 1, 63, 1), ([2], 1, 63, 5)]
    m = PM.decoded(PM.encode(G, coefs, dqt, script))
    assert [tuple(s[5:]) for s in m.script] == [(2,), (4,), (1,), (5,)]
    for c in range(3):
        ins = PM.inside(m.G, c)
        assert (m.coefs[c][ins] == coefs[c][ins]).all()


@pytest.mark.parametrize("name", sorted(PC.refusals()))
def test_model_refuses_with_the_librarys_wording(name):
    stream, text = PC.refusals()[name]
    with pytest.raises(PM.Reject, match=re.escape(text)) as e:
        PM.decoded(stream)
    assert str(e.value).startswith("stream 0")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("progressive_check")
    return PC.build_check(d), d


def test_shared_routine_decodes_every_fixture(check):
    exe, d = check
    got = PC.run_check(exe, d, [(n, PC.jpg(n), PC.model(n).coefs, "ok") for n in PC.NAMES])
    for n in PC.NAMES:
        e = PC.MANIFEST["files"][n]
        assert got[n].startswith(f"ok, {e['nscans']} scans, {e['levels']} levels, coefficients equal"), got[n]


def test_shared_parser_refuses_as_the_model_does(check):
    exe, d = check
    cases = PC.refusals()
    got = PC.run_check(exe, d, [(n, cases[n][0], None, "refused") for n in sorted(cases)])
    for n, (stream, _) in cases.items():
        with pytest.raises(PM.Reject) as e:
            PM.decoded(stream)
        assert got[n] == f"refused: {e.value} (expected refused)", n


def test_corrupt_entropy_data_ends_in_a_status_code(check):
    """each fixture cut in a first and in a refinement scan (the bits end early: 5), an end-of-band run past its
    scan's last block (8), and a flipped bit inside each scan of p420_35x21 (anything, inside the bounds)"""
    exe, d = check
    cases = []
    for n in PC.NAMES:
        b = PC.jpg(n)
        first, refine = PC.first_and_refinement(b)
        cases.append((f"{n}_cut_first", PC.cut_scan(b, first), None, "status"))
        if refine is not None:
            cases.append((f"{n}_cut_refine", PC.cut_scan(b, refine), None, "status"))
    # the two streams the GPU tests send to the device: the exact code and scan, here first
    for label, (stream, scan, code) in PC.corrupt().items():
        cases.append((label, stream, None, f"status:{code}"))
    p = PC.jpg("p420_35x21")
    cases += [(f"flip_scan{k}", PC.flip_bit(p, k), None, "any") for k in range(len(PC.spans(p)))]
    got = PC.run_check(exe, d, cases)
    for label, (_, scan, code) in PC.corrupt().items():
        assert got[label].startswith(f"status {code} in scan {scan} "), got[label]
    first, refine = PC.first_and_refinement(p)
    assert f"in scan {first}" in got["p420_35x21_cut_first"] and f"in scan {refine}" in got["p420_35x21_cut_refine"]
    # the model finds the same streams corrupt, in the same scan
    for label in ("eob_overrun", "cut_refinement", "p420_35x21_cut_first", "p420_35x21_cut_refine"):
        stream = next(c[1] for c in cases if c[0] == label)
        with pytest.raises(PM.Reject, match=r"scan \d+: corrupt entropy data") as e:
            PM.decoded(stream)
        assert re.search(r"scan (\d+)", str(e.value)).group(1) == re.search(r"in scan (\d+)", got[label]).group(1)
