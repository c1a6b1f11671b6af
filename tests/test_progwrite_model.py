"""The model of progressive output (tests/progwrite_model.py)
pinned to independent code, on the CPU: its tokens, coded with the Huffman
tables read from a Pillow file, are that file's entropy data, scan for scan
and interval for interval; the file it writes with the project's own tables
decodes (progressive_model, Pillow) to the source's coefficients and pixels;
and the per-block routines the kernels run (csrc/mij_progwrite.h), compiled
into a program of their own under the sanitizers, give the model's tokens."""
import io

import numpy as np
import pytest

import progressive_model as PM
import progwrite_cases as WC
import progwrite_model as W


# 1. the token rules are libjpeg's: Pillow's bytes from Pillow's tables
@pytest.mark.parametrize("name", WC.PILLOW + WC.LIMITS)
def test_tokens_with_the_files_tables_are_the_files_bytes(name):
    jpg = WC.jpg(name)
    P, D = PM.parse(jpg), PM.decoded(jpg)
    assert [(tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in P["scans"]] == W.script(len(P["comps"]))
    for k, sc in enumerate(P["scans"]):
        parts = W.tokens(D.G, D.coefs, tuple(sc["comps"]), sc["ss"], sc["se"], sc["ah"], sc["al"], sc["ri"])
        codes = [W.huff_codes(t) for t in sc["td"] if t] if sc["ss"] == 0 else [W.huff_codes(sc["ta"])]
        assert [W.entropy(t, codes) for t in parts] == sc["parts"], k


def test_the_limit_fixtures_reach_their_limits():
    D = PM.decoded(WC.jpg("corr_limit"))
    for comps, ss, se, ah, al in W.script(1):
        if ss and ah:
            r = W.runs(D.G, D.coefs, comps, ss, se, ah, al, 0)
            assert len(r) == 6 and max(be for _, be in r) == 940 > W.MAX_BE
    D = PM.decoded(WC.jpg("run_limit"))
    for comps, ss, se, ah, al in W.script(1):
        if ss:
            assert [n for n, _ in W.runs(D.G, D.coefs, comps, ss, se, ah, al, 0)] == [0x7FFF, 33024 - 0x7FFF]


# 2. restart_rows is libjpeg's restart_in_rows: the intervals Pillow chose for the same picture
def test_intervals_are_rows_of_each_scans_own_mcus():
    P = PM.parse(WC.jpg("p420_70x37_rstrow"))
    G = PM.decoded(WC.jpg("p420_70x37_rstrow")).G
    assert [s["ri"] for s in P["scans"]] == [W.across(G, c) for c, _, _, _, _ in W.script(3)]
    assert [s["ri"] for s in PM.parse(W.model(WC.jpg("420_70x37_rstrow"), 1))["scans"]] == [s["ri"] for s in P["scans"]]
    assert [s["ri"] for s in PM.parse(W.model(WC.jpg("420_70x37_rstrow"), 2))["scans"]] == [2 * s["ri"] for s in P["scans"]]


# 3. the whole file with the project's own tables
@pytest.mark.parametrize("rr", [0, 1, 2])
@pytest.mark.parametrize("name", WC.BASELINE + WC.TWINS + ["corr_limit"])
def test_own_file_decodes_to_the_source(name, rr):
    src = WC.jpg(name)
    out = W.model(src, rr)
    w, h, comps, hv, dqt, planes = W.source(src)
    D = PM.decoded(out)
    assert (D.w, D.h) == (w, h) and D.nscans == (10 if len(comps) == 3 else 6)
    assert [(tuple(c), a, b, e, f) for c, a, b, e, f, _ in D.script] == W.script(len(comps))
    for c in range(len(comps)):
        want, got = WC.coded_inside(planes[c], D.coefs[c].astype(np.int64), D.G, c)
        assert (want[0] == got[0]).all() and (want[1] == got[1]).all(), c
    Image = pytest.importorskip("PIL.Image")
    a, b = Image.open(io.BytesIO(out)), Image.open(io.BytesIO(src))
    assert a.mode == b.mode and (np.asarray(a) == np.asarray(b)).all()


def test_refusals():
    src = W.source(WC.jpg("420_35x21"))
    with pytest.raises(ValueError):
        W.build(*src, -1)
    with pytest.raises(ValueError):  # 5 luma blocks across: 13108 rows are 65540 MCUs of the luma scans, 39324 of the DC scan
        W.build(*src, 13108)


# 4. the routines the kernels run, on the CPU under the sanitizers
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("progwrite_check")
    return WC.build_check(d), d


# (the two large pictures once)
@pytest.mark.parametrize("name,rr", [(n, rr) for n in WC.PILLOW + WC.LIMITS for rr in (0, 1)
                                     if not (rr and n in ("p420_1040x520_q30", "run_limit"))])
def test_shared_routines_give_the_models_tokens(check, name, rr):
    exe, d = check
    D = PM.decoded(WC.jpg(name))
    got = WC.run_check(exe, d, f"{name}_{rr}", D.G, D.coefs, rr)
    for (comps, ss, se, ah, al), parts in zip(W.script(D.G["ncomp"]), got):
        assert parts == W.tokens(D.G, D.coefs, comps, ss, se, ah, al, rr * W.across(D.G, comps)), (comps, ss, ah)
