"""The sweep of random scan scripts without a GPU (DESIGN.md §4p,
tests/progressive_sweep.py): what the fixed list of cases is certain to
contain, asserted from its token lists; the plain Python model and the
decode routine the kernel runs per lane (tests/progressive_check.cpp, a
program of its own under the address and undefined-behaviour sanitizers)
against the planes the streams were written from; mutated streams through
that program, the only place they run; and the model's pixels against
Pillow's libjpeg-turbo wherever every IDCT output stays inside libjpeg's
range table."""
import io

import numpy as np
import pytest

import decode_model as M
import progressive_cases as PC
import progressive_model as PM
import progressive_sweep as S

CASES = S.cases()


def _runs(part):
    """(blocks, correction bits behind it) of every EOB run of one interval's tokens"""
    out = []
    for i, (t, sym, extra, _) in enumerate(part):
        if t == 0 and not sym & 15 and sym != 0xF0:
            be = 0
            for u in part[i + 1:]:
                if u[0] != -1:
                    break
                be += 1
            out.append(((1 << (sym >> 4)) + extra, be))
    return out


def test_the_cases_cover_what_they_are_there_for():
    """conditions, not measurements: at least one of each across cases()"""
    seen = set()
    pairs = set()
    for c in CASES:
        pairs.add((c.sampling, c.kind))
        if (c.w, c.h) == (1, 1):
            seen.add("1x1 frame")
        if c.levels >= 4:
            seen.add("script of >= 4 levels")
        first = {}
        times = {}
        for (comps, ss, se, ah, al, ri), parts in zip(c.script, c.tokens):
            assert len(parts) == (-(-S.scan_mcus(c.G, comps) // ri) if ri else 1)
            if len(parts) >= 65:
                seen.add("scan of >= 65 restart intervals")
            if ss and not ah:
                first.setdefault(comps[0], []).append((ss, se))
                if al == 3:
                    seen.add("first-pass Al 3")
            if ss and ah:
                if sum(1 for a, b in first[comps[0]] if a <= se and ss <= b) >= 2:
                    seen.add("refinement band straddling two first-pass bands")
                for z in range(ss, se + 1):
                    times[(comps[0], z)] = times.get((comps[0], z), 0) + 1
            for part in parts:
                for t, sym, _, _ in part:
                    if ss == 0 and not ah and sym == 11:
                        seen.add("DC symbol of category 11")
                    if ss and not ah and t == 0 and sym & 15 == 10:
                        seen.add("AC symbol of category 10")
                    if ss and ah and t == 0 and sym == 0xF0:
                        seen.add("ZRL in a refinement scan")
                if ss:
                    for blocks, be in _runs(part):
                        if be and ah:
                            seen.add("EOB run followed by correction bits")
                        if blocks >= 64:
                            seen.add("EOB run of >= 64 blocks")
        if times and max(times.values()) >= 3:
            seen.add("coefficient refined three times")
    want = {"ZRL in a refinement scan", "EOB run followed by correction bits", "EOB run of >= 64 blocks",
            "DC symbol of category 11", "AC symbol of category 10", "first-pass Al 3", "coefficient refined three times",
            "refinement band straddling two first-pass bands", "script of >= 4 levels", "1x1 frame",
            "scan of >= 65 restart intervals"}
    assert seen == want, sorted(want - seen)
    assert pairs == {(s, k) for s in S.SAMPLINGS for k in S.KINDS}
    assert all(c.w <= 100 and c.h <= 70 and len(c.script) <= S.MAX_SCANS for c in CASES)


def test_planes_are_what_the_kinds_say():
    for c in CASES:
        for p in c.coefs:
            assert p.dtype == np.int16 and p[:, 0].min() >= -1024 and p[:, 0].max() <= 1023
            assert np.abs(p[:, 1:].astype(np.int64)).max(initial=0) <= {"small": 3, "zero": 0}.get(c.kind, 1023)
        for i, p in enumerate(c.coefs):
            ins = PM.inside(c.G, i)
            out = np.setdiff1d(np.arange(len(p)), ins)
            assert not p[out, 1:].any()
            if c.kind == "dense":
                assert p[ins, 1:].all()
            if c.kind == "tail":
                assert not p[:, 2:63].any()


@pytest.mark.parametrize("seed", range(40))
def test_scripts_are_legal_and_fit(seed):
    """any seed, with and without a geometry: the model's parser takes the script, and it is 64 scans at the most"""
    rng = np.random.default_rng([7, seed])
    sampling = list(S.SAMPLINGS)[seed % 4]
    G = S.geometry(*S.SIZES[seed % len(S.SIZES)], sampling)
    sc = S.script(rng, G["ncomp"], G if seed % 3 else None)
    assert 2 <= len(sc) <= S.MAX_SCANS
    coefs = S.planes(rng, G, "zero", sc)
    P = PM.parse(S.write(G, coefs, sc, {0: S.ONES, 1: S.ONES}))
    assert [(tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"], s["ri"]) for s in P["scans"]] == sc
    assert [s["level"] for s in P["scans"]] == S.levels(sc)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_model_returns_the_planes(case):
    m = PM.decoded(case.stream)
    assert (m.w, m.h, m.nscans, m.levels) == (case.w, case.h, len(case.script), case.levels)
    assert [(tuple(s[0]),) + tuple(s[1:]) for s in m.script] == case.script
    assert m.layout == PM.F.layout_list(dict(case.G, ri=0))
    for c, p in enumerate(case.coefs):
        assert m.coefs[c].shape == p.shape and (m.coefs[c] == p).all(), c
    assert all((m.dqt[c] == case.dqt[comp[2]]).all() for c, comp in enumerate(case.G["comps"]))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("progressive_sweep_check")
    return PC.build_check(d), d


def test_shared_routine_returns_the_planes(check):
    exe, d = check
    got = PC.run_check(exe, d, [(c.name, c.stream, c.coefs, "ok") for c in CASES])
    for c in CASES:
        assert got[c.name].startswith(f"ok, {len(c.script)} scans, {c.levels} levels, coefficients equal"), (c.name, got[c.name])


def test_mutated_streams_stay_inside_the_bounds(check):
    """a flipped bit and a lost half in a first scan, a refinement and the last scan of a dozen cases: whatever
    the routine makes of them, it reads and writes nothing out of bounds"""
    exe, d = check
    cases = []
    for c in CASES[3::8]:
        ac = [k for k, s in enumerate(c.script) if s[1]]
        ks = {ac[0], next((k for k in ac if c.script[k][3]), ac[0]), len(c.script) - 1, 0}
        for k in sorted(ks):
            cases.append((f"{c.name}_flip{k}", PC.flip_bit(c.stream, k), None, "any"))
            cases.append((f"{c.name}_cut{k}", PC.cut_scan(c.stream, k), None, "any"))
    assert len(CASES[3::8]) == 12
    PC.run_check(exe, d, cases)


def _outside_the_range_table(m):
    """samples whose IDCT output, before the level shift and the clamp, lies outside -512 .. 511: there libjpeg's
    C code wraps around its 1024-entry range table and its SIMD code saturates in between"""
    n = 0
    for c, coefs in enumerate(m.coefs):
        x = np.zeros((len(coefs), 64), np.int64)
        x[:, M.ZZ] = coefs.astype(np.int64) * np.asarray(m.dqt[c], np.int64)
        x = x.reshape(-1, 8, 8)
        v = M.pass_1d(M.pass_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1), 18)
        n += int(((v < -512) | (v > 511)).sum())
    return n


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_model_matches_pillow_inside_the_range_table(case, record_property):
    """every kind but dense: the model's pixels are Pillow's.  dense (every coefficient nonzero, half at +-1023)
    leaves the range table; libjpeg's builds differ among themselves there and the model clamps, so nothing is
    asserted and the count of differing pixels is printed"""
    Image = pytest.importorskip("PIL.Image")
    m = PM.decoded(case.stream)
    px = np.asarray(Image.open(io.BytesIO(case.stream)).convert("RGB"))
    assert px.shape == m.rgb.shape
    differ = int((px != m.rgb).any(-1).sum())
    if case.kind == "dense":
        outside = _outside_the_range_table(m)
        record_property("pixels_differing_from_pillow", differ)
        print(f"{case.name}: {differ} of {case.w * case.h} pixels differ from Pillow; {outside} samples outside the range table")
    else:
        assert differ == 0, differ
