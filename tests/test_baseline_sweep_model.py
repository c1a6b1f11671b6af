"""The baseline sweep without a GPU (DESIGN.md §4f "The sweep",
tests/baseline_sweep.py): the plain Python model (and, for the three-scan
shape it refuses, a small sequential reader here) and Pillow's libjpeg-turbo
against the planes the streams were written from; the census -- what the
fixed list is certain to put in front of the decoder, asserted from the
writer's bit map, never from a decoder; the decoder's own table builder and
symbol decoder (csrc/mij_huff.h) walking every stream on the CPU in a program
of its own under the address and undefined-behaviour sanitizers
(tests/baseline_check.cpp); and the DC-range rule of the transcoder (DESIGN.md
§4h) in the models."""
import io

import numpy as np
import pytest

import baseline_sweep as B
import foreign_model as FM
import interleave_model as IM
import progressive_sweep as S
import transcode_model as TM

CASES = B.cases()
LOOK, CHUNK = B.LOOK, B.CHUNK
NAMED = ("aligned_grey_136x136_ri0", "aligned_grey_136x136_ri256", "rst1_grey_136x136", "every_1023_interleaved_35x21",
         "every_1023_three_scan_32x32", "dc_swing_interleaved_70x37", "dc_swing_three_scan_48x48", "fib_grey_64x64",
         "ff_tail_grey_100x70")


def test_the_list_is_what_the_issue_asks_for():
    assert len(CASES) == 48 and all(B.by_name(n) in CASES for n in NAMED)
    il = [c for c in CASES if c.shape == "interleaved"]
    ts = [c for c in CASES if c.shape == "three_scan"]
    assert len(ts) >= 8 and min(c.w * c.h for c in ts) == 16 * 16 and max(c.w * c.h for c in ts) == 96 * 80
    assert all(c.w % 16 == 0 and c.h % 16 == 0 and c.ri == 0 and c.sampling == "420" for c in ts)
    assert {(c.sampling, c.kind) for c in il} == {(s, k) for s in S.SAMPLINGS for k in S.KINDS}
    for group in (il, ts):
        assert {c.tables for c in group} == set(B.TABLES) and {c.ids for c in group} == set(B.IDS)
    for s in S.SAMPLINGS:
        assert {c.tables for c in il if c.sampling == s} == set(B.TABLES), s
    assert all((c.w, c.h) in S.SIZES or c.name in NAMED or c.shape == "three_scan" for c in CASES)
    assert all(c.w <= 100 and c.h <= 70 or (c.w, c.h) == (136, 136) or c.shape == "three_scan" for c in CASES)
    # restart intervals: none, one MCU, three, a row of MCUs, a count that does not divide the scan
    kinds = set()
    for c in il:
        nm = c.G["mcus_x"] * c.G["mcus_y"]
        kinds.add("none" if c.ri == 0 else "one" if c.ri == 1 else "three" if c.ri == 3 else None)
        if c.ri == c.G["mcus_x"] and c.G["mcus_y"] > 1:
            kinds.add("a row")
        if c.ri > 1 and nm % c.ri and c.ri % c.G["mcus_x"]:
            kinds.add("not whole rows, not a divisor")
    assert kinds >= {"none", "one", "three", "a row", "not whole rows, not a divisor"}
    # every arrangement of the segments occurs
    for c in CASES:
        head = c.stream[:c.stream.index(b"\xff\xda")]
        I = B.IDS[c.ids]
        assert head.count(b"\xff\xc4") == (1 if I["single"] else len(c.bitmap["tables"])) + (1 if I["redefine"] else 0)
        assert head.count(b"\xff\xdb") == len(set(I["tq"][:c.G["ncomp"]])) + (1 if I["spare"] and 3 not in I["tq"][:c.G["ncomp"]] else 0)


@pytest.mark.parametrize("case", [c for c in CASES if c.shape == "interleaved"], ids=repr)
def test_model_returns_the_planes(case):
    P = FM.parse(case.stream)
    G = FM.geometry(P)
    assert FM.layout_list(G) == FM.layout_list(case.G)
    got = FM.coefficients(P, G)
    for c, want in enumerate(case.coefs):
        assert got[c].shape == want.shape and (got[c] == want).all(), c
    for c, comp in enumerate(G["comps"]):
        assert (P["dqt"][comp[2]] == np.asarray(case.dqt[1 if c else 0])).all()
    assert [c[0] for c in P["comps"]] == list(B.IDS[case.ids]["cids"][:G["ncomp"]])


def _read_three_scan(jpg):
    """a sequential reader of the three-scan shape: segments in order (a DHT replaces what its id held), each SOS
    followed by its entropy data up to the next marker, one component per scan in raster order over its plane,
    the DC prediction running through the scan.  -> (w, h, SOF0 entries, {Tq: table}, planes by SOF0 order)"""
    assert jpg[:2] == b"\xff\xd8"
    i, dht, dqt, planes, sof = 2, {}, {}, {}, None
    while jpg[i + 1] != 0xD9:
        assert jpg[i] == 0xFF
        m, n = jpg[i + 1], (jpg[i + 2] << 8) | jpg[i + 3]
        q = jpg[i + 4:i + 2 + n]
        i += 2 + n
        if m == 0xDB:
            for o in range(0, len(q), 65):
                dqt[q[o]] = list(q[o + 1:o + 65])
        elif m == 0xC4:
            o = 0
            while o < len(q):
                counts = list(q[o + 1:o + 17])
                dht[(q[o] >> 4, q[o] & 15)] = FM._Huff(counts, list(q[o + 17:o + 17 + sum(counts)]))
                o += 17 + sum(counts)
        elif m == 0xC0:
            h, w = (q[1] << 8) | q[2], (q[3] << 8) | q[4]
            sof = [(q[6 + 3 * c], q[7 + 3 * c], q[8 + 3 * c]) for c in range(q[5])]
        elif m == 0xDA:
            assert q[0] == 1 and bytes(q[3:6]) == b"\x00\x3f\x00"
            c = [s[0] for s in sof].index(q[1])
            e = i
            while not (jpg[e] == 0xFF and jpg[e + 1] != 0):
                e += 1
            data = jpg[i:e].replace(b"\xff\x00", b"\xff")
            br = FM._Bits(data)
            i = e
            hs, vs = sof[c][1] >> 4, sof[c][1] & 15
            nb = (w // 16 * hs) * (h // 16 * vs)
            p = np.zeros((nb, 64), np.int64)
            pred = 0
            for b in range(nb):
                s = br.sym(dht[(0, q[2] >> 4)])
                pred += br.mag(s) if s else 0
                p[b, 0] = pred
                k = 1
                while k < 64:
                    rs = br.sym(dht[(1, q[2] & 15)])
                    if rs & 15:
                        k += rs >> 4
                        p[b, k] = br.mag(rs & 15)
                        k += 1
                    elif rs == 0xF0:
                        k += 16
                    else:
                        break
            assert 0 <= 8 * len(data) - br.p < 8 and c not in planes  # nothing but the pad bits is left
            planes[c] = p.astype(np.int16)
    return w, h, sof, dqt, [planes[c] for c in range(len(sof))]


@pytest.mark.parametrize("case", [c for c in CASES if c.shape == "three_scan"], ids=repr)
def test_sequential_reader_returns_the_planes(case):
    w, h, sof, dqt, planes = _read_three_scan(case.stream)
    assert (w, h) == (case.w, case.h) and sof == case.sof[0]
    for c, want in enumerate(case.coefs):
        assert planes[c].shape == want.shape and (planes[c] == want).all(), c
        assert dqt[sof[c][2]] == [int(v) for v in case.dqt[1 if c else 0]]
    # ... and the twin the stream-parsing models take in its place holds the same planes
    P = FM.parse(case.twin)
    for got, want in zip(FM.coefficients(P, FM.geometry(P)), case.coefs):
        assert (got == want).all()
    # mij_decoder_coefs' form: the running sum of the differences is the plane's DC
    for d, want in zip(case.diffed(), case.coefs):
        assert (np.cumsum(d.reshape(-1, 64)[:, 0].astype(np.int64)) == want[:, 0]).all()


@pytest.mark.parametrize("case", [c for c in CASES if c.kind != "dense"], ids=repr)
def test_pillow_decodes_to_the_models_pixels(case):
    """the writer and its crafted tables against libjpeg, whatever foreign_model makes of them: every kind but
    dense, whose samples leave libjpeg's range table"""
    Image = pytest.importorskip("PIL.Image")
    want = FM.decoded(case.twin).rgb
    px = np.asarray(Image.open(io.BytesIO(case.stream)).convert("RGB"))
    assert px.shape == want.shape and not (px != want).any(), int((px != want).any(-1).sum())


def _census(cases):
    seen = set()
    for c in cases:
        ivs = c.bitmap["intervals"]
        per_scan = {}
        for n, iv in enumerate(ivs):
            per_scan[iv["scan"]] = per_scan.get(iv["scan"], 0) + 1
            nbits, starts = iv["nbits"], iv["blocks"]
            if nbits % CHUNK == 0:
                seen.add("interval of a whole number of chunks")
            if nbits < CHUNK:
                seen.add("interval shorter than a chunk")
            if any(p and p % CHUNK == 0 for p in starts):
                seen.add("block start on a chunk boundary inside an interval")
            # chunks that lie wholly inside one block: a lane that starts no block and stores a middle part
            ends = starts[1:] + [iv["used"]]
            if any((e - 1) // CHUNK - s // CHUNK >= 2 for s, e in zip(starts, ends)):
                seen.add("chunk in which no block starts")
            for pos, t, th, s, l, nb, v in iv["syms"]:
                seen.add(("AC" if t else "DC", "length", l if t else ("<= LOOK" if l <= LOOK else l)))
                if l + nb == 26 and t:
                    seen.add("AC symbol of 26 bits")
                if l + nb == 27 and not t:
                    seen.add("DC symbol of 27 bits")
                if l > LOOK:
                    last = pos + l + nb - 1
                    if pos // CHUNK != last // CHUNK:
                        seen.add("long symbol across a chunk boundary")
                    # the window holds words pos / 64 and pos / 64 + 1: the symbol runs on into the second
                    if pos // 64 != last // 64:
                        seen.add("long symbol into the second word of its pair")
                    if pos // 64 != (pos + l - 1) // 64:
                        seen.add("long code across a word boundary")
            stuffed = iv["data"].endswith(b"\xff")
            if stuffed and n + 1 < len(ivs) and ivs[n + 1]["scan"] == iv["scan"]:
                seen.add("stuffed byte in front of RSTn")
            if stuffed and n + 1 == len(ivs):
                seen.add("stuffed byte in front of EOI")
        if max(per_scan.values()) > 256:
            seen.add("scan of more than 256 intervals")
    return seen


WANT = ({("AC", "length", l) for l in range(1, 17)} |
        {("DC", "length", "<= LOOK"), ("DC", "length", LOOK + 1), ("DC", "length", 16)} |
        {"AC symbol of 26 bits", "DC symbol of 27 bits", "long symbol across a chunk boundary",
         "long symbol into the second word of its pair", "long code across a word boundary",
         "chunk in which no block starts", "block start on a chunk boundary inside an interval",
         "interval of a whole number of chunks", "interval shorter than a chunk", "scan of more than 256 intervals",
         "stuffed byte in front of RSTn", "stuffed byte in front of EOI"})


def test_the_census():
    """conditions, not measurements, from the writer's bit map: each occurs at least once across cases().  The
    stuffed bytes in front of RSTn and EOI come from a seed found by a search outside the tests
    (baseline_sweep.FF_SEED, the first of 0, 1, ... that gives both); everything else is arithmetic"""
    seen = _census(CASES)
    assert seen >= WANT, sorted(map(str, WANT - seen))
    stream = B.by_name("ff_tail_grey_100x70").stream
    assert stream.endswith(b"\xff\x00\xff\xd9") and any(bytes([0xFF, 0x00, 0xFF, 0xD0 + k]) in stream for k in range(8))


def test_the_named_cases_hold_by_arithmetic():
    """what each named frame is there for, from its own bit map alone: deleting one fails here"""
    k = B.annexk()
    dc0 = B.PM._codes(*k[(0, 0)])[0]
    eob = B.PM._codes(*k[(1, 0)])[0]
    assert dc0[1] == 2 and eob[1] == 4 and 256 * 6 == 3 * CHUNK
    a0, a256 = B.by_name("aligned_grey_136x136_ri0"), B.by_name("aligned_grey_136x136_ri256")
    for c in (a0, a256):
        assert c.tables == "annexk" and len(c.coefs[0]) == 289 and not c.coefs[0][:256].any() and c.coefs[0][256:, 1:].all()
    (iv,) = a0.bitmap["intervals"]
    assert iv["blocks"][256] == 3 * CHUNK and iv["blocks"][255] == 3 * CHUNK - 6
    first, second = a256.bitmap["intervals"]
    assert a256.ri == 256 and first["used"] == first["nbits"] == 3 * CHUNK and len(second["blocks"]) == 33
    assert "block start on a chunk boundary inside an interval" in _census([a0])
    assert "interval of a whole number of chunks" in _census([a256])
    rst1 = B.by_name("rst1_grey_136x136")
    ivs = rst1.bitmap["intervals"]
    assert rst1.ri == 1 and len(ivs) == 289 > 256 and all(i["nbits"] < CHUNK for i in ivs)
    assert -(-sum(-(-i["nbits"] // CHUNK) for i in ivs) // 256) >= 2  # chunks: one per interval, two workgroups
    for name in ("every_1023_interleaved_35x21", "every_1023_three_scan_32x32"):
        c = B.by_name(name)
        assert c.tables == "reversed"
        for iv in c.bitmap["intervals"]:
            ac = [x for x in iv["syms"] if x[1] == 1]
            assert len(ac) == 63 * len(iv["blocks"]) and all(x[4] == 16 and x[5] == 10 for x in ac)
            ends = iv["blocks"][1:] + [iv["used"]]
            assert all(63 * 26 < e - s <= 63 * 26 + 27 for s, e in zip(iv["blocks"], ends))  # > 3 chunks each
        assert {"chunk in which no block starts", "AC symbol of 26 bits", "long symbol across a chunk boundary",
                "long symbol into the second word of its pair"} <= _census([c])
    for name in ("dc_swing_interleaved_70x37", "dc_swing_three_scan_48x48"):
        c = B.by_name(name)
        dc = [x for iv in c.bitmap["intervals"] for x in iv["syms"] if x[1] == 0]
        assert c.tables == "reversed" and sum(1 for x in dc if x[3] == 11 and x[4] == 16) > len(dc) // 2
        assert "DC symbol of 27 bits" in _census([c])
    fib = B.by_name("fib_grey_64x64")
    ac = [x for x in fib.bitmap["intervals"][0]["syms"] if x[1] == 1]
    count = {}
    for x in ac:
        count[x[3]] = count.get(x[3], 0) + 1
    assert sorted(count.values()) == list(B.FIB) and count[0] == 64
    lengths = {s: l for _, _, _, s, l, _, _ in ac}
    assert sorted(lengths.values()) == list(range(1, 17))
    assert all(lengths[a] > lengths[b] for a in count for b in count if count[a] < count[b])


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("baseline_sweep_check")
    return B.build_check(d), d


def test_the_decoders_own_routines_walk_every_stream(check):
    """csrc/mij_huff.h under the sanitizers: build_table takes every table of the sweep (the incomplete ones too)
    and refuses over-subscribed ones, and decode_one returns the writer's symbol, value and bit count at every
    position of every interval"""
    exe, d = check
    cases = CASES + list(B.dc_range_cases())
    got = B.run_check(exe, d, cases)
    for c in cases:
        ivs = c.bitmap["intervals"]
        want = f"ok, {len(c.bitmap['tables'])} tables, {len(ivs)} intervals, {sum(len(i['syms']) for i in ivs)} symbols"
        assert got[c.name] == want, (c.name, got[c.name])
    assert got["build_table"] == "ok, over-subscribed codes refused"


# ---- the DC range ---------------------------------------------------------------
def _categories(case, restart_rows):
    """the DC categories the transcoder's scan needs for the case's planes (the truth: int16)"""
    G = case.G
    ri = restart_rows * G["mcus_x"]
    syms = B.symbols(G, [p.astype(np.int64) for p in case.coefs], ri, "interleaved")
    return {s for _, parts in syms for blocks in parts for _, ss in blocks for t, s, _, _, _ in ss if t == 0}


def test_dc_range_sources_in_the_models():
    a, b, c = B.dc_range_cases()
    for case in (a, b, c):
        got = FM.decoded(case.stream).coefs
        assert (got[0] == case.coefs[0]).all()  # foreign_model's planes are int16 too: the sums modulo 2^16
    assert np.abs(a.wide[0][:, 0]).max() == 30000 and (a.wide[0] == a.coefs[0]).all()
    assert {x[3] for iv in a.bitmap["intervals"] for x in iv["syms"] if x[1] == 0} == {11}
    assert {x[3] for iv in b.bitmap["intervals"] for x in iv["syms"] if x[1] == 0} == {15} and b.ri == 1
    assert c.wide[0][:, 0].max() == 81000 and (c.wide[0][:, 0] > 32767).sum() == 48
    assert max(x[3] for iv in c.bitmap["intervals"] for x in iv["syms"] if x[1] == 0) == 11
    d = np.diff(c.coefs[0][:, 0].astype(np.int64))
    assert (np.abs(d) > 32767).sum() == 1 and d[15] == -63536  # between the second and the third block row
    # what a transcode needs: (a) category 15 at the row starts and no more; (b) 16 whatever the interval; (c) 16
    # without restarts, 15 where every row (or every second) starts an interval
    assert max(_categories(a, 0)) == 11 and max(_categories(a, 1)) == 15
    assert max(_categories(b, 0)) == 16 and max(_categories(b, 1)) == 16
    assert max(_categories(c, 0)) == 16 and max(_categories(c, 1)) == 15 and max(_categories(c, 2)) == 15
    # ... and wherever it is at most 15, the model's file decodes back to the planes
    for case, rows in ((a, 0), (a, 1), (c, 1), (c, 2)):
        out = TM.model(case.stream, rows)
        assert (FM.decoded(out).coefs[0] == case.coefs[0]).all(), (case, rows)
    assert IM.mag_class(-63536) == 16
