"""Plain Python model of progressive output (include/mijpeg.h
mij_decoder_output): the coefficient planes of an accepted stream, after an
optional transform, written as a SOF2 file with libjpeg's
jpeg_simple_progression script, the token rules of libjpeg's jcphuff.c, one
restart interval of restart_rows rows of each scan's own MCUs, and tables
built by the project's builder (oracle.cref_build_table) from each scan's own
counts.

tokens() is pinned to Pillow by tests/test_progwrite_model.py: coded with the
Huffman tables read from a Pillow file it gives that file's entropy data,
scan for scan.  build() writes the whole file; the kernels must give these
bytes (tests/test_progwrite_gpu.py)."""
import numpy as np

import foreign_model as FM
import interleave_model as IM
import oracle as O
import progressive_model as PM

# (components, Ss, Se, Ah, Al): libjpeg's jpeg_simple_progression for YCbCr
SCRIPT = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
          ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
MAX_EOBRUN = 0x7FFF
MAX_BE = 937  # libjpeg's MAX_CORR_BITS - DCTSIZE2 + 1


def script(ncomp: int):
    """the scans of a frame: all ten for YCbCr, the six of component 0 for greyscale"""
    if ncomp == 3:
        return list(SCRIPT)
    return [((0,), ss, se, ah, al) for comps, ss, se, ah, al in SCRIPT if 0 in comps]


def geometry(w, h, hv):
    """foreign_model.geometry's dict from the sampling in effect"""
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return {"w": w, "h": h, "ncomp": len(hv), "hmax": hmax, "vmax": vmax, "mcus_x": mx, "mcus_y": my, "ri": 0,
            "interleaved": 1, "comps": [(a, b, 0, mx * a, my * b) for a, b in hv]}


def across(G, comps):
    """the scan's own MCUs across: the frame's for an interleaved scan, the component's block grid otherwise"""
    return G["mcus_x"] if len(comps) > 1 else PM.grids(G)[comps[0]][0]


def tokens(G, coefs, comps, ss, se, ah, al, ri):
    """per restart interval the scan's tokens in stream order: (table, symbol, extra value, extra bits); table is
    the index among the scan's own tables (DC: 0 for component 0, 1 for the others; AC: 0) or -1 for bits that
    follow no symbol (DC refinement bits, buffered correction bits)"""
    mcus = PM.scan_blocks(G, list(comps))
    ri = ri or len(mcus)
    out = []
    # |c| >> Al per coefficient, and per block whether the band holds any (most blocks of a flat picture hold none)
    T = {c: np.abs(np.asarray(coefs[c]).astype(np.int64)) >> al for c in comps} if ss else {}
    some = {c: T[c][:, ss:se + 1].any(axis=1) for c in T}
    for u0 in range(0, len(mcus), ri):
        toks = []
        state = {"run": 0, "be": []}

        def flush():
            if state["run"]:
                n = state["run"].bit_length() - 1
                toks.append((0, n << 4, state["run"] - (1 << n), n))
                state["run"] = 0
                toks.extend((-1, 0, b, 1) for b in state["be"])
                state["be"] = []

        pred = [0] * len(comps)
        for mcu in mcus[u0:u0 + ri]:
            for j, b in mcu:
                c = comps[j]
                blk = coefs[c][b]
                if ss == 0:
                    v = int(blk[0]) >> al
                    if ah:
                        toks.append((-1, 0, v & 1, 1))
                        continue
                    d = v - pred[j]
                    pred[j] = v
                    s = abs(d).bit_length()
                    toks.append((1 if c else 0, s, IM.mag_bits(d, s), s))
                    continue
                if not some[c][b]:  # an empty band: the block only extends the run
                    state["run"] += 1
                    if state["run"] == MAX_EOBRUN:
                        flush()
                    continue
                t = T[c][b].tolist()
                r = 0
                if ah == 0:
                    for k in range(ss, se + 1):
                        if t[k] == 0:
                            r += 1
                            continue
                        flush()
                        while r > 15:
                            toks.append((0, 0xF0, 0, 0))
                            r -= 16
                        s = t[k].bit_length()
                        toks.append((0, (r << 4) | s, (t[k] if blk[k] >= 0 else ~t[k]) & ((1 << s) - 1), s))
                        r = 0
                    if r > 0:
                        state["run"] += 1
                        if state["run"] == MAX_EOBRUN:
                            flush()
                    continue
                eob = max([k for k in range(ss, se + 1) if t[k] == 1], default=0)
                br = []
                for k in range(ss, se + 1):
                    if t[k] == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        flush()
                        toks.append((0, 0xF0, 0, 0))
                        r -= 16
                        toks.extend((-1, 0, x, 1) for x in br)
                        br = []
                    if t[k] > 1:
                        br.append(t[k] & 1)
                        continue
                    flush()
                    toks.append((0, (r << 4) | 1, 1 if blk[k] >= 0 else 0, 1))
                    toks.extend((-1, 0, x, 1) for x in br)
                    br = []
                    r = 0
                if r > 0 or br:
                    state["run"] += 1
                    state["be"] += br
                    if state["run"] == MAX_EOBRUN or len(state["be"]) > MAX_BE:
                        flush()
        flush()
        out.append(toks)
    return out


def runs(G, coefs, comps, ss, se, ah, al, ri):
    """[(blocks, correction bits)] of every EOB run the scan codes, in order"""
    out = []
    for toks in tokens(G, coefs, comps, ss, se, ah, al, ri):
        for i, (t, sym, extra, n) in enumerate(toks):
            if t == 0 and not sym & 15 and sym != 0xF0:
                be = 0
                for u in toks[i + 1:]:
                    if u[0] != -1:
                        break
                    be += 1
                out.append(((1 << (sym >> 4)) + extra, be))
    return out


def entropy(toks, codes) -> bytes:
    """one interval's unstuffed bytes; codes[table][symbol] = (code, length)"""
    acc, n = 0, 0
    for t, sym, extra, ne in toks:
        if t >= 0:
            code, l = codes[t][sym]
            acc = (acc << l) | code
            n += l
        acc = (acc << ne) | extra
        n += ne
    pad = -n % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((n + pad) // 8, "big")


def huff_codes(h: FM._Huff) -> dict:
    """{symbol: (code, length)} of a table read from a file"""
    return {s: (code, l) for (l, code), s in h.map.items()}


def build(w, h, comps, hv, dqt, planes, restart_rows):
    """comps: SOF entries (id, H/V byte, Tq) verbatim; hv: the sampling in effect per component (a lone component
    is 1x1); dqt: {id: 64 bytes}; planes: per component (blocks, 64) with absolute DCs, padded to whole MCUs"""
    nc = len(comps)
    G = geometry(w, h, hv)
    sc = script(nc)
    if restart_rows < 0 or any(restart_rows * across(G, s[0]) > 65535 for s in sc):
        raise ValueError(f"restart interval of {restart_rows} rows")
    out = bytearray(IM.APP0)
    for tq in sorted(set(c[2] for c in comps)):
        out += bytes([0xFF, 0xDB, 0x00, 0x43, tq]) + bytes(int(x) for x in dqt[tq])
    n = 8 + 3 * nc
    out += bytes([0xFF, 0xC2, n >> 8, n & 255, 8, h >> 8, h & 255, w >> 8, w & 255, nc])
    for cid, hvb, tq in comps:
        out += bytes([cid, hvb, tq])
    cur_ri = 0
    for cs, ss, se, ah, al in sc:
        ri = restart_rows * across(G, cs)
        if ri != cur_ri:
            out += bytes([0xFF, 0xDD, 0x00, 0x04, ri >> 8, ri & 255])
            cur_ri = ri
        parts = tokens(G, planes, cs, ss, se, ah, al, ri)
        ntab = 0 if ss == 0 and ah else (2 if ss == 0 and len(cs) > 1 else 1)
        codes = []
        for t in range(ntab):
            hist = np.zeros(256, np.int64)
            for toks in parts:
                for tt, sym, _, _ in toks:
                    if tt == t:
                        hist[sym] += 1
            rc, huff = O.cref_build_table(hist)
            assert rc == 0, (cs, ss, t, rc)
            # DC 00 / AC 10 for component 0, 01 / 11 for the others
            th = t if ss == 0 else (1 if cs[0] else 0)
            out += IM._dht(huff, ((1 if ss else 0) << 4) | th)
            codes.append({s: (huff.sym_code[s], huff.sym_code_len[s]) for s in range(256) if huff.sym_code_len[s]})
        out += bytes([0xFF, 0xDA, 0x00, 6 + 2 * len(cs), len(cs)])
        for c in cs:
            out += bytes([comps[c][0], 0x11 if c else 0x00])
        out += bytes([ss, se, (ah << 4) | al])
        for i, toks in enumerate(parts):
            if i:
                out += bytes([0xFF, 0xD0 + (i - 1) % 8])
            out += entropy(toks, codes).replace(b"\xff", b"\xff\x00")
    return bytes(out) + b"\xff\xd9"


_cache = {}


def source(jpg: bytes):
    """(w, h, comps, hv, dqt, planes) of a baseline or progressive file, as build() takes them"""
    if b"\xff\xc2" in jpg[:jpg.find(b"\xff\xda")]:
        P = PM.parse(jpg)
        D = PM.decoded(jpg)
        G, coefs = D.G, D.coefs
    else:
        P = FM.parse(jpg)
        G = FM.geometry(P)
        coefs = FM.coefficients(P, G)
    comps = [(c[0], (c[1] << 4) | c[2], c[3]) for c in P["comps"]]
    hv = [(c[0], c[1]) for c in G["comps"]]
    dqt = {k: [int(x) for x in v] for k, v in P["dqt"].items()}
    return P["w"], P["h"], comps, hv, dqt, [np.asarray(p).astype(np.int64) for p in coefs]


def model(jpg: bytes, restart_rows: int = 0) -> bytes:
    """the progressive file of a baseline or progressive source; computed once per (stream, restart_rows)"""
    key = (jpg, restart_rows)
    out = _cache.get(key)
    if out is None:
        out = _cache[key] = build(*source(jpg), restart_rows)
    return out
