"""Plain Python progressive JPEG decoder: SOF2, 8-bit,
Huffman; marker parsing with the scan-script rules of T.81 G.1.1.1, the four
decoding procedures of G.1.2 / G.2 (DC first, DC refinement, AC first with
EOB runs, AC refinement), restart intervals per scan, then foreign_model's
IDCT, upsampling and colour code.  decoded() returns what
foreign_model.decoded returns: layout, absolute coefficients per padded
plane, planes and pixels; blocks of a padded plane outside the component's
own block grid are never coded and stay zero.  Refusals carry the library's
wording.

Also a small progressive *encoder* from coefficient planes and a scan
script, spectral selection only (Ah = Al = 0): DC scans of any number of
components, AC bands with EOB runs, a restart interval per scan, optimal
Huffman tables per scan.  It writes the fixtures Pillow cannot (Ns = 2 DC
scans, DRI changing between scans, several AC bands)."""
import heapq

import numpy as np

import foreign_model as F

Reject = F.Reject
MAX_SCANS = 64


def _be16(b, i):
    return (b[i] << 8) | b[i + 1]


def parse(jpg: bytes, frame: int = 0) -> dict:
    """headers and scans; scans[k]: comps (indices), td, ta (table snapshots), ss, se, ah, al, ri, parts (unstuffed
    intervals), span (byte range of the entropy data in jpg), level"""
    pre = f"stream {frame}"
    if jpg[:2] != b"\xff\xd8":
        raise Reject(f"{pre}: no SOI")
    P = {"dqt": {}, "ri": 0, "comps": None, "scans": [], "adobe": -1}
    dht = {}
    ri = 0
    last_al = None
    i = 2
    while i + 4 <= len(jpg):
        if jpg[i] != 0xFF:
            raise Reject(f"{pre}: marker expected at byte {i}")
        m = jpg[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD9:
            break
        if 0xD0 <= m <= 0xD7:
            raise Reject(f"{pre}: restart marker RST{m - 0xD0} without a restart interval in force")
        n = _be16(jpg, i + 2)
        q = jpg[i + 4:i + 2 + n]
        if m == 0xDB:
            if P["scans"]:
                raise Reject(f"{pre}: DQT after the first scan of a progressive frame")
            o = 0
            while o + 65 <= len(q):
                if q[o] >> 4:
                    raise Reject(f"{pre}: 16-bit DQT (Pq {q[o] >> 4}) is not baseline 8-bit")
                P["dqt"][q[o] & 15] = np.frombuffer(q, np.uint8, 64, o + 1).astype(np.int64)
                o += 65
        elif m == 0xC4:
            o = 0
            while o + 17 <= len(q):
                counts = list(q[o + 1:o + 17])
                ns = sum(counts)
                if (q[o] >> 4) > 1 or (q[o] & 15) > 3:
                    raise Reject(f"{pre}: DHT Tc/Th {q[o]:02X}")
                dht[(q[o] >> 4, q[o] & 15)] = F._Huff(counts, list(q[o + 17:o + 17 + ns]))
                o += 17 + ns
        elif m == 0xC2:
            if q[0] != 8:
                raise Reject(f"{pre}: {q[0]}-bit samples (only 8-bit)")
            P["h"], P["w"] = _be16(q, 1), _be16(q, 3)
            nc = q[5]
            if nc not in (1, 3):
                raise Reject(f"{pre}: {nc} components (only greyscale and YCbCr)")
            P["comps"] = [(q[6 + 3 * c], q[7 + 3 * c] >> 4, q[7 + 3 * c] & 15, q[8 + 3 * c]) for c in range(nc)]
            if nc == 3:
                hv = [(c[1], c[2]) for c in P["comps"]]
                if hv[1] != (1, 1) or hv[2] != (1, 1):
                    raise Reject(f"{pre}: chroma sampling {hv[1][0]}x{hv[1][1]} / {hv[2][0]}x{hv[2][1]} (only 1x1)")
                if hv[0] not in ((1, 1), (2, 1), (2, 2)):
                    raise Reject(f"{pre}: luma sampling {hv[0][0]}x{hv[0][1]} (only 1x1, 2x1, 2x2)")
            last_al = [[-1] * 64 for _ in range(nc)]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Reject(f"{pre}: SOF 0x{m:02X} in a progressive stream")
        elif m == 0xDD:
            ri = _be16(q, 0)
        elif m == 0xEE:
            if len(q) >= 12 and q[:5] == b"Adobe":
                P["adobe"] = q[11]
        elif m == 0xDA:
            if P["comps"] is None:
                raise Reject(f"{pre}: SOS before SOF2")
            k = len(P["scans"])
            if k >= MAX_SCANS:
                raise Reject(f"{pre}: more than {MAX_SCANS} scans")
            ns = q[0]
            nc = len(P["comps"])
            if ns < 1 or ns > nc:
                raise Reject(f"{pre} scan {k}: {ns} components in a {nc}-component frame")
            ss, se, ah, al = q[1 + 2 * ns], q[2 + 2 * ns], q[3 + 2 * ns] >> 4, q[3 + 2 * ns] & 15
            if (se != 0) if ss == 0 else (se < ss or se > 63):
                raise Reject(f"{pre} scan {k}: Ss {ss} Se {se} (a DC scan has Se 0, an AC scan Ss <= Se <= 63)")
            if ss > 0 and ns != 1:
                raise Reject(f"{pre} scan {k}: AC scan of {ns} components (only 1)")
            if al > 13:
                raise Reject(f"{pre} scan {k}: Al {al} (at most 13)")
            comps, td, ta = [], [], None
            ids = [c[0] for c in P["comps"]]
            for j in range(ns):
                cid, t = q[1 + 2 * j], q[2 + 2 * j]
                c = ids.index(cid) if cid in ids else -1
                if c < 0 or (comps and c <= comps[-1]):
                    raise Reject(f"{pre} scan {k}: SOS selectors are not SOF2 components in order")
                comps.append(c)
                if ss == 0 and ah == 0:
                    if (0, t >> 4) not in dht:
                        raise Reject(f"{pre} scan {k}: DC Huffman table {t >> 4} missing before the scan")
                    td.append(dht[(0, t >> 4)])
                else:
                    td.append(None)
                if ss > 0:
                    if (1, t & 15) not in dht:
                        raise Reject(f"{pre} scan {k}: AC Huffman table {t & 15} missing before the scan")
                    ta = dht[(1, t & 15)]
                    if last_al[c][0] < 0:
                        raise Reject(f"{pre} scan {k}: AC scan of component {c} before its DC scan")
                for z in range(ss, se + 1):
                    prev = last_al[c][z]
                    if (ah != 0) if prev < 0 else (ah != prev or al != ah - 1):
                        after = "no scan, 0" if prev < 0 else f"Al {prev}"
                        raise Reject(f"{pre} scan {k}: component {c} coefficient {z}: Ah {ah} Al {al} after {after} "
                                     "(successive approximation out of order)")
                    last_al[c][z] = al
            level = 1
            for e in P["scans"]:
                if set(e["comps"]) & set(comps) and e["ss"] <= se and ss <= e["se"]:
                    level = max(level, e["level"] + 1)
            e = i + 2 + n
            start = e
            parts, cur = [], bytearray()
            nm = len(scan_blocks(F.geometry(P), comps))  # the scan's own MCUs
            want = -(-nm // ri) if ri else 1
            while True:
                f = jpg.find(b"\xff", e)
                if f < 0 or f + 1 >= len(jpg):
                    raise Reject(f"{pre}: scan {k} runs to the end")
                cur += jpg[e:f + 1]
                e = f
                b = jpg[e + 1]
                if b == 0:
                    e += 2
                elif b == 0xFF:
                    e += 1
                elif ri and 0xD0 <= b <= 0xD7:
                    if b != 0xD0 + len(parts) % 8:
                        raise Reject(f"{pre} scan {k}: restart marker RST{b - 0xD0} where RST{len(parts) % 8} is due "
                                     f"(interval {len(parts)})")
                    if len(parts) + 1 >= want:
                        raise Reject(f"{pre} scan {k}: more restart markers than its {want} intervals need")
                    parts.append(bytes(cur[:-1]))
                    cur = bytearray()
                    e += 2
                else:
                    parts.append(bytes(cur[:-1]))
                    break
            if len(parts) != want:
                raise Reject(f"{pre} scan {k}: {len(parts)} restart intervals, {want} expected ({nm} MCUs, interval {ri})")
            P["scans"].append({"comps": comps, "td": td, "ta": ta, "ss": ss, "se": se, "ah": ah, "al": al, "ri": ri,
                               "parts": parts, "span": (start, e), "level": level})
            i = e
            continue
        i += 2 + n
    if P["comps"] is None:
        raise Reject(f"{pre}: no SOF2")
    if len(P["comps"]) == 3 and P["adobe"] in (0, 2):
        raise Reject(f"{pre}: Adobe APP14 transform {P['adobe']} (RGB / YCCK), only YCbCr")
    for c, comp in enumerate(P["comps"]):
        if comp[3] not in P["dqt"]:
            raise Reject(f"{pre}: DQT {comp[3]} of component {c} missing")
        for z in range(64):
            if last_al[c][z] < 0:
                raise Reject(f"{pre}: incomplete scan script: component {c} coefficient {z} is never coded")
            if last_al[c][z] != 0:
                raise Reject(f"{pre}: incomplete scan script: component {c} coefficient {z} ends at Al {last_al[c][z]}")
    return P


def grids(G: dict):
    """per component the blocks across and down that its own scans cover"""
    out = []
    for hs, vs, _, _, _ in G["comps"]:
        wc, hc = -(-G["w"] * hs // G["hmax"]), -(-G["h"] * vs // G["vmax"])
        out.append((-(-wc // 8), -(-hc // 8)))
    return out


def scan_blocks(G: dict, comps):
    """the scan's MCUs: a list of lists of (component index in the scan, raster block in the padded plane)"""
    gr = grids(G)
    if len(comps) == 1:
        c = comps[0]
        bw = G["comps"][c][3]
        return [[(0, y * bw + x)] for y in range(gr[c][1]) for x in range(gr[c][0])]
    mcus = []
    for my in range(G["mcus_y"]):
        for mx in range(G["mcus_x"]):
            one = []
            for j, c in enumerate(comps):
                hs, vs, _, bw, _ = G["comps"][c]
                one += [(j, (my * vs + y) * bw + mx * hs + x) for y in range(vs) for x in range(hs)]
            mcus.append(one)
    return mcus


class _Reader(F._Bits):
    def __init__(self, data: bytes):
        super().__init__(data)
        self.n = 8 * len(data)

    def bit(self):
        if self.p >= self.n:
            raise Reject("corrupt entropy data (5)")
        self.p += 1
        return self.bits[self.p - 1]

    def raw(self, r):
        v = 0
        for _ in range(r):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, t):
        if self.p >= self.n:
            raise Reject("corrupt entropy data (5)")
        try:
            return self.sym(t)
        except F.Reject:
            raise Reject("corrupt entropy data (6)") from None


def _refine(blk, k, br, p1, m1):
    if br.bit() and not (blk[k] & p1):
        blk[k] += p1 if blk[k] >= 0 else m1


def decode_scan(sc: dict, G: dict, planes) -> None:
    """one scan into the planes (int64 arrays, (blocks, 64)); raises Reject with the status code in the text"""
    mcus = scan_blocks(G, sc["comps"])
    ri = sc["ri"] or len(mcus)
    if len(sc["parts"]) != -(-len(mcus) // ri):
        raise Reject(f"{len(sc['parts'])} restart intervals, {-(-len(mcus) // ri)} expected")
    ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
    p1, m1 = 1 << al, -(1 << al)
    for n, part in enumerate(sc["parts"]):
        br = _Reader(part)
        unit = mcus[n * ri:(n + 1) * ri]
        if ss == 0:
            pred = [0] * len(sc["comps"])
            for mcu in unit:
                for j, b in mcu:
                    blk = planes[sc["comps"][j]][b]
                    if ah == 0:
                        s = br.symbol(sc["td"][j])
                        if s > 15:
                            raise Reject("corrupt entropy data (6)")
                        pred[j] += br.mag(s) if s else 0
                        blk[0] = pred[j] << al
                    elif br.bit():
                        blk[0] |= p1
        else:
            plane = planes[sc["comps"][0]]
            eobrun = 0
            for m, mcu in enumerate(unit):
                blk = plane[mcu[0][1]]
                k = ss
                if ah == 0:
                    if eobrun:
                        eobrun -= 1
                        continue
                    while k <= se:
                        rs = br.symbol(sc["ta"])
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > se:
                                raise Reject("corrupt entropy data (9)")
                            blk[k] = br.mag(s) << al
                            k += 1
                        elif r == 15:
                            k += 16
                        else:
                            eobrun = (1 << r) + br.raw(r)
                            if eobrun > len(unit) - m:
                                raise Reject("corrupt entropy data (8)")
                            eobrun -= 1
                            break
                else:
                    if eobrun == 0:
                        while k <= se:
                            rs = br.symbol(sc["ta"])
                            r, s = rs >> 4, rs & 15
                            new = 0
                            if s:
                                if s != 1:
                                    raise Reject("corrupt entropy data (6)")
                                new = p1 if br.bit() else m1
                            elif r != 15:
                                eobrun = (1 << r) + br.raw(r)
                                if eobrun > len(unit) - m:
                                    raise Reject("corrupt entropy data (8)")
                                break
                            while k <= se:
                                if blk[k]:
                                    _refine(blk, k, br, p1, m1)
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if new:
                                if k > se:
                                    raise Reject("corrupt entropy data (9)")
                                blk[k] = new
                            k += 1
                    if eobrun:
                        while k <= se:
                            if blk[k]:
                                _refine(blk, k, br, p1, m1)
                            k += 1
                        eobrun -= 1
        if br.p > br.n:
            raise Reject("corrupt entropy data (5)")


def coefficients(P: dict, G: dict, frame: int = 0):
    planes = [np.zeros((c[3] * c[4], 64), np.int64) for c in G["comps"]]
    for k, sc in enumerate(P["scans"]):
        try:
            decode_scan(sc, G, planes)
        except Reject as e:
            raise Reject(f"stream {frame} scan {k}: {e}") from None
    return [p.astype(np.int16) for p in planes]


class Decoded:
    def __init__(self, jpg: bytes):
        self.jpg = jpg
        P = parse(jpg)
        nc = len(P["comps"])
        self.G = G = F.geometry(P)
        self.layout = F.layout_list(G)
        self.w, self.h = G["w"], G["h"]
        self.nscans = len(P["scans"])
        self.levels = max(s["level"] for s in P["scans"])
        self.script = [(s["comps"], s["ss"], s["se"], s["ah"], s["al"], s["ri"]) for s in P["scans"]]
        self.coefs = coefficients(P, G)
        self.dqt = [P["dqt"][c[2]] for c in G["comps"]]
        self.planes = [F.idct_plane(self.coefs[c], self.dqt[c], G["comps"][c][3], G["comps"][c][4]) for c in range(nc)]
        y = self.planes[0][:self.h, :self.w].astype(np.int64)
        self.y = y.astype(np.uint8)
        if nc == 1:
            self.rgb = self.bgr = np.repeat(self.y[:, :, None], 3, 2)
        else:
            cb, cr = F.upsample(self.planes[1], G, 1), F.upsample(self.planes[2], G, 2)
            self.rgb, self.bgr = F.colour(y, cb, cr, "rgb"), F.colour(y, cb, cr, "bgr")

    def pixels(self, order="rgb"):
        return self.rgb if order == "rgb" else self.bgr


_cache = {}


def decoded(jpg: bytes) -> Decoded:
    """computed once per stream and shared; callers leave it unchanged"""
    d = _cache.get(jpg)
    if d is None:
        d = _cache[jpg] = Decoded(jpg)
    return d


def inside(G: dict, c: int) -> np.ndarray:
    """raster indices of component c's padded plane that lie inside its own block grid"""
    gw, gh = grids(G)[c]
    bw = G["comps"][c][3]
    return np.array([y * bw + x for y in range(gh) for x in range(gw)])


# ---- encoder: spectral selection only ------------------------------------------
def _code_lengths(freq: dict):
    """Huffman code lengths <= 16 for the symbols of freq (T.81 K.2: a reserved
    all-ones code point, then the length limiting of Figure K.3)"""
    heap = [(f, i, (s,)) for i, (s, f) in enumerate(sorted(freq.items()))]
    heap.append((0, len(heap), (256,)))  # the reserved code point, deepest
    heapq.heapify(heap)
    depth = {s: 0 for _, _, (s,) in heap}
    tie = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
        tie += 1
    bits = [0] * (max(depth.values()) + 2)
    for s, d in depth.items():
        bits[max(d, 1)] += 1
    i = len(bits) - 1
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    bits = (bits + [0] * 17)[:17]
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the reserved code point
    syms = [s for s in sorted(depth, key=lambda s: (depth[s], -freq.get(s, 0), s)) if s != 256]
    return bits[1:17], syms


def _codes(counts, syms):
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[syms[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _mag(v):
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _scan_tokens(G, coefs, comps, ss, se, ri, eob_extra=0):
    """per restart interval a list of tokens (table-relative symbol, extra value, extra bits)"""
    mcus = scan_blocks(G, comps)
    ri = ri or len(mcus)
    out = []
    for u0 in range(0, len(mcus), ri):
        unit, toks = mcus[u0:u0 + ri], []
        if ss == 0:
            pred = [0] * len(comps)
            for mcu in unit:
                for j, b in mcu:
                    dc = int(coefs[comps[j]][b][0])
                    s, bits = _mag(dc - pred[j])
                    pred[j] = dc
                    toks.append((j, s, bits, s))
        else:
            run = 0

            def flush(run):
                if run:
                    r = run.bit_length() - 1
                    toks.append((0, r << 4, run - (1 << r), r))

            for mcu in unit:
                blk = coefs[comps[0]][mcu[0][1]]
                nz = [k for k in range(ss, se + 1) if blk[k]]
                if nz:
                    flush(run)
                    run = 0
                k0 = ss
                for k in nz:
                    z = k - k0
                    while z > 15:
                        toks.append((0, 0xF0, 0, 0))
                        z -= 16
                    s, bits = _mag(int(blk[k]))
                    toks.append((0, (z << 4) | s, bits, s))
                    k0 = k + 1
                if k0 <= se:
                    run += 1
                    if run == 0x7FFF:
                        flush(run)
                        run = 0
            flush(run + (eob_extra if u0 + ri >= len(mcus) else 0))
        out.append(toks)
    return out


def _entropy(tokens, codes):
    acc = nb = 0
    out = bytearray()
    for t, sym, extra, nextra in tokens:
        code, l = codes[t][sym]
        acc = (acc << (l + nextra)) | (code << nextra) | extra
        nb += l + nextra
        while nb >= 8:
            byte = (acc >> (nb - 8)) & 0xFF
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
            nb -= 8
        acc &= (1 << nb) - 1
    if nb:
        byte = ((acc << (8 - nb)) | ((1 << (8 - nb)) - 1)) & 0xFF
        out.append(byte)
        if byte == 0xFF:
            out.append(0)
    return bytes(out)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def encode(G: dict, coefs, dqt: dict, script, eob_extra=None, early_dht=False) -> bytes:
    """G: foreign_model.geometry's dict; coefs: absolute coefficients per padded
    plane; dqt: {Tq: 64 values, zigzag}; script: [(components, Ss, Se, Ri)],
    Ah = Al = 0.  Component ids are 1..n; scan k's tables are written before it
    under ids 0.. (DC: one per component).  eob_extra = (scan, n): that scan's
    last EOB run is coded n blocks too long (a corrupt stream for the tests).
    early_dht: the first scan's tables are written in front of SOF2, under ids
    1.. instead of 0.. (so a DC scan of three components uses Th 1, 2 and 3)."""
    out = bytearray(b"\xff\xd8")
    for tq in sorted(dqt):
        out += _seg(0xDB, bytes([tq]) + bytes(int(v) for v in dqt[tq]))
    nc = G["ncomp"]
    sof = bytes([8]) + G["h"].to_bytes(2, "big") + G["w"].to_bytes(2, "big") + bytes([nc])
    for c, (hs, vs, tq, _, _) in enumerate(G["comps"]):
        sof += bytes([c + 1, (hs << 4) | vs, tq])
    sof_seg = _seg(0xC2, sof)
    if not early_dht:
        out += sof_seg
    cur_ri = 0
    for k, (comps, ss, se, ri) in enumerate(script):
        if ri != cur_ri:
            out += _seg(0xDD, ri.to_bytes(2, "big"))
            cur_ri = ri
        extra = eob_extra[1] if eob_extra and eob_extra[0] == k else 0
        parts = _scan_tokens(G, coefs, comps, ss, se, ri, extra)
        ntab = len(comps) if ss == 0 else 1
        id0 = 1 if k == 0 and early_dht else 0
        codes = []
        for t in range(ntab):
            freq = {}
            for toks in parts:
                for tt, sym, _, _ in toks:
                    if tt == t:
                        freq[sym] = freq.get(sym, 0) + 1
            if not freq:
                freq = {0: 1}
            counts, syms = _code_lengths(freq)
            out += _seg(0xC4, bytes([((0 if ss == 0 else 1) << 4) | (t + id0)]) + bytes(counts) + bytes(syms))
            codes.append(_codes(counts, syms))
        if k == 0 and early_dht:
            out += sof_seg
        sos = bytes([len(comps)])
        for j, c in enumerate(comps):
            sos += bytes([c + 1, ((j + id0) << 4) if ss == 0 else id0])
        out += _seg(0xDA, sos + bytes([ss, se, 0]))
        for n, toks in enumerate(parts):
            if n:
                out += bytes([0xFF, 0xD0 + (n - 1) % 8])
            out += _entropy(toks, codes)
    return bytes(out + b"\xff\xd9")
