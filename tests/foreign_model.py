"""Plain Python / numpy baseline JPEG decoder (DESIGN.md "Decoding ordinary
baseline files"): marker parsing, Huffman decoding of one interleaved scan
with restart intervals, decode_model.py's IDCT passes, and libjpeg's
upsampling and colour rules for greyscale, 4:4:4, 4:2:2 and 4:2:0 at any
size.  The model of everything the GPU decoder accepts beyond the encoder's
own three-scan streams; pinned to Pillow's libjpeg-turbo by
tests/test_foreign_model.py.  All arithmetic is int64."""
import numpy as np

import decode_model as M

LAYOUT_HEAD = 9  # w, h, ncomp, hmax, vmax, mcus_x, mcus_y, ri, interleaved; then h, v, tq, bw, bh per component


class Reject(ValueError):
    pass


def _be16(b, i):
    return (b[i] << 8) | b[i + 1]


def parse(jpg: bytes) -> dict:
    if jpg[:2] != b"\xff\xd8":
        raise Reject("no SOI")
    P = {"dqt": {}, "dht": {}, "ri": 0, "comps": None, "scan": None}
    i = 2
    while i + 4 <= len(jpg):
        if jpg[i] != 0xFF:
            raise Reject(f"marker expected at {i}")
        m = jpg[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD9:
            break
        n = _be16(jpg, i + 2)
        q = jpg[i + 4:i + 2 + n]
        if m == 0xDB:
            o = 0
            while o + 65 <= len(q):
                if q[o] >> 4:
                    raise Reject("16-bit DQT")
                P["dqt"][q[o] & 15] = np.frombuffer(q, np.uint8, 64, o + 1).astype(np.int64)
                o += 65
        elif m == 0xC4:
            o = 0
            while o + 17 <= len(q):
                counts = list(q[o + 1:o + 17])
                ns = sum(counts)
                P["dht"][(q[o] >> 4, q[o] & 15)] = (counts, list(q[o + 17:o + 17 + ns]))
                o += 17 + ns
        elif m == 0xC0:
            if q[0] != 8:
                raise Reject("not 8-bit")
            P["h"], P["w"] = _be16(q, 1), _be16(q, 3)
            P["comps"] = [(q[6 + 3 * c], q[7 + 3 * c] >> 4, q[7 + 3 * c] & 15, q[8 + 3 * c]) for c in range(q[5])]
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Reject(f"SOF {m:02X}")
        elif m == 0xDD:
            P["ri"] = _be16(q, 0)
        elif m == 0xDA:
            if P["scan"] is not None:
                raise Reject("second scan")
            ns = q[0]
            sel = [(q[1 + 2 * k], q[2 + 2 * k] >> 4, q[2 + 2 * k] & 15) for k in range(ns)]
            e = i + 2 + n
            start = e
            while True:
                e = jpg.index(b"\xff", e)
                if jpg[e + 1] == 0 or (P["ri"] and 0xD0 <= jpg[e + 1] <= 0xD7):
                    e += 2
                elif jpg[e + 1] == 0xFF:
                    e += 1
                else:
                    break
            P["scan"] = (sel, jpg[start:e])
            i = e
            continue
        i += 2 + n
    if P["comps"] is None or P["scan"] is None:
        raise Reject("no SOF0 or SOS")
    return P


class _Huff:
    def __init__(self, counts, syms):
        self.map = {}
        code = k = 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                self.map[(l, code)] = syms[k]
                code += 1
                k += 1
            code <<= 1


class _Bits:
    def __init__(self, data: bytes):
        self.bits = np.unpackbits(np.frombuffer(data, np.uint8)).tolist() + [1] * 64
        self.p = 0

    def sym(self, t: _Huff):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bits[self.p]
            self.p += 1
            s = t.map.get((l, code))
            if s is not None:
                return s
        raise Reject("bad code")

    def mag(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bits[self.p]
            self.p += 1
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def geometry(P: dict) -> dict:
    """the layout mij_decoder_layout reports; a single component is 1x1 in effect"""
    comps = P["comps"]
    w, h = P["w"], P["h"]
    if len(comps) == 1:
        hv = [(1, 1)]
    else:
        hv = [(c[1], c[2]) for c in comps]
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return {"w": w, "h": h, "ncomp": len(comps), "hmax": hmax, "vmax": vmax, "mcus_x": mx, "mcus_y": my,
            "ri": P["ri"], "interleaved": 1,
            "comps": [(a, b, comps[c][3], mx * a, my * b) for c, (a, b) in enumerate(hv)]}


def layout_list(G: dict):
    out = [G["w"], G["h"], G["ncomp"], G["hmax"], G["vmax"], G["mcus_x"], G["mcus_y"], G["ri"], G["interleaved"]]
    for c in G["comps"]:
        out += list(c)
    return out


def coefficients(P: dict, G: dict):
    """per component (blocks_down * blocks_across, 64) int16, zigzag order, absolute DC"""
    sel, data = P["scan"]
    if [s[0] for s in sel] != [c[0] for c in P["comps"]]:
        raise Reject("scan is not all components in SOF order")
    tabs = {k: _Huff(*v) for k, v in P["dht"].items()}
    planes = [np.zeros((c[3] * c[4], 64), np.int64) for c in G["comps"]]
    # intervals: split at RSTn (only when a restart interval is in force)
    parts, cur, i = [], bytearray(), 0
    while i < len(data):
        b = data[i]
        if b == 0xFF and i + 1 < len(data):
            nx = data[i + 1]
            if nx == 0:
                cur.append(0xFF)
                i += 2
                continue
            if P["ri"] and 0xD0 <= nx <= 0xD7:
                if nx != 0xD0 + len(parts) % 8:
                    raise Reject("restart numbering")
                parts.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
        cur.append(b)
        i += 1
    parts.append(bytes(cur))
    nm = G["mcus_x"] * G["mcus_y"]
    ri = P["ri"] or nm
    if len(parts) != -(-nm // ri):
        raise Reject("interval count")
    for n, part in enumerate(parts):
        br = _Bits(part)
        pred = [0] * len(planes)
        for m in range(n * ri, min(nm, (n + 1) * ri)):
            my, mx = divmod(m, G["mcus_x"])
            for c, (hs, vs, _, bw, _) in enumerate(G["comps"]):
                dc, ac = tabs[(0, sel[c][1])], tabs[(1, sel[c][2])]
                for j in range(hs * vs):
                    blk = planes[c][(my * vs + j // hs) * bw + mx * hs + j % hs]
                    s = br.sym(dc)
                    pred[c] += br.mag(s) if s else 0
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.sym(ac)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                raise Reject("run past 63")
                            blk[k] = br.mag(s)
                            k += 1
                        elif r == 15:
                            k += 16
                        else:
                            break
    return [p.astype(np.int16) for p in planes]


def idct_plane(coefs, q, bw, bh):
    """uint8 padded (8*bh, 8*bw) plane from absolute-DC zigzag coefficients"""
    c = np.asarray(coefs, np.int64).reshape(-1, 64)
    d = np.zeros_like(c)
    d[:, M.ZZ] = c * np.asarray(q, np.int64).reshape(64)
    d = d.reshape(-1, 8, 8)
    ws = M.pass_1d(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)
    px = np.clip(M.pass_1d(ws, 18) + 128, 0, 255).astype(np.uint8)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw)


def h2v1_fancy(p):
    p = p.astype(np.int64)
    l = np.concatenate([p[:, :1], p[:, :-1]], 1)
    r = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.zeros((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + l + 1) >> 2
    out[:, 1::2] = (3 * p + r + 2) >> 2
    return out


def upsample(plane, G, c):
    """component c's padded sample plane -> (h, w) int64 at full resolution"""
    w, h = G["w"], G["h"]
    hs, vs = G["comps"][c][0], G["comps"][c][1]
    fx, fy = G["hmax"] // hs, G["vmax"] // vs
    cw, ch = -(-w // fx), -(-h // fy)  # libjpeg's downsampled_width / _height
    p = plane[:ch, :cw].astype(np.int64)
    if fx == 1 and fy == 1:
        return p
    if cw <= 2:  # libjpeg takes the fancy upsamplers only for downsampled_width > 2
        up = np.repeat(np.repeat(p, fy, 0), fx, 1)
    elif fy == 1:
        up = h2v1_fancy(p)
    else:
        up = M.upsample(p)
    return up[:h, :w]


def colour(y, cb, cr, order="rgb"):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    ch = (r, g, b) if order == "rgb" else (b, g, r)
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


class Decoded:
    def __init__(self, jpg: bytes):
        self.jpg = jpg
        P = parse(jpg)
        nc = len(P["comps"])
        if nc not in (1, 3):
            raise Reject(f"{nc} components")
        if nc == 3:
            hv = [(c[1], c[2]) for c in P["comps"]]
            if hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0] not in ((1, 1), (2, 1), (2, 2)):
                raise Reject(f"sampling {hv}")
        self.G = G = geometry(P)
        self.layout = layout_list(G)
        self.w, self.h = G["w"], G["h"]
        self.coefs = coefficients(P, G)
        self.dqt = [P["dqt"][c[2]] for c in G["comps"]]
        self.planes = [idct_plane(self.coefs[c], self.dqt[c], G["comps"][c][3], G["comps"][c][4]) for c in range(nc)]
        y = self.planes[0][:self.h, :self.w].astype(np.int64)
        self.y = y.astype(np.uint8)
        if nc == 1:
            self.rgb = self.bgr = np.repeat(self.y[:, :, None], 3, 2)
        else:
            cb, cr = upsample(self.planes[1], G, 1), upsample(self.planes[2], G, 2)
            self.rgb, self.bgr = colour(y, cb, cr, "rgb"), colour(y, cb, cr, "bgr")

    def pixels(self, order="rgb"):
        return self.rgb if order == "rgb" else self.bgr


_cache = {}


def decoded(jpg: bytes) -> Decoded:
    """computed once per stream and shared; callers leave it unchanged"""
    d = _cache.get(jpg)
    if d is None:
        d = _cache[jpg] = Decoded(jpg)
    return d
