"""numpy model of 4:4:0 (luma 1x2, chroma 1x1) on top of the
models that refuse it: foreign_model (parse, geometry, coefficients, IDCT,
colour), progressive_model (the scans of an SOF2 file), scaled_model (the
reduced IDCTs and the IDCT size per component), transform_model (block
permutations) and the two writers.  Only what differs is here: the
admission, libjpeg's h1v2_fancy_upsample, the choice between it and plain
row replication, and the swap of H and V under a transposing operation.
Pinned to Pillow and jpegtran by tests/test_s440_model.py.  All arithmetic
is int64."""
import numpy as np

import foreign_model as F
import progressive_model as PM
import progwrite_model as PW
import scaled_model as S
import transcode_model as TM
import transform_model as XM

PIX_H1V2, PIX_H1V2_REP = 6, 7  # csrc/mij_pixels.h
DENOMS = (1, 2, 4, 8)
SAMPLINGS = ((1, 1), (2, 1), (2, 2), (1, 2))  # luma H x V admitted with MIJ_ACCEPT_440


def is_progressive(jpg: bytes) -> bool:
    return b"\xff\xc2" in jpg[:jpg.find(b"\xff\xda")]


def h1v2_fancy(p):
    """(ch, cw) chroma samples -> (2 * ch, cw): each sample with its upper
    neighbour (rounding + 1) and its lower one (+ 2), the edge rows replicated;
    no horizontal neighbours, so no rule for small widths"""
    p = p.astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]], 0)
    dn = np.concatenate([p[1:], p[-1:]], 0)
    out = np.zeros((2 * p.shape[0], p.shape[1]), np.int64)
    out[0::2] = (3 * p + up + 1) >> 2
    out[1::2] = (3 * p + dn + 2) >> 2
    return out


def _parse(jpg: bytes):
    """(P, G, coefs) of a baseline or progressive stream under the admission with the bit set"""
    if is_progressive(jpg):
        P = _prog_parse(jpg)
    else:
        P = F.parse(jpg)
    nc = len(P["comps"])
    if nc not in (1, 3):
        raise F.Reject(f"{nc} components")
    if nc == 3:
        hv = [(c[1], c[2]) for c in P["comps"]]
        if hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0] not in SAMPLINGS:
            raise F.Reject(f"sampling {hv}")
    G = F.geometry(P)
    coefs = PM.coefficients(P, G) if "scans" in P else F.coefficients(P, G)
    return P, G, coefs


def _prog_parse(jpg: bytes) -> dict:
    """progressive_model.parse refuses luma 1x2 while it reads SOF2; nothing
    else in it depends on the sampling, so it parses the stream with that
    one byte declared 2x1 and the true byte is put back afterwards"""
    i = jpg.find(b"\xff\xc2")
    at = i + 4 + 6 + 1  # the H/V byte of component 0
    if jpg[i + 4 + 5] == 3 and jpg[at] == 0x12:
        P = PM.parse(jpg[:at] + b"\x21" + jpg[at + 1:])
        c = P["comps"][0]
        P["comps"][0] = (c[0], 1, 2, c[3])
        # the scans' intervals were counted on the 2x1 grid: the same number
        # of MCUs only if both grids agree, so count again on the true one
        G = F.geometry(P)
        for sc in P["scans"]:
            mcus = len(PM.scan_blocks(G, sc["comps"]))
            want = -(-mcus // sc["ri"]) if sc["ri"] else 1
            if len(sc["parts"]) != want:
                raise F.Reject("interval count")
        return P
    return PM.parse(jpg)


class Decoded:
    """one stream at full size, as foreign_model.Decoded"""

    def __init__(self, jpg: bytes):
        self.jpg = jpg
        P, G, coefs = _parse(jpg)
        nc = len(P["comps"])
        self.P, self.G = P, G
        self.layout = F.layout_list(G)
        if "scans" in P:  # served as an interleaved frame without restart intervals
            self.layout[7] = 0
        self.w, self.h = G["w"], G["h"]
        self.coefs = coefs
        self.dqt = [P["dqt"][c[2]] for c in G["comps"]]
        self.planes = [F.idct_plane(coefs[c], self.dqt[c], G["comps"][c][3], G["comps"][c][4]) for c in range(nc)]
        y = self.planes[0][:self.h, :self.w].astype(np.int64)
        if nc == 1:
            self.rgb = self.bgr = np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
        else:
            up = [upsample(self.planes[c], G, c) for c in (1, 2)]
            self.rgb, self.bgr = F.colour(y, up[0], up[1], "rgb"), F.colour(y, up[0], up[1], "bgr")

    def pixels(self, order="rgb"):
        return self.rgb if order == "rgb" else self.bgr


def upsample(plane, G, c):
    if (G["hmax"], G["vmax"]) != (1, 2):
        return F.upsample(plane, G, c)
    w, h = G["w"], G["h"]
    return h1v2_fancy(plane[:-(-h // 2), :w])[:h, :w]


_cache = {}


def decoded(jpg: bytes) -> Decoded:
    """computed once per stream and shared; callers leave it unchanged"""
    d = _cache.get(jpg)
    if d is None:
        d = _cache[jpg] = Decoded(jpg)
    return d


class Scaled:
    """one frame at 1/denom (1 included), as scaled_model.Scaled: layout, planes, rgb, bgr"""

    def __init__(self, m: Decoded, denom: int):
        self.denom = denom
        comps = S.comps_of(m)
        hv0 = comps[0][:2] if len(comps) == 3 else (1, 1)
        if hv0 != (1, 2):
            if denom == 1:
                self.ow, self.oh = m.w, m.h
                self.layout = [m.w, m.h, len(comps)] + [v for c in comps for v in (8, 0, 0, 8 * c[2], 8 * c[3])]
                self.planes, self.rgb, self.bgr = m.planes, m.rgb, m.bgr
                self.mode = None
                return
            s = S.Scaled(m.w, m.h, comps, m.coefs, m.dqt, denom)
            self.ow, self.oh, self.mode, self.layout = s.ow, s.oh, s.mode, s.layout
            self.planes, self.rgb, self.bgr = s.planes, s.rgb, s.bgr
            return
        s = 8 // denom
        self.ow, self.oh = -(-m.w * s // 8), -(-m.h * s // 8)
        # every component keeps S = s: nothing is upsampled by 2 both across and down
        self.comps = [(s, -(-m.w * s // 8), -(-m.h * vs * s // 16), -(-s * bw // 8) * 8, s * bh)
                      for _, vs, bw, bh in comps]
        self.mode = PIX_H1V2 if s > 1 else PIX_H1V2_REP  # libjpeg: no fancy upsampling at IDCT size 1
        self.layout = [self.ow, self.oh, 3] + [v for c in self.comps for v in c]
        self.planes = []
        for (_, _, bw, bh), (_, _, _, pitch, rows), cf, q in zip(comps, self.comps, m.coefs, m.dqt):
            px = S.idct_blocks(cf, q, s).reshape(bh, bw, s, s).transpose(0, 2, 1, 3).reshape(s * bh, s * bw)
            plane = np.zeros((rows, pitch), np.uint8)
            plane[:, :s * bw] = px
            self.planes.append(plane)
        y = self.planes[0][:self.oh, :self.ow].astype(np.int64)
        up = []
        for c in (1, 2):
            _, cw, ch, _, _ = self.comps[c]
            p = self.planes[c][:ch, :cw].astype(np.int64)
            p = h1v2_fancy(p) if self.mode == PIX_H1V2 else np.repeat(p, 2, 0)
            up.append(p[:self.oh, :self.ow])
        self.rgb, self.bgr = F.colour(y, up[0], up[1], "rgb"), F.colour(y, up[0], up[1], "bgr")

    def pixels(self, order="rgb"):
        return self.rgb if order == "rgb" else self.bgr


_scache = {}


def scaled(jpg: bytes, denom: int) -> Scaled:
    """computed once per (stream, scale) and shared; callers leave it unchanged"""
    key = (jpg, denom)
    s = _scache.get(key)
    if s is None:
        s = _scache[key] = Scaled(decoded(jpg), denom)
    return s


# ---- the writers ----------------------------------------------------------------
def parts(jpg: bytes, op="none", trim=False, crop=None):
    """transform_model.parts with the bit set: a transposing operation on H != V swaps them"""
    m = decoded(jpg)
    P, G = m.P, m.G
    planes = [np.asarray(p).astype(np.int64) for p in m.coefs]
    hv = [(c[0], c[1]) for c in G["comps"]]
    mw, mh = 8 * G["hmax"], 8 * G["vmax"]  # the source's MCU: crop, trim and the whole-MCU rule
    x, y, w, h = XM.kept(P["w"], P["h"], mw, mh, op, trim, crop)
    t = XM.PARTS[op][0]
    kx, ky = -(-w // mw), -(-h // mh)
    out = []
    for (a, b), p in zip(hv, planes):
        src = p.reshape(G["mcus_y"] * b, G["mcus_x"] * a, 64)
        part = src[y // mh * b:(y // mh + ky) * b, x // mw * a:(x // mw + kx) * a]
        out.append(XM.xform_blocks(part, op).reshape(-1, 64))
    comps = [(c[0], ((c[2] << 4) | c[1]) if t else ((c[1] << 4) | c[2]), c[3]) for c in P["comps"]]
    dqt = {k: (XM.transpose_dqt(v) if t else [int(q) for q in v]) for k, v in P["dqt"].items()}
    if t:
        w, h, hv = h, w, [(b, a) for a, b in hv]
    return w, h, comps, hv, dqt, out


_wcache = {}


def model(jpg: bytes, op="none", trim=False, crop=None, restart_rows=0, output="baseline") -> bytes:
    """the transformed (op "none" without a crop: transcoded) stream, baseline
    or progressive; XM.Refused as the library refuses.  restart_rows counts
    MCU rows of the output's grid (the writers take it from hv)."""
    key = (jpg, op, bool(trim), None if crop is None else tuple(crop), restart_rows, output)
    out = _wcache.get(key)
    if out is None:
        args = parts(jpg, op, trim, crop)
        try:
            out = (TM.build if output == "baseline" else PW.build)(*args, restart_rows)
        except ValueError as e:  # the restart interval
            raise XM.Refused(str(e))
        _wcache[key] = out
    return out
