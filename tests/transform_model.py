"""Plain numpy model of the lossless transforms (include/mijpeg.h
mij_decoder_transform): crop, then the edge rule, then flip / transpose /
rotation, all on the quantised coefficients; the result is coded by
transcode_model.build.  The planes go to natural order, their blocks and the
8x8 coefficients inside them are sliced, transposed and reversed with numpy
indexing, and flipped axes take the sign (-1)^frequency -- no table of the
library's is used.  Pinned to independent code (the float IDCT, Pillow) by
tests/test_transform_model.py; the kernels must give these bytes
(tests/test_transform_gpu.py)."""
import struct

import numpy as np

import decode_model as M
import foreign_cases as FC
import foreign_model as FM
import transcode_model as TM

OPS = ["none", "flip_h", "flip_v", "transpose", "transverse", "rot90", "rot180", "rot270"]  # MIJ_XF_*
# (transpose, then mirror the output left-right, and / or top-bottom)
PARTS = {"none": (0, 0, 0), "flip_h": (0, 1, 0), "flip_v": (0, 0, 1), "transpose": (1, 0, 0),
         "transverse": (1, 1, 1), "rot90": (1, 1, 0), "rot180": (0, 1, 1), "rot270": (1, 0, 1)}
_ALT = np.array([1, -1, 1, -1, 1, -1, 1, -1], np.int64)


class Refused(ValueError):
    pass


def kept(w, h, mw, mh, op, trim=False, crop=None):
    """(x, y, w, h) of the part of a w x h source with mw x mh MCUs that the
    operation keeps: the crop, then the edge rule; Refused as the library refuses"""
    if op not in PARTS:
        raise Refused(f"operation {op!r}")
    x, y = 0, 0
    if crop is not None:
        x, y, cw, ch = crop
        if cw < 1 or ch < 1:
            raise Refused("empty crop")
        if x < 0 or y < 0 or x + cw > w or y + ch > h:
            raise Refused("crop outside the frame")
        if x % mw or y % mh:
            raise Refused("crop not MCU-aligned")
        w, h = cw, ch
    t, fh, fv = PARTS[op]
    mir_h, mir_v = (fv, fh) if t else (fh, fv)  # of the source
    if mir_h and w % mw:
        if not trim:
            raise Refused(f"width {w} is not whole MCUs")
        w -= w % mw
        if not w:
            raise Refused("no width left")
    if mir_v and h % mh:
        if not trim:
            raise Refused(f"height {h} is not whole MCUs")
        h -= h % mh
        if not h:
            raise Refused("no height left")
    return x, y, w, h


def xform_blocks(b, op):
    """b: (blocks down, blocks across, 64) zigzag coefficients -> the same of the transformed plane"""
    t, fh, fv = PARTS[op]
    bh, bw = b.shape[:2]
    nat = np.zeros_like(b)
    nat[:, :, M.ZZ] = b
    nat = nat.reshape(bh, bw, 8, 8)  # [.., v, u]
    if t:
        nat = nat.transpose(1, 0, 3, 2)
    if fh:
        nat = nat[:, ::-1] * _ALT[None, None, None, :]
    if fv:
        nat = nat[::-1] * _ALT[None, None, :, None]
    nat = np.ascontiguousarray(nat)
    return nat.reshape(nat.shape[0], nat.shape[1], 64)[:, :, M.ZZ]


def mapping(sbw, sbh, ox, oy, kw, kh, op):
    """for a source plane of sbw x sbh blocks of which kw x kh blocks at (ox, oy)
    are kept: per destination block (raster) and zigzag position the
    (source block, source position, sign) -- the model run on numbered coefficients"""
    ids = (np.arange(sbw * sbh * 64, dtype=np.int64) + 1).reshape(sbh, sbw, 64)
    out = xform_blocks(ids[oy:oy + kh, ox:ox + kw], op).reshape(-1, 64)
    a = np.abs(out) - 1
    return np.stack([a // 64, a % 64, np.sign(out)], -1)


def transpose_dqt(q):
    nat = np.zeros(64, np.int64)
    nat[M.ZZ] = np.asarray(q, np.int64)
    return [int(v) for v in nat.reshape(8, 8).T.ravel()[M.ZZ]]


_src = {}


def source(jpg: bytes):
    """(P, G, planes) of a one-scan stream, computed once and shared"""
    s = _src.get(jpg)
    if s is None:
        P = FM.parse(jpg)
        G = FM.geometry(P)
        s = _src[jpg] = (P, G, [p.astype(np.int64) for p in FM.coefficients(P, G)])
    return s


def parts(jpg: bytes, op="none", trim=False, crop=None):
    """(w, h, comps, hv, dqt, planes) of the transformed image, as transcode_model.build takes them"""
    P, G, planes = source(jpg)
    hv = [(c[0], c[1]) for c in G["comps"]]
    mw, mh = 8 * G["hmax"], 8 * G["vmax"]
    x, y, w, h = kept(P["w"], P["h"], mw, mh, op, trim, crop)
    t = PARTS[op][0]
    if t and any(a != b for a, b in hv):
        raise Refused(f"sampling {hv} under transposition")
    kx, ky = -(-w // mw), -(-h // mh)
    out = []
    for (a, b), p in zip(hv, planes):
        src = p.reshape(G["mcus_y"] * b, G["mcus_x"] * a, 64)
        part = src[y // mh * b:(y // mh + ky) * b, x // mw * a:(x // mw + kx) * a]
        out.append(xform_blocks(part, op).reshape(-1, 64))
    comps = [(c[0], ((c[2] << 4) | c[1]) if t else ((c[1] << 4) | c[2]), c[3]) for c in P["comps"]]
    dqt = {k: (transpose_dqt(v) if t else [int(q) for q in v]) for k, v in P["dqt"].items()}
    if t:
        w, h, hv = h, w, [(b, a) for a, b in hv]
    return w, h, comps, hv, dqt, out


_cache = {}


def model(jpg: bytes, op="none", trim=False, crop=None, restart_rows=0) -> bytes:
    """the transformed stream; computed once per case and shared"""
    key = (jpg, op, bool(trim), None if crop is None else tuple(crop), restart_rows)
    out = _cache.get(key)
    if out is None:
        w, h, comps, hv, dqt, planes = parts(jpg, op, trim, crop)
        try:
            out = TM.build(w, h, comps, hv, dqt, planes, restart_rows)
        except ValueError as e:  # the restart interval
            raise Refused(str(e))
        _cache[key] = out
    return out


# ---- EXIF orientation: hand-built segments for the tests ------------------------------
def app1(order: str, orientation: int, ifd: int = 8, cut: int = 0, tag: int = 0x0112) -> bytes:
    """an APP1 segment: Exif, an 8-byte TIFF header, IFD0 with one entry; cut bytes dropped from its end"""
    e = "<" if order == "II" else ">"
    tiff = order.encode() + struct.pack(e + "HI", 42, ifd)
    tiff += struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", tag, 3, 1, orientation, 0) + struct.pack(e + "I", 0)
    body = b"Exif\0\0" + tiff
    body = body[:len(body) - cut]
    return b"\xff\xe1" + struct.pack(">H", 2 + len(body)) + body


def spliced(name: str, seg: bytes) -> bytes:
    j = FC.jpg(name)
    return j[:2] + seg + j[2:]
