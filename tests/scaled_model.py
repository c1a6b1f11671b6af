"""numpy model of decoding at 1/2, 1/4 and 1/8 scale:
libjpeg's reduced IDCTs (jidctred.c: 4x4, 2x2, 1x1), its choice of an IDCT
size per component (jdmaster.c) and what is left of upsampling, on top of
foreign_model.Decoded's coefficients, quantisers and geometry.  Pinned to
Pillow's draft decode by tests/test_scaled_model.py.  All arithmetic is
int64, so nothing here can wrap."""
import numpy as np

import decode_model as M
import foreign_model as F

DENOMS = (2, 4, 8)
PIX_GREY, PIX_444, PIX_H2V1, PIX_H2V1_REP = 0, 1, 2, 3  # csrc/mij_pixels.h


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def pass4(i, shift):
    """jpeg_idct_4x4's 1-D pass along the LAST axis (8 long, element 4 unused) -> 4"""
    i0, i1, i2, i3, _, i5, i6, i7 = (i[..., k] for k in range(8))
    t0 = i0 << 14
    t2 = i2 * 15137 - i6 * 6270
    t10, t12 = t0 + t2, t0 - t2
    a = -i7 * 1730 + i5 * 11893 - i3 * 17799 + i1 * 8697
    b = -i7 * 4176 - i5 * 4926 + i3 * 7373 + i1 * 20995
    return descale(np.stack([t10 + b, t12 + a, t12 - a, t10 - b], -1), shift)


def pass2(i, shift):
    """jpeg_idct_2x2's 1-D pass along the LAST axis (elements 0, 1, 3, 5, 7 used) -> 2"""
    i0, i1, _, i3, _, i5, _, i7 = (i[..., k] for k in range(8))
    t10 = i0 << 15
    t0 = -i7 * 5906 + i5 * 6967 - i3 * 10426 + i1 * 29692
    return descale(np.stack([t10 + t0, t10 - t0], -1), shift)


def dequantised(coefs, q):
    """(nblocks, 8, 8) natural-order blocks from absolute-DC zigzag coefficients"""
    c = np.asarray(coefs, np.int64).reshape(-1, 64)
    d = np.zeros_like(c)
    d[:, M.ZZ] = c * np.asarray(q, np.int64).reshape(64)
    return d.reshape(-1, 8, 8)


def idct_blocks(coefs, q, S):
    """(nblocks, S, S) uint8 samples"""
    d = dequantised(coefs, q)
    if S == 8:
        ws = M.pass_1d(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)
        px = M.pass_1d(ws, 18)
    elif S == 4:
        ws = pass4(d.transpose(0, 2, 1), 12).transpose(0, 2, 1)  # down the columns: (n, 4, 8)
        px = pass4(ws, 19)
    elif S == 2:
        ws = pass2(d.transpose(0, 2, 1), 13).transpose(0, 2, 1)
        px = pass2(ws, 20)
    else:
        px = descale(d[:, :1, :1], 3)
    return np.clip(px + 128, 0, 255).astype(np.uint8)


def geometry(w, h, comps, denom):
    """comps: (hs, vs, bw, bh) per component (a single component: 1 x 1).
    -> ow, oh, mode (PIX_*), [(S, cw, ch, pitch, rows)], [(fx, fy)]"""
    s = 8 // denom
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    ow, oh = -(-w * s // 8), -(-h * s // 8)
    out, ups = [], []
    for hs, vs, bw, bh in comps:
        S = s
        while S < 8 and (hmax * s) % (hs * S * 2) == 0 and (vmax * s) % (vs * S * 2) == 0:
            S *= 2
        cw, ch = -(-w * hs * S // (hmax * 8)), -(-h * vs * S // (vmax * 8))
        out.append((S, cw, ch, -(-S * bw // 8) * 8, S * bh))
        ups.append((hmax * s // (hs * S), vmax * s // (vs * S)))
    if len(comps) == 1:
        mode = PIX_GREY
    elif ups[1] == (1, 1):
        mode = PIX_444
    elif ups[1] == (2, 1):
        mode = PIX_H2V1 if out[1][1] > 2 and s > 1 else PIX_H2V1_REP
    else:
        raise F.Reject(f"upsampling {ups[1]} at 1/{denom}")
    return ow, oh, mode, out, ups


class Scaled:
    """one frame at 1/denom: layout (the list mij_decoder_scaled_layout
    gives), planes (padded: rows x pitch, the bytes past S * bw are 0), rgb, bgr"""

    def __init__(self, w, h, comps, coefs, dqt, denom):
        self.denom = denom
        self.ow, self.oh, self.mode, self.comps, ups = geometry(w, h, comps, denom)
        self.layout = [self.ow, self.oh, len(comps)] + [v for c in self.comps for v in c]
        self.planes = []
        for (hs, vs, bw, bh), (S, cw, ch, pitch, rows), cf, q in zip(comps, self.comps, coefs, dqt):
            px = idct_blocks(cf, q, S).reshape(bh, bw, S, S).transpose(0, 2, 1, 3).reshape(S * bh, S * bw)
            plane = np.zeros((rows, pitch), np.uint8)
            plane[:, :S * bw] = px
            self.planes.append(plane)
        y = self.planes[0][:self.oh, :self.ow].astype(np.int64)
        if len(comps) == 1:
            self.rgb = self.bgr = np.repeat(y.astype(np.uint8)[:, :, None], 3, 2)
        else:
            up = []
            for c in (1, 2):
                _, cw, ch, _, _ = self.comps[c]
                p = self.planes[c][:ch, :cw].astype(np.int64)
                if self.mode == PIX_H2V1:
                    p = F.h2v1_fancy(p)
                elif self.mode == PIX_H2V1_REP:
                    p = np.repeat(p, 2, 1)
                up.append(p[:self.oh, :self.ow])
            self.rgb, self.bgr = F.colour(y, up[0], up[1], "rgb"), F.colour(y, up[0], up[1], "bgr")
        for a in (self.rgb, self.bgr, *self.planes):
            a.setflags(write=False)

    def pixels(self, order="rgb"):
        return self.rgb if order == "rgb" else self.bgr


def comps_of(m: F.Decoded):
    return [(c[0], c[1], c[3], c[4]) for c in m.G["comps"]]


_cache = {}


def scaled(m: F.Decoded, denom: int) -> Scaled:
    """computed once per (stream, scale) and shared; callers leave it unchanged"""
    key = (m.jpg, denom)
    s = _cache.get(key)
    if s is None:
        s = _cache[key] = Scaled(m.w, m.h, comps_of(m), m.coefs, m.dqt, denom)
    return s


def scaled_legacy(Y, Cb, Cr, lq, cq, w, h, denom) -> Scaled:
    """a frame of the encoder's own shape (4:2:0, multiples of 16, DC stored
    as the raster-order difference, as decode_model takes it)"""
    coefs = []
    for p in (Y, Cb, Cr):
        c = np.asarray(p, np.int64).reshape(-1, 64).copy()
        c[:, 0] = np.cumsum(c[:, 0])
        coefs.append(c)
    comps = [(2, 2, w // 8, h // 8), (1, 1, w // 16, h // 16), (1, 1, w // 16, h // 16)]
    return Scaled(w, h, comps, coefs, [lq, cq, cq], denom)


def idct_float(coefs, q, S):
    """the float64 reduced IDCT of the same coefficients, clamped to 0..255:
    what jidctred.c's integer forms approximate, i.e. the 8x8 inverse DCT
    averaged over (8/S) x (8/S) cells.  (Coefficient 4 of a 1-D pass cancels
    in the average of 2, coefficients 2, 4 and 6 in the average of 4, which is
    why the integer forms never read them.)"""
    d = dequantised(coefs, q).astype(np.float64)
    k = np.arange(8)
    B = 0.5 * np.cos((2 * k[:, None] + 1) * k[None, :] * np.pi / 16)  # [x, u]
    B[:, 0] *= np.sqrt(0.5)
    B = B.reshape(S, 8 // S, 8).mean(1)
    return np.clip(np.einsum("xu,nuv,yv->nxy", B, d, B) + 128.0, 0.0, 255.0)
