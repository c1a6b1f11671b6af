"""numpy model of the decoder's pixel path (DESIGN.md "Decode to pixels"):
libjpeg's "islow" IDCT, h2v2 "fancy" upsampling and fixed-point colour
conversion, integer only, on the encoder's coefficient planes (per component
blocks in raster order, 64 zigzag coefficients, DC as the coded difference).
All arithmetic is int64, so nothing here can wrap."""
import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
               13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59,
               52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def pass_1d(i, shift):
    """the 1-D pass along the LAST axis (8 long) with DESCALE by `shift`"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (i[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], -1)
    return (out + (1 << (shift - 1))) >> shift


def dequant(coefs, q):
    """(nblocks, 8, 8) natural-order dequantised blocks with absolute DCs"""
    c = np.asarray(coefs, np.int64).reshape(-1, 64).copy()
    c[:, 0] = np.cumsum(c[:, 0])
    d = np.zeros_like(c)
    d[:, ZZ] = c * np.asarray(q, np.int64).reshape(64)
    return d.reshape(-1, 8, 8)


def idct_plane(coefs, q, w, h):
    """uint8 (h, w) plane of a component's zigzag coefficient plane"""
    d = dequant(coefs, q)
    ws = pass_1d(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)  # down each column
    px = np.clip(pass_1d(ws, 18) + 128, 0, 255).astype(np.uint8)
    return px.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w)


def upsample(p):
    """2x both ways, edges replicated"""
    p = p.astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]])
    dn = np.concatenate([p[1:], p[-1:]])
    out = np.zeros((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for row, nb in ((0, up), (1, dn)):
        s = 3 * p + nb
        sl = np.concatenate([s[:, :1], s[:, :-1]], 1)
        sr = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[row::2, 0::2] = (3 * s + sl + 8) >> 4
        out[row::2, 1::2] = (3 * s + sr + 7) >> 4
    return out


def planes(Y, Cb, Cr, lq, cq, w, h):
    return idct_plane(Y, lq, w, h), idct_plane(Cb, cq, w // 2, h // 2), idct_plane(Cr, cq, w // 2, h // 2)


def colour(y, cb, cr, order="rgb"):
    y, cb, cr = y.astype(np.int64), upsample(cb) - 128, upsample(cr) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    ch = (r, g, b) if order == "rgb" else (b, g, r)
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def decode(Y, Cb, Cr, lq, cq, w, h, order="rgb"):
    """(pixels (h, w, 3), (y, cb, cr) planes); lq / cq: the DQTs in zigzag order"""
    pl = planes(Y, Cb, Cr, lq, cq, w, h)
    return colour(*pl, order), pl


def stream_dqt(jpg: bytes):
    """the (luma, chroma) DQTs of a baseline stream, in zigzag order as stored"""
    t, i = {}, 2
    while jpg[i + 1] != 0xDA:
        n = (jpg[i + 2] << 8) | jpg[i + 3]
        if jpg[i + 1] == 0xDB:
            for o in range(i + 4, i + 2 + n, 65):
                t[jpg[o] & 15] = np.frombuffer(jpg, np.uint8, 64, o + 1).astype(np.int64)
        i += 2 + n
    return t[0], t[1]
