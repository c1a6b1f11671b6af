"""Plain numpy model of encoding as libjpeg does (include/
mijpeg.h mij_encode_libjpeg): the IJG scaling of the Annex K tables, libjpeg's
fixed-point colour conversion, its h2v1 / h2v2 downsamplers without smoothing,
its edge rules (pixels replicated to the right and up to a whole row group
downward, then the component's last sample row; dummy blocks with the DC of
the block before them in the MCU), the "islow" forward DCT and the quantiser
that rounds the magnitude; the bytes of transcode_model.build.  All
arithmetic is int64 and stays inside int32 (ijg_check.cpp shows it for the
C++ the kernel runs).  Pinned to Pillow's libjpeg-turbo and to a manifest of
digests by tests/test_ijg_model.py; the kernel must give these planes and
bytes (tests/test_ijg_gpu.py)."""
import numpy as np

import decode_model as M
import sampling_model as SM
import transcode_model as TM

SAMPLINGS = SM.SAMPLINGS

LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)


def FIX(x: float) -> int:
    return int(np.floor(x * 65536 + 0.5))


def quality_tables(q: int):
    """(luma, chroma) in natural order: jpeg_set_quality with force_baseline"""
    if not 1 <= q <= 100:
        raise ValueError(f"quality {q}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * s + 50) // 100, 1, 255) for b in (LUMA_Q, CHROMA_Q))


def dqt_bytes(q: int) -> bytes:
    """what mij_libjpeg_tables returns: luma then chroma, zigzag order"""
    lq, cq = quality_tables(q)
    return bytes(int(lq[z]) for z in M.ZZ) + bytes(int(cq[z]) for z in M.ZZ)


def ycc(frame_bgr: np.ndarray):
    b, g, r = (frame_bgr[..., c].astype(np.int64) for c in range(3))
    y = (FIX(.299) * r + FIX(.587) * g + FIX(.114) * b + 32768) >> 16
    cb = (-FIX(.168735892) * r - FIX(.331264108) * g + FIX(.5) * b + (128 << 16) + 32767) >> 16
    cr = (FIX(.5) * r - FIX(.418687589) * g - FIX(.081312411) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def real_extent(w: int, h: int, sampling: str, c: int):
    """(samples across, samples down, real blocks across, real blocks down) of component c"""
    hmax, vmax = SAMPLINGS[sampling]
    wc, hc = (w, h) if c == 0 else (-(-w // hmax), -(-h // vmax))
    return wc, hc, -(-wc // 8), -(-hc // 8)


def samples(frame_bgr: np.ndarray, sampling: str):
    """per component the int64 sample plane over its real blocks"""
    h, w = frame_bgr.shape[:2]
    hmax, vmax = SAMPLINGS[sampling]
    ncomp = 1 if sampling == "gray" else 3
    # pixels: to the right as far as any real block reaches, downward to a whole row group
    pw = max(real_extent(w, h, sampling, c)[2] * 8 * (1 if c == 0 else hmax) for c in range(ncomp))
    ph = -(-h // vmax) * vmax
    px = np.pad(frame_bgr, ((0, ph - h), (0, pw - w), (0, 0)), mode="edge")
    y, cb, cr = ycc(px)
    out = []
    for c, p in enumerate((y, cb, cr)[:ncomp]):
        wc, hc, rbw, rbh = real_extent(w, h, sampling, c)
        if c and hmax == 2:
            bias = np.arange(p.shape[1] // 2, dtype=np.int64) & 1
            if vmax == 2:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + bias[None, :]) >> 2
            else:
                p = (p[:, 0::2] + p[:, 1::2] + bias[None, :]) >> 1
        p = p[:hc, :rbw * 8]
        out.append(np.pad(p, ((0, rbh * 8 - hc), (0, 0)), mode="edge"))  # the last sample row, replicated
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_pass(d, rows: bool):
    """jfdctint.c's 1-D pass along the last axis of d (..., 8) int64"""
    sh = 11 if rows else 15
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if rows:
        o[0], o[4] = (t10 + t11) * 4, (t10 - t11) * 4
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    e = (t12 + t13) * 4433
    o[2] = _descale(e + t13 * 6270, sh)
    o[6] = _descale(e - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    p4, p5, p6, p7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    q1, q2 = z1 * -7373, z2 * -20995
    q3, q4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(p4 + q1 + q3, sh)
    o[5] = _descale(p5 + q2 + q4, sh)
    o[3] = _descale(p6 + q2 + q3, sh)
    o[1] = _descale(p7 + q1 + q4, sh)
    return np.stack(o, -1)


def fdct(blocks: np.ndarray) -> np.ndarray:
    """(n, 8, 8) samples [y][x] -> (n, 8, 8) [v][u], 8 times the true DCT"""
    r = fdct_pass(blocks.astype(np.int64) - 128, True)
    return fdct_pass(r.transpose(0, 2, 1), False).transpose(0, 2, 1)


def quantise(coef: np.ndarray, q_natural) -> np.ndarray:
    """(n, 64) natural order -> (n, 64) natural order"""
    d = 8 * np.asarray(q_natural, np.int64)[None, :]
    return np.sign(coef) * ((np.abs(coef) + (d >> 1)) // d)


def blocks_of(plane: np.ndarray) -> np.ndarray:
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


def planes(frame_bgr: np.ndarray, quality: int, sampling: str):
    """per component (blocks of the MCU-padded grid, 64) int64: raster blocks,
    zigzag inside, DC absolute, dummy blocks filled as libjpeg fills them"""
    frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
    h, w = frame_bgr.shape[:2]
    G = SM.grid(w, h, sampling)
    tabs = quality_tables(quality)
    out = []
    for c, s in enumerate(samples(frame_bgr, sampling)):
        hs, vs, _, bw, bh = G["comps"][c]
        _, _, rbw, rbh = real_extent(w, h, sampling, c)
        real = quantise(fdct(blocks_of(s)).reshape(-1, 64), tabs[1 if c else 0])[:, M.ZZ].reshape(rbh, rbw, 64)
        P = np.zeros((bh, bw, 64), np.int64)
        P[:rbh, :rbw] = real
        for by in range(rbh):  # to the right of a real block: its DC
            for bx in range(rbw, bw):
                P[by, bx, 0] = P[by, bx - 1, 0]
        for by in range(rbh, bh):  # a dummy row: the DC of the MCU's last block in the row above
            for bx in range(bw):
                P[by, bx, 0] = P[by - 1, bx // hs * hs + hs - 1, 0]
        out.append(P.reshape(-1, 64))
    return out


class Model:
    def __init__(self, frame_bgr: np.ndarray, quality: int, restart_rows: int, sampling: str):
        frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
        self.h, self.w = h, w = frame_bgr.shape[:2]
        self.sampling = sampling
        self.G = G = SM.grid(w, h, sampling)
        self.planes = planes(frame_bgr, quality, sampling)
        self.layout = [w, h, G["ncomp"], G["hmax"], G["vmax"], G["mcus_x"], G["mcus_y"], restart_rows * G["mcus_x"], 1]
        for c in G["comps"]:
            self.layout += list(c)
        lq, cq = quality_tables(quality)
        self.dqt = [np.array([int(t[z]) for z in M.ZZ], np.int64) for t in ((lq,) if sampling == "gray" else (lq, cq, cq))]
        dqt = {0: [int(x) for x in self.dqt[0]]}
        if sampling == "gray":
            comps = [(1, 0x11, 0)]
        else:
            dqt[1] = [int(x) for x in self.dqt[1]]
            hmax, vmax = SAMPLINGS[sampling]
            comps = [(1, (hmax << 4) | vmax, 0), (2, 0x11, 1), (3, 0x11, 1)]
        self.jpg = TM.build(w, h, comps, G["hv"], dqt, self.planes, restart_rows)


_cache = {}


def model(frame_bgr: np.ndarray, quality: int = 75, restart_rows: int = 0, sampling: str = "420") -> Model:
    """computed once per (frame, quality, restart_rows, sampling) and shared; callers leave it unchanged"""
    key = (frame_bgr.shape, frame_bgr.tobytes(), quality, restart_rows, sampling)
    m = _cache.get(key)
    if m is None:
        m = _cache[key] = Model(frame_bgr, quality, restart_rows, sampling)
    return m
