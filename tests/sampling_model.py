"""Plain numpy model of encoding at a chosen chroma sampling (DESIGN.md §4k,
include/mijpeg.h mij_encode_sampled): edge extension to whole MCUs, the
reference's colour expressions per pixel with uint8 truncation, 4:4:4 chroma
as it is, 4:2:2 chroma as the integer mean of a horizontal pair, no chroma
for greyscale; the reference's FP64 DCT, truncating quantisation, clip and
zigzag on every 8x8 block of every plane; the bytes of transcode_model.build.
4:2:0 is interleave_model's, unchanged.  Every FP64 operation is a separate
numpy ufunc call in the reference's order (numpy never contracts them).
Pinned to the oracle by tests/test_sampling_model.py; the kernels must give
these planes and bytes (tests/test_sampling_gpu.py)."""
import numpy as np

import decode_model as M
import interleave_model as IM
import oracle as O
import transcode_model as TM

SAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "gray": (1, 1)}  # Hmax, Vmax

SQRT1_2 = 0.70710678118654752440  # <math.h> M_SQRT1_2
_COS = None


def cos_table() -> np.ndarray:
    """encoder.c:8-16 as the oracle computes it: [t * 8 + f] = cos((2t + 1) f pi / 16)"""
    global _COS
    if _COS is None:
        _COS = np.frombuffer(O.cos_bits_cref().astype(np.int64).tobytes(), np.float64).copy()
    return _COS


def grid(w: int, h: int, sampling: str) -> dict:
    """the layout mij_batch_sampled_layout reports (foreign_model.geometry's keys, ri apart)"""
    hmax, vmax = SAMPLINGS[sampling]
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    hv = [(1, 1)] if sampling == "gray" else [(hmax, vmax), (1, 1), (1, 1)]
    return {"w": w, "h": h, "ncomp": len(hv), "hmax": hmax, "vmax": vmax, "mcus_x": mx, "mcus_y": my,
            "interleaved": 1, "hv": hv,
            "comps": [(a, b, 1 if c else 0, mx * a, my * b) for c, (a, b) in enumerate(hv)]}


def pad_mcu(frame: np.ndarray, sampling: str) -> np.ndarray:
    """last column, then last row, replicated up to whole MCUs"""
    hmax, vmax = SAMPLINGS[sampling]
    h, w = frame.shape[:2]
    return np.pad(frame, ((0, -h % (8 * vmax)), (0, -w % (8 * hmax)), (0, 0)), mode="edge")


def ycc(frame_bgr: np.ndarray):
    """encoder.c:133-135 per pixel: FP64, left to right, truncated to uint8"""
    b = frame_bgr[..., 0].astype(np.float64)
    g = frame_bgr[..., 1].astype(np.float64)
    r = frame_bgr[..., 2].astype(np.float64)
    y = np.add(np.add(np.multiply(0.299, r), np.multiply(0.587, g)), np.multiply(0.114, b))
    cb = np.add(np.subtract(np.subtract(128.0, np.multiply(0.168736, r)), np.multiply(0.331264, g)),
                np.multiply(0.5, b))
    cr = np.subtract(np.subtract(np.add(128.0, np.multiply(0.5, r)), np.multiply(0.418688, g)),
                     np.multiply(0.081312, b))
    return [v.astype(np.int64).astype(np.uint8) for v in (y, cb, cr)]


def samples(frame_bgr: np.ndarray, sampling: str):
    """the uint8 sample planes of the padded frame, one per component"""
    y, cb, cr = ycc(pad_mcu(np.ascontiguousarray(frame_bgr, np.uint8), sampling))
    if sampling == "gray":
        return [y]
    if sampling == "444":
        return [y, cb, cr]
    if sampling == "422":
        return [y] + [((c[:, 0::2].astype(np.int64) + c[:, 1::2]) // 2).astype(np.uint8) for c in (cb, cr)]
    raise ValueError(sampling)


def dct_quant(plane: np.ndarray, q_natural) -> np.ndarray:
    """encoder.c:81-112 on every 8x8 block of a uint8 plane: (blocks, 64)
    int64 in raster block order, zigzag inside, DC absolute"""
    cos = cos_table().reshape(8, 8)  # [t][f]
    h, w = plane.shape
    bh, bw = h // 8, w // 8
    p = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8).astype(np.float64) - 128.0  # [blk][y][x]
    col = np.zeros((p.shape[0], 8, 8))  # [blk][x][v]
    for y in range(8):  # summed from 0 in y order
        col = np.add(col, np.multiply(p[:, y, :, None], cos[y][None, None, :]))
    f = np.zeros((p.shape[0], 8, 8))  # [blk][v][u]
    for x in range(8):  # summed from 0 in x order
        f = np.add(f, np.multiply(col[:, x, :, None], cos[x][None, None, :]))
    f[:, :, 0] = np.multiply(f[:, :, 0], SQRT1_2)  # u == 0 first
    f[:, 0, :] = np.multiply(f[:, 0, :], SQRT1_2)
    f = np.divide(f, 4.0)
    t = np.divide(f.reshape(-1, 64), np.asarray(q_natural, np.float64)[None, :]).astype(np.int64)  # truncation
    t = np.clip(t, -2048, 2047)
    return t[:, M.ZZ]


def planes(frame_bgr: np.ndarray, quality: int, sampling: str):
    if sampling == "420":
        return IM.planes(frame_bgr, quality)
    lq, cq = O.quality_tables(quality)
    return [dct_quant(s, cq if c else lq) for c, s in enumerate(samples(frame_bgr, sampling))]


class Model:
    def __init__(self, frame_bgr: np.ndarray, quality: int, restart_rows: int, sampling: str):
        frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
        self.h, self.w = h, w = frame_bgr.shape[:2]
        self.sampling = sampling
        self.G = G = grid(w, h, sampling)
        self.planes = planes(frame_bgr, quality, sampling)
        self.layout = [w, h, G["ncomp"], G["hmax"], G["vmax"], G["mcus_x"], G["mcus_y"], restart_rows * G["mcus_x"], 1]
        for c in G["comps"]:
            self.layout += list(c)
        if sampling == "420":
            self.jpg = IM.model(frame_bgr, quality, restart_rows).jpg
            return
        lq, cq = O.quality_tables(quality)
        dqt = {0: [int(lq[z]) for z in M.ZZ]}
        if sampling == "gray":
            comps = [(1, 0x11, 0)]
        else:
            dqt[1] = [int(cq[z]) for z in M.ZZ]
            hmax, vmax = SAMPLINGS[sampling]
            comps = [(1, (hmax << 4) | vmax, 0), (2, 0x11, 1), (3, 0x11, 1)]
        self.jpg = TM.build(w, h, comps, G["hv"], dqt, self.planes, restart_rows)


_cache = {}


def model(frame_bgr: np.ndarray, quality: int = 50, restart_rows: int = 0, sampling: str = "444") -> Model:
    """computed once per (frame, quality, restart_rows, sampling) and shared; callers leave it unchanged"""
    key = (frame_bgr.shape, frame_bgr.tobytes(), quality, restart_rows, sampling)
    m = _cache.get(key)
    if m is None:
        m = _cache[key] = Model(frame_bgr, quality, restart_rows, sampling)
    return m
