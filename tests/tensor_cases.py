"""Shared by the GPU tests of the pixels-to-tensor stage:
plain device memory for sources and a caller's destination, the kernel's tile
constants read from its header, and seeded frames."""
import os
import re

import numpy as np

import mijpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "jpeg-encoder-decoder_amd", "csrc", "mij_tensor.h")) as _f:
    _H = _f.read()
TZ_SEG = int(re.search(r"constexpr int TZ_SEG = (\d+);", _H).group(1))    # pixels of a workgroup's row segment
TZ_ROWS = int(re.search(r"constexpr int TZ_ROWS = (\d+);", _H).group(1))  # rows of its tile

FILL = 0xA5


def frame(w: int, h: int, seed: int) -> np.ndarray:
    """(h, w, 3) bytes, every value likely, both extremes certain"""
    px = np.random.default_rng(1000 * w + 10 * h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    px.reshape(-1)[0] = 0
    px.reshape(-1)[-1] = 255
    return px


class Arena:
    """Device memory holding a copy of `host` (a detector's frame buffer serves
    as plain device memory: no second HIP runtime in the process), readable
    back through the resizer's copy of an image whose sizes stay as they are."""

    def __init__(self, host: np.ndarray):
        pitch = 4096
        rows = max((-(-(host.size + 64) // pitch) + 3) & ~3, 16)
        buf = np.full((rows, pitch), FILL, np.uint8)
        buf.reshape(-1)[:host.size] = host
        self.size = host.size
        self.det = mijpeg.Detector(16, rows)
        self.ptr = self.det.upload(buf, pitch)
        self.rs = mijpeg.Resizer(1)
        assert self.ptr % 16 == 0

    def read(self, off: int, nbytes: int) -> np.ndarray:
        assert off + nbytes <= self.size
        w = -(-nbytes // 3)
        self.rs.resize([(self.ptr + off, 3 * w, w, 1)], [(w, 1)], "box")
        return self.rs.pixels(0).reshape(-1)[:nbytes]

    def close(self) -> None:
        self.rs.close()
        self.det.close()


def place(frames, offsets=(0, 1, 3), extra=(0, 5, 16), dst_bytes=0):
    """the frames in one arena, frame i at a byte address that is offsets[i]
    past a multiple of 16, its rows 3 * w + extra[i] bytes apart, the bytes
    between holding FILL; behind them a 16-aligned region of dst_bytes + 64
    bytes of FILL for a caller's tensor: (arena, [(address, pitch, w, h)],
    the region's offset)"""
    at, where = 0, []
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        pitch = 3 * w + extra[i % len(extra)]
        at = (at + 15) // 16 * 16 + offsets[i % len(offsets)]
        where.append((at, pitch, w, h))
        at += pitch * h
    dst = (at + 64 + 15) // 16 * 16
    host = np.full(dst + dst_bytes + 64, FILL, np.uint8)
    for f, (o, pitch, w, h) in zip(frames, where):
        for y in range(h):
            host[o + y * pitch:o + y * pitch + 3 * w] = f[y].reshape(-1)
    arena = Arena(host)
    return arena, [(arena.ptr + o, pitch, w, h) for o, pitch, w, h in where], dst
