"""Frames shared by tests/test_sampling_model.py (CPU) and
tests/test_sampling_gpu.py: built once, left unchanged."""
import os

import numpy as np

import interleave_model as IM
import recipes

_cache = {}


def _once(key, make):
    v = _cache.get(key)
    if v is None:
        v = _cache[key] = make()
    return v


def exception_frame() -> np.ndarray:
    """64x48 B, G, R frame of flat 8x8 patches: eight colours from each of the
    three sets of tests/golden/colour_exceptions.npz (colours whose exact Y, Cb
    or Cr is an integer that the reference's FP64 expression lands one below),
    each followed by a neighbour one step away in one channel"""
    def make():
        ex = np.load(os.path.join(recipes.GOLDEN, "colour_exceptions.npz"))
        cols = []
        for key in ("Y", "Cb", "Cr"):
            t = ex[key].astype(np.int64)
            for i, (r, g, b) in enumerate(t[::max(1, len(t) // 8)][:8]):
                cols.append((r, g, b))
                n = [r, g, b]
                n[i % 3] = n[i % 3] + 1 if n[i % 3] < 255 else n[i % 3] - 1
                cols.append(tuple(n))
        assert len(cols) == 48
        f = np.zeros((48, 64, 3), np.uint8)
        for i, (r, g, b) in enumerate(cols):
            y, x = divmod(i, 8)
            f[8 * y:8 * y + 8, 8 * x:8 * x + 8] = (b, g, r)
        return f
    return _once("exception", make)


def exact_floor_ycc(frame_bgr: np.ndarray):
    """floor of the exact rational Y, Cb, Cr of every pixel (tests/test_oracle.py's integers)"""
    b, g, r = (frame_bgr[..., c].astype(np.int64) for c in range(3))
    return [(299 * r + 587 * g + 114 * b) // 1000,
            (128_000_000 - 168736 * r - 331264 * g + 500000 * b) // 1_000_000,
            (128_000_000 + 500000 * r - 418688 * g - 81312 * b) // 1_000_000]


def _idct_block(F):
    """pixels of natural-order DCT coefficients F[v * 8 + u] (the inverse of encoder.c:81-112), clamped"""
    t = np.arange(8)
    basis = np.cos((2 * t[:, None] + 1) * t[None, :] * np.pi / 16)  # [t][f]
    c = np.where(t == 0, np.sqrt(0.5), 1.0)
    G = F.reshape(8, 8) * c[:, None] * c[None, :]
    px = 128 + (basis @ G.T @ basis.T).T / 4  # [y][x] = sum_vu G[v][u] basis[x][u] basis[y][v] / 4
    return np.clip(px, 0, 255).astype(np.uint8)


def boundary_frame(seed: int = 5) -> np.ndarray:
    """64x32 grey frame whose 8x8 blocks are inverse DCTs of a few coefficients
    at integer multiples of a quantiser (+- 1/128), as tests/tau_check.c's
    gen_block synthesises them: the forward DCT lands on or beside truncation
    boundaries"""
    def make():
        rng = np.random.default_rng(seed)
        f = np.zeros((32, 64, 3), np.uint8)
        for by in range(4):
            for bx in range(8):
                F = np.zeros(64)
                q = 1 + int(rng.integers(0, 40))
                F[0] = float(rng.integers(0, 512)) - 256
                for _ in range(1 + int(rng.integers(0, 4))):
                    F[1 + int(rng.integers(0, 63))] = q * (float(rng.integers(0, 21)) - 10) + \
                        (float(rng.integers(0, 3)) - 1) * 0.5 / 64
                f[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = _idct_block(F)[:, :, None]
        return f
    return _once(("boundary", seed), make)


def grey_levels() -> np.ndarray:
    """256x64: flat 8x8 patches of the greys 0..255, 32 across and 8 down"""
    def make():
        f = np.zeros((64, 256, 3), np.uint8)
        for v in range(256):
            y, x = divmod(v, 32)
            f[8 * y:8 * y + 8, 8 * x:8 * x + 8] = v
        return f
    return _once("greys", make)


def checker_frame() -> np.ndarray:
    """48x32: checkerboards of period 1, 2 and 4 in 0/255 and in two colours, and 0/255 random pixels"""
    def make():
        y, x = np.mgrid[0:32, 0:48]
        f = np.zeros((32, 48, 3), np.uint8)
        for i, p in enumerate((1, 2, 4)):
            f[:16, 16 * i:16 * i + 16] = (((x[:16, :16] // p + y[:16, :16] // p) & 1) * 255)[:, :, None]
        two = np.array([[12, 200, 90], [240, 31, 180]], np.uint8)
        f[16:, :16] = two[(x[16:, :16] + y[16:, :16]) & 1]
        f[16:, 16:] = np.random.default_rng(9).integers(0, 2, (16, 32, 3), dtype=np.uint8) * 255
        return f
    return _once("checker", make)


def photo(w: int, h: int, seed: int = 0) -> np.ndarray:
    return _once(("photo", w, h, seed), lambda: IM.frame(w, h, seed=seed))


def noise(w: int, h: int, seed: int = 0) -> np.ndarray:
    return _once(("noise", w, h, seed), lambda: IM.frame(w, h, seed=seed, kind="noise"))
