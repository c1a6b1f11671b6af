"""The numpy statement of the pixels-to-tensor stage and of
the loader's rectangle rule: what csrc/mij_tensor.h builds its tables from and
k_tensorize looks up, said again without the library.

    t = float32(v) / float32(255);  t = t - float32(mean[c]);  t = t / float32(std[c])

float32 stores t, float16 t.astype(float16) (round to nearest even), bfloat16
t rounded to nearest even on its bit pattern (returned as uint16), uint8 v.
tests/test_tensor_model.py pins this to torch on the CPU."""
import numpy as np

DTYPES = ("uint8", "float16", "bfloat16", "float32")
LAYOUTS = ("nchw", "nhwc")
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
NP_DTYPE = {"uint8": np.uint8, "float16": np.float16, "bfloat16": np.uint16, "float32": np.float32}


def bf16_bits(t: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bit patterns, round to nearest even"""
    x = np.ascontiguousarray(t, np.float32).view(np.uint32).astype(np.uint64)
    nan = (x & 0x7FFFFFFF) > 0x7F800000
    r = (x + 0x7FFF + ((x >> 16) & 1)) >> 16
    return np.where(nan, (x >> 16) | 0x40, r).astype(np.uint16)


def values(v: np.ndarray, mean: float, std: float) -> np.ndarray:
    """float32 t of the bytes v for one channel"""
    t = v.astype(np.float32) / np.float32(255)
    t = t - np.float32(mean)
    with np.errstate(over="ignore"):
        t = t / np.float32(std)
    return t


def cast(t: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "float32":
        return t
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return t.astype(np.float16)
    assert dtype == "bfloat16"
    return bf16_bits(t)


def lut(dtype: str, mean=IMAGENET[0], std=IMAGENET[1]) -> np.ndarray:
    """(3, 256): the element tensor channel c gets for source byte v"""
    v = np.arange(256, dtype=np.uint8)
    if dtype == "uint8":
        return np.stack([v, v, v])
    return np.stack([cast(values(v, mean[c], std[c]), dtype) for c in range(3)])


def tensorize(frames, mirror=None, dtype="float16", layout="nchw", swap=False, mean=IMAGENET[0], std=IMAGENET[1]):
    """frames: n arrays (h, w, 3) uint8 of one size -> (n, 3, h, w) or (n, h, w, 3)"""
    table = lut(dtype, mean, std)
    out = []
    for i, f in enumerate(frames):
        if mirror is not None and mirror[i]:
            f = f[:, ::-1]
        if swap:
            f = f[..., ::-1]
        planes = np.stack([table[c][f[..., c]] for c in range(3)])  # (3, h, w)
        out.append(planes if layout == "nchw" else planes.transpose(1, 2, 0))
    return np.ascontiguousarray(np.stack(out))


def rect(crop, W: int, H: int, d: int):
    """the loader's rectangle (x0, y0, x1, y1) of the image decoded at 1/d for
    crop = (x, y, w, h) in full-size pixels of a W x H frame (None: all of it)"""
    x, y, w, h = crop if crop is not None else (0, 0, W, H)
    assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= W and y + h <= H
    return x // d, y // d, min(-(-W // d), -(-(x + w) // d)), min(-(-H // d), -(-(y + h) // d))


def denom(sizes, crops, out_w: int, out_h: int) -> int:
    """denom = 0: the smallest draft denominator (Pillow's rule: the largest
    of 8, 4, 2, 1 that is <= min(w // out_w, h // out_h)) over the frames' crops"""
    best = 8
    for i, (W, H) in enumerate(sizes):
        _, _, w, h = crops[i] if crops is not None else (0, 0, W, H)
        scale = min(w // out_w, h // out_h)
        best = min(best, next((d for d in (8, 4, 2) if d <= scale), 1))
    return best
