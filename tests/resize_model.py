"""Numpy model of Pillow's 8-bit Image.resize (src/libImaging/Resample.c) for
BOX, BILINEAR and BICUBIC, without `box` and `reducing_gap`.

Coefficients in Python floats (IEEE doubles, one operation at a time, Pillow's
order), weights as 22-bit fixed point, every pass an int32 sum from 1 << 21,
arithmetic shift, clip.  Horizontal first, to an 8-bit intermediate; a pass
whose sizes are equal is skipped.  tests/test_resize_model.py pins it to
Pillow and to the committed digests."""
import functools
import math

import numpy as np

FILTERS = ("box", "bilinear", "bicubic")
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0}
BITS = 22


def _filter(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize(n_in, n_out, name):
    return int(math.ceil(SUPPORT[name] * max(n_in / n_out, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=None)
def axis_table(n_in, n_out, name):
    """(bounds [n_out, 2] = xmin, count; weights [n_out, ksize] int32)"""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = SUPPORT[name] * filterscale
    ss = 1.0 / filterscale
    ks = ksize(n_in, n_out, name)
    bounds = np.zeros((n_out, 2), np.int32)
    weights = np.zeros((n_out, ks), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = [_filter(name, (x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        bounds[xx] = xmin, xmax
        weights[xx, :xmax] = [int(-0.5 + w * (1 << BITS)) if w < 0 else int(0.5 + w * (1 << BITS)) for w in k]
    return bounds, weights


def _pass(a, n_out, name):
    """resample axis 0 of a uint8 array"""
    bounds, weights = axis_table(a.shape[0], n_out, name)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    src = a.astype(np.int64)
    for i, (xmin, n) in enumerate(bounds):
        acc = np.tensordot(weights[i, :n].astype(np.int64), src[xmin:xmin + n], 1) + (1 << (BITS - 1))
        assert np.abs(acc).max() < 2 ** 31  # the kernels' int32
        out[i] = np.clip(acc >> BITS, 0, 255)
    return out


def resize(px, size, name):
    """px [h, w, 3] uint8 -> [size[1], size[0], 3], as PIL.Image.resize(size, FILTER)"""
    ow, oh = size
    h, w = px.shape[:2]
    out = np.ascontiguousarray(px)
    if ow != w:
        out = _pass(out.transpose(1, 0, 2), ow, name).transpose(1, 0, 2)
    if oh != h:
        out = _pass(out, oh, name)
    return np.ascontiguousarray(out)

