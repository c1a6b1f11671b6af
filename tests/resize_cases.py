"""Inputs and cases of the resampler tests: closed-form integer
patterns, no RNG, identical everywhere; the size pairs the model was checked
against Pillow on; the committed digests and tables."""
import functools
import hashlib
import json
import os

import numpy as np

import resize_model as RM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize")
FILTERS = RM.FILTERS

# (in_w, in_h, out_w, out_h)
PAIRS = [(37, 29, 16, 16), (37, 29, 37, 10), (37, 29, 80, 29), (1, 1, 5, 7), (5, 3, 1, 1), (240, 135, 17, 9),
         (64, 48, 100, 75), (33, 70, 32, 69), (480, 270, 7, 3), (2, 2, 3, 3), (96, 80, 24, 20)]
CASES = [(p, f) for p in PAIRS for f in FILTERS]


def case_id(case):
    (w, h, ow, oh), f = case
    return f"{w}x{h}-{ow}x{oh}-{f}"


@functools.lru_cache(maxsize=None)
def frame(w, h):
    """[h, w, 3] uint8: three gradients that wrap at different rates, and in
    the rectangle from (w/4, h/4) to (3w/4, 3h/4) a hard 0 / 255 checkerboard
    of 3 x 2 pixel cells, so that BICUBIC's negative lobes reach both clips"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    px = np.stack([(7 * x + 3 * y) % 256, (5 * x * y + 11 * y + 40) % 256, (x * x + 13 * y + 2 * x) % 251], -1)
    hard = (x >= w // 4) & (x < w - w // 4) & (y >= h // 4) & (y < h - h // 4)
    check = ((x // 3 + y // 2) % 2) * 255
    px[hard] = np.stack([check, 255 - check, check], -1)[hard]
    return np.ascontiguousarray(px.astype(np.uint8))


@functools.lru_cache(maxsize=None)
def model(case):
    (w, h, ow, oh), f = case
    out = RM.resize(frame(w, h), (ow, oh), f)
    out.setflags(write=False)
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def pillow():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def pillow_resize(Image, px, size, f):
    return np.asarray(Image.fromarray(px).resize(size, getattr(Image.Resampling, f.upper())))
