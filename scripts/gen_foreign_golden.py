#!/usr/bin/env python3
"""Writes tests/golden/foreign/: small baseline JPEGs as Pillow's libjpeg-turbo
writes them (interleaved scan, standard or optimised tables, any size,
restart intervals) and manifest.json with, per file, its sha256, the Pillow
save options, and the sha256 of the RGB pixels and of the Y channel Pillow
decodes from it.  Needs Pillow with libjpeg-turbo; runs on the CPU.

    python scripts/gen_foreign_golden.py
"""
import hashlib
import io
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import recipes  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "foreign")


def content(kind: str, w: int, h: int) -> np.ndarray:
    if kind == "noise":
        return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 255 // (w + h - 2)], -1).astype(np.uint8)
    # "mixed": gradients with a noisy band, cropped: edges, colour and some long blocks
    hh, ww = max(16, -(-h // 16) * 16), max(16, -(-w // 16) * 16)
    a = recipes.gradients(hh, ww).astype(np.int64)
    n = recipes.noise(hh, ww, seed=w + h).astype(np.int64)
    a[hh // 3:hh // 2] = (a[hh // 3:hh // 2] + n[hh // 3:hh // 2]) // 2
    a[:, ww // 2:ww // 2 + 3] = 255 - a[:, ww // 2:ww // 2 + 3]
    return a[:h, :w].astype(np.uint8)


# name: (mode, w, h, content, Pillow save options)
CASES = {
    "grey_8x8": ("L", 8, 8, "mixed", {"quality": 75}),
    "grey_35x21": ("L", 35, 21, "mixed", {"quality": 75}),
    "444_40x24": ("RGB", 40, 24, "mixed", {"quality": 75, "subsampling": 0}),
    "444_17x9": ("RGB", 17, 9, "mixed", {"quality": 75, "subsampling": 0}),
    "420_1x1": ("RGB", 1, 1, "mixed", {"quality": 75, "subsampling": 2}),
    "420_16x16": ("RGB", 16, 16, "mixed", {"quality": 75, "subsampling": 2}),
    "420_35x21": ("RGB", 35, 21, "mixed", {"quality": 75, "subsampling": 2}),
    "420_33x17_opt": ("RGB", 33, 17, "mixed", {"quality": 75, "subsampling": 2, "optimize": True}),
    "420_4x4": ("RGB", 4, 4, "noise", {"quality": 90, "subsampling": 2}),
    "420_5x5": ("RGB", 5, 5, "noise", {"quality": 90, "subsampling": 2}),
    "422_3x8": ("RGB", 3, 8, "noise", {"quality": 90, "subsampling": 1}),
    "422_4x8": ("RGB", 4, 8, "noise", {"quality": 90, "subsampling": 1}),
    "422_5x8": ("RGB", 5, 8, "noise", {"quality": 90, "subsampling": 1}),
    "422_35x21": ("RGB", 35, 21, "mixed", {"quality": 75, "subsampling": 1}),
    "420_70x37_rst1": ("RGB", 70, 37, "mixed", {"quality": 75, "subsampling": 2, "restart_marker_blocks": 1}),
    "420_70x37_rstrow": ("RGB", 70, 37, "mixed", {"quality": 75, "subsampling": 2, "restart_marker_rows": 1}),
    "444_24x24_noise_q100": ("RGB", 24, 24, "noise", {"quality": 100, "subsampling": 0}),
    "420_96x80_noise_q95": ("RGB", 96, 80, "noise", {"quality": 95, "subsampling": 2}),
    "420_1040x520_q30": ("RGB", 1040, 520, "smooth", {"quality": 30, "subsampling": 2}),
    "420_1040x520_q30_rst4": ("RGB", 1040, 520, "smooth", {"quality": 30, "subsampling": 2, "restart_marker_rows": 4}),
}


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def main() -> None:
    assert features.check_feature("libjpeg_turbo"), "Pillow without libjpeg-turbo"
    os.makedirs(OUT, exist_ok=True)
    man = {"pillow": PIL.__version__, "libjpeg_turbo": features.version("jpg"), "files": {}}
    for name, (mode, w, h, kind, opts) in CASES.items():
        rgb = content(kind, w, h)
        im = Image.fromarray(rgb).convert(mode) if mode == "L" else Image.fromarray(rgb)
        buf = io.BytesIO()
        im.save(buf, "JPEG", **opts)
        jpg = buf.getvalue()
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(jpg)
        dec = Image.open(io.BytesIO(jpg))
        px = np.asarray(dec.convert("RGB"))
        yim = Image.open(io.BytesIO(jpg))
        if mode != "L":
            yim.draft("YCbCr", (w, h))
        y = np.asarray(yim)[..., 0] if mode != "L" else np.asarray(yim)
        man["files"][name] = {"sha256": sha(jpg), "bytes": len(jpg), "w": w, "h": h, "mode": mode, "content": kind,
                              "save": opts, "rgb_sha256": sha(px.tobytes()),
                              "y_sha256": sha(np.ascontiguousarray(y).tobytes())}
        print(f"{name}: {len(jpg)} bytes")
    # streams the decoder must refuse (whole files; the byte-edited ones are made by tests/foreign_cases.py)
    man["rejects"] = {}
    for name, mode, opts in (("reject_progressive", "RGB", {"quality": 75, "progressive": True}),
                             ("reject_cmyk", "CMYK", {"quality": 75})):
        buf = io.BytesIO()
        Image.fromarray(content("mixed", 16, 16)).convert(mode).save(buf, "JPEG", **opts)
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(buf.getvalue())
        man["rejects"][name] = {"sha256": sha(buf.getvalue()), "bytes": len(buf.getvalue()), "save": opts}
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
