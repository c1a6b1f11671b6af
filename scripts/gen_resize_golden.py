#!/usr/bin/env python3
"""Writes tests/golden/resize/manifest.json with Pillow: per case of
tests/resize_cases.py the sha256 of PIL.Image.resize's pixels, and the tables
the host-only helpers are pinned to: Image.draft's scale per (file size,
requested size) and Image.thumbnail's size per (image size, box).  A case on
which the numpy model (tests/resize_model.py) disagrees with Pillow stops the
run with nothing written, so the digests carry the Pillow equivalence to
machines without Pillow.

    python scripts/gen_resize_golden.py
"""
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import resize_cases as RC  # noqa: E402

# (file w, file h, requested w, requested h) for Image.draft
DRAFT = [(240, 135, 120, 67), (240, 135, 120, 68), (240, 135, 60, 33), (240, 135, 31, 17), (240, 135, 30, 16),
         (240, 135, 7, 100), (240, 135, 240, 135), (240, 135, 500, 500), (240, 135, 1, 1), (3840, 2160, 256, 144),
         (3840, 2160, 481, 270), (3840, 2160, 480, 271), (96, 80, 20, 17), (96, 80, 48, 40), (96, 80, 49, 40),
         (17, 9, 2, 1), (16, 16, 2, 2), (16, 16, 3, 2), (1, 1, 1, 1)]
# (image w, image h, box w, box h) for Image.thumbnail
FIT = [(240, 135, 128, 128), (240, 135, 100, 10), (240, 135, 10, 100), (135, 240, 128, 128), (3840, 2160, 256, 256),
       (3840, 2160, 256, 144), (3840, 2160, 255, 144), (100, 100, 33, 77), (1000, 3, 100, 100), (3, 1000, 100, 100),
       (640, 480, 640, 480), (640, 480, 1000, 1000), (640, 480, 1000, 100), (640, 480, 639, 480), (5, 3, 4, 4),
       (7, 5, 3, 3), (997, 13, 500, 500), (13, 997, 500, 500), (4000, 3000, 1, 1), (2, 3, 1, 2), (3, 2, 2, 1),
       (1920, 1080, 300, 169), (1920, 1080, 301, 169), (65535, 1, 100, 100), (101, 99, 50, 50), (99, 101, 50, 50)]


def main() -> int:
    Image = RC.pillow()
    if Image is None:
        print("Pillow is needed to write the digests", file=sys.stderr)
        return 1
    cases = {}
    for case in RC.CASES:
        (w, h, ow, oh), f = case
        ref = RC.pillow_resize(Image, RC.frame(w, h), (ow, oh), f)
        got = RC.model(case)
        if ref.shape != got.shape or (ref != got).any():
            print(f"{RC.case_id(case)}: Pillow disagrees with the model: nothing written", file=sys.stderr)
            return 1
        cases[RC.case_id(case)] = RC.digest(ref)
    draft = []
    for w, h, ow, oh in DRAFT:
        buf = io.BytesIO()
        Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(buf, "JPEG")
        im = Image.open(io.BytesIO(buf.getvalue()))
        im.draft("RGB", (ow, oh))
        draft.append([w, h, ow, oh, im.decoderconfig[0] if im.decoderconfig else 1])
    fit = []
    for w, h, bw, bh in FIT:
        im = Image.new("RGB", (w, h))
        im.thumbnail((bw, bh))
        fit.append([w, h, bw, bh, *im.size])
    import PIL
    out = {"pillow": PIL.__version__, "cases": cases, "draft": draft, "fit": fit}
    os.makedirs(RC.GOLDEN, exist_ok=True)
    path = os.path.join(RC.GOLDEN, "manifest.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(cases)} cases, {len(draft)} draft rows, {len(fit)} fit rows")
    return 0


if __name__ == "__main__":
    sys.exit(main())
