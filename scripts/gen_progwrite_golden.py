#!/usr/bin/env python3
"""Writes tests/golden/progressive_write/: the two progressive files that
reach the limits of libjpeg's EOB runs, saved by Pillow.

 corr_limit  greyscale 256x64, every block 128 plus twenty DCT basis
             functions of amplitude +-32 with random signs, all quantisers 8:
             in both AC refinement scans every block carries 20 correction
             bits and no new coefficient, so a run is cut when its buffered
             bits pass 937
 run_limit   flat greyscale 2048x1032 (33 024 blocks): every AC scan is one
             end-of-band run, cut at 0x7FFF blocks

This asserts both conditions from tests/progwrite_model.py's tokens, and that
the tokens, coded with the tables of the file, are the file's entropy data.
Needs Pillow; runs on the CPU.

    python scripts/gen_progwrite_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import progressive_model as PM  # noqa: E402
import progwrite_model as W  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "progressive_write")
# the twenty basis functions (u, v): the first of the zigzag order after DC
ZZ20 = [(1, 0), (0, 1), (0, 2), (1, 1), (2, 0), (3, 0), (2, 1), (1, 2), (0, 3), (0, 4), (1, 3), (2, 2), (3, 1), (4, 0),
        (5, 0), (4, 1), (3, 2), (2, 3), (1, 4), (0, 5)]


def corr_limit() -> bytes:
    rng = np.random.default_rng(937)
    x = (2 * np.arange(8) + 1) * np.pi / 16
    img = np.zeros((64, 256))
    for by in range(8):
        for bx in range(32):
            blk = np.full((8, 8), 128.0)
            for u, v in ZZ20:
                blk += 32 * rng.choice((-1, 1)) * np.outer(np.cos(v * x), np.cos(u * x)) / 4
            img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = blk
    buf = io.BytesIO()
    Image.fromarray(np.clip(np.rint(img), 0, 255).astype(np.uint8), "L").save(buf, "JPEG", progressive=True,
                                                                             qtables=[[8] * 64])
    return buf.getvalue()


def run_limit() -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.full((1032, 2048), 100, np.uint8), "L").save(buf, "JPEG", quality=75, progressive=True)
    return buf.getvalue()


def scan_runs(jpg: bytes):
    """per AC scan the model's EOB runs, after pinning the model's tokens to the file's bytes"""
    P, D = PM.parse(jpg), PM.decoded(jpg)
    out = []
    for sc in P["scans"]:
        args = (D.G, D.coefs, tuple(sc["comps"]), sc["ss"], sc["se"], sc["ah"], sc["al"], sc["ri"])
        codes = [W.huff_codes(t) for t in sc["td"] if t] if sc["ss"] == 0 else [W.huff_codes(sc["ta"])]
        assert [W.entropy(t, codes) for t in W.tokens(*args)] == sc["parts"]
        if sc["ss"]:
            out.append((sc["ah"], W.runs(*args)))
    return out


def main() -> None:
    os.makedirs(OUT, exist_ok=True)
    c = corr_limit()
    refine = [r for ah, r in scan_runs(c) if ah]
    assert len(refine) == 2
    for r in refine:
        assert max(be for _, be in r) > W.MAX_BE and len(r) > 1, r  # the BE > 937 rule fired
        assert all(be == 20 * n for n, be in r), r                    # 20 correction bits per block, no new coefficient
    print("corr_limit", len(c), "bytes; runs of a refinement scan:", refine[0])
    f = run_limit()
    for ah, r in scan_runs(f):
        assert [n for n, _ in r] == [W.MAX_EOBRUN, 33024 - W.MAX_EOBRUN], r  # cut at 0x7FFF blocks
    print("run_limit", len(f), "bytes")
    for name, data in (("corr_limit", c), ("run_limit", f)):
        with open(os.path.join(OUT, name + ".jpg"), "wb") as fh:
            fh.write(data)


if __name__ == "__main__":
    main()
