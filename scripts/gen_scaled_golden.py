#!/usr/bin/env python3
"""Writes tests/golden/scaled_pixels.json: per committed foreign fixture and
scale 1/2, 1/4, 1/8 the scaled size and the sha256 of the numpy model's RGB
pixels and of its padded planes (tests/scaled_model.py).  A pair on which
Pillow's libjpeg-turbo decodes at the requested scale and disagrees with the
model stops the run with nothing written, so the digests carry the libjpeg
equivalence to machines without Pillow; pairs on which Pillow picks another
scale (tiny images) are written from the model alone and listed.

    python scripts/gen_scaled_golden.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import foreign_cases as FC  # noqa: E402
import scaled_cases as SC  # noqa: E402


def main() -> int:
    Image = SC.pillow()
    if Image is None:
        print("Pillow with libjpeg-turbo is needed to write the digests", file=sys.stderr)
        return 1
    out, alone = {}, []
    for name in FC.NAMES:
        out[name] = {}
        for denom in SC.DENOMS:
            s = SC.model(name, denom)
            ref = SC.pillow_draft(Image, FC.jpg(name), denom)
            if ref is None:
                alone.append(f"{name} 1/{denom}")
            elif ref.shape != s.rgb.shape or (ref != s.rgb).any():
                print(f"{name} at 1/{denom}: libjpeg disagrees with the model: nothing written", file=sys.stderr)
                return 1
            out[name][str(denom)] = SC.digests(s)
    with open(SC.DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{SC.DIGESTS}: {len(out)} files x {len(SC.DENOMS)} scales; the model alone on: {', '.join(alone)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
