#!/usr/bin/env python3
"""Writes tests/golden/decode_pixels.json: per named case the sha256 of the
numpy model's RGB pixels and of its Y / Cb / Cr planes (tests/decode_model.py
on the oracle's coefficients).  A case is written only if Pillow's
libjpeg-turbo decodes the same stream to the same RGB and the same Y, byte
for byte; so the digests carry the libjpeg equivalence to machines without
Pillow.  Needs the oracle built (make -C oracle)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(REPO, p))

import decode_cases as DC  # noqa: E402


def main() -> int:
    out = {}
    for name in DC.LIBJPEG_CASES:
        c = DC.case(name)
        ref = DC.libjpeg_pixels(c.jpg)
        if ref is None:
            print("Pillow with libjpeg-turbo is needed to write the digests", file=sys.stderr)
            return 1
        rgb, y = ref
        if not ((rgb == c.rgb).all() and (y == c.planes[0]).all()):
            print(f"{name}: libjpeg disagrees with the model ({int((rgb != c.rgb).sum())} RGB bytes, "
                  f"{int((y != c.planes[0]).sum())} Y samples): nothing written", file=sys.stderr)
            return 1
        out[name] = c.digests()
    with open(DC.DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{DC.DIGESTS}: {len(out)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
