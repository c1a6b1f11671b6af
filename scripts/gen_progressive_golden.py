#!/usr/bin/env python3
"""Writes tests/golden/progressive/: small progressive JPEGs and manifest.json
(DESIGN.md §4p).  The p* files are Pillow's libjpeg-turbo saves
(progressive=True) of the pictures, qualities and samplings of their baseline
twins in tests/golden/foreign/; the m* files are written by
tests/progressive_model.py's encoder from a twin's coefficients under scan
scripts Pillow does not use.  For every file this asserts, before it stores
the digests:
 (a) Pillow decodes it to the pixels of its baseline twin,
 (b) progressive_model's pixels equal Pillow's,
 (c) progressive_model's coefficients equal foreign_model's for the twin on
     every block inside the components' own block grids.
Needs Pillow with libjpeg-turbo; runs on the CPU.

    python scripts/gen_progressive_golden.py
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
sys.path.insert(0, os.path.join(REPO, "scripts"))
import foreign_model as FM  # noqa: E402
import gen_foreign_golden as GF  # noqa: E402
import progressive_model as PM  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "progressive")
FOREIGN = os.path.join(REPO, "tests", "golden", "foreign")

# name: the baseline twin in tests/golden/foreign (same picture, quality, sampling, restart options)
PILLOW = {
    "p420_35x21": "420_35x21",
    "p422_35x21": "422_35x21",
    "p444_17x9": "444_17x9",
    "pgrey_35x21": "grey_35x21",
    "p420_1x1": "420_1x1",
    "p420_16x16": "420_16x16",
    "p420_70x37_rstrow": "420_70x37_rstrow",
    "p420_70x37_rst1": "420_70x37_rst1",
    "p420_96x80_noise_q95": "420_96x80_noise_q95",
    "p420_1040x520_q30": "420_1040x520_q30",
}
# name: (twin, scan script [(components, Ss, Se, Ri)], encoder options)
MODEL = {
    # DC of Y alone, DC of Cb and Cr in one Ns = 2 scan, two AC bands per component, a DRI that changes between scans
    "m420_35x21_split": ("420_35x21", [([0], 0, 0, 0), ([1, 2], 0, 0, 0), ([0], 1, 5, 2), ([0], 6, 63, 3),
                                       ([1], 1, 5, 0), ([1], 6, 63, 1), ([2], 1, 5, 4), ([2], 6, 63, 0)], {}),
    # three AC bands
    "m444_17x9_bands": ("444_17x9", [([0, 1, 2], 0, 0, 0)] +
                        [([c], a, b, 0) for c in range(3) for a, b in ((1, 5), (6, 20), (21, 63))], {}),
    # the first scan's DHT in front of SOF2, DC tables under Th 1, 2 and 3; a DRI in the scan's own MCUs
    "m422_35x21_dhtfirst": ("422_35x21", [([0, 1, 2], 0, 0, 2), ([0], 1, 63, 3), ([1], 1, 63, 0), ([2], 1, 63, 0)],
                            {"early_dht": True}),
}


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def twin_jpg(name: str) -> bytes:
    with open(os.path.join(FOREIGN, name + ".jpg"), "rb") as f:
        return f.read()


def pillow_rgb(jpg: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))


def main() -> None:
    assert features.check_feature("libjpeg_turbo"), "Pillow without libjpeg-turbo"
    os.makedirs(OUT, exist_ok=True)
    man = {"pillow": PIL.__version__, "libjpeg_turbo": features.version("jpg"), "files": {}}
    streams = {}
    for name, twin in PILLOW.items():
        mode, w, h, kind, opts = GF.CASES[twin]
        rgb = GF.content(kind, w, h)
        im = Image.fromarray(rgb).convert(mode) if mode == "L" else Image.fromarray(rgb)
        buf = io.BytesIO()
        im.save(buf, "JPEG", progressive=True, **opts)
        streams[name] = (buf.getvalue(), twin, "pillow", dict(opts, progressive=True))
    for name, (twin, script, opts) in MODEL.items():
        t = FM.decoded(twin_jpg(twin))
        dqt = {c[2]: t.dqt[i] for i, c in enumerate(t.G["comps"])}
        streams[name] = (PM.encode(dict(t.G, ri=0), t.coefs, dqt, script, **opts), twin, "model",
                         dict(opts, script=script))
    for name, (jpg, twin, writer, how) in streams.items():
        t = FM.decoded(twin_jpg(twin))
        m = PM.decoded(jpg)
        px = pillow_rgb(jpg)
        assert (px == pillow_rgb(twin_jpg(twin))).all(), (name, "(a) Pillow: progressive != baseline twin")
        assert (m.rgb == px).all(), (name, "(b) model pixels != Pillow")
        assert m.layout == [*t.layout[:7], 0, 1, *t.layout[9:]], (name, "layout")
        for c in range(m.G["ncomp"]):
            ins = PM.inside(m.G, c)
            assert (m.coefs[c][ins] == t.coefs[c][ins]).all(), (name, "(c) coefficients inside the grid", c)
            out = np.setdiff1d(np.arange(len(m.coefs[c])), ins)
            # (an interleaved DC scan walks whole MCUs, so padding blocks may hold a DC; AC bands never reach them)
            assert not m.coefs[c][out][:, 1:].any(), (name, "AC of padding blocks is zero", c)
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(jpg)
        man["files"][name] = {"sha256": sha(jpg), "bytes": len(jpg), "w": m.w, "h": m.h, "twin": twin, "writer": writer,
                              "how": how, "nscans": m.nscans, "levels": m.levels,
                              "script": [list(s) for s in m.script],
                              "rgb_sha256": sha(m.rgb.tobytes()),
                              "coef_sha256": sha(b"".join(c.tobytes() for c in m.coefs))}
        print(f"{name}: {len(jpg)} bytes, {m.nscans} scans, {m.levels} levels")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
