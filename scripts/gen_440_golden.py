#!/usr/bin/env python3
"""Writes tests/golden/s440/: the 4:4:0 fixtures, their
manifest.json, pixels.json, the digests of the numpy model's pixels and planes
at scales 1, 2, 4 and 8 (tests/s440_model.py), and jpegtran_planes.json,
the digests of jpegtran's own coefficient planes of the two 4:2:2 sources
under the four transposing operations with and without -trim.

A 4:4:0 file is what a lossless quarter turn makes of a 4:2:2 one, so every
fixture is a 4:2:2 file written by Pillow's libjpeg-turbo and then turned by
jpegtran (any libjpeg flavour: the coefficient-domain result does not depend
on it); the progressive ones are jpegtran -progressive of two of those.  A
(file, scale) pair on which Pillow decodes at the requested scale and
disagrees with the model stops the run with nothing written, so the digests
carry the libjpeg equivalence to machines without Pillow.  Needs Pillow and
jpegtran; it is run where both are at hand, never as part of a test.

    python scripts/gen_440_golden.py [path to jpegtran]
"""
import hashlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

import gen_foreign_golden as GF  # noqa: E402
import s440_cases as SC  # noqa: E402
import s440_model as SM  # noqa: E402
import scaled_cases  # noqa: E402

# name: (source w, h, content, Pillow save options, jpegtran switches)
CASES = {
    "440_21x35": (35, 21, "mixed", {"quality": 75}, ["-transpose"]),
    "440_8x5": (5, 8, "noise", {"quality": 90}, ["-transpose"]),
    "440_8x3": (3, 8, "noise", {"quality": 90}, ["-transpose"]),
    "440_8x2": (2, 8, "noise", {"quality": 90}, ["-transpose"]),
    "440_8x1": (1, 8, "noise", {"quality": 90}, ["-transpose"]),
    "440_1x1": (1, 1, "mixed", {"quality": 75}, ["-transpose"]),
    "440_2x16": (16, 2, "mixed", {"quality": 75}, ["-transpose"]),
    "440_37x70_rstrow": (70, 37, "mixed", {"quality": 75}, ["-transpose", "-restart", "1"]),
    "440_37x70_rst1": (70, 37, "mixed", {"quality": 75}, ["-transpose", "-restart", "1B"]),
    "440_40x48_noise_q95": (48, 40, "noise", {"quality": 95}, ["-transpose"]),
    "440_520x1040_q30": (1040, 520, "smooth", {"quality": 30}, ["-transpose"]),
}
PROGRESSIVE = {"p440_21x35": "440_21x35", "p440_37x70_rstrow": "440_37x70_rstrow"}
SOURCES = {"422_48x32": (48, 32, "mixed", {"quality": 75})}  # 422_35x21 is tests/golden/foreign's


def sha(b) -> str:
    return hashlib.sha256(bytes(b)).hexdigest()


def pillow_422(Image, w, h, kind, opts) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(GF.content(kind, w, h)).save(buf, "JPEG", subsampling=1, **opts)
    return buf.getvalue()


def jpegtran(exe, switches, jpg: bytes) -> bytes:
    with tempfile.TemporaryDirectory() as t:
        src, dst = os.path.join(t, "a.jpg"), os.path.join(t, "b.jpg")
        with open(src, "wb") as f:
            f.write(jpg)
        subprocess.check_call([exe, *switches, "-outfile", dst, src])
        with open(dst, "rb") as f:
            return f.read()


def main() -> int:
    Image = scaled_cases.pillow()
    exe = sys.argv[1] if len(sys.argv) > 1 else shutil.which("jpegtran")
    if Image is None or not exe:
        print("Pillow with libjpeg-turbo and a jpegtran are needed", file=sys.stderr)
        return 1
    files, man = {}, {"files": {}, "sources": {}}
    for name, (w, h, kind, opts, sw) in CASES.items():
        files[name] = jpegtran(exe, sw, pillow_422(Image, w, h, kind, opts))
        man["files"][name] = {"source": {"w": w, "h": h, "content": kind, "save": dict(opts, subsampling=1)},
                              "jpegtran": sw}
    for name, base in PROGRESSIVE.items():
        files[name] = jpegtran(exe, ["-progressive"], files[base])
        man["files"][name] = {"of": base, "jpegtran": ["-progressive"]}
    digests, alone = {}, []
    for name, jpg in files.items():
        m = SM.decoded(jpg)
        if m.layout[3:5] != [1, 2]:
            print(f"{name}: not 4:4:0", file=sys.stderr)
            return 1
        man["files"][name].update(w=m.w, h=m.h, bytes=len(jpg), sha256=sha(jpg))
        digests[name] = {}
        for denom in SM.DENOMS:
            s = SM.scaled(jpg, denom)
            ref = scaled_cases.pillow_draft(Image, jpg, denom)
            if ref is None:
                alone.append(f"{name} 1/{denom}")
            elif ref.shape != s.rgb.shape or (ref != s.rgb).any():
                print(f"{name} at 1/{denom}: libjpeg disagrees with the model: nothing written", file=sys.stderr)
                return 1
            digests[name][str(denom)] = SC.digests(s)
    os.makedirs(SC.DIR, exist_ok=True)
    for name, jpg in files.items():
        with open(os.path.join(SC.DIR, name + ".jpg"), "wb") as f:
            f.write(jpg)
    for name, (w, h, kind, opts) in SOURCES.items():
        jpg = pillow_422(Image, w, h, kind, opts)
        with open(os.path.join(SC.DIR, name + ".jpg"), "wb") as f:
            f.write(jpg)
        man["sources"][name] = {"w": w, "h": h, "content": kind, "save": dict(opts, subsampling=1),
                                "bytes": len(jpg), "sha256": sha(jpg)}
    man["model_alone"] = alone
    # jpegtran's own transposed planes of the 4:2:2 sources, for every case the transform keeps
    import transform_model as XM
    turned = {}
    for name in SC.SOURCES:
        src = SC.jpg(name)
        for op, sw in SC.TRANSPOSING.items():
            for trim in (False, True):
                try:
                    SM.parts(src, op, trim)
                except XM.Refused:  # jpegtran then leaves the partial edge untransformed: nothing to pin
                    continue
                out = jpegtran(exe, sw + (["-trim"] if trim else []), src)
                turned[f"{name} {op}" + (" trim" if trim else "")] = SC.record_of_file(out)
    for path, obj in ((os.path.join(SC.DIR, "manifest.json"), man), (SC.DIGESTS, digests),
                      (SC.JPEGTRAN_PLANES, turned)):
        with open(path, "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)
            f.write("\n")
    print(f"{SC.DIR}: {len(files)} files x {len(SM.DENOMS)} scales; the model alone on {len(alone)} pairs: "
          f"{', '.join(alone)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
