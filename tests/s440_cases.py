"""What the 4:4:0 tests share: the committed fixtures of
tests/golden/s440/ (written by scripts/gen_440_golden.py with Pillow and
jpegtran), their model decodes at every scale, the committed digests of
those, and jpegtran where one is installed."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

import foreign_cases as FC
import recipes
import s440_model as SM

DIR = os.path.join(recipes.GOLDEN, "s440")
DIGESTS = os.path.join(DIR, "pixels.json")
DENOMS = SM.DENOMS

BASELINE = ["440_21x35", "440_8x5", "440_8x3", "440_8x2", "440_8x1", "440_1x1", "440_2x16", "440_37x70_rstrow",
            "440_37x70_rst1", "440_40x48_noise_q95", "440_520x1040_q30"]
PROGRESSIVE = {"p440_21x35": "440_21x35", "p440_37x70_rstrow": "440_37x70_rstrow"}  # name: its baseline twin
NAMES = BASELINE + sorted(PROGRESSIVE)
SOURCES = ["422_48x32", "422_35x21"]  # 4:2:2, for the transforms; the latter is a foreign fixture


def jpg(name: str) -> bytes:
    if name == "422_35x21":
        return FC.jpg(name)
    with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
        return f.read()


def model(name: str) -> SM.Decoded:
    return SM.decoded(jpg(name))


def scaled(name: str, denom: int) -> SM.Scaled:
    return SM.scaled(jpg(name), denom)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(s) -> dict:
    return {"size": [s.ow, s.oh], "rgb": sha(s.rgb), "planes": [sha(p) for p in s.planes]}


def committed_digests() -> dict:
    with open(DIGESTS) as f:
        return json.load(f)


def jpegtran_exe():
    """$JPEGTRAN, or a jpegtran on the PATH or beside the interpreter, else None"""
    return (os.environ.get("JPEGTRAN") or shutil.which("jpegtran") or
            shutil.which("jpegtran", path=os.path.dirname(sys.executable)))


def jpegtran(exe: str, switches, data: bytes) -> bytes:
    with tempfile.TemporaryDirectory() as t:
        src, dst = os.path.join(t, "a.jpg"), os.path.join(t, "b.jpg")
        with open(src, "wb") as f:
            f.write(data)
        subprocess.check_call([exe, *switches, "-outfile", dst, src])
        with open(dst, "rb") as f:
            return f.read()


JPEGTRAN_PLANES = os.path.join(DIR, "jpegtran_planes.json")
TRANSPOSING = {"transpose": ["-transpose"], "transverse": ["-transverse"], "rot90": ["-rotate", "90"],
               "rot270": ["-rotate", "270"]}


def transposed_record(w, h, comps, dqt, planes) -> dict:
    """what jpegtran_planes.json keeps of a transposed file: size, SOF entries (id, H/V byte, Tq), the DQTs and
    the sha256 of every component's int16 coefficient plane (blocks in raster order, absolute DC)"""
    return {"w": w, "h": h, "comps": [list(c) for c in comps],
            "dqt": {str(k): [int(v) for v in dqt[k]] for k in sorted(dqt)},
            "planes": [sha(np.ascontiguousarray(p, np.int16)) for p in planes]}


def record_of_file(data: bytes) -> dict:
    m = SM.decoded(data)
    comps = [(c[0], (c[1] << 4) | c[2], c[3]) for c in m.P["comps"]]
    return transposed_record(m.w, m.h, comps, m.P["dqt"], m.coefs)


def committed_jpegtran_planes() -> dict:
    """"<source> <operation> [trim]" -> transposed_record of jpegtran's output, written by scripts/gen_440_golden.py"""
    with open(JPEGTRAN_PLANES) as f:
        return json.load(f)


def with_luma_hv(data: bytes, hv: int) -> bytes:
    """the stream with the H/V byte of its first SOF0 / SOF2 component replaced (the header alone matters)"""
    i = max(data.find(b"\xff\xc0"), data.find(b"\xff\xc2"))
    at = i + 4 + 6 + 1
    return data[:at] + bytes([hv]) + data[at + 1:]


def planes_of(data: bytes):
    """(layout, coefficient planes) of a baseline stream of any admitted sampling"""
    m = SM.decoded(data)
    return m.layout, m.coefs
