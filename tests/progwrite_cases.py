"""The sources of the progressive-output tests: the small
baseline files of tests/golden/foreign/, their progressive twins of
tests/golden/progressive/, and the two files of tests/golden/progressive_write/
that reach the limits of an EOB run (scripts/gen_progwrite_golden.py).  Also
the CPU run of the shared per-block routines (tests/progwrite_check.cpp).
Shared by the CPU and the GPU tests, so both see the same bytes."""
import os
import struct
import subprocess

import numpy as np

import foreign_cases as FC
import progressive_cases as PC
import progressive_model as PM
import progwrite_model as W
import recipes

DIR = os.path.join(recipes.GOLDEN, "progressive_write")
LIMITS = ["corr_limit", "run_limit"]
# every sampling, 1x1, partial MCUs whose luma grid is narrower than the padded plane, sources with intervals
BASELINE = ["grey_35x21", "444_17x9", "422_35x21", "420_35x21", "420_1x1", "420_70x37_rstrow", "420_96x80_noise_q95"]
PILLOW = [n for n in PC.NAMES if n.startswith("p")]
TWINS = [n for n in PILLOW if PC.twin(n) in BASELINE]


def jpg(name: str) -> bytes:
    """a fixture by name, from whichever of the three directories holds it"""
    if name in LIMITS:
        with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
            return f.read()
    return PC.jpg(name) if name in PC.NAMES else FC.jpg(name)


def coded_inside(src, got, G, c):
    """(source, decoded) coefficients of component c that a progressive file carries: every DC, the AC
    coefficients of the blocks inside the component's own grid"""
    ins = PM.inside(G, c)
    return (src[:, 0], src[ins]), (got[:, 0], got[ins])


# ---- the CPU run of the shared routines (tests/progwrite_check.cpp) ----
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(directory) -> str:
    """progwrite_check, compiled with the address and undefined-behaviour sanitizers; a program of its own"""
    exe = os.path.join(str(directory), "progwrite_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-Werror", "-I" + os.path.join(REPO, "jpeg-encoder-decoder_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "progwrite_check.cpp")])
    return exe


def run_check(exe: str, directory, label: str, G, coefs, restart_rows: int):
    """every scan of the script through the program -> per scan the intervals' tokens, as W.tokens gives them"""
    sc = W.script(G["ncomp"])
    blob = bytearray(struct.pack("<i", len(sc)))
    for comps, ss, se, ah, al in sc:
        mcus = PM.scan_blocks(G, list(comps))
        ri = restart_rows * W.across(G, comps) or len(mcus)
        bpm = len(mcus[0])
        blob += struct.pack("<6i", ss, se, ah, al, len(mcus) * bpm, ri * bpm)
        rec = np.zeros(len(mcus) * bpm, np.dtype([("t", "<i4"), ("p", "<i4"), ("c", "<i2", 64)]))
        i = 0
        for m, mcu in enumerate(mcus):
            if m % ri == 0:
                last = {}
            for j, b in mcu:
                rec[i] = (1 if comps[j] else 0, last.get(j, -1), np.asarray(coefs[comps[j]][b], np.int16))
                last[j] = i
                i += 1
        blob += rec.tobytes()
    src, dst = os.path.join(str(directory), label + ".in"), os.path.join(str(directory), label + ".out")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    tok = np.fromfile(dst, "<i4").reshape(-1, 4)
    out, k = [], 0
    ends = np.flatnonzero(tok[:, 0] == -2)
    for comps, ss, se, ah, al in sc:
        nint = -(-len(PM.scan_blocks(G, list(comps))) // (restart_rows * W.across(G, comps) or 1 << 62))
        parts = []
        for _ in range(nint):
            start = ends[k - 1] + 1 if k else 0
            parts.append([tuple(int(v) for v in t) for t in tok[start:ends[k]]])
            k += 1
        out.append(parts)
    assert k == len(ends)
    return out
