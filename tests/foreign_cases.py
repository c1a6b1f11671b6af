"""The committed foreign fixtures (tests/golden/foreign/, written by
scripts/gen_foreign_golden.py with Pillow's libjpeg-turbo) and their model
decodes, computed once and shared."""
import hashlib
import json
import os

import foreign_model as F
import recipes

DIR = os.path.join(recipes.GOLDEN, "foreign")

with open(os.path.join(DIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)

NAMES = sorted(MANIFEST["files"])
# the CPU run of the kernels' arithmetic leaves out the two 1040x520 frames
SMALL = [n for n in NAMES if "1040" not in n]


def jpg(name: str) -> bytes:
    with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
        return f.read()


def model(name: str) -> F.Decoded:
    return F.decoded(jpg(name))


def _scan_start(b: bytes) -> int:
    i = 2
    while b[i + 1] != 0xDA:
        i += 2 + ((b[i + 2] << 8) | b[i + 3])
    return i + 2 + ((b[i + 2] << 8) | b[i + 3])


def _segment(b: bytes, marker: int) -> int:
    i = 2
    while b[i + 1] != marker:
        i += 2 + ((b[i + 2] << 8) | b[i + 3])
    return i


def _rst_positions(b: bytes):
    s = _scan_start(b)
    return [i for i in range(s, len(b) - 1) if b[i] == 0xFF and 0xD0 <= b[i + 1] <= 0xD7]


def rejects() -> dict:
    """name -> (stream, word its message must hold): invalid input the decoder must refuse with MIJ_EJPEG"""
    out = {"progressive": (jpg("reject_progressive"), "baseline"), "cmyk": (jpg("reject_cmyk"), "component")}
    plain, rst = jpg("420_35x21"), jpg("420_70x37_rst1")
    s = _scan_start(plain)
    out["cut_in_scan"] = (plain[:s + (len(plain) - s) // 2], "scan")
    pos = _rst_positions(rst)
    e = bytearray(rst)
    e[pos[3] + 1] = 0xD0 + (e[pos[3] + 1] - 0xD0 + 1) % 8
    out["rst_renumbered"] = (bytes(e), "restart")
    out["rst_removed"] = (rst[:pos[5]] + rst[pos[5] + 2:], "restart")
    e = bytearray(rst)
    d = _segment(rst, 0xDD)
    e[d + 4:d + 6] = (7).to_bytes(2, "big")  # 15 MCUs: ceil(15 / 7) = 3 intervals announced, 15 present
    out["dri_too_large"] = (bytes(e), "restart")
    e = bytearray(plain)
    q = _segment(plain, 0xDB)
    e[q + 4] |= 0x10
    out["dqt_16bit"] = (bytes(e), "DQT")
    return out


def sha(a) -> str:
    return hashlib.sha256(a.tobytes()).hexdigest()


def pix_mode(G: dict) -> int:
    """csrc/mij_pixels.h PIX_*"""
    if G["ncomp"] == 1:
        return 0
    hv = (G["hmax"], G["vmax"])
    if hv == (1, 1):
        return 1
    rep = -(-G["w"] // 2) <= 2
    return {(2, 1): 2, (2, 2): 4}[hv] + rep
