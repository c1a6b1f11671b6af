"""The committed progressive fixtures (tests/golden/progressive/, written by
scripts/gen_progressive_golden.py), their model decodes, computed once and
shared, and the streams derived from them that the decoder must refuse
(illegal scan scripts) or find corrupt (cut, overrun and flipped entropy
data).  Shared by the CPU and the GPU tests, so both see the same bytes."""
import json
import os

import foreign_cases as FC
import progressive_model as PM
import recipes

DIR = os.path.join(recipes.GOLDEN, "progressive")

with open(os.path.join(DIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)

NAMES = sorted(MANIFEST["files"])


def jpg(name: str) -> bytes:
    with open(os.path.join(DIR, name + ".jpg"), "rb") as f:
        return f.read()


def model(name: str) -> PM.Decoded:
    return PM.decoded(jpg(name))


def twin(name: str) -> str:
    """the baseline file of the same picture in tests/golden/foreign/"""
    return MANIFEST["files"][name]["twin"]


def spans(b: bytes):
    """(first, one past the last) byte of each scan's entropy data"""
    return [s["span"] for s in PM.parse(b)["scans"]]


def script(b: bytes):
    return [(s["ss"], s["ah"]) for s in PM.parse(b)["scans"]]


def cut_scan(b: bytes, k: int) -> bytes:
    """scan k loses the second half of its entropy data (of its last restart interval, where it has several: the
    markers stay, so the headers stay sound); the scans after it stay"""
    s, e = spans(b)[k]
    rst = [i for i in range(s, e - 1) if b[i] == 0xFF and 0xD0 <= b[i + 1] <= 0xD7]
    if rst:
        s = rst[-1] + 2
    mid = s + (e - s) // 2
    if b[mid - 1] == 0xFF:  # not between a 0xFF and its stuffed zero
        mid -= 1
    return b[:mid] + b[e:]


def flip_bit(b: bytes, k: int) -> bytes:
    """one bit of scan k's entropy data flipped, at a byte where that neither makes nor unmakes a marker"""
    s, e = spans(b)[k]
    for i in list(range(s + (e - s) // 2, e)) + list(range(s, s + (e - s) // 2)):
        if b[i] not in (0xFF, 0xFE) and b[i - 1] != 0xFF:
            return b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    raise AssertionError("no byte to flip")


def _twin_planes(name: str):
    t = FC.model(name)
    return dict(t.G, ri=0), t.coefs, {c[2]: t.dqt[i] for i, c in enumerate(t.G["comps"])}


BANDS = [([0, 1, 2], 0, 0, 0)] + [([c], a, b, 0) for c in range(3) for a, b in ((1, 5), (6, 20), (21, 63))]


def eob_overrun() -> bytes:
    """m444_17x9_bands with the last end-of-band run of its Y 21-63 scan coded 3 blocks too long"""
    return PM.encode(*_twin_planes("444_17x9"), BANDS, eob_extra=(3, 3))


def corrupt() -> dict:
    """name -> (stream, the scan that is corrupt, its status code): the two streams that go on to the device
    (tests/test_progressive_gpu.py) once tests/test_progressive_model.py has run these bytes through the same
    decode routine on the CPU under the sanitizers"""
    p = jpg("p420_35x21")
    _, refine = first_and_refinement(p)
    return {"cut_refinement": (cut_scan(p, refine), refine, 5), "eob_overrun": (eob_overrun(), 3, 8)}


def first_and_refinement(b: bytes):
    """indices of an AC first scan and (where the file has one) an AC refinement scan"""
    sc = script(b)
    first = next(k for k, (ss, ah) in enumerate(sc) if ss > 0 and ah == 0)
    refine = next((k for k, (ss, ah) in enumerate(sc) if ss > 0 and ah > 0), None)
    return first, refine


def _edit_tail(b: bytes, k: int, se=None, ahal=None) -> bytes:
    s = spans(b)[k][0]
    e = bytearray(b)
    if se is not None:
        e[s - 2] = se
    if ahal is not None:
        e[s - 1] = ahal
    return bytes(e)


def refusals() -> dict:
    """name -> (stream, its refusal as the library words it, without the "stream N" in front): scan scripts and
    segments that MIJ_ACCEPT_PROGRESSIVE does not admit"""
    p = jpg("p420_35x21")  # Pillow's script: 0 DC Al 1; 1 Y 1-5 Al 2; 2, 3 Cb, Cr 1-63 Al 1; 4 Y 6-63 Al 2; 5 Y refine ...
    sp = spans(p)
    G, coefs, dqt = _twin_planes("444_17x9")
    enc = lambda sc: PM.encode(G, coefs, dqt, sc)
    out = {
        "dc_scan_with_se": (_edit_tail(p, 0, se=5), "scan 0: Ss 0 Se 5 (a DC scan has Se 0, an AC scan Ss <= Se <= 63)"),
        "ac_scan_of_three": (enc([([0, 1, 2], 0, 0, 0), ([0, 1, 2], 1, 63, 0)]), "scan 1: AC scan of 3 components (only 1)"),
        "al_14": (_edit_tail(p, 0, ahal=0x0E), "scan 0: Al 14 (at most 13)"),
        "first_scan_with_ah": (_edit_tail(p, 0, ahal=0x21), "scan 0: component 0 coefficient 0: Ah 2 Al 1 after no scan, 0 "
                               "(successive approximation out of order)"),
        "refinement_skips_a_bit": (_edit_tail(p, 5, ahal=0x10), "scan 5: component 0 coefficient 1: Ah 1 Al 0 after Al 2 "
                                   "(successive approximation out of order)"),
        "ac_before_dc": (enc([([0], 1, 63, 0)] + BANDS), "scan 0: AC scan of component 0 before its DC scan"),
        "band_never_coded": (enc(BANDS[:-1]), ": incomplete scan script: component 2 coefficient 21 is never coded"),
        # the last scan (Y 1-63 from Al 1 to 0) and its table left out
        "last_refinement_missing": (p[:sp[-2][1]] + b"\xff\xd9", ": incomplete scan script: component 0 coefficient 1 ends at Al 1"),
        "too_many_scans": (enc([([0, 1, 2], 0, 0, 0)] + [([c], k, k, 0) for c in range(3) for k in range(1, 64)]),
                           ": more than 64 scans"),
    }
    q = FC._segment(p, 0xDB)
    dqt_seg = p[q:q + 2 + ((p[q + 2] << 8) | p[q + 3])]
    out["dqt_between_scans"] = (p[:sp[0][1]] + dqt_seg + p[sp[0][1]:], ": DQT after the first scan of a progressive frame")
    # an AC band outside Ss..63 (scan 1 is Y 1-5)
    out["se_below_ss"] = (_edit_tail(p, 1, se=0), "scan 1: Ss 1 Se 0 (a DC scan has Se 0, an AC scan Ss <= Se <= 63)")
    out["se_above_63"] = (_edit_tail(p, 1, se=64), "scan 1: Ss 1 Se 64 (a DC scan has Se 0, an AC scan Ss <= Se <= 63)")
    # restart intervals count the scan's own MCUs: 70x37 at 4:2:0 is 5x3 MCUs, its luma grid 9x5 = 45 blocks; one
    # interval per MCU row gives the DC scan Ri 5 (3 intervals) and the luma scans Ri 9 (5 intervals)
    r = jpg("p420_70x37_rstrow")
    rs, re_ = spans(r)[1]
    rst = [i for i in range(rs, re_ - 1) if r[i] == 0xFF and 0xD0 <= r[i + 1] <= 0xD7]
    assert len(rst) == 4
    e = bytearray(r)
    e[rst[1] + 1] = 0xD3
    out["rst_out_of_order"] = (bytes(e), "scan 1: restart marker RST3 where RST1 is due (interval 1)")
    out["rst_removed"] = (r[:rst[2]] + r[rst[2] + 2:], "scan 1: restart marker RST3 where RST2 is due (interval 2)")
    out["rst_last_removed"] = (r[:rst[3]] + r[rst[3] + 2:], "scan 1: 4 restart intervals, 5 expected (45 MCUs, interval 9)")
    out["rst_one_too_many"] = (r[:re_] + b"\xff\xd4" + r[re_:], "scan 1: more restart markers than its 5 intervals need")
    # the DRI in front of scan 1 says 15: what the MCU grid of the frame would hold, not the component's 45 blocks
    d = max(i for i in range(rs) if r[i] == 0xFF and r[i + 1] == 0xDD)
    assert r[d + 2:d + 6] == b"\x00\x04\x00\x09"
    e = bytearray(r)
    e[d + 4:d + 6] = (15).to_bytes(2, "big")
    out["dri_by_the_frames_mcus"] = (bytes(e), "scan 1: more restart markers than its 3 intervals need")
    # a restart marker where no interval is in force ends the scan and is refused as a stray marker
    s1 = sp[1][0]
    out["rst_without_dri"] = (p[:s1] + b"\xff\xd0" + p[s1:], ": restart marker RST0 without a restart interval in force")
    return out


# ---- the CPU run of the shared decode routine (tests/progressive_check.cpp) ----
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_check(directory) -> str:
    """progressive_check, compiled with the address and undefined-behaviour sanitizers; a program of its own"""
    import subprocess
    exe = os.path.join(str(directory), "progressive_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                           "-Werror", "-I" + os.path.join(REPO, "jpeg-encoder-decoder_amd", "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "progressive_check.cpp")])
    return exe


def run_check(exe: str, directory, cases):
    """cases: [(label, stream, coefficient planes or None, expectation)] -> the program's lines by label; asserts
    that every expectation held and that the sanitizers found nothing"""
    import subprocess
    args = []
    for label, stream, coefs, expect in cases:
        path = os.path.join(str(directory), label + ".jpg")
        with open(path, "wb") as f:
            f.write(stream)
        cpath = "-"
        if coefs is not None:
            cpath = os.path.join(str(directory), label + ".coefs")
            with open(cpath, "wb") as f:
                f.write(b"".join(c.tobytes() for c in coefs))
        args += [path, cpath, expect]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases) + 1
    return {label: line.split(": ", 1)[1] for (label, _, _, _), line in zip(cases, lines)}
