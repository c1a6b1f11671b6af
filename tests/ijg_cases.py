"""The cases of encoding as libjpeg does, shared by
tests/test_ijg_model.py, tests/test_ijg_gpu.py and scripts/gen_ijg_golden.py:
frames, Pillow's own files for them, and the digests the manifest
tests/golden/ijg/manifest.json keeps."""
import hashlib
import io

import numpy as np

import foreign_model as FM
import ijg_model as J
import interleave_model as IM

SIZES = [(1, 1), (3, 8), (5, 5), (9, 1), (1, 9), (8, 8), (16, 16), (17, 9), (24, 8), (33, 17), (35, 21), (40, 24),
         (47, 40), (70, 37), (200, 40)]
SAMPLINGS = ("420", "422", "444", "gray")
QUALITIES = (1, 30, 50, 75, 95, 100)
KINDS = ("photo", "noise")
SPECIAL = ("flat0", "flat255", "checker")  # 16 x 16, at Q = 100 and Q = 1
PIL_SUBSAMPLING = {"420": 2, "422": 1, "444": 0}


def frame(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    if kind == "flat0":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "flat255":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "checker":  # period 1: the largest AC coefficient
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return IM.frame(w, h, seed, kind)


def group(w: int, h: int, s: str):
    """[(name, frame, quality)] of one (size, sampling) group of the manifest"""
    return [(f"{k}_q{q}", frame(k, w, h, seed=q), q) for q in QUALITIES for k in KINDS]


def special_group(s: str):
    return [(f"{k}_q{q}", frame(k, 16, 16), q) for q in (100, 1) for k in SPECIAL]


def groups():
    """{key: (sampling, cases)} of the whole manifest"""
    out = {f"{w}x{h}_{s}": (s, group(w, h, s)) for (w, h) in SIZES for s in SAMPLINGS}
    out.update({f"special_{s}": (s, special_group(s)) for s in SAMPLINGS})
    return out


def digests(s: str, cases):
    """sha256 over every case's planes, and over every case's stream"""
    hp, hj = hashlib.sha256(), hashlib.sha256()
    for _, f, q in cases:
        m = J.model(f, q, 0, s)
        for p in m.planes:
            hp.update(np.ascontiguousarray(p, "<i2").tobytes())
        hj.update(m.jpg)
    return {"planes": hp.hexdigest(), "streams": hj.hexdigest()}


def have_pillow() -> bool:
    try:
        from PIL import features
    except ImportError:
        return False
    return bool(features.check_feature("libjpeg_turbo"))


def pillow_file(frame_bgr: np.ndarray, q: int, s: str) -> bytes:
    """Pillow's save(quality=q, subsampling=s, optimize=True) of the frame; mode L (the model's Y) for greyscale"""
    from PIL import Image
    buf = io.BytesIO()
    if s == "gray":
        y = J.ycc(np.ascontiguousarray(frame_bgr, np.uint8))[0].astype(np.uint8)
        Image.fromarray(y, "L").save(buf, "JPEG", quality=q, optimize=True)
    else:
        rgb = np.ascontiguousarray(frame_bgr[..., ::-1])
        Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=q, subsampling=PIL_SUBSAMPLING[s], optimize=True)
    return buf.getvalue()


def pillow_pixels(jpg: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpg)))


def agrees_with_pillow(frame_bgr: np.ndarray, q: int, s: str):
    """None, or what differs between the model and Pillow's file for the frame"""
    m = J.model(frame_bgr, q, 0, s)
    ref = pillow_file(frame_bgr, q, s)
    P = FM.parse(ref)
    G = FM.geometry(P)
    if FM.layout_list(G) != m.layout:
        return f"layout {FM.layout_list(G)} != {m.layout}"
    co = FM.coefficients(P, G)
    for c in range(m.G["ncomp"]):
        if not (P["dqt"][G["comps"][c][2]] == m.dqt[c]).all():
            return f"DQT of component {c}"
        if co[c].shape != m.planes[c].shape:
            return f"component {c}: {co[c].shape} != {m.planes[c].shape}"
        bad = np.argwhere(co[c] != m.planes[c])
        if bad.size:
            return f"component {c}: {len(bad)} coefficients, first {bad[:4].tolist()}"
    if not (pillow_pixels(m.jpg) == pillow_pixels(ref)).all():
        return "decoded pixels"
    return None
