"""The streams the pixel-path tests decode, with what the numpy model
(decode_model.py) makes of the ORACLE's coefficients of each: shared by
test_decode_model.py, test_pixels.py and scripts/gen_decode_golden.py, each
case computed once per process and never modified."""
import functools
import hashlib
import json
import os

import numpy as np

import decode_model as M
import oracle as O
import recipes

# the cases checked against libjpeg (Pillow) byte for byte and pinned by
# digest in tests/golden/decode_pixels.json.  checkerboards at Q = 100 is
# not among them: libjpeg misreads that stream's last luma block (DESIGN.md
# "Decode to pixels", the unstuffed FF)
LIBJPEG_CASES = (["sample_64x64"]
                 + [f"{r}_q{q}" for r in ("noise", "gradients", "checkerboards") for q in (10, 50, 90)]
                 + ["noise_q100", "gradients_q100", "near_gray_q50", "config3_496x272_q50"])

_FRAMES = {
    "noise": recipes.noise, "gradients": recipes.gradients, "near_gray": recipes.near_gray,
    "checkerboards": lambda: recipes.checkerboards(64, 128),
    "config3_496x272": lambda: recipes.config3_frame(0, 272, 496),
    "config3_1920x1280": lambda: recipes.config3_frame(0, 1280, 1920),
    "noise_16x16": lambda: recipes.noise(16, 16, 11), "noise_16x48": lambda: recipes.noise(48, 16, 12),
    "noise_48x16": lambda: recipes.noise(16, 48, 13),
}
DIGESTS = os.path.join(recipes.GOLDEN, "decode_pixels.json")


class Case:
    def __init__(self, name, jpg, Y, Cb, Cr, w, h):
        self.name, self.jpg, self.coefs, self.w, self.h = name, jpg, (Y, Cb, Cr), w, h
        self.dqt = M.stream_dqt(jpg)
        self.rgb, self.planes = M.decode(Y, Cb, Cr, *self.dqt, w, h)
        self.bgr = np.ascontiguousarray(self.rgb[..., ::-1])
        for a in (self.rgb, self.bgr, *self.planes):
            a.setflags(write=False)

    def digests(self) -> dict:
        sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        return {"rgb": sha(self.rgb), "y": sha(self.planes[0]), "cb": sha(self.planes[1]), "cr": sha(self.planes[2])}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    """`<frame>_q<Q>` (a recipe above, encoded by the oracle) or sample_64x64
    (the committed reference stream and the reference's coefficient dump)"""
    if name == "sample_64x64":
        with open(os.path.join(recipes.GOLDEN, "sample_64x64.jpg"), "rb") as f:
            jpg = f.read()
        z = np.load(os.path.join(recipes.GOLDEN, "sample_64x64.coefs.npz"))
        return Case(name, jpg, z["Y"], z["Cb"], z["Cr"], 64, 64)
    frame, q = name.rsplit("_q", 1)
    bgr = _FRAMES[frame]()
    Y, Cb, Cr, _, jpg = O.cref_stages(bgr, int(q))
    return Case(name, jpg, Y, Cb, Cr, bgr.shape[1], bgr.shape[0])


def committed_digests() -> dict:
    with open(DIGESTS) as f:
        return json.load(f)


def libjpeg_pixels(jpg: bytes):
    """(RGB, Y) as Pillow's libjpeg-turbo decodes the stream, or None where
    Pillow or its libjpeg-turbo is missing"""
    try:
        from PIL import Image, features
    except ImportError:
        return None
    if not features.check_feature("libjpeg_turbo"):
        return None
    import io
    rgb = np.array(Image.open(io.BytesIO(jpg)).convert("RGB"))
    im = Image.open(io.BytesIO(jpg))
    im.draft("YCbCr", im.size)
    return rgb, np.array(im)[..., 0]
