"""What the tests of decoding at 1/2, 1/4, 1/8 scale share:
the committed foreign fixtures at every scale through scaled_model.py, the
digests of those (tests/golden/scaled_pixels.json, written by
scripts/gen_scaled_golden.py), further files made with Pillow where it is
present, and Pillow's own draft decode."""
import hashlib
import io
import json
import os

import numpy as np

import foreign_cases as FC
import foreign_model as F
import recipes
import scaled_model as SM

DENOMS = SM.DENOMS
DIGESTS = os.path.join(recipes.GOLDEN, "scaled_pixels.json")
# made on the fly for the comparison with Pillow only: (w, h) x Pillow's subsampling 0, 1, 2 at quality 92
GENERATED = [(f"gen{('444', '422', '420')[ss]}_{w}x{h}", w, h, ss)
             for (w, h) in ((100, 60), (47, 33), (129, 65), (16, 16), (7, 3)) for ss in (0, 1, 2)]


def model(name: str, denom: int) -> SM.Scaled:
    return SM.scaled(FC.model(name), denom)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests(s: SM.Scaled) -> dict:
    return {"size": [s.ow, s.oh], "rgb": sha(s.rgb), "planes": [sha(p) for p in s.planes]}


def committed_digests() -> dict:
    with open(DIGESTS) as f:
        return json.load(f)


def pillow():
    """PIL.Image where Pillow with libjpeg-turbo is present, else None"""
    try:
        from PIL import Image, features
    except ImportError:
        return None
    return Image if features.check_feature("libjpeg_turbo") else None


def generated_jpg(Image, w: int, h: int, subsampling: int) -> bytes:
    hh, ww = -(-h // 16) * 16, -(-w // 16) * 16
    a = recipes.gradients(hh, ww).astype(np.int64)
    n = recipes.noise(hh, ww, seed=w + h).astype(np.int64)
    a[hh // 3:hh // 2] = (a[hh // 3:hh // 2] + n[hh // 3:hh // 2]) // 2
    buf = io.BytesIO()
    Image.fromarray(a[:h, :w].astype(np.uint8)).save(buf, "JPEG", quality=92, subsampling=subsampling)
    return buf.getvalue()


def pillow_draft(Image, jpg: bytes, denom: int):
    """RGB pixels of Pillow's draft decode at 1/denom, or None where Pillow
    chose another scale (it does for some tiny sizes)"""
    im = Image.open(io.BytesIO(jpg))
    w, h = im.size
    im.draft(im.mode, (max(1, w // denom), max(1, h // denom)))
    if im.decoderconfig[0] != denom:
        return None
    return np.asarray(im.convert("RGB"))
