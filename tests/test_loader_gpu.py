"""The chain that ends in a tensor: mij_loader_load against
the composition of the stages that are pinned one by one -- mijpeg.decode at
the call's scale (tests/test_scaled_gpu.py), the model's rectangle rule,
resize_model.resize (tests/test_resize_gpu.py), the mirror, tensor_model
(tests/test_tensor_gpu.py).  Every comparison is equality of bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import foreign_cases as FC
import mijpeg
import resize_model as RM
import tensor_model as TM

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# different sizes and samplings in one call
NAMES = ("420_1040x520_q30", "444_40x24", "grey_35x21", "422_35x21")
SIZES = ((1040, 520), (40, 24), (35, 21), (35, 21))
CROPS = ((101, 53, 801, 401), (3, 1, 35, 21), (1, 3, 33, 17), (0, 0, 35, 21))  # odd offsets, and a whole frame
MIRROR = (1, 0, 1, 0)
OUT = (16, 12)


def jpgs():
    return [FC.jpg(n) for n in NAMES]


def want(streams, sizes, crops, mirror, d, order, f, **kw):
    frames = []
    for i, s in enumerate(streams):
        px = mijpeg.decode(s, order, scale=d)
        W, H = sizes[i]
        assert px.shape[:2] == (-(-H // d), -(-W // d))
        x0, y0, x1, y1 = TM.rect(crops[i] if crops is not None else None, W, H, d)
        frames.append(RM.resize(np.ascontiguousarray(px[y0:y1, x0:x1]), OUT, f))
    return TM.tensorize(frames, mirror, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


@pytest.fixture(scope="module")
def loader():
    l = mijpeg.Loader(1040, 520, 4)
    yield l
    l.close()


@pytest.mark.parametrize("scale,crops", [(0, CROPS), (0, None), (1, CROPS), (2, CROPS), (4, None)],
                         ids=["auto_crops", "auto_whole", "1_crops", "2_crops", "4_whole"])
def test_load_equals_the_composition_of_its_stages(loader, scale, crops):
    d = TM.denom(SIZES, crops, *OUT)
    assert d == 1  # the small frames decide
    got = loader.load(jpgs(), OUT, crops=crops, mirror=MIRROR, filter="bilinear", scale=scale)
    assert loader.denom() == (scale or d)
    ref = want(jpgs(), SIZES, crops, MIRROR, scale or d, "rgb", "bilinear")
    assert got.shape == (4, 3, 12, 16) and got.dtype == np.float16
    assert (bits(got) == bits(ref)).all(), int((bits(got) != bits(ref)).sum())
    ms = loader.ms()
    assert len(ms) == 4 and all(v >= 0 for v in ms), ms
    assert loader.device()[1] == got.nbytes


def test_auto_scale_of_large_frames_other_filters_dtypes_and_order(loader):
    """two crops of the large file: 801x401 asks for 1/8, 70x500 for 1/4, the call takes 1/4"""
    big = FC.jpg(NAMES[0])
    crops = [CROPS[0], (7, 9, 70, 500)]
    assert mijpeg.thumbnail_denom(801, 401, *OUT) == 8 and mijpeg.thumbnail_denom(70, 500, *OUT) == 4
    for f, dtype, layout, order in (("bicubic", "float32", "nhwc", "bgr"), ("box", "uint8", "nchw", "rgb"),
                                    ("bilinear", "bfloat16", "nhwc", "rgb")):
        got = loader.load([big, big], OUT, crops=crops, mirror=None, filter=f, dtype=dtype, layout=layout, order=order,
                          mean=(0.5, 0.25, 0.125), std=(1 / 3, 0.7, 2.0))
        assert loader.denom() == 4 == TM.denom([SIZES[0]] * 2, crops, *OUT)
        ref = want([big, big], [SIZES[0]] * 2, crops, None, 4, order, f, dtype=dtype, layout=layout,
                   mean=(0.5, 0.25, 0.125), std=(1 / 3, 0.7, 2.0))
        assert got.shape == ref.shape and (bits(got) == bits(ref)).all(), (f, dtype, layout, order)
    got = loader.load([big], OUT, crops=[CROPS[0]])
    assert loader.denom() == 8
    assert (bits(got) == bits(want([big], [SIZES[0]], [CROPS[0]], None, 8, "rgb", "bilinear"))).all()


def test_refusals(loader):
    ok = loader.load(jpgs()[1:3], OUT)
    lib = loader.lib
    with pytest.raises(mijpeg.MijError, match="(?i)baseline"):
        loader.load([jpgs()[1], FC.jpg("reject_progressive")], OUT)
    assert lib.mij_last_error() == 8  # MIJ_EJPEG
    for kw, word in ((dict(crops=[(0, 0, 40, 24), (30, 1, 6, 5)]), "frame 1: crop"), (dict(scale=3), "denom 3"),
                     (dict(dtype=5), "dtype 5"), (dict(filter=4), "filter 4")):
        with pytest.raises(mijpeg.MijError, match=word):
            loader.load(jpgs()[1:3], OUT, **kw)
        assert lib.mij_last_error() == 1  # MIJ_EINVAL
    with pytest.raises(mijpeg.MijError, match="n 5"):
        loader.load(jpgs() + jpgs()[:1], OUT)
    small = mijpeg.Loader(36, 22, 2)
    try:
        with pytest.raises(mijpeg.MijError, match="frame 1: 40x24 exceeds the loader's 36x22"):
            small.load([jpgs()[2], jpgs()[1]], OUT)
        with pytest.raises(mijpeg.MijError, match="no mij_loader_load"):
            small.ms()
    finally:
        small.close()
    # the refused calls left the last result readable
    back = np.zeros_like(ok)
    assert lib.mij_loader_read(loader.h_, back.ctypes.data, back.nbytes) == 0 and (bits(back) == bits(ok)).all()


CHILD = r"""
import sys
import torch  # its HIP runtime before the library's
if not torch.cuda.is_available():
    print("NO DEVICE")
    sys.exit(0)
for p in sys.argv[1:3]:
    sys.path.insert(0, p)
import numpy as np
import foreign_cases as FC
import mijpeg
import test_loader_gpu as T
streams = T.jpgs()
n = len(streams)
out = torch.empty((n, 3, 12, 16), dtype=torch.float16, device="cuda")
l = mijpeg.Loader(1040, 520, n)
assert l.load(streams, T.OUT, crops=T.CROPS, mirror=T.MIRROR, out=out) is out
torch.cuda.synchronize()
got = out.cpu().numpy()
ref = T.want(streams, T.SIZES, T.CROPS, T.MIRROR, l.denom(), "rgb", "bilinear")
assert l.denom() == 1 and got.dtype == ref.dtype and (got.view(np.uint16) == ref.view(np.uint16)).all()
for bad, word in ((torch.empty((n, 3, 12, 15), dtype=torch.float16, device="cuda"), "elements"),
                  (torch.empty((n, 3, 12, 16), dtype=torch.float32, device="cuda"), "dtype"),
                  (torch.empty((n, 3, 12, 32), dtype=torch.float16, device="cuda")[..., ::2], "contiguous")):
    try:
        l.load(streams, T.OUT, out=bad)
    except mijpeg.MijError as e:
        assert word in str(e), e
    else:
        raise AssertionError(word)
l.close()
print("TENSOR OK")
"""


def test_load_into_a_torch_tensor_in_a_fresh_process():
    """a child process that imports torch first, then the library, and loads
    into a tensor torch allocated; skipped where torch sees no device"""
    pkg = os.path.dirname(mijpeg.LIB_PATH)
    run = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "tests"), pkg], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    if "NO DEVICE" in run.stdout:
        pytest.skip("torch sees no device")
    assert "TENSOR OK" in run.stdout, run.stdout + run.stderr
