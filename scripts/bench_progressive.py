#!/usr/bin/env python3
"""Times the progressive decoder and prints one JSON line:
--frames streams of --width x --height (the config-3 recipe's frames, Q = 75,
4:2:0) as progressive files through mij_decoder_decode with
MIJ_ACCEPT_PROGRESSIVE, under both lane mappings of k_prog_scan (one unit per
lane; one unit per wave, the default), next to their baseline twins (the same
pixels, quality and sampling in one interleaved scan) through the same call of the
same build.  The time is the wall clock around the synchronous call: host
parsing and staging, the upload and every launch.  No pass bar: this path has
no predecessor.

The streams are written by Pillow where it is installed ("writer":
"pillow", its 10-scan script with successive approximation); otherwise the
baseline twin is the library's own libjpeg-arithmetic encoder and the
progressive file is tests/progressive_model.py's encoder on the twin's
coefficients ("writer": "model", spectral selection only).

Needs a GPU; there is no CPU fallback.

  python scripts/bench_progressive.py [--frames 64] [--distinct 4] [--reps 5] [--warmup 1]
"""
import argparse
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--quality", type=int, default=75)
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_progressive: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    W, H, n = a.width, a.height, a.frames
    frames = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]  # BGR
    try:
        from PIL import Image
        writer = "pillow"
    except ImportError:
        writer = "model"
    base, prog = [], []
    for bgr in frames:
        if writer == "pillow":
            im = Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1]))
            for progressive, out in ((False, base), (True, prog)):
                buf = io.BytesIO()
                im.save(buf, "JPEG", quality=a.quality, subsampling=2, progressive=progressive)
                out.append(buf.getvalue())
        else:
            import progressive_model as PM
            jpg = mijpeg.encode_libjpeg(bgr, "bgr", a.quality, 0, sampling="420")
            d = mijpeg.Decoder(W, H, 1)
            d.decode([jpg])
            lay = d.layout(0)
            coefs = [d.component(0, c) for c in range(3)]
            dqt = d.info(0)[2]
            d.close()
            G = dict(lay, ri=0)
            tables = {G["comps"][0][2]: dqt[:64], G["comps"][1][2]: dqt[64:]}
            script = [([0, 1, 2], 0, 0, 0)] + [([c], s, e, 0) for c in range(3) for s, e in ((1, 5), (6, 63))]
            base.append(jpg)
            prog.append(PM.encode(G, coefs, tables, script))
    base = [base[f % len(base)] for f in range(n)]
    prog = [prog[f % len(prog)] for f in range(n)]

    d = mijpeg.Decoder(W, H, n, progressive=True)

    def run(streams, mapping=0):
        d.lib.mij_test_prog_mapping(d.h_, mapping)
        ms = []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            d.decode(streams)
            t1 = time.perf_counter()
            if i >= a.warmup:
                ms.append(1e3 * (t1 - t0))
        return stats(ms)

    out = {"what": "mij_decoder_decode, progressive next to baseline twins, one process", "frames": n, "width": W,
           "height": H, "quality": a.quality, "sampling": "420", "writer": writer, "reps": a.reps, "warmup": a.warmup,
           "bytes": {"baseline": sum(map(len, base)), "progressive": sum(map(len, prog))}}
    out["baseline_ms"] = run(base)
    out["progressive_lane_ms"] = run(prog, 0)
    info = d.scan_info(0)
    out["nscans"], out["levels"] = info["nscans"], info["levels"]
    lane = [d.component(0, c).copy() for c in range(3)]
    out["progressive_wave_ms"] = run(prog, 1)
    out["mappings_agree"] = all((d.component(0, c) == lane[c]).all() for c in range(3))
    d.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
