#!/usr/bin/env python3
"""Times mij_decoder_reconstruct_scaled at 1/2, 1/4 and 1/8 against the
full-size mij_decoder_reconstruct of the same decode, in one process, on the
64 config-3 streams (3840x2160, Q = 50) scripts/bench_reconstruct.py uses,
with the decoder's own HIP events, and prints one JSON line.

The frames are the config-3 recipe's frames 0 .. distinct-1 cycled over the
64 slots, encoded by the library itself and entropy-decoded once.  Needs a
GPU; there is no CPU fallback.

  python scripts/bench_scaled.py [--frames 64] [--distinct 8] [--reps 10]

The per-kernel split comes from a run of its own under the profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_scaled.py --reps 3
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_scaled: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    W, H, n = a.width, a.height, a.frames
    distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
    b = mijpeg.Batch(W, H, n, 50)
    for f in range(n):
        b.upload(distinct[f % len(distinct)], first=f)
    b.encode(n)
    streams = [b.output(f) for f in range(n)]
    b.close()

    d = mijpeg.Decoder(W, H, n)
    d.decode(streams)
    out = {"what": "mij_decoder_reconstruct_scaled vs mij_decoder_reconstruct, one decode, one process",
           "frames": n, "width": W, "height": H, "quality": 50, "reps": a.reps, "scales": {}}
    med = lambda v: float(np.median(v))
    for scale in (1, 2, 4, 8):
        d.reconstruct("bgr", scale=scale)  # warm-up: allocates the buffers, loads the code
        d.reconstruct_ms()
        idct, colour = [], []
        for _ in range(a.reps):
            d.reconstruct("bgr", scale=scale)
            t = d.reconstruct_ms()
            idct.append(t[0])
            colour.append(t[1])
        tot = [x + y for x, y in zip(idct, colour)]
        out["scales"][f"1/{scale}"] = {
            "size": list(d.scaled_layout(0, scale)["raw"][:2]),
            "dc_idct_ms": round(med(idct), 4), "colour_ms": round(med(colour), 4), "reconstruct_ms": round(med(tot), 4),
            "reconstruct_ms_min_max": [round(min(tot), 4), round(max(tot), 4)]}
    d.close()
    full = out["scales"]["1/1"]["reconstruct_ms"]
    for k, v in out["scales"].items():
        v["ratio_to_full"] = round(v["reconstruct_ms"] / full, 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
