#!/usr/bin/env python3
"""Times mij_decoder_reconstruct (DC prefix + IDCT, then upsampling + colour)
on 64 config-3 streams (3840x2160, Q = 50) against a device-to-device copy
that moves the same number of bytes, and prints one JSON line.

The two-kernel path is budgeted at 10.5 bytes moved per pixel (DESIGN.md
"Decode to pixels"): the IDCT reads 3 (int16 coefficients, 1.5 samples per
pixel) and writes 1.5, the colour pass is counted with 3 read and 3 written.
The copy moves 10.5 B/px in all too: 5.25 read and 5.25 written.

The frames are the config-3 recipe's frames 0 .. distinct-1 cycled over the
64 slots (as bench.py cycles them), encoded by the library itself.  Needs a
GPU; there is no CPU fallback.

  python scripts/bench_reconstruct.py [--frames 64] [--distinct 8] [--reps 10]
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
        print("bench_reconstruct: no GPU", file=sys.stderr)
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
    d.reconstruct("bgr")  # warm-up: allocates the buffers, loads the code
    d.reconstruct_ms()
    idct, colour = [], []
    for _ in range(a.reps):
        d.reconstruct("bgr")
        t = d.reconstruct_ms()
        idct.append(t[0])
        colour.append(t[1])
    px = W * H * n
    d.close()

    nbytes = px * 21 // 4  # 5.25 B/px read + 5.25 B/px written = 10.5 B/px moved
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    copy = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        copy.append(e0.elapsed_time(e1))
    med = lambda v: float(np.median(v))
    rec = med(idct) + med(colour)
    print(json.dumps({
        "what": "mij_decoder_reconstruct vs a device-to-device copy of the same traffic",
        "frames": n, "width": W, "height": H, "quality": 50, "reps": a.reps,
        "dc_idct_ms": round(med(idct), 4), "colour_ms": round(med(colour), 4), "reconstruct_ms": round(rec, 4),
        "reconstruct_ms_min_max": [round(min(x + y for x, y in zip(idct, colour)), 4),
                                   round(max(x + y for x, y in zip(idct, colour)), 4)],
        "bytes_moved_per_px": 10.5, "copy_bytes": nbytes, "copy_ms": round(med(copy), 4),
        "ratio_to_copy": round(rec / med(copy), 3),
        "reconstruct_GBps": round(10.5 * px / rec / 1e6, 1), "copy_GBps": round(2 * nbytes / med(copy) / 1e6, 1),
        "Mpixels_per_s": round(px / rec / 1e3, 1)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
