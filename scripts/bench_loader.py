#!/usr/bin/env python3
"""Times the chain that ends in a tensor and prints one JSON
line.

  loader     64 stored streams of 3840x2160 at Q = 50 (the config-3 recipe's
             frames, as scripts/bench_scaled.py makes them) through
             mij_loader_load into [64, 3, 224, 224] float16 NCHW and into
             [64, 224, 224, 3] uint8 NHWC, centre crops, auto scale: the four
             stage times of mij_loader_ms over --reps calls after --warmup.
  tensorize  k_tensorize alone on 256 frames of 224x224 out of the resizer:
             the bytes it moves (the source words read plus the tensor bytes
             written) over its HIP-event time, next to a plain device-to-device
             copy of the same byte count measured in the same process.  The
             copy is the yardstick: this path has no predecessor.

Needs a GPU; there is no CPU fallback.

  python scripts/bench_loader.py [--frames 64] [--distinct 8] [--reps 15] [--warmup 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

OUT = (224, 224)


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tensor-frames", type=int, default=256)
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_loader: no GPU", file=sys.stderr)
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

    side = min(W, H)
    crops = [((W - side) // 2, (H - side) // 2, side, side)] * n
    out = {"what": "mij_loader_load and k_tensorize, one process", "frames": n, "width": W, "height": H, "quality": 50,
           "out": list(OUT), "crop": list(crops[0]), "reps": a.reps, "warmup": a.warmup, "loader": {}}
    loader = mijpeg.Loader(W, H, n)
    for dtype, layout in (("float16", "nchw"), ("uint8", "nhwc")):
        dst = torch.empty((n, 3, OUT[1], OUT[0]) if layout == "nchw" else (n, OUT[1], OUT[0], 3),
                          dtype=getattr(torch, dtype), device="cuda")
        rows = []
        for i in range(a.warmup + a.reps):
            loader.load(streams, OUT, crops=crops, dtype=dtype, layout=layout, out=dst)
            ms = loader.ms()
            if i >= a.warmup:
                rows.append(ms)
        cols = list(zip(*rows))
        out["loader"][f"{dtype}_{layout}"] = {
            "denom": loader.denom(), "entropy_decode_ms": stats(cols[0]), "reconstruct_ms": stats(cols[1]),
            "resize_ms": stats(cols[2]), "tensorize_ms": stats(cols[3]),
            "device_stages_ms": stats([r[1] + r[2] + r[3] for r in rows])}
    loader.close()

    # k_tensorize alone: tensor-frames frames of 224x224 as the resizer leaves them, all from one decoded image
    m = a.tensor_frames
    d = mijpeg.Decoder(W, H, 1)
    d.decode(streams[:1])
    d.reconstruct("rgb", scale=8)
    sw, sh = d.scaled_layout(0, 8)["raw"][:2]
    ptr, pitch = d.device_pixels(0)
    r = mijpeg.Resizer(m)
    r.set_stream(d.stream_ptr())
    r.resize([(ptr, pitch, sw, sh)] * m, [OUT] * m, "bilinear")
    images = [r.device_pixels(i) + OUT for i in range(m)]
    t = mijpeg.Tensorizer(m)
    t.set_stream(d.stream_ptr())
    out["tensorize"] = {"frames": m, "size": list(OUT)}
    src_bytes = m * OUT[1] * (-(-3 * OUT[0] // 4) * 4)
    for dtype, layout in (("float16", "nchw"), ("uint8", "nhwc"), ("float32", "nchw"), ("bfloat16", "nhwc")):
        nbytes = mijpeg.tensor_bytes(m, OUT[0], OUT[1], dtype)
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ms = []
        for i in range(a.warmup + a.reps):
            t.run(images, dtype=dtype, layout=layout, dst_ptr=dst.data_ptr(), cap=nbytes)
            v = t.ms()
            if i >= a.warmup:
                ms.append(v)
        moved = src_bytes + nbytes
        # the yardstick: a device-to-device copy that moves as many bytes (reads half, writes half)
        ca = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        cb = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        cms = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cb.copy_(ca)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                cms.append(e0.elapsed_time(e1))
        med, cmed = float(np.median(ms)), float(np.median(cms))
        out["tensorize"][f"{dtype}_{layout}"] = {
            "bytes_read": src_bytes, "bytes_written": nbytes, "ms": stats(ms), "GB_per_s": round(moved / med / 1e6, 1),
            "copy_ms": stats(cms), "copy_GB_per_s": round(moved / cmed / 1e6, 1), "ratio_to_copy": round(med / cmed, 3)}
    t.close()
    r.close()
    d.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
