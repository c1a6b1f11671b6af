#!/usr/bin/env python3
"""Times the interleaved output format: mij_batch_pad_input +
mij_batch_encode_interleaved on 64 device-resident frames of 3840x2160 and of
3837x2157 (Q = 50, restart_rows 0 and 1), HIP-event time on the batch's
stream, median of --reps, and prints one JSON line.

The yardstick, in the same process on the same frames, is the existing split
pipeline (set_split(1) + encode) at 3840x2160: the closest existing path,
which also goes through the coefficient planes.  pad_input ends with a host
synchronisation (the frame sizes come from pageable memory), so the event
time holds one host round trip between the pad kernel and K1.

The frames are the config-3 recipe's frames 0 .. distinct-1 cycled over the
slots (as bench.py cycles them); the odd size is their top-left 3837x2157.
Needs a GPU; there is no CPU fallback.

  python scripts/bench_interleaved.py [--frames 64] [--distinct 8] [--reps 10]
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
    ap.add_argument("--quality", type=int, default=50)
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_interleaved: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    W, H, n, q = a.width, a.height, a.frames, a.quality
    w2, h2 = W - 3, H - 3
    distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
    full = torch.stack([torch.from_numpy(distinct[f % len(distinct)]) for f in range(n)]).cuda()
    odd = full[:, :h2, :w2, :].contiguous()  # packed rows of 3 * 3837 bytes: no alignment at all
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()

    b = mijpeg.Batch(W, H, n, q)
    b.set_stream(int(ts.cuda_stream))
    med = lambda v: float(np.median(v))

    def timed(fn):
        fn()  # warm-up: allocations, code load
        b.sync()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            fn()
            e1.record(ts)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    # yardstick: the split three-scan pipeline on the full-size frames
    for f in range(n):
        b.upload(distinct[f % len(distinct)], first=f)
    b.set_split(True)
    split = timed(lambda: b.encode(n))
    split_bytes = int(b.lengths(n).sum())
    b.set_split(False)

    res = {}
    for name, t, (fw, fh) in (("full", full, (W, H)), ("odd", odd, (w2, h2))):
        fs, pitch = t.stride(0), t.stride(1)
        for rr in (0, 1):
            def run():
                b.pad_input(t.data_ptr(), fs, pitch, [(fw, fh)] * n)
                b.encode_interleaved(n, rr)
            ms = timed(run)
            pad = timed(lambda: b.pad_input(t.data_ptr(), fs, pitch, [(fw, fh)] * n))
            res[f"{name}_rr{rr}"] = {"size": [fw, fh], "restart_rows": rr, "ms": round(med(ms), 4),
                                     "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                     "pad_input_ms": round(med(pad), 4), "bytes": int(b.lengths(n).sum()),
                                     "ratio_to_split": round(med(ms) / med(split), 3),
                                     "Mpixels_per_s": round(fw * fh * n / med(ms) / 1e3, 1)}
    b.set_stream(0)
    b.close()
    print(json.dumps({
        "what": "pad_input + encode_interleaved vs the split three-scan pipeline (set_split(1) + encode)",
        "frames": n, "width": W, "height": H, "quality": q, "reps": a.reps,
        "split_ms": round(med(split), 4), "split_ms_min_max": [round(min(split), 4), round(max(split), 4)],
        "split_bytes": split_bytes, "interleaved": res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
