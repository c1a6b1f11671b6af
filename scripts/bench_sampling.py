#!/usr/bin/env python3
"""Times encoding at a chosen chroma sampling:
mij_batch_pad_input + mij_batch_encode_sampled on 64 device-resident frames
of 3840x2160 and of 3837x2157 (Q = 50), for 4:2:2, 4:4:4 and greyscale,
HIP-event time on the batch's stream, median of --reps, and prints one JSON
line.

The yardstick, in the same process on the same frames, is pad_input +
encode_interleaved (4:2:0 through K1).  Both calls hold host round trips
(pad_input's, and the sampled encode's read-back of the frames' bit counts),
so the event times include them.  "front_end_ms" is the front-end kernel's
own time from the batch's stage events (set_timing): the stretch between the
call's first event and the one recorded after k_samp_dct; "blocks" counts
the 8x8 blocks it transformed and "front_end_fp64_gflops" rates them at 2,112
unfused FP64 operations a block (2 x 64 x 16 for the two passes, 64 for the
scale and the divide).

The frames are the config-3 recipe's frames 0 .. distinct-1 cycled over the
slots (as bench.py cycles them); the odd size is their top-left 3837x2157.
Needs a GPU; there is no CPU fallback.

  python scripts/bench_sampling.py [--frames 64] [--distinct 8] [--reps 10]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

FP64_OPS_PER_BLOCK = 2 * 64 * 16 + 64


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--samplings", default="422,444,gray")
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_sampling: no GPU", file=sys.stderr)
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

    def blocks(fw, fh, s):
        hmax, vmax = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "gray": (1, 1)}[s]
        return -(-fw // (8 * hmax)) * -(-fh // (8 * vmax)) * (hmax * vmax + (0 if s == "gray" else 2)) * n

    res = {}
    for name, t, (fw, fh) in (("full", full, (W, H)), ("odd", odd, (w2, h2))):
        fs, pitch = t.stride(0), t.stride(1)
        dims = [(fw, fh)] * n

        def run420():
            b.pad_input(t.data_ptr(), fs, pitch, dims)
            b.encode_interleaved(n, 0)
        base = timed(run420)
        base_bytes = int(b.lengths(n).sum())
        pad = timed(lambda: b.pad_input(t.data_ptr(), fs, pitch, dims))
        cur = {"size": [fw, fh], "pad_input_ms": round(med(pad), 4),
               "420": {"ms": round(med(base), 4), "ms_min_max": [round(min(base), 4), round(max(base), 4)],
                       "bytes": base_bytes}}
        for s in a.samplings.split(","):
            def run():
                b.pad_input(t.data_ptr(), fs, pitch, dims)
                b.encode_sampled(n, s, 0)
            ms = timed(run)
            nbytes = int(b.lengths(n).sum())
            b.set_timing(True)
            fe, tot = [], []
            for _ in range(a.reps):
                b.encode_sampled(n, s, 0)
                b.sync()
                st = b.stage_ms()
                fe.append(st["k1_colour_dct_quant"])
                tot.append(st["total"])
            b.set_timing(False)
            nb = blocks(fw, fh, s)
            cur[s] = {"ms": round(med(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "bytes": nbytes,
                      "ratio_to_420": round(med(ms) / med(base), 3),
                      "Mpixels_per_s": round(fw * fh * n / med(ms) / 1e3, 1),
                      "encode_sampled_ms": round(med(tot), 4), "front_end_ms": round(med(fe), 4),
                      "front_end_share_of_call": round(med(fe) / med(ms), 3), "blocks": nb,
                      "front_end_fp64_gflops": round(nb * FP64_OPS_PER_BLOCK / med(fe) / 1e6, 1)}
        res[name] = cur
    b.set_stream(0)
    b.close()
    print(json.dumps({
        "what": "pad_input + encode_sampled per sampling vs pad_input + encode_interleaved (4:2:0)",
        "frames": n, "width": W, "height": H, "quality": q, "reps": a.reps, "sizes": res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
