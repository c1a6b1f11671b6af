#!/usr/bin/env python3
"""Times lossless transcoding: mij_decoder_transcode on 64
streams of 3840x2160 at Q = 50 -- interleaved streams made by
mij_batch_encode_interleaved in the same process, transcoded to restart_rows 0
and 1, and the same frames as the encoder's three-scan streams -- HIP-event
time (mij_decoder_transcode_ms, which spans the call's one mid-way wait for
the frames' bit counts), median of --reps, and separately the wall-clock
median of the synchronous mij_decoder_decode that precedes it.  Prints one
JSON line.

The yardstick, in the same process on the same frames, is the entropy part of
encode_interleaved: its stages from k_il_hist through k_il_write (stats +
tables + pack of mij_batch_stage_ms), i.e. the stage total without pad_input,
K1 and k_fix_blocks.  The transcoder runs the same passes over the same
planes, plus the absolute-DC prefix sums and one host round trip.

The frames are the config-3 recipe's frames 0 .. distinct-1 cycled over the
slots (as bench.py cycles them).  Needs a GPU; there is no CPU fallback.

  python scripts/bench_transcode.py [--frames 64] [--distinct 8] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

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
        print("bench_transcode: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    W, H, n, q = a.width, a.height, a.frames, a.quality
    distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
    med = lambda v: float(np.median(v))

    # the sources, and the yardstick's stage times
    b = mijpeg.Batch(W, H, n, q)
    b.set_timing(True)
    for f in range(n):
        b.upload(distinct[f % len(distinct)], first=f)
    b.encode(n)
    three_scan = [b.output(f) for f in range(n)]
    full = torch.stack([torch.from_numpy(distinct[f % len(distinct)]) for f in range(n)]).cuda()
    torch.cuda.synchronize()
    sources, yard = {}, {}
    for rr in (0, 1):
        ent = []
        for _ in range(a.reps + 1):
            b.pad_input(full.data_ptr(), full.stride(0), full.stride(1), [(W, H)] * n)
            b.encode_interleaved(n, rr)
            st = b.stage_ms()
            ent.append(st["stats"] + st["tables"] + st["pack"])
        sources[rr] = [b.output(f) for f in range(n)]
        yard[f"rr{rr}"] = {"entropy_ms": round(med(ent[1:]), 4),
                           "entropy_ms_min_max": [round(min(ent[1:]), 4), round(max(ent[1:]), 4)],
                           "bytes": int(sum(len(s) for s in sources[rr]))}
    b.close()
    del full
    torch.cuda.empty_cache()

    d = mijpeg.Decoder(W, H, n)
    res = {}
    for name, src, rrs in (("interleaved_rr0", sources[0], (0, 1)), ("interleaved_rr1", sources[1], (0, 1)),
                           ("three_scan", three_scan, (0, 1))):
        dec = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            d.decode(src)
            dec.append((time.perf_counter() - t0) * 1e3)
        for rr in rrs:
            ms = []
            for _ in range(a.reps + 1):  # the first: allocations, code load
                d.transcode(rr)
                ms.append(d.transcode_ms())
            out_bytes = sum(len(d.transcoded(f)) for f in range(n))
            ms = ms[1:]
            res[f"{name}_to_rr{rr}"] = {"transcode_ms": round(med(ms), 4),
                                        "transcode_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                        "decode_wall_ms": round(med(dec[1:]), 3),
                                        "passes": d.passes(),
                                        "source_bytes": int(sum(len(s) for s in src)), "bytes": int(out_bytes),
                                        "ratio_to_entropy_of_encode": round(med(ms) / yard[f"rr{rr}"]["entropy_ms"], 3),
                                        "Mpixels_per_s": round(W * H * n / med(ms) / 1e3, 1)}
    # the property the format promises, on the timed data: transcoding the
    # encoder's streams gives the encoder's streams at the new interval
    d.decode(three_scan)
    d.transcode(1)
    same = all(d.transcoded(f) == sources[1][f] for f in range(n))
    d.close()
    print(json.dumps({
        "what": "mij_decoder_transcode vs the entropy stages of encode_interleaved (k_il_hist .. k_il_write)",
        "frames": n, "width": W, "height": H, "quality": q, "reps": a.reps,
        "encode_interleaved_entropy": yard, "transcode": res, "three_scan_to_rr1_equals_encode_any": same}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
