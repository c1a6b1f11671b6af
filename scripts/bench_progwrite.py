#!/usr/bin/env python3
"""Times progressive output against the baseline transcode of
the same decoded planes, in one process: 64 streams of 3840x2160 at Q = 50
and 64 of 1920x1088 at Q = 75, both 4:2:0 from mij_batch_encode_interleaved
on the config-3 recipe's frames (cycled over the slots, as bench.py cycles
them).  Per set it reports the HIP-event time of mij_decoder_transcode
(mij_decoder_transcode_ms, median of --reps) with baseline output and with
progressive output at restart_rows 0 and 1, the bytes of each, and the
wall-clock time of mij_decoder_decode of the written progressive files.
Prints one JSON line.

--only progressive|baseline runs just that transcode --reps times and prints
nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the
split per kernel (counters and traces in runs of their own).

Needs a GPU; there is no CPU fallback.

  python scripts/bench_progwrite.py [--frames 64] [--distinct 8] [--reps 10] [--sets 4k,1080]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

SETS = {"4k": (3840, 2160, 50), "1080": (1920, 1088, 75)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sets", default="4k,1080")
    ap.add_argument("--only", choices=["progressive", "baseline"], default=None)
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_progwrite: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    n = a.frames
    med = lambda v: float(np.median(v))
    res = {}
    for name in a.sets.split(","):
        W, H, q = SETS[name]
        distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
        b = mijpeg.Batch(W, H, n, q)
        full = torch.stack([torch.from_numpy(distinct[f % len(distinct)]) for f in range(n)]).cuda()
        torch.cuda.synchronize()
        b.pad_input(full.data_ptr(), full.stride(0), full.stride(1), [(W, H)] * n)
        b.encode_interleaved(n, 0)
        src = [b.output(f) for f in range(n)]
        b.close()
        del full
        torch.cuda.empty_cache()

        d = mijpeg.Decoder(W, H, n, progressive=True)
        d.decode(src)

        def timed(fmt, rr, keep=False):
            d.output(fmt)
            ms = []
            for _ in range(a.reps + 1):  # the first: allocations, code load
                d.transcode(rr)
                ms.append(d.transcode_ms())
            ms = ms[1:]
            out = [d.transcoded(f) for f in range(n)] if keep else None
            return {"ms": round(med(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}, out

        if a.only:
            timed(a.only, 0)
            d.close()
            continue
        r = {"source_bytes": int(sum(len(s) for s in src))}
        base, out_b = timed("baseline", 0, True)
        r["baseline_rr0"] = dict(base, bytes=int(sum(len(s) for s in out_b)))
        files = {}
        for rr in (0, 1):
            t, files[rr] = timed("progressive", rr, True)
            r[f"progressive_rr{rr}"] = dict(t, bytes=int(sum(len(s) for s in files[rr])),
                                            ratio_to_baseline=round(t["ms"] / base["ms"], 3))
        r["progressive_smaller_by"] = round(1 - r["progressive_rr0"]["bytes"] / r["baseline_rr0"]["bytes"], 4)
        # the written files read back by this library: a scan per restart interval is a unit of k_prog_scan
        planes = [d.component(0, c).copy() for c in range(3)]
        for rr in (0, 1):
            wall = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                d.decode(files[rr])
                wall.append((time.perf_counter() - t0) * 1e3)
            r[f"decode_wall_ms_rr{rr}"] = round(med(wall[1:]), 3)
            # (every block of these frames lies inside the component grids: the planes come back whole)
            r[f"round_trip_rr{rr}"] = all((d.component(0, c) == planes[c]).all() for c in range(3))
        d.close()
        res[name] = dict(r, width=W, height=H, quality=q)
    if not a.only:
        print(json.dumps({"what": "mij_decoder_transcode: progressive output vs baseline output of the same planes",
                          "frames": n, "reps": a.reps, "sets": res}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
