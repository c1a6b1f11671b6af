#!/usr/bin/env python3
"""Times the lossless transforms with the protocol of
scripts/bench_transcode.py (§4h): 64 interleaved streams of 3840x2160 at
Q = 50 made by mij_batch_encode_interleaved in the same process, decoded
once; then, on that one decode, mij_decoder_transcode and
mij_decoder_transform for NONE, FLIP_H, ROT180, TRANSPOSE and ROT90 --
HIP-event time of the call (mij_decoder_transcode_ms), median of --reps after
one untimed call each.  Prints one JSON line.

The stage the transforms add, k_xf_blocks, reads every plane and absolute DC
once and writes them once: "xf_bytes" is that traffic computed from the
geometry.  Its own time comes from a separate kernel-trace run of this script
(rocprofv3 --kernel-trace --stats), not from here.

--transcode-only times mij_decoder_transcode alone and touches none of the
new entry points, and --pkg names the package directory to load (mijpeg.py
and its libmijpeg.so): together they time a checkout of the parent commit
with this same script, for the alternating regression runs of §4i.

Needs a GPU; there is no CPU fallback.

  python scripts/bench_transform.py [--frames 64] [--distinct 8] [--reps 10] [--transcode-only] [--pkg DIR]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--transcode-only", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(REPO, "jpeg-encoder-decoder_amd"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.abspath(a.pkg))
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_transform: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    W, H, n, q = a.width, a.height, a.frames, a.quality
    distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
    med = lambda v: float(np.median(v))

    b = mijpeg.Batch(W, H, n, q)
    full = torch.stack([torch.from_numpy(distinct[f % len(distinct)]) for f in range(n)]).cuda()
    torch.cuda.synchronize()
    b.pad_input(full.data_ptr(), full.stride(0), full.stride(1), [(W, H)] * n)
    b.encode_interleaved(n, 0)
    sources = [b.output(f) for f in range(n)]
    b.close()
    del full
    torch.cuda.empty_cache()

    d = mijpeg.Decoder(W, H, n)
    d.decode(sources)
    calls = [("transcode", lambda: d.transcode(0))]
    if not a.transcode_only:
        for op in ("none", "flip_h", "rot180", "transpose", "rot90"):
            calls.append((op, lambda op=op: d.transform(op)))
    res, streams = {}, {}
    for name, call in calls:
        ms = []
        for _ in range(a.reps + 1):  # the first: allocations, code load
            call()
            ms.append(d.transcode_ms())
        ms = ms[1:]
        streams[name] = d.transcoded(0)
        res[name] = {"ms": round(med(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                     "bytes": int(sum(d.device_transcoded(f)[1] for f in range(n)))}
    out = {"what": "mij_decoder_transform beside mij_decoder_transcode on one decode",
           "lib": mijpeg.LIB_PATH, "frames": n, "width": W, "height": H, "quality": q, "reps": a.reps, "calls": res}
    if not a.transcode_only:
        # what the timed calls wrote, checked on the timed data
        out["none_equals_transcode"] = streams["none"] == streams["transcode"]
        out["rot90_of_frame0_decodes_to"] = list(mijpeg.decode(streams["rot90"]).shape[:2])
        # k_xf_blocks: every block (128 bytes) and absolute DC (2 bytes) read once and written once
        mcus = -(-W // 16) * -(-H // 16)
        blocks = 6 * mcus * n
        out["xf_blocks"] = blocks
        out["xf_bytes"] = 2 * blocks * (128 + 2)
        for op in ("flip_h", "rot180", "transpose", "rot90"):
            res[op]["over_none_ms"] = round(res[op]["ms"] - res["none"]["ms"], 4)
    d.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
