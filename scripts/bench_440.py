#!/usr/bin/env python3
"""Times the 4:4:0 paths with the protocol of
scripts/bench_transform.py: 64 frames of 3840x2160 at Q = 50 encoded at 4:2:2
(mij_batch_encode_sampled) in the same process, turned into 64 streams of
2160x3840 4:4:0 by this library's own rot90, then

  * mij_decoder_reconstruct_ms (IDCT stages, colour stage) at full size and at
    1/2, 1/4, 1/8 of the 4:4:0 streams beside the 4:2:2 sources, and
  * mij_decoder_transcode_ms of rot90 4:2:2 -> 4:4:0 beside rot90 of the same
    frames encoded at 4:2:0,

each the median of --reps after one untimed call.  "colour_bytes" is what the
colour stage must move, computed from the geometry: every luma and chroma
sample read once (the neighbouring chroma rows a lane reads again come from
the caches) and every pixel row written at its pitch; "colour_tbps" is that
over the colour stage's time.

--regress times only what existed before: the full-size reconstruct of 64
4:2:0 streams, touching none of the new entry points; with MIJ_LIB naming
the parent commit's libmijpeg.so it times that library for the alternating
runs of §4r.

Needs a GPU; there is no CPU fallback.  Prints one JSON line.

  python scripts/bench_440.py [--frames 64] [--distinct 8] [--reps 10] [--regress]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def colour_bytes(w, h, denom, sampling, n):
    """bytes the colour stage reads and writes for n frames decoded at 1/denom"""
    ow, oh = -(-w // denom), -(-h // denom)
    cw, ch = {"422": (-(-ow // 2), oh), "440": (ow, -(-oh // 2)), "420": (-(-ow // 2), -(-oh // 2))}[sampling]
    if sampling == "420" and denom > 1:
        cw, ch = ow, oh  # its chroma is scaled up inside the IDCT
    return n * (ow * oh + 2 * cw * ch + (3 * ow + 15) // 16 * 16 * oh)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--regress", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "jpeg-encoder-decoder_amd"))
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_440: no GPU", file=sys.stderr)
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
    s420 = [b.output(f) for f in range(n)]
    s422 = []
    if not a.regress:
        b.encode_sampled(n, "422", 0)
        s422 = [b.output(f) for f in range(n)]
    b.close()
    del full
    torch.cuda.empty_cache()

    def reconstruct(d, scales, sampling, w, h):
        out = {}
        for scale in scales:
            ms = []
            for _ in range(a.reps + 1):  # the first: allocations, code load
                d.reconstruct("rgb", scale)
                ms.append(d.reconstruct_ms())
            idct, col = [m[0] for m in ms[1:]], [m[1] for m in ms[1:]]
            nbytes = colour_bytes(w, h, scale, sampling, n)
            out[str(scale)] = {"idct_ms": round(med(idct), 4), "colour_ms": round(med(col), 4),
                               "colour_ms_min_max": [round(min(col), 4), round(max(col), 4)],
                               "colour_bytes": nbytes, "colour_tbps": round(nbytes / med(col) / 1e9, 3)}
        return out

    def rot90(d):
        ms = []
        for _ in range(a.reps + 1):
            d.transform("rot90")
            ms.append(d.transcode_ms())
        return {"ms": round(med(ms[1:]), 4), "ms_min_max": [round(min(ms[1:]), 4), round(max(ms[1:]), 4)]}

    out = {"what": "full-size reconstruct of 4:2:0 streams" if a.regress else
           "4:4:0 beside 4:2:2: reconstruct at every scale, rot90 beside rot90 of 4:2:0",
           "lib": mijpeg.LIB_PATH, "frames": n, "width": W, "height": H, "quality": q, "reps": a.reps}
    side = max(W, H)
    if a.regress:
        d = mijpeg.Decoder(W, H, n)
        d.decode(s420)
        out["reconstruct_420"] = reconstruct(d, (1,), "420", W, H)
        d.close()
        print(json.dumps(out))
        return 0
    d = mijpeg.Decoder(side, side, n, accept440=True)
    d.decode(s420)
    out["rot90_420"] = rot90(d)
    out["reconstruct_420"] = reconstruct(d, (1,), "420", W, H)
    d.decode(s422)
    out["reconstruct_422"] = reconstruct(d, (1, 2, 4, 8), "422", W, H)
    out["rot90_422_to_440"] = rot90(d)
    s440 = [d.transcoded(f) for f in range(n)]
    d.decode(s440)
    lay = d.layout(0)
    out["440_layout"] = lay["raw"][:7] + list(lay["comps"][0][:2])
    out["reconstruct_440"] = reconstruct(d, (1, 2, 4, 8), "440", H, W)
    # what the timed calls made, checked on the timed data: the quarter turn back is the source's transcode
    d.transform("rot270")
    back = d.transcoded(0)
    d.decode(s422[:1])
    d.transcode(0)
    out["rot270_of_rot90_is_the_transcode"] = back == d.transcoded(0)
    d.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
