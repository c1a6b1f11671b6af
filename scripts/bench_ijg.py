#!/usr/bin/env python3
"""Times encoding as libjpeg does beside the reference's
arithmetic, in one process on the same frames: 64 frames of 3840x2160 of the
config-3 recipe, Q = 50 and 90.

  encode_libjpeg      at 4:4:4, 4:2:2, 4:2:0 and greyscale   (k_ijg_fdct)
  encode_sampled      at 4:4:4, 4:2:2 and greyscale          (k_samp_dct)
  encode_interleaved  at 4:2:0                               (K1)

Per entry: stage [0] of mij_batch_stage_ms (the front end alone) and the
stage total (HIP events; it spans the call's one mid-way wait for the frames'
bit counts where the path has one), median and min/max of --reps after
--warmup; the front end's memory traffic (padded input read once, planes and
DCs written once) over its time; the streams' bytes.

Then what truncation costs, at equal tables: Q = 50 gives the same DQTs on
both quality scales, so the PSNR of mijpeg.decode of both arithmetics'
streams against the source, and their sizes, differ by the arithmetic alone.

Prints one JSON line.  Needs a GPU; there is no CPU fallback.

  python scripts/bench_ijg.py [--frames 64] [--distinct 8] [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--psnr-frames", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_ijg: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    W, H, n = a.width, a.height, a.frames
    W16, H16 = (W + 15) & ~15, (H + 15) & ~15
    distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
    full = torch.stack([torch.from_numpy(distinct[f % len(distinct)]) for f in range(n)]).cuda()
    torch.cuda.synchronize()
    blocks = {"444": 3, "422": 2, "420": 1.5, "gray": 1}  # 8x8 blocks per 64 padded pixels

    def stats(v):
        return {"median": round(float(np.median(v)), 4), "min_max": [round(min(v), 4), round(max(v), 4)]}

    res = {}
    for q in (50, 90):
        b = mijpeg.Batch(W16, H16, n, q)
        b.set_timing(True)
        b.pad_input(full.data_ptr(), full.stride(0), full.stride(1), [(W, H)] * n)
        runs = [("libjpeg", s, lambda s=s: b.encode_libjpeg(n, s, 0)) for s in ("444", "422", "420", "gray")]
        runs += [("reference", s, lambda s=s: b.encode_sampled(n, s, 0)) for s in ("444", "422", "gray")]
        runs += [("reference", "420", lambda: b.encode_interleaved(n, 0))]
        for arith, s, call in runs:
            front, total = [], []
            for i in range(a.warmup + a.reps):
                call()
                st = b.stage_ms()
                if i >= a.warmup:
                    front.append(st[b.STAGES[0]])
                    total.append(st["total"])
            traffic = n * (W16 * H16 * 3 + W16 * H16 / 64 * blocks[s] * 130)
            res[f"q{q}_{arith}_{s}"] = {
                "front_end_ms": stats(front), "total_ms": stats(total),
                "front_end_GB_per_s": round(traffic / np.median(front) / 1e6, 1),
                "bytes": int(b.lengths(n).sum())}
        b.close()
    del full
    torch.cuda.empty_cache()

    # equal tables at Q = 50: what the arithmetic alone changes
    import ijg_model as J
    import foreign_model as FM
    cost, dqts = {}, []
    for s in ("444", "422", "420", "gray"):
        for arith in ("reference", "libjpeg"):
            psnr, size = [], 0
            for f in distinct[:a.psnr_frames]:
                jpg = (mijpeg.encode_libjpeg if arith == "libjpeg" else mijpeg.encode_any)(f, "bgr", 50, 0, s)
                got = mijpeg.decode(jpg, "bgr").astype(np.float64)
                ref = f.astype(np.float64)
                if s == "gray":  # against the luma that went in
                    ref = np.repeat(J.ycc(f)[0][..., None], 3, 2).astype(np.float64)
                psnr.append(10 * np.log10(255.0 ** 2 / np.mean((got - ref) ** 2)))
                size += len(jpg)
                dqts.append(FM.parse(jpg)["dqt"])
            cost[f"{s}_{arith}"] = {"psnr_dB": round(float(np.mean(psnr)), 3), "bytes": size}
    assert all((d[t] == dqts[0][t]).all() for d in dqts for t in d)  # one DQT pair throughout
    print(json.dumps({
        "what": "encode_libjpeg (k_ijg_fdct) beside encode_sampled (k_samp_dct) and encode_interleaved (K1)",
        "frames": n, "width": W, "height": H, "reps": a.reps, "warmup": a.warmup, "encode": res,
        "q50_equal_tables": cost, "psnr_frames": a.psnr_frames}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
