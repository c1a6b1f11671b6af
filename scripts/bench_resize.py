#!/usr/bin/env python3
"""Times the resampler and prints one JSON line.

Resize alone: 64 device frames of 1920x1080 and of 480x270 to 256x144, per
filter, with the resizer's own HIP events (mij_resizer_ms: horizontal,
vertical).  Beside the times, the bytes each pass has to move, computed from
the shapes (source and intermediate rows read, intermediate and output rows
written), that traffic over the time as a share of the HBM peak, and the
intermediate's share of the traffic: what a fused kernel could save.

Thumbnail chain: 64 stored 3840x2160 streams (the config-3 recipe's frames,
Q = 50) to 256x144 JPEGs: decode, reconstruct at 1/8, resize 480x270 ->
256x144, pad + encode, on the decoder's stream; against the existing 1/8
chain without the resize (480x270 JPEGs), alternating, in the same process.

  python scripts/bench_resize.py [--frames 64] [--distinct 8] [--reps 10]

Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "jpeg-encoder-decoder_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

HBM_PEAK = 8.0e12  # bytes / s


def pass_bytes(w, h, ow, oh):
    """bytes the two passes read and written, from the shapes: the source once,
    the intermediate (h rows of ow pixels) written and read, the output once"""
    src, mid, out = 3 * w * h, 3 * ow * h, 3 * ow * oh
    return {"h_read": src, "h_written": mid, "v_read": mid, "v_written": out}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="256x144")
    ap.add_argument("--skip-chain", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch  # its HIP runtime before the library's, as bench.py does

    if not torch.cuda.is_available():
        print("bench_resize: no GPU", file=sys.stderr)
        return 1
    torch.cuda.set_device(0)
    import mijpeg
    import recipes

    n = a.frames
    ow, oh = (int(v) for v in a.out.split("x"))
    med = lambda v: float(np.median(v))
    out = {"what": "mij_resizer_resize alone, and the stored-JPEG thumbnail chain with and without it",
           "frames": n, "out": [ow, oh], "reps": a.reps, "resize": {}, "chain": {}}

    r = mijpeg.Resizer(n)
    for w, h in ((1920, 1080), (480, 270)):
        distinct = [np.ascontiguousarray(recipes.config3_frame(f, h, w)) for f in range(min(a.distinct, n))]
        dev = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        for f in range(n):
            dev[f] = torch.from_numpy(distinct[f % len(distinct)])
        torch.cuda.synchronize()
        images = [(dev[f].data_ptr(), 3 * w, w, h) for f in range(n)]
        by = pass_bytes(w, h, ow, oh)
        total = sum(by.values())
        row = {"bytes_per_frame": by, "intermediate_share_of_traffic": round((by["h_written"] + by["v_read"]) / total, 4)}
        for f in mijpeg.RS_FILTERS:
            r.resize(images, [(ow, oh)] * n, f)  # warm-up: allocates, loads the code
            r.ms()
            hs, vs = [], []
            for _ in range(a.reps):
                r.resize(images, [(ow, oh)] * n, f)
                t = r.ms()
                hs.append(t[0])
                vs.append(t[1])
            hm, vm = med(hs), med(vs)
            row[f] = {"h_ms": round(hm, 4), "v_ms": round(vm, 4), "h_ms_min_max": [round(min(hs), 4), round(max(hs), 4)],
                      "v_ms_min_max": [round(min(vs), 4), round(max(vs), 4)],
                      "h_tb_s": round(n * (by["h_read"] + by["h_written"]) / (hm * 1e-3) / 1e12, 3),
                      "v_tb_s": round(n * (by["v_read"] + by["v_written"]) / (vm * 1e-3) / 1e12, 3),
                      "share_of_hbm_peak": round(n * total / ((hm + vm) * 1e-3) / HBM_PEAK, 4)}
        out["resize"][f"{w}x{h}"] = row
        del dev

    if not a.skip_chain:
        W, H = 3840, 2160
        distinct = [np.ascontiguousarray(recipes.config3_frame(f, H, W)) for f in range(min(a.distinct, n))]
        b = mijpeg.Batch(W, H, n, 50)
        for f in range(n):
            b.upload(distinct[f % len(distinct)], first=f)
        b.encode(n)
        streams = [b.output(f) for f in range(n)]
        b.close()
        d = mijpeg.Decoder(W, H, n)
        sw, sh = W // 8, H // 8
        enc_small = mijpeg.Batch((ow + 15) // 16 * 16, (oh + 15) // 16 * 16, n, 75)
        enc_eighth = mijpeg.Batch((sw + 15) // 16 * 16, (sh + 15) // 16 * 16, n, 75)
        r.set_stream(d.stream_ptr())
        enc_small.set_stream(d.stream_ptr())
        enc_eighth.set_stream(d.stream_ptr())

        def frames_of(obj):
            p0, pitch = obj.device_pixels(0)
            stride = obj.device_pixels(1)[0] - p0 if n > 1 else 0
            assert all(obj.device_pixels(f)[0] == p0 + f * stride for f in range(n))
            return p0, stride, pitch

        def chain(resize):
            t0 = time.perf_counter()
            d.decode(streams)  # synchronous: upload and entropy decode
            t1 = time.perf_counter()
            d.reconstruct("bgr", scale=8)
            p0, stride, pitch = frames_of(d)
            if resize:
                r.resize([(p0 + f * stride, pitch, sw, sh) for f in range(n)], [(ow, oh)] * n, "bicubic")
                q0, qstride, qpitch = frames_of(r)
                enc_small.pad_input(q0, qstride, qpitch, [(ow, oh)] * n)
                enc_small.encode_interleaved(n, 0)
                enc_small.sync()
            else:
                enc_eighth.pad_input(p0, stride, pitch, [(sw, sh)] * n)
                enc_eighth.encode_interleaved(n, 0)
                enc_eighth.sync()
            t2 = time.perf_counter()
            rec = sum(d.reconstruct_ms())
            rs = sum(r.ms()) if resize else 0.0
            return {"decode_ms": (t1 - t0) * 1e3, "rest_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3,
                    "reconstruct_ms": rec, "resize_ms": rs}

        chain(True), chain(False)  # warm-up
        runs = {True: [], False: []}
        for _ in range(a.reps):
            for resize in (True, False):
                runs[resize].append(chain(resize))
        for resize, name in ((True, "eighth_then_resize_256x144"), (False, "eighth_only_480x270")):
            out["chain"][name] = {k: round(med([x[k] for x in runs[resize]]), 4) for k in runs[resize][0]}
            tot = [x["total_ms"] for x in runs[resize]]
            out["chain"][name]["total_ms_min_max"] = [round(min(tot), 3), round(max(tot), 3)]
        small = enc_small.output(0)
        assert mijpeg.decode(small).shape == (oh, ow, 3)
        for o in (enc_small, enc_eighth):
            o.set_stream(0)
            o.close()
        r.set_stream(0)
        d.close()
    r.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
