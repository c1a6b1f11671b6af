"""Plain numpy model of lossless transcoding (include/mijpeg.h
mij_decoder_transcode): the coefficient planes, sampling and quantisation
tables of an accepted baseline stream stay as they are; the entropy code is
rebuilt -- one interleaved scan, tables optimised for the counts that scan
emits (the oracle's builder), restart intervals of whole MCU rows of the
source's MCU grid.  Built from foreign_model.py (parsing, geometry,
coefficients), interleave_model.py (block symbols, bit writer, DHT) and
oracle.cref_build_table.  Pinned to independent code by
tests/test_transcode_model.py; the kernels must give these bytes
(tests/test_transcode_gpu.py)."""
import numpy as np

import foreign_model as FM
import interleave_model as IM
import oracle as O


def build(w, h, comps, hv, dqt, planes, restart_rows):
    """comps: SOF0 entries (id, H/V byte, Tq) verbatim; hv: the sampling in
    effect per component (a lone component is 1x1); dqt: {id: 64 bytes};
    planes: per component (blocks, 64) with absolute DCs, padded to whole MCUs"""
    nc = len(comps)
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    ri = restart_rows * mx
    if restart_rows < 0 or ri > 65535:
        raise ValueError(f"restart interval {ri}")
    nm = mx * my
    hist = np.zeros((4, 256), np.int64)  # DC/AC of component 0, DC/AC of components 1 and 2 together
    syms = []
    pred = [0] * nc
    for m in range(nm):
        if ri and m % ri == 0:
            pred = [0] * nc
        r, c = divmod(m, mx)
        cur = []
        for k, (a, b) in enumerate(hv):
            t0 = 2 if k else 0
            for j in range(a * b):
                blk = planes[k][(r * b + j // a) * (mx * a) + c * a + j % a]
                for t, s, v, n in IM.block_symbols(blk, int(blk[0]) - pred[k]):
                    hist[t0 + t][s] += 1
                    cur.append((t0 + t, s, v, n))
                pred[k] = int(blk[0])
        syms.append(cur)
    ntab = 4 if nc > 1 else 2  # a one-component frame builds and writes only the first two
    tables = []
    for t in range(ntab):
        rc, huff = O.cref_build_table(hist[t])
        assert rc == 0, (t, rc)
        tables.append(huff)
    head = bytearray(IM.APP0)
    for tq in sorted(set(c[2] for c in comps)):
        head += bytes([0xFF, 0xDB, 0x00, 0x43, tq]) + bytes(int(x) for x in dqt[tq])
    for t, tc_th in enumerate((0x00, 0x10, 0x01, 0x11)[:ntab]):
        head += IM._dht(tables[t], tc_th)
    n = 8 + 3 * nc
    head += bytes([0xFF, 0xC0, n >> 8, n & 255, 8, h >> 8, h & 255, w >> 8, w & 255, nc])
    for cid, hvb, tq in comps:
        head += bytes([cid, hvb, tq])
    if restart_rows > 0:
        head += bytes([0xFF, 0xDD, 0x00, 0x04, ri >> 8, ri & 255])
    head += bytes([0xFF, 0xDA, 0x00, 6 + 2 * nc, nc])
    for k, (cid, _, _) in enumerate(comps):
        head += bytes([cid, 0x11 if k else 0x00])
    head += bytes([0x00, 0x3F, 0x00])
    bw = IM._Bits()
    for m, cur in enumerate(syms):
        if ri and m and m % ri == 0:
            bw.pad()
            bw.out += bytes([0xFF, 0xD0 + (m // ri - 1) % 8])
        for t, s, v, nb in cur:
            T = tables[t]
            bw.put(T.sym_code[s], T.sym_code_len[s])
            bw.put(v, nb)
    bw.pad()
    return bytes(head) + bytes(bw.out) + b"\xff\xd9"


_cache = {}


def model(jpg: bytes, restart_rows: int = 0) -> bytes:
    """the transcoded stream of a one-scan (interleaved or greyscale) source;
    computed once per (stream, restart_rows) and shared"""
    key = (jpg, restart_rows)
    out = _cache.get(key)
    if out is None:
        P = FM.parse(jpg)
        G = FM.geometry(P)
        planes = [p.astype(np.int64) for p in FM.coefficients(P, G)]
        comps = [(c[0], (c[1] << 4) | c[2], c[3]) for c in P["comps"]]
        hv = [(c[0], c[1]) for c in G["comps"]]
        dqt = {k: [int(x) for x in v] for k, v in P["dqt"].items()}
        out = _cache[key] = build(P["w"], P["h"], comps, hv, dqt, planes, restart_rows)
    return out


def model_legacy(frame_bgr: np.ndarray, quality: int, restart_rows: int = 0) -> bytes:
    """the transcoded stream of the three-scan stream the oracle (and
    mijpeg.encode) writes for a frame whose sides are multiples of 16:
    foreign_model.parse refuses its second scan, so the planes are the
    oracle's own, as interleave_model.planes takes them"""
    frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
    key = (frame_bgr.shape, frame_bgr.tobytes(), quality, restart_rows)
    out = _cache.get(key)
    if out is None:
        h, w = frame_bgr.shape[:2]
        assert w % 16 == 0 and h % 16 == 0
        lq, cq = O.quality_tables(quality)
        import decode_model as M
        dqt = {0: [int(lq[z]) for z in M.ZZ], 1: [int(cq[z]) for z in M.ZZ]}
        comps = [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
        out = _cache[key] = build(w, h, comps, [(2, 2), (1, 1), (1, 1)], dqt, IM.planes(frame_bgr, quality),
                                  restart_rows)
    return out
