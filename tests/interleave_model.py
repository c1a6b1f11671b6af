"""Plain numpy model of the interleaved output format (DESIGN.md §4g,
include/mijpeg.h "frames of any size"): edge padding to multiples of 16, the
oracle's coefficient planes of the padded frame, symbol counts in MCU order,
the oracle's table builder, and the bytes -- one interleaved scan, restart
intervals of whole MCU rows, every 0xFF of entropy data stuffed.  Pinned to
foreign_model.py and Pillow by tests/test_interleave_model.py; the kernels
must give these bytes (tests/test_interleave_gpu.py)."""
import numpy as np

import decode_model as M
import oracle as O

APP0 = bytes([0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 0x4A, 0x46, 0x49, 0x46,
              0x00, 0x01, 0x01, 0x00, 0x00, 0x48, 0x00, 0x48, 0x00, 0x00])
SOS = bytes([0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00])


def pad16(frame: np.ndarray) -> np.ndarray:
    """last column, then last row, replicated up to multiples of 16"""
    h, w = frame.shape[:2]
    return np.pad(frame, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge")


def planes(frame_bgr: np.ndarray, quality: int):
    """[Y, Cb, Cr] (blocks, 64) int64 of the padded frame: the oracle's, DC absolute"""
    Y, Cb, Cr, _, _ = O.cref_stages(pad16(frame_bgr), quality)
    out = []
    for p in (Y, Cb, Cr):
        p = p.astype(np.int64).reshape(-1, 64)
        p[:, 0] = np.cumsum(p[:, 0])  # undo the raster-order differences (encoder.c:168-177)
        out.append(p)
    return out


def mag_class(v: int) -> int:
    return int(abs(v)).bit_length()


def mag_bits(v: int, cls: int) -> int:
    return (v if v >= 0 else v - 1) & ((1 << cls) - 1)


def block_symbols(blk, diff):
    """[(table 0 DC / 1 AC, symbol, value bits, bit count)] of one block (T.81 F.1.2)"""
    c = mag_class(diff)
    out = [(0, c, mag_bits(diff, c), c)]
    nz = np.nonzero(blk[1:])[0] + 1
    prev = 0
    for k in nz:
        run = int(k) - prev - 1
        while run >= 16:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        v = int(blk[k])
        c = mag_class(v)
        out.append((1, (run << 4) | c, mag_bits(v, c), c))
        prev = int(k)
    if blk[63] == 0:
        out.append((1, 0x00, 0, 0))
    return out


def mcu_blocks(mw: int, mh: int):
    """(component, block index in its plane) in scan order, per MCU"""
    bw = 2 * mw
    for r in range(mh):
        for c in range(mw):
            yield [(0, (2 * r) * bw + 2 * c), (0, (2 * r) * bw + 2 * c + 1),
                   (0, (2 * r + 1) * bw + 2 * c), (0, (2 * r + 1) * bw + 2 * c + 1),
                   (1, r * mw + c), (2, r * mw + c)]


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.nbytes = 0  # entropy bytes before stuffing, markers apart

    def put(self, v, n):
        for i in range(n - 1, -1, -1):
            self.acc = (self.acc << 1) | ((v >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.nbytes += 1
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc = self.n = 0

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _dht(h, tc_th):
    counts = list(h.code_len_freq[1:17])
    n = sum(counts)
    return bytes([0xFF, 0xC4, (19 + n) >> 8, (19 + n) & 255, tc_th] + counts + [h.sym_sorted[i] for i in range(n)])


class Model:
    def __init__(self, frame_bgr: np.ndarray, quality: int = 50, restart_rows: int = 0):
        frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
        self.h, self.w = h, w = frame_bgr.shape[:2]
        mw, mh = -(-w // 16), -(-h // 16)
        self.ri = ri = restart_rows * mw
        assert 0 <= ri <= 65535
        self.planes = P = planes(frame_bgr, quality)
        # symbols in MCU order; prediction per component, back to 0 at each restart
        syms = []  # per MCU
        self.hist = hist = np.zeros((4, 256), np.int64)  # DC-Y, AC-Y, DC-C, AC-C
        pred = [0, 0, 0]
        for m, blocks in enumerate(mcu_blocks(mw, mh)):
            if ri and m % ri == 0:
                pred = [0, 0, 0]
            cur = []
            for comp, b in blocks:
                blk = P[comp][b]
                for t, s, v, n in block_symbols(blk, int(blk[0]) - pred[comp]):
                    hist[(2 if comp else 0) + t][s] += 1
                    cur.append(((2 if comp else 0) + t, s, v, n))
                pred[comp] = int(blk[0])
            syms.append(cur)
        self.tables = []
        for t in range(4):
            rc, huff = O.cref_build_table(hist[t])
            assert rc == 0, (t, rc)
            self.tables.append(huff)
        lq, cq = O.quality_tables(quality)
        head = bytearray(APP0)
        for t, q in enumerate((lq, cq)):
            head += bytes([0xFF, 0xDB, 0x00, 0x43, t]) + bytes(int(q[z]) for z in M.ZZ)
        for t, tc_th in enumerate((0x00, 0x10, 0x01, 0x11)):
            head += _dht(self.tables[t], tc_th)
        head += bytes([0xFF, 0xC0, 0x00, 0x11, 0x08, h >> 8, h & 255, w >> 8, w & 255, 0x03,
                       0x01, 0x22, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01])
        if ri:
            head += bytes([0xFF, 0xDD, 0x00, 0x04, ri >> 8, ri & 255])
        head += SOS
        bw = _Bits()
        self.interval_starts = [0]  # first byte of each interval in the unstuffed entropy data
        for m, cur in enumerate(syms):
            if ri and m and m % ri == 0:
                bw.pad()
                self.interval_starts.append(bw.nbytes)
                bw.out += bytes([0xFF, 0xD0 + (m // ri - 1) % 8])
            for t, s, v, n in cur:
                T = self.tables[t]
                bw.put(T.sym_code[s], T.sym_code_len[s])
                bw.put(v, n)
        bw.pad()
        self.jpg = bytes(head) + bytes(bw.out) + b"\xff\xd9"


_cache = {}


def model(frame_bgr: np.ndarray, quality: int = 50, restart_rows: int = 0) -> Model:
    """computed once per (frame, quality, restart_rows) and shared; callers leave it unchanged"""
    key = (frame_bgr.shape, frame_bgr.tobytes(), quality, restart_rows)
    m = _cache.get(key)
    if m is None:
        m = _cache[key] = Model(frame_bgr, quality, restart_rows)
    return m


def frame(w: int, h: int, seed: int = 0, kind: str = "photo") -> np.ndarray:
    """seeded (h, w, 3) test frames: "photo" (smooth gradients + detail +
    noise), "noise" (uniform), "flat" (one colour)"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([37, 150, 201], np.uint8), (h, w, 3)).copy()
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 90 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) + 30 * ((x // 5 + y // 3 + c) % 2)
                    for c in range(3)], -1)
    img += rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)
