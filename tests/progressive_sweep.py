"""Random legal scan scripts over coefficient planes chosen here (DESIGN.md
§4p): a generator of scripts that are legal by construction under T.81
G.1.1.1, coefficient planes of five kinds of content, and a writer of SOF2
streams for any such script, with tokens from progwrite_model.tokens (pinned
to Pillow's entropy data by tests/test_progwrite_model.py) and optimal tables
from progressive_model._code_lengths.  The planes a stream was written from
are the ground truth of its decode: no decoder is the reference.  cases() is
the fixed list the CPU and the GPU tests share; nothing of it is committed
as a fixture, and since the planes are the truth the tests stay valid if a
numpy release changes what a seed draws."""
import copy

import numpy as np

import progressive_model as PM
import progwrite_model as W

SAMPLINGS = {"grey": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}
KINDS = ("dense", "sparse", "small", "tail", "zero")
MAX_SCANS = PM.MAX_SCANS
ONES = [1] * 64
# DC 1 (a DC of +-1024 stays inside 8 bits), AC 1..4: only for content of +-3
RAMP_A = [1] + [1 + z % 4 for z in range(1, 64)]
RAMP_B = [1] + [1 + (z // 8) % 3 for z in range(1, 64)]


def geometry(w, h, sampling):
    """foreign_model.geometry's dict: luma on DQT 0, chroma on DQT 1"""
    G = W.geometry(w, h, SAMPLINGS[sampling])
    G["comps"] = [(a, b, 1 if c else 0, bw, bh) for c, (a, b, _, bw, bh) in enumerate(G["comps"])]
    return G


def scan_mcus(G, comps):
    """how many MCUs of its own a scan of these components has"""
    if len(comps) == 1:
        gw, gh = PM.grids(G)[comps[0]]
        return gw * gh
    return G["mcus_x"] * G["mcus_y"]


# ---- scripts ----------------------------------------------------------------------
class _State:
    """per component: dc = the DC's Al so far (-1: not coded), dc_plan = the Al its first scan will have; ac[z] and
    plan[z] the same per AC coefficient; bands = the first-pass bands still to come, (Ss, Se, Al)"""

    def __init__(self, ncomp):
        self.dc = [-1] * ncomp
        self.dc_plan = [0] * ncomp
        self.groups = []  # DC first scans still to come
        self.ac = [[-1] * 64 for _ in range(ncomp)]
        self.plan = [[0] * 64 for _ in range(ncomp)]
        self.bands = [[] for _ in range(ncomp)]

    def cost(self):
        """scans that finish the script from here by the plain strategy: every first scan, then per component the
        maximal runs of the highest Al, level by level.  Any other legal move keeps the script finishable; this
        count only says whether it still fits into MAX_SCANS"""
        n = 0
        for c in range(len(self.dc)):
            n += 1 + self.dc_plan[c] if self.dc[c] < 0 else self.dc[c]
            n += len(self.bands[c])
            eff = [a if a >= 0 else p for a, p in zip(self.ac[c], self.plan[c])]
            for level in (1, 2, 3):
                n += sum(1 for z in range(1, 64) if eff[z] >= level and (z == 1 or eff[z - 1] < level))
        return n

    def done(self):
        return self.cost() == 0

    def run(self, c, z):
        """the maximal range of coded AC coefficients around z that share its Al"""
        a, b = z, z
        while a > 1 and self.ac[c][a - 1] == self.ac[c][z]:
            a -= 1
        while b < 63 and self.ac[c][b + 1] == self.ac[c][z]:
            b += 1
        return a, b

    def apply(self, scan):
        comps, ss, se, ah, al = scan
        for c in comps:
            if ss == 0:
                if ah == 0:
                    self.groups = [g for g in self.groups if g != tuple(comps)]
                self.dc[c] = al
            else:
                if ah == 0:
                    self.bands[c] = [b for b in self.bands[c] if b[0] != ss]
                for z in range(ss, se + 1):
                    self.ac[c][z] = al

    def plain(self):
        """the next scan of the plain strategy"""
        if self.groups:
            g = self.groups[0]
            return (g, 0, 0, 0, self.dc_plan[g[0]])
        for c in range(len(self.dc)):
            if self.bands[c]:
                ss, se, al = self.bands[c][0]
                return ((c,), ss, se, 0, al)
        for c in range(len(self.dc)):
            if self.dc[c] > 0:
                return ((c,), 0, 0, self.dc[c], self.dc[c] - 1)
        top = max(max(a[1:]) for a in self.ac)
        for c in range(len(self.dc)):
            for z in range(1, 64):
                if self.ac[c][z] == top:
                    a, b = self.run(c, z)
                    return ((c,), a, b, top, top - 1)
        raise AssertionError("nothing left")

    def draw(self, rng, split):
        """a random legal scan: a DC first scan, a DC refinement of any components that share an Al, an AC first
        scan of a component whose DC is coded, or an AC refinement of a run of one Al or of a part of it"""
        moves = []
        if self.groups:
            moves.append("dc")
        if any(a > 0 for a in self.dc):
            moves.append("dcr")
        if any(self.bands[c] and self.dc[c] >= 0 for c in range(len(self.dc))):
            moves.append("ac")
        if any(a > 0 for row in self.ac for a in row[1:]):
            moves.append("acr")
        move = moves[int(rng.integers(len(moves)))]
        if move == "dc":
            g = self.groups[int(rng.integers(len(self.groups)))]
            return (g, 0, 0, 0, self.dc_plan[g[0]])
        if move == "dcr":
            live = [c for c, a in enumerate(self.dc) if a > 0]
            c = live[int(rng.integers(len(live)))]
            al = self.dc[c]
            comps = tuple(x for x in range(len(self.dc)) if x == c or (self.dc[x] == al and rng.random() < 0.5))
            return (comps, 0, 0, al, al - 1)
        if move == "ac":
            live = [c for c in range(len(self.dc)) if self.bands[c] and self.dc[c] >= 0]
            c = live[int(rng.integers(len(live)))]
            ss, se, al = self.bands[c][int(rng.integers(len(self.bands[c])))]
            return ((c,), ss, se, 0, al)
        live = [(c, z) for c in range(len(self.dc)) for z in range(1, 64) if self.ac[c][z] > 0]
        c, z = live[int(rng.integers(len(live)))]
        a, b = self.run(c, z)
        if rng.random() < split:
            a = int(rng.integers(a, z + 1))
            b = int(rng.integers(z, b + 1))
        al = self.ac[c][z]
        return ((c,), a, b, al, al - 1)


def restart_interval(rng, G, comps):
    """0, 1, 3, one or two rows of the scan's own MCUs, or a count that does not divide the scan (0 where the scan
    has none); without a geometry only the first three"""
    if G is None:
        return int(rng.choice([0, 1, 3]))
    across, nm = W.across(G, list(comps)), scan_mcus(G, comps)
    odd = [r for r in range(2, min(nm, 65536)) if nm % r]
    pick = int(rng.integers(6))
    return [0, 1, 3, across, 2 * across, odd[int(rng.integers(len(odd)))] if odd else 0][pick]


def script(rng, ncomp, G=None):
    """a legal script [(components, Ss, Se, Ah, Al, Ri)] of at most MAX_SCANS scans: the plan (how the DC first scans
    group the components and at which Al 0..3, 1..4 AC bands per component with a first-pass Al 0..3 each) has at
    most 42 scans by the plain strategy; then scans are drawn at random among the legal ones, and a draw that would
    leave too few scans to finish is replaced by the plain strategy's next one, so nothing is drawn and discarded"""
    S = _State(ncomp)
    if ncomp == 1:
        S.groups = [(0,)]
    else:
        S.groups = [[(0, 1, 2)], [(0, 1), (2,)], [(0,), (1, 2)], [(0, 2), (1,)], [(0,), (1,), (2,)]][int(rng.integers(5))]
    for g in S.groups:
        al = int(rng.integers(4))
        for c in g:
            S.dc_plan[c] = al
    for c in range(ncomp):
        cuts = sorted(int(x) for x in rng.choice(np.arange(2, 64), int(rng.integers(4)), replace=False))
        al = int(rng.integers(4))
        for ss, nxt in zip([1] + cuts, cuts + [64]):
            if rng.random() < 0.6:  # else the neighbour's, so that bands merge into one run
                al = int(rng.integers(4))
            S.bands[c].append((ss, nxt - 1, al))
            for z in range(ss, nxt):
                S.plan[c][z] = al
    split = float(rng.choice([0.0, 0.3, 0.7]))
    out = []
    while not S.done():
        scan = S.draw(rng, split)
        T = copy.deepcopy(S)
        T.apply(scan)
        if len(out) + 1 + T.cost() > MAX_SCANS:
            scan = S.plain()
        S.apply(scan)
        out.append(scan + (restart_interval(rng, G, scan[0]),))
    assert len(out) <= MAX_SCANS
    return out


def levels(sc):
    """per scan 1 + the highest level of an earlier scan that shares a component and overlaps its band"""
    out = []
    for k, (comps, ss, se, _, _, _) in enumerate(sc):
        lv = 1
        for (c2, s2, e2, _, _, _), l2 in zip(sc[:k], out):
            if set(comps) & set(c2) and s2 <= se and ss <= e2:
                lv = max(lv, l2 + 1)
        out.append(lv)
    return out


# ---- planes -----------------------------------------------------------------------
def _wide(rng, shape):
    """nonzero values of every magnitude category 1..10 alike, either sign"""
    lo = 1 << rng.integers(0, 10, shape)
    v = np.minimum(lo + (rng.random(shape) * lo).astype(np.int64), 1023)
    return np.where(rng.random(shape) < 0.5, -v, v)


def mask_outside(G, planes, sc):
    """blocks outside a component's own grid keep only what the script codes there: no AC, and of the DC the bits
    that its interleaved DC scans carry (a first scan everything from its Al up, a refinement its one bit)"""
    for c, p in enumerate(planes):
        out = np.setdiff1d(np.arange(len(p)), PM.inside(G, c))
        if len(out):
            keep = 0
            for comps, ss, _, ah, al, _ in sc:
                if ss == 0 and c in comps and len(comps) > 1:
                    keep |= (1 << al) if ah else (-1 << al)
            p[out, 1:] = 0
            p[out, 0] &= keep
    return planes


def planes(rng, G, kind, sc):
    """int16 planes (blocks, 64) per component, zigzag order, absolute DC in [-1024, 1023].  dense: every AC
    coefficient nonzero, half of them +-1023; sparse: 3 % nonzero, up to +-1023; small: 30 % nonzero, +-3; tail:
    only indices 1 (up to +-1023) and 63 (+-7); zero: DC only"""
    out = []
    for _, _, _, bw, bh in G["comps"]:
        n = bw * bh
        p = np.zeros((n, 64), np.int64)
        p[:, 0] = rng.integers(-1024, 1024, n)
        shape = (n, 63)
        if kind == "dense":
            sign = np.where(rng.random(shape) < 0.5, -1, 1)
            p[:, 1:] = np.where(rng.random(shape) < 0.5, 1023 * sign, _wide(rng, shape))
        elif kind == "sparse":
            p[:, 1:] = np.where(rng.random(shape) < 0.03, _wide(rng, shape), 0)
        elif kind == "small":
            v = rng.integers(1, 4, shape) * np.where(rng.random(shape) < 0.5, -1, 1)
            p[:, 1:] = np.where(rng.random(shape) < 0.3, v, 0)
        elif kind == "tail":
            p[:, 1] = np.where(rng.random(n) < 0.7, _wide(rng, n), 0)
            p[:, 63] = np.where(rng.random(n) < 0.7, rng.integers(1, 8, n) * np.where(rng.random(n) < 0.5, -1, 1), 0)
        else:
            assert kind == "zero", kind
        out.append(p)
    return [p.astype(np.int16) for p in mask_outside(G, out, sc)]


# ---- writer -----------------------------------------------------------------------
def scan_tokens(G, coefs, sc):
    """per scan, per restart interval, progwrite_model's tokens"""
    wide = [np.asarray(p).astype(np.int64) for p in coefs]
    return [W.tokens(G, wide, tuple(comps), ss, se, ah, al, ri) for comps, ss, se, ah, al, ri in sc]


def write(G, coefs, sc, dqt, sof_hv=None, toks=None):
    """the SOF2 stream of the planes under the script.  dqt: {Tq: 64 values, zigzag}.  Every scan that reads Huffman
    codes gets tables of its own, optimal for its tokens, defined in front of it under ids 0 (component 0) and 1
    (the others), so a decoder must keep the tables each scan saw.  A DRI is written wherever Ri changes.  sof_hv:
    the sampling factors SOF2 declares for a lone component (in effect it is 1x1 whatever they say)"""
    toks = scan_tokens(G, coefs, sc) if toks is None else toks
    out = bytearray(b"\xff\xd8")
    for tq in sorted(dqt):
        out += PM._seg(0xDB, bytes([tq]) + bytes(int(v) for v in dqt[tq]))
    nc = G["ncomp"]
    sof = bytes([8]) + G["h"].to_bytes(2, "big") + G["w"].to_bytes(2, "big") + bytes([nc])
    for c, (hs, vs, tq, _, _) in enumerate(G["comps"]):
        if sof_hv is not None:
            assert nc == 1
            hs, vs = sof_hv
        sof += bytes([c + 1, (hs << 4) | vs, tq])
    out += PM._seg(0xC2, sof)
    cur_ri = 0
    for (comps, ss, se, ah, al, ri), parts in zip(sc, toks):
        if ri != cur_ri:
            out += PM._seg(0xDD, ri.to_bytes(2, "big"))
            cur_ri = ri
        codes = {}
        for t in sorted({tok[0] for part in parts for tok in part if tok[0] >= 0}):
            freq = {}
            for part in parts:
                for tt, sym, _, _ in part:
                    if tt == t:
                        freq[sym] = freq.get(sym, 0) + 1
            counts, syms = PM._code_lengths(freq)
            # the token's table index is the id for a DC scan; an AC scan's one table goes by its component
            th = t if ss == 0 else (1 if comps[0] else 0)
            out += PM._seg(0xC4, bytes([((1 if ss else 0) << 4) | th]) + bytes(counts) + bytes(syms))
            codes[t] = PM._codes(counts, syms)
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([c + 1, 0x11 if c else 0x00])
        out += PM._seg(0xDA, sos + bytes([ss, se, (ah << 4) | al]))
        for n, part in enumerate(parts):
            if n:
                out += bytes([0xFF, 0xD0 + (n - 1) % 8])
            out += W.entropy(part, codes).replace(b"\xff", b"\xff\x00")
    return bytes(out + b"\xff\xd9")


# ---- the cases --------------------------------------------------------------------
class Case:
    """one frame: its planes (the truth), its script, and lazily its tokens and its stream"""

    def __init__(self, name, sampling, w, h, kind, sc, coefs, dqt, sof_hv=None):
        self.name, self.sampling, self.w, self.h, self.kind = name, sampling, w, h, kind
        self.G = geometry(w, h, sampling)
        self.script, self.coefs, self.dqt, self.sof_hv = sc, coefs, dqt, sof_hv
        self._tokens = self._stream = None

    @property
    def tokens(self):
        if self._tokens is None:
            self._tokens = scan_tokens(self.G, self.coefs, self.script)
        return self._tokens

    @property
    def stream(self) -> bytes:
        if self._stream is None:
            self._stream = write(self.G, self.coefs, self.script, self.dqt, self.sof_hv, self.tokens)
        return self._stream

    @property
    def levels(self):
        return max(levels(self.script))

    def __repr__(self):
        return self.name


def _tables(kind, ncomp):
    """all-ones tables wherever coefficients reach +-1023; two different small ramps for content of +-3 and none"""
    a, b = (RAMP_A, RAMP_B) if kind in ("small", "zero") else (ONES, ONES)
    return {0: a} if ncomp == 1 else {0: a, 1: b}


def _random(name, sampling, w, h, kind, seed, sof_hv=None, ri=None):
    rng = np.random.default_rng(seed)
    G = geometry(w, h, sampling)
    sc = script(rng, G["ncomp"], G)
    if ri is not None:
        sc = [s[:5] + (ri,) for s in sc]
    return Case(name, sampling, w, h, kind, sc, planes(rng, G, kind, sc), _tables(kind, G["ncomp"]), sof_hv)


def _fixed(name, sampling, w, h, kind, sc, seed, edit=None):
    """a script written out here, so that what it is there to show does not hang on a draw"""
    rng = np.random.default_rng(seed)
    G = geometry(w, h, sampling)
    wide = [p.astype(np.int64) for p in planes(rng, G, kind, sc)]
    if edit:
        edit(wide)
    coefs = [p.astype(np.int16) for p in mask_outside(G, wide, sc)]
    return Case(name, sampling, w, h, kind, sc, coefs, _tables(kind, G["ncomp"]))


def _chain(comps, al, ri=0):
    """every component's AC in one band at Al, then refined down to 0 in whole bands"""
    return [((c,), 1, 63, 0, al, ri) for c in comps] + [((c,), 1, 63, a, a - 1, ri) for a in range(al, 0, -1) for c in comps]


def _every_1023(wide):
    for p in wide:
        b = np.arange(len(p))[:, None] + np.arange(63)[None, :]
        p[:, 1:] = np.where(b % 3 == 0, -1023, 1023)


def _dc_swing(wide):
    for p in wide:
        p[:, 0] = np.where(np.arange(len(p)) % 2, 1023, -1024)


def _tail_fixed(wide):
    for p in wide:
        b = np.arange(len(p))
        p[:, 1:] = 0
        p[:, 1] = np.where(b % 2, -1023, 1023) * (b % 5 != 0)
        p[:, 63] = (b % 7 + 1) * np.where(b % 3, 1, -1) * (b % 4 != 0)


SIZES = [(7, 9), (16, 16), (17, 9), (35, 21), (33, 40), (64, 64), (70, 37), (100, 70), (8, 24), (49, 5)]
SEED = 20261021

_cases = None


def cases():
    """the fixed list; built once, shared, left unchanged"""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    for si, sampling in enumerate(SAMPLINGS):
        for ki, kind in enumerate(KINDS):
            for j in range(4):
                w, h = SIZES[(5 * si + ki + 3 * j) % len(SIZES)]
                out.append(_random(f"{sampling}_{kind}_{w}x{h}", sampling, w, h, kind, [SEED, si, ki, j]))
    for si, (sampling, kind) in enumerate(zip(SAMPLINGS, KINDS)):
        out.append(_random(f"{sampling}_{kind}_1x1", sampling, 1, 1, kind, [SEED, 100, si]))
    # 117 restart intervals per luma scan: more than a workgroup of units in one level, and no multiple of 64
    out.append(_random("rst1_grey_sparse_100x70", "grey", 100, 70, "sparse", [SEED, 101], ri=1))
    out.append(_random("rst1_420_small_100x70", "420", 100, 70, "small", [SEED, 102], ri=1))
    # a lone component that SOF2 declares as 2x2
    out.append(_random("grey_h2v2_small_35x21", "grey", 35, 21, "small", [SEED, 103], sof_hv=(2, 2)))
    out.append(_random("grey_h2v2_dense_100x70", "grey", 100, 70, "dense", [SEED, 104], sof_hv=(2, 2)))
    out.append(_random("444_dense_100x70", "444", 100, 70, "dense", [SEED, 105]))
    out.append(_random("420_dense_100x70", "420", 100, 70, "dense", [SEED, 106]))
    # first-pass Al 3 and three refinements of every coefficient: four levels
    dc3 = [((0, 1, 2), 0, 0, 0, 3, 0)] + [((0, 1, 2), 0, 0, a, a - 1, 0) for a in (3, 2, 1)]
    out.append(_fixed("al3_chain_444_dense_35x21", "444", 35, 21, "dense", dc3[:1] + _chain((0, 1, 2), 3) + dc3[1:], [SEED, 107]))
    # refinements that are not a first scan's band: 3-20 straddles 1-5 and 6-63, the rest are parts of one
    straddle = [((0,), 0, 0, 0, 0, 0), ((0,), 1, 5, 0, 1, 0), ((0,), 6, 63, 0, 1, 3), ((0,), 3, 20, 1, 0, 5),
                ((0,), 1, 2, 1, 0, 0), ((0,), 21, 63, 1, 0, 7)]
    out.append(_fixed("straddle_grey_small_33x40", "grey", 33, 40, "small", straddle, [SEED, 108]))
    # all-zero bands without restart intervals: one EOB run of 117 blocks per luma scan, first pass and refinement
    out.append(_fixed("zero_run_420_zero_100x70", "420", 100, 70, "zero", [((0, 1, 2), 0, 0, 0, 0, 0)] + _chain((0, 1, 2), 1),
                      [SEED, 109]))
    # DC first scans of one component each at Al 0 over DCs that swing from -1024 to 1023: differences of category 11
    swing = [((c,), 0, 0, 0, 0, r) for c, r in ((0, 0), (1, 3), (2, 0))] + _chain((0, 1, 2), 0, 4)
    out.append(_fixed("dc_swing_422_sparse_70x37", "422", 70, 37, "sparse", swing, [SEED, 110], _dc_swing))
    # every coefficient of every block at +-1023 in one first pass at Al 0: AC symbols of category 10
    out.append(_fixed("every_1023_grey_dense_64x64", "grey", 64, 64, "dense", [((0,), 0, 0, 0, 0, 0), ((0,), 1, 63, 0, 0, 0)],
                      [SEED, 111], _every_1023))
    # index 1 early and large, index 63 late and small: ZRL chains in the refinements, correction bits in EOB runs
    tail = [((0,), 0, 0, 0, 1, 0)] + _chain((0,), 2) + [((0,), 0, 0, 1, 0, 0)]
    out.append(_fixed("tail_chain_grey_tail_64x64", "grey", 64, 64, "tail", tail, [SEED, 112], _tail_fixed))
    assert len({c.name for c in out}) == len(out)
    _cases = out
    return out


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)
