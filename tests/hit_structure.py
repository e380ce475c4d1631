"""Scenes and queries aimed at the STRUCTURE pm_hit_kernel walks (test helper, not a conftest): tests/test_hit_structure.py runs them
against tests/np_hit.py under the emulation and on the GPU, and checks on the CPU that every scene reaches the edge it names.

The kernel (piet_metal_amd/csrc/pm_hit_test.h) walks the items WAVE at a time from the top of paint order, and reaches a Fill's or a
Polyline's segments through the scene index: chunks of CHUNK_SEGS segments, super-chunks of SUPER_CHUNKS consecutive entries of the
GLOBAL chunk table.  An item of up to WAVE chunks takes one round; a longer one has its super-chunks tested WAVE per round and the
survivors worked off eight at a time.  The builders below choose item sizes by chunk and super-chunk count, put a lead item in front
(so that the long item's first chunk is at any residue of SUPER_CHUNKS) and a trailing item behind (so that its last super-chunk is
shared), and make queries whose answer depends on few segments each:

  loops_scene  a plain Fill of n loops -- a full-height stroke at r_k, the return stroke far to the left -- with 0, 1 or 2 extra points
               on the bottom line before every loop, so that chunks and super-chunks hold irregular numbers of counted strokes
               (even-odd); under the non-zero rule a square wave of strokes up and down in turn, whose winding stays 0 or +-1;
  comb_scene   a compound Fill of n thin full-height rectangles, five entries each: separators and closing segments at every
               residue of a chunk;
  fan_scene    a Polyline that alternates between a centre and rim points: every segment's box has the centre as a corner, so a
               query on a spoke passes the boxes of many super-chunks and is within half the width of one spoke only;
  walk_scene   n items of every kind, a private spot each, and a common point that every non-circle item covers.

index_model() restates pm_index_kernel's boxes in numpy and Contributions evaluates np_hit's own pair functions per chunk; with
them losses() tells for a set of lost chunks whether any query's answer would change -- the CPU check that the inputs are not blind."""
from __future__ import annotations

import struct

import numpy as np

import np_hit

CHUNK_SEGS = 4     # kChunkSegs   (piet_metal_amd/csrc/pm_device.h)
SUPER_CHUNKS = 8   # kSuperChunks
WAVE = 64          # items per step of the walk; chunks and super-chunks per round
NONE = 0xFFFFFFFF  # PM_HIT_NONE

F32 = np.float32


def f32_neighbours(v):
    """[below, v, above] as float32."""
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


class Case:
    """A scene, its queries, and where its long item is."""

    def __init__(self, name, scene, queries, long_item=None, **facts):
        self.name, self.scene, self.long_item, self.facts = name, scene, long_item, facts
        self.queries = np.ascontiguousarray(queries, F32).reshape(-1, 2)

    def __repr__(self):
        return self.name


def _encode(pm, n_root, emit, cap=1 << 18):
    buf = np.zeros(cap, np.uint8)
    e = pm.Encoder(buf)
    e.begin_group(n_root)
    emit(e)
    e.end_group()
    out = buf[: e.bytes_used].copy()
    e.close()
    return out


# ---- A. one long item between a lead and a trailing item ---------------------------------------------------------

L, T, B = 10.0, 40.0, 360.0   # the return strokes' x; the strokes' two ends in y (T < B: a query at y = T is inside, at y = B outside)
R0 = 100.0                    # x of the first stroke
MID = 200.0
BUMP = 8.0                    # the prefix points zigzag between y = B and y = B + BUMP: the only segments below B


def lead_points(lead):
    """A small polygon of `lead` points left of the strokes: ceil(lead / 4) chunks in front of the long item."""
    k = np.arange(lead)
    return np.stack([60.0 + 8.0 * np.cos(2 * np.pi * k / lead), MID + 8.0 * np.sin(2 * np.pi * k / lead)], axis=1)


def trailing_points(x):
    """A thin triangle right of x over the strokes' whole height: its box shares their rows."""
    return np.array([[x + 20.0, T], [x + 24.0, T], [x + 22.0, B]])


def _rows(xs, heights):
    xs = np.asarray(xs, F32)
    return np.concatenate([np.stack([xs, np.full(len(xs), h, F32)], axis=1) for h in heights])


def _edge_heights():
    return f32_neighbours(T) + f32_neighbours(B)


def _extras(rng, n, want):
    """n counts of 0, 1 or 2 extra points from the generator -- moved, if `want` is given, until they sum to it."""
    extras = rng.integers(0, 3, n)
    if want is not None:
        assert 0 <= want <= 2 * n, (want, n)
        order = rng.permutation(n)
        for k in order:
            if extras.sum() < want and extras[k] < 2:
                extras[k] += min(2 - extras[k], want - extras.sum())
        for k in order:
            if extras.sum() > want and extras[k] > 0:
                extras[k] -= min(extras[k], extras.sum() - want)
        assert extras.sum() == want
    return extras


def _prefix(x0, step, prefix):
    """`prefix` points after (x0, B), in turn below the bottom line and on it: a chunk of nothing but leading points still holds
    segments that count for the queries of _bump_queries."""
    return [(x0 + step * (j + 1), B if j % 2 else B + BUMP) for j in range(prefix)]


def _bump_queries(x0, step, prefix):
    if not prefix:
        return np.zeros((0, 2), F32)
    lo, hi = sorted((x0, x0 + step * (prefix + 1)))
    return _rows(np.arange(lo - 1.25, hi + 1.5, 0.5), [B + 2.0, B + 4.0, B + 6.0])


def loops_points(n, prefix, seed, npt=None):
    """Point 0 is (L, B), then `prefix` leading points, then n loops of four points -- (r, B) (r, T) (L, T) (L, B) -- each after 0, 1
    or 2 extra points on y = B; the last loop leaves its last point out, so the CLOSING segment is its return stroke.  Horizontal
    segments add nothing (D13) and the return strokes lie left of the queries, so the winding of a query between two strokes is
    the number of loops to its right, and every chunk and super-chunk to its right passes the box tests.  The irregular extra
    points are what lets the even-odd rule see an even number of lost chunks.  npt: the exact point count wanted."""
    rng = np.random.default_rng([seed, n, prefix])
    extras = _extras(rng, n, None if npt is None else npt - (prefix + 4 * n))
    pts = [(L, B)] + _prefix(L, 2.0, prefix)
    xs = R0 + 0.25 * np.arange(n)
    for k in range(n):
        pts += [(30.0 + 3.0 * j + (k % 7), B) for j in range(int(extras[k]))]
        pts += [(float(xs[k]), B), (float(xs[k]), T), (L, T), (L, B)]
    pts = np.array(pts[:-1])
    assert npt is None or len(pts) == npt
    return pts, xs


def meander_points(n, prefix, seed, npt=None):
    """The non-zero rule's long Fill.  Under it the loops' winding, which only grows to the left, could lose any number of strokes
    unseen; here the strokes go up and down in turn, so the winding of every query is 0 or +-1 and a lost stroke shows under either
    rule.  Point 0 is (RR, B) right of everything, then `prefix` leading points, then a square wave over n strokes (n odd) at r_k
    = R0 + k / 4 -- up at r_0, along y = T, down at r_1, along y = B, ... -- with 0, 1 or 2 extra points in the horizontal run
    before every stroke, then (RR, T); the CLOSING segment is the stroke down at RR."""
    assert n % 2 == 1
    rng = np.random.default_rng([seed, n, prefix, 1])
    extras = _extras(rng, n, None if npt is None else npt - (prefix + 2 * n + 2))
    xs = R0 + 0.25 * np.arange(n)
    rr = float(xs[-1]) + 2.0
    pts = [(rr, B)] + _prefix(rr + 12.0, -2.0, prefix)
    for k in range(n):
        y = T if k % 2 else B   # the run before stroke k is on this line
        x0 = 90.0 if k == 0 else float(xs[k - 1])
        pts += [(x0 + (3.0 if k == 0 else 0.0625) * (j + 1), y) for j in range(int(extras[k]))]
        pts += [(float(xs[k]), y), (float(xs[k]), B if k % 2 else T)]
    pts = np.array(pts + [(rr, T)])
    assert npt is None or len(pts) == npt
    return pts, xs


def _stroke_queries(xs, between, right_end, seed):
    """Between the strokes at mid height and at T, B and their f32 neighbours; on every stroke and its f32 neighbours at a height
    strictly inside; left of, on and next to the return strokes; uniform points."""
    rng = np.random.default_rng([seed, 9])
    on = np.concatenate([np.array(f32_neighbours(x), F32) for x in xs])
    left = np.array([5.0] + f32_neighbours(L), F32)
    uni = rng.uniform(0.0, 1.0, (300, 2)) * (right_end + 40.0, B - T + 40.0) + (0.0, T - 20.0)
    return np.concatenate([_rows(between, [MID]), _rows(between, _edge_heights()), _rows(on, [123.456]),
                           _rows(left, [MID, T, 123.456]), uni.astype(F32)])


def meander_strokes(n, npt=None):
    """Strokes of the meander that stands in for n loops: about as many points -- two a stroke against four a loop --, an odd number."""
    return 2 * (3 * n // 4) + 1 if npt is None else 2 * (npt // 6) + 1


def loops_scene(pm, n, prefix=0, lead=3, even_odd=True, npt=None, seed=1):
    """Even-odd: n loops.  Non-zero: the meander of meander_strokes(n, npt) strokes."""
    if even_odd:
        pts, xs = loops_points(n, prefix, seed, npt=npt)
        right, bump = float(xs[-1]), _bump_queries(L, 2.0, prefix)
    else:
        pts, xs = meander_points(meander_strokes(n, npt), prefix, seed, npt=npt)
        right = float(xs[-1]) + 2.0
        bump = np.concatenate([_bump_queries(right + 12.0, -2.0, prefix), _rows(f32_neighbours(right) + [right - 1.0, right + 1.0], [MID, T])])

    def emit(e):
        e.fill(lead_points(lead), 0x336699FF)
        e.fill(pts, 0xAA5500FF, even_odd=even_odd)
        e.fill(trailing_points(right), 0x2244CCFF)

    between = np.concatenate([[xs[0] - 0.125], xs + 0.125])
    name = f"{'loops' if even_odd else 'meander'} n={len(xs)} npt={len(pts)} prefix={prefix} lead={lead} {'even-odd' if even_odd else 'non-zero'}"
    return Case(name, _encode(pm, 3, emit), np.concatenate([_stroke_queries(xs, between, right, seed), bump]), long_item=1, npt=len(pts))


def comb_scene(pm, n, lead=3, even_odd=False, entries=None, seed=2):
    """Sub-path k is the rectangle [r_k, r_k + 1/8] x [T, B] from (r, T): top, the stroke down at r + 1/8, bottom, and the CLOSING
    stroke up at r, whose target point the separator names; a seeded subset is wound the other way, from (r + 1/8, T), so that its
    closing segment is a stroke too.  Five entries a sub-path against four a chunk: separators and closing segments fall on every
    residue.  entries: the exact entry count wanted, reached by a fifth point in the middle of a stroke of some sub-paths."""
    rng = np.random.default_rng([seed, n])
    xs = R0 + 0.5 * np.arange(n)
    w = 0.125
    flip = rng.integers(0, 2, n).astype(bool)
    more = np.zeros(n, bool)
    more[rng.permutation(n)[: (entries or 5 * n) - 5 * n]] = True
    subs = []
    for r, f, m in zip(xs, flip, more):
        rect = [(r + w, T), (r, T), (r, B), (r + w, B)] if f else [(r, T), (r + w, T), (r + w, B), (r, B)]
        if m:
            rect.insert(2, (rect[1][0], MID + 17.0))
        subs.append(np.array(rect))
    right = float(xs[-1] + w)
    assert sum(len(s) + 1 for s in subs) == (entries or 5 * n)

    def emit(e):
        e.fill(lead_points(lead), 0x336699FF)
        e.fill_compound(subs, 0xAA5500FF, even_odd=even_odd)
        e.fill(trailing_points(right), 0x2244CCFF)

    between = np.concatenate([[xs[0] - 0.25], xs + 0.3125])
    inside = xs + 0.0625
    q = np.concatenate([_stroke_queries(np.concatenate([xs, xs + w]), between, right, seed), _rows(inside, [MID, MID + 30.0]),
                        _rows(inside, _edge_heights())])
    name = f"comb n={n} entries={entries or 5 * n} lead={lead} {'even-odd' if even_odd else 'non-zero'}"
    return Case(name, _encode(pm, 3, emit), q, long_item=1, npt=entries or 5 * n)


FAN_C = (20.0, 20.0)
FAN_WIDTH = 0.25


def fan_points(n):
    """C, rim_0, C, rim_1, ... rim_(n-1): 2 n - 1 segments; the rim at radius 400 over a quarter turn, snapped to 1/64."""
    th = np.linspace(0.0, np.pi / 2, n)
    rim = np.round((np.array(FAN_C) + 400.0 * np.stack([np.cos(th), np.sin(th)], axis=1)) * 64.0) / 64.0
    pts = np.empty((2 * n, 2))
    pts[0::2] = FAN_C
    pts[1::2] = rim
    return pts, rim


def fan_scene(pm, n, lead=3, seed=3):
    """Items: a wide Polyline along the diagonal, the lead Fill, the fan, the trailing Fill."""
    pts, rim = fan_points(n)
    hw = FAN_WIDTH / 2
    wide = np.array([[30.0, 30.0], [150.0, 150.0], [300.0, 300.0]])

    def emit(e):
        e.polyline(wide, 0x11AA22FF, 24.0)
        e.fill(lead_points(lead) + (200.0, 100.0), 0x336699FF)
        e.polyline(pts, 0xAA5500FF, FAN_WIDTH)
        e.fill(np.array([[430.0, 10.0], [434.0, 10.0], [432.0, 430.0]]), 0x2244CCFF)

    c = np.array(FAN_C)
    on10, on30, on75 = c + 0.10 * (rim - c), c + 0.30 * (rim - c), c + 0.75 * (rim - c)
    mid75 = 0.5 * (on75[:-1] + on75[1:])
    # exactly hw right of / below a rim point and of C's other sides: hits ON the widened boxes' edges (every sum exact in f32), and
    # one f32 step out
    edge = []
    for p in rim:
        edge += [(x, p[1]) for x in f32_neighbours(p[0] + hw)] + [(p[0], y) for y in f32_neighbours(p[1] + hw)]
    edge += [(x, c[1]) for x in f32_neighbours(c[0] - hw)] + [(c[0], y) for y in f32_neighbours(c[1] - hw)]
    rng = np.random.default_rng([seed, n])
    uni = rng.uniform(0.0, 440.0, (300, 2))
    q = np.concatenate([on10, on30, on75, mid75, rim, np.array(edge), uni])
    return Case(f"fan n={n} lead={lead}", _encode(pm, 4, emit), q, long_item=2, npt=2 * n)


LOOPS_CASES = [
    # (n, prefix, lead, npt)          chunks = ceil(npt / 4); lead chunks = ceil(lead / 4)
    (64, 0, 3, None), (65, 1, 9, None), (128, 2, 19, None), (513, 3, 28, None), (1030, 0, 32, None),
    (51, 1, 28, 256),     # exactly 64 chunks: the last item that takes one round
    (51, 2, 32, 257),     # exactly 65 chunks, the last one the closing segment alone
    (410, 0, 32, 2048),   # exactly 512 chunks from a multiple of eight: 64 super-chunks, one round of them, full
    (410, 3, 28, 2048),   # ... from residue 7: 65 super-chunks, the first and the last shared
    (410, 1, 32, 2049),   # exactly 513 chunks: the 65th super-chunk holds one chunk of one segment
]
COMB_SIZES = [(51, 3, 256), (51, 28, 260), (103, 9, None), (409, 32, 2048), (409, 28, 2050), (830, 19, None)]   # (sub-paths, lead, entries or 5 per sub-path)
FAN_SIZES = [(128, 3), (129, 28), (1025, 24), (1030, 19)]                    # (spokes, lead): 255 / 257 / 2 049 / 2 059 segments


def structure_cases():
    """[(id, builder(pm) -> Case)] of part A."""
    out = []
    for n, prefix, lead, npt in LOOPS_CASES:
        for eo in (True, False):
            # (the id names the case's own size: loops, or the meander's strokes)
            ident = f"loops-{n}-{npt or 'free'}-p{prefix}-l{lead}-eo" if eo else f"meander-{meander_strokes(n, npt)}-{npt or 'free'}-p{prefix}-l{lead}-nz"
            out.append((ident, lambda pm, a=(n, prefix, lead, eo, npt): loops_scene(pm, a[0], a[1], a[2], a[3], a[4])))
    for n, lead, entries in COMB_SIZES:
        for eo in (False, True):
            out.append((f"comb-{entries or 5 * n}-l{lead}-{'eo' if eo else 'nz'}", lambda pm, a=(n, lead, eo, entries): comb_scene(pm, *a)))
    for n, lead in FAN_SIZES:
        out.append((f"fan-{n}-l{lead}", lambda pm, a=(n, lead): fan_scene(pm, *a)))
    return out


# ---- B. the index restated, and what a query would answer if chunks were lost ----------------------------------------

def _item_header(sc, at):
    tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
    flags = struct.unpack_from("<I", sc, at + 4)[0] if tag == np_hit.FILL else 0
    return tag, flags


def _entries(sc, at):
    """(entry index, a, b) of the segments of a Fill or Polyline item: entry k is what the kernel calls segment k (a compound Fill's
    separators are entries without a segment)."""
    tag, flags = _item_header(sc, at)
    if tag == np_hit.FILL:
        pts = np_hit._points(sc, at)
        a, b = np_hit.fill_segments(pts, bool(flags & np_hit.FILL_COMPOUND))
        ent = np.flatnonzero(~np.isnan(pts[:, 0])) if flags & np_hit.FILL_COMPOUND else np.arange(len(pts))
        return ent, a, b, len(pts)
    if tag == np_hit.POLY:
        a, b, _ = np_hit.stroke_segments(sc, at, tag)
        n = len(np_hit._points(sc, at))
        if n < 2:
            return np.zeros(0, np.int64), a[:0], b[:0], 0
        return np.arange(n - 1), a, b, n - 1
    return np.zeros(0, np.int64), np.zeros((0, 2)), np.zeros((0, 2)), 0


def index_model(scene):
    """(chunk_base [n_items + 1], chunk_bbox [n_chunks, 4], sup_bbox [n_sup, 4]) as pm_index_kernel leaves them: float32 boxes
    {xmin, ymin, xmax, ymax}; a plain Fill's and a Polyline's chunk is the box of its points k0 .. k1, a compound Fill's that of the
    segments that exist; a super-chunk's the union of eight consecutive entries of the whole table.
    A restatement: the library hands its index to no caller, so nothing compares the two tables.  What ties the CPU checks to the
    real index is the constants test and, on the kernel's side, the equality with np_hit of queries exactly on these boxes' edges."""
    sc = bytes(scene)
    items = np_hit.flat_items(sc)
    base, boxes = [0], []
    for at, _ in items:
        ent, a, b, nent = _entries(sc, at)
        tag, flags = _item_header(sc, at)
        nch = -(-nent // CHUNK_SEGS)
        base.append(base[-1] + nch)
        compound = bool(flags & np_hit.FILL_COMPOUND)
        pts = np_hit._points(sc, at).astype(np.float64) if nent else None
        for j in range(nch):
            k0, k1 = CHUNK_SEGS * j, min(CHUNK_SEGS * (j + 1), nent)
            if compound:
                sel = (ent >= k0) & (ent < k1)
                p = np.concatenate([a[sel], b[sel]])
            else:
                p = pts[[k % len(pts) for k in range(k0, k1 + 1)]]
            boxes.append((p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()) if len(p) else (3.0e38, 3.0e38, -3.0e38, -3.0e38))
    chunk = np.array(boxes, np.float64).reshape(-1, 4)
    n_sup = -(-len(chunk) // SUPER_CHUNKS)
    pad = np.tile([3.0e38, 3.0e38, -3.0e38, -3.0e38], (n_sup * SUPER_CHUNKS - len(chunk), 1))
    g = np.concatenate([chunk, pad]).reshape(n_sup, SUPER_CHUNKS, 4)
    sup = np.concatenate([g[:, :, :2].min(axis=1), g[:, :, 2:].max(axis=1)], axis=1)
    return np.array(base, np.int64), chunk.astype(F32), sup.astype(F32)


class Contributions:
    """Of one Fill or Polyline item to a list of queries, per chunk of the item: the winding sum of the chunk's segments (Fill) or
    the number of them within half the width (Polyline), by np_hit's own pair functions."""

    def __init__(self, scene, item, queries):
        sc = bytes(scene)
        at, _ = np_hit.flat_items(sc)[item]
        tag, flags = _item_header(sc, at)
        self.fill = tag == np_hit.FILL
        self.even_odd = bool(flags & np_hit.FILL_EVEN_ODD)
        ent, a, b, nent = _entries(sc, at)
        self.hw = None if self.fill else float(np_hit.stroke_segments(sc, at, tag)[2])
        self.n_chunks = -(-nent // CHUNK_SEGS)
        q = np.asarray(queries, F32).astype(np.float64)
        fin = np.isfinite(q).all(axis=1)
        # gather table: the (up to four) segments of every chunk; len(ent) -> the column of zeros appended to `pairs` below
        table = np.full((self.n_chunks, CHUNK_SEGS), len(ent), np.int64)
        table[ent // CHUNK_SEGS, ent % CHUNK_SEGS] = np.arange(len(ent))
        self.per_chunk = np.zeros((len(q), self.n_chunks), np.int32)
        for q0 in range(0, len(q), 512):
            x, y = q[q0 : q0 + 512, 0, None], q[q0 : q0 + 512, 1, None]
            if self.fill:
                pairs = np_hit._winding_pairs(a[None], b[None], x, y).astype(np.int32)
            else:
                pairs = np_hit._stroke_pairs(a[None], b[None], self.hw, x, y).astype(np.int32)
            pairs = np.concatenate([pairs, np.zeros((len(x), 1), np.int32)], axis=1)
            self.per_chunk[q0 : q0 + 512] = pairs[:, table].sum(axis=2)
        self.per_chunk[~fin] = 0
        self.total = self.per_chunk.sum(axis=1)

    def answer(self, total):
        if not self.fill:
            return total > 0
        return (total & 1) != 0 if self.even_odd else total != 0

    def changed_by(self, lost):
        """bool [queries]: whose answer changes if `lost` -- int [queries] or [queries, k] -- is taken from the item's total."""
        lost = np.asarray(lost)
        total = self.total if lost.ndim == 1 else self.total[:, None]
        return self.answer(total - lost) != self.answer(total)


def box_pass(con, boxes, queries):
    """bool [queries, boxes]: the kernel's box test of the item's kind (Fill: the box's rows hold y and it does not end left of x;
    Polyline: the box widened by half the width holds the point), binary64 on float32 values."""
    q = np.asarray(queries, F32).astype(np.float64)
    x, y = q[:, 0, None], q[:, 1, None]
    bb = np.asarray(boxes, np.float64)
    with np.errstate(invalid="ignore"):
        if con.fill:
            return (bb[None, :, 1] <= y) & (y < bb[None, :, 3]) & (bb[None, :, 2] >= x)
        hw = con.hw
        return ~((x < bb[None, :, 0] - hw) | (x > bb[None, :, 2] + hw) | (y < bb[None, :, 1] - hw) | (y > bb[None, :, 3] + hw))


def boundary_chunks(cb0, cb1):
    """Chunks of an item (positions in the item) at its structural edges: its first and last chunk -- the ones that share a super-chunk
    with a neighbour --, positions 0, 7, 8, 63, 64, 511, 512, and the chunks on either side of the super-chunk boundaries of the
    global table next to those: the item's first and last boundary and the ones that begin its 8th, 9th, 64th and 65th super-chunk."""
    n = cb1 - cb0
    pos = {0, n - 1} | {p for p in (7, 8, 63, 64, 511, 512) if p < n}
    g0 = cb0 // SUPER_CHUNKS
    g_last = (cb1 - 1) // SUPER_CHUNKS
    for g in {g0 + 1, g_last, g0 + 7, g0 + 8, g0 + 63, g0 + 64}:
        for c in (g * SUPER_CHUNKS - 1, g * SUPER_CHUNKS):
            if cb0 <= c < cb1:
                pos.add(c - cb0)
    return sorted(pos)


def losses(case):
    """For the long item of a case of part A: the drop sets the kernel's structure suggests, each with the queries whose answer would change.
    Returns {name: bool [queries] or, for per-chunk / per-super sets, bool [sets]} and the facts the test asserts on."""
    base, chunk_bbox, sup_bbox = index_model(case.scene)
    item = case.long_item
    cb0, cb1 = int(base[item]), int(base[item + 1])
    con = Contributions(case.scene, item, case.queries)
    n = cb1 - cb0
    g0, g1 = cb0 // SUPER_CHUNKS, (cb1 - 1) // SUPER_CHUNKS + 1
    # the item's own chunks per super-chunk of the global table
    sup_of = (cb0 + np.arange(n)) // SUPER_CHUNKS - g0
    per_sup = np.zeros((len(case.queries), g1 - g0), np.int32)
    for g in range(g1 - g0):
        per_sup[:, g] = con.per_chunk[:, sup_of == g].sum(axis=1)
    out = {
        "cb0": cb0, "cb1": cb1, "g0": g0, "g1": g1, "con": con,
        "each_chunk": con.changed_by(con.per_chunk).any(axis=0),
        "each_super": con.changed_by(per_sup).any(axis=0),
        "boundary": boundary_chunks(cb0, cb1),
    }
    if n > WAVE:
        passed = box_pass(con, sup_bbox[g0:g1], case.queries)
        passed &= np.isfinite(case.queries).all(axis=1)[:, None]
        rank = np.cumsum(passed, axis=1)
        out["most_survivors"] = int(rank[:, -1].max())
        # all survivors after the first eight; and the same per round of WAVE super-chunks (what a kernel that stops after one
        # round of eight in every round of WAVE would lose)
        out["after_eight"] = con.changed_by((per_sup * (passed & (rank > 8))).sum(axis=1))
        in_round = np.concatenate([np.cumsum(passed[:, r : r + WAVE], axis=1) for r in range(0, g1 - g0, WAVE)], axis=1)
        out["after_eight_per_round"] = con.changed_by((per_sup * (passed & (in_round > 8))).sum(axis=1))
        if g1 - g0 > WAVE:
            out["from_65th_super"] = con.changed_by(per_sup[:, WAVE:].sum(axis=1))
    return out


# ---- C. the item walk ---------------------------------------------------------------------------------------------

COMMON = (50.0, 50.0)
ARMS_ONLY = (45.0, 45.0)   # in the common square of the Fills, in no private spot
NOTHING = (8.0, 140.0)
WALK_SIZES = (1, 63, 64, 65, 127, 128, 129, 200)
KINDS = ("compound", "polyline", "line", "fill", "circle")   # the circle's place is taken by an ellipse every other time round


def walk_kind(i):
    k = KINDS[i % 5]
    return "ellipse" if k == "circle" and (i // 5) % 2 else k


def walk_scene(pm, n):
    """n items; item i's private spot is the 6 x 6 cell at (72 + 12 (i % 16), 72 + 12 (i // 16)) -- a Line's is on its own ray from the
    common point into the empty quarter instead, since one segment cannot reach a cell without crossing others.  Arms reach the
    common point through the lanes between the cells: a Fill's as a there-and-back path of axis-aligned segments, which cancels
    exactly, a Polyline's (width 1) up the lane right of its cell.  The first n // 2 items sit in a child group."""
    half = n // 2
    sq = lambda x, y, s: np.array([[x, y], [x + s, y], [x + s, y + s], [x, y + s]])  # noqa: E731
    common_sq = sq(44.0, 44.0, 12.0)
    n_lines = sum(walk_kind(i) == "line" for i in range(n))
    spots, li = [], 0

    def item(e, i):
        nonlocal li
        kind = walk_kind(i)
        rgba = (0x10305000 + (i << 8) & 0xFFFFFF00) | (0x00 if i % 3 == 0 else 0xFF)
        cx, cy = 72.0 + 12.0 * (i % 16), 72.0 + 12.0 * (i // 16)
        spot = (cx + 3.0, cy + 3.0)
        if kind == "compound":
            e.fill_compound([sq(cx, cy, 6.0), common_sq], rgba, even_odd=bool(i & 1))
        elif kind == "fill":
            lane = cx - 3.0
            e.fill(np.array([(cx, cy), (cx + 6, cy), (cx + 6, cy + 6), (cx, cy + 6), (cx, cy), (lane, cy), (lane, 60.0), (50.0, 60.0), (50.0, 56.0),
                             (44.0, 56.0), (44.0, 44.0), (56.0, 44.0), (56.0, 56.0), (50.0, 56.0), (50.0, 60.0), (lane, 60.0), (lane, cy)]), rgba)
        elif kind == "polyline":
            e.polyline(np.array([(cx + 3, cy + 3), (cx + 5.5, cy + 5.5), (cx + 9, cy + 9), (cx + 9, 60.0), (50.0, 60.0), COMMON]), rgba, 1.0)
        elif kind == "line":
            th = np.deg2rad(110.0 + 140.0 * (li + 0.5) / n_lines)
            li += 1
            d = np.array([np.cos(th), np.sin(th)])
            e.stroke_line(COMMON, tuple(np.array(COMMON) + 45.0 * d), 1.0, rgba)
            spot = tuple(np.array(COMMON) + 42.0 * d)
        elif kind == "circle":
            e.circle(spot, 3.0)
        else:
            e.ellipse(spot, 3.0, 2.0)
        spots.append(spot)

    def emit(e):
        if half:
            e.begin_group(half)
            for i in range(half):
                item(e, i)
            e.end_group()
        for i in range(half, n):
            item(e, i)

    scene = _encode(pm, (1 if half else 0) + n - half, emit)
    spots = np.array(spots)
    q = np.concatenate([spots, spots + 2.5, [COMMON, ARMS_ONLY, NOTHING]])
    kinds = [walk_kind(i) for i in range(n)]
    covering = [i for i in range(n) if kinds[i] not in ("circle", "ellipse")]
    return Case(f"walk n={n}", scene, q, kinds=kinds, covering=covering, opaque=[i for i in covering if i % 3 != 0], n=n)
