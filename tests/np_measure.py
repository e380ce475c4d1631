"""Independent statement of path measurement, decision D25: the length of every item of a scene byte buffer, the
point at a position along an item, and the position of a point of an edge.  Written from the decision's text, not from the
kernels: no waves, no scan -- the segments of an item are listed one by one in Python, their lengths are Python integers, a
position's owner is found by walking the list.  Test infrastructure; it reads the scene through np_hit.flat_items and shares no
code with np_dash.

Lengths and positions are integers in units of 2^-16 px.  Everything else is numpy float64 on the scene's f32 values, one ufunc
per written operation, rounded once to f32 where the decision says so.
"""
import struct

import numpy as np

import np_hit
from np_hit import FILL, FILL_COMPOUND, LINE, POLY

NONE, OPEN, CLOSED = 0, 1, 2                  # PM_MEASURE_NONE / _OPEN / _CLOSED
FOUND, CLAMPED, DEGENERATE = 1, 2, 4          # PM_MEASURE_FOUND / _CLAMPED / _DEGENERATE
HIT_NONE = 0xFFFFFFFF
SKIP_TRANSPARENT = 1
UNIT = 65536
SEG_CAP = 1 << 32

ITEM_LENGTH = np.dtype([("length", "<u8"), ("n_segments", "<u4"), ("kind", "<u4")])
LENGTH_QUERY = np.dtype([("item", "<u4"), ("reserved", "<u4"), ("s", "<u8")])
LENGTH_POINT = np.dtype([("item", "<u4"), ("status", "<u4"), ("index", "<u4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("tx", "<f4"), ("ty", "<f4")])
EDGE_QUERY = np.dtype([("item", "<u4"), ("index", "<u4"), ("t", "<f4"), ("reserved", "<u4")])
LENGTH_AT = np.dtype([("s", "<u8"), ("item", "<u4"), ("status", "<u4")])
assert (ITEM_LENGTH.itemsize, LENGTH_QUERY.itemsize, LENGTH_POINT.itemsize, EDGE_QUERY.itemsize, LENGTH_AT.itemsize) == (16, 16, 32, 16, 16)


def seg_units(a, b):
    """q of the segment a -> b (f32 pairs): 0 if the binary64 length is a NaN, else min(floor(len * 65536 + 0.5), 2^32)."""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = b[0] - a[0], b[1] - a[1]
        ln = np.sqrt(dx * dx + dy * dy)
        if np.isnan(ln):
            return 0
        f = np.floor(ln * np.float64(UNIT) + np.float64(0.5))
    return SEG_CAP if f >= float(SEG_CAP) else int(f)


class Walk:
    """The walk of one item: kind, the segments [(k, a, b, q)] in increasing k (a, b: f32 pairs as stored), and the first point
    (index, f32 pair) or None."""

    def __init__(self, kind=NONE, segs=(), first=None):
        self.kind, self.segs, self.first = kind, list(segs), first
        self.T = sum(s[3] for s in self.segs)


def walk_of(sc, at, skip_transparent=False):
    (word,) = struct.unpack_from("<I", sc, at)
    tag = word & 0xFFFF
    if tag not in (LINE, FILL, POLY):
        return Walk()
    if skip_transparent:
        (rgba,) = struct.unpack_from("<I", sc, at + (4 if tag == POLY else 8))
        if rgba >> 24 == 0:
            return Walk()
    if tag == LINE:
        p = np.frombuffer(sc, np.float32, 4, at + 16).reshape(2, 2)
        return Walk(OPEN, [(0, p[0], p[1], seg_units(p[0], p[1]))], (0, p[0]))
    p = np_hit._points(sc, at)
    n = len(p)
    if tag == POLY:
        return Walk(OPEN, [(k, p[k], p[k + 1], seg_units(p[k], p[k + 1])) for k in range(n - 1)], (0, p[0]) if n else None)
    if n == 0:
        return Walk()
    compound = bool(struct.unpack_from("<I", sc, at + 4)[0] & FILL_COMPOUND)
    segs, first = [], None
    for k in range(n):
        a = p[k]
        if compound and np.isnan(a[0]):
            continue                       # a separator is no point and starts no segment
        if first is None:
            first = (k, a)
        b = p[0] if k + 1 == n else p[k + 1]
        if compound and np.isnan(b[0]):    # a point followed by a separator closes to the index the separator carries, clamped
            b = p[min(int(np.float32(b[1]).view(np.uint32)), n - 1)]
        segs.append((k, a, b, seg_units(a, b)))
    return Walk(CLOSED, segs, first)


def walks(scene, skip_transparent=False):
    sc = bytes(scene)
    return [walk_of(sc, at, skip_transparent) for at, _ in np_hit.flat_items(sc)]


def item_lengths(scene, skip_transparent=False, ws=None):
    ws = walks(scene, skip_transparent) if ws is None else ws
    out = np.zeros(len(ws), ITEM_LENGTH)
    for i, w in enumerate(ws):
        out[i] = (w.T, len(w.segs), w.kind)
    return out


def _dir(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy = b[0] - a[0], b[1] - a[1]
        ln = np.sqrt(dx * dx + dy * dy)
        return np.float32(dx / ln), np.float32(dy / ln)


def point_at(w, item, s):
    """One LENGTH_POINT record as a tuple."""
    none = (HIT_NONE, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    if w.kind == NONE:
        return none
    positive = [sg for sg in w.segs if sg[3] > 0]
    if not positive:
        if w.first is None:
            return none
        k, p = w.first
        return (item, FOUND | DEGENERATE | (CLAMPED if s > 0 else 0), k, 0.0, p[0], p[1], 0.0, 0.0)
    if s >= w.T:
        k, a, b, _ = positive[-1]
        tx, ty = _dir(a, b)
        return (item, FOUND | (CLAMPED if s > w.T else 0), k, 1.0, b[0], b[1], tx, ty)
    Q = 0
    for k, a, b, q in w.segs:
        if q > 0 and Q <= s < Q + q:
            tx, ty = _dir(a, b)
            if s == Q:
                return (item, FOUND, k, 0.0, a[0], a[1], tx, ty)
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                t64 = np.float64(s - Q) / np.float64(q)
                x = a64[0] + (b64[0] - a64[0]) * t64
                y = a64[1] + (b64[1] - a64[1]) * t64
                return (item, FOUND, k, np.float32(t64), np.float32(x), np.float32(y), tx, ty)
        Q += q
    raise AssertionError("s < T has an owner")


def points_at_length(scene, queries, skip_transparent=False, ws=None):
    """LENGTH_POINT [n] for LENGTH_QUERY-like pairs (item, s)."""
    ws = walks(scene, skip_transparent) if ws is None else ws
    out = np.zeros(len(queries), LENGTH_POINT)
    for j, (item, s) in enumerate(queries):
        item, s = int(item), int(s)
        rec = point_at(ws[item], item, s) if item < len(ws) else point_at(Walk(), item, s)
        with np.errstate(invalid="ignore", over="ignore"):
            out[j] = rec
    return out


def position_on_edge(w, item, index, t):
    t = np.float32(t)
    if w.kind == NONE or not (t >= 0 and t <= 1):
        return (0, HIT_NONE, 0)
    Q = 0
    for k, a, b, q in w.segs:
        if k == index:
            f = int(np.floor(np.float64(t) * np.float64(q) + np.float64(0.5)))
            return (Q + min(f, q), item, FOUND)
        Q += q
    return (0, HIT_NONE, 0)


def positions_on_edges(scene, queries, skip_transparent=False, ws=None):
    """LENGTH_AT [n] for triples (item, index, t)."""
    ws = walks(scene, skip_transparent) if ws is None else ws
    out = np.zeros(len(queries), LENGTH_AT)
    for j, (item, index, t) in enumerate(queries):
        item = int(item)
        out[j] = position_on_edge(ws[item], item, int(index), t) if item < len(ws) else (0, HIT_NONE, 0)
    return out


def has_non_finite_end(w, index):
    """Does segment `index` of the walk have a non-finite end (then the five floats of a point record on it are not promised)."""
    for k, a, b, _ in w.segs:
        if k == index:
            return not (np.isfinite(a).all() and np.isfinite(b).all())
    return False
