"""Independent numpy restatement of snapping, decision D21: the nearest vertex or point of an edge of a scene byte
buffer to a query {x, y, r}.  Written from the decision's text, not from the kernel: no boxes, no index, every (query, candidate)
pair is evaluated.  Test infrastructure.

All arithmetic is numpy float64 on the scene's f32 / u16 values and the query's f32 values, one ufunc per written operation, in the
written order (numpy never fuses a multiply with an add), so d2, t and the point are the decision's bit for bit.

Two evaluation orders give the same records:
  per_item=False  every candidate of the scene at once, listed from the topmost item down and by index within an item: the first
                  minimum of d2 in that list is the winner (numpy's argmin names the first);
  per_item=True   every item's own winner first (the smallest d2, then the smallest index), then the items in paint order, a later
                  item replacing the running winner when its d2 is smaller OR EQUAL.
"""
import struct

import numpy as np

import np_hit

NONE = 0xFFFFFFFF
VERTEX, EDGE = 1, 2
RECORD = np.dtype([("item", "<u4"), ("kind", "<u4"), ("index", "<u4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("d2", "<f8")])
assert RECORD.itemsize == 32


def _finite(p):
    return np.isfinite(p).all(axis=1)


def item_offers(sc, at, bbox, skip_transparent=False):
    """(vertex index int64 [V], vertex f32 [V, 2], edge index int64 [E], a f32 [E, 2], b f32 [E, 2]) of the item at byte offset `at`."""
    none = (np.zeros(0, np.int64), np.zeros((0, 2), np.float32), np.zeros(0, np.int64), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    (word,) = struct.unpack_from("<I", sc, at)
    tag = word & 0xFFFF
    if tag in (np_hit.LINE, np_hit.FILL, np_hit.POLY):
        (rgba,) = struct.unpack_from("<I", sc, at + (4 if tag == np_hit.POLY else 8))
        if skip_transparent and rgba >> 24 == 0:
            return none
    if tag == np_hit.CIRCLE:
        x0, y0, x1, y1 = (np.float64(v) for v in bbox)
        cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
        if word & np_hit.CIRCLE_ELLIPSE and not (cx - x0 > 0 and cy - y0 > 0):
            return none
        return (np.zeros(1, np.int64), np.array([[cx, cy]], np.float32)) + none[2:]
    if tag == np_hit.FILL:
        (flags,) = struct.unpack_from("<I", sc, at + 4)
        pts = np_hit._points(sc, at)
        npt = len(pts)
        if npt == 0:
            return none
        compound = bool(flags & np_hit.FILL_COMPOUND)
        ent = np.flatnonzero(~np.isnan(pts[:, 0])) if compound else np.arange(npt)   # (a separator is no point and starts no segment)
        a64, b64 = np_hit.fill_segments(pts, compound)
        a, b = a64.astype(np.float32), b64.astype(np.float32)     # (f32 values, widened and narrowed: unchanged)
        assert len(a) == len(ent) and np.array_equal(a, pts[ent], equal_nan=True)
        vk = _finite(pts[ent])
        ek = _finite(a) & _finite(b)
        return ent[vk], pts[ent][vk], ent[ek], a[ek], b[ek]
    if tag == np_hit.POLY or tag == np_hit.LINE:
        a64, b64, _ = np_hit.stroke_segments(sc, at, tag)
        a, b = a64.astype(np.float32), b64.astype(np.float32)
        if tag == np_hit.LINE:
            pts = np.concatenate([a, b])
        else:
            pts = np_hit._points(sc, at)
        vi = np.arange(len(pts))
        vk = _finite(pts) if len(pts) else np.zeros(0, bool)
        ei = np.arange(len(a))
        ek = _finite(a) & _finite(b) if len(a) else np.zeros(0, bool)
        return vi[vk], pts[vk], ei[ek], a[ek], b[ek]
    return none


def vertex_d2(p, x, y):
    """float64 [n, V]: D21's d2 of vertices p (f32 [V, 2]) for queries x, y (float64 [n])."""
    px, py = p[:, 0].astype(np.float64)[None, :], p[:, 1].astype(np.float64)[None, :]
    with np.errstate(over="ignore"):
        dx, dy = x[:, None] - px, y[:, None] - py
        return dx * dx + dy * dy


def edge_parts(a, b, x, y):
    """(t, cx, cy, d2), float64, broadcast over a, b (f32 [..., 2]) and x, y: D21's edge distance, D13's own operations."""
    ax, ay, bx, by = (v.astype(np.float64) for v in (a[..., 0], a[..., 1], b[..., 0], b[..., 1]))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        abx, aby = bx - ax, by - ay
        apx, apy = x - ax, y - ay
        L = abx * abx + aby * aby
        t = np.minimum(np.maximum((apx * abx + apy * aby) / np.where(L == 0, 1.0, L), 0.0), 1.0)
        t = np.where(L == 0, 0.0, t)
        cx, cy = ax + abx * t, ay + aby * t
        dx, dy = x - cx, y - cy
        return t, cx, cy, dx * dx + dy * dy


def edge_d2(a, b, x, y):
    return edge_parts(a[None, :, :], b[None, :, :], x[:, None], y[:, None])[3]


class Queries:
    def __init__(self, xyr):
        q = np.ascontiguousarray(xyr, np.float32).reshape(-1, 3)
        self.n = len(q)
        self.x, self.y, r = (q[:, k].astype(np.float64) for k in range(3))
        with np.errstate(invalid="ignore", over="ignore"):
            self.valid = np.isfinite(self.x) & np.isfinite(self.y) & np.isfinite(r) & ~(r < 0)
            self.r2 = r * r


def _offers(scene, skip_transparent, skip_items):
    sc = bytes(scene)
    items = np_hit.flat_items(sc)
    skip = np.zeros(len(items), bool) if skip_items is None else np.asarray(skip_items)[: len(items)] != 0
    return [None if skip[i] else item_offers(sc, at, bbox, skip_transparent) for i, (at, bbox) in enumerate(items)]


def _best_of(d2, r2, valid):
    """(column of the first smallest qualifying d2 [n], found bool [n]) of float64 [n, C]."""
    if d2.shape[1] == 0:
        return np.zeros(len(d2), np.int64), np.zeros(len(d2), bool)
    with np.errstate(invalid="ignore"):
        ok = (d2 <= r2[:, None]) & valid[:, None]
    m = np.where(ok, d2, np.inf)
    col = np.argmin(m, axis=1)
    return col, ok[np.arange(len(d2)), col]


def _winners_at_once(offers, Q, kind):
    """(found, item, index, d2) per query: all candidates of one kind, listed topmost item first."""
    item, index, p, a, b = [], [], [], [], []
    for i in range(len(offers) - 1, -1, -1):
        if offers[i] is None:
            continue
        vi, vp, ei, ea, eb = offers[i]
        k = vi if kind == VERTEX else ei
        item.append(np.full(len(k), i, np.int64))
        index.append(k)
        p.append(vp)
        a.append(ea)
        b.append(eb)
    if not item:
        return np.zeros(Q.n, bool), np.zeros(Q.n, np.int64), np.zeros(Q.n, np.int64), np.zeros(Q.n)
    item, index = np.concatenate(item), np.concatenate(index)
    col, found, d2w = np.zeros(Q.n, np.int64), np.zeros(Q.n, bool), np.zeros(Q.n)
    for q0 in range(0, Q.n, 256):   # (memory)
        sl = slice(q0, q0 + 256)
        d2 = vertex_d2(np.concatenate(p), Q.x[sl], Q.y[sl]) if kind == VERTEX else edge_d2(np.concatenate(a), np.concatenate(b), Q.x[sl], Q.y[sl])
        col[sl], found[sl] = _best_of(d2, Q.r2[sl], Q.valid[sl])
        if d2.shape[1]:
            d2w[sl] = d2[np.arange(d2.shape[0]), col[sl]]
    if len(item) == 0:
        return found, col, col, d2w
    return found, item[col], index[col], d2w


def _winners_per_item(offers, Q, kind):
    found, item, index, best = np.zeros(Q.n, bool), np.zeros(Q.n, np.int64), np.zeros(Q.n, np.int64), np.full(Q.n, np.inf)
    for i, off in enumerate(offers):
        if off is None:
            continue
        vi, vp, ei, ea, eb = off
        k = vi if kind == VERTEX else ei
        if len(k) == 0:
            continue
        d2 = vertex_d2(vp, Q.x, Q.y) if kind == VERTEX else edge_d2(ea, eb, Q.x, Q.y)
        col, ok = _best_of(d2, Q.r2, Q.valid)     # (k ascends: the first minimum has the smallest index)
        mine = d2[np.arange(Q.n), col]
        take = ok & (mine <= best)                # a later item wins a tie
        found |= take
        item[take], index[take], best[take] = i, k[col[take]], mine[take]
    return found, item, index, np.where(found, best, 0.0)


def snap(scene, xyr, vertices=True, edges=True, skip_transparent=False, skip_items=None, per_item=False):
    """RECORD [n]: D21's answer for float32 queries [n, 3] {x, y, r}."""
    assert vertices or edges
    sc = bytes(scene)
    offers = _offers(sc, skip_transparent, skip_items)
    Q = Queries(xyr)
    winners = _winners_per_item if per_item else _winners_at_once
    out = np.zeros(Q.n, RECORD)
    out["item"] = NONE
    done = np.zeros(Q.n, bool)
    for kind in ([VERTEX] if vertices else []) + ([EDGE] if edges else []):     # a qualifying vertex wins over every edge
        found, item, index, d2 = winners(offers, Q, kind)
        for q in np.flatnonzero(found & ~done):
            off = offers[item[q]]
            out["item"][q], out["kind"][q], out["index"][q], out["d2"][q] = item[q], kind, index[q], d2[q]
            if kind == VERTEX:
                p = off[1][np.flatnonzero(off[0] == index[q])[0]]
                out["x"][q], out["y"][q] = p[0], p[1]
            else:
                e = np.flatnonzero(off[2] == index[q])[0]
                t, cx, cy, again = edge_parts(off[3][e], off[4][e], Q.x[q], Q.y[q])
                assert again == d2[q]
                out["t"][q], out["x"][q], out["y"][q] = np.float32(t), np.float32(cx), np.float32(cy)
        done |= found
    return out
