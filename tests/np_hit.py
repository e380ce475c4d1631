"""Independent numpy restatement of point hit testing, decision D13: which items of a scene byte buffer contain a
point.  Written from the decision's text, not from the kernel: no item box, no chunk index, no paint-order walk from the top.
Every item is asked about every query, in paint order, and the last one that says yes is the top item.  Test infrastructure.

All arithmetic is numpy float64 on the scene's f32 / u16 values, one ufunc per written operation, in the written order (numpy
never fuses a multiply with an add), so the results are the decision's bit for bit.

Two evaluation orders give the same booleans:
  brute=True   every (query, segment) pair is evaluated -- the plain statement, O(queries x segments);
  brute=False  the queries are sorted by y once and a segment meets only the queries of a y interval:
               * Fill: exactly those with a.y <= y < b.y (or b.y <= y < a.y) -- np.searchsorted evaluates that very predicate on
                 the sorted values, every other pair adds 0 by the decision's own text;
               * stroke: those with lo - hw - m <= y <= hi + hw + m, where [lo, hi] holds every c.y the decision can compute for
                 the segment (a.y and a.y + (b.y - a.y): t is in [0, 1] and rounding is monotonic) and m = 1e-6 of the values'
                 magnitude, ten orders above what the roundings of d.y and its square can move.  Outside, d.y * d.y alone exceeds
                 hw * hw.  Inside the interval the predicate itself is evaluated.
tests/test_hit_cpu.py checks the two against each other, with queries on vertices, edges and interval ends.
"""
import struct

import numpy as np

HIT_NONE = 0xFFFFFFFF
CIRCLE, LINE, FILL, POLY, GROUP = 1, 2, 3, 4, 5
FILL_EVEN_ODD, FILL_COMPOUND = 1, 2
CIRCLE_ELLIPSE = 1 << 16


def flat_items(scene):
    """[(item offset, (x0, y0, x1, y1))] in flat paint order: nested groups inlined depth first."""
    sc = bytes(scene)
    out = []

    def walk(group, depth):
        assert depth <= 32
        n, items_ix = struct.unpack_from("<II", sc, group)
        for i in range(n):
            at = items_ix + 32 * i
            (tag,) = struct.unpack_from("<I", sc, at)
            if tag & 0xFFFF == GROUP:
                walk(struct.unpack_from("<I", sc, at + 8)[0], depth + 1)
            else:
                out.append((at, struct.unpack_from("<4H", sc, group + 8 + 8 * i)))

    walk(0, 0)
    return out


def _points(sc, at):
    npt, pix = struct.unpack_from("<II", sc, at + 12)
    return np.frombuffer(sc, np.float32, 2 * npt, pix).reshape(npt, 2)


def fill_segments(pts, compound):
    """(a, b) float64 arrays [S, 2]: the segments of a Fill as the frame path takes them."""
    npt = len(pts)
    if npt == 0:
        return np.zeros((0, 2)), np.zeros((0, 2))
    k = np.arange(npt)
    nxt = np.where(k + 1 == npt, 0, k + 1)
    a, b = pts[k], pts[nxt].copy()
    keep = np.ones(npt, bool)
    if compound:
        keep = ~np.isnan(a[:, 0])  # a separator starts no segment
        closing = np.isnan(b[:, 0])  # a point followed by a separator closes to the index the separator carries
        first = np.minimum(np.ascontiguousarray(pts[nxt][:, 1]).view(np.uint32), npt - 1)
        b[closing] = pts[first[closing]]
    return a[keep].astype(np.float64), b[keep].astype(np.float64)


def stroke_segments(sc, at, tag):
    """(a, b, hw) of a Line or Polyline item; a one-point Polyline is one degenerate segment."""
    if tag == LINE:
        w, ax, ay, bx, by = struct.unpack_from("<5f", sc, at + 12)
        a, b = np.array([[ax, ay]], np.float32), np.array([[bx, by]], np.float32)
    else:
        (w,) = struct.unpack_from("<f", sc, at + 8)
        pts = _points(sc, at)
        if len(pts) == 0:
            a = b = np.zeros((0, 2), np.float32)
        elif len(pts) == 1:
            a = b = pts
        else:
            a, b = pts[:-1], pts[1:]
    return a.astype(np.float64), b.astype(np.float64), np.float64(0.5) * np.float64(np.float32(w))


def _winding_pairs(a, b, x, y):
    """Contribution of segment rows a -> b to queries (x, y), elementwise (broadcasting)."""
    ax, ay, bx, by = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
        up = (ay <= y) & (y < by) & (s > 0)
        down = (by <= y) & (y < ay) & (s < 0)
    return up.astype(np.int64) - down.astype(np.int64)


def _stroke_pairs(a, b, hw, x, y):
    ax, ay, bx, by = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        abx, aby = bx - ax, by - ay
        apx, apy = x - ax, y - ay
        L = abx * abx + aby * aby
        t = np.minimum(np.maximum((apx * abx + apy * aby) / np.where(L == 0, 1.0, L), 0.0), 1.0)
        t = np.where(L == 0, 0.0, t) + np.zeros_like(apx)
        cx, cy = ax + abx * t, ay + aby * t
        dx, dy = x - cx, y - cy
        return dx * dx + dy * dy <= hw * hw


def _expand(lo, hi):
    """Pairs (segment, query position) for per-segment ranges [lo, hi) of sorted query positions."""
    cnt = np.maximum(hi - lo, 0)
    seg = np.repeat(np.arange(len(lo)), cnt)
    start = np.cumsum(cnt) - cnt
    pos = lo[seg] + (np.arange(int(cnt.sum())) - start[seg])
    return seg, pos


def _fill_inside(a, b, even_odd, x, y, brute):
    n = len(x)
    if brute:
        wind = np.zeros(n, np.int64)
        for q0 in range(0, n, 4096):  # (memory: 4 096 queries x all segments at a time)
            sl = slice(q0, q0 + 4096)
            wind[sl] = _winding_pairs(a[None, :, :], b[None, :, :], x[sl, None], y[sl, None]).sum(axis=1)
    else:
        ay, by = a[:, 1], b[:, 1]
        ok = ~(np.isnan(ay) | np.isnan(by))
        a, b, ay, by = a[ok], b[ok], ay[ok], by[ok]
        lo = np.searchsorted(y, np.minimum(ay, by), "left")  # y sorted: positions with min <= y < max
        hi = np.searchsorted(y, np.maximum(ay, by), "left")
        seg, pos = _expand(lo, hi)
        wind = np.bincount(pos, weights=_winding_pairs(a[seg], b[seg], x[pos], y[pos]), minlength=n).astype(np.int64)
    return (wind & 1) != 0 if even_odd else wind != 0


def _stroke_inside(a, b, hw, x, y, brute):
    n = len(x)
    inside = np.zeros(n, bool)
    if len(a) == 0:
        return inside
    if brute:
        for q0 in range(0, n, 4096):
            sl = slice(q0, q0 + 4096)
            inside[sl] = _stroke_pairs(a[None, :, :], b[None, :, :], hw, x[sl, None], y[sl, None]).any(axis=1)
        return inside
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)  # (a non-finite end makes c NaN for every query: no hit)
    a, b = a[ok], b[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        far = a[:, 1] + (b[:, 1] - a[:, 1])
        ylo, yhi = np.minimum(a[:, 1], far), np.maximum(a[:, 1], far)
        m = 1e-6 * (1.0 + np.abs(hw) + np.maximum(np.abs(ylo), np.abs(yhi)))
        lo = np.searchsorted(y, ylo - hw - m, "left")
        hi = np.searchsorted(y, yhi + hw + m, "right")
    if np.isnan(hw):
        return inside
    seg, pos = _expand(lo, hi)
    inside[pos[_stroke_pairs(a[seg], b[seg], hw, x[pos], y[pos])]] = True
    return inside


def _circle_inside(bbox, ellipse, x, y):
    x0, y0, x1, y1 = (np.float64(v) for v in bbox)
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    rx, ry = cx - x0, cy - y0
    dx, dy = x - cx, y - cy
    if ellipse:
        if not (rx > 0 and ry > 0):
            return np.zeros(len(x), bool)
        return (dx / rx) * (dx / rx) + (dy / ry) * (dy / ry) <= 1.0
    r = min(rx, ry)
    return dx * dx + dy * dy <= r * r


def _item_inside(sc, at, bbox, x, y, brute, skip_transparent):
    """bool [len(x)]: the item at byte offset `at` contains (x, y) -- finite float64 queries, sorted by y unless brute."""
    (word,) = struct.unpack_from("<I", sc, at)
    tag = word & 0xFFFF
    if tag == CIRCLE:
        return _circle_inside(bbox, bool(word & CIRCLE_ELLIPSE), x, y)
    if tag in (LINE, FILL, POLY):
        (rgba,) = struct.unpack_from("<I", sc, at + (4 if tag == POLY else 8))
        if skip_transparent and rgba >> 24 == 0:
            return np.zeros(len(x), bool)
    if tag == FILL:
        (flags,) = struct.unpack_from("<I", sc, at + 4)
        a, b = fill_segments(_points(sc, at), bool(flags & FILL_COMPOUND))
        return _fill_inside(a, b, bool(flags & FILL_EVEN_ODD), x, y, brute)
    if tag in (LINE, POLY):
        a, b, hw = stroke_segments(sc, at, tag)
        return _stroke_inside(a, b, hw, x, y, brute)
    return np.zeros(len(x), bool)


def _queries(pts):
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    fin = np.flatnonzero(np.isfinite(x) & np.isfinite(y))  # a non-finite coordinate hits nothing
    order = fin[np.argsort(y[fin], kind="stable")]
    return len(pts), order, x[order], y[order]


def item_inside(scene, item, pts, brute=False):
    """bool [n]: does flat item `item` contain each point."""
    sc = bytes(scene)
    n, order, x, y = _queries(pts)
    at, bbox = flat_items(sc)[item]
    out = np.zeros(n, bool)
    out[order] = _item_inside(sc, at, bbox, x, y, brute, False)
    return out


def hit_test(scene, pts, skip_transparent=False, brute=False):
    """(top_item uint32 [n], n_hit uint32 [n]) of the scene byte buffer for float32 points [n, 2]."""
    sc = bytes(scene)
    n, order, x, y = _queries(pts)
    top = np.full(len(order), HIT_NONE, np.uint32)
    cnt = np.zeros(len(order), np.uint32)
    for i, (at, bbox) in enumerate(flat_items(sc)):
        inside = _item_inside(sc, at, bbox, x, y, brute, skip_transparent)
        top[inside] = i
        cnt[inside] += 1
    top_all = np.full(n, HIT_NONE, np.uint32)
    cnt_all = np.zeros(n, np.uint32)
    top_all[order] = top
    cnt_all[order] = cnt
    return top_all, cnt_all
