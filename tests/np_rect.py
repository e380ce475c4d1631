"""Independent numpy restatement of the rectangle queries, decision D19: which items of a scene byte buffer a closed
axis-aligned rectangle TOUCHES, and which it ENCLOSES.  Written from the decision's text, not from the kernels: no item box, no
chunk index, no walk from the top of paint order, no early end.  Every (rectangle, segment) pair is evaluated.  Test
infrastructure; it reuses np_hit's reading of the scene (flat_items, fill_segments, stroke_segments) and D13's own two
predicates (the winding sum and the squared distance to a segment), which D19 refers to.

All arithmetic is numpy float64 on the scene's f32 / u16 values and the query's f32 values, one ufunc per written operation, in
the written order.  np.maximum keeps a NaN, as the decision says its max does.
"""
import struct

import numpy as np

import np_hit
from np_hit import CIRCLE, CIRCLE_ELLIPSE, FILL, FILL_COMPOUND, FILL_EVEN_ODD, HIT_NONE, LINE, POLY

TOUCHES, ENCLOSES = 1, 2


class Rects:
    """n query rectangles: float64 columns of the float32 values, and which of them are valid."""

    def __init__(self, rects):
        r = np.asarray(rects, np.float32).reshape(-1, 4)
        self.n = len(r)
        self.x0, self.y0, self.x1, self.y1 = (r[:, k].astype(np.float64) for k in range(4))
        with np.errstate(invalid="ignore"):
            self.valid = np.isfinite(r).all(axis=1) & ~(self.x1 < self.x0) & ~(self.y1 < self.y0)

    def corners(self):
        """c0 .. c3 as (x, y) pairs of [n] arrays."""
        return [(self.x0, self.y0), (self.x1, self.y0), (self.x1, self.y1), (self.x0, self.y1)]


def dist2_to_rect(R, px, py):
    """dR2(p), [n, S] for points [S]."""
    with np.errstate(invalid="ignore", over="ignore"):
        ex = np.maximum(np.maximum(R.x0[:, None] - px[None, :], 0.0), px[None, :] - R.x1[:, None])
        ey = np.maximum(np.maximum(R.y0[:, None] - py[None, :], 0.0), py[None, :] - R.y1[:, None])
        return ex * ex + ey * ey


def segments_meet(R, a, b):
    """bool [n, S]: segment a[s] -> b[s] meets rectangle r."""
    ax, ay, bx, by = a[None, :, 0], a[None, :, 1], b[None, :, 0], b[None, :, 1]
    fin = (np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1))[None, :]
    x0, y0, x1, y1 = R.x0[:, None], R.y0[:, None], R.x1[:, None], R.y1[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        box = (np.minimum(ax, bx) <= x1) & (np.maximum(ax, bx) >= x0) & (np.minimum(ay, by) <= y1) & (np.maximum(ay, by) >= y0)
        pos = np.ones(box.shape, bool)
        neg = np.ones(box.shape, bool)
        for cx, cy in R.corners():
            s = (bx - ax) * (cy[:, None] - ay) - (cx[:, None] - ax) * (by - ay)
            pos &= s > 0
            neg &= s < 0
    return fin & box & ~(pos | neg)


def _fill(sc, at, R):
    """(touches, encloses) bool [n] of a Fill."""
    (flags,) = struct.unpack_from("<I", sc, at + 4)
    compound = bool(flags & FILL_COMPOUND)
    pts = np_hit._points(sc, at)
    a, b = np_hit.fill_segments(pts, compound)
    if len(pts) == 0:
        return np.zeros(R.n, bool), np.zeros(R.n, bool)
    meets = segments_meet(R, a, b).any(axis=1)
    wind = np_hit._winding_pairs(a[None, :, :], b[None, :, :], R.x0[:, None], R.y0[:, None]).sum(axis=1)
    inside = (wind & 1) != 0 if flags & FILL_EVEN_ODD else wind != 0
    p = pts.astype(np.float64)
    if compound:
        p = p[~np.isnan(p[:, 0])]   # a separator is no point
    with np.errstate(invalid="ignore"):
        within = (R.x0[:, None] <= p[None, :, 0]) & (p[None, :, 0] <= R.x1[:, None]) & (R.y0[:, None] <= p[None, :, 1]) & (p[None, :, 1] <= R.y1[:, None])
    encloses = within.all(axis=1) & bool(len(p)) & bool(np.isfinite(p).all())
    return meets | inside, encloses


def _stroke(sc, at, tag, R):
    a, b, hw = np_hit.stroke_segments(sc, at, tag)
    if len(a) == 0:
        return np.zeros(R.n, bool), np.zeros(R.n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        near = segments_meet(R, a, b)
        for cx, cy in R.corners():
            near |= np_hit._stroke_pairs(a[None, :, :], b[None, :, :], hw, cx[:, None], cy[:, None])
        near |= dist2_to_rect(R, a[:, 0], a[:, 1]) <= hw * hw
        near |= dist2_to_rect(R, b[:, 0], b[:, 1]) <= hw * hw
        touches = near.any(axis=1) & ~np.isnan(hw)
        p = np.concatenate([a[:1], b])   # every point (a one-point Polyline's twice)
        px, py = p[None, :, 0], p[None, :, 1]
        within = (R.x0[:, None] <= px - hw) & (px + hw <= R.x1[:, None]) & (R.y0[:, None] <= py - hw) & (py + hw <= R.y1[:, None])
    return touches, within.all(axis=1) & bool(np.isfinite(p).all())


def _circle(bbox, ellipse, R):
    x0, y0, x1, y1 = (np.float64(v) for v in bbox)
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    rx, ry = cx - x0, cy - y0
    ex = np.maximum(np.maximum(R.x0 - cx, 0.0), cx - R.x1)
    ey = np.maximum(np.maximum(R.y0 - cy, 0.0), cy - R.y1)
    if ellipse:
        if not (rx > 0 and ry > 0):   # it contains no point (D13): no geometry
            return np.zeros(R.n, bool), np.zeros(R.n, bool)
        touches = (ex / rx) * (ex / rx) + (ey / ry) * (ey / ry) <= 1.0
    else:
        r = min(rx, ry)
        touches = ex * ex + ey * ey <= r * r
        rx = ry = r
    encloses = (R.x0 <= cx - rx) & (cx + rx <= R.x1) & (R.y0 <= cy - ry) & (cy + ry <= R.y1)
    return touches, encloses


def item_flags(scene, rects, skip_transparent=False):
    """uint8 [n_items, n]: TOUCHES | ENCLOSES of every item of the scene byte buffer for every float32 rectangle."""
    sc = bytes(scene)
    R = Rects(rects)
    items = np_hit.flat_items(sc)
    out = np.zeros((len(items), R.n), np.uint8)
    for i, (at, bbox) in enumerate(items):
        (word,) = struct.unpack_from("<I", sc, at)
        tag = word & 0xFFFF
        if tag in (LINE, FILL, POLY):
            (rgba,) = struct.unpack_from("<I", sc, at + (4 if tag == POLY else 8))
            if skip_transparent and rgba >> 24 == 0:
                continue
        if tag == CIRCLE:
            t, e = _circle(bbox, bool(word & CIRCLE_ELLIPSE), R)
        elif tag == FILL:
            t, e = _fill(sc, at, R)
        elif tag in (LINE, POLY):
            t, e = _stroke(sc, at, tag, R)
        else:
            continue
        out[i] = (t & R.valid) * TOUCHES + (e & R.valid) * ENCLOSES
    return out


def hit_rects(scene, rects, skip_transparent=False, flags=None):
    """(top_item uint32 [n], n_hit uint32 [n]): the last item in paint order each rectangle touches, and how many it touches."""
    f = item_flags(scene, rects, skip_transparent) if flags is None else flags
    t = (f & TOUCHES) != 0
    n_items, n = t.shape
    top = np.full(n, HIT_NONE, np.uint32)
    if n_items:
        last = n_items - 1 - np.argmax(t[::-1], axis=0)
        top = np.where(t.any(axis=0), last, HIT_NONE).astype(np.uint32)
    return top, t.sum(axis=0).astype(np.uint32)


def pick_rects(points, tolerance):
    """(n, 4) float32: {f32(x) - f32(t), f32(y) - f32(t), f32(x) + f32(t), f32(y) + f32(t)}, each rounded to f32."""
    xy = np.asarray(points, np.float32).reshape(-1, 2)
    t = np.float32(tolerance)
    return np.concatenate([(xy - t).astype(np.float32), (xy + t).astype(np.float32)], axis=1)
