"""Independent numpy restatement of the polygon queries, decision D20: which items of a scene byte buffer a query
polygon K TOUCHES, and which it ENCLOSES.  Written from the decision's text, not from the kernel: no item box, no edge groups, no
chunk index, no early end.  Every (segment, edge) and every (point, edge) pair is evaluated.  Test infrastructure; it reuses
np_hit's reading of the scene (flat_items, fill_segments, stroke_segments) and D13's own two predicates (the winding sum and the
squared distance to a segment), which D20 refers to.

All arithmetic is numpy float64 on the scene's f32 / u16 values and the polygon's f32 values, one ufunc per written operation, in
the written order.  np.minimum / np.maximum keep a NaN, and every comparison with a NaN is false.
"""
import struct

import numpy as np

import np_hit
from np_hit import CIRCLE, CIRCLE_ELLIPSE, FILL, FILL_COMPOUND, FILL_EVEN_ODD, LINE, POLY

TOUCHES, ENCLOSES = 1, 2
MAX_VERTICES = 4096


class Polygon:
    """K: float64 columns of the float32 vertices, its closing edges c -> d, and whether it is valid."""

    def __init__(self, vertices, even_odd=False):
        v = np.asarray(vertices, np.float32).reshape(-1, 2)
        assert 3 <= len(v) <= MAX_VERTICES
        self.m = len(v)
        self.even_odd = bool(even_odd)
        self.valid = bool(np.isfinite(v).all())
        self.c = v.astype(np.float64)
        self.d = np.roll(self.c, -1, axis=0)     # e_j: v_j -> v_(j + 1) mod m


def orient(ax, ay, bx, by, px, py):
    with np.errstate(invalid="ignore", over="ignore"):
        return (bx - ax) * (py - ay) - (px - ax) * (by - ay)


def in_k(K, p):
    """bool [n]: inK(p) for points p float64 [n, 2]."""
    p = np.asarray(p, np.float64).reshape(-1, 2)
    wind = np_hit._winding_pairs(K.c[None, :, :], K.d[None, :, :], p[:, None, 0], p[:, None, 1]).sum(axis=1)
    inside = (wind & 1) != 0 if K.even_odd else wind != 0
    return inside & np.isfinite(p).all(axis=1)


def crosses(K, a, b):
    """bool [S, m]: crosses(a[s] -> b[s], e_j)."""
    ax, ay, bx, by = a[:, None, 0], a[:, None, 1], b[:, None, 0], b[:, None, 1]
    cx, cy, dx, dy = K.c[None, :, 0], K.c[None, :, 1], K.d[None, :, 0], K.d[None, :, 1]
    fin = (np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1))[:, None] & (np.isfinite(K.c).all(axis=1) & np.isfinite(K.d).all(axis=1))[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        box = ((np.minimum(ax, bx) <= np.maximum(cx, dx)) & (np.maximum(ax, bx) >= np.minimum(cx, dx))
               & (np.minimum(ay, by) <= np.maximum(cy, dy)) & (np.maximum(ay, by) >= np.minimum(cy, dy)))
        s1, s2 = orient(ax, ay, bx, by, cx, cy), orient(ax, ay, bx, by, dx, dy)
        s3, s4 = orient(cx, cy, dx, dy, ax, ay), orient(cx, cy, dx, dy, bx, by)
        apart = ((s1 > 0) & (s2 > 0)) | ((s1 < 0) & (s2 < 0)) | ((s3 > 0) & (s4 > 0)) | ((s3 < 0) & (s4 < 0))
    return fin & box & ~apart


def near(K, a, b, hw):
    """bool [S, m]: near(a[s] -> b[s], e_j, hw * hw)."""
    A, B, Cc, D = a[:, None, :], b[:, None, :], K.c[None, :, :], K.d[None, :, :]
    out = np_hit._stroke_pairs(A, B, hw, Cc[..., 0], Cc[..., 1])       # c to a -> b
    out = out | np_hit._stroke_pairs(A, B, hw, D[..., 0], D[..., 1])   # d to a -> b
    out = out | np_hit._stroke_pairs(Cc, D, hw, A[..., 0], A[..., 1])  # a to c -> d
    out = out | np_hit._stroke_pairs(Cc, D, hw, B[..., 0], B[..., 1])  # b to c -> d
    return out


def _answer(reach, inside, extra_touch=False):
    """(touches, encloses) from B, inK of every point [n] (n >= 1: the item has geometry) and a Fill's own term."""
    touches = bool(reach) or bool(inside.any()) or bool(extra_touch)
    encloses = (not reach) and bool(inside.all())       # (inK is false for a non-finite point)
    return touches, encloses


def _fill(sc, at, K):
    (flags,) = struct.unpack_from("<I", sc, at + 4)
    compound = bool(flags & FILL_COMPOUND)
    pts = np_hit._points(sc, at)
    p = pts.astype(np.float64)
    if compound:
        p = p[~np.isnan(p[:, 0])]   # a separator is no point
    if len(p) == 0:
        return False, False
    a, b = np_hit.fill_segments(pts, compound)
    reach = crosses(K, a, b).any()
    wind = np_hit._winding_pairs(a, b, K.c[0, 0], K.c[0, 1]).sum()
    v0_inside = (wind & 1) != 0 if flags & FILL_EVEN_ODD else wind != 0
    return _answer(reach, in_k(K, p), v0_inside)


def _stroke(sc, at, tag, K):
    a, b, hw = np_hit.stroke_segments(sc, at, tag)
    if len(a) == 0 or np.isnan(hw):
        return False, False
    reach = crosses(K, a, b).any() or near(K, a, b, hw).any()
    return _answer(reach, in_k(K, np.concatenate([a[:1], b])))


def _circle(bbox, ellipse, K):
    x0, y0, x1, y1 = (np.float64(v) for v in bbox)
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    rx, ry = cx - x0, cy - y0
    centre = np.array([[cx, cy]])
    if ellipse:
        if not (rx > 0 and ry > 0):
            return False, False
        mc = np.stack([(K.c[:, 0] - cx) / rx, (K.c[:, 1] - cy) / ry], axis=1)
        md = np.stack([(K.d[:, 0] - cx) / rx, (K.d[:, 1] - cy) / ry], axis=1)
        reach = np_hit._stroke_pairs(mc, md, np.float64(1.0), np.float64(0.0), np.float64(0.0)).any()
    else:
        r = min(rx, ry)
        reach = np_hit._stroke_pairs(K.c, K.d, r, cx, cy).any()
    return _answer(reach, in_k(K, centre))


def item_flags(scene, vertices, skip_transparent=False, even_odd=False):
    """uint8 [n_items]: TOUCHES | ENCLOSES of every item of the scene byte buffer for the float32 polygon."""
    sc = bytes(scene)
    K = Polygon(vertices, even_odd)
    items = np_hit.flat_items(sc)
    out = np.zeros(len(items), np.uint8)
    if not K.valid:
        return out
    for i, (at, bbox) in enumerate(items):
        (word,) = struct.unpack_from("<I", sc, at)
        tag = word & 0xFFFF
        if tag in (LINE, FILL, POLY):
            (rgba,) = struct.unpack_from("<I", sc, at + (4 if tag == POLY else 8))
            if skip_transparent and rgba >> 24 == 0:
                continue
        if tag == CIRCLE:
            t, e = _circle(bbox, bool(word & CIRCLE_ELLIPSE), K)
        elif tag == FILL:
            t, e = _fill(sc, at, K)
        elif tag in (LINE, POLY):
            t, e = _stroke(sc, at, tag, K)
        else:
            continue
        out[i] = t * TOUCHES + e * ENCLOSES
    return out
