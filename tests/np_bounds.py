"""Independent numpy restatement of the bounds queries, decision D22: the bounding box of every item of a scene byte
buffer, and the union of boxes per label with its two counts.  Written from the decision's text, not from the kernels: no scene
index, no chunk boxes, no "min first, width afterwards" -- every point of every item is widened by hw on its own and then goes
through numpy's fmin / fmax, which ignore a NaN operand.  Test infrastructure; it reuses np_hit's reading of the scene
(flat_items, _points).

All arithmetic is numpy float64 on the scene's f32 / u16 values, one ufunc per written operation.  The last step is `+ 0.0` on
every value: a bound that is a zero is +0.
"""
import struct

import numpy as np

import np_hit
from np_hit import CIRCLE, CIRCLE_ELLIPSE, FILL, FILL_COMPOUND, LINE, POLY

INF = np.float64(np.inf)
EMPTY = np.array([INF, INF, -INF, -INF], np.float64)
LABEL_BOUNDS = np.dtype([("box", "<f8", (4,)), ("n_items", "<u4"), ("n_boxed", "<u4")])   # pm_label_bounds
assert LABEL_BOUNDS.itemsize == 40


def _of_points(p, hw):
    """D22 over the points p [S, 2] (float64 of f32 values), each widened by hw."""
    box = EMPTY.copy()
    if np.isnan(hw):
        return box
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = p[:, 0], p[:, 1]
        box[0] = np.fmin.reduce(x - hw, initial=INF)
        box[1] = np.fmin.reduce(y - hw, initial=INF)
        box[2] = np.fmax.reduce(x + hw, initial=-INF)
        box[3] = np.fmax.reduce(y + hw, initial=-INF)
    return box


def _circle(bbox, ellipse):
    x0, y0, x1, y1 = (np.float64(v) for v in bbox)
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    rx, ry = cx - x0, cy - y0
    if ellipse:
        if not (rx > 0 and ry > 0):
            return EMPTY.copy()
    else:
        rx = ry = min(rx, ry)
    return np.array([cx - rx, cy - ry, cx + rx, cy + ry], np.float64)


def skipped_items(scene, skip_transparent):
    """bool [n_items]: the items PM_HIT_SKIP_TRANSPARENT skips (as D13 skips them: a Line, Fill or Polyline of alpha 0)."""
    sc = bytes(scene)
    items = np_hit.flat_items(sc)
    out = np.zeros(len(items), bool)
    for i, (at, _) in enumerate(items):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        if skip_transparent and tag in (LINE, FILL, POLY):
            (rgba,) = struct.unpack_from("<I", sc, at + (4 if tag == POLY else 8))
            out[i] = rgba >> 24 == 0
    return out


def item_bounds(scene, skip_transparent=False):
    """float64 [n_items, 4]: {x0, y0, x1, y1} of every item in flat paint order."""
    sc = bytes(scene)
    items = np_hit.flat_items(sc)
    skipped = skipped_items(sc, skip_transparent)
    out = np.tile(EMPTY, (len(items), 1))
    for i, (at, bbox) in enumerate(items):
        (word,) = struct.unpack_from("<I", sc, at)
        tag = word & 0xFFFF
        if skipped[i]:
            continue
        if tag == CIRCLE:
            out[i] = _circle(bbox, bool(word & CIRCLE_ELLIPSE))
        elif tag == FILL:
            (flags,) = struct.unpack_from("<I", sc, at + 4)
            p = np_hit._points(sc, at).astype(np.float64)
            if flags & FILL_COMPOUND:
                p = p[~np.isnan(p[:, 0])]   # a separator is no point
            out[i] = _of_points(p, np.float64(0.0))
        elif tag == LINE:
            w, ax, ay, bx, by = struct.unpack_from("<5f", sc, at + 12)
            out[i] = _of_points(np.array([[ax, ay], [bx, by]], np.float32).astype(np.float64), np.float64(0.5) * np.float64(np.float32(w)))
        elif tag == POLY:
            (w,) = struct.unpack_from("<f", sc, at + 8)
            out[i] = _of_points(np_hit._points(sc, at).astype(np.float64), np.float64(0.5) * np.float64(np.float32(w)))
    return out + 0.0


def boxed(boxes):
    """bool [n]: x0 <= x1 and y0 <= y1."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return (b[:, 0] <= b[:, 2]) & (b[:, 1] <= b[:, 3])


def union_bounds(scene, n_labels, labels=None, words=None, mask=3, skip_transparent=False, boxes=None):
    """LABEL_BOUNDS [n_labels]: per label the union of the boxes of the items that take part with it, how many, how many boxed.
    boxes: item_bounds(scene, skip_transparent), if the caller has them already."""
    b = item_bounds(scene, skip_transparent) if boxes is None else boxes
    n = len(b)
    part = ~skipped_items(scene, skip_transparent)
    if words is not None:
        part &= (np.asarray(words, np.uint32)[:n] & np.uint32(mask)) != 0
    lab = np.zeros(n, np.uint32) if labels is None else np.asarray(labels, np.uint32)[:n]
    part &= lab < n_labels
    out = np.zeros(n_labels, LABEL_BOUNDS)
    out["box"] = EMPTY
    is_boxed = boxed(b)
    for i in np.flatnonzero(part):
        rec = out[lab[i]]
        rec["box"][:2] = np.fmin(rec["box"][:2], b[i, :2])
        rec["box"][2:] = np.fmax(rec["box"][2:], b[i, 2:])
        rec["n_items"] += 1
        rec["n_boxed"] += int(is_boxed[i])
    out["box"] = out["box"] + 0.0
    return out
