"""Independent statement of item crossings, decision D29: every point where an edge of item A crosses an edge of item
B, or where an item crosses itself.  Written from the decision's text over np_measure's segment lists, not from the kernel: no
chunk boxes, no lanes, no ranks -- every pair of edges is asked.  It shares no code with np_cross.  Test infrastructure.

All arithmetic is numpy float64 on the scene's f32 values, one ufunc per written operation, in the written order (numpy never fuses
a multiply with an add), rounded once to f32 where the decision says so.

Every answer is evaluated in two loop orders that must agree record for record:
  * i-major: the pairs as an array [edges of A, edges of B], rows of A at a time;
  * j-major: B's edges outside, A's inside -- in plain Python scalars while the request has at most SCALAR_PAIRS pairs, as an
    array [edges of B, edges of A] beyond -- and the crossings sorted by (i, j) afterwards.
One deduction keeps the far-apart limit case affordable: if the union of A's edge boxes and the union of B's do not meet (the closed
comparisons of the box rule), no pair passes the box rule, and the answer is empty without a pair being asked.
"""
import struct

import numpy as np

import np_hit
import np_measure as nm
from np_hit import FILL, LINE, POLY

TRUNCATED, TOO_MANY = 1, 2                 # PM_CROSSINGS_TRUNCATED / _TOO_MANY
MAX_PAIRS = 1 << 28                        # PM_CROSSINGS_MAX_PAIRS
SIDE_POS, SIDE_NEG = 1, 2                  # PM_CROSSING_SIDE_POS / _NEG
SCALAR_PAIRS = 4096

CROSSINGS_QUERY = np.dtype([("item_a", "<u4"), ("item_b", "<u4"), ("first", "<u4"), ("cap", "<u4")])
CROSSING = np.dtype([("item_a", "<u4"), ("index_a", "<u4"), ("t", "<f4"), ("reserved_a", "<u4"), ("item_b", "<u4"), ("index_b", "<u4"), ("u", "<f4"),
                     ("reserved_b", "<u4"), ("x", "<f4"), ("y", "<f4"), ("side", "<u4"), ("reserved", "<u4")])
CROSSINGS_INFO = np.dtype([("n_crossings", "<u4"), ("flags", "<u4"), ("n_a", "<u4"), ("n_b", "<u4")])
assert (CROSSINGS_QUERY.itemsize, CROSSING.itemsize, CROSSINGS_INFO.itemsize) == (16, 48, 16)


def index_ranges(scene, skip_transparent=False):
    """K(item) for every item of the scene: 1 for a Line, points - 1 for a Polyline of two points or more, entries (separators
    included) for a Fill, 0 for everything without a walk."""
    sc = bytes(scene)
    out = []
    for at, _ in np_hit.flat_items(sc):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        k = 0
        if tag in (LINE, FILL, POLY):
            rgba = struct.unpack_from("<I", sc, at + (4 if tag == POLY else 8))[0]
            if not (skip_transparent and rgba >> 24 == 0):
                npt = struct.unpack_from("<I", sc, at + 12)[0]
                k = 1 if tag == LINE else (npt if tag == FILL else max(npt, 1) - 1)
        out.append(k)
    return out


def edges(w):
    """(indices int64 [n], ends f32 [n, 4] = a.x, a.y, b.x, b.y) of the walk's segments with both ends finite."""
    ks = [k for k, a, b, _ in w.segs if np.isfinite(a).all() and np.isfinite(b).all()]
    keep = set(ks)
    ends = np.array([(a[0], a[1], b[0], b[1]) for k, a, b, _ in w.segs if k in keep], np.float32).reshape(-1, 4)
    return np.array(ks, np.int64), ends


def pair(e, f):
    """D29 on ONE pair, e = a -> b and f = c -> d as four f32 each: None, or (t, u, x, y, side) rounded once."""
    F, D = np.float32, np.float64
    ax, ay, bx, by = (F(v) for v in e)
    cx, cy, dx, dy = (F(v) for v in f)
    if not (max(ax, bx) >= min(cx, dx) and max(cx, dx) >= min(ax, bx) and max(ay, by) >= min(cy, dy) and max(cy, dy) >= min(ay, by)):
        return None
    if (ax == cx and ay == cy) or (ax == dx and ay == dy) or (bx == cx and by == cy) or (bx == dx and by == dy):
        return None
    ax, ay, bx, by, cx, cy, dx, dy = (D(v) for v in (ax, ay, bx, by, cx, cy, dx, dy))
    with np.errstate(all="ignore"):
        rx, ry = bx - ax, by - ay
        sx, sy = dx - cx, dy - cy
        den = rx * sy - ry * sx
        if not den != 0:
            return None
        wx, wy = cx - ax, cy - ay
        t = (wx * sy - wy * sx) / den
        u = (wx * ry - wy * rx) / den
        if not (0 <= t <= 1 and 0 <= u <= 1):
            return None
        x, y = ax + rx * t, ay + ry * t
        return F(t), F(u), F(x), F(y), SIDE_POS if den > 0 else SIDE_NEG


def _grid(EA, EB, a_axis):
    """The rule on every pair of the edges EA x EB at once.  a_axis 0: arrays [A, B]; 1: arrays [B, A].  Returns (mask, t, u, x, y, den)."""
    shape_a, shape_b = ((-1, 1), (1, -1)) if a_axis == 0 else ((1, -1), (-1, 1))
    ax, ay, bx, by = (EA[:, k].reshape(shape_a) for k in range(4))
    cx, cy, dx, dy = (EB[:, k].reshape(shape_b) for k in range(4))
    box = (np.maximum(ax, bx) >= np.minimum(cx, dx)) & (np.maximum(cx, dx) >= np.minimum(ax, bx)) & (np.maximum(ay, by) >= np.minimum(cy, dy)) & \
        (np.maximum(cy, dy) >= np.minimum(ay, by))
    share = ((ax == cx) & (ay == cy)) | ((ax == dx) & (ay == dy)) | ((bx == cx) & (by == cy)) | ((bx == dx) & (by == dy))
    ax, ay, bx, by, cx, cy, dx, dy = (v.astype(np.float64) for v in (ax, ay, bx, by, cx, cy, dx, dy))
    with np.errstate(all="ignore"):
        rx, ry = bx - ax, by - ay
        sx, sy = dx - cx, dy - cy
        den = rx * sy - ry * sx
        wx, wy = cx - ax, cy - ay
        t = (wx * sy - wy * sx) / den
        u = (wx * ry - wy * rx) / den
        mask = box & ~share & (den != 0) & (0 <= t) & (t <= 1) & (0 <= u) & (u <= 1)
        x, y = ax + rx * t, ay + ry * t
    return mask, t, u, x, y, den


def _boxes_meet(EA, EB):
    if not len(EA) or not len(EB):
        return False
    lo = lambda E, k: min(E[:, k].min(), E[:, k + 2].min())  # noqa: E731
    hi = lambda E, k: max(E[:, k].max(), E[:, k + 2].max())  # noqa: E731
    return all(hi(EA, k) >= lo(EB, k) and hi(EB, k) >= lo(EA, k) for k in (0, 1))


def _i_major(ka, EA, kb, EB, self_pairs, rows=256):
    out = []
    for r0 in range(0, len(EA), rows):
        mask, t, u, x, y, den = _grid(EA[r0:r0 + rows], EB, 0)
        if self_pairs:
            mask &= ka[r0:r0 + rows, None] < kb[None, :]
        for r, c in zip(*np.nonzero(mask)):         # (row-major: i, then j, ascending)
            out.append((int(ka[r0 + r]), int(kb[c]), np.float32(t[r, c]), np.float32(u[r, c]), np.float32(x[r, c]), np.float32(y[r, c]),
                        SIDE_POS if den[r, c] > 0 else SIDE_NEG))
    return out


def _j_major(ka, EA, kb, EB, self_pairs, rows=256):
    out = []
    if len(EA) * len(EB) <= SCALAR_PAIRS:
        for j, f in zip(kb.tolist(), EB):
            for i, e in zip(ka.tolist(), EA):
                got = None if self_pairs and not i < j else pair(e, f)
                if got is not None:
                    out.append((i, j) + got)
    else:
        for r0 in range(0, len(EB), rows):
            mask, t, u, x, y, den = _grid(EA, EB[r0:r0 + rows], 1)
            if self_pairs:
                mask &= ka[None, :] < kb[r0:r0 + rows, None]
            for r, c in zip(*np.nonzero(mask)):
                out.append((int(ka[c]), int(kb[r0 + r]), np.float32(t[r, c]), np.float32(u[r, c]), np.float32(x[r, c]), np.float32(y[r, c]),
                            SIDE_POS if den[r, c] > 0 else SIDE_NEG))
    return sorted(out, key=lambda c: (c[0], c[1]))


def as_records(rows):
    """Tuples in the order of CROSSING's fields as records."""
    out = np.zeros(len(rows), CROSSING)
    for k, row in enumerate(rows):
        out[k] = row
    return out


def item_crossings(ws, item_a, item_b):
    """The crossings of one request as tuples in CROSSING's field order, numbered by (i, j) ascending; both loop orders, which must agree."""
    none = nm.Walk()
    wa, wb = ws[item_a] if item_a < len(ws) else none, ws[item_b] if item_b < len(ws) else none
    ka, EA = edges(wa)
    kb, EB = edges(wb)
    if not _boxes_meet(EA, EB):
        return []
    self_pairs = item_a == item_b
    first, second = _i_major(ka, EA, kb, EB, self_pairs), _j_major(ka, EA, kb, EB, self_pairs)
    rows = [(item_a, i, t, 0, item_b, j, u, 0, x, y, side, 0) for i, j, t, u, x, y, side in first]
    again = [(item_a, i, t, 0, item_b, j, u, 0, x, y, side, 0) for i, j, t, u, x, y, side in second]
    assert as_records(rows).tobytes() == as_records(again).tobytes(), (item_a, item_b, "the two loop orders disagree")
    return rows


def crossings(scene, reqs, skip_transparent=False, ws=None, out_cap=None, Ks=None):
    """Requests (item_a, item_b, first, cap).  Returns (writes {row: record tuple}, infos CROSSINGS_INFO [n], per request the tuples of
    its whole answer).  out_cap None: no limit."""
    ws = nm.walks(scene, skip_transparent) if ws is None else ws
    Ks = index_ranges(scene, skip_transparent) if Ks is None else Ks
    writes, answers = {}, []
    infos = np.zeros(len(reqs), CROSSINGS_INFO)
    memo = {}
    for n, (item_a, item_b, first, cap) in enumerate(reqs):
        n_a, n_b = Ks[item_a] if item_a < len(Ks) else 0, Ks[item_b] if item_b < len(Ks) else 0
        if n_a * n_b > MAX_PAIRS:
            infos[n] = (0, TOO_MANY, n_a, n_b)
            answers.append([])
            continue
        if (item_a, item_b) not in memo:
            memo[(item_a, item_b)] = item_crossings(ws, item_a, item_b)
        rows = memo[(item_a, item_b)]
        wrote = 0
        for p, row in enumerate(rows):
            if p < cap and (out_cap is None or first + p < out_cap):
                writes[first + p] = row
                wrote += 1
        infos[n] = (len(rows), TRUNCATED if wrote < len(rows) else 0, n_a, n_b)
        answers.append(rows)
    return writes, infos, answers


def expected_buffer(writes, rows, fill):
    """int32 [rows, 12]: the writes, and `fill` in every other word."""
    out = np.full((rows, 12), fill, np.int32)
    for at, row in writes.items():
        out[at] = as_records([row]).view(np.int32)
    return out


def records(reqs):
    q = np.zeros(len(reqs), CROSSINGS_QUERY)
    for k, r in enumerate(reqs):
        q[k] = r
    return q


def packed(pairs, caps):
    """[(item_a, item_b)] with caps, laid out one behind the other: the requests and the total."""
    out, at = [], 0
    for (a, b), cap in zip(pairs, caps):
        out.append((a, b, at, cap))
        at += cap
    return out, at
