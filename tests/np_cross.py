"""Independent numpy restatement of snapping to intersections, decision D23: the nearest crossing of two edges of a
scene byte buffer to a query {x, y, r}.  Written from the decision's text, not from the kernel: no boxes, no index, every edge's
near test and every pair of near edges is evaluated.  Test infrastructure.

The edges and the near test are D21's, taken from tests/np_snap.py as they are (its item_offers and edge_d2).  All arithmetic is
numpy float64 on the scene's f32 values and the query's f32 values, one ufunc per written operation, in the written order (numpy
never fuses a multiply with an add), so t, u, the point and d2 are the decision's bit for bit.

Edges are listed in the order "precedes": from the topmost item down, by index within an item.  Two evaluation orders give the same
records:
  per_first=False  every pair (i, j), i < j, of the near list at once, row by row: the first minimum of d2 is the winner (numpy's
                   argmin names the first);
  per_first=True   every first edge's own winner (the smallest d2, then the second edge that precedes), then the first edges in
                   order, a later one replacing the running winner only when its d2 is SMALLER.
"""
import numpy as np

import np_snap

NONE = 0xFFFFFFFF
INTERSECTION, TOO_MANY = 3, 4
MAX_NEAR = 512
RECORD = np.dtype(np_snap.RECORD.descr + [("item2", "<u4"), ("index2", "<u4"), ("u", "<f4"), ("n_near", "<u4")])
assert RECORD.itemsize == 48 and [RECORD.fields[k][1] for k in RECORD.names] == [0, 4, 8, 12, 16, 20, 24, 32, 36, 40, 44]


class Edges:
    """Every edge of the scene in the order "precedes": item int64 [E], index int64 [E], a, b f32 [E, 2]."""

    def __init__(self, scene, skip_transparent=False, skip_items=None):
        offers = np_snap._offers(scene, skip_transparent, skip_items)
        item, index, a, b = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 2), np.float32)], [np.zeros((0, 2), np.float32)]
        for i in range(len(offers) - 1, -1, -1):
            if offers[i] is None:
                continue
            _, _, ei, ea, eb = offers[i]
            assert (np.diff(ei) > 0).all()
            item.append(np.full(len(ei), i, np.int64))
            index.append(np.asarray(ei, np.int64))
            a.append(ea)
            b.append(eb)
        self.item, self.index, self.a, self.b = np.concatenate(item), np.concatenate(index), np.concatenate(a), np.concatenate(b)
        self.n = len(self.item)


def near_mask(E, Q, sl=slice(None)):
    """bool [n, E]: D21's edge d2 <= r * r, for valid queries."""
    if E.n == 0:
        return np.zeros((len(Q.x[sl]), 0), bool)
    with np.errstate(invalid="ignore"):
        return (np_snap.edge_d2(E.a, E.b, Q.x[sl], Q.y[sl]) <= Q.r2[sl][:, None]) & Q.valid[sl][:, None]


def pair_parts(a, b, c, d, x, y):
    """(shared, den, t, u, X, Y, d2), float64 / bool, broadcast: D23's operations on the pair e: a -> b, f: c -> d (f32 [..., 2])."""
    shared = (a == c).all(axis=-1) | (a == d).all(axis=-1) | (b == c).all(axis=-1) | (b == d).all(axis=-1)
    ax, ay, bx, by, cx, cy, dx_, dy_ = (v.astype(np.float64) for v in (a[..., 0], a[..., 1], b[..., 0], b[..., 1], c[..., 0], c[..., 1], d[..., 0], d[..., 1]))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rx, ry, sx, sy = bx - ax, by - ay, dx_ - cx, dy_ - cy
        den = rx * sy - ry * sx
        wx, wy = cx - ax, cy - ay
        t = (wx * sy - wy * sx) / den
        u = (wx * ry - wy * rx) / den
        X, Y = ax + rx * t, ay + ry * t
        dx, dy = x - X, y - Y
        return shared, den, t, u, X, Y, dx * dx + dy * dy


def qualifies(a, b, c, d, x, y, r2):
    """(ok bool, parts): is the pair a candidate that qualifies."""
    p = pair_parts(a, b, c, d, x, y)
    shared, den, t, u, _, _, d2 = p
    with np.errstate(invalid="ignore"):
        ok = ~shared & (den != 0) & (0 <= t) & (t <= 1) & (0 <= u) & (u <= 1) & (d2 <= r2)
    return ok, p


def _first_min(ok, d2):
    """(position of the first smallest d2 among ok, found)."""
    if not ok.any():
        return 0, False
    return int(np.argmin(np.where(ok, d2, np.inf))), True


def cross(scene, xyr, skip_transparent=False, skip_items=None, per_first=False):
    """RECORD [n]: D23's answer for float32 queries [n, 3] {x, y, r}."""
    E = Edges(bytes(scene), skip_transparent, skip_items)
    Q = np_snap.Queries(xyr)
    out = np.zeros(Q.n, RECORD)
    out["item"] = NONE
    for q0 in range(0, Q.n, 256):   # (memory)
        near = near_mask(E, Q, slice(q0, q0 + 256))
        for q in range(q0, min(q0 + 256, Q.n)):
            if not Q.valid[q]:
                continue
            ix = np.flatnonzero(near[q - q0])       # in the order "precedes"
            n = len(ix)
            out["n_near"][q] = n
            if n > MAX_NEAR:
                out["kind"][q] = TOO_MANY
                continue
            if n < 2:
                continue
            i, j = np.triu_indices(n, 1)            # row by row: the first edge in order, then the second
            ok, (_, _, t, u, X, Y, d2) = qualifies(E.a[ix[i]], E.b[ix[i]], E.a[ix[j]], E.b[ix[j]], Q.x[q], Q.y[q], Q.r2[q])
            if per_first:
                w, found, best = 0, False, np.inf
                starts = np.concatenate([[0], np.cumsum(np.arange(n - 1, 0, -1))])
                for k in range(n - 1):
                    at, got = _first_min(ok[starts[k] : starts[k + 1]], d2[starts[k] : starts[k + 1]])
                    if got and d2[starts[k] + at] < best:
                        w, found, best = int(starts[k]) + at, True, d2[starts[k] + at]
            else:
                w, found = _first_min(ok, d2)
            if not found:
                continue
            e, f = ix[i[w]], ix[j[w]]
            out[q] = (E.item[e], INTERSECTION, E.index[e], np.float32(t[w]), np.float32(X[w]), np.float32(Y[w]), d2[w], E.item[f], E.index[f], np.float32(u[w]), n)
    return out
