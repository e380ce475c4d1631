"""Independent statement of trimming, decision D27: the piece of an item between two lengths as a list of vertices,
written from the decision's text in Python integers.  No waves, no scan, no ballots: the segments of np_measure's walk are visited
one by one, the previous covered segment's B is a Python variable.  Test infrastructure; it shares no code with the kernel.
"""
import numpy as np

import np_measure as nm

RANGE, PART = 0, 1                        # PM_TRIM_RANGE / _PART
MAX_PARTS = 1 << 20                       # PM_TRIM_MAX_PARTS
MOVE, CUT = 1, 2                          # PM_TRIM_MOVE / _CUT
TRUNCATED, END_CLAMPED = 1, 2             # PM_TRIM_TRUNCATED / _END_CLAMPED
INVALID = 0xFFFFFFFF                      # PM_TRIM_INVALID
U64_MAX = (1 << 64) - 1

TRIM_QUERY = np.dtype([("item", "<u4"), ("mode", "<u4"), ("first", "<u4"), ("cap", "<u4"), ("s0", "<u8"), ("s1", "<u8")])
TRIM_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("index", "<u4"), ("flags", "<u4")])
TRIM_INFO = np.dtype([("length", "<u8"), ("n_vertices", "<u4"), ("n_runs", "<u4"), ("kind", "<u4"), ("flags", "<u4")])
assert (TRIM_QUERY.itemsize, TRIM_VERTEX.itemsize, TRIM_INFO.itemsize) == (32, 16, 24)


def valid(mode, s0, s1):
    """Can the device answer the request."""
    if mode == RANGE:
        return s0 <= s1
    return mode == PART and 1 <= s1 <= MAX_PARTS and s0 < s1


def boundary(T, m, i):
    """b_i: D26's even position i of m gaps."""
    return i * (T // m) + min(i, T % m)


def ends(mode, s0, s1, T):
    """[lo, hi] of a valid request on an item of length T."""
    if mode == RANGE:
        return min(s0, T), min(s1, T)
    return boundary(T, s1, s0), boundary(T, s1, s0 + 1)


def starts(w):
    """[(k, a, b, q, Q)] of a walk (kept with the walk: the case lists ask thousands of pieces of one item)."""
    out = getattr(w, "_starts", None)
    if out is None:
        out, Q = [], 0
        for k, a, b, q in w.segs:
            out.append((k, a, b, q, Q))
            Q += q
        w._starts = out
    return out


def covered(w, lo, hi):
    """The covered segments of the piece [lo, hi], in increasing k."""
    if lo >= hi:
        return []
    return [sg for sg in starts(w) if sg[4] < hi and sg[4] + sg[3] > lo]


def _cut(a, b, Q, q, s):
    """D25's point at s inside the segment (Q < s < Q + q): a + (b - a) * t in binary64, t = (s - Q) / q, rounded once to f32."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t64 = np.float64(s - Q) / np.float64(q)
        return np.float32(a64[0] + (b64[0] - a64[0]) * t64), np.float32(a64[1] + (b64[1] - a64[1]) * t64)


def _equal(p, q):
    """f32 values, both coordinates: -0 equals 0, a NaN nothing."""
    return bool(np.float32(p[0]) == np.float32(q[0]) and np.float32(p[1]) == np.float32(q[1]))


def vertices(w, lo, hi):
    """The piece's vertices [(x, y, index, flags)] in emission order."""
    out, prev = [], None
    for k, a, b, q, Q in covered(w, lo, hi):
        A, fa = ((a[0], a[1]), 0) if lo <= Q else (_cut(a, b, Q, q, lo), CUT)
        B, fb = ((b[0], b[1]), 0) if hi >= Q + q else (_cut(a, b, Q, q, hi), CUT)
        if prev is None or not _equal(A, prev):
            out.append((A[0], A[1], k, MOVE | fa))
        out.append((B[0], B[1], k, fb))
        prev = B
    return out


def trim(scene, requests, skip_transparent=False, ws=None, out_cap=None):
    """requests: (item, mode, first, cap, s0, s1).  Returns (writes, infos, pieces): writes a dict {row: (x, y, index, flags, item)}
    of every row the requests write, in the order given (a later request overwrites an earlier one's), none at or beyond out_cap;
    infos TRIM_INFO [n]; pieces the whole vertex list of every request (None for an invalid one)."""
    ws = nm.walks(scene, skip_transparent) if ws is None else ws
    writes, pieces = {}, []
    infos = np.zeros(len(requests), TRIM_INFO)
    for n, (item, mode, first, cap, s0, s1) in enumerate(requests):
        item, mode, first, cap, s0, s1 = int(item), int(mode), int(first), int(cap), int(s0), int(s1)
        if not valid(mode, s0, s1):
            infos[n] = (0, 0, 0, INVALID, 0)
            pieces.append(None)
            continue
        w = ws[item] if item < len(ws) else nm.Walk()
        lo, hi = ends(mode, s0, s1, w.T)
        vs = vertices(w, lo, hi)
        pieces.append(vs)
        truncated = False
        for p, v in enumerate(vs):
            if p < cap and (out_cap is None or first + p < out_cap):
                writes[first + p] = v + (item,)
            else:
                truncated = True
        flags = (TRUNCATED if truncated else 0) | (END_CLAMPED if mode == RANGE and s1 > w.T else 0)
        infos[n] = (w.T, len(vs), sum(1 for v in vs if v[3] & MOVE), w.kind, flags)
    return writes, infos, pieces


def expected_buffer(writes, n_rows, blank_word):
    """The int32 [n_rows, 4] buffer that started as blank_word everywhere after the writes."""
    buf = np.full((n_rows, 4), blank_word, np.int32)
    if writes:
        rows = np.array(sorted(writes), np.int64)
        rec = np.zeros(len(rows), TRIM_VERTEX)
        for f, col in (("x", 0), ("y", 1), ("index", 2), ("flags", 3)):
            rec[f] = [writes[int(at)][col] for at in rows]
        buf[rows] = rec.view(np.int32).reshape(-1, 4)
    return buf


def unpromised_rows(writes, ws):
    """The rows whose x, y are not promised: a CUT vertex on a segment with a non-finite end."""
    return [at for at, v in writes.items() if v[3] & CUT and v[4] < len(ws) and nm.has_non_finite_end(ws[v[4]], v[2])]


def as_records(vs):
    """A vertex list as TRIM_VERTEX [n]."""
    rec = np.zeros(len(vs), TRIM_VERTEX)
    for f, col in (("x", 0), ("y", 1), ("index", 2), ("flags", 3)):
        rec[f] = [v[col] for v in vs]
    return rec


def packed(requests, caps):
    """(item, mode, s0, s1) with the caps given, `first` the sum of the caps before: [(item, mode, first, cap, s0, s1)] and the total."""
    out, total = [], 0
    for (item, mode, s0, s1), cap in zip(requests, caps):
        out.append((item, mode, total, cap, s0, s1))
        total += cap
    return out, total


def records(requests):
    q = np.zeros(len(requests), TRIM_QUERY)
    for k, (item, mode, first, cap, s0, s1) in enumerate(requests):
        q[k] = (item, mode, first, cap, s0, s1)
    return q
