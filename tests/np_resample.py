"""Independent statement of resampling, decision D26: the positions a request names along an item, the info record
and the number of unclamped answers, in Python integers from the decision's text.  No waves, no cursor: the positions are listed
one by one.  The point records are not restated: D26 defines them as np_measure.points_at_length at these positions, and
`resample` below is that relation written out.  Test infrastructure.
"""
import numpy as np

import np_measure as nm

STEP, EVEN = 0, 1                         # PM_RESAMPLE_STEP / _EVEN
MAX_COUNT = 1 << 20                       # PM_RESAMPLE_MAX_COUNT
INVALID = 0xFFFFFFFF                      # PM_RESAMPLE_INVALID
U64_MAX = (1 << 64) - 1

RESAMPLE_QUERY = np.dtype([("item", "<u4"), ("mode", "<u4"), ("count", "<u4"), ("first", "<u4"), ("start", "<u8"), ("step", "<u8")])
RESAMPLE_INFO = np.dtype([("length", "<u8"), ("n_unclamped", "<u4"), ("kind", "<u4")])
assert (RESAMPLE_QUERY.itemsize, RESAMPLE_INFO.itemsize) == (32, 16)


def valid(mode, count, start, step):
    """Can the device answer the request."""
    return mode in (STEP, EVEN) and count <= MAX_COUNT and (mode == STEP or (start == 0 and step == 0))


def even_m(kind, count):
    """The number of gaps of an even request: the last sample of an open item is its end, sample `count` of a closed one would be
    its start again."""
    if kind == nm.OPEN:
        return max(count - 1, 0)
    return count if kind == nm.CLOSED else 0


def position(mode, j, start=0, step=0, T=0, m=0):
    """s_j."""
    if mode == STEP:
        return min(start + j * step, U64_MAX)
    if m == 0:
        return 0
    return j * (T // m) + min(j, T % m)


def positions(mode, count, start=0, step=0, T=0, kind=nm.NONE):
    m = even_m(kind, count)
    return [position(mode, j, start, step, T, m) for j in range(count)]


def cnt(x, mode, count, start=0, step=0, T=0, m=0):
    """The number of j < count with s_j < x, in closed form: what lets a walk know which samples a stretch [Q0, Q1) owns without
    listing them.  Step mode: none at x <= start, all for step == 0, else the j up to (x - start - 1) div step (a saturated position
    is 2^64 - 1, below no x).  Even mode: two arithmetic runs -- s_j = j (d + 1) for j <= r, and r + j d after."""
    if mode == STEP:
        if x <= start:
            return 0
        if step == 0:
            return count
        return min(count, (x - start - 1) // step + 1)
    if x <= 0:
        return 0
    if m == 0:
        return count
    d, r = T // m, T % m
    if x <= r * (d + 1):                                   # within the first run (x >= 1, so d + 1 divides something)
        return min(count, (x - 1) // (d + 1) + 1)
    if d == 0:                                             # the second run stands still at r
        return count
    return min(count, (x - r - 1) // d + 1)


def unclamped(w, ss):
    """How many of the positions ss have an answer on the walk w that is not "none" and lacks CLAMPED."""
    if w.kind == nm.NONE or (not any(sg[3] > 0 for sg in w.segs) and w.first is None):
        return 0
    return sum(1 for s in ss if s <= w.T)


def resample(scene, requests, skip_transparent=False, ws=None, out_cap=None):
    """requests: (item, mode, count, first, start, step).  Returns (writes, infos): writes a dict {record index: LENGTH_POINT
    record} of every record the requests write, in the order given (a later request overwrites an earlier one's), none at or beyond
    out_cap; infos RESAMPLE_INFO [n]."""
    ws = nm.walks(scene, skip_transparent) if ws is None else ws
    writes = {}
    infos = np.zeros(len(requests), RESAMPLE_INFO)
    asked = {}                 # (item, s) -> the one-record answer of np_measure.points_at_length: many requests share positions
    for k, (item, mode, count, first, start, step) in enumerate(requests):
        item, mode, count, first, start, step = int(item), int(mode), int(count), int(first), int(start), int(step)
        if not valid(mode, count, start, step):
            infos[k] = (0, 0, INVALID)
            continue
        w = ws[item] if item < len(ws) else nm.Walk()
        ss = positions(mode, count, start, step, w.T, w.kind)
        for j, s in enumerate(ss):
            if out_cap is None or first + j < out_cap:
                if (item, s) not in asked:
                    asked[(item, s)] = nm.points_at_length(scene, [(item, s)], skip_transparent, ws)[0]
                writes[first + j] = asked[(item, s)]
        infos[k] = (w.T, unclamped(w, ss), w.kind)
    return writes, infos


def expected_buffer(writes, n_rows, blank_word):
    """The int32 [n_rows, 8] buffer that started as blank_word everywhere after the writes."""
    buf = np.full((n_rows, 8), blank_word, np.int32)
    for at, rec in writes.items():
        buf[at] = np.asarray(rec).reshape(1).view(np.int32)
    return buf


def packed(requests):
    """The requests with `first` set to the sum of the counts before: [(item, mode, count, first, start, step)] and the total."""
    out, total = [], 0
    for item, mode, count, start, step in requests:
        out.append((item, mode, count, total, start, step))
        total += count
    return out, total


def records(requests):
    q = np.zeros(len(requests), RESAMPLE_QUERY)
    for k, (item, mode, count, first, start, step) in enumerate(requests):
        q[k] = (item, mode, count, first, start, step)
    return q
