"""Independent numpy statement of decision D15: a dashed styled stroke as ONE compound non-zero Fill item whose
entries are the D14 outlines (tests/np_stroke.py) of its dashes.  Written from the decision's text, not from the kernels: the
on-intervals are walked one by one in Python integers, the walk's positions Q are an integer cumsum kept whole, the points on the
walk come from searchsorted over it.  Test infrastructure.

Lengths are integers in units of 2^-16 px throughout; a cut point is binary64 on the f32 values, one ufunc per written operation,
rounded once to f32.

    cut(pts, closed, pattern, offset, width_scale)     -> UNDASHED / CLOSED_WHOLE / a list of f32 poly-lines [n, 2], in order
    outline_dashed(pts, closed, width, cap, join, miter_half, pattern, offset, width_scale)
                                                       -> (entries uint32 [E, 2], box)
    entry_count(polys, cap, join, L)                   -> D15's closed form of the entry count
    apply(scene, specs)                                -> the dashed scene's bytes, from the un-dashed poly-line scene
    specs_from_pathset(ps, width_scale)                -> per item: None, or (closed, cap, join, miter_half, dash) with dash = None
                                                          or (pattern, offset, width_scale)
"""
import struct

import numpy as np

import np_stroke

UNDASHED, CLOSED_WHOLE = "undashed", "closed-whole"
ONE = 65536.0
CAP = 1 << 32
OFFSET_CAP = 1 << 62


def fix(v, cap=CAP):
    """min(floor(v * 65536 + 0.5), cap) as an integer; NaN: 0.  v: binary64."""
    v = np.float64(v)
    if v != v:
        return 0
    f = np.floor(v * ONE + 0.5)
    return cap if f >= float(cap) else int(f)


def pattern_fixed(pattern, offset, width_scale):
    """(Pf [c' + 1] prefix sums, G, phi) of the scaled pattern."""
    ws = np.float32(width_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        g = [fix(np.float64(np.float32(v) * ws)) for v in pattern]
        wo = np.float32(offset) * ws
    if len(g) % 2:
        g = g + g
    pf = [0]
    for x in g:
        pf.append(pf[-1] + x)
    G = pf[-1]
    go = fix(abs(np.float64(wo)), OFFSET_CAP)
    phi = 0 if G == 0 else (go % G if wo >= 0 else (G - go % G) % G)
    return pf, G, phi


def walk(pts, closed):
    """(W f32 [N, 2], Q int64 [N]) of the poly-line."""
    P = np.asarray(pts, np.float32).reshape(-1, 2)
    W = np.concatenate([P, P[:1]]) if closed else P
    d = W[1:].astype(np.float64) - W[:-1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    q = [fix(x) for x in ln]
    Q = np.concatenate([[0], np.cumsum(np.array(q, np.int64))]).astype(np.int64) if len(q) else np.zeros(1, np.int64)
    return W, Q


def _point(W, Q, s, end_rule):
    if end_rule:
        k = int(np.searchsorted(Q, s, "left")) - 1   # the smallest k with Q[k + 1] >= s
    else:
        k = int(np.searchsorted(Q, s, "right")) - 1  # the largest k with Q[k] <= s
    if s == Q[k]:
        return W[k]
    if s == Q[k + 1]:
        return W[k + 1]
    a, b = W[k].astype(np.float64), W[k + 1].astype(np.float64)
    t = np.float64(s - Q[k]) / np.float64(Q[k + 1] - Q[k])
    with np.errstate(invalid="ignore", over="ignore"):
        return (a + (b - a) * t).astype(np.float32)


def cut(pts, closed, pattern, offset, width_scale):
    pf, G, phi = pattern_fixed(pattern, offset, width_scale)
    W, Q = walk(pts, closed)
    T = int(Q[-1])
    gaps = [pf[j + 1] - pf[j] for j in range(1, len(pf) - 1, 2)]
    if G == 0 or not any(gaps) or T == 0:
        return UNDASHED
    dashes = []  # (A, B, A', B')
    r = 0
    while r * G - phi < T:
        for j in range(0, len(pf) - 1, 2):
            A, B = r * G + pf[j] - phi, r * G + pf[j + 1] - phi
            if closed and A <= 0 and B >= T:
                return CLOSED_WHOLE
            A1, B1 = max(A, 0), min(B, T)
            if A1 < B1 or (A == B and 0 <= A < T):
                dashes.append((A, B, A1, B1))
        r += 1
    polys = []
    for A, B, A1, B1 in dashes:
        start = _point(W, Q, A1, False)
        end = _point(W, Q, B1, True) if A != B else start
        lo, hi = int(np.searchsorted(Q, A1, "right")), int(np.searchsorted(Q, B1, "left"))
        polys.append(np.concatenate([start[None], W[lo:hi], end[None]]).astype(np.float32))
    if closed and len(dashes) >= 2:
        (A0, B0, _, _), (Al, Bl, _, _) = dashes[0], dashes[-1]
        if A0 <= 0 < B0 and Al < T <= Bl:
            polys[0] = np.concatenate([polys[-1], polys[0]])
            polys.pop()
    return polys


def entry_count(polys, cap, join, L):
    """sum over the dashes of 5 nseg + J (nseg - 1) + 2 C, nseg = the dash's points - 1."""
    fan = (1 << L) + 3
    J, C = {np_stroke.MITER: 5, np_stroke.ROUND_JOIN: fan, np_stroke.BEVEL: 4}[join], {np_stroke.BUTT: 0, np_stroke.ROUND_CAP: fan, np_stroke.SQUARE: 5}[cap]
    return sum(5 * (len(p) - 1) + J * (len(p) - 2) + 2 * C for p in polys)


def outline_dashed(pts, closed, width, cap, join, miter_half, pattern, offset, width_scale):
    """width: the stroke's width as the poly-line item carries it (scaled, after the thin-line rule)."""
    polys = cut(pts, closed, pattern, offset, width_scale)
    if isinstance(polys, str):
        return np_stroke.outline(pts, closed, width, cap, join, miter_half)
    rows, boxes, at = [], [], 0
    for poly in polys:
        e, box = np_stroke.outline(poly, False, width, cap, join, miter_half)
        e = e.copy()
        sep = e[:, 0] == np_stroke.NAN_BITS
        e[sep, 1] += at
        rows.append(e)
        boxes.append(box)
        at += len(e)
    if not rows:
        return np.zeros((0, 2), np.uint32), (0, 0, 0, 0)
    b = np.array(boxes)
    return np.concatenate(rows), (int(b[:, 0].min()), int(b[:, 1].min()), int(b[:, 2].max()), int(b[:, 3].max()))


def apply(scene, specs):
    """np_stroke.apply with dashes: every item whose spec is (closed, cap, join, miter_half, dash) becomes the outline Fill of its
    stroke, cut by dash = (pattern, offset, width_scale) unless that is None; outlines follow the scene's end in paint order."""
    sc = bytearray(bytes(scene))
    n, items_ix = struct.unpack_from("<II", sc, 0)
    assert len(specs) == n
    for i, spec in enumerate(specs):
        if spec is None:
            continue
        closed, cap, join, miter_half, dash = spec
        at = items_ix + 32 * i
        tag, rgba, width, npt, pix = struct.unpack_from("<IIfII", sc, at)
        assert tag == 4, "a styled stroke takes a poly-line's slot"
        pts = np.frombuffer(bytes(sc), np.float32, 2 * npt, pix).reshape(npt, 2)
        if dash is None:
            entries, box = np_stroke.outline(pts, closed, width, cap, join, miter_half)
        else:
            entries, box = outline_dashed(pts, closed, width, cap, join, miter_half, *dash)
        struct.pack_into("<8I", sc, at, 3, 2, rgba, len(entries), len(sc), 0, 0, 0)
        struct.pack_into("<4H", sc, 8 + 8 * i, *box)
        sc += entries.tobytes()
    return bytes(sc)


def specs_from_pathset(ps, width_scale):
    """np_stroke.specs_from_paths plus the dash of every item's path."""
    table = {int(d["path"]): ([float(v) for v in ps.dash_values[int(d["first"]) : int(d["first"]) + int(d["count"])]], float(d["offset"]))
             for d in ps.dashes}
    specs = []
    tags = ps.els["tag"]
    for ip, p in enumerate(ps.paths):
        b, e, fl = int(p["el_begin"]), int(p["el_end"]), int(p["flags"])
        moves = [k for k in range(b, e) if tags[k] == 0]
        if fl & 1:
            specs += [None] * ((1 if moves else 0) if fl & 8 else len(moves))
        if fl & 2:
            dash = (table[ip][0], table[ip][1], float(width_scale)) if ip in table else None
            for j, k in enumerate(moves):
                last = moves[j + 1] if j + 1 < len(moves) else e
                specs.append(((tags[last - 1] == 4), (fl >> 8) & 3, (fl >> 10) & 3, (fl >> 16) & 0xFFFF, dash) if fl & np_stroke.OUTLINE else None)
    return specs
