"""Independent numpy statement of decision D14: the outline of a styled stroke as a compound non-zero Fill item.
Written from the decision's text, not from the kernel: whole arrays per kind of piece, the fans built level by level, the
directions at repeated points found with searchsorted over the non-degenerate segments.  Test infrastructure.

All arithmetic is numpy float64 on the poly-line's f32 points, one ufunc per written operation in the written order (numpy never
fuses a multiply with an add); + - * / sqrt only; an outline point is rounded once to f32 when it is stored.

    outline(pts, closed, width, cap, join, miter_half)   -> (entries uint32 [E, 2], box (x0, y0, x1, y1))
    apply(scene, specs)                                    -> the styled scene's bytes, from the unstyled (poly-line) scene
    specs_from_paths(paths, els)                           -> per item of the unstyled scene: None or the style of its path
"""
import struct

import numpy as np

BUTT, ROUND_CAP, SQUARE = 0, 1, 2
MITER, ROUND_JOIN, BEVEL = 0, 1, 2
OUTLINE = 0x10
NAN_BITS = 0x7FC00000
LEVEL_HW = (0.1, 0.3414, 1.3137, 5.2043, 20.767, 83.018)  # D14's table: hw <= LEVEL_HW[L] -> L, else 6


def level(hw):
    for L, t in enumerate(LEVEL_HW):
        if hw <= t:
            return L
    return 6


def miter_limit(miter_half):
    return 4.0 if miter_half == 0 else float(np.array(miter_half, np.uint16).view(np.float16))


def style_bits(cap, join, miter_half=0):
    return OUTLINE | (cap << 8) | (join << 10) | (miter_half << 16)


def half_bits(v):
    return int(np.array(v, np.float16).view(np.uint16))


def _bis(u, v):
    s = u + v
    ln = np.sqrt(s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1])
    return s / ln[..., None]


def _fan(p, e0, e1, mid, hw, L, collapse):
    """[m, 2^L + 2, 2]: the centre, then p + hw*r[j]; mid = the first bisector (rows where it is given), NaN rows: bis(e0, e1)."""
    m, steps = len(p), 1 << L
    r = np.zeros((m, steps + 1, 2))
    r[:, 0], r[:, steps] = e0, e1
    if L >= 1:
        given = ~np.isnan(mid[:, 0])
        with np.errstate(invalid="ignore", divide="ignore"):
            first = _bis(e0, e1)
        r[:, steps // 2] = np.where(given[:, None], mid, first)
        half = steps // 2
        while half >= 2:
            q = half // 2
            for i in range(0, steps, half):
                with np.errstate(invalid="ignore", divide="ignore"):
                    r[:, i + q] = _bis(r[:, i], r[:, i + half])
            half = q
    rim = p[:, None, :] + hw * r
    out = np.concatenate([p[:, None, :], rim], axis=1)
    out[collapse] = p[collapse, None, :]
    return out


def _corner(kind, p, e0, e1, mid, half_turn, collapse, dot, hw, m, L):
    """Pieces [count, points, 2] about p between e0 and e1: kind = "bevel" / "miter" / "fan" / "square"."""
    c0, c1 = p + hw * e0, p + hw * e1
    if kind == "fan":
        return _fan(p, e0, e1, np.where(half_turn[:, None], mid, np.nan), hw, L, collapse)
    if kind == "square":
        q = p + hw * mid
        out = np.stack([c0, q + hw * e0, q + hw * e1, c1], axis=1)
    elif kind == "bevel":
        out = np.stack([p, c0, c1], axis=1)
    else:
        s = 1.0 + dot
        with np.errstate(invalid="ignore", divide="ignore"):
            k = hw / s
            sharp = p + k[:, None] * (e0 + e1)
            ok = ~half_turn & ((m * m) * s >= 2.0)
        tip = np.where(ok[:, None], sharp, c0)
        out = np.stack([p, c0, tip, c1], axis=1)
    out[collapse] = p[collapse, None, :]
    return out


def outline(pts, closed, width, cap, join, miter_half=0):
    P = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    n = len(P)
    assert n >= 1
    hw = np.float64(np.float32(width) * np.float32(0.5))
    L, m = level(hw), miter_limit(miter_half)
    nseg = n if closed else n - 1
    k = np.arange(nseg)
    a, b = P[k], P[(k + 1) % n]
    d = b - a
    nd = ~((d[:, 0] == 0) & (d[:, 1] == 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        u = d / ln[:, None]
    pieces = []  # arrays [count, points, 2] in entry order

    # segments
    N = np.stack([-(hw * u[:, 1]), hw * u[:, 0]], axis=1)
    quad = np.stack([a - N, b - N, b + N, a + N], axis=1) if nseg else np.zeros((0, 4, 2))
    quad[~nd] = a[~nd, None, :]
    pieces.append(quad)

    # the nearest non-degenerate segment behind (k < i, downwards) and ahead (k >= i, upwards) of every vertex
    good = np.flatnonzero(nd)
    i = np.arange(n)
    if len(good) == 0:
        has_in = has_out = np.zeros(n, bool)
        k_in = k_out = np.zeros(n, np.int64)
    else:
        pos_out = np.searchsorted(good, i, "left")        # first good k >= i
        pos_in = np.searchsorted(good, i - 1, "right") - 1  # last good k <= i - 1
        if closed:
            has_in = has_out = np.ones(n, bool)
            k_out, k_in = good[pos_out % len(good)], good[pos_in % len(good)]
        else:
            has_out, has_in = pos_out < len(good), pos_in >= 0
            k_out, k_in = good[np.minimum(pos_out, len(good) - 1)], good[np.maximum(pos_in, 0)]
    d_in, d_out = (u[k_in] if nseg else np.zeros((n, 2))), (u[k_out] if nseg else np.zeros((n, 2)))

    # joins
    jv = i if closed else i[1 : n - 1] if n >= 3 else i[:0]
    if len(jv):
        p, d1, d2 = P[jv], d_in[jv], d_out[jv]
        both = has_in[jv] & has_out[jv]
        with np.errstate(invalid="ignore"):
            c = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
            dot = d1[:, 0] * d2[:, 0] + d1[:, 1] * d2[:, 1]
            left, right = both & (c > 0), both & (c < 0)
            back = both & (c == 0) & (dot < 0)
        rot = lambda v: np.stack([v[:, 1], -v[:, 0]], axis=1)  # noqa: E731  (d.y, -d.x)
        e0 = np.where(right[:, None], -rot(d2), rot(d1))
        e1 = np.where(right[:, None], -rot(d1), np.where(back[:, None], -rot(d1), rot(d2)))
        kind = {MITER: "miter", ROUND_JOIN: "fan", BEVEL: "bevel"}[join]
        pieces.append(_corner(kind, p, e0, e1, d1, back, ~(left | right | back), dot, hw, m, L))

    # caps
    if cap != BUTT:
        dotty = len(good) == 0
        for end in (0, 1):
            p = P[[0 if end == 0 else n - 1]]
            if dotty:
                dd, collapse = np.array([[-1.0 if end == 0 else 1.0, 0.0]]), np.array([False])
            elif closed:
                dd, collapse = np.zeros((1, 2)), np.array([True])
            else:
                dd, collapse = (-d_out[[0]] if end == 0 else d_in[[n - 1]]), np.array([False])
            e0, e1 = np.stack([dd[:, 1], -dd[:, 0]], axis=1), np.stack([-dd[:, 1], dd[:, 0]], axis=1)
            pieces.append(_corner("square" if cap == SQUARE else "fan", p, e0, e1, dd, np.array([True]), collapse, np.zeros(1), hw, m, L))

    # entries: every piece, then its separator {NaN, index of the piece's first entry}
    rows, at = [], 0
    stored = []
    for arr in pieces:
        cnt, npt = arr.shape[0], arr.shape[1]
        if cnt == 0:
            continue
        f = arr.astype(np.float32)
        stored.append(f.reshape(-1, 2))
        blk = np.zeros((cnt, npt + 1, 2), np.uint32)
        blk[:, :npt] = np.ascontiguousarray(f).view(np.uint32)
        blk[:, npt, 0] = NAN_BITS
        blk[:, npt, 1] = at + (npt + 1) * np.arange(cnt)
        rows.append(blk.reshape(-1, 2))
        at += cnt * (npt + 1)
    entries = np.concatenate(rows) if rows else np.zeros((0, 2), np.uint32)
    box = (0, 0, 0, 0)
    if stored:
        xy = np.concatenate(stored).astype(np.float64)
        with np.errstate(invalid="ignore"):
            lo = np.floor(np.fmin.reduce(xy, axis=0))
            hi = np.ceil(np.fmax.reduce(xy, axis=0))
        sat = lambda v: int(min(max(v, 0.0), 65535.0)) if v == v else 0  # noqa: E731
        box = (sat(lo[0]), sat(lo[1]), sat(hi[0]), sat(hi[1]))
    return entries, box


def entry_count(n, closed, cap, join, L):
    """D14's closed form: nothing of the layout depends on a coordinate."""
    fan = (1 << L) + 3
    nseg, njoin = (n, n) if closed else (n - 1, max(n - 2, 0))
    return 5 * nseg + {MITER: 5, ROUND_JOIN: fan, BEVEL: 4}[join] * njoin + 2 * {BUTT: 0, ROUND_CAP: fan, SQUARE: 5}[cap]


def apply(scene, specs):
    """The styled scene: every item of the (flat, un-nested) poly-line scene whose spec is (closed, cap, join, miter_half) becomes
    its outline Fill; the outlines follow the scene's end in paint order; everything else stays byte for byte."""
    sc = bytearray(bytes(scene))
    n, items_ix = struct.unpack_from("<II", sc, 0)
    assert len(specs) == n
    for i, spec in enumerate(specs):
        if spec is None:
            continue
        closed, cap, join, miter_half = spec
        at = items_ix + 32 * i
        tag, rgba, width, npt, pix = struct.unpack_from("<IIfII", sc, at)
        assert tag == 4, "a styled stroke takes a poly-line's slot"
        pts = np.frombuffer(bytes(sc), np.float32, 2 * npt, pix).reshape(npt, 2)
        entries, box = outline(pts, closed, width, cap, join, miter_half)
        hw = np.float64(np.float32(width) * np.float32(0.5))
        assert len(entries) == entry_count(npt, closed, cap, join, level(hw))
        struct.pack_into("<8I", sc, at, 3, 2, rgba, len(entries), len(sc), 0, 0, 0)
        struct.pack_into("<4H", sc, 8 + 8 * i, *box)
        sc += entries.tobytes()
    return bytes(sc)


def specs_from_paths(paths, els):
    """Per item of the scene pm_flatten_and_encode makes of (paths, els): the fills of a path first (one per sub-path, or one
    compound), then its strokes, one per sub-path; a stroke of a path with PM_PATH_STROKE_OUTLINE gets (closed, cap, join, miter)."""
    specs = []
    tags = els["tag"]
    for p in paths:
        b, e, fl = int(p["el_begin"]), int(p["el_end"]), int(p["flags"])
        moves = [k for k in range(b, e) if tags[k] == 0]
        if fl & 1:
            specs += [None] * ((1 if moves else 0) if fl & 8 else len(moves))
        if fl & 2:
            for j, k in enumerate(moves):
                last = moves[j + 1] if j + 1 < len(moves) else e
                specs.append(((tags[last - 1] == 4), (fl >> 8) & 3, (fl >> 10) & 3, (fl >> 16) & 0xFFFF) if fl & OUTLINE else None)
    return specs


def unstyled(paths):
    """The same paths without any stroke style bit: what draws the poly-line scene."""
    p = paths.copy()
    p["flags"] &= np.uint32(0xF)
    return p
