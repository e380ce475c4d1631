"""Degenerate and grid-aligned scenes, and table-driven sweeps of the per-pixel arithmetic (test helper, not a conftest):
tests/test_edge_scenes.py runs them against the oracle on the CPU, under the emulation and on the GPU.

The random scenes of the rest of the suite (random_ops in tests/test_host_cpu.py) are in general position.  The grammar here draws
what real content is made of instead: vertices on pixel corners, pixel centres, tile corners and quarter pixels, axis-aligned
rectangles, zero-length segments, repeated points, one- and two-point fills, zero widths and radii, alpha 0 and 1, items that
hang over the viewport's sides or lie far outside it.  Every choice belongs to a named CLASS; edge_ops() draws only from the
classes it is given and records the ones it used, so a failing scene is shrunk by switching classes off:

    ops, used = edge_ops(seed, w, h, classes=ALL_CLASSES - {"far", "snap_tile"})

The sweeps (blend_sweep, fill_operand_scenes, stroke_operand_scenes) enumerate the operands of renderKernel's per-pixel
operations -- the blend, the trapezoid area of a fill segment, the distance fields -- one tile or one small scene per operand
pair.  Their expected bytes come from the oracle."""
from __future__ import annotations

import numpy as np

TILE = 16

GROUPS = {
    "snap": ("snap_none", "snap_corner", "snap_centre", "snap_tile", "snap_quarter"),
    "rule": ("fill_plain", "fill_even_odd", "fill_compound", "fill_compound_even_odd"),
    "fill": ("rect_cw", "rect_ccw", "rect_closed_cw", "rect_closed_ccw", "fill_1pt", "fill_2pt", "fill_3pt", "fill_repeated_vertex",
             "polygon"),
    "compound": ("compound_reversed_shifted", "compound_one_point_subpath", "compound_rects"),
    "line": ("line_zero_length", "line_horizontal", "line_vertical", "line_slanted"),
    "width": ("width_0", "width_1e-3", "width_0.5", "width_0.7", "width_1", "width_2", "width_32", "width_random"),
    "poly": ("poly_1", "poly_2", "poly_3", "poly_9", "poly_17", "poly_33", "poly_40"),
    "radius": ("radius_0", "radius_0.5", "radius_1", "radius_8", "radius_16", "radius_random"),
    "rx": ("rx_0", "rx_0.5", "rx_1", "rx_random"),
    "ry": ("ry_0", "ry_0.5", "ry_16", "ry_random"),
    "colour": ("opaque", "alpha_0", "alpha_1", "alpha_random"),
    "place": ("near", "far"),
    "kind": ("kind_fill", "kind_line", "kind_poly", "kind_circle", "kind_ellipse"),
}
ALL_CLASSES = frozenset(c for g in GROUPS.values() for c in g)
# (what the issue's text names; "polygon", "line_slanted", "compound_rects", "near" and the kinds only keep the mix alive)
REQUIRED_CLASSES = ALL_CLASSES - {"polygon", "line_slanted", "compound_rects", "near"}

VIEW_W = (16, 31, 64, 100, 257, 300, 520)
VIEW_H = (16, 17, 48, 100, 200, 330)
FAR = lambda w: (-1.0e4, -300.0, w + 300.0, 7.0e4, 1.0e6)  # noqa: E731

# the committed samples: full-size viewports for the frame path, small ones for the Python restatements
FRAME_SEEDS = tuple(range(1000, 1024))
SMALL_SEEDS = tuple(range(2000, 2160))
HIT_SEEDS = tuple(range(3000, 3008))


def viewport(seed, small=False):
    rng = np.random.default_rng([seed, 1])
    ws = [v for v in VIEW_W if v <= 100] if small else VIEW_W
    hs = [v for v in VIEW_H if v <= 48] if small else VIEW_H
    return int(ws[int(rng.integers(0, len(ws)))]), int(hs[int(rng.integers(0, len(hs)))])


def snap(pts, mode):
    pts = np.asarray(pts, np.float64)
    if mode == "snap_corner":
        return np.round(pts)
    if mode == "snap_centre":
        return np.round(pts) + 0.5
    if mode == "snap_tile":
        return np.round(pts / TILE) * TILE
    if mode == "snap_tile_column":  # x on a tile's edge, y on any pixel row of the tile (interior rows included)
        out = np.round(pts)
        out[..., 0] = np.round(pts[..., 0] / TILE) * TILE
        return out
    if mode == "snap_quarter":
        return np.round(pts * 4.0) / 4.0
    return pts


def edge_ops(seed, w, h, n=None, classes=ALL_CLASSES, far_values=None):
    """-> (op list for encode_ops, the set of classes used).  `far_values` replaces the far coordinates (the coordinate-bound
    test climbs them)."""
    rng = np.random.default_rng([seed, 2])
    used = set()
    far = tuple(far_values) if far_values is not None else FAR(w)

    def pick(group):
        live = [c for c in GROUPS[group] if c in classes] or [GROUPS[group][0]]
        c = live[int(rng.integers(0, len(live)))]
        used.add(c)
        return c

    def colour():
        c = pick("colour")
        rgb = int(rng.integers(0, 1 << 24)) << 8
        if rng.random() < 0.2:  # channels at the ends of the sRGB table
            rgb = int(rng.choice([0x000000, 0xFFFFFF, 0x010101, 0xFEFEFE, 0xFF0000, 0x0000FF])) << 8
        return rgb | {"opaque": 0xFF, "alpha_0": 0, "alpha_1": 1}.get(c, int(rng.integers(0, 256)))

    def width():
        c = pick("width")
        return float(rng.uniform(0.0, 12.0)) if c == "width_random" else float(np.float32(c[6:]))

    def snap_mode():
        m = pick("snap")
        if m == "snap_tile" and rng.random() < 0.5:
            return "snap_tile_column"
        return m

    def push_far(pts, centre_too=True):
        """About a seventh of the items: one coordinate -- of the whole item, or of one of its vertices -- goes far away."""
        if "far" not in classes or rng.random() >= 1.0 / 7.0:
            used.add("near")
            return pts
        used.add("far")
        v = float(far[int(rng.integers(0, len(far)))])
        axis = int(rng.integers(0, 2))
        pts = np.array(pts, np.float64)
        if centre_too and rng.random() < 0.5:
            pts[:, axis] += v - pts[0, axis]
        else:
            pts[int(rng.integers(0, len(pts))), axis] = v
        return pts

    def centre():
        return np.array([rng.uniform(-60.0, w + 60.0), rng.uniform(-60.0, h + 60.0)])

    def size():
        return float(rng.choice([1.0, 3.0, 16.0, 40.0, 130.0]))

    def rect(c, s, kind):
        x0, y0 = c
        x1, y1 = x0 + s * rng.uniform(0.2, 1.0), y0 + s * rng.uniform(0.2, 1.0)
        p = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
        if "ccw" in kind:
            p = p[::-1]
        if "closed" in kind:
            p = np.concatenate([p, p[:1]])
        return p

    def fill_points():
        c, s, kind = centre(), size(), pick("fill")
        if kind.startswith("rect"):
            return rect(c, s, kind)
        if kind in ("fill_1pt", "fill_2pt", "fill_3pt"):
            return c + rng.uniform(-s, s, (int(kind[5]), 2))
        p = c + rng.uniform(-s, s, (int(rng.integers(3, 8)), 2))
        if kind == "fill_repeated_vertex":
            k = int(rng.integers(0, len(p)))
            p = np.insert(p, k, p[k], axis=0)
        return p

    n = int(rng.integers(10, 301)) if n is None else n
    ops = []
    for _ in range(n):
        kind = pick("kind")
        mode = snap_mode()
        if kind == "kind_fill":
            rule = pick("rule")
            eo = "_eo" if rule.endswith("even_odd") else ""
            if "compound" in rule:
                c = pick("compound")
                first = snap(fill_points(), mode)
                if c == "compound_reversed_shifted":  # the first sub-path backwards, moved by a snapped offset
                    subs = [first, first[::-1] + snap(rng.uniform(-20.0, 20.0, 2), mode)]
                elif c == "compound_one_point_subpath":
                    subs = [first, snap(first[:1] + rng.uniform(-8.0, 8.0, 2), mode)]
                    if rng.random() < 0.5:
                        subs = subs[::-1]
                else:
                    subs = [first, snap(rect(first[0] + rng.uniform(-10, 10, 2), size(), "rect_ccw"), mode)]
                k = int(rng.integers(0, len(subs)))
                subs[k] = push_far(subs[k])
                ops.append(("fill_cp" + eo, subs, colour()))
            else:
                ops.append(("fill" + eo, push_far(snap(fill_points(), mode)), colour()))
        elif kind == "kind_line":
            c, s, lk = centre(), size(), pick("line")
            a = snap(c, mode)
            d = snap(rng.uniform(-s, s, 2), mode if mode != "snap_centre" else "snap_corner")
            b = {"line_zero_length": a, "line_horizontal": a + (d[0], 0.0), "line_vertical": a + (0.0, d[1])}.get(lk, a + d)
            p = push_far(np.array([a, b]), centre_too=lk != "line_zero_length")
            if lk == "line_zero_length":
                p[1] = p[0]
            ops.append(("line", float(p[0, 0]), float(p[0, 1]), float(p[1, 0]), float(p[1, 1]), width(), colour()))
        elif kind == "kind_poly":
            m = int(pick("poly")[5:])
            step = float(rng.choice([0.0, 1.0, 6.0, 25.0]))
            p = centre() + np.cumsum(rng.uniform(-step, step, (m, 2)), axis=0)
            if m > 1 and rng.random() < 0.7:
                p[1] = p[0]  # the first point twice
            if m > 2 and rng.random() < 0.3:
                p[-1] = p[0]
            ops.append(("poly", push_far(snap(p, mode)), colour(), width()))
        elif kind == "kind_circle":
            r = pick("radius")
            r = float(rng.uniform(0.0, 40.0)) if r == "radius_random" else float(r[7:])
            c = push_far(snap(centre(), mode)[None])[0]
            ops.append(("circle", float(c[0]), float(c[1]), r))
        else:
            rx, ry = pick("rx"), pick("ry")
            rx = float(rng.uniform(0.0, 40.0)) if rx == "rx_random" else float(rx[3:])
            ry = float(rng.uniform(0.0, 40.0)) if ry == "ry_random" else float(ry[3:])
            c = push_far(snap(centre(), mode)[None])[0]
            ops.append(("ellipse", float(c[0]), float(c[1]), rx, ry))
    return ops, used


def edge_scene(pm, seed, small=False, **kw):
    """-> (scene bytes, width, height, classes used) of a committed seed."""
    from test_host_cpu import encode_ops

    w, h = viewport(seed, small)
    ops, used = edge_ops(seed, w, h, **kw)
    return encode_ops(pm, ops, cap=4 << 20), w, h, used


# ---- styled strokes ------------------------------------------------------------------------------------------

def level_threshold_widths():
    """Stroke widths at 0, at the thin-line threshold and at the half-widths where D14's fan level changes, each with its f32
    neighbours."""
    out = [0.0]
    for hw in (0.35, 0.1, 0.3414, 1.3137, 5.2043, 20.767, 83.018):
        wd = np.float32(2.0 * hw)
        out += [float(np.nextafter(wd, np.float32(0))), float(wd), float(np.nextafter(wd, np.float32(1e9)))]
    return out


def stroke_pathset(seed, flags_of):
    """Grammar poly-lines as a path set of strokes: snapped, collinear, reversing, with repeated points, open and closed;
    `flags_of(k)` gives path k's flags."""
    from path_sets import L, M, Z, pathset

    rng = np.random.default_rng([seed, 3])
    widths = level_threshold_widths()
    paths = []
    modes = GROUPS["snap"] + ("snap_tile_column",)
    for k in range(24):
        mode = modes[k % len(modes)]
        c = np.array([rng.uniform(10.0, 150.0), rng.uniform(10.0, 120.0)])
        shape = k % 6
        if shape == 0:  # collinear, straight on
            d = rng.uniform(-9.0, 9.0, 2)
            p = [c, c + d, c + 2 * d, c + 3.5 * d]
        elif shape == 1:  # a reversal on the same line, then on again
            d = rng.uniform(-15.0, 15.0, 2)
            p = [c, c + d, c + 0.25 * d, c + 2 * d]
        elif shape == 2:  # repeated points at the start, inside, at the end
            q = c + np.cumsum(rng.uniform(-14.0, 14.0, (3, 2)), axis=0)
            p = [q[0], q[0], q[1], q[1], q[1], q[2], q[2]]
        elif shape == 3:  # axis-aligned steps
            s = float(rng.choice([1.0, 4.0, 16.0]))
            p = [c, c + (s, 0), c + (s, s), c + (2 * s, s), c + (2 * s, 0)]
        elif shape == 4:  # a dot and a two-point stroke
            p = [c, c] if k % 12 == 4 else [c, c + rng.uniform(-5.0, 5.0, 2)]
        else:
            p = list(c + np.cumsum(rng.uniform(-12.0, 12.0, (int(rng.integers(3, 9)), 2)), axis=0))
        p = snap(np.array(p), mode)
        els = [(M, float(p[0, 0]), float(p[0, 1]))] + [(L, float(x), float(y)) for x, y in p[1:]]
        if rng.random() < 0.35:
            els.append((Z,))
        paths.append((els, flags_of(k), widths[(k + seed) % len(widths)]))
    return pathset(*paths)


# ---- sweeps of the per-pixel arithmetic ---------------------------------------------------------------------

SWEEP_ALPHAS = (1, 2, 127, 128, 254, 255)  # all 256 channel values at these alphas ...
SWEEP_VALUES = (0, 1, 2, 10, 64, 127, 128, 200, 254, 255)  # ... and all 256 alphas at these channel values


def blend_pairs():
    """4 096 (channel value, alpha) pairs."""
    pairs = [(v, a) for a in SWEEP_ALPHAS for v in range(256)] + [(v, a) for v in SWEEP_VALUES for a in range(256)]
    assert len(pairs) == 4096
    return pairs


def blend_sweep(second, pairs=None, columns=64):
    """One tile per (channel value v, alpha a) pair, `columns` tiles per row: the tile is covered once by a rectangle that reaches
    from the middle of the tile above to the middle of the tile below (a Solid: opaque for odd tiles, translucent for even ones,
    and painted over by the next row's, so that what the second item blends onto varies), then by the second item in the colour
    (v, 255 - v, v ^ 0x5A) with alpha a:
      'edge'   a fill whose slanted edge crosses the tile;
      'wedges' a compound fill of sixteen slivers, one per pixel row, whose height grows along x and from row to row: every
               pixel of the tile has a partial coverage of its own, (i + 0.5)(j + 1) / 272;
      'stroke' a slanted line whose distance field crosses the tile;
      'circle' a circle (black, no colour of its own: the pair only sets what it is blended onto).
    -> (ops, width, height)."""
    pairs = blend_pairs() if pairs is None else pairs
    rows = (len(pairs) + columns - 1) // columns
    w, h = columns * TILE, rows * TILE
    ops = []
    for k, (v, a) in enumerate(pairs):
        x0, y0 = float(TILE * (k % columns)), float(TILE * (k // columns))
        under = ((v * 7 + 13) & 0xFF) << 24 | ((a * 5 + 1) & 0xFF) << 16 | ((v ^ a) & 0xFF) << 8 | (0xFF if k & 1 else (a * 3 + 40) & 0xFF)
        ops.append(("fill", np.array([[x0 - 8, y0 - 8], [x0 + 24, y0 - 8], [x0 + 24, y0 + 24], [x0 - 8, y0 + 24]]), under))
        rgba = v << 24 | (255 - v) << 16 | (v ^ 0x5A) << 8 | a
        if second == "edge":
            t = (k * 37 % 64) / 4.0  # where the edge starts: every quarter pixel of the tile's width
            ops.append(("fill", np.array([[x0 - 4, y0 + 0.25], [x0 + t, y0 + 0.25], [x0 + 16 - t, y0 + 15.5], [x0 - 4, y0 + 15.5]]), rgba))
        elif second == "wedges":
            subs = []
            for j in range(16):
                y = y0 + j + 0.5
                g = (j + 1) / 34.0  # half the height at the tile's right edge
                subs.append(np.array([[x0, y], [x0 + 16, y - g], [x0 + 16, y + g]]))
            ops.append(("fill_cp", subs, rgba))
        elif second == "stroke":
            ops.append(("line", x0 + 1.25, y0 + (k % 7), x0 + 14.5, y0 + 15.0 - (k % 5), 0.25 * (k % 23), rgba))
        else:
            ops.append(("circle", x0 + 8.0 + 0.5 * (k % 3), y0 + 8.0 + 0.5 * (k % 2), 0.5 * (k % 17)))
    return ops, w, h


def _ulp_up(x, k=1):
    x = np.float32(x)
    for _ in range(k):
        x = np.nextafter(x, np.float32(np.inf))
    return float(x)


def fill_operand_scenes():
    """name -> (ops, width, height): segments that put renderKernel's Fill arithmetic (the clipped trapezoid's area divided by
    xmax - xmin, the 1e-6 it keeps that apart from zero with) and tileKernel's fill tests at the ends of their operands."""
    T = 0x2040C0B0  # translucent
    O = 0x802010FF
    tiny = float(np.float32(1e-40))
    out = {}
    # endpoints on pixel corners: every slope dx / dy of corner-to-corner segments inside one tile and across two
    ops = []
    k = 0
    for dx in (0, 1, 2, 3, 5, 16, 17, 31):
        for dy in (1, 2, 7, 16, 33):
            x0, y0 = 8.0 + 48 * (k % 8), 8.0 + 40 * (k // 8)
            ops.append(("fill", np.array([[x0, y0], [x0 + dx, y0 + dy], [x0 - 6.0, y0 + dy]]), T if k & 1 else O))
            ops.append(("fill_eo", np.array([[x0 + 20, y0 + dy], [x0 + 20 + dx, y0], [x0 + 14.0, y0]]), T))
            k += 1
    out["pixel_corner_slopes"] = (ops, 400, 208)
    # near-vertical edges: xmax - xmin = 0, one ulp, 1e-7, 1e-6, at integer, half-integer and in-between x
    ops = []
    k = 0
    for x in (5.0, 5.5, 21.3, 32.0, 47.999996, 64.000008):
        for d in (0.0, "ulp", 1e-7, 1e-6, 2e-6, 1e-5):
            xb = _ulp_up(x) if d == "ulp" else float(np.float32(x) + np.float32(d))
            y0 = 3.0 + 24.5 * (k % 6)
            for sgn in (1, -1):
                p = np.array([[x, y0], [xb, y0 + 20.25], [x + 9.5 * sgn, y0 + 20.25], [x + 9.5 * sgn, y0]])
                ops.append(("fill", p if sgn > 0 else p[::-1], T))
            k += 1
    out["near_vertical"] = (ops, 96, 176)
    # near-horizontal edges: ey - sy one ulp, a few ulps, in the f32 denormals, zero
    ops = []
    k = 0
    for y in (0.0, tiny, 4.0, 4.5, 16.0, 17.25, 31.999998):
        for d in ("ulp", "3ulp", 1e-40, 1e-38, 0.0):
            yb = _ulp_up(y, 1 if d == "ulp" else 3) if isinstance(d, str) else float(np.float32(y) + np.float32(d))
            x0 = 2.0 + 19.0 * (k % 5)
            ops.append(("fill", np.array([[x0, y], [x0 + 17.5, yb], [x0 + 17.5, y + 9.0], [x0, y + 7.5]]), T))
            ops.append(("fill", np.array([[x0, y - 6.0], [x0 + 17.5, y - 5.0], [x0 + 17.5, yb], [x0, y]]), O if k & 1 else T))
            k += 1
    out["near_horizontal"] = (ops, 100, 48)
    # coordinates of +-1e-40 (f32 denormals) against the viewport's origin
    ops = []
    for sx in (tiny, -tiny, 0.0, -0.0):
        for sy in (tiny, -tiny, 0.0):
            ops.append(("fill", np.array([[sx, sy], [20.5, sy], [20.5, 9.25 + sy], [sx, 30.0]]), T))
            ops.append(("fill_eo", np.array([[sx, 12.0], [sx, sy], [14.0, -tiny], [9.0, 12.0]]), T))
            ops.append(("line", sx, sy, 25.0, tiny, 1.5, T))
            ops.append(("poly", np.array([[sx, 40.0], [sx, sy], [-tiny, tiny]]), O, 3.0))
    out["denormal_coordinates"] = (ops, 48, 48)
    # |winding| 1, 2, 3 and 40 under both rules: a rectangle walked that many times, with slanted sides
    ops = []
    for k, turns in enumerate((1, 2, 3, 40)):
        for j, rule in enumerate(("fill", "fill_eo")):
            for i, flip in enumerate((False, True)):
                x0, y0 = 4.0 + 44.0 * k, 5.0 + 50.0 * (2 * j + i)
                quad = np.array([[x0, y0], [x0 + 35.5, y0 + 2.25], [x0 + 38.0, y0 + 40.5], [x0 + 3.25, y0 + 37.0]])
                p = np.concatenate([quad[::-1] if flip else quad] * turns)
                ops.append((rule, p, T if (k + i) & 1 else O))
    out["winding_numbers"] = (ops, 184, 208)
    return out


def far_corner_scene():
    """A 65 535 x 16 viewport: fills, strokes and circles at its far end, where an f32 ulp is 1/256 px."""
    T, O = 0x2040C0B0, 0x802010FF
    ops = []
    for k, x in enumerate((65535.0, 65534.5, 65520.0, 65519.996, 65500.25, 65472.0, 65407.004)):
        y = float(k % 3)
        ops.append(("fill", np.array([[x - 9.0, y], [x, y + 0.25], [x - 2.0039062, y + 13.0], [x - 11.5, y + 12.5]]), T if k & 1 else O))
        ops.append(("fill_eo", np.array([[x - 30.0, 2.0], [x - 29.996094, 14.0], [x - 22.0, 14.0], [x - 22.0, 2.0]]), T))
        ops.append(("line", x - 40.0, 1.5, x - 33.0, 13.0, 1.0 + 0.5 * k, T))
        ops.append(("circle", x - 50.0, 8.0, 0.5 * k))
        ops.append(("ellipse", x - 60.0, 8.0, 3.0, 0.5 + k))
    ops.append(("fill", np.array([[-5.0, -5.0], [70000.0, 3.0], [70000.0, 9.0], [-5.0, 30.0]]), 0x10305080))
    ops.append(("line", 65000.0, 0.0, 65535.0, 16.0, 2.0, O))
    return ops, 65535, 16


def stroke_operand_scenes():
    """name -> (ops, width, height): the distance fields at the ends of their operands."""
    T, O = 0x2040C0B0, 0x802010FF
    tiny = float(np.float32(1e-40))
    out = {}
    # zero-length segments (the 0 / 0 of D5) alone, first, last and in the middle of a poly-line; on pixel centres and corners
    ops = []
    for k, (x, y) in enumerate(((8.0, 8.0), (24.5, 8.5), (40.25, 8.0), (56.0, 24.5), (8.5, 40.0), (16.0, 16.0), (32.0, 48.0))):
        for j, wd in enumerate((0.0, tiny, 1e-3, 0.7, 1.0, 5.0)):
            xx = x + 64.0 * (j % 3)
            yy = y + 64.0 * (j // 3)
            ops.append(("line", xx, yy, xx, yy, wd, T if (k + j) & 1 else O))
            ops.append(("poly", np.array([[xx + 3, yy + 3]]), T, wd))
            ops.append(("poly", np.array([[xx - 3, yy + 3], [xx - 3, yy + 3], [xx - 6, yy + 5], [xx - 6, yy + 5], [xx - 6, yy + 5]]), O, wd))
    out["zero_length_segments"] = (ops, 192, 128)
    # half-widths: 0, f32 denormals, tiny, and 1e6 (every pixel inside)
    ops = []
    for k, wd in enumerate((0.0, tiny, 2 * tiny, 1.1754944e-38, 1e-30, 1e-6, 2.0e6)):
        x = 6.0 + 12.0 * k
        ops.append(("line", x, 3.0, x + 7.5, 44.0, wd, 0x40C02030 if wd > 1 else O))
        ops.append(("line", x + 0.5, 8.5, x + 0.5, 30.5, wd, T))  # through pixel centres: distance exactly 0
        ops.append(("poly", np.array([[x, 60.5], [x + 8.0, 60.5], [x + 8.0, 70.0]]), O, wd))
    out["half_widths"] = (ops, 100, 80)
    # ties: pixel centres at distance exactly half_width + 0.5 (alpha exactly 0), half_width - 0.5 (exactly 1) and half_width
    ops = []
    for k, wd in enumerate((0.0, 1.0, 2.0, 3.0, 5.0, 8.0)):
        y = 12.0 + 20.0 * k  # integer y: pixel centres (px = column index) sit at integer distances from a horizontal line
        ops.append(("line", 10.0, y, 70.0, y, wd, T if k & 1 else O))
        ops.append(("line", 90.0 + 20.0 * k, 5.0, 90.0 + 20.0 * k, 100.0, wd, T))
        ops.append(("line", 10.0, y + 8.5, 70.0, y + 8.5, wd, O))
    out["distance_ties"] = (ops, 208, 136)
    # circles of radius 0 and 0.5, ellipses with the centre on a pixel (len == 0 there) and flat ones
    ops = []
    k = 0
    for r in (0.0, 0.5, 1.0, 1.5, 8.0):
        for cx, cy in ((8.0, 8.0), (8.5, 8.5), (16.0, 16.0), (15.5, 8.0)):
            ops.append(("circle", cx + 32.0 * (k % 5), cy + 32.0 * (k // 5), r))
            k += 1
    for rx in (0.0, 0.5, 1.0, 7.0):
        for ry in (0.0, 0.5, 3.0, 16.0):
            for cx, cy in ((8.0, 8.0), (8.5, 8.0), (16.0, 16.0)):
                ops.append(("ellipse", cx + 32.0 * (k % 5), cy + 32.0 * (k // 5), rx, ry))
                k += 1
    out["circles_and_ellipses"] = (ops, 160, 32 * ((k + 4) // 5))
    return out


def coverage_sweep(n_tiles=4096, columns=64):
    """One tile per row of a table of wedges, nothing under them: an opaque item (black, or one saturated channel) over the white
    clear colour, where one binary16 ulp of coverage is most of an 8-bit step of the dark result.  Sixteen slivers per tile, one
    per pixel row, as in blend_sweep's 'wedges', but with heights, ends and offsets that are no dyadic fractions (the tile's number
    times irrational steps), so that the products area * height of renderKernel's Fill fill their f32 mantissas: on grid-aligned
    operands every one of them is exact, and a conversion to binary16 that rounds once instead of twice cannot show.
    -> (ops, width, height)."""
    rows = (n_tiles + columns - 1) // columns
    ops = []
    for k in range(n_tiles):
        x0, y0 = float(TILE * (k % columns)), float(TILE * (k // columns))
        u = (k * 0.6180339887) % 1.0
        v = (k * 0.4142135623) % 1.0
        rgba = (0x000000FF, 0x000000FF, 0xFF0000FF, 0x00FF00FF, 0x0000FFFF, 0x101010FF)[k % 6]
        subs = []
        for j in range(16):
            y = y0 + j + 0.5 + 0.37 * (u - 0.5)
            g = 0.5 * (0.55 + 0.45 * ((j * 0.7548776662 + v) % 1.0))  # half the height at the wide end: 0.27 .. 0.5
            if (j + k) & 1:
                subs.append(np.array([[x0 - 3.0 * u, y], [x0 + 16.0 + v, y - g], [x0 + 16.0 + v, y + g]]))
            else:
                subs.append(np.array([[x0 + 16.0 + 3.0 * v, y], [x0 - u, y + g], [x0 - u, y - g]]))
        ops.append(("fill_cp", subs, rgba))
    return ops, columns * TILE, rows * TILE
