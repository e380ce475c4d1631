"""Scenes and query rectangles for the rectangle queries, pm_hit_rects / pm_select_rect (test helper, not a conftest):
tests/test_hit_rect.py runs them against tests/np_rect.py under the emulation and on the GPU, and pins on the CPU, with numpy
alone, that the cases are what they claim.

The kernels (piet_metal_amd/csrc/pm_hit_rect.h) walk the items WAVE at a time and reach a Fill's or a Polyline's segments through
the scene index, chunks of CHUNK_SEGS segments and super-chunks of SUPER_CHUNKS chunks, as pm_hit_kernel does.

  small_cases    mixed_scene, edge_scene, the oracle's path test and a scene of non-finite points under a few hundred seeded rectangles of every class;
  walk_case      hit_frame_cases.walk_scene at WALK_SIZES items: the whole scene, one cell, and rectangles whose topmost touched item
                 sits at either end of a step of the walk;
  long_case      one long Fill or Polyline between a lead and a trailing item, and rectangles decided by ONE segment of a named chunk;
  known_scene    a dozen hand-derived answers.

Expectations are np_rect's, computed once per (case, flag) and never written to."""
from __future__ import annotations

import numpy as np

import hit_frame_cases as fc
import hit_structure as hs
import np_hit
import np_rect

F32 = np.float32
NONE = hs.NONE
WAVE = hs.WAVE
WALK_SIZES = (WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1)


class RectCase:
    """A scene and query rectangles, float32 [n, 4]."""

    def __init__(self, ident, scene, rects, **facts):
        self.ident, self.scene, self.facts = ident, scene, facts
        self.rects = np.ascontiguousarray(rects, F32).reshape(-1, 4)
        self._want = {}

    def __repr__(self):
        return f"{self.ident} ({len(self.rects)} rectangles)"

    def flags(self, skip=False):
        """uint8 [n_items, n] by np_rect."""
        if skip not in self._want:
            f = np_rect.item_flags(self.scene, self.rects, skip)
            f.setflags(write=False)
            self._want[skip] = f
        return self._want[skip]

    def expected(self, skip=False):
        """(top_item, n_hit) uint32 [n]."""
        return np_rect.hit_rects(self.scene, self.rects, flags=self.flags(skip))


def around(points, half):
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return np.concatenate([p - half, p + half], axis=1)


INVALID = np.array([[np.nan, 0, 10, 10], [0, np.nan, 10, 10], [0, 0, np.nan, 10], [0, 0, 10, np.nan], [np.inf, 0, np.inf, 10], [-np.inf, 0, 10, 10],
                    [0, 0, np.inf, 10], [0, -np.inf, 10, np.inf], [30, 30, 20, 40], [30, 30, 40, 20], [200, 200, 100, 100]])
FAR = np.array([[1.0e6, 1.0e6, 1.0e6 + 50, 1.0e6 + 50], [-1.0e5, -1.0e5, -9.0e4, -9.0e4], [3.0e9, -3.0e9, 3.1e9, 3.0e9], [-900, 100, -800, 140],
                [66000, 5000, 66100, 5100]])
STRADDLE = np.array([[-5, 0, 5, 10], [-0.5, -0.5, 0.5, 0.5], [-30, 10, 0, 30], [0, 0, 0, 40], [65530, 0, 65540, 30], [65535, 10, 65535, 90],
                     [65534.5, 0, 65535.5, 120], [65000, -20, 70600, 50], [-50, -40, 70, 60], [65400, 90, 65600, 110]])


def seeded_rects(scene, region, seed, extra=()):
    """Every class of rectangle that does not need to know the scene: uniform ones of 0 - 40 px over `region` =
    (xa, ya, xb, yb), point and line rectangles, ones centred on every scene vertex (a point, and 1.5 px wide), rectangles across
    x = 0 and x = 65 535, invalid ones and ones far outside; `extra`: the hand-placed ones of the scene."""
    from test_hit_gpu import scene_vertices_and_segments

    rng = np.random.default_rng(seed)
    xa, ya, xb, yb = region
    c = rng.uniform(0.0, 1.0, (140, 2)) * (xb - xa, yb - ya) + (xa, ya)
    uni = np.concatenate([c, c + rng.uniform(0.0, 40.0, (140, 2))], axis=1)
    p = rng.uniform(0.0, 1.0, (45, 2)) * (xb - xa, yb - ya) + (xa, ya)
    points = np.concatenate([p[:15], p[:15]], axis=1)
    hor = np.concatenate([p[15:30], p[15:30] + np.stack([rng.uniform(0, 60, 15), np.zeros(15)], axis=1)], axis=1)
    ver = np.concatenate([p[30:], p[30:] + np.stack([np.zeros(15), rng.uniform(0, 60, 15)], axis=1)], axis=1)
    verts, a, b = scene_vertices_and_segments(scene)
    verts = verts[np.isfinite(verts).all(axis=1)].astype(np.float64)
    mids = (a + b) * 0.5
    out = [uni, points, hor, ver, around(verts, 0.0), around(verts, 0.75), around(mids[:: max(len(mids) // 40, 1)], 0.0), STRADDLE, INVALID, FAR]
    if len(extra):
        out.append(np.asarray(extra, np.float64).reshape(-1, 4))
    return np.concatenate(out).astype(F32)


# mixed_scene (tests/test_hit_gpu.py), by its own numbers: item 0 the square [20.25, 220.25] x [30.5, 230.5]; item 2 the even-odd
# ring [100.5, 250.5] x [100.25, 250.25] with the hole [140.5, 200.5] x [140.25, 200.25]; item 6 the non-zero ring
# [300.5, 450.5] x [280.25, 430.25] whose reversed hole is [340.5, 400.5] x [320.25, 380.25], with the square [350, 370] x [330, 350] in it
MIXED_INSIDE_FILL = [[30, 40, 50, 55], [25, 200, 60, 228]]                  # in item 0, meeting no edge of it
MIXED_IN_EO_HOLE = [[150, 150, 190, 190], [141, 141, 142, 142]]             # in the hole of item 2
MIXED_NZ_HOLE = [[375, 335, 395, 375], [365, 345, 398, 378], [335, 315, 405, 385], [340.5, 320.25, 400.5, 380.25]]   # in / around item 6's hole
MIXED_ENCLOSING = [[0, 0, 520, 520], [90, 90, 260, 260], [110, 280, 210, 380], [50, 50, 70, 70], [15, 25, 225, 235], [290, 270, 460, 440],
                   [180, 140, 420, 260], [20.25, 30.5, 220.25, 230.5]]   # marquees around whole items (the last: item 0's own box)
MIXED_EXTRA = MIXED_INSIDE_FILL + MIXED_IN_EO_HOLE + MIXED_NZ_HOLE + MIXED_ENCLOSING
# edge_scene: item 0 the fill [-40, 60] x [-30, 50], item 1 the fill [65000, 70500] x [-5, 40]
EDGE_EXTRA = [[-30, -20, -25, -15], [66000, 0, 67000, 30], [70400, 10, 70600, 20], [-45, -35, -38, -28], [65536, 0, 65600, 10], [-41, -31, 61, 51]]


def _region_of(scene, pad=30.0):
    verts = np.concatenate([np_hit._points(bytes(scene), at) for at, _ in np_hit.flat_items(bytes(scene))
                            if np.frombuffer(bytes(scene), np.uint32, 1, at)[0] & 0xFFFF in (np_hit.FILL, np_hit.POLY)])
    return float(verts[:, 0].min() - pad), float(verts[:, 1].min() - pad), float(verts[:, 0].max() + pad), float(verts[:, 1].max() + pad)


def nonfinite_scene(pm):
    """Items with non-finite points and widths: 0 a Fill with two points at x = +inf -- by D13 its falling edge at x = 100 winds
    around every point LEFT of it between y = 10 and 50, outside the item's box --; 1 a Polyline with a NaN point in the middle; 2 a
    Fill with a NaN point; 3 a Line that ends at x = +inf; 4 a Polyline of width NaN (it touches nothing)."""
    def emit(e):
        e.fill(np.array([[100, 10], [np.inf, 10], [np.inf, 50], [100, 50]], np.float64), 0x336699FF)
        e.polyline(np.array([[10, 80], [60, 80], [np.nan, 90], [100, 100], [140, 100]], np.float64), 0x11AA22FF, 2.0)
        e.fill(np.array([[20, 120], [60, 120], [np.nan, 130], [60, 160], [20, 160]], np.float64), 0x884400FF)
        e.stroke_line((10.0, 200.0), (np.inf, 200.0), 3.0, 0x000000FF)
        e.polyline(np.array([[10, 220], [60, 220]], np.float64), 0x11AA22FF, float("nan"))

    return hs._encode(pm, 5, emit)


NONFINITE_EXTRA = [[50, 30, 60, 40], [150, 30, 160, 40], [0, 0, 300, 300], [55, 75, 65, 85], [95, 95, 105, 105], [30, 130, 40, 140], [5, 195, 15, 205],
                   [500, 195, 510, 205], [5, 215, 65, 225], [70, 5, 90, 60], [61, 121, 70, 165], [-50, 20, -40, 25], [99, 9, 141, 102], [9, 78, 61, 82]]

_small = {}
SMALL = ("mixed", "edge", "path_test", "nonfinite")


def small_case(pm, pmo, name):
    if name not in _small:
        from test_hit_gpu import edge_scene, mixed_scene

        if name == "mixed":
            scene = mixed_scene(pm)
            rects = seeded_rects(scene, (-20, -20, 540, 540), 21, MIXED_EXTRA)
        elif name == "edge":
            scene = edge_scene(pm)
            far = seeded_rects(scene, (64900, -40, 65700, 140), 23)[:140]
            rects = np.concatenate([seeded_rects(scene, (-80, -60, 120, 140), 22, EDGE_EXTRA), far])
        elif name == "nonfinite":
            scene = nonfinite_scene(pm)
            rects = seeded_rects(scene, (-60, -20, 260, 260), 25, NONFINITE_EXTRA)
        else:
            scene = pmo.scene_path_test()
            rects = seeded_rects(scene, _region_of(scene), 24)
        _small[name] = RectCase(name, scene, rects)
    return _small[name]


# ---- the item walk -----------------------------------------------------------------------------------------------------

_walks = {}


def walk_case(pm, n):
    """hit_frame_cases.walk_scene of n items.  Rectangles: the whole scene; the cell of one ordinary item; a point in a cell's empty
    corner, which touches the bottom item only; and, in the cells of item n - 3 (the topmost with a cell) and of the items at lanes
    63 and 0 of every step of the walk from the top (items n - 64 k - 64 and n - 64 k - 65, where they have a cell), a rectangle over
    the cell's upper half.
    Item 0 lies under every cell: what such a rectangle touches is the cell's item and item 0, and its top is the cell's item."""
    if n not in _walks:
        wdw = fc.walk_scene(pm, n)
        x0, y0, w, h = wdw.rect
        rects = [[x0 - 2, y0 - 2, x0 + w + 2, y0 + h + 2]]
        cx, cy = fc.walk_cell(7)
        rects.append([cx, cy, cx + fc.CELL, cy + fc.CELL])
        cx, cy = fc.walk_cell(3)
        rects.append([cx + 0.25, cy + 0.25, cx + 0.25, cy + 0.25])
        ends = []
        for i in [n - 3] + [j for k in range(-(-n // WAVE)) for j in (n - WAVE * k - WAVE, n - WAVE * k - WAVE - 1)]:
            if 1 <= i <= n - 3:
                ends.append(i)
                cx, cy = fc.walk_cell(i)
                rects.append([cx + 1.4, cy + 1.1, cx + 2.6, cy + 1.9])
        rects += [[x0 + w + 50, y0, x0 + w + 60, y0 + 5], [np.nan, 0, 1, 1]]
        _walks[n] = RectCase(f"walk-{n}", wdw.scene, rects, n=n, ends=ends, kinds=wdw.facts["kinds"])
    return _walks[n]


# ---- long items --------------------------------------------------------------------------------------------------------

LONG_CHUNKS = (WAVE, WAVE + 1, 8 * WAVE + 1)     # 513 = 8 * 64 + 1 chunks: 65 super-chunks and more, the second round of them
LONG_KINDS = ("fill-nz", "fill-eo", "polyline")
LONG_IDS = [f"{kind}-{chunks}" for kind in LONG_KINDS for chunks in LONG_CHUNKS]
PITCH = 2.0
LONG_ITEM = 1


def long_points(kind, chunks):
    """A Fill of 4 * chunks points: a band between a toothed top edge (y = 100 at every third point, 106 between) and a zigzag bottom edge (y = 130 / 136), closed
    by the vertical edge at x = 10 -- its last segment.  A Polyline of 4 * chunks + 1 points: a zigzag between y = 100 and y = 110."""
    if kind == "polyline":
        k = np.arange(4 * chunks + 1)
        return np.stack([10.0 + PITCH * k, np.where(k & 1, 110.0, 100.0)], axis=1)
    m = 2 * chunks
    k = np.arange(m)
    top = np.stack([10.0 + PITCH * k, np.where(k % 3, 106.0, 100.0)], axis=1)   # (teeth of three segments: a chunk of four is never balanced)
    bottom = np.stack([10.0 + PITCH * k, np.where(k & 1, 136.0, 130.0)], axis=1)[::-1]
    return np.concatenate([top, bottom])


_longs = {}


def long_case(pm, ident):
    """Item 0 a lead Fill of 9 points (3 chunks: the long item's first chunk sits at residue 3 of a super-chunk), item 1 the long
    item, item 2 a trailing Fill.  Rectangles 0, 1: a tenth of a pixel around the middle of one segment of the last chunk and of
    chunk min(64, chunks - 1); 2: none -- between two teeth (a Fill: above the band; the Polyline: beside a tooth); 3 (Fills):
    inside the band, meeting no edge; 4: the whole item, which encloses it; 5: all but its last vertex; 6: see below."""
    if ident not in _longs:
        kind, chunks = ident.rsplit("-", 1)
        chunks = int(chunks)
        pts = long_points(kind, chunks)
        lead = np.array([[300 + 3 * np.cos(t), 20 + 3 * np.sin(t)] for t in np.linspace(0, 2 * np.pi, 9, endpoint=False)])
        right = float(pts[:, 0].max())

        def emit(e):
            e.fill(lead, 0x223344FF)
            if kind == "polyline":
                e.polyline(pts, 0x11AA22FF, 0.5)
            else:
                e.fill(pts, 0x336699FF, even_odd=kind.endswith("eo"))
            e.fill(np.array([[right + 30, 60], [right + 40, 60], [right + 40, 70], [right + 30, 70]], np.float64), 0x884400FF)

        scene = hs._encode(pm, 3, emit, cap=1 << 20)
        sc = bytes(scene)
        ent, a, b, nent = hs._entries(sc, np_hit.flat_items(sc)[LONG_ITEM][0])
        assert -(-nent // hs.CHUNK_SEGS) == chunks
        segs = [4 * (chunks - 1) + 3, 4 * min(WAVE, chunks - 1) + 1]
        rects = [np.concatenate([(a[s] + b[s]) * 0.5 - 0.05, (a[s] + b[s]) * 0.5 + 0.05]) for s in segs]
        xm = 10.0 + PITCH * (2 * (chunks // 2) + 1)
        rects.append([xm - 0.1, 95.0, xm + 0.1, 99.0] if kind != "polyline" else [xm - 0.2, 100.0, xm + 0.2, 100.5])
        rects.append([xm - 3.0, 112.0, xm + 3.0, 124.0] if kind != "polyline" else [xm - 0.2, 120.0, xm + 0.2, 121.0])
        lo, hi = pts.min(axis=0) - 0.25, pts.max(axis=0) + 0.25
        rects.append([lo[0], lo[1], hi[0], hi[1]])
        rects.append([lo[0] + (PITCH if kind != "polyline" else 0.0), lo[1], hi[0] - (PITCH if kind == "polyline" else 0.0), hi[1]])
        # 6 (Fills): a tenth of a pixel around (16, 103), under the tooth at point 3 near the item's left end: it meets no edge, and
        # every chunk of the top edge to its right holds segments that cross y = 103 -- its corner's winding is a sum over ALL of them
        rects.append([15.95, 102.95, 16.05, 103.05] if kind != "polyline" else [15.95, 112.95, 16.05, 113.05])
        _longs[ident] = RectCase(ident, scene, rects, kind=kind, chunks=chunks, segs=segs)
    return _longs[ident]


# ---- hand-derived answers ----------------------------------------------------------------------------------------------

def known_scene(pm):
    """0 the Fill [10, 20]^2; 1 a Polyline (30, 10) -> (50, 10) of width 2; 2 a Circle, centre (70, 15), radius 5; 3 an even-odd ring
    [10, 40] x [40, 70] with the hole [20, 30] x [50, 60]; 4 a Line (60, 40) -> (60, 60) of width 4; 5 an ellipse, centre (90, 50),
    radii 10 and 5; 6 a Fill of two points, (110, 10) and (120, 20): no area, winding 0 everywhere, two edges on each other;
    7 a Polyline of width 1 along y = 90 from x = 10 to x = 120 (the hairline of the pick test); 8 an ellipse with ry = 0, centre (100, 70),
    rx = 10: by D13 it contains no point, so it has no geometry."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)  # noqa: E731

    def emit(e):
        e.fill(sq(10, 10, 20, 20), 0x336699FF)
        e.polyline(np.array([[30.0, 10.0], [50.0, 10.0]]), 0x11AA22FF, 2.0)
        e.circle((70.0, 15.0), 5.0)
        e.fill_compound([sq(10, 40, 40, 70), sq(20, 50, 30, 60)], 0xAA5500FF, even_odd=True)
        e.stroke_line((60.0, 40.0), (60.0, 60.0), 4.0, 0x000000FF)
        e.ellipse((90.0, 50.0), 10.0, 5.0)
        e.fill(np.array([[110.0, 10.0], [120.0, 20.0]]), 0x9900CCFF)
        e.polyline(np.array([[10.0, 90.0], [120.0, 90.0]]), 0x445566FF, 1.0)
        e.ellipse((100.0, 70.0), 10.0, 0.0)

    return hs._encode(pm, 9, emit)


def up(v):
    return float(np.nextafter(F32(v), F32(np.inf)))


T, E = np_rect.TOUCHES, np_rect.TOUCHES | np_rect.ENCLOSES
# (rectangle, item, PM_SEL_* of that item) -- each worked out by hand:
KNOWN = [
    # the Fill [10, 20]^2: R's corner c0 = (20, 20) IS the Fill's vertex: both edges that end there meet R (s_0 = 0)
    ([20, 20, 25, 25], 0, T),
    ([up(20), 10, 25, 20], 0, 0),                 # one f32 step to the right of the edge x = 20: min(a.x, b.x) = 20 < x0 for every edge
    ([12, 12, 18, 18], 0, T),                     # inside: no edge meets R (all four s_k of every edge have one sign), c0 has winding 1
    ([10, 10, 20, 20], 0, E),                     # R is the Fill's own box: closed on both sides
    ([10, 10, 20, up(19.99)], 0, T),              # ... and a hair too short below
    # the Polyline along y = 10, hw = 1: R's upper edge at y = 11 is at distance exactly hw (dR2(a) = 1 = hw * hw)
    ([35, 11, 40, 12], 1, T),
    ([35, up(11), 40, 12], 1, 0),
    ([51, 11, 60, 20], 1, 0),                     # inside the box widened by hw, but (51, 11) is sqrt(2) from the end (50, 10)
    ([50.5, 10.5, 52, 12], 1, T),                 # 0.25 + 0.25 <= 1
    ([29, 9, 51, 11], 1, E),                      # x0 <= 30 - 1, 50 + 1 <= x1, y0 <= 10 - 1, 10 + 1 <= y1: all with equality
    ([29.5, 9, 51, 11], 1, T),
    # the Circle (70, 15), r = 5: c0 = (73, 19) is at (3, 4) from the centre, 9 + 16 = 25 = r * r; (74, 19): 16 + 16 > 25, boxes overlap
    ([73, 19, 80, 25], 2, T),
    ([74, 19, 80, 25], 2, 0),
    ([65, 10, 75, 20], 2, E),
    # the even-odd ring: inside the hole the winding of c0 is 2 and no edge meets R; R reaching x = 30 meets the hole's edge
    ([22, 52, 28, 58], 3, 0),
    ([22, 52, 30, 58], 3, T),
    ([12, 42, 18, 48], 3, T),                     # in the ring's body, no edge: winding 1
    ([9, 39, 41, 71], 3, E),
    # the Line at x = 60, hw = 2: R's left edge at 62 is at exactly hw
    ([62, 45, 63, 50], 4, T),
    ([up(62), 45, 63, 50], 4, 0),
    ([58, 38, 62, 62], 4, E),
    # the ellipse (90, 50), 10 x 5: ex = 10, (10 / 10)^2 + 0 = 1
    ([100, 50, 105, 52], 5, T),
    ([up(100), 50, 105, 52], 5, 0),
    ([80, 45, 100, 55], 5, E),
    # the Fill without area: its edge crosses R, the winding is 0 on both sides -- edges count
    ([114, 14, 116, 16], 6, T),
    ([114, 10, 116, 12], 6, 0),                   # beside it: all four s_k of both edges have one sign
    ([110, 10, 120, 20], 6, E),
    # the ellipse with ry = 0 contains no point (D13): nothing touches it and nothing encloses it, not even a rectangle around or across its box
    ([80, 60, 120, 80], 8, 0),
    ([95, 70, 105, 70], 8, 0),
    ([0, 0, 200, 200], 8, 0),
]
