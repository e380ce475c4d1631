"""Scenes and queries for snapping to intersections, pm_snap_intersections / pm_snap_intersections_device (test helper, not a
conftest): tests/test_snap_cross.py runs them against tests/np_cross.py under the emulation and on the GPU, and pins on the CPU, with
numpy alone, that the cases are what they claim.

The kernel (piet_metal_amd/csrc/pm_snap_cross.h) walks the items WAVE at a time as pm_snap_kernel does, lists the edges within r of
the cursor in LDS -- at most MAX_NEAR of them -- and then looks at every pair of the list.

  small_case   the ties scene below, mixed_scene and edge_scene (tests/test_hit_gpu.py), and snap_cases' scenes of non-finite points and
               of ends at 1e30, under seeded queries of every class: on a crossing with r = 0, at exactly r (3-4-5 offsets), one f32 step
               short, uniform ones, invalid ones;
  walk_case    n items, of which the first and the last are two rails that every item in between crosses and that cross each other;
  long_case    a Fill (loops), a compound Fill (comb) and a Polyline (zigzag) of 64 / 65 / 512 / 513 chunks exactly, between a lead and a trailing
               item, each crossed by short Lines in its named chunks;
  limit_case   a zigzag of K segments near one cursor above two Lines that cross: 511, 512 and 513 near edges;
  KNOWN        hand-derived answers on the ties scene.

Expectations are np_cross's, computed once per (case, skip, mask) and never written to."""
from __future__ import annotations

import numpy as np

import hit_structure as hs
import np_cross
import np_hit
import np_snap
import snap_cases as sc

F32 = np.float32
NONE = hs.NONE
WAVE = hs.WAVE
X, MANY = np_cross.INTERSECTION, np_cross.TOO_MANY
MAX_NEAR = np_cross.MAX_NEAR
down = sc.down
INVALID = sc.INVALID


class CrossCase:
    """A scene, queries float32 [n, 3] {x, y, r}, and a skip_items mask (uint32 [n_items], some words non-zero)."""

    def __init__(self, ident, scene, xyr, mask, **facts):
        self.ident, self.scene, self.facts = ident, scene, facts
        self.xyr = np.ascontiguousarray(xyr, F32).reshape(-1, 3)
        self.mask = np.ascontiguousarray(mask, np.uint32)
        assert len(self.mask) == len(np_hit.flat_items(bytes(scene)))
        self._want = {}

    def __repr__(self):
        return f"{self.ident} ({len(self.xyr)} queries)"

    def expected(self, skip=False, masked=False):
        key = (skip, masked)
        if key not in self._want:
            rec = np_cross.cross(self.scene, self.xyr, skip, self.mask if masked else None)
            rec.setflags(write=False)
            self._want[key] = rec
        return self._want[key]


def crossings(scene, limit=None):
    """float64 [C, 2]: the point of every pair of the scene's edges that is a candidate by D23 (no cursor: every pair of all edges)."""
    E = np_cross.Edges(bytes(scene))
    i, j = np.triu_indices(E.n, 1)
    shared, den, t, u, px, py, _ = np_cross.pair_parts(E.a[i], E.b[i], E.a[j], E.b[j], 0.0, 0.0)
    with np.errstate(invalid="ignore"):
        ok = ~shared & (den != 0) & (0 <= t) & (t <= 1) & (0 <= u) & (u <= 1) & np.isfinite(px) & np.isfinite(py)
    p = np.stack([px[ok], py[ok]], axis=1)
    p = p[np.unique(p.astype(F32), axis=0, return_index=True)[1]]
    if limit is not None and len(p) > limit:
        p = p[:: -(-len(p) // limit)]
    return p


def seeded_queries(scene, region, seed, extra=(), n_cross=40, n_mids=15, n_uniform=120):
    """Every class of query that does not need to know the scene's meaning: on crossings (and on a few edges' middles, where edges are near
    and, mostly, nothing crosses) with r = 0 and r = 1; at (3, 4) / 4 and (-3, 4) from them with r = 1.25 and 5 -- d2 exact where the crossing is on quarter pixels -- and with r one f32 step short; uniform
    points over `region` with radii from half a pixel to 100; invalid ones and ones far away."""
    rng = np.random.default_rng(seed)
    E = np_cross.Edges(bytes(scene))
    mids = ((E.a.astype(np.float64) + E.b) * 0.5)[:: max(E.n // n_mids, 1)]
    pts = np.concatenate([crossings(scene, n_cross), mids[np.isfinite(mids).all(axis=1)]])
    col = lambda p, r: np.concatenate([p, np.full((len(p), 1), r, np.float64)], axis=1)  # noqa: E731
    out = [col(pts, 0.0), col(pts, 1.0), col(pts + (0.75, 1.0), 1.25), col(pts + (0.75, 1.0), down(1.25)), col(pts + (-3.0, 4.0), 5.0),
           col(pts + (-3.0, 4.0), down(5.0)), col(pts + (0.0, 1.5), 1.5), col(pts + (0.0, 1.5), down(1.5))]
    xa, ya, xb, yb = region
    c = rng.uniform(0.0, 1.0, (n_uniform, 2)) * (xb - xa, yb - ya) + (xa, ya)
    out.append(np.concatenate([c, rng.choice([0.5, 2.0, 8.0, 32.0, 100.0], (n_uniform, 1))], axis=1))
    out.append(INVALID)
    if len(extra):
        out.append(np.asarray(extra, np.float64).reshape(-1, 3))
    return np.concatenate(out).astype(F32)


# ---- the ties scene and its hand-derived answers -----------------------------------------------------------------------------

def ties_scene(pm):
    """Integer geometry.  0, 1, 2: the Lines (0, 0) -> (8, 8), (0, 8) -> (8, 0) and (4, 0) -> (4, 8) through (4, 4): three pairs share a d2;
    3: a Line (20, 0) -> (28, 8), 4 and 5: the Line (20, 8) -> (28, 0) twice: the same crossing (24, 4) in two items (4 and 5 are collinear,
    overlap and share both ends); 6: the Polyline (40, 0) -> (48, 8) -> (48, 0) -> (40, 8), whose segments 0 and 2 cross at (44, 4): a pair
    within one item; 7: a Line (60, 0) -> (60, 8) and 8: a Line (60, 4) -> (68, 4) that ends ON it: a T-junction; 9: a Polyline (80, 0) ->
    (88, 0) -> (88, 8): edges that share an end and nothing else; 10, 11: the parallel Lines y = 0 and y = 2 over [100, 108]; 12: a Line
    (104, 0) -> (112, 0), collinear with 10 and overlapping it; 13: a Polyline of the one point (120, 4), a degenerate edge ON 14: a Line
    (116, 4) -> (124, 4); 15: a Line (0, 4) -> (8, 4) through (4, 4) with alpha 0; 16: the Fill [130, 140] x [0, 10], crossed by 17: a Line
    (125, 5) -> (145, 5) in its segment 1 and its closing segment 3; 18: a Circle on the Line 17, which offers nothing; 19: a compound
    Fill of two triangles that cross each other."""
    tri = lambda x, y: np.array([[x, y], [x + 12.0, y], [x + 6.0, y + 8.0]])  # noqa: E731

    def emit(e):
        e.stroke_line((0.0, 0.0), (8.0, 8.0), 1.0, 0x000000FF)
        e.stroke_line((0.0, 8.0), (8.0, 0.0), 1.0, 0x111111FF)
        e.stroke_line((4.0, 0.0), (4.0, 8.0), 1.0, 0x222222FF)
        e.stroke_line((20.0, 0.0), (28.0, 8.0), 1.0, 0x333333FF)
        e.stroke_line((20.0, 8.0), (28.0, 0.0), 1.0, 0x444444FF)
        e.stroke_line((20.0, 8.0), (28.0, 0.0), 1.0, 0x555555FF)
        e.polyline(np.array([[40.0, 0.0], [48.0, 8.0], [48.0, 0.0], [40.0, 8.0]]), 0x11AA22FF, 2.0)
        e.stroke_line((60.0, 0.0), (60.0, 8.0), 1.0, 0x666666FF)
        e.stroke_line((60.0, 4.0), (68.0, 4.0), 1.0, 0x777777FF)
        e.polyline(np.array([[80.0, 0.0], [88.0, 0.0], [88.0, 8.0]]), 0x22BB33FF, 2.0)
        e.stroke_line((100.0, 0.0), (108.0, 0.0), 1.0, 0x888888FF)
        e.stroke_line((100.0, 2.0), (108.0, 2.0), 1.0, 0x999999FF)
        e.stroke_line((104.0, 0.0), (112.0, 0.0), 1.0, 0xAAAAAAFF)
        e.polyline(np.array([[120.0, 4.0]]), 0x445566FF, 3.0)
        e.stroke_line((116.0, 4.0), (124.0, 4.0), 1.0, 0xBBBBBBFF)
        e.stroke_line((0.0, 4.0), (8.0, 4.0), 1.0, 0xCCCCCC00)
        e.fill(np.array([[130.0, 0.0], [140.0, 0.0], [140.0, 10.0], [130.0, 10.0]]), 0x336699FF)
        e.stroke_line((125.0, 5.0), (145.0, 5.0), 1.0, 0xDDDDDDFF)
        e.circle((135.0, 5.0), 2.0)
        e.fill_compound([tri(160.0, 0.0), tri(160.0, 4.0) * (1.0, -1.0) + (0.0, 12.0)], 0xAA5500FF)

    return hs._encode(pm, 20, emit)


Z = (NONE, 0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0)
# (query {x, y, r}, skip_transparent, the record without n_near, n_near) -- each worked out by hand:
KNOWN = [
    # the issue's own: without the transparent item 15 the Lines 0, 1 and 2 are within 2 of (5, 4) -- 1 / sqrt(2), 1 / sqrt(2) and 1 away --
    # and cross at (4, 4), d2 = 1.  Three pairs, one d2: the first edge of the topmost item, 2, then the second edge of the topmost
    # item, 1.  e = 2: (4, 0) -> (4, 8), f = 1: (0, 8) -> (8, 0): r = (0, 8), s = (8, -8), den = 0 * -8 - 8 * 8 = -64, w = (-4, 8),
    # t = (-4 * -8 - 8 * 8) / -64 = 0.5, u = (-4 * 8 - 8 * 0) / -64 = 0.5
    ((5, 4, 2), True, (2, X, 0, 0.5, 4.0, 4.0, 1.0, 1, 0, 0.5), 3),
    # ... with item 15, (0, 4) -> (8, 4), which passes through the cursor: first edge 15, second edge 2: r = (8, 0), s = (0, 8), den = 64,
    # w = (4, -4), t = (4 * 8 - -4 * 0) / 64 = 0.5, u = (4 * 0 - -4 * 8) / 64 = 0.5
    ((5, 4, 2), False, (15, X, 0, 0.5, 4.0, 4.0, 1.0, 2, 0, 0.5), 4),
    # the Lines (0, 0) -> (8, 8) and (0, 8) -> (8, 0) alone, the issue's example: item 2 and item 15 taken out by skip_items (see KNOWN_MASK)
    # e = 1: (0, 8) -> (8, 0), f = 0: r = (8, -8), s = (8, 8), den = 64 + 64 = 128, w = (0, -8), t = (0 + 64) / 128, u = (0 + 64) / 128
    ((5, 4, 2), "mask", (1, X, 0, 0.5, 4.0, 4.0, 1.0, 0, 0, 0.5), 2),
    # r = 0 exactly on the dyadic crossing (24, 4): the pairs (5, 3) and (4, 3) tie, the first edge of the topmost item wins; 4 and 5 share
    # their ends and are no pair.  e = 5: (20, 8) -> (28, 0), f = 3: (20, 0) -> (28, 8): as above with w = (0, -8)
    ((24, 4, 0), False, (5, X, 0, 0.5, 24.0, 4.0, 0.0, 3, 0, 0.5), 3),
    # the Polyline 6 crosses itself: segments 0 and 2, the smaller index first.  e: (40, 0) -> (48, 8), f: (48, 0) -> (40, 8): r = (8, 8),
    # s = (-8, 8), den = 64 + 64 = 128, w = (8, 0), t = 64 / 128, u = (8 * 8 - 0) / 128.  From (44, 7): d2 = 9 = r * r exactly; segment 1,
    # x = 48, is 4 away.  One f32 step less of r: the two segments, 3 / sqrt(2) away, are still near, their crossing is not within r
    ((44, 7, 3), False, (6, X, 0, 0.5, 44.0, 4.0, 9.0, 6, 2, 0.5), 2),
    ((44, 7, float(down(3))), False, Z, 2),
    # the T-junction: e = 8: (60, 4) -> (68, 4), f = 7: (60, 0) -> (60, 8): r = (8, 0), s = (0, 8), den = 64, w = (0, -4), t = 0 / 64 = 0,
    # u = (0 * 0 - -4 * 8) / 64 = 0.5
    ((63, 8, 5), False, (8, X, 0, 0.0, 60.0, 4.0, 25.0, 7, 0, 0.5), 2),
    # edges that share an end are no pair: the bend (88, 0) of item 9, both segments near
    ((88, 0, 1), False, Z, 2),
    # parallel, and collinear and overlapping: den = 0.  Items 10, 11 and 12 within 3 of (106, 1)
    ((106, 1, 3), False, Z, 3),
    # a degenerate edge ON a Line: den = 0
    ((120, 4, 1), False, Z, 2),
    # the Fill 16 and the Line 17: (140, 5) in the Fill's segment 1, (140, 0) -> (140, 10).  e = 17: r = (20, 0), s = (0, 10), den = 200,
    # w = (15, -5), t = 150 / 200 = 0.75, u = (15 * 0 - -5 * 20) / 200 = 0.5; the Circle 18 offers nothing
    ((139, 5, 1), False, (17, X, 0, 0.75, 140.0, 5.0, 1.0, 16, 1, 0.5), 2),
    # ... and (130, 5) in its closing segment 3, (130, 10) -> (130, 0): den = 20 * -10 = -200, w = (5, 5), t = (5 * -10 - 0) / -200 = 0.25,
    # u = (5 * 0 - 5 * 20) / -200 = 0.5
    ((131, 5, 1), False, (17, X, 0, 0.25, 130.0, 5.0, 1.0, 16, 3, 0.5), 2),
    # not a query: a NaN, r < 0 -- n_near is 0 too
    ((np.nan, 4, 5), False, Z, 0),
    ((4, 4, -1), False, Z, 0),
]
KNOWN_MASK_ITEMS = (2, 15)


def known_mask():
    m = np.zeros(20, np.uint32)
    m[list(KNOWN_MASK_ITEMS)] = 1
    return m


def known_records():
    out = np.zeros(len(KNOWN), np_cross.RECORD)
    for k, (_, _, rec, n_near) in enumerate(KNOWN):
        out[k] = rec + (n_near,)
    return out


TIES_EXTRA = [k[0] for k in KNOWN] + [(4, 4, 0), (4, 4, 0.5), (24, 5, 1), (60, 4, 0), (135, 5, 6), (166, 6, 8), (166, 6, 2), (4, 5, 1), (60, 3, 1), (100, 1, 1)]

_small = {}
SMALL = ("ties", "mixed", "edge", "nonfinite", "absorbed")


def small_case(pm, name):
    if name not in _small:
        import rect_cases as rc
        from test_hit_gpu import edge_scene, mixed_scene

        if name == "ties":
            scene = ties_scene(pm)
            xyr = seeded_queries(scene, (-10, -10, 180, 20), 71, TIES_EXTRA)
        elif name == "mixed":
            scene = mixed_scene(pm)
            xyr = seeded_queries(scene, (-20, -20, 540, 540), 72)
        elif name == "edge":
            scene = edge_scene(pm)
            far = seeded_queries(scene, (64900, -40, 70700, 140), 74)[-(120 + len(INVALID)):]
            xyr = np.concatenate([seeded_queries(scene, (-80, -60, 120, 140), 73), far, [[65250, 17, 250], [-40, -30, 0], [70500, 40, 0.5]]]).astype(F32)
        elif name == "absorbed":
            scene = sc.absorbed_scene(pm)
            near = seeded_queries(scene, (64900, -40, 65200, 140), 77)[-(120 + len(INVALID)):]
            xyr = np.concatenate([seeded_queries(scene, (-60, -60, 800, 400), 76, sc.ABSORBED_EXTRA), near]).astype(F32)
        else:
            scene = rc.nonfinite_scene(pm)
            xyr = seeded_queries(scene, (-60, -20, 260, 260), 75, [[120, 30, 25], [200, 200, 5], [60, 85, 6], [40, 130, 12]])
        n_items = len(np_hit.flat_items(bytes(scene)))
        _small[name] = CrossCase(name, scene, xyr, np.where(np.arange(n_items) % 3 == 1, 7, 0))
    return _small[name]


# ---- the item walk -----------------------------------------------------------------------------------------------------

WALK_SIZES = hs.WALK_SIZES
WALK_KINDS = ("line", "polyline", "fill", "circle", "compound")
_walks = {}


def walk_kind(i, n):
    return "rail" if i in (0, n - 1) else WALK_KINDS[i % len(WALK_KINDS)]


def walk_case(pm, n):
    """n items.  Item 0 is the rail y = 3 and item n - 1 (n >= 2) the rail from (-10, 5) to (8 n + 10, 1), which crosses it half way, at
    (4 n, 3); item i in between stands on x in [8 i, 8 i + 4] over y in [0, 8] and crosses both rails -- a Line, a Polyline of two segments, a
    triangle, a Circle (which offers nothing), a compound Fill of two triangles --, every third of them transparent.  Queries: every item's
    own spot (8 i + 2, 4) with r = 3 (the item's edges and the rails) and r = 0.75 (nothing, or an edge alone); the rails' own crossing;
    a point with nothing near; the whole scene from afar."""
    if n not in _walks:
        tri = lambda x: np.array([[x, 0.0], [x + 4.0, 0.0], [x + 2.0, 8.0]])  # noqa: E731
        kinds = [walk_kind(i, n) for i in range(n)]
        far = 8.0 * n + 10.0

        def emit(e):
            for i, kind in enumerate(kinds):
                x = 8.0 * i
                alpha = 0x00 if i % 3 == 1 else 0xFF
                if kind == "rail":
                    e.stroke_line((-10.0, 3.0), (far, 3.0), 1.0, 0x102030FF) if i == 0 else e.stroke_line((-10.0, 5.0), (far, 1.0), 1.0, 0x302010FF)
                elif kind == "line":
                    e.stroke_line((x, 0.0), (x + 4.0, 8.0), 1.0, 0x44556600 | alpha)
                elif kind == "polyline":
                    e.polyline(np.array([[x, 0.0], [x + 2.0, 8.0], [x + 4.0, 0.0]]), 0x11AA2200 | alpha, 1.0)
                elif kind == "fill":
                    e.fill(tri(x), 0x33669900 | alpha)
                elif kind == "circle":
                    e.circle((x + 2.0, 4.0), 2.0)
                else:
                    e.fill_compound([tri(x), tri(x) * (1.0, 0.5) + (0.0, 2.0)], 0xAA550000 | alpha)

        scene = hs._encode(pm, n, emit)
        spots = np.stack([8.0 * np.arange(n) + 2.0, np.full(n, 4.0)], axis=1)
        col = lambda p, r: np.concatenate([p, np.full((len(p), 1), r, np.float64)], axis=1)  # noqa: E731
        meet = (4.0 * n, 3.0)
        xyr = np.concatenate([col(spots, 3.0), col(spots, 0.75), col(spots + (0.0, -1.0), 1.0), [[*meet, 0.0], [*meet, 2.0], [meet[0] + 3.0, 7.0, 5.0], [-30.0, 40.0, 2.0],
                                                                                                 [-30.0, 40.0, 500.0], [4.0 * n, 4.0, 4000.0], [np.nan, 4.0, 5.0]]])
        _walks[n] = CrossCase(f"walk-{n}", scene, xyr, np.where(np.arange(n) % 4 == 2, 1, 0), n=n, kinds=kinds)
    return _walks[n]


# ---- long items --------------------------------------------------------------------------------------------------------

# id: (chunks, what the long item is, its points or sub-paths, the lead item's point count)
def _comb_subs(n, entries):
    """n rectangles [r, r + 1/8] x [T, B] at r = R0 + k / 2, five entries each with their separator; the first entries - 5 n of them have a
    fifth point in the middle of their second stroke."""
    subs = []
    for k in range(n):
        r = hs.R0 + 0.5 * k
        rect = [(r, hs.T), (r + 0.125, hs.T), (r + 0.125, hs.B), (r, hs.B)]
        if k < entries - 5 * n:
            rect.insert(2, (r + 0.125, hs.MID + 17.0))
        subs.append(np.array(rect))
    assert sum(len(s) + 1 for s in subs) == entries
    return subs


def _zigzag_points(segs):
    """A square wave of `segs` segments: strokes at x = R0 + m / 4 between y = T and y = B, down and up in turn, joined by runs of a quarter
    pixel along y = B and y = T.  Segment 2 m is the stroke at x_m, segment 2 m + 1 the run to x_(m + 1): a chunk's first stroke lies ON its
    chunk box's left edge."""
    j = np.arange(segs + 1)
    return np.stack([hs.R0 + 0.25 * (j // 2), np.where(np.isin(j % 4, (0, 3)), hs.T, hs.B)], axis=1)


LONG = {
    "loops-64": (64, "fill", lambda: hs.loops_points(51, 1, 1, npt=256)[0], 28),
    "loops-65": (65, "fill", lambda: hs.loops_points(51, 2, 1, npt=257)[0], 32),
    "loops-512": (512, "fill", lambda: hs.loops_points(410, 3, 1, npt=2048)[0], 28),
    "loops-513": (513, "fill", lambda: hs.loops_points(410, 1, 1, npt=2049)[0], 28),
    "comb-64": (64, "compound", lambda: _comb_subs(51, 256), 3),
    "comb-65": (65, "compound", lambda: _comb_subs(51, 260), 28),
    "comb-512": (512, "compound", lambda: _comb_subs(409, 2048), 32),
    "comb-513": (513, "compound", lambda: _comb_subs(410, 2050), 28),
    "zigzag-64": (64, "polyline", lambda: _zigzag_points(256), 3),
    "zigzag-65": (65, "polyline", lambda: _zigzag_points(258), 28),
    "zigzag-512": (512, "polyline", lambda: _zigzag_points(2048), 19),
    "zigzag-513": (513, "polyline", lambda: _zigzag_points(2049), 24),
}
LONG_IDS = list(LONG)
LONG_ITEM = 1
# the last chunk of these is the Fill's closing segment alone, the return stroke at x = L, which lies ON every earlier return stroke: a
# crossing there is won by the smallest index, another chunk's (tests/test_snap.py has the same exception)
LONE_CLOSING = ("loops-65", "loops-513")
_longs = {}


def _long_scene(pm, kind, geo, lead, lines):
    def emit(e):
        e.fill(hs.lead_points(lead) + (300.0, 400.0), 0x336699FF)
        if kind == "fill":
            e.fill(geo, 0xAA5500FF, even_odd=True)
        elif kind == "compound":
            e.fill_compound(geo, 0xAA5500FF)
        else:
            e.polyline(geo, 0xAA5500FF, 0.25)
        e.fill(np.array([[600.0, 10.0], [604.0, 10.0], [602.0, 430.0]]), 0x2244CCFF)
        for a, b in lines:
            e.stroke_line(tuple(a), tuple(b), 0.5, 0x000000FF)

    return hs._encode(pm, 3 + len(lines), emit, cap=1 << 19)


def long_case(pm, ident):
    """The long item is item 1, between a lead Fill that shifts its first chunk and a trailing Fill.  For every named chunk (snap_cases.
    named_chunks: the first, the last, those either side of the 64th, the first behind the 64th super-chunk) a short Line along (1, 1), an item
    of its own on top, crosses a point M of one of the chunk's segments: the middle of a vertical stroke ON the chunk box's left or right edge
    if the chunk has one, else the middle of another segment or, of a run along y = T or y = B, a point 1/16 from its far end.  The loops'
    return strokes and runs lie on one another: M is taken only where the segment has the smallest index of all the item's edges through M,
    so that the crossing is won in the named chunk (facts["named"] leaves out the lone closing chunk of LONE_CLOSING, where no such point
    exists).  Queries: M with r = 0 and r = 1; (3, 4) / 64 from M with r = 5 / 64 and one f32 step short; 1/8 beside M, outside the chunk's box
    where the stroke is on its edge, with r = 1/8 and one step short -- that edge, the segment and the crossing are then all at exactly r --;
    a few with many edges or the whole item in reach."""
    if ident not in _longs:
        chunks, kind, build, lead = LONG[ident]
        geo = build()
        bare = _long_scene(pm, kind, geo, lead, [])
        base, chunk_bbox, _ = hs.index_model(bare)
        cb0, cb1 = int(base[LONG_ITEM]), int(base[LONG_ITEM + 1])
        assert cb1 - cb0 == chunks, (ident, cb1 - cb0)
        E = np_cross.Edges(bytes(bare), skip_items=np.arange(3) != LONG_ITEM)
        order = np.argsort(E.index)
        index, a32, b32 = E.index[order], E.a[order], E.b[order]
        a, b = a32.astype(np.float64), b32.astype(np.float64)
        named = [p for p in sc.named_chunks(cb0, cb1) if not (ident in LONE_CLOSING and p == chunks - 1)]
        lines, mids, seg_of, sides = [], [], [], []
        for p in named:
            bb = chunk_bbox[cb0 + p].astype(np.float64)
            mine = np.flatnonzero(index // hs.CHUNK_SEGS == p)
            on_edge = (a[mine, 0] == b[mine, 0]) & (a[mine, 1] != b[mine, 1]) & ((a[mine, 0] == bb[0]) | (a[mine, 0] == bb[2]))
            chosen = None
            for k in list(mine[on_edge]) + list(mine[~on_edge]):
                spots = [(a[k] + b[k]) * 0.5]
                if a[k, 1] == b[k, 1] and a[k, 0] != b[k, 0]:
                    spots.append(np.array([max(a[k, 0], b[k, 0]) - 0.0625, a[k, 1]]))
                for m in spots:
                    through = np_snap.edge_d2(a32, b32, m[:1], m[1:])[0] == 0.0
                    if through[k] and index[through].min() == index[k]:
                        chosen = (k, m)
                        break
                if chosen:
                    break
            assert chosen is not None, (ident, p)
            k, m = chosen
            lines.append((m - 1.0, m + 1.0))
            mids.append(m)
            seg_of.append(int(index[k]))
            sides.append(-1.0 if a[k, 0] == b[k, 0] == bb[0] and bb[0] != bb[2] else 1.0)
        scene = _long_scene(pm, kind, geo, lead, lines)
        q = []
        for m, side in zip(mids, sides):
            q += [[*m, 0.0], [*m, 1.0], [m[0] + 3.0 / 64, m[1] + 4.0 / 64, 5.0 / 64], [m[0] + 3.0 / 64, m[1] + 4.0 / 64, down(5.0 / 64)],
                  [m[0] + side * 0.125, m[1], 0.125], [m[0] + side * 0.125, m[1], down(0.125)], [m[0] - 0.5, m[1] + 0.25, 2.0]]
        q += [[150.0, 200.0, 30.0], [150.0, 200.0, 600.0], [0.0, 0.0, 2000.0], [hs.MID, hs.MID, 1.0e9], [20.0, 20.0, 3.0]]
        _longs[ident] = CrossCase(ident, scene, q, np.where(np.arange(3 + len(lines)) == 3, 3, 0), chunks=chunks, cb0=cb0, cb1=cb1, mids=np.array(mids),
                                  segments=seg_of, named=named, kind=kind)
    return _longs[ident]


# ---- the limit -----------------------------------------------------------------------------------------------------------

LIMIT_NEAR = (MAX_NEAR - 1, MAX_NEAR, MAX_NEAR + 1)
LIMIT_CURSOR = (15.0, 10.0)
_limits = {}


def limit_case(pm, n_near):
    """Items 0 and 1: the Lines (19, 9) -> (21, 11) and (19, 11) -> (21, 9), which cross at (20, 10), 5 from the cursor (15, 10); item 2, on top:
    a zigzag Polyline of n_near - 2 segments between x = 9 and x = 9.5 over y in 10 -+ 1, every segment between 5.5 and 6 from the cursor:
    with r = 6 all n_near edges are near -- the zigzag's are listed first, the two Lines are the last two stored --, with r = 5.25 the two
    Lines alone.  A zigzag's segments share ends with their neighbours and cross no other."""
    if n_near not in _limits:
        k = n_near - 2
        j = np.arange(k + 1)
        zig = np.stack([9.0 + 0.5 * (j % 2), 10.0 + (j - k // 2) / 256.0], axis=1)

        def emit(e):
            e.stroke_line((19.0, 9.0), (21.0, 11.0), 1.0, 0x000000FF)
            e.stroke_line((19.0, 11.0), (21.0, 9.0), 1.0, 0x111111FF)
            e.polyline(zig, 0x11AA22FF, 1.0)

        xyr = [[*LIMIT_CURSOR, 6.0], [*LIMIT_CURSOR, 5.25], [*LIMIT_CURSOR, 5.0], [*LIMIT_CURSOR, down(5.0)], [9.25, 10.0, 0.25], [9.25, 10.0, 12.0], [20.0, 10.0, 0.0]]
        _limits[n_near] = CrossCase(f"limit-{n_near}", hs._encode(pm, 3, emit), xyr, [0, 0, 1], n_near=n_near)
    return _limits[n_near]
