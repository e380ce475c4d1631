"""Scenes and queries for snapping, pm_snap / pm_snap_device (test helper, not a conftest): tests/test_snap.py runs them against
tests/np_snap.py under the emulation and on the GPU, and pins on the CPU, with numpy alone, that the cases are what they claim.

The kernel (piet_metal_amd/csrc/pm_snap.h) walks the items WAVE at a time and reaches a Fill's or a Polyline's points through the
scene index, chunks of CHUNK_SEGS segments and super-chunks of SUPER_CHUNKS chunks, as the other query kernels do; it culls by the
distance from the query to a box against r.

  small_case   the ties scene below, mixed_scene and edge_scene (tests/test_hit_gpu.py), rect_cases' scene of non-finite points and a scene of ends at 1e30
               under seeded queries of every class: on vertices and on edges, at exactly r (3-4-5 offsets), one f32 step short,
               r = 0, invalid ones;
  walk_case    hit_structure.walk_scene at its WALK_SIZES: every item's own spot under several radii;
  long_case    hit_structure's loops, comb and fan between a lead and a trailing item, of 64 / 65 / 512 / 513 chunks exactly: queries
               next to named chunks' boxes at exactly r, between two strokes of different chunks at the same distance, ...
  KNOWN        hand-derived answers on the ties scene.

Expectations are np_snap's, computed once per (case, flags, skip, mask) and never written to."""
from __future__ import annotations

import numpy as np

import hit_structure as hs
import np_hit
import np_snap

F32 = np.float32
NONE = hs.NONE
WAVE = hs.WAVE
V, E = np_snap.VERTEX, np_snap.EDGE
FLAG_SETS = ((True, True), (True, False), (False, True))     # (vertices, edges)


class SnapCase:
    """A scene, queries float32 [n, 3] {x, y, r}, and a skip_items mask (uint32 [n_items], some words non-zero)."""

    def __init__(self, ident, scene, xyr, mask, **facts):
        self.ident, self.scene, self.facts = ident, scene, facts
        self.xyr = np.ascontiguousarray(xyr, F32).reshape(-1, 3)
        self.mask = np.ascontiguousarray(mask, np.uint32)
        assert len(self.mask) == len(np_hit.flat_items(bytes(scene)))
        self._want = {}

    def __repr__(self):
        return f"{self.ident} ({len(self.xyr)} queries)"

    def expected(self, vertices=True, edges=True, skip=False, masked=False):
        key = (vertices, edges, skip, masked)
        if key not in self._want:
            rec = np_snap.snap(self.scene, self.xyr, vertices, edges, skip, self.mask if masked else None)
            rec.setflags(write=False)
            self._want[key] = rec
        return self._want[key]


def down(v):
    return F32(np.nextafter(F32(v), F32(-np.inf)))


INVALID = np.array([[np.nan, 10, 5], [10, np.nan, 5], [10, 10, np.nan], [np.inf, 10, 5], [10, -np.inf, 5], [10, 10, np.inf], [10, 10, -1], [10, 10, -1e-30],
                    [30, 10, -0.0], [1.0e6, 1.0e6, 10], [-5000, 30, 100], [3.0e9, -3.0e9, 1.0e9], [200, 200, 1.0e30], [60, 60, 3.0e38], [70000, 20, 3000]])


def seeded_queries(scene, region, seed, extra=(), n_verts=40, n_segs=40, n_uniform=120):
    """Every class of query that does not need to know the scene's meaning: on vertices with r = 0 and r = 1; at (3, 4) / 4 and (-3, 4) from
    vertices with r = 1.25 and 5 -- d2 exact where the coordinates are quarter pixels -- and with r one f32 step short; on segments'
    middles, and 1.5 right of and below them with r = 1.5 and one step short; uniform points over `region` with radii from half a pixel
    to 100; invalid ones and ones far away."""
    from test_hit_gpu import scene_vertices_and_segments

    rng = np.random.default_rng(seed)
    verts, a, b = scene_vertices_and_segments(scene)
    verts = verts[np.isfinite(verts).all(axis=1)].astype(np.float64)
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    mids = (a[ok] + b[ok]) * 0.5
    verts = verts[:: max(len(verts) // n_verts, 1)]
    mids = mids[:: max(len(mids) // n_segs, 1)]
    col = lambda p, r: np.concatenate([p, np.full((len(p), 1), r, np.float64)], axis=1)  # noqa: E731
    out = [col(verts, 0.0), col(verts, 1.0), col(verts + (0.75, 1.0), 1.25), col(verts + (0.75, 1.0), down(1.25)), col(verts + (-3.0, 4.0), 5.0),
           col(verts + (-3.0, 4.0), down(5.0)), col(mids, 0.0), col(mids, 2.0), col(mids + (1.5, 0.0), 1.5), col(mids + (1.5, 0.0), down(1.5)),
           col(mids + (0.0, 1.5), 1.5), col(mids + (0.0, 1.5), down(1.5))]
    xa, ya, xb, yb = region
    c = rng.uniform(0.0, 1.0, (n_uniform, 2)) * (xb - xa, yb - ya) + (xa, ya)
    out.append(np.concatenate([c, rng.choice([0.5, 2.0, 8.0, 32.0, 100.0], (n_uniform, 1))], axis=1))
    out.append(INVALID)
    if len(extra):
        out.append(np.asarray(extra, np.float64).reshape(-1, 3))
    return np.concatenate(out).astype(F32)


# ---- the ties scene and its hand-derived answers -----------------------------------------------------------------------------

def ties_scene(pm):
    """Integer geometry.  0, 1: the same Polyline (10, 10) -> (30, 10) -> (30, 30) twice; 2: the Fill [50, 60] x [10, 20]; 3: the Fill
    [80, 90] x [10, 20] with its first point repeated as its last; 4: a Line (10, 50) -> (40, 50); 5: a Circle, centre (25, 54), radius 1;
    6: a compound Fill of the squares [100, 110] x [10, 20] and [110, 120] x [10, 20], which share the edge x = 110; 7: the Polyline of
    items 0 and 1 a third time, with alpha 0; 8: an ellipse with ry = 0, centre (140, 15): it offers nothing; 9: an ellipse, centre
    (140, 40), radii 10 and 5; 10: a Polyline of the one point (160, 15); 11: a Fill of quarter-pixel points."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)  # noqa: E731
    bend = np.array([[10.0, 10.0], [30.0, 10.0], [30.0, 30.0]])

    def emit(e):
        e.polyline(bend, 0x11AA22FF, 2.0)
        e.polyline(bend, 0x22BB33FF, 2.0)
        e.fill(sq(50, 10, 60, 20), 0x336699FF)
        e.fill(np.concatenate([sq(80, 10, 90, 20), [[80.0, 10.0]]]), 0x884400FF)
        e.stroke_line((10.0, 50.0), (40.0, 50.0), 1.0, 0x000000FF)
        e.circle((25.0, 54.0), 1.0)
        e.fill_compound([sq(100, 10, 110, 20), sq(110, 10, 120, 20)], 0xAA5500FF)
        e.polyline(bend, 0x33CC4400, 2.0)
        e.ellipse((140.0, 15.0), 10.0, 0.0)
        e.ellipse((140.0, 40.0), 10.0, 5.0)
        e.polyline(np.array([[160.0, 15.0]]), 0x445566FF, 3.0)
        e.fill(np.array([[20.25, 70.5], [60.75, 72.25], [44.5, 99.75], [12.0, 90.25]]), 0x9900CCFF)

    return hs._encode(pm, 12, emit)


Z = (NONE, 0, 0, 0.0, 0.0, 0.0, 0.0)
# (query {x, y, r}, (vertices, edges), skip_transparent, the record) -- each worked out by hand:
KNOWN = [
    # 1 above the Line (10, 50) -> (40, 50), 3 below the Circle's centre (25, 54): the vertex within r wins over the nearer edge
    ((25, 51, 4), (True, True), False, (5, V, 0, 0.0, 25.0, 54.0, 9.0)),
    # ... and the edge under PM_SNAP_EDGES alone: ap = (15, 1), ab = (30, 0), t = 450 / 900 = 0.5, c = (25, 50), d2 = 1
    ((25, 51, 4), (False, True), False, (4, E, 0, 0.5, 25.0, 50.0, 1.0)),
    # the centre of the square [50, 60] x [10, 20]: 5 from all four edges -- segment 0, (50, 10) -> (60, 10), has the smallest index
    ((55, 15, 5), (False, True), False, (2, E, 0, 0.5, 55.0, 10.0, 25.0)),
    # ... and sqrt(50) from all four vertices: vertex 0; r = 8 holds it (50 <= 64), r = 7 does not (50 > 49) and the edge answers
    ((55, 15, 8), (True, False), False, (2, V, 0, 0.0, 50.0, 10.0, 50.0)),
    ((55, 15, 7), (True, True), False, (2, E, 0, 0.5, 55.0, 10.0, 25.0)),
    ((55, 15, 7), (True, False), False, Z),
    # the bend (30, 10) of the three equal Polylines, r = 0: the topmost, item 7; without transparent items item 1; its segments 0 (t = 1)
    # and 1 (t = 0) both reach it: segment 0
    ((30, 10, 0), (True, True), False, (7, V, 1, 0.0, 30.0, 10.0, 0.0)),
    ((30, 10, 0), (True, True), True, (1, V, 1, 0.0, 30.0, 10.0, 0.0)),
    ((30, 10, 0), (False, True), False, (7, E, 0, 1.0, 30.0, 10.0, 0.0)),
    # the repeated point (80, 10) of item 3: entries 0 and 4, the smaller index; its edges there: segment 0 (t = 0), segment 3 (t = 1)
    # and the degenerate closing segment 4 -- segment 0
    ((80, 10, 0), (True, False), False, (3, V, 0, 0.0, 80.0, 10.0, 0.0)),
    ((80, 10, 0), (False, True), False, (3, E, 0, 0.0, 80.0, 10.0, 0.0)),
    # (3, 4) from the Polylines' first point: d2 = 9 + 16 = 25 = r * r exactly, a hit; one f32 step less of r, none (the bend is 17 away)
    ((13, 14, 5), (True, False), True, (1, V, 0, 0.0, 10.0, 10.0, 25.0)),
    ((13, 14, float(down(5))), (True, False), True, Z),
    # ... while the edge y = 10 is 4 away: ap = (3, 4), ab = (20, 0), t = 60 / 400 = 0.15, c = (13, 10)
    ((13, 14, float(down(5))), (True, True), True, (1, E, 0, F32(0.15), 13.0, 10.0, 16.0)),
    # the shared edge x = 110 of item 6's squares, from (110, 15): entries 1 (the first square's (110, 10) -> (110, 20)) and 8 (the second
    # square's closing segment (110, 20) -> (110, 10)) at d2 = 0: entry 1
    ((110, 15, 0), (False, True), False, (6, E, 1, 0.5, 110.0, 15.0, 0.0)),
    # an ellipse's centre; an ellipse with ry = 0 offers nothing, and nothing else is within 3 of it
    ((140, 40, 1), (True, True), False, (9, V, 0, 0.0, 140.0, 40.0, 0.0)),
    ((140, 15, 3), (True, True), False, Z),
    # the one-point Polyline: vertex 0, and under PM_SNAP_EDGES the degenerate segment 0 with t = 0
    ((160, 18, 3), (False, True), False, (10, E, 0, 0.0, 160.0, 15.0, 9.0)),
    ((160, 18, 3), (True, True), False, (10, V, 0, 0.0, 160.0, 15.0, 9.0)),
    # not a query: a NaN, r < 0
    ((np.nan, 10, 5), (True, True), False, Z),
    ((30, 10, -1), (True, True), False, Z),
]


def known_records():
    out = np.zeros(len(KNOWN), np_snap.RECORD)
    for k, (_, _, _, rec) in enumerate(KNOWN):
        out[k] = rec
    return out


TIES_EXTRA = [k[0] for k in KNOWN] + [(20, 10, 0), (20, 11, 1), (30, 20, 0.5), (115, 15, 5), (110, 10, 0), (105, 15, 5), (85, 15, 5), (85, 15, 8), (25, 52, 2)]

_small = {}
SMALL = ("ties", "mixed", "edge", "nonfinite", "absorbed")


def absorbed_scene(pm):
    """Segments with one end at 1e30, beyond a saturated side of the item's ShortBbox: b - a absorbs the near end, and D21's own
    c = a + ab * t is 0 at t = 1, far outside the side the box does bound (x0 = 64 999 or so).  0: a Polyline (1e30, 10) ->
    (65000.5, 10); 1: a Fill (1e30, 30), (65000.5, 30), (65000.5, 40); 2: a Polyline (420, 1e30) -> (420, 64000.25), the same along y;
    3: a Fill with a point at y = -1e30; 4: a Line from (1e30, 100)."""
    def emit(e):
        e.polyline(np.array([[1.0e30, 10.0], [65000.5, 10.0]]), 0x11AA22FF, 2.0)
        e.fill(np.array([[1.0e30, 30.0], [65000.5, 30.0], [65000.5, 40.0]]), 0x336699FF)
        e.polyline(np.array([[420.0, 1.0e30], [420.0, 64000.25]]), 0x22BB33FF, 1.0)
        e.fill(np.array([[700.0, -1.0e30], [700.0, 300.5], [710.0, 300.5]]), 0x884400FF)
        e.stroke_line((1.0e30, 100.0), (65100.0, 100.0), 1.0, 0x000000FF)

    return hs._encode(pm, 5, emit)


ABSORBED_EXTRA = [[100, 10, 200], [100, 30, 200], [100, 20, 150], [0, 10, 1], [0, 30, 0.5], [420, 100, 150], [425, 3, 6], [705, 100, 80], [0, 100, 2],
                  [65000.5, 10, 1], [65000.5, 35, 3], [64000, 10, 100], [420, 64000.25, 0], [420, 63000, 5]]


def small_case(pm, name):
    if name not in _small:
        import rect_cases as rc
        from test_hit_gpu import edge_scene, mixed_scene

        if name == "ties":
            scene = ties_scene(pm)
            xyr = seeded_queries(scene, (0, 0, 180, 110), 61, TIES_EXTRA)
        elif name == "mixed":
            scene = mixed_scene(pm)
            xyr = seeded_queries(scene, (-20, -20, 540, 540), 62)
        elif name == "edge":
            scene = edge_scene(pm)
            far = seeded_queries(scene, (64900, -40, 70700, 140), 64)[-(120 + len(INVALID)):]
            xyr = np.concatenate([seeded_queries(scene, (-80, -60, 120, 140), 63), far, [[65250, 17, 250], [-40, -30, 0], [70500, 40, 0.5]]]).astype(F32)
        elif name == "absorbed":
            scene = absorbed_scene(pm)
            near = seeded_queries(scene, (64900, -40, 65200, 140), 67)[-(120 + len(INVALID)):]
            xyr = np.concatenate([seeded_queries(scene, (-60, -60, 800, 400), 66, ABSORBED_EXTRA), near]).astype(F32)
        else:
            scene = rc.nonfinite_scene(pm)
            xyr = seeded_queries(scene, (-60, -20, 260, 260), 65, [[120, 30, 25], [200, 200, 5], [60, 85, 6], [40, 130, 12]])
        n_items = len(np_hit.flat_items(bytes(scene)))
        _small[name] = SnapCase(name, scene, xyr, np.where(np.arange(n_items) % 3 == 1, 7, 0))
    return _small[name]


# ---- the item walk -----------------------------------------------------------------------------------------------------

WALK_SIZES = hs.WALK_SIZES
_walks = {}


def walk_case(pm, n):
    """hit_structure.walk_scene of n items -- the first n // 2 in a child group, every third transparent.  Queries: every item's own
    spot with r = 0.5 (a Circle's centre, a Polyline's first point, a point of a Line: that item alone), 3 (the edges of a Fill's
    cell) and 4.5 (its corners too); the common point; a point with nothing near; the whole scene from afar."""
    if n not in _walks:
        case = hs.walk_scene(pm, n)
        spots = case.queries[:n].astype(np.float64)
        col = lambda p, r: np.concatenate([p, np.full((len(p), 1), r, np.float64)], axis=1)  # noqa: E731
        xyr = np.concatenate([col(spots, 0.5), col(spots, 3.0), col(spots, 4.5), [[*hs.COMMON, 0.0], [*hs.COMMON, 7.0], [*hs.NOTHING, 2.0], [*hs.NOTHING, 500.0],
                                                                                  [300.0, 300.0, 1000.0], [np.nan, 50.0, 5.0]]])
        _walks[n] = SnapCase(f"walk-{n}", case.scene, xyr, np.where(np.arange(n) % 4 == 2, 1, 0), n=n, kinds=case.facts["kinds"])
    return _walks[n]


# ---- long items --------------------------------------------------------------------------------------------------------

# (id, builder): the long item (hs.Case.long_item) has exactly `chunks` chunks; its first chunk sits at residue ceil(lead / 4) % 8
LONG = {
    "loops-64": (64, lambda pm: hs.loops_scene(pm, 51, 1, 28, True, 256)),
    "loops-65": (65, lambda pm: hs.loops_scene(pm, 51, 2, 32, True, 257)),
    "loops-512-r0": (512, lambda pm: hs.loops_scene(pm, 410, 0, 32, True, 2048)),
    "loops-512-r7": (512, lambda pm: hs.loops_scene(pm, 410, 3, 28, True, 2048)),
    "loops-513": (513, lambda pm: hs.loops_scene(pm, 410, 1, 32, True, 2049)),
    "comb-64": (64, lambda pm: hs.comb_scene(pm, 51, 3, False, 256)),
    "comb-65": (65, lambda pm: hs.comb_scene(pm, 51, 28, False, 260)),
    "comb-512": (512, lambda pm: hs.comb_scene(pm, 409, 32, False, 2048)),
    "comb-513": (513, lambda pm: hs.comb_scene(pm, 409, 28, False, 2050)),
    "fan-64": (64, lambda pm: hs.fan_scene(pm, 128, 3)),
    "fan-65": (65, lambda pm: hs.fan_scene(pm, 129, 28)),
    "fan-512": (512, lambda pm: hs.fan_scene(pm, 1024, 19)),
    "fan-513": (513, lambda pm: hs.fan_scene(pm, 1025, 24)),
}
LONG_IDS = list(LONG)
_longs = {}


def named_chunks(cb0, cb1):
    """Positions in the item of its first and last chunk, the chunks either side of its 64th, and the first chunk behind its 64th super-chunk."""
    n = cb1 - cb0
    pos = {0, n - 1} | {p for p in (63, 64) if p < n}
    behind = (cb0 // hs.SUPER_CHUNKS + WAVE) * hs.SUPER_CHUNKS - cb0
    if behind < n:
        pos.add(behind)
    return sorted(pos)


def long_case(pm, ident):
    """Queries: for every named chunk, 1/8 right of the middle of its box's right edge and 1/8 above the middle of its top edge with
    r = 1/8 and one f32 step short, its first, second and fourth point with r = 0, and (3, 4) / 64 from it with r = 5 / 64; about 110 of the builder's
    own queries -- between two strokes, on strokes, at the strokes' ends -- under radii from 0 to 8; a few with the whole item in
    reach."""
    if ident not in _longs:
        chunks, build = LONG[ident]
        case = build(pm)
        sc = bytes(case.scene)
        base, chunk_bbox, _ = hs.index_model(case.scene)
        cb0, cb1 = int(base[case.long_item]), int(base[case.long_item + 1])
        assert cb1 - cb0 == chunks, (ident, cb1 - cb0)
        pts = np_hit._points(sc, np_hit.flat_items(sc)[case.long_item][0]).astype(np.float64)
        q = []
        for p in named_chunks(cb0, cb1):
            x0, y0, x1, y1 = (float(v) for v in chunk_bbox[cb0 + p])
            ym, xm = np.round((y0 + y1) * 2.0) / 4.0, np.round((x0 + x1) * 2.0) / 4.0
            first = pts[hs.CHUNK_SEGS * p]
            if not np.isfinite(first).all():
                first = pts[hs.CHUNK_SEGS * p + 1]
            for k in (1, 3):   # (a fan's even points are all its hub: the odd ones are the chunk's own)
                if hs.CHUNK_SEGS * p + k < len(pts) and np.isfinite(pts[hs.CHUNK_SEGS * p + k]).all():
                    q.append([*pts[hs.CHUNK_SEGS * p + k], 0.0])
            q += [[x1 + 0.125, ym, 0.125], [x1 + 0.125, ym, down(0.125)], [xm, y0 - 0.125, 0.125], [xm, y0 - 0.125, down(0.125)], [first[0], first[1], 0.0],
                  [first[0] + 3.0 / 64, first[1] + 4.0 / 64, 5.0 / 64], [first[0] + 3.0 / 64, first[1] + 4.0 / 64, down(5.0 / 64)]]
        own = case.queries[:: max(len(case.queries) // 110, 1)].astype(np.float64)
        radii = np.array([0.0, 0.125, 0.1875, 0.25, 1.0, 8.0])[np.arange(len(own)) % 6]
        q = np.concatenate([np.array(q), np.concatenate([own, radii[:, None]], axis=1), [[150.0, 200.0, 600.0], [0.0, 0.0, 2000.0], [hs.MID, hs.MID, 1.0e9]]])
        _longs[ident] = SnapCase(ident, case.scene, q, np.where(np.arange(len(base) - 1) == case.long_item, 0, 3), chunks=chunks, long_item=case.long_item, cb0=cb0, cb1=cb1)
    return _longs[ident]
