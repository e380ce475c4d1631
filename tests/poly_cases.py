"""Scenes and query polygons for the polygon queries of decision D20 (test helper, not a conftest): tests/test_hit_polygon.py runs them on
the device and pins on the CPU, with tests/np_poly.py alone, that the cases are what they claim.  They are laid out for a kernel that walks the items
WAVE at a time through the scene index (as pm_select_rect_kernel does) and keeps a box for every GROUP edges of the polygon:

  small_case     rect_cases' mixed / edge / non-finite scenes, the oracle's path test and a scene of loose outlines under ~200 seeded
                 polygons of every class;
  walk_case      hit_frame_cases.walk_scene at rect_cases.WALK_SIZES items;
  long_case      rect_cases' long Fills and Polylines: polygons decided by one segment of the last chunk, by the winding alone, by
                 all points inside;
  size_case      one scene under polygons of M_SIZES vertices;
  origin_case    strokes near (0, 0) under polygons with vertices of 2^60 and 2^100: distances that rounding decides;
  int_scene      integer coordinates: rectangles as 4-gons against D19 (INT_RECTS);
  known_scene    rect_cases' own, with hand-derived answers (KNOWN).

Expectations are np_poly's, computed once per (case, polygon, flags) and never written to."""
from __future__ import annotations

import numpy as np

import hit_frame_cases as fc
import hit_structure as hs
import np_hit
import np_poly
import rect_cases as rc

F32 = np.float32
WAVE = rc.WAVE
GROUP, MAX_VERTICES = 16, 4096   # kPolyGroup, kPolyMaxVertices (pm_hit_poly.h)
# one below / at / one above: a group of edges, a wave (the kernel's round of points), 16 groups; and the ends of the allowed range
M_SIZES = (3, GROUP - 1, GROUP, GROUP + 1, WAVE - 1, WAVE, WAVE + 1, 16 * GROUP - 1, 16 * GROUP, 16 * GROUP + 1, MAX_VERTICES - 1, MAX_VERTICES)
COMBOS = [(False, False), (False, True), (True, False), (True, True)]   # (skip_transparent, even_odd)


class PolyCase:
    """A scene and query polygons, each float32 [m, 2]."""

    def __init__(self, ident, scene, polys, **facts):
        self.ident, self.scene, self.facts = ident, scene, facts
        self.polys = [np.ascontiguousarray(p, F32).reshape(-1, 2) for p in polys]
        self._want = {}

    def __repr__(self):
        return f"{self.ident} ({len(self.polys)} polygons)"

    def flags(self, k, skip=False, even_odd=False):
        """uint8 [n_items] by np_poly."""
        key = (k, skip, even_odd)
        if key not in self._want:
            f = np_poly.item_flags(self.scene, self.polys[k], skip, even_odd)
            f.setflags(write=False)
            self._want[key] = f
        return self._want[key]

    def table(self, skip=False, even_odd=False):
        """uint8 [n_items, n_polys]."""
        return np.stack([self.flags(k, skip, even_odd) for k in range(len(self.polys))], axis=1)


# ---- polygon builders ------------------------------------------------------------------------------------------------------

def ngon(c, r, n, phase=0.0, radii=None):
    t = phase + 2 * np.pi * np.arange(n) / n
    rad = r if radii is None else r * np.asarray(radii)
    return np.stack([c[0] + rad * np.cos(t), c[1] + rad * np.sin(t)], axis=1)


def box(x0, y0, x1, y1, reverse=False):
    p = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)
    return p[::-1] if reverse else p


def bowtie(c, r):
    return np.array([[c[0] - r, c[1] - r], [c[0] + r, c[1] + r], [c[0] + r, c[1] - r], [c[0] - r, c[1] + r]], np.float64)


def pentagram(c, r):
    """Five vertices, every second one of a pentagon: winding 2 in the centre (a hole under even-odd), 1 in the tips."""
    return np.array([[c[0] + r * np.sin(4 * np.pi * k / 5), c[1] - r * np.cos(4 * np.pi * k / 5)] for k in range(5)])


def notch(x0, y0, x1, y1, t):
    """A "C" of thickness t, open to the right: the box [x0 + t, x1] x [y0 + t, y1 - t] is its notch."""
    return np.array([[x0, y0], [x1, y0], [x1, y0 + t], [x0 + t, y0 + t], [x0 + t, y1 - t], [x1, y1 - t], [x1, y1], [x0, y1]], np.float64)


def holed(outer, inner):
    """The box `outer`, a bridge from its first corner to the box `inner` run the other way round, and back: `inner` has winding 0."""
    o, i = box(*outer), box(*inner, reverse=True)
    return np.concatenate([o, o[:1], i, i[:1]])


def lasso(c, r, m, seed):
    """m vertices around c, radii between 0.8 r and r."""
    rng = np.random.default_rng(seed)
    return ngon(c, r, m, radii=rng.uniform(0.8, 1.0, m))


CLASSES = ("triangle", "convex", "concave", "bowtie", "pentagram", "collinear", "repeated", "beyond", "nonfinite", "at-vertex", "whole", "huge")


def seeded_polys(scene, region, seed, extra=()):
    """(polygons, class of each): every class that does not need to know the scene, over `region` = (xa, ya, xb, yb); `extra`:
    (class, polygon) pairs placed by hand."""
    from test_hit_gpu import scene_vertices_and_segments

    rng = np.random.default_rng(seed)
    xa, ya, xb, yb = region
    span = np.array([xb - xa, yb - ya])
    at = lambda n: rng.uniform(0.0, 1.0, (n, 2)) * span + (xa, ya)   # noqa: E731
    size = lambda: float(rng.uniform(0.02, 0.35) * span.min())      # noqa: E731
    out = []
    for c in at(50):
        out.append(("triangle", c + rng.uniform(-1.0, 1.0, (3, 2)) * size()))
    for c in at(28):
        out.append(("convex", ngon(c, size(), int(rng.integers(4, 13)), rng.uniform(0, 6.3))))
    for c in at(28):
        n = int(rng.integers(7, 21))
        out.append(("concave", ngon(c, size(), n, rng.uniform(0, 6.3), rng.uniform(0.25, 1.0, n))))
    for c in at(14):
        out.append(("bowtie", bowtie(c, size())))
    for c in at(14):
        out.append(("pentagram", pentagram(c, size())))
    for c in at(8):
        d = rng.uniform(-1.0, 1.0, 2) * size()
        out.append(("collinear", c + np.outer(rng.permutation(np.arange(-2, 3)), d)))       # five points of one line, shuffled
    for c in at(8):
        t = c + rng.uniform(-1.0, 1.0, (3, 2)) * size()
        out.append(("repeated", t[[0, 0, 1, 2, 2, 2, 0]]))
    big = max(span) * 2
    for k in range(8):
        c = at(1)[0]
        out.append(("beyond", np.array([[-big - 100.0 * k, c[1] - 40], [70000.0 + 1000 * k, c[1] - 10], [c[0], 66000.0 + k], [c[0] - 5, -300.0 - k]])))
    for k, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan)):
        p = box(xa, ya, xb, yb)
        p[k % 4, k % 2] = bad
        out.append(("nonfinite", p))
    verts, a, b = scene_vertices_and_segments(scene)
    verts = verts[np.isfinite(verts).all(axis=1)].astype(np.float64)
    for v in verts[:: max(len(verts) // 24, 1)][:24]:      # a vertex of K exactly on a vertex of the scene
        out.append(("at-vertex", np.array([v, v + rng.uniform(1.0, 30.0, 2), v + rng.uniform(-30.0, 30.0, 2)])))
    out.append(("whole", box(xa - 10, ya - 10, xb + 10, yb + 10)))
    out.append(("whole", box(xa - 10, ya - 10, xb + 10, yb + 10, reverse=True)))
    # vertices of 2^35 and more: D20's once-rounded orient of a long edge can be 0 where the real one is not, so that the winding sum
    # of a point OUTSIDE K's box -- left of it -- is not 0: an apex just beside the region, the two far vertices on each of the four sides
    xm, ym = (xa + xb) / 2, (ya + yb) / 2
    for k, e in enumerate((35, 45, 60, 100)):
        h = 2.0 ** e
        out.append(("huge", np.array([[h, -h], [xb + 5.0 + k, ym + k], [h, h]])))          # the region lies left of K's box
        out.append(("huge", np.array([[-h, h], [xa - 5.0 - k, ym - k], [-h, -h]])))        # right of it
        out.append(("huge", np.array([[-h, h], [xm + k, yb + 5.0 + k], [h, h]])))          # above it
        out.append(("huge", np.array([[h, -h], [xm - k, ya - 5.0 - k], [-h, -h]])))        # below it
        out.append(("huge", np.array([[h, -h], [xm + k, ym], [h, h]])))                    # the apex inside the region
        out.append(("huge", box(-h, -h, h, h, reverse=bool(k % 2))))
    out += list(extra)
    return [p.astype(F32) for _, p in out], [c for c, _ in out]


# mixed_scene (tests/test_hit_gpu.py), by its own numbers: item 0 the square [20.25, 220.25] x [30.5, 230.5]; 2 the even-odd ring
# [100.5, 250.5] x [100.25, 250.25] with the hole [140.5, 200.5] x [140.25, 200.25]; 3 the circle (160, 330), r = 45; 5 a transparent
# square [250, 370] x [40, 160]; 9 a one-point polyline at (60, 60), width 12
MIXED_EXTRA = [
    ("inside-fill", np.array([[30.0, 40.0], [50.0, 45.0], [40.0, 60.0]])),               # wholly inside item 0, no edge reached
    ("inside-fill", np.array([[25.0, 200.0], [90.0, 228.0], [30.0, 229.0], [60.0, 210.0]])),
    ("in-eo-hole", np.array([[150.0, 150.0], [190.0, 155.0], [170.0, 190.0]])),          # in item 2's hole: item 2 untouched, item 0 (under it) touched
    ("in-eo-hole", ngon((170.5, 170.25), 25.0, 9)),
    ("notch", notch(100.0, 270.0, 230.0, 390.0, 8.0)),                                     # item 3, the circle, sits in the notch
    ("notch", notch(40.0, 40.0, 90.0, 80.0, 5.0)),                                         # item 9, the point stroke (hw = 6)
    ("pentagram", pentagram((60.0, 60.0), 60.0)),                                          # item 9 in the centre, where the rules differ
    ("pentagram", pentagram((62.0, 58.0), 45.0)),
    ("pentagram", pentagram((160.0, 330.0), 200.0)),                                       # item 3
    ("item-in-hole", pentagram((160.0, 330.0), 400.0)),                                    # item 3 in the pentagram's centre
    ("item-in-hole", holed((90.0, 260.0, 240.0, 400.0), (110.0, 280.0, 210.0, 380.0))),    # item 3 in a hole of winding 0
]
# edge_scene: item 0 the fill [-40, 60] x [-30, 50], item 1 the fill [65000, 70500] x [-5, 40]
EDGE_EXTRA = [
    ("inside-fill", np.array([[-30.0, -20.0], [-25.0, -15.0], [-35.0, -10.0]])),
    ("inside-fill", np.array([[66000.0, 0.0], [67000.0, 30.0], [66500.0, 5.0]])),
    ("beyond", box(-60.0, -50.0, 71000.0, 200.0)),
    ("beyond", box(64990.0, -20.0, 70600.0, 120.0)),
]

def loose_scene(pm):
    """Items whose outline is not one connected finite line, so that "some point inside", "every point inside" and "reaches the
    boundary" come apart: 0 a compound Fill of two squares far from each other, [20, 40]^2 and [200, 220] x [20, 40]; 1 a Polyline
    whose LAST point is NaN; 2 a Polyline whose first point is +inf; 3 a plain Fill with a NaN point; 4 a Line whose second end is
    NaN; 5 a compound Fill of a square and a far single point."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)  # noqa: E731

    def emit(e):
        e.fill_compound([sq(20, 20, 40, 40), sq(200, 20, 220, 40)], 0x336699FF)
        e.polyline(np.array([[20.0, 80.0], [50.0, 90.0], [80.0, 80.0], [np.nan, 85.0]]), 0x11AA22FF, 2.0)
        e.polyline(np.array([[np.inf, 130.0], [60.0, 130.0], [90.0, 140.0]]), 0x11AA22FF, 2.0)
        e.fill(np.array([[120.0, 80.0], [160.0, 80.0], [np.nan, 100.0], [160.0, 120.0], [120.0, 120.0]]), 0x884400FF)
        e.stroke_line((150.0, 150.0), (np.nan, 150.0), 3.0, 0x000000FF)
        e.fill_compound([sq(20, 180, 60, 220), np.array([[300.0, 200.0]])], 0xAA5500FF)

    return hs._encode(pm, 6, emit)


LOOSE_EXTRA = [
    ("loose", box(10.0, 10.0, 50.0, 50.0)),         # around item 0's first square only: some point inside, not every one, no edge reached
    ("loose", box(10.0, 10.0, 230.0, 50.0)),        # around both
    ("loose", box(10.0, 70.0, 100.0, 100.0)),       # around item 1's finite points: its NaN point keeps it from being enclosed
    ("loose", box(40.0, 120.0, 100.0, 150.0)),      # around item 2's finite points
    ("loose", box(110.0, 70.0, 170.0, 130.0)),      # around item 3's
    ("loose", box(140.0, 140.0, 160.0, 160.0)),     # around item 4's finite end
    ("loose", box(10.0, 170.0, 70.0, 230.0)),       # around item 5's square, not its far point
    ("loose", box(10.0, 170.0, 310.0, 230.0)),      # ... and around both
]

_small = {}
SMALL = rc.SMALL + ("loose",)


def small_case(pm, pmo, name):
    if name not in _small:
        if name == "loose":
            scene = loose_scene(pm)
            polys, cls = seeded_polys(scene, (0, 0, 320, 240), 66, LOOSE_EXTRA)
            _small[name] = PolyCase(name, scene, polys[::3] + polys[-len(LOOSE_EXTRA):], classes=cls[::3] + cls[-len(LOOSE_EXTRA):])
            return _small[name]
        base = rc.small_case(pm, pmo, name)      # (the scene is rect_cases')
        if name == "mixed":
            polys, cls = seeded_polys(base.scene, (-20, -20, 540, 540), 61, MIXED_EXTRA)
        elif name == "edge":
            polys, cls = seeded_polys(base.scene, (-80, -60, 120, 140), 62, EDGE_EXTRA)
            far, fcls = seeded_polys(base.scene, (64900, -40, 65700, 140), 63)
            polys, cls = polys + far[:80], cls + fcls[:80]
        elif name == "nonfinite":
            polys, cls = seeded_polys(base.scene, (-60, -20, 260, 260), 65)
        else:
            polys, cls = seeded_polys(base.scene, rc._region_of(base.scene), 64)
        _small[name] = PolyCase(name, base.scene, polys, classes=cls)
    return _small[name]


# ---- distances that rounding decides -------------------------------------------------------------------------------------------

def origin_case(pm):
    """Strokes with a point within hw of (0, 0), all of them left of x = 70, under triangles (H, -H), apex, (H, H) with H = 2^60 and
    2^100 and the apex at x >= 100.  In D20's arithmetic the apex is lost in `apex - c`, t rounds to 1 and the closest point of the long
    edge to c + (-c) = (0, 0): the computed distance of a stroke's point to that edge is its distance to the ORIGIN, and a stroke
    tens of pixels away from K's box is near K.  0: a Line from (1, 1), hw = 2; 1: a Polyline through (1, -1), hw = 3; 2: a Line from
    (3, 3), hw = 2, too far from the origin for that; 3: a Fill around the origin (its answers there come from rounded windings)."""
    def emit(e):
        e.stroke_line((1.0, 1.0), (40.0, 30.0), 4.0, 0x000000FF)
        e.polyline(np.array([[50.0, 50.0], [1.0, -1.0], [60.0, 0.0]]), 0x11AA22FF, 6.0)
        e.stroke_line((3.0, 3.0), (40.0, 60.0), 4.0, 0x000000FF)
        e.fill(np.array([[-5.0, -5.0], [5.0, -5.0], [5.0, 5.0], [-5.0, 5.0]]), 0x336699FF)

    polys = []
    for e in (60, 100):
        h = 2.0 ** e
        for apex in ((100.0, 20.0), (150.0, -40.0), (500.0, 300.0), (101.0, 0.0)):
            polys.append(np.array([[h, -h], apex, [h, h]]))
            polys.append(np.array([[h, h], apex, [h, -h]]))
    return PolyCase("origin", hs._encode(pm, 4, emit), polys)


# ---- the item walk -----------------------------------------------------------------------------------------------------

_walks = {}


def walk_case(pm, n):
    """hit_frame_cases.walk_scene of n items.  Polygons: a box around the whole scene, either way round; a lasso of 40 vertices around
    it; a triangle over its lower left half; the cell of one item, a triangle in the empty corner of another; a pentagram over the
    scene; one far away."""
    if n not in _walks:
        wdw = fc.walk_scene(pm, n)
        x0, y0, w, h = wdw.rect
        c = (x0 + w / 2, y0 + h / 2)
        cx, cy = fc.walk_cell(7)
        ex, ey = fc.walk_cell(3)
        polys = [box(x0 - 2, y0 - 2, x0 + w + 2, y0 + h + 2), box(x0 - 2, y0 - 2, x0 + w + 2, y0 + h + 2, reverse=True), lasso(c, max(w, h), 40, n),
                 np.array([[x0 - 2, y0 - 2], [x0 - 2, y0 + h + 2], [x0 + w + 2, y0 + h + 2]]), box(cx, cy, cx + fc.CELL, cy + fc.CELL),
                 np.array([[ex + 0.2, ey + 0.2], [ex + 0.3, ey + 0.2], [ex + 0.2, ey + 0.3]]), pentagram(c, max(w, h)),
                 box(x0 + w + 50, y0, x0 + w + 60, y0 + 5)]
        _walks[n] = PolyCase(f"walk-{n}", wdw.scene, polys, n=n)
    return _walks[n]


# ---- long items --------------------------------------------------------------------------------------------------------

LONG_IDS = rc.LONG_IDS
_longs = {}


def long_case(pm, ident):
    """rect_cases.long_case's scene: a long Fill or Polyline (item 1) between a lead and a trailing item.  Polygons 0, 1: a small
    triangle across the middle of one segment of the last chunk and of chunk min(64, chunks - 1); 2: a triangle that reaches nothing;
    3 (Fills): a triangle inside the band, reaching no edge -- the Fill's winding around v_0 alone decides; 4: an 8-gon around the
    whole item (every point inside); 5: the same, but for a wedge that takes the item's LAST point out of it."""
    if ident not in _longs:
        base = rc.long_case(pm, ident)
        kind, chunks = base.facts["kind"], base.facts["chunks"]
        sc = bytes(base.scene)
        ent, a, b, nent = hs._entries(sc, np_hit.flat_items(sc)[rc.LONG_ITEM][0])
        polys = []
        for s in base.facts["segs"]:
            mid = (a[s] + b[s]) * 0.5
            d = (b[s] - a[s]) / np.linalg.norm(b[s] - a[s])
            nrm = np.array([-d[1], d[0]])
            polys.append(np.array([mid - 0.3 * nrm - 0.02 * d, mid + 0.3 * nrm - 0.02 * d, mid + 0.3 * nrm + 0.05 * d]))
        xm = 10.0 + rc.PITCH * (2 * (chunks // 2) + 1)
        polys.append(np.array([[xm - 0.1, 95.0], [xm + 0.1, 95.0], [xm, 99.0]]) if kind != "polyline" else np.array([[xm - 0.2, 120.0], [xm + 0.2, 120.0], [xm, 121.0]]))
        polys.append(np.array([[xm - 3.0, 112.0], [xm + 3.0, 113.0], [xm, 124.0]]) if kind != "polyline" else np.array([[xm - 0.2, 130.0], [xm + 0.2, 130.0], [xm, 131.0]]))
        pts = rc.long_points(kind, chunks)
        lo, hi = pts.min(axis=0) - 4.0, pts.max(axis=0) + 4.0
        around = np.array([[lo[0], lo[1]], [(lo[0] + hi[0]) / 2, lo[1] - 1], [hi[0], lo[1]], [hi[0] + 1, (lo[1] + hi[1]) / 2], [hi[0], hi[1]],
                           [(lo[0] + hi[0]) / 2, hi[1] + 1], [lo[0], hi[1]], [lo[0] - 1, (lo[1] + hi[1]) / 2]])
        polys.append(around)
        # ... with a thin wedge cut in from the nearest side (the left: a Fill's last point; the right: a Polyline's) to just past the item's
        # last point: the outline runs on from that point into K, so the wedge is crossed by a segment of the LAST chunk
        last = pts[-1]
        if kind != "polyline":
            cut = np.concatenate([around[:7], [[lo[0] - 1, last[1] + 0.3], last + (0.4, 0.0), [lo[0] - 1, last[1] - 0.3]]])
        else:
            cut = np.concatenate([around[:3], [[hi[0] + 1, last[1] - 0.3], last - (0.4, 0.0), [hi[0] + 1, last[1] + 0.3]], around[4:]])
        polys.append(cut)
        _longs[ident] = PolyCase(ident, base.scene, polys, kind=kind, chunks=chunks, segs=base.facts["segs"])
    return _longs[ident]


# ---- polygon sizes -----------------------------------------------------------------------------------------------------

_sizes = {}


def size_case(pm, pmo):
    """mixed_scene under lassos of every size in M_SIZES: radius 140 around the even-odd ring (item 2) -- it encloses the ring and cuts
    through its neighbours -- and radius 600, around everything; and a pentagram traced with m vertices, item 9 in its centre (where
    the two rules differ)."""
    if "c" not in _sizes:
        scene = rc.small_case(pm, pmo, "mixed").scene
        polys = []
        for m in M_SIZES:
            polys.append(lasso((170.5, 170.25), 140.0, m, m))
            polys.append(lasso((260.0, 250.0), 600.0, m, m + 1))
            if m >= 5:   # a pentagram, its edges cut into m pieces in all
                p = pentagram((60.0, 60.0), 100.0)
                k = np.arange(m) * 5.0 / m
                j = k.astype(int)
                polys.append(p[j] + (p[(j + 1) % 5] - p[j]) * (k - j)[:, None])
        _sizes["c"] = PolyCase("sizes", scene, polys)
    return _sizes["c"]


# ---- rectangles as 4-gons, on integer coordinates ----------------------------------------------------------------------------

def int_scene(pm):
    """Integer coordinates below 256 and widths / radii that are small integers: every product of D19 and D20 is exact.  Fills
    (plain, a ring under each rule, a triangle), Circles and ellipses, a Line and Polylines."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)  # noqa: E731

    def emit(e):
        e.fill(sq(20, 20, 60, 50), 0x336699FF)
        e.fill_compound([sq(80, 20, 140, 80), sq(100, 40, 120, 60)], 0xAA5500FF, even_odd=True)
        e.fill(np.array([[30.0, 90.0], [70.0, 100.0], [40.0, 140.0]]), 0x884400FF)
        e.circle((170.0, 40.0), 12.0)
        e.ellipse((180.0, 100.0), 24.0, 10.0)
        e.stroke_line((20.0, 170.0), (90.0, 200.0), 4.0, 0x000000FF)
        e.polyline(np.array([[110.0, 150.0], [150.0, 190.0], [200.0, 160.0], [230.0, 210.0]]), 0x11AA22FF, 6.0)
        e.fill_compound([sq(100, 100, 150, 140), sq(110, 110, 130, 130)[::-1]], 0x2244CCFF)
        e.circle((60.0, 230.0), 5.0)
        e.polyline(np.array([[200.0, 20.0], [240.0, 20.0], [240.0, 70.0]]), 0x445566FF, 2.0)

    return hs._encode(pm, 10, emit)


def _int_rects():
    rng = np.random.default_rng(71)
    c = rng.integers(0, 230, (70, 2))
    r = np.concatenate([c, c + rng.integers(0, 120, (70, 2))], axis=1)      # (zero-size ones among them)
    hand = [[20, 20, 60, 50], [19, 19, 61, 51], [0, 0, 255, 255], [60, 50, 80, 60], [100, 40, 120, 60], [101, 41, 119, 59], [158, 28, 182, 52], [157, 27, 183, 53],
            [60, 20, 60, 50], [40, 30, 40, 30], [156, 90, 204, 110], [155, 89, 205, 111], [197, 17, 243, 73], [0, 0, 10, 10],
            [15, 15, 65, 55], [75, 15, 145, 85], [25, 85, 75, 145], [150, 20, 190, 60], [150, 85, 210, 115], [95, 95, 155, 145], [50, 220, 70, 240], [10, 10, 150, 150],
            [0, 0, 200, 120], [90, 90, 240, 220]]
    return np.concatenate([r, hand]).astype(F32)


INT_RECTS = _int_rects()


def rotated_rect_corners(cx, cy, w, h, angle):
    """float32 (4, 2): the corners (-w/2, -h/2), (+w/2, -h/2), (+w/2, +h/2), (-w/2, +h/2) of a w x h rectangle, each turned by `angle`
    radians about the centre (from +x towards +y), moved to (cx, cy) in binary64 and rounded to f32 once, in this order."""
    c, s = np.cos(np.float64(angle)), np.sin(np.float64(angle))
    hx, hy = 0.5 * np.float64(w), 0.5 * np.float64(h)
    local = np.array([[-hx, -hy], [hx, -hy], [hx, hy], [-hx, hy]], np.float64)
    return np.stack([np.float64(cx) + (local[:, 0] * c - local[:, 1] * s), np.float64(cy) + (local[:, 0] * s + local[:, 1] * c)], axis=1).astype(F32)


def rect_as_polygon(rect, reverse=False):
    return box(*[float(v) for v in rect], reverse=reverse).astype(F32)


# ---- hand-derived answers (rect_cases.known_scene) ---------------------------------------------------------------------------

up = rc.up
T, E = np_poly.TOUCHES, np_poly.TOUCHES | np_poly.ENCLOSES
# (polygon, even_odd, item, PM_SEL_* of that item) -- each worked out by hand.  known_scene: 0 the Fill [10, 20]^2; 1 a Polyline
# (30, 10) -> (50, 10), hw = 1; 2 a Circle (70, 15), r = 5; 3 an even-odd ring [10, 40] x [40, 70] with the hole [20, 30] x [50, 60];
# 4 a Line (60, 40) -> (60, 60), hw = 2; 5 an ellipse (90, 50), 10 x 5; 8 an ellipse with ry = 0: no geometry
KNOWN = [
    # K's vertex v_0 = (20, 20) IS the Fill's vertex: for the Fill's edge (20, 10) -> (20, 20) and K's edge (20, 20) -> (25, 20) the
    # extents meet in that point, s1 = orient(a, b, v_0) = 0 and s4 = orient(c, d, b) = 0: neither pair has one sign -- it crosses
    ([[20, 20], [25, 20], [25, 25]], False, 0, T),
    # one f32 step to the right: every edge of K has min x > 20 = the Fill's max x: no crossing; no point of the Fill is in K; v_0
    # is right of every edge of the Fill, where s <= 0 on the rising edge x = 20: winding 0
    ([[up(20), 10], [25, 10], [25, 20]], False, 0, 0),
    # K inside the Fill: no edge reached (the Fill's four edges have all of K on one side), no corner of the Fill in K; the Fill's
    # winding around v_0 = (12, 12) is 1: touched by that term alone
    ([[12, 12], [18, 13], [15, 18]], False, 0, T),
    # K strictly around the Fill: the extents of K's edges and the Fill's never meet (9 < 10, 21 > 20), every corner has winding 1
    ([[9, 9], [21, 9], [21, 21], [9, 21]], False, 0, E),
    # K IS the Fill's outline: every edge lies on an edge of K, all four orients are 0: it reaches the boundary -- touched, NOT enclosed
    ([[10, 10], [20, 10], [20, 20], [10, 20]], False, 0, T),
    # the Polyline along y = 10, hw = 1: K's edge along y = 11 is at distance exactly hw (its end (35, 11): dx = 0, dy = 1, 1 <= 1)
    ([[35, 11], [40, 11], [40, 12], [35, 12]], False, 1, T),
    ([[35, up(11)], [40, up(11)], [40, 12], [35, 12]], False, 1, 0),     # a step further: 1.0000001^2 > 1, and no point of it in K
    # around it at distance 2 > hw: no crossing, every distance >= 2, both points have winding 1 -- enclosed; at distance exactly
    # hw = 1 the outline reaches the boundary: touched, not enclosed
    ([[28, 8], [52, 8], [52, 12], [28, 12]], False, 1, E),
    ([[29, 9], [51, 9], [51, 11], [29, 11]], False, 1, T),
    # the Circle (70, 15), r = 5: K's vertex (73, 19) is at (3, 4) from the centre: 9 + 16 = 25 <= r * r; from (74, 19): 16 + 16 > 25
    # (the clamped projection of the centre on each edge from that vertex is the vertex itself)
    ([[73, 19], [80, 19], [80, 25]], False, 2, T),
    ([[74, 19], [80, 19], [80, 25]], False, 2, 0),
    # around it: edges at distance 6 > 5, the centre has winding 1 -- enclosed; at distance exactly 5: reaches, not enclosed
    ([[64, 9], [76, 9], [76, 21], [64, 21]], False, 2, E),
    ([[65, 10], [75, 10], [75, 20], [65, 20]], False, 2, T),
    # K in the even-odd ring's hole: no edge reached, no point of the ring in K, the ring's winding around v_0 = (22, 52) is 2: even
    ([[22, 52], [28, 52], [25, 58]], False, 3, 0),
    # the ring around a hole of K: K is the box [0, 50] x [30, 80] with the hole [23, 27] x [53, 57] run the other way round.  A
    # polygon is ONE closed line: the hole hangs on the bridge (0, 30) <-> (23, 53), which runs through the ring's corners (10, 40)
    # and (20, 50) -- the ring's outline reaches K's boundary there: touched, not enclosed, under either rule
    (np.concatenate([box(0, 30, 50, 80), [[0, 30]], box(23, 53, 27, 57, True), [[23, 53]]]).tolist(), False, 3, T),
    (np.concatenate([box(0, 30, 50, 80), [[0, 30]], box(23, 53, 27, 57, True), [[23, 53]]]).tolist(), True, 3, T),
    # the Line at x = 60 from y = 40 to 60, hw = 2, in the centre of a pentagram of radius 60 around (60, 50): the centre pentagon
    # reaches 60 cos(72 deg) / cos(36 deg) = 22.9 > 12 from the centre, so the Line is far from every edge; winding 2 there:
    # enclosed by the non-zero rule, not even touched by even-odd
    (pentagram((60.0, 50.0), 60.0).tolist(), False, 4, E),
    (pentagram((60.0, 50.0), 60.0).tolist(), True, 4, 0),
    # the ellipse (90, 50), 10 x 5: K's vertical edge at x = 100 maps to u = 1: distance 1 <= 1 from (0, 0); at up(100): > 1
    ([[100, 45], [105, 45], [105, 55], [100, 55]], False, 5, T),
    ([[up(100), 45], [105, 45], [105, 55], [up(100), 55]], False, 5, 0),
    # the ellipse with ry = 0 has no geometry: nothing touches or encloses it
    ([[0, 0], [200, 0], [200, 200], [0, 200]], False, 8, 0),
]
