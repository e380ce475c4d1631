"""Polygon queries, pm_select_polygon and its device variant (decision D20): which items a query polygon touches, which
it encloses -- lasso selection, and a marquee in a rotated view.  The bar is item_flags EQUAL to tests/np_poly.py, the numpy
restatement of D20, with no tolerance and no polygon left out, through the host and the device call, with and without the skip
flag, under both rules.

  -m gpu   the cases of tests/poly_cases.py (small scenes under ~200 seeded polygons of every class, the item walk, long items,
           polygon sizes), rectangles as 4-gons against select_rect, select_rotated_rect, hand-derived answers, output discipline
           and argument rules, back-to-back device calls, ordering against scene replacement and frames, the CLI;
  CPU      the cases are what they claim (numpy alone); the hand-derived answers hold in numpy; D20 against D13 on grids of points
           and against D19 on integer coordinates; the -m gpu part under the wave64 emulation; the compiler's listing."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hit_structure as hs  # noqa: E402
import np_hit  # noqa: E402
import np_poly  # noqa: E402
import np_rect  # noqa: E402
import poly_cases as pc  # noqa: E402
import rect_cases as rc  # noqa: E402

T, E = np_poly.TOUCHES, np_poly.ENCLOSES
UNTOUCHED = 0x7EADBEEF
# small scenes, walk, long, sizes, rounded distances, 4-gons, rotated marquee, known answers, output discipline and arguments, back to back, ordering (2), CLI
N_GPU_TESTS = len(pc.SMALL) + len(rc.WALK_SIZES) + len(pc.LONG_IDS) + 1 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1


# ---- helpers -------------------------------------------------------------------------------------------

def _kinds(scene):
    sc = bytes(scene)
    return np.array([np.frombuffer(sc, np.uint32, 1, at)[0] & 0xFFFF for at, _ in np_hit.flat_items(sc)])


def _item_points(scene):
    """Per item: float64 [n, 2] points (a Circle: the four extreme points of its box, which is what D19 asks of it)."""
    sc = bytes(scene)
    out = []
    for at, bbox in np_hit.flat_items(sc):
        tag = np.frombuffer(sc, np.uint32, 1, at)[0] & 0xFFFF
        if tag == np_hit.FILL:
            p = np_hit._points(sc, at).astype(np.float64)
            out.append(p[~np.isnan(p[:, 0])])
        elif tag in (np_hit.LINE, np_hit.POLY):
            a, b, _ = np_hit.stroke_segments(sc, at, tag)
            out.append(np.concatenate([a[:1], b]))
        else:
            x0, y0, x1, y1 = (float(v) for v in bbox)
            out.append(np.array([[x0, (y0 + y1) / 2], [x1, (y0 + y1) / 2], [(x0 + x1) / 2, y0], [(x0 + x1) / 2, y1]]))
    return out


def _points_on_boundary(scene, rects):
    """bool [n_items, n_rects]: some point of the item (a Circle: of its box) lies on the rectangle's boundary lines."""
    pts = _item_points(scene)
    r = np.asarray(rects, np.float64)
    out = np.zeros((len(pts), len(r)), bool)
    for i, p in enumerate(pts):
        on_x = (p[:, None, 0] == r[None, :, 0]) | (p[:, None, 0] == r[None, :, 2])
        on_y = (p[:, None, 1] == r[None, :, 1]) | (p[:, None, 1] == r[None, :, 3])
        out[i] = (on_x | on_y).any(axis=0)
    return out


def _diagonal_scene(pm):
    def emit(e):
        for k in range(9):
            c = 20.0 + 20.0 * k
            e.fill(np.array([[c - 3, c - 3], [c + 3, c - 3], [c + 3, c + 3], [c - 3, c + 3]]), 0x336699FF)
        e.fill(np.array([[170.0, 20.0], [180.0, 20.0], [180.0, 30.0], [170.0, 30.0]]), 0x884400FF)

    return hs._encode(pm, 10, emit), (100.0, 100.0, 260.0, 16.0, float(np.pi / 4))


# ---- CPU: the cases are what they claim (numpy alone) -------------------------------------------------------------------------

def test_the_small_cases_have_every_class(pm, pmo):
    mixed = pc.small_case(pm, pmo, "mixed")
    cls = np.array(mixed.facts["classes"])
    nz, eo = mixed.table(), mixed.table(even_odd=True)
    for c, floor in (("triangle", 30), ("convex", 20), ("concave", 20), ("bowtie", 10), ("pentagram", 10), ("collinear", 8), ("repeated", 8), ("beyond", 8),
                     ("nonfinite", 6), ("at-vertex", 20), ("whole", 2), ("huge", 24), ("inside-fill", 2), ("in-eo-hole", 2), ("notch", 2), ("item-in-hole", 2)):
        assert (cls == c).sum() >= floor, c
    assert len(mixed.polys) >= 190
    sc = bytes(mixed.scene)
    K = lambda k, eo_=False: np_poly.Polygon(mixed.polys[k], eo_)   # noqa: E731
    seg = lambda i: np_hit.fill_segments(np_hit._points(sc, np_hit.flat_items(sc)[i][0]), True if i == 2 else False)  # noqa: E731
    for k in np.flatnonzero(cls == "inside-fill"):       # inside item 0: touched by the winding of v_0 alone
        a, b = seg(0)
        assert nz[0, k] == T and not np_poly.crosses(K(k), a, b).any() and not np_poly.in_k(K(k), a).any()
    for k in np.flatnonzero(cls == "in-eo-hole"):        # in the even-odd ring's hole: the ring is not touched, the square under it is
        assert nz[2, k] == 0 and nz[0, k] == T
    boxes = np.array([b for _, b in np_hit.flat_items(sc)], np.float64)
    for k, item in zip(np.flatnonzero(cls == "notch"), (3, 9)):         # the item sits in the notch: inside K's box, not touched
        p = mixed.polys[k]
        assert (boxes[item, 0] >= p[:, 0].min()) and (boxes[item, 2] <= p[:, 0].max()) and (boxes[item, 1] >= p[:, 1].min()) and (boxes[item, 3] <= p[:, 1].max())
        assert nz[item, k] == 0 and eo[item, k] == 0
    k_pent, k_holed = np.flatnonzero(cls == "item-in-hole")
    assert nz[3, k_pent] == (T | E) and eo[3, k_pent] == 0      # the pentagram's centre: winding 2
    assert nz[3, k_holed] == 0 and eo[3, k_holed] == 0          # a hole of winding 0 is one under both rules
    differ = (nz != eo).any(axis=0)
    assert differ[cls == "pentagram"].sum() >= 3 and differ[cls == "bowtie"].sum() == 0 and (nz[:, cls == "bowtie"] != 0).any()
    assert (nz[:, cls == "nonfinite"] == 0).all() and (nz[:, cls == "collinear"] & E == 0).all() and (nz[:, cls == "collinear"] & T).any()
    assert (nz[:, cls == "repeated"] != 0).any() and (nz[:, cls == "beyond"] & T).any() and (nz[:, cls == "at-vertex"] & T).any(axis=0).sum() >= 20
    # huge vertices: items that lie wholly LEFT of K's box and are touched all the same (a rounded orient of 0), which no cull by
    # K's box on that side survives; and the boxes of 2^35 .. 2^100 enclose everything that has geometry
    left_of_k = boxes[:, None, 2] < np.array([p[:, 0].min() for p in mixed.polys], np.float64)[None, :]
    assert ((nz != 0) & left_of_k)[:, cls == "huge"].sum() >= 8 and ((nz != 0) & left_of_k)[:, cls != "huge"].sum() == 0
    assert (nz[:10, cls == "huge"] == (T | E)).all(axis=0).sum() >= 4
    whole = np.flatnonzero(cls == "whole")
    assert np.array_equal(nz[:, whole[0]], nz[:, whole[1]]) and (nz[:10, whole[0]] == (T | E)).all() and nz[10, whole[0]] == 0    # (item 10 has no geometry)
    skipped = mixed.table(skip=True)
    assert (skipped[5] == 0).all() and (nz[5] != 0).any() and np.array_equal(np.delete(skipped, 5, axis=0), np.delete(nz, 5, axis=0))
    assert ((nz & E) != 0).any(axis=1).sum() >= 8 and ((nz & E) != 0).sum() < ((nz & T) != 0).sum()
    edge = pc.small_case(pm, pmo, "edge")
    fe = edge.table()
    ecls = np.array(edge.facts["classes"])
    assert (fe[1, ecls == "beyond"] & T).any() and (fe[0] & E).any() and (fe[3] & T).any() and (fe[1] == (T | E)).any() and len(edge.polys) >= 200
    assert [int(fe[i, np.flatnonzero(ecls == "inside-fill")[i]]) for i in (0, 1)] == [T, T]
    loose = pc.small_case(pm, pmo, "loose")
    fl = loose.table()[:, -len(pc.LOOSE_EXTRA):]
    # some point inside, not every one, no edge reached; both squares; a non-finite point keeps an item from being enclosed
    assert [int(v) for v in (fl[0, 0], fl[0, 1], fl[1, 2], fl[2, 3], fl[3, 4], fl[4, 5], fl[5, 6], fl[5, 7])] == [T, T | E, T, T, T, T, T, T | E]
    for name in ("path_test", "nonfinite"):
        case = pc.small_case(pm, pmo, name)
        f = case.table()
        # (every item of the non-finite scene has a non-finite point, or no geometry: nothing encloses any)
        assert len(case.polys) >= 160 and (f & T).any() and (f & E).any() == (name == "path_test") and (f == 0).any()


@pytest.mark.parametrize("n", rc.WALK_SIZES)
def test_the_walk_cases_are_what_they_claim(pm, n):
    case = pc.walk_case(pm, n)
    f = case.table()
    assert f.shape[0] == n and (f[:, 0] == (T | E)).all() and (f[:, 1] == (T | E)).all()      # the whole scene, either way round
    assert (f[:, 2] == (T | E)).all()                                                         # ... and the lasso around it
    assert 0 < ((f[:, 3] & E) != 0).sum() < n and (f[0, 3] & T)                               # the triangle: half of it
    assert (f[7, 4] & T) and ((f[:, 4] & E) != 0).sum() <= 2                                  # one cell
    assert np.flatnonzero(f[:, 5]).tolist() == [0]                                            # the empty corner: the bottom item alone
    assert (f[:, 7] == 0).all()
    assert not np.array_equal(f[:, 6], case.table(even_odd=True)[:, 6])                       # the pentagram's centre


@pytest.mark.parametrize("ident", pc.LONG_IDS)
def test_the_long_cases_are_decided_where_they_claim(pm, ident):
    """The segments that reach polygons 0 and 1 lie in the chunk named, and in no other; polygon 2 reaches none and holds no point; a
    Fill's polygon 3 reaches none, holds none and is inside by the winding of v_0; 4 encloses the item; 5 is reached by segments of
    the last chunk (and, a Fill, by the closing segment's neighbour) and holds every point but the last."""
    case = pc.long_case(pm, ident)
    sc = bytes(case.scene)
    at = np_hit.flat_items(sc)[rc.LONG_ITEM][0]
    ent, a, b, _ = hs._entries(sc, at)
    fill = case.facts["kind"] != "polyline"
    chunks = case.facts["chunks"]
    pts = np_hit._points(sc, at).astype(np.float64)
    reach, inside = [], []
    for k, p in enumerate(case.polys):
        K = np_poly.Polygon(p)
        r_ = np_poly.crosses(K, a, b).any(axis=1)
        if not fill:
            r_ |= np_poly.near(K, a, b, np.float64(0.25)).any(axis=1)
        reach.append(np.flatnonzero(r_))
        inside.append(np_poly.in_k(K, pts))
    for k, s in enumerate(case.facts["segs"]):
        assert reach[k].tolist() == [s], (ident, k)
    assert case.facts["segs"][0] // 4 == chunks - 1 and case.facts["segs"][1] // 4 == min(64, chunks - 1)
    assert len(reach[2]) == 0 and len(reach[3]) == 0 and len(reach[4]) == 0 and not inside[2].any() and not inside[3].any() and inside[4].all()
    assert len(reach[5]) > 0 and (reach[5] // 4 >= chunks - 1).all() and inside[5][:-1].all() and not inside[5][-1]
    f = [int(case.flags(k)[rc.LONG_ITEM]) for k in range(6)]
    assert f == [T, T, 0, T if fill else 0, T | E, T]
    assert int(case.flags(4)[0]) == 0 and int(case.flags(4)[2]) == 0       # the lead and the trailing item are outside


def test_the_size_case_has_every_size(pm, pmo):
    case = pc.size_case(pm, pmo)
    sizes = sorted({len(p) for p in case.polys})
    assert sizes == sorted(pc.M_SIZES)
    nz, eo = case.table(), case.table(even_odd=True)
    for k, p in enumerate(case.polys):
        assert (nz[:, k] & T).any()
    through = [k for k, p in enumerate(case.polys) if 0 < ((nz[:, k] & E) != 0).sum() < ((nz[:, k] & T) != 0).sum()]
    assert len(through) >= len(pc.M_SIZES) - 1                                # the lassos around item 2: some enclosed, more touched
    assert sum(int((nz[:, k] == (T | E))[:10].all()) for k in range(len(case.polys))) >= len(pc.M_SIZES) - 1   # those around everything
    assert (nz != eo).any(axis=0).sum() >= len(pc.M_SIZES) - 2                # the pentagrams


def test_the_origin_case_is_decided_by_rounding(pm):
    """Every polygon's box begins at x >= 100 and every stroke ends left of x = 70, and still the strokes that come within hw of (0, 0)
    are touched -- at 2^100 under every polygon (at 2^60 the apex is not lost yet and nothing is touched)."""
    case = pc.origin_case(pm)
    f = case.table()
    assert all(p[:, 0].min() >= 100.0 for p in case.polys)
    assert (f[:2, len(case.polys) // 2:] == T).all() and (f[:2] == T).sum() >= len(case.polys) and (f[:, :len(case.polys) // 2] == 0).all()
    assert np.array_equal(f, case.table(even_odd=True))


def test_hand_derived_answers_by_numpy(pm):
    scene = rc.known_scene(pm)
    got = [int(np_poly.item_flags(scene, poly, even_odd=eo)[item]) for poly, eo, item, _ in pc.KNOWN]
    assert got == [want for *_, want in pc.KNOWN], [(pc.KNOWN[k][0], pc.KNOWN[k][2], g, pc.KNOWN[k][3]) for k, g in enumerate(got) if g != pc.KNOWN[k][3]]
    assert len(pc.KNOWN) >= 12


def test_the_rotated_marquee_case_by_numpy(pm):
    scene, marquee = _diagonal_scene(pm)
    corners = pc.rotated_rect_corners(*marquee)
    assert corners.dtype == np.float32 and corners.shape == (4, 2)
    f = np_poly.item_flags(scene, corners)
    assert (f[:9] == (T | E)).all() and f[9] == 0
    side = float(np.sqrt(marquee[2] * marquee[3]))
    best = max(int(((np_rect.item_flags(scene, [[x0, x0, x0 + side, x0 + side]])[:9, 0] & E) != 0).sum()) for x0 in np.arange(0.0, 200.0 - side, 7.0))
    assert 1 <= best <= 3 and (np_rect.item_flags(scene, [[0, 0, 200, 200]])[:, 0] == (T | E)).all()


# ---- CPU: D20 is the right definition (np_poly against np_hit and np_rect, no kernel) ------------------------------------------

WITNESS_SEEDS = (51, 52, 53)


@pytest.mark.parametrize("seed", WITNESS_SEEDS)
def test_d20_agrees_with_d13_on_grids_of_points(pm, seed):
    """Conditions on the restatement, not on a kernel, with no exception, on test_hit_rect's witness scenes under 300 polygons each
    (triangles, convex and concave polygons, bow-ties and pentagrams, under the non-zero rule and, every third, even-odd): every item
    that contains (D13, np_hit) a point p of a 24 x 24 grid over K's box with inK(p) is touched; an enclosed item contains no grid
    point p with inK(p) false that is farther than 1e-6 px from every edge of K."""
    from test_hit_rect import _witness_scene

    scene = _witness_scene(pm, seed)
    polys, cls = pc.seeded_polys(scene, (-20, -20, 300, 300), seed + 2000)
    polys = [p for p, c in zip(polys, cls) if c in ("triangle", "convex", "concave", "bowtie", "pentagram", "at-vertex")]
    rng = np.random.default_rng(seed + 3000)
    while len(polys) < 300:
        c = rng.uniform(0, 280, 2)
        n = int(rng.integers(3, 14))
        polys.append(pc.ngon(c, rng.uniform(10, 120), n, rng.uniform(0, 6.3), rng.uniform(0.3, 1.0, n)).astype(np.float32))
    n_items = len(np_hit.flat_items(bytes(scene)))
    n_in = n_touched = n_enclosed = n_out_checked = 0
    for k, p in enumerate(polys):
        even_odd = k % 3 == 2
        f = np_poly.item_flags(scene, p, even_odd=even_odd)
        K = np_poly.Polygon(p, even_odd)
        lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
        gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 24), np.linspace(lo[1], hi[1], 24))
        g = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)
        ink = np_poly.in_k(K, g.astype(np.float64))
        d2 = np.min([_dist2(K.c[j], K.d[j], g.astype(np.float64)) for j in range(K.m)], axis=0)
        clear_out = ~ink & (d2 > 1e-12)
        for i in range(n_items):
            contains = np_hit.item_inside(scene, i, g)
            if (contains & ink).any():
                n_in += 1
                assert f[i] & T, (seed, k, i)
            if f[i] & E:
                n_enclosed += 1
                n_out_checked += int(clear_out.sum())
                assert not (contains & clear_out).any(), (seed, k, i)
                assert f[i] & T
        n_touched += int(((f & T) != 0).sum())
    print(f"seed {seed}: {n_in} pairs with a grid point of K inside the item, {n_touched} touched, {n_enclosed} enclosed, {n_out_checked} outside points checked")
    assert len(polys) >= 300 and n_in >= 100 and n_enclosed >= 10 and n_out_checked >= 1000     # (floors against a blind test)


def _dist2(c, d, p):
    ab = d - c
    L = (ab * ab).sum()
    t = np.zeros(len(p)) if L == 0 else np.clip(((p - c) * ab).sum(axis=1) / L, 0.0, 1.0)
    q = p - (c + t[:, None] * ab)
    return (q * q).sum(axis=1)


def test_d20_agrees_with_d19_on_integer_coordinates(pm):
    """np_poly against np_rect on the integer scene, every rectangle of INT_RECTS in either orientation.  Fills: touches equal, no
    exception.  Strokes, Circles and ellipses: equal wherever D19's deciding quantity -- the least of its squared distances against
    hw * hw, dR2(c) against r * r, the ellipse's sum against 1 -- differs from its bound by a relative 1e-9 or more; the decisive pairs
    are counted and must be 95 % of all.  The scene's coordinates are integers below 256, so that np_rect alone shows the count."""
    scene = pc.int_scene(pm)
    kinds = _kinds(scene)
    rects = pc.INT_RECTS
    want = np_rect.item_flags(scene, rects)
    decisive = _d19_decisive(scene, rects)
    on_edge = _points_on_boundary(scene, rects)
    pairs = same = n_enclosed = 0
    for k, rect in enumerate(rects):
        for reverse in (False, True):
            f = np_poly.item_flags(scene, pc.rect_as_polygon(rect, reverse))
            fills = kinds == np_hit.FILL
            assert np.array_equal(f[fills] & T, want[fills, k] & T), (rect.tolist(), reverse)
            others = ~fills & decisive[:, k]
            assert np.array_equal(f[others] & T, want[others, k] & T), (rect.tolist(), reverse, np.flatnonzero(others & ((f & T) != (want[:, k] & T))).tolist())
            pairs += int((~fills).sum())
            same += int(others.sum())
            # enclosed: equal for Fills and Circles wherever no point of the item lies on the rectangle's boundary (there D19's closed
            # rectangle encloses and D20, strict, does not)
            free = np.isin(kinds, (np_hit.FILL, np_hit.CIRCLE)) & decisive[:, k] & ~on_edge[:, k]
            assert np.array_equal(f[free] & E, want[free, k] & E), (rect.tolist(), reverse)
            n_enclosed += int(((f[free] & E) != 0).sum())
    print(f"{same} of {pairs} (stroke or circle, rectangle) pairs decisive, {int((want & T != 0).sum())} touches by D19")
    assert n_enclosed >= 40 and len(rects) >= 50 and same >= 0.95 * pairs and (want[kinds != np_hit.FILL] & T).any() and (want[kinds == np_hit.FILL] & T).any()


def _d19_decisive(scene, rects):
    """bool [n_items, n]: D19's deciding quantity of a Line, Polyline, Circle or ellipse is off its bound by a relative 1e-9 or more
    (Fills: True).  By np_rect's own functions."""
    sc = bytes(scene)
    R = np_rect.Rects(rects)
    out = np.ones((len(np_hit.flat_items(sc)), R.n), bool)
    for i, (at, bbox) in enumerate(np_hit.flat_items(sc)):
        word = np.frombuffer(sc, np.uint32, 1, at)[0]
        tag = word & 0xFFFF
        if tag in (np_hit.LINE, np_hit.POLY):
            a, b, hw = np_hit.stroke_segments(sc, at, tag)
            q = np.minimum(np_rect.dist2_to_rect(R, a[:, 0], a[:, 1]), np_rect.dist2_to_rect(R, b[:, 0], b[:, 1]))
            for cx, cy in R.corners():
                q = np.minimum(q, _dist2_pairs(a[None], b[None], cx[:, None], cy[:, None]))
            q = np.where(np_rect.segments_meet(R, a, b), 0.0, q).min(axis=1)
            bound = hw * hw
        elif tag == np_hit.CIRCLE:
            x0, y0, x1, y1 = (np.float64(v) for v in bbox)
            cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
            rx, ry = cx - x0, cy - y0
            ex = np.maximum(np.maximum(R.x0 - cx, 0.0), cx - R.x1)
            ey = np.maximum(np.maximum(R.y0 - cy, 0.0), cy - R.y1)
            if word & np_hit.CIRCLE_ELLIPSE:
                q, bound = (ex / rx) * (ex / rx) + (ey / ry) * (ey / ry), 1.0
            else:
                q, bound = ex * ex + ey * ey, min(rx, ry) ** 2
        else:
            continue
        out[i] = np.abs(q - bound) >= 1e-9 * bound
    return out


def _dist2_pairs(a, b, x, y):
    ax, ay, bx, by = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    abx, aby = bx - ax, by - ay
    L = abx * abx + aby * aby
    t = np.where(L == 0, 0.0, np.clip(((x - ax) * abx + (y - ay) * aby) / np.where(L == 0, 1.0, L), 0.0, 1.0))
    dx, dy = x - (ax + abx * t), y - (ay + aby * t)
    return dx * dx + dy * dy


# ---- the calls --------------------------------------------------------------------------------------------------------

def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


def _flags(pm, skip, even_odd):
    return (pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0) | (pm._lib.PM_SEL_EVEN_ODD if even_odd else 0)


def device_select(pm, r, poly, n_items, skip=False, even_odd=False, pad=0, stream=None):
    """pm_select_polygon_device into n_items + pad words filled with UNTOUCHED, not waited for.  Under the emulation device memory is
    host memory and the array is numpy's; on the GPU it is torch's.  The vertices are a copy that is overwritten at once: the call has
    to have read them."""
    xy = np.array(poly, np.float32).reshape(-1, 2)
    if _emulated():
        words = np.full(n_items + pad, UNTOUCHED, np.uint32)
        pm._lib.check(pm._lib.load().pm_select_polygon_device(r._h, xy.ctypes.data, len(xy), _flags(pm, skip, even_odd), words.ctypes.data, words.size, None),
                      "pm_select_polygon_device")
    else:
        import torch

        words = torch.full((n_items + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
        r.select_polygon_tensor(xy, words, stream=stream, skip_transparent=skip, even_odd=even_odd)
    xy[:] = np.nan
    return words


def as_u32(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy().view(np.uint32)


def check_case(pm, r, case, combos=pc.COMBOS):
    """Host and device call for every polygon of the case, under every combination of the flags: equal to np_poly."""
    r.set_scene_bytes(case.scene)
    n_items = len(case.flags(0))
    for skip, eo in combos:
        words = [device_select(pm, r, poly, n_items, skip, eo) for poly in case.polys]
        r.sync()
        for k, poly in enumerate(case.polys):
            want = case.flags(k, skip, eo)
            got = as_u32(words[k])
            assert np.array_equal(got, want), (case, k, skip, eo, "device", poly[:6].tolist(), [(int(i), int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:8]])
            touched, enclosed = r.select_polygon(poly, skip_transparent=skip, even_odd=eo)
            got = touched * T + enclosed * E
            assert np.array_equal(got, want), (case, k, skip, eo, "host", poly[:6].tolist(), [(int(i), int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:8]])


@pytest.fixture(scope="module")
def poly_renderer(pm):
    """Never resized: the polygon queries need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", pc.SMALL)
def test_small_scenes(pm, pmo, poly_renderer, name):
    """rect_cases' mixed / edge / non-finite scenes, the oracle's path test and a scene of loose outlines under ~200 seeded polygons of
    every class (test_the_small_cases_have_every_class)."""
    check_case(pm, poly_renderer, pc.small_case(pm, pmo, name))


@pytest.mark.gpu
@pytest.mark.parametrize("n", rc.WALK_SIZES)
def test_item_walk_by_item_count(pm, poly_renderer, n):
    """One item fewer than a step of the walk, a step, one more, two steps and one."""
    check_case(pm, poly_renderer, pc.walk_case(pm, n))


@pytest.mark.gpu
@pytest.mark.parametrize("ident", pc.LONG_IDS)
def test_long_items(pm, poly_renderer, ident):
    """Fills and Polylines of 64, 65 and 513 chunks: decided by one segment of the last chunk, by the winding alone, by all points."""
    check_case(pm, poly_renderer, pc.long_case(pm, ident), combos=[(False, False), (True, True)])


@pytest.mark.gpu
def test_polygon_sizes(pm, pmo, poly_renderer):
    """m = 3 .. 4096 (poly_cases.M_SIZES)."""
    check_case(pm, poly_renderer, pc.size_case(pm, pmo), combos=[(False, False), (False, True)])


@pytest.mark.gpu
def test_distances_that_rounding_decides(pm, poly_renderer):
    """Strokes near the origin under polygons with vertices of 2^60 and 2^100 (poly_cases.origin_case): near K by D20's arithmetic,
    far from K's box."""
    check_case(pm, poly_renderer, pc.origin_case(pm), combos=[(False, False), (False, True)])


@pytest.mark.gpu
def test_rectangles_as_4gons_against_select_rect(pm, poly_renderer):
    """On integer coordinates a rectangle given as a 4-gon, either way round, touches the Fills and Circles select_rect says it
    touches, and encloses the same ones wherever no point of the item lies on the rectangle's boundary lines."""
    scene = pc.int_scene(pm)
    r = poly_renderer
    r.set_scene_bytes(scene)
    kinds = _kinds(scene)
    area = (kinds == np_hit.FILL) | (kinds == np_hit.CIRCLE)
    on_edge = _points_on_boundary(scene, pc.INT_RECTS)
    assert len(pc.INT_RECTS) >= 50
    compared = 0
    for k, rect in enumerate(pc.INT_RECTS):
        rt, re_ = r.select_rect(*[float(v) for v in rect])
        for reverse in (False, True):
            pt, pe = r.select_polygon(pc.rect_as_polygon(rect, reverse))
            assert np.array_equal(pt[area], rt[area]), (k, rect.tolist(), reverse)
            clear = area & ~on_edge[:, k]
            assert np.array_equal(pe[clear], re_[clear]), (k, rect.tolist(), reverse)
            compared += int(clear.sum())
    assert compared >= 50 * int(area.sum())


@pytest.mark.gpu
def test_select_rotated_rect(pm, poly_renderer):
    """A marquee turned by 45 degrees encloses the whole diagonal row and nothing else (what no square of its area does,
    test_the_rotated_marquee_case_by_numpy); the corners are poly_cases' and at angle 0 the call is select_polygon of them."""
    scene, marquee = _diagonal_scene(pm)
    r = poly_renderer
    r.set_scene_bytes(scene)
    assert np.array_equal(r.rotated_rect_vertices(*marquee).view(np.uint32), pc.rotated_rect_corners(*marquee).view(np.uint32))
    touched, enclosed = r.select_rotated_rect(*marquee)
    assert touched[:9].all() and enclosed[:9].all() and not touched[9] and not enclosed[9]
    corners = np.array([[30, 92], [170, 92], [170, 108], [30, 108]], np.float32)
    assert np.array_equal(r.rotated_rect_vertices(100.0, 100.0, 140.0, 16.0, 0.0), corners)
    a, b = r.select_rotated_rect(100.0, 100.0, 140.0, 16.0, 0.0), r.select_polygon(corners)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()


@pytest.mark.gpu
def test_hand_derived_answers(pm, poly_renderer):
    """poly_cases.KNOWN, each worked out by hand there."""
    r = poly_renderer
    r.set_scene_bytes(rc.known_scene(pm))
    for poly, eo, item, want in pc.KNOWN:
        touched, enclosed = r.select_polygon(np.array(poly, np.float32), even_odd=eo)
        assert int(touched[item]) * T + int(enclosed[item]) * E == want, (poly, eo, item, want)
    assert len(pc.KNOWN) >= 12


@pytest.mark.gpu
def test_output_discipline_and_argument_rules(pm, pmo, poly_renderer):
    r = poly_renderer
    lib = pm._lib.load()
    L = pm._lib
    case = pc.small_case(pm, pmo, "mixed")
    r.set_scene_bytes(case.scene)
    n_items = len(case.flags(0))
    poly = np.ascontiguousarray(case.polys[0])
    m = len(poly)
    want = case.flags(0)
    got_n, n_t, n_e = C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)
    # words beyond n_items are untouched, the counts are the words'
    words = np.full(n_items + 5, UNTOUCHED, np.uint32)
    assert lib.pm_select_polygon(r._h, poly.ctypes.data, m, 0, words.ctypes.data, words.size, C.byref(got_n), C.byref(n_t), C.byref(n_e)) == L.PM_OK
    assert got_n.value == n_items and np.array_equal(words[:n_items], want) and (words[n_items:] == UNTOUCHED).all()
    assert n_t.value == int((want & T != 0).sum()) and n_e.value == int((want & E != 0).sum())
    dev = device_select(pm, r, poly, n_items, pad=5)
    r.sync()
    assert np.array_equal(as_u32(dev)[:n_items], want) and (as_u32(dev)[n_items:] == UNTOUCHED).all()
    # PM_ERR_CAPACITY sets n_items and writes nothing else
    words[:] = UNTOUCHED
    got_n, n_t, n_e = C.c_uint32(77), C.c_uint32(77), C.c_uint32(77)
    assert lib.pm_select_polygon(r._h, poly.ctypes.data, m, 0, words.ctypes.data, n_items - 1, C.byref(got_n), C.byref(n_t), C.byref(n_e)) == L.PM_ERR_CAPACITY
    assert got_n.value == n_items and n_t.value == 77 and n_e.value == 77 and (words == UNTOUCHED).all()
    assert lib.pm_select_polygon_device(r._h, poly.ctypes.data, m, 0, words.ctypes.data, n_items - 1, None) == L.PM_ERR_CAPACITY
    # m out of range, unknown flag bits, NULL pointers: PM_ERR_INVALID, nothing written
    big = np.zeros((L.PM_POLYGON_MAX_VERTICES + 1, 2), np.float32)
    sel = [lambda *a: lib.pm_select_polygon(r._h, *a, None, None, None), lambda *a: lib.pm_select_polygon_device(r._h, *a, None)]   # (xy, m, flags, words, cap)
    for call in sel:
        assert call(big.ctypes.data, 2, 0, words.ctypes.data, words.size) == L.PM_ERR_INVALID
        assert call(big.ctypes.data, len(big), 0, words.ctypes.data, words.size) == L.PM_ERR_INVALID
        assert call(poly.ctypes.data, m, 4, words.ctypes.data, words.size) == L.PM_ERR_INVALID
        assert call(poly.ctypes.data, m, 0x80000000, words.ctypes.data, words.size) == L.PM_ERR_INVALID
        assert call(None, m, 0, words.ctypes.data, words.size) == L.PM_ERR_INVALID
        assert call(poly.ctypes.data, m, 0, None, words.size) == L.PM_ERR_INVALID
    assert (words == UNTOUCHED).all()
    # PM_SEL_EVEN_ODD is the polygon calls' alone
    rect = np.array([0, 0, 10, 10], np.float32)
    assert lib.pm_select_rect(r._h, rect.ctypes.data, L.PM_SEL_EVEN_ODD, words.ctypes.data, words.size, None, None, None) == L.PM_ERR_INVALID
    assert lib.pm_select_rect_device(r._h, rect.ctypes.data, L.PM_SEL_EVEN_ODD, words.ctypes.data, words.size, None) == L.PM_ERR_INVALID
    # Python: what select_rect / select_rect_tensor raise
    with pytest.raises(ValueError):
        r.select_polygon(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        r.select_polygon(big)
    with pytest.raises(ValueError):
        r.select_polygon(np.zeros((4, 3), np.float32))
    if not _emulated():
        import torch

        with pytest.raises(TypeError):
            r.select_polygon_tensor(poly, torch.zeros(n_items, device="cuda"))
        with pytest.raises(TypeError):
            r.select_polygon_tensor(poly, torch.zeros(n_items, dtype=torch.int32))
        with pytest.raises(RuntimeError):
            r.select_polygon_tensor(poly, torch.zeros(n_items, dtype=torch.int32, device="cuda")[:0])
    # no scene resident
    with pm.Renderer(0) as fresh:
        got_n = C.c_uint32(77)
        assert lib.pm_select_polygon(fresh._h, poly.ctypes.data, m, 0, words.ctypes.data, words.size, C.byref(got_n), None, None) == L.PM_ERR_INVALID
        assert got_n.value == 0
        assert lib.pm_select_polygon_device(fresh._h, poly.ctypes.data, m, 0, words.ctypes.data, words.size, None) == L.PM_ERR_INVALID


@pytest.mark.gpu
def test_back_to_back_device_calls_keep_their_polygons(pm, pmo, poly_renderer):
    """More device calls than the staging ring has slots, none waited for, on one stream and alternating between two: every answer
    is its own polygon's (device_select overwrites the vertices as soon as the call returns)."""
    r = poly_renderer
    case = pc.size_case(pm, pmo)
    r.set_scene_bytes(case.scene)
    n_items = len(case.flags(0))
    ks = [0, 1, 2, 5, 9, 12, 16, 20, 3, 7]
    streams = [None, None]
    if not _emulated():
        import torch

        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for use in ([streams[0]] * len(ks), [streams[j % 2] for j in range(len(ks))]):
        words = [device_select(pm, r, case.polys[k], n_items, stream=q) for k, q in zip(ks, use)]
        r.sync()
        if not _emulated():
            torch.cuda.synchronize()
        for k, w in zip(ks, words):
            assert np.array_equal(as_u32(w), case.flags(k)), k
    assert len({case.flags(k).tobytes() for k in ks}) >= 4


def _tiger_polys(w, h):
    """Lassos over the Tiger's view: one around its middle, a pentagram over all of it, a small triangle, the view as a 4-gon."""
    return [np.ascontiguousarray(p, np.float32) for p in (
        pc.lasso((w / 2.0, h / 2.0), h / 3.0, 40, 5), pc.pentagram((w / 2.0, h / 2.0), 0.6 * h), np.array([[200.0, 100.0], [260.0, 110.0], [230.0, 150.0]]),
        pc.box(0.0, 0.0, float(w), float(h)))]


@pytest.mark.gpu
def test_a_device_call_answers_for_the_scene_resident_at_the_call(pm):
    """The Tiger at 480 x 270: device calls on a caller's stream, followed at once by two re-flattens -- the answers are the first
    scene's (the re-flattens run on the context's stream and have to wait for the event behind the calls); the host call afterwards
    answers for the last."""
    wl = pm.workloads.tiger(480, 270)
    polys = _tiger_polys(wl.width, wl.height)
    with pm.Renderer(0) as r:
        _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene0 = r.download_scene()
        if _emulated():
            s = None
        else:
            import torch

            s = torch.cuda.Stream()
        words = [device_select(pm, r, p, n_items, even_odd=bool(k % 2), stream=s) for k, p in enumerate(polys)]
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        r.reflatten((0.9, 0.0, 0.0, 0.9, 40.0, 30.0), wl.width_scale)
        r.sync()
        if s is not None:
            s.synchronize()
        want0 = [np_poly.item_flags(scene0, p, even_odd=bool(k % 2)) for k, p in enumerate(polys)]
        for k in range(len(polys)):
            assert np.array_equal(as_u32(words[k]), want0[k]), k
        assert all((w & T).any() and not (w & E).all() for w in want0) and (want0[0] & E).any()
        scene2 = r.download_scene()
        for k, p in enumerate(polys):
            touched, enclosed = r.select_polygon(p, even_odd=bool(k % 2))
            want2 = np_poly.item_flags(scene2, p, even_odd=bool(k % 2))
            assert np.array_equal(touched * T + enclosed * E, want2), k
            assert k == 3 or not np.array_equal(want2, want0[k]), k


@pytest.mark.gpu
def test_calls_between_frames_leave_the_frames_alone(pm, pmo):
    """Frames rendered before and after polygon queries have the oracle's bytes, as they have without them."""
    wl = pm.workloads.tiger(480, 270)
    polys = _tiger_polys(wl.width, wl.height)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want = pmo.render(scene, wl.width, wl.height)
        r.render()
        words = [device_select(pm, r, p, n_items) for p in polys]   # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        host = [r.select_polygon(p) for p in polys]
        second = r.read_pixels()
        assert np.array_equal(first, want) and np.array_equal(second, want)
        for k, p in enumerate(polys):
            f = np_poly.item_flags(scene, p)
            assert np.array_equal(as_u32(words[k]), f) and np.array_equal(host[k][0] * T + host[k][1] * E, f), k


@pytest.mark.gpu
def test_cli_lasso(pm, tmp_path, capsys):
    """--lasso prints what select_polygon returns, in --select's format."""
    from piet_metal_amd import cli

    lasso = [60.0, 40.0, 200.0, 60.0, 180.0, 200.0, 50.0, 150.0]
    assert cli.main(["tiger", str(tmp_path / "t.png"), "--width", "256", "--height", "256", "--lasso", ",".join(f"{v:g}" for v in lasso)]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("60,40,")]
    with pm.Renderer(0) as r:
        r.resize(256, 256)
        r.flatten_and_encode(pm.PathSet.tiger(), (256 / 200.0, 0.0, 0.0, 256 / 200.0, 0.0, 0.0), 256 / 200.0)
        touched, enclosed = r.select_polygon(np.array(lasso, np.float32).reshape(-1, 2))
        of_item = r.item_paths()
    name = ",".join(f"{v:g}" for v in lasso)
    want = [f"{name}: item {int(i)} path {int(of_item[i])}" + (" enclosed" if enclosed[i] else "") for i in np.flatnonzero(touched)]
    assert lines == want and len(want) >= 10 and enclosed.any() and not enclosed.all()


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_hit_polygon_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- CPU: the kernel's text and the compiler's listing ---------------------------------------------------------------------------

def test_structural_constants_are_the_kernels():
    """poly_cases.M_SIZES brackets the sizes at which the kernel takes another path: a group of edges with a box of its own, a round
    of 64 points, and the vertex cap."""
    text = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_hit_poly.h")).read()
    assert int(re.search(r"constexpr uint32_t kPolyMaxVertices = (\d+)u;", text).group(1)) == pc.MAX_VERTICES == np_poly.MAX_VERTICES
    assert int(re.search(r"constexpr uint32_t kPolyGroup = (\d+)u;", text).group(1)) == pc.GROUP
    host = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    assert "kPolyGroupEdges" not in host and "constexpr size_t kGroup = pm::kPolyGroup;" in host   # (the host's groups are the kernel's)
    head = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    assert int(re.search(r"#define PM_POLYGON_MAX_VERTICES (\d+)u", head).group(1)) == pc.MAX_VERTICES
    assert int(re.search(r"#define PM_SEL_EVEN_ODD (\d+)u", head).group(1)) == 2
    assert "k0 += 64u" in text and pc.WAVE == 64
    for size in (pc.GROUP, pc.WAVE, pc.MAX_VERTICES):
        assert {size - 1, size} <= set(pc.M_SIZES) and (size == pc.MAX_VERTICES or size + 1 in pc.M_SIZES)
    assert min(pc.M_SIZES) == 3


def test_the_polygon_kernel_uses_no_scratch(tmp_path):
    """pm_select_polygon_kernel by the flags the library is built with: no private segment, no LDS (0 bytes), VGPRs
    within 128.  The figures are printed (pytest -s) and stand in DESIGN.md 4."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = 0
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        if "pm_select_polygon_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        print(f"pm_select_polygon_kernel: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}")
        assert scratch == 0 and vgpr <= 128 and lds == 0, (scratch, vgpr, lds)
    assert found == 1
