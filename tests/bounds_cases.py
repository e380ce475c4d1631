"""Scenes, labels and selection words for the bounds queries, pm_item_bounds / pm_union_bounds (test helper, not a conftest):
tests/test_bounds.py runs them against tests/np_bounds.py under the emulation and on the GPU, and pins on the CPU, with numpy
alone, that the cases are what they claim.

The kernels (piet_metal_amd/csrc/pm_bounds.h) deal the items 64 per step, a lane per item; a plain Fill or a Polyline is the union
of its chunk boxes (a chunk is CHUNK_SEGS segments), a compound Fill and a one-point Polyline are walked point by point; an item
of up to LANE entries is finished by its lane, a longer one by the whole wave, 64 entries per step.

  known_scene     rect_cases.known_scene: one item of every kind, its boxes worked out by hand (KNOWN_BOXES);
  counts_scene    plain Fills, compound Fills and Polylines of 0, 1, 2, 4, 5, 8 and 9 points;
  special_scene   a one-point Polyline, widths 0, negative and NaN, points at -0.0f, NaN points, a chunk of NaNs, points at
                  +-3e38, a compound Fill with a chunk of nothing but separators and one whose separator names a separator,
                  circles and ellipses with saturated ShortBbox edges, rx = 0 and an inverted box, items of alpha 0, a stroke
                  whose box is no f32 value;
  long_scene      Fills, compound Fills and Polylines around every threshold: 8 / 9, 16 / 17, 64 / 65 and 129 chunks (or points),
                  with the extreme values in the first chunk, the last and the one behind the 64th;
  walk scenes     hit_structure.walk_scene at 1, 63, 64, 65 and 257 items: every kind in turn, a child group, every third item of alpha 0.

Values that an encoder would refuse or tidy are written into the encoded bytes afterwards (patch_*): the scene format is data."""
from __future__ import annotations

import struct

import numpy as np

import hit_structure as hs
import np_bounds
import np_hit
import rect_cases

F32 = np.float32
INF = np.inf
WAVE = hs.WAVE
LANE = 16                       # kBoundsLane (pm_bounds.h)
POINT_COUNTS = (0, 1, 2, 4, 5, 8, 9)
LONG_SIZES = (8, 9, LANE, LANE + 1, WAVE, WAVE + 1, 2 * WAVE + 1)
WALK_SIZES = (1, WAVE - 1, WAVE, WAVE + 1, 4 * WAVE + 1)
SEED = F32(3.0e38)              # what pm_index_kernel seeds a chunk box with, and the coordinate bound of DESIGN.md 9

# rect_cases.known_scene, item by item: the Fill [10, 20]^2; the Polyline y = 10, x 30 .. 50, hw 1; the Circle (70, 15) r 5; the
# ring [10, 40] x [40, 70]; the Line x = 60, y 40 .. 60, hw 2; the ellipse (90, 50) 10 x 5; the two-point Fill; the hairline
# y = 90, x 10 .. 120, hw 0.5; the ellipse with ry = 0: no geometry
KNOWN_BOXES = np.array([[10, 10, 20, 20], [29, 9, 51, 11], [65, 10, 75, 20], [10, 40, 40, 70], [58, 38, 62, 62], [80, 45, 100, 55], [110, 10, 120, 20],
                        [9.5, 89.5, 120.5, 90.5], [INF, INF, -INF, -INF]], np.float64)


# ---- writing into encoded bytes --------------------------------------------------------------------------------------------

def _item(scene, i):
    return np_hit.flat_items(bytes(scene))[i][0]


def patch_points(scene, i, at, values):
    """Entries at .. of item i's point array become `values` (float32 pairs; a separator is (NaN, index bits))."""
    v = np.ascontiguousarray(values, F32).reshape(-1, 2)
    npt, pix = struct.unpack_from("<II", bytes(scene), _item(scene, i) + 12)
    assert at + len(v) <= npt
    scene[pix + 8 * at : pix + 8 * (at + len(v))] = v.view(np.uint8).reshape(-1)


def patch_npt(scene, i, npt):
    old = struct.unpack_from("<I", bytes(scene), _item(scene, i) + 12)[0]
    assert npt <= old
    scene[_item(scene, i) + 12 : _item(scene, i) + 16] = np.frombuffer(struct.pack("<I", npt), np.uint8)


def patch_width(scene, i, width):
    at = _item(scene, i)
    tag = struct.unpack_from("<I", bytes(scene), at)[0] & 0xFFFF
    off = {np_hit.LINE: 12, np_hit.POLY: 8}[tag]
    scene[at + off : at + off + 4] = np.frombuffer(struct.pack("<f", width), np.uint8)


def patch_short_bbox(scene, i, box):
    """The ShortBbox of root item i (the scene's first group)."""
    scene[8 + 8 * i : 16 + 8 * i] = np.frombuffer(struct.pack("<4H", *box), np.uint8)


def separator(index):
    return [np.nan, np.frombuffer(struct.pack("<I", index), F32)[0]]


def sq(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def ring(cx, cy, r, n):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1)


# ---- the scenes --------------------------------------------------------------------------------------------------------------

_scenes = {}


def known_scene(pm):
    return rect_cases.known_scene(pm)


def counts_scene(pm):
    """For n in POINT_COUNTS: a plain Fill, a compound Fill (two sub-paths where n allows) and a Polyline of width 3 of n points each,
    3 * len(POINT_COUNTS) items.  n = 0 is an item of one point whose count is set to 0 afterwards."""
    if "counts" not in _scenes:
        def emit(e):
            for k, n in enumerate(POINT_COUNTS):
                m = max(n, 1)
                pts = ring(40.0 + 50 * k, 40.0, 10.0 + k, m) + [0.25, 0.5]
                e.fill(pts, 0x336699FF)
                e.fill_compound([pts[: m // 2] + [0, 60], pts[m // 2 :] + [0, 60]] if m >= 6 else [pts + [0, 60]], 0xAA5500FF, even_odd=bool(k & 1))
                e.polyline(pts + [0, 120], 0x11AA22FF, 3.0)

        scene = hs._encode(pm, 3 * len(POINT_COUNTS), emit)
        for j in range(3):
            patch_npt(scene, j, 0)
        _scenes["counts"] = scene
    return _scenes["counts"]


SPECIAL = {}   # name -> item index, filled by special_scene


def special_scene(pm):
    if "special" in _scenes:
        return _scenes["special"]
    entries = [   # (name, what emits the item, what is written into its bytes afterwards ...)
        ("poly_one_point", lambda e: e.polyline(np.array([[30.0, 20.0]]), 0x11AA22FF, 4.0)),
        ("poly_width_0", lambda e: e.polyline(np.array([[10.0, 40.0], [50.0, 44.0], [30.0, 60.0]]), 0x11AA22FF, 0.0)),
        ("poly_width_negative", lambda e: e.polyline(np.array([[10.0, 70.0], [50.0, 74.0], [30.0, 90.0]]), 0x11AA22FF, 1.0), ("width", -6.0)),
        ("poly_width_nan", lambda e: e.polyline(np.array([[10.0, 100.0], [50.0, 104.0]]), 0x11AA22FF, 1.0), ("width", float("nan"))),
        ("poly_width_very_negative", lambda e: e.polyline(np.array([[10.0, 70.0], [12.0, 74.0]]), 0x11AA22FF, 1.0), ("width", -100.0)),
        ("line_width_nan", lambda e: e.stroke_line((60.0, 10.0), (90.0, 30.0), 2.0, 0x000000FF), ("width", float("nan"))),
        ("line_width_negative", lambda e: e.stroke_line((60.0, 40.0), (90.0, 60.0), 2.0, 0x000000FF), ("width", -3.0)),
        ("line_width_0", lambda e: e.stroke_line((60.0, 70.0), (90.0, 65.0), 0.0, 0x000000FF)),
        ("fill_negative_zero", lambda e: e.fill(sq(1, 1, 2, 2), 0x336699FF), ("points", 0, [[-0.0, -0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]])),
        ("fill_zero_max", lambda e: e.fill(sq(1, 1, 2, 2), 0x336699FF), ("points", 0, [[-5.0, -7.0], [-0.0, -1.0], [-3.0, -0.0], [-0.0, -0.0]])),
        ("poly_negative_zero", lambda e: e.polyline(sq(1, 1, 2, 2), 0x11AA22FF, 0.0), ("points", 0, [[-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [-0.0, -0.0]])),
        ("fill_nan_x", lambda e: e.fill(sq(100, 10, 140, 50), 0x336699FF), ("points", 1, [[np.nan, 5.0]])),
        ("fill_nan_y", lambda e: e.fill(sq(100, 60, 140, 90), 0x336699FF), ("points", 2, [[150.0, np.nan]])),
        ("fill_chunk_of_nans", lambda e: e.fill(ring(120.0, 130.0, 20.0, 12), 0x336699FF), ("points", 4, [[np.nan, np.nan]] * 5)),
        ("fill_all_nan", lambda e: e.fill(sq(1, 1, 2, 2), 0x336699FF), ("points", 0, [[np.nan, np.nan]] * 4)),
        ("poly_all_x_nan", lambda e: e.polyline(ring(160.0, 130.0, 10.0, 9), 0x11AA22FF, 2.0), ("points", 0, [[np.nan, 100.0 + k] for k in range(9)])),
        ("fill_at_plus_seed", lambda e: e.fill(sq(1, 1, 2, 2), 0x336699FF), ("points", 0, [[SEED, SEED]] * 4)),
        ("fill_at_minus_seed", lambda e: e.fill(sq(1, 1, 2, 2), 0x336699FF), ("points", 0, [[-SEED, -SEED]] * 4)),
        ("fill_one_point_at_seed", lambda e: e.fill(ring(200.0, 40.0, 20.0, 9), 0x336699FF), ("points", 6, [[SEED, -SEED]])),
        ("poly_at_minus_seed", lambda e: e.polyline(ring(200.0, 100.0, 20.0, 6), 0x11AA22FF, 2.0), ("points", 5, [[-SEED, SEED]])),
        ("poly_infinite", lambda e: e.polyline(ring(200.0, 100.0, 20.0, 3), 0x11AA22FF, 2.0), ("points", 1, [[INF, -INF]])),
        ("compound_separator_chunk", lambda e: e.fill_compound([ring(260.0, 40.0, 20.0, 12)], 0xAA5500FF),
            ("points", 4, [separator(0), separator(0), separator(8), separator(8)])),
        ("compound_separator_names_separator", lambda e: e.fill_compound([ring(260.0, 100.0, 20.0, 9)], 0xAA5500FF),
            ("points", 3, [separator(7)]), ("points", 7, [[np.nan, 512.0]])),
        ("compound_only_separators", lambda e: e.fill_compound([sq(1, 1, 2, 2)], 0xAA5500FF), ("points", 0, [separator(0)] * 4)),
        ("circle_saturated", lambda e: e.circle((300.0, 40.0), 10.0), ("bbox", (0, 0, 65535, 65535))),
        ("circle_saturated_low", lambda e: e.circle((300.0, 40.0), 10.0), ("bbox", (0, 0, 7, 20))),
        ("ellipse_saturated_high", lambda e: e.ellipse((300.0, 40.0), 10.0, 5.0), ("bbox", (65000, 65530, 65535, 65535))),
        ("ellipse_rx_0", lambda e: e.ellipse((300.0, 100.0), 0.0, 5.0)),
        ("ellipse_ry_0", lambda e: e.ellipse((300.0, 100.0), 6.0, 0.0)),
        ("circle_r_0", lambda e: e.circle((300.0, 150.0), 0.0)),
        ("circle_inverted", lambda e: e.circle((300.0, 40.0), 10.0), ("bbox", (40, 10, 30, 50))),
        ("ellipse_odd_sum", lambda e: e.ellipse((300.0, 40.0), 10.0, 5.0), ("bbox", (10, 20, 21, 45))),
        ("fill_transparent", lambda e: e.fill(sq(400, 400, 500, 500), 0x33669900)),
        ("poly_transparent", lambda e: e.polyline(sq(-400, -400, -300, -300), 0x11AA2200, 2.0)),
        ("line_transparent", lambda e: e.stroke_line((600.0, 0.0), (700.0, 10.0), 2.0, 0x00000000)),
        ("compound_transparent", lambda e: e.fill_compound([sq(0, 600, 10, 610), sq(2, 602, 8, 608)], 0xAA550000)),
        ("poly_inexact_in_f32", lambda e: e.polyline(np.array([[16777216.0, 3.0e7], [16777300.0, 3.0e7 + 64]]), 0x11AA22FF, 0.5)),
        ("fill_last", lambda e: e.fill(sq(5.5, 6.5, 7.5, 8.5), 0x336699FF)),
    ]
    names = [en[0] for en in entries]
    patches = [(i, p) for i, en in enumerate(entries) for p in en[2:]]
    n = len(entries)

    def emit(e):
        for en in entries:
            en[1](e)

    scene = hs._encode(pm, n, emit)
    for i, p in patches:
        if p[0] == "width":
            patch_width(scene, i, p[1])
        elif p[0] == "points":   # (the item's ShortBbox no longer holds its points: saturated on every side, it bounds nothing)
            patch_points(scene, i, p[1], p[2])
            patch_short_bbox(scene, i, (0, 0, 65535, 65535))
        else:
            patch_short_bbox(scene, i, p[1])
    SPECIAL.clear()
    SPECIAL.update({name: i for i, name in enumerate(names)})
    _scenes["special"] = scene
    return scene


LONG = []   # (kind, size) per item of long_scene, between a lead and a trailing item


def long_scene(pm):
    """Item 0 a lead Fill of 9 points (3 chunks: the next item's first chunk sits at residue 3 of a super-chunk); then for every size
    in LONG_SIZES a plain Fill and a Polyline of `size` chunks and a compound Fill of `size` entries; a trailing Fill.  In every long
    item the smallest x is in the first chunk; the largest y (+500) is written into its last point, and the smallest y (-500)
    into the first point behind its 64th chunk (entry) where the item has more than 65, else into point 5."""
    if "long" in _scenes:
        return _scenes["long"]
    LONG.clear()
    for size in LONG_SIZES:
        LONG.extend([("fill", size), ("polyline", size), ("compound", size)])

    def points(kind, size):
        if kind == "compound":
            n = size - 2      # two sub-paths, a separator behind each: `size` entries
            k = np.arange(n)
            pts = np.stack([10.0 + 2.0 * k, np.where(k & 1, 110.0, 100.0)], axis=1)
            return [pts[: n // 2], pts[n // 2 :]]
        return rect_cases.long_points("polyline" if kind == "polyline" else "fill-nz", size)

    def emit(e):
        e.fill(ring(300.0, 20.0, 3.0, 9), 0x223344FF)
        for kind, size in LONG:
            p = points(kind, size)
            if kind == "fill":
                e.fill(p, 0x336699FF)
            elif kind == "polyline":
                e.polyline(p, 0x11AA22FF, 0.5)
            else:
                e.fill_compound(p, 0xAA5500FF)
        e.fill(sq(900, 60, 910, 70), 0x884400FF)

    scene = hs._encode(pm, len(LONG) + 2, emit, cap=1 << 20)
    sc = bytes(scene)
    for j, (kind, size) in enumerate(LONG):
        i = j + 1
        npt = struct.unpack_from("<I", sc, _item(scene, i) + 12)[0]
        per = 1 if kind == "compound" else hs.CHUNK_SEGS
        assert -(-(npt - (kind == "polyline")) // per) == size, (kind, size, npt)
        low = 64 * per if size > 65 else 5          # (entry 64 of the compound Fill of 65 entries is its last separator)
        last = npt - 2 if kind == "compound" else npt - 1
        pts = np_hit._points(sc, _item(scene, i))
        assert not np.isnan(pts[low]).any() and not np.isnan(pts[last]).any()
        patch_points(scene, i, last, [[pts[last][0], 500.0]])
        patch_points(scene, i, low, [[pts[low][0], -500.0]])
        patch_short_bbox(scene, i, (0, 0, 65535, 65535))     # (saturated on every side: it bounds nothing)
    _scenes["long"] = scene
    return scene


def walk_scene(pm, n):
    if ("walk", n) not in _scenes:
        _scenes[("walk", n)] = hs.walk_scene(pm, n).scene
    return _scenes[("walk", n)]


SCENES = ("known", "counts", "special", "long") + tuple(f"walk-{n}" for n in WALK_SIZES)


def scene_of(pm, name):
    if name.startswith("walk-"):
        return walk_scene(pm, int(name[5:]))
    return {"known": known_scene, "counts": counts_scene, "special": special_scene, "long": long_scene}[name](pm)


# ---- labels and selection words -----------------------------------------------------------------------------------------------

def labelings(n):
    """name -> (labels or None, n_labels) for a scene of n items: all equal (no table, and a table of zeros); alternating; runs of 48
    (the second crosses the wave boundary at item 64); some labels >= n_labels, 0xffffffff among them; 65 and 1000 labels with most
    of them unused; every item its own label."""
    i = np.arange(n, dtype=np.uint32)
    out = {
        "none": (None, 1),
        "zeros": (np.zeros(n, np.uint32), 1),
        "alternating": (i % 2, 2),
        "runs_of_48": (i // 48, int((n - 1) // 48 + 1) if n else 1),
        "out_of_range": (np.where(i % 5 == 0, 0xFFFFFFFF, np.where(i % 5 == 1, 3, i % 3)).astype(np.uint32), 3),
        "sparse_65": ((i // 7 * 13) % 65, 65),
        "sparse_1000": (np.where(i % 2 == 0, 999, (i * 37) % 1000).astype(np.uint32), 1000),
        "own": (i, max(n, 1)),
    }
    return out


def selection_words(n, seed):
    """uint32 [n + 3]: PM_SEL_* words as a selection call leaves them -- 0, 1, 2 and 3 in a seeded order -- and three more words than items."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, n + 3).astype(np.uint32)


_boxes = {}


def expected_boxes(pm, name, skip=False):
    """np_bounds.item_bounds of the scene, computed once and never written to."""
    if (name, skip) not in _boxes:
        b = np_bounds.item_bounds(scene_of(pm, name), skip)
        b.setflags(write=False)
        _boxes[(name, skip)] = b
    return _boxes[(name, skip)]
