"""Scenes and pixel windows for the item map, pm_hit_frame (test helper, not a conftest): tests/test_hit_frame.py runs them
against tests/np_hit.py under the emulation and on the GPU, and checks on the CPU that no window is blind.

The kernel (piet_metal_amd/csrc/pm_hit_frame.h) gives a workgroup of 256 threads a 16 x 16 tile of the window, tiles aligned to the
window's origin.  It walks the items ITEMS_PER_STEP at a time from the top of paint order, culls them against the tile, and
reaches a Fill's or a Polyline's segments through the scene index CHUNKS_PER_ROUND chunk ids at a time (an item of more chunks:
CHUNKS_PER_ROUND super-chunks at a time, the survivors expanded CHUNKS_PER_ROUND / SUPER_CHUNKS at a time).

  geometry_windows   part 1: mixed_scene, edge_scene and the oracle's path test under windows of the sizes that matter to the
                     tiling, PLACED over content by place(): the first origin, no multiple of 16, at which the window holds two
                     items and some nothing;
  walk_scene         part 3: n items of every kind on a grid of 4 x 4-pixel cells;
  long_cases         part 4: hit_structure's long items under a thin strip across their strokes;
  centres_scene      part 5: geometry ON pixel centres.

expected() is np_hit on the window's pixel centres, computed once per (case, flag)."""
from __future__ import annotations

import os
import re

import numpy as np

import hit_structure as hs
import np_hit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = hs.NONE
TILE = 16
F32 = np.float32


def kernel_constants():
    """{name: value} of pm_hit_frame.h's structural constants: a retuned kernel moves the cases with it."""
    text = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_hit_frame.h")).read()
    got = {k: int(v) for k, v in re.findall(r"^constexpr uint32_t (kFrameTile|kFrameItems|kFrameChunks) = (\d+);", text, re.M)}
    assert set(got) == {"kFrameTile", "kFrameItems", "kFrameChunks"}, got
    return got


_K = kernel_constants()
ITEMS_PER_STEP = _K["kFrameItems"]
CHUNKS_PER_ROUND = _K["kFrameChunks"]
assert _K["kFrameTile"] == TILE


def centres(x0, y0, w, h):
    """float32 [w * h, 2], row by row: float32(x0 + i) + 0.5 (exact below 65 536)."""
    ys, xs = np.mgrid[0:h, 0:w]
    x = (x0 + xs).astype(F32) + F32(0.5)
    y = (y0 + ys).astype(F32) + F32(0.5)
    assert x.dtype == F32 and (x.astype(np.float64) == x0 + xs + 0.5).all()
    return np.stack([x.ravel(), y.ravel()], axis=1)


class Window:
    """A scene and a pixel rectangle of it."""

    def __init__(self, ident, scene, x0, y0, w, h, **facts):
        self.ident, self.scene, self.rect, self.facts = ident, scene, (x0, y0, w, h), facts
        self._want = {}

    def __repr__(self):
        return f"{self.ident} {self.rect}"

    def expected(self, skip=False):
        """(top_item, n_hit) uint32 [h, w] by np_hit; shared by the tests, never written to."""
        if skip not in self._want:
            x0, y0, w, h = self.rect
            top, cnt = np_hit.hit_test(self.scene, centres(x0, y0, w, h), skip)
            top, cnt = top.reshape(h, w), cnt.reshape(h, w)
            top.setflags(write=False)
            cnt.setflags(write=False)
            self._want[skip] = (top, cnt)
        return self._want[skip]


def not_blind(top, items=2):
    """At least two distinct items and some PM_HIT_NONE."""
    vals = set(np.unique(top).tolist())
    return NONE in vals and len(vals - {NONE}) >= items


def place(scene, w, h, region, items=2):
    """The first origin (x0, y0) in `region` = (xa, ya, xb, yb), scanning rows then columns, neither coordinate a multiple of 16,
    at which the w x h window's expected map is not blind.  One np_hit map of the region serves every candidate."""
    xa, ya, xb, yb = region
    full = np_hit.hit_test(scene, centres(xa, ya, xb - xa, yb - ya))[0].reshape(yb - ya, xb - xa)
    for y0 in range(ya, yb - h + 1):
        for x0 in range(xa, xb - w + 1):
            if x0 % TILE and y0 % TILE and not_blind(full[y0 - ya : y0 - ya + h, x0 - xa : x0 - xa + w], items):
                return x0, y0
    raise AssertionError(f"no {w} x {h} window over two items and nothing in {region}")


# ---- part 1: window geometry -----------------------------------------------------------------------------------------

SIZES = [(16, 16), (17, 1), (1, 17), (33, 18)]
REGIONS = {"mixed": (0, 0, 96, 96), "edge": (65440, 0, 65536, 120), "path_test": None}
# edge_scene's items are 56 pixels and more apart where pixels exist (the second fill ends at y = 40, the line runs at y = 96 and
# below; the first fill is alone in the positive quadrant): its small windows hold ONE item and nothing, the large one at 65 536 two.
# The oracle's path test is one Fill.
ITEMS_WANTED = {"mixed": 2, "edge": 1, "path_test": 1}


def _content_region(scene, limit=160):
    """The boxes of the scene's items, clipped to [0, limit)^2 and widened by a tile."""
    boxes = np.array([b for _, b in np_hit.flat_items(bytes(scene))], np.int64)
    xa, ya = max(int(boxes[:, 0].min()) - TILE, 0), max(int(boxes[:, 1].min()) - TILE, 0)
    return xa, ya, min(xa + limit, int(boxes[:, 2].max()) + TILE), min(ya + limit, int(boxes[:, 3].max()) + TILE)


_geometry = {}


def geometry_windows(pm, pmo):
    """[Window] of part 1.  The 1 x 1 window cannot hold two items and nothing by itself: there are three of them per scene -- the
    first pixel of the placed 16 x 16 window's first and second item and of its nothing -- and TOGETHER they are not blind."""
    if _geometry:
        return list(_geometry.values())
    from test_hit_gpu import edge_scene, mixed_scene

    scenes = {"mixed": mixed_scene(pm), "edge": edge_scene(pm), "path_test": pmo.scene_path_test()}
    out = []
    for name, scene in scenes.items():
        region = REGIONS[name] or _content_region(scene)
        for k, (w, h) in enumerate(SIZES):
            x0, y0 = place(scene, w, h, region, ITEMS_WANTED[name])
            out.append(Window(f"{name}-{w}x{h}", scene, x0, y0, w, h, items=ITEMS_WANTED[name]))
            if (w, h) == (16, 16):
                top = out[-1].expected()[0]
                vals = [v for v in np.unique(top).tolist() if v != NONE][: ITEMS_WANTED[name]] + [NONE]
                for n, v in enumerate(vals):
                    j, i = np.argwhere(top == v)[0]
                    out.append(Window(f"{name}-1x1-{n}", scene, x0 + int(i), y0 + int(j), 1, 1, single=True))
        # (at the origin edge_scene's first fill covers all 48 x 40 pixels: that window has no nothing, the 72 x 64 one below has)
        out.append(Window(f"{name}-48x40-origin", scene, 0, 0, 48, 40, items=ITEMS_WANTED[name], covered=(name == "edge")))
    edge = scenes["edge"]
    # a window ending at x = 65 536: the second fill's box and the line's are saturated at 65 535, the last column's centre, 65 535.5,
    # lies beyond that edge and inside both; the fill ends at y = 40 and the line is far below the first rows
    out.append(Window("edge-ends-at-65536", edge, 65536 - 37, 3, 37, 110))
    # ... and at (0, 0), over the first fill and the polyline, whose boxes are saturated at 0 (they begin at negative coordinates)
    out.append(Window("edge-72x64-origin", edge, 0, 0, 72, 64, items=1))
    for wdw in out:
        _geometry[wdw.ident] = wdw
    return out


# ---- part 3: the item walk, by item count ------------------------------------------------------------------------------

CELL = 4
COLS = 32
WALK_ORIGIN = (3, 5)                     # of the window; no multiple of 16
WALK_KINDS = ("fill", "compound", "polyline", "line", "circle", "ellipse")
WALK_SIZES = (ITEMS_PER_STEP - 1, ITEMS_PER_STEP, ITEMS_PER_STEP + 1, 2 * ITEMS_PER_STEP + 1)


def walk_cell(i):
    """Top-left corner of the cell of ordinary item i (1 <= i <= n - 3): the grid begins one tile right of the window's origin."""
    k = i - 1
    return WALK_ORIGIN[0] + TILE + CELL * (k % COLS), WALK_ORIGIN[1] + CELL * (k // COLS)


def walk_scene(pm, n):
    """n items.  Item 0 is a Fill under everything.  Items 1 .. n - 3 are of every kind in turn, one per 4 x 4 cell, each over the
    pixel centres (1.5, 1.5) and (1.5, 2.5) of its cell or their mirror images, none over (0.5, 0.5).  Item n - 2, the last opaque
    one, is a Fill over exactly the window's first tile, left of the grid.  Item n - 1 is an alpha-0 compound Fill painted over
    everything: one band per grid row over the lower two pixel rows of the cells (and of the first tile), so that it is the top of
    half the pixels of every tile and skip_transparent changes those -- over ALL pixels it would leave no other item the top of
    anything without the skip, and the walk that ends at the first hit would end at once in every tile.  The first n // 2 items sit
    in a child group.  The window has a margin of nothing on the right and below."""
    assert n >= 8
    ox, oy = WALK_ORIGIN
    n_cells = n - 3
    rows = -(-n_cells // COLS)
    gw, gh = TILE + CELL * COLS, max(CELL * rows, TILE)
    rect = lambda x, y, w, h: np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], np.float64)  # noqa: E731
    kinds = ["fill"] + [WALK_KINDS[(i - 1) % len(WALK_KINDS)] for i in range(1, n - 2)] + ["fill", "compound"]

    def item(e, i):
        rgba = ((0x10305000 + (i << 8)) & 0xFFFFFF00) | (0x00 if i % 7 == 3 else 0xFF)
        if i == 0:
            e.fill(rect(ox, oy, gw, gh), 0x808080FF)
        elif i == n - 2:
            e.fill(rect(ox, oy, TILE, TILE), 0x204060FF)
        elif i == n - 1:
            e.fill_compound([rect(ox, oy + CELL * r + 2, gw, 2) for r in range(gh // CELL)], 0x11223300, even_odd=bool(n & 1))
        else:
            cx, cy = walk_cell(i)
            kind = kinds[i]
            if kind == "fill":
                e.fill(rect(cx + 1, cy + 1, 2, 2), rgba, even_odd=bool(i & 8))
            elif kind == "compound":
                hole = rect(cx + 1.25, cy + 1.25, 1.5, 1.5)
                e.fill_compound([rect(cx + 0.25, cy + 1, 3.5, 2), hole if i & 8 else hole[::-1]], rgba, even_odd=bool(i & 8))
            elif kind == "polyline":
                e.polyline(np.array([(cx + 1, cy + 1.5), (cx + 3, cy + 1.5), (cx + 3, cy + 2.5), (cx + 1, cy + 2.5)]), rgba, 0.5)
            elif kind == "line":
                e.stroke_line((cx + 1.5, cy + 0.75), (cx + 1.5, cy + 3.25), 0.5, rgba)
            elif kind == "circle":
                e.circle((cx + 2.0, cy + 2.0), 1.0)
            else:
                e.ellipse((cx + 2.0, cy + 2.0), 2.0, 1.0)

    half = n // 2

    def emit(e):
        e.begin_group(half)
        for i in range(half):
            item(e, i)
        e.end_group()
        for i in range(half, n):
            item(e, i)

    scene = hs._encode(pm, 1 + n - half, emit, cap=1 << 20)
    return Window(f"walk-{n}", scene, ox, oy, gw + 8, gh + 6, n=n, kinds=kinds)


_walks = {}


def walk_window(pm, n):
    if n not in _walks:
        _walks[n] = walk_scene(pm, n)
    return _walks[n]


# ---- part 4: long items, by chunks per round ------------------------------------------------------------------------------

STRIP_X0 = 90      # left of hit_structure.R0: the strip's first tile lies left of every stroke and keeps every chunk
STRIP_Y0 = 198     # across the strokes, about hit_structure.MID
STRIP_H = 4
_C = CHUNKS_PER_ROUND
LONG_CHUNKS = (_C - 1, _C, _C + 1, 2 * _C + 1)


def _long_builders():
    """[(id, builder(pm) -> hit_structure.Case, chunks wanted)].  Chunks = ceil(entries / 4).  The lead of 9 points puts the long
    item's first chunk at residue 3 of a super-chunk; a lead of 32 at residue 0."""
    out = []
    for chunks in LONG_CHUNKS:
        lead = 9 if chunks > _C else 32
        npt = 4 * chunks
        # 4 n + extras = npt with 0 <= extras <= 2 n.  At 0.25-pixel spacing four strokes pass between two pixel centres, so under
        # the even-odd rule a lost round shows only if it holds an odd number of counted strokes to the right of some centre: that
        # depends on where the seeded extra points fall, and test_no_round_is_blind says whether it does -- with one loop fewer in
        # the longest case it does in every round.
        loops = (npt - 24) // 4 - (3 if chunks > _C + 1 else 2)
        out.append((f"loops-{chunks}-eo", lambda pm, a=(loops, 0, lead, True, npt): hs.loops_scene(pm, *a), chunks))
        out.append((f"meander-{chunks}-nz", lambda pm, a=(loops, 0, lead, False, npt): hs.loops_scene(pm, *a), chunks))
        subs = (npt - 3) // 5         # 5 entries a sub-path, a sixth in some
        for eo in (False, True):
            out.append((f"comb-{chunks}-{'eo' if eo else 'nz'}", lambda pm, a=(subs, lead, eo, npt): hs.comb_scene(pm, a[0], a[1], a[2], entries=a[3]), chunks))
        spokes = 2 * chunks           # 4 chunks - 1 segments
        out.append((f"fan-{chunks}", lambda pm, a=(spokes, lead): hs.fan_scene(pm, *a), chunks))
    return out


LONG_BUILDERS = _long_builders()
LONG_IDS = [ident for ident, _, _ in LONG_BUILDERS]
_longs = {}


def long_window(pm, ident):
    """The Window of a long case; facts: the hit_structure.Case (`case`), the long item, the chunks wanted.  A Fill's strip runs from
    STRIP_X0 to a whole tile beyond the last stroke; the fan's starts at the tile that holds the fan's centre -- every segment's
    box has the centre as a corner -- and runs along its first spokes."""
    if ident not in _longs:
        build, chunks = next((b, c) for i, b, c in LONG_BUILDERS if i == ident)
        case = build(pm)
        if ident.startswith("fan"):
            rect = (int(hs.FAN_C[0]) - 2, int(hs.FAN_C[1]) - 2, STRIP_H, 26 * TILE)
        else:
            _, a, b, _ = hs._entries(bytes(case.scene), np_hit.flat_items(bytes(case.scene))[case.long_item][0])
            right = float(max(a[:, 0].max(), b[:, 0].max()))
            tiles = int(np.ceil((right + 25.0 - STRIP_X0) / TILE))   # (the trailing item ends 24 right of the strokes)
            rect = (STRIP_X0, STRIP_Y0, TILE * tiles, STRIP_H)
        _longs[ident] = Window(ident, case.scene, *rect, case=case, long_item=case.long_item, chunks=chunks)
    return _longs[ident]


def tile_extent(rect, tx, ty):
    """(xmin, xmax, ymin, ymax) of the pixel centres of tile (tx, ty) of a window, tightened to the window's edge."""
    x0, y0, w, h = rect
    return (x0 + TILE * tx + 0.5, x0 + min(TILE * (tx + 1), w) - 0.5, y0 + TILE * ty + 0.5, y0 + min(TILE * (ty + 1), h) - 0.5)


def tile_pass(con, boxes, ext):
    """bool [boxes]: pm_hit_frame.h's box test of the item's kind against a tile's extent (binary64 on float32 values)."""
    xmin, xmax, ymin, ymax = ext
    bb = np.asarray(boxes, np.float64)
    with np.errstate(invalid="ignore"):
        if con.fill:
            return (bb[:, 1] <= ymax) & (ymin < bb[:, 3]) & (bb[:, 2] >= xmin)
        hw = con.hw
        return (xmax >= bb[:, 0] - hw) & (xmin <= bb[:, 2] + hw) & (ymax >= bb[:, 1] - hw) & (ymin <= bb[:, 3] + hw)


def rounds_of_first_tile(wdw):
    """For the long item of a part-4 window, in the window's first tile: (chunks that survive the tile's cull, [chunk positions of
    each round], Contributions on the window's pixel centres).  Up to CHUNKS_PER_ROUND chunks: one round.  More: rounds of
    CHUNKS_PER_ROUND super-chunks, and of their survivors CHUNKS_PER_ROUND / SUPER_CHUNKS at a time."""
    base, chunk_bbox, sup_bbox = hs.index_model(wdw.scene)
    item = wdw.facts["long_item"]
    cb0, cb1 = int(base[item]), int(base[item + 1])
    con = hs.Contributions(wdw.scene, item, centres(*wdw.rect))
    ext = tile_extent(wdw.rect, 0, 0)
    keep = tile_pass(con, chunk_bbox[cb0:cb1], ext)
    n = cb1 - cb0
    if n <= CHUNKS_PER_ROUND:
        rounds = [np.flatnonzero(keep)]
    else:
        rounds = []
        g0, g1 = cb0 // hs.SUPER_CHUNKS, (cb1 - 1) // hs.SUPER_CHUNKS + 1
        per = CHUNKS_PER_ROUND // hs.SUPER_CHUNKS
        for gb in range(g0, g1, CHUNKS_PER_ROUND):
            g = np.arange(gb, min(gb + CHUNKS_PER_ROUND, g1))
            alive = g[tile_pass(con, sup_bbox[g], ext)]
            for sb in range(0, len(alive), per):
                c = (alive[sb : sb + per, None] * hs.SUPER_CHUNKS + np.arange(hs.SUPER_CHUNKS)).ravel()
                c = c[(c >= cb0) & (c < cb1)] - cb0
                rounds.append(c[keep[c]])
    return dict(cb0=cb0, cb1=cb1, keep=keep, rounds=rounds, con=con)


# ---- part 5: geometry on pixel centres ----------------------------------------------------------------------------------

CENTRES_RECT = (1, 2, 62, 45)


def centres_scene(pm):
    """Items: 0 a Fill with every vertex on a pixel centre, horizontal edges at y = j + 0.5 and vertical ones at x = k + 0.5 (an L
    shape: a.y <= y < b.y decides at both ends of every vertical edge); 1 a Fill with slanted edges through pixel centres and
    vertices on them; 2 an even-odd Fill that overlaps itself (a pentagram on half-integer vertices); 3 a compound Fill with a
    hole, all edges on centres; 4 a Polyline of width 1 along y = 30 and x = 40 -- the centres of the rows and columns next to it
    are at distance exactly hw --; 5 a Line of width 3 along y = 38: centres at y = 36.5 and 39.5 are at exactly hw; 6 a Circle
    whose box is 5 wide and 6 high (centre (50.5, 10), radius 2.5): the centres at (+-2, +-1.5) from its centre are ON the rim,
    4 + 2.25 = 6.25; 7 an ellipse.  (No pixel centre is exactly on an ellipse's rim: with the box's edges integers, dx / rx and
    dy / ry are fractions of opposite parity in numerator and denominator, and no two such squares sum to 1 -- a Pythagorean
    triple has an odd leg over its odd hypotenuse.  The ellipse here has centres within 2 % of the rim on either side.)"""
    L = np.array([[3.5, 4.5], [15.5, 4.5], [15.5, 9.5], [9.5, 9.5], [9.5, 16.5], [3.5, 16.5]])
    slant = np.array([[20.5, 4.5], [30.5, 4.5], [36.5, 10.5], [30.5, 16.5], [20.5, 16.5], [26.5, 10.5]])
    star = np.array([[12.5 + np.round(2 * 9 * np.sin(4 * np.pi * k / 5)) / 2, 34.5 - np.round(2 * 9 * np.cos(4 * np.pi * k / 5)) / 2] for k in range(5)])
    outer = np.array([[20.5, 20.5], [34.5, 20.5], [34.5, 27.5], [20.5, 27.5]])
    hole = np.array([[24.5, 22.5], [24.5, 25.5], [30.5, 25.5], [30.5, 22.5]])

    def emit(e):
        e.fill(L, 0x336699FF)
        e.fill(slant, 0x884400FF)
        e.fill(star, 0x9900CCFF, even_odd=True)
        e.fill_compound([outer, hole], 0x2244CCFF)
        e.polyline(np.array([[22.0, 30.0], [40.0, 30.0], [40.0, 44.0]]), 0x11AA22FF, 1.0)
        e.stroke_line((4.0, 38.0), (20.0, 38.0), 3.0, 0x000000FF)
        e.circle((50.5, 10.0), 2.5)
        e.ellipse((52.0, 25.0), 6.0, 3.0)

    return hs._encode(pm, 8, emit)


_centres = {}


def centres_window(pm):
    if not _centres:
        _centres["w"] = Window("centres", centres_scene(pm), *CENTRES_RECT)
    return _centres["w"]


def centre_classes(scene, rect):
    """{class name: how many pixel centres of the window are in it}, from the scene's own numbers."""
    sc = bytes(scene)
    q = centres(*rect).astype(np.float64)
    x, y = q[:, 0, None], q[:, 1, None]
    out = dict(vertex=0, horizontal=0, vertical=0, slanted=0, lower_end=0, upper_end=0, poly_hw=0, line_hw=0, circle_rim=0)
    for at, box in np_hit.flat_items(sc):
        tag, flags = hs._item_header(sc, at)
        if tag == np_hit.FILL:
            a, b = np_hit.fill_segments(np_hit._points(sc, at), bool(flags & np_hit.FILL_COMPOUND))
            ax, ay, bx, by = a[None, :, 0], a[None, :, 1], b[None, :, 0], b[None, :, 1]
            out["vertex"] += int(((x == ax) & (y == ay)).any(axis=1).sum())
            s = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
            within = (np.minimum(ax, bx) <= x) & (x <= np.maximum(ax, bx)) & (np.minimum(ay, by) <= y) & (y <= np.maximum(ay, by))
            on = (s == 0) & within
            out["horizontal"] += int((on & (ay == by)).any(axis=1).sum())
            out["vertical"] += int((on & (ax == bx)).any(axis=1).sum())
            out["slanted"] += int((on & (ax != bx) & (ay != by)).any(axis=1).sum())
            # a.y <= y < b.y at its two ends, for centres left of a non-horizontal segment (where it would count)
            left = x < np.minimum(ax, bx)
            out["lower_end"] += int((left & (ay != by) & (y == np.minimum(ay, by))).any(axis=1).sum())
            out["upper_end"] += int((left & (ay != by) & (y == np.maximum(ay, by))).any(axis=1).sum())
        elif tag in (np_hit.LINE, np_hit.POLY):
            a, b, hw = np_hit.stroke_segments(sc, at, tag)
            abx, aby = b[None, :, 0] - a[None, :, 0], b[None, :, 1] - a[None, :, 1]
            t = np.clip(((x - a[None, :, 0]) * abx + (y - a[None, :, 1]) * aby) / (abx * abx + aby * aby), 0.0, 1.0)
            d2 = (x - (a[None, :, 0] + abx * t)) ** 2 + (y - (a[None, :, 1] + aby * t)) ** 2
            out["poly_hw" if tag == np_hit.POLY else "line_hw"] += int((d2 == hw * hw).any(axis=1).sum())
        elif tag == np_hit.CIRCLE and not flags:
            word = int(np.frombuffer(sc, np.uint32, 1, at)[0])
            if not word & np_hit.CIRCLE_ELLIPSE:
                cx, cy = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
                r = min(cx - box[0], cy - box[1])
                out["circle_rim"] += int(((x[:, 0] - cx) ** 2 + (y[:, 0] - cy) ** 2 == r * r).sum())
    return out
