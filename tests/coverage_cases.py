"""Scenes and pixel windows for coverage counts, pm_item_coverage (decision D28; test helper, not a conftest): tests/test_coverage.py
runs them against tests/np_coverage.py under the emulation and on the GPU, and checks on the CPU that no case is blind.

The kernel (piet_metal_amd/csrc/pm_coverage.h) walks a 16 x 16 tile as pm_hit_frame_kernel does -- the windows, the walk scenes and
the long items are tests/hit_frame_cases.py's, imported as they are -- and adds to that walk a table in LDS with a row per survivor
of a step, ITEMS_PER_STEP rows, which is flushed into the items' records once per step.  What is new here:

  occlusion_scene    every class of item -- Fills of alpha 255, 254 and 0, a Circle, a Line, a Polyline -- below AND above an opaque
                     item that overlaps it, in a 50 x 37 window, which is also the window the additivity test cuts in four;
  dense_scene        n items that ALL survive the cull of one 16 x 16 tile: with n = ITEMS_PER_STEP the first step fills the table
                     to its last row, with n = ITEMS_PER_STEP + 1 the item at the bottom is alone in a second step;
  lid_scene          one opaque Fill over a 128 x 128 window, 64 tiles that all add to one record, on top of items nobody sees.

expected() is np_coverage on the window, computed once per (case, skip, visible_only)."""
from __future__ import annotations

import struct

import numpy as np

import hit_frame_cases as fc
import hit_structure as hs
import np_coverage
import np_hit
import np_stack

NONE = np_coverage.HIT_NONE
TILE = fc.TILE
ITEMS_PER_STEP = fc.ITEMS_PER_STEP


class Case:
    """A scene and a pixel rectangle of it."""

    def __init__(self, ident, scene, rect, **facts):
        self.ident, self.scene, self.rect, self.facts = ident, scene, tuple(rect), facts
        self._members, self._want = {}, {}

    def __repr__(self):
        return f"{self.ident} {self.rect}"

    def members(self, skip=False):
        if skip not in self._members:
            H = np_coverage.members(self.scene, self.rect, skip)
            H.setflags(write=False)
            self._members[skip] = H
        return self._members[skip]

    def expected(self, skip=False, visible_only=False):
        """np_coverage.DTYPE [n_items]; shared by the tests, never written to."""
        key = (skip, visible_only)
        if key not in self._want:
            want = np_coverage.coverage(self.scene, self.rect, skip, visible_only, H=self.members(skip))
            want.setflags(write=False)
            self._want[key] = want
        return self._want[key]


_cases = {}


def of_window(wdw):
    """The Case of a hit_frame_cases.Window (one per window: the expectation is shared)."""
    if wdw.ident not in _cases:
        _cases[wdw.ident] = Case(wdw.ident, wdw.scene, wdw.rect, **wdw.facts)
    return _cases[wdw.ident]


def _rect(x, y, w, h):
    return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], np.float64)


# ---- occlusion ---------------------------------------------------------------------------------------------------------------

OCCLUSION_RECT = (5, 7, 50, 37)
OCCLUSION_CLASSES = ("fill255", "fill254", "fill0", "circle", "line", "polyline")
OCCLUSION_CUTS = (23, 19)   # the additivity test cuts the window at these offsets: no multiple of 16


def occlusion_scene(pm):
    """13 items.  0 .. 5 are one of every class, 6 is an opaque Fill over the middle of them, 7 .. 11 one of every other class again
    (the opaque Fill 6 stands for its own), and 12 is a small opaque Fill on top of those.  Colours are 0xRRGGBBAA."""
    def emit(e):
        e.fill(_rect(6, 8, 46, 34), 0x202020FF)                                                     # 0  fill255, under everything
        e.fill(_rect(8, 10, 24, 16), 0x804020FE)                                                    # 1  fill254
        e.fill(_rect(12, 12, 26, 20), 0x11223300)                                                   # 2  fill0
        e.circle((22.0, 22.0), 6.0)                                                                 # 3  circle
        e.stroke_line((8.0, 30.0), (46.0, 13.0), 3.0, 0x3050A0FF)                                   # 4  line, opaque
        e.polyline(np.array([[10.0, 14.0], [30.0, 34.0], [48.0, 20.0]]), 0x50A030FE, 2.5)           # 5  polyline, alpha 254
        e.fill(_rect(16, 14, 20, 14), 0xA0A0A0FF)                                                   # 6  fill255: the occluder
        e.fill(_rect(10, 18, 20, 16), 0x4080C0FE)                                                   # 7  fill254
        e.fill(_rect(22, 9, 20, 14), 0x99887700)                                                    # 8  fill0
        e.ellipse((34.0, 24.0), 7.0, 4.0)                                                           # 9  circle (an ellipse)
        e.stroke_line((12.0, 16.0), (44.0, 30.0), 2.0, 0xC04040FE)                                  # 10 line, alpha 254
        e.polyline(np.array([[14.0, 32.0], [26.0, 16.0], [40.0, 28.0]]), 0x209020FF, 3.0)           # 11 polyline, opaque
        e.fill(_rect(24, 18, 8, 8), 0xF0F000FF)                                                     # 12 fill255, on top

    return hs._encode(pm, 13, emit)


def occlusion_case(pm):
    if "occlusion" not in _cases:
        _cases["occlusion"] = Case("occlusion", occlusion_scene(pm), OCCLUSION_RECT)
    return _cases["occlusion"]


# hit_frame_cases' windows lie where its scenes have little on top of each other: most of them hold no pixel that is in two items.  The
# same sizes again over the middle of the occlusion scene, at an origin that is no multiple of 16
OCCLUSION_WINDOWS = {f"occlusion-{w}x{h}": (11, 15, w, h) for w, h in fc.SIZES}


def occlusion_window(pm, ident):
    if ident not in _cases:
        _cases[ident] = Case(ident, occlusion_case(pm).scene, OCCLUSION_WINDOWS[ident])
    return _cases[ident]


def item_classes(scene):
    """[class name] per item in flat paint order, OCCLUSION_CLASSES' names ("fill<alpha>", "line", "polyline", "circle")."""
    sc = bytes(scene)
    alpha, _ = np_stack.item_alphas(sc)
    out = []
    for i, (at, _) in enumerate(np_hit.flat_items(sc)):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        out.append({np_hit.CIRCLE: "circle", np_hit.LINE: "line", np_hit.POLY: "polyline"}.get(tag, f"fill{int(alpha[i])}"))
    return out


def quarters(rect, cuts):
    """The four disjoint windows a window falls into when cut at (cx, cy) from its origin."""
    x0, y0, w, h = rect
    cx, cy = cuts
    return [(x0, y0, cx, cy), (x0 + cx, y0, w - cx, cy), (x0, y0 + cy, cx, h - cy), (x0 + cx, y0 + cy, w - cx, h - cy)]


# ---- a full table --------------------------------------------------------------------------------------------------------------

DENSE_RECT = (19, 35, TILE, TILE)            # one tile, at no multiple of 16
DENSE_SIZES = (ITEMS_PER_STEP, ITEMS_PER_STEP + 1)


def dense_scene(pm, n):
    """n items, all inside the window's one tile.  Item 0 is an opaque Fill over the tile's left 12 columns.  Item i >= 1 sits at pixel
    (k % 16, k // 16), k = n - 1 - i, of the tile and reaches 1 .. 3 pixels right and 1 .. 2 down, so that the items' counts differ --
    a row of the table flushed into the wrong record shows -- and some lie wholly under the opaque item above them; kind and alpha go
    round with i."""
    x0, y0 = DENSE_RECT[:2]

    def emit(e):
        e.fill(_rect(x0, y0, 12, TILE), 0x303030FF)
        for i in range(1, n):
            k = n - 1 - i    # (the item above, i + 1, sits one pixel to the left and reaches over this one's)
            cx, cy = x0 + k % TILE, y0 + (k // TILE) % TILE
            w, h = 1 + i % 3, 1 + i % 2
            rgba = ((0x20406000 + (i << 10)) & 0xFFFFFF00) | (0xFF, 0xFE, 0x00, 0xFF, 0x80)[i % 5]
            kind = i % 7
            if kind == 3:
                e.circle((cx + 1.0, cy + 1.0), 1.0)
            elif kind == 5:
                e.stroke_line((cx + 0.25, cy + 0.5), (cx + w - 0.25, cy + 0.5), 1.0, rgba)
            elif kind == 6:
                e.polyline(np.array([(cx + 0.25, cy + 0.5), (cx + w - 0.25, cy + 0.5), (cx + w - 0.25, cy + h - 0.5)]), rgba, 0.75)
            else:
                e.fill(_rect(cx, cy, w, h), rgba, even_odd=bool(i & 8))

    return hs._encode(pm, n, emit, cap=1 << 20)


def dense_case(pm, n):
    key = f"dense-{n}"
    if key not in _cases:
        _cases[key] = Case(key, dense_scene(pm, n), DENSE_RECT, n=n)
    return _cases[key]


def step_survivors(scene, rect, tx=0, ty=0, skip=False):
    """[survivors of each step] for tile (tx, ty) of a window: pm_hit_frame.h's item cull against the tile's extent, restated on the
    items' u16 boxes (a saturated edge bounds nothing; a Line is never culled; a Fill is kept when it lies to the right)."""
    sc = bytes(scene)
    xmin, xmax, ymin, ymax = fc.tile_extent(rect, tx, ty)
    alpha, coloured = np_stack.item_alphas(sc)
    keep = []
    for i, (at, (x0, y0, x1, y1)) in enumerate(np_hit.flat_items(sc)):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        if tag == np_hit.CIRCLE:
            keep.append(not (ymax < y0 or ymin > y1 or xmax < x0 or xmin > x1))
            continue
        above, below = y0 != 0 and ymax < y0, y1 != 0xFFFF and ymin > y1
        left, right = x0 != 0 and xmax < x0, x1 != 0xFFFF and xmin > x1
        gone = skip and coloured[i] and alpha[i] == 0
        culled = {np_hit.LINE: False, np_hit.FILL: above or below or right, np_hit.POLY: above or below or left or right}[tag]
        keep.append(not culled and not gone)
    keep = np.array(keep[::-1])    # topmost first
    return [int(keep[s : s + ITEMS_PER_STEP].sum()) for s in range(0, len(keep), ITEMS_PER_STEP)]


# ---- many tiles, one record -------------------------------------------------------------------------------------------------------

LID_RECT = (3, 5, 128, 128)


def lid_scene(pm):
    """Five items nobody sees -- a Fill of alpha 254, a Circle, a Line, a Polyline, an opaque Fill -- under one opaque Fill that covers
    the window and a margin around it."""
    x0, y0, w, h = LID_RECT

    def emit(e):
        e.fill(_rect(x0 + 10, y0 + 20, 90, 70), 0x4080C0FE)
        e.circle((x0 + 64.0, y0 + 64.0), 30.0)
        e.stroke_line((x0 + 4.0, y0 + 120.0), (x0 + 124.0, y0 + 6.0), 5.0, 0x3050A0FF)
        e.polyline(np.array([[x0 + 8.0, y0 + 8.0], [x0 + 100.0, y0 + 40.0], [x0 + 30.0, y0 + 110.0]]), 0x50A030FE, 4.0)
        e.fill(_rect(x0 + 40, y0 + 40, 60, 60), 0x101010FF)
        e.fill(_rect(x0 - 2, y0 - 3, w + 6, h + 5), 0xE0E0E0FF)

    return hs._encode(pm, 6, emit)


def lid_case(pm):
    if "lid" not in _cases:
        _cases["lid"] = Case("lid", lid_scene(pm), LID_RECT)
    return _cases["lid"]


# ---- more tiles than workgroups ---------------------------------------------------------------------------------------------------

STRIP_RECT = (0, 3, 65536, 2)      # 4096 tiles of 16 x 2 pixels
GRID_MAX = 8 * 256                 # the launch's grid on an MI355X (and on the emulated device): eight workgroups on each of 256 CUs


def strip_scene(pm):
    """A window as wide as pixels exist and two rows high: twice as many tiles as the grid has workgroups, so every workgroup walks
    tile b and then tile b + 2048 and its LDS table serves two tiles.  Both tiles of workgroup 0 hold hits -- a Circle in each, of
    different sizes, a translucent Line through every tile, and an opaque Fill and an alpha-0 Fill over the second --, so what the
    first tile leaves behind in the table shows in the second's records; the last tile holds an opaque Fill of its own."""
    def emit(e):
        e.fill(_rect(100, 0, 39900, 10), 0x406080FF)
        e.stroke_line((10.0, 4.0), (65000.0, 4.5), 2.0, 0x3050A0FE)
        e.circle((8.0, 4.0), 3.0)
        e.circle((32776.0, 4.0), 5.0)
        e.fill(_rect(32700, 0, 100, 10), 0x11223300)
        e.fill(_rect(65520, 3, 30, 1), 0xE0E0E0FF)

    return hs._encode(pm, 6, emit)


def strip_case(pm):
    if "strip" not in _cases:
        _cases["strip"] = Case("strip", strip_scene(pm), STRIP_RECT)
    return _cases["strip"]


# ---- the Tiger -------------------------------------------------------------------------------------------------------------------

TIGER_VIEW = (240, 135)
