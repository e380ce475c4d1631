"""Scenes built from the frame path's own constants (tests/test_frame_structure.py uses them; nothing here needs a GPU).

Part A: 48 x 48 views whose action is in tile (1, 1) -- pixels [16, 32) x [16, 32) -- so that the tile's command list, its
candidates and its fragments have exactly the sizes the kernels of pm_fine_tile.h, pm_coarse_tile.h and pm_bin_rows.h are built
around.  Part B: one item whose winding or segment count per tile goes to the limits of the packed per-(candidate, tile) word
`backdrop << kCtShift | relevant segments`.

A scene is a list of ops for test_host_cpu.encode_ops.  Items are translucent, so every command shows in the pixels and no opaque
Solid cuts a list short.  The constants below are checked against the headers by test_frame_structure.py."""
import numpy as np

TILE = 16
SP_CHUNK = 64            # pm_fine_tile.h kSpChunk
MAX_FRAG = 64            # kMaxFrag
FILL_PAIRS_MIN = 9       # kFillPairsMin
ALPHA_SLOTS = 16         # kAlphaSlots
DENSE_LDS_CHUNKS = 2     # kDenseLdsChunks
LDS_CHUNKS = 3           # pm_coarse_tile.h kLdsChunks
WAVE_CANDS = 64          # kWaveCands
CT_SHIFT = 20            # pm_device.h kCtShift
RECORD_CANDS = 256       # pm_bin_rows.h: candidates per record (64 x the waves of a binning workgroup)
RECORD_CANDS_ONE_WAVE = 64
HEAVY_STREAM, HEAVY_STREAM_LONE, VHEAVY_STREAM = 72, 40, 112   # pm_context.hip: defaults of the PM_HEAVY_* switches
MAX_WINDING = (1 << (31 - CT_SHIFT)) - 1                      # 2047: what the signed upper field of the word holds
MAX_TILE_SEGS = (1 << CT_SHIFT) - 1

END, CIRCLE, LINE, FILL, STROKE, FILL_EDGE, DRAW_FILL, SOLID, BAIL = range(1, 10)

VIEW = (48, 48)
CORNER_VIEW = (40, 40)   # tile (1, 1) is then a partial tile at the viewport's corner
TX = TY = 1

_COLOURS = (0x2040C0B0, 0xC0402070, 0x30A05090, 0x8020D060, 0xD0B01050)


def colour(i):
    return _COLOURS[i % len(_COLOURS)]


# ---- one-, two- and four-command items inside tile (1, 1) -----------------------------------------------------------

def circle(i, tx=TX, ty=TY):
    """One command."""
    return ("circle", 16.0 * tx + 3.0 + (i % 10), 16.0 * ty + 3.0 + (i // 10) % 10, 1.0 + 0.5 * (i % 3))


def line(i, tx=TX, ty=TY):
    """A thin translucent line: Line + Stroke."""
    x, y = 16.0 * tx, 16.0 * ty
    return ("line", x + 1.5 + (i * 5) % 13, y + 1.25 + i % 3, x + 14.5 - (i * 3) % 11, y + 14.25 - i % 4, 0.5, colour(i))


def triangle(i, tx=TX, ty=TY):
    """A small fill wholly inside the tile: three Fills + DrawFill."""
    c = np.array([16.0 * tx + 3.0 + i % 9, 16.0 * ty + 3.0 + (i // 9) % 9])
    return ("fill_eo" if i % 5 == 4 else "fill", c + np.array([[-1.5, -1.25], [2.25, -0.5], [0.25, 2.0]]), colour(i))


def small_item(i):
    return (circle, line, triangle)[i % 3](i)


# ---- A1: lists of exactly L commands (the End included, as pmo.Ptcl.count counts) --------------------------------------

LADDER = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300)
COMPOSITIONS = ("circles", "lines", "fills")


def ladder(composition, L):
    n = L - 1
    if composition == "circles":
        return [circle(i) for i in range(n)]
    if composition == "lines":
        return [line(i) for i in range(n // 2)] + [circle(i) for i in range(n % 2)]
    assert composition == "fills"
    return [triangle(i) for i in range(n // 4)] + [circle(i) for i in range(n % 4)]


# ---- A2: one long item --------------------------------------------------------------------------------------------

def zigzag_points(n, tx=TX, ty=TY):
    """A closed outline of n segments (n points), every one of them inside the tile: a slanted quad, then a zigzag between the
    tile's top and bottom from left to right, closed from its last point to the quad's first.  The zigzag's lobes have both
    orientations and lie over the quad, so windings 0, 1 and 2 all occur and the two fill rules differ."""
    assert n >= 8
    m = n - 4
    i = np.arange(m, dtype=np.float64)
    x = 1.5 + 13.0 * i / (m - 1)
    top = 0.75 + 0.5 * ((i * 7) % 11) / 11.0
    bot = 15.25 - 0.5 * ((i * 5) % 13) / 13.0
    y = np.where(i % 2 == 0, top, bot)
    quad = np.array([[1.0, 1.25], [15.0, 1.5], [14.75, 15.0], [1.25, 14.5]])
    return np.concatenate([quad, np.stack([x, y], axis=1)]) + (16.0 * tx, 16.0 * ty)


def sliver_subpaths(n, tx=TX, ty=TY):
    """A compound outline of n segments: thin slivers over the tile's height, three segments each (the last one 3 + n % 3)."""
    k = n // 3
    subs = []
    for j in range(k):
        x = 1.0 + 13.5 * j / k
        pts = [[x, 1.2 + 0.1 * (j % 3)], [x + 0.15, 14.6], [x + 0.3, 1.4]]
        if j == k - 1:
            pts += [[x + 0.25, 1.0], [x + 0.1, 0.8]][: n % 3]
        subs.append(np.array(pts) + (16.0 * tx, 16.0 * ty))
    return subs


LONG_KINDS = ("fill", "fill_eo", "poly", "slivers")


def long_item(kind, n, k=0):
    """One item with n relevant segments in tile (1, 1): n Fill (Line) commands and the closing DrawFill (Stroke)."""
    if kind in ("fill", "fill_eo"):
        return (kind, zigzag_points(n), colour(k))
    if kind == "poly":
        # the zigzag of an outline five segments longer, open: n steep segments.  (Not the quad's sides and the closing segment: the
        # reference tests a Polyline's segment against the tile row of the lane that looks at it, quirk Q4, and drops a shallow
        # one that the tile row above does not see.)
        return ("poly", zigzag_points(n + 5)[4:], colour(k + 1), 0.3)
    assert kind == "slivers"
    return ("fill_cp", sliver_subpaths(n), colour(k + 2))


TRAILER = ("line", 17.5, 30.0, 30.5, 18.0, 0.75, 0x10E02080)   # shows that signedArea and df were reset after the blend

# (chunk boundaries at list positions 64, 128, 192; with lead 0..3 the closing command lands on 62..66, 126..130, 190..194 and all around)
LONG_N = tuple(range(56, 72)) + tuple(range(120, 136)) + tuple(range(184, 200)) + (255, 256, 257, 300)
LEADS = (0, 1, 2, 3)


def cut_item(kind, lead, n, trailer=True):
    return [circle(i) for i in range(lead)] + [long_item(kind, n)] + ([TRAILER] if trailer else [])


# both copies of carry_sa / carry_df in turn: long items back to back, and one over three chunks (positions 3 .. 139)
BACK_TO_BACK = ((2, (60, 70)), (0, (62, 66)), (1, (100, 100)), (3, (136,)), (1, (63, 63, 63)), (61, (200, 9)))


def back_to_back(kind, lead, ns):
    kinds = LONG_KINDS if kind == "mixed" else (kind,)
    return [circle(i) for i in range(lead)] + [long_item(kinds[k % len(kinds)], n, k) for k, n in enumerate(ns)] + [TRAILER]


# passes of CoarseTile by their stream elements (relevant segments, or 1 for a one-command item): one candidate of exactly 64, 65,
# 256, 257 (kPar: 65..256 go over the four waves), and several candidates that sum to the same
PASSES = {
    "one-64": (64,), "one-65": (65,), "one-256": (256,), "one-257": (257,),
    "sum-64": (16, 16, 16, 16), "sum-65": (16, 16, 16, 17), "sum-256": (64, 64, 64, 64), "sum-257": (64, 64, 64, 65),
    "sum-64-ones": (30, 1, 32, 1), "sum-65-ones": (1, 30, 1, 33), "sum-256-ones": (1, 127, 127, 1), "sum-257-ones": (128, 1, 128),
}


def pass_scene(name, kind="fill"):
    return [circle(k) if n == 1 else long_item(kind, n, k) for k, n in enumerate(PASSES[name])]


# ---- A3: candidates -----------------------------------------------------------------------------------------------

CAND_COUNTS = (63, 64, 65, 128, 129, 256, 257)


def around(i):
    """A candidate whose box covers tile (1, 1) and whose segments do not reach it: an L around the tile, as a Polyline or as a
    thin Fill.  It passes the box cull, emits nothing in the tile and leaves its backdrop 0."""
    d = 0.25 * (i % 4)
    if i % 4 < 2:
        return ("poly", np.array([[8.0 - d, 6.0 + d], [8.5 - d, 40.0 + d], [42.0, 40.5 + d]]), colour(i), 1.0)
    return ("fill_eo" if i % 4 == 3 else "fill",
            np.array([[6.0 - d, 6.0], [6.5, 42.0 + d], [42.0, 42.5], [42.0, 40.5], [8.0 + d, 40.0], [8.5, 6.5]]), colour(i))


def candidates(n, silent=None):
    """n candidates reach the tile.  silent None: all emit; 0 or 1: every second one, from that index on, emits nothing (so the
    last of a pass of 64 is silent with 1, the first of the next with 0)."""
    return [around(i) if silent is not None and i % 2 == silent else small_item(i) for i in range(n)]


def emitting(n, silent):
    return n if silent is None else sum(1 for i in range(n) if i % 2 != silent)


def strip_row(before, own=6, after=3):
    """`before` candidates of the strip row that stay out of tile (1, 1) -- they lie in tile (2, 1) --, then `own` items of the
    tile, then `after` more of tile (2, 1): with before = record - 3 the tile's own candidates straddle two binning records."""
    other = lambda i: (circle, line)[i % 2](i, tx=2)  # noqa: E731
    return [other(i) for i in range(before)] + [small_item(i) for i in range(own)] + [other(i) for i in range(after)]


# ---- A4: fragments --------------------------------------------------------------------------------------------------

TALL_COUNTS = (3, 4, 5, 8, 9, 10, 16, 17, 63, 64, 65)


def tall(i, t):
    """A fill with ONE segment in tile (1, 1), live on all its 16 rows: the left side of a quadrilateral that starts above the
    tile, ends below it and closes to the right of it."""
    x = 17.0 + 13.0 * i / t
    return ("fill_eo" if i % 4 == 3 else "fill", np.array([[x, 12.0], [x + 0.7, 36.5], [40.5, 36.0], [40.0, 12.5]]), colour(i))


def talls(t):
    return [tall(i, t) for i in range(t)]


def tall_zigzag(t, rule="fill"):
    """ONE fill with t tall segments in tile (1, 1), from above the tile to below it and back; closed through tile column 0."""
    i = np.arange(t + 1, dtype=np.float64)
    x = 17.5 + 13.0 * i / t
    y = np.where(i % 2 == 0, 12.0 - 0.25 * (i % 3), 36.0 + 0.25 * (i % 5))
    pts = np.stack([x, y], axis=1)
    tail = [[44.0, 44.0], [4.0, 44.5], [3.5, 11.0]] if t % 2 else [[44.0, 8.0], [3.5, 7.0]]
    return (rule, np.concatenate([pts, np.array(tail)]), colour(t))


def mixed_tall_short(t):
    out = []
    for i in range(t):
        out += [tall(i, t), triangle(i)] + ([line(i)] if i % 3 == 0 else [])
    return out


ALPHA_ITEMS = (ALPHA_SLOTS - 1, ALPHA_SLOTS, ALPHA_SLOTS + 1, 2 * ALPHA_SLOTS + 1)


def few_command_items(n):
    return [(triangle, line, triangle)[i % 3](i) for i in range(n)]


def a_scenes(thin=False):
    """name -> (ops, (w, h)): every scene of part A.  thin: fewer steps on the ladders (for the emulated run), the same edges."""
    out = {}
    for comp in COMPOSITIONS:
        for L in LADDER:
            if thin and comp != "circles" and L in (2, 127, 191, 255, 300):
                continue
            out[f"ladder-{comp}-{L}"] = (ladder(comp, L), VIEW)
    out["ladder-lines-129-corner"] = (ladder("lines", 129), CORNER_VIEW)
    for kind in LONG_KINDS:
        for n in LONG_N:
            for lead in LEADS:
                pos = lead + n
                if thin and not (lead == pos % 4 and (pos % SP_CHUNK in (62, 63, 0, 1, 2) or n >= 255)):
                    continue
                out[f"cut-{kind}-l{lead}-n{n}"] = (cut_item(kind, lead, n), VIEW)
        for k, (lead, ns) in enumerate(BACK_TO_BACK):
            out[f"pair-{kind}-l{lead}-" + "-".join(map(str, ns))] = (back_to_back(kind, lead, ns), VIEW)
        out[f"cut-{kind}-l1-n127-corner"] = (cut_item(kind, 1, 127), CORNER_VIEW)
    out["pair-mixed-l2-70-58-64-66"] = (back_to_back("mixed", 2, (70, 58, 64, 66)), VIEW)
    for name in PASSES:
        for kind in ("fill", "poly"):
            out[f"pass-{kind}-{name}"] = (pass_scene(name, kind), VIEW)
    for n in CAND_COUNTS:
        for silent in (None, 0, 1):
            out[f"cands-{n}-" + ("all" if silent is None else f"silent{silent}")] = (candidates(n, silent), VIEW)
    for rec in (RECORD_CANDS, RECORD_CANDS_ONE_WAVE):
        for d in (-4, -3, -2):
            out[f"strip-{rec}{d}"] = (strip_row(rec + d), VIEW)
    for t in TALL_COUNTS:
        out[f"talls-{t}"] = (talls(t), VIEW)
    for t in (63, 64, 65, 128):
        out[f"tall-zigzag-{t}"] = ([tall_zigzag(t, "fill_eo" if t == 65 else "fill"), TRAILER], VIEW)
    out["tall-zigzag-64-lead1"] = ([circle(0), tall_zigzag(64), TRAILER], VIEW)
    out["talls-17-corner"] = (talls(17), CORNER_VIEW)
    for t in (5, 12):
        out[f"mixed-tall-short-{t}"] = (mixed_tall_short(t), VIEW)
    for n in ALPHA_ITEMS:
        out[f"alpha-items-{n}"] = (few_command_items(n), VIEW)
    return out


def a_family(name):
    return name.split("-")[0]


# ---- B: the packed counter ------------------------------------------------------------------------------------------

TURNS = (41, 255, 256, 1023, 1024, 2046, 2047)
TURNS_VIEW = (64, 64)


DOUBLED = (12.0, 11.0)   # here the quad's lower left corner lies just above a tile row: see turns_ops


def quad(x0=4.0, y0=5.0):
    """The slanted quad of edge_scenes' winding_numbers (its first one, where it stands there)."""
    return np.array([[x0, y0], [x0 + 35.5, y0 + 2.25], [x0 + 38.0, y0 + 40.5], [x0 + 3.25, y0 + 37.0]])


def turns_ops(turns, flip=False, rule="fill", rgba=0x2040C0B0, at=None):
    """The quad walked `turns` times.  at=DOUBLED: the tile row below the lower left corner sees both the left and the lower side
    start at or above its top edge, and the reference counts both into its backdrop: twice the winding, in the tiles of that row."""
    q = quad(*at) if at else quad()
    return [(rule, np.concatenate([q[::-1] if flip else q] * turns), rgba)]


BEYOND_VIEW = (96, 96)   # tile columns and rows 4, 5 are outside the quad's box


def beyond_ops(turns):
    """The quad walked `turns` times, and items in the tiles its box does not touch."""
    rest = [f(i, tx, ty) for i, (tx, ty) in enumerate([(4, 0), (5, 1), (4, 4), (5, 5), (0, 4), (1, 5), (4, 2), (2, 5)]) for f in (circle, line, triangle)]
    return rest[:12] + turns_ops(turns) + rest[12:]


STAIR_LEVELS = 16
STAIR_VIEW = (768, 96)   # three strips of 16 tiles


def staircase_loops(per, peak_less=0, reverse=False, aligned=False):
    """16 nested quads, level k 16 px further in on the left and on the right (2 px at the top and the bottom), walked `per`
    times each (the innermost `per - peak_less`): the winding rises level by level across the first strip of 16 tiles, stays
    high over the second, whose tiles see the rising sides only as backdrop, and falls in the third.  aligned: the sides are
    vertical and lie on tile edges exactly; else they are slanted and lie inside tiles.  -> [(quad, loops)]"""
    w, h = STAIR_VIEW
    out = []
    for k in range(STAIR_LEVELS):
        if aligned:
            xl, xr = 16.0 * (k + 1), w - 16.0 * (k + 1)
            q = np.array([[xl, 5.0 + 2 * k], [xr, 6.25 + 2 * k], [xr, h - 6.5 - 2 * k], [xl, h - 5.0 - 2 * k]])
        else:
            xl, xr = 9.0 + 16.0 * k, w - 7.5 - 16.0 * k
            q = np.array([[xl, 5.0 + 2 * k], [xr - 2.5, 6.25 + 2 * k], [xr, h - 6.5 - 2 * k], [xl + 3.25, h - 5.0 - 2 * k]])
        out.append((q[::-1] if reverse else q, per - (peak_less if k == STAIR_LEVELS - 1 else 0)))
    return out


def staircase_ops(per, peak_less=0, reverse=False, aligned=False, rule="fill"):
    # (a compound fill, a sub-path per level: in one outline the walks from level to level would add edges of their own)
    return [("fill_cp_eo" if rule == "fill_eo" else "fill_cp", [np.concatenate([q] * n) for q, n in staircase_loops(per, peak_less, reverse, aligned)], 0x3060B0A0)]


STAIRS = {   # name -> (per, peak_less, reverse, aligned, rule); the peak is 16 * per - peak_less
    "per127-nz": (127, 0, False, False, "fill"),
    "per127-eo-aligned": (127, 0, False, True, "fill_eo"),
    "peak2047-nz-aligned": (128, 1, False, True, "fill"),
    "peak2047-eo": (128, 1, False, False, "fill_eo"),
    "peak-2047-nz": (128, 1, True, False, "fill"),
    "peak-2047-eo-aligned": (128, 1, True, True, "fill_eo"),
}


def stair_peak(name):
    per, less, reverse, _, _ = STAIRS[name]
    return (-1 if reverse else 1) * (STAIR_LEVELS * per - less)


MANY_SEGS = (65535, 65536, 70000)


def many_segs_ops(n, rule="fill"):
    return [circle(0), (rule, zigzag_points(n), 0x2040C0B0), TRAILER]


# ---- numpy: what a scene's name says, from its points -------------------------------------------------------------

def outlines(op):
    """The closed sub-paths of a fill op, as float32 points (what the scene holds)."""
    subs = op[1] if op[0].startswith("fill_cp") else [op[1]]
    return [np.asarray(s, np.float64).astype(np.float32).astype(np.float64) for s in subs]


def winding_at_tile_corners(op, w, h):
    """The winding number of a fill op's outline around every tile's top-left corner, int64 [tiles_y, tiles_x]: the backdrop of
    the tile's DrawFill up to sign.  Corners on the outline are not handled (the scenes here keep them off, but for the aligned
    staircase, where only tiles strictly between the sides are looked at)."""
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    cx = (np.arange(tiles_x) * TILE).astype(np.float64)[None, :, None]
    cy = (np.arange(tiles_y) * TILE).astype(np.float64)[:, None, None]
    total = np.zeros((tiles_y, tiles_x), np.int64)
    for p in outlines(op):
        a, b = p, np.roll(p, -1, axis=0)
        uniq, counts = np.unique(np.concatenate([a, b], axis=1), axis=0, return_counts=True)   # (a loop walked n times: each edge once, n-fold)
        ax, ay, bx, by = (uniq[:, k][None, None, :] for k in range(4))
        up = (ay <= cy) & (by > cy)
        down = (by <= cy) & (ay > cy)
        with np.errstate(all="ignore"):
            xi = ax + (cy - ay) * (bx - ax) / (by - ay)
        left = xi < cx
        total += ((up & left).astype(np.int64) * counts - (down & left).astype(np.int64) * counts).sum(axis=2)
    return total


def segments_inside_tile(op, tx=TX, ty=TY):
    """How many segments of a fill op's outline lie wholly inside the open tile (each is then one relevant segment of it)."""
    n = 0
    for p in outlines(op):
        a, b = p, np.roll(p, -1, axis=0)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        n += int(((lo[:, 0] > TILE * tx) & (hi[:, 0] < TILE * tx + TILE) & (lo[:, 1] > TILE * ty) & (hi[:, 1] < TILE * ty + TILE)
                  & ((a != b).any(axis=1))).sum())
    return n
