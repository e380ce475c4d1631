"""The scenes and request lists of tests/test_crossings.py (decision D29), the smallest shapes at which pm_crossings_kernel can go
wrong.  Test infrastructure; the scenes are built through measure_cases._build, so an entry may patch its points afterwards.

  hand    what can be checked by hand, every group in a place of its own so that within 2^-4 of a crossing no third edge lies: two
          Polylines in an X, a Line through a square Fill, a T-junction of two Lines, two Polylines with a shared end, Lines that
          share their start or their end, parallel and collinear Lines, a figure-8 Polyline, a bow-tie Fill, a compound Fill whose
          sub-paths cross (separators in the index range), two crossing Lines, a Circle, a one-point Polyline, a transparent Line across an opaque Polyline, a Polyline with a NaN point
          beside crossing segments and a Line through it, and edges whose boxes touch in one coordinate;
  lanes   one long Line and zigzag Polylines of ZIG segments, each crossed by the Line in every segment: 1, 4, 5 (a chunk and its
          edge), 255, 256 (64 chunks: a chunk per lane), 257 (65: the super-chunk path) and 300 (more than 64 crossings on ONE edge of
          A and more than 64 surviving chunks: two rounds, the ranks carry); the same zigzags as A (more than 64 values of i); a
          second zigzag of 257 shifted by half a period (crossings over many i AND many j); a star Fill of 261 edges against itself;
  limit   two Polylines of 16 385 segments (their product exceeds 2^28), two of 16 384 far apart in y, and a Line through one of them.
"""
import numpy as np

import bounds_cases as bc
import measure_cases as mc

F32 = np.float32
OPAQUE, CLEAR = mc.OPAQUE, mc.CLEAR
NAN = np.nan
ZIG = (1, 4, 5, 255, 256, 257, 300)
STAR = 261
BIG = 16385

_scenes = {}


def P(*pts):
    return np.array(pts, np.float64)


def hand_scene(pm):
    poly = lambda *pts: (lambda e: e.polyline(P(*pts), OPAQUE, 1.0))  # noqa: E731
    line = lambda a, b, rgba=OPAQUE: (lambda e: e.stroke_line(a, b, 1.0, rgba))  # noqa: E731
    entries = [
        ("x_up", poly((0, 0), (10, 10))),                                             # 0, 1: an X, crossing at (5, 5), t = u = 1/2
        ("x_down", poly((0, 10), (10, 0))),
        ("square", lambda e: e.fill(bc.sq(20, 0, 30, 10), OPAQUE)),                   # 2, 3: a Line through a square: two crossings
        ("through", line((15.0, 5.0), (35.0, 5.0))),
        ("t_bar", line((40.0, 0.0), (50.0, 0.0))),                                    # 4, 5: a T-junction at (45, 0): counts, u = 0
        ("t_stem", line((45.0, 0.0), (45.0, 10.0))),
        ("v_left", poly((60, 0), (65, 5))),                                           # 6, 7: a shared end: none
        ("v_right", poly((65, 5), (70, 0))),
        ("par_a", line((0.0, 20.0), (10.0, 20.0))),                                   # 8, 9: parallel: none
        ("par_b", line((0.0, 22.0), (10.0, 22.0))),
        ("col_a", line((20.0, 20.0), (30.0, 20.0))),                                  # 10, 11: collinear, overlapping: none
        ("col_b", line((25.0, 20.0), (35.0, 20.0))),
        ("eight", poly((0, 40), (10, 50), (10, 40), (0, 50))),                        # 12: segments 0 and 2 cross at (5, 45)
        ("bow_tie", lambda e: e.fill(P((20, 40), (30, 50), (30, 40), (20, 50)), OPAQUE)),   # 13: edges 0 and 2 cross at (25, 45)
        ("compound", lambda e: e.fill_compound([bc.sq(40, 40, 50, 50), P((45, 45), (60, 45), (45, 60))], OPAQUE)),   # 14: (50, 45) and (45, 50)
        ("line_up", line((60.0, 20.0), (70.0, 30.0))),                                # 15, 16: a Line against a Line, at (65, 25)
        ("line_down", line((60.0, 30.0), (70.0, 20.0))),
        ("circle", lambda e: e.circle((80.0, 80.0), 5.0)),                            # 17
        ("one_point", poly((80, 80), (81, 81)), ("npt", 1)),                          # 18
        ("opaque", poly((0, 100), (10, 110))),                                        # 19, 20: crossing at (5, 105) unless the flag skips 20
        ("clear", line((0.0, 110.0), (10.0, 100.0), CLEAR)),
        ("nan_poly", poly((0, 60), (10, 70), (5, 65), (10, 60), (0, 70)), ("points", 2, [[NAN, 65]])),   # 21: segments 0 and 3 cross at (5, 65); 1 and 2 are no edges
        ("nan_line", line((0.0, 62.0), (10.0, 62.0))),                                # 22: crosses segments 0 and 3 of 21
        ("touch_e", poly((0, 80), (10, 90))),                                         # 23: its box ends at x = 10
        ("touch_hit", line((10.0, 85.0), (10.0, 95.0))),                              # 24: on that side, through e's end: t = 1, u = 1/2
        ("touch_miss", line((10.0, 84.0), (20.0, 84.0))),                             # 25: an end on that side, the boxes touch, no crossing
        ("fan_a", line((80.0, 0.0), (90.0, 10.0))),                                   # 26, 27: the same start and nothing else in common: none
        ("fan_b", line((80.0, 0.0), (90.0, 5.0))),
        ("fan_c", line((80.0, 20.0), (90.0, 30.0))),                                  # 28, 29: the same end: none
        ("fan_d", line((85.0, 20.0), (90.0, 30.0))),
    ]
    return mc._build(pm, "crossings-hand", entries)


def zig_points(n_segs, x0=1.0):
    k = np.arange(n_segs + 1)
    return np.stack([x0 + 2.0 * k, 10.0 + 20.0 * (k % 2)], axis=1)


def star_points(n=STAR, cx=300.0, cy=120.0, r=110.0):
    """The star polygon {n / 2}: every edge crosses its two neighbours' neighbours.  The long Line passes through its top, the zigzags'
    band through its upper part: most of its 66 chunks are culled for any one edge, a few are not."""
    k = (2 * np.arange(n)) % n
    return np.stack([cx + r * np.cos(2 * np.pi * k / n), cy + r * np.sin(2 * np.pi * k / n)], axis=1)


def lanes_scene(pm):
    entries = [("lead", lambda e: e.fill(bc.sq(700, 0, 710, 10), OPAQUE)),             # (a chunk in front: the zigzags' first chunks sit at odd places in their super-chunks)
               ("long_line", lambda e: e.stroke_line((0.0, 20.25), (640.0, 20.25), 1.0, OPAQUE))]
    for n in ZIG:
        entries.append((f"zig-{n}", (lambda n: lambda e: e.polyline(zig_points(n), OPAQUE, 1.0))(n)))
    entries.append(("zig-shifted", lambda e: e.polyline(zig_points(257, 2.0), OPAQUE, 1.0)))
    entries.append(("star", lambda e: e.fill(star_points(), OPAQUE)))
    return mc._build(pm, "crossings-lanes", entries)


def big_points(n_segs, y0):
    k = np.arange(n_segs + 1)
    return np.stack([0.03125 * k, y0 + (k % 2)], axis=1)


def limit_scene(pm):
    """The pair of 16 384 is kept far apart: their boxes do not meet, so the 2^28 index pairs are never walked."""
    entries = [
        ("big_a", lambda e: e.polyline(big_points(BIG, 10.0), OPAQUE, 1.0)),
        ("big_b", lambda e: e.polyline(big_points(BIG, 10.5), OPAQUE, 1.0)),
        ("most_a", lambda e: e.polyline(big_points(BIG - 1, 100.0), OPAQUE, 1.0)),
        ("most_far", lambda e: e.polyline(big_points(BIG - 1, 1000.0), OPAQUE, 1.0)),
        ("cut", lambda e: e.stroke_line((100.0, 100.25), (101.0, 100.75), 1.0, OPAQUE)),
    ]
    return mc._build(pm, "crossings-limit", entries, cap=1 << 20)


SCENES = ("hand", "lanes", "limit")


def scene_of(pm, name):
    if name not in _scenes:
        _scenes[name] = {"hand": hand_scene, "lanes": lanes_scene, "limit": limit_scene}[name](pm)
    return _scenes[name]


def names(pm, name):
    scene_of(pm, name)
    return mc.NAMES["crossings-" + name]


def pairs(pm, name):
    """The (item_a, item_b) of the scene's requests."""
    N = names(pm, name)
    n = len(N)
    if name == "hand":      # every ordered pair, every item against itself, and the indices beyond the scene on either side
        out = [(a, b) for a in range(n) for b in range(n)]
        return out + [(0, n), (n, 0), (n, n), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)]
    if name == "lanes":
        L, S = N["long_line"], N["zig-shifted"]
        out = []
        for z in ZIG:
            out += [(L, N[f"zig-{z}"]), (N[f"zig-{z}"], L), (N[f"zig-{z}"], N[f"zig-{z}"])]
        out += [(N["zig-300"], S), (S, N["zig-300"]), (N["zig-257"], S), (S, N["zig-5"]), (N["zig-4"], S), (S, S), (N["star"], N["star"]), (L, N["star"]),
                (N["star"], L), (N["lead"], N["star"]), (L, L)]
        return out
    A, B, M, F, C = (N[k] for k in ("big_a", "big_b", "most_a", "most_far", "cut"))
    return [(A, B), (B, A), (A, A), (A, M), (M, A), (M, F), (F, M), (C, M), (M, C), (C, A), (C, F)]


def layout_requests(pm):
    """On `lanes`: (requests (item_a, item_b, first, cap), out_cap).  The Line against zig-300 answers 300 records: caps below, at and
    above that, 0, and around what a round of 64 lanes holds; firsts the caller chose, out of order, with gaps; a request that runs
    into out_cap, one at out_cap, one at 0xFFFFFFFF."""
    N = names(pm, "lanes")
    L, Z, S = N["long_line"], N["zig-300"], N["zig-shifted"]
    caps = [0, 1, 299, 300, 301, 63, 64, 65, 255, 256, 257]
    out_cap = 4000
    order = [7, 2, 9, 0, 5, 10, 3, 8, 1, 6, 4]
    firsts, at = {}, 3
    for k in order:
        firsts[k] = at
        at += caps[k] + 2
    reqs = [(L, Z, firsts[k], cap) for k, cap in enumerate(caps)]
    assert at < out_cap - 400
    reqs += [(Z, L, out_cap - 10, 9),(L, Z, out_cap, 5), (Z, S, 0xFFFFFFFF, 7), (Z, S, at, 100), (S, Z, out_cap - 1, 0xFFFFFFFF), (L, Z, at + 150, 0)]
    return reqs, out_cap
