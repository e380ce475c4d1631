"""Dashed path sets for the edges of decision D15 (test infrastructure): a seeded grammar whose dash ends land ON vertices, on the
64-segment steps of the kernels' walk and on the ends of the walk; a counter of the event classes a case contains, which uses
tests/np_dash.py alone (never the library); and a table of hand-made extremes for what a random draw reaches rarely or never.

    dash_case(seed)       -> (PathSet, width_scale); drawn under the identity, inside VIEW x VIEW pixels
    subpaths_of(ps)       -> [(path, f32 points [n, 2], closed, pattern or None, offset)] of a set of MoveTo / LineTo / ClosePath
    classes_of(case)      -> per dashed sub-path the set of CLASSES it contains
    is_cut(case)          -> per dashed sub-path: it is cut into at least one dash (not undashed, whole-cover or empty)
    SEEDS                 -> the committed seed list (tests/test_dash_edges.py states what it must contain)
    EXTREMES              -> name -> builder of an Extreme

Every coordinate of the grammar is a multiple of 1/8 and every step is axis-aligned or a 3-4-5 vector, so the segment lengths are
exact on D15's 2^-16 grid; pattern values and offsets are multiples of 1/8 (or prefix sums, or G, or T itself), so "a dash ends
exactly at this vertex" is an event with a probability, not a coincidence.  SECOND_VIEW keeps that: (3, 4, -4, 3) / 4 is a rotation
times 5/4 in exact binary arithmetic, and 1.25 is the width_scale that goes with it."""
from dataclasses import dataclass

import numpy as np

import np_dash
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE, style_bits

M, L, Z = 0, 1, 4
FILL, STROKE = 1, 2
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
VIEW = 608                                            # the grammar's walks stay inside [40, 568]^2
SECOND_VIEW = ((0.75, 1.0, -1.0, 0.75, 600.0, 0.0), 1.25)  # (affine, width_scale)
ONE = 65536

STEPS = [(1, 0), (-1, 0), (0, 1), (0, -1), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3), (0, 0)]
POINT_COUNTS = [2, 3, 5, 9, 63, 64, 65, 66, 129, 130]
PATTERN_COUNTS = [1, 2, 3, 4, 6, 32]
BIG_OFFSETS = [1e9, -1e9, 1e30, -3e38, 12345.625]

CLASSES = (
    "start on a vertex", "end on a vertex", "zero-length dash", "zero-length dash on a vertex", "boundary on a repeated vertex",
    "abutting dashes", "interval at G", "starts at 0", "ends at T", "open across a step", "boundary at a step", "merged",
    "merged at equality", "one side reaches the start", "whole-cover", "whole-cover at equality", "empty item", "undashed: G == 0",
    "undashed: every gap 0", "undashed: T == 0", "phi == 0 from an offset", "negative offset",
)


# ---- the grammar ---------------------------------------------------------------------------------------------

def _walk_points(rng, n, closed):
    pts = [(300.0, 300.0)]
    dot = n <= 3 and rng.random() < 0.3  # a walk of no length
    while len(pts) < n:
        dx, dy = (0, 0) if dot else STEPS[int(rng.integers(0, len(STEPS)))]
        k = int(rng.integers(1, 17)) / 8.0
        x, y = pts[-1][0] + dx * k, pts[-1][1] + dy * k
        if 40.0 <= x <= 568.0 and 40.0 <= y <= 568.0:
            pts.append((x, y))
    if closed and n >= 3 and rng.random() < 0.7:  # an axis-aligned way home: the closing segment's length is exact too
        pts[-1] = (pts[-2][0], 300.0)
    return pts


def _pattern(rng, T_px, step_px, ws):
    """(values, offset or None): step_px is where the kernels' second 64-segment step begins (None: the walk has one step)."""
    c = PATTERN_COUNTS[int(rng.integers(0, len(PATTERN_COUNTS)))]
    v = [int(rng.integers(0, 33)) / 8.0 for _ in range(c)]
    v = [0.0 if rng.random() < 0.3 else x for x in v]  # (without the forced zeros no seed has an interval at G)
    how = rng.random()
    if c >= 2 and how < 0.15:
        v[-2:] = [0.0, 0.0]
    elif c >= 2 and how < 0.25:
        v[:2] = [0.0, 0.0]
    fit = rng.random()
    if fit < 0.25 and T_px > 0:  # an on-interval made to measure: the walk's length, or a little more or less
        want = (T_px + [0.0, 0.0, 0.125, -0.125, 3.0][int(rng.integers(0, 5))]) / ws
        if want > 0 and float(np.float32(want)) == want:
            v[0] = want
            if c >= 2 and v[1] == 0.0:
                v[1] = 0.5
    elif fit < 0.32 and T_px > 0:  # a first gap longer than the walk, behind a dash that ends where the walk begins: no dash at all
        v = [int(rng.integers(0, 9)) / 8.0, (T_px + int(rng.integers(0, 9)) / 8.0) / ws]
        return v, v[0]
    elif fit < 0.6 and step_px:  # a dash that ends, begins or is a dot exactly where the second step begins
        want = step_px / ws
        if float(np.float32(want)) == want:
            how = int(rng.integers(0, 3))
            if how == 0:
                v[0] = want
                return v + [1.0] * (c == 1), 0.0
            v = [float(rng.integers(0, 2)) * v[0], max(v[-1], 0.5)] if how == 1 else v
            return v, -want
    return v, None


def _offset(rng, v):
    full = v + v if len(v) % 2 else v
    pick = int(rng.integers(0, 8))
    if pick == 0:
        return 0.0
    if pick == 1:
        return float(sum(full)) * (1 if rng.random() < 0.5 else -1)
    if pick in (2, 3):
        return float(sum(full[: int(rng.integers(0, len(full) + 1))])) * (1 if rng.random() < 0.5 else -1)
    if pick in (4, 5):
        return int(rng.integers(-40, 41)) / 8.0
    if pick == 6:
        return BIG_OFFSETS[int(rng.integers(0, len(BIG_OFFSETS)))]
    return float(sum(full)) * int(rng.integers(2, 5)) + float(sum(full[: int(rng.integers(0, len(full) + 1))]))


def make_pathset(paths):
    """paths: (elements, flags, width, pattern or None, offset)."""
    from path_sets import pathset

    ps = pathset(*[(els, flags, width) for els, flags, width, _, _ in paths])
    for k, (_, _, _, pattern, offset) in enumerate(paths):
        if pattern is not None:
            ps = ps.with_dashes(pattern, offset, select=[k])
    return ps


def dash_case(seed):
    rng = np.random.default_rng(seed * 7919 + 15)
    ws = [1.0, 2.0, 0.5][int(rng.integers(0, 3))]
    paths = []
    for _ in range(int(rng.integers(1, 7))):
        n = POINT_COUNTS[int(rng.integers(0, len(POINT_COUNTS)))]
        closed = bool(rng.random() < 0.45)
        pts = _walk_points(rng, n, closed)
        els = [(M, *pts[0])] + [(L, *p) for p in pts[1:]] + ([(Z,)] if closed else [])
        Q = np_dash.walk(pts, closed)[1]
        pattern, offset = _pattern(rng, int(Q[-1]) / ONE, int(Q[64]) / ONE if len(Q) >= 66 else None, ws)
        if offset is None:
            offset = _offset(rng, pattern)
        cap, join = [BUTT, ROUND_CAP, SQUARE][int(rng.integers(0, 3))], [MITER, ROUND_JOIN, BEVEL][int(rng.integers(0, 3))]
        width = [0.5, 2.0, 5.0][int(rng.integers(0, 3))]
        paths.append((els, STROKE | style_bits(cap, join), width, pattern, offset))
    return make_pathset(paths), ws


# ---- what a case contains, by np_dash alone ------------------------------------------------------------------------

def subpaths_of(ps):
    table = {int(d["path"]): ([float(v) for v in ps.dash_values[int(d["first"]) : int(d["first"]) + int(d["count"])]], float(d["offset"]))
             for d in ps.dashes}
    out = []
    for ip, p in enumerate(ps.paths):
        if not int(p["flags"]) & STROKE:
            continue
        cur = None
        subs = []
        for k in range(int(p["el_begin"]), int(p["el_end"])):
            tag = int(ps.els["tag"][k])
            if tag == M:
                cur = [[tuple(ps.els["p"][k][:2])], False]
                subs.append(cur)
            elif tag == L:
                cur[0].append(tuple(ps.els["p"][k][:2]))
                cur[1] = False
            elif tag == Z:
                cur[1] = True
            else:
                raise ValueError("subpaths_of reads MoveTo, LineTo and ClosePath")
        pattern, offset = table.get(ip, (None, 0.0))
        out += [(ip, np.asarray(pts, np.float32), closed, pattern, offset) for pts, closed in subs]
    return out


def _classes(pts, closed, pattern, offset, ws):
    pf, G, phi = np_dash.pattern_fixed(pattern, offset, ws)
    W, Q = np_dash.walk(pts, closed)
    Q = [int(q) for q in Q]
    T, N = Q[-1], len(Q)
    gaps = any(pf[j + 1] - pf[j] for j in range(1, len(pf) - 1, 2))
    found = set()
    if G == 0:
        found.add("undashed: G == 0")
    elif not gaps:
        found.add("undashed: every gap 0")
    elif T == 0:
        found.add("undashed: T == 0")
    polys = np_dash.cut(pts, closed, pattern, offset, ws)
    if G == 0 or not gaps or T == 0:
        assert polys == np_dash.UNDASHED
        return found, False
    with np.errstate(over="ignore"):
        wo = np.float32(offset) * np.float32(ws)
    if wo < 0:
        found.add("negative offset")
    if wo != 0 and phi == 0:
        found.add("phi == 0 from an offset")
    # D15's on-intervals, one by one
    spans, r = [], 0
    while r * G - phi < T:
        spans += [(r * G + pf[j] - phi, r * G + pf[j + 1] - phi, pf[j] == G) for j in range(0, len(pf) - 1, 2)]
        r += 1
    whole = [(A, B) for A, B, _ in spans if closed and A <= 0 and B >= T]
    if whole:
        assert polys == np_dash.CLOSED_WHOLE
        found.add("whole-cover")
        if any(A == 0 or B == T for A, B in whole):
            found.add("whole-cover at equality")
        return found, False
    D = [(A, B, at_G) for A, B, at_G in spans if max(A, 0) < min(B, T) or (A == B and 0 <= A < T)]
    if not D:
        assert polys == []
        found.add("empty item")
        return found, False
    at, repeated = set(Q), {Q[k] for k in range(N - 1) if Q[k] == Q[k + 1]}
    steps = [Q[i] for i in (64, 128) if i <= N - 2]  # Q[i] begins a later step of the kernels' walk
    for A, B, at_G in D:
        if 0 < A < T and A in at:
            found.add("start on a vertex")
        if B > A and 0 < B < T and B in at:
            found.add("end on a vertex")
        if A == B:
            found.add("zero-length dash")
            if A in at:
                found.add("zero-length dash on a vertex")
            if at_G:
                found.add("interval at G")
        if (0 <= A <= T and A in repeated) or (0 <= B <= T and B in repeated):
            found.add("boundary on a repeated vertex")
        if A == 0:
            found.add("starts at 0")
        if B == T:
            found.add("ends at T")
        for s in steps:
            if A < s < B:
                found.add("open across a step")
            if A == s or B == s:
                found.add("boundary at a step")
    if any(D[k][1] == D[k + 1][0] for k in range(len(D) - 1)):
        found.add("abutting dashes")
    n_polys = len(D)
    if closed:
        first, last = D[0][0] <= 0 < D[0][1], D[-1][0] < T <= D[-1][1]
        if first and last and len(D) >= 2:
            n_polys -= 1
            found.add("merged")
            if D[0][0] == 0 or D[-1][1] == T:
                found.add("merged at equality")
        elif first != last:
            found.add("one side reaches the start")
    assert len(polys) == n_polys, (len(polys), n_polys)
    return found, True


def classes_of(case):
    ps, ws = case
    return [_classes(pts, closed, pattern, offset, ws)[0] for _, pts, closed, pattern, offset in subpaths_of(ps) if pattern is not None]


def is_cut(case):
    ps, ws = case
    return [_classes(pts, closed, pattern, offset, ws)[1] for _, pts, closed, pattern, offset in subpaths_of(ps) if pattern is not None]


# The committed seeds: tests/test_dash_edges.py::test_committed_dash_seeds_are_not_a_thin_sample states what they must contain.
SEEDS = list(range(100))


# ---- the extremes ----------------------------------------------------------------------------------------------

@dataclass
class Extreme:
    ps: object
    scale: float = 1.0
    affine: tuple = IDENTITY
    view: tuple = None        # (width, height) if the scene lies in a small viewport: render and hit checks too
    saturates: str = None     # "pattern" / "every pattern value" / "segment" / "offset": what must reach its cap, by np_dash alone
    min_dashes: int = 0       # the poly-lines np_dash cuts the scene's strokes into, at least


def _line(x0, y0, x1, y1):
    return [(M, x0, y0), (L, x1, y1)]


def _square(x, y, s):
    return [(M, x, y), (L, x + s, y), (L, x + s, y + s), (L, x, y + s), (Z,)]


def _tiny(pattern, cap):
    e = 1.0 / 64
    return Extreme(make_pathset([([(M, 300, 300), (L, 300 + e, 300), (L, 300 + e, 300 + e)], STROKE | style_bits(cap, MITER), 2.0, pattern, 0.0)]),
                   view=(320, 320), min_dashes=1024)


def _rounding():
    u = 2.0 ** -16
    pats = [[u / 4, 0.25], [0.25, u / 4], [u / 2, 0.25], [0.25, u / 2], [u / 4, u / 4], [u * 0.75, u * 1.25]]
    ends = [14.0] * 5 + [10.0 + 1.0 / 64]  # (the last pattern is [1, 1] in units: 512 dashes on 1/64 px)
    return Extreme(make_pathset([(_line(10, 10 + 8 * k, x1, 10 + 8 * k), STROKE | style_bits(ROUND_CAP, MITER), 3.0, p, 0.0)
                                 for k, (p, x1) in enumerate(zip(pats, ends))]), view=(32, 64), min_dashes=16 + 16 + 16 + 512)


def _long_segments():
    open_ = [(M, 10, 20), (L, 70010, 20), (L, 70010, 60), (L, 69990, 60)]
    closed = [(M, 10, 100), (L, 70010, 100), (L, 70010, 140), (Z,)]
    return Extreme(make_pathset([(open_, STROKE | style_bits(SQUARE, MITER), 4.0, [30000, 20000, 10, 5], 7.0),
                                 (closed, STROKE | style_bits(ROUND_CAP, ROUND_JOIN), 4.0, [30000, 20000], 25000.0)]), saturates="segment", min_dashes=4)


def _long_value():
    z = [(M, 10, 10), (L, 60, 10), (L, 60, 40), (L, 110, 40)]
    return Extreme(make_pathset([(z, STROKE | style_bits(BUTT, BEVEL), 3.0, [70000, 5], 65530.0),
                                 ([(M, 10, 60), (L, 60, 60), (L, 60, 90), (Z,)], STROKE | style_bits(ROUND_CAP, MITER), 3.0, [70000, 5], 65500.0)]),
                   view=(128, 112), saturates="pattern", min_dashes=3)


def _long_value_by_scale():
    z = [(M, 0.1, 0.1), (L, 0.6, 0.1), (L, 0.6, 0.4), (L, 1.1, 0.4)]
    return Extreme(make_pathset([(z, STROKE | style_bits(SQUARE, ROUND_JOIN), 0.03, [700, 0.05], 655.3)]), scale=100.0, affine=(100.0, 0.0, 0.0, 100.0, 0.0, 0.0),
                   view=(128, 64), saturates="pattern", min_dashes=2)


def _every_value_long():
    return Extreme(make_pathset([(_line(10, 10 + 10 * k, 110, 10 + 10 * k), STROKE | style_bits(SQUARE, MITER), 3.0, [70000.0] * 32, off)
                                 for k, off in enumerate([131052.0, 65506.0, 0.0, -30.0, 65536.0 * 31 + 50])]), view=(128, 64),
                   saturates="every pattern value", min_dashes=4)


def _offset_overflow():
    return Extreme(make_pathset([(_line(10, 10 + 10 * k, 110, 10 + 10 * k), STROKE | style_bits(BUTT, MITER), 3.0, [3, 2, 1], off)
                                 for k, off in enumerate([3e38, -3e38])]), scale=2.0, view=(128, 32), saturates="offset", min_dashes=20)


def _many_subpaths():
    els = []
    for k in range(300):
        x, y = 10.0 + 19 * (k % 20), 10.0 + 20 * (k // 20)
        kind = k % 5
        if kind == 0:
            els += [(M, x, y)]
        elif kind == 1:
            els += [(M, x, y), (Z,)]
        elif kind == 2:
            els += [(M, x, y), (L, x + 12, y + 2), (L, x + 5, y + 14), (Z,)]
        elif kind == 3:
            els += [(M, x, y), (L, x + 12, y + 9)]
        else:
            els += [(M, x, y), (L, x, y), (L, x + 12, y), (L, x + 12, y), (L, x + 12, y + 12.5)]
    return Extreme(make_pathset([(els, STROKE | style_bits(ROUND_CAP, BEVEL), 2.0, [3, 2, 0, 2], 1.0)]), view=(400, 320), min_dashes=300)


def _many_paths():
    paths = []
    for k in range(200):
        x, y = 8.0 + 19 * (k % 20), 8.0 + 20 * (k // 20)
        els = [(M, x, y), (L, x + 13, y + 3), (L, x + 4, y + 13)] + ([(Z,)] if k % 3 == 0 else [])
        kind = k % 4
        style = style_bits([BUTT, ROUND_CAP, SQUARE][k % 3], [MITER, ROUND_JOIN, BEVEL][(k // 3) % 3])
        if kind == 0:
            paths.append((els, STROKE | style, 2.0, [2.5, 1.5, 0, 1][: 2 + 2 * (k % 8 == 0)], 0.25 * (k % 7)))
        elif kind == 1:
            paths.append((els, STROKE | style, 2.0, None, 0.0))
        elif kind == 2:
            paths.append((els, STROKE, 2.0, None, 0.0))
        else:
            paths.append((els, FILL, 2.0, None, 0.0))
    return Extreme(make_pathset(paths), view=(400, 224), min_dashes=150)


def _empty(which):
    empty = (_line(10, 50, 60, 50), STROKE | style_bits(ROUND_CAP, ROUND_JOIN), 4.0, [5, 100], 5.0)
    drawn = lambda y: (_line(10, y, 60, y + 5), STROKE | style_bits(SQUARE, MITER), 4.0, [6, 3], 0.0)  # noqa: E731
    if which == "alone":
        paths = [empty]
    elif which == "between":
        paths = [drawn(20), empty, (_square(70, 20, 20), FILL, 1.0, None, 0.0), empty, drawn(80)]
    else:  # a closed one: [-5, 0] ends where the walk begins and [100, 105] begins where it ends
        paths = [(_square(10, 10, 25), STROKE | style_bits(ROUND_CAP, ROUND_JOIN), 4.0, [5, 100], 5.0), drawn(60)]
    return Extreme(make_pathset(paths), view=(112, 96))


def _whole_cover(side):
    """Squares of perimeter 160: the covering interval meets T (or 0) exactly, beside one that misses it by 1/8 px."""
    sq = lambda k: _square(10 + 60 * k, 10, 40)  # noqa: E731
    st = STROKE | style_bits(ROUND_CAP, MITER)
    if side == "B":
        rows = [(sq(0), st, 4.0, [170, 5], 10.0), (sq(1), st, 4.0, [169.875, 5], 10.0), (sq(2), st, 4.0, [160, 5], 0.0)]
    else:
        rows = [(sq(0), st, 4.0, [170, 5], 0.0), (sq(1), st, 4.0, [5, 0.125, 170, 5], 5.125), (sq(2), st, 4.0, [5, 0.125, 170, 5], 5.0),
                (sq(3), st, 4.0, [5, 170], 175.0)]
    return Extreme(make_pathset(rows), view=(256, 64), min_dashes=1)


def _hairline():
    rows = [([(M, 10, 20), (L, 40, 12), (L, 44, 40), (L, 60, 14)], STROKE | style_bits(ROUND_CAP, ROUND_JOIN), 6.0, [8, 4], 0.0),
            (_square(70, 10, 30), STROKE | style_bits(SQUARE, BEVEL), 6.0, [6, 3, 2], 1.5),
            ([(M, 10, 60), (L, 10, 60), (L, 50, 60), (L, 50, 60), (L, 90, 75)], STROKE | style_bits(BUTT, MITER), 6.0, [0, 6], -4.0)]
    return Extreme(make_pathset(rows), scale=0.01, view=(112, 96), min_dashes=2000)


EXTREMES = {
    "pattern_of_two_units": lambda: _tiny([2.0 ** -16, 2.0 ** -16], ROUND_CAP),
    "dots_one_unit_apart": lambda: _tiny([0.0, 2.0 ** -16], SQUARE),
    "values_that_round_to_0_and_to_1": _rounding,
    "segments_beyond_65536_px": _long_segments,
    "pattern_value_beyond_65536_px": _long_value,
    "pattern_value_beyond_65536_px_by_width_scale": _long_value_by_scale,
    "all_32_values_beyond_65536_px": _every_value_long,
    "offset_overflows_f32_under_width_scale": _offset_overflow,
    "three_hundred_subpaths_in_a_path": _many_subpaths,
    "two_hundred_paths_of_four_kinds": _many_paths,
    "empty_item_alone": lambda: _empty("alone"),
    "empty_item_between_drawn_items": lambda: _empty("between"),
    "empty_item_closed": lambda: _empty("closed"),
    "whole_cover_ends_at_T": lambda: _whole_cover("B"),
    "whole_cover_starts_at_0": lambda: _whole_cover("A"),
    "hairline_width_scale": _hairline,
}
