"""Scenes for hit stacks (decision D24) whose items differ in ALPHA (test helper, not a conftest).  hit_structure.walk_scene only has
alphas 0 and 255 and cannot tell "opaque" from "not transparent"; stack_scene takes an alpha per item, from ALPHAS.

n items (n <= 130) of the five kinds in rotation -- Fill, Polyline, Line, Circle (an ellipse every other time round), compound Fill --,
item i along its own ray from the common point C into the right half plane, the first n // 2 in a child group:

  * every item contains C: a Line and a Polyline end there, a Fill is a kite around it, a compound Fill has a square around it, a
    Circle is a petal -- its centre 400 along the ray, radius 402;
  * every item has a private spot that no other item contains: 820 along its ray, beyond every Circle; a Circle's is at its far side;
  * a Circle has no colour and is always opaque, and one item in five is a Circle: at C the first opaque member is never deeper than
    the topmost Circle, so C alone cannot put it at 63 or nowhere.  Hence a second common point A, left of C and outside every
    Circle, that every Fill, Polyline and compound Fill reaches too (the Polyline starts there, the Fills have a square around it,
    the plain Fill's at the end of a there-and-back spur) and no Line and no Circle does: three items in five, whose alphas alone
    decide where the stack at A ends.

CASES puts the first opaque member of A's stack (no skip flag) at POSITIONS 0, 1, 63, 64 and 65 of the stack -- where a list of k = 64
is full --, at the ITEMS 63, 64 and 65 below the top one -- the two sides of the walk's 64-item step, and one more -- and nowhere; at
C it is at 0 (an alpha of 255 on top) or at the topmost Circle.  tests/test_hit_stack.py checks these claims with tests/np_stack.py
before it uses the scenes."""
import numpy as np

import hit_structure as hs

ALPHAS = (0, 1, 128, 254, 255)
KINDS = ("fill", "polyline", "line", "circle", "compound")
C = (1000.0, 1000.0)
A = (960.0, 1000.0)
NOTHING = (100.0, 100.0)
N_MAX = 130


def kind_of(i):
    k = KINDS[i % 5]
    return "ellipse" if k == "circle" and (i // 5) % 2 else k


def reaches_a(i):
    return KINDS[i % 5] in ("fill", "polyline", "compound")


def stack_scene(pm, alphas):
    """The scene for one alpha per item; queries: the n spots, C, A, NOTHING and a point with a NaN."""
    n = len(alphas)
    assert 1 <= n <= N_MAX and all(a in ALPHAS for a in alphas)
    half = n // 2
    c, a_pt = np.array(C), np.array(A)
    sq = lambda p, s: np.array([[p[0] - s, p[1] - s], [p[0] + s, p[1] - s], [p[0] + s, p[1] + s], [p[0] - s, p[1] + s]])  # noqa: E731
    spots = []

    def item(e, i):
        kind = kind_of(i)
        rgba = ((0x10305000 + (i << 8)) & 0xFFFFFF00) | int(alphas[i])
        th = np.deg2rad(-80.0 + 160.0 * (i + 0.5) / n)
        u = np.array([np.cos(th), np.sin(th)])
        v = np.array([-u[1], u[0]])
        spot = c + 820.0 * u
        if kind == "fill":
            back, s = c - 4.0 * u, sq(a_pt, 3.0)
            e.fill(np.array([back, c + 6.0 * v, c + 860.0 * u, c - 6.0 * v, back, s[1], s[2], s[3], s[0], s[1]]), rgba)
        elif kind == "polyline":
            e.polyline(np.array([a_pt, c, c + 400.0 * u, c + 830.0 * u]), rgba, 1.0)
        elif kind == "line":
            e.stroke_line(C, tuple(c + 830.0 * u), 1.0, rgba)
        elif kind == "compound":
            e.fill_compound([sq(c, 4.0), sq(spot, 2.0), sq(a_pt, 3.0)], rgba, even_odd=bool(i & 1))
        else:
            centre = np.round(c + 400.0 * u)
            spot = centre + 401.5 * u
            if kind == "circle":
                e.circle(tuple(centre), 402.0)
            else:
                e.ellipse(tuple(centre), 402.0, 403.0)
        spots.append(spot)

    def emit(e):
        if half:
            e.begin_group(half)
            for i in range(half):
                item(e, i)
            e.end_group()
        for i in range(half, n):
            item(e, i)

    scene = hs._encode(pm, (1 if half else 0) + n - half, emit)
    q = np.concatenate([np.array(spots), [C, A, NOTHING, (np.nan, 600.0)]])
    return hs.Case(f"stack n={n}", scene, q, kinds=[kind_of(i) for i in range(n)], n=n, alphas=list(alphas), common=n, second=n + 1, nothing=n + 2)


def position_at_a(n, item):
    """Where `item` stands in A's stack: how many of the items above it reach A."""
    assert reaches_a(item)
    return sum(reaches_a(i) for i in range(item + 1, n))


def item_at_position(n, pos):
    return next(i for i in range(n - 1, -1, -1) if reaches_a(i) and position_at_a(n, i) == pos)


def _alphas(n, first):
    """n alphas that make item `first` the first opaque member of A's stack (None: it has none).  The items above it that reach A get
    1, 128, 0 and 254 in turn, `first` 255, the ones below all five in turn; the Lines above it -- members of C's stack -- 128, 0, 254
    and 1 in turn, the ones below all five.  (A Circle's alpha is written nowhere.)"""
    out, above, below = [0] * n, 0, 0
    for i in range(n - 1, -1, -1):
        if first is not None and i == first:
            out[i] = 255
        elif first is None or i > first:
            out[i] = ((1, 128, 0, 254) if reaches_a(i) else (128, 0, 254, 1))[above % 4]
            above += 1
        else:
            out[i] = ALPHAS[below % 5]
            below += 1
    return out


def _case(n, first):
    return _alphas(n, first), None if first is None else position_at_a(n, first)


# name -> (alphas, the position of the first opaque member in A's stack, or None)
CASES = {
    "top": _case(130, item_at_position(130, 0)),
    "second": _case(130, item_at_position(130, 1)),
    "at-63": _case(130, item_at_position(130, 63)),
    "at-64": _case(130, item_at_position(130, 64)),
    "at-65": _case(130, item_at_position(130, 65)),
    "item-63": _case(130, 130 - 1 - 63),
    "item-64": _case(130, 130 - 1 - 64),
    "item-65": _case(130, 130 - 1 - 65),
    "nowhere": _case(130, None),
    "nowhere-66": _case(66, None),
}
