"""Request lists for trimming, pm_trim_items and its device call (test helper, not a conftest): tests/test_trim.py runs them against
tests/np_trim.py under the emulation and on the GPU, and pins on the CPU that the cases are what they claim.

The scenes are resample_cases.SCENES as they are: measure_cases' -- segment counts at 16/17, 63/64/65 and 127/128/129, 1/64/65
items, degenerate and compound Fills, the 2^32 cap, the non-finite scene -- and `tiny`, whose items are 11, 12, 0 and 1 units long.

The kernel (piet_metal_amd/csrc/pm_trim.h) walks 64 entries per step and hands the previous covered segment's B from lane to lane
by a shuffle and from step to step in scalar registers, so what matters is WHERE the two ends of a piece lie: on a Q_k, one unit
either side of it, inside a segment, in which step of the walk, either side of a jump of the walk, on and beside a repeated vertex.
Every item of every scene, and the two item indices beyond it, gets

  * the fixed ranges: the whole item {0, 2^64 - 1}, [0, 0], [T, T], [T, 2^64 - 1], [1, T - 1] (where T >= 2);
  * its MARKS: the positions Q_k of the first and the last segment of a length, of the segments at entries 1, 63, 64, 65, 127 and 128,
    of every segment after a jump of the walk (the sub-path breaks of a compound Fill) and of every segment without length and the
    one after it.  Between every two neighbouring marks three pieces: both ends exactly on the marks, both one unit outside, both one
    unit inside; around every mark [Q - 1, Q + 1], [Q - 1, Q] and [Q, Q + 1];
  * both ends inside ONE segment: the first, the middle one and the last segment of a length;
  * where the walk has more than 64 entries: a piece wholly inside entries 64 .. 127 and one from the middle of the last segment
    before entry 63 to the middle of the first after entry 64;
  * the parts: every j of m = 1, 2, 3, 7 and j = 0, 1, m - 2, m - 1 of m = 64, 65.
"""
from __future__ import annotations

import measure_cases as mc
import np_measure as nm
import np_trim as nt
import resample_cases as rc

SCENES = rc.SCENES
U64_MAX = (1 << 64) - 1
SMALL_PARTS, BIG_PARTS = (1, 2, 3, 7), (64, 65)
STEP_ENTRIES = (1, 63, 64, 65, 127, 128)


def jumps(st):
    """The positions i of nt.starts(w) whose segment does not begin where the one before ended (as bytes)."""
    return [i for i in range(1, len(st)) if st[i][1].tobytes() != st[i - 1][2].tobytes()]


def marks(w):
    """The sorted positions Q_k the pieces of an item are hung on."""
    st = nt.starts(w)
    positive = [i for i, sg in enumerate(st) if sg[3] > 0]
    at = set(positive[:1] + positive[-1:])
    at |= {i for i, sg in enumerate(st) if sg[0] in STEP_ENTRIES}
    at |= set(jumps(st))
    for i, sg in enumerate(st):
        if sg[3] == 0:
            at |= {i, min(i + 1, len(st) - 1)}
    return sorted({st[i][4] for i in at})


def range_requests(w):
    """(s0, s1) of one item, valid ones only, without repeats, in a fixed order."""
    T = w.T
    out = [(0, U64_MAX), (0, 0), (T, T), (T, U64_MAX)]
    if T >= 2:
        out.append((1, T - 1))
    ms = marks(w)
    for a, b in zip(ms, ms[1:]):
        out += [(a, b), (a - 1, b + 1), (a + 1, b - 1)]
    for Q in ms:
        out += [(Q - 1, Q + 1), (Q - 1, Q), (Q, Q + 1)]
    st = nt.starts(w)
    positive = [sg for sg in st if sg[3] >= 3]
    for sg in positive[:1] + positive[len(positive) // 2:len(positive) // 2 + 1] + positive[-1:]:
        out.append((sg[4] + sg[3] // 3, sg[4] + 2 * sg[3] // 3))
    mid = lambda sg: sg[4] + sg[3] // 2  # noqa: E731
    second = [sg for sg in st if 66 <= sg[0] <= 120 and sg[3] > 0]
    if len(second) >= 2:
        out.append((mid(second[0]), mid(second[-1])))
    before, after = [sg for sg in st if sg[0] < 63 and sg[3] > 0], [sg for sg in st if sg[0] > 64 and sg[3] > 0]
    if before and after:
        out.append((mid(before[-1]), mid(after[0])))
    seen, kept = set(), []
    for s0, s1 in out:
        if 0 <= s0 <= s1 <= U64_MAX and (s0, s1) not in seen:
            seen.add((s0, s1))
            kept.append((s0, s1))
    return kept


def part_requests():
    """(j, m)."""
    out = [(j, m) for m in SMALL_PARTS for j in range(m)]
    out += [(j, m) for m in BIG_PARTS for j in (0, 1, m - 2, m - 1)]
    return out


_requests = {}


def requests(pm, name, skip=False):
    """Every request of a scene without its place: [(item, mode, s0, s1)]."""
    if (name, skip) not in _requests:
        ws = rc.expected_walks(pm, name, skip)
        n = len(ws)
        out = []
        for i in list(range(n)) + [n, 0xFFFFFFFF]:
            w = ws[i] if i < n else nm.Walk()
            out += [(i, nt.RANGE, s0, s1) for s0, s1 in range_requests(w)]
            out += [(i, nt.PART, j, m) for j, m in part_requests()]
        _requests[(name, skip)] = out
    return _requests[(name, skip)]


def layout_requests(pm):
    """The truncation and layout list on the scene `counts`: ([(item, mode, first, cap, s0, s1)], out_cap, the whole pieces' sizes).
    Said per line what it is there for; `n` is the piece's n_vertices."""
    ws = rc.expected_walks(pm, "counts")
    names = mc.NAMES["counts"]
    a, b, c, d = names["poly-200"], names["fill-129"], names["compound-65"], names["poly-2"]
    whole = (0, U64_MAX)
    n = {i: len(nt.vertices(ws[i], 0, ws[i].T)) for i in (a, b, c, d)}
    assert (n[a], n[b], n[d]) == (201, 130, 3) and n[c] > 66          # compound-65: two runs
    sta = nt.starts(ws[a])
    inner = (sta[3][4] + 1, sta[150][4] - 1)                           # starts and ends inside a segment: A and B of its first segment are two vertices
    out_cap = 900
    laid = [
        (a, nt.RANGE, 0, 0, *whole),                                   # cap = 0: the count pass
        (a, nt.RANGE, 10, 1, *inner),                                  # cap = 1: between the first A and its B
        (a, nt.RANGE, 20, n[a] - 1, *whole),                           # one short
        (b, nt.RANGE, 600, 64, *whole),                                # one short of the first step's vertices (the first A and 64 B) ...
        (b, nt.RANGE, 230, 65, *whole),                                # ... exactly at the step edge ...
        (b, nt.RANGE, 300, 40, *whole),                                # ... in the middle of the first step ...
        (b, nt.RANGE, 700, 100, *whole),                               # ... and in the middle of the second
        (c, nt.PART, 350, n[c], 0, 1),                                 # a whole compound item, out of order, behind a later one
        (a, 2, 430, 50, 0, 7),                                         # invalid: no such mode
        (a, nt.RANGE, 430, 50, 8, 7),                                  # invalid: s0 > s1
        (a, nt.PART, 430, 50, 0, 0),                                   # invalid: no parts
        (a, nt.PART, 430, 50, 3, 3),                                   # invalid: j == m
        (a, nt.PART, 430, 50, 0, nt.MAX_PARTS + 1),                    # invalid: too many parts
        (a, 0xFFFFFFFF, 430, 50, 0, 0),
        (d, nt.RANGE, 490, 5, *whole),                                 # more room than vertices: the rest stays untouched
        (a, nt.RANGE, out_cap - 100, 300, *whole),                     # first + p crosses out_cap
        (b, nt.RANGE, out_cap, 10, *whole),                            # begins at out_cap: nothing of it is written
        (d, nt.RANGE, 0xFFFFFFFF, 3, *whole),                          # first + p passes 2^32
        (d, nt.RANGE, 5, 3, *whole),                                   # ... and a caller-chosen first below everything
    ]
    return laid, out_cap, n


def truncation_sweep(pm):
    """Caps around every place a cap can cut, on fill-129 of `counts` (130 vertices: A_0, then B_0 .. B_128; a step edge after B_63):
    [(item, mode, s0, s1, cap)]."""
    i = mc.NAMES["counts"]["fill-129"]
    return [(i, nt.RANGE, 0, U64_MAX, cap) for cap in (0, 1, 2, 63, 64, 65, 66, 128, 129, 130, 131)]
