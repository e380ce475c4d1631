"""Request lists for resampling, pm_resample_items and its device call (test helper, not a conftest): tests/test_resample.py runs
them against tests/np_resample.py under the emulation and on the GPU, and pins on the CPU that the cases are what they claim.

The scenes are measure_cases.SCENES as they are -- segment counts at 16/17, 63/64/65 and 127/128/129, 1/64/65 items, degenerate and
compound Fills, the 2^32 cap, the non-finite scene -- and ONE more, TINY, whose items are a few units of 2^-16 px long: the only
way to an even request with more gaps than the item has units (m > T > 0).

The kernel (piet_metal_amd/csrc/pm_resample.h) answers 64 samples per round and walks 64 entries per step, so the counts sit at
0, 1, 2, 63, 64, 65 and 129 (step mode) and 0, 1, 2, 3, 64, 65, 129 (even mode).  The twelve (start, step) VARIANTS of an item:

  step 0 (inside the item), step 1 unit (one segment owns every sample), step = the item's first positive q (samples land exactly
  on a Q_k: the start rule), step T and step T + 1 each from start 0, T - 1, T and T + 1, and start 2^64 - 1 with step 1 (saturation).

The full cross of counts and variants on every item of every scene is 4 152 samples an item and 0.9 million in all, where the
whole file is to stay in the tens of thousands.  So:

  * ONE item of each scene in FULL_CROSS -- the one with the most segments: 200 in three steps of the walk and a tail, 69 with
    degenerate segments across a step edge, 70 capped ones, the lone item of walk-1 and the tiny Fill -- gets the full cross: every variant with every
    step count, and every even count;
  * every other item, and the two item indices beyond the scene, gets every variant with one of the counts 0, 1, 2 (which one
    rotates with the item and the variant), the even counts 0, 1, 2, 3, and ONE large request: by turns a step request -- the
    variant and the count out of 63, 64, 65, 129 rotate with the item -- and an even one of 64, 65 or 129 samples;
  * item 0 of every scene gets WIDE_STEPS: steps so wide that j * step itself passes 2^64.
"""
from __future__ import annotations

import numpy as np

import measure_cases as mc
import np_measure as nm
import np_resample as nr

F32 = np.float32
TINY = "tiny"
SCENES = mc.SCENES + (TINY,)
FULL_CROSS = ("counts", "degenerate", "caps", "walk-1", TINY)
STEP_COUNTS = (0, 1, 2, 63, 64, 65, 129)
EVEN_COUNTS = (0, 1, 2, 3, 64, 65, 129)
SMALL, BIG, EVEN_SMALL, EVEN_BIG = (0, 1, 2), (63, 64, 65, 129), (0, 1, 2, 3), (64, 65, 129)
U64_MAX = (1 << 64) - 1
U = 1.0 / 65536.0

_tiny = {}


def scene_of(pm, name):
    if name != TINY:
        return mc.scene_of(pm, name)
    if TINY not in _tiny:
        # 0: a Polyline of 5 + 6 units; 1: a 3-4-5 Fill, 12 units around; 2: a Circle; 3: a Line of 1 unit
        entries = [
            ("poly_11_units", lambda e: e.polyline(mc.zig(3, 1.0, 1.0), mc.OPAQUE, 1.0), ("points", 0, [[0, 0], [3 * U, 4 * U], [3 * U, 10 * U]])),
            ("fill_12_units", lambda e: e.fill(mc.zig(3, 1.0, 1.0), mc.OPAQUE), ("points", 0, [[0, 0], [3 * U, 0], [3 * U, 4 * U]])),
            ("circle", lambda e: e.circle((100.0, 100.0), 10.0)),
            ("line_1_unit", lambda e: e.stroke_line((0.0, 0.0), (1.0, 0.0), 1.0, mc.OPAQUE), ("line", (8.0, 8.0), (8.0, 8.0 + U))),
        ]
        _tiny[TINY] = mc._build(pm, TINY, entries)
    return _tiny[TINY]


_walks = {}


def expected_walks(pm, name, skip=False):
    if name != TINY:
        return mc.expected_walks(pm, name, skip)
    if (name, skip) not in _walks:
        _walks[(name, skip)] = nm.walks(scene_of(pm, name), skip)
    return _walks[(name, skip)]


def variants(w):
    """The twelve (start, step) of a walk."""
    T = w.T
    q_first = next((sg[3] for sg in w.segs if sg[3] > 0), 1)
    out = [(T // 3, 0), (T // 2, 1), (0, q_first)]
    for step in (T, T + 1):
        out += [(start, step) for start in (0, max(T - 1, 0), T, T + 1)]
    out.append((U64_MAX, 1))
    assert len(out) == 12
    return out


def full_cross_item(ws):
    return max(range(len(ws)), key=lambda i: len(ws[i].segs))


def special_requests(name, names, ws):
    """Requests that need a particular item: (item, mode, count, start, step)."""
    out = []
    if name == "caps":          # 70 segments of exactly 2^32 units: a sample in the middle of each, 64 consecutive segments and six more
        for entry in ("poly_70_caps", "fill_70_caps"):
            out.append((names[entry], nr.STEP, 70, 1 << 31, 1 << 32))
    if name == "counts":        # 200 segments are four steps of the walk: the two in the middle own no sample; then one sample per step
        for entry in ("poly-200", "fill-200", "compound-200"):
            i = names[entry]
            out.append((i, nr.STEP, 2, 1, ws[i].T - 2))
            out.append((i, nr.STEP, 5, 3, ws[i].T // 4))
    return out


# Steps whose product j * step passes 2^64 in each way a multiplication in two 32-bit halves can: in the high half alone, in the sum
# of the halves (3 * 0x5555555555555556 is 2^64 + 2: unchecked, sample 3 would land 9 units into the item), and only when start is added
WIDE_STEPS = ((0, 1 << 63), (7, 0x5555555555555556), (1, U64_MAX), (1 << 63, (1 << 62) + 1))


def requests(pm, name, skip=False):
    """Every request of a scene, unpacked: [(item, mode, count, start, step)]."""
    ws = expected_walks(pm, name, skip)
    n = len(ws)
    full = full_cross_item(ws) if name in FULL_CROSS else None
    out = []
    for pos, i in enumerate(list(range(n)) + [n, 0xFFFFFFFF]):
        V = variants(ws[i] if i < n else nm.Walk())
        if i == full:
            out += [(i, nr.STEP, c, start, step) for (start, step) in V for c in STEP_COUNTS]
            out += [(i, nr.EVEN, c, 0, 0) for c in EVEN_COUNTS]
            continue
        out += [(i, nr.STEP, SMALL[(pos + v) % 3], start, step) for v, (start, step) in enumerate(V)]
        out += [(i, nr.EVEN, c, 0, 0) for c in EVEN_SMALL]
        if pos % 2 == 0:
            start, step = V[(pos // 2) % 12]
            out.append((i, nr.STEP, BIG[(pos // 2) % 4], start, step))
        else:
            out.append((i, nr.EVEN, EVEN_BIG[(pos // 2) % 3], 0, 0))
    out += [(0, nr.STEP, 5, start, step) for start, step in WIDE_STEPS]
    out += special_requests(name, mc.NAMES.get(name, {}), ws)
    return out


def n_samples(reqs):
    return sum(r[2] for r in reqs)
