"""Scenes and queries for path measurement, pm_item_lengths / pm_points_at_length / pm_positions_on_edges (test helper, not a
conftest): tests/test_measure.py runs them against tests/np_measure.py under the emulation and on the GPU, and pins on the CPU
that the cases are what they claim.

The kernels (piet_metal_amd/csrc/pm_measure.h) sum an item of up to LANE entries on its lane and a longer one over the wave; the
walk of a point query takes 64 entries per step with a carry between the steps; the items of a scene are dealt 64 per step.

  counts      a Polyline, a plain Fill and a compound Fill of every segment count in SEG_COUNTS;
  degenerate  repeated vertices at the start, in the middle, at the end and across a step edge, items whose every segment is
              degenerate, a one-point Polyline, a Fill of 0 points, a Circle, an ellipse, a Line of no length, a Fill whose closing
              segment has no length, items of alpha 0;
  compound    two and three sub-paths, an empty sub-path, sub-paths that end exactly at a step edge;
  caps        a segment just below, at and above 65 536 px, 70 segments of the cap in one item, coordinates at +-3e38, a mix of
              short and capped segments;
  nonfinite   the ONE scene with non-finite points: the five floats of a point record on a segment with such an end are not
              promised (NONFINITE names it; every record of every other scene is compared in full);
  walk-N      hit_structure.walk_scene at 1, 64 and 65 items: every kind in turn, a child group, every third item of alpha 0.

Values that an encoder would refuse or tidy are written into the encoded bytes afterwards: the scene format is data."""
from __future__ import annotations

import struct

import numpy as np

import bounds_cases as bc
import hit_structure as hs
import np_hit
import np_measure as nm

F32 = np.float32
LANE = 16                       # kMeasureLane (pm_measure.h)
WAVE = 64
SEG_COUNTS = (0, 1, 2, 16, 17, 63, 64, 65, 66, 127, 128, 129, 200)
WALK_SIZES = (1, 64, 65)
NONFINITE = "nonfinite"
SCENES = ("counts", "degenerate", "compound", "caps", NONFINITE) + tuple(f"walk-{n}" for n in WALK_SIZES)
STEP_KS = (1, 63, 64, 65)       # the segments whose Q is asked for, besides the last
TS = [F32(0.0), F32(1.0), F32(0.5), np.nextafter(F32(1.0), F32(0.0)), F32(-0.0), F32(-0.25), F32(1.5), F32(np.nan)]
U64_MAX = (1 << 64) - 1


def zig(n, x0, y0):
    """n points of a zigzag whose segments all have different, irrational lengths."""
    k = np.arange(n)
    return np.stack([x0 + 3.0 * k + 0.25 * (k % 3), y0 + 4.0 * (k % 2) + 0.5 * (k % 5)], axis=1)


def patch_line(scene, i, a, b):
    at = bc._item(scene, i)
    scene[at + 16 : at + 32] = np.array([a, b], F32).view(np.uint8).reshape(-1)


_scenes = {}
NAMES = {}     # scene name -> {entry name: item index}


def _build(pm, name, entries, cap=1 << 18):
    """entries: (name, emit, patches ...) with patches ("points", at, values), ("npt", n), ("line", a, b)."""
    def emit(e):
        for en in entries:
            en[1](e)

    scene = hs._encode(pm, len(entries), emit, cap=cap)
    for i, en in enumerate(entries):
        for p in en[2:]:
            if p[0] == "points":
                bc.patch_points(scene, i, p[1], p[2])
            elif p[0] == "npt":
                bc.patch_npt(scene, i, p[1])
            else:
                patch_line(scene, i, p[1], p[2])
            bc.patch_short_bbox(scene, i, (0, 0, 65535, 65535))
    NAMES[name] = {en[0]: i for i, en in enumerate(entries)}
    return scene


OPAQUE, CLEAR = 0x336699FF, 0x33669900


def counts_scene(pm):
    entries = []
    for j, n in enumerate(SEG_COUNTS):
        y = 20.0 + 30.0 * j
        entries.append((f"poly-{n}", lambda e, n=n, y=y: e.polyline(zig(n + 1, 10.0, y), 0x11AA22FF, 1.0)))
        if n == 0:
            entries.append(("fill-0", lambda e, y=y: e.fill(zig(1, 10.0, y + 10), OPAQUE), ("npt", 0)))
        else:
            entries.append((f"fill-{n}", lambda e, n=n, y=y: e.fill(zig(n, 10.0, y + 10), OPAQUE)))
        m = max(n, 1)     # `m` segments in two sub-paths where there are enough points: m + 2 entries (m + 1 with one sub-path)
        p = zig(m, 10.0, y + 20)
        entries.append((f"compound-{m}", lambda e, p=p, m=m: e.fill_compound([p[: m // 2], p[m // 2 :]] if m >= 4 else [p], 0xAA5500FF)))
    return _build(pm, "counts", entries, cap=1 << 19)


def degenerate_scene(pm):
    A, B, Cc = (10.0, 10.0), (40.0, 50.0), (70.0, 10.0)
    step = zig(70, 10.0, 200.0)
    step[62:67] = step[62]
    entries = [
        ("poly_repeat_start", lambda e: e.polyline(np.array([A, A, A, B, Cc]), OPAQUE, 1.0)),
        ("poly_repeat_middle", lambda e: e.polyline(np.array([A, B, B, B, Cc]), OPAQUE, 1.0)),
        ("poly_repeat_end", lambda e: e.polyline(np.array([A, B, Cc, Cc, Cc]), OPAQUE, 1.0)),
        ("poly_repeat_step_edge", lambda e: e.polyline(step, OPAQUE, 1.0)),
        ("poly_all_degenerate", lambda e: e.polyline(np.array([B] * 5), OPAQUE, 1.0)),
        ("fill_all_degenerate", lambda e: e.fill(np.array([B] * 4), OPAQUE)),
        ("poly_one_point", lambda e: e.polyline(np.array([B]), OPAQUE, 1.0)),
        ("fill_zero_points", lambda e: e.fill(np.array([A]), OPAQUE), ("npt", 0)),
        ("circle", lambda e: e.circle((100.0, 100.0), 10.0)),
        ("ellipse", lambda e: e.ellipse((140.0, 100.0), 10.0, 5.0)),
        ("line_zero_length", lambda e: e.stroke_line(B, B, 2.0, OPAQUE)),
        ("line", lambda e: e.stroke_line((10.0, 120.0), (13.0, 124.0), 2.0, OPAQUE)),
        ("fill_closing_degenerate", lambda e: e.fill(np.array([A, B, Cc, A]), OPAQUE)),
        ("fill_transparent", lambda e: e.fill(np.array([A, B, Cc]), CLEAR)),
        ("poly_transparent", lambda e: e.polyline(np.array([A, B, Cc]), CLEAR, 1.0)),
        ("line_transparent", lambda e: e.stroke_line(A, B, 2.0, CLEAR)),
        ("compound_transparent", lambda e: e.fill_compound([bc.sq(0, 0, 10, 10), bc.sq(2, 2, 8, 8)], CLEAR)),
        ("fill_last", lambda e: e.fill(bc.sq(5.5, 6.5, 7.5, 8.5), OPAQUE)),
    ]
    return _build(pm, "degenerate", entries)


def compound_scene(pm):
    ring = bc.ring
    sep = bc.separator
    entries = [
        ("two", lambda e: e.fill_compound([bc.sq(10, 10, 40, 50), bc.sq(20, 20, 23, 24)], OPAQUE)),
        ("three", lambda e: e.fill_compound([ring(100.0, 40.0, 20.0, 7), bc.sq(90, 30, 110, 50), ring(100.0, 40.0, 5.0, 3)], OPAQUE, even_odd=True)),
        # entries: 5 points, a separator, then an EMPTY sub-path (a separator alone), 4 points and their separator
        ("empty_sub_path", lambda e: e.fill_compound([ring(200.0, 40.0, 20.0, 5), ring(200.0, 40.0, 8.0, 5)], OPAQUE),
            ("points", 6, [sep(6)]), ("points", 11, [sep(7)])),
        ("ends_before_step_edge", lambda e: e.fill_compound([zig(63, 10.0, 100.0), zig(10, 10.0, 120.0)], OPAQUE)),     # its separator is entry 63
        ("ends_at_step_edge", lambda e: e.fill_compound([zig(64, 10.0, 140.0), zig(10, 10.0, 160.0)], OPAQUE)),        # its last point is entry 63
        ("only_separators", lambda e: e.fill_compound([bc.sq(1, 1, 2, 2)], OPAQUE), ("points", 0, [sep(0)] * 5)),
    ]
    return _build(pm, "compound", entries)


BELOW_CAP = np.nextafter(F32(65536.0), F32(0.0))


def caps_scene(pm):
    big = F32(3.0e38)
    bounce = np.array([[0.0 if k % 2 == 0 else 70000.0, float(k)] for k in range(71)])
    entries = [
        ("line_below_cap", lambda e: e.stroke_line((0.0, 0.0), (1.0, 0.0), 1.0, OPAQUE), ("line", (0.0, 0.0), (BELOW_CAP, 0.0))),
        ("line_at_cap", lambda e: e.stroke_line((0.0, 0.0), (1.0, 0.0), 1.0, OPAQUE), ("line", (0.0, 8.0), (65536.0, 8.0))),
        ("line_above_cap", lambda e: e.stroke_line((0.0, 0.0), (1.0, 0.0), 1.0, OPAQUE), ("line", (0.0, 16.0), (65540.0, 16.0))),
        ("poly_70_caps", lambda e: e.polyline(zig(71, 1.0, 1.0), OPAQUE, 1.0), ("points", 0, bounce)),
        ("fill_70_caps", lambda e: e.fill(zig(70, 1.0, 1.0), OPAQUE), ("points", 0, bounce[:70])),
        ("poly_huge", lambda e: e.polyline(zig(4, 1.0, 1.0), OPAQUE, 1.0), ("points", 0, [[-big, -big], [big, big], [big, -big], [-big, big]])),
        ("poly_mixed", lambda e: e.polyline(zig(4, 1.0, 1.0), OPAQUE, 1.0), ("points", 0, [[0, 0], [3, 4], [70003, 4], [70003, 8]])),
    ]
    return _build(pm, "caps", entries)


def nonfinite_scene(pm):
    inf, nan = np.inf, np.nan
    entries = [
        ("poly_inf_middle", lambda e: e.polyline(zig(5, 1.0, 1.0), OPAQUE, 1.0), ("points", 0, [[0, 0], [10, 0], [inf, 0], [20, 0], [30, 0]])),
        ("poly_nan_middle", lambda e: e.polyline(zig(5, 1.0, 1.0), OPAQUE, 1.0), ("points", 0, [[0, 0], [10, 0], [nan, 5], [20, 0], [30, 0]])),
        ("fill_mixed", lambda e: e.fill(zig(6, 1.0, 1.0), OPAQUE), ("points", 0, [[0, 0], [10, 0], [10, nan], [-inf, 10], [0, 10], [0, 5]])),
        ("line_inf_end", lambda e: e.stroke_line((0.0, 0.0), (1.0, 0.0), 1.0, OPAQUE), ("line", (3.0, 4.0), (inf, -inf))),
        ("poly_all_nan", lambda e: e.polyline(zig(3, 1.0, 1.0), OPAQUE, 1.0), ("points", 0, [[nan, nan]] * 3)),
        ("poly_finite", lambda e: e.polyline(np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 0.0]]), OPAQUE, 1.0)),
    ]
    return _build(pm, NONFINITE, entries)


def scene_of(pm, name):
    if name not in _scenes:
        if name.startswith("walk-"):
            _scenes[name] = hs.walk_scene(pm, int(name[5:])).scene
        else:
            _scenes[name] = {"counts": counts_scene, "degenerate": degenerate_scene, "compound": compound_scene, "caps": caps_scene,
                             NONFINITE: nonfinite_scene}[name](pm)
    return _scenes[name]


_walks = {}


def expected_walks(pm, name, skip=False):
    """np_measure.walks of the scene, computed once."""
    if (name, skip) not in _walks:
        _walks[(name, skip)] = nm.walks(scene_of(pm, name), skip)
    return _walks[(name, skip)]


# ---- the queries ----------------------------------------------------------------------------------------------------------

def entry_counts(scene):
    """Per item: how many entry indices its walk runs over (a Line 1, a Polyline npt - 1, a Fill npt, anything else 0)."""
    sc = bytes(scene)
    out = []
    for at, _ in np_hit.flat_items(sc):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        npt = struct.unpack_from("<I", sc, at + 12)[0]
        out.append({np_hit.LINE: 1, np_hit.POLY: max(npt - 1, 0), np_hit.FILL: npt}.get(tag, 0))
    return out


def point_queries(ws, seed=11):
    """(item, s) for every item of the scene and the two item indices beyond it."""
    rng = np.random.default_rng(seed)
    out = []
    for i, w in enumerate(ws):
        Q, starts = 0, {}
        for k, _, _, q in w.segs:
            starts[k] = Q
            Q += q
        T = w.T
        want = {0, 1, T - 1, T, T + 1, U64_MAX}
        ks = [k for k in STEP_KS if k in starts] + ([w.segs[-1][0]] if w.segs else [])
        for k in ks:
            want |= {starts[k] - 1, starts[k], starts[k] + 1}
        want |= {int(rng.integers(0, T + 1)) for _ in range(3)}
        out += [(i, s) for s in sorted(want) if 0 <= s <= U64_MAX]
    n = len(ws)
    out += [(n, 0), (n, 5), (0xFFFFFFFF, 0), (0xFFFFFFFF, U64_MAX)]
    return out


def edge_queries(scene, ws):
    """(item, index, t): every t of TS at the last segment, one past it, index 0 and a separator; 0.5 and 1 at the step edges."""
    out = []
    for i, (w, n_idx) in enumerate(zip(ws, entry_counts(scene))):
        seg_ks = {sg[0] for sg in w.segs}
        separators = [k for k in range(n_idx) if k not in seg_ks][:2] if w.kind == nm.CLOSED else []
        full = {0, n_idx, n_idx + 5} | ({w.segs[-1][0]} if w.segs else set()) | set(separators)
        for index in sorted(full):
            out += [(i, index, t) for t in TS]
        for index in (1, 62, 63, 64, 65, 127, 128):
            if index < n_idx and index not in full:
                out += [(i, index, F32(0.5)), (i, index, F32(1.0)), (i, index, F32(0.0))]
    n = len(ws)
    out += [(n, 0, F32(0.5)), (0xFFFFFFFF, 0, F32(0.0))]
    return out
