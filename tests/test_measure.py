"""Path measurement, pm_item_lengths / pm_points_at_length / pm_positions_on_edges and their device calls (decision D25): how long
every item is, the point and the direction at a length along it, and how far along it a point of an edge lies.

The bar everywhere: records EQUAL to tests/np_measure.py as bytes, through the host and the device calls, with and without
PM_HIT_SKIP_TRANSPARENT.  The one exception: the five floats of a point record whose located segment has a non-finite end, in the
one scene measure_cases.NONFINITE -- item, status and index are compared there too.  tests/measure_cases.py builds the scenes and
the queries.

-m gpu: every case scene (segment counts around the lane / wave threshold and the 64-segment steps, 1 / 64 / 65 items, degenerate
geometry, compound Fills, the cap, non-finite points) with the positions and the inverse queries of measure_cases and the round
trip of relation 3 on the device's own answers; pm_snap's answers into pm_positions_on_edges without a read-back; lengths after
reflatten_groups and after a styled and dashed flatten; capacity, every argument error and n == 0; a scene without items; queries
between frames in flight and after a scene replacement; the CLI.
CPU: np_measure against hand-derived 3-4-5 geometry, against np_dash.walk / _point on the poly-lines of the dash_cases seeds, the
round trip in exact integers; the cases are what they claim; the header; the -m gpu part against the wave64 emulation of the
kernels; the compiler's listing."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hit_structure as hs  # noqa: E402
import measure_cases as mc  # noqa: E402
import np_measure as nm  # noqa: E402

F32 = np.float32
UNTOUCHED = 0x7EADBEEF
INVALID, CAPACITY = -1, -4
FLOATS = ("t", "x", "y", "tx", "ty")
# case scenes, snap composition, groups, styled and dashed, argument rules, no items, ordering, CLI
N_GPU_TESTS = len(mc.SCENES) + 1 + 1 + 1 + 1 + 1 + 1 + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def skip_flag(pm, skip):
    return pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0


def to_device(a):
    """A numpy array of records as int32 words on the device (under the emulation device memory is host memory)."""
    a = np.ascontiguousarray(a)
    words = a.view(np.int32).reshape(len(a), -1)
    if _emulated():
        return words.copy()
    import torch

    return torch.from_numpy(words.copy()).cuda()


def host_view(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def blank(rows, words):
    if _emulated():
        return np.full((rows, words), UNTOUCHED, np.int32)
    import torch

    return torch.full((rows, words), UNTOUCHED, dtype=torch.int32, device="cuda")


def device_lengths(pm, r, n_rows, skip=False, stream=None):
    """pm_item_lengths_device into n_rows records of UNTOUCHED words, not waited for."""
    out = blank(n_rows, 4)
    if _emulated():
        pm._lib.check(pm._lib.load().pm_item_lengths_device(r._h, skip_flag(pm, skip), out.ctypes.data, n_rows, None), "pm_item_lengths_device")
    else:
        r.item_lengths_tensor(out, stream=stream, skip_transparent=skip)
    return out


def device_points(pm, r, q, skip=False, stream=None, pad=1):
    """pm_points_at_length_device for LENGTH_QUERY records q (numpy, or device words as they are): (int32 [n + pad, 8], keep-alive)."""
    dq = to_device(q) if isinstance(q, np.ndarray) and q.dtype.names else q
    n = len(dq)
    out = blank(n + pad, 8)
    if _emulated():
        pm._lib.check(pm._lib.load().pm_points_at_length_device(r._h, dq.ctypes.data, n, skip_flag(pm, skip), out.ctypes.data, None), "pm_points_at_length_device")
    else:
        r.points_at_length_tensor(dq, out[:n], stream=stream, skip_transparent=skip)
    return out, dq


def device_positions(pm, r, q, skip=False, stream=None, pad=1):
    """pm_positions_on_edges_device for EDGE_QUERY records q (numpy, or device words as they are): (int32 [n + pad, 4], keep-alive)."""
    dq = to_device(q) if isinstance(q, np.ndarray) and q.dtype.names else q
    n = len(dq)
    out = blank(n + pad, 4)
    if _emulated():
        pm._lib.check(pm._lib.load().pm_positions_on_edges_device(r._h, dq.ctypes.data, n, skip_flag(pm, skip), out.ctypes.data, None), "pm_positions_on_edges_device")
    else:
        r.positions_on_edges_tensor(dq, out[:n], stream=stream, skip_transparent=skip)
    return out, dq


def as_rec(a, dtype, n=None):
    a = np.ascontiguousarray(host_view(a)[:n] if n is not None else host_view(a))
    return a.view(dtype).reshape(-1)


def same(got, want):
    return np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


def differing(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    size = g.dtype.itemsize
    return np.flatnonzero((g.view(np.uint8).reshape(-1, size) != w.view(np.uint8).reshape(-1, size)).any(axis=1))


def new_stream():
    if _emulated():
        return None
    import torch

    return torch.cuda.Stream()


def wait(r, stream):
    r.sync()
    if stream is not None:
        stream.synchronize()


def length_queries(pairs):
    q = np.zeros(len(pairs), nm.LENGTH_QUERY)
    q["item"] = [p[0] for p in pairs]
    q["s"] = np.array([p[1] for p in pairs], np.uint64)
    return q


def edge_query_records(triples):
    q = np.zeros(len(triples), nm.EDGE_QUERY)
    q["item"] = [t[0] for t in triples]
    q["index"] = [t[1] for t in triples]
    q["t"] = np.array([t[2] for t in triples], F32)
    return q


def unpromised(ws, want):
    """bool [n]: the point records whose located segment has a non-finite end."""
    out = np.zeros(len(want), bool)
    for j, rec in enumerate(want):
        if rec["item"] != nm.HIT_NONE:
            out[j] = nm.has_non_finite_end(ws[int(rec["item"])], int(rec["index"]))
    return out


def assert_points(got, want, ws, exempt, what):
    """Point records equal as bytes; where `exempt` (only ever the non-finite scene) a record on a segment with a non-finite end is
    compared in item, status and index alone."""
    got, want = np.ascontiguousarray(got).copy(), want.copy()
    if exempt:
        loose = unpromised(ws, want)
        for f in FLOATS:
            got[f][loose] = 0
            want[f][loose] = 0
    bad = differing(got, want)
    assert bad.size == 0, (what, len(bad), [(int(k), got[k], want[k]) for k in bad[:6]])


def round_trip_bound(ws, pairs, points, back):
    """Relation 3 in exact integers: the inverse call on a point answer's (item, index, t) returns s where s is an end of the
    located segment (t is exactly 0 or 1), else a position within ceil(q_k 2^-24) + 1 of it.  (An s one unit short of the end of a
    segment of 2^25 units or more has a t64 that rounds to the f32 1: that answer is inside the bound, not exact.)  Returns how many
    answers were checked each way."""
    exact = loose = 0
    for (item, s), p, b in zip(pairs, points, back):
        if p["item"] == nm.HIT_NONE or p["status"] & (nm.CLAMPED | nm.DEGENERATE):
            continue
        Q = 0
        for k, _, _, q in ws[int(item)].segs:
            if k == int(p["index"]):
                break
            Q += q
        assert b["item"] == item and b["status"] == nm.FOUND and Q <= s <= Q + q
        if s == Q or s == Q + q:
            assert float(p["t"]) == (0.0 if s == Q else 1.0) and int(b["s"]) == s, (item, s, p, b)
            exact += 1
        else:
            assert abs(int(b["s"]) - s) <= -(-q // (1 << 24)) + 1, (item, s, q, p, b)
            loose += 1
    return exact, loose


@pytest.fixture(scope="module")
def measure_renderer(pm):
    """Never resized: the queries need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


def check_scene(pm, r, scene, ws_by_skip, exempt, stream=None, what=""):
    """Lengths, points and positions of one resident scene, host and device, with and without the skip flag: equal to np_measure."""
    checked = 0
    for skip in (False, True):
        ws = ws_by_skip[skip]
        n = len(ws)
        want_len = nm.item_lengths(scene, skip, ws)
        pairs = mc.point_queries(ws)
        triples = mc.edge_queries(scene, ws)
        lq, eq = length_queries(pairs), edge_query_records(triples)
        want_pts = nm.points_at_length(scene, pairs, skip, ws)
        want_pos = nm.positions_on_edges(scene, triples, skip, ws)
        dev_len = device_lengths(pm, r, n + 2, skip, stream)
        dev_pts, keep1 = device_points(pm, r, lq, skip, stream)
        dev_pos, keep2 = device_positions(pm, r, eq, skip, stream)
        got_len = r.item_lengths(skip)
        bad = differing(got_len, want_len)
        assert bad.size == 0, (what, skip, "lengths", [(int(k), got_len[k], want_len[k]) for k in bad[:6]])
        got_pts = r.points_at_units(lq["item"], lq["s"], skip)
        assert_points(got_pts, want_pts, ws, exempt, (what, skip, "points"))
        got_pos = r.positions_on_edges(eq["item"], eq["index"], eq["t"], skip)
        bad = differing(got_pos, want_pos)
        assert bad.size == 0, (what, skip, "positions", [(triples[k], got_pos[k], want_pos[k]) for k in bad[:6]])
        wait(r, stream)
        assert same(as_rec(dev_len, nm.ITEM_LENGTH, n), want_len) and (host_view(dev_len)[n:] == UNTOUCHED).all(), (what, skip, "device lengths")
        assert_points(as_rec(dev_pts, nm.LENGTH_POINT, len(lq)), want_pts, ws, exempt, (what, skip, "device points"))
        assert same(as_rec(dev_pos, nm.LENGTH_AT, len(eq)), want_pos), (what, skip, "device positions")
        assert (host_view(dev_pts)[len(lq):] == UNTOUCHED).all() and (host_view(dev_pos)[len(eq):] == UNTOUCHED).all()
        # relation 3 on the device's own answers
        back = r.positions_on_edges(got_pts["item"], got_pts["index"], got_pts["t"], skip)
        if not exempt:
            round_trip_bound(ws, pairs, got_pts, back)
        checked += len(pairs) + len(triples)
    return checked


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.SCENES)
def test_case_scenes(pm, measure_renderer, name):
    """Every case scene: item records, the positions of measure_cases.point_queries on every item and the two indices beyond the
    scene, the inverse queries of measure_cases.edge_queries -- host calls, and device calls on a caller's stream."""
    scene = mc.scene_of(pm, name)
    r = measure_renderer
    r.set_scene_bytes(scene)
    ws = {skip: mc.expected_walks(pm, name, skip) for skip in (False, True)}
    assert r.stats()["n_items"] == len(ws[False])
    assert check_scene(pm, r, scene, ws, name == mc.NONFINITE, new_stream(), name) > 40


@pytest.mark.gpu
def test_snap_answers_go_in_without_a_read_back(pm, measure_renderer):
    """pm_snap_device's edge and vertex records, rearranged on the device into edge queries, into pm_positions_on_edges_device: what
    np_measure says of the snap answers read back afterwards."""
    scene = mc.scene_of(pm, "compound")
    r = measure_renderer
    r.set_scene_bytes(scene)
    ws = mc.expected_walks(pm, "compound")
    rng = np.random.default_rng(5)
    pts = np.concatenate([[sg[1] for w in ws for sg in w.segs[:: max(len(w.segs) // 5, 1)]], rng.uniform(0, 250, (40, 2))]).astype(F32)
    pts[::2] += F32(0.75)
    xyr = np.concatenate([pts, np.full((len(pts), 1), 6.0, F32)], axis=1).astype(F32)
    for vertices, edges in ((True, False), (False, True), (True, True)):
        if _emulated():
            snap = np.zeros((len(xyr), 8), np.int32)
            flags = (pm._lib.PM_SNAP_VERTICES if vertices else 0) | (pm._lib.PM_SNAP_EDGES if edges else 0)
            pm._lib.check(pm._lib.load().pm_snap_device(r._h, xyr.ctypes.data, len(xyr), flags, None, 0, snap.ctypes.data, None), "pm_snap_device")
            r.sync()
            q = np.ascontiguousarray(np.stack([snap[:, 0], snap[:, 2], snap[:, 3], np.zeros(len(snap), np.int32)], axis=1))
        else:
            import torch

            snap = torch.zeros((len(xyr), 8), dtype=torch.int32, device="cuda")
            r.snap_tensor(torch.from_numpy(xyr).cuda(), snap, vertices=vertices, edges=edges)
            q = torch.stack([snap[:, 0], snap[:, 2], snap[:, 3], torch.zeros_like(snap[:, 0])], dim=1).contiguous()
        out, keep = device_positions(pm, r, q)
        r.sync()
        rec = as_rec(snap, pm.renderer.SNAP_DTYPE)
        found = rec["item"] != nm.HIT_NONE
        assert found.sum() >= 10 and (~found).any()
        # a vertex of a Fill is named by its entry, which is the segment that starts there: t = 0 on it
        want = nm.positions_on_edges(scene, list(zip(rec["item"], rec["index"], rec["t"])), ws=ws)
        got = as_rec(out, nm.LENGTH_AT, len(rec))
        assert same(got, want), differing(got, want)[:6]
        assert (got["item"][found] != nm.HIT_NONE).all() and (got["item"][~found] == nm.HIT_NONE).all()


def _device_scene_matches(pm, r, what):
    scene = r.download_scene()
    ws = {skip: nm.walks(scene, skip) for skip in (False, True)}
    check_scene(pm, r, scene, ws, False, None, what)
    return scene, ws[False]


@pytest.mark.gpu
def test_lengths_follow_reflatten_groups(pm):
    """A random path set in three groups: after the flatten, and after reflatten_groups with a translation, a uniform scale by 2 and a
    rotation, every record equals np_measure on the downloaded scene; path_lengths sums them per path; the translated group keeps its
    lengths to rounding and the scaled one doubles them."""
    import path_sets
    from test_groups_gpu import rot

    ps = path_sets.random_case(321).ps
    gmap = (np.arange(len(ps.paths), dtype=np.uint32) % 3).astype(np.uint32)
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 32.0, -16.0), (2.0, 0.0, 0.0, 2.0, 5.0, 5.0), rot(0.7, 1.0, 40.0, 30.0)])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), 1.0)
        _, ws0 = _device_scene_matches(pm, r, "flattened")
        of_item = r.item_paths()
        lengths, counts = r.path_lengths()
        rec = r.item_lengths()
        assert sum(counts) == len(of_item) and lengths == [int(sum(int(v) for v in rec["length"][of_item == p])) for p in range(len(lengths))]
        first = np.array(lengths, np.float64)
        r.reflatten_groups(aff, np.array([1.0, 2.0, 1.0], F32))
        _, ws1 = _device_scene_matches(pm, r, "moved")
        moved = np.array(r.path_lengths()[0], np.float64)
        g = gmap[: len(moved)]
        # (the subdivision of a curve depends on its scale: a flattened curve's length is only near twice the other's)
        assert np.allclose(moved[g == 0], first[g == 0], rtol=1e-3) and np.allclose(moved[g == 1], 2.0 * first[g == 1], rtol=2e-2) and first.sum() > 0
        r.set_scene_bytes(mc.scene_of(pm, "degenerate"))
        with pytest.raises(pm._lib.PietMetalError):
            r.path_lengths()                                             # a scene that came from bytes has no paths


@pytest.mark.gpu
def test_lengths_of_styled_and_dashed_strokes(pm):
    """Outlined strokes with caps, joins and miter spikes, half of them dashed: the items are outline Fills, and the numbers are
    np_measure's of the device's own scene."""
    from np_stroke import MITER, SQUARE, style_bits
    from test_stroke_gpu import shapes

    ps = shapes(lambda k: (3 if k % 4 == 0 else 2) | style_bits(SQUARE, MITER))
    ps = ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps, (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 1.0)
        scene, ws = _device_scene_matches(pm, r, "styled")
        rec = r.item_lengths()
        assert (rec["kind"] == nm.CLOSED).sum() >= len(ps.paths) and (rec["length"] > 0).sum() >= len(ps.paths) and rec["n_segments"].max() > 64


@pytest.mark.gpu
def test_capacity_and_argument_rules(pm):
    lib = pm._lib.load()
    L = pm._lib
    OK = L.PM_OK
    with pm.Renderer(0) as r:
        n_items = C.c_uint32(77)
        lens = np.full((4, 4), UNTOUCHED, np.int32)
        pts = np.full((4, 8), UNTOUCHED, np.int32)
        pos = np.full((4, 4), UNTOUCHED, np.int32)
        lq = length_queries([(0, 0), (0, 5 * 65536), (0, 1 << 40), (7, 0)])
        eq = edge_query_records([(0, 0, 0.5), (0, 1, 1.0), (0, 9, 0.5), (7, 0, 0.0)])
        lp, pp, op, lqp, eqp = lens.ctypes.data, pts.ctypes.data, pos.ctypes.data, lq.ctypes.data, eq.ctypes.data
        items = [lambda flags, out, cap: lib.pm_item_lengths(r._h, flags, out, cap, None), lambda flags, out, cap: lib.pm_item_lengths_device(r._h, flags, out, cap, None)]
        per_query = [(lambda *a: lib.pm_points_at_length(r._h, *a), lqp, pp), (lambda *a: lib.pm_points_at_length_device(r._h, *a, None), lqp, pp),
                     (lambda *a: lib.pm_positions_on_edges(r._h, *a), eqp, op), (lambda *a: lib.pm_positions_on_edges_device(r._h, *a, None), eqp, op)]
        # no resident scene
        for call in items:
            assert call(0, lp, 4) == INVALID
        assert lib.pm_item_lengths(r._h, 0, lp, 4, C.byref(n_items)) == INVALID and n_items.value == 0
        for call, q, out in per_query:                    # (q, n, flags, out)
            assert call(q, 4, 0, out) == INVALID
        # a 3-4-5 Polyline of two segments and a Circle
        scene = hs._encode(pm, 2, lambda e: (e.polyline(np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 10.0]]), 0x112233FF, 1.0), e.circle((50.0, 50.0), 5.0)))
        r.set_scene_bytes(scene)
        assert r.stats()["n_items"] == 2
        for call in items:
            assert call(2, lp, 4) == INVALID                                   # unknown flag bits
            assert call(8, lp, 4) == INVALID
            assert call(0x80000001, lp, 4) == INVALID
            assert call(0, lp, 1) == CAPACITY                                  # too small: nothing is written
            assert call(0, None, 0) == CAPACITY
            assert call(0, None, 4) == INVALID                                 # a NULL out
        n_items.value = 77
        assert lib.pm_item_lengths(r._h, 0, None, 0, C.byref(n_items)) == CAPACITY and n_items.value == 2
        assert lib.pm_item_lengths_device(r._h, 0, lp + 4, 4, None) == INVALID  # not 8-byte aligned
        for call, q, out in per_query:
            assert call(q, 4, 2, out) == INVALID                               # unknown flag bits
            assert call(q, 4, 6, out) == INVALID                               # pm_snap's
            assert call(q, 4, 8, out) == INVALID                               # the stack calls'
            assert call(q, 0, 2, out) == INVALID                               # ... also with nothing to do
            assert call(None, 4, 0, out) == INVALID                            # a NULL pointer with n > 0
            assert call(q, 4, 0, None) == INVALID
            assert call(None, 0, 0, None) == OK                                # nothing to do
            assert call(q, 0, 1, out) == OK
        assert lib.pm_points_at_length_device(r._h, lqp + 4, 1, 0, pp, None) == INVALID      # not 8-byte aligned
        assert lib.pm_positions_on_edges_device(r._h, eqp, 1, 0, op + 4, None) == INVALID
        bad_l, bad_e = lq.copy(), eq.copy()
        bad_l["reserved"][2] = 1
        bad_e["reserved"][3] = 0x80000000
        assert lib.pm_points_at_length(r._h, bad_l.ctypes.data, 4, 0, pp) == INVALID          # a reserved word that is not 0
        assert lib.pm_positions_on_edges(r._h, bad_e.ctypes.data, 4, 0, op) == INVALID
        r.sync()
        assert (lens == UNTOUCHED).all() and (pts == UNTOUCHED).all() and (pos == UNTOUCHED).all()
        # correct calls afterwards, derived by hand: lengths 5 + 6 px; 5 px along is the middle vertex, as the start of segment 1
        assert items[0](1, lp, 4) == OK and (lens[2:] == UNTOUCHED).all()
        got = lens[:2].view(nm.ITEM_LENGTH).reshape(-1)
        assert got.tolist() == [(11 * 65536, 2, nm.OPEN), (0, 0, nm.NONE)]
        assert per_query[0][0](lqp, 3, 0, pp) == OK and (pts[3:] == UNTOUCHED).all()
        p = pts[:3].view(nm.LENGTH_POINT).reshape(-1)
        assert p[0].tolist() == (0, nm.FOUND, 0, 0.0, 0.0, 0.0, F32(0.6), F32(0.8))
        assert p[1].tolist() == (0, nm.FOUND, 1, 0.0, 3.0, 4.0, 0.0, 1.0)
        assert p[2].tolist() == (0, nm.FOUND | nm.CLAMPED, 1, 1.0, 3.0, 10.0, 0.0, 1.0)
        assert per_query[2][0](eqp, 4, 0, op) == OK
        a = pos.view(nm.LENGTH_AT).reshape(-1)
        assert a.tolist() == [(int(2.5 * 65536), 0, nm.FOUND), (11 * 65536, 0, nm.FOUND), (0, nm.HIT_NONE, 0), (0, nm.HIT_NONE, 0)]
        # the _device variants cannot look at a reserved word: such a query answers "none"
        dp, keep1 = device_points(pm, r, bad_l, pad=0)
        de, keep2 = device_positions(pm, r, bad_e, pad=0)
        r.sync()
        assert as_rec(dp, nm.LENGTH_POINT)["item"].tolist() == [0, 0, nm.HIT_NONE, nm.HIT_NONE] and not host_view(dp)[2:, 1:].any()
        assert as_rec(de, nm.LENGTH_AT)["item"].tolist() == [0, 0, nm.HIT_NONE, nm.HIT_NONE]
        assert lib.pm_abi_version() == 600
        # the Python wrappers
        assert r.item_lengths().dtype == pm.renderer.ITEM_LENGTH_DTYPE and len(r.item_lengths()) == 2
        at = r.points_at_length([0, 0, 0, 1], [2.5, -1.0, np.nan, 1.0])
        assert at["x"].tolist() == [1.5, 0.0, 0.0, 0.0] and at["y"].tolist() == [2.0, 0.0, 0.0, 0.0] and at["item"].tolist() == [0, 0, 0, nm.HIT_NONE]
        half = r.points_at_fraction([0, 0, 0], [0.0, 0.5, 1.0])
        assert half["index"].tolist() == [0, 1, 1] and half["y"].tolist() == [0.0, 4.5, 10.0] and half["status"].tolist() == [1, 1, 1]
        assert len(r.points_at_length([], [])) == 0 and len(r.positions_on_edges([], [], [])) == 0
        with pytest.raises(ValueError):
            r.points_at_length([0, 0], [1.0, 2.0, 3.0])
        with pytest.raises(ValueError):
            r.points_at_fraction([[0]], [0.5])
        with pytest.raises(pm._lib.PietMetalError):
            r.path_lengths()                                                    # as item_paths: the scene did not come from paths
        assert pm.renderer.length_units(2.5) == 163840 and pm.renderer.length_units(1e30) == (1 << 64) - 1
        if not _emulated():
            import torch

            o8 = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
            q4 = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
            with pytest.raises(TypeError):
                r.item_lengths_tensor(torch.zeros((2, 4), dtype=torch.int32))                 # not on the device
            with pytest.raises(TypeError):
                r.item_lengths_tensor(torch.zeros((2, 4), device="cuda"))                     # float32
            with pytest.raises(TypeError):
                r.points_at_length_tensor(q4, o8[:1])
            with pytest.raises(TypeError):
                r.points_at_length_tensor(q4[:, :3], o8)
            with pytest.raises(TypeError):
                r.positions_on_edges_tensor(q4, o8)
            with pytest.raises(pm._lib.PietMetalError):
                r.item_lengths_tensor(q4[:1])                                                 # capacity
            r.item_lengths_tensor(q4)
            r.points_at_length_tensor(q4, o8)
            r.sync()
            assert q4.cpu().numpy().view(nm.ITEM_LENGTH).reshape(-1)["length"].tolist() == [11 * 65536, 0]


@pytest.mark.gpu
def test_a_scene_without_items(pm, measure_renderer):
    """n_items == 0: pm_item_lengths writes nothing; every point and position query answers "none"."""
    lib = pm._lib.load()
    r = measure_renderer
    r.set_scene_bytes(hs._encode(pm, 0, lambda e: None))
    assert r.stats()["n_items"] == 0
    n_items = C.c_uint32(77)
    lens = np.full((2, 4), UNTOUCHED, np.int32)
    assert lib.pm_item_lengths(r._h, 0, lens.ctypes.data, 2, C.byref(n_items)) == pm._lib.PM_OK and n_items.value == 0
    assert lib.pm_item_lengths(r._h, 0, None, 0, None) == pm._lib.PM_OK
    dev = device_lengths(pm, r, 2)
    assert len(r.item_lengths()) == 0
    got = r.points_at_units([0, 0xFFFFFFFF], [0, 7])
    assert got["item"].tolist() == [nm.HIT_NONE] * 2 and not got.view(np.uint32).reshape(2, 8)[:, 1:].any()
    back = r.positions_on_edges([0, 5], [0, 0], [0.0, 1.0])
    assert back["item"].tolist() == [nm.HIT_NONE] * 2 and back["s"].tolist() == [0, 0]
    r.sync()
    assert (lens == UNTOUCHED).all() and (host_view(dev) == UNTOUCHED).all()


@pytest.mark.gpu
def test_queries_between_frames_and_after_a_replacement(pm, pmo):
    """Frames rendered before and after measure queries have the bytes they have without them; device calls on a caller's stream
    followed at once by a re-flatten answer for the scene resident at the call; a replacement between two queries gives each its own."""
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        ws = nm.walks(scene)
        want_len = nm.item_lengths(scene, ws=ws)
        longest = int(np.argmax(want_len["length"]))
        pairs = [(i, int(want_len["length"][i]) // 3) for i in range(0, len(ws), 7)] + [(longest, int(want_len["length"][longest]) - 1)]
        want_pts = nm.points_at_length(scene, pairs, ws=ws)
        r.render()
        s = new_stream()
        dev_len = device_lengths(pm, r, len(ws), stream=s)           # behind the frame, not waited for
        dev_pts, keep = device_points(pm, r, length_queries(pairs), stream=s)
        first = r.read_pixels()
        r.render()
        host = r.item_lengths()
        second = r.read_pixels()
        assert np.array_equal(first, want_px) and np.array_equal(second, want_px)
        wait(r, s)
        assert same(as_rec(dev_len, nm.ITEM_LENGTH), want_len) and same(host, want_len)
        assert same(as_rec(dev_pts, nm.LENGTH_POINT, len(pairs)), want_pts) and (want_pts["status"] == nm.FOUND).sum() > 20
        r.render()
        dev_pts, keep = device_points(pm, r, length_queries(pairs), stream=s)    # frame in flight, query, replacement, query
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        dev_after = device_lengths(pm, r, len(ws), stream=s)
        wait(r, s)
        assert same(as_rec(dev_pts, nm.LENGTH_POINT, len(pairs)), want_pts)
        after = nm.item_lengths(r.download_scene())
        assert same(as_rec(dev_after, nm.ITEM_LENGTH), after) and same(r.item_lengths(), after) and not same(after, want_len)


@pytest.mark.gpu
def test_cli_lengths_and_point_at(pm, tmp_path, capsys):
    """--lengths prints one JSON line, per path its length in px and its item count; --point-at ITEM,DIST prints the point, the
    tangent, the segment index and the path, one line each."""
    from piet_metal_amd import cli

    wl = pm.workloads.tiger(480, 270)
    asks = [(0, 10.0), (5, 0.0), (40, 1e9), (100000, 3.0)]
    args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--lengths"]
    for i, d in asks:
        args += ["--point-at", f"{i},{d:g}"]
    assert cli.main(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        lengths, counts = r.path_lengths()
        pts = r.points_at_length([a[0] for a in asks], [a[1] for a in asks])
        of_item = r.item_paths()
    got = json.loads(next(ln for ln in lines if ln.startswith("{")))
    assert got == {"paths": [{"length": v / 65536, "n_items": c} for v, c in zip(lengths, counts)]} and len(lengths) > 100
    want = []
    for (i, d), p in zip(asks, pts):
        head = f"item {i} at {d:g}: "
        if p["item"] == nm.HIT_NONE:
            want.append(head + "none")
        else:
            want.append(head + f"point {float(p['x']):g},{float(p['y']):g} tangent {float(p['tx']):g},{float(p['ty']):g} segment {int(p['index'])} "
                               f"t {float(p['t']):g} path {int(of_item[i])}" + (" (clamped)" if p["status"] & nm.CLAMPED else ""))
    assert [ln for ln in lines if ln.startswith("item ")] == want and want[3].endswith("none") and want[2].endswith("(clamped)")


# ---- CPU: np_measure itself ------------------------------------------------------------------------------------------------------

def hand_scene(pm):
    """0: the Polyline (0, 0) - (3, 4) - (3, 10) - (11, 16): lengths 5, 6, 10.  1: the Fill (0, 0) - (6, 0) - (6, 8): 6, 8 and the closing
    10.  2: the Line (10, 10) - (40, 50): 50.  3: a Circle.  4: the compound Fill of the triangle (0, 0) - (30, 0) - (30, 40) (30, 40,
    50) and the square [100, 103] x [100, 104] (3, 4, 3, 4)."""
    def emit(e):
        e.polyline(np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 10.0], [11.0, 16.0]]), 0x112233FF, 1.0)
        e.fill(np.array([[0.0, 0.0], [6.0, 0.0], [6.0, 8.0]]), 0x112233FF)
        e.stroke_line((10.0, 10.0), (40.0, 50.0), 2.0, 0x11223300)
        e.circle((50.0, 50.0), 5.0)
        e.fill_compound([np.array([[0.0, 0.0], [30.0, 0.0], [30.0, 40.0]]), np.array([[100.0, 100.0], [103.0, 100.0], [103.0, 104.0], [100.0, 104.0]])], 0x112233FF)

    return hs._encode(pm, 5, emit)


def test_np_measure_against_hand_derived_lengths_and_points(pm):
    """Relation 2: on 3-4-5 geometry every Q_k and T is exact."""
    U = 65536
    scene = hand_scene(pm)
    ws = nm.walks(scene)
    assert nm.item_lengths(scene).tolist() == [(21 * U, 3, nm.OPEN), (24 * U, 3, nm.CLOSED), (50 * U, 1, nm.OPEN), (0, 0, nm.NONE), (134 * U, 7, nm.CLOSED)]
    assert nm.item_lengths(scene, True).tolist()[2] == (0, 0, nm.NONE)
    assert [[sg[3] // U for sg in w.segs] for w in ws] == [[5, 6, 10], [6, 8, 10], [50], [], [30, 40, 50, 3, 4, 3, 4]]
    assert [sg[0] for sg in ws[4].segs] == [0, 1, 2, 4, 5, 6, 7]         # entry 3 is the first sub-path's separator
    F, Cl = nm.FOUND, nm.CLAMPED
    cases = [   # (item, s) -> (item, status, index, t, x, y, tx, ty)
        ((0, 0), (0, F, 0, 0.0, 0.0, 0.0, F32(0.6), F32(0.8))),
        ((0, int(2.5 * U)), (0, F, 0, 0.5, 1.5, 2.0, F32(0.6), F32(0.8))),
        ((0, 5 * U), (0, F, 1, 0.0, 3.0, 4.0, 0.0, 1.0)),                 # a vertex belongs to the segment that starts there
        ((0, 5 * U - 1), (0, F, 0, F32((5 * U - 1) / (5 * U)), F32(3.0 * ((5 * U - 1) / (5 * U))), F32(4.0 * ((5 * U - 1) / (5 * U))), F32(0.6), F32(0.8))),
        ((0, 8 * U), (0, F, 1, 0.5, 3.0, 7.0, 0.0, 1.0)),
        ((0, 16 * U), (0, F, 2, 0.5, 7.0, 13.0, F32(0.8), F32(0.6))),
        ((0, 21 * U), (0, F, 2, 1.0, 11.0, 16.0, F32(0.8), F32(0.6))),
        ((0, 21 * U + 1), (0, F | Cl, 2, 1.0, 11.0, 16.0, F32(0.8), F32(0.6))),
        ((1, 19 * U), (1, F, 2, 0.5, 3.0, 4.0, F32(-0.6), F32(-0.8))),    # on the closing segment, back to (0, 0)
        ((1, (1 << 64) - 1), (1, F | Cl, 2, 1.0, 0.0, 0.0, F32(-0.6), F32(-0.8))),
        ((2, 25 * U), (2, F, 0, 0.5, 25.0, 30.0, F32(0.6), F32(0.8))),
        ((3, 0), (nm.HIT_NONE, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)),
        ((4, 120 * U), (4, F, 4, 0.0, 100.0, 100.0, 1.0, 0.0)),           # the second sub-path begins where the first one's 120 px end
        ((4, 125 * U), (4, F, 5, 0.5, 103.0, 102.0, 0.0, 1.0)),
        ((4, 100 * U), (4, F, 2, 0.6, 12.0, 16.0, F32(-0.6), F32(-0.8))),
        ((5, 0), (nm.HIT_NONE, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)),
    ]
    got = nm.points_at_length(scene, [c[0] for c in cases])
    want = np.array([c[1] for c in cases], nm.LENGTH_POINT)
    assert same(got, want), [(cases[k][0], got[k], want[k]) for k in differing(got, want)]
    assert nm.points_at_length(scene, [(2, 0)], True)["item"][0] == nm.HIT_NONE
    back = nm.positions_on_edges(scene, [(0, 0, 0.5), (0, 1, 0.0), (0, 2, 1.0), (0, 3, 0.0), (1, 2, 0.5), (4, 3, 0.5), (4, 4, 0.0), (4, 7, 1.0), (3, 0, 0.0),
                                         (0, 1, np.nan), (0, 1, -0.0), (0, 1, 1.0000001), (0, 1, -1e-9)])
    assert back.tolist() == [(int(2.5 * U), 0, F), (5 * U, 0, F), (21 * U, 0, F), (0, nm.HIT_NONE, 0), (19 * U, 1, F), (0, nm.HIT_NONE, 0), (120 * U, 4, F),
                             (134 * U, 4, F), (0, nm.HIT_NONE, 0), (0, nm.HIT_NONE, 0), (5 * U, 0, F), (0, nm.HIT_NONE, 0), (0, nm.HIT_NONE, 0)]


def test_np_measure_is_np_dash_on_open_polylines(pm):
    """Relation 1: for every poly-line of the committed dash_cases seeds, taken as an open Polyline, T and Q are np_dash.walk's and
    the point at any 0 <= s < T is np_dash._point(W, Q, s, end_rule=False)."""
    import dash_cases as dc
    import np_dash

    checked = vertices = 0
    for seed in dc.SEEDS:
        subs = [np.asarray(pts, np.float64).reshape(-1, 2) for _, pts, _, _, _ in dc.subpaths_of(dc.dash_case(seed)[0])]
        subs = [p for p in subs if len(p) >= 1]
        scene = hs._encode(pm, len(subs), lambda e: [e.polyline(p, 0x112233FF, 1.0) for p in subs], cap=1 << 20)
        ws = nm.walks(scene)
        rng = np.random.default_rng(seed)
        for i, (p, w) in enumerate(zip(subs, ws)):
            W, Q = np_dash.walk(p, False)
            T = int(Q[-1])
            assert w.T == T and [sg[3] for sg in w.segs] == [int(Q[k + 1] - Q[k]) for k in range(len(Q) - 1)]
            if T == 0:
                continue
            ss = {0, T - 1, T // 2} | {int(q) for q in Q[:-1] if q < T} | {int(q) - 1 for q in Q[1:] if q >= 1} | {int(v) for v in rng.integers(0, T, 4)}
            pairs = [(i, s) for s in sorted(ss)]
            got = nm.points_at_length(scene, pairs, ws=ws)
            for (_, s), rec in zip(pairs, got):
                want = np_dash._point(W, Q, s, False)
                assert rec["status"] == nm.FOUND and same(np.array([rec["x"], rec["y"]], F32), np.asarray(want, F32)), (seed, i, s, rec, want)
                vertices += int(rec["t"] == 0.0)
            checked += len(pairs)
    assert checked > 5000 and vertices > 1000


def test_round_trip_in_exact_integers(pm):
    """Relation 3 on np_measure's own answers for every finite case scene: s' == s where t is 0 or 1, else within ceil(q_k 2^-24) + 1."""
    exact = loose = 0
    for name in mc.SCENES:
        if name == mc.NONFINITE:
            continue
        scene = mc.scene_of(pm, name)
        ws = mc.expected_walks(pm, name)
        pairs = mc.point_queries(ws)
        pts = nm.points_at_length(scene, pairs, ws=ws)
        back = nm.positions_on_edges(scene, list(zip(pts["item"], pts["index"], pts["t"])), ws=ws)
        e, lo = round_trip_bound(ws, pairs, pts, back)
        exact, loose = exact + e, loose + lo
    assert exact > 300 and loose > 300, (exact, loose)


# ---- CPU: the cases are what they claim -----------------------------------------------------------------------------------------

def test_the_cases_are_what_they_claim(pm):
    lens = {name: nm.item_lengths(mc.scene_of(pm, name)) for name in mc.SCENES}
    idx = mc.NAMES
    # segment counts on both sides of the lane / wave threshold and of the 64-segment steps, as Polylines, Fills and compound Fills
    c = lens["counts"]
    for n in mc.SEG_COUNTS:
        assert c[idx["counts"][f"poly-{n}"]]["n_segments"] == n and c[idx["counts"][f"fill-{n}"]]["n_segments"] == n
        assert c[idx["counts"][f"compound-{max(n, 1)}"]]["n_segments"] == max(n, 1)
    assert {mc.LANE, mc.LANE + 1, 63, 64, 65, 66, 127, 128, 129, 200} <= set(mc.SEG_COUNTS)
    assert c[idx["counts"]["fill-0"]]["kind"] == nm.NONE and c[idx["counts"]["poly-0"]]["kind"] == nm.OPEN
    # item counts
    assert [len(lens[f"walk-{n}"]) for n in mc.WALK_SIZES] == [1, 64, 65]
    kinds = {int(k) for k in lens["walk-65"]["kind"]}
    assert kinds == {nm.NONE, nm.OPEN, nm.CLOSED}
    skipped = nm.item_lengths(mc.scene_of(pm, "walk-65"), True)
    assert (skipped["kind"] == nm.NONE).sum() > (lens["walk-65"]["kind"] == nm.NONE).sum() + 10
    # degenerate geometry
    d, di = lens["degenerate"], idx["degenerate"]
    ws = mc.expected_walks(pm, "degenerate")
    qs = lambda name: [sg[3] for sg in ws[di[name]].segs]  # noqa: E731
    assert qs("poly_repeat_start")[:2] == [0, 0] and qs("poly_repeat_middle")[1:3] == [0, 0] and qs("poly_repeat_end")[2:] == [0, 0]
    step = qs("poly_repeat_step_edge")
    assert step[62:66] == [0, 0, 0, 0] and step[61] > 0 and step[66] > 0 and len(step) == 69
    for name in ("poly_all_degenerate", "fill_all_degenerate", "line_zero_length"):
        assert d[di[name]]["length"] == 0 and d[di[name]]["n_segments"] > 0 and ws[di[name]].first is not None
    assert d[di["poly_one_point"]].tolist() == (0, 0, nm.OPEN) and ws[di["poly_one_point"]].first is not None
    assert d[di["fill_zero_points"]].tolist() == (0, 0, nm.NONE)
    assert d[di["circle"]]["kind"] == nm.NONE and d[di["ellipse"]]["kind"] == nm.NONE
    assert qs("fill_closing_degenerate")[-1] == 0 and qs("fill_closing_degenerate")[-2] > 0     # the last segment is not the last of a length
    sk = nm.item_lengths(mc.scene_of(pm, "degenerate"), True)
    for name in ("fill_transparent", "poly_transparent", "line_transparent", "compound_transparent"):
        assert d[di[name]]["length"] > 0 and sk[di[name]].tolist() == (0, 0, nm.NONE)
    # compound Fills
    cw, ci = mc.expected_walks(pm, "compound"), idx["compound"]
    seps = lambda name: sorted(set(range(mc.entry_counts(mc.scene_of(pm, "compound"))[ci[name]])) - {sg[0] for sg in cw[ci[name]].segs})  # noqa: E731
    assert len(seps("two")) == 2 and len(seps("three")) == 3
    assert seps("empty_sub_path") == [5, 6, 11] and seps("ends_before_step_edge")[0] == 63 and seps("ends_at_step_edge")[0] == 64
    assert cw[ci["only_separators"]].kind == nm.CLOSED and cw[ci["only_separators"]].first is None and not cw[ci["only_separators"]].segs
    # the cap
    k, ki = lens["caps"], idx["caps"]
    assert k[ki["line_below_cap"]]["length"] == (1 << 32) - 256 and k[ki["line_at_cap"]]["length"] == 1 << 32 == k[ki["line_above_cap"]]["length"]
    assert k[ki["poly_70_caps"]]["length"] == 70 << 32 == k[ki["fill_70_caps"]]["length"] and 70 << 32 > 1 << 38
    assert k[ki["poly_huge"]]["length"] == 3 << 32 and k[ki["poly_mixed"]]["length"] == (5 << 16) + (1 << 32) + (4 << 16)
    # the split of the one exception: no case scene but NONFINITE has a non-finite point on a segment, and that one has
    for name in mc.SCENES:
        loose = sum(nm.has_non_finite_end(w, sg[0]) for w in mc.expected_walks(pm, name) for sg in w.segs)
        if name == mc.NONFINITE:
            pairs = mc.point_queries(mc.expected_walks(pm, name))
            want = nm.points_at_length(mc.scene_of(pm, name), pairs)
            un = unpromised(mc.expected_walks(pm, name), want)
            assert loose >= 8 and un.any() and (~un).sum() > 20
        else:
            assert loose == 0, name
    # the queries: around Q_k at the step edges, T - 1, T, T + 1 and 2^64 - 1; every class of inverse query
    pairs = mc.point_queries(mc.expected_walks(pm, "counts"))
    pts = nm.points_at_length(mc.scene_of(pm, "counts"), pairs)
    assert {0, 1, 62, 63, 64, 65, 199} <= set(pts["index"].tolist()) and {1, 3, 5, 7} <= set(pts["status"].tolist())
    assert (1 << 64) - 1 in [p[1] for p in pairs] and (pts["item"] == nm.HIT_NONE).any()
    tri = mc.edge_queries(mc.scene_of(pm, "compound"), cw)
    back = nm.positions_on_edges(mc.scene_of(pm, "compound"), tri, ws=cw)
    assert (back["item"] == nm.HIT_NONE).any() and (back["item"] != nm.HIT_NONE).sum() > 50 and len(mc.TS) == 8


# ---- CPU: the header ----------------------------------------------------------------------------------------------------------

def test_the_header_and_the_record_sizes(pm):
    hdr = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    got = {k: int(v) for k, v in re.findall(r"^#define (PM_MEASURE_[A-Z]+|PM_ABI_VERSION|PM_HIT_SKIP_TRANSPARENT) (\d+)u", hdr, re.M)}
    assert got == {"PM_MEASURE_NONE": 0, "PM_MEASURE_OPEN": 1, "PM_MEASURE_CLOSED": 2, "PM_MEASURE_FOUND": 1, "PM_MEASURE_CLAMPED": 2, "PM_MEASURE_DEGENERATE": 4,
                   "PM_ABI_VERSION": 600, "PM_HIT_SKIP_TRANSPARENT": 1}
    L = pm._lib
    assert (L.PM_MEASURE_NONE, L.PM_MEASURE_OPEN, L.PM_MEASURE_CLOSED) == (nm.NONE, nm.OPEN, nm.CLOSED) == (0, 1, 2)
    assert (L.PM_MEASURE_FOUND, L.PM_MEASURE_CLAMPED, L.PM_MEASURE_DEGENERATE) == (nm.FOUND, nm.CLAMPED, nm.DEGENERATE) == (1, 2, 4)
    for name, size in (("pm_item_length", 16), ("pm_length_query", 16), ("pm_length_point", 32), ("pm_edge_query", 16), ("pm_length_at", 16)):
        assert re.search(r"\} " + name + r";\s*/\* " + str(size) + r" bytes \*/", hdr), name
    R = pm.renderer
    for mine, theirs in ((R.ITEM_LENGTH_DTYPE, nm.ITEM_LENGTH), (R.LENGTH_QUERY_DTYPE, nm.LENGTH_QUERY), (R.LENGTH_POINT_DTYPE, nm.LENGTH_POINT),
                         (R.EDGE_QUERY_DTYPE, nm.EDGE_QUERY), (R.LENGTH_AT_DTYPE, nm.LENGTH_AT)):
        assert mine == theirs
    kernels = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_measure.h")).read()
    assert f"kMeasureLane = {mc.LANE}u" in kernels and "kMeasureCap = 1ull << 32" in kernels
    host = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    assert "PM_MEASURE_NONE == pm::kMeasureNone" in host and "sizeof(pm_length_point) == 32" in host
    assert "pm_measure.h" in open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_query_common.h")).read().split("#pragma once")[0]
    for fn in ("pm_item_lengths", "pm_points_at_length", "pm_positions_on_edges"):
        assert f"int {fn}(" in hdr and f"int {fn}_device(" in hdr


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_measure_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- CPU: the compiler's listing -----------------------------------------------------------------------------------------------

def test_the_measure_kernels_use_no_scratch(tmp_path):
    """The three kernels of pm_measure.h by the flags the library is built with: no private segment, no LDS, and VGPRs within 128 (the
    bound of the bounds kernels' test).  The figures are printed (pytest -s) and stand in DESIGN.md 4.  Sizes only: the assembly is
    searched for no instruction."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    names = ("pm_item_lengths_kernel", "pm_points_at_length_kernel", "pm_positions_on_edges_kernel")
    found = set()
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        name = next((k for k in names if k in m.group(1)), None)
        if name is None:
            continue
        found.add(name)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"{name}: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and lds == 0, (name, scratch, vgpr, lds)
    assert len(found) == 3, found
    assert "-ffp-contract=off" in flags and "pm_measure.h" in mk     # (editing the header rebuilds the library)
