"""Trimming, pm_trim_items and pm_trim_items_device (decision D27): the piece of an item between two lengths, as poly-line runs.

No tolerance anywhere: vertices, untouched rows (the sentinel word test_measure.UNTOUCHED) and infos EQUAL as bytes to
tests/np_trim.py's, which is written from the decision's text in Python integers over np_measure's segment lists, through the host
call and the device call on a caller's stream, with and without PM_HIT_SKIP_TRANSPARENT.  The one exception: x, y of a CUT vertex on a
segment with a non-finite end, in the one scene measure_cases.NONFINITE.  tests/trim_cases.py builds the request lists.

-m gpu: every case scene (host call packed; device call with a sentinel row between any two requests and after the last) and a scene
without items; truncation and layout; the relations on the device's own answers; after a styled and dashed flatten and after
reflatten_groups; every argument error, n == 0, hand-derived answers and the Python wrappers; requests between frames in flight and
after a scene replacement; the CLI.
CPU: np_trim against hand-derived geometry; part boundaries in exact integers; the cases are what they claim; the header; the -m gpu
part against the wave64 emulation of the kernel; the compiler's listing."""
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
import np_resample as nr  # noqa: E402
import np_trim as nt  # noqa: E402
import resample_cases as rc  # noqa: E402
import test_measure as tm  # noqa: E402  (its helpers: buffers on the device or under the emulation, comparisons)
import trim_cases as tc  # noqa: E402

F32 = np.float32
UNTOUCHED = tm.UNTOUCHED
INVALID, CAPACITY = -1, -4
U = 65536
U64_MAX = (1 << 64) - 1
# case scenes, no items, truncation and layout, relations, groups, styled and dashed, argument rules, ordering, CLI
N_GPU_TESTS = len(tc.SCENES) + 8


# ---- the calls --------------------------------------------------------------------------------------------------------

def host_call(pm, r, q, skip, out_rows, out_cap=None):
    """pm_trim_items into UNTOUCHED buffers: (status, out int32 [out_rows, 4], info int32 [n + 1, 6])."""
    out = np.full((out_rows, 4), UNTOUCHED, np.int32)
    info = np.full((len(q) + 1, 6), UNTOUCHED, np.int32)
    st = pm._lib.load().pm_trim_items(r._h, q.ctypes.data, len(q), tm.skip_flag(pm, skip), out.ctypes.data, out_rows if out_cap is None else out_cap, info.ctypes.data)
    return st, out, info


def device_call(pm, r, q, skip, out_rows, out_cap, stream=None):
    """pm_trim_items_device, not waited for: (out [out_rows, 4], info [n + 1, 6], keep-alive)."""
    dq = tm.to_device(q)
    out, info = tm.blank(out_rows, 4), tm.blank(len(q) + 1, 6)
    if tm._emulated():
        pm._lib.check(pm._lib.load().pm_trim_items_device(r._h, dq.ctypes.data, len(q), tm.skip_flag(pm, skip), out.ctypes.data, out_cap, info.ctypes.data, None),
                      "pm_trim_items_device")
    else:
        r.trim_tensor(dq, out[:out_cap], info[: len(q)], stream=stream, skip_transparent=skip)
    return out, info, dq


def spread(reqs, caps):
    """The requests laid out with one free row between any two: [(item, mode, first, cap, s0, s1)] and the rows used."""
    out, at = [], 0
    for (item, mode, s0, s1), cap in zip(reqs, caps):
        out.append((item, mode, at, cap, s0, s1))
        at += cap + 1
    return out, at


def assert_buffer(got, writes, ws, exempt, what):
    """The int32 [rows, 4] buffer holds the writes and UNTOUCHED everywhere else.  Where `exempt` (only ever the non-finite scene) a CUT
    vertex on a segment with a non-finite end is compared in index and flags alone."""
    got = np.ascontiguousarray(tm.host_view(got)).copy()
    want = nt.expected_buffer(writes, len(got), UNTOUCHED)
    loose = nt.unpromised_rows(writes, ws)
    assert exempt or not loose, what
    if loose:
        got[loose, :2] = 0
        want[loose, :2] = 0
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, len(bad), [(int(k), got[k].view(nt.TRIM_VERTEX), want[k].view(nt.TRIM_VERTEX)) for k in bad[:6]])


def assert_infos(got, want, what):
    got = np.ascontiguousarray(tm.host_view(got))
    assert (got[len(want):] == UNTOUCHED).all(), (what, "info beyond n")
    g = got[: len(want)].view(nt.TRIM_INFO).reshape(-1)
    bad = tm.differing(g, want)
    assert bad.size == 0, (what, [(int(k), g[k], want[k]) for k in bad[:6]])


@pytest.fixture(scope="module")
def trim_renderer(pm):
    """Never resized: the requests need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


def check_requests(pm, r, scene, ws, reqs, skip, exempt, stream, what):
    """One request list (item, mode, s0, s1) on the resident scene, every piece given exactly the room it needs: the host call,
    packed, and the device call, spread.  Returns the number of vertices."""
    _, count_info, _ = nt.trim(scene, [(i, m, 0, 0, a, b) for i, m, a, b in reqs], skip, ws)
    caps = [int(c) for c in count_info["n_vertices"]]
    packed, total = nt.packed(reqs, caps)
    want, want_info, _ = nt.trim(scene, packed, skip, ws)
    laid, rows = spread(reqs, caps)
    want_dev, want_dev_info, _ = nt.trim(scene, laid, skip, ws)
    dev_out, dev_info, keep = device_call(pm, r, nt.records(laid), skip, rows + 2, rows + 1, stream)
    st, out, info = host_call(pm, r, nt.records(packed), skip, total + 2, total)
    assert st == pm._lib.PM_OK, (what, pm._lib.last_error())
    assert_buffer(out, want, ws, exempt, (what, skip, "host"))
    assert_infos(info, want_info, (what, skip, "host"))
    tm.wait(r, stream)
    assert_buffer(dev_out, want_dev, ws, exempt, (what, skip, "device"))
    assert_infos(dev_info, want_dev_info, (what, skip, "device"))
    assert tm.same(want_info, want_dev_info) and not (want_info["flags"] & nt.TRUNCATED).any()
    # the count pass: the same infos but for the truncated bit, and nothing written
    st, out, info = host_call(pm, r, nt.records([(i, m, 0, 0, a, b) for i, m, a, b in reqs]), skip, 2, 0)
    assert st == pm._lib.PM_OK and (out == UNTOUCHED).all()
    assert_infos(info, count_info, (what, skip, "count"))
    return total


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.SCENES)
def test_case_scenes(pm, trim_renderer, name):
    """Every case scene: the request lists of trim_cases on every item and the two indices beyond the scene -- host call, and device
    call on a caller's stream with a sentinel row in every gap."""
    scene = rc.scene_of(pm, name)
    r = trim_renderer
    r.set_scene_bytes(scene)
    stream = tm.new_stream()
    n = 0
    for skip in (False, True):
        ws = rc.expected_walks(pm, name, skip)
        assert r.stats()["n_items"] == len(ws)
        n += check_requests(pm, r, scene, ws, tc.requests(pm, name, skip), skip, name == mc.NONFINITE, stream, name)
    assert n > 100      # (the lone item of walk-1 is one the flag skips)


@pytest.mark.gpu
def test_a_scene_without_items(pm, trim_renderer):
    """n_items == 0: every valid request is the empty piece of an item without a walk."""
    r = trim_renderer
    r.set_scene_bytes(hs._encode(pm, 0, lambda e: None))
    assert r.stats()["n_items"] == 0
    q = nt.records([(0, nt.RANGE, 0, 3, 0, U64_MAX), (0xFFFFFFFF, nt.PART, 3, 2, 4, 7), (5, nt.RANGE, 5, 0, 0, 0)])
    st, out, info = host_call(pm, r, q, False, 6, 5)
    dev_out, dev_info, keep = device_call(pm, r, q, True, 6, 5)
    r.sync()
    for o, i in ((out, info), (tm.host_view(dev_out), tm.host_view(dev_info))):
        assert (o == UNTOUCHED).all() and (i[3:] == UNTOUCHED).all()
        assert i[:3].view(nt.TRIM_INFO).reshape(-1).tolist() == [(0, 0, 0, nm.NONE, nt.END_CLAMPED), (0, 0, 0, nm.NONE, 0), (0, 0, 0, nm.NONE, 0)]
    assert st == pm._lib.PM_OK and len(r.trim([0, 1], 0.0, np.inf)[0]) == 0


@pytest.mark.gpu
def test_truncation_and_layout(pm, trim_renderer):
    """Caps that cut a piece everywhere a cap can -- 0, 1, one short, between an A and its B, inside a step and at a step edge --,
    first + p across out_cap, a request at out_cap, first = 0xFFFFFFFF, caller-chosen firsts out of order, and every kind of invalid
    request among valid ones, whose ranges stay untouched."""
    name = "counts"
    scene = rc.scene_of(pm, name)
    ws = rc.expected_walks(pm, name)
    r = trim_renderer
    r.set_scene_bytes(scene)
    laid, cap, sizes = tc.layout_requests(pm)
    want, want_info, pieces = nt.trim(scene, laid, False, ws, out_cap=cap)
    kinds = [int(k) for k in want_info["kind"]]
    assert kinds.count(nt.INVALID) == 6 and max(want) == cap - 1 and not any(430 <= at < 480 for at in want) and 493 not in want and 492 in want
    assert [int(f) & nt.TRUNCATED for f in want_info["flags"]].count(nt.TRUNCATED) == 10
    for stream in (None, tm.new_stream()):
        out, info, keep = device_call(pm, r, nt.records(laid), False, cap + 4, cap, stream)
        tm.wait(r, stream)
        assert_buffer(out, want, ws, False, "layout")
        assert_infos(info, want_info, "layout")
    # the sweep: one piece under every cap around its step edge
    sweep = tc.truncation_sweep(pm)
    laid, rows = spread([q[:4] for q in sweep], [q[4] for q in sweep])
    want, want_info, _ = nt.trim(scene, laid, False, ws)
    out, info, keep = device_call(pm, r, nt.records(laid), False, rows + 1, rows)
    r.sync()
    assert_buffer(out, want, ws, False, "sweep")
    assert_infos(info, want_info, "sweep")
    assert [int(f) & nt.TRUNCATED for f in want_info["flags"]] == [1] * 9 + [0] * 2 and set(want_info["n_vertices"].tolist()) == {130}


def xyk(v):
    """x, y as bytes and the index of a vertex or a point record."""
    return v["x"].tobytes(), v["y"].tobytes(), int(v["index"])


def _count_then_fill(pm, r, reqs, skip=False, stream=None):
    """What a caller without a model does: the cap = 0 pass, then an exactly packed device call.  Returns (vertices TRIM_VERTEX
    [total], offsets, infos of the full call) and asserts that both passes count alike."""
    q0 = nt.records([(i, m, 0, 0, a, b) for i, m, a, b in reqs])
    _, info0, keep0 = device_call(pm, r, q0, skip, 1, 0, stream)
    tm.wait(r, stream)
    info0 = tm.as_rec(info0, nt.TRIM_INFO, len(reqs)).copy()
    caps = [int(c) for c in info0["n_vertices"]]
    packed, total = nt.packed(reqs, caps)
    out, info, keep = device_call(pm, r, nt.records(packed), skip, total + 1, total, stream)
    tm.wait(r, stream)
    info = tm.as_rec(info, nt.TRIM_INFO, len(reqs)).copy()
    assert info["n_vertices"].tolist() == caps and info["n_runs"].tolist() == info0["n_runs"].tolist() and not (info["flags"] & nt.TRUNCATED).any()
    assert ((info0["flags"] & nt.TRUNCATED) != 0).tolist() == [c > 0 for c in caps]
    out = tm.host_view(out)
    assert (out[total:] == UNTOUCHED).all()
    offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    return np.ascontiguousarray(out[:total]).view(nt.TRIM_VERTEX).reshape(-1), offsets, info


@pytest.mark.gpu
def test_the_relations_on_the_devices_own_answers(pm, trim_renderer):
    """D27's relations between device calls, without a model: a piece's first vertex is pm_points_at_length_device's answer at lo, its
    last the answer at hi (wherever hi is not the very start of a segment of a length, or is T); consecutive parts meet in equal
    bytes where the walk does not jump; the count pass counts what the full pass writes."""
    r = trim_renderer
    firsts = lasts = joints = 0
    for name in ("counts", "degenerate", "compound", "caps", rc.TINY):
        r.set_scene_bytes(rc.scene_of(pm, name))
        for skip in (False, True):
            reqs = tc.requests(pm, name, skip)[::3] + [q for q in tc.requests(pm, name, skip) if q[1] == nt.PART and q[3] in (1, 3, 7)]
            vs, offsets, infos = _count_then_fill(pm, r, reqs, skip)
            pairs, at = [], []
            for k, (item, mode, s0, s1) in enumerate(reqs):
                if offsets[k + 1] > offsets[k]:
                    lo, hi = nt.ends(mode, s0, s1, int(infos[k]["length"]))
                    pairs += [(item, lo), (item, hi)]
                    at.append(k)
            pts, keep = tm.device_points(pm, r, tm.length_queries(pairs), skip)
            r.sync()
            pts = tm.as_rec(pts, nm.LENGTH_POINT, len(pairs))
            for n, k in enumerate(at):
                head, tail, p_lo, p_hi = vs[offsets[k]], vs[offsets[k + 1] - 1], pts[2 * n], pts[2 * n + 1]
                assert xyk(head) == xyk(p_lo) and head["flags"] & nt.MOVE, (name, skip, reqs[k], head, p_lo)
                assert bool(head["flags"] & nt.CUT) == (float(p_lo["t"]) != 0.0)
                firsts += 1
                if float(p_hi["t"]) != 0.0:      # (t == 0 only at the very start of the located segment: 1 unit is 2^-32 of the longest)
                    assert xyk(tail) == xyk(p_hi), (name, skip, reqs[k], tail, p_hi)
                    assert tail["flags"] & nt.CUT or float(p_hi["t"]) == 1.0      # (a t64 one unit short of the end of a long segment rounds to the f32 1)
                    lasts += 1
            # consecutive parts: where the whole item's piece has no MOVE at the segment part j + 1 starts on, the two meet
            whole = {}
            for k, (item, mode, s0, s1) in enumerate(reqs):
                if mode == nt.PART and s1 == 1:
                    mine = vs[offsets[k]:offsets[k + 1]]
                    whole[item] = set(mine["index"][(mine["flags"] & nt.MOVE) != 0].tolist())
            where = {q: k for k, q in enumerate(reqs)}
            for (item, mode, j, m), k in where.items():
                k2 = where.get((item, mode, j + 1, m))
                if mode != nt.PART or k2 is None or offsets[k + 1] == offsets[k] or offsets[k2 + 1] == offsets[k2]:
                    continue
                tail, head = vs[offsets[k + 1] - 1], vs[offsets[k2]]
                if not head["flags"] & nt.CUT and int(head["index"]) in whole[item]:
                    continue                      # the walk jumps there
                assert xyk(tail)[:2] == xyk(head)[:2], (name, skip, item, j, m, tail, head)
                joints += 1
    assert firsts > 2000 and lasts > 2000 and joints > 500, (firsts, lasts, joints)      # (some 3 000 pieces that are not empty, 900 joints)


def _joined(parts):
    """The pieces of consecutive parts as one vertex list with the joints dropped: every CUT vertex goes, and the first vertex of a
    later part goes where it repeats (as f32 values) the vertex kept before it."""
    kept = []
    for n, part in enumerate(parts):
        for p, v in enumerate(part):
            if v["flags"] & nt.CUT:
                continue
            if n and p == 0 and kept and kept[-1]["x"] == v["x"] and kept[-1]["y"] == v["y"]:
                continue
            kept.append(v)
    return kept


def _flattened_scene_matches(pm, r, what):
    """Pieces equal np_trim on the downloaded scene; the m parts of every item of positive length concatenate to the whole piece."""
    scene = r.download_scene()
    ws = nm.walks(scene)
    reqs = []
    for i, w in enumerate(ws):
        reqs += [(i, nt.RANGE, 0, U64_MAX), (i, nt.RANGE, w.T // 3, w.T - w.T // 4), (i, nt.PART, i % 3, 3), (i, nt.RANGE, 3 * U // 2, 40 * U + 77)]
    reqs += [(len(ws), nt.PART, 0, 1)]
    check_requests(pm, r, scene, ws, reqs, False, False, tm.new_stream(), what)
    m = 5
    vs, offsets, infos = r.trim_parts(np.arange(len(ws)), m)
    whole, whole_offsets, whole_infos = r.trim(np.arange(len(ws)), 0.0, np.inf)
    joined = 0
    for i, w in enumerate(ws):
        assert int(whole_infos[i]["length"]) == w.T and int(whole_infos[i]["kind"]) == w.kind
        if w.T == 0:
            continue
        parts = [vs[offsets[i * m + j]:offsets[i * m + j + 1]] for j in range(m)]
        got = _joined(parts)
        want = whole[whole_offsets[i]:whole_offsets[i + 1]]
        assert len(got) == len(want) and all(xyk(g) == xyk(v) for g, v in zip(got, want)), (what, i)
        assert sum(len(run) for run in pm.renderer.trim_runs(want)) == len(want) and len(pm.renderer.trim_runs(want)) == int(whole_infos[i]["n_runs"])
        joined += 1
    return ws, joined


@pytest.mark.gpu
def test_trimming_follows_reflatten_groups(pm):
    import path_sets
    from test_groups_gpu import rot

    ps = path_sets.random_case(321).ps
    gmap = (np.arange(len(ps.paths), dtype=np.uint32) % 3).astype(np.uint32)
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 32.0, -16.0), (2.0, 0.0, 0.0, 2.0, 5.0, 5.0), rot(0.7, 1.0, 40.0, 30.0)])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), 1.0)
        ws0, n0 = _flattened_scene_matches(pm, r, "flattened")
        r.reflatten_groups(aff, np.array([1.0, 2.0, 1.0], F32))
        ws1, n1 = _flattened_scene_matches(pm, r, "moved")
        assert n0 > 5 and n0 == n1 and [w.T for w in ws0] != [w.T for w in ws1]


@pytest.mark.gpu
def test_trimming_styled_and_dashed_strokes(pm):
    from np_stroke import MITER, SQUARE, style_bits
    from test_stroke_gpu import shapes

    ps = shapes(lambda k: (3 if k % 4 == 0 else 2) | style_bits(SQUARE, MITER))
    ps = ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps, (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 1.0)
        ws, n = _flattened_scene_matches(pm, r, "styled")
        assert n >= len(ps.paths) and max(len(w.segs) for w in ws) > 64


@pytest.mark.gpu
def test_argument_rules(pm):
    """Every PM_ERR_INVALID and PM_ERR_CAPACITY case, each with nothing written; n == 0; correct calls afterwards, derived by hand;
    the Python wrappers and trim_runs."""
    lib = pm._lib.load()
    OK = pm._lib.PM_OK
    with pm.Renderer(0) as r:
        out = np.full((16, 4), UNTOUCHED, np.int32)
        info = np.full((5, 6), UNTOUCHED, np.int32)
        # the whole Polyline, [2.5, 8] px of it, its second half, the whole Circle
        good = nt.records(nt.packed([(0, nt.RANGE, 0, U64_MAX), (0, nt.RANGE, 5 * U // 2, 8 * U), (0, nt.PART, 1, 2), (1, nt.RANGE, 0, U64_MAX)], [3, 3, 2, 1])[0])
        op, ip, qp = out.ctypes.data, info.ctypes.data, good.ctypes.data
        host = lambda q, n, flags, o, cap, i: lib.pm_trim_items(r._h, q, n, flags, o, cap, i)  # noqa: E731
        dev = lambda q, n, flags, o, cap, i: lib.pm_trim_items_device(r._h, q, n, flags, o, cap, i, None)  # noqa: E731
        for call in (host, dev):                                   # no resident scene
            assert call(qp, 4, 0, op, 16, ip) == INVALID
        # a 3-4-5 Polyline of two segments (5 + 6 px) and a Circle
        r.set_scene_bytes(hs._encode(pm, 2, lambda e: (e.polyline(np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 10.0]]), 0x112233FF, 1.0), e.circle((50.0, 50.0), 5.0))))
        for call in (host, dev):
            for flags in (2, 6, 8, 0x80000001):                    # unknown flag bits, also with nothing to do
                assert call(qp, 4, flags, op, 16, ip) == INVALID and call(qp, 0, flags, op, 16, ip) == INVALID
            assert call(None, 4, 0, op, 16, ip) == INVALID         # a NULL pointer with n > 0
            assert call(qp, 4, 0, None, 16, ip) == INVALID
            assert call(qp, 4, 0, op, 16, None) == INVALID
            assert call(None, 0, 0, None, 0, None) == OK           # nothing to do
            assert call(qp, 0, 1, op, 16, ip) == OK
        assert dev(qp + 4, 1, 0, op, 16, ip) == INVALID            # not 8-byte aligned
        assert dev(qp, 1, 0, op + 4, 16, ip) == INVALID
        assert dev(qp, 1, 0, op, 16, ip + 4) == INVALID

        def bad(k, **fields):
            q = good.copy()
            for f, v in fields.items():
                q[f][k] = v
            return q

        for q in (bad(1, mode=2), bad(0, mode=0xFFFFFFFF), bad(1, s0=8 * U + 1), bad(0, s0=U64_MAX, s1=U64_MAX - 1), bad(2, s1=0), bad(2, s0=2), bad(2, s0=3, s1=2),
                  bad(2, s1=nt.MAX_PARTS + 1), bad(1, first=4), bad(0, first=1), bad(3, first=0), bad(3, first=9)):   # what the device would call invalid; a wrong first
            assert host(q.ctypes.data, 4, 0, op, 16, ip) == INVALID
        assert host(qp, 4, 0, op, 8, ip) == CAPACITY                # the total is 9
        assert host(qp, 4, 0, op, 0, ip) == CAPACITY
        big = nt.records(nt.packed([(0, nt.RANGE, 0, 1), (0, nt.RANGE, 0, 1)], [1 << 20, 1])[0])
        assert host(big.ctypes.data, 2, 0, op, (1 << 20) + 1, ip) == CAPACITY   # more than 2^20 records in one call
        r.sync()
        assert (out == UNTOUCHED).all() and (info == UNTOUCHED).all()
        # the count pass needs no buffer
        count = good.copy()
        count["first"] = 0
        count["cap"] = 0
        assert host(count.ctypes.data, 4, 0, None, 0, ip) == OK and (info[4:] == UNTOUCHED).all()
        T = 11 * U
        TR, EC = nt.TRUNCATED, nt.END_CLAMPED
        assert info[:4].view(nt.TRIM_INFO).reshape(-1).tolist() == [(T, 3, 1, nm.OPEN, TR | EC), (T, 3, 1, nm.OPEN, TR), (T, 2, 1, nm.OPEN, TR), (0, 0, 0, nm.NONE, EC)]
        # correct calls afterwards, derived by hand
        assert host(qp, 4, 0, op, 9, ip) == OK and (out[8:] == UNTOUCHED).all() and (info[4:] == UNTOUCHED).all()
        v = out[:8].view(nt.TRIM_VERTEX).reshape(-1)
        M, Ct = nt.MOVE, nt.CUT
        assert info[:4].view(nt.TRIM_INFO).reshape(-1).tolist() == [(T, 3, 1, nm.OPEN, EC), (T, 3, 1, nm.OPEN, 0), (T, 2, 1, nm.OPEN, 0), (0, 0, 0, nm.NONE, EC)]
        assert v.tolist() == [(0.0, 0.0, 0, M), (3.0, 4.0, 0, 0), (3.0, 10.0, 1, 0),          # the whole item: one run, the joint once
                              (1.5, 2.0, 0, M | Ct), (3.0, 4.0, 0, 0), (3.0, 7.0, 1, Ct),      # from half way up the first segment to half way up the second
                              (3.0, 4.5, 1, M | Ct), (3.0, 10.0, 1, 0)]                        # [5.5, 11] px
        # the Python wrappers
        R = pm.renderer
        vs, offsets, infos = r.trim([0, 0, 1, 7], [0.0, 2.5, 0.0, 0.0], [np.inf, 8.0, np.inf, 1.0])
        assert vs.dtype == R.TRIM_VERTEX_DTYPE and infos.dtype == R.TRIM_INFO_DTYPE and offsets.tolist() == [0, 3, 6, 6, 6]
        assert tm.same(vs, v[:6]) and infos["n_runs"].tolist() == [1, 1, 0, 0] and infos["flags"].tolist() == [EC, 0, EC, EC]
        vs, offsets, infos = r.trim_parts([0, 1], [2, 3])
        assert offsets.tolist() == [0, 3, 5, 5, 5, 5] and tm.same(vs[3:], v[6:8]) and vs[:3].tolist() == [(0.0, 0.0, 0, M), (3.0, 4.0, 0, 0), (3.0, 4.5, 1, Ct)]
        vs, offsets, infos = r.trim_units([0], 5 * U, [5 * U + 1])
        assert vs.tolist() == [(3.0, 4.0, 1, M), (3.0, F32(4.0 + 6.0 / (6 * U)), 1, Ct)]
        assert len(r.trim([], [], [])[0]) == 0 and r.trim_parts([], 3)[1].tolist() == [0]
        runs = R.trim_runs(np.concatenate([v[:3], v[6:8]]))
        assert [run.tolist() for run in runs] == [[[0.0, 0.0], [3.0, 4.0], [3.0, 10.0]], [[3.0, 4.5], [3.0, 10.0]]] and runs[0].dtype == np.float32 and R.trim_runs(v[:0]) == []
        for wrong in (lambda: r.trim([0, 0], [1.0], 2.0), lambda: r.trim([[0]], 0.0, 1.0), lambda: r.trim([0], 2.0, 1.0), lambda: r.trim_units([0], -1, 5),
                      lambda: r.trim_units([0], 0, 1 << 64), lambda: r.trim_parts([0], 0), lambda: r.trim_parts([0], nt.MAX_PARTS + 1), lambda: r.trim_parts([0, 0], [1]),
                      lambda: R.trim_runs(v[1:3])):
            with pytest.raises(ValueError):
                wrong()
        assert lib.pm_abi_version() == 600
        if not tm._emulated():
            import torch

            q8, o4, i6 = tm.to_device(good), torch.zeros((9, 4), dtype=torch.int32, device="cuda"), torch.zeros((4, 6), dtype=torch.int32, device="cuda")
            for wrong in (lambda: r.trim_tensor(q8.cpu(), o4, i6), lambda: r.trim_tensor(q8[:, :4].contiguous(), o4, i6), lambda: r.trim_tensor(q8, o4[:, :2].contiguous(), i6),
                          lambda: r.trim_tensor(q8, o4, i6[:2]), lambda: r.trim_tensor(q8, o4.float(), i6), lambda: r.trim_tensor(q8, o4, i6[:, :4].contiguous())):
                with pytest.raises(TypeError):
                    wrong()
            r.trim_tensor(q8, o4, i6)
            r.sync()
            assert tm.same(o4.cpu().numpy()[:8], out[:8]) and tm.same(i6.cpu().numpy(), info[:4])


@pytest.mark.gpu
def test_requests_between_frames_and_after_a_replacement(pm, pmo):
    """Frames rendered before and after trimming have the bytes they have without it; a device call on a caller's stream followed at
    once by a re-flatten answers for the scene resident at the call; a replacement between two requests gives each its own."""
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        ws = nm.walks(scene)
        longest = max(range(len(ws)), key=lambda i: ws[i].T)
        reqs = [(i, nt.PART, 1, 3) for i in range(0, len(ws), 9)] + [(longest, nt.RANGE, U // 2, ws[longest].T - U // 3), (longest, nt.RANGE, 0, U64_MAX)]
        _, count_info, _ = nt.trim(scene, [(i, m, 0, 0, a, b) for i, m, a, b in reqs], False, ws)
        caps = [int(c) + 2 for c in count_info["n_vertices"]]          # room to spare: a piece of the replaced scene may be longer
        packed, total = nt.packed(reqs, caps)
        q = nt.records(packed)
        want, want_info, _ = nt.trim(scene, packed, False, ws)
        r.render()
        s = tm.new_stream()
        dev_out, dev_info, keep = device_call(pm, r, q, False, total + 1, total, s)     # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        st, out, info = host_call(pm, r, q, False, total + 1, total)
        second = r.read_pixels()
        assert st == pm._lib.PM_OK and np.array_equal(first, want_px) and np.array_equal(second, want_px)
        tm.wait(r, s)
        for o, i in ((out, info), (dev_out, dev_info)):
            assert_buffer(o, want, ws, False, "between frames")
            assert_infos(i, want_info, "between frames")
        assert len(ws[longest].segs) > 128 and int(want_info["n_vertices"][-1]) > 128
        r.render()
        dev_out, dev_info, keep = device_call(pm, r, q, False, total + 1, total, s)     # frame in flight, request, replacement, request
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        after_out, after_info, keep2 = device_call(pm, r, q, False, total + 1, total, s)
        tm.wait(r, s)
        assert_buffer(dev_out, want, ws, False, "before the replacement")
        assert_infos(dev_info, want_info, "before the replacement")
        scene2 = r.download_scene()
        ws2 = nm.walks(scene2)
        want2, want_info2, _ = nt.trim(scene2, packed, False, ws2)
        assert_buffer(after_out, want2, ws2, False, "after the replacement")
        assert_infos(after_info, want_info2, "after the replacement")
        assert not tm.same(want_info, want_info2)


@pytest.mark.gpu
def test_cli_trim_and_trim_parts(pm, tmp_path, capsys):
    """--trim ITEM,START,END and --trim-parts ITEM,M: a header line per piece, then one line per vertex."""
    from piet_metal_amd import cli

    wl = pm.workloads.tiger(480, 270)
    args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--trim", "40,2.5,30", "--trim", "100000,0,inf", "--trim", "5,0,inf", "--trim-parts", "40,3"]
    assert cli.main(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("trim ", "  move ", "  line "))]
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        want = []
        vs, offsets, infos = r.trim([40, 100000, 5], [2.5, 0.0, 0.0], [30.0, np.inf, np.inf])
        for k, (i, a, b) in enumerate(((40, "2.5", "30"), (100000, "0", "inf"), (5, "0", "inf"))):
            want.append(f"trim item {i} [{a}, {b}]: length {int(infos[k]['length']) / 65536:g} vertices {int(infos[k]['n_vertices'])} runs {int(infos[k]['n_runs'])}")
            want += [cli.vertex_line(v) for v in vs[offsets[k]:offsets[k + 1]]]
        assert want[0].endswith("runs 1") and " (cut)" in want[1] and want[1].startswith("  move ") and int(infos[0]["n_vertices"]) >= 2
        vs, offsets, infos = r.trim_parts([40], 3)
        T = int(infos[0]["length"])
        bs = pm.renderer.resample_positions(1, 4, T, nm.OPEN)
        for j in range(3):
            want.append(f"trim item 40 [{bs[j] / 65536:g}, {bs[j + 1] / 65536:g}]: length {T / 65536:g} vertices {int(infos[j]['n_vertices'])} runs {int(infos[j]['n_runs'])}")
            want += [cli.vertex_line(v) for v in vs[offsets[j]:offsets[j + 1]]]
    assert lines == want and f"trim item 100000 [0, inf]: length 0 vertices 0 runs 0" in want and len(want) > 20
    for wrong in (["--trim", "40"], ["--trim", "40,1"], ["--trim", "40,2,1"], ["--trim", "40,-1,2"], ["--trim", "40,1,2,3"], ["--trim-parts", "40"], ["--trim-parts", "40,0"],
                  ["--trim-parts", "40,2,3"], ["--trim-parts", "-1,2"]):
        with pytest.raises(SystemExit):
            cli.main(args[:6] + wrong)
    capsys.readouterr()


# ---- CPU: np_trim itself ---------------------------------------------------------------------------------------------------------

def test_np_trim_against_hand_derived_geometry(pm):
    """tests/test_measure.py's hand scene: the Polyline 5 + 6 + 10 px, the Fill 6 + 8 + 10 px, the Line of 50 px, a Circle, the compound
    Fill of a 30-40-50 triangle and a 3 x 4 square."""
    scene = tm.hand_scene(pm)
    ws = nm.walks(scene)
    M, Ct = nt.MOVE, nt.CUT
    TR, EC = nt.TRUNCATED, nt.END_CLAMPED
    reqs = [
        (0, nt.RANGE, 0, U64_MAX),                      # the open Polyline, whole
        (0, nt.RANGE, 2 * U, 18 * U),                   # 2 px up its first segment to 7 px along its last
        (0, nt.RANGE, 5 * U, 11 * U),                   # from vertex to vertex: its middle segment alone, nothing cut
        (0, nt.PART, 1, 3),                             # [7, 14] px
        (1, nt.RANGE, 0, U64_MAX),                      # the closed Fill, whole: ends where it began
        (1, nt.PART, 3, 4),                             # [18, 24] px: the last 6 px of the closing segment
        (1, nt.RANGE, 3 * U, 3 * U),                    # empty
        (2, nt.RANGE, 25 * U, 100 * U),                 # the second half of the Line
        (3, nt.RANGE, 0, U64_MAX),                      # the Circle
        (4, nt.RANGE, 100 * U, 127 * U),                # the compound Fill: the triangle's last 20 px (from (12, 16) home), the walk jumps, the square's first 7 px
        (4, nt.RANGE, 120 * U, 120 * U + 1),            # the first unit of the square
        (4, nt.PART, 0, 1),                             # whole: two runs
    ]
    caps = [9] * len(reqs)
    packed, total = nt.packed(reqs, caps)
    writes, infos, pieces = nt.trim(scene, packed, False, ws)
    want = [
        [(0.0, 0.0, 0, M), (3.0, 4.0, 0, 0), (3.0, 10.0, 1, 0), (11.0, 16.0, 2, 0)],
        [(F32(1.2), F32(1.6), 0, M | Ct), (3.0, 4.0, 0, 0), (3.0, 10.0, 1, 0), (F32(8.6), F32(14.2), 2, Ct)],
        [(3.0, 4.0, 1, M), (3.0, 10.0, 1, 0)],
        [(3.0, 6.0, 1, M | Ct), (3.0, 10.0, 1, 0), (F32(5.4), F32(11.8), 2, Ct)],
        [(0.0, 0.0, 0, M), (6.0, 0.0, 0, 0), (6.0, 8.0, 1, 0), (0.0, 0.0, 2, 0)],
        [(F32(3.6), F32(4.8), 2, M | Ct), (0.0, 0.0, 2, 0)],
        [],
        [(25.0, 30.0, 0, M | Ct), (40.0, 50.0, 0, 0)],
        [],
        [(12.0, 16.0, 2, M | Ct), (0.0, 0.0, 2, 0), (100.0, 100.0, 4, M), (103.0, 100.0, 4, 0), (103.0, 104.0, 5, 0)],
        [(100.0, 100.0, 4, M), (F32(100.0 + 3.0 / (3 * U)), 100.0, 4, Ct)],
        [(0.0, 0.0, 0, M), (30.0, 0.0, 0, 0), (30.0, 40.0, 1, 0), (0.0, 0.0, 2, 0), (100.0, 100.0, 4, M), (103.0, 100.0, 4, 0), (103.0, 104.0, 5, 0), (100.0, 104.0, 6, 0),
         (100.0, 100.0, 7, 0)],
    ]
    for k, (got, exp) in enumerate(zip(pieces, want)):
        assert tm.same(nt.as_records(got), nt.as_records(exp)), (k, got, exp)
    kinds = [nm.OPEN] * 4 + [nm.CLOSED] * 3 + [nm.OPEN, nm.NONE] + [nm.CLOSED] * 3
    Ts = [21 * U] * 4 + [24 * U] * 3 + [50 * U, 0] + [134 * U] * 3
    flags = [EC, 0, 0, 0, EC, 0, 0, EC, EC, 0, 0, 0]
    runs = [1, 1, 1, 1, 1, 1, 0, 1, 0, 2, 1, 2]
    assert infos.tolist() == [(T, len(p), n, kind, f) for T, p, n, kind, f in zip(Ts, want, runs, kinds, flags)]
    assert sorted(writes) == [9 * k + p for k, p_ in enumerate(want) for p in range(len(p_))]
    # a cap cuts, and says so; beyond out_cap nothing is written
    writes, infos, _ = nt.trim(scene, [(0, nt.RANGE, 4, 3, 0, U64_MAX), (4, nt.PART, 6, 9, 0, 1)], False, ws, out_cap=8)
    assert sorted(writes) == [4, 5, 6, 7] and infos["flags"].tolist() == [TR | EC, TR] and infos["n_vertices"].tolist() == [4, 9] and writes[6][:4] == (0.0, 0.0, 0, M)
    # with the skip flag the transparent Line has no walk
    _, skipped, _ = nt.trim(scene, [(2, nt.RANGE, 0, 9, 0, U64_MAX)], True)
    assert skipped.tolist() == [(0, 0, 0, nm.NONE, EC)]
    # invalid requests write nothing
    writes, infos, _ = nt.trim(scene, [(0, 2, 0, 9, 0, 0), (0, nt.RANGE, 0, 9, 2, 1), (0, nt.PART, 0, 9, 0, 0), (0, nt.PART, 0, 9, 2, 2), (0, nt.PART, 0, 9, 0, nt.MAX_PARTS + 1)], False, ws)
    assert not writes and infos.tolist() == [(0, 0, 0, nt.INVALID, 0)] * 5
    # a NaN equals nothing, -0 equals 0
    nan, a, b = F32(np.nan), np.array([0, 0], F32), np.array([3, 4], F32)
    w = nm.Walk(nm.OPEN, [(0, a, b, 5 * U), (1, np.array([3, 4], F32), np.array([nan, 4], F32), 0), (2, np.array([nan, 4], F32), b, 0), (3, np.array([-0.0, 4], F32), a, 4 * U)])
    w.segs[2] = (2, w.segs[2][1], np.array([0.0, 4], F32), 0)
    got = nt.vertices(w, 1, w.T)                                                          # the two segments without length sit at 5 px, strictly inside
    assert [(v[2], v[3]) for v in got] == [(0, M | Ct), (0, 0), (1, 0), (2, M), (2, 0), (3, 0)]
    assert [(v[2], v[3]) for v in nt.vertices(w, 0, 5 * U)] == [(0, M), (0, 0)]           # ... and at an end of a piece they are not in it
    assert [(v[2], v[3]) for v in nt.vertices(w, 5 * U, w.T)] == [(3, M), (3, 0)]


def test_part_boundaries_in_exact_integers():
    """Over random T and m: the boundaries never decrease, tile [0, T], neighbouring pieces differ by at most one unit, and every b_i is
    np_resample's even position: count = m on a closed item, m + 1 on an open one."""
    rng = np.random.default_rng(27)
    for n in range(400):
        T = int(rng.integers(0, 1 << int(rng.integers(1, 63))))
        m = int(rng.integers(1, 300)) if n else nt.MAX_PARTS
        bs = [nt.boundary(T, m, i) for i in range(m + 1)]
        assert bs[0] == 0 and bs[-1] == T and bs == sorted(bs)
        sizes = [b - a for a, b in zip(bs, bs[1:])]
        assert max(sizes) - min(sizes) <= 1 and sum(sizes) == T
        if m <= 300:
            assert [nt.ends(nt.PART, j, m, T) for j in range(m)] == list(zip(bs, bs[1:]))
            assert nr.positions(nr.EVEN, m, T=T, kind=nm.CLOSED) == bs[:-1] and nr.positions(nr.EVEN, m + 1, T=T, kind=nm.OPEN) == bs
    assert nt.ends(nt.PART, 0, 1, U64_MAX) == (0, U64_MAX) and nt.ends(nt.RANGE, 5, U64_MAX, 7) == (5, 7) and nt.ends(nt.RANGE, 9, 12, 7) == (7, 7)
    assert not nt.valid(nt.RANGE, 2, 1) and nt.valid(nt.RANGE, 2, 2) and not nt.valid(nt.PART, 0, 0) and not nt.valid(nt.PART, 2, 2) and nt.valid(nt.PART, 1, 2)
    assert nt.valid(nt.PART, 0, nt.MAX_PARTS) and not nt.valid(nt.PART, 0, nt.MAX_PARTS + 1) and not nt.valid(2, 0, 1)


# ---- CPU: the cases are what they claim -----------------------------------------------------------------------------------------

def test_the_cases_are_what_they_claim(pm):
    """Conditions on the committed request lists, not measurements: every situation the kernel treats differently is met."""
    seen = dict.fromkeys(("cut_start", "cut_end", "cut_both", "runs", "straddle", "carry", "zero_in", "zero_out", "empty", "second_step", "tail_zero"), 0)
    for skip in (False, True):
        total = 0
        for name in tc.SCENES:
            ws = rc.expected_walks(pm, name, skip)
            scene = rc.scene_of(pm, name)
            reqs = tc.requests(pm, name, skip)
            assert {q[0] for q in reqs} == set(range(len(ws))) | {len(ws), 0xFFFFFFFF}, name
            loose = sum(nm.has_non_finite_end(w, sg[0]) for w in ws for sg in w.segs)
            assert (loose > 0) == (name == mc.NONFINITE), name
            writes, infos, pieces = nt.trim(scene, [(i, m, 0, 1 << 20, a, b) for i, m, a, b in reqs], skip, ws)
            assert bool(nt.unpromised_rows(writes, ws)) <= (name == mc.NONFINITE)
            total += int(infos["n_vertices"].sum())
            per_item = {}
            for (item, mode, s0, s1), vs in zip(reqs, pieces):
                per_item.setdefault(item, set()).add((mode, s0, s1))
                w = ws[item] if item < len(ws) else nm.Walk()
                lo, hi = nt.ends(mode, s0, s1, w.T)
                cov = nt.covered(w, lo, hi)
                if not vs:
                    seen["empty"] += 1
                    continue
                head, tail = bool(vs[0][3] & nt.CUT), bool(vs[-1][3] & nt.CUT)
                if head or tail:
                    seen["cut_both" if head and tail else "cut_start" if head else "cut_end"] += 1
                seen["runs"] += int(sum(1 for v in vs if v[3] & nt.MOVE) > 1)
                ks = [sg[0] for sg in cov]
                seen["straddle"] += int(ks[0] // 64 != ks[-1] // 64)
                seen["second_step"] += int(64 <= ks[0] and ks[-1] < 128)
                seen["carry"] += sum(1 for x, y in zip(ks, ks[1:]) if x // 64 != y // 64)
                seen["zero_in"] += sum(1 for sg in cov if sg[3] == 0)
                seen["zero_out"] += sum(1 for sg in nt.starts(w) if sg[3] == 0 and sg[4] in (lo, hi) and lo < hi)
                # a segment without length at T itself under an end beyond T: what makes a range request sum the rest of the walk
                seen["tail_zero"] += int(mode == nt.RANGE and s1 > w.T and any(sg[3] == 0 and sg[4] == w.T and sg[4] > lo for sg in nt.starts(w)))
            for item, mine in per_item.items():
                T = ws[item].T if item < len(ws) else 0
                fixed = {(nt.RANGE, 0, U64_MAX), (nt.RANGE, 0, 0), (nt.RANGE, T, T), (nt.RANGE, T, U64_MAX)} | ({(nt.RANGE, 1, T - 1)} if T >= 2 else set())
                assert mine >= fixed | {(nt.PART, j, m) for j, m in tc.part_requests()}, (name, item)
        assert 20000 < total < 100000, total                                  # some 48 000 vertices a flag
    assert all(n > 0 for n in seen.values()), seen
    assert {(j, m) for j, m in tc.part_requests()} == {(j, m) for m in (1, 2, 3, 7) for j in range(m)} | {(j, m) for m in (64, 65) for j in (0, 1, m - 2, m - 1)}
    # the named items: the step-edge pieces on the long items of `counts`, the breaks of `compound`, the repeats of `degenerate`
    ws, names = rc.expected_walks(pm, "counts"), mc.NAMES["counts"]
    for entry in ("poly-65", "poly-128", "fill-129", "poly-200", "compound-200"):
        w = ws[names[entry]]
        got = {(min(k), max(k)) for k in ([sg[0] for sg in nt.covered(w, min(s0, w.T), min(s1, w.T))] for s0, s1 in tc.range_requests(w)) if k}
        assert any(a <= 63 and b >= 64 for a, b in got), entry
        assert len(w.segs) < 128 or any(a >= 64 and b < 128 for a, b in got), entry
    ws, names = rc.expected_walks(pm, "compound"), mc.NAMES["compound"]
    for entry in ("two", "three", "empty_sub_path", "ends_before_step_edge", "ends_at_step_edge"):
        w = ws[names[entry]]
        st = nt.starts(w)
        assert tc.jumps(st), entry
        for i in tc.jumps(st):
            Q = st[i][4]
            assert {(Q - 1, Q + 1), (Q - 1, Q), (Q, Q + 1)} <= set(tc.range_requests(w)), entry
    assert not ws[names["only_separators"]].segs
    ws, names = rc.expected_walks(pm, "degenerate"), mc.NAMES["degenerate"]
    for entry in ("poly_repeat_start", "poly_repeat_middle", "poly_repeat_end", "poly_repeat_step_edge", "fill_closing_degenerate"):
        w = ws[names[entry]]
        zeros = {sg[4] for sg in nt.starts(w) if sg[3] == 0}
        assert zeros and all({(Q, Q + 1)} <= set(tc.range_requests(w)) for Q in zeros), entry
    assert [w.T for w in rc.expected_walks(pm, rc.TINY)] == [11, 12, 0, 1]
    # truncated requests: the layout list and the sweep
    laid, cap, sizes = tc.layout_requests(pm)
    _, infos, _ = nt.trim(rc.scene_of(pm, "counts"), laid, False, rc.expected_walks(pm, "counts"), out_cap=cap)
    assert (infos["flags"] & nt.TRUNCATED).sum() == 10 and len(tc.truncation_sweep(pm)) == 11


# ---- CPU: the header ----------------------------------------------------------------------------------------------------------

def test_the_header_and_the_record_sizes(pm):
    hdr = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    got = dict(re.findall(r"^#define (PM_TRIM_[A-Z_]+) (\w+)u\b", hdr, re.M))
    assert {k: int(v, 0) for k, v in got.items()} == {"PM_TRIM_RANGE": 0, "PM_TRIM_PART": 1, "PM_TRIM_MAX_PARTS": 1 << 20, "PM_TRIM_MOVE": 1, "PM_TRIM_CUT": 2,
                                                      "PM_TRIM_TRUNCATED": 1, "PM_TRIM_END_CLAMPED": 2, "PM_TRIM_INVALID": 0xFFFFFFFF}
    L = pm._lib
    assert (L.PM_TRIM_RANGE, L.PM_TRIM_PART, L.PM_TRIM_MAX_PARTS, L.PM_TRIM_INVALID) == (nt.RANGE, nt.PART, nt.MAX_PARTS, nt.INVALID)
    assert (L.PM_TRIM_MOVE, L.PM_TRIM_CUT, L.PM_TRIM_TRUNCATED, L.PM_TRIM_END_CLAMPED) == (nt.MOVE, nt.CUT, nt.TRUNCATED, nt.END_CLAMPED)
    for name, size in (("pm_trim_query", 32), ("pm_trim_vertex", 16), ("pm_trim_info", 24)):
        assert re.search(r"\} " + name + r";\s*/\* " + str(size) + r" bytes \*/", hdr), name
    assert "uint32_t item, mode, first, cap; uint64_t s0, s1; } pm_trim_query" in hdr and "float x, y; uint32_t index, flags; } pm_trim_vertex" in hdr
    assert "uint64_t length; uint32_t n_vertices, n_runs, kind, flags; } pm_trim_info" in hdr
    R = pm.renderer
    assert R.TRIM_QUERY_DTYPE == nt.TRIM_QUERY and R.TRIM_VERTEX_DTYPE == nt.TRIM_VERTEX and R.TRIM_INFO_DTYPE == nt.TRIM_INFO
    assert "int pm_trim_items(pm_ctx *c, const pm_trim_query *q, size_t n, uint32_t flags, pm_trim_vertex *out, size_t out_cap, pm_trim_info *info);" in hdr
    assert "int pm_trim_items_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream);" in hdr
    assert "#define PM_ABI_VERSION 600" in hdr
    assert len(L.SIGNATURES["pm_trim_items"][1]) == 7 and len(L.SIGNATURES["pm_trim_items_device"][1]) == 8
    kernels = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_trim.h")).read()
    assert "kTrimMaxParts = 1u << 20" in kernels and '#include "pm_resample.h"' in kernels
    for shared in ("MeasureWalkOf(", "MeasureEnds(", "MeasureFix(", "MeasureScan(", "MeasurePoint(", "MeasureLane64(", "MeasureWaveSum("):
        assert shared in kernels.split("#pragma once")[1] and "__device__ __forceinline__ " + shared.split("(")[0] not in kernels.replace("MeasureWalk MeasureWalkOf", "")
    assert "atomic" not in kernels.split("#pragma once")[1] and "__shared__" not in kernels
    host = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    assert "PM_TRIM_MAX_PARTS == pm::kTrimMaxParts" in host and "sizeof(pm_trim_query) == 32" in host and "sizeof(pm_trim_vertex) == 16" in host and "sizeof(pm_trim_info) == 24" in host
    assert host.index('#include "pm_measure.h"') < host.index('#include "pm_resample.h"') < host.index('#include "pm_trim.h"')
    assert "D27" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_trim_under_wave64_emulation(built):
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

def test_the_trim_kernel_uses_no_scratch(tmp_path):
    """pm_trim_kernel by the flags the library is built with: no private segment and VGPRs within 128; the LDS size is printed with
    the rest (pytest -s) and stands in DESIGN.md 4.  Sizes only: the assembly is searched for no instruction."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = 0
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        if "pm_trim_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        sgpr = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"pm_trim_kernel: {vgpr} VGPRs, {sgpr} SGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and lds == 0, (scratch, vgpr, lds)
    assert found == 1
    assert "-ffp-contract=off" in flags and "pm_trim.h" in mk     # (editing the header rebuilds the library)
