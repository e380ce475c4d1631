"""Resampling, pm_resample_items and pm_resample_items_device (decision D26): many points along an item, at positions the device
makes, in one walk of the item.

The bar is D25's: every record EQUAL as bytes to tests/np_measure.py's answer at the position tests/np_resample.py derives from the
decision's text, through the host call and the device call on a caller's stream, with and without PM_HIT_SKIP_TRANSPARENT.  The one
exception: the five floats of a record whose located segment has a non-finite end, in the one scene measure_cases.NONFINITE.
tests/resample_cases.py builds the request lists and says how the counts and the (start, step) variants are dealt over the items.

-m gpu: every case scene (host call packed; device call with a sentinel row between any two requests and after the last); the
device call's layout -- caller-chosen `first` values out of order, a range across out_cap, invalid requests among valid ones; the
relation on the device's own answers (pm_points_at_length_device at the s_j: the same bytes); after a styled and dashed flatten and
after reflatten_groups; every argument error, n == 0 and the Python wrappers; a scene without items; requests between frames in
flight and after a scene replacement; the CLI.
CPU: np_resample against hand-derived 3-4-5 geometry; even mode's properties in exact integers; cnt inverts s_j; the cases are what
they claim; the header; the -m gpu part against the wave64 emulation of the kernel; the compiler's listing."""
import ctypes as C
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
import resample_cases as rc  # noqa: E402
import test_measure as tm  # noqa: E402  (its helpers: buffers on the device or under the emulation, comparisons)

F32 = np.float32
UNTOUCHED = tm.UNTOUCHED
INVALID, CAPACITY = -1, -4
U = 65536
U64_MAX = (1 << 64) - 1
# case scenes, layout, relation, groups, styled and dashed, argument rules, no items, ordering, CLI
N_GPU_TESTS = len(rc.SCENES) + 8


# ---- the calls --------------------------------------------------------------------------------------------------------

def host_call(pm, r, q, skip, out_rows, out_cap=None):
    """pm_resample_items into UNTOUCHED buffers: (status, out int32 [out_rows, 8], info int32 [n + 1, 4])."""
    out = np.full((out_rows, 8), UNTOUCHED, np.int32)
    info = np.full((len(q) + 1, 4), UNTOUCHED, np.int32)
    st = pm._lib.load().pm_resample_items(r._h, q.ctypes.data, len(q), tm.skip_flag(pm, skip), out.ctypes.data, out_rows if out_cap is None else out_cap, info.ctypes.data)
    return st, out, info


def device_call(pm, r, q, skip, out_rows, out_cap, stream=None):
    """pm_resample_items_device, not waited for: (out [out_rows, 8], info [n + 1, 4], keep-alive)."""
    dq = tm.to_device(q)
    out, info = tm.blank(out_rows, 8), tm.blank(len(q) + 1, 4)
    if tm._emulated():
        pm._lib.check(pm._lib.load().pm_resample_items_device(r._h, dq.ctypes.data, len(q), tm.skip_flag(pm, skip), out.ctypes.data, out_cap, info.ctypes.data, None),
                      "pm_resample_items_device")
    else:
        r.resample_tensor(dq, out[:out_cap], info[: len(q)], stream=stream, skip_transparent=skip)
    return out, info, dq


def spread(reqs):
    """The requests laid out with one free record between any two: [(item, mode, count, first, start, step)] and the rows used."""
    out, at = [], 0
    for item, mode, count, start, step in reqs:
        out.append((item, mode, count, at, start, step))
        at += count + 1
    return out, at


def assert_buffer(got, writes, ws, exempt, what):
    """The int32 [rows, 8] buffer holds the writes and UNTOUCHED everywhere else.  Where `exempt` (only ever the non-finite scene) a
    record on a segment with a non-finite end is compared in item, status and index alone."""
    got = np.ascontiguousarray(tm.host_view(got)).copy()
    want = nr.expected_buffer(writes, len(got), UNTOUCHED)
    if exempt and writes:
        rows = np.array(sorted(writes), np.int64)
        loose = rows[tm.unpromised(ws, want[rows].view(nm.LENGTH_POINT).reshape(-1))]
        got[loose, 3:] = 0
        want[loose, 3:] = 0
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, len(bad), [(int(k), got[k].view(nm.LENGTH_POINT), want[k].view(nm.LENGTH_POINT)) for k in bad[:6]])


def assert_infos(got, want, what):
    got = np.ascontiguousarray(tm.host_view(got))
    assert (got[len(want):] == UNTOUCHED).all(), (what, "info beyond n")
    g = got[: len(want)].view(nr.RESAMPLE_INFO).reshape(-1)
    bad = tm.differing(g, want)
    assert bad.size == 0, (what, [(int(k), g[k], want[k]) for k in bad[:6]])


@pytest.fixture(scope="module")
def resample_renderer(pm):
    """Never resized: the requests need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


def check_requests(pm, r, scene, ws, reqs, skip, exempt, stream, what):
    """One request list on the resident scene: the host call, packed, and the device call, spread."""
    packed, total = nr.packed(reqs)
    want, want_info = nr.resample(scene, packed, skip, ws)
    laid, rows = spread(reqs)
    want_dev, want_dev_info = nr.resample(scene, laid, skip, ws)
    dev_out, dev_info, keep = device_call(pm, r, nr.records(laid), skip, rows + 2, rows + 1, stream)
    st, out, info = host_call(pm, r, nr.records(packed), skip, total + 2, total)
    assert st == pm._lib.PM_OK, (what, pm._lib.last_error())
    assert_buffer(out, want, ws, exempt, (what, skip, "host"))
    assert_infos(info, want_info, (what, skip, "host"))
    tm.wait(r, stream)
    assert_buffer(dev_out, want_dev, ws, exempt, (what, skip, "device"))
    assert_infos(dev_info, want_dev_info, (what, skip, "device"))
    assert tm.same(want_info, want_dev_info)
    return total


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.SCENES)
def test_case_scenes(pm, resample_renderer, name):
    """Every case scene: the request lists of resample_cases on every item and the two indices beyond the scene -- host call, and
    device call on a caller's stream with a sentinel record in every gap."""
    scene = rc.scene_of(pm, name)
    r = resample_renderer
    r.set_scene_bytes(scene)
    stream = tm.new_stream()
    for skip in (False, True):
        ws = rc.expected_walks(pm, name, skip)
        assert r.stats()["n_items"] == len(ws)
        n = check_requests(pm, r, scene, ws, rc.requests(pm, name, skip), skip, name == mc.NONFINITE, stream, name)
        assert n > 400


@pytest.mark.gpu
def test_device_call_layout(pm, resample_renderer):
    """Caller-chosen `first` values in an order other than the requests', a range that crosses out_cap, one wholly beyond it, and
    every kind of invalid request among valid ones: the invalid ones' ranges stay untouched and their neighbours are right."""
    name = "counts"
    scene = rc.scene_of(pm, name)
    ws = rc.expected_walks(pm, name)
    r = resample_renderer
    r.set_scene_bytes(scene)
    names = mc.NAMES[name]
    a, b, c = names["poly-200"], names["fill-129"], names["compound-65"]
    cap = 700
    laid = [   # (item, mode, count, first, start, step)
        (a, nr.STEP, 100, 500, 0, ws[a].T // 99),
        (b, nr.EVEN, 65, 10, 0, 0),
        (a, 2, 50, 100, 0, 7),                                  # no such mode
        (c, nr.STEP, 64, 200, 5, 1000),
        (b, nr.EVEN, 30, 300, 1, 0),                            # even with a start
        (c, nr.EVEN, 129, 340, 0, 0),
        (b, nr.EVEN, 30, 300, 0, 1),                            # even with a step
        (a, nr.STEP, nr.MAX_COUNT + 1, 0, 0, 1),                # too many
        (a, nr.STEP, 129, 650, U64_MAX - 64, 1),                # crosses the cap, and saturates on the way
        (b, nr.STEP, 3, 5, 7 * U, 0),
        (c, nr.STEP, 10, cap, 0, U),                            # begins at the cap: nothing of it is written
        (b, nr.STEP, 2, 0xFFFFFFFF, 0, U),                      # first + j passes 2^32
        (a, 0xFFFFFFFF, 1, 90, 0, 0),
    ]
    want, want_info = nr.resample(scene, laid, False, ws, out_cap=cap)
    assert [int(k) for k in want_info["kind"]].count(nr.INVALID) == 5 and max(want) == cap - 1 and 100 not in want and 300 not in want and 0 not in want
    for stream in (None, tm.new_stream()):
        out, info, keep = device_call(pm, r, nr.records(laid), False, cap + 4, cap, stream)
        tm.wait(r, stream)
        assert_buffer(out, want, ws, False, "layout")
        assert_infos(info, want_info, "layout")


@pytest.mark.gpu
def test_the_relation_on_the_devices_own_answers(pm, resample_renderer):
    """D26 is a relation between two device calls: pm_points_at_length_device at the positions s_j answers with the bytes the
    resampling wrote -- on a sample of the requests of four scenes, without any reference."""
    r = resample_renderer
    checked = 0
    for name in ("counts", "degenerate", "caps", rc.TINY):
        scene = rc.scene_of(pm, name)
        r.set_scene_bytes(scene)
        for skip in (False, True):
            ws = rc.expected_walks(pm, name, skip)
            reqs = rc.requests(pm, name, skip)[1::4]
            packed, total = nr.packed(reqs)
            out, info, keep = device_call(pm, r, nr.records(packed), skip, total + 1, total)
            pairs = []
            for item, mode, count, first, start, step in packed:
                w = ws[item] if item < len(ws) else nm.Walk()
                pairs += [(item, s) for s in nr.positions(mode, count, start, step, w.T, w.kind)]
            assert len(pairs) == total
            pts, keep2 = tm.device_points(pm, r, tm.length_queries(pairs), skip)
            r.sync()
            assert tm.same(tm.host_view(out)[:total], tm.host_view(pts)[:total]), (name, skip)
            checked += total
    assert checked > 2000


def _flattened_scene_matches(pm, r, what):
    """Records equal np_resample on the downloaded scene; for every item of positive length an even resampling has no clamped answer,
    and an open item's last sample is the end of its walk."""
    scene = r.download_scene()
    ws = nm.walks(scene)
    reqs = []
    for i, w in enumerate(ws):
        reqs += [(i, nr.EVEN, 5 + i % 3, 0, 0), (i, nr.STEP, 7, 3 * U // 2, 5 * U + 77)]
    reqs += [(len(ws), nr.EVEN, 4, 0, 0)]
    check_requests(pm, r, scene, ws, reqs, False, False, tm.new_stream(), what)
    pts, offsets, infos = r.resample(np.arange(len(ws)), 5)
    n_open = n_closed = 0
    for i, w in enumerate(ws):
        mine = pts[offsets[i]:offsets[i + 1]]
        assert int(infos[i]["length"]) == w.T and int(infos[i]["kind"]) == w.kind
        if w.T == 0:
            continue
        assert int(infos[i]["n_unclamped"]) == 5 and (mine["status"] == nm.FOUND).all(), (what, i, mine)
        k, a, b, _ = [sg for sg in w.segs if sg[3] > 0][-1]
        if w.kind == nm.OPEN:
            last = mine[-1]
            assert (int(last["index"]), float(last["t"]), last["x"], last["y"]) == (k, 1.0, b[0], b[1]), (what, i, last)
            n_open += 1
        else:
            assert float(mine[-1]["t"]) < 1.0 and int(mine[0]["index"]) == [sg for sg in w.segs if sg[3] > 0][0][0] and float(mine[0]["t"]) == 0.0
            n_closed += 1
    return ws, n_open, n_closed


@pytest.mark.gpu
def test_resampling_follows_reflatten_groups(pm):
    import path_sets
    from test_groups_gpu import rot

    ps = path_sets.random_case(321).ps
    gmap = (np.arange(len(ps.paths), dtype=np.uint32) % 3).astype(np.uint32)
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 32.0, -16.0), (2.0, 0.0, 0.0, 2.0, 5.0, 5.0), rot(0.7, 1.0, 40.0, 30.0)])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), 1.0)
        ws0, n_open, n_closed = _flattened_scene_matches(pm, r, "flattened")
        r.reflatten_groups(aff, np.array([1.0, 2.0, 1.0], F32))
        ws1, m_open, m_closed = _flattened_scene_matches(pm, r, "moved")
        assert n_open + n_closed > 5 and (n_open, n_closed) == (m_open, m_closed) and [w.T for w in ws0] != [w.T for w in ws1]


@pytest.mark.gpu
def test_resampling_styled_and_dashed_strokes(pm):
    from np_stroke import MITER, SQUARE, style_bits
    from test_stroke_gpu import shapes

    ps = shapes(lambda k: (3 if k % 4 == 0 else 2) | style_bits(SQUARE, MITER))
    ps = ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps, (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 1.0)
        ws, n_open, n_closed = _flattened_scene_matches(pm, r, "styled")
        assert n_closed >= len(ps.paths) and max(len(w.segs) for w in ws) > 64


@pytest.mark.gpu
def test_argument_rules(pm):
    """Every PM_ERR_INVALID and PM_ERR_CAPACITY case, each with nothing written; n == 0; correct calls afterwards, derived by hand;
    the Python wrappers."""
    lib = pm._lib.load()
    OK = pm._lib.PM_OK
    with pm.Renderer(0) as r:
        out = np.full((16, 8), UNTOUCHED, np.int32)
        info = np.full((4, 4), UNTOUCHED, np.int32)
        good = nr.records(nr.packed([(0, nr.STEP, 3, 0, 5 * U), (0, nr.EVEN, 4, 0, 0), (1, nr.EVEN, 2, 0, 0)])[0])
        op, ip, qp = out.ctypes.data, info.ctypes.data, good.ctypes.data
        host = lambda q, n, flags, o, cap, i: lib.pm_resample_items(r._h, q, n, flags, o, cap, i)  # noqa: E731
        dev = lambda q, n, flags, o, cap, i: lib.pm_resample_items_device(r._h, q, n, flags, o, cap, i, None)  # noqa: E731
        for call in (host, dev):                                   # no resident scene
            assert call(qp, 3, 0, op, 16, ip) == INVALID
        # a 3-4-5 Polyline of two segments (5 + 6 px) and a Circle
        r.set_scene_bytes(hs._encode(pm, 2, lambda e: (e.polyline(np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 10.0]]), 0x112233FF, 1.0), e.circle((50.0, 50.0), 5.0))))
        for call in (host, dev):
            for flags in (2, 6, 8, 0x80000001):                    # unknown flag bits, also with nothing to do
                assert call(qp, 3, flags, op, 16, ip) == INVALID and call(qp, 0, flags, op, 16, ip) == INVALID
            assert call(None, 3, 0, op, 16, ip) == INVALID         # a NULL pointer with n > 0
            assert call(qp, 3, 0, None, 16, ip) == INVALID
            assert call(qp, 3, 0, op, 16, None) == INVALID
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

        for q in (bad(1, mode=2), bad(0, mode=0xFFFFFFFF), bad(2, count=nr.MAX_COUNT + 1, first=7), bad(1, start=1), bad(2, step=1),
                  bad(1, first=4), bad(0, first=1), bad(2, first=0)):           # what the device would call invalid; a wrong first
            assert host(q.ctypes.data, 3, 0, op, 16, ip) == INVALID
        assert host(qp, 3, 0, op, 8, ip) == CAPACITY                # the total is 9
        assert host(qp, 3, 0, op, 0, ip) == CAPACITY
        big = nr.records(nr.packed([(0, nr.STEP, nr.MAX_COUNT, 0, 1), (0, nr.STEP, 1, 0, 1)])[0])
        assert host(big.ctypes.data, 2, 0, op, (1 << 20) + 1, ip) == CAPACITY   # more than 2^20 records in one call
        r.sync()
        assert (out == UNTOUCHED).all() and (info == UNTOUCHED).all()
        # correct calls afterwards, derived by hand: 0, 5 and 10 px; the open item's four even samples at 0, 11/3, 22/3 and 11 px; the Circle
        assert host(qp, 3, 0, op, 9, ip) == OK and (out[9:] == UNTOUCHED).all() and (info[3:] == UNTOUCHED).all()
        p = out[:9].view(nm.LENGTH_POINT).reshape(-1)
        T = 11 * U
        assert info[:3].view(nr.RESAMPLE_INFO).reshape(-1).tolist() == [(T, 3, nm.OPEN), (T, 4, nm.OPEN), (0, 0, nm.NONE)]
        assert p[0].tolist() == (0, nm.FOUND, 0, 0.0, 0.0, 0.0, F32(0.6), F32(0.8))
        assert p[1].tolist() == (0, nm.FOUND, 1, 0.0, 3.0, 4.0, 0.0, 1.0)
        assert p[2].tolist() == (0, nm.FOUND, 1, F32(5 / 6), 3.0, 9.0, 0.0, 1.0)
        s1, s2 = T // 3 + 1, 2 * (T // 3) + 2                        # T mod 3 == 2: the first two gaps are one unit longer
        assert T % 3 == 2 and [tuple(v) for v in p[3:7][["index", "t"]].tolist()] == [(0, 0.0), (0, F32(s1 / (5 * U))), (1, F32((s2 - 5 * U) / (6 * U))), (1, 1.0)]
        assert p[6].tolist() == (0, nm.FOUND, 1, 1.0, 3.0, 10.0, 0.0, 1.0)
        assert p[7:]["item"].tolist() == [nm.HIT_NONE] * 2 and not out[7:9, 1:].any()
        # the Python wrappers
        pts, offsets, infos = r.resample([0, 1, 0], [4, 2, 0])
        assert pts.dtype == pm.renderer.LENGTH_POINT_DTYPE and infos.dtype == pm.renderer.RESAMPLE_INFO_DTYPE and offsets.tolist() == [0, 4, 6, 6]
        assert tm.same(pts[:4], p[3:7]) and infos["n_unclamped"].tolist() == [4, 0, 0]
        pts, offsets, infos = r.resample_step([0, 1, 7], 2.5, 1.0)       # as many as fit: 1, 3.5, 6, 8.5 and 11 px; none on the Circle, none beyond the scene
        assert offsets.tolist() == [0, 5, 5, 5] and infos["n_unclamped"].tolist() == [5, 0, 0] and pts["y"][:5].tolist() == [F32(0.8), F32(2.8), 5.0, 7.5, 10.0]
        assert tm.same(pts[:5], r.points_at_length([0] * 5, [1.0, 3.5, 6.0, 8.5, 11.0]))
        pts, offsets, infos = r.resample_step([0], 4.0, 0.0, counts=5)    # given counts: nothing is read back, the rest is clamped
        assert infos["n_unclamped"].tolist() == [3] and pts["status"].tolist() == [1, 1, 1, 3, 3]
        assert r.resample_step([0, 0], [20.0, 1.0], [12.0, 0.0])[1].tolist() == [0, 0, 12]
        assert len(r.resample([], [])[0]) == 0 and r.resample([], [])[1].tolist() == [0]
        assert pm.renderer.resample_positions(pm._lib.PM_RESAMPLE_EVEN, 4, T, nm.OPEN) == [0, s1, s2, T]
        for wrong in (lambda: r.resample([0, 0], [1, 2, 3]), lambda: r.resample([[0]], 3), lambda: r.resample([0], -1), lambda: r.resample([0], nr.MAX_COUNT + 1),
                      lambda: r.resample([0, 0], nr.MAX_COUNT), lambda: r.resample_step([0], 0.0), lambda: r.resample_step([0, 0], [1.0])):
            with pytest.raises(ValueError):
                wrong()
        assert lib.pm_abi_version() == 600
        if not tm._emulated():
            import torch

            q8, o8, i4 = tm.to_device(good), torch.zeros((9, 8), dtype=torch.int32, device="cuda"), torch.zeros((3, 4), dtype=torch.int32, device="cuda")
            for wrong in (lambda: r.resample_tensor(q8.cpu(), o8, i4), lambda: r.resample_tensor(q8[:, :4].contiguous(), o8, i4),
                          lambda: r.resample_tensor(q8, o8[:, :4].contiguous(), i4), lambda: r.resample_tensor(q8, o8, i4[:2]), lambda: r.resample_tensor(q8, o8.float(), i4)):
                with pytest.raises(TypeError):
                    wrong()
            r.resample_tensor(q8, o8, i4)
            r.sync()
            assert tm.same(o8.cpu().numpy(), out[:9]) and tm.same(i4.cpu().numpy(), info[:3])


@pytest.mark.gpu
def test_a_scene_without_items(pm, resample_renderer):
    """n_items == 0: every request answers "none" count times, with the info {0, 0, PM_MEASURE_NONE}."""
    r = resample_renderer
    r.set_scene_bytes(hs._encode(pm, 0, lambda e: None))
    assert r.stats()["n_items"] == 0
    packed, total = nr.packed([(0, nr.EVEN, 3, 0, 0), (0xFFFFFFFF, nr.STEP, 66, 5, 9), (5, nr.STEP, 0, 0, 0)])
    st, out, info = host_call(pm, r, nr.records(packed), False, total + 1, total)
    dev_out, dev_info, keep = device_call(pm, r, nr.records(packed), True, total + 1, total)
    r.sync()
    for o, i in ((out, info), (tm.host_view(dev_out), tm.host_view(dev_info))):
        assert (o[:total, 0].view(np.uint32) == nm.HIT_NONE).all() and not o[:total, 1:].any() and (o[total:] == UNTOUCHED).all()
        assert i[:3].view(nr.RESAMPLE_INFO).reshape(-1).tolist() == [(0, 0, nm.NONE)] * 3 and (i[3:] == UNTOUCHED).all()
    assert st == pm._lib.PM_OK and r.resample([0, 1], 2)[2]["kind"].tolist() == [0, 0]


@pytest.mark.gpu
def test_requests_between_frames_and_after_a_replacement(pm, pmo):
    """Frames rendered before and after resampling have the bytes they have without it; a device call on a caller's stream followed
    at once by a re-flatten answers for the scene resident at the call; a replacement between two requests gives each its own."""
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        ws = nm.walks(scene)
        longest = max(range(len(ws)), key=lambda i: ws[i].T)
        reqs = [(i, nr.EVEN, 6, 0, 0) for i in range(0, len(ws), 9)] + [(longest, nr.STEP, 300, U // 2, ws[longest].T // 290)]
        packed, total = nr.packed(reqs)
        q = nr.records(packed)
        want, want_info = nr.resample(scene, packed, False, ws)
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
        assert int(want_info["n_unclamped"][-1]) in (290, 291) and len(ws[longest].segs) > 128
        r.render()
        dev_out, dev_info, keep = device_call(pm, r, q, False, total + 1, total, s)     # frame in flight, request, replacement, request
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        after_out, after_info, keep2 = device_call(pm, r, q, False, total + 1, total, s)
        tm.wait(r, s)
        assert_buffer(dev_out, want, ws, False, "before the replacement")
        assert_infos(dev_info, want_info, "before the replacement")
        scene2 = r.download_scene()
        ws2 = nm.walks(scene2)
        want2, want_info2 = nr.resample(scene2, packed, False, ws2)
        assert_buffer(after_out, want2, ws2, False, "after the replacement")
        assert_infos(after_info, want_info2, "after the replacement")
        assert not tm.same(want_info, want_info2)


@pytest.mark.gpu
def test_cli_resample_and_resample_step(pm, tmp_path, capsys):
    """--resample ITEM,N and --resample-step ITEM,STEP[,START]: a line with the item's length and how many points are not clamped,
    then one line per point as --point-at prints it."""
    from piet_metal_amd import cli

    wl = pm.workloads.tiger(480, 270)
    args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--resample", "40,5", "--resample", "100000,2", "--resample-step", "5,3.5",
            "--resample-step", "40,10,2.25"]
    assert cli.main(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    R = pm.renderer
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        of_item = r.item_paths()
        lens = r.item_lengths()
        want = []
        pts, offsets, infos = r.resample([40, 100000], [5, 2])
        for k, (i, n) in enumerate(((40, 5), (100000, 2))):
            want.append(f"resample item {i} {n} even: length {int(infos[k]['length']) / 65536:g} points {n} unclamped {int(infos[k]['n_unclamped'])}")
            ss = R.resample_positions(1, n, int(infos[k]["length"]), int(infos[k]["kind"]))
            want += [cli.point_line(i, s / 65536, p, of_item) for s, p in zip(ss, pts[offsets[k]:offsets[k + 1]])]
        for i, step, start in ((5, 3.5, 0.0), (40, 10.0, 2.25)):
            T = int(lens[i]["length"])
            n = (T - R.length_units(start)) // R.length_units(step) + 1
            ss = [R.length_units(start) + j * R.length_units(step) for j in range(n)]
            got = r.points_at_units([i] * n, ss)
            want.append(f"resample item {i} every {step:g} from {start:g}: length {T / 65536:g} points {n} unclamped {n}")
            want += [cli.point_line(i, s / 65536, p, of_item) for s, p in zip(ss, got)]
    assert [ln for ln in lines if ln.startswith(("resample ", "item "))] == want
    assert want[0].endswith("points 5 unclamped 5") and want[6].endswith("length 0 points 2 unclamped 0") and want[7].endswith("none") and len(want) > 20
    for wrong in (["--resample", "40"], ["--resample", "40,-1"], ["--resample-step", "40,0"], ["--resample-step", "40,1,2,3"], ["--resample-step", "40,1,-2"]):
        with pytest.raises(SystemExit):
            cli.main(args[:6] + wrong)
    capsys.readouterr()


# ---- CPU: np_resample itself -----------------------------------------------------------------------------------------------------

def test_np_resample_against_hand_derived_geometry(pm):
    """tests/test_measure.py's hand scene: the Polyline 5 + 6 + 10 px, the Fill 6 + 8 + 10 px, the Line of 50 px, a Circle.  Even
    samples fall where arithmetic says, open and closed; a step request clamps past the end."""
    scene = tm.hand_scene(pm)
    ws = nm.walks(scene)
    F, Cl = nm.FOUND, nm.CLAMPED
    packed, total = nr.packed([(0, nr.EVEN, 4, 0, 0), (1, nr.EVEN, 4, 0, 0), (2, nr.EVEN, 3, 0, 0), (3, nr.EVEN, 2, 0, 0), (0, nr.STEP, 4, 2 * U, 8 * U), (1, nr.EVEN, 1, 0, 0),
                               (0, nr.EVEN, 1, 0, 0), (2, nr.STEP, 2, 0, 0)])
    writes, infos = nr.resample(scene, packed, False, ws)
    got = np.array([writes[k] for k in range(total)], nm.LENGTH_POINT)
    want = [
        # the open Polyline of 21 px, m = 3: 0, 7, 14 and 21 px -- the start, 2 px along the vertical segment, 3 px along the last, the end
        (0, F, 0, 0.0, 0.0, 0.0, F32(0.6), F32(0.8)), (0, F, 1, F32(2 / 6), 3.0, 6.0, 0.0, 1.0), (0, F, 2, F32(0.3), F32(5.4), F32(11.8), F32(0.8), F32(0.6)),
        (0, F, 2, 1.0, 11.0, 16.0, F32(0.8), F32(0.6)),
        # the closed Fill of 24 px, m = 4: 0, 6, 12 and 18 px -- two vertices, 6 px up the side, 4 px down the closing segment; not the start again
        (1, F, 0, 0.0, 0.0, 0.0, 1.0, 0.0), (1, F, 1, 0.0, 6.0, 0.0, 0.0, 1.0), (1, F, 1, 0.75, 6.0, 6.0, 0.0, 1.0), (1, F, 2, 0.4, F32(3.6), F32(4.8), F32(-0.6), F32(-0.8)),
        # the Line of 50 px, m = 2
        (2, F, 0, 0.0, 10.0, 10.0, F32(0.6), F32(0.8)), (2, F, 0, 0.5, 25.0, 30.0, F32(0.6), F32(0.8)), (2, F, 0, 1.0, 40.0, 50.0, F32(0.6), F32(0.8)),
        # the Circle
        (nm.HIT_NONE, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0), (nm.HIT_NONE, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0),
        # every 8 px from 2 px on: 2, 10, 18 px and, clamped, the end
        (0, F, 0, 0.4, F32(1.2), F32(1.6), F32(0.6), F32(0.8)), (0, F, 1, F32(5 / 6), 3.0, 9.0, 0.0, 1.0), (0, F, 2, 0.7, F32(8.6), F32(14.2), F32(0.8), F32(0.6)),
        (0, F | Cl, 2, 1.0, 11.0, 16.0, F32(0.8), F32(0.6)),
        # one even sample: the start, of a closed item (m = 1) and of an open one (m = 0)
        (1, F, 0, 0.0, 0.0, 0.0, 1.0, 0.0), (0, F, 0, 0.0, 0.0, 0.0, F32(0.6), F32(0.8)),
        # step 0: the same point twice
        (2, F, 0, 0.0, 10.0, 10.0, F32(0.6), F32(0.8)), (2, F, 0, 0.0, 10.0, 10.0, F32(0.6), F32(0.8)),
    ]
    want = np.array(want, nm.LENGTH_POINT)
    assert tm.same(got, want), [(int(k), got[k], want[k]) for k in tm.differing(got, want)]
    assert infos.tolist() == [(21 * U, 4, nm.OPEN), (24 * U, 4, nm.CLOSED), (50 * U, 3, nm.OPEN), (0, 0, nm.NONE), (21 * U, 3, nm.OPEN), (24 * U, 1, nm.CLOSED),
                              (21 * U, 1, nm.OPEN), (50 * U, 2, nm.OPEN)]
    # with the skip flag the transparent Line has no walk
    _, skipped = nr.resample(scene, [(2, nr.EVEN, 3, 0, 0, 0)], True)
    assert skipped.tolist() == [(0, 0, nm.NONE)]
    # invalid requests write nothing
    writes, infos = nr.resample(scene, [(0, 2, 3, 0, 0, 0), (0, nr.EVEN, 3, 0, 1, 0), (0, nr.EVEN, 3, 0, 0, 1), (0, nr.STEP, nr.MAX_COUNT + 1, 0, 0, 0)], False, ws)
    assert not writes and infos.tolist() == [(0, 0, nr.INVALID)] * 4


def test_even_positions_in_exact_integers():
    """Over random T and count: s_0 = 0, the positions never decrease, s_m = T exactly, neighbouring gaps differ by at most one unit."""
    rng = np.random.default_rng(26)
    checked = 0
    for _ in range(400):
        T = int(rng.integers(0, 1 << int(rng.integers(1, 63))))
        count = int(rng.integers(0, 300))
        for kind in (nm.OPEN, nm.CLOSED):
            m = nr.even_m(kind, count)
            ss = nr.positions(nr.EVEN, count, T=T, kind=kind)
            assert len(ss) == count and (count == 0 or ss[0] == 0)
            if m == 0:
                assert not any(ss)
                continue
            full = ss + [nr.position(nr.EVEN, count, T=T, m=m)] if kind == nm.CLOSED else ss      # sample `count` of a closed item: the start again
            assert full[m] == T and max(full) == T
            gaps = [b - a for a, b in zip(full, full[1:])]
            assert min(gaps) >= 0 and max(gaps) - min(gaps) <= 1 and sorted(gaps, reverse=True) == gaps
            checked += 1
    assert checked > 600
    assert nr.positions(nr.EVEN, 5, T=7, kind=nm.NONE) == [0] * 5 and nr.positions(nr.EVEN, 1, T=7, kind=nm.OPEN) == [0]
    assert nr.positions(nr.EVEN, 4, T=U64_MAX, kind=nm.OPEN)[-1] == U64_MAX


def test_cnt_inverts_the_positions():
    """cnt(x) is the number of j < count with s_j < x -- in both modes, with step 0, with saturation, and where m > T."""
    rng = np.random.default_rng(27)
    cases = [(nr.STEP, c, st, sp, 0, 0) for c in (0, 1, 5, 64) for st in (0, 7, U64_MAX - 9, U64_MAX) for sp in (0, 1, 3, 1 << 62, U64_MAX)]
    for _ in range(200):
        T = int(rng.integers(0, 1 << int(rng.integers(1, 40))))
        count = int(rng.integers(0, 130))
        cases.append((nr.EVEN, count, 0, 0, T, nr.even_m(int(rng.integers(0, 3)), count)))
    cases += [(nr.EVEN, 64, 0, 0, 12, 64), (nr.EVEN, 65, 0, 0, 11, 64), (nr.EVEN, 5, 0, 0, 0, 4)]
    for mode, count, start, step, T, m in cases:
        ss = [nr.position(mode, j, start, step, T, m) for j in range(count)]
        assert ss == sorted(ss)
        xs = {0, 1, T, T + 1, U64_MAX, start, min(start + 1, U64_MAX)} | set(ss) | {min(s + 1, U64_MAX) for s in ss} | {max(s - 1, 0) for s in ss}
        for x in xs:
            assert nr.cnt(x, mode, count, start, step, T, m) == sum(1 for s in ss if s < x), (mode, count, start, step, T, m, x)
    assert nr.position(nr.STEP, 3, U64_MAX - 5, 2) == U64_MAX and nr.position(nr.STEP, 2, U64_MAX - 5, 2) == U64_MAX - 1


# ---- CPU: the cases are what they claim -----------------------------------------------------------------------------------------

def test_the_cases_are_what_they_claim(pm):
    total = 0
    circles = 0
    for name in rc.SCENES:
        ws = rc.expected_walks(pm, name)
        scene = rc.scene_of(pm, name)
        reqs = rc.requests(pm, name)
        total += rc.n_samples(reqs) + rc.n_samples(rc.requests(pm, name, True))
        items = {q[0] for q in reqs}
        assert items == set(range(len(ws))) | {len(ws), 0xFFFFFFFF}, name
        circles += sum(struct_tag(scene, at) == nm.np_hit.CIRCLE for at, _ in nm.np_hit.flat_items(bytes(scene)))
        # the one exception: no scene but NONFINITE has a segment with a non-finite end
        loose = sum(nm.has_non_finite_end(w, sg[0]) for w in ws for sg in w.segs)
        assert (loose > 0) == (name == mc.NONFINITE), name
        by_item = {}
        for q in reqs:
            by_item.setdefault(q[0], []).append(q)
        for i, mine in by_item.items():
            w = ws[i] if i < len(ws) else nm.Walk()
            step_reqs = [q for q in mine if q[1] == nr.STEP]
            assert {(q[3], q[4]) for q in step_reqs} >= set(rc.variants(w)), (name, i)            # every variant on every item
            assert {q[2] for q in mine if q[1] == nr.EVEN} >= set(rc.EVEN_SMALL), (name, i)
            assert ({q[2] for q in mine if q[1] == nr.EVEN} & set(rc.EVEN_BIG)) or ({q[2] for q in step_reqs} & set(rc.BIG)), (name, i)
        if name in rc.FULL_CROSS:
            full = by_item[rc.full_cross_item(ws)]
            assert {(q[2], q[3], q[4]) for q in full if q[1] == nr.STEP} >= {(c, st, sp) for st, sp in rc.variants(ws[rc.full_cross_item(ws)]) for c in rc.STEP_COUNTS}
            assert [q[2] for q in full if q[1] == nr.EVEN] == list(rc.EVEN_COUNTS)
    assert circles >= 3                                                                             # a Circle is among the items
    assert 20000 < total < 100000, total                                                           # the case scenes' requests, both flags: some 43 000 a flag
    # the large walk scenes meet every variant with a large count, every large count, and every large even count
    met, evens = set(), set()
    for q in rc.requests(pm, "walk-65"):
        w = rc.expected_walks(pm, "walk-65")[q[0]] if q[0] < 65 else nm.Walk()
        if q[1] == nr.STEP and q[2] in rc.BIG:
            met.add((rc.variants(w).index((q[3], q[4])), q[2]))
        if q[1] == nr.EVEN and q[2] in rc.EVEN_BIG:
            evens.add(q[2])
    assert {v for v, _ in met} == set(range(12)) and {c for _, c in met} == set(rc.BIG) and evens == set(rc.EVEN_BIG)
    # even requests with T mod m != 0, and with more gaps than units (m > T > 0)
    uneven = tight = 0
    for name in rc.SCENES:
        ws = rc.expected_walks(pm, name)
        for q in rc.requests(pm, name):
            if q[1] == nr.EVEN and q[0] < len(ws):
                w, m = ws[q[0]], nr.even_m(ws[q[0]].kind, q[2])
                uneven += int(m > 0 and w.T % m != 0)
                tight += int(m > w.T > 0)
    assert uneven > 100 and tight >= 3
    tiny = rc.expected_walks(pm, rc.TINY)
    assert [w.T for w in tiny] == [11, 12, 0, 1] and [w.kind for w in tiny] == [nm.OPEN, nm.CLOSED, nm.NONE, nm.OPEN]
    # the wide steps pass 2^64 in the high half of the product, in the sum of its halves, and only with the start added
    ways = set()
    for start, step in rc.WIDE_STEPS:
        for j in range(5):
            ph, pl = j * (step >> 32), j * (step & 0xFFFFFFFF)
            ways.add("high" if ph >> 32 else ("sum" if (ph << 32) + pl >> 64 else ("start" if start + j * step >> 64 else "none")))
    assert ways == {"high", "sum", "start", "none"} and all(q in rc.requests(pm, name) for name in rc.SCENES for q in [(0, nr.STEP, 5) + w for w in rc.WIDE_STEPS])
    # caps: 70 consecutive segments own one sample each
    names, ws = mc.NAMES["caps"], rc.expected_walks(pm, "caps")
    for q in rc.special_requests("caps", names, ws):
        w = ws[q[0]]
        owners = [s >> 32 for s in nr.positions(q[1], q[2], q[3], q[4], w.T, w.kind)]
        assert [sg[3] for sg in w.segs] == [1 << 32] * 70 and owners == list(range(70))
    # counts: requests whose samples leave whole steps of 64 entries without one, and one sample in each step
    names, ws = mc.NAMES["counts"], rc.expected_walks(pm, "counts")
    seen = set()
    for q in rc.special_requests("counts", names, ws):
        w = ws[q[0]]
        Q, starts = 0, []
        for k, _, _, qk in w.segs:
            starts.append((Q, k))
            Q += qk
        steps = sorted({max(k for Q0, k in starts if Q0 <= s) // 64 for s in nr.positions(q[1], q[2], q[3], q[4], w.T, w.kind) if s < w.T})
        seen.add(tuple(steps))
    assert (0, 3) in seen and (0, 1, 2, 3) in seen
    # one segment owns every sample of the step-1 variant on the full-cross item of `counts`
    w = ws[rc.full_cross_item(ws)]
    start, step = rc.variants(w)[1]
    owners = {k for k, s in enumerate(w.segs) for p in range(start, start + 129) if sum(x[3] for x in w.segs[:k]) <= p < sum(x[3] for x in w.segs[: k + 1])}
    assert step == 1 and len(owners) == 1 and len(w.segs) == 200
    # ... and the first-q variant puts a sample exactly on a Q_k
    start, step = rc.variants(w)[2]
    assert (start, step) == (0, w.segs[0][3]) and w.segs[0][3] > 0


def struct_tag(scene, at):
    import struct

    return struct.unpack_from("<I", bytes(scene[at:at + 4]), 0)[0] & 0xFFFF


# ---- CPU: the header ----------------------------------------------------------------------------------------------------------

def test_the_header_and_the_record_sizes(pm):
    hdr = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    got = dict(re.findall(r"^#define (PM_RESAMPLE_[A-Z_]+) (\w+)u\b", hdr, re.M))
    assert {k: int(v, 0) for k, v in got.items()} == {"PM_RESAMPLE_STEP": 0, "PM_RESAMPLE_EVEN": 1, "PM_RESAMPLE_MAX_COUNT": 1 << 20, "PM_RESAMPLE_INVALID": 0xFFFFFFFF}
    L = pm._lib
    assert (L.PM_RESAMPLE_STEP, L.PM_RESAMPLE_EVEN, L.PM_RESAMPLE_MAX_COUNT, L.PM_RESAMPLE_INVALID) == (nr.STEP, nr.EVEN, nr.MAX_COUNT, nr.INVALID)
    for name, size in (("pm_resample_query", 32), ("pm_resample_info", 16)):
        assert re.search(r"\} " + name + r";\s*/\* " + str(size) + r" bytes \*/", hdr), name
    assert "uint32_t item, mode, count, first; uint64_t start, step; } pm_resample_query" in hdr and "uint64_t length; uint32_t n_unclamped, kind; } pm_resample_info" in hdr
    R = pm.renderer
    assert R.RESAMPLE_QUERY_DTYPE == nr.RESAMPLE_QUERY and R.RESAMPLE_INFO_DTYPE == nr.RESAMPLE_INFO
    assert "int pm_resample_items(pm_ctx *c, const pm_resample_query *q, size_t n, uint32_t flags, pm_length_point *out, size_t out_cap, pm_resample_info *info);" in hdr
    assert "int pm_resample_items_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream);" in hdr
    assert len(L.SIGNATURES["pm_resample_items"][1]) == 7 and len(L.SIGNATURES["pm_resample_items_device"][1]) == 8
    kernels = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_resample.h")).read()
    assert "kResampleMaxCount = 1u << 20" in kernels and '#include "pm_measure.h"' in kernels
    for shared in ("MeasureWalkOf(", "MeasureEnds(", "MeasureFix(", "MeasureScan(", "MeasurePoint(", "MeasureDir(", "MeasureStore32("):
        assert shared in kernels.split("#pragma once")[1] and "__device__ __forceinline__ " + shared.split("(")[0] not in kernels.replace("MeasureWalk MeasureWalkOf", "")
    host = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    assert "PM_RESAMPLE_MAX_COUNT == pm::kResampleMaxCount" in host and "sizeof(pm_resample_query) == 32" in host
    assert host.index('#include "pm_measure.h"') < host.index('#include "pm_resample.h"')
    assert "D26" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_resample_under_wave64_emulation(built):
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

def test_the_resample_kernel_uses_no_scratch(tmp_path):
    """pm_resample_kernel by the flags the library is built with: no private segment and VGPRs within 128; the LDS size is printed
    with the rest (pytest -s) and stands in DESIGN.md 4.  Sizes only: the assembly is searched for no instruction."""
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
        if "pm_resample_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        sgpr = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"pm_resample_kernel: {vgpr} VGPRs, {sgpr} SGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128, (scratch, vgpr, lds)
    assert found == 1
    assert "-ffp-contract=off" in flags and "pm_resample.h" in mk     # (editing the header rebuilds the library)
