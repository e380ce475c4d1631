"""Item crossings, pm_item_crossings and pm_item_crossings_device (decision D29): every point where two items' edges cross.

No tolerance anywhere: records, untouched rows (the sentinel word test_measure.UNTOUCHED) and infos EQUAL as bytes to
tests/np_crossings.py's, which is written from the decision's text over np_measure's segment lists and evaluates every pair in two
loop orders, through the host call and the device call on a caller's stream, with and without PM_HIT_SKIP_TRANSPARENT.
tests/crossings_cases.py builds the scenes and the request lists.

-m gpu: every case scene (host call packed; device call with a sentinel row between any two requests and after the last) and a scene
without items; truncation and layout; more requests than the grid has waves; the relations on the device's own answers (swap, D23,
positions); the scissors workflow; after a styled and dashed flatten and after reflatten_groups; every argument error, n == 0,
hand-derived answers and the Python wrappers; requests between frames in flight and after a scene replacement; the CLI.
CPU: the rule against exact rational arithmetic; np_crossings against hand-derived coordinates; the cases are what they claim; the
header; the -m gpu part against the wave64 emulation of the kernel; the compiler's listing."""
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crossings_cases as cc  # noqa: E402
import hit_structure as hs  # noqa: E402
import np_cross  # noqa: E402  (the D23 relation's near lists; np_crossings itself shares no code with it)
import np_crossings as nx  # noqa: E402
import np_measure as nm  # noqa: E402
import np_snap  # noqa: E402
import test_measure as tm  # noqa: E402  (its helpers: buffers on the device or under the emulation, comparisons)

F32 = np.float32
UNTOUCHED = tm.UNTOUCHED
INVALID, CAPACITY = -1, -4
NONE = 0xFFFFFFFF
# case scenes, no items, truncation and layout, the grid, relations, workflow, groups, styled and dashed, argument rules, ordering, CLI
N_GPU_TESTS = len(cc.SCENES) + 10

_models = {}


def model(pm, name, skip=False):
    """(scene, walks, index ranges) of a case scene, made once."""
    if (name, skip) not in _models:
        scene = cc.scene_of(pm, name)
        _models[(name, skip)] = (scene, nm.walks(scene, skip), nx.index_ranges(scene, skip))
    return _models[(name, skip)]


# ---- the calls --------------------------------------------------------------------------------------------------------

def host_call(pm, r, q, skip, out_rows, out_cap=None):
    """pm_item_crossings into UNTOUCHED buffers: (status, out int32 [out_rows, 12], info int32 [n + 1, 4])."""
    out = np.full((out_rows, 12), UNTOUCHED, np.int32)
    info = np.full((len(q) + 1, 4), UNTOUCHED, np.int32)
    st = pm._lib.load().pm_item_crossings(r._h, q.ctypes.data, len(q), tm.skip_flag(pm, skip), out.ctypes.data, out_rows if out_cap is None else out_cap, info.ctypes.data)
    return st, out, info


def device_call(pm, r, q, skip, out_rows, out_cap, stream=None):
    """pm_item_crossings_device, not waited for: (out [out_rows, 12], info [n + 1, 4], keep-alive)."""
    dq = tm.to_device(q)
    out, info = tm.blank(out_rows, 12), tm.blank(len(q) + 1, 4)
    if tm._emulated():
        pm._lib.check(pm._lib.load().pm_item_crossings_device(r._h, dq.ctypes.data, len(q), tm.skip_flag(pm, skip), out.ctypes.data, out_cap, info.ctypes.data, None),
                      "pm_item_crossings_device")
    else:
        r.crossings_tensor(dq, out[:out_cap], info[: len(q)], stream=stream, skip_transparent=skip)
    return out, info, dq


def spread(pairs, caps):
    """The requests laid out with one free row between any two: [(item_a, item_b, first, cap)] and the rows used."""
    out, at = [], 0
    for (a, b), cap in zip(pairs, caps):
        out.append((a, b, at, cap))
        at += cap + 1
    return out, at


def assert_buffer(got, writes, what):
    """The int32 [rows, 12] buffer holds the writes and UNTOUCHED everywhere else."""
    got = np.ascontiguousarray(tm.host_view(got))
    want = nx.expected_buffer(writes, len(got), UNTOUCHED)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, len(bad), [(int(k), got[k].view(nx.CROSSING), want[k].view(nx.CROSSING)) for k in bad[:6]])


def assert_infos(got, want, what):
    got = np.ascontiguousarray(tm.host_view(got))
    assert (got[len(want):] == UNTOUCHED).all(), (what, "info beyond n")
    g = got[: len(want)].view(nx.CROSSINGS_INFO).reshape(-1)
    bad = tm.differing(g, want)
    assert bad.size == 0, (what, [(int(k), g[k], want[k]) for k in bad[:6]])


@pytest.fixture(scope="module")
def crossings_renderer(pm):
    """Never resized: the requests need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


def check_requests(pm, r, scene, ws, Ks, pairs, skip, stream, what):
    """One list of (item_a, item_b) on the resident scene, every request given exactly the room it needs: the host call, packed, and
    the device call, spread; then the count pass.  Returns the infos."""
    _, count_info, _ = nx.crossings(scene, [(a, b, 0, 0) for a, b in pairs], skip, ws, Ks=Ks)
    caps = [int(c) for c in count_info["n_crossings"]]
    packed, total = nx.packed(pairs, caps)
    want, want_info, _ = nx.crossings(scene, packed, skip, ws, Ks=Ks)
    laid, rows = spread(pairs, caps)
    want_dev, want_dev_info, _ = nx.crossings(scene, laid, skip, ws, Ks=Ks)
    dev_out, dev_info, keep = device_call(pm, r, nx.records(laid), skip, rows + 2, rows + 1, stream)
    st, out, info = host_call(pm, r, nx.records(packed), skip, total + 2, total)
    assert st == pm._lib.PM_OK, (what, pm._lib.last_error())
    assert_buffer(out, want, (what, skip, "host"))
    assert_infos(info, want_info, (what, skip, "host"))
    tm.wait(r, stream)
    assert_buffer(dev_out, want_dev, (what, skip, "device"))
    assert_infos(dev_info, want_dev_info, (what, skip, "device"))
    assert tm.same(want_info, want_dev_info) and not (want_info["flags"] & nx.TRUNCATED).any()
    # the count pass: the same infos but for the truncated bit, and nothing written
    st, out, info = host_call(pm, r, nx.records([(a, b, 0, 0) for a, b in pairs]), skip, 2, 0)
    assert st == pm._lib.PM_OK and (out == UNTOUCHED).all()
    assert_infos(info, count_info, (what, skip, "count"))
    assert ((count_info["flags"] & nx.TRUNCATED) != 0).tolist() == [c > 0 for c in caps]
    return want_info


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.SCENES)
def test_case_scenes(pm, crossings_renderer, name):
    """Every case scene's request list -- host call, and device call on a caller's stream with a sentinel row in every gap."""
    r = crossings_renderer
    r.set_scene_bytes(cc.scene_of(pm, name))
    stream = tm.new_stream()
    N = cc.names(pm, name)
    for skip in ((False, True) if name == "hand" else (False,)):
        scene, ws, Ks = model(pm, name, skip)
        assert r.stats()["n_items"] == len(ws)
        pairs = cc.pairs(pm, name)
        infos = check_requests(pm, r, scene, ws, Ks, pairs, skip, stream, name)
        at = {p: k for k, p in enumerate(pairs)}
        if name == "hand":
            n = {p: int(infos[k]["n_crossings"]) for p, k in at.items()}
            assert n[(N["clear"], N["opaque"])] == (0 if skip else 1) and int(infos[at[(N["clear"], N["opaque"])]]["n_a"]) == (0 if skip else 1)
            assert n[(N["x_up"], N["x_down"])] == 1 and n[(N["through"], N["square"])] == 2 and n[(N["t_bar"], N["t_stem"])] == 1
            assert sum(n.values()) == (21 if skip else 23)
        elif name == "lanes":
            assert [int(infos[at[(N["long_line"], N[f"zig-{z}"])]]["n_crossings"]) for z in cc.ZIG] == list(cc.ZIG)
            assert int(infos[at[(N["star"], N["star"])]]["n_crossings"]) == cc.STAR
        else:
            flags = {p: int(infos[k]["flags"]) for p, k in at.items()}
            assert flags[(N["big_a"], N["big_b"])] == nx.TOO_MANY and flags[(N["most_a"], N["most_far"])] == 0 and flags[(N["big_a"], N["most_a"])] == nx.TOO_MANY
            assert int(infos[at[(N["cut"], N["most_a"])]]["n_crossings"]) == 32


@pytest.mark.gpu
def test_a_scene_without_items(pm, crossings_renderer):
    """n_items == 0: every request names two items without a walk."""
    r = crossings_renderer
    r.set_scene_bytes(hs._encode(pm, 0, lambda e: None))
    assert r.stats()["n_items"] == 0
    q = nx.records([(0, 0, 0, 3), (0xFFFFFFFF, 1, 3, 2), (5, 0, 5, 0)])
    st, out, info = host_call(pm, r, q, False, 6, 5)
    dev_out, dev_info, keep = device_call(pm, r, q, True, 6, 5)
    r.sync()
    for o, i in ((out, info), (tm.host_view(dev_out), tm.host_view(dev_info))):
        assert (o == UNTOUCHED).all() and (i[3:] == UNTOUCHED).all()
        assert i[:3].view(nx.CROSSINGS_INFO).reshape(-1).tolist() == [(0, 0, 0, 0)] * 3
    assert st == pm._lib.PM_OK and len(r.crossings([0, 1], [1, 1])[0]) == 0


@pytest.mark.gpu
def test_truncation_and_layout(pm, crossings_renderer):
    """Caps below, at and above the answer's size, 0, and around what a round of the lanes holds; firsts the caller chose, out of
    order, with gaps; first + p across out_cap, a request at out_cap, first = 0xFFFFFFFF."""
    scene, ws, Ks = model(pm, "lanes")
    r = crossings_renderer
    r.set_scene_bytes(scene)
    laid, cap = cc.layout_requests(pm)
    want, want_info, _ = nx.crossings(scene, laid, False, ws, out_cap=cap, Ks=Ks)
    assert max(want) == cap - 1 and min(want) == 3
    assert [int(f) & nx.TRUNCATED for f in want_info["flags"]] == [1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    for stream in (None, tm.new_stream()):
        out, info, keep = device_call(pm, r, nx.records(laid), False, cap + 4, cap, stream)
        tm.wait(r, stream)
        assert_buffer(out, want, "layout")
        assert_infos(info, want_info, "layout")


@pytest.mark.gpu
def test_more_requests_than_the_grid_has_waves(pm, crossings_renderer):
    """One request either side of what the grid rule holds at once (32 waves per CU), and three beyond: a wave takes a second request."""
    scene, ws, Ks = model(pm, "hand")
    r = crossings_renderer
    r.set_scene_bytes(scene)
    if tm._emulated():
        cus = int(os.environ.get("PM_EMU_CUS", "256"))  # (what the emulated device reports)
    else:
        import torch

        cus = torch.cuda.get_device_properties(0).multi_processor_count
    base = [p for p in cc.pairs(pm, "hand") if p[0] < len(ws) and p[1] < len(ws)]
    for n in (32 * cus - 1, 32 * cus + 3):
        pairs = [base[(7 * k) % len(base)] for k in range(n)]
        _, count_info, _ = nx.crossings(scene, [(a, b, 0, 0) for a, b in pairs], False, ws, Ks=Ks)
        laid, rows = spread(pairs, [int(c) for c in count_info["n_crossings"]])
        want, want_info, _ = nx.crossings(scene, laid, False, ws, Ks=Ks)
        out, info, keep = device_call(pm, r, nx.records(laid), False, rows + 2, rows + 1)
        r.sync()
        assert_buffer(out, want, ("grid", n))
        assert_infos(info, want_info, ("grid", n))
        assert len(want) > 200


def _count_then_fill(pm, r, pairs, skip=False, stream=None):
    """What a caller without a model does: the cap = 0 pass, then an exactly packed device call.  Returns (records CROSSING [total],
    offsets, infos, the device buffer) and asserts that both passes count alike."""
    q0 = nx.records([(a, b, 0, 0) for a, b in pairs])
    _, info0, keep0 = device_call(pm, r, q0, skip, 1, 0, stream)
    tm.wait(r, stream)
    info0 = tm.as_rec(info0, nx.CROSSINGS_INFO, len(pairs)).copy()
    caps = [int(c) for c in info0["n_crossings"]]
    packed, total = nx.packed(pairs, caps)
    out, info, keep = device_call(pm, r, nx.records(packed), skip, total + 1, total, stream)
    tm.wait(r, stream)
    info = tm.as_rec(info, nx.CROSSINGS_INFO, len(pairs)).copy()
    assert info["n_crossings"].tolist() == caps and not (info["flags"] & nx.TRUNCATED).any()
    host = tm.host_view(out)
    assert (host[total:] == UNTOUCHED).all()
    offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    return np.ascontiguousarray(host[:total]).view(nx.CROSSING).reshape(-1), offsets, info, out


@pytest.mark.gpu
def test_the_relations_on_the_devices_own_answers(pm, crossings_renderer):
    """D29's relations between device calls, without the model.  (1) {B, A} answers {A, B} with the roles exchanged: the same index
    pairs, t and u exchanged bit for bit, side 1 <-> 2.  (2) A record with item_a >= item_b, under a cursor at its point with r = 2^-4
    whose near list is exactly its two edges (asserted on the CPU: a case where it is not is a broken case), is pm_snap_intersections'
    answer in item, index, t, x, y, item2, index2, u, byte for byte.  (3) Both halves of every record go into
    pm_positions_on_edges_device as they lie in device memory and are answered PM_MEASURE_FOUND."""
    r = crossings_renderer
    swapped = snapped = placed = 0
    for name in ("hand", "lanes"):
        scene, ws, Ks = model(pm, name)
        r.set_scene_bytes(scene)
        pairs = [p for p in cc.pairs(pm, name) if p[0] < len(ws) and p[1] < len(ws)]
        recs, offsets, infos, dev = _count_then_fill(pm, r, pairs)
        at = {p: k for k, p in enumerate(pairs)}
        # (1) swap
        for (a, b), k in at.items():
            if a == b or (b, a) not in at:
                continue
            mine, k2 = recs[offsets[k]:offsets[k + 1]], at[(b, a)]
            theirs = recs[offsets[k2]:offsets[k2 + 1]]
            theirs = theirs[np.lexsort((theirs["index_a"], theirs["index_b"]))]       # by (their j, their i): our (i, j)
            assert len(mine) == len(theirs), (name, a, b)
            for f, g in (("index_a", "index_b"), ("index_b", "index_a"), ("t", "u"), ("u", "t"), ("item_a", "item_b")):
                assert mine[f].tobytes() == theirs[g].tobytes(), (name, a, b, f)
            assert (mine["side"] + theirs["side"] == 3).all() and set(mine["side"].tolist()) <= {1, 2}
            swapped += len(mine)
        # (3) positions: the halves as they lie in device memory
        total = int(offsets[-1])
        halves = dev[:total].reshape(-1, 3, 4)[:, :2].reshape(-1, 4)
        halves = np.ascontiguousarray(halves) if isinstance(halves, np.ndarray) else halves.contiguous()
        pos, keep = tm.device_positions(pm, r, halves)
        r.sync()
        pos = tm.as_rec(pos, nm.LENGTH_AT, 2 * total)
        assert (pos["status"] == nm.FOUND).all() and pos["item"][0::2].tobytes() == recs["item_a"].tobytes() and pos["item"][1::2].tobytes() == recs["item_b"].tobytes()
        s_a, s_b = r.crossing_positions(recs)
        assert s_a.tobytes() == pos["s"][0::2].tobytes() and s_b.tobytes() == pos["s"][1::2].tobytes()
        placed += total
        # (2) D23, on the hand scene
        if name != "hand":
            continue
        mine = recs[recs["item_a"] >= recs["item_b"]]
        xyr = np.stack([mine["x"], mine["y"], np.full(len(mine), 2.0 ** -4, F32)], axis=1).astype(F32)
        E, Q = np_cross.Edges(bytes(scene)), np_snap.Queries(xyr)
        near = np_cross.near_mask(E, Q)
        for k, c in enumerate(mine):
            got = {(int(E.item[e]), int(E.index[e])) for e in np.flatnonzero(near[k])}
            assert got == {(int(c["item_a"]), int(c["index_a"])), (int(c["item_b"]), int(c["index_b"]))}, ("a broken case", c, got)
        snap = r.snap_intersections(xyr[:, :2], xyr[:, 2])
        assert (snap["kind"] == np_cross.INTERSECTION).all() and (snap["n_near"] == 2).all()
        for f, g in (("item", "item_a"), ("index", "index_a"), ("t", "t"), ("x", "x"), ("y", "y"), ("item2", "item_b"), ("index2", "index_b"), ("u", "u")):
            assert np.ascontiguousarray(snap[f]).tobytes() == np.ascontiguousarray(mine[g]).tobytes(), f
        snapped += len(mine)
    assert swapped > 2000 and snapped >= 12 and placed > 3000, (swapped, snapped, placed)


@pytest.mark.gpu
def test_the_workflow_cutting_a_polyline_at_its_crossings(pm, crossings_renderer):
    """Scissors: where the long Line crosses zig-5, crossing_positions gives the lengths along the zigzag and trim_units the pieces
    between them.  Every piece starts and ends on a cut vertex (or the item's own end), and a cut vertex lies on the crossing's edge."""
    scene, ws, Ks = model(pm, "lanes")
    N = cc.names(pm, "lanes")
    r = crossings_renderer
    r.set_scene_bytes(scene)
    Z, L = N["zig-5"], N["long_line"]
    recs, offsets, infos = r.crossings([Z], [L])
    assert len(recs) == 5 and recs["index_a"].tolist() == [0, 1, 2, 3, 4] and infos["n_a"].tolist() == [5]
    s_a, s_b = r.crossing_positions(recs)
    assert (np.diff(s_a.astype(np.int64)) > 0).all() and (np.diff(s_b.astype(np.int64)) > 0).all()
    T = ws[Z].T
    cuts = [0] + [int(s) for s in s_a] + [T]
    vs, voff, vinfo = r.trim_units([Z] * 6, cuts[:-1], cuts[1:])
    CUT = pm._lib.PM_TRIM_CUT
    for k in range(6):
        piece = vs[voff[k]:voff[k + 1]]
        assert len(piece) >= 2
        head, tail = piece[0], piece[-1]
        if k > 0:       # starts at crossing k - 1, on its edge
            assert head["flags"] & CUT and int(head["index"]) == int(recs["index_a"][k - 1])
            assert abs(float(head["x"]) - float(recs["x"][k - 1])) < 1e-3 and abs(float(head["y"]) - float(recs["y"][k - 1])) < 1e-3
        if k < 5:       # ends at crossing k
            assert tail["flags"] & CUT and int(tail["index"]) == int(recs["index_a"][k])
            assert abs(float(tail["x"]) - float(recs["x"][k])) < 1e-3 and abs(float(tail["y"]) - float(recs["y"][k])) < 1e-3
    assert sum(int(i["n_vertices"]) for i in vinfo) == 6 + 6 + 4      # two vertices a piece, and the zigzag's four inner vertices once each


def _flattened_scene_matches(pm, r, what):
    """Crossings equal np_crossings on the downloaded scene: every item against its paint-order neighbour, both ways, and against
    itself.  Returns the walks and the number of crossings."""
    scene = r.download_scene()
    ws, Ks = nm.walks(scene), nx.index_ranges(scene)
    n = len(ws)
    pairs = [(i, i + 1) for i in range(n)] + [(i + 1, i) for i in range(0, n, 2)] + [(i, i) for i in range(n)]
    infos = check_requests(pm, r, scene, ws, Ks, pairs, False, tm.new_stream(), what)
    assert infos["n_a"][:n].tolist() == Ks
    return ws, int(infos["n_crossings"].sum())


@pytest.mark.gpu
def test_crossings_follow_reflatten_groups(pm):
    import path_sets
    from test_groups_gpu import rot

    ps = path_sets.random_case(321).ps
    gmap = (np.arange(len(ps.paths), dtype=np.uint32) % 3).astype(np.uint32)
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 32.0, -16.0), (2.0, 0.0, 0.0, 2.0, 5.0, 5.0), rot(0.7, 1.0, 40.0, 30.0)])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), 1.0)
        ws0, n0 = _flattened_scene_matches(pm, r, "flattened")
        before = r.crossings(np.arange(len(ws0) - 1), np.arange(1, len(ws0)))[0]
        r.reflatten_groups(aff, np.array([1.0, 2.0, 1.0], F32))
        ws1, n1 = _flattened_scene_matches(pm, r, "moved")
        after = r.crossings(np.arange(len(ws1) - 1), np.arange(1, len(ws1)))[0]
        assert n0 > 0 and n1 > 0 and len(ws0) == len(ws1) and not tm.same(before, after)


@pytest.mark.gpu
def test_crossings_of_styled_and_dashed_strokes(pm):
    """Styled and dashed strokes answer as the outline Fills they are."""
    from np_stroke import MITER, SQUARE, style_bits
    from test_stroke_gpu import shapes

    ps = shapes(lambda k: (3 if k % 4 == 0 else 2) | style_bits(SQUARE, MITER))
    ps = ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps, (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 1.0)
        ws, n = _flattened_scene_matches(pm, r, "styled")
        assert n > 0 and max(len(w.segs) for w in ws) > 64 and all(w.kind in (nm.CLOSED, nm.NONE) for w in ws)


@pytest.mark.gpu
def test_argument_rules(pm):
    """Every PM_ERR_INVALID and PM_ERR_CAPACITY case, each with nothing written; n == 0; correct calls afterwards, derived by hand;
    the Python wrappers."""
    lib = pm._lib.load()
    OK = pm._lib.PM_OK
    with pm.Renderer(0) as r:
        out = np.full((16, 12), UNTOUCHED, np.int32)
        info = np.full((5, 4), UNTOUCHED, np.int32)
        # the X both ways, the first Polyline against itself, against the Circle
        good = nx.records(nx.packed([(0, 1), (1, 0), (0, 0), (0, 2)], [1, 1, 0, 2])[0])
        op, ip, qp = out.ctypes.data, info.ctypes.data, good.ctypes.data
        host = lambda q, n, flags, o, cap, i: lib.pm_item_crossings(r._h, q, n, flags, o, cap, i)  # noqa: E731
        dev = lambda q, n, flags, o, cap, i: lib.pm_item_crossings_device(r._h, q, n, flags, o, cap, i, None)  # noqa: E731
        for call in (host, dev):                                   # no resident scene
            assert call(qp, 4, 0, op, 16, ip) == INVALID
        # an X of two Polylines -- (0, 0) -> (8, 8) -> (8, 0) and (0, 4) -> (8, 4) -- and a Circle
        r.set_scene_bytes(hs._encode(pm, 3, lambda e: (e.polyline(np.array([[0.0, 0.0], [8.0, 8.0], [8.0, 0.0]]), 0x112233FF, 1.0),
                                                      e.polyline(np.array([[0.0, 4.0], [16.0, 4.0]]), 0x112233FF, 1.0), e.circle((50.0, 50.0), 5.0))))
        for call in (host, dev):
            for flags in (2, 6, 8, 16, 0x80000001):                # unknown flag bits, also with nothing to do
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

        for q in (bad(1, first=0), bad(1, first=2), bad(0, first=1), bad(3, first=3), bad(3, first=0)):   # a wrong first
            assert host(q.ctypes.data, 4, 0, op, 16, ip) == INVALID
        assert host(qp, 4, 0, op, 3, ip) == CAPACITY                # the total is 4
        assert host(qp, 4, 0, op, 0, ip) == CAPACITY
        big = nx.records(nx.packed([(0, 1), (0, 1)], [1 << 20, 1])[0])
        assert host(big.ctypes.data, 2, 0, op, (1 << 20) + 1, ip) == CAPACITY   # more than 2^20 records in one call
        r.sync()
        assert (out == UNTOUCHED).all() and (info == UNTOUCHED).all()
        # the count pass needs no buffer
        count = good.copy()
        count["first"] = 0
        count["cap"] = 0
        TR = nx.TRUNCATED
        assert host(count.ctypes.data, 4, 0, None, 0, ip) == OK and (info[4:] == UNTOUCHED).all()
        assert info[:4].view(nx.CROSSINGS_INFO).reshape(-1).tolist() == [(2, TR, 2, 1), (2, TR, 1, 2), (0, 0, 2, 2), (0, 0, 2, 0)]
        # correct calls afterwards, derived by hand: the first request's cap of 1 cuts its answer of 2, the last one's room stays untouched
        assert host(qp, 4, 0, op, 4, ip) == OK and (out[2:] == UNTOUCHED).all() and (info[4:] == UNTOUCHED).all()
        assert info[:4].view(nx.CROSSINGS_INFO).reshape(-1).tolist() == [(2, TR, 2, 1), (2, TR, 1, 2), (0, 0, 2, 2), (0, 0, 2, 0)]
        v = out[:2].view(nx.CROSSING).reshape(-1)
        # (0, 0) -> (8, 8) meets y = 4 at t = 1/2, u = 4/16; r = (8, 8), s = (16, 0): den = -128, side 2.  Swapped: t and u exchange, side 1
        assert v.tolist() == [(0, 0, 0.5, 0, 1, 0, 0.25, 0, 4.0, 4.0, 2, 0), (1, 0, 0.25, 0, 0, 0, 0.5, 0, 4.0, 4.0, 1, 0)]
        # the Python wrappers
        R = pm.renderer
        recs, offsets, infos = r.crossings([0, 1, 0, 0, 7], [1, 0, 0, 2, 0])
        assert recs.dtype == R.CROSSING_DTYPE and infos.dtype == R.CROSSINGS_INFO_DTYPE and offsets.tolist() == [0, 2, 4, 4, 4, 4]
        assert tm.same(recs[0], v[0]) and tm.same(recs[2], v[1]) and infos["flags"].tolist() == [0] * 5 and infos["n_b"].tolist() == [1, 2, 2, 0, 2]
        # (8, 8) -> (8, 0) meets y = 4 at t = 1/2, u = 8/16; r = (0, -8): den = 128
        assert recs[1].tolist() == (0, 1, 0.5, 0, 1, 0, 0.5, 0, 8.0, 4.0, 1, 0)
        one = r.crossings(0, [1, 1])
        assert one[1].tolist() == [0, 2, 4] and tm.same(one[0][:2], recs[:2]) and tm.same(one[0][2:], recs[:2])
        own = r.self_crossings([0, 1, 2])
        assert len(own[0]) == 0 and own[2]["n_a"].tolist() == [2, 1, 0] and own[2]["n_b"].tolist() == [2, 1, 0]
        assert len(r.crossings([], [])[0]) == 0 and r.self_crossings([])[1].tolist() == [0]
        s_a, s_b = r.crossing_positions(recs)
        U = 65536
        assert s_a.dtype == np.uint64 and s_a.tolist() == [int(np.floor(0.5 * nm.seg_units((0, 0), (8, 8)) + 0.5)), nm.seg_units((0, 0), (8, 8)) + 4 * U, 4 * U, 8 * U]
        assert s_b.tolist() == [4 * U, 8 * U, s_a.tolist()[0], s_a.tolist()[1]] and r.crossing_positions(recs[:0])[0].shape == (0,)
        for wrong in (lambda: r.crossings([0, 0], [1]), lambda: r.crossings([[0]], [1]), lambda: r.crossing_positions(np.zeros((2, 2), R.CROSSING_DTYPE))):
            with pytest.raises(ValueError):
                wrong()
        forged = recs[:1].copy()
        forged["index_a"] = 9
        with pytest.raises(ValueError):
            r.crossing_positions(forged)
        assert lib.pm_abi_version() == 600
        if not tm._emulated():
            import torch

            q4, o12, i4 = tm.to_device(good), torch.zeros((4, 12), dtype=torch.int32, device="cuda"), torch.zeros((4, 4), dtype=torch.int32, device="cuda")
            for wrong in (lambda: r.crossings_tensor(q4.cpu(), o12, i4), lambda: r.crossings_tensor(q4[:, :2].contiguous(), o12, i4),
                          lambda: r.crossings_tensor(q4, o12[:, :4].contiguous(), i4), lambda: r.crossings_tensor(q4, o12, i4[:2]),
                          lambda: r.crossings_tensor(q4, o12.float(), i4), lambda: r.crossings_tensor(q4, o12, i4[:, :2].contiguous())):
                with pytest.raises(TypeError):
                    wrong()
            r.crossings_tensor(q4, o12, i4)
            r.sync()
            assert tm.same(o12.cpu().numpy()[:2], out[:2]) and tm.same(i4.cpu().numpy(), info[:4])


@pytest.mark.gpu
def test_requests_between_frames_and_after_a_replacement(pm, pmo):
    """Frames rendered before and after the requests have the bytes they have without them; a device call on a caller's stream followed
    at once by a re-flatten answers for the scene resident at the call; a replacement between two requests gives each its own."""
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        ws, Ks = nm.walks(scene), nx.index_ranges(scene)
        longest = max(range(len(ws)), key=lambda i: len(ws[i].segs))
        pairs = [(i, i + 1) for i in range(0, len(ws) - 1, 5)] + [(longest, longest), (longest, longest - 1)]
        _, count_info, _ = nx.crossings(scene, [(a, b, 0, 0) for a, b in pairs], False, ws, Ks=Ks)
        caps = [int(c) + 2 for c in count_info["n_crossings"]]          # room to spare
        packed, total = nx.packed(pairs, caps)
        q = nx.records(packed)
        want, want_info, _ = nx.crossings(scene, packed, False, ws, Ks=Ks)
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
            assert_buffer(o, want, "between frames")
            assert_infos(i, want_info, "between frames")
        assert len(ws[longest].segs) > 256 and int(want_info["n_crossings"].sum()) > 0
        r.render()
        dev_out, dev_info, keep = device_call(pm, r, q, False, total + 1, total, s)     # frame in flight, request, replacement, request
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        after_out, after_info, keep2 = device_call(pm, r, q, False, total + 1, total, s)
        tm.wait(r, s)
        assert_buffer(dev_out, want, "before the replacement")
        assert_infos(dev_info, want_info, "before the replacement")
        scene2 = r.download_scene()
        ws2, Ks2 = nm.walks(scene2), nx.index_ranges(scene2)
        want2, want_info2, _ = nx.crossings(scene2, packed, False, ws2, Ks=Ks2)
        assert_buffer(after_out, want2, "after the replacement")
        assert_infos(after_info, want_info2, "after the replacement")
        assert not tm.same(want_info, want_info2) or want != want2


@pytest.mark.gpu
def test_cli_crossings_and_self_crossings(pm, tmp_path, capsys):
    """--crossings A,B and --self-crossings ITEM: a header line per request, then one line per crossing with its position along A."""
    from piet_metal_amd import cli

    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        n_items = r.stats()["n_items"]
        recs, offsets, infos = r.crossings(np.arange(n_items - 1), np.arange(1, n_items))
        a = int(np.argmax(infos["n_crossings"]))
        assert int(infos["n_crossings"][a]) > 0
        pairs = [(a, a + 1), (a + 1, a), (100000, 0), (a, a)]
        recs, offsets, infos = r.crossings([p[0] for p in pairs], [p[1] for p in pairs])
        s_a, _ = r.crossing_positions(recs)
        want = []
        for k, (x, y) in enumerate(pairs):
            head = f"self-crossings item {x}" if x == y else f"crossings items {x},{y}"
            want.append(f"{head}: {int(infos[k]['n_crossings'])} edges {int(infos[k]['n_a'])} x {int(infos[k]['n_b'])}")
            want += [cli.crossing_line(recs[p], s_a[p]) for p in range(int(offsets[k]), int(offsets[k + 1]))]
    args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--crossings", f"{a},{a + 1}", "--crossings", f"{a + 1},{a}", "--crossings", "100000,0",
            "--self-crossings", str(a)]
    assert cli.main(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("crossings items ", "self-crossings item ", "  ")) and (" segment " in ln or " edges " in ln)]
    assert lines == want and "crossings items 100000,0: 0 edges 0 x " in want[1 + int(infos[0]["n_crossings"]) + 1 + int(infos[1]["n_crossings"])]
    assert " a segment " in want[1] and " b segment " in want[1] and " side " in want[1] and " at " in want[1]
    for wrong in (["--crossings", "40"], ["--crossings", "40,1,2"], ["--crossings", "-1,2"], ["--crossings", "a,b"], ["--self-crossings", "1,2"], ["--self-crossings", "-4"]):
        with pytest.raises(SystemExit):
            cli.main(args[:6] + wrong)
    capsys.readouterr()


# ---- CPU: the rule against exact arithmetic ----------------------------------------------------------------------------------------

def _exact(e, f):
    """D29's step 3 in rational arithmetic: (crosses, [(value, bound)]) or (False, None) where den == 0."""
    ax, ay, bx, by, cx, cy, dx, dy = (Fraction(float(v)) for v in (*e, *f))
    rx, ry, sx, sy = bx - ax, by - ay, dx - cx, dy - cy
    den = rx * sy - ry * sx
    if den == 0:
        return False, None
    wx, wy = cx - ax, cy - ay
    t, u = (wx * sy - wy * sx) / den, (wx * ry - wy * rx) / den
    return 0 <= t <= 1 and 0 <= u <= 1, [(t, 0), (t, 1), (u, 0), (u, 1)]


def test_the_rule_against_exact_arithmetic():
    """D23's method: seeded segments on integer coordinates in [0, 32], every pair of them that shares no end.  "Crosses" by Fractions
    EQUALS the rule wherever t and u are off their bounds by a relative 1e-9; and in real arithmetic the box rule removes nothing:
    a pair that crosses exactly has meeting boxes.  The counts stand in D29."""
    eps = Fraction(1, 10**9)
    total = decisive = cross = disagree = 0
    for seed in range(40):
        seg = np.random.default_rng([seed, 29]).integers(0, 33, (14, 4)).astype(F32)
        for i in range(len(seg)):
            for j in range(len(seg)):
                e, f = seg[i], seg[j]
                if i == j or (e[0], e[1]) in ((f[0], f[1]), (f[2], f[3])) or (e[2], e[3]) in ((f[0], f[1]), (f[2], f[3])):
                    continue
                total += 1
                got = nx.pair(e, f) is not None
                exact, parts = _exact(e, f)
                if parts is not None and any(abs(v - bound) <= eps for v, bound in parts):
                    continue            # (on integer coordinates: t or u exactly on a bound; the rule's answer is then the exact one too)
                decisive += 1
                cross += exact
                disagree += got != exact
    for seed in range(40):              # the pairs left out above are decided alike: integer numerators and denominators are exact in binary64
        seg = np.random.default_rng([seed, 29]).integers(0, 33, (14, 4)).astype(F32)
        for i in range(len(seg)):
            for j in range(len(seg)):
                e, f = seg[i], seg[j]
                if i == j or (e[0], e[1]) in ((f[0], f[1]), (f[2], f[3])) or (e[2], e[3]) in ((f[0], f[1]), (f[2], f[3])):
                    continue
                assert (nx.pair(e, f) is not None) == _exact(e, f)[0], (seed, i, j)
    print(f"{total} ordered pairs that share no end, {decisive} decisive ({100.0 * decisive / total:.1f} %), {cross} cross, {disagree} disagreements")
    assert total > 7000 and decisive >= 0.95 * total and cross >= 500 and disagree == 0


# ---- CPU: np_crossings itself -------------------------------------------------------------------------------------------------------

def test_np_crossings_against_hand_derived_coordinates(pm):
    scene, ws, Ks = model(pm, "hand")
    N = cc.names(pm, "hand")
    assert Ks == [1, 1, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 4, 9, 1, 1, 0, 0, 1, 1, 4, 1, 1, 1, 1, 1, 1, 1, 1]

    def ask(a, b, skip=False):
        w, k = (ws, Ks) if not skip else model(pm, "hand", True)[1:]
        _, infos, answers = nx.crossings(scene, [(N[a] if isinstance(a, str) else a, N[b] if isinstance(b, str) else b, 0, 99)], skip, w, Ks=k)
        return [(r[1], r[5], float(r[2]), float(r[6]), float(r[8]), float(r[9]), r[10]) for r in answers[0]], tuple(int(v) for v in infos[0])

    third, two_thirds = float(F32(1.0 / 3.0)), float(F32(2.0 / 3.0))
    assert ask("x_up", "x_down") == ([(0, 0, 0.5, 0.5, 5.0, 5.0, 2)], (1, 0, 1, 1))
    assert ask("x_down", "x_up") == ([(0, 0, 0.5, 0.5, 5.0, 5.0, 1)], (1, 0, 1, 1))
    assert ask("through", "square") == ([(0, 1, 0.75, 0.5, 30.0, 5.0, 1), (0, 3, 0.25, 0.5, 20.0, 5.0, 2)], (2, 0, 1, 4))
    assert ask("square", "through") == ([(1, 0, 0.5, 0.75, 30.0, 5.0, 2), (3, 0, 0.5, 0.25, 20.0, 5.0, 1)], (2, 0, 4, 1))
    assert ask("t_bar", "t_stem") == ([(0, 0, 0.5, 0.0, 45.0, 0.0, 1)], (1, 0, 1, 1))                       # a T-junction counts
    assert ask("v_left", "v_right") == ([], (0, 0, 1, 1)) and ask("par_a", "par_b")[0] == [] and ask("col_a", "col_b")[0] == []
    assert ask("fan_a", "fan_b")[0] == [] and ask("fan_b", "fan_a")[0] == [] and ask("fan_c", "fan_d")[0] == [] and ask("fan_d", "fan_c")[0] == []   # each of the four shared ends
    assert ask("bow_tie", "bow_tie")[1][0] == 1                                                                 # (a == d: the closing joint of edges 0 and 3)
    assert ask("eight", "eight") == ([(0, 2, 0.5, 0.5, 5.0, 45.0, 1)], (1, 0, 3, 3))                         # each pair once
    assert ask("bow_tie", "bow_tie") == ([(0, 2, 0.5, 0.5, 25.0, 45.0, 1)], (1, 0, 4, 4))
    assert ask("compound", "compound") == ([(1, 5, 0.5, third, 50.0, 45.0, 2), (2, 7, 0.5, two_thirds, 45.0, 50.0, 1)], (2, 0, 9, 9))   # (separators at 4 and 8)
    assert ask("line_up", "line_down")[0] == [(0, 0, 0.5, 0.5, 65.0, 25.0, 2)]
    for a in ("circle", "one_point", len(Ks), 0xFFFFFFFF):
        assert ask(a, "x_up") == ([], (0, 0, 0, 1)) and ask("x_up", a) == ([], (0, 0, 1, 0)) and ask(a, a) == ([], (0, 0, 0, 0))
    assert ask("clear", "opaque")[1] == (1, 0, 1, 1) and ask("clear", "opaque", True) == ([], (0, 0, 0, 1)) and ask("opaque", "clear", True) == ([], (0, 0, 1, 0))
    assert ask("nan_poly", "nan_poly") == ([(0, 3, 0.5, 0.5, 5.0, 65.0, 1)], (1, 0, 4, 4))                   # segments 1 and 2 have a NaN end
    assert [c[:2] for c in ask("nan_line", "nan_poly")[0]] == [(0, 0), (0, 3)]
    assert ask("touch_hit", "touch_e") == ([(0, 0, 0.5, 1.0, 10.0, 90.0, 2)], (1, 0, 1, 1)) and ask("touch_miss", "touch_e")[0] == []
    # a cap cuts, and says so; beyond out_cap nothing is written
    T, S = N["through"], N["square"]
    writes, infos, _ = nx.crossings(scene, [(T, S, 4, 1), (T, S, 7, 5), (T, S, 0, 0)], False, ws, out_cap=8, Ks=Ks)
    assert sorted(writes) == [4, 7] and infos["flags"].tolist() == [nx.TRUNCATED] * 3 and infos["n_crossings"].tolist() == [2, 2, 2]
    # the limit is a count of index ranges
    _, infos, _ = nx.crossings(scene, [(0, 1, 0, 9)], False, ws, Ks=[1 << 14, (1 << 14) + 1] + Ks[2:])
    assert infos.tolist() == [(0, nx.TOO_MANY, 1 << 14, (1 << 14) + 1)]


# ---- CPU: the cases are what they claim -----------------------------------------------------------------------------------------

def test_the_cases_are_what_they_claim(pm):
    """Conditions on the committed scenes and request lists, not measurements: every situation the kernel treats differently is met."""
    scene, ws, Ks = model(pm, "lanes")
    N = cc.names(pm, "lanes")
    pairs = cc.pairs(pm, "lanes")
    _, infos, answers = nx.crossings(scene, [(a, b, 0, 0) for a, b in pairs], False, ws, Ks=Ks)
    at = {p: k for k, p in enumerate(pairs)}
    L = N["long_line"]
    assert [Ks[N[f"zig-{z}"]] for z in cc.ZIG] == list(cc.ZIG) == [1, 4, 5, 255, 256, 257, 300] and Ks[L] == 1 and Ks[N["star"]] == cc.STAR > 256
    chunks = lambda k: -(-k // 4)  # noqa: E731
    assert chunks(255) == chunks(256) == 64 and chunks(257) == 65 and chunks(300) > 64 and chunks(cc.STAR) > 64      # either side of ForItemChunks' threshold
    first_chunk = np.cumsum([0] + [chunks(k) if k > 1 or i != L else 0 for i, k in enumerate(Ks)])
    assert any(first_chunk[N[f"zig-{z}"]] % 8 for z in (257, 300))          # an item's first super-chunk holds chunks of its neighbour
    for z in cc.ZIG:
        one = answers[at[(L, N[f"zig-{z}"])]]
        assert [r[5] for r in one] == list(range(z)) and {r[1] for r in one} == {0}                                  # every j on ONE i: more than 64 at 255 and up
        assert [r[1] for r in answers[at[(N[f"zig-{z}"], L)]]] == list(range(z))                                        # ... and every i
        assert answers[at[(N[f"zig-{z}"], N[f"zig-{z}"])]] == []
    many = answers[at[(N["zig-300"], N["zig-shifted"])]]
    assert len({r[1] for r in many}) > 64 and len({r[5] for r in many}) > 64 and len(many) > 256
    star = answers[at[(N["star"], N["star"])]]
    assert len(star) == cc.STAR and all(r[1] < r[5] for r in star) and max(r[5] for r in star) == cc.STAR - 1
    assert 0 < len(answers[at[(L, N["star"])]]) < 20                                                                  # most chunks culled, a few not
    laid, cap = cc.layout_requests(pm)
    _, infos, _ = nx.crossings(scene, laid, False, ws, out_cap=cap, Ks=Ks)
    assert {(int(i["n_crossings"]), c) for i, (_, _, _, c) in zip(infos, laid)} >= {(300, 0), (300, 299), (300, 300), (300, 301), (300, 64), (300, 65)}
    assert any(f + c > cap > f for _, _, f, c in laid) and any(f == cap for _, _, f, _ in laid) and any(f == 0xFFFFFFFF for _, _, f, _ in laid)
    assert sorted(f for _, _, f, _ in laid[:11]) != [f for _, _, f, _ in laid[:11]]                                     # out of order
    # the limit: the products either side of 2^28, and the pair of 16 384 kept apart
    scene, ws, Ks = model(pm, "limit")
    N = cc.names(pm, "limit")
    assert Ks == [cc.BIG, cc.BIG, cc.BIG - 1, cc.BIG - 1, 1] and cc.BIG * cc.BIG > nx.MAX_PAIRS and cc.BIG * (cc.BIG - 1) > nx.MAX_PAIRS == (cc.BIG - 1) ** 2
    ea, eb = nx.edges(ws[N["most_a"]])[1], nx.edges(ws[N["most_far"]])[1]
    assert not nx._boxes_meet(ea, eb) and ea[:, 1::2].max() < eb[:, 1::2].min()
    assert (N["most_a"], N["most_a"]) not in cc.pairs(pm, "limit") and (N["most_far"], N["most_far"]) not in cc.pairs(pm, "limit")   # no uncullable 2^28-pair walk
    # the hand scene: the groups keep apart
    scene, ws, Ks = model(pm, "hand")
    pairs = cc.pairs(pm, "hand")
    _, infos, answers = nx.crossings(scene, [(a, b, 0, 0) for a, b in pairs], False, ws, Ks=Ks)
    assert int(infos["n_crossings"].sum()) == 23 and {p for p in pairs if p[0] == p[1]} >= {(i, i) for i in range(len(ws))}
    assert len(ws[cc.names(pm, "hand")["one_point"]].segs) == 0 and ws[cc.names(pm, "hand")["circle"]].kind == nm.NONE


# ---- CPU: the header ----------------------------------------------------------------------------------------------------------

def test_the_header_and_the_record_sizes(pm):
    hdr = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    got = dict(re.findall(r"^#define (PM_CROSSINGS?_[A-Z_]+) (\w+)u\b", hdr, re.M))
    assert {k: int(v, 0) for k, v in got.items()} == {"PM_CROSSINGS_TRUNCATED": 1, "PM_CROSSINGS_TOO_MANY": 2, "PM_CROSSINGS_MAX_PAIRS": 1 << 28,
                                                      "PM_CROSSING_SIDE_POS": 1, "PM_CROSSING_SIDE_NEG": 2}
    L = pm._lib
    assert (L.PM_CROSSINGS_TRUNCATED, L.PM_CROSSINGS_TOO_MANY, L.PM_CROSSINGS_MAX_PAIRS) == (nx.TRUNCATED, nx.TOO_MANY, nx.MAX_PAIRS)
    assert (L.PM_CROSSING_SIDE_POS, L.PM_CROSSING_SIDE_NEG) == (nx.SIDE_POS, nx.SIDE_NEG)
    for name, size in (("pm_crossings_query", 16), ("pm_crossing", 48), ("pm_crossings_info", 16)):
        assert re.search(r"\} " + name + r";\s*/\* " + str(size) + r" bytes \*/", hdr), name
    assert "uint32_t item_a, item_b, first, cap; } pm_crossings_query" in hdr and "uint32_t n_crossings, flags, n_a, n_b; } pm_crossings_info" in hdr
    R = pm.renderer
    assert R.CROSSINGS_QUERY_DTYPE == nx.CROSSINGS_QUERY and R.CROSSING_DTYPE == nx.CROSSING and R.CROSSINGS_INFO_DTYPE == nx.CROSSINGS_INFO
    offsets = {k: nx.CROSSING.fields[k][1] for k in nx.CROSSING.names}
    assert offsets == {"item_a": 0, "index_a": 4, "t": 8, "reserved_a": 12, "item_b": 16, "index_b": 20, "u": 24, "reserved_b": 28, "x": 32, "y": 36, "side": 40, "reserved": 44}
    assert [nx.CROSSING.fields[k][1] for k in ("item_a", "index_a", "t", "reserved_a")] == [nm.EDGE_QUERY.fields[k][1] for k in ("item", "index", "t", "reserved")]
    assert "int pm_item_crossings(pm_ctx *c, const pm_crossings_query *q, size_t n, uint32_t flags, pm_crossing *out, size_t out_cap, pm_crossings_info *info);" in hdr
    assert "int pm_item_crossings_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream);" in hdr
    assert "#define PM_ABI_VERSION 600" in hdr
    assert len(L.SIGNATURES["pm_item_crossings"][1]) == 7 and len(L.SIGNATURES["pm_item_crossings_device"][1]) == 8
    kernels = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_crossings.h")).read()
    code = kernels.split("#pragma once")[1]
    assert "kCrossingsMaxPairs = 1ull << 28" in code and '#include "pm_trim.h"' in code
    for shared in ("MeasureWalkOf(", "MeasureEnds(", "ForItemChunks(", "BoundsWaveUnion(", "RankBelow(", "TakeLowestLane("):
        assert shared in code and "__device__ __forceinline__ " + shared.split("(")[0] not in kernels.replace("MeasureWalk MeasureWalkOf", "")
    assert "atomic" not in code and "__shared__" not in kernels
    host = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    assert "PM_CROSSINGS_MAX_PAIRS == pm::kCrossingsMaxPairs" in host and "sizeof(pm_crossings_query) == 16" in host and "sizeof(pm_crossing) == 48" in host
    assert "sizeof(pm_crossings_info) == 16" in host and host.index('#include "pm_trim.h"') < host.index('#include "pm_crossings.h"')
    assert "D29" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_crossings_under_wave64_emulation(built):
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

def test_the_crossings_kernel_uses_no_scratch(tmp_path):
    """pm_crossings_kernel by the flags the library is built with: no private segment and VGPRs within 128; the LDS size is printed
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
        if "pm_crossings_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        sgpr = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"pm_crossings_kernel: {vgpr} VGPRs, {sgpr} SGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128, (scratch, vgpr, lds)
    assert found == 1
    assert "-ffp-contract=off" in flags and "pm_crossings.h" in mk     # (editing the header rebuilds the library)
