"""Snapping, pm_snap / pm_snap_device (decision D21): the nearest vertex or point of an edge to a cursor -- which item, which index,
where, how far.

The bar everywhere: the 32-byte records EQUAL to tests/np_snap.py as bytes, the bits of d2 included, no query left out -- through the
host and the device call, under the three combinations of PM_SNAP_VERTICES and PM_SNAP_EDGES, with and without
PM_HIT_SKIP_TRANSPARENT, with and without skip_items.  tests/snap_cases.py builds the scenes and places the queries.

-m gpu: small scenes of every item kind with ties, the item walk, long items, the hand-derived answers, output discipline and the
grid, the argument rules, composition with pm_select_rect_device, ordering against scene replacement and frames, the CLI.
CPU: the cases are what they claim (numpy alone); the hand-derived answers; D21 against D13 on grids of points (np_snap against
np_hit, no kernel); np_snap's two evaluation orders; the -m gpu part against the wave64 emulation of the kernel; the compiler's
listing."""
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
import np_hit  # noqa: E402
import np_snap  # noqa: E402
import snap_cases as sc  # noqa: E402

NONE = sc.NONE
V, E = np_snap.VERTEX, np_snap.EDGE
REC = np_snap.RECORD
UNTOUCHED = 0x7EADBEEF
# small scenes, walk, long, known answers, output discipline, argument rules, composition, ordering (2), CLI
N_GPU_TESTS = len(sc.SMALL) + len(sc.WALK_SIZES) + len(sc.LONG_IDS) + 1 + 1 + 1 + 1 + 2 + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def snap_flags(pm, vertices, edges, skip):
    L = pm._lib
    return (L.PM_SNAP_VERTICES if vertices else 0) | (L.PM_SNAP_EDGES if edges else 0) | (L.PM_HIT_SKIP_TRANSPARENT if skip else 0)


def device_snap(pm, r, xyr, vertices=True, edges=True, skip=False, mask=None, pad=0, stream=None):
    """pm_snap_device into n + pad records filled with UNTOUCHED, not waited for: (records as int32 [n + pad, 8], keep-alive).  Under
    the emulation device memory is host memory and the arrays are numpy's; on the GPU they are torch's.  mask: None, a numpy array
    of words (copied to the device) or device words as they are."""
    xyr = np.ascontiguousarray(xyr, np.float32).reshape(-1, 3)
    n = len(xyr)
    if _emulated():
        out = np.full((n + pad, 8), UNTOUCHED, np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
        pm._lib.check(pm._lib.load().pm_snap_device(r._h, xyr.ctypes.data, n, snap_flags(pm, vertices, edges, skip), m.ctypes.data if m is not None else None,
                                                    m.size if m is not None else 0, out.ctypes.data, None), "pm_snap_device")
        return out, (xyr, m)
    import torch

    dq = torch.from_numpy(xyr).cuda()
    out = torch.full((n + pad, 8), UNTOUCHED, dtype=torch.int32, device="cuda")
    m = None if mask is None else (torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32)).cuda() if isinstance(mask, np.ndarray) else mask)
    r.snap_tensor(dq, out[:n], skip_items=m, stream=stream, vertices=vertices, edges=edges, skip_transparent=skip)
    return out, (dq, m)


def as_rec(a, n=None):
    """RECORD [n] of an int32 [., 8] array of either kind."""
    a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    a = np.ascontiguousarray(a[:n] if n is not None else a)
    return a.view(REC).reshape(-1)


def same(got, want):
    return got.tobytes() == want.tobytes()


def differing(got, want):
    return np.flatnonzero((got.view(np.uint8).reshape(-1, 32) != np.ascontiguousarray(want).view(np.uint8).reshape(-1, 32)).any(axis=1))


def check_case(pm, r, case, skips=(False, True), masks=(False, True)):
    """Host and device, under every combination of flags: equal to np_snap."""
    for vertices, edges in sc.FLAG_SETS:
        for skip in skips:
            for masked in masks:
                want = case.expected(vertices, edges, skip, masked)
                mask = case.mask if masked else None
                dev, keep = device_snap(pm, r, case.xyr, vertices, edges, skip, mask)
                got = r.snap(case.xyr[:, :2], case.xyr[:, 2], vertices, edges, skip, mask)      # (synchronises the context's stream: the device call is done)
                bad = differing(got, want)
                assert bad.size == 0, (case, vertices, edges, skip, masked, len(bad), [(case.xyr[k].tolist(), got[k], want[k]) for k in bad[:6]])
                d = as_rec(dev)
                bad = differing(d, want)
                assert bad.size == 0, (case, "device", vertices, edges, skip, masked, len(bad), [(case.xyr[k].tolist(), d[k], want[k]) for k in bad[:6]])


@pytest.fixture(scope="module")
def snap_renderer(pm):
    """Never resized: snapping needs a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", sc.SMALL)
def test_small_scenes(pm, snap_renderer, name):
    """The ties scene, mixed_scene, edge_scene (items at negative coordinates and beyond 65 535), a scene of non-finite points and one of
    segments whose far end at 1e30 absorbs the near one, under a few hundred queries: on vertices and edges, at exactly r, one f32 step short of it, r = 0, not a query at all."""
    case = sc.small_case(pm, name)
    snap_renderer.set_scene_bytes(case.scene)
    check_case(pm, snap_renderer, case)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sc.WALK_SIZES)
def test_item_walk_by_item_count(pm, snap_renderer, n):
    """One item, one fewer than a step of the walk, a step, one more, two steps and their neighbours, 200: every item is the nearest
    to some query -- the first, the last, the ones at either end of a step."""
    case = sc.walk_case(pm, n)
    snap_renderer.set_scene_bytes(case.scene)
    assert snap_renderer.stats()["n_items"] == n
    check_case(pm, snap_renderer, case)


@pytest.mark.gpu
@pytest.mark.parametrize("ident", sc.LONG_IDS)
def test_long_items(pm, snap_renderer, ident):
    """A Fill, a compound Fill and a Polyline of 64, 65, 512 and 513 chunks exactly: the nearest candidate in the first chunk, the last,
    the one behind the 64th super-chunk; on a chunk box's edge at exactly r; the same distance in two chunks."""
    case = sc.long_case(pm, ident)
    snap_renderer.set_scene_bytes(case.scene)
    check_case(pm, snap_renderer, case, skips=(False,))


@pytest.mark.gpu
def test_hand_derived_answers(pm, snap_renderer):
    """snap_cases.KNOWN, worked out in its comments."""
    r = snap_renderer
    r.set_scene_bytes(sc.ties_scene(pm))
    want = sc.known_records()
    for k, (q, (vertices, edges), skip, _) in enumerate(sc.KNOWN):
        got = r.snap(np.array([q[:2]], np.float32), q[2], vertices, edges, skip)
        assert same(got, want[k : k + 1]), (q, vertices, edges, skip, got, want[k])
        dev, keep = device_snap(pm, r, [q], vertices, edges, skip)
        r.sync()
        assert same(as_rec(dev), want[k : k + 1]), (q, vertices, edges, skip, as_rec(dev), want[k])


@pytest.mark.gpu
def test_output_discipline_and_the_grid(pm, snap_renderer):
    """1 ... 7 queries and one query either side of what the grid holds at once (32 per CU: eight workgroups of four waves) into
    arrays four records too long: the records beyond n stay as they were -- a short list repeated, so that a stride error is a
    wrong VALUE.  n == 0 writes nothing."""
    import ctypes as C

    case = sc.walk_case(pm, 65)
    r = snap_renderer
    r.set_scene_bytes(case.scene)
    short = case.xyr[[0, 64, 65 + 7, 130 + 33, 195, 196, 197, 200, 3]]
    want = np_snap.snap(case.scene, short)
    assert len(set(want["item"].tolist())) >= 5 and NONE in want["item"] and {V, E} <= set(want["kind"].tolist())
    if _emulated():
        cus = int(os.environ.get("PM_EMU_CUS", "256"))  # (what the emulated device reports)
    else:
        import torch

        cus = torch.cuda.get_device_properties(0).multi_processor_count
    lib = pm._lib.load()
    for n in [1, 2, 3, 4, 5, 6, 7, 32 * cus - 1, 32 * cus, 32 * cus + 1]:
        reps = -(-n // len(short))
        q = np.ascontiguousarray(np.tile(short, (reps, 1))[:n])
        w = np.tile(want, reps)[:n]
        dev, keep = device_snap(pm, r, q, pad=4)
        host = np.full((n + 4, 8), UNTOUCHED, np.int32)
        assert lib.pm_snap(r._h, q.ctypes.data, n, snap_flags(pm, True, True, False), None, 0, host.ctypes.data) == pm._lib.PM_OK
        r.sync()
        for got in (host, dev if isinstance(dev, np.ndarray) else dev.cpu().numpy()):
            assert same(as_rec(got, n), w), (n, differing(as_rec(got, n), w)[:8].tolist())
            assert (got[n:] == UNTOUCHED).all(), n
    host = np.full((4, 8), UNTOUCHED, np.int32)
    dev, keep = device_snap(pm, r, np.zeros((0, 3), np.float32), pad=4)
    assert lib.pm_snap(r._h, short.ctypes.data, 0, snap_flags(pm, True, True, False), None, 0, host.ctypes.data) == pm._lib.PM_OK
    assert lib.pm_snap(r._h, None, 0, snap_flags(pm, False, True, False), None, 0, None) == pm._lib.PM_OK
    r.sync()
    assert (host == UNTOUCHED).all() and (as_rec(dev).view(np.int32) == UNTOUCHED).all()
    assert C.sizeof(C.c_double) == 8 and REC.itemsize == 32 and pm.renderer.SNAP_DTYPE == REC


@pytest.mark.gpu
def test_argument_rules(pm, pmo):
    lib = pm._lib.load()
    L = pm._lib
    OK, INVALID = L.PM_OK, L.PM_ERR_INVALID
    both = L.PM_SNAP_VERTICES | L.PM_SNAP_EDGES
    with pm.Renderer(0) as r:
        out = np.full((4, 8), UNTOUCHED, np.int32)
        q = np.array([[50, 50, 10]] * 4, np.float32)
        words = np.zeros(16, np.uint32)
        qp, op, wp = q.ctypes.data, out.ctypes.data, words.ctypes.data
        calls = [lambda *a: lib.pm_snap(r._h, *a), lambda *a: lib.pm_snap_device(r._h, *a, None)]      # (xyr, n, flags, skip_items, n_skip, out)
        for call in calls:
            assert call(qp, 4, both, None, 0, op) == INVALID                   # no scene: what pm_hit_test says
        r.set_scene_bytes(pmo.scene_path_test())
        assert r.stats()["n_items"] == 1
        for call in calls:
            assert call(qp, 4, 0, None, 0, op) == INVALID                      # neither vertices nor edges
            assert call(qp, 4, L.PM_HIT_SKIP_TRANSPARENT, None, 0, op) == INVALID
            assert call(qp, 4, both | 8, None, 0, op) == INVALID               # unknown flag bits
            assert call(qp, 4, both | 0x80000000, None, 0, op) == INVALID
            assert call(None, 4, both, None, 0, op) == INVALID                 # a NULL pointer with n > 0
            assert call(qp, 4, both, None, 0, None) == INVALID
            assert call(qp, 4, both, wp, 0, op) == INVALID                     # skip_items shorter than the scene
            assert call(qp, 4, both, None, 1, op) == INVALID                   # no skip_items, but a count
            assert call(qp, 0, both, wp, 0, op) == INVALID                     # ... also with nothing to do
            assert call(qp, 0, 0, None, 0, op) == INVALID
            assert call(None, 0, both, None, 0, None) == OK                    # nothing to do
            assert call(qp, 0, both, wp, 16, op) == OK
        r.sync()
        assert (out == UNTOUCHED).all()
        # more words than items: fine.  (Only the host call may be given these arrays to work on: they are host memory)
        assert calls[0](qp, 3, L.PM_SNAP_EDGES | L.PM_HIT_SKIP_TRANSPARENT, wp, 16, op) == OK
        assert (out[3] == UNTOUCHED).all() and (out[:3] != UNTOUCHED).any(axis=1).all()
        dev, keep = device_snap(pm, r, q[:3], vertices=False, skip=True, mask=words, pad=1)
        r.sync()
        assert same(as_rec(dev, 3), out[:3].view(REC).reshape(-1)) and (as_rec(dev)[3:].view(np.int32) == UNTOUCHED).all()
        assert lib.pm_abi_version() == 600
        # the Python wrappers
        with pytest.raises(ValueError):
            r.snap(np.zeros((3, 3), np.float32), 1.0)
        with pytest.raises(ValueError):
            r.snap(np.zeros((3, 2), np.float32), [1.0, 2.0])
        with pytest.raises(ValueError):
            r.snap(np.zeros((3, 2), np.float32), 1.0, vertices=False, edges=False)
        got = r.snap(np.zeros((0, 2), np.float32), 1.0)
        assert got.shape == (0,) and got.dtype == REC
        assert r.snap(np.zeros((2, 2), np.float32), [1.0, 2.0]).shape == (2,)
        if not _emulated():
            import torch

            o = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
            x = torch.zeros((4, 3), device="cuda")
            with pytest.raises(TypeError):
                r.snap_tensor(torch.zeros((4, 3)), o)                                  # not on the device
            with pytest.raises(TypeError):
                r.snap_tensor(torch.zeros((4, 2), device="cuda"), o)                   # points without radii
            with pytest.raises(TypeError):
                r.snap_tensor(x, o[:3])
            with pytest.raises(TypeError):
                r.snap_tensor(x, torch.zeros((4, 8), device="cuda"))                   # floating point
            with pytest.raises(TypeError):
                r.snap_tensor(x, o, skip_items=torch.zeros(4, device="cuda"))
            r.snap_tensor(x, o, skip_items=torch.zeros(1, dtype=torch.int32, device="cuda"))
            r.sync()


@pytest.mark.gpu
def test_selection_words_are_skip_items_without_a_read_back(pm, snap_renderer):
    """pm_select_rect_device's words go into pm_snap_device as they were written, on the same stream: what the marquee touched is
    never the answer, and the records are np_snap's under the same mask."""
    import np_rect

    def device_select(rect, n_words):
        """pm_select_rect_device into n_words words filled with UNTOUCHED, not waited for."""
        if _emulated():
            words = np.full(n_words, UNTOUCHED, np.uint32)
            rc = np.ascontiguousarray(rect, np.float32)
            pm._lib.check(pm._lib.load().pm_select_rect_device(r._h, rc.ctypes.data, 0, words.ctypes.data, words.size, None), "pm_select_rect_device")
            return words
        import torch

        words = torch.full((n_words,), UNTOUCHED, dtype=torch.int32, device="cuda")
        r.select_rect_tensor(*[float(v) for v in rect], words)
        return words

    case = sc.small_case(pm, "mixed")
    r = snap_renderer
    r.set_scene_bytes(case.scene)
    n_items = len(case.mask)
    for rect in ([90, 90, 260, 260], [0, 0, 600, 600], [1000, 1000, 1010, 1010]):
        words = device_select(rect, n_items + 3)       # (more words than the scene has items)
        dev, keep = device_snap(pm, r, case.xyr, mask=words)
        r.sync()
        mask = np_rect.item_flags(case.scene, [rect])[:, 0]
        w = words if isinstance(words, np.ndarray) else words.cpu().numpy().view(np.uint32)
        assert np.array_equal(w[:n_items], mask)
        want = np_snap.snap(case.scene, case.xyr, skip_items=mask)
        got = as_rec(dev)
        assert same(got, want), differing(got, want)[:8].tolist()
        found = got["item"][got["item"] != NONE]
        assert not mask[found].any()
        plain = case.expected()
        assert (mask == 0).all() == same(want, plain)
    assert (np_rect.item_flags(case.scene, [[90, 90, 260, 260]])[:, 0] != 0).sum() >= 3


def _tiger_queries(w, h, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (160, 2)) * (w, h)
    return np.concatenate([c, rng.choice([1.0, 4.0, 16.0], (160, 1))], axis=1).astype(np.float32)


@pytest.mark.gpu
def test_a_query_answers_for_the_scene_resident_at_the_call(pm):
    """The Tiger at 480 x 270: a device call on a caller's stream, followed at once by two re-flattens -- the answers are the first
    scene's; the host call afterwards answers for the last."""
    wl = pm.workloads.tiger(480, 270)
    xyr = _tiger_queries(wl.width, wl.height, 43)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene0 = r.download_scene()
        if _emulated():
            s = None
        else:
            import torch

            s = torch.cuda.Stream()
        dev, keep = device_snap(pm, r, xyr, stream=s)
        dev_e, keep_e = device_snap(pm, r, xyr, vertices=False, stream=s)
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        r.reflatten((0.9, 0.0, 0.0, 0.9, 40.0, 30.0), wl.width_scale)
        r.sync()
        if s is not None:
            s.synchronize()
        want = np_snap.snap(scene0, xyr)
        assert same(as_rec(dev), want) and same(as_rec(dev_e), np_snap.snap(scene0, xyr, vertices=False))
        assert len(set(want["item"].tolist())) > 20 and (want["item"] == NONE).any() and {V, E} <= set(want["kind"].tolist())
        scene2 = r.download_scene()
        got = r.snap(xyr[:, :2], xyr[:, 2])
        assert same(got, np_snap.snap(scene2, xyr)) and not same(got, want)


@pytest.mark.gpu
def test_queries_between_frames_leave_the_frames_alone(pm, pmo):
    """Frames rendered before and after snapping queries have the bytes they have without them."""
    wl = pm.workloads.tiger(480, 270)
    xyr = _tiger_queries(wl.width, wl.height, 44)[::4]
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        r.render()
        dev, keep = device_snap(pm, r, xyr)        # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        host = r.snap(xyr[:, :2], xyr[:, 2], vertices=False)
        second = r.read_pixels()
        assert np.array_equal(first, want_px) and np.array_equal(second, want_px)
        assert same(as_rec(dev), np_snap.snap(scene, xyr)) and same(host, np_snap.snap(scene, xyr, vertices=False))


@pytest.mark.gpu
def test_cli_snap(pm, tmp_path, capsys):
    """--snap prints what Renderer.snap returns, and the path the item came from."""
    from piet_metal_amd import cli

    pts = [(240.0, 135.0), (3.0, 3.0), (200.5, 100.5), (176.0, 60.0)]
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        of_item = r.item_paths()
        recs = {to: r.snap(np.array(pts, np.float32), 6.0, vertices=to != "edges", edges=to != "vertices") for to in ("both", "vertices", "edges")}
    for to, rec in recs.items():
        args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--snap-radius", "6"] + ([] if to == "both" else ["--snap-to", to])
        for x, y in pts:
            args += ["--snap", f"{x:g},{y:g}"]
        assert cli.main(args) == 0
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        want = []
        for (x, y), s in zip(pts, rec):
            head = f"{x:g},{y:g} r 6: "
            if s["item"] == NONE:
                want.append(head + "none")
                continue
            what = f"vertex {int(s['index'])}" if s["kind"] == V else f"edge {int(s['index'])} t {float(s['t']):.9g}"
            want.append(head + f"item {int(s['item'])} path {int(of_item[s['item']])} {what} at {float(s['x']):.9g},{float(s['y']):.9g} d2 {float(s['d2']):.17g}")
        assert lines == want
    assert (recs["both"]["item"] == NONE).any() and (recs["edges"]["kind"] == E).any() and (recs["both"]["kind"] == V).any()
    with pytest.raises(SystemExit):
        cli.main(["tiger", str(tmp_path / "t.png"), "--snap", "1,1"])       # no radius


# ---- CPU: the cases are what they claim (numpy alone) -------------------------------------------------------------------------

def test_the_cases_sizes_and_the_header_constants():
    assert sc.WAVE == 64 and sc.WALK_SIZES == (1, 63, 64, 65, 127, 128, 129, 200) and hs.CHUNK_SEGS == 4 and hs.SUPER_CHUNKS == 8
    assert sorted({c for c, _ in sc.LONG.values()}) == [64, 65, 512, 513]
    inc = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    for line in ("#define PM_SNAP_VERTICES 2u", "#define PM_SNAP_EDGES 4u", "#define PM_SNAP_KIND_VERTEX 1u", "#define PM_SNAP_KIND_EDGE 2u", "#define PM_ABI_VERSION 600"):
        assert line in inc, line


def test_hand_derived_answers_by_numpy(pm):
    scene = sc.ties_scene(pm)
    want = sc.known_records()
    for k, (q, (vertices, edges), skip, _) in enumerate(sc.KNOWN):
        for per_item in (False, True):
            got = np_snap.snap(scene, [q], vertices, edges, skip, per_item=per_item)
            assert same(got, want[k : k + 1]), (q, vertices, edges, skip, per_item, got, want[k])
    assert len(sc.KNOWN) >= 12


def _tie_classes(case, vertices, edges):
    """For a case's queries, by np_snap's pair functions alone: how many candidates (item, index) of the winning kind share the winner's
    d2 -- (in other items, in the winner's item), and whether the winner's d2 is exactly r * r."""
    sc_bytes = bytes(case.scene)
    want = case.expected(vertices, edges)
    offers = np_snap._offers(sc_bytes, False, None)
    Q = np_snap.Queries(case.xyr)
    other, own, exact = np.zeros(Q.n, np.int64), np.zeros(Q.n, np.int64), np.zeros(Q.n, bool)
    for q in np.flatnonzero(want["item"] != NONE):
        kind = want["kind"][q]
        for i, off in enumerate(offers):
            d2 = np_snap.vertex_d2(off[1], Q.x[q : q + 1], Q.y[q : q + 1])[0] if kind == V else np_snap.edge_d2(off[3], off[4], Q.x[q : q + 1], Q.y[q : q + 1])[0]
            ties = int((d2 == want["d2"][q]).sum())
            if i == want["item"][q]:
                own[q] = ties - 1
            else:
                other[q] += ties
        exact[q] = want["d2"][q] == Q.r2[q]
    return want, other, own, exact


def test_the_small_cases_have_every_class(pm):
    ties = sc.small_case(pm, "ties")
    for vertices, edges in ((True, False), (False, True)):
        want, other, own, exact = _tie_classes(ties, vertices, edges)
        # the same item twice (and a third time): the topmost wins; equal d2 within one item: the smallest index; d2 == r * r
        assert (other > 0).sum() >= 10 and (own > 0).sum() >= 10 and exact.sum() >= 10, (vertices, edges)
        assert (want["d2"][exact] > 0).sum() >= 5
    both, only_e = ties.expected(True, True), ties.expected(False, True)
    beaten = (both["kind"] == V) & (only_e["kind"] == E) & (only_e["d2"] < both["d2"])      # a vertex within r wins over a nearer edge
    assert beaten.sum() >= 20
    fallback = (both["kind"] == E) & (ties.expected(True, False)["item"] == NONE)
    assert fallback.sum() >= 5 and same(both[fallback], only_e[fallback])
    # one f32 step short of r: a query at exactly r and its twin with the radius one step below answer differently, for both kinds
    at = {tuple(q.tolist()): k for k, q in enumerate(ties.xyr)}
    for vertices, edges in ((True, False), (False, True)):
        want, _, _, exact = _tie_classes(ties, vertices, edges)
        twins = [(k, at.get((ties.xyr[k, 0], ties.xyr[k, 1], float(sc.down(ties.xyr[k, 2]))))) for k in np.flatnonzero(exact & (ties.xyr[:, 2] > 0))]
        assert sum(1 for k, j in twins if j is not None and want["d2"][j] != want["d2"][k]) >= 5, (vertices, edges)
    items = ties.expected()["item"]
    # every item that offers something is an answer: items 0 and 1 lie under their copy, item 7 -- item 1 answers once the transparent
    # item 7 is skipped, item 0 once skip_items takes out items 1 and 7
    assert set(range(12)) - {0, 1, 8} <= set(items.tolist()) and not {0, 1, 8} & set(items.tolist()) and NONE in items
    skip = ties.expected(True, True, True)
    assert 7 in items and 7 not in skip["item"] and 1 in skip["item"] and not same(skip, ties.expected())
    masked = ties.expected(True, True, False, True)
    assert ties.mask[1] and ties.mask[7] and 0 in masked["item"]
    assert not np.isin(masked["item"], np.flatnonzero(ties.mask)).any() and not same(masked, ties.expected())
    valid = np_snap.Queries(ties.xyr).valid
    assert (~valid).sum() >= 9 and (ties.expected()["item"][~valid] == NONE).all()
    zero_r = (ties.xyr[:, 2] == 0) & (items != NONE)
    assert zero_r.sum() >= 30 and (ties.expected()["d2"][zero_r] == 0).all()
    edge = sc.small_case(pm, "edge")
    boxes = np.array([b for _, b in np_hit.flat_items(bytes(edge.scene))])
    assert (boxes[:, :2] == 0).any() and (boxes[:, 2] == 65535).sum() >= 2      # the saturated edges are there
    ee = edge.expected()
    beyond, negative = (edge.xyr[:, 0] > 65535) & (ee["item"] != NONE), (edge.xyr[:, 0] < 0) & (ee["item"] != NONE)
    assert beyond.sum() >= 20 and negative.sum() >= 20 and {1, 3} <= set(ee["item"][beyond].tolist()) and {0, 2} <= set(ee["item"][negative].tolist())
    # ends at 1e30 beyond a saturated side: the answers of the first queries are points at x = 0 of items whose ShortBbox begins at
    # x0 >= 64 999 -- 64 800 and more outside the side the box bounds, with r = 200 --, and the same along y
    ab = sc.small_case(pm, "absorbed")
    ab_boxes = np.array([b for _, b in np_hit.flat_items(bytes(ab.scene))])
    at = {tuple(q.tolist()): k for k, q in enumerate(ab.xyr)}
    for vertices, edges in ((True, True), (False, True)):
        ea = ab.expected(vertices, edges)
        for q, item in (((100.0, 10.0, 200.0), 0), ((100.0, 30.0, 200.0), 1)):
            rec = ea[at[q]]
            assert (rec["item"], rec["kind"], rec["index"], rec["t"], rec["x"], rec["y"], rec["d2"]) == (item, E, 0, 1.0, 0.0, q[1], 10000.0), (q, rec)
            assert ab_boxes[item][0] >= 64999 and ab_boxes[item][2] == 65535 and 0 < ab_boxes[item][1] < ab_boxes[item][3] < 65535
        rec = ea[at[(420.0, 100.0, 150.0)]]
        assert (rec["item"], rec["kind"], rec["x"], rec["y"], rec["d2"]) == (2, E, 420.0, 0.0, 10000.0) and ab_boxes[2][1] >= 63999 and ab_boxes[2][3] == 65535
    assert {0, 1, 2, 3, 4} <= set(ab.expected()["item"].tolist())
    nf = sc.small_case(pm, "nonfinite")
    en = nf.expected()
    assert {0, 1, 2, 3, 4} <= set(en["item"].tolist())     # (item 4, the Polyline of width NaN, snaps: the width plays no part)
    for rec in (ee, en, ties.expected(), sc.small_case(pm, "mixed").expected()):
        assert np.isfinite(rec["d2"]).all() and np.isfinite(rec["x"]).all() and (rec["d2"] >= 0).all()
        none = rec["item"] == NONE
        assert not rec[none].view(np.uint8).reshape(-1, 32)[:, 4:].any()


@pytest.mark.parametrize("n", sc.WALK_SIZES)
def test_the_walk_cases_are_what_they_claim(pm, n):
    case = sc.walk_case(pm, n)
    want = case.expected()
    assert len(np_hit.flat_items(bytes(case.scene))) == n
    # every item is the answer of the query on its own spot with r = 0.5 or 3: the first, the last, and both ends of every step of 64
    near = set(want["item"][:n].tolist()) | set(want["item"][n : 2 * n].tolist())
    assert near >= set(range(n)), sorted(set(range(n)) - near)
    assert (want["item"][:n] == np.arange(n)).sum() >= (3 * n) // 5
    skip = case.expected(True, True, True)
    transparent = [i for i in range(n) if i % 3 == 0 and case.facts["kinds"][i] not in ("circle", "ellipse")]
    assert not np.isin(skip["item"], transparent).any() and (n < 4 or np.isin(want["item"], transparent).any())
    masked = case.expected(True, True, False, True)
    assert not np.isin(masked["item"], np.flatnonzero(case.mask)).any()
    assert want["item"][-1] == NONE and want["item"][-2] != NONE and want["item"][-4] == NONE


@pytest.mark.parametrize("ident", sc.LONG_IDS)
def test_the_long_cases_are_decided_where_they_claim(pm, ident):
    """With hit_structure's model of the index: winners lie in the first chunk, the last, the 64th / 65th and the one behind the 64th
    super-chunk; some winner's segment lies ON its chunk box's edge at distance exactly r from the query; some winner has an equal in
    another chunk of the item."""
    case = sc.long_case(pm, ident)
    chunks, item, cb0, cb1 = case.facts["chunks"], case.facts["long_item"], case.facts["cb0"], case.facts["cb1"]
    base, chunk_bbox, _ = hs.index_model(case.scene)
    assert cb1 - cb0 == chunks
    named = sc.named_chunks(cb0, cb1)
    if chunks >= 512 and (cb1 - 1) // hs.SUPER_CHUNKS - cb0 // hs.SUPER_CHUNKS + 1 > 64:
        assert any((cb0 + p) // hs.SUPER_CHUNKS - cb0 // hs.SUPER_CHUNKS == 64 for p in named)
    won = set()
    on_edge_at_r = 0
    tied_across_chunks = 0
    Q = np_snap.Queries(case.xyr)
    offers = np_snap._offers(bytes(case.scene), False, None)[item]
    for vertices, edges in ((True, False), (False, True)):
        want = case.expected(vertices, edges)
        mine = np.flatnonzero(want["item"] == item)
        chunk_of = np.minimum(want["index"] // hs.CHUNK_SEGS, chunks - 1)      # (a Polyline's last point belongs to its last segment's chunk)
        won |= set(chunk_of[mine].tolist())
        for q in mine:
            bb = chunk_bbox[cb0 + chunk_of[q]].astype(np.float64)
            ex = max(bb[0] - Q.x[q], 0.0, Q.x[q] - bb[2])
            ey = max(bb[1] - Q.y[q], 0.0, Q.y[q] - bb[3])
            if want["d2"][q] == Q.r2[q] and ex * ex + ey * ey == Q.r2[q] and Q.r2[q] > 0:
                on_edge_at_r += 1
            if edges:
                d2 = np_snap.edge_d2(offers[3], offers[4], Q.x[q : q + 1], Q.y[q : q + 1])[0]
                equal = offers[2][d2 == want["d2"][q]] // hs.CHUNK_SEGS
                tied_across_chunks += len(set(equal.tolist())) > 1
    # (the last chunk of loops-65 and loops-513 is the closing segment alone, which lies ON every earlier return stroke: it ties with them
    # wherever it is nearest, and the smaller index -- another chunk's -- wins)
    lone_closing = ident in ("loops-65", "loops-513")
    assert 0 in won and (chunks - 1 in won) != lone_closing and len(won & set(named)) >= len(named) - 1, (sorted(won & set(named)), named)
    assert on_edge_at_r >= 1 and tied_across_chunks >= 1, (on_edge_at_r, tied_across_chunks)
    assert len(won) >= 8


# ---- CPU: D21 is D13's distance (np_snap against np_hit, no kernel) ---------------------------------------------------------------

def test_edge_snap_at_half_the_width_is_d13(pm):
    """On the Polylines and Lines of 40 seeded edge scenes (tests/edge_scenes.py), over grids of points and the strokes' own points: "edge
    snap with r = hw, restricted to the item, finds something" EQUALS np_hit.item_inside -- the same d2 against the same hw * hw.  Zero
    disagreements."""
    import struct

    import edge_scenes as es

    checked = inside_n = items_n = 0
    for seed in es.SMALL_SEEDS[:40]:
        scene, w, h, _ = es.edge_scene(pm, seed, small=True, n=24)
        sb = bytes(scene)
        items = np_hit.flat_items(sb)
        grid = (np.mgrid[-8 : w + 9 : 2, -8 : h + 9 : 2].reshape(2, -1).T + 0.25 * (seed % 4)).astype(np.float32)
        for i, (at, _) in enumerate(items):
            tag = struct.unpack_from("<I", sb, at)[0] & 0xFFFF
            if tag not in (np_hit.LINE, np_hit.POLY):
                continue
            (width,) = struct.unpack_from("<f", sb, at + (12 if tag == np_hit.LINE else 8))
            hw = np.float32(0.5) * np.float32(width)         # (halving is exact)
            a, b, hw64 = np_hit.stroke_segments(sb, at, tag)
            assert not np.isnan(hw) and np.float64(hw) == hw64
            own = np.concatenate([a, b, (a + b) * 0.5, a + (hw64, 0.0), b - (0.0, hw64)]).astype(np.float32)
            g = np.concatenate([grid, own[np.isfinite(own).all(axis=1)]])
            mask = np.ones(len(items), np.uint32)
            mask[i] = 0
            xyr = np.concatenate([g, np.full((len(g), 1), hw, np.float32)], axis=1)
            found = np_snap.snap(scene, xyr, vertices=False, skip_items=mask)["item"] != NONE
            inside = np_hit.item_inside(scene, i, g, brute=True)
            assert np.array_equal(found, inside), (seed, i, np.flatnonzero(found != inside)[:8].tolist())
            checked += len(g)
            inside_n += int(inside.sum())
            items_n += 1
    print(f"{items_n} strokes, {checked} (stroke, point) pairs, {inside_n} inside")
    assert items_n >= 150 and inside_n >= 1000 and inside_n < checked // 2     # (floors against a blind test, far below what the seeds give)


# ---- CPU: np_snap's two evaluation orders ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.SMALL)
def test_evaluation_orders_agree(pm, name):
    case = sc.small_case(pm, name)
    for vertices, edges in sc.FLAG_SETS:
        for skip, masked in ((False, False), (True, True)):
            a = case.expected(vertices, edges, skip, masked)
            b = np_snap.snap(case.scene, case.xyr, vertices, edges, skip, case.mask if masked else None, per_item=True)
            assert same(a, b), (name, vertices, edges, skip, masked, differing(a, b)[:8].tolist())
    walk = sc.walk_case(pm, 129)
    assert same(walk.expected(), np_snap.snap(walk.scene, walk.xyr, per_item=True))
    long = sc.long_case(pm, "comb-65")
    assert same(long.expected(), np_snap.snap(long.scene, long.xyr, per_item=True))


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_snap_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- CPU: the compiler's listing ------------------------------------------------------------------------------------------------

def test_the_snap_kernel_uses_no_scratch(tmp_path):
    """pm_snap_kernel by the flags the library is built with: no private segment (nothing spilled, no indexed local array), no LDS, and
    VGPRs within 128 -- a workgroup of four waves puts one on each SIMD of a CU, which has 512 VGPRs per lane: four such workgroups per
    CU.  The figures are printed (pytest -s) and stand in DESIGN.md 4.  Sizes only: the assembly is searched for no instruction."""
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
        if "pm_snap_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"pm_snap_kernel: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and lds == 0, (m.group(1), scratch, vgpr, lds)
    assert found == 1
    assert "pm_hit_poly.h" in mk and "pm_snap.h" in mk     # (editing either header rebuilds the library)
