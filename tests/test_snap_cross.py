"""Snapping to intersections, pm_snap_intersections / pm_snap_intersections_device (decision D23): the nearest crossing of two edges
to a cursor -- which two edges, where on each, where, how far, and how many edges were near.

The bar everywhere: the 48-byte records EQUAL to tests/np_cross.py as bytes, the bits of d2 included, no query left out -- through the
host and the device call, with and without PM_HIT_SKIP_TRANSPARENT, with and without skip_items.  tests/cross_cases.py builds the
scenes and places the queries.

-m gpu: small scenes with ties, the item walk, long items, the limit of 512 near edges, the hand-derived answers, output discipline and
the grid, the argument rules, composition with pm_select_rect_device, ordering against scene replacement and frames, the CLI.
CPU: the cases are what they claim (numpy alone); the hand-derived answers; np_cross's two evaluation orders; D23 against exact rational
arithmetic; the near rule drops nothing decisive; the relation to D21; the -m gpu part against the wave64 emulation of the kernel; the
compiler's listing; the header's constants."""
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
import cross_cases as cc  # noqa: E402
import hit_structure as hs  # noqa: E402
import np_cross  # noqa: E402
import np_snap  # noqa: E402
import snap_cases as sc  # noqa: E402

NONE = cc.NONE
X, MANY = np_cross.INTERSECTION, np_cross.TOO_MANY
REC = np_cross.RECORD
UNTOUCHED = 0x7EADBEEF
# small scenes, walk, long, the limit, known answers, output discipline, argument rules, composition, ordering (2), CLI
N_GPU_TESTS = len(cc.SMALL) + len(cc.WALK_SIZES) + len(cc.LONG_IDS) + 1 + 1 + 1 + 1 + 1 + 2 + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def device_cross(pm, r, xyr, skip=False, mask=None, pad=0, stream=None):
    """pm_snap_intersections_device into n + pad records filled with UNTOUCHED, not waited for: (records as int32 [n + pad, 12],
    keep-alive).  Under the emulation device memory is host memory and the arrays are numpy's; on the GPU they are torch's.  mask: None, a
    numpy array of words (copied to the device) or device words as they are."""
    xyr = np.ascontiguousarray(xyr, np.float32).reshape(-1, 3)
    n = len(xyr)
    if _emulated():
        out = np.full((n + pad, 12), UNTOUCHED, np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint32)
        pm._lib.check(pm._lib.load().pm_snap_intersections_device(r._h, xyr.ctypes.data, n, pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0,
                                                                  m.ctypes.data if m is not None else None, m.size if m is not None else 0, out.ctypes.data, None),
                      "pm_snap_intersections_device")
        return out, (xyr, m)
    import torch

    dq = torch.from_numpy(xyr).cuda()
    out = torch.full((n + pad, 12), UNTOUCHED, dtype=torch.int32, device="cuda")
    m = None if mask is None else (torch.from_numpy(np.ascontiguousarray(mask, np.uint32).view(np.int32)).cuda() if isinstance(mask, np.ndarray) else mask)
    r.snap_intersections_tensor(dq, out[:n], skip_items=m, stream=stream, skip_transparent=skip)
    return out, (dq, m)


def as_rec(a, n=None):
    """RECORD [n] of an int32 [., 12] array of either kind."""
    a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    a = np.ascontiguousarray(a[:n] if n is not None else a)
    return a.view(REC).reshape(-1)


def same(got, want):
    return got.tobytes() == want.tobytes()


def differing(got, want):
    return np.flatnonzero((np.ascontiguousarray(got).view(np.uint8).reshape(-1, 48) != np.ascontiguousarray(want).view(np.uint8).reshape(-1, 48)).any(axis=1))


def check_case(pm, r, case, skips=(False, True), masks=(False, True)):
    """Host and device, with and without the flag and the mask: equal to np_cross."""
    for skip in skips:
        for masked in masks:
            want = case.expected(skip, masked)
            mask = case.mask if masked else None
            dev, keep = device_cross(pm, r, case.xyr, skip, mask)
            got = r.snap_intersections(case.xyr[:, :2], case.xyr[:, 2], skip, mask)      # (synchronises the context's stream: the device call is done)
            bad = differing(got, want)
            assert bad.size == 0, (case, skip, masked, len(bad), [(case.xyr[k].tolist(), got[k], want[k]) for k in bad[:6]])
            d = as_rec(dev)
            bad = differing(d, want)
            assert bad.size == 0, (case, "device", skip, masked, len(bad), [(case.xyr[k].tolist(), d[k], want[k]) for k in bad[:6]])


@pytest.fixture(scope="module")
def cross_renderer(pm):
    """Never resized: snapping needs a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.SMALL)
def test_small_scenes(pm, cross_renderer, name):
    """The ties scene, mixed_scene, edge_scene, the scene of non-finite points and the one of ends at 1e30, under a few hundred queries: on a
    crossing with r = 0, at exactly r, one f32 step short of it, not a query at all."""
    case = cc.small_case(pm, name)
    cross_renderer.set_scene_bytes(case.scene)
    check_case(pm, cross_renderer, case)


@pytest.mark.gpu
@pytest.mark.parametrize("n", cc.WALK_SIZES)
def test_item_walk_by_item_count(pm, cross_renderer, n):
    """One item, one fewer than a step of the walk, a step, one more, two steps and their neighbours, 200: every item crosses the first and
    the last item, which cross each other."""
    case = cc.walk_case(pm, n)
    cross_renderer.set_scene_bytes(case.scene)
    assert cross_renderer.stats()["n_items"] == n
    check_case(pm, cross_renderer, case)


@pytest.mark.gpu
@pytest.mark.parametrize("ident", cc.LONG_IDS)
def test_long_items(pm, cross_renderer, ident):
    """A Fill, a compound Fill and a Polyline of 64, 65, 512 and 513 chunks exactly, crossed by Lines in the first chunk, the last, the one
    behind the 64th super-chunk; the near edge on a chunk box's edge at exactly r."""
    case = cc.long_case(pm, ident)
    cross_renderer.set_scene_bytes(case.scene)
    check_case(pm, cross_renderer, case, skips=(False,))


@pytest.mark.gpu
def test_the_limit_of_near_edges(pm, cross_renderer):
    """511 and 512 near edges: the crossing of the last two edges stored.  513: PM_SNAP_KIND_TOO_MANY with n_near == 513, and the crossing
    again once r is smaller."""
    for n_near in cc.LIMIT_NEAR:
        case = cc.limit_case(pm, n_near)
        cross_renderer.set_scene_bytes(case.scene)
        check_case(pm, cross_renderer, case, skips=(False,))
        got = cross_renderer.snap_intersections(case.xyr[:2, :2], case.xyr[:2, 2])
        assert got["n_near"].tolist() == [n_near, 2] and got["item"][1] == 1 and got["item2"][1] == 0
        if n_near <= cc.MAX_NEAR:
            assert (got["item"][0], got["kind"][0], got["item2"][0], got["x"][0], got["y"][0], got["d2"][0]) == (1, X, 0, 20.0, 10.0, 25.0)
        else:
            assert (got["item"][0], got["kind"][0]) == (NONE, MANY)


@pytest.mark.gpu
def test_hand_derived_answers(pm, cross_renderer):
    """cross_cases.KNOWN, worked out in its comments."""
    r = cross_renderer
    r.set_scene_bytes(cc.ties_scene(pm))
    want = cc.known_records()
    for k, (q, skip, _, _) in enumerate(cc.KNOWN):
        mask = cc.known_mask() if skip == "mask" else None
        skip = skip is True
        got = r.snap_intersections(np.array([q[:2]], np.float32), q[2], skip, mask)
        assert same(got, want[k : k + 1]), (q, skip, got, want[k])
        dev, keep = device_cross(pm, r, [q], skip, mask)
        r.sync()
        assert same(as_rec(dev), want[k : k + 1]), (q, skip, as_rec(dev), want[k])


@pytest.mark.gpu
def test_output_discipline_and_the_grid(pm, cross_renderer):
    """1 ... 7 queries and one query either side of what pm_snap_kernel's grid rule holds at once (32 per CU) into arrays four records too
    long: the records beyond n stay as they were -- a short list repeated, so that a stride error is a wrong VALUE.  n == 0 writes
    nothing."""
    case = cc.small_case(pm, "ties")
    r = cross_renderer
    r.set_scene_bytes(case.scene)
    short = np.array([q for q, skip, _, _ in cc.KNOWN if skip is False][:9], np.float32)
    want = np_cross.cross(case.scene, short)
    assert len(set(want["item"].tolist())) >= 5 and NONE in want["item"] and len(set(want["n_near"].tolist())) >= 3
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
        dev, keep = device_cross(pm, r, q, pad=4)
        host = np.full((n + 4, 12), UNTOUCHED, np.int32)
        assert lib.pm_snap_intersections(r._h, q.ctypes.data, n, 0, None, 0, host.ctypes.data) == pm._lib.PM_OK
        r.sync()
        for got in (host, dev if isinstance(dev, np.ndarray) else dev.cpu().numpy()):
            assert same(as_rec(got, n), w), (n, differing(as_rec(got, n), w)[:8].tolist())
            assert (got[n:] == UNTOUCHED).all(), n
    host = np.full((4, 12), UNTOUCHED, np.int32)
    dev, keep = device_cross(pm, r, np.zeros((0, 3), np.float32), pad=4)
    assert lib.pm_snap_intersections(r._h, short.ctypes.data, 0, 0, None, 0, host.ctypes.data) == pm._lib.PM_OK
    assert lib.pm_snap_intersections(r._h, None, 0, 0, None, 0, None) == pm._lib.PM_OK
    r.sync()
    assert (host == UNTOUCHED).all() and (as_rec(dev).view(np.int32) == UNTOUCHED).all()
    assert REC.itemsize == 48 and pm.renderer.SNAP_CROSS_DTYPE == REC


@pytest.mark.gpu
def test_argument_rules(pm, pmo):
    lib = pm._lib.load()
    L = pm._lib
    OK, INVALID = L.PM_OK, L.PM_ERR_INVALID
    with pm.Renderer(0) as r:
        out = np.full((4, 12), UNTOUCHED, np.int32)
        q = np.array([[50, 50, 10]] * 4, np.float32)
        words = np.zeros(16, np.uint32)
        qp, op, wp = q.ctypes.data, out.ctypes.data, words.ctypes.data
        calls = [lambda *a: lib.pm_snap_intersections(r._h, *a), lambda *a: lib.pm_snap_intersections_device(r._h, *a, None)]      # (xyr, n, flags, skip_items, n_skip, out)
        for call in calls:
            assert call(qp, 4, 0, None, 0, op) == INVALID                      # no scene: what pm_hit_test says
        r.set_scene_bytes(pmo.scene_path_test())
        assert r.stats()["n_items"] == 1
        for call in calls:
            for bit in (L.PM_SNAP_VERTICES, L.PM_SNAP_EDGES, 8, 0x80000000):
                assert call(qp, 4, bit, None, 0, op) == INVALID                # the only flag is PM_HIT_SKIP_TRANSPARENT
                assert call(qp, 4, bit | L.PM_HIT_SKIP_TRANSPARENT, None, 0, op) == INVALID
            assert call(None, 4, 0, None, 0, op) == INVALID                    # a NULL pointer with n > 0
            assert call(qp, 4, 0, None, 0, None) == INVALID
            assert call(qp, 4, 0, wp, 0, op) == INVALID                        # skip_items shorter than the scene
            assert call(qp, 4, 0, None, 1, op) == INVALID                      # no skip_items, but a count
            assert call(qp, 0, 0, wp, 0, op) == INVALID                        # ... also with nothing to do
            assert call(qp, 0, 8, None, 0, op) == INVALID
            assert call(None, 0, 0, None, 0, None) == OK                       # nothing to do
            assert call(qp, 0, L.PM_HIT_SKIP_TRANSPARENT, wp, 16, op) == OK
        r.sync()
        assert (out == UNTOUCHED).all()
        # more words than items: fine.  (Only the host call may be given these arrays to work on: they are host memory)
        assert calls[0](qp, 3, L.PM_HIT_SKIP_TRANSPARENT, wp, 16, op) == OK
        assert (out[3] == UNTOUCHED).all() and (out[:3] != UNTOUCHED).any(axis=1).all()
        dev, keep = device_cross(pm, r, q[:3], skip=True, mask=words, pad=1)
        r.sync()
        assert same(as_rec(dev, 3), out[:3].view(REC).reshape(-1)) and (as_rec(dev)[3:].view(np.int32) == UNTOUCHED).all()
        assert lib.pm_abi_version() == 600
        assert (L.PM_SNAP_KIND_INTERSECTION, L.PM_SNAP_KIND_TOO_MANY, L.PM_SNAP_MAX_NEAR_EDGES) == (3, 4, 512)
        # the Python wrappers
        with pytest.raises(ValueError):
            r.snap_intersections(np.zeros((3, 3), np.float32), 1.0)
        with pytest.raises(ValueError):
            r.snap_intersections(np.zeros((3, 2), np.float32), [1.0, 2.0])
        with pytest.raises(ValueError):
            r.snap_intersections(np.zeros((3, 2), np.float32), 1.0, skip_items=np.zeros((2, 2)))
        got = r.snap_intersections(np.zeros((0, 2), np.float32), 1.0)
        assert got.shape == (0,) and got.dtype == REC
        assert r.snap_intersections(np.zeros((2, 2), np.float32), [1.0, 2.0]).shape == (2,)
        if not _emulated():
            import torch

            o = torch.zeros((4, 12), dtype=torch.int32, device="cuda")
            x = torch.zeros((4, 3), device="cuda")
            with pytest.raises(TypeError):
                r.snap_intersections_tensor(torch.zeros((4, 3)), o)                                  # not on the device
            with pytest.raises(TypeError):
                r.snap_intersections_tensor(torch.zeros((4, 2), device="cuda"), o)                   # points without radii
            with pytest.raises(TypeError):
                r.snap_intersections_tensor(x, o[:3])
            with pytest.raises(TypeError):
                r.snap_intersections_tensor(x, torch.zeros((4, 8), dtype=torch.int32, device="cuda"))  # pm_snap's record
            with pytest.raises(TypeError):
                r.snap_intersections_tensor(x, torch.zeros((4, 12), device="cuda"))                  # floating point
            with pytest.raises(TypeError):
                r.snap_intersections_tensor(x, o, skip_items=torch.zeros(4, device="cuda"))
            r.snap_intersections_tensor(x, o, skip_items=torch.zeros(1, dtype=torch.int32, device="cuda"))
            r.sync()


@pytest.mark.gpu
def test_selection_words_are_skip_items_without_a_read_back(pm, cross_renderer):
    """pm_select_rect_device's words go into pm_snap_intersections_device as they were written, on the same stream: an edge of what the
    marquee touched is never part of the answer, and the records are np_cross's under the same mask."""
    import np_rect

    r = cross_renderer

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

    case = cc.small_case(pm, "ties")
    r.set_scene_bytes(case.scene)
    n_items = len(case.mask)
    plain = case.expected()
    for rect in ([3, -1, 5, 9], [-20, -20, 600, 600], [1000, 1000, 1010, 1010]):
        words = device_select(rect, n_items + 3)       # (more words than the scene has items)
        dev, keep = device_cross(pm, r, case.xyr, mask=words)
        r.sync()
        mask = np_rect.item_flags(case.scene, [rect])[:, 0]
        w = words if isinstance(words, np.ndarray) else words.cpu().numpy().view(np.uint32)
        assert np.array_equal(w[:n_items], mask)
        want = np_cross.cross(case.scene, case.xyr, skip_items=mask)
        got = as_rec(dev)
        assert same(got, want), differing(got, want)[:8].tolist()
        found = got["item"] != NONE
        assert not mask[got["item"][found]].any() and not mask[got["item2"][found]].any()
        assert (mask == 0).all() == same(want, plain)
    touched = np_rect.item_flags(case.scene, [[3, -1, 5, 9]])[:, 0] != 0
    assert np.flatnonzero(touched).tolist() == [0, 1, 2, 15]       # (the Line x = 4 lies in the marquee; the other Lines through (4, 4) touch it)


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
        dev, keep = device_cross(pm, r, xyr, stream=s)
        dev_s, keep_s = device_cross(pm, r, xyr, skip=True, stream=s)
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        r.reflatten((0.9, 0.0, 0.0, 0.9, 40.0, 30.0), wl.width_scale)
        r.sync()
        if s is not None:
            s.synchronize()
        want = np_cross.cross(scene0, xyr)
        assert same(as_rec(dev), want) and same(as_rec(dev_s), np_cross.cross(scene0, xyr, True))
        assert len(set(want["item"].tolist())) > 10 and (want["item"] == NONE).any() and (want["kind"] == X).sum() > 20
        scene2 = r.download_scene()
        got = r.snap_intersections(xyr[:, :2], xyr[:, 2])
        assert same(got, np_cross.cross(scene2, xyr)) and not same(got, want)


@pytest.mark.gpu
def test_queries_between_frames_leave_the_frames_alone(pm, pmo):
    """Frames rendered before and after intersection queries have the bytes they have without them."""
    wl = pm.workloads.tiger(480, 270)
    xyr = _tiger_queries(wl.width, wl.height, 44)[::4]
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        r.render()
        dev, keep = device_cross(pm, r, xyr)        # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        host = r.snap_intersections(xyr[:, :2], xyr[:, 2], skip_transparent=True)
        second = r.read_pixels()
        assert np.array_equal(first, want_px) and np.array_equal(second, want_px)
        assert same(as_rec(dev), np_cross.cross(scene, xyr)) and same(host, np_cross.cross(scene, xyr, True))


@pytest.mark.gpu
def test_cli_snap_to_intersections(pm, tmp_path, capsys):
    """--snap-to intersections prints what Renderer.snap_intersections returns, and the paths the two items came from."""
    from piet_metal_amd import cli

    pts = [(240.0, 135.0), (3.0, 3.0), (200.5, 100.5), (176.0, 60.0), (230.0, 120.0)]
    wl = pm.workloads.tiger(480, 270)
    lines = {}
    recs = {}
    for radius in (6.0, 60.0):
        with pm.Renderer(0) as r:
            r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            of_item = r.item_paths()
            recs[radius] = r.snap_intersections(np.array(pts, np.float32), radius)
        args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--snap-radius", f"{radius:g}", "--snap-to", "intersections"]
        for x, y in pts:
            args += ["--snap", f"{x:g},{y:g}"]
        assert cli.main(args) == 0
        lines[radius] = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        want = []
        for (x, y), s in zip(pts, recs[radius]):
            head = f"{x:g},{y:g} r {radius:g}: "
            if s["kind"] == MANY:
                want.append(head + f"more than 512 edges within the radius ({int(s['n_near'])}): ask again with a smaller one")
            elif s["item"] == NONE:
                want.append(head + "none")
            else:
                want.append(head + f"item {int(s['item'])} path {int(of_item[s['item']])} edge {int(s['index'])} t {float(s['t']):.9g} crosses "
                            f"item {int(s['item2'])} path {int(of_item[s['item2']])} edge {int(s['index2'])} u {float(s['u']):.9g} "
                            f"at {float(s['x']):.9g},{float(s['y']):.9g} d2 {float(s['d2']):.17g}")
        assert lines[radius] == want
    assert (recs[6.0]["kind"] == X).any() and (recs[6.0]["item"] == NONE).any() and (recs[60.0]["kind"] == MANY).any()


# ---- CPU: the cases are what they claim (numpy alone) -------------------------------------------------------------------------

def test_the_header_constants_and_the_record():
    assert cc.WAVE == 64 and cc.WALK_SIZES == hs.WALK_SIZES == (1, 63, 64, 65, 127, 128, 129, 200) and cc.MAX_NEAR == 512
    assert sorted({v[0] for v in cc.LONG.values()}) == [64, 65, 512, 513] and {v[1] for v in cc.LONG.values()} == {"fill", "compound", "polyline"}
    inc = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    for line in ("#define PM_SNAP_KIND_INTERSECTION 3u", "#define PM_SNAP_KIND_TOO_MANY 4u", "#define PM_SNAP_MAX_NEAR_EDGES 512u", "#define PM_ABI_VERSION 600",
                 "typedef struct { uint32_t item, kind, index; float t; float x, y; double d2; uint32_t item2, index2; float u; uint32_t n_near; } pm_snap_cross_result;",
                 "int pm_snap_intersections(pm_ctx *c, const float *xyr", "int pm_snap_intersections_device(pm_ctx *c, const void *dev_xyr"):
        assert line in inc, line
    # the record as the dtype has it: pm_snap_result's 32 bytes, then item2, index2, u, n_near
    assert REC.itemsize == 48 and {k: REC.fields[k][1] for k in REC.names} == {"item": 0, "kind": 4, "index": 8, "t": 12, "x": 16, "y": 20, "d2": 24, "item2": 32,
                                                                               "index2": 36, "u": 40, "n_near": 44}
    assert REC.descr[:7] == np_snap.RECORD.descr
    ctx = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    for field, at in (("item2", 32), ("index2", 36), ("u", 40), ("n_near", 44)):
        assert f"offsetof(pm_snap_cross_result, {field}) == {at}" in ctx
    assert "sizeof(pm_snap_cross_result) == 48" in ctx
    sys.path.insert(0, ROOT)
    from piet_metal_amd import _lib

    assert {"pm_snap_intersections", "pm_snap_intersections_device"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["pm_snap_intersections"][1]) == 7 and len(_lib.SIGNATURES["pm_snap_intersections_device"][1]) == 8
    assert (_lib.PM_SNAP_KIND_INTERSECTION, _lib.PM_SNAP_KIND_TOO_MANY, _lib.PM_SNAP_MAX_NEAR_EDGES) == (X, MANY, cc.MAX_NEAR)


def test_hand_derived_answers_by_numpy(pm):
    scene = cc.ties_scene(pm)
    want = cc.known_records()
    for k, (q, skip, _, _) in enumerate(cc.KNOWN):
        mask = cc.known_mask() if skip == "mask" else None
        for per_first in (False, True):
            got = np_cross.cross(scene, [q], skip is True, mask, per_first=per_first)
            assert same(got, want[k : k + 1]), (q, skip, per_first, got, want[k])
    assert len(cc.KNOWN) >= 12
    # the issue's own example
    q, skip, rec, n_near = cc.KNOWN[2]
    assert q == (5, 4, 2) and rec[:7] == (1, X, 0, 0.5, 4.0, 4.0, 1.0) and rec[7:] == (0, 0, 0.5)


def _pair_classes(case, skip=False):
    """For a case's queries, by np_cross's pair functions alone: (how many qualifying pairs share the winner's d2, is the winner's d2
    exactly r * r, does the winning pair lie in one item, is t or u exactly 0 or 1)."""
    want = case.expected(skip)
    E = np_cross.Edges(bytes(case.scene), skip)
    Q = np_snap.Queries(case.xyr)
    near = np_cross.near_mask(E, Q)
    ties, exact, own, contact = np.zeros(Q.n, np.int64), np.zeros(Q.n, bool), np.zeros(Q.n, bool), np.zeros(Q.n, bool)
    for q in np.flatnonzero(want["kind"] == X):
        ix = np.flatnonzero(near[q])
        i, j = np.triu_indices(len(ix), 1)
        ok, p = np_cross.qualifies(E.a[ix[i]], E.b[ix[i]], E.a[ix[j]], E.b[ix[j]], Q.x[q], Q.y[q], Q.r2[q])
        ties[q] = int((ok & (p[6] == want["d2"][q])).sum())
        exact[q] = want["d2"][q] == Q.r2[q]
        own[q] = want["item"][q] == want["item2"][q]
        contact[q] = want["t"][q] in (0.0, 1.0) or want["u"][q] in (0.0, 1.0)
    return want, ties, exact, own, contact


def test_the_small_cases_have_every_class(pm):
    ties = cc.small_case(pm, "ties")
    want, n_ties, exact, own, contact = _pair_classes(ties)
    found = want["kind"] == X
    # four Lines through one point, one of them transparent: six pairs of one d2, and three under PM_HIT_SKIP_TRANSPARENT; the same crossing
    # in two items: two; a pair within one item; a T-junction
    assert (n_ties == 6).sum() >= 5 and (_pair_classes(ties, True)[1] == 3).sum() >= 5 and (n_ties == 2).sum() >= 5 and own.sum() >= 10 and contact.sum() >= 5
    assert exact.sum() >= 10 and (want["d2"][exact] > 0).sum() >= 5
    # one f32 step short of r: a query at exactly r and its twin with the radius one step below answer differently
    at = {tuple(q.tolist()): k for k, q in enumerate(ties.xyr)}
    twins = [(k, at.get((ties.xyr[k, 0], ties.xyr[k, 1], float(cc.down(ties.xyr[k, 2]))))) for k in np.flatnonzero(exact & (ties.xyr[:, 2] > 0))]
    assert sum(1 for k, j in twins if j is not None and want["d2"][j] != want["d2"][k]) >= 5
    zero_r = (ties.xyr[:, 2] == 0) & found
    assert zero_r.sum() >= 10 and (want["d2"][zero_r] == 0).all()
    # edges sharing an end, parallel and collinear ones, a degenerate one: near, and no pair
    none_but_near = (want["item"] == NONE) & (want["n_near"] >= 2) & (want["kind"] == 0)
    assert none_but_near.sum() >= 10
    E = np_cross.Edges(bytes(ties.scene))
    i, j = np.triu_indices(E.n, 1)
    shared, den, t, u, _, _, _ = np_cross.pair_parts(E.a[i], E.b[i], E.a[j], E.b[j], 0.0, 0.0)
    assert shared.sum() >= 10 and (~shared & (den == 0)).sum() >= 20 and (E.a == E.b).all(axis=1).sum() == 1
    # the transparent item 15 and the skip_items mask change answers; nothing names an item that was taken out
    skip, masked = ties.expected(True), ties.expected(False, True)
    assert 15 in want["item"] and 15 not in skip["item"] and 15 not in skip["item2"] and not same(skip, want)
    out = np.flatnonzero(ties.mask)
    assert not np.isin(masked["item"], out).any() and not np.isin(masked["item2"][masked["kind"] == X], out).any() and not same(masked, want)
    # the first edge precedes the second; the items that cross something are answers
    assert ((want["item"][found] > want["item2"][found]) | ((want["item"][found] == want["item2"][found]) & (want["index"][found] < want["index2"][found]))).all()
    assert {5, 6, 8, 15, 17, 19} <= set(want["item"].tolist()) and 2 in skip["item"] and 1 in skip["item2"] and {2, 3, 6, 7, 16, 19} <= set(want["item2"][found].tolist())
    valid = np_snap.Queries(ties.xyr).valid
    assert (~valid).sum() >= 9 and not want[~valid].view(np.uint8).reshape(-1, 48)[:, 4:].any() and (want["item"][~valid] == NONE).all()
    for name in cc.SMALL:
        rec = cc.small_case(pm, name).expected()
        got = rec["kind"] == X
        assert np.isfinite(rec["d2"]).all() and np.isfinite(rec["x"]).all() and (rec["d2"] >= 0).all() and (rec["kind"] != MANY).all()
        none = rec["item"] == NONE
        assert not rec[none].view(np.uint8).reshape(-1, 48)[:, 4:44].any() and (rec["n_near"][got] >= 2).all()
        print(f"{name}: {int(got.sum())} of {len(rec)} queries answer an intersection")
        # (floors against a blind test; the scenes of non-finite points and of ends at 1e30 are there for their near counts)
        assert got.sum() >= {"ties": 40, "mixed": 40, "edge": 10}.get(name, 0) and (rec["n_near"] >= 2).sum() >= 10, (name, int(got.sum()))


@pytest.mark.parametrize("n", cc.WALK_SIZES)
def test_the_walk_cases_are_what_they_claim(pm, n):
    case = cc.walk_case(pm, n)
    want = case.expected()
    kinds = case.facts["kinds"]
    assert len(np_snap._offers(bytes(case.scene), False, None)) == n
    found = want["kind"] == X
    if n == 1:
        assert not found.any() and want["n_near"].max() == 1
        return
    # every item with edges is part of the answer at its own spot, crossing a rail (or, a compound Fill, itself): left of the rails' own
    # crossing the top rail is the nearer one, right of it the bottom rail
    partners = set()
    for i in range(1, n - 1):
        pair = {int(want["item"][i]), int(want["item2"][i])}
        if kinds[i] != "circle":
            assert found[i] and i in pair and pair <= {0, i, n - 1}, (i, want[i])
            partners |= pair - {i}
        else:
            assert not found[i] or i not in pair
    assert partners == {0, n - 1}
    # the rails' own crossing: the last item and the first, a step boundary or three apart
    k = 3 * n
    assert (want["item"][k], want["item2"][k], want["d2"][k]) == (n - 1, 0, 0.0) and want["n_near"][k] >= 2
    skip = case.expected(True)
    transparent = [i for i in range(1, n - 1) if i % 3 == 1 and kinds[i] != "circle"]
    assert not np.isin(skip["item2"][skip["kind"] == X], transparent).any() and (n < 6 or np.isin(want["item2"][found], transparent).any())
    masked = case.expected(False, True)
    assert not np.isin(masked["item2"][masked["kind"] == X], np.flatnonzero(case.mask)).any()
    assert want["item"][-1] == NONE and want["item"][-4] == NONE and want["n_near"][-4] == 0 and want["n_near"][-2] == want["n_near"].max() >= min(n, 3)


@pytest.mark.parametrize("ident", cc.LONG_IDS)
def test_the_long_cases_are_decided_where_they_claim(pm, ident):
    """With hit_structure's model of the index: the crossings are won by the long item's edges in exactly the chunks the case names -- its
    first, its last, those either side of its 64th and, where it has more than 64 super-chunks, the first behind the 64th (the lone
    closing chunk of cross_cases.LONE_CLOSING excepted, as said there); and for every case some winner's segment lies ON its chunk box's
    edge with the edge, the segment and the crossing at exactly r from the query, and no answer one f32 step short of r."""
    case = cc.long_case(pm, ident)
    chunks, cb0, cb1, segs, mids = case.facts["chunks"], case.facts["cb0"], case.facts["cb1"], case.facts["segments"], case.facts["mids"]
    base, chunk_bbox, _ = hs.index_model(case.scene)
    assert int(base[cc.LONG_ITEM + 1]) - int(base[cc.LONG_ITEM]) == chunks and int(base[cc.LONG_ITEM]) == cb0
    want = case.expected()
    Q = np_snap.Queries(case.xyr)
    won, on_edge_at_r = [], 0
    for m, (mid, seg) in enumerate(zip(mids, segs)):
        q = 7 * m                     # the query on M with r = 0
        assert (want["kind"][q], want["item"][q], want["item2"][q], want["index2"][q], want["d2"][q]) == (X, 3 + m, cc.LONG_ITEM, seg, 0.0), (ident, m, want[q])
        won.append(seg // hs.CHUNK_SEGS)
        q = 7 * m + 4                 # 1/8 beside M with r = 1/8
        bb = chunk_bbox[cb0 + seg // hs.CHUNK_SEGS].astype(np.float64)
        ex = max(bb[0] - Q.x[q], 0.0, Q.x[q] - bb[2])
        ey = max(bb[1] - Q.y[q], 0.0, Q.y[q] - bb[3])
        if (want["kind"][q] == X and want["item2"][q] == cc.LONG_ITEM and want["index2"][q] == seg and want["d2"][q] == Q.r2[q] == ex * ex + ey * ey > 0
                and want["kind"][q + 1] != X):
            on_edge_at_r += 1
    named = sc.named_chunks(cb0, cb1)
    if ident in cc.LONE_CLOSING:
        assert named[-1] == chunks - 1 and case.facts["named"] == named[:-1]
        named = named[:-1]
    assert won == named and named[0] == 0 and 63 in named and (64 in named) == (chunks > 65 or (chunks == 65 and ident not in cc.LONE_CLOSING)), (won, named)
    assert (chunks - 1 in won) != (ident in cc.LONE_CLOSING)
    if chunks >= 512 and (cb1 - 1) // hs.SUPER_CHUNKS - cb0 // hs.SUPER_CHUNKS + 1 > 64:
        behind = (cb0 // hs.SUPER_CHUNKS + 64) * hs.SUPER_CHUNKS - cb0
        assert behind in won and (cb0 + behind) // hs.SUPER_CHUNKS - cb0 // hs.SUPER_CHUNKS == 64, (won, behind)
    print(f"{ident}: crossings won in chunks {won}, {on_edge_at_r} with the edge, the segment and the crossing at exactly r")
    assert on_edge_at_r >= 1, on_edge_at_r
    assert (want["kind"] == MANY).any() == (chunks >= 512) and want["n_near"].max() >= 3 * chunks


def test_the_limit_cases_have_the_near_counts_they_claim(pm):
    for n_near in cc.LIMIT_NEAR:
        case = cc.limit_case(pm, n_near)
        want = case.expected()
        assert n_near in (511, 512, 513) and want["n_near"][:4].tolist() == [n_near, 2, 2, 2]
        crossing = (1, X, 0, np.float32(0.5), np.float32(20.0), np.float32(10.0), 25.0, 0, 0, np.float32(0.5))
        if n_near <= 512:
            assert want[0].tolist() == crossing + (n_near,)
        else:
            assert want[0].tolist() == (NONE, MANY, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0.0, 513)
        assert want[1].tolist() == crossing + (2,) and want[2].tolist() == crossing + (2,) and want[3]["item"] == NONE and want[3]["n_near"] == 2
        # the two Lines are the last in the order "precedes": what the walk stores last
        E = np_cross.Edges(bytes(case.scene))
        assert E.n == n_near and E.item[-2:].tolist() == [1, 0] and (E.item[:-2] == 2).all()
        assert want[4]["item"] == NONE and 2 <= want[4]["n_near"] < 200 and want[6].tolist() == crossing[:6] + (0.0, 0, 0, np.float32(0.5), 2)


# ---- CPU: np_cross's two evaluation orders -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.SMALL)
def test_evaluation_orders_agree(pm, name):
    case = cc.small_case(pm, name)
    for skip, masked in ((False, False), (True, True)):
        a = case.expected(skip, masked)
        b = np_cross.cross(case.scene, case.xyr, skip, case.mask if masked else None, per_first=True)
        assert same(a, b), (name, skip, masked, differing(a, b)[:8].tolist())
    if name == "ties":
        for other in (cc.walk_case(pm, 129), cc.long_case(pm, "comb-65"), cc.limit_case(pm, 512)):
            assert same(other.expected(), np_cross.cross(other.scene, other.xyr, per_first=True)), other


# ---- CPU: D23 against exact arithmetic; the near rule; the relation to D21 ------------------------------------------------------------

def _integer_segments(seed, n=14):
    """n segments on integer coordinates in [0, 32], float32 [n, 2, 2], and 12 cursors {x, y, r} on quarter pixels."""
    rng = np.random.default_rng([seed, 23])
    seg = rng.integers(0, 33, (n, 2, 2)).astype(np.float32)
    cur = np.concatenate([rng.integers(0, 129, (12, 2)) / 4.0, rng.choice([0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 13.0], (12, 1))], axis=1).astype(np.float32)
    return seg, cur


def _exact_pair(a, b, c, d, x, y, r):
    """D23 in rational arithmetic: (crosses within r, [the values and the bounds they are compared with]) or (False, None) where den == 0."""
    F = Fraction
    ax, ay, bx, by, cx, cy, dx, dy = (F(float(v)) for v in (*a, *b, *c, *d))
    rx, ry, sx, sy = bx - ax, by - ay, dx - cx, dy - cy
    den = rx * sy - ry * sx
    if den == 0:
        return False, None
    wx, wy = cx - ax, cy - ay
    t, u = (wx * sy - wy * sx) / den, (wx * ry - wy * rx) / den
    px, py = ax + rx * t, ay + ry * t
    d2, r2 = (F(float(x)) - px) ** 2 + (F(float(y)) - py) ** 2, F(float(r)) ** 2
    return 0 <= t <= 1 and 0 <= u <= 1 and d2 <= r2, [(t, F(0), F(1)), (t, F(1), F(1)), (u, F(0), F(1)), (u, F(1), F(1)), (d2, r2, r2)]


def test_d23_against_exact_arithmetic_and_the_near_rule():
    """Seeded segments on integer coordinates, every pair of them that shares no end, under 12 cursors each.  "Crosses within r" by
    Fractions EQUALS np_cross's formula wherever t, u and d2 are off their bounds by a relative 1e-9; at least 95 % of the (pair, cursor)
    combinations are that decisive.  And of ALL pairs, not filtered by near: a pair that qualifies by D23's formula while one of its edges
    is not near lies within a relative 1e-9 of r * r."""
    decisive = indecisive = agree_yes = dropped = dropped_far = 0
    eps = Fraction(1, 10**9)
    for seed in range(40):
        seg, cur = _integer_segments(seed)
        i, j = np.triu_indices(len(seg), 1)
        a, b, c, d = seg[i, 0], seg[i, 1], seg[j, 0], seg[j, 1]
        x, y, r = (cur[:, k].astype(np.float64) for k in range(3))
        ok, p = np_cross.qualifies(a[None], b[None], c[None], d[None], x[:, None], y[:, None], (r * r)[:, None])
        shared = p[0][0]
        near = np_snap.edge_d2(seg[:, 0], seg[:, 1], x, y) <= (r * r)[:, None]        # [cursor, segment]
        for q in range(len(cur)):
            for k in np.flatnonzero(~shared):
                exact, parts = _exact_pair(a[k], b[k], c[k], d[k], *cur[q])
                if parts is None:
                    assert not ok[q, k]
                    decisive += 1
                    continue
                # (a value is judged only if the comparisons before it let the decision reach it)
                t_in, u_in = 0 <= parts[0][0] <= 1, 0 <= parts[2][0] <= 1
                judged = parts[:2] + (parts[2:4] if t_in else []) + (parts[4:] if t_in and u_in else [])
                if any(abs(v - bound) <= eps * scale for v, bound, scale in judged):
                    indecisive += 1
                else:
                    decisive += 1
                    assert bool(ok[q, k]) == exact, (seed, q, k, seg[i[k]].tolist(), seg[j[k]].tolist(), cur[q].tolist())
                    agree_yes += exact
                if ok[q, k] and not (near[q, i[k]] and near[q, j[k]]):
                    dropped += 1
                    d2, r2, _ = parts[4]
                    dropped_far += abs(d2 - r2) > eps * r2
    total = decisive + indecisive
    print(f"{total} (pair, cursor) combinations, {decisive} decisive ({100.0 * decisive / total:.1f} %), {agree_yes} cross within r, 0 disagreements; "
          f"{dropped} qualify with an edge that is not near, {dropped_far} of them off r * r by more than 1e-9")
    assert decisive > 0 and decisive >= 0.95 * total and agree_yes >= 500
    assert dropped_far == 0


def test_an_intersection_implies_an_edge_by_d21(pm):
    """Wherever np_cross reports an intersection, np_snap with edges only finds an edge for the same query: both of a crossing's edges are
    within r by D21's own d2."""
    n = 0
    for case in [cc.small_case(pm, name) for name in cc.SMALL] + [cc.walk_case(pm, 65), cc.long_case(pm, "zigzag-65")]:
        for skip, masked in ((False, False), (True, True)):
            want = case.expected(skip, masked)
            snap = np_snap.snap(case.scene, case.xyr, vertices=False, skip_transparent=skip, skip_items=case.mask if masked else None)
            found = want["kind"] == X
            assert (snap["item"][found] != NONE).all() and (snap["d2"][found] <= want["d2"][found]).all(), case
            assert ((want["n_near"] > 0) == (snap["item"] != NONE)).all(), case
            n += int(found.sum())
    assert n >= 500


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_snap_cross_under_wave64_emulation(built):
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

def test_the_cross_kernel_uses_no_scratch(tmp_path):
    """pm_cross_kernel by the flags the library is built with: no private segment (nothing spilled, no indexed local array), VGPRs within
    128, and the LDS the header states: 48 KB a workgroup, three workgroups in a CU's 160 KB.  The VGPR figure is the compiler's count of
    the registers the kernel uses (NumVgprs in the listing).  The descriptor's next_free_vgpr is printed beside it: for a kernel whose
    static LDS bounds it to three waves per SIMD the compiler raises that field to the smallest value that allows no fourth wave, 129,
    whatever the kernel uses.  The figures are printed (pytest -s) and stand in DESIGN.md 4.  Sizes only: the assembly is searched for no
    instruction."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    stated = int(re.search(r"kCrossLdsBytes == (\d+)u", open(os.path.join(src, "pm_snap_cross.h")).read()).group(1))
    assert stated == 4 * cc.MAX_NEAR * 24
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = 0
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        if "pm_cross_kernel" not in m.group(1):
            continue
        found += 1
        assert "pm_snap_kernel" not in m.group(1)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        field = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        used = re.search(re.escape(m.group(1)) + r":.*?; NumVgprs: (\d+)\s*\n; NumAgprs: (\d+)", text, re.S)
        vgpr, agpr = int(used.group(1)), int(used.group(2))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"pm_cross_kernel: {vgpr} VGPRs, {agpr} AGPRs (next_free_vgpr {field}), {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and agpr == 0 and lds == stated, (m.group(1), scratch, vgpr, agpr, lds)
    assert found == 1
    assert "pm_snap_cross.h" in mk and "pm_snap.h" in mk     # (editing either header rebuilds the library)
