"""Rectangle queries, pm_hit_rects / pm_select_rect and their device variants (decision D19): which items a closed rectangle touches,
which it encloses -- picking with a tolerance and marquee selection.

The bar everywhere: top_item, n_hit and item_flags EQUAL to tests/np_rect.py, no tolerance, no query left out -- through the host
and the device calls, with and without counts, with and without skip_transparent.  tests/rect_cases.py builds the scenes and
places the rectangles.

-m gpu: small scenes, the item walk, long items, consistency of the two kernels, point rectangles against D13, the pick tolerance and
the hand-derived answers, output discipline and the argument rules, ordering against scene replacement and frames, the CLI.
CPU: the cases are what they claim (numpy alone); D19 against D13 on grids of points (np_rect against np_hit, no kernel); the
-m gpu part against the wave64 emulation of the kernels; the compiler's listing.

In the walk scene item 0 lies under every cell, so no rectangle touches ONLY the first or the last item of a step: the rectangles
there touch that item and item 0, and their top is that item.  The rectangle that touches the bottom item alone is there too."""
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
import np_rect  # noqa: E402
import rect_cases as rc  # noqa: E402

NONE = rc.NONE
UNTOUCHED = 0x7EADBEEF
T, E = np_rect.TOUCHES, np_rect.ENCLOSES
# small scenes, walk, long, consistency, point rectangles, pick tolerance, known answers, output discipline, argument rules, ordering (2), CLI
N_GPU_TESTS = len(rc.SMALL) + len(rc.WALK_SIZES) + len(rc.LONG_IDS) + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def device_hit_rects(pm, r, rects, skip=False, counts=True, pad=0, stream=None):
    """pm_hit_rects_device into arrays of n + pad words filled with UNTOUCHED: (top, n_hit or None, keep-alive), not waited for.
    Under the emulation device memory is host memory and the arrays are numpy's; on the GPU they are torch's."""
    rects = np.ascontiguousarray(rects, np.float32)
    n = len(rects)
    if _emulated():
        top = np.full(n + pad, UNTOUCHED, np.uint32)
        cnt = np.full(n + pad, UNTOUCHED, np.uint32) if counts else None
        flags = pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0
        pm._lib.check(pm._lib.load().pm_hit_rects_device(r._h, rects.ctypes.data, n, flags, top.ctypes.data, cnt.ctypes.data if counts else None, None),
                      "pm_hit_rects_device")
        return top, cnt, rects
    import torch

    dr = torch.from_numpy(rects).cuda()
    top = torch.full((n + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + pad,), UNTOUCHED, dtype=torch.int32, device="cuda") if counts else None
    r.hit_rects_tensor(dr, top[:n], cnt[:n] if counts else None, stream=stream, skip_transparent=skip)
    return top, cnt, dr


def device_select(pm, r, rect, n_items, skip=False, pad=0, stream=None):
    """pm_select_rect_device into n_items + pad words filled with UNTOUCHED, not waited for."""
    if _emulated():
        words = np.full(n_items + pad, UNTOUCHED, np.uint32)
        rect = np.ascontiguousarray(rect, np.float32)
        flags = pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0
        pm._lib.check(pm._lib.load().pm_select_rect_device(r._h, rect.ctypes.data, flags, words.ctypes.data, words.size, None), "pm_select_rect_device")
        return words
    import torch

    words = torch.full((n_items + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
    r.select_rect_tensor(*[float(v) for v in np.asarray(rect, np.float32)], words, stream=stream, skip_transparent=skip)
    return words


def as_u32(a):
    return a if isinstance(a, np.ndarray) or a is None else a.cpu().numpy().view(np.uint32)


def check_case(pm, r, case, skips=(False, True), select_every=1):
    """Host and device, with counts and without, under every flag: equal to np_rect.  pm_select_rect for every select_every-th rectangle."""
    n_items = case.flags().shape[0]
    for skip in skips:
        want = case.flags(skip)
        want_top, want_cnt = case.expected(skip)
        top, cnt = r.hit_rects(case.rects, skip_transparent=skip, counts=True)
        bad = np.flatnonzero((top != want_top) | (cnt != want_cnt))
        assert bad.size == 0, (case, skip, len(bad), [(case.rects[k].tolist(), int(top[k]), int(want_top[k]), int(cnt[k]), int(want_cnt[k])) for k in bad[:8]])
        first = r.hit_rects(case.rects, skip_transparent=skip)   # the walk that ends at the first item touched
        assert np.array_equal(first, want_top), (case, skip, np.flatnonzero(first != want_top)[:8].tolist())
        dt, dc, k1 = device_hit_rects(pm, r, case.rects, skip)
        d1, _, k2 = device_hit_rects(pm, r, case.rects, skip, counts=False)
        sel = list(range(0, len(case.rects), select_every))
        words = [device_select(pm, r, case.rects[k], n_items, skip) for k in sel]
        r.sync()
        assert np.array_equal(as_u32(dt), want_top) and np.array_equal(as_u32(dc), want_cnt) and np.array_equal(as_u32(d1), want_top), (case, skip)
        for k, w in zip(sel, words):
            assert np.array_equal(as_u32(w), want[:, k]), (case, skip, k, case.rects[k].tolist())
        for k in sel:
            touched, enclosed = r.select_rect(*case.rects[k], skip_transparent=skip)
            got = touched * T + enclosed * E
            assert np.array_equal(got, want[:, k]), (case, skip, k, case.rects[k].tolist(), np.flatnonzero(got != want[:, k])[:8].tolist())


@pytest.fixture(scope="module")
def rect_renderer(pm):
    """Never resized: the rectangle queries need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.SMALL)
def test_small_scenes(pm, pmo, rect_renderer, name):
    """mixed_scene, edge_scene (items at negative coordinates and beyond 65 535) and the oracle's path test and a scene of non-finite points under
    a few hundred seeded rectangles of every class; pm_select_rect and pm_select_rect_device for every one of them."""
    case = rc.small_case(pm, pmo, name)
    rect_renderer.set_scene_bytes(case.scene)
    check_case(pm, rect_renderer, case)


@pytest.mark.gpu
@pytest.mark.parametrize("n", rc.WALK_SIZES)
def test_item_walk_by_item_count(pm, rect_renderer, n):
    """One item fewer than a step of the walk, a step, one more, two steps and one: select_rect over the whole scene and one cell,
    hit_rects that must walk to the bottom item and ones whose top is at either end of a step."""
    case = rc.walk_case(pm, n)
    rect_renderer.set_scene_bytes(case.scene)
    assert rect_renderer.stats()["n_items"] == n
    check_case(pm, rect_renderer, case)


@pytest.mark.gpu
@pytest.mark.parametrize("ident", rc.LONG_IDS)
def test_long_items(pm, rect_renderer, ident):
    """A Fill (both rules) and a Polyline of 64, 65 and 513 chunks: rectangles decided by one segment of the last chunk, of chunk 64,
    by none, by the winding alone -- of few chunks and of all of them --, and ones that enclose all of it and all but a vertex."""
    case = rc.long_case(pm, ident)
    rect_renderer.set_scene_bytes(case.scene)
    check_case(pm, rect_renderer, case, skips=(False,))


@pytest.mark.gpu
def test_the_two_kernels_agree_on_the_device(pm, pmo, rect_renderer):
    """For the same rectangles n_hit is the number of PM_SEL_TOUCHES words of pm_select_rect, top_item the largest such index, and
    encloses implies touches.  (The last is a fact about these scenes' items, which have geometry wherever they have points: D19 does
    not promise it for, say, a rectangle around the point of a Polyline whose width is NaN.)"""
    r = rect_renderer
    for name in ("mixed", "edge"):
        case = rc.small_case(pm, pmo, name)
        r.set_scene_bytes(case.scene)
        rects = case.rects[::5]
        top, cnt = r.hit_rects(rects, counts=True)
        lib = pm._lib.load()
        import ctypes as C

        for k, rect in enumerate(rects):
            n_items, n_t, n_e = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            words = np.full(case.flags().shape[0], UNTOUCHED, np.uint32)
            assert lib.pm_select_rect(r._h, rect.ctypes.data, 0, words.ctypes.data, words.size, C.byref(n_items), C.byref(n_t), C.byref(n_e)) == pm._lib.PM_OK
            t, e = (words & T) != 0, (words & E) != 0
            assert n_items.value == len(words) and n_t.value == t.sum() == cnt[k] and n_e.value == e.sum()
            assert top[k] == (np.flatnonzero(t).max() if t.any() else NONE)
            assert not (e & ~t).any() and not (words & ~np.uint32(T | E)).any()


@pytest.mark.gpu
def test_point_rectangles_equal_point_hit_testing_on_circles(pm, rect_renderer):
    """Hand-derived: for the rectangle {x, y, x, y}, ex(c) = max(max(x - cx, 0), cx - x) = |x - cx| exactly (negation and max round
    nothing), so D19's dR2(c) <= r * r is D13's dx * dx + dy * dy <= r * r with dx = x - cx squared either way round, and the
    ellipse's quotients differ by sign alone.  On Circle and ellipse items hit_rects on {x, y, x, y} EQUALS hit_test on (x, y)."""
    def emit(e):
        e.circle((40.0, 40.0), 25.0)
        e.ellipse((90.0, 50.0), 30.0, 12.0)
        e.circle((100.5, 30.0), 8.5)
        e.ellipse((60.0, 80.0), 7.5, 22.0)
        e.ellipse((20.0, 100.0), 10.0, 0.0)

    scene = hs._encode(pm, 5, emit)
    rng = np.random.default_rng(31)
    q = np.concatenate([rng.uniform(0, 130, (600, 2)), (np.mgrid[0:131:5, 0:131:5].reshape(2, -1).T).astype(np.float64),
                        [[65.0, 40.0], [40.0, 15.0], [55.0, 60.0], [120.0, 50.0], [np.nan, 3.0]]]).astype(np.float32)
    r = rect_renderer
    r.set_scene_bytes(scene)
    top, cnt = r.hit_test(q, counts=True)
    rt, rn = r.hit_rects(np.concatenate([q, q], axis=1), counts=True)
    assert np.array_equal(top, rt) and np.array_equal(cnt, rn)
    assert cnt.max() >= 2 and (top == NONE).sum() > 50 and set(top.tolist()) >= {0, 1, 2, 3, NONE}


@pytest.mark.gpu
def test_the_pick_tolerance_does_what_it_is_for(pm, rect_renderer):
    """A Polyline one pixel wide and points two pixels off it: hit_test names nothing, pick(..., 3) names the Polyline."""
    scene = rc.known_scene(pm)
    r = rect_renderer
    r.set_scene_bytes(scene)
    pts = np.array([[15.0, 92.0], [60.5, 88.0], [118.25, 92.0], [64.0, 91.9]], np.float32)
    assert (r.hit_test(pts) == NONE).all()
    assert (r.pick(pts, 3.0) == 7).all()
    assert (r.pick(pts, 1.0) == NONE).all()                       # 2 - 1 > hw = 0.5 (the last: 1.9 - 1 > 0.5)
    assert r.pick(pts, 1.5).tolist() == [7, 7, 7, 7]              # 2 - 1.5 = hw exactly: a hit
    top, cnt = r.pick(pts, 3.0, counts=True)
    assert np.array_equal(np.stack([top, cnt]), np.stack(np_rect.hit_rects(scene, np_rect.pick_rects(pts, 3.0))))


@pytest.mark.gpu
def test_hand_derived_answers(pm, rect_renderer):
    """rect_cases.KNOWN, worked out in its comments: touching exactly at a corner, at hw exactly, inside a ring's hole, ..."""
    scene = rc.known_scene(pm)
    r = rect_renderer
    r.set_scene_bytes(scene)
    for rect, item, want in rc.KNOWN:
        touched, enclosed = r.select_rect(*rect)
        assert touched[item] * T + enclosed[item] * E == want, (rect, item, want)
    check_case(pm, r, rc.RectCase("known", scene, [k[0] for k in rc.KNOWN]))


@pytest.mark.gpu
def test_output_discipline(pm, pmo, rect_renderer):
    """Words beyond n and beyond n_items stay as they were, in the host and the device variants; without n_hit the array that would
    have been its stays as it was; PM_ERR_CAPACITY writes n_items and nothing else."""
    import ctypes as C

    case = rc.small_case(pm, pmo, "mixed")
    r = rect_renderer
    r.set_scene_bytes(case.scene)
    lib = pm._lib.load()
    rects = case.rects[:37]
    n, n_items = len(rects), case.flags().shape[0]
    want_top, want_cnt = (v[:n] for v in case.expected())
    for counts in (True, False):
        top = np.full(n + 5, UNTOUCHED, np.uint32)
        cnt = np.full(n + 5, UNTOUCHED, np.uint32)
        assert lib.pm_hit_rects(r._h, rects.ctypes.data, n, 0, top.ctypes.data, cnt.ctypes.data if counts else None) == pm._lib.PM_OK
        dt, dc, keep = device_hit_rects(pm, r, rects, counts=counts, pad=5)
        r.sync()
        for t, c in ((top, cnt), (as_u32(dt), as_u32(dc) if counts else cnt)):
            assert np.array_equal(t[:n], want_top) and (t[n:] == UNTOUCHED).all()
            assert (np.array_equal(c[:n], want_cnt) and (c[n:] == UNTOUCHED).all()) if counts else (c == UNTOUCHED).all()
    k = 3
    words = np.full(n_items + 4, UNTOUCHED, np.uint32)
    got_n = C.c_uint32(0)
    assert lib.pm_select_rect(r._h, rects[k].ctypes.data, 0, words.ctypes.data, words.size, C.byref(got_n), None, None) == pm._lib.PM_OK
    dw = device_select(pm, r, rects[k], n_items, pad=4)
    r.sync()
    for w in (words, as_u32(dw)):
        assert np.array_equal(w[:n_items], case.flags()[:, k]) and (w[n_items:] == UNTOUCHED).all()
    assert got_n.value == n_items
    words[:] = UNTOUCHED
    got_n, n_t, n_e = C.c_uint32(0), C.c_uint32(77), C.c_uint32(77)
    assert lib.pm_select_rect(r._h, rects[k].ctypes.data, 0, words.ctypes.data, n_items - 1, C.byref(got_n), C.byref(n_t), C.byref(n_e)) == pm._lib.PM_ERR_CAPACITY
    assert got_n.value == n_items and n_t.value == 77 and n_e.value == 77 and (words == UNTOUCHED).all()
    assert lib.pm_select_rect_device(r._h, rects[k].ctypes.data, 0, words.ctypes.data, n_items - 1, None) == pm._lib.PM_ERR_CAPACITY
    r.sync()
    assert (words == UNTOUCHED).all()


@pytest.mark.gpu
def test_argument_rules(pm, pmo):
    import ctypes as C

    lib = pm._lib.load()
    OK, INVALID = pm._lib.PM_OK, pm._lib.PM_ERR_INVALID
    with pm.Renderer(0) as r:
        top = np.full(4, UNTOUCHED, np.uint32)
        cnt = np.full(4, UNTOUCHED, np.uint32)
        words = np.full(16, UNTOUCHED, np.uint32)
        rects = np.array([[0, 0, 10, 10]] * 4, np.float32)
        tp, cp, rp, wp = top.ctypes.data, cnt.ctypes.data, rects.ctypes.data, words.ctypes.data
        hit = [lambda *a: lib.pm_hit_rects(r._h, *a), lambda *a: lib.pm_hit_rects_device(r._h, *a, None)]     # (rects, n, flags, top, n_hit)
        n_items = C.c_uint32(9)
        sel = [lambda *a: lib.pm_select_rect(r._h, *a, C.byref(n_items), None, None), lambda *a: lib.pm_select_rect_device(r._h, *a, None)]   # (rect, flags, words, cap)
        for call in hit:
            assert call(rp, 4, 0, tp, cp) == INVALID                 # no scene: what pm_hit_test says
        for call in sel:
            assert call(rp, 0, wp, 16) == INVALID
        assert n_items.value == 0
        r.set_scene_bytes(pmo.scene_path_test())
        for call in hit:
            assert call(rp, 4, 2, tp, cp) == INVALID                 # unknown flag bits
            assert call(rp, 4, 0x80000001, tp, cp) == INVALID
            assert call(None, 4, 0, tp, cp) == INVALID               # a NULL pointer with n > 0
            assert call(rp, 4, 0, None, cp) == INVALID
            assert call(None, 0, 0, None, None) == OK                # nothing to do
            assert call(rp, 0, 0, tp, cp) == OK
        for call in sel:
            assert call(rp, 2, wp, 16) == INVALID
            assert call(None, 0, wp, 16) == INVALID
            assert call(rp, 0, None, 16) == INVALID
        r.sync()
        assert (top == UNTOUCHED).all() and (cnt == UNTOUCHED).all() and (words == UNTOUCHED).all()
        assert n_items.value == r.stats()["n_items"] == 1
        assert hit[0](rp, 4, 1, tp, None) == OK and (cnt == UNTOUCHED).all() and (top != UNTOUCHED).all()
        assert sel[0](rp, 1, wp, 16) == OK and (words[1:] == UNTOUCHED).all() and words[0] != UNTOUCHED
        assert lib.pm_abi_version() == 600
        # the Python wrappers
        with pytest.raises(ValueError):
            r.hit_rects(np.zeros((3, 2), np.float32))
        with pytest.raises(ValueError):
            r.pick(np.zeros((3, 4), np.float32), 1.0)
        assert r.hit_rects(np.zeros((0, 4), np.float32)).shape == (0,)
        if not _emulated():
            import torch

            t = torch.zeros(4, dtype=torch.int32, device="cuda")
            with pytest.raises(TypeError):
                r.hit_rects_tensor(torch.zeros((4, 4)), t)                                   # not on the device
            with pytest.raises(TypeError):
                r.hit_rects_tensor(torch.zeros((4, 2), device="cuda"), t)                    # points, not rectangles
            with pytest.raises(TypeError):
                r.hit_rects_tensor(torch.zeros((4, 4), device="cuda"), t[:3])
            with pytest.raises(TypeError):
                r.select_rect_tensor(0, 0, 1, 1, torch.zeros(4, device="cuda"))              # floating point
            with pytest.raises(pm._lib.PietMetalError):
                r.select_rect_tensor(0, 0, 1, 1, t[:0])                                      # too short: PM_ERR_CAPACITY


def _tiger_rects(w, h, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (160, 2)) * (w, h)
    return np.concatenate([np.concatenate([c, c + rng.uniform(0.0, 24.0, (160, 2))], axis=1), [[0, 0, w, h], [w / 4, h / 4, w / 2, h / 2]]]).astype(np.float32)


@pytest.mark.gpu
def test_a_query_answers_for_the_scene_resident_at_the_call(pm):
    """The Tiger at 480 x 270: device calls on a caller's stream, followed at once by two re-flattens -- the answers are the first
    scene's; the host call afterwards answers for the last."""
    wl = pm.workloads.tiger(480, 270)
    rects = _tiger_rects(wl.width, wl.height, 41)
    with pm.Renderer(0) as r:
        _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene0 = r.download_scene()
        if _emulated():
            s = None
        else:
            import torch

            s = torch.cuda.Stream()
        top, cnt, keep = device_hit_rects(pm, r, rects, stream=s)
        words = device_select(pm, r, rects[-1], n_items, stream=s)
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        r.reflatten((0.9, 0.0, 0.0, 0.9, 40.0, 30.0), wl.width_scale)
        r.sync()
        if s is not None:
            s.synchronize()
        f0 = np_rect.item_flags(scene0, rects)
        want_top, want_cnt = np_rect.hit_rects(scene0, rects, flags=f0)
        assert np.array_equal(as_u32(top), want_top) and np.array_equal(as_u32(cnt), want_cnt) and np.array_equal(as_u32(words), f0[:, -1])
        assert len(set(want_top.tolist())) > 20 and (want_top == NONE).any() and (f0[:, -1] & E).any() and not (f0[:, -1] & E).all()
        scene2 = r.download_scene()
        f2 = np_rect.item_flags(scene2, rects)
        t2, c2 = r.hit_rects(rects, counts=True)
        assert np.array_equal(np.stack([t2, c2]), np.stack(np_rect.hit_rects(scene2, rects, flags=f2))) and not np.array_equal(t2, want_top)
        touched, enclosed = r.select_rect(*rects[-2])
        assert np.array_equal(touched * T + enclosed * E, f2[:, -2])


@pytest.mark.gpu
def test_queries_between_frames_leave_the_frames_alone(pm, pmo):
    """Frames rendered before and after rectangle queries have the bytes they have without them."""
    wl = pm.workloads.tiger(480, 270)
    rects = _tiger_rects(wl.width, wl.height, 42)[::4]
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want = pmo.render(scene, wl.width, wl.height)
        r.render()
        top, _, keep = device_hit_rects(pm, r, rects, counts=False)   # behind the frame, not waited for
        words = device_select(pm, r, rects[-1], n_items)
        first = r.read_pixels()
        r.render()
        top_host = r.hit_rects(rects)
        touched, enclosed = r.select_rect(*rects[-1])
        second = r.read_pixels()
        assert np.array_equal(first, want) and np.array_equal(second, want)
        f = np_rect.item_flags(scene, rects)
        assert np.array_equal(as_u32(top), top_host) and np.array_equal(top_host, np_rect.hit_rects(scene, rects, flags=f)[0])
        assert np.array_equal(as_u32(words), f[:, -1]) and np.array_equal(touched * T + enclosed * E, f[:, -1])


@pytest.mark.gpu
def test_cli_pick_tolerance_and_select(pm, tmp_path, capsys):
    """--pick-tolerance and --select print what the Renderer calls return."""
    from piet_metal_amd import cli

    picks = [(240.0, 135.0), (3.0, 3.0), (200.5, 100.5), (176.0, 60.0)]
    sel = (200.0, 100.0, 260.0, 150.0)
    args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--pick-tolerance", "2.5", "--select", ",".join(f"{v:g}" for v in sel)]
    for x, y in picks:
        args += ["--pick", f"{x:g},{y:g}"]
    assert cli.main(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        top = r.pick(np.array(picks, np.float32), 2.5)
        touched, enclosed = r.select_rect(*sel)
        of_item = r.item_paths()
    want = [f"{x:g},{y:g} +-2.5: " + ("none" if t == NONE else f"item {int(t)} path {int(of_item[t])}") for (x, y), t in zip(picks, top)]
    name = ",".join(f"{v:g}" for v in sel)
    want += [f"{name}: item {int(i)} path {int(of_item[i])}" + (" enclosed" if enclosed[i] else "") for i in np.flatnonzero(touched)]
    assert lines == want
    assert any(ln.endswith("none") for ln in lines) and any(ln.endswith("enclosed") for ln in lines) and touched.sum() > enclosed.sum() > 0
    # a rectangle that touches nothing
    assert cli.main(["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270", "--select", "1,1,3,3"]) == 0
    assert [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()] == ["1,1,3,3: none"]


# ---- CPU: the cases are what they claim (numpy alone) -------------------------------------------------------------------------

def test_structural_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_hit_rect.h")).read()
    assert "hi > 64u ? hi - 64u : 0u" in text and "ItemSteps(V.n_items)" in text and "step * 64u + 64u" in text
    common = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_query_common.h")).read()   # (ItemSteps: the steps of 64 items)
    assert "uint32_t ItemSteps(uint32_t n_items) { return (n_items + 63u) / 64u; }" in common
    assert rc.WAVE == 64 and rc.WALK_SIZES == (63, 64, 65, 129) and rc.LONG_CHUNKS == (64, 65, 513) and hs.CHUNK_SEGS == 4
    inc = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    assert "#define PM_SEL_TOUCHES 1u" in inc and "#define PM_SEL_ENCLOSES 2u" in inc and "#define PM_ABI_VERSION 600" in inc


def test_the_small_cases_have_every_class(pm, pmo):
    mixed = rc.small_case(pm, pmo, "mixed")
    f = mixed.flags()
    at = {tuple(np.float32(r).tolist()): k for k, r in enumerate(mixed.rects.tolist())}
    col = lambda r: f[:, at[tuple(np.float32(r).tolist())]]   # noqa: E731
    sc = bytes(mixed.scene)
    for r in rc.MIXED_INSIDE_FILL:    # inside item 0: touched, though no edge of it meets the rectangle
        a, b = np_hit.fill_segments(np_hit._points(sc, np_hit.flat_items(sc)[0][0]), False)
        assert col(r)[0] == T and not np_rect.segments_meet(np_rect.Rects([r]), a, b).any()
    for r in rc.MIXED_IN_EO_HOLE:     # in the even-odd ring's hole: the ring is not touched, the square under it is
        assert col(r)[2] == 0 and col(r)[0] == T
    assert col(rc.MIXED_NZ_HOLE[0])[6] == 0 and col(rc.MIXED_NZ_HOLE[1])[6] == T      # in the reversed hole; ... and reaching the square in it
    assert col(rc.MIXED_NZ_HOLE[2])[6] == T and col(rc.MIXED_NZ_HOLE[3])[6] == T      # around the hole; on its edges
    top, cnt = mixed.expected()
    tops, _ = mixed.expected(True)
    assert set(range(10)) <= set(top.tolist()) and NONE in top and cnt.max() >= 3 and (top != tops).any()
    assert (f & E).any(axis=1).sum() >= 6 and ((f & E) != 0).sum() < ((f & T) != 0).sum()
    valid = np_rect.Rects(mixed.rects).valid
    assert (~valid).sum() == len(rc.INVALID) and (f[:, ~valid] == 0).all()
    degenerate = (mixed.rects[:, 0] == mixed.rects[:, 2]) | (mixed.rects[:, 1] == mixed.rects[:, 3])
    assert degenerate.sum() >= 60 and (f[:, degenerate] & T).any(axis=0).sum() >= 30
    edge = rc.small_case(pm, pmo, "edge")
    fe = edge.flags()
    boxes = np.array([b for _, b in np_hit.flat_items(bytes(edge.scene))])
    assert (boxes[:, :2] == 0).any() and (boxes[:, 2] == 65535).sum() >= 2      # the saturated edges are there
    x0, x1 = edge.rects[:, 0], edge.rects[:, 2]
    beyond, negative = x0 > 65535, x1 < 0
    assert (fe[1, beyond] & T).any() and (fe[3, beyond] & T).any() and (fe[0, negative] & T).any() and (fe[2, negative] & T).any()
    assert (fe[0] & E).any() and len(edge.rects) >= 300 and len(mixed.rects) >= 300
    nf = rc.small_case(pm, pmo, "nonfinite")
    fn = nf.flags()
    box0 = np_hit.flat_items(bytes(nf.scene))[0][1]
    left = nf.rects[:, 2] < box0[0]            # wholly left of item 0's box, and touched by it all the same: D13 never culls by "left"
    assert box0[0] == 100 and (fn[0, left] & T).any() and not (fn[4] & T).any() and (fn[1] & T).any() and (fn[3] & T).any() and len(nf.rects) >= 200
    pt = rc.small_case(pm, pmo, "path_test")
    assert set(pt.expected()[0].tolist()) == {0, NONE} and len(pt.rects) >= 200


@pytest.mark.parametrize("n", rc.WALK_SIZES)
def test_the_walk_cases_are_what_they_claim(pm, n):
    case = rc.walk_case(pm, n)
    f = case.flags()
    top, cnt = case.expected()
    assert f.shape[0] == n and (f[:, 0] == (T | E)).all()            # the whole scene: everything touched and enclosed
    assert ((f[:, 1] & T) != 0).sum() >= 2 and (f[7, 1] & E) and not (f[:, 1] & E).sum() > 2    # one cell: its item, enclosed
    assert top[2] == 0 and cnt[2] == 1                               # the empty corner: the bottom item alone, the walk's last lane
    ends = case.facts["ends"]
    assert top[3 : 3 + len(ends)].tolist() == ends and (cnt[3 : 3 + len(ends)] == 2).all()
    # lane 2 of the first step (the topmost item with a cell), and lanes 63 and 0 of every step where those items have a cell
    assert ends[0] == n - 3 and set(ends[1:]) == {i for k in range(3) for i in (n - 64 * k - 64, n - 64 * k - 65) if 1 <= i <= n - 3}
    assert len(ends) == {63: 1, 64: 1, 65: 2, 129: 4}[n]
    assert top[-1] == NONE and top[-2] == NONE


@pytest.mark.parametrize("ident", rc.LONG_IDS)
def test_the_long_cases_are_decided_where_they_claim(pm, ident):
    """With hit_structure's model of the index: the segments that meet rectangles 0 and 1 lie in the chunk named, and in no other;
    rectangle 2 meets none; a Fill's rectangle 3 meets none and is inside by the winding; 4 encloses the item, 5 does not."""
    case = rc.long_case(pm, ident)
    sc = bytes(case.scene)
    base, chunk_bbox, sup_bbox = hs.index_model(case.scene)
    cb0, cb1 = int(base[rc.LONG_ITEM]), int(base[rc.LONG_ITEM + 1])
    chunks = case.facts["chunks"]
    assert cb1 - cb0 == chunks and cb0 % hs.SUPER_CHUNKS == 3
    assert (chunks > 512) == ((cb1 - 1) // hs.SUPER_CHUNKS - cb0 // hs.SUPER_CHUNKS + 1 > 64)     # 513 chunks: a second round of super-chunks
    ent, a, b, _ = hs._entries(sc, np_hit.flat_items(sc)[rc.LONG_ITEM][0])
    R = np_rect.Rects(case.rects)
    fill = case.facts["kind"] != "polyline"
    if fill:
        near = np_rect.segments_meet(R, a, b)
    else:
        hw = 0.25
        near = np_rect.segments_meet(R, a, b) | (np_rect.dist2_to_rect(R, a[:, 0], a[:, 1]) <= hw * hw) | (np_rect.dist2_to_rect(R, b[:, 0], b[:, 1]) <= hw * hw)
        for cx, cy in R.corners():
            near |= np_hit._stroke_pairs(a[None], b[None], hw, cx[:, None], cy[:, None])
    for k, s in enumerate(case.facts["segs"]):
        assert np.flatnonzero(near[k]).tolist() == [s], (ident, k)
    assert case.facts["segs"][0] // 4 == chunks - 1 and case.facts["segs"][1] // 4 == min(64, chunks - 1)
    assert not near[2].any() and not near[3].any()
    f = case.flags()[rc.LONG_ITEM]
    assert f.tolist() == [T, T, 0, T if fill else 0, T | E, T, T if fill else 0] and not near[6].any()
    if fill:    # rectangle 6: the corner's winding is carried by many chunks, in more super-chunks than one expansion of survivors takes
        con = hs.Contributions(case.scene, rc.LONG_ITEM, case.rects[6:7, :2])
        carrying = np.flatnonzero(con.per_chunk[0])
        passing = np.flatnonzero(hs.box_pass(con, chunk_bbox[cb0:cb1], case.rects[6:7, :2])[0])
        assert set(carrying) <= set(passing) and len(carrying) >= chunks // 4
        assert len(set((cb0 + carrying) // hs.SUPER_CHUNKS)) >= (17 if chunks > 512 else 4)
    assert case.expected()[0].tolist()[:3] == [1, 1, NONE]


def test_hand_derived_answers_by_numpy(pm):
    scene = rc.known_scene(pm)
    f = np_rect.item_flags(scene, [k[0] for k in rc.KNOWN])
    got = [int(f[item, k]) for k, (_, item, _) in enumerate(rc.KNOWN)]
    assert got == [want for _, _, want in rc.KNOWN], [(rc.KNOWN[k][0], rc.KNOWN[k][1], g, rc.KNOWN[k][2]) for k, g in enumerate(got) if g != rc.KNOWN[k][2]]
    assert len(rc.KNOWN) >= 12


# ---- CPU: D19 is the right definition (np_rect against np_hit, no kernel) ---------------------------------------------------------

def _witness_scene(pm, seed):
    """Blobs and strokes at generic, non-aligned coordinates."""
    rng = np.random.default_rng(seed)

    def blob(c, r, n):
        t = np.sort(rng.uniform(0, 2 * np.pi, n))
        rad = r * rng.uniform(0.55, 1.0, n)
        return np.stack([c[0] + rad * np.cos(t), c[1] + rad * np.sin(t)], axis=1)

    def emit(e):
        for k in range(10):
            c = rng.uniform(30, 270, 2)
            kind = k % 5
            if kind == 0:
                e.fill(blob(c, rng.uniform(10, 40), 11), 0x336699FF, even_odd=bool(k & 1))
            elif kind == 1:
                r = rng.uniform(20, 40)
                e.fill_compound([blob(c, r, 9), blob(c, 0.4 * r, 7)[:: -1 if k & 2 else 1]], 0xAA5500FF, even_odd=not (k & 2))
            elif kind == 2:
                e.polyline(c + np.cumsum(rng.uniform(-25, 25, (6, 2)), axis=0), 0x11AA22FF, float(rng.uniform(0.5, 7.0)))
            elif kind == 3:
                e.stroke_line(tuple(c), tuple(c + rng.uniform(-60, 60, 2)), float(rng.uniform(0.5, 9.0)), 0x000000FF)
            else:
                e.ellipse(tuple(np.round(c)), float(rng.integers(5, 30)), float(rng.integers(5, 30))) if k & 1 else e.circle(tuple(np.round(c)), float(rng.integers(5, 30)))

    return hs._encode(pm, 10, emit)


def _grid(rects, n=9):
    """float32 [len(rects), n * n, 2]: an n x n grid of points over every rectangle, ends included."""
    r = np.asarray(rects, np.float32).astype(np.float64)
    t = np.linspace(0.0, 1.0, n)
    x = r[:, 0, None] + (r[:, 2] - r[:, 0])[:, None] * t
    y = r[:, 1, None] + (r[:, 3] - r[:, 1])[:, None] * t
    g = np.stack([np.repeat(x[:, None, :], n, axis=1), np.repeat(y[:, :, None], n, axis=2)], axis=3).reshape(len(r), n * n, 2)
    g = g.astype(np.float32)
    lo, hi = np.asarray(rects, np.float32)[:, None, :2], np.asarray(rects, np.float32)[:, None, 2:]
    return np.clip(g, lo, hi)       # (rounding to f32 never leaves the rectangle)


WITNESS_SEEDS = (51, 52, 53)


@pytest.mark.parametrize("seed", WITNESS_SEEDS)
def test_d19_agrees_with_d13_on_grids_of_points(pm, seed):
    """Conditions on the restatement, not on a kernel, with no exception: every item that contains (D13, np_hit) any point of a 9 x 9
    grid over R is touched by R; and an item R encloses contains no grid point of a rectangle disjoint from R.
    Decisive pairs over the three seeds (51, 52, 53), 600 rectangles each on a scene of 10 items: 1 244 (rectangle, item) pairs with a
    grid point in the item, every one of them touched (of 1 414 touched pairs in all -- the others are thin strokes and edges between
    grid points); 218 enclosed pairs, checked against 96 335 (disjoint rectangle, enclosed item) combinations, none with a grid point
    in the item."""
    scene = _witness_scene(pm, seed)
    rng = np.random.default_rng(seed + 1000)
    c = rng.uniform(-20, 280, (600, 2))
    size = np.where(rng.uniform(0, 1, (600, 1)) < 0.4, rng.uniform(40, 160, (600, 2)), rng.uniform(0.5, 30, (600, 2)))
    rects = np.concatenate([c, c + size], axis=1).astype(np.float32)
    f = np_rect.item_flags(scene, rects)
    n_items = f.shape[0]
    g = _grid(rects)
    inside = np.zeros((n_items, len(rects)), bool)
    contains = np.zeros((n_items, len(rects), g.shape[1]), bool)
    for i in range(n_items):
        contains[i] = np_hit.item_inside(scene, i, g.reshape(-1, 2)).reshape(len(rects), -1)
        inside[i] = contains[i].any(axis=1)
    touched, enclosed = (f & T) != 0, (f & E) != 0
    assert not (inside & ~touched).any(), np.argwhere(inside & ~touched)[:8].tolist()
    assert not (enclosed & ~touched).any()
    r64 = rects.astype(np.float64)
    disjoint = (r64[:, None, 2] < r64[None, :, 0]) | (r64[None, :, 2] < r64[:, None, 0]) | (r64[:, None, 3] < r64[None, :, 1]) | (r64[None, :, 3] < r64[:, None, 1])
    checked = 0
    for i in range(n_items):
        for k in np.flatnonzero(enclosed[i]):
            others = np.flatnonzero(disjoint[k])
            assert not inside[i, others].any(), (i, k, others[inside[i, others]][:4].tolist())
            checked += len(others)
    print(f"seed {seed}: {int(inside.sum())} pairs with a grid point inside, {int(touched.sum())} touched, {int(enclosed.sum())} enclosed, {checked} disjoint combinations")
    assert inside.sum() >= 100 and enclosed.sum() >= 10 and checked >= 1000     # (floors against a blind test, far below what the seeds give)


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_hit_rect_under_wave64_emulation(built):
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

def test_the_rectangle_kernels_use_no_scratch(tmp_path):
    """pm_hit_rects_kernel and pm_select_rect_kernel by the flags the library is built with: no private segment (nothing spilled, no
    indexed local array), no LDS, and VGPRs within 128 -- a workgroup of four waves puts one on each SIMD of a CU, which has 512 VGPRs
    per lane: four such workgroups per CU, the eight the launch asks for at 64.  The figures are printed (pytest -s) and stand in
    DESIGN.md 4."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = set()
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        name = next((k for k in ("pm_hit_rects_kernel", "pm_select_rect_kernel") if k in m.group(1)), None)
        if name is None:
            continue
        found.add(name)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"{name}: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and lds == 0, (m.group(1), scratch, vgpr, lds)
    assert found == {"pm_hit_rects_kernel", "pm_select_rect_kernel"}
