"""The item map, pm_hit_frame / pm_hit_frame_device (decision D18): the topmost item under every pixel of a rectangle.

The bar everywhere: top_item and n_hit EQUAL to tests/np_hit.py on the window's pixel centres, float32(x0 + i) + 0.5 -- with and without
skip_transparent, in the counting walk and in the walk that ends at a pixel's first hit, through the host call and through the device
call.  tests/hit_frame_cases.py builds the scenes and places the windows.

-m gpu: window geometry, output discipline, the item walk by item count, long items by chunks per round, geometry on pixel centres,
the Tiger against pm_hit_test, ordering against frames and scene replacement, the argument rules and the CLI.
CPU: no window is blind (np_hit alone); the -m gpu part against the wave64 emulation of the kernel; the compiler's listing.

Two things the cases cannot do as first written down, and what they do instead (hit_frame_cases.py says why at each place):
  * a 1 x 1 window cannot hold two items and nothing: three 1 x 1 windows per scene do so together; edge_scene's items are too far
    apart, and the oracle's path test is one Fill, so their small windows hold one item and nothing;
  * an alpha-0 Fill over ALL pixels would leave no other item on top without the skip: it covers half the pixels of every tile."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hit_frame_cases as fc  # noqa: E402
import np_hit  # noqa: E402

NONE = fc.NONE
UNTOUCHED = 0x7EADBEEF
GEOMETRY_IDS = [f"{name}-{w}x{h}" for name in fc.REGIONS for w, h in fc.SIZES] + \
               [f"{name}-1x1-{k}" for name in fc.REGIONS for k in range(fc.ITEMS_WANTED[name] + 1)] + \
               [f"{name}-48x40-origin" for name in fc.REGIONS] + ["edge-ends-at-65536", "edge-72x64-origin"]
# geometry, output discipline, walk, long items, centres, batches of rows, the Tiger, ordering (2), argument rules, the CLI
N_GPU_TESTS = len(GEOMETRY_IDS) + 1 + len(fc.WALK_SIZES) + len(fc.LONG_IDS) + 1 + 1 + 1 + 2 + 1 + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def device_frame(pm, r, rect, skip=False, counts=True, pad_rows=0, pad_cols=0, stream=None):
    """pm_hit_frame_device into arrays of h + 2 pad_rows rows of w + pad_cols words filled with UNTOUCHED, the rectangle's rows in
    the middle: (top, n_hit or None) as uint32 [h + 2 pad_rows, w + pad_cols], not waited for.  Under the emulation device memory
    is host memory and the arrays are numpy's; on the GPU they are torch's and go through Renderer.hit_frame_tensor as views."""
    x0, y0, w, h = rect
    shape = (h + 2 * pad_rows, w + pad_cols)
    if _emulated():
        top = np.full(shape, UNTOUCHED, np.uint32)
        cnt = np.full(shape, UNTOUCHED, np.uint32) if counts else None
        flags = pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0
        at = pad_rows * shape[1] * 4
        pm._lib.check(pm._lib.load().pm_hit_frame_device(r._h, x0, y0, w, h, flags, top.ctypes.data + at, cnt.ctypes.data + at if counts else None,
                                                         shape[1], None), "pm_hit_frame_device")
        return top, cnt
    import torch

    top = torch.full(shape, UNTOUCHED, dtype=torch.int32, device="cuda")
    cnt = torch.full(shape, UNTOUCHED, dtype=torch.int32, device="cuda") if counts else None
    view = lambda t: t[pad_rows : pad_rows + h, :w]  # noqa: E731
    r.hit_frame_tensor(view(top), view(cnt) if counts else None, x0=x0, y0=y0, stream=stream, skip_transparent=skip)
    return top, cnt


def as_u32(a):
    return a if isinstance(a, np.ndarray) or a is None else a.cpu().numpy().view(np.uint32)


def check_window(pm, r, wdw, skips=(False, True)):
    """Host and device, with counts and without, under every flag: equal to np_hit.  Returns the expectation without the skip."""
    x0, y0, w, h = wdw.rect
    for skip in skips:
        want_top, want_cnt = wdw.expected(skip)
        top, cnt = r.hit_frame(x0, y0, w, h, skip_transparent=skip, counts=True)
        bad = np.argwhere((top != want_top) | (cnt != want_cnt))
        assert bad.size == 0, (wdw, skip, len(bad), [(int(i), int(j), int(top[j, i]), int(want_top[j, i]), int(cnt[j, i]), int(want_cnt[j, i])) for j, i in bad[:8]])
        first = r.hit_frame(x0, y0, w, h, skip_transparent=skip)   # the walk that ends at a pixel's first hit
        assert np.array_equal(first, want_top), (wdw, skip, np.argwhere(first != want_top)[:8].tolist())
        dt, dc = device_frame(pm, r, wdw.rect, skip)
        d1, _ = device_frame(pm, r, wdw.rect, skip, counts=False)
        r.sync()
        assert np.array_equal(as_u32(dt), want_top) and np.array_equal(as_u32(dc), want_cnt) and np.array_equal(as_u32(d1), want_top), (wdw, skip)
    return wdw.expected(False)


@pytest.fixture(scope="module")
def hit_renderer(pm):
    """Never resized: the item map needs a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ident", GEOMETRY_IDS)
def test_window_geometry(pm, pmo, hit_renderer, ident):
    """Part 1: windows of one pixel, one tile, one pixel more than a tile in either direction, two tiles and a bit at an origin
    that is no multiple of 16, three tiles by two and a half at the origin, and the two ends of what a u16 box can say."""
    wdw = {w.ident: w for w in fc.geometry_windows(pm, pmo)}[ident]
    hit_renderer.set_scene_bytes(wdw.scene)
    want_top, _ = check_window(pm, hit_renderer, wdw)
    if ident == "edge-ends-at-65536":   # the last column's centre is beyond the saturated edge of both boxes, and inside both items
        assert wdw.rect[0] + wdw.rect[2] == 65536 and 1 in want_top[:, -1] and 3 in want_top[:, -1]
    if ident == "edge-72x64-origin":
        assert want_top[0, 0] == 0 and want_top[-1, -1] == NONE


@pytest.mark.gpu
def test_output_discipline(pm, pmo, hit_renderer):
    """Part 2: stride = w + 3 and two padding rows above and below -- every word outside the w x h rectangle stays as it was, in the
    host and in the device variant; without n_hit the array that would have been its stays as it was."""
    wdw = {w.ident: w for w in fc.geometry_windows(pm, pmo)}["mixed-33x18"]
    r = hit_renderer
    r.set_scene_bytes(wdw.scene)
    x0, y0, w, h = wdw.rect
    want_top, want_cnt = wdw.expected()
    lib = pm._lib.load()

    def check(top, cnt, counts):
        assert np.array_equal(top[2 : 2 + h, :w], want_top)
        assert (top[:2] == UNTOUCHED).all() and (top[2 + h :] == UNTOUCHED).all() and (top[:, w:] == UNTOUCHED).all()
        if counts:
            assert np.array_equal(cnt[2 : 2 + h, :w], want_cnt)
            assert (cnt[:2] == UNTOUCHED).all() and (cnt[2 + h :] == UNTOUCHED).all() and (cnt[:, w:] == UNTOUCHED).all()
        else:
            assert (cnt == UNTOUCHED).all()

    for counts in (True, False):
        top = np.full((h + 4, w + 3), UNTOUCHED, np.uint32)
        cnt = np.full((h + 4, w + 3), UNTOUCHED, np.uint32)
        at = 2 * (w + 3) * 4
        assert lib.pm_hit_frame(r._h, x0, y0, w, h, 0, top.ctypes.data + at, cnt.ctypes.data + at if counts else None, w + 3) == pm._lib.PM_OK
        check(top, cnt, counts)
        dt, dc = device_frame(pm, r, wdw.rect, counts=counts, pad_rows=2, pad_cols=3)
        r.sync()
        check(as_u32(dt), as_u32(dc) if counts else np.full((h + 4, w + 3), UNTOUCHED, np.uint32), counts)


@pytest.mark.gpu
@pytest.mark.parametrize("n", fc.WALK_SIZES)
def test_item_walk_by_item_count(pm, hit_renderer, n):
    """Part 3: one item fewer than a step of the walk, a step, one more, two steps and one."""
    wdw = fc.walk_window(pm, n)
    r = hit_renderer
    r.set_scene_bytes(wdw.scene)
    assert r.stats()["n_items"] == n
    want_top, want_cnt = check_window(pm, r, wdw)
    assert want_cnt.max() >= 3 and set(range(n)) <= set(want_top.ravel().tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("ident", fc.LONG_IDS)
def test_long_item_by_chunks_per_round(pm, hit_renderer, ident):
    """Part 4: a long Fill / compound Fill / Polyline of one chunk fewer than a round, a round, one more, two rounds and one."""
    wdw = fc.long_window(pm, ident)
    hit_renderer.set_scene_bytes(wdw.scene)
    want_top, _ = check_window(pm, hit_renderer, wdw, skips=(False,))
    assert (want_top == wdw.facts["long_item"]).sum() >= 16


@pytest.mark.gpu
def test_geometry_on_pixel_centres(pm, hit_renderer):
    """Part 5."""
    wdw = fc.centres_window(pm)
    hit_renderer.set_scene_bytes(wdw.scene)
    want_top, want_cnt = check_window(pm, hit_renderer, wdw)
    assert set(range(8)) <= set(want_top.ravel().tolist()) and want_cnt.max() >= 2


@pytest.mark.gpu
def test_the_host_call_stages_batches_of_rows(pm, hit_renderer):
    """The host variant stages whole rows through device memory, about four million pixels at a time: a window as wide as pixels
    exist, 65 536 (64 rows to a batch), and 70 rows high is two batches.  Both saturated box edges are in it; the destination has
    a stride and a row more than the window."""
    from test_hit_gpu import edge_scene

    scene = edge_scene(pm)
    x0, y0, w, h = 0, 3, 65536, 70
    r = hit_renderer
    r.set_scene_bytes(scene)
    want_top, want_cnt = np_hit.hit_test(scene, fc.centres(x0, y0, w, h))
    assert fc.not_blind(want_top) and want_top[w - 1] == 1 and want_top[0] == 0     # (the first row: both ends lie in a saturated box)
    top = np.full((h + 1, w + 5), UNTOUCHED, np.uint32)
    cnt = np.full((h + 1, w + 5), UNTOUCHED, np.uint32)
    assert pm._lib.load().pm_hit_frame(r._h, x0, y0, w, h, 0, top.ctypes.data, cnt.ctypes.data, w + 5) == pm._lib.PM_OK
    assert np.array_equal(top[:h, :w].ravel(), want_top) and np.array_equal(cnt[:h, :w].ravel(), want_cnt)
    assert (top[h:] == UNTOUCHED).all() and (top[:, w:] == UNTOUCHED).all() and (cnt[h:] == UNTOUCHED).all() and (cnt[:, w:] == UNTOUCHED).all()
    assert np.array_equal(r.hit_frame(x0, y0, w, h).ravel(), want_top)


def _hit_test_map(pm, r, w, h, skip=False):
    """pm_hit_test_device on the w x h pixel centres from (0, 0): (top, n_hit) uint32 [h, w]."""
    q = fc.centres(0, 0, w, h)
    if _emulated():
        top, cnt = r.hit_test(q, skip_transparent=skip, counts=True)
        return top.reshape(h, w), cnt.reshape(h, w)
    import torch

    xy = torch.from_numpy(q).cuda()
    top = torch.empty(w * h, dtype=torch.int32, device="cuda")
    cnt = torch.empty(w * h, dtype=torch.int32, device="cuda")
    r.hit_test_tensor(xy, top, cnt, skip_transparent=skip)
    r.sync()
    return as_u32(top).reshape(h, w), as_u32(cnt).reshape(h, w)


@pytest.mark.gpu
def test_the_tiger_against_pm_hit_test(pm):
    """Part 6: the Tiger flattened on the device at 160 x 90 -- the whole map against pm_hit_test on the same 14 400 points, a 48 x 24
    window against np_hit; again after a re-flatten; again with one group painted to opacity 0, under skip_transparent."""
    wl = pm.workloads.tiger(160, 90)
    paths = wl.paths.with_groups(np.arange(len(wl.paths.paths), dtype=np.uint32) % 4)   # (the Tiger itself is one group)
    W, H = wl.width, wl.height
    sub = (24, 30, 48, 24)

    def compare(r, skip=False):
        top, cnt = device_frame(pm, r, (0, 0, W, H), skip)
        first, _ = device_frame(pm, r, (0, 0, W, H), skip, counts=False)
        r.sync()
        top, cnt, first = as_u32(top), as_u32(cnt), as_u32(first)
        ht, hc = _hit_test_map(pm, r, W, H, skip)
        assert np.array_equal(top, ht) and np.array_equal(cnt, hc) and np.array_equal(first, ht)
        scene = r.download_scene()
        wt, wc = np_hit.hit_test(scene, fc.centres(*sub), skip)
        x0, y0, w, h = sub
        assert np.array_equal(top[y0 : y0 + h, x0 : x0 + w].ravel(), wt) and np.array_equal(cnt[y0 : y0 + h, x0 : x0 + w].ravel(), wc)
        assert fc.not_blind(wt.reshape(h, w))
        return top

    with pm.Renderer(0) as r:
        r.flatten_and_encode(paths, wl.affine, wl.width_scale)
        top = compare(r)
        # item_paths()[map] names the paths that --pick names: the path of what pm_hit_test finds under the point
        of_item = r.item_paths()
        picks = [(80, 45), (1, 1), (66, 33), (86, 63)]
        picked = r.hit_test(np.array([(x + 0.5, y + 0.5) for x, y in picks], np.float32))
        for (x, y), t in zip(picks, picked):
            assert top[y, x] == t and (t == NONE or of_item[top[y, x]] == of_item[t])
        assert (picked == NONE).any() and (picked != NONE).any()
        r.reflatten((0.35, 0.2, -0.2, 0.35, 60.0, 5.0), wl.width_scale)
        top2 = compare(r)
        assert not np.array_equal(top, top2)
        # the skip must see the PAINTED alpha: the group that holds the item on top of the view's centre fades to nothing
        r.reflatten(wl.affine, wl.width_scale)
        groups = np.asarray(paths.groups)
        g = int(groups[of_item[top[45, 80]]])
        opac = np.full(paths.n_groups(), 255, np.uint32)
        opac[g] = 0
        r.repaint_groups(opac)
        faded = compare(r, skip=True)
        assert np.array_equal(compare(r, skip=False), top)
        gone = groups[of_item[top[top != NONE]]] == g
        assert gone.any() and (faded[top != NONE][gone] != top[top != NONE][gone]).all() and not (groups[of_item[faded[faded != NONE]]] == g).any()


@pytest.mark.gpu
def test_item_maps_between_frames_leave_the_frames_alone(pm, pmo):
    """Part 7: frames rendered before and after an item map have the bytes they have without it."""
    wl = pm.workloads.tiger(160, 90)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want = pmo.render(scene, wl.width, wl.height)
        r.render()
        top, _ = device_frame(pm, r, (0, 0, wl.width, wl.height), counts=False)  # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        top_host = r.hit_frame(0, 0, wl.width, wl.height)
        second = r.read_pixels()
        assert np.array_equal(first, want) and np.array_equal(second, want)
        assert np.array_equal(as_u32(top), top_host)
        sub = (56, 30, 48, 24)
        assert np.array_equal(top_host[30:54, 56:104].ravel(), np_hit.hit_test(scene, fc.centres(*sub))[0])


@pytest.mark.gpu
def test_an_item_map_answers_for_the_scene_resident_at_the_call(pm, pmo):
    """Part 7: an item map on a side stream, then at once another scene: the map is the first scene's, the next one the second's."""
    a, b = fc.walk_window(pm, fc.WALK_SIZES[0]), fc.centres_window(pm)
    with pm.Renderer(0) as r:
        r.set_scene_bytes(a.scene)
        if _emulated():
            s = None
        else:
            import torch

            s = torch.cuda.Stream()
        top, cnt = device_frame(pm, r, a.rect, stream=s)
        r.set_scene_bytes(b.scene)
        top_b, cnt_b = device_frame(pm, r, b.rect, stream=s)
        r.sync()
        if s is not None:
            s.synchronize()
        assert np.array_equal(as_u32(top), a.expected()[0]) and np.array_equal(as_u32(cnt), a.expected()[1])
        assert np.array_equal(as_u32(top_b), b.expected()[0]) and np.array_equal(as_u32(cnt_b), b.expected()[1])


@pytest.mark.gpu
def test_argument_rules(pm, pmo):
    """Part 8."""
    lib = pm._lib.load()
    OK, INVALID = pm._lib.PM_OK, pm._lib.PM_ERR_INVALID
    with pm.Renderer(0) as r:
        top = np.full((8, 8), UNTOUCHED, np.uint32)
        cnt = np.full((8, 8), UNTOUCHED, np.uint32)
        host = lambda *a: lib.pm_hit_frame(r._h, *a)                  # noqa: E731  (x0, y0, w, h, flags, top, n_hit, stride)
        dev = lambda *a: lib.pm_hit_frame_device(r._h, *a, None)      # noqa: E731
        tp, cp = top.ctypes.data, cnt.ctypes.data
        for call in (host, dev):
            assert call(0, 0, 4, 4, 0, tp, cp, 8) == INVALID           # no scene: what pm_hit_test says
        r.set_scene_bytes(pmo.scene_path_test())
        for call in (host, dev):
            assert call(0, 0, 4, 4, 2, tp, cp, 8) == INVALID           # unknown flag bits
            assert call(0, 0, 4, 4, 0x80000001, tp, cp, 8) == INVALID
            assert call(65533, 0, 4, 4, 0, tp, cp, 8) == INVALID       # x0 + w > 65 536
            assert call(0, 65533, 4, 4, 0, tp, cp, 8) == INVALID       # y0 + h > 65 536
            assert call(0xFFFFFFFF, 0, 2, 2, 0, tp, cp, 8) == INVALID  # (no wrap-around in 32 bits)
            assert call(0, 0, 2, 0xFFFFFFFF, 0, tp, cp, 8) == INVALID
            assert call(0, 0, 4, 4, 0, tp, cp, 3) == INVALID           # stride < w
            assert call(0, 0, 4, 4, 0, None, cp, 8) == INVALID         # no top_item
            assert call(0, 0, 0, 4, 0, tp, cp, 8) == OK                # nothing to do
            assert call(0, 0, 4, 0, 0, tp, cp, 8) == OK
            assert call(0, 0, 0, 0, 0, None, None, 0) == OK
            r.sync()
            assert (top == UNTOUCHED).all() and (cnt == UNTOUCHED).all()
        assert host(65532, 65532, 4, 4, 1, tp, None, 8) == OK          # the last pixels there are
        assert (top[:4, :4] == NONE).all() and (top[4:] == UNTOUCHED).all() and (top[:, 4:] == UNTOUCHED).all() and (cnt == UNTOUCHED).all()
        assert lib.pm_abi_version() == 600
        # the Python wrappers
        with pytest.raises(ValueError):
            r.hit_frame(0, 0, 65537, 1)
        with pytest.raises(ValueError):
            r.hit_frame(-1, 0, 4, 4)
        with pytest.raises(TypeError):
            r.hit_frame(0.5, 0, 4, 4)
        assert r.hit_frame(3, 3, 0, 5).shape == (5, 0)
        if not _emulated():
            import torch

            t = torch.full((8, 8), UNTOUCHED, dtype=torch.int32, device="cuda")
            with pytest.raises(TypeError):
                r.hit_frame_tensor(torch.zeros((8, 8), dtype=torch.int32))             # not on the device
            with pytest.raises(TypeError):
                r.hit_frame_tensor(torch.zeros((8, 8), dtype=torch.float32, device="cuda"))
            with pytest.raises(TypeError):
                r.hit_frame_tensor(torch.zeros((8, 8), dtype=torch.int64, device="cuda"))
            with pytest.raises(TypeError):
                r.hit_frame_tensor(t.reshape(-1))                                      # not 2-D
            with pytest.raises(ValueError):
                r.hit_frame_tensor(t[:, ::2])                                          # rows not of unit stride
            with pytest.raises(ValueError):
                r.hit_frame_tensor(t, t[:4])                                           # n_hit of another shape
            with pytest.raises(ValueError):
                r.hit_frame_tensor(t, torch.zeros((8, 16), dtype=torch.int32, device="cuda")[:, :8])   # ... of another row stride
            with pytest.raises(ValueError):
                r.hit_frame_tensor(t, x0=65530)
            r.hit_frame_tensor(t[2:6, 1:5], x0=12, y0=12)                              # a view into a larger tensor
            r.sync()
            got = as_u32(t)
            assert np.array_equal(got[2:6, 1:5], r.hit_frame(12, 12, 4, 4)) and (got[:2] == UNTOUCHED).all() and (got[:, 5:] == UNTOUCHED).all()


@pytest.mark.gpu
def test_cli_item_map_saves_the_map_of_the_view(pm, tmp_path, capsys):
    """Part 9."""
    from piet_metal_amd import cli

    out = tmp_path / "map.npy"
    assert cli.main(["tiger", str(tmp_path / "t.png"), "--width", "160", "--height", "90", "--item-map", str(out)]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    got = np.load(out)
    wl = pm.workloads.tiger(160, 90)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        want = r.hit_frame(0, 0, 160, 90)
    assert got.dtype == np.uint32 and got.shape == (90, 160) and np.array_equal(got, want)
    none = int((want == NONE).sum())
    visible = len(set(want.ravel().tolist()) - {NONE})
    assert none > 0 and visible > 20
    assert lines == [f"{out}: {visible} items visible, {none} pixels with no item"]


# ---- CPU: no blind cases (np_hit alone) ------------------------------------------------------------------------------------

def test_structural_constants_are_the_kernels():
    """A retuned kernel must move these tests with it: the constants are read from pm_hit_frame.h, and the walk and the rounds there
    are written in terms of them."""
    text = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_hit_frame.h")).read()
    assert fc.kernel_constants() == {"kFrameTile": 16, "kFrameItems": fc.ITEMS_PER_STEP, "kFrameChunks": fc.CHUNKS_PER_ROUND}
    assert "hi > kFrameItems ? hi - kFrameItems : 0u" in text and "gb += kFrameChunks" in text and "cb1 - cb0 <= kFrameChunks" in text
    assert "sb += kFrameSupers" in text and "kFrameSupers = kFrameChunks / kSuperChunks" in text
    assert fc.WALK_SIZES == (fc.ITEMS_PER_STEP - 1, fc.ITEMS_PER_STEP, fc.ITEMS_PER_STEP + 1, 2 * fc.ITEMS_PER_STEP + 1)


def test_no_geometry_window_is_blind(pm, pmo):
    wins = fc.geometry_windows(pm, pmo)
    assert sorted(w.ident for w in wins) == sorted(GEOMETRY_IDS)
    for w in wins:
        top = w.expected()[0]
        if w.facts.get("single") or w.facts.get("covered"):
            continue
        assert fc.not_blind(top, w.facts.get("items", 2)), w
        assert w.ident.endswith("origin") or (w.rect[0] % 16 and w.rect[1] % 16), w
    for name in fc.REGIONS:   # the 1 x 1 windows, together
        ones = np.array([w.expected()[0][0, 0] for w in wins if w.ident.startswith(f"{name}-1x1")])
        assert fc.not_blind(ones, fc.ITEMS_WANTED[name]), (name, ones)
    covered = [w for w in wins if w.facts.get("covered")]
    assert [w.ident for w in covered] == ["edge-48x40-origin"] and (covered[0].expected()[0] == 0).all()
    by = {w.ident: w for w in wins}
    assert fc.not_blind(by["edge-ends-at-65536"].expected()[0], 2) and fc.not_blind(by["mixed-48x40-origin"].expected()[0], 2)
    # the saturated edges are there: boxes at 0 and at 65 535
    boxes = np.array([b for _, b in np_hit.flat_items(bytes(by["edge-72x64-origin"].scene))])
    assert (boxes[:, :2] == 0).any() and (boxes[:, 2] == 65535).sum() >= 2


@pytest.mark.parametrize("n", fc.WALK_SIZES)
def test_the_walk_scenes_are_what_they_claim(pm, n):
    wdw = fc.walk_window(pm, n)
    top, cnt = wdw.expected()
    tops, _ = wdw.expected(True)
    assert len(np_hit.flat_items(bytes(wdw.scene))) == n
    assert fc.not_blind(top) and set(range(n)) <= set(top.ravel().tolist())      # every item is the top of some pixel
    assert {"fill", "compound", "polyline", "line", "circle", "ellipse"} <= set(wdw.facts["kinds"])
    T = fc.TILE
    # the first tile is wholly covered by the last opaque item (and, in its lower rows, by the alpha-0 Fill above it): done at step
    # one; in its neighbour some pixel shows item 0, and every tile over the grid has pixels whose top the skip changes
    assert set(top[:T, :T].ravel().tolist()) == {n - 2, n - 1} and (tops[:T, :T] == n - 2).all()
    assert (top[:T, T : 2 * T] == 0).any() and (cnt[:T, T : 2 * T][top[:T, T : 2 * T] == 0] == 1).all()
    gw, gh = wdw.rect[2] - 8, wdw.rect[3] - 6
    for ty in range(0, gh, T):
        for tx in range(0, gw, T):
            a, b = top[ty : ty + T, tx : tx + T], tops[ty : ty + T, tx : tx + T]
            assert (a == n - 1).any() and (b[a == n - 1] != n - 1).all() and (b != a).sum() >= (a == n - 1).sum(), (tx, ty)
    assert (top[:, gw:] == NONE).all() and (top[gh:] == NONE).all()


@pytest.mark.parametrize("ident", fc.LONG_IDS)
def test_no_round_is_blind(pm, ident):
    """In the strip's first tile every chunk of the long item survives the cull, their number is the one the case names, and the
    chunks of any one round, dropped, change some pixel of the strip; the last tile keeps none of a Fill's."""
    import hit_structure as hs

    wdw = fc.long_window(pm, ident)
    got = fc.rounds_of_first_tile(wdw)
    con, chunks = got["con"], wdw.facts["chunks"]
    assert got["cb1"] - got["cb0"] == chunks and got["keep"].all()
    C = fc.CHUNKS_PER_ROUND
    if chunks <= C:
        assert [len(c) for c in got["rounds"]] == [chunks]
    else:   # (a first chunk at residue 3 or 4 of a super-chunk: the first round of 32 super-chunks holds 8 - residue chunks fewer)
        res = got["cb0"] % hs.SUPER_CHUNKS
        assert res != 0 and got["cb1"] % hs.SUPER_CHUNKS != 0    # first and last super-chunk shared with the neighbours
        sizes = [len(c) for c in got["rounds"]]
        assert sizes[0] == C - res and all(s == C for s in sizes[1:-1]) and sum(sizes) == chunks and len(sizes) == -(-(chunks + res) // C)
    for k, c in enumerate(got["rounds"]):
        assert con.changed_by(con.per_chunk[:, c].sum(axis=1)).any(), (wdw, "round", k)
    assert fc.not_blind(wdw.expected()[0])
    if con.fill:
        _, chunk_bbox, _ = hs.index_model(wdw.scene)
        last = fc.tile_extent(wdw.rect, wdw.rect[2] // fc.TILE - 1, 0)
        assert not fc.tile_pass(con, chunk_bbox[got["cb0"] : got["cb1"]], last).any()


def test_the_centres_scene_has_every_class(pm):
    wdw = fc.centres_window(pm)
    got = fc.centre_classes(wdw.scene, wdw.rect)
    assert all(v >= 3 for v in got.values()), got
    top, cnt = wdw.expected()
    assert fc.not_blind(top) and set(range(8)) <= set(top.ravel().tolist()) and cnt.max() >= 2
    # centres exactly at hw are hits, the rim is inside, and a.y <= y < b.y: the L's top row of centres is inside, its bottom row is not
    sc, (x0, y0, _, _) = wdw.scene, wdw.rect
    assert np_hit.item_inside(sc, 0, [[5.5, 4.5]])[0] and not np_hit.item_inside(sc, 0, [[5.5, 16.5]])[0]
    assert np_hit.item_inside(sc, 4, [[30.5, 29.5]])[0] and np_hit.item_inside(sc, 5, [[10.5, 36.5]])[0]
    assert np_hit.item_inside(sc, 6, [[52.5, 11.5]])[0] and not np_hit.item_inside(sc, 6, [[53.5, 10.5]])[0]


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_hit_frame_under_wave64_emulation(built):
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

def test_the_item_map_kernel_uses_no_scratch(tmp_path):
    """pm_hit_frame_kernel by the flags the library is built with: no private segment (nothing spilled, no indexed local array), and
    VGPRs within what its launch bound can be given -- a workgroup of 256 threads puts one wave on each SIMD of a CU, which has 512
    VGPRs per lane, so any count up to 512 fits; the test holds the kernel to 128, four such workgroups per CU.  The figures are
    printed (pytest -s) and stand in DESIGN.md 4."""
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
        if "pm_hit_frame_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"pm_hit_frame_kernel: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and lds <= 8192, (m.group(1), scratch, vgpr, lds)
    assert found == 1
