"""Point hit testing on the device (pm_hit_test / pm_hit_test_device / pm_item_paths) against tests/np_hit.py, the independent
numpy statement of decision D13: top_item and n_hit must be EQUAL for every query -- no tolerance, no query left out.

The `small` tests are also what tests/test_hit_cpu.py runs against the emulated library on a box without a GPU."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_hit  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


# ---- scenes --------------------------------------------------------------------------------------

def mixed_scene(pm):
    """Nested groups, compound fills under both rules, ellipses, a circle, strokes, an alpha-0 item -- by the Python Encoder.
    Flat paint order: 0 square, 1 ellipse, 2 ring (even-odd), 3 circle, 4 polyline, 5 transparent square, 6 ring (non-zero),
    7 line, 8 pentagram (even-odd), 9 one-point polyline, 10 flat ellipse (ry = 0)."""
    buf = np.zeros(1 << 16, np.uint8)
    e = pm.Encoder(buf)
    sq = lambda x0, y0, s: np.array([[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]], np.float64)  # noqa: E731
    star = np.array([[400 + 90 * np.sin(4 * np.pi * k / 5), 130 - 90 * np.cos(4 * np.pi * k / 5)] for k in range(5)])
    e.begin_group(7)
    e.fill(sq(20.25, 30.5, 200.0), 0x336699FF)
    e.begin_group(4)
    e.ellipse((300.0, 200.0), 120.0, 60.0)
    e.fill_compound([sq(100.5, 100.25, 150.0), sq(140.5, 140.25, 60.0)], 0xAA5500C0, even_odd=True)
    e.begin_group(2)
    e.circle((160.0, 330.0), 45.0)
    e.polyline(np.array([[30.5, 400.25], [200.0, 350.0], [330.75, 420.5], [480.0, 300.0]]), 0x11AA22FF, 9.0)
    e.end_group()
    e.fill(sq(250.0, 40.0, 120.0), 0xFF000000)  # alpha 0
    e.end_group()
    e.fill_compound([sq(300.5, 280.25, 150.0), sq(340.5, 320.25, 60.0)[::-1], sq(350.0, 330.0, 20.0)], 0x2244CCFF)
    e.stroke_line((10.0, 10.0), (500.0, 470.0), 5.0, 0x000000FF)
    e.fill(star, 0x9900CC80, even_odd=True)
    e.polyline(np.array([[60.0, 60.0]]), 0x445566FF, 12.0)
    e.ellipse((100.0, 480.0), 40.0, 0.0)
    e.end_group()
    return buf[: e.bytes_used].copy()


def edge_scene(pm):
    """Items that reach where a u16 box cannot: negative coordinates and beyond 65 535."""
    buf = np.zeros(1 << 14, np.uint8)
    e = pm.Encoder(buf)
    e.begin_group(4)
    e.fill(np.array([[-40.0, -30.0], [60.0, -30.0], [60.0, 50.0], [-40.0, 50.0]]), 0x102030FF)
    e.fill(np.array([[65000.0, -5.0], [70500.0, -5.0], [70500.0, 40.0], [65000.0, 40.0]]), 0x405060FF)
    e.polyline(np.array([[-20.0, 20.0], [-3.0, -9.0], [30.0, -12.0]]), 0x708090FF, 6.0)
    e.stroke_line((65500.0, 100.0), (70100.0, 8.0), 8.0, 0xA0B0C0FF)
    e.end_group()
    return buf[: e.bytes_used].copy()


def scene_vertices_and_segments(scene):
    """Every vertex and every segment (a, b) of the scene's Fill, Polyline and Line items, float32."""
    sc = bytes(scene)
    verts, seg_a, seg_b = [], [], []
    for at, _ in np_hit.flat_items(sc):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        if tag == np_hit.FILL:
            pts = np_hit._points(sc, at)
            a, b = np_hit.fill_segments(pts, bool(struct.unpack_from("<I", sc, at + 4)[0] & np_hit.FILL_COMPOUND))
            verts.append(pts)
        elif tag in (np_hit.LINE, np_hit.POLY):
            a, b, _ = np_hit.stroke_segments(sc, at, tag)
            verts.append(np.concatenate([a[:1], b]).astype(np.float32))
        else:
            continue
        seg_a.append(a)
        seg_b.append(b)
    if not verts:
        return np.zeros((0, 2), np.float32), np.zeros((0, 2)), np.zeros((0, 2))
    return np.concatenate(verts), np.concatenate(seg_a), np.concatenate(seg_b)


def make_queries(scene, width, height, n_uniform, seed):
    """Uniform points over the viewport, every 97th scene vertex verbatim, the midpoint of every 89th segment, points outside the
    viewport on all four sides (near and far beyond what a u16 holds), and a few non-finite points."""
    rng = np.random.default_rng(seed)
    verts, a, b = scene_vertices_and_segments(scene)
    uni = rng.uniform(0.0, 1.0, (n_uniform, 2)) * (width, height)
    out_n = max(n_uniform // 50, 16)
    t = rng.uniform(0.0, 1.0, (4, out_n, 2))
    outside = np.concatenate([
        t[0] * (width + 400.0, 300.0) - (200.0, 300.0),          # above
        t[1] * (width + 400.0, 300.0) + (-200.0, float(height)),  # below
        t[2] * (300.0, height + 400.0) - (300.0, 200.0),         # left
        t[3] * (300.0, height + 400.0) + (float(width), -200.0),  # right
        np.array([[-5.0, -5.0], [70000.0, 10.0], [-1.0e6, 20.0], [65535.5, 20.5], [66000.0, -3.0], [3.0e9, 3.0e9]]),
    ])
    bad = np.array([[np.nan, 10.0], [10.0, np.nan], [np.inf, 10.0], [10.0, -np.inf], [np.nan, np.nan], [-np.inf, np.inf]])
    mids = (a[::89] + b[::89]) * 0.5
    return np.concatenate([uni, verts[::97].astype(np.float64), mids, outside, bad]).astype(np.float32)


def check_against_np_hit(r, scene, q, skip_transparent=False, brute_sample=0):
    want_top, want_cnt = np_hit.hit_test(scene, q, skip_transparent)
    top, cnt = r.hit_test(q, skip_transparent=skip_transparent, counts=True)
    bad = np.flatnonzero((top != want_top) | (cnt != want_cnt))
    assert bad.size == 0, (bad.size, [(q[k].tolist(), int(top[k]), int(want_top[k]), int(cnt[k]), int(want_cnt[k])) for k in bad[:8]])
    assert np.array_equal(r.hit_test(q, skip_transparent=skip_transparent), want_top)  # the walk that ends at the first hit
    if brute_sample:  # np_hit's two evaluation orders on a sample: every (query, segment) pair, nothing sorted
        sub = np.random.default_rng(7).choice(len(q), min(brute_sample, len(q)), replace=False)
        bt, bc = np_hit.hit_test(scene, q[sub], skip_transparent, brute=True)
        assert np.array_equal(bt, want_top[sub]) and np.array_equal(bc, want_cnt[sub])
    return want_top, want_cnt


def device_hit(r, q, counts=True, stream=None):
    import torch

    xy = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    top = torch.full((len(q),), 0x7EADBEEF, dtype=torch.int32, device="cuda")
    cnt = torch.full((len(q),), 0x7EADBEEF, dtype=torch.int32, device="cuda") if counts else None
    r.hit_test_tensor(xy, top, cnt, stream=stream)
    return xy, top, cnt


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- small cases (also run under emulation) ------------------------------------------------------------

@pytest.mark.parametrize("which", ["mixed", "edge", "path_test"])
def test_hit_small_uploaded_scenes(pm, pmo, which):
    scene = {"mixed": lambda: mixed_scene(pm), "edge": lambda: edge_scene(pm), "path_test": pmo.scene_path_test}[which]()
    q = make_queries(scene, 512, 512, 300, seed=11)
    if which == "edge":
        q = np.concatenate([q, np.array([[-5.0, -5.0], [70000.0, 10.0], [-10.0, 5.0], [67000.0, 60.0]], np.float32)])
    with pm.Renderer(0) as r:  # (never resized: hit testing needs a scene, not a viewport)
        r.set_scene_bytes(scene)
        for skip in (False, True):
            want_top, want_cnt = check_against_np_hit(r, scene, q, skip_transparent=skip, brute_sample=len(q))
        if which == "mixed":
            assert r.stats()["n_items"] == 11 and want_cnt.max() >= 2
            assert r.hit_test(np.array([[300.0, 100.0]], np.float32))[0] == 5  # the alpha-0 square is the top item there ...
            assert r.hit_test(np.array([[300.0, 100.0]], np.float32), skip_transparent=True)[0] != 5  # ... unless it is skipped
        if which == "edge":
            t = r.hit_test(np.array([[-5.0, -5.0], [70000.0, 30.0], [70000.0, 10.0]], np.float32))
            assert t.tolist() == [2, 1, 3]  # the polyline over the first fill; the second fill out at x = 70 000, and the line over it


def test_hit_small_flattened_scene_and_item_paths(pm, pmo):
    """A device-flattened scene with a long outline (more than 64 chunks: the super-chunk level), re-flattened; pm_item_paths."""
    wl = pm.workloads.tiger(160, 90)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        q = make_queries(scene, wl.width, wl.height, 250, seed=12)
        check_against_np_hit(r, scene, q, brute_sample=120)
        want_paths = oracle_item_paths(pmo, wl, wl.affine)
        assert np.array_equal(r.item_paths(), want_paths)
        aff = (0.35, 0.2, -0.2, 0.35, 60.0, 5.0)
        r.reflatten(aff, wl.width_scale)
        scene2 = r.download_scene()
        assert not np.array_equal(scene, scene2)
        check_against_np_hit(r, scene2, q)
        assert np.array_equal(r.item_paths(), want_paths)
        r.set_scene_bytes(pmo.scene_path_test())
        with pytest.raises(pm._lib.PietMetalError) as ei:
            r.item_paths()
        assert ei.value.status == pm._lib.PM_ERR_INVALID


def test_hit_small_argument_rules(pm, pmo):
    import ctypes as C

    lib = pm._lib.load()
    with pm.Renderer(0) as r:
        top = np.zeros(4, np.uint32)
        xy = np.zeros((4, 2), np.float32)
        # no scene: what pm_render says
        assert lib.pm_hit_test(r._h, xy.ctypes.data, 4, 0, top.ctypes.data, None) == pm._lib.PM_ERR_INVALID
        assert lib.pm_render(r._h) == pm._lib.PM_ERR_INVALID
        n = C.c_uint32(7)
        assert lib.pm_item_paths(r._h, None, 0, C.byref(n)) == pm._lib.PM_ERR_INVALID and n.value == 0
        r.set_scene_bytes(pmo.scene_path_test())
        assert lib.pm_hit_test(r._h, None, 0, 0, None, None) == pm._lib.PM_OK
        assert lib.pm_hit_test_device(r._h, None, 0, 0, None, None, None) == pm._lib.PM_OK
        assert lib.pm_hit_test(r._h, xy.ctypes.data, 4, 2, top.ctypes.data, None) == pm._lib.PM_ERR_INVALID
        assert lib.pm_hit_test(r._h, xy.ctypes.data, 4, 0x80000001, top.ctypes.data, None) == pm._lib.PM_ERR_INVALID
        assert lib.pm_hit_test_device(r._h, xy.ctypes.data, 4, 4, top.ctypes.data, None, None) == pm._lib.PM_ERR_INVALID
        assert lib.pm_hit_test(r._h, xy.ctypes.data, 4, 1, top.ctypes.data, None) == pm._lib.PM_OK
        assert lib.pm_abi_version() == 600


# ---- the full cases ----------------------------------------------------------------------------------------

def oracle_item_paths(pmo, wl, affine):
    """path_of_item from the oracle: every path encoded alone, its item count accumulated."""
    paths = pmo.scaled_paths(wl.paths.paths, wl.width_scale)
    out = []
    for i in range(len(paths)):
        one = paths[i : i + 1].copy()
        els = wl.paths.els[int(one["el_begin"][0]) : int(one["el_end"][0])]
        one["el_end"] -= one["el_begin"]
        one["el_begin"] = 0
        _, n = pmo.scene_from_paths(one, els, affine, cap=1 << 20)
        out += [i] * n
    return np.array(out, np.uint32)


SCENES = ["cardioid", "path_test", "tiger_1080", "blobs_2000", "glyphs", "mixed"]


def load_scene(pm, pmo, r, name):
    """Makes `name` resident in r; returns (the scene bytes np_hit reads, width, height)."""
    if name in ("cardioid", "path_test", "mixed"):
        scene = {"cardioid": pmo.scene_cardioid, "path_test": pmo.scene_path_test, "mixed": lambda: mixed_scene(pm)}[name]()
        r.set_scene_bytes(scene)
        return scene, 1024, 768
    wl = {"tiger_1080": lambda: pm.workloads.tiger(1920, 1080), "blobs_2000": lambda: pm.workloads.config4_blobs(2000, 2048),
          "glyphs": lambda: pm.workloads.heldout_glyphs(4000, 1920, 1080)}[name]()
    r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
    return r.download_scene(), wl.width, wl.height


@pytest.mark.parametrize("name", SCENES)
def test_hit_test_equals_np_hit(pm, pmo, name):
    """>= 100 000 seeded queries per scene, host and device variants, before any resize and across viewport changes."""
    with pm.Renderer(0) as r:
        scene, w, h = load_scene(pm, pmo, r, name)
        q = make_queries(scene, w, h, 100_000, seed=100 + SCENES.index(name))
        assert len(q) >= 100_000
        want_top, want_cnt = check_against_np_hit(r, scene, q, brute_sample=1500)  # (never resized so far)
        if name == "mixed":
            check_against_np_hit(r, scene, q, skip_transparent=True)
        _, top, cnt = device_hit(r, q)
        r.sync()
        assert np.array_equal(as_u32(top), want_top) and np.array_equal(as_u32(cnt), want_cnt)
        _, top1, _ = device_hit(r, q, counts=False)
        r.sync()
        assert np.array_equal(as_u32(top1), want_top)
        # independent of the viewport, the band and the target format
        r.resize(w, h)
        assert np.array_equal(r.hit_test(q), want_top)
        r.set_band(1, 3)
        r.set_target_format(True)
        r.render()
        t2, c2 = r.hit_test(q, counts=True)
        assert np.array_equal(t2, want_top) and np.array_equal(c2, want_cnt)
        r.resize(64, 48)
        r.sync()
        assert np.array_equal(r.hit_test(q), want_top)


def test_hit_test_after_reflatten_and_while_the_scene_is_replaced(pm, pmo):
    import torch

    wl = pm.workloads.tiger(1920, 1080)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene0 = r.download_scene()
        ys, xs = np.mgrid[0 : wl.height : 2, 0 : wl.width : 2]
        q = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)  # 518 400 pixel centres
        want0 = np_hit.hit_test(scene0, q)
        aff1 = (4.0, 1.5, -1.5, 4.0, 700.0, -100.0)
        aff2 = (2.0, 0.0, 0.0, 2.0, 100.0, 300.0)
        # the device variant on a stream of the caller's, then at once two scene replacements: the answers are the first scene's
        s = torch.cuda.Stream()
        xy, top, cnt = device_hit(r, q, stream=s)
        r.reflatten(aff1, wl.width_scale)
        r.reflatten(aff2, wl.width_scale)
        r.sync()
        s.synchronize()
        assert np.array_equal(as_u32(top), want0[0]) and np.array_equal(as_u32(cnt), want0[1])
        # ... and the resident scene is the last one
        scene2 = r.download_scene()
        qs = make_queries(scene2, wl.width, wl.height, 100_000, seed=5)
        check_against_np_hit(r, scene2, qs)
        r.reflatten(aff1, wl.width_scale)
        check_against_np_hit(r, r.download_scene(), qs)


def test_item_paths_of_the_tiger(pm, pmo):
    wl = pm.workloads.tiger(1920, 1080)
    want = oracle_item_paths(pmo, wl, wl.affine)
    with pm.Renderer(0) as r:
        _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        got = r.item_paths()
        assert len(got) == n_items and np.array_equal(got, want)
        r.reflatten((3.0, 0.5, -0.5, 3.0, 200.0, 10.0), wl.width_scale)
        assert np.array_equal(r.item_paths(), want)
        r.set_scene_bytes(pmo.scene_cardioid())
        with pytest.raises(pm._lib.PietMetalError) as ei:
            r.item_paths()
        assert ei.value.status == pm._lib.PM_ERR_INVALID


def test_hit_tests_between_frames_leave_the_frames_alone(pm, pmo):
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want = pmo.render(scene, wl.width, wl.height)
        q = make_queries(scene, wl.width, wl.height, 20_000, seed=3)
        r.render()
        _, top, _ = device_hit(r, q, counts=False)  # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        top_host = r.hit_test(q)
        second = r.read_pixels()
        assert np.array_equal(first, want) and np.array_equal(second, want)
        assert np.array_equal(as_u32(top), top_host) and np.array_equal(top_host, np_hit.hit_test(scene, q)[0])


def test_cli_pick_prints_item_and_path(pm, tmp_path, capsys):
    from piet_metal_amd import cli

    picks = [(240.0, 135.0), (3.0, 3.0), (200.5, 100.5), (260.25, 190.75)]
    args = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270"]
    for x, y in picks:
        args += ["--pick", f"{x:g},{y:g}"]
    assert cli.main(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        top = r.hit_test(np.array(picks, np.float32))
        of_item = r.item_paths()
    want = [f"{x:g},{y:g}: " + ("none" if t == NONE else f"item {int(t)} path {int(of_item[t])}") for (x, y), t in zip(picks, top)]
    assert lines == want
    assert any(ln.endswith("none") for ln in lines) and any("path" in ln for ln in lines)
