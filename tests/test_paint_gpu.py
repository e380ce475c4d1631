"""Per-group paint (decision D17: pm_repaint_groups, the kernels of piet_metal_amd/csrc/pm_paint.h) against tests/np_paint.py and
tests/np_groups.py: the downloaded scene must be EQUAL to the scene D1-D16 define for the painted paths -- the splice of one-path
oracle scenes of `np_paint.painted(...)` under the transforms of the call that made the resident scene -- no tolerance, no case
left out.  Frames are compared with the oracle's rendering of the expected bytes, picking with tests/np_hit.py.  The whole file
also runs against the CPU emulation of the library (PM_TEST_EMU=1)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_hit  # noqa: E402
import np_paint  # noqa: E402
import path_sets  # noqa: E402
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE, style_bits  # noqa: E402
from path_sets import COMPOUND, FILL, STROKE, pathset  # noqa: E402
from test_groups_gpu import check_frame, check_scene, expected, group_maps, random_table  # noqa: E402
from test_stroke_gpu import IDENTITY, shapes  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = -1


# ---- helpers ---------------------------------------------------------------------------------------------

def identity_table(n_groups):
    return np.zeros(n_groups, np.uint32), np.full(n_groups, 255, np.uint32)


def random_paints(rng, n_groups):
    tints = (rng.integers(0, 1 << 24, n_groups).astype(np.uint32) << np.uint32(8)) | rng.integers(0, 256, n_groups).astype(np.uint32)
    return tints, rng.integers(0, 256, n_groups).astype(np.uint32)


def extreme_paints(rng, n_groups):
    """Opacity 0 / 1 / 254 / 255 and tint AA 0 / 128 / 255 in turn (from a random start), random tint colours."""
    o = np.array([0, 1, 254, 255], np.uint32)[(np.arange(n_groups) + int(rng.integers(0, 4))) % 4]
    aa = np.array([0, 128, 255], np.uint32)[(np.arange(n_groups) + int(rng.integers(0, 3))) % 3]
    return (rng.integers(0, 1 << 24, n_groups).astype(np.uint32) << np.uint32(8)) | aa, o


def tables(rng, n_groups):
    return {"identity": identity_table(n_groups), "random": random_paints(rng, n_groups), "extremes": extreme_paints(rng, n_groups)}


def want_painted(pmo, ps, gmap, tints, opacities, aff, ws):
    """The expected scene: np_groups.scene of the painted set (through test_groups_gpu.expected, which names the oracle)."""
    return expected(pmo, np_paint.painted(ps, gmap, tints, opacities), gmap, aff, ws)


def uniform(case_affine, scale, n_groups):
    return [case_affine] * n_groups, [scale] * n_groups


# ---- 1. scene and frame parity -------------------------------------------------------------------------------

SEEDS = [500, 501, 502, 503]


@pytest.mark.parametrize("grouped", [False, True], ids=["uniform", "behind-reflatten-groups"])
@pytest.mark.parametrize("seed", SEEDS)
def test_paint_scene_and_frame_parity(pm, pmo, seed, grouped):
    """Random path sets x the four group maps x three paint tables, on the scene flatten_and_encode made and on the one a grouped
    re-flatten made: bytes, item count, item_paths and the frame."""
    case = path_sets.random_case(seed)
    ps = case.ps
    with pm.Renderer(0) as r:
        r.resize(case.width, case.height)
        _, n_items0 = r.flatten_and_encode(ps, case.affine, case.scale)
        paths0 = r.item_paths()
        for name, gmap in group_maps(len(ps.paths)).items():
            n_groups = int(gmap.max()) + 1
            rng = np.random.default_rng(seed * 37 + len(name))
            r.set_path_groups(gmap)
            if grouped:
                aff, ws = random_table(rng, n_groups)
                r.reflatten_groups(aff, ws)
            else:  # (the scene flatten_and_encode made: repaints leave its geometry alone)
                aff, ws = uniform(case.affine, case.scale, n_groups)
            for tname, (tints, opac) in tables(rng, n_groups).items():
                r.repaint_groups(opac, tints)
                want = want_painted(pmo, ps, gmap, tints, opac, aff, ws)
                assert want[1] == n_items0 == r.stats()["n_items"] and np.array_equal(want[2], paths0), (seed, name, tname)
                check_scene(r, want)
                r.render()
                check_frame(pmo, r, want[0], case.width, case.height)


# ---- 2. styles and dashes ------------------------------------------------------------------------------------

def styled_set():
    """The page of strokes with styles and dash patterns; path 1 (one sub-path) and path 9 (two) have a compound fill under their
    stroke, path 9's stroke is dashed [0, 6]: an item of 0 entries with butt caps."""
    def flags_of(cap, join):
        return lambda k: ((FILL | STROKE | COMPOUND) if k in (1, 9) else (3 if k % 4 == 0 else 2)) | style_bits(cap, join)

    def build(cap, join):
        ps = shapes(flags_of(cap, join))
        return ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5]).with_dashes([0, 6], 1.0, select=[9])

    return build


@pytest.mark.parametrize("cap,join", [(BUTT, MITER), (ROUND_CAP, ROUND_JOIN), (SQUARE, BEVEL)], ids=["butt-miter", "round-round", "square-bevel"])
def test_paint_styles_and_dashes(pm, pmo, cap, join):
    """Three groups with their own width_scale: 6 * 0.05 is below the thin-line width (painted alphas go through the thin-line rule,
    on outline and dashed items), 6 * 1 and 6 * 2.5 above.  Then the same paints on the uniform scene below the thin-line width."""
    ps = styled_set()(cap, join)
    gmap = np.arange(len(ps.paths), dtype=np.uint32) % 3
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 4.0, 2.0), (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), (0.9, 0.0, 0.0, -0.9, 10.0, 170.0)])
    ws = np.array([0.05, 1.0, 2.5], np.float32)
    rng = np.random.default_rng(70 + cap * 3 + join)
    with pm.Renderer(0) as r:
        r.resize(192, 176)
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        r.reflatten_groups(aff, ws)
        for tints, opac in (random_paints(rng, 3), extreme_paints(rng, 3), (np.array([0x10203040, 0, 0xFFFFFFFF], np.uint32), np.array([200, 77, 255], np.uint32))):
            r.repaint_groups(opac, tints)
            want = want_painted(pmo, ps, gmap, tints, opac, aff, ws)
            check_scene(r, want)
            r.render()
            check_frame(pmo, r, want[0], 192, 176)
        r.reflatten(IDENTITY, 0.05)  # (keeps the paint; every stroke below the thin-line width)
        tints, opac = random_paints(rng, 3)
        r.repaint_groups(opac, tints)
        check_scene(r, want_painted(pmo, ps, gmap, tints, opac, [IDENTITY] * 3, [0.05] * 3))


# ---- 3. no accumulation, and the identity ---------------------------------------------------------------------

def test_paint_identity_and_no_accumulation(pm, pmo):
    case = path_sets.random_case(510)
    ps, n = case.ps, len(case.ps.paths)
    gmap = np.arange(n, dtype=np.uint32) % 3
    g = int(gmap.max()) + 1
    rng = np.random.default_rng(3)
    p1, p2 = random_paints(rng, g), random_paints(rng, g)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), case.affine, case.scale)
        before = r.download_scene()
        r.repaint_groups(*identity_table(g)[::-1])
        assert np.array_equal(r.download_scene(), before)
        r.repaint_groups(None, np.zeros(g, np.uint32))  # (None: the identity of that field)
        assert np.array_equal(r.download_scene(), before)
        r.repaint_groups(p2[1], p2[0])
        alone = r.download_scene()
        assert not np.array_equal(alone, before)
        r.repaint_groups(p1[1], p1[0])
        r.repaint_groups(p2[1], p2[0])
        assert np.array_equal(r.download_scene(), alone)
        check_scene(r, want_painted(pmo, ps, gmap, p2[0], p2[1], *uniform(case.affine, case.scale, g)))
        r.repaint_groups(np.full(g + 5, 255, np.uint32))  # (a longer table is fine)
        assert np.array_equal(r.download_scene(), before)


# ---- 4. lifetime ------------------------------------------------------------------------------------------------

def test_paint_stays_with_the_paths_until_new_paths_come(pm, pmo):
    case = path_sets.random_case(511)
    ps, n = case.ps, len(case.ps.paths)
    gmap = np.arange(n, dtype=np.uint32) % 4
    g = int(gmap.max()) + 1
    rng = np.random.default_rng(4)
    tints, opac = random_paints(rng, g)
    aff, ws = random_table(rng, g)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), case.affine, case.scale)
        unpainted = r.download_scene()
        # paint, then move the groups == move the groups, then paint
        r.repaint_groups(opac, tints)
        a = r.reflatten_groups(aff, ws)
        first = r.download_scene()
        r.repaint_groups(*identity_table(g)[::-1])
        b = r.reflatten_groups(aff, ws)
        r.repaint_groups(opac, tints)
        assert a == b and np.array_equal(r.download_scene(), first)
        check_scene(r, want_painted(pmo, ps, gmap, tints, opac, aff, ws))
        # the same with the uniform re-flatten
        a = r.reflatten(case.affine2, 0.75)
        first = r.download_scene()
        r.repaint_groups(*identity_table(g)[::-1])
        b = r.reflatten(case.affine2, 0.75)
        r.repaint_groups(opac, tints)
        assert a == b and np.array_equal(r.download_scene(), first)
        check_scene(r, want_painted(pmo, ps, gmap, tints, opac, *uniform(case.affine2, 0.75, g)))
        # a new map does not touch the paint: the colours are those of the old map's groups until the next paint
        r.set_path_groups(np.zeros(n, np.uint32))
        r.reflatten(case.affine, case.scale)
        check_scene(r, want_painted(pmo, ps, gmap, tints, opac, *uniform(case.affine, case.scale, g)))
        # new paths bring their own colours
        r.flatten_and_encode(ps.with_groups(gmap), case.affine, case.scale)
        assert np.array_equal(r.download_scene(), unpainted)
        r.reflatten(case.affine, case.scale)
        assert np.array_equal(r.download_scene(), unpainted)


# ---- 5. the fast path is one ---------------------------------------------------------------------------------

def test_paint_keeps_the_plan_and_the_index(pm, pmo):
    case = path_sets.random_case(512)
    ps, n = case.ps, len(case.ps.paths)
    gmap = np.arange(n, dtype=np.uint32) % 2
    tints, opac = random_paints(np.random.default_rng(5), 2)
    with pm.Renderer(0) as r:
        r.resize(case.width, case.height)
        r.flatten_and_encode(ps.with_groups(gmap), case.affine, case.scale)
        r.render()
        r.sync()
        t0, s0 = r.scene_timings(), r.stats()
        assert t0["scene_index_ms"] > 0
        r.repaint_groups(opac, tints)
        r.render()
        r.sync()
        t1, s1 = r.scene_timings(), r.stats()
        assert t1["binning_plans"] == t0["binning_plans"], (t0, t1)
        assert t1["scene_index_ms"] == 0 and t1["flatten_encode_ms"] > 0
        assert (s1["n_items"], s1["scene_bytes"]) == (s0["n_items"], s0["scene_bytes"])
        want = want_painted(pmo, ps, gmap, tints, opac, *uniform(case.affine, case.scale, 2))
        check_scene(r, want)
        check_frame(pmo, r, want[0], case.width, case.height)


# ---- 6. lists that grow under an unchanged plan -----------------------------------------------------------------

def test_paint_tile_lists_grow_and_shrink_under_one_plan(pm, pmo):
    """48 opaque squares over the same 2 x 2 tiles, a group each: opaque, every tile's list is the top square alone; at opacity
    128 all 48 are on it; opaque again, one."""
    n = 48
    ps = pathset(*[(path_sets._square(0, 0, 32), FILL) for _ in range(n)])
    ps.paths["fill_rgba"] |= 0xFF
    gmap = np.arange(n, dtype=np.uint32)
    aff, ws = uniform(IDENTITY, 1.0, n)
    with pm.Renderer(0) as r:
        r.resize(64, 64)
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        r.render()
        r.sync()
        plans = r.scene_timings()["binning_plans"]
        for step, o in enumerate((255, 128, 255)):
            opac = np.full(n, o, np.uint32)
            r.repaint_groups(opac)
            r.render()
            r.sync()
            want = want_painted(pmo, ps, gmap, None, opac, aff, ws)
            got = r.read_pixels()
            bad = int((got != pmo.render(want[0], 64, 64)).any(axis=2).sum())
            assert bad == 0, f"step {step} (opacity {o}): {bad} pixels differ; stats().overflow = {r.stats()['overflow']}"
            check_scene(r, want)
        assert r.scene_timings()["binning_plans"] == plans


# ---- 7. frames in flight ----------------------------------------------------------------------------------------

def test_paint_with_frames_in_flight(pm, pmo):
    """Six repaints, each followed by three frames into buffers of their own, nothing waited for in between (a repaint writes the
    other scene buffer); after one sync every frame is the oracle's rendering of the scene that was current when it was enqueued."""
    import torch

    case = path_sets.random_case(513)
    ps, w, h = case.ps, case.width, case.height
    gmap = np.arange(len(ps.paths), dtype=np.uint32) % 3
    g = int(gmap.max()) + 1
    rng = np.random.default_rng(7)
    on_device = torch.cuda.is_available()  # (the emulated library of a box without a GPU has no device tensors: it reads each frame back)
    frames = []
    with pm.Renderer(0) as r:
        r.resize(w, h)
        r.flatten_and_encode(ps.with_groups(gmap), case.affine, case.scale)
        for _ in range(6):
            tints, opac = random_paints(rng, g)
            r.repaint_groups(opac, tints)
            want = want_painted(pmo, ps, gmap, tints, opac, *uniform(case.affine, case.scale, g))
            for _ in range(3):
                if on_device:
                    t = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
                    r.render_to(t, None)
                    frames.append((t, want[0]))
                else:
                    r.render()
                    check_frame(pmo, r, want[0], w, h)
        r.sync()
        check_scene(r, want)
        rendered = {}
        for k, (t, scene) in enumerate(frames):
            key = scene.tobytes()
            if key not in rendered:
                rendered[key] = pmo.render(scene, w, h)
            bad = int((t.cpu().numpy() != rendered[key]).any(axis=2).sum())
            assert bad == 0, f"frame {k}: {bad} pixels differ from the oracle's rendering of the scene current when it was enqueued"


# ---- 8. picking -------------------------------------------------------------------------------------------------

def test_paint_picking_skips_a_group_faded_out(pm, pmo):
    ps = pathset((path_sets._square(10, 10, 60), FILL), (path_sets._square(30, 30, 40), FILL | STROKE), (path_sets._tri(120, 120), STROKE, 5.0))
    ps.paths["fill_rgba"] |= 0xFF
    gmap = np.array([0, 1, 0], np.uint32)
    q = np.array([(50.5, 50.5), (15.5, 15.5), (150.5, 50.5), (31.0, 31.0), (200.0, 200.0)], np.float32)
    aff, ws = uniform(IDENTITY, 1.0, 2)
    tops = []
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        for opac in ([255, 255], [255, 0]):
            r.repaint_groups(opac)
            want = want_painted(pmo, ps, gmap, None, opac, aff, ws)
            check_scene(r, want)
            for skip in (False, True):
                top, cnt = r.hit_test(q, skip_transparent=skip, counts=True)
                want_top, want_cnt = np_hit.hit_test(want[0], q, skip_transparent=skip)
                assert np.array_equal(top, want_top) and np.array_equal(cnt, want_cnt), (opac, skip)
            tops.append(top)  # (with skip_transparent)
    paths = want[2]
    assert paths[tops[0][0]] == 1 and paths[tops[1][0]] == 0  # group 1 faded out: the square beneath is hit


# ---- 9. arguments ------------------------------------------------------------------------------------------------

def test_paint_invalid_arguments_change_nothing(pm, pmo, monkeypatch):
    lib = pm._lib.load()
    case = path_sets.random_case(514)
    ps, n = case.ps, len(case.ps.paths)
    assert n >= 2
    gmap = np.arange(n, dtype=np.uint32) % 2
    table = np.zeros(2, pm.Renderer.GROUP_PAINT_DTYPE)
    table["tint_rgba"], table["opacity"] = [0x11223344, 0xFF000080], [200, 90]

    def repaint(h, tab, count):
        return lib.pm_repaint_groups(h, tab.ctypes.data if tab is not None else None, count)

    def invalid(status, *words):
        assert status == INVALID
        text = pm._lib.last_error()
        assert all(w in text for w in words), text

    with pm.Renderer(0) as r:
        invalid(repaint(r._h, table, 2), "no paths resident")
        r.resize(case.width, case.height)
        r.flatten_and_encode(ps, case.affine, case.scale)
        r.render()
        frame = r.read_pixels()
        scene = r.download_scene()
        invalid(repaint(r._h, table, 2), "no group map")
        r.set_path_groups(gmap)
        invalid(repaint(r._h, table, 0), "0 paints")
        invalid(repaint(r._h, table, 1), "1 paints", "index 1")
        invalid(repaint(r._h, None, 2), "NULL")
        invalid(repaint(None, table, 2), "NULL")
        bad = table.copy()
        bad["opacity"][1] = 256
        invalid(repaint(r._h, bad, 2), "opacity 256")
        assert np.array_equal(r.download_scene(), scene)
        r.render()
        assert np.array_equal(r.read_pixels(), frame)
        # an uploaded scene is not the resident paths'
        r.set_scene_bytes(scene)
        invalid(repaint(r._h, table, 2), "did not come from the resident paths")
        assert np.array_equal(r.download_scene(), scene)
        r.render()
        assert np.array_equal(r.read_pixels(), frame)
        # ... nor is what a failed replacement left
        r.reflatten(case.affine, case.scale)
        monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", "64")
        nbytes, n_items = C.c_size_t(0), C.c_uint32(0)
        aff = (C.c_double * 6)(*case.affine)
        assert lib.pm_reflatten(r._h, aff, case.scale, C.byref(nbytes), C.byref(n_items)) == pm._lib.PM_ERR_CAPACITY
        monkeypatch.delenv("PM_FLATTEN_SCENE_CAP")
        invalid(repaint(r._h, table, 2), "did not come from the resident paths")
        # nothing of this touched the paths, the map or their colours
        r.reflatten(case.affine, case.scale)
        assert np.array_equal(r.download_scene(), scene)
        assert repaint(r._h, table, 2) == pm._lib.PM_OK
        want = want_painted(pmo, ps, gmap, table["tint_rgba"], table["opacity"], *uniform(case.affine, case.scale, 2))
        check_scene(r, want)
        r.render()
        check_frame(pmo, r, want[0], case.width, case.height)


# ---- 10. the CLI ---------------------------------------------------------------------------------------------------

FADE_SVG = """<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 64 48">
  <g fill="#c03020"><rect x="4" y="4" width="30" height="30"/><circle cx="40" cy="30" r="9" fill-opacity="0.5"/></g>
  <path d="M10 40 L60 8 L56 44 Z" fill="#2040c0" stroke="#102010" stroke-width="2"/>
  <g stroke="#00a040" stroke-width="0.3" fill="none"><path d="M2 2 L62 46"/><path d="M2 46 L62 2"/></g>
</svg>
"""


def test_cli_fade_frames(pm, pmo, tmp_path):
    """--frames 4 --fade: every PNG is the oracle's rendering of the painted scene of its frame; the last one is the background."""
    from piet_metal_amd import cli

    svg = tmp_path / "fade.svg"
    svg.write_text(FADE_SVG)
    n_frames, w, h = 4, 64, 48
    assert cli.main([str(svg), str(tmp_path / "f.png"), "--width", str(w), "--height", str(h), "--frames", str(n_frames), "--fade"]) == 0
    ps = pm.PathSet.from_svg(FADE_SVG, spec_defaults=True, flat_gradients=True, groups=True)
    assert ps.n_groups() == 3
    base, scale = ps.fit_affine(w, h)
    for k in range(n_frames):
        opac = cli.fade_opacities(k, n_frames, 3)
        want = want_painted(pmo, ps, ps.groups, None, opac, *uniform(base, scale, 3))
        got = cli.read_png_rgba(str(tmp_path / f"f-{k:03d}.png"))
        bad = int((got != pmo.render(want[0], w, h)).any(axis=2).sum())
        assert bad == 0, f"frame {k}: {bad} pixels differ"
    assert len(np.unique(got.reshape(-1, 4), axis=0)) == 1  # every group gone


# ---- 11. a new map behind a grouped scene ----------------------------------------------------------------------------

def test_paint_new_map_behind_a_grouped_scene(pm, pmo):
    """pm_path_groups after pm_reflatten_groups: the paint follows the NEW map, the thin-line rule the width_scales the scene was
    made with (the old map's) -- the new map's indices reach beyond the old table."""
    ps = shapes(lambda k: 3 if k % 2 else 2, width=3.0)
    n = len(ps.paths)
    old = np.arange(n, dtype=np.uint32) % 2
    new = np.arange(n, dtype=np.uint32)[::-1].copy()
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 4.0, 2.0), (0.9, 0.0, 0.0, 0.9, 10.0, 12.0)])
    ws = np.array([0.1, 1.5], np.float32)  # 3 * 0.1 is below the thin-line width
    tints, opac = random_paints(np.random.default_rng(11), n)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(old), IDENTITY, 1.0)
        r.reflatten_groups(aff, ws)
        r.set_path_groups(new)
        r.set_path_groups(new)  # (twice: the scene's own map is kept aside once)
        r.repaint_groups(opac, tints)
        check_scene(r, expected(pmo, np_paint.painted(ps, new, tints, opac), old, aff, ws))
        r.reflatten_groups(np.tile(aff[1], (n, 1)), np.full(n, 0.1, np.float32))  # the new map's scene, still painted
        check_scene(r, expected(pmo, np_paint.painted(ps, new, tints, opac), new, np.tile(aff[1], (n, 1)), np.full(n, 0.1, np.float32)))


# ---- 12. coverage of one item after a repaint --------------------------------------------------------------------------

def test_paint_fill_coverage_reads_the_painted_record(pm, pmo):
    """pm_fill_coverage hands one item record back to the device; the host's copy of the records is colour-stale after a repaint.
    Coverage depends on the alpha: a tile an opaque item covers wholly reports 1.0, a translucent one 0.0 (the reference's
    TileEncoder keeps a translucent Solid out of the solid colour)."""
    ps = pathset((path_sets._square(0, 0, 48), FILL), (path_sets._tri(10, 8), FILL | STROKE))
    ps.paths["fill_rgba"] |= 0xFF
    gmap = np.array([0, 1], np.uint32)
    aff, ws = uniform(IDENTITY, 1.0, 2)
    covs = []
    with pm.Renderer(0) as r:
        r.resize(64, 64)
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        for opac in ([255, 255], [128, 255], [255, 255]):
            r.repaint_groups(opac)
            want = want_painted(pmo, ps, gmap, None, opac, aff, ws)
            got = r.fill_coverage(0)
            assert np.array_equal(got, pmo.fill_coverage(want[0], 0, 64, 64)), opac
            covs.append(got)
            check_scene(r, want)  # (the call put everything back)
    assert covs[0][40, 40] == 1.0 and covs[1][40, 40] == 0.0 and np.array_equal(covs[0], covs[2])  # (tile (2, 2): wholly inside the square)
