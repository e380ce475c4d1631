"""Per-group affines in re-flatten (decision D16: pm_path_groups / pm_reflatten_groups, the K...Grouped kernels of
piet_metal_amd/csrc/pm_flatten.hip) against tests/np_groups.py: the downloaded scene must be EQUAL to the splice of one-path
oracle scenes, every path under its own group's affine and width_scale -- no tolerance, no case left out.  Frames are compared with
the oracle's rendering of the expected bytes, picking with tests/np_hit.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_groups  # noqa: E402
import np_hit  # noqa: E402
import path_sets  # noqa: E402
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE, style_bits  # noqa: E402
from path_sets import COMPOUND, FILL, STROKE, L, M, Z, pathset  # noqa: E402
from test_stroke_gpu import IDENTITY, shapes  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -4


# ---- helpers ---------------------------------------------------------------------------------------------

def expected(pmo, ps, groups, affines, width_scales=None):
    return np_groups.scene(ps, groups, affines, width_scales, lambda p, e, a: pmo.scene_from_paths(p, e, a, cap=96 << 20))


def check_scene(r, want):
    """The resident scene is `want` = (bytes, n_items, path_of_item)."""
    scene, n_items, path_of_item = want
    got = r.download_scene()
    assert len(got) == len(scene), (len(got), len(scene))
    bad = np.flatnonzero(got != scene)
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert np.array_equal(r.item_paths(), path_of_item)


def check_frame(pmo, r, scene, width, height):
    got = r.read_pixels()
    bad = int((got != pmo.render(scene, width, height)).any(axis=2).sum())
    assert bad == 0, f"{bad} pixels differ from the oracle's rendering of the expected bytes"


def group_maps(n):
    """name -> map, for n paths: one group; two interleaved; one per path; the first and the last path alone in theirs."""
    ends = np.ones(n, np.uint32)
    ends[0], ends[-1] = 0, (2 if n > 1 else 0)
    return {"one": np.zeros(n, np.uint32), "interleaved": np.arange(n, dtype=np.uint32) % 2, "per_path": np.arange(n, dtype=np.uint32), "ends": ends}


def rot(th, s=1.0, tx=0.0, ty=0.0):
    return (s * np.cos(th), s * np.sin(th), -s * np.sin(th), s * np.cos(th), tx, ty)


SINGULAR = (2.0, 1.0, 4.0, 2.0, 30.0, 40.0)  # rank 1: every point of the group lands on one line


def random_table(rng, n_groups, singular=False):
    """A transform per group, the kinds in turn from a random start: a translation, a rotation, a non-uniform scale, a reflection
    (negative determinant), a scale that raises the curves' subdivision counts; `singular` makes one of them the rank-1 matrix.
    width_scale: sqrt|det|, except every third group, which gets a value of its own (the device must not derive it)."""
    kinds = [
        lambda: (1.0, 0.0, 0.0, 1.0, float(rng.uniform(-40, 60)), float(rng.uniform(-40, 60))),
        lambda: rot(float(rng.uniform(0.2, 6.0)), float(rng.choice([0.5, 1.0])), float(rng.uniform(20, 120)), float(rng.uniform(20, 120))),
        lambda: (float(rng.uniform(0.3, 1.6)), 0.0, 0.0, float(rng.uniform(0.3, 1.6)), float(rng.uniform(-10, 30)), float(rng.uniform(-10, 30))),
        lambda: (-0.8, 0.3, 0.2, 1.1, float(rng.uniform(100, 200)), float(rng.uniform(-20, 40))),
        lambda: (9.0, 0.0, 0.0, 7.5, float(rng.uniform(-300, 0)), float(rng.uniform(-300, 0))),
    ]
    start = int(rng.integers(0, len(kinds)))
    aff = np.array([kinds[(start + g) % len(kinds)]() for g in range(n_groups)], np.float64)
    if singular:
        aff[int(rng.integers(0, n_groups))] = SINGULAR
    ws = np_groups.default_width_scales(aff)
    ws[2::3] = np.float32(rng.choice([0.25, 1.0, 3.5]))
    return aff, ws


# ---- 1. scene parity ----------------------------------------------------------------------------------------

SEEDS = list(range(300, 312))
N_CHUNKS, SPLIT_CHUNK = 4, 2


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_groups_scene_parity(pm, pmo, monkeypatch, chunk):
    """Random path sets x the four group maps x random tables: bytes, item count, item_paths and the frame; every third scene has
    a singular matrix in its table and is judged on its bytes only.  One chunk goes through the block-parallel scans."""
    if chunk == SPLIT_CHUNK:
        monkeypatch.setenv("PM_SCAN_SPLIT", "4")
    k = 0
    with pm.Renderer(0) as r:
        for seed in SEEDS[chunk::N_CHUNKS]:
            case = path_sets.random_case(seed)
            ps = case.ps
            _, n_items0 = r.flatten_and_encode(ps, case.affine, case.scale)
            paths0 = r.item_paths()
            r.resize(case.width, case.height)
            for name, gmap in group_maps(len(ps.paths)).items():
                rng = np.random.default_rng(seed * 31 + len(name))
                singular = k % 3 == 2
                k += 1
                aff, ws = random_table(rng, int(gmap.max()) + 1, singular)
                r.set_path_groups(gmap)
                nbytes, n_items = r.reflatten_groups(aff, ws)
                want = expected(pmo, ps, gmap, aff, ws)
                assert (nbytes, n_items) == (len(want[0]), want[1]) and n_items == n_items0, (seed, name)
                assert np.array_equal(want[2], paths0)
                check_scene(r, want)
                if not singular:
                    r.render()
                    check_frame(pmo, r, want[0], case.width, case.height)


# ---- 2. an equal table is pm_reflatten -------------------------------------------------------------------------

@pytest.mark.parametrize("styled", [False, True], ids=["plain", "styled-dashed"])
def test_groups_equal_table_is_reflatten(pm, pmo, styled):
    if styled:
        ps = shapes(lambda k: (3 if k % 3 == 0 else 2) | style_bits(k % 3, (k // 3) % 3)).with_dashes([6, 3, 2], -4.0, select=[0, 3, 9])
        aff, scale = (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 2.5
    else:
        case = path_sets.random_case(321)
        ps, aff, scale = case.ps, case.affine2, 0.75
    n = len(ps.paths)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(np.arange(n) % 3), IDENTITY, 1.0)  # (the map goes along with the paths)
        a = r.reflatten(aff, scale)
        scene = r.download_scene()
        b = r.reflatten_groups([aff] * 3, [scale] * 3)
        assert a == b and np.array_equal(r.download_scene(), scene)
        r.set_path_groups(np.arange(n))
        b = r.reflatten_groups([aff] * (n + 2), [scale] * (n + 2))
        assert a == b and np.array_equal(r.download_scene(), scene)
        if not styled:
            check_scene(r, expected(pmo, ps, None, [aff], [scale]))


# ---- 3. styles and dashes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("cap,join", [(BUTT, MITER), (ROUND_CAP, ROUND_JOIN), (SQUARE, BEVEL)], ids=["butt-miter", "round-round", "square-bevel"])
def test_groups_styles_and_dashes(pm, pmo, cap, join):
    """Three groups with their own width_scale: 6 * 0.05 is below the thin-line width, 6 * 1 and 6 * 2.5 above; half of the paths
    dashed, one pattern of an odd count with a negative offset.  Outline levels, pattern lengths and cuts follow the group."""
    ps = shapes(lambda k: (3 if k % 4 == 0 else 2) | style_bits(cap, join))
    ps = ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5]).with_dashes([0, 6], 1.0, select=[9])
    gmap = np.arange(len(ps.paths), dtype=np.uint32) % 3
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 4.0, 2.0), (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), (0.9, 0.0, 0.0, -0.9, 10.0, 170.0)])
    ws = np.array([0.05, 1.0, 2.5], np.float32)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        nbytes, n_items = r.reflatten_groups(aff, ws)
        want = expected(pmo, ps, gmap, aff, ws)
        assert (nbytes, n_items) == (len(want[0]), want[1])
        check_scene(r, want)
        r.resize(192, 176)
        r.render()
        check_frame(pmo, r, want[0], 192, 176)


# ---- 4. structure edges --------------------------------------------------------------------------------------

def _edge_sets():
    tri, sq = path_sets._tri(20, 20), path_sets._square(60, 60, 30)
    cases = path_sets.edge_cases()
    return {
        "empty_path_between_groups": (pathset((tri, FILL | STROKE), ([], FILL | STROKE), (sq, FILL | STROKE)), [0, 1, 2]),
        "empty_path_ends_a_group": (pathset((tri, FILL | STROKE), ([], STROKE), (sq, FILL)), [0, 0, 1]),
        "neither_fill_nor_stroke": (pathset((tri, FILL), (path_sets._tri(50, 40), 0), (sq, STROKE | FILL | COMPOUND)), [1, 0, 1]),
        "compound_many_subpaths": (cases["compound_many_subpaths"].ps, [0, 1]),
        "subpath_of_200_elements": (cases["subpath_of_200_elements"].ps, [1, 0]),
        "unused_group": (pathset((tri, FILL | STROKE), (sq, FILL | STROKE)), [0, 3]),  # groups 1, 2 and 4: no path
    }


@pytest.mark.parametrize("name", sorted(_edge_sets()))
def test_groups_structure_edges(pm, pmo, name):
    ps, gmap = _edge_sets()[name]
    aff, ws = random_table(np.random.default_rng(len(name)), 5)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps, IDENTITY, 1.0)
        r.set_path_groups(gmap)
        nbytes, n_items = r.reflatten_groups(aff, ws)
        want = expected(pmo, ps, gmap, aff, ws)
        assert (nbytes, n_items) == (len(want[0]), want[1])
        check_scene(r, want)


# ---- 5. sequences ---------------------------------------------------------------------------------------------

def test_groups_sequence_with_frames_in_flight(pm, pmo):
    """flatten, groups, three tables, pm_reflatten (which ignores and keeps the map), a fourth table.  Every frame goes into a
    buffer of its own and nothing waits for it before the next re-flatten starts (it reads the other scene buffer); all five are
    compared with the oracle at the end.  New paths forget the map."""
    import torch

    case = path_sets.random_case(333)
    ps, w, h = case.ps, case.width, case.height
    gmap = np.arange(len(ps.paths), dtype=np.uint32) % 3
    rng = np.random.default_rng(9)
    tables = [random_table(rng, 3) for _ in range(4)]
    on_device = torch.cuda.is_available()  # (the emulated library of a box without a GPU has no device tensors: it reads each frame back)
    frames = []

    def frame(r, want):
        check_scene(r, want)
        if on_device:
            t = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
            r.render_to(t, None)
            frames.append((t, want[0]))
        else:
            r.render()
            check_frame(pmo, r, want[0], w, h)

    with pm.Renderer(0) as r:
        r.resize(w, h)
        r.flatten_and_encode(ps, case.affine, case.scale)
        r.set_path_groups(gmap)
        for aff, ws in tables[:3]:
            r.reflatten_groups(aff, ws)
            frame(r, expected(pmo, ps, gmap, aff, ws))
        r.reflatten(case.affine2, case.scale)
        frame(r, expected(pmo, ps, None, [case.affine2], [case.scale]))
        r.reflatten_groups(*tables[3])
        frame(r, expected(pmo, ps, gmap, *tables[3]))
        r.sync()
        for k, (t, scene) in enumerate(frames):
            bad = int((t.cpu().numpy() != pmo.render(scene, w, h)).any(axis=2).sum())
            assert bad == 0, f"frame {k}: {bad} pixels differ from the oracle's rendering of the expected bytes"
        r.flatten_and_encode(ps, case.affine, case.scale)
        with pytest.raises(pm.PietMetalError) as e:
            r.reflatten_groups(*tables[3])
        assert e.value.status == INVALID and "map" in str(e.value)


def test_groups_keep_the_binning_plan_like_reflatten(pm):
    """The same views through equal tables and through pm_reflatten: the two contexts make the same number of binning plans."""
    case = path_sets.random_case(334)
    ps, n = case.ps, len(case.ps.paths)
    views = [(rot(0.02 * k, case.scale, 30.0 + k, 20.0), case.scale) for k in range(1, 6)]
    plans = []
    for grouped in (False, True):
        with pm.Renderer(0) as r:
            r.resize(case.width, case.height)
            r.flatten_and_encode(ps.with_groups(np.arange(n)), case.affine, case.scale)
            r.render()
            for aff, s in views:
                if grouped:
                    r.reflatten_groups([aff] * n, [s] * n)
                else:
                    r.reflatten(aff, s)
                r.render()
            r.sync()
            plans.append(r.scene_timings()["binning_plans"])
    print("binning plans: pm_reflatten", plans[0], "equal tables", plans[1])
    assert plans[0] == plans[1]


# ---- 6. capacity ------------------------------------------------------------------------------------------------

def _call(pm, r, aff, ws):
    table = np.zeros(len(aff), pm.Renderer.GROUP_XFORM_DTYPE)
    table["m"], table["width_scale"] = aff, ws
    nbytes, n_items = C.c_size_t(0), C.c_uint32(0)
    st = pm._lib.load().pm_reflatten_groups(r._h, table.ctypes.data, len(table), C.byref(nbytes), C.byref(n_items))
    return st, nbytes.value


@pytest.mark.parametrize("styled", [False, True], ids=["plain", "styled"])
def test_groups_capacity_answer_is_the_splice_length(pm, pmo, monkeypatch, styled):
    if styled:
        ps = shapes(lambda k: 2 | style_bits(ROUND_CAP, ROUND_JOIN))
    else:
        ps = path_sets.random_case(340).ps
    gmap = np.arange(len(ps.paths), dtype=np.uint32) % 4
    aff, ws = random_table(np.random.default_rng(12), 4)
    want = expected(pmo, ps, gmap, aff, ws)
    need = len(want[0])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps, IDENTITY, 1.0)
        r.set_path_groups(gmap)
        for cap in (need - 8, need // 2):
            monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", str(cap))
            assert _call(pm, r, aff, ws) == (CAPACITY, need)
        monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", str(need))
        assert _call(pm, r, aff, ws) == (pm._lib.PM_OK, need)
        check_scene(r, want)
        monkeypatch.delenv("PM_FLATTEN_SCENE_CAP")


def test_groups_table_that_outgrows_the_scene_buffer(pm, pmo):
    """One group's scale makes its three curves ask for more points than the 16 MiB scene buffer holds: the call grows the buffer
    and runs again, as pm_reflatten does."""
    ps = pathset(*[(path_sets._tri(20 + 10 * k, 20), FILL | (STROKE if k % 2 else 0)) for k in range(6)])
    gmap = np.array([0, 1, 0, 1, 0, 1], np.uint32)
    big = 2.0e13
    aff = np.array([IDENTITY, (big, 0.0, 0.0, big, 5.0, 5.0)])
    ws = np.array([1.0, 1.0], np.float32)
    want = expected(pmo, ps, gmap, aff, ws)
    assert 16 << 20 < len(want[0]) < 64 << 20, len(want[0])
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        nbytes, n_items = r.reflatten_groups(aff, ws)
        assert (nbytes, n_items) == (len(want[0]), want[1])
        check_scene(r, want)
        r.reflatten_groups([IDENTITY, IDENTITY], ws)
        check_scene(r, expected(pmo, ps, gmap, [IDENTITY, IDENTITY], ws))


# ---- 7. arguments ------------------------------------------------------------------------------------------------

def test_groups_invalid_arguments_leave_the_context_usable(pm, pmo):
    lib = pm._lib.load()
    case = path_sets.random_case(350)
    ps, n = case.ps, len(case.ps.paths)
    assert n >= 2
    gmap = np.arange(n, dtype=np.uint32) % 2
    table = np.zeros(2, pm.Renderer.GROUP_XFORM_DTYPE)
    table["m"], table["width_scale"] = [IDENTITY, case.affine2], [1.0, case.scale]
    nbytes, n_items = C.c_size_t(0), C.c_uint32(0)

    def reflatten(h, tab, count):
        return lib.pm_reflatten_groups(h, tab.ctypes.data if tab is not None else None, count, C.byref(nbytes), C.byref(n_items))

    def invalid(status, *words):
        assert status == INVALID
        text = pm._lib.last_error()
        assert all(w in text for w in words), text

    with pm.Renderer(0) as r:
        invalid(lib.pm_path_groups(r._h, gmap.ctypes.data, n), "no paths resident")
        invalid(reflatten(r._h, table, 2), "no paths resident")
        r.resize(case.width, case.height)
        r.flatten_and_encode(ps, case.affine, case.scale)
        invalid(reflatten(r._h, table, 2), "no group map")
        invalid(lib.pm_path_groups(r._h, gmap.ctypes.data, n - 1), "n_paths")
        invalid(lib.pm_path_groups(r._h, gmap.ctypes.data, n + 1), "n_paths")
        invalid(lib.pm_path_groups(r._h, None, n), "NULL")
        invalid(lib.pm_path_groups(None, gmap.ctypes.data, n), "NULL")
        invalid(reflatten(r._h, table, 2), "no group map")  # (a refused map is no map)
        r.set_path_groups(gmap)
        invalid(reflatten(r._h, table, 0), "0 transforms")
        invalid(reflatten(r._h, table, 1), "1 transforms", "index 1")
        invalid(reflatten(r._h, None, 2), "NULL")
        invalid(reflatten(None, table, 2), "NULL")
        bad = table.copy()
        bad["reserved"][1] = 7
        invalid(reflatten(r._h, bad, 2), "reserved")
        # nothing of this touched the scene or the map
        check_scene(r, expected(pmo, ps, None, [case.affine], [case.scale]))
        assert reflatten(r._h, table, 2) == pm._lib.PM_OK
        want = expected(pmo, ps, gmap, table["m"], table["width_scale"])
        assert (nbytes.value, n_items.value) == (len(want[0]), want[1])
        check_scene(r, want)
        r.render()
        check_frame(pmo, r, want[0], case.width, case.height)


# ---- 8. picking ----------------------------------------------------------------------------------------------------

def test_groups_picking_follows_the_moved_group(pm, pmo):
    ps = pathset((path_sets._square(10, 10, 60), FILL), (path_sets._square(30, 30, 40), FILL | STROKE), (path_sets._tri(120, 120), STROKE, 5.0))
    gmap = np.array([0, 1, 0], np.uint32)
    q = np.array([(50.5, 50.5), (15.5, 15.5), (150.5, 50.5), (31.0, 31.0), (200.0, 200.0)], np.float32)
    here = np.array([IDENTITY, IDENTITY])
    away = np.array([IDENTITY, (1.0, 0.0, 0.0, 1.0, 100.0, 0.0)])
    tops = []
    with pm.Renderer(0) as r:
        r.flatten_and_encode(ps.with_groups(gmap), IDENTITY, 1.0)
        for aff in (here, away):
            r.reflatten_groups(aff)
            want = expected(pmo, ps, gmap, aff)
            check_scene(r, want)
            top, cnt = r.hit_test(q, counts=True)
            want_top, want_cnt = np_hit.hit_test(want[0], q)
            assert np.array_equal(top, want_top) and np.array_equal(cnt, want_cnt)
            tops.append(top)
    paths = want[2]
    assert paths[tops[0][0]] == 1 and paths[tops[1][0]] == 0  # the square of group 1 left the first point ...
    assert tops[0][2] == np_hit.HIT_NONE and paths[tops[1][2]] == 1  # ... and arrived at the third
