"""Dashed strokes where dash ends meet vertices, steps and limits (decision D15, piet_metal_amd/csrc/pm_dash.h): the seeded
grammar and the extremes of tests/dash_cases.py on the device, byte for byte against tests/np_dash.py through
test_dash_gpu.dashed_scene_checks -- no tolerance, no case left out.  The equality cases of CountAt, the m_lo rule, PlanOf,
LocateCut, KDash's carry across a 64-segment step, the saturations and the host's capacity growth for dashed scenes.

Without a GPU: the committed seeds must contain every event class (judged by np_dash alone), and the `small` tests run against
the emulated library."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dash_cases  # noqa: E402
import np_dash  # noqa: E402
import np_stroke  # noqa: E402
from dash_cases import CLASSES, EXTREMES, IDENTITY, SECOND_VIEW, SEEDS, VIEW  # noqa: E402
from test_dash_gpu import dashed_scene_checks, plain, polyline_of  # noqa: E402
from test_stroke_gpu import render_and_hit_checks  # noqa: E402

N_CHUNKS = 4
SPLIT_CHUNK = 2  # the chunk that runs with the block-parallel scans
N_SMALL = N_CHUNKS + len(EXTREMES) + 2  # the gpu tests of this file, all of them `small`


# ---- without a GPU ---------------------------------------------------------------------------------------------

def class_counts(seeds, case_of=dash_cases.dash_case):
    found, cut = Counter(), []
    for seed in seeds:
        case = case_of(seed)
        for classes in dash_cases.classes_of(case):
            found.update(classes)
        cut += dash_cases.is_cut(case)
    return found, cut


def test_committed_dash_seeds_are_not_a_thin_sample():
    """A condition on the inputs, judged by np_dash alone: over the committed seeds every event class occurs in at least 3
    sub-paths, and at least half of the sub-paths are cut into dashes (the rest are undashed, whole-cover or empty)."""
    found, cut = class_counts(SEEDS)
    print({k: found[k] for k in CLASSES})
    thin = {k: found[k] for k in CLASSES if found[k] < 3}
    assert not thin, thin
    assert set(found) <= set(CLASSES)
    assert len(cut) >= 200 and 2 * sum(cut) >= len(cut), (sum(cut), len(cut))


def test_dash_edge_kernels_under_wave64_emulation(built):
    """The `small` tests of this file -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "small", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_SMALL} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- on the device ---------------------------------------------------------------------------------------------

def stroke_polylines(pm, r0, ps, affine, scale):
    """The device's own poly-lines of the set's strokes, in item order, beside the spec of each (None: not a styled stroke)."""
    r0.flatten_and_encode(plain(pm, ps), affine, scale)
    scene0 = r0.download_scene()
    specs = np_dash.specs_from_pathset(ps, scale)
    return [(polyline_of(scene0, i), spec) for i, spec in enumerate(specs) if spec is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_dash_small_edge_seeds(pm, pmo, monkeypatch, chunk):
    """Every committed seed: scene bytes under the identity and, re-flattened, under a rotated view with a second width_scale;
    every fourth scene is also rendered and hit-tested.  One pair of renderers per chunk; one chunk with PM_SCAN_SPLIT=4."""
    if chunk == SPLIT_CHUNK:
        monkeypatch.setenv("PM_SCAN_SPLIT", "4")
    seeds = SEEDS[chunk::N_CHUNKS]
    assert len(seeds) >= 20
    with pm.Renderer(0) as r, pm.Renderer(0) as r0:
        for k, seed in enumerate(seeds):
            ps, ws = dash_cases.dash_case(seed)
            try:
                if k == 0:  # classes_of judges the points the kernels walk: under the identity the device's poly-lines are the grammar's
                    subs = dash_cases.subpaths_of(ps)
                    lines = stroke_polylines(pm, r0, ps, IDENTITY, ws)
                    assert len(subs) == len(lines)
                    for (_, pts, closed, _, _), (dev, spec) in zip(subs, lines):
                        assert np.array_equal(pts, dev) and bool(spec[0]) == closed
                scene = dashed_scene_checks(pm, r, ps, IDENTITY, ws, r0=r0)
                if k % 4 == 0:
                    render_and_hit_checks(pmo, r, scene, VIEW, VIEW, 200, seed=1000 + seed)
                dashed_scene_checks(pm, r, ps, SECOND_VIEW[0], SECOND_VIEW[1], reflatten=True, r0=r0)
            except AssertionError as e:
                raise AssertionError(f"seed {seed}: {e}") from e


def really_saturates(ex, lines):
    """By np_dash alone: the case reaches the cap it is there for."""
    ws = np.float32(ex.scale)
    tables = [spec[4] for _, spec in lines if spec[4] is not None]
    assert tables
    with np.errstate(over="ignore"):
        if ex.saturates == "segment":
            return all(int(np.diff(np_dash.walk(pts, spec[0])[1]).max()) == np_dash.CAP for pts, spec in lines)
        if ex.saturates == "pattern":
            return all(max(np_dash.fix(np.float64(np.float32(v) * ws)) for v in pattern) == np_dash.CAP for pattern, _, _ in tables)
        if ex.saturates == "every pattern value":
            return all(np_dash.fix(np.float64(np.float32(v) * ws)) == np_dash.CAP for pattern, _, _ in tables for v in pattern)
        assert ex.saturates == "offset"
        return all(np_dash.fix(abs(np.float64(np.float32(off) * ws)), np_dash.OFFSET_CAP) == np_dash.OFFSET_CAP and np.isinf(np.float32(off) * ws)
                   for _, off, _ in tables)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXTREMES))
def test_dash_small_extremes(pm, pmo, name):
    """The hand-made extremes: scene bytes; render and hit checks where the scene lies in a small viewport; a saturated case
    really saturates and a case of many dashes really has them (by np_dash alone)."""
    ex = EXTREMES[name]()
    with pm.Renderer(0) as r, pm.Renderer(0) as r0:
        lines = stroke_polylines(pm, r0, ex.ps, ex.affine, ex.scale)
        if ex.saturates:
            assert really_saturates(ex, lines), ex.saturates
        polys = [np_dash.cut(pts, spec[0], *spec[4]) for pts, spec in lines if spec[4] is not None]
        assert sum(len(p) for p in polys if isinstance(p, list)) >= ex.min_dashes
        if name.startswith("empty_item"):
            assert any(p == [] for p in polys)
        if name.startswith("whole_cover"):
            assert polys[0] == np_dash.CLOSED_WHOLE and any(isinstance(p, list) for p in polys[1:])
        scene = dashed_scene_checks(pm, r, ex.ps, ex.affine, ex.scale, r0=r0)
        print(name, len(scene), "bytes")
        if ex.view:
            render_and_hit_checks(pmo, r, scene, ex.view[0], ex.view[1], 200, seed=2000 + list(EXTREMES).index(name))
            assert np.array_equal(dashed_scene_checks(pm, r, ex.ps, ex.affine, ex.scale, reflatten=True, r0=r0), scene)


def growth_case(cap):
    """One zigzag of round joins at the top fan level (hw = 100: 72 entries a vertex) whose D14 outline ends some 60 KB short of
    `cap` bytes, cut into some 200 round-capped dashes of 139 entries more each
    (the gaps are shorter than a segment: a vertex in a gap has no join)."""
    n = (cap - 60_000) // (8 + 8 * 72)
    els = [(dash_cases.M, 1000.0, 1000.0)] + [(dash_cases.L, 1000.0 + 3.0 * (k % 2), 1000.0 + 0.5 * k) for k in range(1, n)]
    length = 3.0413812651491097 * (n - 1)  # (a guide to the pattern only)
    return dash_cases.make_pathset([(els, dash_cases.STROKE | np_stroke.style_bits(np_stroke.ROUND_CAP, np_stroke.ROUND_JOIN), 200.0,
                                     [length / 200.0 - 1.0, 1.0], 17.0)])


@pytest.mark.gpu
def test_dash_small_growth_takes_two_attempts(pm):
    """A fresh renderer's scene capacity (pm_scene_buffer's: pm_create reserves the pinned buffer and the device copy alike) holds
    the scene's poly-lines and its undashed outline, but not its dashes: the first attempt counts them from the stored points and
    answers with the need, the second one, after the growth, makes the scene -- PM_OK with np_dash's bytes from the one call; a
    reflatten gives the same bytes."""
    with pm.Renderer(0) as r:
        cap = int(r.scene_buffer().size)
        ps = growth_case(cap)
        with pm.Renderer(0) as r0:
            r0.flatten_and_encode(plain(pm, ps), IDENTITY, 1.0)
            scene0 = r0.download_scene()
        (spec,) = np_dash.specs_from_pathset(ps, 1.0)
        undashed = np_stroke.apply(scene0, [spec[:4]])
        want = np_dash.apply(scene0, [spec])
        polys = np_dash.cut(polyline_of(scene0, 0), False, *spec[4])
        print("capacity", cap, "poly-lines", len(scene0), "undashed", len(undashed), "dashed", len(want), "dashes", len(polys))
        assert len(scene0) < len(undashed) <= cap < len(want) and cap >= (1 << 20)
        assert len(polys) >= 100 and max(len(p) for p in polys) > 130  # dashes that stay open over two steps of the walk
        assert int(r.scene_buffer().size) == cap  # (nothing has grown yet)
        nbytes, n_items = r.flatten_and_encode(ps, IDENTITY, 1.0)
        got = r.download_scene()
        assert (nbytes, n_items) == (len(want), 1) and np.array_equal(got, np.frombuffer(want, np.uint8))
        assert r.reflatten(IDENTITY, 1.0) == (nbytes, n_items) and np.array_equal(r.download_scene(), got)


@pytest.mark.gpu
def test_dash_small_growth_when_the_points_do_not_fit(pm):
    """The other way into the growth loop, the one that needs its second pass: the scene's poly-lines alone (2^21 points of a
    filled curve) exceed a fresh renderer's capacity, so the first attempt stores no point and answers with the need of the UNDASHED
    outline; the second, in a buffer an eighth larger than that, learns the dashes (2 560 of them, 139 entries each: more than the
    eighth) and answers again; the third makes the scene."""
    from path_sets import curve_for_x, p6

    el = (curve_for_x(p6(1 << 20), "at") or curve_for_x(p6(1 << 20), "below"))[0]
    fill = ([(dash_cases.M, 0.0, 0.0), el, el], dash_cases.FILL, 1.0, None, 0.0)
    stroke = ([(dash_cases.M, 300.0, 300.0), (dash_cases.L, 300.078125, 300.0)], dash_cases.STROKE | np_stroke.style_bits(np_stroke.ROUND_CAP, np_stroke.MITER),
              200.0, [2.0 ** -16, 2.0 ** -16], 0.0)
    ps = dash_cases.make_pathset([fill, stroke])
    with pm.Renderer(0) as r:
        cap = int(r.scene_buffer().size)
        with pm.Renderer(0) as r0:
            r0.flatten_and_encode(plain(pm, ps), IDENTITY, 1.0)
            scene0 = r0.download_scene()
        specs = np_dash.specs_from_pathset(ps, 1.0)
        undashed = len(np_stroke.apply(scene0, [None, specs[1][:4]]))
        want = np_dash.apply(scene0, specs)
        print("capacity", cap, "poly-lines", len(scene0), "undashed", undashed, "dashed", len(want))
        assert cap < len(scene0) < undashed and undashed + (undashed >> 3) < len(want)
        nbytes, n_items = r.flatten_and_encode(ps, IDENTITY, 1.0)
        got = r.download_scene()
        assert (nbytes, n_items) == (len(want), 2) and np.array_equal(got, np.frombuffer(want, np.uint8))
        assert r.reflatten(IDENTITY, 1.0) == (nbytes, n_items) and np.array_equal(r.download_scene(), got)
