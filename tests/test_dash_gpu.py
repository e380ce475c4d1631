"""Dashed strokes on the device (decision D15, piet_metal_amd/csrc/pm_dash.h) against tests/np_dash.py, the independent numpy
statement: the scene bytes after flatten_and_encode must be EQUAL to np_dash applied to the un-dashed poly-line scene of the same
paths, which a second renderer makes -- no tolerance, no case left out.  What the renderer, hit testing and item_paths make of the
items is checked against the oracle's renderer and np_hit, which know nothing of dashes.

The `small` tests are also what tests/test_dash_cpu.py runs against the emulated library on a box without a GPU."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_dash  # noqa: E402
import np_hit  # noqa: E402
import np_stroke  # noqa: E402
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE, style_bits  # noqa: E402
from test_stroke_gpu import IDENTITY, render_and_hit_checks, shapes  # noqa: E402

pytestmark = pytest.mark.gpu

M, L, CU, Z = 0, 1, 3, 4
STROKE = 2


# ---- helpers ---------------------------------------------------------------------------------------------

def plain(pm, ps):
    """The same paths without any style bit and without the dash table: what draws the poly-line scene."""
    return pm.PathSet(np_stroke.unstyled(ps.paths), ps.els)


def dashed_scene_checks(pm, r, ps, affine, scale, reflatten=False, r0=None):
    """Flattens (or re-flattens) ps; the scene must be np_dash applied to the poly-line scene of the same paths under the same
    view, which a second renderer makes (r0, or one of its own).  Returns the scene bytes."""
    if reflatten:
        nbytes, n_items = r.reflatten(affine, scale)
    else:
        nbytes, n_items = r.flatten_and_encode(ps, affine, scale)
    got = r.download_scene()
    with contextlib.nullcontext(r0) if r0 is not None else pm.Renderer(0) as r0:
        nbytes0, n_items0 = r0.flatten_and_encode(plain(pm, ps), affine, scale)
        scene0 = r0.download_scene()
        paths0 = r0.item_paths()
    want = np.frombuffer(np_dash.apply(scene0, np_dash.specs_from_pathset(ps, scale)), np.uint8)
    assert n_items == n_items0 and nbytes == len(want) == len(got), (n_items, n_items0, nbytes, len(want), len(got))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert np.array_equal(r.item_paths(), paths0)  # one dashed stroke is one item, in the poly-line's slot
    return got


def polyline_of(scene, item):
    sc = bytes(scene)
    n, items_ix = np_hit.struct.unpack_from("<II", sc, 0)
    tag, _, _, npt, pix = np_hit.struct.unpack_from("<IIfII", sc, items_ix + 32 * item)
    assert tag == 4
    return np.frombuffer(sc, np.float32, 2 * npt, pix).reshape(npt, 2)


def poly_scene(pm, ps, affine=IDENTITY, scale=1.0):
    with pm.Renderer(0) as r0:
        r0.flatten_and_encode(plain(pm, ps), affine, scale)
        return r0.download_scene()


# every path of the `shapes` page its own pattern: even, odd, 32 values, a zero dash, a negative offset, an offset beyond G
PATTERNS = [([8, 4], 0.0), ([5], 0.0), ([6, 3, 2], 1.5), ([3, 1, 2, 1] * 8, 0.0), ([0, 6], 0.0), ([7, 3], -4.0), ([4, 2], 50.0), ([3, 3], 0.0),
            ([2, 2], 1.0), ([10, 5], 3.0)]


def dashed_shapes(flags_of, width=6.0):
    ps = shapes(flags_of, width)
    for k, (pat, off) in enumerate(PATTERNS):
        ps = ps.with_dashes(pat, off, select=[k])
    return ps


# ---- small cases (also run under emulation) -------------------------------------------------------------------

@pytest.mark.parametrize("cap,join", [(BUTT, MITER), (ROUND_CAP, ROUND_JOIN), (SQUARE, BEVEL)], ids=["butt-miter", "round-round", "square-bevel"])
def test_dash_small_shapes_page(pm, pmo, cap, join):
    """Open and closed sub-paths, curves, repeated points, dots, two sub-paths in a path, every path its own pattern; under the
    identity, under a rotation with a wide width_scale and under a hairline one (the thin-line rule; the dashes shrink too)."""
    ps = dashed_shapes(lambda k: STROKE | style_bits(cap, join))
    assert len(ps.dashes) == 10
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, IDENTITY, 1.0)
        n, top = render_and_hit_checks(pmo, r, scene, 176, 160, 300, seed=31)
        assert (top != np_hit.HIT_NONE).sum() >= 10
        scene2 = dashed_scene_checks(pm, r, ps, (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 2.5, reflatten=True)
        assert not np.array_equal(scene, scene2)
        dashed_scene_checks(pm, r, ps, IDENTITY, 0.05, reflatten=True)
        render_and_hit_checks(pmo, r, r.download_scene(), 176, 160, 100, seed=32)


def test_dash_small_one_segment_with_a_thousand_dashes(pm, pmo):
    """One 2-point line: the pieces of one segment are spread over many lane steps."""
    from path_sets import pathset

    ps = pathset(([(M, 10, 20), (L, 340, 20.5)], STROKE | style_bits(ROUND_CAP, MITER), 2.0)).with_dashes([0.2, 0.12], 0.05)
    polys = np_dash.cut(polyline_of(poly_scene(pm, ps), 0), False, [0.2, 0.12], 0.05, 1.0)
    assert len(polys) >= 1000
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, IDENTITY, 1.0)
        render_and_hit_checks(pmo, r, scene, 352, 48, 200, seed=33)


def wavy():
    els = [(M, 10, 100)]
    for k in range(10):  # (S-shaped cubics: some 25 segments each at the flatten tolerance)
        x, s = 10 + 33 * k, (-1) ** k
        els.append((CU, x + 8, 100 + 70 * s, x + 25, 100 - 30 * s, x + 33, 100))
    return els


def test_dash_small_curve_with_a_dash_across_steps(pm, pmo):
    """A flattened curve of >= 200 segments whose dashes span > 64 vertices: the carry of the walk across 64-segment steps, and a
    dash that is open at a step's boundary (looked ahead for, carried)."""
    from path_sets import pathset

    ps = pathset((wavy(), STROKE | style_bits(BUTT, ROUND_JOIN), 3.0)).with_dashes([260, 20, 15, 5], 40.0)
    pts = polyline_of(poly_scene(pm, ps), 0)
    polys = np_dash.cut(pts, False, [260, 20, 15, 5], 40.0, 1.0)
    assert len(pts) >= 201 and max(len(p) for p in polys) > 66 and len(polys) >= 4
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, IDENTITY, 1.0)
        render_and_hit_checks(pmo, r, scene, 352, 200, 200, seed=34)
        dashed_scene_checks(pm, r, ps, (0.9, 0.2, -0.2, 0.9, 30.0, 10.0), 0.7, reflatten=True)


def ring(n=100, cx=100.0, cy=100.0, rad=60.0):
    a = 2 * np.pi * np.arange(n) / n
    pts = [(round(cx + rad * np.cos(t), 3), round(cy + rad * np.sin(t), 3)) for t in a]
    return [(M, *pts[0])] + [(L, *p) for p in pts[1:]] + [(Z,)]


@pytest.mark.parametrize("cap,join", [(ROUND_CAP, MITER), (SQUARE, ROUND_JOIN)], ids=["round-miter", "square-round"])
def test_dash_small_closed_path_merges_across_its_start(pm, pmo, cap, join):
    """A closed path of > 64 vertices: the last dash and the first are one poly-line, the start vertex gets a join and no caps."""
    from path_sets import pathset

    for pattern, offset, n_dashes in (([300, 50], 200.0, 1), ([40, 25], 30.0, None), ([1000, 1], 0.0, "whole")):
        ps = pathset((ring(), STROKE | style_bits(cap, join), 5.0)).with_dashes(pattern, offset)
        pts = polyline_of(poly_scene(pm, ps), 0)
        polys = np_dash.cut(pts, True, pattern, offset, 1.0)
        if n_dashes == "whole":
            assert polys == np_dash.CLOSED_WHOLE
        else:
            assert n_dashes is None or len(polys) == n_dashes
            whole_walk = np_dash.walk(pts, True)[0]
            # merged: the first poly-line runs through the walk's end and its start
            assert any((polys[0][i] == whole_walk[-1]).all() and (polys[0][i + 1] == whole_walk[0]).all() for i in range(len(polys[0]) - 1))
            if n_dashes == 1:
                assert len(polys[0]) > 64
        with pm.Renderer(0) as r:
            scene = dashed_scene_checks(pm, r, ps, IDENTITY, 1.0)
            render_and_hit_checks(pmo, r, scene, 208, 208, 150, seed=35)


def test_dash_small_mixed_paths(pm, pmo):
    """Fill + dashed stroke, compound fills, dashed beside undashed-styled beside plain poly-line strokes."""
    from path_sets import COMPOUND, FILL

    st = [FILL | STROKE | style_bits(SQUARE, MITER), STROKE, FILL | COMPOUND | STROKE | style_bits(ROUND_CAP, ROUND_JOIN), FILL,
          STROKE | style_bits(BUTT, BEVEL), FILL | STROKE, STROKE | style_bits(ROUND_CAP, MITER), FILL | COMPOUND,
          FILL | STROKE | style_bits(BUTT, MITER), FILL | COMPOUND | STROKE | style_bits(SQUARE, BEVEL) | 4]
    ps = shapes(lambda k: st[k], width=4.0)
    ps = ps.with_dashes([6, 4], 1.0, select=[0, 2, 9]).with_dashes([9, 2, 1, 2], -3.0, select=[1, 3, 4, 5, 7])  # (1, 3, 5, 7: not outlined, left alone)
    assert [int(d["path"]) for d in ps.dashes] == [0, 2, 4, 9]
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, IDENTITY, 1.0)
        render_and_hit_checks(pmo, r, scene, 176, 160, 300, seed=36)
        scene2 = dashed_scene_checks(pm, r, ps, (0.9, 0.1, -0.2, -1.1, 20.0, 170.0), 1.5, reflatten=True)
        render_and_hit_checks(pmo, r, scene2, 176, 160, 200, seed=37)
        # a later plain flatten_and_encode forgets the table: the undashed styled scene, also after a reflatten
        undashed = pm.PathSet(ps.paths, ps.els)
        r.flatten_and_encode(undashed, IDENTITY, 1.0)
        a = r.download_scene()
        r.reflatten(IDENTITY, 1.0)
        assert np.array_equal(a, r.download_scene())
        with pm.Renderer(0) as r0:
            r0.flatten_and_encode(plain(pm, ps), IDENTITY, 1.0)
            want = np_stroke.apply(r0.download_scene(), np_stroke.specs_from_paths(ps.paths, ps.els))
        assert np.array_equal(a, np.frombuffer(want, np.uint8))


def call_dashed(lib, r, ps, dashes, values, n_dashes=None, n_values=None, scale=1.0):
    aff = (C.c_double * 6)(*IDENTITY)
    nbytes, nitems = C.c_size_t(0), C.c_uint32(0)
    d = np.ascontiguousarray(dashes)
    v = np.ascontiguousarray(values, np.float32)
    st = lib.pm_flatten_and_encode_dashed(r._h, ps.paths.ctypes.data, len(ps.paths), ps.els.ctypes.data, len(ps.els), d.ctypes.data,
                                          len(d) if n_dashes is None else n_dashes, v.ctypes.data, len(v) if n_values is None else n_values, aff, scale,
                                          C.byref(nbytes), C.byref(nitems))
    return st, nbytes.value


def test_dash_small_no_table_is_the_plain_call(pm):
    lib = pm._lib.load()
    ps = dashed_shapes(lambda k: STROKE | style_bits(ROUND_CAP, BEVEL))
    with pm.Renderer(0) as r:
        st, nbytes = call_dashed(lib, r, ps, ps.dashes, ps.dash_values, n_dashes=0)
        assert st == pm._lib.PM_OK
        a = r.download_scene()
        nbytes2, _ = r.flatten_and_encode(pm.PathSet(ps.paths, ps.els), IDENTITY, 1.0)
        assert nbytes == nbytes2 and np.array_equal(a, r.download_scene())


def test_dash_small_block_parallel_scans(pm, pmo, monkeypatch):
    monkeypatch.setenv("PM_SCAN_SPLIT", "4")
    ps = dashed_shapes(lambda k: (3 if k % 3 == 0 else 2) | style_bits(k % 3, (k // 3) % 3))
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, (2.0, 0.0, 0.0, 2.0, 5.0, 5.0), 2.0)
        render_and_hit_checks(pmo, r, scene, 352, 320, 200, seed=38)


def test_dash_small_capacity_one_entry_short(pm, monkeypatch):
    """One outline entry short of the need the answer is PM_ERR_CAPACITY with the exact needed size (dashes included); at the
    need itself the scene is made, the same bytes."""
    lib = pm._lib.load()
    ps = dashed_shapes(lambda k: STROKE | style_bits(ROUND_CAP, ROUND_JOIN))
    with pm.Renderer(0) as r:
        st, need = call_dashed(lib, r, ps, ps.dashes, ps.dash_values)
        assert st == pm._lib.PM_OK
        want = r.download_scene()
        assert need == len(want)
        with pm.Renderer(0) as r0:
            plain_bytes, _ = r0.flatten_and_encode(plain(pm, ps), IDENTITY, 1.0)
        assert need > plain_bytes
        for cap in (need - 8, plain_bytes):  # (short of the outlines by one entry, and by all of them)
            monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", str(cap))
            assert call_dashed(lib, r, ps, ps.dashes, ps.dash_values) == (pm._lib.PM_ERR_CAPACITY, need)
        monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", str(need))
        assert call_dashed(lib, r, ps, ps.dashes, ps.dash_values) == (pm._lib.PM_OK, need)
        assert np.array_equal(r.download_scene(), want)
        monkeypatch.delenv("PM_FLATTEN_SCENE_CAP")


def test_dash_small_invalid_tables(pm):
    lib = pm._lib.load()
    ps = shapes(lambda k: STROKE | (style_bits(BUTT, MITER) if k != 1 else 0) if k != 2 else 1)  # path 1: a plain stroke, path 2: a fill only
    DT = pm.PathSet.DASH_DTYPE
    ok_values = np.array([4, 2, 3], np.float32)

    def table(*rows):
        return np.array(list(rows), DT)

    inf, nan = float("inf"), float("nan")
    bad = {
        "index >= n_paths": (table((10, 0, 2, 0.0)), ok_values),
        "not ascending": (table((3, 0, 2, 0.0), (0, 0, 2, 0.0)), ok_values),
        "a path twice": (table((3, 0, 2, 0.0), (3, 0, 2, 0.0)), ok_values),
        "no outline bit": (table((1, 0, 2, 0.0)), ok_values),
        "no stroke": (table((2, 0, 2, 0.0)), ok_values),
        "count 0": (table((0, 0, 0, 0.0)), ok_values),
        "count 33": (table((0, 0, 33, 0.0)), np.ones(40, np.float32)),
        "range outside the values": (table((0, 2, 2, 0.0)), ok_values),
        "first outside the values": (table((0, 0xFFFFFFFF, 2, 0.0)), ok_values),
        "negative value": (table((0, 0, 2, 0.0)), np.array([4, -1], np.float32)),
        "infinite value": (table((0, 0, 2, 0.0)), np.array([inf, 1], np.float32)),
        "NaN value": (table((0, 0, 2, 0.0)), np.array([4, nan], np.float32)),
        "infinite offset": (table((0, 0, 2, inf)), ok_values),
        "NaN offset": (table((0, 0, 2, nan)), ok_values),
    }
    with pm.Renderer(0) as r:
        for what, (d, v) in bad.items():
            assert call_dashed(lib, r, ps, d, v)[0] == pm._lib.PM_ERR_INVALID, what
        assert call_dashed(lib, r, ps, table((0, 1, 2, -7.5), (3, 0, 3, 1e6)), ok_values)[0] == pm._lib.PM_OK
        assert call_dashed(lib, r, ps, table((0, 0, 32, 0.0)), np.ones(32, np.float32))[0] == pm._lib.PM_OK


def test_dash_small_non_finite_coordinates_return(pm):
    """NaN and infinite points in a dashed path: NaN entries, no bit pattern promised -- the call returns."""
    from path_sets import pathset

    nan, inf = float("nan"), float("inf")
    ps = pathset(([(M, 10, 10), (L, 60, 10), (L, nan, 40), (L, 90, 50), (L, inf, 60), (L, 20, 80), (Z,)], STROKE | style_bits(ROUND_CAP, ROUND_JOIN), 4.0),
                 ([(M, 10, 100), (L, 80, 100)], STROKE | style_bits(BUTT, MITER), 4.0)).with_dashes([5, 3])
    with pm.Renderer(0) as r:
        nbytes, n_items = r.flatten_and_encode(ps, IDENTITY, 1.0)
        assert n_items == 2 and nbytes == len(r.download_scene())
        r.reflatten((2.0, 0.0, 0.0, 2.0, 0.0, 0.0), 2.0)


SVG_DOC = """<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 400 300">
<style> .dots { stroke-dasharray: 0 14; stroke-linecap: round } </style>
<g fill="none" stroke="#204080" stroke-width="8" stroke-dasharray="20,10">
  <path d="M 20 40 L 120 30 L 60 90 L 180 100"/>
  <path class="dots" d="M 220 40 L 320 30 L 260 90 L 380 100"/>
  <g stroke-dashoffset="7" stroke="#a02040">
    <rect x="30" y="150" width="120" height="70" style="stroke-dasharray: 15 5 5"/>
    <polygon points="240,240 290,290 340,240" stroke-dasharray="none" fill="#ffcc00"/>
    <path d="M 200 160 C 240 120 300 240 380 170" stroke-dasharray="12, -3"/>
  </g>
</g></svg>"""


def test_dash_small_cli_flag(pm, pmo, tmp_path):
    """--stroke-dashes: the file's dashes are drawn; --stroke-styles alone draws what it drew."""
    from piet_metal_amd import cli

    svg = tmp_path / "doc.svg"
    svg.write_text(SVG_DOC)
    outs = []
    for extra in (["--stroke-styles"], ["--stroke-dashes"]):
        out = tmp_path / f"o{len(outs)}.png"
        assert cli.main([str(svg), str(out), "--width", "200", "--height", "150"] + extra) == 0
        outs.append(cli.read_png_rgba(str(out)))
    assert not np.array_equal(outs[0], outs[1])
    solid = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, flat_gradients=True, stroke_styles=True)
    ps = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, flat_gradients=True, stroke_styles=True, stroke_dashes=True)
    assert len(solid.dashes) == 0 and np.array_equal(solid.paths, ps.paths) and [int(d["path"]) for d in ps.dashes] == [0, 1, 2]
    aff, s = ps.fit_affine(200, 150)
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, aff, s)
        assert np.array_equal(outs[1], pmo.render(scene, 200, 150))
        r.flatten_and_encode(solid, aff, s)
        assert np.array_equal(outs[0], pmo.render(r.download_scene(), 200, 150))


# ---- the full case ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap,join", [("round", "round"), ("butt", "miter")], ids=["round-round", "butt-miter"])
def test_tiger_with_every_stroke_dashed(pm, pmo, cap, join):
    wl = pm.workloads.tiger(960, 540)
    ps = wl.paths.with_stroke_style(cap, join).with_dashes([6, 3])
    assert len(ps.dashes) == ((wl.paths.paths["flags"] & 2) != 0).sum() > 0
    with pm.Renderer(0) as r:
        scene = dashed_scene_checks(pm, r, ps, wl.affine, wl.width_scale)
        n, _ = render_and_hit_checks(pmo, r, scene, wl.width, wl.height, 20_000, seed=600)
        assert n >= 20_000
        scene2 = dashed_scene_checks(pm, r, ps, (2.0, 0.7, -0.7, 2.0, 300.0, -60.0), wl.width_scale, reflatten=True)
        render_and_hit_checks(pmo, r, scene2, wl.width, wl.height, 20_000, seed=601)
