"""Stroke caps, joins and miter limits on the device (decision D14, piet_metal_amd/csrc/pm_stroke_outline.h) against
tests/np_stroke.py, the independent numpy statement: the scene bytes after flatten_and_encode must be EQUAL to np_stroke applied to
the unstyled device scene of the same paths -- no tolerance, no case left out.  What the renderer, hit testing and item_paths make of
the outline items is checked against the oracle's renderer and np_hit, which know nothing of strokes' styles.

The `small` tests are also what tests/test_stroke_cpu.py runs against the emulated library on a box without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_hit  # noqa: E402
import np_stroke  # noqa: E402
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE, half_bits, style_bits  # noqa: E402

pytestmark = pytest.mark.gpu

CAPS = {"butt": BUTT, "round": ROUND_CAP, "square": SQUARE}
JOINS = {"miter": MITER, "round": ROUND_JOIN, "bevel": BEVEL}
COMBOS = [(c, j) for c in CAPS for j in JOINS]
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


# ---- helpers ---------------------------------------------------------------------------------------------

def plain(pm, ps):
    """The same paths without any style bit: what draws the poly-line scene."""
    return pm.PathSet(np_stroke.unstyled(ps.paths), ps.els)


def styled_scene_checks(pm, r, ps, affine, scale, reflatten=False):
    """Flattens (or re-flattens) ps; the scene must be np_stroke applied to the poly-line scene of the same paths under the same
    view, which a second renderer makes.  Returns the scene bytes."""
    if reflatten:
        nbytes, n_items = r.reflatten(affine, scale)
    else:
        nbytes, n_items = r.flatten_and_encode(ps, affine, scale)
    got = r.download_scene()
    with pm.Renderer(0) as r0:
        nbytes0, n_items0 = r0.flatten_and_encode(plain(pm, ps), affine, scale)
        scene0 = r0.download_scene()
        paths0 = r0.item_paths()
    want = np.frombuffer(np_stroke.apply(scene0, np_stroke.specs_from_paths(ps.paths, ps.els)), np.uint8)
    assert n_items == n_items0 and nbytes == len(want) == len(got)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert np.array_equal(r.item_paths(), paths0)  # one styled stroke is one item, in the poly-line's slot
    return got


def queries(scene, width, height, n, seed):
    rng = np.random.default_rng(seed)
    uni = rng.uniform(0.0, 1.0, (n, 2)) * (width + 16.0, height + 16.0) - 8.0  # the viewport and a margin around it
    sc = bytes(scene)
    verts = []
    for at, _ in np_hit.flat_items(sc):
        if np_hit.struct.unpack_from("<I", sc, at)[0] & 0xFFFF == np_hit.FILL:
            pts = np_hit._points(sc, at)
            verts.append(pts[~np.isnan(pts[:, 0])][::37])
    v = np.concatenate(verts) if verts else np.zeros((0, 2), np.float32)
    return np.concatenate([uni, v.astype(np.float64), v.astype(np.float64) + rng.uniform(-0.6, 0.6, v.shape)]).astype(np.float32)


def render_and_hit_checks(pmo, r, scene, width, height, n_queries, seed):
    r.resize(width, height)
    r.render()
    got = r.read_pixels()
    want = pmo.render(scene, width, height)
    bad = int((got != want).any(axis=2).sum())
    assert bad == 0, f"{bad} pixels differ from the oracle's rendering of the same bytes"
    q = queries(scene, width, height, n_queries, seed)
    want_top, want_cnt = np_hit.hit_test(scene, q)
    top, cnt = r.hit_test(q, counts=True)
    assert np.array_equal(top, want_top) and np.array_equal(cnt, want_cnt)
    return len(q), want_top


M, L, CU, Z = 0, 1, 3, 4


def shapes(flags_of, width=6.0):
    """A page of strokes: a zigzag with sharp and blunt turns, a closed triangle and the same open, a curve, a reversal, repeated
    points at the start, inside and at the end, a dot (M L to the same point), a lone MoveTo, a closed dot, two sub-paths in one path."""
    from path_sets import pathset

    zig = [(M, 10, 20), (L, 40, 12), (L, 44, 40), (L, 60, 14), (L, 90, 30), (L, 70, 34)]
    tri = [(M, 110, 15), (L, 150, 22), (L, 125, 50), (Z,)]
    tri_open = [(M, 110, 65), (L, 150, 72), (L, 125, 100)]
    curve = [(M, 12, 60), (CU, 30, 40, 60, 110, 90, 62), (L, 96, 90)]
    back = [(M, 15, 110), (L, 60, 110), (L, 30, 110)]
    rep = [(M, 20, 130), (L, 20, 130), (L, 50, 125), (L, 50, 125), (L, 50, 125), (L, 70, 140), (L, 70, 140)]
    dot = [(M, 110, 120), (L, 110, 120)]
    lone = [(M, 130, 120)]
    closed_dot = [(M, 150, 120), (Z,)]
    two = [(M, 100, 135), (L, 120, 150), (L, 140, 135), (Z,), (M, 150, 140), (L, 165, 150)]
    all_ = [zig, tri, tri_open, curve, back, rep, dot, lone, closed_dot, two]
    return pathset(*[(els, flags_of(k), width) for k, els in enumerate(all_)])


# ---- small cases (also run under emulation) -------------------------------------------------------------------

@pytest.mark.parametrize("cap,join", COMBOS, ids=[f"{c}-{j}" for c, j in COMBOS])
def test_stroke_small_every_cap_and_join(pm, pmo, cap, join):
    """All nine combinations, miter limits 1, 4 (as 0 = the default, and spelled out) and 10 by path, open and closed sub-paths,
    curves, repeated points, dots; under the identity and under a rotation with a wide and a hairline (thin-line rule) width."""
    limits = [0, half_bits(1.0), half_bits(4.0), half_bits(10.0)]
    ps = shapes(lambda k: 2 | style_bits(CAPS[cap], JOINS[join], limits[k % 4]))
    with pm.Renderer(0) as r:
        scene = styled_scene_checks(pm, r, ps, IDENTITY, 1.0)
        n, top = render_and_hit_checks(pmo, r, scene, 176, 160, 300, seed=21)
        assert (top != np_hit.HIT_NONE).sum() >= 20
        aff = (1.3, 0.5, -0.5, 1.3, 60.0, -20.0)
        scene2 = styled_scene_checks(pm, r, ps, aff, 2.5, reflatten=True)  # hw = 7.5: level 4
        assert not np.array_equal(scene, scene2)
        styled_scene_checks(pm, r, ps, IDENTITY, 0.05, reflatten=True)     # width 0.3 < 0.7: the thin-line rule, hw = 0.35
        render_and_hit_checks(pmo, r, r.download_scene(), 176, 160, 100, seed=22)


def test_stroke_small_mixed_paths(pm, pmo):
    """A path with fill and stroke, compound fills beside styled strokes, styled and unstyled strokes side by side."""
    from path_sets import COMPOUND, FILL, STROKE

    st = [FILL | STROKE | style_bits(SQUARE, MITER), STROKE, FILL | COMPOUND | STROKE | style_bits(ROUND_CAP, ROUND_JOIN), FILL,
          STROKE | style_bits(BUTT, BEVEL), FILL | STROKE, STROKE | style_bits(ROUND_CAP, MITER, half_bits(10.0)), FILL | COMPOUND,
          FILL | STROKE | style_bits(BUTT, MITER), FILL | COMPOUND | STROKE | style_bits(SQUARE, BEVEL) | 4]
    ps = shapes(lambda k: st[k], width=4.0)
    with pm.Renderer(0) as r:
        scene = styled_scene_checks(pm, r, ps, IDENTITY, 1.0)
        render_and_hit_checks(pmo, r, scene, 176, 160, 300, seed=23)
        scene2 = styled_scene_checks(pm, r, ps, (0.9, 0.1, -0.2, -1.1, 20.0, 170.0), 1.5, reflatten=True)
        render_and_hit_checks(pmo, r, scene2, 176, 160, 200, seed=24)
        # without the outline bit the other bits are ignored: the poly-line scene, byte for byte
        ignored = pm.PathSet(ps.paths.copy(), ps.els)
        ignored.paths["flags"] &= ~np.uint32(np_stroke.OUTLINE)
        r.flatten_and_encode(ignored, IDENTITY, 1.0)
        a = r.download_scene()
        r.flatten_and_encode(plain(pm, ps), IDENTITY, 1.0)
        assert np.array_equal(a, r.download_scene())


def test_stroke_small_block_parallel_scans(pm, pmo, monkeypatch):
    monkeypatch.setenv("PM_SCAN_SPLIT", "4")
    ps = shapes(lambda k: (3 if k % 3 == 0 else 2) | style_bits(k % 3, (k // 3) % 3))
    with pm.Renderer(0) as r:
        scene = styled_scene_checks(pm, r, ps, (2.0, 0.0, 0.0, 2.0, 5.0, 5.0), 2.0)
        render_and_hit_checks(pmo, r, scene, 352, 320, 200, seed=25)


def test_stroke_small_capacity_one_entry_short(pm, monkeypatch):
    """PM_FLATTEN_SCENE_CAP caps what the flatten stage may write: one outline entry short of the need the answer is
    PM_ERR_CAPACITY with the exact needed size (outlines included); at the need itself the scene is made."""
    lib = pm._lib.load()
    ps = shapes(lambda k: 2 | style_bits(ROUND_CAP, ROUND_JOIN))
    aff = (C.c_double * 6)(*IDENTITY)

    def call(r):
        nbytes, nitems = C.c_size_t(0), C.c_uint32(0)
        st = lib.pm_flatten_and_encode(r._h, ps.paths.ctypes.data, len(ps.paths), ps.els.ctypes.data, len(ps.els), aff, 1.0, C.byref(nbytes), C.byref(nitems))
        return st, nbytes.value

    with pm.Renderer(0) as r:
        st, need = call(r)
        assert st == pm._lib.PM_OK
        want = r.download_scene()
        with pm.Renderer(0) as r0:
            plain_bytes, _ = r0.flatten_and_encode(plain(pm, ps), IDENTITY, 1.0)
        assert need > plain_bytes
        for cap in (need - 8, plain_bytes, plain_bytes - 8):  # (short of the outlines by one entry, by all of them, and of the points too)
            monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", str(cap))
            assert call(r) == (pm._lib.PM_ERR_CAPACITY, need)
        monkeypatch.setenv("PM_FLATTEN_SCENE_CAP", str(need))
        assert call(r) == (pm._lib.PM_OK, need)
        assert np.array_equal(r.download_scene(), want)
        monkeypatch.delenv("PM_FLATTEN_SCENE_CAP")


def test_stroke_small_invalid_style_fields(pm):
    with pm.Renderer(0) as r:
        bad = [style_bits(3, MITER), style_bits(BUTT, 3), style_bits(BUTT, MITER, half_bits(0.5)), style_bits(BUTT, MITER, 0x7C00),
               style_bits(BUTT, MITER, 0x7E00), style_bits(BUTT, MITER, half_bits(-4.0)), style_bits(ROUND_CAP, ROUND_JOIN, 0x3BFF)]
        for bits in bad:
            ps = shapes(lambda k: 2 | (bits if k == 3 else 0))
            with pytest.raises(pm._lib.PietMetalError) as ei:
                r.flatten_and_encode(ps, IDENTITY, 1.0)
            assert ei.value.status == pm._lib.PM_ERR_INVALID, hex(bits)
        # ... the same bits without the outline bit, or on a path without a stroke, are ignored
        for bits in bad:
            r.flatten_and_encode(shapes(lambda k: 2 | ((bits & ~np_stroke.OUTLINE) if k == 3 else 0)), IDENTITY, 1.0)
            r.flatten_and_encode(shapes(lambda k: (1 | bits) if k == 3 else 2), IDENTITY, 1.0)
        r.flatten_and_encode(shapes(lambda k: 2 | style_bits(BUTT, MITER, half_bits(1.0))), IDENTITY, 1.0)  # a limit of exactly 1 is valid


def test_stroke_small_cli_flag(pm, pmo, tmp_path):
    """--stroke-styles: the file's caps and joins are drawn; without it the picture is the round poly-lines'."""
    from piet_metal_amd import cli

    svg = tmp_path / "doc.svg"
    svg.write_text(SVG_DOC)
    outs = []
    for extra in ([], ["--stroke-styles"]):
        out = tmp_path / f"o{len(extra)}.png"
        assert cli.main([str(svg), str(out), "--width", "200", "--height", "150"] + extra) == 0
        outs.append(cli.read_png_rgba(str(out)))
    assert not np.array_equal(outs[0], outs[1])
    ps = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, flat_gradients=True, stroke_styles=True)
    aff, s = ps.fit_affine(200, 150)
    with pm.Renderer(0) as r:
        scene = styled_scene_checks(pm, r, ps, aff, s)
    assert np.array_equal(outs[1], pmo.render(scene, 200, 150))


# ---- the full cases ---------------------------------------------------------------------------------------------

AFFINES_1080 = [(4.0, 1.5, -1.5, 4.0, 700.0, -100.0), (2.0, 0.0, 0.0, 2.0, 100.0, 300.0)]


def full_checks(pm, pmo, ps, affine, scale, width, height, seed):
    with pm.Renderer(0) as r:
        scene = styled_scene_checks(pm, r, ps, affine, scale)
        n, _ = render_and_hit_checks(pmo, r, scene, width, height, 100_000, seed)
        assert n >= 100_000
        for k, aff in enumerate(AFFINES_1080):  # render -> reflatten -> render: every frame the oracle's
            scene_k = styled_scene_checks(pm, r, ps, aff, scale, reflatten=True)
            render_and_hit_checks(pmo, r, scene_k, width, height, 100_000, seed + 1 + k)
    return scene


@pytest.mark.parametrize("cap,join", COMBOS, ids=[f"{c}-{j}" for c, j in COMBOS])
def test_tiger_1080p_with_every_stroke_styled(pm, pmo, cap, join):
    wl = pm.workloads.tiger(1920, 1080)
    ps = wl.paths.with_stroke_style(cap, join)
    assert ((ps.paths["flags"] & np_stroke.OUTLINE) != 0).sum() == ((wl.paths.paths["flags"] & 2) != 0).sum() > 0
    full_checks(pm, pmo, ps, wl.affine, wl.width_scale, wl.width, wl.height, seed=300 + COMBOS.index((cap, join)))


def test_glyph_paths_given_strokes(pm, pmo):
    wl = pm.workloads.heldout_glyphs(4000, 1920, 1080)
    p = wl.paths.paths.copy()
    p["flags"] |= 2
    p["stroke_rgba"] = (p["fill_rgba"] ^ 0x00FFFF00) | 0xFF
    p["stroke_width"] = np.where(np.arange(len(p)) % 2 == 0, 1.5, 0.4).astype(np.float32) / np.float32(wl.width_scale)
    ps = pm.PathSet(p, wl.paths.els)
    sel = np.arange(len(p))
    ps = ps.with_stroke_style("round", "round", select=sel[sel % 3 == 0]).with_stroke_style("butt", "miter", 10.0, select=sel[sel % 3 == 1]) \
           .with_stroke_style("square", "bevel", select=sel[sel % 3 == 2])
    full_checks(pm, pmo, ps, wl.affine, wl.width_scale, wl.width, wl.height, seed=400)


SVG_DOC = """<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 400 300">
<style> .soft { stroke-linejoin: round; stroke-linecap: round } path { stroke-miterlimit: 10 } </style>
<g fill="none" stroke="#204080" stroke-width="9">
  <path d="M 20 40 L 120 30 L 60 90 L 180 100"/>
  <path class="soft" d="M 220 40 L 320 30 L 260 90 L 380 100"/>
  <g stroke-linecap="square" stroke-linejoin="bevel" stroke="#a02040">
    <path d="M 20 160 L 120 150 L 60 210 L 180 220"/>
    <rect x="230" y="150" width="120" height="70" style="stroke-linejoin: miter; stroke-miterlimit: 1.2"/>
    <polygon points="40,240 90,290 140,240" style="stroke-linecap:butt" fill="#ffcc00" stroke-opacity="0.5"/>
  </g>
  <path d="M 200 240 C 240 200 300 320 380 250 Z" stroke-linejoin="round" stroke-width="0.5"/>
</g></svg>"""


def test_svg_document_with_the_three_properties(pm, pmo):
    """stroke-linecap / stroke-linejoin / stroke-miterlimit through attributes, style="" and a class rule, inherited; without
    the parser flag the paths are what they were (no style bit)."""
    ps = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, stroke_styles=True)
    want = [style_bits(BUTT, MITER, half_bits(10.0)), style_bits(ROUND_CAP, ROUND_JOIN, half_bits(10.0)), style_bits(SQUARE, BEVEL, half_bits(10.0)),
            style_bits(SQUARE, MITER, half_bits(1.2)), style_bits(BUTT, BEVEL, half_bits(4.0)), style_bits(BUTT, ROUND_JOIN, half_bits(10.0))]
    assert [int(f) & np_stroke.style_bits(3, 3, 0xFFFF) for f in ps.paths["flags"]] == want
    off = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True)
    assert np.array_equal(off.paths, np_stroke.unstyled(ps.paths)) and np.array_equal(off.els, ps.els)
    aff, s = ps.fit_affine(1920, 1080)
    full_checks(pm, pmo, ps, aff, s, 1920, 1080, seed=500)
