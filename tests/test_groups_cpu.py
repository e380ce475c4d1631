"""Per-group affines in re-flatten (decision D16) without a GPU: the helper that states the expected bytes (tests/np_groups.py)
is proven against the oracle before it judges the device, the PathSet plumbing, the SVG front-end's top-level groups against an
independent Python walker, the CLI's offsets, the grouped kernels' listing, and the library's new symbols."""
import os
import re
import shutil
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_dash  # noqa: E402
import np_groups  # noqa: E402
import np_scene  # noqa: E402
import np_stroke  # noqa: E402
import path_sets  # noqa: E402
from np_stroke import style_bits  # noqa: E402

RANDOM_SEEDS = list(range(400, 436))


def _ok_edge_cases():
    return {k: c for k, c in path_sets.edge_cases().items() if c.status == 0}  # (the two rejected sets have no scene)


# ---- 1. the splice ----------------------------------------------------------------------------------------------

def _whole(pmo, case):
    scene, n_items = pmo.scene_from_paths(pmo.scaled_paths(case.ps.paths, case.scale), case.ps.els, case.affine)
    return scene, n_items


def _check_equal_groups(pmo, case, rng, both):
    n = len(case.ps.paths)
    want, n_items = _whole(pmo, case)
    gmap = rng.integers(0, 4, n).astype(np.uint32)
    aff, ws = [case.affine] * 4, [case.scale] * 4
    got = np_groups.scene(case.ps, gmap, aff, ws, pmo.scene_from_paths)
    assert got[1] == n_items and np.array_equal(got[0], want)
    if both:  # the other restatement gives the same splice
        other = np_groups.scene(case.ps, gmap, aff, ws, np_scene.scene_from_paths)
        assert other[1] == n_items and np.array_equal(other[0], want) and np.array_equal(other[2], got[2])


@pytest.mark.parametrize("name", sorted(_ok_edge_cases()))
def test_splice_of_equal_groups_is_the_whole_scene_edge_cases(pmo, name):
    case = _ok_edge_cases()[name]
    _check_equal_groups(pmo, case, np.random.default_rng(len(name)), both=name != "counts_on_sixth_power_boundaries")


def test_splice_of_equal_groups_is_the_whole_scene_random(pmo):
    for seed in RANDOM_SEEDS:
        _check_equal_groups(pmo, path_sets.random_case(seed), np.random.default_rng(seed), both=seed % 6 == 0)


def test_splice_differs_between_groups_and_agrees_between_restatements(pmo):
    """Two groups under different views: the oracle's and the numpy restatement's one-path scenes splice to the same bytes, and
    those are neither group's whole-set scene."""
    case = path_sets.random_case(402)
    ps, n = case.ps, len(case.ps.paths)
    assert n >= 2
    gmap = np.arange(n, dtype=np.uint32) % 2
    aff, ws = [case.affine, case.affine2], [case.scale, 0.25]
    a = np_groups.scene(ps, gmap, aff, ws, pmo.scene_from_paths)
    b = np_groups.scene(ps, gmap, aff, ws, np_scene.scene_from_paths)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for k in range(2):
        whole, _ = pmo.scene_from_paths(pmo.scaled_paths(ps.paths, ws[k]), ps.els, aff[k])
        assert not np.array_equal(a[0], whole)
    assert len(a[2]) == a[1] and np.all(np.diff(a[2].astype(np.int64)) >= 0)  # items in path order


def test_splice_of_equal_groups_with_styles_and_dashes(pm, pmo):
    """Step 4: with one width_scale everywhere the per-path specs are np_dash's own for the whole set."""
    from test_stroke_gpu import shapes

    ps = shapes(lambda k: (3 if k % 3 == 0 else 2) | style_bits(k % 3, (k // 3) % 3)).with_dashes([6, 3, 2], -4.0, select=[0, 3, 9])
    aff, scale = (1.3, 0.5, -0.5, 1.3, 60.0, -20.0), 2.5
    plain, _ = pmo.scene_from_paths(pmo.scaled_paths(np_stroke.unstyled(ps.paths), scale), ps.els, aff)
    want = np.frombuffer(np_dash.apply(plain, np_dash.specs_from_pathset(ps, scale)), np.uint8)
    got = np_groups.scene(ps, np.arange(len(ps.paths)) % 3, [aff] * 3, [scale] * 3, pmo.scene_from_paths)
    assert np.array_equal(got[0], want)
    undashed = pm.PathSet(ps.paths, ps.els)
    want = np.frombuffer(np_stroke.apply(plain, np_stroke.specs_from_paths(ps.paths, ps.els)), np.uint8)
    assert np.array_equal(np_groups.scene(undashed, None, [aff], [scale], pmo.scene_from_paths)[0], want)


# ---- 2. PathSet ------------------------------------------------------------------------------------------------

def test_pathset_carries_and_offsets_groups(pm):
    a = path_sets.random_case(403).ps
    b = path_sets.random_case(404).ps
    assert a.groups is None and a.n_groups() == 1
    ga = np.arange(len(a.paths)) % 3 if len(a.paths) >= 3 else np.zeros(len(a.paths), int)
    ag = a.with_groups(ga)
    assert a.groups is None and ag.groups.dtype == np.uint32 and np.array_equal(ag.groups, ga) and ag.n_groups() == int(ga.max()) + 1
    for copy in (ag._like(ag.paths, ag.els), ag.with_stroke_style("round", "bevel"), ag.with_stroke_style().with_dashes([4, 2]), ag.fills_only(),
                 ag.transformed((2.0, 0.0, 0.0, 2.0, 1.0, 1.0))):
        assert np.array_equal(copy.groups, ga)
    assert ag.with_groups(None).groups is None
    bg = b.with_groups(np.zeros(len(b.paths), np.uint32) + 1)  # (group 0 unused: two groups all the same)
    cat = pm.PathSet.concat([ag, b, bg, a])
    na, nb = len(a.paths), len(b.paths)
    g0 = ag.n_groups()
    want = np.concatenate([ga, np.full(nb, g0), np.full(nb, g0 + 1 + 1), np.full(na, g0 + 1 + 2)])
    assert np.array_equal(cat.groups, want) and cat.groups.dtype == np.uint32 and cat.n_groups() == g0 + 4
    assert pm.PathSet.concat([a, b]).groups is None
    for bad in (np.zeros(len(a.paths) + 1, int), np.full(len(a.paths), -1), np.zeros(len(a.paths), float)):
        with pytest.raises(ValueError):
            a.with_groups(bad)


# ---- 3. SVG: top-level groups against a Python walker -------------------------------------------------------------

SVG = """<?xml version="1.0"?>
<!-- a comment is no element -->
<svg xmlns="http://www.w3.org/2000/svg" xmlns:xlink="http://www.w3.org/1999/xlink" viewBox="0 0 200 200">
  <defs>
    <path id="leaf" d="M0 0 L10 0 L5 8 Z" fill="#0a0"/>
    <g id="pair"><rect x="0" y="0" width="4" height="4" fill="red"/><circle cx="8" cy="2" r="2" fill="blue"/></g>
  </defs>
  <g fill="#123">
    <path d="M10 10 L30 10 L20 30 Z"/>
    <g transform="translate(40 0)"><rect x="0" y="0" width="10" height="10"/><g><path d="M0 20 L10 20 L5 28 Z" fill="#456"/></g></g>
  </g>
  <path d="M100 100 L120 100 L110 120 Z" fill="#789"/>
  <title>no drawing</title>
  <g style="display:none"><path d="M1 1 L2 2 L3 1 Z" fill="black"/></g>
  <g fill="#111"><path d="M5 150 L9 150 L7 160 Z" display="none"/><path d="M15 150 L19 150 L17 160 Z"/></g>
  <use xlink:href="#pair" x="150" y="20"/>
  <g><use href="#leaf" x="20" y="170"/><use href="#pair" x="60" y="170"/><path d="M90 170 L99 170 L95 180 Z" fill="#222"/></g>
  <svg x="0" y="0"><path d="M150 150 L160 150 L155 160 Z" fill="#333"/></svg>
</svg>
"""

SHAPES = {"path", "rect", "circle", "ellipse", "line", "polyline", "polygon"}


def walk_groups(text):
    """Per drawn element, in document order with every <use> expanded where it stands: the ordinal of the element child of the
    outermost <svg> it belongs to.  Every shape of these documents has a paint (own or inherited), so an element is drawn unless
    it or an ancestor -- in the tree the <use> stands in -- says display: none."""
    root = ET.fromstring(text)
    local = lambda e: e.tag.split("}")[-1]
    ids = {e.get("id"): e for e in root.iter() if e.get("id")}
    out = []

    def hidden(e):
        return e.get("display") == "none" or "display:none" in (e.get("style") or "").replace(" ", "")

    def visit(e, ordinal, depth):
        if hidden(e) or local(e) in ("defs", "title", "desc", "symbol", "clipPath", "mask"):
            return
        if local(e) in SHAPES:
            out.append(ordinal)
        elif local(e) == "use":
            ref = e.get("href") or e.get("{http://www.w3.org/1999/xlink}href")
            if ref and ref[1:] in ids and depth < 8:
                visit(ids[ref[1:]], ordinal, depth + 1)
        else:
            for c in e:
                visit(c, ordinal, depth)

    for ordinal, child in enumerate(root):
        visit(child, ordinal, 0)
    return out


def test_svg_top_level_groups_match_the_walker(pm):
    want = walk_groups(SVG)
    assert want == [1, 1, 1, 2, 5, 6, 6, 7, 7, 7, 7, 8]  # nested <g>, a lone <path>, display:none, <use> into <defs>, a nested <svg>
    ps = pm.PathSet.from_svg(SVG, spec_defaults=True, groups=True)
    assert ps.groups.dtype == np.uint32 and ps.groups.tolist() == want
    assert pm.PathSet.from_svg(SVG, spec_defaults=True).groups is None
    # every shape of the document has a fill property, own or inherited: the reference's fill rule draws the same elements
    assert pm.PathSet.from_svg(SVG, groups=True).groups.tolist() == want
    # a document without an <svg> element: its own top-level elements count
    frag = '<g fill="red"><path d="M0 0 L1 0 L1 1 Z"/></g><path fill="blue" d="M2 2 L3 2 L3 3 Z"/><rect fill="red" width="2" height="2"/>'
    assert pm.PathSet.from_svg(frag, groups=True).groups.tolist() == [0, 1, 2]
    tiger = pm.PathSet.tiger(groups=True)
    assert len(tiger.groups) == len(tiger.paths) and pm.PathSet.tiger().groups is None


def test_cli_explode_offsets(pm):
    from piet_metal_amd import cli

    ps = pm.PathSet.from_svg(SVG, spec_defaults=True, groups=True)
    away = cli.group_offsets(ps)
    assert away.shape == (ps.n_groups(), 2) and not away[0].any() and not away[3].any()  # (<defs>, <title>: no path, no move)
    # child 2 is the lone triangle (100,100) (120,100) (110,120); the document's box is that of all coordinates
    xs = np.concatenate([ps.els["p"][ps.els["tag"] <= 1][:, 0], ps.els["p"][ps.els["tag"] == 3][:, 0::2].ravel()])
    ys = np.concatenate([ps.els["p"][ps.els["tag"] <= 1][:, 1], ps.els["p"][ps.els["tag"] == 3][:, 1::2].ravel()])
    doc = np.array([(xs.min() + xs.max()) / 2, (ys.min() + ys.max()) / 2])
    assert np.allclose(away[2], np.array([110.0, 110.0]) - doc, rtol=0, atol=1e-12)
    base = (2.0, 0.5, -0.5, 2.0, 7.0, 9.0)
    affs = cli.explode_affines(base, away * 0.5)
    for g in range(len(affs)):  # base after translate(shift): the same as transforming the shifted point
        dx, dy = away[g] * 0.5
        want = (2.0, 0.5, -0.5, 2.0, 7.0 + 2.0 * dx - 0.5 * dy, 9.0 + 0.5 * dx + 2.0 * dy)
        assert np.allclose(affs[g], want, rtol=0, atol=1e-12)
    assert np.array_equal(cli.explode_affines(base, away * 0.0), np.tile(np.array(base), (len(away), 1)))


# ---- 4. the grouped kernels' listing ------------------------------------------------------------------------------

def test_the_grouped_kernels_use_no_scratch(tmp_path):
    """The K...Grouped instantiations by the flags the library is built with: as their uniform forms, no private segment and
    VGPRs within what a workgroup of 256, the launch bound, can be given; the uniform forms are still there under their names."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_flatten.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_flatten.hip"), "-o", out], stderr=subprocess.DEVNULL)
    found, uniform = set(), set()
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.M | re.S):
        plain = re.search(r"\d(K(?:Count|Points|Items|OutlineCount|Outline|DashCount|Dash))(?=E)", m.group(1))
        if plain:
            uniform.add(plain.group(1))
        name = re.search(r"\d(K(?:Count|Points|Items|OutlineCount|Outline|DashCount|Dash)Grouped)(?=E)", m.group(1))  # (<length><name>E<arguments>)
        if not name:
            continue
        found.add(name.group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        print(name.group(1), "vgpr", vgpr, "scratch", scratch)
        assert scratch == 0 and vgpr <= 256, (m.group(1), scratch, vgpr)
    kernels = {"KCount", "KPoints", "KItems", "KOutlineCount", "KOutline", "KDashCount", "KDash"}
    assert found == {k + "Grouped" for k in kernels} and uniform == kernels


# ---- 5. the library's symbols ---------------------------------------------------------------------------------------

def test_library_exports_and_binds_the_group_symbols(pm):
    lib = pm._lib.load()
    for name in ("pm_path_groups", "pm_reflatten_groups", "pm_svg_path_groups"):
        assert name in pm._lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == pm._lib.SIGNATURES[name][1]
    import ctypes as C

    assert C.sizeof(pm._lib.GroupXform) == 56 == pm.Renderer.GROUP_XFORM_DTYPE.itemsize
    assert [pm.Renderer.GROUP_XFORM_DTYPE.fields[k][1] for k in ("m", "width_scale", "reserved")] == [0, 48, 52]
    header = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    assert "int pm_path_groups(" in header and "int pm_reflatten_groups(" in header and "pm_svg_path_groups(" in header
    assert "#define PM_ABI_VERSION 600u" in header  # (no struct layout changed)
    # without a device the two calls still answer for their arguments
    assert lib.pm_path_groups(None, None, 0) == pm._lib.PM_ERR_INVALID and lib.pm_reflatten_groups(None, None, 0, None, None) == pm._lib.PM_ERR_INVALID
