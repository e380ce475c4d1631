"""Dashed strokes without a GPU: tests/np_dash.py (the numpy statement of decision D15) against hand-derived answers -- judged by
np_hit, which knows Fill items and nothing of strokes or dashes --, D15's entry-count closed form, its scale covariance, the SVG
front-end's two properties, the ABI and the Python helpers, the kernels' logic under wave64 emulation, and the kernels' listing."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_dash  # noqa: E402
import np_hit  # noqa: E402
import np_stroke  # noqa: E402
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE  # noqa: E402


def poly_scene(pts, width, rgba=0x204060FF):
    """One poly-line item by hand (src/lib.rs:60-68): {1, 16}{box}{item}{points}."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    be = struct.unpack("<I", struct.pack(">I", rgba))[0]
    return struct.pack("<II", 1, 16) + bytes(8) + struct.pack("<IIfII", 4, be, width, len(pts), 48) + bytes(12) + pts.tobytes()


def dashed_scene(pts, closed, width, cap, join, pattern, offset=0.0, ws=1.0):
    return np_dash.apply(poly_scene(pts, width), [(closed, cap, join, 0, (pattern, offset, ws))])


def inside(pts, closed, width, cap, join, pattern, offset, q):
    sc = dashed_scene(pts, closed, width, cap, join, pattern, offset)
    a = np_hit.item_inside(sc, 0, np.asarray(q, np.float32))
    assert np.array_equal(a, np_hit.item_inside(sc, 0, np.asarray(q, np.float32), brute=True))
    return a.tolist()


# ---- 1. known answers, derived by hand ------------------------------------------------------------------------

LINE = [(10, 50), (110, 50)]  # width 4: hw = 2


def test_a_line_is_cut_where_the_pattern_says():
    # offset 0: the dashes cover x in [10, 30], [40, 60], [70, 90], [100, 110]
    q = [(20, 51.5), (105, 50), (35, 50), (20, 52.5), (110.5, 50)]
    assert inside(LINE, False, 4.0, BUTT, MITER, [20, 10], 0.0, q) == [True, True, False, False, False]
    # offset 5: [10, 25], [35, 55], ...
    assert inside(LINE, False, 4.0, BUTT, MITER, [20, 10], 5.0, [(24, 50), (36, 50), (30, 50)]) == [True, True, False]
    # offset -5: the pattern starts 5 later: [15, 35], ...
    assert inside(LINE, False, 4.0, BUTT, MITER, [20, 10], -5.0, [(16, 50), (12, 50)]) == [True, False]
    # an odd count repeats once
    assert dashed_scene(LINE, False, 4.0, BUTT, MITER, [10]) == dashed_scene(LINE, False, 4.0, BUTT, MITER, [10, 10])
    # round caps add hw beyond a dash's end (the first dash ends at x = 30)
    assert inside(LINE, False, 4.0, ROUND_CAP, MITER, [20, 10], 0.0, [(31.5, 50), (32.5, 50)]) == [True, False]
    assert inside(LINE, False, 4.0, BUTT, MITER, [20, 10], 0.0, [(31.5, 50)]) == [False]
    assert len(np_dash.cut(LINE, False, [20, 10], 0.0, 1.0)) == 4


ELL = [(20, 20), (120, 20), (120, 120)]  # width 10; the corner (120, 20) lies at length 100, its miter tip at (125, 15)


def test_a_corner_gets_its_join_only_inside_a_dash():
    tip = [(124.5, 15.5), (121.5, 17.5)]
    # [30, 20], offset 0: dashes [0, 30], [50, 80], [100, 130], ...: the corner is a dash START -- a butt end, no join
    assert inside(ELL, False, 10.0, BUTT, MITER, [30, 20], 0.0, tip) == [False, False]
    # offset 10: [-10, 20], [40, 70], [90, 120], [140, 170], [190, 200]: the corner is inside a dash
    assert inside(ELL, False, 10.0, BUTT, MITER, [30, 20], 10.0, tip) == [True, True]
    polys = np_dash.cut(ELL, False, [30, 20], 10.0, 1.0)
    assert [len(p) for p in polys] == [2, 2, 3, 2, 2] and polys[2].tolist() == [[110, 20], [120, 20], [120, 40]]


RECT = [(20, 20), (120, 20), (120, 80), (20, 80)]  # closed, perimeter 320, width 10


def test_a_closed_path_merges_the_dash_across_its_start():
    corner = [(15.5, 15.5)]  # inside the miter at the start vertex (20, 20), outside every butt-ended dash
    # [40, 40], offset 20: [-20, 20], [60, 100], ..., [300, 340]: the last and the first are one poly-line through (20, 20)
    assert inside(RECT, True, 10.0, BUTT, MITER, [40, 40], 20.0, corner) == [True]
    polys = np_dash.cut(RECT, True, [40, 40], 20.0, 1.0)
    assert len(polys) == 4 and polys[0].tolist() == [[20, 40], [20, 20], [20, 20], [40, 20]]
    # offset 0: [0, 40], ..., [240, 280]: nothing reaches the end, no merge
    assert inside(RECT, True, 10.0, BUTT, MITER, [40, 40], 0.0, corner) == [False]
    assert len(np_dash.cut(RECT, True, [40, 40], 0.0, 1.0)) == 4
    # a first dash that covers the whole walk: the D14 closed outline, byte for byte
    assert np_dash.cut(RECT, True, [320, 5], 0.0, 1.0) == np_dash.CLOSED_WHOLE
    want = np_stroke.apply(poly_scene(RECT, 10.0), [(True, BUTT, MITER, 0)])
    assert dashed_scene(RECT, True, 10.0, BUTT, MITER, [320, 5]) == want
    assert dashed_scene(RECT, True, 10.0, BUTT, MITER, [400, 5], 30.0) == want
    assert isinstance(np_dash.cut(RECT, True, [319, 5], 0.0, 1.0), list)


def test_what_is_not_dashed_is_the_d14_outline():
    for cap, join in ((BUTT, MITER), (ROUND_CAP, ROUND_JOIN), (SQUARE, BEVEL)):
        for pts, closed in ((ELL, False), (RECT, True)):
            want = np_stroke.apply(poly_scene(pts, 10.0), [(closed, cap, join, 0)])
            assert dashed_scene(pts, closed, 10.0, cap, join, [0, 0]) == want          # G == 0
            assert dashed_scene(pts, closed, 10.0, cap, join, [5, 0, 3, 0]) == want    # every gap 0
            assert dashed_scene(pts, closed, 10.0, cap, join, [5, 3], ws=1e-7) == want  # (scaled to nothing: G == 0)
        dot = [(5, 5), (5, 5)]
        assert dashed_scene(dot, False, 10.0, cap, join, [5, 3]) == np_stroke.apply(poly_scene(dot, 10.0), [(False, cap, join, 0)])  # T == 0


def test_zero_length_dashes_are_dots():
    q = [(20, 50), (21.5, 50), (20, 51.5), (30, 48.6), (25, 50), (22.5, 50), (10, 50), (8.6, 50)]
    assert inside(LINE, False, 4.0, ROUND_CAP, MITER, [0, 10], 0.0, q) == [True, True, True, True, False, False, True, True]
    assert inside(LINE, False, 4.0, BUTT, MITER, [0, 10], 0.0, q) == [False] * 8
    polys = np_dash.cut(LINE, False, [0, 10], 0.0, 1.0)
    assert len(polys) == 10 and all(len(p) == 2 and (p[0] == p[1]).all() for p in polys)  # at 10, 20, ..., 100; none at the end, 110
    # square caps: D14's axis-aligned square about the point
    assert inside(LINE, False, 4.0, SQUARE, MITER, [0, 10], 0.0, [(21.9, 51.9), (22.1, 50)]) == [True, False]


def test_a_path_shorter_than_its_first_gap_is_an_empty_item():
    short = [(10, 50), (60, 50)]
    assert np_dash.cut(short, False, [5, 100], 5.0, 1.0) == []  # the dash [-5, 0] ends where the path begins; the next starts at 100
    sc = dashed_scene(short, False, 4.0, ROUND_CAP, ROUND_JOIN, [5, 100], 5.0)
    assert len(sc) == len(poly_scene(short, 4.0)) and np_hit.flat_items(sc)[0][1] == (0, 0, 0, 0)
    assert struct.unpack_from("<8I", sc, 16)[:2] == (3, 2) and struct.unpack_from("<8I", sc, 16)[3] == 0


# ---- 2. the entry count and scale covariance --------------------------------------------------------------------

def random_case(rng):
    n = int(rng.integers(1, 12))
    pts = rng.integers(0, 2048, (n, 2)) / 8.0  # multiples of 1/8 in [0, 256)
    for _ in range(int(rng.integers(0, 3))):   # repeated points
        i = int(rng.integers(0, len(pts)))
        pts = np.insert(pts, i, pts[i], axis=0)
    pattern = (rng.integers(0, 400, int(rng.integers(1, 7))) / 8.0).tolist()
    offset = float(rng.integers(-800, 800)) / 8.0
    return pts, bool(rng.integers(0, 2)), pattern, offset


def test_the_entry_count_is_d15s_closed_form():
    rng = np.random.default_rng(15)
    seen_dashed = seen_merged = 0
    for k in range(200):
        pts, closed, pattern, offset = random_case(rng)
        cap, join = [BUTT, ROUND_CAP, SQUARE][k % 3], [MITER, ROUND_JOIN, BEVEL][(k // 3) % 3]
        width = [1.0, 4.0, 12.0][k % 3]
        entries, _ = np_dash.outline_dashed(pts, closed, width, cap, join, 0, pattern, offset, 1.0)
        polys = np_dash.cut(pts, closed, pattern, offset, 1.0)
        L = np_stroke.level(np.float64(np.float32(width) * np.float32(0.5)))
        if isinstance(polys, str):
            assert len(entries) == np_stroke.entry_count(len(pts), closed, cap, join, L)
            continue
        seen_dashed += 1
        assert len(entries) == np_dash.entry_count(polys, cap, join, L)
        # separators: every piece's index points at its own first entry, counted from the item's entry 0
        sep = np.flatnonzero(entries[:, 0] == np_stroke.NAN_BITS)
        firsts = np.concatenate([[0], sep[:-1] + 1]) if len(sep) else sep
        assert np.array_equal(entries[sep, 1], firsts)
        W, Q = np_dash.walk(pts, closed)
        if closed and len(polys) and len(polys[0]) >= 4 and any((polys[0][i] == W[-1]).all() and (polys[0][i + 1] == W[0]).all() for i in range(1, len(polys[0]) - 2)):
            seen_merged += 1
    assert seen_dashed >= 100 and seen_merged >= 5


def test_scale_covariance_bit_for_bit():
    """Coordinates, width, pattern and offset all x 2 -- exact in f32 and, for segments of lengths on the 2^-16 grid (axis-aligned
    ones and 3-4-5 ones here), in the integer walk -- give the outline x 2 bit for bit: what the integer sum buys.  (Styles without
    fans: a fan's level depends on the width.)"""
    rng = np.random.default_rng(16)
    steps = [(1, 0), (0, 1), (-1, 0), (0, -1), (3, 4), (4, -3), (-3, -4), (-4, 3), (5, 12), (-12, 5)]
    for k in range(60):
        closed = bool(k % 2)
        moves = [np.array(steps[int(rng.integers(0, len(steps)))]) * (int(rng.integers(1, 40)) / 8.0) for _ in range(int(rng.integers(1, 6)))]
        if closed:  # (walk the same steps back in another order: the closing segment is one of them, of an exact length too)
            moves = moves + [-moves[i] for i in rng.permutation(len(moves))]
        pts = 128.0 + np.concatenate([np.zeros((1, 2)), np.cumsum(moves, axis=0)])
        if closed:
            pts = pts[:-1]
        pattern = (rng.integers(0, 100, int(rng.integers(1, 5))) / 8.0).tolist()
        offset = float(rng.integers(-80, 80)) / 8.0
        cap, join = [(BUTT, MITER), (SQUARE, BEVEL), (BUTT, BEVEL)][k % 3]
        e1, _ = np_dash.outline_dashed(pts, closed, 3.0, cap, join, 0, pattern, offset, 1.0)
        e2, _ = np_dash.outline_dashed(pts * 2, closed, 6.0, cap, join, 0, [2 * v for v in pattern], 2 * offset, 1.0)
        e3, _ = np_dash.outline_dashed(pts * 2, closed, 6.0, cap, join, 0, pattern, offset, 2.0)  # ... or through width_scale
        assert len(e1) == len(e2) == len(e3)
        sep = e1[:, 0] == np_stroke.NAN_BITS
        assert np.array_equal(e1[sep], e2[sep]) and np.array_equal(e2, e3)
        f1, f2 = e1[~sep].view(np.float32), e2[~sep].view(np.float32)
        assert np.array_equal((f1 * np.float32(2)).view(np.uint32), f2.view(np.uint32))


# ---- 3. the SVG front-end -------------------------------------------------------------------------------------

SVG_DOC = """<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 400 300">
<style> .dots { stroke-dasharray: 0 14 } </style>
<g fill="none" stroke="#204080" stroke-width="8" stroke-dasharray="20,10">
  <path d="M 20 40 L 120 30"/>
  <path class="dots" d="M 220 40 L 320 30"/>
  <g stroke-dashoffset="7">
    <path d="M 30 150 L 150 150" style="stroke-dasharray: 15 5 5"/>
    <path d="M 30 170 L 150 170" stroke-dasharray="none"/>
    <path d="M 30 190 L 150 190" stroke-dasharray="12, -3"/>
    <path d="M 30 210 L 150 210" stroke-dasharray="1mm 2px" stroke-dashoffset="-2.5"/>
    <g transform="scale(2)"><path d="M 30 120 L 150 120"/></g>
  </g>
  <path d="M 30 250 L 150 250" fill="#ff0000" stroke="none"/>
</g></svg>"""


def table_of(ps):
    return {int(d["path"]): (ps.dash_values[int(d["first"]) : int(d["first"]) + int(d["count"])].tolist(), float(d["offset"])) for d in ps.dashes}


def test_svg_dash_properties_need_their_flag(pm):
    ps = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, stroke_styles=True, stroke_dashes=True)
    mm = float(np.float32(96.0 / 25.4))
    assert table_of(ps) == {0: ([20.0, 10.0], 0.0), 1: ([0.0, 14.0], 0.0), 2: ([15.0, 5.0, 5.0], 7.0), 5: ([mm, 2.0], -2.5),
                            6: ([40.0, 20.0], 14.0)}  # (3: none; 4: a negative entry means none; 6: scaled by sqrt|det| like its width; 7: no stroke)
    assert float(ps.paths["stroke_width"][6]) == 16.0 and len(ps.paths) == 8
    assert np.all(np.diff(ps.dashes["path"].astype(np.int64)) > 0)
    # without the flag the parse is what it is today
    styled = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, stroke_styles=True)
    assert len(styled.dashes) == 0 and len(styled.dash_values) == 0
    assert np.array_equal(styled.paths, ps.paths) and np.array_equal(styled.els, ps.els)
    # the flag depends on PM_SVG_STROKE_STYLES
    with pytest.raises(pm._lib.PietMetalError) as ei:
        pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, stroke_dashes=True)
    assert ei.value.status == pm._lib.PM_ERR_INVALID


def test_the_tiger_has_no_dashes_either_way(pm):
    text = open(os.path.join(ROOT, "piet_metal_amd", "assets", "Ghostscript_Tiger.svg"), "rb").read()
    styled = pm.PathSet.from_svg(text, stroke_styles=True)
    dashed = pm.PathSet.from_svg(text, stroke_styles=True, stroke_dashes=True)
    assert len(dashed.dashes) == 0 and np.array_equal(styled.paths, dashed.paths) and np.array_equal(styled.els, dashed.els)


# ---- 4. the ABI and the Python helpers --------------------------------------------------------------------------

def test_abi_is_additive(pm):
    lib = pm._lib.load()
    assert lib.pm_abi_version() == 600

    class Dash(C.Structure):
        _fields_ = [("path", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32), ("offset", C.c_float)]

    assert C.sizeof(Dash) == 16 == pm.PathSet.DASH_DTYPE.itemsize and pm.PathSet.PATH_DTYPE.itemsize == 24 and pm.PathSet.EL_DTYPE.itemsize == 56
    assert [pm.PathSet.DASH_DTYPE.fields[k][1] for k in ("path", "first", "count", "offset")] == [0, 4, 8, 12]
    for name in ("pm_flatten_and_encode_dashed", "pm_svg_dashes", "pm_svg_n_dashes", "pm_svg_dash_values", "pm_svg_n_dash_values"):
        assert getattr(lib, name) is not None
    assert pm._lib.PM_SVG_STROKE_DASHES == 16 and pm._lib.PM_SVG_STROKE_STYLES == 8


def test_pathset_helpers_carry_the_table(pm):
    from path_sets import pathset

    M, L = 0, 1
    a = pathset(([(M, 0, 0), (L, 9, 0)], 2), ([(M, 0, 5), (L, 9, 5)], 1), ([(M, 0, 9), (L, 9, 9)], 3))
    assert len(a.dashes) == 0 and len(a.dash_values) == 0  # PathSet(paths, els) keeps working
    assert len(a.with_dashes([4, 2]).dashes) == 0          # no outlined stroke yet: left alone
    s = a.with_stroke_style("round", "bevel")
    d = s.with_dashes([4, 2], 1.5)
    assert table_of(d) == {0: ([4.0, 2.0], 1.5), 2: ([4.0, 2.0], 1.5)}
    d2 = d.with_dashes([1, 2, 3], select=[2]).with_stroke_style("butt", "miter", select=[0])
    assert table_of(d2) == {0: ([4.0, 2.0], 1.5), 2: ([1.0, 2.0, 3.0], 0.0)}
    assert table_of(d2.transformed((2, 0, 0, 2, 5, 5))) == table_of(d2)
    both = pm.PathSet.concat([d2, a, d])
    assert table_of(both) == {0: ([4.0, 2.0], 1.5), 2: ([1.0, 2.0, 3.0], 0.0), 6: ([4.0, 2.0], 1.5), 8: ([4.0, 2.0], 1.5)}
    assert np_dash.specs_from_pathset(both, 2.0)[3][4] == ([1.0, 2.0, 3.0], 0.0, 2.0)
    d.viewbox, d.size = (0.0, 0.0, 10.0, 10.0), (10.0, 10.0)
    kept = d.with_dashes([3]).with_stroke_style("square", "round")
    assert kept.viewbox == d.viewbox and kept.fit_affine(20, 20) == d.fit_affine(20, 20) and table_of(kept) == {0: ([3.0], 0.0), 2: ([3.0], 0.0)}
    for bad in ([], [1.0] * 33, [-1.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            s.with_dashes(bad)
    with pytest.raises(ValueError):
        s.with_dashes([1, 2], float("inf"))


# ---- 5. the kernels' logic under wave64 emulation -------------------------------------------------------------

def test_dash_kernels_under_wave64_emulation(built):
    """The `small` cases of tests/test_dash_gpu.py -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_dash_gpu.py"), "-q", "-x", "-m", "gpu", "-k", "small", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "14 passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- 6. the kernels' listing ------------------------------------------------------------------------------------

def test_the_dash_kernels_use_no_scratch(tmp_path):
    """KDashCount and KDash by the flags the library is built with: no private segment (the pattern's prefixes and the step's
    segment records live in LDS, no indexed local array) and VGPRs within what a workgroup of 256, the launch bound, can be given."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_flatten.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_flatten.hip"), "-o", out], stderr=subprocess.DEVNULL)
    found = set()
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.M | re.S):
        name = re.search(r"KDash(?:Count)?(?=E)", m.group(1))  # (the mangled name: <length><name>E<arguments>)
        if not name:
            continue
        found.add(name.group(0))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        print(name.group(0), "vgpr", vgpr, "scratch", scratch)
        assert scratch == 0 and vgpr <= 256, (m.group(1), scratch, vgpr)
    assert found == {"KDashCount", "KDash"}
