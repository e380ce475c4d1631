"""Stroke caps, joins and miter limits without a GPU: tests/np_stroke.py (the numpy statement of decision D14) against hand-derived
answers and against derived containment margins on random poly-lines -- judged by np_hit, which knows Fill items and nothing of
strokes' styles --, the SVG front-end's three properties, the kernels' logic under wave64 emulation, and the kernels' listing.

Margins (derived, not measured): a fan is inscribed in its circle and misses at most the sagitta, which D14's level table keeps
within the flatten tolerance 0.1; storing a point as f32 moves it by at most half an ulp of its coordinate (2^-17 below 256).  So a
point closer than hw - 0.11 to the stroke's skeleton is inside and one farther than hw + 1e-3 is outside."""
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
import np_hit  # noqa: E402
import np_stroke  # noqa: E402
from np_stroke import BEVEL, BUTT, MITER, ROUND_CAP, ROUND_JOIN, SQUARE, half_bits, style_bits  # noqa: E402

STYLES = [(c, j) for c in (BUTT, ROUND_CAP, SQUARE) for j in (MITER, ROUND_JOIN, BEVEL)]


def poly_scene(pts, width, rgba=0x204060FF):
    """One poly-line item by hand (src/lib.rs:60-68): {1, 16}{box}{item}{points}."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    be = struct.unpack("<I", struct.pack(">I", rgba))[0]
    return struct.pack("<II", 1, 16) + bytes(8) + struct.pack("<IIfII", 4, be, width, len(pts), 48) + bytes(12) + pts.tobytes()


def outline_scene(pts, closed, width, cap, join, miter=0):
    return np_stroke.apply(poly_scene(pts, width), [(closed, cap, join, miter)])


def inside(pts, closed, width, cap, join, q, miter=0):
    sc = outline_scene(pts, closed, width, cap, join, miter)
    a = np_hit.item_inside(sc, 0, np.asarray(q, np.float32))
    assert np.array_equal(a, np_hit.item_inside(sc, 0, np.asarray(q, np.float32), brute=True))
    return a.tolist()


# ---- 1. known answers -----------------------------------------------------------------------------------------

ELL = [(20, 20), (120, 20), (120, 120)]  # turns by 90 degrees at (120, 20); width 10: the outer corner is (125, 15)


def test_miter_tip_bevel_and_the_limit():
    tip = [(124.5, 15.5), (121.5, 17.5), (126.0, 14.0)]  # just inside the tip; inside the bevel too; beyond the tip
    assert inside(ELL, False, 10.0, BUTT, MITER, tip) == [True, True, False]
    assert inside(ELL, False, 10.0, BUTT, BEVEL, tip) == [False, True, False]
    assert inside(ELL, False, 10.0, BUTT, ROUND_JOIN, tip) == [False, True, False]  # |(4.5, -4.5)| = 6.4 > 5
    # 1 / sin(90 / 2) = 1.41421...: binary16 has 1.4140625 just below it and 1.4150390625 just above
    below, above = half_bits(1.4140625), half_bits(1.4150390625)
    assert np_stroke.miter_limit(below) == 1.4140625 and np_stroke.miter_limit(above) == 1.4150390625
    assert inside(ELL, False, 10.0, BUTT, MITER, tip, miter=below) == [False, True, False]
    assert inside(ELL, False, 10.0, BUTT, MITER, tip, miter=above) == [True, True, False]
    assert inside(ELL, False, 10.0, BUTT, MITER, tip, miter=half_bits(1.0)) == [False, True, False]
    # the turn the other way round (the same corner walked backwards): the tip is on the same side
    assert inside(ELL[::-1], False, 10.0, BUTT, MITER, tip) == [True, True, False]


def test_the_three_caps_at_an_open_end():
    line = [(20, 50), (100, 50)]  # hw = 5; the end is at x = 100
    q = [(99.8, 50.3), (100.2, 50.3), (104.9, 50.3), (104.9, 54.9), (105.1, 50.3), (105.05, 55.05), (19.8, 50.3), (15.1, 45.1), (14.9, 50.3)]
    assert inside(line, False, 10.0, BUTT, MITER, q) == [True, False, False, False, False, False, False, False, False]
    assert inside(line, False, 10.0, SQUARE, MITER, q) == [True, True, True, True, False, False, True, True, False]
    # round: inside at hw - 0.11 along any direction of the half plane beyond the end, outside at hw + 0.001
    ang = np.linspace(-np.pi / 2, np.pi / 2, 181)
    for r, want in ((5.0 - 0.11, True), (5.001, False)):
        ring = np.stack([100.0 + r * np.cos(ang), 50.0 + r * np.sin(ang)], axis=1)
        if not want:
            ring = ring[1:-1]  # (the two end directions run along the segment's own edge)
        assert inside(line, False, 10.0, ROUND_CAP, MITER, ring) == [want] * len(ring)
    assert inside(line, False, 10.0, ROUND_CAP, MITER, [(103.5, 53.5), (103.6, 53.6)]) == [True, False]  # |.| = 4.95, 5.09


def test_closed_triangle_has_its_closing_edge_and_third_corner():
    tri = [(30, 30), (90, 30), (60, 80)]
    mid_closing, third = (45.3, 55.2), (27.4, 28.5)  # on the edge (60, 80) -> (30, 30); 3 beyond the corner (30, 30), outwards
    assert inside(tri, True, 10.0, BUTT, ROUND_JOIN, [mid_closing, third, (60.2, 46.1)]) == [True, True, False]
    assert inside(tri, True, 10.0, BUTT, MITER, [mid_closing, third]) == [True, True]
    assert inside(tri, True, 10.0, BUTT, BEVEL, [mid_closing, third]) == [True, False]  # the bevel reaches 2.46 from the corner
    assert inside(tri, True, 10.0, SQUARE, BEVEL, [mid_closing, third]) == [True, False]  # a closed sub-path has no caps
    # the same path without Z: no closing edge; two caps instead
    beyond_end = (58.5, 82.5)  # 3 beyond (60, 80) along the last segment
    assert inside(tri, False, 10.0, BUTT, ROUND_JOIN, [mid_closing, third, beyond_end]) == [False, False, False]
    assert inside(tri, False, 10.0, SQUARE, ROUND_JOIN, [mid_closing, third, beyond_end]) == [False, True, True]
    assert inside(tri, False, 10.0, ROUND_CAP, ROUND_JOIN, [mid_closing, third, beyond_end]) == [False, True, True]


@pytest.mark.parametrize("pts,closed", [([(50, 60), (50, 60)], False), ([(50, 60)], False), ([(50, 60)], True), ([(50, 60)] * 3, True)],
                         ids=["M-L", "lone-M", "M-Z", "M-L-L-Z"])
def test_a_dot_is_a_disc_a_square_or_nothing(pts, closed):
    q = [(50.3, 60.2), (54.8, 60.2), (50.3, 55.2), (53.4, 63.4), (55.01, 60.2), (54.8, 64.8), (45.2, 55.2), (55.1, 60.2), (50.3, 65.1)]
    assert inside(pts, closed, 10.0, ROUND_CAP, MITER, q) == [True, True, True, True, False, False, False, False, False]
    assert inside(pts, closed, 10.0, SQUARE, ROUND_JOIN, q) == [True, True, True, True, False, True, True, False, False]
    assert inside(pts, closed, 10.0, BUTT, BEVEL, q) == [False] * 9
    sc = outline_scene(pts, closed, 10.0, BUTT, MITER)
    assert np_hit.flat_items(sc)[0][1] == ((0, 0, 0, 0) if len(pts) == 1 and not closed else (50, 60, 50, 60))  # still a valid item


def grid(x0, y0, x1, y1, step):
    ys, xs = np.mgrid[y0:y1:step, x0:x1:step]
    return np.stack([xs.ravel() + 0.137, ys.ravel() + 0.291], axis=1)


@pytest.mark.parametrize("cap,join", STYLES)
def test_a_repeated_point_opens_no_gap(cap, join):
    a = [(20, 20), (60, 30), (90, 80), (40, 70)]
    for rep in ([a[0], a[0]] + a[1:], a[:2] + [a[1], a[1]] + a[2:], a + [a[3]], [a[0]] + a + [a[3], a[3]]):
        q = grid(0, 0, 110, 100, 1.0)
        for closed in (False, True):
            assert inside(rep, closed, 9.0, cap, join, q) == inside(a, closed, 9.0, cap, join, q)


def pieces_of(entries):
    e = np.asarray(entries, np.uint32)
    sep = np.flatnonzero(e[:, 0] == np_stroke.NAN_BITS)
    start = 0
    for s in sep:
        assert e[s, 1] == start  # the separator carries the index of its piece's first entry
        yield np.ascontiguousarray(e[start:s]).view(np.float32).astype(np.float64)
        start = s + 1
    assert start == len(e)


def random_polyline(rng, hw, closed):
    """2-7 points in [30, 220]^2 whose segments (the closing one too) are at least hw long: round joins are fans on the OUTER side of
    a turn, and the inner side is the neighbouring segments' -- which they cover once they are as long as the stroke is wide by half."""
    while True:
        n = int(rng.integers(3 if closed else 2, 8))
        p = np.round(rng.uniform(30, 220, (n, 2)) * 8) / 8
        d = np.diff(np.concatenate([p, p[:1]]) if closed else p, axis=0)
        if (np.hypot(d[:, 0], d[:, 1]) >= max(hw, 2.0)).all():
            return p


def test_every_piece_is_wound_alike():
    rng = np.random.default_rng(14)
    n_pieces = 0
    for trial in range(40):
        width = float(rng.choice([0.8, 3.0, 10.0, 30.0]))
        closed = bool(trial % 2)
        p = random_polyline(rng, width / 2, closed)
        p = np.concatenate([p[:2], p[1:2], p[2:]])  # (a repeated point)
        for cap, join in STYLES:
            entries, _ = np_stroke.outline(p, closed, width, cap, join)
            for pc in pieces_of(entries):
                x, y = pc[:, 0], pc[:, 1]
                area = 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
                assert area > -1e-9, (trial, cap, join, area)  # (1e-9: what f32 storage can turn a zero-area piece into)
                n_pieces += area > 1e-6
    assert n_pieces > 2000


# ---- 2. containment on random poly-lines -----------------------------------------------------------------------

def seg_distance(a, b, q):
    """[Q, S] distances and whether the nearest point is interior to the segment, float64."""
    ab, aq = b[None] - a[None], q[:, None] - a[None]
    L = (ab * ab).sum(-1)
    t = (aq * ab).sum(-1) / L
    tc = np.clip(t, 0.0, 1.0)
    c = a[None] + ab * tc[..., None]
    return np.hypot(*(q[:, None] - c).transpose(2, 0, 1)), (t > 0) & (t < 1)


def test_containment_of_random_polylines_at_every_style():
    rng = np.random.default_rng(2025)
    n_samples = n_decisive = 0
    for trial in range(36):
        width = float(rng.choice([1.5, 3.0, 6.0, 10.0, 24.0, 60.0]))
        hw = float(np.float32(width) * np.float32(0.5))
        closed = trial % 3 == 2
        p = random_polyline(rng, hw, closed).astype(np.float32)
        q = (rng.uniform(0, 1, (2500, 2)) * (np.ptp(p, axis=0) + 2 * hw + 8) + p.min(axis=0) - hw - 4).astype(np.float32)
        ring = np.concatenate([p, p[:1]]) if closed else p
        dist, interior = seg_distance(ring[:-1].astype(np.float64), ring[1:].astype(np.float64), q.astype(np.float64))
        near_interior = ((dist < hw - 0.11) & interior).any(axis=1)
        dmin = dist.min(axis=1)
        far = dmin > hw + 1e-3
        decisive = (dmin < hw - 0.11) | far
        field = np_hit.item_inside(poly_scene(ring, width), 0, q)  # np_hit's stroke predicate: distance <= hw
        assert np.array_equal(field[decisive], (dmin < hw)[decisive])  # (np_hit and this test agree on what the distance is)
        for cap, join in STYLES:
            got = np_hit.item_inside(outline_scene(p, closed, width, cap, join), 0, q)
            assert got[near_interior].all(), (trial, cap, join)
            if cap == BUTT and join in (BEVEL, ROUND_JOIN):
                assert not got[far].any(), (trial, cap, join)
            if cap == ROUND_CAP and join == ROUND_JOIN:
                assert np.array_equal(got[decisive], field[decisive]), (trial, int((got != field)[decisive].sum()))
        n_samples += len(q)
        n_decisive += int(decisive.sum())
    print(f"{n_decisive} of {n_samples} samples decisive")
    assert n_decisive >= 0.9 * n_samples


def test_the_level_table_keeps_a_half_circle_within_the_flatten_tolerance():
    for L, hw in enumerate(np_stroke.LEVEL_HW):
        assert np_stroke.level(hw) == L and np_stroke.level(np.nextafter(hw, 1e9)) == L + 1
        assert hw * (1.0 - np.cos(np.pi / 2 ** (L + 1))) <= 0.1 < (hw * 1.001) * (1.0 - np.cos(np.pi / 2 ** (L + 1)))
    assert np_stroke.level(1e9) == 6
    # the fan itself: every rim point on the circle, neighbouring ones a step apart
    for L, hw in enumerate(np_stroke.LEVEL_HW):
        width = np.float32(2 * hw * 0.99)  # (just below the threshold, as an f32 width)
        entries, _ = np_stroke.outline([(100, 100), (160, 100)], False, width, ROUND_CAP, BEVEL)
        cap = list(pieces_of(entries))[-1]
        assert len(cap) == 2 ** L + 2
        r = np.hypot(cap[1:, 0] - 160.0, cap[1:, 1] - 100.0)
        assert np.allclose(r, np.float64(width * np.float32(0.5)), atol=2e-5)
        ang = np.arctan2(cap[1:, 1] - 100.0, cap[1:, 0] - 160.0)
        assert np.allclose(np.diff(ang), np.pi / 2 ** L, atol=1e-3)


# ---- 3. the SVG front-end ---------------------------------------------------------------------------------------

def test_svg_stroke_properties_need_the_flag(pm):
    from test_stroke_gpu import SVG_DOC

    ps = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True, stroke_styles=True)
    want = [style_bits(BUTT, MITER, half_bits(10.0)), style_bits(ROUND_CAP, ROUND_JOIN, half_bits(10.0)), style_bits(SQUARE, BEVEL, half_bits(10.0)),
            style_bits(SQUARE, MITER, half_bits(1.2)), style_bits(BUTT, BEVEL, half_bits(4.0)), style_bits(BUTT, ROUND_JOIN, half_bits(10.0))]
    assert [int(f) & style_bits(3, 3, 0xFFFF) for f in ps.paths["flags"]] == want
    assert [int(f) & 0xF for f in ps.paths["flags"]] == [2, 2, 2, 2, 3, 2]
    off = pm.PathSet.from_svg(SVG_DOC, spec_defaults=True)
    assert np.array_equal(off.paths, np_stroke.unstyled(ps.paths)) and np.array_equal(off.els, ps.els)
    # ... and a document without the three properties parses to the same paths as one with them, without the flag
    bare = re.sub(r'\s*stroke-(linecap|linejoin|miterlimit)\s*(=\s*"[^"]*"|:\s*[a-z0-9.]+;?)', "", SVG_DOC)
    assert "linecap" not in bare and "miterlimit" not in bare
    b = pm.PathSet.from_svg(bare, spec_defaults=True)
    assert np.array_equal(b.paths, off.paths) and np.array_equal(b.els, off.els)
    # invalid values are ignored (the inherited value stays); a limit below 1 is an error in SVG
    doc = '<svg><g stroke="red" stroke-linecap="round" stroke-miterlimit="7"><path d="M0 0L9 9" stroke-linecap="flat" stroke-miterlimit="0.5" stroke-linejoin="arcs"/></g></svg>'
    p = pm.PathSet.from_svg(doc, stroke_styles=True).paths
    assert int(p["flags"][0]) == 2 | style_bits(ROUND_CAP, MITER, half_bits(7.0))


def test_the_tiger_with_the_flag_gets_svgs_initial_values(pm):
    lib = pm._lib.load()
    plain = pm.PathSet.tiger()
    text = open(os.path.join(ROOT, "piet_metal_amd", "assets", "Ghostscript_Tiger.svg"), "rb").read()
    assert b"linecap" not in text and b"linejoin" not in text and b"miterlimit" not in text
    styled = pm.PathSet.from_svg(text, stroke_styles=True)
    same = pm.PathSet.from_svg(text)
    assert np.array_equal(same.paths, plain.paths) and np.array_equal(same.els, plain.els) and np.array_equal(styled.els, plain.els)
    stroked = (plain.paths["flags"] & 2) != 0
    want = plain.paths["flags"] | np.where(stroked, style_bits(BUTT, MITER, half_bits(4.0)), 0).astype(np.uint32)
    assert np.array_equal(styled.paths["flags"], want) and stroked.sum() > 50
    helper = plain.with_stroke_style("butt", "miter", 4.0)
    assert np.array_equal(helper.paths, styled.paths)
    some = plain.with_stroke_style("round", "bevel", select=[0, 5, 7])
    assert ((some.paths["flags"] & np_stroke.OUTLINE) != 0).sum() == stroked[[0, 5, 7]].sum()
    with pytest.raises(ValueError):
        plain.with_stroke_style(miter_limit=0.5)
    assert lib.pm_abi_version() == 600


# ---- 4. the kernels under emulation -----------------------------------------------------------------------------

def test_outline_kernels_under_wave64_emulation(built):
    """The `small` cases of tests/test_stroke_gpu.py -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_stroke_gpu.py"), "-q", "-x", "-m", "gpu", "-k", "small", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "14 passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- 5. the kernels' listing ------------------------------------------------------------------------------------

def test_the_outline_kernels_use_no_scratch(tmp_path):
    """KOutlineCount, KOutlineScan and KOutline by the flags the library is built with: no private segment (nothing spilled, no
    indexed local array: a fan's rim is found by descent, not kept)."""
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
        name = re.search(r"KOutline(?:Count|Scan)?(?=E)", m.group(1))  # (the mangled name: <length><name>E<arguments>)
        if not name:
            continue
        found.add(name.group(0))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        print(name.group(0), "vgpr", vgpr, "scratch", scratch)
        assert scratch == 0 and vgpr <= 256, (m.group(1), scratch, vgpr)  # (256: what a workgroup of 256, the launch bound, can be given)
    assert found == {"KOutlineCount", "KOutlineScan", "KOutline"}
