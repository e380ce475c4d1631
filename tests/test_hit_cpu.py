"""Point hit testing without a GPU: tests/np_hit.py (the numpy statement of decision D13) against hand-derived answers and
against the oracle's f32 fill coverage, the kernel's logic under wave64 emulation, and the kernel's listing."""
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

NONE = 0xFFFFFFFF
NAN_BITS = 0x7FC00000


# ---- scene bytes by hand (the layout of src/lib.rs:15-77 plus the extensions of pm_layout.h), no encoder involved ----------

def fill(pts, rgba=0x204060FF, even_odd=False):
    return ("fill", [np.asarray(pts, np.float32)], rgba, 1 if even_odd else 0)


def fill_compound(subs, rgba=0x204060FF, even_odd=False):
    return ("fill", [np.asarray(s, np.float32) for s in subs], rgba, 2 | (1 if even_odd else 0))


def polyline(pts, width, rgba=0x204060FF):
    return ("poly", np.asarray(pts, np.float32), rgba, width)


def line(p0, p1, width, rgba=0x204060FF):
    return ("line", p0, p1, rgba, width)


def circle(x0, y0, x1, y1, ellipse=False):
    return ("circle", (x0, y0, x1, y1), ellipse)


def group(*items):
    return ("group", list(items))


def square(x0, y0, s):
    return [(x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s)]


def encode(items, buf=None):
    """A group block {n, items_ix}{boxes}{items} at the end of buf, its point arrays and child groups behind it; returns bytes
    (root call) -- the boxes are zero: np_hit must not look at them for anything but circles."""
    root = buf is None
    buf = bytearray() if root else buf
    at, n = len(buf), len(items)
    buf += bytes(8 + 40 * n)
    struct.pack_into("<II", buf, at, n, at + 8 + 8 * n)
    be = lambda v: struct.unpack("<I", struct.pack(">I", v))[0]  # noqa: E731  (0xRRGGBBAA is stored big-endian)
    for i, it in enumerate(items):
        box, rec = (0, 0, 0, 0), b""
        if it[0] == "group":
            rec = struct.pack("<III", 5, 0, encode(it[1], buf))
        elif it[0] == "circle":
            box, rec = it[1], struct.pack("<I", 1 | ((1 << 16) if it[2] else 0))
        elif it[0] == "line":
            rec = struct.pack("<IIIfffff", 2, 0, be(it[3]), it[4], *it[1], *it[2])
        elif it[0] == "poly":
            pix = len(buf)
            buf += it[1].tobytes()
            rec = struct.pack("<IIfII", 4, be(it[2]), it[3], len(it[1]), pix)
        elif it[0] == "fill":
            pix, npt = len(buf), 0
            for sub in it[1]:
                buf += sub.tobytes()
                if it[3] & 2:
                    buf += struct.pack("<II", NAN_BITS, npt)
                npt += len(sub) + (1 if it[3] & 2 else 0)
            rec = struct.pack("<5I", 3, it[3], be(it[2]), npt, pix)
        struct.pack_into("<4H", buf, at + 8 + 8 * i, *box)
        buf[at + 8 + 8 * n + 32 * i : at + 8 + 8 * n + 32 * i + len(rec)] = rec
    return bytes(buf) if root else at


def ask(scene, pts, skip=False):
    """(top, count) lists -- from both evaluation orders of np_hit, which must agree."""
    a = np_hit.hit_test(scene, np.asarray(pts, np.float32), skip, brute=False)
    b = np_hit.hit_test(scene, np.asarray(pts, np.float32), skip, brute=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return a[0].tolist(), a[1].tolist()


# ---- 1. known answers -------------------------------------------------------------------------------

def test_square():
    sc = encode([fill(square(10, 10, 100))])
    top, cnt = ask(sc, [(50.5, 50.5), (5.5, 50.5), (115.5, 50.5), (50.5, 5.5), (50.5, 115.5), (10.5, 109.5)])
    assert top == [0, NONE, NONE, NONE, NONE, 0] and cnt == [1, 0, 0, 0, 0, 1]


def test_square_with_a_hole_under_both_rules():
    outer, hole = square(0, 0, 100), square(30, 30, 40)
    q = [(50.5, 50.5), (15.5, 50.5), (120.5, 50.5)]
    # hole wound like the outline: winding 2 inside it -- filled by non-zero, a hole by even-odd
    assert ask(encode([fill_compound([outer, hole])]), q)[0] == [0, 0, NONE]
    assert ask(encode([fill_compound([outer, hole], even_odd=True)]), q)[0] == [NONE, 0, NONE]
    # hole wound the other way: winding 0 inside it -- a hole under both rules
    assert ask(encode([fill_compound([outer, hole[::-1]])]), q)[0] == [NONE, 0, NONE]
    assert ask(encode([fill_compound([outer, hole[::-1]], even_odd=True)]), q)[0] == [NONE, 0, NONE]
    # two separate Fill items instead: the "hole" is just another item on top
    assert ask(encode([fill(outer), fill(hole)]), q) == ([1, 0, NONE], [2, 1, 0])


def test_pentagram():
    """Centre (100, 100), radius 80, vertices in star order: the inner pentagon (radius 30.6) has winding 2, the five tips 1.
    The top tip runs from (100, 20) down to y = 75.3, half as wide as 0.325 (y - 20)."""
    star = [(100 + 80 * np.sin(4 * np.pi * k / 5), 100 - 80 * np.cos(4 * np.pi * k / 5)) for k in range(5)]
    q = [(100.1, 100.3), (100.1, 60.3), (100.1, 10.3), (140.3, 50.3), (110.3, 60.3), (115.3, 60.3)]
    assert ask(encode([fill(star)]), q)[0] == [0, 0, NONE, NONE, 0, NONE]
    assert ask(encode([fill(star, even_odd=True)]), q)[0] == [NONE, 0, NONE, NONE, 0, NONE]


def test_strokes_just_inside_and_just_outside_half_the_width():
    sc = encode([polyline([(10, 10), (110, 10), (110, 60)], 8.0), line((20, 200), (20, 300), 3.0), polyline([(300, 300)], 10.0)])
    q = [(60.5, 13.9), (60.5, 14.1), (60.5, 6.1), (60.5, 5.9),      # beside the first segment: hw = 4
         (113.5, 10.25), (114.5, 10.25), (9.5, 6.5), (6.5, 6.5),    # round the corner and the open end
         (106.1, 40.5), (105.9, 40.5),                              # beside the second segment
         (21.4, 250.5), (21.6, 250.5), (20.5, 301.4), (20.5, 301.6),  # the Line: hw = 1.5
         (303.0, 303.9), (303.0, 304.1), (295.5, 300.5)]            # the one-point Polyline: a disc of radius 5
    top, _ = ask(sc, q)
    assert top == [0, NONE, 0, NONE, 0, NONE, 0, NONE, 0, NONE, 1, NONE, 1, NONE, 2, NONE, 2]


def test_circle_and_ellipse():
    sc = encode([circle(200, 20, 260, 80), circle(300, 100, 400, 140, ellipse=True), circle(300, 200, 400, 240), circle(10, 10, 50, 10, ellipse=True)])
    q = [(230.5, 79.4), (251.5, 71.5),    # circle of radius 30 about (230, 50): inside; in the box's corner
         (390.5, 120.5), (390.5, 132.5),  # ellipse 50 x 20 about (350, 120)
         (365.5, 220.5), (375.5, 220.5),  # a circle in a 100 x 40 box has the smaller radius, 20
         (30.5, 10.0)]                    # an ellipse with ry = 0 contains nothing
    assert ask(sc, q)[0] == [0, NONE, 1, NONE, 2, NONE, NONE]


def test_paint_order_nested_groups_and_counts():
    a, b, c, d = square(0, 0, 100), square(50, 50, 100), square(75, 75, 100), square(300, 0, 50)
    sc = encode([fill(a), group(fill(b), group(fill(c)), circle(0, 0, 20, 20)), fill(d)])
    assert len(np_hit.flat_items(sc)) == 5  # flat paint order: a, b, c, circle, d
    q = [(25.5, 25.5), (60.5, 60.5), (80.5, 80.5), (160.5, 160.5), (325.5, 25.5), (10.5, 10.5), (200.5, 25.5)]
    assert ask(sc, q) == ([0, 1, 2, 2, 4, 3, NONE], [1, 2, 3, 1, 1, 2, 0])


def test_transparent_items_and_the_skip_flag():
    sc = encode([fill(square(0, 0, 100)), fill(square(50, 50, 100), rgba=0xFFFFFF00), polyline([(0, 120), (200, 120)], 10.0, rgba=0x11223300),
                 line((0, 140), (200, 140), 10.0, rgba=0x00000000), circle(300, 300, 340, 340)])
    q = [(75.5, 75.5), (125.5, 123.5), (25.5, 25.5), (180.5, 121.5), (180.5, 141.5), (320.5, 320.5)]
    assert ask(sc, q) == ([1, 2, 0, 2, 3, 4], [2, 2, 1, 1, 1, 1])
    assert ask(sc, q, skip=True) == ([0, NONE, 0, NONE, NONE, 4], [1, 0, 1, 0, 0, 1])  # (a Circle is opaque black)


def test_non_finite_and_far_away_queries():
    sc = encode([fill([(-40, -30), (60, -30), (60, 50), (-40, 50)]), fill([(65000, -5), (70500, -5), (70500, 40), (65000, 40)]),
                 polyline([(-20, 20), (-3, -9), (30, -12)], 6.0), line((65500, 100), (70100, 8), 8.0)])
    nan, inf = float("nan"), float("inf")
    q = [(nan, 10.0), (10.0, nan), (inf, 10.0), (10.0, -inf), (-5.0, -5.0), (70000.0, 10.0), (70000.0, 30.0), (-35.5, 40.5), (-45.5, 40.5), (70600.0, 10.0)]
    # (-5, -5): 0.3 from the polyline's second segment; (70 000, 10): on the Line, over the second fill
    assert ask(sc, q) == ([NONE, NONE, NONE, NONE, 2, 3, 1, 0, NONE, NONE], [0, 0, 0, 0, 2, 2, 1, 1, 0, 0])


def test_the_two_evaluation_orders_agree_on_vertices_edges_and_interval_ends():
    """np_hit's sorted evaluation against every-pair evaluation on random scenes, with queries ON vertices, edge midpoints, the
    ends of the strokes' y intervals and integer grid points (where many y values coincide)."""
    rng = np.random.default_rng(2024)
    for trial in range(6):
        items = []
        for _ in range(25):
            k = int(rng.integers(0, 5))
            pts = np.round(rng.uniform(-20, 220, (int(rng.integers(1, 9)), 2)) * 4) / 4
            if k == 0:
                items.append(fill(pts, even_odd=bool(rng.integers(0, 2))))
            elif k == 1:
                items.append(fill_compound([pts, np.round(rng.uniform(0, 200, (3, 2)))], even_odd=bool(rng.integers(0, 2))))
            elif k == 2:
                items.append(polyline(pts, float(rng.choice([0.0, 1.0, 2.5, 7.0]))))
            elif k == 3:
                items.append(line(tuple(pts[0]), tuple(pts[-1]), float(rng.choice([0.0, 3.0, 6.5]))))
            else:
                x0, y0 = (int(v) for v in rng.integers(0, 150, 2))
                items.append(circle(x0, y0, x0 + int(rng.integers(0, 60)), y0 + int(rng.integers(0, 60)), ellipse=bool(rng.integers(0, 2))))
        sc = encode(items)
        verts = np.concatenate([it[1][0] if it[0] == "fill" else it[1] for it in items if it[0] in ("fill", "poly")])
        mids = ((verts[:-1].astype(np.float64) + verts[1:]) * 0.5).astype(np.float32)
        grid = np.stack(np.meshgrid(np.arange(-5.0, 225.0, 7.0), np.arange(-5.0, 225.0, 7.0)), axis=-1).reshape(-1, 2)
        ends = np.concatenate([verts + (0.0, 3.5), verts - (0.0, 3.5), verts + (0.0, 1.25), verts - (0.5, 0.0)])
        q = np.concatenate([verts, mids, grid, ends, rng.uniform(-30, 230, (400, 2))]).astype(np.float32)
        for skip in (False, True):
            top, cnt = ask(sc, q, skip)
        assert max(cnt) >= 3 and NONE in top, trial


# ---- 2. the oracle as a witness -------------------------------------------------------------------------------

def test_np_hit_agrees_with_the_oracles_f32_fill_coverage(pm, pmo):
    """Where the oracle's f32 winding coverage of an item is exactly 1 the pixel centre is inside it, where it is exactly 0 it is
    outside: 40 blobs at 512 x 512, every item, every pixel; at least 80 % of the pixels of every item's box must be decisive.

    The blobs' outlines are the generator's; their colours are made opaque first.  The oracle keeps the reference's TileEncoder
    as it is (PietRender.metal:127-151): a translucent Solid does not clear the encoder's solid colour, so a tile an item covers
    WHOLLY with a translucent colour ends as a lone Bail and pmo.fill_coverage reports 0.0 across the item's interior (item 4 of
    this scene as generated: 7 850 pixels at 1.0 where 57 808 centres are inside).  Coverage is "alpha before colour" -- what
    is witnessed is the outline, which the alpha byte does not touch."""
    wl = pm.workloads.config4_blobs(n_paths=40, size=512)
    wl.paths.paths["fill_rgba"] |= 0xFF
    scene, n_items = pmo.scene_from_paths(pmo.scaled_paths(wl.paths.paths, wl.width_scale), wl.paths.els, wl.affine)
    assert n_items == 40
    ys, xs = np.mgrid[0:512, 0:512]
    centres = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float32)
    items = np_hit.flat_items(scene)
    n_in = n_out = 0
    worst = 1.0
    for i in range(n_items):
        cov = pmo.fill_coverage(scene, i, 512, 512)
        inside = np_hit.item_inside(scene, i, centres).reshape(512, 512)
        ones, zeros = cov == np.float32(1.0), cov == np.float32(0.0)
        assert not (ones & ~inside).any() and not (zeros & inside).any(), i
        x0, y0, x1, y1 = (min(int(v), 512) for v in items[i][1])
        box = (slice(y0, y1), slice(x0, x1))
        assert (y1 - y0) * (x1 - x0) > 0, i
        frac = float((ones | zeros)[box].mean())
        worst = min(worst, frac)
        assert frac >= 0.80, (i, frac)
        n_in += int(ones.sum())
        n_out += int(zeros.sum())
    print(f"decisive pixels: {n_in} inside, {n_out} outside, worst item box {worst:.3f}")
    assert n_in >= 10_000 and n_out >= 10_000


# ---- 3. the kernel under emulation ---------------------------------------------------------------------------------

def test_hit_kernel_under_wave64_emulation(built):
    """The `small` cases of tests/test_hit_gpu.py -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hit_gpu.py"), "-q", "-x", "-m", "gpu", "-k", "small", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "5 passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- 4. the kernel's listing -----------------------------------------------------------------------------------------

def test_the_hit_test_kernel_uses_no_scratch(tmp_path):
    """pm_hit_kernel by the flags the library is built with: no private segment (nothing spilled, no indexed local array) and a
    register count that lets eight waves share a SIMD."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    found = 0
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.M | re.S):
        if "pm_hit_kernel" not in m.group(1):
            continue
        found += 1
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        assert scratch == 0 and vgpr <= 64, (m.group(1), scratch, vgpr)
    assert found == 1
