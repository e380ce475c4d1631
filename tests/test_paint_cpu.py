"""Per-group paint (decision D17) without a GPU: the arithmetic of tests/np_paint.py against exact rational rounding and against
answers derived by hand, the helper that states the expected scenes against the oracle, the library's new symbol, the CLI's
--fade opacities, and the new kernels' listing."""
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_groups  # noqa: E402
import np_paint  # noqa: E402
import path_sets  # noqa: E402


# ---- 1. the arithmetic -------------------------------------------------------------------------------------------

def _nearest(num, den):
    """round-to-nearest of num / den for non-negative integer arrays, by cross-multiplication; asserts that no tie exists."""
    q = num // den
    rem2 = 2 * (num - q * den)
    assert not np.any(rem2 == den)
    return q + (rem2 > den)


def test_alpha_is_round_to_nearest_over_all_inputs():
    a, o = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64), indexing="ij")
    got = np_paint.paint_rgba(a, 0, o) & 0xFF
    assert np.array_equal(got, _nearest(a * o, np.uint64(255)))
    for x, y in ((255, 128), (1, 127), (1, 128), (77, 3), (254, 254)):  # the same through Fraction
        want = int(Fraction(x * y, 255) + Fraction(1, 2))  # (no tie: floor(v + 1/2) is the nearest)
        assert int(got[x, y]) == want


@pytest.mark.parametrize("t", [0, 1, 127, 128, 254, 255])
def test_mix_is_round_to_nearest_over_all_channels_and_amounts(t):
    c, k = np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(256, dtype=np.uint64), indexing="ij")
    want = _nearest(c * (255 - k) + np.uint64(t) * k, np.uint64(255))
    for shift in (8, 16, 24):
        got = np_paint.paint_rgba(c << np.uint64(shift), (np.uint64(t) << np.uint64(shift)) | k, 255)
        assert np.array_equal((got >> np.uint32(shift)) & 0xFF, want)
        assert not np.any(got & ~np.uint32(0xFF << shift))  # (the other channels mix 0 with 0; alpha 0 stays 0)
    assert int(want[200, 51]) == int(Fraction(200 * 204 + t * 51, 255) + Fraction(1, 2))


def test_hand_derived_answers():
    rng = np.random.default_rng(17)
    colours = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64), [0, 0xFFFFFFFF, 0xFF, 0xFFFFFF00, 0x01020304]])
    assert np.array_equal(np_paint.paint_rgba(colours, 0, 255), colours.astype(np.uint32))  # {0, 255}: the identity
    assert np_paint.paint_rgba(0x000000FF, 0, 128) == 0x00000080   # 255 * 128 / 255 = 128
    assert np_paint.paint_rgba(0x00000001, 0, 127) == 0            # 127 / 255 < 1/2
    assert np_paint.paint_rgba(0x00000001, 0, 128) == 1            # 128 / 255 > 1/2
    assert np_paint.paint_rgba(0x00000000, 0xFF000080, 255) == 0x80000000  # c 0, t 255, k 128: 32640 / 255 = 128
    assert np_paint.paint_rgba(0x00C80000, 0x00640033, 255) == 0x00B40000  # c 200, t 100, k 51: (40800 + 5100) / 255 = 180
    # every field at once: R 200 -> 180, G 0 -> 20 (t 100: 5100 / 255), B 255 -> 204 + 20 = 224, A 255 * 128 / 255
    assert np_paint.paint_rgba(0xC800FFFF, 0x64646433, 128) == 0xB414E080


# ---- 2. the helper ------------------------------------------------------------------------------------------------

def test_painted_identity_and_colour_words_only(pmo):
    case = path_sets.random_case(405)
    ps, n = case.ps, len(case.ps.paths)
    gmap = np.arange(n, dtype=np.uint32) % 3
    g = int(gmap.max()) + 1
    for same in (np_paint.painted(ps, gmap, None, None), np_paint.painted(ps, gmap, np.zeros(g, np.uint32), np.full(g, 255)),
                 np_paint.painted(ps, None, [0], [255])):
        assert same.paths.tobytes() == ps.paths.tobytes() and same.els.tobytes() == ps.els.tobytes()
    rng = np.random.default_rng(6)
    tints = (rng.integers(0, 1 << 24, g).astype(np.uint32) << np.uint32(8)) | np.uint32(0x80)
    opac = rng.integers(1, 255, g).astype(np.uint32)
    pp = np_paint.painted(ps, gmap, tints, opac)
    other = [k for k in ps.paths.dtype.names if k not in ("fill_rgba", "stroke_rgba")]
    assert all(np.array_equal(pp.paths[k], ps.paths[k]) for k in other) and not np.array_equal(pp.paths["fill_rgba"], ps.paths["fill_rgba"])
    for p in range(n):  # ... and per path it is the scalar rule
        assert pp.paths["fill_rgba"][p] == np_paint.paint_rgba(ps.paths["fill_rgba"][p], tints[gmap[p]], opac[gmap[p]])
        assert pp.paths["stroke_rgba"][p] == np_paint.paint_rgba(ps.paths["stroke_rgba"][p], tints[gmap[p]], opac[gmap[p]])
    # the oracle's scene of the painted set differs from the unpainted one in item colour words only
    aff, ws = [case.affine] * g, [case.scale] * g
    a, n_items, paths_a = np_groups.scene(ps, gmap, aff, ws, pmo.scene_from_paths)
    b, n_items_b, paths_b = np_groups.scene(pp, gmap, aff, ws, pmo.scene_from_paths)
    assert n_items == n_items_b and len(a) == len(b) and np.array_equal(paths_a, paths_b)
    items_ix = 8 + 8 * n_items
    colour = np.zeros(len(a), bool)
    changed = 0
    for i in range(n_items):
        at = items_ix + 32 * i
        tag = int(a[at : at + 4].view(np.uint32)[0]) & 0xFFFF
        assert tag in (3, 4)
        word = at + (8 if tag == 3 else 4)  # PietFill: word 2, PietStrokePolyLine: word 1
        colour[word : word + 4] = True
        changed += int(not np.array_equal(a[word : word + 4], b[word : word + 4]))
    assert np.array_equal(a[~colour], b[~colour]) and changed > n_items // 2


# ---- 3. the library's symbol ------------------------------------------------------------------------------------------

def test_library_exports_and_binds_pm_repaint_groups(pm):
    import ctypes as C

    lib = pm._lib.load()
    assert "pm_repaint_groups" in pm._lib.SIGNATURES
    fn = getattr(lib, "pm_repaint_groups")
    assert fn.argtypes == pm._lib.SIGNATURES["pm_repaint_groups"][1]
    assert C.sizeof(pm._lib.GroupPaint) == 8 == pm.Renderer.GROUP_PAINT_DTYPE.itemsize
    assert [pm.Renderer.GROUP_PAINT_DTYPE.fields[k][1] for k in ("tint_rgba", "opacity")] == [0, 4]
    header = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    assert "int pm_repaint_groups(" in header and "} pm_group_paint;" in header
    assert "#define PM_ABI_VERSION 600u" in header  # (no struct layout changed)
    # without a device the call still answers for its arguments
    assert lib.pm_repaint_groups(None, None, 0) == pm._lib.PM_ERR_INVALID
    table = np.zeros(1, pm.Renderer.GROUP_PAINT_DTYPE)
    assert lib.pm_repaint_groups(None, table.ctypes.data, 1) == pm._lib.PM_ERR_INVALID and "NULL" in pm._lib.last_error()


# ---- 4. the CLI's --fade ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames,n_groups", [(2, 1), (2, 5), (5, 3), (30, 7), (256, 4), (7, 40)])
def test_cli_fade_opacities(pm, n_frames, n_groups):
    from piet_metal_amd import cli

    frames = np.array([cli.fade_opacities(k, n_frames, n_groups) for k in range(n_frames)], np.int64)
    assert frames.shape == (n_frames, n_groups)
    assert np.all(frames[0] == 255) and np.all(frames[-1] == 0)
    assert np.all(np.diff(frames, axis=0) <= 0)  # monotone per group
    assert np.all(np.diff(frames, axis=1) >= 0)  # group g goes before g + 1 ...
    for k in range(n_frames):
        for g in range(n_groups - 1):  # ... which has not begun to fade while g is there
            assert frames[k, g] == 0 or frames[k, g + 1] == 255
        for g in range(n_groups):
            x = min(max(1 - Fraction(k, n_frames - 1) * n_groups + g, 0), 1) * 255
            assert abs(Fraction(int(frames[k, g])) - x) <= Fraction(1, 2)


# ---- 5. the new kernels' listing ----------------------------------------------------------------------------------------

def test_the_paint_kernels_use_no_scratch_and_no_lds(tmp_path):
    """KKeepColours, KPaintPaths and KRepaintItems by the flags the library is built with: no private segment, no LDS."""
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
        name = re.search(r"\d(K(?:KeepColours|PaintPaths|RepaintItems))(?=E)", m.group(1))  # (<length><name>E<arguments>)
        if not name:
            continue
        found.add(name.group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        print(name.group(1), "vgpr", vgpr, "lds", lds, "scratch", scratch)
        assert scratch == 0 and lds == 0 and vgpr <= 256, (m.group(1), scratch, lds, vgpr)
    assert found == {"KKeepColours", "KPaintPaths", "KRepaintItems"}
