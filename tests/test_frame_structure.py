"""The frame path where its kernels' lists and counters have edges (tests/frame_structure.py builds the scenes).

Every check is equality with the oracle: pixels through pmo.render, per-tile command lists through assert_ptcl_equal.

Part A, 48 x 48 views with the action in tile (1, 1): lists of exactly kSpChunk, kDenseLdsChunks and kLdsChunks chunks and one
command either side; one long item whose closing command is the last of a chunk, the first of the next, the last in LDS and the
first in HBM; passes of CoarseTile of 64 / 65 / 256 / 257 stream elements and of 63 ... 257 candidates, some of which emit
nothing; binning records that end among the tile's own candidates; 64 fragments and one more; FillStep against FillPairs; 15 ... 33
items ahead in workgroup mode -- each rendered by the single-wave path, by a workgroup and by the dense one-wave kernel.
Part B: the packed word `backdrop << kCtShift | relevant segments` at the limits of DESIGN.md section 9: windings up to +-2047,
a staircase of windings across three strips, 65 535 ... 70 000 segments of one item in one tile, and one turn beyond the limit.

CPU: the builders' constants are the headers'; every scene has the sizes its name says; the oracle agrees with np_tile (and, up to
1 024 turns, np_render) on every scene; tests/test_emu_cpu.py runs the gpu-marked part under the wave64 emulation, thinned.  What
the emulation cannot show -- LDS atomics of many lanes on one packed word, ds_bpermute hand-overs, packed-half adds, the four
waves' exchange -- is what the -m gpu run is for."""
import functools
import os
import re
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_structure as fs  # noqa: E402
from test_edge_scenes import ROWS, _assert_pixels, _render_both_formats, _set_row, _tables, oracle_agrees_with_restatements  # noqa: E402
from test_host_cpu import encode_ops  # noqa: E402

TILE = fs.TILE


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


A = fs.a_scenes(thin=_emulated())


@functools.lru_cache(maxsize=None)
def _a_scene(name):
    import piet_metal_amd as pm

    ops, (w, h) = A[name] if name in A else fs.a_scenes()[name]
    return encode_ops(pm, ops, cap=1 << 20), w, h


_WANT = {}


def _want(pmo, key, scene, w, h):
    """The oracle's pixels, computed once per scene and shared (read only)."""
    if key not in _WANT:
        img = pmo.render(scene, w, h)
        img.setflags(write=False)
        _WANT[key] = img
    return _WANT[key]


def _tile_cmds(pmo, scene, w, h, tx=fs.TX, ty=fs.TY):
    P = pmo.Ptcl(scene, w, h)
    try:
        return P.count(tx, ty), P.cmds(tx, ty)
    finally:
        P.close()


# ---- CPU: the constants ------------------------------------------------------------------------------------------

def _src(name):
    return open(os.path.join(ROOT, "piet_metal_amd", "csrc", name)).read()


def test_structural_constants_are_the_kernels():
    """A retuned kernel must move these tests with it."""
    def consts(text, names):
        return {k: int(v) for k, v in re.findall(r"^constexpr uint32_t (" + "|".join(names) + r") = (\d+);", text, re.M)}

    assert consts(_src("pm_fine_tile.h"), ["kSpChunk", "kMaxFrag", "kAlphaSlots", "kDenseLdsChunks", "kFillPairsMin"]) == {
        "kSpChunk": fs.SP_CHUNK, "kMaxFrag": fs.MAX_FRAG, "kAlphaSlots": fs.ALPHA_SLOTS, "kDenseLdsChunks": fs.DENSE_LDS_CHUNKS,
        "kFillPairsMin": fs.FILL_PAIRS_MIN}
    coarse = _src("pm_coarse_tile.h")
    assert consts(coarse, ["kWaveCands", "kLdsChunks"]) == {"kWaveCands": fs.WAVE_CANDS, "kLdsChunks": fs.LDS_CHUNKS}
    assert "lds_n * 64u" in coarse and "if (q < lds_cmds)" in coarse and "float4 segw[64];" in coarse
    assert consts(_src("pm_device.h"), ["kCtShift"]) == {"kCtShift": fs.CT_SHIFT}
    assert "constexpr uint32_t kCtCountMask = (1u << kCtShift) - 1u;" in _src("pm_device.h")
    assert fs.MAX_WINDING == 2047 and fs.MAX_TILE_SEGS == (1 << 20) - 1
    rows = _src("pm_bin_rows.h")
    assert "constexpr uint32_t kBatch = 64u * kW;               // candidates per record" in rows
    threads = int(re.search(r"^constexpr int kThreads = (\d+);", _src("pm_kernels_common.h"), re.M).group(1))
    assert (threads, 64) == (fs.RECORD_CANDS, fs.RECORD_CANDS_ONE_WAVE)
    ctx = _src("pm_context.hip")
    assert f'EnvInt("PM_HEAVY_STREAM", {fs.HEAVY_STREAM}, 1, 1 << 20)' in ctx
    assert f'EnvInt("PM_HEAVY_STREAM_LONE", std::min<int>({fs.HEAVY_STREAM_LONE}, static_cast<int>(c->heavy_stream)), 1, 1 << 20)' in ctx
    assert f'EnvInt("PM_VHEAVY_STREAM", {fs.VHEAVY_STREAM}, 1, 1 << 20)' in ctx
    assert 'EnvInt("PM_DENSE_FACTOR", 4, 1, 1 << 20)' in ctx and 'EnvInt("PM_DENSE_KERNEL", 1, 0, 1)' in ctx


# ---- CPU: the A scenes are what their names say ---------------------------------------------------------------------

def _kinds(cmds):
    return np.bincount(cmds[:, 0].astype(np.int64), minlength=10)


CLOSERS = (fs.CIRCLE, fs.STROKE, fs.DRAW_FILL)


def _a_scene_claims(pm, pmo, name, ops, w, h):
    """-> the stream elements of tile (1, 1) (relevant segments, 1 for a one-command item)."""
    scene = encode_ops(pm, ops, cap=1 << 20)
    count, cmds = _tile_cmds(pmo, scene, w, h)
    kinds = _kinds(cmds)
    assert kinds[fs.SOLID] == 0 and kinds[fs.BAIL] == (1 if count == 1 else 0) and kinds[fs.FILL_EDGE] == 0, name
    part = name.split("-")
    fam = part[0]
    segs = kinds[fs.LINE] + kinds[fs.FILL]
    if fam == "ladder":
        assert count == int(part[2]), (name, count)
    elif fam == "cut":
        kind, lead, n = part[1], int(part[2][1:]), int(part[3][1:])
        assert count == lead + n + 1 + 2 + 1, (name, count)
        assert cmds[lead + n, 0] == (fs.STROKE if kind == "poly" else fs.DRAW_FILL), name      # the closing command's list position
        assert (cmds[lead : lead + n, 0] == (fs.LINE if kind == "poly" else fs.FILL)).all(), name
        assert cmds[lead + n + 1, 0] == fs.LINE and cmds[lead + n + 2, 0] == fs.STROKE, name
        if kind != "poly":
            assert fs.segments_inside_tile(ops[lead]) == n, name
    elif fam == "pair":
        lead, ns = int(part[2][1:]), [int(v) for v in part[3:]]
        assert count == lead + sum(ns) + len(ns) + 2 + 1, (name, count)
        at = lead
        for n in ns:
            at += n
            assert cmds[at, 0] in (fs.STROKE, fs.DRAW_FILL), (name, at)
            at += 1
        # both copies of the carried state: the items are cut by chunk boundaries of both parities
        first = [lead + sum(ns[:k]) + k for k in range(len(ns))]
        cut = {b for f, n in zip(first, ns) for b in range(fs.SP_CHUNK, f + n + 1, fs.SP_CHUNK) if f < b}
        assert len({(b // fs.SP_CHUNK) % 2 for b in cut}) == 2, (name, cut)
    elif fam == "pass":
        ns = fs.PASSES["-".join(part[2:])]
        want = sum(ns)
        assert segs + kinds[fs.CIRCLE] == want and count == want + len([n for n in ns if n > 1]) + 1, (name, count, segs)
        assert int(part[3]) == want, name
    elif fam == "cands":
        n, silent = int(part[1]), {"all": None, "silent0": 0, "silent1": 1}[part[2]]
        assert sum(kinds[k] for k in CLOSERS) == fs.emitting(n, silent), name
        for op in ops:   # every candidate's box reaches the tile (a circle's: its centre and radius)
            lo, hi = (np.array(op[1:3]) - op[3], np.array(op[1:3]) + op[3]) if op[0] == "circle" else (
                (np.array(op[1:5]).reshape(2, 2).min(axis=0), np.array(op[1:5]).reshape(2, 2).max(axis=0)) if op[0] == "line" else
                (np.min(op[1], axis=0), np.max(op[1], axis=0)))
            assert (lo < 32).all() and (hi > 16).all(), name
        if silent is not None:
            loud = encode_ops(pm, [op for i, op in enumerate(ops) if i % 2 != silent], cap=1 << 20)
            assert np.array_equal(_tile_cmds(pmo, loud, w, h)[1], cmds), name    # the silent ones emit nothing here
    elif fam == "strip":
        assert sum(kinds[k] for k in CLOSERS) == 6 and len(ops) == int(part[1]) + int("-" + part[2]) + 6 + 3, name
        P = pmo.Ptcl(scene, w, h)
        assert P.count(2, 1) > len(ops) - 6 and P.count(0, 1) == 1 and P.count(1, 0) == 1, name
        P.close()
    elif fam == "talls":
        t = int(part[1])
        assert kinds[fs.FILL] == t and kinds[fs.DRAW_FILL] == t and count == 2 * t + 1, name
    elif fam == "tall":
        t = int(part[2])
        assert kinds[fs.FILL] == t and kinds[fs.DRAW_FILL] == 1, name
        first = int(np.flatnonzero(cmds[:, 0] == fs.FILL)[0])
        assert first == (1 if "lead1" in name else 0), name
    elif fam == "mixed":
        t = int(part[3])
        assert kinds[fs.DRAW_FILL] == 2 * t and kinds[fs.FILL] == 4 * t, name
    elif fam == "alpha":
        assert sum(kinds[k] for k in CLOSERS) == int(part[2]), name
    else:
        raise AssertionError(name)
    return int(segs + kinds[fs.CIRCLE])


def test_every_a_scene_has_the_sizes_it_is_named_for(pm, pmo):
    """List length, closing-command position, candidates, stream elements: per pmo.Ptcl.  A builder that misses fails here."""
    scenes = fs.a_scenes()
    names = set(scenes)
    for comp in fs.COMPOSITIONS:
        assert {f"ladder-{comp}-{L}" for L in fs.LADDER} <= names
    for kind in fs.LONG_KINDS:
        assert {f"cut-{kind}-l{lead}-n{n}" for lead in fs.LEADS for n in fs.LONG_N} <= names
    assert set(fs.a_scenes(thin=True)) <= names
    closing = {kind: set() for kind in fs.LONG_KINDS}
    for name, (ops, (w, h)) in scenes.items():
        _a_scene_claims(pm, pmo, name, ops, w, h)
        if name.startswith("cut-") and "corner" not in name:
            closing[name.split("-")[1]].add(int(name.split("-")[2][1:]) + int(name.split("-")[3][1:]))
    thin_closing = {int(n.split("-")[2][1:]) + int(n.split("-")[3][1:]) for n in fs.a_scenes(thin=True) if n.startswith("cut-fill-") and "corner" not in n}
    for edge in (fs.SP_CHUNK, 2 * fs.SP_CHUNK, 3 * fs.SP_CHUNK):
        for kind in fs.LONG_KINDS:
            assert set(range(edge - 2, edge + 3)) <= closing[kind], (kind, edge)
        assert set(range(edge - 2, edge + 3)) <= thin_closing, edge
    # the fill rules differ on the zigzag, so a lost winding shows under one of them
    a, b = (pmo.render(encode_ops(pm, fs.cut_item(k, 0, 64)), 48, 48) for k in ("fill", "fill_eo"))
    assert not np.array_equal(a, b)
    # ... and it covers three quarters of the tile's pixels, most of them partially
    t = a[16:32, 16:32].reshape(-1, 4)
    assert (t != 255).any(axis=1).sum() >= 192 and len(np.unique(t, axis=0)) >= 96


def test_oracle_agrees_with_python_restatements_on_a_scenes(pm, pmo):
    """oracle == np_tile (lists) == np_render (pixels) on every scene of part A: the expected bytes rest on two restatements."""
    tables = _tables()
    for name, (ops, (w, h)) in fs.a_scenes().items():
        oracle_agrees_with_restatements(pmo, encode_ops(pm, ops, cap=1 << 20), w, h, tables, name)


# ---- CPU: the B scenes are what their names say ---------------------------------------------------------------------

def _draw_fills(pmo, scene, w, h):
    """-> ({(tx, ty): backdrop of the tile's DrawFill}, {(tx, ty): Fill commands})"""
    P = pmo.Ptcl(scene, w, h)
    try:
        back, fills = {}, {}
        for ty in range(P.tiles_y):
            for tx in range(P.tiles_x):
                c = P.cmds(tx, ty)
                d = c[c[:, 0] == fs.DRAW_FILL]
                if len(d):
                    back[(tx, ty)] = int(np.int32(d[0, 1]))
                fills[(tx, ty)] = int((c[:, 0] == fs.FILL).sum())
        return back, fills
    finally:
        P.close()


@pytest.mark.parametrize("turns", fs.TURNS + (2048,))
def test_turns_scenes_wind_as_often_as_named(pm, pmo, turns):
    """From the points, in numpy: the winding around the inner tile corners is +-turns, and every side of the quad is `turns`
    segments of each tile it passes through; the oracle's DrawFill backdrops (sign reversed: the reference counts the other way)
    and Fill counts say the same in the tiles that one side crosses."""
    w, h = fs.TURNS_VIEW
    for flip in (False, True):
        ops = fs.turns_ops(turns, flip)
        wind = fs.winding_at_tile_corners(ops[0], w, h)
        assert np.abs(wind).max() == turns and set(np.unique(wind)) == {0, -turns if not flip else turns}
        assert len(ops[0][1]) == 4 * turns
        back, fills = _draw_fills(pmo, encode_ops(pm, ops, cap=4 << 20), w, h)
        for (tx, ty) in ((2, 1),):                # the right-hand side alone crosses it
            assert back[(tx, ty)] == -wind[ty, tx] and fills[(tx, ty)] == turns
        assert fills[(0, 1)] == turns and fills[(0, 0)] == 2 * turns and max(fills.values()) == 2 * turns


@pytest.mark.parametrize("name", list(fs.STAIRS))
def test_staircases_peak_where_named(pm, pmo, name):
    per, less, reverse, aligned, rule = fs.STAIRS[name]
    w, h = fs.STAIR_VIEW
    ops = fs.staircase_ops(per, less, reverse, aligned, rule)
    wind = fs.winding_at_tile_corners(ops[0], w, h)
    row = wind[3]
    peak = fs.stair_peak(name)
    assert abs(peak) <= fs.MAX_WINDING and row[20] == -peak == (row.min() if peak > 0 else row.max())
    first = 2 if aligned else 1                                                       # (the first tile column whose corner is inside level 0)
    steps = np.abs(np.diff(row[first - 1 : first + 16]))
    assert (steps[:15] == per).all() and steps[15] == per - less                      # a level per tile column across the first strip
    assert (row[first + 15 : 32] == -peak).all()                                      # ... carried over the whole second strip
    fall = np.abs(np.diff(row[31:48]))
    assert fall.sum() == abs(peak) - per and set(fall) <= {0, per, per - less}   # ... and down again in the third
    if not aligned:   # the DrawFills of the top row of every level's tiles carry the same numbers
        back, _ = _draw_fills(pmo, encode_ops(pm, ops, cap=4 << 20), w, h)
        assert all(back[(tx, 3)] == -row[tx] for tx in range(48) if (tx, 3) in back) and sum((tx, 3) in back for tx in range(48)) >= 30
        assert max(abs(v) for v in back.values()) == abs(peak)


def test_many_segment_scenes_hold_their_segments_in_one_tile(pm, pmo):
    for n in fs.MANY_SEGS:
        ops = fs.many_segs_ops(n)
        assert fs.segments_inside_tile(ops[1]) == n == len(ops[1][1])
        count, cmds = _tile_cmds(pmo, encode_ops(pm, ops, cap=4 << 20), 48, 48)
        assert count == 1 + n + 1 + 2 + 1 and cmds[1 + n, 0] == fs.DRAW_FILL
    assert fs.MANY_SEGS[0] == (1 << 16) - 1 and fs.MANY_SEGS[1] == 1 << 16 and fs.MANY_SEGS[2] < fs.MAX_TILE_SEGS


def test_oracle_agrees_with_python_restatements_on_b_scenes(pm, pmo):
    """Lists through np_tile for the turns ladder up to 1 024 turns (pixels through np_render too), for 2 047 turns in the tiles of
    the quad's sides.  The staircases and the many-segment scenes are not restated here: np_tile would take minutes on them, and they
    differ from these and from part A's zigzag in their counts alone."""
    import np_render
    import np_tile

    tables = _tables()
    w, h = fs.TURNS_VIEW
    for turns in (41, 255, 256, 1023, 1024):
        for flip, rule in ((False, "fill"), (True, "fill_eo")):
            scene = encode_ops(pm, fs.turns_ops(turns, flip, rule), cap=4 << 20)
            oracle_agrees_with_restatements(pmo, scene, w, h, tables, (turns, flip, rule))
    scene = encode_ops(pm, fs.turns_ops(2047, True), cap=4 << 20)
    got = np_tile.tile_lists(scene.tobytes(), w, h)
    P = pmo.Ptcl(scene, w, h)
    want = P.render()
    for ty in range(P.tiles_y):
        for tx in range(P.tiles_x):
            assert np.array_equal(P.cmds(tx, ty), got[(tx, ty)][0]), (tx, ty)
    for (tx, ty) in ((2, 1), (2, 2), (0, 0), (1, 2)):
        img = np_render.render_tile(got[(tx, ty)][0], tx, ty, tables)
        assert np.array_equal(img, want[TILE * ty : TILE * ty + TILE, TILE * tx : TILE * tx + TILE]), (tx, ty)
    P.close()


# ---- -m gpu: part A -------------------------------------------------------------------------------------------------

HUGE = str(1 << 20)
MODES = {
    # the single-wave path of the general kernel: no list is long enough for a workgroup, and the one-wave kernel is off
    "wave": {"PM_HEAVY_STREAM": HUGE, "PM_HEAVY_STREAM_LONE": HUGE, "PM_VHEAVY_STREAM": HUGE, "PM_DENSE_KERNEL": "0"},
    # a workgroup for every list of more than one stream element
    "workgroup": {"PM_HEAVY_STREAM": "1", "PM_HEAVY_STREAM_LONE": "1", "PM_DENSE_KERNEL": "0"},
    # the dense one-wave kernel from the second frame on: one long list calls the frame dense
    "dense": {"PM_HEAVY_STREAM": "1", "PM_HEAVY_STREAM_LONE": "1", "PM_DENSE_FACTOR": HUGE},
    "unfused": {"PM_FUSED": "0"},
    "one_launch": {"PM_ONE_LAUNCH": "1"},
    "one_bin_wave": {"PM_BIN_WAVES": "1"},
}
_MODE_KEYS = {k for env in MODES.values() for k in env}
ALL_FAMILIES = ("ladder", "cut", "pair", "pass", "cands", "strip", "talls", "tall", "mixed", "alpha")
MODE_FAMILIES = {"wave": ALL_FAMILIES, "workgroup": ALL_FAMILIES, "dense": ALL_FAMILIES,
                 "unfused": ("cut", "pair", "pass", "cands", "strip"), "one_launch": ("cut", "pair", "pass", "cands", "strip"),
                 "one_bin_wave": ("cands", "strip")}

# Lists that are never a workgroup tile, whatever PM_HEAVY_STREAM says: the classes compare a tile's stream elements with
# thresholds of at least 1 (EnvInt's lower bound), and "long" is "more than": a tile of no or one element stays a wave's.
#   scene              stream elements of tile (1, 1)
NEVER_A_WORKGROUP = {
    "ladder-circles-1": 0, "ladder-lines-1": 0, "ladder-fills-1": 0,
    "ladder-circles-2": 1, "ladder-lines-2": 1, "ladder-fills-2": 1,
}

GROUP = 48    # scenes per test: a few seconds at most each


def _a_groups():
    out = []
    for mode, fams in MODE_FAMILIES.items():
        for fam in fams:
            names = [n for n in A if fs.a_family(n) == fam]
            for k in range(0, len(names), GROUP):
                out.append(pytest.param(mode, tuple(names[k : k + GROUP]), id=f"{mode}-{fam}-{k // GROUP}"))
    return out


def _set_mode(monkeypatch, env):
    _set_row(monkeypatch, {})
    for k in _MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,names", _a_groups())
def test_tile_lists_at_their_structural_edges(pm, pmo, monkeypatch, mode, names):
    """Every A scene, two frames each (the host picks the dense kernel from the previous frame's verdict): pixels of both frames
    (the first also as BGRA on the single-wave path) and the tile lists equal the oracle's, and the frame was demonstrably the
    named renderer's."""
    from test_gpu_parity import assert_ptcl_equal

    _set_mode(monkeypatch, MODES[mode])
    r = pm.Renderer(0)
    try:
        for name in names:
            scene, w, h = _a_scene(name)
            want = _want(pmo, name, scene, w, h)
            before = r.dense_kernel_frames()
            if mode == "wave":
                _render_both_formats(r, pmo, scene, w, h, f"{mode}, {name}")
                before_second = before
            else:
                r.resize(w, h)
                r.set_scene_bytes(scene)
                r.render()
                r.sync()
                _assert_pixels(r.read_pixels(), want, f"{mode}, {name}, first frame")
                before_second = r.dense_kernel_frames()
            r.render()
            r.sync()
            _assert_pixels(r.read_pixels(), want, f"{mode}, {name}, second frame")
            heavy = r.stats()["heavy_tiles"]
            if mode == "wave":
                assert heavy == 0 and r.dense_kernel_frames() == before, name
            elif mode == "workgroup":
                assert r.dense_kernel_frames() == before, name
                assert (heavy == 0) if name in NEVER_A_WORKGROUP else (heavy >= 1), (name, heavy)
            elif mode == "dense":
                assert r.dense_kernel_frames() == before_second + 1, name
            assert_ptcl_equal(r, pmo, scene, w, h, maxc=1024)
    finally:
        r.close()


# ---- -m gpu: part B -------------------------------------------------------------------------------------------------

def _turn_cases():
    turns = (1024, 2047) if _emulated() else fs.TURNS
    return [(t, flip, rule) for t in turns for flip in (False, True) for rule in ("fill", "fill_eo")]


@pytest.mark.gpu
@pytest.mark.parametrize("turns,flip,rule", _turn_cases())
def test_turns_ladder(pm, pmo, renderer, turns, flip, rule):
    """The slanted quad walked up to 2 047 times: the packed backdrop at the ends of its range, in the LDS atomics of binning, in
    the prefix sum over a strip's tiles and in CoarseTile's arithmetic shift; the pixels' binary16 signedArea where its ulp is a
    whole unit."""
    from test_gpu_parity import assert_ptcl_equal

    w, h = fs.TURNS_VIEW
    scene = encode_ops(pm, fs.turns_ops(turns, flip, rule), cap=4 << 20)
    _render_both_formats(renderer, pmo, scene, w, h, f"{turns} turns, flip {flip}, {rule}")
    assert_ptcl_equal(renderer, pmo, scene, w, h, maxc=6 * turns + 64)


# (turns, flip): the backdrop of the tile row below the quad's lower left corner is twice the winding there (frame_structure.DOUBLED),
# so the packed field's whole range is -2 * 1024 ... 2 * 1023 + 1: both ends but one, and the lower end itself
DOUBLED_CASES = ((1023, False), (1023, True), (1024, True))


def test_doubled_backdrops_are_twice_the_winding(pm, pmo):
    for turns, flip in DOUBLED_CASES:
        ops = fs.turns_ops(turns, flip, at=fs.DOUBLED)
        back, _ = _draw_fills(pmo, encode_ops(pm, ops, cap=4 << 20), *fs.TURNS_VIEW)
        assert np.abs(fs.winding_at_tile_corners(ops[0], *fs.TURNS_VIEW)).max() == turns
        assert back[(1, 3)] == (-2 if flip else 2) * turns and -fs.MAX_WINDING - 1 <= back[(1, 3)] <= fs.MAX_WINDING


@pytest.mark.gpu
@pytest.mark.parametrize("turns,flip", DOUBLED_CASES)
def test_backdrop_field_to_both_ends(pm, pmo, renderer, turns, flip):
    """Backdrops of 2 046, -2 046 and -2 048 -- the last one the lower end of the field -- from windings of half that."""
    from test_gpu_parity import assert_ptcl_equal

    w, h = fs.TURNS_VIEW
    for rule in ("fill", "fill_eo"):
        scene = encode_ops(pm, fs.turns_ops(turns, flip, rule, at=fs.DOUBLED), cap=4 << 20)
        _render_both_formats(renderer, pmo, scene, w, h, f"doubled backdrop, {turns} turns, flip {flip}, {rule}", bgra=False)
        assert_ptcl_equal(renderer, pmo, scene, w, h, maxc=6 * turns + 64)


def _stair_scene(pm, name):
    per, less, reverse, aligned, rule = fs.STAIRS[name]
    return encode_ops(pm, fs.staircase_ops(per, less, reverse, aligned, rule), cap=4 << 20)


def _stair_names():
    return ["peak-2047-nz"] if _emulated() else list(fs.STAIRS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _stair_names())
def test_staircase(pm, pmo, renderer, name):
    """The winding rises by a level per tile column across one strip, is carried over the next as backdrop alone and falls in the
    third: the prefix sum over the 16 tiles of a strip and the re-packed word, at +-2047 at the peak."""
    from test_gpu_parity import assert_ptcl_equal

    w, h = fs.STAIR_VIEW
    scene = _stair_scene(pm, name)
    want = _want(pmo, ("stair", name), scene, w, h)
    renderer.resize(w, h)
    renderer.set_scene_bytes(scene)
    renderer.render()
    renderer.sync()
    _assert_pixels(renderer.read_pixels(), want, f"staircase {name}")
    assert_ptcl_equal(renderer, pmo, scene, w, h, maxc=3072)


def _many_cases():
    return [(65536, "fill")] if _emulated() else [(n, rule) for n in fs.MANY_SEGS for rule in ("fill", "fill_eo")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,rule", _many_cases())
def test_many_segments_of_one_item_in_one_tile(pm, pmo, renderer, n, rule):
    """65 535, 65 536 and 70 000 relevant segments: nothing on the way is 16 bits wide.  (2^20 - 1, the documented limit, is not
    run: the oracle alone takes more than ten seconds on it; tests/README.md has the measured times.)"""
    from test_gpu_parity import assert_ptcl_equal

    scene = encode_ops(pm, fs.many_segs_ops(n, rule), cap=4 << 20)
    want = _want(pmo, ("many", n, rule), scene, 48, 48)
    renderer.resize(48, 48)
    renderer.set_scene_bytes(scene)
    t0 = time.perf_counter()
    renderer.render()
    renderer.sync()
    print(f"many segments: n = {n}, {rule}: first frame {time.perf_counter() - t0:.3f} s")
    _assert_pixels(renderer.read_pixels(), want, f"{n} segments, {rule}")
    assert_ptcl_equal(renderer, pmo, scene, 48, 48, maxc=n + 16)


@pytest.mark.gpu
def test_one_turn_beyond_the_limit_is_silent_and_stays_local(pm, pmo):
    """2 048 turns: no error; every tile the item's box does not touch is the oracle's; the next scene on the same Renderer -- 2 047
    turns -- is the oracle's, pixels and lists.  (What the overflowing tiles show is not asserted: DESIGN.md section 9.)"""
    from test_gpu_parity import assert_ptcl_equal

    w, h = fs.BEYOND_VIEW
    r = pm.Renderer(0)
    try:
        for turns in (2048, 2047):
            ops = fs.beyond_ops(turns)
            scene = encode_ops(pm, ops, cap=4 << 20)
            want = pmo.render(scene, w, h)
            r.resize(w, h)
            r.set_scene_bytes(scene)
            r.render()
            r.sync()
            got = r.read_pixels()
            if turns == 2047:
                _assert_pixels(got, want, "2047 turns after 2048")
                assert_ptcl_equal(r, pmo, scene, w, h, maxc=6 * turns + 64)
                continue
            q = fs.quad()
            lo, hi = np.floor(q.min(axis=0) / TILE).astype(int), np.floor(q.max(axis=0) / TILE).astype(int)
            outside = np.ones((h, w), bool)
            outside[lo[1] * TILE : (hi[1] + 1) * TILE, lo[0] * TILE : (hi[0] + 1) * TILE] = False
            assert outside.sum() >= 20 * TILE * TILE and (want[outside] != 255).any()
            keep = np.where(outside[..., None], got, want)
            _assert_pixels(keep, want, "2048 turns, tiles outside the item's box")
    finally:
        r.close()


def _row_scenes(pm):
    w, h = fs.TURNS_VIEW
    cases = ((2046, False, "fill_eo"), (2046, True, "fill"), (2047, False, "fill"), (2047, True, "fill_eo"))
    out = [(f"turns {t} {rule}", encode_ops(pm, fs.turns_ops(t, flip, rule), cap=4 << 20), w, h, 6 * t + 64)
           for t, flip, rule in (cases[2:] if _emulated() else cases)]
    # (emulated: test_staircase has run one already, on the default row)
    for name in (() if _emulated() else ("per127-nz", "peak2047-nz-aligned", "peak-2047-nz", "peak-2047-eo-aligned")):
        out.append((f"staircase {name}", _stair_scene(pm, name), *fs.STAIR_VIEW, 3072))
    return out


def _rows():
    return [r for r in ROWS if r[0] in ("defaults", "one_launch")] if _emulated() else ROWS


@pytest.mark.gpu
@pytest.mark.parametrize("row,env", _rows(), ids=[r[0] for r in _rows()])
def test_counter_limits_over_switch_rows(pm, pmo, monkeypatch, row, env):
    """The turns ladder at 2 046 and 2 047 turns and the staircases on one Renderer of every row of test_edge_scenes.ROWS: a lone
    frame, three frames in flight, then a band; lists after the lone frame."""
    from test_gpu_parity import assert_ptcl_equal

    _set_row(monkeypatch, env)
    for k in _MODE_KEYS:
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    r = pm.Renderer(0)
    try:
        for what, scene, w, h, maxc in _row_scenes(pm):
            want = _want(pmo, ("row", what), scene, w, h)
            r.resize(w, h)
            r.set_scene_bytes(scene)
            r.render()
            r.sync()
            _assert_pixels(r.read_pixels(), want, f"{row}, {what}, lone frame")
            assert_ptcl_equal(r, pmo, scene, w, h, maxc=maxc)
            for _ in range(3):
                r.render()
            _assert_pixels(r.read_pixels(), want, f"{row}, {what}, three frames in flight")
            rows = (h + TILE - 1) // TILE
            a, b = 1, rows - 1
            r.set_band(a, b)
            r.render()
            _assert_pixels(r.read_pixels(), want[a * TILE : min(b * TILE, h)], f"{row}, {what}, band {a}-{b}")
            r.set_band(0, rows)
    finally:
        r.close()
