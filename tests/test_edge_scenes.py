"""Degenerate and grid-aligned scenes, and sweeps of the per-pixel arithmetic (tests/edge_scenes.py), against the oracle.

CPU: the oracle agrees with the two Python restatements (np_tile, np_render) on the grammar's small scenes and on the sweeps at
reduced size -- so the expected bytes of everything below are pinned twice --, and the committed seeds are not a thin sample
(every class drawn, every command kind in the lists, few blank scenes).
-m gpu (tests/test_emu_cpu.py runs these under the CPU emulation of the kernels, which judges their logic; the device's own
arithmetic -- instruction selection, f16 / f32 denormals, packed-half operations, the division and sqrt expansions -- is judged on
the MI355X alone): frames over rows of frame-path switches, hit testing, styled strokes, the sweeps, and oracle parity at the
coordinate bound of DESIGN.md section 9."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_scenes as es  # noqa: E402
from test_host_cpu import encode_ops  # noqa: E402

TILE = 16
WHITE = 0xFFFFFFFF

# parity holds for coordinates of magnitude up to COORD_BOUND (the f32 scene values); see
# test_parity_at_the_coordinate_bound
COORD_BOUND = 3.0e38


def _tables():
    import np_render

    return (np_render.lut_srgb_to_linear_half(), np_render.lut_unorm_to_half(), np_render.lut_linear_half_to_srgb8())


def oracle_agrees_with_restatements(pmo, scene, w, h, tables, name, pixels=True):
    """Lists word for word, solid colours, and np_render's pixels of np_tile's lists byte for byte.  -> (tags seen, blank?)"""
    import np_render
    import np_tile

    with np.errstate(all="ignore"):  # (far coordinates overflow to infinities and NaNs in both restatements alike)
        got = np_tile.tile_lists(scene.tobytes(), w, h)
    P = pmo.Ptcl(scene, w, h)
    try:
        want = P.render()
        tags = set()
        for ty in range(P.tiles_y):
            for tx in range(P.tiles_x):
                oc = P.cmds(tx, ty)
                g, solid = got[(tx, ty)]
                assert solid == P.solid(tx, ty), (name, tx, ty)
                assert np.array_equal(oc, g), (name, tx, ty)
                tags.update(int(t) for t in oc[:, 0])
                ref = want[TILE * ty : TILE * ty + TILE, TILE * tx : TILE * tx + TILE]
                if g[0, 0] == np_tile.BAIL:
                    img = np.empty((TILE, TILE, 4), np.uint8)
                    img[:] = np.frombuffer(struct.pack("<I", solid), np.uint8)
                elif pixels:
                    img = np_render.render_tile(g, tx, ty, tables)
                else:
                    continue
                assert np.array_equal(img[: ref.shape[0], : ref.shape[1]], ref), (name, tx, ty)
    finally:
        P.close()
    return tags, bool((want == 255).all())


def oracle_tags_and_blank(pmo, scene, w, h):
    P = pmo.Ptcl(scene, w, h)
    try:
        tags = set()
        for ty in range(P.tiles_y):
            for tx in range(P.tiles_x):
                tags.update(int(t) for t in P.cmds(tx, ty)[:, 0])
        return tags, bool((P.render() == 255).all())
    finally:
        P.close()


def assert_sample_is_not_thin(what, classes, tags, blank, n):
    missing = es.REQUIRED_CLASSES - classes
    assert not missing, f"{what}: classes never drawn: {sorted(missing)}"
    assert tags >= set(range(1, 10)), f"{what}: command kinds never seen: {sorted(set(range(1, 10)) - tags)}"
    assert 10 * blank <= n, f"{what}: {blank} of {n} scenes render entirely white"


# ---- CPU ------------------------------------------------------------------------------------------------------

def test_oracle_agrees_with_python_restatements_on_grammar_scenes(pm, pmo):
    """160 grammar scenes at viewports up to 100 x 48: oracle == np_tile (lists, solid colours) == np_render (pixels); and the
    sample's three conditions."""
    tables = _tables()
    classes, tags, blank = set(), set(), 0
    assert len(es.SMALL_SEEDS) >= 150
    for seed in es.SMALL_SEEDS:
        scene, w, h, used = es.edge_scene(pm, seed, small=True)
        assert w <= 100 and h <= 48
        t, b = oracle_agrees_with_restatements(pmo, scene, w, h, tables, seed)
        classes |= used
        tags |= t
        blank += b
    assert_sample_is_not_thin("small scenes", classes, tags, blank, len(es.SMALL_SEEDS))


def test_committed_frame_and_hit_seeds_are_not_a_thin_sample(pm, pmo):
    """The seeds of the -m gpu tests, judged with the oracle alone."""
    for what, seeds in (("frame seeds", es.FRAME_SEEDS), ("hit seeds", es.HIT_SEEDS)):
        classes, tags, blank = set(), set(), 0
        for seed in seeds:
            scene, w, h, used = es.edge_scene(pm, seed)
            t, b = oracle_tags_and_blank(pmo, scene, w, h)
            classes |= used
            tags |= t
            blank += b
        assert_sample_is_not_thin(what, classes, tags, blank, len(seeds))


def test_class_knobs_switch_classes_off():
    ops, used = es.edge_ops(5, 100, 48, n=200, classes=es.ALL_CLASSES - {"far", "snap_tile", "alpha_0", "kind_circle", "width_0"})
    assert not used & {"far", "snap_tile", "alpha_0", "kind_circle", "width_0"}
    assert all(op[0] != "circle" for op in ops)
    again, _ = es.edge_ops(5, 100, 48, n=200, classes=es.ALL_CLASSES - {"far", "snap_tile", "alpha_0", "kind_circle", "width_0"})
    assert repr(ops) == repr(again)


def test_oracle_agrees_with_np_render_on_the_sweeps_at_reduced_size(pm, pmo):
    """The sweeps' scenes through both restatements: every 16th pair of the blend sweep with each second item, the operand tables
    whole (the 65 535-wide one: its last tile columns, through a window of np_tile's lists would take minutes -- the oracle's lists
    of its far end are rendered by np_render instead)."""
    import np_render

    tables = _tables()
    pairs = es.blend_pairs()[::16]
    for second in ("edge", "wedges", "stroke", "circle"):
        ops, w, h = es.blend_sweep(second, pairs, columns=16)
        scene = encode_ops(pm, ops, cap=4 << 20)
        tags, blank = oracle_agrees_with_restatements(pmo, scene, w, h, tables, second)
        assert 8 in tags and not blank, second  # (the Solid under the second item)
    tables_ = {**es.fill_operand_scenes(), **es.stroke_operand_scenes(), "coverage_sweep": es.coverage_sweep(64, 8)}
    for name, (ops, w, h) in tables_.items():
        scene = encode_ops(pm, ops, cap=4 << 20)
        oracle_agrees_with_restatements(pmo, scene, w, h, tables, name)
    ops, w, h = es.far_corner_scene()
    scene = encode_ops(pm, ops)
    P = pmo.Ptcl(scene, w, h)
    try:
        want = P.render()
        drawn = 0
        for tx in range(P.tiles_x - 12, P.tiles_x):
            img = np_render.render_tile(P.cmds(tx, 0), tx, 0, tables)
            ref = want[:, TILE * tx : TILE * tx + TILE]
            assert img is not None and np.array_equal(img[:, : ref.shape[1]], ref), tx
            drawn += int((ref != 255).any())
        assert drawn >= 8
    finally:
        P.close()


# ---- -m gpu: frames ---------------------------------------------------------------------------------------------

COMMON = {"PM_BIN_SPLIT_SLOTS": "48"}
ROWS = [
    ("defaults", {}),
    ("row_lists", {"PM_ROW_LIST_MIN_ITEMS": "1"}),
    ("split2_static_handout", {"PM_BIN_SPLIT": "2", "PM_HANDOUT": "1"}),
    ("unfused_fine_split", {"PM_FUSED": "0", "PM_FINE_SPLIT": "1"}),
    ("dense_factor_64", {"PM_DENSE_FACTOR": "64"}),
    ("one_launch", {"PM_ONE_LAUNCH": "1"}),
    ("split0_handout2_one_wave_unfolded", {"PM_BIN_SPLIT": "0", "PM_HANDOUT": "2", "PM_BIN_WAVES": "1", "PM_FOLD_CLEAR": "0", "PM_BIN_WG_PER_CU": "1"}),
]
_ENV_KEYS = {k for _, env in ROWS for k in env} | set(COMMON) | {"PM_FRAME_STREAMS", "PM_SLOTS", "PM_FINE_HEAVY", "PM_PTCL_INITIAL_CMDS"}


def _set_row(monkeypatch, env):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**COMMON, **env}.items():
        monkeypatch.setenv(k, v)


def _assert_pixels(got, want, what):
    if not np.array_equal(got, want):
        bad = (got != want).any(axis=2)
        ys, xs = np.nonzero(bad)
        tiles = sorted({(int(x) // TILE, int(y) // TILE) for y, x in zip(ys, xs)})
        first = [(int(x), int(y), got[y, x].tolist(), want[y, x].tolist()) for y, x in list(zip(ys, xs))[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} pixels in {len(tiles)} tiles differ from the oracle's; tiles {tiles[:8]}, "
                             f"(x, y, got, want) {first}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", ROWS, ids=[r[0] for r in ROWS])
def test_grammar_scenes_over_frame_sequences(pm, pmo, monkeypatch, name, env):
    """Every frame seed on one Renderer of the row: a lone frame, then up to four more in flight; pixels after every step, the
    lists on a third of the scenes, and on scenes at least 48 rows high a random band rendered twice against the frame's rows."""
    from test_gpu_parity import assert_ptcl_equal

    _set_row(monkeypatch, env)
    r = pm.Renderer(0)
    try:
        for k, seed in enumerate(es.FRAME_SEEDS):
            rng = np.random.default_rng([seed, 4])
            scene, w, h, _ = es.edge_scene(pm, seed)
            want = pmo.render(scene, w, h)
            r.resize(w, h)
            r.set_scene_bytes(scene)
            r.render()
            r.sync()
            _assert_pixels(r.read_pixels(), want, f"{name}, seed {seed} at {w}x{h}, lone frame")
            n = int(rng.integers(0, 5))
            for _ in range(n):
                r.render()
            if n:
                _assert_pixels(r.read_pixels(), want, f"{name}, seed {seed} at {w}x{h}, {n} frames in flight")
            if k % 3 == 0:
                assert_ptcl_equal(r, pmo, scene, w, h, maxc=4096)
            if h >= 48:
                rows = (h + TILE - 1) // TILE
                a = int(rng.integers(0, rows - 1))
                b = int(rng.integers(a + 1, rows + 1))
                r.set_band(a, b)
                for rep in range(2):
                    r.render()
                    _assert_pixels(r.read_pixels(), want[a * TILE : min(b * TILE, h)], f"{name}, seed {seed} at {w}x{h}, band {a}-{b} #{rep}")
                r.set_band(0, rows)
    finally:
        r.close()


# ---- -m gpu: hit testing -----------------------------------------------------------------------------------------

def hit_queries(scene, w, h, seed):
    """Uniform points, integer and half-integer points, every finite vertex verbatim and moved by (0.5, 0), (0, 0.5), (0, -1),
    and every segment's midpoint."""
    from test_hit_gpu import scene_vertices_and_segments

    rng = np.random.default_rng([seed, 5])
    verts, a, b = scene_vertices_and_segments(scene)
    verts = verts[np.isfinite(verts).all(axis=1)].astype(np.float64)
    uni = rng.uniform(0.0, 1.0, (1500, 2)) * (w + 16.0, h + 16.0) - 8.0
    ints = np.floor(rng.uniform(0.0, 1.0, (600, 2)) * (w + 4.0, h + 4.0) - 2.0)
    halves = np.floor(rng.uniform(0.0, 1.0, (600, 2)) * (w + 4.0, h + 4.0) - 2.0) + 0.5
    mixed = np.stack([ints[:300, 0], halves[:300, 1]], axis=1)
    with np.errstate(all="ignore"):
        mids = (a + b) * 0.5
    mids = mids[np.isfinite(mids).all(axis=1)]
    return np.concatenate([uni, ints, halves, mixed, verts, verts + (0.5, 0.0), verts + (0.0, 0.5), verts + (0.0, -1.0), mids]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", es.HIT_SEEDS)
def test_grammar_scenes_hit_testing(pm, pmo, seed):
    from test_hit_gpu import check_against_np_hit

    scene, w, h, _ = es.edge_scene(pm, seed)
    q = hit_queries(scene, w, h, seed)
    with pm.Renderer(0) as r:
        r.set_scene_bytes(scene)
        want_top, want_cnt = check_against_np_hit(r, scene, q, brute_sample=400)
        check_against_np_hit(r, scene, q, skip_transparent=True)
    assert want_cnt.max() >= 2 and (want_top != 0xFFFFFFFF).sum() >= 100


# ---- -m gpu: styled strokes ---------------------------------------------------------------------------------------

def _stroke_combos():
    from test_stroke_gpu import COMBOS

    return COMBOS


@pytest.mark.gpu
@pytest.mark.parametrize("cap,join", _stroke_combos(), ids=[f"{c}-{j}" for c, j in _stroke_combos()])
def test_grammar_polylines_as_styled_strokes(pm, pmo, cap, join):
    """Snapped, collinear, reversing poly-lines with repeated points, open and closed, at widths 0, 0.7 and D14's level thresholds
    (each with its f32 neighbours): the scene is np_stroke's, the pixels the oracle's, the hits np_hit's."""
    from np_stroke import half_bits, style_bits
    from test_stroke_gpu import CAPS, IDENTITY, JOINS, render_and_hit_checks, styled_scene_checks

    limits = [0, half_bits(1.0), half_bits(4.0), half_bits(10.0)]
    combo = _stroke_combos().index((cap, join))
    ps = es.stroke_pathset(40 + combo, lambda k: 2 | style_bits(CAPS[cap], JOINS[join], limits[k % 4]))
    with pm.Renderer(0) as r:
        scene = styled_scene_checks(pm, r, ps, IDENTITY, 1.0)
        render_and_hit_checks(pmo, r, scene, 176, 144, 400, seed=60 + combo)


# ---- -m gpu: sweeps of the pixel arithmetic ------------------------------------------------------------------------

def _render_both_formats(r, pmo, scene, w, h, what, bgra=True):
    want = pmo.render(scene, w, h)
    r.resize(w, h)
    r.set_scene_bytes(scene)
    r.render()
    r.sync()
    _assert_pixels(r.read_pixels(), want, what)
    if bgra:
        try:
            r.set_target_format(bgra=True)
            r.render()
            _assert_pixels(r.read_pixels(bgra=True), want[:, :, [2, 1, 0, 3]], what + ", BGRA")
        finally:
            r.set_target_format(bgra=False)
    return want


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


@pytest.mark.gpu
@pytest.mark.parametrize("second", ["edge", "wedges", "stroke", "circle"])
def test_blend_sweep(pm, pmo, renderer, second):
    """4 096 (channel value, alpha) pairs, one tile each at 1024 x 1024, in RGBA and BGRA (under the emulation every fourth pair:
    it cannot judge the arithmetic, only that the scene is handled)."""
    pairs = es.blend_pairs()
    ops, w, h = es.blend_sweep(second, pairs[::4] if _emulated() else pairs, columns=32 if _emulated() else 64)
    assert _emulated() or (w, h) == (1024, 1024)
    scene = encode_ops(pm, ops, cap=16 << 20)
    want = _render_both_formats(renderer, pmo, scene, w, h, f"blend sweep, {second}")
    # the sweep does sweep: nearly every tile has its own bytes, and partial coverages abound
    tiles = want.reshape(h // TILE, TILE, w // TILE, TILE, 4).swapaxes(1, 2).reshape(-1, TILE * TILE * 4)
    assert len({t.tobytes() for t in tiles}) >= 0.9 * len(tiles)
    if second == "wedges":
        # (8-bit output: at most 86 different colours in a tile of the full sweep, fewer at small alphas)
        assert max(len(np.unique(t.reshape(-1, 4), axis=0)) for t in tiles[:: max(1, len(tiles) // 256)]) >= 64


@pytest.mark.gpu
def test_coverage_sweep(pm, pmo, renderer):
    """4 096 tiles of opaque slivers over white at 1024 x 1024, every pixel partially covered, no operand a dyadic fraction: the
    sweep that shows a binary16 conversion which rounds once instead of twice (ToHalf in pm_fine_tile.h).  Modelled in numpy
    (np_render with the products of its Fill in binary64): 3 pixels of the first 1 024 tiles change, none of the 4.2 M pixels of
    the four blend sweeps, whose operands are grid-aligned and whose products are therefore exact.  Measured on the MI355X with a
    build whose ToHalf has no PinF32 (16 v_fma_mixlo_f16 in the tile kernel): 15 pixels in 15 tiles of this sweep are off by one,
    every other test of this file passes."""
    ops, w, h = es.coverage_sweep(256, 16) if _emulated() else es.coverage_sweep()
    assert _emulated() or (w, h) == (1024, 1024)
    scene = encode_ops(pm, ops, cap=16 << 20)
    want = _render_both_formats(renderer, pmo, scene, w, h, "coverage sweep")
    partial = ((want[..., :3] != 255).any(axis=2) & (want[..., :3] != 0).any(axis=2)).mean()
    assert partial >= 0.8, partial


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(es.fill_operand_scenes()) + sorted(es.stroke_operand_scenes()))
def test_operand_tables(pm, pmo, renderer, name):
    from test_gpu_parity import assert_ptcl_equal

    ops, w, h = {**es.fill_operand_scenes(), **es.stroke_operand_scenes()}[name]
    scene = encode_ops(pm, ops, cap=4 << 20)
    _render_both_formats(renderer, pmo, scene, w, h, name)
    assert_ptcl_equal(renderer, pmo, scene, w, h, maxc=4096)


@pytest.mark.gpu
def test_far_corner_of_the_widest_viewport(pm, pmo, renderer):
    """65 535 x 16: x near 65 535, where an f32 ulp is 1/256 px (under the emulation the last 2 048 columns' worth of tiles only
    as far as the lists go: the frame is rendered whole either way)."""
    ops, w, h = es.far_corner_scene()
    scene = encode_ops(pm, ops)
    want = _render_both_formats(renderer, pmo, scene, w, h, "far corner", bgra=not _emulated())
    assert (want[:, -64:] != 255).any()


# ---- -m gpu: the coordinate bound ----------------------------------------------------------------------------------

def bound_scene(pm, seed, magnitude):
    w, h = es.viewport(seed)
    m = float(magnitude)
    ops, _ = es.edge_ops(seed, w, h, far_values=(-m, m, -0.5 * m, 0.75 * m))
    return encode_ops(pm, ops, cap=4 << 20), w, h


BOUND_SEEDS = (1003, 1007, 1012, 1018)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", BOUND_SEEDS)
def test_parity_at_the_coordinate_bound(pm, pmo, renderer, seed):
    """Grammar scenes whose far coordinates are +-COORD_BOUND (and a half and three quarters of it): pixels and lists are the
    oracle's.  Measured on the oracle built with -fsanitize=float-cast-overflow,undefined over far coordinates of 1e6, 2^24, 1e9,
    2^31, 1e30 and 3e38: no undefined cast at any of them (every float -> integer conversion of the oracle takes a value that was
    clamped or compared first: the u16 boxes, the backdrop, the signs), and the oracle and np_tile agree at every one of them."""
    from test_gpu_parity import assert_ptcl_equal

    scene, w, h = bound_scene(pm, seed, COORD_BOUND)
    want = pmo.render(scene, w, h)
    renderer.resize(w, h)
    renderer.set_scene_bytes(scene)
    renderer.render()
    renderer.sync()
    _assert_pixels(renderer.read_pixels(), want, f"seed {seed} at {w}x{h}, far coordinates {COORD_BOUND:g}")
    assert_ptcl_equal(renderer, pmo, scene, w, h, maxc=4096)


def test_oracle_agrees_with_np_tile_at_the_coordinate_bound(pm, pmo):
    tables = _tables()
    for seed in es.SMALL_SEEDS[:24]:
        w, h = es.viewport(seed, small=True)
        for m in (2.0 ** 31, COORD_BOUND):
            ops, _ = es.edge_ops(seed, w, h, far_values=(-m, m, -0.5 * m, 0.75 * m))
            oracle_agrees_with_restatements(pmo, encode_ops(pm, ops, cap=4 << 20), w, h, tables, (seed, m))
