"""The class queues' sharded cursors and sub-queues (-m gpu; the last test runs the small cases under the CPU emulation).

Binning's work-list entry r queues its tiles in sub-queue r % kClassShards of their cost class (csrc/pm_device.h), and the tile
kernels find a slot's queue entry from the prefix sums of the kClasses x kClassShards cursors (csrc/pm_kernels_common.h,
ClassQueueEntry).  The shapes here are the smallest at which that can go wrong: work lists around the shard count, a last strip of
one tile, shards and classes that stay empty, sub-queues filled to their last entry, chained and cut strip rows, frames in
flight, and every other reader of the cursors (the stand-alone list kernel, the one-wave tile kernel, a band, the overflow
repair, pm_get_stats).  Every case is byte-exact against the oracle; "lists" cases also compare every tile's command list and
pm_get_stats' queued_tiles with the oracle's count of per-pixel tiles."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_host_cpu import encode_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every switch a case sets (pm_create reads them): cleared first, so that a case runs with its own switches only
_SWITCHES = ("PM_BIN_SPLIT", "PM_BIN_WG_PER_CU", "PM_FUSED", "PM_DENSE_FACTOR", "PM_PTCL_INITIAL_CMDS", "PM_HANDOUT", "PM_BIN_WAVES")

# list lengths (stream elements of a tile) on both sides of every class threshold, a lone frame's (112, 76, 40, 30, 20, 12, 6)
# and a frame's behind others (112, 92, 72, 54, 36, 22, 11): pm_context.hip, SetClassThresholds
FAN_SIZES = (3, 6, 7, 11, 12, 13, 20, 21, 23, 30, 31, 37, 40, 41, 55, 73, 77, 93, 112, 114)


def crossing_ops(w, h):
    """A few translucent fills and strokes that cross every tile row of a w x h viewport, and one stroke that crosses every
    strip.  Every tile inside an item's box is reached by the item's outline -- upright 14-pixel rectangles across a tile
    boundary, upright and level strokes -- because pm_get_stats' queued_tiles counts what BINNING queues: a tile inside a box
    that no segment of the item reaches is queued and gets an empty list (the reference draws nothing there), and the count
    would exceed the oracle's count of per-pixel tiles by those."""
    xa, xb = 16.0 * int(w * 0.1 / 16) + 9.0, 16.0 * int(w * 0.55 / 16) + 9.0
    return [
        ("fill", np.array([[xa, -4.0], [xa + 14.0, -4.0], [xa + 14.0, h + 4.0], [xa, h + 4.0]]), 0x3060C0A0),
        ("fill", np.array([[xb, -3.0], [xb, h + 3.0], [xb + 14.0, h + 3.0], [xb + 14.0, -3.0]]), 0xC0402080),
        ("poly", np.array([[w - 1.5, 0.5], [w - 6.0, h * 0.5], [w - 1.5, h - 0.5]]), 0x905010B0, 1.5),
        ("poly", np.array([[w * 0.3, -2.0], [w * 0.3, h * 0.4], [w * 0.3, h + 2.0]]), 0x208040C0, 3.0),
        ("line", w * 0.7, -5.0, w * 0.7, h + 5.0, 5.0, 0xE0E02070),
        ("line", 0.0, h * 0.5 + 0.3, float(w), h * 0.5 + 0.3, 2.5, 0x10101090),
    ]


def diagonal_ops(w, h):
    """Thin translucent diagonal strokes, 16 pixels apart: every tile is crossed by two of them and by nothing else, so that
    every tile is queued, and all of them in the class of the shortest lists."""
    ops = []
    for j in range(-(h // 16) - 1, w // 16 + 1):
        c = 16.0 * j + 5.0
        ops.append(("line", c, 0.0, c + h, float(h), 0.7, 0x204060A0 + ((j & 7) << 12)))
    return ops


def fan_ops(sizes=FAN_SIZES, tile_x=3):
    """Tile row i gets sizes[i] short translucent strokes through the centre of ONE tile: list lengths across every class."""
    ops = []
    for i, n in enumerate(sizes):
        cx, cy = 16.0 * tile_x + 8.0, 16.0 * i + 8.0
        for k in range(n):
            a = np.pi * k / n
            dx, dy = 5.0 * np.cos(a), 5.0 * np.sin(a)
            ops.append(("line", cx - dx, cy - dy, cx + dx, cy + dy, 0.6, 0x40208060 + (k << 24 & 0x7F000000)))
    return ops


def check(pm, pmo, r, scene, w, h, lists, maxc=256, frames=1, sync_between=False):
    r.resize(w, h)
    r.set_scene_bytes(scene)
    for _ in range(frames):
        r.render()
        if sync_between:  # (a frame's verdict on its scene reaches the host when the frame is through)
            r.sync()
    got = r.read_pixels()
    P = pmo.Ptcl(scene, w, h)
    try:
        assert np.array_equal(got, P.render())
        per_pixel = sum(1 for ty in range(P.tiles_y) for tx in range(P.tiles_x) if P.solid(tx, ty) == 0 and P.count(tx, ty) > 1)
        queued = r.stats()["queued_tiles"]
        print(f"{w}x{h}: queued_tiles {queued}, oracle per-pixel tiles {per_pixel}, entries {r.binning_plan_info()['entries']}")
        if lists:
            assert queued == per_pixel
            counts, solid, cmds = r.capture_ptcl(maxc)
            for ty in range(P.tiles_y):
                for tx in range(P.tiles_x):
                    oc = P.cmds(tx, ty)
                    assert counts[ty, tx] == len(oc), (tx, ty)
                    assert solid[ty, tx] == P.solid(tx, ty), (tx, ty)
                    assert np.array_equal(cmds[ty, tx, : len(oc)], oc), (tx, ty)
        return queued, per_pixel
    finally:
        P.close()


@pytest.fixture
def fresh(pm, monkeypatch):
    """A renderer of its own, created under the case's switches."""
    made = []

    def make(**env):
        for k in _SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        made.append(pm.Renderer(0))
        return made[-1]

    yield make
    for r in made:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 7, 8, 9])
def test_small_work_lists_around_the_shard_count(pm, pmo, fresh, k):
    """256 x 16k: k work-list entries -- fewer than, as many as and one more than there are shards."""
    r = fresh(PM_BIN_SPLIT="0")
    w, h = 256, 16 * k
    check(pm, pmo, r, encode_ops(pm, crossing_ops(w, h)), w, h, lists=True)
    assert r.binning_plan_info()["entries"] == k


@pytest.mark.gpu
def test_small_partial_last_strip(pm, pmo, fresh):
    """272 x 144: the second strip of every row has one tile."""
    r = fresh()
    check(pm, pmo, r, encode_ops(pm, crossing_ops(272, 144)), 272, 144, lists=True)


@pytest.mark.gpu
def test_small_one_shard_populated(pm, pmo, fresh):
    """One item in tile row 3 of 256 x 256: one work-list entry, one shard; the other seven cursors of every class stay 0."""
    r = fresh()
    scene = encode_ops(pm, [("line", 5.0, 56.0, 250.0, 57.0, 3.0, 0x3050A0C0)])
    queued, _ = check(pm, pmo, r, scene, 256, 256, lists=True)
    assert queued == 16 and r.binning_plan_info()["entries"] == 1


@pytest.mark.gpu
def test_small_every_tile_in_one_class(pm, pmo, fresh):
    r = fresh()
    queued, _ = check(pm, pmo, r, encode_ops(pm, diagonal_ops(256, 256)), 256, 256, lists=True)
    assert queued == 256 and r.stats()["heavy_tiles"] == 0


@pytest.mark.gpu
def test_small_all_eight_classes(pm, pmo, fresh):
    """A fan of N strokes through one tile per row, N on both sides of every class threshold -- alone, and behind other frames
    (whose thresholds differ)."""
    r = fresh()
    w, h = 256, 16 * len(FAN_SIZES)
    scene = encode_ops(pm, fan_ops())
    check(pm, pmo, r, scene, w, h, lists=True, maxc=512)
    assert r.stats()["heavy_tiles"] >= 3
    check(pm, pmo, r, scene, w, h, lists=True, maxc=512, frames=4)


@pytest.mark.gpu
@pytest.mark.parametrize("h", [128, 144])
def test_sub_queues_exactly_full(pm, pmo, fresh, h):
    """4096 x 128 (128 entries, 16 per shard) and 4096 x 144 (144 entries, 18 per shard): every tile is queued, all in one class,
    so every sub-queue of that class holds queue_sub_cap = 16 x entries / 8 tiles -- its last entry included."""
    r = fresh(PM_BIN_SPLIT="0")
    w = 4096
    queued, _ = check(pm, pmo, r, encode_ops(pm, diagonal_ops(w, h)), w, h, lists=True)
    entries = r.binning_plan_info()["entries"]
    assert entries == (w // 256) * (h // 16) and entries % 8 == 0
    assert queued == (w // 16) * (h // 16) == 8 * 16 * (entries // 8) and r.stats()["heavy_tiles"] == 0


@pytest.mark.gpu
def test_chained_strip_rows(pm, pmo, fresh):
    """4096 x 1024 with one binning workgroup per CU: more work-list entries than workgroups, every workgroup walks a chain."""
    r = fresh(PM_BIN_WG_PER_CU="1")
    queued, per_pixel = check(pm, pmo, r, encode_ops(pm, diagonal_ops(4096, 1024)), 4096, 1024, lists=False)
    assert queued == per_pixel == 256 * 64


@pytest.mark.gpu
def test_small_every_strip_row_cut_in_two(pm, pmo, fresh):
    r = fresh(PM_BIN_SPLIT="2")
    w, h = 528, 144
    check(pm, pmo, r, encode_ops(pm, crossing_ops(w, h) + diagonal_ops(w, h)), w, h, lists=True)
    assert r.binning_plan_info()["rows_cut"] > 0 and r.binning_plan_info()["entries"] > 3 * 9


@pytest.mark.gpu
def test_six_frames_in_flight(pm, pmo, fresh):
    """Six frames submitted without a sync, each into a buffer of its own: frames behind running frames bin from the work list
    without cuts, with a wave per row, and are handed out statically; then one more frame, alone again."""
    import torch

    r = fresh(PM_BIN_SPLIT="2")
    w, h = 1040, 272
    scene = encode_ops(pm, crossing_ops(w, h) + diagonal_ops(w, h) + fan_ops(FAN_SIZES[:17], tile_x=40))
    want = pmo.render(scene, w, h)
    r.resize(w, h)
    r.set_scene_bytes(scene)
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(6)]
    for b in bufs:
        r.render_to(b, None)
    r.sync()
    for k, b in enumerate(bufs):
        assert np.array_equal(b.cpu().numpy(), want), k
    r.render()
    assert np.array_equal(r.read_pixels(), want)
    assert r.stats()["overflow"] == 0


@pytest.mark.gpu
def test_small_stand_alone_list_kernel(pm, pmo, fresh):
    """PM_FUSED=0: pm_coarse_kernel reads the cursors itself."""
    r = fresh(PM_FUSED="0")
    check(pm, pmo, r, encode_ops(pm, crossing_ops(272, 144) + fan_ops(FAN_SIZES[:9])), 272, 144, lists=True, maxc=512)


@pytest.mark.gpu
def test_small_one_wave_tile_kernel(pm, pmo, fresh):
    """PM_DENSE_FACTOR so large that one long list makes a frame dense: the frames submitted after the first is through run the
    one-wave-per-tile instantiation, whose verdict and hand-out read sums over a class's shards."""
    r = fresh(PM_DENSE_FACTOR="100000")
    w, h = 256, 16 * len(FAN_SIZES)
    check(pm, pmo, r, encode_ops(pm, fan_ops() + crossing_ops(w, h)), w, h, lists=True, maxc=512, frames=3, sync_between=True)
    assert r.dense_kernel_frames() > 0


@pytest.mark.gpu
def test_small_band_of_three_tile_rows(pm, pmo, fresh):
    r = fresh()
    w, h = 272, 144
    scene = encode_ops(pm, crossing_ops(w, h) + diagonal_ops(w, h))
    r.resize(w, h)
    r.set_scene_bytes(scene)
    r.set_band(2, 5)
    r.render()
    got = r.read_pixels()
    P = pmo.Ptcl(scene, w, h)
    try:
        assert got.shape[0] == 48 and np.array_equal(got, P.render_rows(2, 5))
        assert r.stats()["queued_tiles"] == sum(1 for ty in range(2, 5) for tx in range(P.tiles_x) if P.solid(tx, ty) == 0 and P.count(tx, ty) > 1)
    finally:
        P.close()


@pytest.mark.gpu
def test_small_arena_overflow_repaired_by_sync(pm, pmo, fresh):
    """A tile arena of 64 commands: the first frame overflows (its tiles are queued, marked "no list"), pm_sync grows the arena
    and renders the frame again."""
    r = fresh(PM_PTCL_INITIAL_CMDS="64")
    w, h = 272, 144
    check(pm, pmo, r, encode_ops(pm, crossing_ops(w, h) + diagonal_ops(w, h)), w, h, lists=True)
    st = r.stats()
    assert st["overflow"] == 0 and st["ptcl_used_cmds"] > 64


def test_small_cases_under_the_wave64_emulation(built):
    """The cases named test_small_* above against the kernels compiled as plain C++ and run lane by lane on the CPU (tests/emu/),
    at the emulation's default device and on two CUs (ten binning workgroups: chains of strip rows)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    for extra in ({}, {"PM_EMU_CUS": "2"}):
        env = dict(os.environ, PM_TEST_EMU="1", **extra)
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_small or exactly_full", "-p", "no:cacheprovider", "-n", "4"]
        p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
        assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
        assert " passed" in p.stdout and "failed" not in p.stdout
