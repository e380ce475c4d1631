"""A fixed script of frames for one Renderer (test helper, not a conftest): tests/test_frame_sequences.py runs it under every
row of its table of frame-path switches.

The host decides frame by frame how the same kernels are launched (piet_metal_amd/csrc/pm_context.hip): the binning plan is
remade at the third frame of a plan from the frames' own report, frames behind running frames bin from the work list without
the cuts and get the static tile hand-out, a band, a scene, a viewport or a view change plans again.  The script walks through
all of that on one context and checks every step against the oracle -- pixels after each step, the per-tile command lists after
the re-plan -- and the plan's bookkeeping (pm_binning_plan_info) alongside:
  - plans_fed_back grows by at most one per (scene, viewport, band);
  - where the frames' report can be used (PM_BIN_SPLIT=1, no per-tile-row item lists, a plan with fewer work-list entries than
    the binning grid the report is judged against), the plan in force after the fourth frame was made with it, and at least one
    plan of the sequence was remade from it;
  - PM_BIN_SPLIT=2 without per-tile-row item lists cuts strip rows;
  - with per-tile-row item lists nothing is cut and no plan is remade from a report.
A row may also ask for a larger last scene (more strip rows than a small binning grid), and for the command-list arena to
overflow there, with frames in flight, after every earlier frame of the sequence fitted.

Scenes come from a small pool, each small enough for the CPU emulation of the kernels (tests/emu/): random Encoder calls, the
encoder extensions (even-odd, compound fills, ellipses, nested groups), a small Tiger through the device flatten (and a view
change through pm_reflatten), and geometry far outside the viewport (the encoder's u16 box clamp, edges that cross the whole
viewport, circles wholly off-screen)."""
from __future__ import annotations

import numpy as np

from test_host_cpu import encode_ops, extend_ops, random_ops

TILE = 16


def far_ops(seed: int, w: int, h: int):
    """Geometry far outside a w x h viewport, between a few items on it."""
    rng = np.random.default_rng(seed)
    far = [-7.0e4, -3.0e4, -2.0e3, 4.0e4, 65535.0, 66000.0, 1.0e6]
    pick = lambda: float(far[int(rng.integers(0, len(far)))])
    on = lambda extent: float(rng.uniform(0, extent))
    col = lambda: int(rng.integers(0, 1 << 32)) | (0xFF if rng.random() < 0.5 else 0)
    ops = list(random_ops(seed, 40, extent=float(max(w, h))))
    for k in range(24):
        kind = k % 6
        if kind == 0:  # an edge that crosses the whole viewport
            ops.append(("line", pick(), on(h), -pick() if rng.random() < 0.5 else on(w), on(h), float(rng.uniform(0.5, 9.0)), col()))
        elif kind == 1:  # a fill with vertices far out on several sides and one inside
            ops.append(("fill", np.array([[pick(), on(h)], [on(w), -pick()], [on(w), on(h)], [pick(), pick()]]), col()))
        elif kind == 2:  # circles wholly off-screen
            ops.append(("circle", float(w) + pick() if rng.random() < 0.5 else -pick(), on(h), float(rng.uniform(1, 40))))
        elif kind == 3:  # a polyline that leaves and comes back
            ops.append(("poly", np.array([[on(w), on(h)], [pick(), on(h)], [on(w), pick()], [on(w), on(h)]]), col(), float(rng.uniform(0.2, 6.0))))
        elif kind == 4:  # a fill that covers the viewport from far outside
            a = -pick() if rng.random() < 0.5 else -2.0e3
            ops.append(("fill", np.array([[a, a], [pick(), a], [pick(), pick()], [a, pick()]]), col() & ~0xFF | 0x40))
        else:  # a line wholly off-screen
            y = -pick()
            ops.append(("line", on(w), y, on(w), y - 10.0, 3.0, col()))
    perm = rng.permutation(len(ops))
    return [ops[i] for i in perm]


class FrameSequence:
    """run() walks the script; every check raises AssertionError naming the step."""

    def __init__(self, pm, pmo, renderer, seed: int, split_mode: int = 1, row_lists: bool = False, feedback_grid: int = 0,
                 big=None, overflow_late: bool = False):
        self.pm, self.pmo, self.r = pm, pmo, renderer
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.split_mode = split_mode
        self.row_lists = row_lists  # every band of the script bins through per-tile-row item lists (PM_ROW_LIST_MIN_ITEMS <= 10)
        # the work-list entries below which the third frame's report is read back (n_cus x PM_BIN_WG_PER_CU, or x 5; 0: never)
        self.feedback_grid = feedback_grid if split_mode == 1 and not row_lists else 0
        self.big = big  # (width, height) of a Tiger at the end of the script, or None
        self.overflow_late = overflow_late  # the lists of `big` overflow the arena; nothing before them may
        self.want = None  # the oracle's full frame of the scene and viewport in force
        self.epoch_fed = 0  # plans_fed_back when the (scene, viewport, band) in force began
        self.epoch_frames = 0  # frames submitted since
        self.epoch_entries = None  # work-list entries of the epoch's first plan
        self.epoch_fresh = True  # the epoch began with a plan of its own (a view change may keep the plan in force)
        self.feedback_epochs = 0  # epochs whose report had to be used

    # ---- state changes: each begins a new (scene, viewport, band) ----------------------------------------------------------------
    def _new_epoch(self, fresh=True):
        self.epoch_fed = self.r.binning_plan_info()["plans_fed_back"]
        self.epoch_frames = 0
        self.epoch_entries = None
        self.epoch_fresh = fresh

    def resize(self, w, h):
        self.r.resize(w, h)
        self.w, self.h = w, h
        self._new_epoch()

    def set_scene(self, scene):
        self.scene = scene
        self.r.set_scene_bytes(scene)
        self.want = self.pmo.render(scene, self.w, self.h)
        self._new_epoch()

    def flatten(self, wl, affine, width_scale, reflatten=False):
        if reflatten:
            self.r.reflatten(affine, width_scale)
        else:
            self.r.flatten_and_encode(wl.paths, affine, width_scale)
        self.scene = self.r.download_scene()
        self.want = self.pmo.render(self.scene, self.w, self.h)
        self._new_epoch(fresh=not reflatten)

    def set_band(self, a, b):
        self.r.set_band(a, b)
        self._new_epoch()

    # ---- checks ---------------------------------------------------------------------------------------------------------------
    def check(self, step):
        got = self.r.read_pixels()
        want = self.want[self.r.row0 * TILE : min(self.r.row1 * TILE, self.h)]
        if not np.array_equal(got, want):
            bad = (got != want).any(axis=2)
            tiles = {(y // TILE, x // TILE) for y, x in zip(*np.nonzero(bad))}
            raise AssertionError(f"seed {self.seed}, {step}: {len(tiles)} wrong tiles ({int(bad.sum())} pixels) at {self.w}x{self.h}, "
                                 f"band {self.r.row0}-{self.r.row1}, plan {self.r.binning_plan_info()}")
        self.check_plan(step)

    def check_plan(self, step):
        info = self.r.binning_plan_info()
        fed = info["plans_fed_back"] - self.epoch_fed
        assert fed <= 1, f"seed {self.seed}, {step}: {fed} plans remade from the frames' report on one scene, viewport and band: {info}"
        if self.epoch_entries is None:
            self.epoch_entries = info["entries"]
            if self.epoch_fresh and self.epoch_entries < self.feedback_grid:
                self.feedback_epochs += 1
        if self.epoch_fresh and self.epoch_entries < self.feedback_grid and self.epoch_frames >= 4:
            assert info["fed_back"], f"seed {self.seed}, {step}: the frames' report was not used by the fourth frame: {info}"
        if self.row_lists:
            assert info["rows_cut"] == 0, f"seed {self.seed}, {step}: strip rows cut with per-tile-row item lists: {info}"
            assert fed == 0, f"seed {self.seed}, {step}: a plan with per-tile-row item lists remade from the frames' report: {info}"
        elif self.split_mode == 2:
            assert info["rows_cut"] > 0, f"seed {self.seed}, {step}: PM_BIN_SPLIT=2 cut no strip row: {info}"

    def check_lists(self, step):
        r, pmo = self.r, self.pmo
        P = pmo.Ptcl(self.scene, self.w, self.h)
        try:
            counts, solid, cmds = r.capture_ptcl(1024)
            for ty in range(r.row0, min(r.row1, P.tiles_y)):
                for tx in range(P.tiles_x):
                    oc = P.cmds(tx, ty)
                    y = ty - r.row0
                    ok = counts[y, tx] == len(oc) and solid[y, tx] == P.solid(tx, ty) and np.array_equal(cmds[y, tx, : len(oc)], oc)
                    assert ok, f"seed {self.seed}, {step}: tile ({tx}, {ty}) list differs from the oracle's"
        finally:
            P.close()

    # ---- frames ---------------------------------------------------------------------------------------------------------------
    def lone(self, step):
        self.r.render()
        self.epoch_frames += 1
        if self.overflow_late:  # (pm_get_stats waits for the frame and leaves an overflow for pm_sync to repair)
            assert self.r.stats()["overflow"] == 0, f"seed {self.seed}, {step}: the command-list arena overflowed before the last scene"
        self.r.sync()
        self.check(step)

    def burst(self, step, n=5):
        for _ in range(n):
            self.r.render()
        self.epoch_frames += n
        self.check(step)

    # ---- the script -----------------------------------------------------------------------------------------------------------
    def random_scene(self, w, h, extended=False):
        s = int(self.rng.integers(0, 1 << 30))
        ops = random_ops(s, int(self.rng.integers(150, 300)), extent=float(max(w, h)))
        if extended:
            ops = extend_ops(s, ops)
        return encode_ops(self.pm, ops)

    def run(self):
        rng = self.rng
        # a lone frame, then frames on one scene and viewport past the third-frame re-plan, then the lists it made
        self.resize(400, 320)
        self.set_scene(self.random_scene(400, 320))
        self.lone("first frame")
        for k in range(7):
            self.lone(f"frame {k + 2} on one plan")
        self.check_lists("lists after the re-plan")
        # frames in flight (the work list without the cuts, static hand-out, a wave per strip row)
        self.burst("burst of 5")
        # a band of six random tile rows (twelve strip rows: on two CUs between the five and the seven binning workgroups per CU
        # that EnsureArena cuts within and FeedBackStripRows reads reports below), past its own third-frame report
        a = int(rng.integers(0, 15))
        b = a + 6
        self.set_band(a, b)
        for k in range(4):
            self.lone(f"band {a}-{b} frame {k + 1}")
        self.burst(f"band {a}-{b} in flight", 3)
        # another scene at the same viewport and band, then the whole viewport again
        self.set_scene(self.random_scene(400, 320, extended=True))
        self.lone("extension scene on the band")
        self.set_band(0, 20)
        for k in range(4):
            self.lone(f"extension scene frame {k + 1}")
        self.burst("extension scene in flight", 4)
        self.check_lists("extension scene lists")
        # a viewport that is not a multiple of a tile, with geometry far outside it
        w, h = 389 + int(rng.integers(0, 12)), 301 + int(rng.integers(0, 14))
        self.resize(w, h)
        self.set_scene(encode_ops(self.pm, far_ops(int(rng.integers(0, 1 << 30)), w, h)))
        for k in range(4):
            self.lone(f"far geometry frame {k + 1}")
        self.burst("far geometry in flight")
        self.check_lists("far geometry lists")
        # the device flatten of a small Tiger, then a view change (pm_reflatten)
        self.resize(432, 270)
        wl = self.pm.workloads.tiger(432, 270)
        self.flatten(wl, wl.affine, wl.width_scale)
        for k in range(4):
            self.lone(f"tiger frame {k + 1}")
        self.burst("tiger in flight", 3)
        aff = list(wl.affine)
        aff[0] *= 1.1
        aff[3] *= 1.1
        aff[4] -= 23.5
        aff[5] -= 11.25
        self.flatten(wl, tuple(aff), wl.width_scale * 1.1, reflatten=True)
        self.lone("view change")
        self.burst("view change in flight", 4)
        self.lone("view change, frame alone")
        self.check_lists("view change lists")
        if self.big:
            # more strip rows than a small binning grid (PM_BIN_WG_PER_CU=1 on the MI355X: 544 at 1080p > 256)
            w, h = self.big
            self.resize(w, h)
            wl = self.pm.workloads.tiger(w, h)
            self.flatten(wl, wl.affine, wl.width_scale)
            if self.overflow_late:  # frames in flight overflow the arena sized for the earlier scenes; pm_sync repairs every one
                for _ in range(3):
                    self.r.render()
                self.epoch_frames += 3
                assert self.r.stats()["overflow"] == 1, f"seed {self.seed}: the {w}x{h} tiger's lists did not overflow the arena"
                self.check(f"{w}x{h} tiger in flight, arena overflowed")
                self.overflow_late = False
            self.lone(f"{w}x{h} tiger")
            self.burst(f"{w}x{h} tiger in flight", 3)
        if self.feedback_epochs:
            assert self.r.binning_plan_info()["plans_fed_back"] >= 1, f"seed {self.seed}: no plan was remade from the frames' report"
