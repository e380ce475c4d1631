"""The seven newer query families on the walk of tests/context_model.py (test helper, not a conftest): pm_select_polygon (D20),
pm_snap (D21), pm_item_bounds / pm_union_bounds (D22), pm_snap_intersections (D23), pm_hit_stack / pm_hit_rects_stack (D24) and
pm_item_lengths / pm_points_at_length / pm_positions_on_edges (D25) -- sixteen entry points -- held against the model behind every
state change of a script, and in flight over two side streams across the replacements an `inflight` observation is straddled by.

The QUERY SET is fixed: these calls are independent of pm_resize / pm_set_band, so it is no function of the viewport (the one of
context_model.query_set is).  The length and the edge queries alone come from the scene: from the reference lengths and the reference
snap answers of the model's bytes.  ANSWERS2 are tests/np_poly.py, np_snap.py, np_cross.py, np_bounds.py, np_stack.py and np_measure.py
on the model's expected bytes, never on a downloaded scene.  QUERYRUNNER keeps everything context_model.Runner does and adds the
calls; every comparison is for equality as bytes (the one exception is tests/test_measure.py's: the five floats of a point record whose
located segment has a non-finite end)."""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np

import context_model as cm
import np_bounds
import np_cross
import np_hit
import np_measure as nm
import np_poly
import np_snap
import np_stack

NONE = np_hit.HIT_NONE
UNTOUCHED = cm.UNTOUCHED
INVALID = cm.INVALID
SPARE = 3                      # records or words behind the end of every buffer of a device call: they stay UNTOUCHED
FAMILIES = ("polygon", "snap", "cross", "bounds", "stack", "measure")     # Answers2's; D22 and D25 also have a Python-side part: "paths"
POINT_FLOATS = ("t", "x", "y", "tx", "ty")
SKIP, STOP, EVEN_ODD = 1, 8, 2     # PM_HIT_SKIP_TRANSPARENT, PM_HIT_STOP_AT_OPAQUE, PM_SEL_EVEN_ODD of include/piet_metal_amd.h
SNAP_V, SNAP_E = 2, 4              # PM_SNAP_VERTICES, PM_SNAP_EDGES

# ---- the fixed query set --------------------------------------------------------------------------------------------------------
_GX = [-8.0 + 12.25 * i for i in range(18)]     # -8 .. 200.25
_GY = [-8.0 + 16.25 * j for j in range(12)]     # -8 .. 170.75
GRID = np.array([(x + 0.25, y + 0.5) for y in _GY for x in _GX], np.float32)
RADII = np.array([(0.75, 3.0, 9.0)[k % 3] for k in range(len(GRID))], np.float32)   # mixed: every scene finds something and misses something
HALF = np.float32(4.0)         # half side of the pick squares
_NAN, _INF = np.float32(np.nan), np.float32(np.inf)
PTS = np.concatenate([GRID, np.array([(_NAN, 5.0)], np.float32)])                                                        # + a non-finite point
XYR = np.concatenate([np.concatenate([GRID, RADII[:, None]], axis=1), np.array([(_NAN, 10.0, 5.0), (40.0, 30.0, -1.0), (_INF, 3.0, 2.0)], np.float32)])
SQUARES = np.concatenate([np.concatenate([GRID - HALF, GRID + HALF], axis=1),
                          np.array([(60.0, 40.0, 50.0, 50.0), (10.0, _NAN, 30.0, 30.0)], np.float32)])              # + an inverted and a non-finite one
LASSO = np.array([(20, 15), (150, 25), (185, 120), (110, 150), (30, 140), (70, 80)], np.float32)    # concave at (70, 80)
# self-intersecting: an outer loop and an inner loop in the same sense, the closing edge crosses (0, 30)-(120, 30); the inner
# region winds twice -- inside by the non-zero rule, outside by the even-odd rule
SPIRAL = np.array([(0, 0), (200, 0), (200, 170), (0, 170), (0, 30), (120, 30), (120, 140), (30, 140)], np.float32)
STACK_K = (1, 4, 16)           # the deepest stack of the pool scenes is 14: 4 clips, 16 pads with PM_HIT_NONE
N_LABELS = 4                   # union_bounds: item i carries label i % 3, label 3 nobody


def labels_of(n_items):
    return (np.arange(n_items, dtype=np.uint32) % 3).astype(np.uint32)


def length_queries(lengths):
    """LENGTH_QUERY records from the reference lengths (no flag): s in {0, T/3, T, T+1} for every third item, and the item n_items."""
    pairs = [(i, s) for i in range(0, len(lengths), 3) for T in [int(lengths["length"][i])] for s in (0, T // 3, T, T + 1)]
    pairs.append((len(lengths), 7))
    q = np.zeros(len(pairs), nm.LENGTH_QUERY)
    q["item"], q["s"] = [p[0] for p in pairs], np.array([p[1] for p in pairs], np.uint64)
    return q


def edge_queries(snapped, n_items):
    """EDGE_QUERY records from the reference snap answers (edges alone, no flag): {item, index, t} of every query that found
    something, then an item out of range, an index that names no segment and a t beyond 1."""
    found = snapped[snapped["item"] != NONE]
    n = len(found)
    q = np.zeros(n + 3, nm.EDGE_QUERY)
    q["item"][:n], q["index"][:n], q["t"][:n] = found["item"], found["index"], found["t"]
    q["item"][n:] = (n_items, 0, 0)
    q["index"][n:] = (0, 0x00FFFFFF, 0)
    q["t"][n:] = (0.5, 0.5, 1.5)
    return q


@dataclass(frozen=True)
class Flags:
    skip: bool = False
    stop: bool = False
    even_odd: bool = False
    counts: bool = False
    vertices: bool = True
    edges: bool = True
    k: int = 4
    mask: int = np_poly.TOUCHES      # the bit of the lasso's words that union_bounds selects by

    def hit(self):
        return SKIP if self.skip else 0

    def snap(self):
        return self.hit() | (SNAP_V if self.vertices else 0) | (SNAP_E if self.edges else 0)

    def stack(self):
        return self.hit() | (STOP if self.stop else 0)

    def poly(self):
        return self.hit() | (EVEN_ODD if self.even_odd else 0)


def draw_flags(seed, index):
    """The flags of the calls behind step `index` of script `seed`: a function of the two alone."""
    rng = np.random.default_rng([zlib.crc32(str(seed).encode()), index, 0xF1A6])
    b = [bool(v) for v in rng.integers(0, 2, 4)]
    v, e = ((True, True), (True, False), (False, True))[int(rng.integers(0, 3))]
    return Flags(b[0], b[1], b[2], b[3], v, e, STACK_K[int(rng.integers(0, 3))], (np_poly.TOUCHES, np_poly.ENCLOSES)[int(rng.integers(0, 2))])


class Answers2:
    """The references on scene bytes, cached by (scene, family, the flags the family reads).  get() returns name -> array (the stacks:
    (items, n_hit))."""

    def __init__(self):
        self.cache = {}

    def _cached(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    @staticmethod
    def _id(scene):
        return (hash(scene.tobytes()), len(scene))

    def lasso_words(self, scene, skip, even_odd):
        return self.get("polygon", scene, Flags(skip=skip, even_odd=even_odd))["lasso"]

    def measure_queries(self, scene):
        """(LENGTH_QUERY, EDGE_QUERY) records of the scene: from the reference alone."""
        def make():
            n = cm.n_flat_items(scene)
            edges = self._cached(("snap1", self._id(scene), False, False, True), lambda: np_snap.snap(scene, XYR, vertices=False, edges=True))
            return length_queries(nm.item_lengths(scene)), edge_queries(edges, n)
        return self._cached(("measure_q", self._id(scene)), make)

    def get(self, family, scene, f: Flags):
        sid = self._id(scene)
        if family == "polygon":
            return self._cached((family, sid, f.skip, f.even_odd), lambda: {
                name: np_poly.item_flags(scene, poly, skip_transparent=f.skip, even_odd=f.even_odd).astype(np.uint32) for name, poly in (("lasso", LASSO), ("spiral", SPIRAL))})
        if family == "snap":
            plain = self._cached(("snap1", sid, f.skip, f.vertices, f.edges), lambda: np_snap.snap(scene, XYR, f.vertices, f.edges, f.skip))
            masked = self._cached(("snap2", sid, f.skip, f.vertices, f.edges, f.even_odd),
                                  lambda: np_snap.snap(scene, XYR, f.vertices, f.edges, f.skip, skip_items=self.lasso_words(scene, f.skip, f.even_odd)))
            return {"snap": plain, "snap_masked": masked}
        if family == "cross":
            return self._cached((family, sid, f.skip), lambda: {"cross": np_cross.cross(scene, XYR, skip_transparent=f.skip)})
        if family == "bounds":
            def make():
                boxes = np_bounds.item_bounds(scene, f.skip)
                words = self.lasso_words(scene, f.skip, f.even_odd)
                return {"item_bounds": boxes, "union_bounds": np_bounds.union_bounds(scene, N_LABELS, labels_of(len(boxes)), words, f.mask, f.skip, boxes=boxes)}
            return self._cached((family, sid, f.skip, f.even_odd, f.mask), make)
        if family == "stack":
            members = self._cached(("members", sid), lambda: (np_stack.point_members(scene, PTS), np_stack.rect_members(scene, SQUARES)))
            return self._cached((family, sid, f.skip, f.stop, f.k), lambda: {
                "hit_stack": np_stack.hit_stack(scene, PTS, f.k, f.skip, f.stop, members=members[0]),
                "hit_rects_stack": np_stack.hit_rects_stack(scene, SQUARES, f.k, f.skip, f.stop, members=members[1])})
        if family == "measure":
            def make():
                lq, eq = self.measure_queries(scene)
                ws = nm.walks(scene, f.skip)
                return {"lengths": nm.item_lengths(scene, f.skip, ws=ws), "points": nm.points_at_length(scene, list(zip(lq["item"].tolist(), lq["s"].tolist())), f.skip, ws=ws),
                        "positions": nm.positions_on_edges(scene, list(zip(eq["item"].tolist(), eq["index"].tolist(), eq["t"].tolist())), f.skip, ws=ws), "ws": ws}
            return self._cached((family, sid, f.skip), make)
        raise KeyError(family)

    def paths(self, scene, path_of_item, gmap, f: Flags):
        """What Renderer.group_bounds and Renderer.path_lengths answer for a scene that came from the paths: the labels are the
        CURRENT map composed with the model's path_of_item (label 0 everywhere without a map), the lengths are summed per path."""
        gkey = None if gmap is None else np.asarray(gmap, np.uint32).tobytes()

        def make():
            if gmap is None:
                gb = np_bounds.union_bounds(scene, 1, None, None, 3, f.skip)
            else:
                g = np.asarray(gmap, np.uint32)
                gb = np_bounds.union_bounds(scene, int(g.max()) + 1 if len(g) else 1, g[path_of_item], None, 3, f.skip)
            rec = self.get("measure", scene, f)["lengths"]
            n_paths = int(path_of_item.max()) + 1 if len(path_of_item) else 0
            lengths, counts = [0] * n_paths, [0] * n_paths
            for p, v in zip(path_of_item.tolist(), rec["length"].tolist()):
                lengths[p] += int(v)
                counts[p] += 1
            return {"group_bounds": gb, "path_lengths": np.array([lengths, counts], np.uint64)}
        return self._cached(("paths", self._id(scene), gkey, f.skip), make)


def loose_points(ws, want):
    """bool [n]: the point records whose located segment has a non-finite end (tests/test_measure.py: unpromised)."""
    out = np.zeros(len(want), bool)
    for j, rec in enumerate(want):
        if rec["item"] != NONE and int(rec["item"]) < len(ws):
            out[j] = nm.has_non_finite_end(ws[int(rec["item"])], int(rec["index"]))
    return out


def _b(a):
    return np.ascontiguousarray(a).tobytes()


# ---- the runner -----------------------------------------------------------------------------------------------------------------

# the state changes behind which every answer must be the one in front of them (the query set is fixed; the bytes stay)
SAME_ANSWERS = {("invalid", v) for v in cm.VARIANTS["invalid"]} | {("repaint", "identity"), ("reflatten_groups", "equal")} | \
    {("resize", v) for v in cm.VARIANTS["resize"]} | {("band", v) for v in cm.VARIANTS["band"]}


class QueryRunner(cm.Runner):
    """cm.Runner, and behind every state change every new call once through its synchronous Python method; with an `inflight`
    observation the device variant of every new call over two side streams."""

    def __init__(self, pm, pmo, r, script, seed, answers=None, answers2=None):
        super().__init__(pm, pmo, r, script, seed, answers=answers)
        self.answers2 = answers2 or Answers2()
        self.pending2 = []
        self.last = None        # (flags, name -> bytes) of the calls behind the state change in front
        self.calls_made = 0
        self.side2 = None if self.dev.emu else self.dev.torch.cuda.Stream()

    # -- buffers of the device calls --
    def _blank(self, rows, words=None):
        """int32 [rows(, words)] of UNTOUCHED: torch on the GPU, numpy under the emulation."""
        shape = (rows,) if words is None else (rows, words)
        if self.dev.emu:
            return np.full(shape, UNTOUCHED, np.int32)
        return self.dev.torch.full(shape, UNTOUCHED, dtype=self.dev.torch.int32, device="cuda:0")

    def _put(self, a):
        """A numpy array (records as rows of int32 words) in device memory."""
        a = np.ascontiguousarray(a)
        if a.dtype.names or a.dtype == np.uint32:
            a = a.view(np.int32).reshape(len(a), -1) if a.dtype.names else a.view(np.int32)
        return a.copy() if self.dev.emu else self.dev.torch.from_numpy(a.copy()).cuda()

    def _host(self, t):
        """int32 words of a buffer, on the host."""
        return np.ascontiguousarray(t if isinstance(t, np.ndarray) else t.cpu().numpy()).view(np.int32)

    @staticmethod
    def _ptr(t):
        return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()

    # -- the synchronous calls --
    def sync_calls(self, f: Flags, n_items):
        """name -> answer of every new call through its Python method, in the order of the chain: the lasso's words go into
        union_bounds and into snap(skip_items=...)."""
        r, got = self.r, {}
        xy, rad = XYR[:, :2], XYR[:, 2]
        lasso = r.select_polygon(LASSO, skip_transparent=f.skip, even_odd=f.even_odd)
        got["lasso"] = lasso[0] * np.uint32(np_poly.TOUCHES) + lasso[1] * np.uint32(np_poly.ENCLOSES)
        star = r.select_polygon(SPIRAL, skip_transparent=f.skip, even_odd=f.even_odd)
        got["spiral"] = star[0] * np.uint32(np_poly.TOUCHES) + star[1] * np.uint32(np_poly.ENCLOSES)
        got["snap"] = r.snap(xy, rad, vertices=f.vertices, edges=f.edges, skip_transparent=f.skip)
        got["snap_masked"] = r.snap(xy, rad, vertices=f.vertices, edges=f.edges, skip_transparent=f.skip, skip_items=got["lasso"])
        got["cross"] = r.snap_intersections(xy, rad, skip_transparent=f.skip)
        got["item_bounds"] = r.item_bounds(skip_transparent=f.skip)
        got["union_bounds"] = r.union_bounds(labels_of(n_items), N_LABELS, item_flags=got["lasso"], mask=f.mask, skip_transparent=f.skip)
        for name, call, q in (("hit_stack", r.hit_stack, PTS), ("hit_rects_stack", r.hit_rects_stack, SQUARES)):
            out = call(q, f.k, skip_transparent=f.skip, stop_at_opaque=f.stop, counts=f.counts)
            got[name] = out if f.counts else (out,)
        lq, eq = self.answers2.measure_queries(self.m.expected()[0])
        got["lengths"] = r.item_lengths(skip_transparent=f.skip)
        got["points"] = r.points_at_units(lq["item"], lq["s"], skip_transparent=f.skip)
        got["positions"] = r.positions_on_edges(eq["item"], eq["index"], eq["t"], skip_transparent=f.skip)
        self.calls_made += 12
        return got

    def wanted(self, scene, f: Flags):
        want = {}
        for family in FAMILIES:
            want.update(self.answers2.get(family, scene, f))
        return want

    def compare(self, got, want, what):
        """Every answer equal as bytes to the reference (the stacks: items, and the counts where they were asked for)."""
        ws = want["ws"]
        for name, g in got.items():
            w = want[name]
            if name in ("hit_stack", "hit_rects_stack"):
                for gg, ww, part in zip(g, w, ("items", "n_hit")):
                    self.check(gg.shape == ww.shape and _b(gg) == _b(ww), f"{what}: {name} {part} differs at {np.argwhere(gg != ww)[:4].tolist() if gg.shape == ww.shape else gg.shape}")
                continue
            g = np.ascontiguousarray(g)
            self.check(len(g) == len(w), f"{what}: {name} has {len(g)} records, expected {len(w)}")
            if name == "points":
                g, w = g.copy(), w.copy()
                loose = loose_points(ws, w)
                for fl in POINT_FLOATS:
                    g[fl][loose] = 0
                    w[fl][loose] = 0
            if _b(g) != _b(w):
                size = max(g.dtype.itemsize * (int(np.prod(g.shape[1:])) if g.ndim > 1 else 1), 1)
                bad = np.flatnonzero((np.frombuffer(_b(g), np.uint8).reshape(-1, size) != np.frombuffer(_b(w), np.uint8).reshape(-1, size)).any(axis=1))
                self.check(False, f"{what}: {name} differs in {len(bad)} of {len(w)} records, first {[(int(k), g[k], w[k]) for k in bad[:3]]}")

    def path_calls(self, f: Flags, scene, paths):
        """Renderer.group_bounds and Renderer.path_lengths: answers for a scene from the paths, refused for an upload."""
        r, m = self.r, self.m
        if paths is None:
            self.refused(lambda: r.group_bounds(skip_transparent=f.skip), "group_bounds of an uploaded scene")
            self.refused(lambda: r.path_lengths(skip_transparent=f.skip), "path_lengths of an uploaded scene")
            return {}
        want = self.answers2.paths(scene, paths, m.gmap, f)
        gb = r.group_bounds(skip_transparent=f.skip)
        lengths, counts = r.path_lengths(skip_transparent=f.skip)
        self.check(len(gb) == len(want["group_bounds"]) and _b(gb) == _b(want["group_bounds"]),
                   f"group_bounds is not the union per group of the current map ({len(gb)} groups, expected {len(want['group_bounds'])})")
        self.check([lengths, counts] == want["path_lengths"].tolist(), "path_lengths is not the sum of the reference lengths per path")
        return {"group_bounds": gb, "path_lengths": np.array([lengths, counts], np.uint64)}

    # -- no scene: every entry point refuses and writes nothing --
    def all_refused(self):
        lib, h, P = self.lib, self.r._h, self._ptr
        host = lambda words: np.full(words, UNTOUCHED, np.int32)   # noqa: E731
        dev = lambda words: self._blank(words)                      # noqa: E731
        xy, xyr, sq = PTS[:4].copy(), XYR[:4].copy(), SQUARES[:4].copy()
        lq, eq = np.zeros(4, nm.LENGTH_QUERY), np.zeros(4, nm.EDGE_QUERY)
        d_xy, d_xyr, d_sq, d_lq, d_eq = (self._put(a) for a in (xy, xyr, sq, lq, eq))
        self.dev.filled()
        n = C.c_uint32(UNTOUCHED)
        outs = []

        def out(make, words):
            outs.append(make(words))
            return P(outs[-1])

        calls = [
            ("pm_select_polygon", lambda: lib.pm_select_polygon(h, LASSO.ctypes.data, len(LASSO), 0, out(host, 8), 8, None, None, None)),
            ("pm_select_polygon_device", lambda: lib.pm_select_polygon_device(h, LASSO.ctypes.data, len(LASSO), 0, out(dev, 8), 8, None)),
            ("pm_snap", lambda: lib.pm_snap(h, P(xyr), 4, SNAP_V | SNAP_E, None, 0, out(host, 32))),
            ("pm_snap_device", lambda: lib.pm_snap_device(h, P(d_xyr), 4, SNAP_V | SNAP_E, None, 0, out(dev, 32), None)),
            ("pm_snap_intersections", lambda: lib.pm_snap_intersections(h, P(xyr), 4, 0, None, 0, out(host, 48))),
            ("pm_snap_intersections_device", lambda: lib.pm_snap_intersections_device(h, P(d_xyr), 4, 0, None, 0, out(dev, 48), None)),
            ("pm_item_bounds", lambda: lib.pm_item_bounds(h, 0, out(host, 64), 8, C.byref(n))),
            ("pm_item_bounds_device", lambda: lib.pm_item_bounds_device(h, 0, out(dev, 64), 8, None)),
            ("pm_union_bounds", lambda: lib.pm_union_bounds(h, 0, None, 0, 0, None, 0, 2, out(host, 20))),
            ("pm_union_bounds_device", lambda: lib.pm_union_bounds_device(h, 0, None, 0, 0, None, 0, 2, out(dev, 20), None)),
            ("pm_hit_stack", lambda: lib.pm_hit_stack(h, P(xy), 4, 4, 0, out(host, 16), out(host, 4))),
            ("pm_hit_stack_device", lambda: lib.pm_hit_stack_device(h, P(d_xy), 4, 4, 0, out(dev, 16), out(dev, 4), None)),
            ("pm_hit_rects_stack", lambda: lib.pm_hit_rects_stack(h, P(sq), 4, 4, STOP, out(host, 16), out(host, 4))),
            ("pm_hit_rects_stack_device", lambda: lib.pm_hit_rects_stack_device(h, P(d_sq), 4, 4, STOP, out(dev, 16), out(dev, 4), None)),
            ("pm_item_lengths", lambda: lib.pm_item_lengths(h, 0, out(host, 32), 8, C.byref(n))),
            ("pm_item_lengths_device", lambda: lib.pm_item_lengths_device(h, 0, out(dev, 32), 8, None)),
            ("pm_points_at_length", lambda: lib.pm_points_at_length(h, P(lq), 4, 0, out(host, 32))),
            ("pm_points_at_length_device", lambda: lib.pm_points_at_length_device(h, P(d_lq), 4, 0, out(dev, 32), None)),
            ("pm_positions_on_edges", lambda: lib.pm_positions_on_edges(h, P(eq), 4, 0, out(host, 16))),
            ("pm_positions_on_edges_device", lambda: lib.pm_positions_on_edges_device(h, P(d_eq), 4, 0, out(dev, 16), None)),
        ]
        assert len(calls) == 20   # every host call of the seven families and its device variant
        for name, call in calls:
            first = len(outs)
            st = call()
            self.check(st == INVALID, f"{name} without a scene: status {st}, not {INVALID}")
            if name in ("pm_item_bounds", "pm_item_lengths"):   # (the one word they report: no items)
                self.check(n.value == 0, f"{name} without a scene reports {n.value} items")
                n.value = UNTOUCHED
            for t in outs[first:]:
                self.check((self._host(t) == UNTOUCHED).all(), f"{name} without a scene wrote into its output")
        self.refused(self.r.group_bounds, "group_bounds without a scene")
        self.refused(self.r.path_lengths, "path_lengths without a scene")
        self.calls_made += len(calls) + 2

    # -- behind every state change --
    def change(self, s: cm.Step):
        index = self.executed
        super().change(s)
        ex = self.m.expected()
        if ex is None:
            self.all_refused()
            self.last = None
            return
        scene, n_items, paths = ex
        same = (s.kind, s.variant) in SAME_ANSWERS and self.last is not None
        f = self.last[0] if same else draw_flags(self.seed, index)   # (the step in front's flags: the answers are compared with its)
        what = f"behind the state change ({f})"
        got = self.sync_calls(f, n_items)
        self.compare(got, self.wanted(scene, f), what)
        got.update(self.path_calls(f, scene, paths))
        as_bytes = {name: b"".join(_b(p) for p in g) if isinstance(g, tuple) else _b(g) for name, g in got.items()}
        if same:
            moved = [name for name in as_bytes if as_bytes[name] != self.last[1].get(name)]
            self.check(not moved and set(as_bytes) == set(self.last[1]), f"{s.kind}:{s.variant} changed the answers of {moved}")
        self.last = (f, as_bytes)

    # -- in flight --
    def enqueue2(self, f: Flags, scene, n_items):
        """The device variant of every new call, nothing waited for, alternating over two side streams A, B, A, ...: a call that
        reads what another one wrote (the lasso's words) goes to the stream of that one."""
        r, d, lib, P = self.r, self.dev, self.lib, self._ptr
        lq, eq = self.answers2.measure_queries(scene)
        n, nq, ns = len(XYR), len(PTS), len(SQUARES)
        B = {"xyr": self._put(XYR), "pts": self._put(PTS), "squares": self._put(SQUARES), "labels": self._put(labels_of(n_items)), "lq": self._put(lq), "eq": self._put(eq),
             "lasso": self._blank(n_items + SPARE), "spiral": self._blank(n_items + SPARE), "snap_masked": self._blank(n + SPARE, 8), "cross": self._blank(n + SPARE, 12),
             "item_bounds": self._blank(n_items + SPARE, 8), "union_bounds": self._blank(N_LABELS + SPARE, 10),
             "hit_stack": (self._blank(nq + SPARE, f.k), self._blank(nq + SPARE)), "hit_rects_stack": (self._blank(ns + SPARE, f.k), self._blank(ns + SPARE)),
             "lengths": self._blank(n_items + SPARE, 4), "points": self._blank(len(lq) + SPARE, 8), "positions": self._blank(len(eq) + SPARE, 4)}
        d.filled()   # (the fills and the uploads ran on torch's current stream: nothing else orders them with the side streams)
        if d.emu:
            chk = self.pm._lib.check
            emu = [
                lambda: chk(lib.pm_select_polygon_device(r._h, LASSO.ctypes.data, len(LASSO), f.poly(), P(B["lasso"]), n_items + SPARE, None), "pm_select_polygon_device"),
                lambda: chk(lib.pm_select_polygon_device(r._h, SPIRAL.ctypes.data, len(SPIRAL), f.poly(), P(B["spiral"]), n_items + SPARE, None), "pm_select_polygon_device"),
                lambda: chk(lib.pm_snap_device(r._h, P(B["xyr"]), n, f.snap(), P(B["lasso"]), n_items + SPARE, P(B["snap_masked"]), None), "pm_snap_device"),
                lambda: chk(lib.pm_snap_intersections_device(r._h, P(B["xyr"]), n, f.hit(), None, 0, P(B["cross"]), None), "pm_snap_intersections_device"),
                lambda: chk(lib.pm_union_bounds_device(r._h, f.hit(), P(B["lasso"]), n_items + SPARE, f.mask, P(B["labels"]), n_items, N_LABELS, P(B["union_bounds"]), None),
                            "pm_union_bounds_device"),
                lambda: chk(lib.pm_item_bounds_device(r._h, f.hit(), P(B["item_bounds"]), n_items + SPARE, None), "pm_item_bounds_device"),
                lambda: chk(lib.pm_hit_stack_device(r._h, P(B["pts"]), nq, f.k, f.stack(), P(B["hit_stack"][0]), P(B["hit_stack"][1]), None), "pm_hit_stack_device"),
                lambda: chk(lib.pm_hit_rects_stack_device(r._h, P(B["squares"]), ns, f.k, f.stack(), P(B["hit_rects_stack"][0]), P(B["hit_rects_stack"][1]), None),
                            "pm_hit_rects_stack_device"),
                lambda: chk(lib.pm_item_lengths_device(r._h, f.hit(), P(B["lengths"]), n_items + SPARE, None), "pm_item_lengths_device"),
                lambda: chk(lib.pm_points_at_length_device(r._h, P(B["lq"]), len(lq), f.hit(), P(B["points"]), None), "pm_points_at_length_device"),
                lambda: chk(lib.pm_positions_on_edges_device(r._h, P(B["eq"]), len(eq), f.hit(), P(B["positions"]), None), "pm_positions_on_edges_device"),
            ]
            for call in emu:
                call()
        else:
            kw = {"skip_transparent": f.skip}
            f64 = self.dev.torch.float64
            gpu = [
                lambda s: r.select_polygon_tensor(LASSO, B["lasso"], stream=s, even_odd=f.even_odd, **kw),
                lambda s: r.select_polygon_tensor(SPIRAL, B["spiral"], stream=s, even_odd=f.even_odd, **kw),
                lambda s: r.snap_tensor(B["xyr"], B["snap_masked"][:n], skip_items=B["lasso"], stream=s, vertices=f.vertices, edges=f.edges, **kw),
                lambda s: r.snap_intersections_tensor(B["xyr"], B["cross"][:n], stream=s, **kw),
                lambda s: r.union_bounds_tensor(B["union_bounds"][:N_LABELS], labels=B["labels"], item_flags=B["lasso"], mask=f.mask, stream=s, **kw),
                lambda s: r.item_bounds_tensor(B["item_bounds"].view(f64), stream=s, **kw),
                lambda s: r.hit_stack_tensor(B["pts"], B["hit_stack"][0][:nq], B["hit_stack"][1][:nq], stream=s, stop_at_opaque=f.stop, **kw),
                lambda s: r.hit_rects_stack_tensor(B["squares"], B["hit_rects_stack"][0][:ns], B["hit_rects_stack"][1][:ns], stream=s, stop_at_opaque=f.stop, **kw),
                lambda s: r.item_lengths_tensor(B["lengths"], stream=s, **kw),
                lambda s: r.points_at_length_tensor(B["lq"], B["points"][:len(lq)], stream=s, **kw),
                lambda s: r.positions_on_edges_tensor(B["eq"], B["positions"][:len(eq)], stream=s, **kw),
            ]
            # (0 lasso: A; 2 snap and 4 union_bounds read its words: A too)
            for k, call in enumerate(gpu):
                call((d.side, self.side2)[k % 2])
        self.calls_made += 11
        return B

    def observe(self, index, s: cm.Step):
        super().observe(index, s)
        ex = self.m.expected()
        if s.kind == "inflight" and ex is not None:
            f = draw_flags(self.seed, index)
            f = Flags(s.args["skip"], f.stop, f.even_odd, True, f.vertices, f.edges, f.k, f.mask)   # (the observation's own skip flag: what `blind` made sure of)
            self.pending2.append((index, ex[0], ex[1], f, self.enqueue2(f, ex[0], ex[1])))

    def flush(self):
        if self.pending2:
            self.r.sync()
            self.dev.wait()
            if self.side2 is not None:
                self.side2.synchronize()
        super().flush()
        for index, scene, n_items, f, B in self.pending2:
            what = f"in flight since step {index} ({f})"
            want = self.wanted(scene, f)
            lq, eq = self.answers2.measure_queries(scene)
            sizes = {"lasso": (n_items, None), "spiral": (n_items, None), "snap_masked": (len(XYR), np_snap.RECORD), "cross": (len(XYR), np_cross.RECORD),
                     "item_bounds": (n_items, np.float64), "union_bounds": (N_LABELS, np_bounds.LABEL_BOUNDS), "lengths": (n_items, nm.ITEM_LENGTH),
                     "points": (len(lq), nm.LENGTH_POINT), "positions": (len(eq), nm.LENGTH_AT)}
            got = {}
            for name, (n, dtype) in sizes.items():
                words = self._host(B[name])
                rows = words.reshape(len(words), -1)
                self.check((rows[n:] == UNTOUCHED).all(), f"{what}: {name} wrote behind its {n} records")
                head = np.ascontiguousarray(rows[:n])
                got[name] = head.view(np.uint32).reshape(-1) if dtype is None else head.view(np.float64).reshape(n, 4) if dtype is np.float64 else head.view(dtype).reshape(n)
            for name, n in (("hit_stack", len(PTS)), ("hit_rects_stack", len(SQUARES))):
                items, cnt = (self._host(t) for t in B[name])
                self.check((items[n:] == UNTOUCHED).all() and (cnt[n:] == UNTOUCHED).all(), f"{what}: {name} wrote behind its {n} queries")
                got[name] = (items[:n].view(np.uint32), cnt[:n].view(np.uint32))
            self.compare(got, want, what + ": not the answer for the scene current at the call")
        self.pending2 = []
