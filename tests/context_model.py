"""One pm_ctx through interleaved replacements, frames and queries (test helper, not a conftest): a model of what a caller is
entitled to believe about the context, a generator of scripts over a fixed alphabet, and a runner that walks a script on one
Renderer.  tests/test_context_sequences.py runs the committed seeds; tests/dev/fuzz_context.py an open range of them.

The MODEL holds viewport and band, the resident paths (styles and dash table), the group map, the paint (the table of the last
repaint and the map it went through: per-path painted colours), the transform last applied (a uniform affine and scale, or a table
indexed through the map resident at that call) and where the resident scene came from (the paths, an upload, or none).  Its expected
scene bytes are `np_paint.painted` -> `np_groups.scene` with the oracle's `scene_from_paths`, or the uploaded bytes: it writes no
flatten, stroke, dash, paint or hit rule again.  The lifetime rules are those of include/piet_metal_amd.h:
  - the paint stays with the paths until new paths come; a new map does not repaint; pm_reflatten ignores and keeps the map;
  - an upload leaves paths, map and paint resident, but repaint_groups and item_paths are invalid until the next re-flatten;
  - an invalid-argument call changes nothing;
  - a replacement that fails after it started leaves no scene (render and every query refused, stats()["n_items"] == 0, an empty
    download), the paths stay: a later reflatten brings a scene back, with its paint.

A SCRIPT is a list of Steps, every argument concrete: `generate(seed)` draws it on the CPU against the model and the oracle and
rejects a state change that would be blind (see `blind`), so a seed always gives the same script.  The RUNNER compares, after every
state change, download_scene() and the returned (nbytes, n_items) with the model; frames with pmo.render(model bytes) over the band's
rows; queries with np_hit / np_rect on the model's bytes; all for equality."""
from __future__ import annotations

import ctypes as C
import os
import struct
from dataclasses import dataclass, field

import numpy as np

import np_groups
import np_hit
import np_paint
import np_rect
import path_sets
from np_stroke import style_bits
from test_host_cpu import encode_ops, extend_ops, random_ops
from test_stroke_gpu import shapes

TILE = 16
INVALID, CAPACITY = -1, -4
UNTOUCHED = 0x7EADBEEF

STATE_OPS = ("flatten", "upload", "reflatten", "groups", "reflatten_groups", "repaint", "resize", "band", "invalid", "fail")
FRAME_OBS = ("lone", "burst", "inflight")
QUERY_OBS = ("hit_test", "hit_frame", "hit_rects", "select_rect")
OTHER_OBS = ("item_paths", "fill_coverage", "capture_ptcl")
OBS = FRAME_OBS + QUERY_OBS + OTHER_OBS

VARIANTS = {
    "flatten": ("strokes_dashed_grouped", "strokes_plain", "random_a", "random_b_grouped"),
    "upload": ("nested_a", "nested_b"),
    "reflatten": ("base", "subtile", "tiles", "width"),
    "groups": ("one", "interleaved", "per_path", "unused"),
    "reflatten_groups": ("one_subtile", "one_far", "equal"),
    "repaint": ("fade0", "half", "solid", "tint", "identity"),
    "resize": ("odd", "even"),
    "band": ("rows", "whole"),
    "invalid": ("short_table", "opacity256", "groups_len", "query_flag"),
    "fail": ("cap", "malformed"),
}
# state changes whose contract is that the scene bytes stay as they are: `blind` asks for identical bytes instead of a changed frame
SAME_BYTES = {("invalid", v) for v in VARIANTS["invalid"]} | {("repaint", "identity"), ("reflatten_groups", "equal")} | {("groups", v) for v in VARIANTS["groups"]}
# what may stand behind a failed replacement: one refused operation, then a recovery
RECOVERIES = ("flatten", "upload", "reflatten", "reflatten_groups")
# the replacements an `inflight` observation is straddled by (the others leave the scene bytes alone: nothing could be seen)
STRADDLERS = ("flatten", "upload", "reflatten", "reflatten_groups", "repaint")
# how often the walk tries each state change (the ones with the most preconditions more often, so that their pairs occur)
WEIGHTS = {"repaint": 4, "reflatten_groups": 2, "groups": 2, "band": 2}
VIEWPORTS = {"even": (192, 160), "odd": (189, 149)}
BAND_ROWS = (2, 7)


@dataclass
class Step:
    kind: str                 # a state change of STATE_OPS or an observation of OBS
    variant: str = ""
    args: dict = field(default_factory=dict)

    def __repr__(self):
        a = {k: (v if np.isscalar(v) or isinstance(v, (str, tuple, bool)) else "...") for k, v in self.args.items()}
        return f"{self.kind}:{self.variant}{a if a else ''}"


# ---- the pool ------------------------------------------------------------------------------------------------------------------

@dataclass
class PoolSet:
    name: str
    ps: object
    affine: tuple
    scale: float


RANDOM_A, RANDOM_B = 500, 513   # path_sets.random_case seeds (tests/test_paint_gpu.py renders both)
_pool = {}


def pool(pm):
    """name -> PoolSet / scene bytes.  (1) test_stroke_gpu.shapes() with mixed styles and three dashed paths (decisions D14, D15);
    (2) path_sets.random_case: fills, compound fills, curves; (3) encoder scenes with nested groups, ellipses and even-odd fills."""
    if _pool:
        return _pool
    strokes = shapes(lambda k: (3 if k % 3 == 0 else 2) | style_bits(k % 3, (k // 3) % 3), width=6.0)
    strokes.paths["fill_rgba"] |= 0xFF   # (opaque fills: the triangle covers whole tiles under the scaled views)
    n = len(strokes.paths)
    view = (1.1, 0.0, 0.0, 1.1, 4.0, 2.0)
    _pool["strokes_dashed_grouped"] = PoolSet("strokes_dashed_grouped", strokes.with_dashes([6, 3, 2], -4.0, select=[0, 3, 9]).with_groups(np.arange(n) % 3), view, 1.0)
    _pool["strokes_plain"] = PoolSet("strokes_plain", strokes.with_groups(None), (1.0, 0.0, 0.0, 1.0, 9.0, 3.0), 1.0)
    a, b = path_sets.random_case(RANDOM_A), path_sets.random_case(RANDOM_B)
    _pool["random_a"] = PoolSet("random_a", a.ps, a.affine, a.scale)
    _pool["random_b_grouped"] = PoolSet("random_b_grouped", b.ps.with_groups(np.arange(len(b.ps.paths)) % 2), b.affine, b.scale)
    # (for the written-out scripts only: a few shapes within three tiles of each other, so that a move of several tiles puts them into
    #  strip rows nothing reached before while every item still reaches the band)
    local = path_sets.pathset((path_sets._square(20, 6, 26), path_sets.FILL | path_sets.STROKE), (path_sets._tri(60, 4), path_sets.FILL | path_sets.STROKE, 3.0),
                              (path_sets._square(100, 10, 20), path_sets.FILL), (path_sets._tri(130, 8), path_sets.STROKE, 5.0))
    local.paths["fill_rgba"] |= 0xFF
    _pool["local_grouped"] = PoolSet("local_grouped", local.with_groups(np.arange(4) % 2), (1.0, 0.0, 0.0, 1.0, 3.0, 2.0), 1.0)
    for name, seed in (("nested_a", 91), ("nested_b", 92)):
        _pool[name] = encode_ops(pm, extend_ops(seed, random_ops(seed, 110, extent=200.0)))
    return _pool


# ---- the query sets: a function of the viewport and the band (a caller picks within what it shows) -----------------------------------

def band_rows(h, row0, row1):
    return row0 * TILE, min(row1 * TILE, h)


def query_set(w, h, row0, row1):
    y0, y1 = band_rows(h, row0, row1)
    pts = np.array([(x + 0.5, y + 0.5) for y in range(y0 - 3, y1 + 3, 5) for x in range(-4, w + 4, 7)], np.float32)
    frame = (5, y0 + 3, min(w - 9, 75), min(y1 - y0 - 5, 37))   # (x0, y0, w, h): no edge on a tile boundary
    rects = [(x, y, x + 12.5, y + 9.25) for y in range(y0 - 4, y1, 19) for x in range(-6, w, 23)]
    rects += [(x + 0.5, y + 0.5, x + 0.5, y + 0.5) for y in range(y0 + 2, y1, 13) for x in range(3, w, 29)]   # points
    rects += [(0.0, float(y0), float(w), float(y1)), (w * 0.25, y0 + 8.0, w * 0.5, y1 - 8.0)]
    select = (w * 0.2, y0 + 6.0, w * 0.75, y1 - 5.0)
    return {"pts": pts, "frame": frame, "rects": np.array(rects, np.float32), "select": tuple(np.float32(v) for v in select)}


def n_flat_items(scene):
    return len(np_hit.flat_items(bytes(scene)))


class Answers:
    """np_hit / np_rect on scene bytes, cached by (scene, query set, flag)."""

    def __init__(self):
        self.cache = {}

    def get(self, kind, scene, view, skip):
        key = (kind, hash(scene.tobytes()), len(scene), view, skip)
        if key not in self.cache:
            q = query_set(*view)
            if kind == "hit_test":
                out = np_hit.hit_test(scene, q["pts"], skip_transparent=skip)
            elif kind == "hit_frame":
                x0, y0, w, h = q["frame"]
                centres = np.array([(x + 0.5, y + 0.5) for y in range(y0, y0 + h) for x in range(x0, x0 + w)], np.float32)
                top, cnt = np_hit.hit_test(scene, centres, skip_transparent=skip)
                out = (top.reshape(h, w), cnt.reshape(h, w))
            elif kind == "hit_rects":
                out = np_rect.hit_rects(scene, q["rects"], skip_transparent=skip)
            else:
                f = np_rect.item_flags(scene, np.array([q["select"]], np.float32), skip_transparent=skip)[:, 0]
                out = ((f & np_rect.TOUCHES) != 0, (f & np_rect.ENCLOSES) != 0)
            self.cache[key] = out
        return self.cache[key]


# ---- the model ------------------------------------------------------------------------------------------------------------------

class Model:
    def __init__(self, pm, pmo):
        self.pm, self.pmo = pm, pmo
        self.w = self.h = self.row0 = self.row1 = 0
        self.ps = None          # the resident paths (PathSet with its dash table), or None
        self.base = None        # (affine, scale) the set came with: what the scripted moves are relative to
        self.gmap = None        # the resident group map, or None
        self.paint = None       # (map at the repaint, tints, opacities), or None: the paths' own colours
        self.xform = None       # ("uniform", affine, scale) or ("table", map at the call, affines, width_scales)
        self.source = "none"    # "paths", "upload" or "none"
        self.upload = None
        self._scenes = {}
        self._frames = {}

    def copy(self):
        m = Model(self.pm, self.pmo)
        m.__dict__.update(self.__dict__)
        return m

    # -- what the caller may expect --
    def view(self):
        return (self.w, self.h, self.row0, self.row1)

    def painted_paths(self):
        if self.paint is None:
            return np_paint.painted(self.ps, None, None, None)
        return np_paint.painted(self.ps, *self.paint)

    def expected(self):
        """(scene bytes as a uint8 array, n_items, path_of_item or None), or None: no scene."""
        if self.source == "none":
            return None
        if self.source == "upload":
            return self.upload, n_flat_items(self.upload), None
        kind = self.xform[0]
        groups = None if kind == "uniform" else self.xform[1]
        aff = [self.xform[1]] if kind == "uniform" else self.xform[2]
        ws = [self.xform[2]] if kind == "uniform" else self.xform[3]
        ps = self.painted_paths()
        key = (ps.paths.tobytes(), ps.els.tobytes(), ps.dashes.tobytes(), ps.dash_values.tobytes(), None if groups is None else np.asarray(groups).tobytes(),
               np.asarray(aff, np.float64).tobytes(), np.asarray(ws, np.float32).tobytes())
        if key not in self._scenes:
            self._scenes[key] = np_groups.scene(ps, groups, aff, ws, lambda p, e, a: self.pmo.scene_from_paths(p, e, a, cap=96 << 20))
        return self._scenes[key]

    def frame(self, scene=None, view=None):
        """The oracle's frame over the band's rows."""
        scene = self.expected()[0] if scene is None else scene
        w, h, row0, row1 = view or self.view()
        key = (hash(scene.tobytes()), len(scene), w, h)
        if key not in self._frames:
            if len(self._frames) > 64:
                self._frames.clear()
            self._frames[key] = self.pmo.render(scene, w, h)
        y0, y1 = band_rows(h, row0, row1)
        return self._frames[key][y0:y1]

    def max_group(self):
        return int(self.gmap.max()) if self.gmap is not None and len(self.gmap) else 0

    # -- preconditions --
    def allowed(self, kind, variant):
        paths, scene = self.ps is not None, self.source != "none"
        if self.w == 0:
            return kind == "resize"
        if kind in ("flatten", "upload", "resize"):
            return True
        if kind == "band":
            return True
        if kind == "reflatten":
            return paths
        if kind == "groups":
            return paths and len(self.ps.paths) >= 2
        if kind == "reflatten_groups":
            ok = paths and self.gmap is not None
            return ok and (variant != "equal" or (self.source == "paths" and self.xform[0] == "uniform"))
        if kind == "repaint":
            return paths and self.gmap is not None and self.source == "paths"
        if kind == "invalid":
            return {"short_table": paths and self.gmap is not None, "opacity256": paths and self.gmap is not None, "groups_len": paths, "query_flag": True}[variant]
        if kind == "fail":
            return scene and (variant == "malformed" or paths)
        raise KeyError(kind)

    # -- state changes: returns "ok", "invalid" or "fail" --
    def apply(self, s: Step):
        k, a = s.kind, s.args
        if k == "flatten":
            self.ps, self.base = a["ps"], (tuple(a["affine"]), float(a["scale"]))
            self.gmap = None if a["ps"].groups is None else a["ps"].groups.copy()
            self.paint = None
            self.xform = ("uniform", tuple(a["affine"]), float(a["scale"]))
            self.source = "paths"
        elif k == "upload":
            self.source, self.upload = "upload", a["scene"]
        elif k == "reflatten":
            self.xform = ("uniform", tuple(a["affine"]), float(a["scale"]))
            self.source = "paths"
        elif k == "groups":
            self.gmap = np.asarray(a["map"], np.uint32).copy()
        elif k == "reflatten_groups":
            self.xform = ("table", self.gmap.copy(), np.asarray(a["affines"], np.float64), np.asarray(a["scales"], np.float32))
            self.source = "paths"
        elif k == "repaint":
            self.paint = (self.gmap.copy(), np.asarray(a["tints"], np.uint32), np.asarray(a["opacities"], np.uint32))
        elif k == "resize":
            self.w, self.h = a["w"], a["h"]
            self.row0, self.row1 = 0, (a["h"] + TILE - 1) // TILE
        elif k == "band":
            self.row0, self.row1 = a["row0"], a["row1"]
        elif k == "invalid":
            return "invalid"
        elif k == "fail":
            self.source = "none"
            return "fail"
        else:
            raise KeyError(k)
        return "ok"


# ---- drawing a script --------------------------------------------------------------------------------------------------------

def _shift(aff, dx, dy):
    return tuple(aff[:4]) + (aff[4] + dx, aff[5] + dy)


def _uniform_of(m: Model):
    """The uniform view the scripted tables are relative to: the one in force, or the set's own."""
    if m.source == "paths" and m.xform[0] == "uniform":
        return m.xform[1], m.xform[2]
    return m.base


def make_step(m: Model, kind, variant, rng, opt=None):
    """The concrete Step of (kind, variant) in the model's state.  Arguments come from small fixed sets, so that the expected scenes
    of different scripts coincide (the model caches them)."""
    pm = m.pm
    P = pool(pm)
    if kind == "flatten":
        s = P[variant]
        return Step(kind, variant, {"ps": s.ps, "affine": s.affine, "scale": s.scale})
    if kind == "upload":
        return Step(kind, variant, {"scene": P[variant]})
    if kind == "reflatten":
        aff, scale = m.base
        if variant == "subtile":      # less than a tile: the plan may be kept
            aff = _shift(aff, 3.25, -2.5)
        elif variant == "tiles":      # several tiles; "away": the upper tile rows are left empty, and filled again by the view after it
            opt = opt or ("far", "away")[int(rng.integers(0, 2))]
            aff = _shift(aff, 37.0, 21.0) if opt == "far" else _shift(aff, 0.0, 100.0)
        elif variant == "width":      # across a D14 level threshold ("wide") or the thin-line width ("thin"), in the view in force:
            opt = opt or ("thin", "wide")[int(rng.integers(0, 2))]   # entry counts, and with them plan_per, change under boxes that hardly move
            aff = _uniform_of(m)[0]
            scale = scale * (0.05 if opt == "thin" else 2.5)
        return Step(kind, variant, {"affine": aff, "scale": float(scale), **({"opt": opt} if opt else {})})
    if kind == "groups":
        n = len(m.ps.paths)
        maps = {"one": np.zeros(n, np.uint32), "interleaved": np.arange(n, dtype=np.uint32) % 2, "per_path": np.arange(n, dtype=np.uint32),
                "unused": (np.arange(n, dtype=np.uint32) % 2) * 3}
        return Step(kind, variant, {"map": maps[variant]})
    if kind == "reflatten_groups":
        aff, scale = _uniform_of(m)
        g = m.max_group() + 1 + int(rng.integers(0, 2))   # (a longer table is fine)
        affs, scales = np.tile(np.asarray(aff, np.float64), (g, 1)), np.full(g, scale, np.float32)
        who = int(rng.integers(0, m.max_group() + 1))
        who = who if (m.gmap == who).any() else int(m.gmap[0])
        if variant == "one_subtile":
            affs[who, 4:] += (3.5, 2.25)
        elif variant == "one_far":
            affs[who, 4:] += (45.0, -30.0)
        return Step(kind, variant, {"affines": affs, "scales": scales, "group": who})
    if kind == "repaint":
        g = m.max_group() + 1
        tints, opac = np.zeros(g, np.uint32), np.full(g, 255, np.uint32)
        who = int(rng.integers(0, g))
        who = who if (m.gmap == who).any() else int(m.gmap[0])
        if variant == "fade0":
            opac[who] = 0
        elif variant == "half":
            opac[:] = 128
        elif variant == "tint":
            tints[:] = [(0x3070B000 + 0x00402010 * i) & 0xFFFFFF00 | 0x90 for i in range(g)]
        return Step(kind, variant, {"tints": tints, "opacities": opac, "group": who})
    if kind == "resize":
        w, h = VIEWPORTS[variant]
        return Step(kind, variant, {"w": w, "h": h})
    if kind == "band":
        a, b = BAND_ROWS if variant == "rows" else (0, (m.h + TILE - 1) // TILE)
        return Step(kind, variant, {"row0": a, "row1": b})
    if kind == "invalid":
        return Step(kind, variant)
    if kind == "fail":
        if variant == "cap":
            aff, scale = m.base
            return Step(kind, variant, {"affine": aff, "scale": float(scale)})
        return Step(kind, variant, {"scene": P["nested_a"]})
    raise KeyError(kind)


def total_cmds(pmo, scene, w, h):
    p = pmo.Ptcl(scene, w, h)
    try:
        return p.total_cmds()[0]
    finally:
        p.close()


def blind(before: Model, after: Model, step: Step, answers: Answers, inflight=()):
    """Why the state change `step` (before -> after) could not be seen by what follows it, or None.  A replacement must change the
    oracle's frame of the band in force and an answer of at least one query kind of the query set in force; with an `inflight`
    observation in front of it (`inflight`: the skip flags of the observations pending), the frame and, under that observation's own
    flag, an answer at the view of that observation; the steps of SAME_BYTES must leave the model's bytes as they are."""
    b, a = before.expected(), after.expected()
    if (step.kind, step.variant) in SAME_BYTES:
        same = (b is None and a is None) or (b is not None and a is not None and np.array_equal(b[0], a[0]))
        return None if same and before.view() == after.view() else "the bytes changed"
    if b is None or a is None:
        return None if (b is None) != (a is None) else "no scene before and after"

    def differs(view_b, view_a, skips=(False, True)):
        fb, fa = before.frame(b[0], view_b), after.frame(a[0], view_a)
        if fb.shape == fa.shape and np.array_equal(fb, fa):
            return "the frame of the band in force does not change"
        for kind in QUERY_OBS:
            for skip in skips:
                qb, qa = answers.get(kind, b[0], view_b, skip), answers.get(kind, a[0], view_a, skip)
                if any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(qb, qa)):
                    return None
        return "no query of the query set changes an answer"

    why = differs(before.view(), after.view())
    for skip in inflight:   # (frames and queries in flight keep the view and the flag they were enqueued with)
        if why is None:
            why = differs(before.view(), before.view(), (skip,))
            why = why and "in flight: " + why
    if why is None and step.kind == "repaint":
        pmo = after.pmo
        if step.variant == "fade0":     # the group's items are on top somewhere in the band
            top = answers.get("hit_test", b[0], before.view(), False)[0]
            hit = top[top != np_hit.HIT_NONE]
            if not (before.gmap[b[2][hit]] == step.args["group"]).any():
                why = "the faded group is on top nowhere"
        elif step.variant == "solid":   # the Solid rule shortens lists
            if not total_cmds(pmo, a[0], after.w, after.h) < total_cmds(pmo, b[0], before.w, before.h):
                why = "no tile list gets shorter"
    return why


def coverage_item(m: Model):
    """(index, stale) of the Fill item pm_fill_coverage is asked for: the first one whose coverage over the viewport is another
    with the paths' own colours than with the painted ones (what the host's colour-stale copy of the records would give: stale is
    True), or else the first Fill; -1 where the scene has none (or there is no scene)."""
    ex = m.expected()
    if ex is None:
        return -1, False
    sc = bytes(ex[0])
    fills = [i for i, (at, _) in enumerate(np_hit.flat_items(sc)) if struct.unpack_from("<I", sc, at)[0] & 0xFFFF == np_hit.FILL]
    if not fills:
        return -1, False
    if m.source == "paths" and m.paint is not None:
        own = m.copy()
        own.paint = None
        for i in fills[:40]:
            if not np.array_equal(m.pmo.fill_coverage(ex[0], i, m.w, m.h), m.pmo.fill_coverage(own.expected()[0], i, m.w, m.h)):
                return i, True
    return fills[0], False


def _obs_step(m: Model, kind, rng):
    skip, counts = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if kind in QUERY_OBS:
        return Step(kind, "", {"skip": skip, "counts": counts})
    if kind == "burst":
        return Step(kind, "", {"n": int(rng.integers(2, 5))})
    if kind == "inflight":
        return Step(kind, "", {"skip": skip})
    if kind == "fill_coverage":
        return Step(kind, "", {"item": coverage_item(m)[0]})
    return Step(kind)


def generate(pm, pmo, seed, n_changes=8, answers=None):
    """The script of `seed`: resize, a first scene, then n_changes state changes, each followed by a block of observations -- a frame
    kind and a query kind at least, in any order, sometimes exactly three lone frames (the third-frame re-plan), an `inflight` last."""
    rng = np.random.default_rng([seed, 0xC0DE])
    answers = answers or Answers()
    m = Model(pm, pmo)
    script = []
    pending_inflight = ()   # the skip flags of the `inflight` observations the next state change straddles
    after_fail = False

    def block():
        nonlocal pending_inflight
        if m.source == "none":   # one operation the "no scene" state must refuse
            return [_obs_step(m, OBS[int(rng.integers(0, len(OBS)))], rng)]
        first = OBS[int(rng.integers(0, len(OBS)))]
        kinds = [first]
        if rng.random() < 0.45:
            kinds += ["lone", "lone", "lone"] if first not in FRAME_OBS + ("capture_ptcl", "fill_coverage") else (["lone", "lone"] if first == "lone" else [])
        if not any(k in FRAME_OBS or k == "capture_ptcl" for k in kinds):
            kinds.append(("lone", "burst")[int(rng.integers(0, 2))])
        if not any(k in QUERY_OBS or k == "inflight" for k in kinds):
            kinds.append(QUERY_OBS[int(rng.integers(0, 4))])
        if "inflight" not in kinds and rng.random() < 0.25:
            kinds.append("inflight")
        if "inflight" in kinds:   # last: the next state change straddles it
            kinds = [k for k in kinds if k != "inflight"] + ["inflight"]
            if kinds[0] != first:   # (drawn first: it stays directly behind the change, something else is in flight at the end)
                kinds = ["inflight"] + kinds
        steps = [_obs_step(m, k, rng) for k in kinds]
        pending_inflight = tuple(s.args["skip"] for s in steps if s.kind == "inflight") if kinds[-1] == "inflight" else ()
        return steps

    def change(step):
        nonlocal after_fail
        m.apply(step)
        script.append(step)
        after_fail = step.kind == "fail"
        script.extend(block())

    change(make_step(m, "resize", ("even", "odd")[int(rng.integers(0, 2))], rng))
    first = ("flatten", "upload")[int(rng.random() < 0.25)]
    change(make_step(m, first, VARIANTS[first][int(rng.integers(0, len(VARIANTS[first])))], rng))
    done = 0
    while done < n_changes:
        ops = RECOVERIES if after_fail else (STRADDLERS + ("fail",) if pending_inflight else STATE_OPS)
        ops = [k for k in ops for _ in range(WEIGHTS.get(k, 1))]
        for _ in range(200):
            kind = ops[int(rng.integers(0, len(ops)))]
            variant = VARIANTS[kind][int(rng.integers(0, len(VARIANTS[kind])))]
            if not m.allowed(kind, variant) or (pending_inflight and (kind, variant) in SAME_BYTES):
                continue
            step = make_step(m, kind, variant, rng)
            after = m.copy()
            after.apply(step)
            if blind(m, after, step, answers, pending_inflight) is None:
                break
        else:
            raise RuntimeError(f"seed {seed}: no state change that can be seen after {script[-1]}")
        change(step)
        done += 1
    if after_fail:   # a script ends with a scene
        change(make_step(m, "reflatten" if m.ps is not None else "upload", "base" if m.ps is not None else "nested_b", rng))
    return script


def scripted(pm, pmo, names, seed=0, answers=None):
    """A script from names: "kind:variant[:option]" for state changes, "kind" for observations ("lone*4": four of them).  Every
    state change must be allowed where it stands and must not be blind."""
    rng = np.random.default_rng([seed, 0x5C21])
    answers = answers or Answers()
    m = Model(pm, pmo)
    script, inflight = [], ()
    for name in names:
        kind, _, rest = name.partition(":")
        if kind.partition("*")[0] in OBS:
            kind, _, times = kind.partition("*")
            script += [_obs_step(m, kind, rng) for _ in range(int(times or 1))]
            inflight = tuple(s.args["skip"] for s in script[-int(times or 1):]) if kind == "inflight" else ()
            continue
        variant, _, opt = rest.partition(":")
        assert m.allowed(kind, variant), name
        for _ in range(20):   # (the group a table or a paint singles out is drawn)
            step = make_step(m, kind, variant, rng, opt or None)
            after = m.copy()
            after.apply(step)
            why = m.w and blind(m, after, step, answers, inflight)
            if not why:
                break
        assert not why, (name, why)
        m.apply(step)
        script.append(step)
        inflight = ()
    return script


# ---- walking a script on a Renderer ----------------------------------------------------------------------------------------------

class _Device:
    """Buffers for the asynchronous calls: torch tensors on the GPU; under the CPU emulation device memory is host memory and the
    buffers are numpy's, handed to the C ABI directly (as tests/test_hit_rect.py does)."""

    def __init__(self, pm):
        self.pm = pm
        self.emu = os.environ.get("PM_TEST_EMU") == "1"
        self.side = None
        if not self.emu:
            import torch

            self.torch = torch
            self.side = torch.cuda.Stream()

    def on_side(self):
        import contextlib

        return contextlib.nullcontext() if self.emu else self.torch.cuda.stream(self.side)

    def full(self, shape, value, dtype=np.uint32):
        if self.emu:
            return np.full(shape, value, dtype)
        t = {np.uint32: self.torch.int32, np.uint8: self.torch.uint8}[dtype]
        return self.torch.full(tuple(np.atleast_1d(shape)), int(value), dtype=t, device="cuda:0")

    def put(self, a):
        return a if self.emu else self.torch.from_numpy(a).cuda()

    def host(self, t, dtype=np.uint32):
        return t if self.emu else t.cpu().numpy().view(dtype)

    def filled(self):
        """Waits for torch's current stream alone (the fills of buffers just made), not for the context's frames."""
        if not self.emu:
            self.torch.cuda.current_stream().synchronize()

    def wait(self):
        if not self.emu:
            self.side.synchronize()


class Runner:
    """run() walks `script` on Renderer `r`; every check raises AssertionError naming seed, step index and operation."""

    def __init__(self, pm, pmo, r, script, seed, answers=None):
        self.pm, self.pmo, self.r, self.script, self.seed = pm, pmo, r, script, seed
        self.lib = pm._lib.load()
        self.m = Model(pm, pmo)
        self.answers = answers or Answers()
        self.dev = _Device(pm)
        self.pending = []       # observations in flight: (step index, scene, view, buffers)
        self.executed = 0
        self.epoch_fed = 0      # plans_fed_back when the plan of the (scene, viewport, band) in force began
        self.epoch_mark = None  # (binning_plans, plans_fed_back) in front of a state change no frame has followed yet
        self.plan_mark = None   # (binning_plans, plans_fed_back) in front of a repaint / invalid step with a frame on its plan
        self.frames_on_plan = 0
        self.where = ""

    # -- failures name the step --
    def check(self, ok, what):
        if not ok:
            raise AssertionError(f"seed {self.seed}, step {self.where}: {what}")

    def refused(self, fn, what, status=INVALID):
        try:
            fn()
        except self.pm.PietMetalError as e:
            self.check(e.status == status, f"{what}: status {e.status}, not {status}")
            return
        self.check(False, f"{what} was not refused")

    # -- state changes --
    def change(self, s: Step):
        r, m, a = self.r, self.m, s.args
        info = r.binning_plan_info()
        plans = (r.scene_timings()["binning_plans"], info["plans_fed_back"], info["fed_back"])
        before = m.expected()
        got = None
        k = s.kind
        if k == "flatten":
            got = r.flatten_and_encode(a["ps"], a["affine"], a["scale"])
        elif k == "upload":
            r.set_scene_bytes(a["scene"])
        elif k == "reflatten":
            got = r.reflatten(a["affine"], a["scale"])
        elif k == "groups":
            r.set_path_groups(a["map"])
        elif k == "reflatten_groups":
            got = r.reflatten_groups(a["affines"], a["scales"])
        elif k == "repaint":
            r.repaint_groups(a["opacities"], a["tints"])
            self.check(r.scene_timings()["scene_index_ms"] == 0, "a repaint rebuilt the scene index")
        elif k == "resize":
            r.resize(a["w"], a["h"])
        elif k == "band":
            r.set_band(a["row0"], a["row1"])
        elif k == "invalid":
            self.invalid(s)
        elif k == "fail":
            self.fail(s)
        m.apply(s)
        want = m.expected()
        scene = r.download_scene()
        if want is None:
            self.check(len(scene) == 0 and r.stats()["n_items"] == 0, f"a failed replacement left {len(scene)} bytes, {r.stats()['n_items']} items")
            self.refused(r.render, "render without a scene")
            if m.ps is not None and m.gmap is not None:   # (pm_repaint_groups: "the last replacement failed")
                self.refused(lambda: r.repaint_groups(np.full(m.max_group() + 1, 255, np.uint32)), "repaint_groups without a scene")
        else:
            self.check(len(scene) == len(want[0]) and np.array_equal(scene, want[0]),
                       f"the resident scene is not the model's ({len(scene)} bytes, expected {len(want[0])}; first difference at "
                       f"{np.flatnonzero(scene[:len(want[0])] != want[0][:len(scene)])[:4].tolist()})")
            self.check(r.stats()["n_items"] == want[1], f"{r.stats()['n_items']} items, expected {want[1]}")
            if got is not None:
                self.check(got == (len(want[0]), want[1]), f"returned {got}, expected {(len(want[0]), want[1])}")
        if (k, s.variant) in SAME_BYTES:
            self.check((before is None and want is None) or np.array_equal(before[0], want[0]), "the model's bytes changed")
        # frames and queries enqueued before this change read the scene that was current then
        self.flush()
        if k in ("repaint", "invalid", "groups"):
            # The plan in force stays.  The call itself makes no plan: asserted here.  Plans are made by frames (EnsureArena), so
            # whether the NEXT frame makes one is asserted behind it (frames_done) -- not as "unchanged", because that frame may be
            # the plan's third, whose report remakes the plan whatever stood in between: binning_plans may move there by exactly
            # what plans_fed_back moves by.  Without a frame on the plan yet, the next frame makes the scene's first plan.
            self.check(r.scene_timings()["binning_plans"] == plans[0], f"{k} made a binning plan: {plans[0]} -> {r.scene_timings()['binning_plans']}")
            self.plan_mark = plans if self.frames_on_plan else None
        else:   # another scene, viewport or band: its first frame says whether the plan in force was kept (frames_done)
            self.plan_mark = None
            self.frames_on_plan = 0
            self.epoch_mark = plans

    def invalid(self, s: Step):
        r, m, pm = self.r, self.m, self.pm
        if s.variant == "short_table":      # a table shorter than the map reaches (no row at all for a map of one group)
            g = m.max_group()
            self.refused(lambda: r.reflatten_groups(np.tile(np.asarray(m.base[0], np.float64), (g, 1)).reshape(g, 6)), "a short table")
            self.refused(lambda: r.repaint_groups(np.full(g, 255, np.uint32)), "a short paint table")
        elif s.variant == "opacity256":
            o = np.full(m.max_group() + 1, 255, np.uint32)
            o[-1] = 256
            self.refused(lambda: r.repaint_groups(o), "opacity 256")
        elif s.variant == "groups_len":
            self.refused(lambda: r.set_path_groups(np.zeros(len(m.ps.paths) + 1, np.uint32)), "a map of another length")
        else:                               # a query with unknown flag bits
            xy, top = np.zeros((1, 2), np.float32), np.zeros(1, np.uint32)
            st = self.lib.pm_hit_test(r._h, xy.ctypes.data, 1, 2, top.ctypes.data, None)
            self.check(st == INVALID, f"pm_hit_test with flag bit 1: status {st}")
            rc = np.zeros(4, np.float32)
            st = self.lib.pm_hit_rects(r._h, rc.ctypes.data, 1, 4, top.ctypes.data, None)
            self.check(st == INVALID, f"pm_hit_rects with flag bit 2: status {st}")

    def fail(self, s: Step):
        r, m, a = self.r, self.m, s.args
        if s.variant == "cap":   # PM_FLATTEN_SCENE_CAP one entry short (tests/test_stroke_gpu.py)
            after = m.copy()
            after.apply(Step("reflatten", "base", a))
            need = len(after.expected()[0])
            os.environ["PM_FLATTEN_SCENE_CAP"] = str(need - 8)
            try:
                nbytes, n_items = C.c_size_t(0), C.c_uint32(0)
                st = self.lib.pm_reflatten(r._h, (C.c_double * 6)(*a["affine"]), a["scale"], C.byref(nbytes), C.byref(n_items))
            finally:
                del os.environ["PM_FLATTEN_SCENE_CAP"]
            self.check((st, nbytes.value) == (CAPACITY, need), f"one entry short: status {st}, needs {nbytes.value}, expected {(CAPACITY, need)}")
        else:                    # a malformed upload (tests/test_gpu_parity.py)
            bad = a["scene"].copy()
            bad[0:4] = np.frombuffer(struct.pack("<I", 0x7FFFFFFF), np.uint8)
            try:
                r.set_scene_bytes(bad)
            except self.pm.PietMetalError:
                return
            self.check(False, "a malformed upload was accepted")

    # -- observations --
    def compare_frame(self, got, scene, view, what):
        want = self.m.frame(scene, view)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad = (got != want).any(axis=2) if got.shape == want.shape else None
            tiles = sorted({(int(y) // TILE + view[2], int(x) // TILE) for y, x in zip(*np.nonzero(bad))}) if bad is not None else []
            self.check(False, f"{what}: {len(tiles)} wrong tiles ({int(bad.sum()) if bad is not None else got.shape} pixels) at {view}, first {tiles[:4]}, "
                              f"plan {self.r.binning_plan_info()}")

    def frames_done(self, n):
        r = self.r
        self.frames_on_plan += n
        info = r.binning_plan_info()
        if self.epoch_mark is not None:
            # a plan of its own: the count of plans made from a report starts again; a plan kept over a view change (EnsureArena)
            # is the same plan, and its frames' report is used once at the most all the same
            if r.scene_timings()["binning_plans"] > self.epoch_mark[0]:
                self.epoch_fed = self.epoch_mark[1]
            else:   # (pm_binning_plan_info: a kept plan that was made with the frames' report still is one)
                self.check(info["fed_back"] or not self.epoch_mark[2], f"the plan kept over the state change forgot that it was made with the frames' report: {info}")
            self.epoch_mark = None
        fed = info["plans_fed_back"] - self.epoch_fed
        self.check(fed <= 1, f"{fed} plans remade from the frames' report on one scene, viewport and band: {info}")
        if self.plan_mark is not None:
            plans = r.scene_timings()["binning_plans"]
            self.check(plans - self.plan_mark[0] == info["plans_fed_back"] - self.plan_mark[1],
                       f"a repaint or an invalid call made a plan: {self.plan_mark[0]} -> {plans} plans, {self.plan_mark[1]} -> {info['plans_fed_back']} from a report")
            self.plan_mark = None

    def query(self, kind, skip, counts):
        """(answers as a tuple of arrays) through the synchronous call."""
        r, q = self.r, query_set(*self.m.view())
        if kind == "hit_test":
            out = r.hit_test(q["pts"], skip_transparent=skip, counts=counts)
        elif kind == "hit_frame":
            out = r.hit_frame(*q["frame"], skip_transparent=skip, counts=counts)
        elif kind == "hit_rects":
            out = r.hit_rects(q["rects"], skip_transparent=skip, counts=counts)
        else:
            return r.select_rect(*q["select"], skip_transparent=skip)
        return out if counts else (out,)

    def enqueue(self, skip):
        """Two frames into buffers of their own on the context's stream and the four queries on a side stream; nothing waited for."""
        r, m, d, lib = self.r, self.m, self.dev, self.lib
        q = query_set(*m.view())
        y0, y1 = band_rows(m.h, m.row0, m.row1)
        flags = self.pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0
        n_items = m.expected()[1]
        bufs = {"frames": [d.full((y1 - y0, m.w, 4), 0, np.uint8) for _ in range(2)]}
        d.filled()   # (the fills ran on torch's stream, the frames run on the context's: nothing else orders them)
        with d.on_side():
            x0, fy, fw, fh = q["frame"]
            pts, rects = d.put(q["pts"]), d.put(q["rects"])
            bufs.update(pts=pts, rects=rects, hit_test=[d.full(len(q["pts"]), UNTOUCHED) for _ in range(2)], hit_frame=[d.full((fh, fw), UNTOUCHED) for _ in range(2)],
                        hit_rects=[d.full(len(q["rects"]), UNTOUCHED) for _ in range(2)], select_rect=d.full(n_items + 3, UNTOUCHED))
        for t in bufs["frames"]:
            if d.emu:
                self.pm._lib.check(lib.pm_render_to(r._h, t.ctypes.data, m.w * 4, None), "pm_render_to")
            else:
                r.render_to(t, None)
        if d.emu:
            chk = self.pm._lib.check
            chk(lib.pm_hit_test_device(r._h, pts.ctypes.data, len(pts), flags, bufs["hit_test"][0].ctypes.data, bufs["hit_test"][1].ctypes.data, None), "pm_hit_test_device")
            chk(lib.pm_hit_frame_device(r._h, x0, fy, fw, fh, flags, bufs["hit_frame"][0].ctypes.data, bufs["hit_frame"][1].ctypes.data, fw, None), "pm_hit_frame_device")
            chk(lib.pm_hit_rects_device(r._h, rects.ctypes.data, len(rects), flags, bufs["hit_rects"][0].ctypes.data, bufs["hit_rects"][1].ctypes.data, None), "pm_hit_rects_device")
            rect = np.array(q["select"], np.float32)
            chk(lib.pm_select_rect_device(r._h, rect.ctypes.data, flags, bufs["select_rect"].ctypes.data, n_items + 3, None), "pm_select_rect_device")
        else:
            r.hit_test_tensor(pts, *bufs["hit_test"], stream=d.side, skip_transparent=skip)
            r.hit_frame_tensor(*bufs["hit_frame"], x0=x0, y0=fy, stream=d.side, skip_transparent=skip)
            r.hit_rects_tensor(rects, *bufs["hit_rects"], stream=d.side, skip_transparent=skip)
            r.select_rect_tensor(*[float(v) for v in q["select"]], bufs["select_rect"], stream=d.side, skip_transparent=skip)
        self.frames_done(2)   # (host bookkeeping only, nothing waited for: these two frames may be the first of their plan)
        return bufs

    def flush(self):
        """Compare what was in flight with the scene that was current when it was enqueued."""
        if not self.pending:
            return
        self.r.sync()
        self.dev.wait()
        d = self.dev
        for index, scene, n_items, view, skip, bufs in self.pending:
            what = f"in flight since step {index}"
            for k, t in enumerate(bufs["frames"]):
                self.compare_frame(d.host(t, np.uint8), scene, view, f"{what}, frame {k}")
            for kind in ("hit_test", "hit_frame", "hit_rects"):
                want = self.answers.get(kind, scene, view, skip)
                for got, w, name in zip(bufs[kind], want, ("top_item", "n_hit")):
                    self.check(np.array_equal(d.host(got), w), f"{what}: {kind} {name} is not the answer for the scene current at the call")
            touched, enclosed = self.answers.get("select_rect", scene, view, skip)
            words = d.host(bufs["select_rect"])
            self.check(np.array_equal(words[:n_items], touched * np_rect.TOUCHES + enclosed * np_rect.ENCLOSES) and (words[n_items:] == UNTOUCHED).all(),
                       f"{what}: select_rect is not the answer for the scene current at the call")
        self.pending = []

    def observe(self, index, s: Step):
        r, m, a = self.r, self.m, s.args
        k = s.kind
        ex = m.expected()
        if ex is None:   # every operation is refused
            calls = {"lone": r.render, "burst": r.render, "capture_ptcl": r.render, "inflight": r.render,
                     "item_paths": r.item_paths, "fill_coverage": lambda: r.fill_coverage(0)}
            fn = calls.get(k) or (lambda: self.query(k, a["skip"], a["counts"]))
            self.refused(fn, f"{k} without a scene")
            self.check(r.stats()["n_items"] == 0, "items without a scene")
            return
        scene, n_items, paths = ex
        if k == "lone":
            r.render()
            self.check(r.stats()["overflow"] == 0, "the command-list arena of a lone frame overflowed: the plan does not fit the scene")
            r.sync()
            self.compare_frame(r.read_pixels(), scene, m.view(), "lone frame")
            self.frames_done(1)
        elif k == "burst":
            for _ in range(a["n"]):
                r.render()
            self.compare_frame(r.read_pixels(), scene, m.view(), f"burst of {a['n']}")
            self.frames_done(a["n"])
        elif k == "inflight":
            self.pending.append((index, scene, n_items, m.view(), a["skip"], self.enqueue(a["skip"])))
        elif k in QUERY_OBS:
            want = self.answers.get(k, scene, m.view(), a["skip"])
            got = self.query(k, a["skip"], a["counts"])
            for g, w, name in zip(got, want, ("top_item / touched", "n_hit / enclosed")):
                self.check(g.shape == w.shape and np.array_equal(g, w), f"{k} (skip {a['skip']}): {name} differs at {np.argwhere(g != w)[:4].tolist() if g.shape == w.shape else g.shape}")
        elif k == "item_paths":
            if paths is None:
                self.refused(r.item_paths, "item_paths of an uploaded scene")
            else:
                self.check(np.array_equal(r.item_paths(), paths), "item_paths differ")
        elif k == "fill_coverage":
            if a["item"] < 0:
                self.refused(lambda: r.fill_coverage(0), "fill_coverage of an item that is no Fill")
            else:
                y0, y1 = band_rows(m.h, m.row0, m.row1)
                want = self.pmo.fill_coverage(scene, a["item"], m.w, m.h)[y0:y1]
                self.check(np.array_equal(r.fill_coverage(a["item"]), want), f"fill_coverage of item {a['item']} differs")
                self.check(np.array_equal(r.download_scene(), scene), "fill_coverage did not put the scene back")
            self.plan_mark = None   # (a validation call: it renders the item alone and plans for that)
        elif k == "capture_ptcl":
            r.render()
            r.sync()
            self.compare_frame(r.read_pixels(), scene, m.view(), "frame in front of the capture")
            self.frames_done(1)
            P = self.pmo.Ptcl(scene, m.w, m.h)
            try:
                counts, solid, cmds = r.capture_ptcl(1024)
                for ty in range(m.row0, min(m.row1, P.tiles_y)):
                    for tx in range(P.tiles_x):
                        oc = P.cmds(tx, ty)
                        y = ty - m.row0
                        ok = counts[y, tx] == len(oc) and solid[y, tx] == P.solid(tx, ty) and np.array_equal(cmds[y, tx, : len(oc)], oc)
                        self.check(ok, f"tile ({tx}, {ty}) list differs from the oracle's")
            finally:
                P.close()
        else:
            raise KeyError(k)

    def run(self):
        for index, s in enumerate(self.script):
            self.where = f"{index} ({s!r})"
            if s.kind in STATE_OPS:
                self.change(s)
            else:
                self.observe(index, s)
            self.executed += 1
        self.where = "end"
        self.flush()
        assert self.executed == len(self.script), f"seed {self.seed}: {self.executed} of {len(self.script)} steps executed"
