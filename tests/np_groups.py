"""Decision D16, the expected bytes of a grouped re-flatten (test infrastructure): path p is flattened under the
affine and width_scale of its own group.  The scene is built by SPLICING scenes the two existing restatements already define --
nothing of the flatten rules is written again here:

  1. every path alone, as the one-path scene of `scene_from_paths` (oracle/pmo.py or tests/np_scene.py: the caller chooses, both
     must give the same splice) under its group's affine, its stroke width multiplied by its group's width_scale;
  2. boxes, item records and points concatenated in path order;
  3. word 4 (points_ix) of every Fill and poly-line record rebased; compound separators are item-relative and stay;
  4. np_stroke.apply / np_dash.apply (decisions D14, D15) with specs built per path from that path's own width_scale.

A table whose groups are all equal must give the whole set's scene: tests/test_groups_cpu.py proves that of this helper before
any device scene is judged by it."""
import struct

import numpy as np

import np_dash
import np_stroke

ITEM, BOX, HEAD = 32, 8, 8


def default_width_scales(affines):
    """sqrt|det| per row, in binary64, rounded to f32 (what Renderer.reflatten_groups uses when none are given)."""
    a = np.asarray(affines, np.float64).reshape(-1, 6)
    return np.sqrt(np.abs(a[:, 0] * a[:, 3] - a[:, 1] * a[:, 2])).astype(np.float32)


def _one_path(ps, p):
    """(path record rebased to its own elements and without style bits, its elements)"""
    row = ps.paths[p : p + 1].copy()
    b, e = int(row["el_begin"][0]), int(row["el_end"][0])
    row["el_begin"], row["el_end"] = 0, e - b
    return np_stroke.unstyled(row), ps.els[b:e]


def _scaled(paths, width_scale):
    """width * (scale as f32) in f32 (src/lib.rs:320), as oracle/pmo.scaled_paths"""
    p = paths.copy()
    p["stroke_width"] = (p["stroke_width"].astype(np.float32) * np.float32(width_scale)).astype(np.float32)
    return p


def poly_scene(ps, groups, affines, width_scales, scene_from_paths):
    """Steps 1-3: the poly-line scene (no outlines, no dashes).  scene_from_paths(paths, els, affine) -> scene bytes (or an array,
    or a tuple whose first entry is one).  Returns (bytes, n_items, path_of_item)."""
    groups = np.zeros(len(ps.paths), np.uint32) if groups is None else np.asarray(groups)
    boxes, items, points, path_of_item = [], [], [], []
    for p in range(len(ps.paths)):
        g = int(groups[p])
        row, els = _one_path(ps, p)
        sc = scene_from_paths(_scaled(row, width_scales[g]), els, tuple(float(v) for v in affines[g]))
        sc = sc[0] if isinstance(sc, tuple) else sc
        sc = bytes(np.asarray(sc, np.uint8)) if not isinstance(sc, (bytes, bytearray)) else bytes(sc)
        n, items_ix = struct.unpack_from("<II", sc, 0)
        assert items_ix == HEAD + BOX * n
        boxes.append(sc[HEAD:items_ix])
        items.append((sc[items_ix : items_ix + ITEM * n], items_ix + ITEM * n))
        points.append(sc[items_ix + ITEM * n :])
        path_of_item += [p] * n
    n_items = len(path_of_item)
    points_start = HEAD + (BOX + ITEM) * n_items
    out = bytearray(struct.pack("<II", n_items, HEAD + BOX * n_items) + b"".join(boxes))
    at = points_start
    for (recs, old_points_start), pts in zip(items, points):
        recs = bytearray(recs)
        for i in range(len(recs) // ITEM):
            tag, pix = struct.unpack_from("<I", recs, ITEM * i)[0], struct.unpack_from("<I", recs, ITEM * i + 16)[0]
            assert tag in (3, 4), "the flatten stage makes Fill and poly-line items only"
            struct.pack_into("<I", recs, ITEM * i + 16, pix - old_points_start + at)
        out += recs
        at += len(pts)
    out += b"".join(points)
    assert len(out) == at
    return bytes(out), n_items, np.array(path_of_item, np.uint32)


def specs(ps, groups, width_scales):
    """Step 4's specs, per item: np_dash.specs_from_pathset of every path alone under its own width_scale (5-tuples), or, for a
    set without a dash table, np_stroke.specs_from_paths (4-tuples)."""
    groups = np.zeros(len(ps.paths), np.uint32) if groups is None else np.asarray(groups)
    if len(ps.dashes) == 0:
        return np_stroke.specs_from_paths(ps.paths, ps.els), False
    table = {int(d["path"]): d for d in ps.dashes}
    out = []
    for p in range(len(ps.paths)):
        one = type(ps)(ps.paths[p : p + 1], ps.els)  # (el_begin / el_end still index the whole element array)
        if p in table:
            d = table[p]
            vals = ps.dash_values[int(d["first"]) : int(d["first"]) + int(d["count"])]
            one = type(ps)(ps.paths[p : p + 1], ps.els, np.array([(0, 0, len(vals), d["offset"])], ps.DASH_DTYPE), vals)
        out += np_dash.specs_from_pathset(one, float(np.float32(width_scales[int(groups[p])])))
    return out, True


def scene(ps, groups, affines, width_scales, scene_from_paths):
    """The D16 scene of path set ps (styles and dash table included) under group map `groups` (None: one group) and the table
    {affines[g], width_scales[g]}.  Returns (scene as a uint8 array, n_items, path_of_item)."""
    affines = np.asarray(affines, np.float64).reshape(-1, 6)
    width_scales = default_width_scales(affines) if width_scales is None else np.asarray(width_scales, np.float32).reshape(-1)
    assert len(width_scales) == len(affines)
    sc, n_items, path_of_item = poly_scene(ps, groups, affines, width_scales, scene_from_paths)
    sp, dashed = specs(ps, groups, width_scales)
    if any(s is not None for s in sp):
        sc = np_dash.apply(sc, sp) if dashed else np_stroke.apply(sc, sp)
    return np.frombuffer(sc, np.uint8), n_items, path_of_item
