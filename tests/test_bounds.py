"""Bounds queries, pm_item_bounds / pm_union_bounds and their device calls (decision D22): where every item is and how big, and
the union of the boxes of a selection or of every group, with its counts.

The bar everywhere: records EQUAL to tests/np_bounds.py as bytes -- the sign of a zero included --, through the host and the device
calls, with and without PM_HIT_SKIP_TRANSPARENT.  tests/bounds_cases.py builds the scenes, the labels and the selection words.

-m gpu: the hand-derived boxes; every case scene's item records and its unions under every labelling and mask; selection words
from pm_select_rect_device into pm_union_bounds_device with no read-back, torch tensors on a caller's stream; D22 against the
device's own pm_select_rect; group_bounds after reflatten_groups and after a styled and dashed flatten; capacity and every
argument error; scenes without items; frames in flight and a scene replacement between two queries; the CLI.
CPU: np_bounds against the hand-derived boxes; D22 against np_rect's "encloses"; the header; the cases are what they claim; the
-m gpu part against the wave64 emulation of the kernels; the compiler's listing."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bounds_cases as bc  # noqa: E402
import hit_structure as hs  # noqa: E402
import np_bounds  # noqa: E402
import np_hit  # noqa: E402
import np_rect  # noqa: E402

F32 = np.float32
REC = np_bounds.LABEL_BOUNDS
UNTOUCHED = 0x7EADBEEF
INVALID, CAPACITY = -1, -4
# known boxes, scenes, selection composition, D22 <=> D19, groups (2), argument rules, no items, ordering (2), CLI
N_GPU_TESTS = 1 + len(bc.SCENES) + 1 + 1 + 2 + 1 + 1 + 2 + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def skip_flag(pm, skip):
    return pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0


def to_device(a):
    """A numpy array of 32-bit words on the device (under the emulation device memory is host memory)."""
    if a is None or _emulated():
        return None if a is None else np.ascontiguousarray(a)
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def host_view(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def device_item_bounds(pm, r, n_rows, skip=False, stream=None):
    """pm_item_bounds_device into n_rows records filled with NaN, not waited for: float64 [n_rows, 4] of either kind."""
    if _emulated():
        out = np.full((n_rows, 4), np.nan, np.float64)
        pm._lib.check(pm._lib.load().pm_item_bounds_device(r._h, skip_flag(pm, skip), out.ctypes.data, n_rows, None), "pm_item_bounds_device")
        return out
    import torch

    out = torch.full((n_rows, 4), float("nan"), dtype=torch.float64, device="cuda")
    r.item_bounds_tensor(out, stream=stream, skip_transparent=skip)
    return out


def device_union(pm, r, n_labels, labels=None, words=None, mask=3, skip=False, stream=None, pad=0):
    """pm_union_bounds_device into n_labels + pad records filled with UNTOUCHED, not waited for: (int32 [n_labels + pad, 10], keep-alive).
    labels / words: None, numpy arrays (copied to the device) or device words as they are."""
    lab = to_device(labels) if labels is None or isinstance(labels, np.ndarray) else labels
    w = to_device(words) if words is None or isinstance(words, np.ndarray) else words
    if _emulated():
        out = np.full((n_labels + pad, 10), UNTOUCHED, np.int32)
        pm._lib.check(pm._lib.load().pm_union_bounds_device(r._h, skip_flag(pm, skip), w.ctypes.data if w is not None else None, w.size if w is not None else 0,
                                                            mask if w is not None else 0, lab.ctypes.data if lab is not None else None,
                                                            lab.size if lab is not None else 0, n_labels, out.ctypes.data, None), "pm_union_bounds_device")
        return out, (lab, w)
    import torch

    out = torch.full((n_labels + pad, 10), UNTOUCHED, dtype=torch.int32, device="cuda")
    r.union_bounds_tensor(out[:n_labels], labels=lab, item_flags=w, mask=mask, stream=stream, skip_transparent=skip)
    return out, (lab, w)


def as_rec(a, n=None):
    a = np.ascontiguousarray(host_view(a)[:n] if n is not None else host_view(a))
    return a.view(REC).reshape(-1)


def same(got, want):
    return np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


def differing(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    size = g.dtype.itemsize if g.dtype.names else g.shape[-1] * g.dtype.itemsize
    return np.flatnonzero((g.view(np.uint8).reshape(-1, size) != w.view(np.uint8).reshape(-1, size)).any(axis=1))


def new_stream():
    if _emulated():
        return None
    import torch

    return torch.cuda.Stream()


def wait(r, stream):
    r.sync()
    if stream is not None:
        stream.synchronize()


@pytest.fixture(scope="module")
def bounds_renderer(pm):
    """Never resized: bounds need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


def check_items(pm, r, scene, name, stream=None):
    """The item records, host and device, with and without the skip flag: equal to np_bounds."""
    for skip in (False, True):
        want = bc.expected_boxes(pm, name, skip) if name is not None else np_bounds.item_bounds(scene, skip)
        n = len(want)
        dev = device_item_bounds(pm, r, n + 2, skip, stream)
        got = r.item_bounds(skip)
        bad = differing(got, want)
        assert bad.size == 0, (name, skip, len(bad), [(int(k), got[k].tolist(), want[k].tolist()) for k in bad[:6]])
        wait(r, stream)
        d = host_view(dev)
        bad = differing(d[:n], want)
        assert bad.size == 0, (name, "device", skip, len(bad), [(int(k), d[k].tolist(), want[k].tolist()) for k in bad[:6]])
        assert np.isnan(d[n:]).all(), (name, "records beyond n_items were written")
    return n


def check_unions(pm, r, scene, name, n, stream=None, labelings=None, masks=(None, 1, 2, 3)):
    """Every labelling under every mask, host and device: equal to np_bounds."""
    words = bc.selection_words(n, 7 + n)
    for lname, (labels, n_labels) in (labelings or bc.labelings(n)).items():
        for mask in masks:
            skip = mask in (1, 3)
            boxes = bc.expected_boxes(pm, name, skip) if name is not None else None
            want = np_bounds.union_bounds(scene, n_labels, labels, None if mask is None else words, mask or 3, skip, boxes)
            dev, keep = device_union(pm, r, n_labels, labels, None if mask is None else words, mask or 3, skip, stream, pad=1)
            got = r.union_bounds(labels, n_labels, None if mask is None else words[:n], mask or 3, skip)
            bad = differing(got, want)
            assert bad.size == 0, (name, lname, mask, len(bad), [(int(k), got[k], want[k]) for k in bad[:4]])
            wait(r, stream)
            d = as_rec(dev)
            bad = differing(d[:n_labels], want)
            assert bad.size == 0, (name, "device", lname, mask, len(bad), [(int(k), d[k], want[k]) for k in bad[:4]])
            assert (host_view(dev)[n_labels:] == UNTOUCHED).all()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_hand_derived_boxes(pm, bounds_renderer):
    """One item of every kind (rect_cases.known_scene): the boxes worked out in bounds_cases.KNOWN_BOXES, the scene's box and its counts."""
    r = bounds_renderer
    r.set_scene_bytes(bc.known_scene(pm))
    got = r.item_bounds()
    assert same(got, bc.KNOWN_BOXES), (got, bc.KNOWN_BOXES)
    dev = device_item_bounds(pm, r, 9)
    r.sync()
    assert same(host_view(dev), bc.KNOWN_BOXES)
    box, n_items, n_boxed = r.selection_bounds()
    assert box.tolist() == [9.5, 9.0, 120.5, 90.5] and (n_items, n_boxed) == (9, 8)
    box, n_items, n_boxed = r.selection_bounds(np.arange(9) == 8)        # the ellipse without geometry alone: counted, not boxed
    assert box.tolist() == [np.inf, np.inf, -np.inf, -np.inf] and (n_items, n_boxed) == (1, 0)
    box, n_items, n_boxed = r.selection_bounds([0, 2, 1, 0, 3, 0, 0, 0, 0], mask=2)      # words 2 and 3: the Polyline and the Line
    assert box.tolist() == [29.0, 9.0, 62.0, 62.0] and (n_items, n_boxed) == (2, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", bc.SCENES)
def test_case_scenes(pm, bounds_renderer, name):
    """The item records of every case scene and its unions under every labelling of bounds_cases.labelings, without words and with
    selection words under the masks 1, 2 and 3 -- host calls, and device calls on a caller's stream."""
    scene = bc.scene_of(pm, name)
    r = bounds_renderer
    r.set_scene_bytes(scene)
    stream = new_stream()
    n = check_items(pm, r, scene, name, stream)
    assert r.stats()["n_items"] == n
    check_unions(pm, r, scene, name, n, stream)


@pytest.mark.gpu
def test_selection_words_go_in_without_a_read_back(pm, bounds_renderer):
    """pm_select_rect_device's words go into pm_union_bounds_device as they were written, on the same (caller's) stream: the
    selection's box and size, and the box of every label, are np_bounds' under np_rect's words, for the masks 1, 2 and 3."""
    from test_hit_gpu import mixed_scene

    scene = mixed_scene(pm)
    r = bounds_renderer
    r.set_scene_bytes(scene)
    n = r.stats()["n_items"]
    stream = new_stream()
    labels = np.arange(n, dtype=np.uint32) % 3
    dev_labels = to_device(labels)
    touched_any = enclosed_any = 0
    for rect in ([90, 90, 260, 260], [0, 0, 600, 600], [1000, 1000, 1010, 1010], [15, 25, 225, 235]):
        if _emulated():
            words = np.full(n + 3, UNTOUCHED, np.uint32)
            rc = np.ascontiguousarray(rect, F32)
            pm._lib.check(pm._lib.load().pm_select_rect_device(r._h, rc.ctypes.data, 0, words.ctypes.data, words.size, None), "pm_select_rect_device")
        else:
            import torch

            words = torch.full((n + 3,), UNTOUCHED, dtype=torch.int32, device="cuda")
            r.select_rect_tensor(*[float(v) for v in rect], words, stream=stream)
        outs = [(mask, device_union(pm, r, 1, None, words, mask, stream=stream), device_union(pm, r, 3, dev_labels, words, mask, stream=stream)) for mask in (1, 2, 3)]
        wait(r, stream)
        model = np_rect.item_flags(scene, [rect])[:, 0].astype(np.uint32)
        assert np.array_equal(host_view(words).view(np.uint32)[:n], model)
        for mask, (one, _), (three, _) in outs:
            assert same(as_rec(one), np_bounds.union_bounds(scene, 1, None, model, mask)), (rect, mask)
            assert same(as_rec(three), np_bounds.union_bounds(scene, 3, labels, model, mask)), (rect, mask)
        touched_any += int((model & 1).any())
        enclosed_any += int((model & 2).any())
    assert touched_any >= 3 and enclosed_any >= 2


def _d19_rects(box):
    """For a boxed, finite D22 box: the rectangle made of the box rounded outward to f32, and the four with one side moved one f32 step
    inward -- each with whether D22 says pm_select_rect encloses (the comparisons in binary64)."""
    lo = box[:2].astype(F32)
    lo = np.where(lo.astype(np.float64) > box[:2], np.nextafter(lo, F32(-np.inf)), lo)
    hi = box[2:].astype(F32)
    hi = np.where(hi.astype(np.float64) < box[2:], np.nextafter(hi, F32(np.inf)), hi)
    outer = np.concatenate([lo, hi]).astype(F32)
    rects = [outer]
    for side in range(4):
        rc = outer.copy()
        rc[side] = np.nextafter(rc[side], F32(np.inf) if side < 2 else F32(-np.inf))
        rects.append(rc)
    rects = np.array(rects, F32)
    r64 = rects.astype(np.float64)
    inside = (r64[:, 0] <= box[0]) & (box[2] <= r64[:, 2]) & (r64[:, 1] <= box[1]) & (box[3] <= r64[:, 3])
    valid = np.isfinite(rects).all(axis=1) & (rects[:, 2] >= rects[:, 0]) & (rects[:, 3] >= rects[:, 1])
    return rects, inside & valid


def _d19_items(scene):
    """The items D22's property speaks about: every point finite and hw finite and >= 0."""
    sc = bytes(scene)
    out = []
    for i, (at, _) in enumerate(np_hit.flat_items(sc)):
        tag = np.frombuffer(sc, np.uint32, 1, at)[0] & 0xFFFF
        if tag in (np_hit.LINE, np_hit.POLY):
            a, b, hw = np_hit.stroke_segments(sc, at, tag)
            ok = np.isfinite(hw) and hw >= 0 and np.isfinite(a).all() and np.isfinite(b).all()
        elif tag == np_hit.FILL:
            p = np_hit._points(sc, at)
            if np.frombuffer(sc, np.uint32, 1, at + 4)[0] & np_hit.FILL_COMPOUND:
                p = p[~np.isnan(p[:, 0])]
            ok = bool(np.isfinite(p).all())
        else:   # (a Circle whose ShortBbox is inverted has a negative radius: the counterpart of hw < 0)
            x0, y0, x1, y1 = np_hit.flat_items(sc)[i][1]
            ok = tag == np_hit.CIRCLE and x1 >= x0 and y1 >= y0
        if ok:
            out.append(i)
    return out


D19_SCENES = ("known", "counts", "special")


@pytest.mark.gpu
def test_d22_is_d19s_encloses_on_the_device(pm, bounds_renderer):
    """For every item of D19_SCENES with finite points and hw >= 0: the device's own pm_select_rect reports PM_SEL_ENCLOSES for a
    rectangle iff the item is boxed and its pm_item_bounds box lies in the rectangle -- for the box rounded outward to f32 and the four
    rectangles with one side one f32 step further in."""
    r = bounds_renderer
    yes = no = 0
    for name in D19_SCENES:
        scene = bc.scene_of(pm, name)
        r.set_scene_bytes(scene)
        boxes = r.item_bounds()
        is_boxed = np_bounds.boxed(boxes)
        for i in _d19_items(scene):
            if not (is_boxed[i] and np.isfinite(boxes[i]).all()):
                _, enclosed = r.select_rect(-3.0e38, -3.0e38, 3.0e38, 3.0e38)
                assert not enclosed[i], (name, i)       # no box: nothing encloses it, not even everything
                continue
            rects, want = _d19_rects(boxes[i])
            for rc, w in zip(rects, want):
                _, enclosed = r.select_rect(*[float(v) for v in rc])
                assert bool(enclosed[i]) == bool(w), (name, i, boxes[i].tolist(), rc.tolist(), bool(w))
                yes += int(w)
                no += int(not w)
    assert yes >= 40 and no >= 160, (yes, no)     # (floors against a blind test: 49 boxed items in the three scenes, five rectangles each)


def _group_case(pm, r, ps, gmap, tables):
    n_groups = int(gmap.max()) + 1
    r.flatten_and_encode(ps.with_groups(gmap), (1.0, 0.0, 0.0, 1.0, 0.0, 0.0), 1.0)
    for aff, ws in tables:
        if aff is not None:
            r.reflatten_groups(aff, ws)
        scene = r.download_scene()
        labels = gmap[r.item_paths()]
        got = r.group_bounds()
        want = np_bounds.union_bounds(scene, n_groups, labels)
        assert same(got, want), (differing(got, want).tolist(), got, want)
        assert same(r.item_bounds(), np_bounds.item_bounds(scene))
        words = bc.selection_words(len(labels), 5)[: len(labels)]
        assert same(r.group_bounds(words, mask=2), np_bounds.union_bounds(scene, n_groups, labels, words, 2))
        assert got["n_items"].sum() == len(labels)
        yield got


@pytest.mark.gpu
def test_group_bounds_follow_reflatten_groups(pm):
    """A random path set in three groups: after the flatten, and after reflatten_groups with a translation, a rotation and a singular
    matrix in the table, group_bounds equals np_bounds on the downloaded scene; the translated group's box moved by the translation."""
    import path_sets
    from test_groups_gpu import SINGULAR, rot

    case = path_sets.random_case(321)
    ps = case.ps
    gmap = (np.arange(len(ps.paths), dtype=np.uint32) % 3).astype(np.uint32)
    aff = np.array([(1.0, 0.0, 0.0, 1.0, 32.0, -16.0), rot(0.7, 1.0, 40.0, 30.0), SINGULAR])
    ws = np.array([1.0, 1.0, 2.0], F32)
    with pm.Renderer(0) as r:
        first, moved = list(_group_case(pm, r, ps, gmap, [(None, None), (aff, ws)]))
        # (the same subdivisions under a translation; the f32 roundings of the points differ)
        assert np.abs(moved["box"][0] - (first["box"][0] + [32.0, -16.0, 32.0, -16.0])).max() < 1e-3
        assert not np.array_equal(moved["box"][1], first["box"][1]) and (moved["n_boxed"] > 0).all()
        r.set_scene_bytes(bc.known_scene(pm))
        with pytest.raises(pm._lib.PietMetalError):
            r.group_bounds()                                             # a scene that came from bytes has no paths


@pytest.mark.gpu
def test_group_bounds_of_styled_and_dashed_strokes(pm):
    """Outlined strokes with caps, joins and miter spikes, half of them dashed, one group per path and three groups: the boxes are
    those of the geometry the device made (np_bounds on the downloaded scene), not of the path elements."""
    from np_stroke import MITER, SQUARE, style_bits
    from test_stroke_gpu import shapes

    ps = shapes(lambda k: (3 if k % 4 == 0 else 2) | style_bits(SQUARE, MITER))
    ps = ps.with_dashes([8, 4], 0.0, select=[0, 4]).with_dashes([6, 3, 2], -4.0, select=[1, 2, 5])
    n = len(ps.paths)
    with pm.Renderer(0) as r:
        for gmap in (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32) % 3):
            aff = np.tile(np.array([(1.3, 0.5, -0.5, 1.3, 60.0, -20.0)]), (int(gmap.max()) + 1, 1))
            (a, b) = list(_group_case(pm, r, ps, gmap, [(None, None), (aff, None)]))
            assert (a["n_boxed"] > 0).all() and not same(a, b)


@pytest.mark.gpu
def test_capacity_and_argument_rules(pm, pmo):
    lib = pm._lib.load()
    L = pm._lib
    OK = L.PM_OK
    with pm.Renderer(0) as r:
        n_items = C.c_uint32(77)
        boxes = np.full((4, 4), np.nan, np.float64)
        rec = np.full((4, 10), UNTOUCHED, np.int32)
        words = np.ones(16, np.uint32)
        labels = np.zeros(16, np.uint32)
        bp, rp, wp, lp = boxes.ctypes.data, rec.ctypes.data, words.ctypes.data, labels.ctypes.data
        items = [lambda flags, out, cap: lib.pm_item_bounds(r._h, flags, out, cap, None), lambda flags, out, cap: lib.pm_item_bounds_device(r._h, flags, out, cap, None)]
        unions = [lambda *a: lib.pm_union_bounds(r._h, *a), lambda *a: lib.pm_union_bounds_device(r._h, *a, None)]   # (flags, words, n_words, mask, labels, n_label_words, n_labels, out)
        # no resident scene
        for call in items:
            assert call(0, bp, 4) == INVALID
        assert lib.pm_item_bounds(r._h, 0, bp, 4, C.byref(n_items)) == INVALID and n_items.value == 0
        for call in unions:
            assert call(0, None, 0, 0, None, 0, 1, rp) == INVALID
        r.set_scene_bytes(pmo.scene_path_test())
        assert r.stats()["n_items"] == 1
        for call in items:
            assert call(2, bp, 4) == INVALID                                   # unknown flag bits
            assert call(0x80000001, bp, 4) == INVALID
            assert call(0, bp, 0) == CAPACITY                                  # too small: nothing is written
            assert call(0, None, 0) == CAPACITY
            assert call(0, None, 4) == INVALID                                 # a NULL out
        n_items.value = 77
        assert lib.pm_item_bounds(r._h, 0, None, 0, C.byref(n_items)) == CAPACITY and n_items.value == 1
        assert lib.pm_item_bounds_device(r._h, 0, bp + 4, 4, None) == INVALID      # not 8-byte aligned
        for call in unions:
            assert call(2, None, 0, 0, None, 0, 1, rp) == INVALID               # unknown flag bits
            assert call(0, None, 0, 0, None, 0, 0, rp) == INVALID               # n_labels == 0
            assert call(0, wp, 0, 1, None, 0, 1, rp) == INVALID                 # fewer words than items
            assert call(0, wp, 16, 0, None, 0, 1, rp) == INVALID                # word_mask == 0
            assert call(0, None, 0, 0, lp, 0, 1, rp) == INVALID                 # fewer labels than items
            assert call(0, None, 0, 0, None, 0, 1, None) == INVALID             # a NULL out
        assert lib.pm_union_bounds_device(r._h, 0, None, 0, 0, None, 0, 1, rp + 4, None) == INVALID      # not 8-byte aligned
        r.sync()
        assert np.isnan(boxes).all() and (rec == UNTOUCHED).all()
        # more words and labels than items, a mask of high bits, NULL words with counts that do not matter: fine.  (Only the host
        # calls may be given these arrays to work on: they are host memory)
        words[0] = 0x80000000
        assert unions[0](1, wp, 16, 0x80000000, lp, 16, 2, rp) == OK
        want = np_bounds.union_bounds(pmo.scene_path_test(), 2, labels, words, 0x80000000, True)
        assert same(rec[:2].view(REC).reshape(-1), want) and (rec[2:] == UNTOUCHED).all() and want["n_items"].tolist() == [1, 0]
        assert unions[0](0, None, 5, 0, None, 7, 1, rp) == OK and rec.view(REC).reshape(-1)[0]["n_items"] == 1
        assert items[0](1, bp, 4) == OK and np.isnan(boxes[1:]).all() and not np.isnan(boxes[0]).any()
        assert lib.pm_abi_version() == 600
        # the Python wrappers
        assert r.item_bounds().shape == (1, 4) and r.item_bounds().dtype == np.float64
        with pytest.raises(ValueError):
            r.union_bounds(None, 0)
        with pytest.raises(ValueError):
            r.union_bounds(np.zeros((1, 1), np.uint32), 1)
        with pytest.raises(pm._lib.PietMetalError):
            r.group_bounds()                                                    # as item_paths: the scene did not come from paths
        if not _emulated():
            import torch

            o = torch.zeros((2, 10), dtype=torch.int32, device="cuda")
            b = torch.zeros((2, 4), dtype=torch.float64, device="cuda")
            with pytest.raises(TypeError):
                r.item_bounds_tensor(torch.zeros((2, 4), dtype=torch.float64))           # not on the device
            with pytest.raises(TypeError):
                r.item_bounds_tensor(torch.zeros((2, 4), device="cuda"))                 # float32
            with pytest.raises(TypeError):
                r.item_bounds_tensor(b[:, :3])
            with pytest.raises(TypeError):
                r.union_bounds_tensor(torch.zeros((2, 10), device="cuda"))               # floating point
            with pytest.raises(TypeError):
                r.union_bounds_tensor(o[:, :8])
            with pytest.raises(TypeError):
                r.union_bounds_tensor(o, labels=torch.zeros(4, device="cuda"))
            with pytest.raises(TypeError):
                r.union_bounds_tensor(o, item_flags=torch.zeros((4, 1), dtype=torch.int32, device="cuda"))
            with pytest.raises(pm._lib.PietMetalError):
                r.item_bounds_tensor(b[:0])                                              # capacity
            r.item_bounds_tensor(b)
            r.union_bounds_tensor(o, labels=torch.zeros(1, dtype=torch.int32, device="cuda"))
            r.sync()
            assert o.cpu().numpy().view(REC).reshape(-1)["n_items"].tolist() == [1, 0]


@pytest.mark.gpu
def test_a_scene_without_items(pm, bounds_renderer):
    """n_items == 0: pm_item_bounds writes nothing; pm_union_bounds writes every record, the empty box and two zeros."""
    lib = pm._lib.load()
    r = bounds_renderer
    r.set_scene_bytes(hs._encode(pm, 0, lambda e: None))
    assert r.stats()["n_items"] == 0
    n_items = C.c_uint32(77)
    boxes = np.full((2, 4), np.nan, np.float64)
    assert lib.pm_item_bounds(r._h, 0, boxes.ctypes.data, 2, C.byref(n_items)) == pm._lib.PM_OK and n_items.value == 0
    assert lib.pm_item_bounds(r._h, 0, None, 0, None) == pm._lib.PM_OK
    dev = device_item_bounds(pm, r, 2)
    assert r.item_bounds().shape == (0, 4)
    want = np.zeros(65, REC)
    want["box"] = np_bounds.EMPTY
    for n_labels in (1, 65):
        out, keep = device_union(pm, r, n_labels, pad=1)
        got = r.union_bounds(None, n_labels)
        r.sync()
        assert same(got, want[:n_labels]) and same(as_rec(out)[:n_labels], want[:n_labels]) and (host_view(out)[n_labels:] == UNTOUCHED).all()
    assert same(r.union_bounds(np.zeros(0, np.uint32), 2, np.zeros(0, np.uint32)), want[:2])
    box, n, nb = r.selection_bounds()
    assert box.tolist() == np_bounds.EMPTY.tolist() and (n, nb) == (0, 0)
    assert np.isnan(boxes).all() and np.isnan(host_view(dev)).all()


@pytest.mark.gpu
def test_a_query_answers_for_the_scene_resident_at_the_call(pm):
    """The Tiger at 480 x 270: device calls on a caller's stream, followed at once by two re-flattens -- the answers are the first
    scene's; the host calls afterwards answer for the last."""
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene0 = r.download_scene()
        n = r.stats()["n_items"]
        labels = r.item_paths().astype(np.uint32) % 40
        s = new_stream()
        dev_b = device_item_bounds(pm, r, n, stream=s)
        dev_u, keep = device_union(pm, r, 40, labels, stream=s)
        r.reflatten((1.8, 0.6, -0.6, 1.8, 150.0, -20.0), wl.width_scale)
        r.reflatten((0.9, 0.0, 0.0, 0.9, 40.0, 30.0), wl.width_scale)
        wait(r, s)
        want0 = np_bounds.item_bounds(scene0)
        assert same(host_view(dev_b), want0) and same(as_rec(dev_u), np_bounds.union_bounds(scene0, 40, labels, boxes=want0))
        scene2 = r.download_scene()
        want2 = np_bounds.item_bounds(scene2)
        assert same(r.item_bounds(), want2) and not same(want2, want0)
        assert same(r.union_bounds(labels, 40), np_bounds.union_bounds(scene2, 40, labels, boxes=want2))
        assert np_bounds.boxed(want2).sum() > 200


@pytest.mark.gpu
def test_queries_between_frames_leave_the_frames_alone(pm, pmo):
    """Frames rendered before and after bounds queries have the bytes they have without them; a scene replacement between two
    queries gives each its own scene."""
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        scene = r.download_scene()
        want_px = pmo.render(scene, wl.width, wl.height)
        want = np_bounds.item_bounds(scene)
        r.render()
        dev_b = device_item_bounds(pm, r, len(want))         # behind the frame, not waited for
        dev_u, keep = device_union(pm, r, 1)
        first = r.read_pixels()
        r.render()
        host = r.item_bounds()
        second = r.read_pixels()
        assert np.array_equal(first, want_px) and np.array_equal(second, want_px)
        assert same(host_view(dev_b), want) and same(host, want) and same(as_rec(dev_u), np_bounds.union_bounds(scene, 1, boxes=want))
        r.render()
        dev_u, keep = device_union(pm, r, 1)                  # frame in flight, query, replacement, query
        r.set_scene_bytes(bc.known_scene(pm))
        dev_k, keep_k = device_union(pm, r, 1)
        r.sync()
        assert same(as_rec(dev_u), np_bounds.union_bounds(scene, 1, boxes=want))
        assert as_rec(dev_k)[0]["box"].tolist() == [9.5, 9.0, 120.5, 90.5] and as_rec(dev_k)[0]["n_items"] == 9


@pytest.mark.gpu
def test_cli_bounds_and_fit(pm, tmp_path, capsys):
    """--bounds prints the scene's box and, with --select, the selection's box and counts as one JSON line; --fit maps that box onto the
    output size before rendering."""
    from piet_metal_amd import cli

    wl = pm.workloads.tiger(480, 270)
    sel = (150.0, 60.0, 330.0, 220.0)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        box, n, nb = r.selection_bounds()
        touched, _ = r.select_rect(*sel)
        sbox, sn, snb = r.selection_bounds(touched)
    out = str(tmp_path / "t.png")
    assert cli.main(["tiger", out, "--width", "480", "--height", "270", "--bounds", "--select", ",".join(f"{v:g}" for v in sel)]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert got["scene"] == {"box": box.tolist(), "n_items": n, "n_boxed": nb}
    assert got["selection"] == {"box": sbox.tolist(), "n_items": sn, "n_boxed": snb} and 0 < sn < n
    plain = cli.read_png_rgba(out)
    assert cli.main(["tiger", out, "--width", "480", "--height", "270", "--fit", "--bounds"]) == 0
    fit = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][0])
    fb = fit["scene"]["box"]
    # the fitted scene's box touches the view's edges along one axis and is centred along the other -- to a pixel: the curves are
    # flattened again at the new scale, within the flattening tolerance of either scale
    assert min(fb[0], fb[1]) > -1.0 and fb[2] < 481.0 and fb[3] < 271.0
    assert (abs(fb[0]) < 1.0 and abs(fb[2] - 480) < 1.0) or (abs(fb[1]) < 1.0 and abs(fb[3] - 270) < 1.0)
    assert abs((fb[0] + fb[2]) - 480) < 2.0 and abs((fb[1] + fb[3]) - 270) < 2.0
    assert max(box[2] - box[0], box[3] - box[1]) < 0.9 * max(fb[2] - fb[0], fb[3] - fb[1]) or box[3] - box[1] > 260      # (it was smaller than the view before)
    assert not np.array_equal(cli.read_png_rgba(out), plain)


# ---- CPU: np_bounds itself, the header, the cases ----------------------------------------------------------------------------------

def test_np_bounds_against_hand_derived_boxes(pm):
    scene = bc.known_scene(pm)
    got = np_bounds.item_bounds(scene)
    assert same(got, bc.KNOWN_BOXES)
    u = np_bounds.union_bounds(scene, 2, np.array([0, 0, 1, 1, 0, 1, 5, 0, 1], np.uint32))
    assert u["box"].tolist() == [[9.5, 9.0, 120.5, 90.5], [10.0, 10.0, 100.0, 70.0]] and u["n_items"].tolist() == [4, 4] and u["n_boxed"].tolist() == [4, 3]
    # by hand, from bounds_cases.special_scene's own numbers
    b = bc.expected_boxes(pm, "special")
    S = bc.SPECIAL
    for name, box in {
        "poly_one_point": [28, 18, 32, 22], "poly_width_0": [10, 40, 50, 60], "poly_width_negative": [13, 73, 47, 87], "poly_width_very_negative": [60, 120, -38, 24],
        "line_width_negative": [61.5, 41.5, 88.5, 58.5], "line_width_0": [60, 65, 90, 70], "fill_negative_zero": [0, 0, 0, 0], "fill_zero_max": [-5, -7, 0, 0],
        "fill_nan_x": [100, 5, 140, 50], "fill_nan_y": [100, 60, 150, 90], "poly_all_x_nan": [np.inf, 99, -np.inf, 109],
        "compound_separator_chunk": [250, 20, 280, 60], "circle_saturated": [0, 0, 65535, 65535], "circle_saturated_low": [0, 6.5, 7, 13.5],
        "ellipse_saturated_high": [65000, 65530, 65535, 65535], "circle_r_0": [300, 150, 300, 150], "circle_inverted": [40, 35, 30, 25],
        "ellipse_odd_sum": [10, 20, 21, 45], "fill_last": [5.5, 6.5, 7.5, 8.5], "poly_infinite": [189, -np.inf, np.inf, 101],
    }.items():
        assert b[S[name]].tolist() == [float(v) for v in box], (name, b[S[name]])
    for name in ("poly_width_nan", "line_width_nan", "fill_all_nan", "compound_only_separators", "ellipse_rx_0", "ellipse_ry_0"):
        assert same(b[S[name]], np_bounds.EMPTY), name
    seed = np.float64(bc.SEED)
    assert b[S["fill_at_plus_seed"]].tolist() == [seed] * 4 and b[S["fill_at_minus_seed"]].tolist() == [-seed] * 4
    assert b[S["fill_one_point_at_seed"]][[1, 2]].tolist() == [-seed, seed] and b[S["poly_at_minus_seed"]][[0, 3]].tolist() == [-seed - 1, seed + 1]
    # a bound that is a zero is +0, whatever the zeros of the points were
    for name in ("fill_negative_zero", "fill_zero_max", "poly_negative_zero"):
        zero = b[S[name]] == 0
        assert zero.any() and not np.signbit(b[S[name]][zero]).any(), name
    # the separator that names a separator: its index bits (512.0 as a float) are no y
    assert b[S["compound_separator_names_separator"]][3] < 121
    skipped = bc.expected_boxes(pm, "special", True)
    gone = [S[k] for k in S if k.endswith("_transparent")]
    assert len(gone) == 4 and all(same(skipped[i], np_bounds.EMPTY) for i in gone) and np_bounds.boxed(b[gone]).all()
    keep = np.setdiff1d(np.arange(len(b)), gone)
    assert same(skipped[keep], b[keep])
    assert not np.isnan(b).any()


def test_the_header_and_the_record_sizes():
    inc = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    for line in ("#define PM_ABI_VERSION 600u", "#define PM_HIT_SKIP_TRANSPARENT 1u", "#define PM_SEL_TOUCHES 1u", "#define PM_SEL_ENCLOSES 2u",
                 "typedef struct { double x0, y0, x1, y1; } pm_bounds;", "typedef struct { pm_bounds box; uint32_t n_items, n_boxed; } pm_label_bounds;"):
        assert line in inc, line

    class Bounds(C.Structure):
        _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("x1", C.c_double), ("y1", C.c_double)]

    class LabelBounds(C.Structure):
        _fields_ = [("box", Bounds), ("n_items", C.c_uint32), ("n_boxed", C.c_uint32)]

    assert C.sizeof(Bounds) == 32 and C.sizeof(LabelBounds) == 40 and LabelBounds.n_items.offset == 32 and LabelBounds.n_boxed.offset == 36
    assert REC.itemsize == 40 and REC.fields["n_items"][1] == 32
    from piet_metal_amd import _lib, renderer

    assert renderer.LABEL_BOUNDS_DTYPE == REC
    for name in ("pm_item_bounds", "pm_item_bounds_device", "pm_union_bounds", "pm_union_bounds_device"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(pm_ctx \*c, uint32_t flags,", inc), name
    assert bc.LANE == 16 and "kBoundsLane = 16u" in open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_bounds.h")).read()


def test_the_cases_are_what_they_claim(pm):
    assert bc.WAVE == 64 and hs.CHUNK_SEGS == 4 and hs.SUPER_CHUNKS == 8
    assert bc.POINT_COUNTS == (0, 1, 2, 4, 5, 8, 9) and bc.WALK_SIZES == (1, 63, 64, 65, 257) and set(bc.LONG_SIZES) >= {8, 9, 16, 17, 64, 65}
    # counts_scene: the point counts, and how many chunks the index gives them
    sc = bytes(bc.counts_scene(pm))
    items = np_hit.flat_items(sc)
    npts = [int(np.frombuffer(sc, np.uint32, 1, at + 12)[0]) for at, _ in items]
    assert npts[0::3] == list(bc.POINT_COUNTS) and npts[2::3] == list(bc.POINT_COUNTS)
    base, chunk_bbox, _ = hs.index_model(bc.counts_scene(pm))
    per_item = np.diff(base)
    assert per_item[0::3].tolist() == [0, 1, 1, 1, 2, 2, 3] and per_item[2::3].tolist() == [0, 0, 1, 1, 1, 2, 2]     # (a one-point Polyline owns no chunk)
    # long_scene: the sizes are exact, and the extremes sit in the first chunk, the last and the one behind the 64th
    scene = bc.long_scene(pm)
    base, chunk_bbox, _ = hs.index_model(scene)
    per_item = np.diff(base)
    boxes = bc.expected_boxes(pm, "long")
    assert per_item[0] == 3 and base[1] % hs.SUPER_CHUNKS == 3
    for j, (kind, size) in enumerate(bc.LONG):
        i = j + 1
        cb0, cb1 = base[i], base[i + 1]
        if kind != "compound":
            assert cb1 - cb0 == size, (kind, size)
            cb = chunk_bbox[cb0:cb1].astype(np.float64)
            assert cb[-1, 3] == 500.0 and (cb[:-1, 3] < 500.0).all() and cb[0, 0] == boxes[i][0] + (0.25 if kind == "polyline" else 0.0)
            low = 64 if size > 65 else 1
            assert cb[low, 1] == -500.0 and (np.delete(cb[:, 1], [low - 1, low]) > -500.0).all()
        assert boxes[i][1] == -500.0 - (0.25 if kind == "polyline" else 0.0) and boxes[i][3] == 500.0 + (0.25 if kind == "polyline" else 0.0)
    # special_scene: the index keeps its seed where a chunk met no value, and a separator's index bits where a separator names a separator
    base, chunk_bbox, _ = hs.index_model(bc.special_scene(pm))
    S = bc.SPECIAL
    sc = bytes(bc.special_scene(pm))
    pts = np_hit._points(sc, np_hit.flat_items(sc)[S["compound_separator_chunk"]][0])
    assert np.isnan(pts[4:8, 0]).all() and not np.isnan(pts[:4, 0]).any() and not np.isnan(pts[8:12, 0]).any() and len(pts) == 13
    assert chunk_bbox[base[S["compound_separator_chunk"]] + 1].tolist() == [bc.SEED, bc.SEED, -bc.SEED, -bc.SEED]
    assert chunk_bbox[base[S["compound_separator_names_separator"]], 3] == 512.0      # (the index bits of the separator that is named, as a y)
    pts = np_hit._points(sc, np_hit.flat_items(sc)[S["fill_chunk_of_nans"]][0])
    assert np.isnan(pts[4:9]).all()
    boxes = [b for _, b in np_hit.flat_items(sc)]
    assert boxes[S["circle_saturated"]] == (0, 0, 65535, 65535) and boxes[S["ellipse_rx_0"]][0] == boxes[S["ellipse_rx_0"]][2]
    # the walk scenes: every kind, a child group, items of alpha 0
    for n in bc.WALK_SIZES:
        scene = bc.walk_scene(pm, n)
        assert len(np_hit.flat_items(bytes(scene))) == n
        assert np_bounds.skipped_items(scene, True).sum() == sum(1 for i in range(n) if i % 3 == 0 and hs.walk_kind(i) not in ("circle", "ellipse"))
    # the labellings: a run that crosses item 64, labels out of range, labels nobody carries
    labs = bc.labelings(257)
    runs = labs["runs_of_48"][0]
    assert runs[63] == runs[64] == 1 and runs[47] != runs[48]
    oor, n_labels = labs["out_of_range"]
    assert (oor == 0xFFFFFFFF).any() and (oor == 3).any() and n_labels == 3
    assert len(np.unique(labs["sparse_1000"][0])) < 200 and labs["sparse_65"][1] == 65 and labs["none"] == (None, 1)
    w = bc.selection_words(257, 1)
    assert len(w) == 260 and set(w.tolist()) == {0, 1, 2, 3}


# ---- CPU: D22 <=> D19 (np_bounds against np_rect, no kernel) ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["known", "counts", "special", "long", "walk-65", "mixed", "edge", "edge-scenes"])
def test_d22_is_d19s_encloses(pm, name):
    """For every item with finite points and hw >= 0: np_rect says "encloses" for the box rounded outward to f32; for each of the four
    rectangles with one side one f32 step further in it says so iff the box still lies inside (never, where the outward rounding was exact)."""
    if name == "edge-scenes":
        import edge_scenes as es

        scenes = [es.edge_scene(pm, seed, small=True, n=24)[0] for seed in es.SMALL_SEEDS[:12]]
    elif name in ("mixed", "edge"):
        from test_hit_gpu import edge_scene, mixed_scene

        scenes = [mixed_scene(pm) if name == "mixed" else edge_scene(pm)]
    else:
        scenes = [bc.scene_of(pm, name)]
    yes = no = exact = 0
    for scene in scenes:
        boxes = np_bounds.item_bounds(scene)
        is_boxed = np_bounds.boxed(boxes)
        items = _d19_items(scene)
        everything = np_rect.item_flags(scene, [[-3.0e38, -3.0e38, 3.0e38, 3.0e38]])[:, 0]
        for i in items:
            if not (is_boxed[i] and np.isfinite(boxes[i]).all()):
                assert not everything[i] & np_rect.ENCLOSES, (name, i)
                continue
            rects, want = _d19_rects(boxes[i])
            got = (np_rect.item_flags(scene, rects)[i] & np_rect.ENCLOSES) != 0
            assert np.array_equal(got, want), (name, i, boxes[i].tolist(), rects.tolist(), got.tolist(), want.tolist())
            assert want[0] or not np.isfinite(rects[0]).all()
            was_exact = (rects[0].astype(np.float64) == boxes[i])
            assert not want[1:][was_exact].any()
            yes += int(want.sum())
            no += int((~want).sum())
            exact += int(was_exact.sum())
    print(f"{name}: {yes} enclosing and {no} not enclosing rectangles, {exact} sides rounded exactly")
    assert yes >= 4 and no >= 16 and (name != "special" or exact < 4 * yes)     # (floors against a blind test; the special scene has a box that is no f32 value)


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_bounds_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout


# ---- CPU: the compiler's listing ------------------------------------------------------------------------------------------------

def test_the_bounds_kernels_use_no_scratch(tmp_path):
    """The four kernels of pm_bounds.h by the flags the library is built with: no private segment (nothing spilled, no indexed local
    array), no LDS, and VGPRs within 128 -- a workgroup of four waves puts one on each SIMD of a CU, which has 512 VGPRs per lane: four
    such workgroups per CU.  The figures are printed (pytest -s) and stand in DESIGN.md 4.  Sizes only: the assembly is searched for no
    instruction."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = set()
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        name = next((k for k in ("pm_item_bounds_kernel", "pm_union_bounds_kernel", "pm_bounds_init_kernel", "pm_bounds_final_kernel") if k in m.group(1)), None)
        if name is None:
            continue
        found.add(name)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"{name}: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        assert scratch == 0 and vgpr <= 128 and lds == 0, (name, scratch, vgpr, lds)
    assert len(found) == 4, found
    assert "pm_bounds.h" in mk     # (editing the header rebuilds the library)
