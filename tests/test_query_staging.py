"""The host-memory query calls share ONE grow-only staging buffer on the device (QueryStaging, piet_metal_amd/csrc/pm_context.hip):
pm_hit_test, pm_hit_frame, pm_hit_rects, pm_select_rect, pm_select_polygon, pm_snap, pm_snap_intersections, pm_item_bounds,
pm_union_bounds, pm_hit_stack, pm_hit_rects_stack, pm_item_lengths, pm_points_at_length and pm_positions_on_edges lay their
records, their queries and their per-item words out in it, each in its own way (the stacks: k words and a count per query in front
of the queries; the measure calls: 16-byte queries behind 32- or 16-byte records, or a record per item), and every such call ends
with the context's stream synchronised.  What one call leaves in the buffer, and whether the buffer grew or was reused, must not
show in the next call's answer.

-m gpu: one context through the calls of every family interleaved, at sizes that make the buffer grow, be reused by smaller
calls and grow again -- every answer EQUAL as bytes to the same call on a fresh context; a device call on a second stream, a host
call of another family and a scene replacement in a row -- the answers are numpy's (tests/np_snap.py, tests/np_hit.py) for the
scene resident at each call.
CPU: the -m gpu part against the wave64 emulation of the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_cross  # noqa: E402
import np_hit  # noqa: E402
from np_measure import ITEM_LENGTH, LENGTH_POINT  # noqa: E402
import np_snap  # noqa: E402
import snap_cases as sc  # noqa: E402
from test_snap import as_rec, device_snap, same  # noqa: E402

NONE = sc.NONE
N_GPU_TESTS = 2
SIZES = (1, 300, 1, 5000)                # queries (pixels, labels) of successive calls: the buffer grows, is reused smaller, grows again
EMULATED_BIG = "snap"                    # under the emulation one family alone goes to 5000, the other is held at 300
FRAMES = {1: (1, 1), 300: (20, 15), 5000: (100, 50)}     # hit_frame: w x h pixels
LASSO = np.array([[60, 40], [300, 70], [420, 260], [250, 330], [90, 300], [150, 180]], np.float32)


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


def _points(n, seed):
    return np.random.default_rng(seed).uniform(-20.0, 540.0, (n, 2)).astype(np.float32)


def _radii(n, seed):
    return np.random.default_rng(seed).choice([1.0, 4.0, 16.0, 64.0], n).astype(np.float32)


def _rects(n, seed):
    p, t = _points(n, seed), _radii(n, seed + 1)[:, None]
    return np.concatenate([p - t, p + t], axis=1).astype(np.float32)


STACK_K = 7


def _items(case, n):
    """n item indices: over the scene's items and one past the last."""
    return (np.arange(n, dtype=np.uint32) * 7) % np.uint32(len(case.mask) + 1)


def _positions(n):
    """n positions in units of 2^-16 px: 0, then steps of 3.25 px, so that ends, interiors and positions beyond the end occur."""
    return (np.arange(n, dtype=np.uint64) % 97) * np.uint64(212992)


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# family -> call(renderer, case, n) -> the answer as bytes, in the order of the calls.  select_rect, select_polygon and item_bounds
# have no number of queries: they stage a word or a record per item.  union_bounds stages n records and two words per item.
# The five calls of D24 and D25 stand at the end, so that the first ten calls of schedule() and their sizes are what they were:
# the stacks stage n * (k + 1) words and the queries (k = 7: records of no power of two), item_lengths a record per item, the two
# per-query measure calls n records and n queries (items cycle over the scene and one past it, positions over a few lengths).
FAMILIES = {
    "hit_test": lambda r, case, n: _bytes(*r.hit_test(_points(n, 11), counts=True)),
    "hit_rects": lambda r, case, n: _bytes(*r.hit_rects(_rects(n, 12), counts=True)),
    "select_rect": lambda r, case, n: _bytes(*r.select_rect(90.0, 90.0, 260.0, 260.0)),
    "snap": lambda r, case, n: _bytes(r.snap(_points(n, 14), _radii(n, 15))),
    "hit_frame": lambda r, case, n: _bytes(*r.hit_frame(60, 40, *FRAMES[n], counts=True)),
    "snap_masked": lambda r, case, n: _bytes(r.snap(_points(n, 14), _radii(n, 15), skip_items=case.mask)),
    "select_polygon": lambda r, case, n: _bytes(*r.select_polygon(LASSO)),
    "snap_intersections": lambda r, case, n: _bytes(r.snap_intersections(_points(n, 16), _radii(n, 17))),
    "item_bounds": lambda r, case, n: _bytes(r.item_bounds()),
    "union_bounds": lambda r, case, n: _bytes(r.union_bounds(np.arange(len(case.mask), dtype=np.uint32) % n, n, item_flags=case.mask == 0, mask=1)),
    "item_lengths": lambda r, case, n: _bytes(r.item_lengths()),
    "hit_stack": lambda r, case, n: _bytes(*r.hit_stack(_points(n, 18), STACK_K, counts=True)),
    "hit_rects_stack": lambda r, case, n: _bytes(*r.hit_rects_stack(_rects(n, 19), STACK_K, stop_at_opaque=True, counts=True)),
    "points_at_length": lambda r, case, n: _bytes(r.points_at_units(_items(case, n), _positions(n))),
    "positions_on_edges": lambda r, case, n: _bytes(r.positions_on_edges(_items(case, n), np.arange(n) % 5, (np.arange(n) % 9) / np.float32(8.0))),
}


SECOND_SIZE = (("hit_test", 5000), ("hit_rects", 1))     # the two batched point and rectangle calls also at the other end of the sizes


def schedule():
    """(family, n) call by call: the query counts go 1, 300, 1, 5000 while the calls cycle through the families; hit_test and
    hit_rects once more at a size they did not have -- a family called small, then large, and large, then small, on the same
    context --; then all of these in reverse order, so that every call is also made behind another one (a small call behind the
    largest, the largest again in a buffer that holds it) and every reference serves twice."""
    calls = [(family, SIZES[k % len(SIZES)]) for k, family in enumerate(FAMILIES)] + list(SECOND_SIZE)
    calls = [(family, 300 if _emulated() and n == 5000 and family != EMULATED_BIG else n) for family, n in calls]
    return calls + calls[::-1]


@pytest.mark.gpu
def test_interleaved_host_calls_answer_as_on_a_fresh_context(pm):
    """mixed_scene (every item class).  ONE context makes the calls of schedule(); each answer is, byte for byte, that of the same call
    as the first and only call of a fresh context (a context takes half a second to make: hence one size for most families)."""
    case = sc.small_case(pm, "mixed")
    calls = schedule()
    assert {f for f, _ in calls} == set(FAMILIES) and [n for _, n in calls[:4]] == list(SIZES) and ("snap", 5000) in calls
    fresh = {}
    for family, n in calls[:len(calls) // 2]:
        with pm.Renderer(0) as r:
            r.set_scene_bytes(case.scene)
            fresh[family, n] = FAMILIES[family](r, case, n)
    assert len(fresh) == len(calls) // 2
    with pm.Renderer(0) as r:
        r.set_scene_bytes(case.scene)
        for k, (family, n) in enumerate(calls):
            assert FAMILIES[family](r, case, n) == fresh[family, n], (k, family, n)
    fresh = {family: fresh[family, n] for family, n in calls[:len(FAMILIES)]}
    # the answers are answers: items are found and missed, every record is there, and the skip words, uploaded behind the records and
    # the queries, take their items out (tests/np_snap.py)
    sizes = dict(calls[:len(FAMILIES)])
    for family, dtype in (("snap", np_snap.RECORD), ("snap_intersections", np_cross.RECORD)):
        rec = np.frombuffer(fresh[family], dtype)
        assert len(rec) == sizes[family] and (rec["item"] != NONE).any() and (rec["item"] == NONE).any(), family
    top = np.frombuffer(fresh["hit_rects"], np.uint32)[:sizes["hit_rects"]]
    assert len(set(top.tolist())) > 4 and (top == NONE).any()
    n = sizes["snap_masked"]
    xyr = np.concatenate([_points(n, 14), _radii(n, 15)[:, None]], axis=1)
    assert fresh["snap_masked"] == np_snap.snap(case.scene, xyr, skip_items=case.mask).tobytes() != np_snap.snap(case.scene, xyr).tobytes()
    assert len(fresh["union_bounds"]) == sizes["union_bounds"] * 40 and len(fresh["item_bounds"]) == len(case.mask) * 32
    assert np.frombuffer(fresh["select_polygon"], np.bool_).any() and np.frombuffer(fresh["select_rect"], np.bool_).any()
    n = sizes["hit_stack"]
    assert len(fresh["hit_stack"]) == n * (STACK_K + 1) * 4 and len(fresh["hit_rects_stack"]) == sizes["hit_rects_stack"] * (STACK_K + 1) * 4
    items, cnt = np.frombuffer(fresh["hit_stack"], np.uint32)[:n * STACK_K].reshape(n, STACK_K), np.frombuffer(fresh["hit_stack"], np.uint32)[n * STACK_K:]
    assert (cnt == 0).any() and (cnt > 1).any() and ((items != NONE).sum(axis=1) == np.minimum(cnt, STACK_K)).all()
    lengths = np.frombuffer(fresh["item_lengths"], ITEM_LENGTH)
    assert len(lengths) == len(case.mask) and (lengths["length"] > 0).any()
    pts = np.frombuffer(fresh["points_at_length"], LENGTH_POINT)
    assert len(pts) == sizes["points_at_length"] and (pts["item"] != NONE).any() and (pts["item"] == NONE).any() and len(set(pts["status"].tolist())) > 2
    assert len(fresh["positions_on_edges"]) == sizes["positions_on_edges"] * 16


@pytest.mark.gpu
def test_a_device_call_a_host_call_and_a_replacement_in_a_row(pm):
    """pm_snap_device on a caller's stream, pm_hit_test (the staging buffer's first use: it is allocated while the device call may
    still run) and a scene replacement, nothing waited for in between: both answer for the first scene, the host calls afterwards
    for the second."""
    first, second = sc.small_case(pm, "mixed"), sc.small_case(pm, "ties")
    pts = _points(300, 21)
    with pm.Renderer(0) as r:
        r.set_scene_bytes(first.scene)
        if _emulated():
            s = None
        else:
            import torch

            s = torch.cuda.Stream()
        dev, keep = device_snap(pm, r, first.xyr, stream=s)
        top, cnt = r.hit_test(pts, counts=True)
        r.set_scene_bytes(second.scene)
        r.sync()
        if s is not None:
            s.synchronize()
        want = np_snap.snap(first.scene, first.xyr)
        assert same(as_rec(dev), want) and not same(want, np_snap.snap(second.scene, first.xyr))
        want_top, want_cnt = np_hit.hit_test(first.scene, pts)
        assert np.array_equal(top, want_top) and np.array_equal(cnt, want_cnt)
        assert same(r.snap(first.xyr[:, :2], first.xyr[:, 2]), np_snap.snap(second.scene, first.xyr))
        top2 = r.hit_test(pts)
        assert np.array_equal(top2, np_hit.hit_test(second.scene, pts)[0]) and not np.array_equal(top2, top)


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_query_staging_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout
