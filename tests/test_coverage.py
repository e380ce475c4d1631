"""Coverage counts, pm_item_coverage / pm_item_coverage_device (decision D28): per item the pixels of a rectangle it covers, those that
show it, those where it is the topmost item, and the first pixel that shows it.

The bar everywhere: the bytes of all n_items records EQUAL to tests/np_coverage.py -- through the host call and the device call, with
and without skip_transparent, with and without visible_only.  tests/coverage_cases.py builds the scenes that are new here; the
windows, the walk scenes and the long items are tests/hit_frame_cases.py's.

-m gpu: window geometry, the item walk by item count, a full table, long items by chunks per round, occlusion, many tiles on one
record, additivity, output discipline, the argument rules, ordering against frames and scene replacement, the Tiger against
pm_hit_frame and pm_hit_stack, the CLI.
CPU: np_coverage against np_hit.hit_test and np_stack.hit_stack; no case is blind; the -m gpu part against the wave64 emulation of the
kernel; the compiler's listing."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coverage_cases as cc  # noqa: E402
import hit_frame_cases as fc  # noqa: E402
import np_coverage  # noqa: E402
import np_hit  # noqa: E402
import np_stack  # noqa: E402

NONE = cc.NONE
UNTOUCHED = 0x7EADBEEF
DTYPE = np_coverage.DTYPE
GEOMETRY_IDS = [f"{name}-{w}x{h}" for name in fc.REGIONS for w, h in fc.SIZES] + \
               [f"{name}-1x1-{k}" for name in fc.REGIONS for k in range(fc.ITEMS_WANTED[name] + 1)] + \
               [f"{name}-48x40-origin" for name in fc.REGIONS] + ["edge-ends-at-65536", "edge-72x64-origin"]
# geometry, walk, a full table, long items, occlusion, many tiles, more tiles than workgroups, additivity, output discipline, argument
# rules, ordering (2), the Tiger, the CLI
OCCLUSION_IDS = list(cc.OCCLUSION_WINDOWS)
N_GPU_TESTS = len(GEOMETRY_IDS) + len(OCCLUSION_IDS) + len(fc.WALK_SIZES) + len(cc.DENSE_SIZES) + len(fc.LONG_IDS) + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 1 + 1
FLAGS = [(False, False), (True, False), (False, True), (True, True)]   # (skip_transparent, visible_only)


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- the calls --------------------------------------------------------------------------------------------------------

def _flags(pm, skip, visible_only):
    return (pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0) | (pm._lib.PM_COVERAGE_VISIBLE_ONLY if visible_only else 0)


def device_coverage(pm, r, rect, skip=False, visible_only=False, extra=0, stream=None):
    """pm_item_coverage_device into n_items + extra records filled with UNTOUCHED: [n_items + extra, 4], not waited for.  Under the
    emulation device memory is host memory and the array is numpy's; on the GPU it is torch's and goes through
    Renderer.item_coverage_tensor."""
    x0, y0, w, h = rect
    n = r.stats()["n_items"] + extra
    if _emulated():
        out = np.full((n, 4), UNTOUCHED, np.uint32)
        pm._lib.check(pm._lib.load().pm_item_coverage_device(r._h, x0, y0, w, h, _flags(pm, skip, visible_only), out.ctypes.data, n, None),
                      "pm_item_coverage_device")
        return out
    import torch

    out = torch.full((n, 4), UNTOUCHED, dtype=torch.int32, device="cuda")
    torch.cuda.current_stream().synchronize()   # (torch fills on ITS stream: the call's first kernel, the records' initial value, must not overtake the fill)
    r.item_coverage_tensor(out, x0=x0, y0=y0, w=w, h=h, stream=stream, skip_transparent=skip, visible_only=visible_only)
    return out


def as_records(a):
    """DTYPE [m] of an [m, 4] array of words, numpy's or torch's."""
    a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4).copy().view(DTYPE).reshape(-1)


def differing(got, want):
    bad = np.flatnonzero(got != want)
    return [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:8]]


def check_case(pm, r, case, flags=FLAGS):
    """Host and device under every pair of flags: the bytes of np_coverage's records.  Returns the expectation without a flag."""
    x0, y0, w, h = case.rect
    for skip, vis in flags:
        want = case.expected(skip, vis)
        got = r.item_coverage(x0, y0, w, h, skip_transparent=skip, visible_only=vis)
        assert got.dtype == DTYPE and got.tobytes() == want.tobytes(), (case, skip, vis, differing(got, want))
        dev = device_coverage(pm, r, case.rect, skip, vis)
        r.sync()
        dev = as_records(dev)
        assert dev.tobytes() == want.tobytes(), (case, skip, vis, "device", differing(dev, want))
    return case.expected()


def order_holds(rec):
    return bool((rec["top"] <= rec["visible"]).all() and (rec["visible"] <= rec["covered"]).all() and
                ((rec["visible"] == 0) == (rec["first_visible"] == NONE)).all())


@pytest.fixture(scope="module")
def cov_renderer(pm):
    """Never resized: coverage counts need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ident", GEOMETRY_IDS + OCCLUSION_IDS)
def test_window_geometry(pm, pmo, cov_renderer, ident):
    """Windows of one pixel, one tile, one pixel more than a tile in either direction, 33 x 18 at an origin that is no multiple of 16,
    and the two ends of what a u16 box can say: where a partial tile's threads can be miscounted.  hit_frame_cases' windows, and their
    sizes again over the occlusion scene, where every window holds items on top of each other."""
    if ident in cc.OCCLUSION_WINDOWS:
        case = cc.occlusion_window(pm, ident)
    else:
        case = cc.of_window({w.ident: w for w in fc.geometry_windows(pm, pmo)}[ident])
    cov_renderer.set_scene_bytes(case.scene)
    want = check_case(pm, cov_renderer, case)
    assert order_holds(want) and want["covered"].sum() == case.members().sum()


@pytest.mark.gpu
@pytest.mark.parametrize("n", fc.WALK_SIZES)
def test_item_walk_by_item_count(pm, cov_renderer, n):
    """One item fewer than a step of the walk, a step, one more, two steps and one: every item has a record, and every one is seen."""
    case = cc.of_window(fc.walk_window(pm, n))
    r = cov_renderer
    r.set_scene_bytes(case.scene)
    assert r.stats()["n_items"] == n
    want = check_case(pm, r, case)
    assert len(want) == n and (want["top"] > 0).all() and (want["visible"] < want["covered"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", cc.DENSE_SIZES)
def test_a_step_that_fills_the_table(pm, cov_renderer, n):
    """One tile whose first step has as many survivors as the LDS table has rows; with one item more, the bottom item is alone in a
    second step of the same tile."""
    case = cc.dense_case(pm, n)
    cov_renderer.set_scene_bytes(case.scene)
    want = check_case(pm, cov_renderer, case)
    assert (want["covered"] > 0).all() and len(want) == n


@pytest.mark.gpu
@pytest.mark.parametrize("ident", fc.LONG_IDS)
def test_long_item_by_chunks_per_round(pm, cov_renderer, ident):
    """A long Fill / compound Fill / Polyline of one chunk fewer than a round, a round, one more, two rounds and one."""
    wdw = fc.long_window(pm, ident)
    case = cc.of_window(wdw)
    cov_renderer.set_scene_bytes(case.scene)
    want = check_case(pm, cov_renderer, case, flags=[(False, False), (False, True)])
    assert want["covered"][wdw.facts["long_item"]] >= 16


@pytest.mark.gpu
def test_occlusion(pm, cov_renderer):
    """Every class of item below and above an opaque one.  The alpha-0 Fills are covered and visible and occlude nothing without the
    skip, and are all zeros and PM_HIT_NONE with it; the sums are pm_hit_frame's on the same window."""
    case = cc.occlusion_case(pm)
    r = cov_renderer
    r.set_scene_bytes(case.scene)
    check_case(pm, r, case)
    x0, y0, w, h = case.rect
    kinds = cc.item_classes(case.scene)
    clear = [i for i, k in enumerate(kinds) if k == "fill0"]
    for skip in (False, True):
        got = r.item_coverage(x0, y0, w, h, skip_transparent=skip)
        top, cnt = r.hit_frame(x0, y0, w, h, skip_transparent=skip, counts=True)
        assert order_holds(got)
        assert int(got["top"].sum()) == int((top != NONE).sum()) and int(got["covered"].sum()) == int(cnt.sum())
        assert np.array_equal(got["top"], np.bincount(top[top != NONE], minlength=len(got)))
        for i in clear:
            if skip:
                assert got[i].tolist() == (0, 0, 0, NONE)
            else:
                assert got["covered"][i] > 0 and got["visible"][i] > 0
    # an alpha-0 Fill occludes nothing: without it (skipped) the others' visible counts are what they are with it
    a, b = r.item_coverage(x0, y0, w, h), r.item_coverage(x0, y0, w, h, skip_transparent=True)
    others = [i for i in range(len(a)) if i not in clear]
    assert np.array_equal(a["visible"][others], b["visible"][others]) and np.array_equal(a["covered"][others], b["covered"][others])
    assert np.array_equal(r.hidden_items(x0, y0, w, h), np.flatnonzero(case.expected()["visible"] == 0))


@pytest.mark.gpu
def test_many_tiles_add_to_one_record(pm, cov_renderer):
    """One opaque Fill over a 128 x 128 window: 64 tiles contend for one record; the items below it are covered and not seen."""
    case = cc.lid_case(pm)
    r = cov_renderer
    r.set_scene_bytes(case.scene)
    check_case(pm, r, case)
    x0, y0, w, h = case.rect
    got = r.item_coverage(x0, y0, w, h)
    assert got[-1].tolist() == (16384, 16384, 16384, 0)
    assert (got["visible"][:-1] == 0).all() and (got["covered"][:-1] > 0).all() and (got["first_visible"][:-1] == NONE).all()
    only = r.item_coverage(x0, y0, w, h, visible_only=True)
    assert only[-1].tolist() == (16384, 16384, 16384, 0) and (only[:-1].view(np.uint32).reshape(-1, 4) == (0, 0, 0, NONE)).all()
    assert np.array_equal(r.hidden_items(x0, y0, w, h), np.arange(len(got) - 1))


@pytest.mark.gpu
def test_more_tiles_than_workgroups(pm, cov_renderer):
    """4096 tiles on a grid of at most 2048 workgroups: the tile loop moves on, and the table a workgroup used for its first tile
    serves its second."""
    case = cc.strip_case(pm)
    cov_renderer.set_scene_bytes(case.scene)
    want = check_case(pm, cov_renderer, case)
    assert (want["covered"] > 0).all()


@pytest.mark.gpu
def test_counts_add_up_over_disjoint_windows(pm, cov_renderer):
    """A 50 x 37 window cut in four at no multiple of 16: the counts add up, and the whole's first_visible is the smallest of the
    parts', mapped back to the whole's indexing."""
    case = cc.occlusion_case(pm)
    r = cov_renderer
    r.set_scene_bytes(case.scene)
    X0, Y0, W, H = case.rect
    for skip, vis in FLAGS:
        whole = r.item_coverage(X0, Y0, W, H, skip_transparent=skip, visible_only=vis)
        assert whole.tobytes() == case.expected(skip, vis).tobytes()
        total = np.zeros((len(whole), 3), np.uint64)
        first = np.full(len(whole), NONE, np.uint64)
        for x0, y0, w, h in cc.quarters(case.rect, cc.OCCLUSION_CUTS):
            part = r.item_coverage(x0, y0, w, h, skip_transparent=skip, visible_only=vis)
            total += np.stack([part["covered"], part["visible"], part["top"]], axis=1).astype(np.uint64)
            f = part["first_visible"].astype(np.uint64)
            seen = part["first_visible"] != NONE
            mapped = (f // max(w, 1) + (y0 - Y0)) * W + f % max(w, 1) + (x0 - X0)
            first = np.where(seen, np.minimum(first, mapped), first)
        assert np.array_equal(total, np.stack([whole["covered"], whole["visible"], whole["top"]], axis=1).astype(np.uint64)), (skip, vis)
        assert np.array_equal(first, whole["first_visible"].astype(np.uint64)), (skip, vis)
    assert (whole["visible"] > 0).sum() >= 6


@pytest.mark.gpu
def test_output_discipline(pm, cov_renderer):
    """Records beyond n_items keep their bytes; cap = n_items - 1 is PM_ERR_CAPACITY with *n_items set and no word written; two calls
    into one buffer give the same bytes; an empty rectangle writes the zero records."""
    import ctypes as C

    case = cc.occlusion_case(pm)
    r = cov_renderer
    r.set_scene_bytes(case.scene)
    lib = pm._lib.load()
    x0, y0, w, h = case.rect
    n = r.stats()["n_items"]
    want = case.expected().view(np.uint32).reshape(n, 4)
    zero = np.tile(np.array([0, 0, 0, NONE], np.uint32), (n, 1))
    # the host call
    out = np.full((n + 3, 4), UNTOUCHED, np.uint32)
    got_n = C.c_uint32(0xABCD)
    assert lib.pm_item_coverage(r._h, x0, y0, w, h, 0, out.ctypes.data, n + 3, C.byref(got_n)) == pm._lib.PM_OK and got_n.value == n
    assert np.array_equal(out[:n], want) and (out[n:] == UNTOUCHED).all()
    assert lib.pm_item_coverage(r._h, x0, y0, w, h, 0, out.ctypes.data, n, None) == pm._lib.PM_OK   # a second call: no accumulation
    assert np.array_equal(out[:n], want) and (out[n:] == UNTOUCHED).all()
    out[:] = UNTOUCHED
    got_n = C.c_uint32(0xABCD)
    assert lib.pm_item_coverage(r._h, x0, y0, w, h, 0, out.ctypes.data, n - 1, C.byref(got_n)) == pm._lib.PM_ERR_CAPACITY
    assert got_n.value == n and (out == UNTOUCHED).all()
    for rect in ((x0, y0, 0, h), (x0, y0, w, 0), (0, 0, 0, 0), (65536, 65536, 0, 0)):
        out[:] = UNTOUCHED
        assert lib.pm_item_coverage(r._h, *rect, 0, out.ctypes.data, n, None) == pm._lib.PM_OK
        assert np.array_equal(out[:n], zero) and (out[n:] == UNTOUCHED).all()
    # the device call
    dev = device_coverage(pm, r, case.rect, extra=3)
    r.sync()
    first = as_records(dev).view(np.uint32).reshape(-1, 4)
    assert np.array_equal(first[:n], want) and (first[n:] == UNTOUCHED).all()
    if _emulated():
        ptr, again = dev.ctypes.data, lambda: dev   # noqa: E731
    else:
        ptr, again = dev.data_ptr(), lambda: dev.cpu().numpy().view(np.uint32)   # noqa: E731
    assert lib.pm_item_coverage_device(r._h, x0, y0, w, h, 0, ptr, n, None) == pm._lib.PM_OK         # into the same buffer
    r.sync()
    assert np.array_equal(again(), first)
    assert lib.pm_item_coverage_device(r._h, x0, y0, 0, h, 0, ptr, n + 3, None) == pm._lib.PM_OK     # an empty rectangle
    r.sync()
    assert np.array_equal(again()[:n], zero) and (again()[n:] == UNTOUCHED).all()
    assert lib.pm_item_coverage_device(r._h, x0, y0, w, h, 0, ptr, n - 1, None) == pm._lib.PM_ERR_CAPACITY
    r.sync()
    assert np.array_equal(again()[:n], zero) and (again()[n:] == UNTOUCHED).all()


@pytest.mark.gpu
def test_argument_rules(pm, pmo):
    """Everything the calls refuse, before anything is enqueued; PM_COVERAGE_VISIBLE_ONLY is nobody else's flag."""
    lib = pm._lib.load()
    OK, INVALID = pm._lib.PM_OK, pm._lib.PM_ERR_INVALID
    SKIP, STOP, ONLY = pm._lib.PM_HIT_SKIP_TRANSPARENT, pm._lib.PM_HIT_STOP_AT_OPAQUE, pm._lib.PM_COVERAGE_VISIBLE_ONLY
    assert ONLY not in (SKIP, STOP, pm._lib.PM_SNAP_VERTICES, pm._lib.PM_SNAP_EDGES) and ONLY & (ONLY - 1) == 0
    with pm.Renderer(0) as r:
        buf = np.full((16, 4), UNTOUCHED, np.uint32)
        if _emulated():
            dbuf, dptr, dwords = buf, buf.ctypes.data, lambda: buf   # noqa: E731
        else:
            import torch

            dbuf = torch.full((16, 4), UNTOUCHED, dtype=torch.int32, device="cuda")
            dptr, dwords = dbuf.data_ptr(), lambda: dbuf.cpu().numpy().view(np.uint32)   # noqa: E731
        host = lambda x0, y0, w, h, flags, p=buf.ctypes.data, cap=16: lib.pm_item_coverage(r._h, x0, y0, w, h, flags, p, cap, None)       # noqa: E731
        dev = lambda x0, y0, w, h, flags, p=dptr, cap=16: lib.pm_item_coverage_device(r._h, x0, y0, w, h, flags, p, cap, None)           # noqa: E731
        for call in (host, dev):
            assert call(0, 0, 4, 4, 0) == INVALID                         # no scene
        r.set_scene_bytes(pmo.scene_path_test())
        n = r.stats()["n_items"]
        assert 1 <= n <= 16
        for call in (host, dev):
            assert call(0, 0, 4, 4, 2) == INVALID                         # unknown flag bits
            assert call(0, 0, 4, 4, 4) == INVALID
            assert call(0, 0, 4, 4, STOP) == INVALID                      # the stack calls' flag is not this call's
            assert call(0, 0, 4, 4, 0x80000000 | ONLY) == INVALID
            assert call(65533, 0, 4, 4, 0) == INVALID                     # x0 + w > 65 536
            assert call(0, 65533, 4, 4, 0) == INVALID                     # y0 + h > 65 536
            assert call(0xFFFFFFFF, 0, 2, 2, 0) == INVALID                # (no wrap-around in 32 bits)
            assert call(0, 0, 2, 0xFFFFFFFF, 0) == INVALID
            assert call(0, 0, 65536, 65536, 0) == INVALID                 # 2^32 pixels: one more than a count holds
            assert call(0, 0, 4, 4, 0, None) == INVALID                   # no out
            r.sync()
            assert (buf == UNTOUCHED).all() and (dwords() == UNTOUCHED).all()
        assert dev(0, 0, 4, 4, 0, dptr + 2) == INVALID                    # a misaligned dev_out
        r.sync()
        assert (dwords() == UNTOUCHED).all()
        assert host(65532, 65532, 4, 4, SKIP | ONLY) == OK                # the last pixels there are, every flag there is
        assert (buf[:n] == (0, 0, 0, NONE)).all() and (buf[n:] == UNTOUCHED).all()
        # the flag is refused by the calls it is not a flag of
        xy = np.array([[1.5, 1.5]], np.float32)
        top = np.full((4, 4), UNTOUCHED, np.uint32)
        assert lib.pm_hit_frame(r._h, 0, 0, 4, 4, ONLY, top.ctypes.data, None, 4) == INVALID
        assert lib.pm_hit_test(r._h, xy.ctypes.data, 1, ONLY, top.ctypes.data, None) == INVALID
        assert lib.pm_hit_stack(r._h, xy.ctypes.data, 1, 4, ONLY, top.ctypes.data, None) == INVALID
        assert lib.pm_hit_stack(r._h, xy.ctypes.data, 1, 4, STOP | ONLY, top.ctypes.data, None) == INVALID
        assert (top == UNTOUCHED).all()
        assert lib.pm_abi_version() == 600
        # the Python wrappers
        with pytest.raises(ValueError):
            r.item_coverage(0, 0, 65537, 1)
        with pytest.raises(ValueError):
            r.item_coverage(-1, 0, 4, 4)
        with pytest.raises(ValueError):
            r.item_coverage(0, 0, 65536, 65536)
        with pytest.raises(TypeError):
            r.item_coverage(0.5, 0, 4, 4)
        empty = r.item_coverage(3, 3, 0, 5)
        assert empty.dtype == DTYPE and len(empty) == n and (empty.view(np.uint32).reshape(n, 4) == (0, 0, 0, NONE)).all()
        assert len(r.hidden_items(3, 3, 0, 5)) == n
        if not _emulated():
            import torch

            with pytest.raises(TypeError):
                r.item_coverage_tensor(torch.zeros((16, 4), dtype=torch.int32), w=4, h=4)               # not on the device
            with pytest.raises(TypeError):
                r.item_coverage_tensor(torch.zeros((16, 4), dtype=torch.float32, device="cuda"), w=4, h=4)
            with pytest.raises(TypeError):
                r.item_coverage_tensor(torch.zeros((16, 3), dtype=torch.int32, device="cuda"), w=4, h=4)
            with pytest.raises(TypeError):
                r.item_coverage_tensor(dbuf[:, :2], w=4, h=4)
            with pytest.raises(ValueError):
                r.item_coverage_tensor(dbuf, x0=65530, w=8, h=1)
            with pytest.raises(pm.PietMetalError):
                r.item_coverage_tensor(dbuf[: n - 1], w=4, h=4)                                          # PM_ERR_CAPACITY


@pytest.mark.gpu
def test_coverage_between_frames_leaves_the_frames_alone(pm, pmo):
    """Frames rendered before and after a device-variant call have the bytes they have without it."""
    wl = pm.workloads.tiger(160, 90)
    with pm.Renderer(0) as r:
        r.resize(wl.width, wl.height)
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        want = pmo.render(r.download_scene(), wl.width, wl.height)
        r.render()
        dev = device_coverage(pm, r, (0, 0, wl.width, wl.height))   # behind the frame, not waited for
        first = r.read_pixels()
        r.render()
        host = r.item_coverage(0, 0, wl.width, wl.height)
        second = r.read_pixels()
        assert np.array_equal(first, want) and np.array_equal(second, want)
        assert as_records(dev).tobytes() == host.tobytes() and host["covered"].sum() > 0
        top = r.hit_frame(0, 0, wl.width, wl.height)
        assert np.array_equal(host["top"], np.bincount(top[top != NONE], minlength=len(host)))


@pytest.mark.gpu
def test_coverage_answers_for_the_scene_resident_at_the_call(pm):
    """A device-variant call on a side stream, then at once another scene: the records are the first scene's, the next ones the
    second's."""
    a, b = cc.occlusion_case(pm), cc.lid_case(pm)
    with pm.Renderer(0) as r:
        r.set_scene_bytes(a.scene)
        if _emulated():
            s = None
        else:
            import torch

            s = torch.cuda.Stream()
        got_a = device_coverage(pm, r, a.rect, stream=s)
        r.set_scene_bytes(b.scene)
        got_b = device_coverage(pm, r, b.rect, stream=s)
        r.sync()
        if s is not None:
            s.synchronize()
        assert as_records(got_a).tobytes() == a.expected().tobytes()
        assert as_records(got_b).tobytes() == b.expected().tobytes()


def _stack_members(pm, r, w, h, n_items):
    """Per item the number of the w x h pixel centres from (0, 0) whose pm_hit_stack answer, with PM_HIT_STOP_AT_OPAQUE and k = 256,
    holds it; and the longest stack."""
    q = fc.centres(0, 0, w, h)
    if _emulated():
        items, cnt = r.hit_stack(q, 256, stop_at_opaque=True, counts=True)
    else:
        import torch

        xy = torch.from_numpy(q).cuda()
        items = torch.empty((w * h, 256), dtype=torch.int32, device="cuda")
        cnt = torch.empty(w * h, dtype=torch.int32, device="cuda")
        r.hit_stack_tensor(xy, items, cnt, stop_at_opaque=True)
        r.sync()
        items, cnt = items.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    return np.bincount(items[items != NONE], minlength=n_items), int(cnt.max())


@pytest.mark.gpu
def test_the_tiger_against_the_item_map_and_the_stacks(pm):
    """The Tiger flattened on the device at 240 x 135, against the device: top is the histogram of pm_hit_frame's map, covered sums
    to its n_hit, visible is the membership count of pm_hit_stack's answers under PM_HIT_STOP_AT_OPAQUE -- on a view that has items
    that are covered and never seen, and no stack longer than pm_hit_stack can return."""
    W, H = cc.TIGER_VIEW
    wl = pm.workloads.tiger(W, H)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        n = r.stats()["n_items"]
        got = r.item_coverage(0, 0, W, H)
        dev = device_coverage(pm, r, (0, 0, W, H))
        only = device_coverage(pm, r, (0, 0, W, H), visible_only=True)
        r.sync()
        assert as_records(dev).tobytes() == got.tobytes()
        only = as_records(only)
        assert np.array_equal(only["visible"], got["visible"]) and np.array_equal(only["covered"], got["visible"])
        assert np.array_equal(only["top"], got["top"]) and np.array_equal(only["first_visible"], got["first_visible"])
        top, cnt = r.hit_frame(0, 0, W, H, counts=True)
        assert np.array_equal(got["top"], np.bincount(top[top != NONE], minlength=n))
        assert int(got["covered"].sum()) == int(cnt.sum())
        assert order_holds(got)
        members, longest = _stack_members(pm, r, W, H, n)
        hidden = np.flatnonzero((got["covered"] > 0) & (got["visible"] == 0))
        assert longest <= 256 and len(hidden) >= 1, (longest, len(hidden))
        assert np.array_equal(got["visible"], members)
        # first_visible is a pixel that shows the item and the first such
        for i in np.flatnonzero(got["visible"])[:: max(1, n // 16)]:
            f = int(got["first_visible"][i])
            stack = r.hit_stack(np.array([[f % W + 0.5, f // W + 0.5]], np.float32), 256, stop_at_opaque=True)
            assert i in stack[0]
        assert set(r.hidden_items(0, 0, W, H).tolist()) == set(np.flatnonzero(got["visible"] == 0).tolist())


SVG = """<svg xmlns="http://www.w3.org/2000/svg" width="32" height="32" viewBox="0 0 32 32">
<path d="M4 4H12V12H4Z" fill="#ff0000"/>
<path d="M2 2H20V20H2Z" fill="#00ff00"/>
<path d="M16 16H30V30H16Z" fill="#0000ff" fill-opacity="0.5"/>
<path d="M40 40H50V50H40Z" fill="#000000"/>
</svg>
"""


@pytest.mark.gpu
def test_cli_coverage_and_hidden(pm, tmp_path, capsys):
    """--coverage and --hidden on four squares: one under an opaque one, one translucent over its corner, one outside the view."""
    from piet_metal_amd import cli

    src = tmp_path / "squares.svg"
    src.write_text(SVG)
    assert cli.main([str(src), str(tmp_path / "s.png"), "--width", "32", "--height", "32", "--scale", "1", "--offset", "0", "0", "--coverage", "--hidden"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert lines == [
        "item 0 path 0: covered 64 visible 0 top 0 first_visible none",
        "item 1 path 1: covered 324 visible 324 top 308 first_visible 2,2",
        "item 2 path 2: covered 196 visible 196 top 196 first_visible 16,16",
        "hidden: 0 3",
    ]


# ---- CPU: the reference against independent restatements --------------------------------------------------------------------

def _cpu_cases(pm, pmo):
    wins = {w.ident: w for w in fc.geometry_windows(pm, pmo)}
    return [cc.occlusion_case(pm), cc.dense_case(pm, cc.DENSE_SIZES[1]), cc.lid_case(pm), cc.of_window(wins["mixed-33x18"]),
            cc.of_window(wins["edge-ends-at-65536"]), cc.of_window(fc.centres_window(pm))]


def test_the_reference_top_is_the_histogram_of_np_hit(pm, pmo):
    for case in _cpu_cases(pm, pmo):
        for skip in (False, True):
            top, cnt = np_hit.hit_test(case.scene, fc.centres(*case.rect), skip)
            want = case.expected(skip)
            assert np.array_equal(want["top"], np.bincount(top[top != NONE], minlength=len(want))), (case, skip)
            assert int(want["covered"].sum()) == int(cnt.sum()) and order_holds(want), (case, skip)
            only = case.expected(skip, True)
            assert np.array_equal(only["covered"], want["visible"]) and np.array_equal(only["visible"], want["visible"])
            assert np.array_equal(only["top"], want["top"]) and np.array_equal(only["first_visible"], want["first_visible"])


def test_the_reference_visible_is_the_membership_of_np_stack(pm, pmo):
    for case in _cpu_cases(pm, pmo):
        if case.ident.startswith("dense"):
            continue   # (up to 257 items under a pixel: more than a stack returns; the test below says so)
        H = np_coverage.members(case.scene, case.rect)     # no flag: np_stack applies the skip itself
        for skip in (False, True):
            items, cnt = np_stack.hit_stack(case.scene, None, np_stack.STACK_MAX, skip, True, members=H)
            assert cnt.max() <= np_stack.STACK_MAX, case
            want = case.expected(skip)
            assert np.array_equal(want["visible"], np.bincount(items[items != NONE], minlength=len(want))), (case, skip)
            for i in np.flatnonzero(want["visible"]):   # the first pixel, row by row, whose stack holds the item
                assert want["first_visible"][i] == np.flatnonzero((items == i).any(axis=1))[0], (case, skip, i)


# ---- CPU: no case is blind -------------------------------------------------------------------------------------------------------

def test_no_geometry_window_is_blind(pm, pmo):
    """Every window has an item that is partly occluded, 0 < visible < covered, or cannot have one: no pixel of it lies in two items
    (hit_frame_cases places its windows over two items and some nothing, not over items on top of each other; edge_scene's items and
    the oracle's one Fill overlap nowhere in their windows), or it is one pixel.  The windows over the occlusion scene all have one."""
    wins = fc.geometry_windows(pm, pmo)
    assert sorted(w.ident for w in wins) == sorted(GEOMETRY_IDS)
    partly = []
    for case in [cc.of_window(w) for w in wins] + [cc.occlusion_window(pm, i) for i in OCCLUSION_IDS]:
        want = case.expected()
        if ((want["visible"] > 0) & (want["visible"] < want["covered"])).any():
            partly.append(case.ident)
        else:
            assert case.rect[2:] == (1, 1) or case.members().sum(axis=0).max() <= 1, case
    assert {"mixed-17x1", "mixed-33x18", "mixed-48x40-origin"} <= set(partly) and set(OCCLUSION_IDS) <= set(partly), partly
    for ident in OCCLUSION_IDS:   # ... and each has a covered pixel in its LAST tile, the partial one
        case = cc.occlusion_window(pm, ident)
        x0, y0, w, h = case.rect
        depth = case.members().sum(axis=0).reshape(h, w)
        assert depth[(h - 1) // 16 * 16 :, (w - 1) // 16 * 16 :].max() >= 1 and x0 % 16 and y0 % 16, ident


def test_the_occlusion_scene_has_every_class_below_and_above_an_opaque_item(pm):
    case = cc.occlusion_case(pm)
    kinds = cc.item_classes(case.scene)
    assert set(kinds) == set(cc.OCCLUSION_CLASSES)
    H = case.members()
    alpha, _ = np_stack.item_alphas(case.scene)
    opaque = np.flatnonzero(alpha == 255)
    below, above = set(), set()
    for i, kind in enumerate(kinds):
        if any(j > i and (H[i] & H[j]).any() for j in opaque):
            below.add(kind)
        if any(j < i and (H[i] & H[j]).any() for j in opaque):
            above.add(kind)
    assert below == set(cc.OCCLUSION_CLASSES) and above == set(cc.OCCLUSION_CLASSES), (below, above)
    want = case.expected()
    assert ((want["visible"] > 0) & (want["visible"] < want["covered"])).sum() >= 6
    assert ((want["top"] > 0) & (want["top"] < want["visible"])).any()      # seen through a translucent item
    assert (want["first_visible"][want["visible"] > 0] > 0).any()
    # the window is cut where no tile ends, and every quarter holds something
    assert all(c % 16 for c in cc.OCCLUSION_CUTS) and case.rect[0] % 16 and case.rect[1] % 16
    for x0, y0, w, h in cc.quarters(case.rect, cc.OCCLUSION_CUTS):
        assert np_coverage.coverage(case.scene, (x0, y0, w, h))["visible"].sum() > 0


@pytest.mark.parametrize("n", cc.DENSE_SIZES)
def test_the_dense_scenes_fill_the_table(pm, n):
    """All n items survive the cull of the window's one tile: ITEMS_PER_STEP of them in the first step, the rest in the second."""
    case = cc.dense_case(pm, n)
    assert case.rect[2:] == (cc.TILE, cc.TILE) and len(np_hit.flat_items(bytes(case.scene))) == n
    steps = cc.step_survivors(case.scene, case.rect)
    assert steps == ([cc.ITEMS_PER_STEP] if n == cc.ITEMS_PER_STEP else [cc.ITEMS_PER_STEP, n - cc.ITEMS_PER_STEP]), steps
    assert cc.step_survivors(case.scene, case.rect, skip=True)[0] < cc.ITEMS_PER_STEP     # (the alpha-0 items leave under the skip)
    want = case.expected()
    assert (want["covered"] > 0).all() and len(set(map(tuple, want.tolist()))) > n // 4   # the records differ
    assert (want["visible"] == 0).any() and ((want["visible"] > 0) & (want["visible"] < want["covered"])).any()
    assert "s_acc[kFrameItems * kCoverageWords]" in open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_coverage.h")).read()


def test_the_strip_has_more_tiles_than_the_grid_has_workgroups(pm):
    """Workgroup 0's two tiles, 0 and GRID_MAX, both hold hits, and different ones."""
    case = cc.strip_case(pm)
    x0, y0, w, h = case.rect
    n_tiles = -(-w // cc.TILE) * -(-h // cc.TILE)
    assert n_tiles == 2 * cc.GRID_MAX
    assert "max(n_cus, 1u) * 8u" in open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_coverage.h")).read()
    H = case.members().reshape(-1, h, w)
    first, second = H[:, :, : cc.TILE].any(axis=(1, 2)), H[:, :, cc.GRID_MAX * cc.TILE : (cc.GRID_MAX + 1) * cc.TILE].any(axis=(1, 2))
    assert first.sum() >= 2 and second.sum() >= 3 and (first != second).any(), (first, second)
    assert H[:, :, -cc.TILE :].any() and order_holds(case.expected())


def test_the_lid_covers_every_tile(pm):
    case = cc.lid_case(pm)
    want = case.expected()
    assert want[-1].tolist() == (128 * 128, 128 * 128, 128 * 128, 0) and (want["visible"][:-1] == 0).all() and (want["covered"][:-1] > 0).all()
    assert case.rect[2] // cc.TILE * (case.rect[3] // cc.TILE) == 64


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_coverage_under_wave64_emulation(built):
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

# pm_hit_frame_kernel at commit 90bc3a1 (the parent of the commit that added pm_coverage.h), by the same flags: this file's kernel is
# built from its pieces and must leave it as it was
PARENT_HIT_FRAME = dict(vgpr=60, lds=3120, scratch=0)


def test_the_coverage_kernel_uses_no_scratch(tmp_path):
    """pm_item_coverage_kernel by the flags the library is built with: no private segment, at most 128 VGPRs (four workgroups of 256
    threads per CU) and at most 16 384 bytes of LDS (eight such workgroups stay inside a CU's 160 KB); and pm_hit_frame_kernel, whose
    pieces it shares, has the figures it had before.  The figures are printed (pytest -s) and stand in DESIGN.md 4."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not shutil.which(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "piet_metal_amd", "csrc")
    mk = open(os.path.join(src, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("$(HERE)", src + "/").replace("$(EXTRA)", "").split()
    out = str(tmp_path / "pm_context.s")
    subprocess.check_call([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(src, "pm_context.hip"), "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        name = next((k for k in ("pm_item_coverage_kernel", "pm_hit_frame_kernel") if k in m.group(1)), None)
        if name is None:
            continue
        assert name not in found
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
        occ = re.search(re.escape(m.group(1)) + r".*?; Occupancy: (\d+)", text, re.S)
        print(f"{name}: {vgpr} VGPRs, {lds} bytes of LDS, scratch {scratch}, occupancy {occ.group(1) if occ else '?'} waves per SIMD")
        found[name] = dict(vgpr=vgpr, lds=lds, scratch=scratch)
    assert set(found) == {"pm_item_coverage_kernel", "pm_hit_frame_kernel"}
    mine = found["pm_item_coverage_kernel"]
    assert mine["scratch"] == 0 and mine["vgpr"] <= 128 and mine["lds"] <= 16384, mine
    assert found["pm_hit_frame_kernel"] == PARENT_HIT_FRAME, found["pm_hit_frame_kernel"]
