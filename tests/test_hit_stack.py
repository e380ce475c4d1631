"""Hit stacks (decision D24): pm_hit_stack / pm_hit_rects_stack -- the k topmost items under a point or a rectangle,
topmost first, and the length of the whole stack.

-m gpu: every word EQUAL to tests/np_stack.py, no tolerance -- the walk scenes of tests/hit_structure.py (depths past 64 and 128) at
k on either side of the 64-item step and of the stack's own length, the alpha patterns of tests/stack_cases.py under
PM_HIT_STOP_AT_OPAQUE, long items, the rectangle variant with pick squares, k = 1 against the device's own pm_hit_test and
pm_hit_rects, output arrays too long whose tail must survive, query counts around the grid, a host call across its batch boundary,
the staging buffer shared with pm_snap and pm_select_rect, every argument error, the CLI's --pick-depth.
CPU: np_stack against hand-derived stacks and against np_hit / np_rect at k = 1; the committed cases are what they claim; the
constants; and the -m gpu part against the wave64 emulation of the kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_scenes as es  # noqa: E402
import hit_structure as hs  # noqa: E402
import np_hit  # noqa: E402
import np_rect  # noqa: E402
import np_stack  # noqa: E402
import stack_cases as stc  # noqa: E402

NONE = np_stack.HIT_NONE
UNTOUCHED = 0x7EADBEEF
KS = (1, 2, 63, 64, 65, 256)
TOLERANCES = (0.0, 0.5, 3.0)
BAD_RECTS = np.array([[np.nan, 40.0, 60.0, 60.0], [60.0, 40.0, 40.0, 60.0]], np.float32)   # a NaN, an inverted one
LONG_IDS = ("meander-85-257-p2-l32-nz", "meander-683-2049-p1-l32-nz")                        # a Fill of 65 chunks, one of 513
STAGE_MAX = 64 << 20    # kStackStageMax (pm_context.hip): the bytes a host call stages at a time
BATCH_TEST = "test_a_host_call_across_its_batch_boundary"
# walk scenes, stack cases, long items, k = 1 on the device, output discipline and the grid, non-finite queries, the batch boundary,
# the shared staging buffer, argument rules, CLI
N_GPU_TESTS = len(hs.WALK_SIZES) + len(stc.CASES) + len(LONG_IDS) + 1 + 1 + 1 + 1 + 1 + 1 + 1
FLAGS = [(False, False), (True, False), (False, True), (True, True)]   # (skip_transparent, stop_at_opaque)


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


def pick_rects(queries):
    """The pick squares of every query at every tolerance, then the two invalid rectangles."""
    return np.concatenate([np_rect.pick_rects(queries, t) for t in TOLERANCES] + [BAD_RECTS])


_MEMBERS = {}


def members(key, scene, q):
    """The membership matrix of a scene's queries (points [n, 2] or rectangles [n, 4]), computed once and left unchanged."""
    q = np.asarray(q, np.float32)
    key = (key, q.shape)
    if key not in _MEMBERS:
        m = np_stack.rect_members(scene, q) if q.shape[1] == 4 else np_stack.point_members(scene, q)
        m.setflags(write=False)
        _MEMBERS[key] = m
    return _MEMBERS[key]


# ---- the calls --------------------------------------------------------------------------------------------------------

def lib_flags(pm, skip, stop):
    return (pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0) | (pm._lib.PM_HIT_STOP_AT_OPAQUE if stop else 0)


def device_stack(pm, r, q, k, skip=False, stop=False, counts=True, pad=0, stream=None):
    """pm_hit_stack_device (q [n, 2]) or pm_hit_rects_stack_device (q [n, 4]) into arrays of n k + pad and n + pad words filled with
    UNTOUCHED: (items, n_hit, keep-alive), not waited for.  Under the emulation device memory is host memory."""
    q = np.ascontiguousarray(q, np.float32)
    n, rect = len(q), q.shape[1] == 4
    if _emulated():
        items, cnt = np.full(n * k + pad, UNTOUCHED, np.uint32), np.full(n + pad, UNTOUCHED, np.uint32)
        lib = pm._lib.load()
        call, name = (lib.pm_hit_rects_stack_device, "pm_hit_rects_stack_device") if rect else (lib.pm_hit_stack_device, "pm_hit_stack_device")
        pm._lib.check(call(r._h, q.ctypes.data, n, k, lib_flags(pm, skip, stop), items.ctypes.data, cnt.ctypes.data if counts else None, None), name)
        return items, cnt, q
    import torch

    dq = torch.from_numpy(q).cuda()
    items = torch.full((n * k + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
    call = r.hit_rects_stack_tensor if rect else r.hit_stack_tensor
    call(dq, items[: n * k].view(n, k), cnt[:n] if counts else None, stream=stream, skip_transparent=skip, stop_at_opaque=stop)
    return items, cnt, dq


def as_u32(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy().view(np.uint32)


def host_stack(r, q, k, skip=False, stop=False, counts=False):
    call = r.hit_rects_stack if np.asarray(q).shape[1] == 4 else r.hit_stack
    return call(q, k, skip_transparent=skip, stop_at_opaque=stop, counts=counts)


def check_stacks(pm, r, scene, q, mem, ks, flag_sets=FLAGS, device_ks=()):
    """Host calls with counts and without for every k and every flag set, the device variant (arrays four words too long) for
    device_ks: every word equal to np_stack's."""
    q = np.ascontiguousarray(q, np.float32)
    n = len(q)
    for skip, stop in flag_sets:
        for k in ks:
            want, want_cnt = np_stack.stack(scene, mem, k, skip, stop)
            items, cnt = host_stack(r, q, k, skip, stop, counts=True)
            bad = np.flatnonzero((items != want).any(axis=1) | (cnt != want_cnt))
            assert bad.size == 0, (k, skip, stop, len(bad), [(q[b].tolist(), items[b][:6].tolist(), want[b][:6].tolist(), int(cnt[b]), int(want_cnt[b])) for b in bad[:4]])
            first = host_stack(r, q, k, skip, stop)   # the walk that may end at its k-th member
            bad = np.flatnonzero((first != want).any(axis=1))
            assert bad.size == 0, (k, skip, stop, "no counts", len(bad), [(q[b].tolist(), first[b][:6].tolist(), want[b][:6].tolist()) for b in bad[:4]])
            if k in device_ks:
                a, ac, keep1 = device_stack(pm, r, q, k, skip, stop, counts=True, pad=4)
                b, bc, keep2 = device_stack(pm, r, q, k, skip, stop, counts=False, pad=4)
                r.sync()
                a, ac, b, bc = as_u32(a), as_u32(ac), as_u32(b), as_u32(bc)
                assert np.array_equal(a[: n * k].reshape(n, k), want) and np.array_equal(ac[:n], want_cnt) and np.array_equal(b[: n * k].reshape(n, k), want), (k, skip, stop)
                assert (a[n * k:] == UNTOUCHED).all() and (ac[n:] == UNTOUCHED).all() and (b[n * k:] == UNTOUCHED).all() and (bc == UNTOUCHED).all(), (k, skip, stop)


# ---- CPU: the constants ------------------------------------------------------------------------------------------------------

def test_constants_agree(pm):
    hdr = open(os.path.join(ROOT, "include", "piet_metal_amd.h")).read()
    got = {k: int(v) for k, v in re.findall(r"^#define (PM_HIT_STOP_AT_OPAQUE|PM_HIT_STACK_MAX|PM_HIT_SKIP_TRANSPARENT|PM_ABI_VERSION) (\d+)u", hdr, re.M)}
    assert got == {"PM_HIT_STOP_AT_OPAQUE": 8, "PM_HIT_STACK_MAX": 256, "PM_HIT_SKIP_TRANSPARENT": 1, "PM_ABI_VERSION": 600}
    assert pm._lib.PM_HIT_STOP_AT_OPAQUE == np_stack.STOP_AT_OPAQUE == 8 and pm._lib.PM_HIT_STACK_MAX == np_stack.STACK_MAX == 256
    assert pm._lib.PM_HIT_SKIP_TRANSPARENT == np_stack.SKIP_TRANSPARENT
    kernels = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_hit_stack.h")).read()
    assert "kHitStopAtOpaque = 8u" in kernels and "kHitStackMax = 256u" in kernels and "hi > 64u ? hi - 64u : 0u" in kernels
    host = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_context.hip")).read()
    assert "kHitBatch = static_cast<size_t>(1) << 22;" in host and "kStackStageMax = kHitBatch * 16;" in host and (1 << 22) * 16 == STAGE_MAX
    assert "PM_HIT_STOP_AT_OPAQUE == pm::kHitStopAtOpaque && PM_HIT_STACK_MAX == pm::kHitStackMax" in host


# ---- CPU: np_stack against stacks derived by hand ---------------------------------------------------------------------------

def hand_scene(pm):
    """Bottom to top: 0 a square [10, 90]^2 of alpha 255; 1 a square [20, 80]^2 of alpha 128; 2 a Circle of radius 20 about (50, 50);
    3 a Line (30, 50) - (70, 50) of width 4 and alpha 0; 4 a Polyline (50, 30) - (50, 70) of width 4 and alpha 254; 5 a square
    [45, 55]^2 of alpha 0."""
    sq = lambda a, b: np.array([[a, a], [b, a], [b, b], [a, b]], np.float64)  # noqa: E731

    def emit(e):
        e.fill(sq(10, 90), 0x112233FF)
        e.fill(sq(20, 80), 0x11223380)
        e.circle((50.0, 50.0), 20.0)
        e.stroke_line((30.0, 50.0), (70.0, 50.0), 4.0, 0x11223300)
        e.polyline(np.array([[50.0, 30.0], [50.0, 70.0]]), 0x112233FE, 4.0)
        e.fill(sq(45, 55), 0x11223300)

    return hs._encode(pm, 6, emit)


# query -> {(skip, stop): the whole stack}
HAND = [
    ((50.0, 50.0), {(False, False): [5, 4, 3, 2, 1, 0], (True, False): [4, 2, 1, 0], (False, True): [5, 4, 3, 2], (True, True): [4, 2]}),
    ((25.0, 25.0), {(False, False): [1, 0], (True, False): [1, 0], (False, True): [1, 0], (True, True): [1, 0]}),
    ((15.0, 15.0), {(False, False): [0], (True, False): [0], (False, True): [0], (True, True): [0]}),
    ((50.0, 68.0), {(False, False): [4, 2, 1, 0], (True, False): [4, 2, 1, 0], (False, True): [4, 2], (True, True): [4, 2]}),
    ((5.0, 5.0), {(False, False): [], (True, False): [], (False, True): [], (True, True): []}),
    ((np.inf, 50.0), {(False, False): [], (True, False): [], (False, True): [], (True, True): []}),
]


def hand_expected(k, skip, stop):
    items = np.full((len(HAND), k), NONE, np.uint32)
    cnt = np.zeros(len(HAND), np.uint32)
    for q, (_, stacks) in enumerate(HAND):
        s = stacks[skip, stop]
        items[q, : min(k, len(s))] = s[:k]
        cnt[q] = len(s)
    return items, cnt


def test_np_stack_against_hand_derived_stacks(pm):
    scene = hand_scene(pm)
    pts = np.array([h[0] for h in HAND], np.float32)
    for skip, stop in FLAGS:
        for k in (1, 3, 4, 6, 8):
            items, cnt = np_stack.hit_stack(scene, pts, k, skip, stop)
            want, want_cnt = hand_expected(k, skip, stop)
            assert np.array_equal(items, want) and np.array_equal(cnt, want_cnt), (k, skip, stop, items.tolist(), want.tolist())
    # a point is the rectangle it degenerates to; a square of half side 6 about (15, 15) reaches the second square too
    for skip, stop in FLAGS:
        items, cnt = np_stack.hit_rects_stack(scene, np_rect.pick_rects(pts[:5], 0.0), 4, skip, stop)
        want, want_cnt = hand_expected(4, skip, stop)
        assert np.array_equal(items, want[:5]) and np.array_equal(cnt, want_cnt[:5])
    items, cnt = np_stack.hit_rects_stack(scene, np_rect.pick_rects(pts[2:3], 6.0), 3, stop_at_opaque=True)
    assert items.tolist() == [[1, 0, NONE]] and cnt.tolist() == [2]


# ---- CPU: k = 1 is hit_test / hit_rects ------------------------------------------------------------------------------------

def _k1_equals(scene, pts, rects, key):
    for skip in (False, True):
        items, cnt = np_stack.hit_stack(scene, pts, 1, skip, members=members(key, scene, pts))
        top, n_hit = np_hit.hit_test(scene, pts, skip)
        assert np.array_equal(items[:, 0], top) and np.array_equal(cnt, n_hit), (key, skip)
        items, cnt = np_stack.hit_rects_stack(scene, rects, 1, skip, members=members(key, scene, rects))
        top, n_hit = np_rect.hit_rects(scene, rects, skip)
        assert np.array_equal(items[:, 0], top) and np.array_equal(cnt, n_hit), (key, skip)
    return cnt


def test_np_stack_at_k1_is_np_hit_and_np_rect(pm):
    for n in hs.WALK_SIZES:
        case = hs.walk_scene(pm, n)
        _k1_equals(case.scene, case.queries, pick_rects(case.queries), ("walk", n))
    for name, (alphas, _) in stc.CASES.items():
        case = stc.stack_scene(pm, alphas)
        _k1_equals(case.scene, case.queries, pick_rects(case.queries), ("stack", name))
    deepest = 0
    for seed in es.SMALL_SEEDS[:12]:
        scene, w, h, _ = es.edge_scene(pm, seed, small=True, n=24)
        rng = np.random.default_rng(seed)
        pts = (rng.uniform(-0.1, 1.1, (200, 2)) * (w, h)).astype(np.float32)
        rects = np.concatenate([np_rect.pick_rects(pts[:100], 2.0), BAD_RECTS])
        deepest = max(deepest, int(_k1_equals(scene, pts, rects, ("edge", seed)).max()))
    assert deepest >= 3


# ---- CPU: the committed cases are what they claim, judged by np_stack alone ---------------------------------------------------

def test_the_stack_cases_are_what_they_claim(pm):
    seen_at_a, seen_at_c, seen_items, kinds, used = set(), set(), set(), set(), set()
    for name, (alphas, at_a) in stc.CASES.items():
        case = stc.stack_scene(pm, alphas)
        n, f = case.facts["n"], case.facts
        used |= set(alphas)
        assert len(np_hit.flat_items(case.scene)) == n
        # at C a Circle is opaque whatever its alpha says
        at_c = next(j for j in range(n) if f["kinds"][n - 1 - j] in ("circle", "ellipse") or alphas[n - 1 - j] == 255)
        mem = members(("stack", name), case.scene, case.queries)
        whole, m = np_stack.stack(case.scene, mem, 256)
        # every item contains C, the items that reach A are the ones the builder names, every spot is private, NOTHING and the NaN are in none
        assert m[f["common"]] == n and whole[f["common"], :n].tolist() == list(range(n - 1, -1, -1))
        assert whole[f["second"], : m[f["second"]]].tolist() == [i for i in range(n - 1, -1, -1) if stc.reaches_a(i)]
        assert (m[:n] == 1).all() and whole[:n, 0].tolist() == list(range(n)), (name, np.flatnonzero(m[:n] != 1)[:8])
        assert m[f["nothing"]] == 0 and m[-1] == 0
        cut, mc = np_stack.stack(case.scene, mem, 256, stop_at_opaque=True)
        for point, claimed, seen in ((f["second"], at_a, seen_at_a), (f["common"], at_c, seen_at_c)):
            if claimed is None:
                assert mc[point] == m[point], name
            else:
                assert mc[point] == claimed + 1 and np.array_equal(cut[point, : claimed + 1], whole[point, : claimed + 1]), (name, point, int(mc[point]))
            seen.add(claimed)
        # under the skip flag the cut moves with the members that are skipped, and is still a cut at an opaque member
        both, mb = np_stack.stack(case.scene, mem, 256, True, True)
        assert (mb <= mc).all() and (mb[f["second"]] < mc[f["second"]] or (at_a is not None and at_a < 3))
        kinds |= {f["kinds"][i] for i in whole[f["common"], :n]}
        if at_a is not None:
            seen_items.add(n - 1 - int(cut[f["second"], at_a]))        # how far below the top item the stack at A ends
        if n == stc.N_MAX:
            assert m[f["common"]] >= 129
    assert {0, 1, 63, 64, 65, None} <= seen_at_a and {0, 1} <= seen_at_c and {63, 64, 65} <= seen_items and used == set(stc.ALPHAS)
    assert kinds == {"fill", "polyline", "line", "circle", "ellipse", "compound"}


# ---- -m gpu -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stack_renderer(pm):
    """Never resized: the queries need a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", hs.WALK_SIZES)
def test_walk_scenes(pm, stack_renderer, n):
    """n items of every kind, the first half in a child group: every query of the scene at k on both sides of the 64-item step, the
    point under all arms also at k = m - 1, m, m + 1 -- where the early end and the PM_HIT_NONE fill meet --, points and pick squares."""
    case = hs.walk_scene(pm, n)
    r, q = stack_renderer, case.queries
    r.set_scene_bytes(case.scene)
    assert r.stats()["n_items"] == n
    mem = members(("walk", n), case.scene, q)
    check_stacks(pm, r, case.scene, q, mem, KS, FLAGS[:2], device_ks=(2, 65))
    common = 2 * n
    for skip in (False, True):
        m = int(np_stack.stack(case.scene, mem, 1, skip)[1][common])
        assert m == len(case.facts["opaque" if skip else "covering"]) and (n < 100 or m > 64) and (n < 200 or m > 128 or skip)
        check_stacks(pm, r, case.scene, q[common:], mem[:, common:], [k for k in (m - 1, m, m + 1) if 1 <= k <= 256], [(skip, False)], device_ks=(m,))
    rects = pick_rects(q)
    check_stacks(pm, r, case.scene, rects, members(("walk", n), case.scene, rects), KS, FLAGS[:2], device_ks=(2, 65))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(stc.CASES))
def test_stack_cases_stop_at_opaque(pm, stack_renderer, name):
    """The alpha patterns: the first opaque member at 0, 1, 63, 64, 65 from the top and nowhere, under PM_HIT_STOP_AT_OPAQUE alone and
    with the skip flag; with counts n_hit is the length after the cut."""
    alphas, at_a = stc.CASES[name]
    case = stc.stack_scene(pm, alphas)
    r, q = stack_renderer, case.queries
    r.set_scene_bytes(case.scene)
    mem = members(("stack", name), case.scene, q)
    ks = sorted({1, 64, 65, 66, 256} | ({at_a, at_a + 1, at_a + 2} - {0} if at_a is not None else set()))
    check_stacks(pm, r, case.scene, q, mem, ks, FLAGS[2:], device_ks=(1, 65))
    check_stacks(pm, r, case.scene, q, mem, (256,), FLAGS[:2])
    rects = pick_rects(q)
    check_stacks(pm, r, case.scene, rects, members(("stack", name), case.scene, rects), ks, FLAGS[2:], device_ks=(1, 65))


@pytest.mark.gpu
@pytest.mark.parametrize("ident", LONG_IDS)
def test_long_items(pm, stack_renderer, ident):
    """A Fill of 65 chunks and one of 513 between a lead and a trailing item: the reused HitFill / RectFill get the right item's chunks."""
    case = dict(hs.structure_cases())[ident](pm)
    r, q = stack_renderer, case.queries[::2]
    r.set_scene_bytes(case.scene)
    mem = members(("long", ident), case.scene, q)
    check_stacks(pm, r, case.scene, q, mem, (3,), FLAGS, device_ks=(3,))
    want, cnt = np_stack.stack(case.scene, mem, 3)
    assert (want[:, 0] == case.long_item).sum() >= case.facts["npt"] // 32 and (cnt == 0).any() and len(set(want[:, 0].tolist())) >= 3
    rects = np_rect.pick_rects(q[::3], 0.5)
    check_stacks(pm, r, case.scene, rects, members(("long", ident), case.scene, rects), (3,), FLAGS[::3], device_ks=(3,))


@pytest.mark.gpu
def test_k1_is_the_devices_own_hit_test_and_hit_rects(pm, stack_renderer):
    """k = 1 without the stop flag: items and n_hit are pm_hit_test's (pm_hit_rects') top_item and n_hit, word for word."""
    r = stack_renderer
    for case in (hs.walk_scene(pm, 129), stc.stack_scene(pm, stc.CASES["at-64"][0])):
        r.set_scene_bytes(case.scene)
        q, rects = case.queries, pick_rects(case.queries)
        for skip in (False, True):
            for with_counts in (True, False):
                items = host_stack(r, q, 1, skip, counts=with_counts)
                top = r.hit_test(q, skip_transparent=skip, counts=with_counts)
                assert np.array_equal(np.ravel(items[0] if with_counts else items), top[0] if with_counts else top) and (not with_counts or np.array_equal(items[1], top[1]))
                items = host_stack(r, rects, 1, skip, counts=with_counts)
                top = r.hit_rects(rects, skip_transparent=skip, counts=with_counts)
                assert np.array_equal(np.ravel(items[0] if with_counts else items), top[0] if with_counts else top) and (not with_counts or np.array_equal(items[1], top[1]))
        assert len(set(r.hit_test(q).tolist())) > 100


@pytest.mark.gpu
def test_output_discipline_and_the_grid(pm, stack_renderer):
    """1 ... 7 queries and one either side of what the grid holds at once (32 per CU), k = 3, into arrays four words too long whose
    tail must stay as it was -- a short list repeated, so that a stride error is a wrong VALUE."""
    case = hs.walk_scene(pm, 5)
    r = stack_renderer
    r.set_scene_bytes(case.scene)
    spots = case.queries[:5]
    short = np.concatenate([spots[:1], [hs.COMMON, hs.NOTHING, (np.nan, 10.0)], spots[4:5], [hs.ARMS_ONLY], spots[1:2]]).astype(np.float32)
    short_rects = np.concatenate([np_rect.pick_rects(short[:5], 3.0), BAD_RECTS])
    want = np_stack.hit_stack(case.scene, short, 3)
    assert want[1].max() >= 3 and 0 in want[1] and NONE in want[0] and (want[0][:, 2] != NONE).any()
    if _emulated():
        cus = int(os.environ.get("PM_EMU_CUS", "256"))  # (what the emulated device reports)
    else:
        import torch

        cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n in [1, 2, 3, 4, 5, 7, 32 * cus - 1, 32 * cus, 32 * cus + 1]:
        reps = -(-n // len(short))
        for base in (short, short_rects):
            q = np.tile(base, (reps, 1))[:n]
            mem = np.tile(members("grid", case.scene, base), (1, reps))[:, :n]
            check_stacks(pm, r, case.scene, q, mem, (3,), FLAGS[::3], device_ks=(3,))


@pytest.mark.gpu
def test_non_finite_queries(pm, stack_renderer):
    """A non-finite point, a non-finite or inverted rectangle: all k words PM_HIT_NONE, count 0 -- between queries that hit."""
    case = hs.walk_scene(pm, 65)
    r = stack_renderer
    r.set_scene_bytes(case.scene)
    bad = [(np.nan, 50.0), (50.0, np.inf), (-np.inf, np.nan)]
    pts = np.array([hs.COMMON, bad[0], hs.COMMON, bad[1], bad[2], hs.COMMON], np.float32)
    rects = np.concatenate([np_rect.pick_rects([hs.COMMON], 1.0), BAD_RECTS, np_rect.pick_rects([hs.COMMON], 1.0), [[40, 60, 60, 40], [0, 0, np.inf, 10]]]).astype(np.float32)
    for q, dead in ((pts, [1, 3, 4]), (rects, [1, 2, 4, 5])):
        for k in (1, 5, 256):
            for skip, stop in FLAGS:
                items, cnt = host_stack(r, q, k, skip, stop, counts=True)
                assert (items[dead] == NONE).all() and (cnt[dead] == 0).all() and (items[0] != NONE).sum() == min(k, cnt[0]) > 0
                d, dc, keep = device_stack(pm, r, q, k, skip, stop)
                r.sync()
                assert np.array_equal(as_u32(d).reshape(len(q), k), items) and np.array_equal(as_u32(dc), cnt)


@pytest.mark.gpu
def test_a_host_call_across_its_batch_boundary(pm, stack_renderer):
    """k = 256: a batch of the host call holds STAGE_MAX / (4 k + 4 + the query's bytes) queries.  Three queries more than one batch,
    on a tiny scene, compared in full."""
    case = hs.walk_scene(pm, 5)
    r = stack_renderer
    r.set_scene_bytes(case.scene)
    short = np.concatenate([case.queries[:5], [hs.COMMON, hs.NOTHING, hs.ARMS_ONLY]]).astype(np.float32)
    for base, in_bytes, counts in ((short, 8, True), (np_rect.pick_rects(short, 3.0), 16, False)):
        n = STAGE_MAX // (4 * 256 + 4 + in_bytes) + 3
        reps = -(-n // len(base))
        q = np.tile(base, (reps, 1))[:n]
        want, want_cnt = np_stack.stack(case.scene, members("batch", case.scene, base), 256)
        got = host_stack(r, q, 256, counts=counts)
        items = got[0] if counts else got
        assert items.shape == (n, 256) and np.array_equal(items, np.tile(want, (reps, 1))[:n])
        assert not counts or np.array_equal(got[1], np.tile(want_cnt, reps)[:n])
        assert want_cnt.max() >= 3 and len({tuple(w) for w in want.tolist()}) >= 6


@pytest.mark.gpu
def test_a_stack_call_between_a_snap_and_a_selection(pm):
    """pm_snap, pm_hit_stack, pm_select_rect, pm_hit_rects_stack and pm_snap again on one context: they lay the ONE staging buffer
    out each in its own way, and every answer is the one the call gives alone."""
    case = hs.walk_scene(pm, 65)
    q = case.queries
    rects = pick_rects(q)
    radius = np.full(len(q), 6.0, np.float32)
    with pm.Renderer(0) as r:
        r.set_scene_bytes(case.scene)
        snap_alone = r.snap(q, radius).tobytes()
    with pm.Renderer(0) as r:
        r.set_scene_bytes(case.scene)
        select_alone = r.select_rect(40.0, 40.0, 120.0, 120.0)
    with pm.Renderer(0) as r:
        r.set_scene_bytes(case.scene)
        assert r.snap(q, radius).tobytes() == snap_alone
        items, cnt = r.hit_stack(q, 7, counts=True)
        touched, enclosed = r.select_rect(40.0, 40.0, 120.0, 120.0)
        ritems, rcnt = r.hit_rects_stack(rects, 130, stop_at_opaque=True, counts=True)
        assert r.snap(q, radius).tobytes() == snap_alone
        again = r.hit_stack(q, 7)
    want, want_cnt = np_stack.stack(case.scene, members(("walk", 65), case.scene, q), 7)
    assert np.array_equal(items, want) and np.array_equal(cnt, want_cnt) and np.array_equal(again, want)
    rwant, rwant_cnt = np_stack.stack(case.scene, members(("walk", 65), case.scene, rects), 130, stop_at_opaque=True)
    assert np.array_equal(ritems, rwant) and np.array_equal(rcnt, rwant_cnt)
    assert np.array_equal(touched, select_alone[0]) and np.array_equal(enclosed, select_alone[1]) and touched.any()


@pytest.mark.gpu
def test_argument_rules(pm):
    """Everything the four calls refuse is PM_ERR_INVALID before anything is enqueued, the context answers a correct call afterwards,
    and every other query call still refuses PM_HIT_STOP_AT_OPAQUE."""
    import ctypes as C

    lib = pm._lib.load()
    OK, INVALID = pm._lib.PM_OK, pm._lib.PM_ERR_INVALID
    STOP = pm._lib.PM_HIT_STOP_AT_OPAQUE
    with pm.Renderer(0) as r:
        items = np.full(4 * 256, UNTOUCHED, np.uint32)
        cnt = np.full(4, UNTOUCHED, np.uint32)
        pts = np.array([[50.0, 50.0]] * 4, np.float32)
        rects = np.array([[0, 0, 400, 400]] * 4, np.float32)
        ip, cp = items.ctypes.data, cnt.ctypes.data
        calls = [(lambda *a: lib.pm_hit_stack(r._h, *a), pts.ctypes.data), (lambda *a: lib.pm_hit_stack_device(r._h, *a, None), pts.ctypes.data),
                 (lambda *a: lib.pm_hit_rects_stack(r._h, *a), rects.ctypes.data), (lambda *a: lib.pm_hit_rects_stack_device(r._h, *a, None), rects.ctypes.data)]
        for call, qp in calls:                                       # (queries, n, k, flags, items, n_hit)
            assert call(qp, 4, 3, 0, ip, cp) == INVALID              # no scene: what pm_hit_test says
        r.set_scene_bytes(hand_scene(pm))
        for call, qp in calls:
            assert call(qp, 4, 0, 0, ip, cp) == INVALID              # k
            assert call(qp, 4, 257, 0, ip, cp) == INVALID
            assert call(qp, 0, 0, 0, ip, cp) == INVALID              # ... also with nothing to do
            assert call(qp, 4, 3, 2, ip, cp) == INVALID              # flag bits other than 1 and 8
            assert call(qp, 4, 3, 4, ip, cp) == INVALID
            assert call(qp, 4, 3, 0x80000009, ip, cp) == INVALID
            assert call(None, 4, 3, 0, ip, cp) == INVALID            # a NULL pointer with n > 0
            assert call(qp, 4, 3, 0, None, cp) == INVALID
            assert call(None, 0, 3, 0, None, None) == OK             # nothing to do
            assert call(qp, 0, 256, 9, ip, cp) == OK
        r.sync()
        assert (items == UNTOUCHED).all() and (cnt == UNTOUCHED).all()
        # a correct call afterwards.  (Only the host variants take these arrays: what the device variants were handed above is host
        # memory, which they must not touch and, refusing, did not.)
        for (call, qp), q in ((calls[0], pts), (calls[2], rects)):
            items[:] = UNTOUCHED
            assert call(qp, 4, 256, 9, ip, None) == OK
            d, dc, keep = device_stack(pm, r, q, 256, True, True, counts=False)
            r.sync()
            for got in (items, as_u32(d)):
                assert (got.reshape(4, 256)[:, :2] == [4, 2]).all() and (got.reshape(4, 256)[:, 2:] == NONE).all()   # (HAND, both flags)
            assert (cnt == UNTOUCHED).all() and (as_u32(dc) == UNTOUCHED).all()
        assert r.stats()["n_items"] == 6 and lib.pm_abi_version() == 600
        # every existing query call still takes the new bit for an unknown one
        words = np.full(16, UNTOUCHED, np.uint32)
        wp, n_items = words.ctypes.data, C.c_uint32(0)
        xyr = np.array([[50.0, 50.0, 5.0]] * 4, np.float32)
        out = np.zeros(6 * 48, np.uint8)
        poly = np.array([[0, 0], [400, 0], [400, 400]], np.float32)
        labels = np.zeros(16, np.uint32)
        for flags in (STOP, STOP | 1):
            assert lib.pm_hit_test(r._h, pts.ctypes.data, 4, flags, ip, cp) == INVALID
            assert lib.pm_hit_test_device(r._h, pts.ctypes.data, 4, flags, ip, cp, None) == INVALID
            assert lib.pm_hit_frame(r._h, 0, 0, 2, 2, flags, ip, cp, 2) == INVALID
            assert lib.pm_hit_frame_device(r._h, 0, 0, 2, 2, flags, ip, cp, 2, None) == INVALID
            assert lib.pm_hit_rects(r._h, rects.ctypes.data, 4, flags, ip, cp) == INVALID
            assert lib.pm_hit_rects_device(r._h, rects.ctypes.data, 4, flags, ip, cp, None) == INVALID
            assert lib.pm_select_rect(r._h, rects.ctypes.data, flags, wp, 16, C.byref(n_items), None, None) == INVALID
            assert lib.pm_select_rect_device(r._h, rects.ctypes.data, flags, wp, 16, None) == INVALID
            assert lib.pm_select_polygon(r._h, poly.ctypes.data, 3, flags, wp, 16, C.byref(n_items), None, None) == INVALID
            assert lib.pm_select_polygon_device(r._h, poly.ctypes.data, 3, flags, wp, 16, None) == INVALID
            assert lib.pm_snap(r._h, xyr.ctypes.data, 4, flags | pm._lib.PM_SNAP_VERTICES, None, 0, out.ctypes.data) == INVALID
            assert lib.pm_snap_device(r._h, xyr.ctypes.data, 4, flags | pm._lib.PM_SNAP_VERTICES, None, 0, out.ctypes.data, None) == INVALID
            assert lib.pm_snap_intersections(r._h, xyr.ctypes.data, 4, flags, None, 0, out.ctypes.data) == INVALID
            assert lib.pm_snap_intersections_device(r._h, xyr.ctypes.data, 4, flags, None, 0, out.ctypes.data, None) == INVALID
            assert lib.pm_item_bounds(r._h, flags, out.ctypes.data, 6, None) == INVALID
            assert lib.pm_item_bounds_device(r._h, flags, out.ctypes.data, 6, None) == INVALID
            assert lib.pm_union_bounds(r._h, flags, None, 0, 0, labels.ctypes.data, 16, 1, out.ctypes.data) == INVALID
            assert lib.pm_union_bounds_device(r._h, flags, None, 0, 0, labels.ctypes.data, 16, 1, out.ctypes.data, None) == INVALID
        r.sync()
        assert (words == UNTOUCHED).all() and not out.any() and (cnt == UNTOUCHED).all()
        # the Python wrappers
        with pytest.raises(ValueError):
            r.hit_stack(pts, 0)
        with pytest.raises(ValueError):
            r.hit_stack(pts, 257)
        with pytest.raises(ValueError):
            r.hit_stack(rects, 3)
        with pytest.raises(ValueError):
            r.hit_rects_stack(pts, 3)
        with pytest.raises(ValueError):
            r.pick_stack(rects, 1.0, 3)
        assert r.hit_stack(np.zeros((0, 2), np.float32), 5).shape == (0, 5)
        assert r.pick_stack(pts, 1.0, 2, counts=True)[1].tolist() == [6] * 4
        if not _emulated():
            import torch

            t = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
            with pytest.raises(TypeError):
                r.hit_stack_tensor(torch.zeros((4, 2)), t)                                   # not on the device
            with pytest.raises(TypeError):
                r.hit_stack_tensor(torch.zeros((4, 4), device="cuda"), t)                    # rectangles, not points
            with pytest.raises(TypeError):
                r.hit_rects_stack_tensor(torch.zeros((4, 4), device="cuda"), t[:3])
            with pytest.raises(TypeError):
                r.hit_stack_tensor(torch.zeros((4, 2), device="cuda"), t, torch.zeros(3, dtype=torch.int32, device="cuda"))
            with pytest.raises(ValueError):
                r.hit_stack_tensor(torch.zeros((4, 2), device="cuda"), torch.zeros((4, 257), dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
def test_cli_pick_depth(pm, tmp_path, capsys):
    """--pick-depth 4 prints what Renderer.hit_stack (with --pick-tolerance: pick_stack) returns; without it --pick prints what it
    printed before."""
    from piet_metal_amd import cli

    picks = [(240.0, 135.0), (3.0, 3.0), (200.5, 100.5), (176.0, 60.0)]
    base = ["tiger", str(tmp_path / "t.png"), "--width", "480", "--height", "270"]
    for x, y in picks:
        base += ["--pick", f"{x:g},{y:g}"]

    def run(extra):
        assert cli.main(base + extra) == 0
        return [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]

    deep, deep_tol, plain, one = run(["--pick-depth", "4"]), run(["--pick-depth", "4", "--pick-tolerance", "2.5"]), run([]), run(["--pick-depth", "1"])
    wl = pm.workloads.tiger(480, 270)
    with pm.Renderer(0) as r:
        r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        xy = np.array(picks, np.float32)
        stack, stack_tol, top = r.hit_stack(xy, 4), r.pick_stack(xy, 2.5, 4), r.hit_test(xy)
        of_item = r.item_paths()

    def line(head, items):
        found = [f"item {int(t)} path {int(of_item[t])}" for t in items if t != NONE]
        return head + (", ".join(found) if found else "none")

    assert deep == [line(f"{x:g},{y:g}: ", s) for (x, y), s in zip(picks, stack)]
    assert deep_tol == [line(f"{x:g},{y:g} +-2.5: ", s) for (x, y), s in zip(picks, stack_tol)]
    assert plain == one == [f"{x:g},{y:g}: " + ("none" if t == NONE else f"item {int(t)} path {int(of_item[t])}") for (x, y), t in zip(picks, top)]
    assert np.array_equal(stack[:, 0], top) and (stack[:, 3] != NONE).any() and any(ln.endswith("none") for ln in deep)


# ---- CPU: the same under emulation -------------------------------------------------------------------------------------------

def test_hit_stack_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library; the batch boundary, 66 MB through an
    emulated copy for what is a host loop, is left to the GPU."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", f"not {BATCH_TEST}"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS - 1} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout
