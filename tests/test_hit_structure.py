"""Hit testing where pm_hit_kernel's item walk and chunk index have edges (tests/hit_structure.py builds the scenes).

-m gpu: every scene through test_hit_gpu.check_against_np_hit -- top_item and n_hit EQUAL to tests/np_hit.py for every query, with
counts and in the walk that ends at the first hit, np_hit's two evaluation orders compared on all of them -- and once through
pm_hit_test_device with output arrays four entries too long, which must stay as they were.
CPU: the structural constants are pm_device.h's; every scene of part A is shown to reach the edge it names (a lost boundary chunk,
a lost super-chunk, the survivors after the first eight, the second round of super-chunks each change some query's answer); and
the -m gpu part runs against the wave64 emulation of the kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hit_structure as hs  # noqa: E402
import np_hit  # noqa: E402

NONE = hs.NONE
UNTOUCHED = 0x7EADBEEF
CASES = dict(hs.structure_cases())
N_GPU_TESTS = len(CASES) + len(hs.WALK_SIZES) + 1


def _emulated():
    return os.environ.get("PM_TEST_EMU") == "1"


# ---- CPU: the constants ------------------------------------------------------------------------------------------

def test_structural_constants_are_pm_device_h():
    """A retuned index must move these tests with it."""
    text = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_device.h")).read()
    got = {k: int(v) for k, v in re.findall(r"^constexpr uint32_t (kChunkSegs|kSuperChunks) = (\d+);", text, re.M)}
    assert got == {"kChunkSegs": hs.CHUNK_SEGS, "kSuperChunks": hs.SUPER_CHUNKS}
    hit = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_hit_test.h")).read()
    chunks = open(os.path.join(ROOT, "piet_metal_amd", "csrc", "pm_query_common.h")).read()   # (ForItemChunks, shared by the query kernels)
    assert f"hi > {hs.WAVE}u ? hi - {hs.WAVE}u : 0u" in hit and f"gb += {hs.WAVE}u" in chunks and f"cb1 - cb0 <= {hs.WAVE}u" in chunks


# ---- CPU: the cases prove what they claim -------------------------------------------------------------------------

def test_the_sizes_are_the_ones_named(pm):
    def chunks(ident):
        case = CASES[ident](pm)
        base, _, _ = hs.index_model(case.scene)
        cb0, cb1 = int(base[case.long_item]), int(base[case.long_item + 1])
        return cb0 % hs.SUPER_CHUNKS, cb1 - cb0, (cb1 - 1) // hs.SUPER_CHUNKS - cb0 // hs.SUPER_CHUNKS + 1

    assert chunks("loops-51-256-p1-l28-eo") == (7, 64, 9)
    assert chunks("meander-85-257-p2-l32-nz") == (0, 65, 9)
    assert chunks("loops-410-2048-p0-l32-eo") == (0, 512, 64)
    assert chunks("loops-410-2048-p3-l28-eo") == (7, 512, 65)
    assert chunks("meander-683-2049-p1-l32-nz") == (0, 513, 65)
    assert chunks("loops-1030-free-p0-l32-eo")[2] > 2 * hs.WAVE          # two full rounds of super-chunks and more
    assert [chunks(f"comb-{e or 5 * n}-l{lead}-nz")[1] for n, lead, e in hs.COMB_SIZES] == [64, 65, 129, 512, 513, 1038]
    assert [chunks(f"fan-{n}-l{lead}")[1:] for n, lead in hs.FAN_SIZES] == [(64, 9), (65, 9), (513, 65), (515, 66)]
    residues = {chunks(ident)[0] for ident in CASES}
    assert {0, 1, 3, 5, 7} <= residues, residues


def test_comb_separators_and_closing_segments_fall_everywhere(pm):
    """In the compound comb a separator is some chunk's first and some chunk's last entry, and closing segments have their target
    point in another chunk and in another super-chunk."""
    case = CASES["comb-515-l9-nz"](pm)
    sc = bytes(case.scene)
    base, _, _ = hs.index_model(sc)
    at, _ = np_hit.flat_items(sc)[case.long_item]
    pts = np_hit._points(sc, at)
    sep = np.flatnonzero(np.isnan(pts[:, 0]))
    assert set(sep % hs.CHUNK_SEGS) == {0, 1, 2, 3}
    closing = sep - 1                                                   # the entry whose segment ends at the sub-path's first point
    target = np.ascontiguousarray(pts[sep, 1]).view(np.uint32).astype(np.int64)
    cb0 = int(base[case.long_item])
    ch = lambda k: cb0 + k // hs.CHUNK_SEGS  # noqa: E731
    assert np.array_equal(target, closing - 3)
    assert (ch(closing) != ch(target)).any() and (ch(closing) == ch(target)).any()
    assert (ch(closing) // hs.SUPER_CHUNKS != ch(target) // hs.SUPER_CHUNKS).any()


@pytest.mark.parametrize("ident", list(CASES))
def test_a_lost_chunk_would_show(pm, ident):
    """From np_hit's pair functions: what the long item adds to every query, per chunk; then for each drop set that the kernel's
    structure suggests, some query's answer must change -- else the scene could not see that loss."""
    case = CASES[ident](pm)
    got = hs.losses(case)
    n = got["cb1"] - got["cb0"]
    blind = [c for c in got["boundary"] if not got["each_chunk"][c]]
    assert not blind, f"{case}: boundary chunks {blind} of {n} change no query's answer"
    assert got["each_chunk"].all(), f"{case}: chunks {np.flatnonzero(~got['each_chunk'])[:8]} change no query's answer"
    assert got["each_super"].all(), f"{case}: super-chunks {np.flatnonzero(~got['each_super'])[:8]} change no query's answer"
    if n > hs.WAVE:
        assert got["most_survivors"] > 8
        assert got["after_eight"].any() and got["after_eight_per_round"].any(), case
    if got["g1"] - got["g0"] > hs.WAVE:
        assert got["from_65th_super"].any(), case
    else:
        assert "from_65th_super" not in got


# ---- -m gpu ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hit_renderer(pm):
    """Never resized: hit testing needs a scene, not a viewport."""
    r = pm.Renderer(0)
    yield r
    r.close()


def device_hit_padded(pm, r, q, skip=False, pad=4):
    """pm_hit_test_device on arrays `pad` entries longer than the query list, filled with UNTOUCHED: (top, n_hit) as uint32
    [n + pad].  Under the emulation device memory is host memory, and the arrays are numpy's."""
    n = len(q)
    if _emulated():
        xy = np.ascontiguousarray(q, np.float32)
        top, cnt = np.full(n + pad, UNTOUCHED, np.uint32), np.full(n + pad, UNTOUCHED, np.uint32)
        flags = pm._lib.PM_HIT_SKIP_TRANSPARENT if skip else 0
        pm._lib.check(pm._lib.load().pm_hit_test_device(r._h, xy.ctypes.data, n, flags, top.ctypes.data, cnt.ctypes.data, None), "pm_hit_test_device")
        r.sync()
        return top, cnt
    import torch

    xy = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    top = torch.full((n + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + pad,), UNTOUCHED, dtype=torch.int32, device="cuda")
    r.hit_test_tensor(xy, top[:n], cnt[:n], skip_transparent=skip)
    r.sync()
    return top.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)


def assert_device_variant(pm, r, q, want_top, want_cnt, skip=False):
    top, cnt = device_hit_padded(pm, r, q, skip)
    n = len(q)
    assert np.array_equal(top[:n], want_top) and np.array_equal(cnt[:n], want_cnt)
    assert (top[n:] == UNTOUCHED).all() and (cnt[n:] == UNTOUCHED).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ident", list(CASES))
def test_long_item_by_chunk_count(pm, hit_renderer, ident):
    """Part A: one long Fill / compound Fill / Polyline between a lead and a trailing item."""
    from test_hit_gpu import check_against_np_hit

    case = CASES[ident](pm)
    r, q = hit_renderer, case.queries
    r.set_scene_bytes(case.scene)
    want_top, want_cnt = check_against_np_hit(r, case.scene, q, brute_sample=len(q))
    assert_device_variant(pm, r, q, want_top, want_cnt)
    assert r.stats()["n_items"] == len(np_hit.flat_items(case.scene))
    n_long = int((want_top == case.long_item).sum())
    assert n_long >= case.facts["npt"] // 16 and (want_top == NONE).sum() >= case.facts["npt"] // 16, (n_long, case)
    if ident.startswith("fan"):
        assert want_cnt.max() >= 2  # (the wide Polyline below the fan: the early exit has something to skip)


@pytest.mark.gpu
@pytest.mark.parametrize("n", hs.WALK_SIZES)
def test_item_walk_by_item_count(pm, hit_renderer, n):
    """Part C: n items of every kind, direct hits and candidates in one ballot, the first half in a child group."""
    from test_hit_gpu import check_against_np_hit

    case = hs.walk_scene(pm, n)
    r, q = hit_renderer, case.queries
    r.set_scene_bytes(case.scene)
    assert r.stats()["n_items"] == n
    covering, opaque = case.facts["covering"], case.facts["opaque"]
    for skip in (False, True):
        want_top, want_cnt = check_against_np_hit(r, case.scene, q, skip_transparent=skip, brute_sample=len(q))
        assert_device_variant(pm, r, q, want_top, want_cnt, skip)
        # the scene is what the construction says: every item is on top somewhere, and the common point is under all the arms
        shown = [i for i in range(n) if not skip or i % 3 != 0 or i not in covering]
        assert set(shown) <= set(want_top.tolist()), sorted(set(shown) - set(want_top.tolist()))
        assert np.array_equal(want_top[:n][shown], shown)
        under = opaque if skip else covering
        common, arms, nothing = 2 * n, 2 * n + 1, 2 * n + 2
        assert want_cnt[common] == len(under) == want_cnt.max() and want_top[common] == (under[-1] if under else NONE)
        assert skip or n < 4 or 0 < want_cnt[arms] < len(covering)
        assert want_top[nothing] == NONE and want_cnt[nothing] == 0
    assert n < 6 or {"compound", "polyline", "line", "fill", "circle", "ellipse"} <= set(case.facts["kinds"])


@pytest.mark.gpu
def test_query_counts_and_the_grid(pm, hit_renderer):
    """Part D: 1 ... 7 queries (fewer than a workgroup's waves, and one more) and one query either side of what the grid holds at
    once (32 per CU: eight workgroups of four waves) -- a short list repeated, so that a stride error is a wrong VALUE."""
    case = hs.walk_scene(pm, 5)
    r = hit_renderer
    r.set_scene_bytes(case.scene)
    spots = case.queries[:5]
    short = np.concatenate([spots[:1], [hs.COMMON, hs.NOTHING, (np.nan, 10.0)], spots[4:5], [hs.ARMS_ONLY], spots[1:2]]).astype(np.float32)
    want_top, want_cnt = np_hit.hit_test(case.scene, short)
    assert len(set(want_top.tolist())) >= 4 and NONE in want_top and want_cnt.max() >= 3
    if _emulated():
        cus = int(os.environ.get("PM_EMU_CUS", "256"))  # (what the emulated device reports)
        extra = [255, 257, 2049]
    else:
        import torch

        cus = torch.cuda.get_device_properties(0).multi_processor_count
        extra = []
    for n in [1, 2, 3, 4, 5, 7, 32 * cus - 1, 32 * cus, 32 * cus + 1] + extra:
        reps = -(-n // len(short))
        q = np.tile(short, (reps, 1))[:n]
        for skip in (False, True):
            wt, wc = (want_top, want_cnt) if not skip else np_hit.hit_test(case.scene, short, True)
            assert_device_variant(pm, r, q, np.tile(wt, reps)[:n], np.tile(wc, reps)[:n], skip)
        assert np.array_equal(r.hit_test(q), np.tile(want_top, reps)[:n])


# ---- CPU: the same under emulation ---------------------------------------------------------------------------------

def test_hit_structure_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    env = dict(os.environ, PM_TEST_EMU="1")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{N_GPU_TESTS} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout
