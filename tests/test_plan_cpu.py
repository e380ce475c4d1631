"""The binning planner (piet_metal_amd/csrc/pm_plan.h) on the CPU: tests/plan/plan_main.cpp, a stand-alone program built here with
g++ -- once plain, once with -fsanitize=address,undefined --, makes the plan of every case below, checks the plan's invariants
itself (regions, chains, the whole-row list, cut rows, idle rows, one-launch chains, per-tile-row offsets, the band list) and
writes every output array and scalar back; the digests of those are compared with tests/golden/plan_parent.json, recorded from the
commit named there, whose EnsureArena the planner was lifted out of: tie orders, headroom and the choice of cut rows are pinned by
that file, not by the invariants.

The cases are the smallest shapes at which each branch of the planner can go wrong; a viewport of 512 x 512 has 2 x 32 strip rows."""
import hashlib
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_parent.json")
PM_OK, PM_ERR_CAPACITY = 0, -4
UNSET = 0xFF  # PM_BIN_WG_PER_CU not given
LINE, FILL, POLY = 2, 3, 4

FIELDS = ("n_items", "n_chunks", "tiles_x", "strips_x", "row0", "row1", "n_cus", "margin", "bin_split_mode", "bin_split_cands",
          "bin_split_slots", "bin_split_fill", "bin_wg_per_cu", "bin_waves_env", "bin_waves_inflight", "one_launch_mode",
          "frame_wg_per_cu", "fold_clear_mode", "row_list_min_items", "row_list_part_items", "arena_cap")
DEFAULTS = dict(n_cus=256, margin=0, bin_split_mode=1, bin_split_cands=1 << 30, bin_split_slots=224, bin_split_fill=15, bin_wg_per_cu=UNSET,
                bin_waves_env=0, bin_waves_inflight=1, one_launch_mode=0, frame_wg_per_cu=0, fold_clear_mode=2, row_list_min_items=2048,
                row_list_part_items=0, arena_cap=0, ptcl_initial_cmds=0, ptcl_want=0)
SCALARS = ("cands", "n_sr_split", "bin_waves", "bin_grid", "one_grid_rows", "use_row_lists", "band_identity", "row_parts", "row_part_items",
           "row_total", "row_want", "sr_empty_dwords", "arena_total", "arena_alloc", "ptcl_want", "fb_applied", "reusable", "still_holds")
ARRAYS = ("desc", "desc_whole", "next_one", "idle", "band_bbox", "band_item", "row_base", "sr_list", "need", "box", "per")


# ---- scenes -----------------------------------------------------------------------------------------------------------

def meta_of(scene):
    """Header + boxes + items of a scene: all the planner reads."""
    scene = np.ascontiguousarray(scene, np.uint8)
    n, items_ix = struct.unpack_from("<II", scene, 0)
    return scene[: items_ix + 32 * n].tobytes()


def hand_meta(boxes, tags, npts):
    """item_meta from boxes (x0, y0, x1, y1), tags and point counts; no points: the planner never dereferences them."""
    n = len(boxes)
    items = np.zeros((n, 8), np.uint32)
    items[:, 0] = tags
    items[:, 3] = npts
    return struct.pack("<II", n, 8 + 8 * n) + np.asarray(boxes, np.uint16).reshape(n, 4).tobytes() + items.tobytes()


def row_grid(n_rows, per_row=1, npt=lambda k: 5 + 4 * (k % 7), extra=0):
    """Small fills, per_row in each of the first n_rows strip rows of a 512 x 512 viewport (every item in one strip row, spanning both
    of its halves), + extra more in strip row 0."""
    boxes, k = [], 0
    for i in range(n_rows):
        sx, r = i % 2, i // 2
        boxes += [(sx * 256 + 100, r * 16 + 2, sx * 256 + 150, r * 16 + 9)] * per_row
    boxes += [(100, 2, 150, 9)] * extra
    return hand_meta(boxes, [FILL] * len(boxes), [npt(k) for k in range(len(boxes))])


def build_cases(pm, pmo):
    """-> [(name, fields)]: fields as in FIELDS + ptcl_initial_cmds, ptcl_want, fb (the frames' report), meta, next (the next scene's meta)."""
    from edge_scenes import edge_scene
    from path_sets import random_case
    from piet_metal_amd import workloads
    from test_host_cpu import encode_ops, random_ops

    cases = []

    def case(name, meta, w=512, h=512, **kw):
        n = struct.unpack_from("<I", meta, 0)[0]
        tiles_x, tiles_y = (w + 15) // 16, (h + 15) // 16
        f = dict(DEFAULTS, n_items=n, n_chunks=2 * n + 1, tiles_x=tiles_x, strips_x=(tiles_x + 15) // 16, row0=0, row1=tiles_y, fb=[], meta=meta, next=b"")
        unknown = set(kw) - set(f)
        assert not unknown, unknown
        f.update(kw)
        cases.append((name, f))

    rand = meta_of(encode_ops(pm, random_ops(11, 120, extent=520.0)))
    blobs_w = workloads.config4_blobs(n_paths=150, size=512)
    blobs = meta_of(pmo.scene_from_paths(pmo.scaled_paths(blobs_w.paths.paths, blobs_w.width_scale), blobs_w.paths.els, blobs_w.affine)[0])
    tiger_w = workloads.tiger(512, 512)
    tiger = meta_of(pmo.scene_from_paths(pmo.scaled_paths(tiger_w.paths.paths, tiger_w.width_scale), tiger_w.paths.els, tiger_w.affine)[0])

    # grids and chains: n_cus 2 (grid 10, chains of several rows) and 256 (no chain); PM_BIN_WG_PER_CU 0, 1, default
    for name, meta in (("rand", rand), ("blobs", blobs), ("tiger", tiger)):
        for n_cus in (2, 256):
            case(f"{name}_cus{n_cus}", meta, n_cus=n_cus)
    for per_cu in (0, 1):
        case(f"rand_cus2_wg{per_cu}", rand, n_cus=2, bin_wg_per_cu=per_cu)
        case(f"tiger_cus2_wg{per_cu}_split2", tiger, n_cus=2, bin_wg_per_cu=per_cu, bin_split_mode=2)
    case("rand_band_5_20", rand, row0=5, row1=20, n_cus=2)
    case("rand_band_5_20_wide", rand, row0=5, row1=20, margin=16)
    case("rand_300x330", rand, w=300, h=330, n_cus=2)
    case("rand_300x330_split2", rand, w=300, h=330, bin_split_mode=2)
    for seed in (1000, 1001, 1002, 1003):
        scene, w, h, _ = edge_scene(pm, seed)
        case(f"edge_{seed}", meta_of(scene), w=w, h=h, n_cus=2, bin_split_mode=2 if seed & 1 else 1)
    for seed in (1, 2, 3):
        c = random_case(seed)
        scene = pmo.scene_from_paths(pmo.scaled_paths(c.ps.paths, c.scale), c.ps.els, c.affine)[0]
        case(f"grammar_{seed}", meta_of(scene), w=c.width, h=c.height, n_cus=2, margin=16 if seed == 2 else 0)
    case("empty", hand_meta([], [], []))
    case("empty_fold3", hand_meta([], [], []), fold_clear_mode=3)
    case("outside", hand_meta([(600, 10, 700, 40), (10, 600, 40, 700), (2000, 2000, 2100, 2100)], [FILL, POLY, LINE], [9, 9, 2]))
    case("outside_wide", hand_meta([(520, 10, 700, 40), (10, 520, 40, 700), (100, 100, 200, 200)], [FILL, POLY, LINE], [9, 9, 2]), margin=16)
    case("clamp_65535", hand_meta([(65000, 65000, 65535, 65535), (5, 5, 65535, 65535), (0, 0, 3, 3)], [FILL, POLY, FILL], [40, 3, 1]), w=65535, h=512, margin=16)

    # cuts
    for mode in (0, 1, 2):
        case(f"tiger_split{mode}", tiger, bin_split_mode=mode)
    case("tiger_split1_cands", tiger, bin_split_cands=24)
    n_sr = 64
    report = [(37 * i) % 223 for i in range(n_sr)]
    case("tiger_report_below", tiger, fb=report[:5] + [223] + report[6:])
    case("tiger_report_at", tiger, fb=report[:5] + [224] + report[6:])
    case("tiger_report_many", tiger, fb=[200 + (13 * i) % 90 for i in range(n_sr)])
    case("tiger_report_wrong_size", tiger, fb=[300] * (n_sr - 1))
    # more heavy rows than room: six strip rows, a resident grid of 2 x 5 x 15 / 16 = 9 -- room for three, picked by weight, ties by row
    case("room_ties", row_grid(6), n_cus=2, fb=[300] * 6 + [0] * 58)
    case("room_weights", row_grid(6), n_cus=2, fb=[300, 400, 300, 500, 400, 224] + [0] * 58)
    case("room_cands", row_grid(6, per_row=3, extra=2), n_cus=2, bin_split_cands=3)
    case("room_fill4", row_grid(6), n_cus=2, bin_split_fill=4, fb=[300] * 6 + [0] * 58)
    # a heavy row one of whose halves nothing reaches stays whole
    halves = hand_meta([(10, 10, 100, 20), (300, 40, 500, 44), (384, 70, 500, 75), (0, 100, 511, 101)], [FILL, POLY, FILL, LINE], [12, 30, 7, 2])
    case("half_empty_split2", halves, bin_split_mode=2)
    case("half_empty_report", halves, fb=[500] * n_sr)

    # per-tile-row item lists forced on: 1, 2 and many parts, an item count that is a multiple of the part size
    grid128 = row_grid(64, per_row=2)
    for part in (0, 1000, 128, 64, 100, 32, 7, 1):
        case(f"rows_grid128_part{part}", grid128, row_list_min_items=0, row_list_part_items=part, n_cus=2)
    case("rows_rand_part50", rand, row_list_min_items=0, row_list_part_items=50, n_cus=256, bin_split_mode=2)
    case("rows_rand_band", rand, row_list_min_items=0, row_list_part_items=13, row0=3, row1=17, n_cus=2, fold_clear_mode=3)
    case("rows_min_at", grid128, row_list_min_items=128)
    case("rows_min_above", grid128, row_list_min_items=129)
    case("rows_empty", hand_meta([], [], []), row_list_min_items=0)

    # a wave per strip row: 2 CUs -> 30 entries and 32 candidates per entry are the thresholds
    for waves in (0, 1, 4):
        case(f"light_29_env{waves}", row_grid(29, per_row=32), n_cus=2, bin_waves_env=waves)
        case(f"light_30_env{waves}", row_grid(30, per_row=32), n_cus=2, bin_waves_env=waves)
        case(f"light_30_heavy_env{waves}", row_grid(30, per_row=32, extra=1), n_cus=2, bin_waves_env=waves)
    case("light_30_wg1", row_grid(30, per_row=32), n_cus=2, bin_wg_per_cu=1)

    # one launch per frame: 2 CUs x 4 workgroups = 8 resident
    for rows in (5, 8, 12, 16, 17, 30):
        case(f"one_launch_{rows}", row_grid(rows), n_cus=2, one_launch_mode=1, frame_wg_per_cu=4)
    case("one_launch_rand", rand, n_cus=16, one_launch_mode=1, frame_wg_per_cu=4)
    case("one_launch_no_wg", row_grid(5), n_cus=2, one_launch_mode=1, frame_wg_per_cu=0)
    case("fold3_rand_cus2", rand, n_cus=2, fold_clear_mode=3)
    case("fold3_rand_cus256", rand, fold_clear_mode=3)

    # sizes: an arena that grows, one that fits, the tile arena's switches
    case("arena_grows", tiger, arena_cap=1000)
    case("arena_fits", tiger, arena_cap=1 << 28)
    case("ptcl_initial", tiger, ptcl_initial_cmds=64)
    case("ptcl_kept", tiger, ptcl_want=1 << 30, bin_waves_inflight=4)
    case("ptcl_many_chunks", tiger, n_chunks=1 << 20)

    # the reuse check
    boxes = [(40 + 50 * (k % 8), 40 + 50 * (k // 8), 70 + 50 * (k % 8), 75 + 50 * (k // 8)) for k in range(48)]
    tags = [(FILL, POLY, LINE)[k % 3] for k in range(48)]
    npts = [8 + k for k in range(48)]

    def moved(k, dx0=0, dy0=0, dx1=0, dy1=0):
        b = list(boxes)
        b[k] = (b[k][0] + dx0, b[k][1] + dy0, b[k][2] + dx1, b[k][3] + dy1)
        return hand_meta(b, tags, npts)

    base = hand_meta(boxes, tags, npts)
    gained = list(npts)
    gained[6] += 4 * 4  # (a zooming plan leaves room for a quarter more segments and two chunks: past that)
    for name, nxt in (("same", base), ("inside", moved(5, -16, -16, 16, 16)), ("outside_x", moved(5, dx1=17)), ("outside_y", moved(7, dy0=-17)),
                      ("chunk", hand_meta(boxes, tags, gained)), ("chunk_within", hand_meta(boxes, tags, [v + 1 for v in npts])),
                      ("fewer", hand_meta(boxes[:-1], tags[:-1], npts[:-1])), ("inverted", moved(9, dx0=40))):
        case(f"reuse_{name}", base, margin=16, next=nxt)
    case("reuse_not_wide", base, next=base)
    case("reuse_row_lists", base, margin=16, row_list_min_items=0, next=base)
    case("reuse_band", base, margin=16, row0=0, row1=10, next=base)

    # capacity: point counts that push the arena past 0xfffffff0 dwords; per-tile-row lists past 2^32 entries (2^20 items in each of
    # 4 096 tile rows).  Both PM_ERR_CAPACITY.
    case("capacity_arena", hand_meta([(0, 0, 511, 511)], [FILL], [0xFFFFFFFF]))
    case("capacity_arena_sum", hand_meta([(0, 0, 511, 511)] * 8, [POLY] * 8, [0x7FFFFFFF] * 8), n_cus=2)
    n_big = 1 << 20
    big = np.zeros((n_big, 8), np.uint32)
    big[:, 0] = LINE
    big[:, 3] = 2
    big_boxes = np.tile(np.asarray([0, 0, 15, 65535], np.uint16), (n_big, 1))
    case("capacity_row_lists", struct.pack("<II", n_big, 8 + 8 * n_big) + big_boxes.tobytes() + big.tobytes(), w=16, h=65535, row_list_min_items=0)
    return cases


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, c in cases:
            f.write(struct.pack("<21I", *[c[k] for k in FIELDS]))
            f.write(struct.pack("<QQ", c["ptcl_initial_cmds"], c["ptcl_want"]))
            f.write(struct.pack("<I", len(c["fb"])) + np.asarray(c["fb"], np.uint32).tobytes())
            f.write(struct.pack("<Q", len(c["meta"])) + c["meta"])
            f.write(struct.pack("<Q", len(c["next"])) + c["next"])


def read_results(path, cases):
    """-> {name: {"rc", "scalars": {..}, "sha256": {array: digest}}} from what plan_main (or the dump of the parent) wrote."""
    data = open(path, "rb").read()
    at, out = 0, {}
    for name, _ in cases:
        (rc,) = struct.unpack_from("<q", data, at)
        at += 8
        res = {"rc": rc}
        if rc == PM_OK:
            vals = struct.unpack_from(f"<{len(SCALARS)}Q", data, at)
            at += 8 * len(SCALARS)
            res["scalars"] = dict(zip(SCALARS, vals))
            res["sha256"] = {}
            for a in ARRAYS:
                (nb,) = struct.unpack_from("<Q", data, at)
                res["sha256"][a] = hashlib.sha256(data[at + 8: at + 8 + nb]).hexdigest() + f":{nb}"
                at += 8 + nb
        out[name] = res
    assert at == len(data)
    return out


# ---- the test ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_run(pm, pmo, tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    cases = build_cases(pm, pmo)
    assert len({n for n, _ in cases}) == len(cases)
    write_cases(d / "cases.bin", cases)
    inc = ["-I" + os.path.join(ROOT, "tests", "emu", "include"), "-I" + os.path.join(ROOT, "piet_metal_amd", "csrc")]
    src = os.path.join(ROOT, "tests", "plan", "plan_main.cpp")
    builds = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
    results, limit = {}, {}
    for name, flags in builds.items():
        exe = str(d / f"plan_main_{name}")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", *flags, *inc, src, "-o", exe])
        # (MakeRowLists at its own limit, 2^32 entries: seconds of counting, so it runs beside the cases)
        limit[name] = subprocess.Popen([exe, "--row-lists-limit"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        p = subprocess.run([exe, str(d / "cases.bin"), str(d / f"out_{name}.bin")], capture_output=True, text=True)
        results[name] = (p, read_results(d / f"out_{name}.bin", cases) if p.returncode in (0, 1) else None)
    for name, p in limit.items():
        _, err = p.communicate()
        results[name] += ((p.returncode, err),)
    return cases, results


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_plan_invariants(plan_run, build):
    """Every case's plan satisfies the invariants plan_main checks, and the sanitizers stay silent."""
    _, results = plan_run
    p, _, limit = results[build]
    assert p.returncode == 0 and p.stderr == "", p.stderr[-4000:]
    assert limit == (0, ""), limit  # MakeRowLists on 2^32 entries: PM_ERR_CAPACITY


def test_plan_builds_agree(plan_run):
    _, results = plan_run
    assert results["plain"][1] == results["sanitized"][1]


def test_plan_capacity_cases(plan_run):
    cases, results = plan_run
    got = results["sanitized"][1]
    for name, _ in cases:
        assert got[name]["rc"] == (PM_ERR_CAPACITY if name.startswith("capacity_") else PM_OK), name


def test_plan_reuse_answers(plan_run):
    """PlanStillHolds: the same scene and a box moved inside its widened box keep the plan; a box one pixel outside, an item gaining a
    chunk, an item fewer and an inverted box do not; nor does a plan that was not made to last."""
    _, results = plan_run
    got = {n: r["scalars"]["still_holds"] for n, r in results["plain"][1].items() if n.startswith("reuse_")}
    assert got == {"reuse_same": 1, "reuse_inside": 1, "reuse_outside_x": 0, "reuse_outside_y": 0, "reuse_chunk": 0, "reuse_chunk_within": 1,
                   "reuse_fewer": 0, "reuse_inverted": 0, "reuse_not_wide": 0, "reuse_row_lists": 0, "reuse_band": 0}


def test_plan_equals_parent(plan_run):
    """Byte for byte what the parent commit's EnsureArena staged for the same inputs: every array's SHA-256 and every scalar."""
    cases, results = plan_run
    golden = json.load(open(GOLDEN))
    assert re.fullmatch(r"[0-9a-f]{40}", golden["parent_commit"]) and golden["recipe"]
    got = results["plain"][1]
    assert set(golden["cases"]) == {n for n, _ in cases}
    for name, _ in cases:
        assert got[name] == golden["cases"][name], name
