"""The seven newer query families -- pm_select_polygon, pm_snap, pm_item_bounds / pm_union_bounds, pm_snap_intersections,
pm_hit_stack / pm_hit_rects_stack, pm_item_lengths / pm_points_at_length / pm_positions_on_edges and their device calls -- on the
committed scripts of tests/test_context_sequences.py (tests/context_queries.py): behind every state change every call once, with
flags drawn from (seed, step), EQUAL as bytes to the numpy references on the MODEL's bytes; selection words chained into
union_bounds and snap; group_bounds under the current map and path_lengths per path, refused after an upload; all of them refused,
nothing written, with no scene; the device variants in flight over two side streams A, B, A across the straddling replacement;
and no answer moved by a resize, a band, an invalid call, the identity repaint or the equal table.

-m gpu: every script of SEEDS + NAMED, and the three switch rows on SWITCH_SEEDS (and, through the CPU test at the end, under the
wave64 emulation of a box without a GPU).  Two omissions in the host code cannot show under the emulation, where every launch has
completed when it returns: a family without QueryOrderBehind, and pm_repaint_groups not waiting for ev_hit.  For these the in-flight
part on the GPU is the test; it runs once per script and is not repeated.
CPU: the scripts are the ones of the parent commit (a digest of their repr); the walk is not blind -- every (state change, family,
skip_transparent) changes a reference answer somewhere, but for a written table of exclusions --; the answers are answers.

Wall time of test_context_queries_under_wave64_emulation on the 8-core box this was written on: 101 s (38 + 2 ids, 4 workers); of
test_context_sequences_under_wave64_emulation on the same box at the parent commit: 79 s (38 + 4 ids).

Regressions -- minimised scripts of bugs this walk finds -- go to REGRESSIONS with a comment saying what was wrong (none so far)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import context_model as cm  # noqa: E402
import context_queries as cq  # noqa: E402
import np_cross  # noqa: E402
import np_measure as nm  # noqa: E402
import np_poly  # noqa: E402
from test_context_sequences import ALL, NAMED, SEEDS, SWITCH_ROWS, SWITCH_SEEDS, _answers, _id, _walk, script_of  # noqa: E402
from test_frame_sequences import COMMON, ROWS, _ENV_KEYS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sha256 over repr of every step of the 29 committed scripts, taken at the parent commit of the one that added this file
SCRIPTS_DIGEST = "af07d0da1af9cf76ded9a834882e6337722a955cb59a6a843885f59b039b5bd0"
REGRESSIONS = {}    # name -> script as in test_context_sequences.NAMED

_answers2 = cq.Answers2()


# ---- -m gpu ------------------------------------------------------------------------------------------------------------------

def _run(pm, pmo, monkeypatch, script, seed, env):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pm.Renderer(0) as r:
        run = cq.QueryRunner(pm, pmo, r, script, seed, answers=_answers, answers2=_answers2)
        run.run()
        changes = sum(s.kind in cm.STATE_OPS for s in script)
        assert run.calls_made >= 12 * (changes - 3) and not run.pending2, (run.calls_made, changes)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ALL + list(REGRESSIONS), ids=[_id(s) for s in ALL + list(REGRESSIONS)])
def test_context_queries(pm, pmo, monkeypatch, seed):
    script = cm.scripted(pm, pmo, REGRESSIONS[seed], answers=_answers) if seed in REGRESSIONS else script_of(pm, pmo, seed)
    _run(pm, pmo, monkeypatch, script, seed, {})


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SWITCH_SEEDS, ids=[_id(s) for s in SWITCH_SEEDS])
@pytest.mark.parametrize("row", SWITCH_ROWS)
def test_context_queries_switches(pm, pmo, monkeypatch, row, seed):
    env = {name: e for name, e, _ in ROWS}[row]
    _run(pm, pmo, monkeypatch, script_of(pm, pmo, seed), seed, {**COMMON, **env})


# ---- CPU: the scripts are the parent's ---------------------------------------------------------------------------------------------

def test_the_committed_scripts_are_the_parents(pm, pmo):
    """cm.generate(seed) for every entry of SEEDS and cm.scripted(NAMED[...]) draw exactly the steps they drew before this file."""
    h = hashlib.sha256()
    assert len(ALL) == 29 and ALL == SEEDS + list(NAMED)
    for seed in ALL:
        h.update((repr(seed) + "\n" + "\n".join(repr(s) for s in script_of(pm, pmo, seed)) + "\n\n").encode())
    assert h.hexdigest() == SCRIPTS_DIGEST
    assert cm.QUERY_OBS == ("hit_test", "hit_frame", "hit_rects", "select_rect") and len(cm.OBS) == 10


# ---- CPU: the walk is not blind ---------------------------------------------------------------------------------------------------

OBSERVED = cq.FAMILIES + ("stack_stop", "group_bounds", "path_lengths")   # stack_stop: the stacks with PM_HIT_STOP_AT_OPAQUE
NO_COLOUR = ("polygon", "snap", "cross", "bounds", "stack", "measure", "group_bounds", "path_lengths")   # without the skip flag these read no colour byte
REPAINTS = tuple(f"repaint:{v}" for v in cm.VARIANTS["repaint"] if v != "identity")
SAME = tuple(sorted(f"{k}:{v}" for k, v in cq.SAME_ANSWERS))


def _key(s):
    return f"{s.kind}:{s.variant}" if s.kind in ("repaint", "reflatten_groups", "invalid", "resize", "band") else s.kind


# (state change, family, skip_transparent) that changes no reference answer in any committed script: why
EXCLUDED = {}
for _k in SAME:
    for _f in OBSERVED:
        for _s in (False, True):
            EXCLUDED[_k, _f, _s] = "the scene bytes and the map stay and the query set is no function of viewport or band: asserted to NEVER change"
for _f in OBSERVED:
    for _s in (False, True):
        if _f != "group_bounds":
            EXCLUDED["groups", _f, _s] = "a new map leaves the bytes alone; group_bounds alone labels items through it: asserted to NEVER change"
for _k in REPAINTS:
    for _f in NO_COLOUR:
        EXCLUDED[_k, _f, False] = "a repaint rewrites colour bytes in place; without PM_HIT_SKIP_TRANSPARENT this family reads none: asserted to NEVER change"
EXCLUDED["repaint:tint", "stack_stop", False] = ("a tint leaves the alpha byte to the opacity, and opacity 255 gives the paths' own alpha: the chain to the first opaque item "
                                                 "moves only where the paint in front had changed the alpha of an item that is opaque of its own under a query; no "
                                                 "committed script has that (repaint:half and repaint:solid cover the byte PM_HIT_STOP_AT_OPAQUE reads)")
NEVER = {k for k, why in EXCLUDED.items() if "NEVER" in why}


def _differs(a, b):
    for name in a:
        if name == "ws":
            continue
        x, y = (v if isinstance(v, tuple) else (v,) for v in (a[name], b[name]))
        if any(np.ascontiguousarray(p).tobytes() != np.ascontiguousarray(q).tobytes() for p, q in zip(x, y)):
            return True
    return False


def _reference(m, ex, family, skip):
    """The reference answer of `family` in the model's state (None: group_bounds / path_lengths of an upload)."""
    f = cq.Flags(skip=skip, stop=family == "stack_stop")
    if family in ("group_bounds", "path_lengths"):
        return None if ex[2] is None else {family: _answers2.paths(ex[0], ex[2], m.gmap, f)[family]}
    return _answers2.get("stack" if family == "stack_stop" else family, ex[0], f)


def _state_changes(pm, pmo):
    """(seed, step, model before, model after) of every state change with a scene on both sides, over the committed scripts."""
    for seed in ALL:
        m = cm.Model(pm, pmo)
        for s, _ in _walk(script_of(pm, pmo, seed)):
            after = m.copy()
            after.apply(s)
            if m.expected() is not None and after.expected() is not None:
                yield seed, s, m, after
            m = after


def test_the_walk_is_not_blind(pm, pmo):
    """Replay every script on the model alone: for every state change (repaints and tables by variant), every family and both values
    of skip_transparent the reference answer changes across the step at least once; the exclusions are EXCLUDED, and those whose
    reason is a contract never change."""
    seen, changed = {}, {}
    for seed, s, before, after in _state_changes(pm, pmo):
        for family in OBSERVED:
            for skip in (False, True):
                b, a = _reference(before, before.expected(), family, skip), _reference(after, after.expected(), family, skip)
                if b is None or a is None:
                    continue
                key = (_key(s), family, skip)
                seen[key] = seen.get(key, 0) + 1
                changed[key] = changed.get(key, 0) + _differs(b, a)
    kinds = {k for k, _, _ in seen}
    want_kinds = {"flatten", "upload", "reflatten", "groups"} | {f"reflatten_groups:{v}" for v in cm.VARIANTS["reflatten_groups"]} | set(REPAINTS) | set(SAME)
    assert kinds == want_kinds, sorted(kinds ^ want_kinds)
    for kind in sorted(kinds):
        for family in OBSERVED:
            for skip in (False, True):
                key = (kind, family, skip)
                if family in ("group_bounds", "path_lengths") and key not in seen:   # (needs the paths on both sides: never at an upload)
                    assert kind == "upload" or key in EXCLUDED, key
                    continue
                assert seen.get(key, 0) > 0, key
                if key in NEVER:
                    assert changed[key] == 0, (key, changed[key], EXCLUDED[key])
                elif key not in EXCLUDED:
                    assert changed[key] > 0, (key, seen[key])
    assert not [k for k in EXCLUDED if k not in seen and k[1] not in ("group_bounds", "path_lengths")], "an exclusion for a pair that does not occur"
    # what the issue names: the byte PM_HIT_STOP_AT_OPAQUE reads moves under repaint:half without the skip flag; a map moves group_bounds
    assert changed["repaint:half", "stack_stop", False] > 0 and changed["groups", "group_bounds", False] > 0 and changed["groups", "group_bounds", True] > 0
    print(f"{sum(seen.values())} (state change, family, flag) steps over {len(kinds)} kinds of state change: {sum(1 for k in seen if k not in EXCLUDED)} pairs change, "
          f"{len(EXCLUDED)} excluded ({len(NEVER)} of them asserted never to change)")


# ---- CPU: the answers are answers -------------------------------------------------------------------------------------------------

# scripts in whose scenes no two edges cross (asserted): why
NO_CROSSINGS = {"kept_plan_rows_that_fill": "its one path set, local_grouped, is four shapes apart from each other, each a convex outline: edges meet at vertices alone"}


def test_the_answers_are_answers(pm, pmo):
    """On the references alone, per script: every family finds and misses; intersections are found and no query meets
    PM_SNAP_KIND_TOO_MANY; items are enclosed and touched without being enclosed; a stack is clipped by k and one is padded; and over
    all scripts the lengths have all three kinds."""
    kinds = set()
    f = cq.Flags()
    for seed in ALL:
        has = set()
        m = cm.Model(pm, pmo)
        for s, _ in _walk(script_of(pm, pmo, seed)):
            m.apply(s)
            ex = m.expected()
            if ex is None:
                continue
            scene = ex[0]
            for name, words in _answers2.get("polygon", scene, f).items():
                has |= {("polygon", "enclosed"), (name, "enclosed")} if (words & np_poly.ENCLOSES).any() else set()
                has |= {("polygon", "touched only"), (name, "touched only")} if (words == np_poly.TOUCHES).any() else set()
                has |= {("polygon", "missed")} if (words == 0).any() else set()
            spiral_eo = _answers2.get("polygon", scene, cq.Flags(even_odd=True))["spiral"]
            has |= {"even_odd matters"} if not np.array_equal(spiral_eo, _answers2.get("polygon", scene, f)["spiral"]) else set()
            for name, rec in list(_answers2.get("snap", scene, f).items()) + list(_answers2.get("cross", scene, f).items()):
                has |= {(name, "found")} if (rec["item"] != cq.NONE).any() else set()
                has |= {(name, "missed")} if (rec["item"] == cq.NONE).any() else set()
                has |= {(name, "kind", int(k)) for k in np.unique(rec["kind"])}
            snap = _answers2.get("snap", scene, f)
            has |= {"the mask matters"} if snap["snap"].tobytes() != snap["snap_masked"].tobytes() else set()
            b = _answers2.get("bounds", scene, f)
            has |= {("union_bounds", "found")} if (b["union_bounds"]["n_boxed"][:3] > 0).any() else set()
            has |= {("union_bounds", "missed")} if b["union_bounds"]["n_items"][3] == 0 and np.isinf(b["union_bounds"]["box"][3]).all() else set()
            has |= {("item_bounds", "found")} if np.isfinite(b["item_bounds"]).all(axis=1).any() else set()
            for k in cq.STACK_K:
                for name, (items, cnt) in _answers2.get("stack", scene, cq.Flags(k=k)).items():
                    has |= {(name, "found")} if (cnt > 0).any() else set()
                    has |= {(name, "missed")} if (cnt == 0).any() else set()
                    has |= {(name, "clipped")} if (cnt > k).any() else set()
                    has |= {(name, "padded")} if ((cnt < k) & (cnt > 0)).any() and (items == cq.NONE).any() else set()
            ms = _answers2.get("measure", scene, f)
            kinds |= set(ms["lengths"]["kind"].tolist())
            has |= {("points", int(st)) for st in np.unique(ms["points"]["status"])}
            for name in ("points", "positions"):
                has |= {(name, "found")} if (ms[name]["item"] != cq.NONE).any() else set()
                has |= {(name, "missed")} if (ms[name]["item"] == cq.NONE).any() else set()
            has |= {("lengths", "found")} if (ms["lengths"]["length"] > 0).any() else set()
        # (the spiral's outer loop is the whole grid: it misses nothing; the lasso does)
        want = {(p, w) for p in ("lasso", "spiral") for w in ("enclosed", "touched only")} | {("polygon", "missed"), "even_odd matters", "the mask matters"}
        want |= {(n, w) for n in ("snap", "snap_masked", "cross", "hit_stack", "hit_rects_stack", "points", "positions", "union_bounds") for w in ("found", "missed")}
        want |= {(n, w) for n in ("hit_stack", "hit_rects_stack") for w in ("clipped", "padded")} | {("item_bounds", "found"), ("lengths", "found")}
        want |= {("snap", "kind", 1), ("snap", "kind", 2), ("cross", "kind", np_cross.INTERSECTION), ("points", nm.FOUND), ("points", nm.FOUND | nm.CLAMPED)}
        if seed in NO_CROSSINGS:
            assert ("cross", "found") not in has, seed
            want -= {("cross", "found"), ("cross", "kind", np_cross.INTERSECTION)}
        assert want <= has, (seed, sorted(map(str, want - has)))
        assert ("cross", "kind", np_cross.TOO_MANY) not in has, seed
    assert kinds == {nm.NONE, nm.OPEN, nm.CLOSED}, kinds


def test_the_flags_are_drawn_from_seed_and_step():
    a = [cq.draw_flags(s, k) for s in ALL for k in range(40)]
    assert a == [cq.draw_flags(s, k) for s in ALL for k in range(40)]
    for name, values in (("skip", (False, True)), ("stop", (False, True)), ("even_odd", (False, True)), ("counts", (False, True)), ("k", cq.STACK_K),
                         ("mask", (np_poly.TOUCHES, np_poly.ENCLOSES))):
        assert {getattr(f, name) for f in a} == set(values), name
    assert {(f.vertices, f.edges) for f in a} == {(True, True), (True, False), (False, True)}
    assert len(cq.GRID) == 216 and cq.STACK_K == (1, 4, 16) and len(cq.LASSO) == 6


# ---- CPU: the gpu part under the wave64 emulation -----------------------------------------------------------------------------------

EMU_TWO_CUS = ["paint_over_maps_and_uploads", SEEDS[0]]


def _emulated(k, n, extra=None):
    env = dict(os.environ, PM_TEST_EMU="1", **(extra or {}))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", k, "-p", "no:cacheprovider", "-n", "4"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=3000)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{n} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_context_queries_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library: every script, the switch rows too,
    and two scripts on a two-CU device."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    _emulated("test_context_queries", len(ALL) + len(REGRESSIONS) + len(SWITCH_ROWS) * len(SWITCH_SEEDS))
    two = " or ".join(_id(s) for s in EMU_TWO_CUS)
    _emulated(f"test_context_queries and not switches and ({two})", len(EMU_TWO_CUS), {"PM_EMU_CUS": "2"})
