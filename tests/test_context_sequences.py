"""One context through interleaved replacements, frames and queries (tests/context_model.py): scripts drawn from SEEDS walk one
Renderer through flatten_and_encode, uploads, uniform and grouped re-flattens, group maps, repaints, resizes, bands, invalid calls
and failed replacements in arbitrary order, with lone frames, bursts, frames and queries in flight, the four query kinds, item_paths,
fill_coverage and the captured tile lists in between -- every one compared, for equality, with what the model says the scene is at
that moment.

-m gpu: the scripts on the device (and, through the CPU test at the end, under the wave64 emulation of a box without a GPU).
CPU: the conditions that keep the GPU part from being blind -- every ordered pair of state changes that preconditions allow, every
variant, every (state change, observation) pair and every straddled replacement occurs; no state change of a committed script is
blind; the model agrees with the helpers of the merged feature tests on their own sequences."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import context_model as cm  # noqa: E402
import path_sets  # noqa: E402
from test_frame_sequences import COMMON, ROWS, _ENV_KEYS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The committed scripts: cm.generate(seed).  Chosen greedily from seeds 0..499 until the coverage conditions below held.
SEEDS = [8, 10, 13, 14, 51, 53, 56, 60, 71, 79, 88, 135, 144, 147, 177, 191, 200, 227, 230, 232, 241, 303, 346, 374, 415]
# Scripts written out, for the orders a mutation of the host code survived in the drawn scripts (HISTORY.md has the list): plans kept
# over view changes and what must end them, and the paint over maps, uploads and the host's colour-stale records.  Regressions --
# minimised scripts of bugs the sequences find -- go here too, with a comment saying what was wrong (none so far).
NAMED = {
    # a view that leaves the upper tile rows empty, the view that fills them again (the box-inside test), a move of less than a tile
    # behind a plan that was remade from its frames' report (kept: no second report), wider strokes under boxes that stay inside
    # their widened boxes (plan_per), a band behind a reusable plan
    "kept_plans": ["resize:even", "lone", "flatten:strokes_dashed_grouped", "lone", "hit_test", "reflatten:tiles:away", "lone*4", "hit_rects",
                   "reflatten:base", "lone*4", "hit_test", "capture_ptcl", "reflatten:subtile", "lone*4", "hit_frame", "reflatten:width:wide", "lone*3",
                   "select_rect", "band:rows", "lone", "hit_frame", "reflatten_groups:one_subtile", "lone*3", "hit_test", "band:whole", "burst", "hit_rects",
                   "reflatten:width:thin", "lone", "item_paths", "hit_test"],
    # a few shapes near the top, planned wide, then moved six tile rows down with every item still in the band: the kept plan's strip
    # rows that nothing reached are occupied now (the box-inside test of the reuse; a plan kept there leaves them background)
    "kept_plan_rows_that_fill": ["resize:even", "hit_test", "flatten:local_grouped", "lone", "hit_test", "reflatten:subtile", "lone*3", "hit_rects",
                                 "reflatten:tiles:away", "lone", "hit_test", "capture_ptcl", "reflatten:base", "burst", "hit_frame", "reflatten_groups:one_far",
                                 "lone*3", "select_rect", "reflatten:tiles:away", "inflight", "reflatten:subtile", "lone", "item_paths", "hit_rects"],
    # Regression of the runner, found by tests/dev/fuzz_context.py at seed 2974 on the MI355X (minimised): the first frames behind a
    # resize were the two of an `inflight` observation, which did not close the plan's count of reports, and the report the plan took
    # at its third frame -- across a view change that kept it -- was counted as a second one of the scene in front of the resize.
    "plan_made_by_frames_in_flight": ["resize:even", "hit_test", "flatten:random_b_grouped", "burst", "resize:odd", "hit_test", "reflatten_groups:one_subtile", "inflight",
                                      "reflatten:subtile", "lone*4", "hit_test"],
    # the paint behind a new map, behind an upload and in the record pm_fill_coverage hands back
    "paint_over_maps_and_uploads": ["resize:odd", "hit_test", "flatten:random_b_grouped", "lone", "hit_test", "repaint:fade0", "lone", "hit_rects", "repaint:half",
                                    "fill_coverage", "lone", "hit_test", "groups:per_path", "lone", "select_rect", "reflatten:subtile", "lone*3", "hit_test",
                                    "repaint:fade0", "fill_coverage", "burst", "hit_frame", "groups:one", "inflight", "reflatten_groups:one_far", "lone",
                                    "hit_test", "upload:nested_a", "item_paths", "lone", "hit_rects", "groups:interleaved", "lone", "hit_test", "reflatten:base", "lone*3",
                                    "item_paths", "select_rect"],
}

# Rows of frame-path switches (tests/test_frame_sequences.py): a pairwise row with two frame streams and five slots, one with one
# stream and one slot, and per-tile-row item lists on every band
SWITCH_ROWS = ["pairwise02", "pairwise00", "row_lists_replan_once"]
SWITCH_SEEDS = ["kept_plans", "paint_over_maps_and_uploads", SEEDS[0]]

# Ordered pairs (state change, next state change) that preconditions exclude, each with its reason
EXCLUDED_PAIRS = {
    ("upload", "repaint"): "an uploaded scene did not come from the resident paths: pm_repaint_groups is invalid until the next re-flatten",
    ("fail", "groups"): "a failed replacement is followed by one refused operation and a recovery: a map brings no scene back",
    ("fail", "repaint"): "no scene: pm_repaint_groups is invalid (it is one of the refused operations)",
    ("fail", "resize"): "a failed replacement is followed by a recovery: a resize brings no scene back",
    ("fail", "band"): "a failed replacement is followed by a recovery: a band brings no scene back",
    ("fail", "invalid"): "a failed replacement is followed by a recovery: the refused operation behind it is the invalid call",
    ("fail", "fail"): "a replacement can fail after it started only where a scene is resident",
}

_scripts = {}
_answers = cm.Answers()


def script_of(pm, pmo, seed):
    if seed not in _scripts:
        _scripts[seed] = cm.scripted(pm, pmo, NAMED[seed], answers=_answers) if seed in NAMED else cm.generate(pm, pmo, seed, answers=_answers)
    return _scripts[seed]


def _id(seed):
    return seed if seed in NAMED else f"seed{seed:03d}"


ALL = SEEDS + list(NAMED)


# ---- -m gpu ------------------------------------------------------------------------------------------------------------------

def _run(pm, pmo, monkeypatch, script, seed, env):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pm.Renderer(0) as r:
        cm.Runner(pm, pmo, r, script, seed, answers=_answers).run()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ALL, ids=[_id(s) for s in ALL])
def test_context_sequence(pm, pmo, monkeypatch, seed):
    _run(pm, pmo, monkeypatch, script_of(pm, pmo, seed), seed, {})


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SWITCH_SEEDS, ids=[_id(s) for s in SWITCH_SEEDS])
@pytest.mark.parametrize("row", SWITCH_ROWS)
def test_context_sequence_switches(pm, pmo, monkeypatch, row, seed):
    env = {name: e for name, e, _ in ROWS}[row]
    _run(pm, pmo, monkeypatch, script_of(pm, pmo, seed), seed, {**COMMON, **env})


# ---- CPU: the conditions on the committed scripts ----------------------------------------------------------------------------------

def test_switch_rows_are_the_rows_asked_for():
    env = {name: e for name, e, _ in ROWS}
    assert (env["pairwise02"]["PM_FRAME_STREAMS"], env["pairwise02"]["PM_SLOTS"]) == ("2", "5")
    assert (env["pairwise00"]["PM_FRAME_STREAMS"], env["pairwise00"]["PM_SLOTS"]) == ("1", "1")
    assert env["row_lists_replan_once"] == {"PM_ROW_LIST_MIN_ITEMS": "10"} and COMMON == {"PM_BIN_SPLIT_SLOTS": "48"}
    assert len(SWITCH_SEEDS) == 3


def _walk(script):
    """[(state change, [observations behind it])]"""
    out = []
    for s in script:
        if s.kind in cm.STATE_OPS:
            out.append((s, []))
        else:
            out[-1][1].append(s)
    return out


def test_committed_scripts_cover_the_alphabet(pm, pmo):
    pairs, variants, first_obs, straddled, three_lone = set(), set(), set(), set(), []
    for seed in ALL:
        script = script_of(pm, pmo, seed)
        assert seed not in SEEDS or 25 <= len(script) <= 45, (seed, len(script))   # (about 30 to 40 steps; a regression is as short as it got)
        walk = _walk(script)
        n3 = 0
        for k, (s, obs) in enumerate(walk):
            variants.add((s.kind, s.variant))
            kinds = [o.kind for o in obs]
            first_obs.add((s.kind, kinds[0]))
            # behind every state change a frame and a query (with no scene resident: the one operation it must refuse)
            if s.kind != "fail" and k > 0 and seed != "plan_made_by_frames_in_flight":   # (a minimised script: what did not matter is gone)
                assert any(o in cm.FRAME_OBS or o == "capture_ptcl" for o in kinds) and any(o in cm.QUERY_OBS or o == "inflight" for o in kinds), (seed, k, s, kinds)
            n3 += kinds.count("lone") == 3 and not any(o in ("burst", "capture_ptcl", "fill_coverage") for o in kinds[: kinds.index("lone") + 3])
            if k + 1 < len(walk):
                nxt = walk[k + 1][0]
                pairs.add((s.kind, nxt.kind))
                if kinds[-1] == "inflight":
                    straddled.add(nxt.kind)
                    assert nxt.kind in cm.STRADDLERS + ("fail",) and (nxt.kind, nxt.variant) not in cm.SAME_BYTES, (seed, k, nxt)
            # (the runner compares what is in flight at the end of a script as well)
        three_lone.append(n3 if seed != "plan_made_by_frames_in_flight" else 2)
    want_pairs = set(itertools.product(cm.STATE_OPS, cm.STATE_OPS)) - set(EXCLUDED_PAIRS)
    assert not (pairs & set(EXCLUDED_PAIRS)), pairs & set(EXCLUDED_PAIRS)
    assert pairs == want_pairs, sorted(want_pairs - pairs)
    assert variants >= {(k, v) for k, vs in cm.VARIANTS.items() for v in vs}, sorted({(k, v) for k, vs in cm.VARIANTS.items() for v in vs} - variants)
    assert first_obs == set(itertools.product(cm.STATE_OPS, cm.OBS)), sorted(set(itertools.product(cm.STATE_OPS, cm.OBS)) - first_obs)
    assert set(cm.STRADDLERS) <= straddled, set(cm.STRADDLERS) - straddled
    assert min(three_lone) >= 2, three_lone   # exactly three lone frames on one plan, several times per script
    print(f"{len(ALL)} scripts, {sum(len(script_of(pm, pmo, s)) for s in ALL)} steps: {len(pairs)} of {len(want_pairs)} pairs of state changes "
          f"({len(EXCLUDED_PAIRS)} excluded), {len(variants)} variants, {len(first_obs)} (state change, observation) pairs, straddled by {sorted(straddled)}")


def test_no_step_of_a_committed_script_is_blind(pm, pmo):
    """Replay every script on the model alone: cm.blind must find nothing, for 100 % of the state changes."""
    checked = exempt = 0
    for seed in ALL:
        m = cm.Model(pm, pmo)
        walk = _walk(script_of(pm, pmo, seed))
        inflight = ()
        for s, obs in walk:
            after = m.copy()
            after.apply(s)
            if m.w:   # (the first resize has nothing in front of it)
                why = cm.blind(m, after, s, _answers, inflight)
                assert why is None, (seed, s, why)
                checked += 1
                exempt += (s.kind, s.variant) in cm.SAME_BYTES
            m = after
            inflight = tuple(o.args["skip"] for o in obs if o.kind == "inflight") if obs[-1].kind == "inflight" else ()
    print(f"{checked} state changes, none blind ({exempt} of them keep the bytes by contract: invalid calls, maps, the identity repaint, the equal table)")
    assert checked - exempt >= 5 * len(ALL)


def test_the_generator_is_deterministic(pm, pmo):
    a, b = cm.generate(pm, pmo, SEEDS[0]), cm.generate(pm, pmo, SEEDS[0])
    assert [repr(s) for s in a] == [repr(s) for s in b]
    for x, y in zip(a, b):
        assert all(np.array_equal(np.asarray(x.args[k]), np.asarray(y.args[k])) for k in x.args if k != "ps")


def _bytes_after(pm, pmo, steps):
    m = cm.Model(pm, pmo)
    out = []
    for s in steps:
        m.apply(s)
        out.append(m.expected())
    return out


def test_the_model_agrees_with_the_merged_feature_tests(pm, pmo):
    """The sequences of test_paint_stays_with_the_paths_until_new_paths_come and test_groups_equal_table_is_reflatten as scripts: the
    model's bytes are what those tests' own helpers (want_painted, expected) give at every point they check."""
    from test_groups_gpu import expected, random_table
    from test_paint_gpu import identity_table, random_paints, uniform, want_painted

    S = cm.Step
    # -- test_paint_stays_with_the_paths_until_new_paths_come --
    case = path_sets.random_case(511)
    ps, n = case.ps, len(case.ps.paths)
    gmap = np.arange(n, dtype=np.uint32) % 4
    g = int(gmap.max()) + 1
    rng = np.random.default_rng(4)
    tints, opac = random_paints(rng, g)
    aff, ws = random_table(rng, g)
    ident_t, ident_o = identity_table(g)
    flatten = S("flatten", "", {"ps": ps.with_groups(gmap), "affine": case.affine, "scale": case.scale})
    paint = S("repaint", "", {"tints": tints, "opacities": opac})
    unpaint = S("repaint", "", {"tints": ident_t, "opacities": ident_o})
    table = S("reflatten_groups", "", {"affines": aff, "scales": ws})
    view2 = S("reflatten", "", {"affine": case.affine2, "scale": 0.75})
    steps = [flatten, paint, table, unpaint, table, paint, view2, unpaint, view2, paint,
             S("groups", "", {"map": np.zeros(n, np.uint32)}), S("reflatten", "", {"affine": case.affine, "scale": case.scale}), flatten,
             S("reflatten", "", {"affine": case.affine, "scale": case.scale})]
    got = _bytes_after(pm, pmo, steps)
    unpainted = expected(pmo, ps, None, [case.affine], [case.scale])
    grouped = want_painted(pmo, ps, gmap, tints, opac, aff, ws)
    second = want_painted(pmo, ps, gmap, tints, opac, *uniform(case.affine2, 0.75, g))
    old_colours = want_painted(pmo, ps, gmap, tints, opac, *uniform(case.affine, case.scale, g))
    for k, want in ((0, unpainted), (2, grouped), (5, grouped), (6, second), (9, second), (11, old_colours), (12, unpainted), (13, unpainted)):
        assert np.array_equal(got[k][0], want[0]) and got[k][1] == want[1] and np.array_equal(got[k][2], want[2]), k
    assert np.array_equal(got[2][0], got[5][0]) and not np.array_equal(got[0][0], got[1][0])
    # -- test_groups_equal_table_is_reflatten[plain] --
    case = path_sets.random_case(321)
    ps, aff, scale = case.ps, case.affine2, 0.75
    n = len(ps.paths)
    steps = [S("flatten", "", {"ps": ps.with_groups(np.arange(n) % 3), "affine": path_sets.IDENTITY, "scale": 1.0}),
             S("reflatten", "", {"affine": aff, "scale": scale}),
             S("reflatten_groups", "", {"affines": [aff] * 3, "scales": [scale] * 3}),
             S("groups", "", {"map": np.arange(n)}),
             S("reflatten_groups", "", {"affines": [aff] * (n + 2), "scales": [scale] * (n + 2)})]
    got = _bytes_after(pm, pmo, steps)
    want = expected(pmo, ps, None, [aff], [scale])
    for k in (1, 2, 3, 4):
        assert np.array_equal(got[k][0], want[0]) and got[k][1] == want[1] and np.array_equal(got[k][2], want[2]), k


# ---- CPU: the gpu part under the wave64 emulation -----------------------------------------------------------------------------------

EMU_TWO_CUS = ["kept_plans", "paint_over_maps_and_uploads", SEEDS[0], SEEDS[1]]


def _emulated(k, n, extra=None):
    env = dict(os.environ, PM_TEST_EMU="1", **(extra or {}))
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-k", k, "-p", "no:cacheprovider", "-n", "4"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=3000)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert f"{n} passed" in p.stdout and "failed" not in p.stdout and "skipped" not in p.stdout, p.stdout[-2000:]


def test_context_sequences_under_wave64_emulation(built):
    """The -m gpu tests above -- the functions the GPU box runs -- against the emulated library: every script at the default device,
    the switch rows too, and two scripts on a two-CU device (a binning grid smaller than the frames' strip rows: chains everywhere)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the gpu-marked tests run on the real library")
    _emulated("test_context_sequence", len(ALL) + len(SWITCH_ROWS) * len(SWITCH_SEEDS))
    two = " or ".join(_id(s) for s in EMU_TWO_CUS)
    _emulated(f"test_context_sequence and not switches and ({two})", len(EMU_TWO_CUS), {"PM_EMU_CUS": "2"})
