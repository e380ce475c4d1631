"""Frame-path switches in combination, over sequences of frames (-m gpu; tests/test_emu_cpu.py runs it under the CPU emulation).

Every row of ROWS is a set of PM_* switches, read once by pm_create; every row runs the script of tests/frame_sequences.py --
lone frames, the third-frame re-plan, bursts of frames in flight, a band, a scene switch, a resize to a viewport that is not a
multiple of a tile, geometry far outside the viewport, the device flatten and a view change -- against the oracle.  The first
rows are a pairwise covering array over FACTORS (generated once, kept as literals so that the test ids stay put; the CPU test
below checks the covering), then a row per bug the sequences found, and one whose command-list arena overflows in its last,
larger scene, after every earlier frame fitted (asserted)."""
import itertools
import os
import zlib

import pytest

from frame_sequences import FrameSequence

FACTORS = {
    "PM_BIN_SPLIT": ("0", "1", "2"),
    "PM_HANDOUT": ("0", "1", "2"),
    "PM_BIN_WG_PER_CU": (None, "1"),
    "PM_BIN_WAVES": (None, "1", "4"),
    "PM_ROW_LIST_MIN_ITEMS": (None, "1"),
    "PM_FUSED": ("0", "1"),
    "PM_FOLD_CLEAR": (None, "0", "1"),
    "PM_FINE_SPLIT": ("0", "1"),
    ("PM_FRAME_STREAMS", "PM_SLOTS"): (None, ("1", "1"), ("2", "5")),
}

# (every row: a strip row with 48 segment slots counts as heavy, so that mode 1 finds rows to cut in these small frames)
COMMON = {"PM_BIN_SPLIT_SLOTS": "48"}

_PAIRWISE = [  # in FACTORS' order
    ("1", "0", None, None, "1", "1", "0", "0", ("1", "1")),
    ("2", "1", "1", "1", None, "0", "1", "1", ("1", "1")),
    ("0", "1", "1", "4", "1", "1", None, "1", ("2", "5")),
    ("1", "2", None, None, None, "0", None, "0", None),
    ("0", "0", None, "4", None, "0", "0", "1", None),
    ("2", "2", None, "4", "1", "0", "1", "0", ("2", "5")),
    ("2", "1", "1", "1", "1", "1", "0", "0", None),
    ("1", "2", "1", None, None, "1", "0", "1", ("2", "5")),
    ("0", "2", None, "1", None, "1", None, "0", ("1", "1")),
    ("1", "0", "1", "1", None, "1", "1", "1", ("2", "5")),
    ("0", "1", None, None, None, "1", "1", "1", None),
    ("2", "0", "1", None, "1", "1", None, "0", None),
    ("1", "1", "1", "4", None, "0", "1", "0", ("1", "1")),
]


def _env(values):
    env = {}
    for key, v in zip(FACTORS, values):
        if v is None:
            continue
        env.update(zip(key, v) if isinstance(key, tuple) else [(key, v)])
    return env


# (name, switches, options of FrameSequence)
ROWS = [(f"pairwise{k:02d}", _env(v), {}) for k, v in enumerate(_PAIRWISE)] + [
    # PM_BIN_SPLIT=2 with static hand-out, more strip rows than the binning grid: frames bound to the work list without the cuts
    # walked no chains, and the rows past the grid were never binned (the 1080p Tiger's 544 rows against 256 workgroups; under
    # the emulation on two CUs every frame of the script)
    ("split2_static_handout_rows_beyond_grid", {"PM_BIN_SPLIT": "2", "PM_HANDOUT": "1", "PM_BIN_WG_PER_CU": "1"}, {"big": (1920, 1080)}),
    # per-tile-row item lists (every band of the script has more than ten items): the plan was remade from the frames' report
    # every third frame, forever (pixels right, pipeline drained each time)
    ("row_lists_replan_once", {"PM_ROW_LIST_MIN_ITEMS": "10"}, {"row_lists": True}),
    # seven binning workgroups per CU: a plan with too many strip rows to cut (five per CU) but few enough for the report to be
    # read back (seven) -- the band's twelve strip rows on two CUs -- was remade from it every third frame as well
    ("wide_grid_replan_once", {"PM_BIN_WG_PER_CU": "7"}, {}),
    # the command-list arena holds every scene of the script but the last, larger one: it overflows there, with frames in
    # flight, after plans, bands and scenes came and went, grows and renders every frame again
    ("ptcl_overflow_midsequence", {"PM_PTCL_INITIAL_CMDS": "330000"}, {"big": (2560, 1440), "overflow_late": True}),
]

_ENV_KEYS = {k for key in FACTORS for k in (key if isinstance(key, tuple) else (key,))} | {"PM_PTCL_INITIAL_CMDS"} | set(COMMON)


def _n_cus():
    if os.environ.get("PM_TEST_EMU") == "1":  # (the CPU emulation, tests/emu/: its "device" has PM_EMU_CUS compute units)
        return max(1, int(os.environ.get("PM_EMU_CUS", "256")))
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def test_pairwise_rows_cover_every_pair_of_values():
    idx = [{v: i for i, v in enumerate(vals)} for vals in FACTORS.values()]
    rows = [[idx[f][v] for f, v in enumerate(row)] for row in _PAIRWISE]
    sizes = [len(vals) for vals in FACTORS.values()]
    for i, j in itertools.combinations(range(len(sizes)), 2):
        seen = {(row[i], row[j]) for row in rows}
        assert len(seen) == sizes[i] * sizes[j], (list(FACTORS)[i], list(FACTORS)[j])


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,opts", ROWS, ids=[r[0] for r in ROWS])
def test_frame_sequence(pm, pmo, monkeypatch, name, env, opts):
    """Regressions (piet_metal_amd/csrc/pm_context.hip):
    - split2_static_handout_rows_beyond_grid: the list without the cuts had no chain links; EnsureArena now links it for the
      plan's grid.
    - row_lists_replan_once: FeedBackStripRows re-planned every third frame on scenes with per-tile-row item lists; it now
      leaves such plans alone.
    - wide_grid_replan_once: so it did for plans with too many strip rows to cut; EnsureArena now marks a plan made with the
      report whether or not it cut, so a report is used at most once per plan."""
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**COMMON, **env}.items():
        monkeypatch.setenv(k, v)
    wg = env.get("PM_BIN_WG_PER_CU")
    r = pm.Renderer(0)
    try:
        FrameSequence(pm, pmo, r, seed=zlib.crc32(name.encode()), split_mode=int(env.get("PM_BIN_SPLIT", "1")),
                      row_lists=opts.get("row_lists", env.get("PM_ROW_LIST_MIN_ITEMS") == "1"),
                      feedback_grid=_n_cus() * (max(1, int(wg)) if wg else 5), big=opts.get("big"),
                      overflow_late=opts.get("overflow_late", False)).run()
    finally:
        r.close()
