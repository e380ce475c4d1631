"""Times the path-measurement queries beside pm_item_bounds and pm_snap on the same scenes, for scale (needs a GPU; not a pytest,
not bench.py).

Scenes: the Tiger flattened on the device at 3840 x 2160 and the 20 000 glyph-like paths of workloads.heldout_glyphs.  Device
calls, all on one caller's stream:
  L   pm_item_lengths_device: a record per item
  PA  pm_points_at_length_device: N_QUERIES positions spread over all items (query j: item j mod n_items, a seeded fraction of its
      length)
  PL  pm_points_at_length_device: N_QUERIES seeded positions on the longest item
  E   pm_positions_on_edges_device on PA's own answers (item, index, t)
  B   pm_item_bounds_device -- the yardstick of L: the same deal of the items, chunk boxes instead of points
  S   pm_snap_device, N_QUERIES queries of radius 4 at PA's own points -- the yardstick of PA: a wave per query over all items
The six alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a second,
timed with events on the stream the calls run on.  Prints one JSON line per scene: medians and spreads (max - min over the
rounds).  Before any timing the lengths and a sample of the points are compared with tests/np_measure on the downloaded scene: what
is timed is what is tested.

No bar is set: the figures are for DESIGN.md 5.

    python tests/dev/time_measure.py [ROUNDS]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S = 0.3   # what a timed window should last at least
N_QUERIES = 100_000
SAMPLE = 400     # point answers compared with np_measure


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_measure needs a GPU", file=sys.stderr)
        return 2
    import np_measure as nm
    import piet_metal_amd as pm

    stream = torch.cuda.Stream()

    def timed(fn, reps):
        """ms per call over `reps` calls, device time between two events on the stream."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / reps

    def reps_for(fn):
        fn()
        stream.synchronize()
        once = timed(fn, 1)   # warmed up by the call before
        return max(1, int(np.ceil(WINDOW_S * 1e3 / max(once, 1e-3))))

    def queries(items, s):
        q = np.zeros(len(items), nm.LENGTH_QUERY)
        q["item"], q["s"] = items, s
        return q, torch.from_numpy(q.view(np.int32).reshape(-1, 4).copy()).cuda()

    scenes = [("tiger", pm.workloads.tiger(3840, 2160)), ("glyphs", pm.workloads.heldout_glyphs())]
    for name, wl in scenes:
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            lengths = r.item_lengths()
            rng = np.random.default_rng(25)
            frac = rng.random(N_QUERIES)
            items = (np.arange(N_QUERIES) % n_items).astype(np.uint32)
            total = lengths["length"].astype(np.float64)
            q_all, d_all = queries(items, np.floor(frac * total[items]).astype(np.uint64))
            longest = int(np.argmax(lengths["length"]))
            q_long, d_long = queries(np.full(N_QUERIES, longest, np.uint32), np.floor(frac * total[longest]).astype(np.uint64))
            rec_len = torch.empty((n_items, 4), dtype=torch.int32, device="cuda")
            boxes = torch.empty((n_items, 4), dtype=torch.float64, device="cuda")
            pts_all = torch.empty((N_QUERIES, 8), dtype=torch.int32, device="cuda")
            pts_long = torch.empty((N_QUERIES, 8), dtype=torch.int32, device="cuda")
            back = torch.empty((N_QUERIES, 4), dtype=torch.int32, device="cuda")
            snapped = torch.empty((N_QUERIES, 8), dtype=torch.int32, device="cuda")
            r.points_at_length_tensor(d_all, pts_all, stream=stream)
            stream.synchronize()
            edge_q = torch.stack([pts_all[:, 0], pts_all[:, 2], pts_all[:, 3], torch.zeros_like(pts_all[:, 0])], dim=1).contiguous()
            xyr = torch.cat([pts_all[:, 4:6].view(torch.float32), torch.full((N_QUERIES, 1), 4.0, device="cuda")], dim=1).contiguous()
            stream.synchronize()
            calls = {
                "item_lengths": lambda: r.item_lengths_tensor(rec_len, stream=stream),
                "points_over_all_items": lambda: r.points_at_length_tensor(d_all, pts_all, stream=stream),
                "points_on_the_longest_item": lambda: r.points_at_length_tensor(d_long, pts_long, stream=stream),
                "positions_on_edges": lambda: r.positions_on_edges_tensor(edge_q, back, stream=stream),
                "item_bounds": lambda: r.item_bounds_tensor(boxes, stream=stream),
                "snap_radius_4": lambda: r.snap_tensor(xyr, snapped, stream=stream),
            }
            reps = {k: reps_for(fn) for k, fn in calls.items()}
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(timed(fn, reps[k]))
            stream.synchronize()
            scene = r.download_scene()
            ws = nm.walks(scene)
            assert rec_len.cpu().numpy().tobytes() == nm.item_lengths(scene, ws=ws).tobytes()
            pick = rng.choice(N_QUERIES, SAMPLE, replace=False)
            for q, got in ((q_all, pts_all), (q_long, pts_long)):
                want = nm.points_at_length(scene, list(zip(q["item"][pick], q["s"][pick])), ws=ws)
                assert got.cpu().numpy().view(nm.LENGTH_POINT).reshape(-1)[pick].tobytes() == want.tobytes()
            rec = {"scene": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "scene_bytes": int(len(scene)), "queries": N_QUERIES, "rounds": rounds, "reps": reps,
                   "segments": int(lengths["n_segments"].sum()), "longest_item_segments": int(lengths["n_segments"][longest])}
            for k in calls:
                rec[k + "_ms"] = [round(v, 5) for v in ms[k]]
                rec[k + "_median_ms"] = round(statistics.median(ms[k]), 5)
                rec[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 5)
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
