"""Times snapping to intersections against snapping to edges (needs a GPU; not a pytest, not bench.py).

Many queries.  Scene: the Tiger flattened on the device, at 3840 x 2160 and at 1920 x 1080; 100 000 seeded cursors of the view.
  E   pm_snap_device with PM_SNAP_EDGES alone on {x, y, r}: one wave per query, the item walk and nothing else -- the yardstick
  X   pm_snap_intersections_device on the very same queries: the same walk, the near list in LDS, the pairs
for r = 2, 8 and 32 px.  E and X alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good
fraction of a second, timed with events on the stream the calls run on.  Prints one JSON line per (size, r): medians, spreads (max - min
over the rounds), how many cursors found a crossing, the share that answered PM_SNAP_KIND_TOO_MANY, the largest and the median n_near
-- the evidence for or against the cap of 512 near edges --, and the ratio X / E.

One query.  The lone-cursor latency of the HOST call pm_snap_intersections (staging, launch, read-back, synchronisation), wall clock
over LONE_CALLS calls at the centre of the view, r = 8, against pm_snap's there -- on the Tiger and on the 20 000 glyph-like paths of
workloads.heldout_glyphs at 3840 x 2160.

No bar is set: the figures are for DESIGN.md 5.

    python tests/dev/time_snap_cross.py [ROUNDS]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOW_S = 0.3   # what a timed window should last at least
N_CURSORS = 100_000
LONE_CALLS = 200


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_snap_cross needs a GPU", file=sys.stderr)
        return 2
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

    def lone(fn):
        """ms per call, wall clock, of a synchronous host call."""
        for _ in range(10):
            fn()
        t = []
        for _ in range(LONE_CALLS):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return t

    for W, H in ((3840, 2160), (1920, 1080)):
        wl = pm.workloads.tiger(W, H)
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            pts = (np.random.default_rng(7).uniform(0.0, 1.0, (N_CURSORS, 2)) * (W, H)).astype(np.float32)
            edge = torch.empty((N_CURSORS, 8), dtype=torch.int32, device="cuda")
            out = torch.empty((N_CURSORS, 12), dtype=torch.int32, device="cuda")
            stream.synchronize()
            for rad in (2.0, 8.0, 32.0):
                xyr = torch.from_numpy(np.concatenate([pts, np.full((N_CURSORS, 1), np.float32(rad), np.float32)], axis=1)).cuda()
                fe = lambda: r.snap_tensor(xyr, edge, stream=stream, vertices=False, edges=True)   # noqa: E731
                fx = lambda: r.snap_intersections_tensor(xyr, out, stream=stream)   # noqa: E731
                fe()
                fx()
                stream.synchronize()
                rec = out.cpu().numpy().view(pm.renderer.SNAP_CROSS_DTYPE).reshape(-1)
                re_, rx = reps_for(fe), reps_for(fx)
                e_ms, x_ms = [], []
                for _ in range(rounds):
                    e_ms.append(timed(fe, re_))
                    x_ms.append(timed(fx, rx))
                print(json.dumps({
                    "view": f"{W}x{H}", "items": n_items, "cursors": N_CURSORS, "r": rad, "rounds": rounds, "reps_edges": re_, "reps_cross": rx,
                    "edge_snaps_that_find_something": int((edge[:, 0] != -1).sum()), "cursors_with_a_crossing": int((rec["kind"] == 3).sum()),
                    "share_too_many": round(float((rec["kind"] == 4).mean()), 6), "largest_n_near": int(rec["n_near"].max()),
                    "median_n_near": float(np.median(rec["n_near"])), "p99_n_near": float(np.percentile(rec["n_near"], 99)),
                    "edges_ms": [round(v, 4) for v in e_ms], "cross_ms": [round(v, 4) for v in x_ms],
                    "edges_median_ms": round(statistics.median(e_ms), 4), "cross_median_ms": round(statistics.median(x_ms), 4),
                    "edges_spread_ms": round(max(e_ms) - min(e_ms), 4), "cross_spread_ms": round(max(x_ms) - min(x_ms), 4),
                    "ratio_cross_over_edges": round(statistics.median(x_ms) / statistics.median(e_ms), 2)}), flush=True)
    for name, wl in (("tiger", pm.workloads.tiger(3840, 2160)), ("glyphs", pm.workloads.heldout_glyphs())):
        with pm.Renderer(0) as r:
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            centre = np.array([[wl.width / 2.0, wl.height / 2.0]], np.float32)
            x_ms = lone(lambda: r.snap_intersections(centre, 8.0))
            s_ms = lone(lambda: r.snap(centre, 8.0))
            rec = r.snap_intersections(centre, 8.0)[0]
            print(json.dumps({
                "lone_cursor": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "r": 8.0, "calls": LONE_CALLS,
                "found_item": int(rec["item"]), "kind": int(rec["kind"]), "n_near": int(rec["n_near"]),
                "cross_median_ms": round(statistics.median(x_ms), 4), "cross_p10_ms": round(float(np.percentile(x_ms, 10)), 4), "cross_p90_ms": round(float(np.percentile(x_ms, 90)), 4),
                "snap_median_ms": round(statistics.median(s_ms), 4), "snap_p10_ms": round(float(np.percentile(s_ms, 10)), 4), "snap_p90_ms": round(float(np.percentile(s_ms, 90)), 4),
                "ratio_cross_over_snap": round(statistics.median(x_ms) / statistics.median(s_ms), 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
