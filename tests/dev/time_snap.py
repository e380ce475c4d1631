"""Times snapping against a pick with the same tolerance (needs a GPU; not a pytest, not bench.py).

Many queries.  Scene: the Tiger flattened on the device, at 3840 x 2160 and at 1920 x 1080; 100 000 seeded cursors of the view.
  P   pm_hit_rects_device on the pick squares of the cursors, half side r (what Renderer.pick asks), without counts: one wave per square
  S   pm_snap_device on {x, y, r} for the same cursors, for vertices, for edges and for both: one wave per query
for r = 2, 8 and 32 px.  P and S alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good
fraction of a second, timed with events on the stream the calls run on.  Prints one JSON line per (size, r, what): medians, spreads
(max - min over the rounds), how many queries found something, and the ratio S / P.

One query.  The lone-cursor latency of the HOST call pm_snap (staging, launch, read-back, synchronisation: what a single mouse move
pays), wall clock over LONE_CALLS calls at the centre of the view, r = 8, both kinds, against Renderer.pick there -- on the Tiger
and on the 20 000 glyph-like paths of workloads.heldout_glyphs at 3840 x 2160.  One wave walks all the items: this is the figure the
wave-per-query design costs a lone cursor.

No bar is set: the figures are for DESIGN.md 5.

    python tests/dev/time_snap.py [ROUNDS]"""
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
WHAT = {"vertices": (True, False), "edges": (False, True), "both": (True, True)}


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_snap needs a GPU", file=sys.stderr)
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
            top = torch.empty(N_CURSORS, dtype=torch.int32, device="cuda")
            out = torch.empty((N_CURSORS, 8), dtype=torch.int32, device="cuda")
            stream.synchronize()
            for rad in (2.0, 8.0, 32.0):
                t = np.float32(rad)
                rects = torch.from_numpy(np.concatenate([pts - t, pts + t], axis=1).astype(np.float32)).cuda()
                xyr = torch.from_numpy(np.concatenate([pts, np.full((N_CURSORS, 1), t, np.float32)], axis=1)).cuda()
                fp = lambda: r.hit_rects_tensor(rects, top, None, stream=stream)   # noqa: E731
                for what, (vertices, edges) in WHAT.items():
                    fs = lambda: r.snap_tensor(xyr, out, stream=stream, vertices=vertices, edges=edges)   # noqa: E731
                    fp()
                    fs()
                    stream.synchronize()
                    found = int((out[:, 0] != -1).sum())
                    picked = int((top != -1).sum())
                    rp, rs = reps_for(fp), reps_for(fs)
                    p_ms, s_ms = [], []
                    for _ in range(rounds):
                        p_ms.append(timed(fp, rp))
                        s_ms.append(timed(fs, rs))
                    print(json.dumps({
                        "view": f"{W}x{H}", "items": n_items, "cursors": N_CURSORS, "r": rad, "snap_to": what, "rounds": rounds, "reps_pick": rp, "reps_snap": rs,
                        "picks_that_name_an_item": picked, "snaps_that_find_something": found,
                        "pick_ms": [round(v, 4) for v in p_ms], "snap_ms": [round(v, 4) for v in s_ms],
                        "pick_median_ms": round(statistics.median(p_ms), 4), "snap_median_ms": round(statistics.median(s_ms), 4),
                        "pick_spread_ms": round(max(p_ms) - min(p_ms), 4), "snap_spread_ms": round(max(s_ms) - min(s_ms), 4),
                        "ratio_snap_over_pick": round(statistics.median(s_ms) / statistics.median(p_ms), 2)}), flush=True)
    for name, wl in (("tiger", pm.workloads.tiger(3840, 2160)), ("glyphs", pm.workloads.heldout_glyphs())):
        with pm.Renderer(0) as r:
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            centre = np.array([[wl.width / 2.0, wl.height / 2.0]], np.float32)
            s_ms = lone(lambda: r.snap(centre, 8.0))
            p_ms = lone(lambda: r.pick(centre, 8.0))
            rec = r.snap(centre, 8.0)[0]
            print(json.dumps({
                "lone_cursor": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "r": 8.0, "calls": LONE_CALLS,
                "found_item": int(rec["item"]), "kind": int(rec["kind"]),
                "snap_median_ms": round(statistics.median(s_ms), 4), "snap_p10_ms": round(float(np.percentile(s_ms, 10)), 4), "snap_p90_ms": round(float(np.percentile(s_ms, 90)), 4),
                "pick_median_ms": round(statistics.median(p_ms), 4), "pick_p10_ms": round(float(np.percentile(p_ms, 10)), 4), "pick_p90_ms": round(float(np.percentile(p_ms, 90)), 4),
                "ratio_snap_over_pick": round(statistics.median(s_ms) / statistics.median(p_ms), 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
