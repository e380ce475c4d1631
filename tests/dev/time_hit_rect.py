"""Times the rectangle queries against point hit testing (needs a GPU; not a pytest, not bench.py).

Scene: the Tiger flattened on the device, at 3840 x 2160 and at 1920 x 1080.
  A   pm_hit_test_device on 100 000 seeded points of the view: one wave per point
  B   pm_hit_rects_device on the pick squares of the same points, tolerance 0, 2 and 8 px: one wave per rectangle
  S   pm_select_rect_device: the whole view, a quarter of it (its middle), a 32 px square at its centre
Before any timing B at tolerance 0 is compared with A: a point rectangle touches whatever contains the point (and, being closed, the
edges D13 leaves out -- the script prints how many of the 100 000 answers differ, it does not require none).  Then A and B alternate
ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a second, timed with events on
the stream the calls run on; B without counts, as a pick is made.  S is timed the same way, alone.

Prints one JSON line per (size, tolerance) and per (size, marquee): medians, spreads (max - min over the rounds) and the ratio B / A.
No bar is set: the figures are for DESIGN.md 5.

    python tests/dev/time_hit_rect.py [ROUNDS]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOW_S = 0.3   # what a timed window should last at least
N_PICKS = 100_000


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_hit_rect needs a GPU", file=sys.stderr)
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

    for W, H in ((3840, 2160), (1920, 1080)):
        wl = pm.workloads.tiger(W, H)
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            pts = (np.random.default_rng(7).uniform(0.0, 1.0, (N_PICKS, 2)) * (W, H)).astype(np.float32)
            xy = torch.from_numpy(pts).cuda()
            top_a = torch.empty(N_PICKS, dtype=torch.int32, device="cuda")
            top_b = torch.empty(N_PICKS, dtype=torch.int32, device="cuda")
            words = torch.empty(n_items, dtype=torch.int32, device="cuda")
            stream.synchronize()
            fa = lambda: r.hit_test_tensor(xy, top_a, None, stream=stream)   # noqa: E731
            for tol in (0.0, 2.0, 8.0):
                t = np.float32(tol)
                rects = torch.from_numpy(np.concatenate([pts - t, pts + t], axis=1).astype(np.float32)).cuda()   # what Renderer.pick asks
                fb = lambda: r.hit_rects_tensor(rects, top_b, None, stream=stream)   # noqa: E731
                fa()
                fb()
                stream.synchronize()
                differ = int((top_a != top_b).sum())
                named = int((top_b != -1).sum())
                ra, rb = reps_for(fa), reps_for(fb)
                a_ms, b_ms = [], []
                for _ in range(rounds):
                    a_ms.append(timed(fa, ra))
                    b_ms.append(timed(fb, rb))
                print(json.dumps({
                    "view": f"{W}x{H}", "items": n_items, "picks": N_PICKS, "tolerance": tol, "rounds": rounds, "reps_a": ra, "reps_b": rb,
                    "picks_that_name_an_item": named, "answers_other_than_the_point_pick": differ,
                    "a_ms": [round(v, 4) for v in a_ms], "b_ms": [round(v, 4) for v in b_ms],
                    "a_median_ms": round(statistics.median(a_ms), 4), "b_median_ms": round(statistics.median(b_ms), 4),
                    "a_spread_ms": round(max(a_ms) - min(a_ms), 4), "b_spread_ms": round(max(b_ms) - min(b_ms), 4),
                    "ratio_b_over_a": round(statistics.median(b_ms) / statistics.median(a_ms), 2)}), flush=True)
            marquees = {"whole view": (0.0, 0.0, float(W), float(H)), "quarter": (W / 4.0, H / 4.0, 3.0 * W / 4.0, 3.0 * H / 4.0),
                        "32 px": (W / 2.0 - 16.0, H / 2.0 - 16.0, W / 2.0 + 16.0, H / 2.0 + 16.0)}
            for name, m in marquees.items():
                fs = lambda: r.select_rect_tensor(*m, words, stream=stream)   # noqa: E731
                rs = reps_for(fs)
                s_ms = [timed(fs, rs) for _ in range(rounds)]
                w = words.cpu().numpy()
                print(json.dumps({
                    "view": f"{W}x{H}", "items": n_items, "marquee": name, "rect": m, "rounds": rounds, "reps": rs,
                    "touched": int((w & 1).sum()), "enclosed": int(((w & 2) != 0).sum()),
                    "s_ms": [round(v, 5) for v in s_ms], "s_median_ms": round(statistics.median(s_ms), 5), "s_spread_ms": round(max(s_ms) - min(s_ms), 5)}),
                    flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
