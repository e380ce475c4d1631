"""Times the polygon queries against the rectangle queries (needs a GPU; not a pytest, not bench.py).

Scene: the Tiger flattened on the device, at 3840 x 2160 and at 1920 x 1080.
  A   pm_select_rect_device: the whole view, a quarter of it (its middle), a 32 px square at its centre
  B   pm_select_polygon_device on the same rectangle given as a 4-gon
  L   pm_select_polygon_device alone on a lasso of 64 and of 1024 vertices around the middle quarter
Before any timing the words of B are compared with A's: the script prints how many items the two touch and on how many the touch
bits differ (in real arithmetic none; strokes may differ in the last bit at exactly hw) -- it does not require none.
Then A and B alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a
second, timed with events on the stream the calls run on.  L is timed the same way, alone.

Prints one JSON line per (size, marquee) and per (size, lasso): medians, spreads (max - min over the rounds) and the ratio B / A.
No bar is set: the figures are for DESIGN.md 5.

    python tests/dev/time_hit_poly.py [ROUNDS]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOW_S = 0.3   # what a timed window should last at least


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_hit_poly needs a GPU", file=sys.stderr)
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
            words_a = torch.empty(n_items, dtype=torch.int32, device="cuda")
            words_b = torch.empty(n_items, dtype=torch.int32, device="cuda")
            stream.synchronize()
            marquees = {"whole view": (0.0, 0.0, float(W), float(H)), "quarter": (W / 4.0, H / 4.0, 3.0 * W / 4.0, 3.0 * H / 4.0),
                        "32 px": (W / 2.0 - 16.0, H / 2.0 - 16.0, W / 2.0 + 16.0, H / 2.0 + 16.0)}
            for name, m in marquees.items():
                gon = np.array([[m[0], m[1]], [m[2], m[1]], [m[2], m[3]], [m[0], m[3]]], np.float32)
                fa = lambda: r.select_rect_tensor(*m, words_a, stream=stream)   # noqa: E731
                fb = lambda: r.select_polygon_tensor(gon, words_b, stream=stream)   # noqa: E731
                fa()
                fb()
                stream.synchronize()
                wa, wb = words_a.cpu().numpy(), words_b.cpu().numpy()
                ra, rb = reps_for(fa), reps_for(fb)
                a_ms, b_ms = [], []
                for _ in range(rounds):
                    a_ms.append(timed(fa, ra))
                    b_ms.append(timed(fb, rb))
                print(json.dumps({
                    "view": f"{W}x{H}", "items": n_items, "marquee": name, "rect": m, "rounds": rounds, "reps_a": ra, "reps_b": rb,
                    "a_touched": int((wa & 1).sum()), "b_touched": int((wb & 1).sum()), "touch_bits_that_differ": int(((wa ^ wb) & 1).sum()),
                    "a_enclosed": int(((wa & 2) != 0).sum()), "b_enclosed": int(((wb & 2) != 0).sum()),
                    "a_ms": [round(v, 5) for v in a_ms], "b_ms": [round(v, 5) for v in b_ms],
                    "a_median_ms": round(statistics.median(a_ms), 5), "b_median_ms": round(statistics.median(b_ms), 5),
                    "a_spread_ms": round(max(a_ms) - min(a_ms), 5), "b_spread_ms": round(max(b_ms) - min(b_ms), 5),
                    "ratio_b_over_a": round(statistics.median(b_ms) / statistics.median(a_ms), 2)}), flush=True)
            for n_v in (64, 1024):
                t = np.arange(n_v) * (2.0 * np.pi / n_v)
                wob = 1.0 + 0.08 * np.sin(7.0 * t)
                lasso = np.stack([W / 2.0 + W / 4.0 * wob * np.cos(t), H / 2.0 + H / 4.0 * wob * np.sin(t)], axis=1).astype(np.float32)
                fl = lambda: r.select_polygon_tensor(lasso, words_b, stream=stream)   # noqa: E731
                rl = reps_for(fl)
                l_ms = [timed(fl, rl) for _ in range(rounds)]
                w = words_b.cpu().numpy()
                print(json.dumps({
                    "view": f"{W}x{H}", "items": n_items, "lasso_vertices": n_v, "rounds": rounds, "reps": rl,
                    "touched": int((w & 1).sum()), "enclosed": int(((w & 2) != 0).sum()),
                    "l_ms": [round(v, 5) for v in l_ms], "l_median_ms": round(statistics.median(l_ms), 5), "l_spread_ms": round(max(l_ms) - min(l_ms), 5)}),
                    flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
