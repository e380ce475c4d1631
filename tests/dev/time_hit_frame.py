"""Times the item map against what it replaces (needs a GPU; not a pytest, not bench.py).

Scene: the Tiger flattened on the device, at 3840 x 2160 and at 1920 x 1080.
  A  pm_hit_test_device on all W * H pixel centres, the points made on the device: one wave per pixel
  B  pm_hit_frame_device on the whole view: one workgroup per 16 x 16 tile
Before any timing A's and B's outputs are compared word for word at the full size.  Then A and B alternate ROUNDS times in this one
process, each window a batch of calls long enough to last a good fraction of a second, timed with events on the stream the calls run
on; with and without counts.  For scale only, the frame time of the same view is measured the same way.

Prints one JSON line per (size, counts) and a verdict: B must be faster than A in EVERY alternation.  Exit status 1 if it is not.

    python tests/dev/time_hit_frame.py [ROUNDS]"""
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
        print("time_hit_frame needs a GPU", file=sys.stderr)
        return 2
    import piet_metal_amd as pm

    stream = torch.cuda.Stream()
    ok = True

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
            r.resize(W, H)
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
            xy = torch.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], dim=1).contiguous()
            top_a = torch.empty(W * H, dtype=torch.int32, device="cuda")
            cnt_a = torch.empty(W * H, dtype=torch.int32, device="cuda")
            top_b = torch.empty((H, W), dtype=torch.int32, device="cuda")
            cnt_b = torch.empty((H, W), dtype=torch.int32, device="cuda")
            stream.synchronize()
            # equal word for word, with counts and in the walk that ends at the first hit
            r.hit_test_tensor(xy, top_a, cnt_a, stream=stream)
            r.hit_frame_tensor(top_b, cnt_b, stream=stream)
            stream.synchronize()
            assert torch.equal(top_a.view(H, W), top_b) and torch.equal(cnt_a.view(H, W), cnt_b), "A and B differ (counts)"
            top_a.fill_(-2)
            top_b.fill_(-3)
            r.hit_test_tensor(xy, top_a, None, stream=stream)
            r.hit_frame_tensor(top_b, None, stream=stream)
            stream.synchronize()
            assert torch.equal(top_a.view(H, W), top_b), "A and B differ (first hit)"
            visible = int(torch.unique(top_b).numel())
            for counts in (False, True):
                fa = lambda: r.hit_test_tensor(xy, top_a, cnt_a if counts else None, stream=stream)   # noqa: E731
                fb = lambda: r.hit_frame_tensor(top_b, cnt_b if counts else None, stream=stream)      # noqa: E731
                ra, rb = reps_for(fa), reps_for(fb)
                a_ms, b_ms = [], []
                for _ in range(rounds):
                    a_ms.append(timed(fa, ra))
                    b_ms.append(timed(fb, rb))
                faster = all(b < a for a, b in zip(a_ms, b_ms))
                ok = ok and faster
                print(json.dumps({
                    "view": f"{W}x{H}", "items": n_items, "values_in_map": visible, "counts": counts, "rounds": rounds, "reps_a": ra, "reps_b": rb,
                    "a_ms": [round(v, 4) for v in a_ms], "b_ms": [round(v, 4) for v in b_ms],
                    "a_median_ms": round(statistics.median(a_ms), 4), "b_median_ms": round(statistics.median(b_ms), 4),
                    "a_spread_ms": round(max(a_ms) - min(a_ms), 4), "b_spread_ms": round(max(b_ms) - min(b_ms), 4),
                    "ratio_a_over_b": round(statistics.median(a_ms) / statistics.median(b_ms), 2), "b_faster_in_every_round": faster}), flush=True)
            # for scale only: the frame of the same view, on the context's own stream
            r.render()
            r.sync()
            lat = r.frame_latency(50)
            print(json.dumps({"view": f"{W}x{H}", "frame_median_ms": round(lat["median_ms"], 4), "frame_min_ms": round(lat["min_ms"], 4)}), flush=True)
    print("verdict: B (pm_hit_frame_device) is faster than A (pm_hit_test_device on every pixel centre) in every alternation" if ok
          else "verdict: B is NOT faster than A in every alternation")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
