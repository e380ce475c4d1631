"""Times the bounds queries against a marquee over the whole view and against the host route they replace (needs a GPU; not a
pytest, not bench.py).

Scenes: the Tiger flattened on the device at 3840 x 2160 and at 1920 x 1080, and the 20 000 glyph-like paths of
workloads.heldout_glyphs at 3840 x 2160.  Device calls, all on one caller's stream:
  I   pm_item_bounds_device: a record per item
  U1  pm_union_bounds_device with one label: the scene's box and size (three launches)
  UG  pm_union_bounds_device with a label per path (item_paths on the device): a box per path
  S   pm_select_rect_device of the whole view -- the yardstick: it walks the same items and additionally tests their segments and
      asks every point whether the rectangle encloses it
The four alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a second,
timed with events on the stream the calls run on.  Prints one JSON line per scene: medians, spreads (max - min over the rounds)
and the ratios to S.

The host route: Renderer.download_scene (a synchronous copy of the scene) and tests/np_bounds.item_bounds on the bytes (numpy's
min / max per item), wall clock over HOST_CALLS calls, against the host calls Renderer.item_bounds and Renderer.selection_bounds
(staging, launch, read-back, synchronisation).

No bar is set: the figures are for DESIGN.md 5.

    python tests/dev/time_bounds.py [ROUNDS]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S = 0.3   # what a timed window should last at least
HOST_CALLS = 20


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_bounds needs a GPU", file=sys.stderr)
        return 2
    import np_bounds
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

    def wall(fn, calls):
        """ms per call, wall clock, of a synchronous host call."""
        fn()
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return t

    scenes = [("tiger", pm.workloads.tiger(3840, 2160)), ("tiger", pm.workloads.tiger(1920, 1080)), ("glyphs", pm.workloads.heldout_glyphs())]
    for name, wl in scenes:
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            of_item = r.item_paths()
            n_paths = int(of_item.max()) + 1
            labels = torch.from_numpy(of_item.view(np.int32)).cuda()
            boxes = torch.empty((n_items, 4), dtype=torch.float64, device="cuda")
            one = torch.empty((1, 10), dtype=torch.int32, device="cuda")
            per_path = torch.empty((n_paths, 10), dtype=torch.int32, device="cuda")
            words = torch.empty(n_items, dtype=torch.int32, device="cuda")
            stream.synchronize()
            calls = {
                "item_bounds": lambda: r.item_bounds_tensor(boxes, stream=stream),
                "union_one_label": lambda: r.union_bounds_tensor(one, stream=stream),
                "union_label_per_path": lambda: r.union_bounds_tensor(per_path, labels=labels, stream=stream),
                "select_rect_whole_view": lambda: r.select_rect_tensor(0.0, 0.0, float(wl.width), float(wl.height), words, stream=stream),
            }
            reps = {k: reps_for(fn) for k, fn in calls.items()}
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(timed(fn, reps[k]))
            stream.synchronize()
            # the answers are the host model's: what is timed is what is tested
            scene = r.download_scene()
            want = np_bounds.item_bounds(scene)
            assert boxes.cpu().numpy().tobytes() == want.tobytes()
            assert per_path.cpu().numpy().tobytes() == np_bounds.union_bounds(scene, n_paths, of_item, boxes=want).tobytes()
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = {"scene": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "paths": n_paths, "scene_bytes": int(len(scene)), "rounds": rounds, "reps": reps,
                   "touched_by_the_whole_view": int((words.cpu().numpy() & 1).sum())}
            for k in calls:
                rec[k + "_ms"] = [round(v, 5) for v in ms[k]]
                rec[k + "_median_ms"] = round(med[k], 5)
                rec[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 5)
            for k in ("item_bounds", "union_one_label", "union_label_per_path"):
                rec["ratio_" + k + "_over_select_rect"] = round(med[k] / med["select_rect_whole_view"], 3)
            # the host route and the host calls, wall clock
            d_ms = wall(r.download_scene, HOST_CALLS)
            w_ms = wall(lambda: np_bounds.item_bounds(r.download_scene()), max(HOST_CALLS // 4, 3))
            i_ms = wall(r.item_bounds, HOST_CALLS)
            s_ms = wall(r.selection_bounds, HOST_CALLS)
            for k, v in (("host_download_scene", d_ms), ("host_download_and_numpy_min_max", w_ms), ("host_call_item_bounds", i_ms), ("host_call_selection_bounds", s_ms)):
                rec[k + "_median_ms"] = round(statistics.median(v), 4)
                rec[k + "_p10_ms"] = round(float(np.percentile(v, 10)), 4)
                rec[k + "_p90_ms"] = round(float(np.percentile(v, 90)), 4)
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
