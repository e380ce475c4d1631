"""Times coverage counts against the walk they share and against the path a caller had before (needs a GPU; not a pytest, not bench.py).

Scenes: the Tiger flattened on the device at 3840 x 2160 and at 1920 x 1080, config 4 (10 000 blobs, 4096 x 4096), and config 4 with
every blob's alpha set to 255 (deep opaque content: what PM_COVERAGE_VISIBLE_ONLY is for); the whole view.
  C   pm_item_coverage_device
  V   the same with PM_COVERAGE_VISIBLE_ONLY
  F   pm_hit_frame_device with counts: the same walk, a word (two) per pixel instead of the reduction
  P   what a caller did before for the topmost counts alone: hit_frame_tensor, a copy to the host, numpy.bincount (host clock around
      it: it ends in a synchronising copy)
Before any timing C's top column is compared with the histogram of F's map, the sum of C's covered column with the sum of F's counts,
and V with C.  Then, warm, each call is timed by itself between two events on the stream it runs on, C, V, F and P in turn, SAMPLES
times; median and spread (max - min) of each are reported.

Prints one JSON line per scene.

    python tests/dev/time_coverage.py [SAMPLES]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(samples=21):
    import torch

    if not torch.cuda.is_available():
        print("time_coverage needs a GPU", file=sys.stderr)
        return 2
    import piet_metal_amd as pm

    stream = torch.cuda.Stream()

    def timed(fn):
        """ms of one call, device time between two events on the stream."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def summary(ms):
        return {"median_ms": round(statistics.median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}

    blobs = pm.workloads.config4_blobs()
    solid = pm.workloads.config4_blobs()        # the same blobs, every one opaque (config 4's alphas are 0x40 .. 0xff: one in 192 is)
    solid.paths.paths["fill_rgba"] |= 0xFF
    scenes = [("tiger", pm.workloads.tiger(3840, 2160)), ("tiger", pm.workloads.tiger(1920, 1080)), ("config4", blobs), ("config4_opaque", solid)]
    for name, wl in scenes:
        W, H = wl.width, wl.height
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            cov = torch.empty((n_items, 4), dtype=torch.int32, device="cuda")
            vis = torch.empty((n_items, 4), dtype=torch.int32, device="cuda")
            top = torch.empty((H, W), dtype=torch.int32, device="cuda")
            cnt = torch.empty((H, W), dtype=torch.int32, device="cuda")
            fc = lambda: r.item_coverage_tensor(cov, w=W, h=H, stream=stream)                       # noqa: E731
            fv = lambda: r.item_coverage_tensor(vis, w=W, h=H, stream=stream, visible_only=True)    # noqa: E731
            ff = lambda: r.hit_frame_tensor(top, cnt, stream=stream)                                # noqa: E731

            def fp():
                r.hit_frame_tensor(top, None, stream=stream)
                m = top.cpu().numpy().view(np.uint32).ravel()
                return np.bincount(m[m != 0xFFFFFFFF], minlength=n_items)

            # the same answers, before any timing
            fc(), fv(), ff()
            stream.synchronize()
            c, v = cov.cpu().numpy().view(np.uint32), vis.cpu().numpy().view(np.uint32)
            assert np.array_equal(c[:, 2], fp()), "top is not the histogram of the item map"
            assert int(c[:, 0].astype(np.uint64).sum()) == int(cnt.sum(dtype=torch.int64)), "covered does not sum to n_hit"
            assert np.array_equal(v[:, 1:], c[:, 1:]) and np.array_equal(v[:, 0], c[:, 1]), "visible_only differs"
            for f in (fc, fv, ff, fp):   # warm
                f()
            stream.synchronize()
            c_ms, v_ms, f_ms, p_ms = [], [], [], []
            for _ in range(samples):
                c_ms.append(timed(fc))
                v_ms.append(timed(fv))
                f_ms.append(timed(ff))
                t0 = time.perf_counter()
                fp()
                p_ms.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median
            print(json.dumps({
                "scene": name, "view": f"{W}x{H}", "items": n_items, "samples": samples,
                "hidden_items": int(((c[:, 0] > 0) & (c[:, 1] == 0)).sum()), "covered_items": int((c[:, 0] > 0).sum()),
                "coverage": summary(c_ms), "visible_only": summary(v_ms), "hit_frame_counts": summary(f_ms), "map_copy_bincount": summary(p_ms),
                "coverage_over_hit_frame": round(med(c_ms) / med(f_ms), 3), "visible_only_over_coverage": round(med(v_ms) / med(c_ms), 3),
                "map_copy_bincount_over_coverage": round(med(p_ms) / med(c_ms), 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 21))
