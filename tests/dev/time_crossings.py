"""Times item crossings (pm_item_crossings_device, decision D29) against the route a caller had before it (needs a GPU; not a pytest,
not bench.py).

Scenes: the Tiger flattened on the device at 3840 x 2160 and the 20 000 glyph-like paths of workloads.heldout_glyphs.  Device
calls on one caller's stream, every crossings arm exactly packed after a count pass (cap = 0) that is not timed:
  a   (Tiger) the longest item against itself, one request: one wave's work
  y   the yardstick for a: Renderer.trim of the whole item (a count pass, a packed pass, the download) and a vectorised numpy
      all-pairs with D29's rule over the vertices, rows of 256 edges at a time (host clock around both)
  b   (Tiger) every item against its paint-order neighbour, one call
  c   (glyphs) every item against itself, one call
  d   (Tiger) the longest item against the item of most edges whose chunk boxes all miss it: request a's walk of A's chunks with
      everything culled
The arms alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a second
(the yardstick: one call a window), timed with events on the stream the calls run on.  Prints one JSON line per scene: medians and
spreads (max - min over the rounds).  Arm a's answer, and 300 sampled requests of b and c, are compared with tests/np_crossings on
the downloaded scene in the same run: what is timed is what is tested.  No gate; the figures are for DESIGN.md 5.

    python tests/dev/time_crossings.py [ROUNDS]"""
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
SAMPLE = 300     # requests compared with np_crossings per arm


def numpy_all_pairs(v, move):
    """The yardstick's host half: the self-crossings of the poly-line runs `v` (float32 [n, 2]; move[k]: vertex k starts a run) by
    D29's rule, vectorised, rows of 256 edges at a time.  Returns how many."""
    keep = ~move[1:]
    E = np.concatenate([v[:-1], v[1:]], axis=1)[keep]
    n, count = len(E), 0
    cx, cy, dx, dy = (E[:, k][None, :] for k in range(4))
    c64 = [w.astype(np.float64) for w in (cx, cy, dx, dy)]
    later = np.arange(n)[None, :]
    for r0 in range(0, n, 256):
        ax, ay, bx, by = (E[r0:r0 + 256, k][:, None] for k in range(4))
        box = (np.maximum(ax, bx) >= np.minimum(cx, dx)) & (np.maximum(cx, dx) >= np.minimum(ax, bx)) & (np.maximum(ay, by) >= np.minimum(cy, dy)) & \
            (np.maximum(cy, dy) >= np.minimum(ay, by))
        share = ((ax == cx) & (ay == cy)) | ((ax == dx) & (ay == dy)) | ((bx == cx) & (by == cy)) | ((bx == dx) & (by == dy))
        ax, ay, bx, by = (w.astype(np.float64) for w in (ax, ay, bx, by))
        with np.errstate(all="ignore"):
            rx, ry = bx - ax, by - ay
            sx, sy = c64[2] - c64[0], c64[3] - c64[1]
            den = rx * sy - ry * sx
            wx, wy = c64[0] - ax, c64[1] - ay
            t = (wx * sy - wy * sx) / den
            u = (wx * ry - wy * rx) / den
            ok = box & ~share & (den != 0) & (0 <= t) & (t <= 1) & (0 <= u) & (u <= 1) & (np.arange(r0, min(r0 + 256, n))[:, None] < later)
        count += int(ok.sum())
    return count


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_crossings needs a GPU", file=sys.stderr)
        return 2
    import np_crossings as nx
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

    def host_timed(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps

    def reps_for(fn, clock):
        fn()
        stream.synchronize()
        once = clock(fn, 1)   # warmed up by the call before
        return max(1, int(np.ceil(WINDOW_S * 1e3 / max(once, 1e-3))))

    def on_device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(len(a), -1).copy()).cuda()

    def arm(r, items_a, items_b):
        """The count pass, then the packed requests and the buffers the timed call writes."""
        q = np.zeros(len(items_a), nx.CROSSINGS_QUERY)
        q["item_a"], q["item_b"] = items_a, items_b
        info = torch.zeros((len(q), 4), dtype=torch.int32, device="cuda")
        r.crossings_tensor(on_device(q), torch.zeros((1, 12), dtype=torch.int32, device="cuda"), info, stream=stream)
        stream.synchronize()
        counts = info.cpu().numpy().view(nx.CROSSINGS_INFO).reshape(-1)["n_crossings"].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        assert offsets[-1] < 1 << 32
        q["first"], q["cap"] = offsets[:-1], counts
        return {"q": q, "req": on_device(q), "offsets": offsets, "out": torch.zeros((max(int(offsets[-1]), 1), 12), dtype=torch.int32, device="cuda"), "info": info}

    def check(X, scene, ws, Ks, rng):
        got = X["out"].cpu().numpy().view(nx.CROSSING).reshape(-1)
        infos = X["info"].cpu().numpy().view(nx.CROSSINGS_INFO).reshape(-1)
        pick = rng.choice(len(X["q"]), min(SAMPLE, len(X["q"])), replace=False)
        reqs = [tuple(int(v) for v in X["q"][k]) for k in pick]
        _, want_info, answers = nx.crossings(scene, reqs, False, ws, Ks=Ks)
        for k, wi, rows in zip(pick, want_info, answers):
            assert infos[k].tobytes() == wi.tobytes(), (k, infos[k], wi)
            assert got[X["offsets"][k]:X["offsets"][k + 1]].tobytes() == nx.as_records(rows).tobytes(), k

    scenes = [("tiger", pm.workloads.tiger(3840, 2160)), ("glyphs", pm.workloads.heldout_glyphs())]
    for name, wl in scenes:
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            lengths = r.item_lengths()
            longest = int(np.argmax(lengths["n_segments"]))
            calls, arms, extra = {}, {}, {}
            if name == "tiger":
                A = arm(r, [longest], [longest])
                B = arm(r, np.arange(n_items - 1), np.arange(1, n_items))
                boxes = r.item_bounds()
                lo = boxes[longest]
                apart = (boxes[:, 2] < lo[0]) | (boxes[:, 0] > lo[2]) | (boxes[:, 3] < lo[1]) | (boxes[:, 1] > lo[3])
                far = int(np.argmax(np.where(apart, lengths["n_segments"], 0)))
                D = arm(r, [longest], [far])
                assert int(D["offsets"][-1]) == 0 and apart[far]
                yardstick = {}

                def host_route():
                    vs, offsets, infos = r.trim([longest], 0.0, np.inf)
                    yardstick["n"] = numpy_all_pairs(np.stack([vs["x"], vs["y"]], axis=1), (vs["flags"] & pm._lib.PM_TRIM_MOVE) != 0)

                calls["a_longest_item_against_itself"] = lambda: r.crossings_tensor(A["req"], A["out"], A["info"], stream=stream)
                calls["y_trim_download_numpy_all_pairs"] = host_route
                calls["b_every_item_against_its_neighbour"] = lambda: r.crossings_tensor(B["req"], B["out"], B["info"], stream=stream)
                calls["d_longest_item_all_culled"] = lambda: r.crossings_tensor(D["req"], D["out"], D["info"], stream=stream)
                arms = {"a": A, "b": B, "d": D}
                extra = {"far_item_segments": int(lengths["n_segments"][far])}
            else:
                Cc = arm(r, np.arange(n_items), np.arange(n_items))
                calls["c_every_item_against_itself"] = lambda: r.crossings_tensor(Cc["req"], Cc["out"], Cc["info"], stream=stream)
                arms = {"c": Cc}
            clocks = {k: host_timed if k.startswith("y_") else timed for k in calls}
            reps = {k: 1 if k.startswith("y_") else reps_for(fn, clocks[k]) for k, fn in calls.items()}
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(clocks[k](fn, reps[k]))
            stream.synchronize()
            # what was timed is what is tested
            scene = r.download_scene()
            ws, Ks = nm.walks(scene), nx.index_ranges(scene)
            rng = np.random.default_rng(29)
            for X in arms.values():
                check(X, scene, ws, Ks, rng)
            if name == "tiger":
                extra["yardstick_crossings"] = yardstick["n"]   # (the host route's own count, over the segments between the trimmed vertices)
            rec = {"scene": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "rounds": rounds, "reps": reps, "segments": int(lengths["n_segments"].sum()),
                   "longest_item_segments": int(lengths["n_segments"][longest]), "requests": {k: len(X["q"]) for k, X in arms.items()},
                   "crossings": {k: int(X["offsets"][-1]) for k, X in arms.items()}, **extra}
            for k in calls:
                rec[k + "_ms"] = [round(v, 5) for v in ms[k]]
                rec[k + "_median_ms"] = round(statistics.median(ms[k]), 5)
                rec[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 5)
            if name == "tiger":
                rec["a_over_yardstick"] = round(rec["a_longest_item_against_itself_median_ms"] / rec["y_trim_download_numpy_all_pairs_median_ms"], 4)
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
