"""Times trimming (pm_trim_items_device, decision D27) against the calls a caller would otherwise make (needs a GPU; not a pytest,
not bench.py).

Scenes: the Tiger flattened on the device at 3840 x 2160 and the 20 000 glyph-like paths of workloads.heldout_glyphs.  Device
calls, all on one caller's stream, every trim arm exactly packed after a count pass (cap = 0) that is not timed:
  a   (Tiger) 100 000 range requests spread over all items: request k on item k mod n, a quarter of the item from a start that moves
      with k
  b   pm_points_at_length_device on the same 100 000 (item, lo) pairs -- the yardstick: existing, unchanged code, in the same run
  c   (Tiger) the same 100 000 requests, all on the longest item
  d   pm_points_at_length_device on c's (item, lo) pairs
  e   (glyphs) every item in 64 even parts (trim_parts' requests)
  f   pm_resample_items_device, 64 even samples per item, there
  g   one whole-item request on the scene's longest item
  h   download_scene(), what a host walk would need first (host clock around the synchronising call)
Trim walks the whole item for T where pm_points_at_length leaves the walk at the owner: it is expected to cost more on long items.
The arms alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a second,
timed with events on the stream the calls run on.  Prints one JSON line per scene: medians and spreads (max - min over the
rounds).  400 sampled pieces per arm are compared with tests/np_trim on the downloaded scene in the same run: what is timed is what
is tested.  No gate; the figures are for DESIGN.md 5.

    python tests/dev/time_trim.py [ROUNDS]"""
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
SAMPLE = 400     # pieces compared with np_trim per arm
N_RANGE = 100000


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_trim needs a GPU", file=sys.stderr)
        return 2
    import np_measure as nm
    import np_resample as nr
    import np_trim as nt
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

    def arm(r, q):
        """TRIM_QUERY records without places: the count pass, then the packed requests and the buffers the timed call writes."""
        q = q.copy()
        q["first"], q["cap"] = 0, 0
        info = torch.zeros((len(q), 6), dtype=torch.int32, device="cuda")
        r.trim_tensor(on_device(q), torch.zeros((1, 4), dtype=torch.int32, device="cuda"), info, stream=stream)
        stream.synchronize()
        counts = info.cpu().numpy().view(nt.TRIM_INFO).reshape(-1)["n_vertices"].astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        assert offsets[-1] < 1 << 32
        q["first"], q["cap"] = offsets[:-1], counts
        return {"q": q, "req": on_device(q), "offsets": offsets, "out": torch.zeros((max(int(offsets[-1]), 1), 4), dtype=torch.int32, device="cuda"), "info": info}

    def length_queries(q):
        lq = np.zeros(len(q), nm.LENGTH_QUERY)
        lq["item"], lq["s"] = q["item"], q["s0"]
        return {"q": on_device(lq), "out": torch.zeros((len(q), 8), dtype=torch.int32, device="cuda")}

    def check(X, scene, ws, rng):
        got = X["out"].cpu().numpy().view(nt.TRIM_VERTEX).reshape(-1)
        infos = X["info"].cpu().numpy().view(nt.TRIM_INFO).reshape(-1)
        pick = rng.choice(len(X["q"]), min(SAMPLE, len(X["q"])), replace=False)
        reqs = [tuple(int(v) for v in X["q"][k]) for k in pick]
        _, want_info, pieces = nt.trim(scene, reqs, False, ws)
        for k, wi, vs in zip(pick, want_info, pieces):
            assert infos[k].tobytes() == wi.tobytes(), (k, infos[k], wi)
            assert got[X["offsets"][k]:X["offsets"][k + 1]].tobytes() == nt.as_records(vs).tobytes(), k

    def range_requests(items, lengths):
        q = np.zeros(N_RANGE, nt.TRIM_QUERY)
        k = np.arange(N_RANGE, dtype=np.uint64)
        T = lengths["length"][items].astype(np.uint64)
        q["item"], q["mode"] = items, nt.RANGE
        q["s0"] = T // np.uint64(2000) * ((k * np.uint64(7919)) % np.uint64(1000))     # a start in the item's first half
        q["s1"] = q["s0"] + T // np.uint64(4)
        return q

    scenes = [("tiger", pm.workloads.tiger(3840, 2160)), ("glyphs", pm.workloads.heldout_glyphs())]
    for name, wl in scenes:
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            lengths = r.item_lengths()
            longest = int(np.argmax(lengths["length"]))
            calls, clocks, arms = {}, {}, {}
            if name == "tiger":
                A = arm(r, range_requests(np.arange(N_RANGE) % n_items, lengths))
                Cc = arm(r, range_requests(np.full(N_RANGE, longest), lengths))
                B, D = length_queries(A["q"]), length_queries(Cc["q"])
                calls["a_trim_100000_spread"] = lambda: r.trim_tensor(A["req"], A["out"], A["info"], stream=stream)
                calls["b_points_at_the_same_los"] = lambda: r.points_at_length_tensor(B["q"], B["out"], stream=stream)
                calls["c_trim_100000_longest"] = lambda: r.trim_tensor(Cc["req"], Cc["out"], Cc["info"], stream=stream)
                calls["d_points_at_the_same_los"] = lambda: r.points_at_length_tensor(D["q"], D["out"], stream=stream)
                arms = {"a": A, "c": Cc}
            else:
                q = np.zeros(n_items * 64, nt.TRIM_QUERY)
                q["item"], q["mode"] = np.repeat(np.arange(n_items), 64), nt.PART
                q["s0"], q["s1"] = np.tile(np.arange(64), n_items), 64
                E = arm(r, q)
                packed, total = nr.packed([(i, nr.EVEN, 64, 0, 0) for i in range(n_items)])
                F = {"req": on_device(nr.records(packed)), "out": torch.zeros((total, 8), dtype=torch.int32, device="cuda"),
                     "info": torch.zeros((n_items, 4), dtype=torch.int32, device="cuda")}
                calls["e_trim_64_parts_per_item"] = lambda: r.trim_tensor(E["req"], E["out"], E["info"], stream=stream)
                calls["f_resample_64_even_per_item"] = lambda: r.resample_tensor(F["req"], F["out"], F["info"], stream=stream)
                arms = {"e": E}
            one = np.zeros(1, nt.TRIM_QUERY)
            one["item"], one["s1"] = longest, (1 << 64) - 1
            G = arm(r, one)
            calls["g_trim_whole_longest_item"] = lambda: r.trim_tensor(G["req"], G["out"], G["info"], stream=stream)
            calls["h_download_scene"] = r.download_scene
            arms["g"] = G
            clocks = {k: host_timed if k.startswith("h_") else timed for k in calls}
            reps = {k: reps_for(fn, clocks[k]) for k, fn in calls.items()}
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(clocks[k](fn, reps[k]))
            stream.synchronize()
            # what was timed is what is tested
            scene = r.download_scene()
            ws = nm.walks(scene)
            rng = np.random.default_rng(27)
            for X in arms.values():
                check(X, scene, ws, rng)
            rec = {"scene": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "rounds": rounds, "reps": reps, "segments": int(lengths["n_segments"].sum()),
                   "longest_item_segments": int(lengths["n_segments"][longest]), "requests": {k: len(X["q"]) for k, X in arms.items()},
                   "vertices": {k: int(X["offsets"][-1]) for k, X in arms.items()}}
            for k in calls:
                rec[k + "_ms"] = [round(v, 5) for v in ms[k]]
                rec[k + "_median_ms"] = round(statistics.median(ms[k]), 5)
                rec[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 5)
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
