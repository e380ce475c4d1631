"""Times resampling (pm_resample_items_device, decision D26) against the call it replaces, pm_points_at_length_device on the same
positions (needs a GPU; not a pytest, not bench.py).

Scenes: the Tiger flattened on the device at 3840 x 2160 and the 20 000 glyph-like paths of workloads.heldout_glyphs.  Device
calls, all on one caller's stream:
  a   100 requests of 1 000 step-mode samples each, all on the scene's longest item (request k starts k units in, the step is
      T div 1 000: every sample is inside the item)
  b   pm_points_at_length_device on exactly those 100 000 (item, s_j) -- the yardstick: existing, unchanged code, in the same run
  c   one even request of 64 samples per item, for every item
  d   pm_points_at_length_device on c's positions
  e   a single request of 2^20 samples on the longest item: the stated limit of a wave per request
The five alternate ROUNDS times in this one process, each window a batch of calls long enough to last a good fraction of a second,
timed with events on the stream the calls run on.  Prints one JSON line per scene: medians and spreads (max - min over the
rounds).  400 sampled answers per arm are compared with tests/np_resample (positions) and tests/np_measure (points) on the
downloaded scene in the same run, and a's and c's records with b's and d's byte for byte: what is timed is what is tested.

On the Tiger arm a must beat arm b by more than the two arms' spreads (exit status 1 if it does not): otherwise the dealing of the
samples over the lanes is wrong.  The other arms are recorded without a gate; the figures are for DESIGN.md 5.

    python tests/dev/time_resample.py [ROUNDS]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_S = 0.3   # what a timed window should last at least
SAMPLE = 400     # answers compared with np_measure per arm


def main(rounds=5):
    import torch

    if not torch.cuda.is_available():
        print("time_resample needs a GPU", file=sys.stderr)
        return 2
    import np_measure as nm
    import np_resample as nr
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

    def on_device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(len(a), -1).copy()).cuda()

    def arm(requests, lengths):
        """Packed requests (item, mode, count, start, step): their records on the device, the (item, s_j) of every sample as length
        queries on the device, and the buffers both calls write."""
        packed, total = nr.packed(requests)
        pairs = []
        for item, mode, count, first, start, step in packed:
            pairs += [(item, s) for s in nr.positions(mode, count, start, step, int(lengths[item]["length"]), int(lengths[item]["kind"]))]
        q = np.zeros(total, nm.LENGTH_QUERY)
        q["item"], q["s"] = [p[0] for p in pairs], np.array([p[1] for p in pairs], np.uint64)
        return {"packed": packed, "pairs": pairs, "req": on_device(nr.records(packed)), "q": on_device(q),
                "out": torch.zeros((total, 8), dtype=torch.int32, device="cuda"), "ref": torch.zeros((total, 8), dtype=torch.int32, device="cuda"),
                "info": torch.zeros((len(packed), 4), dtype=torch.int32, device="cuda")}

    status = 0
    scenes = [("tiger", pm.workloads.tiger(3840, 2160)), ("glyphs", pm.workloads.heldout_glyphs())]
    for name, wl in scenes:
        with pm.Renderer(0) as r, torch.cuda.stream(stream):
            _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
            lengths = r.item_lengths()
            longest = int(np.argmax(lengths["length"]))
            T = int(lengths["length"][longest])
            A = arm([(longest, nr.STEP, 1000, k, T // 1000) for k in range(100)], lengths)
            Cc = arm([(i, nr.EVEN, 64, 0, 0) for i in range(n_items)], lengths)
            big = nr.records(nr.packed([(longest, nr.STEP, nr.MAX_COUNT, 0, max(T // nr.MAX_COUNT, 1))])[0])
            E = {"req": on_device(big), "out": torch.zeros((nr.MAX_COUNT, 8), dtype=torch.int32, device="cuda"), "info": torch.zeros((1, 4), dtype=torch.int32, device="cuda")}
            calls = {
                "a_resample_100x1000_longest": lambda: r.resample_tensor(A["req"], A["out"], A["info"], stream=stream),
                "b_points_at_the_same_100000": lambda: r.points_at_length_tensor(A["q"], A["ref"], stream=stream),
                "c_resample_64_even_per_item": lambda: r.resample_tensor(Cc["req"], Cc["out"], Cc["info"], stream=stream),
                "d_points_at_the_same": lambda: r.points_at_length_tensor(Cc["q"], Cc["ref"], stream=stream),
                "e_resample_one_request_2p20": lambda: r.resample_tensor(E["req"], E["out"], E["info"], stream=stream),
            }
            reps = {k: reps_for(fn) for k, fn in calls.items()}
            ms = {k: [] for k in calls}
            for _ in range(rounds):
                for k, fn in calls.items():
                    ms[k].append(timed(fn, reps[k]))
            stream.synchronize()
            # what was timed is what is tested
            scene = r.download_scene()
            ws = nm.walks(scene)
            rng = np.random.default_rng(26)
            for X in (A, Cc):
                got, ref = X["out"].cpu().numpy(), X["ref"].cpu().numpy()
                assert got.tobytes() == ref.tobytes(), "resampling differs from pm_points_at_length on its own positions"
                pick = rng.choice(len(X["pairs"]), SAMPLE, replace=False)
                want = nm.points_at_length(scene, [X["pairs"][k] for k in pick], ws=ws)
                assert got.view(nm.LENGTH_POINT).reshape(-1)[pick].tobytes() == want.tobytes()
                _, want_info = nr.resample(scene, [(q[0], q[1], 0, 0, q[4], q[5]) for q in X["packed"]], False, ws)
                info = X["info"].cpu().numpy().view(nr.RESAMPLE_INFO).reshape(-1)
                assert info["length"].tobytes() == want_info["length"].tobytes() and info["kind"].tobytes() == want_info["kind"].tobytes()
            pick = rng.choice(nr.MAX_COUNT, SAMPLE, replace=False)
            step = int(big["step"][0])
            want = nm.points_at_length(scene, [(longest, int(j) * step) for j in pick], ws=ws)
            assert E["out"].cpu().numpy().view(nm.LENGTH_POINT).reshape(-1)[pick].tobytes() == want.tobytes()
            e_info = E["info"].cpu().numpy().view(nr.RESAMPLE_INFO).reshape(-1)[0]
            assert int(e_info["length"]) == T and int(e_info["n_unclamped"]) == min(nr.MAX_COUNT, T // step + 1)
            rec = {"scene": name, "view": f"{wl.width}x{wl.height}", "items": n_items, "rounds": rounds, "reps": reps, "segments": int(lengths["n_segments"].sum()),
                   "longest_item_segments": int(lengths["n_segments"][longest]), "samples": {"a": len(A["pairs"]), "c": len(Cc["pairs"]), "e": nr.MAX_COUNT}}
            for k in calls:
                rec[k + "_ms"] = [round(v, 5) for v in ms[k]]
                rec[k + "_median_ms"] = round(statistics.median(ms[k]), 5)
                rec[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 5)
            a, b = "a_resample_100x1000_longest", "b_points_at_the_same_100000"
            rec["a_beats_b"] = bool(rec[b + "_median_ms"] - rec[a + "_median_ms"] > rec[a + "_spread_ms"] + rec[b + "_spread_ms"])
            if name == "tiger" and not rec["a_beats_b"]:
                status = 1
            print(json.dumps(rec), flush=True)
    return status


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 5))
