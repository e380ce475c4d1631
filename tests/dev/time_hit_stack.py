"""Times the hit stacks against pm_hit_test (needs a GPU; not a pytest, not bench.py).

Scene: the Tiger flattened on the device at 1920 x 1080, queries: every pixel centre, made on the device.  DESIGN.md 4's method for
pm_hit_kernel: the device variant on a caller's stream, warm, each call between two HIP events, the median of 21 calls.  The arms
alternate call by call in this one process, so that they share whatever the clock does:
  A0  pm_hit_test_device, top item only            S1   pm_hit_stack_device, k = 1, no counts
  A1  pm_hit_test_device with counts               S4   pm_hit_stack_device, k = 4, with counts     S16  the same at k = 16
Before any timing S1's items are compared word for word with A0's top_item, and S4's counts with A1's.

Prints one JSON line per arm (median, minimum and maximum in ms, queries per second at the median) and the differences S1 - A0,
S4 - A1 and S16 - A1 beside the arms' own spreads.

    python tests/dev/time_hit_stack.py [CALLS]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(calls=21):
    import torch

    if not torch.cuda.is_available():
        print("time_hit_stack needs a GPU", file=sys.stderr)
        return 2
    import piet_metal_amd as pm

    W, H = 1920, 1080
    stream = torch.cuda.Stream()
    wl = pm.workloads.tiger(W, H)
    with pm.Renderer(0) as r, torch.cuda.stream(stream):
        _, n_items = r.flatten_and_encode(wl.paths, wl.affine, wl.width_scale)
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
        xy = torch.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], dim=1).contiguous()
        n = W * H
        top = torch.empty(n, dtype=torch.int32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        items = {k: torch.empty((n, k), dtype=torch.int32, device="cuda") for k in (1, 4, 16)}
        scnt = torch.empty(n, dtype=torch.int32, device="cuda")
        arms = {
            "A0 hit_test top only": lambda: r.hit_test_tensor(xy, top, None, stream=stream),
            "S1 hit_stack k=1 no counts": lambda: r.hit_stack_tensor(xy, items[1], None, stream=stream),
            "A1 hit_test with counts": lambda: r.hit_test_tensor(xy, top, cnt, stream=stream),
            "S4 hit_stack k=4 with counts": lambda: r.hit_stack_tensor(xy, items[4], scnt, stream=stream),
            "S16 hit_stack k=16 with counts": lambda: r.hit_stack_tensor(xy, items[16], scnt, stream=stream),
        }
        for fn in arms.values():   # warm
            fn()
        stream.synchronize()
        assert torch.equal(items[1].view(-1), top), "S1's items are not A0's top_item"
        assert torch.equal(items[4][:, 0], top) and torch.equal(items[16][:, :4], items[4]) and torch.equal(scnt, cnt), "S4 / S16 differ from A1"
        depth = int(cnt.max())
        ms = {name: [] for name in arms}
        for _ in range(calls):
            for name, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, v in ms.items():
        print(json.dumps({"arm": name, "view": f"{W}x{H}", "items": n_items, "queries": n, "deepest_stack": depth, "calls": calls, "median_ms": round(med[name], 4),
                          "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "queries_per_s": round(n / med[name] * 1e3)}), flush=True)
    names = list(arms)
    for s, a in ((1, 0), (3, 2), (4, 2)):
        d = med[names[s]] - med[names[a]]
        print(json.dumps({"difference": f"{names[s].split()[0]} - {names[a].split()[0]}", "ms": round(d, 4), "relative": round(d / med[names[a]], 4),
                          "spread_of_the_two_ms": [round(max(ms[names[k]]) - min(ms[names[k]]), 4) for k in (s, a)]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 21))
