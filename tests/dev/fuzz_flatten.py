"""Randomised check of the on-device flatten + encode (GPU box): random paths (lines, quads,
cubics, several subpaths, open and closed, fills and strokes incl. thin strokes) under random
affines -- device-built scene bytes against the oracle's CPU encoder, then pixels.

    python tests/dev/fuzz_flatten.py [first_seed] [count]
"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import piet_metal_amd as pm
from oracle import pmo
from path_sets import random_pathset  # (shared with tests/test_flatten_edges.py)


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    r = pm.Renderer(0)
    bad = 0
    t0 = time.time()
    for seed in range(first, first + count):
        rng = np.random.default_rng(seed * 104729 + 7)
        ps = random_pathset(rng, int(rng.integers(1, 120)), float(rng.choice([200.0, 800.0])))
        s = float(rng.choice([0.5, 1.0, 2.7, 8.0]))
        th = rng.uniform(0, 6.28) if rng.random() < 0.5 else 0.0
        aff = (s * np.cos(th), s * np.sin(th), -s * np.sin(th), s * np.cos(th), float(rng.uniform(-50, 200)), float(rng.uniform(-50, 200)))
        w, h = int(rng.integers(64, 1600)), int(rng.integers(64, 1200))
        r.resize(w, h)
        r.flatten_and_encode(ps, aff, s)
        dev = r.download_scene()
        ref, _ = pmo.scene_from_paths(pmo.scaled_paths(ps.paths, s), ps.els, aff)
        ok = np.array_equal(dev, ref)
        if ok:
            r.render()
            ok = np.array_equal(r.read_pixels(), pmo.render(ref, w, h))
        if not ok:
            bad += 1
            print(f"MISMATCH seed {seed}: bytes equal: {np.array_equal(dev, ref)} sizes {dev.size} {ref.size}", flush=True)
    print(f"flatten fuzz: {count} path sets from seed {first}: {bad} mismatches, {time.time() - t0:.1f} s")
    return 1 if bad else 0

sys.exit(main())
