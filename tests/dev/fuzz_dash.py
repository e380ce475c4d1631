"""Randomised check of dashed strokes where dash ends meet vertices, steps and limits: the grammar of tests/dash_cases.py at seeds
beyond the committed ones -- the device's scene bytes against tests/np_dash.py applied to the device's own poly-line scene, under
the identity and, re-flattened, under dash_cases.SECOND_VIEW.  Stops at the first failing seed and prints its dash table and the
event classes of its sub-paths.  On a box without a GPU it runs on the wave64 emulation of the kernels.

    python tests/dev/fuzz_dash.py [first_seed] [count]
"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import piet_metal_amd as pm
import dash_cases
import np_dash
import np_stroke


def scene_differs(r, r0, ps, affine, scale, reflatten):
    nbytes, _ = r.reflatten(affine, scale) if reflatten else r.flatten_and_encode(ps, affine, scale)
    got = r.download_scene()
    r0.flatten_and_encode(pm.PathSet(np_stroke.unstyled(ps.paths), ps.els), affine, scale)
    want = np.frombuffer(np_dash.apply(r0.download_scene(), np_dash.specs_from_pathset(ps, scale)), np.uint8)
    if nbytes == len(want) == len(got) and np.array_equal(got, want):
        return None
    n = min(len(got), len(want))
    bad = np.flatnonzero(got[:n] != want[:n])
    return f"{len(got)} bytes, np_dash {len(want)}; {bad.size} differ, the first at {bad[:4].tolist()}"


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else len(dash_cases.SEEDS)
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    import torch

    if not torch.cuda.is_available():
        from emu_swap import swap_in_emulated_library

        swap_in_emulated_library()
        print("no GPU: the emulated library")
    t0 = time.time()
    with pm.Renderer(0) as r, pm.Renderer(0) as r0:
        for seed in range(first, first + count):
            ps, ws = dash_cases.dash_case(seed)
            for view, (affine, scale) in enumerate([(dash_cases.IDENTITY, ws), dash_cases.SECOND_VIEW]):
                what = scene_differs(r, r0, ps, affine, scale, reflatten=view == 1)
                if what is None:
                    continue
                print(f"MISMATCH seed {seed}, view {view} (affine {affine}, width_scale {scale}): {what}")
                for d in ps.dashes:
                    v = ps.dash_values[int(d["first"]) : int(d["first"]) + int(d["count"])]
                    print(f"  path {int(d['path'])}: offset {float(d['offset'])!r} pattern {v.tolist()}")
                for k, (sub, classes) in enumerate(zip(dash_cases.subpaths_of(ps), dash_cases.classes_of((ps, ws)))):
                    print(f"  sub-path {k} (path {sub[0]}, {len(sub[1])} points, {'closed' if sub[2] else 'open'}), under the identity: {sorted(classes)}")
                return 1
    print(f"dash fuzz: {count} path sets from seed {first}: no mismatch, {time.time() - t0:.1f} s")
    return 0


sys.exit(main())
