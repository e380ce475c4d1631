"""Randomised walk of one context through replacements, frames and queries: the generator and the runner of tests/context_model.py
over seeds beyond the committed ones and longer scripts.  One process, one Renderer per script; stops at the first failing seed,
prints the step, and -- for a comparison that failed, not for an error of the runtime -- a minimised script: steps are dropped
greedily while the same kind of failure persists and the script stays one the model allows.  On a box without a GPU it runs on the
wave64 emulation of the kernels (where a host bug reproduces; a missing wait does not).

    python tests/dev/fuzz_context.py [first_seed] [count] [--changes N] [--seconds S] [--queries]

--queries: walk with tests/context_queries.QueryRunner -- the seven newer query families behind every state change and in flight.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import piet_metal_amd as pm  # noqa: E402
from oracle import pmo  # noqa: E402
import context_model as cm  # noqa: E402
import context_queries as cq  # noqa: E402

RUNNER = [cm.Runner]


def allowed(script):
    """The script is one the model allows: every state change meets its preconditions in the state the steps before it leave."""
    m = cm.Model(pm, pmo)
    for s in script:
        if s.kind not in cm.STATE_OPS:
            continue
        if not m.allowed(s.kind, s.variant):
            return False
        if s.kind == "reflatten_groups" and len(s.args["affines"]) <= m.max_group():
            return False
        if s.kind == "repaint" and len(s.args["opacities"]) <= m.max_group():
            return False
        if s.kind == "groups" and len(s.args["map"]) != len(m.ps.paths):
            return False
        m.apply(s)
    return True


def failure(script, seed, answers):
    """None, or the AssertionError of the script on a fresh Renderer."""
    with pm.Renderer(0) as r:
        try:
            RUNNER[0](pm, pmo, r, script, seed, answers=answers).run()
        except AssertionError as e:
            return e
    return None


def what_failed(e):
    """The kind of a failure: its text without seed, step and figures."""
    text = str(e).split(": ", 1)[-1]
    return "".join(ch for ch in text if not ch.isdigit())[:40]


def minimise(script, seed, answers, first):
    kind = what_failed(first)
    k = len(script) - 1
    while k >= 0:
        shorter = script[:k] + script[k + 1:]
        if allowed(shorter):
            e = failure(shorter, seed, answers)
            if e is not None and what_failed(e) == kind:
                script = shorter
        k -= 1
    return script


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("first", nargs="?", type=int, default=1000)
    ap.add_argument("count", nargs="?", type=int, default=50)
    ap.add_argument("--changes", type=int, default=25, help="state changes per script (the committed scripts have 11)")
    ap.add_argument("--seconds", type=float, default=0.0, help="start no script after this much wall time (0: no limit)")
    ap.add_argument("--queries", action="store_true", help="walk with QueryRunner: the newer query families too")
    args = ap.parse_args()
    if args.queries:
        answers2 = cq.Answers2()
        RUNNER[0] = lambda *a, **kw: cq.QueryRunner(*a, answers2=answers2, **kw)
    import torch

    if not torch.cuda.is_available():
        from emu_swap import swap_in_emulated_library

        os.environ["PM_TEST_EMU"] = "1"
        swap_in_emulated_library()
        print("no GPU: the emulated library")
    pmo.load()
    answers = cm.Answers()
    t0 = time.time()
    done = steps = 0
    for seed in range(args.first, args.first + args.count):
        if args.seconds and time.time() - t0 > args.seconds:
            break
        script = cm.generate(pm, pmo, seed, n_changes=args.changes, answers=answers)
        e = failure(script, seed, answers)   # (anything but a failed comparison -- a HIP error -- ends the run here, with its traceback)
        if e is not None:
            print(f"FAILED {e}", flush=True)
            small = minimise(script, seed, answers, e)
            print(f"minimised from {len(script)} to {len(small)} steps ({failure(small, seed, answers)}):")
            for s in small:
                print("   ", repr(s))
            return 1
        done += 1
        steps += len(script)
        if len(answers.cache) > 4000:
            answers.cache.clear()
        if args.queries and len(answers2.cache) > 4000:
            answers2.cache.clear()
        print(f"seed {seed}: {len(script)} steps, {time.time() - t0:.1f} s", flush=True)
    print(f"context fuzz: {done} scripts ({steps} steps, {args.changes} state changes each) from seed {args.first}: no failure, {time.time() - t0:.1f} s")
    return 0


sys.exit(main())
