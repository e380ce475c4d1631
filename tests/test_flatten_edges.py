"""The on-device flatten + encode (piet_metal_amd/csrc/pm_flatten.hip) at its edges: the random path grammar of the flatten
fuzzer and a table of named edge cases (tests/path_sets.py), each against the oracle -- scene bytes after pm_flatten_and_encode
and after pm_reflatten under a second affine, pixels at a small viewport --, once more through the block-parallel prefix sums
(PM_SCAN_SPLIT=0); the host encoder (pm_encoder_fill_path / pm_encoder_stroke_path) on the same cases; the device's points against
an exact rational reference that does not share the kernels' order of operations; and curves whose subdivision counts cannot be
stored (2^30 points for one curve, 2^32 for a path), which must come back as PM_ERR_CAPACITY at once, leave the context usable,
and agree with the host encoder and the oracle.  test_emu_cpu.py runs the gpu-marked tests here under wave64 emulation too."""
import ctypes as C
import time
from fractions import Fraction

import numpy as np
import pytest

from np_scene import p6, subdivision_count, subdivision_count_exact
from path_sets import (COMPOUND, EVEN_ODD, FILL, IDENTITY, MAX_HYPOT2, STROKE, C as CURVE, M, count_boundary_curves, edge_cases, huge_curve_case,
                       p6_rounds_up_above_406, pathset, random_case)

EDGES = edge_cases()


def _oracle_status(pmo, case, affine, cap=1 << 24):
    n_items = C.c_uint32(0)
    buf = np.zeros(cap, np.uint8)
    paths = pmo.scaled_paths(case.ps.paths, case.scale)
    aff = (C.c_double * 6)(*affine)
    return pmo.load().pmo_scene_from_paths(buf.ctypes.data, buf.size, paths.ctypes.data, len(paths), case.ps.els.ctypes.data,
                                           len(case.ps.els), aff, C.byref(n_items))


def _device_matches_oracle(pm, pmo, renderer, case):
    renderer.resize(case.width, case.height)
    if case.status != pm._lib.PM_OK:
        with pytest.raises(pm.PietMetalError) as ei:
            renderer.flatten_and_encode(case.ps, case.affine, case.scale)
        assert ei.value.status == case.status
        assert _oracle_status(pmo, case, case.affine) < 0
        return
    paths = pmo.scaled_paths(case.ps.paths, case.scale)
    for step, aff in enumerate((case.affine, case.affine2)):
        if step == 0:
            nbytes, n_items = renderer.flatten_and_encode(case.ps, aff, case.scale)
        else:
            nbytes, n_items = renderer.reflatten(aff, case.scale)
        want, want_items = pmo.scene_from_paths(paths, case.ps.els, aff)
        got = renderer.download_scene()
        assert (n_items, nbytes) == (want_items, want.size), step
        assert np.array_equal(got, want), f"scene bytes differ from the oracle's (step {step})"
        renderer.render()
        img = renderer.read_pixels()
        assert np.array_equal(img, pmo.render(want, case.width, case.height)), f"pixels differ from the oracle's (step {step})"


@pytest.mark.gpu
@pytest.mark.parametrize("split", [None, 0], ids=["scan_one_workgroup", "scan_split0"])
@pytest.mark.parametrize("seed", range(30))
def test_flatten_edges_random_grammar(pm, pmo, renderer, monkeypatch, seed, split):
    if split is not None:
        monkeypatch.setenv("PM_SCAN_SPLIT", str(split))
    _device_matches_oracle(pm, pmo, renderer, random_case(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("split", [None, 0], ids=["scan_one_workgroup", "scan_split0"])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_flatten_edges_table(pm, pmo, renderer, monkeypatch, name, split):
    if split is not None:
        monkeypatch.setenv("PM_SCAN_SPLIT", str(split))
    _device_matches_oracle(pm, pmo, renderer, EDGES[name])


def _host_encode(pm, ps, cap):
    """Every path through pm_encoder_fill_path / pm_encoder_stroke_path (host flatten, identity transform); returns (status,
    scene).  The group's item count is counted from the MoveTos, as make_tiger's count pass does."""
    buf = np.zeros(cap, np.uint8)
    e = pm.Encoder(buf)
    n_items = 0
    for p in ps.paths:
        # (items per path: sub-paths = MoveTo elements; a compound fill is one item)
        n_sub = int((ps.els["tag"][int(p["el_begin"]) : int(p["el_end"])] == M).sum())
        fl = int(p["flags"])
        n_items += ((min(n_sub, 1) if fl & COMPOUND else n_sub) if fl & FILL else 0) + (n_sub if fl & STROKE else 0)
    e.begin_group(n_items)
    try:
        for p in ps.paths:
            els = ps.els[int(p["el_begin"]) : int(p["el_end"])]
            fl = int(p["flags"])
            if fl & FILL:
                e.fill_path(els, int(p["fill_rgba"]), even_odd=bool(fl & EVEN_ODD), compound=bool(fl & COMPOUND))
            if fl & STROKE:
                e.stroke_path(els, int(p["stroke_rgba"]), float(p["stroke_width"]))
        e.end_group()
    except pm.PietMetalError as err:
        return err.status, None
    return pm._lib.PM_OK, buf[: e.bytes_used].copy()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_flatten_edges_host_encoder(pm, pmo, name):
    """The host encoder (identity transform) on the same paths: the oracle's bytes, or the device's error status."""
    case = EDGES[name]
    status, got = _host_encode(pm, case.ps, 1 << 20)
    assert status == case.status
    if status == pm._lib.PM_OK:
        want, _ = pmo.scene_from_paths(pmo.scaled_paths(case.ps.paths, 1.0), case.ps.els, IDENTITY)
        assert np.array_equal(got, want)


def test_subdivision_count_rule(pmo):
    """One count rule everywhere: the smallest n with p6(n) = ((n*n)*(n*n))*(n*n) in binary64 >= x (oracle/pmo.h).  The oracle's
    count equals np_scene's on both sides of k^6 for k = 1, 2, 7, 64, 405 and at p6(k) for a k above 406 where p6 rounds up; the
    exact-integer rule agrees wherever p6 is exact, and at x = p6(k) it says k + 1 where the product says k."""
    lib = pmo.load()
    lib.pmo_subdivision_count.restype = C.c_size_t
    lib.pmo_subdivision_count.argtypes = [C.c_double]
    xs = [x for _, x in count_boundary_curves()]
    xs += [float(k ** 6) for k in range(1, 407)] + [np.nextafter(float(k ** 6), np.inf) for k in range(1, 407)]
    xs += [0.0, -1.0, 0.5, float("nan"), 1e54, np.nextafter(1e54, np.inf), 1e300, float("inf")]
    k_up = p6_rounds_up_above_406()
    for x in xs:
        n = subdivision_count(x)
        assert lib.pmo_subdivision_count(x) == n, x
        if x == x and x <= float(406 ** 6) + 1e4:
            assert subdivision_count_exact(x) == n, x
    assert subdivision_count(p6(k_up)) == k_up and subdivision_count_exact(p6(k_up)) == k_up + 1
    assert subdivision_count(float("inf")) == 1 << 30 and subdivision_count(float("nan")) == 1


# ---- an exact reference that does not share the kernels' order of operations ----------------------------------------------------

def _exact_affine(aff, x, y):
    a, b, c, d, e, f = (Fraction(v) for v in aff)
    return a * Fraction(x) + c * Fraction(y) + e, b * Fraction(x) + d * Fraction(y) + f


def _kernel_x(aff, p0, el):
    """The count's argument in binary64 as KCount computes it (Python floats are binary64 and unfused)."""
    a, b, c, d, e, f = aff
    xf = lambda x, y: (a * x + c * y + e, b * x + d * y + f)
    (lx, ly), (p1x, p1y), (p2x, p2y), (p3x, p3y) = xf(*p0), xf(el[1], el[2]), xf(el[3], el[4]), xf(el[5], el[6])
    ax, ay = p1x * 3.0 - lx, p1y * 3.0 - ly
    bx, by = p2x * 3.0 - p3x, p2y * 3.0 - p3y
    dx, dy = bx - ax, by - ay
    return (dx * dx + dy * dy) / MAX_HYPOT2


def _curve_only_pathset(rng):
    paths = []
    for _ in range(6):
        subs = []
        for _ in range(int(rng.integers(1, 4))):
            p = rng.uniform(10, 110, 2)
            sub = [(M, p[0], p[1])]
            for _ in range(int(rng.integers(1, 4))):
                q = [p + rng.uniform(-40, 40, 2) for _ in range(3)]
                sub.append((CURVE, q[0][0], q[0][1], q[1][0], q[1][1], q[2][0], q[2][1]))
                p = q[2]
            subs += sub
        paths.append((subs, FILL))
    return pathset(*paths)


@pytest.mark.gpu
@pytest.mark.parametrize("aff", [(0.8, 0.6, -0.6, 0.8, 40.0, -10.0), (-1.3, 0.0, 0.25, 1.1, 170.0, 3.0), (1.0, 0.45, -0.7, 0.95, 60.0, 20.0)],
                         ids=["rotated", "mirrored_sheared", "sheared"])
def test_flatten_edges_points_against_exact_rationals(pm, renderer, aff):
    """Curve-only sub-paths, fills: every device point (f32) lies within half an f32 ulp of the exact value -- the affine and the
    cubic at t = (k+1)/n in rationals -- plus c 2^-52 (|p0| + 3|p1| + 3|p2| + |p3|) for the binary64 evaluation; every item holds
    1 + n points with n the integer count rule of the kernel's x; every ShortBbox is floor / ceil of the exact box, saturated.
    This catches a wrong parameter, control-point order or last point even where the oracle made the same mistake."""
    ps = _curve_only_pathset(np.random.default_rng(11))
    renderer.resize(128, 128)
    n_bytes, n_items = renderer.flatten_and_encode(ps, aff, 1.0)
    scene = renderer.download_scene()
    assert scene.size == n_bytes
    words = scene.view(np.uint32)
    assert words[0] == n_items
    item = 0
    for p in ps.paths:
        subs = []
        for el in ps.els[int(p["el_begin"]) : int(p["el_end"])]:
            el = (int(el["tag"]),) + tuple(float(v) for v in el["p"])
            if el[0] == M:
                subs.append([el])
            else:
                subs[-1].append(el)
        for sub in subs:
            want, mags = _exact_points(aff, sub)
            _check_item(scene, words, int(words[1]), item, want, mags)
            item += 1
    assert item == n_items
    # the curves on the n^6 boundaries, under the identity (what their builder searched)
    sub_ps = pathset(*[([(M, 0.0, 0.0), el], FILL) for el, _ in count_boundary_curves()])
    renderer.flatten_and_encode(sub_ps, IDENTITY, 1.0)
    scene = renderer.download_scene()
    words = scene.view(np.uint32)
    for item, (el, x) in enumerate(count_boundary_curves()):
        want, mags = _exact_points(IDENTITY, [(M, 0.0, 0.0), el])
        assert len(want) == 1 + subdivision_count(x)
        _check_item(scene, words, int(words[1]), item, want, mags)


def _exact_points(aff, sub):
    """Exact points of one sub-path (MoveTo + curves) and, per point, the magnitude sum the binary64 error bound scales with."""
    x0 = (sub[0][1], sub[0][2])
    cur = _exact_affine(aff, *x0)
    cur_mag = _mag(aff, *x0)
    pts, mags = [cur], [cur_mag]
    prev = x0
    for el in sub[1:]:
        n = subdivision_count(_kernel_x(aff, prev, el))
        P = [cur] + [_exact_affine(aff, el[1 + 2 * j], el[2 + 2 * j]) for j in range(3)]
        Mg = [cur_mag] + [_mag(aff, el[1 + 2 * j], el[2 + 2 * j]) for j in range(3)]
        bound = tuple(Mg[0][i] + 3 * Mg[1][i] + 3 * Mg[2][i] + Mg[3][i] for i in range(2))
        for k in range(n):
            t = Fraction(k + 1, n)
            mt = 1 - t
            pts.append(tuple(mt ** 3 * P[0][i] + 3 * mt * mt * t * P[1][i] + 3 * mt * t * t * P[2][i] + t ** 3 * P[3][i] for i in range(2)))
            mags.append(bound)
        cur, cur_mag, prev = P[3], Mg[3], (el[5], el[6])
    return pts, mags


def _mag(aff, x, y):
    a, b, c, d, e, f = aff
    return (abs(a * x) + abs(c * y) + abs(e), abs(b * x) + abs(d * y) + abs(f))


def _check_item(scene, words, items_ix, item, want, mags, c=16):
    it = words[(items_ix + 32 * item) // 4 : (items_ix + 32 * item) // 4 + 5]
    assert it[0] == 3 and it[3] == len(want), (item, it[3], len(want))
    got = scene[int(it[4]) : int(it[4]) + 8 * len(want)].view(np.float32).reshape(-1, 2)
    lo, hi = [None, None], [None, None]
    for (gx, gy), w, m in zip(got, want, mags):
        for i, g in enumerate((gx, gy)):
            err_f64 = c * 2.0 ** -52 * m[i]
            tol = 0.5 * float(np.spacing(np.float32(abs(float(w[i])) + err_f64))) + err_f64
            assert abs(Fraction(float(g)) - w[i]) <= Fraction(tol), (item, i, float(g), float(w[i]), tol)
            lo[i] = w[i] if lo[i] is None else min(lo[i], w[i])
            hi[i] = w[i] if hi[i] is None else max(hi[i], w[i])
    box = scene[8 + 8 * item : 16 + 8 * item].view(np.uint16)
    slack = max(max(m) for m in mags) * c * 2.0 ** -52
    sat = lambda v: int(min(max(v, 0), 65535))
    for got_v, edge, rnd in ((box[0], lo[0], np.floor), (box[1], lo[1], np.floor), (box[2], hi[0], np.ceil), (box[3], hi[1], np.ceil)):
        ok = {sat(rnd(float(edge))), sat(rnd(float(edge) - slack)), sat(rnd(float(edge) + slack))}
        assert int(got_v) in ok, (item, int(got_v), float(edge))


# ---- counts that cannot be stored ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("kind", ["inf", "1e30", "wrap"])
def test_flatten_edges_counts_beyond_the_scene(pm, pmo, renderer, kind):
    """One curve of 2^30 points (an infinite or a 1e30 control point) or 4 096 curves of 2^20 (2^32 points, which wrap to 1 in 32-bit
    sums): PM_ERR_CAPACITY at once, before any point is generated, and no grown buffer (the need is past 4 GiB); the context then
    flattens and renders the next scene as the oracle does; the host encoder returns the device's status on the same elements
    (identity transform -- where an infinite coordinate turns the other one into 0 * inf = NaN and the count into 1)."""
    case = huge_curve_case(kind)
    renderer.resize(case.width, case.height)
    t0 = time.monotonic()
    with pytest.raises(pm.PietMetalError) as ei:
        renderer.flatten_and_encode(case.ps, case.affine, case.scale)
    assert ei.value.status == pm._lib.PM_ERR_CAPACITY
    assert time.monotonic() - t0 < 5.0
    _device_matches_oracle(pm, pmo, renderer, EDGES["affine_sheared"])
    try:
        renderer.flatten_and_encode(case.ps, IDENTITY, case.scale)
        dev_status = pm._lib.PM_OK
    except pm.PietMetalError as err:
        dev_status = err.status
    host_status, _ = _host_encode(pm, case.ps, 1 << 20)
    assert host_status == dev_status == (pm._lib.PM_OK if kind == "inf" else pm._lib.PM_ERR_CAPACITY)
    _device_matches_oracle(pm, pmo, renderer, EDGES["compound_many_subpaths"])


@pytest.mark.timeout(20)
@pytest.mark.parametrize("kind", ["inf", "1e30", "wrap"])
def test_oracle_counts_beyond_the_scene(pm, pmo, kind):
    """The oracle counts a curve that does not fit without generating its points: it fails at once instead of looping 2^30 times
    (or 10^16 before its count rule was settled)."""
    case = huge_curve_case(kind)
    t0 = time.monotonic()
    assert _oracle_status(pmo, case, case.affine) < 0
    assert _oracle_status(pmo, case, case.affine, cap=1 << 31) < 0
    assert time.monotonic() - t0 < 5.0
