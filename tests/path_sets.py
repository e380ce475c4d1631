"""Path sets for the flatten + encode stage (test infrastructure): the random path grammar of the
flatten fuzzer, and a table of named edge cases -- inputs where the device flatten kernels
(piet_metal_amd/csrc/pm_flatten.hip), the host encoder and the oracle could part ways.

Every builder returns a `Case`: a PathSet, the affine and width scale it is encoded under, a small
viewport, and the status pm_flatten_and_encode must return (PM_OK unless the case says otherwise)."""
from dataclasses import dataclass

import numpy as np

import piet_metal_amd as pm
from piet_metal_amd import _lib

from np_scene import p6, subdivision_count

M, L, Q, C, Z = _lib.PM_EL_MOVE, _lib.PM_EL_LINE, _lib.PM_EL_QUAD, _lib.PM_EL_CURVE, _lib.PM_EL_CLOSE
FILL, STROKE, EVEN_ODD, COMPOUND = _lib.PM_PATH_FILL, _lib.PM_PATH_STROKE, _lib.PM_PATH_EVEN_ODD, _lib.PM_PATH_COMPOUND
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
MAX_HYPOT2 = 432.0 * (0.1 * 1e-2) * (0.1 * 1e-2)  # flatten.rs:35, what the kernels divide by


def random_pathset(rng, n_paths, extent):
    """Random paths: lines, quads, cubics, one to three sub-paths, open and closed, fills and strokes
    (thin ones included), even-odd and compound flags."""
    els, paths = [], []
    for _ in range(n_paths):
        e0 = len(els)
        for _sub in range(int(rng.integers(1, 4))):
            p = rng.uniform(0, extent, 2)
            els.append((_lib.PM_EL_MOVE, [p[0], p[1], 0, 0, 0, 0]))
            for _seg in range(int(rng.integers(1, 7))):
                kind = rng.integers(0, 3)
                step = float(rng.choice([3.0, 30.0, 150.0]))
                q = [p + rng.uniform(-step, step, 2) for _ in range(3)]
                if kind == 0:
                    els.append((_lib.PM_EL_LINE, [q[0][0], q[0][1], 0, 0, 0, 0])); p = q[0]
                elif kind == 1:
                    els.append((_lib.PM_EL_QUAD, [q[0][0], q[0][1], q[1][0], q[1][1], 0, 0])); p = q[1]
                else:
                    els.append((_lib.PM_EL_CURVE, [q[0][0], q[0][1], q[1][0], q[1][1], q[2][0], q[2][1]])); p = q[2]
            if rng.random() < 0.6:
                els.append((_lib.PM_EL_CLOSE, [0] * 6))
        flags = int(rng.integers(1, 4))  # fill, stroke or both
        flags |= (4 if rng.random() < 0.3 else 0) | (8 if rng.random() < 0.4 else 0)  # even-odd rule, compound fill
        rgba = lambda: (int(rng.integers(0, 1 << 24)) << 8 | (0xFF if rng.random() < 0.4 else int(rng.integers(1, 255)))) & 0xFFFFFFFF
        width = float(rng.choice([0.05, 0.3, 1.0, 4.0]))
        paths.append((e0, len(els), flags, rgba(), rgba(), width))
    E = np.zeros(len(els), pm.PathSet.EL_DTYPE)
    for i, (t, p) in enumerate(els):
        E["tag"][i] = t; E["p"][i] = p
    P = np.array(paths, dtype=pm.PathSet.PATH_DTYPE)
    return pm.PathSet(P, E)


def random_case(seed):
    """The fuzzer's draw for one seed, at a small viewport (the oracle renders it on the CPU), plus a second affine for
    pm_reflatten."""
    rng = np.random.default_rng(seed * 104729 + 7)
    ps = random_pathset(rng, int(rng.integers(1, 40)), float(rng.choice([100.0, 300.0])))
    s = float(rng.choice([0.5, 1.0, 2.7]))
    th = rng.uniform(0, 6.28) if rng.random() < 0.5 else 0.0
    aff = (s * np.cos(th), s * np.sin(th), -s * np.sin(th), s * np.cos(th), float(rng.uniform(-50, 100)), float(rng.uniform(-50, 100)))
    aff2 = (-0.8 * s, 0.3, 0.2, 1.1 * s, float(rng.uniform(100, 200)), float(rng.uniform(-20, 40)))
    return Case(ps, tuple(float(v) for v in aff), s, int(rng.integers(32, 200)), int(rng.integers(32, 160)), affine2=aff2)


@dataclass
class Case:
    ps: "pm.PathSet"
    affine: tuple = IDENTITY
    scale: float = 1.0
    width: int = 128
    height: int = 128
    status: int = _lib.PM_OK
    affine2: tuple = (0.9, 0.1, -0.2, -1.1, 20.0, 140.0)  # mirrored + sheared: the reflatten under a second view


def pathset(*paths):
    """paths: (elements, flags[, stroke width]); an element is (tag, *coordinates)."""
    els, rows = [], []
    for k, spec in enumerate(paths):
        path_els, flags = spec[0], spec[1]
        width = spec[2] if len(spec) > 2 else 2.0
        e0 = len(els)
        for tag, *xy in path_els:
            els.append((tag, list(xy) + [0.0] * (6 - len(xy))))
        fill = (0x2060A0FF + 0x01230000 * k) & 0xFFFFFFFF
        stroke = (0xC0402080 + 0x00041100 * k) & 0xFFFFFFFF
        rows.append((e0, len(els), flags, fill, stroke, width))
    E = np.zeros(len(els), pm.PathSet.EL_DTYPE)
    for i, (t, p) in enumerate(els):
        E["tag"][i] = t
        E["p"][i] = p
    return pm.PathSet(np.array(rows, dtype=pm.PathSet.PATH_DTYPE), E)


def _square(x, y, s):
    return [(M, x, y), (L, x + s, y), (L, x + s, y + s), (L, x, y + s), (Z,)]


def _wiggle(x, y, n, rng):
    """A sub-path of n elements: one MoveTo, then lines and cubics in turn."""
    out = [(M, x, y)]
    for k in range(n - 1):
        nx, ny = x + rng.uniform(-6, 9), y + rng.uniform(-6, 9)
        if k % 3 == 2:
            out.append((C, x + rng.uniform(-9, 9), y + rng.uniform(-9, 9), nx + rng.uniform(-9, 9), ny + rng.uniform(-9, 9), nx, ny))
        else:
            out.append((L, nx, ny))
        x, y = min(max(nx, 4.0), 120.0), min(max(ny, 4.0), 120.0)
    return out


def _tri(x, y):
    return [(M, x, y), (L, x + 30, y + 5), (C, x + 40, y + 20, x + 10, y + 40, x + 5, y + 30)]


def curve_for_x(target, where):
    """A curve (after MoveTo (0,0), under the identity) whose kernel-side x -- |3 p2 - p3 - 3 p1 + p0|^2 / max_hypot2, in binary64 as
    pm_flatten.hip computes it -- is `target` ('at'), the largest value below it ('below') or the smallest above it ('above') that a
    search of +-4096 ulps of the control point reaches.  Returns (element, x)."""
    c0 = (target * MAX_HYPOT2) ** 0.5 / 3.0
    xs = {}
    c = c0
    for _ in range(4096):
        c = np.nextafter(c, 0.0)
    for _ in range(8192):
        dx = c * 3.0 - 0.0  # bx - ax with p1 = p0 = p3 = (0, 0): (3 p2 - p3) - (3 p1 - p0)
        x = (dx * dx + 0.0 * 0.0) / MAX_HYPOT2
        xs.setdefault(x, float(c))
        c = np.nextafter(c, np.inf)
    if where == "at":
        if target not in xs:
            return None
        x = target
    elif where == "below":
        x = max(v for v in xs if v < target)
    else:
        x = min(v for v in xs if v > target)
    c = xs[x]
    return (C, 0.0, 0.0, c, 0.0, 0.0, 0.0), x


def p6_rounds_up_above_406():
    """The first k > 406 whose binary64 k^6 (p6) lies ABOVE the exact k^6: at x = p6(k) the product's rule says k, exact integers k + 1."""
    from fractions import Fraction

    k = 407
    while Fraction(p6(k)) <= k ** 6:
        k += 1
    return k


def count_boundary_curves():
    """(element, x) at x = k^6 and one reachable ulp either side for k = 1, 2, 7, 64, 405, and at x = p6(k) for a k above 406
    where p6 rounds up."""
    out = []
    for k in (1, 2, 7, 64, 405):
        for where in ("below", "at", "above"):
            r = curve_for_x(float(k ** 6), where)
            if r is not None:
                out.append(r)
    k = p6_rounds_up_above_406()
    for where in ("below", "at", "above"):
        r = curve_for_x(p6(k), where)
        if r is not None:
            out.append(r)
    return out


def _thin_widths():
    w = np.float32(0.7)
    return [float(np.nextafter(w, np.float32(0))), float(w), float(np.nextafter(w, np.float32(1)))]


def edge_cases():
    """name -> Case.  Small scenes; every one is checked against the oracle (bytes, pixels, reflatten)."""
    rng = np.random.default_rng(5)
    cases = {}
    tri = _tri(20, 20)
    cases["empty_paths_start_middle_end"] = Case(pathset(([], FILL), ([], STROKE), (tri, FILL | STROKE), ([], FILL), ([], FILL | COMPOUND),
                                                         (_square(60, 60, 30), FILL), ([], STROKE), ([], FILL)))
    cases["all_paths_empty"] = Case(pathset(([], FILL), ([], STROKE | FILL)))
    cases["lone_move"] = Case(pathset(([(M, 40, 40)], FILL | STROKE), (tri, FILL)))
    cases["consecutive_moves"] = Case(pathset(([(M, 10, 10), (M, 30, 50), (M, 70, 20), (L, 90, 90), (C, 60, 100, 30, 80, 20, 60)], FILL | STROKE),
                                              ([(M, 5, 5), (M, 50, 50), (L, 100, 20), (L, 110, 60)], FILL | COMPOUND)))
    cases["move_last"] = Case(pathset(([(M, 10, 10), (L, 90, 20), (C, 100, 60, 50, 100, 20, 90), (M, 120, 120)], FILL | STROKE),
                                      ([(M, 10, 100), (L, 40, 110), (L, 20, 70), (M, 60, 60)], FILL | COMPOUND | EVEN_ODD)))
    # the curve's start is the point BEFORE the QuadTo / ClosePath (flatten.rs keeps last_pt only across Move / Line / Curve)
    cases["quad_between_line_and_curve"] = Case(pathset(([(M, 10, 10), (L, 60, 15), (Q, 100, 100, 5, 120), (C, 90, 40, 80, 90, 30, 110)], FILL | STROKE)))
    cases["close_between_line_and_curve"] = Case(pathset(([(M, 10, 10), (L, 60, 15), (L, 70, 70), (Z,), (C, 90, 40, 80, 90, 30, 110)], FILL | STROKE)))
    cases["quad_and_close_before_curve"] = Case(pathset(([(M, 20, 10), (C, 60, 5, 80, 40, 70, 60), (Q, 10, 100, 50, 50), (Z,), (Q, 1, 2, 3, 4),
                                                          (C, 100, 100, 20, 110, 10, 70)], FILL | STROKE | EVEN_ODD)))
    cases["curve_after_close"] = Case(pathset(([(M, 10, 10), (L, 80, 20), (L, 60, 70), (Z,), (C, 110, 30, 120, 100, 40, 120), (L, 15, 90), (Z,)],
                                               FILL | STROKE)))
    cases["only_quads_and_closes"] = Case(pathset(([(M, 10, 10), (Q, 50, 90, 100, 10), (Q, 60, 60, 20, 100), (Z,)], FILL | STROKE),
                                                  ([(Q, 5, 5, 50, 50), (Z,), (Q, 1, 1, 2, 2)], FILL | STROKE | COMPOUND), (tri, FILL)))
    cases["line_before_move"] = Case(pathset((tri, FILL), ([(L, 10, 10), (M, 20, 20), (L, 50, 50)], FILL)), status=_lib.PM_ERR_INVALID)
    cases["curve_before_move"] = Case(pathset(([(Q, 1, 1, 2, 2), (C, 10, 10, 20, 20, 30, 30), (M, 20, 20), (L, 50, 50)], STROKE)),
                                      status=_lib.PM_ERR_INVALID)
    cases["degenerate_cubics"] = Case(pathset(
        ([(M, 50, 50), (C, 50, 50, 50, 50, 50, 50), (L, 90, 60)], FILL | STROKE),         # all four points equal
        ([(M, 10, 10), (C, 40, 40, 70, 70, 100, 100), (L, 100, 20)], FILL | STROKE),      # collinear
        ([(M, 10, 110), (C, 110, 10, 10, 10, 110, 110)], FILL | STROKE),                   # crossed control polygon: a cusp
        ([(M, 30, 30), (C, 120, 10, 120, 120, 30, 30)], FILL | STROKE | COMPOUND),         # p3 == p0: a loop
        ([(M, 60, 60), (C, 60, 60, 100, 20, 60, 60)], FILL | STROKE),                      # p3 == p0 == p1
    ))
    cases["signed_zeros"] = Case(pathset(([(M, -0.0, -0.0), (L, 50.0, -0.0), (C, 60.0, 40.0, -0.0, 60.0, -0.0, 30.0)], FILL | STROKE | COMPOUND)))
    for n in (63, 64, 65, 200):  # KItems runs one wave per sub-path
        cases[f"subpath_of_{n}_elements"] = Case(pathset((_wiggle(30, 30, n, rng) + [(Z,)] + _wiggle(80, 80, 3, rng), FILL | STROKE),
                                                         (_wiggle(60, 20, n, rng), FILL | COMPOUND | EVEN_ODD)))
    many = [el for k in range(70) for el in _square(4 + (k % 10) * 12, 4 + (k // 10) * 12 + (k % 3), 8 + (k % 4))]
    cases["compound_many_subpaths"] = Case(pathset((many, FILL | COMPOUND), (many, FILL | COMPOUND | EVEN_ODD | STROKE, 0.5)))
    cases["thin_line_threshold"] = Case(pathset(*[(_wiggle(20 + 25 * k, 30, 8, rng), STROKE | (FILL if k == 1 else 0), w)
                                                  for k, w in enumerate(_thin_widths())]))
    cases["thin_line_threshold_scaled"] = Case(pathset(*[(_wiggle(20 + 25 * k, 30, 8, rng), STROKE, w / 2.0) for k, w in enumerate(_thin_widths())]),
                                               affine=(2.0, 0.0, 0.0, 2.0, 0.0, 0.0), scale=2.0)
    body = lambda: pathset((_wiggle(30, 40, 30, rng), FILL | STROKE), (_tri(50, 10) + _square(10, 80, 30), FILL | COMPOUND | STROKE, 0.4),
                           (_tri(70, 60), STROKE | EVEN_ODD | FILL, 3.0))
    cases["affine_identity"] = Case(body())
    cases["affine_mirrored"] = Case(body(), affine=(-1.25, 0.0, 0.0, 1.0, 150.0, 5.0), scale=1.25)
    cases["affine_sheared"] = Case(body(), affine=(1.0, 0.35, -0.6, 0.9, 60.0, 0.0), scale=1.1)
    cases["affine_far_outside"] = Case(body(), affine=(1.0, 0.0, 0.0, 1.0, -1.0e5, 7.0e4))  # ShortBbox saturates at 0 and 65535
    cases["affine_straddling_u16"] = Case(body(), affine=(3.0, 0.0, 0.0, -3.0, 65480.0, 100.0), scale=3.0, width=160, height=120)
    curves = count_boundary_curves()
    sub = lambda el: [(M, 0.0, 0.0), el, (L, 0.0, 0.0)]
    cases["counts_on_sixth_power_boundaries"] = Case(pathset(*[(sub(el), FILL | STROKE) for el, _ in curves]), affine=(1e-3, 0.0, 0.0, 1e-3, 10.0, 10.0))
    return cases


def huge_curve_case(kind):
    """Curves whose counts cannot be stored: 'inf' -- one control point at +inf (under a rotation, so that no coordinate becomes
    0 * inf = NaN): n = 2^30; '1e30' -- a 1e30 control point, x ~ 2e64 > 1e54: n = 2^30; 'wrap' -- 4 096 curves of n = 2^20 each
    in one filled path: 2^32 + 1 encoded points, which wrap to 1 in 32 bits."""
    rot = (0.8, 0.6, -0.6, 0.8, 10.0, 10.0)
    if kind == "inf":
        return Case(pathset(([(M, 10, 10), (C, np.inf, 5.0, 20, 20, 30, 30), (L, 5, 40)], FILL), (_tri(20, 20), FILL | STROKE)), affine=rot,
                    status=_lib.PM_ERR_CAPACITY)
    if kind == "1e30":
        return Case(pathset((_tri(20, 20), FILL), ([(M, 10, 10), (C, 1e30, 5.0, 20, 20, 30, 30), (L, 5, 40)], STROKE)),
                    status=_lib.PM_ERR_CAPACITY)
    assert kind == "wrap"
    el, x = curve_for_x(p6(1 << 20), "at") or curve_for_x(p6(1 << 20), "below")
    assert subdivision_count(x) == 1 << 20
    return Case(pathset(([(M, 0.0, 0.0)] + [el] * 4096, FILL)), status=_lib.PM_ERR_CAPACITY)
