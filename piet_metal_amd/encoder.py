"""Scene encoder: the piet-metal `Encoder` API (src/lib.rs:79-254) over the C ABI.

Method names, argument order and error behaviour follow the Rust type: a misuse
that panics there (assert!/unwrap) raises PietMetalError here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class Encoder:
    """`Encoder::new(buf)`: writes the scene into a caller-owned byte buffer."""

    def __init__(self, buf: np.ndarray):
        if buf.dtype != np.uint8 or not buf.flags["C_CONTIGUOUS"]:
            raise TypeError("Encoder needs a contiguous uint8 buffer")
        self._lib = _lib.load()
        self._buf = buf  # keep alive
        self._h = self._lib.pm_encoder_new(buf.ctypes.data, buf.size)
        if not self._h:
            raise MemoryError("pm_encoder_new failed")

    def close(self) -> None:
        if self._h:
            self._lib.pm_encoder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, size: int) -> int:
        return int(self._lib.pm_encoder_alloc(self._h, size))

    def write_struct(self, ix: int, data: bytes) -> None:
        """Encoder::write_struct (src/lib.rs:122): raw bytes of a #[repr(C)] value at offset ix."""
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        _lib.check(self._lib.pm_encoder_write_struct(self._h, ix, buf, len(data)), "pm_encoder_write_struct")

    def encode_points(self, points):
        """Encoder::encode_points (src/lib.rs:224) -> (points_ix, (x0, y0, x1, y1))."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        ix = C.c_size_t(0)
        bb = (C.c_double * 4)()
        _lib.check(self._lib.pm_encoder_encode_points(self._h, pts.ctypes.data, len(pts), C.byref(ix), bb), "pm_encoder_encode_points")
        return int(ix.value), tuple(bb)

    def begin_group(self, n_items: int) -> None:
        """`Encoder::begin_group`; inside an open group it starts a nested group (extension)."""
        _lib.check(self._lib.pm_encoder_begin_group(self._h, n_items), "begin_group")

    def end_group(self) -> None:
        _lib.check(self._lib.pm_encoder_end_group(self._h), "end_group")

    def circle(self, center, radius: float) -> None:
        _lib.check(self._lib.pm_encoder_circle(self._h, center[0], center[1], radius), "circle")

    def fill_compound(self, subpaths, rgba: int, even_odd: bool = False) -> None:
        """Beyond the reference: ONE Fill item made of several closed sub-paths that share a winding
        sum (holes); `subpaths` is a sequence of (n, 2) point arrays."""
        subs = [np.ascontiguousarray(s, np.float64).reshape(-1, 2) for s in subpaths]
        counts = np.asarray([len(s) for s in subs], np.uint32)
        pts = np.concatenate(subs) if subs else np.zeros((0, 2), np.float64)
        _lib.check(self._lib.pm_encoder_fill_compound(self._h, pts.ctypes.data, counts.ctypes.data, len(subs), rgba,
                                                     _lib.PM_FILL_EVEN_ODD if even_odd else 0), "fill_compound")

    def fill_path(self, els: np.ndarray, rgba: int, even_odd: bool = False, compound: bool = False) -> None:
        """Beyond the reference: a path with curves and sub-paths (PathSet.EL_DTYPE elements), flattened
        on the host like make_tiger's encode_path; compound=True: ONE Fill item, holes are holes."""
        els = np.ascontiguousarray(els, dtype=_EL_DTYPE)
        flags = (_lib.PM_FILL_EVEN_ODD if even_odd else 0) | (_lib.PM_FILL_COMPOUND if compound else 0)
        _lib.check(self._lib.pm_encoder_fill_path(self._h, els.ctypes.data, len(els), rgba & 0xFFFFFFFF, flags), "fill_path")

    def stroke_path(self, els: np.ndarray, rgba: int, width: float) -> None:
        """A path's sub-paths as poly-lines, with the thin-line rule of encode_path_stroke."""
        els = np.ascontiguousarray(els, dtype=_EL_DTYPE)
        _lib.check(self._lib.pm_encoder_stroke_path(self._h, els.ctypes.data, len(els), rgba & 0xFFFFFFFF, float(width)), "stroke_path")

    def ellipse(self, center, rx: float, ry: float) -> None:
        """Beyond the reference: the ellipse inscribed in the item's bbox (a Circle item with the
        ellipse bit), shaded as PietRender.metal:488-489 says it should be."""
        _lib.check(self._lib.pm_encoder_ellipse(self._h, center[0], center[1], rx, ry), "ellipse")

    def stroke_line(self, p0, p1, width: float, rgba: int) -> None:
        _lib.check(
            self._lib.pm_encoder_stroke_line(self._h, p0[0], p0[1], p1[0], p1[1], width, rgba & 0xFFFFFFFF),
            "stroke_line",
        )

    @staticmethod
    def _pts(points) -> np.ndarray:
        a = np.ascontiguousarray(points, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("points must be (n, 2)")
        return a

    def fill(self, points, rgba: int, even_odd: bool = False) -> None:
        """`Encoder::fill`; even_odd sets the winding-rule bit of PietFill.flags (an extension
        the reference reserves the field for, src/lib.rs:54)."""
        a = self._pts(points)
        if even_odd:
            _lib.check(self._lib.pm_encoder_fill_rule(self._h, a.ctypes.data, a.shape[0], rgba & 0xFFFFFFFF, _lib.PM_FILL_EVEN_ODD), "fill")
        else:
            _lib.check(self._lib.pm_encoder_fill(self._h, a.ctypes.data, a.shape[0], rgba & 0xFFFFFFFF), "fill")

    def polyline(self, points, rgba: int, width: float) -> None:
        a = self._pts(points)
        _lib.check(
            self._lib.pm_encoder_polyline(self._h, a.ctypes.data, a.shape[0], rgba & 0xFFFFFFFF, width), "polyline"
        )

    @property
    def bytes_used(self) -> int:
        return int(self._lib.pm_encoder_bytes_used(self._h))


def scene_cardioid(buf: np.ndarray) -> int:
    """make_cardioid (src/lib.rs:257-270); returns bytes written."""
    n = _lib.load().pm_scene_cardioid(buf.ctypes.data, buf.size)
    if n < 0:
        raise _lib.PietMetalError(int(n), "pm_scene_cardioid")
    return int(n)


def scene_path_test(buf: np.ndarray) -> int:
    """make_path_test (src/lib.rs:273-284); returns bytes written."""
    n = _lib.load().pm_scene_path_test(buf.ctypes.data, buf.size)
    if n < 0:
        raise _lib.PietMetalError(int(n), "pm_scene_path_test")
    return int(n)


def parse_color(s: str) -> int:
    """parse_color (src/lib.rs:375-385)."""
    return int(_lib.load().pm_parse_color(s.encode()))


_PATH_DTYPE = np.dtype(
    [("el_begin", "<u4"), ("el_end", "<u4"), ("flags", "<u4"), ("fill_rgba", "<u4"), ("stroke_rgba", "<u4"), ("stroke_width", "<f4")]
)
_EL_DTYPE = np.dtype([("tag", "<u4"), ("pad", "<u4"), ("p", "<f8", (6,))])
_DASH_DTYPE = np.dtype([("path", "<u4"), ("first", "<u4"), ("count", "<u4"), ("offset", "<f4")])
assert _PATH_DTYPE.itemsize == 24 and _EL_DTYPE.itemsize == 56 and _DASH_DTYPE.itemsize == 16


def _dash_arrays(table: dict):
    """{path: (values, offset)} -> (dashes, dash_values) in the layout of pm_flatten_and_encode_dashed, ascending by path."""
    dashes = np.zeros(len(table), _DASH_DTYPE)
    values = []
    at = 0
    for k, i in enumerate(sorted(table)):
        v, off = table[i]
        dashes[k] = (i, at, len(v), off)
        values.append(np.asarray(v, np.float32))
        at += len(v)
    return dashes, (np.concatenate(values) if values else np.zeros(0, np.float32))


class PathSet:
    """Parsed paths: `paths` (structured, 24 B) and `els` (structured, 56 B) arrays
    in the layout of pm_path / pm_path_el; optionally a dash table (decision D15): `dashes`
    (structured, 16 B, pm_path_dash, ascending by path) and the f32 `dash_values` they index; optionally `groups` (decision D16):
    a uint32 group index per path, what Renderer.reflatten_groups moves together (None: no map; the set counts as one group)."""

    PATH_DTYPE = _PATH_DTYPE
    EL_DTYPE = _EL_DTYPE
    DASH_DTYPE = _DASH_DTYPE

    def __init__(self, paths: np.ndarray, els: np.ndarray, dashes: np.ndarray | None = None, dash_values: np.ndarray | None = None,
                 groups: np.ndarray | None = None):
        self.paths = np.ascontiguousarray(paths, dtype=_PATH_DTYPE)
        self.els = np.ascontiguousarray(els, dtype=_EL_DTYPE)
        self.dashes = np.ascontiguousarray(dashes if dashes is not None else np.zeros(0, _DASH_DTYPE), dtype=_DASH_DTYPE)
        self.dash_values = np.ascontiguousarray(dash_values if dash_values is not None else np.zeros(0, np.float32), dtype=np.float32)
        self.groups = None if groups is None else self._checked_groups(groups, len(self.paths))

    @staticmethod
    def _checked_groups(groups, n_paths: int) -> np.ndarray:
        g = np.asarray(groups)
        if g.shape != (n_paths,) or (g.size and not (np.issubdtype(g.dtype, np.integer) and g.min() >= 0 and g.max() <= 0xFFFFFFFF)):
            raise ValueError("groups is one uint32 group index per path")
        return np.ascontiguousarray(g, dtype=np.uint32)

    def n_groups(self) -> int:
        """Groups the set's map names (largest index + 1); a set without a map, or without paths, counts as one group."""
        return int(self.groups.max()) + 1 if self.groups is not None and len(self.groups) else 1

    def with_groups(self, groups) -> "PathSet":
        """A copy with this group map (decision D16): a uint32 group index per path, or None for no map."""
        out = self._like(self.paths, self.els)
        out.groups = None if groups is None else self._checked_groups(groups, len(self.paths))
        return out

    def _like(self, paths, els, dashes=None, dash_values=None) -> "PathSet":
        """A set of these arrays that keeps this one's dash table (unless given), group map and document attributes."""
        out = PathSet(paths, els, self.dashes if dashes is None else dashes, self.dash_values if dash_values is None else dash_values,
                      self.groups)
        for k in ("viewbox", "size"):
            if hasattr(self, k):
                setattr(out, k, getattr(self, k))
        return out

    @classmethod
    def _from_handle(cls, lib, h, groups: bool = False) -> "PathSet":
        try:
            npaths, nels = lib.pm_svg_n_paths(h), lib.pm_svg_n_els(h)
            paths = np.frombuffer(C.string_at(lib.pm_svg_paths(h), npaths * 24), dtype=_PATH_DTYPE).copy() if npaths else np.zeros(0, _PATH_DTYPE)
            els = np.frombuffer(C.string_at(lib.pm_svg_els(h), nels * 56), dtype=_EL_DTYPE).copy() if nels else np.zeros(0, _EL_DTYPE)
            ndash, nval = lib.pm_svg_n_dashes(h), lib.pm_svg_n_dash_values(h)
            dashes = np.frombuffer(C.string_at(lib.pm_svg_dashes(h), ndash * 16), dtype=_DASH_DTYPE).copy() if ndash else None
            values = np.frombuffer(C.string_at(lib.pm_svg_dash_values(h), nval * 4), dtype=np.float32).copy() if nval else None
            gmap = None
            if groups:
                gmap = np.frombuffer(C.string_at(lib.pm_svg_path_groups(h), npaths * 4), dtype=np.uint32).copy() if npaths else np.zeros(0, np.uint32)
            vb, w, hh = (C.c_double * 4)(), C.c_double(0), C.c_double(0)
            has_vb = lib.pm_svg_viewbox(h, vb, C.byref(w), C.byref(hh))
        finally:
            lib.pm_svg_free(h)
        ps = cls(paths, els, dashes, values, gmap)
        ps.viewbox = tuple(vb) if has_vb else None  # the outermost <svg>'s viewBox (user units)
        ps.size = (w.value, hh.value)                # its width / height in px (0: not given)
        return ps

    def fit_affine(self, width: int, height: int):
        """(affine, scale) that shows the document's viewBox (or its width x height) centred in a
        width x height viewport, aspect ratio kept (SVG's default preserveAspectRatio xMidYMid meet);
        None when the document gives neither."""
        vb = getattr(self, "viewbox", None)
        if vb is None:
            w, h = getattr(self, "size", (0.0, 0.0))
            if not (w > 0 and h > 0):
                return None
            vb = (0.0, 0.0, w, h)
        s = min(width / vb[2], height / vb[3])
        return (s, 0.0, 0.0, s, (width - s * vb[2]) / 2.0 - s * vb[0], (height - s * vb[3]) / 2.0 - s * vb[1]), s

    @classmethod
    def from_svg(cls, text: bytes | str, reject_arc_paths: bool = False, spec_defaults: bool = False, flat_gradients: bool = False,
                 stroke_styles: bool = False, stroke_dashes: bool = False, groups: bool = False) -> "PathSet":
        """Parse an SVG document.  spec_defaults: SVG's initial `fill: black` instead of the
        reference's rule that only a fill property fills (src/lib.rs:299); flat_gradients: a
        url(#gradient) paint becomes the mean colour of the gradient's stops instead of `none`;
        stroke_styles: stroke-linecap / stroke-linejoin / stroke-miterlimit are read and every stroke
        is drawn as its outline (decision D14) instead of the round poly-line; stroke_dashes (needs
        stroke_styles): stroke-dasharray / stroke-dashoffset are read into the dash table (decision D15); groups: `groups` is filled
        with the document's top-level groups (decision D16) -- for every path the ordinal, among the element children of the
        outermost <svg>, of the child that drew it (a <use>: the child where it stands)."""
        lib = _lib.load()
        data = text.encode() if isinstance(text, str) else bytes(text)
        err = C.c_int(0)
        flags = (_lib.PM_SVG_REJECT_ARC_PATHS if reject_arc_paths else 0) | (_lib.PM_SVG_SPEC_DEFAULTS if spec_defaults else 0)
        flags |= _lib.PM_SVG_FLAT_GRADIENTS if flat_gradients else 0
        flags |= _lib.PM_SVG_STROKE_STYLES if stroke_styles else 0
        flags |= _lib.PM_SVG_STROKE_DASHES if stroke_dashes else 0
        h = lib.pm_svg_parse(data, len(data), flags, C.byref(err))
        if not h:
            raise _lib.PietMetalError(err.value, "pm_svg_parse")
        return cls._from_handle(lib, h, groups)

    @classmethod
    def tiger(cls, reject_arc_paths: bool = False, groups: bool = False) -> "PathSet":
        """The embedded Ghostscript_Tiger.svg (src/lib.rs:288); groups as in from_svg."""
        lib = _lib.load()
        err = C.c_int(0)
        h = lib.pm_svg_tiger(_lib.PM_SVG_REJECT_ARC_PATHS if reject_arc_paths else 0, C.byref(err))
        if not h:
            raise _lib.PietMetalError(err.value, "pm_svg_tiger")
        return cls._from_handle(lib, h, groups)

    CAPS = {"butt": _lib.PM_STROKE_CAP_BUTT, "round": _lib.PM_STROKE_CAP_ROUND, "square": _lib.PM_STROKE_CAP_SQUARE}
    JOINS = {"miter": _lib.PM_STROKE_JOIN_MITER, "round": _lib.PM_STROKE_JOIN_ROUND, "bevel": _lib.PM_STROKE_JOIN_BEVEL}

    def with_stroke_style(self, cap="butt", join="miter", miter_limit: float = 4.0, select=None) -> "PathSet":
        """A copy whose stroked paths (all of them, or those of `select`: indices or a boolean mask) are drawn as outlines with
        this cap ("butt" / "round" / "square"), join ("miter" / "round" / "bevel") and miter limit (kept as binary16; >= 1):
        PM_PATH_STROKE_OUTLINE and the style fields of pm_path.flags.  Paths without a stroke are left alone."""
        half = int(np.array(miter_limit, np.float16).view(np.uint16))
        if not (np.float16(miter_limit) >= 1 and np.isfinite(np.float16(miter_limit))):
            raise ValueError("miter_limit must be a finite number >= 1")
        style = (_lib.PM_PATH_STROKE_OUTLINE | (self.CAPS[cap] << _lib.PM_STROKE_CAP_SHIFT) | (self.JOINS[join] << _lib.PM_STROKE_JOIN_SHIFT)
                 | (half << _lib.PM_STROKE_MITER_SHIFT))
        p = self.paths.copy()
        chosen = np.zeros(len(p), bool)
        chosen[slice(None) if select is None else select] = True
        chosen &= (p["flags"] & _lib.PM_PATH_STROKE) != 0
        p["flags"][chosen] = (p["flags"][chosen] & ~np.uint32(_lib.PM_PATH_STROKE_STYLE_MASK)) | np.uint32(style)
        return self._like(p, self.els)

    def with_dashes(self, pattern, offset: float = 0.0, select=None) -> "PathSet":
        """A copy whose stroked, outlined paths (all of them, or those of `select`: indices or a boolean mask) are dashed with
        `pattern` (1 .. 32 finite lengths >= 0 in user units, alternately dash and gap; an odd count repeats once) starting `offset`
        into it (decision D15).  Paths without PM_PATH_STROKE | PM_PATH_STROKE_OUTLINE are left alone (with_stroke_style first);
        a path that had a pattern gets the new one."""
        pat = np.asarray(pattern, np.float32).reshape(-1)
        if not (1 <= len(pat) <= 32 and np.all(np.isfinite(pat)) and np.all(pat >= 0) and np.isfinite(np.float32(offset))):
            raise ValueError("a dash pattern is 1 .. 32 finite values >= 0 and a finite offset")
        need = np.uint32(_lib.PM_PATH_STROKE | _lib.PM_PATH_STROKE_OUTLINE)
        chosen = np.zeros(len(self.paths), bool)
        chosen[slice(None) if select is None else select] = True
        chosen &= (self.paths["flags"] & need) == need
        table = {int(d["path"]): (self.dash_values[int(d["first"]) : int(d["first"]) + int(d["count"])], float(d["offset"])) for d in self.dashes}
        for i in np.flatnonzero(chosen):
            table[int(i)] = (pat, float(offset))
        return self._like(self.paths, self.els, *_dash_arrays(table))

    def fills_only(self) -> "PathSet":
        p = self.paths.copy()
        p["flags"] &= _lib.PM_PATH_FILL
        return PathSet(p, self.els, groups=self.groups)

    @staticmethod
    def concat(sets: list["PathSet"]) -> "PathSet":
        paths, els, base = [], [], 0
        dashes, values, pbase, vbase = [], [], 0, 0
        # group maps (decision D16): every set's indices behind those of the sets before it; a set without a map is one group
        groups, gbase, any_groups = [], 0, any(s.groups is not None for s in sets)
        for s in sets:
            groups.append((s.groups if s.groups is not None else np.zeros(len(s.paths), np.uint32)).astype(np.uint64) + gbase)
            gbase += s.n_groups()
            p = s.paths.copy()
            p["el_begin"] += base
            p["el_end"] += base
            base += len(s.els)
            paths.append(p)
            els.append(s.els)
            d = s.dashes.copy()
            d["path"] += pbase
            d["first"] += vbase
            pbase += len(s.paths)
            vbase += len(s.dash_values)
            dashes.append(d)
            values.append(s.dash_values)
        return PathSet(np.concatenate(paths), np.concatenate(els), np.concatenate(dashes), np.concatenate(values),
                       np.concatenate(groups) if any_groups else None)

    def transformed(self, affine) -> "PathSet":
        """Apply an affine [a b c d e f] to the element coordinates on the host
        (used to lay out multi-copy scenes before the device flatten)."""
        a, b, c, d, e, f = [float(v) for v in affine]
        els = self.els.copy()
        p = els["p"]
        x, y = p[:, 0::2].copy(), p[:, 1::2].copy()
        p[:, 0::2] = a * x + c * y + e
        p[:, 1::2] = b * x + d * y + f
        return PathSet(self.paths, els, self.dashes, self.dash_values, self.groups)  # (dash lengths are in user units: width_scale scales them)
