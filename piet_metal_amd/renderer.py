"""Renderer: the host-side mirror of PietRenderer (TestApp/PietRenderer.{h,m}).

    PietRenderer                          piet_metal_amd.Renderer
    -initWithMetalKitView:                Renderer(device)
    -mtkView:drawableSizeWillChange:      resize(w, h)          (+ set_band for multi-GPU)
    initScene / init_test_scene           scene_buffer() + upload_scene(), or
                                          flatten_and_encode(paths, affine)
    -drawInMTKView:                       render() / render_to(tensor)

All work happens in libpiet_metal_amd.so (HIP kernels); this file only moves
pointers.  torch is optional here and only used as a device-memory / stream
provider (render_to) -- plumbing, not the product.
"""
from __future__ import annotations

import ctypes as C
import operator
from fractions import Fraction

import numpy as np

from . import _lib
from .encoder import PathSet


_warned_default_stream = False

# pm_snap_result (decision D21): what Renderer.snap returns, 32 bytes a record
SNAP_DTYPE = np.dtype([("item", "<u4"), ("kind", "<u4"), ("index", "<u4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("d2", "<f8")])
assert SNAP_DTYPE.itemsize == 32
# pm_snap_cross_result (decision D23): what Renderer.snap_intersections returns, 48 bytes a record whose first 32 are SNAP_DTYPE's
SNAP_CROSS_DTYPE = np.dtype(SNAP_DTYPE.descr + [("item2", "<u4"), ("index2", "<u4"), ("u", "<f4"), ("n_near", "<u4")])
assert SNAP_CROSS_DTYPE.itemsize == 48
# pm_label_bounds (decision D22): what Renderer.union_bounds returns, 40 bytes a record
LABEL_BOUNDS_DTYPE = np.dtype([("box", "<f8", (4,)), ("n_items", "<u4"), ("n_boxed", "<u4")])
assert LABEL_BOUNDS_DTYPE.itemsize == 40
# pm_coverage (decision D28): what Renderer.item_coverage returns, 16 bytes a record
COVERAGE_DTYPE = np.dtype([("covered", "<u4"), ("visible", "<u4"), ("top", "<u4"), ("first_visible", "<u4")])
assert COVERAGE_DTYPE.itemsize == 16
# the records and queries of path measurement (decision D25): lengths and positions are integers in units of 2^-16 px
ITEM_LENGTH_DTYPE = np.dtype([("length", "<u8"), ("n_segments", "<u4"), ("kind", "<u4")])
LENGTH_QUERY_DTYPE = np.dtype([("item", "<u4"), ("reserved", "<u4"), ("s", "<u8")])
LENGTH_POINT_DTYPE = np.dtype([("item", "<u4"), ("status", "<u4"), ("index", "<u4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("tx", "<f4"), ("ty", "<f4")])
EDGE_QUERY_DTYPE = np.dtype([("item", "<u4"), ("index", "<u4"), ("t", "<f4"), ("reserved", "<u4")])
LENGTH_AT_DTYPE = np.dtype([("s", "<u8"), ("item", "<u4"), ("status", "<u4")])
assert (ITEM_LENGTH_DTYPE.itemsize, LENGTH_QUERY_DTYPE.itemsize, LENGTH_POINT_DTYPE.itemsize, EDGE_QUERY_DTYPE.itemsize, LENGTH_AT_DTYPE.itemsize) == (16, 16, 32, 16, 16)
LENGTH_UNIT = 65536  # units of a length per pixel
# the requests and infos of resampling (decision D26); its records are LENGTH_POINT_DTYPE
RESAMPLE_QUERY_DTYPE = np.dtype([("item", "<u4"), ("mode", "<u4"), ("count", "<u4"), ("first", "<u4"), ("start", "<u8"), ("step", "<u8")])
RESAMPLE_INFO_DTYPE = np.dtype([("length", "<u8"), ("n_unclamped", "<u4"), ("kind", "<u4")])
assert (RESAMPLE_QUERY_DTYPE.itemsize, RESAMPLE_INFO_DTYPE.itemsize) == (32, 16)
# the requests, vertices and infos of trimming (decision D27)
TRIM_QUERY_DTYPE = np.dtype([("item", "<u4"), ("mode", "<u4"), ("first", "<u4"), ("cap", "<u4"), ("s0", "<u8"), ("s1", "<u8")])
TRIM_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("index", "<u4"), ("flags", "<u4")])
TRIM_INFO_DTYPE = np.dtype([("length", "<u8"), ("n_vertices", "<u4"), ("n_runs", "<u4"), ("kind", "<u4"), ("flags", "<u4")])
assert (TRIM_QUERY_DTYPE.itemsize, TRIM_VERTEX_DTYPE.itemsize, TRIM_INFO_DTYPE.itemsize) == (32, 16, 24)
# the requests, records and infos of item crossings (decision D29); a record's first and second 16 bytes are each an EDGE_QUERY_DTYPE
CROSSINGS_QUERY_DTYPE = np.dtype([("item_a", "<u4"), ("item_b", "<u4"), ("first", "<u4"), ("cap", "<u4")])
CROSSING_DTYPE = np.dtype([("item_a", "<u4"), ("index_a", "<u4"), ("t", "<f4"), ("reserved_a", "<u4"), ("item_b", "<u4"), ("index_b", "<u4"), ("u", "<f4"),
                           ("reserved_b", "<u4"), ("x", "<f4"), ("y", "<f4"), ("side", "<u4"), ("reserved", "<u4")])
CROSSINGS_INFO_DTYPE = np.dtype([("n_crossings", "<u4"), ("flags", "<u4"), ("n_a", "<u4"), ("n_b", "<u4")])
assert (CROSSINGS_QUERY_DTYPE.itemsize, CROSSING_DTYPE.itemsize, CROSSINGS_INFO_DTYPE.itemsize) == (16, 48, 16)


def length_units(px) -> int:
    """D15's fix: a distance in pixels as a position in units of 2^-16 px -- min(floor(px * 65536 + 0.5), 2^64 - 1), 0 for a NaN or a
    negative value."""
    v = np.float64(px)
    if not v > 0:
        return 0
    f = np.floor(v * np.float64(LENGTH_UNIT) + 0.5)
    return (1 << 64) - 1 if f >= 2.0 ** 64 else int(f)


def resample_positions(mode: int, count: int, length: int, kind: int, start: int = 0, step: int = 0) -> list:
    """D26's positions s_0 .. s_{count-1} of a request, in units of 2^-16 px as Python integers: where the device put the points it
    answered with.  `length` and `kind` are the request's info record's."""
    if mode == _lib.PM_RESAMPLE_STEP:
        return [min(start + j * step, (1 << 64) - 1) for j in range(count)]
    m = count - 1 if kind == _lib.PM_MEASURE_OPEN else (count if kind == _lib.PM_MEASURE_CLOSED else 0)
    if m <= 0:
        return [0] * count
    d, r = divmod(length, m)
    return [j * d + min(j, r) for j in range(count)]


def trim_runs(vertices) -> list:
    """The poly-line runs of trimmed vertices (TRIM_VERTEX_DTYPE, one piece or several in a row): split at every PM_TRIM_MOVE into a
    list of float32 (n, 2) arrays, each what Encoder.polyline takes."""
    v = np.asarray(vertices)
    starts = np.flatnonzero(v["flags"] & _lib.PM_TRIM_MOVE)
    xy = np.stack([v["x"], v["y"]], axis=1).astype(np.float32, copy=False) if len(v) else np.zeros((0, 2), np.float32)
    if len(v) and (len(starts) == 0 or starts[0] != 0):
        raise ValueError("the first vertex of a piece starts a run")
    return [xy[a:b] for a, b in zip(starts.tolist(), starts.tolist()[1:] + [len(v)])]


def _warn_default_stream() -> None:
    global _warned_default_stream
    if not _warned_default_stream:
        _warned_default_stream = True
        import warnings

        warnings.warn("piet_metal_amd: torch's default stream (handle 0) cannot be named through the C ABI -- the frame ran on the context's "
                      "own stream and was waited for; pass a torch.cuda.Stream() to keep the submission asynchronous", RuntimeWarning, stacklevel=3)


class Renderer:
    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        err = C.c_int(0)
        self._h = self._lib.pm_create(device, C.byref(err))
        if not self._h:
            raise _lib.PietMetalError(err.value, "pm_create")
        self.device = device
        self.width = self.height = 0
        self.row0 = self.row1 = 0
        self._path_groups = None  # the map given in set_path_groups (group_bounds labels items with it)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- viewport ---------------------------------------------------------------
    def resize(self, width: int, height: int) -> None:
        _lib.check(self._lib.pm_resize(self._h, width, height), "pm_resize")
        self.width, self.height = width, height
        self.row0, self.row1 = 0, (height + 15) // 16

    def set_band(self, tile_row0: int, tile_row1: int) -> None:
        _lib.check(self._lib.pm_set_band(self._h, tile_row0, tile_row1), "pm_set_band")
        self.row0, self.row1 = tile_row0, tile_row1

    @property
    def band_pixel_rows(self) -> int:
        return min(self.row1 * 16, self.height) - self.row0 * 16

    # ---- scene --------------------------------------------------------------------
    def scene_buffer(self) -> np.ndarray:
        """Pinned host staging buffer (the reference's _sceneBuf.contents)."""
        cap = C.c_size_t(0)
        p = self._lib.pm_scene_buffer(self._h, C.byref(cap))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cap.value,))

    def reserve_scene(self, nbytes: int) -> None:
        _lib.check(self._lib.pm_scene_reserve(self._h, nbytes), "pm_scene_reserve")

    def upload_scene(self, nbytes: int) -> None:
        _lib.check(self._lib.pm_upload_scene(self._h, nbytes), "pm_upload_scene")

    def set_scene_bytes(self, data: bytes | np.ndarray) -> None:
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        if a.size > self.scene_buffer().size:
            self.reserve_scene(int(a.size))
        self.scene_buffer()[: a.size] = a
        self.upload_scene(int(a.size))

    def flatten_and_encode(self, paths: PathSet, affine, width_scale: float) -> tuple[int, int]:
        """On-device flatten + encode; returns (scene_bytes, n_items).  A set with a dash table (PathSet.with_dashes,
        from_svg(stroke_dashes=True)) goes through pm_flatten_and_encode_dashed."""
        aff = (C.c_double * 6)(*[float(v) for v in affine])
        nbytes, nitems = C.c_size_t(0), C.c_uint32(0)
        if len(paths.dashes):
            _lib.check(
                self._lib.pm_flatten_and_encode_dashed(
                    self._h, paths.paths.ctypes.data, len(paths.paths), paths.els.ctypes.data, len(paths.els), paths.dashes.ctypes.data,
                    len(paths.dashes), paths.dash_values.ctypes.data, len(paths.dash_values), aff, float(width_scale), C.byref(nbytes), C.byref(nitems),
                ),
                "pm_flatten_and_encode_dashed",
            )
        else:
            _lib.check(
                self._lib.pm_flatten_and_encode(
                    self._h, paths.paths.ctypes.data, len(paths.paths), paths.els.ctypes.data, len(paths.els), aff,
                    float(width_scale), C.byref(nbytes), C.byref(nitems),
                ),
                "pm_flatten_and_encode",
            )
        self._path_groups = None
        if getattr(paths, "groups", None) is not None:
            self.set_path_groups(paths.groups)
        return nbytes.value, nitems.value

    def set_path_groups(self, groups) -> None:
        """Give every resident path its group index (decision D16): what reflatten_groups moves together.  The map stays with
        the resident paths until the next flatten_and_encode."""
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        if g.ndim != 1:
            raise ValueError("groups is one uint32 group index per path")
        _lib.check(self._lib.pm_path_groups(self._h, g.ctypes.data, len(g)), "pm_path_groups")
        self._path_groups = g.copy()

    GROUP_XFORM_DTYPE = np.dtype([("m", "<f8", (6,)), ("width_scale", "<f4"), ("reserved", "<u4")])  # pm_group_xform

    def reflatten_groups(self, affines, width_scales=None) -> tuple[int, int]:
        """Re-flatten the resident paths with one transform per group (animating objects: no upload, no allocation):
        affines is (G, 6) float64, [a b c d e f] per group; width_scales (G,) scales stroke widths and dash lengths per group,
        by default sqrt|det| of each matrix, computed in float64 and rounded to f32.  Returns (scene_bytes, n_items)."""
        a = np.asarray(affines, np.float64)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError("affines is a (G, 6) array")
        if width_scales is None:
            ws = np.sqrt(np.abs(a[:, 0] * a[:, 3] - a[:, 1] * a[:, 2])).astype(np.float32)
        else:
            ws = np.asarray(width_scales, np.float32).reshape(-1)
            if ws.shape != (len(a),):
                raise ValueError("width_scales is one value per group")
        table = np.zeros(len(a), self.GROUP_XFORM_DTYPE)
        table["m"] = a
        table["width_scale"] = ws
        nbytes, nitems = C.c_size_t(0), C.c_uint32(0)
        _lib.check(self._lib.pm_reflatten_groups(self._h, table.ctypes.data, len(table), C.byref(nbytes), C.byref(nitems)), "pm_reflatten_groups")
        return nbytes.value, nitems.value

    GROUP_PAINT_DTYPE = np.dtype([("tint_rgba", "<u4"), ("opacity", "<u4")])  # pm_group_paint

    def repaint_groups(self, opacities=None, tints=None) -> None:
        """Fade and tint the groups of the resident paths (decision D17: colours only -- no flatten, no read-back, the scene index
        and the binning plan stay): opacities is one value 0..255 per group, multiplying every alpha of the group's paths; tints
        one 0xRRGGBBAA per group, the colour mixed into R, G, B and, as AA, how much of it.  None means the identity for that field
        (opacity 255, tint 0).  Every call starts from the paths' own colours: paints do not accumulate.  The paint stays in force
        for later reflatten / reflatten_groups calls, until the next flatten_and_encode."""
        if opacities is None and tints is None:
            raise ValueError("repaint_groups needs opacities, tints or both (one value per group)")
        o = None if opacities is None else np.asarray(opacities).reshape(-1)
        t = None if tints is None else np.asarray(tints).reshape(-1)
        if o is not None and t is not None and len(o) != len(t):
            raise ValueError("opacities and tints are one value per group each")
        for v in (o, t):
            if v is not None and v.size and not (np.issubdtype(v.dtype, np.integer) and v.min() >= 0 and v.max() <= 0xFFFFFFFF):
                raise ValueError("opacities and tints are unsigned integers")
        table = np.zeros(len(o if o is not None else t), self.GROUP_PAINT_DTYPE)
        table["opacity"] = 255 if o is None else o
        table["tint_rgba"] = 0 if t is None else t
        _lib.check(self._lib.pm_repaint_groups(self._h, table.ctypes.data, len(table)), "pm_repaint_groups")

    def reflatten(self, affine, width_scale: float) -> tuple[int, int]:
        """Re-flatten the resident paths of the last flatten_and_encode under a new affine
        (animation: no upload, no allocation); returns (scene_bytes, n_items)."""
        aff = (C.c_double * 6)(*[float(v) for v in affine])
        nbytes, nitems = C.c_size_t(0), C.c_uint32(0)
        _lib.check(self._lib.pm_reflatten(self._h, aff, float(width_scale), C.byref(nbytes), C.byref(nitems)), "pm_reflatten")
        return nbytes.value, nitems.value

    def download_scene(self) -> np.ndarray:
        nbytes = C.c_size_t(0)
        self._lib.pm_scene_device_ptr(self._h, C.byref(nbytes))
        out = np.zeros(max(nbytes.value, 8), np.uint8)
        _lib.check(self._lib.pm_download_scene(self._h, out.ctypes.data, out.size, C.byref(nbytes)), "pm_download_scene")
        return out[: nbytes.value]

    # ---- frames ---------------------------------------------------------------------
    def render(self) -> None:
        _lib.check(self._lib.pm_render(self._h), "pm_render")

    def render_to(self, tensor, stream=None) -> None:
        """Render into a torch uint8 CUDA tensor of shape [band_rows, width, 4], on `stream` (a torch stream) -- None, or
        torch's legacy default stream (handle 0), means the context's OWN stream: order later work on torch's side with
        sync(), or make the current stream a torch.cuda.Stream() first (bench.py does)."""
        if tensor.dtype.__str__() != "torch.uint8" or not tensor.is_cuda or tensor.dim() != 3 or tensor.shape[2] != 4:
            raise TypeError("render_to needs a CUDA uint8 tensor [rows, width, 4]")
        if tensor.shape[1] != self.width or tensor.shape[0] < self.band_pixel_rows or tensor.stride(1) != 4 or tensor.stride(2) != 1:
            raise ValueError("tensor does not match the viewport band")
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_render_to(self._h, tensor.data_ptr(), tensor.stride(0), s), "pm_render_to")
        if stream is not None and not s:
            # torch's legacy default stream has handle 0, which the C ABI reads as "the context's own stream": the frame would run
            # BESIDE the torch work queued on that tensor, not behind it (round-5 advisor).  Not silently: the frame is waited for
            # here, so that whatever the caller queues next on any stream sees it complete, and the caller is told once.
            _warn_default_stream()
            self.sync()

    def sync(self) -> None:
        _lib.check(self._lib.pm_sync(self._h), "pm_sync")

    def set_target_format(self, bgra: bool) -> None:
        """Byte order the kernels store pixels in from now on: RGBA8 (default) or BGRA8, the
        reference drawable's MTLPixelFormatBGRA8Unorm (PietRenderer.m:29)."""
        _lib.check(self._lib.pm_set_target_format(self._h, _lib.PM_FMT_BGRA8 if bgra else _lib.PM_FMT_RGBA8), "pm_set_target_format")

    def read_pixels(self, bgra: bool = False) -> np.ndarray:
        out = np.zeros((self.band_pixel_rows, self.width, 4), np.uint8)
        _lib.check(
            self._lib.pm_read_pixels(self._h, out.ctypes.data, self.width * 4, _lib.PM_FMT_BGRA8 if bgra else _lib.PM_FMT_RGBA8),
            "pm_read_pixels",
        )
        return out

    def time_frames(self, iters: int, per_kernel: bool = True, pipelined: bool = False) -> dict:
        """total_ms: `iters` frames through the frame pipeline.  bin/coarse/fine_ms: average
        launch duration of the three kernels -- each alone on the GPU (default), or inside
        the overlapping pipelined batch (pipelined=True)."""
        tot, k1, k2, k3, k4 = C.c_float(0), C.c_float(0), C.c_float(0), C.c_float(0), C.c_float(0)
        pk = per_kernel
        fn = self._lib.pm_time_frames_pipelined if pipelined else self._lib.pm_time_frames
        _lib.check(
            fn(self._h, iters, C.byref(tot), C.byref(k1) if pk else None, C.byref(k2) if pk else None, C.byref(k3) if pk else None,
               C.byref(k4) if pk else None),
            "pm_time_frames",
        )
        return {"total_ms": tot.value, "bin_ms": k1.value, "coarse_ms": k2.value, "fine_ms": k3.value, "clear_ms": k4.value, "iters": iters}

    def frame_latency(self, iters: int = 100) -> dict:
        """One frame at a time: first kernel's begin to last kernel's end (median / min, ms)."""
        med, mn = C.c_float(0), C.c_float(0)
        _lib.check(self._lib.pm_frame_latency(self._h, iters, C.byref(med), C.byref(mn)), "pm_frame_latency")
        return {"median_ms": med.value, "min_ms": mn.value, "iters": iters}

    def dense_kernel_frames(self) -> int:
        """Frames rendered with the one-wave-per-tile instantiation of the tile kernel (dense scenes)."""
        n = C.c_uint32(0)
        _lib.check(self._lib.pm_tile_kernel_info(self._h, C.byref(n)), "pm_tile_kernel_info")
        return int(n.value)

    def binning_info(self) -> dict:
        """Frames binned with a wave per strip row since pm_create (all / only because they ran behind other frames / of
        those, with a wave for every row of a plan that chains rows)."""
        out = (C.c_uint32 * 3)()
        _lib.check(self._lib.pm_binning_info(self._h, out), "pm_binning_info")
        return {"wave_per_row": int(out[0]), "inflight_only": int(out[1]), "no_chains": int(out[2])}

    def binning_plan_info(self) -> dict:
        """The binning plan in force: entries of the strip-row work list, strip rows cut in two, plans remade from the frames'
        own report since pm_create, and whether the plan in force is such a plan."""
        out = (C.c_uint32 * 4)()
        _lib.check(self._lib.pm_binning_plan_info(self._h, out), "pm_binning_plan_info")
        return {"entries": int(out[0]), "rows_cut": int(out[1]), "plans_fed_back": int(out[2]), "fed_back": bool(out[3])}

    def one_launch_info(self) -> dict:
        """Frames rendered as one launch so far, and whether a lone frame of the resident scene would be."""
        n = C.c_uint32(0)
        a = C.c_int(0)
        _lib.check(self._lib.pm_one_launch_info(self._h, C.byref(n), C.byref(a)), "pm_one_launch_info")
        return {"frames": int(n.value), "applies": bool(a.value)}

    def time_one_launch(self, iters: int = 100) -> float:
        """Average duration (ms) of pm_frame_kernel, frame alone (dispatch-attached events)."""
        ms = C.c_float(0)
        _lib.check(self._lib.pm_time_one_launch(self._h, iters, C.byref(ms)), "pm_time_one_launch")
        return float(ms.value)

    def fill_coverage(self, item_ix: int) -> np.ndarray:
        """f32-accumulated winding coverage of one Fill item over the viewport band (validation)."""
        out = np.zeros((self.band_pixel_rows, self.width), np.float32)
        _lib.check(self._lib.pm_fill_coverage(self._h, item_ix, out.ctypes.data, self.width), "pm_fill_coverage")
        return out

    # ---- point hit testing ------------------------------------------------------------
    def hit_test(self, points, skip_transparent: bool = False, counts: bool = False):
        """The last-painted item under every point: `points` is (n, 2) float32 {x, y} in scene coordinates (pixel (px, py) has its
        centre at (px + 0.5, py + 0.5)).  Returns top_item, uint32 [n] -- indices in flat paint order, PM_HIT_NONE (0xffffffff)
        where nothing is hit --, and with counts=True also how many items contain each point.  Needs a scene, no viewport."""
        xy = np.ascontiguousarray(points, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("hit_test needs an (n, 2) array of points")
        n = xy.shape[0]
        top = np.empty(n, np.uint32)
        cnt = np.empty(n, np.uint32) if counts else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_hit_test(self._h, xy.ctypes.data, n, flags, top.ctypes.data, cnt.ctypes.data if counts else None), "pm_hit_test")
        return (top, cnt) if counts else top

    def hit_test_tensor(self, xy, top_item, n_hit=None, stream=None, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: xy float32 [n, 2], top_item (and n_hit) int32 or uint32 [n], all
        contiguous.  `stream` as in render_to: None, or torch's legacy default stream (handle 0), means the context's OWN stream."""
        if not (xy.is_cuda and top_item.is_cuda) or str(xy.dtype) != "torch.float32" or xy.dim() != 2 or xy.shape[1] != 2 or not xy.is_contiguous():
            raise TypeError("hit_test_tensor needs a contiguous CUDA float32 tensor [n, 2]")
        n = xy.shape[0]
        for t in (top_item, n_hit):
            if t is not None and not (t.is_cuda and t.element_size() == 4 and t.numel() == n and t.is_contiguous()):
                raise TypeError("hit_test_tensor writes contiguous CUDA tensors of n 32-bit integers")
        s = stream.cuda_stream if stream is not None else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_hit_test_device(self._h, xy.data_ptr(), n, flags, top_item.data_ptr(), n_hit.data_ptr() if n_hit is not None else None, s),
                   "pm_hit_test_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def hit_frame(self, x0: int, y0: int, w: int, h: int, skip_transparent: bool = False, counts: bool = False):
        """The item map of the pixel rectangle [x0, x0 + w) x [y0, y0 + h): uint32 [h, w], what hit_test answers at every pixel's
        centre (x + 0.5, y + 0.5) -- and with counts=True also how many items contain it.  One workgroup per 16 x 16 tile
        instead of a wave per point.  Needs a scene, no viewport; the rectangle must end at or before pixel 65 535."""
        x0, y0, w, h = (operator.index(v) for v in (x0, y0, w, h))
        if min(x0, y0, w, h) < 0 or x0 + w > 65536 or y0 + h > 65536:
            raise ValueError("hit_frame needs a rectangle inside [0, 65536) x [0, 65536)")
        top = np.empty((h, w), np.uint32)
        cnt = np.empty((h, w), np.uint32) if counts else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_hit_frame(self._h, x0, y0, w, h, flags, top.ctypes.data, cnt.ctypes.data if counts else None, w), "pm_hit_frame")
        return (top, cnt) if counts else top

    def hit_frame_tensor(self, top_item, n_hit=None, x0: int = 0, y0: int = 0, stream=None, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: top_item (and n_hit, of the same shape) int32 or uint32 [h, w] with unit
        stride along a row and any row stride >= w -- a view into a larger tensor works, and what lies outside it is not written.
        `stream` as in hit_test_tensor."""
        for t in (top_item, n_hit):
            if t is not None and not (t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.dim() == 2):
                raise TypeError("hit_frame_tensor writes 2-D CUDA tensors of 32-bit integers")
        h, w = top_item.shape
        x0, y0 = operator.index(x0), operator.index(y0)
        if min(x0, y0) < 0 or x0 + w > 65536 or y0 + h > 65536:
            raise ValueError("hit_frame_tensor needs a rectangle inside [0, 65536) x [0, 65536)")
        stride = top_item.stride(0) if h > 1 else max(w, 1)
        for t in (top_item, n_hit):
            if t is None or w == 0 or h == 0:
                continue
            if tuple(t.shape) != (h, w) or t.stride(1) != 1 or (h > 1 and (t.stride(0) < w or t.stride(0) != stride)):
                raise ValueError("hit_frame_tensor: rows of unit stride, a row stride >= w, and the same shape and row stride for both tensors")
        s = stream.cuda_stream if stream is not None else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_hit_frame_device(self._h, x0, y0, w, h, flags, top_item.data_ptr(), n_hit.data_ptr() if n_hit is not None else None,
                                                 stride, s), "pm_hit_frame_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    # ---- rectangle queries (decision D19) ------------------------------------------------
    def hit_rects(self, rects, skip_transparent: bool = False, counts: bool = False):
        """The last-painted item every rectangle touches: `rects` is (n, 4) float32 {x0, y0, x1, y1}, closed, in scene coordinates.
        An item is touched if its shape -- edges included, strokes with their width -- has a point in common with the rectangle.
        Returns top_item, uint32 [n] (PM_HIT_NONE where nothing is touched), and with counts=True also how many items each
        rectangle touches.  A rectangle with a non-finite value or with x1 < x0 or y1 < y0 touches nothing.  Needs a scene, no
        viewport."""
        rc = np.ascontiguousarray(rects, dtype=np.float32)
        if rc.ndim != 2 or rc.shape[1] != 4:
            raise ValueError("hit_rects needs an (n, 4) array of rectangles")
        n = rc.shape[0]
        top = np.empty(n, np.uint32)
        cnt = np.empty(n, np.uint32) if counts else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_hit_rects(self._h, rc.ctypes.data, n, flags, top.ctypes.data, cnt.ctypes.data if counts else None), "pm_hit_rects")
        return (top, cnt) if counts else top

    def hit_rects_tensor(self, rects, top_item, n_hit=None, stream=None, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: rects float32 [n, 4], top_item (and n_hit) int32 or uint32 [n], all
        contiguous.  `stream` as in hit_test_tensor."""
        if not (rects.is_cuda and top_item.is_cuda) or str(rects.dtype) != "torch.float32" or rects.dim() != 2 or rects.shape[1] != 4 or not rects.is_contiguous():
            raise TypeError("hit_rects_tensor needs a contiguous CUDA float32 tensor [n, 4]")
        n = rects.shape[0]
        for t in (top_item, n_hit):
            if t is not None and not (t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.numel() == n and t.is_contiguous()):
                raise TypeError("hit_rects_tensor writes contiguous CUDA tensors of n 32-bit integers")
        s = stream.cuda_stream if stream is not None else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_hit_rects_device(self._h, rects.data_ptr(), n, flags, top_item.data_ptr(), n_hit.data_ptr() if n_hit is not None else None, s),
                   "pm_hit_rects_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    @staticmethod
    def _pick_rects(points, tolerance) -> np.ndarray:
        """(n, 4) float32: the square of half side `tolerance` around every point -- {f32(x) - f32(t), f32(y) - f32(t), f32(x) + f32(t),
        f32(y) + f32(t)}, each value rounded to f32."""
        xy = np.ascontiguousarray(points, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("pick needs an (n, 2) array of points")
        t = np.float32(tolerance)
        return np.concatenate([xy - t, xy + t], axis=1).astype(np.float32)

    def pick(self, points, tolerance, skip_transparent: bool = False, counts: bool = False):
        """hit_test with a tolerance: the last-painted item that comes within the square of half side `tolerance` around each
        point (hit_rects on those squares, each value rounded to f32).  A hairline stroke can be clicked this way."""
        return self.hit_rects(self._pick_rects(points, tolerance), skip_transparent=skip_transparent, counts=counts)

    # ---- hit stacks (decision D24) -----------------------------------------------------------
    @staticmethod
    def _stack_flags(skip_transparent, stop_at_opaque) -> int:
        return (_lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0) | (_lib.PM_HIT_STOP_AT_OPAQUE if stop_at_opaque else 0)

    def _stack(self, call, name, q, k, skip_transparent, stop_at_opaque, counts):
        k = operator.index(k)
        if not 1 <= k <= _lib.PM_HIT_STACK_MAX:
            raise ValueError(f"{name} needs 1 <= k <= {_lib.PM_HIT_STACK_MAX}")
        n = q.shape[0]
        items = np.empty((n, k), np.uint32)
        cnt = np.empty(n, np.uint32) if counts else None
        flags = self._stack_flags(skip_transparent, stop_at_opaque)
        _lib.check(call(self._h, q.ctypes.data, n, k, flags, items.ctypes.data, cnt.ctypes.data if counts else None), name)
        return (items, cnt) if counts else items

    def _stack_tensor(self, call, name, q, width, items, n_hit, stream, skip_transparent, stop_at_opaque) -> None:
        if not (q.is_cuda and items.is_cuda) or str(q.dtype) != "torch.float32" or q.dim() != 2 or q.shape[1] != width or not q.is_contiguous():
            raise TypeError(f"{name} needs a contiguous CUDA float32 tensor [n, {width}]")
        n = q.shape[0]
        if not (items.element_size() == 4 and not items.is_floating_point() and items.dim() == 2 and items.shape[0] == n and items.is_contiguous()):
            raise TypeError(f"{name} writes a contiguous CUDA tensor [n, k] of 32-bit integers")
        k = items.shape[1]
        if not 1 <= k <= _lib.PM_HIT_STACK_MAX:
            raise ValueError(f"{name} needs 1 <= k <= {_lib.PM_HIT_STACK_MAX}")
        if n_hit is not None and not (n_hit.is_cuda and n_hit.element_size() == 4 and not n_hit.is_floating_point() and n_hit.numel() == n and n_hit.is_contiguous()):
            raise TypeError(f"{name} writes the counts to a contiguous CUDA tensor of n 32-bit integers")
        s = stream.cuda_stream if stream is not None else None
        flags = self._stack_flags(skip_transparent, stop_at_opaque)
        _lib.check(call(self._h, q.data_ptr(), n, k, flags, items.data_ptr(), n_hit.data_ptr() if n_hit is not None else None, s), name)
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def hit_stack(self, points, k: int, skip_transparent: bool = False, stop_at_opaque: bool = False, counts: bool = False):
        """The k topmost items under every point, topmost first: uint32 [n, k], PM_HIT_NONE behind the last one -- select-behind, the
        list of objects under a cursor.  `points` as in hit_test, 1 <= k <= PM_HIT_STACK_MAX (256).  stop_at_opaque: the list ends
        at its first opaque item (a circle, or a colour of alpha 255), which is included: the chain of items between the eye and
        the first opaque one.  With counts=True also the full length of each list, uint32 [n], not clipped by k."""
        xy = np.ascontiguousarray(points, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("hit_stack needs an (n, 2) array of points")
        return self._stack(self._lib.pm_hit_stack, "pm_hit_stack", xy, k, skip_transparent, stop_at_opaque, counts)

    def hit_stack_tensor(self, xy, items, n_hit=None, stream=None, skip_transparent: bool = False, stop_at_opaque: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: xy float32 [n, 2], items int32 or uint32 [n, k] (k = items.shape[1]), n_hit
        [n], all contiguous.  `stream` as in hit_test_tensor."""
        self._stack_tensor(self._lib.pm_hit_stack_device, "pm_hit_stack_device", xy, 2, items, n_hit, stream, skip_transparent, stop_at_opaque)

    def hit_rects_stack(self, rects, k: int, skip_transparent: bool = False, stop_at_opaque: bool = False, counts: bool = False):
        """The k topmost items every rectangle touches, topmost first: hit_stack for the rectangles of hit_rects."""
        rc = np.ascontiguousarray(rects, dtype=np.float32)
        if rc.ndim != 2 or rc.shape[1] != 4:
            raise ValueError("hit_rects_stack needs an (n, 4) array of rectangles")
        return self._stack(self._lib.pm_hit_rects_stack, "pm_hit_rects_stack", rc, k, skip_transparent, stop_at_opaque, counts)

    def hit_rects_stack_tensor(self, rects, items, n_hit=None, stream=None, skip_transparent: bool = False, stop_at_opaque: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: rects float32 [n, 4], items [n, k], n_hit [n].  `stream` as in hit_test_tensor."""
        self._stack_tensor(self._lib.pm_hit_rects_stack_device, "pm_hit_rects_stack_device", rects, 4, items, n_hit, stream, skip_transparent, stop_at_opaque)

    def pick_stack(self, points, tolerance, k: int, skip_transparent: bool = False, stop_at_opaque: bool = False, counts: bool = False):
        """hit_stack with a tolerance: the k topmost items that come within the square of half side `tolerance` around each point
        (hit_rects_stack on pick's squares)."""
        return self.hit_rects_stack(self._pick_rects(points, tolerance), k, skip_transparent=skip_transparent, stop_at_opaque=stop_at_opaque, counts=counts)

    # ---- coverage counts (decision D28) ----------------------------------------------------
    @staticmethod
    def _coverage_flags(skip_transparent, visible_only) -> int:
        return (_lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0) | (_lib.PM_COVERAGE_VISIBLE_ONLY if visible_only else 0)

    @staticmethod
    def _coverage_rect(name, x0, y0, w, h):
        x0, y0, w, h = (operator.index(v) for v in (x0, y0, w, h))
        if min(x0, y0, w, h) < 0 or x0 + w > 65536 or y0 + h > 65536 or w * h > 0xFFFFFFFF:
            raise ValueError(f"{name} needs a rectangle inside [0, 65536) x [0, 65536) of fewer than 2^32 pixels")
        return x0, y0, w, h

    def item_coverage(self, x0: int, y0: int, w: int, h: int, skip_transparent: bool = False, visible_only: bool = False) -> np.ndarray:
        """How much of every item can be seen in the pixel rectangle [x0, x0 + w) x [y0, y0 + h): a structured array
        (COVERAGE_DTYPE), one record per item in flat paint order -- `covered`, the pixels whose centre the item contains (what
        hit_frame counts); `visible`, those of them under no opaque item above it (a circle, or a colour of alpha 255: hit_stack's
        stop_at_opaque); `top`, those where it is the topmost item (the histogram of hit_frame's map); `first_visible`, the smallest
        j * w + i over the visible pixels (x0 + i, y0 + j), PM_HIT_NONE if there are none.  visible_only: `covered` is DEFINED to
        equal `visible`, and tiles that lie under opaque items are left early -- cheaper on deep scenes.  Needs a scene, no
        viewport."""
        x0, y0, w, h = self._coverage_rect("item_coverage", x0, y0, w, h)
        out = np.empty(self.stats()["n_items"], COVERAGE_DTYPE)
        _lib.check(self._lib.pm_item_coverage(self._h, x0, y0, w, h, self._coverage_flags(skip_transparent, visible_only), out.ctypes.data, len(out), None),
                   "pm_item_coverage")
        return out

    def item_coverage_tensor(self, out, x0: int = 0, y0: int = 0, w: int = 0, h: int = 0, stream=None, skip_transparent: bool = False,
                             visible_only: bool = False) -> None:
        """The same into a torch CUDA tensor, asynchronous: out int32 or uint32 [m, 4] with m >= n_items, contiguous, a row
        {covered, visible, top, first_visible} per item; rows beyond n_items are not written.  `stream` as in hit_test_tensor."""
        if not (out.is_cuda and out.element_size() == 4 and not out.is_floating_point() and out.dim() == 2 and out.shape[1] == 4 and out.is_contiguous()):
            raise TypeError("item_coverage_tensor writes a contiguous CUDA tensor [m, 4] of 32-bit integers")
        x0, y0, w, h = self._coverage_rect("item_coverage_tensor", x0, y0, w, h)
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_item_coverage_device(self._h, x0, y0, w, h, self._coverage_flags(skip_transparent, visible_only), out.data_ptr(), out.shape[0], s),
                   "pm_item_coverage_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def hidden_items(self, x0: int, y0: int, w: int, h: int, skip_transparent: bool = False) -> np.ndarray:
        """The indices of the items no pixel of the rectangle shows: outside it, or wholly under opaque items (item_coverage with
        visible_only, visible == 0)."""
        return np.flatnonzero(self.item_coverage(x0, y0, w, h, skip_transparent=skip_transparent, visible_only=True)["visible"] == 0)

    def select_rect(self, x0, y0, x1, y1, skip_transparent: bool = False):
        """Marquee selection: (touched, enclosed), bool arrays over the items in flat paint order -- every item the closed rectangle
        touches, occluded ones included, and every item that lies wholly inside it."""
        rect = np.array([x0, y0, x1, y1], np.float32)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        words = np.zeros(self.stats()["n_items"], np.uint32)
        _lib.check(self._lib.pm_select_rect(self._h, rect.ctypes.data, flags, words.ctypes.data, words.size, None, None, None), "pm_select_rect")
        return (words & _lib.PM_SEL_TOUCHES) != 0, (words & _lib.PM_SEL_ENCLOSES) != 0

    def select_rect_tensor(self, x0, y0, x1, y1, item_flags, stream=None, skip_transparent: bool = False) -> None:
        """The same into a torch CUDA tensor, asynchronous: item_flags int32 or uint32, contiguous, of at least n_items words --
        word i becomes PM_SEL_TOUCHES | PM_SEL_ENCLOSES of item i, words beyond n_items are not written."""
        t = item_flags
        if not (t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.dim() == 1 and t.is_contiguous()):
            raise TypeError("select_rect_tensor writes a contiguous 1-D CUDA tensor of 32-bit integers")
        rect = np.array([x0, y0, x1, y1], np.float32)
        s = stream.cuda_stream if stream is not None else None
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_select_rect_device(self._h, rect.ctypes.data, flags, t.data_ptr(), t.numel(), s), "pm_select_rect_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    @staticmethod
    def _polygon(vertices, skip_transparent, even_odd):
        xy = np.ascontiguousarray(vertices, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2 or not 3 <= len(xy) <= _lib.PM_POLYGON_MAX_VERTICES:
            raise ValueError(f"a query polygon is an (m, 2) array of 3 .. {_lib.PM_POLYGON_MAX_VERTICES} vertices")
        return xy, (_lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0) | (_lib.PM_SEL_EVEN_ODD if even_odd else 0)

    def select_polygon(self, vertices, skip_transparent: bool = False, even_odd: bool = False):
        """Lasso selection: (touched, enclosed), bool arrays over the items in flat paint order, for the polygon of the (m, 2)
        vertices, which closes itself.  Touched: the item's outline reaches the polygon's boundary, a point of it lies inside, or the
        polygon lies inside a Fill.  Enclosed: the outline does not reach the boundary and every point of it lies inside.  The
        inside is by the non-zero rule, with even_odd by the even-odd rule."""
        xy, flags = self._polygon(vertices, skip_transparent, even_odd)
        words = np.zeros(self.stats()["n_items"], np.uint32)
        _lib.check(self._lib.pm_select_polygon(self._h, xy.ctypes.data, len(xy), flags, words.ctypes.data, words.size, None, None, None), "pm_select_polygon")
        return (words & _lib.PM_SEL_TOUCHES) != 0, (words & _lib.PM_SEL_ENCLOSES) != 0

    def select_polygon_tensor(self, vertices, item_flags, stream=None, skip_transparent: bool = False, even_odd: bool = False) -> None:
        """The same into a torch CUDA tensor, asynchronous, as select_rect_tensor: the vertices (host) are read before the call
        returns."""
        t = item_flags
        if not (t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.dim() == 1 and t.is_contiguous()):
            raise TypeError("select_polygon_tensor writes a contiguous 1-D CUDA tensor of 32-bit integers")
        xy, flags = self._polygon(vertices, skip_transparent, even_odd)
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_select_polygon_device(self._h, xy.ctypes.data, len(xy), flags, t.data_ptr(), t.numel(), s), "pm_select_polygon_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    @staticmethod
    def rotated_rect_vertices(cx, cy, w, h, angle) -> np.ndarray:
        """The corners (-w/2, -h/2), (+w/2, -h/2), (+w/2, +h/2), (-w/2, +h/2) of a w x h rectangle, in this order, turned by `angle`
        (radians, from +x towards +y) about its centre (cx, cy): computed in binary64, each value rounded to f32 once."""
        ca, sa = np.cos(np.float64(angle)), np.sin(np.float64(angle))
        hx, hy = np.float64(w) * 0.5, np.float64(h) * 0.5
        local = np.array([[-hx, -hy], [hx, -hy], [hx, hy], [-hx, hy]], np.float64)
        out = np.stack([np.float64(cx) + (local[:, 0] * ca - local[:, 1] * sa), np.float64(cy) + (local[:, 0] * sa + local[:, 1] * ca)], axis=1)
        return out.astype(np.float32)

    def select_rotated_rect(self, cx, cy, w, h, angle, skip_transparent: bool = False):
        """A marquee dragged in a rotated view: select_polygon of rotated_rect_vertices(cx, cy, w, h, angle) -- the corners
        (-w/2, -h/2), (+w/2, -h/2), (+w/2, +h/2), (-w/2, +h/2) turned by `angle` radians about (cx, cy), in this order."""
        return self.select_polygon(self.rotated_rect_vertices(cx, cy, w, h, angle), skip_transparent=skip_transparent)

    # ---- snapping (decision D21) ----------------------------------------------------------
    @staticmethod
    def _snap_flags(vertices, edges, skip_transparent) -> int:
        if not (vertices or edges):
            raise ValueError("snap needs vertices, edges or both")
        return (_lib.PM_SNAP_VERTICES if vertices else 0) | (_lib.PM_SNAP_EDGES if edges else 0) | (_lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0)

    def snap(self, points, radius, vertices: bool = True, edges: bool = True, skip_transparent: bool = False, skip_items=None) -> np.ndarray:
        """The nearest piece of geometry within `radius` of every point: `points` is (n, 2) float32 in scene coordinates, `radius` a
        scalar or one value per point (each rounded to f32).  Returns a structured array (SNAP_DTYPE) of n records: `item` in flat
        paint order (PM_HIT_NONE where nothing is within the radius, every other field 0), `kind` 1 for a vertex -- `index` is the
        point's index in the item, `x, y` the point -- or 2 for an edge -- `index` is the segment's, `t` in [0, 1] the parameter
        along it, `x, y` the nearest point on it; `d2` is the squared distance.  A Circle or an ellipse offers its centre; a
        stroke's width plays no part.  Among equal distances the topmost item wins, then the smallest index; with both kinds
        asked for a vertex within the radius wins over every edge.  skip_items: one word (or bool) per item, non-zero takes the
        item out of the search."""
        xy = np.ascontiguousarray(points, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("snap needs an (n, 2) array of points")
        n = xy.shape[0]
        rad = np.asarray(radius, dtype=np.float32)
        if rad.ndim not in (0, 1) or (rad.ndim == 1 and rad.shape[0] != n):
            raise ValueError("snap needs one radius, or one per point")
        xyr = np.ascontiguousarray(np.concatenate([xy, np.broadcast_to(rad, (n,))[:, None]], axis=1), dtype=np.float32)
        flags = self._snap_flags(vertices, edges, skip_transparent)
        skip = None if skip_items is None else np.ascontiguousarray(np.asarray(skip_items) != 0, dtype=np.uint32)
        if skip is not None and skip.ndim != 1:
            raise ValueError("skip_items is one word per item")
        out = np.zeros(n, SNAP_DTYPE)
        _lib.check(self._lib.pm_snap(self._h, xyr.ctypes.data, n, flags, skip.ctypes.data if skip is not None else None, skip.size if skip is not None else 0,
                                     out.ctypes.data), "pm_snap")
        return out

    def snap_tensor(self, xyr, out, skip_items=None, stream=None, vertices: bool = True, edges: bool = True, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: xyr float32 [n, 3] {x, y, r}, out int32 [n, 8] (the 32-byte records:
        out.cpu().numpy().view(SNAP_DTYPE)), skip_items None or a tensor of at least n_items 32-bit integers -- what
        select_rect_tensor / select_polygon_tensor wrote can be handed in as it is --, all contiguous.  `stream` as in
        hit_test_tensor."""
        if not (xyr.is_cuda and out.is_cuda) or str(xyr.dtype) != "torch.float32" or xyr.dim() != 2 or xyr.shape[1] != 3 or not xyr.is_contiguous():
            raise TypeError("snap_tensor needs a contiguous CUDA float32 tensor [n, 3]")
        n = xyr.shape[0]
        if str(out.dtype) != "torch.int32" or tuple(out.shape) != (n, 8) or not out.is_contiguous():
            raise TypeError("snap_tensor writes a contiguous CUDA int32 tensor [n, 8]")
        t = skip_items
        if t is not None and not (t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.dim() == 1 and t.is_contiguous()):
            raise TypeError("snap_tensor reads skip_items from a contiguous 1-D CUDA tensor of 32-bit integers")
        flags = self._snap_flags(vertices, edges, skip_transparent)
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_snap_device(self._h, xyr.data_ptr(), n, flags, t.data_ptr() if t is not None else None, t.numel() if t is not None else 0,
                                            out.data_ptr(), s), "pm_snap_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    # ---- snapping to intersections (decision D23) -------------------------------------------
    def snap_intersections(self, points, radius, skip_transparent: bool = False, skip_items=None) -> np.ndarray:
        """The nearest crossing of two edges within `radius` of every point; `points`, `radius` and `skip_items` as in snap.
        Returns a structured array (SNAP_CROSS_DTYPE) of n records: `kind` 3, `item` / `index` / `t` the first edge (the one of the
        topmost item, then of the smaller index) and the parameter of the crossing along it, `item2` / `index2` / `u` the second,
        `x, y` the point, `d2` its squared distance, `n_near` the number of edges within the radius.  `item` is PM_HIT_NONE where no
        two edges cross within the radius, and `kind` 4 where more than PM_SNAP_MAX_NEAR_EDGES (512) edges are within it: ask
        again with a smaller radius.  Edges that share an end point are no pair (where they meet is a vertex: snap)."""
        xy = np.ascontiguousarray(points, dtype=np.float32)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("snap_intersections needs an (n, 2) array of points")
        n = xy.shape[0]
        rad = np.asarray(radius, dtype=np.float32)
        if rad.ndim not in (0, 1) or (rad.ndim == 1 and rad.shape[0] != n):
            raise ValueError("snap_intersections needs one radius, or one per point")
        xyr = np.ascontiguousarray(np.concatenate([xy, np.broadcast_to(rad, (n,))[:, None]], axis=1), dtype=np.float32)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        skip = None if skip_items is None else np.ascontiguousarray(np.asarray(skip_items) != 0, dtype=np.uint32)
        if skip is not None and skip.ndim != 1:
            raise ValueError("skip_items is one word per item")
        out = np.zeros(n, SNAP_CROSS_DTYPE)
        _lib.check(self._lib.pm_snap_intersections(self._h, xyr.ctypes.data, n, flags, skip.ctypes.data if skip is not None else None,
                                                   skip.size if skip is not None else 0, out.ctypes.data), "pm_snap_intersections")
        return out

    def snap_intersections_tensor(self, xyr, out, skip_items=None, stream=None, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: xyr float32 [n, 3] {x, y, r}, out int32 [n, 12] (the 48-byte records:
        out.cpu().numpy().view(SNAP_CROSS_DTYPE)), skip_items and `stream` as in snap_tensor."""
        if not (xyr.is_cuda and out.is_cuda) or str(xyr.dtype) != "torch.float32" or xyr.dim() != 2 or xyr.shape[1] != 3 or not xyr.is_contiguous():
            raise TypeError("snap_intersections_tensor needs a contiguous CUDA float32 tensor [n, 3]")
        n = xyr.shape[0]
        if str(out.dtype) != "torch.int32" or tuple(out.shape) != (n, 12) or not out.is_contiguous():
            raise TypeError("snap_intersections_tensor writes a contiguous CUDA int32 tensor [n, 12]")
        t = skip_items
        if t is not None and not (t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.dim() == 1 and t.is_contiguous()):
            raise TypeError("snap_intersections_tensor reads skip_items from a contiguous 1-D CUDA tensor of 32-bit integers")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_snap_intersections_device(self._h, xyr.data_ptr(), n, flags, t.data_ptr() if t is not None else None,
                                                          t.numel() if t is not None else 0, out.data_ptr(), s), "pm_snap_intersections_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    # ---- bounds (decision D22) ------------------------------------------------------------
    @staticmethod
    def _is_words(t) -> bool:
        return t.is_cuda and t.element_size() == 4 and not t.is_floating_point() and t.dim() == 1 and t.is_contiguous()

    def item_bounds(self, skip_transparent: bool = False) -> np.ndarray:
        """The bounding box of every item in flat paint order: float64 (n_items, 4), {x0, y0, x1, y1} -- the geometry that is drawn,
        hit and selected (flattened curves, outlined and dashed strokes, a stroke's half width, a circle's radius), not the path
        elements.  An item without geometry, and with skip_transparent an item of alpha 0, has the empty box
        {+inf, +inf, -inf, -inf}."""
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        out = np.empty((self.stats()["n_items"], 4), np.float64)
        _lib.check(self._lib.pm_item_bounds(self._h, flags, out.ctypes.data, len(out), None), "pm_item_bounds")
        return out

    def item_bounds_tensor(self, out, stream=None, skip_transparent: bool = False) -> None:
        """The same into a torch CUDA tensor, asynchronous: out float64 [m, 4] with m >= n_items, contiguous; rows beyond n_items are
        not written.  `stream` as in hit_test_tensor."""
        if not (out.is_cuda and str(out.dtype) == "torch.float64" and out.dim() == 2 and out.shape[1] == 4 and out.is_contiguous()):
            raise TypeError("item_bounds_tensor writes a contiguous CUDA float64 tensor [m, 4]")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_item_bounds_device(self._h, flags, out.data_ptr(), out.shape[0], s), "pm_item_bounds_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def union_bounds(self, labels, n_labels: int, item_flags=None, mask: int = _lib.PM_SEL_TOUCHES | _lib.PM_SEL_ENCLOSES,
                     skip_transparent: bool = False) -> np.ndarray:
        """The union of the item boxes per label: a structured array (LABEL_BOUNDS_DTYPE) of n_labels records {box, n_items,
        n_boxed} -- the union of the boxes of the items that take part with that label, how many they are, and how many of them
        have a box (x0 <= x1 and y0 <= y1).  labels: one uint32 per item, or None for label 0 everywhere; an item whose label is
        >= n_labels takes no part.  item_flags: None, or one word per item (what select_rect / select_polygon report as PM_SEL_*
        words, or any bool array): the item takes part iff word & mask is non-zero.  A label nobody carries has the empty box."""
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
        words = None if item_flags is None else np.ascontiguousarray(item_flags).astype(np.uint32)
        for v, what in ((lab, "labels"), (words, "item_flags")):
            if v is not None and v.ndim != 1:
                raise ValueError(f"{what} is one word per item")
        if int(n_labels) < 1:
            raise ValueError("union_bounds needs n_labels >= 1")
        out = np.zeros(int(n_labels), LABEL_BOUNDS_DTYPE)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_union_bounds(self._h, flags, words.ctypes.data if words is not None else None, words.size if words is not None else 0,
                                             int(mask) if words is not None else 0, lab.ctypes.data if lab is not None else None,
                                             lab.size if lab is not None else 0, int(n_labels), out.ctypes.data), "pm_union_bounds")
        return out

    def union_bounds_tensor(self, out, labels=None, item_flags=None, mask: int = _lib.PM_SEL_TOUCHES | _lib.PM_SEL_ENCLOSES, stream=None,
                            skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: out int32 [n_labels, 10] (the 40-byte records:
        out.cpu().numpy().view(LABEL_BOUNDS_DTYPE)), labels and item_flags None or contiguous 1-D tensors of at least n_items 32-bit
        integers -- what select_rect_tensor / select_polygon_tensor wrote goes in as item_flags as it is.  `stream` as in
        hit_test_tensor."""
        if not (out.is_cuda and str(out.dtype) == "torch.int32" and out.dim() == 2 and out.shape[1] == 10 and out.shape[0] >= 1 and out.is_contiguous()):
            raise TypeError("union_bounds_tensor writes a contiguous CUDA int32 tensor [n_labels, 10]")
        for t, what in ((labels, "labels"), (item_flags, "item_flags")):
            if t is not None and not self._is_words(t):
                raise TypeError(f"union_bounds_tensor reads {what} from a contiguous 1-D CUDA tensor of 32-bit integers")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        w, lab = item_flags, labels
        _lib.check(self._lib.pm_union_bounds_device(self._h, flags, w.data_ptr() if w is not None else None, w.numel() if w is not None else 0,
                                                    int(mask) if w is not None else 0, lab.data_ptr() if lab is not None else None,
                                                    lab.numel() if lab is not None else 0, out.shape[0], out.data_ptr(), s), "pm_union_bounds_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def selection_bounds(self, item_flags=None, mask: int = _lib.PM_SEL_TOUCHES | _lib.PM_SEL_ENCLOSES, skip_transparent: bool = False):
        """(box, n_items, n_boxed) of a selection: box float64 (4,), the union of the boxes of the items whose word in item_flags has
        a bit of mask set (None: of every item -- the scene's box, "zoom to fit"), how many items that is, how many have a box."""
        rec = self.union_bounds(None, 1, item_flags, mask, skip_transparent)[0]
        return rec["box"].copy(), int(rec["n_items"]), int(rec["n_boxed"])

    def group_bounds(self, item_flags=None, mask: int = _lib.PM_SEL_TOUCHES | _lib.PM_SEL_ENCLOSES, skip_transparent: bool = False) -> np.ndarray:
        """union_bounds with every item labelled by the group of the path it came from (item_paths composed with the map given in
        set_path_groups; without a map every path is in group 0): one record per group -- where each group is after
        reflatten_groups, and, with item_flags, which groups a selection reaches (n_items != 0).  Needs a scene made by
        flatten_and_encode / reflatten, as item_paths does."""
        of_item = self.item_paths()
        groups = self._path_groups
        if groups is None:
            return self.union_bounds(None, 1, item_flags, mask, skip_transparent)
        return self.union_bounds(groups[of_item], int(groups.max()) + 1 if len(groups) else 1, item_flags, mask, skip_transparent)

    # ---- path measurement (decision D25) ---------------------------------------------------
    def item_lengths(self, skip_transparent: bool = False) -> np.ndarray:
        """How long every item is, in flat paint order: a structured array (ITEM_LENGTH_DTYPE) of n_items records -- `length` in units
        of 2^-16 px (divide by LENGTH_UNIT for pixels), `n_segments`, and `kind` 1 for an open walk (Line, Polyline), 2 for a closed
        one (Fill: closing segments count), 0 for an item that has none (a Circle, an ellipse, a Fill of no points, and with
        skip_transparent an item of alpha 0).  It is the geometry that is drawn: flattened curves under their groups' affines, a
        styled or dashed stroke's outline."""
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        out = np.zeros(self.stats()["n_items"], ITEM_LENGTH_DTYPE)
        _lib.check(self._lib.pm_item_lengths(self._h, flags, out.ctypes.data, len(out), None), "pm_item_lengths")
        return out

    def item_lengths_tensor(self, out, stream=None, skip_transparent: bool = False) -> None:
        """The same into a torch CUDA tensor, asynchronous: out int32 [m, 4] with m >= n_items, contiguous (the 16-byte records:
        out.cpu().numpy().view(ITEM_LENGTH_DTYPE)); rows beyond n_items are not written.  `stream` as in hit_test_tensor."""
        if not (out.is_cuda and str(out.dtype) == "torch.int32" and out.dim() == 2 and out.shape[1] == 4 and out.is_contiguous()):
            raise TypeError("item_lengths_tensor writes a contiguous CUDA int32 tensor [m, 4]")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_item_lengths_device(self._h, flags, out.data_ptr(), out.shape[0], s), "pm_item_lengths_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def points_at_units(self, items, positions, skip_transparent: bool = False) -> np.ndarray:
        """points_at_length with the positions given as integers in units of 2^-16 px (any value below 2^64)."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        if it.ndim != 1:
            raise ValueError("items is a 1-D array of item indices")
        q = np.zeros(len(it), LENGTH_QUERY_DTYPE)
        q["item"] = it
        pos = np.asarray(positions, dtype=np.uint64) if not isinstance(positions, (list, tuple)) else np.array([int(p) for p in positions], dtype=np.uint64)
        if pos.ndim not in (0, 1) or (pos.ndim == 1 and len(pos) != len(it)):
            raise ValueError("one position, or one per item")
        q["s"] = pos
        out = np.zeros(len(q), LENGTH_POINT_DTYPE)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_points_at_length(self._h, q.ctypes.data, len(q), flags, out.ctypes.data), "pm_points_at_length")
        return out

    def points_at_length(self, items, distances_px, skip_transparent: bool = False) -> np.ndarray:
        """The point at a distance along an item, for every pair (items[k], distances_px[k]): a structured array
        (LENGTH_POINT_DTYPE) -- `x, y` the point, `tx, ty` the unit direction of the path there, `index` the segment it lies on (what
        snap calls an edge's index) and `t` the parameter along that segment; `status` has bit 1 (found), bit 2 if the distance
        was beyond the item's end and the answer is the end, bit 4 if the item has a point and no length (direction (0, 0)).  `item` is
        PM_HIT_NONE for an item without a walk.  A distance is rounded to units of 2^-16 px (length_units); a negative one or a NaN
        is 0."""
        d = np.asarray(distances_px, dtype=np.float64)
        n = len(np.atleast_1d(np.asarray(items)))
        if d.ndim not in (0, 1) or (d.ndim == 1 and len(d) != n):
            raise ValueError("one distance, or one per item")
        units = [length_units(v) for v in np.broadcast_to(d, (n,))]
        return self.points_at_units(items, units, skip_transparent)

    def points_at_fraction(self, items, fractions, skip_transparent: bool = False) -> np.ndarray:
        """points_at_length at the fraction f of every item's own length: position floor(f * T + 0.5) in Python integers, T from
        item_lengths; f is clamped to [0, 1] (a NaN is 0)."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        if it.ndim != 1:
            raise ValueError("items is a 1-D array of item indices")
        f = np.asarray(fractions, dtype=np.float64)
        if f.ndim not in (0, 1) or (f.ndim == 1 and len(f) != len(it)):
            raise ValueError("one fraction, or one per item")
        total = self.item_lengths(skip_transparent)["length"]
        units = []
        for i, v in zip(it.tolist(), np.broadcast_to(f, (len(it),)).tolist()):
            T = int(total[i]) if i < len(total) else 0
            num, den = Fraction(min(max(v, 0.0), 1.0) if v == v else 0.0).as_integer_ratio()
            units.append((2 * num * T + den) // (2 * den))   # floor(f T + 1/2), exactly
        return self.points_at_units(it, units, skip_transparent)

    def points_at_length_tensor(self, queries, out, stream=None, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: queries int32 [n, 4] (the 16-byte LENGTH_QUERY_DTYPE records {item, 0, s low,
        s high}), out int32 [n, 8] (out.cpu().numpy().view(LENGTH_POINT_DTYPE)), both contiguous.  `stream` as in hit_test_tensor."""
        if not (queries.is_cuda and out.is_cuda) or str(queries.dtype) != "torch.int32" or queries.dim() != 2 or queries.shape[1] != 4 or not queries.is_contiguous():
            raise TypeError("points_at_length_tensor needs a contiguous CUDA int32 tensor [n, 4]")
        n = queries.shape[0]
        if str(out.dtype) != "torch.int32" or tuple(out.shape) != (n, 8) or not out.is_contiguous():
            raise TypeError("points_at_length_tensor writes a contiguous CUDA int32 tensor [n, 8]")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_points_at_length_device(self._h, queries.data_ptr(), n, flags, out.data_ptr(), s), "pm_points_at_length_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def positions_on_edges(self, items, indices, ts, skip_transparent: bool = False) -> np.ndarray:
        """How far along its item a point of an edge is -- the inverse of points_at_length, for what snap reports as (item, index, t):
        a structured array (LENGTH_AT_DTYPE) with `s` in units of 2^-16 px and `status` 1; `item` is PM_HIT_NONE (and s 0) where
        `index` names no segment of the item or t is outside [0, 1]."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        if it.ndim != 1:
            raise ValueError("items is a 1-D array of item indices")
        q = np.zeros(len(it), EDGE_QUERY_DTYPE)
        q["item"] = it
        q["index"] = np.asarray(indices, dtype=np.uint32)
        q["t"] = np.asarray(ts, dtype=np.float32)
        out = np.zeros(len(q), LENGTH_AT_DTYPE)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_positions_on_edges(self._h, q.ctypes.data, len(q), flags, out.ctypes.data), "pm_positions_on_edges")
        return out

    def positions_on_edges_tensor(self, queries, out, stream=None, skip_transparent: bool = False) -> None:
        """The same on torch CUDA tensors, asynchronous: queries int32 [n, 4] (the 16-byte EDGE_QUERY_DTYPE records {item, index, t's
        bits, 0} -- columns 0, 2 and 3 of what snap_tensor wrote and a column of zeros), out int32 [n, 4]
        (out.cpu().numpy().view(LENGTH_AT_DTYPE)), both contiguous.  `stream` as in hit_test_tensor."""
        if not (queries.is_cuda and out.is_cuda) or str(queries.dtype) != "torch.int32" or queries.dim() != 2 or queries.shape[1] != 4 or not queries.is_contiguous():
            raise TypeError("positions_on_edges_tensor needs a contiguous CUDA int32 tensor [n, 4]")
        n = queries.shape[0]
        if str(out.dtype) != "torch.int32" or tuple(out.shape) != (n, 4) or not out.is_contiguous():
            raise TypeError("positions_on_edges_tensor writes a contiguous CUDA int32 tensor [n, 4]")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_positions_on_edges_device(self._h, queries.data_ptr(), n, flags, out.data_ptr(), s), "pm_positions_on_edges_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    # ---- resampling (decision D26) -----------------------------------------------------------
    def _resample(self, q: np.ndarray, skip_transparent: bool):
        """Packed requests through pm_resample_items: (records LENGTH_POINT_DTYPE [total], offsets int64 [n + 1], infos RESAMPLE_INFO_DTYPE [n])."""
        offsets = np.zeros(len(q) + 1, np.int64)
        np.cumsum(q["count"], out=offsets[1:])
        if offsets[-1] > _lib.PM_RESAMPLE_MAX_COUNT:
            raise ValueError(f"a resampling call answers at most {_lib.PM_RESAMPLE_MAX_COUNT} samples")
        q["first"] = offsets[:-1]
        out = np.zeros(int(offsets[-1]), LENGTH_POINT_DTYPE)
        info = np.zeros(len(q), RESAMPLE_INFO_DTYPE)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        # (an empty numpy array still has an address: out is never NULL)
        _lib.check(self._lib.pm_resample_items(self._h, q.ctypes.data, len(q), flags, out.ctypes.data, len(out), info.ctypes.data), "pm_resample_items")
        return out, offsets, info

    @staticmethod
    def _resample_requests(items, counts, mode) -> np.ndarray:
        it = np.ascontiguousarray(items, dtype=np.uint32)
        if it.ndim != 1:
            raise ValueError("items is a 1-D array of item indices")
        cn = np.asarray(counts, dtype=np.int64)
        if cn.ndim not in (0, 1) or (cn.ndim == 1 and len(cn) != len(it)):
            raise ValueError("one count, or one per item")
        cn = np.broadcast_to(cn, (len(it),))
        if len(cn) and (cn.min() < 0 or cn.max() > _lib.PM_RESAMPLE_MAX_COUNT):
            raise ValueError(f"0 <= count <= {_lib.PM_RESAMPLE_MAX_COUNT}")
        q = np.zeros(len(it), RESAMPLE_QUERY_DTYPE)
        q["item"] = it
        q["mode"] = mode
        q["count"] = cn
        return q

    def resample(self, items, counts, skip_transparent: bool = False):
        """counts[k] evenly spaced points along items[k], in one call and one walk of each item: an open item (Line, Polyline) from its
        start to its end, both included; a closed one (Fill) from its start, the start not repeated.  Returns (points, offsets,
        infos): the packed LENGTH_POINT_DTYPE records -- request k's are points[offsets[k]:offsets[k + 1]], each what
        points_at_units answers at its position --, and per request a RESAMPLE_INFO_DTYPE record {length, n_unclamped, kind}.  The
        positions are made on the device from the item's own length: s_j = j (T div m) + min(j, T mod m), gaps within one unit of
        2^-16 px of each other."""
        return self._resample(self._resample_requests(items, counts, _lib.PM_RESAMPLE_EVEN), skip_transparent)

    def resample_step(self, items, step_px, start_px=0.0, counts=None, skip_transparent: bool = False):
        """A point every step_px along items[k], the first at start_px (one value each, or one per item; rounded to units of 2^-16 px
        as points_at_length does).  counts=None: as many as fit -- item_lengths() is called once and item k gets
        floor((T - start) / step) + 1 samples, 0 where start > T, PM_RESAMPLE_MAX_COUNT at the most (a step that rounds to 0 is
        refused).  With counts given nothing is read back first: positions beyond the end answer with the end and the
        clamped bit, and infos["n_unclamped"] says how many fitted.  Returns what resample returns."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        n = len(it) if it.ndim == 1 else 0
        sp, st = np.asarray(step_px, dtype=np.float64), np.asarray(start_px, dtype=np.float64)
        for v in (sp, st):
            if v.ndim not in (0, 1) or (v.ndim == 1 and len(v) != n):
                raise ValueError("one step and one start, or one per item")
        steps = [length_units(v) for v in np.broadcast_to(sp, (n,))]
        starts = [length_units(v) for v in np.broadcast_to(st, (n,))]
        if counts is None:
            total = self.item_lengths(skip_transparent)["length"]
            counts = []
            for i, step, start in zip(it.tolist(), steps, starts):
                T = int(total[i]) if i < len(total) else 0
                if step == 0:
                    raise ValueError("a step that rounds to 0 fits any number of samples: give counts")
                counts.append(0 if start > T else min((T - start) // step + 1, _lib.PM_RESAMPLE_MAX_COUNT))
        q = self._resample_requests(it, counts, _lib.PM_RESAMPLE_STEP)
        q["start"] = np.array(starts, dtype=np.uint64)
        q["step"] = np.array(steps, dtype=np.uint64)
        return self._resample(q, skip_transparent)

    def resample_tensor(self, requests, out, info, stream=None, skip_transparent: bool = False) -> None:
        """Resampling on torch CUDA tensors, asynchronous: requests int32 [n, 8] (the 32-byte RESAMPLE_QUERY_DTYPE records), out int32
        [cap, 8] (LENGTH_POINT_DTYPE records), info int32 [n, 4] (RESAMPLE_INFO_DTYPE), all contiguous.  A request's `first` is the
        caller's: sample j goes to out[first + j], and no row at or beyond cap is written.  An invalid request writes no point and
        gets the info kind PM_RESAMPLE_INVALID.  `stream` as in hit_test_tensor."""
        if not (requests.is_cuda and out.is_cuda and info.is_cuda) or str(requests.dtype) != "torch.int32" or requests.dim() != 2 or requests.shape[1] != 8 or \
                not requests.is_contiguous():
            raise TypeError("resample_tensor needs a contiguous CUDA int32 tensor [n, 8]")
        n = requests.shape[0]
        if str(out.dtype) != "torch.int32" or out.dim() != 2 or out.shape[1] != 8 or not out.is_contiguous():
            raise TypeError("resample_tensor writes a contiguous CUDA int32 tensor [cap, 8]")
        if str(info.dtype) != "torch.int32" or tuple(info.shape) != (n, 4) or not info.is_contiguous():
            raise TypeError("resample_tensor writes a contiguous CUDA int32 tensor [n, 4] of infos")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_resample_items_device(self._h, requests.data_ptr(), n, flags, out.data_ptr(), out.shape[0], info.data_ptr(), s),
                   "pm_resample_items_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    # ---- trimming (decision D27) -------------------------------------------------------------
    def _trim(self, q: np.ndarray, skip_transparent: bool):
        """Requests through pm_trim_items twice: the count pass (cap = 0), then exactly packed.  Returns (vertices TRIM_VERTEX_DTYPE
        [total], offsets int64 [n + 1], infos TRIM_INFO_DTYPE [n])."""
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        info = np.zeros(len(q), TRIM_INFO_DTYPE)
        q["first"] = 0
        q["cap"] = 0
        _lib.check(self._lib.pm_trim_items(self._h, q.ctypes.data, len(q), flags, None, 0, info.ctypes.data), "pm_trim_items")
        offsets = np.zeros(len(q) + 1, np.int64)
        np.cumsum(info["n_vertices"], out=offsets[1:])
        if offsets[-1] > 1 << 20:
            raise ValueError(f"a trimming call answers at most {1 << 20} vertices")
        q["first"] = offsets[:-1]
        q["cap"] = info["n_vertices"]
        out = np.zeros(int(offsets[-1]), TRIM_VERTEX_DTYPE)
        if len(out):
            _lib.check(self._lib.pm_trim_items(self._h, q.ctypes.data, len(q), flags, out.ctypes.data, len(out), info.ctypes.data), "pm_trim_items")
        return out, offsets, info

    def trim_units(self, items, s0, s1, skip_transparent: bool = False):
        """The pieces [min(s0[k], T), min(s1[k], T)] of items[k], positions in units of 2^-16 px as integers (one value each, or one
        per item; s0 <= s1; 2^64 - 1 is "to the end").  Returns (vertices, offsets, infos): the packed TRIM_VERTEX_DTYPE records --
        piece k's are vertices[offsets[k]:offsets[k + 1]], poly-line runs that trim_runs splits --, and per piece a TRIM_INFO_DTYPE
        record {length, n_vertices, n_runs, kind, flags}."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        if it.ndim != 1:
            raise ValueError("items is a 1-D array of item indices")
        ends = []
        for v in (s0, s1):
            a = np.asarray(v, dtype=object)
            if a.ndim not in (0, 1) or (a.ndim == 1 and len(a) != len(it)):
                raise ValueError("one position, or one per item")
            vals = [int(x) for x in np.broadcast_to(a, (len(it),)).tolist()]
            if any(not 0 <= x < 1 << 64 for x in vals):
                raise ValueError("0 <= position < 2^64")
            ends.append(vals)
        if any(a > b for a, b in zip(*ends)):
            raise ValueError("a piece's start is not beyond its end")
        q = np.zeros(len(it), TRIM_QUERY_DTYPE)
        q["item"] = it
        q["mode"] = _lib.PM_TRIM_RANGE
        q["s0"] = np.array(ends[0], dtype=np.uint64)
        q["s1"] = np.array(ends[1], dtype=np.uint64)
        return self._trim(q, skip_transparent)

    def trim(self, items, starts_px, ends_px, skip_transparent: bool = False):
        """trim_units with the positions in pixels (rounded to units of 2^-16 px as points_at_length does; an end of inf is "to the
        end"): the geometry of items[k] between the two lengths."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        n = len(it) if it.ndim == 1 else 0
        units = []
        for v in (starts_px, ends_px):
            a = np.asarray(v, dtype=np.float64)
            if a.ndim not in (0, 1) or (a.ndim == 1 and len(a) != n):
                raise ValueError("one position, or one per item")
            units.append([length_units(x) for x in np.broadcast_to(a, (n,))])
        return self.trim_units(it, units[0], units[1], skip_transparent)

    def trim_parts(self, items, parts, skip_transparent: bool = False):
        """Every item of `items` cut into parts[k] even pieces (one count, or one per item; 1 <= parts <= PM_TRIM_MAX_PARTS): the
        pieces of item k in order, then those of item k + 1, in what trim_units returns.  The pieces of an item tile [0, T] exactly,
        and their ends are resample()'s even positions."""
        it = np.ascontiguousarray(items, dtype=np.uint32)
        if it.ndim != 1:
            raise ValueError("items is a 1-D array of item indices")
        m = np.asarray(parts, dtype=np.int64)
        if m.ndim not in (0, 1) or (m.ndim == 1 and len(m) != len(it)):
            raise ValueError("one number of parts, or one per item")
        m = np.broadcast_to(m, (len(it),))
        if len(m) and (m.min() < 1 or m.max() > _lib.PM_TRIM_MAX_PARTS):
            raise ValueError(f"1 <= parts <= {_lib.PM_TRIM_MAX_PARTS}")
        q = np.zeros(int(m.sum()), TRIM_QUERY_DTYPE)
        q["item"] = np.repeat(it, m)
        q["mode"] = _lib.PM_TRIM_PART
        q["s0"] = np.concatenate([np.arange(k, dtype=np.uint64) for k in m.tolist()]) if len(q) else 0
        q["s1"] = np.repeat(m, m).astype(np.uint64)
        return self._trim(q, skip_transparent)

    def trim_tensor(self, requests, out, info, stream=None, skip_transparent: bool = False) -> None:
        """Trimming on torch CUDA tensors, asynchronous: requests int32 [n, 8] (the 32-byte TRIM_QUERY_DTYPE records), out int32
        [cap, 4] (TRIM_VERTEX_DTYPE records), info int32 [n, 6] (TRIM_INFO_DTYPE), all contiguous.  A request's `first` and `cap` are
        the caller's: vertex p goes to out[first + p] for p < cap, and no row at or beyond the tensor's end is written.  An invalid
        request writes no vertex and gets the info kind PM_TRIM_INVALID.  `stream` as in hit_test_tensor."""
        if not (requests.is_cuda and out.is_cuda and info.is_cuda) or str(requests.dtype) != "torch.int32" or requests.dim() != 2 or requests.shape[1] != 8 or \
                not requests.is_contiguous():
            raise TypeError("trim_tensor needs a contiguous CUDA int32 tensor [n, 8]")
        n = requests.shape[0]
        if str(out.dtype) != "torch.int32" or out.dim() != 2 or out.shape[1] != 4 or not out.is_contiguous():
            raise TypeError("trim_tensor writes a contiguous CUDA int32 tensor [cap, 4]")
        if str(info.dtype) != "torch.int32" or tuple(info.shape) != (n, 6) or not info.is_contiguous():
            raise TypeError("trim_tensor writes a contiguous CUDA int32 tensor [n, 6] of infos")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_trim_items_device(self._h, requests.data_ptr(), n, flags, out.data_ptr(), out.shape[0], info.data_ptr(), s), "pm_trim_items_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    # ---- item crossings (decision D29) -------------------------------------------------------
    def crossings(self, items_a, items_b, skip_transparent: bool = False):
        """Every point where an edge of items_a[k] crosses an edge of items_b[k] (one item each, or one per request; the same item
        twice asks for its self-crossings, each once).  Returns (records, offsets, infos): the packed CROSSING_DTYPE records --
        request k's are records[offsets[k]:offsets[k + 1]], in the order (index_a, index_b) --, and per request a
        CROSSINGS_INFO_DTYPE record {n_crossings, flags, n_a, n_b}.  A request of more than PM_CROSSINGS_MAX_PAIRS index pairs has
        the flag PM_CROSSINGS_TOO_MANY and no records: split the item with trim.  Two calls: the count pass, then exactly packed."""
        a, b = np.asarray(items_a, dtype=np.uint32), np.asarray(items_b, dtype=np.uint32)
        if a.ndim > 1 or b.ndim > 1 or (a.ndim == 1 and b.ndim == 1 and len(a) != len(b)):
            raise ValueError("one item, or one per request, on either side")
        n = len(a) if a.ndim == 1 else (len(b) if b.ndim == 1 else 1)
        q = np.zeros(n, CROSSINGS_QUERY_DTYPE)
        q["item_a"] = a
        q["item_b"] = b
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        info = np.zeros(n, CROSSINGS_INFO_DTYPE)
        _lib.check(self._lib.pm_item_crossings(self._h, q.ctypes.data, n, flags, None, 0, info.ctypes.data), "pm_item_crossings")
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(info["n_crossings"], out=offsets[1:])
        if offsets[-1] > 1 << 20:
            raise ValueError(f"a crossings call answers at most {1 << 20} records")
        q["first"] = offsets[:-1]
        q["cap"] = info["n_crossings"]
        out = np.zeros(int(offsets[-1]), CROSSING_DTYPE)
        if len(out):
            _lib.check(self._lib.pm_item_crossings(self._h, q.ctypes.data, n, flags, out.ctypes.data, len(out), info.ctypes.data), "pm_item_crossings")
        return out, offsets, info

    def self_crossings(self, items, skip_transparent: bool = False):
        """crossings(items, items): where every item of `items` crosses itself."""
        it = np.asarray(items, dtype=np.uint32)
        return self.crossings(it, it, skip_transparent)

    def crossings_tensor(self, requests, out, info, stream=None, skip_transparent: bool = False) -> None:
        """Crossings on torch CUDA tensors, asynchronous: requests int32 [n, 4] (the 16-byte CROSSINGS_QUERY_DTYPE records), out int32
        [cap, 12] (CROSSING_DTYPE records), info int32 [n, 4] (CROSSINGS_INFO_DTYPE), all contiguous.  A request's `first` and `cap`
        are the caller's: record p goes to out[first + p] for p < cap, and no row at or beyond the tensor's end is written.  `stream`
        as in hit_test_tensor."""
        if not (requests.is_cuda and out.is_cuda and info.is_cuda) or str(requests.dtype) != "torch.int32" or requests.dim() != 2 or requests.shape[1] != 4 or \
                not requests.is_contiguous():
            raise TypeError("crossings_tensor needs a contiguous CUDA int32 tensor [n, 4]")
        n = requests.shape[0]
        if str(out.dtype) != "torch.int32" or out.dim() != 2 or out.shape[1] != 12 or not out.is_contiguous():
            raise TypeError("crossings_tensor writes a contiguous CUDA int32 tensor [cap, 12]")
        if str(info.dtype) != "torch.int32" or tuple(info.shape) != (n, 4) or not info.is_contiguous():
            raise TypeError("crossings_tensor writes a contiguous CUDA int32 tensor [n, 4] of infos")
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        s = stream.cuda_stream if stream is not None else None
        _lib.check(self._lib.pm_item_crossings_device(self._h, requests.data_ptr(), n, flags, out.data_ptr(), out.shape[0], info.data_ptr(), s),
                   "pm_item_crossings_device")
        if stream is not None and not s:  # (torch's default stream: see render_to)
            _warn_default_stream()
            self.sync()

    def crossing_positions(self, records, skip_transparent: bool = False):
        """(s_a, s_b): how far along item A and along item B every crossing of `records` (CROSSING_DTYPE) lies, in units of 2^-16 px
        as uint64 arrays -- the record's two 16-byte halves through positions_on_edges, which answers PM_MEASURE_FOUND for every
        one.  On the device the same is `rec.view(-1, 3, 4)[:, :2].reshape(-1, 4)` of a crossings_tensor `out`, made contiguous,
        into positions_on_edges_tensor: rows 2 k and 2 k + 1 are crossing k's positions along A and along B."""
        rec = np.ascontiguousarray(records, dtype=CROSSING_DTYPE)
        if rec.ndim != 1:
            raise ValueError("records is a 1-D array of CROSSING_DTYPE")
        q = np.ascontiguousarray(rec.view(np.uint32).reshape(-1, 3, 4)[:, :2]).reshape(-1).view(EDGE_QUERY_DTYPE)
        out = np.zeros(len(q), LENGTH_AT_DTYPE)
        flags = _lib.PM_HIT_SKIP_TRANSPARENT if skip_transparent else 0
        _lib.check(self._lib.pm_positions_on_edges(self._h, q.ctypes.data, len(q), flags, out.ctypes.data), "pm_positions_on_edges")
        if len(out) and not np.all(out["status"] == _lib.PM_MEASURE_FOUND):
            raise ValueError("a record names no edge of the resident scene")
        return out["s"][0::2].copy(), out["s"][1::2].copy()

    def path_lengths(self, skip_transparent: bool = False):
        """(lengths, n_items) per path of the PathSet: the sum of item_lengths over the items each path produced (item_paths), in
        units of 2^-16 px as Python integers, and how many items that is.  Needs a scene made by flatten_and_encode / reflatten."""
        of_item = self.item_paths()
        rec = self.item_lengths(skip_transparent)
        n_paths = int(of_item.max()) + 1 if len(of_item) else 0
        lengths, counts = [0] * n_paths, [0] * n_paths
        for p, v in zip(of_item.tolist(), rec["length"].tolist()):
            lengths[p] += int(v)
            counts[p] += 1
        return lengths, counts

    def item_paths(self) -> np.ndarray:
        """For a scene made by flatten_and_encode / reflatten: the index of the path (into the PathSet) that produced each item."""
        n = C.c_uint32(0)
        st = self._lib.pm_item_paths(self._h, None, 0, C.byref(n))
        if st not in (_lib.PM_OK, _lib.PM_ERR_CAPACITY):
            _lib.check(st, "pm_item_paths")
        out = np.empty(n.value, np.uint32)
        _lib.check(self._lib.pm_item_paths(self._h, out.ctypes.data, out.size, C.byref(n)), "pm_item_paths")
        return out

    def scene_timings(self) -> dict:
        """Host wall-clock cost of the last scene replacement (flatten+encode, index, arena)."""
        t = _lib.SceneTimings()
        _lib.check(self._lib.pm_get_scene_timings(self._h, C.byref(t)), "pm_get_scene_timings")
        out = {name: getattr(t, name) for name, _ in t._fields_}
        n = C.c_uint32(0)
        _lib.check(self._lib.pm_get_binning_plans(self._h, C.byref(n)), "pm_get_binning_plans")
        out["binning_plans"] = int(n.value)
        return out

    def frame_timeline(self, iters: int = 100) -> dict:
        """The lone frame taken apart (ms, medians): kernels and the gaps between them."""
        v = (C.c_float * 6)()
        _lib.check(self._lib.pm_debug_frame_timeline(self._h, iters, v), "pm_debug_frame_timeline")
        return dict(zip(("bin_ms", "gap1_ms", "coarse_ms", "gap2_ms", "fine_ms", "total_ms"), [float(x) for x in v]))

    def stats(self) -> dict:
        s = _lib.Stats()
        _lib.check(self._lib.pm_get_stats(self._h, C.byref(s)), "pm_get_stats")
        return {name: getattr(s, name) for name, _ in s._fields_}

    def capture_ptcl(self, max_cmds_per_tile: int = 512):
        """Per-tile command lists of the last frame in the reference's 24-byte layout.
        Returns (counts[rows, tiles_x], solid[rows, tiles_x], cmds[rows, tiles_x, max, 6])."""
        st = self.stats()
        rows, tx = st["band_row1"] - st["band_row0"], st["tiles_x"]
        counts = np.zeros((rows, tx), np.uint32)
        solid = np.zeros((rows, tx), np.uint32)
        cmds = np.zeros((rows, tx, max_cmds_per_tile, 6), np.uint32)
        _lib.check(
            self._lib.pm_debug_capture_ptcl(self._h, max_cmds_per_tile, counts.ctypes.data, solid.ctypes.data, cmds.ctypes.data),
            "pm_debug_capture_ptcl",
        )
        return counts, solid, cmds


class Comm:
    """pm_comm_* / pm_gather: the C-ABI form of the band gather (RCCL bound at run time).
    The 128-byte id comes from rank 0 (Comm.unique_id()) and reaches the other ranks through
    whatever the host has (here: any picklable channel)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _lib.check(_lib.load().pm_comm_unique_id(buf), "pm_comm_unique_id")
        return bytes(buf)

    def __init__(self, renderer: "Renderer", uid: bytes, rank: int, world: int):
        self._lib = _lib.load()
        self._r = renderer
        self.rank, self.world = rank, world
        err = C.c_int(0)
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._h = self._lib.pm_comm_create(renderer._h, buf, rank, world, C.byref(err))
        if not self._h:
            raise _lib.PietMetalError(err.value, "pm_comm_create")

    def gather(self, layout, root: int = 0, full=None, band=None, stream=None, renderer=None) -> None:
        """layout = [(tile_row0, tile_row1, ...)] per rank; full = torch uint8 [H, W, 4] on the root;
        band = this rank's band tensor (None: the renderer's last frame).  renderer: another context of the same
        device whose band the table names (a rank that renders its band in sub-bands, one context each, gathers every
        sub-band with the one communicator)."""
        rows = (C.c_uint32 * (2 * self.world))(*[v for b in layout for v in (b[0], b[1])])
        _lib.check(
            self._lib.pm_gather(
                (renderer or self._r)._h, self._h, band.data_ptr() if band is not None else None, band.stride(0) if band is not None else 0, rows, root,
                full.data_ptr() if full is not None else None, full.stride(0) if full is not None else 0,
                stream.cuda_stream if stream is not None else None,
            ),
            "pm_gather",
        )
        if stream is not None and not stream.cuda_stream:  # (torch's default stream: see Renderer.render_to)
            _warn_default_stream()
            (renderer or self._r).sync()

    @staticmethod
    def library_path() -> str:
        """The RCCL shared object the C ABI bound (loads it if it has not yet)."""
        buf = C.create_string_buffer(1024)
        _lib.check(_lib.load().pm_comm_info(None, buf, len(buf), None), "pm_comm_info")
        return buf.value.decode()

    def info(self) -> dict:
        """{"rccl_lib": path of the bound library, "rccl_ranks": ncclCommCount of this communicator}"""
        buf = C.create_string_buffer(1024)
        n = C.c_int(0)
        _lib.check(self._lib.pm_comm_info(self._h, buf, len(buf), C.byref(n)), "pm_comm_info")
        return {"rccl_lib": buf.value.decode(), "rccl_ranks": int(n.value)}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.pm_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _time_tiles(self, max_slots: int = 1 << 20) -> np.ndarray:
    """Developer profiling: per-slot timeline of pm_fine_kernel, rows =
    (start, end, tile | quarter << 31, wave << 32 | commands, phase A ticks, phase B ticks,
    list complete (fused kernel), own-item ticks, 4 x packed list-building stages)."""
    out = np.zeros((max_slots, 12), np.uint64)
    n = C.c_size_t(0)
    _lib.check(self._lib.pm_debug_time_tiles(self._h, out.ctypes.data, max_slots, C.byref(n)), "pm_debug_time_tiles")
    return out[: n.value]


Renderer.time_tiles = _time_tiles


def _time_bins(self, max_rows: int = 1 << 20) -> np.ndarray:
    out = np.zeros((max_rows, 16), np.uint64)
    n = C.c_size_t(0)
    _lib.check(self._lib.pm_debug_time_bins(self._h, out.ctypes.data, max_rows, C.byref(n)), "pm_debug_time_bins")
    return out[: n.value]


Renderer.time_bins = _time_bins


def init_test_scene(buf: np.ndarray) -> None:
    """The reference's one FFI symbol (include/piet_metal.h:3): Tiger at scale 8."""
    lib = _lib.load()
    lib.init_test_scene(buf.ctypes.data, buf.size)
