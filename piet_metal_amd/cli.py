"""Headless presentation for the renderer: SVG (or the embedded Tiger) -> PNG.

    python -m piet_metal_amd.cli tiger out.png --width 3840 --height 2160
    python -m piet_metal_amd.cli drawing.svg out.png --scale 4 --width 1024 --height 1024

    python -m piet_metal_amd.cli tiger spin.png --frames 60 --spin 360     (spin-000.png ... spin-059.png)
    python -m piet_metal_amd.cli drawing.svg apart.png --frames 30 --explode 1.5    (the top-level groups move apart)
    python -m piet_metal_amd.cli drawing.svg gone.png --frames 30 --fade            (the top-level groups fade out one after another)
    python -m piet_metal_amd.cli tiger out.png --pick 800,800 --pick 3,3   (what is under these points?)
    python -m piet_metal_amd.cli tiger out.png --pick 800,800 --pick-tolerance 3   (... or within 3 pixels of them?)
    python -m piet_metal_amd.cli tiger out.png --pick 800,800 --pick-depth 4       (... and what lies behind it: up to four items, topmost first)
    python -m piet_metal_amd.cli tiger out.png --select 700,700,900,900    (marquee: what does this rectangle touch, what does it enclose?)
    python -m piet_metal_amd.cli tiger out.png --snap 800,800 --snap-radius 12   (the nearest vertex, or else the nearest edge, within 12 pixels)
    python -m piet_metal_amd.cli tiger out.png --snap 800,800 --snap-radius 12 --snap-to intersections   (the nearest point where two edges cross)
    python -m piet_metal_amd.cli tiger out.png --bounds --select 700,700,900,900   (where is the picture, where the selection, and how many items)
    python -m piet_metal_amd.cli tiger out.png --lengths --point-at 40,37.5        (how long every path is; the point and the tangent 37.5 px along item 40)
    python -m piet_metal_amd.cli tiger out.png --resample 40,12 --resample-step 40,12.5   (twelve even points along item 40; a point every 12.5 px of it)
    python -m piet_metal_amd.cli tiger out.png --trim 40,10,25.5 --trim-parts 40,4   (item 40 between 10 and 25.5 px along it; item 40 in four even pieces)
    python -m piet_metal_amd.cli tiger out.png --crossings 40,41 --self-crossings 40   (where item 40 crosses item 41, and where it crosses itself)
    python -m piet_metal_amd.cli tiger out.png --fit                               (zoom to fit; with --select / --lasso: zoom to the selection)

Replaces the reference's MTKView shell (TestApp/ViewController.m, PietRenderer.m:90-101) for a
machine without a display: the frame is rendered on the MI355X by the same three kernels as
bench.py and read back once.  Files are read with the SVG front-end's full document layer (groups,
transforms, style, opacity, fill-rule, basic shapes; SVG's initial `fill: black`); `tiger` is the
embedded asset read as make_tiger reads it (src/lib.rs:286-328).  --frames renders an animation the
way the reference's view does on every change (PietRenderer.m:90-101, :145): the scene is encoded
again for each frame -- here by re-flattening the resident paths on the device (pm_reflatten; with
--explode pm_reflatten_groups, one affine per top-level group of the document).  --fade changes colours only: nothing is
flattened again, pm_repaint_groups rewrites the colour words of the resident scene (one opacity per top-level group).
"""
from __future__ import annotations

import argparse
import json
import struct
import sys
import zlib

import numpy as np


def write_png(path: str, rgba: np.ndarray) -> None:
    """RGBA8 [H, W, 4] -> PNG (colour type 6, no interlace); stdlib only."""
    h, w, c = rgba.shape
    if c != 4 or rgba.dtype != np.uint8:
        raise ValueError("write_png needs an [H, W, 4] uint8 array")
    raw = np.empty((h, 1 + 4 * w), np.uint8)
    raw[:, 0] = 0  # filter type None
    raw[:, 1:] = rgba.reshape(h, 4 * w)

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def read_png_rgba(path: str) -> np.ndarray:
    """Inverse of write_png (only the subset write_png produces); used by the tests."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        (n,), tag = struct.unpack(">I", data[pos : pos + 4]), data[pos + 4 : pos + 8]
        body = data[pos + 8 : pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 4).copy()


def print_selection(r, values, touched, enclosed) -> None:
    """--select / --lasso: one line per touched item, in paint order, headed by the query's values as they were given."""
    of_item = r.item_paths()
    name = ",".join(f"{v:g}" for v in values)
    for i in np.flatnonzero(touched):
        print(f"{name}: item {int(i)} path {int(of_item[i])}" + (" enclosed" if enclosed[i] else ""))
    if not touched.any():
        print(f"{name}: none")


def print_snaps(r, points, radius, to) -> None:
    """--snap: one line per point with the record Renderer.snap returns for it."""
    if to == "intersections":
        from . import _lib

        rec = r.snap_intersections(np.array(points, np.float32), radius)
        of_item = r.item_paths()
        for (x, y), s in zip(points, rec):
            head = f"{x:g},{y:g} r {radius:g}: "
            if s["kind"] == _lib.PM_SNAP_KIND_TOO_MANY:
                print(head + f"more than {_lib.PM_SNAP_MAX_NEAR_EDGES} edges within the radius ({int(s['n_near'])}): ask again with a smaller one")
            elif s["item"] == _lib.PM_HIT_NONE:
                print(head + "none")
            else:
                print(head + f"item {int(s['item'])} path {int(of_item[s['item']])} edge {int(s['index'])} t {float(s['t']):.9g} crosses "
                      f"item {int(s['item2'])} path {int(of_item[s['item2']])} edge {int(s['index2'])} u {float(s['u']):.9g} "
                      f"at {float(s['x']):.9g},{float(s['y']):.9g} d2 {float(s['d2']):.17g}")
        return
    rec = r.snap(np.array(points, np.float32), radius, vertices=to != "edges", edges=to != "vertices")
    of_item = r.item_paths()
    for (x, y), s in zip(points, rec):
        head = f"{x:g},{y:g} r {radius:g}: "
        if s["item"] == 0xFFFFFFFF:
            print(head + "none")
            continue
        what = f"vertex {int(s['index'])}" if s["kind"] == 1 else f"edge {int(s['index'])} t {float(s['t']):.9g}"
        print(head + f"item {int(s['item'])} path {int(of_item[s['item']])} {what} at {float(s['x']):.9g},{float(s['y']):.9g} d2 {float(s['d2']):.17g}")


def point_line(i, d, p, of_item) -> str:
    """One point record of item i at distance d (pixels) as --point-at prints it."""
    head = f"item {i} at {d:g}: "
    if p["item"] == 0xFFFFFFFF:
        return head + "none"
    return (head + f"point {float(p['x']):g},{float(p['y']):g} tangent {float(p['tx']):g},{float(p['ty']):g} segment {int(p['index'])} "
            f"t {float(p['t']):g} path {int(of_item[i])}" + (" (clamped)" if p["status"] & 2 else ""))


def print_points_at(r, asks) -> None:
    """--point-at: one line per (item, distance in pixels)."""
    rec = r.points_at_length([a[0] for a in asks], [a[1] for a in asks])
    of_item = r.item_paths()
    for (i, d), p in zip(asks, rec):
        print(point_line(i, d, p, of_item))


def print_resampled(r, even, stepped) -> None:
    """--resample ITEM,N and --resample-step ITEM,STEP[,START]: per request a line with the item's length in pixels and how many of
    its points are not clamped, then one line per point as --point-at prints it, at the position the device gave the point."""
    from .renderer import LENGTH_UNIT, length_units, resample_positions

    of_item = r.item_paths()
    for asks, mode in ((even, 1), (stepped, 0)):
        if not asks:
            continue
        items = [a[0] for a in asks]
        if mode == 1:
            pts, offsets, infos = r.resample(items, [a[1] for a in asks])
        else:
            pts, offsets, infos = r.resample_step(items, [a[1] for a in asks], [a[2] for a in asks])
        for k, (a, info) in enumerate(zip(asks, infos)):
            n = int(offsets[k + 1] - offsets[k])
            what = f"{n} even" if mode == 1 else f"every {a[1]:g} from {a[2]:g}"
            print(f"resample item {a[0]} {what}: length {int(info['length']) / LENGTH_UNIT:g} points {n} unclamped {int(info['n_unclamped'])}")
            ss = resample_positions(mode, n, int(info["length"]), int(info["kind"]), 0 if mode == 1 else length_units(a[2]), 0 if mode == 1 else length_units(a[1]))
            for s, p in zip(ss, pts[offsets[k]:offsets[k + 1]]):
                print(point_line(a[0], s / LENGTH_UNIT, p, of_item))


def vertex_line(v) -> str:
    """One trimmed vertex as --trim prints it."""
    return (f"  {'move' if v['flags'] & 1 else 'line'} {float(v['x']):g},{float(v['y']):g} segment {int(v['index'])}" + (" (cut)" if v["flags"] & 2 else ""))


def print_trimmed(r, ranges, parts) -> None:
    """--trim ITEM,START,END and --trim-parts ITEM,M: per piece a header line with its ends and the item's length in pixels and how
    many vertices and runs it has, then one line per vertex."""
    from .renderer import LENGTH_UNIT

    if ranges:
        vs, offsets, infos = r.trim([a[0] for a in ranges], [a[1] for a in ranges], [a[2] for a in ranges])
        for k, (a, info) in enumerate(zip(ranges, infos)):
            print(f"trim item {a[0]} [{a[1]:g}, {a[2]:g}]: length {int(info['length']) / LENGTH_UNIT:g} vertices {int(info['n_vertices'])} runs {int(info['n_runs'])}")
            for v in vs[offsets[k]:offsets[k + 1]]:
                print(vertex_line(v))
    k = 0
    if parts:
        vs, offsets, infos = r.trim_parts([a[0] for a in parts], [a[1] for a in parts])
    for i, m in parts:
        for j in range(m):
            T = int(infos[k]["length"])
            a, b = (j * (T // m) + min(j, T % m)) / LENGTH_UNIT, ((j + 1) * (T // m) + min(j + 1, T % m)) / LENGTH_UNIT
            print(f"trim item {i} [{a:g}, {b:g}]: length {T / LENGTH_UNIT:g} vertices {int(infos[k]['n_vertices'])} runs {int(infos[k]['n_runs'])}")
            for v in vs[offsets[k]:offsets[k + 1]]:
                print(vertex_line(v))
            k += 1


def crossing_line(c, s_a: int) -> str:
    """One crossing as --crossings prints it: the point, the edge and the parameter on either item, how far along A it lies in pixels,
    and which way B crosses A."""
    from .renderer import LENGTH_UNIT

    return (f"  {float(c['x']):g},{float(c['y']):g} a segment {int(c['index_a'])} t {float(c['t']):g} at {int(s_a) / LENGTH_UNIT:g}"
            f" b segment {int(c['index_b'])} u {float(c['u']):g} side {'+' if int(c['side']) == 1 else '-'}")


def print_crossings(r, pairs) -> None:
    """--crossings A,B and --self-crossings ITEM: per request a header line with the number of crossings and the two index ranges, then
    one line per crossing in the order of the edges."""
    recs, offsets, infos = r.crossings([p[0] for p in pairs], [p[1] for p in pairs])
    s_a, _ = r.crossing_positions(recs)
    for k, ((a, b), info) in enumerate(zip(pairs, infos)):
        what = f"self-crossings item {a}" if a == b else f"crossings items {a},{b}"
        print(f"{what}: {int(info['n_crossings'])} edges {int(info['n_a'])} x {int(info['n_b'])}" + (" (too many pairs)" if int(info["flags"]) & 2 else ""))
        for p in range(int(offsets[k]), int(offsets[k + 1])):
            print(crossing_line(recs[p], s_a[p]))


def bounds_record(r, words=None) -> dict:
    """--bounds: the box and the counts of the whole scene (words None) or of the items whose word is non-zero."""
    box, n_items, n_boxed = r.selection_bounds(words)
    return {"box": [float(v) for v in box], "n_items": n_items, "n_boxed": n_boxed}


def fit_affine(base, scale, box, width, height):
    """--fit: (affine, width_scale) -- `base` followed by the uniform scale and the translation that put `box` into the width x height
    view, touching its edges along one axis and centred along the other."""
    x0, y0, x1, y1 = (float(v) for v in box)
    bw, bh = x1 - x0, y1 - y0
    s = min(width / bw if bw > 0 else float("inf"), height / bh if bh > 0 else float("inf"))
    if s == float("inf"):  # a point: nothing to scale
        s = 1.0
    tx, ty = (width - s * (x0 + x1)) / 2.0, (height - s * (y0 + y1)) / 2.0
    a, b, c, d, e, f = base
    return (s * a, s * b, s * c, s * d, s * e + tx, s * f + ty), scale * s


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m piet_metal_amd.cli", description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="an .svg file, or 'tiger' for the embedded Ghostscript Tiger")
    ap.add_argument("output", help="PNG file to write")
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1600)
    ap.add_argument("--scale", type=float, default=None, help="user units -> pixels (default: fit the file's viewBox into the viewport; the Tiger: height / 200)")
    ap.add_argument("--offset", type=float, nargs=2, default=None, metavar=("X", "Y"), help="translation in pixels (default: centre horizontally)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reject-arc-paths", action="store_true", help="skip <path>s that use the arc command (kurbo 0.5.6 question, SURVEY F6)")
    ap.add_argument("--reference-fill-rule", action="store_true", help="files: only a fill property fills (make_tiger, src/lib.rs:299) instead of SVG's initial black")
    ap.add_argument("--no-flat-gradients", action="store_true", help="files: do not draw gradient paints at all (default: as the mean colour of their stops)")
    ap.add_argument("--stroke-styles", action="store_true", help="files: read stroke-linecap / stroke-linejoin / stroke-miterlimit and draw strokes as outlines with those caps and joins (default: every stroke is the round poly-line)")
    ap.add_argument("--stroke-dashes", action="store_true", help="files: also read stroke-dasharray / stroke-dashoffset and cut the outlined strokes into dashes (implies --stroke-styles)")
    ap.add_argument("--frames", type=int, default=1, help="render an animation of this many frames (output NAME-###.png)")
    ap.add_argument("--spin", type=float, default=360.0, help="--frames: total rotation about the viewport centre, degrees")
    ap.add_argument("--explode", type=float, default=None, metavar="F", help="--frames N (>= 2): instead of spinning, frame k moves every top-level group of the document (element child of the outermost <svg>) by F * k / (N - 1) * (its centre - the document's centre); the groups are re-flattened on the device, each under its own affine")
    ap.add_argument("--fade", action="store_true", help="--frames N (>= 2): instead of spinning, the top-level groups of the document fade out one after another: frame k shows group g of G with opacity round(255 * clamp(1 - k / (N - 1) * G + g, 0, 1)); only the colours of the resident scene are rewritten on the device.  With --explode: both")
    ap.add_argument("--pick", action="append", default=[], metavar="X,Y", help="hit test: print the topmost item under this point (pixels) and the path it came from; may be repeated")
    ap.add_argument("--pick-tolerance", type=float, default=None, metavar="T", help="every --pick names the topmost item that comes within the square of half side T (pixels) around its point, instead of the item under the point itself")
    ap.add_argument("--pick-depth", type=int, default=1, metavar="K", help="every --pick names up to K items (1 .. 256) under its point -- with --pick-tolerance: within the square around it --, topmost first, each with the path it came from: select-behind")
    ap.add_argument("--select", default=None, metavar="X0,Y0,X1,Y1", help="marquee selection: print every item the closed rectangle touches, occluded ones included, and the path it came from; items that lie wholly inside it are marked 'enclosed'")
    ap.add_argument("--lasso", default=None, metavar="X,Y,X,Y,...", help="lasso selection: the same for the polygon of these vertices (three or more, pixels), which closes itself, under the non-zero rule; an item is 'enclosed' if its outline lies inside and does not reach the polygon's boundary")
    ap.add_argument("--snap", action="append", default=[], metavar="X,Y", help="snapping: print the nearest vertex or point of an edge within --snap-radius of this point (pixels) -- the item, the path it came from, the vertex's or segment's index in the item, the point and its distance; may be repeated")
    ap.add_argument("--snap-radius", type=float, default=None, metavar="R", help="how far (pixels) a --snap looks; needed with --snap")
    ap.add_argument("--snap-to", choices=("vertices", "edges", "both", "intersections"), default="both", help="what a --snap looks for; with 'both' a vertex within the radius wins over every edge; 'intersections': the nearest point where two edges cross")
    ap.add_argument("--bounds", action="store_true", help="bounds: print one JSON line with the box {x0, y0, x1, y1} (pixels) of everything that is drawn and how many items it has -- \"scene\" -- and, with --select / --lasso, the same for the items the query touches -- \"selection\"; with --fit: of the fitted view")
    ap.add_argument("--fit", action="store_true", help="zoom to fit: before rendering, change the view so that the box of everything drawn -- with --select / --lasso: of what the query touches in the view as given -- fills the output, centred; what --select / --lasso print is what they touched in the view as given")
    ap.add_argument("--item-map", default=None, metavar="OUT.npy", help="save the item map of the rendered view -- uint32 [height, width], the topmost item under every pixel's centre, 0xffffffff where there is none (numpy.save) -- and print how many distinct items are visible and how many pixels show none; with --frames: of the last frame")
    ap.add_argument("--coverage", action="store_true", help="coverage counts: for every item that covers a pixel of the rendered view print its index, the path it came from, how many pixel centres it covers, on how many of them it is under no opaque item (visible), on how many it is the topmost item (top), and the first pixel X,Y that shows it; with --frames: of the first frame")
    ap.add_argument("--hidden", action="store_true", help="coverage counts: print the indices of the items no pixel of the rendered view shows -- outside it, or wholly under opaque items")
    ap.add_argument("--lengths", action="store_true", help="path measurement: print one JSON line {\"paths\": [{\"length\", \"n_items\"}, ...]} -- per path the length in pixels of the geometry it draws (flattened curves, the outlines of styled and dashed strokes, closing segments included) and how many items that is")
    ap.add_argument("--point-at", action="append", default=[], metavar="ITEM,DIST", help="path measurement: print the point DIST pixels along item ITEM, the unit tangent there, the segment it lies on with the parameter along it, and the path the item came from; beyond the item's end: its end, marked (clamped); may be repeated")
    ap.add_argument("--resample", action="append", default=[], metavar="ITEM,N", help="resampling: print N evenly spaced points along item ITEM -- an open item from its start to its end, a closed one from its start without repeating it -- after a line with the item's length in pixels and how many of the points are not clamped; one line per point as --point-at prints it; may be repeated")
    ap.add_argument("--resample-step", action="append", default=[], metavar="ITEM,STEP[,START]", help="resampling: the same for a point every STEP pixels along item ITEM from START pixels on (default 0), as many as fit; may be repeated")
    ap.add_argument("--trim", action="append", default=[], metavar="ITEM,START,END", help="trimming: print the piece of item ITEM between START and END pixels along it (END may be inf) -- a header line with the item's length in pixels and the piece's numbers of vertices and runs, then one line per vertex: 'move' starts a run, '(cut)' marks an interpolated end; may be repeated")
    ap.add_argument("--trim-parts", action="append", default=[], metavar="ITEM,M", help="trimming: the same for each of M even pieces of item ITEM, in order; may be repeated")
    ap.add_argument("--crossings", action="append", default=[], metavar="A,B", help="item crossings: print every point where an edge of item A crosses an edge of item B -- a header line with the number of crossings and the two items' numbers of edge indices, then one line per crossing in the order of the edges: the point, the segment and the parameter on either item, how many pixels along A it lies, and which way B crosses A; may be repeated")
    ap.add_argument("--self-crossings", action="append", default=[], metavar="ITEM", help="item crossings: the same for the points where item ITEM crosses itself, each once; may be repeated")
    args = ap.parse_args(argv)
    try:
        trim_ranges = [(int(p.split(",")[0]), float(p.split(",")[1]), float(p.split(",")[2])) for p in args.trim]
        if any(p.count(",") != 2 for p in args.trim) or any(i < 0 or i > 0xFFFFFFFF or not start >= 0 or not end >= start for i, start, end in trim_ranges):
            raise ValueError
    except (ValueError, IndexError):
        ap.error("--trim takes ITEM,START,END with 0 <= START <= END, in pixels")
    try:
        trim_parts = [(int(p.split(",")[0]), int(p.split(",")[1])) for p in args.trim_parts]
        if any(p.count(",") != 1 for p in args.trim_parts) or any(i < 0 or i > 0xFFFFFFFF or not 1 <= m <= 1 << 20 for i, m in trim_parts):
            raise ValueError
    except (ValueError, IndexError):
        ap.error("--trim-parts takes ITEM,M with 1 <= M <= 1048576")
    try:
        crossing_pairs = [(int(p.split(",")[0]), int(p.split(",")[1])) for p in args.crossings]
        if any(p.count(",") != 1 for p in args.crossings) or any(not 0 <= i <= 0xFFFFFFFF for pair in crossing_pairs for i in pair):
            raise ValueError
    except (ValueError, IndexError):
        ap.error("--crossings takes A,B")
    try:
        crossing_pairs += [(int(p), int(p)) for p in args.self_crossings]
        if any(not 0 <= i <= 0xFFFFFFFF for i, _ in crossing_pairs):
            raise ValueError
    except ValueError:
        ap.error("--self-crossings takes ITEM")
    try:
        resample_even =[(int(p.split(",")[0]), int(p.split(",")[1])) for p in args.resample]
        if any(len(p.split(",")) != 2 for p in args.resample) or any(i < 0 or i > 0xFFFFFFFF or not 0 <= n <= 1 << 20 for i, n in resample_even):
            raise ValueError
    except (ValueError, IndexError):
        ap.error("--resample takes ITEM,N with 0 <= N <= 1048576")
    try:
        resample_step = [(int(p.split(",")[0]), float(p.split(",")[1]), float(p.split(",")[2]) if p.count(",") == 2 else 0.0) for p in args.resample_step]
        if any(p.count(",") not in (1, 2) for p in args.resample_step) or any(i < 0 or i > 0xFFFFFFFF or not step * 65536 >= 0.5 or not start >= 0 for i, step, start in resample_step):
            raise ValueError
    except (ValueError, IndexError):
        ap.error("--resample-step takes ITEM,STEP[,START] with STEP > 0 and START >= 0, in pixels")
    try:
        points_at = [(int(p.split(",")[0]), float(p.split(",")[1])) for p in args.point_at]
        if any(len(p.split(",")) != 2 for p in args.point_at) or any(i < 0 or i > 0xFFFFFFFF for i, _ in points_at):
            raise ValueError
    except (ValueError, IndexError):
        ap.error("--point-at takes ITEM,DIST")
    try:
        picks = [tuple(float(v) for v in p.split(",")) for p in args.pick]
        if any(len(p) != 2 for p in picks):
            raise ValueError
    except ValueError:
        ap.error("--pick takes X,Y")
    try:
        select = tuple(float(v) for v in args.select.split(",")) if args.select is not None else None
        if select is not None and len(select) != 4:
            raise ValueError
    except ValueError:
        ap.error("--select takes X0,Y0,X1,Y1")
    try:
        lasso = tuple(float(v) for v in args.lasso.split(",")) if args.lasso is not None else None
        if lasso is not None and (len(lasso) < 6 or len(lasso) % 2):
            raise ValueError
    except ValueError:
        ap.error("--lasso takes X,Y,X,Y,... with at least three pairs")
    try:
        snaps = [tuple(float(v) for v in p.split(",")) for p in args.snap]
        if any(len(p) != 2 for p in snaps):
            raise ValueError
    except ValueError:
        ap.error("--snap takes X,Y")
    if not 1 <= args.pick_depth <= 256:
        ap.error("--pick-depth takes 1 .. 256")
    if snaps and args.snap_radius is None:
        ap.error("--snap needs --snap-radius R")
    if args.explode is not None and args.frames < 2:
        ap.error("--explode needs --frames N with N >= 2")
    if args.fade and args.frames < 2:
        ap.error("--fade needs --frames N with N >= 2")
    grouped = args.explode is not None or args.fade

    from . import PathSet, Renderer

    if args.input == "tiger":
        paths = PathSet.tiger(args.reject_arc_paths, groups=grouped)
    else:
        with open(args.input, "rb") as f:
            paths = PathSet.from_svg(f.read(), args.reject_arc_paths, spec_defaults=not args.reference_fill_rule, flat_gradients=not args.no_flat_gradients,
                                     stroke_styles=args.stroke_styles or args.stroke_dashes, stroke_dashes=args.stroke_dashes,
                                     groups=grouped)
    scale = args.scale if args.scale is not None else args.height / 200.0
    off = args.offset if args.offset is not None else ((args.width - args.height) / 2.0 if args.scale is None else 0.0, 0.0)
    base = (scale, 0.0, 0.0, scale, float(off[0]), float(off[1]))
    fit = paths.fit_affine(args.width, args.height) if (args.input != "tiger" and args.scale is None and args.offset is None) else None
    if fit is not None:  # a file that says where its picture is: show that, centred (xMidYMid meet)
        base, scale = fit
    with Renderer(args.device) as r:
        r.resize(args.width, args.height)
        nbytes, nitems = r.flatten_and_encode(paths, base, scale)
        # a selection is taken in the view as given; --fit keeps the items (a re-flatten changes no item's index)
        selected = r.select_rect(*select) if select is not None else None
        lassoed = r.select_polygon(np.array(lasso, np.float32).reshape(-1, 2)) if lasso is not None else None
        chosen = selected[0] if selected is not None else (lassoed[0] if lassoed is not None else None)
        if args.fit:
            rec = bounds_record(r, chosen)
            if not rec["n_boxed"]:
                ap.error("--fit: nothing to fit the view to")
            base, scale = fit_affine(base, scale, rec["box"], args.width, args.height)
            nbytes, nitems = r.reflatten(base, scale)
        if args.bounds:
            out = {"scene": bounds_record(r)}
            if chosen is not None:
                out["selection"] = bounds_record(r, chosen)
            print(json.dumps(out))
        r.render()
        img = r.read_pixels()
        if picks and args.pick_depth > 1:  # one line per point: up to K items under it (or within the tolerance), topmost first
            xy = np.array(picks, np.float32)
            stack = r.hit_stack(xy, args.pick_depth) if args.pick_tolerance is None else r.pick_stack(xy, args.pick_tolerance, args.pick_depth)
            of_item = r.item_paths()
            tol = "" if args.pick_tolerance is None else f" +-{args.pick_tolerance:g}"
            for (x, y), items in zip(picks, stack):
                found = [f"item {int(t)} path {int(of_item[t])}" for t in items if t != 0xFFFFFFFF]
                print(f"{x:g},{y:g}{tol}: " + (", ".join(found) if found else "none"))
        elif picks and args.pick_tolerance is None:  # one line per point: the item in flat paint order and the <path> it came from, or none
            top = r.hit_test(np.array(picks, np.float32))
            of_item = r.item_paths()
            for (x, y), t in zip(picks, top):
                print(f"{x:g},{y:g}: " + ("none" if t == 0xFFFFFFFF else f"item {int(t)} path {int(of_item[t])}"))
        elif picks:  # the same with a tolerance: the topmost item the square around the point touches
            top = r.pick(np.array(picks, np.float32), args.pick_tolerance)
            of_item = r.item_paths()
            for (x, y), t in zip(picks, top):
                print(f"{x:g},{y:g} +-{args.pick_tolerance:g}: " + ("none" if t == 0xFFFFFFFF else f"item {int(t)} path {int(of_item[t])}"))
        if select is not None:  # one line per item the rectangle touches, in paint order
            print_selection(r, select, *selected)
        if lasso is not None:  # the same lines for a polygon
            print_selection(r, lasso, *lassoed)
        if snaps:  # one line per point: the record, and the <path> the item came from
            print_snaps(r, snaps, args.snap_radius, args.snap_to)
        if args.lengths:  # one JSON line: per path its length in pixels and its item count
            lengths, counts = r.path_lengths()
            print(json.dumps({"paths": [{"length": v / 65536, "n_items": c} for v, c in zip(lengths, counts)]}))
        if points_at:  # one line per query: the record, and the <path> the item came from
            print_points_at(r, points_at)
        if resample_even or resample_step:  # per request a summary line, then one line per point
            print_resampled(r, resample_even, resample_step)
        if trim_ranges or trim_parts:  # per piece a header line, then one line per vertex
            print_trimmed(r, trim_ranges, trim_parts)
        if crossing_pairs:  # per request a header line, then one line per crossing
            print_crossings(r, crossing_pairs)
        if args.coverage:  # one line per item that covers a pixel of the view
            print_coverage(r, args)
        if args.hidden:  # one line: the items no pixel of the view shows
            print("hidden: " + (" ".join(str(int(i)) for i in r.hidden_items(0, 0, args.width, args.height)) or "none"))
        if args.frames <= 1:
            if args.item_map:
                save_item_map(r, args)
            write_png(args.output, img)
            print(f"{args.output}: {args.width}x{args.height}, {nitems} items, scene {nbytes} bytes", file=sys.stderr)
            return 0
        import math
        import time

        stem = args.output[:-4] if args.output.lower().endswith(".png") else args.output
        cx, cy = args.width / 2.0, args.height / 2.0
        t_gpu = 0.0
        away = group_offsets(paths) if args.explode is not None else None
        for k in range(args.frames):
            aff = spin_affine(base, math.radians(args.spin * k / args.frames), cx, cy)
            t0 = time.perf_counter()
            if away is not None:  # every top-level group under its own affine: base after a translation in user units
                affs = explode_affines(base, away * (args.explode * k / (args.frames - 1)))
                nbytes, nitems = r.reflatten_groups(affs, np.full(len(affs), scale, np.float32))
            elif not args.fade:
                nbytes, nitems = r.reflatten(aff, scale)  # the per-frame re-encode, on the device
            if args.fade:  # colours only: no flatten, the scene index and the binning plan stay
                r.repaint_groups(fade_opacities(k, args.frames, paths.n_groups()))
            r.render()
            r.sync()
            t_gpu += time.perf_counter() - t0
            write_png(f"{stem}-{k:03d}.png", r.read_pixels())
        if args.item_map:
            save_item_map(r, args)
        print(f"{stem}-###.png: {args.frames} frames {args.width}x{args.height}, re-encode + render {t_gpu / args.frames * 1e3:.2f} ms per frame", file=sys.stderr)
    return 0


def print_coverage(r, args) -> None:
    """--coverage: per item that covers a pixel of the view its index, the path it came from where there is one, the three counts
    and the first pixel that shows it."""
    cov = r.item_coverage(0, 0, args.width, args.height)
    of_item = r.item_paths()
    for i in np.flatnonzero(cov["covered"]):
        rec = cov[i]
        path = f" path {int(of_item[i])}" if i < len(of_item) and of_item[i] != 0xFFFFFFFF else ""
        first = int(rec["first_visible"])
        at = "none" if first == 0xFFFFFFFF else f"{first % args.width},{first // args.width}"
        print(f"item {int(i)}{path}: covered {int(rec['covered'])} visible {int(rec['visible'])} top {int(rec['top'])} first_visible {at}")


def save_item_map(r, args) -> None:
    """--item-map: the resident scene's item map over the viewport, to a .npy file, and one line about it."""
    top = r.hit_frame(0, 0, args.width, args.height)
    with open(args.item_map, "wb") as f:  # (numpy.save appends ".npy" to a NAME without it: a file object keeps the name given)
        np.save(f, top)
    none = int((top == 0xFFFFFFFF).sum())
    print(f"{args.item_map}: {len(np.unique(top)) - (1 if none else 0)} items visible, {none} pixels with no item")


def group_offsets(paths) -> np.ndarray:
    """(G, 2): for every group of paths.groups the centre of the box of its elements' coordinates (control points included)
    minus the centre of the box of all of them, in user units; a group without coordinates stays where it is."""
    els, tags = paths.els, paths.els["tag"]
    used = np.zeros((len(els), 6), bool)  # which of p[0..6) an element's tag gives a meaning to
    for tag, n in ((0, 2), (1, 2), (2, 4), (3, 6)):  # MoveTo, LineTo, QuadTo, CurveTo
        used[tags == tag, :n] = True
    group_of_el = np.repeat(paths.groups, paths.paths["el_end"] - paths.paths["el_begin"])

    def centre(mask):
        m = used & mask[:, None]
        if not m.any():
            return None
        x, y = els["p"][:, 0::2][m[:, 0::2]], els["p"][:, 1::2][m[:, 1::2]]
        return np.array([(x.min() + x.max()) / 2.0, (y.min() + y.max()) / 2.0])

    doc = centre(np.ones(len(els), bool))
    out = np.zeros((paths.n_groups(), 2))
    for g in range(len(out)):
        c = centre(group_of_el == g)
        if c is not None:
            out[g] = c - doc
    return out


def fade_opacities(k: int, n_frames: int, n_groups: int) -> np.ndarray:
    """(G,) uint32: the opacity of every group in frame k of n_frames (>= 2): round(255 * clamp(1 - k / (N - 1) * G + g, 0, 1)),
    in exact integer arithmetic.  All 255 in frame 0, all 0 in the last; group g is gone when group g + 1 begins to fade."""
    g = np.arange(n_groups, dtype=np.int64)
    den = n_frames - 1
    num = np.clip(den * (1 + g) - k * n_groups, 0, den)  # clamp(...) * den
    return ((2 * 255 * num + den) // (2 * den)).astype(np.uint32)


def explode_affines(base, shifts) -> np.ndarray:
    """(G, 6): `base` after a translation by shifts[g] (user units), per group."""
    a, b, c, d, e, f = base
    out = np.tile(np.array(base, np.float64), (len(shifts), 1))
    out[:, 4] = e + a * shifts[:, 0] + c * shifts[:, 1]
    out[:, 5] = f + b * shifts[:, 0] + d * shifts[:, 1]
    return out


def spin_affine(base, theta: float, cx: float, cy: float):
    """`base` followed by a rotation by theta about (cx, cy) (kurbo Affine coefficients [a b c d e f])."""
    import math

    a, b, c, d, e, f = base
    cs, sn = math.cos(theta), math.sin(theta)
    # R * base, R = translate(cx, cy) rotate(theta) translate(-cx, -cy)
    re, rf = cx - cs * cx + sn * cy, cy - sn * cx - cs * cy
    return (cs * a - sn * b, sn * a + cs * b, cs * c - sn * d, sn * c + cs * d, cs * e - sn * f + re, sn * e + cs * f + rf)


if __name__ == "__main__":
    sys.exit(main())
