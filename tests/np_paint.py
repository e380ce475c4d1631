"""Decision D17, the expected colours of a painted scene (test infrastructure), written from the decision's text
alone: path p's own fill_rgba / stroke_rgba go through the paint of its group,

    R, G, B:  (c * (255 - k) + t * k + 127) // 255      k = the tint's AA byte, t = the tint's channel
    A:        (a * opacity + 127) // 255

in integers, on the stored bytes of 0xRRGGBBAA.  The painted scene is the scene D1-D16 define for the painted paths: the tests
hand `painted(...)` to tests/np_groups.scene and write no flatten, stroke or dash rule again."""
import numpy as np


def paint_rgba(rgba, tint, opacity):
    """0xRRGGBBAA colours (any shape, broadcast against tint and opacity) -> painted colours, uint32."""
    rgba, tint, opacity = np.asarray(rgba, np.uint64), np.asarray(tint, np.uint64), np.asarray(opacity, np.uint64)
    assert np.all(opacity <= 255) and np.all(rgba <= 0xFFFFFFFF) and np.all(tint <= 0xFFFFFFFF)
    k = tint & 0xFF
    out = ((rgba & 0xFF) * opacity + 127) // 255
    for shift in (8, 16, 24):
        c, t = (rgba >> shift) & 0xFF, (tint >> shift) & 0xFF
        out = out | (((c * (255 - k) + t * k + 127) // 255) << shift)
    return out.astype(np.uint32)


def painted(ps, groups, tints, opacities):
    """The PathSet with painted colours: groups is the map (None: every path in group 0), tints / opacities one value per group
    (None: the identity of that field).  Everything but fill_rgba / stroke_rgba is the set's own."""
    n = len(ps.paths)
    g = np.zeros(n, np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    n_groups = int(g.max()) + 1 if n else 1
    t = np.zeros(n_groups, np.uint64) if tints is None else np.asarray(tints, np.uint64)
    o = np.full(n_groups, 255, np.uint64) if opacities is None else np.asarray(opacities, np.uint64)
    assert len(t) >= n_groups and len(o) >= n_groups
    paths = ps.paths.copy()
    paths["fill_rgba"] = paint_rgba(ps.paths["fill_rgba"], t[g], o[g])
    paths["stroke_rgba"] = paint_rgba(ps.paths["stroke_rgba"], t[g], o[g])
    return ps._like(paths, ps.els)
