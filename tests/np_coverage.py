"""Numpy restatement of coverage counts, decision D28: per item of a scene, how many pixels of a rectangle it covers, on
how many it can be seen, on how many it is the topmost item, and the first pixel that shows it.  Written from the decision's text;
test infrastructure.  It defines no geometry of its own: whether item i contains the centre of a pixel is asked of tests/np_hit.py
(item_inside: D13's "contains", no flag), one item at a time; the skip rule and the opaque byte are read from the scene's item
records by tests/np_stack.py (item_alphas).  No tiles, no walk from the top that ends anywhere: every item is asked about every
pixel, and an item's occluders are the union of the opaque members ABOVE it, accumulated from the top of paint order down.

  H(p)       the items that contain the centre of pixel p, float32(x0 + i) + 0.5, minus -- under skip -- every Line, Fill or
             Polyline whose colour has alpha 0;
  opaque     a Circle or ellipse always, a Line, Fill or Polyline iff its alpha byte is 255;
  covered    |{p : i in H(p)}|;
  visible    |{p : i in H(p), no opaque j > i in H(p)}|;
  top        |{p : i = max H(p)}|;
  first      min {j w + i' : pixel (x0 + i', y0 + j) counted in visible}, HIT_NONE if none;
  visible_only   covered := visible.
"""
import numpy as np

import np_hit
import np_stack

HIT_NONE = np_hit.HIT_NONE
VISIBLE_ONLY = 16   # PM_COVERAGE_VISIBLE_ONLY
DTYPE = np.dtype([("covered", "<u4"), ("visible", "<u4"), ("top", "<u4"), ("first_visible", "<u4")])


def centres(x0, y0, w, h):
    """float32 [w * h, 2], row by row: float32(x0 + i) + 0.5 (exact below 65 536); position j w + i is pixel (x0 + i, y0 + j)."""
    ys, xs = np.mgrid[0:h, 0:w]
    x = (x0 + xs).astype(np.float32) + np.float32(0.5)
    y = (y0 + ys).astype(np.float32) + np.float32(0.5)
    return np.stack([x.ravel(), y.ravel()], axis=1)


def members(scene, rect, skip=False):
    """bool [n_items, w * h]: H as a matrix."""
    sc = bytes(scene)
    n_items = len(np_hit.flat_items(sc))
    q = centres(*rect)
    H = np.zeros((n_items, len(q)), bool)
    if len(q):
        for i in range(n_items):
            H[i] = np_hit.item_inside(sc, i, q)
    if skip:
        alpha, coloured = np_stack.item_alphas(sc)
        H &= ~(coloured & (alpha == 0))[:, None]
    return H


def coverage(scene, rect, skip=False, visible_only=False, H=None):
    """DTYPE [n_items] for rect = (x0, y0, w, h).  H: the matrix of members(scene, rect, skip), if the caller has it."""
    sc = bytes(scene)
    H = members(sc, rect, skip) if H is None else H
    n_items, n = H.shape
    alpha, _ = np_stack.item_alphas(sc)
    out = np.zeros(n_items, DTYPE)
    out["first_visible"] = HIT_NONE
    occluded = np.zeros(n, bool)      # an opaque member above the item at hand
    answered = np.zeros(n, bool)      # any member above it
    for i in range(n_items - 1, -1, -1):
        seen = H[i] & ~occluded
        out["covered"][i] = H[i].sum()
        out["visible"][i] = seen.sum()
        out["top"][i] = (H[i] & ~answered).sum()
        if seen.any():
            out["first_visible"][i] = np.flatnonzero(seen)[0]
        answered |= H[i]
        if alpha[i] == 255:
            occluded |= H[i]
    if visible_only:
        out["covered"] = out["visible"]
    return out
