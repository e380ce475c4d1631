"""Numpy restatement of hit stacks, decision D24: the k topmost items under a point or a rectangle.  Written from the
decision's text; test infrastructure.  It defines no geometry of its own: whether item i is a member of query q's set H is asked of
tests/np_hit.py (item_inside: D13's "contains") or tests/np_rect.py (item_flags & TOUCHES: D19's "touches"), one item at a time, with
no flag; the skip rule and the opaque byte are read from the scene's item records (np_hit.flat_items).

  H         the members, minus -- under skip_transparent -- every Line, Fill or Polyline whose colour has alpha 0;
  order     item index descending (flat paint order, topmost first);
  the cut   under stop_at_opaque the sequence ends at its first opaque member, which is included: a Circle or ellipse always is, a
            Line, Fill or Polyline iff its alpha byte is 255; no opaque member: all of H;
  answer    items[q, j] = the j-th member for j < min(k, m), HIT_NONE behind; n_hit[q] = m, the length after the cut, not clipped by k.
"""
import struct

import numpy as np

import np_hit
import np_rect

HIT_NONE = np_hit.HIT_NONE
STACK_MAX = 256   # PM_HIT_STACK_MAX
SKIP_TRANSPARENT, STOP_AT_OPAQUE = 1, 8   # PM_HIT_SKIP_TRANSPARENT, PM_HIT_STOP_AT_OPAQUE


def item_alphas(scene):
    """(alpha int [n_items], coloured bool [n_items]): the alpha byte of every Line, Fill and Polyline in flat paint order -- the byte
    the skip rule reads --; a Circle or ellipse has no colour of its own (coloured False) and is drawn opaque black: alpha 255."""
    sc = bytes(scene)
    items = np_hit.flat_items(sc)
    alpha, coloured = np.full(len(items), 255, np.int64), np.zeros(len(items), bool)
    for i, (at, _) in enumerate(items):
        tag = struct.unpack_from("<I", sc, at)[0] & 0xFFFF
        if tag in (np_hit.LINE, np_hit.FILL, np_hit.POLY):
            alpha[i] = struct.unpack_from("<I", sc, at + (4 if tag == np_hit.POLY else 8))[0] >> 24
            coloured[i] = True
    return alpha, coloured


def point_members(scene, pts):
    """bool [n_items, n]: item i contains point q (D13, no flag; a non-finite point is in no item)."""
    sc = bytes(scene)
    n_items = len(np_hit.flat_items(sc))
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros((n_items, len(pts)), bool)
    for i in range(n_items):
        out[i] = np_hit.item_inside(sc, i, pts)
    return out


def rect_members(scene, rects):
    """bool [n_items, n]: rectangle q touches item i (D19, no flag; an invalid rectangle touches nothing)."""
    return (np_rect.item_flags(scene, np.asarray(rects, np.float32).reshape(-1, 4)) & np_rect.TOUCHES) != 0


def stack(scene, members, k, skip_transparent=False, stop_at_opaque=False):
    """(items uint32 [n, k], n_hit uint32 [n]) from the membership matrix of point_members / rect_members."""
    assert 1 <= k <= STACK_MAX
    alpha, coloured = item_alphas(scene)
    H = np.array(members, bool)
    n_items, n = H.shape
    assert n_items == len(alpha)
    if skip_transparent:
        H &= ~(coloured & (alpha == 0))[:, None]
    index = np.arange(n_items)
    if stop_at_opaque:
        opaque = H & (alpha == 255)[:, None]
        first = np.where(opaque.any(axis=0), n_items - 1 - np.argmax(opaque[::-1], axis=0), -1) if n_items else np.full(n, -1)
        H &= index[:, None] >= first[None, :]          # everything below the first opaque member is cut
    top_first = H[::-1]
    rank = np.cumsum(top_first, axis=0) - 1
    items = np.full((n, k), HIT_NONE, np.uint32)
    ii, qq = np.nonzero(top_first & (rank < k))
    items[qq, rank[ii, qq]] = index[::-1][ii]
    return items, H.sum(axis=0).astype(np.uint32)


def hit_stack(scene, pts, k, skip_transparent=False, stop_at_opaque=False, members=None):
    return stack(scene, point_members(scene, pts) if members is None else members, k, skip_transparent, stop_at_opaque)


def hit_rects_stack(scene, rects, k, skip_transparent=False, stop_at_opaque=False, members=None):
    return stack(scene, rect_members(scene, rects) if members is None else members, k, skip_transparent, stop_at_opaque)
