// Per-group paint (decision D17): fade and tint groups of the resident paths without flattening anything again.
// Included by pm_flatten.hip inside its anonymous namespace (it uses that unit's ThinLine and layout constants); no existing
// kernel is edited.
//   KKeepColours   one thread per path, behind every upload of paths: the paths' own fill_rgba / stroke_rgba, two words per path,
//                  kept beside d_paths -- every paint starts from them, paints do not accumulate
//   KPaintPaths    one thread per path: d_paths[p].{fill,stroke}_rgba = paint(original, table[group_of_path[p]]), so that every
//                  later re-flatten (KItems, the outline and dash kernels, uniform or grouped) sees painted colours as they are
//   KRepaintItems  one thread per item of the resident scene: the ONE colour word of its record, in the other scene buffer (the
//                  rest of the scene got there by a device-to-device copy in front of this kernel)
// Plain vector loads and stores, no LDS, no scratch.
#pragma once

// Every channel c of R, G, B becomes (c (255 - k) + t k + 127) / 255, k = the tint's AA byte, t = the tint's channel; the alpha
// becomes (a opacity + 127) / 255.  Integer division; 255 is odd, so there is no tie: round to nearest.  {0, 255}: every byte as
// it was.  The mix is in the stored, sRGB-encoded bytes.
__device__ __forceinline__ uint32_t PaintRgba(uint32_t rgba, pm_group_paint paint) {
    const uint32_t k = paint.tint_rgba & 0xffu;
    uint32_t out = ((rgba & 0xffu) * paint.opacity + 127u) / 255u;
#pragma unroll
    for (int sh = 8; sh <= 24; sh += 8) {
        const uint32_t ch = (rgba >> sh) & 0xffu, t = (paint.tint_rgba >> sh) & 0xffu;
        out |= ((ch * (255u - k) + t * k + 127u) / 255u) << sh;
    }
    return out;
}

__global__ void KKeepColours(const pm_path *paths, uint32_t n_paths, uint2 *orig) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_paths) return;
    orig[p] = make_uint2(paths[p].fill_rgba, paths[p].stroke_rgba);
}

// group_of_path[p] < the table's length and opacity <= 255: host checks (pm_path_groups, pm_repaint_groups)
__global__ void KPaintPaths(pm_path *paths, uint32_t n_paths, const uint2 *orig, const uint32_t *group_of_path, const pm_group_paint *table) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_paths) return;
    const pm_group_paint paint = table[group_of_path[p]];
    const uint2 o = orig[p];
    paths[p].fill_rgba = PaintRgba(o.x, paint);
    paths[p].stroke_rgba = PaintRgba(o.y, paint);
}

// `paths` already hold the painted colours (KPaintPaths, earlier on the stream).  path_item_base / el_mvoff: what the scans of the
// call that made the resident scene left (the scene's layout does not depend on a colour).  src: the resident scene, dst: the
// other buffer, a copy of it.  grouped: the scene came from pm_reflatten_groups, a path's width_scale is its group's in `xforms`
// (the table of that call); otherwise width_scale_u, the uniform call's.
__global__ void KRepaintItems(const pm_path *paths, uint32_t n_paths, const uint32_t *path_item_base, const uint32_t *el_mvoff, uint32_t n_items,
                              bool grouped, float width_scale_u, GroupTable gt, const uint8_t *src, uint8_t *dst, uint32_t scene_bytes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const size_t at = sizeof(SimpleGroup) + static_cast<size_t>(n_items) * sizeof(ShortBbox) + static_cast<size_t>(i) * kItemSize;
    if (at + kItemSize > scene_bytes) return;
    uint32_t lo = 0, hi = n_paths;  // the last path whose first item is not behind i (paths without items share their successor's base)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (path_item_base[mid] <= i) lo = mid; else hi = mid;
    }
    const pm_path path = paths[lo];
    // a path's fill items come first: one per sub-path, or one in all when the fill is compound; its stroke items follow
    const uint32_t n_sub_path = el_mvoff[path.el_end] - el_mvoff[path.el_begin];
    const uint32_t n_fill = !(path.flags & PM_PATH_FILL) ? 0u : (path.flags & PM_PATH_COMPOUND) ? min(n_sub_path, 1u) : n_sub_path;
    uint32_t rgba = path.fill_rgba;
    if (i - path_item_base[lo] >= n_fill) {
        // encode_path_stroke, as KItems and MakeOutlineJob have it: the thin-line rule acts on the painted alpha
        float width = path.stroke_width * (grouped ? gt.xforms[gt.group_of_path[lo]].width_scale : width_scale_u);
        rgba = path.stroke_rgba;
        ThinLine(&width, &rgba);
    }
    // PietFill (an outlined or dashed stroke is one too) keeps its colour in word 2, PietStrokePolyLine in word 1
    const uint32_t tag = *reinterpret_cast<const uint32_t *>(src + at) & 0xffffu;
    if (tag == kItemPoly) reinterpret_cast<uint32_t *>(dst + at)[1] = __builtin_bswap32(rgba);
    else if (tag == kItemFill) reinterpret_cast<uint32_t *>(dst + at)[2] = __builtin_bswap32(rgba);
}
