#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/piet_metal_amd.h"

namespace pm {

// Device buffers of the flatten stage, kept between calls (grow only): the parsed paths and the
// scratch arrays.  With `resident` set the paths of the last upload are flattened again -- the
// per-frame re-encode of an animation (PietRenderer.m:90-101 does it on the CPU) then costs four
// kernels and two small read-backs, no allocation and no path upload.
struct FlattenCache {
    pm_path *d_paths = nullptr;
    pm_path_el *d_els = nullptr;
    uint32_t *d_u32 = nullptr;
    double *d_bbox = nullptr;
    size_t cap_paths = 0, cap_els = 0, cap_u32 = 0, cap_bbox = 0;
    size_t n_paths = 0, n_els = 0;  // what is resident in d_paths / d_els
    size_t max_items = 0;           // ... and an upper bound of the items they encode to
    // pinned: {totals[4], error flag, pad} then, at +32, the head of the scene the kernels just wrote
    // (SimpleGroup, boxes, items) -- fetched in the same wait as the totals, for validation and arena sizing
    uint8_t *h_meta = nullptr;
    size_t cap_meta = 0, meta_bytes = 0;  // meta_bytes: valid bytes at h_meta + 32 (0: not fetched)
    bool resident = false;
    bool has_outline = false;  // some resident path asks for PM_PATH_STROKE_OUTLINE: the outline stage runs (pm_stroke_outline.h)
    // the dash table of the resident paths (decision D15, pm_dash.h): n_dashes records of four words, a word per path (its
    // record's index or ~0), the values; n_dashes == 0: no table, the dash kernels are not launched
    uint32_t *d_dash = nullptr;
    size_t cap_dash = 0, n_dashes = 0;
    std::vector<uint32_t> h_dash;  // (the staging copy the upload reads)
    // the group map of the resident paths and the transform table of the last grouped re-flatten (decision D16): a word per path,
    // n_groups records; h_xforms is the pinned staging copy the table's one upload reads.  All three grow only.
    uint32_t *d_groups = nullptr;
    pm_group_xform *d_xforms = nullptr, *h_xforms = nullptr;
    size_t cap_groups = 0, cap_xforms = 0;
    bool has_groups = false;   // a map is resident (pm_path_groups since the last upload of paths)
    uint32_t max_group = 0;    // ... and its largest index
    // per-group paint (decision D17, pm_paint.h): the resident paths' own colours, {fill_rgba, stroke_rgba} per path, written
    // whenever paths are uploaded (d_paths holds the painted ones after pm_repaint_groups); the paint table and its pinned staging
    // copy.  All three grow only.
    uint2 *d_orig = nullptr;
    pm_group_paint *d_paint = nullptr, *h_paint = nullptr;
    size_t cap_orig = 0, cap_paint = 0;
    // the call that made the scene now resident: grouped (its table is still in d_xforms) or uniform with this width_scale --
    // what the thin-line rule of a repainted stroke item needs
    bool scene_grouped = false;
    float scene_width_scale = 1.0f;
    // pm_path_groups behind a grouped scene: the map that scene was made with is kept aside (the buffers change places, once per
    // scene), since its strokes' width_scales are xforms[that map[p]] whatever the new map says
    uint32_t *d_groups_scene = nullptr;
    size_t cap_groups_scene = 0;
    bool scene_map_aside = false;
    void Free();
    hipError_t Reserve(size_t n_paths, size_t n_els);  // room for this many paths / elements (pm_create)
};

// A dash table as pm_flatten_and_encode_dashed takes it (checked by FlattenEncodeOnDevice).
struct DashTable {
    const pm_path_dash *dashes;
    size_t n_dashes;
    const float *values;
    size_t n_values;
};

// Flatten + encode on the device (see pm_flatten.hip).  Synchronises `stream` (once, at the end).
// dash: nullptr or the paths' dash table (ignored with use_resident: the resident one is used again).
// use_resident: ignore h_paths / h_els and flatten the paths resident in `cache` again.
// On PM_ERR_CAPACITY *scene_bytes holds the size that would have been needed.
// grouped (needs use_resident and a resident group map): affine / width_scale are ignored, path p takes those of
// cache->d_xforms[cache->d_groups[p]] (decision D16; FlattenStageGroupTable put the table there).
int FlattenEncodeOnDevice(hipStream_t stream, FlattenCache *cache, bool use_resident, const pm_path *h_paths, size_t n_paths, const pm_path_el *h_els,
                          size_t n_els, const DashTable *dash, const double affine[6], float width_scale, uint8_t *d_scene, size_t scene_cap,
                          size_t *scene_bytes, uint32_t *n_items_out, hipError_t *hip_error, bool grouped = false);

// The group map of the resident paths (n_paths == cache->n_paths, checked by the caller): uploaded, its maximum kept.  Synchronises.
int FlattenSetPathGroups(hipStream_t stream, FlattenCache *cache, const uint32_t *group_of_path, size_t n_paths, hipError_t *hip_error);
// The transform table of a grouped re-flatten: through the pinned staging copy (grown only when n_groups grows), one asynchronous
// copy on `stream` in front of the kernels.
int FlattenStageGroupTable(hipStream_t stream, FlattenCache *cache, const pm_group_xform *xforms, size_t n_groups, hipError_t *hip_error);

// Decision D17: stages the paint table (pinned copy grown only when n_groups grows, one asynchronous copy), paints the resident
// paths' colours from their originals, copies the resident scene d_src (scene_bytes, n_items, made by the last
// FlattenEncodeOnDevice from the resident paths) to d_dst and rewrites the items' colour words there.  All on `stream`, nothing
// waited for, nothing read back.  The caller has checked the table against the resident map.
int FlattenRepaint(hipStream_t stream, FlattenCache *cache, const pm_group_paint *paints, size_t n_groups, const uint8_t *d_src, uint8_t *d_dst,
                   size_t scene_bytes, uint32_t n_items, hipError_t *hip_error);

// First item of every resident path in the scene the kernels last wrote (h_base: cache->n_paths entries; path p's items are
// [h_base[p], h_base[p + 1]), the last path's end at the scene's item count).  Synchronises `stream`.
int FlattenPathItemBases(hipStream_t stream, const FlattenCache *cache, uint32_t *h_base, hipError_t *hip_error);

}  // namespace pm
