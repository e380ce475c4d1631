// What the query kernels share: pm_hit_test.h, pm_hit_frame.h, pm_hit_rect.h, pm_hit_poly.h, pm_hit_stack.h, pm_coverage.h, pm_snap.h, pm_snap_cross.h,
// pm_bounds.h, pm_measure.h, pm_resample.h, pm_trim.h and pm_crossings.h.  None of them is on the frame path: they read the scene and the scene index (pm_index_kernel), nothing a frame
// writes.  Included by pm_context.hip through those headers, in whose unit the kernels are compiled.
//
//  * SceneView: what a kernel reads of the context, the first member of every query's params (the host fills it in ONE place,
//    QueryView in pm_context.hip);
//  * the launch shape: kHitWaves waves to a workgroup, a wave per UNIT -- a query, or a step of 64 items --, the units dealt over
//    a grid of what the chip holds at once (QueryGrid, FirstWaveUnit / GridWaves, LaunchQuery);
//  * the item head: what a lane reads of the item it looks at (LoadItemHead, ItemTransparent);
//  * the D13 predicates the later decisions reuse (HitWinding, HitStroke, HitCircle) and the finiteness tests;
//  * ForItemChunks: a candidate's chunks spread over the lanes; TakeLowestLane: the next candidate of a step.
// The item walks themselves -- topmost first (pm_hit_kernel, pm_hit_rects_kernel, the stack kernels), every candidate of every step (pm_snap_kernel,
// pm_cross_kernel), a word per item with the steps dealt over the grid (pm_select_rect_kernel, pm_select_polygon_kernel) -- are
// written out in the kernels over these pieces.  As templates over lambdas they were measured: every kernel that took one paid
// two to four VGPRs, and pm_hit_rects_kernel, pm_cross_kernel and pm_select_polygon_kernel 1 .. 3 % of their time.
#pragma once

#include "pm_kernels_common.h"

namespace pm {

// The resident scene and its index, and the call's flags
struct SceneView {
    const uint8_t *scene;
    uint32_t n_items, items_ix, bbox_ix;  // the drawn group, as in FrameParams
    const uint32_t *chunk_base;
    const float4 *chunk_bbox;
    const float4 *sup_bbox;
    uint32_t flags;                       // PM_HIT_* (and the call's own: PM_SNAP_*)
};

namespace {

constexpr int kHitWaves = 4;
constexpr int kHitThreads = 64 * kHitWaves;
// the kernels' copies of the public constants: pm_context.hip asserts that they are include/piet_metal_amd.h's
constexpr uint32_t kHitNone = 0xffffffffu;         // PM_HIT_NONE
constexpr uint32_t kHitSkipTransparent = 1u;       // PM_HIT_SKIP_TRANSPARENT
constexpr uint32_t kSelTouches = 1u;               // PM_SEL_TOUCHES
constexpr uint32_t kSelEncloses = 2u;              // PM_SEL_ENCLOSES

// ---- the launch shape ---------------------------------------------------------------------------------------------------------
// grid: what the chip holds at once (eight workgroups of four waves per CU), or a wave per unit if that is less
inline uint32_t QueryGrid(uint32_t n_units, uint32_t n_cus) { return min((n_units + kHitWaves - 1u) / kHitWaves, max(n_cus, 1u) * 8u); }

// the steps of 64 items of a scene
__host__ __device__ __forceinline__ uint32_t ItemSteps(uint32_t n_items) { return (n_items + 63u) / 64u; }

template <typename Params>
void LaunchQuery(void (*kernel)(Params), const Params &p, uint32_t n_units, uint32_t n_cus, hipStream_t stream) {
    if (n_units == 0u) return;
    hipLaunchKernelGGL(kernel, dim3(QueryGrid(n_units, n_cus)), dim3(kHitThreads), 0, stream, p);
}

// The units [0, n_units) dealt over the waves of a QueryGrid: for (u = FirstWaveUnit(); u < n_units; u += GridWaves()), u wave-uniform.
__device__ __forceinline__ uint32_t GridWaves() { return gridDim.x * kHitWaves; }
__device__ __forceinline__ uint32_t FirstWaveUnit() { return blockIdx.x * kHitWaves + WaveId(); }

// The bits of an f32 of the query, which every lane loaded alike, in a scalar register.  (It takes the bits, not the float or its
// address: with either of those the compiler tests finiteness on the vector copy and every kernel pays two to four VGPRs.)
__device__ __forceinline__ uint32_t UniformF32Bits(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }

__device__ __forceinline__ bool RectFiniteBits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool RectFinite(float2 p) { return RectFiniteBits(__float_as_uint(p.x)) && RectFiniteBits(__float_as_uint(p.y)); }

// ---- the item head ------------------------------------------------------------------------------------------------------------
// Item `item`: its record, the record's first word and tag, and its ShortBbox (which saturates at 0 and 65 535)
struct ItemHead {
    uint32_t item;
    const uint8_t *it;
    uint32_t w0, tag;
    uint32_t x0, y0, x1, y1;
};

__device__ __forceinline__ ItemHead LoadItemHead(const SceneView &V, uint32_t item) {
    ItemHead h;
    h.item = item;
    h.it = V.scene + V.items_ix + static_cast<size_t>(item) * kItemSize;
    h.w0 = LoadU32(h.it);
    h.tag = h.w0 & 0xffffu;
    const uint2 bb = *reinterpret_cast<const uint2 *>(V.scene + V.bbox_ix + static_cast<size_t>(item) * sizeof(ShortBbox));
    h.x0 = bb.x & 0xffffu;
    h.y0 = bb.x >> 16;
    h.x1 = bb.y & 0xffffu;
    h.y1 = bb.y >> 16;
    return h;
}

// Has the colour of a Line, a Fill or a Polyline alpha 0 (what PM_HIT_SKIP_TRANSPARENT skips; a Circle has no colour of its own)
__device__ __forceinline__ bool ItemTransparent(const ItemHead &h) { return (LoadU32(h.it + (h.tag == kItemPoly ? 4 : 8)) >> 24) == 0u; }

// ---- D13's predicates ---------------------------------------------------------------------------------------------------------
// D13, Fill: what segment a -> b adds to the winding sum of (x, y)
__device__ __forceinline__ int HitWinding(float2 a, float2 b, double x, double y) {
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    const double s = (bx - ax) * (y - ay) - (x - ax) * (by - ay);
    int w = 0;
    if (ay <= y && y < by && s > 0.0) w = 1;
    if (by <= y && y < ay && s < 0.0) w = -1;
    return w;
}

// D13, Line and Polyline: is (x, y) within hw of segment a -> b (hw2 = hw * hw)
__device__ __forceinline__ bool HitStroke(float2 a, float2 b, double x, double y, double hw2) {
    const double ax = a.x, ay = a.y;
    const double abx = static_cast<double>(b.x) - ax, aby = static_cast<double>(b.y) - ay;
    const double apx = x - ax, apy = y - ay;
    const double L = abx * abx + aby * aby;
    double t = 0.0;
    if (L != 0.0) t = fmin(fmax((apx * abx + apy * aby) / L, 0.0), 1.0);
    const double cx = ax + abx * t, cy = ay + aby * t;
    const double dx = x - cx, dy = y - cy;
    return dx * dx + dy * dy <= hw2;
}

// D13, Circle / ellipse: from the item's ShortBbox alone
__device__ __forceinline__ bool HitCircle(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool ellipse, double x, double y) {
    const double fx0 = static_cast<double>(x0), fy0 = static_cast<double>(y0);
    const double cx = (fx0 + static_cast<double>(x1)) * 0.5, cy = (fy0 + static_cast<double>(y1)) * 0.5;
    const double rx = cx - fx0, ry = cy - fy0;
    const double dx = x - cx, dy = y - cy;
    if (ellipse) return rx > 0.0 && ry > 0.0 && (dx / rx) * (dx / rx) + (dy / ry) * (dy / ry) <= 1.0;
    const double r = fmin(rx, ry);
    return dx * dx + dy * dy <= r * r;
}

// ---- a candidate's chunks -----------------------------------------------------------------------------------------------------
// The chunks [cb0, cb1) of one item, spread over the lanes: work(c) runs on ONE lane for every chunk c whose box passes
// (divergent: no cross-lane operation inside); after every round the uniform done() may end the walk.  Up to 64 chunks: one
// round, a chunk per lane.  More: the super-chunks that hold them are tested first, 64 per round, and the survivors are worked
// off eight at a time -- lane 8 r + u takes chunk u of the r-th surviving super-chunk (a super-chunk's box is the union of
// eight consecutive entries of the GLOBAL chunk table: chunks of the neighbouring items only make it larger).
template <typename Pass, typename Work, typename Done>
__device__ __forceinline__ void ForItemChunks(const SceneView &V, uint32_t cb0, uint32_t cb1, uint32_t lane, Pass &&pass, Work &&work, Done &&done) {
    if (cb1 - cb0 <= 64u) {
        const uint32_t c = cb0 + lane;
        if (c < cb1 && pass(V.chunk_bbox[c])) work(c);
        (void)done();
        return;
    }
    const uint32_t g1 = (cb1 - 1u) / kSuperChunks + 1u;
    for (uint32_t gb = cb0 / kSuperChunks; gb < g1; gb += 64u) {
        const uint32_t g = gb + lane;
        uint64_t m = __ballot(g < g1 && pass(V.sup_bbox[g < g1 ? g : gb]));
        while (m != 0ull) {
            uint64_t mine = m;  // ... with its r lowest bits cleared
            for (uint32_t k = 0; k < (lane >> 3); ++k) mine &= mine - 1ull;
            if (mine != 0ull) {
                const uint32_t c = (gb + static_cast<uint32_t>(__builtin_ctzll(mine))) * kSuperChunks + (lane & 7u);
                if (c >= cb0 && c < cb1 && pass(V.chunk_bbox[c])) work(c);
            }
            if (done()) return;
            for (uint32_t k = 0; k < 8u; ++k) m &= m - 1ull;
        }
    }
}

// ---- the item walks -----------------------------------------------------------------------------------------------------------
// The lowest set bit of a wave-uniform ballot as a scalar, taken out of it
__device__ __forceinline__ uint32_t TakeLowestLane(uint64_t &m) {
    const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(__builtin_ctzll(m)));
    m &= m - 1ull;
    return l;
}

}  // namespace
}  // namespace pm
