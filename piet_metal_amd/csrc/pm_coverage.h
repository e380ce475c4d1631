// pm_item_coverage_kernel: coverage counts -- for every item of the resident scene how many pixels of a rectangle it covers, on how
// many of them it can be seen, on how many it is the topmost item, and one pixel where it can be seen.  Decision D28, a
// definition by reference: "covers" is D13 at the pixel's centre, as pm_hit_frame_kernel evaluates it (D18), "opaque" is D24's
// (ItemOpaque, pm_hit_stack.h).  Not on the frame path; included by pm_context.hip, whose unit it is compiled in.  (The kernel is not
// called pm_coverage_kernel: pm_fine.hip has a validation kernel of that name, behind pm_fill_coverage.)
//
// The walk is pm_hit_frame_kernel's, from its own pieces as they are (FrameTile, the box predicates, ForTileChunks, BlockRank): one
// WORKGROUP of 256 threads per 16 x 16 tile, a thread per pixel, the items from the top of paint order down kFrameItems per step,
// culled against the tile's extent, the survivors compacted into LDS and evaluated one after the other by every thread for its own
// pixel.  What differs is what becomes of a hit.  A thread keeps two bits, `had` (a hit so far: the next one is not the top) and
// `occluded` (a hit on an opaque item so far: the next one cannot be seen).  Per survivor each wave turns three ballots -- hit, hit
// and not occluded, hit and not had -- into three popcounts, and the lowest set lane of the second into the wave's smallest pixel
// index j w + i (a wave's lanes are four rows of the tile, in (j, i) order).  Lane 0 adds them to the survivor's row of an LDS table,
// s_acc[rank in the step][4].  When the step's survivors are worked off, and a barrier, thread r takes row r: the non-zero words go to
// item s_cand[r]'s record with device-scope relaxed atomics -- add, add, add, min -- and the row is left cleared by the thread that
// read it.  At most one flush per (tile, surviving item), spread over the workgroup.
//
// Every word is an integer sum or minimum over pixels: no order of tiles, waves or atomics shows in the bytes.  The record must hold
// {0, 0, 0, PM_HIT_NONE} before the launch (pm_coverage_init_kernel, on the same stream in front of it).
//
// What keeps the table right:
//  * a thread outside the rectangle (a partial tile) is never live: it is in no ballot;
//  * a row is written between the barrier behind the step's compaction and the barrier behind its last survivor, and read and cleared
//    by ONE thread behind that barrier; the next step's (or tile's) first write to it is behind BlockRank's two barriers.  The rows
//    are cleared once before the first step.  A step of 256 survivors uses every row, thread 255 flushes the last;
//  * under PM_COVERAGE_VISIBLE_ONLY a thread is live until it is occluded, so every hit it counts can be seen (covered := visible),
//    and the walk of a tile ends when no thread of it is live -- pm_hit_frame_kernel's s_live look, "answered" replaced by "occluded".
//    The look breaks out of the survivors' loop only: the barrier and the flush behind it run for the step that is left.
#pragma once

#include "pm_hit_frame.h"
#include "pm_hit_stack.h"

namespace pm {

// One launch of pm_item_coverage_kernel: the w x h pixels from (x0, y0) against the resident scene and its index.
struct CoverageParams {
    SceneView V;          // flags: PM_HIT_SKIP_TRANSPARENT, PM_COVERAGE_VISIBLE_ONLY
    uint32_t *out;        // [n_items][4] {covered, visible, top, first_visible}, initialised
    uint32_t x0, y0, w, h;   // x0 + w <= 65 536, y0 + h <= 65 536, w h < 2^32
    uint32_t tiles_x, n_tiles;
};

namespace {

// the kernel's copy of the public constant: pm_context.hip asserts that it is include/piet_metal_amd.h's
constexpr uint32_t kCoverageVisibleOnly = 16u;   // PM_COVERAGE_VISIBLE_ONLY
constexpr uint32_t kCoverageWords = 4;           // words of a record

}  // namespace

// {0, 0, 0, PM_HIT_NONE} for n_items records, a word per thread (the buffer is aligned to 4 bytes, no more)
__global__ __launch_bounds__(kHitThreads) void pm_coverage_init_kernel(uint32_t *out, uint32_t n_items) {
    const size_t n = static_cast<size_t>(n_items) * kCoverageWords;
    for (size_t i = static_cast<size_t>(blockIdx.x) * kHitThreads + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kHitThreads)
        out[i] = (i % kCoverageWords) == 3u ? kHitNone : 0u;
}

__global__ __launch_bounds__(kFrameThreads) void pm_item_coverage_kernel(CoverageParams P) {
    __shared__ uint32_t s_cand[kFrameItems];    // the step's surviving items, topmost first
    __shared__ uint32_t s_sup[kFrameChunks];    // a round's surviving super-chunks
    __shared__ uint32_t s_chunk[kFrameChunks];  // a round's surviving chunks
    __shared__ uint32_t s_part[kFrameWaves];    // BlockRank's
    __shared__ uint32_t s_live[2][kFrameWaves]; // waves with a live pixel, two generations (one barrier per look)
    __shared__ uint32_t s_acc[kFrameItems * kCoverageWords];   // the step's survivors' {covered, visible, top, first_visible} in this tile
    const SceneView &V = P.V;
    const uint32_t t = threadIdx.x;
    const uint32_t wave = t >> 6;
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const bool visible_only = (V.flags & kCoverageVisibleOnly) != 0;
#pragma unroll
    for (uint32_t k = 0; k < kCoverageWords; ++k) s_acc[t * kCoverageWords + k] = k == 3u ? kHitNone : 0u;   // (behind it: the first step's barriers)
    for (uint32_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const uint32_t ox = (tile % P.tiles_x) * kFrameTile, oy = (tile / P.tiles_x) * kFrameTile;   // in the rectangle
        const uint32_t ix = ox + (t % kFrameTile), iy = oy + (t / kFrameTile);
        const bool inside = ix < P.w && iy < P.h;   // (a partial tile's other threads count nothing and keep no walk alive)
        FrameTile T;
        T.xmin = static_cast<double>(P.x0 + ox) + 0.5;
        T.ymin = static_cast<double>(P.y0 + oy) + 0.5;
        T.xmax = static_cast<double>(P.x0 + min(ox + kFrameTile, P.w) - 1u) + 0.5;
        T.ymax = static_cast<double>(P.y0 + min(oy + kFrameTile, P.h) - 1u) + 0.5;
        T.x = static_cast<double>(P.x0 + ix) + 0.5;
        T.y = static_cast<double>(P.y0 + iy) + 0.5;
        T.live = inside;
        bool had = false, occluded = false;
        uint32_t looks = 0;
        bool tile_done = false;
        for (uint32_t hi = V.n_items; hi != 0u && !tile_done; hi = hi > kFrameItems ? hi - kFrameItems : 0u) {
            // thread 0 looks at the topmost item of the step; the cull is pm_hit_frame_kernel's
            bool keep = false;
            const uint32_t mine = hi - 1u - t;
            if (t < hi) {
                const ItemHead h = LoadItemHead(V, mine);
                const uint32_t tag = h.tag, x0 = h.x0, y0 = h.y0, x1 = h.x1, y1 = h.y1;
                if (tag == kItemCircle) {  // the box IS the shape: no edge of it is "saturated"
                    keep = !(T.ymax < static_cast<double>(y0) || T.ymin > static_cast<double>(y1) || T.xmax < static_cast<double>(x0) ||
                             T.xmin > static_cast<double>(x1));
                } else {
                    // the box as bounds in binary64: an edge at a saturated value bounds nothing
                    const bool above = y0 != 0u && T.ymax < static_cast<double>(y0), below = y1 != 0xffffu && T.ymin > static_cast<double>(y1);
                    const bool left = x0 != 0u && T.xmax < static_cast<double>(x0), right = x1 != 0xffffu && T.xmin > static_cast<double>(x1);
                    if (tag == kItemLine) {
                        keep = !(skip && ItemTransparent(h));
                    } else if (tag == kItemFill) {
                        keep = !(above || below || right) && !(skip && ItemTransparent(h));
                    } else if (tag == kItemPoly) {
                        keep = !(above || below || left || right) && !(skip && ItemTransparent(h));
                    }
                }
            }
            uint32_t n_cand = 0;
            const uint32_t rank = BlockRank<kFrameWaves>(keep, s_part, &n_cand);
            if (keep) s_cand[rank] = mine;
            LdsBarrier();
            n_cand = Uniform(n_cand);
            for (uint32_t k = 0; k < n_cand; ++k) {
                if (visible_only) {  // is any pixel of the tile not yet occluded (only those inside the rectangle ever were live)
                    const uint64_t m = __ballot(T.live);
                    if (LaneId() == 0u) s_live[looks & 1u][wave] = m != 0ull ? 1u : 0u;
                    LdsBarrier();
                    uint32_t any = 0;
#pragma unroll
                    for (int w = 0; w < kFrameWaves; ++w) any |= s_live[looks & 1u][w];
                    looks += 1u;
                    if (Uniform(any) == 0u) {
                        tile_done = true;
                        break;   // (to the step's barrier and flush)
                    }
                }
                const uint32_t i = Uniform(s_cand[k]);
                const ItemHead h = LoadItemHead(V, i);
                const uint8_t *it = h.it;
                const uint32_t tag = h.tag;
                bool hit = false;
                if (tag == kItemCircle) {
                    if (T.live) hit = HitCircle(h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0, T.x, T.y);
                } else if (tag == kItemLine) {
                    if (T.live) {
                        const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 12)));
                        hit = HitStroke(LoadF2(it + 16), LoadF2(it + 24), T.x, T.y, hw * hw);
                    }
                } else if (tag == kItemFill) {
                    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
                    const uint8_t *pts = V.scene + LoadU32(it + 16);
                    const bool compound = (flags & kFillCompound) != 0;
                    const uint32_t cb0 = V.chunk_base[i], cb1 = V.chunk_base[i + 1];
                    int wsum = 0;
                    ForTileChunks(
                        V, cb0, cb1, t, s_part, s_sup, s_chunk, [&](float4 bb) { return FrameFillBoxTile(bb, T); },
                        [&](uint32_t c) {
                            if (!(T.live && FrameFillBoxOwn(V.chunk_bbox[c], T))) return;
                            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
                            for (uint32_t s = k0; s < k1; ++s) {
                                float2 a, b;
                                if (FillSegmentEnds(pts, npt, compound, s, a, b)) wsum += HitWinding(a, b, T.x, T.y);
                            }
                        });
                    hit = (flags & kFillEvenOdd) ? (wsum & 1) != 0 : wsum != 0;
                } else if (tag == kItemPoly) {
                    const uint32_t npt = LoadU32(it + 12);
                    const uint8_t *pts = V.scene + LoadU32(it + 16);
                    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 8)));
                    const double hw2 = hw * hw;
                    if (npt == 1u) {  // one degenerate segment (the scene index has no chunk for it)
                        const float2 a = LoadF2(pts);
                        hit = T.live && HitStroke(a, a, T.x, T.y, hw2);
                    } else if (npt != 0u) {
                        const uint32_t cb0 = V.chunk_base[i], cb1 = V.chunk_base[i + 1];
                        ForTileChunks(
                            V, cb0, cb1, t, s_part, s_sup, s_chunk, [&](float4 bb) { return FramePolyBoxTile(bb, hw, T); },
                            [&](uint32_t c) {
                                if (hit || !(T.live && FramePolyBoxOwn(V.chunk_bbox[c], hw, T))) return;
                                const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
                                float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
                                for (uint32_t s = k0; s < k1; ++s) {
                                    const float2 b = LoadF2(pts + static_cast<size_t>(s + 1u) * 8);
                                    hit = hit || HitStroke(a, b, T.x, T.y, hw2);
                                    a = b;
                                }
                            });
                    }
                }
                // the wave's part of survivor k's row: three popcounts and the first lane that sees the item
                hit = hit && T.live;
                const uint64_t mc = __ballot(hit), mv = __ballot(hit && !occluded), mt = __ballot(hit && !had);
                if (LaneId() == 0u && mc != 0ull) {
                    uint32_t *row = s_acc + k * kCoverageWords;
                    (void)__hip_atomic_fetch_add(row + 0, static_cast<uint32_t>(__popcll(mc)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (mv != 0ull) {
                        const uint32_t first = wave * 64u + static_cast<uint32_t>(__builtin_ctzll(mv));   // as a thread of the tile
                        const uint32_t at = (oy + first / kFrameTile) * P.w + ox + first % kFrameTile;    // (inside: below w h)
                        (void)__hip_atomic_fetch_add(row + 1, static_cast<uint32_t>(__popcll(mv)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        (void)__hip_atomic_fetch_min(row + 3, at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    if (mt != 0ull) (void)__hip_atomic_fetch_add(row + 2, static_cast<uint32_t>(__popcll(mt)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                if (hit) {
                    had = true;
                    if (ItemOpaque(h)) {
                        occluded = true;
                        if (visible_only) T.live = false;
                    }
                }
            }
            LdsBarrier();   // every wave's part of every row is in
            if (t < n_cand) {
                uint32_t *row = s_acc + t * kCoverageWords;
                const uint32_t covered = row[0], visible = row[1], top = row[2], first = row[3];
                if (covered != 0u) {
                    uint32_t *rec = P.out + static_cast<size_t>(s_cand[t]) * kCoverageWords;
                    (void)__hip_atomic_fetch_add(rec + 0, covered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (visible != 0u) {
                        (void)__hip_atomic_fetch_add(rec + 1, visible, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        (void)__hip_atomic_fetch_min(rec + 3, first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (top != 0u) (void)__hip_atomic_fetch_add(rec + 2, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    row[0] = 0u;   // (the row's next writer is behind the next step's BlockRank)
                    row[1] = 0u;
                    row[2] = 0u;
                    row[3] = kHitNone;
                }
            }
        }
    }
}

// init: a word per thread; the walk: the grid LaunchHitFrame takes -- what the chip holds at once (eight workgroups of four waves per
// CU), or a workgroup per tile if that is less.  An empty rectangle leaves the initialised records as they are.
void LaunchItemCoverage(CoverageParams p, uint32_t n_cus, hipStream_t stream) {
    if (p.V.n_items == 0u) return;
    const size_t words = static_cast<size_t>(p.V.n_items) * kCoverageWords;
    const uint32_t init_grid = static_cast<uint32_t>(std::min<size_t>((words + kHitThreads - 1u) / kHitThreads, static_cast<size_t>(max(n_cus, 1u)) * 8u));
    hipLaunchKernelGGL(pm_coverage_init_kernel, dim3(init_grid), dim3(kHitThreads), 0, stream, p.out, p.V.n_items);
    if (p.w == 0u || p.h == 0u) return;
    p.tiles_x = (p.w + kFrameTile - 1u) / kFrameTile;
    p.n_tiles = p.tiles_x * ((p.h + kFrameTile - 1u) / kFrameTile);   // (at most 4096 x 4096)
    const uint32_t grid = min(p.n_tiles, max(n_cus, 1u) * 8u);
    hipLaunchKernelGGL(pm_item_coverage_kernel, dim3(grid), dim3(kFrameThreads), 0, stream, p);
}

}  // namespace pm
