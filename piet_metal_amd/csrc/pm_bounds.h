// pm_item_bounds_kernel, pm_union_bounds_kernel: bounds queries -- the bounding box of every item of the resident scene, and the
// union of the boxes of the items that carry a label (a group, a selection) with how many there are.  Not on the frame path: like
// the other query kernels they read the scene and the scene index, nothing a frame writes.  Included by pm_context.hip; the
// item head, the constants and the launch shape of pm_select_rect_kernel (a wave per step of 64 items: FirstWaveUnit / GridWaves) are
// pm_query_common.h's, as they are.  The walks there put lane 0 at the TOPMOST item of a step; here lane l has item 64 step + l, so that
// a run of equal labels is a run of lanes, and the step keeps its own body.
//
// What the bounds of an item are is decision D22: binary64 values of the scene's f32 / u16 values, one rounding per
// written operation (-ffp-contract=off) -- tests/np_bounds.py states the same in numpy from the points alone and the records must
// agree byte for byte.  A minimum and a maximum are exact, and the decision ends with `+ 0.0` on every value, so nothing of the
// order of evaluation can show.
//
// Both kernels deal the items 64 per step over the waves of the grid, a lane per item, lane l item 64 step + l (BoundsOfStep):
//  * a Circle and a Line are evaluated on their lane from the item record;
//  * a plain Fill and a Polyline of two points or more take the union of their CHUNK boxes (pm_index_kernel: the exact f32 minimum
//    and maximum of the chunk's points, NaNs ignored per coordinate) -- 16 bytes per four segments instead of the points.  Every
//    point of such an item is in one of its chunks; `-+ hw` is applied once at the end: rounding is monotonic, min (p.x - hw) is
//    (min p.x) - hw;
//  * the index seeds a box with +-3.0e38f.  A coordinate of a chunk whose low edge is above its high edge met no value (a chunk of
//    NaNs keeps the seed on that axis): it adds nothing.  Within the coordinate bound of DESIGN.md 9 (|v| <= 3.0e38) a value the
//    chunk did meet always gives low <= high, and the seed is the identity.  Beyond the bound the box is whatever the index holds;
//  * a COMPOUND Fill walks its points: a chunk box of the index also holds the closing ends of its segments, and a separator whose
//    closing index names another separator would add that entry's index bits as a y.  The points are D22's own set;
//  * a one-point Polyline owns no chunk (PolySegs(1) == 0): its point is read from the point array.
// An item of up to kBoundsLane chunks (or points) is finished by its lane; a longer one by the whole wave, 64 entries per step and
// six butterfly steps, one item after the other.
//
// pm_union_bounds_kernel then reduces runs of consecutive lanes with the same label (groups are runs of consecutive items) by a
// segmented scan over the wave, and the last lane of every run combines the run into the label's record: 64-bit integer atomic
// min / max on an order-preserving key of the double's bits, and one 64-bit atomic add for the two u32 counts, which are neighbours
// (reading a key first and leaving out an atomic that could change nothing was measured: no gain with one label, a loss with many).
// pm_bounds_init_kernel writes the identity's keys before, pm_bounds_final_kernel turns the keys into doubles (and adds 0.0) behind, both in the caller's array:
// the record pm_label_bounds is its own accumulator.  No float atomics, no wave waits for another, no LDS, no scratch.
#pragma once

#include "pm_query_common.h"

namespace pm {

// One launch of either kernel
struct BoundsParams {
    SceneView V;
    const uint32_t *item_words;     // union: [n_items] the item takes part iff word & word_mask (nullptr: every item)
    const uint32_t *label_of_item;  // union: [n_items] (nullptr: every item has label 0)
    uint32_t word_mask, n_labels;
    uint8_t *out;                   // items: [32 n_items] pm_bounds; union: [40 n_labels] pm_label_bounds
};

namespace {

constexpr uint32_t kBoundsLane = 16u;          // entries a lane works off alone
constexpr uint32_t kBoundsNoLabel = 0xffffffffu;

// A box in binary64; the empty box is the identity of the union
struct BoundsBox {
    double x0 = __builtin_inf(), y0 = __builtin_inf(), x1 = -__builtin_inf(), y1 = -__builtin_inf();
};

// The exact minimum and maximum of f32 values, a NaN ignored per coordinate
struct BoundsAcc {
    float x0 = __builtin_inff(), y0 = __builtin_inff(), x1 = -__builtin_inff(), y1 = -__builtin_inff();
};

__device__ __forceinline__ void BoundsAddPoint(BoundsAcc &a, float2 p) {
    a.x0 = fminf(a.x0, p.x);
    a.y0 = fminf(a.y0, p.y);
    a.x1 = fmaxf(a.x1, p.x);
    a.y1 = fmaxf(a.y1, p.y);
}

// A chunk box of the index: an axis that still holds the seed met no value
__device__ __forceinline__ void BoundsAddChunk(BoundsAcc &a, float4 bb) {
    if (bb.x <= bb.z) {
        a.x0 = fminf(a.x0, bb.x);
        a.x1 = fmaxf(a.x1, bb.z);
    }
    if (bb.y <= bb.w) {
        a.y0 = fminf(a.y0, bb.y);
        a.y1 = fmaxf(a.y1, bb.w);
    }
}

// Where an item's values are: n chunk boxes from `first` on (chunks = true), or n entries of a point array
struct BoundsSource {
    const uint8_t *pts = nullptr;
    uint32_t first = 0u, n = 0u;
    bool chunks = false, compound = false;
};

__device__ __forceinline__ void BoundsAddEntry(const SceneView &V, const BoundsSource &S, uint32_t e, BoundsAcc &a) {
    if (S.chunks) {
        BoundsAddChunk(a, V.chunk_bbox[S.first + e]);
    } else {
        const float2 p = LoadF2(S.pts + static_cast<size_t>(e) * 8);
        if (!(S.compound && p.x != p.x)) BoundsAddPoint(a, p);   // (a separator is no point)
    }
}

// The source of a Fill or a Polyline
__device__ __forceinline__ BoundsSource BoundsSourceOf(const SceneView &V, const ItemHead &h) {
    BoundsSource S;
    const uint32_t i = h.item, tag = h.tag;
    const uint32_t npt = LoadU32(h.it + 12);
    S.pts = V.scene + LoadU32(h.it + 16);
    S.compound = tag == kItemFill && (LoadU32(h.it + 4) & kFillCompound) != 0u;
    S.n = npt;
    if (!S.compound && npt != 0u && !(tag == kItemPoly && npt == 1u)) {
        S.chunks = true;   // (at least one: FillSegs(npt) >= 1, PolySegs(npt) >= 1)
        S.first = V.chunk_base[i];
        S.n = V.chunk_base[i + 1u] - S.first;
    }
    return S;
}

// D22's last two steps: -+ hw once (hw = 0 for a Fill), a NaN -- an infinity against an infinite hw -- ignored, and + 0.0
__device__ __forceinline__ BoundsBox BoundsFinish(const BoundsAcc &a, double hw) {
    BoundsBox b;
    b.x0 = fmin(b.x0, static_cast<double>(a.x0) - hw) + 0.0;
    b.y0 = fmin(b.y0, static_cast<double>(a.y0) - hw) + 0.0;
    b.x1 = fmax(b.x1, static_cast<double>(a.x1) + hw) + 0.0;
    b.y1 = fmax(b.y1, static_cast<double>(a.y1) + hw) + 0.0;
    return b;
}

// D22, Circle / ellipse, from the item's ShortBbox alone
__device__ __forceinline__ BoundsBox BoundsCircle(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool ellipse) {
    const double fx0 = static_cast<double>(x0), fy0 = static_cast<double>(y0);
    const double cx = (fx0 + static_cast<double>(x1)) * 0.5, cy = (fy0 + static_cast<double>(y1)) * 0.5;
    double rx = cx - fx0, ry = cy - fy0;
    BoundsBox b;
    if (ellipse) {
        if (!(rx > 0.0 && ry > 0.0)) return b;
    } else {
        rx = ry = fmin(rx, ry);
    }
    b.x0 = (cx - rx) + 0.0;
    b.y0 = (cy - ry) + 0.0;
    b.x1 = (cx + rx) + 0.0;
    b.y1 = (cy + ry) + 0.0;
    return b;
}

// The wave's union of the lanes' accumulators, in every lane
__device__ __forceinline__ void BoundsWaveUnion(BoundsAcc &a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.x0 = fminf(a.x0, __shfl_xor(a.x0, d, 64));
        a.y0 = fminf(a.y0, __shfl_xor(a.y0, d, 64));
        a.x1 = fmaxf(a.x1, __shfl_xor(a.x1, d, 64));
        a.y1 = fmaxf(a.y1, __shfl_xor(a.y1, d, 64));
    }
}

// The D22 box of item 64 step + lane (mine: there is such an item), and whether the flags skip it.  Called by the whole wave.
__device__ __forceinline__ BoundsBox BoundsOfStep(const SceneView &V, uint32_t step, uint32_t lane, bool mine, bool &skipped) {
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const uint32_t i = step * 64u + lane;
    BoundsBox box;
    BoundsAcc acc;
    double hw = 0.0;
    bool points = false, big = false;
    skipped = false;
    if (mine) {
        const ItemHead h = LoadItemHead(V, i);
        if (h.tag == kItemCircle) {
            box = BoundsCircle(h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0);
        } else if (h.tag == kItemLine) {
            skipped = skip && ItemTransparent(h);
            hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(h.it + 12)));
            if (!skipped && hw == hw) {
                BoundsAddPoint(acc, LoadF2(h.it + 16));
                BoundsAddPoint(acc, LoadF2(h.it + 24));
                points = true;
            }
        } else if (h.tag == kItemFill || h.tag == kItemPoly) {
            skipped = skip && ItemTransparent(h);
            if (h.tag == kItemPoly) hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(h.it + 8)));
            if (!skipped && hw == hw) {
                const BoundsSource S = BoundsSourceOf(V, h);
                points = true;
                big = S.n > kBoundsLane;
                if (!big)
                    for (uint32_t e = 0; e < S.n; ++e) BoundsAddEntry(V, S, e, acc);
            }
        }
    }
    uint64_t m = __ballot(big);
    while (m != 0ull) {   // the long items of the step, one after the other, by the whole wave
        const uint32_t l = TakeLowestLane(m);
        const BoundsSource S = BoundsSourceOf(V, LoadItemHead(V, step * 64u + l));
        BoundsAcc part;
        for (uint32_t e = lane; e < S.n; e += 64u) BoundsAddEntry(V, S, e, part);
        BoundsWaveUnion(part);
        if (lane == l) acc = part;
    }
    if (points) box = BoundsFinish(acc, hw);
    return box;
}

// An order-preserving map of a double's bits onto unsigned integers (no NaN reaches it), and back
__device__ __forceinline__ unsigned long long BoundsKey(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    return (b >> 63) != 0ull ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double BoundsUnkey(unsigned long long k) {
    return __builtin_bit_cast(double, (k >> 63) != 0ull ? k & 0x7fffffffffffffffull : ~k);
}

// v of lane src (src < 64)
__device__ __forceinline__ double BoundsShfl(double v, int src) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const uint32_t lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(b)), src, 64));
    const uint32_t hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(b >> 32)), src, 64));
    return __builtin_bit_cast(double, (static_cast<unsigned long long>(hi) << 32) | lo);
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_item_bounds_kernel(BoundsParams B) {
    const SceneView &V = B.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves(), n_steps = ItemSteps(V.n_items);
    for (uint32_t step = FirstWaveUnit(); step < n_steps; step += n_waves) {
        const uint32_t i = step * 64u + lane;
        const bool mine = i < V.n_items;
        bool skipped;
        const BoundsBox b = BoundsOfStep(V, step, lane, mine, skipped);
        if (mine) {
            double *rec = reinterpret_cast<double *>(B.out + static_cast<size_t>(i) * 32);   // (8-byte aligned)
            rec[0] = b.x0;
            rec[1] = b.y0;
            rec[2] = b.x1;
            rec[3] = b.y1;
        }
    }
}

// The identity in every label's record: the keys of the empty box and two zeros
__global__ __launch_bounds__(256) void pm_bounds_init_kernel(uint8_t *out, uint32_t n_labels) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    unsigned long long *k = reinterpret_cast<unsigned long long *>(out + static_cast<size_t>(l) * 40);
    k[0] = k[1] = BoundsKey(__builtin_inf());
    k[2] = k[3] = BoundsKey(-__builtin_inf());
    k[4] = 0ull;   // n_items, n_boxed
}

__global__ __launch_bounds__(kHitThreads) void pm_union_bounds_kernel(BoundsParams B) {
    const SceneView &V = B.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves(), n_steps = ItemSteps(V.n_items);
    for (uint32_t step = FirstWaveUnit(); step < n_steps; step += n_waves) {
        const uint32_t i = step * 64u + lane;
        const bool mine = i < V.n_items;
        bool skipped;
        BoundsBox b = BoundsOfStep(V, step, lane, mine, skipped);
        uint32_t label = kBoundsNoLabel;
        if (mine && !skipped && (B.item_words == nullptr || (B.item_words[i] & B.word_mask) != 0u)) {
            label = B.label_of_item != nullptr ? B.label_of_item[i] : 0u;
            if (label >= B.n_labels) label = kBoundsNoLabel;
        }
        const bool part = label != kBoundsNoLabel;
        if (!part) b = BoundsBox();
        uint32_t cnt = part ? 1u : 0u, boxed = part && b.x0 <= b.x1 && b.y0 <= b.y1 ? 1u : 0u;
        // runs of equal labels: a lane begins one if its left neighbour's label differs
        const uint32_t left = static_cast<uint32_t>(__shfl(static_cast<int>(label), static_cast<int>(lane == 0u ? 0u : lane - 1u), 64));
        const uint64_t heads = __ballot(lane == 0u || left != label);
        const uint32_t start = 63u - static_cast<uint32_t>(__builtin_clzll(heads & (~0ull >> (63u - lane))));
        // inclusive scan within the run: its last lane ends with the run's union and counts
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const int src = static_cast<int>(lane >= d ? lane - d : 0u);
            const double ox0 = BoundsShfl(b.x0, src), oy0 = BoundsShfl(b.y0, src), ox1 = BoundsShfl(b.x1, src), oy1 = BoundsShfl(b.y1, src);
            const uint32_t oc = static_cast<uint32_t>(__shfl(static_cast<int>(cnt | (boxed << 16)), src, 64));
            if (lane >= d && lane - d >= start) {
                b.x0 = fmin(b.x0, ox0);
                b.y0 = fmin(b.y0, oy0);
                b.x1 = fmax(b.x1, ox1);
                b.y1 = fmax(b.y1, oy1);
                cnt += oc & 0xffffu;
                boxed += oc >> 16;
            }
        }
        const bool tail = lane == 63u || (((heads >> 1) >> lane) & 1ull) != 0ull;
        if (tail && part) {
            uint8_t *rec = B.out + static_cast<size_t>(label) * 40;
            unsigned long long *k = reinterpret_cast<unsigned long long *>(rec);
            (void)__hip_atomic_fetch_min(k + 0, BoundsKey(b.x0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_min(k + 1, BoundsKey(b.y0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_max(k + 2, BoundsKey(b.x1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_max(k + 3, BoundsKey(b.y1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // n_items and n_boxed are neighbours, 8-byte aligned: one add for both (neither can carry: there are < 2^32 items)
            (void)__hip_atomic_fetch_add(k + 4, static_cast<unsigned long long>(cnt) | (static_cast<unsigned long long>(boxed) << 32), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Keys back into doubles, `+ 0.0` on each (a union that is a zero is +0, whichever item's zero won)
__global__ __launch_bounds__(256) void pm_bounds_final_kernel(uint8_t *out, uint32_t n_labels) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_labels) return;
    unsigned long long *k = reinterpret_cast<unsigned long long *>(out + static_cast<size_t>(l) * 40);
    double *v = reinterpret_cast<double *>(k);
    const double x0 = BoundsUnkey(k[0]) + 0.0, y0 = BoundsUnkey(k[1]) + 0.0, x1 = BoundsUnkey(k[2]) + 0.0, y1 = BoundsUnkey(k[3]) + 0.0;
    v[0] = x0;
    v[1] = y0;
    v[2] = x1;
    v[3] = y1;
}

void LaunchItemBounds(const BoundsParams &p, uint32_t n_cus, hipStream_t stream) {
    LaunchQuery(pm_item_bounds_kernel, p, ItemSteps(p.V.n_items), n_cus, stream);
}

// the three launches of a union: all n_labels records are written, also of a scene without items
void LaunchUnionBounds(const BoundsParams &p, uint32_t n_cus, hipStream_t stream) {
    const uint32_t label_grid = (p.n_labels - 1u) / 256u + 1u;   // (n_labels >= 1)
    hipLaunchKernelGGL(pm_bounds_init_kernel, dim3(label_grid), dim3(256), 0, stream, p.out, p.n_labels);
    LaunchQuery(pm_union_bounds_kernel, p, ItemSteps(p.V.n_items), n_cus, stream);
    hipLaunchKernelGGL(pm_bounds_final_kernel, dim3(label_grid), dim3(256), 0, stream, p.out, p.n_labels);
}

}  // namespace pm
