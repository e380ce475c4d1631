// pm_item_lengths_kernel, pm_points_at_length_kernel, pm_positions_on_edges_kernel: path measurement -- how long every item of the
// resident scene is, where the point at a length along an item lies and which way the item runs there, and how far along an item a
// point of one of its edges is.  Not on the frame path: like the other query kernels they read the scene, nothing a frame writes
// (and not the scene index: every segment of an item has to be met).  Included by pm_context.hip; the item head, the constants and
// the launch shape are pm_query_common.h's, as they are.
//
// What a length is, which segment owns a position and what the point there is, is decision D25.  Lengths are D15's:
// unsigned 64-bit integers in units of 2^-16 px, a segment's the rounded binary64 length of b - a, capped at 2^32 -- sums of
// integers, so neither the deal of the segments over the lanes nor the order of a sum can show.  Everything else is binary64 on
// the scene's f32 values, one rounding per written operation (-ffp-contract=off); tests/np_measure.py states the same from the
// scene bytes and the records must agree byte for byte.  MeasureFix, MeasureScan and MeasurePoint restate SegFix, WaveScanQ and
// CutPoint of pm_dash.h, which work on path elements in the flatten unit, over the items every query addresses.
//
// The walk of an item is the run of its entry indices k, D21's edge names: a Line is a Polyline of the two points its record
// holds (one segment, k = 0), a Polyline has segment k from point k to point k + 1, a Fill every k for which FillSegmentEnds gives a
// segment, closing ones included.  A Circle, an ellipse, a Fill of no points and an item the flags skip have no walk.
//
//  * pm_item_lengths_kernel: the launch shape of pm_item_bounds_kernel, a wave per step of 64 items, lane l item 64 step + l.  An
//    item of up to kMeasureLane entries is summed by its lane, a longer one by the whole wave, the lanes striding over its entries,
//    and six butterfly steps;
//  * pm_points_at_length_kernel: a wave per query, ONE pass over the item's entries, 64 per step: q_k per lane, an inclusive scan of
//    the 64-bit integers in two halves with the carry of the steps before, a ballot of the lanes whose [Q_k, Q_k + q_k) holds s.
//    The wave leaves the walk at that step and the owning lane finishes the record.  The last segment of a length met so far is
//    kept in scalar registers: a walk that ends without an owner (s >= T) answers from it, without a second pass;
//  * pm_positions_on_edges_kernel: a wave per query, Q_index a strided sum of the q_j with j < index, lane 0 finishes the record.
// No atomics, no LDS, no scratch.
#pragma once

#include "pm_query_common.h"

namespace pm {

// One launch of any of the three kernels
struct MeasureParams {
    SceneView V;            // flags: PM_HIT_SKIP_TRANSPARENT
    const uint8_t *q;       // points: [16 n] pm_length_query; positions: [16 n] pm_edge_query; lengths: unused
    uint8_t *out;           // lengths: [16 n_items] pm_item_length; points: [32 n] pm_length_point; positions: [16 n] pm_length_at
    uint32_t n;
};

namespace {

constexpr uint32_t kMeasureNone = 0u;         // PM_MEASURE_NONE
constexpr uint32_t kMeasureOpen = 1u;         // PM_MEASURE_OPEN
constexpr uint32_t kMeasureClosed = 2u;       // PM_MEASURE_CLOSED
constexpr uint32_t kMeasureFound = 1u;        // PM_MEASURE_FOUND
constexpr uint32_t kMeasureClamped = 2u;      // PM_MEASURE_CLAMPED
constexpr uint32_t kMeasureDegenerate = 4u;   // PM_MEASURE_DEGENERATE
constexpr unsigned long long kMeasureCap = 1ull << 32;   // a segment longer than 65 536 px counts as that (D15)
constexpr uint32_t kMeasureLane = 16u;        // entries a lane sums alone

// The walk of an item: n_idx entry indices over `npt` entries at pts (kind kMeasureNone: none)
struct MeasureWalk {
    const uint8_t *pts = nullptr;
    uint32_t npt = 0u, n_idx = 0u, kind = kMeasureNone;
    bool compound = false;
};

__device__ __forceinline__ MeasureWalk MeasureWalkOf(const SceneView &V, uint32_t item) {
    MeasureWalk W;
    if (item >= V.n_items) return W;
    const ItemHead h = LoadItemHead(V, item);
    if (h.tag != kItemLine && h.tag != kItemFill && h.tag != kItemPoly) return W;
    if ((V.flags & kHitSkipTransparent) != 0u && ItemTransparent(h)) return W;
    if (h.tag == kItemLine) {   // (its two points are neighbours in the record)
        W.pts = h.it + 16;
        W.npt = 2u;
        W.n_idx = 1u;
        W.kind = kMeasureOpen;
        return W;
    }
    W.npt = LoadU32(h.it + 12);
    W.pts = V.scene + LoadU32(h.it + 16);
    if (h.tag == kItemPoly) {
        W.n_idx = PolySegs(W.npt);
        W.kind = kMeasureOpen;
    } else if (W.npt != 0u) {
        W.n_idx = FillSegs(W.npt);
        W.kind = kMeasureClosed;
        W.compound = (LoadU32(h.it + 4) & kFillCompound) != 0u;
    }
    return W;
}

// The ends of segment k (k < n_idx); false: entry k starts none (a separator)
__device__ __forceinline__ bool MeasureEnds(const MeasureWalk &W, uint32_t k, float2 &a, float2 &b) {
    if (W.kind == kMeasureOpen) {
        a = LoadF2(W.pts + static_cast<size_t>(k) * 8);
        b = LoadF2(W.pts + static_cast<size_t>(k + 1u) * 8);
        return true;
    }
    return FillSegmentEnds(W.pts, W.npt, W.compound, k, a, b);
}

// D15's q of a -> b: 0 if the length is a NaN, else min(floor(len * 65536 + 0.5), 2^32)
__device__ __forceinline__ unsigned long long MeasureFix(float2 a, float2 b) {
    const double dx = static_cast<double>(b.x) - static_cast<double>(a.x), dy = static_cast<double>(b.y) - static_cast<double>(a.y);
    const double len = sqrt(dx * dx + dy * dy);
    if (!(len == len)) return 0ull;
    const double f = floor(len * 65536.0 + 0.5);
    return f >= static_cast<double>(kMeasureCap) ? kMeasureCap : static_cast<unsigned long long>(f);
}

// q of segment k, 0 where there is none
__device__ __forceinline__ unsigned long long MeasureQ(const MeasureWalk &W, uint32_t k, bool &seg) {
    float2 a, b;
    seg = MeasureEnds(W, k, a, b);
    return seg ? MeasureFix(a, b) : 0ull;
}

// inclusive scan of the lanes' q (each <= 2^32) in two 32-bit halves: the low 24 bits and the rest, neither sum can carry out
__device__ __forceinline__ unsigned long long MeasureScan(unsigned long long q, uint32_t lane) {
    uint32_t lo = static_cast<uint32_t>(q & 0xffffffull), hi = static_cast<uint32_t>(q >> 24);
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t tl = __shfl_up(lo, d, 64), th = __shfl_up(hi, d, 64);
        if (lane >= d) {
            lo += tl;
            hi += th;
        }
    }
    return static_cast<unsigned long long>(lo) + (static_cast<unsigned long long>(hi) << 24);
}

// The wave's sum of the lanes' values, in every lane
__device__ __forceinline__ unsigned long long MeasureWaveSum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// v of lane src, wave-uniform
__device__ __forceinline__ uint32_t MeasureLane32(uint32_t v, uint32_t src) {
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(src)));
}
__device__ __forceinline__ unsigned long long MeasureLane64(unsigned long long v, uint32_t src) {
    return (static_cast<unsigned long long>(MeasureLane32(static_cast<uint32_t>(v >> 32), src)) << 32) | MeasureLane32(static_cast<uint32_t>(v), src);
}

// D25's point at s on a -> b, which owns [Q0, Q0 + q), q > 0: a's own values at s == Q0, else a + (b - a) * t
__device__ __forceinline__ void MeasurePoint(float2 a, float2 b, unsigned long long Q0, unsigned long long q, unsigned long long s, float &t, float &x, float &y) {
    if (s == Q0) {
        t = 0.0f;
        x = a.x;
        y = a.y;
        return;
    }
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    const double t64 = static_cast<double>(s - Q0) / static_cast<double>(q);
    t = static_cast<float>(t64);
    x = static_cast<float>(ax + (bx - ax) * t64);
    y = static_cast<float>(ay + (by - ay) * t64);
}

// D14's dir(a, b)
__device__ __forceinline__ void MeasureDir(float2 a, float2 b, float &tx, float &ty) {
    const double dx = static_cast<double>(b.x) - static_cast<double>(a.x), dy = static_cast<double>(b.y) - static_cast<double>(a.y);
    const double len = sqrt(dx * dx + dy * dy);
    tx = static_cast<float>(dx / len);
    ty = static_cast<float>(dy / len);
}

// A 32-byte pm_length_point / a 16-byte record, by ONE lane (8-byte aligned)
__device__ __forceinline__ void MeasureStore32(uint8_t *at, uint32_t item, uint32_t status, uint32_t index, float t, float x, float y, float tx, float ty) {
    uint2 *rec = reinterpret_cast<uint2 *>(at);
    rec[0] = make_uint2(item, status);
    rec[1] = make_uint2(index, __float_as_uint(t));
    rec[2] = make_uint2(__float_as_uint(x), __float_as_uint(y));
    rec[3] = make_uint2(__float_as_uint(tx), __float_as_uint(ty));
}
__device__ __forceinline__ void MeasureStore16(uint8_t *at, unsigned long long v, uint32_t w2, uint32_t w3) {
    uint2 *rec = reinterpret_cast<uint2 *>(at);
    rec[0] = make_uint2(static_cast<uint32_t>(v), static_cast<uint32_t>(v >> 32));
    rec[1] = make_uint2(w2, w3);
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_item_lengths_kernel(MeasureParams M) {
    const SceneView &V = M.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves(), n_steps = ItemSteps(V.n_items);
    for (uint32_t step = FirstWaveUnit(); step < n_steps; step += n_waves) {
        const uint32_t i = step * 64u + lane;
        const bool mine = i < V.n_items;
        const MeasureWalk W = MeasureWalkOf(V, mine ? i : kHitNone);
        unsigned long long len = 0ull;
        uint32_t segs = 0u;
        const bool big = W.n_idx > kMeasureLane;
        if (!big) {
            for (uint32_t k = 0; k < W.n_idx; ++k) {
                bool seg;
                len += MeasureQ(W, k, seg);
                segs += seg ? 1u : 0u;
            }
        }
        uint64_t m = __ballot(big);
        while (m != 0ull) {   // the long items of the step, one after the other, by the whole wave
            const uint32_t l = TakeLowestLane(m);
            const MeasureWalk L = MeasureWalkOf(V, step * 64u + l);
            unsigned long long part = 0ull;   // (the count rides in a sum of its own: a length may use all 64 bits)
            unsigned long long cnt = 0ull;
            for (uint32_t k = lane; k < L.n_idx; k += 64u) {
                bool seg;
                part += MeasureQ(L, k, seg);
                cnt += seg ? 1ull : 0ull;
            }
            part = MeasureWaveSum(part);
            cnt = MeasureWaveSum(cnt);
            if (lane == l) {
                len = part;
                segs = static_cast<uint32_t>(cnt);
            }
        }
        if (mine) MeasureStore16(M.out + static_cast<size_t>(i) * 16, len, segs, W.kind);
    }
}

__global__ __launch_bounds__(kHitThreads) void pm_points_at_length_kernel(MeasureParams M) {
    const SceneView &V = M.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves();
    for (uint32_t qi = FirstWaveUnit(); qi < M.n; qi += n_waves) {
        // {u32 item; u32 reserved; u64 s}, every lane alike: into scalar registers
        const uint2 *in = reinterpret_cast<const uint2 *>(M.q + static_cast<size_t>(qi) * 16);   // (8-byte aligned)
        const uint2 in0 = in[0], in1 = in[1];
        const uint32_t item = UniformF32Bits(in0.x), reserved = UniformF32Bits(in0.y);
        const unsigned long long s = (static_cast<unsigned long long>(UniformF32Bits(in1.y)) << 32) | UniformF32Bits(in1.x);
        uint8_t *out = M.out + static_cast<size_t>(qi) * 32;
        const MeasureWalk W = MeasureWalkOf(V, reserved == 0u ? item : kHitNone);
        unsigned long long carry = 0ull;                 // Q of the step's first entry
        uint32_t first_pt = kHitNone;                    // the first entry that is a point
        uint32_t last_k = kHitNone;                      // the last segment of a length so far, and its ends
        uint32_t lax = 0u, lay = 0u, lbx = 0u, lby = 0u;
        if (W.kind == kMeasureOpen && W.npt != 0u) first_pt = 0u;   // (a one-point Polyline has a point and no entry to walk)
        bool found = false;
        for (uint32_t base = 0; base < W.n_idx; base += 64u) {
            const uint32_t k = base + lane;
            float2 a = make_float2(0.0f, 0.0f), b = a;
            const bool seg = k < W.n_idx && MeasureEnds(W, k, a, b);
            const unsigned long long q = seg ? MeasureFix(a, b) : 0ull;
            const unsigned long long q1 = carry + MeasureScan(q, lane), q0 = q1 - q;
            if (first_pt == kHitNone) {
                const uint64_t pts = __ballot(seg);   // (an entry that starts a segment is a point)
                if (pts != 0ull) first_pt = base + static_cast<uint32_t>(__builtin_ctzll(pts));
            }
            const uint64_t hit = __ballot(q != 0ull && q0 <= s && s < q1);   // D15's start rule
            if (hit != 0ull) {   // (uniform; at most one lane: the intervals of the segments of a length are disjoint)
                if (lane == static_cast<uint32_t>(__builtin_ctzll(hit))) {
                    float t, x, y, tx, ty;
                    MeasurePoint(a, b, q0, q, s, t, x, y);
                    MeasureDir(a, b, tx, ty);
                    MeasureStore32(out, item, kMeasureFound, k, t, x, y, tx, ty);
                }
                found = true;
                break;
            }
            const uint64_t pos = __ballot(q != 0ull);
            if (pos != 0ull) {
                const uint32_t l = 63u - static_cast<uint32_t>(__builtin_clzll(pos));
                last_k = base + l;
                lax = MeasureLane32(__float_as_uint(a.x), l);
                lay = MeasureLane32(__float_as_uint(a.y), l);
                lbx = MeasureLane32(__float_as_uint(b.x), l);
                lby = MeasureLane32(__float_as_uint(b.y), l);
            }
            carry = MeasureLane64(q1, 63u);
        }
        if (found || lane != 0u) continue;
        // the walk ended without an owner: carry is T
        if (last_k != kHitNone) {   // s >= T > 0: the end of the last segment of a length
            const float2 a = make_float2(__uint_as_float(lax), __uint_as_float(lay)), b = make_float2(__uint_as_float(lbx), __uint_as_float(lby));
            float tx, ty;
            MeasureDir(a, b, tx, ty);
            MeasureStore32(out, item, kMeasureFound | (s > carry ? kMeasureClamped : 0u), last_k, 1.0f, b.x, b.y, tx, ty);
        } else if (first_pt != kHitNone) {   // T == 0: the first point
            const float2 p = LoadF2(W.pts + static_cast<size_t>(first_pt) * 8);
            MeasureStore32(out, item, kMeasureFound | kMeasureDegenerate | (s > 0ull ? kMeasureClamped : 0u), first_pt, 0.0f, p.x, p.y, 0.0f, 0.0f);
        } else {
            MeasureStore32(out, kHitNone, 0u, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

__global__ __launch_bounds__(kHitThreads) void pm_positions_on_edges_kernel(MeasureParams M) {
    const SceneView &V = M.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves();
    for (uint32_t qi = FirstWaveUnit(); qi < M.n; qi += n_waves) {
        // {u32 item; u32 index; f32 t; u32 reserved}, every lane alike
        const uint2 *in = reinterpret_cast<const uint2 *>(M.q + static_cast<size_t>(qi) * 16);   // (8-byte aligned)
        const uint2 in0 = in[0], in1 = in[1];
        const uint32_t item = UniformF32Bits(in0.x), index = UniformF32Bits(in0.y), reserved = UniformF32Bits(in1.y);
        const float t = __uint_as_float(UniformF32Bits(in1.x));
        uint8_t *out = M.out + static_cast<size_t>(qi) * 16;
        const MeasureWalk W = MeasureWalkOf(V, reserved == 0u ? item : kHitNone);
        bool valid = index < W.n_idx && t >= 0.0f && t <= 1.0f;   // (a NaN t fails both)
        unsigned long long qx = 0ull;
        if (valid) qx = MeasureQ(W, index, valid);
        unsigned long long Q = 0ull;
        if (valid) {   // (uniform)
            for (uint32_t j = lane; j < index; j += 64u) {
                bool seg;
                Q += MeasureQ(W, j, seg);
            }
            Q = MeasureWaveSum(Q);
        }
        if (lane != 0u) continue;
        if (valid) {
            const double f = floor(static_cast<double>(t) * static_cast<double>(qx) + 0.5);
            const unsigned long long along = f >= static_cast<double>(qx) ? qx : static_cast<unsigned long long>(f);
            MeasureStore16(out, Q + along, item, kMeasureFound);
        } else {
            MeasureStore16(out, 0ull, kHitNone, 0u);
        }
    }
}

void LaunchItemLengths(const MeasureParams &p, uint32_t n_cus, hipStream_t stream) {
    LaunchQuery(pm_item_lengths_kernel, p, ItemSteps(p.V.n_items), n_cus, stream);
}
void LaunchPointsAtLength(const MeasureParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_points_at_length_kernel, p, p.n, n_cus, stream); }
void LaunchPositionsOnEdges(const MeasureParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_positions_on_edges_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
