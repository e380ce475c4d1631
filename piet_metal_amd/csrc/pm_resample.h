// pm_resample_kernel: resampling -- count positions in an arithmetic progression along one item, answered in ONE walk of the item.
// Not on the frame path: like the measure kernels it reads the scene, nothing a frame writes.  Included by pm_context.hip after
// pm_measure.h, whose walk, fix, scan, point, direction and store it uses as they are: that a record is byte for byte what
// pm_points_at_length_kernel answers for the same item at the same position follows from shared code, not from a restatement.
//
// What a request is and what its positions are is decision D26; tests/np_resample.py states the positions from the
// decision's text in Python integers, and the records are np_measure's at those positions.
//
// A wave per request, in pm_query_common.h's persistent launch shape.  The positions s_0 <= s_1 <= ... of a request never decrease
// (step mode saturates, even mode's gaps are >= 0), so the wave keeps ONE cursor j0, the first sample not yet answered, and walks
// the item once, 64 entries per step as pm_points_at_length_kernel does (even mode walks it twice: the first pass is
// pm_item_lengths_kernel's strided sum, for T).  After a step's scan every sample with s < Q_end of the step is the step's:
//
//  * lane l takes sample j0 + l and asks whether its s is below the step's end: the ballot's population is how many of the 64 the
//    step owns -- 0 ends the step at the cost of one multiplication and one ballot, 64 starts another round of the same step;
//  * the owner of a sample is the first lane whose Q1 exceeds s (Q1 never decreases, so that lane has q > 0 and Q0 <= s: D15's start
//    rule): a binary search over the lanes, six rounds of two shuffles; the lane then fetches the owner's a, b, Q1 and q, eight
//    shuffles, and finishes the record with MeasurePoint and MeasureDir.
// So a long segment that owns a thousand samples keeps 64 lanes busy, and so do 64 short ones with a sample each; the cost is
// O(segments + samples).  No division anywhere in the walk (even mode divides once per request).
//
// After the walk the samples from j0 on have s >= T (all of them where T == 0 or the item has no walk): the lanes stride over them
// and answer from the last segment of a length, kept as pm_points_at_length_kernel keeps it, from the first point, or "none".  Lane 0
// writes the info.  No record at or beyond out_cap is written.  No atomics, no LDS, no scratch.
#pragma once

#include "pm_measure.h"

namespace pm {

struct ResampleParams {
    SceneView V;            // flags: PM_HIT_SKIP_TRANSPARENT
    const uint8_t *q;       // [32 n] pm_resample_query
    uint8_t *out;           // [32 out_cap] pm_length_point
    uint8_t *info;          // [16 n] pm_resample_info
    unsigned long long out_cap;
    uint32_t n;
};

namespace {

constexpr uint32_t kResampleStep = 0u;                 // PM_RESAMPLE_STEP
constexpr uint32_t kResampleEven = 1u;                 // PM_RESAMPLE_EVEN
constexpr uint32_t kResampleMaxCount = 1u << 20;       // PM_RESAMPLE_MAX_COUNT
constexpr uint32_t kResampleInvalid = 0xffffffffu;     // PM_RESAMPLE_INVALID

// The positions of a request: s_j = base + j * step, saturating at 2^64 - 1 (step mode: base = start), or j * step + min(j, extra)
// (even mode: step = T div m, extra = T mod m, which cannot overflow: every term is <= T).  j < 2^21.
struct ResamplePositions {
    unsigned long long base = 0ull, step = 0ull, extra = 0ull;
    bool even = false;
};

__device__ __forceinline__ unsigned long long ResampleAt(const ResamplePositions &P, uint32_t j) {
    const unsigned long long jj = j;
    if (P.even) return jj * P.step + (jj < P.extra ? jj : P.extra);
    const unsigned long long ph = jj * (P.step >> 32), pl = jj * (P.step & 0xffffffffull);   // (both below 2^53)
    if ((ph >> 32) != 0ull) return ~0ull;
    const unsigned long long p = (ph << 32) + pl;
    if (p < pl) return ~0ull;
    const unsigned long long s = P.base + p;
    return s < p ? ~0ull : s;
}

__device__ __forceinline__ unsigned long long ResampleShfl64(unsigned long long v, uint32_t src) {
    const uint32_t lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(v)), static_cast<int>(src), 64));
    const uint32_t hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(v >> 32)), static_cast<int>(src), 64));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}
__device__ __forceinline__ float ResampleShflF(float v, uint32_t src) {
    return __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(__float_as_uint(v)), static_cast<int>(src), 64)));
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_resample_kernel(ResampleParams M) {
    const SceneView &V = M.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves();
    for (uint32_t qi = FirstWaveUnit(); qi < M.n; qi += n_waves) {
        // {u32 item; u32 mode; u32 count; u32 first; u64 start; u64 step}, every lane alike: into scalar registers
        const uint2 *in = reinterpret_cast<const uint2 *>(M.q + static_cast<size_t>(qi) * 32);   // (8-byte aligned)
        const uint2 in0 = in[0], in1 = in[1], in2 = in[2], in3 = in[3];
        const uint32_t item = UniformF32Bits(in0.x), mode = UniformF32Bits(in0.y), count = UniformF32Bits(in1.x), first = UniformF32Bits(in1.y);
        const unsigned long long start = (static_cast<unsigned long long>(UniformF32Bits(in2.y)) << 32) | UniformF32Bits(in2.x);
        const unsigned long long step = (static_cast<unsigned long long>(UniformF32Bits(in3.y)) << 32) | UniformF32Bits(in3.x);
        uint8_t *info = M.info + static_cast<size_t>(qi) * 16;
        if (mode > kResampleEven || count > kResampleMaxCount || (mode == kResampleEven && (start | step) != 0ull)) {   // (uniform)
            if (lane == 0u) MeasureStore16(info, 0ull, 0u, kResampleInvalid);
            continue;
        }
        const MeasureWalk W = MeasureWalkOf(V, item);
        ResamplePositions P;
        P.base = start;
        P.step = step;
        if (mode == kResampleEven) {   // T first: pm_item_lengths_kernel's strided sum
            unsigned long long T = 0ull;
            for (uint32_t k = lane; k < W.n_idx; k += 64u) {
                bool seg;
                T += MeasureQ(W, k, seg);
            }
            T = MeasureWaveSum(T);
            T = MeasureLane64(T, 0u);
            const unsigned long long m = W.kind == kMeasureClosed ? count : (count != 0u ? count - 1u : 0u);
            P.even = true;
            P.base = 0ull;
            P.step = m != 0ull ? T / m : 0ull;
            P.extra = m != 0ull ? T % m : 0ull;
        }
        const unsigned long long rec0 = first;             // record of sample j: rec0 + j, written only below out_cap
        uint32_t j0 = 0u;                                   // the first sample not yet answered
        unsigned long long carry = 0ull;                    // Q of the step's first entry
        uint32_t first_pt = kHitNone;                       // the first entry that is a point
        uint32_t last_k = kHitNone;                         // the last segment of a length so far, and its ends
        uint32_t lax = 0u, lay = 0u, lbx = 0u, lby = 0u;
        if (W.kind == kMeasureOpen && W.npt != 0u) first_pt = 0u;
        for (uint32_t base = 0; base < W.n_idx; base += 64u) {
            const uint32_t k = base + lane;
            float2 a = make_float2(0.0f, 0.0f), b = a;
            const bool seg = k < W.n_idx && MeasureEnds(W, k, a, b);
            const unsigned long long q = seg ? MeasureFix(a, b) : 0ull;
            const unsigned long long q1 = carry + MeasureScan(q, lane);
            if (first_pt == kHitNone) {
                const uint64_t pts = __ballot(seg);
                if (pts != 0ull) first_pt = base + static_cast<uint32_t>(__builtin_ctzll(pts));
            }
            const unsigned long long end = MeasureLane64(q1, 63u);
            while (j0 < count) {   // (uniform) rounds of 64 samples of this step
                const uint32_t j = j0 + lane;
                const unsigned long long s = ResampleAt(P, j < count ? j : count - 1u);
                const bool mine = j < count && s < end;
                const uint64_t own = __ballot(mine);   // (a prefix of the lanes: the positions never decrease)
                if (own == 0ull) break;
                // the first lane whose Q1 exceeds s: how many lanes have Q1 <= s (63 at the most for a lane without a sample)
                uint32_t owner = 0u;
#pragma unroll
                for (uint32_t bit = 32u; bit != 0u; bit >>= 1) {
                    const unsigned long long probe = ResampleShfl64(q1, owner + bit - 1u);
                    if (probe <= s) owner += bit;
                }
                const float2 oa = make_float2(ResampleShflF(a.x, owner), ResampleShflF(a.y, owner));
                const float2 ob = make_float2(ResampleShflF(b.x, owner), ResampleShflF(b.y, owner));
                const unsigned long long oq1 = ResampleShfl64(q1, owner), oq = ResampleShfl64(q, owner);
                if (mine && rec0 + j < M.out_cap) {
                    float t, x, y, tx, ty;
                    MeasurePoint(oa, ob, oq1 - oq, oq, s, t, x, y);
                    MeasureDir(oa, ob, tx, ty);
                    MeasureStore32(M.out + static_cast<size_t>(rec0 + j) * 32, item, kMeasureFound, base + owner, t, x, y, tx, ty);
                }
                const uint32_t took = static_cast<uint32_t>(__popcll(own));
                j0 += took;
                if (took < 64u) break;
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
            carry = end;
        }
        // the walk is over: carry is T, and every sample from j0 on has s >= T
        uint32_t n_unclamped = j0;
        uint32_t ritem = kHitNone, status = 0u, index = 0u;
        float t = 0.0f, x = 0.0f, y = 0.0f, tx = 0.0f, ty = 0.0f;
        if (last_k != kHitNone) {   // T > 0: the end of the last segment of a length
            const float2 a = make_float2(__uint_as_float(lax), __uint_as_float(lay)), b = make_float2(__uint_as_float(lbx), __uint_as_float(lby));
            MeasureDir(a, b, tx, ty);
            ritem = item;
            status = kMeasureFound;
            index = last_k;
            t = 1.0f;
            x = b.x;
            y = b.y;
        } else if (first_pt != kHitNone) {   // T == 0: the first point
            const float2 p = LoadF2(W.pts + static_cast<size_t>(first_pt) * 8);
            ritem = item;
            status = kMeasureFound | kMeasureDegenerate;
            index = first_pt;
            x = p.x;
            y = p.y;
        }
        for (uint32_t jb = j0; jb < count; jb += 64u) {   // (uniform)
            const uint32_t j = jb + lane;
            const bool mine = j < count;
            const unsigned long long s = ResampleAt(P, mine ? j : count - 1u);
            const bool clamped = s > carry;
            if (ritem != kHitNone) n_unclamped += static_cast<uint32_t>(__popcll(__ballot(mine && !clamped)));
            if (mine && rec0 + j < M.out_cap)
                MeasureStore32(M.out + static_cast<size_t>(rec0 + j) * 32, ritem, ritem != kHitNone && clamped ? status | kMeasureClamped : status, index, t, x, y, tx, ty);
        }
        if (lane == 0u) MeasureStore16(info, carry, n_unclamped, W.kind);
    }
}

void LaunchResample(const ResampleParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_resample_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
