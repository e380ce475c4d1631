// Stroke caps, joins and miter limits: a styled stroke (PM_PATH_STROKE | PM_PATH_STROKE_OUTLINE) becomes ONE compound non-zero
// Fill item, its outline, built here at the end of the flatten stage.  Included by pm_flatten.hip inside namespace pm { namespace {
// (it uses that unit's PathOf, Overfull, BlockScan1024, WaveBox, SatU16, ThinLine); nothing of the frame path knows about it:
// binning, the tile kernel, hit testing and pm_item_paths see an ordinary Fill item (D11) in the poly-line's slot of paint order.
//
// ---- decision D14 (tests/np_stroke.py is the independent numpy statement) -------------------------------------
// Input: the stroke's f32 poly-line points P[0..n) as KPoints stored them (they stay where they are, unreferenced), closed =
// the sub-path's last element is PM_EL_CLOSE, hw = f64(width * 0.5f) after the thin-line rule, cap, join, the miter limit m
// (binary16 -> f64; 0 means 4) and the level L = the smallest L with hw <= kLevelHw[L], else 6.
// Arithmetic: binary64 on the f32 values, one rounding per written operation in the written order, + - * / sqrt only (no libm,
// no trigonometry, no fused multiply-add); an outline point is rounded once to f32 when it is stored.
//   dir(a, b):  d = b - a; degenerate if d.x == 0 and d.y == 0; else len = sqrt(d.x*d.x + d.y*d.y), u = (d.x/len, d.y/len)
//   segments:   k in [0, nseg), nseg = closed ? n : n - 1, from P[k] to P[k + 1] (the closing one to P[0])
//   din(i):     u of the nearest non-degenerate segment k = i-1, i-2, ... ; dout(i): of k = i, i+1, ... -- cyclically over all
//               nseg segments if closed, to the ends of the poly-line otherwise; either may not exist
// Pieces (each a closed sub-path followed by its D11 separator {NaN, index of its first entry}), all wound alike
// (cross(v1 - v0, v2 - v0) >= 0), so that the non-zero sum is their union.  "p + hw*e" is (p.x + hw*e.x, p.y + hw*e.y).
//   segment k:  a - N, b - N, b + N, a + N with N = (-(hw*u.y), hw*u.x); a degenerate segment: a four times.   [5 entries]
//   join at vertex i (every vertex if closed, else 0 < i < n - 1), p = P[i], d1 = din(i), d2 = dout(i),
//               c = d1.x*d2.y - d1.y*d2.x, dot = d1.x*d2.x + d1.y*d2.y:
//                 c > 0:               e0 = (d1.y, -d1.x), e1 = (d2.y, -d2.x)
//                 c < 0:               e0 = (-d2.y, d2.x), e1 = (-d1.y, d1.x)
//                 c == 0 and dot < 0:  e0 = (d1.y, -d1.x), e1 = (-d1.y, d1.x), a half turn whose first bisector is d1
//                 otherwise (straight on, a missing direction, NaN): every entry of the piece is p
//               bevel  p, p + hw*e0, p + hw*e1                                                               [4 entries]
//               miter  p, p + hw*e0, tip, p + hw*e1; tip = p + k*(e0 + e1) with k = hw / (1 + dot) if no half turn and
//                      (m*m) * (1 + dot) >= 2 (the limit, tested on d1.d2: 1/sin(theta/2) = sqrt(2 / (1 + dot))), else
//                      tip = p + hw*e0: the bevel                                                             [5 entries]
//               round  p, p + hw*r[0], ..., p + hw*r[2^L]: a fan                                         [2^L + 3 entries]
//   fans:       r[0] = e0, r[2^L] = e1, r[2^(L-1)] = the first bisector, every further r[(i + j)/2] = bis(r[i], r[j]) with
//               bis(u, v): s = u + v, (s.x/|s|, s.y/|s|), |s| = sqrt(s.x*s.x + s.y*s.y); the first bisector is bis(e0, e1), or
//               the given direction of a half turn.  A join uses the path's L whatever its turn.
//   caps:       two unless the cap is butt: the start cap at p = P[0] facing d = -dout(0), the end cap at p = P[n-1] facing
//               d = din(n-1); a sub-path without any non-degenerate segment faces (-1, 0) and (1, 0): a disc / an axis-aligned
//               square (closed or not); a closed sub-path WITH one has nothing to cap: every entry is p.
//               e0 = (d.y, -d.x), e1 = (-d.y, d.x), a half turn about d.
//               round   the fan                                                                          [2^L + 3 entries]
//               square  q = p + hw*d: p + hw*e0, q + hw*e0, q + hw*e1, p + hw*e1                              [5 entries]
// Layout of the item's entries: the segments, then the joins (by vertex), then the start cap, then the end cap.
// The item: Fill, flags = compound (non-zero), the stroke's colour (after the thin-line rule), n_points = the entry count,
// points at the end of the scene as it is without outlines (items in paint order).  ShortBbox: floor / ceil of the min / max of
// the stored f32 outline points, saturated to u16 as for fills; no entries: the zero box.
// A non-finite poly-line point makes the entries it touches NaN (no bit pattern is promised for them).
// A path with a dash pattern (decision D15, pm_dash.h) is not outlined here: KOutlineCount and KOutline skip its sub-paths.
#pragma once

// kLevelHw = {0.1, 0.3414, 1.3137, 5.2043, 20.767, 83.018}: 0.1 / (1 - cos(pi / 2^(L+1))) rounded down -- the largest hw whose half
// circle in 2^L steps keeps its sagitta within the flatten tolerance 0.1 (FanLevel)
constexpr uint32_t kMaxLevel = 6;

__host__ __device__ inline double HalfBitsToDouble(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    double v;
    if (e == 0) v = static_cast<double>(m) * (1.0 / 16777216.0);  // m * 2^-24
    else if (e == 31) v = m ? __builtin_nan("") : __builtin_inf();
    else {
        v = 1.0 + static_cast<double>(m) * (1.0 / 1024.0);
        for (uint32_t k = e; k < 15; ++k) v *= 0.5;
        for (uint32_t k = 15; k < e; ++k) v *= 2.0;
    }
    return (h & 0x8000u) ? -v : v;
}

// the style fields of pm_path.flags are well-formed (host check: PM_ERR_INVALID otherwise)
inline bool StrokeStyleValid(uint32_t flags) {
    if (PM_PATH_STROKE_CAP(flags) == 3u || PM_PATH_STROKE_JOIN(flags) == 3u) return false;
    const uint32_t h = PM_PATH_STROKE_MITER_HALF(flags);
    if (h == 0) return true;
    const double m = HalfBitsToDouble(h);
    return m >= 1.0 && m <= 65504.0;  // (NaN fails both)
}

__device__ __forceinline__ bool IsOutlined(uint32_t flags) {
    return (flags & (PM_PATH_STROKE | PM_PATH_STROKE_OUTLINE)) == (PM_PATH_STROKE | PM_PATH_STROKE_OUTLINE);
}

__device__ __forceinline__ uint32_t FanLevel(double hw) {
    if (hw <= 0.1) return 0;  // kLevelHw, written out (no indexed table in a kernel)
    if (hw <= 0.3414) return 1;
    if (hw <= 1.3137) return 2;
    if (hw <= 5.2043) return 3;
    if (hw <= 20.767) return 4;
    if (hw <= 83.018) return 5;
    return kMaxLevel;
}

// What one sub-path's styled stroke is made from.
struct OutlineJob {
    bool styled;
    bool closed;
    uint32_t n;       // poly-line points
    uint32_t item;    // the stroke's item
    uint32_t path;    // its path
    size_t pts_ix;    // byte offset of the poly-line's points
    uint32_t rgba;    // after the thin-line rule
    double hw;
    uint32_t L, cap, join;
    double mlim;
};

template <bool kGrouped>
__device__ __forceinline__ OutlineJob MakeOutlineJob(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale_u,
                                                     const GroupTable &gt, const uint32_t *el_ptoff, const uint32_t *el_mvoff, const uint32_t *path_item_base,
                                                     const uint32_t *path_pt_base, const uint32_t *sub_first_el, uint32_t n_items, uint32_t s) {
    OutlineJob job;
    const uint32_t first = sub_first_el[s];
    const uint32_t p = PathOf(paths, n_paths, first);
    const pm_path path = paths[p];
    job.styled = IsOutlined(path.flags);
    job.path = p;
    if (!job.styled) return job;
    // (the stroke's slot, as KItems numbers it: behind the path's fill items and fill points)
    const uint32_t sub0 = el_mvoff[path.el_begin];
    const uint32_t n_sub_path = el_mvoff[path.el_end] - sub0;
    const uint32_t j = s - sub0;
    const uint32_t last = (j + 1 < n_sub_path) ? sub_first_el[s + 1] : path.el_end;
    const uint32_t path_pts = el_ptoff[path.el_end] - el_ptoff[path.el_begin];
    const uint32_t local = el_ptoff[first] - el_ptoff[path.el_begin];
    const bool has_fill = (path.flags & PM_PATH_FILL) != 0, compound = has_fill && (path.flags & PM_PATH_COMPOUND) != 0;
    const size_t points_start = sizeof(SimpleGroup) + static_cast<size_t>(n_items) * (sizeof(ShortBbox) + kItemSize);
    job.n = el_ptoff[last] - el_ptoff[first];
    job.closed = els[last - 1u].tag == PM_EL_CLOSE;
    job.item = path_item_base[p] + (has_fill ? (compound ? 1u : n_sub_path) : 0u) + j;
    job.pts_ix = points_start + 8 * (static_cast<size_t>(path_pt_base[p]) + (has_fill ? path_pts + (compound ? n_sub_path : 0u) : 0u) + local);
    const float width_scale = WidthScaleOf<kGrouped>(width_scale_u, gt, p);  // (decision D16: the path's own group's)
    float width = path.stroke_width * width_scale;
    job.rgba = path.stroke_rgba;
    ThinLine(&width, &job.rgba);
    job.hw = static_cast<double>(width * 0.5f);
    job.L = FanLevel(job.hw);
    job.cap = PM_PATH_STROKE_CAP(path.flags);
    job.join = PM_PATH_STROKE_JOIN(path.flags);
    const uint32_t mh = PM_PATH_STROKE_MITER_HALF(path.flags);
    job.mlim = mh ? HalfBitsToDouble(mh) : 4.0;
    return job;
}

struct OutlineLayout {
    unsigned long long nseg, njoin, join_size, cap_size, total;
};

// The entry count is a closed form of (n, closed, cap, join, L): nothing of the layout depends on a coordinate.
__device__ __forceinline__ OutlineLayout LayoutOf(const OutlineJob &job) {
    OutlineLayout lay;
    const unsigned long long n = job.n, fan = (1ull << job.L) + 3ull;
    lay.nseg = job.closed ? n : n - 1ull;
    lay.njoin = job.closed ? n : (n >= 2ull ? n - 2ull : 0ull);
    lay.join_size = job.join == PM_STROKE_JOIN_BEVEL ? 4ull : (job.join == PM_STROKE_JOIN_MITER ? 5ull : fan);
    lay.cap_size = job.cap == PM_STROKE_CAP_BUTT ? 0ull : (job.cap == PM_STROKE_CAP_SQUARE ? 5ull : fan);
    lay.total = 5ull * lay.nseg + lay.join_size * lay.njoin + 2ull * lay.cap_size;
    return lay;
}

// no dash table, or none for this path (decision D15, pm_dash.h: a dashed sub-path is KDashCount's and KDash's)
constexpr uint32_t kNoDash = 0xffffffffu;
__device__ __forceinline__ bool IsDashed(const uint32_t *path_dash, uint32_t p) { return path_dash != nullptr && path_dash[p] != kNoDash; }

// One thread per sub-path: out_cnt[s] = entries of its outline (0: not a styled stroke); their 64-bit sum to *out_total.
template <bool kGrouped>
__device__ __forceinline__ void OutlineCountBody(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale, const GroupTable &gt,
                                                 const uint32_t *el_ptoff, const uint32_t *el_mvoff, const uint32_t *path_item_base,
                                                 const uint32_t *path_pt_base, const uint32_t *sub_first_el, const uint32_t *totals,
                                                 const uint32_t *path_dash, uint32_t *out_cnt, unsigned long long *out_total) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long q = 0;
    if (s < totals[2]) {
        const OutlineJob job = MakeOutlineJob<kGrouped>(paths, n_paths, els, width_scale, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, totals[0], s);
        const bool dashed = job.styled && IsDashed(path_dash, job.path);
        if (job.styled && !dashed) q = LayoutOf(job).total;
        if (!dashed) out_cnt[s] = static_cast<uint32_t>(q);  // (a count past 2^32 never fits: the 64-bit sum says so, KOutline then writes nothing)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor(q, d, 64);
    if ((threadIdx.x & 63u) == 0 && q != 0) atomicAdd(out_total, q);
}

__global__ void KOutlineCount(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale, const uint32_t *el_ptoff,
                              const uint32_t *el_mvoff, const uint32_t *path_item_base, const uint32_t *path_pt_base,
                              const uint32_t *sub_first_el, const uint32_t *totals, const uint32_t *path_dash, uint32_t *out_cnt,
                              unsigned long long *out_total) {
    OutlineCountBody<false>(paths, n_paths, els, width_scale, GroupTable{nullptr, nullptr}, el_ptoff, el_mvoff, path_item_base, path_pt_base,
                            sub_first_el, totals, path_dash, out_cnt, out_total);
}

__global__ void KOutlineCountGrouped(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, GroupTable gt, const uint32_t *el_ptoff,
                                     const uint32_t *el_mvoff, const uint32_t *path_item_base, const uint32_t *path_pt_base,
                                     const uint32_t *sub_first_el, const uint32_t *totals, const uint32_t *path_dash, uint32_t *out_cnt,
                                     unsigned long long *out_total) {
    OutlineCountBody<true>(paths, n_paths, els, 0.0f, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, totals, path_dash, out_cnt,
                           out_total);
}

// One workgroup: exclusive scan of out_cnt over the sub-paths.  Then the scene's 64-bit point count grows by the outlines'
// entries (what the host sizes the scene by); the count without them stays in out_total[1] for KOutline.
__global__ __launch_bounds__(kScanThreads) void KOutlineScan(const uint32_t *totals, const uint32_t *out_cnt, uint32_t *out_off,
                                                             unsigned long long *out_total, unsigned long long *n_pts64) {
    __shared__ uint32_t s_w[kScanThreads / 64];
    const uint32_t n_subs = totals[2];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_subs; base += kScanThreads) {
        const uint32_t s = base + threadIdx.x;
        const uint32_t v = s < n_subs ? out_cnt[s] : 0u;
        uint32_t t;
        const uint32_t o = BlockScan1024(v, s_w, &t);
        if (s < n_subs) out_off[s] = carry + o;
        carry += t;
    }
    if (threadIdx.x == 0) {
        const unsigned long long plain = *n_pts64;
        out_total[1] = plain;
        *n_pts64 = plain + out_total[0];
    }
}

struct V2 {
    double x, y;
};

// Writes one item's entries; every store is checked against scene_cap.  Keeps the lane's box of the stored f32 values.
struct OutlineSink {
    uint8_t *scene;
    size_t at;  // byte offset of the item's entry 0
    uint32_t scene_cap;
    double x0, y0, x1, y1;
    bool any;
    __device__ __forceinline__ void Point(unsigned long long e, double x, double y) {
        const float2 f = make_float2(static_cast<float>(x), static_cast<float>(y));
        const unsigned long long o = at + 8ull * e;
        if (o + 8ull <= scene_cap) *reinterpret_cast<float2 *>(scene + o) = f;
        x0 = fmin(x0, static_cast<double>(f.x)); y0 = fmin(y0, static_cast<double>(f.y));
        x1 = fmax(x1, static_cast<double>(f.x)); y1 = fmax(y1, static_cast<double>(f.y));
        any = true;
    }
    __device__ __forceinline__ void Separator(unsigned long long e, unsigned long long first) {
        const unsigned long long o = at + 8ull * e;
        if (o + 8ull <= scene_cap) *reinterpret_cast<uint2 *>(scene + o) = make_uint2(kSubpathSeparatorBits, static_cast<uint32_t>(first));
    }
};

__device__ __forceinline__ V2 LoadPoint(const uint8_t *scene, size_t pts_ix, uint32_t i) {
    const float2 f = *reinterpret_cast<const float2 *>(scene + pts_ix + 8 * static_cast<size_t>(i));
    return V2{static_cast<double>(f.x), static_cast<double>(f.y)};
}

// dir(P[k], P[k + 1]) of segment k; false: degenerate
__device__ __forceinline__ bool SegmentDir(const uint8_t *scene, const OutlineJob &job, uint32_t k, V2 *u) {
    const V2 a = LoadPoint(scene, job.pts_ix, k), b = LoadPoint(scene, job.pts_ix, k + 1u == job.n ? 0u : k + 1u);
    const double dx = b.x - a.x, dy = b.y - a.y;
    if (dx == 0.0 && dy == 0.0) return false;
    const double len = sqrt(dx * dx + dy * dy);
    u->x = dx / len;
    u->y = dy / len;
    return true;
}

// din(i) (back = true) / dout(i): the nearest non-degenerate segment on that side.  (A walk: one step wherever the
// neighbouring segment has a length, which is everywhere but at repeated points.)
__device__ bool VertexDir(const uint8_t *scene, const OutlineJob &job, uint32_t nseg, uint32_t i, bool back, V2 *u) {
    if (nseg == 0) return false;
    uint32_t k = i;
    for (uint32_t step = 0; step < nseg; ++step) {
        if (back) {
            if (k == 0) {
                if (!job.closed) return false;
                k = nseg;
            }
            --k;
        } else if (step) {
            ++k;
        }
        if (k >= nseg) {
            if (!job.closed) return false;
            k = 0;
        }
        if (SegmentDir(scene, job, k, u)) return true;
    }
    return false;
}

__device__ __forceinline__ V2 Bisector(V2 u, V2 v) {
    const double sx = u.x + v.x, sy = u.y + v.y;
    const double len = sqrt(sx * sx + sy * sy);
    return V2{sx / len, sy / len};
}

// r[j] of the fan from e0 to e1 with first bisector `mid`: a descent through the levels, nothing kept in an array
__device__ V2 RimDir(V2 e0, V2 e1, V2 mid, uint32_t L, uint32_t j) {
    uint32_t lo = 0, hi = 1u << L;
    if (j == lo) return e0;
    if (j == hi) return e1;
    V2 a = e0, b = e1, m = mid;
    for (;;) {
        const uint32_t at = (lo + hi) >> 1;
        if (j == at) return m;
        if (j < at) {
            b = m;
            hi = at;
        } else {
            a = m;
            lo = at;
        }
        m = Bisector(a, b);
    }
}

// The corner between e0 and e1 about p (a join, or a cap's half turn): `kind` = the piece.  collapse: every entry is p.
enum CornerKind : uint32_t { kCornerBevel, kCornerMiter, kCornerFan, kCornerSquare };

__device__ void EmitCorner(OutlineSink &sink, unsigned long long e, CornerKind kind, V2 p, V2 e0, V2 e1, V2 mid, bool half_turn, bool collapse,
                           double dot, double hw, double mlim, uint32_t L) {
    const unsigned long long first = e;
    auto rim = [&](V2 r) { return collapse ? p : V2{p.x + hw * r.x, p.y + hw * r.y}; };
    if (kind == kCornerSquare) {
        const V2 q = collapse ? p : V2{p.x + hw * mid.x, p.y + hw * mid.y};
        const V2 c0 = rim(e0), c3 = rim(e1);
        const V2 c1 = collapse ? p : V2{q.x + hw * e0.x, q.y + hw * e0.y}, c2 = collapse ? p : V2{q.x + hw * e1.x, q.y + hw * e1.y};
        sink.Point(e++, c0.x, c0.y);
        sink.Point(e++, c1.x, c1.y);
        sink.Point(e++, c2.x, c2.y);
        sink.Point(e++, c3.x, c3.y);
    } else if (kind == kCornerFan) {
        sink.Point(e++, p.x, p.y);
        const V2 m = (half_turn || collapse) ? mid : Bisector(e0, e1);
        for (uint32_t j = 0; j <= (1u << L); ++j) {
            const V2 r = collapse ? p : rim(RimDir(e0, e1, m, L, j));
            sink.Point(e++, r.x, r.y);
        }
    } else {
        const V2 c0 = rim(e0), c1 = rim(e1);
        sink.Point(e++, p.x, p.y);
        sink.Point(e++, c0.x, c0.y);
        if (kind == kCornerMiter) {
            V2 tip = c0;
            const double s = 1.0 + dot;
            if (!collapse && !half_turn && (mlim * mlim) * s >= 2.0) {
                const double k = hw / s;
                tip = V2{p.x + k * (e0.x + e1.x), p.y + k * (e0.y + e1.y)};
            }
            sink.Point(e++, tip.x, tip.y);
        }
        sink.Point(e++, c1.x, c1.y);
    }
    sink.Separator(e, first);
}

// The join at p between the directions d1 (in) and d2 (out), either of which may not exist.
__device__ __forceinline__ void EmitJoin(OutlineSink &sink, unsigned long long e, CornerKind kind, V2 p, bool has1, V2 d1, bool has2, V2 d2, double hw,
                                         double mlim, uint32_t L) {
    const double c = d1.x * d2.y - d1.y * d2.x, dot = d1.x * d2.x + d1.y * d2.y;
    V2 e0 = p, e1 = p, mid = p;
    bool half_turn = false, collapse = false;
    if (has1 && has2 && c > 0.0) {
        e0 = V2{d1.y, -d1.x};
        e1 = V2{d2.y, -d2.x};
    } else if (has1 && has2 && c < 0.0) {
        e0 = V2{-d2.y, d2.x};
        e1 = V2{-d1.y, d1.x};
    } else if (has1 && has2 && c == 0.0 && dot < 0.0) {
        e0 = V2{d1.y, -d1.x};
        e1 = V2{-d1.y, d1.x};
        mid = d1;
        half_turn = true;
    } else {
        collapse = true;
    }
    EmitCorner(sink, e, kind, p, e0, e1, mid, half_turn, collapse, dot, hw, mlim, L);
}

// The D14 outline of one sub-path, by one wave: the lanes stride over the vertices; a lane writes its vertex's segment, join and
// cap pieces.
__device__ __forceinline__ void OutlineSubpath(const uint8_t *scene, const OutlineJob &job, const OutlineLayout &lay, OutlineSink &sink, uint32_t lane) {
    const uint32_t n = job.n, nseg = static_cast<uint32_t>(lay.nseg);
    const double hw = job.hw;
    const unsigned long long joins_at = 5ull * lay.nseg, caps_at = joins_at + lay.join_size * lay.njoin;
    const CornerKind join_kind = job.join == PM_STROKE_JOIN_BEVEL ? kCornerBevel : (job.join == PM_STROKE_JOIN_MITER ? kCornerMiter : kCornerFan);
    const CornerKind cap_kind = job.cap == PM_STROKE_CAP_SQUARE ? kCornerSquare : kCornerFan;
    for (uint32_t i = lane; i < n; i += 64u) {
        const V2 p = LoadPoint(scene, job.pts_ix, i);
        if (i < nseg) {  // the segment that starts here
            const V2 b = LoadPoint(scene, job.pts_ix, i + 1u == n ? 0u : i + 1u);
            V2 u;
            const unsigned long long e = 5ull * i;
            if (SegmentDir(scene, job, i, &u)) {
                const double nx = -(hw * u.y), ny = hw * u.x;
                sink.Point(e + 0, p.x - nx, p.y - ny);
                sink.Point(e + 1, b.x - nx, b.y - ny);
                sink.Point(e + 2, b.x + nx, b.y + ny);
                sink.Point(e + 3, p.x + nx, p.y + ny);
            } else {
                for (uint32_t k = 0; k < 4; ++k) sink.Point(e + k, p.x, p.y);
            }
            sink.Separator(e + 4, e);
        }
        const bool joined = job.closed || (i > 0 && i + 1u < n);
        const bool capped = lay.cap_size != 0 && (i == 0 || i + 1u == n);
        if (!joined && !capped) continue;
        V2 d1{0.0, 0.0}, d2{0.0, 0.0};
        const bool has1 = VertexDir(scene, job, nseg, i, true, &d1), has2 = VertexDir(scene, job, nseg, i, false, &d2);
        if (joined) EmitJoin(sink, joins_at + lay.join_size * (job.closed ? i : i - 1u), join_kind, p, has1, d1, has2, d2, hw, job.mlim, job.L);
        if (capped) {
            // (a sub-path of one point is both ends)
            for (uint32_t end = 0; end < 2; ++end) {
                if (end == 0 ? i != 0 : i + 1u != n) continue;
                // (at an end vertex has1 || has2 says whether the sub-path has a non-degenerate segment at all)
                V2 d = end == 0 ? V2{-d2.x, -d2.y} : d1;
                bool collapse = false;
                if (!has1 && !has2) d = V2{end == 0 ? -1.0 : 1.0, 0.0};  // a dot: the caps face (-1, 0) and (1, 0)
                else if (job.closed) collapse = true;                    // nothing to cap
                EmitCorner(sink, caps_at + lay.cap_size * end, cap_kind, p, V2{d.y, -d.x}, V2{-d.y, d.x}, d, true, collapse, 0.0, hw, job.mlim, job.L);
            }
        }
    }
}

// The box is reduced over the wave and lane 0 rewrites the item record and its ShortBbox in place.
__device__ __forceinline__ void WriteOutlineItem(uint8_t *scene, uint32_t scene_cap, uint32_t n_items, const OutlineJob &job, OutlineSink &sink,
                                                 uint32_t total, uint32_t lane) {
    const size_t bbox_start = sizeof(SimpleGroup);
    const size_t items_start = bbox_start + static_cast<size_t>(n_items) * sizeof(ShortBbox);
    WaveBox(sink.x0, sink.y0, sink.x1, sink.y1);
    if (__ballot(sink.any) == 0ull) sink.x0 = sink.y0 = sink.x1 = sink.y1 = 0.0;
    if (lane == 0 && items_start + (static_cast<size_t>(job.item) + 1) * kItemSize <= scene_cap) {
        ShortBbox sb{SatU16(floor(sink.x0)), SatU16(floor(sink.y0)), SatU16(ceil(sink.x1)), SatU16(ceil(sink.y1))};
        *reinterpret_cast<ShortBbox *>(scene + bbox_start + static_cast<size_t>(job.item) * sizeof(ShortBbox)) = sb;
        uint32_t *it = reinterpret_cast<uint32_t *>(scene + items_start + static_cast<size_t>(job.item) * kItemSize);
        it[0] = kItemFill;
        it[1] = kFillCompound;
        it[2] = __builtin_bswap32(job.rgba);
        it[3] = total;
        it[4] = static_cast<uint32_t>(sink.at);
        it[5] = it[6] = it[7] = 0;
    }
}

// One WAVE per sub-path, as in KItems.
template <bool kGrouped>
__device__ __forceinline__ void OutlineBody(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale, const GroupTable &gt,
                                            const uint32_t *el_ptoff, const uint32_t *el_mvoff, const uint32_t *path_item_base,
                                            const uint32_t *path_pt_base, const uint32_t *sub_first_el, const uint32_t *totals,
                                            const unsigned long long *n_pts64, const uint32_t *out_off, const unsigned long long *out_total,
                                            const uint32_t *path_dash, uint8_t *scene, uint32_t scene_cap) {
    const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_items = totals[0], n_subs = totals[2];
    if (s >= n_subs || Overfull(n_items, *n_pts64, scene_cap)) return;  // (whole waves; *n_pts64 counts the outlines by now)
    const OutlineJob job = MakeOutlineJob<kGrouped>(paths, n_paths, els, width_scale, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, n_items, s);
    if (!job.styled || IsDashed(path_dash, job.path)) return;  // (uniform)
    const OutlineLayout lay = LayoutOf(job);
    const size_t outlines_start = sizeof(SimpleGroup) + static_cast<size_t>(n_items) * (sizeof(ShortBbox) + kItemSize) + 8 * static_cast<size_t>(out_total[1]);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    OutlineSink sink{scene, outlines_start + 8 * static_cast<size_t>(out_off[s]), scene_cap, nan, nan, nan, nan, false};
    OutlineSubpath(scene, job, lay, sink, lane);
    WriteOutlineItem(scene, scene_cap, n_items, job, sink, static_cast<uint32_t>(lay.total), lane);
}

__global__ __launch_bounds__(256) void KOutline(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale, const uint32_t *el_ptoff,
                         const uint32_t *el_mvoff, const uint32_t *path_item_base, const uint32_t *path_pt_base, const uint32_t *sub_first_el,
                         const uint32_t *totals, const unsigned long long *n_pts64, const uint32_t *out_off, const unsigned long long *out_total,
                         const uint32_t *path_dash, uint8_t *scene, uint32_t scene_cap) {
    OutlineBody<false>(paths, n_paths, els, width_scale, GroupTable{nullptr, nullptr}, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el,
                       totals, n_pts64, out_off, out_total, path_dash, scene, scene_cap);
}

__global__ __launch_bounds__(256) void KOutlineGrouped(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, GroupTable gt,
                                                       const uint32_t *el_ptoff, const uint32_t *el_mvoff, const uint32_t *path_item_base,
                                                       const uint32_t *path_pt_base, const uint32_t *sub_first_el, const uint32_t *totals,
                                                       const unsigned long long *n_pts64, const uint32_t *out_off, const unsigned long long *out_total,
                                                       const uint32_t *path_dash, uint8_t *scene, uint32_t scene_cap) {
    OutlineBody<true>(paths, n_paths, els, 0.0f, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, totals, n_pts64, out_off,
                      out_total, path_dash, scene, scene_cap);
}
