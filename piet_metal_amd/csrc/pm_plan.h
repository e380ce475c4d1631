// Binning's host side as a pure function: which strip rows of the band get a binning workgroup, which are cut in two, where
// every strip row's arena region lies, how the work list is chained over the resident grid, the band's item list and the
// per-tile-row list offsets.  Plain arithmetic on the scene's header, boxes and item records and a dozen integers: no HIP
// runtime call, no context, no environment, no global state -- pm_context.hip (EnsureArena) hands the result to the device,
// tests/plan/ runs it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/piet_metal_amd.h"
#include "pm_device.h"

namespace pm {

constexpr uint64_t kArenaLimit = 0xfffffff0ull;  // dwords: a slot's binning arena, and the entries of the per-tile-row item lists
constexpr uint32_t kBinWgPerCuUnset = 0xffu;     // PM_BIN_WG_PER_CU not given: by the number of strip rows
constexpr uint32_t kBinWgPerCu = 5;              // ... pm_bin_kernel's workgroups a CU holds (its LDS is sized for that)

// Binning workgroups the chip holds at once.  per_cu is PM_BIN_WG_PER_CU as the context keeps it: unset counts as kBinWgPerCu,
// 0 ("a workgroup per strip row") as `if_zero` -- the callers differ in exactly that, and in whether they look at the switch at all.
inline size_t ResidentBinWorkgroups(int n_cus, uint32_t per_cu, uint32_t if_zero) {
    if (per_cu == kBinWgPerCuUnset) per_cu = kBinWgPerCu;
    if (per_cu == 0u) per_cu = if_zero;
    return static_cast<size_t>(n_cus) * per_cu;
}

// Worst-case binning-arena demand of one item record in one strip row (dwords): kChunkSegs segment slots (16 B) + meta words
// per chunk (every chunk surviving), plus a token amount that tells a strip row some item reaches from one nothing reaches.
// margin > 0 (a plan made to last through a zooming view): curves flatten into more segments as they grow.
inline uint64_t ItemArenaDwords(const uint8_t *item, int margin) {
    uint32_t tag, npt = 0;
    std::memcpy(&tag, item, 4);
    tag &= 0xffffu;
    std::memcpy(&npt, item + 12, 4);
    uint64_t nseg = 0;
    if (tag == kItemFill) nseg = npt;
    if (tag == kItemPoly && npt >= 2) nseg = npt - 1;
    if (tag == kItemLine) nseg = 1;
    if (margin > 0 && tag != kItemLine) nseg += nseg / 4 + 2 * kChunkSegs;
    const uint64_t nch = (nseg + kChunkSegs - 1) / kChunkSegs;
    return 4u + static_cast<uint64_t>(kSlotDwords) * kChunkSegs * nch;
}

// Everything a plan depends on.
struct PlanInput {
    const uint8_t *item_meta = nullptr;  // header + boxes + items of the scene (never a point: the planner reads no further)
    uint32_t n_items = 0;
    uint32_t n_chunks = 0;
    uint32_t tiles_x = 0, strips_x = 0, row0 = 0, row1 = 0;
    int n_cus = 0;
    int margin = 0;  // pixels every box is widened by (0, or kTileW for a plan made to last through a view change)
    int bin_split_mode = 1;
    uint32_t bin_split_cands = 1u << 30, bin_split_slots = 224, bin_split_fill = 15;
    uint32_t bin_wg_per_cu = kBinWgPerCuUnset, bin_waves_env = 0, bin_waves_inflight = 1;
    int one_launch_mode = 0;
    uint32_t frame_wg_per_cu = 0;
    int fold_clear_mode = 2;
    const uint32_t *fb_slots = nullptr;  // the frames' report: segment slots per strip row of the band (n_fb_slots == 0: none yet)
    size_t n_fb_slots = 0;
    int row_list_min_items = 2048;   // PM_ROW_LIST_MIN_ITEMS
    int row_list_part_items = 0;     // PM_ROW_LIST_PART_ITEMS (0: not given -- by the number of CUs and tile rows)
    uint64_t ptcl_initial_cmds = 0;  // PM_PTCL_INITIAL_CMDS (0: not given)
    uint32_t arena_cap = 0;          // capacities the result is a maximum with: dwords of a slot's binning arena
    uint64_t ptcl_want = 0;          // ... and quads of its tile arena
};

// Everything a plan produces.  One lives in the context and is built into again and again: the vectors keep their capacity (a
// re-planning animation allocates nothing) and are the sources of the asynchronous uploads.
struct BinPlan {
    std::vector<uint4> desc;         // the strip-row work list: {strip | tiles << 8 | row << 16, arena region begin, end, next of the chain}
    std::vector<uint4> desc_whole;   // ... with every cut strip row whole again (empty: nothing is cut)
    std::vector<uint32_t> next_one;  // chains of the one-launch grid
    std::vector<uint32_t> idle;      // strip rows without a workgroup (only for frames that clear them from this list)
    std::vector<uint2> band_bbox;    // items that reach the band, paint order: boxes
    std::vector<uint32_t> band_item; // ... and scene indices
    std::vector<uint32_t> row_base;  // per-tile-row item lists: rb[r * parts + p] = where part p of row r writes (+ total)
    std::vector<uint2> sr_list;      // ... and every work-list entry's {first entry, entries} of its tile row
    std::vector<uint16_t> box;       // [4 n] the boxes the plan was made for (widened by the margin)
    std::vector<uint32_t> per;       // [n] arena dwords per item
    uint64_t cands = 0;              // (item, strip row) pairs: candidates the strip rows will look at
    uint32_t n_sr_split = 0;         // strip rows cut in two
    uint32_t bin_waves = 4, bin_grid = 1, one_grid_rows = 0;
    bool use_row_lists = false;
    bool band_identity = false;  // the band's item list IS the scene's item list: the kernels read the scene's own boxes
    uint32_t row_parts = 1, row_part_items = kRowCullStep, row_total = 0;
    uint64_t row_want = 0;
    uint32_t sr_empty_dwords = 0;  // size of a region no item reaches
    uint64_t arena_total = 0;      // dwords the regions take
    uint32_t arena_alloc = 0;      // ... and what a slot's arena is to hold (with headroom when it has to grow)
    uint64_t ptcl_want = 0;
    bool fb_applied = false;    // made with the frames' report
    bool reusable = false;      // made with widened boxes, for the whole item list in scene order: the next scene may keep it
    // scratch
    std::vector<uint64_t> need, need_half, diff, diff_half;
    std::vector<int64_t> diff_cnt;
    std::vector<uint32_t> row_cands, first, extra;
    std::vector<uint8_t> cut, listed;
    std::vector<std::pair<uint32_t, uint32_t>> heavy;  // {weight, strip row}

    uint32_t n_sr_active() const { return static_cast<uint32_t>(desc.size()); }  // entries of the work list
    uint32_t n_sr_whole() const { return static_cast<uint32_t>(desc_whole.size()); }
};

inline uint32_t PlanBandRows(const PlanInput &in) { return in.row1 - in.row0; }

// Worst-case binning-arena demand of every strip row of the band (plan->need, dwords).  The binning kernel bump-allocates inside
// these private regions, so the bound must be exact or larger.
// halves: also the same bound for the two halves of every strip row [2 i], [2 i + 1] (tiles 0-7, 8-15; plan->need_half), and the
// candidates of every strip row (plan->row_cands): what heavy strip rows are cut in two with.
inline void StripRowBounds(const PlanInput &in, BinPlan *plan, bool halves) {
    const uint8_t *meta = in.item_meta;
    uint32_t n, items_ix;
    std::memcpy(&n, meta, 4);
    std::memcpy(&items_ix, meta + 4, 4);
    const uint32_t rows = PlanBandRows(in);
    const size_t strips = in.strips_x;
    std::vector<uint64_t> &need = plan->need, &diff = plan->diff, &diff_half = plan->diff_half;
    std::vector<int64_t> &diff_cnt = plan->diff_cnt;
    need.assign(static_cast<size_t>(rows) * strips, 0);
    const size_t w = strips + 1;
    diff.assign((static_cast<size_t>(rows) + 1) * w, 0);
    const size_t wh = 2 * strips + 1;
    if (halves) diff_half.assign((static_cast<size_t>(rows) + 1) * wh, 0);
    if (halves) diff_cnt.assign((static_cast<size_t>(rows) + 1) * w, 0);
    plan->box.resize(4ull * n);
    plan->per.resize(n);
    plan->cands = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint16_t bb[4];
        std::memcpy(bb, meta + 8 + 8ull * i, 8);
        // (the box the plan is made for: the item's own, or widened by the margin on every side)
        bb[0] = static_cast<uint16_t>(std::max(0, static_cast<int>(bb[0]) - in.margin));
        bb[1] = static_cast<uint16_t>(std::max(0, static_cast<int>(bb[1]) - in.margin));
        bb[2] = static_cast<uint16_t>(std::min(65535, static_cast<int>(bb[2]) + in.margin));
        bb[3] = static_cast<uint16_t>(std::min(65535, static_cast<int>(bb[3]) + in.margin));
        std::memcpy(&plan->box[4ull * i], bb, 8);
        const uint64_t per = ItemArenaDwords(meta + items_ix + 32ull * i, in.margin);
        plan->per[i] = static_cast<uint32_t>(std::min<uint64_t>(per, 0xffffffffull));
        // strips: bz >= sx0 && bx < sx0 + 256 ; rows: bw >= y0 && by < y0 + 16
        const int64_t s_lo = bb[0] / 256, s_hi = std::min<int64_t>(bb[2] / 256, static_cast<int64_t>(strips) - 1);
        const int64_t r_lo = std::max<int64_t>(bb[1] / 16, in.row0), r_hi = std::min<int64_t>(bb[3] / 16, static_cast<int64_t>(in.row1) - 1);
        if (r_lo > r_hi || s_lo > s_hi) continue;
        plan->cands += static_cast<uint64_t>(r_hi - r_lo + 1) * static_cast<uint64_t>(s_hi - s_lo + 1);
        // (a 2-D difference array: four updates per item instead of one per strip row it covers -- config 5's
        //  7 600 items cover millions of them: arena sizing 0.26 -> 0.10 ms)
        const size_t a = static_cast<size_t>(r_lo - in.row0), b = static_cast<size_t>(r_hi - in.row0) + 1;
        diff[a * w + static_cast<size_t>(s_lo)] += per;
        diff[a * w + static_cast<size_t>(s_hi) + 1] -= per;
        diff[b * w + static_cast<size_t>(s_lo)] -= per;
        diff[b * w + static_cast<size_t>(s_hi) + 1] += per;
        if (halves) {
            diff_cnt[a * w + static_cast<size_t>(s_lo)] += 1;
            diff_cnt[a * w + static_cast<size_t>(s_hi) + 1] -= 1;
            diff_cnt[b * w + static_cast<size_t>(s_lo)] -= 1;
            diff_cnt[b * w + static_cast<size_t>(s_hi) + 1] += 1;
            // half strips: bz >= hx0 && bx < hx0 + 128
            const size_t h_lo = bb[0] / 128, h_hi = std::min<size_t>(bb[2] / 128, 2 * strips - 1);
            diff_half[a * wh + h_lo] += per;
            diff_half[a * wh + h_hi + 1] -= per;
            diff_half[b * wh + h_lo] -= per;
            diff_half[b * wh + h_hi + 1] += per;
        }
    }
    if (halves) {
        std::vector<uint32_t> &cnt = plan->row_cands;
        cnt.assign(static_cast<size_t>(rows) * strips, 0);
        for (size_t r = 0; r < rows; ++r) {
            int64_t run = 0;
            for (size_t sx = 0; sx < strips; ++sx) {
                run += diff_cnt[r * w + sx];
                cnt[r * strips + sx] = static_cast<uint32_t>(run + (r ? static_cast<int64_t>(cnt[(r - 1) * strips + sx]) : 0));
            }
        }
        std::vector<uint64_t> &need_half = plan->need_half;
        const size_t hs = 2 * strips;
        need_half.assign(static_cast<size_t>(rows) * hs, 0);
        for (size_t r = 0; r < rows; ++r) {
            uint64_t run = 0;
            for (size_t hx = 0; hx < hs; ++hx) {
                run += diff_half[r * wh + hx];
                need_half[r * hs + hx] = run + (r ? need_half[(r - 1) * hs + hx] : 0);
            }
        }
    }
    for (size_t r = 0; r < rows; ++r) {  // prefix sums along the strips, then down the rows (mod 2^64: the totals are exact)
        uint64_t run = 0;
        for (size_t sx = 0; sx < strips; ++sx) {
            run += diff[r * w + sx];
            need[r * strips + sx] = run + (r ? need[(r - 1) * strips + sx] : 0);
        }
    }
}

// Does `plan` still hold for the scene in `in`?  Same items in the same order, every item with no more arena need than it was
// planned with and its box inside the (widened) box it was planned with.
inline bool PlanStillHolds(const PlanInput &in, const BinPlan &plan) {
    const uint8_t *meta = in.item_meta;
    uint32_t n, items_ix;
    std::memcpy(&n, meta, 4);
    std::memcpy(&items_ix, meta + 4, 4);
    bool ok = plan.reusable && in.arena_cap != 0 && plan.band_identity && n == plan.per.size() && n == plan.band_item.size();
    for (uint32_t i = 0; i < n && ok; ++i) {
        uint16_t bb[4];
        std::memcpy(bb, meta + 8 + 8ull * i, 8);
        const uint16_t *pb = &plan.box[4ull * i];
        const uint64_t per = ItemArenaDwords(meta + items_ix + 32ull * i, 0);
        ok = per <= plan.per[i] && bb[0] >= pb[0] && bb[1] >= pb[1] && bb[2] <= pb[2] && bb[3] <= pb[3] && bb[2] >= bb[0] && bb[3] >= bb[1];
    }
    return ok;
}

// Makes the plan for `in` into *plan (the vectors' capacity is kept): the band's item list, the work list with its regions and
// chains, the sizes.  MakeSideLists makes the rest from it (plans without use_row_lists leave row_base, sr_list and the row_*
// scalars as they were -- nobody reads them).
// PM_ERR_CAPACITY: the arena regions pass kArenaLimit dwords; *plan is then half made and good for nothing: the caller starts
// over from BinPlan().
inline int MakeBinPlan(const PlanInput &in, BinPlan *plan) {
    const uint8_t *meta = in.item_meta;
    const uint32_t rows = PlanBandRows(in);
    const size_t strips = in.strips_x;
    plan->reusable = false;  // (until MakeSideLists has made the rest)
    bool may_split = in.bin_split_mode != 0 && in.one_launch_mode == 0;  // (scenes with per-tile-row item lists: decided below, once the band's list is made)
    StripRowBounds(in, plan, false);
    const std::vector<uint64_t> &need = plan->need, &need_half = plan->need_half;
    const std::vector<uint32_t> &row_cands = plan->row_cands;
    if (may_split && in.bin_split_mode == 1) {  // (cuts only while the plan's rows leave room in the resident grid: large frames pay for no second sizing pass)
        size_t n_rows = 0;
        for (size_t i = 0; i < need.size(); ++i) n_rows += need[i] != 0 ? 1u : 0u;
        may_split = n_rows < ResidentBinWorkgroups(in.n_cus, kBinWgPerCuUnset, kBinWgPerCu);
    }
    if (may_split) StripRowBounds(in, plan, true);
    plan->sr_empty_dwords = 0;  // (a strip row no item's bbox reaches has nothing reserved)
    // the items whose bbox reaches the band (rows: bw >= y0 && by < y1, PietRender.metal:198/:214), paint order
    std::vector<uint2> &bbs = plan->band_bbox;
    std::vector<uint32_t> &ids = plan->band_item;
    {
        bbs.clear();
        ids.clear();
        const uint32_t y0 = in.row0 * kTileH, y1 = in.row1 * kTileH;
        for (uint32_t i = 0; i < in.n_items; ++i) {
            uint32_t w[2];
            std::memcpy(w, meta + 8 + 8ull * i, 8);
            const uint16_t *pb = &plan->box[4ull * i];  // (the box the plan is made for: widened for a view change)
            const uint32_t bx = pb[0], by = pb[1], bw = pb[3];
            if (bw >= y0 && by < y1 && bx < in.strips_x * kGroupW) {
                bbs.push_back(make_uint2(w[0], w[1]));
                ids.push_back(i);
            }
        }
        // every item of the scene, in scene order: the kernels can read the scene's own boxes (nothing to upload, and the
        // list stays right for the next scene with the same items)
        plan->use_row_lists = static_cast<int>(ids.size()) >= in.row_list_min_items && !ids.empty();
        plan->band_identity = ids.size() == in.n_items && !plan->use_row_lists;
    }
    // The strip rows some item's bbox reaches get a workgroup of pm_bin_kernel each; the others are
    // background for as long as this scene and viewport last.  (An empty list still launches one
    // workgroup: it resets the frame counters.)
    std::vector<uint4> &desc = plan->desc;
    desc.clear();
    uint32_t per_cu = in.bin_wg_per_cu;
    if (per_cu == kBinWgPerCuUnset) per_cu = kBinWgPerCu;
    // Which strip rows are cut in two (bin_split_mode): the heaviest ones, as many as the resident grid has workgroups to spare.
    std::vector<uint8_t> &cut = plan->cut;
    cut.assign(need.size(), 0);
    plan->n_sr_split = 0;
    // (the plan is made with the frames' report whether or not it can cut: a report is read back once per plan at most,
    //  FeedBackStripRows -- round-6 advisor: scenes with per-tile-row item lists drained the pipeline every third frame)
    const bool fed = in.n_fb_slots == need.size();  // (frames of this scene and viewport have reported)
    plan->fb_applied = fed;
    if (may_split && !plan->use_row_lists) {  // (per-tile-row item lists are addressed by entry of the one work list)
        size_t n_rows = 0;
        for (size_t i = 0; i < need.size(); ++i) n_rows += ((need[i] + 3u) & ~3ull) != plan->sr_empty_dwords ? 1u : 0u;
        // (not to the last workgroup the chip holds: with all 1 280 places taken -- 171 rows cut at the 4K Tiger -- binning was 1.7 us
        //  SLOWER than with 1 214; the dispatcher's placement is not perfectly even, and a workgroup that has to wait for a place
        //  starts when a first one ends)
        const size_t resident = ResidentBinWorkgroups(in.n_cus, in.bin_wg_per_cu, kBinWgPerCu) * static_cast<size_t>(in.bin_split_fill) / 16u;
        const size_t room = in.bin_split_mode == 2 ? need.size() : (resident > n_rows ? resident - n_rows : 0u);
        std::vector<std::pair<uint32_t, uint32_t>> &heavy = plan->heavy;
        heavy.clear();
        for (size_t i = 0; i < need.size() && room != 0; ++i) {
            if (((need[i] + 3u) & ~3ull) == plan->sr_empty_dwords) continue;
            if (in.bin_split_mode == 2) heavy.emplace_back(row_cands[i], static_cast<uint32_t>(i));
            else if (fed ? in.fb_slots[i] >= in.bin_split_slots : row_cands[i] >= in.bin_split_cands) heavy.emplace_back(fed ? in.fb_slots[i] : row_cands[i], static_cast<uint32_t>(i));
        }
        if (heavy.size() > room) {
            std::partial_sort(heavy.begin(), heavy.begin() + static_cast<ptrdiff_t>(room), heavy.end(),
                              [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
            heavy.resize(room);
        }
        for (const auto &h : heavy) cut[h.second] = 1;
    }
    uint64_t total = kArenaBase;  // offset 0 means "no record"
    constexpr uint32_t kWholeStrip = 15u << 12, kLeftHalf = 7u << 12, kRightHalf = (7u << 12) | (8u << 8);  // tiles - 1 << 12 | first tile << 8
    auto push = [&](size_t i, uint32_t run, uint64_t need_dwords) -> bool {
        const uint64_t sz = (need_dwords + 3u) & ~3ull;
        if (sz == plan->sr_empty_dwords) return true;
        const uint64_t begin = total;
        total += sz;
        if (total > kArenaLimit) return false;
        desc.push_back(make_uint4(static_cast<uint32_t>(i % strips) | run | (static_cast<uint32_t>(i / strips) << 16), static_cast<uint32_t>(begin),
                                  static_cast<uint32_t>(total), 0u));
        return true;
    };
    for (size_t i = 0; i < need.size(); ++i) {
        bool ok = true;
        const size_t h = (i / strips) * 2 * strips + 2 * (i % strips);
        // (a half no item reaches gets no entry -- and nobody would write its pixels: such a row stays whole)
        if (cut[i] && ((need_half[h] + 3u) & ~3ull) != plan->sr_empty_dwords && ((need_half[h + 1] + 3u) & ~3ull) != plan->sr_empty_dwords) {
            ok = push(i, kLeftHalf, need_half[h]) && push(i, kRightHalf, need_half[h + 1]);
            plan->n_sr_split += 1;
        } else {
            ok = push(i, kWholeStrip, need[i]);
        }
        if (!ok) {
            plan->arena_total = total;
            return PM_ERR_CAPACITY;
        }
    }
    plan->arena_total = total;
    if (desc.empty()) desc.push_back(make_uint4(kWholeStrip, kArenaBase, kArenaBase, 0u));
    // (exact for a context's first scene; a quarter of headroom when it has to GROW: an animation's
    //  demand creeps from frame to frame, and re-allocating four 100 MB arenas costs milliseconds)
    const uint64_t alloc_dwords = total <= in.arena_cap ? in.arena_cap : (in.arena_cap == 0 ? total : std::min<uint64_t>(kArenaLimit, total + total / 4));
    plan->arena_alloc = std::max<uint32_t>(in.arena_cap, static_cast<uint32_t>(alloc_dwords));
    {
        // Tile arena (per-tile pieces + command lists, 16-byte quads): sized from what binning
        // actually finds, so there is no static bound; start generously (HBM is 288 GB), in proportion
        // to EVERY scene that comes (a max: what pm_sync grew it to is kept), and let pm_sync grow it on
        // overflow.
        uint64_t cmds = std::max<uint64_t>(1u << 22, 64ull * in.n_chunks * kChunkSegs);
        if (in.ptcl_initial_cmds != 0) cmds = in.ptcl_initial_cmds;  // tests: force the overflow -> grow -> re-render path
        // (a frame behind running frames may bin with a wave per strip row, Enqueue: records of 64 candidates instead of 256,
        //  up to four pieces -- four headers, four times the slack behind the candidates -- where a lone frame leaves one.  The
        //  arena a plan starts with holds that variant too: a frame that fits alone must not overflow in flight.  Round-4 advisor.)
        if (in.bin_waves_inflight == 1 && in.ptcl_initial_cmds == 0)
            cmds = std::max<uint64_t>(cmds, 80ull * in.n_chunks * kChunkSegs + 4ull * std::max<size_t>(static_cast<size_t>(rows) * in.tiles_x, 1));
        plan->ptcl_want = std::max<uint64_t>(in.ptcl_want, std::min<uint64_t>(cmds * kCmdQuadsNum / kCmdQuadsDen, 0x7fffffffull));
    }
    // (strip rows stay in their natural order: heaviest-first was measured 2.5 us slower -- the heavy
    //  ones then share CUs -- and so was a snake order over CU periods; neighbouring strip rows share
    //  data and belong together)
    {
        // pm_bin_kernel's grid is no larger than what the chip holds at once: five workgroups per CU (its LDS
        // is sized for that).  A group walks a chain of strip rows (desc.w = index of the next one, 0 = none):
        // row b, b + grid, b + 2 grid ... in natural order -- a grid larger than the residency would start its
        // last groups when the first END their chains.  Measured and not kept: any permutation of ALL rows, +25 %
        // (neighbouring strip rows share data); pairing the lightest rows by their arena need, +9 % (the need is
        // the worst case of the chunk test, not the work); rows DRAWN from counters instead of dealt (a returning
        // atomic per row, sent off a row ahead): config 5 0.229 -> 0.211 ms with a workgroup per row but config 4
        // 0.140 -> 0.150, and 0.195 -> 0.207 with a wave per row.
        const size_t n = desc.size();
        // A wave per strip row instead of a workgroup when there are several times more strip rows than the chip holds
        // workgroups AND the rows are light (a record of 64 candidates holds nearly every row's): sixteen one-wave
        // groups share a CU, no workgroup barriers, a quarter fewer vector and a third fewer scalar instructions per
        // strip row -- a row takes twice as long, three times as many are in flight.  Config 5 (16 160 rows of 11
        // candidates): binning 0.229 -> 0.195 ms, sustained +7 %; config 4 (4 096 rows of 108): 0.140 -> 0.162, stays
        // with workgroups; so does any frame whose rows all fit the chip at once (the 4K Tiger: 25 -> 52 us).
        const bool many_light_rows = n >= ResidentBinWorkgroups(in.n_cus, kBinWgPerCuUnset, kBinWgPerCu) * 3u && plan->cands <= 32ull * n;
        plan->bin_waves = in.bin_waves_env == 1 || in.bin_waves_env == 4 ? in.bin_waves_env : (many_light_rows ? 1u : 4u);
        if (plan->bin_waves == 1 && in.bin_wg_per_cu == kBinWgPerCuUnset) per_cu = 16u;
        const size_t grid = per_cu == 0 ? n : std::min<size_t>(n, static_cast<size_t>(in.n_cus) * per_cu);
        if (n > grid) {
            for (size_t i = 0; i + grid < n; ++i) desc[i].w = static_cast<uint32_t>(i + grid);
        }
        plan->bin_grid = static_cast<uint32_t>(grid);
    }
    return PM_OK;
}

// The per-tile-row item lists of a plan with use_row_lists (large scenes: every tile row gets its own item list each frame,
// pm_rowcull_kernel; the host only sizes the lists, with the kernel's predicate): row_base, sr_list and the row_* scalars (called by
// MakeSideLists).  PM_ERR_CAPACITY: the lists pass kArenaLimit entries.
inline int MakeRowLists(const PlanInput &in, BinPlan *plan) {
    const uint32_t rows = PlanBandRows(in);
    const std::vector<uint2> &bbs = plan->band_bbox;
    const std::vector<uint4> &desc = plan->desc;
    // A tile row's scan is cut into parts (workgroups of pm_rowcull_kernel), about four workgroups per CU in all, a part no
    // shorter than one step of the kernel: rb[r * parts + p] = where part p of row r writes.
    const uint32_t n_it = static_cast<uint32_t>(bbs.size());
    const uint32_t parts_wanted = std::max<uint32_t>(1u, (4u * static_cast<uint32_t>(in.n_cus)) / std::max<uint32_t>(rows, 1u));
    const uint64_t per_part = static_cast<uint64_t>(kRowCullStep) * parts_wanted;
    // (PM_ROW_LIST_PART_ITEMS: the tests cut small scenes into many parts)
    const uint32_t part_items = in.row_list_part_items != 0 ? static_cast<uint32_t>(in.row_list_part_items)
                                                             : kRowCullStep * static_cast<uint32_t>(std::max<uint64_t>(1u, (n_it + per_part - 1u) / per_part));
    const uint32_t parts = std::max<uint32_t>(1u, (n_it + part_items - 1u) / part_items);
    plan->row_parts = parts;
    plan->row_part_items = part_items;
    std::vector<uint32_t> &rb = plan->row_base;
    rb.assign(static_cast<size_t>(rows) * parts + 1, 0u);
    for (uint32_t k = 0; k < n_it; ++k) {
        const uint2 &b = bbs[k];
        const uint32_t by = b.x >> 16, bw = b.y >> 16;
        const uint32_t r_lo = std::max(by / kTileH, in.row0), r_hi = std::min(bw / kTileH, in.row1 - 1);
        const uint32_t pk = k / part_items;
        for (uint32_t r = r_lo; r <= r_hi && r_hi >= r_lo; ++r) rb[static_cast<size_t>(r - in.row0) * parts + pk + 1] += 1;
    }
    uint64_t run = 0;
    for (size_t i = 0; i < static_cast<size_t>(rows) * parts; ++i) {
        const uint32_t n_i = rb[i + 1];
        rb[i] = static_cast<uint32_t>(run);
        run += n_i;
    }
    if (run > kArenaLimit) return PM_ERR_CAPACITY;
    rb[static_cast<size_t>(rows) * parts] = static_cast<uint32_t>(run);
    plan->row_total = static_cast<uint32_t>(run);
    // every strip row's descriptor gets its tile row's {first entry, entries} next to it
    std::vector<uint2> &sl = plan->sr_list;
    sl.resize(desc.size());
    for (size_t i = 0; i < sl.size(); ++i) {
        const uint32_t r = desc[i].x >> 16;
        sl[i] = r < rows ? make_uint2(rb[static_cast<size_t>(r) * parts], rb[static_cast<size_t>(r + 1) * parts] - rb[static_cast<size_t>(r) * parts]) : make_uint2(0u, 0u);
    }
    plan->row_want = std::max<uint64_t>(run, 1);
    return PM_OK;
}

// The rest of a plan MakeBinPlan made, none of it needed for the work list itself: the work list without the cuts, the one-launch
// chains, the idle strip rows and (use_row_lists) the per-tile-row item lists.  Apart from MakeBinPlan because of when EnsureArena
// runs it: behind the uploads of the work list and the band list, whose way to the device hides this host work (a view change
// of a large scene is bound by the host; with everything in front of the uploads config 5's re-plan took 0.78 instead of 0.74 ms).
// PM_ERR_CAPACITY: MakeRowLists'.
inline int MakeSideLists(const PlanInput &in, BinPlan *plan) {
    const std::vector<uint4> &desc = plan->desc;
    const std::vector<uint64_t> &need = plan->need;
    const size_t strips = in.strips_x;
    {
        // the work list without the cuts: the two halves of a cut strip row lie next to each other, in the list and in the arena
        std::vector<uint4> &whole = plan->desc_whole;
        whole.clear();
        for (size_t k = 0; k < desc.size() && plan->n_sr_split != 0; ++k) {
            const uint32_t key = desc[k].x & 0xffff00ffu;
            if (!whole.empty() && (whole.back().x & 0xffff00ffu) == key) whole.back().z = desc[k].z;
            else whole.push_back(make_uint4(key | (15u << 12), desc[k].y, desc[k].z, 0u));
        }
        // (chained for the plan's grid like the list with the cuts: frames that bind this list run min(grid, rows) groups, Enqueue,
        //  and with more rows than the grid -- PM_BIN_SPLIT=2, or PM_BIN_WG_PER_CU=1 at 1080p -- a row past the grid is reached by
        //  its chain only.  Round-6 advisor: unchained, those rows were never binned and their tiles stayed unrendered.)
        for (size_t k = 0; k + plan->bin_grid < whole.size(); ++k) whole[k].w = static_cast<uint32_t>(k + plan->bin_grid);
    }
    {
        // Chains of the one-launch grid (four workgroups per CU, all resident): workgroup b bins strip row b; with more strip rows
        // than workgroups the rows beyond go, heaviest first, to the workgroups whose own row is lightest (by the arena bound,
        // the only estimate there is) -- a second light row ends before the frame's heaviest row does.
        std::vector<uint32_t> &nx = plan->next_one;
        const size_t n = desc.size();
        nx.assign(n, 0u);
        const size_t resident = static_cast<size_t>(in.n_cus) * in.frame_wg_per_cu;
        plan->one_grid_rows = 0;
        if (in.one_launch_mode != 0 && resident != 0 && n <= 2 * resident) {  // (only a context that renders one-launch frames pays for their lists)
            const size_t rows_one = std::min(n, resident);
            plan->one_grid_rows = static_cast<uint32_t>(rows_one);
            if (n > rows_one) {
                std::vector<uint32_t> &first = plan->first, &extra = plan->extra;
                first.resize(rows_one);
                extra.resize(n - rows_one);
                for (size_t i = 0; i < rows_one; ++i) first[i] = static_cast<uint32_t>(i);
                for (size_t i = rows_one; i < n; ++i) extra[i - rows_one] = static_cast<uint32_t>(i);
                auto weight = [&](uint32_t i) { return desc[i].z - desc[i].y; };
                std::stable_sort(first.begin(), first.end(), [&](uint32_t a, uint32_t b) { return weight(a) < weight(b); });
                std::stable_sort(extra.begin(), extra.end(), [&](uint32_t a, uint32_t b) { return weight(a) > weight(b); });
                for (size_t k = 0; k < extra.size(); ++k) nx[first[k]] = extra[k];
            }
        }
    }
    {
        // the strip rows without a workgroup: the binning launch (clear_in_bin) or a one-launch frame writes their (background) pixels from this list
        std::vector<uint32_t> &idle = plan->idle;
        idle.clear();
        std::vector<uint8_t> &listed = plan->listed;  // (the empty list's one workgroup "has" strip row 0; a strip row cut in two is listed twice)
        listed.assign(need.size(), 0);
        for (const uint4 &d : desc) {
            const size_t i = static_cast<size_t>(d.x >> 16) * strips + (d.x & 0xffu);
            if (i < listed.size()) listed[i] = 1;
        }
        for (size_t i = 0; i < need.size() && (plan->one_grid_rows != 0 || in.fold_clear_mode >= 3); ++i)
            if (!listed[i]) idle.push_back(static_cast<uint32_t>(i));
    }
    if (plan->use_row_lists && MakeRowLists(in, plan) != PM_OK) return PM_ERR_CAPACITY;
    plan->reusable = in.margin > 0 && plan->band_identity;
    return PM_OK;
}

}  // namespace pm
