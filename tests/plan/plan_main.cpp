// TEST INFRASTRUCTURE: runs the binning planner (piet_metal_amd/csrc/pm_plan.h) on the CPU.  Built by tests/test_plan_cpu.py
// against tests/emu/include; never part of the product.
//
//   plan_main <cases.bin> <out.bin>
//
// Reads the cases the test wrote, makes every plan, checks the plan's invariants itself (a violated one is reported on stderr and
// the program exits with 1) and writes every output array and scalar back for the test to compare with the recorded digests.
//
// cases.bin: u32 n_cases, then per case
//   u32 x 21  n_items n_chunks tiles_x strips_x row0 row1 n_cus margin bin_split_mode bin_split_cands bin_split_slots bin_split_fill
//             bin_wg_per_cu bin_waves_env bin_waves_inflight one_launch_mode frame_wg_per_cu fold_clear_mode row_list_min_items
//             row_list_part_items arena_cap
//   u64 x 2   ptcl_initial_cmds ptcl_want
//   u32 n_fb, u32 fb[n_fb]
//   u64 meta_len, bytes          header + boxes + items
//   u64 next_len, bytes          (0: none) the next scene's, for PlanStillHolds against the plan just made
// out.bin: per case  u64 x kScalars (rc first), then per array u64 n_bytes + bytes (arrays only when rc == 0)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pm_plan.h"

namespace {

int g_case = 0;
bool g_bad = false;

#define CHECK(cond, ...)                                           \
    do {                                                           \
        if (!(cond)) {                                             \
            std::fprintf(stderr, "case %d: %s: ", g_case, #cond);  \
            std::fprintf(stderr, __VA_ARGS__);                     \
            std::fprintf(stderr, "\n");                            \
            g_bad = true;                                          \
            return;                                                \
        }                                                          \
    } while (0)

struct Reader {
    FILE *f;
    template <typename T>
    T get() {
        T v{};
        if (std::fread(&v, sizeof(T), 1, f) != 1) {
            std::fprintf(stderr, "short case file\n");
            std::exit(2);
        }
        return v;
    }
    template <typename T>
    std::vector<T> vec(size_t n) {
        std::vector<T> v(n);
        if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
            std::fprintf(stderr, "short case file\n");
            std::exit(2);
        }
        return v;
    }
};

struct Box {
    uint32_t x0, y0, x1, y1;
};

// item i's box as the plan is made for it (widened by the margin, clamped) and its own
Box ItemBox(const uint8_t *meta, uint32_t i, int margin) {
    uint16_t bb[4];
    std::memcpy(bb, meta + 8 + 8ull * i, 8);
    Box b;
    b.x0 = static_cast<uint32_t>(std::max(0, static_cast<int>(bb[0]) - margin));
    b.y0 = static_cast<uint32_t>(std::max(0, static_cast<int>(bb[1]) - margin));
    b.x1 = static_cast<uint32_t>(std::min(65535, static_cast<int>(bb[2]) + margin));
    b.y1 = static_cast<uint32_t>(std::min(65535, static_cast<int>(bb[3]) + margin));
    return b;
}

// An item record's arena dwords, restated from the arena's layout (pm_device.h) and not through pm::ItemArenaDwords: a fill has
// as many segments as points, a polyline one fewer, a line one, anything else none; a plan made to last (margin > 0) leaves room
// for a quarter more and two chunks, lines excepted; a chunk is four segments, a segment slot 16 B + a meta word; four dwords on top.
uint64_t NaiveItemDwords(const uint8_t *item, int margin) {
    uint32_t w[8];
    std::memcpy(w, item, 32);
    const uint32_t tag = w[0] & 0xffffu;
    uint64_t segs = tag == pm::kItemFill ? w[3] : tag == pm::kItemPoly ? (w[3] >= 2 ? w[3] - 1 : 0) : tag == pm::kItemLine ? 1 : 0;
    if (margin > 0 && tag != pm::kItemLine) segs = segs + segs / 4 + 8;
    const uint64_t chunks = segs / 4 + (segs % 4 ? 1 : 0);
    return 4 + chunks * 4 * 5;
}

// The arena bound of the pixel columns [px0, px1) of tile row `row`, item by item, with the binning kernel's predicates:
// strips bz >= sx0 && bx < sx0 + 256, rows bw >= y0 && by < y0 + 16
uint64_t NaiveBound(const pm::PlanInput &in, uint32_t row, uint32_t px0, uint32_t px1) {
    uint32_t n, items_ix;
    std::memcpy(&n, in.item_meta, 4);
    std::memcpy(&items_ix, in.item_meta + 4, 4);
    const uint32_t y0 = row * pm::kTileH;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const Box b = ItemBox(in.item_meta, i, in.margin);
        if (b.x1 >= px0 && b.x0 < px1 && b.y1 >= y0 && b.y0 < y0 + pm::kTileH) sum += NaiveItemDwords(in.item_meta + items_ix + 32ull * i, in.margin);
    }
    return sum;
}

// heads 0 .. grid - 1, every chain followed to its end: every entry exactly once
bool ChainsCoverOnce(const std::vector<uint4> &list, size_t grid) {
    std::vector<uint8_t> seen(list.size(), 0);
    size_t visited = 0;
    for (size_t h = 0; h < grid && h < list.size(); ++h) {
        for (size_t k = h;;) {
            if (k >= list.size() || seen[k]) return false;
            seen[k] = 1;
            visited += 1;
            if (list[k].w == 0u) break;
            k = list[k].w;
        }
    }
    return visited == list.size();
}

void CheckPlan(const pm::PlanInput &in, const pm::BinPlan &plan) {
    const uint32_t rows = in.row1 - in.row0;
    const size_t strips = in.strips_x, n_sr = static_cast<size_t>(rows) * strips;
    const std::vector<uint4> &desc = plan.desc;
    CHECK(!desc.empty(), "empty work list");
    // arena regions
    std::vector<uint32_t> listed(n_sr, 0);
    uint64_t at = pm::kArenaBase;
    const bool dummy = desc.size() == 1 && desc[0].y == desc[0].z;
    for (size_t k = 0; k < desc.size(); ++k) {
        const uint4 d = desc[k];
        const uint32_t strip = d.x & 0xffu, first = (d.x >> 8) & 0xfu, tiles = ((d.x >> 12) & 0xfu) + 1u, row = d.x >> 16;
        CHECK(row < rows && strip < strips && first + tiles <= pm::kStripTiles, "entry %zu names strip row %u/%u tiles %u+%u", k, row, strip, first, tiles);
        CHECK(d.y == at && d.z >= d.y, "entry %zu region [%u, %u) does not follow %" PRIu64, k, d.y, d.z, at);
        CHECK((d.z - d.y) % 4u == 0, "entry %zu region of %u dwords", k, d.z - d.y);
        const uint32_t px0 = strip * pm::kGroupW + first * pm::kTileW;
        const uint64_t bound = NaiveBound(in, in.row0 + row, px0, px0 + tiles * pm::kTileW);
        CHECK(d.z - d.y >= bound, "entry %zu region of %u dwords, bound %" PRIu64, k, d.z - d.y, bound);
        CHECK(dummy || d.z > d.y, "entry %zu is empty", k);
        at = d.z;
        listed[static_cast<size_t>(row) * strips + strip] += 1;
        if (tiles != pm::kStripTiles) {  // a cut row: two non-empty halves next to each other
            CHECK(tiles == 8 && (first == 0 || first == 8), "entry %zu is no half", k);
            const size_t o = first == 0 ? k + 1 : k - 1;
            CHECK(o < desc.size() && (desc[o].x & 0xffff00ffu) == (d.x & 0xffff00ffu) && ((desc[o].x >> 8) & 0xfu) == 8u - first && desc[o].z > desc[o].y && d.z > d.y,
                  "entry %zu has no other half", k);
        }
    }
    CHECK(at == plan.arena_total && plan.arena_total <= pm::kArenaLimit && plan.arena_alloc >= plan.arena_total && plan.arena_alloc >= in.arena_cap, "arena total %" PRIu64, plan.arena_total);
    size_t n_cut = 0;
    for (size_t i = 0; i < n_sr; ++i) {
        const uint32_t sx = static_cast<uint32_t>(i % strips);
        const uint64_t bound = NaiveBound(in, in.row0 + static_cast<uint32_t>(i / strips), sx * pm::kGroupW, (sx + 1) * pm::kGroupW);
        CHECK(listed[i] <= 2 && (dummy || (listed[i] != 0) == (bound != 0)), "strip row %zu listed %u times, bound %" PRIu64, i, listed[i], bound);
        CHECK(bound == plan.need[i], "strip row %zu: bound %" PRIu64 ", need %" PRIu64, i, bound, plan.need[i]);
        n_cut += listed[i] == 2 ? 1u : 0u;
    }
    CHECK(n_cut == plan.n_sr_split, "%zu rows cut, n_sr_split %u", n_cut, plan.n_sr_split);
    // chains
    CHECK(plan.bin_grid >= 1 && plan.bin_grid <= desc.size(), "grid %u", plan.bin_grid);
    CHECK(ChainsCoverOnce(desc, plan.bin_grid), "the chains of the work list");
    // the whole-row list: the cut list with neighbouring halves merged, the same regions, chained for the same grid
    std::vector<uint4> merged;
    for (size_t k = 0; k < desc.size() && n_cut != 0; ++k) {
        const uint32_t key = desc[k].x & 0xffff00ffu;
        if (!merged.empty() && (merged.back().x & 0xffff00ffu) == key) merged.back().z = desc[k].z;
        else merged.push_back(make_uint4(key | (15u << 12), desc[k].y, desc[k].z, 0u));
    }
    CHECK(merged.size() == plan.desc_whole.size() && (n_cut == 0 || merged.size() + n_cut == desc.size()), "whole-row list of %zu entries", plan.desc_whole.size());
    for (size_t k = 0; k < merged.size(); ++k)
        CHECK(merged[k].x == plan.desc_whole[k].x && merged[k].y == plan.desc_whole[k].y && merged[k].z == plan.desc_whole[k].z, "whole-row entry %zu", k);
    CHECK(ChainsCoverOnce(plan.desc_whole, plan.bin_grid), "the chains of the whole-row list");
    // idle strip rows
    if (plan.one_grid_rows != 0 || in.fold_clear_mode >= 3) {
        std::vector<uint8_t> idle(n_sr, 0);
        for (uint32_t i : plan.idle) {
            CHECK(i < n_sr && !idle[i], "idle strip row %u", i);
            idle[i] = 1;
        }
        for (size_t i = 0; i < n_sr; ++i) CHECK((listed[i] != 0) != (idle[i] != 0), "strip row %zu listed %u idle %u", i, listed[i], idle[i]);
    } else {
        CHECK(plan.idle.empty(), "an idle list nobody asked for");
    }
    // one-launch chains
    CHECK(plan.next_one.size() == desc.size(), "one-launch chains of %zu", plan.next_one.size());
    {
        std::vector<uint8_t> pred(desc.size(), 0);
        for (size_t k = 0; k < plan.next_one.size(); ++k) {
            const uint32_t nx = plan.next_one[k];
            if (nx == 0) continue;
            CHECK(plan.one_grid_rows != 0 && k < plan.one_grid_rows && nx >= plan.one_grid_rows && nx < desc.size() && !pred[nx], "one-launch chain %zu -> %u", k, nx);
            pred[nx] = 1;
        }
        for (size_t k = plan.one_grid_rows; k < desc.size() && plan.one_grid_rows != 0; ++k) CHECK(pred[k], "entry %zu past the resident ones has no predecessor", k);
        if (in.one_launch_mode != 0) CHECK((plan.one_grid_rows != 0) == (static_cast<size_t>(in.n_cus) * in.frame_wg_per_cu != 0 && desc.size() <= 2ull * in.n_cus * in.frame_wg_per_cu), "one_grid_rows %u", plan.one_grid_rows);
        else CHECK(plan.one_grid_rows == 0, "one_grid_rows %u", plan.one_grid_rows);
    }
    // the band's item list
    const uint32_t by0 = in.row0 * pm::kTileH, by1 = in.row1 * pm::kTileH;
    std::vector<uint32_t> band;
    for (uint32_t i = 0; i < in.n_items; ++i) {
        const Box b = ItemBox(in.item_meta, i, in.margin);
        if (b.y1 >= by0 && b.y0 < by1 && b.x0 < in.strips_x * pm::kGroupW) band.push_back(i);
    }
    CHECK(band == plan.band_item && plan.band_bbox.size() == band.size(), "band list of %zu items, %zu expected", plan.band_item.size(), band.size());
    for (size_t k = 0; k < band.size(); ++k) CHECK(std::memcmp(&plan.band_bbox[k], in.item_meta + 8 + 8ull * band[k], 8) == 0, "band box %zu", k);
    bool in_order = band.size() == in.n_items;
    for (size_t k = 0; k < band.size() && in_order; ++k) in_order = band[k] == k;
    CHECK(!plan.band_identity || (in_order && !plan.use_row_lists), "band_identity");
    CHECK(plan.use_row_lists == (!band.empty() && static_cast<int>(band.size()) >= in.row_list_min_items), "use_row_lists");
    CHECK(plan.reusable == (in.margin > 0 && plan.band_identity), "reusable");
    // per-tile-row lists
    if (plan.use_row_lists) {
        const uint32_t parts = plan.row_parts, pi = plan.row_part_items;
        CHECK(pi >= 1 && parts == std::max<uint32_t>(1u, static_cast<uint32_t>((band.size() + pi - 1) / pi)), "%u parts of %u items", parts, pi);
        CHECK(in.row_list_part_items == 0 || pi == static_cast<uint32_t>(in.row_list_part_items), "part of %u items", pi);
        CHECK(plan.row_base.size() == static_cast<size_t>(rows) * parts + 1, "row_base of %zu", plan.row_base.size());
        uint64_t run = 0;
        for (uint32_t r = 0; r < rows; ++r) {
            const uint32_t y0 = (in.row0 + r) * pm::kTileH;
            for (uint32_t p = 0; p < parts; ++p) {
                CHECK(plan.row_base[static_cast<size_t>(r) * parts + p] == run, "row_base[%u, %u]", r, p);
                for (size_t k = static_cast<size_t>(p) * pi; k < band.size() && k < (static_cast<size_t>(p) + 1) * pi; ++k) {
                    const Box b = ItemBox(in.item_meta, band[k], 0);  // (pm_rowcull_kernel reads the items' own boxes)
                    run += b.y1 >= y0 && b.y0 < y0 + pm::kTileH ? 1u : 0u;
                }
            }
        }
        CHECK(plan.row_base.back() == run && plan.row_total == run && plan.row_want == std::max<uint64_t>(run, 1), "row lists of %u entries, %" PRIu64 " expected", plan.row_total, run);
        CHECK(plan.sr_list.size() == desc.size(), "sr_list of %zu", plan.sr_list.size());
        for (size_t k = 0; k < desc.size(); ++k) {
            const uint32_t r = desc[k].x >> 16;
            const uint32_t b = plan.row_base[static_cast<size_t>(r) * parts], e = plan.row_base[static_cast<size_t>(r + 1) * parts];
            CHECK(plan.sr_list[k].x == b && plan.sr_list[k].y == e - b, "sr_list[%zu]", k);
        }
        CHECK(plan.n_sr_split == 0, "cuts and per-tile-row lists");
    }
}

struct Writer {
    FILE *f;
    void u64(uint64_t v) { std::fwrite(&v, 8, 1, f); }
    template <typename T>
    void arr(const std::vector<T> &v) {
        u64(v.size() * sizeof(T));
        if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    }
};

}  // namespace

// plan_main --row-lists-limit: MakeRowLists on a hand-set band list of 2^20 items in each of 4 096 tile rows, 2^32 entries -- out of
// reach through MakeBinPlan, whose arena check fails such a scene first.  PM_ERR_CAPACITY.  (4 x 10^9 steps of its loop: a quarter of a minute under the sanitizers.)
int RowListsLimit() {
    pm::PlanInput in;
    in.tiles_x = in.strips_x = 1;
    in.row1 = 4096;
    in.n_cus = 2;
    in.row_list_part_items = 1 << 30;
    pm::BinPlan plan;
    plan.use_row_lists = true;
    plan.desc.push_back(make_uint4(15u << 12, pm::kArenaBase, pm::kArenaBase + 4, 0u));
    plan.band_bbox.assign(1u << 20, make_uint2(0u, (65535u << 16) | 15u));
    const int rc = pm::MakeRowLists(in, &plan);
    if (rc != PM_ERR_CAPACITY) std::fprintf(stderr, "row lists of 2^32 entries: %d\n", rc);
    return rc == PM_ERR_CAPACITY ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--row-lists-limit") return RowListsLimit();
    if (argc != 3) return 2;
    FILE *fi = std::fopen(argv[1], "rb"), *fo = std::fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    Reader rd{fi};
    Writer wr{fo};
    const uint32_t n_cases = rd.get<uint32_t>();
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        g_case = static_cast<int>(ci);
        pm::PlanInput in;
        in.n_items = rd.get<uint32_t>();
        in.n_chunks = rd.get<uint32_t>();
        in.tiles_x = rd.get<uint32_t>();
        in.strips_x = rd.get<uint32_t>();
        in.row0 = rd.get<uint32_t>();
        in.row1 = rd.get<uint32_t>();
        in.n_cus = static_cast<int>(rd.get<uint32_t>());
        in.margin = static_cast<int>(rd.get<uint32_t>());
        in.bin_split_mode = static_cast<int>(rd.get<uint32_t>());
        in.bin_split_cands = rd.get<uint32_t>();
        in.bin_split_slots = rd.get<uint32_t>();
        in.bin_split_fill = rd.get<uint32_t>();
        in.bin_wg_per_cu = rd.get<uint32_t>();
        in.bin_waves_env = rd.get<uint32_t>();
        in.bin_waves_inflight = rd.get<uint32_t>();
        in.one_launch_mode = static_cast<int>(rd.get<uint32_t>());
        in.frame_wg_per_cu = rd.get<uint32_t>();
        in.fold_clear_mode = static_cast<int>(rd.get<uint32_t>());
        in.row_list_min_items = static_cast<int>(rd.get<uint32_t>());
        in.row_list_part_items = static_cast<int>(rd.get<uint32_t>());
        in.arena_cap = rd.get<uint32_t>();
        in.ptcl_initial_cmds = rd.get<uint64_t>();
        in.ptcl_want = rd.get<uint64_t>();
        const std::vector<uint32_t> fb = rd.vec<uint32_t>(rd.get<uint32_t>());
        const std::vector<uint8_t> meta = rd.vec<uint8_t>(rd.get<uint64_t>());
        const std::vector<uint8_t> next = rd.vec<uint8_t>(rd.get<uint64_t>());
        in.fb_slots = fb.data();
        in.n_fb_slots = fb.size();
        in.item_meta = meta.data();
        pm::BinPlan plan;
        int rc = pm::MakeBinPlan(in, &plan);
        if (rc == PM_OK) rc = pm::MakeSideLists(in, &plan);
        if (rc != PM_OK && rc != PM_ERR_CAPACITY) {
            std::fprintf(stderr, "case %u: MakeBinPlan returned %d\n", ci, rc);
            g_bad = true;
        }
        if (rc == PM_OK) CheckPlan(in, plan);
        uint64_t holds = 2;  // (not asked)
        if (rc == PM_OK && !next.empty()) {
            pm::PlanInput in2 = in;
            in2.item_meta = next.data();
            in2.arena_cap = plan.arena_alloc;
            in2.ptcl_want = plan.ptcl_want;
            holds = pm::PlanStillHolds(in2, plan) ? 1u : 0u;
        }
        wr.u64(static_cast<uint64_t>(static_cast<int64_t>(rc)));
        if (rc != PM_OK) continue;
        for (uint64_t v : {plan.cands, uint64_t{plan.n_sr_split}, uint64_t{plan.bin_waves}, uint64_t{plan.bin_grid}, uint64_t{plan.one_grid_rows},
                           uint64_t{plan.use_row_lists}, uint64_t{plan.band_identity}, uint64_t{plan.row_parts}, uint64_t{plan.row_part_items},
                           uint64_t{plan.row_total}, plan.row_want, uint64_t{plan.sr_empty_dwords}, plan.arena_total, uint64_t{plan.arena_alloc},
                           plan.ptcl_want, uint64_t{plan.fb_applied}, uint64_t{plan.reusable}, holds})
            wr.u64(v);
        wr.arr(plan.desc);
        wr.arr(plan.desc_whole);
        wr.arr(plan.next_one);
        wr.arr(plan.idle);
        wr.arr(plan.band_bbox);
        wr.arr(plan.band_item);
        wr.arr(plan.row_base);
        wr.arr(plan.sr_list);
        wr.arr(plan.need);
        wr.arr(plan.box);
        wr.arr(plan.per);
    }
    std::fclose(fi);
    if (std::fclose(fo) != 0) return 2;
    return g_bad ? 1 : 0;
}
