// Stand-alone host check of the JPEG coders' plans and workspace carves (csrc/jpeg_u8.h and the two units that use it), for a run under
// the host sanitizers on a machine without a GPU: nothing here touches the device.  It includes a unit whole, because the plans are
// static to their unit; build it once per unit (tools/README.md has the two command lines):
//     default                  jpeg_u8.hip: the baseline and the optimised plan
//     -DCIAOSR_CHECK_PROG      jpeg_prog_u8.hip: the progressive plan
// For every rect list of tests/test_jpeg_sizes_host.py, every mode and every mcus_per_chunk it runs the plan with the table fill, reads
// the whole table back (crops, chunks, streams: every range closed, in order and inside its crop) and carves the workspace from offsets
// alone, at the exported size (must fit) and one byte below it (must not).  Prints one line per kind; exit status 0: all held.
#ifdef CIAOSR_CHECK_PROG
#include "../ciaosr_amd/csrc/jpeg_prog_u8.hip"
#else
#include "../ciaosr_amd/csrc/jpeg_u8.hip"
#endif
#include <cstdio>

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("FAILED %s (line %d, case %s)\n", #cond, __LINE__, what); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

// tiles [nt] and their chunks [nc] as the device walks them: every tile's chunks follow the one before, cover [0, nmcu) in steps of at
// most `per`, and the tiles' first blocks add up
static void walk(const TileT* tiles, int nt, const ChunkT* chunks, int nc, u64 per, u64 units_per_mcu, const char* what) {
    u32 c = 0;
    u64 first = 0;
    for (int k = 0; k < nt; ++k) {
        EXPECT(tiles[k].first_chunk == c && tiles[k].block0 == first && tiles[k].nmcu > 0);
        for (int m = 0; m < tiles[k].nmcu; ++c) {
            EXPECT((int)c < nc);
            if ((int)c >= nc) return;
            EXPECT(chunks[c].tile == k && chunks[c].mcu0 == m && chunks[c].mcu1 > m && chunks[c].mcu1 <= tiles[k].nmcu);
            EXPECT((u64)(chunks[c].mcu1 - m) <= per);
            m = chunks[c].mcu1;
        }
        first += (u64)tiles[k].nmcu * units_per_mcu;
    }
    EXPECT((int)c == nc);
}

template <typename W, typename P>
static void carve_check(const P& t, const char* what) {
    const size_t need = work_bytes<W>(t);
    EXPECT(need > 0);
    static char origin[1];
    for (int short_by = 0; short_by < 2; ++short_by) {
        Arena a(origin, need - short_by);
        W w;
        w.carve(a, t);
        EXPECT(a.ok == (short_by == 0) && a.off == need);
        const uintptr_t base = reinterpret_cast<uintptr_t>(a.base), table = reinterpret_cast<uintptr_t>(w.s.table), ubuf = reinterpret_cast<uintptr_t>(w.s.ubuf);
        EXPECT(table == base && ubuf % 256 == base % 256 && ubuf + 4 * ((t.ubytes + 3) / 4) <= base + need);
    }
}

static void check_crops(const Request& r, const CropPlan& t, const std::vector<unsigned char>& table, const char* what) {
    EXPECT(table.size() == t.table_bytes && t.nt == r.n && t.capacity > 0 && t.ubytes > 0);
    const TileT* crops = reinterpret_cast<const TileT*>(table.data() + t.o_crops);
    walk(crops, t.nt, reinterpret_cast<const ChunkT*>(table.data() + t.o_cchunks), t.ncc, (u64)t.per, (u64)blocks_per_mcu(t.mode), what);
    u64 blocks = 0;
    for (int k = 0; k < r.n; ++k) {
        EXPECT(crops[k].y0 == r.rects[4 * k] && crops[k].x0 == r.rects[4 * k + 1] && crops[k].h == r.rects[4 * k + 2] && crops[k].w == r.rects[4 * k + 3]);
        blocks += (u64)crops[k].nmcu * (u64)blocks_per_mcu(t.mode);
    }
    EXPECT(blocks == t.blocks);
}

static void one(const int* rects, int n, int mode, int mcus, int H, int W, bool accepted, const char* what) {
    const Request r{nullptr, 0, H, W, 0, rects, n, 90, mode, mcus};
#ifdef CIAOSR_CHECK_PROG
    std::vector<unsigned char> table;
    const ProgPlan t = plan(r, &table);
    EXPECT((t.rc == CIAOSR_OK) == (accepted && mode != kModeGrey));
    if (t.rc != CIAOSR_OK) {
        EXPECT(table.empty() && work_bytes<ProgWork>(t) == 0 && t.capacity == 0);
        return;
    }
    check_crops(r, t, table, what);
    EXPECT(t.ns == kScans * n && t.per_items == (u64)t.per * (u64)blocks_per_mcu(mode));
    walk(reinterpret_cast<const TileT*>(table.data() + t.o_streams), t.ns, reinterpret_cast<const ChunkT*>(table.data() + t.o_chunks), t.nc, t.per_items,
         1, what);
    carve_check<ProgWork>(t, what);
#else
    for (int opt = 0; opt < 2; ++opt) {
        std::vector<unsigned char> table;
        const Plan t = plan(r, opt != 0, &table);
        EXPECT((t.rc == CIAOSR_OK) == accepted);
        if (t.rc != CIAOSR_OK) {
            EXPECT(table.empty() && work_bytes<Work>(t) == 0 && t.capacity == 0);
            continue;
        }
        check_crops(r, t, table, what);
        EXPECT(t.ns == t.nt && t.nc == t.ncc);
        carve_check<Work>(t, what);
    }
#endif
}

int main() {
    static const int lists[][20] = {{0, 0, 1, 1},
                                    {0, 0, 64, 31, 5, 7, 33, 65, 63, 199, 1, 1},
                                    {0, 0, 1000, 18256, 3, 5, 255, 255, 10, 10, 1, 1, 0, 0, 65535, 1, 7, 7, 9, 65535}};
    static const int counts[] = {1, 3, 5};
    static const int refused[][8] = {{0, 0, 0, 5}, {0, 0, 5, 0}, {0, 0, 65536, 5}, {0, 0, 5, 5, 0, -1, 5, 5}, {-1, 0, 5, 5}};
    static const int refused_counts[] = {1, 1, 1, 2, 1};
    static const int mcus[] = {0, 1, 5, 128};
    int cases = 0;
    for (int mode = kMode444; mode <= kModeGrey; ++mode) {
        for (int l = 0; l < 3; ++l)
            for (int m = 0; m < 4; ++m, ++cases) one(lists[l], counts[l], mode, mcus[m], 0, 0, true, "accepted list");
        for (int l = 0; l < 5; ++l, ++cases) one(refused[l], refused_counts[l], mode, 0, 0, 0, false, "refused list");
        one(lists[1], 3, mode, 0, 64, 200, true, "list inside its image");
        one(lists[1], 3, mode, 0, 64, 199, false, "list outside its image");
        one(lists[0], 1, mode, -1, 0, 0, false, "negative mcus");
        one(nullptr, 1, mode, 0, 0, 0, false, "null list");
        one(lists[0], 0, mode, 0, 0, 0, false, "no rects");
        cases += 5;
    }
    one(lists[0], 1, -1, 0, 0, 0, false, "unknown mode");
#ifdef CIAOSR_CHECK_PROG
    std::printf("jpeg_plan_check (progressive plan): %d cases, %d failures\n", cases + 1, failures);
#else
    std::printf("jpeg_plan_check (baseline and optimised plan): %d cases, %d failures\n", cases + 1, failures);
#endif
    return failures ? 1 : 0;
}
