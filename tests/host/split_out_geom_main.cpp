// Stand-alone check of the host-side geometry of the persistent output convolution (cwfa_amd/csrc/conv_split_out_geom.h): the packed
// image's index arithmetic and the tile walk.  Plain C++ with its own main; tests/test_split_out_cpu.py builds it with
// -fsanitize=address,undefined and runs it.  Every index is used to address a buffer of exactly the size the library allocates, so
// an index out of range is a sanitizer report, and every count is checked.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_split_out_geom.h"

using namespace cwfa_out;

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
            ++fails;                      \
        }                                 \
    } while (0)

// the pack map of a bank with `cout` rows: every 16-byte element of the image is written exactly once, every weight of the bank is
// read exactly once, nothing outside either
static void check_pack(int cout) {
    const int mt = mt_of(cout), rows = 16 * mt;
    CHECK(mt >= 1 && mt <= MAX_MT, "cout %d: %d m-tiles", cout, mt);
    CHECK(packed_bytes(cout) == (int64_t)NSL * slice_bytes(mt) && slice_bytes(mt) == 3 * 4 * rows * 16, "cout %d: image size", cout);
    std::vector<int> dst((size_t)(packed_bytes(cout) / 16), 0);
    std::vector<int> src((size_t)cout * CIN * 9, 0);
    for (int sl = 0; sl < NSL; ++sl)
        for (int g = 0; g < 4; ++g)
            for (int co = 0; co < rows; ++co) {
                for (int q = 0; q < 3; ++q) {
                    // slice sl occupies [sl * slice_bytes, (sl + 1) * slice_bytes): the DMA of a step reads exactly that range
                    const int d = pack_dst(sl, q, g, co, mt);
                    CHECK(d * 16 >= sl * slice_bytes(mt) && d * 16 + 16 <= (sl + 1) * slice_bytes(mt), "cout %d: element outside its slice", cout);
                    // piece q of a slice is the contiguous block [q * rows * 64, (q + 1) * rows * 64) of it (plain operands read piece 0 alone)
                    const int in_slice = d * 16 - sl * slice_bytes(mt);
                    CHECK(in_slice / (rows * 64) == q, "cout %d: piece planes are not contiguous", cout);
                    dst.at((size_t)d) += 1;
                }
                if (co < cout)
                    for (int j = 0; j < 8; ++j) src.at((size_t)pack_src(sl, g, j, co)) += 1;
            }
    for (size_t i = 0; i < dst.size(); ++i) CHECK(dst[i] == 1, "cout %d: image element %zu written %d times", cout, i, dst[i]);
    for (size_t i = 0; i < src.size(); ++i) CHECK(src[i] == 1, "cout %d: weight %zu read %d times", cout, i, src[i]);
}

// the walk of `grid` persistent workgroups over the tiles of [B, H, W]: every tile exactly once, inside the image
static void check_walk(int B, int H, int W, int cus, int xcd_map) {
    const Walk wk = walk_of(B, H, W);
    CHECK(wk.tiles_x * TC >= W && (wk.tiles_x - 1) * TC < W && wk.tiles_y * TR >= H && (wk.tiles_y - 1) * TR < H, "tile counts of %d x %d", H, W);
    const int grid = grid_of(wk.ntiles, cus), ntiles = (int)wk.ntiles;
    CHECK(grid >= 1 && grid <= cus && grid <= ntiles, "grid %d for %d tiles on %d CUs", grid, ntiles, cus);
    const bool xmap = xcd_walk(xcd_map, ntiles, grid);
    CHECK(!xmap || (ntiles % 8 == 0 && grid % 8 == 0), "XCD walk on %d tiles, %d workgroups", ntiles, grid);
    std::vector<int> seen((size_t)ntiles, 0);
    for (int w = 0; w < grid; ++w)
        for (int it = w; it < ntiles; it += grid) {
            int b = -1, row0 = -1, col0 = -1;
            tile_coords(it, xmap, ntiles, wk.tiles_x, wk.tiles_y, b, row0, col0);
            CHECK(b >= 0 && b < B && row0 >= 0 && row0 < H && col0 >= 0 && col0 < W && row0 % TR == 0 && col0 % TC == 0,
                  "tile %d of [%d,%d,%d]: sample %d, row %d, col %d", it, B, H, W, b, row0, col0);
            seen.at(((size_t)b * wk.tiles_y + row0 / TR) * wk.tiles_x + col0 / TC) += 1;
        }
    for (int i = 0; i < ntiles; ++i) CHECK(seen[(size_t)i] == 1, "[%d,%d,%d] on %d CUs, map %d: tile %d visited %d times", B, H, W, cus, xcd_map, i, seen[(size_t)i]);
}

int main() {
    for (int cout = 1; cout <= MAX_COUT; ++cout) check_pack(cout);
    const int shapes[][3] = {{1, 40, 72}, {2, 16, 32}, {2, 150, 430}, {1, 512, 512}, {3, 1, 1}, {1, 17, 33}, {5, 100, 257}, {8, 16, 32}};
    for (const auto& s : shapes)
        for (int cus : {1, 8, 200, 256, 304})
            for (int xm : {0, 1}) check_walk(s[0], s[1], s[2], cus, xm);
    CHECK(grid_of(0, 256) == 0, "empty problem");
    std::printf("%s\n", fails ? "split_out_geom: FAILED" : "split_out_geom: ok");
    return fails ? 1 : 0;
}
