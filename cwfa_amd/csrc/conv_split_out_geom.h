// Host-side geometry of the persistent output convolution (conv_split_out.hip): the packed image's index arithmetic and the tile
// walk, free of device code so that a plain C++ program can check them (tests/host/split_out_geom_main.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CWFA_GEOM_HD __host__ __device__
#else
#define CWFA_GEOM_HD
#endif

namespace cwfa_out {

constexpr int TR = 16, TC = 32;             // tile: 16 rows x 32 pixels
constexpr int CIN = 64, NSL = 18;           // input channels; weight slices (conv steps) per tile
constexpr int MAX_COUT = 48, MAX_MT = 3;

CWFA_GEOM_HD constexpr int mt_of(int cout) { return (cout + 15) / 16; }                   // 16-channel m-tiles in use
CWFA_GEOM_HD constexpr int slice_bytes(int mt) { return 3 * 4 * 16 * mt * 16; }           // [piece 3][k group 4][16 mt rows][8] bf16
CWFA_GEOM_HD constexpr int64_t packed_bytes(int cout) { return (int64_t)NSL * slice_bytes(mt_of(cout)); }

// 16-byte element (slice sl, piece q, k group g, row co) of the packed image
CWFA_GEOM_HD constexpr int pack_dst(int sl, int q, int g, int co, int mt) { return (sl * 3 + q) * (64 * mt) + g * 16 * mt + co; }
// its j-th value: w[co][chunk * 16 + (g & 1) * 8 + j][tap] of the unit u = 2 sl + (g >> 1) = (chunk u / 9, tap u % 9)
CWFA_GEOM_HD constexpr int64_t pack_src(int sl, int g, int j, int co) {
    const int u = 2 * sl + (g >> 1), c = u / 9, t = u % 9;
    return ((int64_t)co * CIN + c * 16 + (g & 1) * 8 + j) * 9 + t;
}

struct Walk {
    int tiles_x, tiles_y;
    int64_t ntiles;
};
CWFA_GEOM_HD constexpr Walk walk_of(int B, int H, int W) {
    const int tx = (W + TC - 1) / TC, ty = (H + TR - 1) / TR;
    return Walk{tx, ty, (int64_t)tx * ty * B};
}
CWFA_GEOM_HD constexpr int grid_of(int64_t ntiles, int cus) { return (int)(ntiles < cus ? ntiles : cus); }
// the XCD-aware order applies when tiles and workgroups both divide over the eight XCDs
CWFA_GEOM_HD constexpr bool xcd_walk(int xcd_map, int ntiles, int grid) { return xcd_map && (ntiles & 7) == 0 && (grid & 7) == 0; }
// logical index `it` (workgroup w's k-th tile: w + k * grid) -> sample and top-left pixel of the tile
CWFA_GEOM_HD constexpr void tile_coords(int it, bool xmap, int ntiles, int tiles_x, int tiles_y, int& b, int& row0, int& col0) {
    const int tile = xmap ? (it & 7) * (ntiles >> 3) + (it >> 3) : it;
    const int per = tiles_x * tiles_y;
    b = tile / per;
    const int rem = tile - b * per;
    const int ty = rem / tiles_x;
    row0 = ty * TR;
    col0 = (rem - ty * tiles_x) * TC;
}

}  // namespace cwfa_out
