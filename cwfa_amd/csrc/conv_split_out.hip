// Output convolution of a coupling sub-network on the bf16 matrix cores with fp32-equivalent arithmetic:
//
//     y = conv3x3(x, W) + b,   64 -> Cout <= 48 channels, NCHW planes of y (possibly a channel slice)      (networks.py:632, 666)
//
// The conv phase of the fused layer (conv_split_layer.hip) with MT = ceil(Cout / 16) m-tiles instead of four and a plain epilogue:
// the same tile (16 rows x 32 pixels, eight waves as eight row groups, four n-tiles per wave), the same LDS image of the haloed
// input chunk ([piece 3][k half 2][18 rows][34 px] x 16 B, two buffers), staging map, tap pairing with its 9-step period, operand
// formats (SIX / F16) and XCD-aware walk of one PERSISTENT workgroup per CU; see that file for the derivation.  What differs:
//   * a weight slice holds only the 16 MT rows in use ([piece][k group 4][16 MT cout][8], 3 MT KB); there is ONE bank per launch, so
//     the ring simply runs on round the tiles.  It has FOUR slots and step s requests slice s + 3 (for s = 15, 16, 17 the next tile's
//     slice 0, 1, 2), which has to have landed at the end of step s + 1: a step of MT <= 3 m-tiles is shorter than the latency of its own
//     request.  18 = 2 mod 4: slice s of a workgroup's k-th tile sits in slot (s & 3) ^ 2 (k & 1).
//   * the A-fragment set alternates over (step, m-tile) = (s MT + mt) & 1, so that for odd MT the first fragments of the next step
//     do not land in the set the last m-tile multiplies from (18 MT is even: a tile starts on set 0 again).
//   * after step 17 each wave stores its MT x 4 accumulator tiles (the bias rode in their initial value); channels >= Cout and
//     pixels outside the image are not written.  Step 0's request (slice 3 of the next tile) goes out BEFORE the stores, so that
//     the waits of steps 0 and 1 can leave the stores in flight (the counter retires in order); step 17 has already requested the next
//     tile's first operand fragments, there is no barrier or refill between two tiles.
#include "conv_internal.h"
#include "conv_split_out_geom.h"

extern int g_cwfa_split_xcd_map;        // conv2d.hip ("split3x3_xcd_map" option)

namespace {

using namespace cwfa_out;

constexpr int XR = TR + 2, XC = TC + 2;
constexpr int KHB = 9984;                   // bytes of one k-half plane: 18 x 34 x 16 = 9792 padded to a multiple of 256 (bank phase)
constexpr int XPB = 2 * KHB;                // bytes of one piece plane
constexpr int XB = 3 * XPB;                 // bytes of one input buffer (59 904)
constexpr int OFF_W = 2 * XB;               // the ring of four weight slices, then 16 MT biases
constexpr int NE = 2 * XR * XC;             // 1224 staging entries (k half, row, col) per chunk
constexpr int lds_bytes(int mt) { return OFF_W + 4 * slice_bytes(mt) + 64 * mt; }
static_assert(lds_bytes(MAX_MT) <= 160 * 1024, "LDS budget");

struct OParams {
    const float* x;
    float* y;
    const void* wp;
    const float* bias;                // may be NULL
    int B, H, W, Cout, tiles_x, tiles_y, ntiles;
    int64_t x_bs, y_bs;
    int xcd_map;
};

// (chunk, tap) unit u = 0..35 of the 3x3: byte offset of its B fragments relative to the lane base
__host__ __device__ constexpr int unit_off(int u) {
    const int chunk = u / 9, tap = u % 9;
    return (chunk & 1) * XB + ((tap / 3) * XC + tap % 3) * 16;
}

template <bool SIX, bool F16, bool INB, int MT>
__global__ __launch_bounds__(512, 1) void split_out_kernel(OParams p) {
    static_assert(MT >= 1 && MT <= MAX_MT, "one to three m-tiles");
    constexpr int WSL = slice_bytes(MT), OFF_BIAS = OFF_W + 4 * WSL;
    constexpr int NQ = SIX ? 3 : 1;
    constexpr int NKB = NQ * MT;                         // 1 KB blocks (one DMA instruction of a wave) of a slice that are read
    constexpr int NST = 16 * MT;                         // stores per lane and tile
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, g = lane >> 4;
    const int HW = p.H * p.W;
    const int plane = HW * 4;
    constexpr unsigned OOB = 0x80000000u;

    // ---- staging entries e = tid + k*512 < NE of the [k half][18 rows][34 px] tile
    int epk[3], edst[3];                       // column | row << 8 | k half << 16;  byte offset of the entry in an input buffer
    bool fin[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = tid + k * 512;
        fin[k] = e < NE;
        const int c_ = e % XC, r_ = (e / XC) % XR, h_ = (e / (XR * XC)) & 1;
        epk[k] = c_ | (r_ << 8) | (h_ << 16);
        edst[k] = h_ * KHB + (r_ * XC + c_) * 16;
    }
    const bool stage2 = wave < 4;              // entry 2 exists only for tid < 200: waves 0..3 (wave 3 partly)
    auto entry_offsets = [&](bool valid, int row0, int col0, unsigned (&fo)[3]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int gr = row0 + ((epk[k] >> 8) & 255) - 1, gc = col0 + (epk[k] & 255) - 1, eh = epk[k] >> 16;
            const bool ok = valid && fin[k] && gr >= 0 && gr < p.H && gc >= 0 && gc < p.W;
            // NCHW: channel 8 eh of the chunk, pixel (gr, gc); blocked: 32-byte entry (gr, gc) of channel block eh of the chunk
            fo[k] = !ok ? OOB : INB ? (unsigned)((eh * HW + gr * p.W + gc) * 32) : (unsigned)((eh * 8 * HW + gr * p.W + gc) * 4);
        }
    };
    const bool xmap = xcd_walk(p.xcd_map, p.ntiles, (int)gridDim.x);
    auto coords = [&](int it, int& b, int& row0, int& col0) { tile_coords(it, xmap, p.ntiles, p.tiles_x, p.tiles_y, b, row0, col0); };
    auto load_entry = [&](f32x4 (&xv)[2], const float* base, unsigned fo, int chunk) {
        const auto rs = CWFA_RSRC(base, 64 * plane);
        if constexpr (INB) {                          // chunk = channel blocks 2 chunk, 2 chunk + 1: 16 planes further
            xv[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, fo, chunk * 16 * plane, 0));
            xv[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, fo, chunk * 16 * plane + 16, 0));
            return;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            xv[j >> 2][j & 3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, fo, (chunk * 16 + j) * plane, 0));
    };
    auto store_entry = [&](auto kc, const f32x4 (&xv)[2], int buf) {
        constexpr int k = decltype(kc)::value;
        if (k == 2 && !stage2) return;
        bf16x8 pc[3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 a1, a2 = (__bf16)0.f, a3 = (__bf16)0.f;
            cwfa_split3<SIX, F16>(xv[j >> 2][j & 3], a1, a2, a3);
            pc[0][j] = a1; pc[1][j] = a2; pc[2][j] = a3;
        }
        if (fin[k]) {
            char* dst = lds + buf * XB + edst[k];
#pragma unroll
            for (int q = 0; q < NQ; ++q) *reinterpret_cast<bf16x8*>(dst + q * XPB) = pc[q];
        }
    };

    // ---- weight slices by LDS-DMA: wave w moves block w (the piece planes of a slice are contiguous: the NKB blocks in front
    // are the ones read; plain operands: the leading piece only), wave 0 also block 8 of the nine of <true, 3>
    const auto rw = CWFA_RSRC(p.wp, NSL * WSL);
    // slice s = 0 .. 21 of the current tile (18 .. 21: slices 0 .. 3 of the next one): byte offset of its ring slot (s & 3) ^ 2 (k & 1);
    // `tw` = 2 WSL on a workgroup's odd tiles, else 0
    int tw = 0;
    auto slot_off = [&](int s) { return (s & 3) * WSL + ((s & 2) ? -tw : tw); };
    auto dma_w = [&](int s) {
        const int so = slot_off(s), src = (s % NSL) * WSL;
        if (wave < NKB)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(lds + OFF_W + so + wave * 1024), 16, (unsigned)tid * 16u, src, 0, 0);
        if constexpr (NKB > 8) {
            if (wave == 0)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(lds + OFF_W + so + 8192), 16, 8192u + (unsigned)tid * 16u, src, 0, 0);
        }
    };

    const int alane = OFF_W + (g * 16 * MT + c16) * 16;                       // + slot_off + (q*64*MT + mt*16)*16
    const int blane = (g & 1) * KHB + ((2 * wave) * XC + c16) * 16;           // + unit_off + q*XPB + ((nt>>1)*XC + 16*(nt&1))*16
    const bool sel = (g >> 1) != 0;                                           // lane groups 2, 3 read the step's second unit
    const f32x4* bias4 = reinterpret_cast<const f32x4*>(lds + OFF_BIAS);

    f32x4 acc[MT][4];
    bf16x8 A[2][3], Bq[4][3];
    f32x4 xa[3][2], xb[3][2];                   // staged entries (8 channels of a pixel) of the next even / odd chunk
    unsigned fo_c[3], fo_n[3];                  // entry offsets in the current / next tile

    auto read_a = [&](int set, int s, int mt) {           // fragments of slice s (as for slot_off)
        const int ab = alane + slot_off(s);
#pragma unroll
        for (int q = 0; q < NQ; ++q) A[set][q] = *reinterpret_cast<const bf16x8*>(lds + ab + (q * 64 * MT + mt * 16) * 16);
    };
    auto read_b = [&](int nt, int bbase) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            Bq[nt][q] = *reinterpret_cast<const bf16x8*>(lds + bbase + q * XPB + ((nt >> 1) * XC + 16 * (nt & 1)) * 16);
    };
    auto mfma6 = [&](f32x4& c, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
        if constexpr (SIX) {
            CWFA_MFMA(a[2], b[0], c);
            CWFA_MFMA(a[1], b[1], c);
            CWFA_MFMA(a[0], b[2], c);
            CWFA_MFMA(a[1], b[0], c);
            CWFA_MFMA(a[0], b[1], c);
        }
        CWFA_MFMA_OP(F16, a[0], b[0], c);
    };
    auto bbase_of = [&](int offA, int offB) { return blane + (sel ? offB : offA); };

    // ---------------------------------------------------------------------------------------------- prologue
    if (tid < 16 * MT) reinterpret_cast<float*>(lds + OFF_BIAS)[tid] = (p.bias != nullptr && tid < p.Cout) ? p.bias[tid] : 0.f;
    int tile = blockIdx.x;
    int tb, row0, col0;
    coords(tile, tb, row0, col0);
    const float* xs_cur = p.x + (int64_t)tb * p.x_bs;
    entry_offsets(true, row0, col0, fo_c);
    cwfa_static_for<3>([&](auto kc) { load_entry(xa[decltype(kc)::value], xs_cur, fo_c[decltype(kc)::value], 0); });
    cwfa_static_for<3>([&](auto kc) { load_entry(xb[decltype(kc)::value], xs_cur, fo_c[decltype(kc)::value], 1); });
    dma_w(0);
    dma_w(1);
    dma_w(2);
    dma_w(3);
    cwfa_static_for<3>([&](auto kc) { store_entry(kc, xa[decltype(kc)::value], 0); });
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    read_a(0, 0, 0);
    {
        const int bb = bbase_of(unit_off(0), unit_off(1));
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) read_b(nt, bb);
    }

    for (; tile < p.ntiles; tile += gridDim.x) {
        const int ntile = tile + gridDim.x;
        const bool has_next = ntile < p.ntiles;
        int nb, nrow0, ncol0;
        coords(has_next ? ntile : tile, nb, nrow0, ncol0);
        const float* xs_next = p.x + (int64_t)nb * p.x_bs;
        entry_offsets(has_next, nrow0, ncol0, fo_n);

        // accumulators start from the bias (channel mt*16 + 4g + r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4 bv = bias4[mt * 4 + g];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = bv;
        }

        // ------------------------------------------------------------------------------------------ 18 conv steps
        cwfa_static_for<NSL>([&](auto sc) {
            constexpr int S = decltype(sc)::value, P = S % 9, PER = S / 9;
            constexpr bool LASTP = PER == 1;                   // the last period stages the NEXT tile's chunks 0 and 1
            constexpr auto loads_in = [](int s) { return ((s % 9 >= 2 && s % 9 <= 4) || s % 9 >= 6) ? (INB ? 2 : 8) : 0; };
            // staging loads of this step and of the one before (two 16-byte loads per entry from a channel-blocked map, eight four-byte
            // loads from NCHW planes)
            constexpr int NL = loads_in(S), NLP = loads_in((S + NSL - 1) % NSL);
            // the slice DMA, then this step's staging loads (all of which may stay in flight across the barrier), issued from inside
            // the MFMA stream (step 0's slice went out ahead of the previous tile's stores)
            auto issue_memory = [&]() {
                if constexpr (S != 0) dma_w(S + 3);
                if constexpr (P >= 2 && P <= 4) {               // even chunk 2*PER+2 (last period: chunk 0 of the next tile)
                    constexpr int k = P - 2;
                    if constexpr (!LASTP) load_entry(xa[k], xs_cur, fo_c[k], 2 * PER + 2);
                    else load_entry(xa[k], xs_next, fo_n[k], 0);
                }
                if constexpr (P >= 6) {                         // odd chunk 2*PER+3 (last period: chunk 1 of the next tile)
                    constexpr int k = P - 6;
                    if constexpr (!LASTP) load_entry(xb[k], xs_cur, fo_c[k], 2 * PER + 3);
                    else load_entry(xb[k], xs_next, fo_n[k], 1);
                }
            };
            constexpr int NS = (S + 1) % NSL;                   // next step (step 17: step 0 of the next tile)
            const int bbn = bbase_of(unit_off(2 * NS), unit_off(2 * NS + 1));
            CWFA_FENCE();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int set = (S * MT + mt) & 1;
                if (mt < MT - 1) read_a(set ^ 1, S, mt + 1);
                else read_a(set ^ 1, S + 1, 0);                 // first fragments of the next step
                CWFA_FENCE();
#pragma unroll
                for (int np = 0; np < 4; np += 2) {
                    mfma6(acc[mt][np], A[set], Bq[np]);
                    mfma6(acc[mt][np + 1], A[set], Bq[np + 1]);
                    CWFA_FENCE();
                    if (mt == MT - 1) {                         // the next step's B fragments, behind their last use
                        read_b(np, bbn);
                        read_b(np + 1, bbn);
                        CWFA_FENCE();
                    }
                }
                // after the first m-tile: this step's memory traffic and the vector-heavy part of staging (split + LDS stores of one
                // entry).  MT = 1: the first m-tile is also the last; the B requests above then have this work to land behind
                if (mt == 0) {
                    issue_memory();
                    CWFA_FENCE();
                    if constexpr (P <= 2) store_entry(cwfa_ic<P>{}, xb[P], 1);
                    if constexpr (P >= 5 && P <= 7) store_entry(cwfa_ic<P - 5>{}, xa[P - 5], 0);
                    CWFA_FENCE();
                }
            }
            // the slice DMA of the step BEFORE this one (slice S + 2: the next step reads its first fragments) has landed.  Behind it in
            // the counter: that step's staging loads, this step's DMA (waves that issue one: the wait is one operation stricter for them)
            // and loads; steps 0 and 1: also the NST stores of the tile before (step 0 issues no DMA: its slice went out ahead of them)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S == 0 ? NLP + NST : S == 1 ? NST : NLP + NL) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        });

        // ------------------------------------------------------------------------------------------ epilogue
        dma_w(NSL + 3);                         // step 0's request; its slot held slice 17: the readers are behind step 17's barrier
        {
            const auto ry = CWFA_RSRC(p.y + (int64_t)tb * p.y_bs, p.Cout * plane);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int row = row0 + 2 * wave + (nt >> 1), col = col0 + 16 * (nt & 1) + c16;
                const bool ok = col < p.W && row < p.H;
                const unsigned oo = (unsigned)(row * p.W + col) * 4u + (unsigned)g * 4u * (unsigned)plane;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {    // channel mt*16 + 4g + r: r planes further in the scalar offset
                        const float v = acc[mt][nt][r];          // (a copy: a bit cast straight from the vector element reads element 0)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry,
                                                              (ok && mt * 16 + 4 * g + r < p.Cout) ? oo : OOB, (mt * 16 + r) * plane, 0);
                    }
            }
        }
        tb = nb; row0 = nrow0; col0 = ncol0;
        xs_cur = xs_next;
        tw = 2 * WSL - tw;
#pragma unroll
        for (int k = 0; k < 3; ++k) fo_c[k] = fo_n[k];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // slice DMAs issued past the end
}

// packed image: 18 slices [piece 3][k group 4][16 MT cout][8] of bf16 (F16: piece 0 = the fp16 weights, pieces 1, 2 zero); slice =
// conv step s: group g = unit u = 2s + (g >> 1) = (chunk u / 9, tap u % 9), k half g & 1 (conv_split_out_geom.h).  Rows >= Cout: zeros.
template <bool F16>
__global__ __launch_bounds__(256) void split_out_pack_kernel(const float* __restrict__ w, uint4* __restrict__ out, int Cout, int mt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;            // over [slice 18][g 4][co 16 mt]
    const int rows = 16 * mt;
    if (i >= NSL * 4 * rows) return;
    const int co = i % rows, g = (i / rows) % 4, sl = i / (4 * rows);
    unsigned short pc[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = co < Cout ? w[pack_src(sl, g, j, co)] : 0.f;
        __bf16 a1, a2, a3;
        if constexpr (F16) {
            cwfa_split3<false, true>(v, a1, a2, a3);
            a2 = a3 = __builtin_bit_cast(__bf16, (unsigned short)0);
        } else {
            cwfa_split3<true>(v, a1, a2, a3);
        }
        pc[0][j] = __builtin_bit_cast(unsigned short, a1);
        pc[1][j] = __builtin_bit_cast(unsigned short, a2);
        pc[2][j] = __builtin_bit_cast(unsigned short, a3);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint4 u;
        u.x = pc[q][0] | ((unsigned)pc[q][1] << 16);
        u.y = pc[q][2] | ((unsigned)pc[q][3] << 16);
        u.z = pc[q][4] | ((unsigned)pc[q][5] << 16);
        u.w = pc[q][6] | ((unsigned)pc[q][7] << 16);
        out[pack_dst(sl, q, g, co, mt)] = u;
    }
}

int g_out_cus = 0;

template <bool SIX, bool F16, bool INB, int MT>
int out_launch(const OParams& p, int grid, hipStream_t st) {
    constexpr auto kern = &split_out_kernel<SIX, F16, INB, MT>;
    const int rc = cwfa_max_lds<kern>(lds_bytes(MT), "cwfa_conv3x3_out_split_f32");
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds_bytes(MT), st, p);
    CWFA_LAUNCH_CHECK("cwfa_conv3x3_out_split_f32");
    return CWFA_OK;
}

}  // namespace

extern "C" int64_t cwfa_conv3x3_out_split_packed_bytes(int Cout) {
    if (Cout < 1 || Cout > MAX_COUT) return -1;
    return packed_bytes(Cout);
}

extern "C" int cwfa_conv3x3_out_split_pack_f32(const float* w, void* packed, int Cout, void* stream) {
    CWFA_REQUIRE(w && packed, CWFA_E_INVAL, "cwfa_conv3x3_out_split_pack_f32: null pointer");
    CWFA_REQUIRE(Cout >= 1 && Cout <= MAX_COUT, CWFA_E_SHAPE, "cwfa_conv3x3_out_split_pack_f32: 1 <= Cout <= 48 (got %d)", Cout);
    CWFA_REQUIRE(cwfa_aligned16(packed), CWFA_E_ALIGN, "cwfa_conv3x3_out_split_pack_f32: packed image must be 16-byte aligned");
    const int mt = mt_of(Cout);
    const dim3 grid((unsigned)((NSL * 4 * 16 * mt + 255) / 256));
    uint4* out = reinterpret_cast<uint4*>(packed);
    cwfa_with_operand([&](auto, auto f16) -> int {
        hipLaunchKernelGGL(split_out_pack_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, w, out, Cout, mt);
        return CWFA_OK;
    });
    CWFA_LAUNCH_CHECK("cwfa_conv3x3_out_split_pack_f32");
    return CWFA_OK;
}

extern "C" int cwfa_conv3x3_out_split_f32(const float* x, const void* packed, const float* bias, float* y, int B, int H, int W, int Cout,
                                          int64_t x_bs, int64_t y_bs, int in_blocked, void* stream) {
    CWFA_REQUIRE(Cout >= 1 && Cout <= MAX_COUT, CWFA_E_SHAPE, "cwfa_conv3x3_out_split_f32: 1 <= Cout <= 48 (got %d)", Cout);
    CWFA_REQUIRE(B >= 0 && H >= 0 && W >= 0, CWFA_E_INVAL, "cwfa_conv3x3_out_split_f32: bad size");
    if (B == 0 || H == 0 || W == 0) return CWFA_OK;
    CWFA_REQUIRE(x && packed && y, CWFA_E_INVAL, "cwfa_conv3x3_out_split_f32: null pointer");
    CWFA_REQUIRE((const void*)x != (const void*)y, CWFA_E_INVAL, "cwfa_conv3x3_out_split_f32: in-place not supported (3x3 halo)");
    CWFA_REQUIRE(cwfa_aligned16(packed), CWFA_E_ALIGN, "cwfa_conv3x3_out_split_f32: packed image must be 16-byte aligned");
    CWFA_REQUIRE(!in_blocked || cwfa_aligned16(x), CWFA_E_ALIGN, "cwfa_conv3x3_out_split_f32: blocked input must be 16-byte aligned");
    CWFA_REQUIRE(!in_blocked || (x_bs & 3) == 0, CWFA_E_ALIGN, "cwfa_conv3x3_out_split_f32: blocked input batch stride must be a multiple of 4");
    CWFA_REQUIRE((int64_t)CIN * H * W * 4 < (1ll << 31), CWFA_E_SHAPE, "cwfa_conv3x3_out_split_f32: image too large for 32-bit offsets");
    const Walk wk = walk_of(B, H, W);
    CWFA_REQUIRE(wk.ntiles < (1ll << 31), CWFA_E_SHAPE, "cwfa_conv3x3_out_split_f32: too many tiles");
    OParams p{};
    p.x = x; p.y = y; p.wp = packed; p.bias = bias;
    p.B = B; p.H = H; p.W = W; p.Cout = Cout; p.x_bs = x_bs; p.y_bs = y_bs;
    p.tiles_x = wk.tiles_x; p.tiles_y = wk.tiles_y; p.ntiles = (int)wk.ntiles;
    p.xcd_map = g_cwfa_split_xcd_map;
    if (g_out_cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            cwfa_set_error("cwfa_conv3x3_out_split_f32: cannot query the CU count");
            return CWFA_E_HIP;
        }
        g_out_cus = n;
    }
    const int grid = grid_of(wk.ntiles, g_out_cus);
    const hipStream_t st = (hipStream_t)stream;
    const int mt = mt_of(Cout);
    return cwfa_with_operand([&](auto six, auto f16) -> int {
        auto go = [&](auto inb) -> int {
            if (mt == 1) return out_launch<six, f16, inb, 1>(p, grid, st);
            if (mt == 2) return out_launch<six, f16, inb, 2>(p, grid, st);
            return out_launch<six, f16, inb, 3>(p, grid, st);
        };
        return in_blocked ? go(std::true_type{}) : go(std::false_type{});
    });
}
