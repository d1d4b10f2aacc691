// 3x3 convolution (stride 1, zero padding 1) with fp32-equivalent arithmetic on the bf16 matrix cores -- the UNet layers of
// the LRNN (unet.py:94-113: 256 / 512 / 1024 channels) and, with the narrow tilings, the output convolutions of the coupling
// sub-networks (networks.py:633-638).
//
// Every fp32 operand is split EXACTLY into three bf16 pieces (24 significand bits) and the six partial products with
// i + j <= 4 are accumulated in fp32 by v_mfma_f32_16x16x32_bf16 (dropped terms <= 2^-24 relative); `split_products` = 1:
// plain bf16 operands (BASELINE.json configs[4]); with `split_operand` = 1 as well: plain fp16 operands on
// v_mfma_f32_16x16x32_f16 (template flag F16; same fragments, LDS images and schedule).  The input is the fp32 tensor itself: the load-side prologue of the UNet
// (BatchNorm affine x dropout mask of the producer, + skip tensor) is applied and the value split on the way into LDS.
//
// Block = 512 threads = 8 waves, two per SIMD, tile = CT = 64*MPW output channels x 8 rows x 32 pixels.  Wave (wm, wn) owns
// 16*MPW channels x 4 rows: MPW m-tiles x 8 n-tiles of 16x16 accumulators (MPW = 4: 128 registers); a B fragment (16 bytes
// per lane from LDS) feeds 6*MPW MFMAs and an A fragment 48: a k-step is ONE pass over the n-tiles with the A fragments of all MPW
// m-tiles held, so every fragment is read from LDS once per step (MPW = 4: 12 + 24 ds_read_b128 per 192 MFMAs, B fragments
// requested two n-tiles ahead of the MFMAs that consume them).  (One wave per SIMD with the whole 256-pixel tile -- 256
// accumulator registers -- was tried first: every issue cost of the single stream, LDS-DMA above all (12 instructions of
// ~60 cycles per step), is then exposed: 225 TF/s against 260 for the two-wave form's predecessor.)
//   K = 32 per MFMA = TWO (16-channel chunk, tap) units of the 9 * ceil(Cin / 16) a 3x3 has; lane group g = lane >> 4
//   reads k-half g & 1 of unit g >> 1.  The haloed input tile of a chunk, [piece 3][k half 2][9 rows][34 px] x 16 B, sits
//   in one of TWO LDS buffers (even / odd chunks); a tap only shifts the B-operand address.  A 9-step period covers an even
//   and an odd chunk: taps (0,1)(2,3)(4,5)(6,7) of the even one, its tap 8 with tap 0 of the odd one, then (1,2)...(7,8).
//   The even buffer is free from step 5 and refilled there (loads in steps 2..4), the odd one in steps 0..2 (loads in steps
//   6..8 of the period before): buffer loads, padding / border / channels >= Cin come back as 0.0 from the range check.
//   Weights: one slice [piece][k group 4][CT][8] per step through a two-slot ring by LDS-DMA, slot(s) = s & 1.
//   ONE barrier per step, and it sits in the MIDDLE of the step: mid(s), behind n-tile NT/2 - 1 (MIDSTEP; the skip-add forms
//   keep it at the step boundary, see MIDSTEP in the kernel).  The step boundary then needs no synchronisation: inside the last
//   n-tile of step s, once the MFMAs that read A[mt] have issued, A[mt] of step s+1 (m-tiles < MA) and the B fragments of its
//   n-tile 0 are requested, and the MFMA stream of a wave runs from one step into the next without a wait.  (With the barrier at
//   the boundary all eight waves left it together, asked for their A fragments at once -- 48 KB of LDS reads -- and no matrix
//   pipe of the CU had an MFMA to issue until they came back, once per step.)  Per step s:
//     first half    MFMAs of n-tiles 0 .. NT/2-1; A[MA .. MPW) from slot(s) behind the first MFMAs
//     mid(s)        s_waitcnt vmcnt(0) (this wave's pieces of slice s+1 and its staging loads), the LDS wait that leaves only the
//                   B look-ahead outstanding, s_barrier
//     second half   staging stores (steps SB + k / SA + k), staging loads (LA + k / LB + k), dma_w(s + 2, slot(s)), pre-reads
//   Why that is safe (tests/test_split3x3_schedule_cpu.py replays it with the constants read from this file):
//     weight ring, write after read: slot(s) is read at the end of step s-1 and the start of step s; every wave has finished
//       those reads (its LDS wait) when it arrives at mid(s), and dma_w(s + 2, slot(s)) is issued behind mid(s).
//     weight ring, read after write: slice s+2 is waited for by the wave that requested it (vmcnt(0)) in front of mid(s+1) and
//       first read at the end of step s+1, behind that barrier; the DMA has one full step in flight.  The prologue lands
//       slices 0 and 1 in front of its barrier.
//     input buffers, 3x3: the even buffer is last read in step 4 (tap 8); its stores sit in the second halves of steps SA + k =
//       5, 6 (, 7), behind mid(5), which a wave reaches after it has finished step 4; they are published by mid(6) .. mid(8) and
//       first read by the B pre-read at the end of step 8.  The odd buffer is last read in step 8; its stores sit behind mid(0) ..
//       mid(2) of the next period and its first read is the pre-read at the end of step 3, behind mid(3).
//       7x7: the even buffer is last read in step 24, stored behind mid(26) .. mid(28), read again at the end of step 48; the
//       odd one stored behind mid(0) .. mid(2), first read at the end of step 23.  (static_asserts in the loop.)
//     one staging register set per entry: entry k is stored at SB + k / SA + k and loaded at LA + k / LB + k, different steps
//       except SA + k = LB + k in the 3x3, where the step's stores come before its loads.
//     barriers are uniform: NT, the barrier's n-tile and p.nrun are the same for all waves of a block and the barrier sits in
//       compile-time-unrolled code: one barrier per executed step plus the prologue's (plus one in front of the statistics
//       epilogue, which overlays the input buffers that slower waves may still be reading in the last step's second half).
#include "conv_internal.h"

extern int g_cwfa_split_xcd_map;        // conv2d.hip ("split3x3_xcd_map" option)
extern int g_cwfa_split_rows16;         // conv2d.hip ("split3x3_rows16" option: 16-row tiles for the 64-channel tiling)

namespace {

constexpr int TR = 8, TC = 32;              // default tile: 8 rows x 32 pixels (four rows per wave); XG<KS, 8>: 16 rows

// input-tile geometry of a KS x KS convolution (KS = 3: the form everything above describes; KS = 7: the ConvNeXt convolution of
// the LRNN, networks.py:488 -- the same kernel with a 3-pixel halo, 49 taps and a 49-step period over two 16-channel chunks)
// RPW = image rows per wave: 4 (tile of 8 rows, 8 n-tiles per wave) or, for the 64-channel tiling of the 3x3, 8 (tile of 16 rows:
// twice the MFMAs per barrier and per A fragment, 18/16 instead of 10/8 halo rows -- the output convolutions of the sub-networks,
// whose K = 9 x 64 is too short to amortise a tile's fill and drain on 8 rows)
template <int KS, int RPW = 4>
struct XG {
    static constexpr int TRW = 2 * RPW, NT = 2 * RPW;   // tile rows; n-tiles per wave (RPW rows x 2 halves of 16 pixels)
    static constexpr int PAD = KS / 2, XR = TRW + 2 * PAD, XC = TC + 2 * PAD, NTAP = KS * KS;
    static constexpr int EPK = XR * XC;                 // entries per k half: 306 (3x3), 612 (3x3, 16 rows), 532 (7x7)
    // bytes of one k-half plane: EPK x 16 padded so that the two k halves differ by 64 bytes modulo 256 (bank phase):
    // 3x3: 4896 -> 5440;  3x3 on 16 rows: 9792 and 7x7: 8512 already are
    static constexpr int KHB = KS == 7 ? 8512 : RPW == 8 ? 9792 : 5440;
    static constexpr int XPB = 2 * KHB;                 // one piece plane
    static constexpr int XB = 3 * XPB;                  // one input buffer (3x3: 32 640 / 58 752; 7x7: 51 072)
    static constexpr bool SPECIAL = KS == 3 && RPW == 4;        // the two-entry staging map with a wave-uniform k half
    static constexpr int NEK = SPECIAL ? 2 : 3;         // staging entries per thread and chunk
    static_assert(EPK * 16 <= KHB && KHB % 256 == 64 && 2 * EPK <= 512 * NEK, "staging entry map");
    static_assert(!SPECIAL || (EPK > 256 && EPK <= 384), "3x3 staging entry map");
    static_assert(KS == 3 || RPW == 4, "7x7: 8-row tiles");
};

template <int MPW, int KS = 3, int RPW = 4, int WM = 4>
struct Geo {
    static constexpr int CT = 16 * MPW * WM;            // output channels per block (WM channel groups of 16 MPW)
    static constexpr int WSL = 3 * 4 * CT * 16;         // bytes of one weight slice (K = 32)
    static constexpr int LDS = 2 * XG<KS, RPW>::XB + 2 * WSL;   // 3x3, MPW = 4: 163 584 ... see the static_assert
    static_assert(LDS <= 160 * 1024, "LDS budget");
};

struct SParams {
    const float* x;
    const void* wp;
    float* y;
    int B, Cin, H, W, Cout, nchunks, nsteps, tiles_x, ntiles, ctiles, xcd_map;
    int nrun;                 // steps that are executed: nsteps, minus the trailing steps of an all-zero odd chunk (3x3 with an odd chunk count)
    int64_t x_bs, y_bs;
    cwfa_conv_opts o;
    cwfa_couple cp;             // EPI_COUPLE only
};

// byte offset of the B fragments of tap t in buffer `buf`, relative to the lane base
template <int KS, int RPW>
__host__ __device__ constexpr int tap_off(int buf, int tap) { return buf * XG<KS, RPW>::XB + ((tap / KS) * XG<KS, RPW>::XC + tap % KS) * 16; }

enum { EPI_RUNTIME = -1, EPI_COUPLE = -2 };

// ADD: a second tensor is added on load (UNet skip); ACT1: compile-time activation of the common epilogues (bias -> ACT1),
// EPI_RUNTIME = whatever cwfa_conv_opts says (bias -> act -> + residual -> act2)
// WM = channel groups per block (4: the form described above; 2 / 1: the narrow tilings for banks with <= 32 / <= 16 outputs -- the
// condition nets' 2-D convolutions and the output convolutions of the coarse steps' sub-networks, networks.py:212-219,633-638 --
// on the 16-row tile: the eight waves are WM channel groups x 8 / WM row groups of 16 WM / 8 rows each)
// F16: fp16 operands (single product only)
template <int MPW, bool SIX, bool ADD, int ACT1, int KS = 3, int RPW = 4, int WM = 4, bool F16 = false>
__global__ __launch_bounds__(512, 1) void conv3x3_split_kernel(SParams p) {
    typedef XG<KS, RPW> G;
    constexpr int XC = G::XC, EPK = G::EPK, KHB = G::KHB, XPB = G::XPB, XB = G::XB, NTAP = G::NTAP, PAD = G::PAD;
    constexpr int WN = 8 / WM, RW = G::TRW / WN, NT = 2 * RW;      // row groups, image rows and n-tiles per wave
    constexpr bool SPECIAL = G::SPECIAL;
    static_assert(SPECIAL || ((MPW == 1 || WM != 4) && !ADD), "7x7 / 16-row tiles: the 64-channel and narrow tilings, without a skip add");
    static_assert(WM == 4 || (((KS == 3 && RPW == 8) || KS == 7) && MPW <= 3 && !ADD && ACT1 != EPI_COUPLE),
                  "narrow tilings: 16-row tile (7x7: 8-row), <= 3 m-tiles per wave");
    static_assert(MPW != 3 || WM != 4, "three m-tiles per wave: the 48- / 96-channel tilings only");
    constexpr int CT = 16 * MPW * WM;                   // output channels per block
    constexpr int WSL = 3 * 4 * CT * 16;                // bytes of one weight slice (K = 32)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // scalar: everything derived from it stays in SGPRs
    const int wm = wave % WM, wn = wave / WM;                           // channel group / row group of this wave
    const int HW = p.H * p.W;
    const int plane = HW * 4;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int NQ = SIX ? 3 : 1;
    constexpr int OFF_W = 2 * XB;
    // XCD-aware block -> (spatial tile, cout tile) map.  Workgroups are dealt round-robin over the 8 XCDs (blocks L and L + 8 share
    // an L2): XCD x works through its own contiguous band of spatial tiles (row-major: halo rows are re-read from that L2) with the
    // cout tiles of one spatial tile in consecutive slots, so the second .. fourth read of an input tile hits L2, not the fabric.
    const int b = blockIdx.z;
    int sp, ct;
    if (p.xcd_map && (p.ntiles & 7) == 0) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        sp = xcd * (p.ntiles >> 3) + slot / p.ctiles;
        ct = slot % p.ctiles;
    } else {
        sp = blockIdx.x / p.ctiles;
        ct = blockIdx.x % p.ctiles;
    }
    const int row0 = (sp / p.tiles_x) * G::TRW, col0 = (sp % p.tiles_x) * TC;

    // ---- staging entries (two per thread): k = 0: k half wave >> 2, entries 0..255; k = 1: entries 256..339 of k half
    // (wave >> 1) & 1 for waves 0..3 (so that the k half, hence the channel, is uniform over a wave)
    // (7x7: three per thread, entry e = tid + 512 k of the 2 x 532; the k half is NOT uniform over a wave there, so it rides in the
    // per-lane offset and the form has no load-side affine)
    constexpr int NEK = G::NEK;
    int ekh[NEK], eidx[NEK];
    bool fin[NEK];
    unsigned fo[NEK];
    if constexpr (SPECIAL) {
        ekh[0] = wave >> 2; eidx[0] = tid & 255; fin[0] = true;
        ekh[1] = (wave >> 1) & 1; eidx[1] = 256 + (tid & 127); fin[1] = wave < 4 && eidx[1] < EPK;
    } else {
#pragma unroll
        for (int k = 0; k < NEK; ++k) {
            const int e = tid + 512 * k;
            ekh[k] = e >= EPK;
            eidx[k] = e - ekh[k] * EPK;
            fin[k] = e < 2 * EPK;
        }
    }
    bool fok[NEK];
#pragma unroll
    for (int k = 0; k < NEK; ++k) {
        const int r = eidx[k] / XC, c = eidx[k] % XC;
        const int gr = row0 + r - PAD, gc = col0 + c - PAD;
        fok[k] = fin[k] && gr >= 0 && gr < p.H && gc >= 0 && gc < p.W;
        // blocked input ([Cin/8][H][W][8], cwfa_conv_opts.in_blocked8): the 32-byte entry of the pixel; its channel block rides
        // in the scalar offset
        fo[k] = !fok[k] ? OOB : p.o.in_blocked8 ? (unsigned)((gr * p.W + gc) * 32) : (unsigned)((gr * p.W + gc) * 4);
        if constexpr (!SPECIAL) fo[k] = !fok[k] ? OOB : fo[k] + (unsigned)(ekh[k] * 8) * (unsigned)plane;    // (either layout: 8 planes)
    }
    const int xbytes = p.Cin * plane;                   // channels >= Cin: out of range, 0.0
    const auto rx = CWFA_RSRC(p.x + (int64_t)b * p.x_bs, xbytes);
    const auto ra = CWFA_RSRC(ADD ? p.o.in_add + (int64_t)b * p.o.in_add_bs : p.x, ADD ? xbytes : 0);
    const bool has_aff = p.o.in_scale != nullptr;
    // the load-side affine tables are read through the SCALAR cache (constant address space; they were written by an
    // earlier kernel and the channel index is uniform over a wave): as vector loads each cost a full memory round trip
    // in the middle of the step
    typedef const float __attribute__((address_space(4))) cfloat;
    cfloat* sc = has_aff ? (cfloat*)(p.o.in_scale + (int64_t)b * p.o.in_affine_bs) : nullptr;
    cfloat* sh = has_aff ? (cfloat*)(p.o.in_shift + (int64_t)b * p.o.in_affine_bs) : nullptr;

    auto load_entry = [&](auto kc, float (&xv)[8], float (&av)[8], int chunk) {
        constexpr int k = decltype(kc)::value;
        const int ch0 = chunk * 16 + (SPECIAL ? ekh[k] * 8 : 0);        // (otherwise the k half is in the lane's offset)
        if (KS == 3 && !ADD && p.o.in_blocked8) {                  // (uniform) channel block ch0 / 8 = 8 planes' worth of bytes each (the
                                                        // load-side affine is per channel: unchanged)
            const f32x4 lo4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, fo[k], ch0 * plane, 0));
            const f32x4 hi4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, fo[k], ch0 * plane + 16, 0));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                xv[j] = lo4[j];
                xv[4 + j] = hi4[j];
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, fo[k], (ch0 + j) * plane, 0));
        if constexpr (ADD) {
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, fo[k], (ch0 + j) * plane, 0));
        }
    };
    auto store_entry = [&](auto kc, const float (&xv)[8], const float (&av)[8], int chunk, int buf) {
        constexpr int k = decltype(kc)::value;
        if (SPECIAL && k == 1 && !fin[1]) return;
        const int ch0 = chunk * 16 + ekh[k] * 8;          // wave-uniform (two-entry map): the affine tables are read through scalar loads
        bf16x8 pc[3];
        float scv[8], shv[8];
        if (has_aff) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ch = ch0 + j < p.Cin ? ch0 + j : p.Cin - 1;
                scv[j] = ch0 + j < p.Cin ? sc[ch] : 0.f;
                shv[j] = ch0 + j < p.Cin ? sh[ch] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = xv[j];
            if (has_aff) v = fok[k] ? v * scv[j] + shv[j] : 0.f;       // padding stays zero
            if constexpr (ADD) v += av[j];
            __bf16 a1, a2 = (__bf16)0.f, a3 = (__bf16)0.f;
            cwfa_split3<SIX, F16>(v, a1, a2, a3);
            pc[0][j] = a1; pc[1][j] = a2; pc[2][j] = a3;
        }
        char* dst = lds + buf * XB + ekh[k] * KHB + eidx[k] * 16;
        if (SPECIAL || fin[k]) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) *reinterpret_cast<bf16x8*>(dst + q * XPB) = pc[q];
        }
    };

    // ---- weight slices by LDS-DMA: WSL / 1024 wave instructions per slice, a quarter per wave
    // 1 KB pieces per slice (12 / 24 / 48), dealt round-robin over the 8 waves; plain-bf16 mode reads only the leading piece plane of a
    // slice ([piece][k group][CT][8]: its first third), so only that is fetched
    constexpr int NPC = (SIX ? WSL : WSL / 3) / 1024;
    const int64_t wtile = (int64_t)ct * p.nsteps * WSL;
    const char* wbase = reinterpret_cast<const char*>(p.wp) + wtile;
    const auto rw = CWFA_RSRC(wbase, p.nsteps * WSL);
    auto dma_w = [&](int slice, int slot) {              // slices past the end: out of range, zeros, never read
        cwfa_static_for<(NPC + 7) / 8>([&](auto ic_) {
            constexpr int i = decltype(ic_)::value;
            const int piece = i * 8 + wave;
            if (piece < NPC) {                           // wave-uniform
                char* dst = lds + OFF_W + slot * WSL + piece * 1024;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)dst, 16, (unsigned)(lane * 16), slice * WSL + piece * 1024, 0, 0);
            }
        });
    };

    const int alane = OFF_W + (g * CT + wm * MPW * 16 + c16) * 16;        // + slot*WSL + (q*4*CT + mt*16)*16
    const int blane = (g & 1) * KHB + (wn * RW * XC + c16) * 16;             // + tap_off + q*XPB + ((nt>>1)*XC + 16*(nt&1))*16
    const bool sel = (g >> 1) != 0;

    f32x4 acc[MPW][NT];
#pragma unroll
    for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // ONE pass over the n-tiles per step: the A fragments of all MPW m-tiles are held (MPW = 4: 48 registers), so every B fragment is
    // read once per step and feeds 6 MPW MFMAs.  NB sets of B fragments = NB - 1 n-tiles of look-ahead (256-channel tiling: two);
    // the A fragments of m-tiles >= MA are requested behind the step's first MFMAs, not in front of them.
    constexpr int NB = MPW == 4 ? 3 : 2, MA = MPW == 4 ? 2 : MPW;
    static_assert(NB - 1 < NT, "B look-ahead");
    // where the step's one barrier sits: in the MIDDLE of the step (see the header) -- or, for the skip-add forms, at the step
    // boundary: their staging set is twice as large (input + skip tensor), and with the split in the middle of the step, where
    // all A fragments and the B look-ahead are live, the allocator spilled 24 of its registers to scratch inside the loop
    constexpr bool MIDSTEP = !ADD;
    bf16x8 A[MPW][3], Bq[NB][3];
    // staged entries of the chunk after next (+ skip tensor): ONE register set per entry serves the even and the odd chunk in turn
    // (its even-chunk value is stored at SA + k, before the odd-chunk load at LB + k, and that one at SB + k of the next period,
    // before the even-chunk load at LA + k: see the staging schedule in the loop)
    float xs[NEK][8], sk[NEK][8];

    auto read_a = [&](int abase, int m0, int m1) {
#pragma unroll
        for (int mt = m0; mt < m1; ++mt)
#pragma unroll
            for (int q = 0; q < NQ; ++q) A[mt][q] = *reinterpret_cast<const bf16x8*>(lds + abase + (q * 4 * CT + mt * 16) * 16);
    };
    auto read_b = [&](int set, int bbase, int nt) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            Bq[set][q] = *reinterpret_cast<const bf16x8*>(lds + bbase + q * XPB + ((nt >> 1) * XC + 16 * (nt & 1)) * 16);
    };
    auto mfma6 = [&](f32x4& c, const bf16x8 (&a)[3], const bf16x8 (&bb)[3]) {
        if constexpr (SIX) {
            CWFA_MFMA(a[2], bb[0], c);
            CWFA_MFMA(a[1], bb[1], c);
            CWFA_MFMA(a[0], bb[2], c);
            CWFA_MFMA(a[1], bb[0], c);
            CWFA_MFMA(a[0], bb[1], c);
        }
        CWFA_MFMA_OP(F16, a[0], bb[0], c);
    };

    // ---------------------------------------------------------------------------------------------- prologue
    {
        float x0[NEK][8], s0[NEK][8];                     // chunk 0: stored right here; chunk 1 goes straight into the set (stored at SB + k)
        cwfa_static_for<NEK>([&](auto kc) { load_entry(kc, x0[decltype(kc)::value], s0[decltype(kc)::value], 0); });
        cwfa_static_for<NEK>([&](auto kc) { load_entry(kc, xs[decltype(kc)::value], sk[decltype(kc)::value], 1); });
        dma_w(0, 0);
        if constexpr (MIDSTEP) dma_w(1, 1);               // (published with slice 0 right here; mid(0) then frees slot 0 for slice 2)
        cwfa_static_for<NEK>([&](auto kc) { store_entry(kc, x0[decltype(kc)::value], s0[decltype(kc)::value], 0, 0); });
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    if constexpr (MIDSTEP) read_a(alane, 0, MA);                                    // step 0: slice 0 in slot 0
    read_b(0, blane + (sel ? tap_off<KS, RPW>(0, 1) : tap_off<KS, RPW>(0, 0)), 0);  // step 0: taps 0 | 1 of chunk 0
    // ONE step as the body of a rolled loop (the accumulators are loop-carried values: unrolling the nine steps of a period
    // makes the register allocator split their live ranges and keep copies); P = position in the 9-step period
    int sl = 0, P = 0, ce = 0;                           // ring slot of this step's slice; period position; even chunk of the period
    for (int step = 0; step < p.nrun; ++step) {
        const int co = ce + 1;                            // odd chunk (past the end: all zeros, costs only time)
        // units of this step: even chunk taps (2P, 2P+1) for P < 4; (tap 8 | odd tap 0) at P = 4; odd taps (2P-9, 2P-8) after
        // (7x7: 49 taps, the same pairing with a 49-step period)
        const int uA = 2 * P, uB = 2 * P + 1;
        const int bufA = uA >= NTAP, tA = uA - NTAP * bufA, bufB = uB >= NTAP, tB = uB - NTAP * bufB;
        const int offA = bufA * XB + ((tA / KS) * XC + tA % KS) * 16, offB = bufB * XB + ((tB / KS) * XC + tB % KS) * 16;
        // staging schedule inside a period (MIDSTEP: everything in the SECOND half of its step, behind the step's barrier; otherwise
        // stores at the start of the step and loads behind its first n-tile): the odd buffer is
        // free from step 0 (stores SB + k of the entries loaded in the period before), the even one from the step after the one
        // that pairs tap NTAP-1 with the odd chunk's tap 0 (stores SA + k, loads LA + k a few steps earlier); the odd chunk after
        // next is loaded at LB + k
        constexpr int SB = 0, SA = KS == 3 ? 5 : 26, LA = KS == 3 ? 2 : 22, LB = KS == 3 ? 6 : 44;       // (+ k < NEK: all below NTAP)
        constexpr int MID = NT / 2;                       // the step's barrier sits behind n-tile MID - 1
        constexpr int FO = (NTAP - 1) / 2;                // the step that reads the even buffer last and the odd one first
        static_assert(LB + NEK - 1 < NTAP && LA + NEK - 1 < SA, "staging schedule");
        static_assert(SB < LA && SA <= LB, "staging schedule: one register set per entry (a step's stores come before its loads)");
        // a store behind mid(t) is published by mid(t + 1); a buffer's first B fragments are requested at the END of the step before
        static_assert(!MIDSTEP || SB + NEK - 1 <= FO - 2, "staging schedule: the odd buffer is complete one barrier before the end of step FO - 1");
        static_assert(!MIDSTEP || (SA >= FO + 1 && SA + NEK - 1 <= NTAP - 2), "staging schedule: the even buffer is written behind mid(FO + 1) ... mid(NTAP - 2)");
        static_assert(MID >= 1 && MID + NB - 2 < NT, "mid-step barrier: the B look-ahead it leaves outstanding lies inside the step");
        // the n-tiles behind which the staging loads and the weight DMA are issued
        constexpr int LOAD_NT = MIDSTEP ? MID : 0, DMA_NT = !MIDSTEP ? 1 : NT >= 8 ? MID + 1 : MID;
        // the staging split + LDS stores of one entry of the chunk after next, into the buffer this step does not read.
        // -- order matters: in this rolled loop the compiler cannot count the vector-memory operations between a staging load
        // and its use, so it waits for ALL of them (vmcnt(0)) before the split: that must come right behind the wait in front of
        // the step's barrier, when nothing is outstanding, and BEFORE the step issues its own loads and DMA (after them it cost
        // 2 - 9 thousand cycles per step)
        // (written out per entry: behind a generic lambda the staged-entry arrays stopped being promoted to registers)
        auto staging_stores = [&]() {
            const bool odd0 = P == SB, odd1 = P == SB + 1;          // the entry in the set: of the odd chunk (-> buffer 1) or the even one
            if (odd0 || P == SA) store_entry(cwfa_ic<0>{}, xs[0], sk[0], odd0 ? co : ce + 2, odd0);
            if (odd1 || P == SA + 1) store_entry(cwfa_ic<1>{}, xs[1], sk[1], odd1 ? co : ce + 2, odd1);
            if constexpr (NEK > 2) {
                const bool odd2 = P == SB + 2;
                if (odd2 || P == SA + 2) store_entry(cwfa_ic<NEK - 1>{}, xs[NEK - 1], sk[NEK - 1], odd2 ? co : ce + 2, odd2);
            }
            CWFA_FENCE();
        };
        // MIDSTEP: this step's A fragments of m-tiles < MA and the B fragments of n-tile 0 were requested inside the last n-tile of the step
        // before (the prologue for step 0): the first MFMA issues at once, there is no wait and no barrier at the step boundary
        const int abase = alane + sl * WSL, anext = alane + (sl ^ 1) * WSL;
        const int bbase = blane + (sel ? offB : offA);
        // first B fragments of the next step (the input tiles it reads were completed at least one barrier ago)
        auto read_b_next = [&]() {
            const int nP = P == NTAP - 1 ? 0 : P + 1;
            const int nA = 2 * nP, nB = 2 * nP + 1;
            const int nbufA = nA >= NTAP, ntA = nA - NTAP * nbufA, nbufB = nB >= NTAP, ntB = nB - NTAP * nbufB;
            const int noffA = nbufA * XB + ((ntA / KS) * XC + ntA % KS) * 16, noffB = nbufB * XB + ((ntB / KS) * XC + ntB % KS) * 16;
            read_b(0, blane + (sel ? noffB : noffA), 0);
            CWFA_FENCE();
        };
        static_assert((NT - 1) % NB != 0 && NT >= 2, "the last n-tile is not multiplied from B set 0 (the next step's first fragments land there)");
        if constexpr (!MIDSTEP) {
            // boundary barrier: the stores, then the first A fragments (the step's first B fragments were requested before the
            // barrier of the step before).  Nothing else is requested in front of the first MFMA: behind the conditional staging
            // stores the compiler drains the LDS counter there (lgkmcnt(0)), so every read issued up here would be waited for
            staging_stores();
            read_a(abase, 0, MA);
            CWFA_FENCE();
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            // NB - 1 n-tiles ahead, into the set the n-tile before this one has just been multiplied from (256-channel tiling, n-tile 0:
            // behind its first MFMAs, see there); the compiler's waits are counted: only the fragment about to be used
            if ((MA == MPW || nt > 0) && nt + NB - 1 < NT) read_b((nt + NB - 1) % NB, bbase, nt + NB - 1);
            // MIDSTEP: the look-ahead runs on into the next step -- its n-tile 0 is requested in front of this step's last n-tile
            // (set 0 is free since n-tile NT - 2 at the latest), so the step boundary exposes no LDS round trip
            if (MIDSTEP && nt == NT - 1) read_b_next();
            CWFA_FENCE();
#pragma unroll
            for (int mt = 0; mt < MPW; ++mt) {
                mfma6(acc[mt][nt], A[mt], Bq[nt % NB]);
                CWFA_FENCE();                 // keep the six products of a tile back to back (accumulator forwarding)
                if (MA < MPW && nt == 0 && mt == 0) {
                    // behind the step's first MFMAs, in the order of their use: the remaining A fragments (the MFMAs of m-tile 1
                    // cover them; this step's slot, published by the barrier of the step before), then the B fragments of the look-ahead
                    read_a(abase, MA, MPW);
#pragma unroll
                    for (int n2 = 1; n2 < NB && n2 < NT; ++n2) read_b(n2, bbase, n2);
                    CWFA_FENCE();
                }
                if (MIDSTEP && nt == NT - 1 && mt < MA) {
                    // last n-tile: A[mt] has fed its last MFMAs of this step -> the NEXT step's fragment, from the other slot (its
                    // slice was waited for in front of this step's barrier); the MFMAs of the m-tiles behind cover the round trip
                    read_a(anext, mt, mt + 1);
                    CWFA_FENCE();
                }
            }
            if (MIDSTEP && nt == MID - 1) {
                // ---- the step's ONE barrier.  In front of it: this wave's pieces of the next slice (requested behind the barrier of
                // the step before: one full step in flight) and its staging loads have landed; every LDS access of this wave but the
                // NB - 1 sets of B fragments of the look-ahead is done -- its reads of this step's slot, its staging stores
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"((NB - 1) * NQ) : "memory");
                __builtin_amdgcn_s_barrier();
                staging_stores();
            }
            // this step's staging loads and the weight slice after next (boundary barrier: the next one) are issued from INSIDE the
            // MFMA stream, MIDSTEP: of the second half
            // (in a burst right behind the barrier, all eight waves stood in their issue cost -- ~100 cycles per DMA instruction --
            // at once with the matrix pipe idle; here the SIMD partner's MFMAs run meanwhile).  Loads BEFORE the DMA: they
            // overwrite loop-carried registers, so the compiler waits for every older vector-memory operation first -- which must
            // not include a DMA issued a moment ago.
            if (nt == LOAD_NT) {
                if (P == LA || P == LB) load_entry(cwfa_ic<0>{}, xs[0], sk[0], P == LA ? ce + 2 : co + 2);
                if (P == LA + 1 || P == LB + 1) load_entry(cwfa_ic<1>{}, xs[1], sk[1], P == LA + 1 ? ce + 2 : co + 2);
                if constexpr (NEK > 2) {
                    if (P == LA + 2 || P == LB + 2) load_entry(cwfa_ic<NEK - 1>{}, xs[NEK - 1], sk[NEK - 1], P == LA + 2 ? ce + 2 : co + 2);
                }
                CWFA_FENCE();
            }
            if (nt == DMA_NT) {
                if constexpr (MIDSTEP) dma_w(step + 2, sl);     // into THIS step's slot: every wave finished reading it in front of the barrier
                else dma_w(step + 1, sl ^ 1);
                CWFA_FENCE();
            }
        }
        if constexpr (!MIDSTEP) read_b_next();       // (boundary barrier: requested in front of it)
        if constexpr (!MIDSTEP) {
            // boundary barrier: the next slice (the youngest vector-memory operation of the step) has landed; LDS: everything but the
            // B-fragment reads just issued is done, the staging stores of this step included
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(NQ) : "memory");
            __builtin_amdgcn_s_barrier();
        }
        sl ^= 1;
        if (++P == NTAP) {
            P = 0;
            ce += 2;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // DMAs / loads past the end

    // ---------------------------------------------------------------------------------------------- epilogue
    // accumulator register r of tile (mt, nt): channel ct*CT + (wm*MPW + mt)*16 + 4g + r, pixel (row0 + 4*wn + nt/2, col0 + 16*(nt&1) + c16).
    // Buffer stores: the descriptor ends at channel Cout and a pixel outside the image carries an out-of-range offset.
    const auto ry = CWFA_RSRC(p.y + (int64_t)b * p.y_bs, p.Cout * plane);
    const auto rr = CWFA_RSRC(p.o.residual ? p.o.residual + (int64_t)b * p.o.res_bs : p.y, p.o.residual ? p.Cout * plane : 0);
    const auto rb = CWFA_RSRC(p.o.bias ? p.o.bias : p.y, p.o.bias ? p.Cout * 4 : 0);
    const bool alpha_pc = p.o.prelu_per_channel != 0;          // (uniform) one PReLU slope per output channel
    const float alpha = (p.o.prelu_alpha && !alpha_pc) ? *p.o.prelu_alpha : 0.f;
    const auto rpa = CWFA_RSRC(alpha_pc ? p.o.prelu_alpha : p.y, alpha_pc ? p.Cout * 4 : 0);
    const int cwave = ct * CT + wm * MPW * 16;      // uniform: rides in the scalar offset
    const unsigned glane = (unsigned)(4 * g) * (unsigned)plane;                           // the lane group's channel offset
    if constexpr (ACT1 == EPI_COUPLE) {
        // The bank's rows were interleaved at pack time (cwfa_couple_rows) so that this lane holds s_j AND t_j of its pixels:
        //   MPW = 1: pair j = 8 wm + 2 g + h  ->  s in register h, t in register h + 2 of the one m-tile
        //   MPW = 2: pair j = 16 wm + 4 g + r ->  s in m-tile 0, t in m-tile 1, register r
        // x / y descriptors end at channel n: pairs >= n read 0.0 and their stores are dropped (their s is 0: zero rows).
        static_assert(MPW <= 2 && !ADD, "coupling epilogue: narrow tilings only");
        constexpr int NP = MPW == 1 ? 2 : 4;                                       // pairs per lane and n-tile
        const cwfa_couple& cp = p.cp;
        const auto cx = CWFA_RSRC(cp.x + (int64_t)b * cp.x_bs, cp.n * plane);
        const auto cy = CWFA_RSRC(cp.y + (int64_t)b * cp.y_bs, cp.n * plane);
        const unsigned jlane = (unsigned)((MPW == 1 ? 2 : 4) * g) * (unsigned)plane;
        const int jwave = wm * (MPW == 1 ? 8 : 16);
        float bs[NP], bt[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int rs = k, rt = MPW == 1 ? k + 2 : 16 + k;                        // packed rows of s_j / t_j relative to cwave + 4g
            bs[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, (unsigned)(16 * g), (cwave + rs) * 4, 0));
            bt[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, (unsigned)(16 * g), (cwave + rt) * 4, 0));
        }
        float ssum = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int row = row0 + wn * RW + (nt >> 1), col = col0 + 16 * (nt & 1) + c16;
            const bool ok = row < p.H && col < p.W;
            const unsigned po = ok ? (unsigned)((row * p.W + col) * 4) + jlane : OOB;
            float xv[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) xv[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(cx, po, (jwave + k) * plane, 0));
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const float sr = acc[0][nt][k] + bs[k];
                float tr;
                if constexpr (MPW == 1) tr = acc[0][nt][k + 2] + bt[k];
                else tr = acc[MPW - 1][nt][k] + bt[k];
                const float sv = cwfa_soft_clamp(sr * cp.pre_scale, cp.clamp_kind, cp.clamp);
                const float tv = tr * cp.pre_scale;
                const float yv = cp.rev ? (xv[k] - tv) * __expf(-sv) : __expf(sv) * xv[k] + tv;     // |s| <= clamp: v_exp_f32, rel. error ~2e-7
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, yv), cy, po, (jwave + k) * plane, 0);
                ssum += ok ? sv : 0.f;
            }
            CWFA_FENCE();
        }
        if (cp.logdet) {                                  // block sum -> one float64 atomic per block
            const double ws = cwfa_wave_sum((double)ssum);
            double* red = reinterpret_cast<double*>(lds);  // the operand buffers are dead once every wave has passed this barrier
            __builtin_amdgcn_s_barrier();
            if (lane == 0) red[wave] = ws;
            __syncthreads();
            if (tid == 0) {
                double tot = 0.0;
#pragma unroll
                for (int w = 0; w < 8; ++w) tot += red[w];
                atomicAdd(&cp.logdet[b], cp.rev ? -tot : tot);
            }
        }
        return;
    }
    const bool outb = p.o.out_blocked8 != 0;           // (uniform) y channel-blocked [Cout/8][H][W][8]: the lane's four channels = 16 bytes
    // cwfa_conv_opts.out_stats: per-channel (sum, sum of squares) of the output for the BatchNorm that follows (unet.py:99-107):
    // lane sums over its n-tiles, 16-lane DPP sums (pixels of a row), the block's two row halves through LDS (the operand
    // buffers are dead), then one float64 atomic pair per channel and block
    const bool want_stats = ACT1 != EPI_RUNTIME && p.o.out_stats != nullptr;
    float* red = reinterpret_cast<float*>(lds);        // [wn WN][CT][2]
#pragma unroll
    for (int mt = 0; mt < MPW; ++mt) {
        float bias[4];
        float st1[4] = {0.f, 0.f, 0.f, 0.f}, st2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r)
            bias[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, (unsigned)(16 * g), (cwave + mt * 16 + r) * 4, 0));
        float al[4] = {alpha, alpha, alpha, alpha};
        if (alpha_pc) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                al[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rpa, (unsigned)(16 * g), (cwave + mt * 16 + r) * 4, 0));
        }
        // run-time epilogue: the residual of n-tile nt + RLA is requested while n-tile nt is finished (one tile at a time -- as the
        // FENCE below orders it -- every n-tile stood in the full latency of its four loads: 160 -> 1xx us for 64 -> 64 at 512 x 512)
        constexpr int RLA = NT < 4 ? NT : 4;
        float rv[ACT1 == EPI_RUNTIME ? NT : 1][4];
        auto load_res = [&](int nt) {
            const int row = row0 + wn * RW + (nt >> 1), col = col0 + 16 * (nt & 1) + c16;
            const unsigned po = (row < p.H && col < p.W) ? (unsigned)((row * p.W + col) * 4) + glane : OOB;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                rv[ACT1 == EPI_RUNTIME ? nt : 0][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, po, (cwave + mt * 16 + r) * plane, 0));
        };
        if constexpr (ACT1 == EPI_RUNTIME) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) rv[nt][r] = 0.f;
            if (p.o.residual) {
#pragma unroll
                for (int nt = 0; nt < RLA; ++nt) load_res(nt);
            }
            CWFA_FENCE();
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int row = row0 + wn * RW + (nt >> 1), col = col0 + 16 * (nt & 1) + c16;
            if constexpr (ACT1 == EPI_RUNTIME) {
                if (nt + RLA < NT && p.o.residual) load_res(nt + RLA);
                CWFA_FENCE();
            }
            if constexpr (ACT1 != EPI_RUNTIME) {
                if (outb) {
                    f32x4 o4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o4[r] = cwfa_act_ct<ACT1>(acc[mt][nt][r] + bias[r], al[r]);
                    const unsigned pb = (row < p.H && col < p.W) ? (unsigned)(((g >> 1) * HW + row * p.W + col) * 32 + (g & 1) * 16) : OOB;
                    cwfa_buffer_store_b128(__builtin_bit_cast(u32x4, o4), ry, pb, (cwave + mt * 16) * plane);   // (+ wait states: common.h)
                    continue;
                }
            }
            const unsigned po = (row < p.H && col < p.W) ? (unsigned)((row * p.W + col) * 4) + glane : OOB;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int soff = (cwave + mt * 16 + r) * plane;
                float v = acc[mt][nt][r] + bias[r];
                if constexpr (ACT1 == EPI_RUNTIME) {
                    v = cwfa_act(v, p.o.act, al[r]);
                    v += rv[nt][r];
                    v = cwfa_act(v, p.o.act2, al[r]);
                } else {
                    v = cwfa_act_ct<ACT1>(v, al[r]);
                    if (want_stats) {
                        const float vm = po != OOB ? v : 0.f;
                        st1[r] += vm;
                        st2[r] += vm * vm;
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, po, soff, 0);
            }
            CWFA_FENCE();                 // keep the results from being staged in registers all at once
        }
        if constexpr (ACT1 != EPI_RUNTIME) {
            if (want_stats) {
                // MIDSTEP: the loop's last barrier sits in the MIDDLE of the last step, so the other waves may still be reading B
                // fragments of its second half out of the buffer `red` overlays: one more barrier in front of the first write to it
                // (uniform: want_stats is a kernel argument, mt a compile-time index)
                if (MIDSTEP && mt == 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float a1 = cwfa_row16_sum(st1[r]), a2 = cwfa_row16_sum(st2[r]);
                    if (c16 == 0) {
                        const int ch = (wm * MPW + mt) * 16 + 4 * g + r;
                        red[(wn * CT + ch) * 2] = a1;
                        red[(wn * CT + ch) * 2 + 1] = a2;
                    }
                }
            }
        }
    }
    if constexpr (ACT1 != EPI_RUNTIME) {
        if (want_stats) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            const int ch = ct * CT + tid;
            if (tid < CT && ch < p.Cout) {
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int k = 0; k < WN; ++k) {
                    s1 += (double)red[(k * CT + tid) * 2];
                    s2 += (double)red[(k * CT + tid) * 2 + 1];
                }
                atomicAdd(&p.o.out_stats[2 * ch], s1);
                atomicAdd(&p.o.out_stats[2 * ch + 1], s2);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 7x7 over <= 8 input channels
// The few-channel form of the 7x7 (the ConvNeXt 1x1 + 7x7 of the LRNN's mean-volume branch composed into ONE 7x7 over the block's
// few inputs and a ones channel, ops.pack_convnext_composed): with <= 8 input channels a 16-byte B fragment is ALL the channels of a
// pixel, so a K = 32 step is FOUR (8-channel, tap) units -- lane group g reads the fragment of tap 4 s + g -- and the 49 taps take
// 13 steps instead of the 49 a 16-channel chunk costs on the kernel above.  The same block (512 threads, 64 channels x 8 rows x 32
// pixels, 2 m-tiles x 2 channel groups, 4 n-tiles per wave), fragments, XCD block map and bias-only NCHW epilogue.
//   input tile: one k half only, [piece 3][14 rows][38 px] x 16 B = 25 536 bytes, staged ONCE per block (two entries per thread;
//   channels >= Cin and pixels outside the image come back as 0.0 from the range check); nothing is refilled in the step loop.
//   taps 49 .. 51 (the padding of the last step) have zero weights; their B address is that of tap 48: staged, finite data.
//   weights: one slice [piece][k group 4][64][8] per step (group g of step s = tap 4 s + g) through the two-slot LDS-DMA ring of
//   the kernel above: slice s + 1 is requested behind the first n-tile of step s and has landed at the step's one barrier.
//   With 13 steps a tile's fill (the staging round trip) and drain (64 KB of stores) weigh as much as its loop, and nothing inside a
//   block overlaps them: the block needs 50 112 bytes of LDS and <= 128 registers, so TWO blocks share a CU and one block's steps run
//   under the other's fill and drain (and under its barriers).
namespace few {
constexpr int XR = TR + 6, XC = TC + 6, EPK = XR * XC;      // 14 x 38 = 532 entries
constexpr int XPB = EPK * 16;                               // one piece plane: 8512 bytes (= 64 modulo 256)
constexpr int NSTEP = 13, CT = 64, MPW = 2, WM = 2, WN = 4, RW = 2, NT = 4;
constexpr int WSL = 3 * 4 * CT * 16;                        // one weight slice: 12 288 bytes
constexpr int OFF_W = 3 * XPB, LDS = OFF_W + 2 * WSL;       // 50 112 bytes
static_assert(2 * 512 >= EPK && 2 * LDS <= 160 * 1024, "few-channel 7x7: staging map / two blocks per CU");
}  // namespace few

template <bool SIX, bool F16>
__global__ __launch_bounds__(512, 2) void conv7x7_few_split_kernel(SParams p) {
    using namespace few;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int plane = p.H * p.W * 4;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int NQ = SIX ? 3 : 1;
    const int b = blockIdx.z;
    int sp;                                              // (one cout tile: Cout <= 64) the XCD map of the kernel above
    if (p.xcd_map && (p.ntiles & 7) == 0) sp = (blockIdx.x & 7) * (p.ntiles >> 3) + (blockIdx.x >> 3);
    else sp = blockIdx.x;
    const int row0 = (sp / p.tiles_x) * TR, col0 = (sp % p.tiles_x) * TC;

    // ---- weight slices by LDS-DMA, 1 KB pieces dealt over the waves (plain 16-bit operands: the leading piece plane only)
    constexpr int NPC = (SIX ? WSL : WSL / 3) / 1024;
    const auto rw = CWFA_RSRC(p.wp, NSTEP * WSL);
    auto dma_w = [&](int slice, int slot) {
        cwfa_static_for<(NPC + 7) / 8>([&](auto ic_) {
            constexpr int i = decltype(ic_)::value;
            const int piece = i * 8 + wave;
            if (piece < NPC) {                           // wave-uniform
                char* dst = lds + OFF_W + slot * WSL + piece * 1024;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)dst, 16, (unsigned)(lane * 16), slice * WSL + piece * 1024, 0, 0);
            }
        });
    };

    // ---- the input tile, once: entries tid and tid + 512 of the 532; the eight channels of a pixel -> three 16-byte pieces
    {
        const auto rx = CWFA_RSRC(p.x + (int64_t)b * p.x_bs, p.Cin * plane);       // channels >= Cin: out of range, 0.0
        float xv[2][8];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = tid + 512 * k, r = e / XC, c = e % XC;
            const int gr = row0 + r - 3, gc = col0 + c - 3;
            const bool ok = e < EPK && gr >= 0 && gr < p.H && gc >= 0 && gc < p.W;
            const unsigned fo = ok ? (unsigned)((gr * p.W + gc) * 4) : OOB;
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[k][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, fo, j * plane, 0));
        }
        dma_w(0, 0);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = tid + 512 * k;
            bf16x8 pc[3];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 a1, a2 = (__bf16)0.f, a3 = (__bf16)0.f;
                cwfa_split3<SIX, F16>(xv[k][j], a1, a2, a3);
                pc[0][j] = a1; pc[1][j] = a2; pc[2][j] = a3;
            }
            if (e < EPK) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) *reinterpret_cast<bf16x8*>(lds + q * XPB + e * 16) = pc[q];
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const int alane = OFF_W + (g * CT + wm * MPW * 16 + c16) * 16;       // + slot*WSL + (q*4*CT + mt*16)*16
    const int blane = (wn * RW * XC + c16) * 16;                         // + tap offset + q*XPB + ((nt>>1)*XC + 16*(nt&1))*16
    // B-fragment base of step s for this lane group: tap 4 s + g, the padding taps of the last step on tap 48's (staged) data
    auto bbase_of = [&](int s) {
        const int t = 4 * s + g < 48 ? 4 * s + g : 48;
        return blane + ((t / 7) * XC + t % 7) * 16;
    };

    f32x4 acc[MPW][NT];
#pragma unroll
    for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 A[MPW][3], Bq[2][3];
    auto read_b = [&](int set, int bbase, int nt) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            Bq[set][q] = *reinterpret_cast<const bf16x8*>(lds + bbase + q * XPB + ((nt >> 1) * XC + 16 * (nt & 1)) * 16);
    };
    auto mfma6 = [&](f32x4& c, const bf16x8 (&a)[3], const bf16x8 (&bb)[3]) {
        if constexpr (SIX) {
            CWFA_MFMA(a[2], bb[0], c);
            CWFA_MFMA(a[1], bb[1], c);
            CWFA_MFMA(a[0], bb[2], c);
            CWFA_MFMA(a[1], bb[0], c);
            CWFA_MFMA(a[0], bb[1], c);
        }
        CWFA_MFMA_OP(F16, a[0], bb[0], c);
    };

    int bbase = bbase_of(0);
    read_b(0, bbase, 0);
    int sl = 0;
#pragma unroll 1
    for (int step = 0; step < NSTEP; ++step) {           // rolled: the accumulators are loop-carried (see the kernel above)
        const int abase = alane + sl * WSL;
#pragma unroll
        for (int mt = 0; mt < MPW; ++mt)
#pragma unroll
            for (int q = 0; q < NQ; ++q) A[mt][q] = *reinterpret_cast<const bf16x8*>(lds + abase + (q * 4 * CT + mt * 16) * 16);
        CWFA_FENCE();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (nt + 1 < NT) read_b((nt + 1) & 1, bbase, nt + 1);
            CWFA_FENCE();
#pragma unroll
            for (int mt = 0; mt < MPW; ++mt) {
                mfma6(acc[mt][nt], A[mt], Bq[nt & 1]);
                CWFA_FENCE();
            }
            // the next slice, from inside the MFMA stream; its slot was last read in the step before this one's barrier
            if (nt == 0 && step + 1 < NSTEP) {
                dma_w(step + 1, sl ^ 1);
                CWFA_FENCE();
            }
        }
        bbase = bbase_of(step + 1 < NSTEP ? step + 1 : step);     // (last step: a staged address, read and dropped)
        read_b(0, bbase, 0);
        CWFA_FENCE();
        // the next slice has landed; every LDS read of this step but the B fragments just requested is done
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (SIX) asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        sl ^= 1;
    }

    // ---- epilogue (bias only, NCHW): accumulator register r of tile (mt, nt) = channel (wm*MPW + mt)*16 + 4g + r, pixel
    // (row0 + 2 wn + nt/2, col0 + 16 (nt&1) + c16); the descriptor ends at channel Cout, pixels outside the image are out of range
    const auto ry = CWFA_RSRC(p.y + (int64_t)b * p.y_bs, p.Cout * plane);
    const auto rb = CWFA_RSRC(p.o.bias ? p.o.bias : p.y, p.o.bias ? p.Cout * 4 : 0);
    const int cwave = wm * MPW * 16;
    const unsigned glane = (unsigned)(4 * g) * (unsigned)plane;
    // cwfa_conv_opts.out_sample_stats: (sum, sum of squares) of the values stored below, for the LayerNorm over (C,H,W) behind this
    // convolution -- float64 from the first addition (32 values per thread), pixels outside the image and channels >= Cout left out
    const bool want_stats = p.o.out_sample_stats != nullptr;       // (uniform)
    double ssum = 0.0, ssq = 0.0;
#pragma unroll
    for (int mt = 0; mt < MPW; ++mt) {
        float bias[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            bias[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, (unsigned)(16 * g), (cwave + mt * 16 + r) * 4, 0));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int row = row0 + wn * RW + (nt >> 1), col = col0 + 16 * (nt & 1) + c16;
            const unsigned po = (row < p.H && col < p.W) ? (unsigned)((row * p.W + col) * 4) + glane : OOB;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[mt][nt][r] + bias[r];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[r]), ry, po, (cwave + mt * 16 + r) * plane, 0);
            }
            if (want_stats) {                             // one uniform branch per n-tile; the masks are selects
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double dv = (po != OOB && cwave + mt * 16 + 4 * g + r < p.Cout) ? (double)v[r] : 0.0;
                    ssum += dv;
                    ssq += dv * dv;
                }
            }
            CWFA_FENCE();
        }
    }
    if (want_stats) {                                     // block sum -> one float64 atomic pair per block
        ssum = cwfa_wave_sum(ssum);
        ssq = cwfa_wave_sum(ssq);
        double* red = reinterpret_cast<double*>(lds);      // the operand buffers are dead (every wave passed the loop's last barrier)
        if (lane == 0) {
            red[2 * wave] = ssum;
            red[2 * wave + 1] = ssq;
        }
        __syncthreads();
        if (tid == 0) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int w = 0; w < 8; ++w) {
                t1 += red[2 * w];
                t2 += red[2 * w + 1];
            }
            atomicAdd(&p.o.out_sample_stats[2 * b], t1);
            atomicAdd(&p.o.out_sample_stats[2 * b + 1], t2);
        }
    }
}

// its packed image: [step 13][piece 3][k group 4][64][8] of bf16, group g of step s = tap 4 s + g: element j = w[co][j][tap]
// (0 beyond Cout / Cin / tap 48); F16 as below
template <bool F16>
__global__ __launch_bounds__(256) void split7x7_few_pack_kernel(const float* __restrict__ w, uint4* __restrict__ out, int Cout, int Cin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;                    // over [step][g 4][co 64]
    if (i >= few::NSTEP * 4 * 64) return;
    const int co = i % 64, g = (i / 64) % 4, s = i / 256, tap = 4 * s + g;
    unsigned short pc[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = 0.f;
        if (co < Cout && j < Cin && tap < 49) v = w[((int64_t)co * Cin + j) * 49 + tap];
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
        uint4 v4;
        v4.x = pc[q][0] | ((unsigned)pc[q][1] << 16);
        v4.y = pc[q][2] | ((unsigned)pc[q][3] << 16);
        v4.z = pc[q][4] | ((unsigned)pc[q][5] << 16);
        v4.w = pc[q][6] | ((unsigned)pc[q][7] << 16);
        out[((s * 3 + q) * 4 + g) * 64 + co] = v4;
    }
}

// packed image: [cout tile][step][piece 3][k group 4][CT][8] of bf16; group g of step s = unit u = 2s + (g >> 1) =
// (chunk u / 9, tap u % 9), k half g & 1: element j = w[co][chunk*16 + (g&1)*8 + j][tap] (0 beyond Cout / Cin / the last unit)
// F16: piece 0 holds the fp16 weights, pieces 1 and 2 are zero (the same image size and layout)
template <int CT, bool F16 = false>
__global__ __launch_bounds__(256) void split3x3_pack_kernel(const float* __restrict__ w, uint4* __restrict__ out, int Cout, int Cin,
                                                            int nchunks, int nsteps, int64_t total, int ntap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // over [ctile][step][g 4][co CT]
    if (i >= total) return;
    const int col = (int)(i % CT), g = (int)((i / CT) % 4), s = (int)((i / (4 * CT)) % nsteps), ctile = (int)(i / ((int64_t)4 * CT * nsteps));
    const int u = 2 * s + (g >> 1), chunk = u / ntap, tap = u % ntap, co = ctile * CT + col;
    unsigned short pc[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = chunk * 16 + (g & 1) * 8 + j;
        float v = 0.f;
        if (co < Cout && ci < Cin && chunk < nchunks) v = w[((int64_t)co * Cin + ci) * ntap + tap];
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
        uint4 v4;
        v4.x = pc[q][0] | ((unsigned)pc[q][1] << 16);
        v4.y = pc[q][2] | ((unsigned)pc[q][3] << 16);
        v4.z = pc[q][4] | ((unsigned)pc[q][5] << 16);
        v4.w = pc[q][6] | ((unsigned)pc[q][7] << 16);
        out[(((int64_t)ctile * nsteps + s) * 3 + q) * 4 * CT + g * CT + col] = v4;
    }
}

// (m-tiles per wave, channel groups per block) by bank size -- packing and launch must agree.  WM = 4: 64 / 128 / 256 channels per
// block on 8-row tiles (64: also 16-row).  The narrow tilings (16-row tile, no load-side prologue) fit the small banks WITHOUT zero
// rows and with more m-tiles per B fragment: 16 = (1,1); 32 = (2,1); 48 = (3,1): the 64 -> 48 output convolutions of the sub-networks
// (on the 64-channel tiling a B fragment fed ONE m-tile and a quarter of the MFMAs ran on zero rows); 96 = (3,2): the 64 -> 96 ones
// (a quarter of the 128-channel tiling was zero rows).
inline int mpw_of(int Cout) { return Cout > 128 ? 4 : Cout > 96 ? 2 : Cout > 64 ? 3 : Cout > 48 ? 1 : Cout > 32 ? 3 : Cout > 16 ? 2 : 1; }
inline int wm_of(int Cout) { return Cout > 96 ? 4 : Cout > 64 ? 2 : Cout > 48 ? 4 : 1; }
inline int ct_of(int Cout) { return 16 * mpw_of(Cout) * wm_of(Cout); }
inline int nsteps_of(int Cin, int ntap = 9) { return ntap * (((Cin + 15) / 16 + 1) / 2); }   // whole periods of two 16-channel chunks

template <int MPW, bool ADD, int ACT1, int KS = 3, int RPW = 4, int WM = 4>
int launch(const SParams& p, hipStream_t stream) {
    typedef Geo<MPW, KS, RPW, WM> G;
    constexpr int TRW = XG<KS, RPW>::TRW;
    const int tiles_y = (p.H + TRW - 1) / TRW, ctiles = (p.Cout + G::CT - 1) / G::CT;
    SParams q = p;
    q.ntiles = p.tiles_x * tiles_y;
    q.ctiles = ctiles;
    q.xcd_map = g_cwfa_split_xcd_map;
    if ((int64_t)q.ntiles * ctiles >= (1ll << 31)) {
        cwfa_set_error("cwfa_conv3x3_split_f32: grid too large");
        return CWFA_E_SHAPE;
    }
    // the run-time and coupling epilogues write neither statistics nor a channel-blocked output: a dispatch that lands here
    // with either requested would drop them silently
    if ((ACT1 == EPI_RUNTIME || ACT1 == EPI_COUPLE) && (p.o.out_stats || p.o.out_blocked8)) {
        cwfa_set_error("cwfa_conv3x3_split_f32: out_stats / out_blocked8 reached a run-time epilogue");
        return CWFA_E_INVAL;
    }
    return cwfa_with_operand([&](auto six, auto f16) -> int {
        constexpr auto kern = &conv3x3_split_kernel<MPW, six, ADD, ACT1, KS, RPW, WM, f16>;
        const int rc = cwfa_max_lds<kern>(G::LDS, "cwfa_conv3x3_split_f32");
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)(q.ntiles * ctiles), 1, p.B), dim3(512), G::LDS, stream, q);
        CWFA_LAUNCH_CHECK("cwfa_conv3x3_split_f32");
        return CWFA_OK;
    });
}

template <int MPW>
int launch_epi(const SParams& p, hipStream_t st) {
    const bool plain = !p.o.residual && p.o.act2 == CWFA_ACT_NONE;
    if (p.o.in_add) {
        if (plain && p.o.act == CWFA_ACT_PRELU) return launch<MPW, true, CWFA_ACT_PRELU>(p, st);
        return launch<MPW, true, EPI_RUNTIME>(p, st);
    }
    if (plain && p.o.act == CWFA_ACT_PRELU) return launch<MPW, false, CWFA_ACT_PRELU>(p, st);
    if (plain && p.o.act == CWFA_ACT_NONE) return launch<MPW, false, CWFA_ACT_NONE>(p, st);
    return launch<MPW, false, EPI_RUNTIME>(p, st);
}

// the weight image of a bank for ct output channels per block (ct_of; the 7x7: 64) in the active operand format
void pack_bank(const float* w, void* packed, int Cout, int Cin, int ct, int ntap, hipStream_t st) {
    const int nchunks = (Cin + 15) / 16, nsteps = nsteps_of(Cin, ntap);
    const int64_t total = (int64_t)((Cout + ct - 1) / ct) * nsteps * 4 * ct;
    cwfa_with_operand([&](auto, auto f16) -> int {
        auto go = [&](auto CT) {
            hipLaunchKernelGGL((split3x3_pack_kernel<decltype(CT)::value, f16>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w,
                               reinterpret_cast<uint4*>(packed), Cout, Cin, nchunks, nsteps, total, ntap);
        };
        if (ct == 16) go(cwfa_ic<16>{});
        else if (ct == 32) go(cwfa_ic<32>{});
        else if (ct == 48) go(cwfa_ic<48>{});
        else if (ct == 96) go(cwfa_ic<96>{});
        else if (ct == 128) go(cwfa_ic<128>{});
        else if (ct == 256) go(cwfa_ic<256>{});
        else go(cwfa_ic<64>{});
        return CWFA_OK;
    });
}

}  // namespace

// packed row r of a coupling bank <- source row of the torch weight [2n, Cin, 3, 3] (s_j = row j, t_j = row n + j), -1 = zero row
static int couple_row_source(int n, int r) {
    int j, which;
    if (n <= 32) {                         // MPW = 1: row = 16 wm + 4 g + (h + 2 which), j = 8 wm + 2 g + h
        const int wm = r >> 4, g = (r >> 2) & 3, q = r & 3;
        j = 8 * wm + 2 * g + (q & 1);
        which = q >> 1;
    } else {                               // MPW = 2: row = 16 (2 wm + which) + 4 g + r4, j = 16 wm + 4 g + r4
        const int wm = r >> 5;
        which = (r >> 4) & 1;
        j = 16 * wm + (r & 15);
    }
    return j < n ? which * n + j : -1;
}

extern "C" int cwfa_couple_rows(int n, int* rows) {
    if (n <= 0 || n > 64) return -1;
    const int total = n <= 32 ? 64 : 128;
    if (rows)
        for (int r = 0; r < total; ++r) rows[r] = couple_row_source(n, r);
    return total;
}

extern "C" int cwfa_conv3x3_split_couple_f32(const float* x, const void* w_packed, const float* bias_rows, int B, int Cin, int H, int W,
                                             int64_t x_bs, const cwfa_couple* cp, void* stream) {
    CWFA_REQUIRE(B >= 0 && Cin > 0 && H >= 0 && W >= 0, CWFA_E_INVAL, "cwfa_conv3x3_split_couple_f32: bad size");
    CWFA_REQUIRE(cp, CWFA_E_INVAL, "cwfa_conv3x3_split_couple_f32: null coupling descriptor");
    CWFA_REQUIRE(cp->n > 0 && cp->n <= 64, CWFA_E_SHAPE, "cwfa_conv3x3_split_couple_f32: 1 <= n <= 64 (got %d)", cp->n);
    if (B == 0 || H == 0 || W == 0) return CWFA_OK;
    CWFA_REQUIRE(x && w_packed && cp->x && cp->y, CWFA_E_INVAL, "cwfa_conv3x3_split_couple_f32: null pointer");
    CWFA_REQUIRE(cwfa_aligned16(w_packed), CWFA_E_ALIGN, "cwfa_conv3x3_split_couple_f32: packed weights must be 16-byte aligned");
    CWFA_REQUIRE(cp->clamp_kind >= CWFA_CLAMP_NONE && cp->clamp_kind <= CWFA_CLAMP_SIGMOID, CWFA_E_INVAL,
                 "cwfa_conv3x3_split_couple_f32: bad clamp kind %d", cp->clamp_kind);
    SParams p{};
    p.x = x; p.wp = w_packed; p.y = cp->y;
    p.B = B; p.Cin = Cin; p.H = H; p.W = W; p.x_bs = x_bs; p.y_bs = cp->y_bs;
    p.Cout = cwfa_couple_rows(cp->n, nullptr);
    p.o.bias = bias_rows;
    p.o.in_blocked8 = cp->in_blocked8;
    CWFA_REQUIRE(!cp->in_blocked8 || (Cin % 8 == 0 && cwfa_aligned16(x) && (x_bs & 3) == 0), CWFA_E_ALIGN,
                 "cwfa_conv3x3_split_couple_f32: blocked input needs Cin %% 8 == 0 and 16-byte alignment");
    p.cp = *cp;
    p.nchunks = (Cin + 15) / 16;
    p.nsteps = nsteps_of(Cin);
    p.nrun = p.nsteps - ((p.nchunks & 1) ? 4 : 0);
    p.tiles_x = (W + TC - 1) / TC;
    CWFA_REQUIRE((int64_t)(Cin + 64) * H * W * 4 < (1ll << 31) && (int64_t)(cp->n + 64) * H * W * 4 < (1ll << 31), CWFA_E_SHAPE,
                 "cwfa_conv3x3_split_couple_f32: one sample's input / active half must stay below 2 GiB");
    CWFA_REQUIRE((int64_t)p.tiles_x * ((H + TR - 1) / TR) < (1ll << 31) && B <= 65535, CWFA_E_SHAPE,
                 "cwfa_conv3x3_split_couple_f32: grid too large");
    hipStream_t st = (hipStream_t)stream;
    if (p.Cout == 64) {
        if (g_cwfa_split_rows16 && H > 8)       // 16-row tiles (no load-side prologue here by construction)
            return launch<1, false, EPI_COUPLE, 3, 8>(p, st);
        return launch<1, false, EPI_COUPLE>(p, st);
    }
    return launch<2, false, EPI_COUPLE>(p, st);
}

extern "C" int64_t cwfa_conv3x3_split_packed_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0) return -1;
    const int ct = ct_of(Cout);
    return (int64_t)((Cout + ct - 1) / ct) * nsteps_of(Cin) * 3 * 4 * ct * 16;
}

extern "C" int cwfa_conv3x3_split_pack_f32(const float* w, void* packed, int Cout, int Cin, void* stream) {
    CWFA_REQUIRE(w && packed, CWFA_E_INVAL, "cwfa_conv3x3_split_pack_f32: null pointer");
    CWFA_REQUIRE(Cout > 0 && Cin > 0, CWFA_E_SHAPE, "cwfa_conv3x3_split_pack_f32: bad shape");
    CWFA_REQUIRE(cwfa_aligned16(packed), CWFA_E_ALIGN, "cwfa_conv3x3_split_pack_f32: packed image must be 16-byte aligned");
    pack_bank(w, packed, Cout, Cin, ct_of(Cout), 9, (hipStream_t)stream);
    CWFA_LAUNCH_CHECK("cwfa_conv3x3_split_pack_f32");
    return CWFA_OK;
}

extern "C" int cwfa_conv3x3_split_f32(const float* x, const void* w_packed, float* y, int B, int Cin, int H, int W, int Cout,
                                      int64_t x_bs, int64_t y_bs, const cwfa_conv_opts* opts, void* stream) {
    CWFA_REQUIRE(B >= 0 && Cin > 0 && Cout > 0 && H >= 0 && W >= 0, CWFA_E_INVAL, "cwfa_conv3x3_split_f32: bad size");
    if (B == 0 || H == 0 || W == 0) return CWFA_OK;
    CWFA_REQUIRE(x && w_packed && y, CWFA_E_INVAL, "cwfa_conv3x3_split_f32: null pointer");
    CWFA_REQUIRE(cwfa_aligned16(w_packed), CWFA_E_ALIGN, "cwfa_conv3x3_split_f32: packed weights must be 16-byte aligned");
    SParams p{};
    p.x = x; p.wp = w_packed; p.y = y;
    p.B = B; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.x_bs = x_bs; p.y_bs = y_bs;
    if (opts) p.o = *opts;
    CWFA_REQUIRE(!p.o.upshuffle2 && !p.o.in_cat, CWFA_E_SHAPE, "cwfa_conv3x3_split_f32: upshuffle2 / in_cat are 1x1 features");
    CWFA_REQUIRE(!p.o.out_sample_stats, CWFA_E_INVAL, "cwfa_conv3x3_split_f32: out_sample_stats is a feature of the few-channel cwfa_conv7x7_split_f32");
    CWFA_REQUIRE(!p.o.in_blocked8 || (Cin % 8 == 0 && cwfa_aligned16(x) && (x_bs & 3) == 0 && !p.o.in_add), CWFA_E_ALIGN,
                 "cwfa_conv3x3_split_f32: blocked input needs Cin %% 8 == 0, 16-byte alignment and no added tensor");
    CWFA_REQUIRE(!p.o.out_blocked8 || (Cout % 8 == 0 && cwfa_aligned16(y) && (y_bs & 3) == 0 && !p.o.residual && p.o.act2 == CWFA_ACT_NONE &&
                                       (p.o.act == CWFA_ACT_NONE || p.o.act == CWFA_ACT_PRELU)),
                 CWFA_E_ALIGN, "cwfa_conv3x3_split_f32: blocked output needs Cout %% 8 == 0, 16-byte alignment and a bias / PReLU epilogue");
    CWFA_REQUIRE(!(p.o.in_scale && !p.o.in_shift), CWFA_E_INVAL, "cwfa_conv3x3_split_f32: in_scale without in_shift");
    CWFA_REQUIRE(!p.o.out_stats || (!p.o.out_blocked8 && !p.o.residual && p.o.act2 == CWFA_ACT_NONE &&
                                    (p.o.act == CWFA_ACT_NONE || p.o.act == CWFA_ACT_PRELU)),
                 CWFA_E_INVAL, "cwfa_conv3x3_split_f32: out_stats needs an NCHW output and a bias / PReLU epilogue");
    // (a skip add with a bias-only epilogue runs on the run-time epilogue, which writes neither: launch_epi)
    CWFA_REQUIRE(!((p.o.out_stats || p.o.out_blocked8) && p.o.in_add && p.o.act == CWFA_ACT_NONE), CWFA_E_INVAL,
                 "cwfa_conv3x3_split_f32: out_stats / out_blocked8 with in_add need a PReLU epilogue");
    CWFA_REQUIRE(p.o.act >= 0 && p.o.act <= CWFA_ACT_RELU && p.o.act2 >= 0 && p.o.act2 <= CWFA_ACT_RELU, CWFA_E_INVAL,
                 "cwfa_conv3x3_split_f32: bad activation");
    CWFA_REQUIRE(!((p.o.act == CWFA_ACT_PRELU || p.o.act2 == CWFA_ACT_PRELU) && !p.o.prelu_alpha), CWFA_E_INVAL,
                 "cwfa_conv3x3_split_f32: PReLU without prelu_alpha");
    p.nchunks = (Cin + 15) / 16;
    p.nsteps = nsteps_of(Cin);
    // an odd number of 16-channel chunks: the last period's odd chunk is all zeros and the steps that pair ONLY its taps (positions 5 .. 8 of
    // the period: odd taps (1,2) (3,4) (5,6) (7,8)) add nothing -- not run (a 6 -> 256 convolution: five steps instead of nine)
    p.nrun = p.nsteps - ((p.nchunks & 1) ? 4 : 0);
    p.tiles_x = (W + TC - 1) / TC;
    const int mpw = mpw_of(Cout);
    CWFA_REQUIRE((int64_t)(Cin + 64) * H * W * 4 < (1ll << 31) && (int64_t)(Cout + 64 * mpw) * H * W * 4 < (1ll << 31) &&
                     (int64_t)(p.nsteps + 2) * 3 * 4 * 64 * mpw * 16 < (1ll << 31), CWFA_E_SHAPE,
                 "cwfa_conv3x3_split_f32: one sample's input / output / one cout tile's weights must stay below 2 GiB");
    CWFA_REQUIRE((int64_t)p.tiles_x * ((H + TR - 1) / TR) < (1ll << 31) && B <= 65535, CWFA_E_SHAPE, "cwfa_conv3x3_split_f32: grid too large");
    hipStream_t st = (hipStream_t)stream;
    const int wm = wm_of(Cout);
    if (wm != 4) {       // narrow tilings (<= 48 or 65 .. 96 outputs): 16-row tile, no load-side prologue, NCHW / blocked input, bias / PReLU / generic epilogue
        CWFA_REQUIRE(!p.o.in_scale && !p.o.in_add && !p.o.out_blocked8, CWFA_E_INVAL,
                     "cwfa_conv3x3_split_f32: banks with <= 48 or 65 .. 96 outputs take no load-side prologue and write NCHW");
        const bool plain = !p.o.residual && p.o.act2 == CWFA_ACT_NONE;
        const int epi = plain && p.o.act == CWFA_ACT_NONE ? 0 : plain && p.o.act == CWFA_ACT_PRELU ? 1 : 2;
#define CWFA_NARROW(M, W_)                                                                                                                   \
    do {                                                                                                                                     \
        if (epi == 0) return launch<M, false, CWFA_ACT_NONE, 3, 8, W_>(p, st);                                                               \
        if (epi == 1) return launch<M, false, CWFA_ACT_PRELU, 3, 8, W_>(p, st);                                                              \
        return launch<M, false, EPI_RUNTIME, 3, 8, W_>(p, st);                                                                               \
    } while (0)
        if (mpw == 3 && wm == 2) CWFA_NARROW(3, 2);
        if (mpw == 3) CWFA_NARROW(3, 1);
        if (mpw == 2) CWFA_NARROW(2, 1);
        CWFA_NARROW(1, 1);
#undef CWFA_NARROW
    }
    if (mpw == 4) return launch_epi<4>(p, st);
    if (mpw == 2) return launch_epi<2>(p, st);
    // 64-channel tiling: 16-row tiles for the plain bias-only form (the output convolutions of the sub-networks)
    if (g_cwfa_split_rows16 && H > 8 && !p.o.in_scale && !p.o.in_add && !p.o.residual && p.o.act == CWFA_ACT_NONE && p.o.act2 == CWFA_ACT_NONE)
        return launch<2, false, CWFA_ACT_NONE, 3, 8, 2>(p, st);
    // (two m-tiles per wave x two channel groups instead of one x four: the same 64 channels per block and the same packed image, but a
    //  B fragment feeds two m-tiles -- 30 instead of 51 ds_read_b128 per 96 MFMAs)
    // ... and for any other epilogue without a load-side prologue (activation / residual / second activation: the data-gradient and
    // unfused forward convolutions of the sub-networks in training, 64 -> 64): 160 -> ~100 us at 512 x 512; not when statistics or a
    // blocked output are asked for (only the compile-time epilogues write them: a plain PReLU then takes launch_epi<1>)
    if (g_cwfa_split_rows16 && H > 8 && !p.o.in_scale && !p.o.in_add && !p.o.out_stats && !p.o.out_blocked8)
        return launch<2, false, EPI_RUNTIME, 3, 8, 2>(p, st);
    return launch_epi<1>(p, st);
}

// ------------------------------------------------------------------------------------------------ 7x7 (ConvNeXt, networks.py:488)
extern "C" int64_t cwfa_conv7x7_split_packed_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cout > 64 || Cin <= 0) return -1;
    if (Cin <= 8) return (int64_t)few::NSTEP * few::WSL;          // the few-channel form: 13 slices of four (8-channel, tap) units
    return (int64_t)nsteps_of(Cin, 49) * 3 * 4 * 64 * 16;
}

extern "C" int cwfa_conv7x7_split_pack_f32(const float* w, void* packed, int Cout, int Cin, void* stream) {
    CWFA_REQUIRE(w && packed, CWFA_E_INVAL, "cwfa_conv7x7_split_pack_f32: null pointer");
    CWFA_REQUIRE(Cout > 0 && Cout <= 64 && Cin > 0, CWFA_E_SHAPE, "cwfa_conv7x7_split_pack_f32: 1 <= Cout <= 64");
    CWFA_REQUIRE(cwfa_aligned16(packed), CWFA_E_ALIGN, "cwfa_conv7x7_split_pack_f32: packed image must be 16-byte aligned");
    if (Cin <= 8) {
        cwfa_with_operand([&](auto, auto f16) -> int {
            hipLaunchKernelGGL((split7x7_few_pack_kernel<f16>), dim3((few::NSTEP * 4 * 64 + 255) / 256), dim3(256), 0, (hipStream_t)stream, w,
                               reinterpret_cast<uint4*>(packed), Cout, Cin);
            return CWFA_OK;
        });
    } else {
        pack_bank(w, packed, Cout, Cin, 64, 49, (hipStream_t)stream);
    }
    CWFA_LAUNCH_CHECK("cwfa_conv7x7_split_pack_f32");
    return CWFA_OK;
}

extern "C" int cwfa_conv7x7_split_f32(const float* x, const void* w_packed, float* y, int B, int Cin, int H, int W, int Cout,
                                      int64_t x_bs, int64_t y_bs, const cwfa_conv_opts* opts, void* stream) {
    CWFA_REQUIRE(B >= 0 && Cin > 0 && Cout > 0 && Cout <= 64 && H >= 0 && W >= 0, CWFA_E_INVAL, "cwfa_conv7x7_split_f32: bad size (Cout <= 64)");
    if (B == 0 || H == 0 || W == 0) return CWFA_OK;
    CWFA_REQUIRE(x && w_packed && y, CWFA_E_INVAL, "cwfa_conv7x7_split_f32: null pointer");
    CWFA_REQUIRE(cwfa_aligned16(w_packed), CWFA_E_ALIGN, "cwfa_conv7x7_split_f32: packed weights must be 16-byte aligned");
    SParams p{};
    p.x = x; p.wp = w_packed; p.y = y;
    p.B = B; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.x_bs = x_bs; p.y_bs = y_bs;
    if (opts) p.o = *opts;
    CWFA_REQUIRE(!p.o.upshuffle2 && !p.o.in_cat && !p.o.in_scale && !p.o.in_add && !p.o.in_blocked8 && !p.o.out_blocked8 && !p.o.residual && !p.o.out_stats &&
                     p.o.act == CWFA_ACT_NONE && p.o.act2 == CWFA_ACT_NONE,
                 CWFA_E_INVAL, "cwfa_conv7x7_split_f32: bias-only epilogue, no load-side prologue, NCHW maps");
    CWFA_REQUIRE(!p.o.out_sample_stats || Cin <= 8, CWFA_E_INVAL, "cwfa_conv7x7_split_f32: out_sample_stats is written by the few-channel form (Cin <= 8) only");
    p.nchunks = (Cin + 15) / 16;
    p.nsteps = nsteps_of(Cin, 49);
    // a single 16-channel chunk (9 .. 16 inputs): the odd chunk of the one period is all zeros (zero-filled in steps 0 .. 2, zero weights) and
    // the steps that pair ONLY its taps add nothing -- taps (0,1) .. (46,47), then tap 48 with the odd buffer's tap 0: 25 steps of the 49
    p.nrun = p.nchunks == 1 ? 25 : p.nsteps;
    p.tiles_x = (W + TC - 1) / TC;
    CWFA_REQUIRE((int64_t)(Cin + 64) * H * W * 4 < (1ll << 31) && (int64_t)(Cout + 64) * H * W * 4 < (1ll << 31), CWFA_E_SHAPE,
                 "cwfa_conv7x7_split_f32: one sample's input / output must stay below 2 GiB");
    CWFA_REQUIRE((int64_t)p.tiles_x * ((H + TR - 1) / TR) < (1ll << 31) && B <= 65535, CWFA_E_SHAPE, "cwfa_conv7x7_split_f32: grid too large");
    hipStream_t st = (hipStream_t)stream;
    if (Cin <= 8) {                        // the few-channel form: 13 steps of four (8-channel, tap) units
        p.ntiles = p.tiles_x * ((H + TR - 1) / TR);
        p.ctiles = 1;
        p.xcd_map = g_cwfa_split_xcd_map;
        return cwfa_with_operand([&](auto six, auto f16) -> int {
            constexpr auto kern = &conv7x7_few_split_kernel<six, f16>;
            const int rc = cwfa_max_lds<kern>(few::LDS, "cwfa_conv7x7_split_f32");
            if (rc) return rc;
            hipLaunchKernelGGL(kern, dim3((unsigned)p.ntiles, 1, B), dim3(512), few::LDS, st, p);
            CWFA_LAUNCH_CHECK("cwfa_conv7x7_split_f32");
            return CWFA_OK;
        });
    }
    // (2 m-tiles per wave x 2 channel groups: a B fragment feeds two m-tiles -- 18 instead of 27 ds_read_b128 per 48 MFMAs)
    return launch<2, false, CWFA_ACT_NONE, 7, 4, 2>(p, st);
}
