// Weight-streaming decode GEMM over fp8 (OCP e4m3) weights on gfx950, weight-only quantisation ("W8A16"):
//
//   y[m, n] = bf16( (sum_k x[m, k] f(w8[n, k])) s[n] + bias[n] )                        per-tensor / per-channel scales
//   y[m, n] = bf16(  sum_c s[n / 128, c] (sum_{k in chunk c} x[m, k] f(w8[n, k])) + bias[n] )      128 x 128 block scales
//
// x bf16, w8 e4m3 [N, K] (row stride in bytes, a multiple of 16), f the exact e4m3 -> bf16 widening (three significand
// bits fit), fp32 accumulation, fp32 scales.  The scale meets the fp32 accumulator before anything else does: before a
// split-K partial is written and before the one-pass silu, so the combine kernels of wstream_gemm.hip (bias, silu, add +
// RMSNorm, rope + KV store) run unchanged on scaled partials and every epilogue keeps its bf16 rounding points.
//
// Replaces, for decode-sized M over fp8 checkpoints, the reference's fp8 linear method (/root/reference/python/sglang:
// srt/layers/quantization/fp8.py Fp8LinearMethod.apply -> fp8_utils.py apply_fp8_linear: per-token activation quantisation +
// a scaled fp8 matmul, "w8a8").  This is deliberately NOT that arithmetic: the activations stay bf16, so the result is
// closer to the unquantised model than the reference's own fp8 path.  At decode sizes the GEMM is an HBM stream of W; the
// matrix pipes have slack for the bf16 MFMA behind an in-register widen, and halving the weight bytes is the lever.
// Oracle: fp64 (x . f(w8)^T) s + bias on the CPU.
//
// Same frame as wstream_gemm_kernel (one workgroup resident per CU, a wave owns 16-row weight tiles, weights and
// activations HBM -> LDS by global_load_lds dwordx4 into a ring, counters waited on by hand, XOR-swizzled images, the
// staggered K start without split-K, split-K partials in split order) with its own data movement:
//
//   * A 128-wide K chunk of a 16-row e4m3 tile is 2 KiB: two DMA instructions of 8 rows x 128 B (one whole cache line
//     per row).  With the bf16 ring geometry the weight bytes in flight per CU would halve.  A ring slot therefore
//     covers TWO chunks (256 K elements: 4 KiB per wave-tile, two 128-B lines per row) wherever a ring of three such
//     slots fits the 160 KiB; the activation image of the slot is the two consecutive 128-wide chunk images of the bf16
//     kernel, so row-major and chunk-major [K/128, M, 128] activations both keep working.  An odd chunk count (K = 896,
//     384, 128) ends in a half slot: the DMAs of its second chunk go to the dummy landing zone, its products are skipped.
//     Where three 256-wide slots do not fit (the activation image grows with M) the slot is one chunk wide and the ring
//     deeper.  Slot width x ring depth = weight bytes in flight per CU, next to the bf16 kernel's:
//
//       one tile per wave      NW = 4             5              6              7              8
//        MT 1 (<= 16 rows)  256x6  96K ( 96K) 256x5 100K (120K) 256x4  96K (120K) 256x4 112K (112K) 256x3  96K (128K)
//        MT 2               256x4  64K ( 96K) 256x4  80K (100K) 256x3  72K ( 96K) 256x3  84K (112K) 256x3  96K ( 96K)
//        MT 3               256x3  48K ( 80K) 256x3  60K ( 80K) 256x3  72K ( 96K) 256x3  84K ( 84K) 128x5  80K ( 96K)
//        MT 4 (<= 64 rows)  256x3  48K ( 64K) 256x3  60K ( 80K) 128x5  60K ( 72K) 128x5  70K ( 84K) 128x4  64K ( 96K)
//        MT 6 (<= 96 rows)  128x4  32K ( 48K) 128x4  40K ( 60K) 128x4  48K ( 72K) 128x4  56K ( 84K) 128x3  48K (  -- )
//        MT 8 (<= 128 rows) 128x3  24K ( 48K) 128x3  30K ( 60K) 128x3  36K (  -- ) 128x3  42K (  -- ) 128x3  48K (  -- )
//       two tiles per wave     NW = 2             3              4
//        MT 1               256x6  96K ( 96K) 256x4  96K (120K) 256x3  96K (128K)
//        MT 2               256x4  64K ( 96K) 256x3  72K ( 96K) 256x3  96K ( 96K)
//        MT 3               256x3  48K ( 80K) 256x3  72K ( 96K) 128x5  80K ( 96K)
//        MT 4               256x3  48K ( 64K) 128x5  60K ( 72K) 128x4  64K ( 96K)
//        MT 6               128x4  32K ( 48K) 128x4  48K ( 72K) 128x3  48K (  -- )
//        MT 8               128x3  24K ( 48K) 128x3  36K (  -- ) 128x3  48K (  -- )
//
//     Beyond 64 rows the 16-32 KiB activation image of a chunk owns the LDS whatever the weights weigh: there the fp8
//     ring holds half the bf16 ring's weight bytes (but takes every group size, the weights being half as large).
//
//   * Fragments.  The weight image of a chunk is [16 rows][128 B]; a lane (row r, lane group g) reads the 16-byte
//     pieces j * 4 + g, j = 0, 1, of its row: one ds_read_b128 feeds TWO 16x16x32 k-steps (bytes 0..7 -> step 2 j,
//     8..15 -> step 2 j + 1).  That permutes the k order inside a chunk; the activation side reads its 16-byte bf16
//     pieces in the same order ((j * 4 + g) * 2 + h for step 2 j + h), so both operands of every product agree on k.
//     Piece s of row r lives at position s ^ (r >> 1) of the row: the 16 lanes of one ds_read_b128 pass (16 rows, one
//     piece index) then cover 16 different 16-byte bank groups of the 256-byte bank line -- rows 128 B apart alternate
//     between its halves, r >> 1 spreads the eight rows of a half.  (The bf16 kernel's (s ^ r) & 15 is for 256-byte
//     rows.)  As there, the swizzle is applied on the global side of the DMA.  The widening (v_cvt_pk_f32_fp8 x 4 +
//     v_cvt_pk_bf16_f32 x 4 per fragment, fp8x8_to_bf16x8 of kv_format.hpp) of k-step s + 1 is issued ahead of the
//     MFMAs of k-step s.
//
//   * Scales.  Per-tensor / per-channel: one multiply when the accumulator leaves the main loop.  128 x 128 blocks
//     (template flag): a 16-row tile lies inside one block row and a 128-wide chunk is one block column, so every chunk
//     is accumulated on its own and folded into the running accumulator with one fp32 FMA per element by a wave-uniform
//     scale.  The scales are ordinary loads from a wave-uniform address, issued right behind the weight DMAs of their
//     slot (PD slots ahead) into a register queue: vector memory returns in order, so a load issued where the scale is
//     used would wait for the whole ring.
//
// Not built: the interleaved one-tile silu form (pair_silu == 2 of the bf16 kernel; the policy does not select it) and
// the grouped (MoE) form.
#include "common.hpp"
#include "kv_format.hpp"
#include "sglang_amd.h"
#include "wstream_combine.hpp"

using namespace sgl_amd;

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

constexpr int kKC = 128;              // K elements per chunk: 128 B of every weight row, 256 B of every activation row
constexpr int kKSteps = kKC / 32;     // MFMA k-steps per chunk
constexpr int kWTile = 16 * kKC;      // bytes of one 16-row weight tile of one chunk

struct W8Params {
  const uint16_t* x;        // [M, K] bf16 (row-major or chunk-major, see blocked_off() of wstream_gemm.hip)
  const unsigned char* w;   // [N, K] e4m3
  const uint16_t* bias;     // optional [N] (only applied when y is written directly)
  uint16_t* y;              // bf16 output (no partials)
  float* part;              // [splits, M, N] fp32 scaled partials, or NULL: write y directly
  const float* scale;       // mode 0: [1], 1: [N], 2: [ceil(N / 128), scale_stride >= K / 128]
  int64_t x_stride, w_stride /* bytes */, y_stride, x_cstride, y_cstride, scale_stride;
  int M, N, K, splits, ntiles;
  int scale_mode;
  int pair_silu;            // two-tile waves: y[:, 16 t ..] = silu(tile t) * tile (t + ntiles / 2)
  int plain_part;           // partial buffers of 2 GiB and more: plain stores (32-bit buffer offsets)
};

__device__ __forceinline__ int64_t blocked_off(int64_t m, int n, int64_t stride, int64_t cstride) {
  return static_cast<int64_t>(n >> 7) * cstride + m * stride + (n & 127);
}

// ---- LDS-DMA plumbing: as in wstream_gemm.hip (hipcc would order every LDS read it can see behind ALL pending LDS-DMA,
// so the fragment reads are inline-asm ds_read_b128 and both counters are waited on by hand)
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) unsigned char* lds_bytes_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

template <int AUX>
__device__ __forceinline__ void dma16(const void* src, lds_ptr_t dst) {
  __builtin_amdgcn_global_load_lds((glb_ptr_t)(src), dst, 16, 0, AUX);
}

template <int OFF>
__device__ __forceinline__ u32x4_t lds_rd(uint32_t addr) {
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}

template <int N>
__device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N)); }
__device__ __forceinline__ void pin(u32x4_t& v) { asm volatile("" : "+v"(v)); }

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ---- ring geometry: chunks per slot (2 where three such slots fit, else 1) and ring depth (LDS, at most 6, and the
// 6-bit vmcnt: the DMAs outstanding while chunk c is awaited must stay below 64)
struct Geo { int cps, pd; };
constexpr int slot_bytes(int mt, int nw, int tpw, int cps) { return cps * (nw * tpw * kWTile + mt * 4096); }
constexpr int vm_outstanding(int mt, int nw, int tpw, int cps, int pd) {
  return (pd - 1) * (tpw * cps * 2) + (pd - 2) * ((cps * mt * 4 + nw - 1) / nw);
}
constexpr Geo geometry(int mt, int nw, int tpw) {
  for (int cps = mt <= 4 ? 2 : 1; cps >= 1; --cps) {
    int pd = (160 * 1024 - 1024) / slot_bytes(mt, nw, tpw, cps);
    if (pd > 6) pd = 6;
    while (pd >= 3 && vm_outstanding(mt, nw, tpw, cps, pd) >= 64) --pd;
    if (pd >= 3) return Geo{cps, pd};
  }
  return Geo{1, 0};
}

// half h of a 16-byte weight piece -> the bf16 A fragment of k-step 2 j + h
__device__ __forceinline__ bf16x8_t widen(const u32x4_t& v, int h) {
  uint2 w;
  w.x = h ? v[2] : v[0];
  w.y = h ? v[3] : v[1];
  return __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16x8(w));
}

template <int MT, int NW, int TPW, bool BLOCK>
__global__ __launch_bounds__(64 * NW, 1) void wstream_fp8_gemm_kernel(W8Params p) {
  constexpr Geo G = geometry(MT, NW, TPW);
  constexpr int CPS = G.cps, PD = G.pd;                 // chunks per ring slot, ring depth
  constexpr int XCH = MT * 4;                           // 1 KiB pieces (4 rows x 256 B) of one chunk's activation image
  constexpr int XIMG = XCH * 1024;
  constexpr int XPIECES = CPS * XCH;
  constexpr int XP = (XPIECES + NW - 1) / NW;           // pieces each wave fetches per slot (surplus -> dummy slot)
  constexpr int WPC = TPW * CPS * 2;                    // weight DMA instructions per wave per slot
  constexpr int TILEB = CPS * kWTile;                   // one tile of one wave in a slot: [CPS][16 rows][128 B]
  constexpr int WWAVE = TPW * TILEB;
  constexpr int WCH = NW * WWAVE;
  constexpr int CH = WCH + CPS * XIMG;                  // ring slot: [weights of wave 0..NW) | activation images of its chunks]
  static_assert(PD >= 3 && PD * CH + 1024 <= 160 * 1024, "LDS ring does not fit");
  static_assert((PD - 1) * WPC + (PD - 2) * XP < 64, "vmcnt range");
  static_assert(WCH + 12288 < 65536, "ds_read offset field");
  __shared__ __attribute__((aligned(1024))) unsigned char ring[PD * CH + 1024];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  const int wtiles = p.ntiles / TPW;                    // tiles a wave index ranges over
  const int bx = blockIdx.x, split = blockIdx.y;
  const int tile = bx * NW + wid;
  const bool active = tile < wtiles;
  const int tl = active ? tile : wtiles - 1;            // idle waves of the last workgroup stream the last tile again
  const int nch = p.K / kKC;
  const int cb = static_cast<int>(static_cast<int64_t>(split) * nch / p.splits);
  const int ce = static_cast<int>(static_cast<int64_t>(split + 1) * nch / p.splits);
  const int n = ce - cb;                                // chunks of this K range
  const int ns = (n + CPS - 1) / CPS;                   // ring slots of this K range (the last one may be half full)

  // ---- DMA roles.  Weights: an instruction moves 8 rows x 128 B; the lane at (row q8, position p8) of the LDS image
  // fetches piece p8 ^ (row >> 1) of its row.  Activations: 1 KiB = 4 rows x 16 pieces, piece s16 ^ row (bf16 kernel).
  const int q8 = lane >> 3, p8 = lane & 7;
  const unsigned char* wsrc[TPW][2];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = 8 * j + q8;
      const int64_t wrow = (tl + static_cast<int64_t>(t) * wtiles) * 16 + row;
      wsrc[t][j] = p.w + wrow * p.w_stride + ((p8 ^ (row >> 1)) & 7) * 16 + static_cast<int64_t>(cb) * kKC;
    }
  const int q4 = lane >> 4, s16 = lane & 15;
  const uint16_t* xsrc[XP];                             // piece wid + NW i of the slot: chunk piece / XCH, rows 4 (piece % XCH) ..
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = wid + NW * i;
    const bool real = piece < XPIECES;
    const int ch = real ? piece / XCH : 0;
    const int row = real ? 4 * (piece - ch * XCH) + q4 : 0;
    const int srow = row < p.M ? row : p.M - 1;
    xsrc[i] = p.x + static_cast<int64_t>(srow) * p.x_stride + ((s16 ^ row) & 15) * 8 + static_cast<int64_t>(cb + ch) * p.x_cstride;
  }
  lds_bytes_t ring3 = (lds_bytes_t)(ring);
  // Slot c of the K range lives in ring slot c % PD.  As in the bf16 kernel a wave's weight tiles of a slot are private to
  // it (copied to registers at the top of compute(), refilled at once with slot c + PD) and the activation images are
  // shared (slot c + PD - 1's go in after the barrier that retires slot c - 1); behind the end of the K range, and for
  // the second chunk of a half slot, a dummy DMA (L2-resident source, the 1 KiB landing zone) keeps the in-order vmcnt
  // arithmetic the same in every iteration.
  const uint16_t* dummy_src = p.x + s16 * 8;
  lds_ptr_t dummy_dst = (lds_ptr_t)(ring3 + PD * CH);
  // without split-K the workgroups walk the K range from staggered starting slots, wrapping around (see wstream_gemm.hip)
  const int rot = p.splits == 1 && ns > 1 ? static_cast<int>((static_cast<int64_t>(bx) * ns) / gridDim.x) : 0;
  auto slot_of = [&](int c_rel) { return c_rel + rot < ns ? c_rel + rot : c_rel + rot - ns; };
  auto issue_w = [&](int c_rel, int slot) {
    const int sr = c_rel < ns ? slot_of(c_rel) : 0;
    const int nin = c_rel < ns ? (n - sr * CPS < CPS ? n - sr * CPS : CPS) : 0;
    const int base = slot * CH + wid * WWAVE;
#pragma unroll
    for (int ch = 0; ch < CPS; ++ch) {
      if (ch < nin) {
        const int koff = (sr * CPS + ch) * kKC;
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
          for (int j = 0; j < 2; ++j) dma16<2>(wsrc[t][j] + koff, (lds_ptr_t)(ring3 + base + t * TILEB + ch * kWTile + j * 1024));
      } else {
#pragma unroll
        for (int i = 0; i < TPW * 2; ++i) dma16<0>(dummy_src, dummy_dst);
      }
    }
  };
  auto issue_x = [&](int c_rel, int slot) {
    const int sr = c_rel < ns ? slot_of(c_rel) : 0;
    const int nin = c_rel < ns ? (n - sr * CPS < CPS ? n - sr * CPS : CPS) : 0;
    const int64_t koff = static_cast<int64_t>(sr) * CPS * p.x_cstride;
    const int base = slot * CH;
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int piece = wid + NW * i;
      if (piece < nin * XCH) dma16<0>(xsrc[i] + koff, (lds_ptr_t)(ring3 + base + WCH + piece * 1024));
      else dma16<0>(dummy_src, dummy_dst);
    }
  };

  // ---- fragment read addresses (bytes).  Weights: piece j * 4 + g of row r16; activations: the same k order
  const uint32_t ring_addr = (uint32_t)(uintptr_t)(ring3);
  uint32_t afoff[2], foff[kKSteps];
#pragma unroll
  for (int j = 0; j < 2; ++j) afoff[j] = r16 * kKC + (((j * 4 + g) ^ (r16 >> 1)) & 7) * 16;
#pragma unroll
  for (int kk = 0; kk < kKSteps; ++kk) foff[kk] = r16 * 256 + (((((kk >> 1) * 4 + g) * 2 + (kk & 1)) ^ r16) & 15) * 16;

  f32x4_t acc[TPW][MT];
  f32x4_t cacc[BLOCK ? TPW : 1][BLOCK ? MT : 1];        // block scales: the accumulator of the chunk in hand
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // Block scales travel like the weights: the scales of slot c are loaded (ordinary loads from a wave-uniform address) right
  // behind the weight DMAs of slot c, PD slots ahead, into a register queue that moves up one place per slot.  Vector memory
  // returns in order, so a scale has landed when its slot's weights have -- a load issued where it is used would wait for the
  // whole ring.  The extra loads only make the hand-written vmcnt below stricter than it needs to be.
  const float* bscale[TPW];                             // this wave's rows of the scale matrix, at chunk cb
  float sq[BLOCK ? PD : 1][CPS][TPW];
  auto load_scales = [&](int c_rel, float (&dst)[CPS][TPW]) {
    const int sr = c_rel < ns ? slot_of(c_rel) : 0;
#pragma unroll
    for (int ch = 0; ch < CPS; ++ch)
#pragma unroll
      for (int t = 0; t < TPW; ++t) dst[ch][t] = bscale[t][sr * CPS + ch < n ? sr * CPS + ch : n - 1];
  };
  if constexpr (BLOCK) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) bscale[t] = p.scale + ((tl + static_cast<int64_t>(t) * wtiles) >> 3) * p.scale_stride + cb;
  }

  // activation fragments by "stage" as in the bf16 kernel: up to 64 rows a stage is a whole k-step, beyond it half of one
  constexpr bool WIDE = MT > 4;
  constexpr int H = WIDE ? MT / 2 : MT;                // B tiles per stage
  constexpr int NST = WIDE ? 2 * kKSteps : kKSteps;    // stages per chunk
  auto read_stage = [&](uint32_t img_addr, int st, u32x4_t (&b)[H]) {
    const int kk = WIDE ? st >> 1 : st;
    const int half = WIDE ? st & 1 : 0;
    const uint32_t bd = img_addr + foff[kk] + half * (H * 4096);
    b[0] = lds_rd<WCH>(bd);
    if constexpr (H > 1) b[1] = lds_rd<WCH + 4096>(bd);
    if constexpr (H > 2) b[2] = lds_rd<WCH + 8192>(bd);
    if constexpr (H > 3) b[3] = lds_rd<WCH + 12288>(bd);
  };
  // the products of one chunk: a[j][t] = the wave's 16-byte weight pieces; b0 = stage 0, already on its way
  auto chunk = [&](uint32_t img_addr, const u32x4_t (&a)[2][TPW], u32x4_t (&b)[2][H], const float (&bs)[TPW]) {
    if constexpr (BLOCK) {
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) cacc[t][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    bf16x8_t aw[2][TPW];                                // widened A fragments, by k-step parity
#pragma unroll
    for (int t = 0; t < TPW; ++t) aw[0][t] = widen(a[0][t], 0);
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      const int kk = WIDE ? st >> 1 : st;
      const int half = WIDE ? st & 1 : 0;
      const int bc = st & 1;
      if (st + 1 < NST) read_stage(img_addr, st + 1, b[bc ^ 1]);
      if ((!WIDE || half == 1) && kk + 1 < kKSteps) {   // the next k-step's weights widen under this one's MFMAs
#pragma unroll
        for (int t = 0; t < TPW; ++t) aw[(kk + 1) & 1][t] = widen(a[(kk + 1) >> 1][t], (kk + 1) & 1);
      }
      if (st + 1 < NST) wait_lgkm<H>();
      else wait_lgkm<0>();
#pragma unroll
      for (int j = 0; j < H; ++j) pin(b[bc][j]);
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int j = 0; j < H; ++j) {
          f32x4_t& d = BLOCK ? cacc[BLOCK ? t : 0][BLOCK ? half * H + j : 0] : acc[t][half * H + j];
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[kk & 1][t], __builtin_bit_cast(bf16x8_t, b[bc][j]), d, 0, 0, 0);
        }
    }
    if constexpr (BLOCK) {
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] += cacc[t][mt] * bs[t];
    }
  };
  auto compute = [&](int slot, int c) {
    const uint32_t slot_addr = ring_addr + slot * CH;
    const int nin = n - slot_of(c) * CPS < CPS ? n - slot_of(c) * CPS : CPS;
    u32x4_t a[CPS][2][TPW], b[2][H];
#pragma unroll
    for (int ch = 0; ch < CPS; ++ch)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < TPW; ++t) a[ch][j][t] = lds_rd<0>(slot_addr + wid * WWAVE + t * TILEB + ch * kWTile + afoff[j]);
    read_stage(slot_addr, 0, b[0]);
    wait_lgkm<H>();                                      // LDS returns in order: the weight pieces are in
#pragma unroll
    for (int ch = 0; ch < CPS; ++ch)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < TPW; ++t) pin(a[ch][j][t]);
    issue_w(c + PD, slot);                               // the tiles just copied out are free: refill them now
    float snew[CPS][TPW];
    if constexpr (BLOCK) load_scales(c + PD, snew);
    chunk(slot_addr, a[0], b, sq[0][0]);
    if constexpr (CPS > 1) {
      if (nin > 1) {                                     // (a half slot: its second chunk was never fetched)
        read_stage(slot_addr + XIMG, 0, b[0]);
        chunk(slot_addr + XIMG, a[CPS - 1], b, sq[0][CPS - 1]);
      }
    }
    if constexpr (BLOCK) {
#pragma unroll
      for (int u = 0; u < PD; ++u)
#pragma unroll
        for (int ch = 0; ch < CPS; ++ch)
#pragma unroll
          for (int t = 0; t < TPW; ++t) sq[u][ch][t] = u + 1 < PD ? sq[u + 1 < PD ? u + 1 : u][ch][t] : snew[ch][t];
    }
  };

  // ---- pipeline: weights PD slots ahead, activations PD - 1, one barrier per slot ----
#pragma unroll
  for (int u = 0; u < PD - 1; ++u) {
    issue_w(u, u);
    if constexpr (BLOCK) load_scales(u, sq[u]);
    issue_x(u, u);
  }
  issue_w(PD - 1, PD - 1);
  if constexpr (BLOCK) load_scales(PD - 1, sq[PD - 1]);
  int slot = 0, nslot = PD - 1;                          // ring slot of slot c, of slot c - 1 (= c + PD - 1)
  for (int c = 0; c < ns; ++c) {
    // slot c has landed once only the DMAs issued after its activations are outstanding:
    // weights of c+1 .. c+PD-1 and activations of c+1 .. c+PD-2
    wait_vm<(PD - 1) * WPC + (PD - 2) * XP>();
    __builtin_amdgcn_s_barrier();                        // everyone's pieces of slot c are visible,
                                                         // everyone is done reading the activations of slot c - 1
    issue_x(c + PD - 1, nslot);
    compute(slot, c);
    slot = slot + 1 == PD ? 0 : slot + 1;
    nslot = nslot + 1 == PD ? 0 : nslot + 1;
  }

  if (!active) return;
  // lane holds C[m = 16 mt + r16][n = 16 tile + 4 g + r].  The scale first: nothing sees an unscaled accumulator.
  const int n0 = tile * 16 + g * 4;
  if constexpr (!BLOCK) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      f32x4_t sc;
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[r] = p.scale[p.scale_mode == 1 ? n0 + t * wtiles * 16 + r : 0];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[t][mt] *= sc;
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int64_t m = mt * 16 + r16;                     // output row
    if (m >= p.M) continue;
    auto put = [&](float (&o)[4], int nn) {
      uint2 w2;
      w2.x = pack_bf2(o[0], o[1]);
      w2.y = pack_bf2(o[2], o[3]);
      *reinterpret_cast<uint2*>(p.y + blocked_off(m, nn, p.y_stride, p.y_cstride)) = w2;
    };
    if (TPW == 2 && p.pair_silu) {
      // linear -> bf16, silu -> bf16, product -> bf16 (activation.py:141-143)
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gb = rbf(acc[0][mt][r]);
        const float sl = rbf(gb / (1.0f + expf(-gb)));
        o[r] = sl * rbf(acc[TPW - 1][mt][r]);
      }
      put(o, n0);
      continue;
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {                      // tile t of the wave is output tile `tile + t * wtiles`
      const int nn = n0 + t * wtiles * 16;
      if (p.part) {
        const int64_t e = (static_cast<int64_t>(split) * p.M + m) * p.N + nn;
        if (!p.plain_part) {  // write-through (sc1), as the bf16 kernel: the partials leave the L2 while the stream runs
          const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(p.part, 0, static_cast<int>(static_cast<int64_t>(p.splits) * p.M * p.N * 4), 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[t][mt]), r, static_cast<int>(e * 4), 0, 16);
        } else {
          *reinterpret_cast<f32x4_t*>(p.part + e) = acc[t][mt];
        }
        continue;
      }
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = acc[t][mt][r] + (p.bias ? bf2f(p.bias[nn + r]) : 0.f);
      put(o, nn);
    }
  }
}

template <int MT, int NW, int TPW>
int launch_main(const W8Params& p, hipStream_t st) {
  if constexpr (geometry(MT, NW, TPW).pd >= 3) {
    dim3 grid((p.ntiles / TPW + NW - 1) / NW, p.splits);
    if (p.scale_mode == 2) hipLaunchKernelGGL((wstream_fp8_gemm_kernel<MT, NW, TPW, true>), grid, dim3(64 * NW), 0, st, p);
    else hipLaunchKernelGGL((wstream_fp8_gemm_kernel<MT, NW, TPW, false>), grid, dim3(64 * NW), 0, st, p);
    return 0;
  } else {
    return -1;
  }
}

template <int MT>
int launch_nw(const W8Params& p, int nw, bool two_tiles, hipStream_t st) {
  if (two_tiles) {
    switch (nw) {
      case 2: return launch_main<MT, 2, 2>(p, st);
      case 3: return launch_main<MT, 3, 2>(p, st);
      case 4: return launch_main<MT, 4, 2>(p, st);
      default: return -1;
    }
  }
  switch (nw) {
    case 4: return launch_main<MT, 4, 1>(p, st);
    case 5: return launch_main<MT, 5, 1>(p, st);
    case 6: return launch_main<MT, 6, 1>(p, st);
    case 7: return launch_main<MT, 7, 1>(p, st);
    case 8: return launch_main<MT, 8, 1>(p, st);
    default: return -1;
  }
}

// shared by the two entry points: validates the GEMM part and launches the main kernel
int fp8_launch_main(const char* who, const void* x, const void* w, const void* bias, void* y, int64_t M, int64_t N, int64_t K,
                    int64_t x_row_stride, int64_t x_chunk_stride, int64_t w_row_stride, const float* w_scale, int scale_mode,
                    int64_t scale_row_stride, int64_t y_row_stride, int64_t y_chunk_stride, bool fused_silu, int tiles_per_wave,
                    bool to_partials, int waves_per_group, int num_k_splits, void* ws_partials, hipStream_t st) {
  SGL_CHECK_ARG(M >= 1 && M <= 128, "%s: M=%lld rows (supported: 1..128)", who, (long long)M);
  SGL_CHECK_ARG(N > 0 && N % 16 == 0 && K >= kKC && K % kKC == 0,
                "%s: need N %% 16 == 0 and K %% %d == 0 (got N=%lld K=%lld)", who, kKC, (long long)N, (long long)K);
  SGL_CHECK_ARG(x_row_stride % 8 == 0 && w_row_stride % 16 == 0 && w_row_stride >= K && y_row_stride % 4 == 0,
                "%s: row strides must keep 16-byte (x, w: in bytes) / 8-byte (y) alignment", who);
  SGL_CHECK_ARG(w_scale && scale_mode >= 0 && scale_mode <= 2, "%s: fp8 weights need w_scale and scale_mode 0 (tensor), 1 (channel) or 2 (128 x 128 blocks)", who);
  SGL_CHECK_ARG(scale_mode != 2 || scale_row_stride >= K / kKC, "%s: block scales are [ceil(N / 128), K / 128] (row stride %lld < %lld)", who,
                (long long)scale_row_stride, (long long)(K / kKC));
  SGL_CHECK_ARG(tiles_per_wave == 0 || tiles_per_wave == 1 || tiles_per_wave == 2, "%s: tiles_per_wave must be 1 or 2 (0: the default of the form)", who);
  const bool two_tiles = fused_silu || tiles_per_wave == 2;
  SGL_CHECK_ARG(!two_tiles || N % 32 == 0, "%s: two tiles per wave need N %% 32 == 0", who);
  SGL_CHECK_ARG(two_tiles ? (waves_per_group >= 2 && waves_per_group <= 4) : (waves_per_group >= 4 && waves_per_group <= 8),
                "%s: waves_per_group must be 4..8 (2..4 with two tiles per wave), got %d", who, waves_per_group);
  SGL_CHECK_ARG(num_k_splits >= 1 && num_k_splits <= K / kKC, "%s: bad split count %d", who, num_k_splits);
  SGL_CHECK_ARG(!to_partials || ws_partials, "%s: needs the fp32 partials workspace", who);
  SGL_CHECK_ARG(x_chunk_stride % 8 == 0 && y_chunk_stride % 4 == 0 && x_chunk_stride >= 0 && y_chunk_stride >= 0,
                "%s: chunk strides must keep 16-byte (x) / 8-byte (y) alignment", who);
  W8Params p{};
  p.x = static_cast<const uint16_t*>(x);
  p.w = static_cast<const unsigned char*>(w);
  p.bias = to_partials ? nullptr : static_cast<const uint16_t*>(bias);
  p.y = static_cast<uint16_t*>(y);
  p.part = to_partials ? static_cast<float*>(ws_partials) : nullptr;
  p.scale = w_scale; p.scale_mode = scale_mode; p.scale_stride = scale_row_stride;
  p.x_stride = x_row_stride; p.w_stride = w_row_stride; p.y_stride = y_row_stride;
  p.x_cstride = x_chunk_stride ? x_chunk_stride : kKC;
  p.y_cstride = y_chunk_stride ? y_chunk_stride : 128;
  p.M = static_cast<int>(M); p.N = static_cast<int>(N); p.K = static_cast<int>(K);
  p.splits = num_k_splits; p.ntiles = static_cast<int>(N / 16);
  p.pair_silu = fused_silu ? 1 : 0;
  p.plain_part = static_cast<int64_t>(num_k_splits) * M * N * 4 >= (int64_t{1} << 31) ? 1 : 0;
  int rc;
  switch (static_cast<int>((M + 15) / 16)) {
    case 1: rc = launch_nw<1>(p, waves_per_group, two_tiles, st); break;
    case 2: rc = launch_nw<2>(p, waves_per_group, two_tiles, st); break;
    case 3: rc = launch_nw<3>(p, waves_per_group, two_tiles, st); break;
    case 4: rc = launch_nw<4>(p, waves_per_group, two_tiles, st); break;
    case 5: case 6: rc = launch_nw<6>(p, waves_per_group, two_tiles, st); break;
    default: rc = launch_nw<8>(p, waves_per_group, two_tiles, st); break;
  }
  SGL_CHECK_ARG(rc == 0, "%s: unsupported configuration", who);
  return 0;
}

}  // namespace

extern "C" {

int sgl_amd_wstream_gemm_fp8(const void* x, const void* w, const void* bias, void* y, int64_t M, int64_t N, int64_t K,
                             int64_t x_row_stride, int64_t x_chunk_stride, int64_t w_row_stride, int64_t y_row_stride,
                             int64_t y_chunk_stride, int epilogue, void* residual, int64_t residual_row_stride,
                             const void* norm_weight, float eps, int waves_per_group, int tiles_per_wave, int num_k_splits,
                             void* ws_partials, void* stream, const float* w_scale, int scale_mode, int64_t scale_row_stride) {
  SGL_CLEAR_STALE_ERROR();
  if (M == 0) return 0;
  SGL_CHECK_ARG(epilogue >= 0 && epilogue <= 2, "wstream_gemm_fp8: epilogue must be 0 (bias), 1 (silu_and_mul) or 2 (add_rmsnorm)");
  SGL_CHECK_ARG(epilogue != 1 || N % 8 == 0, "wstream_gemm_fp8: silu_and_mul needs N %% 8 == 0");
  SGL_CHECK_ARG(epilogue != 1 || !bias, "wstream_gemm_fp8: the silu_and_mul epilogue takes no bias");
  SGL_CHECK_ARG(!(epilogue == 1 && num_k_splits == 1 && tiles_per_wave == 1),
                "wstream_gemm_fp8: the interleaved one-tile silu form (tiles_per_wave = 1 in one pass, pair_silu == 2 of the bf16 kernel) is not built "
                "for fp8 weights");
  SGL_CHECK_ARG(epilogue != 2 || (residual && norm_weight && N <= wstream_combine_norm_max_n() && residual_row_stride % 4 == 0),
                "wstream_gemm_fp8: add_rmsnorm needs residual, norm_weight and N <= %d", wstream_combine_norm_max_n());
  SGL_CHECK_ARG(y_chunk_stride == 0 || (epilogue == 1 ? N % 256 == 0 : N % 128 == 0),
                "wstream_gemm_fp8: a chunk-major y needs whole 128-column blocks");
  // silu(gate) * up in the GEMM's own epilogue: two tiles per wave (a gate tile and its up tile)
  const bool fused_silu = epilogue == 1 && num_k_splits == 1 && N % 32 == 0;
  const bool combine = !fused_silu && (num_k_splits > 1 || epilogue != 0);
  hipStream_t st = as_stream(stream);
  if (int rc = fp8_launch_main("wstream_gemm_fp8", x, w, bias, y, M, N, K, x_row_stride, x_chunk_stride, w_row_stride, w_scale, scale_mode,
                               scale_row_stride, y_row_stride, y_chunk_stride, fused_silu, tiles_per_wave, combine, waves_per_group,
                               num_k_splits, ws_partials, st))
    return rc;
  if (combine && epilogue != 2) {
    launch_wstream_combine(static_cast<const float*>(ws_partials), static_cast<const uint16_t*>(bias), static_cast<uint16_t*>(y),
                           y_row_stride, y_chunk_stride ? y_chunk_stride : 128, static_cast<int>(M), static_cast<int>(N),
                           num_k_splits, epilogue == 1, st);
  } else if (combine) {
    launch_wstream_combine_norm(static_cast<const float*>(ws_partials), static_cast<const uint16_t*>(bias), static_cast<uint16_t*>(y),
                                static_cast<uint16_t*>(residual), static_cast<const uint16_t*>(norm_weight), y_row_stride,
                                y_chunk_stride ? y_chunk_stride : 128, residual_row_stride, static_cast<int>(M), static_cast<int>(N),
                                num_k_splits, eps, st);
  }
  SGL_CHECK_LAUNCH("wstream_gemm_fp8");
  return 0;
}

int sgl_amd_wstream_qkv_rope_fp8(const void* x, const void* w_qkv, const void* bias, void* q_out, int64_t M, int64_t K,
                                 int num_q_heads, int num_kv_heads, int head_dim, int64_t x_row_stride, int64_t x_chunk_stride,
                                 int64_t w_row_stride, int64_t q_row_stride, const int64_t* positions, const void* cos_sin_cache,
                                 int cache_is_f32, int64_t rotary_dim, void* k_cache, void* v_cache, const int64_t* cache_loc,
                                 int64_t cache_row_stride, int kv_fp8, float k_scale, float v_scale, int page_size,
                                 int kv_layout_hnd, int waves_per_group, int tiles_per_wave, int num_k_splits, void* ws_partials,
                                 void* stream, const float* w_scale, int scale_mode, int64_t scale_row_stride) {
  SGL_CLEAR_STALE_ERROR();
  if (M == 0) return 0;
  struct Main {
    const void *x, *w;
    int64_t M, K, x_rs, x_cs, w_rs, scale_rs;
    const float* scale;
    int mode, nw, tpw, splits;
    void* ws;
  } ctx{x, w_qkv, M, K, x_row_stride, x_chunk_stride, w_row_stride, scale_row_stride, w_scale, scale_mode, waves_per_group,
        tiles_per_wave, num_k_splits, ws_partials};
  return wstream_qkv_rope_combine(
      "wstream_qkv_rope_fp8",
      [](void* c, int64_t N, hipStream_t st) {
        const Main& m = *static_cast<const Main*>(c);
        return fp8_launch_main("wstream_qkv_rope_fp8", m.x, m.w, nullptr, nullptr, m.M, N, m.K, m.x_rs, m.x_cs, m.w_rs, m.scale, m.mode,
                               m.scale_rs, 4, 0, false, m.tpw, true, m.nw, m.splits, m.ws, st);
      },
      &ctx, bias, q_out, M, num_q_heads, num_kv_heads, head_dim, q_row_stride, positions, cos_sin_cache, cache_is_f32, rotary_dim,
      k_cache, v_cache, cache_loc, cache_row_stride, kv_fp8, k_scale, v_scale, page_size, kv_layout_hnd, num_k_splits, ws_partials,
      as_stream(stream));
}

}  // extern "C"
