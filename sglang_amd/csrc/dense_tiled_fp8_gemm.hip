// Dense MFMA tile GEMM over fp8 (OCP e4m3) weights on gfx950, weight-only quantisation ("W8A16"), any row count:
//
//   y[m, n] = bf16( (sum_k x[m, k] f(w8[n, k])) s[n] + bias[n] )                        per-tensor / per-channel scales
//   y[m, n] = bf16(  sum_c s[n / 128, c] (sum_{k in chunk c} x[m, k] f(w8[n, k])) + bias[n] )      128 x 128 block scales
//
// The contract of wstream_fp8_gemm.hip (x bf16, w8 e4m3 [N, K] with 16-byte aligned rows, f the exact e4m3 -> bf16 widening,
// bf16 MFMA, fp32 accumulation, fp32 scales that meet the accumulator before a split-K partial is written and before any
// epilogue) for the rows that kernel does not take: prefill, chunked / mixed prefill, decode batches beyond 128 rows.  No
// activation quantisation, no fp8 / scaled MFMA: prefill and decode stay the same function of the weights.
//
// Replaces, for prefill-sized M over fp8 checkpoints, the reference's fp8 linear method (python/sglang of the sglang tree:
// srt/layers/quantization/fp8.py Fp8LinearMethod.apply -> fp8_utils.py apply_fp8_linear) and -- `silu_and_mul` epilogue -- the
// pair gate_up_proj + srt/layers/activation.py:130-143 SiluAndMul.forward_native.  Oracle: fp64 (x . f(w8)^T) s + bias.
//
//   work split   a workgroup (8 waves: 2 along the weight rows x 4 along the activation rows) owns BM = 256 activation rows
//                x BN weight rows and walks one contiguous K range of whole 128-element chunks in 64-wide steps.  The grid
//                covers ceil(M / 256) row blocks x column strips x K splits; rows past M are clamped on load and dropped on
//                store, weight rows past N likewise.
//   tile forms   an e4m3 W stage is BN x 64 B next to the activation tile's 256 x 128 B = 32 KiB, so the LDS the bf16 kernel
//                spends on 128 weight rows (16 KiB) holds 256 of them.  Both ways of spending it are built:
//                  wide   BN = 256, THREE stages of 16 + 32 = 48 KiB (144 KiB).  A wave owns 128 x 64 outputs = 8 x 4 tiles:
//                         per 64-wide step 8 (W) + 8 (X) ds_read_b128 feed 64 MFMAs -- twice the products per LDS byte of
//                         the 256 x 128 tile, which is what a compute-bound prefill needs; this is the default form.
//                  narrow BN = 128, FOUR stages of 8 + 32 = 40 KiB (160 KiB).  4 x 4 tiles per wave, 12 reads per 32 MFMAs.
//                         Twice the workgroups for the shapes that do not fill the chip, and the form of the block scales:
//                         their second accumulator set (below) does not fit next to 128 accumulator registers.
//   launch order one-dimensional grid; the hardware deals workgroups to the 8 XCDs round robin by linear id (workgroup i runs
//                on XCD x = i % 8, the mapping dense_tiled_gemm.hip relies on) and an XCD keeps 32 of them resident (32 CUs,
//                one workgroup each).  A unit u = (split, strip) = (u / strips, u % strips) belongs to XCD u % 8, so every row
//                block of a unit runs on one XCD.  On XCD x, slot j = i / 8 walks its local units v = u / 8 in groups of 4
//                and, inside a group, the row blocks in groups of 8:
//                    vg = j / (4 RB);  r = j % (4 RB);  nv = min(4, U8 - 4 vg);  rg = r / (8 nv);  r2 = r - 8 nv rg;
//                    nb = min(8, RB - 8 rg);  v = 4 vg + r2 / nb;  rb = 8 rg + r2 % nb           (U8 = ceil(U / 8), RB row blocks)
//                so the 32 workgroups resident together are (up to) 4 units x 8 row blocks: a weight strip is read from HBM by
//                one of them and from that XCD's L2 by the other 7, an activation block by one and from L2 by the other 3,
//                however many row blocks there are.  HBM then sees a byte of W once per group of 8 row blocks (once in all
//                while the 4 strips of a group, <= 1 KiB x K, stay in the 4 MiB L2 across the row-block walk) and a byte of
//                X once per XCD and group of 4 local units: U / 4 times instead of U.
//   data path    both operands HBM / L2 -> LDS by LDS-DMA (global_load_lds, 16 bytes per lane, 1 KiB per wave instruction:
//                8 activation rows x 128 B or 16 weight rows x 64 B), stages as above: while step t multiplies, the tiles of
//                steps t + 1 .. t + stages - 1 are in flight.  One barrier per K step: it publishes tile t and retires the
//                reads of tile t - 1, whose stage the DMA of tile t + stages - 1 then refills.  The e4m3 tile stays bytes in LDS.
//   swizzle      X: row r at r * 128, 16-byte piece pc in slot pc ^ (r & 7) (the bf16 kernel's).  W: row r at r * 64, piece
//                pc in slot pc ^ ((r >> 2) & 3): the 16 rows of a ds_read_b128 fragment read sit 64 B apart, 4 r mod 16 takes
//                4 values (r & 3), and the four rows that share one differ in r >> 2, so the 16 lanes cover all 16 16-byte
//                bank groups of the 256-byte bank line.  Both are applied on the global side of the DMA (lane -> piece).
//   fragments    one ds_read_b128 of a weight row is 16 K elements = two 16x16x32 k-steps: lane group g reads piece g and in
//                k-step s uses bytes 8 s .. 8 s + 7 = K elements 16 g + 8 s ..; the activation side reads its bf16 pieces in
//                the same permuted order (piece 2 g + s).  Widening: fp8x8_to_bf16x8 of kv_format.hpp (v_cvt_pk_f32_fp8 +
//                v_cvt_pk_bf16_f32); k-step 1 is widened in program order ahead of the MFMAs of k-step 0, so the VALU work
//                is scheduled under the matrix pipe.
//   products     v_mfma_f32_16x16x32_bf16 on the transposed problem (C^T = W . x^T): a lane ends up with 4 consecutive
//                output columns of one row -> 8-byte bf16 stores, 16-byte fp32 partial stores.
//   scales       tensor / channel: one multiply as the accumulator leaves the loop.  Block (template flag, narrow form): a
//                128-wide chunk is accumulated on its own and folded into the running accumulator with one FMA per element
//                at the chunk boundary, by the scale of the 16-row tile's block row (a tile never straddles a block row, so
//                gate and up tiles of the silu form simply carry their own row).  The scales of chunk c + 1 are loaded
//                at the top of chunk c: scalar loads from wave-uniform addresses, outside the vector-memory counter that the
//                hand-written vmcnt keeps for the DMAs.
//   split-K      splits > 1: scaled fp32 partials [splits, M, N] into the caller's workspace, summed in split order by the
//                combine kernels of wstream_gemm.hip (wstream_combine.hpp).  No atomics: a fixed function of (shape, BN, splits).
//   epilogues    none: bf16(acc s + bias).  silu_and_mul with one split: the weight rows of a wave's slice are [gate | up]
//                halves of the same output columns (wide: 64 | 64, narrow: 32 | 32), so a lane holds gate and up of the
//                same element and applies linear -> bf16, silu -> bf16, product -> bf16 (activation.py:141-143) in
//                registers; the [M, 2I] intermediate is never written.  More splits: plain partials + the combine-silu kernel.
//
//   registers    wide: 128 accumulators + 32 raw weight + 16 widened (four tiles of one k-step) + 2 x 16 activation fragments
//                = 208 + addresses; narrow: 64 (+ 64 chunk accumulators with block scales) + 16 + 16 + 2 x 16.  All <= 256:
//                8 waves, two per SIMD, one workgroup per CU of the 160 KiB LDS.
#include <type_traits>

#include "common.hpp"
#include "kv_format.hpp"
#include "sglang_amd.h"
#include "wstream_combine.hpp"

using namespace sgl_amd;

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) unsigned char* lds_bytes_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;
typedef const __attribute__((address_space(4))) float* cst_f32_t;

constexpr int kBM = 256, kBK = 64, kKC = 128;         // rows per block, K step, K chunk (the unit split-K deals out)
constexpr int kXBytes = kBM * kBK * 2;                // 32 KiB: the activation tile of a stage
constexpr int kThreads = 512;
constexpr int kUnitGroup = 4, kRowGroup = 8;          // local units x row blocks resident together on an XCD
constexpr int kMaxCombineRows = 65535;                // the combine kernels index rows by grid y

struct Dense8Params {
  const uint16_t* x;            // [M, K] bf16
  const unsigned char* w;       // [N, K] e4m3 (silu: N = 2 I, gate rows then up rows)
  const uint16_t* bias;         // optional [N]; null when writing partials
  uint16_t* y;                  // [M, N]   ([M, I] fused silu)
  float* part;                  // [splits, M, N] when splits > 1, else null
  const float* scale;           // mode 0: [1], 1: [N], 2: [ceil(N / 128), scale_stride >= K / 128]
  int64_t x_stride, w_stride /* bytes */, y_stride, scale_stride;
  int M, N, K;
  int splits, nstrips, units;   // units = splits * nstrips
  int row_blocks, units8;       // ceil(M / 256), ceil(units / 8)
  int scale_mode;
  int fuse_silu;                // one split only: N/2 output columns
};

__device__ __forceinline__ void dma16(const void* src, lds_ptr_t dst) {
  __builtin_amdgcn_global_load_lds((glb_ptr_t)(src), dst, 16, 0, 0);
}
template <int OFF>
__device__ __forceinline__ u32x4_t lds_rd(uint32_t addr) {
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N>
__device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N)); }
__device__ __forceinline__ void pin(u32x4_t& v) { asm volatile("" : "+v"(v)); }

// half s of a 16-byte weight piece -> the bf16 A fragment of k-step s
__device__ __forceinline__ bf16x8_t widen(const u32x4_t& v, int s) {
  uint2 w;
  w.x = s ? v[2] : v[0];
  w.y = s ? v[3] : v[1];
  return __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16x8(w));
}

template <int BN, bool BLOCK>
__global__ __launch_bounds__(kThreads, 1) void dense_tiled_fp8_gemm_kernel(Dense8Params p) {
  static_assert(BN == 128 || BN == 256, "narrow (128) and wide (256) forms");
  static_assert(!BLOCK || BN == 128, "block scales: the narrow form");
  constexpr int kStages = BN == 256 ? 3 : 4;
  constexpr int kWI = BN / 128;                        // W-tile DMA instructions per wave and step (the X tile: 4)
  constexpr int kPerStep = 4 + kWI;                    // LDS-DMA instructions a wave has in flight per tile
  constexpr int kWavesX = 4;                           // waves: 2 (weight rows) x 4 (activation rows)
  constexpr int kSL = BN / 2;                          // weight rows of a wave's slice
  constexpr int kWT = kSL / 16, kXT = 4;               // 16-row weight / activation tiles per wave
  constexpr int kWBytes = BN * kBK;
  constexpr int kStage = kWBytes + kXBytes;            // [W tile | X tile]
  static_assert(kStages * kStage <= 160 * 1024 && (kStages - 2) * kPerStep < 64, "LDS / vmcnt range");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[kStages * kStage];

  // ---- workgroup -> (unit, row block): see "launch order" in the header ----
  const int id = blockIdx.x;
  const int xcd = id & 7, slot = id >> 3;
  const int per_vg = kUnitGroup * p.row_blocks;
  const int vg = slot / per_vg, r = slot - vg * per_vg;
  const int nv = min(kUnitGroup, p.units8 - vg * kUnitGroup);
  const int rg = r / (kRowGroup * nv), r2 = r - rg * (kRowGroup * nv);
  const int nb = min(kRowGroup, p.row_blocks - rg * kRowGroup);
  const int unit = (vg * kUnitGroup + r2 / nb) * 8 + xcd;
  const int rb = rg * kRowGroup + r2 % nb;
  if (unit >= p.units) return;                         // padding of the last 8 units (whole workgroup, ahead of any barrier)
  const int split = unit / p.nstrips, strip = unit - split * p.nstrips;
  const int nch = p.K / kKC;
  const int c0 = static_cast<int>(static_cast<int64_t>(split) * nch / p.splits);
  const int c1 = static_cast<int>(static_cast<int64_t>(split + 1) * nch / p.splits);
  const int k0 = c0 * kKC, nk = (c1 - c0) * (kKC / kBK);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / kWavesX, wc = wid % kWavesX;    // this wave: weight rows kSL wr .., activation rows 64 wc ..
  const int r16 = lane & 15, g = lane >> 4;
  const int half = p.N >> 1;

  // ---- DMA roles.  X: instruction j of a tile covers its rows 8j .. 8j+7; lane i -> (row 8j + i/8, LDS slot i%8) and fetches the
  // 16-byte piece (slot ^ (row & 7)) of that row; wave w issues j = 4w .. 4w+3.  W: instruction j covers rows 16j .. 16j+15; lane i ->
  // (row 16j + i/4, slot i%4), piece slot ^ ((row >> 2) & 3); wave w issues j = kWI w ..  Every source is a wave-uniform base
  // (scalar registers; the K walk advances it) plus a 32-bit lane offset: twelve 64-bit lane pointers do not fit next to the
  // wide form's accumulators.
  const int rows_here = min(kBM, p.M - rb * kBM) - 1;  // last valid row of this block
  const unsigned char* xbase = reinterpret_cast<const unsigned char*>(p.x + static_cast<int64_t>(rb) * kBM * p.x_stride + k0);
  const unsigned char* wbase[kWI];
  uint32_t xoff[4], woff[kWI];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = (wid * 4 + u) * 8 + (lane >> 3);   // 0..255
    const int piece = (lane & 7) ^ (row & 7);
    xoff[u] = static_cast<uint32_t>(min(row, rows_here)) * static_cast<uint32_t>(p.x_stride * 2) + piece * 16;
  }
#pragma unroll
  for (int u = 0; u < kWI; ++u) {
    const int first = (wid * kWI + u) * 16, lr = lane >> 2;   // tile rows first .. first + 15: one 16-row weight tile
    const int piece = (lane & 3) ^ (lr >> 2);
    int col0, lim, add = 0;
    if (p.fuse_silu) {
      // tile rows: per kSL-row wave slice [gate | up] halves of output columns strip * BN/2 + slice * kSL/2 + c
      const int slice = first / kSL, in = first % kSL;
      col0 = strip * (BN / 2) + slice * (kSL / 2) + (in % (kSL / 2));
      lim = half - 1;
      add = in < kSL / 2 ? 0 : half;
    } else {
      col0 = strip * BN + first;
      lim = p.N - 1;
    }
    const int base_row = min(col0, lim);
    wbase[u] = p.w + static_cast<int64_t>(add + base_row) * p.w_stride + k0;
    woff[u] = static_cast<uint32_t>(min(col0 + lr, lim) - base_row) * static_cast<uint32_t>(p.w_stride) + piece * 16;
  }
  lds_bytes_t sm3 = (lds_bytes_t)(smem);
  auto issue = [&](int kt, int stage) {
#pragma unroll
    for (int u = 0; u < kWI; ++u) dma16(wbase[u] + kt * kBK + woff[u], (lds_ptr_t)(sm3 + stage * kStage + (wid * kWI + u) * 1024));
#pragma unroll
    for (int u = 0; u < 4; ++u) dma16(xbase + kt * (kBK * 2) + xoff[u], (lds_ptr_t)(sm3 + stage * kStage + kWBytes + (wid * 4 + u) * 1024));
  };

  // ---- this wave's weight tiles: first (unclamped) weight row of tile i; past-the-end tiles are multiplied and dropped ----
  auto tile_row0 = [&](int i) {
    if (p.fuse_silu) return (i < kWT / 2 ? 0 : half) + strip * (BN / 2) + wr * (kSL / 2) + (i % (kWT / 2)) * 16;
    return strip * BN + wr * kSL + i * 16;
  };

  // ---- fragment addresses ----
  const uint32_t sm_addr = (uint32_t)(uintptr_t)(sm3);
  const uint32_t wfoff = wr * (kSL * kBK) + r16 * 64 + ((g ^ (r16 >> 2)) & 3) * 16;
  uint32_t xfoff[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) xfoff[s] = kWBytes + wc * (64 * 128) + r16 * 128 + (((2 * g + s) ^ (r16 & 7)) & 7) * 16;

  f32x4_t acc[kWT][kXT];                               // [weight 16-row tile][activation 16-row tile]
  f32x4_t cacc[BLOCK ? kWT : 1][BLOCK ? kXT : 1];      // block scales: the accumulator of the chunk in hand
#pragma unroll
  for (int i = 0; i < kWT; ++i)
#pragma unroll
    for (int j = 0; j < kXT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if constexpr (BLOCK) {
#pragma unroll
    for (int i = 0; i < kWT; ++i)
#pragma unroll
      for (int j = 0; j < kXT; ++j) cacc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // block scales: row of the scale matrix of tile i, read through the constant address space so that the wave-uniform loads are
  // scalar loads (their own counter) and never queue up with the DMAs
  cst_f32_t bscale[BLOCK ? kWT : 1];
  float sc_cur[BLOCK ? kWT : 1], sc_nxt[BLOCK ? kWT : 1];
  if constexpr (BLOCK) {
#pragma unroll
    for (int i = 0; i < kWT; ++i) {
      const int row0 = __builtin_amdgcn_readfirstlane(min(tile_row0(i), p.N - 1));
      bscale[i] = (cst_f32_t)(p.scale + static_cast<int64_t>(row0 >> 7) * p.scale_stride);
      sc_cur[i] = bscale[i][c0];
    }
  }

  auto read_w = [&](uint32_t ad, u32x4_t (&wf)[4]) {
    wf[0] = lds_rd<0>(ad); wf[1] = lds_rd<1024>(ad); wf[2] = lds_rd<2048>(ad); wf[3] = lds_rd<3072>(ad);
  };
  auto read_x = [&](uint32_t ad, u32x4_t (&xf)[kXT]) {
    xf[0] = lds_rd<0>(ad); xf[1] = lds_rd<2048>(ad); xf[2] = lds_rd<4096>(ad); xf[3] = lds_rd<6144>(ad);
  };
  // the products of one k-step of four weight tiles (tiles i0 ..); NEXT: the second k-step's weights are widened row by row
  // behind the MFMAs that used the first's
  auto products = [&](int i0, bf16x8_t (&aw)[4], u32x4_t (&xf)[kXT], const u32x4_t (&wf)[4], auto next) {
#pragma unroll
    for (int j = 0; j < kXT; ++j) pin(xf[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < kXT; ++j) {
        f32x4_t& d = BLOCK ? cacc[BLOCK ? i0 + i : 0][BLOCK ? j : 0] : acc[i0 + i][j];
        d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[i], __builtin_bit_cast(bf16x8_t, xf[j]), d, 0, 0, 0);
      }
      if constexpr (decltype(next)::value) aw[i] = widen(wf[i], 1);
    }
  };

  // ---- the K walk.  Top of step t: this wave's pieces of tile t have landed once only the DMAs of the (up to kStages - 2)
  // tiles behind it are outstanding; barrier: tile t is complete and nobody reads tile t - 1 any more; refill that stage with
  // tile t + kStages - 1; multiply tile t.
#pragma unroll
  for (int u = 0; u < kStages - 1; ++u)
    if (u < nk) issue(u, u);
  int stage = 0;
  auto step = [&](int kt) {
    const int behind = nk - 1 - kt;                    // tiles after this one
    if (behind >= kStages - 2) wait_vm<(kStages - 2) * kPerStep>();
    else if (kStages > 3 && behind == 1) wait_vm<kPerStep>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + kStages - 1 < nk) issue(kt + kStages - 1, stage == 0 ? kStages - 1 : stage - 1);
    const uint32_t base = sm_addr + stage * kStage;
    // four weight tiles at a time (the wide form's second four are read last and multiplied last: 16 raw + 16 widened weight
    // registers in hand instead of 32 + 32)
    u32x4_t wf[kWT / 4][4], xf[2][kXT];
    bf16x8_t aw[4];
    read_w(base + wfoff, wf[0]);
    read_x(base + xfoff[0], xf[0]);
    read_x(base + xfoff[1], xf[1]);
    if constexpr (kWT == 8) read_w(base + wfoff + 4096, wf[1]);
    wait_lgkm<kXT + kWT - 4>();                        // LDS returns in order: four weight tiles and the first k-step's activations
#pragma unroll
    for (int i = 0; i < 4; ++i) pin(wf[0][i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) aw[i] = widen(wf[0][i], 0);
    products(0, aw, xf[0], wf[0], std::true_type{});
    wait_lgkm<kWT - 4>();
    products(0, aw, xf[1], wf[0], std::false_type{});
    if constexpr (kWT == 8) {
      wait_lgkm<0>();
#pragma unroll
      for (int i = 0; i < 4; ++i) pin(wf[1][i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) aw[i] = widen(wf[1][i], 0);
      products(4, aw, xf[0], wf[1], std::true_type{});
      products(4, aw, xf[1], wf[1], std::false_type{});
    }
    stage = stage == kStages - 1 ? 0 : stage + 1;
  };
  for (int c = c0; c < c1; ++c) {
    if constexpr (BLOCK) {
      const int cn = c + 1 < c1 ? c + 1 : c;
#pragma unroll
      for (int i = 0; i < kWT; ++i) sc_nxt[i] = bscale[i][cn];
    }
    step((c - c0) * 2);
    step((c - c0) * 2 + 1);
    if constexpr (BLOCK) {
#pragma unroll
      for (int i = 0; i < kWT; ++i) {
#pragma unroll
        for (int j = 0; j < kXT; ++j) {
          acc[i][j] += cacc[i][j] * sc_cur[i];
          cacc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        sc_cur[i] = sc_nxt[i];
      }
    }
  }

  // ---- epilogue: lane holds C^T[n = tile_row0(i) + 4 g + r][m = 16 j + r16] of this wave's patch.  The scale first: nothing
  // sees an unscaled accumulator.
  const int n_lim = p.fuse_silu ? half : p.N;          // columns of the output
  auto out_col = [&](int i) { return p.fuse_silu ? tile_row0(i) - (i < kWT / 2 ? 0 : half) : tile_row0(i); };
  if constexpr (!BLOCK) {
#pragma unroll
    for (int i = 0; i < kWT; ++i) {
      if (out_col(i) >= n_lim) continue;
      f32x4_t sc;
#pragma unroll
      for (int q = 0; q < 4; ++q) sc[q] = p.scale[p.scale_mode == 1 ? tile_row0(i) + g * 4 + q : 0];
#pragma unroll
      for (int j = 0; j < kXT; ++j) acc[i][j] *= sc;
    }
  }
#pragma unroll
  for (int j = 0; j < kXT; ++j) {
    const int64_t m = static_cast<int64_t>(rb) * kBM + wc * (kXT * 16) + j * 16 + r16;
    if (m >= p.M) continue;
    if (p.fuse_silu) {
      // weight tiles [0, kWT/2) = gate columns of this wave's slice, the other half = the matching up columns
#pragma unroll
      for (int i = 0; i < kWT / 2; ++i) {
        const int col = out_col(i) + g * 4;
        if (col >= half) continue;
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float gb = rbf(acc[i][j][q]);
          const float sl = rbf(gb / (1.0f + expf(-gb)));
          o[q] = sl * rbf(acc[i + kWT / 2][j][q]);
        }
        uint2 w2;
        w2.x = pack_bf2(o[0], o[1]); w2.y = pack_bf2(o[2], o[3]);
        *reinterpret_cast<uint2*>(p.y + m * p.y_stride + col) = w2;
      }
    } else {
#pragma unroll
      for (int i = 0; i < kWT; ++i) {
        const int col = tile_row0(i) + g * 4;
        if (col >= p.N) continue;
        if (p.part) {
          *reinterpret_cast<f32x4_t*>(p.part + (static_cast<int64_t>(split) * p.M + m) * p.N + col) = acc[i][j];
        } else {
          float o[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) o[q] = acc[i][j][q] + (p.bias ? bf2f(p.bias[col + q]) : 0.f);
          uint2 w2;
          w2.x = pack_bf2(o[0], o[1]); w2.y = pack_bf2(o[2], o[3]);
          *reinterpret_cast<uint2*>(p.y + m * p.y_stride + col) = w2;
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int64_t sgl_amd_dense_tiled_gemm_fp8_workspace_floats(int64_t M, int64_t N, int num_k_splits) {
  return num_k_splits > 1 ? static_cast<int64_t>(num_k_splits) * M * N : 0;
}

int sgl_amd_dense_tiled_gemm_fp8(const void* x, const void* w, const void* bias, void* y, int64_t M, int64_t N, int64_t K,
                                 int64_t x_row_stride, int64_t w_row_stride, int64_t y_row_stride, int epilogue, int block_n,
                                 int num_k_splits, void* ws_partials, void* stream, const float* w_scale, int scale_mode,
                                 int64_t scale_row_stride) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(M >= 1 && M <= 0x7fffffffLL, "dense_tiled_gemm_fp8: M=%lld rows (supported: >= 1)", (long long)M);
  SGL_CHECK_ARG(N > 0 && N % 16 == 0 && N <= 0x7fffffffLL && K >= kKC && K % kKC == 0 && K <= 0x7fffffffLL,
                "dense_tiled_gemm_fp8: need N %% 16 == 0 and K %% %d == 0 (got N=%lld K=%lld)", kKC, (long long)N, (long long)K);
  SGL_CHECK_ARG(x_row_stride % 8 == 0 && w_row_stride % 16 == 0 && y_row_stride % 4 == 0 && x_row_stride >= K && w_row_stride >= K,
                "dense_tiled_gemm_fp8: row strides must keep 16-byte (x, w: in bytes) / 8-byte (y) alignment");
  SGL_CHECK_ARG(w_scale && scale_mode >= 0 && scale_mode <= 2,
                "dense_tiled_gemm_fp8: fp8 weights need w_scale and scale_mode 0 (tensor), 1 (channel) or 2 (128 x 128 blocks)");
  SGL_CHECK_ARG(scale_mode != 2 || scale_row_stride >= K / kKC, "dense_tiled_gemm_fp8: block scales are [ceil(N / 128), K / 128] (row stride %lld < %lld)",
                (long long)scale_row_stride, (long long)(K / kKC));
  SGL_CHECK_ARG(epilogue == 0 || epilogue == 1, "dense_tiled_gemm_fp8: epilogue must be 0 (bias) or 1 (silu_and_mul)");
  SGL_CHECK_ARG(epilogue != 1 || (N % 32 == 0 && !bias), "dense_tiled_gemm_fp8: silu_and_mul needs N %% 32 == 0 (w is [2 I, K], I %% 16 == 0) and no bias");
  SGL_CHECK_ARG(block_n == 128 || block_n == 256, "dense_tiled_gemm_fp8: block_n must be 128 or 256 (got %d)", block_n);
  SGL_CHECK_ARG(scale_mode != 2 || block_n == 128, "dense_tiled_gemm_fp8: block scales run on the 128-row tile");
  SGL_CHECK_ARG(num_k_splits >= 1 && num_k_splits <= K / kKC, "dense_tiled_gemm_fp8: bad split count %d", num_k_splits);
  SGL_CHECK_ARG(num_k_splits == 1 || ws_partials, "dense_tiled_gemm_fp8: split-K needs the fp32 partials workspace");
  SGL_CHECK_ARG(num_k_splits == 1 || M <= kMaxCombineRows, "dense_tiled_gemm_fp8: split-K takes at most %d rows", kMaxCombineRows);
  SGL_CHECK_ARG(x && w && y, "dense_tiled_gemm_fp8: null operand");
  SGL_CHECK_ARG(reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(w) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 8 == 0,
                "dense_tiled_gemm_fp8: x and w must be 16-byte aligned, y 8-byte aligned");
  SGL_CHECK_ARG(x_row_stride <= (int64_t{1} << 22) && w_row_stride <= (int64_t{1} << 27),
                "dense_tiled_gemm_fp8: row stride beyond the 32-bit lane offsets of a tile");
  const int64_t n_out = epilogue == 1 ? N / 2 : N;
  SGL_CHECK_ARG(y_row_stride >= n_out, "dense_tiled_gemm_fp8: y row stride shorter than a row");
  hipStream_t st = as_stream(stream);
  Dense8Params p{};
  p.x = static_cast<const uint16_t*>(x); p.w = static_cast<const unsigned char*>(w); p.y = static_cast<uint16_t*>(y);
  p.part = num_k_splits > 1 ? static_cast<float*>(ws_partials) : nullptr;
  p.bias = p.part ? nullptr : static_cast<const uint16_t*>(bias);
  p.scale = w_scale; p.scale_mode = scale_mode; p.scale_stride = scale_row_stride;
  p.x_stride = x_row_stride; p.w_stride = w_row_stride; p.y_stride = y_row_stride;
  p.M = static_cast<int>(M); p.N = static_cast<int>(N); p.K = static_cast<int>(K);
  p.splits = num_k_splits;
  p.fuse_silu = epilogue == 1 && num_k_splits == 1;
  const int64_t strips = p.fuse_silu ? (N / 2 + block_n / 2 - 1) / (block_n / 2) : (N + block_n - 1) / block_n;
  const int64_t units = strips * num_k_splits;
  const int64_t row_blocks = (M + kBM - 1) / kBM, units8 = (units + 7) / 8;
  const int64_t wgs = 8 * units8 * row_blocks;
  SGL_CHECK_ARG(wgs <= 0x7fffffffLL, "dense_tiled_gemm_fp8: too many tiles");
  p.nstrips = static_cast<int>(strips); p.units = static_cast<int>(units);
  p.row_blocks = static_cast<int>(row_blocks); p.units8 = static_cast<int>(units8);
  const dim3 grid(static_cast<unsigned>(wgs)), block(kThreads);
  if (scale_mode == 2) {
    hipLaunchKernelGGL((dense_tiled_fp8_gemm_kernel<128, true>), grid, block, 0, st, p);
  } else if (block_n == 128) {
    hipLaunchKernelGGL((dense_tiled_fp8_gemm_kernel<128, false>), grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL((dense_tiled_fp8_gemm_kernel<256, false>), grid, block, 0, st, p);
  }
  if (p.part)
    launch_wstream_combine(p.part, static_cast<const uint16_t*>(bias), p.y, y_row_stride, 128, p.M, p.N, num_k_splits, epilogue == 1, st);
  SGL_CHECK_LAUNCH("dense_tiled_gemm_fp8");
  return 0;
}

}  // extern "C"
