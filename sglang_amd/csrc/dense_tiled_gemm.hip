// Dense MFMA GEMM for tall decode batches on gfx950: y[M, N] = x[M, K] . w[N, K]^T (+ bias), 128 < M <= 512, bf16 in / out,
// fp32 accumulation.
//
// Replaces (reference: python/sglang of the sglang tree):
//   srt/layers/linear.py:1596-1660 UnquantizedLinearMethod.apply (the library matmul) for the decode projections of the
//   weak-scaled tensor-parallel batches (64 rows per rank x TP), and -- `silu_and_mul` epilogue -- the pair
//   gate_up_proj + srt/layers/activation.py:130-143 SiluAndMul.forward_native.
//
// The weight stream (wstream_gemm.hip) keeps the whole activation image next to its LDS ring, which ends at 128 rows; the
// MoE tile kernel (moe_tiled_gemm.hip) gathers rows and never splits K.  This kernel is the dense form between them:
//
//   work split   a workgroup (8 waves) owns BM = 256 activation rows x BN weight rows and walks one contiguous K range
//                in 64-wide steps.  BN = 128 (wide) or 64 (narrow).  One row block serves M <= 256, two serve M <= 512;
//                rows past M are clamped on load and dropped on store, weight rows past N likewise.  K is cut into
//                `splits` ranges of whole 128-element chunks (the ranges differ by at most one chunk).
//   launch order one-dimensional grid.  The hardware deals workgroups to the 8 XCDs round robin by their linear index
//                (workgroup i runs on XCD i % 8; the mapping this file relies on, as moe_gemm256_kernel does).  A unit =
//                (split, column strip), consecutive units walk the strips of one split.  With two row blocks, 16
//                consecutive workgroups are 8 units x 2 row blocks: workgroups 16 q + s and 16 q + 8 + s are the two row
//                blocks of unit 8 q + s, so they land on the same XCD one dispatch apart, run side by side and the later
//                read of every weight line hits that XCD's L2: HBM sees a weight byte once.
//   data path    both operands HBM / L2 -> LDS by LDS-DMA (global_load_lds, 16 bytes per lane, 1 KiB per wave
//                instruction: 8 rows x 128 bytes), THREE stages deep: while step t multiplies, the tiles of steps t + 1
//                and t + 2 are in flight.  One barrier per K step: it publishes tile t and retires the reads of tile t - 1,
//                whose stage the DMA of tile t + 2 then refills.  Row r of a tile lives at r * 128, its 16-byte piece pc in
//                slot pc ^ (r & 7); the swizzle is applied on the global side (lane -> piece), so the 16 rows a
//                ds_read_b128 fragment read touches spread over all 8 slots of the 128-byte rows: conflict-free.
//   products     v_mfma_f32_16x16x32_bf16 on the transposed problem (C^T = W . x^T): a lane ends up with 4 consecutive
//                output columns of one row -> 8-byte bf16 stores, 16-byte fp32 partial stores.  Wide: waves 2 (weight rows)
//                x 4 (activation rows), 64 x 64 outputs = 4 x 4 tiles each.  Narrow: waves 1 x 8, 64 x 32 = 4 x 2 tiles.
//                The fragments of both 32-wide halves of a step are read up front; the second half lands behind the
//                products of the first.
//   split-K      splits > 1: fp32 partials [splits, M, N] into the caller's workspace, summed in split order by the
//                combine kernels of wstream_gemm.hip (wstream_combine.hpp).  No atomics: the result is a fixed function of
//                (shape, BN, splits).
//   epilogues    none: bf16(acc + bias).  silu_and_mul with one split: the BN weight rows of a tile are, per 64-row wave
//                slice, [32 gate | 32 up] rows of the same 32 output columns, so a lane holds gate and up of the same
//                element and applies linear -> bf16, silu -> bf16, product -> bf16 (activation.py:141-143) in registers;
//                the [M, 2I] intermediate is never written.  With more splits: plain partials + the combine-silu kernel.
//
//   LDS / occupancy   stage = BN x 128 B (W) + 256 x 128 B (X).  Wide: 48 KiB x 3 = 144 KiB; narrow: 40 KiB x 3 = 120 KiB.
//                     Both forms: one workgroup (8 waves, 2 per SIMD) per CU of the 160 KiB LDS.
#include "common.hpp"
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

constexpr int kMinRows = 129, kMaxRows = 512;
constexpr int kBM = 256, kBK = 64, kKC = 128;         // rows per block, K step, K chunk (the unit split-K deals out)
constexpr int kXBytes = kBM * kBK * 2;                // 32 KiB: the activation tile of a stage
constexpr int kStages = 3;
constexpr int kThreads = 512;

struct DenseParams {
  const uint16_t* x;            // [M, K]
  const uint16_t* w;            // [N, K]   (silu: N = 2 I, gate rows then up rows)
  const uint16_t* bias;         // optional [N]; null when writing partials
  uint16_t* y;                  // [M, N]   ([M, I] fused silu)
  float* part;                  // [splits, M, N] when splits > 1, else null
  int64_t x_stride, w_stride, y_stride;
  int M, N, K;
  int splits, nstrips, units;   // units = splits * nstrips
  int row_blocks;               // 1 or 2
  int fuse_silu;                // one split only: N/2 output columns
};

__device__ __forceinline__ void dma16(const uint16_t* src, lds_ptr_t dst) {
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

template <int BN>
__global__ __launch_bounds__(kThreads, 1) void dense_tiled_gemm_kernel(DenseParams p) {
  static_assert(BN == 64 || BN == 128, "narrow (64) and wide (128) forms");
  constexpr int kWI = BN / 64;                         // W-tile DMA instructions per wave and step (the X tile: 4)
  constexpr int kPerStep = 4 + kWI;                    // LDS-DMA instructions a wave has in flight per tile
  constexpr int kWavesW = BN / 64, kWavesX = 8 / kWavesW;
  constexpr int kXT = kBM / kWavesX / 16;              // 16-row activation tiles per wave: 4 (wide) / 2 (narrow)
  constexpr int kWBytes = BN * kBK * 2;
  constexpr int kStage = kWBytes + kXBytes;            // [W tile | X tile]
  __shared__ __attribute__((aligned(1024))) unsigned char smem[kStages * kStage];

  // ---- workgroup -> (unit, row block): see "launch order" in the header ----
  const int id = blockIdx.x;
  const int unit = p.row_blocks == 2 ? (id >> 4) * 8 + (id & 7) : id;
  const int rb = p.row_blocks == 2 ? (id >> 3) & 1 : 0;
  if (unit >= p.units) return;                         // padding of the last group of 16 (whole workgroup, ahead of any barrier)
  const int split = unit / p.nstrips, strip = unit - split * p.nstrips;
  const int nch = p.K / kKC;
  const int c0 = static_cast<int>(static_cast<int64_t>(split) * nch / p.splits);
  const int c1 = static_cast<int>(static_cast<int64_t>(split + 1) * nch / p.splits);
  const int k0 = c0 * kKC, nk = (c1 - c0) * (kKC / kBK);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / kWavesX, wc = wid % kWavesX;    // this wave: weight rows 64 wr .., activation rows 16 kXT wc ..
  const int r16 = lane & 15, g = lane >> 4;

  // ---- DMA roles: instruction j of a tile covers its rows 8j .. 8j+7; lane i -> (row 8j + i/8, LDS slot i%8) and fetches the
  // global 16-byte piece (slot ^ (row & 7)) of that row.  Wave w issues j = 4w .. 4w+3 of X and j = kWI w .. of W.
  const int dr = lane >> 3, ds = lane & 7;
  const uint16_t* xsrc[4];
  const uint16_t* wsrc[kWI];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = (wid * 4 + u) * 8 + dr;            // 0..255
    const int piece = (ds ^ (row & 7)) * 8;
    const int m = rb * kBM + row;
    xsrc[u] = p.x + static_cast<int64_t>(m < p.M ? m : p.M - 1) * p.x_stride + k0 + piece;
  }
#pragma unroll
  for (int u = 0; u < kWI; ++u) {
    const int row = (wid * kWI + u) * 8 + dr;          // 0..BN-1
    const int piece = (ds ^ (row & 7)) * 8;
    int wrow;
    if (p.fuse_silu) {
      // tile rows: per 64-row wave slice [32 gate | 32 up] of output columns strip * BN/2 + slice * 32 + c
      const int half = p.N >> 1, slice = row >> 6, in = row & 63;
      const int col = strip * (BN / 2) + slice * 32 + (in & 31);
      wrow = (in < 32 ? 0 : half) + (col < half ? col : half - 1);
    } else {
      const int col = strip * BN + row;
      wrow = col < p.N ? col : p.N - 1;
    }
    wsrc[u] = p.w + static_cast<int64_t>(wrow) * p.w_stride + k0 + piece;
  }
  lds_bytes_t sm3 = (lds_bytes_t)(smem);
  auto issue = [&](int kt, int stage) {
    const int koff = kt * kBK;
#pragma unroll
    for (int u = 0; u < kWI; ++u) dma16(wsrc[u] + koff, (lds_ptr_t)(sm3 + stage * kStage + (wid * kWI + u) * 1024));
#pragma unroll
    for (int u = 0; u < 4; ++u) dma16(xsrc[u] + koff, (lds_ptr_t)(sm3 + stage * kStage + kWBytes + (wid * 4 + u) * 1024));
  };

  // ---- fragment addresses: row r of a tile at r * 128 bytes, piece pc in slot pc ^ (r & 7) ----
  const uint32_t sm_addr = (uint32_t)(uintptr_t)(sm3);
  uint32_t foff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) foff[kk] = r16 * 128 + (((kk * 4 + g) ^ (r16 & 7)) & 7) * 16;
  const uint32_t w_base = wr * (64 * 128);
  const uint32_t x_base = kWBytes + wc * (kXT * 16 * 128);

  f32x4_t acc[4][kXT];                                 // [weight 16-row tile][activation 16-row tile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < kXT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto read_frags = [&](uint32_t ad, u32x4_t (&wf)[4], u32x4_t (&xf)[kXT]) {
    wf[0] = lds_rd<0>(ad + w_base); wf[1] = lds_rd<2048>(ad + w_base); wf[2] = lds_rd<4096>(ad + w_base); wf[3] = lds_rd<6144>(ad + w_base);
    xf[0] = lds_rd<0>(ad + x_base); xf[1] = lds_rd<2048>(ad + x_base);
    if constexpr (kXT == 4) { xf[2] = lds_rd<4096>(ad + x_base); xf[3] = lds_rd<6144>(ad + x_base); }
  };
  auto products = [&](u32x4_t (&wf)[4], u32x4_t (&xf)[kXT]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) pin(wf[i]);
#pragma unroll
    for (int j = 0; j < kXT; ++j) pin(xf[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < kXT; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[i]), __builtin_bit_cast(bf16x8_t, xf[j]),
                                                            acc[i][j], 0, 0, 0);
  };

  // ---- the K walk.  Top of step t: this wave's pieces of tile t have landed (its pieces of tile t + 1 may still fly);
  // barrier: tile t is complete and nobody reads tile t - 1 any more; refill that stage with tile t + 2; multiply tile t.
  issue(0, 0);
  if (nk > 1) issue(1, 1);
  int stage = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) wait_vm<kPerStep>(); else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) issue(kt + 2, stage == 0 ? 2 : stage - 1);
    const uint32_t base = sm_addr + stage * kStage;
    u32x4_t wf[2][4], xf[2][kXT];
    read_frags(base + foff[0], wf[0], xf[0]);
    read_frags(base + foff[1], wf[1], xf[1]);
    wait_lgkm<4 + kXT>();                              // LDS returns in order: the first half's fragments are in
    products(wf[0], xf[0]);
    __builtin_amdgcn_sched_barrier(0);
    wait_lgkm<0>();
    products(wf[1], xf[1]);
    stage = stage == kStages - 1 ? 0 : stage + 1;
  }

  // ---- epilogue: lane holds C^T[n = 16 i + 4 g + r][m = 16 j + r16] of this wave's 64 x (16 kXT) patch ----
#pragma unroll
  for (int j = 0; j < kXT; ++j) {
    const int m = rb * kBM + wc * (kXT * 16) + j * 16 + r16;
    if (m >= p.M) continue;
    if (p.fuse_silu) {
      // weight tiles 0,1 = gate columns [0, 32) of this wave's slice, tiles 2,3 = the matching up columns
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int col = strip * (BN / 2) + wr * 32 + i * 16 + g * 4;
        if (col >= (p.N >> 1)) continue;
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gb = rbf(acc[i][j][r]);
          const float sl = rbf(gb / (1.0f + expf(-gb)));
          o[r] = sl * rbf(acc[i + 2][j][r]);
        }
        uint2 w2;
        w2.x = pack_bf2(o[0], o[1]); w2.y = pack_bf2(o[2], o[3]);
        *reinterpret_cast<uint2*>(p.y + static_cast<int64_t>(m) * p.y_stride + col) = w2;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = strip * BN + wr * 64 + i * 16 + g * 4;
        if (col >= p.N) continue;
        if (p.part) {
          *reinterpret_cast<f32x4_t*>(p.part + (static_cast<int64_t>(split) * p.M + m) * p.N + col) = acc[i][j];
        } else {
          float o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = acc[i][j][r] + (p.bias ? bf2f(p.bias[col + r]) : 0.f);
          uint2 w2;
          w2.x = pack_bf2(o[0], o[1]); w2.y = pack_bf2(o[2], o[3]);
          *reinterpret_cast<uint2*>(p.y + static_cast<int64_t>(m) * p.y_stride + col) = w2;
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int sgl_amd_dense_tiled_gemm_min_rows(void) { return kMinRows; }
int sgl_amd_dense_tiled_gemm_max_rows(void) { return kMaxRows; }

int64_t sgl_amd_dense_tiled_gemm_workspace_floats(int64_t M, int64_t N, int num_k_splits) {
  return num_k_splits > 1 ? static_cast<int64_t>(num_k_splits) * M * N : 0;
}

int sgl_amd_dense_tiled_gemm(const void* x, const void* w, const void* bias, void* y, int64_t M, int64_t N, int64_t K,
                             int64_t x_row_stride, int64_t w_row_stride, int64_t y_row_stride, int epilogue, int block_n,
                             int num_k_splits, void* ws_partials, void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(M >= kMinRows && M <= kMaxRows, "dense_tiled_gemm: M=%lld rows (supported: %d..%d)", (long long)M, kMinRows, kMaxRows);
  SGL_CHECK_ARG(N > 0 && N % 16 == 0 && N <= 0x7fffffffLL && K >= kKC && K % kKC == 0 && K <= 0x7fffffffLL,
                "dense_tiled_gemm: need N %% 16 == 0 and K %% %d == 0 (got N=%lld K=%lld)", kKC, (long long)N, (long long)K);
  SGL_CHECK_ARG(x_row_stride % 8 == 0 && w_row_stride % 8 == 0 && y_row_stride % 4 == 0 && x_row_stride >= K && w_row_stride >= K,
                "dense_tiled_gemm: row strides must keep 16-byte (x, w) / 8-byte (y) alignment");
  SGL_CHECK_ARG(epilogue == 0 || epilogue == 1, "dense_tiled_gemm: epilogue must be 0 (bias) or 1 (silu_and_mul)");
  SGL_CHECK_ARG(epilogue != 1 || (N % 32 == 0 && !bias), "dense_tiled_gemm: silu_and_mul needs N %% 32 == 0 (w is [2 I, K], I %% 16 == 0) and no bias");
  SGL_CHECK_ARG(block_n == 64 || block_n == 128, "dense_tiled_gemm: block_n must be 64 or 128 (got %d)", block_n);
  SGL_CHECK_ARG(num_k_splits >= 1 && num_k_splits <= K / kKC, "dense_tiled_gemm: bad split count %d", num_k_splits);
  SGL_CHECK_ARG(num_k_splits == 1 || ws_partials, "dense_tiled_gemm: split-K needs the fp32 partials workspace");
  SGL_CHECK_ARG(x && w && y, "dense_tiled_gemm: null operand");
  const int64_t n_out = epilogue == 1 ? N / 2 : N;
  SGL_CHECK_ARG(y_row_stride >= n_out, "dense_tiled_gemm: y row stride shorter than a row");
  hipStream_t st = as_stream(stream);
  DenseParams p{};
  p.x = static_cast<const uint16_t*>(x); p.w = static_cast<const uint16_t*>(w); p.y = static_cast<uint16_t*>(y);
  p.part = num_k_splits > 1 ? static_cast<float*>(ws_partials) : nullptr;
  p.bias = p.part ? nullptr : static_cast<const uint16_t*>(bias);
  p.x_stride = x_row_stride; p.w_stride = w_row_stride; p.y_stride = y_row_stride;
  p.M = static_cast<int>(M); p.N = static_cast<int>(N); p.K = static_cast<int>(K);
  p.splits = num_k_splits;
  p.fuse_silu = epilogue == 1 && num_k_splits == 1;
  const int64_t strips = p.fuse_silu ? (N / 2 + block_n / 2 - 1) / (block_n / 2) : (N + block_n - 1) / block_n;
  const int64_t units = strips * num_k_splits;
  p.row_blocks = M > kBM ? 2 : 1;
  const int64_t wgs = p.row_blocks == 2 ? (units + 7) / 8 * 16 : units;
  SGL_CHECK_ARG(wgs <= 0x7fffffffLL, "dense_tiled_gemm: too many tiles");
  p.nstrips = static_cast<int>(strips); p.units = static_cast<int>(units);
  if (block_n == 128) {
    hipLaunchKernelGGL(dense_tiled_gemm_kernel<128>, dim3(static_cast<unsigned>(wgs)), dim3(kThreads), 0, st, p);
  } else {
    hipLaunchKernelGGL(dense_tiled_gemm_kernel<64>, dim3(static_cast<unsigned>(wgs)), dim3(kThreads), 0, st, p);
  }
  if (p.part)
    launch_wstream_combine(p.part, static_cast<const uint16_t*>(bias), p.y, y_row_stride, 128, p.M, p.N, num_k_splits, epilogue == 1, st);
  SGL_CHECK_LAUNCH("dense_tiled_gemm");
  return 0;
}

}  // extern "C"
