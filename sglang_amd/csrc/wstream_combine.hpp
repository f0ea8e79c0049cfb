// Internal launchers of the split-K combine kernels of wstream_gemm.hip, for the other GEMMs that write fp32 partials
// [splits, M, N] (dense_tiled_gemm.hip, wstream_fp8_gemm.hip).  Not part of the C ABI.
#pragma once

#include "common.hpp"

namespace sgl_amd {

// silu == false: y[m, n] = bf16(sum over splits + bias[n])                     (bias may be null)
// silu == true : y[m, j] = silu_and_mul of the [gate | up] halves of the sum   (j < N / 2, no bias)
// The partials are summed in split order.  y_chunk_stride: 128 for a row-major y (see blocked_off()).
void launch_wstream_combine(const float* part, const uint16_t* bias, uint16_t* y, int64_t y_row_stride, int64_t y_chunk_stride,
                            int M, int N, int splits, bool silu, hipStream_t stream);

// h = bf16(sum over splits + bias); residual <- bf16(h + residual); y = bf16(RMSNorm(residual) * norm_w): one workgroup per row,
// N <= wstream_combine_norm_max_n()
int wstream_combine_norm_max_n();
void launch_wstream_combine_norm(const float* part, const uint16_t* bias, uint16_t* y, uint16_t* residual, const uint16_t* norm_w,
                                 int64_t y_row_stride, int64_t y_chunk_stride, int64_t residual_row_stride, int M, int N, int splits,
                                 float eps, hipStream_t stream);

// The body of sgl_amd_wstream_qkv_rope behind its GEMM: checks the rope / KV-pool arguments, runs `main_fn(ctx, N, stream)` (the
// GEMM that writes the [splits, M, N = (Hq + 2 Hkv) D] partials; non-zero = its error, passed on), then the rope + KV-store combine.
typedef int (*WstreamMainFn)(void* ctx, int64_t N, hipStream_t stream);
int wstream_qkv_rope_combine(const char* who, WstreamMainFn main_fn, void* ctx, const void* bias, void* q_out, int64_t M,
                             int num_q_heads, int num_kv_heads, int head_dim, int64_t q_row_stride, const int64_t* positions,
                             const void* cos_sin_cache, int cache_is_f32, int64_t rotary_dim, void* k_cache, void* v_cache,
                             const int64_t* cache_loc, int64_t cache_row_stride, int kv_fp8, float k_scale, float v_scale,
                             int page_size, int kv_layout_hnd, int num_k_splits, void* ws_partials, hipStream_t stream);

}  // namespace sgl_amd
