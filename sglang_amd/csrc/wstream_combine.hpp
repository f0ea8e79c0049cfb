// Internal launcher of the split-K combine kernels of wstream_gemm.hip, for the other GEMMs that write fp32 partials
// [splits, M, N] (dense_tiled_gemm.hip).  Not part of the C ABI.
#pragma once

#include "common.hpp"

namespace sgl_amd {

// silu == false: y[m, n] = bf16(sum over splits + bias[n])                     (bias may be null)
// silu == true : y[m, j] = silu_and_mul of the [gate | up] halves of the sum   (j < N / 2, no bias)
// The partials are summed in split order.  y_chunk_stride: 128 for a row-major y (see blocked_off()).
void launch_wstream_combine(const float* part, const uint16_t* bias, uint16_t* y, int64_t y_row_stride, int64_t y_chunk_stride,
                            int M, int N, int splits, bool silu, hipStream_t stream);

}  // namespace sgl_amd
