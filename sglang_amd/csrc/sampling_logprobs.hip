// Log-probabilities straight from the logits for gfx950: the chosen token's, the n_top largest and a listed set of ids per row,
// without ever writing a [B, V] matrix.
//
// Replaces (reference, /root/reference/python/sglang):
//   srt/layers/sampler.py:143-146 (torch.log_softmax of the greedy branch), :237-271 (torch.log(probs) of the sampled
//   branch + the logprob outputs), get_top_logprobs / get_token_ids_logprobs (logprobs.topk, a gather per request).
//
// logprob(j) = z_j - lse,  z = x / T (one correctly rounded fp32 division, the rounding point of logits.div_(temperatures);
// z = x without temperatures),  lse = M + logf(S) with (M, S) the row's maximum and sum of expf(z - M).  Every one of
// the outputs is a small function of ONE pass over the logits, so the work is two launches:
//
//   ranges  grid (ranges, rows), 256 threads.  A workgroup owns one column range of one row (split_range_of's geometry) and
//           walks it in bursts of 8192 columns held in REGISTERS (8 slots x 4 columns per thread, one vector load each; 32
//           VGPRs).  From the registers it takes
//             - the burst's (max, sum) partial: the maximum of z is (the maximum of x) / T for T > 0 -- a correctly rounded
//               division is monotone -- so the first pass divides once, the second once per column; bursts are folded into
//               the range's partial in burst order with merge_partials' formula (fixed association: deterministic);
//             - its n_top best columns.  The order is (raw logit descending, column ascending) on a 64-bit key
//               (order-preserving value bits << 32 | 2^32 - 1 - column: kernels.argmax's key), never on z.  The registers
//               are turned into value bits in place; every wave runs n_top rounds of {wave arg-max of the lanes' current
//               best, the owning lane rescans its 32 registers for its next best BELOW the one just taken}: keys are unique,
//               so "below the last winner" replaces any bookkeeping of taken elements, and nothing is sorted.  No barrier
//               inside the rounds; the 4 wave lists and the range's running list (<= 160 keys) are merged by counting ranks.
//           Columns past the range's end, the <= 3 columns behind the last whole vector and rows that are not vector-aligned
//           go through the same code as masked lanes / element loads.
//   finish  grid (rows), 256 threads: merges the range partials in range order into lse, ranks the ranges x n_top keys in LDS
//           (counting: keys are unique) and writes the first n_top (column, z - lse), then gathers logits[row, ids[row]] and
//           the row's listed ids straight from global memory.
//
// Only enqueues on the given stream (hipGraph-capturable), no hidden state, caller-owned workspace with no initial state.
#include "common.hpp"
#include "sglang_amd.h"
#include "softmax_ranges.hpp"

using namespace sgl_amd;

namespace {

constexpr int kLogprobsMaxTop = 32;                 // >= 20 (the OpenAI limit on top_logprobs)
constexpr int kLpThreads = kSplitThreads;           // 256: four waves
constexpr int kLpWaves = kLpThreads / kWave;
constexpr int kLpSlots = 8;                         // 4-column vectors per thread and burst
constexpr int kLpRegs = 4 * kLpSlots;               // a thread's columns of one burst
constexpr int kLpSlotCols = 4 * kLpThreads;         // 1024 columns per slot
constexpr int kLpBurst = kLpSlots * kLpSlotCols;    // 8192 columns per burst
constexpr int kLpMaxSplits = 64;

typedef unsigned long long u64;

// order-preserving value bits: larger value = larger word, -0 == +0, NaN above everything (argmax_key of sampling.hip).
// Never 0 for a real column (-inf maps to 0x007fffff), so 0 marks "no column".
__device__ __forceinline__ uint32_t order_bits(float v) {
  uint32_t u = __float_as_uint(v + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return v != v ? 0xffffffffu : u;
}
__device__ __forceinline__ u64 order_key(uint32_t bits, uint32_t col) { return (static_cast<u64>(bits) << 32) | (0xffffffffu - col); }
__device__ __forceinline__ int key_col(u64 key) { return static_cast<int>(0xffffffffu - static_cast<uint32_t>(key)); }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// The thread's best register below the bound (lim_bits, lim_j) in the thread's own order (value bits descending, register index
// ascending = column ascending) among the first `ns` slots: its bits (0: none left) and index.  Statically indexed: the registers never leave the VGPRs.
__device__ __forceinline__ void next_best(const uint32_t (&u)[kLpRegs], int ns, uint32_t lim_bits, int lim_j, uint32_t* best_bits, int* best_j) {
  uint32_t bb = 0;
  int bj = 0;
#pragma unroll
  for (int j = 0; j < kLpRegs; ++j) {
    if (j / 4 < ns) {                               // (uniform: the burst's live slots)
      const bool below = u[j] < lim_bits || (u[j] == lim_bits && j > lim_j);
      if (below && u[j] > bb) { bb = u[j]; bj = j; }
    }
  }
  *best_bits = bb;
  *best_j = bj;
}

struct LogprobWs {
  float* partials;   // [B, S, 2]  (max, sum) of every range
  u64* cand;         // [B, S, n_top]  every range's best keys, descending; 0 = none
};
__host__ __device__ inline int64_t logprob_ws_bytes(int64_t batch, int splits, int n_top) {
  return batch * splits * 8 + batch * splits * n_top * 8;
}
__host__ __device__ inline LogprobWs logprob_ws_view(void* base, int64_t batch, int splits) {
  LogprobWs w;
  w.partials = static_cast<float*>(base);
  w.cand = reinterpret_cast<u64*>(static_cast<unsigned char*>(base) + batch * splits * 8);
  return w;
}

template <typename IN>
__global__ __launch_bounds__(kLpThreads) void logprob_ranges_kernel(const IN* __restrict__ logits, int64_t row_stride,
                                                                    const float* __restrict__ temperatures, int64_t V, int S, int n_top,
                                                                    LogprobWs ws) {
  __shared__ float red[kLpWaves];
  __shared__ u64 keys[(kLpWaves + 1) * kLogprobsMaxTop];   // [wave][n_top] lists of the burst, then the range's running list
  const int row = blockIdx.y, r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const IN* x = logits + static_cast<int64_t>(row) * row_stride;
  const bool has_t = temperatures != nullptr;
  const float t = has_t ? temperatures[row] : 1.0f;
  const bool max_first = !has_t || t > 0.f;         // (uniform) max(x / t) = max(x) / t
  const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(IN) - 1)) == 0;   // (uniform) the row takes vector loads
  int64_t b, e;
  split_range_of(V, S, r, &b, &e);
  u64* run = keys + kLpWaves * n_top;
  if (tid < n_top) run[tid] = 0;
  float M = -INFINITY, Sum = 0.f;                   // the range's partial so far (the same in every thread)

  for (int64_t cb = b; cb < e; cb += kLpBurst) {
    // ---- one burst: up to 8192 columns into registers ----
    float v[kLpRegs];
    uint32_t on = 0;                                // bit j: register j holds a column of the row
    const int64_t left = e - cb;
    const int ns = left >= kLpBurst ? kLpSlots : static_cast<int>((left + kLpSlotCols - 1) / kLpSlotCols);   // (uniform) live slots
#pragma unroll
    for (int s = 0; s < kLpSlots; ++s) {
      const int64_t i = cb + s * kLpSlotCols + 4 * tid;
      if (s >= ns) {                                // (uniform) a slot past the range's end costs nothing below
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * s + k] = -INFINITY;
      } else if (vec_ok && i + 4 <= e) {
        float q[4];
        ld4<IN>(x + i, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * s + k] = q[k];
        on |= 0xfu << (4 * s);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool in = i + k < e;
          v[4 * s + k] = in ? ld1(x + (in ? i + k : b)) : -INFINITY;
          on |= in ? (1u << (4 * s + k)) : 0u;
        }
      }
    }
    // ---- the burst's (max, sum): masked registers hold -inf (no effect on a maximum, expf(-inf - m) = 0) ----
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kLpRegs; ++j)
      if (j / 4 < ns) m = fmaxf(m, max_first ? v[j] : (((on >> j) & 1u) ? v[j] / t : -INFINITY));
    m = wave_max(m);
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (max_first && has_t) m = m / t;
    __syncthreads();
    float sum = 0.f;
    if (m > -INFINITY) {
#pragma unroll
      for (int j = 0; j < kLpRegs; ++j) {
        if (j / 4 < ns) {
          const float z = has_t ? v[j] / t : v[j];
          sum += ((on >> j) & 1u) ? expf(z - m) : 0.f;
        }
      }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    sum = (red[0] + red[2]) + (red[1] + red[3]);
    // fold into the range's partial, burst order (merge_partials' formula)
    const float nm = fmaxf(M, m);
    float acc = 0.f;
    if (M > -INFINITY) acc = Sum * expf(M - nm);
    if (m > -INFINITY) acc = __fmaf_rn(sum, expf(m - nm), acc);
    M = nm;
    Sum = acc;

    // ---- the burst's n_top best columns (uniform branch) ----
    if (n_top > 0) {
      uint32_t u[kLpRegs];
#pragma unroll
      for (int j = 0; j < kLpRegs; ++j) u[j] = ((on >> j) & 1u) ? order_bits(v[j]) : 0u;
      uint32_t bb;
      int bj;
      next_best(u, ns, 0xffffffffu, -1, &bb, &bj);
      for (int round = 0; round < n_top; ++round) {
        // register j = 4 s + k is column cb + 1024 s + 4 tid + k
        const uint32_t col = static_cast<uint32_t>(cb + (bj >> 2) * kLpSlotCols + 4 * tid + (bj & 3));
        const u64 mine = bb ? order_key(bb, col) : 0ull;
        const u64 win = wave_max_u64(mine);
        if (lane == 0) keys[wid * n_top + round] = win;
        if (win == 0ull) {                          // (wave-uniform) the wave ran out of columns
          for (int q = round + 1; q < n_top; ++q)
            if (lane == 0) keys[wid * n_top + q] = 0ull;
          break;
        }
        if (mine == win) next_best(u, ns, bb, bj, &bb, &bj);
      }
      __syncthreads();
      // the 4 wave lists + the running list -> the running list: rank = how many keys are larger (keys are unique)
      const int N = (kLpWaves + 1) * n_top;         // <= 160
      u64 key = 0;
      int rank = 0;
      if (tid < N) {
        key = keys[tid];
        if (key) {
          for (int q = 0; q < N; ++q) rank += keys[q] > key;
        }
      }
      __syncthreads();
      if (tid < n_top) run[tid] = 0;
      __syncthreads();
      if (key && rank < n_top) run[rank] = key;
    }
    __syncthreads();                                // (red and the lists are rewritten by the next burst)
  }

  const int64_t o = static_cast<int64_t>(row) * S + r;
  if (tid == 0) { ws.partials[2 * o] = M; ws.partials[2 * o + 1] = Sum; }
  if (tid < n_top) ws.cand[o * n_top + tid] = run[tid];
}

template <typename IN>
__global__ __launch_bounds__(kLpThreads) void logprob_finish_kernel(const IN* __restrict__ logits, int64_t row_stride,
                                                                    const float* __restrict__ temperatures, const void* __restrict__ ids,
                                                                    int ids_is_int64, int64_t V, int S, int n_top,
                                                                    const int32_t* __restrict__ req_offsets, const int32_t* __restrict__ req_ids,
                                                                    float* __restrict__ chosen, float* __restrict__ top_val,
                                                                    int32_t* __restrict__ top_idx, float* __restrict__ req_val, LogprobWs ws) {
  __shared__ u64 keys[kLpMaxSplits * kLogprobsMaxTop];
  __shared__ int filled[kLogprobsMaxTop];
  const int row = blockIdx.x, tid = threadIdx.x;
  const IN* x = logits + static_cast<int64_t>(row) * row_stride;
  const bool has_t = temperatures != nullptr;
  const float t = has_t ? temperatures[row] : 1.0f;
  float M, Sum;
  merge_partials(ws.partials + static_cast<int64_t>(row) * S * 2, S, &M, &Sum);
  const float lse = M + logf(Sum);
  auto logprob_at = [&](int64_t col) {
    const float v = ld1(x + col);
    return (has_t ? v / t : v) - lse;
  };

  if (n_top > 0) {
    const int N = S * n_top;
    const u64* cand = ws.cand + static_cast<int64_t>(row) * N;
    for (int i = tid; i < N; i += kLpThreads) keys[i] = cand[i];
    if (tid < n_top) filled[tid] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kLpThreads) {
      const u64 key = keys[i];
      if (key == 0ull) continue;
      int rank = i % n_top;                         // a range's list is descending: its own earlier entries are larger
      const int own = i - rank;
      for (int q = 0; q < own; ++q) rank += keys[q] > key;
      for (int q = own + n_top; q < N; ++q) rank += keys[q] > key;
      if (rank < n_top) {
        const int col = key_col(key);
        top_idx[static_cast<int64_t>(row) * n_top + rank] = col;
        top_val[static_cast<int64_t>(row) * n_top + rank] = logprob_at(col);
        filled[rank] = 1;
      }
    }
    __syncthreads();
    // fewer than n_top columns in the row: the rest of the list is (-1, -inf)
    if (tid < n_top && !filled[tid]) {
      top_idx[static_cast<int64_t>(row) * n_top + tid] = -1;
      top_val[static_cast<int64_t>(row) * n_top + tid] = -INFINITY;
    }
  }

  // an id outside [0, V) is never dereferenced: its entry is NaN
  if (ids != nullptr && tid == 0) {
    const int64_t id = ids_is_int64 ? static_cast<const int64_t*>(ids)[row] : static_cast<int64_t>(static_cast<const int32_t*>(ids)[row]);
    chosen[row] = (id >= 0 && id < V) ? logprob_at(id) : __uint_as_float(0x7fc00000u);
  }
  if (req_offsets != nullptr && req_ids != nullptr) {
    const int lo = req_offsets[row], hi = req_offsets[row + 1];
    for (int i = lo + tid; i < hi; i += kLpThreads) {
      const int64_t id = req_ids[i];
      req_val[i] = (id >= 0 && id < V) ? logprob_at(id) : __uint_as_float(0x7fc00000u);
    }
  }
}

}  // namespace

extern "C" {

int sgl_amd_logprobs_max_top(void) { return kLogprobsMaxTop; }

int64_t sgl_amd_logprobs_workspace_bytes(int64_t batch, int num_splits, int n_top) { return logprob_ws_bytes(batch, num_splits, n_top); }

int sgl_amd_logprobs_from_logits(const void* logits, int logits_is_bf16, int64_t row_stride, const float* temperatures, const void* ids,
                                 int ids_is_int64, int64_t batch, int64_t vocab, int n_top, const int32_t* req_offsets,
                                 const int32_t* req_ids, int64_t req_total, float* chosen_logprob, float* top_val, int32_t* top_idx,
                                 float* req_val, int num_splits, void* workspace, void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(n_top >= 0 && n_top <= kLogprobsMaxTop, "logprobs_from_logits: n_top must be in [0, %d] (sgl_amd_logprobs_max_top), got %d",
                kLogprobsMaxTop, n_top);
  SGL_CHECK_ARG(n_top == 0 || (top_val != nullptr && top_idx != nullptr), "logprobs_from_logits: n_top = %d needs top_val and top_idx", n_top);
  SGL_CHECK_ARG(ids == nullptr || chosen_logprob != nullptr, "logprobs_from_logits: ids need chosen_logprob");
  const bool listed = req_offsets != nullptr && req_ids != nullptr;
  SGL_CHECK_ARG(req_total >= 0 && req_total <= 0x7fffffffLL && (!listed || req_total == 0 || req_val != nullptr),
                "logprobs_from_logits: %lld listed ids need req_val", static_cast<long long>(req_total));
  SGL_CHECK_ARG(vocab > 0 && vocab <= 0x7fffffffLL, "logprobs_from_logits: vocab must be in [1, 2^31)");
  SGL_CHECK_ARG(batch >= 0 && batch <= 65535, "logprobs_from_logits: batch <= 65535");
  SGL_CHECK_ARG(num_splits >= 1 && num_splits <= kLpMaxSplits, "logprobs_from_logits: 1..%d column ranges", kLpMaxSplits);
  SGL_CHECK_ARG(logits != nullptr && row_stride >= vocab, "logprobs_from_logits: logits [batch, vocab] with row stride >= vocab");
  SGL_CHECK_ARG(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "logprobs_from_logits: needs an 8-byte aligned workspace");
  if (batch == 0) return 0;
  const LogprobWs ws = logprob_ws_view(workspace, batch, num_splits);
  const dim3 rgrid(num_splits, static_cast<unsigned>(batch));
#define SGL_LAUNCH_LOGPROBS(IN_)                                                                                                          \
  do {                                                                                                                                    \
    const IN_* x = static_cast<const IN_*>(logits);                                                                                       \
    hipLaunchKernelGGL(logprob_ranges_kernel<IN_>, rgrid, dim3(kLpThreads), 0, as_stream(stream), x, row_stride, temperatures, vocab,     \
                       num_splits, n_top, ws);                                                                                            \
    hipLaunchKernelGGL(logprob_finish_kernel<IN_>, dim3(batch), dim3(kLpThreads), 0, as_stream(stream), x, row_stride, temperatures, ids, \
                       ids_is_int64, vocab, num_splits, n_top, listed ? req_offsets : nullptr, listed ? req_ids : nullptr, chosen_logprob, \
                       top_val, top_idx, req_val, ws);                                                                                    \
  } while (0)
  if (logits_is_bf16) SGL_LAUNCH_LOGPROBS(uint16_t);
  else SGL_LAUNCH_LOGPROBS(float);
#undef SGL_LAUNCH_LOGPROBS
  SGL_CHECK_LAUNCH("logprobs_from_logits");
  return 0;
}

}  // extern "C"
