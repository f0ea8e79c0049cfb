// The second half of a speculative verify step for gfx950: the tree tables from parent lists, and tree acceptance + the bonus token
// straight from the verify forward's logits, without ever writing a [rows, V] probability (or fp32) matrix.
//
// Replaces (reference, /root/reference): sgl-kernel build_tree_kernel_efficient (mask, positions, retrive_next_token /
// retrive_next_sibling), verify_tree_greedy and tree_speculative_sampling_target_only with zero draft probabilities
// (speculative/eagle_info.py EagleVerifyInput.verify: softmax(logits / T) over [B * nd, V] first, then the op).
//
// build_verify_tree   grid (B, row-blocks), 256 threads.  A workgroup puts its request's parent list and one 64-bit ancestor word
//           per node into LDS (nd <= 64), writes positions / next_token / next_sibling (row-block 0) and its share of the request's
//           [nd, kv + nd] mask block as 16-byte stores: the block is a byte range of the flat mask, cut at 16-byte boundaries of the
//           mask itself (its offset is whatever the earlier requests left), head and tail bytes by element stores.
//
// tree_accept_from_logits: p(.) = softmax(logits[row] / T) is only ever needed at a handful of columns per row plus, for the B last
// rows, as a cumulative sum, so:
//   ranges  grid (ranges, B * nd), 256 threads: THE one pass over the logits.  A workgroup walks its column range of one row in
//           bursts of 8192 columns held in registers (8 x 4 columns per thread, one vector load each) and leaves one 8-byte slot:
//           the (max, sum) partial of softmax_ranges.hpp for a sampled request, the range's arg-max key (kernels.argmax's order:
//           value bits << 32 | 2^32 - 1 - column) for a greedy one.
//   walk    grid (B), 64 threads.  Lane j merges the partials of node j's row (merge_partials: range order), the lanes rebuild the
//           parent of every node from the two tables, lane j gathers logits[b, parent(j), token(j)] and turns it into a probability
//           with softmax_prob (greedy: compares the token with the parent row's arg-max); lane 0 walks the tree.  Writes
//           accept_index / accept_len / last_node, for greedy requests the bonus token (they are finished), for sampled ones the
//           last node's rejected tokens and (max, sum) into the workspace.
//   final   grid (final ranges, B), 256 threads, sampled requests only, row last_node: the residual mass of every range --
//           the probabilities with the rejected tokens at exactly zero, through an LDS bitmap of the burst's 8192 columns (no
//           subtract-afterwards cancellation) -- summed in a fixed order.
//   pick    grid (B), 256 threads: scans the range masses in range order for the range holding u * total, then rescans that one
//           range in 1024-column steps with a block prefix scan for the first column whose inclusive mass exceeds it (the last
//           column with residual mass when rounding leaves none).
// Rows that are not vector-aligned and the columns behind the last whole vector take element loads through the same code.
// Only enqueues on the given stream (hipGraph-capturable), no hidden state, caller-owned workspace with no initial state; every
// sum has a fixed association, so the result is run-to-run deterministic.
#include "common.hpp"
#include "sglang_amd.h"
#include "softmax_ranges.hpp"

using namespace sgl_amd;

namespace {

constexpr int kTaMaxNodes = 64;                     // one 64-bit ancestor word per node; a lane per node in the walk
constexpr int kTaMaxSplits = 64;
constexpr int kTaThreads = kSplitThreads;           // 256: four waves
constexpr int kTaWaves = kTaThreads / kWave;
constexpr int kTaSlots = 8;                         // 4-column vectors per thread and burst
constexpr int kTaRegs = 4 * kTaSlots;
constexpr int kTaSlotCols = 4 * kTaThreads;         // 1024 columns per slot
constexpr int kTaBurst = kTaSlots * kTaSlotCols;    // 8192 columns per burst

typedef unsigned long long u64;

// kernels.argmax's key: larger value = larger key, on ties the smaller column, NaN above everything, -0 == +0; never 0 for a column
__device__ __forceinline__ u64 argmax_key(float v, uint32_t col) {
  uint32_t u = __float_as_uint(v + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if (v != v) u = 0xffffffffu;
  return (static_cast<u64>(u) << 32) | (0xffffffffu - col);
}
__device__ __forceinline__ int key_col(u64 key) { return static_cast<int>(0xffffffffu - static_cast<uint32_t>(key)); }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

struct TreeAcceptWs {
  u64* slots;      // [B * nd, S]  a range's (max, sum) pair (sampled request) or arg-max key (greedy request)
  float* stat;     // [B, 2]       (max, sum) of the last node's row
  float* fin;      // [B, S2]      residual mass of every final range
  int32_t* rej;    // [B, nd]      the tokens rejected at the last node
  int32_t* nrej;   // [B]
};
__host__ __device__ inline int64_t tree_accept_ws_bytes(int64_t batch, int nd, int splits, int final_splits) {
  return batch * nd * splits * 8 + batch * 8 + (batch * final_splits * 4 + batch * nd * 4 + batch * 4 + 7) / 8 * 8;
}
__host__ __device__ inline TreeAcceptWs tree_accept_ws_view(void* base, int64_t batch, int nd, int splits, int final_splits) {
  TreeAcceptWs w;
  w.slots = static_cast<u64*>(base);
  w.stat = reinterpret_cast<float*>(w.slots + batch * nd * splits);
  w.fin = w.stat + 2 * batch;
  w.rej = reinterpret_cast<int32_t*>(w.fin + batch * final_splits);
  w.nrej = w.rej + batch * nd;
  return w;
}

// Columns [cb, min(cb + kTaBurst, e)) of the row into registers: register 4 s + k = column cb + 1024 s + 4 tid + k, -inf past e.
// Returns the live slots (uniform).  cb is a multiple of four columns behind the row's start: with vec_ok every slot is aligned.
template <typename IN>
__device__ __forceinline__ int load_burst(const IN* x, bool vec_ok, int64_t cb, int64_t e, float (&v)[kTaRegs]) {
  const int64_t left = e - cb;
  const int ns = left >= kTaBurst ? kTaSlots : static_cast<int>((left + kTaSlotCols - 1) / kTaSlotCols);
#pragma unroll
  for (int s = 0; s < kTaSlots; ++s) {
    const int64_t i = cb + s * kTaSlotCols + 4 * threadIdx.x;
    if (s >= ns) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[4 * s + k] = -INFINITY;
    } else if (vec_ok && i + 4 <= e) {
      float q[4];
      ld4<IN>(x + i, q);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[4 * s + k] = q[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = i + k < e;
        v[4 * s + k] = in ? ld1(x + (in ? i + k : cb)) : -INFINITY;
      }
    }
  }
  return ns;
}

__device__ __forceinline__ float request_temperature(const float* temperatures, int b) { return temperatures != nullptr ? temperatures[b] : 0.f; }

template <typename IN>
__global__ __launch_bounds__(kTaThreads) void tree_accept_ranges_kernel(const IN* __restrict__ logits, int64_t row_stride,
                                                                        const float* __restrict__ temperatures, int nd, int64_t V, int S,
                                                                        TreeAcceptWs ws) {
  __shared__ float red[kTaWaves];
  __shared__ u64 kred[kTaWaves];
  const int row = blockIdx.y, r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const IN* x = logits + static_cast<int64_t>(row) * row_stride;
  const float t = request_temperature(temperatures, row / nd);
  const bool greedy = !(t > 0.f);                   // (uniform)
  const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(IN) - 1)) == 0;
  int64_t b, e;
  split_range_of(V, S, r, &b, &e);
  float M = -INFINITY, Sum = 0.f;                   // the range's partial so far (the same in every thread)
  u64 best = 0ull;

  for (int64_t cb = b; cb < e; cb += kTaBurst) {
    float v[kTaRegs];
    const int ns = load_burst<IN>(x, vec_ok, cb, e, v);
    if (greedy) {
#pragma unroll
      for (int j = 0; j < kTaRegs; ++j) {
        const int64_t col = cb + (j >> 2) * kTaSlotCols + 4 * tid + (j & 3);
        if (j / 4 < ns && col < e) {
          const u64 key = argmax_key(v[j], static_cast<uint32_t>(col));
          best = key > best ? key : best;
        }
      }
      continue;
    }
    // the burst's (max, sum): the maximum of x / t is (the maximum of x) / t for t > 0 (a correctly rounded division is monotone);
    // masked registers hold -inf: no effect on the maximum, expf(-inf - m) = 0
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kTaRegs; ++j)
      if (j / 4 < ns) m = fmaxf(m, v[j]);
    m = wave_max(m);
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) / t;
    __syncthreads();
    float sum = 0.f;
    if (m > -INFINITY) {
#pragma unroll
      for (int j = 0; j < kTaRegs; ++j)
        if (j / 4 < ns) sum += expf(v[j] / t - m);
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    sum = (red[0] + red[2]) + (red[1] + red[3]);
    __syncthreads();
    // fold into the range's partial in burst order (merge_partials' formula)
    const float nm = fmaxf(M, m);
    float acc = 0.f;
    if (M > -INFINITY) acc = Sum * expf(M - nm);
    if (m > -INFINITY) acc = __fmaf_rn(sum, expf(m - nm), acc);
    M = nm;
    Sum = acc;
  }

  u64* slot = ws.slots + static_cast<int64_t>(row) * S + r;
  if (greedy) {
    best = wave_max_u64(best);
    if (lane == 0) kred[wid] = best;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kTaWaves; ++w) best = kred[w] > best ? kred[w] : best;
      *slot = best;
    }
  } else if (tid == 0) {
    float* pr = reinterpret_cast<float*>(slot);
    pr[0] = M;
    pr[1] = Sum;
  }
}

template <typename IN>
__global__ __launch_bounds__(kTaMaxNodes) void tree_accept_walk_kernel(
    const IN* __restrict__ logits, int64_t row_stride, const float* __restrict__ temperatures, const void* __restrict__ candidates,
    int cand_is_int64, const int32_t* __restrict__ next_token, const int32_t* __restrict__ next_sibling, const float* __restrict__ uniform,
    float threshold_single, float threshold_acc, int nd, int64_t V, int S, int32_t* __restrict__ accept_index,
    int32_t* __restrict__ accept_len, int32_t* __restrict__ bonus_token, int32_t* __restrict__ last_node, TreeAcceptWs ws) {
  __shared__ float sM[kTaMaxNodes], sSum[kTaMaxNodes], sProb[kTaMaxNodes];
  __shared__ int sArg[kTaMaxNodes], sParent[kTaMaxNodes], sTok[kTaMaxNodes], sNext[kTaMaxNodes], sSib[kTaMaxNodes];
  __shared__ int sAccepted;
  const int b = blockIdx.x, j = threadIdx.x;
  const int64_t base = static_cast<int64_t>(b) * nd;
  const float t = request_temperature(temperatures, b);
  const bool greedy = !(t > 0.f);

  if (j < nd) {
    const u64* slots = ws.slots + (base + j) * S;
    sM[j] = 0.f;
    sSum[j] = 1.f;
    sArg[j] = -1;
    if (greedy) {
      u64 k = 0ull;
      for (int s = 0; s < S; ++s) k = slots[s] > k ? slots[s] : k;
      sArg[j] = k ? key_col(k) : -1;
    } else {
      merge_partials(reinterpret_cast<const float*>(slots), S, &sM[j], &sSum[j]);
    }
    // a child or a later sibling has a higher index than the node: anything else ends the list (and every loop below)
    const int nt = next_token[base + j], sb = next_sibling[base + j];
    sNext[j] = (nt > j && nt < nd) ? nt : -1;
    sSib[j] = (sb > j && sb < nd) ? sb : -1;
    sParent[j] = -1;
    const int64_t tok = cand_is_int64 ? static_cast<const int64_t*>(candidates)[base + j]
                                      : static_cast<int64_t>(static_cast<const int32_t*>(candidates)[base + j]);
    sTok[j] = (tok >= 0 && tok < V) ? static_cast<int>(tok) : -1;    // outside the vocabulary: never read, probability 0
  }
  __syncthreads();
  if (j < nd)
    for (int c = sNext[j]; c != -1; c = sSib[c]) sParent[c] = j;
  __syncthreads();
  if (j < nd) {
    const int p = sParent[j], tok = sTok[j];
    float q = 0.f;                                  // p(token of j | parent's row); greedy: 1 iff it is the parent row's arg-max
    if (p >= 0 && tok >= 0) {
      if (greedy) q = tok == sArg[p] ? 1.f : 0.f;
      else q = softmax_prob(ld1(logits + (base + p) * row_stride + tok), t, sM[p], sSum[p]);
    }
    sProb[j] = q;
  }
  __syncthreads();

  if (j == 0) {
    int cur = 0, n = 0, nrej = 0;
    float coin = uniform != nullptr ? uniform[base] : 0.f;
    accept_index[base] = 0;
    for (;;) {
      float prob_acc = 0.f;
      nrej = 0;
      int c = sNext[cur];
      for (; c != -1; c = sSib[c]) {
        const float q = sProb[c];
        bool take;
        if (greedy) {
          take = q != 0.f;
        } else {
          prob_acc += q;
          take = coin <= prob_acc / threshold_acc || q >= threshold_single;
        }
        if (take) break;
        if (!greedy && sTok[c] >= 0) ws.rej[base + nrej++] = sTok[c];
      }
      if (c == -1) break;
      cur = c;
      accept_index[base + ++n] = c;
      coin = uniform != nullptr ? uniform[base + c] : 0.f;
    }
    accept_len[b] = n;
    last_node[b] = cur;
    sAccepted = n;
    if (greedy) {
      bonus_token[b] = sArg[cur] >= 0 ? sArg[cur] : 0;
    } else {
      ws.nrej[b] = nrej;
      ws.stat[2 * b] = sM[cur];
      ws.stat[2 * b + 1] = sSum[cur];
    }
  }
  __syncthreads();
  if (j < nd && j > sAccepted) accept_index[base + j] = -1;
}

template <typename IN>
__global__ __launch_bounds__(kTaThreads) void tree_accept_final_kernel(const IN* __restrict__ logits, int64_t row_stride,
                                                                       const float* __restrict__ temperatures,
                                                                       const int32_t* __restrict__ last_node, int nd, int64_t V, int S2,
                                                                       TreeAcceptWs ws) {
  __shared__ float red[kTaWaves];
  __shared__ uint32_t bits[kTaBurst / 32];          // 256 words: a bit per column of the burst
  __shared__ int srej[kTaMaxNodes];
  const int b = blockIdx.y, r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float t = request_temperature(temperatures, b);
  if (!(t > 0.f)) return;                           // (uniform) greedy requests were finished by the walk
  const int64_t base = static_cast<int64_t>(b) * nd;
  int last = last_node[b];
  last = last >= 0 && last < nd ? last : 0;
  const IN* x = logits + (base + last) * row_stride;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(IN) - 1)) == 0;
  int nrej = ws.nrej[b];
  nrej = nrej < 0 ? 0 : (nrej > nd ? nd : nrej);
  if (tid < nrej) srej[tid] = ws.rej[base + tid];
  const float M = ws.stat[2 * b], Sum = ws.stat[2 * b + 1];
  int64_t rb, re;
  split_range_of(V, S2, r, &rb, &re);
  __syncthreads();
  float mass = 0.f;

  for (int64_t cb = rb; cb < re; cb += kTaBurst) {
    bool masked = false;                            // (uniform) a rejected token falls into this burst
    for (int i = 0; i < nrej; ++i) masked = masked || (srej[i] >= cb && srej[i] < cb + kTaBurst);
    if (masked) {
      bits[tid] = 0u;
      __syncthreads();
      if (tid < nrej && srej[tid] >= cb && srej[tid] < cb + kTaBurst) {
        const int o = static_cast<int>(srej[tid] - cb);
        atomicOr(&bits[o >> 5], 1u << (o & 31));
      }
      __syncthreads();
    }
    float v[kTaRegs];
    const int ns = load_burst<IN>(x, vec_ok, cb, re, v);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < kTaRegs; ++j) {
      if (j / 4 < ns) {
        const int o = (j >> 2) * kTaSlotCols + 4 * tid + (j & 3);
        float p = softmax_prob(v[j], t, M, Sum);    // (a column past the range's end holds -inf: exactly 0)
        if (masked && ((bits[o >> 5] >> (o & 31)) & 1u)) p = 0.f;
        sum += p;
      }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    mass += (red[0] + red[2]) + (red[1] + red[3]);
    __syncthreads();                                // (red and the bitmap are rewritten by the next burst)
  }
  if (tid == 0) ws.fin[static_cast<int64_t>(b) * S2 + r] = mass;
}

template <typename IN>
__global__ __launch_bounds__(kTaThreads) void tree_accept_pick_kernel(const IN* __restrict__ logits, int64_t row_stride,
                                                                      const float* __restrict__ temperatures,
                                                                      const int32_t* __restrict__ last_node,
                                                                      const float* __restrict__ uniform_final, int nd, int64_t V, int S2,
                                                                      int32_t* __restrict__ bonus_token, TreeAcceptWs ws) {
  __shared__ float wtot[kTaWaves];
  __shared__ int srej[kTaMaxNodes];
  __shared__ int sFound, sLast;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float t = request_temperature(temperatures, b);
  if (!(t > 0.f)) return;                           // (uniform)
  const int64_t base = static_cast<int64_t>(b) * nd;
  int last = last_node[b];
  last = last >= 0 && last < nd ? last : 0;
  const IN* x = logits + (base + last) * row_stride;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(IN) - 1)) == 0;
  int nrej = ws.nrej[b];
  nrej = nrej < 0 ? 0 : (nrej > nd ? nd : nrej);
  if (tid < nrej) srej[tid] = ws.rej[base + tid];
  if (tid == 0) { sFound = 0x7fffffff; sLast = -1; }
  const float M = ws.stat[2 * b], Sum = ws.stat[2 * b + 1];

  // the range holding u * total: the first whose inclusive mass exceeds it, in range order (every thread, the same bits)
  const float* fin = ws.fin + static_cast<int64_t>(b) * S2;
  float total = 0.f;
  for (int r = 0; r < S2; ++r) total += fin[r];
  float target = (uniform_final != nullptr ? uniform_final[b] : 0.f) * total;
  int pick = -1, lastnz = -1;
  float cum = 0.f, start = 0.f, start_nz = 0.f;
  for (int r = 0; r < S2; ++r) {
    const float f = fin[r];
    if (f > 0.f) { lastnz = r; start_nz = cum; }
    if (pick < 0 && f > 0.f && cum + f > target) { pick = r; start = cum; }
    cum += f;
  }
  if (pick < 0) {                                   // rounding (or u >= 1) left no range: the last column with residual mass wins
    if (lastnz < 0) {                               // no residual mass at all (every column rejected or a NaN row): token 0
      if (tid == 0) bonus_token[b] = 0;
      return;
    }
    pick = lastnz;
    start = start_nz;
    target = INFINITY;
  }
  int64_t rb, re;
  split_range_of(V, S2, pick, &rb, &re);
  __syncthreads();

  float run = start;                                // the residual mass in front of the step (the same in every thread)
  for (int64_t cb = rb; cb < re; cb += kTaSlotCols) {
    const int64_t i = cb + 4 * tid;
    float p[4];
    if (vec_ok && i + 4 <= re) {
      ld4<IN>(x + i, p);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = i + k < re;
        p[k] = in ? ld1(x + (in ? i + k : cb)) : -INFINITY;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p[k] = softmax_prob(p[k], t, M, Sum);
      for (int q = 0; q < nrej; ++q)
        if (srej[q] == i + k) p[k] = 0.f;
    }
    const float local = ((p[0] + p[1]) + p[2]) + p[3];
    float incl = local;                             // inclusive scan over the wave's lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    const float before = __shfl_up(incl, 1, 64);
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    float c = run;
    for (int w = 0; w < wid; ++w) c += wtot[w];
    if (lane > 0) c += before;
    int found = 0x7fffffff, nz = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c += p[k];
      if (p[k] > 0.f) {
        nz = static_cast<int>(i + k);
        if (c > target && found == 0x7fffffff) found = static_cast<int>(i + k);
      }
    }
    if (found != 0x7fffffff) atomicMin(&sFound, found);
    if (nz >= 0) atomicMax(&sLast, nz);
    run = (((run + wtot[0]) + wtot[1]) + wtot[2]) + wtot[3];
    __syncthreads();
    if (sFound != 0x7fffffff) break;                // (uniform: read behind the barrier, next written behind the next one)
  }
  if (tid == 0) bonus_token[b] = sFound != 0x7fffffff ? sFound : (sLast >= 0 ? sLast : 0);
}

// ---- tree tables ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTaThreads) void build_verify_tree_kernel(const int32_t* __restrict__ parents, const int32_t* __restrict__ seq_lens,
                                                                       int B, int nd, uint8_t* __restrict__ mask, int64_t mask_bytes,
                                                                       int64_t* __restrict__ mask_indptr, int64_t* __restrict__ positions,
                                                                       int32_t* __restrict__ next_token, int32_t* __restrict__ next_sibling) {
  __shared__ int sPar[kTaMaxNodes];
  __shared__ u64 sAnc[kTaMaxNodes];
  __shared__ long long sred[kTaWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t base = static_cast<int64_t>(b) * nd;
  // where the request's block starts: nd * (the earlier requests' kv + nd)
  long long s = 0;
  for (int i = tid; i < b; i += kTaThreads) s += seq_lens[i] > 0 ? seq_lens[i] : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) sred[wid] = s;
  if (tid < nd) {
    const int p = parents[base + tid];
    sPar[tid] = (p >= 0 && p < tid) ? p : -1;       // (a parent has a lower index: every walk up ends)
  }
  __syncthreads();
  s = (sred[0] + sred[1]) + (sred[2] + sred[3]);
  const int kv = seq_lens[b] > 0 ? seq_lens[b] : 0;
  const int64_t L = static_cast<int64_t>(kv) + nd;
  int64_t off = static_cast<int64_t>(nd) * (s + static_cast<int64_t>(b) * nd);
  int64_t end = off + nd * L;
  if (tid < nd) {
    u64 anc = 0ull;
    for (int a = tid; a >= 0; a = sPar[a]) anc |= 1ull << a;
    sAnc[tid] = anc;
    if (blockIdx.y == 0) {
      positions[base + tid] = kv + __popcll(anc) - 1;
      int nt = -1, sb = -1;
      for (int i = nd - 1; i > tid; --i) {
        if (sPar[i] == tid) nt = i;
        if (sPar[tid] >= 0 && sPar[i] == sPar[tid]) sb = i;
      }
      next_token[base + tid] = nt;
      next_sibling[base + tid] = sb;
    }
  }
  if (blockIdx.y == 0 && tid == 0) {
    mask_indptr[b] = off;
    if (b == B - 1) mask_indptr[B] = end;
  }
  __syncthreads();

  // the block as a byte range of the flat mask, in 16-byte pieces of the mask itself; never past the caller's buffer
  off = off < mask_bytes ? off : mask_bytes;
  end = end < mask_bytes ? end : mask_bytes;
  const int64_t c1 = (end + 15) >> 4;
  for (int64_t c = (off >> 4) + static_cast<int64_t>(blockIdx.y) * kTaThreads + tid; c < c1; c += static_cast<int64_t>(gridDim.y) * kTaThreads) {
    const int64_t g = c << 4;
    const int64_t lo = g > off ? g : off, hi = g + 16 < end ? g + 16 : end;
    const int64_t rel = lo - off;
    int row = static_cast<int>(rel / L);
    int64_t col = rel - row * L;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (g + i >= lo && g + i < hi) {
        const uint32_t bit = col < kv ? 1u : static_cast<uint32_t>((sAnc[row] >> (col - kv)) & 1ull);
        w[i >> 2] |= bit << (8 * (i & 3));
        if (++col == L) { col = 0; ++row; }
      }
    }
    if (lo == g && hi == g + 16) {
      U4 q;
      q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
      st16(mask + g, q);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (g + i >= lo && g + i < hi) mask[g + i] = static_cast<uint8_t>((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
    }
  }
}

}  // namespace

extern "C" {

int sgl_amd_tree_accept_max_nodes(void) { return kTaMaxNodes; }

int sgl_amd_build_verify_tree(const int32_t* parents, const int32_t* seq_lens, int64_t batch, int nd, void* mask, int64_t mask_bytes,
                              int64_t* mask_indptr, int64_t* positions, int32_t* next_token, int32_t* next_sibling, void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(nd >= 1 && nd <= kTaMaxNodes, "build_verify_tree: 1 <= nodes <= %d (sgl_amd_tree_accept_max_nodes), got %d", kTaMaxNodes, nd);
  SGL_CHECK_ARG(batch >= 1 && batch * nd <= 65535, "build_verify_tree: 1 <= batch, batch * nodes <= 65535");
  SGL_CHECK_ARG(parents != nullptr && seq_lens != nullptr && mask_indptr != nullptr && positions != nullptr && next_token != nullptr &&
                    next_sibling != nullptr, "build_verify_tree: parents, seq_lens and the four tables are required");
  SGL_CHECK_ARG(mask != nullptr && mask_bytes >= 0 && (reinterpret_cast<uintptr_t>(mask) & 15) == 0,
                "build_verify_tree: needs a 16-byte aligned mask buffer");
  int yb = static_cast<int>(512 / batch);
  yb = yb < 1 ? 1 : (yb > 16 ? 16 : yb);
  hipLaunchKernelGGL(build_verify_tree_kernel, dim3(static_cast<unsigned>(batch), yb), dim3(kTaThreads), 0, as_stream(stream), parents, seq_lens,
                     static_cast<int>(batch), nd, static_cast<uint8_t*>(mask), mask_bytes, mask_indptr, positions, next_token, next_sibling);
  SGL_CHECK_LAUNCH("build_verify_tree");
  return 0;
}

int64_t sgl_amd_tree_accept_workspace_bytes(int64_t batch, int nd, int num_splits, int final_splits) {
  return tree_accept_ws_bytes(batch, nd, num_splits, final_splits);
}

int sgl_amd_tree_accept_from_logits(const void* logits, int logits_is_bf16, int64_t row_stride, const float* temperatures,
                                    const void* candidates, int candidates_is_int64, const int32_t* next_token,
                                    const int32_t* next_sibling, const float* uniform, const float* uniform_final, float threshold_single,
                                    float threshold_acc, int64_t batch, int nd, int64_t vocab, int32_t* accept_index, int32_t* accept_len,
                                    int32_t* bonus_token, int32_t* last_node, int num_splits, int final_splits, void* workspace,
                                    void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(nd >= 1 && nd <= kTaMaxNodes, "tree_accept_from_logits: 1 <= nodes <= %d (sgl_amd_tree_accept_max_nodes), got %d", kTaMaxNodes, nd);
  SGL_CHECK_ARG(batch >= 1 && batch * nd <= 65535, "tree_accept_from_logits: 1 <= batch, batch * nodes <= 65535");
  SGL_CHECK_ARG(vocab >= 1 && vocab <= 0x7fffffffLL, "tree_accept_from_logits: vocab must be in [1, 2^31)");
  SGL_CHECK_ARG(logits != nullptr && row_stride >= vocab, "tree_accept_from_logits: logits [batch * nodes, vocab] with row stride >= vocab");
  SGL_CHECK_ARG(candidates != nullptr && next_token != nullptr && next_sibling != nullptr, "tree_accept_from_logits: candidates and the tree tables are required");
  SGL_CHECK_ARG(accept_index != nullptr && accept_len != nullptr && bonus_token != nullptr && last_node != nullptr,
                "tree_accept_from_logits: the four outputs are required");
  SGL_CHECK_ARG(temperatures == nullptr || (uniform != nullptr && uniform_final != nullptr),
                "tree_accept_from_logits: sampled requests need uniform [batch, nodes] and uniform_final [batch]");
  SGL_CHECK_ARG(threshold_single > 0.f && threshold_acc > 0.f, "tree_accept_from_logits: thresholds must be positive");
  SGL_CHECK_ARG(num_splits >= 1 && num_splits <= kTaMaxSplits && final_splits >= 1 && final_splits <= kTaMaxSplits,
                "tree_accept_from_logits: 1..%d column ranges", kTaMaxSplits);
  SGL_CHECK_ARG(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "tree_accept_from_logits: needs an 8-byte aligned workspace");
  const TreeAcceptWs ws = tree_accept_ws_view(workspace, batch, nd, num_splits, final_splits);
  const dim3 rgrid(num_splits, static_cast<unsigned>(batch * nd)), fgrid(final_splits, static_cast<unsigned>(batch));
  const unsigned nb = static_cast<unsigned>(batch);
#define SGL_LAUNCH_TREE_ACCEPT(IN_)                                                                                                          \
  do {                                                                                                                                       \
    const IN_* x = static_cast<const IN_*>(logits);                                                                                          \
    hipLaunchKernelGGL(tree_accept_ranges_kernel<IN_>, rgrid, dim3(kTaThreads), 0, as_stream(stream), x, row_stride, temperatures, nd, vocab, \
                       num_splits, ws);                                                                                                      \
    hipLaunchKernelGGL(tree_accept_walk_kernel<IN_>, dim3(nb), dim3(kTaMaxNodes), 0, as_stream(stream), x, row_stride, temperatures,          \
                       candidates, candidates_is_int64, next_token, next_sibling, uniform, threshold_single, threshold_acc, nd, vocab,       \
                       num_splits, accept_index, accept_len, bonus_token, last_node, ws);                                                    \
    if (temperatures != nullptr) { /* without temperatures every request is greedy: finished by the walk */                                 \
      hipLaunchKernelGGL(tree_accept_final_kernel<IN_>, fgrid, dim3(kTaThreads), 0, as_stream(stream), x, row_stride, temperatures,          \
                         last_node, nd, vocab, final_splits, ws);                                                                            \
      hipLaunchKernelGGL(tree_accept_pick_kernel<IN_>, dim3(nb), dim3(kTaThreads), 0, as_stream(stream), x, row_stride, temperatures,        \
                         last_node, uniform_final, nd, vocab, final_splits, bonus_token, ws);                                                \
    }                                                                                                                                        \
  } while (0)
  if (logits_is_bf16) SGL_LAUNCH_TREE_ACCEPT(uint16_t);
  else SGL_LAUNCH_TREE_ACCEPT(float);
#undef SGL_LAUNCH_TREE_ACCEPT
  SGL_CHECK_LAUNCH("tree_accept_from_logits");
  return 0;
}

}  // extern "C"
