// The draft side of a speculative step for gfx950 without a draft model: the n-gram ("prompt lookup") drafter.  The request's last
// max_n tokens are looked up in its own history (prompt + output, an int32 row of a device-side token table) and what followed the
// earlier occurrences becomes a draft tree in the layout build_verify_tree / tree_accept_from_logits take.
//
// Serves what the reference offers as --speculative-algorithm NGRAM, with the history on the device: a host-side search pays a
// device-to-host copy of the new tokens and a host search per step before it can draft.
//
// The rule (integer work, reproduced exactly; include/sglang_amd.h states it in full): an end position p in [lo, L - 1) is a hit of
// length m = the number of tokens h[p], h[p - 1], ... that equal h[L - 1], h[L - 2], ... (at most max_n), kept if m >= min_n.  The
// `branches` best hits by (m, p) -- longest first, then the most recent -- are inserted into a trie rooted at node 0 = h[L - 1], each
// with its continuation h[p + 1 .. p + depth]; the tree is padded to nd nodes with a chain below the last node created.
//
// ngram_scan   grid (splits, B), 256 threads.  Split s owns a run of whole 1024-token tiles of the request's searched range (computed
//           on the device from lens[b]: the grid never depends on the lengths).  A tile goes through LDS: one 16-byte load per thread
//           (tile starts are multiples of 1024 tokens, rows are 16-byte aligned) plus an 8-token halo in front of it for the backward
//           compare, so a position never looks at global memory twice.  The suffix sits in 8 registers; thread t scores positions
//           t, t + 256, t + 512, t + 768 of the tile (adjacent lanes, adjacent LDS words).  A hit is one ordered 32-bit key, m << 27 | p:
//           unique per position, so nothing depends on arrival order.  Hits above the workgroup's current cut go to an LDS list (one
//           LDS atomic per wave and slot, offsets by ballot); the list holds a tile's worth of hits plus the 8 kept, and is pruned to
//           the exact top `branches` (eight block-wide maxima) whenever it holds more than 8 after a tile: hits are never dropped, the
//           worst case -- every position hits -- only prunes once per tile.  The workgroup leaves its top keys as 8 words, zero = none.
// ngram_tree   grid (B), one wave.  The lanes merge the splits x 8 keys to the top `branches` (wave maxima, key order), then build the
//           trie with lane j holding node j's (parent, token): a continuation is loaded once, one token per lane; finding a child is
//           one ballot of parent == cur && token == tok below the node count, a new node a write by lane `count`.  Then the padding.
// ngram_commit grid (B), one wave.  After acceptance: the accepted draft tokens and the bonus token go behind the request's history
//           and lens[b] grows, on the device: the next step's draft does not wait for the host.
// Only enqueues on the given stream (hipGraph-capturable), no hidden state, caller-owned workspace with no initial state.
#include "common.hpp"
#include "sglang_amd.h"

using namespace sgl_amd;

namespace {

constexpr int kNgMaxNgram = 8;
constexpr int kNgMaxBranches = 8;                   // the words a split leaves
constexpr int kNgMaxNodes = 64;                     // sgl_amd_tree_accept_max_nodes(): a lane per node
constexpr int kNgMaxSplits = 64;
constexpr int kNgThreads = 256;
constexpr int kNgWaves = kNgThreads / kWave;
constexpr int kNgTile = 4 * kNgThreads;             // 1024 tokens: one 16-byte load per thread
constexpr int kNgPerThread = kNgTile / kNgThreads;  // positions a thread scores per tile
constexpr int kNgHalo = 8;                          // tokens in front of a tile (>= kNgMaxNgram - 1, two vectors)
constexpr int kNgCap = kNgTile + kNgMaxBranches;    // the hit list: the kept keys + every position of one tile
constexpr int kNgCapPerThread = (kNgCap + kNgThreads - 1) / kNgThreads;
constexpr int kNgPosBits = 27;                      // key = m << 27 | p: table width < 2^27, m <= 8
constexpr uint32_t kNgPosMask = (1u << kNgPosBits) - 1u;

static_assert(kNgHalo % 4 == 0 && kNgHalo >= kNgMaxNgram - 1 && kNgHalo / 4 <= kNgThreads, "the halo is whole vectors in front of the tile");
static_assert(kNgMaxSplits * kNgMaxBranches <= kNgMaxBranches * kWave, "the merge holds splits x 8 keys in 8 registers per lane");

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// the request's history length: lens[b] held to [1, width] (the entry point's contract; nothing is ever read outside the row)
__device__ __forceinline__ int history_len(const int32_t* lens, int b, int width) {
  const int L = lens[b];
  return L < 1 ? 1 : (L > width ? width : L);
}

// The exact top `branches` of list[0 .. count) by a kNgThreads workgroup, in key order, zero where there are fewer: every thread
// returns the same eight words.  Keys are unique and non-zero.  `red` = kNgWaves words of LDS.  Ends behind a barrier.
__device__ __forceinline__ void block_top_keys(const uint32_t* list, int count, int branches, uint32_t* red, uint32_t (&win)[kNgMaxBranches]) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t mine[kNgCapPerThread];
#pragma unroll
  for (int i = 0; i < kNgCapPerThread; ++i) {
    const int idx = tid + i * kNgThreads;
    mine[i] = (idx < count && idx < kNgCap) ? list[idx] : 0u;
  }
#pragma unroll
  for (int r = 0; r < kNgMaxBranches; ++r) {
    win[r] = 0u;
    if (r < branches) {                             // (uniform)
      uint32_t m = 0u;
#pragma unroll
      for (int i = 0; i < kNgCapPerThread; ++i) m = mine[i] > m ? mine[i] : m;
      m = wave_max_u32(m);
      if (lane == 0) red[wid] = m;
      __syncthreads();
      m = red[0];
#pragma unroll
      for (int w = 1; w < kNgWaves; ++w) m = red[w] > m ? red[w] : m;
      __syncthreads();
      win[r] = m;
#pragma unroll
      for (int i = 0; i < kNgCapPerThread; ++i)
        if (mine[i] == m) mine[i] = 0u;
    }
  }
}

__global__ __launch_bounds__(kNgThreads) void ngram_scan_kernel(const int32_t* __restrict__ token_table, int64_t row_stride,
                                                                const int64_t* __restrict__ req_pool_indices,
                                                                const int32_t* __restrict__ lens, int max_n, int min_n, int branches,
                                                                int window, uint32_t* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) int32_t sTok[kNgHalo + kNgTile];
  __shared__ uint32_t sList[kNgCap];
  __shared__ uint32_t sRed[kNgWaves];
  __shared__ int sCount;
  const int s = blockIdx.x, S = gridDim.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int width = static_cast<int>(row_stride);
  const int L = history_len(lens, b, width);
  const int32_t* row = token_table + req_pool_indices[b] * row_stride;
  uint32_t* out = ws + (static_cast<int64_t>(b) * S + s) * kNgMaxBranches;

  // end positions [lo, hi) of the request, in whole tiles [t0, t1); this split's run of them
  const int hi = L - 1;
  const int lo = window > 0 ? (hi - window > 0 ? hi - window : 0) : 0;
  const int t0 = lo / kNgTile, t1 = (hi + kNgTile - 1) / kNgTile;
  const int per = (t1 - t0 + S - 1) / S;
  const int tb = t0 + s * per;
  const int te = tb + per < t1 ? tb + per : t1;
  if (hi <= lo || tb >= te) {                       // (uniform) nothing to search here: the words still have to say so
    if (tid < kNgMaxBranches) out[tid] = 0u;
    return;
  }

  int32_t suf[kNgMaxNgram];                         // suf[i] = h[L - 1 - i]
#pragma unroll
  for (int i = 0; i < kNgMaxNgram; ++i) suf[i] = (i < max_n && L - 1 - i >= 0) ? row[L - 1 - i] : 0;
  if (tid == 0) sCount = 0;
  uint32_t cut = 0u;                                // only keys above it can still reach the top `branches`

  for (int t = tb; t < te; ++t) {
    const int g = t * kNgTile;                      // the tile's first token: a multiple of 1024
    __syncthreads();                                // the last tile's scores (and sCount = 0 / the pruned list) are done
    {
      const int i = g + 4 * tid;                    // a vector with a token of the history in it lies inside the row: width % 4 == 0
      if (i < L) st16(&sTok[kNgHalo + 4 * tid], ld16(row + i));
      if (tid < kNgHalo / 4) {
        U4 h = {0u, 0u, 0u, 0u};
        if (g > 0) h = ld16(row + g - kNgHalo + 4 * tid);
        st16(&sTok[4 * tid], h);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kNgPerThread; ++k) {
      const int off = tid + k * kNgThreads;
      const int p = g + off;
      uint32_t key = 0u;
      if (p >= lo && p < hi) {
        int m = 0;
#pragma unroll
        for (int i = 0; i < kNgMaxNgram; ++i) {
          const bool eq = m == i && i < max_n && p - i >= 0 && sTok[kNgHalo + off - i] == suf[i];
          m += eq ? 1 : 0;
        }
        if (m >= min_n) key = (static_cast<uint32_t>(m) << kNgPosBits) | static_cast<uint32_t>(p);
      }
      const bool hit = key > cut;                   // (m >= min_n >= 1: a hit's key is never 0)
      const unsigned long long mask = __ballot(hit);
      if (mask != 0ull) {                           // (wave-uniform) one LDS atomic per wave: the order inside the list is free
        const int leader = __ffsll(mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&sCount, __popcll(mask));
        base = __shfl(base, leader, 64);
        // at most kNgTile hits per tile on top of the <= kNgMaxBranches the list starts a tile with: base + rank < kNgCap
        const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && slot < kNgCap) sList[slot] = key;
      }
    }
    __syncthreads();
    const int count = sCount;
    if (count > kNgMaxBranches) {                   // (uniform) prune to the exact top before the next tile can fill the list
      uint32_t win[kNgMaxBranches];
      block_top_keys(sList, count, branches, sRed, win);
      if (tid < kNgMaxBranches) sList[tid] = win[tid];
      if (tid == 0) sCount = branches;              // (count > 8 >= branches: all of them are real)
      cut = win[0];
#pragma unroll
      for (int r = 1; r < kNgMaxBranches; ++r)
        if (r < branches) cut = win[r];
    }
  }
  __syncthreads();
  uint32_t win[kNgMaxBranches];
  block_top_keys(sList, sCount, branches, sRed, win);
  if (tid < kNgMaxBranches) out[tid] = win[tid];
}

__global__ __launch_bounds__(kWave) void ngram_tree_kernel(const int32_t* __restrict__ token_table, int64_t row_stride,
                                                           const int64_t* __restrict__ req_pool_indices, const int32_t* __restrict__ lens,
                                                           int nd, int branches, int depth, int64_t pad_token, int S,
                                                           const uint32_t* __restrict__ ws, int64_t* __restrict__ tree_tokens,
                                                           int32_t* __restrict__ parents, int32_t* __restrict__ num_real) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int L = history_len(lens, b, static_cast<int>(row_stride));
  const int32_t* row = token_table + req_pool_indices[b] * row_stride;

  // the top `branches` of the splits' keys, in key order (the same words in every lane)
  const uint32_t* keys = ws + static_cast<int64_t>(b) * S * kNgMaxBranches;
  const int nkeys = S * kNgMaxBranches;
  uint32_t mine[kNgMaxBranches];
#pragma unroll
  for (int i = 0; i < kNgMaxBranches; ++i) {
    const int idx = lane + i * kWave;
    mine[i] = idx < nkeys ? keys[idx] : 0u;
  }
  uint32_t win[kNgMaxBranches];
#pragma unroll
  for (int r = 0; r < kNgMaxBranches; ++r) {
    win[r] = 0u;
    if (r < branches) {
      uint32_t m = 0u;
#pragma unroll
      for (int i = 0; i < kNgMaxBranches; ++i) m = mine[i] > m ? mine[i] : m;
      m = wave_max_u32(m);
      win[r] = m;
#pragma unroll
      for (int i = 0; i < kNgMaxBranches; ++i)
        if (mine[i] == m) mine[i] = 0u;
    }
  }

  // the trie: lane j = node j
  int par = -1;
  int64_t tok = lane == 0 ? static_cast<int64_t>(row[L - 1]) : pad_token;
  int count = 1;
#pragma unroll
  for (int r = 0; r < kNgMaxBranches; ++r) {
    if (win[r] == 0u) continue;                     // (uniform; the keys are in order: nothing real follows a zero)
    const int p = static_cast<int>(win[r] & kNgPosMask);                  // p < L - 1
    const int clen = depth < L - 1 - p ? depth : L - 1 - p;               // the continuation h[p + 1 .. p + clen], clen <= 63
    const int32_t cont = lane < clen ? row[p + 1 + lane] : 0;
    int cur = 0;
    for (int t = 0; t < clen; ++t) {
      const int32_t tk = __shfl(cont, t, 64);
      const unsigned long long found = __ballot(lane < count && par == cur && tok == static_cast<int64_t>(tk));
      int nxt;
      if (found != 0ull) {
        nxt = __ffsll(found) - 1;
      } else {
        if (count == nd) break;                     // the node budget cuts this continuation (a later one may still walk the trie)
        if (lane == count) {
          tok = tk;
          par = cur;
        }
        nxt = count++;
      }
      cur = nxt;
    }
  }
  // static shape: a chain of pad tokens below the last node created (a leaf: no sibling can carry the same token)
  if (lane >= count) {
    tok = pad_token;
    par = lane - 1;
  }
  if (lane < nd) {
    tree_tokens[static_cast<int64_t>(b) * nd + lane] = tok;
    parents[static_cast<int64_t>(b) * nd + lane] = par;
  }
  if (lane == 0) num_real[b] = count;
}

__global__ __launch_bounds__(kWave) void ngram_commit_kernel(int32_t* __restrict__ token_table, int64_t row_stride,
                                                             const int64_t* __restrict__ req_pool_indices, int32_t* __restrict__ lens,
                                                             const void* __restrict__ candidates, int cand_is_int64,
                                                             const int32_t* __restrict__ accept_index, const int32_t* __restrict__ accept_len,
                                                             const int32_t* __restrict__ bonus_token, int nd) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int width = static_cast<int>(row_stride);
  int L = lens[b];
  L = L < 0 ? 0 : (L > width ? width : L);
  int n = accept_len[b];
  n = n < 0 ? 0 : (n > nd - 1 ? nd - 1 : n);
  int32_t* row = token_table + req_pool_indices[b] * row_stride;
  const int64_t base = static_cast<int64_t>(b) * nd;
  if (lane <= n && L + lane < width) {              // lane i < n: the i-th accepted draft token; lane n: the bonus token
    int32_t t;
    if (lane == n) {
      t = bonus_token[b];
    } else {
      int node = accept_index[base + lane + 1];
      node = node < 0 ? 0 : (node > nd - 1 ? nd - 1 : node);
      t = cand_is_int64 ? static_cast<int32_t>(static_cast<const int64_t*>(candidates)[base + node])
                        : static_cast<const int32_t*>(candidates)[base + node];
    }
    row[L + lane] = t;
  }
  if (lane == 0) lens[b] = L + n + 1 < width ? L + n + 1 : width;
}

}  // namespace

extern "C" {

int sgl_amd_ngram_draft_max_ngram(void) { return kNgMaxNgram; }

int sgl_amd_ngram_draft_tile(void) { return kNgTile; }

int64_t sgl_amd_ngram_draft_workspace_bytes(int64_t batch, int num_splits) {
  return batch * num_splits * kNgMaxBranches * static_cast<int64_t>(sizeof(uint32_t));
}

int sgl_amd_ngram_draft_tree(const int32_t* token_table, int64_t table_row_stride, const int64_t* req_pool_indices, const int32_t* lens,
                             int64_t batch, int nd, int max_ngram, int min_ngram, int branches, int depth, int window, int64_t pad_token,
                             int64_t* tree_tokens, int32_t* parents, int32_t* num_real, int num_splits, void* workspace, void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(nd >= 1 && nd <= kNgMaxNodes, "ngram_draft_tree: 1 <= nodes <= %d (sgl_amd_tree_accept_max_nodes), got %d", kNgMaxNodes, nd);
  SGL_CHECK_ARG(max_ngram >= 1 && max_ngram <= kNgMaxNgram, "ngram_draft_tree: 1 <= max_ngram <= %d (sgl_amd_ngram_draft_max_ngram), got %d",
                kNgMaxNgram, max_ngram);
  SGL_CHECK_ARG(min_ngram >= 1 && min_ngram <= max_ngram, "ngram_draft_tree: 1 <= min_ngram <= max_ngram, got %d and %d", min_ngram, max_ngram);
  SGL_CHECK_ARG(branches >= 1 && branches <= kNgMaxBranches, "ngram_draft_tree: 1 <= branches <= %d, got %d", kNgMaxBranches, branches);
  SGL_CHECK_ARG(depth >= 1 && depth <= kNgMaxNodes - 1, "ngram_draft_tree: 1 <= depth <= %d, got %d", kNgMaxNodes - 1, depth);
  SGL_CHECK_ARG(window >= 0, "ngram_draft_tree: window >= 0 (0 = the whole history), got %d", window);
  SGL_CHECK_ARG(num_splits >= 1 && num_splits <= kNgMaxSplits, "ngram_draft_tree: num_splits must be in 1..%d, got %d", kNgMaxSplits, num_splits);
  SGL_CHECK_ARG(batch >= 1 && batch <= 65535, "ngram_draft_tree: 1 <= batch <= 65535");
  SGL_CHECK_ARG(table_row_stride >= 4 && table_row_stride % 4 == 0 && table_row_stride < (1ll << kNgPosBits),
                "ngram_draft_tree: the table's row stride (= its width) must be a multiple of 4 tokens (16-byte rows) in [4, 2^27), got %lld",
                static_cast<long long>(table_row_stride));
  SGL_CHECK_ARG(token_table != nullptr && (reinterpret_cast<uintptr_t>(token_table) & 15) == 0, "ngram_draft_tree: needs a 16-byte aligned token table");
  SGL_CHECK_ARG(req_pool_indices != nullptr && lens != nullptr && tree_tokens != nullptr && parents != nullptr && num_real != nullptr,
                "ngram_draft_tree: req_pool_indices, lens and the three outputs are required");
  SGL_CHECK_ARG(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "ngram_draft_tree: needs a 4-byte aligned workspace");
  const unsigned nb = static_cast<unsigned>(batch);
  hipLaunchKernelGGL(ngram_scan_kernel, dim3(num_splits, nb), dim3(kNgThreads), 0, as_stream(stream), token_table, table_row_stride,
                     req_pool_indices, lens, max_ngram, min_ngram, branches, window, static_cast<uint32_t*>(workspace));
  hipLaunchKernelGGL(ngram_tree_kernel, dim3(nb), dim3(kWave), 0, as_stream(stream), token_table, table_row_stride, req_pool_indices, lens, nd,
                     branches, depth, pad_token, num_splits, static_cast<const uint32_t*>(workspace), tree_tokens, parents, num_real);
  SGL_CHECK_LAUNCH("ngram_draft_tree");
  return 0;
}

int sgl_amd_ngram_commit(int32_t* token_table, int64_t table_row_stride, const int64_t* req_pool_indices, int32_t* lens,
                         const void* candidates, int candidates_is_int64, const int32_t* accept_index, const int32_t* accept_len,
                         const int32_t* bonus_token, int64_t batch, int nd, void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(nd >= 1 && nd <= kNgMaxNodes, "ngram_commit: 1 <= nodes <= %d (sgl_amd_tree_accept_max_nodes), got %d", kNgMaxNodes, nd);
  SGL_CHECK_ARG(batch >= 1 && batch <= 65535, "ngram_commit: 1 <= batch <= 65535");
  SGL_CHECK_ARG(table_row_stride >= 4 && table_row_stride % 4 == 0 && table_row_stride < (1ll << kNgPosBits),
                "ngram_commit: the table's row stride (= its width) must be a multiple of 4 tokens in [4, 2^27), got %lld",
                static_cast<long long>(table_row_stride));
  SGL_CHECK_ARG(token_table != nullptr && req_pool_indices != nullptr && lens != nullptr, "ngram_commit: the token table, req_pool_indices and lens are required");
  SGL_CHECK_ARG(candidates != nullptr && accept_index != nullptr && accept_len != nullptr && bonus_token != nullptr,
                "ngram_commit: candidates, accept_index, accept_len and bonus_token are required");
  hipLaunchKernelGGL(ngram_commit_kernel, dim3(static_cast<unsigned>(batch)), dim3(kWave), 0, as_stream(stream), token_table, table_row_stride,
                     req_pool_indices, lens, candidates, candidates_is_int64, accept_index, accept_len, bonus_token, nd);
  SGL_CHECK_LAUNCH("ngram_commit");
  return 0;
}

}  // extern "C"
