// Split-KV short-extend ("tree verify") attention over the paged token->KV pool, gfx950 MFMA.
//
// Replaces, for the TARGET_VERIFY step of speculative decoding (reference, /root/reference/python/sglang):
//   srt/layers/attention/triton_backend.py:860-919 (the verify call), kernels/ops/attention/extend_attention.py
//   _fwd_kernel with USE_CUSTOM_MASK and skip_prefix_custom_mask = 1.
// Every request extends by a handful of tokens (e_b) over its whole context; the tree mask decides among the new tokens
// only.  The prefill kernel (extend_attention.hip) gives such a batch one workgroup per (request, kv head) that walks the
// whole context alone.  This kernel is shaped like a decode kernel instead:
//
//   * grid = (split, kv head, request), fixed by the host.  Split s of request b owns a contiguous run of whole
//     64-token tiles of [0, seq_lens[b]), computed here from the step's own lengths: a captured graph follows the lengths.
//     A split without tiles writes the neutral partial (m = -inf, l = 0) and leaves; the merge skips it.
//   * a row is a (query token, q head of the GQA group) pair; the 16 * MT <= 64 rows of ONE (request, kv head) are held
//     by EVERY wave (Q^T fragments in registers for the whole split).  The four waves of the workgroup split the KV
//     TOKENS: a tile is two 32-token units, wave w takes units w, w + 4, ... of the split's run, with a private running
//     (m, l, O) and no workgroup barrier inside the loop.  Few rows keep all four waves busy this way (16 rows on
//     four waves would idle three of them under a row split), and each K/V row is read from HBM once per launch, per kv
//     head.
//   * K never touches LDS: the A operand of S^T = K . Q^T (v_mfma_f32_16x16x32_bf16) is 8 consecutive head dims of one
//     token per lane, a plain 16-byte row read from the pool.  V needs token-major -> d-major: it goes through a
//     wave-private LDS image ([16 head dims][32 tokens] sub-images of 32-byte rows) and comes back through
//     ds_read_b64_tr_b16 as the A operand of O^T = V^T . P^T, in the token order of the P^T fragments built from the
//     S^T accumulators (the layout of extend_attention_dbuf_kernel).  The image is private to the wave, LDS operations of
//     a wave complete in order, so write -> read -> write needs no barrier.
//   * the rows of unit u + 4 are requested right after the S^T products of unit u consumed the K registers and the V
//     registers went to LDS: they travel under the softmax and the PV products; slot ids run one unit further ahead.
//   * only units that overlap [prefix_lens[b], seq_lens[b]) take the masked path (wave-uniform); all others run
//     without a compare.  Mask bytes under the prefix columns are never read.
//   * the softmax scale is applied to the fp32 scores (one fma inside the exp2 argument), not folded into the bf16 Q
//     fragments: re-rounding Q to bf16 would put a 2^-9 relative error on every score that the prefill kernel, whose
//     results this kernel must reproduce, does not have.
//   * end of split: (m, l) of the four waves meet in LDS, every wave rescales its O^T to the common maximum, and the
//     O^T tiles are summed in wave order through the (now free) V image, 16 rows at a time.  num_splits == 1 writes bf16
//     `out` directly; otherwise fp32 partials go to ws_acc / ws_ml and verify_merge_kernel sums them IN SPLIT ORDER.
//     The result is a fixed function of (inputs, num_splits).
//
// Every row must see at least one position (true of any tree mask: a draft token sees itself, and of the causal rule).
// A row that sees none gets zeros.
#include "common.hpp"
#include "sglang_amd.h"

using namespace sgl_amd;

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef short v4s16_t __attribute__((ext_vector_type(4)));

constexpr int kVfTile = 64;        // split granularity: tokens per tile
constexpr int kVfUnit = 32;        // tokens a wave multiplies at a time (one k-step of the PV product)
constexpr int kVfWaves = 4;
constexpr int kVfMaxRows = 64;     // (query token, q head of the group) pairs of one (request, kv head)
constexpr int kVfMaxSplits = 64;
constexpr float kNegBig = -1.0e30f;

__device__ __forceinline__ bf16x8_t as_frag(const U4& v) { return __builtin_bit_cast(bf16x8_t, v); }

struct VerifyParams {
  const uint16_t* q;                // [T, Hq, D]
  uint16_t* out;                    // [T, Hq, D]
  const uint16_t* k_cache;          // [slots, Hkv, D]
  const uint16_t* v_cache;
  const int32_t* req_to_token;      // [reqs, max_ctx]
  const int64_t* req_pool_indices;  // [B]
  const int32_t* seq_lens;          // [B] prefix + extend
  const int32_t* prefix_lens;       // [B]
  const int32_t* qo_indptr;         // [B + 1]
  int64_t q_stride, out_stride, kc_stride, vc_stride, r2t_stride;
  int num_q_heads, group, num_splits;
  float scale_log2;
  const uint8_t* custom_mask;       // NULL: causal among the new tokens
  const int64_t* mask_indptr;
  float* ws_acc;                    // [T, Hq, num_splits, D]
  float* ws_ml;                     // [T, Hq, num_splits, 2]  (m in log2 units, l)
};

// MT = 16-row M-tiles every wave carries (rows = 16 MT >= e_b * group).
template <int D, int MT>
__global__ __launch_bounds__(64 * kVfWaves, MT == 4 ? 1 : 2) void verify_attention_kernel(VerifyParams p) {
  constexpr int CPR = D / 8;                  // 16-byte chunks per KV row
  constexpr int KC = D / 32;                  // MFMA k-steps over the head dim
  constexpr int ND = D / 16;                  // 16-wide output tiles over the head dim
  constexpr int RPP = 64 / CPR;               // V rows one pass of the wave's 64 lanes covers
  constexpr int VL = kVfUnit / RPP;           // 16-byte V loads per lane per unit
  constexpr int kVSub = kVfUnit * 32 + 32;    // bytes of one 16-dim V sub-image + bank skew
  constexpr int kVWave = ND * kVSub;          // a wave's V image
  constexpr int kAccRow = D + 4;              // floats per row of the end-of-split sum image (+4: bank skew)
  constexpr int kVBytes = kVfWaves * kVWave, kAccBytes = kVfWaves * 16 * kAccRow * 4;
  __shared__ __attribute__((aligned(16))) unsigned char sm_raw[kVBytes > kAccBytes ? kVBytes : kAccBytes];
  __shared__ float sm_m[kVfWaves][kVfMaxRows], sm_l[kVfWaves][kVfMaxRows];

  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15;
  const int g = lane >> 4;
  const int S = p.num_splits;

  const int q_begin = p.qo_indptr[b];
  const int ext_len = p.qo_indptr[b + 1] - q_begin;
  if (ext_len <= 0) return;
  int n_rows = ext_len * p.group;
  if (n_rows > 16 * MT) n_rows = 16 * MT;     // (the host refuses such a launch; nothing is addressed beyond the rows held)
  const int kv_len = p.seq_lens[b];
  const int prefix = p.prefix_lens[b] < kv_len ? p.prefix_lens[b] : kv_len;

  // ---- this split's run of whole tiles -----------------------------------------------------------------------------
  const int n_tiles = kv_len > 0 ? (kv_len + kVfTile - 1) / kVfTile : 0;
  const int tps = (n_tiles + S - 1) / S;
  const int t0 = split * tps < n_tiles ? split * tps : n_tiles;
  const int t1 = t0 + tps < n_tiles ? t0 + tps : n_tiles;
  if (S > 1 && t0 >= t1) {
    for (int r = tid; r < n_rows; r += 64 * kVfWaves) {
      const int t = r / p.group, head = kvh * p.group + (r - t * p.group);
      float* ml = p.ws_ml + ((static_cast<int64_t>(q_begin + t) * p.num_q_heads + head) * S + split) * 2;
      ml[0] = -INFINITY;
      ml[1] = 0.f;
    }
    return;
  }

  // ---- this lane's rows (one per M-tile) and their Q^T fragments -----------------------------------------------------
  int row_tok[MT];
  bool row_ok[MT];
  U4 qf[MT][KC];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int r = mt * 16 + l15;
    const int t = r / p.group;
    row_tok[mt] = t;
    row_ok[mt] = r < n_rows;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      U4 v = U4{0u, 0u, 0u, 0u};
      if (row_ok[mt])
        v = ld16(p.q + static_cast<int64_t>(q_begin + t) * p.q_stride + (kvh * p.group + (r - t * p.group)) * D + kc * 32 + g * 8);
      qf[mt][kc] = v;
    }
  }

  f32x4_t ot[MT][ND];
  float m_run[MT], l_run[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    m_run[mt] = kNegBig;
    l_run[mt] = 0.f;
#pragma unroll
    for (int n = 0; n < ND; ++n) ot[mt][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // ---- row traffic: lane l < 32 of the wave fetches the slot id of token l of the unit, the row loads take theirs by
  // a lane exchange.  K: lane (l15, g) reads head dims [32 kc + 8 g, +8) of tokens l15 and 16 + l15.  V: lane
  // (st_r, st_c) reads chunk st_c of tokens st_r + RPP i.
  const int32_t* idx_base = p.req_to_token + p.req_pool_indices[b] * p.r2t_stride;
  const int u_end = (2 * t1 < (kv_len + kVfUnit - 1) / kVfUnit) ? 2 * t1 : (kv_len + kVfUnit - 1) / kVfUnit;
  auto load_idx = [&](int u) {
    int tok = u * kVfUnit + (lane & 31);
    if (tok > kv_len - 1) tok = kv_len - 1;       // rows past the end: the last row again, masked below
    return idx_base[tok];
  };
  const int st_c = lane % CPR, st_r = lane / CPR;
  const uint16_t* k_lane = p.k_cache + kvh * D + g * 8;
  const uint16_t* v_lane_src = p.v_cache + kvh * D + st_c * 8;
  U4 kst[2][KC], vst[VL];
  auto load_rows = [&](int my_idx) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int64_t slot = __shfl(my_idx, nt * 16 + l15, 64);
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) kst[nt][kc] = ld16(k_lane + slot * p.kc_stride + kc * 32);
    }
#pragma unroll
    for (int i = 0; i < VL; ++i) {
      const int64_t slot = __shfl(my_idx, st_r + RPP * i, 64);
      vst[i] = ld16(v_lane_src + slot * p.vc_stride);
    }
  };
  unsigned char* vimg = sm_raw + wid * kVWave;
  unsigned char* v_commit = vimg + (st_c >> 1) * kVSub + st_r * 32 + (st_c & 1) * 16;
  // V^T fragment reads: token rows 4 g + (l15 >> 2), 8-byte piece l15 & 3 of a sub-image
  const unsigned char* v_frag = vimg + (4 * g + (l15 >> 2)) * 32 + (l15 & 3) * 8;
  const uint8_t* cmask = p.custom_mask ? p.custom_mask + p.mask_indptr[b] : nullptr;

  int u = 2 * t0 + wid;
  int idx_next = 0;
  if (u < u_end) {
    const int idx = load_idx(u);
    if (u + kVfWaves < u_end) idx_next = load_idx(u + kVfWaves);
    load_rows(idx);
  }

  for (; u < u_end; u += kVfWaves) {
    const int kv0 = u * kVfUnit;

    // ---- S^T = K . Q^T: lane gets tokens 16 nt + 4 g + r of row l15 + 16 mt --------------------------------------
    f32x4_t st_acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) st_acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          st_acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(kst[nt][kc]), as_frag(qf[mt][kc]), st_acc[mt][nt], 0, 0, 0);

    // ---- V of this unit to the wave's image, then the next unit's rows are asked for ---------------------------
#pragma unroll
    for (int i = 0; i < VL; ++i) st16(v_commit + RPP * i * 32, vst[i]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (u + kVfWaves < u_end) {
      const int idx = idx_next;
      if (u + 2 * kVfWaves < u_end) idx_next = load_idx(u + 2 * kVfWaves);
      load_rows(idx);
    }

    // ---- online softmax (log2 units) ----------------------------------------------------------------------------
    const bool masked = kv0 + kVfUnit > prefix;          // wave-uniform: the unit reaches into the new tokens (or past the end)
    U4 pfrag[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float pv[2][4];
      float m_new, psum = 0.f;
      if (!masked) {
        float mx = st_acc[mt][0][0];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st_acc[mt][nt][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        m_new = fmaxf(m_run[mt], mx * p.scale_log2);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = fast_exp2(fmaf(st_acc[mt][nt][r], p.scale_log2, -m_new));
            pv[nt][r] = e;
            psum += e;
          }
      } else {
        float sv[2][4];
        float mx = kNegBig;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kvpos = kv0 + nt * 16 + g * 4 + r;
            bool on = row_ok[mt] && kvpos < kv_len;
            if (on && kvpos >= prefix)
              on = cmask != nullptr ? cmask[static_cast<int64_t>(row_tok[mt]) * kv_len + kvpos] != 0 : (kvpos - prefix <= row_tok[mt]);
            const float s = on ? st_acc[mt][nt][r] * p.scale_log2 : kNegBig;
            sv[nt][r] = s;
            mx = fmaxf(mx, s);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        m_new = fmaxf(m_run[mt], mx);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = (sv[nt][r] > 0.5f * kNegBig) ? fast_exp2(sv[nt][r] - m_new) : 0.f;   // masked scores add nothing, even while the maximum is the sentinel
            pv[nt][r] = e;
            psum += e;
          }
      }
      const float alpha = fast_exp2(m_run[mt] - m_new);
      m_run[mt] = m_new;
      l_run[mt] = l_run[mt] * alpha + psum;
      if (__ballot(alpha != 1.0f) != 0ull) {
#pragma unroll
        for (int n = 0; n < ND; ++n) ot[mt][n] *= alpha;
      }
      // P^T operand: k index 8 g + j  <->  token 4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4)
      pfrag[mt].x = pack_bf2(pv[0][0], pv[0][1]);
      pfrag[mt].y = pack_bf2(pv[0][2], pv[0][3]);
      pfrag[mt].z = pack_bf2(pv[1][0], pv[1][1]);
      pfrag[mt].w = pack_bf2(pv[1][2], pv[1][3]);
    }

    // ---- O^T += V^T . P^T ------------------------------------------------------------------------------------------
    typedef __attribute__((address_space(3))) v4s16_t* lds_v4_t;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
      const v4s16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(v_frag + n * kVSub));
      const v4s16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4_t)(v_frag + n * kVSub + 512));
      U4 vf;
      vf.x = __builtin_bit_cast(uint2, lo).x; vf.y = __builtin_bit_cast(uint2, lo).y;
      vf.z = __builtin_bit_cast(uint2, hi).x; vf.w = __builtin_bit_cast(uint2, hi).y;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        ot[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(vf), as_frag(pfrag[mt]), ot[mt][n], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the image is rewritten by the next unit
  }

  // ---- the four waves' (m, l) meet; every wave moves its O^T to the common maximum -----------------------------------
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    float l = l_run[mt];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (g == 0) {
      sm_m[wid][mt * 16 + l15] = m_run[mt];
      sm_l[wid][mt * 16 + l15] = l;
    }
  }
  __syncthreads();                                   // also: every wave is done with its V image
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = mt * 16 + l15;
    float M = sm_m[0][row];
#pragma unroll
    for (int w = 1; w < kVfWaves; ++w) M = fmaxf(M, sm_m[w][row]);
    const float f = fast_exp2(m_run[mt] - M);       // a wave that saw nothing: exp2(sentinel - M) = 0, or 1 on zeros
#pragma unroll
    for (int n = 0; n < ND; ++n) ot[mt][n] *= f;
  }

  // ---- sum over the waves in wave order, 16 rows at a time, through the freed image ----------------------------------
  float* acc_img = reinterpret_cast<float*>(sm_raw);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    if (mt > 0) __syncthreads();
    {
      float* dst = acc_img + (wid * 16 + l15) * kAccRow + g * 4;       // lane holds O^T[d = 16 n + 4 g + r][row l15]
#pragma unroll
      for (int n = 0; n < ND; ++n) *reinterpret_cast<f32x4_t*>(dst + n * 16) = ot[mt][n];
    }
    __syncthreads();
    for (int it = tid; it < 16 * (D / 4); it += 64 * kVfWaves) {
      const int row = it / (D / 4), c = it - row * (D / 4);
      const int r = mt * 16 + row;
      if (r >= n_rows) continue;
      float M = sm_m[0][r];
#pragma unroll
      for (int w = 1; w < kVfWaves; ++w) M = fmaxf(M, sm_m[w][r]);
      float L = 0.f;
      f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < kVfWaves; ++w) {
        L += sm_l[w][r] * fast_exp2(sm_m[w][r] - M);
        a += *reinterpret_cast<const f32x4_t*>(acc_img + (w * 16 + row) * kAccRow + c * 4);
      }
      const int t = r / p.group, head = kvh * p.group + (r - t * p.group);
      if (S == 1) {
        const float inv = L > 0.f ? 1.0f / L : 0.f;
        uint2 w2;
        w2.x = pack_bf2(a[0] * inv, a[1] * inv);
        w2.y = pack_bf2(a[2] * inv, a[3] * inv);
        *reinterpret_cast<uint2*>(p.out + static_cast<int64_t>(q_begin + t) * p.out_stride + head * D + c * 4) = w2;
      } else {
        const int64_t slot = (static_cast<int64_t>(q_begin + t) * p.num_q_heads + head) * S + split;
        *reinterpret_cast<f32x4_t*>(p.ws_acc + slot * D + c * 4) = a;
        if (c == 0) {
          p.ws_ml[slot * 2] = L > 0.f ? M : -INFINITY;
          p.ws_ml[slot * 2 + 1] = L;
        }
      }
    }
  }
}

// One (token, q head) per D / 4 lanes: the partials of its splits, summed in split order.
template <int D>
__global__ __launch_bounds__(256) void verify_merge_kernel(const float* __restrict__ ws_acc, const float* __restrict__ ws_ml,
                                                            uint16_t* __restrict__ out, int64_t out_stride, int num_q_heads, int S,
                                                            int64_t total_rows) {
  constexpr int LPR = D / 4;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * (256 / LPR) + threadIdx.x / LPR;
  const int c = threadIdx.x % LPR;
  if (row >= total_rows) return;
  const float* ml = ws_ml + row * S * 2;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, ml[2 * s]);
  float L = 0.f;
  f32x4_t a = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const float m = ml[2 * s];
    if (!(m > -INFINITY)) continue;                  // a split without tiles (or without a visible position): its acc is not read
    const float w = fast_exp2(m - M);
    L += w * ml[2 * s + 1];
    a += w * *reinterpret_cast<const f32x4_t*>(ws_acc + (row * S + s) * D + c * 4);
  }
  const float inv = L > 0.f ? 1.0f / L : 0.f;
  const int64_t t = row / num_q_heads;
  const int head = static_cast<int>(row - t * num_q_heads);
  uint2 w2;
  w2.x = pack_bf2(a[0] * inv, a[1] * inv);
  w2.y = pack_bf2(a[2] * inv, a[3] * inv);
  *reinterpret_cast<uint2*>(out + t * out_stride + head * D + c * 4) = w2;
}

}  // namespace

extern "C" {

int sgl_amd_verify_attention_max_rows(void) { return kVfMaxRows; }

int sgl_amd_verify_attention(const void* q, void* out, const void* k_cache, const void* v_cache, const int32_t* req_to_token,
                             int64_t req_to_token_stride, const int64_t* req_pool_indices, const int32_t* seq_lens,
                             const int32_t* prefix_lens, const int32_t* qo_indptr, int64_t batch, int64_t total_tokens,
                             int max_extend_len, int num_q_heads, int num_kv_heads, int head_dim, int64_t q_token_stride,
                             int64_t out_token_stride, int64_t k_cache_row_stride, int64_t v_cache_row_stride, float sm_scale,
                             const void* custom_mask, const int64_t* mask_indptr, int num_splits, float* ws_acc, float* ws_ml,
                             void* stream) {
  SGL_CLEAR_STALE_ERROR();
  SGL_CHECK_ARG(head_dim == 64 || head_dim == 128, "verify_attention: head_dim=%d not supported (64/128)", head_dim);
  SGL_CHECK_ARG(num_kv_heads > 0 && num_q_heads > 0 && num_q_heads % num_kv_heads == 0,
                "verify_attention: num_q_heads=%d not a multiple of num_kv_heads=%d", num_q_heads, num_kv_heads);
  const int group = num_q_heads / num_kv_heads;
  SGL_CHECK_ARG(max_extend_len >= 0 && static_cast<int64_t>(max_extend_len) * group <= kVfMaxRows,
                "verify_attention: max_extend_len %d x GQA group %d exceeds %d rows (sgl_amd_verify_attention_max_rows); use extend_attention",
                max_extend_len, group, kVfMaxRows);
  SGL_CHECK_ARG(num_splits >= 1 && num_splits <= kVfMaxSplits, "verify_attention: num_splits must be in [1, %d], got %d", kVfMaxSplits, num_splits);
  SGL_CHECK_ARG(num_splits == 1 || (ws_acc != nullptr && ws_ml != nullptr), "verify_attention: num_splits=%d needs the ws_acc / ws_ml workspaces", num_splits);
  SGL_CHECK_ARG((custom_mask == nullptr) == (mask_indptr == nullptr), "verify_attention: custom_mask and mask_indptr come together");
  SGL_CHECK_ARG(q_token_stride % 8 == 0 && out_token_stride % 4 == 0 && k_cache_row_stride % 8 == 0 && v_cache_row_stride % 8 == 0,
                "verify_attention: strides must keep 16-byte row alignment");
  SGL_CHECK_ARG(batch >= 0 && batch <= 65535 && num_kv_heads <= 65535, "verify_attention: grid too large");
  SGL_CHECK_ARG(total_tokens >= 0 && total_tokens * num_q_heads <= 0x7fffffffLL, "verify_attention: too many (token, head) rows");
  if (batch == 0 || max_extend_len == 0 || total_tokens == 0) return 0;
  SGL_CHECK_ARG(q != nullptr && out != nullptr && k_cache != nullptr && v_cache != nullptr && req_to_token != nullptr &&
                    req_pool_indices != nullptr && seq_lens != nullptr && prefix_lens != nullptr && qo_indptr != nullptr,
                "verify_attention: null tensor");
  VerifyParams p;
  p.q = static_cast<const uint16_t*>(q);
  p.out = static_cast<uint16_t*>(out);
  p.k_cache = static_cast<const uint16_t*>(k_cache);
  p.v_cache = static_cast<const uint16_t*>(v_cache);
  p.req_to_token = req_to_token;
  p.req_pool_indices = req_pool_indices;
  p.seq_lens = seq_lens;
  p.prefix_lens = prefix_lens;
  p.qo_indptr = qo_indptr;
  p.q_stride = q_token_stride;
  p.out_stride = out_token_stride;
  p.kc_stride = k_cache_row_stride;
  p.vc_stride = v_cache_row_stride;
  p.r2t_stride = req_to_token_stride;
  p.num_q_heads = num_q_heads;
  p.group = group;
  p.num_splits = num_splits;
  p.scale_log2 = sm_scale * 1.4426950408889634f;
  p.custom_mask = static_cast<const uint8_t*>(custom_mask);
  p.mask_indptr = mask_indptr;
  p.ws_acc = ws_acc;
  p.ws_ml = ws_ml;
  const int rows = max_extend_len * group;
  const dim3 grid(num_splits, num_kv_heads, static_cast<unsigned>(batch));
  hipStream_t st = as_stream(stream);
#define SGL_LAUNCH_VERIFY(D_)                                                                                       \
  do {                                                                                                              \
    if (rows <= 16) hipLaunchKernelGGL((verify_attention_kernel<D_, 1>), grid, dim3(64 * kVfWaves), 0, st, p);      \
    else if (rows <= 32) hipLaunchKernelGGL((verify_attention_kernel<D_, 2>), grid, dim3(64 * kVfWaves), 0, st, p); \
    else hipLaunchKernelGGL((verify_attention_kernel<D_, 4>), grid, dim3(64 * kVfWaves), 0, st, p);                 \
    if (num_splits > 1) {                                                                                           \
      const int64_t total_rows = total_tokens * num_q_heads;                                                        \
      const int rpb = 256 / (D_ / 4);                                                                               \
      hipLaunchKernelGGL((verify_merge_kernel<D_>), dim3(static_cast<unsigned>((total_rows + rpb - 1) / rpb)), dim3(256), 0, st, \
                         ws_acc, ws_ml, p.out, out_token_stride, num_q_heads, num_splits, total_rows);              \
    }                                                                                                               \
  } while (0)
  if (head_dim == 128) SGL_LAUNCH_VERIFY(128);
  else SGL_LAUNCH_VERIFY(64);
#undef SGL_LAUNCH_VERIFY
  SGL_CHECK_LAUNCH("verify_attention");
  return 0;
}

}  // extern "C"
