// General-shape fused multi-head attention for gfx950 (flash-style, online softmax).
//
// transformer.hip's attn:: kernels hold a whole S x S score tile in registers and so only
// take head dim 64 with S in {64, 128} (BERT-base fine-tuning).  These kernels stream the
// keys (forward, dQ) or queries (dK/dV) through LDS in 64-row tiles, so S is any length
// (the last tile's rows past S are masked: -inf key bias / +inf log-sum-exp) and the head
// dim D is 64 or 128; the per-step work is O(S) registers and LDS.
// Reference behaviour: the attention inside the BERT encoder the reference fine-tunes
// through Catalyst; numerics match ops/transformer.py attn_fwd/attn_bwd.
//
// Layout: qkv [B*S][3*H*D] bf16 (q | k | v column blocks, head h at h*D), out / dout
// [B*S][H*D], key_bias [B][S] fp32 (0 / -inf padding mask, any finite bias works),
// lse / dot [B*H*S] fp32.  Dropout on the attention probabilities uses the softmax
// kernel's element index ((b*H + h)*S + q)*S + key (dropout.h), so every attention path
// drops the same elements.
//
// Masks (the *_masked entry points; a compile-time mode of the three streaming kernels, mode 0
// being the unmasked code): causal (query q sees keys <= q: a 128-query block streams only
// the key tiles t < 2*blk + 2, a 128-key block only the query tiles t >= 2*blk, and only the
// two tiles that cross the diagonal compare indices) and an additive fp32 bias
// [b*stride_b + h*stride_h + q*S + key] read straight from global memory (forward / dQ: a
// lane's registers are consecutive keys of one row, 16-byte loads when rows are aligned;
// dK/dV: a register is one query row, the lanes read consecutive keys).  Masked entries get
// -inf before the running max (forward) or in the exponent (backward), so their
// probabilities are exactly 0 whatever the saved log-sum-exp.
//
// Packed variable-length batches (the *_varlen entry points; mode bit M_VARLEN of the same
// three streaming kernels): sequences lie back to back in a [T]-row buffer and block (b, h, blk)
// reads its sequence's first row and length from cu_seqlens in device memory.  The grid is sized
// from nseq_max, H and ceil(max_len / 128); a block whose 128 rows start at or past the length
// returns before any barrier or LDS traffic, and no key / query tile past the length is
// fetched.  Dropout keeps the padded layout's element index at S = max_len.
//
// Work split (one 256-thread block = 4 waves x 32 rows, blocks XCD-remapped so the blocks
// sharing one (b, h) K/V slice sit on one XCD's L2):
// * forward: a wave owns 32 queries; scores are computed transposed, S^T = K Q^T
//   (v_mfma_f32_32x32x16_bf16, A = K rows from LDS, B = Q rows held in registers), so a
//   lane holds ONE query's scores for 32 keys of the 64-key tile and the running max /
//   sum are in-register plus one lane^32 exchange; the unnormalised probabilities feed
//   O^T += V^T P^T straight from the accumulators (B operand) with V read transposed
//   (ds_read_b64_tr_b16).  The accumulator key order is the natural order with bits 2
//   and 3 swapped, so every LDS tile stores logical row r at image row swap23(r).
// * backward, two kernels (no atomics): dq_kernel (a wave owns 32 queries, streams
//   K / V tiles) recomputes P from the saved log-sum-exp, forms dS and accumulates
//   dQ^T = K^T dS^T; it also writes dot = rowsum(dO * O), which equals sum_k P dP
//   with or without dropout.  dkv_kernel (a wave owns 32 keys, streams Q / dO tiles
//   plus their lse / dot) computes S = Q K^T directly (lane = key), and accumulates
//   dV^T = dO^T Pd and dK^T = Q^T dS.
// LDS images: [64 rows][D] bf16, 16-byte chunks XOR-swizzled so that both the row reads
// (ds_read_b128, the MFMA A/B fragment of one row) and the transposed reads are
// conflict-free (checked with the bank model of MI355X_MICROARCH.md §LDS: D=128 is the
// guide's dual-use image (b), D=64 a swizzle over row bits 1, 3, 4 found the same way).
#include "gfx950.h"
#include "dropout.h"
#include <stdlib.h>

namespace {

constexpr int NT = 256;
constexpr int KT = 64;   // rows per streamed tile
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ __forceinline__ int swap23(int k) { return (k & ~12) | ((k >> 1) & 4) | ((k << 1) & 8); }
// row (within a 32-row MFMA tile) of accumulator register r of lane half hh
__device__ __forceinline__ int acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

template <int D>
__device__ __forceinline__ int off(int r, int c) {
  if constexpr (D == 64)
    return r * 128 + 16 * (c ^ ((((r >> 1) & 1) << 2) ^ ((r >> 3) & 1) ^ (((r >> 4) & 1) << 1)));
  else
    return r * 256 + 16 * (c ^ (((r & 3) << 2) | ((r >> 2) & 3)));
}
// operand fragment of logical row `row` (k = d = 16s + 8*(lane>>5) + 0..7)
template <int D>
__device__ __forceinline__ bf16x8 rowf(const char* img, int row, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + off<D>(swap23(row), 2 * s + (lane >> 5)));
}
// transposed operand fragment: column d = base + (lane&31), k = image rows k0 + 8*(lane>>5) + 0..7
template <int D>
__device__ __forceinline__ bf16x8 trf(const char* img, int base, int k0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int col = base + 16 * (g & 1) + 4 * p;
  const int kr = k0 + 8 * (g >> 1);
  return tr_pair(tr_read(img + off<D>(kr + q, col >> 3) + (col & 7) * 2),
                 tr_read(img + off<D>(kr + 4 + q, col >> 3) + (col & 7) * 2));
}
// K-contiguous fragment of row `row` straight from global (ld elements per row)
__device__ __forceinline__ bf16x8 gfrag(const bf16* base, int ld, int row, int s, int lane) {
  return *reinterpret_cast<const bf16x8*>(base + (size_t)row * ld + 16 * s + 8 * (lane >> 5));
}
// accumulator registers 8s..8s+7 as a bf16 B fragment
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& a, int s) {
  bf16x8 r;
#pragma unroll
  for (int t = 0; t < 8; ++t) r[t] = (bf16)a[8 * s + t];
  return r;
}
__device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void zero(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
// store transposed accumulators acc[j][r] = X[lane's row][d = 32j + acc_row(r, hh)] as
// 8-byte pieces
template <int NJ>
__device__ __forceinline__ void store_rows(bf16* dst, const f32x16 (&acc)[NJ], int lane) {
  const int hh = lane >> 5;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint2 u;
      u.x = pack2_bf16(acc[j][4 * g], acc[j][4 * g + 1]);
      u.y = pack2_bf16(acc[j][4 * g + 2], acc[j][4 * g + 3]);
      *reinterpret_cast<uint2*>(dst + 32 * j + 8 * g + 4 * hh) = u;
    }
}

// a 64-row x D tile copied global -> registers -> swizzled LDS image (row r at swap23(r))
template <int D>
struct Tile {
  static constexpr int CH = D / 8, N = KT * CH / NT;
  uint4 v[N];
  __device__ __forceinline__ void load(const bf16* src, int ld, int tid, int valid = KT) {
    // rows past `valid` (the tail tile of an S that is not a multiple of 64) re-read the
    // last valid row: in bounds, finite, and masked out by the caller (-inf key bias /
    // +inf log-sum-exp), so they contribute exactly zero
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int c = tid + NT * j, r = min(c / CH, valid - 1), ch = c % CH;
      v[j] = *reinterpret_cast<const uint4*>(src + (size_t)r * ld + ch * 8);
    }
  }
  __device__ __forceinline__ void store(char* img, int tid) const {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int c = tid + NT * j, r = c / CH, ch = c % CH;
      *reinterpret_cast<uint4*>(img + off<D>(swap23(r), ch)) = v[j];
    }
  }
};

// Mask modes (a template parameter of the streaming kernels; 0 is the unmasked code).
constexpr int M_CAUSAL = 1;   // top-left aligned: query q sees keys <= q
constexpr int M_BIAS = 2;     // additive fp32 bias[b * sb + h * sh + q * S + key], finite or -inf
constexpr int M_VARLEN = 4;   // packed sequences: rows and length of slot b from cu_seqlens (no bias operands)
struct AttnBias {
  const float* p;
  long sb, sh;   // batch / head strides in elements (0 broadcasts)
  int vec;       // rows are 16-byte aligned (S % 4 == 0, aligned base and strides)
};
// bias of this lane's query row for the keys of its accumulator registers: bv[i][g][e] is
// key k0 + 32i + 8g + e (k0 = 64t + 4*hh).  Keys past S (tail tile) are clamped in bounds;
// their scores are -inf from the key bias already.
__device__ __forceinline__ void load_bias_keys(f32x4 (&bv)[2][4], const float* row, int k0, int S, int vec) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int key = k0 + 32 * i + 8 * g;
      if (vec) {
        bv[i][g] = *reinterpret_cast<const f32x4*>(row + min(key, S - 4));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[i][g][e] = row[min(key + e, S - 1)];
      }
    }
}

// Packed variable-length batches (the *_varlen entry points): sequence b owns rows
// cu[b] .. cu[b+1]-1 of the [T]-row buffers; the kernels' S is then max_len (the grid's and the
// dropout index's sequence length) and lse / dot are [H][T].
struct VarLen {
  const int* cu;   // int32 [nseq_max + 1], device memory
  int T;
};
// rows of one (sequence, head): first row, length, and base of its lse / dot entries
struct Seq {
  long row0, stat0;
  int len;
};
template <bool VARLEN>
__device__ __forceinline__ Seq seq_of(int b, int hd, int bh, int S, const VarLen& vl) {
  Seq s;
  if constexpr (VARLEN) {
    // cu_seqlens is device memory nobody has checked since the host did: clamp the start into
    // [0, T] and the length to max_len and to the rows left, so no index leaves the buffers
    const int c0 = min(max(vl.cu[b], 0), vl.T);
    s.len = min(min(vl.cu[b + 1] - c0, S), vl.T - c0);
    s.row0 = c0;
    s.stat0 = (long)hd * vl.T + c0;
  } else {
    s.len = S;
    s.row0 = (long)b * S;
    s.stat0 = (long)bh * S;
  }
  return s;
}

struct Geo {
  int b, hd, bh, blk;
};
__device__ __forceinline__ Geo geo(int H, int nblk) {
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  Geo g;
  g.bh = lin / nblk;
  g.blk = lin - g.bh * nblk;
  g.b = g.bh / H;
  g.hd = g.bh - g.b * H;
  return g;
}

// Causal blocks have unequal work (block blk of a query-block kernel streams 2*blk + 2 key
// tiles, of a key-block kernel nt - 2*blk query tiles), so they are issued heaviest first
// across the whole grid - slot s of every (b, h) before slot s + 1 - and the light blocks
// that arrive last fill in beside the heavy ones.
__device__ __forceinline__ Geo geo_heavy_first(int H, int nblk, bool last_is_heaviest) {
  const int nbh = gridDim.x / nblk;
  const int slot = blockIdx.x / nbh;
  Geo g;
  g.bh = blockIdx.x - slot * nbh;
  g.blk = last_is_heaviest ? nblk - 1 - slot : slot;
  g.b = g.bh / H;
  g.hd = g.bh - g.b * H;
  return g;
}

// ------------------------------------------------------------------ forward
template <int D, bool DROP, int MASK>
__global__ void __launch_bounds__(NT)
fwd_kernel(const bf16* __restrict__ qkv, const float* __restrict__ key_bias, bf16* __restrict__ out,
           float* __restrict__ lse, int S, int H, int nqb, float sl2, uint32_t thr, float inv_keep,
           const uint32_t* __restrict__ seedp, uint32_t salt, AttnBias ab, VarLen vl) {
  constexpr int NS = D / 16, NJ = D / 32, IMG = KT * D * 2, BUF = 2 * IMG + KT * 4;
  constexpr bool CAUSAL = (MASK & M_CAUSAL) != 0, BIAS = (MASK & M_BIAS) != 0, VARLEN = (MASK & M_VARLEN) != 0;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];   // [buffer][K | V | key bias * log2e]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l32 = lane & 31;
  const Geo G = CAUSAL ? geo_heavy_first(H, nqb, true) : geo(H, nqb);
  const int E = H * D, ld = 3 * E;
  const Seq sq = seq_of<VARLEN>(G.b, G.hd, G.bh, S, vl);
  const int L = sq.len;   // this sequence's length (S itself unless packed)
  if (VARLEN && G.blk * 128 >= L) return;   // a grid slot past the sequence (or an empty slot): block-uniform
  const bf16* Qg = qkv + (size_t)sq.row0 * ld + G.hd * D;
  const bf16* Kg = Qg + E;
  const bf16* Vg = Qg + 2 * E;
  const int q = G.blk * 128 + 32 * w + l32;
  const int qc = min(q, L - 1);
  bf16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) qf[s] = gfrag(Qg, ld, qc, s, lane);
  f32x16 o[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) zero(o[j]);
  float m = -INFINITY, l = 0.f;
  const float* kb = key_bias ? key_bias + (size_t)G.b * S : nullptr;
  const uint32_t seed = seedp ? *seedp : 0u;
  const uint32_t rowidx = ((uint32_t)G.bh * S + qc) * S;
  Tile<D> tk, tv;
  float kbv = 0.f;
  auto fetch = [&](int t) {
    const int valid = min(KT, L - t * KT);
    tk.load(Kg + (size_t)t * KT * ld, ld, tid, valid);
    tv.load(Vg + (size_t)t * KT * ld, ld, tid, valid);
    if (tid < KT) kbv = tid >= valid ? -INFINITY : kb ? kb[t * KT + tid] * LOG2E : 0.f;
  };
  auto put = [&](int t) {
    char* bp = smem + (t & 1) * BUF;
    tk.store(bp, tid);
    tv.store(bp + IMG, tid);
    if (tid < KT) reinterpret_cast<float*>(bp + 2 * IMG)[tid] = kbv;
  };
  fetch(0);
  put(0);
  __syncthreads();
  // a partial last tile is masked; a causal query block stops at the tile of its last query
  const int nt = CAUSAL ? min((L + KT - 1) / KT, 2 * G.blk + 2) : (L + KT - 1) / KT;
  const float* brow = BIAS ? ab.p + G.b * ab.sb + G.hd * ab.sh + (size_t)qc * S : nullptr;
  const int wq_last = G.blk * 128 + 32 * __builtin_amdgcn_readfirstlane(w) + 31;   // this wave's last query
  for (int t = 0; t < nt; ++t) {
    const char* Ki = smem + (t & 1) * BUF;
    const char* Vi = Ki + IMG;
    const float* Kb = reinterpret_cast<const float*>(Ki + 2 * IMG);
    if (t + 1 < nt) fetch(t + 1);
    // causal: a wave whose 32 queries all precede the tile's keys has nothing to add (its
    // scores would all be -inf and contribute zero); it still stages and synchronises
    if (!(CAUSAL && t * KT > wq_last)) {
    f32x4 bv[2][4];
    if constexpr (BIAS) load_bias_keys(bv, brow, t * KT + 4 * hh, S, ab.vec);
    f32x16 a[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      zero(a[i]);
#pragma unroll
      for (int s = 0; s < NS; ++s) a[i] = mfma(rowf<D>(Ki, 32 * i + l32, s, lane), qf[s], a[i]);
    }
    const bool diag = CAUSAL && t >= 2 * G.blk;   // the tile crosses the diagonal (block-uniform)
    float tmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(Kb + 32 * i + 8 * g + 4 * hh);   // keys of regs 4g..4g+3
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float x = a[i][4 * g + e] * sl2 + k4[e];
          if constexpr (BIAS) x += bv[i][g][e] * LOG2E;
          if constexpr (CAUSAL)
            if (diag && t * KT + 32 * i + 8 * g + 4 * hh + e > q) x = -INFINITY;
          a[i][4 * g + e] = x;
          tmax = fmaxf(tmax, x);
        }
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);
    if (__any(mn > m)) {   // rescale only when some query's running max moved (wave-uniform)
      const float corr = mn > m ? __builtin_amdgcn_exp2f(m - mn) : 1.f;   // m = -inf: 0
      l *= corr;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] *= corr;
      m = mn;
    }
    const float mref = m == -INFINITY ? 0.f : m;   // fully masked so far: p = 0, o stays 0
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(a[i][r] - mref);
        l += e;
        a[i][r] = e;
      }
    if constexpr (DROP) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          a[i][r] = keep(seed, salt, rowidx + t * KT + 32 * i + acc_row(r, hh), thr) ? a[i][r] * inv_keep : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pb = acc_frag(a[i], s);
#pragma unroll
        for (int j = 0; j < NJ; ++j) o[j] = mfma(trf<D>(Vi, 32 * j, 32 * i + 16 * s, lane), pb, o[j]);
      }
    }
    if (t + 1 < nt) put(t + 1);
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[j][r] *= inv;
  if (q < L) {
    if (hh == 0) lse[sq.stat0 + q] = l > 0.f ? (m + __log2f(l)) * LN2 : INFINITY;
    store_rows<NJ>(out + ((size_t)sq.row0 + q) * E + G.hd * D, o, lane);
  }
}

// ------------------------------------------------------------------ backward: dQ (+ dot)
template <int D, bool DROP, int MASK>
__global__ void __launch_bounds__(NT)
dq_kernel(const bf16* __restrict__ qkv, const float* __restrict__ key_bias, const bf16* __restrict__ out,
          const bf16* __restrict__ dout, const float* __restrict__ lse, float* __restrict__ dot,
          bf16* __restrict__ dqkv, int S, int H, int nqb, float scale, float sl2, uint32_t thr, float inv_keep,
          const uint32_t* __restrict__ seedp, uint32_t salt, AttnBias ab, VarLen vl) {
  constexpr int NS = D / 16, NJ = D / 32, IMG = KT * D * 2, BUF = 2 * IMG + KT * 4;
  constexpr bool CAUSAL = (MASK & M_CAUSAL) != 0, BIAS = (MASK & M_BIAS) != 0, VARLEN = (MASK & M_VARLEN) != 0;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];   // [buffer][K | V | key bias * log2e]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l32 = lane & 31;
  const Geo G = CAUSAL ? geo_heavy_first(H, nqb, true) : geo(H, nqb);
  const int E = H * D, ld = 3 * E;
  const Seq sq = seq_of<VARLEN>(G.b, G.hd, G.bh, S, vl);
  const int L = sq.len;
  if (VARLEN && G.blk * 128 >= L) return;   // as in fwd_kernel
  const bf16* Qg = qkv + (size_t)sq.row0 * ld + G.hd * D;
  const bf16* Kg = Qg + E;
  const bf16* Vg = Qg + 2 * E;
  const bf16* Og = out + (size_t)sq.row0 * E + G.hd * D;
  const bf16* dOg = dout + (size_t)sq.row0 * E + G.hd * D;
  const int q = G.blk * 128 + 32 * w + l32;
  const int qc = min(q, L - 1);
  bf16x8 qf[NS], of[NS];
  float dt = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    qf[s] = gfrag(Qg, ld, qc, s, lane);
    of[s] = gfrag(dOg, E, qc, s, lane);
    const bf16x8 ov = gfrag(Og, E, qc, s, lane);
#pragma unroll
    for (int e = 0; e < 8; ++e) dt += (float)of[s][e] * (float)ov[e];
  }
  dt += __shfl_xor(dt, 32, 64);
  if (q < L && hh == 0) dot[sq.stat0 + q] = dt;
  const float l2 = lse[sq.stat0 + qc] * LOG2E;
  const float* kb = key_bias ? key_bias + (size_t)G.b * S : nullptr;
  const uint32_t seed = seedp ? *seedp : 0u;
  const uint32_t rowidx = ((uint32_t)G.bh * S + qc) * S;
  f32x16 dq[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) zero(dq[j]);
  Tile<D> tk, tv;
  float kbv = 0.f;
  auto fetch = [&](int t) {
    const int valid = min(KT, L - t * KT);
    tk.load(Kg + (size_t)t * KT * ld, ld, tid, valid);
    tv.load(Vg + (size_t)t * KT * ld, ld, tid, valid);
    if (tid < KT) kbv = tid >= valid ? -INFINITY : kb ? kb[t * KT + tid] * LOG2E : 0.f;
  };
  auto put = [&](int t) {
    char* bp = smem + (t & 1) * BUF;
    tk.store(bp, tid);
    tv.store(bp + IMG, tid);
    if (tid < KT) reinterpret_cast<float*>(bp + 2 * IMG)[tid] = kbv;
  };
  fetch(0);
  put(0);
  __syncthreads();
  // a partial last tile is masked; a causal query block stops at the tile of its last query
  const int nt = CAUSAL ? min((L + KT - 1) / KT, 2 * G.blk + 2) : (L + KT - 1) / KT;
  const float* brow = BIAS ? ab.p + G.b * ab.sb + G.hd * ab.sh + (size_t)qc * S : nullptr;
  const int wq_last = G.blk * 128 + 32 * __builtin_amdgcn_readfirstlane(w) + 31;   // this wave's last query
  for (int t = 0; t < nt; ++t) {
    const char* Ki = smem + (t & 1) * BUF;
    const char* Vi = Ki + IMG;
    const float* Kb = reinterpret_cast<const float*>(Ki + 2 * IMG);
    if (t + 1 < nt) fetch(t + 1);
    if (!(CAUSAL && t * KT > wq_last)) {   // as in fwd_kernel: nothing but exact zeros to add
    f32x4 bv[2][4];
    if constexpr (BIAS) load_bias_keys(bv, brow, t * KT + 4 * hh, S, ab.vec);
    const bool diag = CAUSAL && t >= 2 * G.blk;
    f32x16 sp[2], dp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      zero(sp[i]);
      zero(dp[i]);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        sp[i] = mfma(rowf<D>(Ki, 32 * i + l32, s, lane), qf[s], sp[i]);
        dp[i] = mfma(rowf<D>(Vi, 32 * i + l32, s, lane), of[s], dp[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(Kb + 32 * i + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float x = sp[i][r] * sl2 + k4[e];
          if constexpr (BIAS) x += bv[i][g][e] * LOG2E;
          if constexpr (CAUSAL)
            if (diag && t * KT + 32 * i + 8 * g + 4 * hh + e > q) x = -INFINITY;   // p exactly 0
          const float p = __builtin_amdgcn_exp2f(x - l2);
          float d = dp[i][r];
          if constexpr (DROP) d = keep(seed, salt, rowidx + t * KT + 32 * i + 8 * g + 4 * hh + e, thr) ? d * inv_keep : 0.f;
          sp[i][r] = scale * p * (d - dt);
        }
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 sb = acc_frag(sp[i], s);
#pragma unroll
        for (int j = 0; j < NJ; ++j) dq[j] = mfma(trf<D>(Ki, 32 * j, 32 * i + 16 * s, lane), sb, dq[j]);
      }
    }
    if (t + 1 < nt) put(t + 1);
    __syncthreads();
  }
  if (q < L) store_rows<NJ>(dqkv + ((size_t)sq.row0 + q) * ld + G.hd * D, dq, lane);
}

// ------------------------------------------------------------------ backward: dK, dV
template <int D, bool DROP, int MASK>
__global__ void __launch_bounds__(NT)
dkv_kernel(const bf16* __restrict__ qkv, const float* __restrict__ key_bias, const bf16* __restrict__ dout,
           const float* __restrict__ lse, const float* __restrict__ dot, bf16* __restrict__ dqkv, int S, int H,
           int nkb, float scale, float sl2, uint32_t thr, float inv_keep, const uint32_t* __restrict__ seedp,
           uint32_t salt, AttnBias ab, VarLen vl) {
  constexpr int NS = D / 16, NJ = D / 32, IMG = KT * D * 2, BUF = 2 * IMG + 2 * KT * 4;
  constexpr bool CAUSAL = (MASK & M_CAUSAL) != 0, BIAS = (MASK & M_BIAS) != 0, VARLEN = (MASK & M_VARLEN) != 0;
  // [buffer][Q image | dO image | lse*log2e [64] | dot [64]]
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l32 = lane & 31;
  const Geo G = CAUSAL ? geo_heavy_first(H, nkb, false) : geo(H, nkb);
  const int E = H * D, ld = 3 * E;
  const Seq sq = seq_of<VARLEN>(G.b, G.hd, G.bh, S, vl);
  const int L = sq.len;
  if (VARLEN && G.blk * 128 >= L) return;   // as in fwd_kernel
  const bf16* Qg = qkv + (size_t)sq.row0 * ld + G.hd * D;
  const bf16* Kg = Qg + E;
  const bf16* Vg = Qg + 2 * E;
  const bf16* dOg = dout + (size_t)sq.row0 * E + G.hd * D;
  const float* Lg = lse + sq.stat0;
  const float* Dg = dot + sq.stat0;
  const int key = G.blk * 128 + 32 * w + l32;
  const int kc = min(key, L - 1);
  bf16x8 kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    kf[s] = gfrag(Kg, ld, kc, s, lane);
    vf[s] = gfrag(Vg, ld, kc, s, lane);
  }
  const float kbl = key_bias ? key_bias[(size_t)G.b * S + kc] * LOG2E : 0.f;
  const uint32_t seed = seedp ? *seedp : 0u;
  f32x16 dk[NJ], dv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    zero(dk[j]);
    zero(dv[j]);
  }
  Tile<D> tq, to;
  float ld_v = 0.f;   // this thread's lse / dot element of the next tile (threads 0..127)
  auto fetch = [&](int t) {
    const int valid = min(KT, L - t * KT);
    tq.load(Qg + (size_t)t * KT * ld, ld, tid, valid);
    to.load(dOg + (size_t)t * KT * E, E, tid, valid);
    // queries past S: lse = +inf makes their probabilities exactly 0
    if (tid < KT) ld_v = tid < valid ? Lg[t * KT + tid] * LOG2E : INFINITY;
    else if (tid < 2 * KT) ld_v = tid - KT < valid ? Dg[t * KT + tid - KT] : 0.f;
  };
  auto put = [&](int t) {
    char* bp = smem + (t & 1) * BUF;
    tq.store(bp, tid);
    to.store(bp + IMG, tid);
    if (tid < 2 * KT) reinterpret_cast<float*>(bp + 2 * IMG)[tid] = ld_v;
  };
  // causal: the first query tile that sees this key block (128 * blk < L, so t0 < nt); the
  // staging buffers alternate on the tile's parity, whichever tile comes first
  const int t0 = CAUSAL ? 2 * G.blk : 0;
  fetch(t0);
  put(t0);
  __syncthreads();
  const int nt = (L + KT - 1) / KT;   // a partial last tile is masked
  const float* bcol = BIAS ? ab.p + G.b * ab.sb + G.hd * ab.sh + kc : nullptr;
  const int wk_first = G.blk * 128 + 32 * __builtin_amdgcn_readfirstlane(w);   // this wave's first key
  for (int t = t0; t < nt; ++t) {
    const char* bp = smem + (t & 1) * BUF;
    const char* Qi = bp;
    const char* Oi = bp + IMG;
    const float* Ls = reinterpret_cast<const float*>(bp + 2 * IMG);
    const float* Ds = Ls + KT;
    if (t + 1 < nt) fetch(t + 1);
    // causal: a wave whose 32 keys all follow the tile's queries has nothing but exact zeros
    // to add; it still stages and synchronises
    if (!(CAUSAL && t * KT + KT - 1 < wk_first)) {
    const bool diag = CAUSAL && t < t0 + 2;   // the tile crosses the diagonal (block-uniform)
    f32x16 sc[2], dp[2];   // C[q][key]: lane = key, register r = query 32i + acc_row(r, hh)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      zero(sc[i]);
      zero(dp[i]);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        sc[i] = mfma(rowf<D>(Qi, 32 * i + l32, s, lane), kf[s], sc[i]);
        dp[i] = mfma(rowf<D>(Oi, 32 * i + l32, s, lane), vf[s], dp[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int q0 = 32 * i + 8 * g + 4 * hh;   // registers 4g..4g+3 are queries q0..q0+3
        const f32x4 L4 = *reinterpret_cast<const f32x4*>(Ls + q0);
        const f32x4 D4 = *reinterpret_cast<const f32x4*>(Ds + q0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float x = sc[i][r] * sl2 + kbl;
          // padded queries of a tail tile re-read the last row (their lse = +inf zeroes them)
          if constexpr (BIAS) x += bcol[(size_t)min(t * KT + q0 + e, L - 1) * S] * LOG2E;
          if constexpr (CAUSAL)
            if (diag && t * KT + q0 + e < key) x = -INFINITY;   // p exactly 0
          const float p = __builtin_amdgcn_exp2f(x - L4[e]);
          float d = dp[i][r], pd = p;
          if constexpr (DROP) {
            const bool kp = keep(seed, salt, ((uint32_t)G.bh * S + t * KT + q0 + e) * S + kc, thr);
            d = kp ? d * inv_keep : 0.f;
            pd = kp ? p * inv_keep : 0.f;
          }
          dp[i][r] = scale * p * (d - D4[e]);   // dS
          sc[i][r] = pd;                        // Pd
        }
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pb = acc_frag(sc[i], s);
        const bf16x8 sb = acc_frag(dp[i], s);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          dv[j] = mfma(trf<D>(Oi, 32 * j, 32 * i + 16 * s, lane), pb, dv[j]);
          dk[j] = mfma(trf<D>(Qi, 32 * j, 32 * i + 16 * s, lane), sb, dk[j]);
        }
      }
    }
    if (t + 1 < nt) put(t + 1);
    __syncthreads();
  }
  if (key < L) {
    bf16* dst = dqkv + ((size_t)sq.row0 + key) * ld + G.hd * D;
    store_rows<NJ>(dst + E, dk, lane);
    store_rows<NJ>(dst + 2 * E, dv, lane);
  }
}

// ------------------------------------------------------------------ backward, S = 128: fused
// One block per (b, h) holds the whole 128-query x 128-key problem, so P is recomputed once
// (not once per dq / dkv kernel) and there is one launch instead of two:
// * phase 0: every wave forms dot = rowsum(dO * O) for its 32 queries; Q, dO (as the
//   dkv_kernel's swap23 images) and K (natural row order, for the dQ GEMM's transposed
//   reads) are staged in LDS;
// * phase A (dkv_kernel orientation, lane = key): wave w owns keys 32w..32w+31, computes
//   S = Q K^T and dP = dO V^T over both 64-query tiles, P from the saved log-sum-exp, dS,
//   accumulates dV^T = dO^T Pd and dK^T = Q^T dS in registers, and writes dS (bf16) into a
//   [query][key] LDS image;
// * phase B (lane = query): wave w owns queries 32w..32w+31 and forms dQ^T = K^T dS^T from
//   the K and dS images.
// LDS: 3 x 16 KB operand images + the 32 KB dS image + lse / dot = 81 KB (one block per CU).
// (A 65 KB variant with K staged over Q after phase A, two blocks per CU at 231 VGPRs,
// measured 36.5 vs 28.3 us on BERT-base: the co-resident blocks share the matrix pipe and
// the extra barrier/staging did not pay.)
template <int D, bool DROP>
__global__ void __launch_bounds__(NT)
bwd128_kernel(const bf16* __restrict__ qkv, const float* __restrict__ key_bias, const bf16* __restrict__ out,
              const bf16* __restrict__ dout, const float* __restrict__ lse, bf16* __restrict__ dqkv, int H,
              float scale, float sl2, uint32_t thr, float inv_keep, const uint32_t* __restrict__ seedp,
              uint32_t salt) {
  constexpr int S = 128, NS = D / 16, NJ = D / 32, IMG = KT * D * 2;
  constexpr int DS_BYTES = S * S * 2;
  __shared__ __attribute__((aligned(16))) char smem[6 * IMG + DS_BYTES + 2 * S * 4];
  char* Qi = smem;               // two 64-row images each, rows at swap23 (as Tile::store)
  char* Oi = smem + 2 * IMG;
  char* Ki = smem + 4 * IMG;     // 128 rows in natural order
  char* dSi = smem + 6 * IMG;    // [query at swap23][key] bf16, 256-B rows
  float* Ls = reinterpret_cast<float*>(dSi + DS_BYTES);
  float* Dt = Ls + S;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l32 = lane & 31;
  const Geo G = geo(H, 1);
  const int E = H * D, ld = 3 * E;
  const bf16* Qg = qkv + (size_t)G.b * S * ld + G.hd * D;
  const bf16* Kg = Qg + E;
  const bf16* Vg = Qg + 2 * E;
  const bf16* Og = out + (size_t)G.b * S * E + G.hd * D;
  const bf16* dOg = dout + (size_t)G.b * S * E + G.hd * D;
  const uint32_t seed = seedp ? *seedp : 0u;
  // ---- phase 0
  {
    Tile<D> q0, q1, o0, o1, k0, k1;
    q0.load(Qg, ld, tid);
    q1.load(Qg + (size_t)KT * ld, ld, tid);
    o0.load(dOg, E, tid);
    o1.load(dOg + (size_t)KT * E, E, tid);
    k0.load(Kg, ld, tid);
    k1.load(Kg + (size_t)KT * ld, ld, tid);
    const int qr = 32 * w + l32;
    float dt = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const bf16x8 of = gfrag(dOg, E, qr, s, lane), ov = gfrag(Og, E, qr, s, lane);
#pragma unroll
      for (int e = 0; e < 8; ++e) dt += (float)of[e] * (float)ov[e];
    }
    dt += __shfl_xor(dt, 32, 64);
    if (hh == 0) {
      Dt[qr] = dt;
      Ls[qr] = lse[(size_t)G.bh * S + qr] * LOG2E;
    }
    q0.store(Qi, tid);
    q1.store(Qi + IMG, tid);
    o0.store(Oi, tid);
    o1.store(Oi + IMG, tid);
    constexpr int CH = D / 8;
#pragma unroll
    for (int j = 0; j < Tile<D>::N; ++j) {   // K rows in natural order
      const int c = tid + NT * j, r = c / CH, ch = c % CH;
      *reinterpret_cast<uint4*>(Ki + off<D>(r, ch)) = k0.v[j];
      *reinterpret_cast<uint4*>(Ki + off<D>(r + KT, ch)) = k1.v[j];
    }
  }
  // this wave's keys: K / V fragments (B operands) and the key bias
  const int key = 32 * w + l32;
  bf16x8 kf[NS], vf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    kf[s] = gfrag(Kg, ld, key, s, lane);
    vf[s] = gfrag(Vg, ld, key, s, lane);
  }
  const float kbl = key_bias ? key_bias[(size_t)G.b * S + key] * LOG2E : 0.f;
  __syncthreads();
  // ---- phase A
  f32x16 dk[NJ], dv[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    zero(dk[j]);
    zero(dv[j]);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const char* Qt = Qi + t * IMG;
    const char* Ot = Oi + t * IMG;
    f32x16 sc[2], dp[2];   // C[q][key]: lane = key, register r = query 64t + 32i + acc_row(r, hh)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      zero(sc[i]);
      zero(dp[i]);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        sc[i] = mfma(rowf<D>(Qt, 32 * i + l32, s, lane), kf[s], sc[i]);
        dp[i] = mfma(rowf<D>(Ot, 32 * i + l32, s, lane), vf[s], dp[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int q0 = KT * t + 32 * i + 8 * g + 4 * hh;   // registers 4g..4g+3: queries q0..q0+3
        const f32x4 L4 = *reinterpret_cast<const f32x4*>(Ls + q0);
        const f32x4 D4 = *reinterpret_cast<const f32x4*>(Dt + q0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float p = __builtin_amdgcn_exp2f(sc[i][r] * sl2 + kbl - L4[e]);
          float d = dp[i][r], pd = p;
          if constexpr (DROP) {
            const bool kp = keep(seed, salt, ((uint32_t)G.bh * S + q0 + e) * S + key, thr);
            d = kp ? d * inv_keep : 0.f;
            pd = kp ? p * inv_keep : 0.f;
          }
          const float ds = scale * p * (d - D4[e]);
          dp[i][r] = ds;
          sc[i][r] = pd;
          *reinterpret_cast<bf16*>(dSi + off<128>(swap23(q0 + e), key >> 3) + (key & 7) * 2) = (bf16)ds;
        }
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pb = acc_frag(sc[i], s);
        const bf16x8 sb = acc_frag(dp[i], s);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          dv[j] = mfma(trf<D>(Ot, 32 * j, 32 * i + 16 * s, lane), pb, dv[j]);
          dk[j] = mfma(trf<D>(Qt, 32 * j, 32 * i + 16 * s, lane), sb, dk[j]);
        }
      }
  }
  {
    bf16* dst = dqkv + ((size_t)G.b * S + key) * ld + G.hd * D;
    store_rows<NJ>(dst + E, dk, lane);
    store_rows<NJ>(dst + 2 * E, dv, lane);
  }
  __syncthreads();   // every wave's dS is in the image
  // ---- phase B: dQ^T[d][q] = sum_key K^T[d][key] dS^T[key][q], lane = query 32w + l32
  f32x16 dq[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) zero(dq[j]);
  const int qr = 32 * w + l32;
#pragma unroll
  for (int s = 0; s < S / 16; ++s) {
    const bf16x8 sb = rowf<128>(dSi, qr, s, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) dq[j] = mfma(trf<D>(Ki, 32 * j, 16 * s, lane), sb, dq[j]);
  }
  store_rows<NJ>(dqkv + ((size_t)G.b * S + qr) * ld + G.hd * D, dq, lane);
}

// ------------------------------------------------------------------ forward, S = 128
// The whole key range at once: K and V (128 rows each, two consecutive swap23 images = one
// 128-row image) land in LDS behind ONE barrier, the 4 key tiles of S^T = K Q^T are formed,
// and the softmax runs over the complete row (no running max / rescale), then O^T = V^T P^T.
// Same numerics and dropout indexing as fwd_kernel.
template <int D, bool DROP>
__global__ void __launch_bounds__(NT)
fwd128_kernel(const bf16* __restrict__ qkv, const float* __restrict__ key_bias, bf16* __restrict__ out,
              float* __restrict__ lse, int H, float sl2, uint32_t thr, float inv_keep,
              const uint32_t* __restrict__ seedp, uint32_t salt) {
  constexpr int S = 128, NS = D / 16, NJ = D / 32, IMG = KT * D * 2;
  __shared__ __attribute__((aligned(16))) char smem[4 * IMG + S * 4];   // K (2 images) | V (2) | bias
  char* Ki = smem;
  char* Vi = smem + 2 * IMG;
  float* Kb = reinterpret_cast<float*>(smem + 4 * IMG);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l32 = lane & 31;
  const Geo G = geo(H, 1);
  const int E = H * D, ld = 3 * E;
  const bf16* Qg = qkv + (size_t)G.b * S * ld + G.hd * D;
  const bf16* Kg = Qg + E;
  const bf16* Vg = Qg + 2 * E;
  const int q = 32 * w + l32;
  {
    Tile<D> k0, k1, v0, v1;
    k0.load(Kg, ld, tid);
    k1.load(Kg + (size_t)KT * ld, ld, tid);
    v0.load(Vg, ld, tid);
    v1.load(Vg + (size_t)KT * ld, ld, tid);
    if (tid < S) Kb[tid] = key_bias ? key_bias[(size_t)G.b * S + tid] * LOG2E : 0.f;
    k0.store(Ki, tid);
    k1.store(Ki + IMG, tid);
    v0.store(Vi, tid);
    v1.store(Vi + IMG, tid);
  }
  bf16x8 qf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) qf[s] = gfrag(Qg, ld, q, s, lane);
  const uint32_t seed = seedp ? *seedp : 0u;
  const uint32_t rowidx = ((uint32_t)G.bh * S + q) * S;
  __syncthreads();
  f32x16 a[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    zero(a[i]);
#pragma unroll
    for (int s = 0; s < NS; ++s) a[i] = mfma(rowf<D>(Ki, 32 * i + l32, s, lane), qf[s], a[i]);
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(Kb + 32 * i + 8 * g + 4 * hh);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = a[i][4 * g + e] * sl2 + k4[e];
        a[i][4 * g + e] = x;
        m = fmaxf(m, x);
      }
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float mref = m == -INFINITY ? 0.f : m;
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = __builtin_amdgcn_exp2f(a[i][r] - mref);
      l += e;
      a[i][r] = e;
    }
  if constexpr (DROP) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        a[i][r] = keep(seed, salt, rowidx + 32 * i + acc_row(r, hh), thr) ? a[i][r] * inv_keep : 0.f;
  }
  f32x16 o[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) zero(o[j]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 pb = acc_frag(a[i], s);
#pragma unroll
      for (int j = 0; j < NJ; ++j) o[j] = mfma(trf<D>(Vi, 32 * j, 32 * i + 16 * s, lane), pb, o[j]);
    }
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[j][r] *= inv;
  if (hh == 0) lse[(size_t)G.bh * S + q] = l > 0.f ? (m + __log2f(l)) * LN2 : INFINITY;
  store_rows<NJ>(out + ((size_t)G.b * S + q) * E + G.hd * D, o, lane);
}

// MLC_ATTN_BWD128=0 routes S = 128, D = 64 back to the streaming kernels (fwd_kernel and the
// dq / dkv pair)
int g_bwd128 = -1;

bool flash_shape_ok(int B, int S, int H, int D) {
  return B > 0 && H > 0 && S >= 1 && (D == 64 || D == 128);
}

}  // namespace

namespace {

void resolve_bwd128() {
  if (g_bwd128 < 0) {
    const char* e = getenv("MLC_ATTN_BWD128");
    g_bwd128 = e ? atoi(e) : 1;
  }
}

// the mask mode of a call and the bias operand the kernels take
int mask_mode(int causal, const float* attn_bias) { return (causal ? M_CAUSAL : 0) | (attn_bias ? M_BIAS : 0); }
AttnBias bias_arg(const float* attn_bias, long stride_b, long stride_h, int S) {
  AttnBias ab;
  ab.p = attn_bias;
  ab.sb = stride_b;
  ab.sh = stride_h;
  ab.vec = attn_bias && S % 4 == 0 && (reinterpret_cast<uintptr_t>(attn_bias) & 15) == 0 && stride_b % 4 == 0 &&
           stride_h % 4 == 0;
  return ab;
}

// instantiate X(D, DROP, MASK) for the call's head dim, dropout and mask mode
#define FLASH_DISPATCH(X)                                                     \
  do {                                                                        \
    if (D == 64) { if (t) { FLASH_MASKS(X, 64, true) } else { FLASH_MASKS(X, 64, false) } }   \
    else { if (t) { FLASH_MASKS(X, 128, true) } else { FLASH_MASKS(X, 128, false) } }         \
  } while (0)
#define FLASH_MASKS(X, DD, DR)                  \
  switch (mode) {                               \
    case 0: X(DD, DR, 0); break;                \
    case M_CAUSAL: X(DD, DR, M_CAUSAL); break;  \
    case M_BIAS: X(DD, DR, M_BIAS); break;      \
    default: X(DD, DR, M_CAUSAL | M_BIAS); break; \
  }

int flash_fwd(const bf16* qkv, const float* key_bias, bf16* out, float* lse, int B, int S, int H, int D, float scale,
              float p, const uint32_t* seed, uint32_t salt, int causal, const float* attn_bias, long stride_b,
              long stride_h, hipStream_t st) {
  if (!flash_shape_ok(B, S, H, D)) return -1;
  const uint32_t t = p > 0.f ? drop_threshold(p) : 0u;
  const float k = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int mode = mask_mode(causal, attn_bias);
  resolve_bwd128();
  if (S == 128 && D == 64 && g_bwd128 && !mode) {   // whole-key-range forward (MLC_ATTN_BWD128 covers both)
    const dim3 grid(B * H);
    if (t)
      hipLaunchKernelGGL((fwd128_kernel<64, true>), grid, dim3(NT), 0, st, qkv, key_bias, out, lse, H, scale * LOG2E,
                         t, k, seed, salt);
    else
      hipLaunchKernelGGL((fwd128_kernel<64, false>), grid, dim3(NT), 0, st, qkv, key_bias, out, lse, H, scale * LOG2E,
                         t, k, seed, salt);
    return hipGetLastError();
  }
  const int nqb = (S + 127) / 128;
  const dim3 grid(B * H * nqb);
  const AttnBias ab = bias_arg(attn_bias, stride_b, stride_h, S);
  const VarLen vl{nullptr, 0};
#define FWD(DD, DR, MM) hipLaunchKernelGGL((fwd_kernel<DD, DR, MM>), grid, dim3(NT), 0, st, qkv, key_bias, out, lse, S, \
                                           H, nqb, scale * LOG2E, t, k, seed, salt, ab, vl)
  FLASH_DISPATCH(FWD);
#undef FWD
  return hipGetLastError();
}

// instantiate X(D, DROP, MASK) of the packed form: M_VARLEN with or without M_CAUSAL
#define VARLEN_DISPATCH(X)                                                                            \
  do {                                                                                                \
    if (D == 64) { if (t) { VARLEN_MASKS(X, 64, true) } else { VARLEN_MASKS(X, 64, false) } }         \
    else { if (t) { VARLEN_MASKS(X, 128, true) } else { VARLEN_MASKS(X, 128, false) } }               \
  } while (0)
#define VARLEN_MASKS(X, DD, DR) \
  if (causal) X(DD, DR, M_VARLEN | M_CAUSAL); else X(DD, DR, M_VARLEN);

// the packed calls' shape rule: T rows, nseq slots of at most max_len rows each
bool varlen_shape_ok(const int* cu, int T, int nseq, int max_len, int H, int D) {
  return cu && T > 0 && nseq > 0 && max_len >= 1 && H > 0 && (D == 64 || D == 128);
}

int flash_fwd_varlen(const bf16* qkv, const int* cu, bf16* out, float* lse, int T, int nseq, int max_len, int H, int D,
                     float scale, float p, const uint32_t* seed, uint32_t salt, int causal, hipStream_t st) {
  if (!varlen_shape_ok(cu, T, nseq, max_len, H, D)) return -1;
  const uint32_t t = p > 0.f ? drop_threshold(p) : 0u;
  const float k = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int nqb = (max_len + 127) / 128;
  const dim3 grid(nseq * H * nqb);   // from nseq_max, H and max_len only: fixed under graph replay
  const AttnBias ab = bias_arg(nullptr, 0, 0, max_len);
  const VarLen vl{cu, T};
#define FWD(DD, DR, MM) hipLaunchKernelGGL((fwd_kernel<DD, DR, MM>), grid, dim3(NT), 0, st, qkv, nullptr, out, lse, \
                                           max_len, H, nqb, scale * LOG2E, t, k, seed, salt, ab, vl)
  VARLEN_DISPATCH(FWD);
#undef FWD
  return hipGetLastError();
}

int flash_bwd_varlen(const bf16* qkv, const int* cu, const bf16* out, const bf16* dout, const float* lse, float* dot,
                     bf16* dqkv, int T, int nseq, int max_len, int H, int D, float scale, float p,
                     const uint32_t* seed, uint32_t salt, int causal, hipStream_t st) {
  if (!varlen_shape_ok(cu, T, nseq, max_len, H, D)) return -1;
  const uint32_t t = p > 0.f ? drop_threshold(p) : 0u;
  const float k = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int nb = (max_len + 127) / 128;
  const dim3 grid(nseq * H * nb);
  const AttnBias ab = bias_arg(nullptr, 0, 0, max_len);
  const VarLen vl{cu, T};
#define BWD(DD, DR, MM)                                                                                             \
  do {                                                                                                              \
    hipLaunchKernelGGL((dq_kernel<DD, DR, MM>), grid, dim3(NT), 0, st, qkv, nullptr, out, dout, lse, dot, dqkv,     \
                       max_len, H, nb, scale, scale * LOG2E, t, k, seed, salt, ab, vl);                            \
    hipLaunchKernelGGL((dkv_kernel<DD, DR, MM>), grid, dim3(NT), 0, st, qkv, nullptr, dout, lse, dot, dqkv,         \
                       max_len, H, nb, scale, scale * LOG2E, t, k, seed, salt, ab, vl);                            \
  } while (0)
  VARLEN_DISPATCH(BWD);
#undef BWD
  return hipGetLastError();
}
#undef VARLEN_MASKS
#undef VARLEN_DISPATCH

int flash_bwd(const bf16* qkv, const float* key_bias, const bf16* out, const bf16* dout, const float* lse, float* dot,
              bf16* dqkv, int B, int S, int H, int D, float scale, float p, const uint32_t* seed, uint32_t salt,
              int causal, const float* attn_bias, long stride_b, long stride_h, hipStream_t st) {
  resolve_bwd128();
  if (!flash_shape_ok(B, S, H, D)) return -1;
  const uint32_t t = p > 0.f ? drop_threshold(p) : 0u;
  const float k = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int mode = mask_mode(causal, attn_bias);
  if (S == 128 && D == 64 && g_bwd128 && !mode) {   // whole-problem fused backward (MLC_ATTN_BWD128)
    const dim3 grid(B * H);
    if (t)
      hipLaunchKernelGGL((bwd128_kernel<64, true>), grid, dim3(NT), 0, st, qkv, key_bias, out, dout, lse, dqkv, H,
                         scale, scale * LOG2E, t, k, seed, salt);
    else
      hipLaunchKernelGGL((bwd128_kernel<64, false>), grid, dim3(NT), 0, st, qkv, key_bias, out, dout, lse, dqkv, H,
                         scale, scale * LOG2E, t, k, seed, salt);
    return hipGetLastError();
  }
  const int nb = (S + 127) / 128;
  const dim3 grid(B * H * nb);
  const AttnBias ab = bias_arg(attn_bias, stride_b, stride_h, S);
  const VarLen vl{nullptr, 0};
#define BWD(DD, DR, MM)                                                                                              \
  do {                                                                                                               \
    hipLaunchKernelGGL((dq_kernel<DD, DR, MM>), grid, dim3(NT), 0, st, qkv, key_bias, out, dout, lse, dot, dqkv, S, H, \
                       nb, scale, scale * LOG2E, t, k, seed, salt, ab, vl);                                          \
    hipLaunchKernelGGL((dkv_kernel<DD, DR, MM>), grid, dim3(NT), 0, st, qkv, key_bias, dout, lse, dot, dqkv, S, H, nb, \
                       scale, scale * LOG2E, t, k, seed, salt, ab, vl);                                              \
  } while (0)
  FLASH_DISPATCH(BWD);
#undef BWD
  return hipGetLastError();
}
#undef FLASH_MASKS
#undef FLASH_DISPATCH

}  // namespace

// out [B*S][H*D] = softmax(scale * Q K^T + key_bias) V per head, lse [B*H*S] (natural log;
// +inf for a fully masked row).  Any S >= 1 (a partial last 64-key tile is masked), D in {64, 128}.
MLC_EXPORT int mlc_flash_fwd(const bf16* qkv, const float* key_bias, bf16* out, float* lse, int B, int S, int H,
                             int D, float scale, float p, const uint32_t* seed, uint32_t salt, hipStream_t st) {
  return flash_fwd(qkv, key_bias, out, lse, B, S, H, D, scale, p, seed, salt, 0, nullptr, 0, 0, st);
}

// dqkv [B*S][3*H*D] fully overwritten (dQ | dK | dV); out = the forward's output; dot
// [B*H*S] fp32 scratch.
MLC_EXPORT int mlc_flash_bwd(const bf16* qkv, const float* key_bias, const bf16* out, const bf16* dout,
                             const float* lse, float* dot, bf16* dqkv, int B, int S, int H, int D, float scale,
                             float p, const uint32_t* seed, uint32_t salt, hipStream_t st) {
  return flash_bwd(qkv, key_bias, out, dout, lse, dot, dqkv, B, S, H, D, scale, p, seed, salt, 0, nullptr, 0, 0, st);
}

// The same with attention masks: softmax(scale * Q K^T + key_bias + attn_bias [+ causal]).
// causal != 0: query q sees keys <= q (a query block streams only the key tiles up to its
// diagonal).  attn_bias (may be null): fp32, element (b, h, q, key) at
// attn_bias[b * stride_b + h * stride_h + q * S + key], a stride of 0 broadcasts; values finite
// or -inf.  A fully masked row gives zero output, lse = +inf and zero gradients.  Masked calls
// always run the streaming kernels (also at S = 128, D = 64).
MLC_EXPORT int mlc_flash_fwd_masked(const bf16* qkv, const float* key_bias, bf16* out, float* lse, int B, int S,
                                    int H, int D, float scale, float p, const uint32_t* seed, uint32_t salt,
                                    int causal, const float* attn_bias, long stride_b, long stride_h,
                                    hipStream_t st) {
  return flash_fwd(qkv, key_bias, out, lse, B, S, H, D, scale, p, seed, salt, causal, attn_bias, stride_b, stride_h,
                   st);
}

MLC_EXPORT int mlc_flash_bwd_masked(const bf16* qkv, const float* key_bias, const bf16* out, const bf16* dout,
                                    const float* lse, float* dot, bf16* dqkv, int B, int S, int H, int D,
                                    float scale, float p, const uint32_t* seed, uint32_t salt, int causal,
                                    const float* attn_bias, long stride_b, long stride_h, hipStream_t st) {
  return flash_bwd(qkv, key_bias, out, dout, lse, dot, dqkv, B, S, H, D, scale, p, seed, salt, causal, attn_bias,
                   stride_b, stride_h, st);
}

// Packed variable-length batches: qkv [T][3*H*D], out / dout [T][H*D], lse / dot fp32 [H][T]
// (index h*T + row).  cu_seqlens int32 [nseq_max + 1] in device memory, non-decreasing,
// cu[0] = 0, cu[nseq_max] <= T: sequence b owns rows cu[b] .. cu[b+1]-1 (none: an empty slot);
// max_len bounds every length.  The grid depends on nseq_max, H and max_len only, and every
// length is read (and clamped to max_len and to the rows left) on the device, so a captured
// graph replays on another split.  Rows of no sequence are not written: the caller passes
// zero-filled out / lse / dqkv.  Dropout drops element ((b*H + h)*max_len + q)*max_len + key
// (q, key within the sequence), what the padded call at S = max_len drops.  causal != 0 as in
// the masked entry points; no bias operands.
MLC_EXPORT int mlc_flash_fwd_varlen(const bf16* qkv, const int* cu_seqlens, bf16* out, float* lse, int T,
                                    int nseq_max, int max_len, int H, int D, float scale, float p,
                                    const uint32_t* seed, uint32_t salt, int causal, hipStream_t st) {
  return flash_fwd_varlen(qkv, cu_seqlens, out, lse, T, nseq_max, max_len, H, D, scale, p, seed, salt, causal, st);
}

MLC_EXPORT int mlc_flash_bwd_varlen(const bf16* qkv, const int* cu_seqlens, const bf16* out, const bf16* dout,
                                    const float* lse, float* dot, bf16* dqkv, int T, int nseq_max, int max_len,
                                    int H, int D, float scale, float p, const uint32_t* seed, uint32_t salt,
                                    int causal, hipStream_t st) {
  return flash_bwd_varlen(qkv, cu_seqlens, out, dout, lse, dot, dqkv, T, nseq_max, max_len, H, D, scale, p, seed,
                          salt, causal, st);
}

// A/B knob of the S = 128 fused backward: value 0 / 1 sets it, < 0 only reads; returns the
// previous setting (resolving MLC_ATTN_BWD128 first)
MLC_EXPORT int mlc_flash_bwd128(int value) {
  if (g_bwd128 < 0) {
    const char* e = getenv("MLC_ATTN_BWD128");
    g_bwd128 = e ? atoi(e) : 1;
  }
  const int old = g_bwd128;
  if (value >= 0) g_bwd128 = value ? 1 : 0;
  return old;
}

