// The two ends of the BERT steps (padded and packed) for gfx950: the embedding gather fused
// with its LayerNorm, the packed embedding backward, and the packed classification head's
// slot-weighted cross-entropy and [CLS] gradient scatter.
//
// * embed_ln_fwd_kernel: e = bf16((word[id] + pos[p]) + tok[ty]) and y = dropout(LN(e)) in one
//   pass.  One 64-lane wave per row, four rows per block, the row held in registers, as
//   ln_fwd_kernel (transformer.hip); the three indices of a row are wave-uniform, the three
//   table rows, gamma and beta are all in flight before the first reduction.  The LayerNorm
//   arithmetic repeats ln_fwd_kernel's in its order, so y / e / mean / rstd carry the bits of
//   mlc_ln_fwd over a torch gather.
// * embed_bwd_packed_kernel: packed rows [T] whose position is pos_ids[row].  A block owns
//   EB_ROWS consecutive rows, threads lie along the columns (one column per thread and step),
//   so every atomic wave-instruction covers 256 contiguous bytes of one table row (the rule
//   above embed_bwd_kernel).  word and pos take direct fp32 atomics; the per-type sums stay
//   in registers over the block's run and leave once per block into copy (block % 32) of a
//   scratch [32][ntypes][H], which embed_bwd_packed_finish_kernel folds into tok and zeroes.
// * softmax_ce_slots_kernel: one thread per slot of [n][ld] logits, fp32 throughout.
// * cls_scatter_kernel: writes all of dh [T][H] (16-byte stores), row r = the sum of dcls[b]
//   over the slots with min(cu[b], T-1) == r, found by binary search in an LDS copy of cu.
//
// Indices come from device memory inside a captured graph: every kernel clamps them where it
// reads them (ids to [0, vocab), types to [0, ntypes), positions to [0, npos), labels to
// [0, num_labels)), forward and backward alike.  A bad index gives wrong numbers, never an
// access out of range.
#include "gfx950.h"
#include "dropout.h"
#include <type_traits>

namespace {

constexpr int NT = 256;
constexpr int EMB_MAXT = 4;     // token types held in registers (as mlc_embed_bwd)
constexpr int EB_ROWS = 8;      // rows per block of the packed backward
constexpr int EB_COPIES = 32;   // token-type scratch copies
constexpr int CLS_NMAX = 1024;  // slots whose cu fits the LDS copy
// The file is built without the packed fp32 VALU forms (mlcomp_amd/build.py FILE_FLAGS).

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ long clampl(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ void load4f(const float* p, float* f) {
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  const f32x4v v = *reinterpret_cast<const f32x4v*>(p);
  f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}
__device__ __forceinline__ void unpack4(const u32x2 u, float* f) {
  f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
}
__device__ __forceinline__ void store4(bf16* p, const float* f) {
  uint2 u;
  u.x = pack2_bf16(f[0], f[1]);
  u.y = pack2_bf16(f[2], f[3]);
  *reinterpret_cast<uint2*>(p) = u;
}

// ------------------------------------------------------------------ embedding + LayerNorm fwd
template <int MAXC>
__global__ void __launch_bounds__(NT)
embed_ln_fwd_kernel(const long* __restrict__ ids, const long* __restrict__ tt, const long* __restrict__ pos_ids,
                    const bf16* __restrict__ word, const bf16* __restrict__ pos, const bf16* __restrict__ tok,
                    const float* __restrict__ gamma, const float* __restrict__ beta, bf16* __restrict__ e_out,
                    bf16* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out, int T, int S,
                    int H, int vocab, int npos, int ntypes, float eps, uint32_t thr_out, float inv_keep_out,
                    const uint32_t* __restrict__ seedp, uint32_t salt_out) {
  // every product and sum below is rounded on its own, except the one fused multiply-add written
  // out in the affine step: that is the instruction sequence mlc_ln_fwd runs (its squares are
  // packed multiplies followed by adds), which the bit-equality with it depends on
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  // the row in a scalar register: the three index loads below are then scalar loads
  const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (NT / 64) + (threadIdx.x >> 6)));
  if (row >= T) return;
  const int nch = H >> 2;
  const uint32_t seed = seedp ? *seedp : 0u;
  const size_t base = (size_t)row * H;
  const long id = clampl(ids[row], vocab - 1);
  const long ty = tt ? clampl(tt[row], ntypes - 1) : 0;
  const long ps = clampl(pos_ids ? pos_ids[row] : (long)(row % S), npos - 1);
  const bf16* wr = word + id * H;
  const bf16* pr = pos + ps * H;
  const bf16* tr = tok + ty * H;
  // every load of the row in flight at once: 3 x 8 bytes per chunk (kept packed, two
  // registers each) and this lane's gamma / beta columns
  u32x2 wv[MAXC], pv[MAXC], tv[MAXC];
  float ga[MAXC][4], be[MAXC][4];
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int c = lane + 64 * k;
    const int o = 4 * (c < nch ? c : 0);   // clamped, always valid: no load under a lane branch
    wv[k] = *reinterpret_cast<const u32x2*>(wr + o);
    pv[k] = *reinterpret_cast<const u32x2*>(pr + o);
    tv[k] = *reinterpret_cast<const u32x2*>(tr + o);
    load4f(gamma + o, ga[k]);
    load4f(beta + o, be[k]);
  }
  float v[MAXC][4];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int c = lane + 64 * k;
    float wf[4], pf[4], tf[4];
    unpack4(wv[k], wf);
    unpack4(pv[k], pf);
    unpack4(tv[k], tf);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[k][e] = 0.f;
    if (c < nch) {
      float s[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = (wf[e] + pf[e]) + tf[e];
      // one rounding to bf16; the LayerNorm reads the rounded value back, as it would from memory
      u32x2 u;
      u.x = pack2_bf16(s[0], s[1]);
      u.y = pack2_bf16(s[2], s[3]);
      *reinterpret_cast<u32x2*>(e_out + base + 4 * c) = u;
      unpack4(u, v[k]);
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += v[k][e];
    }
  }
  const float mean = wave_sum(sum) / (float)H;
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int c = lane + 64 * k;
    if (c < nch) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float d = v[k][e] - mean; sq += d * d; }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)H + eps);
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
#pragma unroll
  for (int k = 0; k < MAXC; ++k) {
    const int c = lane + 64 * k;
    if (c < nch) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = 4 * c + e;
        o[e] = __builtin_fmaf((v[k][e] - mean) * rstd, ga[k][e], be[k][e]);
        if (thr_out)
          o[e] = keep(seed, salt_out, (uint32_t)(base + col), thr_out) ? o[e] * inv_keep_out : 0.f;
      }
      store4(y + base + 4 * c, o);
    }
  }
}

// ------------------------------------------------------------------ packed embedding bwd
__global__ void __launch_bounds__(NT)
embed_bwd_packed_kernel(const bf16* __restrict__ ds, const long* __restrict__ ids, const long* __restrict__ tt,
                        const long* __restrict__ pos_ids, float* __restrict__ word, float* __restrict__ pos,
                        float* __restrict__ scratch, int T, int H, int vocab, int npos, int ntypes) {
  // the run's clamped indices, read once per block; a row past T repeats row T - 1 with a
  // zero gradient, so the loop below has no row branch
  __shared__ long s_id[EB_ROWS], s_pos[EB_ROWS];
  __shared__ int s_ty[EB_ROWS];
  const int r0 = blockIdx.x * EB_ROWS;
  if (threadIdx.x < EB_ROWS) {
    const int r = min(r0 + (int)threadIdx.x, T - 1);
    s_id[threadIdx.x] = clampl(ids[r], vocab - 1);
    s_pos[threadIdx.x] = clampl(pos_ids[r], npos - 1);
    s_ty[threadIdx.x] = tt ? (int)clampl(tt[r], ntypes - 1) : 0;
  }
  __syncthreads();
  float* dst = scratch ? scratch + (size_t)(blockIdx.x % EB_COPIES) * ntypes * H : nullptr;
  // lane-consecutive columns: each atomic wave-instruction is 64 consecutive floats of one row
  for (int c = threadIdx.x; c < H; c += NT) {
    float d[EB_ROWS];
#pragma unroll
    for (int i = 0; i < EB_ROWS; ++i) {   // the run's gradients in flight before the first atomic
      const int r = min(r0 + i, T - 1);
      d[i] = (float)ds[(size_t)r * H + c];
    }
    float ta[EMB_MAXT] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < EB_ROWS; ++i) {
      const float g = r0 + i < T ? d[i] : 0.f;
      atomicAdd(word + s_id[i] * H + c, g);
      atomicAdd(pos + s_pos[i] * H + c, g);
      const int ty = s_ty[i];
#pragma unroll
      for (int k = 0; k < EMB_MAXT; ++k) ta[k] += ty == k ? g : 0.f;
    }
    if (dst) {
#pragma unroll
      for (int k = 0; k < EMB_MAXT; ++k)
        if (k < ntypes) atomicAdd(dst + (size_t)k * H + c, ta[k]);
    }
  }
}

// tok[i] += the EB_COPIES copies of scratch[.][i] in a fixed order; scratch is left zeroed
__global__ void __launch_bounds__(NT)
embed_bwd_packed_finish_kernel(float* __restrict__ scratch, float* __restrict__ tok, int n) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  float v[EB_COPIES];
#pragma unroll
  for (int k = 0; k < EB_COPIES; ++k) v[k] = scratch[(size_t)k * n + i];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < EB_COPIES; ++k) {
    s += v[k];
    scratch[(size_t)k * n + i] = 0.f;
  }
  tok[i] += s;
}

// ------------------------------------------------------------------ packed head
// one block: thread t takes slots t, t + NT, ...; the three sums are reduced in a fixed order
__global__ void __launch_bounds__(NT)
softmax_ce_slots_kernel(const float* __restrict__ logits, const long* __restrict__ labels, const float* __restrict__ w,
                        bf16* __restrict__ dl, float* __restrict__ loss_sum, float* __restrict__ correct,
                        float* __restrict__ wloss, int n, int V, int ld, int num_labels) {
  __shared__ float red[3][NT / 64];
  float ls = 0.f, cs = 0.f, ws = 0.f;
  for (int b = threadIdx.x; b < n; b += NT) {
    const float* x = logits + (size_t)b * ld;
    bf16* g = dl + (size_t)b * ld;
    const int lab = (int)clampl(labels[b], num_labels - 1);
    const float wb = w[b];
    float mx = x[0];
    int am = 0;
    for (int j = 1; j < V; ++j) {
      const float xj = x[j];
      if (xj > mx) { mx = xj; am = j; }   // strict: the first maximum, as torch.argmax
    }
    float se = 0.f;
    for (int j = 0; j < V; ++j) se += expf(x[j] - mx);
    const float lse = logf(se);
    const float nll = -((x[lab] - mx) - lse);
    for (int j = 0; j < V; ++j) {
      const float p = expf((x[j] - mx) - lse);
      g[j] = (bf16)((p - (j == lab ? 1.f : 0.f)) * wb);
    }
    for (int j = V; j < ld; ++j) g[j] = (bf16)0.f;
    if (wb > 0.f) {
      ls += nll;
      cs += am == lab ? 1.f : 0.f;
    }
    ws += nll * wb;
  }
  ls = wave_sum(ls); cs = wave_sum(cs); ws = wave_sum(ws);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = ls; red[1][wave] = cs; red[2][wave] = ws; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) { a += red[0][k]; b += red[1][k]; c += red[2][k]; }
    *loss_sum += a;
    if (correct) *correct += b;
    *wloss = c;
  }
}

// dh [T][H] flat in 16-byte chunks, one per thread, so every store of the pass is independent
// (a wave walking rows one after another behind its search ran at 29.6 us for 6 MB, slower than
// the torch zeros + index_add_ + cast at 17.6 us)
__global__ void __launch_bounds__(NT)
cls_scatter_kernel(const bf16* __restrict__ dcls, const int* __restrict__ cu, bf16* __restrict__ dh, int n, int T,
                   int H) {
  __shared__ int s_key[CLS_NMAX];   // min(cu[b], T - 1): the row slot b gathered
  for (int b = threadIdx.x; b < n; b += NT) s_key[b] = min(cu[b], T - 1);
  __syncthreads();
  const int nch = H >> 3;
  const int i = blockIdx.x * NT + threadIdx.x;   // T * nch <= 2^20 * 2^8
  if (i >= T * nch) return;
  const int r = i / nch, ch = i - r * nch;
  int lo = 0, hi = n;   // the first slot whose row is >= r (the keys of a valid cu ascend)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_key[mid] < r) lo = mid + 1; else hi = mid;
  }
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = lo; b < n && s_key[b] == r; ++b) {   // the equal neighbours, in slot order
    float f[8];
    unpack8(ldg16(dcls + (size_t)b * H + 8 * ch), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
  }
  *reinterpret_cast<uint4*>(dh + (size_t)i * 8) = pack8(acc);
}

template <class K>
int pick_maxc(int cols, K&& launch) {   // the widths mlc_ln_fwd dispatches to
  const int per_lane = (cols / 4 + 63) / 64;
  if (per_lane <= 1) return launch(std::integral_constant<int, 1>{});
  if (per_lane <= 2) return launch(std::integral_constant<int, 2>{});
  if (per_lane <= 4) return launch(std::integral_constant<int, 4>{});
  if (per_lane <= 8) return launch(std::integral_constant<int, 8>{});
  return -1;
}

constexpr int TMAX = 1 << 20;

}  // namespace

// e_out = bf16((word[ids] + pos[p]) + tok[tt]) and y = dropout_out(LN(e_out) * gamma + beta), rows
// [T] of width H; mean / rstd [T].  ids / tt / pos_ids int64 [T]; tt null: type 0; pos_ids null:
// the position of row r is r % S (the padded layout [B][S]).  Tables bf16 [vocab | npos |
// ntypes][H].  -1 without launching for a null required pointer, H % 4 != 0, H > 2048, T outside
// [1, 2^20], S < 1, or an empty table.
MLC_EXPORT int mlc_embed_ln_fwd(const long* ids, const long* tt, const long* pos_ids, const bf16* word,
                                const bf16* pos, const bf16* tok, const float* gamma, const float* beta,
                                bf16* e_out, bf16* y, float* mean, float* rstd, int T, int S, int H, int vocab,
                                int npos, int ntypes, float eps, float p_out, const uint32_t* seed,
                                uint32_t salt_out, hipStream_t st) {
  if (!ids || !word || !pos || !tok || !gamma || !beta || !e_out || !y || !mean || !rstd) return -1;
  if (H < 4 || H % 4 || T < 1 || T > TMAX || S < 1 || vocab < 1 || npos < 1 || ntypes < 1) return -1;
  const uint32_t to = p_out > 0.f ? drop_threshold(p_out) : 0u;
  const float ko = p_out > 0.f ? 1.f / (1.f - p_out) : 1.f;
  const int blocks = (T + NT / 64 - 1) / (NT / 64);
  return pick_maxc(H, [&](auto mc) {
    hipLaunchKernelGGL((embed_ln_fwd_kernel<decltype(mc)::value>), dim3(blocks), dim3(NT), 0, st, ids, tt, pos_ids,
                       word, pos, tok, gamma, beta, e_out, y, mean, rstd, T, S, H, vocab, npos, ntypes, eps, to, ko,
                       seed, salt_out);
    return (int)hipGetLastError();
  });
}

// word[ids[r]] += ds[r], pos[pos_ids[r]] += ds[r], tok[tt[r]] += ds[r] over the packed rows
// r < T (fp32, accumulated).  tt null: type 0; tok null: no token-type table (scratch unused).
// scratch: fp32 [32][ntypes][H], zero on entry and left zeroed.  -1 without launching for a
// null required pointer, T outside [1, 2^20], H < 1, ntypes outside [1, 4] or an empty table.
MLC_EXPORT int mlc_embed_bwd_packed(const bf16* ds, const long* ids, const long* tt, const long* pos_ids,
                                    float* word, float* pos, float* tok, float* scratch, int T, int H, int vocab,
                                    int npos, int ntypes, hipStream_t st) {
  if (!ds || !ids || !pos_ids || !word || !pos || (tok && !scratch)) return -1;
  if (T < 1 || T > TMAX || H < 1 || vocab < 1 || npos < 1 || ntypes < 1 || ntypes > EMB_MAXT) return -1;
  hipLaunchKernelGGL(embed_bwd_packed_kernel, dim3((T + EB_ROWS - 1) / EB_ROWS), dim3(NT), 0, st, ds, ids, tt,
                     pos_ids, word, pos, tok ? scratch : nullptr, T, H, vocab, npos, ntypes);
  if (tok)
    hipLaunchKernelGGL(embed_bwd_packed_finish_kernel, dim3((ntypes * H + NT - 1) / NT), dim3(NT), 0, st, scratch,
                       tok, ntypes * H);
  return hipGetLastError();
}

// Slot-weighted softmax cross-entropy over the first V columns of logits [n][ld] (fp32, as the
// classifier GEMM writes them), dl bf16 [n][ld]:
// dl[b][:V] = (softmax - onehot(labels[b])) * w[b], zero in the padding columns;
// *loss_sum += the nll of the slots with w > 0, *correct += their argmax hits (null: not
// counted), *wloss = sum nll * w (written).  -1 without launching for a null required
// pointer, n outside [1, 2^20] or unless 1 <= num_labels <= V <= ld.
MLC_EXPORT int mlc_softmax_ce_slots(const float* logits, const long* labels, const float* w, bf16* dl,
                                    float* loss_sum, float* correct, float* wloss, int n, int V, int ld,
                                    int num_labels, hipStream_t st) {
  if (!logits || !labels || !w || !dl || !loss_sum || !wloss) return -1;
  if (n < 1 || n > TMAX || num_labels < 1 || num_labels > V || V > ld) return -1;
  hipLaunchKernelGGL(softmax_ce_slots_kernel, dim3(1), dim3(NT), 0, st, logits, labels, w, dl, loss_sum, correct,
                     wloss, n, V, ld, num_labels);
  return hipGetLastError();
}

// dh [T][H] (bf16, every row written): row r = the fp32 sum, rounded once, of dcls[b] over the
// slots b < n with min(cu[b], T - 1) == r, zero elsewhere.  cu int32 [n + 1] ascending.  -1
// without launching for a null pointer, n outside [1, 1024], T outside [1, 2^20], H outside
// [8, 2048] or H % 8 != 0.
MLC_EXPORT int mlc_cls_scatter(const bf16* dcls, const int* cu, bf16* dh, int n, int T, int H, hipStream_t st) {
  if (!dcls || !cu || !dh) return -1;
  if (n < 1 || n > CLS_NMAX || T < 1 || T > TMAX || H < 8 || H > 2048 || H % 8) return -1;
  const long chunks = (long)T * (H / 8);
  hipLaunchKernelGGL(cls_scatter_kernel, dim3((unsigned)((chunks + NT - 1) / NT)), dim3(NT), 0, st, dcls, cu, dh, n,
                     T, H);
  return hipGetLastError();
}
