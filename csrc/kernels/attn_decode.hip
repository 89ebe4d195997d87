// Flash-decoding for gfx950: ONE new query row per sequence against a bf16 K/V cache, grouped-query.
//
// Layouts: kv_cache [B][Smax][2*Hkv*D] (K head j of a position at column j*D, V head j at
// (Hkv + j)*D: the tail of a packed qkv row after its H*D query columns), seq_lens int32 [B] in
// device memory (read here, never by the host), q [B][H*D] with any row stride, ctx [B][H*D] bf16,
// lse [B][H] fp32 = log sum_k exp(scale * q.k).  D is 64 or 128, G = H / Hkv <= 16.
// Paged: kv_pool [num_blocks][page][2*Hkv*D] with the same row layout, page 16 / 32 / 64 / 128, and
// block_table int32 [B][table_stride] in device memory: entry [b][p] is the pool block that holds
// positions [p * page, (p + 1) * page) of sequence b; a sequence holds at most max_blocks * page keys.
//
// * decode_kernel<D>: grid B * Hkv * nsplit, 4 waves.  A block owns one contiguous key range of one
//   (b, K/V head j): the sequence's 128-key units dealt evenly over the splits, the range computed
//   from seq_lens[b], so a short sequence leaves its first splits empty.  The G query heads of the
//   group are the MFMA's narrow dimension (zero-padded to 16), so ONE read of K and V serves them all.
//   The waves take the range's 32-key tiles interleaved (wave w: tiles w, w + 4, ...) and never
//   meet inside the loop: each wave streams its own tiles through its own LDS ring (a stage = the
//   [32][D] K image and the [32][D] V image, filled by LDS-DMA; 2 stages at D = 128, 3 at D = 64),
//   waits with a counted vmcnt and uses no barrier.  A tile past the wave's last gets the
//   out-of-range offset, so the count of copies in flight is the same in every iteration.
//   Scores are transposed, S^T = K Q^T (v_mfma_f32_16x16x32_bf16: A = 16 keys, B = the 16 head
//   columns held in registers for the whole block), so lane l holds head l & 15 and keys
//   4 (l >> 4) + i of each 16-key half.  The running maximum of a head is made uniform over the
//   four lanes of its column with two lane exchanges per tile (the O accumulator of the column is
//   rescaled by it); the running sum stays a per-lane partial until the end.  The eight
//   probabilities of a lane, rounded to bf16 once, ARE the B fragment of O^T += V^T P^T with the
//   tile's keys in the order k = 8g + t -> key 4g + t (t < 4), 16 + 4g + t - 4 (t >= 4); V is read
//   transposed (ds_read_b64_tr_b16) in the same order.
//   Both images keep 16-byte chunk c of row r in slot c ^ swz(r) (the swizzle is on the DMA's source
//   side), which makes the row reads of K conflict-free and spreads the transposed reads of V.
//   The cache is addressed through buffer resources that end with row len - 1: rows at or past the
//   length read as zeros whatever the memory holds (it may be NaN), K scores there are set to -inf,
//   and p = 0 meets v = 0.
//   At the end the four waves put (m, l, O) into their (now idle) LDS regions and the block folds
//   them: nsplit == 1 normalises and stores ctx and lse, otherwise the block stores an fp32 partial
//   [B][H][nsplit][D + 2] (O unnormalised, then m, then l); an empty range gives m = -inf, l = 0.
// * decode_paged_kernel<D>: the same grid, tiles, ring, arithmetic and partial record (wave_tiles,
//   tile_step and fold_store are shared), so with one split count its ctx and lse are bit-equal to
//   decode_kernel's on the same logical data.  Only the addressing differs.  A 16-row half of a tile
//   never crosses a page, and one LDS-DMA instruction covers whole rows (4 or 8) of one half, so every
//   half tile gets its own pair of resources (K | V), built in scalar registers: base = the 64-bit
//   address of its page in the pool plus the head's column offset, num_records = the page's rows below
//   len (clamp(len - p * page, 0, page)) times the row bytes minus the column bytes.  Rows at or past
//   the length therefore read as zeros as above, and no offset spans more than one page, so the pool
//   may be larger than 2^31 bytes.  With page >= 32 the two halves share a table entry; page == 16 reads
//   two.  A block id outside [0, num_blocks) gives an EMPTY resource (num_records 0) before any address
//   is formed, and an entry at or past ceil(len / page) is never loaded: whatever the table, the
//   lengths and the pool hold, nothing outside the pool is read.  The table is read through the
//   constant address space with a wave-uniform index (a scalar load, outside vmcnt), one iteration
//   ahead of the issue() that uses it: the loop's lgkmcnt(0) covers it.
// * decode_combine_kernel<D>: one wave per (b, h) folds the partials in split order (no atomics: the
//   same bits every run), skipping empty ones.  len == 0 gives ctx = 0 and lse = -inf.
// * kv_append_kernel: the 2*Hkv*D K/V columns of B packed rows go to kv_cache[b][seq_lens[b]] (16-byte
//   loads and stores); a position outside [0, Smax) drops its row.  seq_lens is not advanced.
// * kv_append_paged_kernel: the same rows go to kv_pool[table[b][pos / page]][pos % page], pos =
//   seq_lens[b]; a position outside [0, max_blocks * page) or a block id outside [0, num_blocks) drops
//   its row.
// All stores are plain global stores (no buffer store, so no scalar-offset store either).
#include "gfx950.h"

namespace {

constexpr int NT = 256, KT = 32, BT = 128;   // threads, keys per wave tile, keys per block step (4 waves)
constexpr int NCU = 256;
constexpr int MIN_SPLIT_KEYS = 256;          // splits = 0 never makes a split shorter than this

template <int D>
struct Cfg {
  static constexpr int ROWB = 2 * D;                 // bytes of one head row
  static constexpr int CH = D / 8;                   // 16-byte chunks per row
  static constexpr int IMG = KT * ROWB;              // one [32][D] image
  static constexpr int NDMA = IMG / 1024;            // LDS-DMA instructions per image (64 lanes x 16 B)
  static constexpr int NST = D == 128 ? 2 : 3;       // ring stages per wave
  static constexpr int STAGE = 2 * IMG;              // K image | V image
  static constexpr int REGION = NST * STAGE;         // one wave's ring: 32 KB / 24 KB
  static constexpr int INFLIGHT = (NST - 1) * 2 * NDMA;
};

template <int D>
__device__ __forceinline__ int swz(int r) { return D == 128 ? (r & 15) : ((r >> 1) & 7); }
template <int D>
__device__ __forceinline__ int ioff(int r, int c) { return r * Cfg<D>::ROWB + ((c ^ swz<D>(r)) << 4); }

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// ds_read_b64_tr_b16 as tr_read() issues it, but outside the compiler's wait-count bookkeeping: before
// a transposed-read builtin hipcc waits for EVERY LDS-DMA copy in flight (vmcnt(0)), the next tiles'
// too, which would end the pipeline.  The caller waits (lgkmcnt) before it uses the result.
__device__ __forceinline__ s16x4 tr_read_untracked(const char* p) {
  s16x4 r;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"((LDS_PTR(const char))p) : "memory");
  return r;
}
__device__ __forceinline__ void st16(void* p, const uint4& v) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  *reinterpret_cast<u32x4*>(p) = u32x4{v.x, v.y, v.z, v.w};
}

// 128-key units [sp * units / nsplit, (sp + 1) * units / nsplit) of a sequence of `units` units
__device__ __forceinline__ int split_unit(int sp, int units, int nsplit) { return (int)((long)sp * units / nsplit); }

// ---------------------------------------------------------------- shared by decode_kernel and decode_paged_kernel
// this block's 32-key tiles [t0, t1); this wave's are t0 + wave + 4n, n < nt
__device__ __forceinline__ void wave_tiles(int len, int sp, int nsplit, int wave, int& t0, int& nt) {
  const int units = (len + BT - 1) / BT, tiles = (len + KT - 1) / KT;
  t0 = split_unit(sp, units, nsplit) * (BT / KT);
  const int t1e = split_unit(sp + 1, units, nsplit) * (BT / KT), t1 = t1e < tiles ? t1e : tiles;
  nt = t1 - t0 - wave > 0 ? (t1 - t0 - wave + 3) / 4 : 0;
}

// Q^T: head l15 of the group (zero from G on), d = 32 s + 8 g .. + 7
template <int D>
__device__ __forceinline__ void load_q(bf16x8 (&qf)[D / 32], const bf16* __restrict__ q, long q_stride, int b, int j,
                                       int G, int l15, int g) {
  const bf16* qrow = q + (size_t)b * q_stride + (size_t)(j * G + (l15 < G ? l15 : 0)) * D + 8 * g;
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    qf[s] = ldfrag(qrow + 32 * s);
    if (l15 >= G) {
#pragma unroll
      for (int t = 0; t < 8; ++t) qf[s][t] = (bf16)0.f;
    }
  }
}

// The landed tile of keys k0 .. k0 + 31 (images kimg | vimg) folded into the wave's running state.
// m: uniform over the 4 lanes of a head column; l: this lane's part; o: O^T, head l15, d = 16 dt + 4 g + i
template <int D>
__device__ __forceinline__ void tile_step(const char* kimg, const char* vimg, const bf16x8 (&qf)[D / 32], int k0, int len,
                                          float scale, int l15, int g, float& m, float& l, f32x4 (&o)[D / 16]) {
  f32x4 sc[2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    sc[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < D / 32; ++s)
      sc[sub] = mfma16(*reinterpret_cast<const bf16x8*>(kimg + ioff<D>(16 * sub + l15, 4 * s + g)), qf[s], sc[sub]);
  }
  float p[8];                              // p[4 sub + i]: key k0 + 16 sub + 4 g + i
  float mx = -INFINITY;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = k0 + 16 * sub + 4 * g + i < len ? sc[sub][i] * scale : -INFINITY;
      p[4 * sub + i] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mn = fmaxf(m, mx);           // finite: every tile of the range has a key below len
  const float alpha = __expf(m - mn);
  m = mn;
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    p[t] = __expf(p[t] - mn);
    sum += p[t];
  }
  l = l * alpha + sum;
  bf16x8 pb;
#pragma unroll
  for (int t = 0; t < 8; ++t) pb[t] = (bf16)p[t];
  const int qq = l15 >> 2, pp = l15 & 3;
#pragma unroll
  for (int dg = 0; dg < D / 64; ++dg) {    // four 16-column blocks of d at a time: 8 transposed reads, one wait
    s16x4 lo[4], hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 2 * (4 * dg + e) + (pp >> 1), within = (pp & 1) * 8;
      lo[e] = tr_read_untracked(vimg + ioff<D>(4 * g + qq, c) + within);
      hi[e] = tr_read_untracked(vimg + ioff<D>(16 + 4 * g + qq, c) + within);
    }
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3])
                 :
                 : "memory");
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int dt = 4 * dg + e;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[dt][i] *= alpha;
      o[dt] = mfma16(tr_pair(lo[e], hi[e]), pb, o[dt]);
    }
  }
}

// The end of a block: each wave's (O [16][D], m [16], l [16]) into its own region `ring` of smem, then
// the block folds the four and stores ctx / lse (nsplit == 1) or its partial record.
template <int D>
__device__ __forceinline__ void fold_store(char* smem, char* ring, float m, float l, const f32x4 (&o)[D / 16],
                                           float* __restrict__ part, bf16* __restrict__ ctx, float* __restrict__ lse,
                                           int b, int j, int sp, int nsplit, int H, int G, int tid, int l15, int g) {
  using C = Cfg<D>;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  float* wo = reinterpret_cast<float*>(ring);
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<f32x4*>(wo + l15 * D + 16 * dt + 4 * g) = o[dt];
  if (g == 0) {
    wo[16 * D + l15] = m;
    wo[16 * D + 16 + l15] = l;
  }
  __syncthreads();

  constexpr int DE = D / 16;               // thread: head hh, d = d0 .. d0 + DE - 1
  const int hh = tid >> 4, d0 = (tid & 15) * DE;
  float mw[4], M = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    mw[w] = reinterpret_cast<const float*>(smem + w * C::REGION)[16 * D + hh];
    M = fmaxf(M, mw[w]);
  }
  float L = 0.f, acc[DE];
#pragma unroll
  for (int e = 0; e < DE; ++e) acc[e] = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float* ws = reinterpret_cast<const float*>(smem + w * C::REGION);
    const float f = mw[w] == -INFINITY ? 0.f : expf(mw[w] - M);
    L += ws[16 * D + 16 + hh] * f;
#pragma unroll
    for (int e = 0; e < DE; ++e) acc[e] += ws[hh * D + d0 + e] * f;
  }
  if (hh >= G) return;
  const size_t row = (size_t)b * H + j * G + hh;
  if (nsplit == 1) {
    const float inv = L > 0.f ? 1.f / L : 0.f;
    bf16* dst = ctx + row * D + d0;
    if constexpr (DE == 8) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = acc[e] * inv;
      st16(dst, pack8(f));
    } else {
      uint2 u;
      u.x = pack2_bf16(acc[0] * inv, acc[1] * inv);
      u.y = pack2_bf16(acc[2] * inv, acc[3] * inv);
      *reinterpret_cast<uint2*>(dst) = u;
    }
    if ((tid & 15) == 0) lse[row] = L > 0.f ? M + logf(L) : -INFINITY;
  } else {
    float* pr = part + (row * nsplit + sp) * (D + 2);
#pragma unroll
    for (int e = 0; e < DE; ++e) pr[d0 + e] = acc[e];
    if ((tid & 15) == 0) {
      pr[D] = M;
      pr[D + 1] = L;
    }
  }
}

template <int D>
__global__ void __launch_bounds__(NT)
decode_kernel(const bf16* __restrict__ q, long q_stride, const bf16* __restrict__ kv, const int* __restrict__ seq_lens,
              float* __restrict__ part, bf16* __restrict__ ctx, float* __restrict__ lse, int Smax, int H, int Hkv,
              int nsplit, float scale) {
  using C = Cfg<D>;
  __shared__ __attribute__((aligned(16))) char smem[4 * C::REGION];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int G = H / Hkv, W = 2 * Hkv * D;
  int id = blockIdx.x;
  const int sp = id % nsplit;
  id /= nsplit;
  const int j = id % Hkv, b = id / Hkv;
  int len = seq_lens[b];
  len = __builtin_amdgcn_readfirstlane(len < 0 ? 0 : (len > Smax ? Smax : len));
  int t0, nt;
  wave_tiles(len, sp, nsplit, wave, t0, nt);

  // resources that end with row len - 1 of this sequence (num_records < 2^31: the launcher checks)
  const unsigned rowb = (unsigned)W * 2u;
  const bf16* cb = kv + (size_t)b * Smax * W;
  const Rsrc rk = rsrc(cb + j * D, len > 0 ? (unsigned)len * rowb - (unsigned)(j * D) * 2u : 0u);
  const Rsrc rv = rsrc(cb + (Hkv + j) * D, len > 0 ? (unsigned)len * rowb - (unsigned)((Hkv + j) * D) * 2u : 0u);
  // copy i of an image: this lane's 16 bytes land at image byte i * 1024 + lane * 16 = (row r, slot c)
  // and come from logical chunk c ^ swz(r) of that row
  unsigned src[C::NDMA];
#pragma unroll
  for (int i = 0; i < C::NDMA; ++i) {
    const int pos = i * 1024 + lane * 16, r = pos / C::ROWB, c = (pos % C::ROWB) >> 4;
    src[i] = (unsigned)r * rowb + (unsigned)((c ^ swz<D>(r)) << 4);
  }
  char* ring = smem + wave * C::REGION;
  auto issue = [&](int n, int stage) {
    char* dst = ring + stage * C::STAGE;
    const bool on = n < nt;
    const unsigned k0b = (unsigned)((t0 + wave + 4 * n) * KT) * rowb;
#pragma unroll
    for (int i = 0; i < C::NDMA; ++i) dma16(rk, dst + i * 1024, on ? src[i] + k0b : OOB);
#pragma unroll
    for (int i = 0; i < C::NDMA; ++i) dma16(rv, dst + C::IMG + i * 1024, on ? src[i] + k0b : OOB);
  };

  bf16x8 qf[D / 32];
  load_q<D>(qf, q, q_stride, b, j, G, l15, g);
  float m = -INFINITY, l = 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int n = 0; n < C::NST - 1; ++n) issue(n, n);
  int cur = 0, nxt = C::NST - 1;           // stage of tile n, stage of tile n + NST - 1
  for (int n = 0; n < nt; ++n) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads of tile n - 1, whose stage is refilled now
    issue(n + C::NST - 1, nxt);
    vmwait<C::INFLIGHT>();                               // tile n has landed
    const char* kimg = ring + cur * C::STAGE;
    cur = cur + 1 == C::NST ? 0 : cur + 1;
    nxt = nxt + 1 == C::NST ? 0 : nxt + 1;
    tile_step<D>(kimg, kimg + C::IMG, qf, (t0 + wave + 4 * n) * KT, len, scale, l15, g, m, l, o);
  }
  vmwait<0>();                             // the out-of-range copies past the last tile too
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  fold_store<D>(smem, ring, m, l, o, part, ctx, lse, b, j, sp, nsplit, H, G, tid, l15, g);
}

// the block table of one sequence, read through the constant address space: with a wave-uniform
// index that is a scalar load, which vmcnt (the ring's count of copies in flight) does not see
typedef const int __attribute__((address_space(4))) * Table;

template <int D>
__global__ void __launch_bounds__(NT)
decode_paged_kernel(const bf16* __restrict__ q, long q_stride, const bf16* __restrict__ pool,
                    const int* __restrict__ block_table, long table_stride, const int* __restrict__ seq_lens,
                    float* __restrict__ part, bf16* __restrict__ ctx, float* __restrict__ lse, int num_blocks, int lgpage,
                    int max_blocks, int H, int Hkv, int nsplit, float scale) {
  using C = Cfg<D>;
  constexpr int HD = C::NDMA / 2;          // LDS-DMA instructions per 16-row half of an image
  __shared__ __attribute__((aligned(16))) char smem[4 * C::REGION];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int G = H / Hkv, W = 2 * Hkv * D;
  int id = blockIdx.x;
  const int sp = id % nsplit;
  id /= nsplit;
  const int j = id % Hkv, b = id / Hkv;
  const int page = 1 << lgpage, cap = max_blocks << lgpage;   // cap < 2^31: the launcher checks
  int len = seq_lens[b];
  len = __builtin_amdgcn_readfirstlane(len < 0 ? 0 : (len > cap ? cap : len));
  int t0, nt;
  wave_tiles(len, sp, nsplit, wave, t0, nt);
  const int npages = (len + page - 1) >> lgpage;              // table entries [0, npages) may be read

  const unsigned rowb = (unsigned)W * 2u;
  const size_t pageb = (size_t)rowb << lgpage;                // bytes of one pool block
  const unsigned colk = (unsigned)(j * D) * 2u, colv = (unsigned)((Hkv + j) * D) * 2u;
  const Table tab = (Table)(block_table + (size_t)b * table_stride);
  // copy i of an image as in decode_kernel, but relative to the first row of its 16-row half
  unsigned src[C::NDMA];
#pragma unroll
  for (int i = 0; i < C::NDMA; ++i) {
    const int pos = i * 1024 + lane * 16, r = pos / C::ROWB, c = (pos % C::ROWB) >> 4;
    src[i] = (unsigned)(r & 15) * rowb + (unsigned)((c ^ swz<D>(r)) << 4);
  }
  char* ring = smem + wave * C::REGION;
  // the table entries of the two halves of this wave's tile n (-1 for a tile past its last: no load)
  auto fetch = [&](int n, int& e0, int& e1) {
    e0 = e1 = -1;
    if (n < nt) {
      const int k0 = (t0 + wave + 4 * n) * KT;                // k0 < len, so its page is below npages
      const int p1 = (k0 + 16) >> lgpage;                     // the second half may start past the length:
      e0 = tab[k0 >> lgpage];                                 // it then takes the last entry and gets no rows
      e1 = tab[p1 < npages ? p1 : npages - 1];
    }
    e0 = __builtin_amdgcn_readfirstlane(e0);
    e1 = __builtin_amdgcn_readfirstlane(e1);
  };
  auto issue = [&](int n, int stage, int e0, int e1) {
    char* dst = ring + stage * C::STAGE;
    const bool on = n < nt;
    const int k0 = (t0 + wave + 4 * n) * KT;
    Rsrc rk[2], rv[2];
    unsigned rb[2];                                           // byte offset of the half's first row in its page
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kh = k0 + 16 * h, e = h ? e1 : e0;
      int rows = len - (kh >> lgpage << lgpage);              // the page's rows below len
      rows = rows < 0 ? 0 : (rows > page ? page : rows);
      const bool ok = on && (unsigned)e < (unsigned)num_blocks && rows > 0;
      const char* pb = reinterpret_cast<const char*>(pool) + (ok ? (size_t)e * pageb : (size_t)0);
      rk[h] = rsrc(pb + colk, ok ? (unsigned)rows * rowb - colk : 0u);
      rv[h] = rsrc(pb + colv, ok ? (unsigned)rows * rowb - colv : 0u);
      rb[h] = (unsigned)(kh & (page - 1)) * rowb;
    }
#pragma unroll
    for (int i = 0; i < C::NDMA; ++i) dma16(rk[i / HD], dst + i * 1024, on ? src[i] + rb[i / HD] : OOB);
#pragma unroll
    for (int i = 0; i < C::NDMA; ++i) dma16(rv[i / HD], dst + C::IMG + i * 1024, on ? src[i] + rb[i / HD] : OOB);
  };

  bf16x8 qf[D / 32];
  load_q<D>(qf, q, q_stride, b, j, G, l15, g);
  float m = -INFINITY, l = 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  int e0, e1;
#pragma unroll
  for (int n = 0; n < C::NST - 1; ++n) {
    fetch(n, e0, e1);
    issue(n, n, e0, e1);
  }
  fetch(C::NST - 1, e0, e1);
  int cur = 0, nxt = C::NST - 1;           // stage of tile n, stage of tile n + NST - 1
  for (int n = 0; n < nt; ++n) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads of tile n - 1, and the entries fetched then
    issue(n + C::NST - 1, nxt, e0, e1);
    fetch(n + C::NST, e0, e1);                           // for the next iteration's issue
    vmwait<C::INFLIGHT>();                               // tile n has landed
    const char* kimg = ring + cur * C::STAGE;
    cur = cur + 1 == C::NST ? 0 : cur + 1;
    nxt = nxt + 1 == C::NST ? 0 : nxt + 1;
    tile_step<D>(kimg, kimg + C::IMG, qf, (t0 + wave + 4 * n) * KT, len, scale, l15, g, m, l, o);
  }
  vmwait<0>();                             // the out-of-range copies past the last tile too
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  fold_store<D>(smem, ring, m, l, o, part, ctx, lse, b, j, sp, nsplit, H, G, tid, l15, g);
}

template <int D>
__global__ void __launch_bounds__(NT)
decode_combine_kernel(const float* __restrict__ part, bf16* __restrict__ ctx, float* __restrict__ lse, int rows,
                      int nsplit) {
  constexpr int DE = D / 64;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* pr = part + (size_t)row * nsplit * (D + 2);
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, pr[s * (D + 2) + D]);
  float L = 0.f, acc[DE];
#pragma unroll
  for (int e = 0; e < DE; ++e) acc[e] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = pr[s * (D + 2) + D], ls = pr[s * (D + 2) + D + 1];
    if (ms == -INFINITY || ls == 0.f) continue;          // an empty split
    const float f = expf(ms - M);
    L += ls * f;
#pragma unroll
    for (int e = 0; e < DE; ++e) acc[e] += pr[s * (D + 2) + lane * DE + e] * f;
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  bf16* dst = ctx + (size_t)row * D + lane * DE;
  if constexpr (DE == 2)
    *reinterpret_cast<uint32_t*>(dst) = pack2_bf16(acc[0] * inv, acc[1] * inv);
  else
    dst[0] = f2bf(acc[0] * inv);
  if (lane == 0) lse[row] = L > 0.f ? M + logf(L) : -INFINITY;
}

__global__ void __launch_bounds__(NT)
kv_append_kernel(const bf16* __restrict__ rows, long row_stride, bf16* __restrict__ kv,
                 const int* __restrict__ seq_lens, int B, int Smax, int W, int col0) {
  const int cpr = W / 8, idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= B * cpr) return;
  const int b = idx / cpr, c = idx - b * cpr;
  const int pos = seq_lens[b];
  if (pos < 0 || pos >= Smax) return;
  st16(kv + ((size_t)b * Smax + pos) * W + c * 8, ldg16(rows + (size_t)b * row_stride + col0 + c * 8));
}

__global__ void __launch_bounds__(NT)
kv_append_paged_kernel(const bf16* __restrict__ rows, long row_stride, bf16* __restrict__ pool,
                       const int* __restrict__ block_table, long table_stride, const int* __restrict__ seq_lens, int B,
                       int num_blocks, int lgpage, int max_blocks, int W, int col0) {
  const int cpr = W / 8, idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= B * cpr) return;
  const int b = idx / cpr, c = idx - b * cpr;
  const int pos = seq_lens[b];
  if (pos < 0 || pos >= max_blocks << lgpage) return;         // also keeps the table read inside row b
  const int e = block_table[(size_t)b * table_stride + (pos >> lgpage)];
  if ((unsigned)e >= (unsigned)num_blocks) return;
  const size_t row = ((size_t)e << lgpage) + (pos & ((1 << lgpage) - 1));
  st16(pool + row * W + c * 8, ldg16(rows + (size_t)b * row_stride + col0 + c * 8));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool heads_ok(int B, int H, int Hkv, int D) {
  if (B < 1 || Hkv < 1 || H < Hkv || H % Hkv || H / Hkv > 16 || (D != 64 && D != 128)) return false;
  return (long)B * Hkv * 1024 < 0x7fffffffL;
}

// the cache of one sequence, and a last tile's offsets past it, stay below 2^31 bytes (the buffer
// resources' range and the out-of-range offset), G <= 16
bool shape_ok(int B, int Smax, int H, int Hkv, int D) {
  if (Smax < 1 || !heads_ok(B, H, Hkv, D)) return false;
  return ((long)Smax + KT) * 2 * Hkv * D * 2 < 0x7ffffff0L;
}

// log2(page) for page 16 / 32 / 64 / 128, else -1
int lg_page(int page) { return page == 16 ? 4 : page == 32 ? 5 : page == 64 ? 6 : page == 128 ? 7 : -1; }

// A sequence's capacity max_blocks * page, and the key index of a tile a few ring stages past it, stay
// below 2^31; one pool block stays below 2^31 bytes (128 rows at the most, so it does unless the row
// itself is out of any proportion); the pool as a whole may be of any size.
bool paged_ok(int B, int num_blocks, int page, int max_blocks, long table_stride, int H, int Hkv, int D) {
  if (num_blocks < 1 || max_blocks < 1 || lg_page(page) < 0 || table_stride < max_blocks || !heads_ok(B, H, Hkv, D))
    return false;
  return (long)max_blocks * page + 16L * KT < 0x7fffffffL && ((long)page + KT) * 2 * Hkv * D * 2 < 0x7ffffff0L;
}

template <int D>
void launch_combine(float* part, bf16* ctx, float* lse, int rows, int nsplit, hipStream_t st) {
  hipLaunchKernelGGL(decode_combine_kernel<D>, dim3((rows + 3) / 4), dim3(NT), 0, st, (const float*)part, ctx, lse, rows,
                     nsplit);
}

}  // namespace

// The split count the launcher uses.  splits = 0: enough that B * Hkv * nsplit reaches two blocks per
// CU, never so many that a split of `max_len` keys is shorter than 256; an explicit count is clamped
// to the 128-key units of max_len.  max_len is a host-side upper bound of the lengths (Smax will do).
MLC_EXPORT int mlc_attn_decode_splits(int B, int Hkv, int max_len, int splits) {
  if (B < 1 || Hkv < 1 || max_len < 1) return -1;
  const long groups = (long)B * Hkv;
  const int units = (max_len + BT - 1) / BT;
  if (splits <= 0) {
    const long want = (2 * NCU + groups - 1) / groups;
    const int cap = max_len / MIN_SPLIT_KEYS > 1 ? max_len / MIN_SPLIT_KEYS : 1;
    splits = (int)(want < cap ? want : cap);
  }
  splits = splits < units ? splits : units;
  return splits < 1024 ? splits : 1024;
}

// part: fp32 [B * H * nsplit * (D + 2)] with nsplit = mlc_attn_decode_splits(B, Hkv, max_len, splits),
// fully overwritten; not read (may be null) when nsplit == 1.  q_stride in elements.
MLC_EXPORT int mlc_attn_decode(const void* q, long q_stride, const void* kv_cache, const void* seq_lens, void* part,
                               void* ctx, void* lse, int B, int Smax, int H, int Hkv, int D, int max_len, int splits,
                               float scale, hipStream_t st) {
  if (!q || !kv_cache || !seq_lens || !ctx || !lse || !shape_ok(B, Smax, H, Hkv, D)) return -1;
  if (!aligned16(q) || !aligned16(kv_cache) || !aligned16(ctx) || q_stride % 8 || q_stride < (long)H * D) return -1;
  const int nsplit = mlc_attn_decode_splits(B, Hkv, max_len, splits);
  if (nsplit < 1 || (nsplit > 1 && !part)) return -1;
  const dim3 grid(B * Hkv * nsplit);
  if (D == 64)
    hipLaunchKernelGGL(decode_kernel<64>, grid, dim3(NT), 0, st, (const bf16*)q, q_stride, (const bf16*)kv_cache,
                       (const int*)seq_lens, (float*)part, (bf16*)ctx, (float*)lse, Smax, H, Hkv, nsplit, scale);
  else
    hipLaunchKernelGGL(decode_kernel<128>, grid, dim3(NT), 0, st, (const bf16*)q, q_stride, (const bf16*)kv_cache,
                       (const int*)seq_lens, (float*)part, (bf16*)ctx, (float*)lse, Smax, H, Hkv, nsplit, scale);
  if (nsplit > 1) {
    if (D == 64)
      launch_combine<64>((float*)part, (bf16*)ctx, (float*)lse, B * H, nsplit, st);
    else
      launch_combine<128>((float*)part, (bf16*)ctx, (float*)lse, B * H, nsplit, st);
  }
  return 0;
}

// The same over a paged pool: kv_pool [num_blocks][page][2*Hkv*D], block_table int32 [B][table_stride]
// (table_stride >= max_blocks, in elements), page 16 / 32 / 64 / 128.  max_len: a host-side upper bound
// of the lengths (max_blocks * page will do); part as for mlc_attn_decode.
MLC_EXPORT int mlc_attn_decode_paged(const void* q, long q_stride, const void* kv_pool, const void* block_table,
                                     long table_stride, const void* seq_lens, void* part, void* ctx, void* lse, int B,
                                     int num_blocks, int page, int max_blocks, int H, int Hkv, int D, int max_len,
                                     int splits, float scale, hipStream_t st) {
  if (!q || !kv_pool || !block_table || !seq_lens || !ctx || !lse) return -1;
  if (!paged_ok(B, num_blocks, page, max_blocks, table_stride, H, Hkv, D)) return -1;
  if (!aligned16(q) || !aligned16(kv_pool) || !aligned16(ctx) || q_stride % 8 || q_stride < (long)H * D) return -1;
  if (((uintptr_t)block_table | (uintptr_t)seq_lens) & 3) return -1;
  const int nsplit = mlc_attn_decode_splits(B, Hkv, max_len, splits);
  if (nsplit < 1 || (nsplit > 1 && !part)) return -1;
  const dim3 grid(B * Hkv * nsplit);
  if (D == 64)
    hipLaunchKernelGGL(decode_paged_kernel<64>, grid, dim3(NT), 0, st, (const bf16*)q, q_stride, (const bf16*)kv_pool,
                       (const int*)block_table, table_stride, (const int*)seq_lens, (float*)part, (bf16*)ctx,
                       (float*)lse, num_blocks, lg_page(page), max_blocks, H, Hkv, nsplit, scale);
  else
    hipLaunchKernelGGL(decode_paged_kernel<128>, grid, dim3(NT), 0, st, (const bf16*)q, q_stride, (const bf16*)kv_pool,
                       (const int*)block_table, table_stride, (const int*)seq_lens, (float*)part, (bf16*)ctx,
                       (float*)lse, num_blocks, lg_page(page), max_blocks, H, Hkv, nsplit, scale);
  if (nsplit > 1) {
    if (D == 64)
      launch_combine<64>((float*)part, (bf16*)ctx, (float*)lse, B * H, nsplit, st);
    else
      launch_combine<128>((float*)part, (bf16*)ctx, (float*)lse, B * H, nsplit, st);
  }
  return 0;
}

// kv_cache[b][seq_lens[b]] = columns [H*D, (H + 2*Hkv)*D) of packed row b (row_stride in elements)
MLC_EXPORT int mlc_kv_append(const void* qkv_rows, long row_stride, void* kv_cache, const void* seq_lens, int B,
                             int Smax, int H, int Hkv, int D, hipStream_t st) {
  if (!qkv_rows || !kv_cache || !seq_lens || !shape_ok(B, Smax, H, Hkv, D)) return -1;
  if (!aligned16(qkv_rows) || !aligned16(kv_cache) || row_stride % 8 || row_stride < (long)(H + 2 * Hkv) * D) return -1;
  const int W = 2 * Hkv * D;
  const long n = (long)B * (W / 8);
  hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, (const bf16*)qkv_rows,
                     row_stride, (bf16*)kv_cache, (const int*)seq_lens, B, Smax, W, H * D);
  return 0;
}

// kv_pool[block_table[b][pos / page]][pos % page] = the same columns of packed row b, pos = seq_lens[b]
MLC_EXPORT int mlc_kv_append_paged(const void* qkv_rows, long row_stride, void* kv_pool, const void* block_table,
                                   long table_stride, const void* seq_lens, int B, int num_blocks, int page,
                                   int max_blocks, int H, int Hkv, int D, hipStream_t st) {
  if (!qkv_rows || !kv_pool || !block_table || !seq_lens) return -1;
  if (!paged_ok(B, num_blocks, page, max_blocks, table_stride, H, Hkv, D)) return -1;
  if (!aligned16(qkv_rows) || !aligned16(kv_pool) || row_stride % 8 || row_stride < (long)(H + 2 * Hkv) * D) return -1;
  if (((uintptr_t)block_table | (uintptr_t)seq_lens) & 3) return -1;
  const int W = 2 * Hkv * D;
  const long n = (long)B * (W / 8);
  hipLaunchKernelGGL(kv_append_paged_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st,
                     (const bf16*)qkv_rows, row_stride, (bf16*)kv_pool, (const int*)block_table, table_stride,
                     (const int*)seq_lens, B, num_blocks, lg_page(page), max_blocks, W, H * D);
  return 0;
}
