// Language-model head fused with softmax cross-entropy for gfx950: the logits z = h w^T of
// h [T][K] and w [V][K] (both bf16, K-contiguous) exist only in MFMA accumulators.
//
// * lmhead_lse_kernel (forward): grid = (128-token row tile) x (vocabulary split), one linear
//   block id, XCD-remapped so the blocks of one XCD walk the same w tiles.  A block keeps its
//   128 rows and walks the 128-column vocabulary tiles of its split; per tile it runs the K
//   loop in 64-deep steps.  The h and w tiles of a step are two [128][64] bf16 images in the
//   128-byte-row swizzle (kc_off), filled by LDS-DMA with the swizzle on the source side
//   (dma_chunk); two stages (64 KB), the copies of step s+1 in flight under the MFMAs of step s,
//   counted vmwait and raw barriers.  The pipeline runs on across tile boundaries.  Rows past T
//   and vocabulary rows past V get the out-of-range offset and read as zero.
//   Scores are computed transposed, z^T = w h^T (A = w rows, B = h rows), as in the streaming
//   flash kernels: a lane then holds ONE token (lane & 31) per 32x32 tile and its registers run
//   over vocabulary columns, so the online softmax is lane-local: each of the 4 waves owns 64
//   tokens x 64 columns, a lane keeps (m, l) and the captured label logit for its two tokens
//   over the columns it sees, and nothing crosses lanes until the split ends.  Then the two lane
//   halves fold by one shuffle, the two column waves through LDS, and the block writes (m, l)
//   into part [2*splits + 1][T] (m rows, then l rows); the split whose range holds the label
//   column writes that logit into the last row.  The h tile is re-read once per vocabulary tile
//   (from L2: 128 x K bf16); only w streams from HBM.
// * lmhead_finish_kernel: folds the partials in split order (no atomics: the same bits every
//   run) into lse [T] and nll [T] = lse - z[label]; nll = 0 where the label is ignore_index.
// * lmhead_dlogits_kernel (backward): the same main loop (lmhead_loop, the kernels differ in the
//   epilogue object only); the epilogue forms g = (exp(z - lse) - [col == label]) * dnll from
//   the accumulator, rounds once to bf16 and stores 16 bytes per lane: a lane holds 4
//   consecutive columns per register quad, the other half-wave the next 4, so one exchange with
//   lane ^ 32 gives each lane 8 consecutive columns.  Stores carry their whole offset in the
//   vector register (scalar offset 0).  Splits are independent; there are no partials.
//
// Labels are clamped into [0, V) where they are read; an ignored row's label column is 0 in the
// forward (its nll is zeroed by the finish kernel) and none in the backward (dnll taken as 0).
#include "gfx950.h"

namespace {

constexpr int NT = 256, BM = 128, BN = 128, BK = 64;
constexpr int IMG = BM * BK * 2;          // one [128][64] bf16 image
constexpr int STAGE = 2 * IMG;            // h image | w image
constexpr float M_INIT = -3.0e38f;        // finite floor of the running maximum: exp(M_INIT - m) = 0, no inf - inf
constexpr int NCU = 256;

typedef f32x16 Acc[2][2];                 // [j: 32 vocabulary columns][i: 32 tokens]

// vocabulary column of accumulator register r (of tile j) in lane half `half`, from the wave's first column
__device__ __forceinline__ int acc_col(int j, int r, int half) { return 32 * j + (r & 3) + 8 * (r >> 2) + 4 * half; }

// tiles [sp * tiles / splits, (sp + 1) * tiles / splits): never empty while splits <= tiles
__device__ __forceinline__ int split_tile(int sp, int tiles, int splits) { return sp * tiles / splits; }   // tiles <= 2^15

// ------------------------------------------------------------------ main loop
// Rows m0 .. m0 + 127 of h against vocabulary tiles [tile0, tile1); epi.tile(acc, c0) is called
// with the finished fp32 logits of this wave's 64 tokens x 64 columns from column c0 on.
template <class Epi>
__device__ __forceinline__ void lmhead_loop(const bf16* __restrict__ h, const bf16* __restrict__ w, int T, int V, int K,
                                            int m0, int tile0, int tile1, Epi& epi, char* smem) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nk = K / BK;
  // copy i of this thread lands in image row (tid >> 3) + 32 i, slot tid & 7, and fetches
  // logical chunk dma_chunk(tid) of that row
  unsigned off[4];
  bool hrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (tid >> 3) + 32 * i;
    off[i] = (unsigned)(r * K + dma_chunk(tid) * 8) * 2u;
    hrow[i] = m0 + r < T;
  }
  int ivt = tile0, ikt = 0;               // the next step to issue
  auto issue = [&](char* buf) {
    const int n0 = ivt * BN, k0 = ikt * BK;
    const Rsrc rh = rsrc(h + (size_t)m0 * K + k0), rw = rsrc(w + (size_t)n0 * K + k0);
    char* dst = buf + wave * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16(rh, dst + i * 4096, hrow[i] ? off[i] : OOB);
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16(rw, dst + IMG + i * 4096, n0 + (tid >> 3) + 32 * i < V ? off[i] : OOB);
    if (++ikt == nk) { ikt = 0; ++ivt; }
  };
  const int nsteps = (tile1 - tile0) * nk;
  issue(smem);
  int s = 0;
  for (int vt = tile0; vt < tile1; ++vt) {
    Acc acc;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;
    for (int kt = 0; kt < nk; ++kt, ++s) {
      const char* cur = smem + (s & 1) * STAGE;
      if (s + 1 < nsteps) {
        issue(smem + ((s + 1) & 1) * STAGE);
        vmwait<8>();                       // this wave's 8 copies of step s (and any older store) are done
      } else {
        vmwait<0>();
      }
      lds_barrier();                       // every wave's copies of step s landed
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bf16x8 hf[2], wf[2];
        const int c = 2 * q + (lane >> 5);
#pragma unroll
        for (int i = 0; i < 2; ++i)
          hf[i] = *reinterpret_cast<const bf16x8*>(cur + kc_off(wm * 64 + 32 * i + (lane & 31), c));
#pragma unroll
        for (int j = 0; j < 2; ++j)
          wf[j] = *reinterpret_cast<const bf16x8*>(cur + IMG + kc_off(wn * 64 + 32 * j + (lane & 31), c));
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[j], hf[i], acc[j][i], 0, 0, 0);
      }
      lds_barrier();                       // step s's stage is free for step s + 2
    }
    epi.tile(acc, vt * BN + wn * 64);
  }
}

// label of a row as the kernels use it: clamped into [0, V); `ign` for an ignored row
__device__ __forceinline__ int read_label(const long* labels, int row, int T, int V, long ignore, int ign) {
  if (row >= T) return -1;
  const long v = labels[row];
  if (v == ignore) return ign;
  return (int)(v < 0 ? 0 : (v > V - 1 ? V - 1 : v));
}

// ------------------------------------------------------------------ forward
struct LseEpi {
  int V, half;
  int lab[2];
  float m[2], l[2], zl[2];
  __device__ __forceinline__ void tile(Acc& acc, int c0) {
    if (c0 + 64 > V) {                      // wave-uniform: only a split's last tile masks
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (c0 + acc_col(j, r, half) >= V) acc[j][i][r] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float mx = m[i];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          mx = fmaxf(mx, acc[j][i][r]);
          if (c0 + acc_col(j, r, half) == lab[i]) zl[i] = acc[j][i][r];
        }
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __expf(acc[j][i][r] - mx);
      l[i] = l[i] * __expf(m[i] - mx) + sum;
      m[i] = mx;
    }
  }
};

__global__ void __launch_bounds__(NT, 2)
lmhead_lse_kernel(const bf16* __restrict__ h, const bf16* __restrict__ w, const long* __restrict__ labels,
                  float* __restrict__ part, int T, int V, int K, int splits, long ignore) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tiles_m = (T + BM - 1) / BM, tiles_n = (V + BN - 1) / BN;
  const int id = xcd_remap(blockIdx.x, tiles_m * splits);
  const int tm = id % tiles_m, sp = id / tiles_m;
  const int m0 = tm * BM;
  const int tile0 = split_tile(sp, tiles_n, splits), tile1 = split_tile(sp + 1, tiles_n, splits);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;

  LseEpi epi;
  epi.V = V;
  epi.half = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    epi.lab[i] = read_label(labels, m0 + wm * 64 + 32 * i + (lane & 31), T, V, ignore, 0);
    epi.m[i] = M_INIT; epi.l[i] = 0.f; epi.zl[i] = 0.f;
  }
  lmhead_loop(h, w, T, V, K, m0, tile0, tile1, epi, smem);

  // fold the lane halves, then the two column waves (through LDS: the loop's last barrier freed it)
  float* sh = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float mo = __shfl_xor(epi.m[i], 32, 64), lo = __shfl_xor(epi.l[i], 32, 64);
    const float mx = fmaxf(epi.m[i], mo);
    epi.l[i] = epi.l[i] * __expf(epi.m[i] - mx) + lo * __expf(mo - mx);
    epi.m[i] = mx;
    epi.zl[i] += __shfl_xor(epi.zl[i], 32, 64);     // one lane of the block holds it, the others 0
    const int row = wm * 64 + 32 * i + (lane & 31);
    if (wn == 1 && lane < 32) { sh[row] = epi.m[i]; sh[BM + row] = epi.l[i]; sh[2 * BM + row] = epi.zl[i]; }
  }
  __syncthreads();
  if (wn == 0 && lane < 32) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = wm * 64 + 32 * i + lane;
      if (m0 + row >= T) continue;
      const float mo = sh[row], lo = sh[BM + row];
      const float mx = fmaxf(epi.m[i], mo);
      part[(size_t)sp * T + m0 + row] = mx;
      part[(size_t)(splits + sp) * T + m0 + row] = epi.l[i] * __expf(epi.m[i] - mx) + lo * __expf(mo - mx);
      if (epi.lab[i] >= tile0 * BN && epi.lab[i] < tile1 * BN)
        part[(size_t)2 * splits * T + m0 + row] = epi.zl[i] + sh[2 * BM + row];
    }
  }
}

__global__ void __launch_bounds__(NT)
lmhead_finish_kernel(const float* __restrict__ part, const long* __restrict__ labels, float* __restrict__ lse,
                     float* __restrict__ nll, int T, int splits, long ignore) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t >= T) return;
  float mx = M_INIT;
  for (int sp = 0; sp < splits; ++sp) mx = fmaxf(mx, part[(size_t)sp * T + t]);
  float l = 0.f;
  for (int sp = 0; sp < splits; ++sp) l += part[(size_t)(splits + sp) * T + t] * expf(part[(size_t)sp * T + t] - mx);
  const float v = mx + logf(l);
  lse[t] = v;
  nll[t] = labels[t] == ignore ? 0.f : v - part[(size_t)2 * splits * T + t];
}

// ------------------------------------------------------------------ backward
struct DlEpi {
  int V, half;
  int lab[2];
  float lse[2], dn[2];
  unsigned rowoff[2];                      // OOB for a row past the end
  Rsrc rdl;
  __device__ __forceinline__ void tile(Acc& acc, int c0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint32_t pk[8];                    // quad q = registers 4q .. 4q + 3 = 4 consecutive columns
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          float g[2];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float hit = c0 + acc_col(j, r + e, half) == lab[i] ? 1.f : 0.f;
            g[e] = (__expf(acc[j][i][r + e] - lse[i]) - hit) * dn[i];
          }
          pk[r >> 1] = pack2_bf16(g[0], g[1]);
        }
        // 8-column chunk q is columns 8q .. 8q + 7: its first four are half 0's quad q, the rest
        // half 1's.  Half 0 assembles chunks 0 and 2, half 1 chunks 1 and 3: each sends the
        // quads the other needs.
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const uint32_t a0 = pk[4 * p], a1 = pk[4 * p + 1], b0 = pk[4 * p + 2], b1 = pk[4 * p + 3];
          const uint32_t r0 = (uint32_t)__shfl_xor((int)(half ? a0 : b0), 32, 64);
          const uint32_t r1 = (uint32_t)__shfl_xor((int)(half ? a1 : b1), 32, 64);
          const uint4 out = half ? make_uint4(r0, r1, b0, b1) : make_uint4(a0, a1, r0, r1);
          const int col = c0 + 32 * j + 16 * p + 8 * half;
          bstore(rdl, rowoff[i] != OOB && col < V ? rowoff[i] + (unsigned)col * 2u : OOB, 0, out);
        }
      }
  }
};

__global__ void __launch_bounds__(NT, 2)
lmhead_dlogits_kernel(const bf16* __restrict__ h, const bf16* __restrict__ w, const long* __restrict__ labels,
                      const float* __restrict__ lse, const float* __restrict__ dnll, bf16* __restrict__ dl, int T,
                      int V, int K, int splits, long ignore) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tiles_m = (T + BM - 1) / BM, tiles_n = (V + BN - 1) / BN;
  const int id = xcd_remap(blockIdx.x, tiles_m * splits);
  const int tm = id % tiles_m, sp = id / tiles_m;
  const int m0 = tm * BM;
  const int tile0 = split_tile(sp, tiles_n, splits), tile1 = split_tile(sp + 1, tiles_n, splits);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1;

  DlEpi epi;
  epi.V = V;
  epi.half = lane >> 5;
  epi.rdl = rsrc(dl + (size_t)m0 * V, (long)(T - m0) * V * 2);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wm * 64 + 32 * i + (lane & 31);
    const bool on = m0 + row < T;
    epi.lab[i] = read_label(labels, m0 + row, T, V, ignore, -1);
    epi.lse[i] = on ? lse[m0 + row] : 0.f;
    epi.dn[i] = on && epi.lab[i] >= 0 ? dnll[m0 + row] : 0.f;
    epi.rowoff[i] = on ? (unsigned)row * (unsigned)V * 2u : OOB;
  }
  lmhead_loop(h, w, T, V, K, m0, tile0, tile1, epi, smem);
}

bool shape_ok(int T, int V, int K) {
  // a tile's byte offsets (127 rows of K or V elements) stay below 2^31
  return T >= 1 && V >= 8 && V % 8 == 0 && V <= (1 << 22) && K >= BK && K % BK == 0 && K <= (1 << 20);
}

}  // namespace

// the split count the launchers pick for splits = 0: enough that row tiles x splits fills the
// chip, never more than there are vocabulary tiles; an explicit count is clamped to the tiles
MLC_EXPORT int mlc_lmhead_splits(int T, int V, int splits) {
  if (T < 1 || V < 1) return -1;
  const int tiles_m = (T + BM - 1) / BM, tiles_n = (V + BN - 1) / BN;
  if (splits <= 0) splits = (NCU + tiles_m - 1) / tiles_m;
  return splits < tiles_n ? splits : tiles_n;
}

// part: fp32 [(2 * mlc_lmhead_splits(T, V, splits) + 1) * T], fully overwritten
MLC_EXPORT int mlc_lmhead_lse(const void* h, const void* w, const void* labels, void* part, void* lse, void* nll, int T,
                              int V, int K, int splits, long ignore_index, hipStream_t st) {
  if (!h || !w || !labels || !part || !lse || !nll || !shape_ok(T, V, K)) return -1;
  splits = mlc_lmhead_splits(T, V, splits);
  const int tiles_m = (T + BM - 1) / BM;
  hipLaunchKernelGGL(lmhead_lse_kernel, dim3(tiles_m * splits), dim3(NT), 0, st, (const bf16*)h, (const bf16*)w,
                     (const long*)labels, (float*)part, T, V, K, splits, ignore_index);
  hipLaunchKernelGGL(lmhead_finish_kernel, dim3((T + NT - 1) / NT), dim3(NT), 0, st, (const float*)part,
                     (const long*)labels, (float*)lse, (float*)nll, T, splits, ignore_index);
  return 0;
}

// dl [T][V] bf16 = (softmax(h w^T) - onehot(labels)) * dnll[row]; zeros in an ignored row
MLC_EXPORT int mlc_lmhead_dlogits(const void* h, const void* w, const void* labels, const void* lse, const void* dnll,
                                  void* dl, int T, int V, int K, int splits, long ignore_index, hipStream_t st) {
  if (!h || !w || !labels || !lse || !dnll || !dl || !shape_ok(T, V, K)) return -1;
  splits = mlc_lmhead_splits(T, V, splits);
  const int tiles_m = (T + BM - 1) / BM;
  hipLaunchKernelGGL(lmhead_dlogits_kernel, dim3(tiles_m * splits), dim3(NT), 0, st, (const bf16*)h, (const bf16*)w,
                     (const long*)labels, (const float*)lse, (const float*)dnll, (bf16*)dl, T, V, K, splits,
                     ignore_index);
  return 0;
}
