// Forward of a channel-expanding 1x1 / stride-1 / pad-0 conv with BN statistics as a
// weight-stationary streaming kernel:
//   y[rows][Co] = x[rows][K] . W[Co][K]^T   (bf16)   +   per-channel sum(y), sum(y^2) partials
// The igemm tile loop gives such a conv 2 or 4 K-tiles per 128x128 output tile, and every
// tile pays a cold DMA prologue, an LDS-staged epilogue, 256 float atomics and a fresh fetch
// of the weights.  Here the weights stay put and the rows stream past:
//   * one persistent block of 4 waves per CU owns a 256-channel chunk of W; wave w holds its
//     64 x K slice as MFMA A-fragments in registers (K/16 * 2 fragments), loaded once;
//   * the block walks 64-row tiles of x (tile = row group + i * groups).  A tile goes
//     global -> registers -> LDS (two buffers); its loads are issued a whole tile ahead and
//     fly during the previous tile's MFMAs and stores.  One raw s_barrier per tile and counted
//     vmcnt waits, never a drain;
//   * the product is formed transposed (A = W, B = x): a lane then holds one output row and
//     runs of 4 consecutive channels, two half-waves are paired with v_permlane32_swap, and y
//     leaves in 16-byte stores straight from the accumulators - no LDS staging, no barrier;
//   * sum(y) and sum(y^2) are accumulated per lane over the whole row loop (from the fp32
//     accumulators, the values the igemm EpiBF16 statistics use) and leave once per block:
//     a 32-lane reduction and 2 * 256 float atomics into copy (row group % ncopy).
// K is walked in ascending 16-steps with v_mfma_f32_32x32x16_bf16 and the lane -> k mapping of
// the igemm fragments, so the accumulators and the stored y are bit-identical to igemm's.
// Blocks that share rows (the Co / 256 chunks of one row group) are launched 8 ids apart, i.e.
// on the same XCD, so the repeated reads of x meet in that XCD's L2.
// The inference form (conv1x1_fwd_res_kernel, further down) keeps all of that and ends in
// z = act(acc + bias + addend) instead of the statistics; its addend is brought to the
// accumulator layout with the inverse v_permlane32_swap and added to the un-swapped fp32 values.
#include "gfx950.h"

namespace {

constexpr int NT = 256;      // 4 waves
constexpr int BM = 64;       // rows per tile
constexpr int CHUNK = 256;   // output channels per block (64 per wave)

// x and y go through bounded buffer resources (gfx950.h) that span from a tile's first row to
// the end of the tensor, so whatever the offsets are, the hardware confines every access to
// the tensor

struct FwdArgs {
  const bf16* x; const bf16* w; bf16* y; float* sum; float* sumsq;
  long rows; int Co; int groups; int ncopy;
};

template <int K>
__global__ void __launch_bounds__(NT, 1) conv1x1_fwd_kernel(const FwdArgs a) {
  constexpr int LD = K + 8;               // LDS row of x (bf16 elements): rows 4 banks apart
  constexpr int KS = K / 16;              // MFMA k-steps
  constexpr int CPR = K / 8;              // 16-byte chunks per x row
  constexpr int RPI = NT / CPR;           // rows staged per iteration
  constexpr int CPT = BM / RPI;           // chunks per thread and tile
  static_assert(NT % CPR == 0 && BM % RPI == 0, "x tile staging");
  __shared__ __attribute__((aligned(16))) bf16 sX[2][BM * LD];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l32 = lane & 31, h = lane >> 5;
  const long rows = a.rows;
  const int ntiles = (int)((rows + BM - 1) / BM);
  const int G = a.groups, nch = a.Co / CHUNK;
  // (row group, chunk) of this block; with G % 8 == 0 the chunks of a row group share an XCD
  int rg, chunk;
  if ((G & 7) == 0) {
    const int q = blockIdx.x >> 3;
    chunk = q % nch;
    rg = (q / nch) * 8 + (blockIdx.x & 7);
  } else {
    chunk = blockIdx.x % nch;
    rg = blockIdx.x / nch;
  }
  if (rg >= ntiles) return;
  const int cb = chunk * CHUNK + wv * 64;   // first channel of this wave

  // ---- this wave's 64 x K slice of W as A-fragments: lane (l32, h) holds
  //      W[cb + 32 i + l32][16 s + 8 h .. + 7], the k mapping of igemm's read_frag
  bf16x8 wf[2][KS];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < KS; ++s)
      wf[i][s] = ldfrag(a.w + (long)(cb + 32 * i + l32) * K + s * 16 + h * 8);

  // per-lane statistics of channel cb + 32 i + (r & 3) + 8 (r >> 2) + 4 h over rows = l32 mod 32
  f32x16 s1[2], s2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { s1[i][r] = 0.f; s2[i][r] = 0.f; }

  // staging: chunk xc of rows xr0 + RPI * u of the tile
  const int xc = t % CPR, xr0 = t / CPR;
  uint4 xv[CPT];
  // rows of `tile` inside the tensor (0 past the last tile: every offset out of bounds, no traffic)
  auto rows_left = [&](int tile) {
    const long left = rows - (long)tile * BM;
    return (int)(left < 0 ? 0 : left > BM ? BM : left);
  };
  unsigned xoff[CPT];
#pragma unroll
  for (int u = 0; u < CPT; ++u) xoff[u] = (unsigned)((xr0 + RPI * u) * K + xc * 8) * 2u;
  auto prefetch = [&](int tile) {
    const int left = rows_left(tile);
    const long m0 = left > 0 ? (long)tile * BM : 0;
    const Rsrc rs = rsrc(a.x + m0 * K, (rows - m0) * K * 2);
#pragma unroll
    for (int u = 0; u < CPT; ++u) xv[u] = bload(rs, xr0 + RPI * u < left ? xoff[u] : OOB);
  };

  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < CPT; ++u) *reinterpret_cast<uint4*>(sX[buf] + (xr0 + RPI * u) * LD + xc * 8) = xv[u];
  };

  // software pipeline: entering the loop, this block's tile is in LDS buffer `buf` (not yet
  // fenced) and the following tile's loads are in flight; the loop stages them after the
  // tile's stores have been issued, so the wait is a counted vmcnt, never a drain
  int tile = rg, buf = 0;
  // W has landed before the first x load is issued: otherwise its waits end up inside the
  // loop, where they would also wait for the tile in flight
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
  prefetch(tile);
  stage(0);
  prefetch(tile + G);
#pragma unroll 1
  for (; tile < ntiles; tile += G, buf ^= 1) {
    const long m0 = (long)tile * BM;
    const bf16* sx = sX[buf];
    // the only barrier of the tile.  The other buffer is written at the end of this
    // iteration: every wave has passed this barrier by then, so its reads of the previous
    // tile are done
    lds_barrier();

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      bf16x8 xf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        xf[j] = *reinterpret_cast<const bf16x8*>(sx + (32 * j + l32) * LD + s * 16 + h * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][s], xf[j], acc[i][j], 0, 0, 0);
    }

    // ---- epilogue: statistics, then y from the registers.  acc[i][j][r] is channel
    //      cb + 32 i + (r & 3) + 8 (r >> 2) + 4 h of row m0 + 32 j + l32 (rows past the end
    //      were loaded as zeros: they add 0 to the sums, and their stores are out of bounds)
    const Rsrc ys = rsrc(a.y + m0 * a.Co, (rows - m0) * a.Co * 2);
    const int left = rows_left(tile);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned yoff = 32 * j + l32 < left ? (unsigned)((32 * j + l32) * a.Co + cb + 8 * h) * 2u : OOB;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[i][j][r];
          s1[i][r] += v;
          s2[i][r] += v * v;
        }
        // channel groups q, q + 1 (4 channels per half-wave each): after the half exchange
        // lanes 0-31 hold the 8 channels of group q, lanes 32-63 those of group q + 1
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
          uint32_t a0 = pack2_bf16(acc[i][j][4 * q], acc[i][j][4 * q + 1]);
          uint32_t a1 = pack2_bf16(acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
          uint32_t b0 = pack2_bf16(acc[i][j][4 * q + 4], acc[i][j][4 * q + 5]);
          uint32_t b1 = pack2_bf16(acc[i][j][4 * q + 6], acc[i][j][4 * q + 7]);
          const auto e0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          const auto e1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          bstore(ys, yoff, (32 * i + 8 * q) * 2, make_uint4(e0[0], e1[0], e0[1], e1[1]));
        }
      }
    }
    // keep the staging behind the stores: hoisted, its wait for the loads would stall the MFMAs
    __builtin_amdgcn_sched_barrier(0);
    stage(buf ^ 1);
    prefetch(tile + 2 * G);
  }

  // ---- leave: fold the 32 lanes that share a channel, one set of atomics per block ----------
  float* d1 = a.sum + (size_t)((unsigned)rg % (unsigned)a.ncopy) * a.Co;
  float* d2 = a.sumsq + (size_t)((unsigned)rg % (unsigned)a.ncopy) * a.Co;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float u = s1[i][r], v = s2[i][r];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) { u += __shfl_xor(u, o, 64); v += __shfl_xor(v, o, 64); }
      if (l32 == 0) {
        const int c = cb + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
        atomicAdd(d1 + c, u);
        atomicAdd(d2 + c, v);
      }
    }
}

// ---------------------------------------------------------------- inference form
// z[rows][Co] = act(x . W^T + bias[co] + addend[m][co]): a BN-folded conv unit (bias = folded
// shift, addend = the bottleneck's shortcut), the arithmetic of igemm's EpiRes in EpiRes's order
// - v = acc + bias; v += float(addend); ReLU; one rounding to bf16 - on the accumulators of the
// kernel above, so z equals mlc_conv_fwd_res's element for element.  Grid, (row group, chunk)
// mapping, weight fragments, x pipeline and k order are those of conv1x1_fwd_kernel; there are
// no statistics and no atomics, so the result does not depend on the order of the blocks.
//   * bias: a lane's 32 channels (cb + 32 i + (r & 3) + 8 (r >> 2) + 4 h) are read once per
//     block, before the row loop, through a resource of Co floats (none: 0 bytes, reads 0);
//   * addend: 8 16-byte buffer loads per lane and tile at the channel offsets of the 16-byte
//     stores, issued before the tile's barrier so they fly during its MFMAs.  Exchange choice:
//     the addend is brought to the accumulator layout - v_permlane32_swap is its own inverse,
//     so swapping dwords (0, 2) and (1, 3) of a loaded 16 bytes gives each half-wave the bf16
//     pairs of its own 2 x 4 channels - and is added to the un-swapped fp32 accumulators; the
//     packed results then take the store's swap as in the kernel above;
//   * the addend resource ends with the last valid element, ((rows - m0 - 1) * lda + Co) * 2
//     bytes from the tile's first row: the addend may be the leading channels of a wider buffer
//     that ends there.  Rows past the end use OOB: they read 0 and their stores are dropped.
struct ResArgs {
  const bf16* x; const bf16* w; bf16* y; const float* bias; const bf16* addend;
  long rows; int Co; int groups; int lda; int relu;
};

template <int K, bool ADD>
__global__ void __launch_bounds__(NT, 1) conv1x1_fwd_res_kernel(const ResArgs a) {
  constexpr int LD = K + 8;
  constexpr int KS = K / 16;
  constexpr int CPR = K / 8;
  constexpr int RPI = NT / CPR;
  constexpr int CPT = BM / RPI;
  static_assert(NT % CPR == 0 && BM % RPI == 0, "x tile staging");
  __shared__ __attribute__((aligned(16))) bf16 sX[2][BM * LD];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l32 = lane & 31, h = lane >> 5;
  const long rows = a.rows;
  const int ntiles = (int)((rows + BM - 1) / BM);
  const int G = a.groups, nch = a.Co / CHUNK;
  int rg, chunk;
  if ((G & 7) == 0) {
    const int q = blockIdx.x >> 3;
    chunk = q % nch;
    rg = (q / nch) * 8 + (blockIdx.x & 7);
  } else {
    chunk = blockIdx.x % nch;
    rg = blockIdx.x / nch;
  }
  if (rg >= ntiles) return;
  const int cb = chunk * CHUNK + wv * 64;

  bf16x8 wf[2][KS];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < KS; ++s)
      wf[i][s] = ldfrag(a.w + (long)(cb + 32 * i + l32) * K + s * 16 + h * 8);

  // bias of acc[i][.][4 g .. 4 g + 3]: channels cb + 32 i + 8 g + 4 h .. + 3
  uint4 bv[2][4];
  {
    const Rsrc bs = rsrc(a.bias, a.bias ? (unsigned)a.Co * 4u : 0u);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) bv[i][g] = bload(bs, (unsigned)(cb + 32 * i + 8 * g + 4 * h) * 4u);
  }

  const int xc = t % CPR, xr0 = t / CPR;
  uint4 xv[CPT];
  auto rows_left = [&](int tile) {
    const long left = rows - (long)tile * BM;
    return (int)(left < 0 ? 0 : left > BM ? BM : left);
  };
  unsigned xoff[CPT];
#pragma unroll
  for (int u = 0; u < CPT; ++u) xoff[u] = (unsigned)((xr0 + RPI * u) * K + xc * 8) * 2u;
  auto prefetch = [&](int tile) {
    const int left = rows_left(tile);
    const long m0 = left > 0 ? (long)tile * BM : 0;
    const Rsrc rs = rsrc(a.x + m0 * K, (rows - m0) * K * 2);
#pragma unroll
    for (int u = 0; u < CPT; ++u) xv[u] = bload(rs, xr0 + RPI * u < left ? xoff[u] : OOB);
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < CPT; ++u) *reinterpret_cast<uint4*>(sX[buf] + (xr0 + RPI * u) * LD + xc * 8) = xv[u];
  };

  int tile = rg, buf = 0;
  // W and the bias have landed before the first x load is issued (see the kernel above)
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
  __builtin_amdgcn_sched_barrier(0);
  prefetch(tile);
  stage(0);
  prefetch(tile + G);
#pragma unroll 1
  for (; tile < ntiles; tile += G, buf ^= 1) {
    const long m0 = (long)tile * BM;
    const bf16* sx = sX[buf];
    const int left = rows_left(tile);   // >= 1 inside the loop

    // the tile's addend, in the layout of the stores: av[j][i][p] is row m0 + 32 j + l32,
    // channels cb + 32 i + 16 p + 8 h .. + 7
    uint4 av[2][2][2];
    if constexpr (ADD) {
      const Rsrc as = rsrc(a.addend + m0 * a.lda, ((rows - m0 - 1) * a.lda + a.Co) * 2);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned aoff = 32 * j + l32 < left ? (unsigned)((32 * j + l32) * a.lda + cb + 8 * h) * 2u : OOB;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int p = 0; p < 2; ++p) av[j][i][p] = bload(as, aoff, (32 * i + 16 * p) * 2);
      }
    }
    lds_barrier();

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      bf16x8 xf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        xf[j] = *reinterpret_cast<const bf16x8*>(sx + (32 * j + l32) * LD + s * 16 + h * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i][s], xf[j], acc[i][j], 0, 0, 0);
    }
    // keep the epilogue behind the MFMAs: hoisted among them, its wait for the addend would
    // also wait for the x tile issued just before it, at the start of the MFMA phase
    __builtin_amdgcn_sched_barrier(0);

    // ---- epilogue: acc[i][j][r] is channel cb + 32 i + (r & 3) + 8 (r >> 2) + 4 h of row
    //      m0 + 32 j + l32
    const Rsrc ys = rsrc(a.y + m0 * a.Co, (rows - m0) * a.Co * 2);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned yoff = 32 * j + l32 < left ? (unsigned)((32 * j + l32) * a.Co + cb + 8 * h) * 2u : OOB;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
          // ad[e]: the addend of acc[i][j][4 q + e] as two packed bf16 per dword.  The store's
          // swap maps (a0, a1 | b0, b1) to dwords (0, 1 | 2, 3); the same swap undoes it
          uint32_t ad[4] = {0u, 0u, 0u, 0u};
          if constexpr (ADD) {
            const uint4 d = av[j][i][q >> 1];
            const auto r0 = __builtin_amdgcn_permlane32_swap(d.x, d.z, false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(d.y, d.w, false, false);
            ad[0] = r0[0]; ad[1] = r1[0]; ad[2] = r0[1]; ad[3] = r1[1];
          }
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const uint4 b4 = bv[i][q + (e >> 2)];
            const uint32_t bb = (e & 3) == 0 ? b4.x : (e & 3) == 1 ? b4.y : (e & 3) == 2 ? b4.z : b4.w;
            float u = acc[i][j][4 * q + e] + __uint_as_float(bb);
            if constexpr (ADD) u += __uint_as_float((e & 1) ? ad[e >> 1] & 0xffff0000u : ad[e >> 1] << 16);
            v[e] = a.relu ? fmaxf(u, 0.f) : u;
          }
          uint32_t a0 = pack2_bf16(v[0], v[1]);
          uint32_t a1 = pack2_bf16(v[2], v[3]);
          uint32_t b0 = pack2_bf16(v[4], v[5]);
          uint32_t b1 = pack2_bf16(v[6], v[7]);
          const auto e0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          const auto e1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          bstore(ys, yoff, (32 * i + 8 * q) * 2, make_uint4(e0[0], e1[0], e0[1], e1[1]));
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    stage(buf ^ 1);
    prefetch(tile + 2 * G);
  }
}

int g_fwd_max_blocks = 0;   // 0: one block per CU

int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 256;
    n = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }
  return n;
}

}  // namespace

// 1: (Cin, Cout) has an instantiation and the mode allows it (not deterministic mode: the
// per-block statistics atomics are unordered)
MLC_EXPORT int mlc_conv1x1_fwd_ok(int Cin, int Cout) {
  return !g_mlc_det && ((Cin == 128 && Cout == 512) || (Cin == 256 && Cout == 1024));
}

// A/B knob: key 0 = block cap (0 = one per CU); value < 0 only reads.  Returns the previous value.
MLC_EXPORT int mlc_conv1x1_fwd_get_set(int key, int value) {
  if (key != 0) return -1;
  const int old = g_fwd_max_blocks;
  if (value >= 0) g_fwd_max_blocks = value;
  return old;
}

// y[rows][Cout] = x[rows][Cin] . w[Cout][Cin]^T (bf16, dense rows); sum / sumsq: the BN's
// ncopy * Cout fp32 partial sums of y and y^2, ADDED to (as mlc_conv_fwd does).
// -1: no instantiation for the shape / mode, or no statistics buffers.
MLC_EXPORT int mlc_conv1x1_fwd(const bf16* x, const bf16* w, bf16* y, float* sum, float* sumsq, long rows,
                               int Cin, int Cout, hipStream_t st) {
  if (!mlc_conv1x1_fwd_ok(Cin, Cout) || !sum || !sumsq || rows < 1 || rows > (1L << 36)) return -1;
  const int nch = Cout / CHUNK;
  const long ntiles = (rows + BM - 1) / BM;
  long groups = (g_fwd_max_blocks > 0 ? g_fwd_max_blocks : cu_count()) / nch;
  if (groups > ntiles) groups = ntiles;
  if (groups < 1) groups = 1;
  const FwdArgs a{x, w, y, sum, sumsq, rows, Cout, (int)groups, g_mlc_ncopy};
  const dim3 grid((unsigned)(groups * nch));
  if (Cin == 128) hipLaunchKernelGGL((conv1x1_fwd_kernel<128>), grid, dim3(NT), 0, st, a);
  else hipLaunchKernelGGL((conv1x1_fwd_kernel<256>), grid, dim3(NT), 0, st, a);
  return hipGetLastError();
}

// 1: the inference form has an instantiation for (Cin, Cout).  Nothing in it is unordered, so
// deterministic mode takes it too.
MLC_EXPORT int mlc_conv1x1_fwd_res_ok(int Cin, int Cout) {
  return (Cin == 128 && Cout == 512) || (Cin == 256 && Cout == 1024);
}

// Inference 1x1 unit: y[rows][Cout] = act(x[rows][Cin] . w[Cout][Cin]^T + bias + addend), the
// operands and the result of mlc_conv_fwd_res for a 1x1 / stride-1 / pad-0 conv: act 0 or
// 3 = ReLU; bias ([Cout] fp32) and addend (bf16, rows of lda >= Cout elements, lda % 8 == 0,
// 16-byte aligned) are optional.  -1: no instantiation for the shape, act outside {0, 3}, a bad
// lda, or rows < 1.  The block cap of mlc_conv1x1_fwd_get_set key 0 applies.
MLC_EXPORT int mlc_conv1x1_fwd_res(const bf16* x, const bf16* w, bf16* y, const float* bias, int act,
                                   const bf16* addend, int lda, long rows, int Cin, int Cout, hipStream_t st) {
  if (!mlc_conv1x1_fwd_res_ok(Cin, Cout) || (act != 0 && act != 3) || rows < 1 || rows > (1L << 36)) return -1;
  // 64 rows of lda elements stay far inside the 31 bits of a buffer offset
  if (addend && (lda < Cout || lda % 8 || lda > (1 << 20))) return -1;
  const int nch = Cout / CHUNK;
  const long ntiles = (rows + BM - 1) / BM;
  long groups = (g_fwd_max_blocks > 0 ? g_fwd_max_blocks : cu_count()) / nch;
  if (groups > ntiles) groups = ntiles;
  if (groups < 1) groups = 1;
  const ResArgs a{x, w, y, bias, addend, rows, Cout, (int)groups, lda, act == 3};
  const dim3 grid((unsigned)(groups * nch));
  if (Cin == 128) {
    if (addend) hipLaunchKernelGGL((conv1x1_fwd_res_kernel<128, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((conv1x1_fwd_res_kernel<128, false>), grid, dim3(NT), 0, st, a);
  } else {
    if (addend) hipLaunchKernelGGL((conv1x1_fwd_res_kernel<256, true>), grid, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((conv1x1_fwd_res_kernel<256, false>), grid, dim3(NT), 0, st, a);
  }
  return hipGetLastError();
}
