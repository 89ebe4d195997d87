// Backward of a narrow-in / wide-out 1x1 ConvBN unit in ONE streaming kernel:
//   dy = k1*dz + k2 + k3*(y - mean)     (BN-backward apply, formed on the fly, never stored)
//   dx = dy . W  (+ addend) (masked + reduced for the previous BN, as the igemm dgrad does)
//   dW += dy^T . x
// The three-kernel path (bn_bwd_fused -> dgrad -> wgrad) writes dy (as wide as the unit's
// output) once and reads it twice; here a row tile of dz / y / x is read once, dy lives in
// LDS for the two GEMMs of the tile, and the only wide traffic is the two compulsory reads.
//
// One persistent block of 4 waves per CU loops over 64-row tiles:
//   * the NEXT tile's global loads (dz, y, x, addend, previous y) are issued into registers
//     as soon as the current tile's registers are consumed, and fly during the tile's MFMAs;
//   * dy is rounded to bf16 exactly where bn_bwd_fused_kernel rounds it and staged twice:
//     row-major [r][co] (A operand of dx = dy.W) and transposed [co][r] (A operand of
//     dW = dy^T.x; a thread owns an 8-row x 8-channel patch, so both are 16-byte writes);
//   * W sits in LDS transposed ([ci][co], loaded once per block), x transposed [ci][r];
//   * the dW accumulators (Cout x Cin fp32, 64 registers per lane) stay in registers over the
//     whole row loop and leave with one set of fp32 atomics per block; the previous BN's
//     partial sums stay in registers too and leave with one set of atomics per block.
// (k1, k2, k3) come from the NSTAT partial copies in the prologue, summed in the order
// bn_bwd_fused_kernel sums them; block 0 publishes dgamma / dbeta.
#include "common.h"

namespace {

constexpr int NT = 256;   // 4 waves
constexpr int BM = 64;    // rows per tile

struct C1x1Args {
  const bf16* dz; const bf16* y; const bf16* x; const bf16* w;
  const float* mean; const float* invstd; const float* gamma; const float* sums; int ncopy;
  float* dgamma; float* dbeta; float* dw;
  bf16* dx; const bf16* addend;            // dx may alias addend
  // previous BN (single-y affine ReLU form of BnBwdSpec), all null when absent
  const bf16* py; const float* pmean; float* psums; const float* psc; const float* psh; int pncopy;
  long rows;
};

template <int CI, int CO>
__global__ void __launch_bounds__(NT, 1) conv1x1_bn_bwd_kernel(const C1x1Args a) {
  static_assert(CI == 64 && CO == 256, "tile geometry below is laid out for (64, 256)");
  constexpr int LDA = CO + 8;   // row-major dy / transposed W rows (bf16 elements)
  constexpr int LDT = BM + 8;   // transposed dy / x rows
  constexpr int LDO = CI + 8;   // dx staging rows (over sA)
  constexpr int GO = CO / 8, GI = CI / 8;
  __shared__ __attribute__((aligned(16))) bf16 sW[CI * LDA];   // [ci][co]
  __shared__ __attribute__((aligned(16))) bf16 sA[BM * LDA];   // dy [r][co]; then dx [r][ci]
  __shared__ __attribute__((aligned(16))) bf16 sT[CO * LDT];   // dy [co][r]
  __shared__ __attribute__((aligned(16))) bf16 sX[CI * LDT];   // x  [ci][r]
  __shared__ float sk[4][CO];
  static_assert(sizeof(float) * NT * 16 <= sizeof(bf16) * CO * LDT, "final reduction reuses sT");

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l32 = lane & 31, h = lane >> 5;
  const long rows = a.rows;
  const int ntiles = (int)((rows + BM - 1) / BM);

  // ---- prologue: (k1, k2, k3, mean) of this unit's BN; W -> LDS, transposed -------------
  for (int c = t; c < CO; c += NT) {
    float S1 = 0.f, S2 = 0.f;
#pragma unroll 16
    for (int k = 0; k < a.ncopy; ++k) {
      S1 += a.sums[(long)k * 2 * CO + c];
      S2 += a.sums[(long)k * 2 * CO + CO + c];
    }
    const float invM = 1.f / (float)rows;
    const float is = a.invstd[c];
    const float k1 = a.gamma[c] * is;
    sk[0][c] = k1;
    sk[1][c] = -k1 * S1 * invM;
    sk[2][c] = -k1 * is * is * S2 * invM;
    sk[3][c] = a.mean[c];
    if (blockIdx.x == 0 && a.dgamma) { a.dgamma[c] = S2 * is; a.dbeta[c] = S1; }
  }
  for (int co = t; co < CO; co += NT) {
    uint4 wr[GI];
#pragma unroll
    for (int g = 0; g < GI; ++g) wr[g] = ldg16(a.w + (long)co * CI + g * 8);
#pragma unroll
    for (int g = 0; g < GI; ++g) {
      const uint32_t q[4] = {wr[g].x, wr[g].y, wr[g].z, wr[g].w};
#pragma unroll
      for (int e = 0; e < 8; ++e)
        reinterpret_cast<unsigned short*>(sW)[(g * 8 + e) * LDA + co] =
            (unsigned short)((q[e >> 1] >> (16 * (e & 1))) & 0xffffu);
    }
  }
  __syncthreads();

  // dy patch of this thread: rows 8*rb .. 8*rb+7, channels 8*g .. 8*g+7
  const int g = t % GO, rb = t / GO;
  static_assert(NT / GO * 8 == BM, "one 8x8 dy patch per thread");
  float k1[8], k2[8], k3[8], mu[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    k1[e] = sk[0][g * 8 + e]; k2[e] = sk[1][g * 8 + e]; k3[e] = sk[2][g * 8 + e]; mu[e] = sk[3][g * 8 + e];
  }
  // x patch: rows 2*xr, 2*xr+1, channels 8*xg ..; dx chunk: rows er + 32*u, channels 8*ec ..
  const int xg = t % GI, xr = (t / GI) * 2;
  static_assert(NT / GI * 2 == BM, "one 2x8 x patch per thread");
  const int ec = t % GI, er = t / GI;
  static_assert(NT / GI * 2 == BM, "two dx chunks per thread");
  const bool red = a.py != nullptr, has_add = a.addend != nullptr;
  float pmu[8], pa[8], pb[8], ps1[8], ps2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { pmu[e] = 0.f; pa[e] = 0.f; pb[e] = 0.f; ps1[e] = 0.f; ps2[e] = 0.f; }
  if (red) { ldg8f(a.pmean + ec * 8, pmu); ldg8f(a.psc + ec * 8, pa); ldg8f(a.psh + ec * 8, pb); }

  f32x16 accW[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) accW[i][j][r] = 0.f;

  uint4 dv[8], yv[8], xv[2], aaN[2], ppN[2];
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  // every row index is clamped to the last row: always a valid address; rows past the end
  // contribute zeros (dy, x) and are never stored (dx)
  auto prefetch = [&](int tile) {
    const long m0 = (long)(tile < ntiles ? tile : ntiles - 1) * BM;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long r = min(m0 + rb * 8 + j, rows - 1);
      dv[j] = ldg16(a.dz + (r * GO + g) * 8);
      yv[j] = ldg16(a.y + (r * GO + g) * 8);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long r = min(m0 + xr + j, rows - 1);
      xv[j] = ldg16(a.x + (r * GI + xg) * 8);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long r = min(m0 + er + 32 * u, rows - 1);
      aaN[u] = has_add ? ldg16(a.addend + (r * GI + ec) * 8) : zero4;
      ppN[u] = red ? ldg16(a.py + (r * GI + ec) * 8) : zero4;
    }
  };

  int tile = blockIdx.x;
  if (tile < ntiles) prefetch(tile);
#pragma unroll 1
  for (; tile < ntiles; tile += gridDim.x) {
    const long m0 = (long)tile * BM;
    // ---- consume the registers of this tile ------------------------------------------
    float o[8][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float d[8], yy[8];
      unpack8(dv[j], d);
      unpack8(yv[j], yy);
      const bool in = m0 + rb * 8 + j < rows;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = k1[e] * d[e] + k2[e] + k3[e] * (yy[e] - mu[e]);
        o[j][e] = in ? v : 0.f;
      }
    }
    uint4 xc[2], aa[2], pp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      xc[j] = m0 + xr + j < rows ? xv[j] : zero4;
      aa[j] = aaN[j];
      pp[j] = ppN[j];
    }
    prefetch(tile + (int)gridDim.x);   // past the end: the last tile again, unused
    // ---- stage dy (both layouts) and x ------------------------------------------------
#pragma unroll
    for (int j = 0; j < 8; ++j)
      *reinterpret_cast<uint4*>(sA + (rb * 8 + j) * LDA + g * 8) = pack8(o[j]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      uint4 q;
      q.x = pack2_bf16(o[0][e], o[1][e]);
      q.y = pack2_bf16(o[2][e], o[3][e]);
      q.z = pack2_bf16(o[4][e], o[5][e]);
      q.w = pack2_bf16(o[6][e], o[7][e]);
      *reinterpret_cast<uint4*>(sT + (g * 8 + e) * LDT + rb * 8) = q;
    }
    {
      const uint32_t q0[4] = {xc[0].x, xc[0].y, xc[0].z, xc[0].w};
      const uint32_t q1[4] = {xc[1].x, xc[1].y, xc[1].z, xc[1].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t lo = (q0[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        const uint32_t hi = (q1[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        *reinterpret_cast<uint32_t*>(sX + (xg * 8 + e) * LDT + xr) = lo | (hi << 16);
      }
    }
    __syncthreads();
    // ---- dx tile = dy[64 x CO] . W[CO x CI]: wave (wm, wn) owns a 32 x 32 block --------
    const int wm = wv >> 1, wn = wv & 1;
    f32x16 accD;
#pragma unroll
    for (int r = 0; r < 16; ++r) accD[r] = 0.f;
#pragma unroll
    for (int s = 0; s < CO / 16; ++s) {
      const bf16x8 fa = *reinterpret_cast<const bf16x8*>(sA + (wm * 32 + l32) * LDA + s * 16 + h * 8);
      const bf16x8 fb = *reinterpret_cast<const bf16x8*>(sW + (wn * 32 + l32) * LDA + s * 16 + h * 8);
      accD = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, accD, 0, 0, 0);
    }
    // ---- dW[co][ci] += dy^T . x: wave wv owns channels 64*wv .. 64*wv+63 ---------------
#pragma unroll
    for (int s = 0; s < BM / 16; ++s) {
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fa[i] = *reinterpret_cast<const bf16x8*>(sT + (wv * 64 + i * 32 + l32) * LDT + s * 16 + h * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(sX + (j * 32 + l32) * LDT + s * 16 + h * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          accW[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], accW[i][j], 0, 0, 0);
    }
    __syncthreads();   // sA is free: it takes the dx tile (bf16, as the igemm epilogue stages it)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      sA[m * LDO + wn * 32 + l32] = (bf16)accD[r];
    }
    __syncthreads();
    // ---- dx epilogue: + addend, ReLU mask of the previous BN, its sums, 16-byte stores --
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int row = er + 32 * u;
      const long m = m0 + row;
      if (m >= rows) continue;
      uint4 v = *reinterpret_cast<const uint4*>(sA + row * LDO + ec * 8);
      if (has_add || red) {
        float f[8];
        unpack8(v, f);
        if (has_add) {
          float b[8];
          unpack8(aa[u], b);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] += b[e];
        }
        float yp[8];
        unpack8(pp[u], yp);
        if (red) {
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = yp[e] * pa[e] + pb[e] > 0.f ? f[e] : 0.f;
        }
        v = pack8(f);
        if (red) {
          unpack8(v, f);   // reduce exactly the bf16 values that are stored
#pragma unroll
          for (int e = 0; e < 8; ++e) { ps1[e] += f[e]; ps2[e] += f[e] * (yp[e] - pmu[e]); }
        }
      }
      *reinterpret_cast<uint4*>(a.dx + (m * GI + ec) * 8) = v;
    }
    __syncthreads();   // the next tile's staging overwrites sA
  }

  // ---- leave: the block's dW and the previous BN's partial sums, one set of atomics -----
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = wv * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        atomicAdd(a.dw + (long)co * CI + j * 32 + l32, accW[i][j][r]);
      }
  if (red) {
    float* rbuf = reinterpret_cast<float*>(sT);   // [NT][16]
#pragma unroll
    for (int e = 0; e < 8; ++e) { rbuf[t * 16 + e] = ps1[e]; rbuf[t * 16 + 8 + e] = ps2[e]; }
    __syncthreads();
    if (t < CI) {
      const int cc = t >> 3, e = t & 7;
      float s1 = 0.f, s2 = 0.f;
      for (int r = 0; r < NT / GI; ++r) {
        const float* q = rbuf + (cc + GI * r) * 16;
        s1 += q[e];
        s2 += q[8 + e];
      }
      float* d0 = a.psums + (size_t)(blockIdx.x % (unsigned)a.pncopy) * 2 * CI;
      atomicAdd(d0 + t, s1);
      atomicAdd(d0 + CI + t, s2);
    }
  }
}

int g_c1x1_max_blocks = 0;   // 0: one block per CU

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

// 1: (Cin, Cout) has a fused instantiation and the mode allows it (not deterministic mode:
// the block-level atomics are unordered)
MLC_EXPORT int mlc_conv1x1_bn_bwd_ok(int Cin, int Cout) {
  return !g_mlc_det && Cin == 64 && Cout == 256;
}

// A/B knob: key 0 = block cap (0 = one per CU); value < 0 only reads.  Returns the previous value.
MLC_EXPORT int mlc_conv1x1_bwd_get_set(int key, int value) {
  if (key != 0) return -1;
  const int old = g_c1x1_max_blocks;
  if (value >= 0) g_c1x1_max_blocks = value;
  return old;
}

// Fused backward of a 1x1 / stride-1 / pad-0 ConvBN unit over `rows` pixels.
//   dz, y [rows][Cout], x [rows][Cin], w [Cout][Cin] bf16; sums: the BN's NSTAT*2*Cout
//   partial sums (complete on entry); dw fp32 [Cout][Cin] is ADDED to; dx [rows][Cin]
//   (may alias addend).  p*: the previous BN of a single-y affine BnBwdSpec (py null: none);
//   psums its NSTAT*2*Cin scratch.  -1: no instantiation for the shape / mode.
MLC_EXPORT int mlc_conv1x1_bn_bwd(const bf16* dz, const bf16* y, const bf16* x, const bf16* w, const float* mean,
                                  const float* invstd, const float* gamma, const float* sums, float* dgamma,
                                  float* dbeta, float* dw, bf16* dx, const bf16* addend, const bf16* py,
                                  const float* pmean, float* psums, const float* psc, const float* psh, long rows,
                                  int Cin, int Cout, hipStream_t st) {
  if (!mlc_conv1x1_bn_bwd_ok(Cin, Cout) || rows < 1 || rows > (1L << 36)) return -1;
  if (py && (!pmean || !psums || !psc || !psh)) return -1;
  const C1x1Args a{dz, y, x, w, mean, invstd, gamma, sums, g_mlc_ncopy, dgamma, dbeta, dw, dx, addend,
                   py, pmean, psums, psc, psh, g_mlc_ncopy, rows};
  const long ntiles = (rows + BM - 1) / BM;
  long blocks = g_c1x1_max_blocks > 0 ? g_c1x1_max_blocks : cu_count();
  if (blocks > ntiles) blocks = ntiles;
  hipLaunchKernelGGL((conv1x1_bn_bwd_kernel<64, 256>), dim3((unsigned)blocks), dim3(NT), 0, st, a);
  return hipGetLastError();
}
