// Device half of the native input pipeline (host half: csrc/runtime/records.cpp).
//
// src: a batch of raw uint8 HWC records [B][H][W][C] (C <= 4, copied to the device as
// is); par: per sample {y0, x0, h, w, flip} - the source box of a RandomResizedCrop /
// centre crop and a horizontal flip.  One pass crops, resizes the box to oh x ow
// (bilinear, half-pixel centres, clamped at the box edge: torchvision's Resize of the
// cropped region, antialias off), flips, normalises (x - mean) / std and writes:
//   layout 0: the native ResNet stem's 2x2 space-to-depth image of the pad-3 image,
//             bf16 [B][(oh+6)/2][(ow+6)/2][16], channel (dy*2+dx)*3 + ci, 12..15 zero
//             (ops.functional.stem_s2d layout);
//   layout 1: NHWC bf16 with channels padded to 8;
//   layout 2: NCHW fp32 (the torch engine).
#include "common.h"

namespace {

constexpr int NT = 256;

struct Box {
  float y0, x0, sy, sx;   // source box origin and scale (box / output)
  int h, w, flip;
};

__device__ __forceinline__ Box box(const int* par, int b, int oh, int ow) {
  const int* p = par + 5 * b;
  Box r;
  r.y0 = (float)p[0]; r.x0 = (float)p[1]; r.h = p[2]; r.w = p[3]; r.flip = p[4];
  r.sy = (float)r.h / (float)oh;
  r.sx = (float)r.w / (float)ow;
  return r;
}

// bilinear sample of the box at row u / column v of its resize (scales sy, sx = box /
// grid): out[c] for c < C.  Half-pixel centres, clamped at the box edge.
template <int C>
__device__ __forceinline__ void sample_at(const uint8_t* img, int W, const Box& bx, int u, int v, float sy,
                                          float sx, float* out) {
  float fy = ((float)u + 0.5f) * sy - 0.5f, fx = ((float)v + 0.5f) * sx - 0.5f;
  fy = fminf(fmaxf(fy, 0.f), (float)(bx.h - 1));
  fx = fminf(fmaxf(fx, 0.f), (float)(bx.w - 1));
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = min(y0 + 1, bx.h - 1), x1 = min(x0 + 1, bx.w - 1);
  const float wy = fy - (float)y0, wx = fx - (float)x0;
  const int by = (int)bx.y0, bxo = (int)bx.x0;
  const uint8_t* p00 = img + ((size_t)(by + y0) * W + bxo + x0) * C;
  const uint8_t* p01 = img + ((size_t)(by + y0) * W + bxo + x1) * C;
  const uint8_t* p10 = img + ((size_t)(by + y1) * W + bxo + x0) * C;
  const uint8_t* p11 = img + ((size_t)(by + y1) * W + bxo + x1) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float top = (float)p00[c] + wx * ((float)p01[c] - (float)p00[c]);
    const float bot = (float)p10[c] + wx * ((float)p11[c] - (float)p10[c]);
    out[c] = top + wy * (bot - top);
  }
}

// the classification transform at output pixel (oy, ox): horizontal flip, then the sample
template <int C>
__device__ __forceinline__ void sample(const uint8_t* img, int W, const Box& bx, int oy, int ox, int ow,
                                       float* out) {
  if (bx.flip) ox = ow - 1 - ox;
  sample_at<C>(img, W, bx, oy, ox, bx.sy, bx.sx, out);
}

template <int C>
__global__ void __launch_bounds__(NT)
augment_s2d_kernel(const uint8_t* __restrict__ src, const int* __restrict__ par, const float* __restrict__ ms,
                   bf16* __restrict__ out, int B, int H, int W, int oh, int ow, int Hb, int Wb) {
  const long total = (long)B * Hb * Wb;
  for (long q = (long)blockIdx.x * NT + threadIdx.x; q < total; q += (long)gridDim.x * NT) {
    const int j = (int)(q % Wb);
    const long t = q / Wb;
    const int i = (int)(t % Hb);
    const int b = (int)(t / Hb);
    const Box bx = box(par, b, oh, ow);
    const uint8_t* img = src + (size_t)b * H * W * C;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int oy = 2 * i + dy - 3, ox = 2 * j + dx - 3;   // stem padding 3
        if ((unsigned)oy < (unsigned)oh && (unsigned)ox < (unsigned)ow) {
          float f[C];
          sample<C>(img, W, bx, oy, ox, ow, f);
#pragma unroll
          for (int c = 0; c < 3 && c < C; ++c) v[(dy * 2 + dx) * 3 + c] = (f[c] - ms[c]) * ms[4 + c];
        }
      }
    uint4* dst = reinterpret_cast<uint4*>(out + q * 16);
    dst[0] = pack8(v);
    dst[1] = pack8(v + 8);
  }
}

template <int C>
__global__ void __launch_bounds__(NT)
augment_pix_kernel(const uint8_t* __restrict__ src, const int* __restrict__ par, const float* __restrict__ ms,
                   void* __restrict__ out, int B, int H, int W, int oh, int ow, int layout) {
  const long total = (long)B * oh * ow;
  for (long q = (long)blockIdx.x * NT + threadIdx.x; q < total; q += (long)gridDim.x * NT) {
    const int ox = (int)(q % ow);
    const long t = q / ow;
    const int oy = (int)(t % oh);
    const int b = (int)(t / oh);
    const Box bx = box(par, b, oh, ow);
    float f[C];
    sample<C>(src + (size_t)b * H * W * C, W, bx, oy, ox, ow, f);
    if (layout == 1) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = (f[c] - ms[c]) * ms[4 + c];
      *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(out) + q * 8) = pack8(v);
    } else {
      float* o = reinterpret_cast<float*>(out);
#pragma unroll
      for (int c = 0; c < C; ++c) o[(((size_t)b * C + c) * oh + oy) * ow + ox] = (f[c] - ms[c]) * ms[4 + c];
    }
  }
}

// ---- segmentation: image + mask under one geometric transform (mlc_augment_seg) ----
// par: per sample {y0, x0, h, w, hflip, vflip, transpose, 0}.  Output pixel (oy, ox) reads
// the box at row u of gh and column v of gw:
//   transpose ? (u, v, gh, gw) = (ox, oy, ow, oh) : (oy, ox, oh, ow);
//   hflip: v = gw-1-v;  vflip: u = gh-1-u.
// The image is sample_at(u, v) with scales h/gh, w/gw; the mask is the nearest source
// pixel in integers, row ((2u+1)*h) / (2*gh), column ((2v+1)*w) / (2*gw), which lies in
// the box without clamping.
struct SegBox {
  Box bx;   // origin, size and the scales h/gh, w/gw (flip unused)
  int y0, x0, gh, gw, hflip, vflip, tr;
};

// The box is clamped into the image, so no par can make a thread read outside
// [0,H) x [0,W); a box the host loader draws is unchanged by it.
__device__ __forceinline__ SegBox seg_box(const int* par, int b, int H, int W, int oh, int ow) {
  const int* p = par + 8 * b;
  SegBox s;
  s.y0 = min(max(p[0], 0), H - 1);
  s.x0 = min(max(p[1], 0), W - 1);
  s.bx.h = min(max(p[2], 1), H - s.y0);
  s.bx.w = min(max(p[3], 1), W - s.x0);
  s.hflip = p[4]; s.vflip = p[5]; s.tr = p[6];
  s.gh = s.tr ? ow : oh;
  s.gw = s.tr ? oh : ow;
  s.bx.y0 = (float)s.y0; s.bx.x0 = (float)s.x0; s.bx.flip = 0;
  s.bx.sy = (float)s.bx.h / (float)s.gh;
  s.bx.sx = (float)s.bx.w / (float)s.gw;
  return s;
}

__device__ __forceinline__ void seg_coord(const SegBox& s, int oy, int ox, int& u, int& v) {
  u = s.tr ? ox : oy;
  v = s.tr ? oy : ox;
  if (s.hflip) v = s.gw - 1 - v;
  if (s.vflip) u = s.gh - 1 - u;
}

// mask of output pixel `pix` (= (b*oh + oy)*ow + ox) from grid position (u, v): planes
// (kind 0) fp32 0/1 [pix][K], index (kind 1) int64 [pix]
__device__ __forceinline__ void write_mask(const uint8_t* mask, int W, int K, int kind, const SegBox& s, int u,
                                           int v, void* out, long pix) {
  const int row = ((2 * u + 1) * s.bx.h) / (2 * s.gh), col = ((2 * v + 1) * s.bx.w) / (2 * s.gw);
  const uint8_t* m = mask + ((size_t)(s.y0 + row) * W + s.x0 + col) * K;
  if (kind == 1) {
    reinterpret_cast<long long*>(out)[pix] = (long long)m[0];
  } else if (K == 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(m);
    float4 f;
    f.x = (w & 0xffu) ? 1.f : 0.f;
    f.y = (w & 0xff00u) ? 1.f : 0.f;
    f.z = (w & 0xff0000u) ? 1.f : 0.f;
    f.w = (w & 0xff000000u) ? 1.f : 0.f;
    reinterpret_cast<float4*>(out)[pix] = f;
  } else {
    float* o = reinterpret_cast<float*>(out) + pix * K;
    for (int k = 0; k < K; ++k) o[k] = m[k] ? 1.f : 0.f;
  }
}

__global__ void __launch_bounds__(NT)
augment_seg_s2d_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ msk,
                       const int* __restrict__ par, const float* __restrict__ ms, bf16* __restrict__ out,
                       void* __restrict__ out_mask, int B, int H, int W, int K, int kind, int oh, int ow, int Hb,
                       int Wb) {
  constexpr int C = 3;
  const long total = (long)B * Hb * Wb;
  for (long q = (long)blockIdx.x * NT + threadIdx.x; q < total; q += (long)gridDim.x * NT) {
    const int j = (int)(q % Wb);
    const long t = q / Wb;
    const int i = (int)(t % Hb);
    const int b = (int)(t / Hb);
    const SegBox s = seg_box(par, b, H, W, oh, ow);
    const uint8_t* img = src + (size_t)b * H * W * C;
    const uint8_t* mask = msk + (size_t)b * H * W * K;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int oy = 2 * i + dy - 3, ox = 2 * j + dx - 3;   // stem padding 3
        if ((unsigned)oy < (unsigned)oh && (unsigned)ox < (unsigned)ow) {
          int gu, gv;
          seg_coord(s, oy, ox, gu, gv);
          float f[C];
          sample_at<C>(img, W, s.bx, gu, gv, s.bx.sy, s.bx.sx, f);
#pragma unroll
          for (int c = 0; c < C; ++c) v[(dy * 2 + dx) * 3 + c] = (f[c] - ms[c]) * ms[4 + c];
          write_mask(mask, W, K, kind, s, gu, gv, out_mask, ((long)b * oh + oy) * ow + ox);
        }
      }
    uint4* dst = reinterpret_cast<uint4*>(out + q * 16);
    dst[0] = pack8(v);
    dst[1] = pack8(v + 8);
  }
}

template <int C>
__global__ void __launch_bounds__(NT)
augment_seg_pix_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ msk,
                       const int* __restrict__ par, const float* __restrict__ ms, void* __restrict__ out,
                       void* __restrict__ out_mask, int B, int H, int W, int K, int kind, int oh, int ow,
                       int layout) {
  const long total = (long)B * oh * ow;
  for (long q = (long)blockIdx.x * NT + threadIdx.x; q < total; q += (long)gridDim.x * NT) {
    const int ox = (int)(q % ow);
    const long t = q / ow;
    const int oy = (int)(t % oh);
    const int b = (int)(t / oh);
    const SegBox s = seg_box(par, b, H, W, oh, ow);
    int gu, gv;
    seg_coord(s, oy, ox, gu, gv);
    float f[C];
    sample_at<C>(src + (size_t)b * H * W * C, W, s.bx, gu, gv, s.bx.sy, s.bx.sx, f);
    if (layout == 1) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = (f[c] - ms[c]) * ms[4 + c];
      *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(out) + q * 8) = pack8(v);
    } else {
      float* o = reinterpret_cast<float*>(out);
#pragma unroll
      for (int c = 0; c < C; ++c) o[(((size_t)b * C + c) * oh + oy) * ow + ox] = (f[c] - ms[c]) * ms[4 + c];
    }
    write_mask(msk + (size_t)b * H * W * K, W, K, kind, s, gu, gv, out_mask, q);
  }
}

// ---- video clips: one box and one flip for every frame of a clip (mlc_augment_clip) ----
// par: per clip {y0, x0, h, w, flip, t0, frame stride, 0}; t0 and the stride say which
// frames of the record the host gathered and are not read here.  The box is clamped into
// the image as seg_box does, so no par can make a thread read outside its clip.
__device__ __forceinline__ Box clip_box(const int* par, int b, int H, int W, int oh, int ow) {
  const int* p = par + 8 * b;
  const int y0 = min(max(p[0], 0), H - 1), x0 = min(max(p[1], 0), W - 1);
  Box r;
  r.h = min(max(p[2], 1), H - y0);
  r.w = min(max(p[3], 1), W - x0);
  r.y0 = (float)y0; r.x0 = (float)x0; r.flip = p[4];
  r.sy = (float)r.h / (float)oh;
  r.sx = (float)r.w / (float)ow;
  return r;
}

// one bf16 pixel of 3 channels at flattened pixel index g (6 bytes): a dword and a short,
// in the order that keeps the dword aligned
__device__ __forceinline__ void store_px3(bf16* out, long g, const float* v) {
  bf16* o = out + g * 3;
  if (g & 1) {
    o[0] = f2bf(v[0]);
    *reinterpret_cast<uint32_t*>(o + 1) = pack2_bf16(v[1], v[2]);
  } else {
    *reinterpret_cast<uint32_t*>(o) = pack2_bf16(v[0], v[1]);
    o[2] = f2bf(v[2]);
  }
}

// L = 0: fp32 [B][C][T][oh][ow];  L = 1: bf16 [B][T][oh][ow][C], exactly C channels.
// A thread owns NP output pixels of a clip (two adjacent ones of the 3-channel bf16 form,
// stored as three dwords where the flattened pixel index is even) and loops over the T
// frames: the sample position does not depend on the frame, so the clamped coordinates,
// the four tap offsets and the two weights of sample_at are loop invariants and a frame
// costs 4*C byte loads at a stride of H*W*C plus the store.
template <int C, int L>
__global__ void __launch_bounds__(NT)
augment_clip_kernel(const uint8_t* __restrict__ src, const int* __restrict__ par, const float* __restrict__ ms,
                    void* __restrict__ out, int B, int T, int H, int W, int oh, int ow) {
  constexpr int NP = (L == 1 && C == 3) ? 2 : 1;
  const long px = (long)oh * ow;   // pixels of a frame
  const long groups = (px + NP - 1) / NP;
  const long total = (long)B * groups;
  const size_t fb = (size_t)H * W * C;
  for (long q = (long)blockIdx.x * NT + threadIdx.x; q < total; q += (long)gridDim.x * NT) {
    const long pix = (q % groups) * NP;
    const int b = (int)(q / groups);
    const Box bx = clip_box(par, b, H, W, oh, ow);
    const bool two = NP == 2 && pix + 1 < px;
    const int oy0 = (int)(pix / ow), ox0 = (int)(pix % ow);
    const int oy1 = (int)((pix + 1) / ow), ox1 = (int)((pix + 1) % ow);
    const uint8_t* img = src + (size_t)b * T * fb;
    for (int t = 0; t < T; ++t, img += fb) {
      float f[C], v[NP][C];
      sample<C>(img, W, bx, oy0, ox0, ow, f);
#pragma unroll
      for (int c = 0; c < C; ++c) v[0][c] = (f[c] - ms[c]) * ms[4 + c];
      if constexpr (NP == 2) if (two) {
        sample<C>(img, W, bx, oy1, ox1, ow, f);
#pragma unroll
        for (int c = 0; c < C; ++c) v[NP - 1][c] = (f[c] - ms[c]) * ms[4 + c];
      }
      if constexpr (L == 0) {
        float* o = reinterpret_cast<float*>(out);
#pragma unroll
        for (int c = 0; c < C; ++c) o[(((size_t)b * C + c) * T + t) * px + pix] = v[0][c];
      } else {
        bf16* o = reinterpret_cast<bf16*>(out);
        const long g = ((long)b * T + t) * px + pix;   // flattened pixel index
        if constexpr (C == 1) {
          o[g] = f2bf(v[0][0]);
        } else if constexpr (C == 2) {
          reinterpret_cast<uint32_t*>(o)[g] = pack2_bf16(v[0][0], v[0][1]);
        } else if constexpr (C == 4) {
          reinterpret_cast<uint2*>(o)[g] = make_uint2(pack2_bf16(v[0][0], v[0][1]), pack2_bf16(v[0][2], v[0][3]));
        } else if (two && !(g & 1)) {
          uint32_t* d = reinterpret_cast<uint32_t*>(o + g * 3);
          d[0] = pack2_bf16(v[0][0], v[0][1]);
          d[1] = pack2_bf16(v[0][2], v[NP - 1][0]);
          d[2] = pack2_bf16(v[NP - 1][1], v[NP - 1][2]);
        } else {
          store_px3(o, g, v[0]);
          if (two) store_px3(o, g + 1, v[NP - 1]);
        }
      }
    }
  }
}

}  // namespace

// mean_istd: 8 floats {mean[0..3], 1/std[0..3]} (uint8 scale) on the device
MLC_EXPORT int mlc_augment(const uint8_t* src, const int* par, const float* mean_istd, void* out, int B, int H,
                           int W, int C, int oh, int ow, int layout, hipStream_t st) {
  if (C < 1 || C > 4 || B <= 0 || oh <= 0 || ow <= 0 || layout < 0 || layout > 2) return -1;
  if (layout == 0 && (C != 3 || (oh & 1) || (ow & 1))) return -1;
  if (layout == 1 && C > 8) return -1;
  const int Hb = (oh + 6) / 2, Wb = (ow + 6) / 2;
  const long total = layout == 0 ? (long)B * Hb * Wb : (long)B * oh * ow;
  long blocks = (total + NT - 1) / NT;
  if (blocks > 16384) blocks = 16384;
  if (layout == 0) {
    hipLaunchKernelGGL(augment_s2d_kernel<3>, dim3((int)blocks), dim3(NT), 0, st, src, par, mean_istd,
                       reinterpret_cast<bf16*>(out), B, H, W, oh, ow, Hb, Wb);
    return hipGetLastError();
  }
#define AUG_PIX(CC) hipLaunchKernelGGL(augment_pix_kernel<CC>, dim3((int)blocks), dim3(NT), 0, st, src, par, \
                                       mean_istd, out, B, H, W, oh, ow, layout)
  if (C == 1) AUG_PIX(1);
  else if (C == 2) AUG_PIX(2);
  else if (C == 3) AUG_PIX(3);
  else AUG_PIX(4);
#undef AUG_PIX
  return hipGetLastError();
}

// Image + mask records under one transform: img [B][H][W][C], mask [B][H][W][K] uint8,
// par int32 [B][8] = {y0, x0, h, w, hflip, vflip, transpose, 0}.  out_img: `layout` as
// in mlc_augment; out_mask: mask_kind 0 (planes) fp32 0/1 [B][oh][ow][K] in pixel order,
// mask_kind 1 (index, K = 1) int64 [B][oh][ow].  One launch; a thread derives the source
// coordinate of its output pixel once and samples both operands there.  Returns -1 for
// arguments out of range; par lives on the device, so its boxes are clamped into the
// image by the kernel instead.
MLC_EXPORT int mlc_augment_seg(const uint8_t* img, const uint8_t* mask, const int* par, const float* mean_istd,
                               void* out_img, void* out_mask, int B, int H, int W, int C, int K, int oh, int ow,
                               int layout, int mask_kind, hipStream_t st) {
  if (C < 1 || C > 4 || K < 1 || K > 4 || B <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0 || layout < 0 ||
      layout > 2 || mask_kind < 0 || mask_kind > 1)
    return -1;
  if (mask_kind == 1 && K != 1) return -1;
  if (layout == 0 && (C != 3 || (oh & 1) || (ow & 1))) return -1;
  if (!img || !mask || !par || !mean_istd || !out_img || !out_mask) return -1;
  const int Hb = (oh + 6) / 2, Wb = (ow + 6) / 2;
  const long total = layout == 0 ? (long)B * Hb * Wb : (long)B * oh * ow;
  long blocks = (total + NT - 1) / NT;
  if (blocks > 16384) blocks = 16384;
  if (layout == 0) {
    hipLaunchKernelGGL(augment_seg_s2d_kernel, dim3((int)blocks), dim3(NT), 0, st, img, mask, par, mean_istd,
                       reinterpret_cast<bf16*>(out_img), out_mask, B, H, W, K, mask_kind, oh, ow, Hb, Wb);
    return hipGetLastError();
  }
#define AUG_SEG(CC) hipLaunchKernelGGL(augment_seg_pix_kernel<CC>, dim3((int)blocks), dim3(NT), 0, st, img, mask, \
                                       par, mean_istd, out_img, out_mask, B, H, W, K, mask_kind, oh, ow, layout)
  if (C == 1) AUG_SEG(1);
  else if (C == 2) AUG_SEG(2);
  else if (C == 3) AUG_SEG(3);
  else AUG_SEG(4);
#undef AUG_SEG
  return hipGetLastError();
}

// Video clips: src uint8 [B][T][H][W][C] (the frames the host gathered), par int32 [B][8] =
// {y0, x0, h, w, flip, t0, frame stride, 0} on the device, one transform per clip.
// layout 0: fp32 [B][C][T][oh][ow] (NCTHW); layout 1: bf16 [B][T][oh][ow][C] with exactly
// C channels (the channels_last_3d storage of a [B, C, T, oh, ow] tensor).  One launch; per
// frame the arithmetic is mlc_augment's, so the values are the same bits.  Returns -1 for
// arguments out of range; the boxes are clamped into the image by the kernel.
MLC_EXPORT int mlc_augment_clip(const uint8_t* src, const int* par, const float* mean_istd, void* out, int B, int T,
                                int H, int W, int C, int oh, int ow, int layout, hipStream_t st) {
  if (C < 1 || C > 4 || B <= 0 || T <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0 || layout < 0 || layout > 1)
    return -1;
  if (!src || !par || !mean_istd || !out) return -1;
  const long px = (long)oh * ow;
  const long total = (long)B * (layout == 1 && C == 3 ? (px + 1) / 2 : px);
  long blocks = (total + NT - 1) / NT;
  if (blocks > 16384) blocks = 16384;
#define AUG_CLIP(CC, LL) hipLaunchKernelGGL((augment_clip_kernel<CC, LL>), dim3((int)blocks), dim3(NT), 0, st, src, \
                                            par, mean_istd, out, B, T, H, W, oh, ow)
#define AUG_CLIP_C(LL) \
  do {                 \
    if (C == 1) AUG_CLIP(1, LL); \
    else if (C == 2) AUG_CLIP(2, LL); \
    else if (C == 3) AUG_CLIP(3, LL); \
    else AUG_CLIP(4, LL); \
  } while (0)
  if (layout == 0) AUG_CLIP_C(0);
  else AUG_CLIP_C(1);
#undef AUG_CLIP_C
#undef AUG_CLIP
  return hipGetLastError();
}
