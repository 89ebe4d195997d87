// Text batches: one launch turns the slot the text record loader staged (csrc/runtime/records.cpp,
// mlr_text_*) into every device tensor the BERT step reads (mlc_text_unpack).
//
// slot (int32): {nseq, total}, {length, type0_length, label}[nmax], tokens[T]; the sequences'
// tokens lie back to back.  Packed mode (mode 0) writes ids / tt / pos_ids int64 [T] (rows past
// the total are 0), cu int32 [nmax + 1] (empty slots hold the total), y int64 [nmax] (0 for
// empty slots) and slot_w f32 [nmax] (1 / nreal for a slot of length > 0, else 0; nreal = the
// slots of length > 0).  Padded mode (mode 1) writes ids / tt / attention mask int64
// [nmax][max_len], right-padded with 0, and y; cu and slot_w are not touched.
//
// The kernel is total: whatever the slot holds it reads only slot[0 .. 2 + 3*nmax + T) and
// writes only the outputs, because everything is clamped first and every clamp adds one to the
// int32 counter *err:
//   nseq -> [0, nmax]; length i -> [0, max_len], then cut to what is left of T after the
//   sequences before it (cu[i] = min(sum of the clamped lengths before i, T), so the cut is a
//   plain prefix sum); type0_length -> [0, length after clamping]; label -> [0, num_labels);
//   token id -> [0, vocab); slot[1] -> the total of the clamped lengths.
// Row r of the packed outputs is token r of the slot, so a clamped length shifts nothing out
// of range.  text_unpack_reference (mlcomp_amd/train/records.py) is the same arithmetic.
//
// Every block scans the <= 1024 clamped lengths into LDS (4 per thread, a shuffle scan inside
// each wave of 64, the 4 wave totals through LDS); block 0 writes the per-slot outputs; a
// packed row finds its sequence by binary search in the LDS prefix sums, a padded element
// knows it from its index.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int NMAX = 1024;        // 4 entries per thread
constexpr int TMAX = 1 << 20;     // NMAX * TMAX stays inside an int

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// s_cu[0 .. nseq] = saturated prefix sums of the clamped lengths; returns nseq (clamped).
// err_slots (block-uniform after the call) counts the nseq / length / total clamps.
__device__ int scan_lengths(const int* __restrict__ slot, int T, int nmax, int max_len, int* s_cu, int* s_wave,
                            int* err_slots, int* nreal) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseq_raw = slot[0];
  const int nseq = clampi(nseq_raw, 0, nmax);
  int a[4], sum = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid * 4 + j;
    a[j] = i < nseq ? clampi(slot[2 + 3 * i], 0, max_len) : 0;
    sum += a[j];
  }
  int inc = sum;   // inclusive scan of the per-thread sums inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int base = inc - sum;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  if (tid == 0) s_cu[0] = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    base += a[j];
    const int i = tid * 4 + j;
    if (i < nseq) s_cu[i + 1] = min(base, T);
  }
  __syncthreads();
  // the clamps of this thread's entries, then block sums (s_wave[4..7] / [8..11])
  int e = 0, real = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = tid * 4 + j;
    if (i < nseq) {
      const int len = s_cu[i + 1] - s_cu[i];
      e += len != slot[2 + 3 * i];
      real += len > 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    e += __shfl_xor(e, o, 64);
    real += __shfl_xor(real, o, 64);
  }
  if (lane == 0) { s_wave[4 + wave] = e; s_wave[8 + wave] = real; }
  __syncthreads();
  *err_slots = s_wave[4] + s_wave[5] + s_wave[6] + s_wave[7] + (nseq_raw != nseq) + (slot[1] != s_cu[nseq]);
  *nreal = s_wave[8] + s_wave[9] + s_wave[10] + s_wave[11];
  return nseq;
}

template <int MODE>
__global__ void __launch_bounds__(NT)
text_unpack_kernel(const int* __restrict__ slot, long* __restrict__ ids, long* __restrict__ tt, long* __restrict__ pos,
                   int* __restrict__ cu, long* __restrict__ y, float* __restrict__ slot_w, int* __restrict__ err,
                   int T, int nmax, int max_len, int vocab, int num_labels) {
  __shared__ int s_cu[NMAX + 1];
  __shared__ int s_wave[12];
  int err_slots, nreal;
  const int nseq = scan_lengths(slot, T, nmax, max_len, s_cu, s_wave, &err_slots, &nreal);
  const int total = s_cu[nseq];
  const int* __restrict__ ent = slot + 2;
  const int* __restrict__ tok = slot + 2 + 3 * nmax;
  int e = 0;
  if (blockIdx.x == 0) {   // the per-slot outputs
    if (threadIdx.x == 0) e += err_slots;
    const float w = nreal > 0 ? __fdiv_rn(1.0f, (float)nreal) : 0.f;
    for (int i = threadIdx.x; i < nmax; i += NT) {
      long lab = 0;
      int len = 0;
      if (i < nseq) {
        const int raw = ent[3 * i + 2];
        const int c = clampi(raw, 0, num_labels - 1);
        e += c != raw;
        lab = c;
        len = s_cu[i + 1] - s_cu[i];
      }
      y[i] = lab;
      if (MODE == 0) {
        cu[i + 1] = i < nseq ? s_cu[i + 1] : total;
        slot_w[i] = len > 0 ? w : 0.f;
      }
    }
    if (MODE == 0 && threadIdx.x == 0) cu[0] = 0;
    // a type0_length past its (clamped) length is counted once, here
    for (int i = threadIdx.x; i < nseq; i += NT) {
      const int raw = ent[3 * i + 1];
      e += clampi(raw, 0, s_cu[i + 1] - s_cu[i]) != raw;
    }
  }
  if (MODE == 0) {
    for (int r = blockIdx.x * NT + threadIdx.x; r < T; r += gridDim.x * NT) {
      long id = 0, ty = 0, p = 0;
      if (r < total) {
        int lo = 0, hi = nseq;   // the sequence i with s_cu[i] <= r < s_cu[i + 1]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (s_cu[mid] <= r) lo = mid; else hi = mid;
        }
        const int q = r - s_cu[lo];
        const int t0 = clampi(ent[3 * lo + 1], 0, s_cu[lo + 1] - s_cu[lo]);
        const int raw = tok[r];
        const int c = clampi(raw, 0, vocab - 1);
        e += c != raw;
        id = c; ty = q >= t0; p = q;
      }
      ids[r] = id; tt[r] = ty; pos[r] = p;
    }
  } else {
    const int n = nmax * max_len;
    for (int k = blockIdx.x * NT + threadIdx.x; k < n; k += gridDim.x * NT) {
      const int i = k / max_len, q = k - i * max_len;
      long id = 0, ty = 0, m = 0;
      if (i < nseq && q < s_cu[i + 1] - s_cu[i]) {
        const int t0 = clampi(ent[3 * i + 1], 0, s_cu[i + 1] - s_cu[i]);
        const int raw = tok[s_cu[i] + q];
        const int c = clampi(raw, 0, vocab - 1);
        e += c != raw;
        id = c; ty = q >= t0; m = 1;
      }
      ids[k] = id; tt[k] = ty; pos[k] = m;
    }
  }
  if (e) atomicAdd(err, e);
}

}  // namespace

// slot: the staged int32 slot (see above); mode 0 packed, 1 padded (pos is then the attention
// mask, cu and slot_w may be null).  -1 without launching for T <= 0, T % 8 != 0, T > 2^20, nmax
// outside [1, 1024], max_len outside [1, T], vocab <= 0, num_labels <= 0 or a null pointer.
MLC_EXPORT int mlc_text_unpack(const int* slot, int mode, long* ids, long* tt, long* pos, int* cu, long* y,
                               float* slot_w, int* err, int T, int nmax, int max_len, int vocab, int num_labels,
                               hipStream_t st) {
  if (mode < 0 || mode > 1 || T <= 0 || T % 8 != 0 || T > TMAX || nmax < 1 || nmax > NMAX || max_len < 1 ||
      max_len > T || vocab <= 0 || num_labels <= 0)
    return -1;
  if (!slot || !ids || !tt || !pos || !y || !err || (mode == 0 && (!cu || !slot_w))) return -1;
  const long work = mode == 0 ? (long)T : (long)nmax * max_len;
  long blocks = (work + NT - 1) / NT;
  if (blocks > 1024) blocks = 1024;
  if (mode == 0)
    hipLaunchKernelGGL(text_unpack_kernel<0>, dim3((int)blocks), dim3(NT), 0, st, slot, ids, tt, pos, cu, y, slot_w,
                       err, T, nmax, max_len, vocab, num_labels);
  else
    hipLaunchKernelGGL(text_unpack_kernel<1>, dim3((int)blocks), dim3(NT), 0, st, slot, ids, tt, pos, cu, y, slot_w,
                       err, T, nmax, max_len, vocab, num_labels);
  return hipGetLastError();
}
