// degrade.h -- the line degrader (clstm_amd/host/degrade.h) on the device: a minibatch of raw line images in, the same number of
// images of the same sizes out -- a small elastic distortion, an affine jitter, a little blur -- BIT FOR BIT what degrade_line gives.
// The host file is the specification; the contract is normalize.h's:
//
//   * No contraction, from the pragma below to the one at the end of this file.
//   * The device evaluates no transcendental: the Gaussian masks come from the normaliser's mask() rule on the host (one per distinct
//     sigma, cached by its bits), the matrix m arrives as floats.
//   * Parallelism is over OUTPUTS only; every output of a filter pass is one double chain over its taps in ascending order.
//   * Host-built NzItem lists, one workgroup per item; everything on the library's one stream.
//
// Stages (DgStage numbers the items):
//   0  k_dg_noise_cols   the column pass of gauss2d over the two noise fields with its inputs COMPUTED, not loaded: the workgroup hashes
//                        the values its 256 outputs reach straight into LDS; the unsmoothed fields never exist in memory
//   1  k_nz_filter_rows  (normalize.h, as it is) the row pass, over the degrader's own NzLine array: one entry per (line, field) with
//                        mask[0] = mask[1] = the line's sigma
//   2  k_dg_minmax       partial minimum and maximum of 4096 values of a smoothed field (wave reductions; min and max are exact and
//                        independent of order, so any tree gives the host's value)
//   3  k_dg_bounds       one workgroup per field reduces its partials to lo, hi -- in device memory; the host never sees them
//   4  k_dg_warp         256 consecutive outputs: displacement from the field, lo, hi; affine map; four taps, background outside
//   5  k_nz_filter_run   (normalize.h, as it is, which = 0) and
//   6  k_nz_filter_rows  the blur, over a second NzLine array: mask[0] = mask[1] = the line's blur
// A line with maxdelta == 0 has no items in stages 0-3 and no field storage; one with blur == 0 has none in stages 5-6.
#pragma once
#include "normalize.h"

#pragma clang fp contract(off)

constexpr int DG_MM_CHUNK = 4096;   // values per partial of the min / max stage

struct DgField { unsigned key, f; };   // dg_seed_key(seed) of the line (host/degrade.h), field number 0 / 1
struct DgWarp {
  long long fld;        // first float of the line's field 0 in the smoothed-field buffer (field 1 follows: + w*h)
  int bound;            // index of the line's field 0 in the bounds array (lo at 2*bound, hi at 2*bound + 1; field 1 at bound + 1); -1: no distortion
  float m[4], tx, ty, maxdelta;
};

// lowbias32 (host/degrade.h: dg_lowbias32), integer operations only
DEVFN unsigned dg_lowbias32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
DEVFN float dg_uniform(unsigned key, unsigned f, unsigned p) { return (float)(dg_lowbias32(key + (2U * p + f)) >> 8) * 0x1p-24f; }

// ---- stage 0: k_nz_filter_run's column pass (which = 0) over a noise field: same staging window, same tap order, same accumulation;
// s_in[k] is the hash of pixel lo + k instead of a load
__global__ void __launch_bounds__(NZ_THREADS) k_dg_noise_cols(const NzItem* items, const NzLine* lines, const DgField* fields, float* out,
                                                                const float* masks) {
  __shared__ float s_mask[NZ_MAXTAPS];
  __shared__ float s_in[NZ_THREADS + 2 * NZ_MAXRANGE];
  const NzItem it = items[blockIdx.x];
  const NzLine* L = lines + it.line;
  const DgField F = fields[it.line];
  const int n = L->h;
  const long long base = L->pix;
  const int r = L->range[0], m = 2 * r + 1;
  const float* msk = masks + L->mask[0];
  const int f0 = it.first, f1 = it.first + it.count - 1;
  const int lo = (f0 / n) * n + nz_max(f0 % n - r, 0), hi = (f1 / n) * n + nz_min(f1 % n + r, n - 1);
  for (int k = threadIdx.x; k < m; k += NZ_THREADS) s_mask[k] = msk[k];
  for (int k = threadIdx.x; k <= hi - lo; k += NZ_THREADS) s_in[k] = dg_uniform(F.key, F.f, (unsigned)(lo + k));
  __syncthreads();
  if ((int)threadIdx.x >= it.count) return;
  const int f = f0 + (int)threadIdx.x, c = f / n, j = f - c * n;
  const int k_lo = nz_min(nz_max(r - j, 0), m), k_hi = nz_min(n - j + r, m);
  const float* p = s_in + (c * n - lo);
  const float first = k_lo > 0 ? p[0] : 0.0f, last = k_hi < m ? p[n - 1] : 0.0f;
  double acc = 0.0;
  int k = 0;
  for (; k < k_lo; k++) acc += (double)(first * s_mask[k]);
  for (; k < k_hi; k++) acc += (double)(p[j + k - r] * s_mask[k]);
  for (; k < m; k++) acc += (double)(last * s_mask[k]);
  out[base + f] = (float)acc;
}

// minimum and maximum over the workgroup; valid in thread 0.  The values are finite (sums of products of values in [0, 1) and mask
// entries), so fminf / fmaxf never meet a NaN, and the minimum is -max(-x) exactly
DEVFN void dg_block_minmax(float& lo, float& hi, float* s_red) {
  hi = wave_max(hi);
  lo = -wave_max(-lo);
  const int wv = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) { s_red[2 * wv] = lo; s_red[2 * wv + 1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < NZ_THREADS / 64; k++) { lo = fminf(lo, s_red[2 * k]); hi = fmaxf(hi, s_red[2 * k + 1]); }
}

// ---- stage 2: item {field, 2, first, count <= DG_MM_CHUNK}: partial[2 blockIdx] = min, [2 blockIdx + 1] = max of field values first ...
__global__ void __launch_bounds__(NZ_THREADS) k_dg_minmax(const NzItem* items, const NzLine* lines, const float* field, float* partial) {
  __shared__ float s_red[2 * NZ_THREADS / 64];
  const NzItem it = items[blockIdx.x];
  const float* v = field + lines[it.line].pix + it.first;
  float lo = v[0], hi = lo;   // (count >= 1: every thread starts from a value of the chunk)
  for (int k = threadIdx.x; k < it.count; k += NZ_THREADS) { const float x = v[k]; lo = fminf(lo, x); hi = fmaxf(hi, x); }
  dg_block_minmax(lo, hi, s_red);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo; partial[2 * blockIdx.x + 1] = hi; }
}

// ---- stage 3: item {field, 3, first partial, count >= 1}: bounds[2 field] = lo, [2 field + 1] = hi
__global__ void __launch_bounds__(NZ_THREADS) k_dg_bounds(const NzItem* items, const float* partial, float* bounds) {
  __shared__ float s_red[2 * NZ_THREADS / 64];
  const NzItem it = items[blockIdx.x];
  const float* v = partial + 2 * (long long)it.first;
  float lo = v[0], hi = v[1];
  for (int k = threadIdx.x; k < it.count; k += NZ_THREADS) { lo = fminf(lo, v[2 * k]); hi = fmaxf(hi, v[2 * k + 1]); }
  dg_block_minmax(lo, hi, s_red);
  if (threadIdx.x == 0) { bounds[2 * it.line] = lo; bounds[2 * it.line + 1] = hi; }
}

// ---- stage 4: steps 3 and 4 of degrade_line.  `lines` is the array of the IMAGES (one entry per line of the call)
DEVFN float dg_tap(const float* a, int w, int h, int i, int j) { return i >= 0 && i < w && j >= 0 && j < h ? a[(long long)i * h + j] : 0.0f; }
DEVFN float dg_displace(float v, float lo, float hi, float maxdelta) { return hi > lo ? (((v - lo) / (hi - lo)) * 2.0f - 1.0f) * maxdelta : 0.0f; }
__global__ void __launch_bounds__(NZ_THREADS) k_dg_warp(const NzItem* items, const NzLine* lines, const DgWarp* warps, const float* pix,
                                                          const float* field, const float* bounds, float* out) {
  const NzItem it = items[blockIdx.x];
  if ((int)threadIdx.x >= it.count) return;
  const NzLine* L = lines + it.line;
  const DgWarp* W = warps + it.line;
  const int w = L->w, h = L->h;
  const int f = it.first + (int)threadIdx.x, i = f / h, j = f - i * h;
  float dx = 0.0f, dy = 0.0f;
  if (W->bound >= 0) {   // (maxdelta == 0: the fields were not produced and are not touched)
    const float* b = bounds + 2 * W->bound;
    const float* fl = field + W->fld;
    dx = dg_displace(fl[f], b[0], b[1], W->maxdelta);
    dy = dg_displace(fl[(long long)w * h + f], b[2], b[3], W->maxdelta);
  }
  const float cx = (w - 1) * 0.5f, cy = (h - 1) * 0.5f;
  const float x = ((W->m[0] * (i - cx) + W->m[1] * (j - cy)) + cx) + W->tx + dx;
  const float y = ((W->m[2] * (i - cx) + W->m[3] * (j - cy)) + cy) + W->ty + dy;
  float res = 0.0f;
  if (x >= -0x1p30f && x <= 0x1p30f && y >= -0x1p30f && y <= 0x1p30f) {
    const float* a = pix + L->pix;
    const int si = (int)floorf(x), sj = (int)floorf(y);
    const float l = x - si, m = y - sj;
    const float s00 = dg_tap(a, w, h, si, sj), s01 = dg_tap(a, w, h, si, sj + 1);
    const float s10 = dg_tap(a, w, h, si + 1, sj), s11 = dg_tap(a, w, h, si + 1, sj + 1);
    res = (float)((1.0 - l) * ((1.0 - m) * s00 + m * s01) + l * ((1.0 - m) * s10 + m * s11));
  }
  out[L->pix + f] = res;
}

// back to the defaults of the two compilation passes (device: fast, host: on) for the rest of the translation unit
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang fp contract(fast)
#else
#pragma clang fp contract(on)
#endif
