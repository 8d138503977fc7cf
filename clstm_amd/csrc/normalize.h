// normalize.h -- CenterNormalizer (clstm_amd/host/normalizer.h; reference extras.cc:53-131, 205-285) on the device: raw line images
// in, input frames out, BIT FOR BIT what the host code gives.  The host file is the specification: every kernel below evaluates
// its expressions with the same types, in the same order, one IEEE operation per rounding.
//
//   * No contraction.  hipcc fuses a*b + c in device code by default; from the file-scope `#pragma clang fp contract(off)` below to
//     the pragma at the end of this file, which puts the compiler's default back for whatever the translation unit includes
//     next, it does not.  The emulator build (g++, no FMA target) evaluates the same expressions.
//   * The device never evaluates exp: the Gaussian masks are computed on the host inside the library (normalize_run.inc) with
//     gauss1d's own expressions, one mask per distinct sigma, cached and uploaded.
//   * Parallelism is over OUTPUTS only.  Each output pixel of a filter pass keeps one double accumulator and walks its taps in
//     ascending order with the addend (double)(float product); no tap is skipped, reordered or tree-reduced.  The smear is one
//     sequential double chain per row, the sums s1 / sy of `measure` are ONE float chain per line (i outer, j inner) walked by one
//     lane while the other waves of the workgroup stage its operands in LDS: about w.h dependent float adds, the latency floor of
//     the call, accepted because any other order changes mad and r = (float)int(range*mad + 1) truncates.
//   * Work distribution is a host-built item list, one workgroup per item: NzItem{line, stage, first, count}.  Rows and columns
//     are staged in LDS in TILES WITH HALOS (the halo is the mask's reach, clamped at the ends as pad[k] = in[clamp(k - range)]),
//     never as whole rows: no width is refused because a row does not fit.  What is limited is the mask's reach:
//     1 + int(3 sigma) <= NZ_MAXRANGE (800) for the three sigmas h/2, h.smooth2d, h.smooth1d -- any h <= 256 at the default
//     parameters (reach 769) -- so that a row tile with both halos and its mask stay below 64 KB of LDS.
//   * center[int(x)] in `normalize`: the host indexes without a bound; the device clamps the index to w - 1 and is identical
//     wherever the host's index is in range.
//   * Everything is enqueued on the library's ONE stream (clstm_set_stream), never on a stream of its own: the fused forward and
//     backward launches assume that their workgroups are co-resident, and a concurrent kernel from a second stream
//     could starve a role that polls.
//
// Buffers (floats): pix / tmp / smooth are the lines' images back to back in the host Image layout (pixel (x = i, y = j) of a
// line at pix + i*h + j); amax / center hold one value per column, lines back to back (NzLine::col).
#pragma once
#include "devintrin.h"

#pragma clang fp contract(off)

constexpr int NZ_MAXRANGE = 800;                 // largest mask reach 1 + int(3 sigma)
constexpr int NZ_MAXTAPS = 2 * NZ_MAXRANGE + 1;
constexpr int NZ_THREADS = 256;
constexpr int NZ_ROW_TI = 64, NZ_ROW_TJ = 8;     // row pass: a tile is 64 output columns x 8 rows
constexpr int NZ_MAD_CHUNK = 2048;               // pixels staged per hand-over to the summing lane

DEVFN int nz_min(int a, int b) { return a < b ? a : b; }
DEVFN int nz_max(int a, int b) { return a > b ? a : b; }

struct NzLine {
  int w, h;
  long long pix;        // first pixel of the line in pix / tmp / smooth
  long long col;        // first column of the line in amax / center
  int mask[3];          // offsets into the mask pool: [0] sigma h/2 (column pass), [1] h.smooth2d (row pass), [2] h.smooth1d (centre line)
  int range[3];         // their reach: the mask has 2 range + 1 taps
};
// one workgroup's work.  `first` / `count`: stage 0 (column pass) outputs in memory order i*h + j; stage 1 (row pass) `first` =
// (j / 8)*w + i of the tile's first output, `count` output columns (<= 64) of the 8 rows j & ~7 ...; stage 2 (smear) rows;
// stage 3 (argmax) columns; stage 4 (centre line) columns; stage 5 (mad) the whole line; stage 6 (warp) outputs t*target_height + j
struct NzItem { int line, stage, first, count; };
struct NzWarp {
  float scale;          // (float)((2.0 * r) / target_height), computed on the host from the line's r
  int T;                // target_width
  long long out;        // first float of the line's frames
};

// ---- stages 0 and 4: Gaussian along sequences that are contiguous in memory (a column of the image: n = h; the centre line:
// n = w).  256 consecutive outputs per workgroup; staged: the inputs they reach, which never leave their own sequence because the
// index is clamped -- at most count + 2 range floats.
__global__ void __launch_bounds__(NZ_THREADS) k_nz_filter_run(const NzItem* items, const NzLine* lines, const float* in, float* out,
                                                                const float* masks, int which) {
  __shared__ float s_mask[NZ_MAXTAPS];
  __shared__ float s_in[NZ_THREADS + 2 * NZ_MAXRANGE];
  const NzItem it = items[blockIdx.x];
  const NzLine* L = lines + it.line;     // (read in place: a private copy indexed by `which` would live in scratch)
  const int n = which == 0 ? L->h : L->w;
  const long long base = which == 0 ? L->pix : L->col;
  const int r = L->range[which], m = 2 * r + 1;
  const float* msk = masks + L->mask[which];
  const int f0 = it.first, f1 = it.first + it.count - 1;
  const int lo = (f0 / n) * n + nz_max(f0 % n - r, 0), hi = (f1 / n) * n + nz_min(f1 % n + r, n - 1);
  for (int k = threadIdx.x; k < m; k += NZ_THREADS) s_mask[k] = msk[k];
  for (int k = threadIdx.x; k <= hi - lo; k += NZ_THREADS) s_in[k] = in[base + lo + k];
  __syncthreads();
  if ((int)threadIdx.x >= it.count) return;
  const int f = f0 + (int)threadIdx.x, c = f / n, j = f - c * n;
  // taps k < k_lo read in[0] of the sequence, taps k >= k_hi read in[n - 1], the ones between read in[j + k - r]
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

// ---- stage 1: Gaussian along rows (fixed y = j; consecutive positions are h floats apart).  A tile is 64 output columns x 8 rows:
// LDS holds tile[p][jj] = in(clamp(i0 + p - range), j0 + jj) for p < count + 2 range -- the 8 rows interleaved, so that the 64 lanes
// of a wave (8 rows x 8 columns) read 64 consecutive floats for every tap.  Thread (jj, oo) owns outputs i0 + oo and i0 + oo + 32.
__global__ void __launch_bounds__(NZ_THREADS) k_nz_filter_rows(const NzItem* items, const NzLine* lines, const float* in, float* out,
                                                                 const float* masks) {
  float* s_mask = dyn_smem<float>();
  const NzItem it = items[blockIdx.x];
  const NzLine L = lines[it.line];
  const int w = L.w, h = L.h;
  const int r = L.range[1], m = 2 * r + 1;
  float* tile = s_mask + ((m + 3) & ~3);
  const float* msk = masks + L.mask[1];
  const int j0 = (it.first / w) * NZ_ROW_TJ, i0 = it.first % w, count = it.count;
  const int jj = threadIdx.x % NZ_ROW_TJ, oo = threadIdx.x / NZ_ROW_TJ;
  const float* src = in + L.pix;
  for (int k = threadIdx.x; k < m; k += NZ_THREADS) s_mask[k] = msk[k];
  for (int p = oo; p < count + 2 * r; p += NZ_THREADS / NZ_ROW_TJ) {
    const int col = nz_min(nz_max(i0 + p - r, 0), w - 1);
    tile[p * NZ_ROW_TJ + jj] = j0 + jj < h ? src[(long long)col * h + j0 + jj] : 0.0f;
  }
  __syncthreads();
  double acc0 = 0.0, acc1 = 0.0;
  const float* t0 = tile + oo * NZ_ROW_TJ + jj;
  const float* t1 = t0 + 32 * NZ_ROW_TJ;
  if (oo + 32 < count) {
    for (int k = 0; k < m; k++) {
      const float mk = s_mask[k];
      acc0 += (double)(t0[k * NZ_ROW_TJ] * mk);
      acc1 += (double)(t1[k * NZ_ROW_TJ] * mk);
    }
  } else if (oo < count) {
    for (int k = 0; k < m; k++) acc0 += (double)(t0[k * NZ_ROW_TJ] * s_mask[k]);
  }
  if (j0 + jj >= h) return;
  float* dst = out + L.pix;
  if (oo < count) dst[(long long)(i0 + oo) * h + j0 + jj] = (float)acc0;
  if (oo + 32 < count) dst[(long long)(i0 + oo + 32) * h + j0 + jj] = (float)acc1;
}
static inline size_t nz_rows_smem(int range) { return ((size_t)((2 * range + 1 + 3) & ~3) + (size_t)(NZ_ROW_TI + 2 * range) * NZ_ROW_TJ) * sizeof(float); }

// ---- stage 2: add_smear (measure :90-96).  One thread per row j: a sequential double chain over the columns; v*0.9 is rounded,
// then + line (contraction is off), the addend to smooth is (float)(fmin(1.0, v) * 1e-3).  Consecutive lanes read consecutive j.
__global__ void __launch_bounds__(NZ_THREADS) k_nz_smear(const NzItem* items, const NzLine* lines, const float* pix, float* smooth) {
  const NzItem it = items[blockIdx.x];
  if ((int)threadIdx.x >= it.count) return;
  const NzLine L = lines[it.line];
  const int j = it.first + (int)threadIdx.x;
  const float* line = pix + L.pix + j;
  float* sm = smooth + L.pix + j;
  double v = 0.0;
  for (int i = 0; i < L.w; i++) {
    const long long o = (long long)i * L.h;
    v = v * 0.9 + (double)line[o];
    sm[o] = sm[o] + (float)(fmin(1.0, v) * 1e-3);
  }
}

// ---- stage 3: argmax1 (measure :97-106).  One thread per column; ties go to the LAST row
__global__ void __launch_bounds__(NZ_THREADS) k_nz_argmax(const NzItem* items, const NzLine* lines, const float* smooth, float* amax) {
  const NzItem it = items[blockIdx.x];
  if ((int)threadIdx.x >= it.count) return;
  const NzLine L = lines[it.line];
  const int i = it.first + (int)threadIdx.x;
  const float* s = smooth + L.pix + (long long)i * L.h;
  float mv = s[0], mj = 0.0f;
  for (int j = 1; j < L.h; j++) {
    const float val = s[j];
    if (val < mv) continue;
    mv = val;
    mj = (float)j;
  }
  amax[L.col + i] = mj;
}

// ---- stage 5: s1 and sy of measure :108-113, float sums over i outer, j inner: memory order.  One workgroup per line.  Waves 1-3
// stage the next NZ_MAD_CHUNK operands -- line(i, j) and the float product line(i, j) * |j - center[i]| -- while lane 0 of wave 0
// adds the chunk before it to the two chains, in order.  sums[2 line] = s1, sums[2 line + 1] = sy; mad and r are the host's.
DEVFN void nz_mad_stage(float* sv, float* sp, const float* pix, const float* center, int h, int f0, int f1, int t, int nt) {
  for (int f = f0 + t; f < f1; f += nt) {
    const int i = f / h, j = f - i * h;
    const float v = pix[f];
    sv[f - f0] = v;
    sp[f - f0] = v * fabsf((float)j - center[i]);
  }
}
__global__ void __launch_bounds__(NZ_THREADS) k_nz_mad(const NzItem* items, const NzLine* lines, const float* pix, const float* center,
                                                         float* sums) {
  __shared__ float s_v[2][NZ_MAD_CHUNK];
  __shared__ float s_p[2][NZ_MAD_CHUNK];
  const NzItem it = items[blockIdx.x];
  const NzLine L = lines[it.line];
  const int total = L.w * L.h, nch = (total + NZ_MAD_CHUNK - 1) / NZ_MAD_CHUNK;
  const float* px = pix + L.pix;
  const float* ce = center + L.col;
  const int t = threadIdx.x;
  nz_mad_stage(s_v[0], s_p[0], px, ce, L.h, 0, nz_min(NZ_MAD_CHUNK, total), t, NZ_THREADS);
  __syncthreads();
  float s1 = 0.0f, sy = 0.0f;
  for (int c = 0; c < nch; c++) {
    const int b = c & 1;
    if (t >= 64 && c + 1 < nch)
      nz_mad_stage(s_v[b ^ 1], s_p[b ^ 1], px, ce, L.h, (c + 1) * NZ_MAD_CHUNK, nz_min((c + 2) * NZ_MAD_CHUNK, total), t - 64, NZ_THREADS - 64);
    if (t == 0) {
      const int len = nz_min(NZ_MAD_CHUNK, total - c * NZ_MAD_CHUNK);
      for (int q = 0; q < len; q++) {
        s1 += s_v[b][q];
        sy += s_p[b][q];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    sums[2 * it.line] = s1;
    sums[2 * it.line + 1] = sy;
  }
}

// ---- stage 6: normalize + bilin (:72-79, :117-129).  256 consecutive outputs t*target_height + j per workgroup
DEVFN int nz_clipi(int x, int n) { return x < 0 ? 0 : x >= n ? n - 1 : x; }
__global__ void __launch_bounds__(NZ_THREADS) k_nz_warp(const NzItem* items, const NzLine* lines, const NzWarp* warps, const float* pix,
                                                          const float* center, float* frames, int target_height) {
  const NzItem it = items[blockIdx.x];
  if ((int)threadIdx.x >= it.count) return;
  const NzLine L = lines[it.line];
  const NzWarp W = warps[it.line];
  const int w = L.w, h = L.h;
  const int f = it.first + (int)threadIdx.x, ti = f / target_height, tj = f - ti * target_height;
  const float* a = pix + L.pix;
  const float x = W.scale * ti;
  const float y = W.scale * (tj - target_height / 2) + center[L.col + nz_min((int)x, w - 1)];
  const int i = (int)floorf(x), j = (int)floorf(y);
  const float l = x - i, m = y - j;
  const float s00 = a[(long long)nz_clipi(i, w) * h + nz_clipi(j, h)], s01 = a[(long long)nz_clipi(i, w) * h + nz_clipi(j + 1, h)];
  const float s10 = a[(long long)nz_clipi(i + 1, w) * h + nz_clipi(j, h)], s11 = a[(long long)nz_clipi(i + 1, w) * h + nz_clipi(j + 1, h)];
  frames[W.out + f] = (float)((1.0 - l) * ((1.0 - m) * s00 + m * s01) + l * ((1.0 - m) * s10 + m * s11));
}

// back to the defaults of the two compilation passes (device: fast, host: on) for the rest of the translation unit
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang fp contract(fast)
#else
#pragma clang fp contract(on)
#endif
