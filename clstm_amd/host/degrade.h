// degrade.h -- the SPECIFICATION of the line degrader (clstm_degrader_*, clstm_amd/csrc/degrade.h): a raw line image in, a degraded
// image of the same size out -- a small elastic distortion, an affine jitter, a little blur.  The device kernels are accepted when
// their output equals degrade_line's AS BYTES, so every expression below is a fixed sequence of IEEE basic operations: one operation
// per rounding, no contraction (-ffp-contract=off in the Makefile), the order written out.  No transcendental is evaluated here
// except inside gauss1d's mask (a function of sigma alone); the matrix m arrives as floats (clstm_degrade_draw makes it).
//
// Images are in the host Image layout: pixel (x = i, y = j) at i*h + j, ink = 1, background = 0.
//
//   1. noise      skipped when maxdelta == 0.  Two fields f = 0 (x displacement), 1 (y displacement) of w*h values
//                 u = (float)(dg_mix(seed, f, p) >> 8) * 0x1p-24f, p = i*h + j: 24 random bits, exact in float, in [0, 1).
//   2. smoothing  gauss2d(field, sigma, sigma) of normalizer.h, unchanged.
//   3. bounding   lo / hi = min / max of the smoothed field (exact, independent of order);
//                 d = hi > lo ? (((v - lo) / (hi - lo)) * 2.0f - 1.0f) * maxdelta : 0.0f     -- within [-maxdelta, maxdelta]
//   4. warp       cx = (w - 1) * 0.5f, cy = (h - 1) * 0.5f;
//                 x = ((m[0]*(i - cx) + m[1]*(j - cy)) + cx) + tx + d0,  y = ((m[2]*(i - cx) + m[3]*(j - cy)) + cy) + ty + d1
//                 out(i, j) = bilin's double expression rounded to float once, where a tap outside the image reads 0.0f
//                 (background) instead of the clamped edge pixel; a coordinate that is not within [-2^30, 2^30] (NaN included)
//                 makes the output 0.0f.
//   5. blur       skipped when blur == 0: gauss2d(out, blur, blur).
//
// Identity (m = {1, 0, 0, 1}, tx = ty = 0, maxdelta = 0, blur = 0) gives the input back byte for byte (for pixels that are not -0.0f)
// for w, h <= 2^23: i - cx is a multiple of 0.5 below 2^22 in magnitude, hence exact; 1*(i - cx) is itself; 0*(j - cy) is a zero and
// adding it changes nothing; (i - cx) + cx is the integer i < 2^23, exact; + 0 + 0 likewise.  So x is exactly i, floor(x) = i, the
// fractions are 0, and the double expression is 1.0*(1.0*s00 + 0.0*s01) + 0.0*(...) = s00.
#pragma once
#include "normalizer.h"

namespace clstmhost {

struct DegradeLine { float m[4]; float tx, ty; float sigma, maxdelta; float blur; unsigned seed; };

// The hash: the 32-bit finaliser "lowbias32" (C. Wellons, "Prospecting for hash functions", 2018; public domain), integer
// operations only.  The stream of a seed is the finaliser of a counter offset by the finalised seed; the counter of field f at
// pixel p is 2p + f (p < 2^30).  The value depends on nothing but (seed, f, p).
inline unsigned dg_lowbias32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU;
  x ^= x >> 15; x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
inline unsigned dg_seed_key(unsigned seed) { return dg_lowbias32(seed ^ 0x9e3779b9U); }
inline unsigned dg_mix(unsigned seed, unsigned f, unsigned p) { return dg_lowbias32(dg_seed_key(seed) + (2U * p + f)); }
inline float dg_uniform(unsigned seed, unsigned f, unsigned p) { return (float)(dg_mix(seed, f, p) >> 8) * 0x1p-24f; }

inline void degrade_noise(Image& field, int w, int h, unsigned seed, unsigned f) {   // step 1
  field.resize(w, h);
  for (size_t p = 0; p < field.d.size(); p++) field.d[p] = dg_uniform(seed, f, (unsigned)p);
}

// step 3: the field's values become displacements in place
inline void degrade_bound(Image& field, float maxdelta) {
  float lo = field.d[0], hi = field.d[0];
  for (float v : field.d) { lo = std::min(lo, v); hi = std::max(hi, v); }
  for (float& v : field.d) v = hi > lo ? (((v - lo) / (hi - lo)) * 2.0f - 1.0f) * maxdelta : 0.0f;
}

inline float degrade_tap(const Image& a, int i, int j) { return i >= 0 && i < a.w && j >= 0 && j < a.h ? a(i, j) : 0.0f; }

inline float degrade_bilin(const Image& a, float x, float y) {   // bilin (normalizer.h) with background outside
  if (!(x >= -0x1p30f && x <= 0x1p30f && y >= -0x1p30f && y <= 0x1p30f)) return 0.0f;
  const int i = (int)floorf(x), j = (int)floorf(y);
  const float l = x - i, m = y - j;
  const float s00 = degrade_tap(a, i, j), s01 = degrade_tap(a, i, j + 1);
  const float s10 = degrade_tap(a, i + 1, j), s11 = degrade_tap(a, i + 1, j + 1);
  return (float)((1.0 - l) * ((1.0 - m) * s00 + m * s01) + l * ((1.0 - m) * s10 + m * s11));
}

inline void degrade_line(const Image& in, const DegradeLine& p, Image& out) {
  const int w = in.w, h = in.h;
  Image d0, d1;
  const bool distort = p.maxdelta != 0.0f;
  if (distort) {
    degrade_noise(d0, w, h, p.seed, 0);
    degrade_noise(d1, w, h, p.seed, 1);
    gauss2d(d0, p.sigma, p.sigma);
    gauss2d(d1, p.sigma, p.sigma);
    degrade_bound(d0, p.maxdelta);
    degrade_bound(d1, p.maxdelta);
  }
  out.resize(w, h);
  const float cx = (w - 1) * 0.5f, cy = (h - 1) * 0.5f;
  for (int i = 0; i < w; i++)
    for (int j = 0; j < h; j++) {
      const float dx = distort ? d0(i, j) : 0.0f, dy = distort ? d1(i, j) : 0.0f;
      const float x = ((p.m[0] * (i - cx) + p.m[1] * (j - cy)) + cx) + p.tx + dx;
      const float y = ((p.m[2] * (i - cx) + p.m[3] * (j - cy)) + cy) + p.ty + dy;
      out(i, j) = degrade_bilin(in, x, y);
    }
  if (p.blur != 0.0f) gauss2d(out, p.blur, p.blur);
}

}  // namespace clstmhost
