// ctc_score.h -- per-transcript CTC score and forced alignment on device: the forward half of ctc.h's phase B on its own.
//
// For a line of T frames and a candidate of S states (one class per state) the kernel evaluates forward_algorithm (ctc.cc:24-40)
// over the match scores of ctc_align_targets (ctc.cc:66-77, Classes overload :136-146):
//   lmatch(t,s) = log(out_t[class_s]),  out_t = max(1e-5, p_t) / sum
//   score  = lr(T-1, S-1), skip = -5: initial row v(j) = skip j, w(0) = skip i, stay / advance-only transitions, log_add with
//            its cut-off at 10 (tensor.h:86-89; ctc_log_add<false>, every float rounding of the reference reproduced)
//   vscore = the same recursion with max(same, next) in place of log_add (plain float adds), and a best path by back-trace
//            from (T-1, S-1): advance iff next > same (ties stay); the walk ends at frame 0 or at a frame i0 > 0 where state 0 was
//            entered through w(0) -- frames before i0 then carry -1.
// This is the reference's UNNORMALISED score, not the textbook CTC likelihood: every state and frame carries a skip term, and
// frame 0 of state 0 counts `same` and `next` both (log_add of two equal terms = + ln 2), so a score can be slightly positive.
// A frame with a non-finite posterior makes that frame's match scores NaN: the scores of the line's candidates are then
// non-finite, the path entries stay in [-1, S).
//
// Work list: groups of (line, candidate) items, one workgroup (256 threads) per group.
//   S <= 64 (and T <= SCORE_TMAX)   one WAVE per item, lane = state, the j-1 neighbour by the DPP wave shift, no barrier per frame;
//                                   up to four items of ONE line per workgroup: the per-frame normalisers 1 / sum_c max(1e-5, p)
//                                   are computed once per workgroup into LDS.  A line whose posteriors fit the LDS tile whole
//                                   (T <= tile: the OCR shapes) stays there and is turned IN PLACE into log(out_t[c]) for every
//                                   class by all 256 threads: one table of match scores for all of the line's candidates, read
//                                   by the waves CTC_PD frames ahead, the logarithm off the serial chain.  (A longer line takes
//                                   its posteriors from memory CTC_PD frames ahead and the logarithm in the step.)
//   64 < S <= CTC_SMAX_LDS          the workgroup cooperates on one item: up to CTC_RMAX states per lane, the first neighbour of
//                                   a lane through a double-buffered LDS vector, one barrier per frame (ctc_lattice's scheme)
//   S > CTC_SMAX_LDS                rounds over the label axis, two rolling rows in the workspace (correctness path)
// No T x S float lattice exists anywhere: O(S) state per item.  MAXPLUS records one back-pointer BIT per cell
// (wave_ballot(next > same): one 64-bit word per frame and 64 states), in LDS for the one-wave form, in the workspace otherwise;
// the back-trace runs in the same launch.
#pragma once
#include "ctc.h"

namespace clstm {

constexpr int SCORE_THREADS = CTC_GROUP;
constexpr int SCORE_WAVES = SCORE_THREADS / 64;
constexpr int SCORE_TMAX = 1024;         // one-wave form: the normalisers and back-pointer words of a line this long fit the LDS carve
constexpr int SCORE_ROW_WORDS = 20480;   // LDS words of the posterior tile the normalisers are summed from (the bench line whole: 200 x 101)
constexpr int SCORE_MLP = 16;            // posteriors a thread keeps in flight while it stages the tile

// one candidate; ws_off: this item's part of the workspace, in 8-byte words (forms 1, 2: normalisers | rolling rows | words)
struct ScoreItem { long long ws_off; int off, T, soff, S, out, path_off; };
struct ScoreGroup { int first, n, form, lml; };   // form 0: one wave per item (n <= 4, one line; lml: the line's match scores resident in LDS), 1: registers, 2: rounds
struct ScoreArgs {
  const ScoreGroup* groups;
  const ScoreItem* items;
  const float* P;           // [N][nc] softmax outputs
  const int* states;        // packed state classes
  const double* tables;     // ctc_tables.h, as CtcArgs::tables
  float* score;             // [ncand]
  int* path;                // packed, or null
  unsigned long long* ws;
  int nc, ncp, tile, tmax, ncand, npath;
};
struct ScoreLds { int tables, inv, vx, bits, rowbuf, words; };
inline __host__ __device__ ScoreLds score_lds_layout(int tmax, int tile, int ncp, bool maxplus) {
  ScoreLds l;
  int o = 0;
  l.tables = o; o += CTC_TABLE_WORDS;    // doubles first: 8-byte aligned
  l.inv = o;    o += 2 * tmax;
  l.bits = o;   o += maxplus ? SCORE_WAVES * 2 * tmax : 0;
  l.vx = o;     o += 2 * (CTC_GROUP + 2);
  l.rowbuf = o; o += tile * ncp;   // posterior tile; a resident line's match scores
  l.words = o;
  return l;
}
// words of 64 back-pointer bits per frame (forms 1, 2)
inline __host__ __device__ int score_frame_words(int S) {
  return S <= CTC_SMAX_LDS ? SCORE_WAVES * ((S + CTC_GROUP - 1) / CTC_GROUP) : (S + 63) / 64;
}

// lmatch of one cell from the raw posterior and the frame's 1 / sum (x / sum as (float)((double)x * (1 / sum)), as ctc.h)
DEVFN float score_lmatch(float x, double iv, const CrTables tb) {
  const float xm = x < 1e-5f ? 1e-5f : x;   // fmax(lo, x) of the reference for finite x; a NaN stays one
  const float q = (float)((double)xm * iv);
  const float l = cr_logf(q, tb);
  return f32_finite(q) ? l : __builtin_nanf("");
}

// inv[t] = 1 / sum_c max(1e-5, p_t[c]), the sum sequential in class order in float as asum1() (tensor.h:337-342); NaN for a
// frame that holds a non-finite posterior.  The frames pass through an LDS tile [tile][ncp] (coalesced reads, one thread per
// frame sums its row); class counts beyond the tile (tile = 0) are summed straight from memory.
// logs (T <= tile only): the tile is then turned in place into the line's match scores, rowbuf[t ncp + c] = log(out_t[c]).
DEVFN void score_frame_norms(const float* P, const int T, const int nc, const int ncp, const int tile, float* rowbuf, double* inv,
                             const bool logs, const CrTables tb) {
  const int tid = threadIdx.x;
  const BufF32 pb = make_buf(P, (size_t)T * nc * 4);
  if (tile >= 1) {
    const int dq = SCORE_THREADS / nc, dr = SCORE_THREADS - dq * nc;
    for (int t0 = 0; t0 < T; t0 += tile) {
      const int nt = (T - t0) < tile ? (T - t0) : tile, n = nt * nc;
      __syncthreads();
      int tq = tid / nc, cq = tid - tq * nc;   // (frame, class) of element i, followed incrementally
      for (int i0 = tid; i0 < n; i0 += SCORE_MLP * SCORE_THREADS) {
        float x[SCORE_MLP];
#pragma unroll
        for (int u = 0; u < SCORE_MLP; u++) {
          const int i = i0 + u * SCORE_THREADS;
          x[u] = buf_load(pb, i < n ? (unsigned)(t0 * nc + i) * 4u : BUF_OOB);
        }
#pragma unroll
        for (int u = 0; u < SCORE_MLP; u++) {
          if (i0 + u * SCORE_THREADS < n) rowbuf[tq * ncp + cq] = x[u];
          tq += dq; cq += dr;
          if (cq >= nc) { cq -= nc; tq++; }
        }
      }
      __syncthreads();
      if (tid < nt) {
        const float* r = rowbuf + tid * ncp;
        float acc = 0.0f;
        bool bad = false;
        for (int c = 0; c < nc; c++) {
          const float x = r[c];
          bad = bad || !f32_finite(x);
          acc += x < 1e-5f ? 1e-5f : x;
        }
        inv[t0 + tid] = bad ? __builtin_nan("") : 1.0 / (double)acc;
      }
    }
    if (logs) {   // workgroup-uniform; one iteration above: frame t of the line is row t of the tile
      __syncthreads();
      const int n = T * nc;
      int tq = tid / nc, cq = tid - tq * nc;
      for (int i0 = tid; i0 < n; i0 += 8 * SCORE_THREADS) {
        float l[8];
        float* w[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const bool in = i0 + u * SCORE_THREADS < n;
          w[u] = rowbuf + (in ? tq * ncp + cq : 0);
          l[u] = score_lmatch(*w[u], inv[in ? tq : 0], tb);
          tq += dq; cq += dr;
          if (cq >= nc) { cq -= nc; tq++; }
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (i0 + u * SCORE_THREADS < n) *w[u] = l[u];
      }
    }
  } else {
    for (int t = tid; t < T; t += SCORE_THREADS) {
      float acc = 0.0f;
      bool bad = false;
      for (int c0 = 0; c0 < nc; c0 += CTC_MLP) {
        float x[CTC_MLP];
#pragma unroll
        for (int u = 0; u < CTC_MLP; u++) x[u] = buf_load(pb, c0 + u < nc ? (unsigned)(t * nc + c0 + u) * 4u : BUF_OOB);
#pragma unroll
        for (int u = 0; u < CTC_MLP; u++) {
          bad = bad || !f32_finite(x[u]);
          acc += c0 + u < nc ? (x[u] < 1e-5f ? 1e-5f : x[u]) : 0.0f;   // + 0.0f is exact
        }
      }
      inv[t] = bad ? __builtin_nan("") : 1.0 / (double)acc;
    }
  }
}

DEVFN unsigned long long score_word_wt(const unsigned long long* p) {   // a word another wave of the workgroup wrote
  const int* q = reinterpret_cast<const int*>(p);
  const unsigned lo = (unsigned)load_i32_wt(q), hi = (unsigned)load_i32_wt(q + 1);
  return ((unsigned long long)hi << 32) | lo;
}

// Back-trace by one wave, every lane walking the same (wave-uniform) states: lane l keeps the state of frame 64 k + l, a chunk of
// 64 frames leaves in one coalesced store.  adv(t, j): the back-pointer bit of cell (t, j).
template <class Adv>
DEVFN void score_backtrace(int* path, const int T, const int S, Adv adv) {
  const int lane = threadIdx.x & 63;
  const BufF32 pathb = make_buf(reinterpret_cast<const float*>(path), (size_t)T * 4);
  int j = S - 1, mine = -1;
  bool stopped = false;
  for (int t = T - 1; t >= 0; t--) {
    if ((t & 63) == lane) mine = stopped ? -1 : j;
    if (!stopped && t > 0 && adv(t, j)) {
      if (j == 0) stopped = true;   // state 0 entered through w(0) = skip t: the path starts here
      else j--;
    }
    if ((t & 63) == 0) buf_store_u32(pathb, t + lane < T ? (unsigned)(t + lane) * 4u : BUF_OOB, (unsigned)mine);
  }
}

// The same where the word of a frame does not depend on the state (S <= 64, words in LDS): eight words are read ahead of the
// eight dependent steps that use them.
DEVFN void score_backtrace_words(int* path, const int T, const int S, const unsigned long long* words) {
  const int lane = threadIdx.x & 63;
  const BufF32 pathb = make_buf(reinterpret_cast<const float*>(path), (size_t)T * 4);
  int j = S - 1, mine = -1;
  bool stopped = false;
  for (int t0 = (T - 1) & ~7; t0 >= 0; t0 -= 8) {
    unsigned long long w[8];
#pragma unroll
    for (int u = 0; u < 8; u++) w[u] = words[t0 + u < T ? t0 + u : T - 1];
#pragma unroll
    for (int u = 7; u >= 0; u--) {
      const int t = t0 + u;
      if (t < T) {   // wave-uniform
        if ((t & 63) == lane) mine = stopped ? -1 : j;
        if (!stopped && t > 0 && ((w[u] >> j) & 1ull)) {
          if (j == 0) stopped = true;
          else j--;
        }
      }
    }
    if ((t0 & 63) == 0) buf_store_u32(pathb, t0 + lane < T ? (unsigned)(t0 + lane) * 4u : BUF_OOB, (unsigned)mine);
  }
}

// ---- S <= 64: one wave per item -------------------------------------------------------------------------------------
// LML: the line's match scores lie in LDS (lm[t ncp + class]); otherwise posteriors from memory, the logarithm in the step
template <bool MAXPLUS, bool LML>
DEVFN void score_one_wave(const ScoreArgs& a, const ScoreItem it, const float* P, const double* inv, unsigned long long* bitsw,
                          const float* lm, const CrTables tb) {
  const int lane = threadIdx.x & 63;
  const int T = it.T, S = it.S, nc = a.nc, j = lane;
  const int cls = a.states[it.soff + (j < S ? j : 0)];
  const BufF32 pb = make_buf(P, (size_t)T * nc * 4);
  // posterior of (frame, this lane's class): lane part + wave-uniform frame part; masked lanes sit at BUF_OOB_BASE, requests past
  // the end re-read the end frame
  const unsigned lanepart = j < S ? (unsigned)cls * 4u : BUF_OOB_BASE;
  const int rowbytes = nc * 4, lastb = (T - 1) * rowbytes;
  const int ncp = a.ncp;
  const float* lp = lm + cls;                        // LML: this lane's column, at the frame of the next request
  const float* const lplast = lp + (T - 1) * ncp;
  float v = -5.0f * (float)j;   // skip * j, exact in float
  float skipi = 0.0f;           // skip * i, accumulated: exact while 5 T < 2^24
  float pq[CTC_PD];
  int pf = 0;
#pragma unroll
  for (int q = 0; q < CTC_PD; q++) {
    if constexpr (LML) { pq[q] = *lp; lp = lp + ncp > lplast ? lplast : lp + ncp; }
    else { pq[q] = buf_load_s(pb, lanepart, (unsigned)pf); pf = pf + rowbytes > lastb ? lastb : pf + rowbytes; }
  }
  int t = 0;
  auto step = [&](float& pr) {
    float lmv;
    if constexpr (LML) {
      lmv = pr;
      pr = *lp;                                      // CTC_PD frames ahead
      lp = lp + ncp > lplast ? lplast : lp + ncp;
    } else {
      lmv = score_lmatch(pr, inv[t], tb);
      pr = buf_load_s(pb, lanepart, (unsigned)pf);   // CTC_PD frames ahead
      pf = pf + rowbytes > lastb ? lastb : pf + rowbytes;
    }
    const float same = v + lmv;
    // next = w + lmatch with w = v[j-1] (lane 0: skip * i), the lane shift folded into the add
    const float next = add_wave_shr1(skipi + lmv, v, lmv);
    skipi -= 5.0f;
    if constexpr (MAXPLUS) {
      const bool ad = next > same;   // ties (and NaN) stay
      const unsigned long long word = wave_ballot(ad);
      if (lane == 0) bitsw[t] = word;
      v = ad ? next : same;
    } else {
      v = ctc_log_add<false>(same, next, tb);
    }
    t++;
  };
  while (t + CTC_PD <= T) {
#pragma unroll
    for (int q = 0; q < CTC_PD; q++) step(pq[q]);
  }
#pragma unroll
  for (int q = 0; q < CTC_PD - 1; q++)
    if (t < T) step(pq[q]);   // wave-uniform
  const BufF32 outb = make_buf(a.score, (size_t)a.ncand * 4);
  buf_store(outb, j == S - 1 ? (unsigned)it.out * 4u : BUF_OOB, v);
  if constexpr (MAXPLUS) {
    if (a.path && it.path_off >= 0) {
      wave_lds_fence();
      score_backtrace_words(a.path + it.path_off, T, S, bitsw);
    }
  }
}

// ---- 64 < S <= CTC_SMAX_LDS: lane u holds the states u R .. u R + R - 1 in registers -----------------------------------
template <bool MAXPLUS>
DEVFN void score_regs(const ScoreArgs& a, const ScoreItem it, const float* P, const double* inv, unsigned long long* bits,
                      float* vx, const CrTables tb) {
  constexpr int RM = CTC_RMAX;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6), u = tid;
  const int T = it.T, S = it.S, nc = a.nc;
  const int R = (S + CTC_GROUP - 1) / CTC_GROUP, nw = SCORE_WAVES * R;
  const BufF32 pb = make_buf(P, (size_t)T * nc * 4);
  vx[u] = (float)(-5.0 * (u * R + R - 1));
  __syncthreads();
  unsigned cp[RM];
  float v[RM], pA[RM], pB[RM];
  auto poff = [&](int t, unsigned c) -> unsigned { return (t < T && c != BUF_OOB) ? (unsigned)(t * nc) * 4u + c : BUF_OOB; };
#pragma unroll
  for (int r = 0; r < RM; r++) {
    const int j = u * R + r;
    const bool in = r < R && j < S;
    cp[r] = in ? (unsigned)a.states[it.soff + j] * 4u : BUF_OOB;
    v[r] = (float)(-5.0 * j);
    pA[r] = buf_load(pb, poff(0, cp[r]));
    pB[r] = buf_load(pb, poff(1, cp[r]));
  }
  double ivA = inv[0], ivB = inv[T > 1 ? 1 : 0];
  auto step = [&](const int i, float (&pr)[RM], double& ivr) {
    const float from_prev = vx[(i & 1) * (CTC_GROUP + 2) + (u > 0 ? u - 1 : 0)];
    const double iv = ivr;
    float lmv[RM];
#pragma unroll
    for (int r = 0; r < RM; r++) {
      lmv[r] = score_lmatch(pr[r], iv, tb);
      pr[r] = buf_load(pb, poff(i + 2, cp[r]));   // two frames ahead
    }
    ivr = inv[i + 2 < T ? i + 2 : T - 1];
    bool ad[RM];
#pragma unroll
    for (int r = RM - 1; r >= 0; r--) {
      ad[r] = false;
      if (r < R) {
        const int j = u * R + r;
        float w = (r == 0) ? from_prev : v[r - 1];
        if (j == 0) w = (float)(-5.0 * i);
        const float same = v[r] + lmv[r];
        const float next = w + lmv[r];
        if constexpr (MAXPLUS) {
          ad[r] = next > same;
          v[r] = ad[r] ? next : same;
        } else {
          v[r] = ctc_log_add<false>(same, next, tb);
        }
      }
    }
    float last = v[0];
#pragma unroll
    for (int r = 1; r < RM; r++)
      if (r == R - 1) last = v[r];
    vx[((i + 1) & 1) * (CTC_GROUP + 2) + u] = last;
    if constexpr (MAXPLUS) {
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (r < R) {   // workgroup-uniform
          const unsigned long long word = wave_ballot(ad[r]);
          if (lane == 0) bits[(size_t)i * nw + wave * R + r] = word;
        }
      }
    }
    __syncthreads();
  };
  int i = 0;
  for (; i + 1 < T; i += 2) {
    step(i, pA, ivA);
    step(i + 1, pB, ivB);
  }
  if (i < T) step(i, pA, ivA);
  const BufF32 outb = make_buf(a.score, (size_t)a.ncand * 4);
#pragma unroll
  for (int r = 0; r < RM; r++) buf_store(outb, (r < R && u * R + r == S - 1) ? (unsigned)it.out * 4u : BUF_OOB, v[r]);
  if constexpr (MAXPLUS) {
    if (a.path && it.path_off >= 0) {
      drain_vmem();
      __syncthreads();   // every word written
      if (wave == 0)
        score_backtrace(a.path + it.path_off, T, S, [&](int tt, int jj) -> bool {
          const int uu = jj / R, rr = jj - uu * R;
          return (score_word_wt(bits + (size_t)tt * nw + (uu >> 6) * R + rr) >> (uu & 63)) & 1ull;
        });
    }
  }
}

// ---- S > CTC_SMAX_LDS: the label axis in rounds of 256, the previous row read back from the workspace (system-scope accesses
// + one barrier per frame: the rows are written and read by different waves) ---------------------------------------------
template <bool MAXPLUS>
DEVFN void score_rounds(const ScoreArgs& a, const ScoreItem it, const float* P, const double* inv, float* rows,
                        unsigned long long* bits, const CrTables tb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int T = it.T, S = it.S, nc = a.nc, nw = (S + 63) / 64;
  const BufF32 pb = make_buf(P, (size_t)T * nc * 4);
  for (int i = 0; i < T; i++) {
    const double iv = inv[i];
    const BufF32 cur = make_buf(rows + ((i & 1) ? S : 0), (size_t)S * 4), nxt = make_buf(rows + ((i & 1) ? 0 : S), (size_t)S * 4);
    for (int j0 = 0; j0 < S; j0 += SCORE_THREADS) {
      const int j = j0 + tid;
      const bool in = j < S;
      const int cls = a.states[it.soff + (in ? j : 0)];
      const float lmv = score_lmatch(buf_load(pb, in ? (unsigned)(i * nc + cls) * 4u : BUF_OOB), iv, tb);
      const unsigned jo = in ? (unsigned)j * 4u : BUF_OOB;
      const float vj = i == 0 ? (float)(-5.0 * j) : buf_load_wt(cur, jo);
      const float w = j == 0 ? (float)(-5.0 * i) : (i == 0 ? (float)(-5.0 * (j - 1)) : buf_load_wt(cur, in ? jo - 4u : BUF_OOB));
      const float same = vj + lmv, next = w + lmv;
      float vn;
      if constexpr (MAXPLUS) {
        const bool ad = in && next > same;
        vn = ad ? next : same;
        const unsigned long long word = wave_ballot(ad);
        const int wi = (j0 >> 6) + wave;
        if (lane == 0 && wi < nw) bits[(size_t)i * nw + wi] = word;
      } else {
        vn = ctc_log_add<false>(same, next, tb);
      }
      buf_store_wt(nxt, jo, vn);
    }
    drain_vmem();
    __syncthreads();
  }
  const BufF32 outb = make_buf(a.score, (size_t)a.ncand * 4);
  if (tid < 64) {
    const float vs = buf_load_wt(make_buf(rows + ((T & 1) ? S : 0), (size_t)S * 4), (unsigned)(S - 1) * 4u);
    buf_store(outb, tid == 0 ? (unsigned)it.out * 4u : BUF_OOB, vs);
  }
  if constexpr (MAXPLUS) {
    if (a.path && it.path_off >= 0 && wave == 0)
      score_backtrace(a.path + it.path_off, T, S, [&](int tt, int jj) -> bool {
        return (score_word_wt(bits + (size_t)tt * nw + (jj >> 6)) >> (jj & 63)) & 1ull;
      });
  }
}

template <bool MAXPLUS>
__global__ __launch_bounds__(SCORE_THREADS) void ctc_score_kernel(ScoreArgs a) {
  float* lds = dyn_smem<float>();
  const ScoreLds L = score_lds_layout(a.tmax, a.tile, a.ncp, MAXPLUS);
  double* tabs = reinterpret_cast<double*>(lds + L.tables);
  const CrTables tb{tabs, tabs + 32, tabs + 96, tabs + 160};
  const int tid = threadIdx.x, wave = wave_uniform(tid >> 6);
  const ScoreGroup g = a.groups[blockIdx.x];
  const ScoreItem it0 = a.items[g.first];
  for (int i = tid; i < CTC_TABLE_DOUBLES; i += SCORE_THREADS) tabs[i] = a.tables[i];
  const float* P = a.P + (size_t)it0.off * a.nc;   // the group's line
  double* wsd = reinterpret_cast<double*>(a.ws + it0.ws_off);
  double* inv = g.form == 0 ? reinterpret_cast<double*>(lds + L.inv) : wsd;
  const bool resident = g.form == 0 && g.lml != 0;   // the line's posteriors fit the tile whole: they become its match scores
  score_frame_norms(P, it0.T, a.nc, a.ncp, a.tile, lds + L.rowbuf, inv, resident, tb);
  __syncthreads();   // (forms 1, 2: the normalisers are in memory, first read here)
  if (g.form == 0) {
    if (wave < g.n) {
      unsigned long long* bitsw = reinterpret_cast<unsigned long long*>(lds + L.bits) + (MAXPLUS ? wave * a.tmax : 0);
      if (resident) score_one_wave<MAXPLUS, true>(a, a.items[g.first + wave], P, inv, bitsw, lds + L.rowbuf, tb);
      else score_one_wave<MAXPLUS, false>(a, a.items[g.first + wave], P, inv, bitsw, lds + L.rowbuf, tb);
    }
  } else {
    float* rows = reinterpret_cast<float*>(wsd + it0.T);                          // two rows of S floats = S words
    unsigned long long* bits = a.ws + it0.ws_off + it0.T + it0.S;
    if (g.form == 1) score_regs<MAXPLUS>(a, it0, P, inv, bits, lds + L.vx, tb);
    else score_rounds<MAXPLUS>(a, it0, P, inv, rows, bits, tb);
  }
}

}  // namespace clstm
