// lstm_xd_prologue.h -- the softmax layer's x.d = z.d . W, computed by the workgroup that reads it.
//
// The backward recurrence workgroup of (line b, direction d) is the only reader of dH[frames of b][d*no .. d*no+no).  As a
// launch of its own that product (12800 x 200 x 83 at the bench shape) pays ~12 us for well under 2 us of MFMA work.  Here every
// recurrence workgroup computes its own T x no x nc slice in front of its first step, on the matrix cores its CU leaves idle,
// stores it, meets at ONE barrier and starts the time loop.  Producer and consumer are the same workgroup: no flag, no poll.
// (Producer form, further down: only the 32 frames the workgroup visits first are computed here, helper workgroups of the fused
// launch compute the others while the time loop already runs.)
//
// Arithmetic: gemm_x3_body<GEMM_KC, GEMM_KC, StorePlain, NT> (gemm_bf16.h), expression for expression -- the same term split
// (bf16_pack8, then the exact remainder), contraction indices >= nc zeroed, accumulators from zero, k-blocks ascending, inside a
// block the products in the order w = NT-1..0, ta = w..0, and the same eight consecutive k per lane group in every MFMA -- so
// every element of dH is bit-identical to what the launch stored.  (That launch always runs a multiple of three k-blocks; so
// does this: XD_KB = 3 blocks, the ones past nc all zero.  Hence nc <= XD_MAX_K.)
//
// Work split: wave w owns column tile w (16 columns; the host launches 64 * ceil(no / 16) threads, so every tile has a wave) and
// keeps its W fragments in registers (3 blocks x NT terms x 4 VGPRs).  z.d is staged by all threads as swizzled bf16 term images
// in rounds of XD_ROWS = 32 frames, double-buffered in LDS: one barrier per round, the loads of rounds r + 1 .. r + 3 in flight
// under the MFMAs of round r (a ring of three register sets; one round ahead left every round waiting for memory).  The barrier inside the loop is a bare s_barrier behind this wave's LDS writes: __syncthreads() would also
// wait for the dH stores of the round before.
#pragma once
#include "gemm_dw.h"
#include "lstm_seq.h"

namespace clstm {

constexpr int XD_KB = 3;                 // k-blocks of 32: what gemm_x3_body runs for K <= 96
constexpr int XD_MAX_K = 32 * XD_KB;
constexpr int XD_ROWS = 32;              // frames per round (two 16-row MFMA tiles)
constexpr int XD_UNITS = XD_ROWS * XD_KB * 4;   // staging units of a round: 8 consecutive k of one row
constexpr int XD_RING = 3;               // rounds of z.d in flight in registers
// staging units per thread: the smallest workgroup of an NK4 instantiation (narrow_class: 1 -> one wave, 2 -> two, 4 -> three,
// 7 -> five, 8 -> eight) still covers a round; the host checks nthreads * xd_maxu >= XD_UNITS
constexpr int xd_maxu(int nk4) { return nk4 <= 1 ? 6 : nk4 == 2 ? 3 : nk4 <= 7 ? 2 : 1; }
constexpr int xd_smem_floats(int nt) { return 2 * nt * XD_KB * XD_ROWS * 32 / 2; }   // 24 KB (NT = 2) / 36 KB (NT = 3)

// xd_rounds: `nr` rounds of one (line, direction) -- round p is the 32 frames from row0 + p * rstep on; frames outside [0, T)
// are neither read nor stored, so a round may hang over either end of the line.  Both callers of the producer form share this
// body with the whole prologue: the recurrence role computes the round it visits first, a helper item the others in the order the
// recurrence reaches them.  A row of dH depends on nothing but its own row of z.d, so which round (and which workgroup) computes a
// frame does not change its bytes.
// WT: the rows leave write-through (sc0 sc1), for readers on another XCD.  word != nullptr (WT only): after every round each wave
// drains its stores, the workgroup meets at the round's barrier, and one lane publishes word0 + rounds complete at system scope --
// word0 is the launch's prog_base, so a word left by an earlier pass is below every value this one waits for.
template <int NT, int MAXU, bool WT = false>
DEVFN void xd_rounds(float* smem, const XdArgs& x, const int* line_off, const int b, const int dir, const int no,
                     const int row0, const int rstep, const int nr, int* word = nullptr, const int word0 = 0) {
  static_assert(NT == 2 || NT == 3, "two or three bf16 terms per operand");
  unsigned short* img = reinterpret_cast<unsigned short*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const int nthreads = blockDim.x;
  const int off = line_off[b];
  const int T = line_off[b + 1] - off;
  if (T <= 0) return;
  const int K = x.K;
  const BufF32 abuf = make_buf(x.A.p + (size_t)off * x.A.ld, (size_t)(x.A.elems - (long long)off * x.A.ld) * 4);
  const BufF32 bbuf = make_buf(x.B.p, (size_t)x.B.elems * 4);
  const BufF32 obuf = make_buf(x.out + (size_t)off * x.ld, (size_t)T * x.ld * 4);
  const int fk = lane >> 4, fi = lane & 15;
  constexpr int IMG = XD_ROWS * 32;            // halfs per (term, k-block) image
  constexpr int BUFH = NT * XD_KB * IMG;       // halfs per buffer

  // staging unit u of a round: row u / 12 of the round, k-block (u % 12) >> 2, k = 8 ((u % 12) & 3) .. + 7 of the block
  auto load_round = [&](const int r, f32x4 (&ra)[MAXU][2]) {   // (rounds past the line: every lane out of range, zeros)
#pragma unroll
    for (int i = 0; i < MAXU; i++) {
      if (i * nthreads + (tid & ~63) >= XD_UNITS) break;   // (wave-uniform)
      const int u = i * nthreads + tid;
      const int row = row0 + r * rstep + u / (XD_KB * 4), ku = u % (XD_KB * 4);
      const unsigned o = u < XD_UNITS && r < nr && (unsigned)row < (unsigned)T ? ((unsigned)row * (unsigned)x.A.ld + (unsigned)((ku >> 2) * 32 + (ku & 3) * 8)) * 4u : BUF_OOB_BASE;
      ra[i][0] = buf_load4(abuf, o);
      ra[i][1] = buf_load4(abuf, o + 16u);
    }
  };
  auto stage_round = [&](unsigned short* dst, const f32x4 (&ra)[MAXU][2]) {
#pragma unroll
    for (int i = 0; i < MAXU; i++) {
      if (i * nthreads + (tid & ~63) >= XD_UNITS) break;
      const int u = i * nthreads + tid;
      if (u < XD_UNITS) {
        const int row = u / (XD_KB * 4), ku = u % (XD_KB * 4), kb = ku >> 2, kk = (ku & 3) * 8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = kb * 32 + kk + e < K ? ra[i][e >> 2][e & 3] : 0.0f;
        const int o = kb * IMG + row * 32 + (((kk >> 3) ^ gb2_sw(row)) << 3);
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const u16x8 h = bf16_pack8(v);
          *reinterpret_cast<u16x8*>(dst + t * XD_KB * IMG + o) = h;
          if (t + 1 < NT) {
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] -= __builtin_bit_cast(float, (unsigned)h[e] << 16);
          }
        }
      }
    }
  };

  // z.d rounds 0 .. XD_RING-1 are requested first, W behind them: one memory latency for both
  f32x4 ring[XD_RING][MAXU][2];
#pragma unroll
  for (int p = 0; p < XD_RING; p++) {
    load_round(p, ring[p]);
    SCHED_FENCE();
  }

  // this wave's W fragments: column n = 16 wave + fi, k = 32 kb + 8 fk .. + 7, split into NT terms
  const int n = wave * 16 + fi;
  const bool has_tile = wave * 16 < no;        // (wave-uniform; the spare waves of a wider launch only help stage)
  u16x8 bt[XD_KB][NT];
  if (has_tile) {
    const unsigned brow = n < no ? (unsigned)(dir * no + n) * (unsigned)x.B.ld * 4u : BUF_OOB_BASE;
    f32x4 rb[XD_KB][2];
#pragma unroll
    for (int kb = 0; kb < XD_KB; kb++) {
      rb[kb][0] = buf_load4(bbuf, brow + (unsigned)(kb * 32 + fk * 8) * 4u);
      rb[kb][1] = buf_load4(bbuf, brow + (unsigned)(kb * 32 + fk * 8 + 4) * 4u);
    }
#pragma unroll
    for (int kb = 0; kb < XD_KB; kb++) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; i++) v[i] = kb * 32 + fk * 8 + i < K ? rb[kb][i >> 2][i & 3] : 0.0f;
#pragma unroll
      for (int t = 0; t < NT; t++) {   // term t, then the exact remainder
        const u16x8 h = bf16_pack8(v);
        bt[kb][t] = h;
        if (t + 1 < NT) {
#pragma unroll
          for (int i = 0; i < 8; i++) v[i] -= __builtin_bit_cast(float, (unsigned)h[i] << 16);
        }
      }
    }
  }

  const int fofs = fi * 32 + ((fk ^ gb2_sw(fi)) << 3);   // (rows 16 apart share the swizzle)
  const unsigned ocol = n < no ? (unsigned)(dir * no + n) * 4u : BUF_OOB_BASE;
  auto round = [&](const int r, f32x4 (&ra)[MAXU][2]) {
    unsigned short* cur = img + (r & 1) * BUFH;
    stage_round(cur, ra);
    // every wave's images of this round are in LDS (the other buffer's readers passed the barrier of the round before)
    wait_lgkmcnt0();
    if constexpr (WT) {
      if (word) drain_vmem();                  // this wave's rows of the rounds before are in memory ...
    }
    wg_barrier();
    COMPILER_MEMORY_BARRIER();
    if constexpr (WT) {
      if (word && r > 0 && tid == 0) store_i32_wt(word, word0 + r);   // ... and now every wave's: rounds < r are complete
    }
    load_round(r + XD_RING, ra);   // into the set this round has just staged from: in flight for XD_RING rounds
    SCHED_FENCE();
    if (has_tile) {
      f32x4 acc[2];
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[m][q] = 0.0f;
#pragma unroll
      for (int kb = 0; kb < XD_KB; kb++) {
        u16x8 at[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int m = 0; m < 2; m++) at[t][m] = *reinterpret_cast<const u16x8*>(cur + (t * XD_KB + kb) * IMG + m * 16 * 32 + fofs);
        // smallest terms first: ta + tb = NT - 1 .. 0
#pragma unroll
        for (int w = NT - 1; w >= 0; w--)
#pragma unroll
          for (int ta = w; ta >= 0; ta--)
#pragma unroll
            for (int m = 0; m < 2; m++) acc[m] = mfma16x16x32_bf16(at[ta][m], bt[kb][w - ta], acc[m]);
      }
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int row = row0 + r * rstep + m * 16 + fk * 4 + q;
          const unsigned o = (unsigned)row < (unsigned)T ? (unsigned)row * (unsigned)x.ld * 4u + ocol : BUF_OOB_BASE;
          if constexpr (WT) buf_store_wt(obuf, o, acc[m][q]);
          else buf_store(obuf, o, acc[m][q]);
        }
    }
  };
  for (int r = 0; r < nr; r += XD_RING) {
#pragma unroll
    for (int p = 0; p < XD_RING; p++)
      if (r + p < nr) round(r + p, ring[p]);
  }
  // every dH store of every wave acknowledged, then one barrier, then the recurrence's first loads / the last publication
  drain_vmem();
  __syncthreads();
  if constexpr (WT) {
    if (word && tid == 0) store_i32_wt(word, word0 + nr);
  }
}

// the whole prologue: every round of the line, in frame order
template <int NT, int MAXU>
DEVFN void xd_prologue(float* smem, const XdArgs& x, const int* line_off, const int b, const int dir, const int no) {
  const int T = line_off[b + 1] - line_off[b];
  xd_rounds<NT, MAXU>(smem, x, line_off, b, dir, no, 0, XD_ROWS, (T + XD_ROWS - 1) / XD_ROWS);
}

// ---- the producer form (experiment option xd_prologue=2, fused launch only) ------------------------------------------------------
// The recurrence reads dH[t] two steps before it uses it and reaches the frames of its k-th 32 iterations only ~15 k us into its
// time loop: only the round it visits FIRST has to exist before step 0.  Rounds are counted in visit order -- visit round j is
// iterations 32 j .. 32 j + 31: frames 32 j .. for direction 1, frames T - 32 (j + 1) .. T - 32 j - 1 for direction 0, which
// walks the line backwards (so the short round of a line whose length is no multiple of 32 is the LAST visited in both).
// The recurrence workgroup computes visit round 0; item (line, direction) of the helper role computes rounds 1 .. in visit order
// and publishes after each (xd_rounds); lstm_bwd_body<.., XDP> checks the word before its prefetch enters a round.
DEVFN int xd_visit_rounds(const int T) { return (T + XD_ROWS - 1) / XD_ROWS; }
template <int NT, int MAXU>
DEVFN void xd_own_round(float* smem, const XdArgs& x, const int* line_off, const int b, const int dir, const int no) {
  const int T = line_off[b + 1] - line_off[b];
  xd_rounds<NT, MAXU, true>(smem, x, line_off, b, dir, no, dir == 0 ? T - XD_ROWS : 0, 0, 1);
}
// helper item i: the rounds of the line and direction that recurrence workgroup i walks (every wave of the launch stays: one
// per column tile, as in the recurrence role).  Lines of at most 32 frames have nothing left to compute.
template <int NT, int MAXU>
DEVFN void xd_item(float* smem, const XdArgs& x, const int* line_off, const int* order, const int bs, const int i, const int no) {
  const int bl = i % bs, dir = i / bs;
  const int b = order ? order[bl] : bl;
  const int T = line_off[b + 1] - line_off[b];
  const int nv = xd_visit_rounds(T);
  if (nv <= 1) return;
  xd_rounds<NT, MAXU, true>(smem, x, line_off, b, dir, no, dir == 0 ? T - 2 * XD_ROWS : XD_ROWS, dir == 0 ? -XD_ROWS : XD_ROWS, nv - 1,
                            x.ready + ((size_t)dir * bs + b) * PROG_STRIDE, x.ready0);
}

// the per-line backward kernel with the prologue in front: the two-launch form of the overlapped backward pass
// (layers of fewer than four waves, the host emulator)
template <int NK4, int KU, int NT>
__global__ __launch_bounds__(64 * NK4) CLSTM_TWO_WAVES_PER_SIMD void lstm_bwd_xd_kernel(LstmSeqArgs a, XdArgs x) {
  __shared__ __attribute__((aligned(16))) float xsm[xd_smem_floats(NT)];
  const int b = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
  xd_prologue<NT, xd_maxu(NK4)>(xsm, x, a.line_off, b, (int)blockIdx.y, a.no);
  lstm_bwd_body<NK4, KU>(a, b, (int)blockIdx.y);
}

}  // namespace clstm
