// lstm_bwd_dw.h -- the backward recurrence and its weight-gradient GEMM as ONE launch with two workgroup roles.
//
// The recurrence occupies 2 x lines workgroups (128 at the bench minibatch) of a 256-CU chip for ~95 us while the
// split-K weight-gradient GEMM behind it (gemm_dw.h: its slabs follow the recurrence's iterations) needs the whole
// chip for ~52 us.  Running the GEMM on a second stream costs more than it saves (fork and join through events
// ~37 us, profiles/r02_timeline_overlap.txt).  Here both live in one grid: blocks [0, nrec) walk their line exactly as
// lstm_bwd_kernel does -- they are dispatched first, never wait for anything and run at raised priority -- the block
// behind them is the monitor, and every further block computes ONE (slab, output tile) item of the GEMM as soon as every
// line reports the slab's iterations complete (gemm_dw_body).  (Persistent workers pulling items from per-XCD queues were
// measured slower -- 0.362 vs 0.356 ms per step: a 448-thread slot per worker leaves room for two on an idle CU.)
#pragma once
#include "gemm_dw.h"
#include "lstm_seq.h"
#include "lstm_xd_prologue.h"

namespace clstm {

// The item role's k-tile table area: 1024 entries although the items use DW_STAB_MAX = 256 -- 8 KB more than they need, on
// purpose: with 50 KB a third item workgroup fits a CU beside the recurrence's, and the 64-line step measured 0.3 us slower for
// it (three interleaved runs, 0.2866 vs 0.2861 ms)
constexpr int DW_FUSED_STAB_ENTRIES = 1024;
static_assert(DW_FUSED_STAB_ENTRIES >= DW_STAB_MAX, "the items' k-tile table fits");
static_assert(xd_smem_floats(2) <= dw_img_floats(2) && xd_smem_floats(3) <= dw_img_floats(3), "the recurrence role's x.d prologue stages in the items' carve");

// NT: the weight-gradient items' arithmetic (gemm_dw_body): 0 f32 MFMA, 2 / 3 bf16 terms per operand
template <int NK4, int KU, int NT>
__global__ __launch_bounds__(64 * NK4) CLSTM_TWO_WAVES_PER_SIMD void lstm_bwd_dw_kernel(LstmSeqArgs a, GemmDwArgs g, int nrec) {
  __shared__ __attribute__((aligned(16))) float gsm[dw_img_floats(NT) + 2 * DW_FUSED_STAB_ENTRIES];
  if ((int)blockIdx.x < nrec) {
#ifndef CLSTM_HIP_EMU
    __builtin_amdgcn_s_setprio(3);
#endif
    const long long t0 = g.trace ? wall_clock() : 0;
    const int bl = (int)blockIdx.x % a.bs;
    const int b = a.order ? a.order[bl] : bl, dir = (int)blockIdx.x / a.bs;
    // top layer: the workgroup first computes its own slice of dH (the recurrence role has no other use for gsm); this sits in
    // front of the body's recurrent-weight loads, so the two register populations are never live together.  Producer form
    // (g.xd.ready): only the 32 frames it visits first; the helper items behind the monitor compute the rest and the body checks
    // their word before its prefetch enters a round it did not make.
    bool producers = false;
    if constexpr (NT >= 2) {
      if (g.xd.A.p) {
        producers = g.xd.ready != nullptr;   // (kernel argument: uniform)
        if (producers) xd_own_round<NT, xd_maxu(NK4)>(gsm, g.xd, a.line_off, b, dir, a.no);
        else xd_prologue<NT, xd_maxu(NK4)>(gsm, g.xd, a.line_off, b, dir, a.no);
      }
    }
    const long long t1 = g.trace ? wall_clock() : 0;
    if constexpr (NT >= 2) {
      if (producers) lstm_bwd_body<NK4, KU, true>(a, b, dir, g.xd.ready + ((size_t)dir * a.bs + b) * PROG_STRIDE, g.xd.ready0);
      else lstm_bwd_body<NK4, KU>(a, b, dir);
    } else lstm_bwd_body<NK4, KU>(a, b, dir);
    if (g.done && threadIdx.x == 0) atomic_add_i32(g.done, 1);   // (the body ended with drain + barrier: this line's deltas are in memory)
    if (g.trace && threadIdx.x == 0) { g.trace[blockIdx.x * 4] = t0; g.trace[blockIdx.x * 4 + 1] = t1; g.trace[blockIdx.x * 4 + 2] = wall_clock(); }
  } else {
    unsigned blk = blockIdx.x - (unsigned)nrec;
    if constexpr (NT >= 2) {
      // producer form: the dH items sit behind the monitor and in front of everything that waits -- one per recurrence workgroup,
      // in the same (longest line first) order; they never wait, and all waves of the launch stay for them
      if (g.xd.ready) {
        if (blk >= 1u && blk <= (unsigned)nrec) { xd_item<NT, xd_maxu(NK4)>(gsm, g.xd, a.line_off, a.order, a.bs, (int)blk - 1, a.no); return; }
        if (blk > (unsigned)nrec) blk -= (unsigned)nrec;
      }
    }
    if (threadIdx.x >= 256) return;   // the GEMM role is four waves; the others retire (a barrier counts live waves only)
    gemm_dw_body<NT>(g, gsm, blk);   // the monitor, then one item per workgroup in dispatch order
  }
}

}  // namespace clstm
