// ctc_beam.h -- CTC prefix beam search on device: the n best labellings of a line, one workgroup per line, every frame of the line
// walked in one launch.
//
// Plain posteriors, class 0 = blank, lp[t][c] = log(max(p[t][c], 1e-30f)), all arithmetic f32.  A beam entry is a label sequence l
// with lb (log-probability of the paths so far that collapse to l and end in blank) and lnb (those that end in l's last label);
// tot = logadd(lb, lnb).  Start: l = (), lb = 0, lnb = -inf.  Per frame, from the current entries:
//   stay i (last label e)   lb' = tot_i + lp[0];  lnb' = lnb_i + lp[e] (-inf for the empty prefix);  when l_i minus its last label is
//                           entry j of the beam: lnb' = logadd(lnb', lp[e] + (last(l_j) == e ? lb_j : tot_j))        (the merge)
//   extend i by c != 0      not when l_i + c is itself an entry (the merge counted it there);  lb' = -inf,
//                           lnb' = lp[c] + (c == e ? lb_i : tot_i)
// and the `beam` candidates of largest logadd(lb', lnb') are kept (never one of -inf).  After the last frame the first nbest entries
// by tot leave, best first.  These scores are true log-probabilities of a labelling (sums over a subset of its paths): they are NOT
// comparable with ctc_score.h's unnormalised score (skip = -5 per state and frame, posteriors floored at 1e-5 and renormalised).
//
// Selection is a total order: the key of a candidate is (orderable score bits, ~index) in 64 bits, index = i for stay i and
// beam + i nc + c for extension (i, c); key 0 = no candidate.  The rank of a candidate is the number of larger keys, counted in LDS
// in two passes: against the first 64 keys only (the stays and every entry's best extensions) -- a candidate that already finds
// `beam` larger keys there is out, and everything larger than a candidate that is in survives this --, then among the survivors.
// A candidate of rank r < beam becomes entry r of the next frame, so the beam is always sorted and the result of a line depends on
// nothing but the line.
//
// Which extensions can win does not depend on the chain: an entry's extensions are ordered by lp[c] alone (c == e only loses by
// it: lb <= tot), and at most beam - 1 of them are skipped.  So only the K = min(nc - 1, 2 beam) classes of largest lp of a frame
// are candidates at all; the prologue ranks every frame's classes with all threads, and the chain looks at beam (1 + K) candidates
// per frame whatever nc is.  (Where lp values tie exactly, a class outside those K could have tied with the last one kept: the rule
// "the K largest by (lp bits, smaller class first)" is as deterministic as any.)
//
// Prefixes live in a trie (parent, label, depth per node; at most 1 + T beam nodes), identity is by content: (parent, label) -> node
// goes through an open-addressed table that persists for the whole line, so a prefix that leaves the beam and is extended again is
// the same node and its descendants keep merging.  "l_i + c is an entry" and "the parent of l_i is an entry" are then comparisons of
// node ids within the beam.  Table, nodes, the per-frame class lists and the line's lp each lie in LDS when the line's fit (the host
// decides per line, BeamLine::in_lds) and in the workspace otherwise; the code is the same, only slower.  The trie is touched by
// wave 0 alone: look-ups one entry per lane, the few insertions one lane at a time.
//
// ---- with a character n-gram language model (ctc_beam_kernel<.., true>: clstm_ctc_beam_lm_batch / clstm_net_beam_lm) ----
// The model is a dense f32 table lm[ctx][c] of order 2 or 3: nc^(order-1) rows of nc columns, labels 1 .. nc-1, 0 = "no label yet".
// Order 2: ctx = the last label (0 for the empty prefix); order 3: ctx = nc (the label before last, or 0) + the last label.
// Column 0 (blank) is never read.  An end table end[ctx] is optional.  Entries are finite (checked at creation), not necessarily
// normalised.  The LM value of a prefix: lm(()) = 0, lm(l + c) = lm(l) + (weight lm[ctx(l)][c] + bonus), f32 in exactly that
// association (beam_lm_term: the product rounded, then the sum), weight >= 0.  It depends on the prefix alone, so it is stored once per
// trie node when the node is made (nlm, nctx beside parent / label / depth); a prefix that leaves the beam and is extended again
// finds its node and with it the same value.  A stay adds nothing; the second a of "a a" (through a blank) is an extension and adds
// its term.
//   (lb, lnb), stay, merge, extend and tot are the expressions above, unchanged.  Only selection changes: the key of a candidate is
// (logadd(lb', lnb') + lm(its prefix), ~index) -- -inf stays -inf and is never kept --, index and total order as above.  The key no
// longer carries a candidate's acoustic value: a kept stay takes tot from stay_tot, a kept extension recomputes lp[c] + (c == e ?
// lb_i : tot_i), the same expression on the same operands.  After the last frame the live entries are ranked by
// (tot + lm(l)) + weight end[ctx(l)] (the last term with an end table only), key (that total, ~entry position), and the first nbest
// leave with two scores: that total, and the acoustic tot -- the log-probability the beam gathered, what the search without a model
// reports.
//   The class list is lossless by being complete: with a model every entry has its own order of extensions, so K = nc - 1 and every
// class is a candidate of every entry, beam (nc - 1) <= BEAM_LM_CANDS extension keys per frame (the host refuses more).  The
// prologue still sorts a frame's classes by lp: the order decides nothing, it only puts the acoustically likely candidates in front
// of the key list, where the first counting pass finds them.  That list (2 T (nc - 1) words) always lies in the workspace -- it is
// read one frame ahead into the small LDS tile --, so ALL_LDS here means the other three sections.  Each entry gets ctx and lm from
// its node when phase C names the node, so phase A reads them from LDS; the table itself lies in global memory (one read per
// candidate, rows of one context contiguous).
//
// ---- constrained to a lexicon (ctc_beam_kernel<.., true, true>: clstm_ctc_beam_lex_batch / clstm_net_beam_lex) ----
// A lexicon over nc classes has a flag per class, word_class[c]; class 0 (blank) is never a word class, the classes 1 .. nc-1 without
// the flag are separators (space, punctuation, digits: whatever the caller leaves out), and a set of words: non-empty label sequences
// over word classes.  The words form a trie with root 0; a node is terminal when a word ends there.  Every prefix l has a lexicon
// state: x(()) = root; x(l + c) = root when c is a separator, allowed only if x(l) is the root or terminal; x(l + c) = child(x(l), c)
// when c is a word class, allowed only if that child exists.  The second a of "a a" (through a blank) is an extension and moves the
// state; a stay moves nothing.
//   The search is the language model form above, expression for expression: (lb, lnb), stay, merge, extend, tot, the key
// (logadd(lb', lnb') + lm(prefix), ~index), the same index and total order.  One difference: an extension (i, c) that is not allowed
// is no candidate (key 0).  The character model is optional: without one (table == null) the table term is that of an all-zero table,
// lm(l + c) = lm(l) + (weight 0 + bonus), and there is no end table.  After the last frame only the live entries whose state is the
// root or terminal are ranked, by the LM form's final ranking; nhyp = min(nbest, their number), which can be 0: then len = 0, both
// scores -inf and the label slots zero, exactly what a line without frames reports.
//   Device form (BeamArgs::lex, one buffer of 32-bit words): [nodes, edges, W = ceil(nc / 32), 0], then per node W words of allowed
// next classes -- bit c of a row: (i, c) is allowed, separators set on the root and on terminal nodes, and bit 0 (blank is no class)
// says "root or terminal" --, then a CSR of children: nodes + 1 offsets, the labels sorted within a node, the targets.  "Is (i, c)
// allowed" is one bit test, the same for both kinds of class.  The state depends on the prefix alone, so it is the sixth array of the
// trie (nlex, beside nlm / nctx), written once by the lane that makes the node: a binary search over the parent state's children,
// bounded by the child count; a class that was allowed and is no child is a separator (-> root).  A prefix that leaves the beam and
// is extended again finds its node and with it the same state.  Phase C copies the new entries' rows to LDS (n W words, at most
// 32 x 129), so phase A makes no extra global read per candidate, and the final ranking reads bit 0 there.
#pragma once
#include "devintrin.h"
#include <math.h>

namespace clstm {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX = 32;
constexpr int BEAM_LM_CANDS = 4096;         // with a language model: beam (nc - 1), the extension keys of a frame, at most
constexpr int BEAM_LDS_WORDS = 36 * 1024;   // of the 40 K words (160 KB) of a CU: fixed part + the sections of a line that fit
enum BeamSection { BS_HASH = 0, BS_NODES, BS_CLS, BS_LP, BS_COUNT };

// off[s]: word offset of section s, in the LDS carve's section area (in_lds bit s) or in the workspace
struct BeamLine { long long off[BS_COUNT]; int in_lds, row, T, line, hmask, nnmax; };
struct BeamArgs {
  const BeamLine* lines;
  const float* P;      // [N][nc]
  int* ws;
  int* nhyp;           // [bs]
  int* len;            // [bs nbest]
  float* score;        // [bs nbest]
  int* labels;         // [nbest N], or null
  int nc, beam, nbest, K, bs, N;
  // language model form only
  const float* table;  // [nc^(order-1)][nc]
  const float* end;    // [nc^(order-1)], or null
  float* am_score;     // [bs nbest], or null
  float weight, bonus;
  int order;
  // lexicon form only (the header's third part); then table may be null
  const int* lex;
};
// fixed LDS words in front of the sections
struct BeamLds { int ent, stay, misc, ft, keys, surv, lm, lex, sections; };
constexpr int BEAM_ENT_FIELDS = 7;   // node, last, lb, lnb, tot, ppos, pnode / written flag
constexpr int BEAM_LM_WORDS = 5 * BEAM_MAX;   // language model form: ctx and lm of the entries, double-buffered, and the stays' tot
inline __host__ __device__ int beam_lex_words(int nc) { return (nc + 31) >> 5; }   // lexicon form: words of a node's row of allowed classes
// lex_rows: the entries' rows of allowed classes, beam * beam_lex_words(nc) (lexicon form), else 0
inline __host__ __device__ BeamLds beam_lds_layout(int beam, int K, bool lm = false, int lex_rows = 0) {
  BeamLds l;
  int o = 0;
  l.keys = o; o += 2 * (beam + beam * K);       // 64-bit keys first: 8-byte aligned
  l.surv = o; o += 2 * (beam + beam * K);       // the keys that may still be among the `beam` largest
  l.ent = o;  o += 2 * BEAM_ENT_FIELDS * BEAM_MAX;
  l.stay = o; o += 2 * BEAM_MAX;
  l.ft = o;   o += 2 * (2 * K + 2);             // the next frame's class list, their lp and lp[0], double-buffered
  l.misc = o; o += 4;
  l.lm = o;   o += lm ? BEAM_LM_WORDS : 0;
  l.lex = o;  o += lex_rows;
  o += o & 1;
  l.sections = o;
  return l;
}
inline __host__ __device__ int beam_classes(int nc, int beam) { return nc - 1 < 2 * beam ? nc - 1 : 2 * beam; }

DEVFN float beam_neg_inf() { return -__builtin_inff(); }
DEVFN float beam_logadd(float a, float b) {
  const float m = a > b ? a : b;
  if (m == beam_neg_inf()) return m;
  return m + log1pf(expf(-fabsf(a - b)));
}
DEVFN unsigned beam_ord(float x) {   // larger float <-> larger unsigned
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEVFN float beam_unord(unsigned o) { return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
DEVFN unsigned long long beam_key(float s, unsigned index) {
  const unsigned o = beam_ord(s);
  return o <= 0x007FFFFFu ? 0ull : (((unsigned long long)o << 32) | (unsigned)~index);   // -inf (and below): never kept
}
// weight x + bonus with the product rounded before the sum (no fused multiply-add: the referee's two roundings)
DEVFN float beam_lm_term(float weight, float x, float bonus) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float p = weight * x;
  return p + bonus;
}
DEVFN unsigned beam_hash(int parent, int label) {
  unsigned h = (unsigned)parent * 0x9E3779B1u ^ ((unsigned)label * 0x85EBCA6Bu + 0x7F4A7C15u);
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 13;
  return h;
}

// one side of the double-buffered beam
struct BeamEnt { int* node; int* last; float* lb; float* lnb; float* tot; int* ppos; int* aux; };
DEVFN BeamEnt beam_ent(float* base, int side) {
  float* p = base + side * BEAM_ENT_FIELDS * BEAM_MAX;
  BeamEnt e;
  e.node = reinterpret_cast<int*>(p); e.last = reinterpret_cast<int*>(p + BEAM_MAX);
  e.lb = p + 2 * BEAM_MAX; e.lnb = p + 3 * BEAM_MAX; e.tot = p + 4 * BEAM_MAX;
  e.ppos = reinterpret_cast<int*>(p + 5 * BEAM_MAX); e.aux = reinterpret_cast<int*>(p + 6 * BEAM_MAX);
  return e;
}

// ALL_LDS: every section of every line of the launch lies in LDS (the OCR shapes): the section pointers are LDS addresses the
// compiler can see, not a choice between two address spaces that only flat instructions can follow.  The arithmetic is the same.
// LM: the language model form (the header's second part); without it the kernel is the plain search, instruction for instruction.
// LEX: the lexicon form (the third part), on top of LM only: <.., true, true>.
template <bool ALL_LDS, bool LM = false, bool LEX = false>
__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_kernel(BeamArgs a) {
  float* lds = dyn_smem<float>();
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_uniform(tid >> 6);
  const BeamLine ln = a.lines[blockIdx.x];
  const int T = ln.T, nc = a.nc, beam = a.beam, K = a.K;
  static_assert(LM || !LEX, "the lexicon rides the complete-class-list form");
  const int W = LEX ? beam_lex_words(nc) : 0;
  const BeamLds L = beam_lds_layout(beam, K, LM, beam * W);
  auto section = [&](int s) -> int* {
    if (LM && s == BS_CLS) return a.ws + ln.off[s];   // (the complete class list: always in the workspace)
    if constexpr (ALL_LDS) return reinterpret_cast<int*>(lds + L.sections) + (int)ln.off[s];
    else return (ln.in_lds >> s & 1) ? reinterpret_cast<int*>(lds + L.sections) + ln.off[s] : a.ws + ln.off[s];
  };
  int* const tab = section(BS_HASH);
  int* const npar = section(BS_NODES);
  int* const nlab = npar + ln.nnmax;
  int* const ndep = nlab + ln.nnmax;
  int* const nlm = ndep + ln.nnmax;                          // (LM: the prefix's LM value as float bits, then its context)
  int* const nctx = nlm + ln.nnmax;
  int* const nlex = nctx + ln.nnmax;                         // (LEX: the prefix's lexicon state)
  unsigned* const ent_allow = reinterpret_cast<unsigned*>(lds + L.lex);   // (LEX) [beam][W] the current entries' allowed classes
  const int lex_nodes = LEX ? a.lex[0] : 0, lex_edges = LEX ? a.lex[1] : 0;
  const unsigned* const lex_allow = reinterpret_cast<const unsigned*>(a.lex + 4);   // (LEX) [nodes][W]
  const int* const lex_off = a.lex + 4 + (size_t)lex_nodes * W;                   // (LEX) [nodes + 1]
  const int* const lex_lab = lex_off + lex_nodes + 1;                             // (LEX) [edges] sorted within a node
  const int* const lex_tgt = lex_lab + lex_edges;                                 // (LEX) [edges]
  int* const ent_ctx = reinterpret_cast<int*>(lds + L.lm);   // (LM) [side][BEAM_MAX]
  float* const ent_lm = lds + L.lm + 2 * BEAM_MAX;           // (LM) [side][BEAM_MAX]
  float* const stay_tot = lds + L.lm + 4 * BEAM_MAX;         // (LM)
  int* const ccls = section(BS_CLS);                         // [T][K] classes, then [T][K] their lp
  float* const clp = reinterpret_cast<float*>(ccls) + (size_t)T * K;
  float* const lp = reinterpret_cast<float*>(section(BS_LP));   // [T][nc]
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(lds + L.keys);
  unsigned long long* const surv = reinterpret_cast<unsigned long long*>(lds + L.surv);
  float* const stay_lb = lds + L.stay;
  float* const stay_lnb = stay_lb + BEAM_MAX;
  int* const misc = reinterpret_cast<int*>(lds + L.misc);    // [0] nodes so far, [1] live entries, [2] survivors of the frame
  const int ftw = 2 * K + 2;
  const float* P = a.P + (size_t)ln.row * nc;
  const int hmask = ln.hmask;

  // ---- prologue: logs, the empty table, the root, every frame's K best classes ----
  const int nlp = T * nc;
  for (int i = tid; i < nlp; i += BEAM_THREADS) lp[i] = logf(fmaxf(P[i], 1e-30f));
  for (int i = tid; i <= hmask; i += BEAM_THREADS) tab[i] = 0;
  if (tid == 0) {
    npar[0] = -1; nlab[0] = 0; ndep[0] = 0;
    misc[0] = 1; misc[1] = 1; misc[2] = 0;
    const BeamEnt e = beam_ent(lds + L.ent, 0);
    e.node[0] = 0; e.last[0] = 0; e.lb[0] = 0.0f; e.lnb[0] = beam_neg_inf(); e.tot[0] = 0.0f; e.ppos[0] = -1;
    if constexpr (LM) { nlm[0] = 0; nctx[0] = 0; ent_ctx[0] = 0; ent_lm[0] = 0.0f; }
    if constexpr (LEX) nlex[0] = 0;
  }
  if constexpr (LEX) { if (tid < W) ent_allow[tid] = lex_allow[tid]; }   // the empty prefix: the root's row (W <= 129)
  drain_vmem();   // (sections in the workspace: written here, read by other waves -- the trie with system-scope loads)
  __syncthreads();
  const int ncl = nc - 1;   // classes 1 .. nc-1
  for (int i = tid; i < T * ncl; i += BEAM_THREADS) {
    const int t = i / ncl, c = 1 + (i - t * ncl);
    const float* row = lp + (size_t)t * nc;
    const float x = row[c];
    const unsigned o = beam_ord(x);
    int rank = 0;
    for (int c0 = 1; c0 < nc && rank < K; c0 += 8) {   // eight independent reads per look at the count
      float y[8];
#pragma unroll
      for (int u = 0; u < 8; u++) y[u] = row[c0 + u < nc ? c0 + u : c];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const unsigned o2 = beam_ord(y[u]);
        const int c2 = c0 + u;
        rank += (c2 < nc && (o2 > o || (o2 == o && c2 < c))) ? 1 : 0;
      }
    }
    if (rank < K) { ccls[(size_t)t * K + rank] = c; clp[(size_t)t * K + rank] = x; }
  }
  drain_vmem();
  __syncthreads();
  auto stage_frame = [&](int t, int j) {   // frame t's class list into the small LDS tile, by K + 1 threads (j)
    float* ft = lds + L.ft + (t & 1) * ftw;
    if (j < K) { ft[j] = __builtin_bit_cast(float, ccls[(size_t)t * K + j]); ft[K + j] = clp[(size_t)t * K + j]; }
    else if (j == K) ft[2 * K] = lp[(size_t)t * nc];
  };
  if constexpr (LM) { for (int j = tid; j <= K; j += BEAM_THREADS) stage_frame(0, j); }   // (K = nc - 1: more than one round)
  else if (tid <= K) stage_frame(0, tid);
  __syncthreads();

  int n = 1;   // live entries (workgroup-uniform)
  for (int t = 0; t < T; t++) {
    const BeamEnt cur = beam_ent(lds + L.ent, t & 1), nxt = beam_ent(lds + L.ent, (t + 1) & 1);
    const float* ft = lds + L.ft + (t & 1) * ftw;
    const float* row = lp + (size_t)t * nc;
    const int next = n * K, ncand = beam + next;
    const int* const cctx = ent_ctx + (t & 1) * BEAM_MAX;   // (LM) the current entries' context and LM value
    const float* const clm = ent_lm + (t & 1) * BEAM_MAX;
    // ---- A: the candidates' keys; stay i -> keys[i], extension (i, class of rank r) -> keys[beam + r n + i] ----
    if (tid < beam) {
      unsigned long long key = 0ull;
      if (tid < n) {
        const int i = tid, e = cur.last[i], j = cur.ppos[i];
        const float lbn = cur.tot[i] + ft[2 * K];
        float lnbn = beam_neg_inf();
        if (e != 0) {
          const float le = row[e];
          lnbn = cur.lnb[i] + le;
          if (j >= 0) lnbn = beam_logadd(lnbn, le + (cur.last[j] == e ? cur.lb[j] : cur.tot[j]));
        }
        stay_lb[i] = lbn; stay_lnb[i] = lnbn;
        const float totn = beam_logadd(lbn, lnbn);
        if constexpr (LM) { stay_tot[i] = totn; key = beam_key(totn + clm[i], (unsigned)i); }
        else key = beam_key(totn, (unsigned)i);
      }
      keys[tid] = key;
      nxt.aux[tid] = 0;
    }
    for (int m = tid; m < next; m += BEAM_THREADS) {
      const int r = m / n, i = m - r * n;
      const int c = __builtin_bit_cast(int, ft[r]);
      const float v = ft[K + r] + (c == cur.last[i] ? cur.lb[i] : cur.tot[i]);
      bool skip = false;
#pragma unroll 8
      for (int k = 0; k < n; k++) skip |= (cur.ppos[k] == i) & (cur.last[k] == c);   // (no short circuit: independent reads)
      float s = v;
      if constexpr (LEX) {
        skip |= !(ent_allow[i * W + (c >> 5)] >> (c & 31) & 1u);   // not allowed: no candidate
        s = v + (clm[i] + beam_lm_term(a.weight, a.table ? a.table[(size_t)cctx[i] * nc + c] : 0.0f, a.bonus));
      } else if constexpr (LM) s = v + (clm[i] + beam_lm_term(a.weight, a.table[(size_t)cctx[i] * nc + c], a.bonus));
      keys[beam + m] = skip ? 0ull : beam_key(s, (unsigned)(beam + i * nc + c));
    }
    __syncthreads();
    // ---- B: rank by counting.  First against the front of the list; who may still be in goes to the survivors ----
    const int front = ncand < 64 ? ncand : 64;
    for (int m = tid; m < ncand; m += BEAM_THREADS) {
      const unsigned long long key = keys[m];
      if (key == 0ull) continue;
      int rank = 0;
      for (int q0 = 0; q0 < front && rank < beam; q0 += 16) {   // sixteen independent reads per look at the count
        unsigned long long kq[16];
#pragma unroll
        for (int u = 0; u < 16; u++) kq[u] = keys[q0 + u < front ? q0 + u : m];
#pragma unroll
        for (int u = 0; u < 16; u++) rank += kq[u] > key ? 1 : 0;
      }
      if (rank < beam) surv[atomic_fetch_add_i32(misc + 2, 1)] = key;   // (their order is free: ranks are counted)
    }
    __syncthreads();
    // ---- then among the survivors; rank r < beam: entry r of the next frame ----
    const int ns = misc[2];
    for (int m = tid; m < ns; m += BEAM_THREADS) {
      const unsigned long long key = surv[m];
      int rank = 0;
      for (int q0 = 0; q0 < ns && rank < beam; q0 += 16) {
        unsigned long long kq[16];
#pragma unroll
        for (int u = 0; u < 16; u++) kq[u] = surv[q0 + u < ns ? q0 + u : m];
#pragma unroll
        for (int u = 0; u < 16; u++) rank += kq[u] > key ? 1 : 0;
      }
      if (rank >= beam) continue;
      const int index = (int)~(unsigned)key;
      const float v = beam_unord((unsigned)(key >> 32));
      if (index < beam) {
        const int i = index;
        nxt.node[rank] = cur.node[i]; nxt.last[rank] = cur.last[i];
        nxt.lb[rank] = stay_lb[i]; nxt.lnb[rank] = stay_lnb[i];
        if constexpr (LM) nxt.tot[rank] = stay_tot[i];
        else nxt.tot[rank] = v;
        nxt.aux[rank] = 1;
      } else {
        const int i = (index - beam) / nc, c = (index - beam) - i * nc;
        nxt.node[rank] = -1; nxt.last[rank] = c;
        float va = v;
        if constexpr (LM) va = row[c] + (c == cur.last[i] ? cur.lb[i] : cur.tot[i]);   // (the key holds va + lm: the acoustic value again)
        nxt.lb[rank] = beam_neg_inf(); nxt.lnb[rank] = va; nxt.tot[rank] = va;
        nxt.aux[rank] = 2 + cur.node[i];   // the parent's node
      }
    }
    __syncthreads();
    // ---- C: wave 0 names the new entries' nodes; the other waves stage the next frame's class list ----
    if constexpr (LM) { if (tid >= 64 && t + 1 < T) for (int j = tid - 64; j <= K; j += BEAM_THREADS - 64) stage_frame(t + 1, j); }
    else if (tid >= 64 && t + 1 < T && tid - 64 <= K) stage_frame(t + 1, tid - 64);
    if (wave == 0) {
      const int w = lane < beam ? lane : 0;
      const int aux = lane < beam ? nxt.aux[w] : 0;
      const int nn = __builtin_popcountll(wave_ballot(aux != 0));   // ranks are dense: entries 0 .. nn-1 are written
      const bool ext = aux >= 2;
      const int pn = aux - 2, c = nxt.last[w];
      int nd = ext ? 0 : nxt.node[w];
      unsigned slot = 0;
      if (ext) {
        slot = beam_hash(pn, c) & (unsigned)hmask;
        for (int probe = 0; probe <= hmask; probe++) {
          const int id = load_i32_wt(tab + slot);
          if (id == 0) break;
          if (load_i32_wt(npar + id) == pn && load_i32_wt(nlab + id) == c) { nd = id; break; }
          slot = (slot + 1) & (unsigned)hmask;
        }
      }
      unsigned long long todo = wave_ballot(ext && nd == 0);
      while (todo) {   // wave-uniform: one new node at a time
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        if (lane == l) {
          for (int probe = 0; probe <= hmask && load_i32_wt(tab + slot) != 0; probe++) slot = (slot + 1) & (unsigned)hmask;
          nd = misc[0];
          misc[0] = nd + 1;
          store_i32_wt(npar + nd, pn); store_i32_wt(nlab + nd, c); store_i32_wt(ndep + nd, load_i32_wt(ndep + pn) + 1);
          if constexpr (LM) {   // the prefix's LM value and context, once
            const int pctx = load_i32_wt(nctx + pn);
            const float plm = __builtin_bit_cast(float, load_i32_wt(nlm + pn));
            float x = 0.0f;
            if constexpr (LEX) { if (a.table) x = a.table[(size_t)pctx * nc + c]; }
            else x = a.table[(size_t)pctx * nc + c];
            const float lmv = plm + beam_lm_term(a.weight, x, a.bonus);
            store_i32_wt(nlm + nd, __builtin_bit_cast(int, lmv));
            store_i32_wt(nctx + nd, a.order == 3 ? nc * load_i32_wt(nlab + pn) + c : c);
          }
          if constexpr (LEX) {   // the prefix's lexicon state, once: the child of the parent's state by c; no such child: a separator
            const int px = load_i32_wt(nlex + pn);
            int lo = lex_off[px], hi = lex_off[px + 1], x = 0;
            for (int it = 0; it < 32 && lo < hi; it++) {   // (binary search: at most log2 of the child count rounds)
              const int mid = lo + ((hi - lo) >> 1), lc = lex_lab[mid];
              if (lc == c) { x = lex_tgt[mid]; break; }
              if (lc < c) lo = mid + 1; else hi = mid;
            }
            store_i32_wt(nlex + nd, x);
          }
          store_i32_wt(tab + slot, nd);
        }
        drain_vmem();
        wave_lds_fence();
      }
      if (lane < nn) nxt.node[lane] = nd;
      if constexpr (LM) {
        if (lane < nn) {
          ent_ctx[((t + 1) & 1) * BEAM_MAX + lane] = load_i32_wt(nctx + nd);
          ent_lm[((t + 1) & 1) * BEAM_MAX + lane] = __builtin_bit_cast(float, load_i32_wt(nlm + nd));
        }
      }
      wave_lds_fence();
      if constexpr (LEX) {   // the new entries' rows of allowed classes, all lanes: word j of entry i
        for (int q = lane; q < nn * W; q += 64) {
          const int i = q / W, j = q - i * W;
          ent_allow[q] = lex_allow[(size_t)load_i32_wt(nlex + nxt.node[i]) * W + j];
        }
      }
      if (lane < nn) {
        const int par = nd == 0 ? -1 : load_i32_wt(npar + nd);
        int pp = -1;
        for (int j = 0; j < nn; j++) pp = nxt.node[j] == par ? j : pp;
        nxt.ppos[lane] = pp;
      }
      if (lane == 0) { misc[1] = nn; misc[2] = 0; }
    }
    __syncthreads();
    n = misc[1];
  }

  // ---- results: the first nbest entries, labels by the walk to the root ----
  const BeamEnt fin = beam_ent(lds + L.ent, T & 1);
  int nh = n < a.nbest ? n : a.nbest;
  if constexpr (!LEX) { if (tid == 0) a.nhyp[ln.line] = nh; }
  if constexpr (LM) {   // the live entries ranked by their total; entry ent_ctx[r] of the beam leaves as hypothesis r
    const float* const flm = ent_lm + (T & 1) * BEAM_MAX;
    int* const fctx = ent_ctx + (T & 1) * BEAM_MAX;
    unsigned long long key = 0ull;
    if (tid < n) {
      float total = fin.tot[tid] + flm[tid];
      if (a.end) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
        const float e = a.weight * a.end[fctx[tid]];
        total = total + e;
      }
      stay_tot[tid] = total;
      key = ((unsigned long long)beam_ord(total) << 32) | (unsigned)~(unsigned)tid;   // (never 0: beam_ord(-inf) is not)
      if constexpr (LEX) { if (!(ent_allow[tid * W] & 1u)) key = 0ull; }   // a word left unfinished: not ranked
      keys[tid] = key;
    }
    __syncthreads();
    if constexpr (LEX) {
      int adm = 0;
      for (int q = 0; q < n; q++) adm += keys[q] != 0ull ? 1 : 0;
      nh = adm < a.nbest ? adm : a.nbest;
      if (tid == 0) a.nhyp[ln.line] = nh;
    }
    if (tid < n && (!LEX || key != 0ull)) {
      int rank = 0;
      for (int q = 0; q < n; q++) rank += keys[q] > key ? 1 : 0;
      fctx[rank] = tid;
    }
    __syncthreads();
  }
  if (tid < a.nbest) {
    const int k = tid, slot = ln.line * a.nbest + k;
    int len = 0;
    float sc = beam_neg_inf(), am = beam_neg_inf();
    if (k < nh) {
      int src = k;
      if constexpr (LM) src = ent_ctx[(T & 1) * BEAM_MAX + k];
      int nd = fin.node[src];
      len = load_i32_wt(ndep + nd);
      len = len > T ? T : len;
      sc = fin.tot[src];
      if constexpr (LM) { am = sc; sc = stay_tot[src]; }
      if (a.labels) {
        int* out = a.labels + (size_t)a.nbest * ln.row + (size_t)k * T;
        for (int d = len - 1; d >= 0 && nd > 0; d--) {
          out[d] = load_i32_wt(nlab + nd);
          nd = load_i32_wt(npar + nd);
        }
      }
    }
    if (a.len) a.len[slot] = len;
    a.score[slot] = sc;
    if constexpr (LM) { if (a.am_score) a.am_score[slot] = am; }
  }
}

}  // namespace clstm
