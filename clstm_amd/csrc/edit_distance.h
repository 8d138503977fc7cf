// edit_distance.h -- batched unit-cost Levenshtein distance with the canonical edit script (include/clstm_abi.h:
// clstm_edit_distance_batch, clstm_net_errors).  Integer arithmetic only.
//
// D[i][j], 0 <= i <= la (hypothesis h), 0 <= j <= lb (reference r): D[i][0] = i, D[0][j] = j,
//   D[i][j] = min(D[i-1][j-1] + (h[i-1] != r[j-1]), D[i-1][j] + 1, D[i][j-1] + 1);  the distance is D[la][lb] -- what the reference's
// levenshtein returns (clstm.h:329-351).
// The script is the canonical one: from (la, lb), at (i, j) go DIAGONAL if i, j > 0 and D[i-1][j-1] + (h[i-1] != r[j-1]) == D[i][j]
// (code 0 match / 1 substitution), else UP (i - 1) if i > 0 and D[i-1][j] + 1 == D[i][j] (code 2: an insertion, a hypothesis symbol with
// nothing in the reference), else LEFT (j - 1; code 3: a deletion, a reference symbol that was not output); reported in forward order.
//
// Shape of the work.  One wave per pair, EDIT_WAVES pairs per workgroup, no workgroup barrier anywhere.  The reference positions lie
// on the lanes in strips of 64 columns (lane l of strip k: column j = 64 k + l + 1) and a strip is walked by anti-diagonals: at
// step s lane l computes row i = s - l.  Its upper neighbour is its own value of the step before, its left neighbour lane l - 1's
// value of the step before (one wave_shr:1 DPP move), its diagonal neighbour that shifted value one step older.  The hypothesis
// symbol travels the same way: lane 0 takes h[s-1] at step s, lane l receives it l steps later by the same shift.  What lane 0
// takes -- the symbol, and from the second strip on the left strip's right-edge column D[s][64 k] -- is loaded 64 rows at a time, one
// per lane, and read out by a wave-uniform lane read: no memory access on the per-step chain.  A pair's serial chain is la + 63 steps
// per strip.  Lane 63 leaves its column to the next strip in the edge array, rewritten in place: the rows a strip still has to read
// lie ahead of the rows it writes.
// Directions (only when a script, counts or confusions are asked for): each cell's script code in 2 bits; a lane gathers 16 rows of
// its column in a register and stores one word per 16 steps: word (j - 1) * nw + (i - 1) / 16, bits 2 ((i - 1) % 16).  The back-trace
// is lane 0's walk of at most la + lb steps that reads nothing but those words and writes the codes backwards into the pair's slots;
// the wave then moves them to the front in chunks of 64, and from the codes of a chunk -- two ballots give every code its (i, j) --
// counts the three kinds and adds to the confusion table (ordinary atomics on int).
#pragma once
#include "devintrin.h"

constexpr int EDIT_WAVES = 4, EDIT_THREADS = 64 * EDIT_WAVES;
constexpr int EDIT_WAVE_WORDS = 4096;   // LDS carve of one wave: 16 KiB, a workgroup's 64 KiB need no opt-in
constexpr int EDIT_EDGE_LDS = 1024;     // rows of an edge column that may stay in LDS (the directions have the rest)

// ---- WHICH form a pair takes: the one statement of the rule.  The host sizes the launch's LDS and workspace with it, the wave of a
// pair addresses with it, clstm_debug_edit_plan answers with it (tests/test_edit_distance.py asserts the path it means to cover).
// la: the most hypothesis symbols the pair can have (clstm_net_errors: the line's frames; the length itself is on the device).
enum EditPlace { EDIT_NONE = 0, EDIT_LDS = 1, EDIT_WS = 2 };
struct EditPlan {
  int nstrips;             // strips of 64 reference columns (0: an empty reference, no table)
  int dirs, edge;          // EditPlace of the direction words / of the edge column between strips
  int nw;                  // direction words per column: ceil(la / 16), odd (columns a bank apart)
  int edge_words;          // la + 1 where an edge column exists
  long long dir_words;     // lb * nw where directions are kept
  int lds_words;           // of the wave's carve: [edge | directions], each only where it is EDIT_LDS
};
inline __host__ __device__ EditPlan edit_plan(int la, int lb, bool want_script) {
  EditPlan p{0, EDIT_NONE, EDIT_NONE, 0, 0, 0, 0};
  if (lb <= 0) return p;
  p.nstrips = (lb + 63) / 64;
  if (la <= 0) return p;
  if (p.nstrips > 1) {
    p.edge_words = la + 1;
    p.edge = p.edge_words <= EDIT_EDGE_LDS ? EDIT_LDS : EDIT_WS;
    if (p.edge == EDIT_LDS) p.lds_words = p.edge_words;
  }
  if (want_script) {
    p.nw = ((la + 15) / 16) | 1;
    p.dir_words = (long long)lb * p.nw;
    p.dirs = p.dir_words <= EDIT_WAVE_WORDS - p.lds_words ? EDIT_LDS : EDIT_WS;
    if (p.dirs == EDIT_LDS) p.lds_words += (int)p.dir_words;
  }
  return p;
}

struct EditPair {
  long long ws_dirs, ws_edge;   // first word in the workspace (where the plan says EDIT_WS)
  int hyp_off, la_cap;          // hypothesis: first symbol in EditArgs::hyp, the length the plan was made for
  int ref_off, lb;
  int ops_off;                  // first of the pair's la_cap + lb slots in EditArgs::ops
  int idx;                      // the caller's pair index: where the results go, and -- with hyp_len -- the hypothesis length
};
struct EditArgs {
  const EditPair* pairs;
  const int* hyp;
  const int* hyp_len;           // per pair index (clstm_net_errors: what decode_kernel counted); NULL: la = la_cap
  const int* ref;
  int* ws;
  int* dist;                    // [npairs]
  int* counts;                  // [npairs][3] substitutions, insertions, deletions
  int* nops;                    // [npairs]
  int* ops;                     // the scripts (also the back-trace's scratch: present whenever directions are kept)
  int* conf;                    // [nsym][nsym] or NULL
  int npairs, nsym, lds_wave_words;
};

DEVFN int edit_min(int a, int b) { return a < b ? a : b; }

template <bool SCRIPT>
__global__ void __launch_bounds__(EDIT_THREADS) edit_distance_kernel(EditArgs a) {
  const int lane = threadIdx.x & 63, wave = wave_uniform((int)(threadIdx.x >> 6));
  const int p = (int)blockIdx.x * EDIT_WAVES + wave;
  if (p >= a.npairs) return;
  const EditPair pr = a.pairs[p];
  int la = pr.la_cap;
  if (a.hyp_len) la = edit_min(a.hyp_len[pr.idx], pr.la_cap);
  la = wave_uniform(la < 0 ? 0 : la);
  const int lb = wave_uniform(pr.lb);
  const EditPlan pl = edit_plan(pr.la_cap, lb, SCRIPT);
  int* const lds = dyn_smem<int>() + (size_t)wave * a.lds_wave_words;
  int* const edge = pl.edge == EDIT_LDS ? lds : a.ws + pr.ws_edge;
  int* const dirs = pl.dirs == EDIT_LDS ? lds + (pl.edge == EDIT_LDS ? pl.edge_words : 0) : a.ws + pr.ws_dirs;
  const int* const h = a.hyp + pr.hyp_off;
  const int* const r = a.ref + pr.ref_off;

  int dist = la + lb;   // (an empty side: no table)
  if (la > 0 && lb > 0) {
    int prev = 0;
    for (int strip = 0; strip < pl.nstrips; strip++) {
      const int j = 64 * strip + lane + 1;
      const bool col = j <= lb;
      const int rj = col ? r[j - 1] : -1;
      const bool hand_on = strip + 1 < pl.nstrips && lane == 63;   // (then all 64 columns of the strip exist)
      const int nsteps = la + edit_min(64, lb - 64 * strip) - 1;
      prev = j;           // D[0][j]
      int diag = j - 1;   // D[0][j-1]
      int hs = 0, hch = 0, ech = 0, word = 0;
      for (int s = 1; s <= nsteps; s++) {
        const int k = (s - 1) & 63;
        if (k == 0) {   // what lane 0 takes during the next 64 steps: h[s-1 ..], D[s ..][64 strip]
          hch = s - 1 + lane < la ? h[s - 1 + lane] : 0;
          ech = strip > 0 && s + lane <= la ? edge[s + lane] : 0;
        }
        int left = wave_shr1_i(prev);
        hs = wave_shr1_i(hs);
        const int h0 = wave_readlane_i(hch, k), e0 = wave_readlane_i(ech, k);
        if (lane == 0) { hs = h0; left = strip == 0 ? s : e0; }
        const int i = s - lane;
        const int ne = hs != rj ? 1 : 0;
        const int sub = diag + ne, ins = prev + 1, del = left + 1;
        const int cur = edit_min(sub, edit_min(ins, del));
        diag = left;
        if (col && i >= 1 && i <= la) {
          prev = cur;
          if (SCRIPT) {
            const int code = sub == cur ? ne : ins == cur ? 2 : 3;
            word |= code << (2 * ((i - 1) & 15));
            if (((i - 1) & 15) == 15 || i == la) { dirs[(long long)(j - 1) * pl.nw + ((i - 1) >> 4)] = word; word = 0; }
          }
          if (hand_on) edge[i] = cur;
        }
      }
      wave_lds_fence();   // the edge column and the direction words: written by some lanes, read by others
      drain_vmem();
    }
    dist = wave_shfl_i(prev, (lb - 1) & 63);
  }
  if (lane == 0) a.dist[pr.idx] = dist;
  if (!SCRIPT) return;

  // ---- the back-trace: lane 0 walks, codes written backwards to the end of the pair's slots
  int* const ops = a.ops + pr.ops_off;
  int n = 0;
  if (lane == 0) {
    int i = la, j = lb, e = la + lb;
    while (i > 0 || j > 0) {
      int op;
      if (i == 0) op = 3;
      else if (j == 0) op = 2;
      else op = (dirs[(long long)(j - 1) * pl.nw + ((i - 1) >> 4)] >> (2 * ((i - 1) & 15))) & 3;
      ops[--e] = op;
      i -= op != 3;
      j -= op != 2;
    }
    n = la + lb - e;
  }
  drain_vmem();
  n = wave_shfl_i(n, 0);
  const int off = la + lb - n;
  int ci = 0, cj = 0, nsub = 0;   // symbols consumed before the chunk, substitutions so far
  for (int c = 0; c < n; c += 64) {
    const int k = c + lane;
    const bool v = k < n;
    const int op = v ? ops[off + k] : -1;
    const unsigned long long mh = wave_ballot(v && op != 3), mr = wave_ballot(v && op != 2), ms = wave_ballot(v && op == 1);
    const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
    if (v) {
      if (off > 0) ops[k] = op;   // (reads of later chunks lie beyond every slot written so far: off >= 0)
      if (a.conf) {
        const int hsym = op != 3 ? h[ci + __builtin_popcountll(mh & below)] : 0;
        const int rsym = op != 2 ? r[cj + __builtin_popcountll(mr & below)] : 0;
        atomic_add_i32(&a.conf[(size_t)rsym * a.nsym + hsym], 1);
      }
    }
    ci += __builtin_popcountll(mh);
    cj += __builtin_popcountll(mr);
    nsub += __builtin_popcountll(ms);
  }
  if (lane == 0) {
    a.nops[pr.idx] = n;
    a.counts[3 * (size_t)pr.idx] = nsub;
    a.counts[3 * (size_t)pr.idx + 1] = n - cj;   // codes that consumed no reference symbol
    a.counts[3 * (size_t)pr.idx + 2] = n - ci;   // codes that consumed no hypothesis symbol
  }
}
