// lexicon_trie.h -- the lexicon of the beam search (ctc_beam.h, third part) on the host: checks, the trie builder, the device form and
// the walk of clstm_lexicon_admits.  Plain C++, no device code and no runtime: clstm_hip.hip includes it for clstm_lexicon_create, and
// clstm_amd/host/lexicon_check.cc compiles it alone under the sanitizers.  A refusal throws std::runtime_error with the entry's name.
//
// `words` is the device form word for word -- [nodes, edges, W = ceil(nc / 32), 0 | allow [nodes][W] | off [nodes + 1] | lab [edges] |
// tgt [edges]], bit c of a node's row: class c may follow, bit 0: "root or terminal" -- and clstm_lexicon_admits walks exactly it.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace clstm {

#define LEX_REQUIRE(cond, msg)                                \
  do {                                                        \
    if (!(cond)) throw std::runtime_error(std::string(msg)); \
  } while (0)

constexpr long long LEX_MAX_NODES = 1ll << 24;    // trie nodes, the root included
constexpr long long LEX_MAX_BYTES = 1ll << 28;    // the device form
struct LexiconTrie {
  int nc = 0, W = 0;
  long long nwords = 0, nnodes = 0, nedges = 0;   // distinct words, nodes, edges
  std::vector<int> words;                         // [nodes, edges, W, 0 | allow [nodes][W] | off [nodes + 1] | lab [edges] | tgt [edges]]
  const unsigned* allow() const { return reinterpret_cast<const unsigned*>(words.data() + 4); }
  const int* off() const { return words.data() + 4 + nnodes * W; }
  const int* lab() const { return off() + nnodes + 1; }
  const int* tgt() const { return lab() + nedges; }
  // the state after c in state x (c allowed there): the child by c, or the root for a separator
  int next(int x, int c) const {
    const int* l0 = lab() + off()[x], * l1 = lab() + off()[x + 1];
    const int* it = std::lower_bound(l0, l1, c);
    return it != l1 && *it == c ? tgt()[it - lab()] : 0;
  }
};
// Everything is checked before anything is uploaded; the trie is deterministic: the words sorted, duplicates merged, so the children
// of a node are made in the order of their labels and the nodes are numbered in the order of the sorted words' first visit.
inline void build_lexicon(LexiconTrie& lx, int nc, const unsigned char* word_class_h, const int* words_h, const int* word_off_h, int nwords) {
  LEX_REQUIRE(nc >= 2 && nc < (1 << 26), "clstm_lexicon_create: the class count must lie in [2, 2^26)");
  LEX_REQUIRE(word_class_h, "clstm_lexicon_create: word_class_h is required");
  LEX_REQUIRE(word_class_h[0] == 0, "clstm_lexicon_create: class 0 (blank) cannot be a word class");
  LEX_REQUIRE(nwords >= 0, "clstm_lexicon_create: the word count is negative");
  LEX_REQUIRE(nwords == 0 || (words_h && word_off_h), "clstm_lexicon_create: words_h and word_off_h are required");
  LEX_REQUIRE(nwords == 0 || word_off_h[0] >= 0, "clstm_lexicon_create: bad word offsets");
  for (int w = 0; w < nwords; w++) {
    const long long len = (long long)word_off_h[w + 1] - word_off_h[w];
    LEX_REQUIRE(len >= 0, "clstm_lexicon_create: bad word offsets");
    LEX_REQUIRE(len > 0, "clstm_lexicon_create: word " + std::to_string(w) + " is empty");
    for (int k = word_off_h[w]; k < word_off_h[w + 1]; k++) {
      const int c = words_h[k];
      LEX_REQUIRE(c >= 1 && c < nc, "clstm_lexicon_create: word " + std::to_string(w) + " holds a label outside 1 .. nc-1");
      LEX_REQUIRE(word_class_h[c] != 0, "clstm_lexicon_create: word " + std::to_string(w) + " holds a label that is not a word class");
    }
  }
  const long long total = nwords ? (long long)word_off_h[nwords] - word_off_h[0] : 0;
  LEX_REQUIRE(total < LEX_MAX_NODES, "clstm_lexicon_create: the words need more than 2^24 trie nodes");   // (nodes <= 1 + labels)
  std::vector<int> order(nwords);
  for (int w = 0; w < nwords; w++) order[w] = w;
  auto span = [&](int w) { return std::make_pair(words_h + word_off_h[w], words_h + word_off_h[w + 1]); };
  std::sort(order.begin(), order.end(), [&](int x, int y) {
    const auto a = span(x), b = span(y);
    return std::lexicographical_compare(a.first, a.second, b.first, b.second);
  });
  // sorted insertion: the child of a node by c exists iff it is the child that node got last
  std::vector<int> epar, elab, last_child(1, -1), last_label(1, 0);
  std::vector<char> term(1, 0);
  long long distinct = 0;
  for (int w : order) {
    int x = 0;
    const auto sp = span(w);
    for (const int* q = sp.first; q != sp.second; q++) {
      if (last_child[x] >= 0 && last_label[x] == *q) { x = last_child[x]; continue; }
      const int nd = (int)term.size();
      epar.push_back(x); elab.push_back(*q);   // (edge e leads to node e + 1)
      last_child[x] = nd; last_label[x] = *q;
      last_child.push_back(-1); last_label.push_back(0); term.push_back(0);
      x = nd;
    }
    distinct += term[x] ? 0 : 1;
    term[x] = 1;
  }
  const long long nn = (long long)term.size(), ne = (long long)epar.size();
  const int W = (nc + 31) >> 5;
  const long long nwordsdev = 4 + nn * W + (nn + 1) + 2 * ne;
  LEX_REQUIRE(nn <= LEX_MAX_NODES, "clstm_lexicon_create: the words need more than 2^24 trie nodes");
  LEX_REQUIRE(nwordsdev * 4 <= LEX_MAX_BYTES, "clstm_lexicon_create: the device form exceeds 2^28 bytes (nodes * ceil(nc / 32) words of allowed classes)");
  lx.nc = nc; lx.W = W; lx.nwords = distinct; lx.nnodes = nn; lx.nedges = ne;
  lx.words.assign((size_t)nwordsdev, 0);
  int* const d = lx.words.data();
  d[0] = (int)nn; d[1] = (int)ne; d[2] = W;
  unsigned* const allow = reinterpret_cast<unsigned*>(d + 4);
  int* const off = d + 4 + nn * W;
  int* const lab = off + nn + 1;
  int* const tgt = lab + ne;
  std::vector<unsigned> sep((size_t)W, 0u);   // the separators, and bit 0: "root or terminal"
  sep[0] = 1u;
  for (int c = 1; c < nc; c++) if (!word_class_h[c]) sep[c >> 5] |= 1u << (c & 31);
  term[0] = 1;   // (for the rows only: the root takes separators as a terminal node does)
  for (long long x = 0; x < nn; x++) if (term[x]) for (int j = 0; j < W; j++) allow[x * W + j] = sep[j];
  for (long long e = 0; e < ne; e++) { off[epar[e] + 1]++; allow[(long long)epar[e] * W + (elab[e] >> 5)] |= 1u << (elab[e] & 31); }
  for (long long x = 0; x < nn; x++) off[x + 1] += off[x];
  std::vector<int> fill(off, off + nn);
  for (long long e = 0; e < ne; e++) {   // (edges of one parent come in the order of their labels)
    const int at = fill[epar[e]]++;
    lab[at] = elab[e]; tgt[at] = (int)e + 1;
  }
}
// 0: not an admissible prefix; 1: an admissible prefix whose last run is unfinished; 2: an admissible labelling
inline int lexicon_admits(const LexiconTrie& lx, const int* labels_h, int L) {
  int x = 0;
  for (int k = 0; k < L; k++) {
    const int c = labels_h[k];
    if (c < 1 || c >= lx.nc) return 0;
    if (!(lx.allow()[(size_t)x * lx.W + (c >> 5)] >> (c & 31) & 1u)) return 0;
    x = lx.next(x, c);
  }
  return (lx.allow()[(size_t)x * lx.W] & 1u) ? 2 : 1;
}

#undef LEX_REQUIRE

}  // namespace clstm
