// lexicon_check -- a stand-alone program over lexicon.h (the word-list loader) and ../csrc/lexicon_trie.h (the trie builder of
// clstm_lexicon_create and the walk of clstm_lexicon_admits) alone: no library, no device.  `make check-lexicon` builds it with
// -fsanitize=address,undefined and runs it; exit status 0 = every check held.
#include <set>

#include "../csrc/lexicon_trie.h"
#include "lexicon.h"
using namespace clstmhost;

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { failures++; std::cerr << "FAILED line " << __LINE__ << ": " #cond << std::endl; } \
  } while (0)

static void write_bytes(const string& fname, const string& bytes) {
  std::ofstream f(fname, std::ios::binary);
  f.write(bytes.data(), (std::streamsize)bytes.size());
}
static bool refused(int nc, const vector<unsigned char>& wc, const vector<vector<int>>& words, const char* why) {
  vector<int> flat, off(1, 0);
  for (const auto& w : words) { flat.insert(flat.end(), w.begin(), w.end()); off.push_back((int)flat.size()); }
  flat.push_back(0);
  clstm::LexiconTrie t;
  try {
    clstm::build_lexicon(t, nc, wc.data(), flat.data(), off.data(), (int)words.size());
  } catch (const std::runtime_error& e) {
    return strstr(e.what(), why) != nullptr;
  }
  return false;
}
// a small generator of its own (no <random>: the same numbers everywhere)
struct Lcg {
  unsigned long long s;
  unsigned next(unsigned n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((s >> 33) % n); }
};

int main(int argc, char** argv) {
  if (argc != 2) { std::cerr << "usage: lexicon_check SCRATCH-DIRECTORY\n"; return 2; }
  const string dir = argv[1], f = dir + "/check.words";
  // the codec: a b c t - and e-acute, classes 1 .. 6; class 0 is blank
  std::map<int, int> enc = {{'a', 1}, {'b', 2}, {'c', 3}, {'t', 4}, {'-', 5}, {0xe9, 6}, {0, 0}};
  const int nc = 7;
  // ---- the loader ----
  {
    write_bytes(f, "");
    const WordList w = WordList::load(f, enc, nc);
    CHECK(w.words.empty() && w.lines == 0 && w.dropped() == 0 && w.word_class == vector<unsigned char>(nc, 0));
  }
  {
    write_bytes(f, "\n\n  \r\n");
    CHECK(WordList::load(f, enc, nc).words.empty() && WordList::load(f, enc, nc).lines == 0);
  }
  {   // CRLF, blanks around a word, a duplicate, no newline at the end, two bytes of UTF-8
    write_bytes(f, "cat\r\n  tab\t\r\ncat\ncat\xc3\xa9");
    const WordList w = WordList::load(f, enc, nc);
    CHECK(w.lines == 4 && w.dropped() == 0 && w.words.size() == 4);
    CHECK(w.words[0] == vector<int>({3, 1, 4}) && w.words[1] == vector<int>({4, 1, 2}) && w.words[2] == w.words[0]);
    CHECK(w.words[3].size() == 4 && w.words[3][3] == 6);   // c a t e-acute: the two bytes are one character
    CHECK(w.word_class == vector<unsigned char>({0, 1, 1, 1, 1, 0, 1}));   // '-' occurs in no word: a separator
  }
  {   // invalid UTF-8: a lone continuation byte, a truncated sequence, an overlong form, a surrogate, above U+10FFFF
    write_bytes(f, "a\x80" "b\ncat\nab\xc3\n\xc0\xaf\n\xed\xa0\x80\n\xf4\x90\x80\x80\nab\n");
    const WordList w = WordList::load(f, enc, nc);
    CHECK(w.lines == 7 && w.bad_utf8 == 5 && w.words.size() == 2 && w.words[1] == vector<int>({1, 2}));
  }
  {   // an over-long word (257 code points) beside the longest admitted one
    write_bytes(f, string(257, 'a') + "\n" + string(256, 'b') + "\n");
    const WordList w = WordList::load(f, enc, nc);
    CHECK(w.too_long == 1 && w.words.size() == 1 && w.words[0].size() == 256 && w.words[0][0] == 2);
  }
  {   // only out-of-codec words: nothing kept, no word classes, and the trie of it admits only separators
    write_bytes(f, "dog\nxyz\ncow\n");
    const WordList w = WordList::load(f, enc, nc);
    CHECK(w.outside_codec == 3 && w.words.empty() && w.word_class == vector<unsigned char>(nc, 0));
    vector<int> flat, off;
    w.pack(flat, off);
    clstm::LexiconTrie t;
    clstm::build_lexicon(t, nc, w.word_class.data(), flat.data(), off.data(), 0);
    const int l[3] = {1, 5, 3};
    CHECK(t.nnodes == 1 && t.nedges == 0 && t.nwords == 0 && clstm::lexicon_admits(t, l, 3) == 2 && clstm::lexicon_admits(t, l, 0) == 2);
  }
  {   // word_chars: the named set; a word with a character outside it is dropped
    write_bytes(f, "cat\nc-t\nab\n");
    const string set = "abct\xc3\xa9";
    const WordList w = WordList::load(f, enc, nc, &set);
    CHECK(w.words.size() == 2 && w.outside_word_chars == 1 && w.word_class == vector<unsigned char>({0, 1, 1, 1, 1, 0, 1}));
    const string bad = "ab\xff";
    bool threw = false;
    try { WordList::load(f, enc, nc, &bad); } catch (const HostError&) { threw = true; }
    CHECK(threw);
  }
  {
    bool threw = false;
    try { WordList::load(dir + "/no such file", enc, nc); } catch (const HostError&) { threw = true; }
    CHECK(threw);
  }
  remove(f.c_str());
  // ---- the trie builder's refusals ----
  const vector<unsigned char> wc = {0, 1, 1, 1, 0, 0};
  CHECK(refused(6, {1, 1, 1, 1, 0, 0}, {{1}}, "class 0 (blank) cannot be a word class"));
  CHECK(refused(6, wc, {{1}, {2, 6}}, "word 1 holds a label outside 1 .. nc-1") && refused(6, wc, {{0}}, "word 0 holds a label outside"));
  CHECK(refused(6, wc, {{-3}}, "outside") && refused(6, wc, {{1, 4}}, "word 0 holds a label that is not a word class"));
  CHECK(refused(6, wc, {{1}, {}, {2}}, "word 1 is empty") && refused(1, {0}, {}, "class count"));
  CHECK(refused(1 << 16, vector<unsigned char>(1 << 16, 0), {}, "") == false);   // nc = 65536 without words: 2048 words of one row, legal
  // ---- admits against a brute-force set: 300 random words over classes 1 .. 3 (4, 5 separators), every sequence up to length 6 ----
  {
    Lcg rng{12345};
    vector<vector<int>> words;
    for (int k = 0; k < 300; k++) {
      vector<int> w(1 + rng.next(5));
      for (int& c : w) c = 1 + (int)rng.next(3);
      words.push_back(w);
    }
    std::set<vector<int>> have(words.begin(), words.end()), prefixes;
    for (const auto& w : have) for (size_t k = 0; k <= w.size(); k++) prefixes.insert(vector<int>(w.begin(), w.begin() + k));
    prefixes.insert(vector<int>());
    vector<int> flat, off(1, 0);
    for (const auto& w : words) { flat.insert(flat.end(), w.begin(), w.end()); off.push_back((int)flat.size()); }
    clstm::LexiconTrie t, t2;
    clstm::build_lexicon(t, 6, wc.data(), flat.data(), off.data(), (int)words.size());
    CHECK(t.nwords == (long long)have.size() && t.nnodes == (long long)prefixes.size() && t.nedges == t.nnodes - 1);
    CHECK((long long)t.words.size() == 4 + t.nnodes * 1 + t.nnodes + 1 + 2 * t.nedges);
    // deterministic: the same words in another order give the same arrays
    vector<int> rflat, roff(1, 0);
    for (size_t k = words.size(); k-- > 0;) { rflat.insert(rflat.end(), words[k].begin(), words[k].end()); roff.push_back((int)rflat.size()); }
    clstm::build_lexicon(t2, 6, wc.data(), rflat.data(), roff.data(), (int)words.size());
    CHECK(t2.words == t.words);
    for (long long x = 0; x < t.nnodes; x++)   // the children of a node sorted by label
      for (int e = t.off()[x] + 1; e < t.off()[x + 1]; e++) CHECK(t.lab()[e - 1] < t.lab()[e]);
    auto brute = [&](const vector<int>& l) {
      vector<int> run;
      for (int c : l) {
        if (c < 1 || c >= 6) return 0;
        if (wc[c]) { run.push_back(c); if (!prefixes.count(run)) return 0; }
        else { if (!run.empty() && !have.count(run)) return 0; run.clear(); }
      }
      return run.empty() || have.count(run) ? 2 : 1;
    };
    int seen[3] = {0, 0, 0};
    vector<int> l;
    for (int len = 0; len <= 6; len++) {
      long long total = 1;
      for (int k = 0; k < len; k++) total *= 5;
      for (long long code = 0; code < total; code++) {
        l.assign(len, 0);
        long long q = code;
        for (int k = 0; k < len; k++) { l[k] = 1 + (int)(q % 5); q /= 5; }
        const int want = brute(l), got = clstm::lexicon_admits(t, l.data(), len);
        seen[want]++;
        if (want != got) { CHECK(want == got); break; }
      }
    }
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0);
    const int out_of_range[2] = {1, 6};
    CHECK(clstm::lexicon_admits(t, out_of_range, 2) == 0);
  }
  if (failures) { std::cerr << failures << " checks FAILED" << std::endl; return 1; }
  std::cout << "lexicon_check: ok" << std::endl;
  return 0;
}
