// lexicon.h -- word lists for the lexicon-constrained beam search (clstm_ctc_beam_lex_batch / clstm_net_beam_lex): the loader of
// clstm_amd/lexicon.py in C++; the two derive the same words and word classes from the same file.  Host code only: nothing here touches
// the device (CLSTMOCR::set_lexicon hands the result to clstm_lexicon_create, which builds the trie).
//
// A word list is a UTF-8 text file, one word per line.  Line ends are LF or CRLF; blanks and tabs around a word are dropped; empty
// lines are skipped.  Each word is encoded through the model's codec (code point -> class).  Dropped and counted, never an error: a
// line that is not valid UTF-8 (strictly: no overlong forms, no surrogates, nothing above U+10FFFF), a word longer than
// MAX_WORD code points, a word with a character the codec lacks (or that maps to class 0).  Word classes: by default a class is a
// word character iff it occurs in a kept word; word_chars=STRING names them instead, and a word with a character outside that set is
// dropped too (it could never be written).  Duplicates are kept here and merged by the trie builder.
#pragma once
#include <map>

#include "hostutil.h"

namespace clstmhost {

struct WordList {
  static constexpr size_t MAX_WORD = 256;   // code points
  vector<vector<int>> words;                // encoded, in file order
  vector<unsigned char> word_class;         // [nc]
  long long lines = 0, bad_utf8 = 0, too_long = 0, outside_codec = 0, outside_word_chars = 0;
  long long dropped() const { return bad_utf8 + too_long + outside_codec + outside_word_chars; }

  // strict UTF-8 -> code points; false when `s` is not valid
  static bool decode_utf8(const string& s, ustring& out) {
    out.clear();
    size_t i = 0;
    while (i < s.size()) {
      const unsigned c = (unsigned char)s[i];
      unsigned w, min;
      int more;
      if (c < 0x80) { w = c; more = 0; min = 0; }
      else if ((c & 0xe0) == 0xc0) { w = c & 0x1f; more = 1; min = 0x80; }
      else if ((c & 0xf0) == 0xe0) { w = c & 0x0f; more = 2; min = 0x800; }
      else if ((c & 0xf8) == 0xf0) { w = c & 0x07; more = 3; min = 0x10000; }
      else return false;
      if (i + more >= s.size()) return false;   // (the sequence runs past the end)
      for (int k = 1; k <= more; k++) {
        const unsigned d = (unsigned char)s[i + k];
        if ((d & 0xc0) != 0x80) return false;
        w = (w << 6) | (d & 0x3f);
      }
      if (w < min || w > 0x10ffff || (w >= 0xd800 && w <= 0xdfff)) return false;
      out.push_back((char32_t)w);
      i += 1 + more;
    }
    return true;
  }
  // the lines of `bytes` as words: split at LF, blanks / tabs / CR around a word dropped, empty lines skipped
  static vector<string> split_lines(const string& bytes) {
    vector<string> out;
    size_t at = 0;
    while (at <= bytes.size()) {
      size_t nl = bytes.find('\n', at);
      if (nl == string::npos) nl = bytes.size();
      size_t a = at, b = nl;
      while (a < b && (bytes[a] == ' ' || bytes[a] == '\t' || bytes[a] == '\r')) a++;
      while (b > a && (bytes[b - 1] == ' ' || bytes[b - 1] == '\t' || bytes[b - 1] == '\r')) b--;
      if (b > a) out.push_back(bytes.substr(a, b - a));
      at = nl + 1;
    }
    return out;
  }
  // encoder: code point -> class (the model's codec); nc classes; word_chars: null = the default rule
  static WordList parse(const string& bytes, const std::map<int, int>& encoder, int nc, const string* word_chars = nullptr) {
    if (nc < 2) fail("lexicon: the class count must be at least 2");
    WordList wl;
    wl.word_class.assign((size_t)nc, 0);
    auto encode = [&](char32_t ch) {
      auto it = encoder.find((int)ch);
      return it == encoder.end() || it->second < 1 || it->second >= nc ? -1 : it->second;
    };
    if (word_chars) {
      ustring wc;
      if (!decode_utf8(*word_chars, wc)) fail("lexicon: word_chars is not valid UTF-8");
      for (char32_t ch : wc) { const int c = encode(ch); if (c > 0) wl.word_class[c] = 1; }
    }
    ustring u;
    for (const string& line : split_lines(bytes)) {
      wl.lines++;
      if (!decode_utf8(line, u)) { wl.bad_utf8++; continue; }
      if (u.size() > MAX_WORD) { wl.too_long++; continue; }
      vector<int> w;
      bool ok = true, in_set = true;
      for (char32_t ch : u) {
        const int c = encode(ch);
        if (c < 0) { ok = false; break; }
        in_set = in_set && (!word_chars || wl.word_class[c]);
        w.push_back(c);
      }
      if (!ok) { wl.outside_codec++; continue; }
      if (!in_set) { wl.outside_word_chars++; continue; }
      wl.words.push_back(w);
    }
    if (!word_chars) for (const vector<int>& w : wl.words) for (int c : w) wl.word_class[c] = 1;
    return wl;
  }
  static WordList load(const string& fname, const std::map<int, int>& encoder, int nc, const string* word_chars = nullptr) {
    std::ifstream stream(fname, std::ios::binary);
    if (!stream) fail("cannot open: " + fname);
    const string bytes((std::istreambuf_iterator<char>(stream)), std::istreambuf_iterator<char>());
    return parse(bytes, encoder, nc, word_chars);
  }
  // packed for clstm_lexicon_create
  void pack(vector<int>& flat, vector<int>& off) const {
    flat.clear();
    off.assign(1, 0);
    for (const vector<int>& w : words) { flat.insert(flat.end(), w.begin(), w.end()); off.push_back((int)flat.size()); }
    if (flat.empty()) flat.push_back(0);
  }
};

}  // namespace clstmhost
