// charlm.h -- character n-gram language models for the beam search (clstm_ctc_beam_lm_batch / clstm_net_beam_lm): the estimator
// and the file format of clstm_amd/lm.py in C++; the two write the same bytes for the same input.  Host arithmetic only: nothing
// here touches the device (CLSTMOCR::set_lm hands the tables to clstm_charlm_create).
//
// A model is a dense float32 table lm[ctx][c] of order 2 or 3 -- nc^(order-1) rows of nc columns, labels 1 .. nc-1, 0 = "no label
// yet"; order 2: ctx = the last label, order 3: ctx = nc * (the label before last) + the last label -- and an optional end table
// end[ctx].  File (little endian): 8 bytes magic "CLSTMLM1", int32 order, int32 nc, int32 end flag (0 | 1), nc^order float32 of the
// table row by row, then nc^(order-1) float32 of the end table when the flag is 1.
#pragma once
#include <stdint.h>

#include <cmath>

#include "hostutil.h"

namespace clstmhost {

struct CharLMTables {
  int order = 0, nc = 0;
  bool has_end = false;
  vector<float> table, end;
  static constexpr long long MAX_FLOATS = 1ll << 26;

  long long nctx() const { return order == 3 ? (long long)nc * nc : nc; }
  static bool shape_ok(long long order, long long nc) {
    if ((order != 2 && order != 3) || nc < 2 || nc > MAX_FLOATS) return false;
    long long n = nc * nc;                       // (nc <= 2^26: no overflow)
    if (order == 3) { if (n > MAX_FLOATS) return false; n *= nc; }
    return n <= MAX_FLOATS;
  }
  // ctx of a prefix whose last two labels are `before` and `last` (0 where there is none)
  int context(int before, int last) const { return order == 2 ? last : nc * before + last; }

  // add-k smoothed log relative frequencies.  The events of a context are the nc - 1 labels and the line end: lm[ctx][c] =
  // log((count[ctx][c] + k) / (total[ctx] + k nc)), end[ctx] the same with the count of lines that ended in ctx, total[ctx] = all of
  // them; column 0 is 0.  Quotient and logarithm in double, rounded to float once.  Start contexts are padded with 0.
  static CharLMTables estimate(const vector<vector<int>>& sequences, int nc, int order, double add_k) {
    if (!(add_k > 0.0) || !std::isfinite(add_k)) fail("charlm: add_k must be positive and finite");
    if (!shape_ok(order, nc)) fail("charlm: order must be 2 or 3, nc at least 2, the table at most 2^26 floats");
    CharLMTables m;
    m.order = order; m.nc = nc; m.has_end = true;
    const size_t nctx = (size_t)m.nctx();
    vector<long long> cnt(nctx * nc, 0), endc(nctx, 0);
    for (const vector<int>& seq : sequences) {
      int before = 0, last = 0;
      for (int c : seq) {
        if (c < 1 || c >= nc) fail("charlm: a label lies outside 1 .. nc-1");
        cnt[(size_t)m.context(before, last) * nc + c]++;
        before = last; last = c;
      }
      endc[m.context(before, last)]++;
    }
    m.table.assign(nctx * nc, 0.0f);
    m.end.assign(nctx, 0.0f);
    for (size_t x = 0; x < nctx; x++) {
      long long total = endc[x];
      for (int c = 0; c < nc; c++) total += cnt[x * nc + c];
      const double den = (double)total + add_k * (double)nc;
      for (int c = 1; c < nc; c++) m.table[x * nc + c] = (float)log(((double)cnt[x * nc + c] + add_k) / den);
      m.end[x] = (float)log(((double)endc[x] + add_k) / den);
    }
    return m;
  }

  string tobytes() const {
    string out("CLSTMLM1");
    const int32_t head[3] = {order, nc, has_end ? 1 : 0};
    out.append(reinterpret_cast<const char*>(head), sizeof head);
    out.append(reinterpret_cast<const char*>(table.data()), table.size() * sizeof(float));
    if (has_end) out.append(reinterpret_cast<const char*>(end.data()), end.size() * sizeof(float));
    return out;
  }
  void save(const string& fname) const {
    std::ofstream stream(fname, std::ios::binary);
    const string bytes = tobytes();
    stream.write(bytes.data(), (std::streamsize)bytes.size());
    stream.close();
    if (!stream) fail("cannot write: " + fname);
  }
  // a file that is not exactly a header and the tables it announces is refused: bad magic, a header outside the limits, truncated,
  // bytes after the tables, a non-finite entry.  Nothing is allocated before the header has been checked.
  static CharLMTables load(const string& fname) {
    std::ifstream stream(fname, std::ios::binary);
    if (!stream) fail("cannot open: " + fname);
    char head[20];
    stream.read(head, sizeof head);
    if (stream.gcount() != (std::streamsize)sizeof head || memcmp(head, "CLSTMLM1", 8) != 0) fail(fname + ": not a CLSTMLM1 file");
    int32_t h[3];
    memcpy(h, head + 8, sizeof h);
    if (!shape_ok(h[0], h[1]) || (h[2] != 0 && h[2] != 1)) fail(fname + ": bad header");
    CharLMTables m;
    m.order = h[0]; m.nc = h[1]; m.has_end = h[2] == 1;
    const size_t nctx = (size_t)m.nctx(), ntab = nctx * m.nc, nend = m.has_end ? nctx : 0;
    stream.seekg(0, std::ios::end);
    const long long size = (long long)stream.tellg();
    const long long want = (long long)sizeof head + (long long)(ntab + nend) * (long long)sizeof(float);
    if (size < want) fail(fname + ": truncated");
    if (size > want) fail(fname + ": bytes after the tables");
    stream.seekg(sizeof head, std::ios::beg);
    m.table.resize(ntab);
    m.end.resize(nend);
    stream.read(reinterpret_cast<char*>(m.table.data()), (std::streamsize)(ntab * sizeof(float)));
    if (nend) stream.read(reinterpret_cast<char*>(m.end.data()), (std::streamsize)(nend * sizeof(float)));
    if (!stream) fail(fname + ": truncated");
    for (float v : m.table) if (!std::isfinite(v)) fail(fname + ": a table entry is not finite");
    for (float v : m.end) if (!std::isfinite(v)) fail(fname + ": a table entry is not finite");
    return m;
  }
};

}  // namespace clstmhost
