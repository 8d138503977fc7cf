// charlm_check -- a stand-alone program over charlm.h alone (no library, no device): the loader on good, truncated, oversized
// and corrupt files, and the estimator against counts done by hand.  `make check-charlm` builds it with
// -fsanitize=address,undefined and runs it; exit status 0 = every check held.
#include "charlm.h"
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
static bool refused(const string& fname, const char* why) {
  try {
    CharLMTables::load(fname);
  } catch (const HostError& e) {
    return strstr(e.what(), why) != nullptr;
  }
  return false;
}
static string header(int32_t order, int32_t nc, int32_t flag) {
  string s("CLSTMLM1");
  const int32_t h[3] = {order, nc, flag};
  s.append(reinterpret_cast<const char*>(h), sizeof h);
  return s;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::cerr << "usage: charlm_check SCRATCH-DIRECTORY\n"; return 2; }
  const string dir = argv[1], f = dir + "/check.lm";
  // ---- the estimator: six lines over classes 1 .. 3, counted by hand ----
  const vector<vector<int>> corpus = {{1, 2}, {1, 2, 3}, {2}, {1, 1}, {}, {3, 1, 2}};
  const double k = 0.1;
  {
    const CharLMTables m = CharLMTables::estimate(corpus, 4, 2, k);
    CHECK(m.order == 2 && m.nc == 4 && m.has_end && m.table.size() == 16 && m.end.size() == 4);
    // context 0 (line start): 1 x3, 2 x1, 3 x1, end x1 (the empty line): total 6
    const double d0 = 6 + 4 * k;
    CHECK(m.table[0 * 4 + 1] == (float)log((3 + k) / d0) && m.table[0 * 4 + 2] == (float)log((1 + k) / d0));
    CHECK(m.table[0 * 4 + 3] == (float)log((1 + k) / d0) && m.end[0] == (float)log((1 + k) / d0));
    // context 1: -> 2 x3, -> 1 x1, end x1 (1 1): total 5
    const double d1 = 5 + 4 * k;
    CHECK(m.table[1 * 4 + 2] == (float)log((3 + k) / d1) && m.table[1 * 4 + 1] == (float)log((1 + k) / d1));
    CHECK(m.table[1 * 4 + 3] == (float)log((0 + k) / d1) && m.end[1] == (float)log((1 + k) / d1));
    // context 2: -> 3 x1, end x3: total 4;  context 3: -> 1 x1, end x1: total 2
    CHECK(m.table[2 * 4 + 3] == (float)log((1 + k) / (4 + 4 * k)) && m.end[2] == (float)log((3 + k) / (4 + 4 * k)));
    CHECK(m.table[3 * 4 + 1] == (float)log((1 + k) / (2 + 4 * k)) && m.end[3] == (float)log((1 + k) / (2 + 4 * k)));
    for (int x = 0; x < 4; x++) CHECK(m.table[x * 4] == 0.0f);   // column 0
  }
  {
    const CharLMTables m = CharLMTables::estimate(corpus, 4, 3, k);
    CHECK(m.table.size() == 64 && m.end.size() == 16);
    // context (0, 1) = 1: -> 2 x2, -> 1 x1: total 3;  context (1, 2) = 6: -> 3 x1, end x2: total 3;  context (3, 1) = 13: -> 2 x1
    CHECK(m.table[1 * 4 + 2] == (float)log((2 + k) / (3 + 4 * k)) && m.table[1 * 4 + 1] == (float)log((1 + k) / (3 + 4 * k)));
    CHECK(m.table[6 * 4 + 3] == (float)log((1 + k) / (3 + 4 * k)) && m.end[6] == (float)log((2 + k) / (3 + 4 * k)));
    CHECK(m.table[13 * 4 + 2] == (float)log((1 + k) / (1 + 4 * k)));
    CHECK(m.table[9 * 4 + 1] == (float)log(k / (4 * k)) && m.end[9] == (float)log(k / (4 * k)));   // a context never seen
    // ---- save / load round trip ----
    m.save(f);
    const CharLMTables r = CharLMTables::load(f);
    CHECK(r.order == 3 && r.nc == 4 && r.has_end && r.table == m.table && r.end == m.end && r.tobytes() == m.tobytes());
    // ---- truncated at every length, and oversized ----
    const string bytes = m.tobytes();
    for (size_t n = 0; n < bytes.size(); n += (n < 24 ? 1 : 37)) {
      write_bytes(f, bytes.substr(0, n));
      CHECK(refused(f, n < 20 ? "not a CLSTMLM1 file" : "truncated"));
    }
    write_bytes(f, bytes + string(1, '\0'));
    CHECK(refused(f, "bytes after the tables"));
    write_bytes(f, bytes + bytes);
    CHECK(refused(f, "bytes after the tables"));
    CharLMTables noend = m;
    noend.has_end = false;
    noend.end.clear();
    noend.save(f);
    CHECK(CharLMTables::load(f).end.empty() && !CharLMTables::load(f).has_end);
    write_bytes(f, noend.tobytes() + string(64, '\0'));   // (exactly the size WITH an end table, the flag says without)
    CHECK(refused(f, "bytes after the tables"));
    // ---- headers that announce what the file cannot hold: refused before anything is allocated ----
    string bad = bytes;
    bad[0] = 'X';
    write_bytes(f, bad);
    CHECK(refused(f, "not a CLSTMLM1 file"));
    const int32_t shapes[][3] = {{1, 4, 1}, {4, 4, 1}, {3, 1, 1}, {3, -4, 1}, {3, 1 << 30, 1}, {2, 0x7fffffff, 0}, {3, 407, 0}, {2, 8193, 0}, {3, 4, 2}, {3, 4, -1}};
    for (auto& sh : shapes) {
      write_bytes(f, header(sh[0], sh[1], sh[2]) + bytes.substr(20));
      CHECK(refused(f, "bad header"));
    }
    write_bytes(f, header(2, 8192, 0));   // the largest table admitted (2^26 floats), none of it there
    CHECK(refused(f, "truncated"));
    // ---- a non-finite entry ----
    bad = bytes;
    const float inf = INFINITY, nan = NAN;
    memcpy(&bad[20 + 4 * 5], &inf, 4);
    write_bytes(f, bad);
    CHECK(refused(f, "not finite"));
    bad = bytes;
    memcpy(&bad[bad.size() - 4], &nan, 4);
    write_bytes(f, bad);
    CHECK(refused(f, "not finite"));
  }
  CHECK(refused(dir + "/no such file", "cannot open"));
  // ---- the estimator's refusals ----
  auto estimate_refuses = [&](const vector<vector<int>>& c, int nc, int order, double add_k) {
    try { CharLMTables::estimate(c, nc, order, add_k); } catch (const HostError&) { return true; }
    return false;
  };
  CHECK(estimate_refuses({{1, 4}}, 4, 2, k) && estimate_refuses({{0}}, 4, 2, k) && estimate_refuses({{-1}}, 4, 3, k));
  CHECK(estimate_refuses(corpus, 4, 1, k) && estimate_refuses(corpus, 4, 4, k) && estimate_refuses(corpus, 1, 2, k) && estimate_refuses(corpus, 407, 3, k));
  CHECK(estimate_refuses(corpus, 4, 2, 0.0) && estimate_refuses(corpus, 4, 2, -1.0) && estimate_refuses(corpus, 4, 2, NAN));
  remove(f.c_str());
  if (failures) { std::cerr << failures << " checks FAILED" << std::endl; return 1; }
  std::cout << "charlm_check: ok" << std::endl;
  return 0;
}
