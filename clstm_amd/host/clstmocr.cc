// clstmocr -- the reference's recognition driver (clstmocr.cc:40-117) on the MI355X path.
#include "clstmhl.h"
#include <sstream>
using namespace clstmhost;

static float scaled_log(float x) {  // clstmocr.cc:33-40 (float arithmetic, clamped to [0, 1])
  const float thresh = 10.0f;
  if (x <= 0.0f) return 0.0f;
  float l = logf(x);
  if (l < -thresh) return 0.0f;
  if (l > 0) return 1.0f;
  return (l + thresh) / thresh;
}

static int main1(int argc, char** argv) {
  if (argc != 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) {
    std::cerr << "Usage: [VAR=VAL...] " << argv[0] << " IMAGEFILE-LIST\n  Variables: load (required) conf output save_text\n"
              << "             batch (lines per recognition call, default 1)  prep_threads (<= 16)\n"
              << "             beam nbest (beam=W: the nbest <= W best transcripts of every line follow its output; default off)   (not in the reference)\n"
              << "             lm lm_weight lm_bonus (with beam=W: a character n-gram model file inside the search; hypotheses gain an am_score column)   (not in the reference)\n"
              << "             lexicon word_chars (with beam=W: a UTF-8 word list, one word per line; every run of word characters of a hypothesis is a word of it)   (not in the reference)\n"
              << "             errs (1: ERRS / CER / CONF lines for the lines that have a .gt.txt beside them, counted on the device; default 0)   (not in the reference)\n"
              << "             gpu_prep (1: lines are normalised on the device, helper threads only read PNGs; default 0)   (not in the reference)\n";
    return EXIT_FAILURE;
  }
  string load_name = getsenv("load", "");
  if (load_name == "") fail("must give load= parameter");
  CLSTMOCR clstm;
  clstm.load(load_name);
  bool conf = getienv("conf", 0);
  string output = getsenv("output", "text");
  bool save_text = getienv("save_text", 1);
  // batch=N (not in the reference; default 1 = the loop below, line by line): N lines per clstm_net_predict_h call.  Lines are read
  // and normalised ahead on up to prep_threads (<= 16) helper threads -- a chunk is prepared while the device recognises the one
  // before it -- and results are printed and written in input order, in the formats of the per-line loop.
  const int batch = std::max(1, getienv("batch", 1));
  const int prep_threads = std::max(1, std::min(std::min(getienv("prep_threads", 16), 16), std::max(1, (int)std::thread::hardware_concurrency())));
  // gpu_prep=1 (default 0: nothing changes): the helper threads only read the PNGs and every chunk goes through
  // CLSTMOCR::predict_batch_gpu -- CenterNormalizer on the device (clstm_normalizer_run_h), its frames handed to clstm_net_predict
  // where they lie.  The frames are the host normaliser's bit for bit, so the output is the same bytes.
  const bool gpu_prep = getienv("gpu_prep", 0) != 0;
  // align=1 (default 0: nothing changes): for every input line with a ground truth beside it (<name up to its first '.'>.gt.txt) the
  // forced alignment follows the line's ordinary output: "align <file>", then per ground-truth character "<char>\t<x0>\t<x1>" --
  // the first and last frame column it occupies on the best path (-1 -1: never visited) --, then "end <score>" with the ground
  // truth's CTC score on the line (CLSTMOCR::score)
  const bool do_align = getienv("align", 0) != 0;
  // beam=W nbest=K (default beam=0: nothing changes): every line's ordinary output is followed by "nbest <file>", one line
  // "<k>\t<score>\t<text>" per hypothesis of the device's CTC prefix beam search (CLSTMOCR::predict_nbest; width W, the K best,
  // K defaults to W; the score is the log-probability the beam gathered for the text), then "end".  With align=1 a line that has no
  // ground truth beside it gets the alignment of its top hypothesis.
  const int beam = getienv("beam", 0);
  const int nbest = beam > 0 ? getienv("nbest", beam) : 0;
  if (beam != 0 && (beam < 1 || beam > 32 || nbest < 1 || nbest > beam)) fail("beam / nbest: 1 <= nbest <= beam <= 32");
  // lm=FILE lm_weight=A lm_bonus=B (with beam=W only; default none: nothing changes): the search runs with the character n-gram model
  // of FILE (clstmlm writes one) inside the extension step (CLSTMOCR::set_lm), and a hypothesis line becomes
  // "<k>\t<score>\t<am_score>\t<text>": the total that was ranked, then the acoustic log-probability beam=W alone prints.
  const string lm_name = getsenv("lm", "");
  const bool with_lm = !lm_name.empty();
  if (with_lm && beam == 0) fail("lm= needs beam=W: the language model works inside the beam search");
  if (with_lm) clstm.set_lm(lm_name, (float)getdenv("lm_weight", 1.0), (float)getdenv("lm_bonus", 0.0));
  // lexicon=FILE [word_chars=STRING] (with beam=W only; default none: nothing changes): the search is constrained to the word list of
  // FILE (UTF-8, one word per line; CLSTMOCR::set_lexicon, clstm_net_beam_lex): every run of word characters of a hypothesis is a word
  // of the list.  A class is a word character iff it occurs in a word of the list, or, with word_chars=, iff it occurs in that string;
  // every other class separates words.  Works with and without lm=; lm_bonus= applies either way.  A line on which no admissible
  // transcript survived gets the hypotheses of the search WITHOUT the lexicon, each prefixed "LEXMISS\t"; the number of such lines is
  // reported on stderr at the end.
  const string lex_name = getsenv("lexicon", "");
  const bool with_lex = !lex_name.empty();
  if (with_lex && beam == 0) fail("lexicon= needs beam=W: the lexicon works inside the beam search");
  if (with_lex) {
    const string word_chars = getsenv("word_chars", "");
    clstm.set_lexicon(lex_name, word_chars.empty() ? nullptr : &word_chars);
    if (!with_lm) clstm.lm_bonus = (float)getdenv("lm_bonus", 0.0);
    std::cerr << "lexicon: " << clstm.lexicon_words << " words, " << clstm.lexicon_dropped << " lines of " << lex_name << " dropped" << std::endl;
  }
  long long lexmiss = 0;
  // the lines of the current minibatch the lexicon left without a hypothesis: theirs are those of the search without it
  auto fill_misses = [&](const vector<int>& Ts, vector<vector<Hypothesis>>& hyps, vector<char>& miss) {
    miss.assign(hyps.size(), 0);
    if (!with_lex) return;
    bool any = false;
    for (size_t k = 0; k < hyps.size(); k++) if (hyps[k].empty() && Ts[k] > 0) { miss[k] = 1; any = true; lexmiss++; }
    if (!any) return;
    vector<vector<Hypothesis>> plain;
    clstm.nbest_current(Ts, beam, nbest, plain, false);
    for (size_t k = 0; k < hyps.size(); k++) if (miss[k]) hyps[k] = plain[k];
  };
  auto print_nbest = [&](const string& name, const vector<Hypothesis>& hyps, bool miss = false) {
    std::cout << "nbest " << name << std::endl;
    for (size_t k = 0; k < hyps.size(); k++) {
      char buf[64], am[64];
      snprintf(buf, sizeof buf, "%.9g", (double)hyps[k].score);
      snprintf(am, sizeof am, "%.9g", (double)hyps[k].am_score);
      if (miss) std::cout << "LEXMISS\t";
      std::cout << k << "\t" << buf << "\t";
      if (with_lm) std::cout << am << "\t";
      std::cout << utf32_to_utf8(hyps[k].text) << std::endl;
    }
    std::cout << "end" << std::endl;
  };
  auto print_alignment = [&](const string& name, const vector<CharSpan>& spans, float score) {
    std::cout << "align " << name << std::endl;
    for (const CharSpan& c : spans) std::cout << utf32_to_utf8(ustring(1, c.c)) << "\t" << c.x0 << "\t" << c.x1 << std::endl;
    char buf[64];
    snprintf(buf, sizeof buf, "%.9g", (double)score);
    std::cout << "end " << buf << std::endl;
  };
  // false: no ground truth beside the line, or one the model's codec cannot encode (then "noalign <file>\t<reason>" is printed where
  // the alignment would have stood, and recognition goes on)
  vector<string> noalign;   // notes of the current chunk, by line index
  auto ground_truth = [&](const string& name, ustring& gt, string* note) -> bool {
    const string gtname = basename_noext(name) + ".gt.txt";
    if (!std::ifstream(gtname)) return false;
    gt = utf8_to_utf32(read_text(gtname));
    try {
      Classes cs;
      clstm.codec.encode(cs, gt);
    } catch (const std::exception& e) {
      *note = "noalign " + name + "\t" + e.what();
      return false;
    }
    return true;
  };
  // errs=1 (default 0: nothing changes): every input line with a ground truth beside it (<name up to its first '.'>.gt.txt) is followed by
  // "ERRS <file> <dist> <sub> <ins> <del> <reflen>" -- the Levenshtein distance of its output against the ground truth and the
  // substitutions, insertions (output only) and deletions (ground truth only) of the canonical edit script, counted on the device
  // (CLSTMOCR::errors_current) -- and, with beam=W, by "ORACLE <file> <dist> <k>": the smallest distance among its n best and the first
  // hypothesis that has it.  After the last line: "CER <total dist> <total reflen> <rate>", then the 20 largest off-diagonal entries of the
  // confusion table as "CONF <count> <ref char or _> <out char or _>" (_: nothing -- an insertion or a deletion; ?: a character outside the
  // codec), largest first, equal counts by the reference character's code, then the output character's, _ first.
  const bool do_errs = getienv("errs", 0) != 0;
  const int nsym = clstm.nclasses + 1;
  vector<long long> confusion((size_t)nsym * nsym, 0);
  long long total_dist = 0, total_ref = 0;
  // the lines of the current minibatch (Ts) named `names`: ERRS and ORACLE lines by line index, the totals
  auto count_errors = [&](const vector<string>& names, const vector<int>& Ts, const vector<ustring>& outs, const vector<vector<Hypothesis>>* hyps,
                          vector<string>& lines_out) {
    lines_out.assign(names.size(), "");
    vector<ustring> with_gt;
    vector<int> gt_line;
    for (size_t k = 0; k < names.size(); k++) {
      const string gtname = basename_noext(names[k]) + ".gt.txt";
      if (!std::ifstream(gtname)) continue;
      gt_line.push_back((int)k);
      with_gt.push_back(utf8_to_utf32(read_text(gtname)));
    }
    if (gt_line.empty()) return;
    // every line has one: the decoded classes are compared where they lie on the device; else the texts of the lines that have one
    vector<int> dist, counts, conf;
    if (gt_line.size() == names.size()) clstm.errors_current(Ts, with_gt, &dist, &counts, &conf);
    else {
      vector<ustring> texts;
      for (int k : gt_line) texts.push_back(outs[k]);
      clstm.errors_texts(texts, with_gt, &dist, &counts, &conf);
    }
    for (size_t i = 0; i < conf.size(); i++) confusion[i] += conf[i];
    vector<int> best, best_k;
    if (hyps) clstm.oracle_distance(*hyps, with_gt, gt_line, best, best_k);
    for (size_t g = 0; g < gt_line.size(); g++) {
      const int k = gt_line[g];
      std::ostringstream o;
      o << "ERRS " << names[k] << " " << dist[g] << " " << counts[3 * g] << " " << counts[3 * g + 1] << " " << counts[3 * g + 2] << " "
        << with_gt[g].size() << "\n";
      if (hyps) o << "ORACLE " << names[k] << " " << best[g] << " " << best_k[g] << "\n";
      lines_out[k] = o.str();
      total_dist += dist[g];
      total_ref += (long long)with_gt[g].size();
    }
  };
  auto print_error_totals = [&]() {
    std::cout << "CER " << total_dist << " " << total_ref << " " << (total_ref ? (double)total_dist / (double)total_ref : 0.0) << std::endl;
    struct Entry { long long n; int r, h; };
    vector<Entry> top;
    for (int r = 0; r < nsym; r++)
      for (int h = 0; h < nsym; h++)
        if (r != h && confusion[(size_t)r * nsym + h] > 0) top.push_back(Entry{confusion[(size_t)r * nsym + h], r, h});
    std::stable_sort(top.begin(), top.end(), [](const Entry& x, const Entry& y) { return x.n > y.n; });   // (built in label = code order)
    auto name_of = [&](int c) { return c == 0 ? string("_") : c == clstm.nclasses ? string("?") : utf32_to_utf8(ustring(1, (char32_t)clstm.codec.codec[c])); };
    for (size_t i = 0; i < top.size() && i < 20; i++)
      std::cout << "CONF " << top[i].n << " " << name_of(top[i].r) << " " << name_of(top[i].h) << std::endl;
  };
  if (batch > 1 || gpu_prep) {
    if (output != "text" && output != "logs" && output != "posteriors") fail("unknown output format");
    vector<string> names;
    read_lines(names, argv[1]);
    struct Chunk { vector<string> names; vector<Image> frames; };
    auto prepare = [&](Chunk& c, size_t first) {
      c.names.assign(names.begin() + first, names.begin() + std::min(names.size(), first + (size_t)batch));
      c.frames.assign(c.names.size(), Image());
      auto work = [&](int k0) {
        for (size_t k = k0; k < c.names.size(); k += prep_threads) {
          Image raw;
          read_png(raw, c.names[k]);
          for (float& v : raw.d) v = -v + 1.0f;
          if (gpu_prep) c.frames[k] = std::move(raw);   // (the raw line: normalised on the device, by the main thread)
          else clstm.normalize_line(c.frames[k], raw);
        }
      };
      vector<std::future<void>> pool;
      for (int t = 1; t < prep_threads && t < (int)c.names.size(); t++) pool.push_back(std::async(std::launch::async, work, t));
      work(0);
      for (auto& f : pool) f.get();   // (rethrows a worker's exception)
    };
    Chunk cur, next;
    std::future<void> helper;
    if (!names.empty()) prepare(next, 0);
    for (size_t first = 0; first < names.size(); first += batch) {
      std::swap(cur, next);
      if (first + batch < names.size()) helper = std::async(std::launch::async, [&, first] { prepare(next, first + batch); });
      vector<const Image*> ptrs;
      for (auto& f : cur.frames) ptrs.push_back(&f);
      vector<ustring> outs;
      vector<vector<CharPrediction>> preds;
      vector<vector<Hypothesis>> hyps;
      vector<char> miss;
      if (beam > 0) { clstm.predict_nbest(ptrs, beam, nbest, outs, hyps, conf ? &preds : nullptr, gpu_prep); fill_misses(clstm.batch_T, hyps, miss); }
      else if (gpu_prep) clstm.predict_batch_gpu(ptrs, outs, conf ? &preds : nullptr);
      else clstm.predict_frames(ptrs, outs, conf ? &preds : nullptr);
      vector<Image> posteriors;
      if (output != "text") clstm.get_outputs_batch(posteriors);
      vector<vector<CharSpan>> spans;   // of the lines that have a ground truth, in input order
      vector<int> gt_line;
      vector<float> gt_score;
      if (do_align) {
        vector<ustring> gts;
        noalign.assign(cur.names.size(), "");
        for (size_t k = 0; k < cur.names.size(); k++) {
          ustring gt;
          if (!ground_truth(cur.names[k], gt, &noalign[k])) {
            if (beam == 0 || !noalign[k].empty() || hyps[k].empty()) continue;
            gt = hyps[k][0].text;   // no ground truth: the top hypothesis
          }
          gt_line.push_back((int)k);
          gts.push_back(gt);
        }
        clstm.score_current(clstm.batch_T, gts, &gt_score, &spans, &gt_line);
      }
      vector<string> errs_lines;
      if (do_errs) count_errors(cur.names, clstm.batch_T, outs, beam > 0 ? &hyps : nullptr, errs_lines);
      size_t next_gt = 0;
      for (size_t k = 0; k < cur.names.size(); k++) {
        const string& name = cur.names[k];
        string basename = name.substr(0, name.find_last_of("."));
        if (!conf) {
          string out = utf32_to_utf8(outs[k]);
          std::cout << name << "\t" << out << std::endl;
          if (save_text) write_text(basename + ".txt", out);
        } else {
          std::cout << "file " << name << std::endl;
          for (auto& p : preds[k]) {
            ustring c(1, p.c);
            std::cout << p.i << "\t" << p.x << "\t" << utf32_to_utf8(c) << "\t" << p.p << std::endl;
          }
        }
        if (output != "text") {
          if (output == "logs")
            for (float& v : posteriors[k].d) v = scaled_log(v);
          write_png(basename + (output == "logs" ? ".lp.png" : ".p.png"), posteriors[k]);
        }
        if (beam > 0) print_nbest(name, hyps[k], miss[k] != 0);
        if (next_gt < gt_line.size() && gt_line[next_gt] == (int)k) { print_alignment(name, spans[next_gt], gt_score[next_gt]); next_gt++; }
        else if (do_align && !noalign[k].empty()) std::cout << noalign[k] << std::endl;
        if (do_errs) std::cout << errs_lines[k] << std::flush;
      }
      if (helper.valid()) helper.get();
    }
    if (do_errs) print_error_totals();
    if (with_lex) std::cerr << "lexicon: " << lexmiss << " lines without an admissible transcript (LEXMISS)" << std::endl;
    return 0;
  }
  std::ifstream stream(argv[1]);
  string line;
  while (getline(stream, line)) {
    Image raw;
    string basename = line.substr(0, line.find_last_of("."));
    read_png(raw, line);
    for (float& v : raw.d) v = -v + 1.0f;
    ustring out32;   // (errs=1: the line's output as text)
    if (!conf) {
      string out = clstm.predict_utf8(raw);
      out32 = utf8_to_utf32(out);
      std::cout << line << "\t" << out << std::endl;
      if (save_text) write_text(basename + ".txt", out);
    } else {
      std::cout << "file " << line << std::endl;
      vector<CharPrediction> preds;
      clstm.predict(preds, raw);
      for (auto& p : preds) out32.push_back(p.c);
      for (auto& p : preds) {
        ustring c(1, p.c);
        std::cout << p.i << "\t" << p.x << "\t" << utf32_to_utf8(c) << "\t" << p.p << std::endl;
      }
    }
    if (output == "text") {
    } else if (output == "logs" || output == "posteriors") {
      Image outputs;
      clstm.get_outputs(outputs);
      if (output == "logs")
        for (float& v : outputs.d) v = scaled_log(v);
      write_png(basename + (output == "logs" ? ".lp.png" : ".p.png"), outputs);
    } else fail("unknown output format");
    vector<vector<Hypothesis>> hyps;
    if (beam > 0) {
      vector<char> miss;
      clstm.nbest_current(vector<int>(1, clstm.T), beam, nbest, hyps);
      fill_misses(vector<int>(1, clstm.T), hyps, miss);
      print_nbest(line, hyps[0], miss[0] != 0);
    }
    ustring gt;
    string note;
    bool have_gt = do_align && ground_truth(line, gt, &note);
    if (do_align && !have_gt && note.empty() && beam > 0 && !hyps[0].empty()) { gt = hyps[0][0].text; have_gt = true; }
    if (do_align && !have_gt) {
      if (!note.empty()) std::cout << note << std::endl;
    } else if (do_align) {
      vector<vector<CharSpan>> spans;
      vector<float> sc;
      clstm.score_current(vector<int>(1, clstm.T), vector<ustring>(1, gt), &sc, &spans);
      print_alignment(line, spans[0], sc[0]);
    }
    if (do_errs) {
      vector<string> errs_lines;
      count_errors(vector<string>(1, line), vector<int>(1, clstm.T), vector<ustring>(1, out32), beam > 0 ? &hyps : nullptr, errs_lines);
      std::cout << errs_lines[0] << std::flush;
    }
  }
  if (do_errs) print_error_totals();
  if (with_lex) std::cerr << "lexicon: " << lexmiss << " lines without an admissible transcript (LEXMISS)" << std::endl;
  return 0;
}

int main(int argc, char** argv) {
  try { return main1(argc, argv); }
  catch (const std::exception& e) { std::cerr << "FATAL: " << e.what() << std::endl; return 1; }
}
