// clstmlm -- estimates a character n-gram language model for the beam search (clstmocr beam=W lm=FILE) from ground-truth texts
// through a model's codec (not in the reference): for every file name of the list, <name up to its first '.'>.gt.txt is read as
// clstmocrtrain reads it and encoded to the model's classes; charlm.h holds the estimator and the file format, the same as
// clstm_amd.lm.CharLM.estimate / save.  No device work.
#include "clstmhl.h"
using namespace clstmhost;

static int main1(int argc, char** argv) {
  if (argc != 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) {
    std::cerr << "Usage: [VAR=VAL...] " << argv[0] << " IMAGEFILE-LIST\n  Variables: load out (required)  order (2 | 3, default 3)  add_k (default 0.1)\n";
    return EXIT_FAILURE;
  }
  const string load_name = getsenv("load", ""), out_name = getsenv("out", "");
  if (load_name == "") fail("must give load= parameter");
  if (out_name == "") fail("must give out= parameter");
  const int order = getienv("order", 3);
  const double add_k = getdenv("add_k", 0.1);
  Model model;
  model.load(load_name);
  Codec codec;
  codec.set(model.codec);
  vector<string> names;
  read_lines(names, argv[1]);
  vector<vector<int>> sequences;
  for (const string& name : names) {
    if (name.empty()) continue;
    Classes cs;
    codec.encode(cs, utf8_to_utf32(read_text(basename_noext(name) + ".gt.txt")));
    sequences.push_back(cs);
  }
  const CharLMTables m = CharLMTables::estimate(sequences, codec.size(), order, add_k);
  m.save(out_name);
  std::cerr << "# " << sequences.size() << " lines, order " << order << ", " << codec.size() << " classes -> " << out_name << std::endl;
  return 0;
}

int main(int argc, char** argv) {
  try { return main1(argc, argv); }
  catch (const std::exception& e) { std::cerr << "FATAL: " << e.what() << std::endl; return 1; }
}
