// clstm_hosttool -- test helper exposing the GPU-free host pieces (PNG, normaliser, model files) to
// the Python test-suite.  Raw float dumps are little-endian float32 preceded by two int32 (w, h).
#include "degrade.h"
#include "lexicon.h"
#include "model.h"
#include "normalizer.h"
#include "png_io.h"
#include <thread>
using namespace clstmhost;

static void read_raw(const string& fname, Image& im) {
  std::ifstream f(fname, std::ios::binary);
  int hdr[2] = {0, 0};
  f.read((char*)hdr, 8);
  if (!f || hdr[0] < 1 || hdr[1] < 1) fail("bad raw image: " + fname);
  im.resize(hdr[0], hdr[1]);
  f.read((char*)im.d.data(), im.d.size() * 4);
  if ((size_t)f.gcount() != im.d.size() * 4) fail("short raw image: " + fname);
}

static void dump(const string& fname, const Image& im) {
  std::ofstream f(fname, std::ios::binary);
  int hdr[2] = {im.w, im.h};
  f.write((const char*)hdr, 8);
  f.write((const char*)im.d.data(), im.d.size() * 4);
}

int main(int argc, char** argv) {
  try {
    string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "png2raw" && argc == 4) {  // read_png
      Image im;
      read_png(im, argv[2]);
      dump(argv[3], im);
    } else if (cmd == "normalize" && argc == 5) {  // read_png, invert, CenterNormalizer -> frames
      Image im, out;
      read_png(im, argv[2]);
      for (float& v : im.d) v = -v + 1.0f;
      CenterNormalizer nz;
      nz.target_height = atoi(argv[4]);
      nz.measure(im);
      nz.normalize(out, im);
      dump(argv[3], out);
      std::cout << "r " << nz.r << " width " << out.w << std::endl;
    } else if (cmd == "normalize-raw" && (argc == 5 || argc == 8)) {  // IN.raw OUT.raw HEIGHT [SMOOTH2D SMOOTH1D RANGE]
      // CenterNormalizer on a raw dump with ink = 1: the bit-level referee of the device normaliser for arbitrary images
      std::ifstream f(argv[2], std::ios::binary);
      int hdr[2] = {0, 0};
      f.read((char*)hdr, 8);
      if (!f || hdr[0] < 1 || hdr[1] < 1) fail(string("bad raw image: ") + argv[2]);
      Image im, out;
      im.resize(hdr[0], hdr[1]);
      f.read((char*)im.d.data(), im.d.size() * 4);
      if ((size_t)f.gcount() != im.d.size() * 4) fail(string("short raw image: ") + argv[2]);
      CenterNormalizer nz;
      nz.target_height = atoi(argv[4]);
      if (argc == 8) { nz.smooth2d = (float)atof(argv[5]); nz.smooth1d = (float)atof(argv[6]); nz.range = (float)atof(argv[7]); }
      nz.measure(im);
      nz.normalize(out, im);
      dump(argv[3], out);
      std::cout << "r " << nz.r << " width " << out.w << std::endl;
    } else if (cmd == "normalize-bench" && argc == 5) {  // IN.raws HEIGHT THREADS: the host CenterNormalizer's rate on a file of raw dumps
      std::ifstream f(argv[2], std::ios::binary);
      vector<Image> ims;
      int hdr[2];
      while (f.read((char*)hdr, 8)) {
        ims.emplace_back();
        ims.back().resize(hdr[0], hdr[1]);
        f.read((char*)ims.back().d.data(), ims.back().d.size() * 4);
      }
      const int height = atoi(argv[3]), nthreads = std::max(1, atoi(argv[4]));
      vector<int> widths(ims.size());
      const double t0 = now();
      vector<std::thread> pool;
      for (int t = 0; t < nthreads; t++)
        pool.emplace_back([&, t] {
          for (size_t k = t; k < ims.size(); k += nthreads) {
            CenterNormalizer nz;
            Image out;
            nz.target_height = height;
            nz.measure(ims[k]);
            nz.normalize(out, ims[k]);
            widths[k] = out.w;
          }
        });
      for (auto& th : pool) th.join();
      const double dt = now() - t0;
      long long frames = 0;
      for (int w : widths) frames += w;
      std::cout << ims.size() << " lines " << frames << " frames in " << dt << " s = " << ims.size() / dt << " lines/s" << std::endl;
    } else if (cmd == "degrade-raw" && (argc == 14 || argc == 15)) {  // IN.raw OUT.raw m0 m1 m2 m3 tx ty sigma maxdelta blur seed [noise0|noise1]
      // degrade_line (degrade.h) on a raw dump with ink = 1: the bit-level referee of the device degrader.  With noise0 / noise1
      // OUT.raw is the UNSMOOTHED field 0 / 1 of step 1 instead (the statistics of the hash are tested on it)
      Image im, out;
      read_raw(argv[2], im);
      DegradeLine p{};
      for (int k = 0; k < 4; k++) p.m[k] = (float)atof(argv[4 + k]);
      p.tx = (float)atof(argv[8]); p.ty = (float)atof(argv[9]);
      p.sigma = (float)atof(argv[10]); p.maxdelta = (float)atof(argv[11]); p.blur = (float)atof(argv[12]);
      p.seed = (unsigned)strtoul(argv[13], nullptr, 10);
      if (argc == 15) {
        const string which = argv[14];
        if (which != "noise0" && which != "noise1") fail("degrade-raw: the optional last argument is noise0 or noise1");
        degrade_noise(out, im.w, im.h, p.seed, which == "noise1");
      } else degrade_line(im, p, out);
      dump(argv[3], out);
    } else if (cmd == "degrade-bench" && argc == 4) {  // IN.raws THREADS: the host degrader's rate on a file of raw dumps, parameters
      std::ifstream f(argv[2], std::ios::binary);      // drawn at the default ranges (clstm_degrade_draw, seed 0, key = position, visit 0)
      vector<Image> ims;
      int hdr[2];
      while (f.read((char*)hdr, 8)) {
        ims.emplace_back();
        ims.back().resize(hdr[0], hdr[1]);
        f.read((char*)ims.back().d.data(), ims.back().d.size() * 4);
      }
      const int nthreads = std::max(1, atoi(argv[3]));
      clstm_degrade_ranges rg;
      if (clstm_degrade_default_ranges(&rg)) fail(clstm_last_error());
      vector<DegradeLine> ps(ims.size());
      static_assert(sizeof(DegradeLine) == sizeof(clstm_degrade_line), "DegradeLine is clstm_degrade_line");
      for (size_t k = 0; k < ims.size(); k++)
        if (clstm_degrade_draw(0, k, 0, &rg, ims[k].w, ims[k].h, (clstm_degrade_line*)&ps[k])) fail(clstm_last_error());
      vector<double> ink(ims.size());
      const double t0 = now();
      vector<std::thread> pool;
      for (int t = 0; t < nthreads; t++)
        pool.emplace_back([&, t] {
          for (size_t k = t; k < ims.size(); k += nthreads) {
            Image out;
            degrade_line(ims[k], ps[k], out);
            double s = 0.0;
            for (float v : out.d) s += v;
            ink[k] = s;
          }
        });
      for (auto& th : pool) th.join();
      const double dt = now() - t0;
      double total = 0.0;
      for (double s : ink) total += s;
      std::cout << ims.size() << " lines (ink " << total << ") in " << dt << " s = " << ims.size() / dt << " lines/s" << std::endl;
    } else if (cmd == "writepng" && argc == 4) {  // raw -> png (write_png)
      std::ifstream f(argv[2], std::ios::binary);
      int hdr[2];
      f.read((char*)hdr, 8);
      Image im;
      im.resize(hdr[0], hdr[1]);
      f.read((char*)im.d.data(), im.d.size() * 4);
      write_png(argv[3], im);
    } else if (cmd == "init-model" && argc >= 8) {  // kind ninput nhidden nhidden2 nclasses seed out
      Model m;
      LCG lcg(atof(argv[7]));
      m.create(argv[2], atoi(argv[3]), atoi(argv[6]), atoi(argv[4]), atoi(argv[5]), lcg);
      for (int i = 0; i < m.desc.nclasses; i++) m.codec.push_back(i == 0 ? 0 : 96 + i);
      m.attr["learning_rate"] = std::to_string(1e-4);
      m.attr["momentum"] = std::to_string(0.9);
      m.save(argv[8]);
    } else if (cmd == "roundtrip" && argc == 4) {  // load model file, save it again
      Model m;
      m.load(argv[2]);
      m.save(argv[3]);
      std::cout << m.kind() << " ninput " << m.desc.ninput << " nhidden " << m.desc.nhidden[0] << " nclasses "
                << m.desc.nclasses << " nparams " << m.nparams() << std::endl;
    } else if (cmd == "params" && argc == 4) {  // flat float32 params of a model file
      Model m;
      m.load(argv[2]);
      std::ofstream f(argv[3], std::ios::binary);
      f.write((const char*)m.params.data(), m.params.size() * 4);
    } else if (cmd == "codec" && argc == 3) {  // the code point of every class of a model file, one per line
      Model m;
      m.load(argv[2]);
      for (int c : m.codec) std::cout << c << std::endl;
    } else if (cmd == "lexicon" && (argc == 4 || argc == 5)) {  // MODEL WORDLIST [WORD_CHARS]: what lexicon.h makes of a word list
      Model m;                                                    // under the model's codec: counts, word classes, the words
      m.load(argv[2]);
      std::map<int, int> enc;
      for (int i = 0; i < (int)m.codec.size(); i++) enc.insert(std::make_pair(m.codec[i], i));
      const string wc = argc == 5 ? argv[4] : "";
      const WordList wl = WordList::load(argv[3], enc, (int)m.codec.size(), argc == 5 ? &wc : nullptr);
      std::cout << "lines " << wl.lines << " kept " << wl.words.size() << " dropped " << wl.dropped() << std::endl << "classes";
      for (int c = 0; c < (int)wl.word_class.size(); c++) if (wl.word_class[c]) std::cout << " " << c;
      std::cout << std::endl;
      for (const auto& w : wl.words) { std::cout << "word"; for (int c : w) std::cout << " " << c; std::cout << std::endl; }
    } else {
      std::cerr << "usage: clstm_hosttool png2raw|normalize|normalize-raw|normalize-bench|degrade-raw|degrade-bench|writepng|init-model|roundtrip|params|codec|lexicon ...\n";
      return 2;
    }
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "FATAL: " << e.what() << std::endl;
    return 1;
  }
}
