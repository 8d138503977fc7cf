// clstmhl.h -- CLSTMOCR (clstmhl.h:146-272) and Codec (clstm.h:82-93, clstm.cc:219-263) on top of the
// C ABI of libclstm_hip.so.  Same members and call order as the reference: measure/normalize ->
// set_inputs -> forward -> mktargets/ctc_align_targets -> backward -> trivial_decode -> sgd_update.
// The host holds only small arrays (the line image, transcripts, decodes); all network arithmetic
// runs on the MI355X.
#pragma once
#include "model.h"
#include <future>
#include <thread>
#include "charlm.h"
#include "lexicon.h"
#include "normalizer.h"
#include "png_io.h"

namespace clstmhost {

typedef vector<int> Classes;

inline void chk(int rc, const char* what) {
  if (rc) fail(string(what) + ": " + clstm_last_error());
}

struct Codec {
  vector<int> codec;
  std::map<int, int> encoder;
  int size() const { return (int)codec.size(); }
  void set(const vector<int>& a) {
    codec = a;
    encoder.clear();
    for (int i = 0; i < (int)codec.size(); i++) encoder.insert(std::make_pair(codec[i], i));
  }
  void encode(Classes& cs, const ustring& s) const {  // clstm.cc:226-236 (asserts become errors)
    cs.clear();
    for (char32_t ch : s) {
      auto it = encoder.find((int)ch);
      if (it == encoder.end()) fail("character not in codec: U+" + std::to_string((unsigned)ch));
      if (it->second == 0) fail("transcript maps to class 0 (reserved for blank)");
      cs.push_back(it->second);
    }
  }
  ustring decode(const Classes& cs) const {
    ustring s;
    for (int c : cs) s.push_back((char32_t)codec.at(c));
    return s;
  }
  void build(const vector<string>& fnames, const ustring& extra = U"") {  // clstm.cc:246-267
    std::set<int> codes;
    codes.insert(0);
    for (char32_t c : extra) codes.insert((int)c);
    for (auto& fname : fnames) {
      std::ifstream stream(fname);
      string line;
      while (getline(stream, line)) {
        if (line.substr(0, 1) == "#") continue;
        if (line.size() == 0) continue;
        for (char32_t c : utf8_to_utf32(line)) codes.insert((int)c);
      }
    }
    set(vector<int>(codes.begin(), codes.end()));
  }
};

// trivial_decode (ctc.cc:159-190) on a host matrix [T][nc]; used for the "ALN" report line only
inline void trivial_decode_host(Classes& cs, const float* out, int T, int nc) {
  cs.clear();
  float mv = 0;
  int mc = -1;
  for (int t = 0; t < T; t++) {
    const float* p = out + (size_t)t * nc;
    int index = -1;
    float best = p[0];
    for (int i = 0; i < nc; i++) {
      if (p[i] < best) continue;
      index = i;
      best = p[i];
    }
    if (index == 0) {
      if (mc != -1 && mc != 0) cs.push_back(mc);
      mv = 0;
      mc = -1;
      continue;
    }
    if (best > mv) { mv = best; mc = index; }
  }
}

struct CharPrediction { int i, x; char32_t c; float p; };
// one of a line's n best transcripts (CLSTMOCR::predict_nbest)
// (score: what the search ranked; am_score: the acoustic log-probability -- the same number unless a language model is set)
struct Hypothesis { ustring text; float score; float am_score; };
// forced alignment: the frame columns x0 .. x1 a transcript's i-th character occupies on a best path (-1, -1: the path never visits it)
struct CharSpan { int i, x0, x1; char32_t c; };

// predict(): the forward pass belongs to no training step -- a non-finite logit there must not arm the device flag that blocks
// updates (clstm_net_set_training; the reference only asserts in backward, clstm.cc:630-649)
struct InferenceScope {
  clstm_net* net;
  explicit InferenceScope(clstm_net* n) : net(n) { clstm_net_set_training(net, 0); }
  ~InferenceScope() { clstm_net_set_training(net, 1); }
};

struct CLSTMOCR {
  Model model;
  Codec codec;
  CenterNormalizer normalizer;
  clstm_net* net = nullptr;
  int target_height = 48;
  int nclasses = -1;
  Image image;
  vector<float> aligned;  // [T][nclasses] of the last fwdbwd
  int T = 0;

  clstm_charlm* lm = nullptr;                   // set_lm: the n-best calls search with it (clstm_net_beam_lm)
  float lm_weight = 0.0f, lm_bonus = 0.0f;
  clstm_lexicon* lexicon = nullptr;             // set_lexicon: the n-best calls are constrained to it (clstm_net_beam_lex)
  long long lexicon_words = 0, lexicon_dropped = 0;   // distinct words in the trie; lines of the word list that were dropped
  clstm_normalizer* gpu_normalizer = nullptr;   // the device twin of `normalizer` (created at first use: predict_batch_gpu, normalize_batch_gpu)
  // set_degrade: normalize_batch_gpu degrades its lines on the device first (clstm_degrader_*; training only, never recognition)
  clstm_degrader* gpu_degrader = nullptr;
  unsigned long long degrade_seed = 0;
  clstm_degrade_ranges degrade_ranges{};
  void set_degrade(unsigned long long seed, const clstm_degrade_ranges& ranges) {
    if (!gpu_degrader) chk(clstm_degrader_create(&gpu_degrader), "clstm_degrader_create");
    degrade_seed = seed;
    degrade_ranges = ranges;
  }
  ~CLSTMOCR() {
    if (lm) clstm_charlm_destroy(lm);
    if (lexicon) clstm_lexicon_destroy(lexicon);
    if (gpu_normalizer) clstm_normalizer_destroy(gpu_normalizer);
    if (gpu_degrader) clstm_degrader_destroy(gpu_degrader);
    if (net) clstm_net_destroy(net);
  }
  void attach() {  // device network from the host model
    if (net) { clstm_net_destroy(net); net = nullptr; }
    chk(clstm_net_create(&net, &model.desc, nullptr, nullptr, nullptr), "clstm_net_create");
    chk(clstm_net_set_params_h(net, model.params.data()), "clstm_net_set_params_h");
    nclasses = model.desc.nclasses;
    target_height = model.desc.ninput;
    normalizer.target_height = target_height;
    if (gpu_normalizer) { clstm_normalizer_destroy(gpu_normalizer); gpu_normalizer = nullptr; }
    codec.set(model.codec);
    const float lr = atof(attr_get("learning_rate", "1e-4").c_str());
    const float mom = atof(attr_get("momentum", "0.9").c_str());
    chk(clstm_net_set_learning_rate(net, lr, mom), "clstm_net_set_learning_rate");
  }
  string attr_get(const string& k, const string& dflt) const {
    auto it = model.attr.find(k);
    return it == model.attr.end() ? dflt : it->second;
  }
  void setLearningRate(float lr, float mom) {  // INetwork::setLearningRate, clstm.cc:158-161
    model.attr["learning_rate"] = std::to_string((double)lr);   // String(double) = std::to_string
    model.attr["momentum"] = std::to_string((double)mom);
    if (net) chk(clstm_net_set_learning_rate(net, lr, mom), "clstm_net_set_learning_rate");
  }
  void createBidi(const vector<int>& codec_, int nhidden) {  // clstmhl.h:191-200
    LCG lcg;
    model.create("bidi", target_height, (int)codec_.size(), nhidden, 0, lcg);
    model.codec = codec_;
    attach();
  }
  void createBidi2(const vector<int>& codec_, int nhidden, int nhidden2) {  // make_net("bidi2", ...), clstm_prefab.cc:86-109
    LCG lcg;
    model.create("bidi2", target_height, (int)codec_.size(), nhidden, nhidden2, lcg);
    model.codec = codec_;
    attach();
  }
  void load(const string& fname) {  // clstmhl.h:157-175
    model.load(fname);
    attach();
  }
  void save(const string& fname) {
    chk(clstm_net_get_params_h(net, model.params.data()), "clstm_net_get_params_h");
    model.save(fname);
  }
  void set_line(const Image& raw) {  // measure / normalize / set_inputs, clstmhl.h:202-205
    normalizer.measure(raw);
    normalizer.normalize(image, raw);
    T = image.w;
    chk(clstm_net_set_batch(net, &T, 1), "clstm_net_set_batch");
    chk(clstm_net_set_inputs_h(net, image.d.data()), "clstm_net_set_inputs_h");  // image(t,i) is frame-major
  }
  Classes decode_outputs(vector<int>* where = nullptr) {
    vector<int> cls(T), loc(T);
    int cnt = 0;
    chk(clstm_net_decode(net, cls.data(), loc.data(), &cnt), "clstm_net_decode");
    cls.resize(cnt);
    if (where) where->assign(loc.begin(), loc.begin() + cnt);
    return cls;
  }
  ustring fwdbwd(const Image& raw, const ustring& target) {  // clstmhl.h:201-217
    set_line(raw);
    chk(clstm_net_forward(net), "clstm_net_forward");
    Classes transcript;
    codec.encode(transcript, target);
    const int L = (int)transcript.size();
    aligned.resize((size_t)T * nclasses);
    chk(clstm_net_ctc(net, transcript.data(), &L, aligned.data()), "clstm_net_ctc");
    chk(clstm_net_backward(net), "clstm_net_backward");
    return codec.decode(decode_outputs());
  }
  void update() { chk(clstm_net_update(net), "clstm_net_update"); }
  ustring train(const Image& raw, const ustring& target) {
    ustring r = fwdbwd(raw, target);
    update();
    return r;
  }
  // ---- a minibatch of lines per update (the batched MI355X path: all lines through ONE forward / CTC / backward,
  // Params.d receives the SUM of the lines' gradients exactly as consecutive CLSTMOCR::fwdbwd calls without an
  // update in between would leave it, clstmhl.h:201-217) ----------------------------------------------------
  struct Prepared {          // host-side half of a minibatch: normalised frames + encoded transcripts
    vector<int> T, L;
    vector<float> frames;    // packed line after line, frame-major
    Classes labels;          // packed transcripts
    vector<ustring> targets;
  };
  // GPU-free: may run on a helper thread while the device works on the previous minibatch (uses only its own
  // normaliser; `codec` is read-only after attach())
  struct Line {              // one normalised line + its encoded transcript (what a dataset cache keeps per file)
    Image frames;            // (w = T, h = target_height)
    Classes labels;
    ustring target;
  };
  void prepare_line(Line& out, const Image& raw, const ustring& target) const {   // (thread-safe: own normaliser)
    CenterNormalizer nz;
    nz.target_height = target_height;
    nz.measure(raw);
    nz.normalize(out.frames, raw);
    codec.encode(out.labels, target);
    out.target = target;
  }
  void pack(Prepared& p, const vector<const Line*>& lines) const {
    p.T.clear(); p.L.clear(); p.frames.clear(); p.labels.clear(); p.targets.clear();
    for (const Line* l : lines) {
      p.T.push_back(l->frames.w);
      p.frames.insert(p.frames.end(), l->frames.d.begin(), l->frames.d.end());
      p.L.push_back((int)l->labels.size());
      p.labels.insert(p.labels.end(), l->labels.begin(), l->labels.end());
      p.targets.push_back(l->target);
    }
  }
  void prepare(Prepared& p, const vector<Image>& raws, const vector<ustring>& targets) const {
    vector<Line> lines(raws.size());
    vector<const Line*> ptrs;
    for (size_t b = 0; b < raws.size(); b++) { prepare_line(lines[b], raws[b], targets[b]); ptrs.push_back(&lines[b]); }
    pack(p, ptrs);
  }
  vector<ustring> train_batch(const Prepared& p) {
    const int bs = (int)p.T.size();
    chk(clstm_net_set_batch(net, p.T.data(), bs), "clstm_net_set_batch");
    chk(clstm_net_set_inputs_h(net, p.frames.data()), "clstm_net_set_inputs_h");
    chk(clstm_net_forward(net), "clstm_net_forward");
    int N = 0;
    for (int t : p.T) N += t;
    vector<int> cls(N), loc(N), cnt(bs);
    chk(clstm_net_decode(net, cls.data(), loc.data(), cnt.data()), "clstm_net_decode");
    aligned.resize((size_t)N * nclasses);
    Classes dummy(1, 1);
    chk(clstm_net_ctc(net, p.labels.empty() ? dummy.data() : p.labels.data(), p.L.data(), aligned.data()), "clstm_net_ctc");
    chk(clstm_net_backward(net), "clstm_net_backward");
    chk(clstm_net_update(net), "clstm_net_update");
    vector<ustring> out;
    int o = 0;
    for (int b = 0; b < bs; b++) {
      out.push_back(codec.decode(Classes(cls.begin() + o, cls.begin() + o + cnt[b])));
      o += p.T[b];
    }
    T = p.T.back();   // aligned_utf8() reports the last line of the minibatch
    if (bs > 1) aligned.erase(aligned.begin(), aligned.begin() + (size_t)(N - T) * nclasses);
    return out;
  }
  // The same minibatch without any host synchronisation (clstm_net_train_step_h: frames on a copy stream, every kernel
  // and the update enqueued): the training loop calls this for the minibatches whose result nobody prints, and
  // train_batch() -- which reads the decode and the alignment back -- where a report is due.  `p` must stay untouched
  // until the call after the next one (the frames are pageable memory: the library copies them before it returns).
  void train_batch_async(const Prepared& p) {
    Classes dummy(1, 1);
    chk(clstm_net_train_step_h(net, p.T.data(), (int)p.T.size(), p.frames.data(), p.labels.empty() ? dummy.data() : p.labels.data(),
                               p.L.data()), "clstm_net_train_step_h");
  }
  void synchronize() { chk(clstm_synchronize(), "clstm_synchronize"); }
  string aligned_utf8() {  // clstmhl.h:224-229
    Classes cs;
    trivial_decode_host(cs, aligned.data(), T, nclasses);
    return utf32_to_utf8(codec.decode(cs));
  }
  ustring predict(const Image& raw, vector<int>* where = nullptr) {  // clstmhl.h:233-242
    set_line(raw);
    InferenceScope inference(net);
    chk(clstm_net_forward(net), "clstm_net_forward");
    return codec.decode(decode_outputs(where));
  }
  string predict_utf8(const Image& raw) { return utf32_to_utf8(predict(raw)); }
  void get_outputs(Image& out) {  // [T][nclasses]
    out.resize(T, nclasses);
    chk(clstm_net_get_outputs_h(net, out.d.data()), "clstm_net_get_outputs_h");
  }
  void predict(vector<CharPrediction>& preds, const Image& raw) {  // clstmhl.h:243-262
    vector<int> where;
    set_line(raw);
    InferenceScope inference(net);
    chk(clstm_net_forward(net), "clstm_net_forward");
    Classes cs = decode_outputs(&where);
    Image out;
    get_outputs(out);
    preds.clear();
    for (int i = 0; i < (int)cs.size(); i++)
      preds.push_back(CharPrediction{i, where[i], (char32_t)codec.codec[cs[i]], out(where[i], cs[i])});
  }
  // ---- batched recognition: predict() for many lines through ONE clstm_net_predict_h call (the no-save forward kernels; the
  // same outputs as the per-line loop above, which runs the same kernel families through clstm_net_forward) -------------------
  // GPU-free and thread-safe (own normaliser, as prepare_line): a driver normalises lines ahead on helper threads
  void normalize_line(Image& frames, const Image& raw) const {
    CenterNormalizer nz;
    nz.target_height = target_height;
    nz.measure(raw);
    nz.normalize(frames, raw);
  }
  // Recognition results should not depend on how many lines share a call.  A line alone (predict above) is computed by the per-line
  // kernels -- unless it has 2048 frames or more, see below --, and those give a line the same bits in any minibatch; but from 2048
  // frames per call on (64 lines of 32) the library would pick its fused forward launch, whose producer / consumer items sum in
  // another order (outputs differ in the last bit, ~4e-7).  So the batched calls keep the per-line family (overlap mode 0 for the
  // call; the mode the net had is read and put back): clstmocr batch=N prints what batch=1 prints, byte for byte.
  // Two limits.  (1) A single line of >= 2048 frames takes the fused launch in predict() (the library's rule admits one line) and
  // the per-line kernels here: for such a line batch=1 and batch=N agree to the last bit but one, not byte for byte.  (2) From 640
  // lines per call on the library's batched MFMA recurrence takes over (f16 split products, 1e-4 class: same text on trained
  // models, not the same bits); CLSTM_DEBUG="fwd_mfma=0" keeps the per-line kernels there too.
  vector<int> batch_T;   // line lengths of the last predict_frames() / predict_batch_gpu() minibatch (get_outputs_batch)
  void predict_frames(const vector<const Image*>& lines, vector<ustring>& out, vector<vector<CharPrediction>>* preds = nullptr) {
    out.clear();
    if (preds) preds->clear();
    if (lines.empty()) return;
    batch_T.clear();
    vector<float> frames;
    for (const Image* l : lines) { batch_T.push_back(l->w); frames.insert(frames.end(), l->d.begin(), l->d.end()); }
    predict_packed(frames.data(), true, out, preds);
  }
  // one clstm_net_predict_h (frames on the host) / clstm_net_predict (frames on the device) call on the lines of batch_T
  void predict_packed(const float* frames, bool on_host, vector<ustring>& out, vector<vector<CharPrediction>>* preds) {
    const int bs = (int)batch_T.size();
    int N = 0;
    for (int t : batch_T) N += t;
    vector<int> cls(N), loc(N), cnt(bs);
    vector<float> conf(preds ? N : 0);
    int train_overlap = 1;
    chk(clstm_net_get_overlap(net, &train_overlap), "clstm_net_get_overlap");
    chk(clstm_net_set_overlap(net, 0), "clstm_net_set_overlap");
    const int rc = on_host ? clstm_net_predict_h(net, batch_T.data(), bs, frames, cls.data(), loc.data(), preds ? conf.data() : nullptr, cnt.data())
                           : clstm_net_predict(net, batch_T.data(), bs, frames, cls.data(), loc.data(), preds ? conf.data() : nullptr, cnt.data());
    const string err = rc ? clstm_last_error() : "";
    chk(clstm_net_set_overlap(net, train_overlap), "clstm_net_set_overlap");
    if (rc) fail(string(on_host ? "clstm_net_predict_h: " : "clstm_net_predict: ") + err);
    int o = 0;
    for (int b = 0; b < bs; b++) {
      out.push_back(codec.decode(Classes(cls.begin() + o, cls.begin() + o + cnt[b])));
      if (preds) {
        preds->emplace_back();
        for (int i = 0; i < cnt[b]; i++)
          preds->back().push_back(CharPrediction{i, loc[o + i], (char32_t)codec.codec[cls[o + i]], conf[o + i]});
      }
      o += batch_T[b];
    }
    T = batch_T.back();
  }
  // ---- raw line images normalised ON THE DEVICE (clstm_normalizer_*: the frames are the host normaliser's, bit for bit).  Main
  // thread only: the call goes to the library's stream, which is per thread.
  // measure + normalize of `raws` in one call; T: frames per line, *frames_d: DEVICE [sum T][target_height], valid until the next call
  // keys / visits (with set_degrade; one of each per line): the lines are degraded first, in the same call sequence -- line b with the
  // parameters clstm_degrade_draw gives (degrade_seed, keys[b], visits[b]) -- and the normaliser reads the degraded pixels where the
  // degrader left them, on the device
  void normalize_device(const vector<const Image*>& raws, vector<int>& T_out, float** frames_d, const vector<unsigned long long>* keys = nullptr,
                        const vector<unsigned long long>* visits = nullptr) {
    if (!gpu_normalizer)
      chk(clstm_normalizer_create(&gpu_normalizer, target_height, normalizer.smooth2d, normalizer.smooth1d, normalizer.range), "clstm_normalizer_create");
    vector<int> w, h;
    vector<float> pix;
    for (const Image* r : raws) { w.push_back(r->w); h.push_back(r->h); pix.insert(pix.end(), r->d.begin(), r->d.end()); }
    T_out.assign(raws.size(), 0);
    if (keys) {
      if (!gpu_degrader) fail("normalize_device: keys without set_degrade");
      if (!visits || keys->size() != raws.size() || visits->size() != raws.size()) fail("normalize_device: one key and one visit per line");
      vector<clstm_degrade_line> lines(raws.size());
      for (size_t b = 0; b < raws.size(); b++)
        chk(clstm_degrade_draw(degrade_seed, (*keys)[b], (*visits)[b], &degrade_ranges, w[b], h[b], &lines[b]), "clstm_degrade_draw");
      float* pix_d = nullptr;
      chk(clstm_degrader_run_h(gpu_degrader, pix.data(), w.data(), h.data(), (int)raws.size(), lines.data(), &pix_d), "clstm_degrader_run_h");
      chk(clstm_normalizer_run_d(gpu_normalizer, pix_d, w.data(), h.data(), (int)raws.size(), T_out.data(), nullptr, frames_d), "clstm_normalizer_run_d");
      return;
    }
    chk(clstm_normalizer_run_h(gpu_normalizer, pix.data(), w.data(), h.data(), (int)raws.size(), T_out.data(), nullptr, frames_d), "clstm_normalizer_run_h");
  }
  // the same with the frames read back once into one Image per line (what a dataset cache keeps)
  void normalize_batch_gpu(const vector<const Image*>& raws, vector<Image*>& frames, const vector<unsigned long long>* keys = nullptr,
                           const vector<unsigned long long>* visits = nullptr) {
    if (raws.empty()) return;
    vector<int> Ts;
    float* frames_d = nullptr;
    normalize_device(raws, Ts, &frames_d, keys, visits);
    size_t N = 0;
    for (int t : Ts) N += t;
    vector<float> all(N * target_height);
    chk(clstm_normalizer_get_frames_h(gpu_normalizer, all.data()), "clstm_normalizer_get_frames_h");
    size_t o = 0;
    for (size_t b = 0; b < raws.size(); b++) {
      frames[b]->resize(Ts[b], target_height);
      std::copy(all.begin() + o, all.begin() + o + (size_t)Ts[b] * target_height, frames[b]->d.begin());
      o += (size_t)Ts[b] * target_height;
    }
  }
  // predict_batch with the normaliser on the device: pack the raw images, clstm_normalizer_run_h, clstm_net_predict on the frames
  // where they lie.  Same overlap-mode bracket as predict_frames, so results do not depend on `batch`.
  void predict_batch_gpu(const vector<const Image*>& raws, vector<ustring>& out, vector<vector<CharPrediction>>* preds = nullptr) {
    out.clear();
    if (preds) preds->clear();
    if (raws.empty()) return;
    float* frames_d = nullptr;
    normalize_device(raws, batch_T, &frames_d);
    predict_packed(frames_d, false, out, preds);
  }
  void predict_batch(const vector<Image>& raws, vector<ustring>& out, vector<vector<CharPrediction>>* preds = nullptr) {
    vector<Image> frames(raws.size());
    vector<const Image*> ptrs;
    for (size_t b = 0; b < raws.size(); b++) { normalize_line(frames[b], raws[b]); ptrs.push_back(&frames[b]); }
    predict_frames(ptrs, out, preds);
  }
  // ---- scores and forced alignments of known transcripts (clstm_net_score: the reference's forward_algorithm, ctc.cc:24-40, and its
  // max-plus twin with a back-trace; include/clstm_abi.h states the semantics).  score_current works on the net's CURRENT
  // minibatch, one transcript per line -- the lines of the last predict_frames() / predict_batch_gpu() (Ts = batch_T) or the line of
  // the last predict() (Ts = {T}); either result may be null.  lines (optional): the line of each transcript, for several candidates
  // per line or transcripts for some of the lines only.
  void score_current(const vector<int>& Ts, const vector<ustring>& transcripts, vector<float>* scores, vector<vector<CharSpan>>* spans,
                     const vector<int>* lines = nullptr) {
    const int n = (int)transcripts.size();
    if (n != (int)(lines ? lines->size() : Ts.size())) fail("score: one transcript per line expected");
    if (n == 0) return;
    vector<int> Tc;   // frames of each candidate's line
    for (int c = 0; c < n; c++) {
      const int b = lines ? (*lines)[c] : c;
      if (b < 0 || b >= (int)Ts.size()) fail("score: no such line");
      Tc.push_back(Ts[b]);
    }
    Classes labels, one;
    vector<int> L;
    for (const ustring& t : transcripts) {
      codec.encode(one, t);
      L.push_back((int)one.size());
      labels.insert(labels.end(), one.begin(), one.end());
    }
    Classes dummy(1, 1);
    size_t N = 0;
    for (int t : Tc) N += t;
    vector<int> path(spans ? std::max<size_t>(N, 1) : 0);
    if (scores) scores->assign(n, 0.0f);
    chk(clstm_net_score(net, labels.empty() ? dummy.data() : labels.data(), L.data(), lines ? lines->data() : nullptr, n, scores ? scores->data() : nullptr,
                        nullptr, spans ? path.data() : nullptr), "clstm_net_score");
    if (!spans) return;
    spans->assign(n, vector<CharSpan>());
    size_t o = 0;
    for (int b = 0; b < n; b++) {
      vector<CharSpan>& sp = (*spans)[b];
      for (int k = 0; k < L[b]; k++) sp.push_back(CharSpan{k, -1, -1, transcripts[b][k]});
      for (int t = 0; t < Tc[b]; t++) {
        const int st = path[o + t];
        if (st < 0 || st % 2 == 0) continue;   // a late start's prefix / a blank state; label k is state 2 k + 1
        CharSpan& c = sp[st / 2];
        if (c.x0 < 0) c.x0 = t;
        c.x1 = t;
      }
      o += Tc[b];
    }
  }
  // normalised lines (the frames path of predict_frames) against one transcript each
  void score(const vector<const Image*>& lines, const vector<ustring>& transcripts, vector<float>& scores) {
    vector<ustring> texts;
    predict_frames(lines, texts);
    score_current(batch_T, transcripts, &scores, nullptr);
  }
  void align(const vector<const Image*>& lines, const vector<ustring>& transcripts, vector<vector<CharSpan>>& spans) {
    vector<ustring> texts;
    predict_frames(lines, texts);
    score_current(batch_T, transcripts, nullptr, &spans);
  }
  // ---- errors of the CURRENT minibatch against ground truths, counted on the device (clstm_net_errors: Levenshtein distance of every
  // line's trivial_decode, the canonical script's substitutions / insertions / deletions, the confusion table; include/clstm_abi.h).
  // One transcript per line of Ts, as score_current without `lines`.  A character the codec does not hold becomes label nclasses, which
  // matches no output: the distance is levenshtein(predicted text, ground truth)'s.  Any result may be null.  counts: 3 per line;
  // confusion: (nclasses + 1)^2, [reference label][output label], row / column 0 = insertions / deletions.
  Classes encode_lenient(const ustring& s) const {
    Classes cs;
    for (char32_t ch : s) {
      auto it = codec.encoder.find((int)ch);
      cs.push_back(it == codec.encoder.end() || it->second == 0 ? nclasses : it->second);
    }
    return cs;
  }
  void errors_current(const vector<int>& Ts, const vector<ustring>& transcripts, vector<int>* dist, vector<int>* counts, vector<int>* confusion) {
    const int n = (int)transcripts.size();
    if (n != (int)Ts.size()) fail("errors: one transcript per line expected");
    if (dist) dist->assign(n, 0);
    if (counts) counts->assign((size_t)3 * n, 0);
    if (confusion) confusion->assign((size_t)(nclasses + 1) * (nclasses + 1), 0);
    if (n == 0 || (!dist && !counts && !confusion)) return;
    Classes labels;
    vector<int> L;
    for (const ustring& t : transcripts) {
      const Classes one = encode_lenient(t);
      L.push_back((int)one.size());
      labels.insert(labels.end(), one.begin(), one.end());
    }
    Classes dummy(1, 1);
    chk(clstm_net_errors(net, labels.empty() ? dummy.data() : labels.data(), L.data(), dist ? dist->data() : nullptr,
                         counts ? counts->data() : nullptr, confusion ? confusion->data() : nullptr), "clstm_net_errors");
  }
  // the same figures for texts the host already holds (clstm_edit_distance_batch): text k against transcript k
  void errors_texts(const vector<ustring>& texts, const vector<ustring>& transcripts, vector<int>* dist, vector<int>* counts, vector<int>* confusion) {
    const int n = (int)transcripts.size();
    if (n != (int)texts.size()) fail("errors: one transcript per text expected");
    if (dist) dist->assign(n, 0);
    if (counts) counts->assign((size_t)3 * n, 0);
    if (confusion) confusion->assign((size_t)(nclasses + 1) * (nclasses + 1), 0);
    if (n == 0 || (!dist && !counts && !confusion)) return;
    Classes hyp(1, 1), ref(1, 1);   // (never empty arrays)
    vector<int> hoff(1, 0), roff(1, 0);
    for (int k = 0; k < n; k++) {
      const Classes h = encode_lenient(texts[k]), r = encode_lenient(transcripts[k]);
      hyp.insert(hyp.end(), h.begin(), h.end());
      ref.insert(ref.end(), r.begin(), r.end());
      hoff.push_back((int)hyp.size() - 1);
      roff.push_back((int)ref.size() - 1);
    }
    chk(clstm_edit_distance_batch(hyp.data() + 1, hoff.data(), n, ref.data() + 1, roff.data(), n, nullptr, nclasses + 1, dist ? dist->data() : nullptr,
                                  counts ? counts->data() : nullptr, nullptr, nullptr, confusion ? confusion->data() : nullptr),
        "clstm_edit_distance_batch");
  }
  // best-of-n ("oracle") distance: per line with a ground truth (gt_line[k] names the line of gts[k]) the smallest distance among the
  // line's hypotheses and which one has it (-1: the line has none) -- one clstm_edit_distance_batch call in its ref_of form
  void oracle_distance(const vector<vector<Hypothesis>>& hyps, const vector<ustring>& gts, const vector<int>& gt_line, vector<int>& best,
                       vector<int>& best_k) {
    best.assign(gts.size(), 0);
    best_k.assign(gts.size(), -1);
    Classes hyp, ref;
    vector<int> hoff(1, 0), roff(1, 0), ref_of, first;
    for (size_t k = 0; k < gts.size(); k++) {
      const Classes r = encode_lenient(gts[k]);
      ref.insert(ref.end(), r.begin(), r.end());
      roff.push_back((int)ref.size());
      first.push_back((int)ref_of.size());
      for (const Hypothesis& h : hyps[gt_line[k]]) {
        const Classes c = encode_lenient(h.text);
        hyp.insert(hyp.end(), c.begin(), c.end());
        hoff.push_back((int)hyp.size());
        ref_of.push_back((int)k);
      }
    }
    first.push_back((int)ref_of.size());
    if (ref_of.empty()) return;
    vector<int> dist(ref_of.size());
    Classes dummy(1, 1);
    chk(clstm_edit_distance_batch(hyp.empty() ? dummy.data() : hyp.data(), hoff.data(), (int)ref_of.size(), ref.empty() ? dummy.data() : ref.data(),
                                  roff.data(), (int)gts.size(), ref_of.data(), nclasses + 1, dist.data(), nullptr, nullptr, nullptr, nullptr),
        "clstm_edit_distance_batch");
    for (size_t k = 0; k < gts.size(); k++)
      for (int i = first[k]; i < first[k + 1]; i++)
        if (best_k[k] < 0 || dist[i] < best[k]) { best[k] = dist[i]; best_k[k] = i - first[k]; }
  }
  // ---- n-best transcripts (clstm_net_beam: CTC prefix beam search on the device, include/clstm_abi.h).  nbest_current works on the
  // net's CURRENT minibatch as score_current does; per line up to nbest hypotheses, best first.  A score is the log-probability the
  // beam gathered for the text -- not on the scale of score().
  // set_lm: a character n-gram model (charlm.h; written by clstmlm or clstm_amd.lm.CharLM.save) for the model's classes; from then
  // on predict_nbest / nbest_current search with it inside the beam (weight >= 0, bonus per character) and a Hypothesis carries both
  // scores.  An empty path takes the model away again.
  void set_lm(const string& path, float weight, float bonus) {
    if (lm) chk(clstm_charlm_destroy(lm), "clstm_charlm_destroy");
    lm = nullptr;
    if (path.empty()) return;
    const CharLMTables m = CharLMTables::load(path);
    if (m.nc != nclasses) fail(path + ": the language model has " + std::to_string(m.nc) + " classes, the network " + std::to_string(nclasses));
    chk(clstm_charlm_create(&lm, m.order, m.nc, m.table.data(), m.has_end ? m.end.data() : nullptr), "clstm_charlm_create");
    lm_weight = weight; lm_bonus = bonus;
  }
  // set_lexicon: a UTF-8 word list, one word per line (lexicon.h), encoded through the model's codec; from then on predict_nbest /
  // nbest_current report only transcripts whose every run of word characters is a word of the list (a line on which no such
  // transcript survived has no hypotheses).  word_chars (UTF-8, or null: a class is a word character iff it occurs in a kept word)
  // names the word characters; every other class is a separator.  Works with and without set_lm; without a model the score is the
  // acoustic one plus lm_bonus per character.  An empty path takes the lexicon away again.
  void set_lexicon(const string& path, const string* word_chars = nullptr) {
    if (lexicon) chk(clstm_lexicon_destroy(lexicon), "clstm_lexicon_destroy");
    lexicon = nullptr;
    lexicon_words = lexicon_dropped = 0;
    if (path.empty()) return;
    const WordList wl = WordList::load(path, codec.encoder, nclasses, word_chars);
    vector<int> flat, off;
    wl.pack(flat, off);
    chk(clstm_lexicon_create(&lexicon, nclasses, wl.word_class.data(), flat.data(), off.data(), (int)wl.words.size()), "clstm_lexicon_create");
    long long info[4];
    chk(clstm_lexicon_info(lexicon, info), "clstm_lexicon_info");
    lexicon_words = info[0]; lexicon_dropped = wl.dropped();
  }
  // use_lexicon = false: the search without the lexicon although one is set (what a caller shows for a line the lexicon left empty)
  void nbest_current(const vector<int>& Ts, int beam, int nbest, vector<vector<Hypothesis>>& out, bool use_lexicon = true) {
    const int bs = (int)Ts.size();
    out.assign(bs, vector<Hypothesis>());
    if (bs == 0) return;
    size_t N = 0;
    for (int t : Ts) N += t;
    vector<int> nhyp(bs), len((size_t)bs * nbest), labels(std::max<size_t>(N * nbest, 1));
    vector<float> sc((size_t)bs * nbest), am((size_t)bs * nbest);
    if (lexicon && use_lexicon)
      chk(clstm_net_beam_lex(net, beam, nbest, lexicon, lm, lm ? lm_weight : 0.0f, lm_bonus, nhyp.data(), len.data(), sc.data(), am.data(), labels.data()),
          "clstm_net_beam_lex");
    else if (lm) chk(clstm_net_beam_lm(net, beam, nbest, lm, lm_weight, lm_bonus, nhyp.data(), len.data(), sc.data(), am.data(), labels.data()), "clstm_net_beam_lm");
    else {
      chk(clstm_net_beam(net, beam, nbest, nhyp.data(), len.data(), sc.data(), labels.data()), "clstm_net_beam");
      am = sc;
    }
    size_t off = 0;
    for (int b = 0; b < bs; b++) {
      for (int k = 0; k < nhyp[b]; k++) {
        const int* l = labels.data() + (size_t)nbest * off + (size_t)k * Ts[b];
        out[b].push_back(Hypothesis{codec.decode(Classes(l, l + len[(size_t)b * nbest + k])), sc[(size_t)b * nbest + k], am[(size_t)b * nbest + k]});
      }
      off += Ts[b];
    }
  }
  // predict_frames (normalised lines) or, with gpu_prep, predict_batch_gpu (raw lines), then the n best of every line
  void predict_nbest(const vector<const Image*>& lines, int beam, int nbest, vector<ustring>& out, vector<vector<Hypothesis>>& hyps,
                     vector<vector<CharPrediction>>* preds = nullptr, bool gpu_prep = false) {
    hyps.clear();
    if (gpu_prep) predict_batch_gpu(lines, out, preds);
    else predict_frames(lines, out, preds);
    if (!lines.empty()) nbest_current(batch_T, beam, nbest, hyps);
  }
  void get_outputs_batch(vector<Image>& outs) {   // [T_b][nclasses] of every line of the last predict_frames() minibatch
    int N = 0;
    for (int t : batch_T) N += t;
    vector<float> z((size_t)N * nclasses);
    chk(clstm_net_get_outputs_h(net, z.data()), "clstm_net_get_outputs_h");
    outs.resize(batch_T.size());
    size_t o = 0;
    for (size_t b = 0; b < batch_T.size(); b++) {
      outs[b].resize(batch_T[b], nclasses);
      std::copy(z.begin() + o, z.begin() + o + (size_t)batch_T[b] * nclasses, outs[b].d.begin());
      o += (size_t)batch_T[b] * nclasses;
    }
  }
};

// CLSTMText (clstmhl.h:24-144): text in, text out through the same BiLSTM + CTC path; characters are
// one-hot frames separated by `neps` all-zero frames (setInputs, clstmhl.h:83-100).
struct CLSTMText {
  Model model;
  Codec codec, icodec;
  clstm_net* net = nullptr;
  int nclasses = -1, iclasses = -1;
  int neps = 3;  // the reference never overrides it: maybe_load() shadows the member (clstmhl.h:53)
  vector<float> frames, aligned;
  int T = 0;
  ~CLSTMText() { if (net) clstm_net_destroy(net); }
  void attach() {
    if (net) { clstm_net_destroy(net); net = nullptr; }
    chk(clstm_net_create(&net, &model.desc, nullptr, nullptr, nullptr), "clstm_net_create");
    chk(clstm_net_set_params_h(net, model.params.data()), "clstm_net_set_params_h");
    nclasses = model.desc.nclasses;
    iclasses = model.desc.ninput;
    codec.set(model.codec);
    icodec.set(model.icodec);
    auto get = [&](const char* k, const char* d) { auto it = model.attr.find(k); return it == model.attr.end() ? string(d) : it->second; };
    chk(clstm_net_set_learning_rate(net, atof(get("learning_rate", "1e-4").c_str()), atof(get("momentum", "0.9").c_str())),
        "clstm_net_set_learning_rate");
  }
  void setLearningRate(float lr, float mom) {
    model.attr["learning_rate"] = std::to_string((double)lr);
    model.attr["momentum"] = std::to_string((double)mom);
    if (net) chk(clstm_net_set_learning_rate(net, lr, mom), "clstm_net_set_learning_rate");
  }
  void createBidi(const vector<int>& icodec_, const vector<int>& codec_, int nhidden) {  // clstmhl.h:70-82
    LCG lcg;
    model.create("bidi", (int)icodec_.size(), (int)codec_.size(), nhidden, 0, lcg);
    model.attr["neps"] = std::to_string(neps);
    model.icodec = icodec_;
    model.codec = codec_;
    attach();
  }
  void load(const string& fname) { model.load(fname); attach(); }
  void save(const string& fname) {
    chk(clstm_net_get_params_h(net, model.params.data()), "clstm_net_get_params_h");
    model.save(fname);
  }
  void setInputs(const ustring& s) {
    Classes cs;
    icodec.encode(cs, s);
    T = (int)cs.size() * (neps + 1) + neps;
    frames.assign((size_t)T * iclasses, 0.0f);
    int index = neps;
    for (int c : cs) {
      frames[(size_t)index * iclasses + c] = 1.0f;
      index += neps + 1;
    }
    chk(clstm_net_set_batch(net, &T, 1), "clstm_net_set_batch");
    chk(clstm_net_set_inputs_h(net, frames.data()), "clstm_net_set_inputs_h");
  }
  ustring decode_outputs() {
    vector<int> cls(T), loc(T);
    int cnt = 0;
    chk(clstm_net_decode(net, cls.data(), loc.data(), &cnt), "clstm_net_decode");
    cls.resize(cnt);
    return codec.decode(cls);
  }
  ustring train(const ustring& in, const ustring& target) {  // clstmhl.h:103-117
    setInputs(in);
    chk(clstm_net_forward(net), "clstm_net_forward");
    Classes transcript;
    codec.encode(transcript, target);
    const int L = (int)transcript.size();
    aligned.resize((size_t)T * nclasses);
    chk(clstm_net_ctc(net, transcript.data(), &L, aligned.data()), "clstm_net_ctc");
    chk(clstm_net_backward(net), "clstm_net_backward");
    ustring out = decode_outputs();   // decode before the update, as the reference's outputs are
    chk(clstm_net_update(net), "clstm_net_update");
    return out;
  }
  ustring predict(const ustring& in) {
    setInputs(in);
    InferenceScope inference(net);
    chk(clstm_net_forward(net), "clstm_net_forward");
    return decode_outputs();
  }
  string predict_utf8(const string& in) { return utf32_to_utf8(predict(utf8_to_utf32(in))); }
  string aligned_utf8() {
    Classes cs;
    trivial_decode_host(cs, aligned.data(), T, nclasses);
    return utf32_to_utf8(codec.decode(cs));
  }
};

}  // namespace clstmhost
