// abi.inc -- part of clstm_hip.hip: the extern "C" entry points of include/clstm_abi.h (per-op, CTC, fused network, one-call
// training step, communicator, debug hooks): argument checks and the call into net.inc / ctc_run.inc / step.inc -- the step sequence and
// its launches are step.inc's.  Included once by clstm_hip.hip behind the namespace.
using namespace clstm;
struct clstm_net {
  // bytes held by the grow-only buffers of the members below (runtime.inc: AcctScope).  Declared first = destroyed last: the buffers
  // report their release to it
  std::unique_ptr<size_t> dev_bytes;
  Net net;
  CtcWorkspace ctc;
  DecodeWorkspace dec;
  ScoreWorkspace score;
  BeamWorkspace beam;
  EditWorkspace edit;
};

#define EW(kernel, len, ...) \
  CLSTM_LAUNCH(kernel, dim3(nblocks(len)), dim3(256), 0, g_stream, __VA_ARGS__); check_launch();

// a net-level query entry's roctx range with its timing bracket on g_stream, both ended on every exit path
struct QueryScope {
  RoctxRange range;
  Timing& timing;
  bool timed = false;
  QueryScope(Net& n, const char* range_name, const char* bracket = nullptr) : range(range_name), timing(n.timing) { if (bracket) time(bracket); }
  void time(const char* bracket) { timing.begin(bracket, g_stream); timed = true; }   // (the launches from here on)
  ~QueryScope() { if (timed) timing.end(g_stream); }
};
// What a per-minibatch entry point needs of the net is ONE line at its top: Net::require(needs, name) (net.inc; the table: include/clstm_abi.h).
struct clstm_charlm { CharLm lm; };
struct clstm_lexicon { Lexicon lex; };
struct clstm_normalizer {
  std::unique_ptr<size_t> dev_bytes;   // (declared first = destroyed last, as in clstm_net)
  Normalizer nz;
};
struct clstm_degrader {
  std::unique_ptr<size_t> dev_bytes;
  Degrader dg;
};
extern "C" {

const char* clstm_last_error(void) { return g_err.c_str(); }
int clstm_abi_version(void) { return 1; }
int clstm_set_stream(void* s) { g_stream = (hipStream_t)s; return 0; }
int clstm_synchronize(void) { ABI_BEGIN HIPCHECK(hipStreamSynchronize(g_stream)); check_device_errors(); ABI_END }

// ---- per-op entry points -------------------------------------------------------------------------
int clstm_forward_nonlin0(float* y, int len, int nl) { ABI_BEGIN EW(k_forward_nonlin0, len, y, (size_t)len, nl) ABI_END }
int clstm_backward_nonlin0(const float* yv, float* yd, int len, int nl) { ABI_BEGIN EW(k_backward_nonlin0, len, yv, yd, (size_t)len, nl) ABI_END }
int clstm_forward_nonlin(float* y, const float* x, int len, int nl) { ABI_BEGIN EW(k_forward_nonlin, len, y, x, (size_t)len, nl) ABI_END }
int clstm_backward_nonlin(const float* yv, const float* yd, float* xd, int len, int nl) { ABI_BEGIN EW(k_backward_nonlin, len, yv, yd, xd, (size_t)len, nl) ABI_END }
int clstm_forward_lin1(float* y, const float* W, const float* x, int n, int m, int bs) {
  ABI_BEGIN EW(k_forward_lin1, (size_t)n * bs, y, W, x, n, m, bs, -1) ABI_END
}
int clstm_backward_lin1(const float* yd, const float* W, float* Wd, const float* x, float* xd, int n, int m, int bs) {
  ABI_BEGIN
  EW(k_backward_lin1_dx, (size_t)(m - 1) * bs, yd, W, xd, n, m, bs, 0)
  EW(k_backward_lin1_dw, (size_t)n * m, yd, Wd, x, n, m, bs)
  ABI_END
}
int clstm_forward_full1(float* y, const float* W, const float* x, int n, int m, int bs, int nl) {
  ABI_BEGIN
  REQUIRE(nl >= 0 && nl <= 4, "bad nonlinearity code (clstm_compute.cc:147 aborts)");
  EW(k_forward_lin1, (size_t)n * bs, y, W, x, n, m, bs, nl)
  ABI_END
}
int clstm_backward_full1(const float* yv, float* yd, const float* W, float* Wd, const float* x, float* xd,
                         int n, int m, int bs, int nl) {
  ABI_BEGIN
  REQUIRE(nl >= 0 && nl <= 4, "bad nonlinearity code");
  EW(k_backward_nonlin0, (size_t)n * bs, yv, yd, (size_t)n * bs, nl)
  EW(k_backward_lin1_dx, (size_t)(m - 1) * bs, (const float*)yd, W, xd, n, m, bs, 0)
  EW(k_backward_lin1_dw, (size_t)n * m, (const float*)yd, Wd, x, n, m, bs)
  ABI_END
}
int clstm_forward_softmax(float* z, const float* W, const float* x, int n, int m, int bs) {
  ABI_BEGIN
  REQUIRE(n >= 2, "Softmax requires n>=2 (clstm_compute.cc:328)");
  EW(k_forward_lin1, (size_t)n * bs, z, W, x, n, m, bs, -1)
  CLSTM_LAUNCH(k_softmax_norm, dim3((bs + 3) / 4), dim3(256), 0, g_stream, z, n, (size_t)bs, (int*)nullptr, 0);
  check_launch();
  ABI_END
}
int clstm_backward_softmax(const float* zd, const float* W, float* Wd, const float* x, float* xd, int n, int m, int bs) {
  ABI_BEGIN
  EW(k_backward_lin1_dx, (size_t)(m - 1) * bs, zd, W, xd, n, m, bs, 1)
  EW(k_backward_lin1_dw, (size_t)n * m, zd, Wd, x, n, m, bs)
  ABI_END
}
int clstm_forward_stack(float* z, const float* x, const float* y, int nx, int ny, int bs) {
  ABI_BEGIN REQUIRE(y != nullptr, "null operand"); EW(k_stack, (size_t)(nx + ny) * bs, z, x, y, nx, ny, bs) ABI_END
}
int clstm_backward_stack(const float* zd, float* xd, float* yd, int nx, int ny, int bs) {
  ABI_BEGIN REQUIRE(yd != nullptr, "null operand"); EW(k_unstack_add, (size_t)(nx + ny) * bs, zd, xd, yd, nx, ny, bs) ABI_END
}
int clstm_forward_stack_delay(float* z, const float* x, const float* ylast, int nx, int ny, int bs) {
  ABI_BEGIN EW(k_stack, (size_t)(nx + ny) * bs, z, x, ylast, nx, ny, bs) ABI_END
}
int clstm_backward_stack_delay(const float* zd, float* xd, float* ylastd, int nx, int ny, int bs) {
  ABI_BEGIN EW(k_unstack_add, (size_t)(nx + ny) * bs, zd, xd, ylastd, nx, ny, bs) ABI_END
}
int clstm_forward_reverse(float* y, const float* x, int rows, int bs, int N) {
  ABI_BEGIN EW(k_forward_reverse, (size_t)rows * bs * 2 * N, y, x, (size_t)rows * bs * 2, N) ABI_END
}
int clstm_backward_reverse(const float* y, float* x, int rows, int bs, int N) {
  ABI_BEGIN EW(k_backward_reverse, (size_t)rows * bs * N, y, x, (size_t)rows * bs, N) ABI_END
}
int clstm_forward_btswitch(float* y, const float* x, int rows, int bs, int N) {
  ABI_BEGIN EW(k_forward_btswitch, (size_t)rows * bs * N, y, x, rows, bs, N) ABI_END
}
int clstm_backward_btswitch(const float* y, float* x, int rows, int bs, int N) {
  ABI_BEGIN EW(k_backward_btswitch, (size_t)rows * bs * N, y, x, rows, bs, N) ABI_END
}
int clstm_forward_batchstack(float* y, const float* x, int d, int bs, int N, int pre, int post) {
  ABI_BEGIN
  REQUIRE(pre >= 0 && post >= 0, "batchstack: negative pre/post");
  EW(k_forward_batchstack, (size_t)(pre + post + 1) * d * bs * 2 * N, y, x, d, bs, N, pre, post)
  ABI_END
}
int clstm_backward_batchstack(const float* y, float* x, int d, int bs, int N, int pre, int post) {
  ABI_BEGIN
  REQUIRE(pre >= 0 && post >= 0, "batchstack: negative pre/post");
  EW(k_backward_batchstack, (size_t)d * bs * N, y, x, d, bs, N, pre, post)
  ABI_END
}
int clstm_forward_statemem(float* st, const float* ci, const float* gi, const float* last, const float* gf, int len) {
  ABI_BEGIN EW(k_forward_statemem, len, st, ci, gi, last, gf, (size_t)len) ABI_END
}
int clstm_backward_statemem(const float* sd, const float* ci, float* cid, const float* gi, float* gid,
                            const float* last, float* lastd, const float* gf, float* gfd, int len) {
  ABI_BEGIN EW(k_backward_statemem, len, sd, ci, cid, gi, gid, last, lastd, gf, gfd, (size_t)len) ABI_END
}
int clstm_forward_nonlingate(float* out, const float* st, const float* go, int len, int nl) {
  ABI_BEGIN EW(k_forward_nonlingate, len, out, st, go, (size_t)len, nl) ABI_END
}
int clstm_backward_nonlingate(const float* outd, const float* st, float* std_, const float* go, float* god, int len, int nl) {
  ABI_BEGIN EW(k_backward_nonlingate, len, outd, st, std_, go, god, (size_t)len, nl) ABI_END
}
int clstm_clip_gradient(float* d, int len, float clip) {
  ABI_BEGIN
  if (clip >= 1e6f) return 0;  // clstm_compute.cc:554
  REQUIRE(clip > 0, "clip must be positive (clstm_compute.cc:555)");
  EW(k_clip, len, d, (size_t)len, clip)
  ABI_END
}
int clstm_sgd_update(float* v, float* d, int len, float lr, float mom) { ABI_BEGIN EW(k_sgd, len, v, d, (size_t)len, lr, mom) ABI_END }

// ---- CTC ------------------------------------------------------------------------------------------
int clstm_mktargets(int* states_h, const int* transcript_h, int L) {
  for (int t = 0; t < 2 * L + 1; t++) states_h[t] = (t % 2 == 1) ? transcript_h[(t - 1) / 2] : 0;
  return 0;
}
int clstm_ctc_align_batch(const float* probs, float* deltas, float* aligned, int nc, const int* line_off_h,
                          const int* states_h, const int* state_off_h, int bs) {
  ABI_BEGIN
  run_ctc(thread_workspace<CtcWorkspace>(), probs, deltas, aligned, nc, line_off_h, states_h, state_off_h, bs, g_stream);
  ABI_END
}
int clstm_ctc_score_batch(const float* probs, int nc, const int* line_off_h, int bs, const int* states_h, const int* state_off_h,
                          const int* cand_line_h, int ncand, float* score_h, float* vscore_h, int* path_h) {
  ABI_BEGIN
  run_ctc_score(thread_workspace<ScoreWorkspace>(), probs, nc, line_off_h, bs, states_h, state_off_h, cand_line_h, ncand, score_h, vscore_h, path_h, g_stream);
  ABI_END
}
int clstm_ctc_beam_batch(const float* probs, int nc, const int* line_off_h, int bs, int beam, int nbest, int* nhyp_h, int* len_h,
                         float* score_h, int* labels_h) {
  ABI_BEGIN
  run_ctc_beam(thread_workspace<BeamWorkspace>(), probs, nc, line_off_h, bs, beam, nbest, nhyp_h, len_h, score_h, labels_h, g_stream);
  ABI_END
}
int clstm_charlm_create(clstm_charlm** out, int order, int nc, const float* table_h, const float* end_h) {
  ABI_BEGIN
  REQUIRE(out && table_h, "null argument");
  REQUIRE(order == 2 || order == 3, "clstm_charlm_create: order must be 2 or 3");
  REQUIRE(nc >= 2, "clstm_charlm_create: the class count must be at least 2");
  long long nctx = 1;
  for (int k = 1; k < order; k++) nctx *= nc;   // (nc < 2^31: no overflow for order <= 3)
  REQUIRE(nctx * nc <= (1ll << 26), "clstm_charlm_create: the table exceeds 2^26 floats");
  for (long long i = 0; i < nctx * nc; i++) REQUIRE(std::isfinite(table_h[i]), "clstm_charlm_create: a table entry is not finite");
  for (long long i = 0; end_h && i < nctx; i++) REQUIRE(std::isfinite(end_h[i]), "clstm_charlm_create: an end table entry is not finite");
  std::unique_ptr<clstm_charlm> h(new clstm_charlm());
  h->lm.order = order; h->lm.nc = nc; h->lm.nctx = nctx; h->lm.has_end = end_h != nullptr;
  h->lm.table.reserve((size_t)(nctx * nc));
  copy_h2d(h->lm.table.p, table_h, (size_t)(nctx * nc));
  if (end_h) {
    h->lm.end.reserve((size_t)nctx);
    copy_h2d(h->lm.end.p, end_h, (size_t)nctx);
  }
  *out = h.release();
  ABI_END
}
int clstm_charlm_destroy(clstm_charlm* lm) { ABI_BEGIN delete lm; ABI_END }
int clstm_ctc_beam_lm_batch(const float* probs, int nc, const int* line_off_h, int bs, int beam, int nbest, const clstm_charlm* lm,
                            float weight, float bonus, int* nhyp_h, int* len_h, float* score_h, float* am_score_h, int* labels_h) {
  ABI_BEGIN
  REQUIRE(lm, "clstm_ctc_beam_lm: the language model is required");
  const BeamLm with{&lm->lm, weight, bonus, am_score_h};
  run_ctc_beam(thread_workspace<BeamWorkspace>(), probs, nc, line_off_h, bs, beam, nbest, nhyp_h, len_h, score_h, labels_h, g_stream, &with);
  ABI_END
}
int clstm_lexicon_create(clstm_lexicon** out, int nc, const unsigned char* word_class_h, const int* words_h, const int* word_off_h, int nwords) {
  ABI_BEGIN
  REQUIRE(out, "clstm_lexicon_create: null argument");
  std::unique_ptr<clstm_lexicon> h(new clstm_lexicon());
  build_lexicon(h->lex, nc, word_class_h, words_h, word_off_h, nwords);   // (every refusal is here, before the upload)
  REQUIRE(h->lex.W == beam_lex_words(nc), "internal: the trie's row width is not the kernel's");
  h->lex.dev.reserve(h->lex.words.size());
  HIPCHECK(hipMemcpyAsync(h->lex.dev.p, h->lex.words.data(), h->lex.words.size() * sizeof(int), hipMemcpyHostToDevice, g_stream));
  HIPCHECK(hipStreamSynchronize(g_stream));
  *out = h.release();
  ABI_END
}
int clstm_lexicon_destroy(clstm_lexicon* lex) { ABI_BEGIN delete lex; ABI_END }
int clstm_lexicon_info(const clstm_lexicon* lex, long long info[4]) {
  ABI_BEGIN
  REQUIRE(lex && info, "clstm_lexicon_info: null argument");
  info[0] = lex->lex.nwords; info[1] = lex->lex.nnodes; info[2] = lex->lex.nedges;
  info[3] = (long long)(lex->lex.words.size() * sizeof(int));
  ABI_END
}
int clstm_lexicon_admits(const clstm_lexicon* lex, const int* labels_h, int L, int* out) {
  ABI_BEGIN
  REQUIRE(lex && out && L >= 0 && (labels_h || L == 0), "clstm_lexicon_admits: null argument or negative length");
  *out = lexicon_admits(lex->lex, labels_h, L);
  ABI_END
}
int clstm_ctc_beam_lex_batch(const float* probs, int nc, const int* line_off_h, int bs, int beam, int nbest, const clstm_lexicon* lex,
                             const clstm_charlm* lm, float weight, float bonus, int* nhyp_h, int* len_h, float* score_h,
                             float* am_score_h, int* labels_h) {
  ABI_BEGIN
  REQUIRE(lex, "clstm_ctc_beam_lex: the lexicon is required");
  const BeamLm with{lm ? &lm->lm : nullptr, weight, bonus, am_score_h};
  run_ctc_beam(thread_workspace<BeamWorkspace>(), probs, nc, line_off_h, bs, beam, nbest, nhyp_h, len_h, score_h, labels_h, g_stream, &with,
               &lex->lex);
  ABI_END
}
int clstm_edit_distance_batch(const int* hyp_h, const int* hyp_off_h, int npairs, const int* ref_h, const int* ref_off_h, int nref,
                              const int* ref_of_h, int nsym, int* dist_h, int* counts_h, int* nops_h, int* ops_h, int* confusion_h) {
  ABI_BEGIN
  edit_distance_batch(thread_workspace<EditWorkspace>(), hyp_h, hyp_off_h, npairs, ref_h, ref_off_h, nref, ref_of_h, nsym, dist_h, counts_h, nops_h, ops_h, confusion_h,
                      g_stream);
  ABI_END
}
int clstm_debug_edit_plan(int la, int lb, int want_script, int* plan) { ABI_BEGIN describe_edit_plan(la, lb, want_script, plan); ABI_END }
int clstm_trivial_decode_batch(const float* probs, int nc, const int* line_off_h, int bs, int* classes_h,
                               int* locs_h, int* counts_h) {
  ABI_BEGIN
  run_decode(thread_workspace<DecodeWorkspace>(), probs, nc, line_off_h, bs, classes_h, locs_h, counts_h, g_stream);
  ABI_END
}

// ---- fused network ----------------------------------------------------------------------------------
int clstm_net_nparams_for(const clstm_net_desc* ds) {
  long long total = 0;
  int ni = ds->ninput;
  const int nd = ds->unidirectional ? 1 : 2;
  for (int l = 0; l < ds->nlayers; l++) {
    const int no = ds->nhidden[l];
    total += (long long)nd * 4 * no * (ni + no + 1);
    ni = nd * no;
  }
  total += (long long)ds->nclasses * (ni + 1);
  return (int)total;
}
int clstm_net_create(clstm_net** out, const clstm_net_desc* ds, float* pv, float* pd, float* pg) {
  ABI_BEGIN
  REQUIRE(out && ds, "null argument");
  size_t* bytes = new size_t(0);
  AcctScope acct_(bytes);   // every DevBuf constructed from here to the end of build() reports to this net's counter
  clstm_net* h = nullptr;
  try { h = new clstm_net(); } catch (...) { delete bytes; throw; }
  h->dev_bytes.reset(bytes);
  try { h->net.build(*ds, pv, pd, pg); } catch (...) { delete h; throw; }
  *out = h;
  ABI_END
}
int clstm_net_destroy(clstm_net* h) { ABI_BEGIN delete h; ABI_END }
int clstm_net_nparams(clstm_net* h) { return h->net.nparams; }
int clstm_net_buffers(clstm_net* h, float** v, float** d, float** g) {
  if (v) *v = h->net.v;
  if (d) *d = h->net.d;
  if (g) *g = h->net.g;
  return 0;
}
int clstm_net_set_params_h(clstm_net* h, const float* p) { ABI_BEGIN copy_h2d(h->net.v, p, h->net.nparams); h->net.packed_dirty = true; h->net.params_epoch++; ABI_END }
int clstm_net_get_params_h(clstm_net* h, float* p) { ABI_BEGIN copy_d2h(p, h->net.v, h->net.nparams); ABI_END }
int clstm_net_set_derivs_h(clstm_net* h, const float* p) { ABI_BEGIN copy_h2d(h->net.d, p, h->net.nparams); ABI_END }
int clstm_net_get_derivs_h(clstm_net* h, float* p) { ABI_BEGIN copy_d2h(p, h->net.d, h->net.nparams); ABI_END }
int clstm_net_get_grads_h(clstm_net* h, float* p) { ABI_BEGIN copy_d2h(p, h->net.g, h->net.nparams); ABI_END }
int clstm_net_params_changed(clstm_net* h) { h->net.packed_dirty = true; h->net.params_epoch++; return 0; }
int clstm_net_set_learning_rate(clstm_net* h, float lr, float mom) { h->net.lr = lr; h->net.mom = mom; return 0; }
int clstm_net_set_gradient_clip(clstm_net* h, float c) {
  ABI_BEGIN REQUIRE(c > 0, "clip must be positive"); h->net.gclip = c; ABI_END
}
int clstm_net_set_batch(clstm_net* h, const int* T_h, int bs) { ABI_BEGIN h->net.set_batch(T_h, bs); ABI_END }
int clstm_net_set_inputs_h(clstm_net* h, const float* x) {
  ABI_BEGIN
  h->net.require(Net::NEED_BATCH, "clstm_net_set_inputs_h");
  h->net.next_adopted();   // (a declared next minibatch whose frames the caller replaces is not that minibatch any more)
  h->net.ensure_training_buffers();
  copy_h2d(h->net.X.p, x, (size_t)h->net.N * h->net.desc.ninput);
  h->net.frames_ingested(false);
  ABI_END
}
int clstm_net_set_inputs_d(clstm_net* h, const float* x) {
  ABI_BEGIN
  h->net.require(Net::NEED_BATCH, "clstm_net_set_inputs_d");
  h->net.next_adopted();
  net_ingest(h->net, h->ctc, x);
  ABI_END
}
// (after clstm_net_train_step_next: the declared minibatch becomes the current one -- its outputs are addressable, and a later step
//  call declares and ingests it again)
int clstm_net_forward(clstm_net* h) { ABI_BEGIN h->net.require(Net::NEED_BATCH, "clstm_net_forward"); h->net.next_adopted(); h->net.forward(); ABI_END }
int clstm_net_outputs(clstm_net* h, float** p, float** d) {
  if (p) *p = h->net.Z.p;
  if (d) *d = h->net.Dz.p;
  return 0;
}
int clstm_net_get_outputs_h(clstm_net* h, float* p) { ABI_BEGIN h->net.require(Net::NEED_OUTPUTS, "clstm_net_get_outputs_h"); copy_d2h(p, h->net.Z.p, (size_t)h->net.N * h->net.desc.nclasses); ABI_END }
int clstm_net_set_output_deltas_h(clstm_net* h, const float* p) { ABI_BEGIN h->net.require(Net::NEED_PASS, "clstm_net_set_output_deltas_h"); copy_h2d(h->net.Dz.p, p, (size_t)h->net.N * h->net.desc.nclasses); ABI_END }
int clstm_net_ctc(clstm_net* h, const int* labels_h, const int* L_h, float* aligned_h) {
  ABI_BEGIN
  h->net.require(Net::NEED_PASS, "clstm_net_ctc");
  net_ctc(h->net, h->ctc, Minibatch{nullptr, h->net.bs, nullptr, labels_h, L_h}, aligned_h);
  ABI_END
}
// score / forced alignment of candidate transcripts against the current minibatch: reads Z only (so it also follows clstm_net_predict),
// writes nothing of the net's -- no Dz, no error words, not the prepared alignment of a declared next minibatch (ScoreWorkspace)
int clstm_net_score(clstm_net* h, const int* labels_h, const int* L_h, const int* cand_line_h, int ncand, float* score_h,
                    float* vscore_h, int* path_h) {
  ABI_BEGIN
  REQUIRE(h, "null argument");
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_score");
  REQUIRE(score_h || vscore_h || path_h, "clstm_net_score: score_h, vscore_h and path_h are all NULL");
  REQUIRE(labels_h && L_h && ncand > 0, "null argument / no candidates");
  std::vector<int> soff, states;
  expand_transcripts(labels_h, L_h, ncand, states, soff);
  QueryScope scope_(n, "clstm:score", "ctc_score");
  run_ctc_score(h->score, n.Z.p, n.desc.nclasses, n.line_off_h.data(), n.bs, states.data(), soff.data(), cand_line_h, ncand,
                score_h, vscore_h, path_h, g_stream);
  ABI_END
}
// n-best transcripts of the current minibatch's lines: the guards and guarantees of clstm_net_score (reads Z only, BeamWorkspace)
int clstm_net_beam(clstm_net* h, int beam, int nbest, int* nhyp_h, int* len_h, float* score_h, int* labels_h) {
  ABI_BEGIN
  REQUIRE(h, "null argument");
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_beam");
  REQUIRE(nhyp_h && score_h, "clstm_net_beam: nhyp_h and score_h are required");
  REQUIRE(beam >= 1 && beam <= BEAM_MAX && nbest >= 1 && nbest <= beam, "clstm_net_beam: 1 <= nbest <= beam <= 32");
  QueryScope scope_(n, "clstm:beam", "ctc_beam");
  run_ctc_beam(h->beam, n.Z.p, n.desc.nclasses, n.line_off_h.data(), n.bs, beam, nbest, nhyp_h, len_h, score_h, labels_h, g_stream);
  ABI_END
}
int clstm_net_beam_lm(clstm_net* h, int beam, int nbest, const clstm_charlm* lm, float weight, float bonus, int* nhyp_h, int* len_h,
                      float* score_h, float* am_score_h, int* labels_h) {
  ABI_BEGIN
  REQUIRE(h, "null argument");
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_beam_lm");
  REQUIRE(lm, "clstm_net_beam_lm: the language model is required");
  REQUIRE(nhyp_h && score_h, "clstm_net_beam_lm: nhyp_h and score_h are required");
  REQUIRE(beam >= 1 && beam <= BEAM_MAX && nbest >= 1 && nbest <= beam, "clstm_net_beam_lm: 1 <= nbest <= beam <= 32");
  QueryScope scope_(n, "clstm:beam_lm", "ctc_beam_lm");
  const BeamLm with{&lm->lm, weight, bonus, am_score_h};
  run_ctc_beam(h->beam, n.Z.p, n.desc.nclasses, n.line_off_h.data(), n.bs, beam, nbest, nhyp_h, len_h, score_h, labels_h, g_stream, &with);
  ABI_END
}
int clstm_net_beam_lex(clstm_net* h, int beam, int nbest, const clstm_lexicon* lex, const clstm_charlm* lm, float weight, float bonus,
                       int* nhyp_h, int* len_h, float* score_h, float* am_score_h, int* labels_h) {
  ABI_BEGIN
  REQUIRE(h, "clstm_net_beam_lex: null net");
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_beam_lex");
  REQUIRE(lex, "clstm_net_beam_lex: the lexicon is required");
  REQUIRE(nhyp_h && score_h, "clstm_net_beam_lex: nhyp_h and score_h are required");
  REQUIRE(beam >= 1 && beam <= BEAM_MAX && nbest >= 1 && nbest <= beam, "clstm_net_beam_lex: 1 <= nbest <= beam <= 32");
  QueryScope scope_(n, "clstm:beam_lex", "ctc_beam_lex");
  const BeamLm with{lm ? &lm->lm : nullptr, weight, bonus, am_score_h};
  run_ctc_beam(h->beam, n.Z.p, n.desc.nclasses, n.line_off_h.data(), n.bs, beam, nbest, nhyp_h, len_h, score_h, labels_h, g_stream, &with,
               &lex->lex);
  ABI_END
}
// edit distance of every line's trivial_decode against its transcript: the guards and guarantees of clstm_net_score (reads Z only; the
// decode and edit workspaces are its own).  The decoded classes are compared where decode_kernel leaves them: their lengths are known to
// the device alone, so every line is planned for as many symbols as it has frames.
int clstm_net_errors(clstm_net* h, const int* labels_h, const int* L_h, int* dist_h, int* counts_h, int* confusion_h) {
  ABI_BEGIN
  REQUIRE(h, "null argument");
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_errors");
  const char* const E = "clstm_net_errors";
  const int nc = n.desc.nclasses, nsym = nc + 1;
  check_edit_common(E, nsym, dist_h || counts_h || confusion_h, confusion_h != nullptr);
  REQUIRE(labels_h && L_h, "clstm_net_errors: null argument");
  std::vector<int> roff(n.bs + 1, 0);
  for (int b = 0; b < n.bs; b++) {
    REQUIRE(L_h[b] >= 0, std::string(E) + ": L_h[" + std::to_string(b) + "] is negative");
    REQUIRE((long long)roff[b] + L_h[b] < 0x7FFFFFFFll, std::string(E) + ": the transcripts exceed 2^31 labels");
    roff[b + 1] = roff[b] + L_h[b];
  }
  check_edit_labels(E, "reference", labels_h, roff[n.bs], nsym);   // (a hypothesis label would be checked against nc: decode emits none outside [1, nc))
  EditJob job;
  job.script = counts_h || confusion_h;
  const int* lo = n.line_off_h.data();
  for (int b = 0; b < n.bs; b++) edit_add_pair(job, E, b, lo[b], lo[b + 1] - lo[b], roff[b], L_h[b]);
  QueryScope scope_(n, "clstm:errors");
  launch_decode(h->dec, n.Z.p, nc, lo, n.bs, g_stream, false);   // (outside the bracket)
  scope_.time("edit_distance");
  run_edit_distance(h->edit, job, roff[n.bs] ? labels_h : &EDIT_NO_LABELS, roff[n.bs], nullptr, 0, h->dec.cls.dev(), h->dec.cnt.dev(), nsym,
                    dist_h, counts_h, nullptr, nullptr, confusion_h, g_stream);
  ABI_END
}
int clstm_net_backward(clstm_net* h) { ABI_BEGIN h->net.require(Net::NEED_PASS, "clstm_net_backward"); h->net.backward(); ABI_END }
int clstm_net_enable_input_deltas(clstm_net* h, int on) { h->net.want_dx0 = on != 0; return 0; }
int clstm_net_get_input_deltas_h(clstm_net* h, float* dx) {
  ABI_BEGIN
  h->net.require(Net::NEED_DX0, "clstm_net_get_input_deltas_h");
  copy_d2h(dx, h->net.dX0.p, (size_t)h->net.N * h->net.desc.ninput);
  ABI_END
}
// (a backward pass of its own call ran the default plan: it left nothing for the update -- net.inc: StepPlan, PassLeft)
int clstm_net_update(clstm_net* h) { ABI_BEGIN PassLeft nothing; h->net.update(nothing); ABI_END }
int clstm_net_decode(clstm_net* h, int* cls, int* locs, int* cnt) {
  ABI_BEGIN
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_decode");
  run_decode(h->dec, n.Z.p, n.desc.nclasses, n.line_off_h.data(), n.bs, cls, locs, cnt, g_stream);
  ABI_END
}
// ---- recognition: CLSTMOCR::predict for a whole minibatch in one call (include/clstm_abi.h) ------------------------
static void net_predict(clstm_net* h, const int* T_h, int bs, const float* x, bool x_host, int* cls, int* locs, float* conf, int* cnt) {
  REQUIRE(h && T_h && x && cnt && bs > 0, "null argument (counts_h is required)");
  Net& n = h->net;
  n.set_batch_predict(T_h, bs);   // (T_h / bs are validated before the net is touched; drops a minibatch declared by clstm_net_train_step_next)
  // the frames into the net's input block: no ingest launch -- that one writes layer 0's source rows, which predict does not have
  const size_t nx = (size_t)n.N * n.desc.ninput;
  if (x_host) HIPCHECK(hipMemcpyAsync(n.X.p, x, nx * sizeof(float), hipMemcpyHostToDevice, g_stream));
  else {   // device frames: one launch, the line offsets riding it (ops.h: k_ingest_predict)
    const int nbx = nblocks(nx);
    const int* const lo = n.unsent_offsets();
    CLSTM_LAUNCH(k_ingest_predict, dim3(nbx + (lo ? 1 : 0)), dim3(256), 0, g_stream, x, n.X.p, nx, nbx, lo, n.line_off.p, 2 * n.bs + 1);
    check_launch();
    if (lo) n.offsets_sent(g_stream);
  }
  n.frames_ingested(false);
  n.predict();
  run_decode(h->dec, n.Z.p, n.desc.nclasses, n.line_off_h.data(), n.bs, cls, locs, cnt, g_stream, conf);
  // (as clstm_net_decode: the device error words are left to the next synchronisation point of the training loop)
}
int clstm_net_predict(clstm_net* h, const int* T_h, int bs, const float* x_d, int* cls, int* locs, float* conf, int* cnt) {
  ABI_BEGIN net_predict(h, T_h, bs, x_d, false, cls, locs, conf, cnt); ABI_END
}
int clstm_net_predict_h(clstm_net* h, const int* T_h, int bs, const float* x_h, int* cls, int* locs, float* conf, int* cnt) {
  ABI_BEGIN net_predict(h, T_h, bs, x_h, true, cls, locs, conf, cnt); ABI_END
}
// ---- line normalisation on the device (normalize.h, normalize_run.inc) ---------------------------------------------
int clstm_normalizer_create(clstm_normalizer** out, int target_height, float smooth2d, float smooth1d, float range) {
  ABI_BEGIN
  REQUIRE(out, "null argument");
  REQUIRE(target_height >= 1, "clstm_normalizer_create: target_height must be at least 1");
  REQUIRE(smooth2d > 0.0f && smooth1d > 0.0f && range > 0.0f && std::isfinite(smooth2d) && std::isfinite(smooth1d) && std::isfinite(range),
          "clstm_normalizer_create: smooth2d, smooth1d and range must be positive and finite");
  size_t* bytes = new size_t(0);
  AcctScope acct_(bytes);
  clstm_normalizer* h = nullptr;
  try { h = new clstm_normalizer(); } catch (...) { delete bytes; throw; }
  h->dev_bytes.reset(bytes);
  h->nz.target_height = target_height; h->nz.smooth2d = smooth2d; h->nz.smooth1d = smooth1d; h->nz.range = range;
  *out = h;
  ABI_END
}
int clstm_normalizer_destroy(clstm_normalizer* h) { ABI_BEGIN delete h; ABI_END }
int clstm_normalizer_run_h(clstm_normalizer* h, const float* pix_h, const int* w_h, const int* h_h, int bs, int* T_h, float* r_h, float** frames_d) {
  ABI_BEGIN REQUIRE(h, "null argument"); h->nz.run(pix_h, true, w_h, h_h, bs, T_h, r_h, frames_d); ABI_END
}
int clstm_normalizer_run_d(clstm_normalizer* h, const float* pix_d, const int* w_h, const int* h_h, int bs, int* T_h, float* r_h, float** frames_d) {
  ABI_BEGIN REQUIRE(h, "null argument"); h->nz.run(pix_d, false, w_h, h_h, bs, T_h, r_h, frames_d); ABI_END
}
int clstm_normalizer_get_frames_h(clstm_normalizer* h, float* frames_h) {
  ABI_BEGIN
  REQUIRE(h && frames_h, "null argument");
  REQUIRE(h->nz.last_frames > 0, "clstm_normalizer_get_frames_h: the last clstm_normalizer_run_* call on this normalizer produced no frames");
  HIPCHECK(hipMemcpyAsync(frames_h, h->nz.frames.p, h->nz.last_frames * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIPCHECK(hipStreamSynchronize(g_stream));
  ABI_END
}
int clstm_normalizer_device_bytes(clstm_normalizer* h, long long* bytes) {
  ABI_BEGIN
  REQUIRE(h && bytes, "null argument");
  *bytes = (long long)*h->dev_bytes;
  ABI_END
}
int clstm_degrader_create(clstm_degrader** out) {
  ABI_BEGIN
  REQUIRE(out, "null argument");
  size_t* bytes = new size_t(0);
  AcctScope acct_(bytes);
  clstm_degrader* h = nullptr;
  try { h = new clstm_degrader(); } catch (...) { delete bytes; throw; }
  h->dev_bytes.reset(bytes);
  *out = h;
  ABI_END
}
int clstm_degrader_destroy(clstm_degrader* h) { ABI_BEGIN delete h; ABI_END }
int clstm_degrader_run_h(clstm_degrader* h, const float* pix_h, const int* w_h, const int* h_h, int bs, const clstm_degrade_line* lines_h, float** out_pix_d) {
  ABI_BEGIN REQUIRE(h, "null argument"); h->dg.run(pix_h, true, w_h, h_h, bs, lines_h, out_pix_d); ABI_END
}
int clstm_degrader_run_d(clstm_degrader* h, const float* pix_d, const int* w_h, const int* h_h, int bs, const clstm_degrade_line* lines_h, float** out_pix_d) {
  ABI_BEGIN REQUIRE(h, "null argument"); h->dg.run(pix_d, false, w_h, h_h, bs, lines_h, out_pix_d); ABI_END
}
int clstm_degrader_get_pixels_h(clstm_degrader* h, float* out_h) {
  ABI_BEGIN
  REQUIRE(h && out_h, "null argument");
  REQUIRE(h->dg.last_pixels > 0, "clstm_degrader_get_pixels_h: the last clstm_degrader_run_* call on this degrader produced nothing");
  copy_d2h(out_h, h->dg.out.p, h->dg.last_pixels);
  ABI_END
}
int clstm_degrader_device_bytes(clstm_degrader* h, long long* bytes) {
  ABI_BEGIN
  REQUIRE(h && bytes, "null argument");
  *bytes = (long long)*h->dev_bytes;
  ABI_END
}
int clstm_degrade_default_ranges(clstm_degrade_ranges* out) {
  ABI_BEGIN
  REQUIRE(out, "null argument");
  *out = degrade_default_ranges();
  ABI_END
}
int clstm_degrade_draw(unsigned long long seed, unsigned long long key, unsigned long long visit, const clstm_degrade_ranges* rg, int w, int h,
                       clstm_degrade_line* out) {
  ABI_BEGIN
  REQUIRE(rg && out, "null argument");
  REQUIRE(w >= 1 && h >= 1, "clstm_degrade_draw: w and h must be at least 1");
  for (float a : {rg->angle, rg->scale, rg->aniso, rg->translate})
    REQUIRE(std::isfinite(a) && a >= 0.0f, "clstm_degrade_draw: angle, scale, aniso and translate must be finite and not negative");
  for (const float* iv : {rg->sigma, rg->maxdelta, rg->blur})
    REQUIRE(std::isfinite(iv[0]) && std::isfinite(iv[1]) && iv[0] >= 0.0f && iv[0] <= iv[1],
            "clstm_degrade_draw: the sigma, maxdelta and blur intervals must be finite, not negative, and ordered LO <= HI");
  degrade_draw(seed, key, visit, *rg, w, h, out);
  ABI_END
}
int clstm_net_device_bytes(clstm_net* h, long long* bytes) {
  ABI_BEGIN
  REQUIRE(h && bytes, "null argument");
  *bytes = (long long)(h->net.fixed_bytes + *h->dev_bytes);
  ABI_END
}
int clstm_net_get_state_h(clstm_net* h, int layer, int dir, int which, float* out) {
  ABI_BEGIN
  Net& n = h->net;
  n.require(Net::NEED_OUTPUTS, "clstm_net_get_state_h");
  REQUIRE(layer >= 0 && layer < (int)n.L.size() && dir >= 0 && dir < n.ndir && which >= 0 && which <= 9, "bad state selector");
  if (which != 5) n.require(Net::NEED_PASS, "clstm_net_get_state_h (which != 5)");
  Layer& y = n.L[layer];
  n.tmp.reserve((size_t)n.N * y.no);
  if (which >= 6) n.ensure_delta_f32(layer);   // (a persistent bf16 backward pass leaves the deltas as bf16 only)
  if (which == 5) n.ensure_h_f32(layer);       // (... forward pass of a lower layer: the outputs as bf16 only)
  const float* src = which < 4 ? y.G.p : which == 4 ? y.C.p : y.D.p;
  const int slot = which < 4 ? which : which >= 6 ? which - 6 : -1;
  if (which == 5)
    CLSTM_LAUNCH(k_gather_rows, dim3(nblocks((size_t)n.N * y.no)), dim3(256), 0, g_stream, (const float*)(y.hrow() + dir * y.no),
                 n.tmp.p, (size_t)n.N, y.no, y.ldh);
  else
    CLSTM_LAUNCH(k_gather_state, dim3(nblocks((size_t)n.N * y.no)), dim3(256), 0, g_stream, src, n.tmp.p, (size_t)n.N, y.no, n.ndir, dir, slot);
  check_launch();
  copy_d2h(out, n.tmp.p, (size_t)n.N * y.no);
  ABI_END
}
int clstm_net_set_gemm_precision(clstm_net* h, int mode) {
  ABI_BEGIN
  REQUIRE(mode >= 0 && mode <= 2, "precision: 0 = f32 (exact), 1 = bf16 inputs / f32 accumulation in the hoisted GEMMs, 2 = 1 + bf16 MFMA operands in the lock-step recurrence");
  Net& n = h->net;
  const bool rec = mode == 2;
  if (rec != n.bf16_rec) n.packed_dirty = true;   // the other weight packing is needed
  n.bf16_gemm = mode >= 1;
  n.bf16_rec = rec;
  if (n.holds.batch != Net::Holds::NONE && rec)   // a batch is already declared: make room for the bf16 operand copies
    for (auto& y : n.L)
      if (y.wide) n.reserve_wide_rings(y);
  ABI_END
}
int clstm_net_enable_timing(clstm_net* h, int on) { h->net.timing.on = on != 0; return 0; }
int clstm_net_kernel_time_ms(clstm_net* h, const char* name, double* total_ms, int* launches) {
  ABI_BEGIN
  h->net.timing.collect(g_stream);
  auto it = h->net.timing.acc.find(name);
  if (it == h->net.timing.acc.end()) { *total_ms = 0; *launches = 0; }
  else { *total_ms = it->second.first; *launches = it->second.second; }
  ABI_END
}
int clstm_net_reset_timing(clstm_net* h) { ABI_BEGIN h->net.timing.collect(g_stream); h->net.timing.acc.clear(); ABI_END }

// ---- one-call training step (step.inc: train_step) -------------------------------------------------------
// The same step for a loop that knows its NEXT minibatch (all of the `n` arguments NULL / 0: exactly clstm_net_train_step): its front
// half rides this step's last launch, and the next call -- which must bring that very minibatch -- starts with the forward launch.
// Between the two calls the net's per-batch accessors (outputs, decode, states) have no valid batch to refer to and refuse.
int clstm_net_train_step_next(clstm_net* h, const int* T_h, int bs, const float* x_d, const int* labels_h, const int* L_h,
                              const int* Tn_h, int bsn, const float* xn_d, const int* labels_n_h, const int* Ln_h) {
  ABI_BEGIN
  REQUIRE(h && T_h && x_d && labels_h && L_h, "null argument");
  train_step(h->net, h->ctc, Minibatch{T_h, bs, x_d, labels_h, L_h}, Minibatch{Tn_h, bsn, xn_d, labels_n_h, Ln_h}, nullptr);
  ABI_END
}
int clstm_net_train_step(clstm_net* h, const int* T_h, int bs, const float* x_d, const int* labels_h, const int* L_h) {
  return clstm_net_train_step_next(h, T_h, bs, x_d, labels_h, L_h, nullptr, 0, nullptr, nullptr, nullptr);
}
// host frames in, no host synchronisation: see Net::HostFeed
int clstm_net_train_step_h(clstm_net* h, const int* T_h, int bs, const float* x_h, const int* labels_h, const int* L_h) {
  ABI_BEGIN
  REQUIRE(h && T_h && x_h && labels_h && L_h && bs > 0, "null argument");
  Net& n = h->net;
  const long long N = batch_frames(T_h, bs);
  HostTicket ticket;
  const float* x_d = n.hf.stage(x_h, (size_t)N * n.desc.ninput, ticket);
  train_step(n, h->ctc, Minibatch{T_h, bs, x_d, labels_h, L_h}, Minibatch{}, &ticket);
  ABI_END
}
int clstm_host_alloc(void** p, size_t bytes) { ABI_BEGIN REQUIRE(p, "null argument"); HIPCHECK(hipHostMalloc(p, bytes ? bytes : 1)); ABI_END }
int clstm_host_free(void* p) { ABI_BEGIN if (p) HIPCHECK(hipHostFree(p)); ABI_END }

// ---- state externalisation (clstm.cc:762-811) -----------------------------------------------------------
namespace clstm {
// One entry per Sequence that walk_states(net, f, "", true) visits (clstm.cc:63-70): every node's inputs and
// outputs, then its registered states in std::map order (NPLSTM: ci, gf, gi, go, source, state --
// ENROLL(gi, gf, go, ci, state, source), clstm.cc:560), then its subs in order.
struct StateEntry {
  enum Kind { X, Z, LIN, HBOTH, HDIR, GATE, CELL, SOURCE } kind;
  int layer, dir, slot, rows;
  bool rev;   // stored in the time order of the NPLSTM inside Reversed (frame T-1-t at step t)
};
static std::vector<StateEntry> state_walk(const Net& n) {
  std::vector<StateEntry> w;
  const int nl = (int)n.L.size();
  auto lin_rows = [&](int l) { return l == 0 ? n.desc.ninput : n.ndir * n.L[l - 1].no; };
  auto nplstm = [&](int l, int dir, bool rev) {
    const int no = n.L[l].no;
    w.push_back({StateEntry::LIN, l, dir, 0, lin_rows(l), rev});            // inputs
    w.push_back({StateEntry::HDIR, l, dir, 0, no, rev});                    // outputs
    w.push_back({StateEntry::GATE, l, dir, 3, no, rev});                    // ci
    w.push_back({StateEntry::GATE, l, dir, 1, no, rev});                    // gf
    w.push_back({StateEntry::GATE, l, dir, 0, no, rev});                    // gi
    w.push_back({StateEntry::GATE, l, dir, 2, no, rev});                    // go
    w.push_back({StateEntry::SOURCE, l, dir, 0, lin_rows(l) + no, rev});    // source = [x_t ; h_{t-1}]
    w.push_back({StateEntry::CELL, l, dir, 0, no, rev});                    // state
  };
  w.push_back({StateEntry::X, 0, 0, 0, n.desc.ninput, false});              // Stacked.inputs
  w.push_back({StateEntry::Z, 0, 0, 0, n.desc.nclasses, false});            // Stacked.outputs
  for (int l = 0; l < nl; l++) {
    if (n.ndir == 2) {
      w.push_back({StateEntry::LIN, l, 0, 0, lin_rows(l), false});          // Parallel.inputs
      w.push_back({StateEntry::HBOTH, l, 0, 0, 2 * n.L[l].no, false});      // Parallel.outputs
      nplstm(l, 0, false);
      w.push_back({StateEntry::LIN, l, 1, 0, lin_rows(l), false});          // Reversed.inputs
      w.push_back({StateEntry::HDIR, l, 1, 0, n.L[l].no, false});           // Reversed.outputs
      nplstm(l, 1, true);
    } else {
      nplstm(l, 0, false);
    }
  }
  w.push_back({StateEntry::LIN, nl, 0, 0, lin_rows(nl), false});            // SoftmaxLayer.inputs
  w.push_back({StateEntry::Z, 0, 0, 0, n.desc.nclasses, false});            // SoftmaxLayer.outputs
  return w;
}
// a reference Sequence is rectangular (size x rows x cols): every line of the batch must have the same length
static int states_T(const Net& n) {
  const int T = n.line_off_h[1] - n.line_off_h[0];
  for (int b = 0; b < n.bs; b++)
    REQUIRE(n.line_off_h[b + 1] - n.line_off_h[b] == T, "state externalisation needs equal-length lines (a Sequence is size x rows x cols)");
  return T;
}
struct HostArrays {   // host mirrors of the device arrays the walk touches
  std::vector<float> X, Z;
  std::vector<std::vector<float>> G, C, H, S;
};
// element (t, i, b) of entry e <-> (array, flat index)
static float* state_elem(const Net& n, HostArrays& a, const StateEntry& e, int T, int t, int i, int b) {
  const int tf = e.rev ? T - 1 - t : t;
  const size_t f = (size_t)n.line_off_h[b] + tf;
  switch (e.kind) {
    case StateEntry::X: return &a.X[f * n.desc.ninput + i];
    case StateEntry::Z: return &a.Z[f * n.desc.nclasses + i];
    case StateEntry::LIN:
      if (e.layer == 0) return &a.X[f * n.desc.ninput + i];
      return &a.H[e.layer - 1][f * n.L[e.layer - 1].ldh + n.L[e.layer - 1].hofs + i];
    case StateEntry::HBOTH: return &a.H[e.layer][f * n.L[e.layer].ldh + n.L[e.layer].hofs + i];
    case StateEntry::HDIR: return &a.H[e.layer][f * n.L[e.layer].ldh + n.L[e.layer].hofs + e.dir * n.L[e.layer].no + i];
    case StateEntry::GATE: return &a.G[e.layer][((f * n.ndir + e.dir) * n.L[e.layer].no + i) * 4 + e.slot];
    case StateEntry::CELL: return &a.C[e.layer][(f * n.ndir + e.dir) * n.L[e.layer].no + i];
    case StateEntry::SOURCE: return &a.S[e.layer][(size_t)e.dir * n.N * n.L[e.layer].lds + f * n.L[e.layer].lds + 1 + i];
  }
  return nullptr;
}
static long long states_total(const Net& n, int T) {
  long long total = 0;
  for (auto& e : state_walk(n)) total += (long long)T * e.rows * n.bs + 4;   // n_states, clstm.cc:762-769
  return total;
}
}  // namespace clstm
int clstm_net_n_states(clstm_net* h, long long* out) {
  ABI_BEGIN
  REQUIRE(out, "null argument");
  h->net.require(Net::NEED_PASS, "clstm_net_n_states");
  *out = states_total(h->net, states_T(h->net));
  ABI_END
}
static void states_transfer(clstm_net* h, float* data, long long total, bool get) {
  Net& n = h->net;
  const int T = states_T(n);
  REQUIRE(total == states_total(n, T), get ? "size mismatch in get_states" : "size mismatch in set_states");
  HostArrays a;
  const size_t N = (size_t)n.N;
  a.X.resize(N * n.desc.ninput); a.Z.resize(N * n.desc.nclasses);
  a.G.resize(n.L.size()); a.C.resize(n.L.size()); a.H.resize(n.L.size()); a.S.resize(n.L.size());
  n.flush_line_off();
  // both directions start from the device contents: set_states only overwrites what the walk covers
  copy_d2h(a.X.data(), n.X.p, a.X.size());
  copy_d2h(a.Z.data(), n.Z.p, a.Z.size());
  for (size_t l = 0; l < n.L.size(); l++) {
    Layer& y = n.L[l];
    a.G[l].resize(N * n.ndir * 4 * y.no); a.C[l].resize(N * n.ndir * y.no);
    a.H[l].resize(N * y.ldh); a.S[l].resize(N * n.ndir * y.lds);
    n.ensure_source((int)l); n.ensure_h_f32((int)l);
    copy_d2h(a.G[l].data(), y.G.p, a.G[l].size()); copy_d2h(a.C[l].data(), y.C.p, a.C[l].size());
    copy_d2h(a.H[l].data(), y.H.p, a.H[l].size()); copy_d2h(a.S[l].data(), y.S.p, a.S[l].size());
  }
  long long index = 0;
  for (auto& e : state_walk(n)) {
    if (get) {
      data[index++] = 999999.0f; data[index++] = (float)T; data[index++] = (float)e.rows; data[index++] = (float)n.bs;
    } else {   // set_states: magic, size, rows, cols must describe this net and batch (clstm.cc:795-803)
      REQUIRE((int)data[index] == 999999 && (int)data[index + 1] == T && (int)data[index + 2] == e.rows &&
                  (int)data[index + 3] == n.bs, "size mismatch in set_states");
      index += 4;
    }
    for (int t = 0; t < T; t++)
      for (int i = 0; i < e.rows; i++)
        for (int b = 0; b < n.bs; b++) {
          float* p = state_elem(n, a, e, T, t, i, b);
          if (get) data[index++] = *p; else *p = data[index++];
        }
  }
  REQUIRE(index == total, "size mismatch in states walk");
  if (!get) {
    copy_h2d(n.X.p, a.X.data(), a.X.size());
    copy_h2d(n.Z.p, a.Z.data(), a.Z.size());
    for (size_t l = 0; l < n.L.size(); l++) {
      Layer& y = n.L[l];
      for (size_t f = 0; f < N; f++) {   // the bias inputs of the packed rows are constants, not states
        a.H[l][f * y.ldh + y.hofs - 1] = 1.0f;
        for (int d = 0; d < n.ndir; d++) a.S[l][(size_t)d * N * y.lds + f * y.lds] = 1.0f;
      }
      copy_h2d(y.G.p, a.G[l].data(), a.G[l].size()); copy_h2d(y.C.p, a.C[l].data(), a.C[l].size());
      copy_h2d(y.H.p, a.H[l].data(), a.H[l].size()); copy_h2d(y.S.p, a.S[l].data(), a.S[l].size());
    }
    n.states_set();   // (the f32 arrays were just written whole; the bf16 copies made by the forward pass no longer match them)
  }
}
int clstm_net_get_states_h(clstm_net* h, float* data, long long total) {
  ABI_BEGIN
  REQUIRE(data, "null argument");
  h->net.require(Net::NEED_PASS, "clstm_net_get_states_h");
  states_transfer(h, data, total, true);
  ABI_END
}
int clstm_net_set_states_h(clstm_net* h, const float* data, long long total) {
  ABI_BEGIN
  REQUIRE(data && total >= 4, "null argument");
  Net& n = h->net;
  // the first header carries the batch geometry (set_states resizes every Sequence from its header, clstm.cc:804)
  REQUIRE((int)data[0] == 999999, "bad magic in set_states");
  const int T = (int)data[1], bs = (int)data[3];
  REQUIRE(T > 0 && bs > 0 && (int)data[2] == n.desc.ninput, "size mismatch in set_states");
  std::vector<int> Ts(bs, T);
  n.set_batch(Ts.data(), bs);
  states_transfer(h, const_cast<float*>(data), total, false);
  ABI_END
}

// ---- data-parallel exchange ---------------------------------------------------------------------------
struct clstm_comm { Comm c; };
int clstm_comm_unique_id(char* id_h) {
  ABI_BEGIN
  REQUIRE(id_h, "null argument");
#ifndef CLSTM_HIP_EMU
  if (getenv("CLSTM_COMM_NO_RCCL") && atoi(getenv("CLSTM_COMM_NO_RCCL")) != 0) {   // (tests: ranks that share one device)
    FILE* f = fopen("/dev/urandom", "rb");
    REQUIRE(f && fread(id_h, 1, CLSTM_COMM_ID_BYTES, f) == (size_t)CLSTM_COMM_ID_BYTES, "cannot read /dev/urandom");
    fclose(f);
    return 0;
  }
  ncclUniqueId id;
  static_assert(sizeof(id) == CLSTM_COMM_ID_BYTES, "ncclUniqueId size");
  RCCLCHECK(RcclApi::get().GetUniqueId(&id));
  memcpy(id_h, &id, sizeof(id));
#else
  static int counter = 0;
  memset(id_h, 0, CLSTM_COMM_ID_BYTES);
  snprintf(id_h, CLSTM_COMM_ID_BYTES, "/clstm_emu_%d_%d", (int)getpid(), counter++);   // name of the shared segment
#endif
  ABI_END
}
int clstm_comm_create(clstm_comm** out, const char* id_h, int rank, int nranks) {
  ABI_BEGIN
  REQUIRE(out && id_h && nranks >= 1 && rank >= 0 && rank < nranks, "bad communicator arguments");
  clstm_comm* c = new clstm_comm();
  c->c.rank = rank; c->c.nranks = nranks;
#ifndef CLSTM_HIP_EMU
  try {
    memcpy(c->c.id, id_h, CLSTM_COMM_ID_BYTES);
    // CLSTM_COMM_NO_RCCL=1 (tests): no RCCL communicator -- the exchange is the peer-read path alone, which also works
    // between rank processes that share ONE device (RCCL refuses that: "duplicate GPU")
    if (!(getenv("CLSTM_COMM_NO_RCCL") && atoi(getenv("CLSTM_COMM_NO_RCCL")) != 0)) {
      ncclUniqueId id;
      memcpy(&id, id_h, sizeof(id));
      RCCLCHECK(RcclApi::get().CommInitRank(&c->c.comm, nranks, id, rank));
    }
  } catch (...) { delete c; throw; }
#else
  try { c->c.open(id_h, rank, nranks); } catch (...) { delete c; throw; }
#endif
  *out = c;
  ABI_END
}
int clstm_comm_destroy(clstm_comm* c) { ABI_BEGIN delete c; ABI_END }
int clstm_comm_rank(clstm_comm* c) { return c ? c->c.rank : 0; }
int clstm_comm_size(clstm_comm* c) { return c ? c->c.nranks : 1; }
int clstm_comm_peer_active(clstm_comm* c) { return c && c->c.peer.ok ? 1 : 0; }
int clstm_comm_peer_capacity(clstm_comm* c, long long* floats) {
  ABI_BEGIN
  REQUIRE(c && floats, "null argument");
  *floats = c->c.peer.ok ? (long long)c->c.peer.cap : 0;
  ABI_END
}
int clstm_allreduce_flat(clstm_comm* c, float* buf_d, long long n) {
  ABI_BEGIN
  REQUIRE(c && buf_d && n >= 0, "bad all-reduce arguments");
  if (n > 0) c->c.allreduce(buf_d, n, g_stream);
  ABI_END
}
int clstm_net_set_overlap(clstm_net* h, int mode) {
  ABI_BEGIN
  REQUIRE(mode >= 0 && mode <= 2, "overlap mode: 0 off, 1 one launch with two roles where it pays, 2 the same always (tests)");
  h->net.overlap = mode;
  ABI_END
}
int clstm_net_set_strict_f32(clstm_net* h, int on) {
  ABI_BEGIN
  Net& n = h->net;
  n.strict_f32 = on != 0;
  if (on) { n.dw_x3 = false; n.gemm_x3_on = false; }
  else {
    n.dw_x3 = dbg_opt("dw_x3") != 0;
    n.gemm_x3_on = dbg_opt("gemm_x3") != 0;
    n.split_terms = dbg_opt("split_terms");
  }
  n.packed_dirty = true;   // (the hi | lo weights of the f32-grade backward recurrence are only packed while that mode is on)
  ABI_END
}
int clstm_net_get_overlap(clstm_net* h, int* mode) {
  ABI_BEGIN
  REQUIRE(h && mode, "null argument");
  *mode = h->net.overlap;
  ABI_END
}
int clstm_net_overlap_stats(clstm_net* h, long long* launches, int* timeouts) {
  ABI_BEGIN
  Net& n = h->net;
  if (launches) *launches = n.dw_launches;
  if (timeouts) {
    *timeouts = 0;
    if (g_dev_err) {   // (process-wide count; also reported -- and cleared -- by the next synchronisation point)
      HIPCHECK(hipStreamSynchronize(g_stream));
      HIPCHECK(hipMemcpy(timeouts, g_dev_err + 1, sizeof(int), hipMemcpyDeviceToHost));
    }
  }
  ABI_END
}
int clstm_net_set_comm(clstm_net* h, clstm_comm* c) { h->net.comm = c ? &c->c : nullptr; return 0; }
int clstm_net_replica_check(clstm_net* h) {
  ABI_BEGIN
  REQUIRE(h, "null argument");
  h->net.replica_check(g_stream);   // (no-op without a communicator of several ranks; the verdict arrives with the next synchronisation)
  ABI_END
}
int clstm_net_set_training(clstm_net* h, int on) {
  ABI_BEGIN
  REQUIRE(h, "null argument");
  h->net.training = on != 0;
  ABI_END
}

// ---- diagnostics ----------------------------------------------------------------------------------
int clstm_debug_ctc_cycles(long long* out_h) {
  ABI_BEGIN
  REQUIRE(g_last_ctc_prof, "no CTC launch yet");
  HIPCHECK(hipStreamSynchronize(g_stream));
  HIPCHECK(hipMemcpy(out_h, g_last_ctc_prof, 16 * sizeof(long long), hipMemcpyDeviceToHost));
  ABI_END
}
#ifdef CLSTM_LSTM_PROF
int clstm_debug_lstm_cycles(clstm_net* h, long long* out_h) {   // diagnostics build only (not in the product ABI)
  ABI_BEGIN
  HIPCHECK(hipStreamSynchronize(g_stream));
  HIPCHECK(hipMemcpy(out_h, h->net.lstm_prof.p, 96 * sizeof(long long), hipMemcpyDeviceToHost));
  ABI_END
}
#endif
int clstm_debug_set_device_error(int which, int value) {   // tests: what a failed persistent launch / a timed-out item leaves behind
  ABI_BEGIN
  REQUIRE(which >= 0 && which <= 7, "bad error word");
  HIPCHECK(hipStreamSynchronize(g_stream));
  if (which == 4) { g_debug_fail_claims = value & 255; g_debug_fail_skip = value >> 8; return 0; }   // after (value >> 8) persistent launches the next (value & 255) fail their placement check
  if (which == 5) {                                                  // forget a placement failure: persistent launches again, `value` of them verified synchronously
    g_xcd_failed = false;
    g_xcd_outcome.check_all();
    g_xcd_outcome.verified = value ? 4 : 0;
    return 0;
  }
  HIPCHECK(hipMemcpy(dev_err_words() + which, &value, sizeof(int), hipMemcpyHostToDevice));
  ABI_END
}
int clstm_debug_set_option(const char* name, int value) {   // experiment switches (dbgopt.h); name NULL: forget every option set so far
  ABI_BEGIN
  HIPCHECK(hipStreamSynchronize(g_stream));
  if (!name) {
    dbg_opts().clear();
  } else {
    REQUIRE(dbg_opt_def(name), std::string("unknown option '") + name + "' (clstm_amd/csrc/dbgopt.h lists them)");
    dbg_opts()[name] = value;
  }
  ABI_END
}
int clstm_debug_path_count(int which, long long* out_h) {
  ABI_BEGIN
  REQUIRE(which >= 0 && which < PC_COUNT && out_h, "bad path index");
  if (which == PC_MFMA_ROUTED) {   // counted on the device: minibatches whose forward pass the batched recurrence handed to its routed per-line twins (lstm_mfma.h)
    int n = 0;
    HIPCHECK(hipStreamSynchronize(g_stream));
    HIPCHECK(hipMemcpy(&n, dev_err_words() + 8, sizeof(int), hipMemcpyDeviceToHost));
    *out_h = n;
    return 0;
  }
  *out_h = g_path_count[which];
  ABI_END
}
int clstm_debug_net_holds(clstm_net* h, int* out) {   // host only: what the net holds (net.inc: Net::Holds), nothing enqueued, no device memory touched
  ABI_BEGIN
  REQUIRE(h && out, "null argument");
  const Net& n = h->net;
  const int rec[8] = {n.bs, (int)std::min<long long>(n.N, 2147483647LL), n.holds.batch, n.holds.training_buffers, n.holds.forward, n.holds.frames,
                      n.holds.offsets_sent, n.holds.dx0};
  memcpy(out, rec, sizeof(rec));
  ABI_END
}
int clstm_debug_wide_plan(const int* shape, int* plan) {   // host arithmetic only: no net, no device (runtime.inc:wide_plan)
  ABI_BEGIN
  REQUIRE(shape && plan, "null argument");
  static_assert(sizeof(WideShape) == 20 * sizeof(int) && sizeof(WidePlan) == 14 * sizeof(int), "include/clstm_abi.h documents the int layout");
  WideShape h;
  memcpy(&h, shape, sizeof(h));
  REQUIRE(h.no > 0 && h.ndir >= 1 && h.bs > 0 && h.ncu >= 0, "bad shape");
  const WidePlan p = wide_plan(h);
  memcpy(plan, &p, sizeof(p));
  ABI_END
}
int clstm_debug_narrow_plan(const int* shape, int* plan) {   // host arithmetic only: no net, no device (runtime.inc:narrow_plan)
  ABI_BEGIN
  REQUIRE(shape && plan, "null argument");
  static_assert(sizeof(NarrowShape) == 30 * sizeof(int) && sizeof(NarrowPlan) == 11 * sizeof(int), "include/clstm_abi.h documents the int layout");
  NarrowShape h;
  memcpy(&h, shape, sizeof(h));
  REQUIRE(h.pass >= NP_FWD_SAVE && h.pass <= NP_BWD && h.no > 0 && h.ndir >= 1 && h.bs > 0 && h.ncu >= 0, "bad shape");
  const NarrowPlan p = narrow_plan(h);
  memcpy(plan, &p, sizeof(p));
  ABI_END
}
int clstm_debug_product_plan(const int* shape, int* plan) {   // host arithmetic only: no net, no device (runtime.inc:product_plan)
  ABI_BEGIN
  REQUIRE(shape && plan, "null argument");
  static_assert(sizeof(ProductShape) == 35 * sizeof(int) && sizeof(ProductPlan) == 39 * sizeof(int), "include/clstm_abi.h documents the int layout");
  ProductShape h;
  memcpy(&h, shape, sizeof(h));
  REQUIRE(h.pass >= PP_FWD && h.pass <= PP_BWD && h.no > 0 && h.ni > 0 && h.ndir >= 1 && h.N > 0 && h.nclasses >= 2 && h.ncu >= 0, "bad shape");
  const ProductPlan p = product_plan(h);
  memcpy(plan, &p, sizeof(p));
  ABI_END
}
int clstm_debug_ctc_plan(int nc, const int* line_off_h, const int* states_h, const int* state_off_h, int bs, int* batch_plan_h,
                         int* line_plan_h) {   // host arithmetic only: no net, no device (ctc.h: ctc_batch_plan / ctc_line_plan)
  ABI_BEGIN
  describe_ctc_plan(nc, line_off_h, states_h, state_off_h, bs, batch_plan_h, line_plan_h);
  ABI_END
}
int clstm_debug_ctc_split(int bs, int ncu, int* nsplit_h) {   // host arithmetic only (ctc.h: ctc_nsplit under the option ctc_split as it stands)
  ABI_BEGIN
  REQUIRE(bs > 0 && ncu >= 0 && nsplit_h, "bad argument");
  const int opt = dbg_opt("ctc_split");
  REQUIRE(opt == 0 || opt == 1 || opt == 2 || opt == 4, "option ctc_split must be 0, 1, 2 or 4");
  *nsplit_h = ctc_nsplit(bs, ncu > 0 ? ncu : device_cu_count(), opt);
  ABI_END
}
int clstm_debug_ctc_part_frames(int T, int n, int k, int* range_h) {   // host arithmetic only (ctc.h: ctc_part_frames, the kernel's own)
  ABI_BEGIN
  REQUIRE(T >= 0 && n >= 1 && k >= 0 && k < n && range_h, "bad argument");
  const CtcFrames f = ctc_part_frames(T, n, k);
  range_h[0] = f.lo; range_h[1] = f.hi;
  ABI_END
}
int clstm_debug_ctc_cycles_part(int part, long long* out_h) {
  ABI_BEGIN
  REQUIRE(g_last_ctc_prof, "no CTC launch yet");
  REQUIRE(part >= 0 && part < 4 && out_h, "bad argument");
  HIPCHECK(hipStreamSynchronize(g_stream));
  HIPCHECK(hipMemcpy(out_h, g_last_ctc_prof + 16 * part, 16 * sizeof(long long), hipMemcpyDeviceToHost));
  ABI_END
}
int clstm_debug_lane_ops(float* out) {
  ABI_BEGIN
  CLSTM_LAUNCH(k_debug_lane_ops, dim3(1), dim3(64), 0, g_stream, out);
  check_launch();
  ABI_END
}
int clstm_debug_gemm(int mode, const float* A, const float* B, float* Cm, int R, int Cn, int K, int nsplit) {
  ABI_BEGIN
  static thread_local DevBuf<float>* part = nullptr;
  // (no net, no plan: the tile rule of runtime.inc asked directly, as product_plan asks it)
  const int sq = gemm_bf16_big(R, Cn) ? GB2_BT : GEMM_BT, kk = gemm_tile256(R, Cn) ? 256 : GB2_BT;
  // user arrays are exact-size: no slack, the descriptor ends at the last element
  if (mode == 0) gemm_f32<GEMM_KC, GEMM_MC>(g_stream, gemm_kc(A, K, R, 0), gemm_mc(B, Cn, K, 0), StorePlain{Cm, Cn}, R, Cn, K);
  else if (mode == 1) gemm_f32<GEMM_KC, GEMM_KC>(g_stream, gemm_kc(A, K, R, 0), gemm_kc(B, K, Cn, 0), StorePlain{Cm, Cn}, R, Cn, K);
  else if (mode == 2) {
    if (!part) part = new DevBuf<float>();
    if (nsplit < 1) nsplit = 1;
    part->reserve((size_t)nsplit * R * Cn);
    gemm_f32<GEMM_MC, GEMM_MC>(g_stream, gemm_mc(A, R, K, 0), gemm_mc(B, Cn, K, 0), StorePartial{part->p, R, Cn}, R, Cn, K, nsplit);
    CLSTM_LAUNCH(k_reduce_scatter, dim3(nblocks((size_t)R * Cn)), dim3(256), 0, g_stream,
                 (ReduceDesc{part->p, nullptr, 0LL, nsplit, 1, R, Cn, Cn}), (ReduceDesc{}), Cm, (int*)nullptr, 0, (UpdateFuse{}));
  } else if (mode == 10) gemm_bf16<GEMM_KC, GEMM_MC>(g_stream, gemm_kc(A, K, R, 0), gemm_mc(B, Cn, K, 0), StorePlain{Cm, Cn}, R, Cn, K, sq);
  else if (mode == 11) gemm_bf16<GEMM_KC, GEMM_KC>(g_stream, gemm_kc(A, K, R, 0), gemm_kc(B, K, Cn, 0), StorePlain{Cm, Cn}, R, Cn, K, sq);
  else if (mode == 12) {
    if (!part) part = new DevBuf<float>();
    if (nsplit < 1) nsplit = 1;
    part->reserve((size_t)nsplit * R * Cn);
    gemm_bf16<GEMM_MC, GEMM_MC>(g_stream, gemm_mc(A, R, K, 0), gemm_mc(B, Cn, K, 0), StorePartial{part->p, R, Cn}, R, Cn, K, sq, nsplit);
    CLSTM_LAUNCH(k_reduce_scatter, dim3(nblocks((size_t)R * Cn)), dim3(256), 0, g_stream,
                 (ReduceDesc{part->p, nullptr, 0LL, nsplit, 1, R, Cn, Cn}), (ReduceDesc{}), Cm, (int*)nullptr, 0, (UpdateFuse{}));
  } else if (mode == 34) {   // the kk product with its tiles brought in by LDS-DMA (gemm_b16kk_dma_kernel)
    gemm_b16kk(g_stream, GemmOperand16{(const unsigned short*)A, K, (long long)R * K}, GemmOperand16{(const unsigned short*)B, K, (long long)Cn * K},
               StorePlain{Cm, Cn}, R, Cn, K, kk, 2);
  } else if (mode == 30 || mode == 31) {   // A: [R][K] bf16, B: [Cn][K] bf16 (the caller passes halfs in float-typed pointers); 31: the one-barrier loop
    gemm_b16kk(g_stream, GemmOperand16{(const unsigned short*)A, K, (long long)R * K}, GemmOperand16{(const unsigned short*)B, K, (long long)Cn * K},
               StorePlain{Cm, Cn}, R, Cn, K, kk, mode == 31 ? 0 : 1);
  } else if (mode == 32 || mode == 33 || mode == 35) {   // A: [K][R] bf16, B: [K][Cn] bf16 (R, Cn multiples of 8), split-K slabs reduced afterwards; 33: the one-barrier loop
    if (!part) part = new DevBuf<float>();
    if (nsplit < 1) nsplit = 1;
    part->reserve((size_t)nsplit * R * Cn);
    gemm_b16mc(g_stream, GemmOperand16B{(const unsigned short*)A, R, (long long)K * R, 0}, GemmOperand16B{(const unsigned short*)B, Cn, (long long)K * Cn, 0},
               StorePartial{part->p, R, Cn}, R, Cn, K, gemm_mc_rows_per_tile(R, Cn), mode == 33 ? 0 : mode == 35 ? 3 : 1, nsplit);   // 35: tiles by LDS-DMA
    CLSTM_LAUNCH(k_reduce_scatter, dim3(nblocks((size_t)R * Cn)), dim3(256), 0, g_stream,
                 (ReduceDesc{part->p, nullptr, 0LL, nsplit, 1, R, Cn, Cn}), (ReduceDesc{}), Cm, (int*)nullptr, 0, (UpdateFuse{}));
  } else if (mode == 20) gemm_x3<GEMM_KC, GEMM_MC>(g_stream, gemm_kc(A, K, R, 0), gemm_mc(B, Cn, K, 0), StorePlain{Cm, Cn}, R, Cn, K);
  else if (mode == 21) gemm_x3<GEMM_KC, GEMM_KC>(g_stream, gemm_kc(A, K, R, 0), gemm_kc(B, K, Cn, 0), StorePlain{Cm, Cn}, R, Cn, K);
  else if (mode == 22) {
    if (!part) part = new DevBuf<float>();
    if (nsplit < 1) nsplit = 1;
    part->reserve((size_t)nsplit * R * Cn);
    gemm_x3<GEMM_MC, GEMM_MC>(g_stream, gemm_mc(A, R, K, 0), gemm_mc(B, Cn, K, 0), StorePartial{part->p, R, Cn}, R, Cn, K, nsplit);
    CLSTM_LAUNCH(k_reduce_scatter, dim3(nblocks((size_t)R * Cn)), dim3(256), 0, g_stream,
                 (ReduceDesc{part->p, nullptr, 0LL, nsplit, 1, R, Cn, Cn}), (ReduceDesc{}), Cm, (int*)nullptr, 0, (UpdateFuse{}));
  } else if (mode == 23) gemm_x3_big<GEMM_KC, GEMM_MC>(g_stream, gemm_kc(A, K, R, 0), gemm_mc(B, Cn, K, 0), StorePlain{Cm, Cn}, R, Cn, K);
  else if (mode == 24) gemm_x3_big<GEMM_KC, GEMM_KC>(g_stream, gemm_kc(A, K, R, 0), gemm_kc(B, K, Cn, 0), StorePlain{Cm, Cn}, R, Cn, K);
  else if (mode == 25) {
    if (!part) part = new DevBuf<float>();
    if (nsplit < 1) nsplit = 1;
    part->reserve((size_t)nsplit * R * Cn);
    gemm_x3_big<GEMM_MC, GEMM_MC>(g_stream, gemm_mc(A, R, K, 0), gemm_mc(B, Cn, K, 0), StorePartial{part->p, R, Cn}, R, Cn, K, nsplit);
    CLSTM_LAUNCH(k_reduce_scatter, dim3(nblocks((size_t)R * Cn)), dim3(256), 0, g_stream,
                 (ReduceDesc{part->p, nullptr, 0LL, nsplit, 1, R, Cn, Cn}), (ReduceDesc{}), Cm, (int*)nullptr, 0, (UpdateFuse{}));
  } else throw Error("bad mode");
  check_launch();
  ABI_END
}

}  // extern "C"

