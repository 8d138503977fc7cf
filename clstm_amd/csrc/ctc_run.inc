// ctc_run.inc -- part of clstm_hip.hip (namespace clstm): host side of the CTC, score and decode launches (workspaces, metadata staging,
// the table upload, transcript expansion and the one alignment launch site).
static thread_local long long* g_last_ctc_prof = nullptr;
// CTC on an arbitrary packed batch (used by the net and by the stand-alone ABI entry)
struct CtcWorkspace {
  CtcArgs pending{};            // kernel arguments of a prepared-but-not-launched alignment (train step)
  size_t pending_smem = 0;
  int pending_bs = 0;
  StagedBlock meta;             // [line records (32 bytes each, in workgroup order) | states]
  DevBuf<long long> prof;
  DevBuf<double> tables;
  DevBuf<float> lat;
  std::vector<int> nu, seen;    // host scratch of ctc_distinct_classes, kept across calls
};
// the ctc_tables.h block (ctc.h: CTC_TABLE_DOUBLES) in a workspace's own device buffer, uploaded when the workspace first needs it
static void upload_ctc_tables(DevBuf<double>& tables) {
  if (tables.p) return;
  tables.reserve(CTC_TABLE_DOUBLES);
  std::vector<double> tb(CTC_TABLE_DOUBLES);
  for (int i = 0; i < 32; i++) tb[i] = CTC_EXP2_32[i];
  for (int i = 0; i < 64; i++) { tb[32 + i] = CTC_LOG_INVC[i]; tb[96 + i] = CTC_LOG_LOGC[i]; }
  for (int k = 0; k < 2 * CTC_SP_KMAX + 1; k++)
    for (int c = 0; c < 4; c++) tb[160 + 4 * k + c] = CTC_SOFTPLUS[k][c];
  HIPCHECK(hipMemcpy(tables.p, tb.data(), CTC_TABLE_DOUBLES * sizeof(double), hipMemcpyHostToDevice));
}
// the alignment run_ctc prepared (w.pending): at once, or -- in a training step -- behind the forward pass (step.inc)
static void launch_ctc_align(const CtcWorkspace& w, hipStream_t s) {
  const dim3 grid((unsigned)w.pending_bs * (unsigned)w.pending.nsplit);   // part-major: workgroup i is part i / bs of line record i % bs
  if (!w.pending.float_logadd) {
    allow_dynamic_lds((const void*)ctc_align_kernel<false>, w.pending_smem);
    CLSTM_LAUNCH(ctc_align_kernel<false>, grid, dim3(CTC_THREADS), w.pending_smem, s, w.pending);
  } else {
    allow_dynamic_lds((const void*)ctc_align_kernel<true>, w.pending_smem);
    CLSTM_LAUNCH(ctc_align_kernel<true>, grid, dim3(CTC_THREADS), w.pending_smem, s, w.pending);
  }
  check_launch();
}
// n transcripts (packed labels, lengths) as blank-interleaved target states (clstm_mktargets) with their offsets: what the alignment
// and the score take
static void expand_transcripts(const int* labels_h, const int* L_h, int n, std::vector<int>& states, std::vector<int>& soff) {
  soff.assign(n + 1, 0);
  int lpos = 0;
  for (int b = 0; b < n; b++) {
    const int L = L_h[b];
    REQUIRE(L >= 0, "negative transcript length");
    states.resize(soff[b] + 2 * L + 1);
    clstm_mktargets(states.data() + soff[b], labels_h + lpos, L);
    for (int i = 0; i < L; i++) REQUIRE(labels_h[lpos + i] != 0, "transcript contains the blank class (Codec::encode asserts c != 0, clstm.cc:232)");
    lpos += L;
    soff[b + 1] = soff[b] + 2 * L + 1;
  }
}
// target states are classes: the one statement of this refusal (the alignment, the plan's description, the score, check_minibatch)
static void check_target_classes(int nc, const int* states_h, int ns) {
  for (int i = 0; i < ns; i++) REQUIRE(states_h[i] >= 0 && states_h[i] < nc, "target class out of range");
}
// the batch arithmetic of a minibatch (ctc.h: ctc_batch_plan) from its offsets, with the refusals run_ctc has always made
// ncu, split_opt: the device's CUs and the experiment option ctc_split (ctc.h: ctc_nsplit); the description of a plan asks for neither
static CtcBatchPlan ctc_minibatch_plan(int nc, const int* line_off_h, const int* state_off_h, int bs, int ncu = 0, int split_opt = 1) {
  int smax = 1, tmax = 1;
  for (int b = 0; b < bs; b++) {
    smax = std::max(smax, state_off_h[b + 1] - state_off_h[b]);
    tmax = std::max(tmax, line_off_h[b + 1] - line_off_h[b]);
  }
  REQUIRE(split_opt == 0 || split_opt == 1 || split_opt == 2 || split_opt == 4, "option ctc_split must be 0, 1, 2 or 4");
  const CtcBatchPlan bp = ctc_batch_plan(nc, smax, tmax, bs, ncu, split_opt);
  REQUIRE(bp.tile >= 1, "too many classes / target states for the CTC row tile");
  REQUIRE(bp.smem <= 160 * 1024, "CTC LDS carve exceeds 160 KiB");
  return bp;
}
// distinct classes of every line (CtcLine::nu) into nu[0 .. bs); the states are known to lie in [0, nc).  seen: scratch of the caller's
static void ctc_distinct_classes(int nc, const int* states_h, const int* state_off_h, int bs, std::vector<int>& nu, std::vector<int>& seen) {
  nu.assign(bs, 0);
  seen.assign(nc, -1);
  for (int b = 0; b < bs; b++)
    for (int i = state_off_h[b]; i < state_off_h[b + 1]; i++)
      if (seen[states_h[i]] != b) { seen[states_h[i]] = b; nu[b]++; }
}
// clstm_debug_ctc_plan: what run_ctc and the workgroups of its launch decide for this minibatch, without a device
constexpr int CTC_PLAN_INTS = 13;   // include/clstm_abi.h documents the record
static void describe_ctc_plan(int nc, const int* line_off_h, const int* states_h, const int* state_off_h, int bs, int* batch_plan_h,
                              int* line_plan_h) {
  REQUIRE(bs > 0 && nc >= 1 && line_off_h && states_h && state_off_h && batch_plan_h && line_plan_h, "empty batch / null argument");
  for (int b = 0; b < bs; b++)
    REQUIRE(line_off_h[b + 1] >= line_off_h[b] && state_off_h[b + 1] >= state_off_h[b], "bad offsets");
  check_target_classes(nc, states_h, state_off_h[bs]);
  const CtcBatchPlan bp = ctc_minibatch_plan(nc, line_off_h, state_off_h, bs);
  batch_plan_h[0] = bp.tile; batch_plan_h[1] = bp.smax; batch_plan_h[2] = bp.ncp; batch_plan_h[3] = bp.smem;
  const int cap = ctc_region_words(ctc_lds_layout(bp.tile, bp.ncp, bp.smax), bp.tile);
  std::vector<int> nus, seen;
  ctc_distinct_classes(nc, states_h, state_off_h, bs, nus, seen);
  for (int b = 0; b < bs; b++) {
    const int T = line_off_h[b + 1] - line_off_h[b], S = state_off_h[b + 1] - state_off_h[b];
    const int nu = nus[b];
    const CtcLinePlan p = ctc_line_plan(T, S, nu, nc, bp.ncp, bp.tile, cap);
    const int rec[CTC_PLAN_INTS] = {T, S, nu, p.form, p.rec, p.flat, p.lds_lat, (int)ctc_scores_in_lds(p, T, S, bp.ncp, nu, cap), p.lanemap,
                                    p.flat_stage, p.c_in_regs, p.d_per_state, p.ntiles};
    memcpy(line_plan_h + (size_t)b * CTC_PLAN_INTS, rec, sizeof(rec));
  }
}
// `defer` (non-null): the copy of the metadata block is not enqueued -- the caller folds it into a kernel it launches anyway before
// the CTC kernel (the input-ingest launch of a training step), receives source, destination and size here and commits the slot.
static void run_ctc(CtcWorkspace& w, const float* probs, float* deltas, float* aligned, int nc,
                    const int* line_off_h, const int* states_h, const int* state_off_h, int bs,
                    hipStream_t s, StagedCopy* defer = nullptr, bool launch = true) {
  REQUIRE(bs > 0, "empty batch");
  std::vector<long long> lo(bs + 1, 0);
  for (int b = 0; b < bs; b++) {
    const long long T = line_off_h[b + 1] - line_off_h[b], S = state_off_h[b + 1] - state_off_h[b];
    REQUIRE(T >= 0 && S >= 0, "bad offsets");
    // three lattices; lines of more than CTC_SMAX_LDS states keep their per-state totals (S doubles) behind them
    lo[b + 1] = lo[b] + 3 * T * S + (S > CTC_SMAX_LDS ? 2 * S + 2 : 0);
    lo[b + 1] += lo[b + 1] & 1;   // (8-byte alignment of those doubles)
  }
  const int ns = state_off_h[bs];
  check_target_classes(nc, states_h, ns);
  w.lat.reserve((size_t)(lo[bs] > 0 ? lo[bs] : 1));
  ctc_distinct_classes(nc, states_h, state_off_h, bs, w.nu, w.seen);
  const std::vector<int>& nus = w.nu;
  const size_t nst = (size_t)(ns > 0 ? ns : 1);   // (never an empty section)
  CtcArgs a{};
  w.meta.begin((size_t)bs * sizeof(CtcLine) + nst * sizeof(int));
  {
    // workgroups take the lines largest lattice first (nsplit workgroups per line, part-major; more workgroups than CUs run in rounds)
    std::vector<int> order(bs);
    for (int b = 0; b < bs; b++) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lo[x + 1] - lo[x] > lo[y + 1] - lo[y]; });
    const auto ln = w.meta.add<CtcLine>(bs);
    for (int i = 0; i < bs; i++) {
      const int b = order[i];
      ln.host[i] = CtcLine{lo[b], b, line_off_h[b], line_off_h[b + 1] - line_off_h[b], state_off_h[b], state_off_h[b + 1] - state_off_h[b], nus[b]};
    }
    const auto st = w.meta.add<int>(nst);
    if (ns > 0) memcpy(st.host, states_h, (size_t)ns * sizeof(int));
    a.lines = ln.dev; a.states = st.dev;
    if (defer) *defer = w.meta.deferred(); else w.meta.send(s);
  }
  a.P = probs; a.Dz = deltas; a.aligned = aligned;
  a.lat = w.lat.p; a.nc = nc;
  w.prof.reserve(16 * 4); a.prof = w.prof.p; g_last_ctc_prof = w.prof.p;   // (16 stamps per part of line 0)
  a.float_logadd = dbg_opt("ctc_float") != 0;   // experiment option (ctc.h: ctc_softplus_float); read per alignment
  upload_ctc_tables(w.tables);
  a.tables = w.tables.p;
  // (ctc.h: the one statement of the batch arithmetic; the option is read per alignment)
  const CtcBatchPlan bp = ctc_minibatch_plan(nc, line_off_h, state_off_h, bs, device_cu_count(), dbg_opt("ctc_split"));
  a.smax = bp.smax; a.ncp = bp.ncp; a.tile = bp.tile;
  a.bs = bs; a.nsplit = bp.nsplit;
  if (a.nsplit > 1) {
    // One workgroup per line after all where no line splits (the other workgroups would only read their record and leave), and where
    // an output overlaps the posteriors: one workgroup reads every posterior of an item before it writes there, several of a line would
    // write rows that another still reads.
    const int cap = ctc_region_words(ctc_lds_layout(bp.tile, bp.ncp, bp.smax), bp.tile);
    bool any = false;
    for (int b = 0; b < bs && !any; b++) {
      const int T = line_off_h[b + 1] - line_off_h[b], S = state_off_h[b + 1] - state_off_h[b];
      any = ctc_line_splits(ctc_line_plan(T, S, nus[b], nc, bp.ncp, bp.tile, cap), T, S, bp.ncp, nus[b], cap);
    }
    const uintptr_t p0 = (uintptr_t)probs, p1 = p0 + (size_t)line_off_h[bs] * nc * sizeof(float);
    auto overlaps = [&](const float* o) { return o && (uintptr_t)o < p1 && (uintptr_t)o + (p1 - p0) > p0; };
    if (!any || overlaps(deltas) || overlaps(aligned)) a.nsplit = 1;
  }
  w.pending = a; w.pending_smem = (size_t)bp.smem; w.pending_bs = bs;
  if (launch) launch_ctc_align(w, s);
}
struct DecodeWorkspace {
  DevBuf<int> line_off, idx;
  DevBuf<float> val;
  ResultBlock res;
  ResultBlock::Sec<int> cnt, cls, loc;   // the sections of the last launch_decode, in the block's order: counts bs, classes N, locations N,
  ResultBlock::Sec<float> conf;          // peak values N
};
// the two launches of a decode; the results stay in w.res on the device (run_decode brings them back, clstm_net_errors compares them
// where they lie)
static void launch_decode(DecodeWorkspace& w, const float* probs, int nc, const int* line_off_h, int bs, hipStream_t s, bool want_conf) {
  const int N = line_off_h[bs];
  REQUIRE(bs > 0 && N > 0, "empty batch");
  w.line_off.reserve(bs + 1); w.idx.reserve(N); w.val.reserve(N);
  w.res.begin();
  w.cnt = w.res.add<int>(bs); w.cls = w.res.add<int>(N); w.loc = w.res.add<int>(N); w.conf = w.res.add<float>(N);
  w.res.reserve();
  HIPCHECK(hipMemcpyAsync(w.line_off.p, line_off_h, (bs + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  CLSTM_LAUNCH(argmax_kernel, dim3((N + 255) / 256), dim3(256), 0, s, probs, w.idx.p, w.val.p, N, nc);
  CLSTM_LAUNCH(decode_kernel, dim3(bs), dim3(64), 0, s, (const int*)w.idx.p, (const float*)w.val.p,
               (const int*)w.line_off.p, w.cls.dev(), w.loc.dev(), w.cnt.dev(), want_conf ? w.conf.dev() : (float*)nullptr);
  check_launch();
}
// conf_h (may be null): the peak value of every emitted class (decode_kernel: out_val)
static void run_decode(DecodeWorkspace& w, const float* probs, int nc, const int* line_off_h, int bs,
                       int* classes_h, int* locs_h, int* counts_h, hipStream_t s, float* conf_h = nullptr) {
  launch_decode(w, probs, nc, line_off_h, bs, s, conf_h != nullptr);
  const size_t N = (size_t)line_off_h[bs];
  // (one transfer instead of one per array.  Measured on whole recognition calls of one line of 200 frames, before -> after this and
  //  predict's one-launch ingest: set_batch + set_inputs_d + forward + decode 199 -> 172 us per call, clstm_net_predict with conf 210 ->
  //  172 us; EXPERIMENTS 13.4)
  ResultBlock::Span last = w.cnt;   // the block up to the last array asked for
  if (classes_h) last = w.cls;
  if (locs_h) last = w.loc;
  if (conf_h) last = w.conf;
  w.res.fetch(s, last);
  memcpy(counts_h, w.cnt.host(), (size_t)bs * sizeof(int));
  if (classes_h) memcpy(classes_h, w.cls.host(), N * sizeof(int));
  if (locs_h) memcpy(locs_h, w.loc.host(), N * sizeof(int));
  if (conf_h) memcpy(conf_h, w.conf.host(), N * sizeof(float));
}

// ---- scores and forced alignments (ctc_score.h) ------------------------------------------------------------------------
// A workspace of its own: metadata block, rolling rows / back-pointer words, result block.  Nothing here touches a
// CtcWorkspace: an alignment that clstm_net_train_step_next prepared and has not launched survives a score call.
struct ScoreWorkspace {
  StagedBlock meta;
  DevBuf<double> tables;
  DevBuf<unsigned long long> ws;
  ResultBlock res;
};
// what the launch will be, decided on the host from the arguments alone (nothing is enqueued while this can still refuse)
struct ScorePlan {
  std::vector<ScoreGroup> groups;
  std::vector<ScoreItem> items;
  std::vector<long long> path_off;   // per candidate, in ints
  long long npath = 0, ws_words = 0;
  int tmax = 1, tile = 0;
};
static void plan_ctc_score(ScorePlan& pl, int nc, const int* line_off_h, int bs, const int* states_h, const int* state_off_h,
                           const int* cand_line_h, int ncand, bool any_out, bool maxplus) {
  REQUIRE(any_out, "clstm_ctc_score: score_h, vscore_h and path_h are all NULL");
  REQUIRE(bs > 0 && ncand > 0 && nc >= 1 && line_off_h && states_h && state_off_h, "empty batch / null argument");
  REQUIRE(cand_line_h || ncand == bs, "cand_line_h is NULL: one candidate per line expected (ncand == bs)");
  for (int b = 0; b < bs; b++) {
    const long long T = (long long)line_off_h[b + 1] - line_off_h[b];
    REQUIRE(T >= 0 && line_off_h[b] >= 0, "bad offsets");
    REQUIRE(T * nc * 4 < 0x7FFFFFF0ll, "a line's posteriors exceed 2 GB");
  }
  for (int c = 0; c < ncand; c++) {
    REQUIRE(state_off_h[c] >= 0 && state_off_h[c + 1] - state_off_h[c] >= 1, "bad offsets (a candidate has at least one state)");
    if (cand_line_h) REQUIRE(cand_line_h[c] >= 0 && cand_line_h[c] < bs, "cand_line out of range");
  }
  check_target_classes(nc, states_h, state_off_h[ncand]);
  // items in candidate order first; T = 0 lines have no lattice (the caller fills -inf)
  pl.path_off.assign(ncand + 1, 0);
  struct Cand { int c, b, T, S, form; };
  std::vector<Cand> small, big;
  for (int c = 0; c < ncand; c++) {
    const int b = cand_line_h ? cand_line_h[c] : c;
    const int T = line_off_h[b + 1] - line_off_h[b], S = state_off_h[c + 1] - state_off_h[c];
    pl.path_off[c + 1] = pl.path_off[c] + T;
    if (T == 0) continue;
    const int form = (S <= 64 && T <= SCORE_TMAX) ? 0 : (S <= CTC_SMAX_LDS ? 1 : 2);
    (form == 0 ? small : big).push_back(Cand{c, b, T, S, form});
    if (form == 0) pl.tmax = std::max(pl.tmax, T);
  }
  pl.npath = pl.path_off[ncand];
  {   // frames of the LDS tile: what SCORE_ROW_WORDS hold, one thread per frame at most, no more than the longest line
    int tall = 1;
    for (int b = 0; b < bs; b++) tall = std::max(tall, line_off_h[b + 1] - line_off_h[b]);
    pl.tile = std::min(std::min(SCORE_THREADS, SCORE_ROW_WORDS / (nc | 1)), tall);
  }
  // one-wave items: a line's candidates side by side, largest first, four to a workgroup
  std::stable_sort(small.begin(), small.end(), [](const Cand& x, const Cand& y) { return x.b != y.b ? x.b < y.b : x.S > y.S; });
  auto item_of = [&](const Cand& k, long long ws_off) {
    return ScoreItem{ws_off, line_off_h[k.b], k.T, state_off_h[k.c], k.S, k.c, (int)pl.path_off[k.c]};
  };
  struct G { ScoreGroup g; long long cost; std::vector<ScoreItem> it; };
  std::vector<G> gs;
  for (size_t i = 0; i < small.size();) {
    G g{ScoreGroup{0, 0, 0, 0}, 0, {}};
    const int b = small[i].b;
    while (i < small.size() && small[i].b == b && g.g.n < SCORE_WAVES) { g.it.push_back(item_of(small[i], 0)); g.g.n++; i++; }
    g.g.lml = g.it[0].T <= pl.tile;   // the line fits the LDS tile whole: its match scores are made there once, for all candidates
    g.cost = (long long)g.it[0].T * 64;
    gs.push_back(g);
  }
  for (const Cand& k : big) {
    G g{ScoreGroup{0, 1, k.form, 0}, (long long)k.T * k.S, {}};
    g.it.push_back(item_of(k, pl.ws_words));
    pl.ws_words += (long long)k.T + k.S + (maxplus ? (long long)k.T * score_frame_words(k.S) : 0);
    gs.push_back(g);
  }
  REQUIRE(pl.npath < 0x7FFFFFFFll, "paths exceed 2^31 entries");
  std::stable_sort(gs.begin(), gs.end(), [](const G& x, const G& y) { return x.cost > y.cost; });   // workgroups largest first
  for (G& g : gs) {
    g.g.first = (int)pl.items.size();
    pl.groups.push_back(g.g);
    pl.items.insert(pl.items.end(), g.it.begin(), g.it.end());
  }
}
static void run_ctc_score(ScoreWorkspace& w, const float* probs, int nc, const int* line_off_h, int bs, const int* states_h,
                          const int* state_off_h, const int* cand_line_h, int ncand, float* score_h, float* vscore_h,
                          int* path_h, hipStream_t s) {
  const bool sum = score_h != nullptr, maxplus = vscore_h != nullptr || path_h != nullptr;
  ScorePlan pl;
  plan_ctc_score(pl, nc, line_off_h, bs, states_h, state_off_h, cand_line_h, ncand, sum || maxplus, maxplus);
  REQUIRE(probs, "null argument");
  if (!pl.groups.empty()) {
    const size_t ns = (size_t)state_off_h[ncand];
    ScoreArgs a{};
    w.meta.begin(pl.groups.size() * sizeof(ScoreGroup) + pl.items.size() * sizeof(ScoreItem) + ns * sizeof(int));
    a.groups = w.meta.put(pl.groups);
    a.items = w.meta.put(pl.items);
    a.states = w.meta.put(states_h, ns);
    w.ws.reserve((size_t)(pl.ws_words > 0 ? pl.ws_words : 1));
    w.res.begin();
    const auto score = w.res.add<float>(ncand), vscore = w.res.add<float>(ncand);
    const auto path = w.res.add<int>(path_h ? (size_t)pl.npath : 0);
    w.res.reserve();
    upload_ctc_tables(w.tables);
    w.meta.send(s);
    a.P = probs; a.tables = w.tables.p; a.ws = w.ws.p;
    a.nc = nc; a.ncp = nc | 1; a.tile = pl.tile; a.tmax = pl.tmax; a.ncand = ncand; a.npath = (int)pl.npath;
    const int ng = (int)pl.groups.size();
    if (sum) {
      const size_t smem = (size_t)score_lds_layout(a.tmax, a.tile, a.ncp, false).words * sizeof(float);
      allow_dynamic_lds((const void*)ctc_score_kernel<false>, smem);
      a.score = score.dev(); a.path = nullptr;
      CLSTM_LAUNCH(ctc_score_kernel<false>, dim3(ng), dim3(SCORE_THREADS), smem, s, a);
      check_launch();
      g_path_count[PC_SCORE]++;
    }
    if (maxplus) {
      const size_t smem = (size_t)score_lds_layout(a.tmax, a.tile, a.ncp, true).words * sizeof(float);
      allow_dynamic_lds((const void*)ctc_score_kernel<true>, smem);
      a.score = vscore.dev(); a.path = path_h ? path.dev() : nullptr;
      CLSTM_LAUNCH(ctc_score_kernel<true>, dim3(ng), dim3(SCORE_THREADS), smem, s, a);
      check_launch();
      g_path_count[PC_SCORE]++;
    }
    w.res.fetch(s, path);
    if (score_h) memcpy(score_h, score.host(), (size_t)ncand * sizeof(float));
    if (vscore_h) memcpy(vscore_h, vscore.host(), (size_t)ncand * sizeof(float));
    if (path_h) memcpy(path_h, path.host(), (size_t)pl.npath * sizeof(int));
  }
  for (int c = 0; c < ncand; c++) {   // a line without frames has no lattice
    if (pl.path_off[c + 1] != pl.path_off[c]) continue;
    if (score_h) score_h[c] = -INFINITY;
    if (vscore_h) vscore_h[c] = -INFINITY;
  }
}

// ---- n-best transcripts by prefix beam search (ctc_beam.h) -------------------------------------------------------------
// A workspace of its own, as the score's: a beam call touches neither a prepared alignment nor a score in flight.
struct BeamWorkspace {
  StagedBlock meta;
  DevBuf<int> ws;
  ResultBlock res;
};
// what the launch will be, from the arguments alone; every section of a line goes to LDS while the line's sections still fit
struct BeamPlan {
  std::vector<BeamLine> lines;
  long long ws_words = 0;
  int K = 1, lds_words = 0;
  bool all_lds = true;        // every section of every line in LDS: ctc_beam_kernel<true>
};
// a character n-gram model on the device (ctc_beam.h, second part): the table is checked and uploaded once, at creation
struct CharLm {
  int order = 0, nc = 0;
  long long nctx = 0;
  bool has_end = false;
  DevBuf<float> table, end;
};
// what a language model call brings beside the plain search's arguments
struct BeamLm { const CharLm* lm; float weight, bonus; float* am_score_h; };
// a lexicon on the device (ctc_beam.h, third part): the trie is built and checked on the host (lexicon_trie.h), uploaded once, at creation
struct Lexicon : LexiconTrie { DevBuf<int> dev; };
static void plan_ctc_beam(BeamPlan& pl, int nc, const int* line_off_h, int bs, int beam, int nbest, bool lm = false, bool lex = false) {
  REQUIRE(bs > 0 && line_off_h, "empty batch / null argument");
  REQUIRE(nc >= 2 && nc < (1 << 26), "clstm_ctc_beam: the class count must lie in [2, 2^26)");
  REQUIRE(beam >= 1 && beam <= BEAM_MAX, "clstm_ctc_beam: beam must lie in [1, 32]");
  REQUIRE(nbest >= 1 && nbest <= beam, "clstm_ctc_beam: nbest must lie in [1, beam]");
  REQUIRE(line_off_h[0] >= 0, "bad offsets");
  if (lex) REQUIRE((long long)beam * (nc - 1) <= BEAM_LM_CANDS, "clstm_ctc_beam_lex: beam * (nc - 1) exceeds 4096 (every class is a candidate of every entry)");
  else if (lm) REQUIRE((long long)beam * (nc - 1) <= BEAM_LM_CANDS, "clstm_ctc_beam_lm: beam * (nc - 1) exceeds 4096 (every class is a candidate of every entry)");
  pl.K = lm ? nc - 1 : beam_classes(nc, beam);
  const BeamLds L = beam_lds_layout(beam, pl.K, lm, lex ? beam * beam_lex_words(nc) : 0);
  const long long room = BEAM_LDS_WORDS - L.sections;
  for (int b = 0; b < bs; b++) {
    const long long T = (long long)line_off_h[b + 1] - line_off_h[b];
    REQUIRE(T >= 0, "bad offsets");
    REQUIRE(T * nc < (1ll << 29) && T * beam < (1ll << 28), "clstm_ctc_beam: a line's posteriors or its prefix trie exceed 2 GB");
    if (T == 0) continue;
    const long long nn = 1 + T * beam;
    long long H = 64;
    while (H < 2 * nn) H *= 2;
    const long long need[BS_COUNT] = {H, (lex ? 6 : lm ? 5 : 3) * nn, 2 * T * pl.K, T * nc};   // (nodes: + nlm, nctx; + nlex)
    BeamLine ln{};
    ln.row = line_off_h[b]; ln.T = (int)T; ln.line = b; ln.hmask = (int)(H - 1); ln.nnmax = (int)nn;
    long long used = 0;
    for (int s = 0; s < BS_COUNT; s++) {
      if (used + need[s] <= room && !(lm && s == BS_CLS)) { ln.in_lds |= 1 << s; ln.off[s] = used; used += need[s]; }
      else { ln.off[s] = pl.ws_words; pl.ws_words += need[s]; }
    }
    pl.lds_words = std::max(pl.lds_words, (int)used);
    pl.all_lds = pl.all_lds && (ln.in_lds | (lm ? 1 << BS_CLS : 0)) == (1 << BS_COUNT) - 1;
    pl.lines.push_back(ln);
  }
  REQUIRE(pl.ws_words < (1ll << 40), "clstm_ctc_beam: workspace too large");
  std::stable_sort(pl.lines.begin(), pl.lines.end(), [](const BeamLine& x, const BeamLine& y) { return x.T > y.T; });   // longest first
  pl.lds_words += L.sections;
}
static void run_ctc_beam(BeamWorkspace& w, const float* probs, int nc, const int* line_off_h, int bs, int beam, int nbest,
                         int* nhyp_h, int* len_h, float* score_h, int* labels_h, hipStream_t s, const BeamLm* lm = nullptr,
                         const Lexicon* lex = nullptr) {
  if (lex) {   // (the lexicon form: lm is given, its model may be null; everything is refused before anything is enqueued or written)
    REQUIRE(lm, "internal: the lexicon form takes weight and bonus from a BeamLm");
    REQUIRE(lex->nc == nc, "clstm_ctc_beam_lex: the lexicon was made for another class count");
    REQUIRE(!lm->lm || lm->lm->nc == nc, "clstm_ctc_beam_lex: the language model was made for another class count");
    REQUIRE(std::isfinite(lm->weight) && lm->weight >= 0.0f, "clstm_ctc_beam_lex: weight must be finite and not negative");
    REQUIRE(std::isfinite(lm->bonus), "clstm_ctc_beam_lex: bonus must be finite");
  } else if (lm) {   // (everything is refused before anything is enqueued or written)
    REQUIRE(lm->lm, "clstm_ctc_beam_lm: the language model is required");
    REQUIRE(lm->lm->nc == nc, "clstm_ctc_beam_lm: the language model was made for another class count");
    REQUIRE(std::isfinite(lm->weight) && lm->weight >= 0.0f, "clstm_ctc_beam_lm: weight must be finite and not negative");
    REQUIRE(std::isfinite(lm->bonus), "clstm_ctc_beam_lm: bonus must be finite");
  }
  BeamPlan pl;
  plan_ctc_beam(pl, nc, line_off_h, bs, beam, nbest, lm != nullptr, lex != nullptr);
  REQUIRE(probs && nhyp_h && score_h, "clstm_ctc_beam: probs, nhyp_h and score_h are required");
  const size_t N = (size_t)line_off_h[bs], nslot = (size_t)bs * nbest;
  for (int b = 0; b < bs; b++) nhyp_h[b] = 0;
  for (size_t i = 0; i < nslot; i++) {
    score_h[i] = -INFINITY;
    if (len_h) len_h[i] = 0;
    if (lm && lm->am_score_h) lm->am_score_h[i] = -INFINITY;
  }
  if (pl.lines.empty()) return;
  BeamArgs a{};
  w.meta.begin(pl.lines.size() * sizeof(BeamLine));
  a.lines = w.meta.put(pl.lines);
  w.ws.reserve((size_t)(pl.ws_words > 0 ? pl.ws_words : 1));
  w.res.begin();   // (am_score: only with a language model; labels: only where asked for)
  const auto nhyp = w.res.add<int>(bs), len = w.res.add<int>(nslot);
  const auto score = w.res.add<float>(nslot), am_score = w.res.add<float>(lm ? nslot : 0);
  const auto labels = w.res.add<int>(labels_h ? (size_t)nbest * N : 0);
  w.res.reserve();
  w.meta.send(s);
  w.res.zero(s, nhyp, labels);   // the whole block: lines without frames, label slots beyond a hypothesis
  a.P = probs; a.ws = w.ws.p;
  a.nhyp = nhyp.dev(); a.len = len.dev(); a.score = score.dev();
  a.labels = labels_h ? labels.dev() : nullptr;
  a.nc = nc; a.beam = beam; a.nbest = nbest; a.K = pl.K; a.bs = bs; a.N = (int)N;
  if (lm) {
    if (lm->lm) { a.table = lm->lm->table.p; a.end = lm->lm->has_end ? lm->lm->end.p : nullptr; }
    a.am_score = am_score.dev();
    a.weight = lm->weight; a.bonus = lm->bonus; a.order = lm->lm ? lm->lm->order : 2;
  }
  if (lex) a.lex = lex->dev.p;
  const size_t smem = (size_t)pl.lds_words * sizeof(float);
  auto launch = [&](auto kernel) {
    allow_dynamic_lds((const void*)kernel, smem);
    CLSTM_LAUNCH(kernel, dim3((unsigned)pl.lines.size()), dim3(BEAM_THREADS), smem, s, a);
  };
  if (lex) { if (pl.all_lds) launch(ctc_beam_kernel<true, true, true>); else launch(ctc_beam_kernel<false, true, true>); }
  else if (lm) { if (pl.all_lds) launch(ctc_beam_kernel<true, true>); else launch(ctc_beam_kernel<false, true>); }
  else if (pl.all_lds) launch(ctc_beam_kernel<true, false>);
  else launch(ctc_beam_kernel<false, false>);
  check_launch();
  g_path_count[lex ? PC_BEAM_LEX : lm ? PC_BEAM_LM : PC_BEAM]++;
  w.res.fetch(s, labels);
  for (const BeamLine& ln : pl.lines) {   // (lines without frames keep nhyp = 0, len = 0, score = -inf)
    const int b = ln.line;
    nhyp_h[b] = nhyp.host()[b];
    for (int k = 0; k < nbest; k++) {
      const size_t i = (size_t)b * nbest + k;
      if (len_h) len_h[i] = len.host()[i];
      memcpy(&score_h[i], score.host() + i, sizeof(float));
      if (lm && lm->am_score_h) memcpy(&lm->am_score_h[i], am_score.host() + i, sizeof(float));
    }
  }
  if (labels_h) memcpy(labels_h, labels.host(), (size_t)nbest * N * sizeof(int));
}

// ---- edit distance, edit script, confusions (edit_distance.h) ----------------------------------------------------------------
// A workspace of its own, as the score's and the beam's: an error count touches neither a prepared alignment nor anything of the net's.
struct EditWorkspace {
  StagedBlock meta;
  DevBuf<int> ws;             // direction words and edge columns beyond a wave's LDS carve
  ResultBlock res;
};
// what the launch will be, from the arguments alone (nothing is enqueued while this can still refuse)
struct EditJob {
  std::vector<EditPair> pairs;
  long long ws_words = 0, ops_words = 0;
  int lds_wave_words = 0;
  bool script = false;
};
constexpr int EDIT_PLAN_INTS = 5;   // include/clstm_abi.h documents the record
static void describe_edit_plan(int la, int lb, int want_script, int* plan) {
  REQUIRE(la >= 0 && lb >= 0 && plan, "clstm_debug_edit_plan: negative length / null argument");
  const EditPlan p = edit_plan(la, lb, want_script != 0);
  plan[0] = p.nstrips; plan[1] = p.dirs; plan[2] = p.edge; plan[3] = p.nw; plan[4] = p.lds_words;
}
// the refusals every caller shares; each names the entry and the offending index
static void check_edit_offsets(const char* entry, const char* what, const int* off, int n) {
  REQUIRE(off[0] >= 0, std::string(entry) + ": " + what + "[0] is negative");
  for (int i = 0; i < n; i++)
    REQUIRE(off[i + 1] >= off[i], std::string(entry) + ": " + what + "[" + std::to_string(i + 1) + "] is smaller than the offset before it");
}
// labels lie in [1, bound): bound = nsym, except that a hypothesis of clstm_net_errors has no label nclasses = nsym - 1
static void check_edit_labels(const char* entry, const char* what, const int* lab, long long n, int bound) {
  for (long long i = 0; i < n; i++)
    REQUIRE(lab[i] >= 1 && lab[i] < bound, std::string(entry) + ": " + what + " label " + std::to_string(lab[i]) + " at index " +
                                               std::to_string(i) + " is outside [1, " + std::to_string(bound) + ")");
}
static void check_edit_common(const char* entry, int nsym, bool any_out, bool conf) {
  REQUIRE(nsym >= 2, std::string(entry) + ": nsym must be at least 2");
  REQUIRE(any_out, std::string(entry) + ": every output is NULL");
  REQUIRE(!conf || (long long)nsym * nsym <= (1ll << 26), std::string(entry) + ": the confusion table exceeds 2^26 ints");
}
// one pair into the job: its slots, its workspace, the launch's LDS
static void edit_add_pair(EditJob& job, const char* entry, int idx, int hyp_off, int la_cap, int ref_off, int lb) {
  const EditPlan pl = edit_plan(la_cap, lb, job.script);
  EditPair pr{};
  pr.hyp_off = hyp_off; pr.la_cap = la_cap; pr.ref_off = ref_off; pr.lb = lb; pr.idx = idx;
  pr.ops_off = (int)job.ops_words;
  if (job.script) job.ops_words += (long long)la_cap + lb;
  if (pl.dirs == EDIT_WS) { pr.ws_dirs = job.ws_words; job.ws_words += pl.dir_words; }
  if (pl.edge == EDIT_WS) { pr.ws_edge = job.ws_words; job.ws_words += pl.edge_words; }
  job.lds_wave_words = std::max(job.lds_wave_words, pl.lds_words);
  REQUIRE(job.ops_words < 0x7FFFFFFFll, std::string(entry) + ": the scripts exceed 2^31 slots");
  REQUIRE(job.ws_words < (1ll << 33), std::string(entry) + ": workspace too large");
  job.pairs.push_back(pr);
}
static const int EDIT_NO_LABELS = 0;   // stands for an empty label array (no hypothesis symbol at all is still the host form: hyps_h set)
// refs_h: nref_words packed reference labels; hyps_h (or NULL): nhyp_words packed hypothesis labels, copied behind them -- else the
// hypotheses are hyp_d / hyp_len_d on the device (clstm_net_errors).  Everything has been validated.
static void run_edit_distance(EditWorkspace& w, EditJob& job, const int* refs_h, long long nref_words, const int* hyps_h, long long nhyp_words,
                              const int* hyp_d, const int* hyp_len_d, int nsym, int* dist_h, int* counts_h, int* nops_h, int* ops_h,
                              int* conf_h, hipStream_t s) {
  const size_t np = job.pairs.size(), nconf = conf_h ? (size_t)nsym * nsym : 0;
  if (np == 0) {
    if (conf_h) memset(conf_h, 0, nconf * sizeof(int));
    return;
  }
  // waves take the pairs largest table first; a pair's results do not depend on where it runs
  std::stable_sort(job.pairs.begin(), job.pairs.end(), [](const EditPair& x, const EditPair& y) {
    return (long long)x.la_cap * x.lb > (long long)y.la_cap * y.lb;
  });
  const size_t nrf = (size_t)nref_words, nhy = (size_t)(hyps_h ? nhyp_words : 0);
  EditArgs a{};
  w.meta.begin(np * sizeof(EditPair) + (nrf + nhy) * sizeof(int));   // [pair records | references | hypotheses, where they come from the host]
  a.pairs = w.meta.put(job.pairs);
  a.ref = w.meta.put(refs_h, nrf);
  a.hyp = hyps_h ? w.meta.put(hyps_h, nhy) : hyp_d;
  a.hyp_len = hyps_h ? nullptr : hyp_len_d;
  w.ws.reserve((size_t)(job.ws_words > 0 ? job.ws_words : 1));
  w.res.begin();
  const auto dist = w.res.add<int>(np), counts = w.res.add<int>(3 * np), nops = w.res.add<int>(np);
  const auto conf = w.res.add<int>(nconf), ops = w.res.add<int>((size_t)job.ops_words);
  w.res.reserve();
  w.meta.send(s);
  if (nconf) w.res.zero(s, conf, conf);
  a.ws = w.ws.p;
  a.dist = dist.dev(); a.counts = counts.dev(); a.nops = nops.dev();
  a.conf = nconf ? conf.dev() : nullptr;
  a.ops = ops.dev();
  a.npairs = (int)np; a.nsym = nsym; a.lds_wave_words = job.lds_wave_words;
  const size_t smem = (size_t)EDIT_WAVES * job.lds_wave_words * sizeof(int);   // (<= 64 KiB: EDIT_WAVE_WORDS)
  const dim3 grid((unsigned)((np + EDIT_WAVES - 1) / EDIT_WAVES));
  if (job.script) CLSTM_LAUNCH(edit_distance_kernel<true>, grid, dim3(EDIT_THREADS), smem, s, a);
  else CLSTM_LAUNCH(edit_distance_kernel<false>, grid, dim3(EDIT_THREADS), smem, s, a);
  check_launch();
  g_path_count[PC_EDIT]++;
  w.res.fetch(s, !job.script ? dist : ops_h ? ops : conf);   // (the distances alone; everything; everything but the scripts)
  if (dist_h) memcpy(dist_h, dist.host(), np * sizeof(int));
  if (counts_h) memcpy(counts_h, counts.host(), 3 * np * sizeof(int));
  if (nops_h) memcpy(nops_h, nops.host(), np * sizeof(int));
  if (conf_h) memcpy(conf_h, conf.host(), nconf * sizeof(int));
  if (ops_h)   // (only the codes of each script: the rest of a pair's slots stays the caller's)
    for (const EditPair& pr : job.pairs) {
      const int n = nops.host()[pr.idx];
      memcpy(ops_h + pr.ops_off, ops.host() + pr.ops_off, (size_t)n * sizeof(int));
    }
}
// clstm_edit_distance_batch: validation, the job, the call
static void edit_distance_batch(EditWorkspace& w, const int* hyp_h, const int* hyp_off_h, int npairs, const int* ref_h, const int* ref_off_h,
                                int nref, const int* ref_of_h, int nsym, int* dist_h, int* counts_h, int* nops_h, int* ops_h, int* conf_h,
                                hipStream_t s) {
  const char* const E = "clstm_edit_distance_batch";
  check_edit_common(E, nsym, dist_h || counts_h || nops_h || ops_h || conf_h, conf_h != nullptr);
  REQUIRE(npairs >= 0 && nref >= 0 && hyp_off_h && ref_off_h, std::string(E) + ": negative count / null offsets");
  REQUIRE(ref_of_h || nref == npairs, std::string(E) + ": ref_of_h is NULL: one reference per pair expected (nref == npairs)");
  check_edit_offsets(E, "hyp_off_h", hyp_off_h, npairs);
  check_edit_offsets(E, "ref_off_h", ref_off_h, nref);
  const int h0 = hyp_off_h[0], r0 = ref_off_h[0];
  const long long nh = (long long)hyp_off_h[npairs] - h0, nr = (long long)ref_off_h[nref] - r0;
  REQUIRE((nh == 0 || hyp_h) && (nr == 0 || ref_h), std::string(E) + ": null labels");
  for (int p = 0; ref_of_h && p < npairs; p++)
    REQUIRE(ref_of_h[p] >= 0 && ref_of_h[p] < nref, std::string(E) + ": ref_of_h[" + std::to_string(p) + "] is out of range");
  if (nh) check_edit_labels(E, "hypothesis", hyp_h + h0, nh, nsym);
  if (nr) check_edit_labels(E, "reference", ref_h + r0, nr, nsym);
  EditJob job;
  job.script = counts_h || nops_h || ops_h || conf_h;
  for (int p = 0; p < npairs; p++) {
    const int q = ref_of_h ? ref_of_h[p] : p;
    edit_add_pair(job, E, p, hyp_off_h[p] - h0, hyp_off_h[p + 1] - hyp_off_h[p], ref_off_h[q] - r0, ref_off_h[q + 1] - ref_off_h[q]);
  }
  run_edit_distance(w, job, nr ? ref_h + r0 : &EDIT_NO_LABELS, nr, nh ? hyp_h + h0 : &EDIT_NO_LABELS, nh, nullptr, nullptr, nsym, dist_h, counts_h,
                    nops_h, ops_h, conf_h, s);
}

// the calling thread's own workspace of a kind, made at its first use and kept (the stand-alone batch entries; a net brings its own)
template <class W>
static W& thread_workspace() {
  static thread_local W* w = nullptr;
  if (!w) w = new W();
  return *w;
}
