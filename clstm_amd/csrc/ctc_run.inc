// ctc_run.inc -- part of clstm_hip.hip (namespace clstm): host side of the CTC and decode launches (workspaces, metadata staging).
static thread_local long long* g_last_ctc_prof = nullptr;
// CTC on an arbitrary packed batch (used by the net and by the stand-alone ABI entry)
struct CtcWorkspace {
  CtcArgs pending{};            // kernel arguments of a prepared-but-not-launched alignment (train step)
  size_t pending_smem = 0;
  int pending_bs = 0;
  PinnedRing ring;
  DevBuf<long long> prof;
  DevBuf<double> tables;
  DevBuf<char> meta;
  DevBuf<float> lat;
};
// The per-minibatch metadata block [line records | states] is staged in a pinned slot;
// `defer` (non-null): do not enqueue its copy -- the caller folds it into a kernel it launches anyway before the CTC
// kernel (the input-ingest launch of a training step) and receives source, destination and size here.
struct CtcMetaCopy { const int* src = nullptr; int* dst = nullptr; int nwords = 0; };
static void run_ctc(CtcWorkspace& w, const float* probs, float* deltas, float* aligned, int nc,
                    const int* line_off_h, const int* states_h, const int* state_off_h, int bs,
                    hipStream_t s, CtcMetaCopy* defer = nullptr, bool launch = true) {
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
  for (int i = 0; i < ns; i++) REQUIRE(states_h[i] >= 0 && states_h[i] < nc, "target class out of range");
  w.lat.reserve((size_t)(lo[bs] > 0 ? lo[bs] : 1));
  // one pinned slot, one device block, one copy: [line records (bs x 32 bytes, in workgroup order) | states]
  const size_t nln = (size_t)bs * sizeof(CtcLine), nst = (size_t)(ns > 0 ? ns : 1) * sizeof(int);
  w.meta.reserve(nln + nst);
  {
    char* stage = (char*)w.ring.acquire(nln + nst);
    // workgroups take the lines largest lattice first (one workgroup per line; more lines than CUs run in rounds)
    std::vector<int> order(bs);
    for (int b = 0; b < bs; b++) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return lo[x + 1] - lo[x] > lo[y + 1] - lo[y]; });
    CtcLine* ln = (CtcLine*)stage;
    for (int i = 0; i < bs; i++) {
      const int b = order[i];
      ln[i] = CtcLine{lo[b], b, line_off_h[b], line_off_h[b + 1] - line_off_h[b], state_off_h[b], state_off_h[b + 1] - state_off_h[b], 0};
    }
    if (ns > 0) memcpy(stage + nln, states_h, (size_t)ns * sizeof(int));
    if (defer) {
      defer->src = (const int*)stage; defer->dst = (int*)w.meta.p; defer->nwords = (int)((nln + nst) / sizeof(int));
    } else {
      HIPCHECK(hipMemcpyAsync(w.meta.p, stage, nln + nst, hipMemcpyHostToDevice, s));
      w.ring.commit(s);
    }
  }
  CtcArgs a{};
  a.lines = (const CtcLine*)w.meta.p;
  a.P = probs; a.Dz = deltas; a.aligned = aligned;
  a.states = (const int*)(w.meta.p + nln);
  a.lat = w.lat.p; a.nc = nc;
  w.prof.reserve(16); a.prof = w.prof.p; g_last_ctc_prof = w.prof.p;
  a.float_logadd = dbg_opt("ctc_float") != 0;   // experiment option (ctc.h: ctc_softplus_float); read per alignment
  if (!w.tables.p) {
    w.tables.reserve(CTC_TABLE_DOUBLES);
    std::vector<double> tb(CTC_TABLE_DOUBLES);
    for (int i = 0; i < 32; i++) tb[i] = CTC_EXP2_32[i];
    for (int i = 0; i < 64; i++) { tb[32 + i] = CTC_LOG_INVC[i]; tb[96 + i] = CTC_LOG_LOGC[i]; }
    for (int k = 0; k < 2 * CTC_SP_KMAX + 1; k++)
      for (int c = 0; c < 4; c++) tb[160 + 4 * k + c] = CTC_SOFTPLUS[k][c];
    HIPCHECK(hipMemcpy(w.tables.p, tb.data(), CTC_TABLE_DOUBLES * sizeof(double), hipMemcpyHostToDevice));
  }
  a.tables = w.tables.p;
  int smax = 1, tmax = 1;
  for (int b = 0; b < bs; b++) {
    smax = std::max(smax, state_off_h[b + 1] - state_off_h[b]);
    tmax = std::max(tmax, line_off_h[b + 1] - line_off_h[b]);
  }
  if (smax > CTC_SMAX_LDS) smax = CTC_SMAX_LDS;     // (longer lines do not use the per-state LDS arrays)
  a.smax = smax;
  a.ncp = nc | 1;                                   // odd row stride: conflict-free row-per-lane access
  // frames per LDS tile: what the 160 KiB carve leaves after the tables and the per-state vectors
  const long fixed = (long)ctc_lds_layout(0, a.ncp, smax).words * (long)sizeof(float);
  int tile = (int)((160 * 1024 - fixed) / (long)((a.ncp + (smax | 1) + 1) * sizeof(float)));
  if (tile > CTC_MAX_TILE) tile = CTC_MAX_TILE;
  if (tile > tmax) tile = tmax;
  REQUIRE(tile >= 1, "too many classes / target states for the CTC row tile");
  a.tile = tile;
  const size_t smem = (size_t)ctc_lds_layout(a.tile, a.ncp, a.smax).words * sizeof(float);
  REQUIRE(smem <= 160 * 1024, "CTC LDS carve exceeds 160 KiB");
#ifndef CLSTM_HIP_EMU
  static size_t smem_set = 0;
  if (smem > smem_set) {
    HIPCHECK(hipFuncSetAttribute((const void*)ctc_align_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    HIPCHECK(hipFuncSetAttribute((const void*)ctc_align_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    smem_set = smem;
  }
#endif
  w.pending = a; w.pending_smem = smem; w.pending_bs = bs;
  if (launch) {
    if (a.float_logadd) CLSTM_LAUNCH(ctc_align_kernel<true>, dim3(bs), dim3(CTC_THREADS), smem, s, a);
    else CLSTM_LAUNCH(ctc_align_kernel<false>, dim3(bs), dim3(CTC_THREADS), smem, s, a);
    check_launch();
  }
}
struct DecodeWorkspace {
  DevBuf<int> line_off, idx;
  DevBuf<float> val;
  DevBuf<int> out;            // [counts bs | classes N | locs N | peak values N (float bits)]: ONE copy brings the results back
  int* host = nullptr;        // pinned landing buffer of that copy
  size_t host_cap = 0;
  ~DecodeWorkspace() { if (host) (void)hipHostFree(host); }
};
// conf_h (may be null): the peak value of every emitted class (decode_kernel: out_val)
static void run_decode(DecodeWorkspace& w, const float* probs, int nc, const int* line_off_h, int bs,
                       int* classes_h, int* locs_h, int* counts_h, hipStream_t s, float* conf_h = nullptr) {
  const int N = line_off_h[bs];
  REQUIRE(bs > 0 && N > 0, "empty batch");
  const size_t nout = (size_t)bs + 3 * (size_t)N;
  w.line_off.reserve(bs + 1); w.idx.reserve(N); w.val.reserve(N); w.out.reserve(nout);
  if (w.host_cap < nout) {
    if (w.host) HIPCHECK(hipHostFree(w.host));
    w.host = nullptr; w.host_cap = 0;
    HIPCHECK(hipHostMalloc((void**)&w.host, (nout + nout / 4 + 64) * sizeof(int)));
    w.host_cap = nout + nout / 4 + 64;
  }
  int* cnt_d = w.out.p; int* cls_d = cnt_d + bs; int* loc_d = cls_d + N; float* conf_d = reinterpret_cast<float*>(loc_d + N);
  HIPCHECK(hipMemcpyAsync(w.line_off.p, line_off_h, (bs + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  CLSTM_LAUNCH(argmax_kernel, dim3((N + 255) / 256), dim3(256), 0, s, probs, w.idx.p, w.val.p, N, nc);
  CLSTM_LAUNCH(decode_kernel, dim3(bs), dim3(64), 0, s, (const int*)w.idx.p, (const float*)w.val.p,
               (const int*)w.line_off.p, cls_d, loc_d, cnt_d, conf_h ? conf_d : (float*)nullptr);
  check_launch();
  // (one transfer instead of one per array.  Measured on whole recognition calls of one line of 200 frames, before -> after this and
  //  predict's one-launch ingest: set_batch + set_inputs_d + forward + decode 199 -> 172 us per call, clstm_net_predict with conf 210 ->
  //  172 us; EXPERIMENTS 13.4)
  const size_t ncopy = (size_t)bs + (conf_h ? 3 : locs_h ? 2 : classes_h ? 1 : 0) * (size_t)N;
  HIPCHECK(hipMemcpyAsync(w.host, w.out.p, ncopy * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  memcpy(counts_h, w.host, (size_t)bs * sizeof(int));
  if (classes_h) memcpy(classes_h, w.host + bs, (size_t)N * sizeof(int));
  if (locs_h) memcpy(locs_h, w.host + bs + N, (size_t)N * sizeof(int));
  if (conf_h) memcpy(conf_h, w.host + bs + 2 * (size_t)N, (size_t)N * sizeof(float));
}

static thread_local CtcWorkspace* g_ctc_ws = nullptr;
static thread_local DecodeWorkspace* g_dec_ws = nullptr;

