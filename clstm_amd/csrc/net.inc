// net.inc -- part of clstm_hip.hip (namespace clstm): Layer and Net = the step scheduler of the fused path -- arenas per layer,
// batch geometry, forward / CTC hand-off / backward / update with every launch decision (which recurrence kernel, fused or separate
// launches, which GEMM form), the chunk tables of the in-launch weight-gradient items, reductions, the gradient exchange.
// Which kernels a layer's pass runs is decided in ONE place per layer kind, both in runtime.inc: narrow_plan for the register-resident
// layers (Net::narrow_shape reads the device, the options and the build into its shape), wide_plan for the lock-step ones (Net::wide_shape).
// forward() and predict() are the same layer loop (forward_pass, with and without save) and reserve_batch sizes the predict geometry by
// the same plan.  backward() asks for every layer's backward plan once, then is backward_softmax and per layer the recurrence, the
// weight gradient, the input deltas.  The matrix products around the recurrences -- kernel, tile, rows, slabs, the bf16 arrays a pass writes for
// them -- are decided by product_plan (runtime.inc; Net::product_shape reads the device, the options and the Layer into its shape): the passes
// here ask for a layer's ProductPlan once and switch on it.
// And the step: Net::step_plan decides a StepPlan ONCE per training step; backward(plan) returns what the pass left (PassLeft) and
// update(left) consumes it -- nothing of a step's plan is a member of Net.  The step sequence itself is step.inc.
// Not a stand-alone header: included once by clstm_hip.hip behind runtime.inc.
struct Layer {
  int ni, no, nk4, nthreads;
  bool wide = false;          // lock-step recurrence (lstm_wide.h) instead of the register-resident one
  int kpf = 0, kpb = 0;
  // padded contraction lengths of the bf16 rows and the rows of the packed bf16 weights per direction, forward | backward; bwd_exact: the
  // backward rows are exactly the 4 no gate columns (no % 32 == 0), so per-frame bf16 deltas (Dbf) can be a GEMM operand as they are
  int kp16f = 0, kp16b = 0, rowsf = 0, rowsb = 0;
  bool bwd_exact = false;
  long long nwf = 0, nwb = 0;
  PackDesc pd;
  float *Wt = nullptr, *bias = nullptr, *Rf = nullptr, *Rb = nullptr, *Rwf = nullptr, *Rwb = nullptr;
  float* Wk = nullptr;        // k-contiguous W_x rows for the producer items of the fused forward launch (ops.h:PackFused)
  int wk_kp = 0, wk_njp = 0;
  DevBuf<float> dCc;
  // minibatches that fill the chip: the recurrence batched over 16 lines on the f16 MFMA (lstm_mfma.h); fragments repacked when
  // the parameters have moved (Net::params_epoch)
  DevBuf<unsigned short> Wmf;
  DevBuf<float> mf_scale;
  DevBuf<unsigned> mf_xmax;   // partial maxima of |x| of the current minibatch (k_mfma_xmax): batched recurrence or its routed per-line twins
  long long mf_epoch = -1;
  DevBuf<unsigned short> Wmfb;   // R^T fragments of the batched backward recurrence (lstm_mfma_bwd.h)
  long long mfb_epoch = -1;
  DevBuf<int> pack_tab;       // source index of every packed element (k_pack_index), narrow layers in training steps
  DevBuf<int> pack_inv;       // ... and its inverse, PACK_KD packed elements per parameter (ops.h: PackDst); pack_inv_state: 0 not built, 1 ready, -1 unusable
  int pack_inv_state = 0;
  // bf16 recurrence of a wide layer (lstm_wide_bf16.h): packed weights and the bf16 copies of h / the deltas
  unsigned short *Rbf = nullptr, *Rbb = nullptr;
  DevBuf<unsigned short> R2b, D2;   // f32-grade backward recurrence on the bf16 MFMA (lstm_xcd_bwd_x3): hi | lo planes of the weights and of the delta ring
  bool r2b_ready = false;           // ... R2b holds the CURRENT weights (set / cleared by every repack)
  DevBuf<unsigned short> Hb, Db;
  DevBuf<float> Rf32;          // tiled lock-step ring of the persistent f32 recurrences (one pass at a time uses it)
  long long* moff = nullptr;  // [ndir*4no] flat offset of packed row m (column 0)
  DevBuf<float> G, C, H, D, dH, S;
  DevBuf<unsigned short> Hbf;  // per-frame bf16 h of both directions written by the persistent forward kernel (A operand of the next layer's W_x product)
  DevBuf<unsigned short> WtbT; // bf16 W_x, k-contiguous ([M][ni]): B operand of that product
  DevBuf<unsigned short> Sbf;  // bf16 source rows [x | h_{t-1} | 1] per direction (x: k_source_x_bf16, h: the persistent forward kernel)
  long long sbf_one_key = -1;  // batch geometry (N) the constant bias column of Sbf was written for: a cache key of that column, not a fact of a pass
  // ---- the layer record: which copies of this layer's arrays are current.  Written by the five transitions below and by Net::ensure_* (each its
  // own member) and by nothing else; read by Net::product_shape, the ensure_* functions and the forward scheduler.
  struct Current {
    bool h_f32 = true;         // the f32 outputs H (a persistent bf16 forward pass of a lower layer leaves only Hbf)
    bool sx = true;            // the [1 | x] columns of S (f32) (built lazily when the bf16 rows serve the weight gradient)
    bool sh = true;            // the h_{t-1} columns of S (f32) (a persistent bf16 forward pass may leave only Sbf)
    bool d_f32 = true;         // D, the f32 gate deltas (a persistent bf16 backward pass may leave only Dbf)
    bool hbf = false;          // Hbf: this forward pass ran the persistent kernel and it wrote Hbf
    bool sbf = false;          // Sbf: complete for this forward pass (except the x columns where ProductPlan::a2_rows says the weight-gradient
                               // GEMM reads those from the layer below's Hbf)
  } cur;
  // a saving forward pass begins; rows0: this is layer 0 and the ingest has written its [1 | x] columns already (Net::Holds::frames)
  void forward_begins(bool rows0) { cur.sx = rows0; }
  // the forward recurrence left ...: every family says so -- the per-line, batched-MFMA and fused launches store everything (all false)
  void recurrence_left(bool persistent, bool skip_h, bool skip_s, bool wrote_hbf, bool wrote_sbf) {
    cur.hbf = persistent && wrote_hbf; cur.sbf = persistent && wrote_sbf;
    cur.h_f32 = !(persistent && skip_h); cur.sh = !(persistent && skip_s);
  }
  void backward_left(bool skipped_d) { cur.d_f32 = !skipped_d; }   // the backward recurrence left the f32 deltas, or only Dbf
  // predict begins (no-save kernels: narrow layers in f32 mode): S is not written, H is; no bf16 copy is made.  Sbf is not touched, so
  // sbf_one_key stands; D is not touched, so d_f32 stands
  void predict_begins() { cur.sx = cur.sh = false; cur.h_f32 = true; cur.sbf = cur.hbf = false; }
  // clstm_net_set_states_h wrote G, C, H and S whole: the f32 arrays are current and the bf16 copies the forward pass made (Sbf, Hbf) no longer
  // match them.  Sbf's constant column is still what sbf_one_key says.  (hbf used to stay set here.  It could not feed a stale Hbf to a
  // product: the only backward reader of the layer below's Hbf is the bf16-source weight gradient -- ProductPlan::a2_rows, which asks for
  // THIS layer's sbf, cleared here on every layer -- and a forward pass runs the layer below first.  Cleared all the same: it is not true.)
  void states_set() { cur.h_f32 = cur.sx = cur.sh = true; cur.sbf = cur.hbf = false; }
  DevBuf<unsigned short> Dbf;  // per-frame bf16 gate deltas written by the persistent backward kernel (A operand of the x.d GEMM)
  DevBuf<float> dbias;         // [bs][ndir][no][4] per-line sums of those deltas (the bias row of the weight gradient), same kernel
  DevBuf<float> partial;       // stacked nets: this layer's own split-K slabs of the weight gradient (reduced behind the LAST recurrence of the pass)
  DevBuf<unsigned short> Wtb;  // bf16 copy of Wt ([ni][M], k = gate column contiguous): B operand of the bf16-source x.d product
  int lds = 0;
  int wt_slack = 32;          // floats past Wt a vectorised staging load may touch
  int ldh = 0, hofs = 4;      // H rows: [pad pad pad 1 | h_dir0 | h_dir1], h at column hofs (16-byte aligned)
  float* hrow() const { return H.p + hofs; }            // h block of frame 0
  float* srow() const { return H.p + hofs - 1; }        // [1 | h] = the next layer's / softmax's source row
};

// the backward recurrence of one layer of the current minibatch (Net::backward): with the chunked weight-gradient items of gemm_dw.h in
// or behind its launch (backward_layer_overlapped; NarrowPlan::overlapped), lock-step (lstm_wide.h), or the narrow layer's alone with the
// weight gradient as a product behind it
enum class BwdFamily { Overlapped, Wide, Narrow };

// host-side view of one minibatch as the step entries take it: line lengths, frames, packed transcripts and their lengths
struct Minibatch {
  const int* T; int bs; const float* x; const int* labels; const int* L;
  bool given() const { return T && x && labels && L && bs > 0; }
};
// frames of a minibatch whose line lengths are acceptable: every refusal line lengths can earn, made here and nowhere else
static long long batch_frames(const int* T_h, int nb) {
  REQUIRE(T_h && nb > 0, "empty batch");
  long long n = 0;
  for (int b = 0; b < nb; b++) { REQUIRE(T_h[b] >= 0, "negative line length"); n += T_h[b]; }
  REQUIRE(n > 0, "batch has no frames");
  REQUIRE(n < 2147483000LL, "batch has too many frames");   // (the line offsets are ints)
  return n;
}
// (host-fed steps) the pinned word the step's last kernel writes `id` into, and that number: Net::HostFeed::stage
struct HostTicket { int* word = nullptr; int id = 0; };
// The plan of one training step, decided once (Net::step_plan) and passed by value.  The default is the plan of separate calls:
// clstm_net_backward leaves the gradient in g, clstm_net_update exchanges it if there are ranks and launches k_update.
struct StepPlan {
  bool fuse = false;         // the update rides the slab reductions of the backward pass
  bool peer = false;         // the gradient goes into the communicator's exchange slot: update() runs the peer-read all-reduce fused with the update
  bool defer_last = false;   // the last reduction is described instead of enqueued: the next minibatch's ingest goes behind it (step.inc)
  HostTicket ticket;         // host-fed step: its last kernel publishes the step number
};
// the last reduction launch of a fused-update step, described (gates ... q) and not yet enqueued: Net::launch_deferred_reduce
struct DeferredReduce { bool armed = false; ReduceDesc gates, extra; float* gdst = nullptr; UpdateFuse uf; size_t work = 0; hipStream_t q = nullptr; };
// what a backward pass left behind for update()
struct PassLeft {
  bool update_applied = false;        // the reductions applied the update: update() has nothing left to launch
  bool packs_follow_update = false;   // ... and rewrote the packed copies of the parameters they moved
  bool peer_pending = false;          // the gradient is in the exchange slot
  DeferredReduce deferred;
  HostTicket ticket;                  // word: null once a kernel of the step has taken it
};

struct Net {
  clstm_net_desc desc;
  int ndir;
  std::vector<Layer> L;
  int sm_ni = 0;
  long long sm_off = 0;
  int nparams = 0;
  float *v = nullptr, *d = nullptr, *g = nullptr;
  bool own_v = false, own_d = false, own_g = false;
  float lr = 1e-4f, mom = 0.9f, gclip = 100.0f;
  bool packed_dirty = true;
  long long params_epoch = 0;   // bumped whenever v may have changed (set_params, params_changed, every update)
  bool bf16_gemm = false;   // hoisted gate GEMMs: bf16 in, f32 accumulate   (clstm_net_set_gemm_precision)
  bool bf16_rec = false;    // wide layers: bf16 MFMA operands in the recurrence
  bool want_dx0 = false;
  // batch
  int bs = 0, tmax = 0;
  long long N = 0;
  std::vector<int> line_off_h;
  DevBuf<int> line_off;            // [bs + 1] first frame of each line | [bs] dispatch order (set_batch)
  std::vector<int> order_h;
  PinnedRing ring;
  const int* lo_stage = nullptr;   // pinned copy of the line offsets (unsent_offsets: while they are not on the device)
  // ---- the minibatch record: which minibatch this net holds and which of its results stand.  Plain data, reported as it is by
  // clstm_debug_net_holds.  It changes through the transitions below and declare_batch / reserve_batch, all methods of Net; step.inc and
  // abi.inc call those and ask require(), and assign nothing.  (Parameters are not the minibatch's: packed_dirty, the epochs, training.)
  struct Holds {
    enum Batch { NONE, CURRENT, NEXT };       // whose geometry bs / N / tmax / line_off_h are: nobody's; the current minibatch's; a declared NEXT one's, which a
                                              // step's tail declared and ingested behind its last launch -- outputs of that minibatch do not exist
    enum Forward { NO_PASS, SAVED, NOSAVE };  // no forward pass of this minibatch yet; one that saved what a backward pass needs; predict's, which saved nothing
    enum Frames { NO_FRAMES, BLOCK, ROWS };   // its frames: nowhere; in the input block X; in X and in layer 0's source rows [1 | x]
    int batch = NONE;
    int training_buffers = 0;                 // the buffers are those of a training pass (0: the forward-only geometry of predict; reserve_batch)
    int forward = NO_PASS;
    int frames = NO_FRAMES;
    int offsets_sent = 0;                     // the line offsets and the dispatch order are on the device (or ride a launch already enqueued)
    int dx0 = 0;                              // a backward pass of this minibatch has written dX0
  } holds;
  // declared: declare_batch (resets the record; a declared next minibatch is dropped by it).  The other transitions:
  void offsets_sent(hipStream_t s) { ring.commit(s); holds.offsets_sent = 1; }   // s: the stream of the copy / the launch that reads the pinned slot
  const int* unsent_offsets() const { return holds.offsets_sent ? nullptr : lo_stage; }
  void frames_ingested(bool rows) { holds.frames = rows ? Holds::ROWS : Holds::BLOCK; }
  void forward_ran(bool saved) { holds.forward = saved ? Holds::SAVED : Holds::NOSAVE; }
  void backward_ran() { holds.dx0 = want_dx0; }
  void next_declared(const Minibatch& m) { next.remember(m); holds.batch = Holds::NEXT; }   // (by a step's tail: declared, ingested, its alignment prepared)
  bool next_is(const Minibatch& m) const { return holds.batch == Holds::NEXT && holds.frames == Holds::ROWS && holds.offsets_sent && next.matches(m); }
  void next_adopted() { if (holds.batch == Holds::NEXT) holds.batch = Holds::CURRENT; }   // the step that brings it; clstm_net_forward and clstm_net_set_inputs_*
  void states_set() { frames_ingested(true); forward_ran(true); for (auto& y : L) y.states_set(); }   // clstm_net_set_states_h wrote every array of a forward pass
  // The one guard of the per-minibatch entry points (abi.inc; the table is in include/clstm_abi.h): what the caller `who` needs of the record.
  enum Need { NEED_BATCH = 1, NEED_CURRENT = 2, NEED_SAVED = 4, NEED_BACKWARD = 8,
              NEED_OUTPUTS = NEED_BATCH | NEED_CURRENT, NEED_PASS = NEED_OUTPUTS | NEED_SAVED, NEED_DX0 = NEED_PASS | NEED_BACKWARD };
  void require(int needs, const char* who) const {
    REQUIRE(!(needs & NEED_BATCH) || holds.batch != Holds::NONE, "set_batch first");
    REQUIRE(!(needs & NEED_CURRENT) || holds.batch != Holds::NEXT, "no current minibatch: the last clstm_net_train_step_next replaced it with the declared next one (its outputs are not addressable any more)");
    REQUIRE(!(needs & NEED_SAVED) || holds.forward != Holds::NOSAVE, std::string(who) + ": the current minibatch was computed by clstm_net_predict, which saves nothing for a backward pass (run clstm_net_forward or a training step first)");
    REQUIRE(!(needs & NEED_BACKWARD) || (want_dx0 && holds.dx0), "input deltas not enabled / no backward yet");
  }
  void flush_line_off() {
    if (holds.offsets_sent) return;
    hipStream_t s = stream();
    HIPCHECK(hipMemcpyAsync(line_off.p, lo_stage, (2 * bs + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    offsets_sent(s);
  }
  DevBuf<float> X, Z, Dz, dX0, partial, partial_sm, aligned, tmp;
  DevBuf<unsigned short> xbf;   // bf16 copy of the input frames (first wide layer's W_x product in precision mode 2)
  ReduceDesc sm_red{};
  DevBuf<long long> lstm_prof;  // diagnostics build only
  StepGraphCache step_graphs;   // captured per-step launch sequences of the lock-step recurrence
  XcdSync coop_sync;          // sync words of the persistent lock-step kernels + the stamp base of their next launch
  Timing timing;
  // --- weight-gradient GEMM beside the backward recurrence (gemm_dw.h) ---
  static const int PROG_WORDS = 2 * PROG_LINES * PROG_STRIDE;   // progress words at the tail of a narrow layer's D allocation: [ndir][bs], one per 128 B
  // CLSTM_OVERLAP / clstm_net_set_overlap: 0 off (GEMM after the recurrence); 1 (default): recurrence and GEMM as two
  // roles of ONE launch (lstm_bwd_dw.h) for batches large enough -- 0.369 -> 0.356 ms per step at the bench shape;
  // 2: the same always (tests force it onto tiny nets).  (Two streams with complementary CU masks were measured
  // slower than mode 0 -- 0.443 vs 0.377 ms per step, profiles/r02_timeline_overlap.txt -- and are gone.)
  int overlap = getenv("CLSTM_OVERLAP") ? atoi(getenv("CLSTM_OVERLAP")) : 1;
  unsigned dw_done_total = 0;     // recurrence workgroups launched so far through the fused launch (GemmDwArgs::done)
  DevBuf<long long> dw_trace;
  DevBuf<int> xd_ready;           // producer form of the top layer's x.d (NarrowPlan::xd = 2): rounds-complete words of the dH items
  DevBuf<int> dw_ktab, dw_slabs, dw_queue;   // dw_queue: the monitor's published minima and the `done` counter, each on its own 128-byte line
  std::vector<int> dw_key;        // line offsets the tables were built for
  // the softmax layer's W.d as independent items of the top layer's fused backward launch (gemm_dw.h, GemmDwArgs::x*; NarrowPlan::dwx)
  DevBuf<int> dwx_tab;            // [entries][2] contiguous 16-frame entries | slabs
  long long dwx_N = -1;
  int dwx_nslabs = 0, dwx_entries = 0;
  int dw_nslabs = 0, dw_slabs_per_dir = 0, dw_ntiles_max = 0;
  int prog_base = 1024;           // grows with every backward launch: stale progress words never look complete
  long long dw_launches = 0;      // overlapped backward passes so far (tests check the path was taken)
  Comm* comm = nullptr;         // data-parallel ranks: all-reduce of g before the update (not owned)
  // --- host-fed training steps (clstm_net_train_step_h): frames travel on a copy stream into one of two device input
  // buffers while the previous step computes; the compute stream waits for the copy's event; a slot is rewritten only
  // after the step that read it has ended -- that step's update kernel says so in a pinned host word (no event record on
  // the compute stream: one costs ~5 us of stream time)
  struct HostFeed {
    hipStream_t cs = nullptr;
    hipEvent_t copied[2] = {};
    DevBuf<float> xin[2];
    PinnedBuf<char> pin[2];                // staging for pageable sources
    int* step_done = nullptr;              // pinned: number of the last step whose update kernel has run
    long long steps = 0;
    bool ready = false;
    // The slot for the next step's `nfloats` frames at x_h: waits until the step that last read it has ended, copies the frames in
    // on the copy stream and makes the compute stream wait for them.  Returns the device frames and the step's ticket.
    // The step's number (1, 2, ...) is COMMITTED (commit) only when its last kernel -- the one that publishes it in the pinned
    // word -- has been enqueued: a call that fails on the way (a bad label, a launch error) leaves `steps` where it was, so the
    // next call reuses number and slot and never waits for a step that was not enqueued (two failed calls in a row used to spin
    // here for ever).
    const float* stage(const float* x_h, size_t nfloats, HostTicket& ticket) {
      if (!ready) {
        ready = true;
        HIPCHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) HIPCHECK(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
        HIPCHECK(hipHostMalloc((void**)&step_done, 64));
        *step_done = 0;
      }
      const long long k = steps + 1;
      const int slot = (int)(k & 1);
      // the slot was read by step k - 2: its update kernel has run when the pinned word says so (the host is at most a few
      // steps ahead of the GPU, so this rarely waits).  Bounded: after ~2 s of yielding the stream is drained instead --
      // everything enqueued has then run, whatever the word says.
      {
        const auto t0 = std::chrono::steady_clock::now();
        int spins = 0;
        while (k > 2 && (int)((unsigned)(k - 2) - (unsigned)__atomic_load_n(step_done, __ATOMIC_ACQUIRE)) > 0) {   // (wrap-safe)
          sched_yield();
          if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIPCHECK(hipStreamSynchronize(g_stream));
            check_device_errors();
            break;
          }
        }
      }
      const size_t bytes = nfloats * sizeof(float);
      xin[slot].reserve(nfloats + 64);
      const void* src = x_h;
#ifndef CLSTM_HIP_EMU
      hipPointerAttribute_t attr;
      const bool pinned = hipPointerGetAttributes(&attr, x_h) == hipSuccess && attr.type == hipMemoryTypeHost;
      if (!pinned) {   // pageable memory: one host copy into the slot's pinned staging buffer, then the same DMA
        (void)hipGetLastError();
        pin[slot].reserve(bytes);
        memcpy(pin[slot].p, x_h, bytes);
        src = pin[slot].p;
      }
#endif
      HIPCHECK(hipMemcpyAsync(xin[slot].p, src, bytes, hipMemcpyHostToDevice, cs));
      HIPCHECK(hipEventRecord(copied[slot], cs));
      HIPCHECK(hipStreamWaitEvent(g_stream, copied[slot], 0));
      ticket = HostTicket{step_done, (int)(unsigned)k};
      return xin[slot].p;
    }
    void commit() { steps++; }
  } hf;
  // --- fused forward launch (lstm_fwd_fused.h): W_x GEMM producers + recurrence + softmax consumers ---
  float* W1k = nullptr;         // k-contiguous softmax rows (PackFused)
  int w1k_kps = 0;
  DevBuf<int> fw_items, fw_flags;
  std::vector<int> fw_key;      // line offsets the item lists were built for
  int fw_npitems = 0, fw_ncitems = 0, fw_chunks = 0;
  int fw_epoch = 0, fw_prog_base = 1024;
  long long fw_launches = 0;

  hipStream_t stream() const { return g_stream; }
  bool in_predict = false;      // a predict call is running: no training NaN flag (fwd_nanflag)
  size_t fixed_bytes = 0;       // device allocations of build() (clstm_net_device_bytes; the grow-only buffers count themselves: DevBuf)
  void dev_malloc(void** q, size_t bytes) { HIPCHECK(hipMalloc(q, bytes)); fixed_bytes += bytes; }

  static bool l_is_only_layer(const clstm_net_desc& ds) { return ds.nlayers == 1; }
  // source-index table of a narrow layer's per-step repack (ops.h:k_pack_index), built at first use
  int* pack_table(Layer& y) {
    if (!y.pack_tab.p) {
      const PackFused pf = pack_fused_desc(y);
      const size_t n = pack_count(y);
      y.pack_tab.reserve(n);
      CLSTM_LAUNCH(k_pack_index, dim3(nblocks(n)), dim3(256), 0, stream(), y.pack_tab.p, y.pd, pf);
      check_launch();
    }
    return y.pack_tab.p;
  }
  // the inverse of pack_table(): built once per net on the host (one synchronous read-back of the table)
  static constexpr int PACK_KD = 4;
  size_t pack_count(const Layer& y) const {
    const PackFused pf = pack_fused_desc(y);
    return (size_t)(1 + y.ni) * ndir * 4 * y.no + 2 * ((size_t)ndir * 4 * 4 * y.nk4 * y.nthreads) +
           (pf.Wk ? (size_t)ndir * pf.njp * 16 * pf.kp + (size_t)96 * pf.kps : 0);
  }
  bool pack_inverse(Layer& y) {
    if (y.pack_inv_state) return y.pack_inv_state > 0;
    const int* tab = pack_table(y);
    const size_t n = pack_count(y);
    std::vector<int> t(n);
    HIPCHECK(hipMemcpyAsync(t.data(), tab, n * sizeof(int), hipMemcpyDeviceToHost, stream()));
    HIPCHECK(hipStreamSynchronize(stream()));
    std::vector<int> inv((size_t)nparams * PACK_KD, -1), cnt(nparams, 0);
    y.pack_inv_state = 1;
    for (size_t e = 0; e < n && y.pack_inv_state > 0; e++) {
      const int si = t[e];
      if (si < 0) continue;
      if (si >= nparams || cnt[si] >= PACK_KD) { y.pack_inv_state = -1; break; }
      inv[(size_t)si * PACK_KD + cnt[si]++] = (int)e;
    }
    if (y.pack_inv_state < 0) return false;
    y.pack_inv.reserve(inv.size());
    HIPCHECK(hipMemcpyAsync(y.pack_inv.p, inv.data(), inv.size() * sizeof(int), hipMemcpyHostToDevice, stream()));
    HIPCHECK(hipStreamSynchronize(stream()));
    return true;
  }
  PackFused pack_fused_desc(const Layer& y) const {
    PackFused f{};
    if (y.Wk) { f.Wk = y.Wk; f.kp = y.wk_kp; f.njp = y.wk_njp; f.W1k = W1k; f.kps = w1k_kps; f.nc = desc.nclasses; f.sm_k = sm_ni; f.sm_off = sm_off; }
    return f;
  }
  void build(const clstm_net_desc& ds, float* pv, float* pd, float* pg) {
    desc = ds;
    REQUIRE(ds.nlayers >= 1 && ds.nlayers <= CLSTM_MAX_LAYERS, "nlayers out of range");
    REQUIRE(ds.ninput > 0 && ds.nclasses >= 2, "bad ninput/nclasses (Softmax requires no>=2, clstm.cc:399)");
    ndir = ds.unidirectional ? 1 : 2;
    static const int blockidx[4] = {2, 1, 3, 0};  // slot gi,gf,go,ci -> alphabetical WCI,WGF,WGI,WGO
    long long off = 0;
    int ni = ds.ninput;
    L.resize(ds.nlayers);
    for (int l = 0; l < ds.nlayers; l++) {
      Layer& y = L[l];
      y.ni = ni;
      y.no = ds.nhidden[l];
      REQUIRE(y.no > 0, "nhidden must be positive");
      const NarrowClass k = narrow_class(y.no);
      const bool force_wide = getenv("CLSTM_FORCE_WIDE") && atoi(getenv("CLSTM_FORCE_WIDE")) != 0;
      y.wide = !k.nk4 || force_wide;
      y.nk4 = y.wide ? 1 : k.nk4;
      y.nthreads = y.wide ? 64 : 64 * k.waves;
      // (what the x.d prologue asks of a class, not of a minibatch: its smallest workgroup covers a staging round -- lstm_xd_prologue.h)
      REQUIRE(y.wide || y.nthreads * xd_maxu(y.nk4) >= XD_UNITS, "internal: a workgroup of this class does not cover a staging round of the x.d prologue");
      y.kp16f = wide_kp16_fwd(y.no); y.kp16b = wide_kp16_bwd(y.no);
      y.rowsf = (y.no + 3) / 4 * 16; y.rowsb = (y.no + 15) / 16 * 16;
      y.bwd_exact = y.kp16b == 4 * y.no;
      y.lds = ((1 + y.ni + y.no + 15) / 16) * 16;   // source rows [1 | x | h_prev], padded to 64-byte rows
      y.ldh = ((y.hofs + ndir * y.no + 15) / 16) * 16;   // 64-byte aligned rows
      const long long blk = (long long)y.no * (1 + y.ni + y.no);
      y.pd.ni = y.ni; y.pd.no = y.no; y.pd.ndir = ndir; y.pd.nk4 = y.nk4; y.pd.nthreads = y.wide ? 0 : y.nthreads; y.pd.ku = y.wide ? 4 : k.ku;
      for (int dir = 0; dir < ndir; dir++) {
        for (int s = 0; s < 4; s++) y.pd.p_off[dir][s] = off + blockidx[s] * blk;
        off += 4 * blk;
      }
      if (ndir == 1) for (int s = 0; s < 4; s++) y.pd.p_off[1][s] = y.pd.p_off[0][s];
      ni = ndir * y.no;
    }
    sm_ni = ni;
    sm_off = off;
    off += (long long)ds.nclasses * (1 + sm_ni);
    nparams = (int)off;
    auto own = [&](float*& dst, float* given, bool& flag) {
      if (given) { dst = given; flag = false; }
      else {
        dev_malloc((void**)&dst, (size_t)nparams * sizeof(float));
        zero_fill(dst, (size_t)nparams * sizeof(float));
        flag = true;
      }
    };
    own(v, pv, own_v); own(d, pd, own_d); own(g, pg, own_g);
    for (auto& y : L) {
      const int M = ndir * 4 * y.no, KQP = 4 * y.nk4;
      dev_malloc((void**)&y.Wt, ((size_t)y.ni * M + y.wt_slack) * sizeof(float));
      zero_fill(y.Wt, ((size_t)y.ni * M + y.wt_slack) * sizeof(float));
      dev_malloc((void**)&y.bias, (size_t)M * sizeof(float));
      if (y.wide) {
        y.kpf = wide_kp_fwd(y.no); y.kpb = wide_kp_bwd(y.no);
        y.nwf = (long long)ndir * y.rowsf * y.kpf;
        y.nwb = (long long)ndir * y.rowsb * y.kpb;
        dev_malloc((void**)&y.Rwf, (size_t)(y.nwf + 4) * sizeof(float));
        dev_malloc((void**)&y.Rwb, (size_t)(y.nwb + 4) * sizeof(float));
        dev_malloc((void**)&y.Rbf, ((size_t)ndir * y.rowsf * y.kp16f + 8) * sizeof(unsigned short));
        dev_malloc((void**)&y.Rbb, ((size_t)ndir * y.rowsb * y.kp16b + 8) * sizeof(unsigned short));
      } else {
        dev_malloc((void**)&y.Rf, (size_t)ndir * 4 * KQP * y.nthreads * sizeof(float));
        dev_malloc((void**)&y.Rb, (size_t)ndir * 4 * KQP * y.nthreads * sizeof(float));
      }
      if (!y.wide && l_is_only_layer(ds) && ds.nclasses <= SMX_COLS) {
        y.wk_kp = (y.ni + 15) / 16 * 16; y.wk_njp = (4 * y.no + 15) / 16;
        dev_malloc((void**)&y.Wk, ((size_t)ndir * y.wk_njp * 16 * y.wk_kp + 64) * sizeof(float));
        w1k_kps = (ndir * y.no + 15) / 16 * 16;
        dev_malloc((void**)&W1k, ((size_t)96 * w1k_kps + 64) * sizeof(float));
      }
      dev_malloc((void**)&y.moff, (size_t)M * sizeof(long long));
      std::vector<long long> mo(M);
      for (int m = 0; m < M; m++) {
        const int dir = m / (4 * y.no), c = (m % (4 * y.no)) >> 2, s = m & 3;
        mo[m] = y.pd.p_off[dir][s] + c;
      }
      HIPCHECK(hipMemcpy(y.moff, mo.data(), (size_t)M * sizeof(long long), hipMemcpyHostToDevice));
    }
    packed_dirty = true;
  }
  ~Net() {
    for (auto& y : L) {
      (void)hipFree(y.Wt); (void)hipFree(y.bias); (void)hipFree(y.Rf); (void)hipFree(y.Rb); (void)hipFree(y.moff); (void)hipFree(y.Wk);
      (void)hipFree(y.Rwf); (void)hipFree(y.Rwb); (void)hipFree(y.Rbf); (void)hipFree(y.Rbb); y.dCc.release(); y.Hb.release(); y.Db.release(); y.Rf32.release(); y.R2b.release(); y.D2.release();
      y.G.release(); y.C.release(); y.H.release(); y.D.release(); y.dH.release(); y.S.release(); y.Sbf.release(); y.pack_tab.release(); y.pack_inv.release(); y.Wmf.release(); y.mf_scale.release(); y.mf_xmax.release(); y.Wmfb.release(); y.pack_inv_state = 0; y.partial.release(); y.dbias.release();
    }
    (void)hipFree(W1k); fw_items.release(); fw_flags.release();
    for (int i = 0; i < 2; i++) { hf.xin[i].release(); if (hf.copied[i]) (void)hipEventDestroy(hf.copied[i]); }
    if (hf.step_done) (void)hipHostFree(hf.step_done);
    if (hf.cs) (void)hipStreamDestroy(hf.cs);
    if (own_v) (void)hipFree(v);
    if (own_d) (void)hipFree(d);
    if (own_g) (void)hipFree(g);
    line_off.release(); X.release(); Z.release(); Dz.release();
    dX0.release(); partial.release(); partial_sm.release(); coop_sync.words.release(); lstm_prof.release(); aligned.release(); tmp.release();
  }

  void repack() {
    if (!packed_dirty) return;
    hipStream_t s = stream();
    for (auto& y : L) {
      const int M = ndir * 4 * y.no, KQP = 4 * y.nk4;
      const size_t nr = y.wide ? 0 : (size_t)ndir * 4 * KQP * y.nthreads;
      if (product_plan(product_shape((int)(&y - L.data()), PP_FWD)).tiled_pack) {
        // every bf16-mode copy of the layer in one tiled pass (ops.h:k_pack_wide_tiles)
        y.Wtb.reserve((size_t)y.ni * M + 64);
        y.WtbT.reserve((size_t)y.ni * M + 64);
        const unsigned nblk = (unsigned)ndir * (unsigned)((y.ni + y.no) / 32) * (unsigned)(y.no / 32);
        CLSTM_LAUNCH(k_pack_wide_tiles, dim3(nblk), dim3(256), 0, s, (const float*)v, y.pd, y.Wt, y.bias, y.Wtb.p, y.WtbT.p, y.Rbf, y.Rbb, y.kp16f, y.kp16b, y.rowsf, y.rowsb);
        continue;
      }
      if (y.wide && bf16_rec) {
        CLSTM_LAUNCH(k_pack_wide_bf16, dim3(nblocks((size_t)ndir * ((size_t)y.rowsf * y.kp16f + (size_t)y.rowsb * y.kp16b))), dim3(256), 0, s,
                     (const float*)v, y.Rbf, y.Rbb, y.pd, y.rowsf, y.kp16f, y.rowsb, y.kp16b);
      }
      else if (y.wide) {
        CLSTM_LAUNCH(k_pack_wide, dim3(nblocks((size_t)(y.nwf + y.nwb))), dim3(256), 0, s, (const float*)v, y.Rwf, y.Rwb,
                     y.pd, y.kpf, y.kpb);
        y.r2b_ready = false;
        if (rec_x3()) {   // hi | lo planes of the backward recurrence's weights
          y.r2b_ready = true;
          const long long pb = (long long)ndir * y.rowsb * y.kp16b;
          y.R2b.reserve((size_t)2 * pb + 64);
          CLSTM_LAUNCH(k_pack_wide_split, dim3(nblocks((size_t)pb)), dim3(256), 0, s, (const float*)v, y.R2b.p, y.pd, y.rowsb, y.kp16b, pb);
        }
      }
      CLSTM_LAUNCH(k_pack_layer, dim3(nblocks((size_t)(1 + y.ni) * M + 2 * nr)), dim3(256), 0, s, (const float*)v, y.Wt,
                   y.bias, y.Rf, y.Rb, y.pd, pack_fused_desc(y));
      if (y.wide && bf16_rec) {   // bf16 copy of W_x^T for the bf16-source x.d product
        y.Wtb.reserve((size_t)y.ni * M + 64);
        CLSTM_LAUNCH(k_to_bf16, dim3(nblocks((size_t)y.ni * M)), dim3(256), 0, s, (const float*)y.Wt, y.Wtb.p, (size_t)y.ni * M);
        y.WtbT.reserve((size_t)y.ni * M + 64);
        CLSTM_LAUNCH(k_transpose_to_bf16, dim3(nblocks((size_t)y.ni * M)), dim3(256), 0, s, (const float*)y.Wt, y.WtbT.p, y.ni, M);
      }
    }
    check_launch();
    packed_dirty = false;
  }

  void set_batch(const int* T_h, int nb) { declare_batch(T_h, nb); reserve_batch(false); }
  void set_batch_predict(const int* T_h, int nb) { declare_batch(T_h, nb); reserve_batch(true); }   // forward-only geometry (clstm_net_predict)
  // a minibatch declared by predict that something else now wants to train on / write into: the buffers of a training pass
  void ensure_training_buffers() { if (holds.batch != Holds::NONE && !holds.training_buffers) reserve_batch(false); }
  // no-save kernels exist for narrow layers in f32 mode (lstm_seq.h, lstm_fwd_fused.h, lstm_mfma.h); a net with a wide layer
  // (lstm_wide.h) or in a bf16 mode runs the unchanged forward pass under predict
  bool predict_nosave_ok() const {
    if (bf16_gemm || bf16_rec) return false;
    for (auto& y : L) if (y.wide) return false;
    return true;
  }
  // T_h / nb are validated BEFORE the net is touched: a refused declaration leaves the previous minibatch the current one
  void declare_batch(const int* T_h, int nb) {
    const long long n = batch_frames(T_h, nb);
    holds = Holds{};   // (whatever a step's tail had prepared is replaced by this declaration)
    holds.batch = Holds::CURRENT;
    bs = nb;
    line_off_h.assign(nb + 1, 0);
    for (int b = 0; b < nb; b++) line_off_h[b + 1] = line_off_h[b] + T_h[b];
    N = n;
    tmax = 0;
    for (int b = 0; b < nb; b++) tmax = std::max(tmax, T_h[b]);
    // behind the offsets: the order in which the per-line workgroups take the lines -- longest first, so that when
    // there are more lines than CUs the long ones are not the last to start (stable: equal lengths keep their order)
    order_h.resize(nb);
    for (int b = 0; b < nb; b++) order_h[b] = b;
    std::stable_sort(order_h.begin(), order_h.end(), [&](int x, int y) { return T_h[x] > T_h[y]; });
    line_off.reserve(2 * nb + 1);
    int* stage = (int*)ring.acquire((2 * nb + 1) * sizeof(int));
    memcpy(stage, line_off_h.data(), (nb + 1) * sizeof(int));
    memcpy(stage + nb + 1, order_h.data(), nb * sizeof(int));
    // The device copy is made by the next input-ingest launch (which reads the pinned slot directly: one DMA
    // launch of ~4 us less per step) or, if something else needs it first, by flush_line_off().
    lo_stage = stage;
  }
  // predict: only what a forward-only pass writes -- the input block, H, Z and, for the families that stage pre-activations in
  // it (every one but the batched-MFMA recurrence of an upper layer; layer 0's routed twins stage theirs there when the device
  // finds |x| > 255), G.  No C, S, D, dH, Dz.  A net that has no no-save kernels (predict_nosave_ok) reserves everything.
  // (By the layer's forward plan, as forward_pass launches: the fused launch's rule looks at H, which grows here, but it stages like the per-line kernels.)
  void reserve_batch(bool predict) {
    if (predict && !predict_nosave_ok()) predict = false;
    holds.training_buffers = !predict;
    hipStream_t s = stream();
    X.reserve((size_t)N * desc.ninput);
    for (auto& y : L) {
      const NarrowPlan np = forward_plan((int)(&y - L.data()), false);
      const bool mf_full = predict && np.saves;   // (the training-form kernel under predict: it writes G, C, S)
      const bool mf_upper = predict && &y != &L[0] && np.fwd == NF_MFMA && !mf_full;
      if (!mf_upper) y.G.reserve((size_t)N * ndir * 4 * y.no);
      if (!predict || mf_full) y.C.reserve((size_t)N * ndir * y.no);
      {
        const size_t cap0 = y.H.cap;
        y.H.reserve((size_t)N * y.ldh + 64 + (y.Wk ? PROG_WORDS : 0));   // (fused forward: progress words behind the rows)
        if (y.H.cap != cap0) {
          const size_t rows = (y.H.cap - (y.Wk ? PROG_WORDS + 64 : 0)) / y.ldh;
          CLSTM_LAUNCH(k_fill_col0, dim3(nblocks(rows)), dim3(256), 0, s, y.H.p, rows, y.ldh, y.hofs - 1);
        }
      }
      if (mf_full) y.S.reserve((size_t)N * ndir * y.lds + 64);
      if (predict) continue;
      y.D.reserve((size_t)N * ndir * 4 * y.no + (y.wide ? 0 : PROG_WORDS + 64));
      y.dH.reserve((size_t)N * ndir * y.no);
      if (y.wide && bf16_rec) reserve_wide_rings(y);
      y.S.reserve((size_t)N * ndir * y.lds + 64);
    }
    Z.reserve((size_t)N * desc.nclasses);
    if (!predict) Dz.reserve((size_t)N * desc.nclasses);
  }

  // bf16 operand copies of a wide layer in precision mode 2: the lock-step rings [step parity][dir][line][k] (lstm_wide.h); never
  // smaller than the per-frame layout of the first version
  void reserve_wide_rings(Layer& y) {
    y.Hb.reserve((size_t)std::max<long long>(N, 4LL * bs + 32) * ndir * y.kp16f + 64);   // (2 x whole 16-line blocks: the tiled ring of the persistent kernels)
    y.Db.reserve((size_t)std::max<long long>(N, 2LL * bs + 32) * ndir * y.kp16b + 64);
  }
  // workgroups of the ingest of frames at x -- k_ingest_pack's leading blocks, the IngestTail's.  (The 16-byte form -- ops.h:
  // k_ingest_pack -- has one item per four input floats: launching a thread per float there dispatched 1,800 workgroups that found
  // nothing to do)
  int ingest_blocks(const float* x) const {
    const Layer& y = L[0];
    const bool vec16 = (y.ni & 3) == 0 && (y.lds & 3) == 0 && ((size_t)x & 15) == 0;
    return nblocks(vec16 ? (size_t)N * (y.ni / 4 + 1) : (size_t)N * (1 + y.ni));
  }

  const float* layer_input(int l) const { return l == 0 ? X.p : L[l - 1].hrow(); }
  int layer_input_ld(int l) const { return l == 0 ? desc.ninput : L[l - 1].ldh; }
  int layer_input_slack(int l) const { return 32; }   // X and H are over-allocated by >= 64 floats

  // ---- the products: what product_plan (runtime.inc) decides from, read HERE and nowhere else -- the device, the net's settings, the experiment
  // options (per pass: tests switch them inside one process), the layer's recurrence plan and the facts earlier launches left in the Layer
  ProductShape product_shape(int l, int pass, const NarrowPlan& np = NarrowPlan{}) const {
    const Layer& y = L[l];
    ProductShape h{};
    h.pass = pass; h.ni = y.ni; h.no = y.no; h.ndir = ndir; h.wide = y.wide;
    h.first = l == 0; h.top = l + 1 == (int)L.size(); h.nlayers = (int)L.size();
    h.bwd_exact = y.bwd_exact; h.kp16f_is_no = y.kp16f == y.no;
    h.N = (int)N; h.bs = bs; h.nclasses = desc.nclasses; h.sm_ni = sm_ni;
    h.precision = bf16_rec ? 2 : bf16_gemm ? 1 : 0; h.gemm_x3_on = gemm_x3_on; h.split_terms = split_terms; h.strict = strict_f32;
    h.gemm_b16mc = dbg_opt("gemm_b16mc") != 0; h.gemm_stag = dbg_opt("gemm_stag"); h.pack_tiles = dbg_opt("pack_tiles") != 0; h.fuse_wx = dbg_opt("fuse_wx");
    h.ncu = device_cu_count(); h.want_dx0 = want_dx0;
    h.fwd_family = np.fwd; h.overlapped = np.overlapped; h.dwx = np.dwx; h.xd = np.xd;
    h.dw_slabs_per_dir = dw_slabs_per_dir; h.dwx_nslabs = dwx_nslabs;
    h.below_hbf = l > 0 && L[l - 1].cur.hbf; h.fwd_sbf = y.cur.sbf;
    h.packs = y.WtbT.p && y.Wtb.p; h.above_packs = !h.top && L[l + 1].WtbT.p;
    return h;
  }
  // what wide_plan decides from, read here: the device, the environment, the options (each per pass: tests switch them inside one process)
  WideShape wide_shape(const Layer& y, bool fwd, const ProductPlan& pp, bool fx = false) const {
    WideShape h{};
    h.fwd = fwd; h.no = y.no; h.x_ni = y.ni; h.ndir = ndir; h.bs = bs; h.tmax = tmax; h.N = (int)N;
    h.kp = fwd ? y.kpf : y.kpb; h.kp16 = fwd ? y.kp16f : y.kp16b;
    h.bf16 = bf16_rec; h.x3 = !fwd && rec_x3() && y.r2b_ready; h.fx_mode = fx ? pp.fx_mode : 0;
    h.ncu = device_cu_count();
    h.xcd_on = !(getenv("CLSTM_XCD_REC") && atoi(getenv("CLSTM_XCD_REC")) == 0);
    h.xcd_failed = g_xcd_failed;
    h.c32_on = dbg_opt("bwd_c32") != 0;
    h.sbf = (pp.writes & PW_SBF) != 0; h.sbf_ld = y.ni + y.no + 8; h.lds = y.lds; h.ldh = y.ldh;
    return h;
  }
  LstmWideArgs wide_args(Layer& y, bool fwd, const ProductPlan& pp) {   // (the bf16 arrays the pass writes and the f32 stores it skips: the plan's)
    REQUIRE((double)N * ndir * 4 * y.no * 4 < 2147483000.0,
            "minibatch too large for the lock-step recurrence (frames x 4 x nhidden x ndir x 4 B must stay below 2 GiB)");
    LstmWideArgs w{};
    w.Rw = fwd ? y.Rwf : y.Rwb; w.rw_elems = fwd ? y.nwf : y.nwb;
    w.G = y.G.p; w.C = y.C.p; w.H = y.H.p; w.dH = y.dH.p; w.D = y.D.p;
    y.dCc.reserve((size_t)bs * ndir * y.no);
    w.dC = y.dCc.p; w.line_off = line_off.p; w.S = y.S.p; w.sdir = (long long)N * y.lds; w.N = N;
    w.lds = y.lds; w.sofs = 1 + y.ni; w.ldh = y.ldh; w.hofs = y.hofs; w.no = y.no; w.ndir = ndir; w.bs = bs;
    w.kp = fwd ? y.kpf : y.kpb; w.tmax = tmax;
    if (!bf16_rec) { y.Rf32.reserve(ring32_floats(ndir, bs, std::max(y.kpf, y.kpb)) + 64); w.Rf = y.Rf32.p; }
    if (!bf16_rec && !fwd && rec_x3() && y.r2b_ready) {   // (wide_plan's x3: planned instead of the f32 kernel)
      const int nblk = (bs + 15) / 16;
      w.kp16 = y.kp16b;
      w.ring_plane = 2LL * ndir * nblk * 16 * w.kp16;
      y.D2.reserve((size_t)2 * w.ring_plane + 64);
      w.Db = y.D2.p; w.Rw16 = y.R2b.p; w.rw_plane = (long long)ndir * y.rowsb * w.kp16;
    }
    if (bf16_rec) {
      w.Rw16 = fwd ? y.Rbf : y.Rbb;
      w.kp16 = fwd ? y.kp16f : y.kp16b;
      w.rw_elems = (long long)ndir * (fwd ? y.rowsf : y.rowsb) * w.kp16;
      w.Hb = y.Hb.p; w.Db = y.Db.p;
      if (pp.writes & PW_DBF) {
        y.Dbf.reserve((size_t)N * ndir * w.kp16 + 64); w.Dbf = y.Dbf.p;
        y.dbias.reserve((size_t)bs * ndir * 4 * y.no + 64); w.dbias = y.dbias.p;   // per-line bias-gradient sums (lstm_wide.h: LstmWideArgs::dbias)
      }
      if (pp.writes & PW_SBF) {
        const int ldsb = y.ni + y.no + 8;
        { const size_t cap0 = y.Sbf.cap; y.Sbf.reserve((size_t)N * ndir * ldsb + 64); if (y.Sbf.cap != cap0) y.sbf_one_key = -1; }
        w.Sbf = y.Sbf.p; w.sbf_ld = ldsb; w.sbf_ofs = y.ni; w.sbf_dir = (long long)N * ldsb;
      }
      if (pp.writes & PW_HBF) { y.Hbf.reserve((size_t)N * ndir * y.no + 64); w.Hbf = y.Hbf.p; w.hbf_ld = ndir * y.no; }
      w.skip_h = (pp.skips & PS_H) != 0; w.skip_s = (pp.skips & PS_S) != 0; w.skip_d = (pp.skips & PS_D) != 0;
    }
#ifdef CLSTM_LSTM_PROF
    lstm_prof.reserve(128); w.prof = lstm_prof.p;    // (the last pass launched before clstm_debug_lstm_cycles is what it reads)
#endif
    w.sync = coop_sync.reserve();
    return w;
  }

  void ensure_delta_f32(int l) {
    Layer& y = L[l];
    if (y.cur.d_f32) return;
    CLSTM_LAUNCH(k_bf16_to_f32, dim3(nblocks((size_t)N * ndir * 4 * y.no)), dim3(256), 0, stream(), y.Dbf.p, y.D.p, (size_t)N * ndir * 4 * y.no);
    y.cur.d_f32 = true;
  }
  void ensure_h_f32(int l) {   // exact: the kernel's own h = tanh(c) * go (ops.h:k_h_from_state)
    Layer& y = L[l];
    if (y.cur.h_f32) return;
    CLSTM_LAUNCH(k_h_from_state, dim3(nblocks((size_t)N * ndir * y.no)), dim3(256), 0, stream(), y.H.p, (const float*)y.G.p, (const float*)y.C.p,
                 (size_t)N, y.no, ndir, y.ldh, y.hofs);
    y.cur.h_f32 = true;
  }
  void ensure_source_h(int l) {
    Layer& y = L[l];
    if (y.cur.sh) return;
    ensure_h_f32(l);
    flush_line_off();
    CLSTM_LAUNCH(k_source_h, dim3(nblocks((size_t)N * ndir * y.no)), dim3(256), 0, stream(), y.S.p, (const float*)y.H.p, (const int*)line_off.p, bs,
                 (size_t)N, y.no, ndir, y.ldh, y.hofs, y.lds, 1 + y.ni, (long long)N * y.lds);
    y.cur.sh = true;
  }
  void ensure_source(int l) { ensure_source_x(l); ensure_source_h(l); }   // whole f32 source rows [1 | x | h_prev]
  void ensure_source_x(int l) {
    Layer& y = L[l];
    if (y.cur.sx) return;
    if (l > 0) ensure_h_f32(l - 1);   // (reads the layer below's f32 outputs)
    hipStream_t s = stream();
    timing.begin("build_source", s);
    CLSTM_LAUNCH(k_build_source, dim3(nblocks((size_t)N * (1 + y.ni))), dim3(256), 0, s, y.S.p, layer_input(l),
                 (size_t)N, y.ni, layer_input_ld(l), y.lds, ndir, (long long)N * y.lds);
    timing.end(s);
    y.cur.sx = true;
  }

  // ---- narrow layers: what narrow_plan (runtime.inc) decides from, read HERE and nowhere else -- the device, the net's settings, the
  // experiment options (each per pass: tests switch them inside one process; a forward pass reads fwd_mfma, a backward pass the other
  // three) and whether this is the host emulator build
  NarrowShape narrow_shape(int l, int pass) const {
    const Layer& y = L[l];
    NarrowShape h{};
    h.pass = pass; h.no = y.no; h.ni = y.ni; h.ndir = ndir;
    h.nlayers = (int)L.size(); h.first = l == 0; h.top = l + 1 == (int)L.size();
    h.bs = bs; h.tmax = tmax; h.N = (int)N; h.nc = desc.nclasses;
    h.ldh = y.ldh; h.lds = y.lds; h.ldx = layer_input_ld(l);
    h.h_cap = (int)std::min<size_t>(y.H.cap, 2147483647); h.d_cap = (int)std::min<size_t>(y.D.cap, 2147483647);
    h.wk = y.Wk != nullptr; h.wk_njp = y.wk_njp; h.w1k_kps = w1k_kps;
    h.overlap = overlap; h.bf16_gemm = bf16_gemm; h.strict_f32 = strict_f32;
    h.dw_x3 = dw_x3; h.split_terms = split_terms;
    if (pass != NP_BWD) h.fwd_mfma = dbg_opt("fwd_mfma");
    else { h.bwd_mfma = dbg_opt("bwd_mfma"); h.bwd_mfma_fused = dbg_opt("bwd_mfma_fused"); h.xd_prologue = dbg_opt("xd_prologue"); }
    h.ncu = device_cu_count();
#ifdef CLSTM_HIP_EMU
    h.emu = 1;
#endif
    return h;
  }
  // the plan of layer l's forward / backward pass; of a wide layer: none (fwd NF_NONE, bwd NB_NONE, nothing rides its launch)
  NarrowPlan forward_plan(int l, bool save) const { return L[l].wide ? NarrowPlan{} : narrow_plan(narrow_shape(l, save ? NP_FWD_SAVE : NP_FWD_NOSAVE)); }
  NarrowPlan backward_plan_narrow(int l) const { return L[l].wide ? NarrowPlan{} : narrow_plan(narrow_shape(l, NP_BWD)); }
#ifndef CLSTM_HIP_EMU
  template <int NO, int NI, bool SAVE = true>
  void launch_mfma_no(Layer& y, hipStream_t s) {
    using Gm = MfmaGeom<NO, NI, SAVE>;
    const int l = (int)(&y - L.data());
    if (y.mf_epoch != params_epoch) {
      y.Wmf.reserve((size_t)ndir * Gm::W_HALFS_PER_DIR + 64);
      y.mf_scale.reserve(8);
      MfmaPackArgs p{};
      p.v = v; p.ni = y.ni; p.no = y.no; p.nt = Gm::NT; p.kb = Gm::KB; p.W = y.Wmf.p; p.inv_scale = y.mf_scale.p;
      for (int d = 0; d < 2; d++) for (int q = 0; q < 4; q++) p.p_off[d][q] = y.pd.p_off[d][q];
      CLSTM_LAUNCH(k_pack_mfma, dim3(32, (unsigned)ndir), dim3(1024), 0, s, p);
      y.mf_epoch = params_epoch;
    }
    LstmMfmaArgs a{};
    a.W = y.Wmf.p; a.inv_scale = y.mf_scale.p; a.G = y.G.p; a.C = y.C.p; a.H = y.H.p; a.S = y.S.p; a.dH = y.dH.p; a.D = y.D.p;
    a.line_off = line_off.p; a.order = line_off.p + bs + 1; a.bs = bs; a.ndir = ndir; a.ldh = y.ldh; a.hofs = y.hofs;
    a.lds = y.lds; a.sofs = 1 + y.ni; a.sdir = (long long)N * y.lds; a.N = N;
    a.X = layer_input(l); a.ldx = layer_input_ld(l); a.store_s = 1;
    if (!SAVE) { a.G = a.C = a.S = nullptr; a.dH = nullptr; a.D = nullptr; a.store_s = 0; }   // (not addressed by the no-save form)
    if (l == 0) {   // the caller's frames, any magnitude: the device decides between this kernel and its routed twins (lstm_mfma.h: Input range)
      y.mf_xmax.reserve(MF_XMAX_SLOTS);
      CLSTM_LAUNCH(k_mfma_xmax, dim3(MF_XMAX_SLOTS), dim3(256), 0, s, (const float*)X.p, (size_t)N * desc.ninput, y.mf_xmax.p);
      a.xmax = y.mf_xmax.p;
    }
#ifdef CLSTM_LSTM_PROF
    lstm_prof.reserve(128); a.prof = lstm_prof.p;
#endif
    allow_dynamic_lds((const void*)lstm_fwd_mfma_kernel<NO, NI, SAVE>, (size_t)Gm::SMEM);
    CLSTM_LAUNCH((lstm_fwd_mfma_kernel<NO, NI, SAVE>), dim3((unsigned)((bs + 15) / 16), (unsigned)ndir), dim3(512), (size_t)Gm::SMEM, s, a);
    if (l == 0) launch_routed_per_line(y, s, SAVE);
  }
  // the per-line forward pass of layer 0 (hoisted f32 W_x.x product + lstm_seq.h recurrence, as forward() launches them for
  // smaller minibatches) behind the branch that lets it run only when the batched kernel has declined the minibatch
  template <int NK4, int KU>
  void launch_routed_lstm(Layer& y, const LstmSeqArgs& a, hipStream_t s, bool save) {
    const size_t smem = (2 * 4 * (size_t)lstm_qstride(NK4) + 4) * sizeof(float);
    if (save) CLSTM_LAUNCH((lstm_fwd_routed_kernel<NK4, KU>), dim3(bs, ndir), dim3(y.nthreads), smem, s, a, (const unsigned*)y.mf_xmax.p, dev_err_words() + 8);
    else CLSTM_LAUNCH((lstm_fwd_routed_kernel<NK4, KU, false>), dim3(bs, ndir), dim3(y.nthreads), smem, s, a, (const unsigned*)y.mf_xmax.p, dev_err_words() + 8);
  }
  void launch_routed_per_line(Layer& y, hipStream_t s, bool save = true) {
    const int M = ndir * 4 * y.no;
    const int ksplit = (y.ni + GEMM_BK - 1) / GEMM_BK * GEMM_BK;
    const unsigned gx = (unsigned)((M + GEMM_BT - 1) / GEMM_BT), gy = (unsigned)((N + GEMM_BT - 1) / GEMM_BT);
    CLSTM_LAUNCH((gemm_f32_routed_kernel<GEMM_KC, GEMM_MC, StoreBias>), dim3(std::min(gx * gy, 2048u)), dim3(256), 0, s,
                 gemm_kc(layer_input(0), layer_input_ld(0), N), gemm_mc(y.Wt, M, y.ni, 0), StoreBias{y.G.p, M, y.bias}, (int)N, M, y.ni, ksplit,
                 gx, gy, (const unsigned*)y.mf_xmax.p);
    const LstmSeqArgs a = seq_args(y, true, save);
    narrow_dispatch<NCAP_ROUTED>(y.nk4, y.pd.ku, [&](auto c) { launch_routed_lstm<decltype(c)::NK4, decltype(c)::KU>(y, a, s, save); });
  }
#endif
  // the argument block of the per-line recurrence kernels (lstm_seq.h) for one layer and pass; save = false: C and S stay null
  // -- the no-save kernels do not address them and the predict geometry does not have them.  No progress words (prog_off = -1);
  // the launches that overlap consumers with the recurrence set theirs.
  LstmSeqArgs seq_args(const Layer& y, bool fwd, bool save = true) const {
    LstmSeqArgs a{};
    a.Rpk = fwd ? y.Rf : y.Rb; a.G = y.G.p; a.C = save ? y.C.p : nullptr; a.H = y.H.p; a.dH = fwd ? nullptr : y.dH.p; a.D = fwd ? nullptr : y.D.p;
    a.line_off = line_off.p; a.order = line_off.p + bs + 1; a.no = y.no; a.ndir = ndir; a.bs = bs; a.ldh = y.ldh; a.hofs = y.hofs;
    a.S = save ? y.S.p : nullptr; a.lds = y.lds; a.sofs = 1 + y.ni; a.sdir = (long long)N * y.lds;
    a.prog_off = -1; a.prog_base = 0;
    return a;
  }
#ifndef CLSTM_HIP_EMU
  // argument block of the batched backward kernels from the per-line one; the R^T fragments repacked when the parameters have moved
  template <int NO, int NT>
  LstmMfmaBwdArgs mfma_bwd_args(Layer& y, const LstmSeqArgs& sa, hipStream_t s) {
    using Gm = MfmaBwdGeom<NO, NT>;
    if (y.mfb_epoch != params_epoch) {
      y.Wmfb.reserve((size_t)ndir * Gm::W_HALFS_PER_DIR + 64);
      MfmaBwdPackArgs p{};
      p.v = v; p.ni = y.ni; p.no = y.no; p.ntl = Gm::NTL; p.kb = Gm::KB; p.nt = NT; p.W = y.Wmfb.p;
      for (int d = 0; d < 2; d++) for (int q = 0; q < 4; q++) p.p_off[d][q] = y.pd.p_off[d][q];
      CLSTM_LAUNCH(k_pack_mfma_bwd, dim3(64, (unsigned)ndir), dim3(256), 0, s, p);
      y.mfb_epoch = params_epoch;
    }
    LstmMfmaBwdArgs a{};
    a.W = y.Wmfb.p; a.G = sa.G; a.C = sa.C; a.dH = sa.dH; a.D = sa.D; a.line_off = sa.line_off; a.order = sa.order;
    a.bs = bs; a.ndir = ndir; a.N = N; a.prog_off = sa.prog_off; a.prog_base = sa.prog_base;
    return a;
  }
  template <int NO>
  void launch_mfma_bwd_no(Layer& y, const LstmSeqArgs& sa, hipStream_t s) {
    constexpr int NT = 2;
    using Gr = MfmaBwdRowsGeom<NO, NT>;
    const LstmMfmaBwdArgs a = mfma_bwd_args<NO, NT>(y, sa, s);
    allow_dynamic_lds((const void*)lstm_bwd_mfma_rows_kernel<NO, NT>, (size_t)Gr::SMEM);
    CLSTM_LAUNCH((lstm_bwd_mfma_rows_kernel<NO, NT>), dim3((unsigned)((bs + 15) / 16), (unsigned)ndir), dim3(512), (size_t)Gr::SMEM, s, a);
  }
  // ... and as ONE launch with the weight-gradient items (lstm_mfma_bwd_dw.h), whose items are instantiated for three split terms
  template <int NO>
  void launch_mfma_bwd_dw_no(Layer& y, const LstmSeqArgs& sa, const GemmDwArgs& g, unsigned ngemm, hipStream_t s) {
    constexpr int NT = 2;
    using Gr = MfmaBwdRowsGeom<NO, NT>;
    const LstmMfmaBwdArgs a = mfma_bwd_args<NO, NT>(y, sa, s);
    const int ngroups = (bs + 15) / 16, nrec = ngroups * ndir;
    allow_dynamic_lds((const void*)lstm_bwd_mfma_dw_kernel<NO, NT, 3>, (size_t)Gr::SMEM);
    CLSTM_LAUNCH((lstm_bwd_mfma_dw_kernel<NO, NT, 3>), dim3((unsigned)nrec + ngemm), dim3(512), (size_t)Gr::SMEM, s, a, g, nrec, ngroups);
  }
#endif
  // the batched forward recurrence of the plan (lstm_mfma.h), in its saving or its no-save form
  void launch_mfma(Layer& y, hipStream_t s, bool save) {
#ifndef CLSTM_HIP_EMU
    if (save) mfma_dispatch<MCAP_FWD>(y.no, [&](auto no) { launch_mfma_no<decltype(no)::value, 48>(y, s); });
    else mfma_dispatch<MCAP_NOSAVE>(y.no, [&](auto no) { launch_mfma_no<decltype(no)::value, 48, false>(y, s); });
#else
    (void)y; (void)s; (void)save; no_instantiation();
#endif
  }
  // ... and the batched backward recurrence (lstm_mfma_bwd.h): alone, or (g) as one launch with the weight-gradient items
  void launch_mfma_bwd(Layer& y, const LstmSeqArgs& a, hipStream_t s, const GemmDwArgs* g = nullptr, unsigned ngemm = 0) {
#ifndef CLSTM_HIP_EMU
    mfma_dispatch<MCAP_BWD>(y.no, [&](auto no) {
      if (g) launch_mfma_bwd_dw_no<decltype(no)::value>(y, a, *g, ngemm, s); else launch_mfma_bwd_no<decltype(no)::value>(y, a, s);
    });
#else
    (void)y; (void)a; (void)s; (void)g; (void)ngemm; no_instantiation();
#endif
  }
  // the narrow layer's backward recurrence alone, in the plan's form: batched over lines on the MFMA, one workgroup per line, or that with
  // the softmax layer's x.d as the prologue of every workgroup (xd: the top layer where NarrowPlan::xd = 1 meets the two-launch form)
  void launch_bwd_narrow(Layer& y, const NarrowPlan& np, const LstmSeqArgs& a, hipStream_t s, const XdArgs* xd = nullptr) {
    if (np.bwd == NB_LINE_XD_DW) launch_lstm_bwd_xd(y.nk4, y.pd.ku, a, *xd, np.terms, bs, y.nthreads, s);
    else if (np.bwd == NB_MFMA || np.bwd == NB_MFMA_THEN_DW) launch_mfma_bwd(y, a, s);
    else launch_lstm(false, y.nk4, y.pd.ku, a, bs, y.nthreads, s);
  }

  void forward() {
    RoctxRange range_("clstm:forward");
    ensure_training_buffers();   // (a minibatch that clstm_net_predict declared)
    forward_pass(true);
    forward_ran(true);
  }
  // The forward pass of training (save) and of recognition (!save: predict, on its own geometry).  Every layer runs the family
  // its plan names (narrow_plan / wide_plan), in the form NarrowPlan::saves names; without save nothing is kept for a backward pass -- no C, no source
  // rows S (ensure_source_x is never called), G only as staging -- and the per-layer validity flags are left as predict set them.
  // Wide layers and the bf16 modes exist with save only (predict_nosave_ok).
  void forward_pass(bool save) {
    flush_line_off();
    repack();
    hipStream_t s = stream();
    Product logits{};
    for (int l = 0; l < (int)L.size(); l++) {
      Layer& y = L[l];
      const int M = ndir * 4 * y.no;
      const NarrowPlan np = forward_plan(l, save);
      if (save) y.forward_begins(l == 0 && holds.frames == Holds::ROWS);   // (without save the record stays as predict_begins left it)
      if (np.fwd == NF_FUSED) { forward_fused(np, save); return; }   // (a net of one layer: the launch is the whole forward half)
      const ProductPlan pp = product_plan(product_shape(l, PP_FWD, np));   // (the layer below has run: what it left is a fact)
      const bool x_from_hbf = pp.wx.kernel == PK_B16KK && !pp.x_copy;
      logits = pp.logits;   // (the top layer's plan names the softmax layer's product)
      // the lock-step recurrence of a wide layer as planned + what follows it (bf16 source rows for the weight gradient); false: the
      // plan was the kernel with the input projection folded in (lstm_wide.h:lstm_xcd_fwd_bf16_fx) and it did not run
      auto run_wide = [&](const WidePlan& plan, const LstmWideArgs& w) {
        timing.begin("lstm_fwd", s);
        const WideRan ran = launch_lstm_wide(plan, w, coop_sync, step_graphs, s);
        timing.end(s);
        if (ran == WideRan::Nothing) return false;
        y.recurrence_left(ran == WideRan::Persistent && bf16_rec, w.skip_h, w.skip_s, w.Hbf != nullptr, w.Sbf != nullptr);   // (the per-step kernels store everything)
        if (y.cur.sbf) {   // the non-recurrent columns of the bf16 source rows (the recurrence stored the h columns)
          // x columns that fill whole tiles of the weight-gradient GEMM are not copied: the GEMM reads them from Hbf itself (ProductPlan::a2_rows)
          if (pp.a2_rows) {
            if (y.sbf_one_key != (long long)N) {
              CLSTM_LAUNCH(k_source_one_bf16, dim3(nblocks((size_t)N)), dim3(256), 0, s, y.Sbf.p, (size_t)N, y.ni + y.no, w.sbf_ld, ndir, w.sbf_dir);
              y.sbf_one_key = (long long)N;
            }
          } else {
            y.sbf_one_key = -1;
            CLSTM_LAUNCH(k_source_x_bf16, dim3(nblocks((size_t)N * ((y.ni >> 3) + 1))), dim3(256), 0, s, y.Sbf.p, x_from_hbf ? nullptr : layer_input(l),
                         x_from_hbf ? L[l - 1].Hbf.p : nullptr, x_from_hbf ? y.ni : layer_input_ld(l), (size_t)N, y.ni, y.ni + y.no, w.sbf_ld, ndir, w.sbf_dir);
          }
        }
        return true;
      };
      // bf16 mode, wide layer: no hoisted product at all when the persistent recurrence can take the input projection with it (wide_plan's
      // gate, asked where ProductPlan::fx_mode says its operands exist).  Experiment option fuse_wx: 0 never, 1 (default) layers of up to 128
      // inputs, 2 every eligible layer.  Measured at configs[4]
      // (profiles/r04_xcd_phase_cycles_fused_wx.txt): there is no idle shadow to hide the x-part in -- a step's "group wait" is
      // one L2 round trip of the poll, not waiting for late tiles -- so the fused work lands on the chain: +400 cycles per step
      // for 64 inputs (67 us per pass against the 121 us of product + bf16 copy it replaces: kept), +2,950 for 1024 inputs
      // (490 us against 321: not kept).
      bool fx_done = false;
      if (pp.fx_mode) {
        const WidePlan plan = wide_plan(wide_shape(y, true, pp, true));
        if (plan.fx_ngx) {   // asked for: the bf16 input frames are made before the rest of the gate is looked at (as ever; the hoisted product makes them again)
          const unsigned short* xb = l > 0 ? L[l - 1].Hbf.p : nullptr;
          if (l == 0) {
            xbf.reserve((size_t)N * y.ni + 64);
            CLSTM_LAUNCH(k_to_bf16, dim3(nblocks((size_t)N * y.ni)), dim3(256), 0, s, layer_input(0), xbf.p, (size_t)N * y.ni);
            xb = xbf.p;
          }
          LstmWideArgs w = wide_args(y, true, pp);
          w.Xb = xb; w.x_ld = y.ni; w.x_ni = y.ni; w.Wxb = y.WtbT.p; w.bias = y.bias;
          fx_done = plan.kernel == WK_XCD_FWD_BF16_FX && run_wide(plan, w);
        }
      }
      if (fx_done) { if (!y.cur.sbf) ensure_source_x(l); continue; }
      if (pp.needs & PN_H_BELOW) ensure_h_f32(l - 1);   // the products below read the f32 outputs of the layer underneath
      if (np.fwd == NF_MFMA) {
        // chip-filling minibatch of a narrow layer: the input product is part of the batched recurrence (lstm_mfma.h) -- no
        // hoisted W_x GEMM, no pre-activation array; the [1 | x] columns of the source rows are still the weight gradient's
        // (so not built without save, not even for the 128-cell layer whose training form runs then -- it has no no-save
        //  instantiation, reserve_batch kept its arrays: the kernel reads the frames themselves)
        if (save) ensure_source_x(l);
        timing.begin("lstm_fwd", s);
        launch_mfma(y, s, np.saves);
        count_moves(np.moves);
        if (save) y.recurrence_left(false, false, false, false, false);
        timing.end(s);
        continue;
      }
      if (!save) REQUIRE(y.G.p && y.G.cap >= (size_t)N * M, "internal: predict geometry without a pre-activation array");
      timing.begin("gemm_gates_x", s);
      const int ldx = layer_input_ld(l);
      const StoreBias gates{y.G.p, M, y.bias};
      count_moves(pp.moves);
      switch (pp.wx.kernel) {
        case PK_B16KK: {   // both operands k-contiguous bf16 arrays, to LDS as they are: the layer below's outputs, or a copy of the input frames
          if (pp.x_copy) {
            xbf.reserve((size_t)N * y.ni + 64);
            CLSTM_LAUNCH(k_to_bf16, dim3(nblocks((size_t)N * y.ni)), dim3(256), 0, s, layer_input(0), xbf.p, (size_t)N * y.ni);
          }
          gemm_b16kk(s, GemmOperand16{pp.x_copy ? xbf.p : L[l - 1].Hbf.p, y.ni, (long long)N * y.ni}, GemmOperand16{y.WtbT.p, y.ni, (long long)M * y.ni}, gates,
                     (int)N, M, y.ni, pp.wx.tile, pp.stag);
          break;
        }
        case PK_BF16:
          gemm_bf16<GEMM_KC, GEMM_MC>(s, gemm_kc(layer_input(l), ldx, N, layer_input_slack(l)), gemm_mc(y.Wt, M, y.ni, y.wt_slack), gates, (int)N, M, y.ni, pp.wx.tile);
          break;
        default: gemm_f32<GEMM_KC, GEMM_MC>(s, gemm_kc(layer_input(l), ldx, N), gemm_mc(y.Wt, M, y.ni, 0), gates, (int)N, M, y.ni);
      }
      timing.end(s);
      check_launch();
      // the [1 | x] columns of the f32 source rows: written now -- unless this is an upper layer whose weight-gradient
      // product will read the bf16 rows instead (decided after the recurrence below; ensure_source_x() then builds them
      // only if something still asks for them: a fallback path or the state API)
      if (save && (l == 0 || !y.wide)) ensure_source_x(l);   // (the register-resident recurrence of narrow layers reads whole source rows)
      if (y.wide) run_wide(wide_plan(wide_shape(y, true, pp)), wide_args(y, true, pp));
      else {
        LstmSeqArgs a = seq_args(y, true, save);
#ifdef CLSTM_LSTM_PROF
        if (save) { lstm_prof.reserve(128); a.prof = lstm_prof.p; }
#endif
        timing.begin("lstm_fwd", s);
        launch_lstm(true, y.nk4, y.pd.ku, a, bs, y.nthreads, s, save);
        count_moves(np.moves);
        if (save) y.recurrence_left(false, false, false, false, false);
        timing.end(s);
      }
      if (save && !y.cur.sbf) ensure_source_x(l);
    }
    forward_softmax(logits);
  }
  // the softmax layer behind the top recurrence (every family but the fused launch, whose consumer items are that layer)
  void forward_softmax(const Product& logits) {
    hipStream_t s = stream();
    const int nc = desc.nclasses;
    const float* W1 = v + sm_off;
    // the top layer's output rows are [1 | h]: they ARE the softmax layer's source rows
    if (logits.kernel == PK_SOFTMAX_FUSED) {   // logits, limexp and normalisation in one kernel (softmax_fused.h)
      timing.begin("gemm_softmax", s);
      softmax_fwd(s, gemm_kc(L.back().hrow(), L.back().ldh, N), W1, (long long)nc * (1 + sm_ni), Z.p, (int)N, nc, sm_ni, fwd_nanflag(), step_no() + 1);
      timing.end(s);
      check_launch();
    } else {
      timing.begin("gemm_softmax", s);
      if (logits.kernel == PK_X3_BIG)   // bf16 modes: f32-grade bf16 x 3 on 128 x 128 tiles
        gemm_x3_big<GEMM_KC, GEMM_MC>(s, gemm_kc(L.back().hrow(), L.back().ldh, N, 32), gemm_mc(W1 + nc, nc, sm_ni, 0),
                                      StoreBias{Z.p, nc, W1}, (int)N, nc, sm_ni);
      else
      gemm_f32<GEMM_KC, GEMM_MC>(s, gemm_kc(L.back().hrow(), L.back().ldh, N), gemm_mc(W1 + nc, nc, sm_ni, 0),
                                 StoreBias{Z.p, nc, W1}, (int)N, nc, sm_ni);
      timing.end(s);
      check_launch();
      timing.begin("softmax_norm", s);
      CLSTM_LAUNCH(k_softmax_norm, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, Z.p, nc, (size_t)N, fwd_nanflag(), step_no() + 1);
      timing.end(s);
      check_launch();
    }
  }

  // ---- recognition: the forward pass of a minibatch nobody will run backward on (clstm_net_predict) ----
  // forward_pass without save: the family of every layer is chosen by its forward plan, the one rule forward() and
  // reserve_batch ask too (fused launch / batched MFMA / per line, strict and forced options included), and runs in its no-save
  // form: identical arithmetic, so identical outputs.  The training NaN flag is not passed (what clstm_net_set_training(net, 0)
  // does, without changing that setting), nbackward and the training state are untouched.
  // Wide layers and the bf16 modes have no no-save kernels: today's forward pass, without the NaN flag.
  // clstm_debug_path_count: 22 per-line no-save recurrences, 23 fused no-save launches, 15 batched-MFMA no-save launches.
  // The batched recurrence of a 128-cell layer has no no-save instantiation (lstm_mfma.h): its training form runs (counter 16).
  void predict() {
    RoctxRange range_("clstm:predict");
    struct Guard { bool& f; Guard(bool& x) : f(x) { f = true; } ~Guard() { f = false; } } guard_(in_predict);
    if (holds.training_buffers) { forward(); return; }   // (no no-save kernels for this net: see reserve_batch)
    for (auto& y : L) y.predict_begins();
    forward_pass(false);
    forward_ran(false);
  }

  // ---- the forward half as one launch: W_x GEMM producers + recurrence + softmax consumers (lstm_fwd_fused.h; the rule: narrow_plan) ----
  void build_fwd_items() {
    if (fw_key == line_off_h && fw_ncitems > 0) return;
    fw_chunks = (tmax + 15) / 16;
    std::vector<int> items;
    // producers: time order from chunk 1 on (chunk 0 is the recurrence workgroup's own), the longest lines of a chunk
    // first; records of 4 ints: code, the line's first frame, its length, 0
    for (int c = 1; c < fw_chunks; c += FWD_FT)
      for (int i = 0; i < bs; i++) {
        const int b = order_h[i], T = line_off_h[b + 1] - line_off_h[b];
        if (T > 16 * c)
          for (int dir = 0; dir < ndir; dir++) { items.push_back(b << 13 | dir << 12 | c); items.push_back(line_off_h[b]); items.push_back(T); items.push_back(0); }
      }
    fw_npitems = (int)items.size() / 4;
    std::vector<std::pair<int, int>> cons;                    // (iteration at which the block is complete, code)
    for (int b = 0; b < bs; b++) {
      const int T = line_off_h[b + 1] - line_off_h[b];
      for (int blk = 0; 16 * blk < T; blk++)
        cons.push_back({std::max(std::min(16 * blk + 16, T), ndir > 1 ? T - 16 * blk : 0), b << 12 | blk});
    }
    std::stable_sort(cons.begin(), cons.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first < y.first; });
    fw_ncitems = (int)cons.size();
    for (auto& c : cons) items.push_back(c.second);
    fw_items.reserve(items.size() + 8);
    fw_flags.reserve((size_t)ndir * bs * fw_chunks + 8);      // (zero-filled when it grows; flags carry the launch epoch)
    hipStream_t s = stream();
    int* stage = (int*)ring.acquire(items.size() * sizeof(int));
    memcpy(stage, items.data(), items.size() * sizeof(int));
    HIPCHECK(hipMemcpyAsync(fw_items.p, stage, items.size() * sizeof(int), hipMemcpyHostToDevice, s));
    ring.commit(s);
    fw_key = line_off_h;
  }
  void forward_fused(const NarrowPlan& np, bool save) {   // save = false: the recurrence role in its no-save form (predict)
    hipStream_t s = stream();
    Layer& y = L[0];
    build_fwd_items();
    if (++fw_epoch > (1 << 30)) fw_epoch = 1;
    fw_prog_base += tmax + 64;
    if (fw_prog_base > (1 << 30)) fw_prog_base = 1024;
    fw_launches++;
    count_moves(np.moves);
    FwdFusedKernelArgs k{};
    LstmSeqArgs& a = k.a;
    a = seq_args(y, true, save);
    a.prog_off = (long long)y.H.cap - 64 - PROG_WORDS;
    REQUIRE(a.prog_off >= (long long)N * y.ldh + 16, "internal: progress words overlap the output rows");
    a.prog_base = fw_prog_base;
    a.gflag = fw_flags.p; a.gchunks = fw_chunks; a.gepoch = fw_epoch; a.timeouts = dev_err_words() + 2;   // (the forward launch's own error word)
    FwdFusedArgs& h = k.h;
    h.X = layer_input(0); h.ldx = layer_input_ld(0); h.x_elems = (long long)N * h.ldx + 32;
    h.Wk = y.Wk; h.kp = y.wk_kp; h.njp = y.wk_njp; h.bias = y.bias;
    h.pitems = fw_items.p; h.npitems = fw_npitems; h.gflag = fw_flags.p;
    h.W1k = W1k; h.kps = w1k_kps; h.sm_k = sm_ni; h.b1 = v + sm_off; h.Z = Z.p; h.nc = desc.nclasses;
    h.citems = fw_items.p + 4 * fw_npitems; h.ncitems = fw_ncitems;
    h.nanflag = fwd_nanflag(); h.step_no = step_no() + 1;
    h.prog = (const int*)(y.H.p + a.prog_off);
    h.nrec = bs * ndir; h.npb = fw_npitems;
    const unsigned nblk = (unsigned)(h.nrec + h.npb + fw_ncitems);   // one item per helper workgroup
    if (save) ensure_source_x(0);
    static const char* trace_path = getenv("CLSTM_FW_TRACE");   // diagnostics: wall-clock stamps of every workgroup / item of the launch
    const size_t trace_rows = (size_t)h.nrec + fw_npitems + fw_ncitems;
    if (trace_path) { dw_trace.reserve(trace_rows * 4); HIPCHECK(hipMemsetAsync(dw_trace.p, 0, trace_rows * 4 * sizeof(long long), s)); h.trace = dw_trace.p; }
    timing.begin("lstm_fwd", s);
    launch_lstm_fwd_fused(y.nk4, y.pd.ku, k, nblk, y.nthreads, s, save);
    timing.end(s);
    if (save) y.recurrence_left(false, false, false, false, false);
    if (trace_path)
      dump_trace(trace_path, dw_trace.p, trace_rows, s,
                 "# %d recurrence rows (start - end -), %d producer items (start - done chunk), %d consumer items (start ready done ready_iteration); 100 MHz ticks\n",
                 h.nrec, fw_npitems, fw_ncitems);
  }

  // overlapped weight-gradient GEMM: true = bf16 MFMA on f32 operands split into bf16 terms (gemm_dw.h), false = f32 MFMA
  // (experiment option dw_x3=0)
  bool dw_x3 = dbg_opt("dw_x3") != 0;
  // terms per operand of those split products and of the softmax layer's (gemm_x3): 3 = operand-exact (x1 + x2 + x3 is the f32
  // itself, six products), 2 = hi + lo, three products (< 2^-16 per product; rounds 3-5)
  int split_terms = dbg_opt("split_terms");
  // the softmax layer's backward products W.d / x.d the same way (gemm_x3, gemm_bf16.h); experiment option gemm_x3=0 (CLSTM_DEBUG): f32 MFMA.
  // NOT the forward product W_x.x: its ~2^-17 relative error per product shows up in gate pre-activations that cancel to
  // ~0 (a tanh gate at -0.0021 came out 5.6e-6 off where the parity bar allows 2.2e-6), and with K = 49 the split costs
  // more staging than it saves MFMA time (28.5 vs 20.9 us).
  bool gemm_x3_on = dbg_opt("gemm_x3") != 0;
  bool strict_f32 = false;   // clstm_net_set_strict_f32: no split-product recurrences by the library's own rule either (narrow_plan)
  // exact-f32 mode, wide layers: the persistent BACKWARD recurrence as an f32-grade x3 product on the bf16 MFMA (lstm_wide.h:
  // lstm_xcd_bwd_x3) like the backward GEMMs of this mode; off with them (gemm_x3=0 / strict f32) or alone (rec_x3=0, CLSTM_DEBUG options;
  // read per pass: tests compare both kernels in one process)
  bool rec_x3() const {
    if (bf16_gemm || bf16_rec || !gemm_x3_on) return false;
    return dbg_opt("rec_x3") != 0;
  }
  // ---- overlap machinery ---------------------------------------------------------------------------------------
  // the operands of the softmax layer's x.d for the top layer's backward launch (NarrowPlan::xd: the prologue forms of lstm_xd_prologue.h)
  XdArgs xd_args() const {
    const Layer& top = L.back();
    const int nc = desc.nclasses;
    return XdArgs{gemm_kc(Dz.p, nc, N), gemm_kc(v + sm_off + nc, nc, sm_ni, 0), top.dH.p, sm_ni, nc, nullptr, 0};
  }
  // Slab geometry of the chunked weight-gradient GEMM (measured at the bench shape unless said otherwise):
  // - chunks of DW_CHUNK iterations (8: 0.407 ms per step, 16: 0.356, 32: 0.359, 48: 0.360, a decreasing plan 64..16: 0.3615);
  // - ~16 slabs per direction, at most DW_STAB_MAX k-tiles (of 16 frames) each: a slab's table must fit the items' LDS copy.  At
  //   1024 / 2048 lines 256 instead of 800 / 1024 tiles: 1,092 long items on 512 workgroup slots became 3,000+ shorter ones --
  //   weight-gradient launch 0.613 -> 0.559 / 1.259 -> 1.119 ms;
  // - the last DW_TAIL_CHUNKS chunks (those whose items still run when the recurrence ends) in at least DW_TAIL_PARTS slabs: parts
  //   1: 118 us, 4: 112, 8: 115 -- more items than free CUs at the end; with the six-product items 2 chunks instead of 3: -1 us.
  static constexpr int DW_CHUNK = 16, DW_TAIL_PARTS = 4, DW_TAIL_CHUNKS = 2;
  // k-tile tables and slabs of the chunked weight-gradient GEMM for the current batch geometry (rebuilt only when the
  // line lengths change).  Chunks are ranges of recurrence iterations, longest first: the work left when the
  // recurrence ends is what the last (short) chunk holds.
  void build_dw_tables() {
    if (dw_key == line_off_h && dw_nslabs > 0) return;
    std::vector<int> cb;   // chunk ends (iterations), multiples of DW_CHUNK except the last
    for (int done = DW_CHUNK; done < tmax; done += DW_CHUNK) cb.push_back(done);
    cb.push_back(tmax);
    const int tiles_per_slab = std::min(DW_STAB_MAX, std::max(8, (int)((N / 16 + 15) / 16)));
    std::vector<std::vector<int>> tab(ndir);                            // (first frame, count) pairs
    struct Sl { int tb, nt, need, dir, chunk, part; };
    std::vector<std::vector<Sl>> sl(ndir);
    for (int dir = 0; dir < ndir; dir++) {
      int cs = 0;
      for (size_t c = 0; c < cb.size(); c++) {
        const int ce = cb[c];
        const int t0 = (int)tab[dir].size() / 2;
        for (int b = 0; b < bs; b++) {
          const int off = line_off_h[b], T = line_off_h[b + 1] - off;
          if (T <= cs) continue;
          const int e = std::min(ce, T);
          // iterations [cs, e): dir 0 of the backward pass visits frame T-1-it, dir 1 frame it
          const int f_lo = dir == 0 ? T - e : cs, f_hi = dir == 0 ? T - cs : e;
          for (int f = f_lo; f < f_hi; f += 16) { tab[dir].push_back(off + f); tab[dir].push_back(std::min(16, f_hi - f)); }
        }
        const int nt = (int)tab[dir].size() / 2 - t0;
        int parts = std::max(1, (nt + tiles_per_slab - 1) / tiles_per_slab);
        // The items of the LAST chunks cannot start before the recurrence ends, so their latency -- a serial walk over a
        // slab's frames, ~1 us per 32 -- is the launch's tail (profiles/r02_dw_timeline.txt): cut those chunks into
        // more, shorter slabs (>= 2 table entries each).
        if (c + DW_TAIL_CHUNKS >= cb.size()) parts = std::max(parts, std::min(DW_TAIL_PARTS, std::max(1, nt / 2)));
        for (int p = 0; p < parts; p++) {
          const int a0 = t0 + (int)((long long)nt * p / parts), a1 = t0 + (int)((long long)nt * (p + 1) / parts);
          REQUIRE(a1 - a0 <= DW_STAB_MAX, "internal: weight-gradient slab longer than its LDS table");
          sl[dir].push_back(Sl{a0, a1 - a0, ce, dir, (int)c, p});
        }
        cs = ce;
      }
    }
    dw_slabs_per_dir = (int)sl[0].size();
    for (int dir = 1; dir < ndir; dir++) REQUIRE((int)sl[dir].size() == dw_slabs_per_dir, "internal: asymmetric slab lists");
    dw_ntiles_max = 0;
    for (int dir = 0; dir < ndir; dir++) dw_ntiles_max = std::max(dw_ntiles_max, (int)tab[dir].size() / 2);
    // readiness order: chunk, then part, then direction
    std::vector<DwSlab> slabs;
    for (int i = 0; i < dw_slabs_per_dir; i++)
      for (int dir = 0; dir < ndir; dir++) {
        const Sl& x = sl[dir][i];
        slabs.push_back(DwSlab{x.tb, x.nt, x.need, dir, dir * dw_slabs_per_dir + i, {0, 0, 0}});
      }
    dw_nslabs = (int)slabs.size();
    const size_t nk = (size_t)ndir * dw_ntiles_max * 2, nsw = slabs.size() * sizeof(DwSlab) / sizeof(int);
    dw_ktab.reserve(nk + 8);
    dw_slabs.reserve(nsw + 8);
    hipStream_t s = stream();
    int* stage = (int*)ring.acquire((nk + nsw) * sizeof(int));
    for (int dir = 0; dir < ndir; dir++) {
      std::fill(stage + (size_t)dir * dw_ntiles_max * 2, stage + (size_t)(dir + 1) * dw_ntiles_max * 2, 0);
      std::copy(tab[dir].begin(), tab[dir].end(), stage + (size_t)dir * dw_ntiles_max * 2);
    }
    memcpy(stage + nk, slabs.data(), nsw * sizeof(int));
    HIPCHECK(hipMemcpyAsync(dw_ktab.p, stage, nk * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(dw_slabs.p, stage + nk, nsw * sizeof(int), hipMemcpyHostToDevice, s));
    ring.commit(s);
    dw_key = line_off_h;
  }
  // backward recurrence + the chunked weight-gradient GEMM, as one launch or as two: the launch form the layer's plan names (NarrowPlan::bwd)
  void backward_layer_overlapped(Layer& y, const NarrowPlan& np, LstmSeqArgs a, int R, int Cn) {
    hipStream_t s = stream();
    build_dw_tables();
    const int M = ndir * 4 * y.no;
    const long long prog_off = (long long)y.D.cap - 64 - PROG_WORDS;
    REQUIRE(prog_off >= (long long)N * M, "internal: progress words overlap the deltas");
    prog_base += tmax + 64;
    dw_launches++;
    const bool prog_base_wrapped = prog_base > (1 << 30);
    if (prog_base_wrapped) prog_base = 1024;   // (words left from ~5 million launches ago could look complete: harmless in practice, D is rewritten)
    a.prog_off = prog_off;
    a.prog_base = prog_base;
    DevBuf<float>& partial = layer_partial(y);
    partial.reserve((size_t)ndir * dw_slabs_per_dir * R * Cn);
    GemmDwArgs g{};
    g.S = y.S.p; g.sdir = (long long)N * y.lds; g.lds = y.lds; g.s_elems = (long long)N * ndir * y.lds + 3;
    g.D = y.D.p; g.M = M; g.no4 = 4 * y.no; g.d_elems = (long long)N * M + 3;
    g.ktab = dw_ktab.p; g.ntiles_max = dw_ntiles_max; g.slabs = (const DwSlab*)dw_slabs.p; g.nslabs = dw_nslabs;
    g.prog = (const int*)(y.D.p + prog_off); g.line_off = line_off.p; g.bs = bs; g.prog_base = prog_base;
    g.partial = partial.p; g.R = R; g.Cn = Cn;
    g.gx = (unsigned)((Cn + GEMM_BT - 1) / GEMM_BT); g.gy = (unsigned)((R + GEMM_BT - 1) / GEMM_BT);
    g.timeouts = dev_err_words() + 1;
    if (!dw_queue.p) dw_queue.reserve(5 * PROG_STRIDE);
    g.ndir = ndir;
    g.minprog = dw_queue.p + PROG_STRIDE;   // own 128-byte lines
    g.tcap = tmax + 32;
    g.done = nullptr; g.done_target = 0;
    g.x3 = dw_x3;
    g.terms = split_terms;
    unsigned nextra = 0;
    if (np.xd) g.xd = xd_args();   // (only the top layer's plan has it: only its dH comes from the softmax layer)
    if (np.xd == 2) {   // the items' rounds-complete words: [ndir][bs], one per 128 bytes; zero is below every prog_base
      const size_t nw = (size_t)ndir * bs * PROG_STRIDE;
      if (nw > xd_ready.cap || prog_base_wrapped) {
        xd_ready.reserve(nw);
        HIPCHECK(hipMemsetAsync(xd_ready.p, 0, xd_ready.cap * sizeof(int), s));
      }
      g.xd.ready = xd_ready.p; g.xd.ready0 = prog_base;
      a.timeouts = g.timeouts;   // (the recurrence role's bounded wait for a round)
    }
    if (np.dwx) {
      const int xR = 1 + sm_ni, xCn = desc.nclasses;
      g.xS = y.srow(); g.xlds = y.ldh; g.xs_elems = (long long)N * y.ldh + 3;
      g.xD = Dz.p; g.xM = xCn; g.xd_elems = (long long)N * xCn + 3;
      g.xtab = dwx_tab.p; g.xslabs = (const DwSlab*)(dwx_tab.p + 2 * dwx_entries); g.xnslabs = dwx_nslabs;
      g.xpartial = partial_sm.p; g.xR = xR; g.xCn = xCn;
      g.xgx = (unsigned)((xCn + GEMM_BT - 1) / GEMM_BT); g.xgy = (unsigned)((xR + GEMM_BT - 1) / GEMM_BT);
      nextra = (unsigned)dwx_nslabs * g.xgx * g.xgy;
    }
    static const char* trace_path = getenv("CLSTM_DW_TRACE");   // diagnostics: wall-clock stamps of every workgroup of the fused launch
    const size_t trace_rows = (size_t)bs * ndir + (size_t)((dw_nslabs + 7) / 8) * 8 * g.gx * g.gy + 8;
    if (trace_path) { dw_trace.reserve(trace_rows * 4); g.trace = dw_trace.p; g.trace_base = bs * ndir; }
    // the monitor + (producer form) one dH item per recurrence workgroup + the independent items + one per item
    const unsigned nblk = 1u + (np.xd == 2 ? (unsigned)(bs * ndir) : 0u) + nextra + (unsigned)((dw_nslabs + 7) / 8) * 8u * g.gx * g.gy;
    timing.begin("lstm_bwd", s);
    if (np.bwd == NB_MFMA_DW) launch_mfma_bwd(y, a, s, &g, nblk);   // chip-filling minibatch: the batched-MFMA recurrence and the items as one launch (every chunk through the monitor)
    else if (np.bwd == NB_BWD_DW) {   // ONE launch: the recurrence's workgroups first, the GEMM's (one (slab, tile) item each) behind them
      g.done = g.minprog + 2 * PROG_STRIDE;   // own 128-byte line behind the monitor's words; zero-filled once, then only added to
      dw_done_total += (unsigned)(bs * ndir);
      g.done_target = (int)dw_done_total;
      launch_lstm_bwd_dw(y.nk4, y.pd.ku, a, g, np.terms, bs * ndir, nblk, y.nthreads, s);
    } else launch_bwd_narrow(y, np, a, s, &g.xd);   // two launches one after the other: the items find every progress word complete
    timing.end(s);
    if (np.bwd == NB_BWD_DW && trace_path)
      dump_trace(trace_path, dw_trace.p, trace_rows, s,
                 "# rows 0..%d: recurrence workgroups (start, x.d prologue returned, end); then one row per (slab, tile) item: start ready done need_it; 100 MHz ticks\n", bs * ndir - 1);
    if (np.bwd == NB_MFMA_DW || np.bwd == NB_BWD_DW) return;
    timing.begin("gemm_gates_dw", s);
    launch_gemm_dw(g, np.terms, nblk, s);
    timing.end(s);
  }

  // ... and of the softmax layer's W.d items in the top layer's launch (NarrowPlan::dwx): contiguous frames, entries of 16, slabs of
  // 32 entries (512 frames: one short item each)
  void build_dwx_table() {
    if (dwx_N == N) return;
    hipStream_t s = stream();
    dwx_entries = (int)((N + 15) / 16);
    const int eps = std::min(DW_STAB_MAX, std::max(32, (dwx_entries + 63) / 64));   // entries per slab: at most ~64 slabs to reduce
    dwx_nslabs = (dwx_entries + eps - 1) / eps;
    const size_t nsw = (size_t)dwx_nslabs * sizeof(DwSlab) / sizeof(int);
    dwx_tab.reserve((size_t)2 * dwx_entries + nsw + 8);
    int* stage = (int*)ring.acquire(((size_t)2 * dwx_entries + nsw) * sizeof(int));
    for (int e = 0; e < dwx_entries; e++) { stage[2 * e] = 16 * e; stage[2 * e + 1] = (int)std::min<long long>(16, N - 16LL * e); }
    DwSlab* sl = (DwSlab*)(stage + 2 * dwx_entries);
    for (int i = 0; i < dwx_nslabs; i++) sl[i] = DwSlab{eps * i, std::min(eps, dwx_entries - eps * i), 0, 0, i, {0, 0, 0}};
    for (int i = 0; i < dwx_nslabs; i++) REQUIRE(sl[i].ntiles <= DW_STAB_MAX, "internal: weight-gradient slab longer than its LDS table");
    HIPCHECK(hipMemcpyAsync(dwx_tab.p, stage, ((size_t)2 * dwx_entries + nsw) * sizeof(int), hipMemcpyHostToDevice, s));
    ring.commit(s);
    dwx_N = N;
  }
  // of a pass's reductions: the step's plan (the update rides them / they leave the gradient in the peer exchange's slot), where
  // the gradient goes, and what they leave for update()
  struct ReduceTarget { const StepPlan& plan; float* gdst; PassLeft& left; };
  PassLeft backward(const StepPlan& plan = StepPlan{}) {
    PassLeft left;
    left.ticket = plan.ticket;
    const ReduceTarget rt{plan, plan.peer ? comm->peer.slot_ptr(comm->peer.seq + 1) : g, left};
    nbackward++;
    RoctxRange range_("clstm:backward");
    pending_red.clear();   // (entries a throwing pass left behind must not be reduced -- or, with the update fused in, APPLIED -- by this one)
    flush_line_off();
    repack();
    hipStream_t s = stream();
    // every layer's backward plan, asked for ONCE, in front of backward_softmax (which reads the top layer's)
    // ... and every layer's product plan (the slab tables of the Overlapped items first: the plans name their slab counts)
    NarrowPlan np[CLSTM_MAX_LAYERS];
    ProductShape ps[CLSTM_MAX_LAYERS];
    ProductPlan pp[CLSTM_MAX_LAYERS];
    const int top = (int)L.size() - 1;
    for (int l = 0; l <= top; l++) {
      np[l] = backward_plan_narrow(l);
      if (np[l].overlapped) build_dw_tables();
      if (np[l].dwx) build_dwx_table();
      ps[l] = product_shape(l, PP_BWD, np[l]);
      pp[l] = product_plan(ps[l]);
    }
    // every entry of g is assigned by exactly one reduce below: no clearing pass
    backward_softmax(np[top], pp[top]);
    for (int l = top; l >= 0; l--) {
      const BwdFamily fam = L[l].wide ? BwdFamily::Wide : np[l].overlapped ? BwdFamily::Overlapped : BwdFamily::Narrow;
      // the one fact only the launch can tell completes the layer's plan: the recurrence ran as a persistent lock-step kernel
      ps[l].bwd_persistent = backward_recurrence(l, fam, np[l], pp[l]);
      if (ps[l].bwd_persistent) pp[l] = product_plan(ps[l]);
      if (pp[l].needs & PN_SOURCE) ensure_source(l);   // the f32-source products below read S and D
      if (pp[l].needs & PN_DELTA_F32) ensure_delta_f32(l);
      int moves = pp[l].moves;
      if (!backward_weight_gradient(l, fam, pp[l], rt)) {   // (false: an unaligned x.d operand kept the input deltas out of the weight-gradient launch)
        if (pp[l].merged) { moves &= ~(1 << PC_DW_DX_ONE_LAUNCH); pp[l].dx = Product{PK_B16KK, pp[l].dx.tile, pp[l].dx.rows, 1}; }
        backward_input_deltas(l, pp[l]);
      }
      count_moves(moves);
    }
    if (!pending_red.empty()) {
      timing.begin("reduce_scatter", s);
      for (size_t i = 0; i < pending_red.size(); i++) reduce_layer(pending_red[i].gates, pending_red[i].extra, i + 1 == pending_red.size(), rt);
      pending_red.clear();
      timing.end(s);
      check_launch();
    }
    backward_ran();
    return left;
  }
  // SoftmaxLayer::backward (clstm.cc:411-417): x.d = W^T z.d ; W.d += z.d [1;x]^T.  (A side stream for these products was measured
  // on MI355X: no gain -- the recurrence workgroups it would overlap with slow down by as much -- so everything stays on one stream.)
  void backward_softmax(const NarrowPlan& top_plan, const ProductPlan& pp) {
    hipStream_t s = stream();
    Layer& top = L.back();
    const int nc = desc.nclasses, R = 1 + sm_ni, Cn = nc;
    const float* W1 = v + sm_off;
    // W.d depends on nothing the backward recurrence produces: when the top layer's backward runs as the fused launch
    // (lstm_bwd_dw.h) its slabs are items of THAT launch -- they execute on the idle half of the chip during the ~14 us
    // before the recurrence's first chunk is released -- and only x.d stays in front of the recurrence.
    // (NarrowPlan::dwx: the rule; ProductPlan::sm_wd, sm_xd: the kernels and the slab count)
    const int ns = pp.sm_wd.slabs;
    partial_sm.reserve((size_t)ns * R * Cn);
    // W.d (split-K slabs) and x.d in ONE launch: two small independent products, each mostly prologue and
    // epilogue latency on its own (13.9 + 12.4 us back to back)
    const GemmOperand Wk = gemm_kc(W1 + nc, nc, sm_ni, 0);
    const StorePartial wd_store{partial_sm.p, R, Cn};
    const StorePlain xd_store{top.dH.p, sm_ni};
    const bool launches = pp.sm_wd.kernel != PK_NONE || pp.sm_xd.kernel != PK_NONE;   // (else the top layer's backward launch computes both)
    if (launches) timing.begin("gemm_softmax_dw_dx", s);
    if (top_plan.dwx) {
      if (launches) gemm_x3<GEMM_KC, GEMM_KC>(s, gemm_kc(Dz.p, nc, N), Wk, xd_store, (int)N, sm_ni, nc, 1, 1, pp.terms);
    } else if (pp.sm_wd.kernel == PK_X3_BIG) {
      gemm_x3_big<GEMM_MC, GEMM_MC>(s, gemm_mc(top.srow(), top.ldh, N, 32), gemm_mc(Dz.p, nc, N, 32), wd_store, R, Cn, (int)N, ns);
      gemm_x3_big<GEMM_KC, GEMM_KC>(s, gemm_kc(Dz.p, nc, N, 32), Wk, xd_store, (int)N, sm_ni, nc);
    } else {
      const GemmProblem wd = gemm_problem(gemm_mc(top.srow(), top.ldh, N), gemm_mc(Dz.p, nc, N), R, Cn, (int)N, ns);
      const GemmProblem xd = gemm_problem(gemm_kc(Dz.p, nc, N), Wk, (int)N, sm_ni, nc);
      if (pp.sm_wd.kernel == PK_X3_PAIR) gemm_x3_pair<GEMM_MC, GEMM_MC, StorePartial, GEMM_KC, GEMM_KC, StorePlain>(s, wd, wd_store, xd, xd_store, pp.terms);
      else gemm_f32_pair<GEMM_MC, GEMM_MC, StorePartial, GEMM_KC, GEMM_KC, StorePlain>(s, wd, wd_store, xd, xd_store);
    }
    if (launches) timing.end(s);
    // the slabs are reduced together with the top layer's weight-gradient slabs (backward_weight_gradient)
    sm_red = ReduceDesc{partial_sm.p, nullptr, (long long)sm_off, ns, 1, R, Cn, nc};
    check_launch();
  }
  // the backward recurrence of layer l in the family and form its plan named; returns whether it ran as a persistent lock-step kernel
  bool backward_recurrence(int l, BwdFamily fam, const NarrowPlan& np, const ProductPlan& pp) {
    Layer& y = L[l];
    hipStream_t s = stream();
    const LstmSeqArgs a = seq_args(y, false);   // (no progress words: backward_layer_overlapped sets them in its copy)
    if (fam == BwdFamily::Overlapped) {   // the recurrence and the weight-gradient GEMM run side by side (gemm_dw.h)
      backward_layer_overlapped(y, np, a, 1 + y.ni + y.no, 4 * y.no);
      count_moves(np.moves);
      return false;
    }
    timing.begin("lstm_bwd", s);
    WideRan ran = WideRan::Nothing;
    int skipped_d = 0;
    if (fam == BwdFamily::Wide) {
      const LstmWideArgs w = wide_args(y, false, pp);
      ran = launch_lstm_wide(wide_plan(wide_shape(y, false, pp)), w, coop_sync, step_graphs, s);
      skipped_d = w.skip_d;
    } else { launch_bwd_narrow(y, np, a, s); count_moves(np.moves); }
    timing.end(s);
    const bool persistent = ran == WideRan::Persistent;
    y.backward_left(persistent && bf16_rec && skipped_d);   // (launch_lstm_wide moved the plan's path counters)
    return persistent;
  }
  // W.d += delta [1; x_t; h_{t-1}]^T for the four gates of each direction (both directions in one batched launch: half the slabs per
  // direction fill the chip) unless the recurrence launch's items have left the slabs already (Overlapped), and the slab reduction: queued
  // in a stacked net (see reduce_layer), launched here, in this step's bracket, for a single layer.  true: x.d rode the launch (gemm_dw_dx).
  bool backward_weight_gradient(int l, BwdFamily fam, const ProductPlan& pp, const ReduceTarget& rt) {
    Layer& y = L[l];
    hipStream_t s = stream();
    const int M = ndir * 4 * y.no, R = 1 + y.ni + y.no, Cn = 4 * y.no;
    const bool product = fam != BwdFamily::Overlapped, stacked = L.size() > 1;
    const int ns = pp.dw.slabs;
    DevBuf<float>& pbuf = layer_partial(y);
    // the bracket of this step: a product family reports its GEMM -- and, in a single-layer net, the reduction behind it -- as
    // "gemm_gates_dw"; a single overlapped layer reports its reduction as "reduce_scatter"; a stacked overlapped layer launches
    // nothing here (its reduction is queued) and opens none
    const char* const bracket = product ? "gemm_gates_dw" : stacked ? nullptr : "reduce_scatter";
    if (bracket) timing.begin(bracket, s);
    bool dx_done = false;
    if (product) {
      pbuf.reserve((size_t)ndir * ns * R * Cn);
      const GemmOperand src = gemm_batched(gemm_mc(y.S.p, y.lds, N), (long long)N * y.lds, ndir);
      const GemmOperand dlt = gemm_batched(gemm_mc(y.D.p, M, N, 0), 4LL * y.no, 1);
      const StorePartial store{pbuf.p, R, Cn};
      switch (pp.dw.kernel) {
        case PK_B16MC: case PK_DW_DX: dx_done = backward_dw_bf16(l, pp, pbuf.p); break;
        case PK_BF16: gemm_bf16<GEMM_MC, GEMM_MC>(s, src, dlt, store, R, Cn, (int)N, pp.dw.tile, ns, ndir); break;
        case PK_X3_BIG: gemm_x3_big<GEMM_MC, GEMM_MC>(s, src, dlt, store, R, Cn, (int)N, ns, ndir); break;
        default: gemm_f32<GEMM_MC, GEMM_MC, StorePartial, GEMM_BK_DW>(s, src, dlt, store, R, Cn, (int)N, ns, ndir);
      }
    }
    const ReduceDesc gates{pbuf.p, y.moff, 0LL, ns, ndir, R, Cn, y.no};
    const ReduceDesc extra = l == (int)L.size() - 1 ? sm_red : ReduceDesc{};   // the softmax layer's slabs ride the top layer's
    if (stacked) pending_red.push_back(PendingReduce{gates, extra});
    else reduce_layer(gates, extra, true, rt);
    if (bracket) timing.end(s);
    check_launch();
    return dx_done;
  }
  // ... from both operands in bf16 as their producers left them (deltas: the persistent backward recurrence; sources: the forward
  // pass), transposed by the LDS on the way into the MFMA.  true: the layer's input deltas were computed by the same launch.
  bool backward_dw_bf16(int l, const ProductPlan& pp, float* slabs) {
    Layer& y = L[l];
    hipStream_t s = stream();
    const int M = ndir * 4 * y.no, R = 1 + y.ni + y.no, Cn = 4 * y.no, ldsb = y.ni + y.no + 8, ns = pp.dw.slabs;
    const GemmOperand16B src{y.Sbf.p, ldsb, (long long)N * ndir * ldsb, (long long)N * ldsb}, dlt{y.Dbf.p, M, (long long)N * M, 4LL * y.no};
    const GemmOperand16B a2 = pp.a2_rows ? GemmOperand16B{L[l - 1].Hbf.p, y.ni, (long long)N * y.ni, 0} : GemmOperand16B{nullptr, 0, 0, 0};
    if (!pp.bias_out) { gemm_b16mc(s, src, dlt, StorePartialRot{slabs, R, Cn}, R, Cn, (int)N, pp.dw.tile, pp.stag, ns, ndir, a2, pp.a2_rows); return false; }
    // The bias row W.d[:,0] += sum_b y.d (clstm_compute.cc:301) is not a row of this product (product_plan: dw16_rows) -- the persistent backward
    // recurrence sums the deltas of a line while it produces them (LstmWideArgs::dbias) and k_bias_rows lays the sum over lines into row 0 of the
    // first slab.  Where the plan says so, the layer's input deltas ride the launch (gemm_bf16.h:gemm_dw_dx_kernel)
    REQUIRE(y.dbias.p, "internal: bias row left out of the weight-gradient product without the recurrence's per-line sums");
    const StorePartialShift store{slabs, R, Cn};
    const bool dx_done = pp.merged && gemm_dw_dx(s, src, dlt, store, pp.dw.rows, Cn, (int)N, pp.dw.tile, ns, ndir, a2, pp.a2_rows, GemmOperand16{y.Dbf.p, M, (long long)N * M},
                                                 GemmOperand16{y.Wtb.p, M, (long long)y.ni * M}, StorePlain{L[l - 1].dH.p, y.ni}, (int)N, y.ni, M);
    if (!dx_done) gemm_b16mc(s, src, dlt, store, pp.dw.rows, Cn, (int)N, pp.dw.tile, pp.stag, ns, ndir, a2, pp.a2_rows);
    CLSTM_LAUNCH(k_bias_rows, dim3((unsigned)(((size_t)ndir * Cn + 63) / 64)), dim3(64), 0, s, (const float*)y.dbias.p, slabs, bs, ndir, ns, R, Cn);
    return dx_done;
  }
  // input deltas: x.d = sum_dir W_x^T delta (Parallel::backward sums both subs, clstm.cc:538-541)
  void backward_input_deltas(int l, const ProductPlan& pp) {
    Layer& y = L[l];
    hipStream_t s = stream();
    const int M = ndir * 4 * y.no;
    if (l == 0 && want_dx0) dX0.reserve((size_t)N * y.ni);
    float* const dx = l > 0 ? L[l - 1].dH.p : want_dx0 ? dX0.p : nullptr;   // the layer below's output deltas, or what the caller asked for
    if (pp.dx.kernel == PK_NONE) return;
    timing.begin("gemm_gates_dx", s);
    const GemmOperand D = gemm_kc(y.D.p, M, N, 32), W = gemm_kc(y.Wt, M, y.ni, y.wt_slack);
    switch (pp.dx.kernel) {
      case PK_B16KK:   // the persistent recurrence left the deltas as a k-contiguous bf16 array: both operands go to LDS as they are
        gemm_b16kk(s, GemmOperand16{y.Dbf.p, M, (long long)N * M}, GemmOperand16{y.Wtb.p, M, (long long)y.ni * M}, StorePlain{dx, y.ni}, (int)N, y.ni, M, pp.dx.tile, pp.stag);
        break;
      case PK_BF16: gemm_bf16<GEMM_KC, GEMM_KC>(s, D, W, StorePlain{dx, y.ni}, (int)N, y.ni, M, pp.dx.tile); break;
      case PK_X3_BIG: gemm_x3_big<GEMM_KC, GEMM_KC>(s, D, W, StorePlain{dx, y.ni}, (int)N, y.ni, M); break;
      default: gemm_f32<GEMM_KC, GEMM_KC>(s, gemm_kc(y.D.p, M, N), gemm_kc(y.Wt, M, y.ni, 0), StorePlain{dx, y.ni}, (int)N, y.ni, M);
    }
    timing.end(s);
    check_launch();
  }
  // The slab reduction of one layer (+ the softmax layer's, riding the top layer's).  `last`: the last reduction launch of the
  // backward pass.  With the update riding the reductions (fuse: train_step without an exchange), ALL of them must see the final
  // error state of the pass -- a sticky device error raised by a lower layer's recurrence after an upper layer had taken its update
  // would leave half a step applied -- so a stacked net keeps a slab buffer per layer (Layer::partial) and reduces every layer here,
  // behind the LAST recurrence; a single layer is reduced where it always was.  (What a reduction itself can still find is a
  // non-finite gradient ENTRY: skipped entry by entry, ops.h:k_update.)
  struct PendingReduce { ReduceDesc gates, extra; };
  std::vector<PendingReduce> pending_red;
  // ---- the NEXT minibatch's ingest behind this step's last reduction (step.inc: train_step; ops.h: IngestTail) ----
  // StepPlan::defer_last: the last reduction launch of a fused-update step is described in PassLeft::deferred instead of enqueued;
  // the step declares the next minibatch (set_batch + the host half of its alignment: neither touches anything the described
  // launch reads) and enqueues it with the ingest blocks behind its own.
  void launch_deferred_reduce(DeferredReduce& deferred, const IngestTail* tail) {
    if (!deferred.armed) return;
    const int nb = nblocks(deferred.work);
    timing.begin("reduce_scatter", deferred.q);
    if (tail) {
      IngestTail t = *tail;
      t.nb_main = nb;
      const int ntrail = (t.lo_src ? 1 : 0) + (t.aux_src ? (t.aux_n + 255) / 256 : 0);
      CLSTM_LAUNCH(k_reduce_scatter_ingest, dim3(nb + t.nbi + ntrail), dim3(256), 0, deferred.q, deferred.gates, deferred.extra, deferred.gdst, (int*)nullptr, 0, deferred.uf, t);
      g_path_count[PC_INGEST_TAIL]++;
    } else {
      CLSTM_LAUNCH(k_reduce_scatter, dim3(nb), dim3(256), 0, deferred.q, deferred.gates, deferred.extra, deferred.gdst, (int*)nullptr, 0, deferred.uf);
    }
    timing.end(deferred.q);
    check_launch();
    deferred.armed = false;   // only now: a launch that threw leaves it armed, and the caller's plain launch_deferred_reduce(.., nullptr) still enqueues it
  }
  // the minibatch whose front half (batch geometry, alignment metadata, ingest) the last step's tail has already done
  struct NextBatch {   // (its content; WHETHER the net holds it is Holds::batch)
    const float* x = nullptr;
    std::vector<int> T, labels, L;
    static size_t nlabels(const Minibatch& m) {
      size_t nl = 0;
      for (int b = 0; b < m.bs; b++) nl += (size_t)m.L[b];
      return nl;
    }
    bool matches(const Minibatch& m) const {
      if (x != m.x || (int)T.size() != m.bs) return false;
      if (memcmp(T.data(), m.T, (size_t)m.bs * sizeof(int)) || memcmp(L.data(), m.L, (size_t)m.bs * sizeof(int))) return false;
      const size_t nl = nlabels(m);
      return nl == labels.size() && (nl == 0 || !memcmp(labels.data(), m.labels, nl * sizeof(int)));
    }
    void remember(const Minibatch& m) {
      x = m.x; T.assign(m.T, m.T + m.bs); L.assign(m.L, m.L + m.bs);
      labels.assign(m.labels, m.labels + nlabels(m));
    }
  } next;
  DevBuf<float>& layer_partial(Layer& y) { return L.size() > 1 ? y.partial : partial; }
  void reduce_layer(const ReduceDesc& gates, const ReduceDesc& extra, bool last, const ReduceTarget& rt) {
    hipStream_t q = stream();
    const size_t work = (size_t)gates.nbatch * gates.R * gates.Cn + (size_t)extra.R * extra.Cn * extra.nbatch;
    UpdateFuse uf{};
    uf.nanflag = nanflag(); uf.step_no = step_no();
    PassLeft& left = rt.left;
    if (rt.plan.fuse) {   // (train_step without a communicator) this layer's parameters are updated by the reduction itself
      uf = UpdateFuse{v, d, lr, mom, gclip, (const int*)dev_err_words(), last ? left.ticket.word : nullptr, left.ticket.id, nanflag(), step_no(), PackDst{}};
      if (last) { left.ticket.word = nullptr; left.update_applied = true; }
      // a single narrow layer whose packed copies are current: the update keeps them current (ops.h: PackDst) and the next
      // step's ingest launch has nothing to repack
      left.packs_follow_update = false;
      if (L.size() == 1 && !L[0].wide && !packed_dirty && pack_inverse(L[0])) {
        Layer& y = L[0];
        const size_t nr = (size_t)ndir * 4 * 4 * y.nk4 * y.nthreads;
        uf.pk = PackDst{y.pack_inv.p, PACK_KD, y.Wt, y.bias, y.Rf, y.Rb, y.pd, pack_fused_desc(y), (unsigned)((size_t)(1 + y.ni) * ndir * 4 * y.no), (unsigned)nr};
        left.packs_follow_update = true;
        g_path_count[PC_PACKS_FOLLOW_UPDATE]++;
      }
    }
    if (rt.plan.defer_last && last && rt.plan.fuse) {   // enqueued by launch_deferred_reduce, the next minibatch's ingest behind it
      left.deferred = DeferredReduce{true, gates, extra, rt.gdst, uf, work, q};
      return;
    }
    CLSTM_LAUNCH(k_reduce_scatter, dim3(nblocks(work)), dim3(256), 0, q, gates, extra, rt.gdst, (int*)nullptr, 0, uf);
    if (rt.plan.peer && last) left.peer_pending = true;
  }

  long long nbackward = 0;           // backward passes of this net so far = the number of the current training step (from 1)
  int step_no() const { return (int)std::min<long long>(nbackward, 2147483647LL); }
  // The reference asserts on non-finite values in BACKWARD only (clstm.cc:630-649): a forward pass that belongs to no
  // training step (predict, the test-set pass of clstmocrtrain: clstm_net_set_training(net, 0)) must not arm the process-wide
  // word -- one NaN logit in an inference pass would block the updates of every net of the process.
  bool training = true;
  int* fwd_nanflag() const { return training && !in_predict ? nanflag() : nullptr; }
  static int* nanflag() {            // device error word [3], or null when CLSTM_NANCHECK=0
    static const bool on = !(getenv("CLSTM_NANCHECK") && atoi(getenv("CLSTM_NANCHECK")) == 0);
    return on ? dev_err_words() + 3 : nullptr;
  }
  // The update rides the slab reductions (train_step without an exchange).  All or nothing: every reduction of a pass runs behind
  // its last recurrence (reduce_layer) -- in a stacked net the layers' reductions used to sit between the recurrences, top down, and
  // an error word raised by a lower layer found the upper layers' parameters already updated: half a step.
  bool fuse_eligible() const { return !comm || comm->nranks == 1; }
  // the plan of a one-call step: no exchange between backward pass and update -> the update rides the reductions; several ranks that
  // could map each other -> the peer exchange; a next minibatch to ingest behind the last reduction only where that one carries the update
  StepPlan step_plan(bool next_given, const HostTicket* ticket) {
    StepPlan p;
    p.fuse = fuse_eligible();
    p.peer = comm && comm->nranks > 1 && comm->peer_ready((size_t)nparams, stream());
    p.defer_last = next_given && p.fuse;
    if (ticket) p.ticket = *ticket;
    return p;
  }
  // `left`: what the backward pass just enqueued returned.  Of a backward pass and an update made by separate calls nothing has to
  // reach this function: that pass ran the default plan, which leaves a default PassLeft -- the last branch below.
  void update(PassLeft& left) {
    hipStream_t s = stream();
    RoctxRange range_("clstm:update");
    params_epoch++;
    if (left.update_applied) {   // done by the reductions of the backward pass just enqueued
      packed_dirty = !left.packs_follow_update;
      return;
    }
    HostTicket& tk = left.ticket;
    if (left.peer_pending) {   // peer all-reduce fused into the update, one-shot or two-phase (comm.h: peer_use_two_phase; ops.h)
      RoctxRange range2_("clstm:allreduce+update");
      const int sq = ++comm->peer.seq;
      const bool two = peer_use_two_phase((size_t)nparams, comm->nranks);
      timing.begin("allreduce_grads", s);
      peer_exchange_begin(*comm, sq, two, (size_t)nparams, s);   // (the hosts announce the exchange to each other first: Comm::peer_barrier)
      timing.end(s);
      timing.begin("sgd_update", s);
      peer_exchange_finish(*comm, sq, two, v, d, g, (size_t)nparams, lr, mom, gclip, (const int*)dev_err_words(), tk.word, tk.id, nanflag(),
                           step_no(), s);
      tk.word = nullptr;
      timing.end(s);
      check_launch();
      g_path_count[PC_PEER_EXCHANGE]++;
      if (two) g_path_count[PC_PEER_TWO_PHASE]++;
      packed_dirty = true;
      maybe_replica_check(s);
      return;
    }
    if (comm && comm->nranks > 1) {   // sum of the ranks' fresh minibatch gradients, in place, on this stream (share_deltas, clstm.cc:731-744)
      RoctxRange range2_("clstm:allreduce");
      timing.begin("allreduce_grads", s);
      comm->allreduce(g, nparams, s);
      timing.end(s);
    }
    timing.begin("sgd_update", s);
    CLSTM_LAUNCH(k_update, dim3(nblocks(nparams)), dim3(256), 0, s, v, d, (const float*)g, (size_t)nparams, lr, mom, gclip, (const int*)dev_err_words(), tk.word, tk.id,
                 nanflag(), step_no());
    tk.word = nullptr;
    timing.end(s);
    check_launch();
    packed_dirty = true;
    if (comm && comm->nranks > 1) maybe_replica_check(s);
  }
  // Replica consistency (ops.h:k_param_checksum ...): every replica_every-th update of a net whose communicator has several
  // ranks, and on request (clstm_net_replica_check).  Everything stays on the stream; a mismatch lands in device error word [7].
  long long nupdates_dp = 0;
  static int replica_every() {
    static const int n = getenv("CLSTM_REPLICA_CHECK_EVERY") ? atoi(getenv("CLSTM_REPLICA_CHECK_EVERY")) : 256;
    return n;
  }
  void maybe_replica_check(hipStream_t s) {
    nupdates_dp++;
    const int every = replica_every();
    if (every > 0 && nupdates_dp % every == 0) replica_check(s);
  }
  void replica_check(hipStream_t s) {
    if (!comm || comm->nranks < 2) return;
    RoctxRange range_("clstm:replica_check");
    comm->chk.reserve(8);
    comm->chk_acc.reserve(2);
    CLSTM_LAUNCH(k_param_checksum, dim3(std::min<unsigned>(nblocks(nparams), 1024u)), dim3(256), 0, s, (const float*)v, (size_t)nparams, comm->chk_acc.p);
    CLSTM_LAUNCH(k_checksum_pieces, dim3(1), dim3(64), 0, s, comm->chk_acc.p, comm->chk.p);
    comm->allreduce(comm->chk.p + 4, 4, s, true);   // (four floats: one-shot whatever the rule says)
    CLSTM_LAUNCH(k_replica_verify, dim3(1), dim3(64), 0, s, (const float*)comm->chk.p, comm->nranks, dev_err_words() + 7, step_no());
    check_launch();
    g_path_count[PC_REPLICA_CHECK]++;
  }
};

