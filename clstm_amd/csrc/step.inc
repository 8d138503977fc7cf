// step.inc -- part of clstm_hip.hip (namespace clstm): one training step of the fused network, written ONCE -- declare, ingest,
// forward, CTC, backward, tail, update -- for the three step entries of abi.inc (plain, with a declared next minibatch, host-fed),
// and the pieces of it the separate calls share: the ingest launch, the alignment's host half and its launch.  Included once by
// clstm_hip.hip behind ctc_run.inc: a step drives a Net and the CtcWorkspace beside it.  What the net holds changes through Net's named
// transitions only (net.inc: Net::Holds): nothing here assigns a member of that record or commits the net's pinned ring.

// Every refusal a minibatch can earn, made on the host BEFORE anything of a net is touched, by the very functions that make them where a
// minibatch is declared and aligned: the line lengths (batch_frames, as declare_batch), the transcripts (expand_transcripts), the classes
// (check_target_classes, as run_ctc) and the alignment's batch arithmetic (ctc_minibatch_plan, as run_ctc).  Returns the expanded transcripts.
struct Targets { std::vector<int> states, soff; };
static Targets check_minibatch(int nclasses, const Minibatch& m) {
  batch_frames(m.T, m.bs);
  Targets t;
  expand_transcripts(m.labels, m.L, m.bs, t.states, t.soff);
  check_target_classes(nclasses, t.states.data(), t.soff[m.bs]);
  std::vector<int> lo(m.bs + 1, 0);
  for (int b = 0; b < m.bs; b++) lo[b + 1] = lo[b] + m.T[b];
  ctc_minibatch_plan(nclasses, lo.data(), t.soff.data(), m.bs);
  return t;
}

// the frames at x (device) into the net's input block and layer 0's source rows; aux: the CTC metadata copy of a training step rides
// the launch
static void net_ingest(Net& n, CtcWorkspace& ctc, const float* x, const StagedCopy* aux = nullptr) {
  n.ensure_training_buffers();   // (the ingest writes layer 0's source rows)
  RoctxRange range_("clstm:ingest");
  Layer& y = n.L[0];
  bool aux_done = false;
  const bool with_pack = n.packed_dirty && n.L.size() == 1 && !y.wide;   // the training step of a narrow net: ingest + weight repack in one launch
  const int* const lo = n.unsent_offsets();   // (the pinned slot, while the line offsets are not on the device)
  if (with_pack || lo || (aux && aux->nwords > 0)) {
    // (any net: the small host arrays of the step ride the ingest launch -- a separate copy of the CTC metadata cost a
    // configs[4] step ~25 us of DMA set-up in front of its first kernel)
    const int M = n.ndir * 4 * y.no, KQP = 4 * y.nk4;
    const size_t nr = (size_t)n.ndir * 4 * KQP * y.nthreads;
    const int nbi = n.ingest_blocks(x), nbp = with_pack ? nblocks((size_t)(1 + y.ni) * M + 2 * nr) : 0;
    const bool ax = aux && aux->nwords > 0;
    // optional trailing blocks read small host arrays straight from their pinned slots: the line offsets and -- in a
    // training step -- the CTC metadata (no DMA launches, no event records on the stream's critical path)
    CLSTM_LAUNCH(k_ingest_pack, dim3(nbi + nbp + (lo ? 1 : 0) + (ax ? (aux->nwords + 255) / 256 : 0)), dim3(256), 0, g_stream, x, n.X.p, y.S.p, (size_t)n.N, y.ni, y.lds,
                 n.ndir, (long long)n.N * y.lds, nbi, nbp, (const float*)n.v, y.Wt, y.bias, y.Rf, y.Rb, y.pd, n.pack_fused_desc(y),
                 lo, n.line_off.p, 2 * n.bs + 1, ax ? aux->src : nullptr, ax ? aux->dst : nullptr, ax ? aux->nwords : 0,
                 with_pack ? (const int*)n.pack_table(y) : (const int*)nullptr);
    if (lo) n.offsets_sent(g_stream);
    if (ax) { ctc.meta.commit(g_stream); aux_done = true; }
    if (with_pack) n.packed_dirty = false;
  } else {
    CLSTM_LAUNCH(k_ingest, dim3(nblocks((size_t)n.N * (1 + y.ni))), dim3(256), 0, g_stream, x, n.X.p, y.S.p, (size_t)n.N, y.ni,
                 y.lds, n.ndir, (long long)n.N * y.lds);
  }
  check_launch();
  if (aux && aux->nwords > 0 && !aux_done) {   // not the fused launch: a plain asynchronous copy
    HIPCHECK(hipMemcpyAsync(aux->dst, aux->src, (size_t)aux->nwords * sizeof(int), hipMemcpyHostToDevice, g_stream));
    ctc.meta.commit(g_stream);
  }
  n.frames_ingested(true);
}
// the same ingest as trailing workgroups of a step's last reduction (ops.h: IngestTail; Net::launch_deferred_reduce): the declared
// geometry is the NEXT minibatch's
static IngestTail ingest_tail(const Net& n, const float* x, const StagedCopy& meta) {
  const Layer& y = n.L[0];
  IngestTail t{};
  t.x = x; t.X = n.X.p; t.S = y.S.p; t.N = (unsigned long long)n.N; t.ni = y.ni; t.lds = y.lds; t.ndir = n.ndir; t.sdir = (long long)n.N * y.lds;
  t.nbi = n.ingest_blocks(x);
  t.lo_src = n.unsent_offsets(); t.lo_dst = n.line_off.p; t.lo_n = 2 * n.bs + 1;
  t.aux_src = meta.nwords > 0 ? meta.src : nullptr; t.aux_dst = meta.dst; t.aux_n = meta.nwords;
  return t;
}
// CTC alignment of the current minibatch against m's transcripts (m.labels, m.L; one per declared line): the host half, and --
// launch -- the alignment itself.  launch = false (training steps): prepared here, launched behind the forward pass by net_ctc_launch.
// made: the transcripts as check_minibatch has expanded them already.
static void net_ctc(Net& n, CtcWorkspace& ctc, const Minibatch& m, float* aligned_h, StagedCopy* defer = nullptr, bool launch = true,
                    const Targets* made = nullptr) {
  Targets own;
  if (!made) expand_transcripts(m.labels, m.L, n.bs, own.states, own.soff);
  const std::vector<int>&states = made ? made->states : own.states, &soff = made ? made->soff : own.soff;
  float* al = nullptr;
  if (aligned_h) { n.aligned.reserve((size_t)n.N * n.desc.nclasses); al = n.aligned.p; }
  RoctxRange range_(launch ? "clstm:ctc" : "clstm:ctc_prepare");
  if (launch) n.timing.begin("ctc_align", g_stream);
  run_ctc(ctc, n.Z.p, n.Dz.p, al, n.desc.nclasses, n.line_off_h.data(), states.data(), soff.data(), n.bs, g_stream, defer, launch);
  if (launch) n.timing.end(g_stream);
  if (aligned_h && launch) copy_d2h(aligned_h, al, (size_t)n.N * n.desc.nclasses);
}
static void net_ctc_launch(Net& n, CtcWorkspace& ctc) {
  RoctxRange range_("clstm:ctc");
  n.timing.begin("ctc_align", g_stream);
  launch_ctc_align(ctc, g_stream);
  n.timing.end(g_stream);
}

// One training step on `cur`.
// next (given()): the front half of the NEXT step -- batch geometry, the host half of its alignment, the ingest of its frames, the
// copies of its line offsets and CTC metadata -- is done HERE: on the host while this step's launches run, on the device by extra
// workgroups of this step's last launch (the slab reduction + fused update; ops.h: k_reduce_scatter_ingest), whose CUs are mostly
// idle.  The next call finds its minibatch declared (same x pointer, same T / transcripts: compared by content) and starts with the
// forward launch; anything else -- another minibatch, clstm_net_set_batch in between, a communicator of several ranks, a net whose
// update does not keep its packed weights current -- takes the ordinary path.
// ticket (host-fed step, cur.x is the slot Net::HostFeed::stage filled): the step's last kernel publishes the step number, which is
// committed once that kernel is enqueued.
// Exchange between backward pass and update (Net::step_plan): none -- no communicator, or one of a single rank -- and the reductions of
// the backward pass apply the update themselves; a communicator of several ranks: the peer-read all-reduce fused into the update where
// the ranks could map each other, else ncclAllReduce + k_update.
static void train_step(Net& n, CtcWorkspace& ctc, const Minibatch& cur, const Minibatch& next, const HostTicket* ticket) {
  if (!ticket && n.next_is(cur)) {   // (host-fed frames are new with every call)
    n.next_adopted();                      // declared and ingested by the previous call's tail
    g_path_count[PC_INGEST_TAIL_USED]++;
  } else {
    n.set_batch(cur.T, cur.bs);
    StagedCopy meta;
    net_ctc(n, ctc, cur, nullptr, &meta, false);
    net_ingest(n, ctc, cur.x, &meta);
  }
  n.forward();
  net_ctc_launch(n, ctc);
  PassLeft left = n.backward(n.step_plan(next.given(), ticket));
  if (left.deferred.armed) {
    // (a single narrow layer whose update does not keep the packed weights current: its ingest launch also repacks -- not the tail's job)
    bool tail = !(n.L.size() == 1 && !n.L[0].wide && !left.packs_follow_update);
    Targets made;
    if (tail) {
      // the NEXT minibatch at fault (a bad label, a size): nothing of the net has been touched, this step completes with its own minibatch
      // the current one; the next call declares its minibatch itself and reports the error where it belongs.  Everything else propagates.
      try { made = check_minibatch(n.desc.nclasses, next); } catch (const Error&) { tail = false; }
    }
    if (tail) {
      n.set_batch(next.T, next.bs);
      StagedCopy meta;
      net_ctc(n, ctc, next, nullptr, &meta, false, &made);
      const IngestTail t = ingest_tail(n, next.x, meta);
      n.launch_deferred_reduce(left.deferred, &t);
      if (t.lo_src) n.offsets_sent(g_stream);
      if (t.aux_src) ctc.meta.commit(g_stream);
      n.frames_ingested(true);
      n.next_declared(next);
    } else n.launch_deferred_reduce(left.deferred, nullptr);
  }
  n.update(left);
  if (ticket) {
    REQUIRE(left.ticket.word == nullptr, "internal: no kernel of the step took the step word");
    n.hf.commit();
  }
}
