// step.inc -- part of clstm_hip.hip (namespace clstm): one training step of the fused network, written ONCE -- declare, ingest,
// forward, CTC, backward, tail, update -- for the three step entries of abi.inc (plain, with a declared next minibatch, host-fed),
// and the pieces of it the separate calls share: the ingest launch, the alignment's host half and its launch.  Included once by
// clstm_hip.hip behind ctc_run.inc: a step drives a Net and the CtcWorkspace beside it.

// the frames at x (device) into the net's input block and layer 0's source rows; aux: the CTC metadata copy of a training step rides
// the launch
static void net_ingest(Net& n, CtcWorkspace& ctc, const float* x, const CtcMetaCopy* aux = nullptr) {
  REQUIRE(n.N > 0, "set_batch first");
  n.ensure_training_buffers();   // (the ingest writes layer 0's source rows)
  RoctxRange range_("clstm:ingest");
  Layer& y = n.L[0];
  bool aux_done = false;
  const bool with_pack = n.packed_dirty && n.L.size() == 1 && !y.wide;   // the training step of a narrow net: ingest + weight repack in one launch
  if (with_pack || n.lo_pending || (aux && aux->nwords > 0)) {
    // (any net: the small host arrays of the step ride the ingest launch -- a separate copy of the CTC metadata cost a
    // configs[4] step ~25 us of DMA set-up in front of its first kernel)
    const int M = n.ndir * 4 * y.no, KQP = 4 * y.nk4;
    const size_t nr = (size_t)n.ndir * 4 * KQP * y.nthreads;
    const int nbi = n.ingest_blocks(x), nbp = with_pack ? nblocks((size_t)(1 + y.ni) * M + 2 * nr) : 0;
    const bool lo = n.lo_pending, ax = aux && aux->nwords > 0;
    // optional trailing blocks read small host arrays straight from their pinned slots: the line offsets and -- in a
    // training step -- the CTC metadata (no DMA launches, no event records on the stream's critical path)
    CLSTM_LAUNCH(k_ingest_pack, dim3(nbi + nbp + (lo ? 1 : 0) + (ax ? (aux->nwords + 255) / 256 : 0)), dim3(256), 0, g_stream, x, n.X.p, y.S.p, (size_t)n.N, y.ni, y.lds,
                 n.ndir, (long long)n.N * y.lds, nbi, nbp, (const float*)n.v, y.Wt, y.bias, y.Rf, y.Rb, y.pd, n.pack_fused_desc(y),
                 lo ? n.lo_stage : nullptr, n.line_off.p, 2 * n.bs + 1, ax ? aux->src : nullptr, ax ? aux->dst : nullptr, ax ? aux->nwords : 0,
                 with_pack ? (const int*)n.pack_table(y) : (const int*)nullptr);
    if (lo) { n.ring.commit(g_stream); n.lo_pending = false; }
    if (ax) { ctc.ring.commit(g_stream); aux_done = true; }
    if (with_pack) n.packed_dirty = false;
  } else {
    CLSTM_LAUNCH(k_ingest, dim3(nblocks((size_t)n.N * (1 + y.ni))), dim3(256), 0, g_stream, x, n.X.p, y.S.p, (size_t)n.N, y.ni,
                 y.lds, n.ndir, (long long)n.N * y.lds);
  }
  check_launch();
  if (aux && aux->nwords > 0 && !aux_done) {   // not the fused launch: a plain asynchronous copy
    HIPCHECK(hipMemcpyAsync(aux->dst, aux->src, (size_t)aux->nwords * sizeof(int), hipMemcpyHostToDevice, g_stream));
    ctc.ring.commit(g_stream);
  }
  n.src0_ready = true;
}
// the same ingest as trailing workgroups of a step's last reduction (ops.h: IngestTail; Net::launch_deferred_reduce): the declared
// geometry is the NEXT minibatch's
static IngestTail ingest_tail(const Net& n, const float* x, const CtcMetaCopy& meta) {
  const Layer& y = n.L[0];
  IngestTail t{};
  t.x = x; t.X = n.X.p; t.S = y.S.p; t.N = (unsigned long long)n.N; t.ni = y.ni; t.lds = y.lds; t.ndir = n.ndir; t.sdir = (long long)n.N * y.lds;
  t.nbi = n.ingest_blocks(x);
  t.lo_src = n.lo_pending ? n.lo_stage : nullptr; t.lo_dst = n.line_off.p; t.lo_n = 2 * n.bs + 1;
  t.aux_src = meta.nwords > 0 ? meta.src : nullptr; t.aux_dst = meta.dst; t.aux_n = meta.nwords;
  return t;
}
// CTC alignment of the current minibatch against m's transcripts (m.labels, m.L; one per declared line): the host half, and --
// launch -- the alignment itself.  launch = false (training steps): prepared here, launched behind the forward pass by net_ctc_launch.
static void net_ctc(Net& n, CtcWorkspace& ctc, const Minibatch& m, float* aligned_h, CtcMetaCopy* defer = nullptr, bool launch = true) {
  REQUIRE(n.N > 0, "set_batch first");
  std::vector<int> soff, states;
  expand_transcripts(m.labels, m.L, n.bs, states, soff);
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
  if (!ticket && n.next.matches(cur) && n.src0_ready && !n.lo_pending) {   // (host-fed frames are new with every call)
    n.next.valid = false;                  // declared and ingested by the previous call's tail
    g_path_count[PC_INGEST_TAIL_USED]++;
  } else {
    n.set_batch(cur.T, cur.bs);
    CtcMetaCopy meta;
    net_ctc(n, ctc, cur, nullptr, &meta, false);
    net_ingest(n, ctc, cur.x, &meta);
  }
  n.forward();
  net_ctc_launch(n, ctc);
  PassLeft left = n.backward(n.step_plan(next.given(), ticket));
  if (left.deferred.armed) {
    // (a single narrow layer whose update does not keep the packed weights current: its ingest launch also repacks -- not the tail's job)
    bool tail = !(n.L.size() == 1 && !n.L[0].wide && !left.packs_follow_update);
    if (tail) {
      try {
        n.set_batch(next.T, next.bs);
        CtcMetaCopy meta;
        net_ctc(n, ctc, next, nullptr, &meta, false);
        const IngestTail t = ingest_tail(n, next.x, meta);
        n.launch_deferred_reduce(left.deferred, &t);
        if (t.lo_src) { n.ring.commit(g_stream); n.lo_pending = false; }
        if (t.aux_src) ctc.ring.commit(g_stream);
        n.src0_ready = true;
        n.next.remember(next);
      } catch (...) {
        // the NEXT minibatch is at fault (a bad label, a size): this step still completes; the next call declares its minibatch
        // itself and reports the error where it belongs
        n.next.valid = false;
        tail = false;
      }
    }
    if (!tail) n.launch_deferred_reduce(left.deferred, nullptr);
  }
  n.update(left);
  if (ticket) {
    REQUIRE(left.ticket.word == nullptr, "internal: no kernel of the step took the step word");
    n.hf.commit();
  }
}
