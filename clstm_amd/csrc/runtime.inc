// runtime.inc -- part of clstm_hip.hip (namespace clstm): errors, device buffers and the pinned staging ring, GEMM store functors,
// kernel launch helpers (per-line / fused / lock-step recurrences, hipGraph cache), the layers' kernel choices (narrow_plan, wide_plan, product_plan),
// device error words, per-kernel timing, roctx.
// Not a stand-alone header: included once, inside the namespace, by clstm_hip.hip.

static thread_local std::string g_err;
static thread_local hipStream_t g_stream = nullptr;

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};
#define HIPCHECK(expr)                                                                       \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      throw Error(std::string(#expr) + " failed: " + hipGetErrorString(e_) + " (" + __FILE__ + \
                  ":" + std::to_string(__LINE__) + ")");                                     \
  } while (0)
#define REQUIRE(cond, msg)                    \
  do {                                        \
    if (!(cond)) throw Error(std::string(msg)); \
  } while (0)
#define ABI_BEGIN try {
#define ABI_END                         \
  return 0;                             \
  }                                     \
  catch (const std::exception& e) {     \
    g_err = e.what();                   \
    return 1;                           \
  }                                     \
  catch (...) {                         \
    g_err = "unknown error";            \
    return 1;                           \
  }

static inline int nblocks(size_t n, int bs = 256) {
  size_t b = (n + bs - 1) / bs;
  if (b < 1) b = 1;
  if (b > 4096) b = 4096;
  return (int)b;
}
static void check_launch() { HIPCHECK(hipGetLastError()); }
// The dynamic-LDS ceiling of a kernel (hipFuncAttributeMaxDynamicSharedMemorySize), the one rule: raised when a launch asks for more
// than the kernel has been given so far, never lowered -- a ceiling above a launch's own size is harmless, the launch states its size.
// The ceiling belongs to the function, not to a thread, so the record is process-wide behind a lock (streams and workspaces are
// thread_local; a per-thread record would let a second thread's smaller first request lower what the first thread relies on).
// Not keyed by device: one process drives one GPU (DESIGN.md 4.2, 6), as g_dev_err and device_cu_count() assume.
static void allow_dynamic_lds(const void* kernel, size_t bytes) {   // (declared in gemm_bf16.h, whose gemm_x3_big comes before this file)
#ifndef CLSTM_HIP_EMU
  static std::mutex lock;
  static std::map<const void*, size_t> given;
  const std::lock_guard<std::mutex> hold(lock);
  size_t& have = given[kernel];
  if (bytes <= have) return;
  HIPCHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  have = bytes;
#else
  (void)kernel; (void)bytes;
#endif
}

// zero-fill ordered before everything that follows on ANY stream (see DevBuf::reserve)
static void zero_fill(void* p, size_t bytes) {
  HIPCHECK(hipMemsetAsync(p, 0, bytes, g_stream));
  HIPCHECK(hipStreamSynchronize(g_stream));
}
// Byte accounting (clstm_net_device_bytes): a DevBuf constructed inside an AcctScope -- every buffer of a net and of its CTC / decode
// workspaces: clstm_net_create -- keeps the address of that net's counter and moves it whenever it grows or is released, so a buffer
// added to any of those structs later is counted without anyone listing it.  Buffers constructed outside a scope are not counted.
static thread_local size_t* g_acct = nullptr;
struct AcctScope {
  size_t* prev;
  explicit AcctScope(size_t* c) : prev(g_acct) { g_acct = c; }
  ~AcctScope() { g_acct = prev; }
};
template <class T>
struct DevBuf {  // grow-only device buffer
  T* p = nullptr;
  size_t cap = 0;
  size_t* acct = g_acct;
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) HIPCHECK(hipFree(p));
    p = nullptr;
    if (acct) *acct -= cap * sizeof(T);
    cap = 0;
    size_t want = n + n / 4 + 64;
    HIPCHECK(hipMalloc((void**)&p, want * sizeof(T)));
    // zero-fill on the library stream and wait for it: whatever initialises parts of the fresh buffer next --
    // kernels on this stream (k_fill_col0 ...) or a blocking null-stream copy (the CTC tables) -- is then ordered
    // behind the fill without relying on how a null-stream hipMemset synchronises with a non-blocking stream.
    // Buffers only grow, so this drain happens a handful of times per process (hipFree drains the device anyway).
    zero_fill(p, want * sizeof(T));
    cap = want;
    if (acct) *acct += cap * sizeof(T);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    if (acct) *acct -= cap * sizeof(T);
    cap = 0;
  }
};

// Pinned host staging ring: small per-minibatch host arrays (line offsets, CTC target states) are
// copied here and DMA'd asynchronously, so declaring a batch never drains the stream and the host
// can run ahead of the GPU.  A slot is reused only after the copy recorded on it has completed.
struct PinnedRing {
  // An event record between two kernels costs ~5 us of stream time on MI355X (a barrier packet the next dispatch waits
  // for; profiles/r02_timeline_one_stream.txt of the first version shows the gaps), so slots are recycled in GROUPS:
  // one event per GROUP commits, recorded behind the group's last copy and waited for when the ring comes round to
  // the group's first slot again.
  static const int SLOTS = 32, GROUP = 8;
  void* h[SLOTS] = {};
  size_t cap[SLOTS] = {};
  hipEvent_t ev[SLOTS / GROUP] = {};
  bool busy[SLOTS / GROUP] = {};
  int cur = SLOTS - 1;
  void* acquire(size_t bytes) {
    cur = (cur + 1) % SLOTS;
    const int g = cur / GROUP;
    if (cur % GROUP == 0 && busy[g]) { HIPCHECK(hipEventSynchronize(ev[g])); busy[g] = false; }
    if (cap[cur] < bytes) {
      if (h[cur]) (void)hipHostFree(h[cur]);
      cap[cur] = bytes * 2 + 256;
      HIPCHECK(hipHostMalloc(&h[cur], cap[cur]));
    }
    return h[cur];
  }
  void commit(hipStream_t s) {   // the copy / kernel reading the current slot has been enqueued on s
    if (cur % GROUP != GROUP - 1) return;
    const int g = cur / GROUP;
    if (!ev[g]) HIPCHECK(hipEventCreateWithFlags(&ev[g], hipEventDisableTiming));
    HIPCHECK(hipEventRecord(ev[g], s));
    busy[g] = true;
  }
  ~PinnedRing() {
    for (int i = 0; i < SLOTS / GROUP; i++)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    for (int i = 0; i < SLOTS; i++)
      if (h[i]) (void)hipHostFree(h[i]);
  }
};
// Grow-only pinned host buffer: the landing buffer of a results copy (decode, score), the staging of pageable frames (HostFeed)
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  void reserve(size_t n) {
    if (n <= cap) return;
    if (p) HIPCHECK(hipHostFree(p));
    p = nullptr; cap = 0;
    HIPCHECK(hipHostMalloc((void**)&p, (n + n / 4 + 64) * sizeof(T)));
    cap = n + n / 4 + 64;
  }
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};
// The metadata block of a batched call (ctc_run.inc): its small host arrays, written section by section into one pinned ring slot
// and brought to the device by ONE copy.  add() / put() answer where a section WILL lie on the device and the kernel's arguments are
// filled from that, so the order of the calls is the one statement of a layout.  Sections lie back to back: a block whose records
// hold 8-byte members puts them first.
struct StagedCopy { const int* src = nullptr; int* dst = nullptr; int nwords = 0; };   // a copy its caller folds into a launch (step.inc)
struct StagedBlock {
  template <class T> struct Sec { T* host; const T* dev; };
  PinnedRing ring;
  DevBuf<char> dev;
  char* slot = nullptr;
  size_t cap = 0, used = 0;
  void begin(size_t bytes) { dev.reserve(bytes); slot = (char*)ring.acquire(bytes); cap = bytes; used = 0; }
  template <class T> Sec<T> add(size_t n) {   // n elements the caller writes itself
    REQUIRE(used % alignof(T) == 0 && used + n * sizeof(T) <= cap, "internal: a staged section is misaligned or exceeds its block");
    const size_t at = used;
    used += n * sizeof(T);
    return Sec<T>{reinterpret_cast<T*>(slot + at), reinterpret_cast<const T*>(dev.p + at)};
  }
  template <class T> const T* put(const T* src, size_t n) {
    const Sec<T> sec = add<T>(n);
    if (n) memcpy(sec.host, src, n * sizeof(T));
    return sec.dev;
  }
  template <class T> const T* put(const std::vector<T>& v) { return put(v.data(), v.size()); }
  void send(hipStream_t s) {
    HIPCHECK(hipMemcpyAsync(dev.p, slot, used, hipMemcpyHostToDevice, s));
    ring.commit(s);
  }
  // ... or the caller folds the copy into a kernel it launches anyway, and commits the slot behind that launch
  StagedCopy deferred() const { return StagedCopy{reinterpret_cast<const int*>(slot), reinterpret_cast<int*>(dev.p), (int)(used / sizeof(int))}; }
  void commit(hipStream_t s) { ring.commit(s); }
};
// The result block of a batched call: 4-byte sections (floats travel as their bits) declared in order, in ONE device buffer with a
// pinned landing buffer.  A section's handle gives its device address for the kernel's arguments and, after fetch(), its host copy.
struct ResultBlock {
  struct Span { size_t at = 0, n = 0; };   // words [at, at + n) of the block
  template <class T> struct Sec : Span {
    const ResultBlock* blk = nullptr;
    T* dev() const { return reinterpret_cast<T*>(blk->buf.p + at); }
    const T* host() const { return reinterpret_cast<const T*>(blk->land.p + at); }
  };
  DevBuf<int> buf;
  PinnedBuf<int> land;
  size_t words = 0;
  void begin() { words = 0; }
  template <class T> Sec<T> add(size_t n) {
    static_assert(sizeof(T) == sizeof(int), "result sections are 4-byte words");
    Sec<T> sec;
    sec.at = words; sec.n = n; sec.blk = this;
    words += n;
    return sec;
  }
  void reserve() { buf.reserve(words); }   // every section declared: dev() holds from here on
  void zero(hipStream_t s, Span from, Span to) { HIPCHECK(hipMemsetAsync(buf.p + from.at, 0, (to.at + to.n - from.at) * sizeof(int), s)); }
  // ONE copy brings back the block up to the end of `last` -- the last section the caller asked for -- and the stream is drained
  void fetch(hipStream_t s, Span last) {
    land.reserve(words);
    HIPCHECK(hipMemcpyAsync(land.p, buf.p, (last.at + last.n) * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
};

// ---- GEMM operand functors ---------------------------------------------------------------------
// operator(): one element; row4(): four consecutive columns of one row (c % 4 == 0) when vec4() says the
// destination rows are 16-byte aligned -- the GEMM epilogue then writes whole 256-byte row segments
struct StoreBias {  // out[r*ld + c] = val + bias[c]
  float* out; long long ld; const float* bias;
  DEVMFN void operator()(int r, int c, float v, int) const { out[(long long)r * ld + c] = v + bias[c]; }
  DEVMFN bool vec4() const { return (ld & 3) == 0 && (((size_t)out | (size_t)bias) & 15) == 0; }
  DEVMFN void row4(int r, int c, f32x4 v, int) const {
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + c);
    f32x4 o;
    o[0] = v[0] + b[0]; o[1] = v[1] + b[1]; o[2] = v[2] + b[2]; o[3] = v[3] + b[3];
    *reinterpret_cast<f32x4*>(out + (long long)r * ld + c) = o;
  }
};
// clstm_debug_path_count (diagnostics): the numbers are ABI -- tests and scripts pass them as integers, include/clstm_abi.h explains each
enum PathCounter {
  PC_FWD_PERSISTENT = 0, PC_BWD_PERSISTENT = 1, PC_WX_FROM_BF16 = 2, PC_DX_FROM_BF16 = 3, PC_DW_FROM_BF16 = 4, PC_FWD_FUSED = 5,
  PC_FWD_FUSED_WX = 6, PC_PEER_EXCHANGE = 7, PC_DW_X_EXTERNAL = 8, PC_BWD_C32 = 9, PC_PACKS_FOLLOW_UPDATE = 10, PC_BWD_X3 = 11,
  PC_REPLICA_CHECK = 12, PC_DW_BIAS_OUT = 13, PC_DW_DX_ONE_LAUNCH = 14, PC_MFMA_NOSAVE = 15, PC_MFMA_FWD = 16, PC_MFMA_BWD = 17,
  PC_MFMA_BWD_DW = 18, PC_INGEST_TAIL = 19, PC_INGEST_TAIL_USED = 20, PC_MFMA_ROUTED = 21 /* counted on the device */,
  PC_LINE_NOSAVE = 22, PC_FUSED_NOSAVE = 23, PC_PEER_TWO_PHASE = 24, PC_NORMALIZED = 25, PC_XD_PROLOGUE = 26, PC_XD_PRODUCERS = 27, PC_SCORE = 28, PC_BEAM = 29, PC_BEAM_LM = 30, PC_EDIT = 31, PC_BEAM_LEX = 32, PC_DEGRADED = 33, PC_COUNT
};
static long long g_path_count[PC_COUNT];
struct StorePlain {
  float* out; long long ld;
  DEVMFN void operator()(int r, int c, float v, int) const { out[(long long)r * ld + c] = v; }
  DEVMFN bool vec4() const { return (ld & 3) == 0 && ((size_t)out & 15) == 0; }
  DEVMFN void row4(int r, int c, f32x4 v, int) const { *reinterpret_cast<f32x4*>(out + (long long)r * ld + c) = v; }
};
struct StorePartial {  // split-K slabs [z][R][Cn]
  float* out; int R, Cn;
  DEVMFN void operator()(int r, int c, float v, int z) const { out[((long long)z * R + r) * Cn + c] = v; }
  DEVMFN bool vec4() const { return (Cn & 3) == 0 && ((size_t)out & 15) == 0; }
  DEVMFN void row4(int r, int c, f32x4 v, int z) const {
    *reinterpret_cast<f32x4*>(out + ((long long)z * R + r) * Cn + c) = v;
  }
};
struct StorePartialShift {  // split-K slabs of a product WITHOUT the bias row: operand rows [x | h], row r lands in row r + 1 of [1 | x | h] (R = rows of the slab)
  float* out; int R, Cn;
  DEVMFN void operator()(int r, int c, float v, int z) const { out[((long long)z * R + r + 1) * Cn + c] = v; }
  DEVMFN bool vec4() const { return (Cn & 3) == 0 && ((size_t)out & 15) == 0; }
  DEVMFN void row4(int r, int c, f32x4 v, int z) const { *reinterpret_cast<f32x4*>(out + ((long long)z * R + r + 1) * Cn + c) = v; }
};
struct StorePartialRot {  // split-K slabs whose operand rows were ordered [x | h | 1]: row r lands in row (r + 1) mod R of [1 | x | h]
  float* out; int R, Cn;
  DEVMFN void operator()(int r, int c, float v, int z) const { out[((long long)z * R + (r + 1 == R ? 0 : r + 1)) * Cn + c] = v; }
  DEVMFN bool vec4() const { return (Cn & 3) == 0 && ((size_t)out & 15) == 0; }
  DEVMFN void row4(int r, int c, f32x4 v, int z) const {
    *reinterpret_cast<f32x4*>(out + ((long long)z * R + (r + 1 == R ? 0 : r + 1)) * Cn + c) = v;
  }
};
#ifndef GEMM_BK_DW
#define GEMM_BK_DW 16   // frames staged per barrier pair in the weight-gradient GEMM (32 measured slower: 61.1 vs 58.3 us)
#endif
// ---- the register-resident (narrow, nhidden <= 128) recurrence: every instantiation of its kernels is named HERE, once ----
// The six (NK4, KU) classes of lstm_seq.h: NK4 k-quads per lane, KU the k values per lane actually used -- the padded 4 * NK4 in general,
// exact for the 97..100-cell case (uw3 BiLSTM(100)).  Every class has the per-line kernels (forward, no-save forward, backward, backward
// with the x.d prologue); the columns say what a class has beyond them:
//   FUSED   lstm_fwd_fused_kernel (the fused form needs >= 6 waves, 64 * FWD_CW threads: a polling wave among the first four, consumer
//           waves behind them, so the classes that reach six waves);
//   DW      lstm_bwd_dw_kernel (the thread count must cover the GEMM role's 256: the classes that reach four waves);
//   ROUTED  lstm_fwd_routed_kernel, the per-line twins of the batched-MFMA forward (the classes of its cell counts: 64, 100, 128).
#define NARROW_CLASSES(X) X(1, 4, 0, 0, 0) X(2, 8, 0, 0, 0) X(4, 16, 0, 1, 1) X(7, 25, 1, 1, 1) X(7, 28, 1, 1, 0) X(8, 32, 1, 1, 1)
// ... and the geometries (cells; 48 inputs) of the recurrence batched over 16 lines on the MFMA: NOSAVE lstm_fwd_mfma_kernel<.., false>
// (not the 128-cell one, which spills), BWD lstm_bwd_mfma_rows_kernel / lstm_bwd_mfma_dw_kernel (128 cells: image + operand staging would
// need 176 KB of LDS); every geometry has the saving forward kernel
#define MFMA_GEOMS(X) X(64, 1, 1) X(100, 1, 1) X(128, 0, 0)
struct NarrowClass { int nk4, ku, waves; bool fused, dw, routed; };   // nk4 = 0: no instantiation (the layer is wide); waves = ceil(no / 16)
static NarrowClass narrow_class(int no) {
  const int k4 = (no + 3) / 4, waves = (no + 15) / 16;   // the first class whose 4 NK4 k-quads hold the cells' k4, KU exact or padded
#define ROW_(N, K, F, D, R) if (4 * N >= k4 && (K == 4 * N || K == k4)) return NarrowClass{N, K, waves, F != 0, D != 0, R != 0};
  NARROW_CLASSES(ROW_)
#undef ROW_
  return NarrowClass{0, 0, 1, false, false, false};
}
struct MfmaGeomCaps { int no; bool nosave, bwd; };
static const MfmaGeomCaps* mfma_geom(int no) {
#define ROW_(NO, NOSAVE, BWD) {NO, NOSAVE != 0, BWD != 0},
  static const MfmaGeomCaps table[] = {MFMA_GEOMS(ROW_)};
#undef ROW_
  for (const auto& g : table)
    if (g.no == no) return &g;
  return nullptr;
}
// the lookup: f(NarrowNK<NK4, KU>) for the class if it has capability CAP -- a plan (narrow_plan answers from the same lists) cannot
// name a kernel that is not instantiated, and no kernel is instantiated for a class that has none
[[noreturn]] static void no_instantiation() { throw Error("internal: the plan names a recurrence kernel that is not instantiated"); }
template <int N, int K> struct NarrowNK { static constexpr int NK4 = N, KU = K; };
enum NarrowCap { NCAP_LINE, NCAP_FUSED, NCAP_DW, NCAP_ROUTED };
template <int CAP, class F>
static void narrow_dispatch(int nk4, int ku, F&& f) {
#define CASE_(N, K, FUSED, DW, ROUTED) \
  if constexpr (CAP == NCAP_LINE || (CAP == NCAP_FUSED && FUSED) || (CAP == NCAP_DW && DW) || (CAP == NCAP_ROUTED && ROUTED)) \
    if (nk4 == N && ku == K) { f(NarrowNK<N, K>{}); check_launch(); return; }
  NARROW_CLASSES(CASE_)
#undef CASE_
  no_instantiation();
}
// ... and of the MFMA geometries: f(integral_constant<int, cells>) where the geometry has the kernel asked for
enum MfmaCap { MCAP_FWD, MCAP_NOSAVE, MCAP_BWD };
template <int CAP, class F>
static void mfma_dispatch(int no, F&& f) {
#define CASE_(NO, NOSAVE, BWD) \
  if constexpr (CAP == MCAP_FWD || (CAP == MCAP_NOSAVE && NOSAVE) || (CAP == MCAP_BWD && BWD)) \
    if (no == NO) { f(std::integral_constant<int, NO>{}); check_launch(); return; }
  MFMA_GEOMS(CASE_)
#undef CASE_
  no_instantiation();
}
template <int NK4, int KU, bool SAVE = true>
static void launch_fwd(const LstmSeqArgs& a, int bs, int nthreads, hipStream_t s) {
  const size_t smem = (2 * 4 * (size_t)lstm_qstride(NK4) + 4) * sizeof(float);
  CLSTM_LAUNCH((lstm_fwd_kernel<NK4, KU, SAVE>), dim3(bs, a.ndir), dim3(nthreads), smem, s, a);
}
template <int NK4, int KU>
static void launch_bwd(const LstmSeqArgs& a, int bs, int nthreads, hipStream_t s) {
  const size_t smem = (2 * 16 * (size_t)lstm_qstride(NK4) + 4) * sizeof(float);
  CLSTM_LAUNCH((lstm_bwd_kernel<NK4, KU>), dim3(bs, a.ndir), dim3(nthreads), smem, s, a);
}
template <int NK4, int KU, bool SAVE = true>
static void launch_fwd_fused(const FwdFusedKernelArgs& k, unsigned nblk, int nthreads, hipStream_t s) {
  const size_t smem = (2 * 4 * (size_t)lstm_qstride(NK4) + 4) * sizeof(float);
#ifdef CLSTM_HIP_EMU
  CLSTM_LAUNCH_COOP((lstm_fwd_fused_kernel<NK4, KU, SAVE>), dim3(nblk), dim3(nthreads), smem, s, k);   // emulator: every workgroup live at once
#else
  CLSTM_LAUNCH((lstm_fwd_fused_kernel<NK4, KU, SAVE>), dim3(nblk), dim3(nthreads), smem, s, k);
#endif
}
// save = false: the recurrence role in its no-save form (recognition; lstm_seq.h)
static void launch_lstm_fwd_fused(int nk4, int ku, const FwdFusedKernelArgs& k, unsigned nblk, int nthreads, hipStream_t s, bool save = true) {
  narrow_dispatch<NCAP_FUSED>(nk4, ku, [&](auto c) {
    constexpr int N = decltype(c)::NK4, K = decltype(c)::KU;
    if (save) launch_fwd_fused<N, K>(k, nblk, nthreads, s); else launch_fwd_fused<N, K, false>(k, nblk, nthreads, s);
  });
}
// save = false (forward only): the recurrence in its no-save form (recognition: only h leaves; lstm_seq.h)
static void launch_lstm(bool fwd, int nk4, int ku, const LstmSeqArgs& a, int bs, int nthreads, hipStream_t s, bool save = true) {
  narrow_dispatch<NCAP_LINE>(nk4, ku, [&](auto c) {
    constexpr int N = decltype(c)::NK4, K = decltype(c)::KU;
    if (!fwd) launch_bwd<N, K>(a, bs, nthreads, s); else if (save) launch_fwd<N, K>(a, bs, nthreads, s); else launch_fwd<N, K, false>(a, bs, nthreads, s);
  });
}
// the per-line backward recurrence with the softmax layer's x.d as its prologue (lstm_xd_prologue.h); terms: 3 or 2 (NarrowPlan::terms)
static void launch_lstm_bwd_xd(int nk4, int ku, const LstmSeqArgs& a, const XdArgs& x, int terms, int bs, int nthreads, hipStream_t s) {
  narrow_dispatch<NCAP_LINE>(nk4, ku, [&](auto c) {
    constexpr int N = decltype(c)::NK4, K = decltype(c)::KU;
    const size_t smem = (2 * 16 * (size_t)lstm_qstride(N) + 4) * sizeof(float);
    if (terms >= 3) CLSTM_LAUNCH((lstm_bwd_xd_kernel<N, K, 3>), dim3(bs, a.ndir), dim3(nthreads), smem, s, a, x);
    else CLSTM_LAUNCH((lstm_bwd_xd_kernel<N, K, 2>), dim3(bs, a.ndir), dim3(nthreads), smem, s, a, x);
  });
}
// recurrence + weight-gradient items as two workgroup roles of one launch (lstm_bwd_dw.h); terms: 3, 2 or 0 = f32 MFMA (NarrowPlan::terms)
static void launch_lstm_bwd_dw(int nk4, int ku, const LstmSeqArgs& a, const GemmDwArgs& g, int terms, int nrec, unsigned ngemm, int nthreads, hipStream_t s) {
  narrow_dispatch<NCAP_DW>(nk4, ku, [&](auto c) {
    constexpr int N = decltype(c)::NK4, K = decltype(c)::KU;
    const size_t smem = (2 * 16 * (size_t)lstm_qstride(N) + 4) * sizeof(float);
    if (terms >= 3) CLSTM_LAUNCH((lstm_bwd_dw_kernel<N, K, 3>), dim3(nrec + ngemm), dim3(nthreads), smem, s, a, g, nrec);
    else if (terms) CLSTM_LAUNCH((lstm_bwd_dw_kernel<N, K, 2>), dim3(nrec + ngemm), dim3(nthreads), smem, s, a, g, nrec);
    else CLSTM_LAUNCH((lstm_bwd_dw_kernel<N, K, 0>), dim3(nrec + ngemm), dim3(nthreads), smem, s, a, g, nrec);
  });
}
// the chunked weight-gradient items as a launch of their own, behind a recurrence that has marked every line complete (gemm_dw.h)
static void launch_gemm_dw(const GemmDwArgs& g, int terms, unsigned nblk, hipStream_t s) {
  if (terms >= 3) CLSTM_LAUNCH(gemm_dw_kernel<3>, dim3(nblk), dim3(256), 0, s, g);
  else if (terms) CLSTM_LAUNCH(gemm_dw_kernel<2>, dim3(nblk), dim3(256), 0, s, g);
  else CLSTM_LAUNCH(gemm_dw_kernel<0>, dim3(nblk), dim3(256), 0, s, g);
  check_launch();
}

// lock-step recurrence (lstm_wide.h): one persistent launch for the whole sequence when every workgroup
// can be resident at once (grid <= CU count, weights fit LDS), else one launch per time step
static int device_cu_count() {
#ifndef CLSTM_HIP_EMU
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
  }();
  return n;
#else
  static const int n = getenv("CLSTM_EMU_CUS") ? atoi(getenv("CLSTM_EMU_CUS")) : 16;   // emulator: keeps cooperative test grids small
  return n;
#endif
}
// The per-step launches of one sequence pass are a launch-bound inner loop of up to a few hundred
// dependent kernels: captured once into a hipGraph and replayed while the batch geometry and the buffers
// stay the same (the per-line lengths live in device memory, so only tmax / bs / pointers key the graph).
struct StepGraphCache {
  bool unsupported = false;   // the stream refused capture once: keep launching directly
#ifndef CLSTM_HIP_EMU
  struct Entry { std::vector<char> key; int kind; int tmax; hipGraphExec_t exec; };
  std::vector<Entry> entries;
  // key: the kernel argument struct with the per-step fields zeroed (pointers, geometry), kind: which pass / kernel family
  hipGraphExec_t find(int kind, const std::vector<char>& key, int tmax) {
    for (auto& e : entries)
      if (e.kind == kind && e.tmax == tmax && e.key == key) return e.exec;
    return nullptr;
  }
  void put(int kind, const std::vector<char>& key, int tmax, hipGraphExec_t exec) {
    if (entries.size() >= 16) { (void)hipGraphExecDestroy(entries.front().exec); entries.erase(entries.begin()); }
    entries.push_back(Entry{key, kind, tmax, exec});
  }
  ~StepGraphCache() { for (auto& e : entries) (void)hipGraphExecDestroy(e.exec); }
#endif
};
template <class A>
static std::vector<char> graph_key(A a) {
  a.step = 0;
  std::vector<char> k(sizeof(A));
  memcpy(k.data(), &a, sizeof(A));
  return k;
}
template <class A, class F>
static void launch_steps(StepGraphCache& cache, int kind, const A& a, int tmax, hipStream_t s, F&& body) {
#ifndef CLSTM_HIP_EMU
  if (tmax >= 8) {
    const std::vector<char> key = graph_key(a);
    hipGraphExec_t exec = cache.find(kind, key, tmax);
    if (!exec && !cache.unsupported) {
      hipGraph_t graph = nullptr;
      if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();      // e.g. the legacy default stream cannot be captured: plain launches
        cache.unsupported = true;
      } else {
        body();
        HIPCHECK(hipStreamEndCapture(s, &graph));
        HIPCHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        HIPCHECK(hipGraphDestroy(graph));
        cache.put(kind, key, tmax, exec);
      }
    }
    if (exec) {
      HIPCHECK(hipGraphLaunch(exec, s));
      return;
    }
  }
#endif
  body();
}
// Outcome of the persistent (one launch per pass) recurrence kernels.  The first launches of a process are checked
// synchronously -- a failed placement check (error word 1: nothing written) falls back to the per-step launches for
// good.  Later launches copy their error word into a pinned ring and are checked when the slot comes round again or at
// the next host read-back: the host keeps enqueueing ahead of the GPU (four stream synchronisations per minibatch cost
// ~0.1 ms of idle GPU at the configs[4] shape).
// Device error words shared by every net of the process: [0] sticky outcome of persistent recurrence launches,
// [1] weight-gradient items of the fused backward launch that gave up waiting (gemm_dw.h), [2] waits of the fused FORWARD
// launch that gave up (lstm_fwd_fused.h, lstm_seq.h:wait_chunk), [3] number of the training step whose gradient had a
// non-finite entry (ops.h:k_update; the reference asserts on NaN in every backward step, clstm.cc:630-649), [6] device-side
// peer-barrier waits that timed out (ops.h:k_peer_barrier), [7] the training step at which the replica check found the ranks'
// parameters different (ops.h:k_replica_verify); [4], [5] unused.  The update
// kernels skip the update while any is set; the host throws at its next synchronisation point (clstm_synchronize, any
// read-back).
static int* g_dev_err = nullptr;
static int* dev_err_words() {
  if (!g_dev_err) {
    HIPCHECK(hipMalloc((void**)&g_dev_err, 16 * sizeof(int)));
    zero_fill(g_dev_err, 16 * sizeof(int));
  }
  return g_dev_err;
}
static bool g_xcd_failed = false;   // a persistent launch failed its placement check: wide layers use the per-step launches from now on
struct XcdOutcome {
  // The persistent kernels publish their own outcome (lstm_wide.h:xcd_finish): the last workgroup to leave stores the launch's
  // error word into a pinned host word and -- if non-zero -- into the sticky device word the update kernels look at.  The host
  // marks the slot pending (-1) before the launch; a slot is looked at when the ring comes round to it again (16 launches
  // later: long finished) or at a synchronisation point.  No event record, no extra kernel on the stream.
  static const int SLOTS = 16;
  volatile int* pinned = nullptr;
  bool pending[SLOTS] = {};
  int next = 0, verified = 0;
  void check_slot(int i) {
    if (!pending[i]) return;
    if (pinned[i] == -1) {   // (only when the ring wraps within one un-synchronised burst: wait for that launch)
      const auto t0 = std::chrono::steady_clock::now();
      while (pinned[i] == -1 && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(20)) sched_yield();
      if (pinned[i] == -1) { HIPCHECK(hipDeviceSynchronize()); }
    }
    pending[i] = false;
    const int e = pinned[i];
    if (e > 0 && g_dev_err) (void)hipMemset(g_dev_err, 0, sizeof(int));   // reported once: updates resume
    if (e == 1) g_xcd_failed = true;   // not all workgroups were resident (another tenant on the device): per-step launches from now on
    if (e > 0)
      throw Error(e == 1 ? "persistent recurrence: the workgroups of a later launch were not all resident / not spread evenly over the XCDs (another process or stream on the device?); "
                           "the minibatches enqueued since then were NOT applied -- every later update was skipped; in a multi-layer net the layers above the failing one may "
                           "have taken their update of that one minibatch -- and the library has switched to the per-step launches (CLSTM_XCD_REC=0) for the rest of the process"
                         : "persistent recurrence: a group barrier timed out in the middle of the sequence; the minibatches enqueued since then were NOT applied (layers above the "
                           "failing one may have taken their update of that one minibatch) -- set CLSTM_XCD_REC=0");
  }
  void check_all() { for (int i = 0; i < SLOTS; i++) check_slot(i); }
  // before a launch: the pinned word the kernel reports to (null while launches are still verified synchronously / on the emulator)
  int* prepare() {
#ifdef CLSTM_HIP_EMU
    return nullptr;
#else
    if (verified < 4) return nullptr;
    if (!pinned) { int* p = nullptr; HIPCHECK(hipHostMalloc((void**)&p, SLOTS * sizeof(int))); pinned = p; }
    const int i = next;
    next = (next + 1) % SLOTS;
    check_slot(i);
    pinned[i] = -1;
    pending[i] = true;
    return (int*)(pinned + i);
#endif
  }
  // after it; returns false if the launch failed its placement check and nothing was written (synchronous phase only).
  // last_err_d: the launch's surviving outcome word (XcdSyncLayout::LAST_ERROR)
  bool after_launch(const int* last_err_d, hipStream_t s) {
#ifdef CLSTM_HIP_EMU
    if (*last_err_d != 0 && g_dev_err) g_dev_err[0] = 0;   // handled right here (emulator: device memory is host memory)
    if (*last_err_d == 2) throw Error("persistent recurrence: group barrier timed out");
    return *last_err_d == 0;
#else
    if (verified < 4) {
      int flag = 0;
      HIPCHECK(hipMemcpyAsync(&flag, last_err_d, sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      if (flag == 0) { verified++; return true; }
      if (g_dev_err) (void)hipMemset(g_dev_err, 0, sizeof(int));   // handled right here: nothing was written, the per-step path redoes the pass
      if (flag != 1) throw Error("persistent recurrence: a group barrier timed out in the middle of the sequence; set CLSTM_XCD_REC=0");
      return false;
    }
    return true;
#endif
  }
};
static XcdOutcome g_xcd_outcome;
// after a stream synchronisation: everything enqueued so far has run -- report what the device flagged
static void check_device_errors() {
  g_xcd_outcome.check_all();
  if (!g_dev_err) return;
  int w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHECK(hipMemcpy(w, g_dev_err, sizeof(w), hipMemcpyDeviceToHost));
  if ((w[0] | w[1] | w[2] | w[3] | w[6] | w[7]) == 0) return;
  (void)hipMemset(g_dev_err, 0, sizeof(w));
  if (w[7]) throw Error("data-parallel replicas diverged: the parameter checksums of the ranks differ at training step " + std::to_string(w[7]) + " of a net (replica check, "
                        "CLSTM_REPLICA_CHECK_EVERY); every rank applies the identical update to the identical all-reduced gradient, so this is a fault (a skipped update on "
                        "one rank, memory corruption), not drift -- no update was applied since.  The reference re-broadcasts the weights instead (distribute_weights, clstm.cc:718-729)");
  if (w[6]) throw Error("gradient exchange: " + std::to_string(w[6]) + " wait(s) of the device-side peer barrier timed out (CLSTM_PEER_TIMEOUT_S, default 120 s) although every "
                        "rank's host had announced the exchange: a peer's GPU never reached it; the minibatches enqueued since then were NOT applied -- CLSTM_PEER_ALLREDUCE=0 "
                        "puts the exchange back on RCCL");
  if (w[3]) throw Error("non-finite value (NaN or Inf) in the softmax logits or the gradient of training step " + std::to_string(w[3]) + " of a net (forward passes counted per net "
                        "from 1): no non-finite entry reaches the parameters or the momentum -- a diverged forward pass skips the whole update, a non-finite gradient entry is "
                        "skipped -- and no update enqueued since was applied.  The reference aborts here (clstm.cc:630-649).  Lower the learning rate, or CLSTM_NANCHECK=0 "
                        "to train on regardless");
  if (w[2]) throw Error("fused forward launch: " + std::to_string(w[2]) + " wait(s) for a gate-GEMM chunk / a finished frame block gave up (watchdog): outputs read back since then are "
                        "not valid and the minibatches enqueued since then were NOT applied -- set CLSTM_OVERLAP=0");
  if (w[0] == 1) g_xcd_failed = true;
  if (w[0]) throw Error("persistent recurrence: a launch failed (code " + std::to_string(w[0]) + (w[0] == 1 ? ": workgroups not all resident; per-step launches from now on" : "") +
                        "); the minibatches enqueued since then were NOT applied (layers above the failing one may have taken their update of that one minibatch) -- set CLSTM_XCD_REC=0");
  throw Error("fused backward launch: " + std::to_string(w[1]) + " weight-gradient item(s) gave up waiting for the recurrence (watchdog); the "
              "minibatches since then were NOT applied -- set CLSTM_OVERLAP=0");
}
// synchronous float copies of the accessors (set / get of parameters, outputs, states)
static void copy_h2d(float* dst, const float* src, size_t n) {
  HIPCHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, g_stream));
  HIPCHECK(hipStreamSynchronize(g_stream));
}
static void copy_d2h(float* dst, const float* src, size_t n) {
  HIPCHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIPCHECK(hipStreamSynchronize(g_stream));
  check_device_errors();   // whatever is read back was produced by launches whose outcome is known now
}
static int g_debug_fail_claims = 0;      // tests: this many upcoming persistent launches fail their placement check ...
static int g_debug_fail_skip = 0;        // ... after this many that do not

// ---- the narrow layer (register-resident, nhidden <= 128): WHICH kernels a pass runs, in how many launches, is decided once per layer
// and pass by narrow_plan, a pure function of a NarrowShape (no device, no global, no environment, no option: Net::narrow_shape reads those
// into the shape); the passes of net.inc only execute the plan.  clstm_debug_narrow_plan asks narrow_plan without a net: both structs are
// plain ints in the order documented in include/clstm_abi.h.
enum NarrowPass { NP_FWD_SAVE = 0, NP_FWD_NOSAVE, NP_BWD };
enum NarrowFwd { NF_NONE = 0, NF_LINE, NF_FUSED, NF_MFMA };   // one workgroup per line (lstm_seq.h) | the whole forward half as one launch (lstm_fwd_fused.h) | 16 lines per workgroup on the MFMA (lstm_mfma.h)
enum NarrowBwd {
  NB_NONE = 0,
  NB_LINE,           // lstm_bwd_kernel; the weight gradient is a product behind it (family Narrow)
  NB_LINE_DW,        // (Overlapped) lstm_bwd_kernel, then gemm_dw_kernel: the items find every progress word complete
  NB_LINE_XD_DW,     // (Overlapped) lstm_bwd_xd_kernel -- the x.d prologue in every workgroup -- then gemm_dw_kernel
  NB_BWD_DW,         // (Overlapped) ONE launch, lstm_bwd_dw_kernel: the recurrence's workgroups first, the items behind them
  NB_MFMA,           // lstm_bwd_mfma_rows_kernel alone (family Narrow)
  NB_MFMA_THEN_DW,   // (Overlapped) lstm_bwd_mfma_rows_kernel (it marks its lines complete), then gemm_dw_kernel
  NB_MFMA_DW         // (Overlapped) ONE launch, lstm_bwd_mfma_dw_kernel: the batched recurrence and the items
};
struct NarrowShape {
  int pass, no, ni, ndir;                  // NarrowPass; the layer: cells, inputs, directions
  int nlayers, first, top;                 // layers of the net; this one is the first / the top one
  int bs, tmax, N, nc;                     // the minibatch: lines, longest line, frames; classes of the softmax layer
  int ldh, lds, ldx, h_cap, d_cap;         // what the 32-bit offsets must cover: row strides of H, S and the input rows, capacities of H and D (floats)
  int wk, wk_njp, w1k_kps;                 // the fused forward's operands: Wk packed, its column tiles, the softmax rows' padded k
  int overlap, bf16_gemm, strict_f32;      // clstm_net_set_overlap / CLSTM_OVERLAP, clstm_net_set_gemm_precision, clstm_net_set_strict_f32
  int dw_x3, split_terms;                  // options read when the net was created (strict_f32 clears dw_x3)
  int fwd_mfma, bwd_mfma, bwd_mfma_fused, xd_prologue;   // options read per pass (forward passes: fwd_mfma; backward: the other three)
  int ncu, emu;                            // CUs of the device; this is the host emulator build
};
struct NarrowPlan {
  int nk4, ku, waves;                      // the class (narrow_class)
  int fwd, saves;                          // forward passes: NarrowFwd, and whether it runs its saving form (G, C, S written)
  int overlapped, bwd;                     // backward: the family is Overlapped (the chunked weight-gradient items in or behind the launch), NarrowBwd
  int terms;                               // ... split-term instantiation of the items and of the x.d prologue: 3, 2, or 0 = f32 MFMA
  int dwx, xd;                             // top layer: the softmax layer's W.d slabs ride its launch; x.d form 0 a launch of its own, 1 the whole prologue, 2 producers
  int moves;                               // bit c: the pass moves path counter c
};
static const int PROG_LINES = 2048;        // progress words exist for minibatches up to this many lines (Net::PROG_WORDS)
static NarrowPlan narrow_plan(const NarrowShape& h) {
  NarrowPlan p{};
  const NarrowClass k = narrow_class(h.no);
  p.nk4 = k.nk4; p.ku = k.ku; p.waves = k.waves;
  const int nthreads = 64 * k.waves, ncu = h.ncu;
  const MfmaGeomCaps* const mg = mfma_geom(h.no);
  const double lim = 2147483000.0;   // 32-bit byte offsets inside one descriptor
  const bool gates32 = (double)h.N * h.ndir * 4 * h.no * 4 < lim;
  const bool big_enough = h.overlap != 1 || (h.tmax >= 64 && h.N >= 2048);   // overlap = 1: smaller minibatches are too small to profit
  if (h.pass != NP_BWD) {
    // ---- THE launch rule of the forward pass: forward_pass (training and recognition) launches by it and reserve_batch sizes the predict
    // geometry by it -- nothing else decides.  The batched recurrence goes before the fused launch (which only a net of one narrow layer
    // can take); the strict and forced options act through the two rules.
    // Chip-filling minibatches: the recurrence batched over 16 lines per workgroup on the MFMA (lstm_mfma.h).  fwd_mfma: 0 never, 1 (default)
    // from 640 lines per GPU on (measured crossover, profiles/r06_mfma_v3_vs_perline.txt: below that the launch has fewer 16-line workgroups
    // than the chip has CUs and the per-line kernel wins), 2 always (tests).  clstm_net_set_strict_f32: never by the rule (its products are
    // f16 split products, not the f32 MFMA's); the forced option wins.  The instantiated (cells, inputs) geometries: MFMA_GEOMS x 48.
    const bool mfma = !h.emu && h.fwd_mfma && !h.bf16_gemm && !(h.strict_f32 && h.fwd_mfma < 2) && mg && h.ni == 48 && (!h.first || k.routed) &&
                      gates32 && (double)h.N * h.ldh * 4 < lim && (double)h.N * h.lds * 4 < lim && (double)h.N * h.ldx * 4 < lim &&
                      (h.fwd_mfma >= 2 || h.bs >= 640);
    // The forward half as one launch: W_x GEMM producers + recurrence + softmax consumers (lstm_fwd_fused.h).  Six waves (FWD_CW) of which the
    // last lane owns no cell, at most FWD_JW column tiles per wave, the softmax operand in FWD_CG 16-k groups of registers; H addressed by 32-bit
    // byte offsets.  The recurrence workgroups (one per CU, dispatched first) wait for producers: CUs must be left for those.
    const bool fused = !mfma && h.overlap && h.nlayers == 1 && !h.bf16_gemm && h.wk && k.fused && nthreads >= 64 * FWD_CW && h.no % 16 != 0 &&
                       h.wk_njp <= FWD_JW * FWD_CW && h.w1k_kps <= 16 * FWD_CG && h.nc <= SMX_COLS && h.bs <= PROG_LINES && h.bs < (1 << 18) &&
                       h.tmax < (1 << 16) && big_enough && (double)h.h_cap * 4.0 < lim && h.bs * h.ndir <= ncu - std::max(8, ncu / 8);
    p.fwd = mfma ? NF_MFMA : fused ? NF_FUSED : NF_LINE;
    // ... and whether that family runs its training form -- G, C and S written -- in a pass that asked for save or not: always when asked
    // to, and where the family has no no-save instantiation for the layer
    p.saves = h.pass == NP_FWD_SAVE || (mfma && !mg->nosave);
    p.moves = mfma ? 1 << (p.saves ? PC_MFMA_FWD : PC_MFMA_NOSAVE) : fused ? 1 << (p.saves ? PC_FWD_FUSED : PC_FUSED_NOSAVE) : p.saves ? 0 : 1 << PC_LINE_NOSAVE;
    return p;
  }
  // ---- THE launch rule of the backward pass: the layer loop, the slab count, the weight-gradient step and backward_softmax all read this plan.
  // Overlapped: recurrence and the chunked weight-gradient GEMM (gemm_dw.h) side by side.  The reporting lane must own no cell; progress words
  // for up to PROG_LINES lines at the tail of D, addressed by 32-bit byte offsets; by the rule (overlap = 1) only where the one-launch form
  // with its two workgroup roles exists (lstm_bwd_dw.h: four waves), forced (overlap = 2: tests) everywhere.
  p.overlapped = !h.bf16_gemm && h.overlap && h.no % 16 != 0 && h.bs <= PROG_LINES && big_enough && (double)h.d_cap * 4.0 < lim &&
                 (h.overlap == 2 || nthreads >= 256);
  // bwd_mfma: the batched backward twin (lstm_mfma_bwd.h): 0 never, 1 (default) from 640 lines per GPU on, 2 always (tests).  It gives up the
  // fused launch (the weight-gradient items then run behind it as a launch of their own).  Crossover with the per-line fused launch, whole
  // step (profiles/r06_mfma_bwd_leaveout.txt): 512 lines 311.9k vs 327.3k lines/s, 640: 343.6k vs 330.4k, 768: 373.7k vs 355.8k, 896: 403.7k
  // vs 358.4k.  (strict: R^T.delta from two bf16 terms is not what strict promises; forced: the option wins)
  const bool mfma = !h.emu && h.bwd_mfma && !h.bf16_gemm && !(h.strict_f32 && h.bwd_mfma < 2) && mg && mg->bwd && gates32 && (h.bwd_mfma >= 2 || h.bs >= 640);
  p.terms = !h.dw_x3 ? 0 : h.split_terms >= 3 ? 3 : 2;   // (the launch rounds split_terms to one of the two, as gemm_x3 does)
  // The softmax layer's W.d depends on nothing the backward recurrence produces: when the top layer's backward runs overlapped its slabs are
  // items of THAT launch (only while the recurrence leaves CUs idle: with 256 lines the same items cost the fused launch +42 us for 19 saved)
  p.dwx = h.top && h.dw_x3 && p.overlapped && (long long)h.bs * h.ndir * 4 <= 3LL * ncu;
  // Does the top layer's backward launch compute the softmax layer's x.d itself (lstm_xd_prologue.h)?  All of:
  //  * dwx -- this pass's condition for the lone x.d launch: top layer Overlapped, dw_x3, bs * ndir * 4 <= 3 * CUs;
  //  * the per-line recurrence kernel runs it (one launch or, below four waves / on the host emulator, the two-launch form): the batched-MFMA
  //    backward recurrence keeps the separate launch;
  //  * the split is two or three bf16 terms (dw_x3 says so);
  //  * nc <= XD_MAX_K = 96: three k-blocks of W fragments (3 x NT x 4 VGPRs) stay in registers for the whole prologue, and three blocks are
  //    what the launch it replaces runs for such nc, zero blocks included (bit-identity);
  //  * experiment option xd_prologue (default 2: the producer form where admitted, else as 1; 1 the whole prologue; 0 the separate launch).
  // (Every class's smallest workgroup covers a staging round, nthreads * xd_maxu(nk4) >= XD_UNITS: checked once, in Net::build.)
  // Lines: inherits dwx's bound (bs * ndir <= 192 on 256 CUs); measured 64 / 96 bidirectional lines, EXPERIMENTS 15.
  // Form 2, the producer form: the recurrence workgroup computes only the 32 frames it visits first, helper items of the same launch the rest.
  // It needs the one-launch form (below) and recurrence workgroups on at most half of the CUs -- the items are workgroups of its helper role, one
  // wave per column tile like the recurrence role -- i.e. a CU of its own for every item: an item that shares a CU with a recurrence workgroup takes issue
  // slots from the latency-bound time loop (96 bidirectional lines, 192 + 192 workgroups on 256 CUs: form 2 measured 5.5 us per step SLOWER
  // than form 1; 64 lines, 128 + 128: 4.1 us faster -- profiles/ab_xd_producers.txt).  Whatever is eligible for 1 but not for 2 runs 1 unchanged.
  const bool one_launch = !h.emu && k.dw && nthreads >= 256 && !mfma;   // (the emulator, and layers too narrow for the GEMM role's 256 threads when the tests force the path: two launches)
  p.xd = !(p.dwx && !mfma && h.nc <= XD_MAX_K && h.xd_prologue != 0) ? 0 : h.xd_prologue >= 2 && one_launch && (long long)h.bs * h.ndir * 2 <= ncu ? 2 : 1;
  if (!p.overlapped) p.bwd = mfma ? NB_MFMA : NB_LINE;
  // the batched recurrence and the items as ONE launch pays while the recurrence leaves most CUs idle -- same box, lines/s fused vs separate:
  // 640 lines 368.1k vs 340.0k, 768: 395.7k vs 374.8k, 896: 398.0k vs 395.1k, 960: 406.6k vs 407.9k, 1024: 414.6k vs 419.0k, 1536: 430.2k vs
  // 471.2k; option bwd_mfma_fused: 0 never, 1 that rule, 2 always (tests); instantiated for three split terms only
  else if (mfma) p.bwd = h.bwd_mfma_fused && p.terms == 3 && (h.bwd_mfma_fused >= 2 || h.bs < 900) ? NB_MFMA_DW : NB_MFMA_THEN_DW;
  else p.bwd = one_launch ? NB_BWD_DW : p.xd ? NB_LINE_XD_DW : NB_LINE_DW;
  p.moves = (mfma ? 1 << PC_MFMA_BWD : 0) | (p.bwd == NB_MFMA_DW ? 1 << PC_MFMA_BWD_DW : 0) | (p.xd == 2 ? 1 << PC_XD_PRODUCERS : p.xd ? 1 << PC_XD_PROLOGUE : 0);
  return p;
}
static void count_moves(int moves) {
  for (int c = 0; c < PC_COUNT; c++)
    if (moves >> c & 1) g_path_count[c]++;
}

// ---- the matrix products around the recurrences -- the input projection W_x.x, the softmax layer's logits, its W.d and x.d, a layer's weight
// gradient and its input deltas: WHICH kernel, tile, row count and slab count each is launched with, which bf16 arrays a pass writes for them and
// which f32 stores it skips, is decided once per layer and pass by product_plan, a pure function of a ProductShape (no device, no global, no
// environment, no option, no pointer: Net::product_shape reads those into the shape); the passes of net.inc and the launchers of gemm_bf16.h only
// execute the plan.  clstm_debug_product_plan asks product_plan without a net: both structs are plain ints in the order documented in
// include/clstm_abi.h.
enum ProductPass { PP_FWD = 0, PP_BWD };
enum ProductKernel {
  PK_NONE = 0,        // nothing launched for it: part of a recurrence launch (fused forward, batched MFMA, the Overlapped items, the x.d prologue)
  PK_F32,             // gemm_f32, 64 x 64 tiles
  PK_BF16,            // gemm_bf16: f32 operands rounded on the way in, 64- or 128-tiles
  PK_B16KK,           // gemm_b16kk: both operands bf16 and k-contiguous as their producers left them, 128- or 256-tiles
  PK_B16MC,           // gemm_b16mc: both operands bf16 and contraction-major, 128 x 128, 192 x 256 or 256 x 256 tiles
  PK_DW_DX,           // gemm_dw_dx: the weight gradient (as PK_B16MC) and the input deltas (as PK_B16KK, 256-tiles) as ONE launch
  PK_X3,              // gemm_x3: f32-grade bf16 split product, 64-tiles
  PK_X3_BIG,          // gemm_x3_big: the same on 128 x 128 tiles
  PK_X3_PAIR,         // gemm_x3_pair: the softmax layer's W.d and x.d as one launch
  PK_F32_PAIR,        // gemm_f32_pair: the same on the f32 MFMA
  PK_SOFTMAX_FUSED    // softmax_fwd: logits, limexp and normalisation in one kernel (tile 0: the kernel's own)
};
enum ProductWrites { PW_SBF = 1, PW_HBF = 2, PW_DBF = 4 };               // bf16 arrays the recurrence of the pass writes: Sbf | Hbf | Dbf and dbias
enum ProductSkips { PS_H = 1, PS_S = 2, PS_D = 4 };                      // f32 stores its persistent kernel may skip: H | the h columns of S | D
enum ProductNeeds { PN_SOURCE = 1, PN_DELTA_F32 = 2, PN_H_BELOW = 4 };   // built first: ensure_source | ensure_delta_f32 | ensure_h_f32 of the layer below
struct ProductShape {
  int pass;                                    // ProductPass
  int ni, no, ndir, wide;                      // the layer: inputs, cells, directions, lock-step
  int first, top, nlayers;                     // it is the first / the top layer; layers of the net
  int bwd_exact, kp16f_is_no;                  // Layer::bwd_exact, kp16f == no (the rule reads no row stride: those it needs follow from ni, no, ndir)
  int N, bs;                                   // the minibatch: frames, lines (bs: carried, read by no rule today)
  int nclasses, sm_ni;                         // the softmax layer
  int precision, gemm_x3_on, split_terms, strict;   // clstm_net_set_gemm_precision 0 / 1 / 2; options read at net creation; clstm_net_set_strict_f32
  int gemm_b16mc, gemm_stag, pack_tiles, fuse_wx;   // options read per pass
  int ncu, want_dx0;                           // CUs of the device; clstm_net_enable_input_deltas
  int fwd_family, overlapped, dwx, xd;         // the layer's recurrence plan: NarrowPlan::fwd (a wide layer: NF_NONE) / overlapped / dwx / xd
  int dw_slabs_per_dir, dwx_nslabs;            // slab counts of the Overlapped items' tables (Net::build_dw_tables, build_dwx_table)
  // facts of earlier launches:
  int below_hbf;                               // the layer below ran its persistent bf16 forward kernel and left Hbf
  int fwd_sbf;                                 // this layer's forward pass ran persistent and wrote Sbf
  int bwd_persistent;                          // its backward recurrence ran persistent (known once launched: Net::backward completes the shape)
  int packs, above_packs;                      // the bf16 packs of W_x (Wtb, WtbT) exist for this layer / for the layer above
};
struct Product { int kernel, tile, rows, slabs; };   // ProductKernel; rows of a tile (64 / 128 / 192 / 256); rows it is launched with; split-K slabs per direction
struct ProductPlan {
  Product wx, logits;                          // forward: the input projection (behind the folded one where that does not run: fx_mode) | the softmax layer's logits (top layer)
  Product sm_wd, sm_xd, dw, dx;                // backward: the softmax layer's W.d and x.d (top layer) | the layer's weight gradient | its input deltas
  int merged;                                  // dw and dx are one launch (PK_DW_DX)
  int bias_out;                                // the bias row is produced outside dw (k_bias_rows from dbias)
  int dw16_rows, dw16_tile, x_external;        // FROM THE SHAPE AND MODE ALONE, equal in both passes whatever the facts: rows and tile height of the
                                               // bf16-source weight gradient, and whether the x block fills whole tiles of it (may stay external, A2)
  int a2_rows;                                 // ... and does: rows the product reads from the layer below's Hbf instead of copies in Sbf (0: copied)
  int x_copy;                                  // wx reads a bf16 copy of the input frames (k_to_bf16 first)
  int fx_mode;                                 // WideShape::fx_mode: option fuse_wx where the folded input projection has its operands, else 0
  int tiled_pack;                              // Net::repack: every bf16 copy of the layer by k_pack_wide_tiles
  int stag, terms;                             // option gemm_stag for PK_B16KK / PK_B16MC; split terms (3 / 2) for PK_X3 / PK_X3_PAIR
  int writes, skips, needs;                    // ProductWrites, ProductSkips, ProductNeeds
  int moves;                                   // bit c: the pass moves path counter c (2, 3, 4, 8, 13, 14)
};
// shapes that fill 128 x 128 tiles reasonably
static bool gemm_bf16_big(int R, int Cn) { return R >= 96 && Cn >= 96; }
// 256 x 256 tiles where the problem is large enough and their padding costs at most 25 % more work than 128 x 128 tiles do:
// the big tile runs ~1.4x faster per flop (1537 rows: 7 x 256 vs 13 x 128, + 8 %; 561 rows: 3 x 256 vs 5 x 128, + 20 %:
// 98 vs 116 us for one direction of the first layer's weight gradient)
static bool gemm_tile256(int R, int Cn) {
  if (R < 192 || Cn < 192) return false;
  const long long w256 = (long long)((R + 255) / 256) * ((Cn + 255) / 256) * 4, w128 = (long long)((R + 127) / 128) * ((Cn + 127) / 128);
  return 4 * w256 <= 5 * w128;
}
// tile height of the big-tile contraction-major product: 256 rows, or 192 where that pads R less (576 = 3 x 192)
static int gemm_mc_tile_rows(int R) {
  const int p256 = (R + 255) / 256 * 256, p192 = (R + 191) / 192 * 192;
  return p192 < p256 ? 192 : 256;
}
// rows of one output tile of gemm_b16mc / gemm_dw_dx for an R x Cn product
static int gemm_mc_rows_per_tile(int R, int Cn) { return gemm_tile256(R, Cn) ? gemm_mc_tile_rows(R) : GB2_BT; }
static ProductPlan product_plan(const ProductShape& h) {
  ProductPlan p{};
  const bool bf16_gemm = h.precision >= 1, bf16_rec = h.precision == 2, x3 = h.gemm_x3_on && !h.strict;
  const int N = h.N, M = h.ndir * 4 * h.no, R = 1 + h.ni + h.no, Cn = 4 * h.no, nc = h.nclasses;
  const auto sq = [](int R_, int Cn_) { return gemm_bf16_big(R_, Cn_) ? GB2_BT : GEMM_BT; };   // 128- or 64-tiles of gemm_bf16
  const auto kk = [](int R_, int Cn_) { return gemm_tile256(R_, Cn_) ? 256 : GB2_BT; };        // 256- or 128-tiles of gemm_b16kk
  // split-K slabs for the weight-gradient GEMMs: enough workgroups to cover the CUs, at least 64 frames per slab, 1..64 slabs
  const auto clamp_split = [&](long long want) { return (int)std::max(1LL, std::min({want, ((long long)N + 63) / 64, 64LL})); };
  const auto split = [&](int R_, int Cn_, int nbatch, int tile) {
    const long long tiles = (long long)((R_ + tile - 1) / tile) * ((Cn_ + tile - 1) / tile) * nbatch;
    const long long target = tile == GEMM_BT ? 640 : 480;   // 64 x 64 tiles: 640 workgroups measured best (272: slower); 128 x 128 tiles: two workgroups per CU
    return clamp_split((target + tiles - 1) / tiles);
  };
  // big tiles of the contraction-major bf16 product (256 or 192 rows x 256 columns): one workgroup per CU, never a second round
  const auto split_mc = [&](int R_, int Cn_, int nbatch) {
    const int th = gemm_mc_tile_rows(R_);
    return clamp_split(h.ncu / ((long long)((R_ + th - 1) / th) * ((Cn_ + 255) / 256) * nbatch));
  };
  p.stag = h.gemm_stag; p.terms = h.split_terms >= 3 ? 3 : 2;
  // ---- ONE answer for both passes.  Rows of the bf16-source weight gradient: R - 1 when the bias row is produced outside it (1 + ni + no rows
  // are one more than a whole number of row panels at both configs[4] layers -- 1537 = 6 x 256 + 1: a seventh panel, 14 % of the product, for
  // one row; 577 = 3 x 192 + 1), else R.  The forward pass leaves the x block of Sbf external (a2_rows) only where it fills whole tiles of THAT
  // height, and the backward pass launches with these same fields: nothing here reads a fact that is unknown during the forward pass.
  // (Requiring BOTH R and R - 1 to fit, the first form of this rule, switched the path off at configs[4]: 1537 rows pick 192-row tiles.)
  p.dw16_rows = h.bwd_exact && gemm_bf16_big(R - 1, Cn) ? R - 1 : R;
  p.dw16_tile = gemm_mc_rows_per_tile(p.dw16_rows, Cn);
  p.x_external = bf16_rec && !h.first && h.ni % p.dw16_tile == 0;
  // this layer takes the bf16 rows the layer below left as they are (its ni is ndir x the cells below: Net::build)
  const bool x_from_hbf = bf16_rec && !h.first && h.below_hbf && h.packs && (h.ni & 1) == 0;
  if (h.pass == PP_FWD) {
    p.tiled_pack = h.wide && bf16_rec && h.no % 128 == 0 && h.ni % 32 == 0 && h.kp16f_is_no && h.bwd_exact && h.pack_tiles;
    if (h.wide && bf16_rec) {
      // bf16 source rows [x | h_{t-1} | 1] for the weight-gradient product; bf16 outputs for the layer above.  Stores nobody reads in this mode
      // (the per-frame stores of the persistent kernel cost per INSTRUCTION, seven per wave and step; measured at configs[4]: forward passes
      // 1.647 -> 1.580 ms per minibatch): the f32 outputs of a layer whose consumer takes Hbf, the f32 h_{t-1} source columns when the weight
      // gradient takes Sbf.  ensure_h_f32 / ensure_source rebuild them exactly.  (Only the persistent kernel reads the skips.)
      if (h.gemm_b16mc && (h.ni & 7) == 0 && (h.no & 7) == 0 && h.bwd_exact) { p.writes |= PW_SBF; p.skips |= PS_S; }
      if ((h.no & 1) == 0 && !h.top) { p.writes |= PW_HBF; if (h.above_packs) p.skips |= PS_H; }
    }
    // the input projection folded into the persistent forward kernel (wide_plan's gate; here only whether its operands exist: the bf16 rows the
    // layer below left, or a bf16 copy of the input frames)
    p.fx_mode = h.wide && bf16_rec && h.packs && (h.first || x_from_hbf) ? h.fuse_wx : 0;
    if (!h.first && !x_from_hbf) p.needs |= PN_H_BELOW;   // the products read the f32 outputs of the layer underneath
    if (h.fwd_family == NF_FUSED) return p;               // the launch is the whole forward half, logits included
    if (h.fwd_family == NF_MFMA) p.wx = Product{};        // the input product is part of the batched recurrence
    else if (x_from_hbf) p.wx = Product{PK_B16KK, kk(N, M), N, 1};
    // first layer: a bf16 copy of the input frames (N x ni, a few MB) buys the bf16-source kernel with its 256 x 256 tiles and 16-byte stores
    // for the product whose 4 M floats of pre-activations per frame-line are its whole cost
    else if (bf16_rec && h.first && h.wide && h.packs && (h.ni & 7) == 0 && gemm_tile256(N, M)) { p.wx = Product{PK_B16KK, 256, N, 1}; p.x_copy = 1; }
    else if (bf16_gemm) p.wx = Product{PK_BF16, sq(N, M), N, 1};
    else p.wx = Product{PK_F32, GEMM_BT, N, 1};
    if (p.wx.kernel == PK_B16KK) p.moves |= 1 << PC_WX_FROM_BF16;
    p.a2_rows = x_from_hbf && p.x_external ? h.ni : 0;    // (where Sbf is written: else nobody reads it)
    // the fused softmax up to SMX_COLS classes; beyond, in the bf16 modes: f32-grade bf16 x 3 on 128 x 128 tiles (88 -> ~30 us at configs[4])
    if (h.top) p.logits = nc <= SMX_COLS ? Product{PK_SOFTMAX_FUSED, 0, N, 1} : bf16_gemm && x3 && gemm_bf16_big(N, nc) ? Product{PK_X3_BIG, GB2_BT, N, 1} : Product{PK_F32, GEMM_BT, N, 1};
    return p;
  }
  if (h.wide && bf16_rec && h.bwd_exact) {
    // per-frame bf16 deltas and per-line bias sums; with bf16 GEMMs behind it nobody reads the f32 deltas of a persistent pass (16 bytes per
    // lane and step, 0.17 ms per configs[4] minibatch): ensure_delta_f32 expands Dbf for a fallback product
    p.writes |= PW_DBF;
    if (bf16_gemm) p.skips |= PS_D;
  }
  if (h.top) {
    // the softmax layer's W.d (split-K slabs) and x.d.  W.d depends on nothing the backward recurrence produces: where the top layer's plan says
    // so (dwx) its slabs are items of THAT launch and only x.d stays in front of it -- or rides it too (xd).  Else in ONE launch: two small
    // independent products, each mostly prologue and epilogue latency on its own (13.9 + 12.4 us back to back); bf16 modes, shapes that fill
    // 128 x 128 tiles: two launches of the big-tile f32-grade kernel
    const int sR = 1 + h.sm_ni;
    const bool sm_big = bf16_gemm && x3 && gemm_bf16_big(sR, nc) && gemm_bf16_big(N, h.sm_ni);
    const int ns = h.dwx ? h.dwx_nslabs : split(sR, nc, 1, sm_big ? GB2_BT : GEMM_BT);
    const int pair = x3 ? PK_X3_PAIR : PK_F32_PAIR;
    p.sm_wd = h.dwx ? Product{PK_NONE, GEMM_BT, sR, ns} : sm_big ? Product{PK_X3_BIG, GB2_BT, sR, ns} : Product{pair, GEMM_BT, sR, ns};
    p.sm_xd = h.dwx ? Product{h.xd ? PK_NONE : PK_X3, GEMM_BT, N, 1} : sm_big ? Product{PK_X3_BIG, GB2_BT, N, 1} : Product{pair, GEMM_BT, N, 1};
  }
  // the weight gradient from both operands in bf16 as their producers left them (Sbf: the forward pass, Dbf: the persistent backward recurrence)
  const bool dw16 = bf16_rec && h.bwd_persistent && h.fwd_sbf && h.bwd_exact && gemm_bf16_big(R, Cn);
  const int rows = dw16 ? p.dw16_rows : R;
  p.bias_out = rows < R;
  // exact-f32 mode, wide layer: the backward products as f32-grade bf16 x 3 on 128 x 128 tiles -- what narrow layers already do inside their
  // fused backward launch; gemm_x3 = 0 / clstm_net_set_strict_f32: the f32 MFMA
  const bool x3_big = !bf16_gemm && h.wide && x3 && gemm_bf16_big(R, Cn);
  const int ns = h.overlapped ? h.dw_slabs_per_dir
                 : p.bias_out && gemm_tile256(rows, Cn) ? split_mc(rows, Cn, h.ndir)
                 : dw16 && gemm_tile256(R, Cn) ? split_mc(R, Cn, h.ndir)
                 : (bf16_gemm || x3_big) && gemm_bf16_big(R, Cn) ? split(R, Cn, h.ndir, GB2_BT) : split(R, Cn, h.ndir, GEMM_BT);
  // the input deltas from the bf16 deltas and the bf16 pack of W_x^T
  const bool has_dx = !h.first || h.want_dx0, dx16 = bf16_rec && h.bwd_persistent && h.bwd_exact && h.packs;
  // ... and where the layer owes both from the same bf16 delta array: BOTH products as one launch (apart, each leaves a quarter of the chip
  // idle).  Both on their big tiles, the x.d role's operands (contraction length M) by LDS-DMA
  p.merged = dw16 && p.bias_out && !h.first && dx16 && h.gemm_stag == 2 && gemm_tile256(rows, Cn) && gemm_tile256(N, h.ni) && M % GB_BK == 0 && M >= 2 * GB_BK;
  p.dw = h.overlapped ? Product{PK_NONE, GEMM_BT, R, ns} : dw16 ? Product{p.merged ? PK_DW_DX : PK_B16MC, p.dw16_tile, rows, ns}
         : bf16_gemm ? Product{PK_BF16, sq(R, Cn), R, ns} : x3_big ? Product{PK_X3_BIG, GB2_BT, R, ns} : Product{PK_F32, GEMM_BT, R, ns};
  if (has_dx)
    p.dx = p.merged ? Product{PK_DW_DX, 256, N, 1} : dx16 ? Product{PK_B16KK, kk(N, h.ni), N, 1} : bf16_gemm ? Product{PK_BF16, sq(N, h.ni), N, 1}
           : h.wide && x3 && gemm_bf16_big(N, h.ni) ? Product{PK_X3_BIG, GB2_BT, N, 1} : Product{PK_F32, GEMM_BT, N, 1};
  p.a2_rows = dw16 && x_from_hbf && p.x_external ? h.ni : 0;
  if (!dw16) p.needs |= PN_SOURCE | PN_DELTA_F32;   // the f32-source products read S and D
  if (has_dx && p.dx.kernel != PK_DW_DX && p.dx.kernel != PK_B16KK) p.needs |= PN_DELTA_F32;
  p.moves = (dw16 ? 1 << PC_DW_FROM_BF16 : 0) | (p.bias_out ? 1 << PC_DW_BIAS_OUT : 0) | (p.a2_rows ? 1 << PC_DW_X_EXTERNAL : 0) |
            (p.merged ? 1 << PC_DW_DX_ONE_LAUNCH : 0) | (p.dx.kernel == PK_DW_DX || p.dx.kernel == PK_B16KK ? 1 << PC_DX_FROM_BF16 : 0);
  return p;
}

// ---- the lock-step layer (lstm_wide.h): WHICH of its eleven kernels runs is decided once per pass by wide_plan, a pure function of a
// WideShape (no device, no global, no environment: the caller reads those into the shape -- Net::wide_shape); launch_lstm_wide only
// executes the plan.  clstm_debug_wide_plan asks wide_plan without a net: both structs are plain ints in the order documented there.
enum WideKernel {
  WK_NONE = 0, WK_XCD_FWD_F32, WK_XCD_FWD_BF16 /* <MT> */, WK_XCD_FWD_BF16_FX /* <NGX> */, WK_XCD_BWD_X3, WK_XCD_BWD_F32, WK_XCD_BWD_BF16_C32 /* <EPT, FULLK> */,
  WK_XCD_BWD_BF16 /* <MT> */, WK_FWD_STEP /* <MT> */, WK_FWD_STEP16_BF16, WK_BWD_STEP, WK_BWD_STEP16_BF16
};
struct WideShape {
  int fwd, no, x_ni, ndir, bs, tmax, N;   // the pass, the layer (x_ni: its inputs), the minibatch (N frames)
  int kp, kp16;                           // padded contraction lengths of this pass: f32 rows (Layer::kpf / kpb), bf16 rows (kp16f / kp16b)
  int bf16;                               // bf16 MFMA operands in the recurrence (precision mode 2)
  int x3;                                 // backward, exact-f32 mode: the x3 kernel is asked for (Net::rec_x3) and R2b holds the current weights
  int fx_mode;                            // forward: option fuse_wx where the operands of the folded input projection exist, else 0
  int ncu, xcd_on, xcd_failed, c32_on;    // CUs of the device, CLSTM_XCD_REC, g_xcd_failed, option bwd_c32
  int sbf, sbf_ld, lds, ldh;              // what the 32-bit offsets of the persistent bf16 kernels must cover: the bf16 source rows (sbf: written by
                                          // this pass -- the f32 h_{t-1} columns of S are then skipped: Net::wide_args), the f32 source and output rows
};
struct WidePlan {
  int kernel, param, fullk;               // the persistent kernel to try (WK_NONE: none applies) and its template parameter MT / NGX / EPT
  int nzb, zb_per, launches, lds_bytes;   // its line blocks, how many of them one launch walks, hence the launches; dynamic LDS
  int step_kernel, step_param;            // the per-step kernel that runs if none applies or chunk 0 failed its placement check (WK_NONE behind
  int step_grid[3];                       // WK_XCD_FWD_BF16_FX: the caller runs the hoisted product first and asks again without fx) and its grid
  int moves;                              // bit c: a successful persistent pass moves path counter c
  int fx_ngx;                             // the folded input projection was ASKED for (fuse_wx and the input width admit it): its NGX, else 0
};
static WidePlan wide_plan(const WideShape& h) {
  WidePlan p{};
  const bool fwd = h.fwd != 0, bf16 = h.bf16 != 0;
  const int no = h.no, ntile = (no + 15) / 16, nzb16 = (h.bs + 15) / 16;
  // persistent bf16 kernels: 32-line groups (two 16-line MFMA tiles per workgroup) once 16-line groups would need more than
  // one launch of 8 groups -- a step's barrier and ring round trip are then paid once for twice the lines
  const int mt = !bf16 ? 1 : nzb16 * h.ndir > 16 ? 4 : nzb16 * h.ndir > 8 ? 2 : 1;
  // the fallback, and the rule where no persistent kernel applies: one launch per time step
  if (fwd && !bf16) {
    const int mts = h.bs > 32 ? 4 : h.bs > 16 ? 2 : 1;
    p.step_kernel = WK_FWD_STEP; p.step_param = mts;
    p.step_grid[0] = (no + 3) / 4; p.step_grid[1] = h.ndir; p.step_grid[2] = (h.bs + 16 * mts - 1) / (16 * mts);
  } else if (!bf16) {
    p.step_kernel = WK_BWD_STEP;
    p.step_grid[0] = ntile; p.step_grid[1] = h.ndir; p.step_grid[2] = nzb16;
  } else {
    p.step_kernel = fwd ? WK_FWD_STEP16_BF16 : WK_BWD_STEP16_BF16;
    p.step_grid[0] = ntile * h.ndir * nzb16; p.step_grid[1] = p.step_grid[2] = 1;
  }
  // ONE launch per pass, a workgroup group per XCD with its weight rows resident in LDS (lstm_xcd_*: the default); minibatches of
  // more than 8 / ndir line blocks: one launch per chunk of line blocks.  CLSTM_XCD_REC=0 selects the per-step launches.
  // (The persistent bf16 kernels address their per-frame arrays through 32-bit buffer offsets: G / C / D / Dbf are covered by
  // Net::wide_args' check, the bf16 and f32 source rows -- ndir x N x (ni + no + 8) halfs / (1 + ni + no) floats -- and the output rows
  // must stay below 2 GiB too, or the per-step launches run)
  const double lim = 2147483000.0;
  const bool off32 = !bf16 || ((!h.sbf || (double)h.ndir * h.N * h.sbf_ld * 2 < lim) && (h.sbf || (double)h.ndir * h.N * h.lds * 4 < lim) && (double)h.N * h.ldh * 4 < lim);
  const bool fits = h.xcd_on && !h.xcd_failed && off32 && h.tmax > 1 && ntile <= 32 && 8 * ntile <= std::max(h.ncu, 16);
  p.nzb = (h.bs + 16 * mt - 1) / (16 * mt);
  p.zb_per = std::max(1, 8 / h.ndir);
  // The input projection folded into the persistent bf16 forward kernel (lstm_xcd_fwd_bf16_fx; measurements: Net::forward_pass).  fuse_wx:
  // 0 never, 1 (default) layers of up to 128 inputs, 2 every eligible layer; whole 32-k groups of inputs, NGX x 128 of them at most.
  // ONLY that kernel is planned then: where it does not apply, kernel names what runs behind the hoisted product.
  if (fwd && h.fx_mode > 0 && (h.fx_mode > 1 || h.x_ni <= 128) && (h.x_ni & 31) == 0)
    p.fx_ngx = h.x_ni <= 128 ? 1 : h.x_ni <= 512 ? 4 : h.x_ni <= 1024 ? 8 : 0;
  auto take = [&](int kernel, int param, int lds_bytes, int moves = 0) { p.kernel = kernel; p.param = param; p.lds_bytes = lds_bytes; p.moves = moves; };
  if (fits && p.fx_ngx && bf16 && mt == 1 && h.kp16 <= 512 && (no & 3) == 0 && h.x_ni <= 128 * p.fx_ngx && h.x_ni <= 2048) {
    take(WK_XCD_FWD_BF16_FX, p.fx_ngx, xcd_fwd_lds_bytes(1), 1 << PC_FWD_FUSED_WX);
    p.step_kernel = WK_NONE;
  } else if (fits && fwd) {
    if (!bf16 && xcd_fwd_f32_lds_bytes(h.kp) <= 160 * 1024) take(WK_XCD_FWD_F32, 0, xcd_fwd_f32_lds_bytes(h.kp));
    else if (bf16 && h.kp16 <= 512) take(WK_XCD_FWD_BF16, mt, xcd_fwd_lds_bytes(mt));
  } else if (fits && !bf16) {   // (an x3 pass whose placement failed does not try the f32 kernel: one persistent kernel per plan)
    if (h.x3 && h.kp16 <= 2048) take(WK_XCD_BWD_X3, 0, xcd_bwd_lds_bytes(1), 1 << PC_BWD_X3);
    else if (xcd_bwd_f32_lds_bytes(h.kp) <= 160 * 1024) take(WK_XCD_BWD_F32, 0, xcd_bwd_f32_lds_bytes(h.kp));
  } else if (fits && h.kp16 <= 2048) {
    // 32 cells per workgroup, two groups per XCD, groups of 8 / 16 / 32 lines (lstm_wide.h:lstm_xcd_bwd_bf16_c32): half the
    // delta block per step and CU of the 16-cell kernel, which stays for hidden sizes that are not multiples of 32
    if (h.c32_on && no % 32 == 0 && h.ndir <= 2) {
      p.zb_per = 16 / h.ndir;   // line groups per launch
      const int ept = h.bs <= 8 * p.zb_per ? 1 : h.bs <= 16 * p.zb_per ? 2 : 4;
      take(WK_XCD_BWD_BF16_C32, ept, xcd_bwd_c32_lds_bytes(ept), 1 << PC_BWD_C32);
      p.fullk = h.kp16 == 2048;
      p.nzb = (h.bs + 8 * ept - 1) / (8 * ept);
    } else take(WK_XCD_BWD_BF16, mt, xcd_bwd_lds_bytes(mt));
  }
  if (p.kernel != WK_NONE) {
    p.moves |= 1 << (fwd ? PC_FWD_PERSISTENT : PC_BWD_PERSISTENT);
    p.launches = (p.nzb + p.zb_per - 1) / p.zb_per;
  } else p.launches = h.tmax;
  return p;
}
// every instantiation of the lock-step kernels: the ONE place that names them (in the order of their first use so far: the
// order of the instantiations in the code object)
using WideFn = void (*)(LstmWideArgs);
static WideFn wide_kernel_fn(int kernel, int param, int fullk) {
  static const struct { int kernel, param, fullk; WideFn fn; } table[] = {
      {WK_XCD_FWD_BF16_FX, 1, 0, lstm_xcd_fwd_bf16_fx<1>}, {WK_XCD_FWD_BF16_FX, 4, 0, lstm_xcd_fwd_bf16_fx<4>}, {WK_XCD_FWD_BF16_FX, 8, 0, lstm_xcd_fwd_bf16_fx<8>},
      {WK_XCD_FWD_F32, 0, 0, lstm_xcd_fwd_f32},
      {WK_XCD_FWD_BF16, 4, 0, lstm_xcd_fwd_bf16<4>}, {WK_XCD_FWD_BF16, 2, 0, lstm_xcd_fwd_bf16<2>}, {WK_XCD_FWD_BF16, 1, 0, lstm_xcd_fwd_bf16<1>},
      {WK_FWD_STEP16_BF16, 0, 0, lstm_wide_fwd_step16_bf16},
      {WK_FWD_STEP, 4, 0, lstm_wide_fwd_step<4>}, {WK_FWD_STEP, 2, 0, lstm_wide_fwd_step<2>}, {WK_FWD_STEP, 1, 0, lstm_wide_fwd_step<1>},
      {WK_XCD_BWD_X3, 0, 0, lstm_xcd_bwd_x3}, {WK_XCD_BWD_F32, 0, 0, lstm_xcd_bwd_f32},
      {WK_XCD_BWD_BF16_C32, 1, 1, lstm_xcd_bwd_bf16_c32<1, true>}, {WK_XCD_BWD_BF16_C32, 1, 0, lstm_xcd_bwd_bf16_c32<1, false>},
      {WK_XCD_BWD_BF16_C32, 2, 1, lstm_xcd_bwd_bf16_c32<2, true>}, {WK_XCD_BWD_BF16_C32, 2, 0, lstm_xcd_bwd_bf16_c32<2, false>},
      {WK_XCD_BWD_BF16_C32, 4, 1, lstm_xcd_bwd_bf16_c32<4, true>}, {WK_XCD_BWD_BF16_C32, 4, 0, lstm_xcd_bwd_bf16_c32<4, false>},
      {WK_XCD_BWD_BF16, 4, 0, lstm_xcd_bwd_bf16<4>}, {WK_XCD_BWD_BF16, 2, 0, lstm_xcd_bwd_bf16<2>}, {WK_XCD_BWD_BF16, 1, 0, lstm_xcd_bwd_bf16<1>},
      {WK_BWD_STEP16_BF16, 0, 0, lstm_wide_bwd_step16_bf16}, {WK_BWD_STEP, 0, 0, lstm_wide_bwd_step}};
  for (const auto& e : table)
    if (e.kernel == kernel && e.param == param && e.fullk == fullk) return e.fn;
  throw Error("internal: no lock-step kernel for this plan");
}
// The sync words of the persistent kernels and where the group-barrier stamps of the buffer's next launch start.  (The counter words are
// zero: DevBuf zero-fills, and every persistent launch returns them to zero as its last act; the stamps keep counting up: lstm_wide.h:xcd_finish)
struct XcdSync {
  DevBuf<int> words;
  int base = 0;
  int* reserve() { words.reserve(XcdSyncLayout::WORDS); return words.p; }
  int take_stamps(int tmax, hipStream_t s) {
    if (base > (1 << 30)) {   // (once per ~2 million launches)
      HIPCHECK(hipMemsetAsync(words.p, 0, XcdSyncLayout::WORDS * sizeof(int), s));
      base = 0;
    }
    const int b = base;
    base += tmax + 2;
    return b;
  }
};
// the persistent kernel of the plan over its chunks of line blocks; false: chunk 0 failed its placement check and nothing was written
static bool launch_wide_persistent(const WidePlan& p, LstmWideArgs& a, XcdSync& sync, hipStream_t s) {
  const WideFn kernel = wide_kernel_fn(p.kernel, p.param, p.fullk);
  const int ntile = (a.no + 15) / 16;
  bool ok = true;
  for (int zb0 = 0; zb0 < p.nzb && ok; zb0 += p.zb_per) {
    a.zb0 = zb0; a.zbn = std::min(p.zb_per, p.nzb - zb0);
    a.debug_fail_claim = g_debug_fail_skip > 0 ? (g_debug_fail_skip--, 0) : g_debug_fail_claims > 0 ? (g_debug_fail_claims--, 1) : 0;
    a.stamp_base = sync.take_stamps(a.tmax, s);
    a.out_sticky = dev_err_words();
    a.out_host = g_xcd_outcome.prepare();
    allow_dynamic_lds((const void*)kernel, (size_t)p.lds_bytes);
    // An ORDINARY launch: one workgroup per CU (LDS), at most as many workgroups as CUs, the stream's previous kernel complete --
    // they are all resident, and if they ever were not, the placement check of xcd_claim times out with error 1 before anything
    // has been written.  The first four launches of a process are checked synchronously and the per-step path redoes such a pass;
    // a later failure is found asynchronously (XcdOutcome): the updates since then are skipped on the device, the host reports it
    // at its next check and uses the per-step launches from then on.  hipLaunchCooperativeKernel cost ~20 us of gaps around every
    // one of the four launches of a configs[4] step.  (The host emulator needs its "all workgroups live" launch.)
#ifdef CLSTM_HIP_EMU
    CLSTM_LAUNCH_COOP(kernel, dim3(8 * ntile), dim3(WIDE_THREADS), (size_t)p.lds_bytes, s, a);
#else
    CLSTM_LAUNCH(kernel, dim3(8 * ntile), dim3(WIDE_THREADS), (size_t)p.lds_bytes, s, a);
#endif
    check_launch();
    ok = g_xcd_outcome.after_launch(sync.words.p + XcdSyncLayout::LAST_ERROR, s);
    REQUIRE(ok || zb0 == 0, "persistent recurrence: placement failed after the first chunk had run; set CLSTM_XCD_REC=0");
  }
  if (!ok) g_xcd_failed = true;
  return ok;
}
// ... and its per-step kernel, one launch per time step (a replayed graph from 8 steps on: launch_steps)
static void launch_wide_steps(const WidePlan& p, const LstmWideArgs& a, StepGraphCache& graphs, hipStream_t s) {
  const WideFn kernel = wide_kernel_fn(p.step_kernel, p.step_param, 0);
  const int kind = p.step_kernel == WK_FWD_STEP ? 0 : p.step_kernel == WK_BWD_STEP ? 1 : p.step_kernel == WK_FWD_STEP16_BF16 ? 2 : 3;
  const dim3 grid(p.step_grid[0], p.step_grid[1], p.step_grid[2]);
  launch_steps(graphs, kind, a, a.tmax, s, [&]() {
    LstmWideArgs w = a;
    for (int t = 0; t < a.tmax; t++) {
      w.step = t;
      CLSTM_LAUNCH(kernel, grid, dim3(WIDE_THREADS), 0, s, w);
    }
  });
  check_launch();
}
// What launch_lstm_wide ran.  The persistent kernel is tried first; a placement failure in chunk 0 (nothing written) falls back to the
// per-step launches, a later one is fatal.  Nothing: the plan was the fx kernel alone and it failed its placement check.
enum class WideRan { Nothing, Steps, Persistent };
static WideRan launch_lstm_wide(const WidePlan& p, LstmWideArgs a, XcdSync& sync, StepGraphCache& graphs, hipStream_t s) {
  if (p.kernel != WK_NONE && launch_wide_persistent(p, a, sync, s)) {
    count_moves(p.moves);
    return WideRan::Persistent;
  }
  if (p.step_kernel == WK_NONE) return WideRan::Nothing;
  launch_wide_steps(p, a, graphs, s);
  return WideRan::Steps;
}
// diagnostics (CLSTM_FW_TRACE / CLSTM_DW_TRACE): the stamp rows a launch left on the device, four per line, under the caller's header
template <class... A>
static void dump_trace(const char* path, const long long* rows_d, size_t rows, hipStream_t s, const char* header_fmt, A... header_args) {
  HIPCHECK(hipStreamSynchronize(s));
  std::vector<long long> t(rows * 4);
  HIPCHECK(hipMemcpy(t.data(), rows_d, t.size() * sizeof(long long), hipMemcpyDeviceToHost));
  FILE* f = fopen(path, "w");
  if (!f) return;
  fprintf(f, header_fmt, header_args...);
  for (size_t i = 0; i < rows; i++) fprintf(f, "%lld %lld %lld %lld\n", t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
  fclose(f);
}

// ---- per-kernel device timing (bench.py roofline) ---------------------------------------------
#ifndef CLSTM_HIP_EMU
struct Timing {
  bool on = false;
  struct Rec { std::string name; std::vector<ClstmLaunchEvents> launches; };
  std::vector<Rec> pending;
  std::map<std::string, std::pair<double, int>> acc;
  // a bracket names the launches issued inside it; each launch brings its own pair of events (devintrin.h, CLSTM_LAUNCH)
  void begin(const char* name, hipStream_t) {
    if (!on) return;
    pending.emplace_back();
    pending.back().name = name;
    clstm_launch_sink = &pending.back().launches;
  }
  void end(hipStream_t) {
    if (!on) return;
    clstm_launch_sink = nullptr;
  }
  void collect(hipStream_t s) {
    clstm_launch_sink = nullptr;
    if (pending.empty()) return;
    HIPCHECK(hipStreamSynchronize(s));
    for (auto& r : pending) {
      double sum = 0;
      for (auto& e : r.launches) {
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, e.a, e.b));
        sum += ms;
        clstm_event_pool.push_back(e);
      }
      if (r.launches.empty()) continue;      // (a bracket around graph replays or copies only: nothing to report)
      auto& a = acc[r.name];
      a.first += sum; a.second += 1;
    }
    pending.clear();
  }
};
#else
struct Timing {
  bool on = false;
  std::map<std::string, std::pair<double, int>> acc;
  void begin(const char*, hipStream_t) {}
  void end(hipStream_t) {}
  void collect(hipStream_t) {}
};
#endif

// ---- roctx ranges (SURVEY 5: a rocprofv3 --marker-trace of a drop-in run should read ingest / forward / ctc / backward /
// allreduce / update) ----------------------------------------------------------------------------------------------------
// librocprofiler-sdk-roctx is bound at first use like RCCL; ranges are emitted when a profiler tool is attached to the
// process (rocprofv3 exports ROCP_TOOL_LIBRARIES) or CLSTM_ROCTX=1 asks for them; CLSTM_ROCTX=0 switches them off.
#ifndef CLSTM_HIP_EMU
}  // namespace clstm
#include <dlfcn.h>
namespace clstm {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  static Roctx& get() {
    static Roctx r = [] {
      Roctx x;
      const char* e = getenv("CLSTM_ROCTX");
      const bool want = e ? atoi(e) != 0 : getenv("ROCP_TOOL_LIBRARIES") != nullptr;
      if (!want) return x;
      void* h = nullptr;
      for (const char* name : {"librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1", "libroctx64.so.4", "libroctx64.so"})
        if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
      if (!h) return x;
      x.push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      x.pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!x.push || !x.pop) x.push = nullptr;
      return x;
    }();
    return r;
  }
};
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char* name) : on(Roctx::get().push != nullptr) { if (on) Roctx::get().push(name); }
  ~RoctxRange() { if (on) Roctx::get().pop(); }
};
#else
struct RoctxRange { explicit RoctxRange(const char*) {} };
#endif

#include "comm.h"   // the gradient exchange: communicator, peer-read all-reduce, replica check buffers

