// normalize_run.inc -- part of clstm_hip.hip (namespace clstm): host side of the device line normaliser (normalize.h): the Gaussian
// masks, the item lists, the launches of one clstm_normalizer_run_* call.  Everything goes to the library's one stream (g_stream).

// The mask pool of a normaliser or of one degrader call (degrade_run.inc): gauss1d's mask of every sigma seen so far, computed on the
// host -- the device never evaluates exp -- and cached by the bits of sigma
struct NzMasks {
  std::vector<float> mask_pool;
  std::map<unsigned, std::pair<int, int>> mask_of;   // bits of sigma -> (offset, reach)
  static int reach(float sigma) { return 1 + int(3.0 * sigma); }   // gauss1d :29
  std::pair<int, int> mask(float sigma) {
    unsigned key;
    memcpy(&key, &sigma, 4);
    auto it = mask_of.find(key);
    if (it != mask_of.end()) return it->second;
    // gauss1d :33-42, expression for expression: double exp, float store, sequential float total, float divide
    const int rg = reach(sigma);
    std::vector<float> m(2 * rg + 1, 0.0f);
    for (int i = 0; i <= rg; i++) {
      double y = exp(-i * i / 2.0 / sigma / sigma);
      m[rg + i] = m[rg - i] = (float)y;
    }
    float total = 0.0f;
    for (float v : m) total += v;
    for (float& v : m) v /= total;
    const std::pair<int, int> e((int)mask_pool.size(), rg);
    mask_pool.insert(mask_pool.end(), m.begin(), m.end());
    while (mask_pool.size() & 3) mask_pool.push_back(0.0f);
    mask_of[key] = e;
    return e;
  }
};

struct Normalizer : NzMasks {
  int target_height = 48;
  float smooth2d = 1.0f, smooth1d = 0.3f, range = 4.0f;
  // grow-only device buffers, constructed inside an AcctScope (clstm_normalizer_create): clstm_normalizer_device_bytes sums them
  DevBuf<float> pix, tmp, smooth, amax, center, sums, masks, frames;
  DevBuf<NzLine> lines;
  DevBuf<NzItem> items;
  DevBuf<NzWarp> warps;
  ~Normalizer() {
    for (DevBuf<float>* b : {&pix, &tmp, &smooth, &amax, &center, &sums, &masks, &frames}) b->release();
    lines.release(); items.release(); warps.release();
  }
  size_t masks_uploaded = 0;   // floats of mask_pool the device copy holds (refreshed when the pool has grown)
  std::vector<NzLine> lines_h;
  std::vector<NzItem> items_h;
  std::vector<NzWarp> warps_h;
  std::vector<float> sums_h;
  size_t last_frames = 0;   // floats of the last successful call's frames (0: none)

  template <class T>
  static void upload(DevBuf<T>& d, const std::vector<T>& h) {
    d.reserve(h.size());
    HIPCHECK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, g_stream));
  }
  void add_items(int line, int stage, int total, int per) {
    for (int f = 0; f < total; f += per) items_h.push_back(NzItem{line, stage, f, std::min(per, total - f)});
  }
  template <class F>
  void launch_stage(int stage, F&& go) {   // the items of one stage are contiguous in the list
    size_t a = 0;
    while (a < items_h.size() && items_h[a].stage != stage) a++;
    size_t b = a;
    while (b < items_h.size() && items_h[b].stage == stage) b++;
    if (b > a) { go(items.p + a, (unsigned)(b - a)); check_launch(); }
  }

  void run(const float* pixels, bool pix_host, const int* w_h, const int* h_h, int bs, int* T_h, float* r_h, float** frames_d) {
#pragma clang fp contract(off)
    REQUIRE(pixels && w_h && h_h && T_h && frames_d, "null argument");
    REQUIRE(bs > 0, "clstm_normalizer_run: bs must be positive");
    // ---- validation, before anything is touched
    long long npix = 0, ncol = 0;
    for (int b = 0; b < bs; b++) {
      REQUIRE(w_h[b] >= 1 && h_h[b] >= 1, "clstm_normalizer_run: line " + std::to_string(b) + " has width " + std::to_string(w_h[b]) + ", height " +
              std::to_string(h_h[b]) + " (both must be at least 1)");
      REQUIRE((long long)w_h[b] * h_h[b] <= (1LL << 30), "clstm_normalizer_run: line " + std::to_string(b) + " has more than 2^30 pixels");
      const float sig[3] = {h_h[b] * 0.5f, h_h[b] * smooth2d, h_h[b] * smooth1d};
      for (float s : sig)
        REQUIRE(s > 0.0f && 3.0 * s < 1e6 && reach(s) <= NZ_MAXRANGE,
                "clstm_normalizer_run: line " + std::to_string(b) + " of height " + std::to_string(h_h[b]) + ": a Gaussian mask would reach " +
                std::to_string(3.0 * s < 1e6 ? reach(s) : -1) + " pixels; the limit is NZ_MAXRANGE = " + std::to_string(NZ_MAXRANGE) +
                " (1 + int(3 sigma) for the sigmas h/2, h*smooth2d, h*smooth1d; any h <= 256 at the default parameters)");
      npix += (long long)w_h[b] * h_h[b];
      ncol += w_h[b];
    }
    last_frames = 0;
    // ---- line descriptors, masks, items
    lines_h.clear();
    items_h.clear();
    long long po = 0, co = 0;
    for (int b = 0; b < bs; b++) {
      NzLine L{};
      L.w = w_h[b]; L.h = h_h[b]; L.pix = po; L.col = co;
      const float sig[3] = {L.h * 0.5f, L.h * smooth2d, L.h * smooth1d};
      for (int k = 0; k < 3; k++) { const auto e = mask(sig[k]); L.mask[k] = e.first; L.range[k] = e.second; }
      lines_h.push_back(L);
      po += (long long)L.w * L.h;
      co += L.w;
    }
    int max_row_reach = 0;
    for (int stage = 0; stage < 6; stage++)
      for (int b = 0; b < bs; b++) {
        const NzLine& L = lines_h[b];
        if (stage == 0) add_items(b, 0, L.w * L.h, NZ_THREADS);
        else if (stage == 1) {
          for (int jb = 0; jb * NZ_ROW_TJ < L.h; jb++)
            for (int i0 = 0; i0 < L.w; i0 += NZ_ROW_TI) items_h.push_back(NzItem{b, 1, jb * L.w + i0, std::min(NZ_ROW_TI, L.w - i0)});
          max_row_reach = std::max(max_row_reach, L.range[1]);
        } else if (stage == 2) add_items(b, 2, L.h, NZ_THREADS);
        else if (stage == 3 || stage == 4) add_items(b, stage, L.w, NZ_THREADS);
        else items_h.push_back(NzItem{b, 5, 0, L.w * L.h});
      }
    tmp.reserve((size_t)npix);
    smooth.reserve((size_t)npix);
    amax.reserve((size_t)ncol);
    center.reserve((size_t)ncol);
    sums.reserve(2 * (size_t)bs);
    const float* px = pixels;
    if (pix_host) {
      pix.reserve((size_t)npix);
      HIPCHECK(hipMemcpyAsync(pix.p, pixels, (size_t)npix * sizeof(float), hipMemcpyHostToDevice, g_stream));
      px = pix.p;
    }
    upload(lines, lines_h);
    upload(items, items_h);
    if (masks.cap < mask_pool.size()) masks_uploaded = 0;   // (reserve will reallocate: the whole pool goes up again)
    masks.reserve(mask_pool.size());
    if (masks_uploaded < mask_pool.size()) {
      HIPCHECK(hipMemcpyAsync(masks.p + masks_uploaded, mask_pool.data() + masks_uploaded, (mask_pool.size() - masks_uploaded) * sizeof(float),
                              hipMemcpyHostToDevice, g_stream));
      masks_uploaded = mask_pool.size();
    }
    // ---- measure
    const dim3 blk(NZ_THREADS);
    launch_stage(0, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_filter_run, dim3(n), blk, 0, g_stream, it, (const NzLine*)lines.p, px, tmp.p, (const float*)masks.p, 0); });
    launch_stage(1, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_filter_rows, dim3(n), blk, nz_rows_smem(max_row_reach), g_stream, it, (const NzLine*)lines.p, (const float*)tmp.p, smooth.p, (const float*)masks.p); });
    launch_stage(2, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_smear, dim3(n), blk, 0, g_stream, it, (const NzLine*)lines.p, px, smooth.p); });
    launch_stage(3, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_argmax, dim3(n), blk, 0, g_stream, it, (const NzLine*)lines.p, (const float*)smooth.p, amax.p); });
    launch_stage(4, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_filter_run, dim3(n), blk, 0, g_stream, it, (const NzLine*)lines.p, (const float*)amax.p, center.p, (const float*)masks.p, 2); });
    launch_stage(5, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_mad, dim3(n), blk, 0, g_stream, it, (const NzLine*)lines.p, px, (const float*)center.p, sums.p); });
    sums_h.resize(2 * (size_t)bs);
    HIPCHECK(hipMemcpyAsync(sums_h.data(), sums.p, sums_h.size() * sizeof(float), hipMemcpyDeviceToHost, g_stream));
    HIPCHECK(hipStreamSynchronize(g_stream));
    // ---- mad, r (measure :114-115) and the geometry of normalize (:120-121), on the host: bs values
    warps_h.clear();
    items_h.clear();
    long long fo = 0;
    for (int b = 0; b < bs; b++) {
      const float s1 = sums_h[2 * b], sy = sums_h[2 * b + 1];
      const float mad = sy / s1;
      REQUIRE(s1 != 0.0f && std::isfinite(mad), "clstm_normalizer_run: line " + std::to_string(b) + " cannot be measured (" +
              (s1 == 0.0f ? "no ink: the sum of its pixels is 0" : "its mean absolute deviation is not finite") + "); no frames were produced for this call");
      const float r = (float)int(range * mad + 1);
      const float scale = (float)((2.0 * r) / target_height);
      const int tw = std::max(int(lines_h[b].w / scale), 1);
      REQUIRE(scale > 0.0f && (long long)tw * target_height <= (1LL << 30), "clstm_normalizer_run: line " + std::to_string(b) + ": r = " + std::to_string(r) + " gives no usable scale");
      warps_h.push_back(NzWarp{scale, tw, fo});
      add_items(b, 6, tw * target_height, NZ_THREADS);
      sums_h[2 * b] = r;   // (kept for the outputs below: nothing is written while a later line may still be refused)
      fo += (long long)tw * target_height;
    }
    frames.reserve((size_t)fo);
    upload(warps, warps_h);
    upload(items, items_h);
    launch_stage(6, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_warp, dim3(n), blk, 0, g_stream, it, (const NzLine*)lines.p, (const NzWarp*)warps.p, px, (const float*)center.p, frames.p, target_height); });
    for (int b = 0; b < bs; b++) {
      T_h[b] = warps_h[b].T;
      if (r_h) r_h[b] = sums_h[2 * b];
    }
    last_frames = (size_t)fo;
    *frames_d = frames.p;
    g_path_count[PC_NORMALIZED] += bs;
  }
};
