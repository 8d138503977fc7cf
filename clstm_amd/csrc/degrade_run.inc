// degrade_run.inc -- part of clstm_hip.hip (namespace clstm): host side of the device line degrader (degrade.h): the checks, the masks, the
// item lists and the launches of one clstm_degrader_run_* call, and clstm_degrade_draw's generator.  Everything goes to the library's
// one stream (g_stream); nothing is read back: run() enqueues and returns.

struct Degrader {
  // grow-only device buffers, constructed inside an AcctScope (clstm_degrader_create): clstm_degrader_device_bytes sums them.
  // fcol / fld: the two fields of every distorted line after the column pass / smoothed; partial, bounds: the min / max stages;
  // out: the result; tmp: the blur's column pass; pix: the uploaded pixels of run_h
  DevBuf<float> pix, fcol, fld, partial, bounds, out, tmp;
  StagedBlock meta;   // [image lines | field lines | blur lines | warps | fields | items | masks]: one copy per call
  ~Degrader() {
    for (DevBuf<float>* b : {&pix, &fcol, &fld, &partial, &bounds, &out, &tmp}) b->release();
    meta.dev.release();
  }
  NzMasks pool;       // the masks of ONE call (the sigmas are drawn afresh for every line and visit: a pool kept across calls would only grow)
  std::vector<NzLine> img_h, fld_h, blur_h;
  std::vector<DgWarp> warps_h;
  std::vector<DgField> fields_h;
  std::vector<NzItem> items_h;
  size_t last_pixels = 0;   // floats of the last successful call's output (0: none)

  enum Stage { NOISE_COLS = 0, NOISE_ROWS, MINMAX, BOUNDS, WARP, BLUR_COLS, BLUR_ROWS, NSTAGES };
  static constexpr int MAX_SIDE = 1 << 23;   // (i - cx) + cx must give i back exactly in float (host/degrade.h)

  static bool reach_ok(float s) { return 3.0 * s < 1e6 && NzMasks::reach(s) <= NZ_MAXRANGE; }
  static std::string reach_text(const char* what, int b, float s) {
    return "clstm_degrader_run: line " + std::to_string(b) + ": the Gaussian mask of " + what + " = " + std::to_string(s) + " would reach " +
           std::to_string(3.0 * s < 1e6 ? NzMasks::reach(s) : -1) + " pixels; the limit is NZ_MAXRANGE = " + std::to_string(NZ_MAXRANGE) + " (1 + int(3 sigma))";
  }
  void add_row_items(int line, int stage, int w, int h) {   // the 64 x 8 tiles of k_nz_filter_rows
    for (int jb = 0; jb * NZ_ROW_TJ < h; jb++)
      for (int i0 = 0; i0 < w; i0 += NZ_ROW_TI) items_h.push_back(NzItem{line, stage, jb * w + i0, std::min(NZ_ROW_TI, w - i0)});
  }
  void add_items(int line, int stage, int total, int per) {
    for (int f = 0; f < total; f += per) items_h.push_back(NzItem{line, stage, f, std::min(per, total - f)});
  }

  void run(const float* pixels, bool pix_host, const int* w_h, const int* h_h, int bs, const clstm_degrade_line* p, float** out_d) {
    REQUIRE(pixels && w_h && h_h && p && out_d, "null argument");
    REQUIRE(bs > 0, "clstm_degrader_run: bs must be positive");
    // ---- validation, before anything is touched
    long long npix = 0, nfld = 0;
    for (int b = 0; b < bs; b++) {
      const std::string line = "clstm_degrader_run: line " + std::to_string(b);
      REQUIRE(w_h[b] >= 1 && h_h[b] >= 1, line + " has width " + std::to_string(w_h[b]) + ", height " + std::to_string(h_h[b]) + " (both must be at least 1)");
      REQUIRE((long long)w_h[b] * h_h[b] <= (1LL << 30), line + " has more than 2^30 pixels");
      REQUIRE(w_h[b] <= MAX_SIDE && h_h[b] <= MAX_SIDE, line + " has a side above 2^23 pixels");
      const clstm_degrade_line& q = p[b];
      REQUIRE(std::isfinite(q.m[0]) && std::isfinite(q.m[1]) && std::isfinite(q.m[2]) && std::isfinite(q.m[3]) && std::isfinite(q.tx) && std::isfinite(q.ty),
              line + ": m, tx and ty must be finite");
      REQUIRE(std::isfinite(q.maxdelta) && q.maxdelta >= 0.0f, line + ": maxdelta must be finite and not negative");
      REQUIRE(std::isfinite(q.sigma), line + ": sigma must be finite");
      REQUIRE(std::isfinite(q.blur) && q.blur >= 0.0f, line + ": blur must be finite and not negative");
      if (q.maxdelta > 0.0f) {
        REQUIRE(q.sigma > 0.0f, line + ": sigma must be positive where maxdelta > 0");
        REQUIRE(reach_ok(q.sigma), reach_text("sigma", b, q.sigma));
        nfld += 2LL * w_h[b] * h_h[b];
      }
      if (q.blur > 0.0f) REQUIRE(reach_ok(q.blur), reach_text("blur", b, q.blur));
      npix += (long long)w_h[b] * h_h[b];
    }
    last_pixels = 0;
    // ---- line descriptors, masks, items
    pool.mask_pool.clear();
    pool.mask_of.clear();
    img_h.clear(); fld_h.clear(); blur_h.clear(); warps_h.clear(); fields_h.clear(); items_h.clear();
    long long po = 0, fo = 0;
    for (int b = 0; b < bs; b++) {
      const clstm_degrade_line& q = p[b];
      NzLine L{};
      L.w = w_h[b]; L.h = h_h[b]; L.pix = po;
      DgWarp W{};
      W.fld = fo; W.bound = -1;
      for (int k = 0; k < 4; k++) W.m[k] = q.m[k];
      W.tx = q.tx; W.ty = q.ty; W.maxdelta = q.maxdelta;
      if (q.maxdelta > 0.0f) {
        W.bound = (int)fld_h.size();
        const auto e = pool.mask(q.sigma);
        // (dg_seed_key of host/degrade.h, computed once per line)
        unsigned key = q.seed ^ 0x9e3779b9U;
        key ^= key >> 16; key *= 0x7feb352dU; key ^= key >> 15; key *= 0x846ca68bU; key ^= key >> 16;
        for (unsigned f = 0; f < 2; f++) {
          NzLine F = L;
          F.pix = fo;
          F.mask[0] = F.mask[1] = e.first; F.range[0] = F.range[1] = e.second;
          fld_h.push_back(F);
          fields_h.push_back(DgField{key, f});
          fo += (long long)L.w * L.h;
        }
      }
      NzLine B = L;   // (an entry for every line keeps the blur items' line numbers those of the call; without blur it has no items)
      if (q.blur > 0.0f) {
        const auto e = pool.mask(q.blur);
        B.mask[0] = B.mask[1] = e.first; B.range[0] = B.range[1] = e.second;
      }
      blur_h.push_back(B);
      img_h.push_back(L);
      warps_h.push_back(W);
      po += (long long)L.w * L.h;
    }
    int reach_noise = 0, reach_blur = 0;
    size_t stage_at[NSTAGES + 1];
    int npartial = 0;
    for (int stage = 0; stage < NSTAGES; stage++) {
      stage_at[stage] = items_h.size();
      if (stage <= BOUNDS) {
        for (int k = 0; k < (int)fld_h.size(); k++) {
          const NzLine& F = fld_h[k];
          if (stage == NOISE_COLS) add_items(k, stage, F.w * F.h, NZ_THREADS);
          else if (stage == NOISE_ROWS) { add_row_items(k, stage, F.w, F.h); reach_noise = std::max(reach_noise, F.range[1]); }
          else if (stage == MINMAX) add_items(k, stage, F.w * F.h, DG_MM_CHUNK);
          else {   // the field's partials are the items MINMAX has just listed for it, in order
            const int n = (F.w * F.h + DG_MM_CHUNK - 1) / DG_MM_CHUNK;
            items_h.push_back(NzItem{k, stage, npartial, n});
            npartial += n;
          }
        }
      } else
        for (int b = 0; b < bs; b++) {
          const NzLine& L = img_h[b];
          if (stage == WARP) add_items(b, stage, L.w * L.h, NZ_THREADS);
          else if (p[b].blur > 0.0f) {
            if (stage == BLUR_COLS) add_items(b, stage, L.w * L.h, NZ_THREADS);
            else { add_row_items(b, stage, L.w, L.h); reach_blur = std::max(reach_blur, blur_h[b].range[1]); }
          }
        }
    }
    stage_at[NSTAGES] = items_h.size();
    // ---- buffers; the per-call arrays go up as one staged block (records with 8-byte members first)
    out.reserve((size_t)npix);
    if (nfld) {
      fcol.reserve((size_t)nfld);
      fld.reserve((size_t)nfld);
      partial.reserve(2 * (size_t)npartial);
      bounds.reserve(2 * fld_h.size());
    }
    if (stage_at[BLUR_ROWS + 1] > stage_at[BLUR_COLS]) tmp.reserve((size_t)npix);
    const float* px = pixels;
    if (pix_host) {
      pix.reserve((size_t)npix);
      HIPCHECK(hipMemcpyAsync(pix.p, pixels, (size_t)npix * sizeof(float), hipMemcpyHostToDevice, g_stream));
      px = pix.p;
    }
    meta.begin((img_h.size() + fld_h.size() + blur_h.size()) * sizeof(NzLine) + warps_h.size() * sizeof(DgWarp) + fields_h.size() * sizeof(DgField) +
               items_h.size() * sizeof(NzItem) + pool.mask_pool.size() * sizeof(float));
    const NzLine* img_d = meta.put(img_h);
    const NzLine* fld_d = meta.put(fld_h);
    const NzLine* blur_d = meta.put(blur_h);
    const DgWarp* warps_d = meta.put(warps_h);
    const DgField* fields_d = meta.put(fields_h);
    const NzItem* items_d = meta.put(items_h);
    const float* masks_d = meta.put(pool.mask_pool);
    meta.send(g_stream);
    // ---- the launches
    const dim3 blk(NZ_THREADS);
    auto stage = [&](int s, auto&& go) {
      const unsigned n = (unsigned)(stage_at[s + 1] - stage_at[s]);
      if (n) { go(items_d + stage_at[s], n); check_launch(); }
    };
    stage(NOISE_COLS, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_dg_noise_cols, dim3(n), blk, 0, g_stream, it, fld_d, fields_d, fcol.p, masks_d); });
    stage(NOISE_ROWS, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_filter_rows, dim3(n), blk, nz_rows_smem(reach_noise), g_stream, it, fld_d, (const float*)fcol.p, fld.p, masks_d); });
    stage(MINMAX, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_dg_minmax, dim3(n), blk, 0, g_stream, it, fld_d, (const float*)fld.p, partial.p); });
    stage(BOUNDS, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_dg_bounds, dim3(n), blk, 0, g_stream, it, (const float*)partial.p, bounds.p); });
    stage(WARP, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_dg_warp, dim3(n), blk, 0, g_stream, it, img_d, warps_d, px, (const float*)fld.p, (const float*)bounds.p, out.p); });
    stage(BLUR_COLS, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_filter_run, dim3(n), blk, 0, g_stream, it, blur_d, (const float*)out.p, tmp.p, masks_d, 0); });
    stage(BLUR_ROWS, [&](const NzItem* it, unsigned n) { CLSTM_LAUNCH(k_nz_filter_rows, dim3(n), blk, nz_rows_smem(reach_blur), g_stream, it, blur_d, (const float*)tmp.p, out.p, masks_d); });
    last_pixels = (size_t)npix;
    *out_d = out.p;
    g_path_count[PC_DEGRADED] += bs;
  }
};

// ---- clstm_degrade_draw: the one statement of how a line's parameters are drawn.  Counter-based: splitmix64's finaliser (Steele, Lea, Flood
// 2014; public domain) chained over seed, key, visit gives the line's stream; its k-th value is the finaliser of stream + (k + 1) golden-ratio
// increments, the top 53 bits a double in [0, 1).  Values k, in this order: 0 angle, 1 log-scale, 2 anisotropy, 3 tx, 4 ty, 5 sigma, 6 maxdelta,
// 7 blur, 8 the seed of the noise fields.
static unsigned long long dg_splitmix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
static clstm_degrade_ranges degrade_default_ranges() {
  clstm_degrade_ranges r{};
  r.angle = 0.02f; r.scale = 0.03f; r.aniso = 0.02f; r.translate = 0.03f;
  r.sigma[0] = 3.0f; r.sigma[1] = 8.0f;
  r.maxdelta[0] = 0.0f; r.maxdelta[1] = 1.5f;
  r.blur[0] = 0.0f; r.blur[1] = 0.7f;
  return r;
}
static void degrade_draw(unsigned long long seed, unsigned long long key, unsigned long long visit, const clstm_degrade_ranges& rg, int w, int h,
                         clstm_degrade_line* out) {
#pragma clang fp contract(off)
  (void)w;
  const unsigned long long stream = dg_splitmix(dg_splitmix(dg_splitmix(seed) ^ key) ^ visit);
  auto bits = [&](int k) { return dg_splitmix(stream + (unsigned long long)(k + 1) * 0x9e3779b97f4a7c15ULL); };
  auto u = [&](int k) { return (double)(bits(k) >> 11) * 0x1p-53; };
  auto sym = [&](int k, double a) { return -a + (2.0 * a) * u(k); };                       // uniform in [-a, a)
  auto within = [&](int k, const float* iv) { return (double)iv[0] + ((double)iv[1] - (double)iv[0]) * u(k); };
  const double angle = sym(0, rg.angle), ls = sym(1, rg.scale), an = sym(2, rg.aniso);
  const double sx = exp(ls + an), sy = exp(ls - an), c = cos(angle), s = sin(angle);
  // the map from an output pixel to its source, about the centre of the line: a rotation by `angle` of the scaled axes
  out->m[0] = (float)(c * sx); out->m[1] = (float)(0.0 - s * sy);
  out->m[2] = (float)(s * sx); out->m[3] = (float)(c * sy);
  const double t = (double)rg.translate * h;
  out->tx = (float)sym(3, t); out->ty = (float)sym(4, t);
  out->sigma = (float)within(5, rg.sigma);
  out->maxdelta = (float)within(6, rg.maxdelta);
  out->blur = (float)within(7, rg.blur);
  out->seed = (unsigned)(bits(8) >> 32);
}
