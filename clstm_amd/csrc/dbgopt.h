// dbgopt.h -- the library's EXPERIMENT switches: paths that tests compare against bit for bit, and real fallbacks, selectable
// within one process.  None is a product setting (DESIGN.md 9 lists those: a dozen environment variables).  An option is set by
// the tests through clstm_debug_set_option(name, value) -- they compare two kernels bit for bit within one process -- or, for A/B
// runs of a whole program, through ONE environment variable read when the library first reads an option:
//     CLSTM_DEBUG="gemm_stag=1,bwd_c32=0"
// A name the table below does not hold is an error in both (EXPERIMENTS.md lists the retired ones).
#pragma once
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>

namespace clstm {
struct DbgOptDef { const char* name; int dflt; };
inline constexpr DbgOptDef DBG_OPTS[] = {
    {"gemm_stag", 2},        // operand tiles of the bf16-source GEMMs: 2 LDS-DMA + staggered wave groups, 1 register-staged +
                             //   staggered, 0 the one-barrier loop of round 4
    {"bwd_c32", 1},          // 0: the 16-cell persistent backward kernel
    {"rec_x3", 1},           // 0: the exact-f32 persistent backward recurrence on the f32 MFMA
    {"pack_tiles", 1},       // 0: the five single-purpose repack kernels
    {"fuse_wx", 1},          // input projection of layers of <= 128 inputs inside the persistent forward kernel; 0 never,
                             //   2 every eligible layer
    {"gemm_b16mc", 1},       // 0: weight gradient of wide layers from f32 source rows
    {"dw_x3", 1},            // 0: the f32 MFMA for the fused launch's weight-gradient items ...
    {"gemm_x3", 1},          // 0: ... / for the softmax layer's backward pair (what clstm_net_set_strict_f32 selects per net)
    {"split_terms", 3},      // 2: two-term split of the backward products
    {"xd_prologue", 2},      // the softmax layer's x.d: 2 the recurrence workgroups of the top layer's fused backward launch compute
                             //   only the 32 frames they visit first, helper items of the launch the rest (where narrow_plan
                             //   admits it, else as 1); 1 every recurrence workgroup computes its whole slice in front of its
                             //   first step; 0 a launch of its own in front of the backward launch
    {"fwd_mfma", 1},         // the batched-MFMA narrow forward recurrence: 0 never, 1 from 640 lines, 2 always
    {"bwd_mfma", 1},         // ... and backward recurrence: the same
    {"bwd_mfma_fused", 1},   // the batched backward recurrence and its weight-gradient items as one launch: 0 never,
                             //   1 below 900 lines, 2 always
    {"ctc_float", 0},        // 1: float-only log_add in the CTC alignment
    {"ctc_split", 0},        // workgroups per line of the CTC alignment: 0 the rule (ctc.h: ctc_nsplit -- the largest of 4, 2, 1 that
                             //   keeps lines x workgroups within the device's CUs), 1 one, 2 / 4 that many for every line that splits
    {"peer_two_phase", 1},   // form of the peer gradient exchange: 1 one-shot up to 4 MB and at two ranks, two-phase above 4 MB at
                             //   three or more (comm.h); 0 one-shot at every size; 2 two-phase at every size and rank count
};
inline const DbgOptDef* dbg_opt_def(const char* name) {
  for (const DbgOptDef& o : DBG_OPTS)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}
// the options set so far (CLSTM_DEBUG, then clstm_debug_set_option); throws while CLSTM_DEBUG names an unknown option
inline std::map<std::string, int>& dbg_opts() {
  static std::map<std::string, int> m = [] {
    std::map<std::string, int> r;
    const char* e = getenv("CLSTM_DEBUG");
    if (e) {
      std::string s(e);
      size_t i = 0;
      while (i < s.size()) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        const std::string kv = s.substr(i, j - i);
        const size_t eq = kv.find('=');
        if (!kv.empty()) {
          const std::string name = kv.substr(0, eq);
          if (eq == std::string::npos || !dbg_opt_def(name.c_str()))
            throw std::runtime_error("CLSTM_DEBUG: unknown option '" + name + "' (clstm_amd/csrc/dbgopt.h lists them as name=value)");
          r[name] = atoi(kv.c_str() + eq + 1);
        }
        i = j + 1;
      }
    }
    return r;
  }();
  return m;
}
inline int dbg_opt(const char* name) {
  const DbgOptDef* d = dbg_opt_def(name);
  if (!d) throw std::logic_error(std::string("internal: option '") + name + "' is not in DBG_OPTS");
  const auto& m = dbg_opts();
  const auto it = m.find(name);
  return it == m.end() ? d->dflt : it->second;
}
}  // namespace clstm
