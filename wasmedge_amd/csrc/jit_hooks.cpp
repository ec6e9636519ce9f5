// jit_hooks.cpp -- test hooks of the run compiler (CPU tests call them through the
// library; the product path never does) with their own debugging knobs: WB_JIT_LIST,
// WB_JIT_DUMP / WB_JIT_DUMP_SIMT / WB_JIT_DUMP_TRIP, WB_JIT_CHECK_PAGES, WB_JIT_CHECK_COST.
#include <cstdio>
#include <cstdlib>

#include <string>
#include <vector>

#include "frontend.h"
#include "jit_int.h"
#include "tc_slots.h"

// TEST hook (tests/test_jit.py, CPU): lower a module, pick its runs and assemble them for
// gfx950 without a device. Returns the number of runs, or -1 with the error in err.
extern "C" __attribute__((visibility("default"))) int wb_jit_check(const uint8_t *wasm, uint32_t len,
                                                                   uint32_t glog, uint32_t *instrs,
                                                                   char *err, uint32_t errlen) {
  wb::Program P;
  uint8_t ec = 0;
  // WB_JIT_CHECK_COST=1: as a metered context compiles them (unit costs, plain runs only)
  const char *mc = getenv("WB_JIT_CHECK_COST");
  const bool metered = mc && mc[0] == '1';
  std::string e = wb::load_program(wasm, len, P, &ec, metered, nullptr, true, true);
  std::vector<uint32_t> cost_off;
  std::vector<uint64_t> cost_pool;
  const wb::JitCost jc{&cost_off, &cost_pool, 1};
  if (e.empty() && metered) {
    const std::vector<uint64_t> tab(65536, 1ull);
    bool exceeded = false;
    wb::build_cost_pool(P, tab.data(), ~0ull, cost_off, cost_pool, &exceeded);
  }
  std::vector<wb::JitRun> runs;
  if (e.empty() && P.total_cells() > TC_VF_CELLS) e = "frame too large for V frames";
  // extra memories laid out at their minimum sizes (batch_api.cpp reserves more for grown ones)
  std::vector<uint32_t> xinfo;
  uint64_t words = 0;
  for (const auto &xm : P.xmems) {
    xinfo.push_back(uint32_t(words));
    xinfo.push_back(xm.min);
    words += uint64_t(xm.min) << 14;
  }
  if (e.empty()) {
    std::vector<DInstr> code = P.code;
    code.push_back(DInstr{0, 0, 0, 0});
    const std::vector<TInstr> tc = wb::build_threaded(P, code, true);
    runs = wb::jit_runs(P, tc);
    // debug listing: every DBC instruction (op, fields) with the SIMT run it belongs to
    if (const char *lst = getenv("WB_JIT_LIST"))
      if (FILE *f = fopen(lst, "w")) {
        static const char *const names[] = {
#define WB_NAME(x) #x,
            DBC_OPS(WB_NAME)
#undef WB_NAME
        };
        const std::vector<wb::JitRun> sr = wb::jit_runs(P, tc, true);
        std::vector<int> at(P.code.size(), -1);
        for (size_t k = 0; k < sr.size(); k++)
          for (uint32_t i = 0; i < sr[k].len; i++) at[sr[k].pc + i] = int(k);
        for (size_t pc = 0; pc < P.code.size(); pc++) {
          const DInstr &I = P.code[pc];
          const uint16_t op = uint16_t(I.w0 & 0x7FFFu);
          fprintf(f, "%4zu %s%-4s %-22s a=%u b=%u c=%u d=%d imm=0x%x cnt=%u\n", pc,
                  at[pc] >= 0 && sr[at[pc]].pc == pc ? "R" : " ",
                  at[pc] >= 0 ? std::to_string(at[pc]).c_str() : "-",
                  op < OP_DBC_NUM_OPS ? names[op] : "?", I.w1 & 0xFFFFu, I.w1 >> 16, I.w2 & 0xFFFFu,
                  int(int16_t(I.w2 >> 16)), I.w3, (I.w0 >> 16) & 0xFFu);
        }
        fclose(f);
      }
    if (instrs) {
      *instrs = 0;
      for (const auto &r : runs) *instrs += r.len;
    }
    // every flavour: plain runs, SIMT scheduling (KParams::simt, its own run choice) and
    // trip mode (its own run choice too)
    for (int simt = 0; simt < (metered ? 1 : 3) && e.empty(); simt++) {
      if (simt) runs = wb::jit_runs(P, tc, true, simt == 2);
      if (runs.empty()) continue;
      std::vector<char> obj;
      // (a memory below kMadPages unless WB_JIT_CHECK_PAGES says otherwise: the 32-bit
      // granule addresses of trip stages assembled too)
      const char *cp = getenv("WB_JIT_CHECK_PAGES");
      const std::string src = wb::jit_source(P, runs, glog, metered ? &jc : nullptr, simt != 0, simt == 2, &xinfo,
                                             P.divergent_xmem ? 5u : 0u, cp ? uint32_t(atoi(cp)) : wb::jit::kMadPages);
      if (const char *dump = getenv(simt == 2 ? "WB_JIT_DUMP_TRIP" : simt ? "WB_JIT_DUMP_SIMT" : "WB_JIT_DUMP"))
        if (FILE *f = fopen(dump, "w")) { fputs(src.c_str(), f); fclose(f); }
      e = src.empty() ? "no source" : wb::jit_compile(src, &obj);
    }
  }
  if (!e.empty()) {
    if (err && errlen) snprintf(err, errlen, "%s", e.c_str());
    return -1;
  }
  return int(runs.size());
}

// TEST hook (tests/test_jit.py, CPU): whether a SIMT context of this module runs trip mode
// (Program::divergent_mem or wb::trips_pay; WB_TRIP unset). 1 / 0, or -1 when it fails to load.
extern "C" __attribute__((visibility("default"))) int wb_trip_choice(const uint8_t *wasm, uint32_t len) {
  wb::Program P;
  uint8_t ec = 0;
  if (!wb::load_program(wasm, len, P, &ec).empty()) return -1;
  return P.divergent_mem || P.divergent_xmem || wb::trips_pay(P) ? 1 : 0;
}

// TEST hook (tests/test_depth_pick.py, CPU): whether the module counts as recursive for the
// depth-keyed SIMT pick (wb::recursive). 1 / 0, or -1 when it fails to load.
extern "C" __attribute__((visibility("default"))) int wb_recursive(const uint8_t *wasm, uint32_t len) {
  wb::Program P;
  uint8_t ec = 0;
  if (!wb::load_program(wasm, len, P, &ec).empty()) return -1;
  return wb::jit::recursive(P) ? 1 : 0;
}
