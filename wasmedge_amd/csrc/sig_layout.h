// sig_layout.h -- how a function signature's values lie in the three forms the host moves them
// between, and the device tables built from that. Plain C++ (tests/c/sig_layout_check.cpp
// compiles it alone); args_io.h and calls_io.h take the table formats' constants from here.
//   cells: 32-bit words, [n][cells] row-major, what the device keeps (kparams.h): an i32 / f32
//          / reference one, an i64 / f64 two, a v128 four, low word first
//   slots: a device row's 64-bit slots (include/wasmedge_batch.h "device-resident arguments
//          and results"), one per value, a v128 two (low half first)
//   a WasmEdge_Value's 128 bits
#pragma once
#include <cstdint>
#include <vector>

#include "frontend.h"

constexpr uint32_t kArgsNoCell = 0xFFFFFFFFu;   // unpack: a slot's upper word that reads zero
constexpr uint32_t kCallSkip = 0xFFFFFF00u;     // kparams.h WB_CALL_SKIP (calls_io.h checks it)

// The per-function table of a staging, one row of kCallsFnWords words per name of FuncNames,
// one zero word, then the names' word_of maps back to back (the meaning of
// ArgsPackParams::word_of: the 32-bit word of the slot row each parameter cell takes).
constexpr uint32_t kCallsFnWords = 5;
constexpr uint32_t kCallsFnEntry = 0;    // calls[2i]: entry pc, or WB_CALL_SKIP | status (an import: WB_CALL_SKIP)
constexpr uint32_t kCallsFnCells = 1;    // calls[2i + 1]: parameter cells (0 unless the function runs)
constexpr uint32_t kCallsFnFunc = 2;     // module function index, 0xFFFFFFFF (-1): not found / mismatch
constexpr uint32_t kCallsFnImport = 3;   // 1: the export is a host import
constexpr uint32_t kCallsFnMap = 4;      // offset of its word_of map, in words from the table's start

constexpr uint32_t kCallsNoCall = 0xFFFFFFFFu;   // WASMEDGE_BATCH_NO_CALL

// The per-module result table, one row of kCallsResWords words per module function, then the
// functions' cell_of maps (two words per result slot: the result cell of the slot's low word,
// then of its high word or kArgsNoCell), then one zero word (never empty).
constexpr uint32_t kCallsResWords = 3;
constexpr uint32_t kCallsResLen = 0;     // result values (BatchGetReturnLens)
constexpr uint32_t kCallsResSlots = 1;   // result slots
constexpr uint32_t kCallsResMap = 2;     // offset of its cell_of map

namespace wb {

inline uint32_t slots_of(uint8_t t) { return t == V128 ? 2 : 1; }

struct SigLayout {
  uint32_t param_cells = 0, result_cells = 0, param_slots = 0, result_slots = 0;
  bool param_xref = false, result_xref = false;   // an externref among them
};

inline SigLayout layout_of(const FuncType &t) {
  SigLayout L;
  for (uint8_t ty : t.params) {
    L.param_cells += cells_of(ty);
    L.param_slots += slots_of(ty);
    L.param_xref |= ty == EXTERNREF;
  }
  for (uint8_t ty : t.results) {
    L.result_cells += cells_of(ty);
    L.result_slots += slots_of(ty);
    L.result_xref |= ty == EXTERNREF;
  }
  return L;
}

// pack: parameter cell c is 32-bit word map[c] of the slot row (slot * 2 + half)
inline std::vector<uint32_t> pack_map(const std::vector<uint8_t> &params) {
  std::vector<uint32_t> map;
  uint32_t slot = 0;
  for (uint8_t ty : params) {
    for (uint32_t q = 0; q < cells_of(ty); q++) map.push_back(slot * 2 + q);
    slot += slots_of(ty);
  }
  return map;
}

// unpack: word w of the slots of the first k results is result cell map[w], or kArgsNoCell
inline std::vector<uint32_t> unpack_map(const std::vector<uint8_t> &results, size_t k) {
  std::vector<uint32_t> map;
  uint32_t cell = 0;
  for (size_t r = 0; r < k && r < results.size(); r++) {
    const uint32_t nc = cells_of(results[r]);
    for (uint32_t q = 0; q < nc; q++) map.push_back(cell++);
    if (nc == 1) map.push_back(kArgsNoCell);
  }
  return map;
}

// a value's low cells_of(ty) words into cells (returns their number), and back
inline uint32_t to_cells(uint8_t ty, unsigned __int128 v, uint32_t *cells) {
  const uint32_t nc = cells_of(ty);
  const uint64_t lo = uint64_t(v), hi = uint64_t(v >> 64);
  cells[0] = uint32_t(lo);
  if (nc > 1) cells[1] = uint32_t(lo >> 32);
  if (nc > 2) {
    cells[2] = uint32_t(hi);
    cells[3] = uint32_t(hi >> 32);
  }
  return nc;
}
inline unsigned __int128 from_cells(uint8_t ty, const uint32_t *cells) {
  unsigned __int128 v = 0;
  for (uint32_t q = 0; q < cells_of(ty); q++) v |= (unsigned __int128)(cells[q]) << (32 * q);
  return v;
}

// One name of a SetCallsDevice: status 0 with the export it resolved to, or the status every
// instance that names it sits the run out with (FuncNotFound, FuncSigMismatch)
struct CallName {
  uint8_t status = 0;
  uint32_t func = 0, entry_pc = 0;
  bool imported = false;
  const FuncType *type = nullptr;
};

inline std::vector<uint32_t> calls_fn_table(const std::vector<CallName> &names) {
  std::vector<uint32_t> tab(names.size() * kCallsFnWords + 1, 0), maps;
  for (size_t j = 0; j < names.size(); j++) {
    const CallName &N = names[j];
    uint32_t *row = &tab[j * kCallsFnWords];
    row[kCallsFnMap] = uint32_t(tab.size());
    row[kCallsFnEntry] = kCallSkip | N.status;
    row[kCallsFnFunc] = 0xFFFFFFFFu;
    if (N.status) continue;
    const std::vector<uint32_t> map = pack_map(N.type->params);
    row[kCallsFnEntry] = N.imported ? kCallSkip : N.entry_pc;   // (an import: BatchRun refuses)
    row[kCallsFnCells] = uint32_t(map.size());
    row[kCallsFnFunc] = N.func;
    row[kCallsFnImport] = N.imported ? 1u : 0u;
    row[kCallsFnMap] += uint32_t(maps.size());
    maps.insert(maps.end(), map.begin(), map.end());
  }
  tab.insert(tab.end(), maps.begin(), maps.end());
  return tab;
}

inline std::vector<uint32_t> calls_res_table(const std::vector<const FuncType *> &funcs) {
  std::vector<uint32_t> tab(funcs.size() * kCallsResWords, 0), maps;
  for (size_t f = 0; f < funcs.size(); f++) {
    const std::vector<uint32_t> map = unpack_map(funcs[f]->results, funcs[f]->results.size());
    tab[f * kCallsResWords + kCallsResLen] = uint32_t(funcs[f]->results.size());
    tab[f * kCallsResWords + kCallsResSlots] = uint32_t(map.size() / 2);
    tab[f * kCallsResWords + kCallsResMap] = uint32_t(tab.size() + maps.size());
    maps.insert(maps.end(), map.begin(), map.end());
  }
  tab.insert(tab.end(), maps.begin(), maps.end());
  tab.push_back(0);   // (never empty)
  return tab;
}

}  // namespace wb
