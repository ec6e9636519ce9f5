// sig_layout_check.cpp -- wasmedge_amd/csrc/sig_layout.h against literals written out by hand
// from the formats (args_io.h: cells, slots and the pack / unpack maps; calls_io.h: the per-name
// table and the per-module result table). Host code only, built with the address and
// undefined-behaviour sanitizers by tests/test_sig_layout.py. Prints "ok <checks>" or the
// first difference.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sig_layout.h"

using wb::FuncType;
using U = std::vector<uint32_t>;
using u128 = unsigned __int128;

static int checks = 0;

static void same(const char *what, const U &got, const U &want) {
  checks++;
  if (got == want) return;
  printf("%s:\n  got ", what);
  for (uint32_t w : got) printf(" %x", w);
  printf("\n  want");
  for (uint32_t w : want) printf(" %x", w);
  printf("\n");
  exit(1);
}

static void layout(const char *what, const FuncType &t, const U &want) {
  const wb::SigLayout L = wb::layout_of(t);
  same(what, U{L.param_cells, L.result_cells, L.param_slots, L.result_slots, L.param_xref, L.result_xref}, want);
}

int main() {
  const uint32_t N = 0xFFFFFFFFu;
  const uint8_t I32 = 0x7F, I64 = 0x7E, F32 = 0x7D, F64 = 0x7C, V128 = 0x7B, FUNCREF = 0x70, EXTERNREF = 0x6F;
  same("constants", U{kArgsNoCell, kCallsNoCall, kCallSkip, kCallsFnWords, kCallsFnEntry, kCallsFnCells, kCallsFnFunc,
                      kCallsFnImport, kCallsFnMap, kCallsResWords, kCallsResLen, kCallsResSlots, kCallsResMap},
       U{N, N, 0xFFFFFF00u, 5, 0, 1, 2, 3, 4, 3, 0, 1, 2});

  // (i32, v128, i64) -> (i32, i64, v128): 7 cells and 4 slots on either side
  const FuncType mixed{{I32, V128, I64}, {I32, I64, V128}};
  layout("mixed layout", mixed, U{7, 7, 4, 4, 0, 0});
  same("mixed pack map", wb::pack_map(mixed.params), U{0, 2, 3, 4, 5, 6, 7});
  same("mixed unpack map", wb::unpack_map(mixed.results, 3), U{0, N, 1, 2, 3, 4, 5, 6});
  same("mixed unpack map, two results", wb::unpack_map(mixed.results, 2), U{0, N, 1, 2});
  same("mixed unpack map, more asked than there are", wb::unpack_map(mixed.results, 9), U{0, N, 1, 2, 3, 4, 5, 6});
  same("mixed unpack map, none", wb::unpack_map(mixed.results, 0), U{});

  const FuncType empty{};
  layout("empty layout", empty, U{0, 0, 0, 0, 0, 0});
  same("empty pack map", wb::pack_map(empty.params), U{});
  same("empty unpack map", wb::unpack_map(empty.results, 4), U{});

  const FuncType fl{{F32, F64}, {F32, F64}};
  layout("float layout", fl, U{3, 3, 2, 2, 0, 0});
  same("float pack map", wb::pack_map(fl.params), U{0, 2, 3});
  same("float unpack map", wb::unpack_map(fl.results, 2), U{0, N, 1, 2});

  // an externref on one side only; a funcref is no externref
  layout("externref parameter", FuncType{{I64, EXTERNREF}, {FUNCREF}}, U{3, 1, 2, 1, 1, 0});
  layout("externref result", FuncType{{FUNCREF, V128}, {I32, EXTERNREF}}, U{5, 2, 3, 2, 0, 1});
  same("externref pack map", wb::pack_map({I64, EXTERNREF}), U{0, 1, 2});
  same("externref unpack map", wb::unpack_map({I32, EXTERNREF}, 2), U{0, N, 1, N});

  // the codec: a type's cells are the value's low words, and only they are written or read
  const uint8_t types[7] = {I32, I64, F32, F64, V128, FUNCREF, EXTERNREF};
  const uint32_t ncells[7] = {1, 2, 1, 2, 4, 1, 1};
  const uint32_t word[4] = {0x11111111u, 0x22222222u, 0x33333333u, 0x44444444u};
  const u128 distinct = (u128(0x4444444433333333ull) << 64) | 0x2222222211111111ull;
  for (int k = 0; k < 7; k++)
    for (int ones = 0; ones < 2; ones++) {
      const u128 v = ones ? ~u128(0) : distinct;
      uint32_t cells[5] = {0xABABABABu, 0xABABABABu, 0xABABABABu, 0xABABABABu, 0xABABABABu};
      U want(5, 0xABABABABu), got;
      for (uint32_t q = 0; q < ncells[k]; q++) want[q] = ones ? N : word[q];
      same("to_cells count", U{wb::to_cells(types[k], v, cells), wb::cells_of(types[k])}, U{ncells[k], ncells[k]});
      same("to_cells", U(cells, cells + 5), want);
      const u128 low = ncells[k] == 4 ? v : v & ((u128(1) << (32 * ncells[k])) - 1);
      const u128 back = wb::from_cells(types[k], cells);
      for (int q = 0; q < 4; q++) got.push_back(uint32_t(back >> (32 * q)));
      same("from_cells", got, U{uint32_t(low), uint32_t(low >> 32), uint32_t(low >> 64), uint32_t(low >> 96)});
    }

  // the per-name table: 5 words per name, one zero word, the found names' pack maps; a map
  // offset counts from the table's start (16 = 3 * 5 + 1 here), also in a row without a map
  const FuncType one{{I64}, {}};
  same("per-name table", wb::calls_fn_table({{0, 7, 100, false, &mixed}, {0x05, 0, 0, false, nullptr},
                                             {0x83, 0, 0, false, nullptr}}),
       U{100, 7, 7, 0, 16,
         0xFFFFFF05u, 0, N, 0, 16,
         0xFFFFFF83u, 0, N, 0, 16,
         0,
         0, 2, 3, 4, 5, 6, 7});
  // ... an import sits the run out (BatchRun refuses it), and the second map follows the first
  same("per-name table, import", wb::calls_fn_table({{0, 2, 55, true, &fl}, {0x83, 0, 0, false, nullptr},
                                                     {0, 9, 200, false, &one}, {0, 4, 300, false, &empty}}),
       U{0xFFFFFF00u, 3, 2, 1, 21,
         0xFFFFFF83u, 0, N, 0, 21,
         200, 2, 9, 0, 24,
         300, 0, 4, 0, 26,
         0,
         0, 2, 3,
         0, 1});
  same("per-name table, no names", wb::calls_fn_table({}), U{0});

  // the per-module result table: 3 words per function, the unpack maps, one zero word
  const FuncType f32r{{}, {F32}};
  same("result table", wb::calls_res_table({&mixed, &empty, &f32r}),
       U{3, 4, 9,
         0, 0, 17,
         1, 1, 17,
         0, N, 1, 2, 3, 4, 5, 6,
         0, N,
         0});
  same("result table, no functions", wb::calls_res_table({}), U{0});
  printf("ok %d\n", checks);
  return 0;
}
