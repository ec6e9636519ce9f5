// jit_int.h -- what the units of the run compiler (jit.h) share: jit.cpp (the code
// generator), jit_sched.cpp (text post-passes), jit_load.cpp (hiprtc, loading, patching)
// and jit_hooks.cpp (test hooks). Included by them only.
#pragma once
#include <cstdint>
#include <string>

#include "jit.h"

namespace wb {
namespace jit {

// the first memory's page limit (jit_source's mem_pages): at most kMadPages, a lane's
// granule address fits 32 bits (granule_addr)
constexpr uint32_t kMadPages = 1000;
constexpr uint32_t kTripScan = 4;   // trip mode: scan iterations per trip (trip_scan_stage)
constexpr uint32_t kFwdUnroll = 1;  // counted trips: trips per pass of the counted copy (RunCompile::counted_edge)

// Every environment variable the code generator reads, each an A/B or debugging aid (results
// never depend on them). read_knobs() fills one per jit_source call -- tests set these
// between contexts of one process. Off-switches are on unless the variable starts with '0'.
struct JitKnobs {
  bool hybrid;         // WB_HYBRID=0: trip mode alone, not beside SIMT scheduling
  bool nanobs;         // WB_NANOBS=0: NaN fixes everywhere, not only where a payload is observed
  bool fold;           // WB_FOLD=0: no constant folds, no fused any_true (no liveness)
  bool cmpany;         // WB_CMPANY=0: an f64x2 compare never hands its masks to the branch
  bool jit_sched;      // WB_JIT_SCHED=0: the runs' code stays in program order
  bool sched_stores;   // WB_SCHED_STORES=0: stores stay barriers of the list scheduler
  bool load_batch;     // WB_LOAD_BATCH=0: loads in program order
  bool depth;          // WB_DEPTH=0: pc-only scheduler picks for recursive modules too
  bool inline_calls;   // WB_INLINE=0: no inlined leaf calls
  bool fwd;            // WB_FWD=0: no loop-carried forwarding copies
  bool fwd_store;      // WB_FWD_STORE=0: a forwarded word is copied after its store
  bool fwd_alias;      // WB_FWD_ALIAS=0: a forwarded load is a move, not a renamed cell
  bool kprop;          // WB_KPROP=0: every CONST32 / MOV32 of a compiled run writes its register
  bool fwd_lazy;       // WB_FWD_LAZY=0: a forwarding copy's stores go to memory every trip
  bool fwd_loop;       // WB_FWD_LOOP=0: the copies keep their stack check, jump and second count
  bool fwd_tail;       // WB_FWD_TAIL=0: a tight loop tests LOW, OTHER and the count limit every trip
  bool fwd_count;      // WB_FWD_COUNT=0: no counted copy of a tight loop's block (off with WB_FWD_TAIL)
  uint32_t fwd_unroll; // WB_FWD_UNROLL=n: trips per pass of the counted copy (1, 2 or 4; default kFwdUnroll)
  bool ret_pf;         // WB_RET_PF=0: POST_CALL never reads the RET's record along
  bool brt_thread;     // WB_BRT_THREAD=0: a JMP onto a br_table's run does not take the table
  bool trip_fwd;       // WB_TRIP_FWD=0: no trip-mode load cache
  bool trip_fwdchk;    // WB_TRIP_FWDCHK=0: stages test every access group again
  bool trip_mad;       // WB_TRIP_MAD=0: 64-bit granule addresses in trip stages
  bool trip_split;     // WB_TRIP_SPLIT=0: every run whole in stage B
  bool trip_pf;        // WB_TRIP_PF=0: no successor-window prefetch
  bool trip_x4;        // WB_TRIP_X4=0: scan windows word by word always
  bool trip_scanbf;    // WB_TRIP_SCANBF=0: a scan's stage B iteration by iteration
  bool trip_batch;     // WB_TRIP_BATCH=0: no batched lane tests
  bool trip_inline;    // WB_TRIP_INLINE=0: every stage out of line
  bool trip_smask;     // WB_TRIP_SMASK=0: moved lanes join a batch by compares
  bool trip_cmpbr;     // WB_TRIP_CMPBR=0: br_if / br_unless compare their cell again
  bool trip_chain;     // WB_TRIP_CHAIN=0: no forward chaining
  bool trip_guard;     // WB_TRIP_GUARD=0: no guard blocks
  bool trip_conv1;     // WB_TRIP_CONV1=1 (the one on-switch): the one-pc test after every trip
  unsigned simt_x;     // WB_SIMT_X=n: divergence events kept in the core (1 | 2 | 4; default 7)
  uint32_t trip_scan;  // WB_TRIP_SCAN=n: scan iterations per trip (at most kTripScan, the default; below 2: off)
  uint32_t trip_convp; // WB_TRIP_CONVP=k: the one-pc test after every 2^k-th trip (1..8, default 4)
  int trip_outsh;      // WB_TRIP_OUTSH=k: leave the trips at 2^k times as many lanes outside (0..6, default 6)
  const char *nanobs_list;   // WB_NANOBS_LIST=<file>: nan_observable's result per pc (null: none)
};
JitKnobs read_knobs();

// text post-passes (jit_sched.cpp)
std::string schedule(const std::string &body, const JitKnobs &kn);
std::string resolve_jumps(const std::string &body);

// Whether a function can reach itself through calls (jit.cpp; the depth-keyed SIMT pick)
bool recursive(const Program &P);

}  // namespace jit
}  // namespace wb
