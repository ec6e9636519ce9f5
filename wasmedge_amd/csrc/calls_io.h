// calls_io.h -- launch parameters of the device-resident per-instance calls (calls_io.hip),
// by value: WasmEdge_BatchSetCallsDevice / CallsResultsDevice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "args_io.h"
#include "kparams.h"

static_assert(kCallSkip == WB_CALL_SKIP, "sig_layout.h names kparams.h's word");

// (sig_layout.h: the per-name table and the per-module result table, kCallsFn* / kCallsRes*)

// What the pack kernel reduces into, zero at the launch; the host reads it back in one copy.
struct CallsSummary {
  uint64_t fp;        // += args_fp_mix over the call-table words (indices [0, 2n)) and the
                      //    cells (indices 2n + i * pc + c): order-independent
  uint32_t bad;       // max over invalid FuncOf[i] of ~i: 0 = none, else ~bad is the lowest such i
  uint32_t imported;  // != 0: some instance calls an export that is a host import
};

// FuncOf + slot rows -> a call table, parameter cells and each instance's function. It writes
// only the buffers named here, which the caller swaps in when `bad` came back 0.
struct CallsPackParams {
  const uint32_t *func_of;   // device, [n]
  const uint64_t *slots;     // device, [n][stride] (NULL when no function has parameters)
  const uint32_t *table;     // device, the per-function table
  uint32_t *calls;           // [n][2]
  uint32_t *params;          // [n][pc]
  int32_t *call_fn;          // [n]
  CallsSummary *sum;
  uint64_t stride;           // slots per row
  uint32_t n, pc, nfuncs;    // pc > 0
};

// KParams::results -> slot rows of `width` slots: the function's result slots, then zeroes; a
// row whose status is not 0 or whose call_fn is negative is all zeroes. lens[i] (when not
// NULL) = the function's result count, 0 for a negative call_fn.
struct CallsUnpackParams {
  const uint32_t *results;   // [n][cells]
  const uint8_t *status;     // [n]
  const int32_t *call_fn;    // [n]
  const uint32_t *table;     // device, the per-module result table
  uint64_t *slots;           // device, [n][stride], or NULL
  uint32_t *lens;            // device, [n], or NULL
  uint64_t stride;
  uint32_t n, cells, width;  // width = 0 with NULL slots
};

extern "C" hipError_t wb_launch_calls_pack(const CallsPackParams *p, hipStream_t s);
extern "C" hipError_t wb_launch_calls_unpack(const CallsUnpackParams *p, hipStream_t s);
