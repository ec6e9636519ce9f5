// args_io.h -- launch parameters of the device-resident argument and result rows
// (args_io.hip), by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sig_layout.h"

// A slot row (include/wasmedge_batch.h "device-resident arguments and results") is a
// function's values back to back, one 64-bit slot each, a v128 two (low half first). The
// device keeps arguments and results as 32-bit cells, [n][cells] row-major (kparams.h). A
// per-signature table in device memory names, for every cell, the 32-bit word of the slot
// row it is: entry = slot * 2 + half. Its length is the signature's, not the kernarg's.
// (sig_layout.h: the maps and kArgsNoCell)

// slots -> KParams::params, and the arguments' fingerprint (args_fp_mix summed over all cells)
struct ArgsPackParams {
  const uint64_t *slots;   // device, [n][stride]
  const uint32_t *word_of; // device, [cells]: the word of the slot row each cell takes
  uint32_t *params;        // [n][cells]
  uint64_t *fp;            // device word, zero at the launch: += the sum over all cells
  uint64_t stride;         // slots per row
  uint32_t n, cells;       // cells > 0
};

// KParams::results -> slots: the first `words` / 2 slots of every row; a row whose status is
// not 0 gets zeroes there. Slots past them, and the rows' padding, are not written.
struct ArgsUnpackParams {
  const uint32_t *results; // [n][cells]
  const uint8_t *status;   // [n]
  const uint32_t *cell_of; // device, [words]: the result cell each word of the slot row is,
                           // or kArgsNoCell (zero: the upper word of a 32-bit value)
  uint64_t *slots;         // device, [n][stride]
  uint64_t stride;
  uint32_t n, cells, words;   // words > 0 and even
};

// One cell's term of the fingerprint: a mix of its index in [n][cells] and its value. The
// fingerprint is the wrapping 64-bit sum of the terms, so any reduction order and any launch
// geometry give the same value.
__host__ __device__ inline uint64_t args_fp_mix(uint64_t index, uint32_t value) {
  uint64_t x = index ^ 0x9E3779B97F4A7C15ull;
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33;
  x += value;
  x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
  return x;
}

// threads per block: 256, or WB_ARGS_BLOCK (a multiple of 64 up to 1024) -- the results and
// the fingerprint do not depend on it
extern "C" uint32_t wb_args_io_block(void);
extern "C" hipError_t wb_launch_args_pack(const ArgsPackParams *p, hipStream_t s);
extern "C" hipError_t wb_launch_args_unpack(const ArgsUnpackParams *p, hipStream_t s);
