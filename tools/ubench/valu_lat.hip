// Issue-to-use latency of the chain loop's VALU instructions (tuning aid only; the list
// scheduler's table, jit_sched.cpp). One wave per SIMD, as C2 runs: a lone wave issues one
// instruction every 4 cycles and nothing hides a dependent instruction's wait. Each
// variant times (s_memtime) a block of `rept x group` instructions in which every
// instruction reads the result of the one `dist` slots before it: cycles per instruction
// = max(4, latency / dist), so dist 1 reads the latency and dist 8 the issue rate. The
// mixed variants are the loop's producer -> consumer pairs and the whole G chain
// (add3, xor, rotate, add, xor, rotate). Each block runs four times; the first pass
// (instruction cache cold) is dropped and the fastest of the rest kept.
//
// Prints one line per variant: instructions, and over the waves the least, median and
// greatest cycles per instruction (less the empty block's time).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

constexpr uint32_t kWaves = 1024;

#define XOR(d) "v_xor_b32 v" #d ", v15, v" #d "\n"
#define ADD(d) "v_add_u32 v" #d ", v15, v" #d "\n"
#define ADD3(d) "v_add3_u32 v" #d ", v" #d ", v15, v14\n"
#define ROT(d) "v_alignbit_b32 v" #d ", v" #d ", v" #d ", 7\n"
#define G(d) ADD3(d) XOR(d) ROT(d) ADD(d) XOR(d) ROT(d)
#define P_ADD3_XOR(d) ADD3(d) XOR(d)
#define P_XOR_ROT(d) XOR(d) ROT(d)
#define P_ROT_ADD(d) ROT(d) ADD(d)
#define P_ADD_XOR(d) ADD(d) XOR(d)
#define D1(I) I(0)
#define D2(I) I(0) I(1)
#define D3(I) I(0) I(1) I(2)
#define D4(I) I(0) I(1) I(2) I(3)
#define D8(I) I(0) I(1) I(2) I(3) I(4) I(5) I(6) I(7)
// a G chain interleaved over 4 registers instruction by instruction, as the scheduled loop is
#define G4 ADD3(0) ADD3(1) ADD3(2) ADD3(3) XOR(0) XOR(1) XOR(2) XOR(3) ROT(0) ROT(1) ROT(2) ROT(3) \
           ADD(0) ADD(1) ADD(2) ADD(3) XOR(0) XOR(1) XOR(2) XOR(3) ROT(0) ROT(1) ROT(2) ROT(3)

#define GX(D) D(ADD3) D(XOR) D(ROT) D(ADD) D(XOR) D(ROT)
// G4's opcodes in G4's order with no instruction reading another's result
#define NADD3(d) "v_add3_u32 v" #d ", v14, v15, v14\n"
#define NXOR(d) "v_xor_b32 v" #d ", v15, v14\n"
#define NROT(d) "v_alignbit_b32 v" #d ", v14, v14, 7\n"
#define NADD(d) "v_add_u32 v" #d ", v15, v14\n"
#define D4B(I) I(4) I(5) I(6) I(7)
#define D4C(I) I(8) I(9) I(10) I(11)
#define G4N D4(NADD3) D4B(NXOR) D4C(NROT) D4(NADD) D4B(NXOR) D4C(NROT)

#define STR2(x) #x
#define STR(x) STR2(x)
#define TIMED(IDX, REPT, BODY)                                                                   \
  {                                                                                              \
    uint64_t best = ~0ull;                                                                       \
    _Pragma("unroll 1") /* (one copy of the block: the later passes find it cached) */           \
    for (int pass = 0; pass < 4; pass++) {                                                       \
      uint64_t t0, t1;                                                                           \
      asm volatile("s_memtime %0\n"                                                              \
                   "s_waitcnt lgkmcnt(0)\n"                                                      \
                   ".rept " STR(REPT) "\n" BODY ".endr\n"                                        \
                   "s_memtime %1\n"                                                              \
                   "s_waitcnt lgkmcnt(0)\n"                                                      \
                   : "=&s"(t0), "=&s"(t1)                                                        \
                   :                                                                             \
                   : "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v14", "v15",    \
                     "memory");                                                                  \
      if (pass && t1 - t0 < best) best = t1 - t0;                                                \
    }                                                                                            \
    if (lane == 0) out[(IDX) * kWaves + wave] = best;                                            \
  }

struct Variant {
  const char *name;
  uint32_t n;   // instructions in the block
};
static const Variant kVariants[] = {
    {"empty", 0},
    {"xor dist 1", 2048}, {"xor dist 2", 2048}, {"xor dist 3", 2049}, {"xor dist 4", 2048}, {"xor dist 8", 2048},
    {"add dist 1", 2048}, {"add dist 2", 2048}, {"add dist 3", 2049}, {"add dist 4", 2048}, {"add dist 8", 2048},
    {"add3 dist 1", 2048}, {"add3 dist 2", 2048}, {"add3 dist 3", 2049}, {"add3 dist 4", 2048}, {"add3 dist 8", 2048},
    {"alignbit dist 1", 2048}, {"alignbit dist 2", 2048}, {"alignbit dist 3", 2049}, {"alignbit dist 4", 2048},
    {"alignbit dist 8", 2048},
    {"add3->xor pair", 2048}, {"xor->alignbit pair", 2048}, {"alignbit->add pair", 2048}, {"add->xor pair", 2048},
    {"G chain dist 1", 2046}, {"G chain x4 interleaved", 2040},
    {"add3->xor dist 2", 2048}, {"add3->xor dist 4", 2048}, {"xor->alignbit dist 4", 2048},
    {"alignbit->add dist 4", 2048}, {"add->xor dist 4", 2048}, {"alignbit->add3 dist 4", 2048},
    {"G chain x2 interleaved", 2040}, {"G chain x3 interleaved", 2034}, {"G chain x8 interleaved", 2016},
    {"G x4 opcodes, independent", 2040},
};
constexpr uint32_t kNV = sizeof(kVariants) / sizeof(kVariants[0]);

__global__ void __launch_bounds__(64) k_lat(uint64_t *out) {
  const uint32_t wave = blockIdx.x, lane = threadIdx.x;
  TIMED(0, 1, "")
  TIMED(1, 2048, D1(XOR)) TIMED(2, 1024, D2(XOR)) TIMED(3, 683, D3(XOR)) TIMED(4, 512, D4(XOR)) TIMED(5, 256, D8(XOR))
  TIMED(6, 2048, D1(ADD)) TIMED(7, 1024, D2(ADD)) TIMED(8, 683, D3(ADD)) TIMED(9, 512, D4(ADD)) TIMED(10, 256, D8(ADD))
  TIMED(11, 2048, D1(ADD3)) TIMED(12, 1024, D2(ADD3)) TIMED(13, 683, D3(ADD3)) TIMED(14, 512, D4(ADD3))
  TIMED(15, 256, D8(ADD3))
  TIMED(16, 2048, D1(ROT)) TIMED(17, 1024, D2(ROT)) TIMED(18, 683, D3(ROT)) TIMED(19, 512, D4(ROT))
  TIMED(20, 256, D8(ROT))
  TIMED(21, 1024, D1(P_ADD3_XOR)) TIMED(22, 1024, D1(P_XOR_ROT)) TIMED(23, 1024, D1(P_ROT_ADD))
  TIMED(24, 1024, D1(P_ADD_XOR))
  TIMED(25, 341, D1(G)) TIMED(26, 85, G4)
  TIMED(27, 512, D2(ADD3) D2(XOR)) TIMED(28, 256, D4(ADD3) D4(XOR)) TIMED(29, 256, D4(XOR) D4(ROT))
  TIMED(30, 256, D4(ROT) D4(ADD)) TIMED(31, 256, D4(ADD) D4(XOR)) TIMED(32, 256, D4(ROT) D4(ADD3))
  TIMED(33, 170, GX(D2)) TIMED(34, 113, GX(D3)) TIMED(35, 42, GX(D8))
  TIMED(36, 85, G4N)
}

int main() {
  uint64_t *out;
  const size_t bytes = size_t(kNV) * kWaves * sizeof(uint64_t);
  if (hipMalloc(&out, bytes) != hipSuccess) {
    printf("alloc failed\n");
    return 1;
  }
  std::vector<uint64_t> h(size_t(kNV) * kWaves);
  bool ok = hipMemset(out, 0, bytes) == hipSuccess;
  k_lat<<<kWaves, 64>>>(out);
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  ok = ok && hipMemcpy(h.data(), out, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) {
    printf("kernel failed\n");
    return 1;
  }
  std::vector<uint64_t> e(h.begin(), h.begin() + kWaves);
  std::sort(e.begin(), e.end());
  const double empty = double(e[kWaves / 2]);
  printf("waves %u, empty block %.0f cycles (median)\n", kWaves, empty);
  printf("%-26s %6s %8s %8s %8s\n", "variant", "instrs", "min", "median", "max");
  for (uint32_t v = 1; v < kNV; v++) {
    std::vector<uint64_t> w(h.begin() + size_t(v) * kWaves, h.begin() + size_t(v + 1) * kWaves);
    std::sort(w.begin(), w.end());
    const double n = kVariants[v].n;
    printf("%-26s %6u %8.2f %8.2f %8.2f\n", kVariants[v].name, kVariants[v].n, (double(w[0]) - empty) / n,
           (double(w[kWaves / 2]) - empty) / n, (double(w[kWaves - 1]) - empty) / n);
  }
  return 0;
}
