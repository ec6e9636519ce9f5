// jit_load.cpp -- the generated source through hiprtc, onto the device and into the
// threaded code (jit.h).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "jit.h"
#include "tc_slots.h"

namespace wb {

std::string jit_compile(const std::string &src, std::vector<char> *code, const std::string &arch) {
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, src.c_str(), "wbjit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    return "hiprtcCreateProgram failed";
  const std::string target = "--offload-arch=" + arch;
  const char *opts[] = {target.c_str(), "-O1"};
  if (hiprtcCompileProgram(prog, 2, opts) != HIPRTC_SUCCESS) {
    size_t n = 0;
    hiprtcGetProgramLogSize(prog, &n);
    std::string log(n + 1, '\0');
    hiprtcGetProgramLog(prog, log.data());
    hiprtcDestroyProgram(&prog);
    return "compiled-run assembly failed: " + log.substr(0, 2000);
  }
  size_t sz = 0;
  hiprtcGetCodeSize(prog, &sz);
  code->assign(sz, 0);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  return "";
}

std::string jit_load(const std::string &src, size_t nruns, int device, std::vector<uint64_t> *addr) {
  // one code object per (HIP context, device, source) while that context lives: contexts
  // of the same module share it (a new primary context after hipDeviceReset gets its own)
  static std::mutex mu;
  static std::map<std::tuple<uintptr_t, int, std::string>, std::vector<uint64_t>> cache;
  std::lock_guard<std::mutex> lock(mu);
  hipCtx_t hctx = nullptr;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wdeprecated-declarations"
  (void)hipCtxGetCurrent(&hctx);
#pragma clang diagnostic pop
  const auto key = std::make_tuple(uintptr_t(hctx), device, src);
  auto it = cache.find(key);
  if (it != cache.end()) { *addr = it->second; return ""; }
  // the device's own target (gfx950 on MI355X), not a hard-coded one
  std::string arch = "gfx950";
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.gcnArchName[0]) {
    arch = prop.gcnArchName;
    const size_t colon = arch.find(':');   // (feature suffixes such as :sramecc+:xnack-)
    if (colon != std::string::npos) arch.resize(colon);
  }
  std::vector<char> code;
  std::string err = jit_compile(src, &code, arch);
  if (!err.empty()) return err;
  hipModule_t mod;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess) return "hipModuleLoadData failed";
  hipFunction_t fn;
  if (hipModuleGetFunction(&fn, mod, "wbjit_addrs") != hipSuccess) return "hipModuleGetFunction failed";
  uint64_t *dout = nullptr;
  if (hipMalloc(&dout, std::max<size_t>(1, nruns) * 8) != hipSuccess) return "hipMalloc failed";
  unsigned nr = unsigned(nruns);
  void *args[] = {&dout, &nr};
  std::vector<uint64_t> a(nruns, 0);
  // (a private stream: BatchCreate must not wait for other contexts' kernels)
  hipStream_t qs = nullptr;
  const bool ok = hipStreamCreateWithFlags(&qs, hipStreamNonBlocking) == hipSuccess &&
                  hipModuleLaunchKernel(fn, 1, 1, 1, 64, 1, 1, 0, qs, args, nullptr) == hipSuccess &&
                  hipMemcpyAsync(a.data(), dout, nruns * 8, hipMemcpyDeviceToHost, qs) == hipSuccess &&
                  hipStreamSynchronize(qs) == hipSuccess;
  if (qs) (void)hipStreamDestroy(qs);
  (void)hipFree(dout);
  if (!ok) return "compiled-run address query failed";
  for (uint64_t x : a)
    if (x == 0 || (x & 63)) return "compiled-run address query returned a bad address";
  cache[key] = a;   // the module stays loaded: its code is jumped to
  *addr = a;
  return "";
}

void jit_patch(std::vector<TInstr> &tc, const std::vector<JitRun> &runs, const std::vector<uint64_t> &addr) {
  for (size_t k = 0; k < runs.size(); k++) {
    uint32_t *w = tc[runs[k].pc].w;
    w[0] = TC_SLOT_JIT * TC_SLOT_BYTES;
    w[1] = uint32_t(addr[k]);
    w[2] = uint32_t(addr[k] >> 32);
    w[3] = w[4] = w[6] = w[7] = 0;
    w[5] = (runs[k].len - 1) * 32u;
  }
}

}  // namespace wb
