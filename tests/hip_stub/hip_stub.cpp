// hip_stub.cpp — TEST INFRASTRUCTURE (tests/test_device_order.py), never part of the product.
//
// An LD_PRELOAD interposer for the HIP runtime entry points libbsx.so imports, for a box WITHOUT a GPU: "device memory" is host memory, launches do nothing, and every
// call is logged with the calling thread's CURRENT device.  It pretends to have BSX_STUB_NDEV (default 2) devices, so the code path `device != 0` — which no
// single-GPU test box can execute — runs its real host code (plan, hipRTC cache load, per-device attributes, hipGraph capture, every entry point's device guard)
// and the test can assert that no device-affine HIP call is made while another device is current, that streams / events / allocations are only used on the device
// they were created on, and that the caller's device is restored.  Results of the "kernels" are meaningless; order and device affinity are what is checked.
// Launch lines also name the kernel and its geometry (`name g=x,y,z b=x,y,z sh=<dynamic LDS> s=<stream>`), stream waits and event records name their handles,
// copies and allocations their sizes: tools/step_trace.py turns that into a launch trace to compare two builds of the library.
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

namespace {
thread_local int t_dev = 0;
std::mutex g_mu;
std::map<const void*, int> g_owner;       // stream / event / allocation / module / graph → device it was created on
FILE* g_log = nullptr;
int g_capture = 0;

int ndev() { const char* e = getenv("BSX_STUB_NDEV"); return e ? atoi(e) : 2; }
void logf(const char* api, const char* kind, const char* note = "") {
  std::lock_guard<std::mutex> l(g_mu);
  if (!g_log) { const char* p = getenv("BSX_STUB_LOG"); g_log = p ? fopen(p, "a") : nullptr; if (!g_log) return; }
  fprintf(g_log, "%s %s %d %s\n", kind, api, t_dev, note);
  fflush(g_log);
}
void own(const void* p) { std::lock_guard<std::mutex> l(g_mu); g_owner[p] = t_dev; }
void disown(const void* p) { std::lock_guard<std::mutex> l(g_mu); g_owner.erase(p); }
// a handle used while a device other than its creator's is current → "MISMATCH" line
void use(const char* api, const void* p) {
  if (!p) return;
  int o = -1;
  { std::lock_guard<std::mutex> l(g_mu); auto it = g_owner.find(p); if (it != g_owner.end()) o = it->second; }
  if (o >= 0 && o != t_dev) { char b[64]; snprintf(b, sizeof b, "owner=%d", o); logf(api, "MISMATCH", b); }
}
void* handle() { return calloc(1, 64); }
std::map<const void*, std::string> g_kernel;   // host stub (triple-chevron launches) or hipFunction_t (module launches) → kernel name
struct CallConfig { dim3 g, b; size_t sh = 0; hipStream_t s = nullptr; };
thread_local CallConfig t_cfg;
std::string kernel_name(const void* f) {
  std::lock_guard<std::mutex> l(g_mu);
  auto it = g_kernel.find(f);
  return it == g_kernel.end() ? "?" : it->second;
}
void log_launch(const char* api, const void* f, dim3 g, dim3 b, size_t sh, hipStream_t s) {
  char note[512];
  snprintf(note, sizeof note, "%s g=%u,%u,%u b=%u,%u,%u sh=%zu s=%p", kernel_name(f).c_str(), g.x, g.y, g.z, b.x, b.y, b.z, sh, (void*)s);
  logf(api, "affine", note);
}
void log_ptrs(const char* api, const char* fmt, const void* a, const void* b) { char note[96]; snprintf(note, sizeof note, fmt, a, b); logf(api, "affine", note); }
void log_size(const char* api, size_t n, hipStream_t s = nullptr) { char note[64]; snprintf(note, sizeof note, "n=%zu s=%p", n, (void*)s); logf(api, "affine", note); }
}  // namespace

extern "C" {
int bsx_stub_current_device() { return t_dev; }
void bsx_stub_set_device(int d) { t_dev = d; }

hipError_t hipGetDeviceCount(int* n) { *n = ndev(); logf("hipGetDeviceCount", "neutral"); return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = t_dev; return hipSuccess; }
hipError_t hipSetDevice(int d) { if (d < 0 || d >= ndev()) return hipErrorInvalidDevice; t_dev = d; logf("hipSetDevice", "neutral"); return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub error"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int dev) {
  memset(p, 0, sizeof *p);
  snprintf(p->gcnArchName, sizeof p->gcnArchName, "gfx950:sramecc+:xnack-");
  p->multiProcessorCount = 256;
  char b[32]; snprintf(b, sizeof b, "queried=%d", dev);
  logf("hipGetDeviceProperties", "neutral", b);
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { logf("hipDeviceSynchronize", "affine"); return hipSuccess; }

hipError_t hipMalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); own(*p); log_size("hipMalloc", n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { use("hipFree", p); disown(p); free(p); logf("hipFree", "affine"); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = calloc(1, n ? n : 1); log_size("hipHostMalloc", n); return hipSuccess; }
hipError_t hipHostFree(void* p) { free(p); logf("hipHostFree", "affine"); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { use("hipMemcpy", d); use("hipMemcpy", s); memmove(d, s, n); log_size("hipMemcpy", n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
  use("hipMemcpyAsync", d); use("hipMemcpyAsync", s); use("hipMemcpyAsync", st);
  if (!g_capture) memmove(d, s, n);
  log_size("hipMemcpyAsync", n, st);
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t st) {
  use("hipMemcpy2DAsync", d); use("hipMemcpy2DAsync", s); use("hipMemcpy2DAsync", st);
  if (!g_capture) for (size_t y = 0; y < h; y++) memmove((char*)d + y * dp, (const char*)s + y * sp, w);
  log_size("hipMemcpy2DAsync", w * h, st);
  return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) { use("hipMemset", d); memset(d, v, n); log_size("hipMemset", n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) { use("hipMemsetAsync", d); use("hipMemsetAsync", st); memset(d, v, n); log_size("hipMemsetAsync", n, st); return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)handle(); own(*s); logf("hipStreamCreateWithFlags", "affine"); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { *s = (hipStream_t)handle(); own(*s); logf("hipStreamCreateWithPriority", "affine"); return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; logf("hipDeviceGetStreamPriorityRange", "affine"); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { use("hipStreamDestroy", s); disown(s); free(s); logf("hipStreamDestroy", "affine"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { use("hipStreamSynchronize", s); log_ptrs("hipStreamSynchronize", "s=%p", s, nullptr); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { use("hipStreamWaitEvent", s); use("hipStreamWaitEvent", e); log_ptrs("hipStreamWaitEvent", "s=%p e=%p", s, e); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)handle(); own(*e); logf("hipEventCreate", "affine"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)handle(); own(*e); logf("hipEventCreateWithFlags", "affine"); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { use("hipEventDestroy", e); disown(e); free(e); logf("hipEventDestroy", "affine"); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { use("hipEventRecord", e); use("hipEventRecord", s); log_ptrs("hipEventRecord", "e=%p s=%p", e, s); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t e) { use("hipEventQuery", e); logf("hipEventQuery", "affine"); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { use("hipEventElapsedTime", a); use("hipEventElapsedTime", b); *ms = 1.0f; logf("hipEventElapsedTime", "affine"); return hipSuccess; }

hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { logf("hipFuncSetAttribute", "affine"); return hipSuccess; }
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { use("launch", s); t_cfg = {g, b, sh, s}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = t_cfg.g; *b = t_cfg.b; *sh = t_cfg.sh; *s = t_cfg.s; return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t sh, hipStream_t s) { use("hipLaunchKernel", s); log_launch("hipLaunchKernel", f, g, b, sh, s); return hipSuccess; }
// the names of the triple-chevron kernels: recorded, then registered with the real runtime (which owns the fat binary these come from)
void __hipRegisterFunction(void** modules, const void* host_fn, char* device_fn, const char* device_name, unsigned limit, void* tid, void* bid, dim3* bdim, dim3* gdim,
                           int* wsize) {
  { std::lock_guard<std::mutex> l(g_mu); g_kernel[host_fn] = device_name; }
  using Fn = void (*)(void**, const void*, char*, const char*, unsigned, void*, void*, dim3*, dim3*, int*);
  static Fn real = (Fn)dlsym(RTLD_NEXT, "__hipRegisterFunction");
  if (real) real(modules, host_fn, device_fn, device_name, limit, tid, bid, bdim, gdim, wsize);
}
hipError_t hipModuleLoadData(hipModule_t* m, const void*) { *m = (hipModule_t)handle(); own(*m); logf("hipModuleLoadData", "affine"); return hipSuccess; }
hipError_t hipModuleUnload(hipModule_t m) { use("hipModuleUnload", m); disown(m); free(m); logf("hipModuleUnload", "affine"); return hipSuccess; }
// BSX_STUB_NO_FUNCTION=<kernel>: that kernel is missing from every module (a code object that lacks one symbol)
hipError_t hipModuleGetFunction(hipFunction_t* f, hipModule_t m, const char* name) {
  use("hipModuleGetFunction", m);
  const char* missing = getenv("BSX_STUB_NO_FUNCTION");
  if (missing && strcmp(missing, name) == 0) { logf("hipModuleGetFunction", "affine", name); return hipErrorNotFound; }
  *f = (hipFunction_t)handle(); own(*f);
  { std::lock_guard<std::mutex> l(g_mu); g_kernel[*f] = name; }
  logf("hipModuleGetFunction", "affine");
  return hipSuccess;
}
hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by, unsigned bz, unsigned sh, hipStream_t s, void**, void**) {
  use("hipModuleLaunchKernel", f); use("hipModuleLaunchKernel", s); log_launch("hipModuleLaunchKernel", f, dim3(gx, gy, gz), dim3(bx, by, bz), sh, s); return hipSuccess;
}

hipError_t hipStreamBeginCapture(hipStream_t s, hipStreamCaptureMode) { use("hipStreamBeginCapture", s); g_capture++; logf("hipStreamBeginCapture", "affine"); return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t s, hipGraph_t* g) { use("hipStreamEndCapture", s); g_capture--; *g = (hipGraph_t)handle(); own(*g); logf("hipStreamEndCapture", "affine"); return hipSuccess; }
hipError_t hipGraphInstantiate(hipGraphExec_t* e, hipGraph_t g, hipGraphNode_t*, char*, size_t) { use("hipGraphInstantiate", g); *e = (hipGraphExec_t)handle(); own(*e); logf("hipGraphInstantiate", "affine"); return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t g) { use("hipGraphDestroy", g); disown(g); free(g); logf("hipGraphDestroy", "affine"); return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t e) { use("hipGraphExecDestroy", e); disown(e); free(e); logf("hipGraphExecDestroy", "affine"); return hipSuccess; }
hipError_t hipGraphLaunch(hipGraphExec_t e, hipStream_t s) { use("hipGraphLaunch", e); use("hipGraphLaunch", s); log_ptrs("hipGraphLaunch", "s=%p", s, nullptr); return hipSuccess; }
}
