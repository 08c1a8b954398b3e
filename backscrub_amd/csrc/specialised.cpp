// specialised.cpp — variant, build and load of the graph-specialised kernels (see specialised.hpp).
#include "specialised.hpp"

#include "debug_switches.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gen_mid.hpp"
#include "gen_seg.hpp"
#include "rtc.hpp"

namespace bsx {

KernelVariant kernel_variant(const Plan& plan) {
  const char* a16 = getenv("BSX_ACT16");
  KernelVariant v;
  v.act16 = a16 && atoi(a16) != 0 && plan.seg.on;
  v.u8in = BSX_DBG_ENV("BSX_F32_INPUT") == nullptr;
  return v;
}

namespace {

// part->source → part->code (hipRTC, or the cache); on failure no code and the note "<what> (hipRTC: <the log, cut at `cut` bytes>)"
bool compile(SpecialisedCode* part, const std::string& arch, const char* what, size_t cut) {
  std::string log;
  if (rtc_build(part->source, arch, &part->code, &log, &part->cached)) return true;
  if (BSX_DBG_ENV("BSX_RTC_DEBUG")) fprintf(stderr, "%s\n", log.c_str());
  part->code.clear();
  part->fallback = std::string(what) + " (hipRTC: " + log.substr(0, cut) + ")";
  return false;
}

// The middle kernel in the form that spills least.  The plain form lets the compiler share every lane-derived value between ops; where that pushes the kernel into
// scratch (MLKit: 352 bytes at 128 registers) the opaque-lane-index form (mid_prelude.hip: tid_now; 92 registers, no scratch) is compiled too and taken if its
// scratch is smaller — read from the code objects' kernel descriptors, so the choice needs no GPU (both code objects sit in the cache).
void build_mid(const Plan& plan, bool act16, const std::string& arch, SpecialisedBuild* b) {
  int force = -1;                                                 // debug build: BSX_RTC_TID=0 | 1 forces the plain / the opaque form (A/B timing)
  if (const char* e = BSX_DBG_ENV("BSX_RTC_TID")) force = atoi(e) != 0;
  auto form = [&](bool opaque, SpecialisedCode* m, long* scratch) {
    m->source = generate_mid_source(plan, &m->why, act16, opaque);
    if (m->source.empty()) { m->fallback = "interpreted (" + m->why + ")"; return false; }
    if (!compile(m, arch, "interpreted", 400)) return false;
    *scratch = code_object_scratch_bytes(m->code, "bsx_mid");
    return true;
  };
  if (!form(force == 1, &b->mid, &b->scratch)) return;
  b->opaque_tid = force == 1;
  if (force >= 0 || b->scratch <= 0) return;
  SpecialisedCode alt;
  long alt_scratch = -1;
  if (form(true, &alt, &alt_scratch) && alt_scratch >= 0 && alt_scratch < b->scratch) { b->mid = std::move(alt); b->scratch = alt_scratch; b->opaque_tid = true; }
}

void build_seg(const Plan& plan, KernelVariant v, const std::string& arch, SpecialisedCode* s) {
  s->source = generate_seg_source(plan, v.act16, v.u8in, &s->why);
  if (BSX_DBG_ENV("BSX_NO_SEG_RTC")) s->fallback = "ahead-of-time kernels (BSX_NO_SEG_RTC)";
  else if (s->source.empty()) s->fallback = "ahead-of-time kernels (" + s->why + ")";
  else compile(s, arch, "ahead-of-time kernels", 600);
}

// hipModuleLoadData, then every kernel of names[0, n) resolved: all or nothing.  On failure the module is unloaded and *mod, fn[] stay as they were.
bool load_module(const std::vector<char>& code, const char* const* names, int n, hipModule_t* mod, hipFunction_t* fn) {
  hipModule_t m = nullptr;
  if (hipModuleLoadData(&m, code.data()) != hipSuccess) { (void)hipGetLastError(); return false; }
  hipFunction_t f[5] = {};
  for (int i = 0; i < n; i++) {
    if (hipModuleGetFunction(&f[i], m, names[i]) != hipSuccess) { (void)hipModuleUnload(m); (void)hipGetLastError(); return false; }
  }
  *mod = m;
  std::copy(f, f + n, fn);
  return true;
}

}  // namespace

SpecialisedBuild build_specialised(const Plan& plan, KernelVariant v, const std::string& arch, unsigned parts) {
  SpecialisedBuild b;
  if (parts & kBuildMid) build_mid(plan, v.act16, arch, &b);
  if (parts & kBuildSeg) build_seg(plan, v, arch, &b.seg);
  b.seg_k3_frame = plan.seg.on && plan.seg.k3f.on;
  return b;
}

void no_specialised(const char* why, SpecialisedKernels* k) {
  k->mid_note = std::string("interpreted (") + why + ")";
  k->seg_note = std::string("ahead-of-time kernels (") + why + ")";
}

void load_specialised(const SpecialisedBuild& b, SpecialisedKernels* k) {
  static const char* const kMid[] = {"bsx_mid"};
  static const char* const kSeg[] = {"bsx_seg_head", "bsx_seg_k2", "bsx_seg_k3", "bsx_seg_tail", "bsx_seg_k3f"};
  k->mid_note = b.mid.fallback;
  if (!b.mid.code.empty()) {
    if (!load_module(b.mid.code, kMid, 1, &k->mid_mod, &k->mid)) k->mid_note = "interpreted (code object did not load)";
    else k->mid_note = std::string("specialised kernel (hipRTC") + (b.mid.cached ? ", from the cache" : ", compiled now") + (b.opaque_tid ? ", lane indices re-derived per op" : "") +
                       (b.scratch > 0 ? ", " + std::to_string(b.scratch) + " B of scratch" : "") + ")";
  }
  k->seg_note = b.seg.fallback;
  if (!b.seg.code.empty()) {
    hipFunction_t fn[5] = {};
    if (!load_module(b.seg.code, kSeg, b.seg_k3_frame ? 5 : 4, &k->seg_mod, fn)) k->seg_note = "ahead-of-time kernels (code object did not load)";
    else {
      std::copy(fn, fn + 4, k->seg);
      k->k3_frame = fn[4];
    }
    if (k->seg_mod) k->seg_note = std::string("specialised kernels (hipRTC") + (b.seg.cached ? ", from the cache)" : ", compiled now)");
  }
}

void unload_specialised(SpecialisedKernels* k) {
  if (k->mid_mod) (void)hipModuleUnload(k->mid_mod);
  if (k->seg_mod) (void)hipModuleUnload(k->seg_mod);
  *k = SpecialisedKernels{};
}

}  // namespace bsx
