// specialised.hpp — the graph-specialised kernels of a plan in one place: which variant, built how, loaded whether.
//
// Two kinds, both compiled by hipRTC for the loaded graph (rtc.cpp, cached on disk): the middle kernel (gen_mid.cpp), whose fallback is the interpreter
// (kernels_frame.hip), and the four segment kernels (gen_seg.cpp: head, k2, k3, tail), whose fallback is the ahead-of-time templates of kernels_seg.hip.
// bsx_new and the bsx_model_* entry points derive the variant and build the code objects here, so bsx_model_precompile fills exactly the cache entries a
// context created under the same environment hits later.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "plan.hpp"

namespace bsx {

// The variant of the specialised kernels a context for `plan` runs, from the plan and the environment.
struct KernelVariant {
  bool act16 = false;   // BSX_ACT16=1 on a segmented plan: 16-bit activation storage at the segment boundaries and in the middle kernel's arena tensors
  bool u8in = false;    // the stems with a byte path read the 8-bit network input (not under the debug build's BSX_F32_INPUT)
};
KernelVariant kernel_variant(const Plan& plan);

// One specialised code object of a plan.
struct SpecialisedCode {
  std::string source;         // the generated source; "" when the generator does not cover the plan (its reason in `why`)
  std::string why;
  std::vector<char> code;     // empty: the fallback runs, for the reason in `fallback` ("interpreted (...)" / "ahead-of-time kernels (...)")
  std::string fallback;
  bool cached = false;        // the code object came from the on-disk cache
};

// The middle kernel (in the form that spills least: plain, or with its lane indices re-derived per op) and the segment code object of `plan` in variant `v`,
// compiled for `arch` or fetched from the cache.  Needs no GPU.  `parts` selects what to build; the segment kernels are built only for a segmented plan.
struct SpecialisedBuild {
  SpecialisedCode mid, seg;
  bool opaque_tid = false;    // the middle kernel's form
  bool seg_k3_frame = false;  // the segment source has bsx_seg_k3f (the plan takes k3's per-frame form)
  long scratch = -1;          // the middle kernel's scratch bytes per lane, from its kernel descriptor (-1: unreadable)
};
enum : unsigned { kBuildMid = 1, kBuildSeg = 2 };
SpecialisedBuild build_specialised(const Plan& plan, KernelVariant v, const std::string& arch, unsigned parts = kBuildMid | kBuildSeg);

// The specialised kernels a context loaded.  A null function means its fallback runs; the segment kernels are loaded all four or none.
struct SpecialisedKernels {
  hipModule_t mid_mod = nullptr, seg_mod = nullptr;
  hipFunction_t mid = nullptr;
  hipFunction_t seg[4] = {};      // bsx_seg_head, bsx_seg_k2, bsx_seg_k3, bsx_seg_tail
  hipFunction_t k3_frame = nullptr;   // bsx_seg_k3f: part of the segment module where the plan takes k3's per-frame form (SegPlan::k3f.on), loaded with the four or not at all
  std::string mid_note, seg_note; // plan(): "program execution: <mid_note>", "segment execution: <seg_note>"
};
// Nothing specialised, for `why` (BSX_NO_RTC, no device properties).
void no_specialised(const char* why, SpecialisedKernels* k);
// Load what `b` holds on the current device.  Never an error: a code object that does not load, or lacks one of its kernels, is unloaded and the fallback runs.
void load_specialised(const SpecialisedBuild& b, SpecialisedKernels* k);
void unload_specialised(SpecialisedKernels* k);

}  // namespace bsx
