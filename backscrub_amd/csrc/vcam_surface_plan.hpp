// The item checks of bsx_step_batch_surfaces: what concerns one NV12 input surface alone.  Plain C++ on host memory — no HIP type, no context — like
// vcam_nv12_plan.hpp, so a stand-alone program can drive it (tests/test_surfaces_host.py does, under the host sanitizers).  The output records of the call are
// vcam_nv12_plan's, unchanged.
//   vcam_surface_class   is a class admitted for NV12 items?  The proper INTER_LINEAR down-scale table (ResizeTab::mode 0), an even width and height, a width of at
//                        least 4 (the prep kernel's 4-byte windows).  Chroma is addressed by the frame's column and row, so the ROI's parity is free;
//   vcam_surface_item    the setting bits, the two planes, the two pitches, the background where it is read;
//   a plane's extent     vcam_nv12_extent(pitch, rows, W) (vcam_nv12_plan.hpp): what the overlap test of bsx_api.hip judges an input plane on.
// Both return true, or false with a text that names items[i] and the value.
#pragma once
#include "vcam_nv12_plan.hpp"

namespace bsx {
constexpr unsigned kSurfaceStreamFlags = BSX_STEP_FLIP_H | BSX_STEP_FLIP_V | BSX_STREAM_FILTER_OFF;
struct SurfaceRefusal { char text[320] = {0}; };

// item i is stream `id` of class g (W x H, down-scale table mode tab_mode)
inline bool vcam_surface_class(int i, int id, int g, int W, int H, int tab_mode, int roi_w, int roi_h, SurfaceRefusal* r) {
  char why[160];
  if (tab_mode == 1) snprintf(why, sizeof why, "its down-scale table is a copy (capture ROI %d x %d = model ROI)", roi_w, roi_h);
  else if (tab_mode == 2) snprintf(why, sizeof why, "its down-scale table is the 2x2 area mean (capture ROI %d x %d = twice the model ROI)", roi_w, roi_h);
  else if (tab_mode != 0) snprintf(why, sizeof why, "its down-scale table has mode %d", tab_mode);
  else if ((W | H) & 1) snprintf(why, sizeof why, "NV12 needs an even width and height");
  else if (W < 4) snprintf(why, sizeof why, "the width %d is below 4", W);
  else return true;
  snprintf(r->text, sizeof r->text, "items[%d]: stream %d is of class %d (%d x %d), which has no fused NV12 prep: %s; convert such surfaces with bsx_nv12_to_bgr", i, id, g, W, H, why);
  return false;
}

inline bool vcam_surface_item(const bsx_surface_item& it, int i, int W, int H, SurfaceRefusal* r) {
#define BSX_VS_REFUSE(...) do { snprintf(r->text, sizeof r->text, __VA_ARGS__); return false; } while (0)
  const unsigned f = it.setting.flags;
  if (f & 0xFF00u) BSX_VS_REFUSE("items[%d]: setting flags 0x%x asks for a background blur, which the multi-geometry step does not take", i, f);
  if (f & BSX_STREAM_YUYV_IN) BSX_VS_REFUSE("items[%d]: setting flags 0x%x has the yuyv-in bit: every frame of this call is an NV12 surface", i, f);
  if (f & ~kSurfaceStreamFlags) BSX_VS_REFUSE("items[%d]: setting flags 0x%x has bits outside flip / filter-off", i, f);
  if (!it.d_y) BSX_VS_REFUSE("items[%d]: d_y is NULL", i);
  if ((uintptr_t)it.d_y & 3) BSX_VS_REFUSE("items[%d]: d_y %p is not 4-byte aligned", i, (const void*)it.d_y);
  if (!it.d_uv) BSX_VS_REFUSE("items[%d]: d_uv is NULL", i);
  if ((uintptr_t)it.d_uv & 3) BSX_VS_REFUSE("items[%d]: d_uv %p is not 4-byte aligned", i, (const void*)it.d_uv);
  if (it.pitch_y < W) BSX_VS_REFUSE("items[%d]: pitch_y = %d is below the width %d of its class", i, it.pitch_y, W);
  if (it.pitch_y & 3) BSX_VS_REFUSE("items[%d]: pitch_y = %d is not a multiple of 4", i, it.pitch_y);
  if (it.pitch_uv < W) BSX_VS_REFUSE("items[%d]: pitch_uv = %d is below the width %d of its class", i, it.pitch_uv, W);
  if (it.pitch_uv & 3) BSX_VS_REFUSE("items[%d]: pitch_uv = %d is not a multiple of 4", i, it.pitch_uv);
  if ((unsigned long long)it.pitch_y * (unsigned long long)H >= (1ull << 31) || (unsigned long long)it.pitch_uv * (unsigned long long)(H / 2) >= (1ull << 31))
    BSX_VS_REFUSE("items[%d]: pitch_y = %d, pitch_uv = %d at %d rows: a plane of 2 GiB or more", i, it.pitch_y, it.pitch_uv, H);
  if (!(f & BSX_STREAM_FILTER_OFF)) {                                // (filter off: reads no background)
    if (!it.setting.d_bg) BSX_VS_REFUSE("items[%d]: setting.d_bg is NULL", i);
    if ((uintptr_t)it.setting.d_bg & 3) BSX_VS_REFUSE("items[%d]: setting.d_bg %p is not 4-byte aligned", i, (const void*)it.setting.d_bg);
  }
#undef BSX_VS_REFUSE
  return true;
}
}  // namespace bsx
