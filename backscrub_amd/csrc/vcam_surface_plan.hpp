// The item checks of bsx_step_batch_surfaces — vcam_surface_item, vcam_surface_class, SurfaceRefusal — live in geoms_request.hpp with the rules they share with the
// other multi-geometry steps.  This header keeps their earlier name for a program that includes it (tests/test_surfaces_host.py drives them stand-alone).
#pragma once
#include "geoms_request.hpp"
