"""The segment kernels' text as the compiler sees it: csrc/kernels_seg.hip with its local includes (seg_gate.inc, seg_gated_row.inc, seg_k3_rows.inc: bodies that several
kernels share) spliced in place — for the tests that evaluate the kernels' own index expressions (test_lds_layouts, test_k2_staging, test_k3_frame_codegen)."""
import functools
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "backscrub_amd", "csrc")


@functools.lru_cache(None)
def seg_kernel_text(name="kernels_seg.hip"):
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r'^[ \t]*#include "(\w+\.inc)"[ \t]*$', lambda m: seg_kernel_text(m.group(1)), text, flags=re.M)
