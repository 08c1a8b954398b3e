"""Generate tests/golden/ref_pin_digests.json — what the reference's own object code (oracle/_ref/libbs_ref.so) computes on the
inputs of tests/test_ref_pin.py, as digests, so that those tests pin the oracle where the library cannot be built.

Runs every case of the test module with the live library, the oracle-side assertions included: a recording is only written when
the oracle agrees with the reference on every case.

    python tools/make_ref_pin.py       # rewrites the digest file (needs oracle/_ref/libbs_ref.so or a reference checkout)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_ref_pin as T  # noqa: E402
from oracle import ref_py  # noqa: E402


def record():
    if not ref_py.available():
        sys.exit("oracle/_ref/libbs_ref.so is absent and there is no reference checkout to build it from")
    T._RECORDING = {}
    for key, w, h in T.GEOMS:
        T.test_whole_process_matches_reference_object_code(key, w, h)
    T.test_whole_process_deeplab_one_frame()
    for key in T.DECODE_KEYS:
        T.test_decode_and_iir_match_reference_loops(key)
    for args in T.TCONV:
        T.test_transpose_conv_bias_matches_reference_op(*args)
    T.test_alpha_blend_all_byte_triples_match_reference()
    for w, h in T.YUYV:
        T.test_yuyv_packing_matches_reference(w, h)
    rec, T._RECORDING = T._RECORDING, None
    with open(T.RECORDED, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return rec


if __name__ == "__main__":
    print("%d cases -> %s" % (len(record()), T.RECORDED))
