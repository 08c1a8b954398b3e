import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


REFERENCE_MODELS = os.path.join(ROOT, "tests", "golden", "reference_models")


def _real_models():
    return sorted(p for p in (reference_model_path(k) for k in MODEL_KEYS) if os.path.exists(p))


MODEL_KEYS = {
    "lite": "segm_lite_v681.tflite",
    "full": "segm_full_v679.tflite",
    "mlkit": "selfiesegmentation_mlkit-256x256-2021_01_19-v1215.f16.tflite",
    "deeplab": "deeplabv3_257_mv_gpu.tflite",
}


def reference_model_path(key):
    """The reference's real .tflite: the test fixture under tests/golden/reference_models (the Meet and MLKit models; DeepLab's
    2.7 MB file is not kept in the repository), else a copy staged into models/ by tools/stage_models.py from a reference checkout."""
    fixture = os.path.join(REFERENCE_MODELS, MODEL_KEYS[key])
    return fixture if os.path.exists(fixture) else os.path.join(ROOT, "models", MODEL_KEYS[key])


def model_path(key, prefer_real=True):
    """Path of a model for tests: the reference's real .tflite (reference_model_path), else the synthetic
    same-architecture model with seeded random weights under tests/golden/models."""
    real = reference_model_path(key)
    if prefer_real and os.path.exists(real):
        return real
    return synthetic_model_path(key)


def synthetic_model_path(key):
    from tools import make_synthetic_model
    return make_synthetic_model.ensure(key)


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


@pytest.fixture
def debug_switches(monkeypatch):
    """The A/B knobs, alternate code paths and work-skipping experiments (csrc/debug_switches.hpp) are compiled out of libbsx.so; tests that cross-check an
    alternate path against the default one run against libbsx_dbg.so (same sources, -DBSX_DEBUG_SWITCHES; built by backscrub_amd/build.py).  For the duration of the
    test the Python binding is re-pointed at it; contexts must be closed inside the test."""
    from backscrub_amd import api, build
    if not os.path.exists(build.LIB_DBG):
        pytest.fail("libbsx_dbg.so is missing: run `python -m backscrub_amd.build`")
    saved = api._LIB
    api._LIB = None
    monkeypatch.setenv("BSX_LIBRARY", build.LIB_DBG)
    api.lib()
    yield api
    api._LIB = saved
