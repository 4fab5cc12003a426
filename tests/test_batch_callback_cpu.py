"""CPU-side checks of the batch's caller-supplied objective (no GPU): the typedefs and the prototype in
the public header, the unchanged ABI version, the exported name, the refusal of a NULL batch, and the
method of Batch."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-lbfgs_amd")
sys.path.insert(0, PKG)
import lbfgs_amd as L  # noqa: E402

NAME = "lbfgs_batch_set_device_objective"
BAD_ARG = -1


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


def test_prototypes_in_the_header_and_abi_version():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "lbfgs_hip.h")).read())
    assert ("typedef int (*lbfgs_batch_device_eval)(const double* z_dev, int64_t ldz, double* f_dev, double* g_dev, "
            "int64_t ldg, const int* active_dev, int n_active, int batch, int64_t n, void* user);") in src
    assert "typedef struct { lbfgs_batch_device_eval eval; void* user; unsigned flags; /* 0 */ } lbfgs_batch_device_fn;" in src
    assert "int lbfgs_batch_set_device_objective(lbfgs_batch* b, const lbfgs_batch_device_fn* fn);" in src
    assert "#define LBFGS_HIP_ABI_VERSION 3 " in src


def test_name_exported():
    _ensure_built()
    lib = ctypes.CDLL(L.LIB_PATH)
    assert NAME in L.EXPORTED_SYMBOLS
    assert hasattr(lib, NAME)


def test_null_batch_is_bad_arg():
    _ensure_built()
    fn = L.BatchDeviceFn(L.BATCH_DEVICE_EVAL(lambda *a: 0), None, 0)
    assert L.lib().lbfgs_batch_set_device_objective(None, ctypes.byref(fn)) == BAD_ARG
    assert L.lib().lbfgs_batch_set_device_objective(None, None) == BAD_ARG


def test_batch_has_the_method_and_the_binding_matches_the_header():
    assert callable(getattr(L.Batch, "set_device_objective", None))
    assert [f[0] for f in L.BatchDeviceFn._fields_] == ["eval", "user", "flags"]
    # z_dev, ldz, f_dev, g_dev, ldg, active_dev, n_active, batch, n, user
    assert L.BATCH_DEVICE_EVAL._argtypes_ == (ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int64, ctypes.c_void_p)
    assert L.BATCH_DEVICE_EVAL._restype_ is ctypes.c_int
