"""CPU-side checks of the device-objective surface (no GPU compute): the new names are declared with
the documented prototypes, exported by the library and bound by the Python layer, and the reducer
reports a missing device as an error code."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-lbfgs_amd")
sys.path.insert(0, PKG)
import lbfgs_amd as L  # noqa: E402

PROTOTYPES = {
    "lbfgs_set_device_objective": "int lbfgs_set_device_objective(lbfgs_ctx* ctx, const lbfgs_device_fn* fn);",
    "lbfgs_minimize_device":
        "int lbfgs_minimize_device(lbfgs_ctx* ctx, int objective, const lbfgs_host_fn* cb, int line_search, "
        "const lbfgs_constants* k, const double* x0_dev, double* x_out_dev, int max_iterations, double tolerance, "
        "unsigned flags, lbfgs_result* out);",
    "lbfgs_solver_init_device":
        "int lbfgs_solver_init_device(lbfgs_ctx* ctx, int objective, const lbfgs_host_fn* cb, int line_search, "
        "const lbfgs_constants* k, const double* x0_dev, double tolerance, unsigned flags);",
    "lbfgs_get_x_device": "int lbfgs_get_x_device(lbfgs_ctx* ctx, double* x_out_dev);",
    "lbfgs_reducer_create": "int lbfgs_reducer_create(lbfgs_reducer** out, int64_t n, int device);",
    "lbfgs_reducer_destroy": "void lbfgs_reducer_destroy(lbfgs_reducer* r);",
    "lbfgs_reducer_dot":
        "int lbfgs_reducer_dot(lbfgs_reducer* r, const double* a_dev, const double* b_dev, void* hip_stream, "
        "double* out_host);",
}


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


def _header():
    src = open(os.path.join(ROOT, "include", "lbfgs_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)  # comments out
    return re.sub(r"\s+", " ", src)


def test_header_declares_the_prototypes():
    h = _header()
    for name, proto in PROTOTYPES.items():
        assert proto in h, name
    assert "#define LBFGS_HIP_ABI_VERSION 3 " in h
    assert re.search(r"LBFGS_OBJ_DEVICE = 5\b", h)
    assert "#define LBFGS_DEVICE_EAGER_GRAD 1u " in h
    assert ("typedef int (*lbfgs_device_eval)(const double* x_dev, int64_t n, double* f_out, double* g_dev, "
            "void* user);") in h
    assert re.search(r"typedef struct \{ lbfgs_device_eval eval; void\* user; unsigned flags; \} lbfgs_device_fn;", h)
    assert "typedef struct lbfgs_reducer lbfgs_reducer;" in h
    # additions only: the ids before it keep their values
    for name, v in [("ROSENBROCK", 0), ("QUAD_TRIDIAG", 1), ("QUAD_SEPARABLE", 2), ("HOST", 3), ("DENSE_QUAD", 4)]:
        assert re.search(rf"LBFGS_OBJ_{name} = {v}\b", h), name


def test_library_and_binding_have_the_names():
    _ensure_built()
    lib = ctypes.CDLL(L.LIB_PATH)
    bound = L.lib()
    for s in PROTOTYPES:
        assert hasattr(lib, s), s
        assert s in L.EXPORTED_SYMBOLS, s
        nargs = PROTOTYPES[s].split("(", 1)[1].count(",") + 1
        assert len(getattr(bound, s).argtypes) == nargs, s
    assert L.OBJECTIVES["device"] == 5
    assert L.OBJECTIVES == {"rosenbrock": 0, "quad_tridiag": 1, "quad_sep": 2, "host": 3, "dense": 4, "device": 5}
    assert L.DEVICE_EAGER_GRAD == 1
    assert ctypes.sizeof(L.DeviceFn) == 3 * ctypes.sizeof(ctypes.c_void_p)  # eval, user, flags + padding
    for m in ("set_device_objective", "minimize_device", "init_device", "get_x_device"):
        assert callable(getattr(L.Context, m)), m
    assert callable(L.Reducer.dot) and callable(L.Reducer.sum)


def test_reducer_create_bad_arguments():
    _ensure_built()
    h = ctypes.c_void_p()
    for n, dev in [(0, 0), (-5, 0), (1000, -1)]:
        assert L.lib().lbfgs_reducer_create(ctypes.byref(h), n, dev) == -1  # LBFGS_ERR_BAD_ARG
        assert not h.value
    assert L.lib().lbfgs_reducer_create(None, 1000, 0) == -1
    L.lib().lbfgs_reducer_destroy(None)  # a no-op


def test_reducer_create_without_a_device_is_an_error_code():
    """No device (or an ordinal past the last one): an error code and no object, not a crash."""
    _ensure_built()
    count = L.device_count()
    h = ctypes.c_void_p()
    rc = L.lib().lbfgs_reducer_create(ctypes.byref(h), 1000, count)  # one past the last device
    assert rc == -2 and not h.value  # LBFGS_ERR_HIP


def _run(code):
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_import_order_with_torch_is_diagnosed():
    """A torch wheel that brings its own HIP runtime shares device memory with the library only when
    both are on one copy of it: torch imported first, the library binds to torch's copy; the other
    order maps two copies and the torch entry points say so instead of failing later. (No GPU is
    touched: the check reads the process's mappings. A torch built on the system runtime has one
    copy either way.)"""
    _ensure_built()
    pre = f"import sys; sys.path.insert(0, {PKG!r}); "
    first = _run(pre + "import torch, lbfgs_amd as L; L._torch(); print(len(L.hip_runtimes()))")
    assert first.returncode == 0 and first.stdout.strip() == "1", first.stdout + first.stderr
    late = _run(pre + "import lbfgs_amd as L; L.lib(); n0 = len(L.hip_runtimes()); import torch\n"
                      "try:\n    L.Reducer(8); print('created')\n"
                      "except L.LbfgsError as e:\n    print('refused' if 'import torch before' in str(e) else e)\n"
                      "print(n0, len(L.hip_runtimes()))")
    assert late.returncode == 0, late.stdout + late.stderr
    out = late.stdout.split()
    assert out[1] == "1", late.stdout  # the library alone: one runtime
    # two copies mapped: refused with the advice; one shared copy: nothing to refuse (no device here)
    assert (out[2] == "1") or out[0] == "refused", late.stdout
