"""Python binding of liblbfgs_hip.so (include/lbfgs_hip.h) — the MI355X L-BFGS solver.

The shared library is the product: HIP kernels for gfx950 plus the C host driver. This module
is a thin ctypes layer for tests and benchmarks; it never computes anything itself and raises
if the library is missing (there is no CPU fallback).

    import lbfgs_amd as L
    with L.Context(n=10**8, m=10) as ctx:
        res = ctx.minimize("rosenbrock", x0, "backtracking", max_iterations=100)
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LBFGS_LIB") or os.path.join(HERE, "liblbfgs_hip.so")  # LBFGS_LIB: A/B builds

OBJECTIVES = {"rosenbrock": 0, "quad_tridiag": 1, "quad_sep": 2, "host": 3, "dense": 4, "device": 5}
LINE_SEARCHES = {"backtracking": 0, "interpolation": 1, "wolfe": 2, "backtracking_wolfe": 3}
STATUS = {0: "converged", 1: "max_iter", 2: "ls_failed", 3: "running"}
FLAG_VERBOSE, FLAG_QUIET, FLAG_TRACE, FLAG_UNFUSED, FLAG_VECTOR_FREE = 1, 2, 4, 8, 16
FLAG_REFERENCE_CALLS = 32
FLAG_CUDA_COMPAT = 64
DEVICE_EAGER_GRAD = 1  # lbfgs_device_fn.flags: every device-callback call asks for f and grad together
FLAG_CUDA_VARIANT = 128  # LBFGS_CUDA's semantics (parallel-implementation/L-BFGS.cu), include/lbfgs_hip.h
KERNELS = ["dot", "axpy_dot", "mid", "axpy2_dot", "last", "negdot", "eval", "trial_f",
           "trial_fg", "commit", "point", "checksum", "update", "vf_commit", "vf_dir", "small_iter",
           "group_reduce", "exchange"]


class LbfgsError(RuntimeError):
    pass


class Constants(C.Structure):
    _fields_ = [("c1", C.c_double), ("c2", C.c_double), ("initial_step", C.c_double),
                ("backtracking_alpha", C.c_double), ("backtracking_tol", C.c_double),
                ("wolfe_interp_min", C.c_double), ("wolfe_interp_max", C.c_double)]


class Result(C.Structure):
    _fields_ = [("iterations", C.c_int), ("status", C.c_int), ("f", C.c_double),
                ("gnorm", C.c_double), ("trials_f", C.c_int64), ("trials_fg", C.c_int64),
                ("commits", C.c_int64), ("passes", C.c_int64), ("bytes", C.c_double),
                ("seconds", C.c_double), ("h_min", C.c_int), ("h_max", C.c_int),
                ("f_calls", C.c_int64), ("grad_calls", C.c_int64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["status"] = STATUS.get(self.status, self.status)
        return d


class BatchEvents(C.Structure):
    _fields_ = [("not_descent", C.c_int), ("skipped_updates", C.c_int), ("invalid_rho", C.c_int),
                ("invalid_gamma", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


HOST_F = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int64, C.c_void_p)
HOST_G = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.c_void_p)


class HostFn(C.Structure):
    _fields_ = [("f", HOST_F), ("grad", HOST_G), ("user", C.c_void_p)]


# int eval(const double* x_dev, int64_t n, double* f_out, double* g_dev, void* user)
DEVICE_EVAL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.c_void_p, C.c_void_p)


class DeviceFn(C.Structure):
    _fields_ = [("eval", DEVICE_EVAL), ("user", C.c_void_p), ("flags", C.c_uint)]


# int eval(const double* z_dev, int64_t ldz, double* f_dev, double* g_dev, int64_t ldg, const int* active_dev,
#          int n_active, int batch, int64_t n, void* user)
BATCH_DEVICE_EVAL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                C.c_int, C.c_int64, C.c_void_p)


class BatchDeviceFn(C.Structure):
    _fields_ = [("eval", BATCH_DEVICE_EVAL), ("user", C.c_void_p), ("flags", C.c_uint)]


_lib = None


def lib():
    """Load liblbfgs_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LbfgsError(f"{LIB_PATH} not built: run `make -C cuda-lbfgs_amd` "
                         "(or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    vp = C.c_void_p
    L.lbfgs_ctx_create.argtypes = [C.POINTER(vp), C.c_int64, C.c_int, C.c_int]
    L.lbfgs_ctx_create_sharded.argtypes = [C.POINTER(vp), C.c_int64, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_char_p]
    L.lbfgs_unique_id.argtypes = [C.c_char_p]
    L.lbfgs_device_count.argtypes = []
    L.lbfgs_host_group_create.argtypes = [C.POINTER(vp), C.c_int]
    L.lbfgs_host_group_destroy.argtypes = [vp]
    L.lbfgs_host_group_destroy.restype = None
    L.lbfgs_ctx_create_emulated.argtypes = [C.POINTER(vp), C.c_int64, C.c_int, C.c_int, C.c_int, vp]
    L.lbfgs_ctx_destroy.argtypes = [vp]
    L.lbfgs_ctx_destroy.restype = None
    L.lbfgs_last_error.argtypes = [vp]
    L.lbfgs_last_error.restype = C.c_char_p
    L.lbfgs_local_range.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lbfgs_shard_range.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64)]
    L.lbfgs_constants_default.argtypes = [C.POINTER(Constants)]
    L.lbfgs_constants_default.restype = None
    L.lbfgs_constants_cuda.argtypes = [C.POINTER(Constants)]
    L.lbfgs_constants_cuda.restype = None
    L.lbfgs_minimize.argtypes = [vp, C.c_int, C.POINTER(HostFn), C.c_int, C.POINTER(Constants),
                                 dp, dp, C.c_int, C.c_double, C.c_uint, C.POINTER(Result)]
    L.lbfgs_solver_init.argtypes = [vp, C.c_int, C.POINTER(HostFn), C.c_int,
                                    C.POINTER(Constants), dp, C.c_double, C.c_uint]
    L.lbfgs_solver_step.argtypes = [vp, C.c_int, C.POINTER(Result)]
    L.lbfgs_get_x.argtypes = [vp, dp]
    L.lbfgs_sync.argtypes = [vp]
    L.lbfgs_messages.argtypes = [vp, C.c_char_p, C.c_int]
    L.lbfgs_trace_len.argtypes = [vp]
    L.lbfgs_trace_enable.argtypes = [vp, C.c_int]
    L.lbfgs_trace_get.argtypes = [vp, dp, dp, dp, np.ctypeslib.ndpointer(dtype=np.uint64),
                                  np.ctypeslib.ndpointer(dtype=np.uint64), C.c_int]
    L.lbfgs_dev_dot.argtypes = [vp, dp, dp, C.POINTER(C.c_double)]
    L.lbfgs_dev_norm.argtypes = [vp, dp, C.POINTER(C.c_double)]
    L.lbfgs_dev_objective.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_double), vp]
    L.lbfgs_dev_trial.argtypes = [vp, C.c_int, dp, dp, C.c_double, C.POINTER(C.c_double), vp,
                                  C.POINTER(C.c_double)]
    L.lbfgs_dev_twoloop.argtypes = [vp, dp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                    dp, C.POINTER(C.c_double)]
    L.lbfgs_peer_handle.argtypes = [vp, C.c_char_p]
    L.lbfgs_peer_connect.argtypes = [vp, C.c_char_p]
    L.lbfgs_peer_enable.argtypes = [vp, C.c_int]
    L.lbfgs_rccl_attach.argtypes = [vp, C.c_char_p]
    L.lbfgs_exchange_backend.argtypes = [vp]
    L.lbfgs_exchange_fold.argtypes = [vp]
    L.lbfgs_exchange_latency.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.lbfgs_spec_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lbfgs_search_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lbfgs_cu_partition.argtypes = [vp]
    L.lbfgs_coop_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lbfgs_wait_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.lbfgs_vector_fallbacks.argtypes = [vp]
    L.lbfgs_vector_pool.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.lbfgs_stream_probe.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.lbfgs_stream_probe_variant.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.lbfgs_stream_probe_vectors.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.lbfgs_vector_address.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64)]
    L.lbfgs_prof_enable.argtypes = [vp, C.c_int]
    L.lbfgs_prof_enable.restype = None
    L.lbfgs_prof_reset.argtypes = [vp]
    L.lbfgs_prof_reset.restype = None
    L.lbfgs_prof_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                 C.POINTER(C.c_double)]
    L.lbfgs_batch_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.lbfgs_batch_create.argtypes = [C.POINTER(vp), C.c_int64, C.c_int, C.c_int, C.c_int]
    L.lbfgs_batch_destroy.argtypes = [vp]
    L.lbfgs_batch_destroy.restype = None
    L.lbfgs_batch_last_error.argtypes = [vp]
    L.lbfgs_batch_last_error.restype = C.c_char_p
    L.lbfgs_batch_set_launch.argtypes = [vp, C.c_int, C.c_int]
    L.lbfgs_batch_minimize.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Constants), dp, dp, C.c_int, C.c_double,
                                       C.c_uint, C.POINTER(Result)]
    L.lbfgs_batch_trace_len.argtypes = [vp, C.c_int]
    L.lbfgs_batch_trace_get.argtypes = [vp, C.c_int, dp, dp, dp, C.c_int]
    L.lbfgs_batch_events_get.argtypes = [vp, C.c_int, C.POINTER(BatchEvents)]
    L.lbfgs_batch_dense_plan.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.lbfgs_batch_set_dense_quadratics.argtypes = [vp, vp, C.c_int, vp]
    L.lbfgs_batch_minimize_device.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Constants), vp, C.c_int64, vp, C.c_int64,
                                              C.c_int, C.c_double, C.c_uint, C.POINTER(Result)]
    L.lbfgs_batch_set_dense_quadratics_device.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, C.c_int64]
    L.lbfgs_batch_ragged_plan.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.lbfgs_batch_create_ragged.argtypes = [C.POINTER(vp), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int]
    L.lbfgs_batch_sizes.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lbfgs_batch_set_device_objective.argtypes = [vp, C.POINTER(BatchDeviceFn)]
    L.lbfgs_set_device_objective.argtypes = [vp, C.POINTER(DeviceFn)]
    L.lbfgs_minimize_device.argtypes = [vp, C.c_int, C.POINTER(HostFn), C.c_int, C.POINTER(Constants),
                                        vp, vp, C.c_int, C.c_double, C.c_uint, C.POINTER(Result)]
    L.lbfgs_solver_init_device.argtypes = [vp, C.c_int, C.POINTER(HostFn), C.c_int, C.POINTER(Constants),
                                           vp, C.c_double, C.c_uint]
    L.lbfgs_get_x_device.argtypes = [vp, vp]
    L.lbfgs_reducer_create.argtypes = [C.POINTER(vp), C.c_int64, C.c_int]
    L.lbfgs_reducer_destroy.argtypes = [vp]
    L.lbfgs_reducer_destroy.restype = None
    L.lbfgs_reducer_dot.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double)]
    L.lbfgs_reduce_rows.argtypes = [C.c_int, C.c_int64, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, vp]
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "lbfgs_constants_default", "lbfgs_constants_cuda", "lbfgs_ctx_create",
    "lbfgs_ctx_create_sharded", "lbfgs_unique_id", "lbfgs_host_group_create",
    "lbfgs_host_group_destroy", "lbfgs_ctx_create_emulated", "lbfgs_ctx_destroy", "lbfgs_last_error",
    "lbfgs_local_range", "lbfgs_shard_range", "lbfgs_minimize", "lbfgs_solver_init", "lbfgs_solver_step",
    "lbfgs_get_x", "lbfgs_sync", "lbfgs_messages", "lbfgs_trace_len", "lbfgs_trace_get",
    "lbfgs_trace_enable",
    "lbfgs_dev_dot", "lbfgs_dev_norm", "lbfgs_dev_objective", "lbfgs_dev_trial",
    "lbfgs_dev_twoloop", "lbfgs_dev_elementwise", "lbfgs_line_search", "lbfgs_prof_enable",
    "lbfgs_prof_reset", "lbfgs_prof_get", "lbfgs_peer_handle", "lbfgs_peer_connect", "lbfgs_peer_enable", "lbfgs_rccl_attach",
    "lbfgs_exchange_backend", "lbfgs_exchange_fold", "lbfgs_exchange_latency", "lbfgs_device_count", "lbfgs_set_dense_quadratic", "lbfgs_build_info",
    "lbfgs_spec_stats", "lbfgs_cu_partition", "lbfgs_stream_probe", "lbfgs_stream_probe_variant", "lbfgs_stream_probe_vectors", "lbfgs_vector_address", "lbfgs_coop_info", "lbfgs_wait_stats", "lbfgs_vector_fallbacks", "lbfgs_vector_pool", "lbfgs_search_stats",
    "lbfgs_batch_plan", "lbfgs_batch_create", "lbfgs_batch_destroy", "lbfgs_batch_last_error",
    "lbfgs_batch_set_launch", "lbfgs_batch_minimize", "lbfgs_batch_trace_len", "lbfgs_batch_trace_get",
    "lbfgs_batch_events_get", "lbfgs_batch_dense_plan", "lbfgs_batch_set_dense_quadratics",
    "lbfgs_batch_minimize_device", "lbfgs_batch_set_dense_quadratics_device",
    "lbfgs_batch_ragged_plan", "lbfgs_batch_create_ragged", "lbfgs_batch_sizes", "lbfgs_batch_set_device_objective",
    "lbfgs_set_device_objective", "lbfgs_minimize_device", "lbfgs_solver_init_device", "lbfgs_get_x_device",
    "lbfgs_reducer_create", "lbfgs_reducer_destroy", "lbfgs_reducer_dot", "lbfgs_reduce_rows",
]
PEER_HANDLE_BYTES = 64
BACKENDS = {0: "single", 1: "rccl", 2: "xgmi", 3: "host-group"}


def constants(profile="config"):
    k = Constants()
    (lib().lbfgs_constants_cuda if profile == "cuda" else lib().lbfgs_constants_default)(C.byref(k))
    return k


def shard_range(n, rank, world):
    """(elem_lo, n_loc) of `rank` when n is sharded over `world` ranks (no device needed)."""
    lo, nl = C.c_int64(), C.c_int64()
    rc = lib().lbfgs_shard_range(int(n), int(rank), int(world), C.byref(lo), C.byref(nl))
    if rc != 0:
        raise LbfgsError(f"cannot shard n={n} over {world} ranks")
    return lo.value, nl.value


def build_info():
    """(the library's embedded build string, the source hash of this tree, match?): a library
    built from other sources than the ones beside it is stale."""
    lib().lbfgs_build_info.restype = C.c_char_p
    info = lib().lbfgs_build_info().decode()
    return info, source_hash(), info.startswith("src=" + source_hash() + " ")


def source_hash():
    """sha256 over the library's sources, in cuda-lbfgs_amd/Makefile's SRC_HASH order."""
    import glob
    import hashlib

    here = os.path.dirname(os.path.abspath(__file__))
    rel = []
    for pat in ("csrc/*.hip", "csrc/*.h", "csrc/*.c", "csrc/*.cpp", "../include/*.h"):
        rel += glob.glob(pat, root_dir=here)
    h = hashlib.sha256()
    for r in sorted(set(rel)):
        with open(os.path.join(here, r), "rb") as fp:
            h.update(fp.read())
    return h.hexdigest()[:16]


def device_count():
    return int(lib().lbfgs_device_count())


def unique_id():
    buf = C.create_string_buffer(128)
    rc = lib().lbfgs_unique_id(buf)
    if rc != 0:
        raise LbfgsError(f"lbfgs_unique_id failed ({rc})")
    return buf.raw


def x0_uniform(n, seed=42, lo=-2.0, hi=2.0):
    """x0 exactly as std::mt19937(seed) + std::uniform_real_distribution<double>(lo, hi)
    (libstdc++: generate_canonical<double,53> from two 32-bit draws), main.cpp:36-43."""
    rs = np.random.RandomState(seed)  # MT19937 with init_genrand(seed) == std::mt19937(seed)
    out = np.empty(n, dtype=np.float64)
    chunk = 1 << 22
    for s in range(0, n, chunk):
        k = min(chunk, n - s)
        raw = rs.randint(0, 1 << 32, size=2 * k, dtype=np.uint64).reshape(k, 2).astype(np.float64)
        u = (raw[:, 0] + raw[:, 1] * 4294967296.0) / 18446744073709551616.0
        u[u >= 1.0] = np.nextafter(1.0, 0.0)
        out[s:s + k] = u * (hi - lo) + lo
    return out


class HostGroup:
    """Exchange group for emulated ranks (threads of one process, e.g. on one GPU)."""

    def __init__(self, world):
        h = C.c_void_p()
        rc = lib().lbfgs_host_group_create(C.byref(h), int(world))
        if rc != 0:
            raise LbfgsError(f"lbfgs_host_group_create failed ({rc})")
        self.h, self.world = h, int(world)

    def close(self):
        if getattr(self, "h", None):
            lib().lbfgs_host_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan(n, m, batch):
    """Device bytes a Batch(n, m, batch) would take (no device needed); raises LbfgsError when
    (n, m, batch) is outside the batched solver's limits (lbfgs_batch_plan)."""
    b = C.c_double()
    rc = lib().lbfgs_batch_plan(int(n), int(m), int(batch), C.byref(b))
    if rc != 0:
        e = LbfgsError(f"lbfgs_batch_plan({n}, {m}, {batch}) failed ({rc}): 1 <= n <= 32768, 1 <= m <= 16, batch >= 1")
        e.rc = rc
        raise e
    return b.value


DENSE_BATCH_NMAX = 4096  # the dense batch's limit on n (lbfgs_batch_dense_plan)


def plan_dense(n, m, batch, shared=False):
    """Device bytes a Batch(n, m, batch) with dense quadratics set would take, the matrices included
    (one matrix when shared); raises LbfgsError outside the dense batch's limits (lbfgs_batch_dense_plan)."""
    b = C.c_double()
    rc = lib().lbfgs_batch_dense_plan(int(n), int(m), int(batch), int(bool(shared)), C.byref(b))
    if rc != 0:
        e = LbfgsError(f"lbfgs_batch_dense_plan({n}, {m}, {batch}) failed ({rc}): 1 <= n <= {DENSE_BATCH_NMAX}, "
                       "1 <= m <= 16, batch >= 1")
        e.rc = rc
        raise e
    return b.value


BATCH_PACKED = -1  # LBFGS_BATCH_PACKED: the stride of a ragged batch's packed rows


def _sizes_array(sizes):
    a = np.asarray(list(sizes))
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise ValueError(f"a ragged batch's sizes: a non-empty sequence of integers is required, got {sizes!r}")
    return (C.c_int64 * a.size)(*[int(v) for v in a])


def plan_ragged(sizes, m, dense=False):
    """Device bytes a ragged Batch(sizes, m) would take (no device needed), with dense its t, gt, b and
    packed matrices included; raises LbfgsError outside the limits (lbfgs_batch_ragged_plan)."""
    arr = _sizes_array(sizes)
    b = C.c_double()
    rc = lib().lbfgs_batch_ragged_plan(arr, len(arr), int(m), int(bool(dense)), C.byref(b))
    if rc != 0:
        e = LbfgsError(f"lbfgs_batch_ragged_plan failed ({rc}): 1 <= n_p <= {DENSE_BATCH_NMAX if dense else 32768} "
                       "for every problem, 1 <= m <= 16")
        e.rc = rc
        raise e
    return b.value


class Batch:
    """`batch` independent small problems (same n, m, objective, line search, constants, tolerance
    and iteration limit; their own x0, and for objective "dense" their own A and b, see
    set_dense_quadratics) solved at once, one workgroup each, the whole solver loop on
    the device; every problem's result is bit for bit Context.minimize's for it alone.

        with L.Batch(n=10_000, m=5, batch=256) as b:
            res = b.minimize("rosenbrock", X0, "backtracking", max_iterations=100)   # X0: 256 x n

    A sequence of sizes for `n` makes a RAGGED batch, problem p of size n[p] (batch = len(n)): .ragged,
    .sizes, .offsets (batch + 1 packed offsets) and .n, the largest size. Its host arrays are lists of
    per-problem arrays or one packed array; its device tensors padded rows or one packed tensor.

        with L.Batch(n=[513, 5, 1537], m=5) as b:
            res = b.minimize("rosenbrock", [x0_a, x0_b, x0_c])                      # res["x"]: 3 arrays
    """

    def __init__(self, n, m, batch=None, device=0):
        self.m, self.device = int(m), int(device)
        self._dq_refs = None  # the tensors set_dense_quadratics_device refers to
        self._dev_cb, self._dev_exc = None, None  # set_device_objective's callback, and what it raised
        if isinstance(n, np.ndarray) and n.ndim == 0:
            n = n.item()  # a 0-d array is one size
        self.ragged = not np.isscalar(n)
        h = C.c_void_p()
        if self.ragged:
            arr = _sizes_array(n)
            if batch is not None and int(batch) != len(arr):
                raise ValueError(f"Batch: {len(arr)} sizes for batch = {batch}")
            self.batch, self.n = len(arr), int(max(arr))
            rc = lib().lbfgs_batch_create_ragged(C.byref(h), arr, self.m, self.batch, int(device))
        else:
            if batch is None:
                raise TypeError("Batch: batch is required with one size n")
            self.n, self.batch = int(n), int(batch)
            rc = lib().lbfgs_batch_create(C.byref(h), self.n, self.m, self.batch, int(device))
        if rc != 0:
            e = LbfgsError(f"lbfgs_batch_create{'_ragged' if self.ragged else ''} failed ({rc})")
            e.rc = rc
            raise e
        self.h = h
        sz, of = (C.c_int64 * self.batch)(), (C.c_int64 * (self.batch + 1))()
        lib().lbfgs_batch_sizes(h, sz, of)
        self.sizes, self.offsets = [int(v) for v in sz], [int(v) for v in of]

    def close(self):
        if getattr(self, "h", None):
            lib().lbfgs_batch_destroy(self.h)
            self.h = None
        self._dq_refs = None
        self._dev_cb = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what, rc):
        exc, self._dev_exc = self._dev_exc, None
        if exc is not None:  # the device callback raised: the library saw a nonzero return
            raise exc
        msg = lib().lbfgs_batch_last_error(self.h)
        e = LbfgsError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        e.rc = rc
        raise e

    def set_launch(self, max_workgroups=0, iters_per_launch=0):
        """Tuning only (results do not depend on it): workgroups per launch and iterations a launch
        takes every unfinished problem further; 0 = the default for either."""
        rc = lib().lbfgs_batch_set_launch(self.h, int(max_workgroups), int(iters_per_launch))
        if rc != 0:
            self._err("lbfgs_batch_set_launch", rc)

    def set_device_objective(self, fn):
        """The "device" objective of the whole batch: fn(Z, active) -> (F, G), called once per round for
        every problem that waits for an evaluation. Z is a float64 CUDA tensor of shape (batch, n), a
        zero-copy view of the batch's point rows (row stride > n), valid during the call and read-only
        by contract; active a (batch,) int32 view, nonzero for the rows to evaluate. F of shape (batch,)
        and G of shape (batch, n) are CUDA float64; what they hold for inactive rows is ignored (such a
        row of Z holds the last point that problem was evaluated at). The glue copies F and G into
        views of the batch's own rows, [0, n) of each, and then synchronises the stream that is current
        when fn has returned. Every problem's result is bit for bit what Context.set_device_objective(
        eager_grad=True) + Context.minimize_device("device") gives for it alone with the same f and g;
        f_calls / grad_calls are the rounds the problem was active in. Uniform batches only. An
        exception raised by fn ends the solve and is re-raised by minimize. fn = None clears.
        For F in the solver's canonical order (reproducible, the bits of Reducer.sum per row) fn forms it
        with reduce_rows(T, active=active), T the (batch, n) table of per-element terms: one launch for
        all rows and no host wait, where Reducer.sum is two launches and a host wait per row."""
        if fn is None:
            rc = lib().lbfgs_batch_set_device_objective(self.h, None)
            self._dev_cb = None
            if rc != 0:
                self._err("lbfgs_batch_set_device_objective", rc)
            return
        torch = _torch()
        dev = torch.device("cuda", self.device)

        def rows(ptr, ld, B, n, typestr="<f8"):
            flat = torch.as_tensor(_DeviceView(ptr, (B - 1) * ld + n, typestr), device=dev)
            return flat.as_strided((B, n), (ld, 1))

        def ev(zp, ldz, fp, gp, ldg, ap, n_active, B, n, user):
            try:
                with torch.cuda.device(dev):
                    Z = rows(zp, ldz, B, n)
                    active = torch.as_tensor(_DeviceView(ap, B, "<i4"), device=dev)
                    F, G = fn(Z, active)
                    torch.as_tensor(_DeviceView(fp, B), device=dev).copy_(
                        torch.as_tensor(F, dtype=torch.float64, device=dev).reshape(B))
                    rows(gp, ldg, B, n).copy_(torch.as_tensor(G, dtype=torch.float64, device=dev).reshape(B, n))
                    torch.cuda.current_stream(dev).synchronize()
                return 0
            except BaseException as e:  # never unwinds through the C frames
                self._dev_exc = e
                return 1

        cb = BATCH_DEVICE_EVAL(ev)
        fnc = BatchDeviceFn(cb, None, 0)
        rc = lib().lbfgs_batch_set_device_objective(self.h, C.byref(fnc))
        if rc != 0:
            self._err("lbfgs_batch_set_device_objective", rc)
        self._dev_cb = cb

    def set_dense_quadratics(self, A, b):
        """Data of objective "dense", problem p minimising x'A[p]x + b[p]'x: A of shape (batch, n, n), or
        (n, n) for one matrix shared by every problem; b of shape (batch, n). float64. Copied to the
        device; may be called again with new data between solves."""
        if self.ragged:
            A, b = self._pack(A, "set_dense_quadratics: A", True), self._pack(b, "set_dense_quadratics: b", False)
            rc = lib().lbfgs_batch_set_dense_quadratics(self.h, A.ctypes.data_as(C.c_void_p), 0,
                                                        b.ctypes.data_as(C.c_void_p))
            if rc != 0:
                self._err("lbfgs_batch_set_dense_quadratics", rc)
            self._dq_refs = None
            return
        A, b = np.asarray(A), np.asarray(b)
        if A.dtype != np.float64 or b.dtype != np.float64:
            raise TypeError(f"set_dense_quadratics: A and b must be float64, got {A.dtype} and {b.dtype}")
        if A.shape not in ((self.n, self.n), (self.batch, self.n, self.n)):
            raise ValueError(f"set_dense_quadratics: A has shape {A.shape}, expected ({self.batch}, {self.n}, {self.n}) "
                             f"or, shared, ({self.n}, {self.n})")
        if b.shape != (self.batch, self.n):
            raise ValueError(f"set_dense_quadratics: b has shape {b.shape}, expected ({self.batch}, {self.n})")
        A, b = np.ascontiguousarray(A), np.ascontiguousarray(b)
        rc = lib().lbfgs_batch_set_dense_quadratics(self.h, A.ctypes.data_as(C.c_void_p), int(A.ndim == 2),
                                                    b.ctypes.data_as(C.c_void_p))
        if rc != 0:
            self._err("lbfgs_batch_set_dense_quadratics", rc)
        self._dq_refs = None  # the batch reads its own copies now

    def _pack(self, v, what, square):
        """A ragged batch's host data as one packed float64 array: a list of `batch` arrays of shapes
        (n_p,) (square: (n_p, n_p)), or the packed 1-D array itself."""
        want = [(k, k) if square else (k,) for k in self.sizes]
        total = sum(k * k if square else k for k in self.sizes)
        if isinstance(v, np.ndarray) and v.ndim == 1 and v.dtype != object:
            if v.dtype != np.float64:
                raise TypeError(f"{what}: float64 is required, got {v.dtype}")
            if v.shape != (total,):
                raise ValueError(f"{what}: packed length {v.shape[0]}, expected {total}")
            return np.ascontiguousarray(v)
        parts = [np.asarray(q) for q in v]
        if len(parts) != self.batch:
            raise ValueError(f"{what}: {len(parts)} arrays for a batch of {self.batch}")
        for p, q in enumerate(parts):
            if q.dtype != np.float64:
                raise TypeError(f"{what}: float64 is required, problem {p} has {q.dtype}")
            if q.shape != want[p]:
                raise ValueError(f"{what}: problem {p} has shape {q.shape}, expected {want[p]}")
        return np.concatenate([q.ravel() for q in parts])

    def _ragged_tensor(self, t, what, square):
        """Checks a ragged batch's float64 CUDA tensor: padded, (batch, W) or square (batch, W, W) with
        W >= n, last stride 1 and the other strides >= n (matrices apart); or packed, 1-D contiguous of
        the sum of n_p (n_p * n_p) elements. Returns (batch stride, row stride), both BATCH_PACKED for a
        packed tensor; for rows only the batch stride counts. Never a copy."""
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: a torch tensor is required, got {type(t).__name__}")
        if t.dtype != torch.float64:
            raise TypeError(f"{what}: dtype float64 is required, got {t.dtype}")
        if not t.is_cuda or (t.device.index or 0) != self.device:
            raise ValueError(f"{what}: a CUDA tensor on device {self.device} is required, got {t.device}")
        n, B = self.n, self.batch
        total = sum(k * k if square else k for k in self.sizes)
        if t.dim() == 1:
            if t.shape[0] != total or (total > 1 and t.stride(0) != 1):
                raise ValueError(f"{what}: a packed tensor has {total} elements at stride 1, got shape "
                                 f"{tuple(t.shape)}, strides {t.stride()}")
            return BATCH_PACKED, BATCH_PACKED
        dims = 3 if square else 2
        if t.dim() != dims or t.shape[0] != B or any(w < n for w in t.shape[1:]) or (square and t.shape[1] != t.shape[2]):
            raise ValueError(f"{what}: shape {tuple(t.shape)}, expected ({B}, W" + (", W" if square else "") +
                             f") with W >= {n}, or 1-D packed of {total} elements")
        st = t.stride()
        if st[-1] != 1 and t.shape[-1] > 1:
            raise ValueError(f"{what}: the last dimension must have stride 1, got strides {st} (no copy is made)")
        if square:
            lda = st[1] if t.shape[1] > 1 else max(n, 1)
            if lda < n:
                raise ValueError(f"{what}: row stride {lda} must be >= the largest n = {n}")
            bs = st[0] if B > 1 else (n - 1) * lda + n
            if bs < (n - 1) * lda + n:
                raise ValueError(f"{what}: batch stride {bs} must be >= (n - 1) * {lda} + n (matrices that do not "
                                 "interleave); a ragged batch has no shared matrix")
            return bs, lda
        ld = st[0] if B > 1 else n
        if ld < n:
            raise ValueError(f"{what}: row stride {ld} must be >= the largest n = {n}; a ragged batch has no shared row")
        return ld, ld

    def _rows(self, t, what, shapes, shared_ok):
        """Checks a float64 CUDA tensor on the batch's device whose last stride is 1 and whose other
        strides are >= n (or, where shared_ok, 0 in dimension 0, the batch's); returns its strides. Never a
        copy: the library works on the tensor's own memory."""
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: a torch tensor is required, got {type(t).__name__}")
        if t.dtype != torch.float64:
            raise TypeError(f"{what}: dtype float64 is required, got {t.dtype}")
        if not t.is_cuda or (t.device.index or 0) != self.device:
            raise ValueError(f"{what}: a CUDA tensor on device {self.device} is required, got {t.device}")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{what}: shape {tuple(t.shape)}, expected " + " or ".join(str(s) for s in shapes))
        st = t.stride()
        if st[-1] != 1 and self.n > 1:
            raise ValueError(f"{what}: the last dimension must have stride 1, got strides {st} (no copy is made)")
        for d in range(t.dim() - 1):
            size, ok0 = t.shape[d], shared_ok and d == 0
            if size > 1 and not (st[d] >= self.n or (ok0 and st[d] == 0)):
                raise ValueError(f"{what}: stride {st[d]} of dimension {d} must be >= n = {self.n}"
                                 + (" (or 0, an expanded row)" if ok0 else ""))
        return st

    def set_dense_quadratics_device(self, A, b):
        """set_dense_quadratics BY REFERENCE to CUDA tensors: A of shape (batch, n, n) with last stride
        1, row stride >= n and any batch stride that keeps the matrices apart (0, from expand, or a 2-D
        (n, n) tensor: one matrix shared by every problem); b of shape (batch, n), last stride 1, row
        stride >= n or 0. float64, on the batch's device. Nothing is copied (so nothing is made
        contiguous either): every later "dense" solve reads the tensors' memory as it then is, and the
        object keeps references to both until they are replaced or close() is called."""
        torch = _torch()
        n, B = self.n, self.batch
        if self.ragged:
            abs_, lda = self._ragged_tensor(A, "set_dense_quadratics_device: A", True)
            ldb, _ = self._ragged_tensor(b, "set_dense_quadratics_device: b", False)
            torch.cuda.current_stream(self.device).synchronize()
            rc = lib().lbfgs_batch_set_dense_quadratics_device(self.h, A.data_ptr(), int(abs_), int(lda), b.data_ptr(),
                                                               int(ldb))
            if rc != 0:
                self._err("lbfgs_batch_set_dense_quadratics_device", rc)
            self._dq_refs = (A, b)
            return
        sa = self._rows(A, "set_dense_quadratics_device: A", ((B, n, n), (n, n)), getattr(A, "ndim", 0) == 3)
        sb = self._rows(b, "set_dense_quadratics_device: b", ((B, n),), True)
        lda = sa[-2] if n > 1 else n
        abs_ = 0 if A.dim() == 2 else (sa[0] if B > 1 else (n - 1) * lda + n)
        if abs_ != 0 and abs_ < (n - 1) * lda + n:
            raise ValueError(f"set_dense_quadratics_device: A: batch stride {abs_} must be >= (n - 1) * {lda} + n "
                             "(matrices that do not interleave), or 0")
        ldb = sb[0] if B > 1 else n
        torch.cuda.current_stream(self.device).synchronize()  # the caller's work on A and b is complete
        rc = lib().lbfgs_batch_set_dense_quadratics_device(self.h, A.data_ptr(), int(abs_), int(lda), b.data_ptr(),
                                                           int(ldb))
        if rc != 0:
            self._err("lbfgs_batch_set_dense_quadratics_device", rc)
        self._dq_refs = (A, b)

    def minimize_device(self, objective, X0, line_search="backtracking", max_iterations=1000, tolerance=1e-5,
                        consts=None, trace=False, flags=0, out=None):
        """minimize() with X0 and the result in device memory: float64 CUDA tensors of shape (batch, n) on
        the batch's device with last stride 1; X0 with any row stride >= n or 0 (an expanded row), out
        with a row stride >= n (a new contiguous tensor when None; X0 itself solves in place). A storage
        offset is fine. No copy is made. Returns minimize()'s dictionary, bit for bit, with x the tensor."""
        torch = _torch()
        n, B = self.n, self.batch
        if self.ragged:  # padded rows (B, W) or one packed tensor; out=None gives X0's form
            ldx0, _ = self._ragged_tensor(X0, "minimize_device: X0", False)
            X = out if out is not None else torch.empty_like(X0, memory_format=torch.contiguous_format)
            ldx, _ = self._ragged_tensor(X, "minimize_device: out", False)
        else:
            s0 = self._rows(X0, "minimize_device: X0", ((B, n),), True)
            if out is not None:
                self._rows(out, "minimize_device: out", ((B, n),), False)
            X = out if out is not None else torch.empty((B, n), dtype=torch.float64, device=X0.device)
            ldx0 = s0[0] if B > 1 else n
            ldx = X.stride(0) if B > 1 else n
        torch.cuda.current_stream(self.device).synchronize()  # the caller's work on X0 (and A, b) is complete
        res = (Result * B)()
        k = consts if consts is not None else constants()
        fl = FLAG_QUIET | (FLAG_TRACE if trace else 0) | int(flags)
        obj = OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        self._dev_exc = None
        rc = lib().lbfgs_batch_minimize_device(self.h, obj, LINE_SEARCHES[line_search], C.byref(k), X0.data_ptr(),
                                               int(ldx0), X.data_ptr(), int(ldx), int(max_iterations), float(tolerance),
                                               fl, res)
        if rc < 0:
            self._err("lbfgs_batch_minimize_device", rc)
        return self._results(res, X, trace)

    def minimize(self, objective, X0, line_search="backtracking", max_iterations=1000, tolerance=1e-5,
                 consts=None, trace=False, flags=0, out=None):
        """X0: batch x n. Returns per-problem arrays x (batch x n), f, gnorm, iterations, status
        (names; status_code: the numbers), commits, trials_f, trials_fg, h_min, h_max, bytes, and the
        call's launches and seconds; with trace also the lists tr_f / tr_gnorm / tr_alpha and events.
        flags: further LBFGS_FLAG_* bits, passed through (the library refuses what a batch cannot do)."""
        if self.ragged:  # a list of per-problem arrays or one packed array; x comes back as a list of views
            X0 = self._pack(X0, "minimize: X0", False)
            if out is not None:
                if not isinstance(out, np.ndarray) or out.dtype != np.float64:
                    raise TypeError("minimize: out must be a float64 numpy array")
                if out.shape != X0.shape or not out.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"minimize: out must be a packed contiguous array of {X0.shape[0]} elements, got shape "
                                     f"{out.shape}")
        else:
            X0 = np.ascontiguousarray(X0, dtype=np.float64)
            assert X0.shape == (self.batch, self.n)
            if out is not None:
                assert out.dtype == np.float64 and out.shape == X0.shape and out.flags["C_CONTIGUOUS"]
        X = out if out is not None else np.zeros_like(X0)
        res = (Result * self.batch)()
        k = consts if consts is not None else constants()
        fl = FLAG_QUIET | (FLAG_TRACE if trace else 0) | int(flags)
        obj = OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        self._dev_exc = None
        rc = lib().lbfgs_batch_minimize(self.h, obj, LINE_SEARCHES[line_search], C.byref(k), X0, X,
                                        int(max_iterations), float(tolerance), fl, res)
        if rc < 0:
            self._err("lbfgs_batch_minimize", rc)
        if self.ragged:
            X = [X[self.offsets[p]:self.offsets[p + 1]] for p in range(self.batch)]
        return self._results(res, X, trace)

    def _results(self, res, X, trace):
        col = lambda name, dt: np.array([getattr(r, name) for r in res], dtype=dt)  # noqa: E731
        code = col("status", np.int64)
        d = dict(x=X, f=col("f", np.float64), gnorm=col("gnorm", np.float64), iterations=col("iterations", np.int64),
                 status=[STATUS.get(int(s), int(s)) for s in code], status_code=code,
                 commits=col("commits", np.int64), trials_f=col("trials_f", np.int64),
                 trials_fg=col("trials_fg", np.int64), h_min=col("h_min", np.int64), h_max=col("h_max", np.int64),
                 bytes=col("bytes", np.float64), f_calls=col("f_calls", np.int64),
                 grad_calls=col("grad_calls", np.int64), launches=int(res[0].passes), seconds=float(res[0].seconds))
        if trace:
            d["tr_f"], d["tr_gnorm"], d["tr_alpha"], d["events"] = [], [], [], []
            for p in range(self.batch):
                f, g, a = self.trace(p)
                d["tr_f"].append(f)
                d["tr_gnorm"].append(g)
                d["tr_alpha"].append(a)
                d["events"].append(self.events(p))
        return d

    def trace(self, problem):
        """(f, |g|, alpha) per iteration of one problem of the last traced solve"""
        n = lib().lbfgs_batch_trace_len(self.h, int(problem))
        if n < 0:
            self._err("lbfgs_batch_trace_len", n)
        f, g, a = np.empty(max(n, 1)), np.empty(max(n, 1)), np.empty(max(n, 1))
        lib().lbfgs_batch_trace_get(self.h, int(problem), f, g, a, n)
        return f[:n], g[:n], a[:n]

    def events(self, problem):
        """dict(not_descent, skipped_updates, invalid_rho, invalid_gamma) of one problem of the last solve"""
        ev = BatchEvents()
        rc = lib().lbfgs_batch_events_get(self.h, int(problem), C.byref(ev))
        if rc != 0:
            self._err("lbfgs_batch_events_get", rc)
        return ev.as_dict()


class _DeviceView:
    """n float64 at a device address, for torch.as_tensor(view, device=...): a zero-copy tensor over
    memory the library owns (torch takes no ownership; the view is valid while the library says so)."""

    def __init__(self, ptr, n, typestr="<f8"):
        # torch accepts writable views only; a read-only buffer (the callback's x) is one by contract
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr=typestr, data=(int(ptr), False), version=2,
                                             strides=None)


def hip_runtimes():
    """Paths of the HIP runtime copies mapped into this process."""
    try:
        with open("/proc/self/maps") as fp:
            return sorted({ln.split()[-1] for ln in fp if "libamdhip64" in ln})
    except OSError:
        return []


_torch_checked = False


def _torch():
    """torch, for the entry points that share device memory with it. A torch wheel brings its own copy
    of the HIP runtime; device memory cannot be shared across two copies in one process (and the
    second to initialise finds no GPU). liblbfgs_hip.so binds to torch's copy when torch is imported
    before the library is loaded; the other order is an error here, not a crash later."""
    global _torch_checked
    import torch

    if _torch_checked:
        return torch
    lib()
    rt = hip_runtimes()
    if len(rt) > 1:
        raise LbfgsError("torch and liblbfgs_hip.so are on different copies of the HIP runtime (" + ", ".join(rt) +
                         "): import torch before the first lbfgs_amd call loads the library, so that it binds "
                         "to the runtime torch brought")
    _torch_checked = True
    return torch


def _device_tensor(ptr, n, device):
    import torch

    return torch.as_tensor(_DeviceView(ptr, n), device=device)


def _check_device_tensor(t, n, device, what):
    torch = _torch()

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1 and
            t.numel() == n and t.is_contiguous() and (t.device.index or 0) == device):
        raise ValueError(f"{what}: a contiguous float64 CUDA tensor of {n} elements on device {device} is required")


class Reducer:
    """The solver's canonical fixed-order reduction over CUDA tensors of n float64 (lbfgs_reducer_*):
    dot(a, b) has the bits of Context.dot for the same data, sum(t) those of the dot with ones. For
    device objectives (Context.set_device_objective) that reduce their per-element terms to f. The
    tensors may sit at any storage offset; nothing outside them is read. Runs on torch's current
    stream (the null stream orders nothing against the library's own non-blocking streams, so when
    that is the current one it is synchronised first and the reducer's own stream is used); the
    value is complete on return. One vector per call, two launches and a host wait: inside a batch
    callback (Batch.set_device_objective) use the row form, reduce_rows, which gives the same bits for
    every row of a table in one launch and leaves them on the device."""

    def __init__(self, n, device=0):
        _torch()
        self.n, self.device = int(n), int(device)
        h = C.c_void_p()
        rc = lib().lbfgs_reducer_create(C.byref(h), self.n, self.device)
        if rc != 0:
            e = LbfgsError(f"lbfgs_reducer_create failed ({rc})")
            e.rc = rc
            raise e
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().lbfgs_reducer_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dot(self, a, b=None):
        torch = _torch()

        _check_device_tensor(a, self.n, self.device, "Reducer: a")
        if b is not None:
            _check_device_tensor(b, self.n, self.device, "Reducer: b")
        st = torch.cuda.current_stream(self.device)
        if not st.cuda_stream:
            st.synchronize()
        out = C.c_double()
        rc = lib().lbfgs_reducer_dot(self.h, a.data_ptr(), b.data_ptr() if b is not None else None,
                                     st.cuda_stream or None, C.byref(out))
        if rc != 0:
            e = LbfgsError(f"lbfgs_reducer_dot failed ({rc})")
            e.rc = rc
            raise e
        return out.value

    def sum(self, t):
        return self.dot(t, None)


REDUCE_ROWS_NMAX = 32768  # the batched solver's limit: L = 512, at most 64 segments


def reduce_rows(a, b=None, active=None, out=None):
    """The canonical fixed-order sum of every row of a table in one launch (lbfgs_reduce_rows): out[p] =
    sum_i a[p, i] * b[p, i] (b = None: of a[p, i]), bit for bit Reducer.dot / Reducer.sum of that row.
    The form for a batch callback (Batch.set_device_objective): one launch whatever the batch, the
    result left in device memory, no host wait.

    a: a 2-D float64 CUDA tensor (B, n) with stride(1) == 1 and stride(0) >= n, at any storage offset,
    n <= 32768. b: None, the same kind of tensor, or a 1-D contiguous (n,) tensor shared by every row.
    active: None or a (B,) int32 contiguous CUDA tensor (the view a batch callback receives); a row with
    0 is skipped and its out[p] is not written. out: None (a new (B,) tensor filled with NaN, so that
    skipped rows are recognisable) or a (B,) contiguous float64 CUDA tensor. Returns out. Runs on torch's
    current stream of the tensors' device, the null stream included, and does not synchronise.
    ValueError for anything else, before anything is launched; LbfgsError with .rc on a nonzero return."""
    torch = _torch()

    def f64(t, what):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
            raise ValueError(f"reduce_rows: {what}: a float64 CUDA tensor is required")

    f64(a, "a")
    if a.dim() != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("reduce_rows: a: a 2-D tensor (B, n) with B >= 1 and n >= 1 is required")
    B, n = a.shape
    dev = a.device
    if n > REDUCE_ROWS_NMAX:
        raise ValueError(f"reduce_rows: n = {n} is above {REDUCE_ROWS_NMAX} (a longer row uses Reducer)")

    def rows(t, what):  # the row stride of a (B, n) table with unit inner stride
        if t.shape != (B, n) or t.stride(1) != 1 and n > 1 or t.stride(0) < n and B > 1:
            raise ValueError(f"reduce_rows: {what}: shape ({B}, {n}) with stride(1) == 1 and stride(0) >= n is required")
        return t.stride(0) if B > 1 else n

    lda = rows(a, "a")
    ldb = 0
    if b is not None:
        f64(b, "b")
        if b.device != dev:
            raise ValueError("reduce_rows: b: on another device than a")
        if b.dim() == 1:
            if b.shape != (n,) or not b.is_contiguous():
                raise ValueError(f"reduce_rows: b: a shared b is a contiguous 1-D tensor of {n} elements")
        elif b.dim() == 2:
            ldb = rows(b, "b")
        else:
            raise ValueError("reduce_rows: b: a 1-D or 2-D tensor is required")
    if active is not None:
        if not (isinstance(active, torch.Tensor) and active.is_cuda and active.dtype == torch.int32 and
                active.shape == (B,) and active.is_contiguous() and active.device == dev):
            raise ValueError(f"reduce_rows: active: a contiguous int32 CUDA tensor of shape ({B},) on a's device is required")
    if out is None:
        out = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    else:
        f64(out, "out")
        if out.shape != (B,) or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"reduce_rows: out: a contiguous tensor of shape ({B},) on a's device is required")
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    rc = lib().lbfgs_reduce_rows(index, n, B, a.data_ptr(), lda, b.data_ptr() if b is not None else None, ldb,
                                 active.data_ptr() if active is not None else None, out.data_ptr(),
                                 torch.cuda.current_stream(index).cuda_stream or None)
    if rc != 0:
        e = LbfgsError(f"lbfgs_reduce_rows failed ({rc})")
        e.rc = rc
        raise e
    return out


class Context:
    """A persistent solver context: device vectors for n (or this rank's shard of n) and the
    m-pair history ring stay resident across calls."""

    def __init__(self, n, m=10, device=0, rank=0, world=1, uid=None, group=None):
        self.n, self.m = int(n), int(m)
        h = C.c_void_p()
        if group is not None:
            rc = lib().lbfgs_ctx_create_emulated(C.byref(h), self.n, self.m, device, rank, group.h)
        elif world == 1 and uid is None:
            rc = lib().lbfgs_ctx_create(C.byref(h), self.n, self.m, device)
        else:
            rc = lib().lbfgs_ctx_create_sharded(C.byref(h), self.n, self.m, device, rank, world, uid)
        if rc != 0:
            raise LbfgsError(f"lbfgs_ctx_create failed ({rc})")
        self.h = h
        lo, nl = C.c_int64(), C.c_int64()
        lib().lbfgs_local_range(self.h, C.byref(lo), C.byref(nl))
        self.elem_lo, self.n_loc = lo.value, nl.value
        self._cb = None
        self.device = int(device)
        self._dev_cb = None   # keeps the device callback's ctypes thunk alive
        self._dev_exc = None  # a Python exception raised inside it, re-raised by the calling method

    def close(self):
        if getattr(self, "h", None):
            lib().lbfgs_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def spec_stats(self):
        """(adopted, dropped): speculative next-iteration launches the host took / discarded
        since solver init (small n, cooperative iteration; LBFGS_SPEC=0: none)."""
        a, d = C.c_int64(), C.c_int64()
        lib().lbfgs_spec_stats(self.h, C.byref(a), C.byref(d))
        return a.value, d.value

    def search_stats(self):
        """(launches, commits): line searches continued on the device since solver init, and the
        commits those launches took at the step they found (small n; LBFGS_DEV_SEARCH=0: none)."""
        a, d = C.c_int64(), C.c_int64()
        lib().lbfgs_search_stats(self.h, C.byref(a), C.byref(d))
        return a.value, d.value

    def set_dense_quadratic(self, A, b):
        """Upload A (n x n, symmetric) and b for the "dense" objective f = x'Ax + b'x."""
        A = np.ascontiguousarray(A, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        assert A.shape == (self.n, self.n) and b.shape == (self.n,)
        rc = lib().lbfgs_set_dense_quadratic(self.h, A.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        if rc != 0:
            self._err("lbfgs_set_dense_quadratic", rc)

    # ---- sharded runs: xGMI peer exchange ----
    def peer_handle(self):
        buf = C.create_string_buffer(PEER_HANDLE_BYTES)
        rc = lib().lbfgs_peer_handle(self.h, buf)
        if rc != 0:
            self._err("lbfgs_peer_handle", rc)
        return buf.raw

    def connect_peers(self, allgather, agree):
        """Switch this sharded context's exchanges to the xGMI peer mailboxes.
        allgather(bytes) -> list of every rank's bytes (rank order); agree(ok: bool) -> True iff
        every rank passed (e.g. torch.distributed gloo all_gather_object / all_reduce MIN).
        Returns (enabled, this rank's connect error or None); when a rank fails, no rank enables
        and the context keeps its RCCL communicator (if it has one)."""
        msg = None
        try:
            mine = self.peer_handle()
        except LbfgsError as e:  # no mailbox on this rank: every rank still joins the collectives
            mine, msg = b"", str(e)
        handles = allgather(mine)
        if all(len(h) == PEER_HANDLE_BYTES for h in handles):
            rc = lib().lbfgs_peer_connect(self.h, b"".join(handles))
            if rc != 0:
                m = lib().lbfgs_last_error(self.h)
                msg = f"lbfgs_peer_connect failed ({rc}): {m.decode() if m else ''}"
        else:
            rc = -1
            msg = msg or "a peer has no mailbox"
        ok = agree(rc == 0)
        if ok:
            rc2 = lib().lbfgs_peer_enable(self.h, 1)
            if rc2 != 0:
                self._err("lbfgs_peer_enable", rc2)
        return ok, msg

    def peer_enable(self, on=True):
        """Route this context's exchanges through the peer mailboxes (after connect_peers) or
        back to its RCCL communicator. Every rank must make the same choice."""
        rc = lib().lbfgs_peer_enable(self.h, 1 if on else 0)
        if rc != 0:
            self._err("lbfgs_peer_enable", rc)

    def rccl_attach(self, uid):
        """Give this sharded context (created without an RCCL id) a communicator: collective over
        every rank, bounded by LBFGS_RCCL_TIMEOUT (60 s); raises LbfgsError on a failed or stalled
        init, leaving the context on its mailboxes."""
        rc = lib().lbfgs_rccl_attach(self.h, uid)
        if rc != 0:
            self._err("lbfgs_rccl_attach", rc)

    def exchange_latency(self, backend, components=8, iters=200):
        """Collective: microseconds per exchange through 'rccl' or 'xgmi' (every rank calls)."""
        us = C.c_double()
        rc = lib().lbfgs_exchange_latency(self.h, {"rccl": 1, "xgmi": 2}[backend], int(components), int(iters),
                                          C.byref(us))
        if rc != 0:
            self._err("lbfgs_exchange_latency", rc)
        return us.value

    @property
    def backend(self):
        return BACKENDS.get(lib().lbfgs_exchange_backend(self.h), "unknown")

    def coop_info(self):
        """dict(coop_max, search_max, fallbacks): the cooperative forms' grid caps (segments) and
        the device line searches redone on the host loop after a grid-barrier time-out"""
        a, b, f = C.c_int(), C.c_int(), C.c_int()
        lib().lbfgs_coop_info(self.h, C.byref(a), C.byref(b), C.byref(f))
        return dict(coop_max=a.value, search_max=b.value, fallbacks=f.value)

    def stream_probe_vectors(self, q, y, s, launches=20):
        """the probe's stream over three of the context's vectors by allocation index
        (lbfgs_stream_probe_vectors): mean microseconds per launch"""
        us = C.c_double()
        rc = lib().lbfgs_stream_probe_vectors(self.h, int(q), int(y), int(s), int(launches), C.byref(us))
        if rc != 0:
            self._err("lbfgs_stream_probe_vectors", rc)
        return us.value

    def vector_address(self, k):
        a = C.c_uint64()
        if lib().lbfgs_vector_address(self.h, int(k), C.byref(a)) != 0:
            return None
        return a.value

    @property
    def vector_pool(self):
        """(mode, vectors of this context taken from / added to the contiguous pool, GiB the process's
        pool owns); mode 'pool' (default), 'plain' or 'contiguous' (lbfgs_vector_pool)"""
        n, gb = C.c_int(), C.c_double()
        mode = int(lib().lbfgs_vector_pool(self.h, C.byref(n), C.byref(gb)))
        return {0: "pool", 1: "plain", 2: "contiguous"}.get(mode, mode), n.value, gb.value

    @property
    def vector_fallbacks(self):
        """vectors that asked for a physically contiguous allocation (LBFGS_VEC_ALLOC=contiguous) and got a plain one"""
        return int(lib().lbfgs_vector_fallbacks(self.h))

    @staticmethod
    def work_split_stats():
        """the split work vector's process-wide counters (LBFGS_WORK_SPLIT; the device layer's
        lbk_work_split_stats): dict(passes, copies, alloc_failed, given_up) - split passes launched,
        consolidation copies of a displaced middle, failed allocations of the alternate buffer (the
        context then stays unsplit), displaced middles given up when the other work vector took
        the alternate buffer"""
        out = (C.c_uint64 * 4)()
        fn = lib().lbk_work_split_stats  # (bound here: an older library selected with LBFGS_LIB lacks it)
        fn.argtypes, fn.restype = [C.POINTER(C.c_uint64)], None
        fn(out)
        return dict(passes=int(out[0]), copies=int(out[1]), alloc_failed=int(out[2]), given_up=int(out[3]))

    def wait_stats(self):
        """host waits on completion words: dict(slept_s, waits, adaptive) (lbfgs_wait_stats)"""
        s, w, a = C.c_double(), C.c_uint64(), C.c_int()
        lib().lbfgs_wait_stats(self.h, C.byref(s), C.byref(w), C.byref(a))
        return dict(slept_s=s.value, waits=w.value, adaptive=bool(a.value))

    @property
    def cu_partition(self):
        """CUs this rank's solver stream is confined to (LBFGS_CU_PARTITION=1), 0 if not"""
        return int(lib().lbfgs_cu_partition(self.h))

    def stream_probe(self, launches=20, variant=0):
        """This box's rate for the two-loop passes' 3 R + 1 W access pattern over the context's own
        buffers (lbfgs_stream_probe; after init): dict(avg_launch_us, bytes_per_launch, gbps).
        variant > 0: the pass's machinery added piece by piece (lbfgs_stream_probe_variant)."""
        us, b = C.c_double(), C.c_double()
        rc = lib().lbfgs_stream_probe_variant(self.h, int(variant), int(launches), C.byref(us), C.byref(b))
        if rc != 0:
            self._err("lbfgs_stream_probe", rc)
        return dict(avg_launch_us=us.value, bytes_per_launch=b.value,
                    gbps=b.value / (us.value * 1e-6) / 1e9 if us.value > 0 else None)

    @property
    def folded(self):
        """the two-loop's mailbox exchanges ride inside the passes (lbfgs_exchange_fold)"""
        return lib().lbfgs_exchange_fold(self.h) == 1

    def _err(self, what, rc):
        exc, self._dev_exc = self._dev_exc, None
        if exc is not None:  # the device callback raised: the library saw a nonzero return
            raise exc
        msg = lib().lbfgs_last_error(self.h)
        e = LbfgsError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        e.rc = rc
        raise e

    # ---- device-callback objective, device-resident x0 / x ----
    def set_device_objective(self, fn, eager_grad=False):
        """The "device" objective: fn(x, want_grad) -> f, or (f, g) when want_grad. x is a float64 CUDA
        tensor of n elements, a zero-copy view of solver memory, valid during the call and read-only
        by contract; g is a tensor of n elements (copied into a zero-copy view of the solver's
        gradient buffer); f a number or a one-element tensor. The solver's work on x is complete when
        fn is called, so fn may read it on any torch stream; the glue copies g and then synchronises
        on the stream that is current when fn has returned, so an fn that worked on a stream it
        entered itself synchronises that one before it returns. eager_grad: every call asks for the gradient (for objectives
        whose backward pass is cheap next to a second forward pass); the iterates are the same.
        An exception raised by fn ends the solve and is re-raised by the method that ran it.
        fn = None clears the objective."""
        if fn is None:
            rc = lib().lbfgs_set_device_objective(self.h, None)
            self._dev_cb = None
            if rc != 0:
                self._err("lbfgs_set_device_objective", rc)
            return
        torch = _torch()
        dev = torch.device("cuda", self.device)

        def ev(xp, n, fp, gp, user):
            try:
                with torch.cuda.device(dev):
                    x = _device_tensor(xp, n, dev)
                    r = fn(x, bool(gp))
                    f, g = (r if isinstance(r, (tuple, list)) else (r, None))
                    if gp:
                        if g is None:
                            raise ValueError("device objective: a gradient was asked for, fn returned none")
                        _device_tensor(gp, n, dev).copy_(torch.as_tensor(g, dtype=torch.float64, device=dev)
                                                         .reshape(n))
                    if fp:
                        fp[0] = float(f)
                    torch.cuda.current_stream(dev).synchronize()
                return 0
            except BaseException as e:  # never unwinds through the C frames
                self._dev_exc = e
                return 1

        cb = DEVICE_EVAL(ev)
        fnc = DeviceFn(cb, None, DEVICE_EAGER_GRAD if eager_grad else 0)
        rc = lib().lbfgs_set_device_objective(self.h, C.byref(fnc))
        if rc != 0:
            self._err("lbfgs_set_device_objective", rc)
        self._dev_cb = cb

    def _flags(self, verbose=False, quiet=True, trace=False, unfused=False, vector_free=False,
               reference_calls=False, cuda_compat=False, cuda_variant=False):
        return (FLAG_VERBOSE if verbose else 0) | (FLAG_QUIET if quiet else 0) | \
               (FLAG_TRACE if trace else 0) | (FLAG_UNFUSED if unfused else 0) | \
               (FLAG_VECTOR_FREE if vector_free else 0) | (FLAG_REFERENCE_CALLS if reference_calls else 0) | \
               (FLAG_CUDA_COMPAT if cuda_compat else 0) | (FLAG_CUDA_VARIANT if cuda_variant else 0)

    def minimize_device(self, objective, x0, line_search="backtracking", max_iterations=1000, tolerance=1e-5,
                        verbose=False, quiet=True, trace=False, consts=None, f=None, grad=None, unfused=False,
                        vector_free=False, reference_calls=False, out=None, cuda_compat=False,
                        cuda_variant=False):
        """minimize() with x0 and the result in device memory: x0 and out are contiguous float64 CUDA
        tensors of n elements (a slice at any storage offset is fine; out: a new tensor when None).
        One rank, every objective. The result's "x" is the tensor; every number is bit for bit
        minimize()'s, except passes / bytes, which also count the two copy passes."""
        torch = _torch()

        _check_device_tensor(x0, self.n, self.device, "minimize_device: x0")
        if out is not None:
            _check_device_tensor(out, self.n, self.device, "minimize_device: out")
        x = out if out is not None else torch.empty(self.n, dtype=torch.float64, device=x0.device)
        torch.cuda.current_stream(self.device).synchronize()  # the caller's work on x0 is complete
        res = Result()
        flags = self._flags(verbose, quiet, trace, unfused, vector_free, reference_calls, cuda_compat, cuda_variant)
        cb = self._host_fn(f, grad) if objective == "host" else None
        k = consts if consts is not None else constants("cuda" if cuda_compat else "config")
        self._dev_exc = None
        rc = lib().lbfgs_minimize_device(self.h, OBJECTIVES[objective], C.byref(cb) if cb else None,
                                         LINE_SEARCHES[line_search], C.byref(k), x0.data_ptr(), x.data_ptr(),
                                         int(max_iterations), float(tolerance), flags, C.byref(res))
        if rc < 0:
            self._err("lbfgs_minimize_device", rc)
        r = res.as_dict()
        r["x"] = x
        r["messages"] = self.messages()
        if trace:
            r.update(self.trace())
        return r

    def init_device(self, objective, x0, line_search="backtracking", tolerance=1e-5, quiet=True, trace=False,
                    consts=None, unfused=False, vector_free=False):
        """init() with x0 a CUDA tensor (see minimize_device)."""
        torch = _torch()

        _check_device_tensor(x0, self.n, self.device, "init_device: x0")
        torch.cuda.current_stream(self.device).synchronize()
        flags = self._flags(quiet=quiet, trace=trace, unfused=unfused, vector_free=vector_free)
        k = consts if consts is not None else constants()
        self._dev_exc = None
        rc = lib().lbfgs_solver_init_device(self.h, OBJECTIVES[objective], None, LINE_SEARCHES[line_search],
                                            C.byref(k), x0.data_ptr(), float(tolerance), flags)
        if rc != 0:
            self._err("lbfgs_solver_init_device", rc)

    def get_x_device(self, out=None):
        """get_x() into a CUDA tensor (a new one when out is None); complete on return."""
        torch = _torch()

        if out is not None:
            _check_device_tensor(out, self.n, self.device, "get_x_device: out")
        x = out if out is not None else torch.empty(self.n, dtype=torch.float64,
                                                    device=torch.device("cuda", self.device))
        rc = lib().lbfgs_get_x_device(self.h, x.data_ptr())
        if rc != 0:
            self._err("lbfgs_get_x_device", rc)
        return x

    def _host_fn(self, f, grad):
        def cf(xp, n, user):
            return float(f(np.ctypeslib.as_array(xp, shape=(n,)).copy()))

        def cg(xp, n, gp, user):
            g = np.asarray(grad(np.ctypeslib.as_array(xp, shape=(n,)).copy()), dtype=np.float64)
            np.ctypeslib.as_array(gp, shape=(n,))[:] = g

        self._cb = (HOST_F(cf), HOST_G(cg))
        return HostFn(self._cb[0], self._cb[1], None)

    def minimize(self, objective, x0, line_search="backtracking", max_iterations=1000, m=None,
                 tolerance=1e-5, verbose=False, quiet=True, trace=False, consts=None,
                 f=None, grad=None, unfused=False, vector_free=False, reference_calls=False, out=None,
                 cuda_compat=False, cuda_variant=False):
        """out: a caller-owned float64 buffer of n for the result (else a new array; a fresh
        array's pages are first touched by the result's copy, which costs as much as the copy)"""
        assert m is None or m == self.m
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        assert x0.shape == (self.n,)
        if out is not None:
            assert out.dtype == np.float64 and out.shape == (self.n,) and out.flags["C_CONTIGUOUS"]
        x = out if out is not None else np.zeros(self.n)
        res = Result()
        flags = (FLAG_VERBOSE if verbose else 0) | (FLAG_QUIET if quiet else 0) | \
                (FLAG_TRACE if trace else 0) | (FLAG_UNFUSED if unfused else 0) | \
                (FLAG_VECTOR_FREE if vector_free else 0) | (FLAG_REFERENCE_CALLS if reference_calls else 0) | \
                (FLAG_CUDA_COMPAT if cuda_compat else 0) | (FLAG_CUDA_VARIANT if cuda_variant else 0)
        cb = self._host_fn(f, grad) if objective == "host" else None
        # the CUDA path reads parallel-implementation/constants.h (C2 = 0.7), not config.h
        k = consts if consts is not None else constants("cuda" if cuda_compat else "config")
        rc = lib().lbfgs_minimize(self.h, OBJECTIVES[objective], C.byref(cb) if cb else None,
                                  LINE_SEARCHES[line_search], C.byref(k), x0, x,
                                  int(max_iterations), float(tolerance), flags, C.byref(res))
        if rc < 0:
            self._err("lbfgs_minimize", rc)
        out = res.as_dict()
        out["x"] = x
        out["messages"] = self.messages()
        if trace:
            out.update(self.trace())
        return out

    def init(self, objective, x0, line_search="backtracking", tolerance=1e-5, quiet=True,
             trace=False, consts=None, unfused=False, vector_free=False):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        flags = (FLAG_QUIET if quiet else 0) | (FLAG_TRACE if trace else 0) | \
            (FLAG_UNFUSED if unfused else 0) | (FLAG_VECTOR_FREE if vector_free else 0)
        k = consts if consts is not None else constants()
        rc = lib().lbfgs_solver_init(self.h, OBJECTIVES[objective], None,
                                     LINE_SEARCHES[line_search], C.byref(k), x0, float(tolerance),
                                     flags)
        if rc != 0:
            self._err("lbfgs_solver_init", rc)

    def step(self, steps):
        res = Result()
        rc = lib().lbfgs_solver_step(self.h, int(steps), C.byref(res))
        if rc < 0:
            self._err("lbfgs_solver_step", rc)
        return res.as_dict()

    def sync(self):
        rc = lib().lbfgs_sync(self.h)
        if rc != 0:
            self._err("lbfgs_sync", rc)

    def get_x(self):
        x = np.zeros(self.n)
        rc = lib().lbfgs_get_x(self.h, x)
        if rc != 0:
            self._err("lbfgs_get_x", rc)
        return x

    def messages(self):
        buf = C.create_string_buffer(1 << 20)
        lib().lbfgs_messages(self.h, buf, len(buf))
        return buf.value.decode()

    def trace_enable(self, on=True):
        """Record (or stop recording) the per-iteration trace between step() calls."""
        rc = lib().lbfgs_trace_enable(self.h, 1 if on else 0)
        if rc != 0:
            self._err("lbfgs_trace_enable", rc)

    def trace(self):
        n = lib().lbfgs_trace_len(self.h)
        f, g, a = np.empty(max(n, 1)), np.empty(max(n, 1)), np.empty(max(n, 1))
        c1, c2 = np.empty(max(n, 1), np.uint64), np.empty(max(n, 1), np.uint64)
        lib().lbfgs_trace_get(self.h, f, g, a, c1, c2, n)
        return dict(tr_f=f[:n], tr_gnorm=g[:n], tr_alpha=a[:n], tr_c1=c1[:n], tr_c2=c2[:n])

    # ---- primitives ----
    def dot(self, a, b):
        out = C.c_double()
        rc = lib().lbfgs_dev_dot(self.h, np.ascontiguousarray(a, np.float64),
                                 np.ascontiguousarray(b, np.float64), C.byref(out))
        if rc != 0:
            self._err("lbfgs_dev_dot", rc)
        return out.value

    def objective(self, objective, x, with_grad=True):
        f = C.c_double()
        g = np.zeros(self.n) if with_grad else None
        rc = lib().lbfgs_dev_objective(self.h, OBJECTIVES[objective],
                                       np.ascontiguousarray(x, np.float64), C.byref(f),
                                       g.ctypes.data_as(C.c_void_p) if with_grad else None)
        if rc != 0:
            self._err("lbfgs_dev_objective", rc)
        return f.value, g

    def trial(self, objective, x, d, alpha, with_grad=True):
        f, dphi = C.c_double(), C.c_double()
        g = np.zeros(self.n) if with_grad else None
        rc = lib().lbfgs_dev_trial(self.h, OBJECTIVES[objective],
                                   np.ascontiguousarray(x, np.float64),
                                   np.ascontiguousarray(d, np.float64), float(alpha), C.byref(f),
                                   g.ctypes.data_as(C.c_void_p) if with_grad else None,
                                   C.byref(dphi))
        if rc != 0:
            self._err("lbfgs_dev_trial", rc)
        return f.value, g, dphi.value

    def line_search(self, objective, line_search, x, d, g, consts=None):
        """lbfgs_line_search: the reference's free line-search functions (line_search.cpp) at x along
        d with gradient g, device objective; returns the step"""
        a = C.c_double()
        k = consts if consts is not None else constants()
        dp = lambda v: np.ascontiguousarray(v, np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        xs, ds, gs = (np.ascontiguousarray(v, np.float64) for v in (x, d, g))
        rc = lib().lbfgs_line_search(self.h, OBJECTIVES[objective], None, LINE_SEARCHES[line_search], C.byref(k),
                                     dp(xs), dp(ds), dp(gs), C.byref(a))
        if rc != 0:
            self._err("lbfgs_line_search", rc)
        return a.value

    def twoloop(self, g, S, Y):
        h = len(S)
        S = [np.ascontiguousarray(s, np.float64) for s in S]
        Y = [np.ascontiguousarray(y, np.float64) for y in Y]
        sp = (C.c_void_p * h)(*[s.ctypes.data for s in S])
        yp = (C.c_void_p * h)(*[y.ctypes.data for y in Y])
        d = np.zeros(self.n)
        gd = C.c_double()
        rc = lib().lbfgs_dev_twoloop(self.h, np.ascontiguousarray(g, np.float64), sp, yp, h, d,
                                     C.byref(gd))
        if rc != 0:
            self._err("lbfgs_dev_twoloop", rc)
        return d, gd.value

    # ---- profiling ----
    def prof_enable(self, on=True):
        lib().lbfgs_prof_enable(self.h, int(on))

    def prof_reset(self):
        lib().lbfgs_prof_reset(self.h)

    def prof_get(self, kind):
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        rc = lib().lbfgs_prof_get(self.h, KERNELS.index(kind), C.byref(ms), C.byref(n), C.byref(b))
        if rc != 0:
            self._err("lbfgs_prof_get", rc)
        return dict(ms=ms.value, launches=n.value, bytes=b.value)
