"""CPU-side checks of the row reducer's surface (no GPU compute): lbfgs_reduce_rows is declared with the
documented prototype, exported by the library and bound by the Python layer; every refusal is decided
before any HIP call, so a machine without a GPU gives it too; a missing device is an error code."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-lbfgs_amd")
sys.path.insert(0, PKG)
import lbfgs_amd as L  # noqa: E402

NAME = "lbfgs_reduce_rows"
PROTOTYPE = ("int lbfgs_reduce_rows(int device, int64_t n, int batch, const double* a_dev, int64_t lda, "
             "const double* b_dev, int64_t ldb, const int* active_dev, double* out_dev, void* hip_stream);")
BAD_ARG, ERR_HIP = -1, -2
A, B, ACT, OUT = 0x10000, 0x20000, 0x30000, 0x40000  # dummy addresses, 16-byte aligned: nothing reads them


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        subprocess.run(["make", "-C", PKG, "-j8"], check=True, capture_output=True)


def _header():
    src = open(os.path.join(ROOT, "include", "lbfgs_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)  # comments out
    return re.sub(r"\s+", " ", src)


def test_header_declares_the_prototype():
    h = _header()
    assert PROTOTYPE in h
    assert "#define LBFGS_HIP_ABI_VERSION 3 " in h  # additive: the version stays


def test_library_and_binding_have_the_name():
    _ensure_built()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    assert NAME in L.EXPORTED_SYMBOLS
    assert len(getattr(L.lib(), NAME).argtypes) == PROTOTYPE.split("(", 1)[1].count(",") + 1
    assert callable(L.reduce_rows)


def call(device=0, n=1000, batch=4, a=A, lda=1000, b=B, ldb=1000, active=ACT, out=OUT, stream=None):
    return L.lib().lbfgs_reduce_rows(device, n, batch, a, lda, b, ldb, active, out, stream)


REFUSED = {
    "n = 0": dict(n=0, lda=0, ldb=0),
    "n < 0": dict(n=-1),
    "n above the limit": dict(n=32769, lda=32769, ldb=32769),
    "batch = 0": dict(batch=0),
    "batch < 0": dict(batch=-3),
    "null a": dict(a=None),
    "null out": dict(out=None),
    "a not 8-byte aligned": dict(a=A + 4),
    "b not 8-byte aligned": dict(b=B + 2),
    "out not 8-byte aligned": dict(out=OUT + 1),
    "lda < n": dict(lda=999),
    "ldb between 0 and n": dict(ldb=999),
    "ldb < 0": dict(ldb=-1000),
    "negative device": dict(device=-1),
}


def test_refusals_need_no_device():
    _ensure_built()
    for what, kw in REFUSED.items():
        assert call(**kw) == BAD_ARG, what
        assert call(**dict(dict(active=None), **kw)) == BAD_ARG, what
    # what is not refused at the limits (no device here, or one past the last: LBFGS_ERR_HIP, below)
    past = L.device_count()
    for kw in (dict(n=32768, lda=32768, ldb=0), dict(n=1, lda=1, ldb=1), dict(b=None, ldb=999), dict(a=A + 8, out=OUT + 8),
               dict(ldb=0), dict(batch=1)):
        assert call(device=past, **kw) == ERR_HIP, kw


def test_a_device_past_the_last_is_an_error_code():
    """No device (or an ordinal past the last one): an error code, not a crash, and nothing launched."""
    _ensure_built()
    assert call(device=L.device_count()) == ERR_HIP
