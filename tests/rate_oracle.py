"""The CPU oracle at a chosen rate_bits (tests/rate_oracle/rate_oracle.cpp) -- TEST INFRASTRUCTURE ONLY.

build() compiles the unit with the flags of oracle/Makefile into tests/_scratch/librate_oracle.so; prove() / verify() are
oracle_lib.prove / verify with a rate_bits argument (same config forms, same return values)."""
import ctypes as C
import os
import subprocess
import numpy as np
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rate_oracle", "rate_oracle.cpp")
LIB_PATH = os.path.join(HERE, "_scratch", "librate_oracle.so")
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function", "-DNDEBUG_OFF"]   # oracle/Makefile

_lib = None


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [SRC] + [os.path.join(O.ORACLE_DIR, f) for f in os.listdir(O.ORACLE_DIR) if f.endswith((".cpp", ".hpp", ".inc"))]
    return any(os.path.getmtime(d) > t for d in deps)


def build():
    """Idempotent; writes to a temporary name first so that concurrent test workers never load a half-written library."""
    if not _stale():
        return
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    subprocess.check_call([os.environ.get("CXX", "g++")] + CXXFLAGS + ["-shared", "-o", tmp, SRC])
    os.replace(tmp, LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        u64p = C.POINTER(C.c_uint64)
        L.orc_prove_rate.restype = C.c_int
        L.orc_prove_rate.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_uint, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint,
                                     C.POINTER(u64p), C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
        L.orc_verify_rate.restype = C.c_int
        L.orc_verify_rate.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.POINTER(C.c_char_p)]
        L.orc_free.argtypes = [C.c_void_p]
        if "OMP_NUM_THREADS" not in os.environ:
            L.orc_set_threads(O._effective_cpus())
        _lib = L
    return _lib


def _cfg(config, rate_bits):
    """config as oracle_lib._config_words takes it; None = the oracle's default fields (cap 4, 16 grinding bits, arity 4, final 5)
    with the query count of the rate: ceil(84 / rate_bits)."""
    if config is None:
        config = (4, 16, 4, 5, -(-84 // rate_bits))
    return O._config_words(config)


def prove(kind, num_io, trace, pi, rate_bits, config=None):
    """-> (proof words, seconds)"""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    pi = np.ascontiguousarray(pi, dtype=np.uint64)
    degree_bits = trace.shape[1].bit_length() - 1
    out, nw, secs = C.POINTER(C.c_uint64)(), C.c_size_t(), C.c_double()
    cw = _cfg(config, rate_bits)
    rc = lib().orc_prove_rate(kind, num_io, O.ptr(trace), degree_bits, O.ptr(pi), len(pi), O.ptr(cw), rate_bits, C.byref(out), C.byref(nw), C.byref(secs))
    if rc != 0:
        raise RuntimeError(f"orc_prove_rate failed rc={rc}")
    words = np.ctypeslib.as_array(out, shape=(nw.value,)).copy()
    lib().orc_free(out)
    return words, secs.value


def verify(kind, num_io, words, rate_bits, config=None):
    """-> (0 accepted / negative rejected, reason)"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    why = C.c_char_p()
    cw = _cfg(config, rate_bits)
    rc = lib().orc_verify_rate(kind, num_io, O.ptr(words), len(words), O.ptr(cw), rate_bits, C.byref(why))
    return rc, (why.value or b"").decode()


if __name__ == "__main__":
    build()
