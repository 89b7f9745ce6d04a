"""CPU test: the Lanczos vector operations of the C ABI (ovqe_vec_*) are declared alike in include/ovqe_sv.h, in the cffi header
include/ovqe_sv.cdef.h and in the ctypes table of openvqe_amd/_lib.py, and the library exports them."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> C parameter types in order (what header and cdef must spell, and what the ctypes table must mean)
EXPECTED = {
    "ovqe_vec_dot": ["ovqe_handle", "const void *", "const void *", "double *"],
    "ovqe_vec_lanczos_update": ["ovqe_handle", "void *", "const void *", "const void *", "double", "double", "double *"],
    "ovqe_vec_scale": ["ovqe_handle", "void *", "double"],
    "ovqe_vec_axpy": ["ovqe_handle", "void *", "const void *", "double", "int"],
}


def _declarations(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int)\s+(ovqe_vec_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        types = []
        for p in params.split(","):
            p = re.sub(r"\s+", " ", p).strip()
            types.append(re.sub(r"\s*\b[a-z_0-9]+$", "", p).strip() if not p.endswith("*") else p)   # drop the parameter name
        out[name] = types
    return out


def test_vector_operations_agree_between_header_cdef_and_ctypes(gpu_lib):
    from openvqe_amd import _lib
    header = _declarations(os.path.join(ROOT, "include", "ovqe_sv.h"))
    cdef = _declarations(os.path.join(ROOT, "include", "ovqe_sv.cdef.h"))
    assert header == cdef == EXPECTED
    ctype_of = {"ovqe_handle": [ctypes.c_void_p], "void *": [ctypes.c_void_p], "const void *": [ctypes.c_void_p],
                "double": [ctypes.c_double], "int": [ctypes.c_int]}
    raw = ctypes.CDLL(os.path.join(ROOT, "openvqe_amd", "lib", "libovqe_sv.so"))
    for name, params in EXPECTED.items():
        assert hasattr(raw, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params)
        for c_type, arg in zip(params, argtypes):
            if c_type == "double *":      # a ctypes pointer to double, or numpy's float64 array pointer
                assert arg is ctypes.POINTER(ctypes.c_double) or getattr(arg, "_dtype_", None) == "float64" or "float64" in repr(arg), (name, arg)
            else:
                assert arg in ctype_of[c_type], (name, c_type, arg)
