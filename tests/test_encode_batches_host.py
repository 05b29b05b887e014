"""revel_gpu_encode_batches on a host without a GPU: the symbol, its prototype
and the null-argument checks that come before any GPU use."""
import ctypes
import os
import re

import numpy as np

import revel_amd
from revel_amd import _lib
from conftest import ROOT


def header_prototype(name):
    with open(os.path.join(ROOT, "include", "revel_wal.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{)]*)\)\s*;", text)
    assert m, f"{name} is not declared in revel_wal.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_encode_symbol_matches_header():
    args = header_prototype("revel_gpu_encode_batches")
    assert args == ["revel_gpu_context* ctx", "const void* d_data", "uint64_t data_bytes",
                    "const revel_batch_entry* d_entries", "size_t nentries", "const revel_batch_info* d_info",
                    "size_t nbatches", "void* d_reps", "uint64_t reps_cap", "uint64_t* lens", "uint64_t* reps_bytes",
                    "void* stream"]
    L = revel_amd.lib()
    assert hasattr(L, "revel_gpu_encode_batches")
    res, argtypes = _lib.SIGNATURES["revel_gpu_encode_batches"]
    assert res is ctypes.c_int and len(argtypes) == len(args)
    # u64 / size_t / pointer arguments are all 8 bytes wide where the header says so
    for a, t in zip(args, argtypes):
        assert ctypes.sizeof(t) == 8, (a, t)


def test_encode_null_arguments_need_no_gpu():
    """Null ctx, lens or reps_bytes: INVALID_ARGUMENT before the context is
    looked at (the stand-in context below is 4 KiB of zeros, not a context)."""
    L = revel_amd.lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    lens = np.full(3, 77, np.uint64)
    total = ctypes.c_uint64(99)
    rb = ctypes.byref(total)
    for args in [(None, lens.ctypes.data, rb), (ctx, None, rb), (ctx, lens.ctypes.data, None)]:
        rc = L.revel_gpu_encode_batches(args[0], None, 0, None, 0, None, 3, None, 0, args[1], args[2], None)
        assert rc == _lib.INVALID_ARGUMENT
        assert b"null" in L.revel_last_error()
    assert (lens == 77).all() and total.value == 99
    # nothing to encode: OK and 0 bytes, still without a look at the context
    assert L.revel_gpu_encode_batches(ctx, None, 0, None, 0, None, 0, None, 0, lens.ctypes.data, rb, None) == _lib.OK
    assert total.value == 0
