"""Device WriteBatch encode on db_bench-shaped logs: decode's tables -> reps
-> append framing, all in HBM.

Workloads: fill1 and fill100 exactly as tools/bench_batches.py builds them
(16-B keys, 100-B values, 1 GiB image framed by revel_gpu_append_records).
The image is replayed once (verify -> reassemble -> decode); then
revel_gpu_encode_batches is timed on decode's own output (HIP events around
the call: its kernels, the read-back of the per-rep lengths and its
synchronisation), and encode + revel_gpu_append_records; the image they write
is compared byte for byte with the input image.  `lens` is pinned host memory
(revel_gpu_host_alloc).  Prints one JSON line per workload; GiB/s are rep
bytes per second.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_batches import make_reps  # noqa: E402
from revel_amd import gpu  # noqa: E402
from revel_amd._lib import check, lib  # noqa: E402
from revel_amd.gpu import BATCH_ENTRY_DTYPE, BATCH_INFO_DTYPE, LOGICAL_DTYPE, RECORD_DTYPE  # noqa: E402


def run(ctx, name, per_batch, target, iters, warmup):
    L = lib()
    size = 12 + per_batch * 119
    nb = max(1, target // (size + 7))
    dpay = ctx.upload(make_reps(nb, per_batch).reshape(-1))
    img, n, _ = ctx.append_records(dpay, np.full(nb, size, np.uint64))
    dpay.free()
    # replay once: verify -> reassemble -> decode
    nblocks = (n + 32767) // 32768
    counts, first = ctx.alloc(4 * nblocks), ctx.alloc(4 * nblocks)
    check(L.revel_gpu_count_scan_records(ctx.handle, img.ptr, n, counts.ptr, first.ptr, None))
    ctx.sync()
    nphys = int(ctx.d2h(first, 4, np.uint32, 4 * (nblocks - 1))[0]) + int(ctx.d2h(counts, 4, np.uint32,
                                                                                4 * (nblocks - 1))[0])
    phys = ctx.alloc(nphys * RECORD_DTYPE.itemsize)
    check(L.revel_gpu_verify_records(ctx.handle, img.ptr, n, 0, first.ptr, phys.ptr, None))
    logical, payload = ctx.alloc(nphys * LOGICAL_DTYPE.itemsize), ctx.alloc(n)
    nl, pb, ne = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    check(L.revel_gpu_reassemble(ctx.handle, img.ptr, 0, n, phys.ptr, nphys, 1, logical.ptr, payload.ptr,
                                 ctypes.byref(nl), ctypes.byref(pb), None))
    info = ctx.alloc(nl.value * BATCH_INFO_DTYPE.itemsize)
    ents = ctx.alloc((nb * per_batch) * BATCH_ENTRY_DTYPE.itemsize)
    check(L.revel_gpu_decode_batches(ctx.handle, payload.ptr, pb.value, logical.ptr, nl.value, info.ptr, ents.ptr,
                                     nb * per_batch, ctypes.byref(ne), None))
    for b in (counts, first, phys, logical):
        b.free()
    assert nl.value == nb and ne.value == nb * per_batch
    # encode
    plens = ctypes.c_void_p()
    check(L.revel_gpu_host_alloc(ctx.handle, 8 * nb, ctypes.byref(plens)))
    lens = np.ctypeslib.as_array((ctypes.c_uint64 * nb).from_address(plens.value))
    total = ctypes.c_uint64()
    args = (ctx.handle, payload.ptr, pb.value, ents.ptr, ne.value, info.ptr, nb)
    ev = [ctx.event() for _ in range(3)]
    t = {"size": [], "encode": [], "encode_append": []}
    ev[0].record()
    check(L.revel_gpu_encode_batches(*args, None, 0, plens.value, ctypes.byref(total), None))
    ev[1].record()
    ctx.sync()
    first_sizing_ms = ev[0].elapsed_ms(ev[1])
    reps = ctx.alloc(total.value)
    out = ctx.alloc(int(L.revel_log_framed_size(plens.value, nb, 0)))
    for it in range(warmup + iters):
        ev[0].record()
        check(L.revel_gpu_encode_batches(*args, None, 0, plens.value, ctypes.byref(total), None))
        ev[1].record()
        ctx.sync()
        sizing = ev[0].elapsed_ms(ev[1])
        bo, on = ctypes.c_uint64(0), ctypes.c_size_t()
        ev[0].record()
        check(L.revel_gpu_encode_batches(*args, reps.ptr, reps.nbytes, plens.value, ctypes.byref(total), None))
        ev[1].record()
        check(L.revel_gpu_append_records(ctx.handle, reps.ptr, plens.value, nb, ctypes.byref(bo), out.ptr, out.nbytes,
                                         ctypes.byref(on), None))
        ev[2].record()
        ctx.sync()
        if it >= warmup:
            t["size"].append(sizing)
            t["encode"].append(ev[0].elapsed_ms(ev[1]))
            t["encode_append"].append(ev[0].elapsed_ms(ev[2]))
    equal = on.value == n
    step = 64 << 20
    for at in range(0, n if equal else 0, step):  # compared in pieces: no second GiB on the host
        m = min(step, n - at)
        equal = equal and bool((ctx.d2h(out, m, src_offset=at) == ctx.d2h(img, m, src_offset=at)).all())
    lens_ok = bool((lens == size).all())
    check(L.revel_gpu_host_free(ctx.handle, plens.value))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {
        "workload": name, "image_bytes": n, "batches": nb, "entries": int(ne.value), "rep_bytes": int(total.value),
        "image_equal": equal, "lens_ok": lens_ok, "iters": iters, "warmup": warmup,
        "first_sizing_call_ms": round(first_sizing_ms, 4),
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
        "GiB_s": {k: round(total.value / 2**30 / (v / 1e3), 1) for k, v in med.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib", default=None, help="another build of librevel_wal.so (A/B)")
    a = ap.parse_args()
    if a.lib:
        from revel_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    ctx = gpu.GpuContext(0)
    for name, per in [("fill1", 1), ("fill100", 100)]:
        print(json.dumps(run(ctx, name, per, a.bytes, a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
