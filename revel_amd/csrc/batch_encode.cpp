// batch_encode.cpp -- revel_gpu_encode_batches: the C-ABI driver of the device
// WriteBatch encode (sizes -> scan -> lengths -> scan -> headers -> emit),
// write_batch.rs:44-55,67-69,160-166 + db.rs:103-108 for a table of batches.
#include <hip/hip_runtime_api.h>

#include <algorithm>

#include "gpu_internal.h"
#include "revel_wal.h"

using revel::set_error;

extern "C" int revel_gpu_encode_batches(revel_gpu_context* ctx, const void* d_data, uint64_t data_bytes,
                                        const revel_batch_entry* d_entries, size_t nentries,
                                        const revel_batch_info* d_info, size_t nbatches, void* d_reps,
                                        uint64_t reps_cap, uint64_t* lens, uint64_t* reps_bytes, void* stream) {
    if (!ctx || !lens || !reps_bytes) return set_error(REVEL_INVALID_ARGUMENT, "null argument");
    *reps_bytes = 0;
    if (nbatches == 0) return REVEL_OK;
    if (!d_info || (nentries && !d_entries) || (data_bytes && !d_data) || (reps_cap && !d_reps))
        return set_error(REVEL_INVALID_ARGUMENT, "null device buffer");
    const bool sizing = !d_reps;  // reps_cap is 0 here: lens and the total only
    CHECK_CTX(ctx);
    hipStream_t st = revel::pick(ctx, stream);
    const uint64_t ne = nentries, nb = nbatches;
    revel::DeviceScratch S(&ctx->arena);
    // sizes[ne + 1] becomes the entries' destination offsets once E is scanned from it
    uint64_t *sizes = nullptr, *E = nullptr, *blen = nullptr, *roff = nullptr, *tiles = nullptr, *err = nullptr,
             *hdr_seq = nullptr;
    uint32_t* hdr_n = nullptr;
    hipError_t e = S.get(&sizes, ne + 1);
    if (e == hipSuccess) e = S.get(&E, ne + 1);
    if (e == hipSuccess) e = S.get(&blen, nb + 1);
    if (e == hipSuccess) e = S.get(&roff, nb + 1);
    if (e == hipSuccess) e = S.get(&tiles, revel::scan_scratch_words(std::max(ne, nb) + 1));
    if (e == hipSuccess) e = S.get(&err, 1);
    if (e == hipSuccess && !sizing) e = S.get(&hdr_seq, ne);
    if (e == hipSuccess && !sizing) e = S.get(&hdr_n, ne);
    if (e == hipSuccess) e = hipMemsetAsync(err, 0xFF, 8, st);
    if (e == hipSuccess) e = revel::encode_sizes(ctx->di, d_entries, ne, data_bytes, sizes, err, st);
    if (e == hipSuccess) e = revel::exclusive_scan_u64(ctx->di, sizes, E, ne + 1, tiles, st);
    if (e == hipSuccess) e = revel::encode_lengths(ctx->di, d_info, nb, ne, E, blen, err, st);
    if (e == hipSuccess) e = revel::exclusive_scan_u64(ctx->di, blen, roff, nb + 1, tiles, st);
    // The lengths are final here.  With reps to write, they are read back on the context's second stream while
    // the header and emit kernels run on st (fill1's 7.8 M lengths take about as long as its emit kernel).
    hipStream_t copy = st;
    if (!sizing) {
        if (e == hipSuccess && !ctx->enc_copy) e = hipStreamCreateWithFlags(&ctx->enc_copy, hipStreamNonBlocking);
        if (e == hipSuccess && !ctx->enc_lens_ready)
            e = hipEventCreateWithFlags(&ctx->enc_lens_ready, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ctx->enc_lens_ready, st);
        // the kernels check the error word and the total against reps_cap themselves: no sync before them
        if (e == hipSuccess) e = hipMemsetAsync(sizes, 0xFF, (ne + 1) * 8, st);
        if (e == hipSuccess)
            e = revel::encode_emit(ctx->di, d_data, d_entries, ne, d_info, nb, E, roff, err, reps_cap, sizes, hdr_seq, hdr_n,
                                   d_reps, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->enc_copy, ctx->enc_lens_ready, 0);
        if (e == hipSuccess) copy = ctx->enc_copy;
    }
    uint64_t bad = 0, total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(lens, blen, nb * 8, hipMemcpyDeviceToHost, copy);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, err, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, roff + nb, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && copy != st) e = hipStreamSynchronize(copy);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);  // the context's scratch is free before the next call
        if (ctx->enc_copy) (void)hipStreamSynchronize(ctx->enc_copy);
        return revel::hip_fail(e, "encode_batches");
    }
    *reps_bytes = total;
    if (bad != ~0ull) {
        if (bad >> 63)
            return set_error(REVEL_INVALID_ARGUMENT,
                             "encode_batches: entry %llu: type not 0/1, or key/value span outside the %llu data bytes",
                             (unsigned long long)(bad & ~(1ull << 63)), (unsigned long long)data_bytes);
        return set_error(REVEL_INVALID_ARGUMENT, "encode_batches: batch %llu: entry range past the %zu table entries",
                         (unsigned long long)bad, nentries);
    }
    if (!sizing && total > reps_cap)
        return set_error(REVEL_INVALID_ARGUMENT, "encode_batches: %llu rep bytes exceed capacity %llu",
                         (unsigned long long)total, (unsigned long long)reps_cap);
    return REVEL_OK;
}
