// batch_encode.hip -- device WriteBatch encode: decoded batch tables -> reps
// (gfx950).
//
// Reference: write_batch.rs:44-55 (put / delete append tag, varint32 key
// length, key [, varint32 value length, value]), :160-166 (count), :67-69
// (set_sequence), coding.rs:18-49 (encode_varint32); db.rs:103-108 hands
// contents() to add_record.  The inverse of batch.hip, for a whole table of
// batches at once.
//
// Layout: entry i's encoded size is a function of its own row, so an exclusive
// u64 scan of the sizes (E) places every entry inside its batch; a batch's rep
// length is 12 + E[first + n] - E[first] and a second scan of the lengths
// places the reps.  k_enc_head (one lane per batch) stamps each of its entries
// with its destination offset and hands the header fields to the first one;
// entries no batch covers keep the stamp ~0 and are skipped.  k_enc_emit then
// writes the headers and copies every key
// and value with the span engine of device_common.h.  No atomics on the data
// path (the only atomic is the error word's min, taken on bad input), no LDS.
//
// Bad input never reaches a copy: the size pass checks every entry's type and
// spans, the length pass every batch's entry range, both record the lowest bad
// index in *err, and k_enc_head / k_enc_emit return at once unless *err is
// clear and the scanned total fits the caller's capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device_common.h"

using namespace revel;

namespace {

// The error word: ~0 = none; else the lowest bad batch index, or with
// kEncEntryBit the lowest bad entry index when every batch range is good.
constexpr uint64_t kEncNone = ~0ull;
constexpr uint64_t kEncEntryBit = 1ull << 63;

__device__ __forceinline__ uint32_t varint_len(uint32_t v) {
    return 1u + (v >= (1u << 7)) + (v >= (1u << 14)) + (v >= (1u << 21)) + (v >= (1u << 28));
}
// byte k (< n = varint_len(v)) of v's minimal varint32 (coding.rs:18-49)
__device__ __forceinline__ uint8_t varint_byte(uint32_t v, uint32_t k, uint32_t n) {
    return (uint8_t)(((v >> (7u * k)) & 127u) | (k + 1u < n ? 128u : 0u));
}
__device__ __forceinline__ bool span_ok(uint64_t off, uint32_t len, uint64_t data_bytes) {
    return off <= data_bytes && len <= data_bytes - off;
}
__device__ __forceinline__ void note_error(uint64_t* err, uint64_t code) {
    atomicMin(reinterpret_cast<unsigned long long*>(err), (unsigned long long)code);
}

// sizes[i] = encoded bytes of entry i (i < n), sizes[n] = 0 (so the scan's
// last element is the sum).  Every entry of the table is checked, covered by a
// batch or not.
__global__ void k_enc_size(const revel_batch_entry* __restrict__ entries, uint64_t n, uint64_t data_bytes,
                           uint64_t* __restrict__ sizes, uint64_t* __restrict__ err) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t size = 0;
        if (i < n) {
            const uint64_t koff = entries[i].key_offset, voff = entries[i].value_offset;
            const uint32_t klen = entries[i].key_len, vlen = entries[i].value_len;
            const uint32_t type = entries[i].type;
            bool ok = type <= REVEL_TYPE_VALUE && span_ok(koff, klen, data_bytes);
            size = 1u + varint_len(klen) + (uint64_t)klen;
            if (type == REVEL_TYPE_VALUE) {
                ok = ok && span_ok(voff, vlen, data_bytes);
                size += varint_len(vlen) + (uint64_t)vlen;
            }
            if (!ok) {
                note_error(err, kEncEntryBit | i);
                size = 0;
            }
        }
        sizes[i] = size;
    }
}

// blen[b] = rep length of batch b (b < nb), blen[nb] = 0.
__global__ void k_enc_len(const revel_batch_info* __restrict__ info, uint64_t nb, uint64_t nentries,
                          const uint64_t* __restrict__ E, uint64_t* __restrict__ blen, uint64_t* __restrict__ err) {
    for (uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; b <= nb; b += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t len = 0;
        if (b < nb) {
            const uint64_t first = info[b].first_entry, n = info[b].nentries;
            len = REVEL_BATCH_HEADER;
            if (first <= nentries && n <= nentries - first)
                len += E[first + n] - E[first];
            else
                note_error(err, b);
        }
        blen[b] = len;
    }
}

// ent_dst[i] = rep offset of entry i's tag byte for the entries of each batch
// (ent_dst is preset to ~0).  A batch's first entry also carries kEncFirstBit
// and the header fields in hdr_seq / hdr_n: k_enc_emit writes the 12-byte
// header next to that entry's bytes (a 12-byte store of its own per batch, at
// any alignment, cost 0.36 ms for 7.8 M batches).  Only a batch without
// entries gets its header here.
constexpr uint64_t kEncFirstBit = 1ull << 63;
__global__ void k_enc_head(const revel_batch_info* __restrict__ info, uint64_t nb, const uint64_t* __restrict__ E,
                           const uint64_t* __restrict__ roff, const uint64_t* __restrict__ err, uint64_t cap,
                           uint8_t* __restrict__ reps, uint64_t* __restrict__ ent_dst,
                           uint64_t* __restrict__ hdr_seq, uint32_t* __restrict__ hdr_n) {
    if (*err != kEncNone || roff[nb] > cap) return;
    for (uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t seq = info[b].sequence, first = info[b].first_entry;
        const uint32_t n = info[b].nentries;
        const uint64_t at = roff[b];
        if (n == 0) {
            uint8_t* p = reps + at;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) p[k] = (uint8_t)(seq >> (8u * k));
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) p[8 + k] = 0;
            continue;
        }
        hdr_seq[first] = seq;
        hdr_n[first] = n;
        ent_dst[first] = (at + REVEL_BATCH_HEADER) | kEncFirstBit;
        const uint64_t body = at + REVEL_BATCH_HEADER - E[first];
        for (uint64_t k = first + 1; k < first + n; ++k) ent_dst[k] = body + E[k];
    }
}

// Entries, kEncEpg per 8-lane group and visit; each entry is a few header
// bytes (tag + varints, one byte per lane of the group) and two spans, key and
// value, copied by the span engine of device_common.h.
#ifndef REVEL_ENC_EPG
#define REVEL_ENC_EPG 2
#endif
// entries per 8-lane group and visit: 1 = 125 VGPRs, 4 waves per SIMD; 2 = 189 VGPRs, 2 waves per SIMD, the
// same spans in flight per SIMD either way (still 189 with the header fields).  Measured before the lengths'
// second stream and the header fields, the whole call on 1 GiB of 16-B keys + 100-B values: 3.20 / 3.10 ms at
// one batch per entry, 1.66 / 1.67 ms at 100 entries per batch.
constexpr uint32_t kEncEpg = REVEL_ENC_EPG;
__global__ __launch_bounds__(256) void k_enc_emit(const uint8_t* __restrict__ data,
                                                  const revel_batch_entry* __restrict__ entries, uint64_t n,
                                                  const uint64_t* __restrict__ ent_dst,
                                                  const uint64_t* __restrict__ hdr_seq,
                                                  const uint32_t* __restrict__ hdr_n,
                                                  const uint64_t* __restrict__ total, const uint64_t* __restrict__ err,
                                                  uint64_t cap, uint8_t* __restrict__ reps) {
    if (*err != kEncNone || *total > cap) return;
    using Visit = SpanVisit<kEncEpg>;
    const uint8_t* safe = reinterpret_cast<const uint8_t*>(err);  // 8 readable bytes for the idle lanes' loads
    const uint32_t lane = lane_id(), gl = lane & 7u;
    const uint64_t start = Visit::first(), stride = Visit::stride();
    // descriptors one visit ahead, clamped loads + ~0 for "nothing here"
    uint64_t dst_n[kEncEpg], koff_n[kEncEpg], voff_n[kEncEpg], seq_n[kEncEpg];
    uint32_t klen_n[kEncEpg], vlen_n[kEncEpg], type_n[kEncEpg], cnt_n[kEncEpg];
    auto fetch = [&](uint64_t base) {
#pragma unroll
        for (uint32_t j = 0; j < kEncEpg; ++j) {
            const uint64_t k = Visit::index(base, j);
            const uint64_t kc = k < n ? k : n - 1;
            const uint64_t d = ent_dst[kc];
            dst_n[j] = k < n ? d : kEncNone;
            koff_n[j] = entries[kc].key_offset;
            voff_n[j] = entries[kc].value_offset;
            klen_n[j] = entries[kc].key_len;
            vlen_n[j] = entries[kc].value_len;
            type_n[j] = entries[kc].type;
            seq_n[j] = hdr_seq[kc];  // meaningful for a batch's first entry only
            cnt_n[j] = hdr_n[kc];
        }
    };
    if (start < n) fetch(start);
    for (uint64_t base = start; base < n; base += stride) {
        // spans of entry j, data -> reps: 2 j = key, 2 j + 1 = value (dead for a deletion or a skipped entry)
        Span s[2 * kEncEpg];
        uint8_t* tag_at[kEncEpg];
        uint32_t klen[kEncEpg], vlen[kEncEpg], type[kEncEpg], cnt[kEncEpg];
        uint64_t seq[kEncEpg];
        bool live[kEncEpg], first[kEncEpg];
#pragma unroll
        for (uint32_t j = 0; j < kEncEpg; ++j) {
            live[j] = dst_n[j] != kEncNone;
            first[j] = live[j] && (dst_n[j] & kEncFirstBit) != 0;
            seq[j] = seq_n[j];
            cnt[j] = cnt_n[j];
            klen[j] = klen_n[j];
            vlen[j] = vlen_n[j];
            type[j] = type_n[j];
            const bool value = live[j] && type[j] == REVEL_TYPE_VALUE;
            const uint64_t tag = live[j] ? dst_n[j] & ~kEncFirstBit : 0u;
            tag_at[j] = reps + tag;
            s[2 * j] = {koff_n[j], tag + 1u + varint_len(klen[j]), live[j] ? klen[j] : 0u};
            s[2 * j + 1] = {voff_n[j], s[2 * j].dst + klen[j] + varint_len(vlen[j]), value ? vlen[j] : 0u};
        }
        if (base + stride < n) fetch(base + stride);
        TinyCopy c[2 * kEncEpg];
        spans_load(data, reps, s, lane, safe, c);
        // tag + key-length varint (lanes 0..vk), value-length varint (lanes 0..vv-1): behind the loads
#pragma unroll
        for (uint32_t j = 0; j < kEncEpg; ++j) {
            const uint32_t vk = varint_len(klen[j]), vv = varint_len(vlen[j]);
            if (first[j]) {  // the batch header in front of its first entry: sequence, count
                uint8_t* h = tag_at[j] - REVEL_BATCH_HEADER;
                h[gl] = (uint8_t)(seq[j] >> (8u * gl));
                if (gl < 4u) h[8u + gl] = (uint8_t)(cnt[j] >> (8u * gl));
            }
            if (live[j] && gl <= vk) tag_at[j][gl] = gl == 0 ? (uint8_t)type[j] : varint_byte(klen[j], gl - 1u, vk);
            if (live[j] && type[j] == REVEL_TYPE_VALUE && gl < vv)
                reps[s[2 * j].dst + klen[j] + gl] = varint_byte(vlen[j], gl, vv);
        }
        spans_finish(data, reps, s, lane, c);
    }
}

uint32_t grid_for(const revel::DeviceInfo& di, uint64_t n, uint64_t per_block) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)di.num_cu * 8, (n + per_block - 1) / per_block));
}

}  // namespace

namespace revel {

hipError_t encode_sizes(const DeviceInfo& di, const revel_batch_entry* d_entries, uint64_t nentries,
                        uint64_t data_bytes, uint64_t* d_sizes, uint64_t* d_err, hipStream_t st) {
    hipLaunchKernelGGL(k_enc_size, dim3(grid_for(di, nentries + 1, 256)), dim3(256), 0, st, d_entries, nentries,
                       data_bytes, d_sizes, d_err);
    return hipGetLastError();
}

hipError_t encode_lengths(const DeviceInfo& di, const revel_batch_info* d_info, uint64_t nbatches, uint64_t nentries,
                          const uint64_t* d_E, uint64_t* d_blen, uint64_t* d_err, hipStream_t st) {
    hipLaunchKernelGGL(k_enc_len, dim3(grid_for(di, nbatches + 1, 256)), dim3(256), 0, st, d_info, nbatches, nentries,
                       d_E, d_blen, d_err);
    return hipGetLastError();
}

hipError_t encode_emit(const DeviceInfo& di, const void* d_data, const revel_batch_entry* d_entries, uint64_t nentries,
                       const revel_batch_info* d_info, uint64_t nbatches, const uint64_t* d_E, const uint64_t* d_roff,
                       const uint64_t* d_err, uint64_t cap, uint64_t* d_ent_dst, uint64_t* d_hdr_seq, uint32_t* d_hdr_n,
                       void* d_reps, hipStream_t st) {
    hipLaunchKernelGGL(k_enc_head, dim3(grid_for(di, nbatches, 256)), dim3(256), 0, st, d_info, nbatches, d_E, d_roff,
                       d_err, cap, static_cast<uint8_t*>(d_reps), d_ent_dst, d_hdr_seq, d_hdr_n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nentries == 0) return e;
    using Visit = SpanVisit<kEncEpg>;
    hipLaunchKernelGGL(k_enc_emit, dim3(Visit::grid(di, nentries)), dim3(Visit::kThreads), 0, st,
                       static_cast<const uint8_t*>(d_data), d_entries, nentries, d_ent_dst, d_hdr_seq, d_hdr_n,
                       d_roff + nbatches, d_err, cap, static_cast<uint8_t*>(d_reps));
    return hipGetLastError();
}

}  // namespace revel
