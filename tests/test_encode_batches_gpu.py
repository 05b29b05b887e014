"""Device WriteBatch encode (revel_gpu_encode_batches) against the oracle's
encoder (oracle/write_batch_oracle.py WriteBatch.put / delete / set_sequence /
contents): every expected rep is built by the oracle, never by the library."""
import ctypes
import re

import numpy as np
import pytest

from revel_amd._lib import INVALID_ARGUMENT, OK, RevelError, check, lib
from revel_amd.gpu import BATCH_ENTRY_DTYPE, BATCH_INFO_DTYPE
from oracle import oracle_c as oc
from oracle import write_batch_oracle as wb
from tests_gen import batch_log, malformed_batches

pytestmark = pytest.mark.gpu


# ---- oracle side ----
def oracle_rep(seq, ops):
    """ops: (type, key, value) in order -> contents() after set_sequence(seq)."""
    b = wb.WriteBatch()
    for t, key, val in ops:
        if t == wb.TYPE_VALUE:
            b.put(key, val)
        else:
            b.delete(key)
    b.set_sequence(seq)
    return b.contents()


def oracle_reencode(rep, keep=lambda t: True):
    """The rep the oracle builds from what it decodes out of `rep`."""
    _, seq, _, ents = wb.decode(rep)
    return oracle_rep(seq, [(t, k, v) for _, t, k, v in ents if keep(t)])


# ---- device side ----
class Tables:
    """Caller-built data buffer + entry / info tables, as decode lays them out."""

    def __init__(self, rng=None):
        self.data = bytearray()
        self.ents = []
        self.infos = []
        self.rng = rng

    def blob(self, b, residue=None):
        if residue is not None:
            self.data += bytes((residue - len(self.data)) % 16)
        off = len(self.data)
        self.data += b
        return off

    def entry(self, t, key, val=b"", residue=None, **stale):
        ko = self.blob(key, residue)
        vo = self.blob(val) if t == wb.TYPE_VALUE else stale.get("value_offset", ko + len(key))
        e = np.zeros((), BATCH_ENTRY_DTYPE)
        e["key_offset"], e["key_len"], e["value_offset"], e["type"] = ko, len(key), vo, t
        e["value_len"] = len(val) if t == wb.TYPE_VALUE else stale.get("value_len", 0)
        e["sequence"], e["batch"] = stale.get("sequence", 0), stale.get("batch", 0)
        self.ents.append(e)
        return len(self.ents) - 1

    def batch(self, seq, first, n, count=0, status=0):
        i = np.zeros((), BATCH_INFO_DTYPE)
        i["sequence"], i["first_entry"], i["nentries"], i["count"], i["status"] = seq, first, n, count, status
        self.infos.append(i)

    def upload(self, ctx):
        data = np.frombuffer(bytes(self.data), np.uint8)
        ents = np.array(self.ents, BATCH_ENTRY_DTYPE) if self.ents else np.zeros(0, BATCH_ENTRY_DTYPE)
        infos = np.array(self.infos, BATCH_INFO_DTYPE)
        return (ctx.upload(data), len(data), ctx.upload(ents.view(np.uint8)), len(ents),
                ctx.upload(infos.view(np.uint8)), len(infos))


def encode(ctx, tables):
    reps, lens, total = ctx.encode_batches_device(*tables)
    return (ctx.d2h(reps, total).tobytes() if total else b""), lens, total


def check_encode(ctx, tables, want):
    got, lens, total = encode(ctx, tables)
    assert [int(x) for x in lens] == [len(r) for r in want]
    assert total == sum(len(r) for r in want)
    at = 0
    for b, r in enumerate(want):  # per rep first: a mismatch names its batch
        assert got[at:at + len(r)] == r, f"rep {b} at byte {at}"
        at += len(r)
    assert got == b"".join(want)


def decoded_tables(ctx, img):
    """WAL image -> verify -> reassemble -> decode, everything left in HBM."""
    d = ctx.upload(np.frombuffer(img, dtype=np.uint8))
    events, nl, pay, pb, _ = ctx.reassemble_device(d, len(img))
    info, ent, ne = ctx.decode_batches_device(pay, pb, events, nl)
    return pay, pb, ent, ne, info, nl


def raw_encode(ctx, tables, reps_ptr, cap):
    data, nbytes, ent, ne, info, nb = tables
    lens = np.full(max(1, nb), 0xDEAD, np.uint64)
    total = ctypes.c_uint64(0xDEAD)
    rc = lib().revel_gpu_encode_batches(ctx.handle, data.ptr, nbytes, ent.ptr, ne, info.ptr, nb, reps_ptr, cap,
                                        lens.ctypes.data, ctypes.byref(total), None)
    return rc, lens[:nb], total.value, (lib().revel_last_error() or b"").decode()


@pytest.fixture(scope="module")
def random_log(gpu_ctx):
    """batch_log(rng(41), 60, big_every=17): 70 000-B multi-fragment values in
    batches 16, 33, 50; the oracle reps and the device tables decode made."""
    reps = batch_log(np.random.default_rng(41), 60, big_every=17)
    want = [oracle_reencode(r) for r in reps]
    tables = decoded_tables(gpu_ctx, oc.write_image(reps))
    return reps, want, tables


# ---- 1. round trip of a random log ----
def test_round_trip_random_log(gpu_ctx, random_log):
    reps, want, tables = random_log
    assert want == reps  # CPU: for minimal-varint, right-count reps the oracle re-encode is the identity
    assert sum(len(r) for r in reps) < 4 << 20 and any(len(r) > 70000 for r in reps)
    assert tables[5] == len(reps)
    check_encode(gpu_ctx, tables, want)
    for bo in (0, 32761):
        img, n, new_bo = gpu_ctx.write_batches(*tables, block_offset=bo)
        ref = oc.write_image(want, bo)
        assert n == len(ref) and new_bo == (bo + len(ref)) % 32768
        assert gpu_ctx.d2h(img, n).tobytes() == ref


# ---- 2. length edges: varint widths, kTinyCopy = 140 and the 1 KiB copy class ----
EDGE_LENGTHS = [0, 1, 15, 16, 17, 127, 128, 129, 139, 140, 141, 1023, 1024, 1025, 16383, 16384, 16385, 70000]


def test_length_edges(gpu_ctx):
    """45 puts whose key lengths walk EDGE_LENGTHS (i mod 18) and whose value
    lengths walk them with stride 7 (7 i + 5 mod 18: every length is a key's and
    a value's, tiny keys meet large values and the reverse), each followed by
    the deletion of its key: one 90-entry batch of 758 789 bytes in the
    oracle, sequence 2**40 + 3."""
    rng = np.random.default_rng(42)
    n = len(EDGE_LENGTHS)
    t, ops = Tables(), []
    for i in range(45):
        key = rng.integers(0, 256, EDGE_LENGTHS[i % n], dtype="u1").tobytes()
        val = rng.integers(0, 256, EDGE_LENGTHS[(7 * i + 5) % n], dtype="u1").tobytes()
        t.entry(wb.TYPE_VALUE, key, val)
        t.entry(wb.TYPE_DELETION, key)
        ops += [(wb.TYPE_VALUE, key, val), (wb.TYPE_DELETION, key, b"")]
    assert {len(k) for _, k, _ in ops} == set(EDGE_LENGTHS) == {len(v) for tp, _, v in ops if tp == wb.TYPE_VALUE}
    seq = 2**40 + 3
    t.batch(seq, 0, 90)
    want = oracle_rep(seq, ops)
    st, dseq, cnt, ents = wb.decode(want)
    assert (st, dseq, cnt, len(ents), len(want)) == (wb.OK, seq, 90, 90, 758789)
    check_encode(gpu_ctx, t.upload(gpu_ctx), [want])


# ---- 3. every source residue x every destination residue ----
def test_alignments(gpu_ctx):
    """A 37-B key and a 150-B value (a tiny and a group copy) at all 16 x 16
    (source, destination) residues mod 16: the source shifted by padding the
    data buffer, the destination by a preceding batch whose single key has
    length 0..15."""
    rng = np.random.default_rng(7)
    t, want, seen, at = Tables(), [], set(), 0
    for s in range(16):
        for d in range(16):
            pad = (d - at - 14) % 16  # the shim rep is 12 + tag + varint + pad bytes
            shim = rng.integers(0, 256, pad, dtype="u1").tobytes()
            e = t.entry(wb.TYPE_DELETION, shim)
            t.batch(1000 + e, e, 1)
            want.append(oracle_rep(1000 + e, [(wb.TYPE_DELETION, shim, b"")]))
            at += len(want[-1])
            key = rng.integers(0, 256, 37, dtype="u1").tobytes()
            val = rng.integers(0, 256, 150, dtype="u1").tobytes()
            e = t.entry(wb.TYPE_VALUE, key, val, residue=s)
            assert t.ents[e]["key_offset"] % 16 == s
            seen.add((s, at % 16))
            t.batch(2000 + e, e, 1)
            want.append(oracle_rep(2000 + e, [(wb.TYPE_VALUE, key, val)]))
            at += len(want[-1])
    assert len(seen) == 256
    check_encode(gpu_ctx, t.upload(gpu_ctx), want)


# ---- 4. table shapes the decoder never produces ----
def test_caller_built_table_shapes(gpu_ctx):
    """Empty batches first, in the middle and last; batches out of table
    order; entries no batch covers; stale .batch / .sequence / .count /
    .status and a deletion's stale value fields."""
    rng = np.random.default_rng(11)
    t, ops = Tables(), []
    for i in range(40):
        key = rng.integers(0, 256, int(rng.integers(0, 300)), dtype="u1").tobytes()
        if i % 3 == 1:
            t.entry(wb.TYPE_DELETION, key, sequence=int(rng.integers(0, 2**63)), batch=0xDEADBEEF,
                    value_offset=2**60, value_len=2**31)
            ops.append((wb.TYPE_DELETION, key, b""))
        else:
            val = rng.integers(0, 256, int(rng.integers(0, 2000)), dtype="u1").tobytes()
            t.entry(wb.TYPE_VALUE, key, val, sequence=int(rng.integers(0, 2**63)), batch=i * 977)
            ops.append((wb.TYPE_VALUE, key, val))
    # entries 7..9 and 35..39 are covered by no batch
    ranges = [(3, 0), (22, 13), (10, 12), (22, 0), (0, 7), (40, 0)]
    want = []
    for b, (first, n) in enumerate(ranges):
        seq = 2**63 + 5 * b
        t.batch(seq, first, n, count=999 - b, status=(b % 5) + 1)
        want.append(oracle_rep(seq, ops[first:first + n]))
    assert [len(want[b]) for b in (0, 3, 5)] == [12, 12, 12]
    check_encode(gpu_ctx, t.upload(gpu_ctx), want)


def test_filtered_rewrite(gpu_ctx, random_log):
    """Drop every deletion from the decoded tables on the host, renumber
    first_entry / nentries, encode: the oracle built the same way."""
    reps, _, (pay, pb, ent, ne, info, nb) = random_log
    ents = gpu_ctx.d2h(ent, ne * BATCH_ENTRY_DTYPE.itemsize).view(BATCH_ENTRY_DTYPE)
    infos = gpu_ctx.d2h(info, nb * BATCH_INFO_DTYPE.itemsize).view(BATCH_INFO_DTYPE).copy()
    keep = ents["type"] == wb.TYPE_VALUE
    assert 0 < keep.sum() < len(ents)
    before = np.concatenate([[0], np.cumsum(keep)])
    for i in range(nb):
        f, n = int(infos["first_entry"][i]), int(infos["nentries"][i])
        infos["first_entry"][i], infos["nentries"][i] = before[f], before[f + n] - before[f]
    kept = np.ascontiguousarray(ents[keep])
    tables = (pay, pb, gpu_ctx.upload(kept.view(np.uint8)), len(kept), gpu_ctx.upload(infos.view(np.uint8)), nb)
    want = [oracle_reencode(r, keep=lambda t: t == wb.TYPE_VALUE) for r in reps]
    assert sum(len(r) for r in want) < sum(len(r) for r in reps)
    check_encode(gpu_ctx, tables, want)
    img, n, _ = gpu_ctx.write_batches(*tables)
    assert gpu_ctx.d2h(img, n).tobytes() == oc.write_image(want)


# ---- 5. many batches: more than one scan tile of batches and of entries ----
def test_many_batches(gpu_ctx):
    reps = batch_log(np.random.default_rng(43), 9000, max_entries=3, max_key=40, max_value=200, big_every=1501)
    # the malformed batches that decode (>= 12 bytes): what decode returned for them is re-encoded,
    # so a non-minimal varint or a wrong count comes back in the oracle's minimal form
    cases = [r for _, r, st in malformed_batches() if st != wb.TOO_SMALL]
    for k, r in enumerate(cases):
        reps.insert(40 * k + 7, r)
    assert len(reps) > 8 * 1024 and sum(len(r) for r in reps) < 4 << 20
    want = [oracle_reencode(r) for r in reps]
    assert sum(a != b for a, b in zip(want, reps)) >= 5
    tables = decoded_tables(gpu_ctx, oc.write_image(reps))
    assert tables[5] == len(reps) and tables[3] > 8 * 1024  # scan tiles are 1 024 elements
    check_encode(gpu_ctx, tables, want)


# ---- 6. capacity and errors ----
def test_capacity_and_errors(gpu_ctx):
    reps = batch_log(np.random.default_rng(44), 20)
    want = [oracle_reencode(r) for r in reps]
    total = sum(len(r) for r in want)
    tables = decoded_tables(gpu_ctx, oc.write_image(reps))
    pay, pb, ent, ne, info, nb = tables
    # sizing call
    rc, lens, got_total, _ = raw_encode(gpu_ctx, tables, None, 0)
    assert rc == OK and got_total == total and [int(x) for x in lens] == [len(r) for r in want]
    # canary-filled reps buffer with a guard zone behind the capacity
    guard = 4096
    reps_d = gpu_ctx.alloc(total + guard)

    def canary():
        gpu_ctx.memset(reps_d, 0xA5, total + guard)
        gpu_ctx.sync()

    def untouched(upto):
        buf = gpu_ctx.d2h(reps_d, total + guard)
        return bool((buf[upto:] == 0xA5).all()) if upto else bool((buf == 0xA5).all())

    canary()
    rc, lens, got_total, msg = raw_encode(gpu_ctx, tables, reps_d.ptr, total - 1)
    assert rc == INVALID_ARGUMENT and got_total == total and [int(x) for x in lens] == [len(r) for r in want]
    assert str(total) in msg and untouched(0)
    # exact capacity: the reps, and nothing behind them
    rc, _, got_total, _ = raw_encode(gpu_ctx, tables, reps_d.ptr, total)
    assert rc == OK and got_total == total
    assert gpu_ctx.d2h(reps_d, total).tobytes() == b"".join(want) and untouched(total)

    ents = gpu_ctx.d2h(ent, ne * BATCH_ENTRY_DTYPE.itemsize).view(BATCH_ENTRY_DTYPE)
    infos = gpu_ctx.d2h(info, nb * BATCH_INFO_DTYPE.itemsize).view(BATCH_INFO_DTYPE)

    def bad_call(new_ents=None, new_infos=None):
        t = (pay, pb, gpu_ctx.upload(new_ents.view(np.uint8)) if new_ents is not None else ent, ne,
             gpu_ctx.upload(new_infos.view(np.uint8)) if new_infos is not None else info, nb)
        canary()
        rc, _, _, msg = raw_encode(gpu_ctx, t, reps_d.ptr, total)
        assert rc == INVALID_ARGUMENT, msg
        assert untouched(total)  # contents unspecified, the bytes behind the capacity are not
        return msg

    keyed = [int(i) for i in np.flatnonzero(ents["key_len"] > 0)]
    lo, hi = keyed[len(keyed) // 3], keyed[2 * len(keyed) // 3]
    # a key span ending at data_bytes + 1
    e2 = ents.copy()
    for i in (hi, lo):
        e2["key_offset"][i] = pb + 1 - int(e2["key_len"][i])
    assert int(re.search(r"entry (\d+)", bad_call(new_ents=e2)).group(1)) == lo
    # a value span ending past the data
    vals = [int(i) for i in np.flatnonzero((ents["type"] == 1) & (ents["value_len"] > 0))]
    e2 = ents.copy()
    e2["value_offset"][vals[-1]] = pb + 1 - int(e2["value_len"][vals[-1]])
    assert int(re.search(r"entry (\d+)", bad_call(new_ents=e2)).group(1)) == vals[-1]
    # a type of 2
    e2 = ents.copy()
    e2["type"][[hi, lo + 1]] = 2
    assert int(re.search(r"entry (\d+)", bad_call(new_ents=e2)).group(1)) == lo + 1
    # an entry range past the table (and a bad entry too: the batch is named)
    i2 = infos.copy()
    i2["nentries"][7] = ne - int(i2["first_entry"][7]) + 1
    i2["first_entry"][12] = ne + 1
    e2 = ents.copy()
    e2["type"][0] = 9
    assert int(re.search(r"batch (\d+)", bad_call(new_ents=e2, new_infos=i2)).group(1)) == 7
    # the same checks in the sizing call
    t = (pay, pb, ent, ne, gpu_ctx.upload(i2.view(np.uint8)), nb)
    rc, _, _, msg = raw_encode(gpu_ctx, t, None, 0)
    assert rc == INVALID_ARGUMENT and "batch 7" in msg
    # nothing to encode
    rc, _, got_total, _ = raw_encode(gpu_ctx, (pay, pb, ent, ne, info, 0), reps_d.ptr, total)
    assert rc == OK and got_total == 0
    reps0, lens0, total0 = gpu_ctx.encode_batches_device(pay, pb, ent, ne, info, 0)
    assert len(lens0) == 0 and total0 == 0
    # a good call on the same context after all the refused ones
    check_encode(gpu_ctx, tables, want)
    with pytest.raises(RevelError) as err:
        check(lib().revel_gpu_encode_batches(gpu_ctx.handle, pay.ptr, pb, ent.ptr, ne, info.ptr, nb, None, 5,
                                             lens.ctypes.data, ctypes.byref(ctypes.c_uint64()), None))
    assert err.value.code == INVALID_ARGUMENT  # a capacity without a buffer


# ---- 7. offsets past 2^32 ----
def test_rep_above_4_gib(gpu_ctx):
    """A rep of more than 4 GiB (130 puts of one 32 MiB value) and a small
    batch behind it: lengths, the total and the destination offsets are u64.
    The head, the last entry of the large rep (its bytes lie past 2^32) and the
    whole small rep are compared."""
    rng = np.random.default_rng(5)
    big = 32 << 20
    t = Tables()
    t.data += rng.integers(0, 256, big, dtype="u1").tobytes()
    nput = 130
    for _ in range(nput):
        e = np.zeros((), BATCH_ENTRY_DTYPE)
        e["key_offset"], e["key_len"], e["value_offset"], e["value_len"], e["type"] = 3, 5, 0, big, wb.TYPE_VALUE
        t.ents.append(e)
    tail_key, tail_val = b"after-4-GiB", rng.integers(0, 256, 777, dtype="u1").tobytes()
    t.entry(wb.TYPE_VALUE, tail_key, tail_val)
    t.batch(9, 0, nput)
    t.batch(2**32 + 1, nput, 1)
    data = bytes(t.data)
    entry = oracle_rep(0, [(wb.TYPE_VALUE, data[3:8], data[:big])])[12:]
    small = oracle_rep(2**32 + 1, [(wb.TYPE_VALUE, tail_key, tail_val)])
    big_len = 12 + nput * len(entry)
    assert big_len > 2**32
    reps, lens, total = gpu_ctx.encode_batches_device(*t.upload(gpu_ctx))
    assert [int(x) for x in lens] == [big_len, len(small)] and total == big_len + len(small)
    head = gpu_ctx.d2h(reps, 12 + len(entry)).tobytes()
    assert head == oracle_rep(9, [(wb.TYPE_DELETION, b"", b"")] * nput)[:12] + entry  # the oracle's header for 130 entries
    last = gpu_ctx.d2h(reps, len(entry), src_offset=big_len - len(entry)).tobytes()
    assert big_len - len(entry) > 2**32 and last == entry
    assert gpu_ctx.d2h(reps, len(small), src_offset=big_len).tobytes() == small
