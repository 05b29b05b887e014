"""bench.py's own options: a plain run is the headline alone (the other legs
need --full), and --dump-outputs writes what the timed path computed."""
import json
import os

import numpy as np
import pytest

import bench
from oracle import oracle_c as oc


def test_bench_legs_beside_the_headline_need_full():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


class _FakeCtx:
    """d2h of host arrays standing in for device buffers."""

    def d2h(self, src, nbytes, dtype=np.uint8, src_offset=0):
        return src.view(np.uint8)[src_offset:src_offset + nbytes].view(dtype).copy()


class _World:
    def __init__(self, rank=0, world=1):
        self.rank, self.world = rank, world


def test_dump_outputs_writes_every_block(tmp_path):
    n = 1000
    masked = np.random.default_rng(3).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    masked[:2] = (0, 0xFFFFFFFF)
    ok = (np.arange(n) % 3 != 0).astype(np.uint8)
    bench.dump_outputs(_FakeCtx(), _World(), str(tmp_path / "out"), masked, ok, n)
    assert sorted(os.listdir(tmp_path / "out")) == ["masked_crc.npy", "verify_ok.npy"]
    m = np.load(tmp_path / "out" / "masked_crc.npy")
    k = np.load(tmp_path / "out" / "verify_ok.npy")
    assert m.dtype == np.float64 and np.array_equal(m.astype(np.uint32), masked)  # a u32 is exact in float64
    assert k.dtype == np.float32 and np.array_equal(k, ok)
    bench.dump_outputs(_FakeCtx(), _World(1, 2), str(tmp_path / "out2"), masked, ok, n)
    assert sorted(os.listdir(tmp_path / "out2")) == ["masked_crc_rank1.npy", "verify_ok_rank1.npy"]


def test_dump_outputs_samples_a_large_run(tmp_path, monkeypatch):
    """Past the cap the dump is a fixed sample: the ascending block indices
    that dump_sample names, the same on every run, and no file beside the
    values."""
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * bench.DUMP_BLOCK_BYTES)
    n = 1000
    masked = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761))
    ok = (np.arange(n) % 3 != 0).astype(np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(_FakeCtx(), _World(), str(tmp_path / d), masked, ok, n)
        assert sorted(os.listdir(tmp_path / d)) == ["masked_crc.npy", "verify_ok.npy"]
    idx = bench.dump_sample(n)
    assert len(idx) == 64 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < n
    assert bench.dump_sample(64) is None and len(bench.dump_sample(65)) == 64
    assert len(bench.dump_sample(n, world=4)) == 16  # the cap is shared by the ranks
    for d in ("a", "b"):
        assert np.array_equal(np.load(tmp_path / d / "masked_crc.npy").astype(np.uint32), masked[idx])
        assert np.array_equal(np.load(tmp_path / d / "verify_ok.npy"), ok[idx])
    assert 0 < ok[idx].sum() < 64  # the sample holds both flag values


def _dump_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


@pytest.mark.parametrize("world, n", [(1, 5_000_001), (8, 1 << 20)])
def test_dump_outputs_stays_within_64_mb(tmp_path, world, n):
    """The files of all ranks together, headers included, with the real cap:
    one rank of just more blocks than it admits, and the default 1 Mi blocks
    on each of 8 ranks (96 MiB unsampled)."""
    assert n * bench.DUMP_BLOCK_BYTES * world > bench.DUMP_MAX_BYTES
    masked = np.arange(n, dtype=np.uint32)
    ok = np.ones(n, np.uint8)
    for r in range(world):
        bench.dump_outputs(_FakeCtx(), _World(r, world), str(tmp_path), masked, ok, n)
    assert len(os.listdir(tmp_path)) == 2 * world
    assert bench.DUMP_MAX_BYTES - bench.DUMP_BLOCK_BYTES * world < _dump_bytes(tmp_path) <= 64_000_000
    last = "" if world == 1 else f"_rank{world - 1}"
    assert np.array_equal(np.load(tmp_path / f"masked_crc{last}.npy"), masked[bench.dump_sample(n, world)])


@pytest.mark.gpu
def test_bench_plain_run_and_dump_vs_oracle(tmp_path, capsys, monkeypatch):
    """A plain run over 193 blocks (not a multiple of a workgroup's 16): the
    line holds the headline with the steps asked for and none of the --full
    legs, and the dumped CRCs and flags are the oracle's for the same seed."""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    n = 193
    assert bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", str(n),
                       "--dump-outputs", str(tmp_path)]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "GiB/s" and d["higher_is_better"] and d["dtype"] == "u32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    # value is the bytes over ms_per_step: within 2 % (ms_per_step is printed to 1e-4 ms, 1 % of
    # the ~0.01 ms that the shortest step, one launch and its sync, takes) and value's own 0.1
    rate = n * 32768 / 2**30 / (d["ms_per_step"] / 1e3)
    assert abs(d["value"] - rate) <= 0.02 * rate + 0.05
    assert d["config"]["all_verify_flags_ok"]
    assert all(d[leg] is None for leg in ("cpu_baseline", "end_to_end", "c3", "c3_small"))
    want = oc.full_block_crcs(oc.synth_full_blocks(n, seed=bench.SEED))
    got = np.load(tmp_path / "masked_crc.npy")
    assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "verify_ok.npy"), np.ones(n, np.float32))
