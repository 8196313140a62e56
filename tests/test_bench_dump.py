"""CPU: bench.py --dump-outputs.  dump_sweep against the real presentation loop (sharding.run_sweep) with the ranks emulated in one process
(every rank makes the same gather calls; a gather copies the slots that travel into rank 0's receive buffers), for even and uneven deals and
several batch sizes: the files must hold exactly the frames of the sweep's last batch, as they arrived.  dump_single against a stand-in context:
the last frame's key / index pair, dtypes, the seeded sample and the 64 MB budget."""
import importlib
import os

import numpy as np
import pytest
import torch

import bench

sharding = importlib.import_module("4dgaussiansplatrendering_amd.sharding")


def _pixel(k, r, npx):
    """RGBA8 words of rank r's frame k: bytes (k & 255, k >> 8, r, pixel & 255)"""
    pix = np.arange(npx, dtype=np.int64)
    return torch.from_numpy(((k & 255) | ((k >> 8) << 8) | (r << 16) | ((pix & 255) << 24)).astype(np.uint32).view(np.int32))


def _emulate_sweeps(world, pct, G, npx, sweeps=2):
    mine = [sharding.frames_for_rank(bench.SWEEP_FRAMES, r, world, pct) for r in range(world)]
    most = sharding.most_frames(bench.SWEEP_FRAMES, world, pct)
    gathered = [[torch.full((G, npx), -1, dtype=torch.int32) for _ in range(world)] for _ in range(2)]
    calls = []
    for r in range(world):
        batch = [torch.full((G, npx), -1, dtype=torch.int32) for _ in range(2)]

        def pack(j, _frames_back, x, slot, r=r, batch=batch):
            batch[x][slot] = _pixel(mine[r][j], r, npx)

        def gather(x, lo, hi, _first, r=r, batch=batch):
            gathered[x][r][lo:hi] = batch[x][lo:hi]

        for _ in range(sweeps):
            calls.append(sharding.run_sweep(len(mine[r]), most, G, True, lambda j: None, pack, gather))
    assert all(c == calls[0] for c in calls)                    # every rank made the same collective calls
    return mine, most, gathered


@pytest.mark.parametrize("world,pct,G", [(1, 100, 8), (2, 100, 8), (3, 100, 3), (3, 70, 8), (8, 87, 8), (2, 98, 5)])
def test_dump_sweep_writes_the_last_batch_as_received(tmp_path, monkeypatch, world, pct, G):
    monkeypatch.setattr(bench, "H", 6)
    monkeypatch.setattr(bench, "W", 7)
    npx = bench.H * bench.W
    mine, most, gathered = _emulate_sweeps(world, pct, G, npx)
    bench.dump_sweep(str(tmp_path), gathered[((most - 1) // G) & 1], mine, most, G)
    assert sorted(os.listdir(tmp_path)) == ["frame_index.npy", "frames_rgba8.npy"]
    idx, fr = np.load(tmp_path / "frame_index.npy"), np.load(tmp_path / "frames_rgba8.npy")
    assert idx.dtype == np.float64 and fr.dtype == np.float32 and fr.shape == (idx.size, npx, 4)
    # the last batch of every rank: its presentations from the last batch boundary on, where it has a frame
    b = (most - 1) // G
    want = [(r, k) for r in range(world) for k in mine[r][b * G:most]]
    assert idx.astype(int).tolist() == [k for _, k in want]
    assert all(mine[r][-1] in idx for r in range(world) if len(mine[r]) > b * G)    # each rank's last frame is there
    for (r, k), f in zip(want, fr.astype(np.int64)):
        assert (f[:, 0] | (f[:, 1] << 8)).tolist() == [k] * npx and (f[:, 2] == r).all()
        assert (f[:, 3] == np.arange(npx) & 255).all()


def test_dump_sweep_samples_pixels_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "H", 16)
    monkeypatch.setattr(bench, "W", 16)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20000)
    npx, world, G = 256, 3, 8
    mine, most, gathered = _emulate_sweeps(world, 100, G, npx, sweeps=1)
    for d in ("a", "b"):
        bench.dump_sweep(str(tmp_path / d), gathered[((most - 1) // G) & 1], mine, most, G)
    pix = np.load(tmp_path / "a" / "pixel_positions.npy")
    fr = np.load(tmp_path / "a" / "frames_rgba8.npy")
    assert 0 < pix.size < npx and (np.diff(pix) > 0).all() and pix.max() < npx
    assert fr.nbytes + pix.nbytes + np.load(tmp_path / "a" / "frame_index.npy").nbytes <= 20000
    assert (fr[:, :, 3] == (pix.astype(np.int64) & 255)).all()                     # the sampled pixels, in order
    for f in ("pixel_positions.npy", "frames_rgba8.npy", "frame_index.npy"):       # the sample is fixed: the same in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


class _Ctx:
    def __init__(self):
        self.img = np.random.default_rng(1).random((bench.H, bench.W, 4), dtype=np.float32)

    def read_pixels(self):
        return self.img

    def read(self, buf, dtype, count):
        return (np.arange(count, dtype=np.uint64) * 2654435761 + buf * 977).astype(dtype)       # distinct words per buffer, the whole uint32 range


class _Scene:
    def __init__(self, n, frames):
        self.ctx, self.n, self.k = _Ctx(), n, frames
        self.keybufs = [(10 + 2 * i, 11 + 2 * i) for i in range(4)]


@pytest.mark.parametrize("n,sample", [(1000, 1 << 20), (1000, 100), (1_000_000, 1 << 20)])
def test_dump_single_writes_the_last_frames_buffers(tmp_path, monkeypatch, n, sample):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    sc = _Scene(n, frames=7)                                   # frame 7 used key / index pair 6 % 4
    keys, idx = sc.keybufs[2]
    for d in ("a", "b"):
        bench.dump_single(str(tmp_path / d), sc)
    out = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(out) == ({"image", "sorted_keys", "sort_permutation"} | ({"sample_positions"} if n > sample else set()))
    assert out["image"].dtype == np.float32 and np.array_equal(out["image"], sc.ctx.img)
    pos = out["sample_positions"].astype(np.int64) if n > sample else np.arange(n)
    assert pos.size == min(n, sample) and (np.diff(pos) > 0).all()
    for name, buf in (("sorted_keys", keys), ("sort_permutation", idx)):
        assert out[name].dtype == np.float64
        assert np.array_equal(out[name], sc.ctx.read(buf, np.uint32, n)[pos].astype(np.float64))
        assert np.array_equal(out[name], np.load(tmp_path / "b" / f"{name}.npy"))
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_BUDGET
