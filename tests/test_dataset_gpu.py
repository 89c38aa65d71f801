"""-m gpu: the device-resident packed dataset.  The collate kernel's batch equals the host batch bit for bit (every id list
of the CPU test, B = 1 / 70 / 130 with repetition, a side stream, device ids), writes exactly its outputs, flags a device
id out of range without leaving the store, and train.py trains on a pack as it does on the generator's graphs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from singa_amd import dataset as D
from singa_amd import graph as G
from tests.test_dataset_cpu import ID_LISTS, assert_same_graph, small_graphs, without_rot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def drawn(B):
    return np.random.RandomState(B).randint(0, 12, B).tolist()


CASES = [list(i) for i in ID_LISTS] + [[7], drawn(70), drawn(130), [4], [4, 4, 4]]       # graph 4 has no lp / pl edges


@pytest.fixture(scope="module")
def stores():
    import __graft_entry__
    __graft_entry__.build()
    host = D.PackedDataset.from_graphs(small_graphs())
    return host, D.PackedDataset.from_graphs(small_graphs()).to(DEV)


@pytest.fixture(scope="module")
def host_batches(stores):
    """The reference of every case, computed once on the host and left unchanged."""
    return {tuple(ids): stores[0].host_batch(ids) for ids in CASES}


@pytest.mark.parametrize("case", range(len(CASES)))
def test_device_batch_equals_host_batch(stores, host_batches, case):
    ids = CASES[case]
    _, dev = stores
    want = host_batches[tuple(ids)]
    got = dev.batch(ids)
    assert got[G.PA]["x"].is_cuda and got.num_graphs == len(ids)
    assert_same_graph(got, want)
    assert int(dev.last_status.item()) == 0
    if ids == [4]:
        assert tuple(got[G.E_LP]["edge_index"].shape) == (2, 0) and tuple(got[G.E_PL]["edge_index"].shape) == (2, 0)
    # a side stream, and the ids as a device tensor (a slice of a longer one: 4-byte aligned only)
    s = torch.cuda.Stream()
    longer = torch.tensor([0] + ids + [0], dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        again = dev.batch(longer[1:1 + len(ids)], host_ids=ids)
    s.synchronize()
    assert_same_graph(again, want)
    assert int(dev.last_status.item()) == 0


def test_store_without_rot_rand(stores):
    gs = without_rot(small_graphs())
    dev = D.PackedDataset.from_graphs(gs).to(DEV)
    got = dev.batch([11, 0, 5, 5, 3])
    assert "rot_rand" not in got.extras
    assert_same_graph(got, G.collate([gs[i] for i in [11, 0, 5, 5, 3]]))


def test_host_fallback_and_memory_refusal(stores, host_batches):
    ids = CASES[1]
    off = D.PackedDataset.from_graphs(small_graphs()).to(DEV, device_resident=False)
    got = off.batch(ids)
    assert got[G.PA]["x"].is_cuda
    assert_same_graph(got, host_batches[tuple(ids)])
    with pytest.raises(RuntimeError, match="device_resident=False") as e:
        D.PackedDataset.from_graphs(small_graphs()).to(DEV, reserve_bytes=1 << 50)
    assert str(1 << 50) in str(e.value) and str(off.nbytes + off.offsets.nbytes) in str(e.value)
    with pytest.raises(IndexError):
        stores[1].batch([0, 12])                               # host ids out of range are refused on the host


@pytest.mark.parametrize("ids", [[11, 0, 5, 5, 3], [4, 4], drawn(130)])
def test_write_footprint(stores, ids):
    """Every output carved out of one arena between sentinel guard bands: the guards are intact and every output element is
    written (the outputs equal the host batch under two different sentinels, so no element kept the arena's fill)."""
    _, dev = stores
    want = stores[0].host_batch(ids)
    for fill in (0xA5, 0x3C):
        arena = torch.full((16 << 20,), fill, dtype=torch.uint8, device=DEV)
        spans, at = [], [256]

        def alloc(shape, dt):
            n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            lo = at[0]
            at[0] = -(-(lo + n + 200) // 8) * 8 + 8            # guard of at least 200 bytes; outputs 8-byte aligned only
            spans.append((lo, lo + n))
            return arena[lo:lo + n].view(dt).view(*shape)

        got = dev.batch(ids, alloc=alloc)
        torch.cuda.synchronize()
        assert at[0] < arena.numel()
        assert_same_graph(got, want)
        guard = torch.ones_like(arena, dtype=torch.bool)
        for lo, hi in spans:
            guard[lo:hi] = False
        assert bool((arena[guard] == fill).all()), "a guard band was written"
    if ids == [4, 4]:
        assert tuple(got[G.E_LP]["edge_index"].shape) == (2, 0)


def test_device_id_out_of_range_is_clamped_and_flagged(stores):
    """Device ids the host copy does not match (the caller's mistake): the status word counts them, every read stays inside
    the store (the id is clamped) and every write inside the outputs the host sized."""
    _, dev = stores
    host_ids = [3, 0, 11, 2]                                    # what the outputs are sized for
    bad = torch.tensor([3, -1, 99, 2], dtype=torch.int32, device=DEV)      # clamps to 3, 0, 11, 2
    got = dev.batch(bad, host_ids=host_ids)
    assert int(dev.last_status.item()) == 2
    assert_same_graph(got, stores[0].host_batch(host_ids))


def _train(args, logdir):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--lmax", "2", "--batch-size", "3", "--no-dropout", "--logdir", logdir] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    return [float(l.split("Loss ")[1].split(" ")[0]) for l in out.splitlines() if "[Train]" in l]


def test_train_on_a_pack_equals_train_on_the_generator(tmp_path):
    """train.py --data packed on a pack of synthetic_graph(3..11) (they carry their edge-frame draws) against --data
    synthetic, whose iterations 1 to 3 use exactly these graphs: the logged losses agree to 1e-4 relative (the project's bound
    for the same inputs through two paths, tests/test_train_entry_gpu.py), eager and replayed, and the loss falls."""
    pack = D.PackedDataset.from_graphs([G.synthetic_graph(i, with_lap=False) for i in range(3, 12)],
                                       names=[f"synthetic_{i}" for i in range(3, 12)],
                                       splits={"train": range(9), "val": range(3), "test": []})
    pack.save(str(tmp_path / "pack"))
    ref = _train(["--data", "synthetic", "--max-iters", "3"], str(tmp_path / "s"))
    packed = _train(["--data", "packed", "--dataset", str(tmp_path / "pack"), "--no-shuffle", "--max-iters", "3"], str(tmp_path / "p"))
    print("synthetic", ref, "packed", packed)
    assert len(ref) == 3 and len(packed) == 3 and packed[-1] < packed[0]
    assert all(abs(p - r) < 1e-4 * r for p, r in zip(packed, ref)), (packed, ref)
    graph = _train(["--data", "packed", "--dataset", str(tmp_path / "pack"), "--no-shuffle", "--max-iters", "2", "--graph"],
                   str(tmp_path / "g"))
    print("packed --graph", graph)
    assert len(graph) == 2 and all(abs(g - r) < 1e-4 * r for g, r in zip(graph, ref)), (graph, ref)
