"""CPU: the N>1 path (one process per GPU, image i -> rank i mod N, one gather at the end) with two gloo ranks."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from upsnet_amd.upsnet_end2end_test import gather_results, init_distributed, shard_indices
    torch.cuda.is_available = lambda: False      # the host path (gloo, CPU tensors) also where GPUs are visible: this rank never opens one
    r, w, dev = init_distributed()
    assert (r, w) == (rank, world) and dist.get_backend() == 'gloo'
    ids = shard_indices(7, rank, world)           # uneven: rank 0 gets 4 images, rank 1 gets 3
    local = [(i, torch.full((6, 10), i, dtype=torch.uint8), 10 + i) for i in ids]
    out = gather_results(local, world, dev, 6, 10)
    if rank != 0:
        assert out is None                       # gather to rank 0 ONLY (reference: outputs are collected on the first device)
        out = {}
    empty = gather_results([] if rank == 1 else local[:1], world, dev, 6, 10)   # a rank without images must not break the collective
    assert rank != 0 or sorted(empty) == [0]
    # many records per rank, small chunks: several chunk collectives + a ragged last one, label maps of two sizes (void padded)
    many = [(i, torch.full((6, 10) if i % 3 else (4, 7), i, dtype=torch.uint8), i) for i in shard_indices(23, rank, world)]
    big = gather_results(many, world, dev, 6, 10, chunk=4)
    if rank == 0:
        assert sorted(big) == list(range(23))
        for i, (m, n) in big.items():
            h, w = (6, 10) if i % 3 else (4, 7)
            assert n == i and bool((m[:h, :w] == i).all()) and (h == 6 or (int(m[h:].min()) == 255 and int(m[:, w:].min()) == 255))
    # the streamed form of the timed loop: every rank adds `rows` records, full chunks leave asynchronously while the loop runs
    from upsnet_amd.upsnet_end2end_test import ResultGatherer
    g = ResultGatherer(world, dev, 6, 10, rows=11, chunk=4)
    for s in range(11):
        g.add(s * world + rank, torch.full((6, 10), (s * world + rank) % 251, dtype=torch.int64), s)   # int64 label map: converted in the copy
        assert g.sent == (s + 1) // 4 * 4          # chunk collectives are issued as soon as a chunk is full
    streamed = g.finish()
    assert g.collectives == 3 and g.bytes_sent == 3 * 4 * 60 and g.gather_s >= 0.0
    if rank == 0:
        assert sorted(streamed) == list(range(22))
        assert all(bool((m == i % 251).all()) and n == i // world for i, (m, n) in streamed.items())
        assert g.store.shape == (2, 12, 60)        # the result store; the collective in flight is world x chunk rows
    else:
        assert streamed is None and g.store is None
    bad = ResultGatherer(world, dev, 6, 10, rows=2, chunk=4)
    for s in range(2 if rank == 0 else 1):         # a rank that breaks the equal-count promise is reported, not silently truncated
        bad.add(s, torch.zeros((6, 10), dtype=torch.uint8), 0)
    try:
        bad.finish()
        raised = False
    except RuntimeError:
        raised = True
    assert raised
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)     # max-over-ranks timing reduction used by the bench
    q.put((rank, sorted(out.keys()), [int(out[i][0][0, 0]) for i in sorted(out)], [out[i][1] for i in sorted(out)], float(t)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_shard_and_gather():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29600 + os.getpid() % 300
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, keys, vals, ninst, tmax in res:
        if rank == 0:
            assert keys == list(range(7)) and vals == list(range(7)) and ninst == [10 + i for i in range(7)]
        else:
            assert keys == []
        assert tmax == 2.0


def test_shard_indices_cover_exactly_once():
    from upsnet_amd.upsnet_end2end_test import shard_indices
    for world in (1, 2, 4, 8):
        for n in (0, 1, 7, 64):
            got = sorted(sum([shard_indices(n, r, world) for r in range(world)], []))
            assert got == list(range(n))


def test_bench_refuses_to_misreport_gpu_count():
    """`bench.py --gpus N` must run N ranks or fail loudly (round-1 bug: the flag was parsed and ignored)."""
    import subprocess
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], env=env, capture_output=True, text=True, timeout=300)
    if torch.cuda.device_count() < 2:
        assert r.returncode != 0 and 'only' in r.stderr
    env['WORLD_SIZE'] = '4'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'WORLD_SIZE=4' in r.stderr


def test_rank_cpu_slices_partition_the_host():
    """8 ranks on a 256-thread host: disjoint contiguous slices of 32 CPUs, every CPU used once; fewer CPUs than ranks wrap around."""
    from upsnet_amd.upsnet_end2end_test import rank_cpu_slice
    cpus = list(range(256))
    slices = [rank_cpu_slice(r, 8, cpus) for r in range(8)]
    assert all(len(s) == 32 for s in slices) and sorted(sum(slices, [])) == cpus
    assert slices[3] == list(range(96, 128))
    assert rank_cpu_slice(5, 8, [0, 1, 2, 3]) in ([0], [1], [2], [3])
    assert rank_cpu_slice(0, 1, cpus) == cpus


def test_records_are_void_padded_and_single_rank_collective_flag():
    """the record outside a smaller label map is 255 (void), not class 0; gather_results(collective=False) is the
    local pack / unpack."""
    from upsnet_amd.upsnet_end2end_test import gather_results, pack_records, unpack_records
    lab = torch.full((4, 6), 3, dtype=torch.uint8)
    rec = pack_records([(7, lab, 2)], 5, 8, torch.device('cpu'))
    out = unpack_records(rec, 5, 8)
    m, n = out[7]
    assert n == 2 and torch.equal(m[:4, :6], lab) and int(m[4:].min()) == 255 and int(m[:, 6:].min()) == 255
    got = gather_results([(1, lab, 0)], 1, torch.device('cpu'), 4, 6)
    assert sorted(got) == [1] and torch.equal(got[1][0], lab)
