"""CPU, gloo, world_size 2 and 3: train_dist.GradExchange.reduce_ leaves ((g0 + g1) + g2) on every rank, bit for bit.  The
exchange under test is the product code (shard layout, batch_isend_irecv of the slices, all_gather of the summed shards); the
rank sum is the injected stand-in of sequential torch adds -- IEEE fp32 adds in slice order, what tm_op_rank_sum computes on the
GPU (tests/test_gpu_rank_sum.py holds the kernel to the same adds)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from teramind_amd.train_dist import GradExchange, shard_layout

N = 4100                      # not a multiple of 4 * world: the last shard is part gradient, part zero pad


def rank_grad(rank: int, n: int = N) -> torch.Tensor:
    """Standard normals times 2^k, k in [-8, 8] (sums that round, differently in different orders), and a few -0.0."""
    g = torch.Generator().manual_seed(1000 + rank)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-8, 9, (n,), generator=g).float())
    x[[0, 17, n - 1]] = -0.0
    return x


def sequential_sum(parts: torch.Tensor, out: torch.Tensor):
    """The stand-in for tm_op_rank_sum: out = ((parts[0] + parts[1]) + parts[2]) + ... starting from slice 0's value."""
    acc = parts[0].clone()
    for k in range(1, parts.shape[0]):
        acc = acc + parts[k]
    out.copy_(acc)


def ordered_sum(grads):
    acc = grads[0].clone()
    for g in grads[1:]:
        acc = acc + g
    return acc


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ex = GradExchange(N, rank, world, "cpu", rank_sum=sequential_sum)
        g = rank_grad(rank)
        first = ex.reduce_(g.clone()).clone()
        second = ex.reduce_(rank_grad(rank))                       # the buffers are reused: a second call gives the same bits
        losses = ex.all_gather_scalars(0.5 + rank)
        q.put((rank, first.view(torch.int32).numpy(), second.view(torch.int32).numpy(), losses, ex.bytes_sent, float(ex.send[N:].abs().sum())))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_is_the_rank_ordered_sum_on_every_rank(world):
    grads = [rank_grad(r) for r in range(world)]
    want = ordered_sum(grads).view(torch.int32)
    if world >= 3:                                                 # otherwise the test would prove nothing about order
        assert not torch.equal(ordered_sum(grads[::-1]).view(torch.int32), want), "the inputs do not tell the orders apart"
    assert (want[[0, 17, N - 1]] == torch.tensor(-0.0).view(torch.int32)).all()        # -0.0 + -0.0 = -0.0: slice 0 starts the sum, not zero
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shard, _ = shard_layout(N, world)
    assert sorted(g[0] for g in got) == list(range(world))
    for rank, first, second, losses, sent, pad in got:
        assert torch.equal(torch.from_numpy(first), want), f"rank {rank}: not the rank-ordered sum"
        assert torch.equal(torch.from_numpy(second), want), f"rank {rank}: second call differs"
        assert losses == [0.5 + r for r in range(world)]
        assert sent == 2 * 2 * (world - 1) * shard * 4 and pad == 0.0          # two calls; ring all-reduce traffic, not world * n


def test_exchange_needs_a_process_group():
    assert not dist.is_initialized()
    with pytest.raises(RuntimeError, match="launch.init_distributed"):
        GradExchange(N, 0, 2, "cpu", rank_sum=sequential_sum)
