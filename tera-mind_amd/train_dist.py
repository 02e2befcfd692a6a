"""Data-parallel training: the gradient exchange that makes W rank processes one training run (the reference wraps its model
in DDP over a list of GPUs, experiment.py:449-490, and lets the collective library pick the order of the sums).

Here the order of every sum is stated and fixed: micro-batches in index order inside a rank (AdamTrainer.accumulate), then
ranks in index order (this file).  `GradExchange.reduce_` is a reduce-scatter + all-gather whose only arithmetic is
tm_op_rank_sum on the rank's own shard:

  1. the flat gradient [n] is padded with zeros to W shards of `shard` floats (shard_layout); rank r receives shard r of every
     rank's gradient into recv [W][shard], slot k from rank k, its own shard copied into slot r (batch_isend_irecv);
  2. tm_op_rank_sum: shard r of the sum = ((recv[0] + recv[1]) + recv[2]) + ...  -- plain fp32 adds in rank order;
  3. all_gather of the W summed shards, [:n] copied back.

Data movement changes no bit, so every rank ends with the same bits, the bits of an in-process `((g0 + g1) + g2) + ...`, whatever
the backend, the topology or the route (RCCL on the device; under gloo with device tensors staged through host memory, as
launch.broadcast_arena does).  Per rank 2 (W - 1) / W * n floats go out and come in: the traffic of a ring all-reduce.

Clip and Adam then run replicated on the full arena: bit-equal inputs give bit-equal parameters, nothing is broadcast after
step 0.  Not done: sharded optimizer state, overlap of the exchange with the backward."""
from typing import Callable, List, Optional, Tuple

import torch

from . import _lib


def shard_layout(n: int, world: int) -> Tuple[int, int]:
    """(shard, padded): shard = ceil(n / world) rounded up to a multiple of 4 floats (16-byte aligned slices for the kernel's
    vector accesses), padded = world * shard.  The pad floats are zeros and are never read back."""
    if n < 1 or world < 1:
        raise ValueError(f"shard_layout: n = {n}, world = {world}")
    shard = (-(-n // world) + 3) // 4 * 4
    return shard, world * shard


def require_group(world: int):
    """torch.distributed, after checking that a process group of `world` ranks is initialised."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() != world:
        have = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 0
        raise RuntimeError(f"data-parallel training with world = {world} needs an initialised process group of that size "
                           f"(found {have or 'none'}): call teramind_amd.launch.init_distributed in every rank process first")
    return dist


def hip_rank_sum(parts: torch.Tensor, out: torch.Tensor):
    """out [n] = the rank-ordered sum of parts [W][n] by tm_op_rank_sum, queued on the current stream."""
    if not (parts.is_cuda and out.is_cuda):
        raise RuntimeError("tm_op_rank_sum works on device tensors (teramind_amd has no CPU fallback)")
    W, n = parts.shape
    _lib.check(_lib.lib().tm_op_rank_sum(_lib.ptr(parts), _lib.ptr(out), W, n, _lib.current_stream_ptr()), "tm_op_rank_sum")


class GradExchange:
    """reduce_(g): g [n] fp32 on `device` <- sum over ranks of their g, added in rank order; the same bits on every rank.
    `rank_sum(parts [W][shard], out [shard])`: None = the HIP op; the CPU gloo test injects sequential torch adds (as
    launch.run_sweep takes its compute objects injected)."""

    def __init__(self, n: int, rank: int, world: int, device, rank_sum: Optional[Callable] = None):
        if world < 2 or not 0 <= rank < world:
            raise ValueError(f"GradExchange: rank {rank} of world {world}")
        dist = require_group(world)
        if dist.get_rank() != rank:
            raise RuntimeError(f"GradExchange: rank {rank}, but the process group says {dist.get_rank()}")
        self.n, self.rank, self.world, self.dev = int(n), int(rank), int(world), torch.device(device)
        self.shard, self.padded = shard_layout(self.n, self.world)
        self.rank_sum = rank_sum or hip_rank_sum
        # wire buffers live where the backend moves them: device memory under nccl, host memory under gloo
        self.via_host = self.dev.type == "cuda" and dist.get_backend() == "gloo"
        wire = torch.device("cpu") if self.via_host else self.dev
        self.send = torch.zeros(self.padded, dtype=torch.float32, device=wire)      # [n:] stays zero
        self.recv = torch.empty(self.world, self.shard, dtype=torch.float32, device=wire)
        self.full = torch.empty(self.padded, dtype=torch.float32, device=wire)
        self.parts = torch.empty_like(self.recv, device=self.dev) if self.via_host else self.recv
        self.sum = torch.empty(self.shard, dtype=torch.float32, device=self.dev)
        self.bytes_sent = 0

    def reduce_(self, g: torch.Tensor) -> torch.Tensor:
        import torch.distributed as dist
        if g.shape != (self.n,) or g.dtype != torch.float32 or g.device != self.dev or not g.is_contiguous():
            raise ValueError(f"reduce_: expected a contiguous fp32 [{self.n}] tensor on {self.dev}")
        W, r, sh = self.world, self.rank, self.shard
        self.send[:self.n].copy_(g)                                                  # device -> host under gloo
        ops = []
        for k in range(W):
            if k == r:
                self.recv[r].copy_(self.send[r * sh:(r + 1) * sh])
            else:
                ops += [dist.P2POp(dist.isend, self.send[k * sh:(k + 1) * sh], k), dist.P2POp(dist.irecv, self.recv[k], k)]
        for req in dist.batch_isend_irecv(ops):
            req.wait()
        if self.via_host:
            self.parts.copy_(self.recv)
        self.rank_sum(self.parts, self.sum)
        mine = self.sum.cpu() if self.via_host else self.sum
        dist.all_gather(list(self.full.view(W, sh).unbind(0)), mine)
        g.copy_(self.full[:self.n])
        self.bytes_sent += 4 * 2 * (W - 1) * sh
        return g

    def all_gather_scalars(self, x: float) -> List[float]:
        """One float64 per rank, in rank order (the logged loss: its mean over ranks is taken on the host, in rank order)."""
        import torch.distributed as dist
        wire = self.dev if dist.get_backend() == "nccl" else torch.device("cpu")
        out = torch.empty(self.world, 1, dtype=torch.float64, device=wire)
        dist.all_gather(list(out.unbind(0)), torch.tensor([float(x)], dtype=torch.float64, device=wire))
        return [float(v) for v in out.cpu().reshape(-1)]
