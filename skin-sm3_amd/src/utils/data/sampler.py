"""Batch index order of the tools on a real dataset, in plain torch (no DataLoader, no worker processes).

Training: per rank, the order of torch.utils.data.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=0,
drop_last=False) after set_epoch(epoch) -- a permutation drawn from a generator seeded with seed + epoch, padded by its own
head to a multiple of the world size, every world-th index from `rank` on -- cut into batches of the per-rank batch size,
the last, partial batch kept (the reference's loaders use drop_last=False, src/utils/misc.py:418-459).
Evaluation: 0 .. n-1 in order, no sampler, same batching.
"""
import math

import torch


def distributed_order(n, world, rank, epoch, seed=0):
    """int64 [ceil(n / world)]: the dataset indices rank `rank` visits in epoch `epoch`."""
    if n <= 0 or world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad sampler geometry: n={n} world={world} rank={rank}")
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    order = torch.randperm(n, generator=g)
    per_rank = math.ceil(n / world)
    total = per_rank * world
    if total > n:
        order = torch.cat([order] * math.ceil(total / n))[:total]
    return order[rank:total:world]


def batches(order, batch_size):
    """Consecutive slices of `order`, the last one possibly shorter."""
    if batch_size <= 0:
        raise ValueError("batch size must be positive")
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def train_batches(n, world, rank, epoch, batch_size, seed=0):
    return batches(distributed_order(n, world, rank, epoch, seed), batch_size)


def eval_batches(n, batch_size):
    return batches(torch.arange(n), batch_size)
