"""The host side of data-parallel epochs over a sharded cohort (dp.shard_slides, epoch_orders, global_order,
gather_ragged): pure functions of host lists, and the one ragged all-gather under gloo on the CPU at world 2 and 3.
Nothing here launches a kernel."""
import random

import numpy as np
import pytest
import torch

from dp_spawn import run_world
from multimodal_path_omic_amd import dp, harness


# ------------------------------------------------------------------------------------------------ shard_slides
def check_shards(lengths, world):
    shards = dp.shard_slides(lengths, world)
    assert len(shards) == world and all(s == sorted(s) for s in shards)
    assert sorted(i for s in shards for i in s) == list(range(len(lengths)))          # disjoint, and every slide
    sizes = [len(s) for s in shards]
    assert max(sizes) - min(sizes) <= 1, (lengths, world, sizes)
    loads = [sum(lengths[i] for i in s) for s in shards]
    assert max(loads) - min(loads) <= max(lengths, default=0), (lengths, world, loads)
    assert dp.shard_slides(list(lengths), world) == shards                            # deterministic
    return shards


def test_shard_slides_properties_over_seeded_cases():
    gen = random.Random(20261020)
    for case in range(600):
        world = gen.choice([1, 2, 3, 4, 8])
        n = gen.randint(0, 40)
        kind = case % 4
        if kind == 0:
            lengths = [gen.randint(1, 30000) for _ in range(n)]
        elif kind == 1:
            lengths = [gen.randint(1, 5) for _ in range(n)]                           # many ties
        elif kind == 2:
            lengths = [4096] * n                                                      # all equal
        else:
            lengths = [gen.randint(1, 300) for _ in range(n)]
            if n:
                lengths[gen.randrange(n)] = 1_000_000                                 # one giant slide
        check_shards(lengths, world)
    for n in (1, 2, 3, 5, 8, 13):
        check_shards(list(range(100, 100 + n)), n)                                    # world equal to the number of slides
        assert dp.shard_slides([7] * n, 1) == [list(range(n))]                        # world 1: everything, in id order
    with pytest.raises(ValueError, match="world_size 0"):
        dp.shard_slides([1, 2], 0)


def test_shard_slides_literal():
    # sorted by (-length, id): 1 (40), 4 (29), 7 (23), 2 (17), 5 (11), 6 (8), 0 (5), 3 (3)
    lengths = [5, 40, 17, 3, 29, 11, 8, 23]
    assert dp.shard_slides(lengths, 3) == [[0, 1, 6], [3, 4, 5], [2, 7]]              # dealt 0 1 2 | 2 1 0 | 0 1
    assert dp.shard_slides(lengths, 2) == [[1, 2, 3, 5], [0, 4, 6, 7]]                # dealt 0 1 | 1 0 | 0 1 | 1 0
    assert dp.shard_slides([9, 9, 9], 2) == [[0], [1, 2]]                             # ties go by id; the turn gives rank 1 two


# ------------------------------------------------------------------------------------------------ epoch_orders, global_order
def test_epoch_orders():
    sizes = [7, 6, 7]
    orders, n_windows = dp.epoch_orders(sizes, 2, seed=11, epoch=0)
    assert n_windows == 3 and [sorted(o) for o in orders] == [list(range(s)) for s in sizes]
    assert dp.epoch_orders(sizes, 2, seed=11, epoch=0) == (orders, n_windows)         # equal on recomputation
    assert dp.epoch_orders(sizes, 3, seed=11, epoch=0) == (orders, 2)                 # the window size moves the count alone
    assert dp.epoch_orders([7, 40, 7], 2, seed=11, epoch=0)[0][0] == orders[0]        # a pure function of (seed, epoch, r, size)
    assert dp.epoch_orders([7, 40, 7], 2, seed=11, epoch=0)[0][2] == orders[2]
    later, _ = dp.epoch_orders(sizes, 2, seed=11, epoch=1)
    other, _ = dp.epoch_orders(sizes, 2, seed=12, epoch=0)
    for r in range(3):
        assert later[r] != orders[r] and other[r] != orders[r]                        # the epoch and the seed move every order
    assert orders[0] != orders[2]                                                     # equal sizes, different ranks
    for n, want in ((1, 6), (2, 3), (4, 1), (6, 1)):
        assert dp.epoch_orders(sizes, n, 0, 0)[1] == want == min(s // n for s in sizes)
    with pytest.raises(ValueError, match="rank 1's shard holds 6 slides, fewer than one window of 7"):
        dp.epoch_orders(sizes, 7, 0, 0)
    with pytest.raises(ValueError):
        dp.epoch_orders([], 2, 0, 0)
    seen = {tuple(dp.epoch_orders([5], 1, 3, e)[0][0]) for e in range(200)}
    assert len(seen) > 60                                                             # (120 permutations of 5: a real shuffle)


def test_global_order_is_the_ranks_windows_side_by_side():
    lengths = [300, 20, 4000, 77, 1500, 640, 9, 2500, 31, 800, 450]
    for world, n in ((2, 2), (3, 1), (3, 2), (1, 4)):
        shards = dp.shard_slides(lengths, world)
        orders, n_windows = dp.epoch_orders([len(s) for s in shards], n, seed=5, epoch=2)
        flat = dp.global_order(orders, shards, n, n_windows)
        assert len(flat) == n_windows * n * world and len(set(flat)) == len(flat)
        for w in range(n_windows):
            want = [shards[r][i] for r in range(world) for i in orders[r][w * n:(w + 1) * n]]
            assert flat[w * n * world:(w + 1) * n * world] == want
    with pytest.raises(ValueError, match="no window 1"):
        dp.global_order([[0, 1], [0]], [[0, 2], [1]], 1, 2)


# ------------------------------------------------------------------------------------------------ gather_ragged
def _rows(rank, size, two_d):
    """Rank `rank`'s tensor: values that name their rank and row, with a NaN and a negative zero among them."""
    g = torch.Generator().manual_seed(1000 + rank)
    t = torch.randn((size, 3) if two_d else (size,), generator=g, dtype=torch.float64 if two_d else torch.float32)
    flat = t.view(-1)
    if rank == 1 and flat.numel():
        flat[0] = float("nan")
    if rank == 0 and flat.numel() > 1:
        flat[1] = -0.0
    return t


def _survival(rank, size):
    g = torch.Generator().manual_seed(2000 + rank)
    cens = (torch.rand(size, generator=g) < 0.4).float()
    months = torch.randint(1, 9, (size,), generator=g).double()                      # ties in time
    risk = torch.randint(0, 5, (size,), generator=g).float() / 4                     # ties in risk
    return cens, months, risk


def _gather_worker(rank, world, sizes, out):
    got = {}
    for two_d in (False, True):
        mine = _rows(rank, sizes[rank], two_d)
        keep = mine.clone()
        got[two_d] = dp.gather_ragged(mine, sizes)
        assert torch.equal(mine.view(torch.int64 if two_d else torch.int32), keep.view(torch.int64 if two_d else torch.int32))
    ints = dp.gather_ragged(torch.arange(sizes[rank], dtype=torch.int64) + 100 * rank, sizes)
    cens, months, risk = (dp.gather_ragged(t, sizes) for t in _survival(rank, sizes[rank]))
    c = harness.concordance_index_censored(1 - cens.numpy(), months.numpy(), risk.numpy())
    with pytest.raises(ValueError, match="gather_ragged: sizes"):                     # refused before any collective: on every rank
        dp.gather_ragged(torch.zeros(sizes[rank] + 1), sizes)
    with pytest.raises(ValueError, match="gather_ragged: sizes"):
        dp.gather_ragged(torch.zeros(sizes[rank]), sizes + [1])
    torch.save({"1d": got[False], "2d": got[True], "ints": ints, "c": c}, f"{out}.{rank}")


@pytest.mark.timeout(180)
@pytest.mark.parametrize("sizes", [[3, 2], [1, 4, 2], [2, 2, 2]], ids=["3_2", "1_4_2", "2_2_2"])
def test_gather_ragged_under_gloo(tmp_path, sizes):
    world, out = len(sizes), str(tmp_path / "gathered.pt")
    run_world(_gather_worker, world, sizes, out, limit=150.0)
    got = [torch.load(f"{out}.{r}", weights_only=True) for r in range(world)]
    want_1d = torch.cat([_rows(r, s, False) for r, s in enumerate(sizes)])
    want_2d = torch.cat([_rows(r, s, True) for r, s in enumerate(sizes)])
    want_ints = torch.cat([torch.arange(s, dtype=torch.int64) + 100 * r for r, s in enumerate(sizes)])
    cens, months, risk = (torch.cat(parts) for parts in zip(*[_survival(r, s) for r, s in enumerate(sizes)]))
    want_c = harness.concordance_index_censored(1 - cens.numpy(), months.numpy(), risk.numpy())
    assert bool(torch.isnan(want_1d).any()) and bool(torch.isnan(want_2d).any())
    for r in range(world):
        assert got[r]["1d"].dtype == torch.float32 and got[r]["1d"].shape == (sum(sizes),)
        assert torch.equal(got[r]["1d"].view(torch.int32), want_1d.view(torch.int32))          # bit for bit: NaN and -0.0 too
        assert got[r]["2d"].shape == (sum(sizes), 3)
        assert torch.equal(got[r]["2d"].view(torch.int64), want_2d.view(torch.int64))
        assert torch.equal(got[r]["ints"], want_ints)
        assert got[r]["c"] == want_c                                                          # the union's C-index, on every rank


def test_gather_ragged_without_a_group_returns_its_argument():
    t = torch.arange(6.0).view(3, 2)
    assert dp.gather_ragged(t, [3]) is t
    assert dp.gather_ragged(t, [99, 1]) is t                      # (no group: nothing to check `sizes` against)
    assert np.array_equal(t.numpy(), np.arange(6.0).reshape(3, 2))
