"""ops.map_block_stats (csrc/map_stats.hip): [min, max, mean] of every slide's block of a ragged attention map, built here
directly (no model).  min and max equal torch's exactly; the mean lies within 1e-6 relative of the fp64 mean.  Slide
lengths 1, 63, 64, 65, 255, 256, 257 and 20 000 in one window (blocks shorter than a wave, than a workgroup's trip, than a
chunk of 4096 values, and of many chunks: 20 000 x 16 = 79 chunks) plus a one-slide window, for 1, 6 and 16 queries;
softmax-like values (positive, every row sums to 1) and signed random ones."""
import pytest
import torch

from multimodal_path_omic_amd import ops
from multimodal_path_omic_amd.ops import BagBatch

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 20000]


def ragged_maps(dev, lengths, n_q, kind, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    blocks = []
    for m in lengths:
        x = torch.randn(n_q, m, generator=g)
        blocks.append(torch.softmax(3.0 * x, dim=1) if kind == "softmax" else x)
    flat = torch.cat([b.reshape(-1) for b in blocks]).to(dev)
    bags = BagBatch.from_lengths(torch.empty(sum(lengths), 8, device=dev), lengths)
    return bags.split_map(flat, n_q)


def check(maps):
    stats = ops.map_block_stats(maps)
    assert stats.shape == (len(maps), 3) and stats.dtype == torch.float32
    again = ops.map_block_stats(maps)
    assert torch.equal(stats, again)                                     # a fixed order of additions: the same bits
    for b, block in enumerate(maps):
        lo, hi, mean = (float(v) for v in stats[b])
        ref = float(block.double().mean())
        print(f"[map stats] slide {b} ({block.shape[0]} x {block.shape[1]}): mean {mean!r} fp64 {ref!r} "
              f"rel {abs(mean - ref) / abs(ref):.2e}")
        assert lo == float(block.min()) and hi == float(block.max())
        assert abs(mean - ref) <= 1e-6 * abs(ref), (b, mean, ref)


@pytest.mark.parametrize("kind", ["softmax", "signed"])
@pytest.mark.parametrize("n_q", [1, 6, 16])
def test_window_of_every_edge_length(dev, n_q, kind):
    check(ragged_maps(dev, LENGTHS, n_q, kind, seed=10 * n_q + (kind == "signed")))


@pytest.mark.parametrize("n_q", [1, 6, 16])
@pytest.mark.parametrize("m", [1, 257, 20000])
def test_one_slide_window(dev, n_q, m):
    check(ragged_maps(dev, [m], n_q, "softmax", seed=m + n_q))


def test_the_longest_slide_first_and_a_nan(dev):
    """The grid is sized by the longest slide wherever it stands; min and max carry a NaN as torch's do."""
    maps = ragged_maps(dev, [20000, 1, 300], 6, "softmax", seed=3)
    check(maps)
    maps.flat[6 * 20000 + 6 + 17] = float("nan")                         # in the third slide
    stats = ops.map_block_stats(maps)
    assert bool(torch.isnan(stats[2]).all()) and not bool(torch.isnan(stats[:2]).any())
    assert float(stats[1, 0]) == float(maps[1].min())


def test_no_host_sync_and_refusals(dev):
    maps = ragged_maps(dev, [65, 4097], 6, "softmax", seed=4)
    ops.map_block_stats(maps)
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            int(probe)
        stats = ops.map_block_stats(maps)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert float(stats[1, 1]) == float(maps[1].max())
    short = ops.RaggedMaps(maps)
    short.flat, short.batch, short.n_q = maps.flat[:-1], maps.batch, 6
    with pytest.raises(ValueError, match="map values"):
        ops.map_block_stats(short)
    maps.flat = maps.flat.double()
    with pytest.raises(ValueError, match="fp32"):
        ops.map_block_stats(maps)
