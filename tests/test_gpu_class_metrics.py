"""csrc/class_metrics.hip (harness.classification_metrics_device) against the host form harness.classification_metrics at the
sizes where its loops change shape -- one wave, one tile, one more row, several workgroups, several tiles per workgroup --
and at the head's class counts: predictions, confusion matrix and counts bit for bit, the fp64 figures within 1e-15 (the
same IEEE operations), the mean loss within the worst-case bound of a recursive fp64 sum, the same bits on a second call,
and the call captured into a graph."""
import math
from fractions import Fraction

import pytest
import torch

from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness

pytestmark = pytest.mark.gpu

T = L.lib().mpo_class_metrics_tile()
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 100003]
CLASSES = [2, 3, 8]


def planted(n, c, seed):
    """Random softmax rows, labels and losses on the host, with the edge rows planted at either end (where n has room): two
    equal maxima, an all-equal row, a NaN at index 1 beside a larger value (at index 2; with two classes at index 0), a label
    of -1 and a label of C."""
    g = torch.Generator().manual_seed(seed)
    y = torch.softmax(2.0 * torch.randn(n, c, generator=g), dim=1)
    label = torch.randint(0, c, (n,), generator=g)
    loss = -torch.log(y[torch.arange(n), label])
    for first in (0, n - 5) if n >= 10 else (0,):
        at = [first + j for j in range(5) if first + j < n]
        if len(at) > 0:
            y[at[0]] = 0.1 / c
            y[at[0], c - 1] = y[at[0], c // 2 - 1 if c > 2 else 0] = 0.45           # two equal maxima: the first index wins
        if len(at) > 1:
            y[at[1]] = 1.0 / c
        if len(at) > 2:
            y[at[2], 1] = float("nan")
            y[at[2], 2 if c > 2 else 0] = 0.99
        if len(at) > 3:
            label[at[3]] = -1
        if len(at) > 4:
            label[at[4]] = c
    return y, label, loss


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def assert_matches_host(got, y, label, loss, tag):
    pred, confusion, counts, summary = (t.cpu() for t in got)
    h_pred, h_confusion, h_counts, h_summary = harness.classification_metrics(y, label, loss)
    assert pred.dtype == confusion.dtype == counts.dtype == torch.int64 and summary.dtype == torch.float64
    assert torch.equal(pred, h_pred), tag
    assert torch.equal(confusion, h_confusion), tag
    assert torch.equal(counts, h_counts), tag
    for k, name in ((0, "accuracy"), (1, "balanced accuracy")):
        a, b = summary[k].item(), h_summary[k].item()
        print(f"[class metrics {tag}] {name} {a!r} host {b!r}")
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-15, (tag, name, a, b)
    if loss is None:
        assert math.isnan(summary[2].item()), tag
        return
    n = int(y.shape[0])
    values = [float(v) for v in loss.double().tolist()]
    exact, magnitude = math.fsum(values), math.fsum(abs(v) for v in values)
    bound = n * 2.0 ** -53 * magnitude                  # the worst case of a recursive fp64 sum of n terms, from this data
    err = abs(float(Fraction(summary[2].item()) * n - Fraction(exact)))
    print(f"[class metrics {tag}] |n mean_loss - sum| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("c", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_host_form(dev, n, c):
    y, label, loss = planted(n, c, seed=1000 * c + n % 997)
    args = (y.to(dev), label.to(dev), loss.to(dev))
    got = harness.classification_metrics_device(*args)
    assert got[0].shape == (n,) and got[1].shape == (c, c) and got[2].shape == (4,) and got[3].shape == (3,)
    assert_matches_host(got, y, label, loss, f"n={n} C={c}")
    if n >= 10:
        assert int(got[2][2]) == 4 and int(got[2][3]) == 2          # the planted invalid labels and NaN rows were counted
    again = harness.classification_metrics_device(*args)
    for a, b in zip(got, again):
        assert torch.equal(bits(a), bits(b))                         # the same bits on a second call
    # without the predictions: the same figures
    no_pred = harness.classification_metrics_device(*args, want_pred=False)
    assert no_pred[0] is None and all(torch.equal(bits(a), bits(b)) for a, b in zip(got[1:], no_pred[1:]))


def test_no_loss_one_class_and_no_valid_label(dev):
    y, label, loss = planted(T + 7, 3, seed=5)
    got = harness.classification_metrics_device(y.to(dev), label.to(dev))
    assert_matches_host(got, y, label, None, "no loss")
    assert math.isnan(got[3][2].item())
    only = torch.full_like(label, 2)                                  # all labels of one class: one row of the matrix
    got = harness.classification_metrics_device(y.to(dev), only.to(dev), loss.to(dev))
    assert_matches_host(got, y, only, loss, "one class")
    assert int(got[1][:2].sum()) == 0 and int(got[1][2].sum()) == T + 7
    assert got[3][1].item() == got[3][0].item()                       # one class with support: its recall is the accuracy
    got = harness.classification_metrics_device(y[:1].to(dev), torch.tensor([3], device=dev), loss[:1].to(dev))
    assert_matches_host(got, y[:1], torch.tensor([3]), loss[:1], "n=1, invalid label")
    assert got[2].tolist() == [0, 0, 1, 0] and math.isnan(got[3][0].item()) and math.isnan(got[3][1].item())
    nan_loss = loss.clone()
    nan_loss[T] = float("nan")
    assert math.isnan(harness.classification_metrics_device(y.to(dev), label.to(dev), nan_loss.to(dev))[3][2].item())


def test_checked_front_refuses_what_the_host_knows(dev):
    y, label, loss = (t.to(dev) for t in planted(10, 3, seed=1))
    with pytest.raises(ValueError, match="y must be a tensor on the GPU"):
        harness.classification_metrics_device(y.cpu(), label, loss)
    with pytest.raises(ValueError, match="loss must be a tensor on the GPU"):
        harness.classification_metrics_device(y, label, loss.cpu())
    with pytest.raises(ValueError, match="equal and at least one"):
        harness.classification_metrics_device(y, label[:9], loss)
    with pytest.raises(ValueError, match="equal and at least one"):
        harness.classification_metrics_device(y, label, loss[:9])
    with pytest.raises(ValueError, match="equal and at least one"):
        harness.classification_metrics_device(y[:0], label[:0])
    for c in (1, 9):
        with pytest.raises(ValueError, match=f"{c} classes outside 2..8"):
            harness.classification_metrics_device(torch.zeros(10, c, device=dev), label)


def test_captured_call_follows_the_contents(dev):
    n, c = 3 * T + 5, 3
    y, label, loss = planted(n, c, seed=11)
    y_dev, label_dev, loss_dev = y.to(dev), label.to(dev), loss.to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        harness.classification_metrics_device(y_dev, label_dev, loss_dev)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        got = harness.classification_metrics_device(y_dev, label_dev, loss_dev)
    graph.replay()
    assert_matches_host(got, y, label, loss, "captured")
    y2, _, _ = planted(n, c, seed=12)
    y_dev.copy_(y2)
    graph.replay()
    assert_matches_host(got, y2, label, loss, "captured, y overwritten")
    assert not torch.equal(harness.classification_metrics(y, label)[0], harness.classification_metrics(y2, label)[0])
