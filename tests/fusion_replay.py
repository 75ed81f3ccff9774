"""Host restatement of the gated-concat and bilinear heads (include/mpo_fusion_next.h, csrc/fusion_next.hip + K6) in fp64
torch: the fusion layers (the bilinear one with explicit dropout masks), the classifier, the survival head and the per-slide
`ces` / `sct` losses, so a GPU run can be held to a reference that is itself pinned to the oracle and to the reference's golden
vectors (tests/test_fusion_next_cpu.py); and of where the bilinear head's five dropout sites draw their counters, on the
generator of tests/dropout_replay.py.  The gated-concat layer has no dropout site: its span is 0."""
from __future__ import annotations

import numpy as np
import torch

import dropout_replay as R

PARAM_NAMES = ("gates.0.0.weight", "gates.0.0.bias", "gates.1.0.weight", "gates.1.0.bias", "fusion_layer.0.weight",
               "fusion_layer.0.bias", "fusion_layer.2.weight", "fusion_layer.2.bias")
HEAD_NAMES = ("classifier.weight", "classifier.bias")
D_BUILT = (128, 256, 512)
MAX_CLASSES = 16            # kMaxC, csrc/tail.hip


def gated_concat_shapes(d: int, n_classes: int) -> dict:
    """The entry's ten parameters in its order (GatedConcatFusion(dims=[d, d], hidden_size=d, output_size=d) + classifier)."""
    return {"gates.0.0.weight": (1, d), "gates.0.0.bias": (1,), "gates.1.0.weight": (1, d), "gates.1.0.bias": (1,),
            "fusion_layer.0.weight": (d, 2 * d), "fusion_layer.0.bias": (d,), "fusion_layer.2.weight": (d, d),
            "fusion_layer.2.bias": (d,), "classifier.weight": (n_classes, d), "classifier.bias": (n_classes,)}


def gated_concat_span(n_slides: int, d: int) -> int:
    """Counters one call takes from the generator: the layer has no dropout site."""
    return 0


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def gated_concat_saved_floats(n_slides: int, d: int, n_classes: int, with_loss: bool) -> int:
    """hcat [B, 2d] | g [2B] | z1 [B, d] | z2 [B, d] | logits [B, C] (| d_logits [B, C]), every block padded to 64 floats."""
    b = n_slides
    blocks = [b * 2 * d, 2 * b, b * d, b * d, b * n_classes] + ([b * n_classes] if with_loss else [])
    return sum(_pad64(n) for n in blocks)


def gated_concat_workspace_bytes(n_slides: int, d: int, n_classes: int) -> int:
    """d_hcat [B, 2d] | t [2B] | d_logits [B, C] | d_z2 [B, d] | d_z1 [B, d]: blocks start at multiples of 256 bytes, + 256."""
    b, end = n_slides, 0
    for n in (b * 2 * d, 2 * b, b * n_classes, b * d, b * d):
        end = (end + 255) // 256 * 256 + 4 * n
    return end + 256


def gated_concat_fusion(h_path, h_omic, p):
    """(B, d), (B, d) fp64 -> fused (B, d): models/fusion.py:22-41 with the gates as parameters.  p: PARAM_NAMES -> fp64."""
    items = []
    for i, x in enumerate((h_path, h_omic)):
        g = torch.sigmoid(x @ p[f"gates.{i}.0.weight"].t() + p[f"gates.{i}.0.bias"])          # (B, 1)
        items.append(x * g)
    h = torch.cat(items, dim=1)
    h = torch.relu(h @ p["fusion_layer.0.weight"].t() + p["fusion_layer.0.bias"])
    return torch.relu(h @ p["fusion_layer.2.weight"].t() + p["fusion_layer.2.bias"])


def survival_head(fused, p):
    """models/mcat/mcat.py:126-138 per slide: -> hazards, survs, Y (B, C)."""
    logits = fused @ p["classifier.weight"].t() + p["classifier.bias"]
    hazards = torch.sigmoid(logits)
    return hazards, torch.cumprod(1 - hazards, dim=1), torch.softmax(logits, dim=1)


def ces_per_slide(hazards, survs, label, cens, alpha=0.75, eps=1e-7):
    """CrossEntropySurvivalLoss (models/loss.py:5-28) of every slide on its own (the reference's batch is one slide)."""
    y, c = label.view(-1, 1), cens.view(-1, 1).to(hazards.dtype)
    s_pad = torch.cat([torch.ones_like(c), survs], 1)
    reg = -(1 - c) * (torch.log(torch.gather(s_pad, 1, y).clamp(min=eps)) + torch.log(torch.gather(hazards, 1, y).clamp(min=eps)))
    s_y = torch.gather(survs, 1, y).clamp(min=eps)
    ce = -(c * torch.log(s_y) + (1 - c) * torch.log(1 - s_y))
    return ((1 - alpha) * ce + alpha * reg).view(-1)


def sct_per_slide(y, label, cens, eps=1e-7):
    """SurvivalClassificationTobitLoss (models/loss.py:62-85) on Y, per slide."""
    idx = torch.arange(y.shape[1])[None, :]
    lab = label.view(-1, 1)
    keep = torch.where(cens.view(-1, 1) != 0, idx >= lab, idx == lab)
    return -torch.log((y * keep).sum(1) + eps)


def gated_concat_head(h_path, h_omic, p):
    """-> fused, hazards, survs, Y."""
    fused = gated_concat_fusion(h_path, h_omic, p)
    return (fused, *survival_head(fused, p))


def gated_concat_head_loss(h_path, h_omic, p, label, cens, kind, alpha=0.75, eps=1e-7):
    """-> per-slide loss, risk, hazards, survs, Y   (kind: 'ces' | 'sct'; risk = -sum_j survs_j, models/mcat/main.py:56)."""
    _, hz, sv, y = gated_concat_head(h_path, h_omic, p)
    loss = ces_per_slide(hz, sv, label, cens, alpha, eps) if kind == "ces" else sct_per_slide(y, label, cens, eps)
    return loss, -sv.sum(1), hz, sv, y


# ------------------------------------------------------------------------------------------- bilinear fusion
BIL_H, BIL_M, BIL_KRON, BIL_CAT = 32, 64, 33 * 33, 64 + 2 * 33
BILINEAR_SITES = ("linear_o1", "linear_o2", "post_fusion", "fc1", "fc2")


def bilinear_shapes(d: int, n_classes: int) -> dict:
    """The entry's eighteen parameters in its order (BilinearFusion(dim1=d, dim2=d, output_size=d) + classifier)."""
    s = {}
    for i in (1, 2):
        s.update({f"linear_h{i}.0.weight": (BIL_H, d), f"linear_h{i}.0.bias": (BIL_H,), f"linear_z{i}.weight": (BIL_H, d, d),
                  f"linear_z{i}.bias": (BIL_H,), f"linear_o{i}.0.weight": (BIL_H, BIL_H), f"linear_o{i}.0.bias": (BIL_H,)})
    s.update({"fc1.0.weight": (BIL_M, BIL_KRON), "fc1.0.bias": (BIL_M,), "fc2.0.weight": (d, BIL_CAT), "fc2.0.bias": (d,),
              "classifier.weight": (n_classes, d), "classifier.bias": (n_classes,)})
    return s


def bilinear_stride(n_slides: int) -> int:
    return (n_slides * BIL_KRON + 3) // 4 + 2


def bilinear_span(n_slides: int, d: int) -> int:
    """mpo_bilinear_head_rng_span restated."""
    return 5 * bilinear_stride(n_slides)


def bilinear_site_elements(n_slides: int, d: int):
    return (n_slides * BIL_H, n_slides * BIL_H, n_slides * BIL_KRON, n_slides * BIL_M, n_slides * d)


def bilinear_sites(n_slides: int, d: int, off: int = 0):
    """[(site name, lo, hi)]: the counters [lo, hi) each site touches (one counter per four elements)."""
    stride = bilinear_stride(n_slides)
    return [(name, off + s * stride, off + s * stride + (n + 3) // 4)
            for s, (name, n) in enumerate(zip(BILINEAR_SITES, bilinear_site_elements(n_slides, d)))]


def bilinear_keeps(seed: int, off: int, n_slides: int, d: int, p: float, epoch: int = 0) -> dict:
    """The five keep-scale masks (0 or 1 / (1 - p), float64 torch) of a call that reserved `off`, at device epoch `epoch`."""
    base, stride, b = R.epoch_off(off, epoch), bilinear_stride(n_slides), n_slides
    shapes = ((b, BIL_H), (b, BIL_H), (b, BIL_KRON), (b, BIL_M), (b, d))
    return {name: torch.from_numpy(R.keep_scale(seed, base + s * stride, int(np.prod(shape)), p).reshape(shape))
            for s, (name, shape) in enumerate(zip(BILINEAR_SITES, shapes))}


def bilinear_ones(n_slides: int, d: int) -> dict:
    b = n_slides
    shapes = ((b, BIL_H), (b, BIL_H), (b, BIL_KRON), (b, BIL_M), (b, d))
    return {name: torch.ones(shape, dtype=torch.float64) for name, shape in zip(BILINEAR_SITES, shapes)}


def bilinear_fusion(x1, x2, p, keeps=None):
    """(B, d), (B, d) fp64 -> fused (B, d): models/fusion.py:44-113 with its defaults, every dropout as a product with the
    given keep-scale mask (None: eval mode)."""
    k = keeps if keeps is not None else bilinear_ones(x1.shape[0], x1.shape[1])

    def branch(i, a, b):
        z = torch.einsum("bi,kij,bj->bk", a, p[f"linear_z{i}.weight"], b) + p[f"linear_z{i}.bias"]
        h = torch.relu(a @ p[f"linear_h{i}.0.weight"].t() + p[f"linear_h{i}.0.bias"])
        o = torch.relu((torch.sigmoid(z) * h) @ p[f"linear_o{i}.0.weight"].t() + p[f"linear_o{i}.0.bias"])
        return o * k[f"linear_o{i}"]

    ones = torch.ones(x1.shape[0], 1, dtype=x1.dtype)
    o1, o2 = torch.cat([branch(1, x1, x2), ones], 1), torch.cat([branch(2, x2, x1), ones], 1)
    kron = (o1.unsqueeze(2) * o2.unsqueeze(1)).flatten(1) * k["post_fusion"]
    u = torch.relu(kron @ p["fc1.0.weight"].t() + p["fc1.0.bias"]) * k["fc1"]
    cat = torch.cat([u, o1, o2], 1)
    return torch.relu(cat @ p["fc2.0.weight"].t() + p["fc2.0.bias"]) * k["fc2"]


def bilinear_head(x1, x2, p, keeps=None):
    """-> fused, hazards, survs, Y."""
    fused = bilinear_fusion(x1, x2, p, keeps)
    return (fused, *survival_head(fused, p))


def bilinear_head_loss(x1, x2, p, label, cens, kind, keeps=None, alpha=0.75, eps=1e-7):
    """-> per-slide loss, risk, hazards, survs, Y."""
    _, hz, sv, y = bilinear_head(x1, x2, p, keeps)
    loss = ces_per_slide(hz, sv, label, cens, alpha, eps) if kind == "ces" else sct_per_slide(y, label, cens, eps)
    return loss, -sv.sum(1), hz, sv, y
