"""Names the dropout streams of one whole window step of a fusion model (MCAT / NaCAGaT forward_window), so a test can replay
every mask of a GPU step in the fp64 oracle.  Plain module (not a conftest); host only apart from the two read-backs below.

`recording()` wraps ops._reserve -- the one place the generator's counter space is carved -- and lists (span, offset) of every
reservation made inside the block.  `match_sites()` tells the records apart by their span, restated by tests/dropout_replay.py
for the geometry forward_window runs the tail with: the SNN over (B, N, d); the two branches' encoders stacked into ONE
entry call over 2 B sequences of N tokens; the two pooling heads stacked likewise, rho's rows interleaved [slide][branch][d].
The patch layer reserves rows * E // 16 + 2 counters, NaCAGaT's map (N * rows + 3) // 4; anything else a caller expects (the row
sampler's single counter, a fusion head's sites) is named through `extra`.  Every expected site must appear exactly once and
no record may be left over.  `host_keeps()` then rebuilds the SNN's, the encoders' and the pooling heads' masks for a
(seed, epoch) through dropout_replay's *_keeps functions and `slide_keeps()` cuts them into the per-slide arguments of
oracle.mpo_oracle.mcat_forward / nacagat_forward.

The patch layer's mask has no host restatement and is read back from the device, as the per-stage tests do: from the
training-mode H_bag (zeros are ReLU zeros or dropped elements; both carry neither value nor gradient).  The K2 map's can be
read back the same way from the returned post-dropout map (the softmax is positive everywhere before dropout) or rebuilt on
the host (`host_keeps(..., lengths=...)`, dropout_replay.map_keeps).  `tap()` captures both device read-backs, and the outputs
of forward_window, from an eager step.

Rates: P and MAP_P are the constructors' defaults; `host_keeps`, `patch_keep` and `map_keep` take the rate of the site they
restate (the model's own, the pooling heads', the map's), so a step at other rates is replayed with each site's own."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import dropout_replay as R
from multimodal_path_omic_amd import ops

FF, HEADS, LAYERS = 512, 8, 2          # make_set_transformer's defaults, as the models build their encoders
P = 0.25                               # every dropout site of the models (the constructor's default and the hard-wired ones)
MAP_P = 0.25                           # blocks.PreGatingContextualAttention's dropout_p


@contextlib.contextmanager
def recording():
    """-> the list of (span, offset) of every ops._reserve call made inside the block, in call order."""
    records = []
    reserve = ops._reserve

    def record(span):
        seed, off = reserve(span)
        records.append((int(span), int(off)))
        return seed, off
    ops._reserve = record
    try:
        yield records
    finally:
        ops._reserve = reserve


def expected_spans(kind, rows, n_slides, n_groups, d, extra=None):
    """{site: span} of one training-mode window step."""
    spans = {"snn": R.snn_span(n_slides, n_groups, d),
             "patch": rows * d // 16 + 2,
             "encoder": R.encoder_span(2 * n_slides, n_groups, d, FF, LAYERS),
             "pool": R.pool_span(2 * n_slides, n_groups, d)}
    if kind == "nacagat":
        spans["map"] = (n_groups * rows + 3) // 4
    spans.update(extra or {})
    return spans


def match_sites(records, kind, rows, n_slides, n_groups, d, extra=None):
    """{site: offset}.  Every expected site exactly once, nothing unaccounted for."""
    spans = expected_spans(kind, rows, n_slides, n_groups, d, extra)
    assert len(set(spans.values())) == len(spans), f"two sites of this geometry reserve the same span: {spans}"
    sites = {}
    for name, span in spans.items():
        offs = [o for s, o in records if s == span]
        assert len(offs) == 1, f"site '{name}' (span {span}) reserved {len(offs)} times: {records}"
        sites[name] = offs[0]
    left = [(s, o) for s, o in records if s not in spans.values()]
    assert not left and len(records) == len(spans), f"reservations no site accounts for: {left} of {records}"
    return sites


def ranges_overlap(records):
    """Pairs of records whose counter ranges [off, off + span] intersect (empty: pairwise disjoint)."""
    r = sorted((o, o + s) for s, o in records)
    return [(a, b) for a, b in zip(r, r[1:]) if b[0] <= a[1]]


def host_keeps(sites, seed, epoch, n_slides, n_groups, d, p=P, p_head=P, p_map=MAP_P, lengths=None):
    """The masks with a host restatement, window-wide: {'snn', 'encoder', 'pool'} as dropout_replay returns them.  Three rates:
    p the model's own (the constructor's `dropout`: SNN, both encoders, rho), p_head the pooling heads' scorer dropouts
    (AttentionNetGated.drop_p), p_map the K2 map's (PreGatingContextualAttention.dropout).  With `lengths` (the slides' row
    counts) and a 'map' site, 'map' is added: the per-slide keep scales of dropout_replay.map_keeps."""
    keeps = {"snn": R.snn_keeps(seed, sites["snn"], n_slides, n_groups, d, p, epoch),
             "encoder": R.encoder_keeps(seed, sites["encoder"], 2, n_slides, n_groups, d, FF, HEADS, LAYERS, p, epoch),
             "pool": R.pool_keeps(seed, sites["pool"], 2, n_slides, n_groups, d, p_head, p, True, epoch)}
    if lengths is not None and "map" in sites:
        keeps["map"] = R.map_keeps(seed, sites["map"], n_groups, lengths, p_map, epoch)
    return keeps


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def slide_keeps(keeps, b):
    """Slide b's share of host_keeps() as keyword arguments of the oracle's forward: ad_keeps, enc_keeps, pool_keeps."""
    ad = [(_t(k1[b]), _t(k2[b])) for k1, k2 in keeps["snn"]]
    enc = tuple([tuple(_t(k[br, b]) for k in layer) for layer in keeps["encoder"]] for br in (0, 1))
    pool = tuple(tuple(_t(k[br, b]) for k in keeps["pool"]) for br in (0, 1))
    return dict(ad_keeps=ad, enc_keeps=enc, pool_keeps=pool)


def patch_keep(h, p=P):
    """The patch layer's keep scale read off the training-mode H_bag (rows, d).  The patch-layer kernels draw 8 bits per
    element: the realised rate is thr8 / 256 with thr8 = round(256 p), and the survivors are scaled by 256 / (256 - thr8) --
    NOT 1 / (1 - p), which is the same number only where 256 p is an integer (0.25, 0.5)."""
    h = h.detach().float().cpu()
    zeros = float((h == 0).double().mean())
    thr8 = int(p * 256.0 + 0.5)
    assert 0.3 < zeros < 0.8 and thr8 < 256, (zeros, thr8)  # ~half ReLU zeros, thr8 / 256 of the rest dropped
    return (h > 0).double() * (256.0 / (256.0 - thr8))


def map_keep(a, p=MAP_P):
    """The K2 map's keep scale read off one slide's post-dropout map (N, M_b); 24-bit site: 1 / (1 - p)."""
    return (a.detach().cpu() > 0).double() / (1.0 - p)


@contextlib.contextmanager
def tap(model):
    """Captures, from every forward_window call inside the block, into the yielded dict: 'h' the H_bag the patch layer wrote
    (through model._patch_fc, or ops.patch_coattn_mcat on the fused bf16 MCAT path, whose third output it is), 'maps' the
    co-attention maps where the model returns them, and 'out' = (hazards, survs, Y, att)."""
    got = {}
    patch_fc, fused, forward_window = model._patch_fc, ops.patch_coattn_mcat, model.forward_window

    def tap_patch(bags):
        out = patch_fc(bags)
        got["h"] = out.data.detach()
        return out

    def tap_fused(*args, **kw):
        res = fused(*args, **kw)
        got["h"] = res[2].detach()
        return res

    def tap_forward(*args, **kw):
        res = forward_window(*args, **kw)
        got["out"] = res
        got["maps"] = res[3]["coattn"]
        return res
    model._patch_fc, ops.patch_coattn_mcat, model.forward_window = tap_patch, tap_fused, tap_forward
    try:
        yield got
    finally:
        ops.patch_coattn_mcat = fused
        del model._patch_fc, model.forward_window
