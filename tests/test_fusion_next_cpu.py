"""CPU-only checks of the gated-concat head (include/mpo_fusion_next.h): the companion header and its exports, the size and
span queries against their host restatement (tests/fusion_replay.py), refusals that come before any launch, and the fp64
restatement the GPU tests lean on against the oracle and the reference's golden vectors."""
import ctypes
import os

import pytest
import torch

import cases as C
import fusion_replay as F
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import synthetic as syn
from oracle import mpo_oracle as O

HEADER = "mpo_fusion_next.h"
GRID = [(b, d) for b in (1, 5, 32, 64, 300) for d in F.D_BUILT]
FAKE = 0x1000                  # never dereferenced: every call below is refused while its arguments are checked


def _rc(name, *args):
    rc = getattr(L.lib(), name)(*args)
    msg = L.lib().mpo_last_error()
    return rc, (msg.decode() if msg else "")


def test_companion_header_parses_and_every_entry_is_exported():
    path = [p for p in L.COMPANION_HEADER_PATHS if os.path.basename(p) == HEADER]
    assert len(path) == 1 and os.path.dirname(path[0]) == os.path.dirname(L.HEADER_PATH)
    with open(path[0]) as f:
        signatures, constants, version = L.parse_header(f.read())
    assert not constants and version is None                       # entries only: no enum, no ABI version of its own
    assert list(signatures) == L.companion_symbols(HEADER) and len(signatures) == 16
    assert L.all_companion_symbols() == L.companion_symbols() + L.companion_symbols(HEADER)
    handle = ctypes.CDLL(L.LIB_PATH)
    for name, (res, args) in signatures.items():
        assert hasattr(handle, name), f"{name} declared in include/{HEADER} but not exported"
        assert name not in L.exported_symbols()
        fn = getattr(L.lib(), name)
        assert fn.restype is res and list(fn.argtypes) == args
    with open(L.HEADER_PATH) as f:
        assert f'#include "{HEADER}"' in f.read()
    assert L.lib().mpo_abi_version() == 14 and L.ABI_VERSION == 14
    assert L.lib().mpo_gated_concat_head_rng_span.restype is ctypes.c_uint64
    assert L.lib().mpo_gated_concat_head_loss_forward.argtypes[12] is ctypes.c_int          # loss_kind: a plain int


@pytest.mark.parametrize("b,d", GRID)
def test_span_and_size_queries_equal_their_host_restatement(b, d):
    lib = L.lib()
    assert lib.mpo_gated_concat_head_rng_span(b, d) == F.gated_concat_span(b, d) == 0       # no dropout site, no counters
    for c in (1, 4, F.MAX_CLASSES):
        assert lib.mpo_gated_concat_head_saved_floats(b, d, c) == F.gated_concat_saved_floats(b, d, c, False)
        assert lib.mpo_gated_concat_head_loss_saved_floats(b, d, c) == F.gated_concat_saved_floats(b, d, c, True)
        assert lib.mpo_gated_concat_head_workspace_bytes(b, d, c) == F.gated_concat_workspace_bytes(b, d, c)


def _fwd(h0=FAKE, h1=FAKE + 1024, ld=512, b=3, d=256, c=4, params=FAKE, hz=FAKE, sv=FAKE, y=FAKE, saved=FAKE):
    return _rc("mpo_gated_concat_head_forward", h0, h1, ld, b, d, c, params, hz, sv, y, saved, None)


def _bwd(ws_bytes, h0=FAKE, ld=512, b=3, d=256, c=4, dh0=FAKE, ws=FAKE):
    return _rc("mpo_gated_concat_head_backward", h0, FAKE + 1024, ld, b, d, c, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, None,
               dh0, FAKE + 1024, FAKE, ws, ws_bytes, None)


def _loss_fwd(kind=0, label=FAKE, d=256, c=4):
    return _rc("mpo_gated_concat_head_loss_forward", FAKE, FAKE + 1024, 512, 3, d, c, FAKE, label, FAKE, FAKE, 0.75, 1e-7, kind,
               FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None)


def _loss_bwd(ws_bytes, d=256, saved=FAKE):
    return _rc("mpo_gated_concat_head_loss_backward", FAKE, FAKE + 1024, 512, 3, d, 4, FAKE, saved, FAKE, FAKE + 1024, FAKE,
               FAKE, ws_bytes, None)


def test_refusals_come_before_any_launch():
    """On a machine without a GPU a launch would fail with a HIP error; every case here is refused with its own reason."""
    need = L.lib().mpo_gated_concat_head_workspace_bytes(3, 256, 4)
    for (rc, msg), text in ((_bwd(need - 257), "workspace too small"),
                            (_loss_bwd(need - 257), "workspace too small"),
                            (_loss_bwd(0), "workspace too small"),
                            (_fwd(h0=None), "null argument"),
                            (_fwd(saved=None), "null argument"),
                            (_fwd(params=None), "null argument"),
                            (_bwd(need, dh0=None), "null argument"),
                            (_bwd(need, ws=None), "null argument"),
                            (_loss_fwd(label=None), "null argument"),
                            (_loss_bwd(need, saved=None), "null argument"),
                            (_fwd(d=192, ld=384), "d 192 is not 128, 256 or 512"),
                            (_bwd(need, d=192, ld=384), "d 192 is not 128, 256 or 512"),
                            (_loss_fwd(d=192), "d 192 is not 128, 256 or 512"),
                            (_loss_bwd(need, d=192), "d 192 is not 128, 256 or 512"),
                            (_fwd(d=1024, ld=2048), "d 1024 is not 128, 256 or 512"),
                            (_fwd(c=0), "n_classes 0 not in 1..16"),
                            (_fwd(c=17), "n_classes 17 not in 1..16"),
                            (_loss_fwd(c=17), "n_classes 17 not in 1..16"),
                            (_fwd(b=0), "n_slides 0 not in"),
                            (_fwd(ld=255), "row stride 255"),
                            (_fwd(ld=258), "row stride 258"),
                            (_fwd(h0=FAKE + 4), "not 16-byte aligned"),
                            (_bwd(need, dh0=FAKE + 8), "not 16-byte aligned"),
                            (_loss_fwd(kind=2), "loss_kind 2")):
        assert rc == 1 and text in msg, (text, rc, msg)


def _concat(name, *, hcat=FAKE, params=FAKE, label=FAKE, hz=FAKE, saved=FAKE):
    geom = (hcat, 3, 512, 256, 256, 4, params)
    if name == "forward":
        return _rc("mpo_fusion_head_forward", *geom, hz, FAKE, FAKE, saved, None)
    if name == "loss_forward":
        return _rc("mpo_fusion_head_loss_forward", *geom, label, FAKE, FAKE, 0.75, 1e-7, hz, FAKE, FAKE, FAKE, FAKE, saved, None)
    return _rc("mpo_fusion_head_sct_loss_forward", *geom, label, FAKE, FAKE, 1e-7, hz, FAKE, FAKE, FAKE, FAKE, saved, None)


def test_concat_forward_entries_refuse_null_arguments():
    """K6's three forward entries answer a missing pointer as the other two fusions' do, naming themselves (its two backward
    entries answer an empty call with 'workspace too small', tests/test_host_cpu.py)."""
    for name, who in (("forward", "fusion head forward"), ("loss_forward", "fusion head + loss forward"),
                      ("sct_loss_forward", "fusion head + sct loss forward")):
        for kw in (dict(hcat=None), dict(params=None), dict(hz=None), dict(saved=None)) + ((dict(label=None),) if name != "forward" else ()):
            rc, msg = _concat(name, **kw)
            assert rc == 1 and msg == who + ": null argument", (name, kw, rc, msg)


def _golden_case():
    sd = syn.fill_state_dict(C.GATED_CONCAT_SHAPES, 720)
    hp, ho, _ = C.fusion_inputs()
    return sd, hp, ho


def test_fp64_restatement_equals_the_oracle():
    """Per slide the helper IS oracle.gated_concat_fusion + survival_head + ces_loss (to 1e-12), also for a window of slides."""
    sd, hp, ho = _golden_case()
    cls = syn.fill_state_dict({"classifier.weight": (4, C.E), "classifier.bias": (4,)}, 721)
    p = {k: v.double() for k, v in {**sd, **cls}.items()}
    po = {**{"fusion_layer." + k: v for k, v in p.items() if not k.startswith("classifier")},
          "classifier.weight": p["classifier.weight"], "classifier.bias": p["classifier.bias"]}
    h_path = torch.stack([hp, ho * 0.5, -hp]).double()
    h_omic = torch.stack([ho, hp, ho * 2.0]).double()
    label, cens = torch.tensor([2, 0, 3]), torch.tensor([0.0, 1.0, 0.0])
    fused, hz, sv, y = F.gated_concat_head(h_path, h_omic, p)
    loss, risk, *_ = F.gated_concat_head_loss(h_path, h_omic, p, label, cens, "ces")
    for b in range(3):
        ref = O.gated_concat_fusion(h_path[b], h_omic[b], po)
        assert float((fused[b] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
        hz_o, sv_o, y_o = O.survival_head(ref, po)
        for got, want in ((hz[b], hz_o[0]), (sv[b], sv_o[0]), (y[b], y_o[0])):
            assert float((got - want).abs().max()) <= 1e-12
        assert abs(float(loss[b] - O.ces_loss(hz_o, sv_o, label[b:b + 1], cens[b:b + 1]))) <= 1e-12
        assert abs(float(risk[b] - O.risk_score(sv_o)[0])) <= 1e-12


def test_fp64_restatement_reproduces_the_reference_golden(golden):
    """fusion_next.npz (the reference's own GatedConcatFusion, fp32) at the bars the GPU layer is held to against that file
    (tests/test_gpu_tail.py: output 1e-4 relative, gradients 2e-3 of the reference gradient's max)."""
    g = golden("fusion_next")
    sd, hp, ho = _golden_case()
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    a, b = hp.double().requires_grad_(True), ho.double().requires_grad_(True)
    y = F.gated_concat_fusion(a[None], b[None], p)[0]
    ref = g["gated_concat/out"].double()
    assert y.shape == ref.shape
    assert float((y.detach() - ref).abs().max() / ref.abs().max()) < 1e-4
    probe = syn.normal(syn.rng(711), tuple(y.shape)).double()
    names = ["h_path", "h_omic"] + list(sd)
    grads = torch.autograd.grad((y * probe).sum(), [a, b] + [p[k] for k in sd])
    for n, gr in zip(names, grads):
        want = g["gated_concat/grad/" + n].double()
        err = float((syn.subsample(gr) - want).abs().max()) / max(float(want.abs().max()), 1e-5)
        assert err < 2e-3, (n, err)


# ------------------------------------------------------------------------------------------- bilinear head
@pytest.mark.parametrize("b,d", GRID)
def test_bilinear_span_and_sites(b, d):
    """The span query equals its restatement; every site's counters lie inside the span; no two sites share a counter."""
    span = L.lib().mpo_bilinear_head_rng_span(b, d)
    assert span == F.bilinear_span(b, d) > 0
    off = 1000
    sites = F.bilinear_sites(b, d, off)
    assert [n for n, _, _ in sites] == list(F.BILINEAR_SITES) and len(sites) == 5      # two of the five are per branch
    for (name, lo, hi), n in zip(sites, F.bilinear_site_elements(b, d)):
        assert off <= lo < hi <= off + span, name
        assert hi - lo == (n + 3) // 4, name
    for (_, _, hi), (name, lo, _) in zip(sites, sites[1:]):
        assert hi <= lo, name                                                           # ascending and disjoint
    # ops._reserve(span) hands the next call off + span + 1: its first counter is behind this call's last
    assert sites[-1][2] <= off + span + 1


def test_bilinear_keep_masks_are_distinct_per_site_and_epoch():
    k0 = F.bilinear_keeps(77, 500, 33, 256, 0.25)
    k1 = F.bilinear_keeps(77, 500, 33, 256, 0.25, epoch=1)
    assert not torch.equal(k0["linear_o1"], k0["linear_o2"])
    for name in F.BILINEAR_SITES:
        assert set(k0[name].unique().tolist()) == {0.0, 1.0 / 0.75}
        assert not torch.equal(k0[name], k1[name])


def _bil(name, *, h0=FAKE, ld=512, b=3, d=256, hid=32, mm=64, c=4, params=FAKE, p=0.0, saved=FAKE, ws=FAKE, ws_bytes=None, dh0=FAKE,
         label=FAKE, kind=0):
    h1, dh1 = FAKE + 1024, FAKE + 1024
    head = (h0, h1, ld, b, d, hid, mm, c, params, p, 1, 0, None)
    if ws_bytes is None:
        ws_bytes = L.lib().mpo_bilinear_head_workspace_bytes(3, 256, 4)
    if name == "forward":
        return _rc("mpo_bilinear_head_forward", *head, FAKE, FAKE, FAKE, saved, None)
    if name == "backward":
        return _rc("mpo_bilinear_head_backward", *head, saved, FAKE, FAKE, FAKE, None, None, None, dh0, dh1, FAKE, ws, ws_bytes, None)
    if name == "loss_forward":
        return _rc("mpo_bilinear_head_loss_forward", *head, label, FAKE, FAKE, 0.75, 1e-7, kind, FAKE, FAKE, FAKE, FAKE, FAKE, saved, None)
    return _rc("mpo_bilinear_head_loss_backward", *head, saved, dh0, dh1, FAKE, ws, ws_bytes, None)


def test_bilinear_refusals_come_before_any_launch():
    need = L.lib().mpo_bilinear_head_workspace_bytes(3, 256, 4)
    for (rc, msg), text in ((_bil("backward", ws_bytes=need - 257), "workspace too small"),
                            (_bil("loss_backward", ws_bytes=need - 257), "workspace too small"),
                            (_bil("loss_backward", ws_bytes=0), "workspace too small"),
                            (_bil("forward", h0=None), "null argument"),
                            (_bil("forward", saved=None), "null argument"),
                            (_bil("backward", dh0=None), "null argument"),
                            (_bil("loss_forward", label=None), "null argument"),
                            (_bil("loss_backward", ws=None), "null argument"),
                            (_bil("forward", d=192, ld=384), "d 192 is not 128, 256 or 512"),
                            (_bil("backward", d=192, ld=384), "d 192 is not 128, 256 or 512"),
                            (_bil("loss_forward", d=192, ld=384), "d 192 is not 128, 256 or 512"),
                            (_bil("loss_backward", d=192, ld=384), "d 192 is not 128, 256 or 512"),
                            (_bil("forward", hid=16), "hidden_size 16 is not 32"),
                            (_bil("backward", hid=64), "hidden_size 64 is not 32"),
                            (_bil("loss_forward", hid=33), "hidden_size 33 is not 32"),
                            (_bil("loss_backward", hid=31), "hidden_size 31 is not 32"),
                            (_bil("forward", mm=32), "mm_hidden_size 32 is not 64"),
                            (_bil("forward", c=17), "n_classes 17 not in 1..16"),
                            (_bil("forward", b=0), "n_slides 0 not in"),
                            (_bil("forward", ld=255), "row stride 255"),
                            (_bil("forward", h0=FAKE + 4), "not 16-byte aligned"),
                            (_bil("backward", dh0=FAKE + 8), "not 16-byte aligned"),
                            (_bil("forward", p=1.0), "dropout probability"),
                            (_bil("loss_forward", kind=2), "loss_kind 2")):
        assert rc == 1 and text in msg, (text, rc, msg)


@pytest.mark.parametrize("b,d,c", [(1, 128, 4), (5, 256, 4), (300, 512, 16)])
def test_bilinear_size_queries_follow_their_layout(b, d, c):
    lib = L.lib()
    pad = lambda n: (n + 63) // 64 * 64                                                 # noqa: E731
    blocks = [2 * b * 32] * 4 + [2 * 32 * 4 * b, b * 130, b * d, b * c]
    assert lib.mpo_bilinear_head_saved_floats(b, d, c) == sum(pad(n) for n in blocks)
    assert lib.mpo_bilinear_head_loss_saved_floats(b, d, c) == sum(pad(n) for n in blocks + [b * c])
    end = 0
    for n in (b * c, b * d, b * 130, b * 64, 2 * b * 32, 2 * b * 32, 2 * b * 32, 2 * b * 32, 2 * 32 * b * d, 2 * 128 * b * d):
        end = (end + 255) // 256 * 256 + 4 * n
    assert lib.mpo_bilinear_head_workspace_bytes(b, d, c) == end + 256


def test_bilinear_fp64_restatement_equals_the_oracle():
    """All-ones masks: per slide the helper IS oracle.bilinear_fusion (to 1e-12), also for a window of slides."""
    sd = syn.fill_state_dict(C.BILINEAR_SHAPES, 710, gain=3.0)
    hp, ho, _ = C.fusion_inputs()
    p = {k: v.double() for k, v in sd.items()}
    po = {"fusion_layer." + k: v for k, v in p.items()}
    x1, x2 = torch.stack([hp, ho * 0.5, -hp]).double(), torch.stack([ho, hp, ho * 2.0]).double()
    for keeps in (None, F.bilinear_ones(3, C.E)):
        fused = F.bilinear_fusion(x1, x2, p, keeps)
        for b in range(3):
            ref = O.bilinear_fusion(x1[b], x2[b], po)
            assert float((fused[b] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_bilinear_fp64_restatement_reproduces_the_reference_golden(golden):
    g = golden("fusion_next")
    sd = syn.fill_state_dict(C.BILINEAR_SHAPES, 710, gain=3.0)
    hp, ho, _ = C.fusion_inputs()
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    a, b = hp.double().requires_grad_(True), ho.double().requires_grad_(True)
    y = F.bilinear_fusion(a[None], b[None], p)[0]
    ref = g["bilinear/out"].double()
    assert y.shape == ref.shape
    assert float((y.detach() - ref).abs().max() / ref.abs().max()) < 1e-4
    probe = syn.normal(syn.rng(711), tuple(y.shape)).double()
    names = ["h_path", "h_omic"] + list(sd)
    grads = torch.autograd.grad((y * probe).sum(), [a, b] + [p[k] for k in sd])
    for n, gr in zip(names, grads):
        want = g["bilinear/grad/" + n].double()
        err = float((syn.subsample(gr) - want).abs().max()) / max(float(want.abs().max()), 1e-5)
        assert err < 2e-3, (n, err)
