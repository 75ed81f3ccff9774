"""The oracle's training mode (keep arguments of mcat_forward / nacagat_forward / _tail) on the CPU: with every keep None,
and again with every keep all ones (unscaled), the outputs are bit-equal to the eval-mode call -- the keep arguments reach
their sites and nothing else moved.  The AlphaDropout site is exempt (an all-kept AlphaDropout is the affine map a x + b, not
the identity): it is checked against _alpha_dropout directly, and through a whole forward in which only it is live.  A keep
of zeros at each site must move the output: an argument that is accepted and dropped would pass the all-ones check."""
import pytest
import torch

import cases as C
from multimodal_path_omic_amd import synthetic as syn
from oracle import mpo_oracle as O

SIZES, M, D, FF, HEADS, LAYERS = [64] * 6, 37, C.E, 512, 8, 2
N = len(SIZES)


def _setup(kind):
    sd = syn.fill_state_dict(C.model_shapes(SIZES, kind == "nacagat"), 3101)
    wsi, omics, _, _ = C.model_inputs(M, SIZES, 3102)
    return sd, wsi, omics


def _ones(scale=1.0):
    """Every keep of one slide (all kept, unscaled), as the forward functions take them; AlphaDropout apart."""
    enc = [(torch.full((HEADS, N, N), scale), torch.full((N, D), scale), torch.full((N, FF), scale), torch.full((N, D), scale))
           for _ in range(LAYERS)]
    pool = (torch.full((N, D), scale), torch.full((N, D), scale), torch.full((D,), scale))
    return dict(keep_h=torch.full((M, D), scale), enc_keeps=(enc, enc), pool_keeps=(pool, pool))


def _forward(kind, sd, wsi, omics, **kw):
    with torch.no_grad():
        if kind == "mcat":
            hz, sv, y, att = O.mcat_forward(sd, wsi, omics, inference=True, **kw)
        else:
            hz, sv, y, att = O.nacagat_forward(sd, wsi, omics, **kw)
    return [hz, sv, y, att["coattn"], att["path"], att["omic"]]


@pytest.mark.parametrize("storage", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_none_and_all_ones_keeps_are_the_eval_forward(kind, storage):
    sd, wsi, omics = _setup(kind)
    ev = _forward(kind, sd, wsi, omics, bag_storage=storage)
    none = dict(keep_h=None, ad_keeps=None, enc_keeps=None, pool_keeps=None)
    ones = _ones()
    if kind == "nacagat":
        none["keep_map"] = None
        ones["keep_map"] = torch.ones(N, M)
    for what, kw in (("None", none), ("ones", ones)):
        got = _forward(kind, sd, wsi, omics, bag_storage=storage, **kw)
        for name, a, b in zip(("hazards", "survs", "Y", "coattn", "path", "omic"), got, ev):
            assert torch.equal(a, b), (kind, what, name)


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_a_zero_keep_at_any_site_moves_the_output(kind):
    """Each keep argument reaches a site the hazards depend on."""
    sd, wsi, omics = _setup(kind)
    ev = _forward(kind, sd, wsi, omics)[0]
    ones = _ones()
    if kind == "nacagat":
        ones["keep_map"] = torch.ones(N, M)
    enc, pool = ones["enc_keeps"][0], ones["pool_keeps"][0]
    variants = {"keep_h": dict(ones, keep_h=torch.zeros(M, D))}
    for br in (0, 1):
        for layer in range(LAYERS):
            for site in range(4):
                e = [tuple(torch.zeros_like(k) if (l, s) == (layer, site) else k for s, k in enumerate(ks)) for l, ks in enumerate(enc)]
                variants[f"enc br{br} layer{layer} site{site}"] = dict(ones, enc_keeps=(e, enc) if br == 0 else (enc, e))
        for site in range(3):
            q = tuple(torch.zeros_like(k) if s == site else k for s, k in enumerate(pool))
            variants[f"pool br{br} site{site}"] = dict(ones, pool_keeps=(q, pool) if br == 0 else (pool, q))
    if kind == "nacagat":
        variants["keep_map"] = dict(ones, keep_map=torch.zeros(N, M))
    for what, kw in variants.items():
        assert not torch.equal(_forward(kind, sd, wsi, omics, **kw)[0], ev), (kind, what)


def test_step_replay_matches_every_reservation_to_one_site():
    """tests/step_replay.py on made-up records: sites are told apart by span, each exactly once, nothing left over; the
    per-slide cut of the host masks has the shapes the oracle's forward takes."""
    import step_replay as S
    rows, b = 463, 4
    spans = S.expected_spans("nacagat", rows, b, N, D)
    assert spans == {"snn": 18456, "patch": 7410, "encoder": 73744, "pool": 9234, "map": 695}
    records, off = [], 500
    for name in ("snn", "patch", "map", "encoder", "pool"):
        records.append((spans[name], off))
        off += spans[name] + 1
    sites = S.match_sites(records, "nacagat", rows, b, N, D)
    assert sites["snn"] == 500 and sites["patch"] == 500 + 18457 and not S.ranges_overlap(records)
    assert S.ranges_overlap(records + [(3, 510)])
    with pytest.raises(AssertionError, match="map"):
        S.match_sites(records[:2] + records[3:], "nacagat", rows, b, N, D)              # a site missing
    with pytest.raises(AssertionError, match="patch"):
        S.match_sites(records + [records[1]], "nacagat", rows, b, N, D)                  # a site twice
    with pytest.raises(AssertionError, match="no site accounts for"):
        S.match_sites(records + [(5, off)], "nacagat", rows, b, N, D)                    # a stream nobody named
    S.match_sites(records + [(0, off)], "nacagat", rows, b, N, D, extra={"sampler": 0})
    with pytest.raises(AssertionError, match="no site accounts for"):
        S.match_sites(records, "mcat", rows, b, N, D)                                    # MCAT has no map stream
    keeps = S.host_keeps(sites, 77, 2, b, N, D)
    kw = S.slide_keeps(keeps, 3)
    assert len(kw["ad_keeps"]) == N and kw["ad_keeps"][0][0].shape == (D,) and kw["ad_keeps"][0][0].dtype == torch.bool
    assert [tuple(k.shape) for k in kw["enc_keeps"][1][0]] == [(HEADS, N, N), (N, D), (N, FF), (N, D)]
    assert [tuple(k.shape) for k in kw["pool_keeps"][0]] == [(N, D), (N, D), (D,)]
    other = S.slide_keeps(S.host_keeps(sites, 77, 3, b, N, D), 3)                        # the epoch moves every mask
    assert not torch.equal(other["enc_keeps"][0][0][1], kw["enc_keeps"][0][0][1])
    assert not torch.equal(other["pool_keeps"][1][2], kw["pool_keeps"][1][2])
    assert not torch.equal(other["ad_keeps"][5][1], kw["ad_keeps"][5][1])


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_alpha_dropout_site_is_alpha_dropout_of_the_snn_layers(kind):
    """ad_keeps reaches omic_fc: with only that site live, the forward equals the rest of the model fed the SNN rows that
    _alpha_dropout gives layer by layer -- for an all-kept mask (the affine map) and for a mixed one."""
    sd, wsi, omics = _setup(kind)
    g = torch.Generator().manual_seed(5)
    for keeps in ([(torch.ones(D, dtype=torch.bool),) * 2] * N,
                  [(torch.rand(D, generator=g) >= 0.25, torch.rand(D, generator=g) >= 0.25) for _ in range(N)]):
        rows = []
        for i, o in enumerate(omics):
            x = O._elu(O._lin(o.reshape(1, -1), sd, f"G.{i}.0.0"))
            x = O._alpha_dropout(x, keeps[i][0].reshape(1, -1), 0.25)
            x = O._elu(O._lin(x, sd, f"G.{i}.1.0"))
            rows.append(O._alpha_dropout(x, keeps[i][1].reshape(1, -1), 0.25))
        g_bag = torch.cat(rows, 0)
        assert torch.equal(O.omic_fc(omics, sd, ad_keeps=keeps), g_bag)
        assert not torch.equal(O.omic_fc(omics, sd), g_bag)             # all kept is not the identity
        with torch.no_grad():
            h_bag = O.patch_fc(wsi, sd)
            if kind == "mcat":
                h_co, a_co = O.mcat_coattention(g_bag, h_bag, sd, need_weights=True)
            else:
                h_co, a_co = O.pregating_contextual_attention(g_bag, h_bag, sd)
            want = O._tail(h_co, g_bag, a_co, sd)
        got = _forward(kind, sd, wsi, omics, ad_keeps=keeps)
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a, b)
