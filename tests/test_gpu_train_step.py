"""The whole training-mode window step of the fusion models (MCAT, NaCAGaT), every dropout site live:

  * the EAGER step (bucket.begin, harness.train_window, bucket.finish) against the fp64 oracle run with the step's own masks
    -- per-slide loss, risk, hazards, both pooling score vectors and every parameter's gradient from the bucket views.  The
    masks come from tests/step_replay.py: every ops._reserve of the step is recorded and matched to its site, the SNN's,
    the encoders' and the pooling heads' masks are rebuilt on the host for (seed, epoch), the patch layer's and the K2 map's
    are read back from the device.  Each case runs without an epoch tensor and with one set to 2; MCAT with the bilinear
    head (five more dropout sites, restated by tests/fusion_replay.py) at epoch 2.
  * the CAPTURED step (harness.GraphedWindowStep) against its eager twin: a second model with the same weights stepped
    eagerly at (seed, the first offset the captured body reserved, the epoch the replay runs at) draws the replay's masks,
    so the two must agree as closely as two eager runs agree with each other -- also with Adam inside the graph, with the
    patch layer's weight gradient split into a second graph, with the row sampler in front and with the bilinear head.

Window: four slides of 300, 129, 33 and 1 rows (several 32-row tiles; one row past the 128-row edge; one row past a tile; a
single row), six omic groups of 64 features, the medium model, 4 classes, grad_acc_step 4.  Every stage's own shape edges
are pinned by its own test; this file is about the composition: a site that ignores the epoch, two sites on overlapping
counters, a backward that regenerates another mask than its forward drew, a wrong keep scale handed from the patch layer to
the co-attention backward.

Bars (max-norm relative error, tail_helpers.relerr / grad_errs).  None is new; each is the one an existing test applies to
that quantity, named beside it in `_bars`.  The controls replay, site by site, the masks of the NEXT epoch in the oracle:
each must miss those bars."""
import contextlib

import pytest
import torch

import cases as C
import fusion_replay as F
import step_replay as S
from multimodal_path_omic_amd import _lib as L
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatAdam, FlatGradBucket
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer
from multimodal_path_omic_amd.ops import BagBatch
from oracle import mpo_oracle as O
from tail_helpers import grad_errs, relerr
from test_gpu_coattn_nacagat import GRAD_TOL_BF16_PARAM

pytestmark = pytest.mark.gpu

SIZES = [64] * 6
N, D = len(SIZES), C.E
LENGTHS = [300, 129, 33, 1]
ROWS, B, ACC = sum(LENGTHS), len(LENGTHS), 4
SEED, BASE = 20261019, 7001                  # the generator's seed and the counter value every pinned step starts from
WEIGHTS, INPUTS = 61, 62
KINDS = ["mcat", "nacagat"]
DTYPES = [torch.float32, torch.bfloat16]
DTYPE_IDS = ["fp32", "bf16"]
TAIL = ("G.", "path_transformer.", "omic_transformer.", "path_attention_head.", "omic_attention_head.", "path_rho.", "omic_rho.")


def _bars(dtype):
    """{quantity: bar}; gradients: 'grad/tail' (the SNN, both encoders, both pooling heads), 'grad/H' (the patch layer),
    'grad/rest' (co-attention, fusion layer, classifier)."""
    if dtype == torch.float32:
        return {"loss": 1e-4,          # test_gpu_models.py::test_model_matches_reference_golden (loss)
                "risk": 1e-4,          # ... (survs; risk = -sum survs)
                "hazards": 1e-4,       # ... (hazards)
                "path": 1e-3,          # ... (A_path)
                "omic": 1e-3,          # ... (A_omic)
                "grad/tail": 2e-3,     # test_gpu_train_dropout.py (tail_helpers.GRAD_TOL: tail and SNN gradients)
                "grad/H": 5e-3,        # test_gpu_train_dropout.py::test_ge_model_training_step_equals_fp64_oracle
                "grad/rest": 5e-3}     # ... (every parameter of a whole model on an fp32 window)
    return {"loss": 2e-4,              # test_gpu_models.py::test_model_bf16_bag_within_north_star (hazards against the same-storage
            "risk": 2e-4,              #  oracle; loss and risk are functions of hazards / survs alone)
            "hazards": 2e-4,           # ... (hazards against the same-storage oracle)
            "path": 1e-3,              # test_gpu_models.py::test_model_bf16_bag_vs_fp32_reference_golden (path map: 1e-3 where
            "omic": 1e-3,              #  the storage floor allows; the oracle here is fed the same stored values)
            "grad/tail": GRAD_TOL_BF16_PARAM,      # test_gpu_coattn_nacagat.py (parameter gradients on a bf16 bag)
            "grad/H": 2e-2,            # test_gpu_patch_coattn.py::test_fused_dropout_masks (H.0.* with a replayed mask),
            #                            test_gpu_models.py::test_model_bf16_bag_within_north_star (H.* of both models)
            "grad/rest": GRAD_TOL_BF16_PARAM}      # test_gpu_coattn_nacagat.py


def _grad_class(name):
    return "grad/H" if name.startswith("H.") else ("grad/tail" if name.startswith(TAIL) else "grad/rest")


# ------------------------------------------------------------------------------------------- models, window, generator
def _slides(lengths=LENGTHS):
    g = syn.rng(INPUTS)
    return [dict(wsi=syn.normal(g, (m, 1024)), omics=[syn.normal(g, (s,)) for s in SIZES], survival_class=(b + 1) % 4,
                 censorship=b % 2) for b, m in enumerate(lengths)]


def _build(dev, kind, dtype, fusion="concat", rates=None):
    """rates: None (every site at the constructors' 0.25) or (the model's `dropout`, the pooling heads' drop_p)."""
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=SIZES, bag_dtype=dtype, fusion=fusion, **({} if rates is None else {"dropout": rates[0]}))
    if rates is not None:
        model.path_attention_head.drop_p = model.omic_attention_head.drop_p = float(rates[1])
    shapes = C.model_shapes(SIZES, kind == "nacagat") if fusion == "concat" else \
        {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = syn.fill_state_dict(shapes, WEIGHTS)
    model.load_state_dict(sd, strict=True)
    return model.to(dev).train(), sd


@contextlib.contextmanager
def _generator_restored():
    """No epoch tensor on entry; the generator's three values as they were on exit, whatever happened in between."""
    ops.set_rng_epoch(None)
    keep = ops.rng_state()
    try:
        yield
    finally:
        ops.set_rng_epoch(None)
        ops.set_rng_state(keep)


def _pin(dev, calls, epoch):
    """(SEED, calls, epoch); epoch None: no epoch tensor installed."""
    if epoch is None:
        ops.set_rng_epoch(None)
    elif ops._rng_epoch_tensor is None:
        ops.set_rng_epoch(torch.zeros(1, dtype=torch.int64, device=dev))
    ops.set_rng_state({"seed": SEED, "calls": calls, "epoch": epoch})
    assert torch.initial_seed() == SEED and ops._rng_calls == calls


# ------------------------------------------------------------------------------------------- the eager step and its oracle
_RUNS = {}          # (kind, dtype, fusion, epoch, rates) -> the eager step's outputs and masks; computed once per case, never written afterwards


def _head_sites(fusion):
    """The reservations a fusion head adds to the step's (the bilinear layer's five dropout sites are one reservation)."""
    return {"bilinear head": F.bilinear_span(B, D)} if fusion == "bilinear" else None


def _eager_run(dev, kind, dtype, epoch, fusion="concat", rates=None):
    """rates: see _build; the masks are then rebuilt at those rates (the K2 map's stays at the module's own S.MAP_P)."""
    key = (kind, dtype, fusion, epoch, rates)
    if key in _RUNS:
        return _RUNS[key]
    if any(k[:3] != key[:3] or k[4] != rates for k in _RUNS):    # one case's runs at a time (each holds a model's worth of gradients)
        _RUNS.clear()
    p, p_head = (S.P, S.P) if rates is None else rates
    model, sd = _build(dev, kind, dtype, fusion, rates)
    window = harness.make_window(_slides(), dev, dtype)
    bucket = FlatGradBucket(list(model.parameters()))
    _pin(dev, BASE, epoch)
    with S.recording() as records, S.tap(model) as got:
        bucket.begin()
        loss, risk = harness.train_window(model, *window, ACC)
        bucket.finish()
    torch.cuda.synchronize()
    hz, _, _, att = got["out"]
    run = dict(sd=sd, fusion=fusion, records=list(records), loss=loss.detach().cpu(), risk=risk.detach().cpu(), hazards=hz.detach().cpu(),
               path=att["path"].detach().cpu(), omic=att["omic"].detach().cpu(),
               grads={n: p._mpo_grad_view.detach().cpu().clone() for n, p in model.named_parameters()},
               p=p, keep_h=S.patch_keep(got["h"], p),
               keep_maps=[S.map_keep(a) for a in got["maps"]] if kind == "nacagat" else None)
    assert tuple(got["h"].shape) == (ROWS, D) and run["path"].shape == (B, 1, N)
    run["sites"] = S.match_sites(run["records"], kind, ROWS, B, N, D, _head_sites(fusion))
    run["host"] = S.host_keeps(run["sites"], SEED, epoch or 0, B, N, D, p, p_head, S.MAP_P, LENGTHS)
    if fusion == "bilinear":
        rate = ops._bilinear_drop_p(model.fusion_layer, True)
        assert rate > 0
        run["head_keeps"] = F.bilinear_keeps(SEED, run["sites"]["bilinear head"], B, D, rate, epoch or 0)
    _RUNS[key] = run
    return run


def _oracle(kind, dtype, run, host=None, keep_h=None, keep_maps=None, head_keeps=None):
    """The fp64 step on the stored operands, slide by slide, under the given masks (default: the run's own) -> the quantities
    _compare reads."""
    if run["fusion"] == "bilinear":
        return _oracle_bilinear(run, host, keep_h, head_keeps)
    host = run["host"] if host is None else host
    keep_h = run["keep_h"] if keep_h is None else keep_h
    keep_maps = run["keep_maps"] if keep_maps is None else keep_maps
    slides = _slides()
    p = {k: v.double().requires_grad_(True) for k, v in run["sd"].items()}
    storage = torch.bfloat16 if dtype == torch.bfloat16 else None
    out = dict(loss=[], risk=[], hazards=[], path=[], omic=[])
    total, row = 0.0, 0
    for b, s in enumerate(slides):
        m = s["wsi"].shape[0]
        kw = S.slide_keeps(host, b)
        kw["keep_h"] = keep_h[row:row + m]
        if kind == "nacagat":
            kw["keep_map"] = keep_maps[b]
        fwd = O.mcat_forward if kind == "mcat" else O.nacagat_forward
        hz, sv, _, att = fwd(p, s["wsi"], s["omics"], bag_storage=storage, drop_p=run["p"], **kw)
        loss = O.ces_loss(hz, sv, torch.tensor([s["survival_class"]]), torch.tensor([float(s["censorship"])]))
        total = total + loss / ACC                               # slide weight 1 / grad_acc_step
        for k, v in (("loss", loss.reshape(())), ("risk", O.risk_score(sv)[0]), ("hazards", hz[0]), ("path", att["path"]),
                     ("omic", att["omic"])):
            out[k].append(v.detach())
        row += m
    total.backward()
    out = {k: torch.stack(v) for k, v in out.items()}
    out["grads"] = {n: (p[n].grad if p[n].grad is not None else torch.zeros_like(p[n])) for n in p}
    return out


def _oracle_bilinear(run, host=None, keep_h=None, head_keeps=None):
    """_oracle for MCAT with fusion="bilinear" (fp32 window): the oracle's pieces up to the pooled rows slide by slide, then
    the head of tests/fusion_replay.py on the (B, d) rows under the head's five masks."""
    host = run["host"] if host is None else host
    keep_h = run["keep_h"] if keep_h is None else keep_h
    head_keeps = run["head_keeps"] if head_keeps is None else head_keeps
    slides = _slides()
    p = {k: v.double().requires_grad_(True) for k, v in run["sd"].items()}
    head = {k[len("fusion_layer."):]: v for k, v in p.items() if k.startswith("fusion_layer.")}
    head.update({k: p[k] for k in F.HEAD_NAMES})
    rows, row = dict(path=[], omic=[], h_path=[], h_omic=[]), 0
    for b, s in enumerate(slides):
        m = s["wsi"].shape[0]
        kw = S.slide_keeps(host, b)
        g_bag = O.omic_fc(s["omics"], p, ad_keeps=kw["ad_keeps"])
        h_co, _ = O.mcat_coattention(g_bag, O.patch_fc(s["wsi"], p, keep=keep_h[row:row + m]), p, need_weights=False)
        a_path, h_path, a_omic, h_omic = O._pooled(h_co, g_bag, p, kw["enc_keeps"], kw["pool_keeps"])
        for k, v in (("path", a_path.detach()), ("omic", a_omic.detach()), ("h_path", h_path), ("h_omic", h_omic)):
            rows[k].append(v)
        row += m
    label = torch.tensor([s["survival_class"] for s in slides])
    cens = torch.tensor([float(s["censorship"]) for s in slides])
    loss, risk, hz, _, _ = F.bilinear_head_loss(torch.stack(rows["h_path"]), torch.stack(rows["h_omic"]), head, label, cens, "ces",
                                                head_keeps)
    (loss / ACC).sum().backward()                                # slide weight 1 / grad_acc_step
    out = dict(loss=loss.detach(), risk=risk.detach(), hazards=hz.detach(), path=torch.stack(rows["path"]),
               omic=torch.stack(rows["omic"]))
    out["grads"] = {n: (p[n].grad if p[n].grad is not None else torch.zeros_like(p[n])) for n in p}
    return out


def _compare(run, ora, dtype):
    """{quantity: (error, bar)}; the three gradient classes carry their worst parameter's name."""
    bars = _bars(dtype)
    errs = {k: (relerr(run[k], ora[k]), bars[k]) for k in ("loss", "risk", "hazards", "path", "omic")}
    worst = {}
    for n, g in run["grads"].items():
        e = grad_errs([g], [ora["grads"][n]])[0]
        c = _grad_class(n)
        if c not in worst or e > worst[c][0]:
            worst[c] = (e, n)
    for c, (e, n) in worst.items():
        errs[c] = (e, bars[c], n)
    return errs


def _line(errs):
    return " ".join(f"{k} {v[0]:.1e}" + (f" ({v[2]})" if len(v) > 2 else "") for k, v in errs.items())


def _factor(errs):
    """By how much the worst quantity misses its bar (<= 1: every assertion of the step test holds)."""
    return max(v[0] / v[1] for v in errs.values())


def _installed(epoch):
    return "no epoch tensor" if epoch is None else f"epoch tensor = {epoch}"


@pytest.mark.parametrize("epoch", [None, 2], ids=["no_epoch_tensor", "epoch_2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_eager_training_step_equals_fp64_oracle(dev, kind, dtype, epoch):
    with _generator_restored():
        run = _eager_run(dev, kind, dtype, epoch)
        assert not S.ranges_overlap(run["records"]), (S.ranges_overlap(run["records"]), run["records"])
        if epoch is not None:                                # the epoch moved every mask: nothing of the epoch-0 step is left
            other = _eager_run(dev, kind, dtype, None)
            assert other["sites"] == run["sites"]
            assert not torch.equal(other["keep_h"], run["keep_h"]) and not torch.equal(other["loss"], run["loss"])
        errs = _compare(run, _oracle(kind, dtype, run), dtype)
        print(f"[train step] {kind} {DTYPE_IDS[DTYPES.index(dtype)]} {_installed(epoch)}: {_line(errs)}")
        for k, v in errs.items():
            assert v[0] < v[1], (k, v)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_step_controls_next_epoch_masks_at_one_site_fail(dev, kind, dtype):
    """The oracle fed ONE site's masks as drawn at the next epoch (everything else right) must miss the bars of
    test_eager_training_step_equals_fp64_oracle: patch layer, SNN, encoders, pooling heads, and the K2 map for NaCAGaT."""
    with _generator_restored():
        run = _eager_run(dev, kind, dtype, 2)
        nxt = _eager_run(dev, kind, dtype, 3)                # (the device-read masks of the next epoch)
        assert nxt["sites"] == run["sites"]
        right = _factor(_compare(run, _oracle(kind, dtype, run), dtype))
        wrong = {"patch": dict(keep_h=nxt["keep_h"])}
        for site in ("snn", "encoder", "pool"):
            wrong[site] = dict(host=dict(run["host"], **{site: nxt["host"][site]}))
        if kind == "nacagat":
            wrong["map"] = dict(keep_maps=nxt["keep_maps"])
        for site, kw in wrong.items():
            errs = _compare(run, _oracle(kind, dtype, run, **kw), dtype)
            worst = max(errs, key=lambda k: errs[k][0] / errs[k][1])
            print(f"  control [{kind} {DTYPE_IDS[DTYPES.index(dtype)]}] {site} masks of epoch 3: {_factor(errs):.0f} x the bar "
                  f"({worst}; the right masks: {right:.2f} x)")
            assert _factor(errs) > 1.0, (site, errs)


def test_eager_bilinear_training_step_equals_fp64_oracle(dev):
    """MCAT with fusion="bilinear" on the fp32 window at epoch 2: the head's five dropout sites (one more reservation) replayed
    through tests/fusion_replay.py, everything in front of it as above.  Same bars; the controls: the head's masks, and each
    other site's, as drawn at epoch 3."""
    kind, dtype = "mcat", torch.float32
    with _generator_restored():
        run = _eager_run(dev, kind, dtype, 2, "bilinear")
        nxt = _eager_run(dev, kind, dtype, 3, "bilinear")
        assert not S.ranges_overlap(run["records"]) and nxt["sites"] == run["sites"]
        errs = _compare(run, _oracle(kind, dtype, run), dtype)
        print(f"[train step] mcat fp32 bilinear {_installed(2)}: {_line(errs)}")
        for k, v in errs.items():
            assert v[0] < v[1], (k, v)
        wrong = {"bilinear head": dict(head_keeps=nxt["head_keeps"]), "patch": dict(keep_h=nxt["keep_h"])}
        for site in ("snn", "encoder", "pool"):
            wrong[site] = dict(host=dict(run["host"], **{site: nxt["host"][site]}))
        for site, kw in wrong.items():
            bad = _compare(run, _oracle(kind, dtype, run, **kw), dtype)
            print(f"  control [mcat fp32 bilinear] {site} masks of epoch 3: {_factor(bad):.0f} x the bar "
                  f"(the right masks: {_factor(errs):.2f} x)")
            assert _factor(bad) > 1.0, (site, bad)


# ------------------------------------------------------------------------------------------- captured step against its twin
# Gradients that are bit-stable from one eager run to the next but may differ in a replay by two fp32 summation orders
# (1e-5 max-norm relative, test_gpu_hand_on_grads.py::TOL): only tensors behind one of the atomic accumulation sites
# (tail.hip's chunked pooling-scorer sums, gemm_f32_longk.hip's K slices, patch_epilogue.hip's column sums) may be named
# here, each with its site.  None is needed: at this window every one of them takes its single-chunk, fixed-order form.
ATOMIC_SITES = {}
ATOMIC_TOL = 1e-5


def _snapshot(model, bucket, loss, risk, opt=None):
    snap = {"loss": loss.detach().clone(), "risk": risk.detach().clone(), "bucket": bucket.flat.clone()}
    for n, p in model.named_parameters():
        snap["grad/" + n] = p._mpo_grad_view.clone()
    if opt is not None:
        snap.update(flat_p=opt.flat_p.clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone())
    return snap


def _maxabs(a, b):
    return float((a.double() - b.double()).abs().max())


def _misses(a, a_again, b):
    """tests/test_gpu_checkpoint.py::_hold per tensor: `b` against `a`, with `a_again` (a second run of what made `a`) as the
    yardstick -- bit-identical where a and a_again are, within twice their difference elsewhere (and ATOMIC_SITES).
    -> ([(tensor, noise, diff)] of the tensors that miss, the largest noise, the largest relative difference)."""
    assert a.keys() == a_again.keys() == b.keys()
    bad, noise_max, rel_max = [], 0.0, 0.0
    for k in a:
        assert bool(torch.isfinite(b[k]).all()) and bool(torch.isfinite(a[k]).all()), k
        noise, diff = _maxabs(a[k], a_again[k]), _maxabs(a[k], b[k])
        ok = torch.equal(a[k], b[k]) if noise == 0.0 else diff <= 2 * noise
        if not ok and k in ATOMIC_SITES and noise == 0.0:
            ok = relerr(b[k], a[k]) <= ATOMIC_TOL
        if not ok:
            bad.append((k, noise, diff))
        noise_max, rel_max = max(noise_max, noise), max(rel_max, relerr(b[k], a[k]))
    return bad, noise_max, rel_max


def _twin_step(dev, model, bucket, window, calls, epoch, opt=None):
    _pin(dev, calls, epoch)
    bucket.begin()
    loss, risk = harness.train_window(model, *window, ACC)
    bucket.finish()
    if opt is not None:
        opt.step()
    return _snapshot(model, bucket, loss, risk, opt)


def _capture(dev, kind, dtype, window, fusion="concat", extra=None, rows=ROWS, **kw):
    """A captured training-mode step pinned at (SEED, BASE) -> (step, model, bucket, the captured body's reservations)."""
    model, _ = _build(dev, kind, dtype, fusion)
    bucket = FlatGradBucket(list(model.parameters()))
    if "opt" in kw:
        kw["opt"] = kw["opt"](bucket)
    _pin(dev, BASE, None)
    with S.recording() as records:
        step = harness.GraphedWindowStep(model, bucket, window, ACC, warmup=1, **{"opt": None, **kw})
    assert len(records) % 2 == 0                                           # one warm-up body, then the captured one
    captured = records[len(records) // 2:]
    assert captured[0][1] == step.rng_base and [s for s, _ in records[:len(captured)]] == [s for s, _ in captured]
    S.match_sites(captured, kind, rows, B, N, D, extra)
    assert not S.ranges_overlap(captured), captured
    assert step.epoch is ops._rng_epoch_tensor and int(step.epoch) == 0
    return step, model, bucket, captured


def _check_replays_against_twin(dev, kind, dtype, fusion="concat", extra=None):
    tag = f"{kind} {DTYPE_IDS[DTYPES.index(dtype)]} {fusion}"
    window = harness.make_window(_slides(), dev, dtype)
    step, model, bucket, captured = _capture(dev, kind, dtype, window, fusion, extra)
    twin, _ = _build(dev, kind, dtype, fusion)
    twin_bucket = FlatGradBucket(list(twin.parameters()))
    twin_window = harness.make_window(_slides(), dev, dtype)
    epochs = (1, 2, 3)
    replays = {}
    for e in epochs:
        step.epoch.fill_(e - 1)                                  # the body starts with the bump: this replay runs at epoch e
        loss, risk = step()
        replays[e] = _snapshot(model, bucket, loss, risk)
        assert int(step.epoch) == e
    twins = {e: [_twin_step(dev, twin, twin_bucket, twin_window, step.rng_base, e) for _ in range(2)] for e in (*epochs, 4)}
    for e in epochs:
        a, a_again = twins[e]
        bad, noise, rel = _misses(a, a_again, replays[e])
        wrong, _, rel_wrong = _misses(*twins[e + 1], replays[e])
        print(f"[captured vs twin] {tag} epoch {e}: eager to eager max |diff| {noise:.1e}; replay against twin max rel {rel:.1e}, "
              f"{len(bad)} of {len(a)} tensors miss; against the twin of epoch {e + 1}: max rel {rel_wrong:.1e} = "
              f"{rel_wrong / ATOMIC_TOL:.0f} x {ATOMIC_TOL:.0e}, {len(wrong)} tensors miss")
        assert not bad, (tag, e, bad[:8])
        assert len(wrong) > len(a) // 2 and rel_wrong > 100 * ATOMIC_TOL, (tag, e, len(wrong), rel_wrong)
    return step


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_captured_replay_equals_the_eager_step_at_its_epoch(dev, kind, dtype):
    with _generator_restored():
        _check_replays_against_twin(dev, kind, dtype)


def test_captured_bilinear_step_equals_the_eager_step_at_its_epoch(dev):
    """fusion="bilinear": five further dropout sites inside the captured body, one more reservation."""
    with _generator_restored():
        assert F.bilinear_span(B, D) == int(L.lib().mpo_bilinear_head_rng_span(B, D))
        _check_replays_against_twin(dev, "mcat", torch.float32, "bilinear", extra=_head_sites("bilinear"))


def test_captured_adam_step_equals_eager_twin_steps(dev):
    """Adam inside the graph: four replays (epochs and step counts 1..4, fresh masks each) against four eager steps of a twin at
    those epochs -- parameters, both moments, the last gradients."""
    with _generator_restored():
        window = harness.make_window(_slides(), dev, torch.bfloat16)

        def adam(bucket):
            return FlatAdam(bucket, lr=1e-3, weight_decay=1e-5)
        step, model, bucket, _ = _capture(dev, "mcat", torch.bfloat16, window, opt=adam)
        assert int(step.opt.t_dev) == 0                          # warm-up and priming trained nothing
        before = step.opt.flat_p.clone()
        for _ in range(4):
            loss, risk = step()
        got = _snapshot(model, bucket, loss, risk, step.opt)
        assert int(step.opt.t_dev) == 4 and int(step.epoch) == 4
        runs = []
        for _ in range(2):
            twin, _ = _build(dev, "mcat", torch.bfloat16)
            twin_bucket = FlatGradBucket(list(twin.parameters()))
            opt = adam(twin_bucket)
            for e in (1, 2, 3, 4):
                snap = _twin_step(dev, twin, twin_bucket, window, step.rng_base, e, opt)
            assert int(opt.t_dev) == 4
            runs.append(snap)
        bad, noise, rel = _misses(runs[0], runs[1], got)
        print(f"[captured Adam] four steps: eager to eager max |diff| {noise:.1e}; graph against twin max rel {rel:.1e}, "
              f"{len(bad)} tensors miss")
        assert not bad, bad[:8]
        assert float(got["exp_avg_sq"].max()) > 0 and not torch.equal(got["flat_p"], before)      # it did train


@pytest.mark.parametrize("kind", KINDS)
def test_split_step_fills_the_same_bucket_in_training_mode(dev, kind):
    """test_gpu_graph.py::test_split_step_fills_the_same_bucket with every dropout site on: main graph + replay_tail() at an
    epoch leave the one-graph step's bucket of that epoch, bit for bit; the main graph alone leaves the head slice alone."""
    with _generator_restored():
        def build(split):
            window = harness.make_window(_slides(), dev, torch.bfloat16)
            return _capture(dev, kind, torch.bfloat16, window, split_patch_grad=split, rng_base=BASE)
        one, _, bucket_a, streams_a = build(False)
        two, model_b, bucket_b, streams_b = build(True)
        assert streams_a == streams_b                                      # (same seed, same offsets; each sets its epoch below)
        one.epoch.fill_(4)
        loss_a = one()[0].clone()
        ref = bucket_a.flat.clone()
        one.epoch.fill_(5)
        one()
        assert not torch.equal(bucket_a.flat, ref)                         # (the masks are live: another epoch, other gradients)
        head = two.head_numel()
        assert head == model_b.H[0].weight.numel()
        bucket_b.flat[:head].fill_(123.0)
        two.epoch.fill_(4)
        loss_b = two()[0].clone()                                          # main graph only
        assert torch.equal(bucket_b.flat[:head], torch.full_like(bucket_b.flat[:head], 123.0))
        torch.testing.assert_close(bucket_b.flat[head:], ref[head:], rtol=0, atol=0)
        torch.testing.assert_close(loss_b, loss_a, rtol=0, atol=0)
        two.replay_tail()
        torch.testing.assert_close(bucket_b.flat, ref, rtol=0, atol=0)
        assert not ops._deferred_patch


def test_captured_sampled_step_equals_the_eager_step_on_its_sample(dev):
    """sample_rows=32 with dropout on: the replay against the eager train_window on the rows the replay drew
    (step.sampler.out), the counter at the offset the body reserved right after the sampler's own."""
    with _generator_restored():
        k = 32
        slides = syn.make_cohort(6, 200, 700, SIZES, 56)[:B]
        window = harness.make_window(slides, dev, torch.bfloat16)
        step, model, bucket, captured = _capture(dev, "mcat", torch.bfloat16, window, extra={"sampler": 0}, rows=B * k,
                                                 sample_rows=k)
        assert captured[0] == (0, step.rng_base)                            # the sampler's counter leads the body
        after_sampler = captured[1][1]
        twin, _ = _build(dev, "mcat", torch.bfloat16)
        twin_bucket = FlatGradBucket(list(twin.parameters()))
        samples = []
        for e in (1, 2, 3):
            step.epoch.fill_(e - 1)
            loss, risk = step()
            got = _snapshot(model, bucket, loss, risk)
            sample = step.sampler.out.clone()
            samples.append(sample)
            on_sample = (BagBatch.from_lengths(sample, [k] * B), *window[1:])
            a, a_again = (_twin_step(dev, twin, twin_bucket, on_sample, after_sampler, e) for _ in range(2))
            bad, noise, rel = _misses(a, a_again, got)
            wrong, _, rel_wrong = _misses(*(_twin_step(dev, twin, twin_bucket, on_sample, after_sampler, e + 1) for _ in range(2)), got)
            print(f"[captured sampled step] epoch {e}: eager to eager max |diff| {noise:.1e}; replay against twin max rel {rel:.1e}, "
                  f"{len(bad)} tensors miss; twin at epoch {e + 1}: max rel {rel_wrong:.1e}, {len(wrong)} tensors miss")
            assert not bad, (e, bad[:8])
            assert len(wrong) > len(a) // 2 and rel_wrong > 100 * ATOMIC_TOL
        assert not torch.equal(samples[0], samples[1]) and not torch.equal(samples[1], samples[2])   # fresh rows per replay
