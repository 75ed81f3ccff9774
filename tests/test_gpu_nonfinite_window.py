"""One corrupt slide in a window of four (lengths 33, 300, 129, 77; slide 1 holds a NaN, a +Inf or a -Inf in one patch
feature) through the models and the harness.

  * forward_window in eval mode and harness.train_window against the fp64 oracle, slide by slide, on bf16, fp32 and fp16
    windows (the gene-expression model on bf16 and fp32): where the oracle's hazards / survs / Y / loss / risk are non-finite ours
    are (element by element), the co-attention map per query row; the three clean slides are finite and within the bars of
    tests/test_gpu_train_step.py, and on a bf16 window -- no cross-slide state -- bit-equal to the window without the plant;
    every parameter whose oracle gradient holds a non-finite element has one here.  The plant: a patch feature, or an omic value.  An fp32 window's feature scale falls back to 1.0 when anything is non-finite:
    bars there, no bit comparison; the features are N(0, 1).
  * one eager step under FlatOptimizer(skip_nonfinite=True): the corrupt slide's loss and risk are non-finite, the step is
    skipped (skipped_steps + 1, t_dev unchanged, every parameter and optimiser state keeps its bits), and the next, clean
    window steps normally.  MCAT with `ces`, NaCAGaT with `cesar`, on bf16, fp32 and fp16 windows; the gene-expression model
    with its `ce` head on bf16 and fp32.
  * the same once through GraphedWindowStep (the plant written in place into the window the graph reads).
  * CohortEvaluator, eager and captured, over a resident cohort with the corrupt slide: its loss and risk are non-finite, every
    other slide's figures equal the clean cohort's within test_gpu_validate.BAR."""
import pytest
import torch

import cases as C
import nonfinite_cases as N
import tail_helpers as H
import test_gpu_fp16_window as F16
import test_gpu_ge_train as GE
import test_gpu_train_step as STEP
import test_gpu_validate as V
from multimodal_path_omic_amd import harness, ops
from multimodal_path_omic_amd import synthetic as syn
from multimodal_path_omic_amd.dp import FlatGradBucket, FlatOptimizer
from multimodal_path_omic_amd.models import MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer
from oracle import mpo_oracle as O

pytestmark = pytest.mark.gpu
LENGTHS = [33, 300, 129, 77]
CORRUPT, ROW, COL = 1, 299, 100                 # slide 1, its last row
SIZES = [64] * 6
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}


@pytest.fixture(autouse=True)
def _rng_put_back():
    calls = ops._rng_calls
    ops.set_rng_epoch(None)
    yield
    ops.set_rng_epoch(None)
    ops._rng_calls = calls


def _slides(plant=None):
    g = syn.rng(9400)
    slides = []
    for i, m in enumerate(LENGTHS):
        wsi = syn.normal(g, (m, 1024))
        if plant is not None and i == CORRUPT:
            wsi[ROW, COL] = N.PLANTS[plant]
        slides.append(dict(wsi=wsi, omics=[syn.normal(g, (s,)) for s in SIZES], survival_class=i % 4, censorship=i % 2,
                           survival_months=10.0 + 7 * i, gene_expr_class=i % 2))
    return slides


def _model(dev, kind, dtype, seed=55):
    cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
    model = cls(omic_sizes=SIZES, bag_dtype=dtype)
    sd = syn.fill_state_dict(C.model_shapes(SIZES, kind == "nacagat"), seed)
    model.load_state_dict(sd)
    return model.to(dev), sd


def _oracle_kw(dtype):
    """The oracle on the values the window stores: bf16 at X, W_H and H_bag; fp16 at X alone (tests/test_gpu_fp16_window.py)."""
    return {} if dtype == torch.float32 else (dict(F16.X_ONLY) if dtype == torch.float16 else dict(bag_storage=dtype))


def _bars(dtype):
    """tests/test_gpu_train_step.py::_bars; an fp16 window is held to the fp32 row (tests/test_gpu_fp16_window.py)."""
    return STEP._bars(torch.bfloat16 if dtype == torch.bfloat16 else torch.float32)


def _oracle_window(kind, sd, slides, dtype, loss_kind=None):
    """The fp64 model slide by slide -> hazards, survs, Y (B, 4), the co-attention maps, and with loss_kind ('ces' | 'cesar') the
    per-slide loss and risk and the gradients of sum(loss) / B, as harness.train_window accumulates them."""
    p = {k: v.double().requires_grad_(loss_kind is not None) for k, v in sd.items()}
    fwd = O.mcat_forward if kind == "mcat" else O.nacagat_forward
    kw = dict(inference=True) if kind == "mcat" else {}
    rows, maps, losses, total = [], [], [], 0.0
    with torch.set_grad_enabled(loss_kind is not None):
        for s in slides:
            hz, sv, y, att = fwd(p, s["wsi"], s["omics"], **_oracle_kw(dtype), **kw)
            rows.append((hz[0].detach(), sv[0].detach(), y[0].detach()))
            maps.append(att["coattn"].detach())
            if loss_kind:
                lab, cen = torch.tensor([s["survival_class"]]), torch.tensor([float(s["censorship"])])
                loss = O.ces_loss(hz, sv, lab, cen) if loss_kind == "ces" else O.cesar_loss(hz, sv, lab, cen, att["coattn"])[0]
                losses.append(loss.reshape(()).detach())
                total = total + loss.reshape(()) / len(slides)
        out = dict(zip(("hazards", "survs", "Y"), (torch.stack([r[k] for r in rows]) for k in range(3))), maps=maps)
        if loss_kind:
            total.backward()
            out.update(loss=torch.stack(losses), risk=-out["survs"].sum(1),
                       grads={n: (t.grad if t.grad is not None else torch.zeros_like(t)) for n, t in p.items()})
    return out


def _plant_omic(slides, plant):
    slides[CORRUPT]["omics"][2][5] = N.PLANTS[plant]
    return slides


@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("where", ["patch", "omic"])
@pytest.mark.parametrize("store", list(DTYPES))
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_forward_window_keeps_the_corrupt_slide_non_finite_and_the_others_clean(dev, kind, store, where, plant):
    """Rules 1-3 on hazards, survs, Y (element by element) and on the co-attention map (per query row of the slide); the plant
    in a patch feature or in one omic value of slide 1."""
    dtype = DTYPES[store]
    model, sd = _model(dev, kind, dtype)
    model.eval()
    bad = _slides(plant) if where == "patch" else _plant_omic(_slides(), plant)
    with torch.no_grad():
        clean = model.forward_window(*harness.make_window(_slides(), dev, dtype)[:2], inference=True)
        got = model.forward_window(*harness.make_window(bad, dev, dtype)[:2], inference=True)
    ref, bars = _oracle_window(kind, sd, bad, dtype), _bars(dtype)
    assert not bool(torch.isfinite(ref["hazards"][CORRUPT]).any()), "the oracle's hazards of the corrupt slide"
    for k, name in enumerate(("hazards", "survs", "Y")):
        r, g = ref[name], got[k].double().cpu()
        swallowed = ~torch.isfinite(r) & torch.isfinite(g)
        assert not bool(swallowed.any()), (name, g.tolist(), r.tolist())
        for i in range(len(LENGTHS)):
            if not bool(torch.isfinite(r[i]).all()):
                continue
            assert bool(torch.isfinite(g[i]).all()), (name, i)
            assert float((g[i] - r[i]).abs().max()) < bars["hazards"], (name, i, float((g[i] - r[i]).abs().max()))
            if dtype == torch.bfloat16 and i != CORRUPT:
                assert torch.equal(got[k][i], clean[k][i]), (name, i)
    for i, (a, a_o) in enumerate(zip(got[3]["coattn"], ref["maps"])):
        a = a.double().cpu()
        swallowed = ~torch.isfinite(a_o).all(1) & torch.isfinite(a).all(1)
        assert not bool(swallowed.any()), ("map", i, swallowed.nonzero().flatten().tolist())
        if i != CORRUPT:
            assert bool(torch.isfinite(a_o).all()) and bool(torch.isfinite(a).all()), ("map", i)
            if dtype == torch.bfloat16:
                assert torch.equal(got[3]["coattn"][i], clean[3]["coattn"][i]), ("map", i)


@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("store", list(DTYPES))
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_train_window_against_the_oracle_slide_by_slide(dev, kind, store, plant):
    """harness.train_window (`ces`; `cesar` for NaCAGaT) in eval mode -- no masks to replay -- against the fp64 step.  The clean
    window first: loss, risk and every parameter gradient at the bars of tests/test_gpu_train_step.py.  Then with the corrupt
    slide: where the oracle's loss or risk is non-finite ours is; the clean slides' loss and risk are finite and within the
    bars; every parameter whose oracle gradient holds a non-finite element has one here (tensor level)."""
    dtype = DTYPES[store]
    model, sd = _model(dev, kind, dtype)
    model.eval()
    loss_kind = "ces" if kind == "mcat" else "cesar"
    bars, others = _bars(dtype), [i for i in range(len(LENGTHS)) if i != CORRUPT]

    def run(slides):
        for q in model.parameters():
            q.grad = None
        loss, risk = harness.train_window(model, *harness.make_window(slides, dev, dtype), len(LENGTHS), loss=loss_kind)
        ops.flush_patch_weight_grads()
        grads = {n: (q.grad.double().cpu() if q.grad is not None else torch.zeros_like(q).double().cpu()) for n, q in model.named_parameters()}
        return loss.double().cpu(), risk.double().cpu(), grads

    loss, risk, grads = run(_slides())
    ref = _oracle_window(kind, sd, _slides(), dtype, loss_kind)
    assert H.relerr(loss, ref["loss"]) < bars["loss"] and float((risk - ref["risk"]).abs().max()) < bars["risk"]
    for n, e in zip(grads, H.grad_errs([grads[n] for n in grads], [ref["grads"][n] for n in grads])):
        assert e < bars[STEP._grad_class(n)], (n, e)
    loss, risk, grads = run(_slides(plant))
    ref = _oracle_window(kind, sd, _slides(plant), dtype, loss_kind)
    for name, g, r in (("loss", loss, ref["loss"]), ("risk", risk, ref["risk"])):
        assert not bool((~torch.isfinite(r) & torch.isfinite(g)).any()), (name, g.tolist(), r.tolist())
        assert not bool(torch.isfinite(r[CORRUPT])) and bool(torch.isfinite(r[others]).all()), (name, r.tolist())
        assert bool(torch.isfinite(g[others]).all()), (name, g.tolist())
    assert H.relerr(loss[others], ref["loss"][others]) < bars["loss"], H.relerr(loss[others], ref["loss"][others])
    assert float((risk[others] - ref["risk"][others]).abs().max()) < bars["risk"]
    poisoned = [n for n, r in ref["grads"].items() if not bool(torch.isfinite(r).all())]
    assert poisoned, "the oracle's gradients do not see the corrupt slide"
    for n in poisoned:
        assert not bool(torch.isfinite(grads[n]).all()), (n, "finite where the oracle's gradient holds a non-finite element")


@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("store", ["bf16", "fp32"])
def test_gene_expression_window_against_the_oracle_bag_by_bag(dev, store, plant):
    """The gene-expression model: forward_window in eval mode (Y element by element; the clean bags at the bars of
    tests/test_gpu_ge_train.py / test_gpu_bag_selfattn.py) and train_ge_window (per-bag `ce` loss; parameter gradients at tensor
    level) against O.ge_nacagat_forward / O.ge_ce_loss in fp64."""
    dtype = DTYPES[store]
    model, sd = GE.build_ge(dev, 57, dtype)
    others = [i for i in range(len(LENGTHS)) if i != CORRUPT]
    y_bar = GE.GOLDEN_ABS if dtype == torch.float32 else GE.BF16_SAME_STORAGE_ABS
    slides = _slides(plant)
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ys, losses, total = [], [], 0.0
    for s in slides:
        y, _ = O.ge_nacagat_forward(p, s["wsi"], bag_storage=None if dtype == torch.float32 else dtype)
        loss = O.ge_ce_loss(y, torch.tensor(s["gene_expr_class"]))
        ys.append(y.detach())
        losses.append(loss.reshape(()).detach())
        total = total + loss.reshape(()) / len(slides)
    total.backward()
    y_o, loss_o = torch.stack(ys), torch.stack(losses)
    assert not bool(torch.isfinite(y_o[CORRUPT]).any()) and bool(torch.isfinite(y_o[others]).all())
    bags, labels = harness.make_ge_window(slides, dev, dtype)
    with torch.no_grad():
        y = model.forward_window(bags)[0].double().cpu()
    assert not bool((~torch.isfinite(y_o) & torch.isfinite(y)).any()), y.tolist()
    assert bool(torch.isfinite(y[others]).all()) and float((y[others] - y_o[others]).abs().max()) < y_bar
    loss = harness.train_ge_window(model, bags, labels, len(LENGTHS)).double().cpu()
    assert not bool(torch.isfinite(loss[CORRUPT])) and bool(torch.isfinite(loss[others]).all()), loss.tolist()
    assert float((loss[others] - loss_o[others]).abs().max()) < y_bar
    poisoned = [n for n, t in p.items() if t.grad is not None and not bool(torch.isfinite(t.grad).all())]
    assert poisoned
    got = dict(model.named_parameters())
    for n in poisoned:
        assert got[n].grad is not None and not bool(torch.isfinite(got[n].grad).all()), n


def _assert_skipped_then_steps(opt, run_bad, run_clean):
    """One clean step, one on the corrupt window (skipped, no trace), one clean step again."""
    run_clean()
    assert int(opt.skipped_steps) == 0 and int(opt.t_dev) == 1
    before = [t.clone() for t in (opt.flat_p, *opt._moments(), opt.t_dev)]
    loss, risk = run_bad()
    for t, k in zip((opt.flat_p, *opt._moments(), opt.t_dev), before):
        assert torch.equal(t, k)
    assert int(opt.skipped_steps) == 1 and int(opt.t_dev) == 1
    clean = [i for i in range(len(LENGTHS)) if i != CORRUPT]
    assert not bool(torch.isfinite(loss[CORRUPT])), loss.tolist()
    assert bool(torch.isfinite(loss[clean]).all()), loss.tolist()
    if risk is not None:
        assert not bool(torch.isfinite(risk[CORRUPT])) and bool(torch.isfinite(risk[clean]).all()), risk.tolist()
    run_clean()
    assert int(opt.skipped_steps) == 1 and int(opt.t_dev) == 2
    assert bool(torch.isfinite(opt.flat_p).all()) and not torch.equal(opt.flat_p, before[0])


@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("store", list(DTYPES))
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_eager_guarded_step_skips_the_corrupt_window(dev, kind, store, plant):
    dtype = DTYPES[store]
    model, _ = _model(dev, kind, dtype)
    model.train()
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "adam", lr=1e-3, skip_nonfinite=True)
    good, bad = harness.make_window(_slides(), dev, dtype), harness.make_window(_slides(plant), dev, dtype)
    loss_kind = "ces" if kind == "mcat" else "cesar"

    def run(window):
        bucket.begin()
        out = harness.train_window(model, *window, len(LENGTHS), loss=loss_kind)
        bucket.finish()
        opt.step()
        return out

    _assert_skipped_then_steps(opt, lambda: run(bad), lambda: run(good))


@pytest.mark.parametrize("plant", list(N.PLANTS))
@pytest.mark.parametrize("store", ["bf16", "fp32"])
def test_eager_guarded_step_of_the_gene_expression_model(dev, store, plant):
    dtype = DTYPES[store]
    model, _ = GE.build_ge(dev, 57, dtype)
    model.train()
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "adam", lr=1e-3, skip_nonfinite=True)
    good, bad = harness.make_ge_window(_slides(), dev, dtype), harness.make_ge_window(_slides(plant), dev, dtype)

    def run(window):
        bucket.begin()
        loss = harness.train_ge_window(model, *window, len(LENGTHS))
        bucket.finish()
        opt.step()
        return loss, None

    _assert_skipped_then_steps(opt, lambda: run(bad), lambda: run(good))


@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_captured_guarded_step_skips_the_corrupt_window(dev, kind):
    """tests/test_gpu_grad_guard.py plants a NaN in an omic vector; here it is a patch feature of slide 1's last row, written
    in place into the bf16 window the graph reads."""
    model, _ = _model(dev, kind, torch.bfloat16)
    model.eval()
    window = harness.make_window(_slides(), dev, torch.bfloat16)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "adam", lr=1e-3, skip_nonfinite=True)
    step = harness.GraphedWindowStep(model, bucket, window, len(LENGTHS), opt=opt)
    step()
    assert int(opt.skipped_steps) == 0 and int(opt.t_dev) == 1
    before = [t.clone() for t in (opt.flat_p, *opt._moments(), opt.t_dev)]
    data, at = window[0].data, sum(LENGTHS[:CORRUPT]) + ROW
    keep = data[at, COL].clone()
    for plant in N.PLANTS.values():
        data[at, COL] = plant
        step()
        for t, k in zip((opt.flat_p, *opt._moments(), opt.t_dev), before):
            assert torch.equal(t, k)
    assert int(opt.skipped_steps) == 3 and int(opt.t_dev) == 1
    data[at, COL] = keep
    step()
    assert int(opt.t_dev) == 2 and int(opt.skipped_steps) == 3 and bool(torch.isfinite(opt.flat_p).all())
    assert not torch.equal(opt.flat_p, before[0])


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["mcat", "nacagat"])
def test_cohort_evaluator_reports_the_corrupt_slide_and_only_it(dev, kind, storage, capture):
    dtype = V.DTYPE[storage]
    model, _ = _model(dev, kind, dtype)
    model.eval()
    ids = list(range(len(LENGTHS)))
    clean = harness.CohortEvaluator(model, harness.ResidentCohort(_slides(), dev, bag_dtype=dtype), ids, capture=capture)()
    others = [i for i in ids if i != CORRUPT]
    assert bool(torch.isfinite(clean.loss).all()) and bool(torch.isfinite(clean.risk).all())
    for plant in N.PLANTS:
        r = harness.CohortEvaluator(model, harness.ResidentCohort(_slides(plant), dev, bag_dtype=dtype), ids, capture=capture)()
        assert not bool(torch.isfinite(r.loss[CORRUPT])) and not bool(torch.isfinite(r.risk[CORRUPT])), (plant, r.loss.tolist(), r.risk.tolist())
        for name in ("loss", "risk", "hazards", "survs", "Y"):
            got, want = getattr(r, name)[others], getattr(clean, name)[others]
            assert bool(torch.isfinite(got).all()), (plant, name)
            assert float((got - want).abs().max()) < V.BAR[storage], (plant, name)
