"""A whole run from the reference's files (multimodal_path_omic_amd/main.py) on the device: main.run over a cohort CSV, a
signatures CSV and a directory of .pt files, against fit.fit over a cohort built by hand from the same dataset's dicts.

Measure of equality: tests/test_gpu_fit.py's `hold`, imported -- the comparison run is made twice from identical state
(test_gpu_fit.fresh()'s recipe); main.run must be bit-equal to it where those two are bit-equal and within twice their largest
difference otherwise.  No other tolerance.

Shapes: test_gpu_fit's -- 14 slides of 40-120 rows x 1024 of seven patients (synthetic.make_cohort(14, 40, 120, [64] * 6, 770)
/ make_ge_cohort(14, 40, 120, seed=771)), six signatures of 64 genes holding the synthetic omics, standardize and normalize
off, medium models, bf16 rows, a lapping cohort, sample_rows 32, windows of 4 slides, three epochs, one warm-up run.  The
dataset's survival_class (pandas.qcut's rule) generally differs from make_cohort's searchsorted classes; the hand-built cohort
comes from the dataset's own dicts, so both runs see the same labels."""
import os

import numpy as np
import pytest
import torch

import cases as C
from test_gpu_fit import final_tensors, fresh, hold
from multimodal_path_omic_amd import dataset as D
from multimodal_path_omic_amd import fit, harness, main, ops
from multimodal_path_omic_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SIZES = [64] * 6
ACC, K = 4, 32
SEED = 7                    # the split's and the epoch orders'
WEIGHTS = 61
STAMP = "S0"
KINDS = ("mcat", "nacagat", "ge_nacagat")
NAMES = {"mcat": "MCAT", "nacagat": "NaCAGaT", "ge_nacagat": "GeneExpr-NaCAGaT"}
PATIENTS = [f"P{i // 2}" for i in range(14)]
GENE = "CCNE1"


def write_csv(path, header, rows):
    with open(path, "w") as f:
        f.write(",".join(header) + "\n")
        for r in rows:
            f.write(",".join(r) + "\n")
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Both datasets on disk -> {'survival' | 'ge': (cohort csv, patches dir), 'signatures': csv, 'slides' | 'ge_slides'}."""
    root = tmp_path_factory.mktemp("reference_files")
    slides = syn.make_cohort(14, 40, 120, SIZES, 770)
    ge_slides = syn.make_ge_cohort(14, 40, 120, seed=771)
    out = {"slides": slides, "ge_slides": ge_slides}
    genes = [[f"G{g}N{j}" for j in range(d)] for g, d in enumerate(SIZES)]
    out["signatures"] = write_csv(root / "signatures.csv", [f"SIG{g}" for g in range(len(SIZES))],
                                  [[genes[g][j] for g in range(len(SIZES))] for j in range(SIZES[0])])
    for name, cohort in (("survival", slides), ("ge", ge_slides)):
        patches = root / name
        patches.mkdir()
        for i, s in enumerate(cohort):
            torch.save(s["wsi"], patches / f"S{i:02d}.pt")
        head = ["patient", "slide_id"]
        if name == "survival":
            # repr of the fp64 / of the fp32's fp64 value: float() reads the same number back, and the float32 cast is exact
            head += ["survival_months", "censorship"] + [g + "_rnaseq" for group in genes for g in group]
            rows = [[PATIENTS[i], f"S{i:02d}.svs", repr(s["survival_months"]), str(s["censorship"])] +
                    [repr(float(v)) for o in s["omics"] for v in o] for i, s in enumerate(cohort)]
        else:
            values = syn.rng(772).standard_normal(14)
            head += [f"{GENE}_rnaseq"]
            rows = [[PATIENTS[i], f"S{i:02d}.svs", repr(float(values[i]))] for i in range(14)]
        out[name] = (write_csv(root / f"{name}.csv", head, rows), str(patches))
    return out


def config(kind, files, epochs=3, out=None, **over):
    """The reference's config layout; `over` goes to `training:` unless it names a top-level key."""
    file, patches = files["ge" if kind == "ge_nacagat" else "survival"]
    c = {"device": "cuda", "wandb": {"enabled": False, "project": "P"},
         "dataset": {"name": "SYN-OV", "file": file, "patches_dir": patches, "signatures": files["signatures"],
                     "decider_only": False, "tcga_only": False, "diagnostic_only": False, "normalize": False, "standardize": False},
         "model": {"name": NAMES[kind], "load_from_checkpoint": None, "checkpoint_epoch": 0, "checkpoint_dir": None,
                   "fusion": "concat", "model_size": "medium", "gene": GENE},
         "training": {"leave_one_out": None, "output_attn_epoch": 20,
                      "test_output_dir": None if out is None else os.path.join(str(out), "outputs"), "train_size": 0.8,
                      "loss": "ce" if kind == "ge_nacagat" else "ces", "epochs": epochs, "optimizer": "adam", "lr": 1e-3,
                      "weight_decay": 1e-5, "grad_acc_step": ACC, "scheduler": None, "alpha": 0.75, "lambda": 0.0, "gamma": 1.0}}
    for key, value in over.items():
        if key in c:
            c[key] = value
        else:
            c["training"][key] = value
    return c


@pytest.fixture
def filled(monkeypatch):
    """Every model build_model builds gets synthetic.fill_state_dict's weights, applied after build_model -- inside main.run
    too, which looks the function up in its module."""
    real = main.build_model

    def build(cfg, dataset, kind, bag_dtype=torch.bfloat16):
        model = real(cfg, dataset, kind, bag_dtype)
        shapes = C.ge_model_shapes(d=256) if kind == "ge_nacagat" else C.model_shapes(SIZES, kind == "nacagat")
        model.load_state_dict(syn.fill_state_dict(shapes, WEIGHTS), strict=True)
        return model
    monkeypatch.setattr(main, "build_model", build)


@pytest.fixture
def generator():
    """The dropout generator as the test found it, afterwards; torch's host generator too, which every default
    initialisation inside build_model draws from."""
    keep, torch_keep = ops.rng_state(), torch.get_rng_state()
    yield
    ops.set_rng_epoch(None)
    ops.set_rng_state(keep)
    torch.set_rng_state(torch_keep)


def results(kind, res):
    return [res.history] + final_tensors(kind, res.final)


# ------------------------------------------------------------------------------------------------ 1. run is fit over the hand-built cohort
@pytest.mark.parametrize("kind", KINDS)
def test_run_is_fit_over_the_hand_built_cohort(dev, kind, files, filled, generator):
    cfg = config(kind, files)
    ds = main.build_dataset(cfg, kind)
    split = ds.split(0.8, None, SEED)
    assert split == fit.split_patients(PATIENTS, 0.8, seed=SEED) and (len(split.train), len(split.val)) == (10, 4)
    cls = harness.GeResidentCohort if kind == "ge_nacagat" else harness.ResidentCohort
    cohort = cls(ds.slides(), dev, cycle=True)
    runs = []
    for _ in range(2):
        fresh()
        model = main.build_model(cfg, ds, kind).to(dev)
        res = fit.fit(model, cohort, split.train, split.val, fit.fit_options(cfg, kind), sample_rows=K, seed=SEED, stamp=STAMP,
                      warmup=1)
        runs.append(results(kind, res))
    fresh()
    r = main.run(cfg, kind, sample_rows=K, device=dev, cycle=True, seed=SEED, stamp=STAMP, warmup=1)
    assert isinstance(r, main.RunResult) and r.split == split and r.fit.epochs_run == [0, 1, 2] and r.fit.leftover == 2
    assert type(r.dataset) is type(ds) and r.dataset.slide_ids == ds.slide_ids and type(r.cohort) is cls and r.cohort.cycle
    assert r.cohort.device == dev and next(r.model.parameters()).device == dev and r.model.bag_dtype == torch.bfloat16
    assert r.fit.history.shape == (3, 5) and bool(torch.isfinite(r.fit.history).all())
    hold(f"main.run {kind}", runs[0], runs[1], results(kind, r.fit))
    if kind != "ge_nacagat":
        assert ds.signature_sizes == SIZES and [tuple(o.shape) for o in ds.omics] == [(14, 64)] * 6


# ------------------------------------------------------------------------------------------------ 2. the cohort on the device
def test_the_cohort_on_the_device_holds_the_files(dev, files):
    cfg = config("mcat", files)
    ds = D.SurvivalDataset(cfg["dataset"]["file"], cfg)
    cohort = ds.cohort(dev)
    assert isinstance(cohort, harness.ResidentCohort) and cohort.n_slides == 14 and not cohort.cycle
    for i, s in enumerate(files["slides"]):
        assert cohort.rows[i].dtype == torch.bfloat16 and cohort.rows[i].device == dev
        assert torch.equal(cohort.rows[i].cpu(), s["wsi"].to(torch.bfloat16)), i
        for g in range(len(SIZES)):                                   # the CSV round trip is exact: the synthetic omics, bit for bit
            assert torch.equal(ds.omics[g][i], s["omics"][g])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(cohort.omics, ds.omics))
    assert cohort.labels.cpu().tolist() == ds.survival_class.tolist()
    assert cohort.censorship.cpu().tolist() == [float(c) for c in ds.censorship] == [float(s["censorship"]) for s in files["slides"]]
    assert cohort.survival_months.cpu().tolist() == ds.survival_months.tolist() == [s["survival_months"] for s in files["slides"]]
    edges = ds.class_intervals
    assert all(edges[c] <= m <= edges[c + 1] for c, m in zip(ds.survival_class, ds.survival_months))
    assert np.bincount(ds.survival_class, minlength=4).tolist() == [4, 3, 3, 4]


# ------------------------------------------------------------------------------------------------ 3. leave-one-out, W&B, log
@pytest.mark.parametrize("kind", ["nacagat"])
def test_leave_one_out_from_the_config(dev, kind, files, filled, generator, tmp_path):
    whole = fit.split_patients(PATIENTS, 0.8, seed=SEED)
    patient = PATIENTS[whole.train[0]]
    cfg = config(kind, files, out=tmp_path, leave_one_out=patient, output_attn_epoch=2, wandb={"enabled": True, "project": "P"})
    fresh()
    logged = []
    with pytest.warns(UserWarning, match="log="):
        r = main.run(cfg, kind, sample_rows=K, device=dev, cycle=True, seed=SEED, stamp=STAMP, warmup=1, log=logged.append)
    assert r.split == fit.split_patients(PATIENTS, 0.8, leave_one_out=patient, seed=SEED)
    assert [r.dataset.patients[i] for i in r.split.test] == [patient] * 2 and len(r.split.train) == 8 and r.split.val == whole.val
    names = [f"ATTN_{NAMES[kind]}_{patient}_{STAMP}_E2_{i}.pt" for i in r.split.test]
    assert sorted(os.listdir(tmp_path / "outputs")) == sorted(names)                  # epoch 2 only, one per test slide
    for name, i in zip(names, r.split.test):
        stored = torch.load(tmp_path / "outputs" / name, weights_only=True)
        assert stored.shape == (len(SIZES), r.cohort.lengths[i]) and bool(torch.isfinite(stored).all())
    assert logged == [{**row, "leftover": 0} for row in r.fit.table()]                # log: every epoch's row of the table


# ------------------------------------------------------------------------------------------------ 4. the command line
def test_the_command_line_prints_the_table(dev, files, generator, tmp_path, capsys):
    yaml = pytest.importorskip("yaml")
    path = tmp_path / "config.yaml"
    with open(path, "w") as f:
        yaml.safe_dump(config("ge_nacagat", files, epochs=2), f)
    fresh()
    main.main(["--model", "ge_nacagat", "--config", str(path), "--sample-rows", str(K), "--cycle", "--seed", str(SEED)])
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith("epoch ")]
    assert len(lines) == 2 and lines[0].startswith("epoch 0  lr 0.001  train_loss ") and "val_balanced_accuracy" in lines[1]
