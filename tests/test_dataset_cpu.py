"""The datasets from the reference's files (multimodal_path_omic_amd/dataset.py) and the front of main.run
(multimodal_path_omic_amd/main.py), on the host: parity with what the reference's MultimodalDataset /
MultimodalGeneExprPredDataset and pandas.qcut gave on tests/golden/dataset/ (recorded by tests/golden/make_dataset_golden.py),
the two documented deviations, the host-memory behaviour of slides(), the refusals, build_model, the imports.

Bars.  Ids, classes, sizes, censorship, months: equal.  class_intervals: equal as fp64 (the same numpy call on the same
operand).  Omics: within ONE fp32 ulp of the recorded value -- derived, not measured: the fp64 mean / std here may differ from
pandas' by a few fp64 ulps (summation order), which can move the float32 cast by at most one step, and only at a rounding
tie.  Nothing here launches a kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multimodal_path_omic_amd import dataset as D
from multimodal_path_omic_amd import fit, harness, main
from multimodal_path_omic_amd.models import (GeneExprNarrowContextualAttentionGateTransformer,
                                             MultimodalCoAttentionTransformer, NarrowContextualAttentionGateTransformer)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset")
COHORT, SIGNATURES = os.path.join(GOLDEN, "cohort.csv"), os.path.join(GOLDEN, "signatures.csv")
N_SLIDES = 23
CONFIGS = ["TFFFF", "FTFTF", "TTFFT", "FFTFF"]          # standardize, normalize, decider_only, tcga_only, diagnostic_only

with open(os.path.join(GOLDEN, "expected.json")) as _f:
    EXPECTED = json.load(_f)
with open(os.path.join(GOLDEN, "qcut_cases.json")) as _f:
    QCUT_CASES = json.load(_f)["cases"]


def has_file(i):
    return i % 7 != 3


def patch_tensor(i):
    return torch.randn(5 + i, 8, generator=torch.Generator().manual_seed(1000 + i))


@pytest.fixture(scope="module")
def patches_dir(tmp_path_factory):
    """The fixture's patch files: slide i has one unless i % 7 == 3, a (5 + i, 8) fp32 tensor."""
    d = tmp_path_factory.mktemp("patches")
    for i in range(N_SLIDES):
        if has_file(i):
            torch.save(patch_tensor(i), d / f"S{i:02d}.pt")
    return str(d)


def config_of(key, patches_dir, **over):
    flags = [c == "T" for c in key]
    section = dict(zip(("standardize", "normalize", "decider_only", "tcga_only", "diagnostic_only"), flags))
    section.update(file=COHORT, patches_dir=patches_dir, signatures=SIGNATURES, name="SYN")
    section.update(over)
    return {"dataset": section}


def slide_number(slide_id):
    return int(slide_id[1:3])


def ulps32(got: torch.Tensor, want: torch.Tensor) -> int:
    """The largest distance in fp32 steps (both finite, the same shape)."""
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all())

    def ordinal(t):
        bits = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(bits < 0, -(bits & 0x7FFFFFFF), bits)
    return int((ordinal(got) - ordinal(want)).abs().max())


def recorded_f32(rows):
    return torch.tensor([[float(v) for v in row] for row in rows], dtype=torch.float64).to(torch.float32)


# ------------------------------------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("key", CONFIGS)
def test_survival_dataset_is_the_reference(key, patches_dir):
    want = EXPECTED["configs"][key]
    ds = D.SurvivalDataset(COHORT, config_of(key, patches_dir))
    assert ds.slide_ids == want["slide_ids"] and ds.patients == want["patients"] and len(ds) == len(want["slide_ids"])
    assert all(has_file(slide_number(s)) for s in ds.slide_ids)
    assert ds.survival_class.dtype == np.int64 and ds.survival_class.tolist() == want["survival_class"]
    assert ds.survival_months.dtype == np.float64 and ds.survival_months.tolist() == want["survival_months"]
    assert ds.censorship.dtype == np.int64 and ds.censorship.tolist() == want["censorship"]
    assert ds.class_intervals.dtype == np.float64 and ds.class_intervals.tolist() == want["class_intervals"]
    assert ds.signatures == want["signatures"] == ["SIG_A", "SIG_B", "SIG_C"]
    assert ds.signature_sizes == want["signature_sizes"] == [3, 2, 1]
    worst = 0
    for name, got in zip(ds.signatures, ds.omics):
        rec = recorded_f32(want["omics"][name])
        assert got.dtype == torch.float32 and got.shape == (len(ds), rec.shape[1])
        worst = max(worst, ulps32(got, rec))
    print(f"[dataset {key}] {len(ds)} slides, largest omic difference from the reference: {worst} fp32 ulp")
    assert worst <= 1


@pytest.mark.parametrize("key", CONFIGS)
def test_getitem_is_the_reference_tuple(key, patches_dir):
    want = EXPECTED["configs"][key]
    ds = D.SurvivalDataset(COHORT, config_of(key, patches_dir))
    for i, rec in enumerate(want["getitem"]):
        months, cls, cens, omics, patches = ds[i]
        assert (float(months), int(cls), int(cens)) == (rec["survival_months"], rec["survival_class"], rec["censorship"])
        assert len(omics) == 3 and [tuple(o.shape) for o in omics] == [(3,), (2,), (1,)]
        for o, r in zip(omics, rec["omics"]):
            assert ulps32(o, recorded_f32([r])[0]) <= 1
        file = patch_tensor(slide_number(ds.slide_ids[i]))
        assert list(patches.shape) == rec["patches_shape"] and torch.equal(patches, file)


def test_a_leading_one_is_squeezed(tmp_path):
    for i in range(N_SLIDES):
        torch.save(patch_tensor(i).unsqueeze(0), tmp_path / f"S{i:02d}.pt")
    ds = D.SurvivalDataset(COHORT, config_of("FFFFF", str(tmp_path)))
    assert len(ds) == N_SLIDES and ds[4][4].shape == (9, 8) and ds.slides()[4]["wsi"].shape == (9, 8) and ds.patch_dim == 8


def test_without_the_file_filter_every_row_stays(patches_dir):
    ds = D.SurvivalDataset(COHORT, config_of("FFFFF", patches_dir), remove_incomplete_samples=False)
    assert len(ds) == N_SLIDES and ds.slide_ids == [f"S{i:02d}.svs" for i in range(N_SLIDES)]


@pytest.mark.parametrize("key", ["F", "T"])
def test_gene_expression_dataset_is_the_reference(key, patches_dir):
    want = EXPECTED["gene_expression"][key]
    ds = D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": patches_dir, "decider_only": key == "T"}}, want["gene"])
    assert ds.slide_ids == want["slide_ids"] and ds.patients == want["patients"]
    assert ds.gene_expr_class.dtype == np.int64 and ds.gene_expr_class.tolist() == want["gene_expr_class"]
    assert ds.class_intervals.dtype == np.float64 and ds.class_intervals.tolist() == want["class_intervals"]
    label, patches = ds[2]
    assert int(label) == want["gene_expr_class"][2] and torch.equal(patches, patch_tensor(slide_number(ds.slide_ids[2])))


# ------------------------------------------------------------------------------------------------ qcut
@pytest.mark.parametrize("n_case", range(len(QCUT_CASES)))
def test_qcut_is_the_recorded_pandas_qcut(n_case):
    case = QCUT_CASES[n_case]
    if case["raises"]:
        with pytest.raises(ValueError, match="Bin edges must be unique"):
            D.qcut(case["values"], case["q"])
        return
    labels, edges = D.qcut(case["values"], case["q"])
    assert labels.dtype == np.int64 and edges.dtype == np.float64 and edges.shape == (case["q"] + 1,)
    assert edges.tolist() == case["edges"] and labels.tolist() == case["labels"]


def test_the_recorded_qcut_cases_cover_the_hazard():
    shapes = {(len(c["values"]), c["q"]) for c in QCUT_CASES}
    assert shapes >= {(n, q) for q in (3, 4) for n in (4, 5, 7, 10, 13, 16, 22)}
    assert sum(c["raises"] for c in QCUT_CASES) == 2 and len(QCUT_CASES) >= 40
    assert any((len(c["values"]) - 1) % c["q"] == 0 and c["q"] == 3 for c in QCUT_CASES)
    assert any(len(set(c["values"])) < len(c["values"]) and not c["raises"] for c in QCUT_CASES)


def test_qcut_against_pandas_live():
    pd = pytest.importorskip("pandas")
    gen = np.random.Generator(np.random.PCG64(5))
    compared = 0
    for case in range(300):
        n, q = int(gen.integers(4, 41)), (3, 4)[case % 2]
        values = (gen.standard_normal(n) * 10.0, gen.integers(0, 3 * n, n) * 0.1, np.round(gen.random(n) * 50, 1))[case % 3]
        try:
            want_labels, want_edges = pd.qcut(values, q=q, retbins=True, labels=False)
        except ValueError:
            with pytest.raises(ValueError, match="Bin edges must be unique"):
                D.qcut(values, q)
            continue
        labels, edges = D.qcut(values, q)
        assert edges.tobytes() == np.asarray(want_edges, dtype=np.float64).tobytes(), (case, values.tolist(), q)
        assert labels.tolist() == [int(x) for x in want_labels], (case, values.tolist(), q)
        compared += 1
    assert compared >= 200


def test_qcut_refuses_what_it_cannot_label():
    with pytest.raises(ValueError, match="not finite"):
        D.qcut([1.0, float("nan"), 2.0, 3.0], 3)
    with pytest.raises(ValueError, match="0 values"):
        D.qcut([], 4)


# ------------------------------------------------------------------------------------------------ the two deviations, pinned
def test_omics_follow_the_slide(patches_dir):
    ds = D.SurvivalDataset(COHORT, config_of("TFFFF", patches_dir))
    whole = {s: [o[i].clone() for o in ds.omics] for i, s in enumerate(ds.slide_ids)}
    split = ds.split(0.6, leave_one_out="P04", seed=3)
    for ids in split:
        assert ids and ids != list(range(len(ids)))              # no part is the dataset's first rows: the reference's defect would show
        for g in range(3):
            rows = ds.omics[g][ids]
            assert torch.equal(rows, torch.stack([whole[ds.slide_ids[i]][g] for i in ids]))
        for i in ids:                                            # and through the dicts a cohort is built from
            assert all(torch.equal(a, b) for a, b in zip(ds.slides()[i]["omics"], whole[ds.slide_ids[i]]))


def test_gene_expression_labels_follow_the_slide(patches_dir):
    ds = D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": patches_dir}}, "CCNE1")
    whole = dict(zip(ds.slide_ids, ds.gene_expr_class.tolist()))
    split = ds.split(0.6, leave_one_out="P04", seed=3)
    slides = ds.slides()
    for ids in split:
        assert ids and ids != list(range(len(ids)))
        assert [slides[i]["gene_expr_class"] for i in ids] == [whole[ds.slide_ids[i]] for i in ids]
        assert ds.gene_expr_class[ids].tolist() == [whole[ds.slide_ids[i]] for i in ids]
    # the values decide the class, slide by slide, whatever order the parts come in
    for i in range(len(ds)):
        v = ds.gene_expr_value[i]
        assert ds.class_intervals[ds.gene_expr_class[i]] <= v <= ds.class_intervals[ds.gene_expr_class[i] + 1]


def test_split_is_split_patients(patches_dir):
    for ds in (D.SurvivalDataset(COHORT, config_of("FFFFF", patches_dir)),
               D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": patches_dir}}, "MYC")):
        assert ds.split(0.8, seed=5) == fit.split_patients(ds.patients, 0.8, seed=5)
        order = list(dict.fromkeys(ds.patients))[::-1]
        assert ds.split(0.5, permutation=order) == fit.split_patients(ds.patients, 0.5, permutation=order)
        s = ds.split(0.8, leave_one_out="P07", seed=5)
        assert s == fit.split_patients(ds.patients, 0.8, leave_one_out="P07", seed=5)
        assert s.test == [i for i, p in enumerate(ds.patients) if p == "P07"] and len(s.test) == 2
        assert {ds.slide_ids[i] for i in s.test} == {"S14.svs", "S15.svs"}
        with pytest.raises(ValueError, match="leave_one_out patient 'P99'"):
            ds.split(0.8, leave_one_out="P99")


# ------------------------------------------------------------------------------------------------ host memory
def is_mapped(t: torch.Tensor, path: str) -> bool:
    """Backed by the file's mapping, not by host memory of its own: the tensor's first byte lies inside a mapping of `path`
    in the process's list of mappings.  No row is in memory until it is touched."""
    with open("/proc/self/maps") as f:
        for line in f:
            fields = line.split(None, 5)
            if len(fields) == 6 and fields[5].strip() == os.path.realpath(path):
                lo, hi = (int(x, 16) for x in fields[0].split("-"))
                if lo <= t.data_ptr() < hi:
                    return True
    return False


def test_slides_are_memory_mapped_and_a_cpu_cohort_holds_their_rows(patches_dir):
    ds = D.SurvivalDataset(COHORT, config_of("TFFFF", patches_dir))
    slides = ds.slides()
    assert [set(s) for s in slides] == [{"wsi", "omics", "survival_months", "survival_class", "censorship"}] * len(ds)
    for i, s in enumerate(slides):
        assert is_mapped(s["wsi"], ds.patch_path(i))
    assert not is_mapped(torch.load(ds.patch_path(0), weights_only=True), ds.patch_path(0))      # a plain load is a copy
    # slabs of three rows' bytes at the least: several slabs, every slide whole
    cohort = ds.cohort("cpu", bag_dtype=torch.bfloat16, slab_bytes=40 * 8 * 2)
    assert isinstance(cohort, harness.ResidentCohort) and len(cohort.slabs) > 3 and cohort.n_slides == len(ds)
    assert cohort.lengths == [5 + slide_number(s) for s in ds.slide_ids]
    for i, s in enumerate(ds.slide_ids):
        assert cohort.rows[i].dtype == torch.bfloat16 and torch.equal(cohort.rows[i], patch_tensor(slide_number(s)).to(torch.bfloat16))
    assert all(torch.equal(a, b) for a, b in zip(cohort.omics, ds.omics))
    assert cohort.labels.tolist() == ds.survival_class.tolist() and cohort.labels.dtype == torch.int64
    assert cohort.censorship.tolist() == [float(c) for c in ds.censorship]
    assert cohort.survival_months.dtype == torch.float64 and cohort.survival_months.tolist() == ds.survival_months.tolist()
    one = ds.cohort("cpu", bag_dtype=torch.float32)
    assert len(one.slabs) == 1 and all(torch.equal(r, patch_tensor(slide_number(s))) for r, s in zip(one.rows, ds.slide_ids))


def test_gene_expression_slides_are_memory_mapped_and_a_cpu_cohort_holds_their_rows(patches_dir):
    ds = D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": patches_dir, "decider_only": True}}, "CCNE1")
    slides = ds.slides()
    assert [set(s) for s in slides] == [{"wsi", "gene_expr_class"}] * len(ds)
    assert all(is_mapped(s["wsi"], ds.patch_path(i)) for i, s in enumerate(slides))
    cohort = ds.cohort("cpu", bag_dtype=torch.bfloat16, slab_bytes=40 * 8 * 2)
    assert isinstance(cohort, harness.GeResidentCohort) and len(cohort.slabs) > 2
    assert cohort.lengths == [5 + slide_number(s) for s in ds.slide_ids]
    for i, s in enumerate(ds.slide_ids):
        assert torch.equal(cohort.rows[i], patch_tensor(slide_number(s)).to(torch.bfloat16))
    assert cohort.labels.tolist() == ds.gene_expr_class.tolist()


# ------------------------------------------------------------------------------------------------ refusals
def write_csv(path, header, rows):
    with open(path, "w") as f:
        f.write(",".join(header) + "\n")
        for r in rows:
            f.write(",".join(str(c) for c in r) + "\n")
    return str(path)


def small_files(tmp_path, constant=None, n=8):
    """A cohort of n slides with genes A, B, C (column `constant` the same in every row), its patch files, signatures."""
    rows = [[f"P{i // 2}", f"T{i}.svs", 1.0, "diagnostic_slide", 10.5 + 3 * i, i % 2] +
            [2.0 if g == constant else 1.0 + 0.25 * ((i * (k + 3)) % 7) for k, g in enumerate("ABC")] for i in range(n)]
    cohort = write_csv(tmp_path / "cohort.csv", ["patient", "slide_id", "is_decider", "source", "survival_months", "censorship",
                                                 "A_rnaseq", "B_rnaseq", "C_rnaseq"], rows)
    for i in range(n):
        torch.save(torch.zeros(3, 8), tmp_path / f"T{i}.pt")
    return cohort


def small_config(tmp_path, cohort, signatures, **over):
    section = {"file": cohort, "patches_dir": str(tmp_path), "signatures": signatures, "decider_only": False, "tcga_only": False,
               "diagnostic_only": False, "standardize": False, "normalize": False}
    section.update(over)
    return {"dataset": section}


def test_a_signature_without_a_matching_gene_is_refused(tmp_path):
    cohort = small_files(tmp_path)
    sigs = write_csv(tmp_path / "sigs.csv", ["GOOD", "EMPTY_ONE"], [["A", "X"], ["B", "Y"]])
    with pytest.raises(ValueError, match="signature 'EMPTY_ONE'"):
        D.SurvivalDataset(cohort, small_config(tmp_path, cohort, sigs))


def test_a_constant_column_is_refused_only_where_a_signature_uses_it(tmp_path):
    cohort = small_files(tmp_path, constant="B")
    uses = write_csv(tmp_path / "uses.csv", ["S1", "S2"], [["A", "B"], ["C", ""]])
    skips = write_csv(tmp_path / "skips.csv", ["S1", "S2"], [["A", "C"], ["C", ""]])
    for over in (dict(standardize=True), dict(normalize=True), dict(standardize=True, normalize=True)):
        with pytest.raises(ValueError, match="column 'B_rnaseq'"):
            D.SurvivalDataset(cohort, small_config(tmp_path, cohort, uses, **over))
        ds = D.SurvivalDataset(cohort, small_config(tmp_path, cohort, skips, **over))       # B is not checked: nobody reads it
        assert ds.signature_sizes == [2, 1] and all(bool(torch.isfinite(o).all()) for o in ds.omics)
    ds = D.SurvivalDataset(cohort, small_config(tmp_path, cohort, uses))                     # unscaled, a constant is a value
    assert ds.omics[1][:, 0].tolist() == [2.0] * 8


def test_a_single_row_is_refused_by_qcut_before_the_scaling(tmp_path):
    """One row under `standardize` has no ddof-1 deviation; it never gets that far: its four quantile edges coincide, here as
    in the reference."""
    cohort = small_files(tmp_path)
    sigs = write_csv(tmp_path / "sigs.csv", ["S1"], [["A"]])
    for i in range(1, 8):
        os.remove(tmp_path / f"T{i}.pt")
    with pytest.raises(ValueError, match="Bin edges must be unique"):                         # qcut of one row comes first
        D.SurvivalDataset(cohort, small_config(tmp_path, cohort, sigs, standardize=True))


def test_h5_dataset_is_refused(tmp_path, patches_dir):
    with pytest.raises(ValueError, match="h5py"):
        D.SurvivalDataset(COHORT, config_of("TFFFF", patches_dir, h5_dataset="/data/cohort.h5"))
    with pytest.raises(ValueError, match="h5py"):
        D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": patches_dir, "h5_dataset": "/data/cohort.h5"}}, "CCNE1")
    assert len(D.SurvivalDataset(COHORT, config_of("TFFFF", patches_dir, h5_dataset=None))) == 20      # null: the .pt layout


def test_a_missing_gene_column_is_refused(patches_dir):
    with pytest.raises(ValueError, match="gene 'NOGENE' has no column 'NOGENE_rnaseq'"):
        D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": patches_dir}}, "NOGENE")


def test_filters_that_leave_no_row_are_refused(tmp_path, patches_dir):
    with pytest.raises(ValueError, match="no row of .*cohort.csv is left after decider_only, tcga_only"):
        D.SurvivalDataset(COHORT, config_of("FFTTF", patches_dir))                # is_decider == 1.0 and then == 0.0
    with pytest.raises(ValueError, match="no row of .*cohort.csv is left after the files under"):
        D.SurvivalDataset(COHORT, config_of("FFFFF", str(tmp_path)))              # a directory without a single file
    with pytest.raises(ValueError, match="no row of .*cohort.csv is left after the files under"):
        D.GeneExprDataset(COHORT, {"dataset": {"patches_dir": str(tmp_path)}}, "CCNE1")


def test_required_keys(patches_dir):
    config = config_of("TFFFF", patches_dir)
    for key in ("patches_dir", "signatures"):
        broken = {"dataset": {k: v for k, v in config["dataset"].items() if k != key}}
        with pytest.raises(KeyError, match=key):
            D.SurvivalDataset(COHORT, broken)
    bare = {"dataset": {"patches_dir": patches_dir, "signatures": SIGNATURES}}          # every flag missing: read as false
    assert D.SurvivalDataset(COHORT, bare).slide_ids == D.SurvivalDataset(COHORT, config_of("FFFFF", patches_dir)).slide_ids


def run_config(patches_dir, kind="mcat", **over):
    c = config_of("TFFFF", patches_dir)
    c["model"] = {"name": "M", "load_from_checkpoint": None, "checkpoint_epoch": 0, "checkpoint_dir": None, "fusion": "concat",
                  "model_size": "medium", "gene": "CCNE1"}
    c["training"] = {"leave_one_out": None, "output_attn_epoch": 20, "test_output_dir": None, "train_size": 0.8,
                     "loss": "ce" if kind == "ge_nacagat" else "ces", "epochs": 1, "optimizer": "adam", "lr": 1e-3,
                     "weight_decay": 1e-5, "grad_acc_step": 4, "scheduler": None, "alpha": 0.75, "lambda": 0.0, "gamma": 1.0}
    c.update(over)
    return c


def test_run_refuses_before_any_file_is_opened(tmp_path):
    nowhere = run_config(str(tmp_path / "missing"))
    nowhere["dataset"]["file"] = str(tmp_path / "missing.csv")                     # nothing here exists: no file is reached
    with pytest.raises(ValueError, match="device 'cpu' is a CPU"):
        main.run(nowhere, "mcat", sample_rows=4, device="cpu")
    with pytest.raises(ValueError, match="device 'cpu' is a CPU"):
        main.run(nowhere, "ge_nacagat", sample_rows=4, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="model_kind 'porpoise' is not one of mcat | nacagat | ge_nacagat".replace("|", r"\|")):
        main.run(nowhere, "porpoise", sample_rows=4)
    with pytest.raises(ValueError, match="sample_rows is missing"):
        main.run(nowhere, "nacagat", device="cuda")
    with pytest.raises(ValueError, match="model_kind 'porpoise'"):
        main.build_model(nowhere, None, "porpoise")


def test_run_reads_a_config_path(tmp_path):
    yaml = pytest.importorskip("yaml")
    config = run_config(str(tmp_path))
    path = tmp_path / "config.yaml"
    with open(path, "w") as f:
        yaml.safe_dump(config, f)
    assert main.load_config(str(path)) == config and main.load_config(path) == config and main.load_config(config) is config
    for given in (config, str(path)):
        with pytest.raises(ValueError, match="device 'cpu' is a CPU"):
            main.run(given, "mcat", sample_rows=4, device="cpu")


# ------------------------------------------------------------------------------------------------ build_model
@pytest.fixture(scope="module")
def wide_patches_dir(tmp_path_factory):
    """The fixture's cohort with files of a width the patch layer is built for: (2, 512)."""
    d = tmp_path_factory.mktemp("wide")
    for i in range(N_SLIDES):
        if has_file(i):
            torch.save(torch.zeros(2, 512), d / f"S{i:02d}.pt")
    return str(d)


def shapes_of(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("kind", ["mcat", "nacagat", "ge_nacagat"])
@pytest.mark.parametrize("size,fusion", [("small", "concat"), ("medium", "bilinear")])
def test_build_model_is_the_hand_built_model(kind, size, fusion, wide_patches_dir):
    config = run_config(wide_patches_dir, kind)
    config["model"].update(model_size=size, fusion=fusion)
    ds = main.build_dataset(config, kind)
    model = main.build_model(config, ds, kind, torch.bfloat16)
    if kind == "ge_nacagat":
        assert isinstance(ds, D.GeneExprDataset) and ds.gene == "CCNE1"
        hand = GeneExprNarrowContextualAttentionGateTransformer(model_size=size, bag_dtype=torch.bfloat16, patch_dim=512)
    else:
        cls = MultimodalCoAttentionTransformer if kind == "mcat" else NarrowContextualAttentionGateTransformer
        assert isinstance(ds, D.SurvivalDataset) and ds.signature_sizes == [3, 2, 1]
        hand = cls(omic_sizes=[3, 2, 1], model_size=size, fusion=fusion, bag_dtype=torch.bfloat16, patch_dim=512)
    assert type(model) is type(hand) and shapes_of(model) == shapes_of(hand)
    assert model.patch_dim == 512 and model.bag_dtype == torch.bfloat16
    assert [tuple(p.shape) for p in model.parameters()] == [tuple(p.shape) for p in hand.parameters()]
    other = dict(config, model=dict(config["model"], model_size="big" if size == "small" else "small"))
    assert shapes_of(main.build_model(other, ds, kind)) != shapes_of(model)                  # the size is read
    if kind != "ge_nacagat":
        other = dict(config, model=dict(config["model"], fusion="concat" if fusion == "bilinear" else "bilinear"))
        assert shapes_of(main.build_model(other, ds, kind)) != shapes_of(model)              # and the fusion


def test_build_model_refuses_a_width_the_patch_layer_is_not_built_for(patches_dir):
    config = run_config(patches_dir)
    with pytest.raises(ValueError, match="patch_dim 8"):
        main.build_model(config, main.build_dataset(config, "mcat"), "mcat")


# ------------------------------------------------------------------------------------------------ imports
def test_the_optional_libraries_are_not_imported():
    code = ("import sys; import multimodal_path_omic_amd.dataset, multimodal_path_omic_amd.main; "
            "print([m for m in ('pandas', 'scipy', 'h5py', 'yaml', 'wandb') if m in sys.modules])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[]"
