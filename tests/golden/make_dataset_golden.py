#!/usr/bin/env python3
"""Generate tests/golden/dataset/ by running THE REFERENCE'S dataset classes (dataset/dataset.py, dataset/ge_dataset.py,
imported from the read-only checkout at REF, first argument or /root/reference) and pandas.qcut on a small synthetic cohort:

    cohort.csv        23 slides of 12 patients (two slides each, the last patient one)
    signatures.csv    three signatures of 3 / 2 / 1 matching genes; one name has no column; ragged columns
    expected.json     per configuration what MultimodalDataset(file, config, use_signatures=True) holds and yields,
                      and for one gene what MultimodalGeneExprPredDataset holds
    qcut_cases.json   (values, q, labels, edges) from pandas.qcut(values, q=q, retbins=True, labels=False)

Which patch files exist is part of the fixture: slide i has one unless i % 7 == 3 (has_file below; the tests restate it).
The files this script writes for the reference to find go to a temporary directory and are not kept.

Both reference files import h5py at the top, which is absent here and unused on the .pt path: an empty module of that name
is put into sys.modules first.  No test runs this script; it needs pandas and scipy, which the package does not."""
import json
import os
import sys
import tempfile
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "dataset")
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

N_SLIDES = 23
GENES = ["CCNE1", "BRCA1", "TP53", "MYC", "KRAS", "PTEN", "RB1"]            # the seven *_rnaseq columns
SIGNATURES = {"SIG_A": ["CCNE1", "NOGENE", "TP53", "MYC"],                  # NOGENE has no column: 3 genes
              "SIG_B": ["KRAS", "BRCA1"],                                      # 2 genes, not in the CSV's column order
              "SIG_C": ["TP53"]}                                               # 1 gene, shared with SIG_A; RB1, PTEN: unused
CONFIGS = [(True, False, False, False, False), (False, True, False, True, False), (True, True, False, False, True),
           (False, False, True, False, False)]          # (standardize, normalize, decider_only, tcga_only, diagnostic_only)
GE_GENE = "CCNE1"


def has_file(i: int) -> bool:
    return i % 7 != 3


def six_digits(x: float) -> float:
    """At most 6 significant digits: every CSV reader agrees on the fp64 value."""
    return float(f"{x:.6g}")


def write_cohort(path):
    gen = np.random.Generator(np.random.PCG64(2024))
    header = ["patient", "slide_id", "is_decider", "source", "survival_months", "censorship"] + \
        [g + "_rnaseq" for g in GENES] + ["CCNE1_cnv", "TP53_mut"]
    months = [six_digits(float(np.exp(3.0 + 0.9 * gen.standard_normal()))) for _ in range(N_SLIDES)]
    months[12] = months[5]                                                     # two rows share a survival_months
    lines = [",".join(header)]
    for i in range(N_SLIDES):
        row = [f"P{i // 2:02d}", f"S{i:02d}.svs", "1.0" if (i // 2) % 2 == 0 else "0.0",
               "diagnostic_slide" if i % 4 != 1 else "frozen_slide", repr(months[i]), str(int(gen.random() < 0.4))]
        row += [repr(six_digits(float(5.0 + 2.5 * gen.standard_normal()))) for _ in GENES]
        row += [str(int(gen.integers(-2, 3))), str(int(gen.random() < 0.3))]
        lines.append(",".join(row))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_signatures(path):
    depth = max(len(v) for v in SIGNATURES.values())
    lines = [",".join(SIGNATURES)]
    for r in range(depth):
        lines.append(",".join(v[r] if r < len(v) else "" for v in SIGNATURES.values()))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_patches(patches_dir):
    """Slide i's file: (5 + i, 8) fp32 from a generator seeded by i (the tests write the same)."""
    for i in range(N_SLIDES):
        if has_file(i):
            g = torch.Generator().manual_seed(1000 + i)
            torch.save(torch.randn(5 + i, 8, generator=g), os.path.join(patches_dir, f"S{i:02d}.pt"))


def f32_reprs(t):
    return [[repr(float(v)) for v in row] for row in t.tolist()]


def record_survival(ref_dataset, config):
    import pandas as pd
    ds = ref_dataset.MultimodalDataset(config["dataset"]["file"], config, use_signatures=True)
    # the reference prints the intervals and keeps the classes alone: the same call again, over the rows it kept
    edges = [float(x) for x in pd.qcut(ds.data["survival_months"], q=4, retbins=True, labels=False)[1]]
    items = []
    for i in range(len(ds)):
        months, cls, cens, omics, patches = ds[i]
        items.append({"survival_months": float(months), "survival_class": int(cls), "censorship": int(cens),
                      "omics": [[repr(float(v)) for v in o.tolist()] for o in omics], "patches_shape": list(patches.shape)})
    return {"slide_ids": [str(s) for s in ds.data["slide_id"]],
            "patients": [str(p) for p in ds.data["patient"]],
            "survival_months": [float(x) for x in ds.survival_months],
            "censorship": [int(x) for x in ds.censorship],
            "survival_class": [int(x) for x in ds.survival_class],
            "class_intervals": edges,
            "signatures": [str(s) for s in ds.signatures],
            "signature_sizes": [int(s) for s in ds.signature_sizes],
            "omics": {str(s): f32_reprs(ds.signature_data[s]) for s in ds.signatures},
            "getitem": items}


def record_ge(ref_ge, config, gene):
    import pandas as pd
    ds = ref_ge.MultimodalGeneExprPredDataset(config["dataset"]["file"], config, gene)
    edges = pd.qcut(ds.gene_expr_value, q=3, retbins=True, labels=False)[1]
    return {"gene": gene, "slide_ids": [str(s) for s in ds.data["slide_id"]], "patients": [str(p) for p in ds.data["patient"]],
            "gene_expr_class": [int(x) for x in ds.gene_expr_class], "class_intervals": [float(x) for x in edges]}


def qcut_cases():
    import pandas as pd
    gen = np.random.Generator(np.random.PCG64(77))
    cases = []

    def record(values, q):
        values = [float(v) for v in values]
        try:
            labels, edges = pd.qcut(np.array(values), q=q, retbins=True, labels=False)
        except ValueError:
            cases.append({"values": values, "q": q, "raises": True})
            return False
        cases.append({"values": values, "q": q, "raises": False, "labels": [int(x) for x in labels],
                      "edges": [float(x) for x in edges]})
        return True

    for q in (3, 4):
        for n in (4, 5, 7, 10, 13, 16, 22):
            record(gen.standard_normal(n) * 10.0, q)                          # distinct reals
            record(gen.permutation(n) * 0.1 + 0.3, q)                         # an edge IS a sample where (n - 1) % q == 0
            if n >= 7:                                                         # a tie away from the edges
                while True:
                    v = np.sort(gen.standard_normal(n))
                    j = int(gen.integers(1, n - 1))
                    v[j] = v[j - 1]
                    before = len(cases)
                    if record(gen.permutation(v), q):
                        break
                    del cases[before:]
    assert record([2.5] * 5, 4) is False                                       # repeated edges: pandas raises
    assert record([1.0, 1.0, 1.0, 1.0, 2.0, 3.0, 4.0], 4) is False
    return cases


def main():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, os.path.join(REF, "dataset"))
    import dataset as ref_dataset
    import ge_dataset as ref_ge
    import pandas as pd

    os.makedirs(OUT, exist_ok=True)
    cohort, signatures = os.path.join(OUT, "cohort.csv"), os.path.join(OUT, "signatures.csv")
    write_cohort(cohort)
    write_signatures(signatures)
    expected = {"pandas": pd.__version__, "configs": {}, "gene_expression": {}}
    with tempfile.TemporaryDirectory() as patches_dir:
        write_patches(patches_dir)
        for standardize, normalize, decider_only, tcga_only, diagnostic_only in CONFIGS:
            config = {"dataset": {"file": cohort, "patches_dir": patches_dir, "signatures": signatures,
                                  "decider_only": decider_only, "tcga_only": tcga_only, "diagnostic_only": diagnostic_only,
                                  "standardize": standardize, "normalize": normalize}}
            key = "".join("T" if b else "F" for b in (standardize, normalize, decider_only, tcga_only, diagnostic_only))
            expected["configs"][key] = record_survival(ref_dataset, config)
        for decider_only in (False, True):
            config = {"dataset": {"file": cohort, "patches_dir": patches_dir, "decider_only": decider_only}}
            expected["gene_expression"]["T" if decider_only else "F"] = record_ge(ref_ge, config, GE_GENE)
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
        f.write("\n")
    with open(os.path.join(OUT, "qcut_cases.json"), "w") as f:
        json.dump({"pandas": pd.__version__, "numpy": np.__version__, "cases": qcut_cases()}, f)
        f.write("\n")
    print(f"wrote {OUT}: {sorted(os.listdir(OUT))}")


if __name__ == "__main__":
    main()
