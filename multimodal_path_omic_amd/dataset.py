"""The reference's datasets, from the reference's files: the cohort CSV, the signatures CSV and the directory of per-slide
`.pt` files (dataset/dataset.py:12-114, dataset/ge_dataset.py:11-47), read with the stdlib csv module and numpy.

    qcut               pandas.qcut(values, q=q, retbins=True, labels=False), the call both reference datasets label with
    SurvivalDataset    MultimodalDataset(file, config, use_signatures=True): what all three main.py construct
    GeneExprDataset    MultimodalGeneExprPredDataset(file, config, gene)

A dataset holds one row per slide it kept, hands harness.ResidentCohort / GeResidentCohort their dicts (`slides()`, `cohort()`)
and splits by patient into slide ids of that ONE cohort (`split()`: fit.split_patients).  Host code: no kernel, no C entry; the
rows reach the device through harness._ResidentRows as every cohort's do.  pandas, scipy, h5py and yaml are the reference's
dependencies and are not imported here.

Numbers are parsed with Python's float(), which rounds correctly; pandas' default C parser does not always, so a cell of
more than 15 significant digits may differ from the reference's value in its last bit.  An empty cell reads as NaN.

Two deviations from the reference, both defects there that one cohort indexed by slide id does not have:

1. MultimodalDataset.from_dataframe (dataset/dataset.py:234-241) indexes the parent's signature tensors with the RESET index
   of the split frame: the train / val / test datasets carry the parent's first len(split) rows of omics, not their own
   slides'.  Here `split` returns ids into the one dataset, so a slide keeps its own omics.
2. MultimodalGeneExprPredDataset.from_dataframe (dataset/ge_dataset.py:114) hands every split the parent's whole label array,
   so split slide j is labelled as the parent's slide j.  Here a slide keeps its own label.
"""
from __future__ import annotations

import csv
import os
from typing import List, Sequence

import numpy as np
import torch

from . import fit, harness


# ------------------------------------------------------------------------------------ pandas.qcut
def qcut(values, q: int):
    """pandas.qcut(values, q=q, retbins=True, labels=False) -> (labels int64 (n,), edges fp64 (q + 1,)).

    The path pandas takes (core/reshape/tile.py qcut -> Series.quantile -> core/array_algos/quantile.py
    quantile_with_mask): edges = numpy.percentile(values, numpy.linspace(0, 1, q + 1) * 100.0, method='linear').  The
    quantiles go through `* 100.0` there and `/ 100` inside numpy, and that round trip, not linspace's own value, decides
    the virtual index (n - 1) * quantile: where (n - 1) * k / q is an integer the edge IS a sample, and one ulp in the
    index would hand that sample to the neighbouring class.  So the same numpy call is made here, on the same operand.
    Labels (tile.py _bins_to_cuts, right=True, include_lowest=True): edges.searchsorted(values, side='left') - 1, and a
    value equal to edges[0] is in bin 0: bins are right-closed and the lowest value is included.

    ValueError: repeated edges (pandas' "Bin edges must be unique", duplicates='raise'); an empty or non-finite input --
    pandas labels NaN as NaN, which no class tensor here can hold."""
    x = np.asarray(values, dtype=np.float64).reshape(-1)
    if x.size == 0 or not np.isfinite(x).all():
        raise ValueError(f"qcut: {x.size} values, {int((~np.isfinite(x)).sum())} of them not finite: every row needs a finite value")
    edges = np.asarray(np.percentile(x, np.linspace(0, 1, int(q) + 1) * 100.0, method="linear"), dtype=np.float64)
    if len(np.unique(edges)) < len(edges):
        raise ValueError(f"Bin edges must be unique: {edges.tolist()!r}")
    labels = edges.searchsorted(x, side="left").astype(np.int64)
    labels[x == edges[0]] = 1
    return labels - 1, edges


# ------------------------------------------------------------------------------------ the files
class _Table:
    """A CSV file as columns of strings, in file order (csv.reader: quoted cells and embedded commas as pandas reads them)."""

    def __init__(self, path: str):
        self.path = path
        with open(path, newline="") as f:
            rows = [r for r in csv.reader(f) if r]
        if not rows:
            raise ValueError(f"{path}: an empty CSV file")
        self.names = rows[0]
        width = len(self.names)
        for n, r in enumerate(rows[1:], 2):
            if len(r) != width:
                raise ValueError(f"{path}: line {n} has {len(r)} cells, the header names {width} columns")
        self.rows = rows[1:]
        self.index = {name: j for j, name in enumerate(self.names)}

    def __contains__(self, name: str) -> bool:
        return name in self.index

    def keep(self, mask: Sequence[bool]):
        self.rows = [r for r, m in zip(self.rows, mask) if m]

    def text(self, name: str) -> List[str]:
        if name not in self.index:
            raise ValueError(f"{self.path}: no column '{name}'")
        j = self.index[name]
        return [r[j] for r in self.rows]

    def numbers(self, name: str) -> np.ndarray:
        cells = self.text(name)
        try:
            return np.array([float(c) if c.strip() else float("nan") for c in cells], dtype=np.float64)
        except ValueError as e:
            raise ValueError(f"{self.path}: column '{name}' holds a cell that is no number ({e})") from None


def _flag(section: dict, key: str) -> bool:
    return bool(section.get(key))


def _patch_path(patches_dir: "str | None", slide_id: str) -> str:
    return os.path.join(patches_dir or "", slide_id.replace(".svs", ".pt"))


def _open_patches(path: str) -> torch.Tensor:
    """ingest.PtDirStore's rule: nothing from the file is executed, nothing is read until the rows are touched; the leading
    1 of a (1, M, width) file is squeezed."""
    t = torch.load(path, map_location="cpu", weights_only=True, mmap=True)
    if t.dim() == 3:
        t = t.squeeze(0)
    return t


class _SlideDataset:
    """What both datasets share: the table after its filters, the patch files, the patients and the split."""

    def _read(self, who: str, file: str, config: dict, filters, remove_incomplete_samples: bool):
        section = config["dataset"]
        self.file = file
        self.patches_dir = section["patches_dir"] or ""
        if section.get("h5_dataset") is not None:
            raise ValueError(f"{who}: dataset.h5_dataset = {section['h5_dataset']!r} asks for the HDF5 layout, which needs h5py; "
                             "h5py is absent here (ingest.py): store one .pt file per slide under dataset.patches_dir")
        table = _Table(file)
        applied = []
        for key, column, test in filters:
            if _flag(section, key):
                applied.append(key)
                if column == "is_decider":
                    table.keep(table.numbers(column) == test)
                else:
                    table.keep([c == test for c in table.text(column)])
        if remove_incomplete_samples:
            applied.append(f"the files under {self.patches_dir or '.'!r}")
            table.keep([os.path.exists(_patch_path(self.patches_dir, s)) for s in table.text("slide_id")])
        if not table.rows:
            raise ValueError(f"{who}: no row of {file} is left after {', '.join(applied) or 'reading it'}")
        self.slide_ids = table.text("slide_id")
        self.patients = table.text("patient")
        return table

    def __len__(self) -> int:
        return len(self.slide_ids)

    def patch_path(self, i: int) -> str:
        return _patch_path(self.patches_dir, self.slide_ids[i])

    def patches(self, i: int) -> torch.Tensor:
        """Slide i's (M, width) features, memory-mapped."""
        return _open_patches(self.patch_path(i))

    @property
    def patch_dim(self) -> int:
        """The width of the first slide's file."""
        return int(self.patches(0).shape[-1])

    def split(self, train_size: float, leave_one_out=None, seed: int = 0, permutation=None) -> fit.Split:
        """fit.split_patients(self.patients, ...): slide ids into this dataset, and so into its cohort."""
        return fit.split_patients(self.patients, train_size, leave_one_out, seed, permutation)


class SurvivalDataset(_SlideDataset):
    """The reference's MultimodalDataset(file, config, use_signatures=True) (dataset/dataset.py:12-114); the
    use_signatures=False dict layout is not offered.  config: the whole YAML dict, of which config['dataset'] alone is read.

    Keys of config['dataset'].  Required (KeyError, as in the reference): `patches_dir` (None = the working directory) and
    `signatures`.  Read as false / null where missing (the reference raises KeyError on all but h5_dataset; a config that
    runs there reads the same here): `decider_only`, `tcga_only`, `diagnostic_only`, `standardize`, `normalize`,
    `h5_dataset`.  Columns of the CSV: `slide_id`, `patient`, `survival_months`, `censorship`, the `*_rnaseq` columns the
    signatures name, and `is_decider` / `source` where a filter that reads them is set.

    In the reference's order:
      1. filters, each only if set: decider_only (is_decider == 1.0), then tcga_only (is_decider == 0.0), then
         diagnostic_only (source == 'diagnostic_slide');
      2. with remove_incomplete_samples, a row stays iff os.path.join(patches_dir or '', slide_id.replace('.svs', '.pt'))
         exists; CSV order is kept;
      3. survival_class, class_intervals = qcut(survival_months, 4) over the rows that remain;
      4. `standardize`: every *_rnaseq column becomes (x - mean) / std, std at ddof = 1 (pandas' Series.std); then `normalize`:
         2 (x - min) / (max - min) - 1; both over the remaining rows, in fp64;
      5. the `signatures` CSV: one column per signature in file order, blanks dropped; a signature's group is the columns
         g + '_rnaseq' of its genes g, in its row order, that the cohort CSV has, cast to float32: omics[i] is (N, d_i),
         signature_sizes = [d_i].

    Public: slide_ids, patients, survival_months (fp64), censorship (int64 where every cell is an integer, as pandas infers,
    else fp64), survival_class (int64), class_intervals (fp64, 5 values) -- numpy arrays; signatures (names),
    signature_sizes, omics (list of (N, d_i) float32 tensors); len(), [i], slides(), cohort(), split(), patch_dim.

    ValueError: h5_dataset set (h5py is absent); no row left; repeated qcut edges; a signature none of whose genes has a column
    (the reference fails later, with a shape error); a column a signature uses that is not finite after the scaling -- a
    constant column or an empty cell, on which the reference would train on NaN -- named in the message (a single row, which
    has no ddof-1 deviation either, is refused by qcut first, as in the reference).  Columns no signature uses are not checked."""

    def __init__(self, file: str, config: dict, *, remove_incomplete_samples: bool = True):
        section = config["dataset"]
        table = self._read("SurvivalDataset", file, config,
                           (("decider_only", "is_decider", 1.0), ("tcga_only", "is_decider", 0.0),
                            ("diagnostic_only", "source", "diagnostic_slide")), remove_incomplete_samples)
        self.survival_months = table.numbers("survival_months")
        cens = table.numbers("censorship")
        self.censorship = cens.astype(np.int64) if all(_is_int(c) for c in table.text("censorship")) else cens
        self.survival_class, self.class_intervals = qcut(self.survival_months, 4)

        standardize, normalize = _flag(section, "standardize"), _flag(section, "normalize")
        sig_table = _Table(section["signatures"])
        self.signatures = list(sig_table.names)
        self.signature_sizes, self.omics, scaled = [], [], {}
        for name in self.signatures:
            columns = [g + "_rnaseq" for g in dict.fromkeys(c for c in sig_table.text(name) if c.strip()) if g + "_rnaseq" in table]
            if not columns:
                raise ValueError(f"SurvivalDataset: signature '{name}' of {sig_table.path} names no gene with a *_rnaseq column "
                                 f"in {file}")
            for c in columns:
                if c not in scaled:
                    scaled[c] = _scale(table.numbers(c), standardize, normalize)
                    if not np.isfinite(scaled[c]).all():
                        steps = " and ".join(k for k, on in (("standardize", standardize), ("normalize", normalize)) if on)
                        raise ValueError(f"SurvivalDataset: column '{c}' (signature '{name}') is not finite after "
                                         f"{steps or 'parsing'} over {len(self)} rows: a constant column, a single row or a "
                                         "missing value")
            self.omics.append(torch.from_numpy(np.stack([scaled[c] for c in columns], axis=1).astype(np.float32)))
            self.signature_sizes.append(len(columns))

    def __getitem__(self, i: int):
        """The reference's tuple: (survival_months, survival_class, censorship, [omics_g[i]], patches)."""
        return (self.survival_months[i], self.survival_class[i], self.censorship[i], [o[i] for o in self.omics], self.patches(i))

    def slides(self) -> "List[dict]":
        """The dicts harness.ResidentCohort takes.  Each `wsi` is the memory-mapped file: no row is read until
        harness._ResidentRows concatenates a slab, and then one slab's rows (slab_bytes of the bag dtype; twice that in
        fp32 for a bf16 cohort) are in host memory at a time, never the cohort's."""
        return [{"wsi": self.patches(i), "omics": [o[i] for o in self.omics], "survival_months": float(self.survival_months[i]),
                 "survival_class": int(self.survival_class[i]), "censorship": self.censorship[i].item()} for i in range(len(self))]

    def cohort(self, device, bag_dtype=torch.bfloat16, cycle: bool = False, slab_bytes: int = 1 << 30) -> harness.ResidentCohort:
        return harness.ResidentCohort(self.slides(), device, bag_dtype=bag_dtype, cycle=cycle, slab_bytes=slab_bytes)


class GeneExprDataset(_SlideDataset):
    """The reference's MultimodalGeneExprPredDataset(file, config, gene) (dataset/ge_dataset.py:11-47): the decider_only filter
    alone, the existing-file filter always, gene_expr_class, class_intervals = qcut(data[gene + '_rnaseq'], 3), no scaling.
    config['dataset']: `patches_dir` required; `decider_only` and `h5_dataset` read as false / null where missing.

    Public: slide_ids, patients, gene, gene_expr_value (fp64), gene_expr_class (int64), class_intervals (fp64, 4 values); len(),
    [i] -> (gene_expr_class, patches), slides() ({'wsi', 'gene_expr_class'}), cohort() (a harness.GeResidentCohort), split(),
    patch_dim.  ValueError: no column gene + '_rnaseq'; h5_dataset set; no row left; repeated or non-finite qcut input."""

    def __init__(self, file: str, config: dict, gene: str):
        table = self._read("GeneExprDataset", file, config, (("decider_only", "is_decider", 1.0),), True)
        self.gene = str(gene)
        column = f"{self.gene}_rnaseq"
        if column not in table:
            raise ValueError(f"GeneExprDataset: gene '{self.gene}' has no column '{column}' in {file}")
        self.gene_expr_value = table.numbers(column)
        self.gene_expr_class, self.class_intervals = qcut(self.gene_expr_value, 3)

    def __getitem__(self, i: int):
        return self.gene_expr_class[i], self.patches(i)

    def slides(self) -> "List[dict]":
        """The dicts harness.GeResidentCohort takes; `wsi` memory-mapped, as SurvivalDataset.slides says."""
        return [{"wsi": self.patches(i), "gene_expr_class": int(self.gene_expr_class[i])} for i in range(len(self))]

    def cohort(self, device, bag_dtype=torch.bfloat16, cycle: bool = False, slab_bytes: int = 1 << 30) -> harness.GeResidentCohort:
        return harness.GeResidentCohort(self.slides(), device, bag_dtype=bag_dtype, cycle=cycle, slab_bytes=slab_bytes)


def _is_int(cell: str) -> bool:
    try:
        int(cell)
    except ValueError:
        return False
    return True


def _scale(x: np.ndarray, standardize: bool, normalize: bool) -> np.ndarray:
    """dataset/dataset.py:74-81 on one column, in fp64.  mean and std as pandas' nanops takes them: sum / n, and
    sqrt(sum((mean - x)^2) / (n - 1)).  A constant column or a single row gives NaN or infinity, as there."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if standardize:
            mean = x.sum() / x.size
            std = np.sqrt(((mean - x) ** 2).sum() / np.float64(x.size - 1))
            x = (x - mean) / std
        if normalize:
            x = 2 * (x - x.min()) / (x.max() - x.min()) - 1
    return x
