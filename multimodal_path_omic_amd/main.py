"""The reference's main(config_path) for all three models (models/mcat/main.py:218-337, models/nacagat/main.py,
models/ge_nacagat/main.py:171-282), from the reference's files: the dataset (dataset.py), the model its config describes,
the patient split, the cohort on the device, and fit.Fit over them.

    build_model   config + dataset -> the model, as the reference's main() constructs it
    run           the whole main(); -> RunResult
    python -m multimodal_path_omic_amd.main --model nacagat --config path.yaml --sample-rows 4096

Host code over dataset, fit and harness: no kernel, no C entry.  yaml is imported only where `config` is a path; wandb is
never imported.  Data-parallel runs are not arranged here: Fit's group= / shard arguments pass through **fit_kwargs for a
caller who shards the ids themselves.
"""
from __future__ import annotations

import os
import warnings
from typing import Callable, NamedTuple

import torch

from . import dataset as datasets
from . import fit

MODEL_KINDS = ("mcat", "nacagat", "ge_nacagat")
BAG_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


class RunResult(NamedTuple):
    dataset: object                 # SurvivalDataset | GeneExprDataset
    split: fit.Split
    model: torch.nn.Module
    cohort: object                  # harness.ResidentCohort | harness.GeResidentCohort
    fit: fit.FitResult


def _check_kind(model_kind: str):
    if model_kind not in MODEL_KINDS:
        raise ValueError(f"model_kind {model_kind!r} is not one of {' | '.join(MODEL_KINDS)}")


def load_config(config) -> dict:
    """A dict as it is; a path through yaml.safe_load (imported here, so that a caller with a dict needs no yaml)."""
    if isinstance(config, dict):
        return config
    import yaml
    with open(os.fspath(config)) as f:
        return yaml.safe_load(f)


def build_dataset(config: dict, model_kind: str):
    """SurvivalDataset(dataset.file, config), or GeneExprDataset(dataset.file, config, model.gene) for 'ge_nacagat'."""
    _check_kind(model_kind)
    file = config["dataset"]["file"]
    if model_kind == "ge_nacagat":
        return datasets.GeneExprDataset(file, config, config["model"]["gene"])
    return datasets.SurvivalDataset(file, config)


def build_model(config: dict, dataset, model_kind: str, bag_dtype=torch.bfloat16) -> torch.nn.Module:
    """The model of config['model'] for `dataset`, on the CPU: model_size, fusion (the fusion models) and omic_sizes =
    dataset.signature_sizes, as the reference's main() passes them; patch_dim = the width of the first slide's file (the
    reference fixes 1024) -- a width outside ops.PATCH_DIMS is refused by the constructor."""
    from .models import (GeneExprNarrowContextualAttentionGateTransformer, MultimodalCoAttentionTransformer,
                         NarrowContextualAttentionGateTransformer)
    _check_kind(model_kind)
    size = config["model"]["model_size"]
    if model_kind == "ge_nacagat":
        return GeneExprNarrowContextualAttentionGateTransformer(model_size=size, bag_dtype=bag_dtype, patch_dim=dataset.patch_dim)
    cls = MultimodalCoAttentionTransformer if model_kind == "mcat" else NarrowContextualAttentionGateTransformer
    return cls(omic_sizes=list(dataset.signature_sizes), model_size=size, fusion=config["model"]["fusion"], bag_dtype=bag_dtype,
               patch_dim=dataset.patch_dim)


def run(config, model_kind: str, *, sample_rows: "int | None" = None, device="cuda", bag_dtype=torch.bfloat16,
        cycle: bool = False, seed: int = 0, permutation=None, log: "Callable | None" = None, **fit_kwargs) -> RunResult:
    """The reference's main(): config (the YAML dict, or a path to it) -> a finished run.

      1. the dataset: build_dataset(config, model_kind);
      2. build_model(config, dataset, model_kind, bag_dtype), moved to `device`;
      3. dataset.split(training.train_size, training.leave_one_out, seed, permutation);
      4. dataset.cohort(device, bag_dtype, cycle);
      5. fit.fit_options(config, model_kind);
      6. fit.Fit(model, cohort, split.train, split.val, options, sample_rows=sample_rows, seed=seed, test_ids=split.test or
         None, log=log, **fit_kwargs).run().
    `seed` keys both the split and the epoch orders (their streams are disjoint: fit.split_patients).
    model.load_from_checkpoint goes through Fit's `resume`.  The config's `device` key is not read: `device` is the argument.
    wandb.enabled: true is not acted on -- one warning points to `log=`, which is called with every epoch's row.

    ValueError, before any file of patches is opened: `device` resolving to a CPU (Fit captures graphs); an unknown
    model_kind; sample_rows missing.  Then the dataset's, fit_options' and Fit's own."""
    _check_kind(model_kind)
    dev = torch.device(device)
    if dev.type == "cpu":
        raise ValueError(f"run: device {str(device)!r} is a CPU; a run captures graphs of HIP kernels and needs the GPU")
    if sample_rows is None:
        raise ValueError("run: sample_rows is missing: the captured step's k rows per slide (the reference takes every row)")
    config = load_config(config)
    if (config.get("wandb") or {}).get("enabled"):
        warnings.warn("wandb.enabled is set, and this package does not log to W&B: pass log=callable, which is called with "
                      "every epoch's row of the table", stacklevel=2)
    data = build_dataset(config, model_kind)
    model = build_model(config, data, model_kind, bag_dtype).to(dev)
    training = config["training"]
    split = data.split(float(training["train_size"]), training.get("leave_one_out"), seed, permutation)
    cohort = data.cohort(dev, bag_dtype, cycle)
    options = fit.fit_options(config, model_kind)
    result = fit.Fit(model, cohort, split.train, split.val, options, sample_rows=sample_rows, seed=seed,
                     test_ids=split.test or None, log=log, **fit_kwargs).run()
    return RunResult(data, split, model, cohort, result)


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(prog="python -m multimodal_path_omic_amd.main",
                                     description="Train one of the reference's models from its config.yaml.")
    parser.add_argument("--model", required=True, choices=MODEL_KINDS)
    parser.add_argument("--config", required=True, help="the reference's config.yaml")
    parser.add_argument("--sample-rows", type=int, required=True, help="rows sampled per slide and step")
    parser.add_argument("--bag-dtype", choices=sorted(BAG_DTYPES), default="bf16")
    parser.add_argument("--cycle", action="store_true", help="lap slides shorter than --sample-rows")
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args(argv)
    result = run(args.config, args.model, sample_rows=args.sample_rows, bag_dtype=BAG_DTYPES[args.bag_dtype], cycle=args.cycle,
                 seed=args.seed)
    for row in result.fit.table():                      # the one host read, at the end
        print("  ".join(f"{k} {v}" if k == "epoch" else f"{k} {v:.6g}" for k, v in row.items()))


if __name__ == "__main__":
    main()
