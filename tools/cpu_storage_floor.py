"""CPU: attribute the bf16 storage mode's co-attention map error (against the fp32 reference fixtures) to its storage points --
patch matrix X, patch-layer weight operand W_H, H_bag -- with the oracle, at the benchmarked bag length.
    python tools/cpu_storage_floor.py [--dtype bfloat16|float16] [case ...]        default: bfloat16; mcat_m15000 nacagat_m15000
--dtype float16: the same attribution for fp16 storage (an fp16 window stores X alone in fp16: the row "x")."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import cases as C  # noqa: E402
from multimodal_path_omic_amd import synthetic as syn  # noqa: E402
from oracle import mpo_oracle as O  # noqa: E402

with np.load(os.path.join(ROOT, "tests", "golden", "models.npz"), allow_pickle=False) as z:
    g = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
args = sys.argv[1:]
storage = torch.bfloat16
if "--dtype" in args:
    i = args.index("--dtype")
    storage = {"bfloat16": torch.bfloat16, "float16": torch.float16}[args[i + 1]]
    del args[i:i + 2]
tag = {torch.bfloat16: "bf16", torch.float16: "fp16"}[storage]
for case in (args or ["mcat_m15000", "nacagat_m15000"]):
    kind, m, omic_sizes, seed = C.MODEL_CASES[case]
    sd = syn.fill_state_dict(C.model_shapes(omic_sizes, kind == "nacagat"), seed)
    wsi, omics, _, _ = C.model_inputs(m, omic_sizes, seed + 1)
    fwd = O.mcat_forward if kind == "mcat" else O.nacagat_forward
    kw = dict(inference=True) if kind == "mcat" else {}
    ga = g[f"{case}/A_coattn_sub"]
    with torch.no_grad():
        for pts in (("x",), ("w",), ("h",), ("x", "w"), ("x", "h"), ("w", "h"), ("x", "w", "h")):
            hz, _, _, att = fwd(sd, wsi, omics, bag_storage=storage, storage_points=pts, **kw)
            e_a = float(((syn.subsample(att["coattn"]) - ga).abs() / ga.clamp_min(1e-30)).max())
            e_p = float((att["path"].reshape(-1) - g[f"{case}/A_path"].reshape(-1)).abs().max() / g[f"{case}/A_path"].abs().max())
            e_h = float((hz - g[f"{case}/hazards"]).abs().max())
            print(f"{case:16s} {tag} at {'+'.join(pts):6s}: coattn map rel {e_a:.2e}   path map rel {e_p:.2e}   hazards {e_h:.1e}", flush=True)
