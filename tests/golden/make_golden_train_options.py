#!/usr/bin/env python3
"""Generate tests/golden/train_options.npz by running THE REFERENCE ITSELF (torch CPU fp32) for the training options beside
the default one: the `sct` loss (models/loss.py:62-85), l1_reg (models/utils.py:33-40) and three cohort runs of the
reference's train()/validate() loop (models/mcat/main.py:19-155, restated as make_golden.gen_cohort does: model.eval(),
fixed slide order and split) with the optimiser, schedule and penalty its main() builds from the config
(main.py:272-318; nacagat/main.py:283-296 for `cesar`).

Run in the authoring container only:   python tests/golden/make_golden_train_options.py
Reuses make_golden.py's import recipe, build_model and save (that file is not modified)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np                                                        # noqa: E402
import torch                                                              # noqa: E402
import torch.nn.functional as F                                           # noqa: E402

from make_golden import C, build_model, save, syn, REF                    # noqa: E402  (sets up the reference imports)
from models.loss import (CrossEntropySurvivalAttnRegLoss, CrossEntropySurvivalLoss,  # noqa: E402
                         SurvivalClassificationTobitLoss)
from models.utils import l1_reg                                           # noqa: E402
from mcat import MultimodalCoAttentionTransformer                         # noqa: E402
import torch.optim.lr_scheduler as lrs                                    # noqa: E402

import train_option_cases as T                                            # noqa: E402

assert os.path.isdir(REF)


def gen_sct(out):
    """Every label, both censorings, ordinary and peaky logits (Y[y] down to ~1e-9); gradient into the logits via softmax."""
    sct = SurvivalClassificationTobitLoss()
    g = syn.rng(T.SCT_SEED)
    logits = syn.normal(g, (16, 4)) * 2.0
    peaky = torch.zeros(8, 4)
    for i in range(8):
        peaky[i, (i + 1) % 4] = 21.0 + i % 3             # softmax mass on another class: Y[label] ~ 1e-9 .. 1e-10
    logits = torch.cat([logits, peaky])
    labels, cens, losses, grads = [], [], [], []
    for i in range(logits.shape[0]):
        y_lab, c = i % 4, float((i // 4) % 2)
        lg = logits[i:i + 1].clone().requires_grad_(True)
        Y = F.softmax(lg, dim=1)
        loss = sct(Y, torch.tensor([y_lab]), c=torch.tensor([c]))
        loss.backward()
        labels.append(y_lab), cens.append(c), losses.append(loss.detach().reshape(())), grads.append(lg.grad[0])
    out["sct/logits"] = logits
    out["sct/label"] = np.array(labels, dtype=np.int64)
    out["sct/censorship"] = np.array(cens, dtype=np.float32)
    out["sct/loss"] = torch.stack(losses).reshape(-1)
    out["sct/dlogits"] = torch.stack(grads)


def build(kind, fusion, omic_sizes, seed):
    if fusion == "concat":
        return build_model(kind, omic_sizes, seed)
    assert kind == "mcat"
    model = MultimodalCoAttentionTransformer(omic_sizes=omic_sizes, model_size="medium", fusion=fusion).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.fill_state_dict(shapes, seed), strict=True)
    return model


def gen_l1(out):
    cfg = C.COHORT
    model = build("mcat", "concat", cfg["omic_sizes"], T.L1_SEED)
    out["l1/value"] = l1_reg(model).detach().double().reshape(1)


def make_optimizer(tr, model):
    """models/mcat/main.py:284-300."""
    params = filter(lambda p: p.requires_grad, model.parameters())
    name = tr["optimizer"]
    if name == "sgd":
        return torch.optim.SGD(params, lr=tr["lr"])
    if name == "adadelta":
        return torch.optim.Adadelta(params, lr=tr["lr"], weight_decay=tr["weight_decay"])
    if name == "adamax":
        return torch.optim.Adamax(params, lr=tr["lr"], weight_decay=tr["weight_decay"])
    return torch.optim.Adam(params, lr=tr["lr"], weight_decay=tr["weight_decay"])


def gen_runs(out):
    cfg = C.COHORT
    slides = syn.make_cohort(cfg["n_slides"], cfg["m_lo"], cfg["m_hi"], cfg["omic_sizes"], cfg["seed"])
    n_train = int(cfg["train_frac"] * len(slides))
    for name, (kind, fusion, tr) in T.RUNS.items():
        acc = tr["grad_acc_step"]
        assert n_train % acc == 0
        model = build(kind, fusion, cfg["omic_sizes"], cfg["weight_seed"])
        model.eval()
        opt = make_optimizer(tr, model)
        sched = lrs.ExponentialLR(opt, gamma=tr["gamma"]) if tr["scheduler"] == "exp" else None
        lam = tr["lambda"]
        if tr["loss"] == "ces":
            loss_fn = CrossEntropySurvivalLoss(alpha=tr["alpha"])
        elif tr["loss"] == "sct":
            loss_fn = SurvivalClassificationTobitLoss()
        else:
            loss_fn = CrossEntropySurvivalAttnRegLoss()
        for epoch in range(cfg["epochs"]):
            risks, losses = [], []
            for i, s in enumerate(slides[:n_train]):
                kw = dict(inference=True) if kind == "mcat" else {}
                hz, sv, Y, att = model(wsi=s["wsi"].unsqueeze(0), omics=[o.unsqueeze(0) for o in s["omics"]], **kw)
                label = torch.tensor([s["survival_class"]])
                c = torch.tensor([float(s["censorship"])])
                if tr["loss"] == "ces":
                    loss = loss_fn(hz, sv, label, c=c)
                elif tr["loss"] == "sct":
                    loss = loss_fn(Y, label, c=c)
                else:
                    loss, _ = loss_fn(hz, sv, label, c=c, attention=att["coattn"])
                loss_reg = l1_reg(model) * lam if lam else 0
                losses.append(loss.item() + float(loss_reg))
                risks.append(-torch.sum(sv, dim=1).item())
                (loss / acc + loss_reg).backward()
                if (i + 1) % acc == 0:
                    opt.step()
                    opt.zero_grad()
            out[f"{name}/train_risk/{epoch}"] = np.array(risks)
            out[f"{name}/train_loss/{epoch}"] = np.array(losses)
            out[f"{name}/lr/{epoch}"] = np.array([opt.param_groups[0]["lr"]])
            if sched is not None:
                sched.step()
            vr = []
            with torch.no_grad():
                for s in slides[n_train:]:
                    kw = dict(inference=True) if kind == "mcat" else {}
                    _, sv, _, _ = model(wsi=s["wsi"].unsqueeze(0), omics=[o.unsqueeze(0) for o in s["omics"]], **kw)
                    vr.append(-torch.sum(sv, dim=1).item())
            out[f"{name}/val_risk/{epoch}"] = np.array(vr)
            print(f"{name} epoch {epoch}: loss {np.mean(losses):.4f}", flush=True)


if __name__ == "__main__":
    out = {}
    gen_sct(out)
    gen_l1(out)
    gen_runs(out)
    save("train_options", out)
