"""The host side of a whole run (multimodal_path_omic_amd/fit.py): the patient-level split against the reference's
MultimodalDataset.split, property by property, and the reference's three config.yaml files -- written out here as the dicts
yaml.safe_load gives -- through fit_options.  Nothing here launches a kernel."""
import pytest

from multimodal_path_omic_amd import dp, fit, harness
from multimodal_path_omic_amd.harness import CE_REFUSAL

# seven patients of two slides, interleaved so that first appearance is not sorted order
PATIENTS = ["P3", "P1", "P3", "P7", "P2", "P1", "P5", "P2", "P4", "P7", "P6", "P5", "P6", "P4"]
UNIQUE = ["P3", "P1", "P7", "P2", "P5", "P4", "P6"]


def slides_of(*patients):
    return [i for i, p in enumerate(PATIENTS) if p in patients]


# ------------------------------------------------------------------------------------------------ split_patients
@pytest.mark.parametrize("train_size", [0.2, 0.5, 0.8, 0.99])
@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_split_counts_and_sides(train_size, seed):
    s = fit.split_patients(PATIENTS, train_size, seed=seed)
    assert s.test == [] and s.train == sorted(s.train) and s.val == sorted(s.val)
    assert sorted(s.train + s.val) == list(range(len(PATIENTS)))
    train_patients, val_patients = {PATIENTS[i] for i in s.train}, {PATIENTS[i] for i in s.val}
    assert not train_patients & val_patients                              # no patient on two sides
    assert len(train_patients) == int(len(UNIQUE) * train_size)           # the reference's cut
    assert len(val_patients) == len(UNIQUE) - int(len(UNIQUE) * train_size)


def test_split_shuffles_the_patients_in_order_of_first_appearance():
    """The shuffle permutes pandas.unique's order -- first appearance -- under the documented key, which is not an epoch's."""
    perm = dp._permutation(len(UNIQUE), 5, fit.SPLIT_EPOCH, 0)
    want = [UNIQUE[i] for i in perm]
    s = fit.split_patients(PATIENTS, 0.6, seed=5)
    assert s.train == slides_of(*want[:4]) and s.val == slides_of(*want[4:])
    assert fit.split_patients(PATIENTS, 0.6, permutation=want) == s
    assert fit.SPLIT_EPOCH < 0                                            # dp.epoch_orders' epochs count from 0
    assert perm != dp._permutation(len(UNIQUE), 5, 0, 0)


def test_split_is_a_function_of_the_seed():
    a = fit.split_patients(PATIENTS, 0.8, seed=3)
    assert fit.split_patients(list(PATIENTS), 0.8, seed=3) == a
    others = [fit.split_patients(PATIENTS, 0.8, seed=s) for s in range(4, 12)]
    assert any(o != a for o in others)


def test_split_with_an_explicit_permutation_is_the_hand_computed_one():
    # cut = int(7 * 0.5) = 3: train P5, P3, P6; val P1, P2, P4, P7
    s = fit.split_patients(PATIENTS, 0.5, seed=99, permutation=["P5", "P3", "P6", "P1", "P2", "P4", "P7"])
    assert s == fit.Split([0, 2, 6, 10, 11, 12], [1, 3, 4, 5, 7, 8, 9, 13], [])
    assert fit.split_patients(PATIENTS, 0.5, seed=0, permutation=["P5", "P3", "P6", "P1", "P2", "P4", "P7"]) == s   # seed ignored


@pytest.mark.parametrize("patient,side", [("P3", "train"), ("P4", "val")])
def test_leave_one_out_leaves_both_sides_after_the_cut(patient, side):
    order = ["P5", "P3", "P6", "P1", "P2", "P4", "P7"]
    whole = fit.split_patients(PATIENTS, 0.5, permutation=order)
    s = fit.split_patients(PATIENTS, 0.5, leave_one_out=patient, permutation=order)
    assert s.test == slides_of(patient) and len(s.test) == 2
    assert not set(s.test) & set(s.train) and not set(s.test) & set(s.val)
    # removed AFTER the cut: the other side is untouched, the patient's own side shrinks, nobody moves across
    if side == "train":
        assert s.val == whole.val and s.train == [i for i in whole.train if i not in s.test]
    else:
        assert s.train == whole.train and s.val == [i for i in whole.val if i not in s.test]
    for seed in range(6):
        r = fit.split_patients(PATIENTS, 0.8, leave_one_out=patient, seed=seed)
        assert r.test == slides_of(patient) and patient not in {PATIENTS[i] for i in r.train + r.val}
        assert sorted(r.train + r.val + r.test) == list(range(len(PATIENTS)))


def test_split_refusals():
    for bad in (0, 1, 0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError, match="train_size should be a float between 0 and 1."):
            fit.split_patients(PATIENTS, bad)
    with pytest.raises(ValueError, match="leave_one_out patient 'P9'"):
        fit.split_patients(PATIENTS, 0.8, leave_one_out="P9")
    with pytest.raises(ValueError, match="permutation holds 6 patients, the slides name 7"):
        fit.split_patients(PATIENTS, 0.8, permutation=UNIQUE[:6])
    with pytest.raises(ValueError, match="not a permutation of the 7 unique patients"):
        fit.split_patients(PATIENTS, 0.8, permutation=UNIQUE[:6] + ["P1"])
    with pytest.raises(ValueError, match="not a permutation of the 7 unique patients"):
        fit.split_patients(PATIENTS, 0.8, permutation=UNIQUE[:6] + ["P8"])
    with pytest.raises(ValueError, match="0 train and 14 val"):           # int(7 * 0.1) = 0 patients
        fit.split_patients(PATIENTS, 0.1)
    with pytest.raises(ValueError, match="12 train and 0 val"):           # the one val patient is the one left out
        fit.split_patients(PATIENTS, 0.9, leave_one_out="P6", permutation=["P3", "P1", "P7", "P2", "P5", "P4", "P6"])


# ------------------------------------------------------------------------------------------------ fit_options
def survival_config(name):
    """models/mcat/config/config.yaml and models/nacagat/config/config.yaml: they differ in model.name alone."""
    return {
        "device": "cuda",
        "wandb": {"enabled": True, "project": "CCNE1"},
        "dataset": {"name": "TCGA-OV", "file": "/work/h2020deciderficarra_shared/mgualtieri/ov/ov_fullest.csv",
                    "patches_dir": "/work/h2020deciderficarra_shared/mgualtieri/ov/slides/",
                    "signatures": "/work/tesi_mgualtieri/decider/multimodal-path-omic/input/signatures/ccne1.csv",
                    "decider_only": False, "tcga_only": True, "diagnostic_only": False, "normalize": False, "standardize": True},
        "model": {"name": name, "load_from_checkpoint": None, "checkpoint_epoch": 20, "checkpoint_dir": "checkpoints/",
                  "fusion": "concat", "model_size": "medium"},
        "training": {"leave_one_out": None, "output_attn_epoch": 20, "test_output_dir": "outputs/", "train_size": 0.8,
                     "loss": "ces", "epochs": 20, "optimizer": "adam", "lr": 0.0002, "weight_decay": 0.00001,
                     "grad_acc_step": 32, "scheduler": None, "alpha": 0.75, "lambda": 0.0, "gamma": 1.0},
    }


GE_CONFIG = {
    "device": "cuda",
    "wandb": {"enabled": True, "project": "GeneExpr-NaCAGaT-CCNE1"},
    "dataset": {"name": "DECIDER-OV", "file": "/work/h2020deciderficarra_shared/mgualtieri/ov/ov_fullest.csv",
                "patches_dir": "/work/h2020deciderficarra_shared/mgualtieri/ov/slides/",
                "signatures": "/work/tesi_mgualtieri/decider/multimodal-path-omic/input/signatures/signatures.csv",
                "decider_only": True},
    "model": {"name": "GeneExpr-NaCAGaT", "load_from_checkpoint": None, "checkpoint_epoch": 20, "checkpoint_dir": "checkpoints/",
              "fusion": "concat", "model_size": "medium", "gene": "CCNE1"},
    "training": {"leave_one_out": "M013", "output_attn_epoch": 5, "test_output_dir": "outputs/", "train_size": 0.8, "loss": "ce",
                 "epochs": 20, "optimizer": "adam", "lr": 0.0002, "weight_decay": 0.00001, "grad_acc_step": 32,
                 "scheduler": None, "lambda": 0.0, "gamma": 1.0},
}


@pytest.mark.parametrize("kind,name", [("mcat", "MCAT"), ("nacagat", "NaCAGaT")])
def test_fit_options_of_the_survival_configs(kind, name):
    config = survival_config(name)
    o = fit.fit_options(config, kind)
    assert o == fit.FitOptions(model_kind=kind, epochs=20, train_size=0.8, leave_one_out=None, output_attn_epoch=20,
                               test_output_dir="outputs/", model_name=name, checkpoint_epoch=20, checkpoint_dir="checkpoints/",
                               load_from_checkpoint=None, dataset_name="TCGA-OV",
                               train=harness.training_options(config["training"], kind))
    assert (o.train.loss, o.train.grad_acc_step, o.train.optimizer, o.train.lr, o.train.weight_decay, o.train.l1, o.train.gamma) == \
        ("ces", 32, "adam", 0.0002, 0.00001, 0.0, None)


def test_fit_options_of_the_gene_expression_config():
    o = fit.fit_options(GE_CONFIG, "ge_nacagat")
    assert o == fit.FitOptions(model_kind="ge_nacagat", epochs=20, train_size=0.8, leave_one_out="M013", output_attn_epoch=5,
                               test_output_dir="outputs/", model_name="GeneExpr-NaCAGaT", checkpoint_epoch=20,
                               checkpoint_dir="checkpoints/", load_from_checkpoint=None, dataset_name="DECIDER-OV",
                               train=harness.training_options(GE_CONFIG["training"], "ge_nacagat"))
    assert o.train.loss == "ce" and o.train.gamma is None


def test_fit_options_reads_a_checkpoint_path_and_a_schedule():
    config = survival_config("MCAT")
    config["model"].update(load_from_checkpoint="checkpoints/MCAT_20_202408081300.pt", checkpoint_epoch=0)
    config["training"].update(scheduler="exp", gamma=0.95, leave_one_out="H042")
    o = fit.fit_options(config, "mcat")
    assert (o.load_from_checkpoint, o.checkpoint_epoch, o.leave_one_out, o.train.gamma) == \
        ("checkpoints/MCAT_20_202408081300.pt", 0, "H042", 0.95)


@pytest.mark.parametrize("kind,name", [("mcat", "MCAT"), ("nacagat", "NaCAGaT")])
def test_fit_options_refuses_ce_for_a_fusion_model(kind, name):
    config = survival_config(name)
    config["training"]["loss"] = "ce"
    with pytest.raises(ValueError) as e:
        fit.fit_options(config, kind)
    assert str(e.value) == CE_REFUSAL
