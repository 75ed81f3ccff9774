"""Seeded cases of tests/golden/train_options.npz (make_golden_train_options.py) shared with the tests that read it: the
reference's `training:` dicts of the three cohort runs, on the cohort of cases.COHORT."""

# (model kind, fusion, training dict as models/{mcat,nacagat}/config/config.yaml spells it)
RUNS = {
    "mcat_sct_adamax": ("mcat", "concat", dict(loss="sct", optimizer="adamax", lr=5e-4, weight_decay=1e-5, grad_acc_step=8,
                                               scheduler="exp", gamma=0.8, alpha=0.75, **{"lambda": 1e-5})),
    "nacagat_cesar_adadelta": ("nacagat", "concat", dict(loss="cesar", optimizer="adadelta", lr=1.0, weight_decay=1e-5,
                                                         grad_acc_step=8, scheduler=None, gamma=1.0, alpha=0.3,
                                                         **{"lambda": 0.0})),
    "mcat_bilinear_ces_sgd": ("mcat", "bilinear", dict(loss="ces", optimizer="sgd", lr=1e-2, weight_decay=1e-5,
                                                       grad_acc_step=8, scheduler="~", gamma=0.5, alpha=0.5,
                                                       **{"lambda": None})),
}

SCT_SEED, L1_SEED = 811, 812
