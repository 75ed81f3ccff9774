"""state_dict() / load_state_dict() of the flat optimisers and checkpoint.save / load, without a device: the flat
optimisers construct on CPU parameters (only step() calls the library), so non-zero state is made by filling the flat
buffers with seeded values.  What stock torch.optim writes is taken from the installed torch at run time, and the
reference's parameter names and order from tests/golden/state_dicts.npz."""
import os

import numpy as np
import pytest
import torch

from multimodal_path_omic_amd import checkpoint, ops
from multimodal_path_omic_amd import models as ours
from multimodal_path_omic_amd.dp import (SLICE_ALIGN, FlatAdam, FlatExponentialLR, FlatGradBucket, FlatOptimizer,
                                         package_only_parameter_names)

SIZES = [100, 200, 300, 400, 500, 600]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_dicts.npz")
ALGORITHMS = ["adam", "adamax", "adadelta", "sgd"]
KW = {"adam": dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-5),
      "adamax": dict(lr=2e-3, betas=(0.85, 0.98), eps=1e-7, weight_decay=1e-5),
      "adadelta": dict(lr=0.7, rho=0.85, eps=1e-5, weight_decay=1e-5),
      "sgd": dict(lr=1e-2, weight_decay=1e-5)}
VARIANTS = [(kind, fusion) for kind in ("mcat", "nacagat") for fusion in ("concat", "bilinear", "gated_concat")]


def _listing(key):
    with np.load(GOLDEN, allow_pickle=False) as z:
        names, shapes = z[key + "/names"].tolist(), z[key + "/shapes"].tolist()
    return [str(n) for n in names], [tuple(d for d in s if d >= 0) for s in shapes]


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen) * 0.05) for s in _listing("mcat/concat")[1]]


def _torch_opt(alg, params):
    cls = {"adam": torch.optim.Adam, "adamax": torch.optim.Adamax, "adadelta": torch.optim.Adadelta, "sgd": torch.optim.SGD}
    return cls[alg](params, **KW[alg])


def _flat(alg, params, cls=FlatOptimizer):
    bucket = FlatGradBucket(params)
    if cls is FlatAdam:
        return FlatAdam(bucket, **KW["adam"])
    return FlatOptimizer(bucket, alg, **KW[alg])


def _moment_buffers(opt):
    return opt._moments()


def _seed_state(opt, seed, t):
    """Seeded non-zero moments in every parameter's slice (the padding between slices stays zero, as a step keeps it)."""
    gen = torch.Generator().manual_seed(seed)
    for flat in _moment_buffers(opt):
        for p, off in zip(opt.bucket.params, opt.bucket.offsets):
            flat[off:off + p.numel()].copy_(torch.rand(p.numel(), generator=gen) + 0.1)
    opt.t_dev.fill_(t)


def _padding_mask(bucket):
    pad = torch.ones_like(bucket.flat, dtype=torch.bool)
    for p, off in zip(bucket.params, bucket.offsets):
        pad[off:off + p.numel()] = False
    return pad


def _model(kind, fusion):
    cls = ours.MultimodalCoAttentionTransformer if kind == "mcat" else ours.NarrowContextualAttentionGateTransformer
    return cls(omic_sizes=SIZES, fusion=fusion)


def _structure(v):
    """Nesting, keys, and dtype / shape of every tensor; other leaves by type."""
    if torch.is_tensor(v):
        return ("tensor", v.dtype, tuple(v.shape), v.device.type)
    if isinstance(v, dict):
        return {k: _structure(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v), [_structure(x) for x in v]
    return type(v)


# ------------------------------------------------------------------------------------ 1. structure
@pytest.mark.parametrize("alg", ALGORITHMS)
def test_state_dict_has_the_structure_of_stock_torch(alg):
    stock_params = _params()
    stock = _torch_opt(alg, stock_params)
    for p in stock_params:
        p.grad = torch.ones_like(p)
    stock.step()
    want = stock.state_dict()
    flat = _flat(alg, _params())
    _seed_state(flat, 5, t=1)
    got = flat.state_dict()
    assert list(got) == list(want)
    assert _structure(got) == _structure(want)
    assert got["param_groups"] == want["param_groups"]                 # hyper-parameters, flags, params 0 .. n-1
    if alg != "sgd":
        assert all(float(e["step"]) == 1.0 for e in got["state"].values())
    # the tensors are clones: compact storages, none shared with the flat buffers
    bases = {m.untyped_storage().data_ptr() for m in _moment_buffers(flat)}
    for e in got["state"].values():
        for v in e.values():
            assert v.untyped_storage().data_ptr() not in bases
            assert v.untyped_storage().nbytes() == v.numel() * v.element_size()
    # and stock torch takes the dict
    fresh = _torch_opt(alg, _params())
    fresh.load_state_dict(got)
    for i, e in got["state"].items():
        for k, v in e.items():
            assert torch.equal(fresh.state[fresh.param_groups[0]["params"][i]][k], v)


def test_flat_adam_writes_the_same_dict_as_the_adam_algorithm():
    a, o = _flat("adam", _params(), FlatAdam), _flat("adam", _params())
    _seed_state(a, 9, t=4)
    _seed_state(o, 9, t=4)
    sa, so = a.state_dict(), o.state_dict()
    assert sa["param_groups"] == so["param_groups"] and _structure(sa) == _structure(so)
    assert all(torch.equal(sa["state"][i][k], so["state"][i][k]) for i in so["state"] for k in so["state"][i])
    b = _flat("adam", _params(1), FlatAdam)
    b.load_state_dict(so)
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq) and int(b.t_dev) == 4


# ------------------------------------------------------------------------------------ 2. parameter order
@pytest.mark.parametrize("kind,fusion", VARIANTS)
def test_parameter_order_is_the_reference_models(kind, fusion, tmp_path):
    names, shapes = _listing(f"{kind}/{fusion}")
    model = _model(kind, fusion)
    own = dict(model.named_parameters())
    assert all(n in own for n in names)                    # (the reference models hold no buffers: every entry is a parameter)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, "adam")
    # mark every parameter's first-moment slice with its index in the bucket
    for i, (p, off) in enumerate(zip(bucket.params, bucket.offsets)):
        opt.state1[off:off + p.numel()] = float(i + 1)
    opt.t_dev.fill_(2)
    index = {id(p): i for i, p in enumerate(bucket.params)}
    sd, only = opt.state_dict(model)
    assert sd["param_groups"][0]["params"] == list(range(len(names)))
    assert sorted(sd["state"]) == list(range(len(names)))
    for j, (n, s) in enumerate(zip(names, shapes)):
        e = sd["state"][j]["exp_avg"]
        assert tuple(e.shape) == s, (n, tuple(e.shape), s)
        assert bool((e == float(index[id(own[n])] + 1)).all()), n
    gates = [n for n in own if n not in names]
    assert sorted(only) == sorted(gates) == sorted(package_only_parameter_names(model))
    if fusion == "gated_concat":
        assert gates and all(n.startswith("fusion_layer.gates.") for n in gates)
        for n in gates:
            assert bool((only[n]["exp_avg"] == float(index[id(own[n])] + 1)).all())
    else:
        assert not gates
    # the file: the reference's two dicts hold the reference's entries only, the gates travel in `mpo`
    path = tmp_path / "ck.pt"
    checkpoint.save(path, model, opt, 3, 0.25)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "loss", "mpo"]
    assert list(ck["model_state_dict"]) == names
    assert len(ck["optimizer_state_dict"]["state"]) == len(names)
    assert sorted(ck["mpo"]["model_state"]) == sorted(ck["mpo"]["optimizer_state"]) == sorted(gates)


# ------------------------------------------------------------------------------------ 3. safe load, file size
@pytest.mark.parametrize("kind,fusion,alg", [("mcat", "concat", "adam"), ("nacagat", "gated_concat", "adamax"),
                                             ("mcat", "bilinear", "sgd")])
def test_file_loads_safely_and_holds_no_flat_storage(kind, fusion, alg, tmp_path):
    model = _model(kind, fusion)
    bucket = FlatGradBucket(list(model.parameters()))
    opt = FlatOptimizer(bucket, alg, **KW[alg])
    _seed_state(opt, 3, t=7)
    sched = FlatExponentialLR(opt, 0.8)
    sched.step()
    path = tmp_path / "ck.pt"
    checkpoint.save(path, model, opt, 4, torch.tensor(0.5), scheduler=sched)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["epoch"] == 4 and float(ck["loss"]) == 0.5
    assert ck["mpo"]["algorithm"] == alg and ck["mpo"]["step"] == 7
    assert ck["mpo"]["scheduler"] == {"gamma": 0.8, "last_epoch": 1} and ck["mpo"]["graph_rng_base"] is None
    assert ck["mpo"]["rng"] == ops.rng_state()
    assert ck["optimizer_state_dict"]["param_groups"][0]["lr"] == KW[alg]["lr"] * 0.8
    model_bytes = sum(v.numel() * v.element_size() for v in model.state_dict().values())
    state_bytes = 0 if alg == "sgd" else sum(2 * p.numel() * 4 + 4 for p in bucket.params)
    size = os.path.getsize(path)
    print(f"[checkpoint {kind}/{fusion} {alg}] file {size} B = model {model_bytes} + optimiser state {state_bytes} "
          f"+ {size - model_bytes - state_bytes}")
    assert size <= model_bytes + state_bytes + 64 * 1024
    assert os.listdir(tmp_path) == ["ck.pt"]                      # no temporary left behind


# ------------------------------------------------------------------------------------ 4. in-place load
@pytest.mark.parametrize("alg", ALGORITHMS)
def test_load_is_in_place_and_keeps_the_padding_zero(alg):
    src = _flat(alg, _params(1))
    _seed_state(src, 11, t=6)
    sd = src.state_dict()
    dst = _flat(alg, _params(2))
    _seed_state(dst, 12, t=1)
    params = dst.bucket.params
    tensors = [t for t in (dst.flat_p, dst.state1, dst.state2, dst.t_dev, dst.lr_dev, dst.bucket.flat) if t is not None]
    ptrs = [t.data_ptr() for t in tensors] + [p.data_ptr() for p in params]
    sd["param_groups"][0]["lr"] = 1.25e-3
    dst.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in tensors] + [p.data_ptr() for p in params]
    assert all(p.untyped_storage().data_ptr() == dst.flat_p.untyped_storage().data_ptr() for p in params)
    pad = _padding_mask(dst.bucket)
    assert int(pad.sum()) > 0 and dst.flat_p.numel() % SLICE_ALIGN == 0
    for flat in [dst.flat_p] + _moment_buffers(dst):
        assert float(flat[pad].abs().max()) == 0.0
    for a, b in zip(_moment_buffers(src), _moment_buffers(dst)):
        assert torch.equal(a, b)
    if alg != "sgd":
        assert int(dst.t_dev) == 6
    assert dst.lr == 1.25e-3 and float(dst.lr_dev) == float(np.float32(1.25e-3))
    assert dst.wd == KW[alg]["weight_decay"]
    # torch's own dict (steps as tensors) and one with integer steps load alike
    for e in sd["state"].values():
        e["step"] = int(e["step"])
    dst.load_state_dict(sd)
    assert alg == "sgd" or int(dst.t_dev) == 6


def test_checkpoint_load_is_in_place_and_restores_everything(tmp_path):
    model = _model("mcat", "gated_concat")
    opt = FlatOptimizer(FlatGradBucket(list(model.parameters())), "adamax", **KW["adamax"])
    _seed_state(opt, 21, t=9)
    sched = FlatExponentialLR(opt, 0.5)
    sched.step()
    path = tmp_path / "ck.pt"
    ops.set_rng_epoch(None)
    before = ops.rng_state()
    checkpoint.save(path, model, opt, 1, 0.125, scheduler=sched)
    try:
        ops._rng_calls += 12345                                    # whatever ran in between
        other = _model("mcat", "gated_concat")
        opt2 = FlatOptimizer(FlatGradBucket(list(other.parameters())), "adamax")
        sched2 = FlatExponentialLR(opt2, 0.9)
        ptrs = [t.data_ptr() for t in opt2.state_tensors()] + [p.data_ptr() for p in other.parameters()]
        assert not torch.equal(opt2.flat_p, opt.flat_p)
        res = checkpoint.load(path, other, opt2, sched2)
        assert (res.epoch, res.loss, res.graph_rng_base, res.from_reference) == (1, 0.125, None, False)
        assert ptrs == [t.data_ptr() for t in opt2.state_tensors()] + [p.data_ptr() for p in other.parameters()]
        for a, b in zip(opt.state_tensors(), opt2.state_tensors()):
            assert torch.equal(a, b)
        assert opt2.lr == opt.lr and torch.equal(opt2.lr_dev, opt.lr_dev) and opt2.betas == opt.betas and opt2.eps == opt.eps
        assert (sched2.gamma, sched2.last_epoch) == (0.5, 1)
        assert ops.rng_state() == before
    finally:
        ops.set_rng_state(before)


def test_file_of_the_reference_loads_and_leaves_the_generator_alone(tmp_path):
    """What the reference's main.py writes: its model's state_dict, stock torch.optim's state_dict, no `mpo`."""
    names, shapes = _listing("mcat/gated_concat")
    gen = torch.Generator().manual_seed(4)
    ref_params = [torch.nn.Parameter(torch.randn(*s, generator=gen) * 0.05) for s in shapes]
    stock = torch.optim.Adam(ref_params, lr=2e-4, weight_decay=1e-5)
    stock_sched = torch.optim.lr_scheduler.ExponentialLR(stock, 0.5)
    for _ in range(3):
        for p in ref_params:
            p.grad = torch.randn(p.shape, generator=gen)
        stock.step()
    stock_sched.step()
    path = tmp_path / "ref.pt"
    torch.save({"epoch": 2, "model_state_dict": {n: p.detach() for n, p in zip(names, ref_params)},
                "optimizer_state_dict": stock.state_dict(), "loss": 1.5}, path)
    model = _model("mcat", "gated_concat")
    opt = FlatOptimizer(FlatGradBucket(list(model.parameters())), "adam")
    sched = FlatExponentialLR(opt, 0.5)
    gates_before = {n: p.detach().clone() for n, p in model.named_parameters() if n in package_only_parameter_names(model)}
    rng = ops.rng_state()
    res = checkpoint.load(path, model, opt, sched)
    assert (res.epoch, res.loss, res.from_reference) == (2, 1.5, True) and ops.rng_state() == rng
    own = dict(model.named_parameters())
    index = {id(p): i for i, p in enumerate(opt.bucket.params)}
    for j, n in enumerate(names):
        assert torch.equal(own[n].detach(), ref_params[j].detach())
        off = opt.bucket.offsets[index[id(own[n])]]
        assert torch.equal(opt.state1[off:off + own[n].numel()].view(own[n].shape), stock.state[ref_params[j]]["exp_avg"])
    for n, v in gates_before.items():
        off = opt.bucket.offsets[index[id(own[n])]]
        assert torch.equal(own[n].detach(), v) and float(opt.state1[off:off + v.numel()].abs().max()) == 0.0
    assert int(opt.t_dev) == 3 and opt.lr == 2e-4 * 0.5 and opt.wd == 1e-5
    sched.step()                                                    # continues from the group's lr, as the reference's resume
    assert opt.lr == 2e-4 * 0.5 * 0.5


# ------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_problem():
    adamax = _flat("adamax", _params())
    _seed_state(adamax, 1, t=3)
    good = _flat("adam", _params())
    _seed_state(good, 2, t=3)
    dst = _flat("adam", _params())
    keep = [t.clone() for t in dst.state_tensors()]
    with pytest.raises(ValueError, match=r"exp_inf.*not the moments of 'adam'"):
        dst.load_state_dict(adamax.state_dict())
    sd = good.state_dict()
    sd["state"][5]["exp_avg_sq"] = sd["state"][5]["exp_avg_sq"].reshape(-1)[:-1].clone()
    with pytest.raises(ValueError, match=r"shape of exp_avg_sq of parameter 5 differs"):
        dst.load_state_dict(sd)
    sd = good.state_dict()
    sd["state"][7]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match=r"per-parameter steps differ"):
        dst.load_state_dict(sd)
    sd = good.state_dict()
    n = len(sd["param_groups"][0]["params"])
    sd["param_groups"][0]["params"].append(n)
    sd["state"][n] = {k: v.clone() for k, v in sd["state"][n - 1].items()}
    with pytest.raises(ValueError, match=rf"parameter count differs.*{n + 1} parameters.*holds {n}"):
        dst.load_state_dict(sd)
    sd = good.state_dict()
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match=r"amsgrad"):
        dst.load_state_dict(sd)
    for t, k in zip(dst.state_tensors(), keep):                     # a refused load has written nothing
        assert torch.equal(t, k)


# ------------------------------------------------------------------------------------ 6. interrupted write
def test_interrupted_write_keeps_the_previous_checkpoint(tmp_path, monkeypatch):
    model = _model("mcat", "concat")
    opt = FlatOptimizer(FlatGradBucket(list(model.parameters())), "adam")
    _seed_state(opt, 31, t=2)
    path = tmp_path / "ck.pt"
    checkpoint.save(path, model, opt, 0, 0.75)
    first = path.read_bytes()
    real_save = torch.save

    def dies_mid_write(obj, f, *args, **kwargs):
        real_save(obj, f, *args, **kwargs)
        size = os.path.getsize(f)
        with open(f, "r+b") as fh:
            fh.truncate(size // 2)
        raise OSError("killed mid-write")

    monkeypatch.setattr(torch, "save", dies_mid_write)
    _seed_state(opt, 32, t=5)
    with pytest.raises(OSError, match="killed mid-write"):
        checkpoint.save(path, model, opt, 1, 0.5)
    monkeypatch.undo()
    assert path.read_bytes() == first and os.listdir(tmp_path) == ["ck.pt"]
    other = _model("mcat", "concat")
    opt2 = FlatOptimizer(FlatGradBucket(list(other.parameters())), "adam")
    rng = ops.rng_state()
    try:
        res = checkpoint.load(path, other, opt2)
    finally:
        ops.set_rng_state(rng)
    assert (res.epoch, res.loss) == (0, 0.75) and int(opt2.t_dev) == 2


def test_rng_state_round_trip_and_default_graph_arguments():
    """ops.rng_state() / set_rng_state() carry the three values; GraphedWindowStep takes rng_base and defaults to None."""
    import inspect
    from multimodal_path_omic_amd import harness
    assert inspect.signature(harness.GraphedWindowStep.__init__).parameters["rng_base"].default is None
    ops.set_rng_epoch(None)
    before = ops.rng_state()
    try:
        assert set(before) == {"seed", "calls", "epoch"} and before["epoch"] is None
        ops.set_rng_epoch(torch.full((1,), 5, dtype=torch.int64))
        t = ops._rng_epoch_tensor
        ops.next_dropout_stream(1000)
        assert ops.rng_state() == {"seed": before["seed"], "calls": before["calls"] + 251, "epoch": 5}
        ops.set_rng_state({"seed": before["seed"], "calls": 17, "epoch": 9})
        assert ops._rng_epoch_tensor is t and int(t) == 9 and ops.next_dropout_stream(4) == (before["seed"] & (2 ** 64 - 1), 17)
        ops.set_rng_epoch(None)
        ops.set_rng_state({"seed": before["seed"], "calls": 3, "epoch": 2}, device="cpu")
        assert int(ops._rng_epoch_tensor) == 2 and ops._rng_epoch_tensor.dtype == torch.int64
    finally:
        ops.set_rng_epoch(None)
        ops.set_rng_state(before)
