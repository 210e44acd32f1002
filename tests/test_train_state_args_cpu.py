"""CPU: what opt.train_state accepts and refuses before anything is built, and the host half of train_state.py -- the atomic file,
its format version, the optimizer state's round trip and the digest comparison (no kernel is launched here)."""
from types import SimpleNamespace

import pytest
import torch

from helpers import make_opt

C = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)


def option(**kw):
    from de_i2i_gan_amd import train_state as TS
    return TS.train_state_option(SimpleNamespace(device=torch.device("cuda:0"), style_norm_block_type="spade", **kw))


def test_off_when_absent_none_or_false():
    assert option() is False and option(train_state=None) is False and option(train_state=False) is False
    assert option(train_state=True) is True


@pytest.mark.parametrize("bad", [1, 0, "yes", "true", 2.0])
def test_only_booleans(bad):
    with pytest.raises(ValueError, match="train_state"):
        option(train_state=bad)


def test_sean_and_cpu_devices_are_refused():
    from de_i2i_gan_amd import train_state as TS
    with pytest.raises(NotImplementedError, match="sean"):
        TS.train_state_option(SimpleNamespace(device=torch.device("cuda:0"), style_norm_block_type="sean", train_state=True))
    with pytest.raises(ValueError, match="GPU"):
        TS.train_state_option(SimpleNamespace(device=torch.device("cpu"), style_norm_block_type="spade", train_state=True))
    # ... and off, neither matters
    assert TS.train_state_option(SimpleNamespace(device=torch.device("cpu"), style_norm_block_type="sean")) is False


def test_trainers_refuse_before_anything_is_built(monkeypatch):
    from de_i2i_gan_amd.trainers import base_trainer
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer

    def no_model(opt):
        raise AssertionError("the model was built")
    monkeypatch.setattr(base_trainer, "create_model", no_model)
    for cls in (DefectGanTrainer, MAETrainer):
        with pytest.raises(NotImplementedError, match="sean"):
            cls(make_opt(C, "cpu", style_norm_block_type="sean", train_state=True))
        with pytest.raises(ValueError, match="GPU"):
            cls(make_opt(C, "cpu", train_state=True))
        with pytest.raises(ValueError, match="train_state"):
            cls(make_opt(C, "cpu", train_state="on"))


def test_option_off_builds_the_trainer_it_always_built():
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    tr = DefectGanTrainer(make_opt(C, "cpu"))
    assert tr.train_state is False and tr.train_state_restored is None
    tr.resume_train_state()                                 # (nothing to do, nothing read)
    assert tr.train_state_restored is None


def test_file_is_atomic_versioned_and_tensor_only(tmp_path):
    from de_i2i_gan_amd import train_state as TS
    path = tmp_path / "run" / "latest_train_state.pth"
    state = {"iters": 3, "digests": {"net_G": 2 ** 64 - 1}, "rng": TS.rng_state("cpu"), "mask_rng": [2 ** 64 - 1, 5],
             "optimizers": {"G": [[{"step": 2, "exp_avg": torch.ones(3)}, None]]}}
    TS.write(state, path)
    assert sorted(p.name for p in path.parent.iterdir()) == ["latest_train_state.pth"]
    back = TS.read(path)
    assert back["format_version"] == TS.FORMAT_VERSION == 1 and back["digests"] == state["digests"] and back["mask_rng"] == state["mask_rng"]
    assert torch.equal(back["rng"]["cpu"], state["rng"]["cpu"]) and "device" not in back["rng"]
    assert torch.load(path, weights_only=True)["iters"] == 3
    # a failed write leaves the previous file and no temporary
    with pytest.raises(Exception):
        TS.write({"bad": lambda: None}, path)
    assert sorted(p.name for p in path.parent.iterdir()) == ["latest_train_state.pth"] and TS.read(path)["iters"] == 3
    for version in (2, 0, "1", None):
        torch.save(dict(state, format_version=version), path)
        with pytest.raises(RuntimeError, match="format version"):
            TS.read(path)
    torch.save([1, 2], path)
    with pytest.raises(RuntimeError, match="format version"):
        TS.read(path)


def test_cpu_rng_round_trip():
    from de_i2i_gan_amd import train_state as TS
    torch.manual_seed(5)
    torch.rand(3)
    state = TS.rng_state("cpu")
    want = torch.rand(4)
    torch.manual_seed(99)
    TS.set_rng_state(state, "cpu")
    assert torch.equal(torch.rand(4), want)


def _optimizer(shapes=((3, 2), (4,), (2, 2))):
    from de_i2i_gan_amd.optim import FusedAdam
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    return FusedAdam([{"params": params[:2]}, {"params": params[2:]}], lr=1e-3), params


def test_optimizer_state_round_trip_keeps_the_learning_rates():
    from de_i2i_gan_amd import train_state as TS
    src, params = _optimizer()
    for i, p in enumerate(params[:2]):                      # (the third parameter never had a gradient: no state)
        src.state[p] = {"step": 7 + i, "exp_avg": torch.full_like(p, 0.5 + i), "exp_avg_sq": torch.full_like(p, 0.25)}
    src.param_groups[0]["lr"] = 123.0
    stored = TS.optimizer_state(src)
    assert [[None if st is None else sorted(st) for st in rows] for rows in stored] == [[["exp_avg", "exp_avg_sq", "step"]] * 2, [None]]
    assert len(TS.optimizer_tensors(src)) == 4
    dst, dparams = _optimizer()
    dst.state[dparams[2]] = {"step": 1, "exp_avg": torch.ones(2, 2), "exp_avg_sq": torch.ones(2, 2)}      # (dropped by the load)
    TS.load_optimizer_state(dst, stored, "G")
    assert dst.param_groups[0]["lr"] == 1e-3                 # the lr is the scheduler's business
    assert not dst.state.get(dparams[2])
    for i, p in enumerate(dparams[:2]):
        st = dst.state[p]
        assert st["step"] == 7 + i and isinstance(st["step"], int)
        assert torch.equal(st["exp_avg"], torch.full_like(p, 0.5 + i)) and st["exp_avg"].is_contiguous()
        assert st["exp_avg"].data_ptr() != src.state[params[i]]["exp_avg"].data_ptr()
    other, _ = _optimizer(((3, 2), (5,), (2, 2)))
    with pytest.raises(RuntimeError, match="shape"):
        TS.load_optimizer_state(other, stored, "G")
    with pytest.raises(RuntimeError, match="parameters per group"):
        TS.load_optimizer_state(other, stored[:1], "G")


def test_digest_comparison_names_the_file():
    from de_i2i_gan_amd import train_state as TS
    stored = {"net_G": 5, "net_D": 6, "net_G_ema": 7}
    TS.check_digests(stored, {"net_G": 5, "net_D": 6, "ada": 9}, lambda name: f"latest_{name}.pth")      # (one-sided names: skipped)
    with pytest.raises(RuntimeError, match="latest_net_D.pth"):
        TS.check_digests(stored, {"net_G": 5, "net_D": 2 ** 64 - 1}, lambda name: f"latest_{name}.pth")
    assert TS.digests({"a": [], "b": []}) == {}
