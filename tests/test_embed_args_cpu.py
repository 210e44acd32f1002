"""CPU: the numpy reference of the device-drawn SEAN style embeddings (tests/embed_reference.py) on its own -- the Random123 known
answer and the frequencies of its indices --, what ``opt.embed_rng`` accepts and refuses before anything is built, the doors it
opens in ``train_state_option`` and ``graph_step.unsupported``, and the packing rules of ``ops.embed_pack`` (the host half of
``ops.EmbedBank``).  No kernel is launched here."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import embed_reference as R

SEED = 0x5DEECE66D1234567
CUDA = torch.device("cuda:0")


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_philox_reproduces_a_random123_known_answer():
    got = R.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
    assert tuple(int(v) for v in got) == (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def _indices(count, num_embeds):
    """calls 0..63, rows 0..15, every row the one combination whose list holds ``count`` embeddings at offset 0"""
    labels = np.zeros((16, 1), dtype=np.float32)
    table = np.array([[0, count], [0, 0]])
    return np.concatenate([R.draw_index(SEED, call, labels, table, num_embeds).ravel() for call in range(64)])


@pytest.mark.parametrize("count,num_embeds,draws", [(3, 4, 4096), (7, 5, 5120)])
def test_every_index_is_drawn_as_often_as_a_uniform_draw_gives(count, num_embeds, draws):
    """each index's frequency within 4 sigma of n / count, sigma = sqrt(n p (1 - p)) (the reference gives 0.33 and 1.06 sigma)"""
    index = _indices(count, num_embeds)
    assert index.shape == (draws,) and index.min() >= 0 and index.max() < count
    p = 1.0 / count
    sigma = np.sqrt(draws * p * (1 - p))
    freq = np.bincount(index, minlength=count)
    worst = np.abs(freq - draws * p).max() / sigma
    print(f"count {count}: worst deviation {worst:.2f} sigma")
    assert worst < 4.0, (freq.tolist(), worst)


def test_a_long_list_is_indexed_inside_its_bounds():
    index = _indices(1000, 9)
    assert index.shape == (64 * 16 * 9,) and index.min() >= 0 and index.max() < 1000
    assert len(np.unique(index)) > 900                      # (9216 draws from 1000: all but a handful are hit)


def test_reference_label_rules():
    labels = np.array([[0, 0, 1], [1, 0, 0], [1, 1, 1], [0, 2, 0], [0, -1, 0], [0.5, 1.9, -0.5], [np.nan, 0, 0]], dtype=np.float32)
    combo, valid = R.combinations(labels)
    assert valid.tolist() == [True, True, True, False, False, True, False]
    assert combo[valid].tolist() == [1, 4, 7, 2]              # the first label is the slowest digit; (int) truncates toward zero
    table = np.zeros((8, 2), dtype=np.int64)
    table[1], table[4] = (0, 2), (2, 5)
    index = R.draw_index(SEED, 0, labels, table, 3)
    assert ((0 <= index[0]) & (index[0] < 2)).all() and ((2 <= index[1]) & (index[1] < 7)).all()
    assert (index[2:] == -1).all()                           # an empty list, and the invalid rows
    part = R.draw_index(SEED, 0, labels[1:3], table, 3, row0=1)
    assert np.array_equal(part, index[1:3])                  # rows are a slice of the whole batch's draw
    assert not np.array_equal(R.draw_index(SEED, 1, labels, table, 3)[:2], index[:2])


# ---- opt.embed_rng ---------------------------------------------------------------------------------------------------------
def _opt(**kw):
    return SimpleNamespace(**{"device": CUDA, "style_norm_block_type": "sean", "sean_alpha": None, **kw})


def test_embed_rng_option_values_and_requirements():
    from de_i2i_gan_amd.models.defectgan_model import embed_rng_option
    assert embed_rng_option(_opt()) == "host" and embed_rng_option(_opt(embed_rng=None)) == "host"
    assert embed_rng_option(_opt(embed_rng="host", style_norm_block_type="spade", device=torch.device("cpu"))) == "host"
    assert embed_rng_option(_opt(embed_rng="device")) == "device" and embed_rng_option(_opt(embed_rng="device", sean_alpha=1.0)) == "device"
    with pytest.raises(ValueError, match="embed_rng gpu"):
        embed_rng_option(_opt(embed_rng="gpu"))
    with pytest.raises(ValueError, match="opt.device is cpu"):
        embed_rng_option(_opt(embed_rng="device", device=torch.device("cpu")))
    with pytest.raises(ValueError, match="style_norm_block_type is 'spade'"):
        embed_rng_option(_opt(embed_rng="device", style_norm_block_type="spade"))
    with pytest.raises(ValueError, match="sean_alpha=0"):
        embed_rng_option(_opt(embed_rng="device", sean_alpha=0))


def test_the_model_refuses_before_it_builds_its_networks(monkeypatch):
    from helpers import make_opt
    from de_i2i_gan_amd.models import defectgan_model as M

    def no_net(opt):
        raise AssertionError("a network was built")
    monkeypatch.setattr(M, "DefectGanGenerator", no_net)
    c = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)
    for over in (dict(embed_rng="device", style_norm_block_type="sean", sean_alpha=1.0),          # (a CPU device)
                 dict(embed_rng="device"), dict(embed_rng="gpu", style_norm_block_type="sean")):
        with pytest.raises(ValueError, match="embed_rng"):
            M.DefectGanModel(make_opt(c, "cpu", **over))


def test_host_draws_build_the_model_they_always_built(tmp_path):
    from helpers import make_opt
    from de_i2i_gan_amd.models.defectgan_model import DefectGanModel
    from oracle import defectgan_oracle as O
    c = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)
    cfg = O.Cfg(image_size=32, ngf=8, ndf=8, num_layers=3, hidden_nc=16, style_norm="sean", embed_nc=8, num_embeds=3)
    path = tmp_path / "embeds.pth"
    torch.save(O.synthetic_embeddings(cfg), path)
    for over in (dict(), dict(embed_rng=None), dict(embed_rng="host")):
        model = DefectGanModel(make_opt(c, "cpu", style_norm_block_type="sean", sean_alpha=1.0, embed_nc=8, num_embeds=3, embed_path=path,
                                        **over))
        assert model.embed_rng is None and model.embed_bank is None and model.embed_ranks is None
        assert len(model.embeddings) == 64 and len(model.embeddings[(0, 1, 0, 0, 0, 0)]) == 3
    plain = DefectGanModel(make_opt(c, "cpu"))
    assert plain.embed_rng is None and plain.embed_bank is None and not hasattr(plain, "embeddings")


# ---- the doors -------------------------------------------------------------------------------------------------------------
def _ts(**kw):
    from de_i2i_gan_amd import train_state as TS
    return TS.train_state_option(SimpleNamespace(**{"device": CUDA, "style_norm_block_type": "sean", "train_state": True, **kw}))


def test_train_state_takes_sean_with_device_draws_only():
    assert _ts(embed_rng="device") is True
    assert _ts(embed_rng="device", style_distill=True) is True        # (no host state between steps)
    assert _ts(embed_rng="device", use_running_stats=False) is True
    for kw in (dict(), dict(embed_rng=None), dict(embed_rng="host")):
        with pytest.raises(NotImplementedError, match="sean.*random.choices"):
            _ts(**kw)
    with pytest.raises(NotImplementedError, match="use_running_stats"):
        _ts(embed_rng="device", use_running_stats=True)
    with pytest.raises(ValueError, match="GPU"):
        _ts(embed_rng="device", device=torch.device("cpu"))
    assert _ts(train_state=False) is False and _ts(train_state=None, use_running_stats=True) is False


def _stub_trainer(bank=None, **kw):
    from de_i2i_gan_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.zeros(1))
    opt = SimpleNamespace(**{"device": CUDA, "style_norm_block_type": "sean", "sean_alpha": None, "diff_aug": "", "compute_dtype": "bf16",
                             "optimizer": "adam", **kw})
    model = SimpleNamespace(embed_bank=bank, mask_rng=None, diffaug_rng=None)
    return SimpleNamespace(opt=opt, model=model, optimizers={"G": FusedAdam([p], lr=1e-3)}, reducer=None, scaler=None)


def test_graph_step_takes_sean_with_a_bank_only():
    from de_i2i_gan_amd.trainers.graph_step import unsupported
    bank = object()
    assert unsupported(_stub_trainer(bank)) is None
    why = unsupported(_stub_trainer(None))
    assert "random.choices" in why and "embed_rng='device'" in why
    assert "use_running_stats" in unsupported(_stub_trainer(bank, use_running_stats=True))
    assert "use_running_stats" in unsupported(_stub_trainer(None, use_running_stats=True))
    why = unsupported(_stub_trainer(bank, style_distill=True))
    assert "style_distill" in why and "random.choices" not in why
    assert "adain" in unsupported(_stub_trainer(bank, style_norm_block_type="adain"))
    assert unsupported(_stub_trainer(None, style_norm_block_type="spade")) is None
    mae = _stub_trainer(bank)
    mae.draws_masks = True
    assert "mask_rng" in unsupported(mae)
    mae.model.mask_rng = object()
    assert unsupported(mae) is None


# ---- the packing rules -----------------------------------------------------------------------------------------------------
def _file(label_nc=3, embed_nc=4):
    """lists of 2, 0 and 3 embeddings, written in an order that is not the combination order; integer values, all distinct"""
    rows = torch.arange(5 * embed_nc, dtype=torch.float32).reshape(5, embed_nc)
    return {(1, 1, 0): [rows[0], rows[1]], (0, 1, 0): [], (0, 0, 1): [rows[2], rows[3], rows[4]]}


def test_pack_lays_the_lists_out_by_combination_index():
    from de_i2i_gan_amd import ops
    emb = _file()
    bank, table = ops.embed_pack(emb, 3, 4)
    assert bank.dtype == torch.float32 and tuple(bank.shape) == (5, 4) and table.dtype == torch.int32 and tuple(table.shape) == (8, 2)
    want = torch.zeros(8, 2, dtype=torch.int32)
    want[1], want[6] = torch.tensor([0, 3]), torch.tensor([3, 2])                    # (0,0,1) = 1 comes first, (1,1,0) = 6 after it
    assert torch.equal(table, want)
    assert torch.equal(bank, torch.stack(emb[(0, 0, 1)] + emb[(1, 1, 0)]))           # list order kept inside a combination
    ref_bank, ref_table = R.pack({k: [e.numpy() for e in v] for k, v in emb.items()}, 3, 4)
    assert np.array_equal(bank.numpy(), ref_bank) and np.array_equal(table.numpy(), ref_table)
    empty_bank, empty_table = ops.embed_pack({(0, 1): []}, 2, 4)
    assert tuple(empty_bank.shape) == (0, 4) and not empty_table.any()


def test_pack_matches_the_synthetic_embeddings_file():
    from de_i2i_gan_amd import ops
    from oracle import defectgan_oracle as O
    cfg = O.Cfg(image_size=32, ngf=8, ndf=8, num_layers=3, hidden_nc=16, style_norm="sean", embed_nc=8, num_embeds=3)
    emb = O.synthetic_embeddings(cfg)
    bank, table = ops.embed_pack(emb, 6, 8)
    assert tuple(bank.shape) == (3 * (6 + 15), 8) and int(table[:, 1].sum()) == bank.shape[0]
    for combo, key in enumerate(O.multilabel_combinations(6)):
        off, cnt = table[combo].tolist()
        assert cnt == len(emb[key])
        for j, e in enumerate(emb[key]):
            assert torch.equal(bank[off + j], e)


@pytest.mark.parametrize("bad,names", [
    ({(0, 1): [torch.zeros(4)]}, r"\(0, 1\)"),                                        # a key of another length
    ({(0, 1, 0, 1): []}, r"\(0, 1, 0, 1\)"),
    ({(0, 2, 0): []}, r"\(0, 2, 0\)"),                                                # a label that is no bit
    ({"010": []}, "010"),
    ({(0, 1, 0): [torch.zeros(4), torch.zeros(5)]}, r"embedding 1 of key \(0, 1, 0\)"),      # another shape
    ({(0, 1, 0): [torch.zeros(1, 4)]}, r"\(0, 1, 0\)"),
    ({(0, 1, 0): [torch.zeros(4, dtype=torch.float64)]}, r"\(0, 1, 0\).*float64"),    # another dtype
    ({(0, 1, 0): [[0.0, 0.0, 0.0, 0.0]]}, r"\(0, 1, 0\).*list"),
])
def test_pack_refuses_and_names_the_key(bad, names):
    from de_i2i_gan_amd import ops
    with pytest.raises(ValueError, match=names):
        ops.embed_pack(bad, 3, 4)


def test_pack_refuses_more_than_16_labels_and_the_bank_a_cpu_device():
    from de_i2i_gan_amd import ops
    with pytest.raises(ValueError, match="label_nc 17"):
        ops.embed_pack({}, 17, 4)
    with pytest.raises(ValueError, match="label_nc 0"):
        ops.embed_pack({}, 0, 4)
    assert tuple(ops.embed_pack({}, 16, 4)[1].shape) == (65536, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.EmbedBank(_file(), 3, 4, 1, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.embed_draw(SimpleNamespace(device=CUDA), torch.zeros(2, 3), 4)
