"""opt.clf_loss_type = "cce" (and "mse") through the model, both trainers and graph capture.

The classifier head's loss is the only thing that changes against the "bce" runs the neighbouring files pin, so every bound here is
the one its neighbour applies to the same quantity:
  * D step, f32, against float64: losses 1e-5 absolute, every D parameter gradient 1e-4 relative L2, on replayed LeakyReLU branches
    (test_model_gpu.py::test_step_gradients_match_oracle_fp64).  The float64 reference is composed here from the oracle's pieces the
    way its discriminator_losses composes them, with F.cross_entropy for the two classifier terms;
  * G step, f32: clf_loss 1e-5 absolute against the same composition; the paired (`whole`) branch against the split one
    |a - b| <= 1e-5 * max(|b|, 1e-3) (test_fused_norm_gpu.py::test_paired_generator_passes_equal_the_four_passes);
  * trainer steps and graph replays: bits (test_graph_step_gpu.py, test_graph_mae_gpu.py -- their builders and comparison are used
    as they are)."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_graph_mae_gpu as GM
import test_graph_step_gpu as GS
from helpers import formula_fill, make_opt, record_kinks, unbatch_discriminator
from oracle import defectgan_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)          # the t0_img32_b2 configuration
SMALL = GS.SMALL


def note(*a):
    print("[clf-step]", *a, flush=True)


def build_t0(**over):
    from de_i2i_gan_amd import ops
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    ops.noise_source = None
    tr = DefectGanTrainer(make_opt(T0, DEV, "f32", **over))
    formula_fill(tr.model.netG)
    formula_fill(tr.model.netD)
    return tr


def oracle_states(cfg):
    SG = {k: (v.double() if v.is_floating_point() else v) for k, v in O.make_state(O.generator_state_shapes(cfg)).items()}
    SD = {k: v.double() for k, v in O.make_state(O.discriminator_state_shapes(cfg)).items()}
    return SG, SD


def cce64(logits, labels):
    n = logits.shape[0]
    return F.cross_entropy(logits.reshape(n, -1), labels.reshape(n, -1))


def d_losses_cce(SG, SD, bg, labels, df, cfg):
    """oracle.discriminator_losses with the classifier terms as cross entropy"""
    nm_l, df_l = O._labels(labels)
    with torch.no_grad():
        fake_defects, _ = O.generator_forward(SG, bg, df_l, cfg, training=False, style_feat=None)
        fake_normals, _ = O.generator_forward(SG, df, nm_l, cfg, training=False, style_feat=None)
    fd_src, _ = O.discriminator_forward(SD, fake_defects, cfg, training=True)
    fn_src, _ = O.discriminator_forward(SD, fake_normals, cfg, training=True)
    rd_src, rd_cls = O.discriminator_forward(SD, df, cfg, training=True)
    rn_src, rn_cls = O.discriminator_forward(SD, bg, cfg, training=True)
    ones, zeros = torch.ones_like(rd_src), torch.zeros_like(fd_src)
    gan = torch.stack([O.bce_logits(fd_src, zeros), O.bce_logits(fn_src, zeros), O.bce_logits(rd_src, ones), O.bce_logits(rn_src, ones)]).mean()
    clf = torch.stack([cce64(rd_cls, df_l), cce64(rn_cls, nm_l)]).mean()
    return gan, clf


def g_clf_cce(SG, SD, bg, labels, df, cfg):
    """the clf term of oracle.generator_losses as cross entropy: it reads the two chain heads only (training-mode BatchNorm takes
    batch statistics, so the recover passes in between change nothing it sees).  SG's running statistics are updated: pass a copy."""
    nm_l, df_l = O._labels(labels)
    with torch.no_grad():
        fake_defects, _ = O.generator_forward(SG, bg, df_l, cfg, training=True, style_feat=None)
        fake_normals, _ = O.generator_forward(SG, df, nm_l, cfg, training=True, style_feat=None)
        _, fd_cls = O.discriminator_forward(SD, fake_defects, cfg)
        _, fn_cls = O.discriminator_forward(SD, fake_normals, cfg)
        return torch.stack([cce64(fd_cls, df_l), cce64(fn_cls, nm_l)]).mean()


def test_d_step_cce_matches_float64():
    cfg = O.Cfg(image_size=T0["image_size"], ngf=T0["ngf"], ndf=T0["ndf"], num_layers=T0["num_layers"], hidden_nc=T0["hidden_nc"])
    bg, labels, df = O.synthetic_batch(T0["batch"], T0["image_size"])
    assert bool(((labels == 0) | (labels == 1)).all()) and bool((labels.sum(1) == 1).all())      # one-hot rows
    SG, SD = oracle_states(cfg)
    tr = build_t0(clf_loss_type="cce")
    with record_kinks() as tape:
        gan, clf = tr.model("discriminator", bg, labels, df)
    (gan + 2 * clf).backward()
    decisions = unbatch_discriminator(tape, 4, T0["batch"])       # product: one D pass over 4 batches; oracle: 4 passes
    for k in O.param_keys(SD):
        SD[k].requires_grad_(True)
    O.KINK_TAPE = kt = O.KinkTape(decisions)
    try:
        gan64, clf64 = d_losses_cce(SG, SD, bg.double(), labels.double(), df.double(), cfg)
    finally:
        O.KINK_TAPE = None
    assert kt.exhausted() and kt.sites == len(decisions) and kt.worst < 2e-3, (kt.flips, kt.worst)
    gD = O._grads(gan64 + 2 * clf64, SD)
    note(f"D step cce: gan {float(gan):.7f} vs {float(gan64):.7f}  clf {float(clf):.7f} vs {float(clf64):.7f}")
    assert abs(float(gan) - float(gan64)) < 1e-5 and abs(float(clf) - float(clf64)) < 1e-5
    worst = 0.0
    for k, p in tr.model.netD.named_parameters():
        e = ((p.grad.double().cpu() - gD[k]).norm() / gD[k].norm()).item()
        worst = max(worst, e)
        assert e < 1e-4, (k, e)
    note(f"D step cce: worst parameter gradient error {worst:.3e} (bound 1e-4)")
    tr_bce = build_t0()                         # bce gives another number: a model that ignored clf_loss_type would be noticed
    _, clf_bce = tr_bce.model("discriminator", bg, labels, df)
    assert abs(float(clf_bce) - float(clf)) > 1e-3


def test_g_step_cce_clf_loss_and_the_paired_branch():
    from de_i2i_gan_amd import ops
    cfg = O.Cfg(image_size=T0["image_size"], ngf=T0["ngf"], ndf=T0["ndf"], num_layers=T0["num_layers"], hidden_nc=T0["hidden_nc"])
    bg, labels, df = O.synthetic_batch(T0["batch"], T0["image_size"])
    SG, SD = oracle_states(cfg)
    ref = float(g_clf_cce({k: v.clone() for k, v in SG.items()}, SD, bg.double(), labels.double(), df.double(), cfg))
    got = {}
    keep = ops.paired_passes
    try:
        for paired in (True, False):
            ops.paired_passes = paired
            tr = build_t0(clf_loss_type="cce")
            assert bool(tr.model._pairs_generator_passes(bg.to(DEV), df.to(DEV), None)) == paired
            ls = tr.model("generator", bg, labels, df)
            (ls[0] + 5 * ls[1] + 5 * ls[2] + 5 * ls[3] + ls[4]).backward()          # the backward kernel runs on both branches
            assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in tr.model.netG.parameters())
            got[paired] = [float(v) for v in ls]
    finally:
        ops.paired_passes = keep
    note(f"G step cce clf_loss: paired {got[True][1]:.7f} split {got[False][1]:.7f} float64 {ref:.7f}")
    assert abs(got[True][1] - ref) < 1e-5 and abs(got[False][1] - ref) < 1e-5
    for a, b in zip(got[True], got[False]):
        assert abs(a - b) <= 1e-5 * max(abs(b), 1e-3), (got[True], got[False])


def _finite(losses):
    vals = [v for d in losses.values() for series in d.values() for v in series]
    return len(vals) > 0 and all(math.isfinite(v) for v in vals)


def _two_steps(mod, kind, **over):
    """mod: test_graph_step_gpu (DefectGanTrainer) or test_graph_mae_gpu (MAETrainer) -- their seeded builder, batches and snapshot"""
    tr = mod.build(SMALL, "bf16", clf_loss_type=kind, **over)
    for _ in mod.run(tr, SMALL, 2):
        pass
    return mod.snapshot(tr)


@pytest.mark.parametrize("kind", ["cce", "mse"])
def test_defectgan_trainer_steps(kind):
    """DefectGanTrainer.step() x 2 in bf16: finite losses, a classifier loss that is not the bce run's, and the same bits from a
    second fresh trainer."""
    a, b, bce = _two_steps(GS, kind), _two_steps(GS, kind), _two_steps(GS, "bce")
    assert _finite(a["losses"]) and len(a["losses"]["clf"]["D"]) == 2 and len(a["losses"]["clf"]["G"]) == 2
    GS.assert_same(a, b, f"{kind}: two fresh trainers")
    note(f"defectgan {kind}: clf D {a['losses']['clf']['D']} vs bce {bce['losses']['clf']['D']}")
    assert a["losses"]["clf"]["D"][0] != bce["losses"]["clf"]["D"][0] and a["losses"]["clf"]["G"][0] != bce["losses"]["clf"]["G"][0]


def test_mae_trainer_steps_cce():
    masks = dict(mask_rng="device", mask_seed=GM.SEED)
    a, b, bce = _two_steps(GM, "cce", **masks), _two_steps(GM, "cce", **masks), _two_steps(GM, "bce", **masks)
    assert _finite(a["losses"]) and len(a["losses"]["clf"]["D"]) == 2 and len(a["losses"]["clf"]["G"]) == 2
    GM.assert_same(a, b, "cce: two fresh trainers")
    note(f"mae cce: clf D {a['losses']['clf']['D']} vs bce {bce['losses']['clf']['D']}")
    assert a["losses"]["clf"]["D"][0] != bce["losses"]["clf"]["D"][0] and a["losses"]["clf"]["G"][0] != bce["losses"]["clf"]["G"][0]


def test_graph_step_cce_defectgan():
    """warm-up (3 eager calls), capture and replays: over 6 steps every loss, parameter, buffer and Adam moment equals the eager run's"""
    GS.compare(SMALL, steps=6, clf_loss_type="cce")


def test_graph_step_cce_mae_device_masks():
    GM.compare(SMALL, steps=6, clf_loss_type="cce")
