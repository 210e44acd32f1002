"""MAETrainer (trainers/mae_trainer.py:13-158): the MAE-GAN pre-training stage -- the documented first stage of the
reference recipe (defectGAN/README.md:6-10).  Per iteration one discriminator update and (every ``num_critics``
iterations) one generator update on the same image batch; each update draws its own shifted patch mask
(``utils/masks.py``), the generator repairs ``MaskToken(imgs, mask)``.

Same kernels as the defectGAN stage (one generator pass per update instead of four).

GradScaler.  The reference wraps both updates in ``torch.cuda.amp.GradScaler`` (base_trainer.py:61, mae_trainer.py:139-158)
although it never enables autocast (defectgan_model.py:54 is commented out): with fp32 gradients, scaling the loss by 2^16
and un-scaling before the update is the identity unless a gradient overflows fp32, and on the CPU -- the path the goldens
come from -- torch disables the scaler altogether.  ``opt.grad_scaler = True`` routes the updates through
``torch.amp.GradScaler`` exactly like the reference's GPU path (one host sync per update for its overflow check); the
default applies the update directly, which is the reference's CPU semantics and keeps the step free of host syncs.
``opt.max_grad_norm`` (global-norm clipping inside the fused Adam, G's norm taken jointly with the mask token's) needs nothing
more under the scaler: ``GradScaler.step`` has un-scaled the gradients before it calls ``FusedAdam.step``, so the norm that is
clipped and logged as ``losses["grad_norm"]`` is that of the un-scaled gradients (an update the scaler skips logs the last norm).
TensorBoard logging, image grids and FID validation are host-side tooling outside the step and are not part of this
package."""
import torch

from .. import ops
from .base_trainer import BaseTrainer


class MAETrainer(BaseTrainer):
    draws_masks = True           # every update draws a patch mask (graph_step captures it only when opt.mask_rng = "device")
    metric_names = ("psnr", "ssim", "l1", "psnr_masked", "clf_acc", "clf_f1")      # (ops.IMAGE_SCORES, then clf_ + ops.CLF_SCORES)

    def __init__(self, opt, data_types=("fusion",)):
        super().__init__(opt)
        assert len(opt.loss_weight) == 3, f"length of loss weights must be 3, not {len(opt.loss_weight)}"
        self.loss_weights = {"rec": opt.loss_weight[0], "clf_D": opt.loss_weight[1], "clf_G": opt.loss_weight[2]}
        self.distill = opt.style_norm_block_type == "sean" and getattr(opt, "style_distill", False)      # mae_trainer.py:20-21
        self._set_loss_types(["rec", "gan", "clf"] + ["distill"] * bool(self.distill))
        self.data_types = data_types
        if opt.phase == "val":
            raise NotImplementedError("phase='val' builds FID metric networks (downloaded weights): out of scope")
        # the mask token is trained by the generator's optimizer (mae_trainer.py:28)
        self.optimizers["G"].add_param_group({"params": list(self.model.mask_token.parameters())})
        device_type = torch.device(opt.device).type
        self.scaler = torch.amp.GradScaler(device_type, enabled=device_type == "cuda" and bool(getattr(opt, "grad_scaler", False)))
        self.resume_train_state()         # (opt.train_state: the mask token's param group and the scaler exist now)

    def _scaled_update(self, loss, name):
        net = self.model.networks[name]
        self.scaler.scale(loss).backward()
        if self.reducer is not None:
            self.reducer.reduce(net)
            if name == "G":
                self.reducer.reduce(self.model.mask_token)
        self.scaler.step(self.optimizers[name])
        self.scaler.update()

    def _train_generator_once(self, data, labels):
        """mae_trainer.py:124-147"""
        self.optimizers["G"].zero_grad()
        with self._bn_scope():
            losses = self.model("mae_generator", data, labels)
        rec_loss, gan_loss, clf_loss = losses[:3]
        g_loss = gan_loss + rec_loss * self.loss_weights["rec"] + clf_loss * self.loss_weights["clf_G"]
        self._scaled_update(g_loss, "G")
        if self.reducer is not None:
            self.reducer.broadcast_buffers(self.model.netG)
        # opt.ema_beta (with grad_scaler, after a skipped optimizer step too: the copies then move towards unchanged weights)
        self.model.update_ema(self.iters)
        norm_keys, norms = self._grad_norm_records("G")
        self._record([("rec", "train"), ("gan", "G"), ("clf", "G")] + norm_keys, [rec_loss, gan_loss, clf_loss] + norms)
        if self.distill and len(losses) == 5:             # (:125-131) logged only
            self._record([("distill", "latent"), ("distill", "embed")], list(losses[3:5]))

    def _train_discriminator_once(self, data, labels):
        """mae_trainer.py:149-158"""
        self.optimizers["D"].zero_grad()
        with self._bn_scope():
            gan_loss, clf_loss = self.model("mae_discriminator", data, labels)
        d_loss = gan_loss + clf_loss * self.loss_weights["clf_D"]
        self._scaled_update(d_loss, "D")
        norm_keys, norms = self._grad_norm_records("D")
        self._record([("gan", "D"), ("clf", "D")] + norm_keys, [gan_loss, clf_loss] + norms)

    # ---- validation ---------------------------------------------------------------------------------------------------------
    def validate(self, loader, max_batches=None):
        """One pass over ``loader`` (it yields ``(images, labels, _)``; at most ``max_batches`` batches) -> {name: float}, each value
        also appended to ``self.metrics[name]``: ``l1``, ``psnr``, ``ssim`` of the repaired image against the original over the whole
        image, ``psnr_masked`` over the pixels the generator had to invent (ops.image_metrics: one fused pass per batch), and
        ``clf_acc`` / ``clf_f1`` of D's classifier on the real images (exact-match rate; macro F1 over the classes with any positive).
        Per batch one no-grad eval pass ``_repair_mask`` of what ``mae_inference`` runs (the EMA copies under ``opt.ema_inference``),
        on masks drawn from validation's own generators seeded by ``opt.val_seed`` (``_validation_scope``): every call sees the same
        masks on the same loader order, so scores compare across epochs.  Everything accumulates on the device; ONE host read at
        the end.  Runs eagerly, keeps captured graphs, and leaves training exactly where it was (``state_digest()``, every RNG state
        and counter, BatchNorm statistics, ``training`` flags, ``iters``).  Under ``attach_ddp`` this is a local call on whatever
        loader the rank passes: no collective."""
        model, device = self.model, self.opt.device
        sums, counts, chw = [], None, None
        with self._validation_scope():
            model.netD.eval()
            model.netG.eval()
            with model._ema_scope():
                for i, (imgs, labels, *_) in enumerate(loader):
                    if max_batches is not None and i >= max_batches:
                        break
                    imgs, labels = imgs.to(device, non_blocking=True), labels.to(device, non_blocking=True)
                    predicted, masks = model._repair_mask(imgs, labels)
                    sums.append(ops.image_metrics(predicted, imgs, mask=1.0 - masks))       # (masks: 1 = kept, 0 = the token's)
                    counts = self._classify(imgs, labels, counts)
                    chw = tuple(imgs.shape[1:])
            if not sums:
                raise ValueError("validate: the loader yielded no batch")
            return self._finish_validation(self.metric_names, [ops.image_scores(torch.cat(sums), chw), ops.clf_scores_dev(counts)])

    def step(self, data, labels):
        """One iteration of the reference's loop (mae_trainer.py:92-99).  ``opt.graph_step``: replayed from a captured graph after
        ``opt.graph_warmup`` eager calls (trainers/graph_step.py); that needs device-drawn masks (``opt.mask_rng = "device"``) and
        refuses ``opt.grad_scaler``."""
        self._step(data, labels)
