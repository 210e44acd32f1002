"""DefectGanTrainer (trainers/defectgan_trainer.py:19-188): the two ``_train_*_once`` methods with the reference's
signatures and side effects, ``step()`` = one D update then (every ``num_critics`` iterations) one G update, and the
epoch loop ``train()`` / ``_train_epoch()`` with the reference's checkpoint / resume behaviour (``latest`` weights and
``iter.txt`` every ``save_latest_freq`` iterations, numbered weights every ``save_ckpt_freq`` epochs, one scheduler step per
epoch).

TensorBoard logging, progress bars, image grids and FID/IS/LPIPS validation are host-side tooling outside the hot path
 and are not part of this package."""
import torch

from .. import ops
from .base_trainer import BaseTrainer


class DefectGanTrainer(BaseTrainer):
    diff_augments = True
    metric_names = ("cyc_psnr", "cyc_ssim", "cyc_df_psnr", "cyc_df_ssim", "clf_acc_real", "clf_f1_real", "clf_acc_fake", "clf_f1_fake")

    def __init__(self, opt):
        super().__init__(opt)
        assert len(opt.loss_weight) == 5, f"length of loss weights must be 5, not {len(opt.loss_weight)}"
        self.loss_weights = {"clf_d": opt.loss_weight[0], "clf_g": opt.loss_weight[1], "rec": opt.loss_weight[2],
                             "sd_cyc": opt.loss_weight[3], "sd_con": opt.loss_weight[4]}
        self.distill = opt.style_norm_block_type == "sean" and getattr(opt, "style_distill", False)      # defectgan_trainer.py:29-30
        # (opt.ada_target: p and r_t after the controller's launch, per D update)
        self._set_loss_types(["gan", "clf", "aux"] + ["distill"] * bool(self.distill), ["ada"] * (self.model.ada is not None))
        if opt.phase == "val":
            raise NotImplementedError("phase='val' builds FID/LPIPS metric networks (downloaded weights): out of scope")
        self.resume_train_state()         # (opt.train_state: the optimizers exist now)

    # ---- the step ---------------------------------------------------------------------------------------------
    def _train_generator_once(self, bg_data, df_labels, df_data):
        """defectgan_trainer.py:138-168"""
        self.optimizers["G"].zero_grad()
        with_e = "E" in self.optimizers                  # adain: the StyleExtractor is trained by the G loss (:140-141,161-163)
        if with_e:
            self.optimizers["E"].zero_grad()
        with self._bn_scope():
            losses = self.model("generator", bg_data, df_labels, df_data)
        gan_loss, clf_loss, rec_loss, sd_cyc_loss, sd_con_loss = losses[:5]
        g_loss = gan_loss + clf_loss * self.loss_weights["clf_g"] + rec_loss * self.loss_weights["rec"] + \
            sd_cyc_loss * self.loss_weights["sd_cyc"] + sd_con_loss * self.loss_weights["sd_con"]
        g_loss.backward()
        if self.reducer is not None:
            self.reducer.reduce(self.model.netG)
            if with_e:
                self.reducer.reduce(self.model.netE)
        self.optimizers["G"].step()
        if with_e:
            self.optimizers["E"].step()
        if self.reducer is not None:
            self.reducer.broadcast_buffers(self.model.netG)      # BatchNorm running stats follow rank 0 (sync_bn: equal already)
        # opt.ema_beta: no collective -- every rank applies one function to equal parameters and to buffers already synchronised
        self.model.update_ema(self.iters)
        norm_keys, norms = self._grad_norm_records(*(("G", "E") if with_e else ("G",)))
        self._record([("gan", "G"), ("clf", "G"), ("aux", "rec"), ("aux", "cyc"), ("aux", "con")] + norm_keys,
                     [gan_loss, clf_loss, rec_loss, sd_cyc_loss, sd_con_loss] + norms)
        if self.distill:                                  # (:142-146) logged; the gradients were taken inside the SEAN layers
            self._record([("distill", "latent"), ("distill", "embed")], list(losses[5:7]))

    def _train_discriminator_once(self, bg_data, df_labels, df_data):
        """defectgan_trainer.py:170-180"""
        self.optimizers["D"].zero_grad()
        with self._bn_scope():
            gan_loss, clf_loss = self.model("discriminator", bg_data, df_labels, df_data)
        d_loss = gan_loss + clf_loss * self.loss_weights["clf_d"]
        d_loss.backward()
        if self.reducer is not None:
            self.reducer.reduce(self.model.netD)
        self.optimizers["D"].step()
        norm_keys, norms = self._grad_norm_records("D")
        ada = self.model.ada
        if ada is not None:                               # read from device memory like a loss (deferred, or by the replay)
            norm_keys, norms = norm_keys + [("ada", "p"), ("ada", "rt")], norms + [ada.p[0], ada.rt[0]]
        self._record([("gan", "D"), ("clf", "D")] + norm_keys, [gan_loss, clf_loss] + norms)

    def step(self, bg_data, df_labels, df_data):
        """One iteration of the reference's hot loop (defectgan_trainer.py:96-109).  ``opt.graph_step``: replayed from a
        captured graph after ``opt.graph_warmup`` eager calls (trainers/graph_step.py)."""
        self._step(bg_data, df_labels, df_data)

    # ---- the epoch loop with the reference's checkpoint / resume rules (defectgan_trainer.py:75-120) -------------------
    def train(self, train_loaders, val_loaders=None):
        """Epochs ``first_epoch .. num_epochs`` (1-based, like the reference): ``train_loaders['defects']`` is iterated once
        per epoch, ``train_loaders['background']`` is an (infinite) iterator drawn with ``next`` -- both yield
        ``(images, labels, _)``.  ``opt.val_freq = E`` (> 0): after every E-th epoch ``validate(val_loaders, opt.val_max_batches)``
        runs (``val_loaders``: the same two keys; required then) and, with ``opt.save_best``, ``maybe_save_best(epoch)``; without it
        ``val_loaders`` is not read."""
        val_freq = self.val_opts["val_freq"]
        if val_freq > 0 and val_loaders is None:
            raise ValueError(f"val_freq={val_freq} validates every {val_freq} epoch(s): train() needs val_loaders")
        for epoch in range(self.first_epoch, self.opt.num_epochs + 1):
            self._init_losses()
            self._train_epoch(train_loaders, epoch)
            if epoch % getattr(self.opt, "save_ckpt_freq", 10 ** 9) == 0:
                self.save_checkpoint(epoch, epoch)
            if val_freq > 0 and epoch % val_freq == 0:
                self.validate(val_loaders, self.val_opts["val_max_batches"])
                self.maybe_save_best(epoch)
            self._update_per_epoch(epoch)

    # ---- validation ---------------------------------------------------------------------------------------------------------
    def validate(self, loaders, max_batches=None):
        """One pass over ``loaders`` (the ``defects`` / ``background`` shape of ``train_loaders``; at most ``max_batches`` batches) ->
        {name: float}, each value also appended to ``self.metrics[name]``.  Per batch ``(bg, df, df_labels)``, every generator pass
        through ``model("inference", ...)`` (the EMA copies under ``opt.ema_inference``; SPADE, AdaIN and SEAN alike):
          ``fake_df = G(bg, df_labels)``, ``restored = G(fake_df, normal_labels)``: ``cyc_psnr`` / ``cyc_ssim`` of restored vs bg;
          the mirror image df -> normal -> df_labels against df: ``cyc_df_psnr`` / ``cyc_df_ssim`` (ops.image_metrics);
          ``clf_acc_real`` / ``clf_f1_real``: D's classifier on df against df_labels (exact-match rate; macro F1 over the classes with
          any positive); ``clf_acc_fake`` / ``clf_f1_fake``: the same on fake_df -- does it find the defect that was asked for?
        Every draw (NoiseInjection, SEAN's ``random.choices`` or its device draws) comes from validation's own generators seeded by
        ``opt.val_seed`` (``_validation_scope``), so scores compare across epochs.  Everything accumulates on the device; ONE host
        read at the end.  Runs eagerly, keeps captured graphs, and leaves training exactly where it was (``state_digest()``, every
        RNG state and counter, BatchNorm statistics, ``training`` flags, ``iters``).  Under ``attach_ddp`` this is a local call on
        whatever loaders the rank passes: no collective."""
        model, device = self.model, self.opt.device
        cyc, cyc_df, real, fake, chw = [], [], None, None, None
        with self._validation_scope():
            for i, (df, df_labels, *_) in enumerate(loaders["defects"]):
                if max_batches is not None and i >= max_batches:
                    break
                bg = next(loaders["background"])[0][:df.size(0)]
                bg, df, df_labels = (t.to(device, non_blocking=True) for t in (bg, df, df_labels))
                nm_labels = torch.zeros_like(df_labels)
                nm_labels[:, 0] = 1
                fake_df = model("inference", bg, df_labels)[0]
                restored = model("inference", fake_df, nm_labels)[0]
                fake_nm = model("inference", df, nm_labels)[0]
                recovered = model("inference", fake_nm, df_labels)[0]
                cyc.append(ops.image_metrics(restored, bg))
                cyc_df.append(ops.image_metrics(recovered, df))
                real = self._classify(df, df_labels, real)
                fake = self._classify(fake_df, df_labels, fake)
                chw = tuple(bg.shape[1:])
            if not cyc:
                raise ValueError("validate: the loaders yielded no batch")
            scores = [ops.image_scores(torch.cat(cyc), chw)[:2], ops.image_scores(torch.cat(cyc_df), chw)[:2],
                      ops.clf_scores_dev(real), ops.clf_scores_dev(fake)]
            return self._finish_validation(self.metric_names, scores)

    def _train_epoch(self, data_loaders, epoch):
        for df_data, df_labels, _ in data_loaders["defects"]:
            bg_data, bg_labels, _ = next(data_loaders["background"])
            bg_data = bg_data[:df_data.size(0)]            # truncate to the defect batch (defectgan_trainer.py:102-105)
            self.step(bg_data, df_labels, df_data)
            if self.iters % self.opt.save_latest_freq == 0:
                self.save_latest(epoch)
