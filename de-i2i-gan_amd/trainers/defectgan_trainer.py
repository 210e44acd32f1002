"""DefectGanTrainer (trainers/defectgan_trainer.py:19-188): the two ``_train_*_once`` methods with the reference's
signatures and side effects, ``step()`` = one D update then (every ``num_critics`` iterations) one G update, and the
epoch loop ``train()`` / ``_train_epoch()`` with the reference's checkpoint / resume behaviour (``latest`` weights and
``iter.txt`` every ``save_latest_freq`` iterations, numbered weights every ``save_ckpt_freq`` epochs, one scheduler step per
epoch).

TensorBoard logging, progress bars, image grids and FID/IS/LPIPS validation are host-side tooling outside the hot path
 and are not part of this package."""
from .base_trainer import BaseTrainer


class DefectGanTrainer(BaseTrainer):
    diff_augments = True

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
        ``(images, labels, _)``.  ``val_loaders`` is accepted for signature compatibility (metrics are out of scope)."""
        for epoch in range(self.first_epoch, self.opt.num_epochs + 1):
            self._init_losses()
            self._train_epoch(train_loaders, epoch)
            if epoch % getattr(self.opt, "save_ckpt_freq", 10 ** 9) == 0:
                self.save_checkpoint(epoch, epoch)
            self._update_per_epoch(epoch)

    def _train_epoch(self, data_loaders, epoch):
        for df_data, df_labels, _ in data_loaders["defects"]:
            bg_data, bg_labels, _ = next(data_loaders["background"])
            bg_data = bg_data[:df_data.size(0)]            # truncate to the defect batch (defectgan_trainer.py:102-105)
            self.step(bg_data, df_labels, df_data)
            if self.iters % self.opt.save_latest_freq == 0:
                self.save_latest(epoch)
