"""BaseTrainer (trainers/base_trainer.py:12-131): model creation, one optimizer + one LR scheduler per network."""
import contextlib
import math
from collections import defaultdict

import numpy as np
import torch
from torch import optim

from .. import ops
from .. import train_state as TS
from ..models import create_model
from ..networks import tensors_dropped_on_load
from ..optim import (LOWER_IS_BETTER, FusedAdam, FusedRMSprop, FusedSGD, ada_options, clip_options, ema_options,
                     validation_options)


# opt.optimizer -> keyword arguments of the fused optimizer (the reference builds torch.optim.Adam(betas=(0.5, 0.999)) /
# torch.optim.AdamW(betas=(0.9, 0.95)) with AdamW's default weight decay: trainers/base_trainer.py:75-80)
_OPTIMIZER_ARGS = {
    "adam": {"betas": (0.5, 0.999)},
    "adamw": {"betas": (0.9, 0.95), "weight_decay": 1e-2},
}
_STEP_LR_STAGES = 4          # 'step' schedule: lr_decay is reached after four equal stages (base_trainer.py:94-98)


class BaseTrainer:
    """Same attributes and resume rules as the reference's BaseTrainer (trainers/base_trainer.py:12-131): ``model``,
    ``losses`` / ``dis_outputs`` (dict of lists), ``iters`` / ``first_epoch`` (restored from ``iter.txt`` when continuing),
    ``optimizers`` / ``schedulers`` keyed by network name; the schedulers are stepped ``first_epoch`` times at construction
    like the reference does."""
    diff_augments = False        # whether the trainer's stage applies opt.diff_aug (optim.ada_options)
    metric_names = ()            # what the stage's validate() returns (optim.validation_options: opt.save_best names one of them)

    def __init__(self, opt):
        self.opt = opt
        ema_options(opt)                  # (an invalid opt.ema_beta is refused before anything is built)
        # opt.train_state: every save also writes <epoch>_train_state.pth (optimizers, GradScaler, RNG states, the digests of the
        # sibling files) and a resume restores it, so that a stopped and continued run is the uninterrupted run bit for bit
        self.train_state = TS.train_state_option(opt)
        self.train_state_restored = None  # True: resumed from a train-state file; False: from weights only; None: no resume asked
        # opt.max_grad_norm > 0: every FusedAdam clips its gradients to this global L2 norm inside the update (optim.FusedAdam)
        self.max_grad_norm = clip_options(opt)
        # opt.diff_aug_p / opt.ada_target: gated DiffAugment and its controller (the defectGAN stage; refused elsewhere, and an
        # invalid combination before anything is built)
        self.ada_opts = ada_options(opt, diffaug_stage=self.diff_augments)
        # opt.val_freq / val_max_batches / val_seed / save_best: the validation pass (validate()), its hook in train() and the "best"
        # checkpoint -- an invalid value or a metric this stage does not have is refused before anything is built
        self.val_opts = validation_options(opt, self.metric_names)
        self.best = None                  # (epoch, iters, value) of the "best" checkpoint
        self.model = create_model(opt)
        # opt.ema_beta > 0: the EMA copies of what the G optimizer trains start from the weights just initialised or restored
        self.model.create_ema(self._restore_or_init_weights(opt))
        self.losses, self.dis_outputs = defaultdict(list), defaultdict(list)
        self.metrics = defaultdict(list)  # {metric name: one value per validate() call}
        self._resume_progress(opt)
        best_path = opt.ckpt_dir / opt.name / "best.txt"
        if opt.continue_training and self.val_opts["save_best"] and best_path.exists():      # (a continued run keeps its best so far)
            epoch, iters, value = best_path.read_text().strip().split(",")
            self.best = (int(epoch), int(iters), float(value))
        self._init_lr(opt)
        self._create_optimizer(opt)
        self._create_scheduler(opt)
        # defer_loss_sync: keep the per-step losses on the device and convert them in one batch in flush_losses()
        # instead of the reference's .item() per loss (one host sync each, defectgan_trainer.py:164-168,179-180)
        self.defer_loss_sync = bool(getattr(opt, "defer_loss_sync", False))
        self._pending = []
        # graph_step (trainers/graph_step.py): replay the step from captured graphs after graph_warmup eager calls (opt-in)
        self.graph_step = bool(getattr(opt, "graph_step", False))
        self.graph_warmup = int(getattr(opt, "graph_warmup", 3))
        self._graphs = None
        self._graph_records = None        # (keys, stacked losses) of the step being captured
        self.reducer = None               # set by parallel.attach_ddp(): gradient all-reduce across ranks

    def _restore_or_init_weights(self, opt):
        """-> the checkpoint epoch the weights were restored from (None: initialised)"""
        if opt.continue_training:
            self.model.load("latest")
            return "latest"
        if opt.load_model_name is not None:
            self.model.load(opt.which_epoch)
            return opt.which_epoch
        self.model.init_weights()
        return None

    def _resume_progress(self, opt):
        """Epoch / iteration counters and the derived run length (num_epochs == -1 means 'from num_iters')."""
        if not hasattr(opt, "iters_per_epoch"):
            raise AssertionError("opt must have attribute {iters_per_epoch}, it can be calculated by length of loader")
        self.iter_record_path = opt.ckpt_dir / opt.name / "iter.txt"
        self.first_epoch, self.iters = 1, 0
        if opt.continue_training:
            self.first_epoch, self.iters = np.loadtxt(self.iter_record_path, delimiter=",", dtype=int)
        if opt.num_epochs == -1:
            opt.num_epochs = math.ceil(opt.num_iters / (opt.iters_per_epoch + 1e-12))
        opt.num_iters = opt.num_epochs * opt.iters_per_epoch
        if not self.first_epoch < opt.num_epochs:
            raise AssertionError(f"first_epoch {self.first_epoch} should not larger than num_epochs {opt.num_epochs}")
        if not self.iters < opt.num_iters:
            raise AssertionError(f"iters {self.iters} should not larger than num_iters {opt.num_iters}")
        opt.first_epoch = self.first_epoch

    def _init_lr(self, opt):
        assert len(opt.lr) in (1, 2), f"length of lr must be 1 or 2, not {len(opt.lr)}"
        self.lr = {"D": opt.lr[0], "G": opt.lr[1]} if len(opt.lr) == 2 else opt.lr[0]

    def _lr_of(self, network_name):
        return self.lr[network_name] if isinstance(self.lr, dict) else self.lr

    def _create_optimizer(self, opt):
        if not isinstance(self.lr, (int, float, dict)):
            raise AssertionError("type of lr should be scalar or dict")
        if opt.optimizer in ("sgd", "rmsprop"):          # torch's defaults, lr only (base_trainer.py:71-74)
            cls = FusedSGD if opt.optimizer == "sgd" else FusedRMSprop
            self.optimizers = {name: cls(net.parameters(), lr=self._lr_of(name)) for name, net in self.model.networks.items()}
            return
        if opt.optimizer not in _OPTIMIZER_ARGS:
            raise NameError(f"optimizer named {opt.optimizer} not defined")
        self.optimizers = {name: FusedAdam(net.parameters(), lr=self._lr_of(name), max_grad_norm=self.max_grad_norm,
                                           **_OPTIMIZER_ARGS[opt.optimizer])
                           for name, net in self.model.networks.items()}

    def _scheduler_for(self, opt, name, optimizer):
        kind = opt.scheduler
        if kind == "step":
            return optim.lr_scheduler.StepLR(optimizer, step_size=opt.num_epochs // _STEP_LR_STAGES,
                                             gamma=opt.lr_decay ** (1 / _STEP_LR_STAGES))
        if kind == "exp":
            return optim.lr_scheduler.ExponentialLR(optimizer, gamma=opt.lr_decay ** (1 / opt.num_epochs))
        if kind == "cos":                          # anneals to lr * lr_decay over the run (base_trainer.py:103-111)
            return optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.num_epochs, eta_min=self._lr_of(name) * opt.lr_decay)
        raise NameError(f"scheduler named {kind} not defined")

    def _create_scheduler(self, opt):
        self.schedulers = {name: self._scheduler_for(opt, name, o) for name, o in self.optimizers.items()}
        for _ in range(self.first_epoch):          # the reference fast-forwards to first_epoch (>= 1) at construction
            for scheduler in self.schedulers.values():
                scheduler.step()

    # ---- the step both stages share: one D update, then (every ``num_critics`` iterations) one G update -------------------
    def _step(self, *inputs):
        """``opt.graph_step``: replayed from a captured graph after ``opt.graph_warmup`` eager calls (trainers/graph_step.py)"""
        if self.graph_step:
            if self._graphs is None:
                from .graph_step import GraphStep
                self._graphs = GraphStep(self)
            self._graphs.step(*inputs)
        else:
            self._eager_step(*inputs)

    def _eager_step(self, *inputs):
        self.iters += 1
        self._train_discriminator_once(*inputs)
        if self.iters % self.opt.num_critics == 0:
            self._train_generator_once(*inputs)

    # ---- loss bookkeeping (self.losses[kind][name] lists, like the reference) ----------------------------------
    def _set_loss_types(self, own, last=()):
        """``loss_types``: the stage's ``own`` kinds, "grad_norm" with ``opt.max_grad_norm`` (the norm before clipping, per update),
        then the stage's ``last`` ones; and their empty lists."""
        self.loss_types = list(own) + ["grad_norm"] * (self.max_grad_norm is not None) + list(last)
        self._init_losses()

    def _init_losses(self):
        self.losses = {loss_type: defaultdict(list) for loss_type in self.loss_types}

    def _record(self, keys, tensors):
        stacked = torch.stack([t.detach() for t in tensors])
        if self._graph_records is not None:          # being captured: the replays hand the losses over (graph_step.py)
            self._graph_records.append((keys, stacked))
        elif self.defer_loss_sync:
            self._pending.append((keys, stacked))
        else:
            for (kind, name), v in zip(keys, stacked.tolist()):        # ONE device->host read for the group
                self.losses[kind][name].append(v)

    def _grad_norm_records(self, *names):
        """-> (keys, tensors) to add to a ``_record`` call after the updates of the optimizers ``names``: with ``opt.max_grad_norm``
        the norm each of them measured before clipping, ``("grad_norm", name)``, read from device memory like a loss (NaN when the
        optimizer has not stepped yet: a GradScaler skipped its first update); else nothing."""
        if self.max_grad_norm is None:
            return [], []
        norms = [self.optimizers[name].grad_norm for name in names]
        return ([("grad_norm", name) for name in names],
                [torch.full((), float("nan"), device=self.opt.device) if n is None else n[0] for n in norms])

    def flush_losses(self):
        if self._pending:
            flat = torch.cat([s for _, s in self._pending]).tolist()
            i = 0
            for keys, s in self._pending:
                for kind, name in keys:
                    self.losses[kind][name].append(flat[i])
                    i += 1
            self._pending = []

    def _bn_scope(self):
        """What the model calls of a step run in: under a reducer with ``sync_bn`` (parallel.attach_ddp) the scope in which training-mode
        BatchNorm takes the global batch's statistics and the MAE stage draws the global batch's masks (ops.bn_sync); else nothing."""
        red = getattr(self, "reducer", None)
        return red.bn_scope() if red is not None else contextlib.nullcontext()

    def release_graphs(self):
        """Drop the captured graphs of ``graph_step`` (the next step() warms up and captures again)."""
        if self._graphs is not None:
            self._graphs.release()

    # ---- validation: a pass that leaves training exactly where it was ------------------------------------------------------------
    def _generators(self):
        """the generator and its EMA copy: every module validation may run that memoizes SPADE tables"""
        nets = [self.model.netG] + [net for label, net in self.model.ema.items() if label == "G"]
        return [net for net in nets if hasattr(net, "clear_spade_cache")]

    @contextlib.contextmanager
    def _validation_scope(self):
        """What ``validate()`` runs in: no grad, every draw from generators of validation's own, seeded by ``opt.val_seed`` -- the
        torch CPU and device RNGs inside ``torch.random.fork_rng``, Python's ``random`` saved and put back, and a fresh
        ``ops.DeviceRng(val_seed)`` swapped in for the model's ``mask_rng`` / ``embed_rng``, whose counters therefore never move
        (``diffaug_rng`` is not drawn from: no inference mode augments).  On exit every module has the ``training`` flag it had
        (the inference modes put the networks in eval mode, so BatchNorm's running statistics and ``num_batches_tracked`` are only
        read), the generator has the table marks it had, and the SPADE tables and the label-set memo are dropped: the next train
        pass on the same label tensor re-primes.  Nothing inside touches ``iters``, an optimizer or a captured graph."""
        import random
        model, seed = self.model, self.val_opts["val_seed"]
        device = torch.device(self.opt.device)
        modules = [m for net in list(model.networks.values()) + list(self._extra_modules().values()) for m in net.modules()]
        flags = [m.training for m in modules]
        marks = model.netG.table_marks() if hasattr(model.netG, "table_marks") else None
        swapped = {}
        if getattr(model, "mask_rng", None) is not None:
            swapped["mask_rng"], model.mask_rng = model.mask_rng, ops.DeviceRng(seed, device)
        bank = getattr(model, "embed_bank", None)
        if bank is not None:
            swapped["embed_rng"], bank.rng = bank.rng, ops.DeviceRng(seed, device)
            model.embed_rng = bank.rng
        py_state = random.getstate()
        try:
            with torch.no_grad(), torch.random.fork_rng(devices=[device] if device.type == "cuda" else []):
                torch.manual_seed(seed)
                random.seed(seed)
                yield
        finally:
            random.setstate(py_state)
            if "mask_rng" in swapped:
                model.mask_rng = swapped["mask_rng"]
            if "embed_rng" in swapped:
                bank.rng = model.embed_rng = swapped["embed_rng"]
            for m, flag in zip(modules, flags):
                m.__dict__["training"] = flag
            for net in self._generators():
                net.clear_spade_cache()
            if marks is None and hasattr(model.netG, "table_marks") and model.netG.table_marks() is not None:
                for m in model.netG._table_modules():        # (a pass before the first step: that step still finds an unmarked tree)
                    m.__dict__.pop("_ran_class_mode", None)
                model.netG.__dict__.pop("_marked_table_modules", None)
            if hasattr(model, "_label_sets"):
                model._label_sets = None

    def _classify(self, images, labels, counts):
        """D's classifier on ``images`` against ``labels``: its confusion counts added to ``counts`` (None: a fresh buffer) -> counts"""
        _, logits = self.model.netD(images)
        return ops.clf_counts(logits, labels.to(logits.device).reshape(logits.shape[0], -1), self.model.clf_loss_type, out=counts)

    def _finish_validation(self, names, scores):
        """``scores``: float64 device tensors whose concatenation holds one value per name -> {name: float}, with the ONE host read
        of the pass; each value is appended to ``self.metrics[name]``"""
        values = torch.cat([s.reshape(-1) for s in scores]).tolist()
        assert len(values) == len(names)
        out = dict(zip(names, values))
        for name, v in out.items():
            self.metrics[name].append(v)
        return out

    def maybe_save_best(self, epoch):
        """With ``opt.save_best = "<metric>"``, after a ``validate()``: when the metric's newest value beats the best one so far (higher
        is better, lower for ``l1``; NaN never does), ``save_checkpoint("best", epoch)`` -- ``best_net_*.pth``, with ``opt.train_state``
        ``best_train_state.pth`` -- and ``best.txt`` = (epoch, iters, value) next to them.  -> whether it saved."""
        name = self.val_opts["save_best"]
        if name is None or not self.metrics[name]:
            return False
        value = self.metrics[name][-1]
        sign = -1.0 if name in LOWER_IS_BETTER else 1.0
        if math.isnan(value) or (self.best is not None and not sign * value > sign * self.best[2]):
            return False
        self.best = (int(epoch), int(self.iters), float(value))
        self.save_checkpoint("best", epoch)
        path = self.opt.ckpt_dir / self.opt.name / "best.txt"
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(f"{self.best[0]},{self.best[1]},{self.best[2]!r}\n")
        return True

    # ---- checkpoints: weights as the reference writes them; with opt.train_state one more file, written last --------------------
    def save_checkpoint(self, label, epoch, latest=False):
        """The one place that writes a checkpoint: the weight files of ``label`` ("latest" or an epoch number; ``model.save``),
        ``iter.txt`` = (epoch, iters) for ``latest`` (what ``--continue_training`` restores), and with ``opt.train_state``
        ``<label>_train_state.pth`` last of all, whose digests tie the other files to it."""
        self.model.save(label)
        if latest:
            self.iter_record_path.parent.mkdir(parents=True, exist_ok=True)
            np.savetxt(self.iter_record_path, (epoch, self.iters), fmt="%i", delimiter=",")
        if self.train_state:
            TS.write(self._train_state(epoch), self._train_state_path(self.opt.name, label))

    def save_latest(self, epoch):
        """``latest_net_{G,D}.pth`` + ``iter.txt`` = (epoch, iters), what ``--continue_training`` restores
        (defectgan_trainer.py:111-113, base_trainer.py:38-44).  The reference saves no optimizer state; with ``opt.train_state``
        ``latest_train_state.pth`` carries it, with the RNG states and the digests of the other files (train_state.py)."""
        self.save_checkpoint("latest", epoch, latest=True)

    def _train_state_path(self, run_name, label):
        return self.opt.ckpt_dir / run_name / f"{label}_train_state.pth"

    def _extra_modules(self):
        """{name: module}: what an optimizer trains outside ``model.networks`` and therefore outside the weight files -- the MAE
        stage's mask token where it has a parameter.  The train-state file carries their ``state_dict``s."""
        token = getattr(self.model, "mask_token", None)
        if isinstance(token, torch.nn.Module) and next(token.parameters(), None) is not None:
            return {"mask_token": token}
        return {}

    def _sibling_networks(self):
        """{name: module} of the weight files: ``net_<label>`` the networks, ``net_<label>_ema`` their EMA copies"""
        out = {f"net_{label}": net for label, net in self.model.networks.items()}
        out.update({f"net_{label}_ema": net for label, net in self.model.ema.items()})
        return out

    def _sibling_tensors(self):
        """{name: tensors}: what each sibling file of a checkpoint holds, from the live modules -- ``net_<label>`` and
        ``net_<label>_ema`` (``state_dict()`` values in key order), ``ada`` (p_rt, acc); file ``<epoch>_<name>.pth``"""
        model = self.model
        out = {name: list(net.state_dict().values()) for name, net in self._sibling_networks().items()}
        ada = getattr(model, "ada", None)
        if ada is not None:
            out["ada"] = [ada.p_rt, ada.acc]
        return out

    def state_digest(self):
        """{name: 64-bit int}: one digest (ops.state_digest) per network, EMA copy and ADA word pair (the names of
        ``_sibling_tensors``), per module of ``_extra_modules`` and per optimizer (``optim_<name>``: its moments in parameter
        order).  Computed on the device, ONE host read in total: two runs, or two ranks, compare their whole state by it."""
        groups = self._sibling_tensors()
        groups.update({name: list(mod.state_dict().values()) for name, mod in self._extra_modules().items()})
        groups.update({f"optim_{name}": TS.optimizer_tensors(o) for name, o in self.optimizers.items()})
        return TS.digests(groups)

    def _train_state(self, epoch):
        model, device = self.model, self.opt.device
        state = {"iters": int(self.iters), "epoch": int(epoch),
                 "optimizers": {name: TS.optimizer_state(o) for name, o in self.optimizers.items()},
                 "modules": {name: {k: v.detach().cpu() for k, v in mod.state_dict().items()}
                             for name, mod in self._extra_modules().items()},
                 # (host state that decides launches: which SPADE table modules the generator's first forward found running)
                 "table_marks": {label: net.table_marks() for label, net in model.networks.items() if hasattr(net, "table_marks")},
                 "rng": TS.rng_state(device), "digests": TS.digests(self._sibling_tensors())}
        # (what load_network drops from a weight file -- SEAN's label-latent layers, like the reference: a resumed run needs them)
        dropped = {name: {k: v.detach().cpu() for k, v in tensors_dropped_on_load(net).items()}
                   for name, net in self._sibling_networks().items()}
        if any(dropped.values()):
            state["dropped_on_load"] = {name: tensors for name, tensors in dropped.items() if tensors}
        scaler = getattr(self, "scaler", None)
        if scaler is not None and scaler.is_enabled():
            state["grad_scaler"] = scaler.state_dict()
        for key in ("diffaug_rng", "mask_rng", "embed_rng"):
            rng = getattr(model, key, None)
            if rng is not None:
                state[key] = list(rng.state())
        bank = getattr(model, "embed_bank", None)
        if bank is not None:              # (the draws index the packed embeddings file: a resumed run must pack the same one)
            state["embed_digest"] = int(bank.digest().item()) & (2 ** 64 - 1)
        return state

    def resume_train_state(self):
        """With ``opt.train_state``, under ``continue_training`` (label "latest") or ``load_model_name`` + ``which_epoch``, once the
        weights are loaded and the optimizers (and the MAE stage's GradScaler) exist: check the loaded modules against the digests
        of ``<label>_train_state.pth`` (RuntimeError naming the file that does not belong), then restore the optimizers' state,
        the modules no weight file holds, the GradScaler and every RNG.  Learning rates are not stored (TS.optimizer_state), and
        under ``load_model_name`` alone ``iters`` and the epoch stay the new run's.  Without the file the run resumes from the
        weights alone, as it did before, and says so.  Captured graphs are released."""
        opt = self.opt
        if not self.train_state:
            return
        if opt.continue_training:
            label = "latest"
        elif opt.load_model_name is not None:
            label = opt.which_epoch
        else:
            return
        path = self._train_state_path(opt.load_model_name, label)
        if not path.exists():
            print(f"no train state at {path}: resuming from the weights only (optimizers and RNGs start anew)")
            self.train_state_restored = False
            return
        state = TS.read(path)
        if opt.continue_training and int(state["iters"]) != int(self.iters):
            raise RuntimeError(f"{self.iter_record_path} does not belong to this checkpoint: it records iteration {int(self.iters)}, "
                               f"{path.name} was saved at iteration {int(state['iters'])}")
        for name, tensors in state.get("dropped_on_load", {}).items():       # (before the digests: they cover these tensors too)
            net = self._sibling_networks().get(name)
            if net is not None:
                net.load_state_dict(tensors, strict=False)
                ops.mark_written(*net.parameters())
        TS.check_digests(state["digests"], TS.digests(self._sibling_tensors()), lambda name: path.with_name(f"{label}_{name}.pth"))
        if sorted(state["optimizers"]) != sorted(self.optimizers):
            raise RuntimeError(f"{path}: saved with optimizers {sorted(state['optimizers'])}, this trainer has {sorted(self.optimizers)}")
        bank = getattr(self.model, "embed_bank", None)
        if bank is not None and "embed_digest" in state:
            now = int(bank.digest().item()) & (2 ** 64 - 1)
            if now != int(state["embed_digest"]):
                raise RuntimeError(f"opt.embed_path ({opt.embed_path}) does not hold the embeddings this checkpoint was saved with: "
                                   f"{path.name} records digest {int(state['embed_digest']):#018x} of the packed file, this one gives "
                                   f"{now:#018x} (the embeddings file changed between the save and the resume)")
        self.release_graphs()
        for name, o in self.optimizers.items():
            TS.load_optimizer_state(o, state["optimizers"][name], name)
        for name, mod in self._extra_modules().items():
            if name in state["modules"]:
                mod.load_state_dict(state["modules"][name])
                ops.mark_written(*mod.parameters())
        for label, marks in state.get("table_marks", {}).items():
            if marks is not None and label in self.model.networks:
                self.model.networks[label].set_table_marks(marks)
        scaler = getattr(self, "scaler", None)
        if scaler is not None and scaler.is_enabled() and "grad_scaler" in state:
            scaler.load_state_dict(state["grad_scaler"])
        for key in ("diffaug_rng", "mask_rng", "embed_rng"):
            rng = getattr(self.model, key, None)
            if rng is not None and key in state:
                rng.set_state(tuple(state[key]))
        TS.set_rng_state(state["rng"], opt.device)
        self.train_state_restored = True

    def _update_per_epoch(self, epoch=None):
        for scheduler in self.schedulers.values():
            scheduler.step()
        self.model.update_per_epoch(epoch)
