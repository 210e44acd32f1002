"""BaseModel: what the reference's trainers rely on from a model object (models/base_model.py:7-86) -- the ``networks``
mapping discovered from ``net*`` attributes, weight initialisation, checkpoint save / load per network, the mean-reduced
loss helper and the per-epoch hook."""
import copy

import torch.nn

from .. import ops, optim
from ..networks import _checkpoint_path, load_network, save_network

# the helper's four kinds as HIP ops: bce and l1 are what the hot path itself names; cce / mse arrive as opt.clf_loss_type
_LOSSES = {"bce": ops.bce_logits, "bce_logits": ops.bce_logits, "cce": ops.cce_logits, "l1": ops.l1, "mse": ops.mse}


class BaseModel:
    network_prefix = "net"

    def __init__(self, opt):
        self.opt = opt
        # opt.ema_beta > 0: eval-mode copies of the modules the G optimizer trains, keyed like ``networks`` and made by
        # create_ema() -- held here and not under ``net*`` names, so that ``networks`` (one optimizer each) does not grow
        self.ema = {}
        self.ema_group = None        # optim.EmaGroup over every tensor of the copies

    @property
    def networks(self):
        """{'G': self.netG, 'D': self.netD, ...}: every nn.Module attribute whose name starts with 'net', keyed by the rest
        of the name (trainers index optimizers by these keys)."""
        cut = len(self.network_prefix)
        return {attr[cut:] if attr.startswith(self.network_prefix) else attr: module
                for attr, module in vars(self).items()
                if attr.startswith(self.network_prefix) and isinstance(module, torch.nn.Module)}

    def _each_network(self):
        return self.networks.items()

    def init_weights(self):
        kind, gain = self.opt.init_type, self.opt.init_variance
        print(f"initialize model's parameters using {kind} with variance={gain}")
        for label, net in self._each_network():
            if label.endswith("_"):               # a trailing underscore marks a network that keeps its own weights
                continue
            net.init_weights(kind, gain)

    def save(self, epoch):
        for label, net in self._each_network():
            save_network(net, label, epoch, self.opt)
        for label, net in self.ema.items():              # <epoch>_net_<label>_ema.pth
            save_network(net, label + "_ema", epoch, self.opt)

    def load(self, epoch):
        self.load_serial = getattr(self, "load_serial", 0) + 1        # (a trainer's captured graphs are released: graph_step.py)
        print(f"load model's weights from epoch {epoch}")
        for label, net in self._each_network():
            load_network(net, label, epoch, self.opt)
        self.load_ema(epoch)

    # ---- EMA of the generator side (opt.ema_beta) ------------------------------------------------------------------------
    def _ema_sources(self):
        """{label: the live module}: what the G optimizer trains (a model with an EMA names them)"""
        return {}

    def create_ema(self, epoch=None):
        """Called by the trainer once the live weights are initialised or restored, and before the first forward: with
        ``opt.ema_beta > 0`` a copy of every module of ``_ema_sources`` -- equal to it, in eval mode, no parameter requiring a
        gradient, its own packed-weight caches -- and the launch group that updates them.  ``epoch``: the checkpoint the live
        weights came from, whose EMA files the copies are restored from where they exist."""
        beta, _, _ = optim.ema_options(self.opt)
        self.ema, self.ema_group = {}, None
        if beta == 0.0:
            return
        lerp, buffers = [], []
        for label, net in self._ema_sources().items():
            # (shared, not copied: the option object, and the precision singletons, which the ops compare by identity)
            twin = copy.deepcopy(net, {id(o): o for o in (self.opt, ops.BF16, ops.F32)})
            twin.requires_grad_(False)
            twin.eval()
            self.ema[label] = twin
            lerp += list(zip(twin.parameters(), net.parameters()))
            buffers += list(zip(twin.buffers(), net.buffers()))
        self.ema_group = optim.EmaGroup(lerp, buffers)
        if epoch is not None:
            self.load_ema(epoch)

    def load_ema(self, epoch):
        """The copies as checkpoint ``epoch`` holds them; a copy without a file (a run trained without EMA) restarts from the
        live weights just loaded."""
        live = self._ema_sources()
        for label, net in self.ema.items():
            if _checkpoint_path(self.opt, self.opt.load_model_name, label + "_ema", epoch).exists():
                load_network(net, label + "_ema", epoch, self.opt)
            else:
                net.load_state_dict(live[label].state_dict())

    def update_ema(self, iters):
        """After the G update that ends iteration ``iters``: every copy follows its module (optim.EmaGroup.update)."""
        if self.ema_group is not None:
            beta, start_iter, _ = optim.ema_options(self.opt)
            self.ema_group.update(optim.ema_weight(iters, start_iter, beta))

    def ema_graph_prepare(self, plan, iters):
        beta, start_iter, _ = optim.ema_options(self.opt)
        self.ema_group.graph_prepare(plan, iters, self.opt.num_critics, start_iter, beta)

    def load_network(self, network_name, epoch):
        self.load_serial = getattr(self, "load_serial", 0) + 1
        print(f"load net_{network_name}'s weights from epoch {epoch}")
        load_network(self.networks[network_name], network_name, epoch, self.opt)

    def __repr__(self):
        blocks = []
        for label, net in self._each_network():
            rule = "=" * 50 + f"{self.network_prefix + label:^8}" + "=" * 50 + "\n"
            blocks.append(rule + repr(net) + "\n" + rule)
        return "".join(blocks)

    def _cal_loss(self, logits, targets, loss_type):
        """base_model.py:68-80 -- mean-reduced; `targets` may be a python constant (all-ones / all-zeros labels) for bce and mse;
        cce takes class weights of the logits' shape (one-hot rows: the class-index form)."""
        fn = _LOSSES.get(loss_type)
        if fn is None:
            raise ValueError(f"loss_type: {loss_type} is not on the MI355X hot path (bce | cce | l1 | mse)")
        return fn(logits, targets)

    def update_per_epoch(self, epoch):
        for _, net in self._each_network():
            hook = getattr(net, "update_per_epoch", None)
            if hook is not None:
                hook(epoch)
