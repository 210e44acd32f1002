"""The reference's stargan-v2 loss functions and train iteration (stargan-v2/core/solver.py) on the product's networks: same function
names, argument meaning and return values (loss tensor + a namespace of floats); ``Solver.train_iteration`` is one pass of the body of
``Solver.train`` (solver.py:262-296) for ``norm_type adain``, ``w_hpf 0``:

  * DiffAugment(., args.DiffAugment) on what the discriminator sees -- x_real and x_fake of the D loss, x_fake of the G loss
    (solver.py:472,481,510), drawn from the global CPU RNG in the reference's order; the R1 penalty is taken with respect to the
    un-augmented x_real, through the augmentation (ops.diff_augment is differentiable twice);
  * lambda_ds decayed linearly to 0 over args.ds_iter iterations (solver.py:311-313), after the EMA;
  * Adam with coupled weight decay per network, EMA (beta 0.999) of the generator-side networks.

Not the reference's iteration: ``generator.update_stats()`` is not called (open item), and the w_hpf > 0 / SEAN paths
(heat-map masks, their downloaded weights) are not built.

Data-parallel (``parallel.attach_ddp(solver)``, the reference's ``nn.DataParallel``): every rank holds rows [rank * b, (rank + 1) * b)
of the same global batch and the ranks together compute what one process computes on the whole batch -- stargan-v2 has no batch
statistics and every loss term is a mean over samples, so the SUM of the ranks' gradients with 1/world in Adam is the global batch's
gradient; DiffAugment draws the global batch's parameters on every rank and applies the rank's rows (``ops.diffaug_sharded``); the
reported losses are the global batch's (``global_means``)."""
import contextlib
from pathlib import Path
from types import SimpleNamespace

import torch
import torch.distributed as dist

from .. import ops
from .. import train_state as TS
from ..optim import FusedAdam, ema_lerp_

_reducer = None         # the attached GradReducer while Solver.train_iteration runs data-parallel: the loss reads become global_means


def global_means(terms, n, group=None):
    """Per-rank loss terms (0-dim tensors, each a mean over the rank's n samples) -> the global batch's values as floats, the same on
    every rank: ONE small SUM all-reduce of the stacked terms and one device-to-host read.  The message also carries n and n * n:
    sum(n)^2 == world * sum(n^2) holds only when every rank has the same n, and only then is the mean of the ranks' means the global
    mean (and 1/world the right gradient average).  On a mismatch every rank has received the same sums and raises ValueError, so no
    rank goes on to a collective the others skip."""
    world = dist.get_world_size(group)
    v = torch.stack([t.detach().double() for t in terms])
    v = torch.cat([v, v.new_tensor([float(n), float(n) * n])])
    dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
    s = v.tolist()
    if s[-2] * s[-2] != world * s[-1]:
        raise ValueError(f"stargan data-parallel: the ranks' local batch sizes differ (sum {s[-2]:.0f}, sum of squares {s[-1]:.0f} over "
                         f"{world} ranks); every rank must hold the same number of rows of the global batch")
    return [x / world for x in s[:-2]]


def _floats(n, *losses):
    """the values of 0-dim loss tensors (means over a batch of n), in one device-to-host read -- the global batch's values while the
    Solver runs data-parallel"""
    if _reducer is not None:
        return global_means(losses, n, _reducer.pg)
    return torch.stack([t.detach().float() for t in losses]).tolist()


def adv_loss(logits, target):
    """solver.py:566-570"""
    assert target in [1, 0]
    return ops.bce_logits(logits, float(target))


def r1_reg(d_out, x_in):
    """solver.py:573-583: zero-centred gradient penalty on real images -- a DOUBLE backward through the discriminator (ops._ConvDgradFn &c.)"""
    batch_size = x_in.size(0)
    grad_dout = torch.autograd.grad(outputs=d_out.sum(), inputs=x_in, create_graph=True, retain_graph=True, only_inputs=True)[0]
    grad_dout2 = grad_dout.pow(2)
    assert grad_dout2.size() == x_in.size()
    return 0.5 * grad_dout2.view(batch_size, -1).sum(1).mean(0)


def get_style_code(nets, norm_type, num_embeds, y_trg, x_ref, z_trg):
    """core/utils.py:485-490"""
    if norm_type != "adain":
        raise NotImplementedError("stargan: norm_type 'adain' is built")
    return nets.mapping_network(z_trg, y_trg) if z_trg is not None else nets.style_encoder(x_ref, y_trg)


def compute_d_loss(nets, args, x_real, y_org, y_trg, z_trg=None, x_ref=None, masks=None):
    """solver.py:467-491"""
    assert (z_trg is None) != (x_ref is None)
    policy = getattr(args, "DiffAugment", "")
    x_real.requires_grad_()
    out = nets.discriminator(ops.diff_augment(x_real, policy), y_org)
    loss_real = adv_loss(out, 1)
    loss_reg = r1_reg(out, x_real)
    with torch.no_grad():
        s_trg = get_style_code(nets, args.norm_type, 1, y_trg, x_ref, z_trg)
        x_fake = nets.generator(x_real, s_trg, labels=y_trg, masks=masks)
    out = nets.discriminator(ops.diff_augment(x_fake, policy), y_trg)
    loss_fake = adv_loss(out, 0)
    loss = loss_real + loss_fake + args.lambda_reg * loss_reg
    real, fake, reg = _floats(x_real.size(0), loss_real, loss_fake, loss_reg)
    return loss, SimpleNamespace(real=real, fake=fake, reg=reg)


def compute_g_loss(nets, args, x_real, y_org, y_trg, z_trgs=None, x_refs=None, masks=None):
    """solver.py:494-546 (w_hpf = 0: no heat-map masks)"""
    assert (z_trgs is None) != (x_refs is None)
    z_trg, z_trg2 = z_trgs if z_trgs is not None else (None, None)
    x_ref, x_ref2 = x_refs if x_refs is not None else (None, None)
    s_trg = get_style_code(nets, args.norm_type, args.num_embeds, y_trg, x_ref, z_trg)
    x_fake = nets.generator(x_real, s_trg, labels=y_trg, masks=masks)
    out = nets.discriminator(ops.diff_augment(x_fake, getattr(args, "DiffAugment", "")), y_trg)
    loss_adv = adv_loss(out, 1)
    s_pred = get_style_code(nets, args.norm_type, args.num_embeds, y_trg, x_fake, z_trg=None)
    loss_sty = ops.l1(s_pred, s_trg)
    s_trg2 = get_style_code(nets, args.norm_type, args.num_embeds, y_trg, x_ref2, z_trg=z_trg2)
    x_fake2 = nets.generator(x_real, s_trg2, labels=y_trg, masks=masks).detach()
    loss_ds = ops.l1(x_fake, x_fake2)
    s_org = get_style_code(nets, args.norm_type, args.num_embeds, y_org, x_real, z_trg=None)
    x_rec = nets.generator(x_fake, s_org, labels=y_org, masks=None)
    loss_cyc = ops.l1(x_rec, x_real)
    loss = loss_adv + args.lambda_sty * loss_sty - args.lambda_ds * loss_ds + args.lambda_cyc * loss_cyc
    adv, sty, ds, cyc = _floats(x_real.size(0), loss_adv, loss_sty, loss_ds, loss_cyc)
    return loss, SimpleNamespace(adv=adv, sty=sty, ds=ds, cyc=cyc)


def moving_average(model, model_test, beta=0.999):
    """solver.py:549-551: param_test = lerp(param, param_test, beta), every tensor of the network in one launch, in place"""
    with torch.no_grad():
        ema_lerp_(model_test.parameters(), model.parameters(), beta)


class Solver:
    """solver.py:33-56 (networks, EMA copies, one Adam per network: lr / f_lr for the mapping network, betas, coupled weight decay)
    + one iteration of ``train`` (solver.py:262-296 and the lambda_ds decay of 311-313, norm_type adain).  The optimizers are the
    product's fused multi-tensor Adam, the EMA one multi-tensor launch per network."""

    def __init__(self, args, nets, nets_ema, device="cuda:0"):
        self.args, self.nets, self.nets_ema, self.device = args, nets, nets_ema, torch.device(device)
        self.initial_lambda_ds = args.lambda_ds          # the lambda_ds decay step is initial / ds_iter (solver.py:311-313)
        self.reducer = None                              # set by parallel.attach_ddp(): gradient all-reduce across ranks
        for ns in (nets, nets_ema):
            for m in vars(ns).values():
                m.to(self.device)
        self.optims = SimpleNamespace()
        for name, net in vars(nets).items():
            lr = args.f_lr if name == "mapping_network" else args.lr
            setattr(self.optims, name, FusedAdam(net.parameters(), lr=lr, betas=(args.beta1, args.beta2), weight_decay=args.weight_decay,
                                                 decoupled=False))

    # ---- checkpoints: the reference CheckpointIO's three files (solver.py:58-63: nets, nets_ema, optims; each a dict from network
    # name to state_dict) and a train-state file (train_state.py) that makes the resumed run the uninterrupted one ----------------
    def _ckpt_paths(self, step):
        root = Path(self.args.checkpoint_dir)
        return {kind: root / f"{step:06d}_{kind}.ckpt" for kind in ("nets", "nets_ema", "optims", "train_state")}

    def _ckpt_tensors(self):
        """{file kind: its tensors, network by network in name order of the namespace} from the live objects"""
        return {"nets": [v for net in vars(self.nets).values() for v in net.state_dict().values()],
                "nets_ema": [v for net in vars(self.nets_ema).values() for v in net.state_dict().values()],
                "optims": [t for o in vars(self.optims).values() for t in TS.optimizer_tensors(o)]}

    def save(self, step):
        """``{step:06d}_nets.ckpt``, ``_nets_ema.ckpt``, ``_optims.ckpt`` under ``args.checkpoint_dir``, then ``_train_state.ckpt``:
        the decayed ``args.lambda_ds`` (and the initial one its decay step comes from), the CPU and device RNG states and the
        digests of the three files' tensors, written last and atomically."""
        paths = self._ckpt_paths(step)
        paths["nets"].parent.mkdir(parents=True, exist_ok=True)
        torch.save({name: net.state_dict() for name, net in vars(self.nets).items()}, paths["nets"])
        torch.save({name: net.state_dict() for name, net in vars(self.nets_ema).items()}, paths["nets_ema"])
        torch.save({name: o.state_dict() for name, o in vars(self.optims).items()}, paths["optims"])
        TS.write({"step": int(step), "lambda_ds": float(self.args.lambda_ds), "initial_lambda_ds": float(self.initial_lambda_ds),
                  "rng": TS.rng_state(self.device), "digests": TS.digests(self._ckpt_tensors())}, paths["train_state"])

    def load(self, step):
        """The inverse of ``save``.  The optimizers take their per-parameter state (moments, step counts) from the file and keep
        their own hyper-parameters.  After the load the digests of the loaded tensors are compared with the stored ones: a file of
        another save, or a damaged one, raises RuntimeError naming it."""
        paths = self._ckpt_paths(step)
        state = TS.read(paths["train_state"])
        for kind, ns in (("nets", self.nets), ("nets_ema", self.nets_ema)):
            stored = torch.load(paths[kind], map_location="cpu", weights_only=True)
            for name, net in vars(ns).items():
                net.load_state_dict(stored[name])
                ops.mark_written(*net.parameters())
        stored = torch.load(paths["optims"], map_location="cpu", weights_only=True)
        for name, o in vars(self.optims).items():
            groups = o.state_dict()["param_groups"]          # (this solver's lr, betas, weight decay)
            o.load_state_dict({"state": stored[name]["state"], "param_groups": groups})
        TS.check_digests(state["digests"], TS.digests(self._ckpt_tensors()), lambda kind: paths[kind])
        self.args.lambda_ds = float(state["lambda_ds"])
        self.initial_lambda_ds = float(state["initial_lambda_ds"])
        TS.set_rng_state(state["rng"], self.device)

    def _reset_grad(self):
        for opt in vars(self.optims).values():
            opt.zero_grad()

    @contextlib.contextmanager
    def _data_parallel(self):
        """while the iteration runs under an active reducer: the loss reads are global_means, DiffAugment draws the global batch"""
        global _reducer
        red = self.reducer
        if red is None or not red.active:
            yield None
            return
        prev, _reducer = _reducer, red
        try:
            with ops.diffaug_sharded(dist.get_rank(red.pg), red.world):
                yield red
        finally:
            _reducer = prev

    @staticmethod
    @contextlib.contextmanager
    def _frozen(red, *nets):
        """Under a reducer: the networks' parameters do not require grad while a G loss graph is built and differentiated.  The reference
        computes their weight gradients there and zeroes them before they are used; here they are not computed, so they never enter a
        collective (gradients still flow THROUGH the networks)."""
        params = [p for net in nets for p in net.parameters() if p.requires_grad] if red is not None else []
        for p in params:
            p.requires_grad_(False)
        try:
            yield
        finally:
            for p in params:
                p.requires_grad_(True)

    def train_iteration(self, x_real, y_org, y_trg, x_ref, x_ref2, z_trg, z_trg2):
        """One iteration on (a rank's rows of) the batch.  Under ``parallel.attach_ddp``: every rank passes rows
        [rank * b, (rank + 1) * b) of the same global batch (z codes included) and the same b; the returned losses are the global
        batch's on every rank."""
        args, nets, optims = self.args, self.nets, self.optims
        out = {}
        with self._data_parallel() as red:
            d_loss, out["d_latent"] = compute_d_loss(nets, args, x_real, y_org, y_trg, z_trg=z_trg)
            self._reset_grad()
            d_loss.backward()
            if red is not None:
                red.reduce(nets.discriminator)
            optims.discriminator.step()
            d_loss, out["d_ref"] = compute_d_loss(nets, args, x_real, y_org, y_trg, x_ref=x_ref)
            self._reset_grad()
            d_loss.backward()
            if red is not None:
                red.reduce(nets.discriminator)
            optims.discriminator.step()
            with self._frozen(red, nets.discriminator):
                g_loss, out["g_latent"] = compute_g_loss(nets, args, x_real, y_org, y_trg, z_trgs=[z_trg, z_trg2])
                self._reset_grad()
                g_loss.backward()
            if red is not None:
                red.reduce(nets.generator, nets.mapping_network, nets.style_encoder)
            optims.generator.step()
            optims.mapping_network.step()
            optims.style_encoder.step()
            with self._frozen(red, nets.discriminator, nets.style_encoder):
                g_loss, out["g_ref"] = compute_g_loss(nets, args, x_real, y_org, y_trg, x_refs=[x_ref, x_ref2])
                self._reset_grad()
                g_loss.backward()
            if red is not None:
                red.reduce(nets.generator)
            optims.generator.step()
        for name in ("generator", "mapping_network", "style_encoder"):
            moving_average(getattr(nets, name), getattr(self.nets_ema, name), beta=0.999)
        if args.lambda_ds > 0:
            args.lambda_ds -= self.initial_lambda_ds / getattr(args, "ds_iter", 100000)
        return out
