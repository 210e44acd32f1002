"""Exact-resume checkpoints (``opt.train_state``; stargan ``Solver.save`` / ``load``): what the weight files do not carry -- optimizer
moments and step counts, the GradScaler, the CPU and device RNG states, the device-drawn generators' counters -- in one more file
next to them, and the digests that tie the files of one save together.

The weight files keep the reference's format (plain ``state_dict``s).  The train-state file is a dict of tensors, numbers, strings,
lists and dicts only, so ``torch.load(..., weights_only=True)`` reads it.  It is written last, to a temporary name that
``os.replace`` moves into place: a save cut short leaves the previous file, whose digests then refuse the newer weights.

A digest (``ops.state_digest``) is one 64-bit word over every bit of a list of device tensors, computed on the device; ``digests``
reads any number of them in one transfer.  At save time they are taken from the live modules, after a load from the modules just
filled: a sibling file from another save, or a damaged one, shows as a mismatch and ``check_digests`` names the file."""
import os
from pathlib import Path

import torch

from . import ops

FORMAT_VERSION = 1
_STATE_TENSORS = ("exp_avg", "exp_avg_sq", "square_avg")      # FusedAdam's moments, FusedRMSprop's square average


# ---- the file ------------------------------------------------------------------------------------------------------------
def write(state, path):
    """``state`` (+ the format version) at ``path``, atomically: no reader ever sees half a file, and no temporary file stays"""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(path.name + f".tmp{os.getpid()}")
    try:
        torch.save(dict(state, format_version=FORMAT_VERSION), tmp)
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()


def read(path):
    """-> the dict ``write`` stored (tensors on the CPU); a file of a later format version is refused"""
    state = torch.load(path, map_location="cpu", weights_only=True)
    version = state.get("format_version") if isinstance(state, dict) else None
    if not isinstance(version, int) or not 1 <= version <= FORMAT_VERSION:
        raise RuntimeError(f"{path}: train-state format version {version!r}; this package reads versions 1..{FORMAT_VERSION}")
    return state


# ---- optimizers ----------------------------------------------------------------------------------------------------------
def optimizer_state(optimizer):
    """-> per param group, per parameter in order: None (no state yet) or {"step", and the state tensors on the CPU}.  Learning rates
    are not stored: a resumed trainer's schedulers are fast-forwarded at construction, which leaves every group's ``lr`` and
    ``initial_lr`` where the uninterrupted run has them; a stored ``lr`` would be decayed a second time."""
    out = []
    for group in optimizer.param_groups:
        rows = []
        for p in group["params"]:
            st = optimizer.state.get(p)
            rows.append({k: (v.detach().cpu() if isinstance(v, torch.Tensor) else int(v)) for k, v in st.items()} if st else None)
        out.append(rows)
    return out


def load_optimizer_state(optimizer, stored, who):
    """the inverse, onto the optimizer's own parameters (same groups, same order, same shapes: else RuntimeError)"""
    groups = optimizer.param_groups
    if len(stored) != len(groups) or any(len(rows) != len(g["params"]) for rows, g in zip(stored, groups)):
        raise RuntimeError(f"train state: optimizer {who} was saved with {[len(r) for r in stored]} parameters per group, "
                           f"this one has {[len(g['params']) for g in groups]}")
    for rows, group in zip(stored, groups):
        for st, p in zip(rows, group["params"]):
            optimizer.state.pop(p, None)
            if st is None:
                continue
            new = {}
            for k, v in st.items():
                if isinstance(v, torch.Tensor):
                    if v.shape != p.shape:
                        raise RuntimeError(f"train state: optimizer {who}: {k} of shape {tuple(v.shape)} for a parameter of shape "
                                           f"{tuple(p.shape)}")
                    new[k] = torch.empty_like(p, memory_format=torch.contiguous_format).copy_(v)
                else:
                    new[k] = int(v)
            optimizer.state[p] = new


def optimizer_tensors(optimizer):
    """the state tensors in group, parameter and name order: what an optimizer's digest covers"""
    return [st[k] for group in optimizer.param_groups for p in group["params"] for st in (optimizer.state.get(p) or {},)
            for k in _STATE_TENSORS if k in st]


# ---- random-number generators ----------------------------------------------------------------------------------------------
def rng_state(device):
    """-> {"cpu": torch.get_rng_state(), "device": the default generator's state of a GPU ``device`` (absent on the CPU)}"""
    out = {"cpu": torch.get_rng_state()}
    device = torch.device(device)
    if device.type == "cuda":
        out["device"] = torch.cuda.get_rng_state(device)
    return out


def set_rng_state(state, device):
    torch.set_rng_state(state["cpu"])
    device = torch.device(device)
    if device.type == "cuda" and "device" in state:
        torch.cuda.set_rng_state(state["device"], device)


# ---- digests ---------------------------------------------------------------------------------------------------------------
def digests(groups):
    """{name: list of device tensors} -> {name: the list's digest as an int in [0, 2^64)}: one launch group per name, ONE host read
    for all of them.  A name with no tensors is left out."""
    names = [name for name, tensors in groups.items() if tensors]
    if not names:
        return {}
    words = torch.cat([ops.state_digest(groups[name]) for name in names])
    return {name: int(w) & (2 ** 64 - 1) for name, w in zip(names, words.tolist())}


def check_digests(stored, now, file_of):
    """``stored``: the digests of the train-state file, ``now``: those of the modules just loaded; ``file_of(name)``: the sibling file
    a name stands for.  Names only one side has are not compared (an option, such as the EMA, turned on or off in between)."""
    for name, word in stored.items():
        if name in now and int(word) != now[name]:
            raise RuntimeError(f"{file_of(name)} does not belong to this checkpoint: the train-state file was saved with digest "
                               f"{int(word):#018x} of its tensors, the loaded ones give {now[name]:#018x} (files of different saves, "
                               "or a damaged file)")


# ---- the option --------------------------------------------------------------------------------------------------------------
def train_state_option(opt):
    """-> ``opt.train_state`` as a bool (absent, None or False: off -- no file is written or read and no launch is made).  Refused
    before anything is built: SEAN generators with host-drawn embeddings (the ``random.choices`` draws live in Python's RNG) or with
    ``use_running_stats`` (the tracked codes live in Python lists) -- ``opt.embed_rng = "device"`` draws from a counter the file
    carries -- and a CPU device (the digests are computed on the GPU)."""
    on = getattr(opt, "train_state", None)
    if on is None or on is False:
        return False
    if on is not True:
        raise ValueError(f"|train_state {on!r}| is invalid (True or False)")
    if getattr(opt, "style_norm_block_type", None) == "sean":
        if getattr(opt, "embed_rng", None) != "device":
            raise NotImplementedError("train_state with style_norm_block_type='sean' (its embedding lists and the host's random.choices "
                                      "draws are not part of a checkpoint; build the trainer with embed_rng='device')")
        if getattr(opt, "use_running_stats", False):
            raise NotImplementedError("train_state with style_norm_block_type='sean' and use_running_stats=True (the tracked codes "
                                      "live in Python lists that are not part of a checkpoint)")
    if torch.device(opt.device).type != "cuda":
        raise ValueError(f"train_state computes its digests on the GPU; opt.device is {opt.device}")
    return True
