"""CPU: the host halves of data-parallel stargan-v2 (parallel.attach_ddp(solver)).

* DiffAugment's sharded draw (utils.diffaug.draw_params(shard=(rank, world))): the ranks' rows, concatenated, are the global batch's
  draw, and each rank leaves the global CPU RNG where the global draw leaves it -- so ranks that start from the same RNG state apply
  the augmentation one process applies to the global batch, and stay in lockstep.
* The loss-averaging / shard-size helper (stargan.solver.global_means) on a world-2 gloo group: equal shards give the mean of the
  ranks' values on both ranks, unequal shards raise ValueError on both ranks (and neither hangs)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

POLICIES = ["color", "translation", "cutout", "color,translation", "translation,cutout", "color,translation,cutout"]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("policy", POLICIES)
def test_sharded_draws_are_the_global_draw(policy, world):
    from de_i2i_gan_amd.utils.diffaug import draw_params
    n, h, w = 3, 32, 48
    torch.manual_seed(1234)
    start = torch.get_rng_state()
    ref, ref_runs = draw_params(policy, n * world, h, w)
    after = torch.get_rng_state()
    parts = []
    for rank in range(world):
        torch.set_rng_state(start)
        rec, runs = draw_params(policy, n, h, w, shard=(rank, world))
        assert runs == ref_runs
        assert rec.shape == (len(runs), n, ref.shape[2]) and rec.dtype == ref.dtype and rec.flags["C_CONTIGUOUS"]
        assert torch.equal(torch.get_rng_state(), after), (policy, world, rank)
        parts.append(rec)
    assert np.array_equal(np.concatenate(parts, axis=1), ref)


def test_unsharded_draw_is_unchanged_by_the_shard_argument():
    from de_i2i_gan_amd.utils.diffaug import draw_params
    torch.manual_seed(7)
    a, _ = draw_params("color,translation,cutout", 5, 16, 16)
    torch.manual_seed(7)
    b, _ = draw_params("color,translation,cutout", 5, 16, 16, shard=(0, 1))
    assert np.array_equal(a, b)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from de_i2i_gan_amd.stargan.solver import global_means
    terms = [torch.tensor(0.25 * (rank + 1)), torch.tensor(-3.0 * (rank + 1)), torch.tensor(1e-6 * (rank + 1))]
    res = {"equal": global_means(terms, 4)}
    try:
        global_means(terms, 2 + rank)
        res["unequal"] = "returned"
    except ValueError as e:
        res["unequal"] = "ValueError: " + str(e)
    res["after"] = global_means([torch.tensor(float(rank))], 4)          # both ranks are still in step
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_global_means_average_equal_shards_and_refuse_unequal_ones(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"r{i}.pt", weights_only=True) for i in range(world)]
    for i in range(world):
        assert np.allclose(r[i]["equal"], [0.375, -4.5, 1.5e-6], rtol=1e-7, atol=0.0), r[i]["equal"]
        assert r[i]["unequal"].startswith("ValueError"), r[i]["unequal"]
        assert r[i]["after"] == [0.5]
    assert r[0]["equal"] == r[1]["equal"]
