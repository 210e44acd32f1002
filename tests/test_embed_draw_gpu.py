"""Device-drawn SEAN style embeddings (csrc/embed.hip: dei2i_embed_draw, dei2i_embed_gather; ops.EmbedBank, ops.embed_draw).

Everything is compared bit for bit with ``torch.equal``; nothing needs a tolerance: the draw is integer arithmetic, checked against
the numpy Philox4x32-10 and index formula of tests/embed_reference.py, and the gather is a copy.  The bank is synthetic: label_nc = 6,
the number of embeddings per label combination drawn from {0, 1, 3, 1000}, every bank row integer-valued and unlike every other
(row r holds r + (column % 5)), so a row gathered from the wrong place cannot compare equal."""
import ctypes

import numpy as np
import pytest
import torch

import embed_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5DEECE66D1234567
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
LABEL_NC = 6
NS, EMBEDS, WIDTHS = (1, 2, 300), (1, 3, 4, 5, 9), (1, 5, 768)

_banks = {}


def synthetic(embed_nc):
    """-> (ops.EmbedBank, reference bank (total, embed_nc) float32, reference table (64, 2) int32), once per width"""
    from de_i2i_gan_amd import ops
    if embed_nc not in _banks:
        counts = np.random.RandomState(7).choice([0, 1, 3, 1000], size=1 << LABEL_NC)
        counts[[1, 2, 4, 3]] = (0, 1, 3, 1000)              # (whatever the draw gave: every count occurs, at combinations the small cases use)
        total = int(counts.sum())
        rows = (torch.arange(total, dtype=torch.float32)[:, None] + (torch.arange(embed_nc) % 5).float()[None, :])
        emb, at = {}, 0
        for combo, cnt in enumerate(counts.tolist()):
            key = tuple((combo >> (LABEL_NC - 1 - i)) & 1 for i in range(LABEL_NC))
            if combo % 7 != 5:                              # (some empty combinations are missing from the file altogether)
                emb[key] = list(rows[at:at + cnt].unbind(0))
            at += cnt if combo % 7 != 5 else 0
        ref_bank, ref_table = R.pack({k: [e.numpy() for e in v] for k, v in emb.items()}, LABEL_NC, embed_nc)
        bank = ops.EmbedBank(dict(reversed(list(emb.items()))), LABEL_NC, embed_nc, SEED, DEV)      # (the file's key order is not the layout's)
        assert bank.total == ref_bank.shape[0] and torch.equal(bank.bank.cpu(), torch.from_numpy(ref_bank))
        assert torch.equal(bank.table.cpu(), torch.from_numpy(ref_table))
        assert len(np.unique(ref_bank, axis=0)) == len(ref_bank)
        _banks[embed_nc] = (bank, ref_bank, ref_table)
    return _banks[embed_nc]


def labels_for(n, seed=3):
    """(n, 6) float32 rows of zeros and ones; the first rows are the combinations 4 (3 embeddings), 3 (1000), 1 (none), 2 (one)"""
    bits = np.random.RandomState(seed).randint(0, 2, size=(n, LABEL_NC))
    for j, combo in enumerate((4, 3, 1, 2)[:n]):
        bits[j] = [(combo >> (LABEL_NC - 1 - i)) & 1 for i in range(LABEL_NC)]
    return bits.astype(np.float32)


def want(ref_bank, ref_table, call, labels, num_embeds, row0=0):
    index = R.draw_index(SEED, call, labels, ref_table, num_embeds, row0)
    return torch.from_numpy(R.gather(ref_bank, index)), torch.from_numpy(index)


def same(got, wanted, what):
    feat, index = got
    assert feat.dtype == torch.float32 and index.dtype == torch.int32 and feat.shape == wanted[0].shape, what
    assert torch.equal(index.cpu(), wanted[1]), what
    assert torch.equal(feat.cpu(), wanted[0]), what


# ---- 1. the draw and the gather against the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("embed_nc", WIDTHS)
def test_index_and_features_equal_the_reference(embed_nc):
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(embed_nc)
    bank.rng.set_state((SEED, 0))
    call = 0
    for n in NS:
        labels = labels_for(n)
        dev = torch.from_numpy(labels).to(DEV)
        for num_embeds in EMBEDS:
            got = ops.embed_draw(bank, dev, num_embeds)
            assert tuple(got[0].shape) == (n, num_embeds, embed_nc) and (got[0].data_ptr() % 16 == 0)
            same(got, want(ref_bank, ref_table, call, labels, num_embeds), (n, num_embeds))
            call += 1
    assert bank.rng.state() == (SEED, call)
    hit = want(ref_bank, ref_table, 0, labels_for(300), 9)[1]
    assert (hit == -1).any() and (hit >= 0).any() and int(hit.max()) > 1000       # empty lists, and draws deep inside a long one


def test_label_forms_and_dtypes_draw_the_same():
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(5)
    labels = labels_for(7)
    wanted = want(ref_bank, ref_table, 11, labels, 4)
    base = torch.from_numpy(labels).to(DEV)
    forms = [base, base.reshape(7, LABEL_NC, 1, 1), base.long(), base.to(torch.int32), base.to(torch.uint8), base.bfloat16(), base.half(),
             base.double(), torch.cat([base, base], 1)[:, :LABEL_NC], base + 0.75]      # (a view that is not contiguous; (int) truncates)
    before = bank.invalid()
    for form in forms:
        bank.rng.set_state((SEED, 11))
        same(ops.embed_draw(bank, form, 4), wanted, (form.dtype, tuple(form.shape)))
    assert bank.invalid() == before


def test_unaligned_output_takes_the_scalar_path():
    """an output one float past an aligned address with embed_nc % 4 == 0: float4 stores would fault or misplace"""
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(768)
    index = torch.from_numpy(R.draw_index(SEED, 5, labels_for(10), ref_table, 3)).to(DEV)
    flat = torch.full((30 * 768 + 2,), -7.0, device=DEV)
    out = flat[1:-1]
    assert out.data_ptr() % 16 == 4 and bank.bank.data_ptr() % 16 == 0
    lib = ops._lib_for(flat)
    assert lib.dei2i_embed_gather(30, 768, ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(bank.bank.data_ptr()), bank.bank.shape[0],
                                  ctypes.c_void_p(out.data_ptr()), ops._stream()) == 0
    assert torch.equal(out.view(10, 3, 768).cpu(), torch.from_numpy(R.gather(ref_bank, index.cpu().numpy())))
    assert flat[0].item() == -7.0 and flat[-1].item() == -7.0
    src = bank.bank.reshape(-1)                               # ... and a bank one float past it
    shifted = torch.empty(src.numel() + 1, device=DEV)
    shifted[1:].copy_(src)
    out2 = torch.empty(30, 768, device=DEV)
    assert lib.dei2i_embed_gather(30, 768, ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(shifted[1:].data_ptr()), bank.bank.shape[0],
                                  ctypes.c_void_p(out2.data_ptr()), ops._stream()) == 0
    assert torch.equal(out2, out.view(30, 768))


# ---- 2. the counter --------------------------------------------------------------------------------------------------------
def test_counter_goes_up_by_one_per_call_and_carries():
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(5)
    labels = labels_for(6)
    dev = torch.from_numpy(labels).to(DEV)
    bank.rng.set_state((SEED, 0))
    first = ops.embed_draw(bank, dev, 5)
    assert bank.rng.state() == (SEED, 1)
    second = ops.embed_draw(bank, dev, 5)
    assert bank.rng.state() == (SEED, 2)
    same(first, want(ref_bank, ref_table, 0, labels, 5), "call 0")
    same(second, want(ref_bank, ref_table, 1, labels, 5), "call 1")
    assert not torch.equal(first[1], second[1])
    bank.rng.set_state((SEED, 2 ** 32 - 1))                 # the next launch carries into the high counter word
    same(ops.embed_draw(bank, dev, 5), want(ref_bank, ref_table, 2 ** 32 - 1, labels, 5), "call 2^32 - 1")
    assert bank.rng.state() == (SEED, 2 ** 32)
    same(ops.embed_draw(bank, dev, 5), want(ref_bank, ref_table, 2 ** 32, labels, 5), "call 2^32")
    assert bank.rng.state() == (SEED, 2 ** 32 + 1)
    other = ops.EmbedBank({}, LABEL_NC, 5, SEED + 1, DEV)   # another seed, and a bank without a single embedding
    assert other.rng.state() == (SEED + 1, 0) and other.total == 0 and other.invalid() == 0
    feat, index = ops.embed_draw(other, dev, 5)
    assert bool((index == -1).all()) and not feat.any() and other.rng.state() == (SEED + 1, 1)


# ---- 3. empty lists and invalid rows -------------------------------------------------------------------------------------------
def test_empty_lists_give_zeros_and_index_minus_one():
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(768)
    empty = [c for c in range(1 << LABEL_NC) if ref_table[c, 1] == 0][:5]
    assert 1 in empty and len(empty) >= 2
    labels = np.array([[(c >> (LABEL_NC - 1 - i)) & 1 for i in range(LABEL_NC)] for c in empty + [4]], dtype=np.float32)
    before = bank.invalid()
    feat, index = ops.embed_draw(bank, torch.from_numpy(labels).to(DEV), 9)
    assert bool((index[:-1] == -1).all()) and not feat[:-1].any()
    assert bool((index[-1] >= 0).all()) and bool((feat[-1] != 0).any(dim=1).all())
    assert bank.invalid() == before                          # (an empty list is no invalid row)


def test_invalid_rows_give_zeros_and_are_counted():
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(5)
    labels = labels_for(300)
    bad = {1: 2.0, 7: -1.0, 256: 2.0, 299: -1.0, 100: float("nan"), 101: float("inf"), 102: 3e9}
    for row, value in bad.items():
        labels[row, row % LABEL_NC] = value
    labels[7, 0] = 2.0                                        # (two bad labels in one row: counted once)
    bank.rng.set_state((SEED, 21))
    before = bank.invalid()
    got = ops.embed_draw(bank, torch.from_numpy(labels).to(DEV), 5)
    assert bank.invalid() == before + len(bad)
    same(got, want(ref_bank, ref_table, 21, labels, 5), "invalid rows")
    rows = sorted(bad)
    assert bool((got[1][rows] == -1).all()) and not got[0][rows].any()
    clean = labels_for(300)
    keep = [r for r in range(300) if r not in bad]
    assert torch.equal(got[1].cpu()[keep], want(ref_bank, ref_table, 21, clean, 5)[1][keep])      # the valid rows do not move
    ops.embed_draw(bank, torch.from_numpy(labels[:8]).to(DEV), 1)
    assert bank.invalid() == before + len(bad) + 2           # (rows 1 and 7)


# ---- 4. rows of the global batch -------------------------------------------------------------------------------------------
def test_rows_are_a_slice_of_the_whole_batch():
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(5)
    labels = labels_for(5)
    labels[3] = labels[1]                                     # (rows 1 and 3: the combination with 1000 embeddings)
    dev = torch.from_numpy(labels).to(DEV)
    bank.rng.set_state((SEED, 7))
    whole = ops.embed_draw(bank, dev, 9)
    assert not torch.equal(whole[1][1], whole[1][3])          # (the same labels in another row draw other embeddings)
    bank.rng.set_state((SEED, 7))
    part = ops.embed_draw(bank, dev[2:5], 9, row0=2)
    assert torch.equal(part[1], whole[1][2:5]) and torch.equal(part[0], whole[0][2:5])
    same(part, want(ref_bank, ref_table, 7, labels[2:5], 9, row0=2), "rows [2, 5)")
    bank.rng.set_state((SEED, 7))
    assert not torch.equal(ops.embed_draw(bank, dev[2:5], 9)[1], part[1])       # (row0 is part of the counter)


# ---- 5. the gather tolerates any index --------------------------------------------------------------------------------------
@pytest.mark.parametrize("embed_nc", [5, 768])
def test_gather_writes_zeros_for_an_index_off_the_bank_and_stays_inside_its_output(embed_nc):
    """indices a caller may hand over: -1, bank_rows, 2^31 - 1, the most negative one.  No address is formed from them (the kernel
    compares before it multiplies), and the cells around the output keep their value."""
    from de_i2i_gan_amd import ops
    bank, ref_bank, ref_table = synthetic(embed_nc)
    rows = bank.bank.shape[0]
    hand = [0, -1, rows - 1, rows, 2 ** 31 - 1, 5, -2 ** 31, rows + 1, 1]
    index = torch.tensor(hand, dtype=torch.int32, device=DEV)
    guard = 64
    flat = torch.full((guard + len(hand) * embed_nc + guard,), -7.0, device=DEV)
    out = flat[guard:guard + len(hand) * embed_nc]
    lib = ops._lib_for(flat)
    assert lib.dei2i_embed_gather(len(hand), embed_nc, ctypes.c_void_p(index.data_ptr()), ctypes.c_void_p(bank.bank.data_ptr()), rows,
                                  ctypes.c_void_p(out.data_ptr()), ops._stream()) == 0
    got = out.view(len(hand), embed_nc).cpu()
    assert torch.equal(got, torch.from_numpy(R.gather(ref_bank, np.array(hand))))
    for r, idx in enumerate(hand):
        assert bool(got[r].any()) == (0 <= idx < rows), (r, idx)
    assert bool((flat[:guard] == -7.0).all()) and bool((flat[-guard:] == -7.0).all())


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing():
    from de_i2i_gan_amd import ops
    bank, _, _ = synthetic(5)
    bank.rng.set_state((SEED, 40))
    labels = torch.from_numpy(labels_for(4)).to(DEV)
    index = torch.full((4, 3), -9, dtype=torch.int32, device=DEV)
    feat = torch.full((12, 5), -9.0, device=DEV)
    invalid = bank.invalid()
    lib = ops._lib_for(feat)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()

    def draw(counter=p(bank.rng.counter), n=4, row0=0, label_nc=LABEL_NC, num_embeds=3, lab=p(labels), tab=p(bank.table), total=bank.total,
             idx=p(index), inv=p(bank.invalid_word)):
        return lib.dei2i_embed_draw(SEED, counter, n, row0, label_nc, num_embeds, lab, tab, total, idx, inv, st)

    for bad in (dict(counter=None), dict(lab=None), dict(tab=None), dict(idx=None), dict(inv=None), dict(n=0), dict(n=-1), dict(row0=-1),
                dict(n=2, row0=2 ** 31 - 1), dict(label_nc=0), dict(label_nc=17), dict(num_embeds=0), dict(num_embeds=-3), dict(total=-1)):
        assert draw(**bad) == BAD_ARG, bad

    def gather(rows=12, embed_nc=5, idx=p(index), src=p(bank.bank), bank_rows=bank.bank.shape[0], dst=p(feat)):
        return lib.dei2i_embed_gather(rows, embed_nc, idx, src, bank_rows, dst, st)

    for bad in (dict(idx=None), dict(src=None), dict(dst=None), dict(rows=0), dict(rows=-1), dict(embed_nc=0), dict(bank_rows=0),
                dict(rows=2 ** 40), dict(rows=2 ** 38, embed_nc=4), dict(bank_rows=2 ** 40), dict(bank_rows=2 ** 38, embed_nc=4),
                dict(rows=2 ** 62, embed_nc=2 ** 30)):
        assert gather(**bad) == BAD_ARG, bad
    torch.cuda.synchronize()
    assert bool((index == -9).all()) and bool((feat == -9.0).all())      # the sentinels
    assert bank.rng.state() == (SEED, 40) and bank.invalid() == invalid
    assert draw() == 0 and gather() == 0                                 # ... and the same calls with good arguments run
    assert bank.rng.state() == (SEED, 41) and bool((index != -9).all()) and bool((feat != -9.0).all())

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.embed_draw(bank, labels.cpu(), 3)
    for shape in ((4, 5), (4, 6, 2, 2), (4 * 6,), (0, 6)):
        with pytest.raises(ValueError, match="labels of shape"):
            ops.embed_draw(bank, torch.zeros(shape, device=DEV), 3)
    with pytest.raises(ValueError, match="num_embeds"):
        ops.embed_draw(bank, labels, 0)
    with pytest.raises(TypeError):
        ops.embed_draw(bank, labels.bool(), 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.EmbedBank({}, LABEL_NC, 5, 1, "cpu")
    with pytest.raises(ValueError, match="label_nc 17"):
        ops.EmbedBank({}, 17, 5, 1, DEV)
    assert bank.rng.state() == (SEED, 41)


def test_digest_follows_every_bit_of_the_bank_and_the_table():
    import digest_reference
    from de_i2i_gan_amd import ops
    emb = {(0, 1): [torch.tensor([1.0, 2.0, 3.0]), torch.tensor([4.0, 5.0, 6.0])], (1, 0): [torch.tensor([7.0, 8.0, 9.0])]}
    a, b = ops.EmbedBank(emb, 2, 3, 1, DEV), ops.EmbedBank(emb, 2, 3, 99, DEV)
    assert int(a.digest().item()) == int(b.digest().item())             # (the seed is no part of it)
    emb[(1, 0)][0][2] = 9.5
    c = ops.EmbedBank(emb, 2, 3, 1, DEV)
    moved = ops.EmbedBank({(1, 1): emb[(0, 1)], (1, 0): emb[(1, 0)]}, 2, 3, 1, DEV)
    words = {int(x.digest().item()) for x in (a, c, moved)}
    assert len(words) == 3
    assert int(a.digest().item()) & (2 ** 64 - 1) == digest_reference.digest([a.bank.cpu().numpy(), a.table.cpu().numpy()])
