"""numpy reference of the device-drawn SEAN style embeddings (include/dei2i_hip.h: dei2i_embed_draw, dei2i_embed_gather): the
Philox4x32-10 of tests/test_mask_dev_gpu.py, the combination index of a label row, the index formula and the gather.  Integer
arithmetic and copies only: every comparison against it is exact."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
EMBED_STREAM = 0xA0000000          # counter word c2 of slot quad q: EMBED_STREAM | q


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two uint32 scalars -> four uint32 arrays (Salmon et al. 2011)"""
    c = list(np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & LOW for v in ctr]))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & LOW, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & LOW]
        k0, k1 = (k0 + np.uint64(W0)) & LOW, (k1 + np.uint64(W1)) & LOW
    return [v.astype(np.uint32) for v in c]


def draw_words(seed, call, n, row0, num_embeds):
    """-> uint64 (n, num_embeds): the 32-bit word of slot e of global row row0 + i -- word x[e % 4] of the block whose counter is
    (call low, call high, EMBED_STREAM | e // 4, row0 + i) under the key (seed low, seed high)"""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    e = np.arange(num_embeds, dtype=np.uint64)
    rows = np.arange(row0, row0 + n, dtype=np.uint64)
    blocks = philox4x32_10((call & 0xFFFFFFFF, call >> 32, np.uint64(EMBED_STREAM) | (e[None, :] // np.uint64(4)), rows[:, None]), key)
    words = np.stack(blocks, -1).astype(np.uint64)                                      # (n, num_embeds, 4)
    pick = np.broadcast_to((e % np.uint64(4)).astype(np.int64)[None, :, None], (n, num_embeds, 1))
    return np.take_along_axis(words, pick, -1)[..., 0]


def combinations(labels):
    """labels (n, label_nc) float -> (combo int64 (n,), valid bool (n,)): b_i = trunc(labels[i]), the first label the slowest
    digit; a row with some b_i outside {0, 1} (or a NaN) is invalid (its combo is 0 here and never used)"""
    labels = np.asarray(labels, dtype=np.float64)
    n, label_nc = labels.shape
    with np.errstate(invalid="ignore"):
        bits = np.trunc(labels)
    valid = np.all((bits == 0) | (bits == 1), axis=1)
    bits = np.where(valid[:, None], bits, 0).astype(np.int64)
    weights = np.int64(1) << np.arange(label_nc - 1, -1, -1, dtype=np.int64)
    return (bits * weights[None, :]).sum(1), valid


def draw_index(seed, call, labels, table, num_embeds, row0=0):
    """-> int32 (n, num_embeds): offset + (word * count >> 32) of the row's combination; -1 for an empty combination or an invalid
    row.  ``table``: int (1 << label_nc, 2) of (offset, count)."""
    table = np.asarray(table, dtype=np.int64)
    combo, valid = combinations(labels)
    n = combo.shape[0]
    offset, count = table[combo, 0], np.where(valid, table[combo, 1], 0)
    words = draw_words(seed, call, n, row0, num_embeds)
    index = offset[:, None] + ((words * count.astype(np.uint64)[:, None]) >> np.uint64(32)).astype(np.int64)
    return np.where(count[:, None] > 0, index, -1).astype(np.int32)


def gather(bank, index):
    """-> float32 index.shape + (embed_nc,): bank[index], zeros where the index lies outside [0, len(bank))"""
    bank = np.asarray(bank, dtype=np.float32)
    index = np.asarray(index, dtype=np.int64)
    hit = (index >= 0) & (index < bank.shape[0])
    out = bank[np.where(hit, index, 0)]
    out[~hit] = 0
    return out


def pack(embeddings, label_nc, embed_nc):
    """{label tuple: [array (embed_nc,), ...]} -> (bank float32 (total, embed_nc), table int32 (1 << label_nc, 2)): ascending
    combination index, list order inside a combination, a missing key an empty list"""
    table = np.zeros((1 << label_nc, 2), dtype=np.int32)
    rows = []
    by_combo = {}
    for key, embeds in embeddings.items():
        combo = 0
        for b in key:
            combo = (combo << 1) | int(b)
        by_combo[combo] = embeds
    for combo in sorted(by_combo):
        if not len(by_combo[combo]):
            continue                                          # (an empty list stays (0, 0), like a missing key)
        table[combo] = (len(rows), len(by_combo[combo]))
        rows.extend(np.asarray(e, dtype=np.float32) for e in by_combo[combo])
    bank = np.stack(rows) if rows else np.zeros((0, embed_nc), dtype=np.float32)
    return bank, table
