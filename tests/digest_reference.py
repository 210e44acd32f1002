"""numpy reference of the state digest (include/dei2i_hip.h): every 32-bit word of a list of arrays reduced to one 64-bit word,
    digest = sum_k sum_i splitmix64(splitmix64((k << 32) | i) + w[k][i])  mod 2^64.
uint64 arithmetic wraps in numpy, which is the arithmetic the definition asks for."""
import numpy as np

SPLITMIX64_OF_ZERO = 0xE220A8397B1DCDAF
DIGEST_OF_ONE_FP32_ZERO = 0xA706DD2F4D197E6F


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def words_of(array):
    """the memory of a C-contiguous numpy array as 32-bit words"""
    a = np.ascontiguousarray(array)
    assert a.nbytes % 4 == 0, a.nbytes
    return a.reshape(-1).view(np.uint32) if a.size else np.zeros(0, np.uint32)


def digest(arrays, row0=0):
    """-> int in [0, 2^64): the digest of the list, array j taking place k = row0 + j"""
    total = np.uint64(0)
    with np.errstate(over="ignore"):
        for j, a in enumerate(arrays):
            w = words_of(a).astype(np.uint64)
            at = (np.uint64(row0 + j) << np.uint64(32)) | np.arange(w.size, dtype=np.uint64)
            total = total + np.sum(splitmix64(splitmix64(at) + w), dtype=np.uint64)
    return int(total)


def of_tensors(tensors, row0=0):
    """the same for torch tensors (any device, any 4-byte-multiple dtype): their bytes, through a uint8 view"""
    import torch
    return digest([t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy() for t in tensors], row0)
