"""The state digest's rule in numpy, written from DESIGN.md section 17 (not from csrc/digest.hip): what tests/test_digest_cpu.py
examines on its own and tests/test_digest_gpu.py holds the kernel to, bit for bit.

    The operand is a contiguous view of n 16-bit words.  Its bytes are zero-padded to a multiple of 8 and read as little-endian u64
    chunks q_c, c = 0 .. ceil(n / 4) - 1, counted from the view's first word.  With all arithmetic mod 2^64:
        z = c + 0x9E3779B97F4A7C15 * (salt + 1)
        z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9
        z = (z ^ z >> 27) * 0x94D049BB133111EB
        z ^= z >> 31
        digest = sum_c (q_c + 1) * (z | 1) + n * 0xD1B54A32D192ED03
"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN, MUL1, MUL2, LENGTH = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD1B54A32D192ED03


def chunks(words) -> np.ndarray:
    """The u64 chunks q_c of a 1-d array of 16-bit words (any 2-byte dtype: the bits count)."""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint16)
    n = w.size
    padded = np.zeros((n + 3) // 4 * 4, dtype="<u2")
    padded[:n] = w
    return padded.view("<u8").astype(np.uint64)


def weights(count: int, salt: int = 0) -> np.ndarray:
    """z | 1 for c = 0 .. count - 1 (uint64 array arithmetic wraps)."""
    key = np.uint64((GOLDEN * ((int(salt) & M64) + 1)) & M64)
    z = np.arange(count, dtype=np.uint64) + key
    z = (z ^ (z >> np.uint64(30))) * np.uint64(MUL1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(MUL2)
    z = z ^ (z >> np.uint64(31))
    return z | np.uint64(1)


def terms(words, salt: int = 0) -> np.ndarray:
    q = chunks(words)
    return (q + np.uint64(1)) * weights(q.size, salt)


def digest(words, salt: int = 0) -> int:
    """The digest as a Python int in [0, 2^64)."""
    n = np.ascontiguousarray(words).size
    if n == 0:
        raise ValueError("an empty view has no digest")
    total = int(np.add.reduce(terms(words, salt), dtype=np.uint64))
    return (total + n * LENGTH) & M64


def digest_python(words, salt: int = 0) -> int:
    """The same rule chunk by chunk in Python integers (slow; the check of the vectorised form on small inputs)."""
    w = [int(x) for x in np.ascontiguousarray(words).reshape(-1).view(np.uint16)]
    n = len(w)
    w += [0] * (-n % 4)
    total = 0
    for c in range(len(w) // 4):
        q = w[4 * c] | w[4 * c + 1] << 16 | w[4 * c + 2] << 32 | w[4 * c + 3] << 48
        z = (c + GOLDEN * ((salt & M64) + 1)) & M64
        z = ((z ^ z >> 30) * MUL1) & M64
        z = ((z ^ z >> 27) * MUL2) & M64
        z ^= z >> 31
        total = (total + (q + 1) * (z | 1)) & M64
    return (total + n * LENGTH) & M64
