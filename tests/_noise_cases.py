"""Shared by tests/test_seed_seq_host.py, tests/test_noise_host.py and tests/test_noise_gpu.py: the entropy list, numpy's
coercion of an entropy to uint32 words, numpy's noise as the reference, and the margin of the decline tests."""
import numpy as np

from trajectory_generation_amd.dataset import schema as S

ZIG_R = 3.6541528853610087963519472518      # the ziggurat's tail starts here (csrc/gen_rng.h ZIG_NOR_R)
DECLINE_MARGIN = 3e-4      # declines some of ids 0..63 at 129 rows, not all (tests/test_noise_host.py checks it on the CPU)

ENTROPIES = [0, 1, 12345, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 63 - 1, [0, 5], [7, 0], [2 ** 33, 1],
             [0x01234567, 0x89abcdef, 0xdeadbeef, 0x0badcafe],
             [5, 4, 3, 2, 1],
             [0xffffffff, 0, 0x80000000, 1, 2, 3, 0x7fffffff, 0xfffffffe]]


def coerce(entropy):
    """numpy's coercion of an int or a sequence of ints to uint32 words: little-endian, at least one word per int."""
    words = []
    for v in ([entropy] if isinstance(entropy, int) else entropy):
        if v < 0:
            raise ValueError("expected non-negative integer")
        words.append(v & 0xffffffff)
        v >>= 32
        while v:
            words.append(v & 0xffffffff)
            v >>= 32
    return np.array(words, dtype=np.uint32)



def numpy_noise(ids, n, stds=None, seed_base=S.NOISE_SEED_BASE):
    return np.stack([S.measurement_noise(int(i), n, stds, seed_base) for i in ids])
