"""Host restatement of the library's Philox4x32-10 (csrc/cgl_common.h: cgl_philox) and of the streams built on it.

Shared by the tests that compare a device stream with the host bit for bit or value by value
(test_gpu_normal_fill.py: the N(0,1) stream; test_gpu_conv_state_ops.py: the Dropout2d masks).  The
Random123 known answers below pin the restatement itself (test_gpu_normal_fill.py checks them on the CPU)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al., SC'11; Random123) on uint32 arrays: c [..., 4] counters, k [..., 2] keys."""
    c = [np.asarray(c[..., j], dtype=np.uint64) for j in range(4)]
    k0, k1 = np.asarray(k[..., 0], dtype=np.uint64), np.asarray(k[..., 1], dtype=np.uint64)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0]
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


# Random123 kat_vectors, philox4x32 10 rounds: (counter, key, output)
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def dropout2d_mask_ref(n, p, seed, counter):
    """fp32 host value of cgl_dropout2d_mask's n = images * channels scales (cgl_dropout_mask_k): element i draws
    Philox counter (i lo, i hi, counter lo, counter hi ^ 0x5bd1e995) under key (seed lo, seed hi), u = (word 0 >> 8)
    2^-24, and is fp32(1 / fp32(1 - p)) when u < fp32(1 - p), else 0.  seed and counter are taken modulo 2^64."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    i = np.arange(n, dtype=np.uint64)
    ctr = np.stack([i & M32, i >> np.uint64(32), np.full(n, counter & 0xFFFFFFFF, dtype=np.uint64),
                    np.full(n, (counter >> 32) ^ 0x5BD1E995, dtype=np.uint64)], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    w = philox4x32_10(ctr, np.broadcast_to(key, (n, 2)))
    u = (w[:, 0] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)     # exact: 24 bits
    keep = np.float32(1.0 - p)
    scale = np.float32(1.0) / keep
    assert u.dtype == np.float32 and scale.dtype == np.float32
    return np.where(u < keep, scale, np.float32(0.0)).astype(np.float32)
