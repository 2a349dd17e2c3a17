"""Host restatement of the library's shuffle sampler (csrc/cgl_common.h: cgl_hash, cgl_permute) and of the conv
round's real-batch sampler built on it (csrc/cgl_conv.hip: cgl_sample_rows_at).

Shared by test_gpu_short_batch.py (the MLP round's prologue sampler) and test_gpu_conv_state_ops.py
(cgl_sample_rows_dev).  Plain Python integers, masked to 32 bits where the device wraps."""
M32 = 0xFFFFFFFF


def _hash(x, k):
    x ^= k
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def _permute(i, n, key):
    """cgl_permute (csrc/cgl_common.h): 4-round Feistel on the smallest even bit width >= log2 n,
    cycle-walked into [0, n)."""
    bits = 2
    while (1 << bits) < n:
        bits += 1
    bits += bits & 1
    hb = bits // 2
    mask = (1 << hb) - 1
    x = i
    while True:
        l, r = x >> hb, x & mask
        for rnd in range(4):
            t = l ^ (_hash(r, (key + 0x9E3779B9 * (rnd + 1)) & M32) & mask)
            l, r = r, t
        x = (l << hb) | r
        if x < n:
            return x


def conv_batch(n_src, nrows, seed, rnd, drop_last=False):
    """(source row of each of the nrows destination rows, real rows) of cgl_sample_rows_dev's round ``rnd``.

    DataLoader mode: a pass is ceil(n_src / nrows) rounds, batch b of pass ep takes positions b nrows + r of the
    pass's permutation (key = low word of the seed ^ (ep 0x85ebca6b + 0x1234567) mod 2^32); positions past the end
    repeat the last one (padding), and the real rows are min(nrows, n_src - b nrows).
    drop_last: a pass is n_src // nrows whole batches; position round nrows + r of the stream, pass = position //
    (whole batches nrows).  The real rows are then always nrows."""
    if drop_last:
        per = (n_src // nrows) * nrows
        pos = [rnd * nrows + r for r in range(nrows)]
        eps, js, nv = [q // per for q in pos], [q % per for q in pos], nrows
    else:
        nb = (n_src + nrows - 1) // nrows
        ep, b = rnd // nb, rnd % nb
        js = [min(b * nrows + r, n_src - 1) for r in range(nrows)]
        eps, nv = [ep] * nrows, min(nrows, n_src - b * nrows)
    idx = []
    for ep, j in zip(eps, js):
        key = (seed & M32) ^ (((ep & M32) * 0x85EBCA6B + 0x1234567) & M32)
        idx.append(_permute(j, n_src, key))
    return idx, nv
