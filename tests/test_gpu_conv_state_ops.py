"""Op-level references for the small kernels around the conv round's convolutions: the
Dropout2d masks, the real-batch sampler, multi-tensor Adam, the adversarial loss head, the ticketed reductions'
scratch reuse, and the layout / gather / column-sum utilities.  They decide what data a round sees, which
activations are dropped, how the loss is averaged and how the parameters move; whole-round parity at two batch
sizes cannot tell a wrong counter word or a wrong mean divisor from noise.

Conventions of this file:
  * every output buffer is followed by SENT sentinel words that must come back unchanged;
  * references are computed on the CPU from the same fp32 inputs the kernel gets;
  * u = 2^-24, the unit roundoff of fp32 (one rounding to nearest: relative error <= u).  hipcc's default
    correctly rounded fp32 division and sqrtf are one rounding each; expf / logf are taken at 2 ulp, i.e. a relative
    error of the result of at most 4u.  Every bound below is derived from the kernel's operation sequence next to
    the code that evaluates it; none is fitted to a measurement.  Measured worst ratios are in DESIGN.md section 5a.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

from philox_ref import dropout2d_mask_ref
from sampler_ref import conv_batch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENT = 64
PAT32 = 0x7FBADBAD                # a NaN bit pattern no kernel writes
PAT64 = 0x7FF0BADBADBADBAD


def ops():
    from cglgan import conv_ops
    return conv_ops


def padded(n, dtype=torch.float32):
    """n elements followed by SENT sentinel words, all pre-filled with a NaN pattern: (view of the n, whole buffer)."""
    if dtype == torch.float64:
        buf = torch.full((n + SENT,), PAT64, dtype=torch.int64, device=DEV).view(torch.float64)
    else:
        buf = torch.full((n + SENT,), PAT32, dtype=torch.int32, device=DEV).view(dtype)
    return buf[:n], buf


def sent_ok(buf, n, what=""):
    tail = buf[n:]
    pat = PAT64 if buf.dtype == torch.float64 else PAT32
    it = torch.int64 if buf.dtype == torch.float64 else torch.int32
    assert bool((tail.view(it) == pat).all()), f"{what}: sentinel words after the buffer were overwritten"


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def _batch(on):
    return ops().launch_batch() if on else contextlib.nullcontext()


# =====================================================================================================================
# a. Dropout2d masks: bit-exact against the host Philox (philox_ref.dropout2d_mask_ref)
# =====================================================================================================================
MASK_SHAPES = [(1, 1), (3, 85), (4, 64), (257, 1), (64, 128)]          # 1, 255, 256, 257 and 8192 elements
SEEDS = [1234, 2 ** 63 + 5]
COUNTERS = [7, 2 ** 32 + 7, 2 ** 64 - 1]


def _ref_mask(n, p, seed, ctr):
    return torch.from_numpy(dropout2d_mask_ref(n, p, seed, ctr))


@pytest.mark.parametrize("p", [0.0, 0.25, 0.5, 0.999])
@pytest.mark.parametrize("n,c", MASK_SHAPES)
def test_dropout2d_mask_bit_exact(n, c, p):
    """cgl_dropout2d_mask equals the host restatement bit for bit for every (seed, counter), the high halves of both
    included (a dropped high word, a wrong counter word or a different u -> keep comparison changes elements)."""
    O = ops()
    seen = []
    for seed in SEEDS:
        for ctr in COUNTERS:
            m, buf = padded(n * c)
            O.dropout2d_mask(m, n, c, p, seed, ctr)
            torch.cuda.synchronize()
            sent_ok(buf, n * c, "mask")
            got = m.cpu()
            assert torch.equal(bits(got), bits(_ref_mask(n * c, p, seed, ctr))), (seed, ctr)
            seen.append(got)
    if n * c >= 255 and 0.0 < p < 0.999:      # the six (seed, counter) streams are six different masks
        for i in range(len(seen)):
            for j in range(i):
                assert not torch.equal(seen[i], seen[j]), (i, j)
    if p == 0.0:
        assert bool((seen[0] == 1.0).all())


def _mask_list(nm):
    """nm (images, channels) pairs cycling through MASK_SHAPES from its second entry, so that a mask's first block
    follows masks of 255, 1, 256, 257 ... elements: block ranges that begin after a partly filled block, after a
    full one and after a two-block mask whose second block holds one element."""
    shapes = [MASK_SHAPES[(j + 1) % len(MASK_SHAPES)] for j in range(nm)]
    ctrs = [COUNTERS[j % 3] - 3 * j if j % 3 == 2 else COUNTERS[j % 3] + 11 * j for j in range(nm)]
    return shapes, ctrs


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("nm", [1, 5, 16])
def test_dropout2d_masks_equal_single_calls(nm, batch):
    """Mask j of the one-launch form is bitwise cgl_dropout2d_mask(n[j], C[j], p, seed, counters[j]) and the host
    reference, stand-alone and inside a launch batch (an off-by-one block range shifts or truncates a mask)."""
    O = ops()
    shapes, ctrs = _mask_list(nm)
    for p, seed in ((0.25, SEEDS[0]), (0.5, SEEDS[1])):
        pads = [padded(n * c) for n, c in shapes]
        with _batch(batch):
            O.dropout2d_masks([m for m, _ in pads], [n for n, _ in shapes], [c for _, c in shapes], p, seed, ctrs)
        singles = []
        for (n, c), ctr in zip(shapes, ctrs):
            s, sb = padded(n * c)
            O.dropout2d_mask(s, n, c, p, seed, ctr)
            singles.append((s, sb))
        torch.cuda.synchronize()
        for j, ((n, c), ctr) in enumerate(zip(shapes, ctrs)):
            sent_ok(pads[j][1], n * c, f"mask {j}")
            sent_ok(singles[j][1], n * c, f"single mask {j}")
            assert same_bits(pads[j][0], singles[j][0]), j
            assert torch.equal(bits(pads[j][0].cpu()), bits(_ref_mask(n * c, p, seed, ctr))), j


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("rnd", [0, 1, 7])
def test_dropout2d_masks_dev_counter_carry(rnd, batch):
    """counter j = counters[j] + round_stride * (*round_dev) in 64-bit arithmetic: bitwise cgl_dropout2d_masks with
    the summed counters.  At round 7 mask 0's sum carries from the low into the high counter word (2^32 - 3 + 7,
    and 2^32 - 3 + 7 (2^31 + 1) with the large stride) and mask 2's wraps past 2^64."""
    O = ops()
    shapes = [(3, 85), (4, 64), (257, 1), (64, 128), (1, 1)]
    base = [2 ** 32 - 3, 5, 2 ** 64 - 2, 2 ** 33 + 1, 2 ** 63]
    rd = torch.tensor([rnd, -1], dtype=torch.int32, device=DEV)
    for stride in (1, 2 ** 31 + 1):
        summed = [(b + stride * rnd) % 2 ** 64 for b in base]
        a = [padded(n * c) for n, c in shapes]
        b = [padded(n * c) for n, c in shapes]
        ns, cs = [n for n, _ in shapes], [c for _, c in shapes]
        with _batch(batch):
            O.dropout2d_masks_dev([m for m, _ in a], ns, cs, 0.25, SEEDS[1], base, rd, stride)
        O.dropout2d_masks([m for m, _ in b], ns, cs, 0.25, SEEDS[1], summed)
        torch.cuda.synchronize()
        for j, (n, c) in enumerate(shapes):
            sent_ok(a[j][1], n * c, f"dev mask {j}")
            assert same_bits(a[j][0], b[j][0]), (stride, j)
            assert torch.equal(bits(a[j][0].cpu()), bits(_ref_mask(n * c, 0.25, SEEDS[1], summed[j]))), (stride, j)


# =====================================================================================================================
# b. cgl_sample_rows_dev: the real-batch sampler
# =====================================================================================================================
N_SRC = [1, 2, 3, 4, 5, 15, 16, 17, 27, 63, 64, 65, 255, 256, 257, 1000, 4097]
WIDE = {(27, 8), (257, 64), (5, 3), (64, 1)}       # the cases that run with 1024-float rows (the conv round's width)
SAMPLER_SEED = 20211212


def _row_floats(n_src, nrows):
    return 1024 if (n_src, nrows) in WIDE else (4 if n_src % 2 else 8)


def _sample(n_src, nrows, rowf, seed, rounds, drop_last=False, batch=False):
    """cgl_sample_rows_dev for every round of ``rounds`` (device int32), each into its own slot of one sentinel-
    terminated buffer, launched LAST SLOT FIRST -- a row written past its slot would land in a slot that is already
    filled and show below.  Source row i holds i in every column, so a copied row names its source and a torn row
    shows.  Returns (source index of every destination row [R, nrows], real rows [R] or None)."""
    O = ops()
    R = len(rounds)
    src = torch.arange(n_src, dtype=torch.float32).view(-1, 1).expand(n_src, rowf).contiguous().to(DEV)
    rd = torch.tensor(rounds, dtype=torch.int32, device=DEV)
    dst, dbuf = padded(R * nrows * rowf)
    nv, nbuf = padded(R, torch.int32)
    slots = dst.view(R, nrows, rowf)
    for k in reversed(range(R)):
        with _batch(batch):
            O.sample_rows_dev(src, nrows, seed, rd[k:k + 1], slots[k], None if drop_last else nv[k:k + 1])
    torch.cuda.synchronize()
    sent_ok(dbuf, R * nrows * rowf, "sampled rows")
    sent_ok(nbuf, R, "nv_out")
    rows = slots.cpu()
    assert bool((rows == rows[..., :1]).all()), "a destination row mixes two source rows (or was not written)"
    idx = rows[..., 0]
    assert bool(((idx >= 0) & (idx < n_src) & (idx == idx.floor())).all()), "a destination row is no source row"
    if drop_last:
        assert bool((nv.view(torch.int32) == PAT32).all())
        return idx.long(), None
    return idx.long(), nv.cpu().long()


@pytest.mark.parametrize("nrows", [1, 3, 8, 64])
def test_sampler_passes_and_host_restatement(nrows):
    """DataLoader(shuffle=True) semantics from the device alone, then index-for-index equality with the host
    restatement (sampler_ref.conv_batch), for n_src at and around the powers of four where the Feistel width grows,
    n_src < nrows and n_src = 1."""
    for n_src in N_SRC:
        rowf = _row_floats(n_src, nrows)
        nb = (n_src + nrows - 1) // nrows
        rounds = list(range(2 * nb + 1))
        idx, nv = _sample(n_src, nrows, rowf, SAMPLER_SEED, rounds)
        last = n_src - (nb - 1) * nrows          # n_src mod nrows, or nrows (n_src < nrows: n_src, every round)
        assert nv.tolist() == ([nrows] * (nb - 1) + [last]) * 2 + [nrows if nb > 1 else last], (n_src, nv.tolist())
        passes = []
        for ps in range(2):
            seq = [int(i) for k in range(ps * nb, (ps + 1) * nb) for i in idx[k, :nv[k]]]
            assert sorted(seq) == list(range(n_src)), f"n_src {n_src}: pass {ps} is no permutation of the rows"
            passes.append(seq)
        if n_src >= 16:
            assert passes[0] != passes[1], f"n_src {n_src}: two passes in the same order (the pass does not key it)"
            other, _ = _sample(n_src, nrows, rowf, SAMPLER_SEED + 1, rounds[:nb])
            assert other.tolist() != idx[:nb].tolist(), f"n_src {n_src}: the seed does not key the permutation"
        for k, r in enumerate(rounds):
            hidx, hnv = conv_batch(n_src, nrows, SAMPLER_SEED, r)
            assert hnv == int(nv[k]) and hidx == idx[k].tolist(), (n_src, r)


@pytest.mark.parametrize("nrows", [1, 3, 8, 64])
def test_sampler_drop_last(nrows):
    """nv_out null: whole batches only.  A pass of n_src // nrows rounds returns that many * nrows distinct rows, the
    next pass is keyed anew, and every index equals the host restatement."""
    for n_src in [n for n in N_SRC if n >= nrows]:
        rowf = _row_floats(n_src, nrows)
        per = n_src // nrows
        rounds = list(range(2 * per + 1))
        idx, _ = _sample(n_src, nrows, rowf, SAMPLER_SEED, rounds, drop_last=True)
        passes = [idx[ps * per:(ps + 1) * per].reshape(-1).tolist() for ps in range(2)]
        for seq in passes:
            assert len(set(seq)) == per * nrows, f"n_src {n_src}: a drop_last pass repeats a row"
        if n_src >= 16:
            assert passes[0] != passes[1], n_src
        for k, r in enumerate(rounds):
            hidx, _ = conv_batch(n_src, nrows, SAMPLER_SEED, r, drop_last=True)
            assert hidx == idx[k].tolist(), (n_src, r)


@pytest.mark.parametrize("n_src,nrows", [(5, 8), (27, 8), (1000, 64), (4097, 3)])
def test_sampler_large_round_and_batch(n_src, nrows):
    """Rounds from 2^30 on (the batch position and the drop_last row position 2^30 nrows stay exact in 64 bits), both
    modes, and the same calls inside a launch batch: bitwise the stand-alone launches, equal to the host."""
    rowf = _row_floats(n_src, nrows)
    nb = (n_src + nrows - 1) // nrows
    rounds = [2 ** 30 + k for k in range(min(nb, 6) + 1)] + [0, 1, nb - 1, nb]
    idx, nv = _sample(n_src, nrows, rowf, SAMPLER_SEED, rounds)
    bidx, bnv = _sample(n_src, nrows, rowf, SAMPLER_SEED, rounds, batch=True)
    assert torch.equal(idx, bidx) and torch.equal(nv, bnv)
    for k, r in enumerate(rounds):
        hidx, hnv = conv_batch(n_src, nrows, SAMPLER_SEED, r)
        assert hnv == int(nv[k]) and hidx == idx[k].tolist(), (n_src, r)
    if n_src >= nrows:
        didx, _ = _sample(n_src, nrows, rowf, SAMPLER_SEED, rounds, drop_last=True)
        dbidx, _ = _sample(n_src, nrows, rowf, SAMPLER_SEED, rounds, drop_last=True, batch=True)
        assert torch.equal(didx, dbidx)
        for k, r in enumerate(rounds):
            assert conv_batch(n_src, nrows, SAMPLER_SEED, r, drop_last=True)[0] == didx[k].tolist(), (n_src, r)


# =====================================================================================================================
# c. cgl_adam_multi / cgl_adam_multi_dev
# =====================================================================================================================
def adam_ref(p, g, m, v, step, lr, b1, b2, eps):
    """One step in fp64, torch _single_tensor_adam's order, from the fp32 state and with the kernel's own fp32
    constants (cgl_conv.hip: adam_multi_impl), so that only the arithmetic roundings separate it from the kernel.
    Returns (p', m', v') and their elementwise bounds:

      m' = lerp(m, g, w1): d = fl(g - m) (u |g - m|), then m + w1 d (w1 < 0.5) or g - d (1 - w1) (w1 >= 0.5, where
        1 - w1 is exact): one product (u w |d|, w <= 0.5 either way) and the final rounding (u |m'|, and m' lies
        between m and g) -- fused or not: |dm| <= (0.5 + 0.5 + 1) u (|m| + |g|) = 2u (|m| + |g|).
      v' = fl(fl(v b2) + fl(fl(w2 g) g)), all terms >= 0: three roundings deep, |dv| <= 3u v' (1 + O(u)) <= 4u v'.
      p' = fl(p + fl(fl(-ss m') / den)), den = fl(fl(sqrtf(v') / bc) + eps): v' carries 3u -> sqrt 1.5u, + u each
        for sqrtf, the division by bc and the sum with eps (eps exact, both terms >= 0): 4.5u on den; the product
        ss m' and the division one u each: 6.5u <= 8u on upd = ss m' / den; m's own error enters as ss |dm| / den;
        the last addition u |p'|:  |dp| <= u |p'| + 8u |upd| + ss 2u (|m| + |g|) / den."""
    f32 = np.float32
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    w1, b2f, w2 = float(f32(1.0 - b1)), float(f32(b2)), float(f32(1.0 - b2))
    bc1, bc2 = 1.0 - math.pow(b1, step), 1.0 - math.pow(b2, step)
    ss, bc, epsf = float(f32(lr / bc1)), float(f32(math.pow(bc2, 0.5))), float(f32(eps))
    m1 = m + w1 * (g - m)
    v1 = v * b2f + w2 * g * g
    den = np.sqrt(v1) / bc + epsf
    upd = ss * m1 / den
    p1 = p - upd
    bm = 2 * U * (np.abs(m) + np.abs(g))
    bv = 4 * U * v1
    bp = U * np.abs(p1) + 8 * U * np.abs(upd) + ss * bm / den
    return (p1, m1, v1), (bp, bm, bv)


def _ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 / 0 counts as 0: an exact value with a zero bound passes)."""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


class _AdamState:
    """p, m, v (sentinel-terminated device buffers) and a gradient per tensor of ``sizes``."""

    def __init__(self, sizes, gen):
        self.sizes = sizes
        self.pads = {k: [padded(n) for n in sizes] for k in "pmv"}
        for (pv, _), n in zip(self.pads["p"], sizes):
            pv.copy_(torch.randn(n, generator=gen))
        for k in "mv":
            for t, _ in self.pads[k]:
                t.zero_()
        self.gen = gen

    def t(self, k):
        return [a for a, _ in self.pads[k]]

    def host(self, k):
        return [a.cpu().numpy().copy() for a, _ in self.pads[k]]

    def grads(self):
        """~N(0, 1e-2) gradients with every 7th element exactly 0"""
        out = []
        for n in self.sizes:
            g = torch.randn(n, generator=self.gen) * 0.1
            g[::7] = 0.0
            out.append(g)
        return out

    def sentinels(self):
        for k in "pmv":
            for (a, buf), n in zip(self.pads[k], self.sizes):
                sent_ok(buf, n, f"adam {k}")


ADAM_LISTS = {"mixed": [1, 255, 256, 257, 0, 70001, 0],                    # an empty tensor in the middle and last
              "nt32": [(37 * i) % 300 + 1 for i in range(32)],            # a full launch of small tensors
              "nt33": [(53 * i) % 200 + 1 for i in range(32)] + [513]}    # the wrapper's second launch


@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.999)], ids=["lerp_end", "lerp_self"])
@pytest.mark.parametrize("name", list(ADAM_LISTS))
def test_adam_multi_elementwise(name, betas):
    """Steps 1, 2, 3 and a jump to step 1000, each judged from the state the kernel itself left (so one step's
    roundings, not a trajectory's), element by element against adam_ref's bounds -- a tensor's largest element no
    longer hides the others.  beta1 = 0.5 takes at::lerp's `end - (end - self)(1 - w)` branch, 0.9 the other.
    Elements with g = 0 and, at the jump, v = 0 as well (denominator = eps exactly) are part of every tensor.

    Worst |err| / bound measured on the MI355X: m 0.44, v 0.48, p 0.998 -- the p bound's u |p'| term is the final
    rounding alone and is attained whenever p' lies just above a power of two (half an ulp there is u |p'|), so a
    ratio close to 1 is the bound being sharp, not the kernel being close to wrong."""
    O = ops()
    sizes = ADAM_LISTS[name]
    st = _AdamState(sizes, torch.Generator().manual_seed(len(sizes)))
    lr, eps = 2e-4, 1e-8
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 3, 1000):
        if step == 1000:
            for v in st.t("v"):
                v[::7] = 0.0
        gs = st.grads()
        before = {k: st.host(k) for k in "pmv"}
        O.adam_multi(st.t("p"), [g.to(DEV) for g in gs], st.t("m"), st.t("v"), step, lr=lr, betas=betas, eps=eps)
        torch.cuda.synchronize()
        st.sentinels()
        after = {k: st.host(k) for k in "pmv"}
        for i, n in enumerate(sizes):
            refs, bounds = adam_ref(before["p"][i], gs[i].numpy(), before["m"][i], before["v"][i], step, lr, *betas,
                                    eps)
            for q, k in enumerate("pmv"):
                worst[q] = max(worst[q], _ratio(after[k][i], refs[q], bounds[q]))
    print(f"adam_multi {name} betas={betas}: worst |err| / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("s", [0, 1, 9, 999, 99999])
def test_adam_multi_dev_is_the_host_step(s):
    """cgl_adam_multi_dev with *step_dev = s takes step s + 1: the same m, v AND p as cgl_adam_multi(step = s + 1),
    bit for bit -- the device computes the two bias corrections with the same double pow as the host.  (Measured on
    the MI355X: equal at all five steps; had p differed, the two fp32 corrections would have rounded apart.)"""
    O = ops()
    sizes = [1, 255, 257, 0, 4099]
    outs = []
    for dev in (False, True):
        st = _AdamState(sizes, torch.Generator().manual_seed(77))
        for k in "mv":                                  # non-zero moments, v >= 0
            for t in st.t(k):
                t.copy_(torch.randn(t.numel(), generator=st.gen).abs() * (0.1 if k == "m" else 1e-3))
        gs = [g.to(DEV) for g in st.grads()]
        sd = torch.tensor([s, 12345], dtype=torch.int32, device=DEV)
        O.adam_multi(st.t("p"), gs, st.t("m"), st.t("v"), s + 1, step_dev=sd if dev else None)
        torch.cuda.synchronize()
        st.sentinels()
        outs.append(st)
    for k in "mvp":
        for a, b in zip(outs[0].t(k), outs[1].t(k)):
            assert same_bits(a, b), f"{k} differs between step = {s + 1} and step_dev = {s}"


# =====================================================================================================================
# d. cgl_adv_loss
# =====================================================================================================================
LOSSES = {"ce": 0, "bce_prob": 1, "mse": 2, "bce": 3}


def adv_ref(x, kind, target, weight, M):
    """Per-row loss term l and gradient g = weight d(mean loss)/dx of the first M rows in fp64, with elementwise
    bounds (bl, bg) from the kernel's operations (cgl_conv.hip: cgl_adv_row1, cgl_adv_loss_at).  invM = fl(1 / M)
    and every product / quotient cost one u each; expf / logf 4u relative (2 ulp).

    mse: d = fl(z - y) (u), l = fl(d d): 3u l.  g = weight (2 d invM): d, invM, two products: 4u -> 5u |g|.
    bce_prob (pr = z in [0.01, 0.99]): l = -logf(pr) (y = 1): 4u |l|; l = -logf(fl(1 - pr)) (y = 0): the subtraction
        rounds relatively (u; exact above 0.5), which moves the logarithm by u ABSOLUTELY: 4u |l| + u.
        g = (weight invM)(pr - y) / fl(fl(1 - pr) pr): seven roundings -> 8u |g|.
    bce (pr = fl(1 / fl(1 + expf(-z)))): e = exp(-z) carries 4u, the sum u + 4u e / (1 + e), the division u:
        pr is off by dp = (2u + 4u (1 - p)) p absolutely.  y = 1: l = -logf(pr): 4u |l| + dp / p.  y = 0:
        l = -logf(fl(1 - pr)): 1 - pr inherits dp ABSOLUTELY (plus u relative below 0.5): 4u |l| + dp / (1 - p) + u --
        not a relative bound; dp / (1 - p) grows like 2u e^z, which is why the moderate inputs stop at |z| <= 8
        (1 - p >= 2^12 u there: the subtraction is still well conditioned; see test_adv_loss_saturated for the rest).
        g = gp (1 - pr) pr with gp as above: fl(1 - pr) pr / fl(fl(1 - pr) pr) = 1 within u, so (y = 0) g = weight
        invM pr within 7 roundings + pr's 6u: 13u |g|; (y = 1) pr - 1 = -(1 - pr) carries dp / (1 - p) + u
        relatively: (9u + dp / (1 - p)) |g|.
    ce (two logits, D = |z0 - z1|, mx the larger): fl(z_i - mx) is off by u D, e = expf(.) <= 1 by 4u + 0.37u, the sum
        s in [1, 2] by 2u more, lse = logf(s) by 6.4u + 4u log 2 <= 9.2u, o_i = fl(fl(z_i - mx) - lse) by
        Eo_i = u (D + 10 + |o_i|), and l = -o_target: bl = Eo_t.  g_i = expf(o_i) w - [i = t] w, w = fl(weight invM)
        (2u, a common factor): the exponential carries Eo_i + 4u, the product (or the fused multiply-add) u:
        bg_i = (weight / M) p_i (Eo_i + 5u) + 3u |g_i|."""
    z = x.astype(np.float64)[:M * (2 if kind == "ce" else 1)]
    w = float(np.float32(weight))
    y = float(target)
    if kind == "mse":
        d = z - y
        l, g = d * d, w * 2 * d / M
        return l, g, 4 * U * l, 5 * U * np.abs(g)
    if kind == "bce_prob":
        p = z
        l = -np.log(p) if target else -np.log1p(-p)
        g = w / M * (p - y) / ((1 - p) * p)
        return l, g, 4 * U * np.abs(l) + (0.0 if target else 1.01 * U), 8 * U * np.abs(g)
    if kind == "bce":
        e = np.exp(-z)
        p, q = 1 / (1 + e), e / (1 + e)            # q = 1 - p without cancellation
        dp = (2 * U + 4 * U * q) * p
        if target:
            l, bl = np.log1p(e), 4 * U * np.log1p(e) + dp / p
            g = -w / M * q
            bg = (9 * U + dp / q) * np.abs(g)
        else:
            l = np.log1p(np.exp(z))
            bl = 4 * U * l + 1.01 * (dp / q + U)
            g = w / M * p
            bg = 13 * U * np.abs(g)
        return l, g, bl, bg
    assert kind == "ce"
    z = z.reshape(-1, 2)
    mx = z.max(1, keepdims=True)
    lse = np.log(np.exp(z - mx).sum(1, keepdims=True))
    o = z - mx - lse
    pr = np.exp(o)
    D = np.abs(z[:, :1] - z[:, 1:])
    eo = U * (D + 10 + np.abs(o))
    l = -o[:, target]
    onehot = np.zeros_like(z)
    onehot[:, target] = 1.0
    g = w / M * (pr - onehot)
    bg = w / M * pr * (eo + 5 * U) + 3 * U * np.abs(g)
    return l, g.reshape(-1), eo[:, target], bg.reshape(-1)


def _adv_inputs(kind, M, gen):
    C = 2 if kind == "ce" else 1
    if kind == "bce_prob":
        return (0.01 + 0.98 * torch.rand(M * C, generator=gen)).clamp(0.01, 0.99)
    # |z| <= 8: above it the Sigmoid form's 1 - pr is a few ulps wide (adv_ref)
    return (4 * torch.randn(M * C, generator=gen)).clamp(-8.0, 8.0)


def _adv_call(x, M, kind, target, weight, nv=None, grad=True):
    """One cgl_adv_loss launch on M rows: (loss [1], gradient [M C] or None), sentinels checked."""
    O = ops()
    C = 2 if kind == "ce" else 1
    lo, lbuf = padded(1)
    gr, gbuf = padded(M * C) if grad else (None, None)
    O.adv_loss(x, M, C, kind, target, weight, loss_out=lo, grad=gr, nvalid=nv)
    torch.cuda.synchronize()
    sent_ok(lbuf, 1, "loss_out")
    if grad:
        sent_ok(gbuf, M * C, "gradient rows past M")
    return lo.cpu(), (gr.cpu() if grad else None)


def _loss_bound(l, bl):
    """The kernel sums the fp32 row terms in double and rounds the mean once: |dL| <= u |L| + mean |dl_r| (+ the
    double sum's own 2^-53 per addition, against the same magnitude)."""
    L = float(l.mean())
    return L, U * abs(L) + float(bl.mean()) + len(l) * 2.0 ** -53 * float(np.abs(l).mean())


ADV_M = [1, 2, 255, 256, 257, 1000]


@pytest.mark.parametrize("target", [0, 1])
@pytest.mark.parametrize("kind", list(LOSSES))
def test_adv_loss_moderate_inputs(kind, target):
    """Loss and gradient against fp64 with adv_ref's elementwise bounds, M around the 256-thread workgroup (one
    strided pass, two, four).

    Worst |err| / bound measured on the MI355X (loss, gradient): ce 0.19, 0.66; bce_prob 0.43, 0.38; mse 0.19, 0.57;
    bce 0.29, 0.69."""
    gen = torch.Generator().manual_seed(17 * LOSSES[kind] + target)
    worst_l = worst_g = 0.0
    for weight in (0.5, 1.0):
        for M in ADV_M:
            x = _adv_inputs(kind, M, gen)
            lo, gr = _adv_call(x.to(DEV), M, kind, target, weight)
            l, g, bl, bg = adv_ref(x.numpy(), kind, target, weight, M)
            L, bL = _loss_bound(l, bl)
            worst_l = max(worst_l, abs(float(lo[0]) - L) / bL)
            worst_g = max(worst_g, _ratio(gr.numpy(), g, bg))
            assert math.isfinite(float(lo[0])) and bool(torch.isfinite(gr).all())
    print(f"adv_loss {kind} target={target}: worst |err| / bound  loss {worst_l:.3f}  grad {worst_g:.3f}")
    assert worst_l <= 1.0 and worst_g <= 1.0, (worst_l, worst_g)


SAT_LOGITS = [17.5, -17.5, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0]
SAT_PROBS = [0.0, 1.0, 2.0 ** -149, 1.0 - 2.0 ** -24]
SAT_PAIRS = [(80.0, -80.0), (-80.0, 80.0), (3.0, 3.0)]


def _torch_row(kind, x, target):
    """torch's own fp32 CPU modules on one row: (loss term, gradient w.r.t. the row's inputs)."""
    import torch.nn as nn
    z = torch.tensor(x, dtype=torch.float32, requires_grad=True)
    if kind == "ce":
        l = nn.CrossEntropyLoss()(z.view(1, 2), torch.tensor([target]))
    else:
        pr = torch.sigmoid(z) if kind == "bce" else z
        l = nn.BCELoss()(pr.view(1), torch.full((1,), float(target)))
    l.backward()
    return float(l.detach()), z.grad.view(-1).numpy().astype(np.float64)


@pytest.mark.parametrize("kind", ["bce", "bce_prob", "ce"])
def test_adv_loss_saturated(kind):
    """Saturated inputs against torch's fp32 CPU modules (BCELoss on Sigmoid, BCELoss, CrossEntropyLoss: the
    semantics include/cglgan.h cites), one row per call (M = 1, weight 1: invM and the weight are exact, so the call
    shows the row's own term and gradient): the -100 logarithm clamp, the 1e-12 gradient clamp (torch: loss 100 and
    gradient 0 at a logit of +20 with target 0; loss 100 and gradient -999999995904 at probability 0 with target 1).
    Required: the term within 4u (1 + |l|) of torch's, the gradient within 4u |g| and exactly 0 where torch's is.
    -log(1 - pr) at pr < u is 0 here (1 - pr rounds to 1) where torch's log1p returns pr: an absolute u, inside the
    4u above.  Logits in (8, 17.5) with target 0 are left out on purpose: 1 - pr is a few ulps wide there and any
    fp32 evaluation of its logarithm is ill-conditioned (adv_ref gives the bound that applies below 8).

    Measured on the MI355X: every gradient equals torch's; every term too, except logit -17.5 with target 1
    (17.500002 against 17.5: 0.43 of the bound) and the two log1p cases above (0 against 2.5e-8 and 2.1e-9)."""
    rows = SAT_PAIRS if kind == "ce" else [(v,) for v in (SAT_LOGITS if kind == "bce" else SAT_PROBS)]
    worst_l = worst_g = 0.0
    for row in rows:
        for target in (0, 1):
            x = torch.tensor(row, dtype=torch.float32)
            lo, gr = _adv_call(x.to(DEV), 1, kind, target, 1.0)
            tl, tg = _torch_row(kind, list(row), target)
            got_l, got_g = float(lo[0]), gr.numpy().astype(np.float64)
            print(f"adv_loss saturated {kind} x={row} target={target}: loss {got_l!r} (torch {tl!r})  "
                  f"grad {got_g.tolist()} (torch {tg.tolist()})")
            assert abs(got_l - tl) <= 4 * U * (1 + abs(tl)), (row, target, got_l, tl)
            worst_l = max(worst_l, abs(got_l - tl) / (4 * U * (1 + abs(tl))))
            for a, b in zip(got_g, tg):
                if b == 0.0:
                    assert a == 0.0, (row, target, got_g, tg)
                else:
                    assert abs(a - b) <= 4 * U * abs(b), (row, target, got_g, tg)
                    worst_g = max(worst_g, abs(a - b) / (4 * U * abs(b)))
    print(f"adv_loss saturated {kind}: worst |err| / bound  loss {worst_l:.3f}  grad {worst_g:.3f}")


@pytest.mark.parametrize("M", [8, 257])
@pytest.mark.parametrize("kind", list(LOSSES))
def test_adv_loss_nvalid(kind, M):
    """*nvalid rows form the batch: the loss is the mean over the first min(max(nv, 1), M) rows, those rows'
    gradients are bitwise the gradients of a call with that M, the rows past them are exactly 0, and nothing is
    written after row M."""
    C = 2 if kind == "ce" else 1
    gen = torch.Generator().manual_seed(5 * LOSSES[kind] + M)
    x = _adv_inputs(kind, M, gen)
    xd = x.to(DEV)
    for target in (0, 1):
        full = _adv_call(xd, M, kind, target, 0.5)
        for nv in (None, 1, M - 1, M, M + 5, 0):
            m_eff = M if nv is None else min(max(nv, 1), M)
            nvd = None if nv is None else torch.tensor([nv, 99], dtype=torch.int32, device=DEV)
            lo, gr = _adv_call(xd, M, kind, target, 0.5, nv=nvd)
            short_l, short_g = _adv_call(xd, m_eff, kind, target, 0.5)
            assert same_bits(lo, short_l), (nv, float(lo[0]), float(short_l[0]))
            assert same_bits(gr[:m_eff * C], short_g), nv
            assert bool((bits(gr[m_eff * C:]) == 0).all()), f"nvalid {nv}: a padding row got a gradient"
            l, _, bl, _ = adv_ref(x.numpy(), kind, target, 0.5, m_eff)
            L, bL = _loss_bound(l, bl)
            assert abs(float(lo[0]) - L) <= bL, (nv, float(lo[0]), L)     # the mean over m_eff rows, not over M
            if m_eff == M:
                assert same_bits(lo, full[0]) and same_bits(gr, full[1])


def test_adv_loss_batched_heads():
    """Two cgl_adv_loss calls recorded in a launch batch (the D step's real and fake heads) run as two blocks of one
    launch and are bitwise the stand-alone calls; a third call in the same batch is refused."""
    O = ops()
    gen = torch.Generator().manual_seed(3)
    for kind in LOSSES:
        C = 2 if kind == "ce" else 1
        xs = [_adv_inputs(kind, M, gen).to(DEV) for M in (257, 8)]
        nvd = torch.tensor([200], dtype=torch.int32, device=DEV)
        alone = [_adv_call(xs[0], 257, kind, 1, 0.5, nv=nvd), _adv_call(xs[1], 8, kind, 0, 0.5)]
        lo = [padded(1) for _ in range(2)]
        gr = [padded(257 * C), padded(8 * C)]
        with O.launch_batch():
            O.adv_loss(xs[0], 257, C, kind, 1, 0.5, loss_out=lo[0][0], grad=gr[0][0], nvalid=nvd)
            O.adv_loss(xs[1], 8, C, kind, 0, 0.5, loss_out=lo[1][0], grad=gr[1][0])
        torch.cuda.synchronize()
        for k, n in enumerate((257 * C, 8 * C)):
            sent_ok(lo[k][1], 1)
            sent_ok(gr[k][1], n)
            assert same_bits(lo[k][0].cpu(), alone[k][0]) and same_bits(gr[k][0].cpu(), alone[k][1]), (kind, k)
    x = _adv_inputs("mse", 8, gen).to(DEV)
    out = torch.zeros(3, device=DEV)
    with pytest.raises(RuntimeError):
        with O.launch_batch():
            for k in range(3):
                O.adv_loss(x, 8, 1, "mse", 0, 1.0, loss_out=out[k:k + 1])
    torch.cuda.synchronize()
    assert float(out[2]) == 0.0 and float(out[0]) == float(out[1]) != 0.0     # the two recorded calls still ran


# =====================================================================================================================
# e. one scratch, launches of different sizes (the ticket returns to 0 after every launch)
# =====================================================================================================================
@pytest.mark.parametrize("ncalls", [1, 2])
@pytest.mark.parametrize("kind", ["mse", "bce"])
def test_dense1_head_scratch_reuse(kind, ncalls):
    """cgl_dense1_head_nhwc on ONE zeroed scratch with n = 8, 12, 4, 512, 8 (grids of 2, 3, 1, 128, 2 workgroups):
    after every launch the losses, Y, dY and dX are bitwise those of the separate launches (dense1_fwd_nhwc +
    adv_loss + dense1_bwd_data_nhwc) and the ticket word is 0 again.  With a ticket that only grew and was taken
    modulo the current grid, the second launch's FIRST workgroup (ticket 2 of a grid of 3) reduced the losses before
    the others had published theirs.  (That race rarely shows at these sizes -- the previous library passed the
    comparisons here -- so the ticket word is what pins the fix for the head; the finalize below showed wrong
    statistics at its second launch.)"""
    O = ops()
    c, hw = 128, 4
    scratch, sbuf = padded(512 + 16)
    scratch.zero_()
    gen = torch.Generator().manual_seed(7 + ncalls)
    w = (torch.randn(c * hw, generator=gen) * 0.05).to(DEV)
    b = torch.randn(1, generator=gen).to(DEV)
    for it, n in enumerate((8, 12, 4, 512, 8)):
        x = (torch.randn(n, hw, c, generator=gen) * (1 + it)).to(DEV)      # other values every launch: stale terms show
        n0 = n // 2 if ncalls == 2 else n
        spec = [(n0, 1, 0.5), (n - n0, 0, 0.5)][:ncalls]
        y, ybuf = padded(n)
        dy, dybuf = padded(n)
        dx, dxbuf = padded(n * c * hw)
        lo, lobuf = padded(2)
        calls = [(rows, t, wt, lo[k:k + 1], None) for k, (rows, t, wt) in enumerate(spec)]
        O.dense1_head_nhwc(x, w, b, y, dy, dx, n, c, hw, kind, calls, scratch)
        y2, dy2, dx2, lo2 = (torch.empty(n, device=DEV), torch.empty(n, device=DEV),
                             torch.empty(n * c * hw, device=DEV), torch.empty(2, device=DEV))
        O.dense1_fwd_nhwc(x, w, b, y2, n, c, hw)
        r0 = 0
        for k, (rows, t, wt) in enumerate(spec):
            O.adv_loss(y2[r0:r0 + rows], rows, 1, kind, t, wt, loss_out=lo2[k:k + 1], grad=dy2[r0:r0 + rows])
            r0 += rows
        O.dense1_bwd_data_nhwc(dy2, w, dx2, n, c, hw)
        torch.cuda.synchronize()
        for buf, m, what in ((ybuf, n, "Y"), (dybuf, n, "dY"), (dxbuf, n * c * hw, "dX"), (sbuf, 528, "scratch")):
            sent_ok(buf, m, what)
        assert bool((bits(lo[ncalls:]) == PAT32).all())
        assert same_bits(y, y2) and same_bits(dy, dy2) and same_bits(dx, dx2), f"launch {it} (n = {n})"
        assert same_bits(lo[:ncalls], lo2[:ncalls]), (f"launch {it} (n = {n}): losses", lo[:ncalls].tolist(),
                                                      lo2[:ncalls].tolist())
        assert int(bits(scratch)[0]) == 0, f"launch {it} (n = {n}): the ticket is not back at 0"


def _chunk_partials(x, rows, c, R=32):
    """{sum, M2 about the chunk mean} of every R-row chunk of x [rows][c], in fp64 on the device: the partials a
    conv3x3_fwd(stats=...) epilogue hands to bn2d_fwd_stats."""
    xc = x.double().view(rows // R, R, c)
    s = xc.sum(1)
    m2 = ((xc - (s / R).unsqueeze(1)) ** 2).sum(1)
    return torch.stack([s, m2], dim=-1).contiguous()


def test_bn2d_fwd_stats_scratch_reuse():
    """bn2d_fwd_stats' sliced finalize on ONE zeroed scratch with hw = 1024, C = 64, R = 32 and n = 64, 40, 64: 2048,
    1280, 2048 chunks per call (> 1024: sliced), S = 4, 3, 4 slices per channel.  Every result equals the two-pass
    bn2d_fwd within the tolerance of test_gpu_conv_stats_canary.py and is bitwise the same call on a freshly zeroed
    scratch; the tickets are 0 after every launch."""
    O = ops()
    c, hw = 64, 1024
    nbytes = int(O.bn2d_stats_scratch(c, 1, DEV).numel())
    scratch, sbuf = padded(nbytes // 4)
    scratch.zero_()
    gen = torch.Generator().manual_seed(21)
    gam = (1 + 0.1 * torch.randn(c, generator=gen)).to(DEV)
    bet = (0.1 * torch.randn(c, generator=gen)).to(DEV)
    for it, n in enumerate((64, 40, 64)):
        rows = n * hw
        assert rows // 32 > 1024
        # another mean and spread per launch: statistics merged from the previous launch's slices would be far off
        x = (torch.randn(rows, c, generator=gen) * (1 + it) + 0.5 * it).to(DEV)
        part = _chunk_partials(x, rows, c)
        outs = []
        for scr in (scratch.view(torch.uint8), O.bn2d_stats_scratch(c, 1, DEV)):
            y, ybuf = padded(rows * c)
            rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
            sm, smbuf = padded(c)
            si, sibuf = padded(c)
            O.bn2d_fwd_stats(part, x, n, hw, c, gam, bet, y, groups=1, running_mean=rm, running_var=rv, save_mean=sm,
                             save_invstd=si, scratch=scr)
            torch.cuda.synchronize()
            sent_ok(ybuf, rows * c, "bn output")
            sent_ok(smbuf, c, "save_mean")
            sent_ok(sibuf, c, "save_invstd")
            outs.append((y, sm, si, rm, rv, scr.view(torch.int32)[:c].clone()))
        sent_ok(sbuf, nbytes // 4, "ticket scratch")
        ref = torch.empty(rows * c, device=DEV)
        rm2, rv2 = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        sm2, si2 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        O.bn2d_fwd(x, n, hw, c, gam, bet, ref, groups=1, running_mean=rm2, running_var=rv2, train=True, save_mean=sm2,
                   save_invstd=si2)
        torch.cuda.synchronize()
        y, sm, si, rm, rv, _ = outs[0]
        assert float((y - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), f"launch {it} (n = {n}) vs two-pass"
        assert torch.allclose(sm, sm2, rtol=1e-5, atol=1e-6) and torch.allclose(si, si2, rtol=1e-5, atol=1e-6), it
        assert torch.allclose(rm, rm2, rtol=1e-5, atol=1e-6) and torch.allclose(rv, rv2, rtol=1e-5, atol=1e-6), it
        for a, b in zip(outs[0], outs[1]):
            assert same_bits(a, b), f"launch {it} (n = {n}): reused scratch differs from a freshly zeroed one"
        assert bool((outs[0][5] == 0).all()), f"launch {it} (n = {n}): tickets not back at 0"


# =====================================================================================================================
# f. layout and reduction utilities
# =====================================================================================================================
def test_gather_rows_bitwise():
    """2049 rows of 1024 floats are 2049 * 4 blocks' worth of elements, one block more than the 8192-block grid: the
    grid-stride loop wraps once.  Index list reversed and with repeats; then the row0 form with a row width that is
    no multiple of 4; then nrows = 0."""
    O = ops()
    gen = torch.Generator().manual_seed(9)
    src = torch.randn(300, 1024, generator=gen).to(DEV)
    idx = (torch.arange(2048, -1, -1) * 7 % 300).to(torch.int32)
    assert len(set(idx.tolist())) < 2049
    dst, dbuf = padded(2049 * 1024)
    O.gather_rows(src, idx.to(DEV), 0, 2049, 1024, dst)
    torch.cuda.synchronize()
    sent_ok(dbuf, 2049 * 1024, "gathered rows")
    assert same_bits(dst.view(2049, 1024), src[idx.long().to(DEV)])
    src3 = torch.randn(20, 3, generator=gen).to(DEV)
    d3, d3buf = padded(7 * 3)
    O.gather_rows(src3, None, 5, 7, 3, d3)
    torch.cuda.synchronize()
    sent_ok(d3buf, 21, "row0 gather")
    assert same_bits(d3.view(7, 3), src3[5:12])
    d0, d0buf = padded(8)
    O.gather_rows(src3, None, 0, 0, 3, d0)
    torch.cuda.synchronize()
    assert bool((bits(d0buf) == PAT32).all()), "nrows = 0 wrote to dst"


@pytest.mark.parametrize("n,c,hw", [(1, 1, 1), (2, 3, 5), (3, 33, 31), (2, 32, 33), (1, 65, 1024), (2, 128, 4)])
def test_layout_transposes_bitwise(n, c, hw):
    """nchw_to_nhwc is permute(0, 2, 1) of [n, c, hw] bit for bit, nhwc_to_nchw its inverse: ragged 32 x 32 tiles in
    either dimension, one element, and a tile row that ends exactly at 32."""
    O = ops()
    x = torch.randn(n, c, hw, generator=torch.Generator().manual_seed(n * c + hw)).to(DEV)
    y, ybuf = padded(n * c * hw)
    O.nchw_to_nhwc(x, y, n, c, hw)
    back, bbuf = padded(n * c * hw)
    O.nhwc_to_nchw(y, back, n, c, hw)
    torch.cuda.synchronize()
    sent_ok(ybuf, n * c * hw, "nhwc")
    sent_ok(bbuf, n * c * hw, "nchw")
    assert same_bits(y.view(n, hw, c), x.permute(0, 2, 1))
    assert same_bits(back.view(n, c, hw), x)


@pytest.mark.parametrize("c", [1, 3, 64, 128])
def test_colsum_finalize(c):
    """out[c] = fp32(sum over the chunks of part[q][c][0]), the chunks summed in double in a fixed order: within one
    fp32 ulp of the exact sum plus nch 2^-53 sum |part| for the order of the double additions.  Slot [q][c][1] is NaN:
    it must not be read.  nch around the 256 threads of the channel's workgroup and past four strides.
    Worst |err| / bound measured on the MI355X: 0.50 (half an ulp: the final rounding)."""
    O = ops()
    gen = torch.Generator().manual_seed(c)
    worst = 0.0
    for nch in (1, 2, 255, 256, 257, 1025):
        part = torch.full((nch, c, 2), float("nan"), dtype=torch.float64)
        part[:, :, 0] = torch.randn(nch, c, generator=gen, dtype=torch.float64) * 100
        out, obuf = padded(c)
        O.colsum_finalize(part.to(DEV), nch, c, out)
        torch.cuda.synchronize()
        sent_ok(obuf, c, "column sums")
        v = part[:, :, 0].numpy()
        exact = v.astype(np.longdouble).sum(0).astype(np.float64)
        tol = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64) + nch * 2.0 ** -53 * np.abs(v).sum(0)
        got = out.cpu().numpy()
        assert np.isfinite(got).all()
        worst = max(worst, _ratio(got, exact, tol))
    print(f"colsum_finalize C={c}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0
