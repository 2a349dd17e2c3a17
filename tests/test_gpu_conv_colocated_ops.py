"""The co-located conv round's grouped ops against the single-worker ops they group, bitwise: the exchange launch
(cgl_conv_alpha_combine) against W cgl_weights_scale calls and the rank-order sum of ConvLocalComm, the grouped
sampler against W cgl_sample_rows_dev calls, the per-mask-seed Dropout2d masks against W cgl_dropout2d_masks_dev
calls, cgl_bcast_rows against copies -- each also recorded into a launch batch (one launch)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHTINGS = ["capgan", "mean", "mix_single", "mix_double", "cglgan"]
# the exchange kernel's grid is capped at 1024 workgroups of 256 lanes x 4 floats: past 1 Mi floats the grid-stride
# loop takes a second trip (the last size; its tail of 1024 floats leaves most of the grid idle in that trip)
WRAP = 1024 * 256 * 4
NXS = [4, 1020, 2048, 9216, WRAP + 1024]


@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("W", [2, 3, 16])
def test_alpha_combine(W, nx):
    from cglgan import conv_ops as O
    g = torch.Generator().manual_seed(100 * W + nx % 97)
    d = torch.randn(W, nx, generator=g).cuda()
    lbuf = torch.rand(W, 8, generator=g).cuda() * 2      # the G loss of worker q at [q][2], as the step lays them out
    beta = [(q + 1.0) / (W * (W + 1) / 2) for q in range(W)]           # unequal, sums to 1
    for weighting in WEIGHTINGS:
        for lam in (0.0, 0.37):
            lam_dev = torch.tensor([lam, 9.0], dtype=torch.float32).cuda()
            losses = lbuf[:, 2].contiguous()
            ref_alpha = torch.zeros(W, device="cuda")
            parts = []
            for q in range(W):
                x = d[q].clone()
                O.weights_scale(weighting, lam, beta, losses, q, x, alpha_out=ref_alpha)
                parts.append(x)
            tot = parts[0].clone()
            for x in parts[1:]:
                tot += x
            out = torch.full((nx,), 7.0, device="cuda")
            alpha, lall = torch.zeros(W, device="cuda"), torch.zeros(W, device="cuda")
            O.alpha_combine(weighting, beta, lbuf.view(-1)[2:], 8, lam_dev, d, out, alpha, lall)
            tag = (weighting, lam)
            assert torch.equal(alpha, ref_alpha), tag
            assert torch.equal(lall, losses), tag
            assert torch.equal(out, tot), tag
            assert abs(float(alpha.sum()) - 1.0) < 1e-5, tag
    # in place over worker 0's buffer (dimg may be d[0])
    d2 = d.clone()
    O.alpha_combine(weighting, beta, lbuf.view(-1)[2:], 8, lam_dev, d2, d2[0], alpha, lall)
    assert torch.equal(d2[0], tot) and torch.equal(d2[1:], d[1:])


SHARDS = [20, 12, 9]     # B = 8: every shard crosses a pass boundary in rounds 0 .. 5 and has a short batch


def _shards(seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, 1024, generator=g).cuda() for n in SHARDS]


@pytest.mark.parametrize("batched", [False, True])
def test_sample_rows_multi(batched):
    from cglgan import conv_ops as O
    B, W = 8, len(SHARDS)
    shards = _shards()
    rdev = torch.zeros(1, dtype=torch.int32, device="cuda")
    dst = [torch.zeros(2 * B, 1024, device="cuda") for _ in range(W)]        # rows past B must stay untouched
    nv = torch.zeros(W, dtype=torch.int32, device="cuda")
    multi = O.SampleRowsMulti([(shards[q], 11 + q, dst[q], nv[q:q + 1]) for q in range(W)], B, rdev)
    seen = [set() for _ in range(W)]
    for rnd in range(6):
        rdev.fill_(rnd)
        for t in dst:
            t.fill_(-1.0)
        with O.launch_batch(batched):
            multi()
        for q in range(W):
            ref, rnv = torch.full((B, 1024), -1.0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            O.sample_rows_dev(shards[q], B, 11 + q, rdev, ref, nv_out=rnv)
            assert torch.equal(dst[q][:B], ref), (rnd, q)
            assert bool((dst[q][B:] == -1.0).all()), (rnd, q)
            assert int(nv[q]) == int(rnv), (rnd, q)
            seen[q].add(int(rnv))
    for q, n in enumerate(SHARDS):
        assert n % B in seen[q] and B in seen[q], (q, seen[q])      # a short batch and a whole one were drawn


def test_sample_rows_multi_drop_last():
    """nv_out null on one job: that job cuts its passes drop_last, as the single call does."""
    from cglgan import conv_ops as O
    B = 8
    shards = _shards(5)
    rdev = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    dst = [torch.zeros(B, 1024, device="cuda") for _ in range(2)]
    nv = torch.zeros(1, dtype=torch.int32, device="cuda")
    O.SampleRowsMulti([(shards[0], 5, dst[0], None), (shards[1], 6, dst[1], nv)], B, rdev)()
    for q, nvq in ((0, None), (1, torch.zeros(1, dtype=torch.int32, device="cuda"))):
        ref = torch.zeros(B, 1024, device="cuda")
        O.sample_rows_dev(shards[q], B, 5 + q, rdev, ref, nv_out=nvq)
        assert torch.equal(dst[q], ref)


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("rnd", [0, 5])
def test_dropout_masks_multi(rnd, batched):
    from cglgan import conv_ops as O
    from cglgan.conv_step import D_CONVS, DROP_P
    B, W, seed = 8, 3, 7
    cs = [co for _, _, _, co, _ in D_CONVS]
    ns = [2 * B] * 4 + [B] * 4                      # the D step's masks (2B images), the G-loss pass's (B)
    ctrs = [call * 4 + k for call in (0, 1) for k in range(4)]
    rdev = torch.full((1,), rnd, dtype=torch.int32, device="cuda")
    masks = [[torch.full((n, c), -1.0, device="cuda") for n, c in zip(ns, cs + cs)] for _ in range(W)]
    multi = O.DropoutMasksMulti([(masks[q][j], ns[j], (cs + cs)[j], seed * 7919 + q, ctrs[j])
                                 for q in range(W) for j in range(8)], DROP_P, rdev, 8)
    with O.launch_batch(batched):
        multi()
    for q in range(W):
        ref = [torch.zeros(n, c, device="cuda") for n, c in zip(ns, cs + cs)]
        O.dropout2d_masks_dev(ref, ns, cs + cs, DROP_P, seed * 7919 + q, ctrs, rdev, 8)
        for j in range(8):
            assert torch.equal(masks[q][j], ref[j]), (q, j)
    assert not torch.equal(masks[0][0], masks[1][0])      # the workers' streams differ
    kept = torch.cat([m.view(-1) for m in masks[0]])
    assert set(kept.unique().tolist()) <= {0.0, float(torch.tensor(1.0 / (1.0 - DROP_P), dtype=torch.float32))}


def test_bcast_rows():
    from cglgan import conv_ops as O
    B, W = 3, 4          # 3 images: not a multiple of the workgroup
    src = torch.randn(B, 1024, device="cuda")
    dst = torch.full((W, 2 * B, 1024), -1.0, device="cuda")
    O.bcast_rows(src, dst[0][B:], 2 * B * 1024, W)
    assert torch.equal(dst[:, B:], src.expand(W, B, 1024))
    assert bool((dst[:, :B] == -1.0).all())
