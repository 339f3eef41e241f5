"""gnx_batchnorm_bwd_x (``ops.batchnorm_bwd(..., beta=beta)``): the BatchNorm(+ReLU) backward that recomputes the ReLU
mask as x * a + b' > 0 instead of reading y.  It must give the bits of gnx_batchnorm_bwd with the forward's y: same
mask on every element (signed zeros, tiny positives, non-finite input), same partial sums, same dx / dgamma / dbeta."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))  # (NaN-safe: the two paths run the same operations on the same inputs)


def _forward(x, gamma, beta, relu):
    from gnnepcsaft_amd import ops
    return ops.batchnorm_fwd(x, gamma, beta, None, None, 0.1, EPS, True, relu)


def _both_backwards(dy, x, y, gamma, beta, mean, rstd, relu, seed=0):
    """(dx, dgamma, dbeta) of the y-reading entry and of the x-only entry, each accumulated into non-zero buffers"""
    from gnnepcsaft_amd import ops
    H = x.size(1)
    acc = torch.randn(2, H, generator=torch.Generator().manual_seed(seed)).to(x.device)
    old = ops.batchnorm_bwd(dy, x, y, gamma, mean, rstd, relu, dgamma=acc[0].clone(), dbeta=acc[1].clone())
    new = ops.batchnorm_bwd(dy, x, None, gamma, mean, rstd, relu, dgamma=acc[0].clone(), dbeta=acc[1].clone(), beta=beta)
    return old, new


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("H", [4, 60, 128, 130])
@pytest.mark.parametrize("M", [2, 7, 255, 256, 257, 1031, 8192 + 5])
def test_bwd_x_is_bitwise_the_y_reading_backward(gpu_device, M, H, relu):
    g = torch.Generator().manual_seed(M * 131 + H)
    x = (torch.randn(M, H, generator=g) * 3 + 5).to(gpu_device)
    gamma = torch.empty(H).uniform_(-1.5, 1.5, generator=g)
    gamma[::3] = -gamma[::3].abs()
    gamma[1] = 0.0
    beta = torch.empty(H).uniform_(-1, 1, generator=g)
    dy = torch.randn(M, H, generator=g).to(gpu_device)
    gamma, beta = gamma.to(gpu_device), beta.to(gpu_device)
    y, mean, rstd = _forward(x, gamma, beta, relu)
    old, new = _both_backwards(dy, x, y, gamma, beta, mean, rstd, relu, seed=M + H)
    for o, n, name in zip(old, new, ("dx", "dgamma", "dbeta")):
        assert _same_bits(o, n), name


@pytest.mark.parametrize("H", [128, 130])  # float4 and scalar kernels
def test_mask_edge_cases(gpu_device, H):
    """Columns whose forward value x * a + b' is exactly +0 / -0 (mask off), the smallest positive normal and a positive
    denormal (mask on), built by choosing gamma / beta from the forward's own mean and rstd in fp32 on the host; and
    columns holding a NaN, +inf, -inf.  The x-derived mask (evaluated on the host exactly as the kernel spells it)
    equals y > 0 on EVERY element, the per-column count of kept gradients equals that of y > 0, and the gradients are
    the y-reading backward's bits."""
    from gnnepcsaft_amd import ops
    M = 1031
    g = torch.Generator().manual_seed(77 + H)
    x = torch.randn(M, H, generator=g) * 3 + 5
    x[5, 20], x[6, 21], x[7, 22] = float("nan"), float("inf"), float("-inf")
    x[3, 0] = -x[3, 0].abs()
    xh = x.numpy()
    xd = x.to(gpu_device)
    _, mean, rstd = _forward(xd, None, None, True)  # the statistics do not depend on gamma / beta
    mean_h, rstd_h = mean.cpu().numpy(), rstd.cpu().numpy()
    gamma = torch.empty(H).uniform_(0.5, 1.5, generator=g).numpy().astype(np.float32)
    beta = torch.empty(H).uniform_(-1, 1, generator=g).numpy().astype(np.float32)
    f32 = np.float32
    tiny, denorm = f32(2.0 ** -126), f32(2.0 ** -140)
    # columns 0 / 1: gamma = 0 -> a = 0, x * a = +-0 by the sign of x, b' = beta - (+0): every entry is +0 or -0 ...
    gamma[0], beta[0] = 0.0, -0.0   # ... -0 where x < 0 (-0 + -0), +0 elsewhere
    gamma[1], beta[1] = 0.0, 0.0    # ... +0 everywhere
    # columns 2 / 3 / 4: one entry hits exactly +0 / 2^-126 / 2^-140 with a != 0: the target t needs
    # fl(fl(x * a) + fl(beta - fl(mean * a))) = t.  Columns 3 / 4 use a ~ 2^-120, where x * a, mean * a and beta sit on
    # a grid of 2^-142 or finer and the sums are exact.  The first row for which some beta does it is taken.
    targets = {2: f32(0.0), 3: tiny, 4: denorm}
    gamma[3] = gamma[4] = f32(2.0 ** -120)
    hit = {}
    with np.errstate(all="ignore"):
        for c, t in targets.items():
            a = f32(rstd_h[c] * gamma[c])
            m = f32(mean_h[c] * a)
            for row in range(M):
                p = f32(xh[row, c] * a)
                want_b = f32(t - p)
                b0 = f32(want_b + m)
                up = down = b0
                for _ in range(8):  # beta and a few of its neighbours
                    for cnd in (up, down):
                        if c not in hit and f32(cnd - m) == want_b and f32(p + f32(cnd - m)) == t:
                            hit[c], beta[c] = row, cnd
                    up, down = np.nextafter(up, f32(np.inf)), np.nextafter(down, f32(-np.inf))
                if c in hit:
                    break
            assert c in hit, f"column {c}: no (row, beta) gives x * a + b' = {t}"
    gd, bd = torch.from_numpy(gamma).to(gpu_device), torch.from_numpy(beta).to(gpu_device)
    y, mean2, rstd2 = _forward(xd, gd, bd, True)
    assert _same_bits(mean, mean2) and _same_bits(rstd, rstd2)
    yh = y.cpu().numpy()
    # the test built what it claims
    assert np.all(yh[:, 0] == 0) and np.all(yh[:, 1] == 0)
    assert yh[hit[2], 2] == 0 and yh[hit[3], 3] == tiny and yh[hit[4], 4] == denorm
    assert np.all(yh[:, 20] == 0)  # NaN statistics: max(NaN, 0) = 0 in the whole column
    assert np.all(yh[:, 21] == 0)  # mean = +inf, var = max(NaN, 0) = 0: b' = -inf
    assert yh[7, 22] == 0 and np.all(np.delete(yh[:, 22], 7) == np.inf)  # mean = -inf: b' = +inf, and -inf + inf = NaN
    # the kernel's predicate, spelled on the host as in the kernel (fp32 multiply, then add)
    with np.errstate(all="ignore"):
        a = (rstd_h * gamma).astype(np.float32)
        b = (beta - (mean_h * a).astype(np.float32)).astype(np.float32)
        o = ((xh * a[None, :]).astype(np.float32) + b[None, :]).astype(np.float32)
        assert np.signbit(o[3, 0]) and o[3, 0] == 0 and not np.signbit(o[0, 1])
        assert o[hit[2], 2] == 0 and not np.signbit(o[hit[2], 2]) and o[hit[3], 3] == tiny and o[hit[4], 4] == denorm
        assert np.array_equal(o > 0, yh > 0)
    dy = torch.ones(M, H, device=gpu_device)
    old, new = _both_backwards(dy, xd, y, gd, bd, mean, rstd, True, seed=H)
    for o_, n_, name in zip(old, new, ("dx", "dgamma", "dbeta")):
        assert _same_bits(o_, n_), name
    # dy = 1: dbeta (into a zero buffer) counts the kept gradients of each column exactly
    _, _, kept = ops.batchnorm_bwd(dy, xd, None, gd, mean, rstd, True, beta=bd)
    assert torch.equal(kept, (y > 0).sum(0).float())
    dyr = torch.randn(M, H, generator=g).to(gpu_device)
    old, new = _both_backwards(dyr, xd, y, gd, bd, mean, rstd, True, seed=H + 1)
    for o_, n_, name in zip(old, new, ("dx", "dgamma", "dbeta")):
        assert _same_bits(o_, n_), name


def test_no_affine_parameters(gpu_device):
    """gamma = beta = NULL (1 and 0) through the keyword ``beta=None``"""
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(257, 60, generator=g) * 3 + 5).to(gpu_device)
    dy = torch.randn(257, 60, generator=g).to(gpu_device)
    y, mean, rstd = _forward(x, None, None, True)
    old, new = _both_backwards(dy, x, y, None, None, mean, rstd, True)
    for o, n in zip(old, new):
        assert _same_bits(o, n)


def test_autograd_does_not_keep_y_and_gives_the_same_bits(gpu_device):
    from gnnepcsaft_amd import nn as gnn, ops
    M, H = 1031, 60
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M, H, generator=g) * 3 + 5).to(gpu_device).requires_grad_(True)
    bn = gnn.BatchNorm1d(H)
    with torch.no_grad():
        bn.weight.uniform_(-1.5, 1.5, generator=g)
        bn.bias.uniform_(-1, 1, generator=g)
    bn.to(gpu_device)
    y = bn(x, relu=True)
    saved = y.grad_fn.saved_tensors
    assert all(s is None or s.data_ptr() != y.data_ptr() for s in saved)
    assert all(s is None or s.numel() <= H or s.data_ptr() == x.data_ptr() for s in saved)  # x and [H] vectors only
    dy = torch.randn(M, H, generator=g).to(gpu_device)
    dx, dgamma, dbeta = torch.autograd.grad(y, [x, bn.weight, bn.bias], dy)
    # the y-reading backward on the same forward
    y2, mean, rstd = _forward(x.detach(), bn.weight.detach(), bn.bias.detach(), True)
    assert _same_bits(y2, y)
    rx, rg, rb = ops.batchnorm_bwd(dy, x.detach(), y2, bn.weight.detach(), mean, rstd, True)
    assert _same_bits(dx, rx) and _same_bits(dgamma, rg) and _same_bits(dbeta, rb)
