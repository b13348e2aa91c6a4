"""Shared by tests/test_backbone_train.py (CPU) and tests/test_backbone_train_kernels.py (GPU): the dense restatement of
tests/backbone_helpers.py with batch-statistics BatchNorm1d - the sparse backbone in train() mode, without spconv and without a GPU.

BatchNorm1d over the feature rows of a sparse tensor = per channel over the ACTIVE sites of the dense form: mean and biased variance of
those sites normalise, the unbiased variance goes into the running statistics.  Per layer the rule is torch's: batch statistics where
`bn.training` is true, the running statistics where it is false."""
import numpy as np
import torch

from tests import backbone_helpers as BH
from tests.backbone_helpers import SUBM


def dense_bn_train(y, mask, gamma, beta, eps):
    """Batch-statistics BatchNorm over the active sites of (y, mask).  Returns (normalised * mask, (mean (C,), M2 (C,), n)): M2 is the sum
    of squared deviations from the mean over the n active sites, all in y's dtype."""
    n = float(mask.sum())
    axes = (0, 2, 3, 4)
    mean = (y * mask).sum(axes) / n
    dev = (y - mean.view(1, -1, 1, 1, 1)) * mask
    m2 = (dev * dev).sum(axes)
    g, b = gamma.to(y.dtype).view(1, -1, 1, 1, 1), beta.to(y.dtype).view(1, -1, 1, 1, 1)
    out = (dev / torch.sqrt(m2 / n + eps).view(1, -1, 1, 1, 1) * g + b) * mask
    return out, (mean, m2, n)


class _Restatement:
    """Walks the (conv, BatchNorm1d) pairs in the order of SpMiddleResNetFHD._pairs() and keeps each layer's statistics."""

    def __init__(self):
        self.stats = []  # per pair: (mean, M2, n) of a layer on batch statistics, None of one on running statistics

    def bn(self, y, mask, bn):
        if bn.training:
            out, st = dense_bn_train(y, mask, bn.weight.detach(), bn.bias.detach(), bn.eps)
            self.stats.append(st)
            return out
        self.stats.append(None)
        return BH.dense_bn(y, mask, BH._bn_tensors(bn), bn.eps)

    def block(self, x, mask, blk):
        h, _ = BH.dense_conv(x, mask, blk.conv1.weight.detach(), blk.conv1.bias.detach(), SUBM, True)
        h = torch.relu(self.bn(h, mask, blk.bn1))
        o, _ = BH.dense_conv(h, mask, blk.conv2.weight.detach(), blk.conv2.bias.detach(), SUBM, True)
        return torch.relu(self.bn(o, mask, blk.bn2) + x) * mask


def reference_forward_train(module, features, coords, B, input_shape, dtype):
    """SpMiddleResNetFHD.forward restated densely on the CPU in `dtype`, with batch statistics for every layer whose `bn.training` is
    true (the module's own tensors are read, none is written).  Returns (ret, levels, stats): ret and levels as
    backbone_helpers.reference_forward, stats = one entry per (conv, norm) pair in forward order, see _Restatement."""
    grid = tuple(int(v) for v in (np.array(input_shape[::-1]) + [1, 0, 0]))
    x, mask = BH.to_dense(torch.as_tensor(features).to(dtype), coords, B, grid)
    levels, r = {}, _Restatement()
    with torch.no_grad():
        c0, n0 = module.conv_input[0], module.conv_input[1]
        x, _ = BH.dense_conv(x, mask, c0.weight.detach(), None, SUBM, True)
        x = torch.relu(r.bn(x, mask, n0))
        for blk in module.conv1:
            x = r.block(x, mask, blk)
        levels["conv1"] = (x, mask)
        for name in ("conv2", "conv3", "conv4", "extra_conv"):
            seq = getattr(module, name)
            conv, bn = seq[0], seq[1]
            x, mask = BH.dense_conv(x, mask, conv.weight.detach(), None, (conv.kernel_size, conv.stride, conv.padding), False)
            x = torch.relu(r.bn(x, mask, bn))
            for blk in list(seq)[3:]:
                x = r.block(x, mask, blk)
            levels["ret" if name == "extra_conv" else name] = (x, mask)
    Bn, C, D, H, W = x.shape
    return x.reshape(Bn, C * D, H, W), levels, r.stats


def expected_running(module, stats):
    """Float64 running statistics after one forward, from the module's tensors BEFORE it and the reference's per-layer statistics:
    per pair (running_mean, running_var) as nn.BatchNorm1d updates them - (1 - m) r + m new with the unbiased variance - or None."""
    out = []
    for (_, bn), st in zip(module._pairs(), stats):
        if st is None:
            out.append(None)
            continue
        mean, m2, n = st
        m = float(bn.momentum)
        out.append(((1 - m) * bn.running_mean.detach().double().cpu() + m * mean.double(),
                    (1 - m) * bn.running_var.detach().double().cpu() + m * m2.double() / (n - 1)))
    return out


def randomize_train(module, gen):
    """backbone_helpers.randomize, then running means moved away from zero (0.05 .. 0.15 in magnitude, random sign): the update
    (1 - m) r + m mean is compared at a RELATIVE bar, which means nothing for a channel whose running mean happens to sit at zero."""
    BH.randomize(module, gen)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                n = m.num_features
                sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
                m.running_mean.copy_(sign * (0.05 + 0.1 * torch.rand(n, generator=gen)))
