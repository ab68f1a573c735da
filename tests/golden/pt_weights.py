"""Deterministic PointTransformer parameters and buffers, keyed by state_dict
name and by module kind (shared by the golden generator and the tests: the
model has about 5 M parameters at fixed widths, so no weights are stored).

The names alone do not tell a BatchNorm from a Linear here (``linear_w.0`` is
a BatchNorm, ``linear_w.2`` a Linear), so the kind comes from the module:
BatchNorm weight 1 + 0.1 N, bias 0.1 N, running mean 0.1 N, running variance
U[1, 1.5); Linear weight N / sqrt(fan-in), bias 0.05 N; each from
default_rng(crc32(name))."""
import zlib

import numpy as np
import torch


def fill(name, shape, is_bn):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.endswith("num_batches_tracked"):
        return np.zeros(shape, np.int64)
    if name.endswith("running_var"):
        return (1.0 + 0.5 * rng.random(shape)).astype(np.float32)
    if name.endswith("running_mean"):
        return (0.1 * rng.standard_normal(shape)).astype(np.float32)
    if is_bn:
        base = 1.0 if name.endswith("weight") else 0.0
        return (base + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    if name.endswith("bias"):
        return (0.05 * rng.standard_normal(shape)).astype(np.float32)
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    return (rng.standard_normal(shape) / np.sqrt(max(fan_in, 1))).astype(np.float32)


def state_dict_for(model):
    """Values for every entry of model.state_dict(), in its order."""
    bn = {name for name, mod in model.named_modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)}
    out = {}
    for k, v in model.state_dict().items():
        out[k] = torch.from_numpy(fill(k, tuple(v.shape), k.rsplit(".", 1)[0] in bn))
    return out
