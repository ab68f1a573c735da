"""Deterministic PointRCNN parameters and buffers, keyed by state_dict name and
module kind (shared by the golden generator and the tests: the model has about
3.9 M parameters at the yml's widths, so no weights are stored).

BatchNorm weight 1 + 0.1 N, bias 0.1 N, running mean 0.1 N, running variance
U[1, 1.5); conv weight N * sqrt(2 / fan-in) (ReLU networks keep their scale),
bias 0.05 N; each from default_rng(crc32(name)).  The last conv of every head
(rpn / rcnn cls_blocks and reg_blocks) gets a gain so that scores and bin
logits spread over O(1) instead of the reference's 1e-3 init, where every
argmax would be a near-tie; the three size residuals (last rows of a reg head)
get a tenth of it, so that decoded box sizes stay positive and car-like; the
RCNN's score bias is shifted so that the score threshold splits the rois."""
import zlib

import numpy as np
import torch

HEAD_GAIN = {"rpn.cls_blocks.4": 16.0, "rpn.reg_blocks.4": 4.0, "rcnn.cls_blocks.4": 4.0, "rcnn.reg_blocks.4": 4.0}
SIZE_GAIN = 0.1
BIAS_SHIFT = {"rcnn.cls_blocks.4": -2.0}  # so that the score threshold keeps some rois and drops others


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
    module = name.rsplit(".", 1)[0]
    gain = np.full((shape[0],) + (1,) * (len(shape) - 1), HEAD_GAIN.get(module, 1.0))
    if module in HEAD_GAIN and "reg_blocks" in module:
        gain[-3:] *= SIZE_GAIN
    if name.endswith("bias"):
        return (0.05 * rng.standard_normal(shape) * gain + BIAS_SHIFT.get(module, 0.0)).astype(np.float32)
    fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    return (rng.standard_normal(shape) * np.sqrt(2.0 / max(fan_in, 1)) * gain).astype(np.float32)


def state_dict_for(model):
    """Values for every entry of model.state_dict(), in its order."""
    bn = {name for name, mod in model.named_modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)}
    out = {}
    for k, v in model.state_dict().items():
        out[k] = torch.from_numpy(fill(k, tuple(v.shape), k.rsplit(".", 1)[0] in bn))
    return out
