"""CPU restatement of torchvision's densenet121 features (conv0 / norm0 / pool0, four dense blocks with transitions, norm5,
relu, global average pool) and the reference's HDEN head (Dropout(.3), Linear(1024, 256), ReLU, Dropout(.2), Linear(256, 3)),
in whatever dtype the state_dict has (float64 for the oracle, float32 for the fp32 error yardstick).  Test helper only.

`state_dict` tensors are used in place: in train mode F.batch_norm updates the running buffers the way nn.BatchNorm2d does
(momentum 0.1, unbiased running variance) and num_batches_tracked is incremented.  `relu_masks` maps a parameter name to the
0/1 mask a ReLU must use instead of its own sign test (replaying the kinks the HIP kernels saw):
  <p>.conv0.weight         relu0 after norm0            <p>.<layer>.norm1.weight   the pre-activation ReLU of norm1
  <p>.<layer>.conv1.weight the ReLU after norm2          <p>.transitionK.norm.weight, <p>.norm5.weight  likewise
"""
import torch
import torch.nn.functional as F

BLOCKS = (6, 12, 24, 16)
P = "backbone.features."


def _bn(x, sd, name, training):
    if training:
        sd[name + ".num_batches_tracked"] += 1
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        training=training, momentum=0.1, eps=1e-5)


def _relu(y, key, relu_masks):
    if relu_masks is not None and key in relu_masks:
        return y * relu_masks[key].to(y.dtype)
    return F.relu(y)


def features(x, sd, training=False, relu_masks=None):
    """[N,3,H,W] -> pooled features [N,1024]"""
    h = F.conv2d(x, sd[P + "conv0.weight"], stride=2, padding=3)
    h = _relu(_bn(h, sd, P + "norm0", training), P + "conv0.weight", relu_masks)
    h = F.max_pool2d(h, 3, 2, 1)
    for bi, nl in enumerate(BLOCKS, start=1):
        feats = [h]
        for li in range(1, nl + 1):
            q = f"{P}denseblock{bi}.denselayer{li}"
            cat = torch.cat(feats, 1)
            a = _relu(_bn(cat, sd, q + ".norm1", training), q + ".norm1.weight", relu_masks)
            b = F.conv2d(a, sd[q + ".conv1.weight"])
            b = _relu(_bn(b, sd, q + ".norm2", training), q + ".conv1.weight", relu_masks)
            feats.append(F.conv2d(b, sd[q + ".conv2.weight"], padding=1))
        h = torch.cat(feats, 1)
        if bi < 4:
            q = f"{P}transition{bi}"
            a = _relu(_bn(h, sd, q + ".norm", training), q + ".norm.weight", relu_masks)
            h = F.avg_pool2d(F.conv2d(a, sd[q + ".conv.weight"]), 2, 2)
    h = _relu(_bn(h, sd, P + "norm5", training), P + "norm5.weight", relu_masks)
    return F.adaptive_avg_pool2d(h, 1).flatten(1)


def classifier_forward(x, sd, training=False, drop_masks=None, relu_masks=None):
    """-> (logits [N,3], features [N,1024]); drop_masks = (m0 [N,1024], m1 [N,256]) pre-scaled dropout masks (train mode)"""
    feats = features(x, sd, training, relu_masks)
    h = feats if drop_masks is None else feats * drop_masks[0]
    h = F.relu(F.linear(h, sd["classifier.1.weight"], sd["classifier.1.bias"]))
    if drop_masks is not None:
        h = h * drop_masks[1]
    return F.linear(h, sd["classifier.4.weight"], sd["classifier.4.bias"]), feats
