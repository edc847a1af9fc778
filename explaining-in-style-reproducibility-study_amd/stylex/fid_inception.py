"""The Inception-v3 of the Frechet Inception Distance (reference stylex/stylex_train.py:1579, 1622: the pytorch_fid
package), as an in-repo definition with the published state-dict layout — the treatment tv_models.py and lpips_alex.py
give the other two frozen networks.

Layout: torchvision's ``Inception3`` naming without ``AuxLogits``; every conv is a ``BasicConv2d`` (``conv`` without bias,
``bn`` with eps 0.001, ReLU); 94 convs.  The FID variant differs from torchvision's in two places: the pool branch of
``Mixed_5*``, ``Mixed_6b-6e`` and ``Mixed_7b`` is ``avg_pool2d(3, 1, 1, count_include_pad=False)``, and the pool branch of
``Mixed_7c`` is ``max_pool2d(3, 1, 1)``.  The module ends at the last feature map [B, 2048, 8, 8]: the global average
pool is part of the moments kernel (hip_backend.fid_moments_acc).

Weights: ``pt_inception-2015-12-05-6726825d.pth``, loaded by key (``fc.*`` and ``*.num_batches_tracked`` ignored, every
other key required).  Nothing is downloaded; a missing file is an error that names it; ``random:<seed>`` builds seeded
weights for tests and timing.  Written from the package's published layout and not checked against the package itself
(it is not installable here): "parity unpinned" in DESIGN.md §11.

On the GPU in fp32 the forward keeps the convolutions on the stock library, as the frozen classifier does; the eval
BatchNorm + ReLU behind each is one launch of ``stylex_affine_act_nchw_fwd``, and the last layer of a branch writes its
channel slice of the block's output through ``stylex_affine_act_nchw_slice_fwd``, so no ``torch.cat`` runs.
"""
import hashlib
import os

import torch
import torch.nn.functional as F
from torch import nn

WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"


class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _avg_pool(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def _max_pool_same(x):
    return F.max_pool2d(x, 3, 1, 1)


def _max_pool_down(x):
    return F.max_pool2d(x, 3, 2)


class _Mixed(nn.Module):
    """One Inception block: parallel branches over the same input, concatenated along channels.  A branch is (pool, layer
    names): the pool (or None) runs first, then the named BasicConv2d children in order; a branch without layers passes its
    pooled input through.  A name may be a tuple of names: those layers read the same tensor and their outputs are
    concatenated (the 1x3 / 3x1 fork of the E blocks)."""

    def __init__(self, layers, branches):
        super().__init__()
        for name, (cin, cout, k, s, p) in layers.items():
            setattr(self, name, BasicConv2d(cin, cout, k, s, p))
        self._branches = branches
        widths = []
        for pool, names in branches:
            last = names[-1] if names else None
            if last is None:
                widths.append(None)  # pass-through: the block's input width
            else:
                widths.append(sum(layers[n][1] for n in (last if isinstance(last, tuple) else (last,))))
        self._widths = widths
        self._cin = next(iter(layers.values()))[0]
        self.out_channels = sum(self._cin if w is None else w for w in widths)

    def forward(self, x, tails=None):
        """tails = None: plain ATen (any device, any float dtype).  Otherwise the _Tails of the device path."""
        if tails is None:
            outs = []
            for pool, names in self._branches:
                t = pool(x) if pool is not None else x
                for n in names:
                    t = torch.cat([getattr(self, m)(t) for m in n], 1) if isinstance(n, tuple) else getattr(self, n)(t)
                outs.append(t)
            return torch.cat(outs, 1)
        out, c0 = None, 0
        for (pool, names), width in zip(self._branches, self._widths):
            t = pool(x) if pool is not None else x
            if out is None:  # the output's spatial size: that of any branch; ask the first one's geometry
                h, w = self._out_hw(t, names)
                out = torch.empty((x.shape[0], self.out_channels, h, w), dtype=torch.float32, device=x.device)
            if not names:
                out[:, c0:c0 + t.shape[1]].copy_(t)
                c0 += t.shape[1]
                continue
            for n in names[:-1]:
                t = tails.layer(getattr(self, n), t)
            last = names[-1]
            for m in (last if isinstance(last, tuple) else (last,)):
                layer = getattr(self, m)
                tails.layer_into(layer, t, out, c0)
                c0 += layer.conv.out_channels
        return out

    def _out_hw(self, t, names):
        h, w = t.shape[2], t.shape[3]
        for n in names:
            c = getattr(self, n[0] if isinstance(n, tuple) else n).conv
            h = (h + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
            w = (w + 2 * c.padding[1] - c.kernel_size[1]) // c.stride[1] + 1
        return h, w


def _block_a(cin, pool_features):
    layers = {"branch1x1": (cin, 64, 1, 1, 0),
              "branch5x5_1": (cin, 48, 1, 1, 0), "branch5x5_2": (48, 64, 5, 1, 2),
              "branch3x3dbl_1": (cin, 64, 1, 1, 0), "branch3x3dbl_2": (64, 96, 3, 1, 1), "branch3x3dbl_3": (96, 96, 3, 1, 1),
              "branch_pool": (cin, pool_features, 1, 1, 0)}
    return _Mixed(layers, [(None, ["branch1x1"]), (None, ["branch5x5_1", "branch5x5_2"]),
                           (None, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"]), (_avg_pool, ["branch_pool"])])


def _block_b(cin):
    layers = {"branch3x3": (cin, 384, 3, 2, 0),
              "branch3x3dbl_1": (cin, 64, 1, 1, 0), "branch3x3dbl_2": (64, 96, 3, 1, 1), "branch3x3dbl_3": (96, 96, 3, 2, 0)}
    return _Mixed(layers, [(None, ["branch3x3"]), (None, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"]),
                           (_max_pool_down, [])])


def _block_c(cin, c7):
    layers = {"branch1x1": (cin, 192, 1, 1, 0),
              "branch7x7_1": (cin, c7, 1, 1, 0), "branch7x7_2": (c7, c7, (1, 7), 1, (0, 3)),
              "branch7x7_3": (c7, 192, (7, 1), 1, (3, 0)),
              "branch7x7dbl_1": (cin, c7, 1, 1, 0), "branch7x7dbl_2": (c7, c7, (7, 1), 1, (3, 0)),
              "branch7x7dbl_3": (c7, c7, (1, 7), 1, (0, 3)), "branch7x7dbl_4": (c7, c7, (7, 1), 1, (3, 0)),
              "branch7x7dbl_5": (c7, 192, (1, 7), 1, (0, 3)),
              "branch_pool": (cin, 192, 1, 1, 0)}
    return _Mixed(layers, [(None, ["branch1x1"]), (None, ["branch7x7_1", "branch7x7_2", "branch7x7_3"]),
                           (None, ["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"]),
                           (_avg_pool, ["branch_pool"])])


def _block_d(cin):
    layers = {"branch3x3_1": (cin, 192, 1, 1, 0), "branch3x3_2": (192, 320, 3, 2, 0),
              "branch7x7x3_1": (cin, 192, 1, 1, 0), "branch7x7x3_2": (192, 192, (1, 7), 1, (0, 3)),
              "branch7x7x3_3": (192, 192, (7, 1), 1, (3, 0)), "branch7x7x3_4": (192, 192, 3, 2, 0)}
    return _Mixed(layers, [(None, ["branch3x3_1", "branch3x3_2"]),
                           (None, ["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"]),
                           (_max_pool_down, [])])


def _block_e(cin, pool):
    layers = {"branch1x1": (cin, 320, 1, 1, 0),
              "branch3x3_1": (cin, 384, 1, 1, 0), "branch3x3_2a": (384, 384, (1, 3), 1, (0, 1)),
              "branch3x3_2b": (384, 384, (3, 1), 1, (1, 0)),
              "branch3x3dbl_1": (cin, 448, 1, 1, 0), "branch3x3dbl_2": (448, 384, 3, 1, 1),
              "branch3x3dbl_3a": (384, 384, (1, 3), 1, (0, 1)), "branch3x3dbl_3b": (384, 384, (3, 1), 1, (1, 0)),
              "branch_pool": (cin, 192, 1, 1, 0)}
    return _Mixed(layers, [(None, ["branch1x1"]), (None, ["branch3x3_1", ("branch3x3_2a", "branch3x3_2b")]),
                           (None, ["branch3x3dbl_1", "branch3x3dbl_2", ("branch3x3dbl_3a", "branch3x3dbl_3b")]),
                           (pool, ["branch_pool"])])


class _Tails:
    """The device path's layer: library convolution, then the eval BatchNorm + ReLU as one launch.  (scale, shift) of a layer
    are computed once per Inception instance and device."""

    def __init__(self, cache):
        import hip_backend as hb

        self.hb, self.cache = hb, cache

    def _affine(self, layer):
        sc = self.cache.get(layer)
        if sc is None:
            from frozen_resnet import _affine

            sc = self.cache[layer] = _affine(layer.bn)
        return sc

    def _conv(self, layer, x):
        c = layer.conv
        return F.conv2d(x, c.weight, None, c.stride, c.padding)

    def layer(self, layer, x):
        scale, shift = self._affine(layer)
        return self.hb.affine_act_fwd(self._conv(layer, x).contiguous(), scale, shift, relu=True)

    def layer_into(self, layer, x, out, c0):
        scale, shift = self._affine(layer)
        self.hb.affine_act_slice_fwd(self._conv(layer, x).contiguous(), scale, shift, out, c0, relu=True)


_STEM = [("Conv2d_1a_3x3", (3, 32, 3, 2, 0)), ("Conv2d_2a_3x3", (32, 32, 3, 1, 0)), ("Conv2d_2b_3x3", (32, 64, 3, 1, 1)),
         ("Conv2d_3b_1x1", (64, 80, 1, 1, 0)), ("Conv2d_4a_3x3", (80, 192, 3, 1, 0))]
_POOL_AFTER = ("Conv2d_2b_3x3", "Conv2d_4a_3x3")  # max_pool2d(3, 2) behind these stem layers
_BLOCKS = ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a",
           "Mixed_7b", "Mixed_7c"]


class FIDInceptionV3(nn.Module):
    """[B, 3, 299, 299] in [-1, 1] -> the last feature map [B, 2048, 8, 8] (its spatial mean is the FID feature)."""

    def __init__(self):
        super().__init__()
        for name, (cin, cout, k, s, p) in _STEM:
            setattr(self, name, BasicConv2d(cin, cout, k, s, p))
        self.Mixed_5b, self.Mixed_5c, self.Mixed_5d = _block_a(192, 32), _block_a(256, 64), _block_a(288, 64)
        self.Mixed_6a = _block_b(288)
        self.Mixed_6b, self.Mixed_6c = _block_c(768, 128), _block_c(768, 160)
        self.Mixed_6d, self.Mixed_6e = _block_c(768, 160), _block_c(768, 192)
        self.Mixed_7a = _block_d(768)
        self.Mixed_7b, self.Mixed_7c = _block_e(1280, _avg_pool), _block_e(2048, _max_pool_same)
        self._affine_cache = {}
        self.weights_id = None  # set by the loaders: what a cached statistics file is tagged with
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)

    def _apply(self, fn, *a, **k):  # .to() / .double(): the folded BatchNorm vectors belong to the old tensors
        self._affine_cache = {}
        return super()._apply(fn, *a, **k)

    def forward(self, x, plain=None, taps=None):
        """plain = True: ATen only; False: the fused tails (GPU, fp32); None: fused wherever they apply.  `taps` (a dict)
        receives the output of every Mixed block by name."""
        fused = x.is_cuda and x.dtype == torch.float32
        if plain is False and not fused:
            raise RuntimeError("the fused Inception forward runs on the GPU in fp32 (got %s, %s)" % (x.device, x.dtype))
        tails = _Tails(self._affine_cache) if (fused and not plain) else None
        for name, _ in _STEM:
            layer = getattr(self, name)
            x = layer(x) if tails is None else tails.layer(layer, x)
            if name in _POOL_AFTER:
                x = F.max_pool2d(x, 3, 2)
        for name in _BLOCKS:
            x = getattr(self, name)(x, tails)
            if taps is not None:
                taps[name] = x
        return x

    # ---- weights --------------------------------------------------------------------------------------------------

    def load_fid_state_dict(self, sd):
        """Load pytorch_fid's state dict by key: `fc.*` and `*.num_batches_tracked` are ignored, every other key of this
        module is required and no other key is accepted; the error names what is missing or unexpected."""
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.") and not k.endswith("num_batches_tracked")}
        own = {k: v for k, v in self.state_dict().items() if not k.endswith("num_batches_tracked")}
        missing = sorted(set(own) - set(sd))
        unexpected = sorted(set(sd) - set(own))
        bad = sorted(k for k in own if k in sd and tuple(sd[k].shape) != tuple(own[k].shape))
        if missing or unexpected or bad:
            raise KeyError("FID Inception weights do not match: missing keys %s; unexpected keys %s; wrong shapes %s"
                           % (missing, unexpected, bad))
        with torch.no_grad():
            for k, v in own.items():
                v.copy_(sd[k])
        self._affine_cache = {}
        return self

    def init_random(self, seed):
        """Seeded stand-in weights (tests, timing): conv weights N(0, 2 / fan_in); BatchNorm gamma 1, beta 0, running mean 0,
        running variance 1."""
        g = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                    w = torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5
                    m.weight.copy_(w.to(m.weight.dtype))
                elif isinstance(m, nn.BatchNorm2d):
                    m.weight.fill_(1.)
                    m.bias.zero_()
                    m.running_mean.zero_()
                    m.running_var.fill_(1.)
        self._affine_cache = {}
        self.weights_id = "random:%d" % int(seed)
        return self


def resolve_weights(spec=None):
    """The weight file to use: `spec` (Trainer(fid_weights=...), --fid_weights), else $STYLEX_FID_WEIGHTS, else torch hub's
    checkpoint folder.  `random:<seed>` is returned as it is.  Nothing is downloaded: a missing file raises, naming it."""
    spec = spec or os.environ.get("STYLEX_FID_WEIGHTS")
    if spec and str(spec).startswith("random:"):
        return str(spec)
    path = str(spec) if spec else os.path.join(os.path.expanduser("~"), ".cache", "torch", "hub", "checkpoints", WEIGHTS_FILE)
    if not os.path.isfile(path):
        raise FileNotFoundError("FID needs the Inception weights of pytorch_fid (%s): no such file: %s.  Give its path with "
                                "fid_weights= / --fid_weights or STYLEX_FID_WEIGHTS (nothing is downloaded, and a FID from "
                                "random weights would be a meaningless number; fid_weights='random:<seed>' is for tests and "
                                "timing only)" % (WEIGHTS_FILE, path))
    return path


def build(spec=None, device=None):
    """FIDInceptionV3 with the weights `spec` resolves to, on `device`."""
    src = resolve_weights(spec)
    net = FIDInceptionV3()
    if src.startswith("random:"):
        net.init_random(int(src.split(":", 1)[1]))
    else:
        h = hashlib.sha256()
        with open(src, "rb") as f:
            for chunk in iter(lambda: f.read(1 << 20), b""):
                h.update(chunk)
        net.load_fid_state_dict(torch.load(src, map_location="cpu", weights_only=True))
        net.weights_id = "sha256:" + h.hexdigest()[:16]
    return net.to(device) if device is not None else net
