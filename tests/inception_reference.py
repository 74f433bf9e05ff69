"""The yardstick of the FID network: an independent fp64 restatement of the 2015 Inception-v3 feature extractor in the layout of
``pytorch-fid``'s ``pt_inception-2015-12-05`` port, with torch.nn.functional on the CPU.  Written from the network's description
(every unit a bias-free convolution, eval BatchNorm with eps 1e-3, ReLU), with the BatchNorm UNFOLDED - the fold of
map-dit_amd/fid.py is under test, not assumed - and module by module, not from a layer table.  The FID variant's three departures
from torchvision are here by name: average pools with count_include_pad=False, a max pool in Mixed_7c, bilinear resize to 299 with
align_corners=False."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-3
BETA0 = 0.25           # the mean of the BatchNorm shifts: keeps most units of a layer alive


class _Net:
    """Walks the network once.  With ``sd is None`` it CREATES each unit's parameters (seeded, He-scaled) as it meets it, on the way
    through a calibration batch; with a state dict it only computes.  One description, so the shapes the weights are made with and
    the ones the forward uses cannot differ."""

    def __init__(self, sd=None, gen=None, operand_dtype=None):
        self.sd, self.gen, self.make, self.od = ({} if sd is None else sd), gen, sd is None, operand_dtype

    def _rt(self, t):               # round to the kernels' operand format and back (None: exact fp64)
        return t if self.od is None else t.to(torch.float32).to(self.od).to(torch.float64)

    def unit(self, x, name, cin, cout, k=1, stride=1, pad=0):
        kh, kw = (k, k) if isinstance(k, int) else k
        if self.make:
            g = self.gen
            w = torch.randn(cout, cin, kh, kw, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (cin * kh * kw))
            self.sd[f"{name}.conv.weight"] = w
            self.sd[f"{name}.bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=g, dtype=torch.float64)
            self.sd[f"{name}.bn.bias"] = BETA0 + 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
            # running_mean: what the unit's convolution gives on the calibration images, as a trained BatchNorm would hold it, off by
            # 0.1 N(0, 1).  (Inputs are >= 0 after a ReLU: a filter's sum turns their mean into a per-channel constant; a running
            # mean that knows nothing of it leaves that constant in, it swamps the signal within a few layers and channels die.)
            self.sd[f"{name}.bn.running_mean"] = F.conv2d(x, w, None, stride, pad).mean(dim=(0, 2, 3)) + 0.1 * torch.randn(cout, generator=g, dtype=torch.float64)
            self.sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(cout, generator=g, dtype=torch.float64)
            self.sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(1)
        sd = self.sd
        w = sd[f"{name}.conv.weight"].double()
        gamma = sd.get(f"{name}.bn.weight")
        if self.od is not None:
            # the kernels multiply operands rounded to 16 bits: the folded weight and the activation; everything else stays exact
            s = (torch.ones(cout, dtype=torch.float64) if gamma is None else gamma.double()) / torch.sqrt(sd[f"{name}.bn.running_var"].double() + EPS)
            y = F.conv2d(self._rt(x), self._rt(w * s[:, None, None, None]), None, stride, pad)
            y = y + (sd[f"{name}.bn.bias"].double() - sd[f"{name}.bn.running_mean"].double() * s)[None, :, None, None]
            return F.relu(y)
        y = F.conv2d(x, w, None, stride, pad)
        y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].double(), sd[f"{name}.bn.running_var"].double(),
                         None if gamma is None else gamma.double(), sd[f"{name}.bn.bias"].double(), False, 0.0, EPS)
        return F.relu(y)

    def cat(self, xs):
        return torch.cat(xs, 1)

    def avg(self, x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    def max2(self, x):
        return F.max_pool2d(x, 3, 2)

    def max1(self, x):
        return F.max_pool2d(x, 3, 1, 1)

    def inception_a(self, x, p, cin, pool):
        b1 = self.unit(x, p + ".branch1x1", cin, 64)
        b5 = self.unit(self.unit(x, p + ".branch5x5_1", cin, 48), p + ".branch5x5_2", 48, 64, 5, 1, 2)
        b3 = self.unit(x, p + ".branch3x3dbl_1", cin, 64)
        b3 = self.unit(b3, p + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        b3 = self.unit(b3, p + ".branch3x3dbl_3", 96, 96, 3, 1, 1)
        bp = self.unit(self.avg(x), p + ".branch_pool", cin, pool)
        return self.cat([b1, b5, b3, bp])

    def inception_b(self, x, p):
        b3 = self.unit(x, p + ".branch3x3", 288, 384, 3, 2)
        bd = self.unit(x, p + ".branch3x3dbl_1", 288, 64)
        bd = self.unit(bd, p + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        bd = self.unit(bd, p + ".branch3x3dbl_3", 96, 96, 3, 2)
        return self.cat([b3, bd, self.max2(x)])

    def inception_c(self, x, p, c7):
        b1 = self.unit(x, p + ".branch1x1", 768, 192)
        b7 = self.unit(x, p + ".branch7x7_1", 768, c7)
        b7 = self.unit(b7, p + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        b7 = self.unit(b7, p + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        bd = self.unit(x, p + ".branch7x7dbl_1", 768, c7)
        bd = self.unit(bd, p + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        bd = self.unit(bd, p + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        bd = self.unit(bd, p + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        bd = self.unit(bd, p + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        bp = self.unit(self.avg(x), p + ".branch_pool", 768, 192)
        return self.cat([b1, b7, bd, bp])

    def inception_d(self, x, p):
        b3 = self.unit(self.unit(x, p + ".branch3x3_1", 768, 192), p + ".branch3x3_2", 192, 320, 3, 2)
        b7 = self.unit(x, p + ".branch7x7x3_1", 768, 192)
        b7 = self.unit(b7, p + ".branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
        b7 = self.unit(b7, p + ".branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
        b7 = self.unit(b7, p + ".branch7x7x3_4", 192, 192, 3, 2)
        return self.cat([b3, b7, self.max2(x)])

    def inception_e(self, x, p, cin, pool):
        b1 = self.unit(x, p + ".branch1x1", cin, 320)
        b3 = self.unit(x, p + ".branch3x3_1", cin, 384)
        b3 = self.cat([self.unit(b3, p + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), self.unit(b3, p + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))])
        bd = self.unit(x, p + ".branch3x3dbl_1", cin, 448)
        bd = self.unit(bd, p + ".branch3x3dbl_2", 448, 384, 3, 1, 1)
        bd = self.cat([self.unit(bd, p + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), self.unit(bd, p + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))])
        bp = self.unit(pool(x), p + ".branch_pool", cin, 192)
        return self.cat([b1, b3, bd, bp])

    def forward(self, x):
        x = self.unit(x, "Conv2d_1a_3x3", 3, 32, 3, 2)
        x = self.unit(x, "Conv2d_2a_3x3", 32, 32, 3)
        x = self.unit(x, "Conv2d_2b_3x3", 32, 64, 3, 1, 1)
        x = self.max2(x)
        x = self.unit(x, "Conv2d_3b_1x1", 64, 80)
        x = self.unit(x, "Conv2d_4a_3x3", 80, 192, 3)
        x = self.max2(x)
        x = self.inception_a(x, "Mixed_5b", 192, 32)
        x = self.inception_a(x, "Mixed_5c", 256, 64)
        x = self.inception_a(x, "Mixed_5d", 288, 64)
        x = self.inception_b(x, "Mixed_6a")
        x = self.inception_c(x, "Mixed_6b", 128)
        x = self.inception_c(x, "Mixed_6c", 160)
        x = self.inception_c(x, "Mixed_6d", 160)
        x = self.inception_c(x, "Mixed_6e", 192)
        x = self.inception_d(x, "Mixed_7a")
        x = self.inception_e(x, "Mixed_7b", 1280, self.avg)
        x = self.inception_e(x, "Mixed_7c", 2048, self.max1)               # the port's quirk: a max pool here
        return x.mean(dim=(2, 3))


def init_state_dict(seed=0, with_fc=True) -> dict:
    """A full fp64 state dict: He-scaled convolutions, BatchNorm gamma in [0.8, 1.2], beta = 0.25 + 0.1 N(0, 1), running_var in
    [0.5, 1.5], running_mean calibrated on two seeded noise images (``_Net.unit``) - features stay O(1) through the 47 layers of the
    longest path and no channel dies.  ``with_fc``: the classifier head and an auxiliary
    key, which a loader must ignore."""
    g = torch.Generator().manual_seed(seed)
    net = _Net(None, g)
    with torch.no_grad():
        net.forward(prepare(torch.randint(0, 256, (2, 16, 16, 3), generator=g, dtype=torch.uint8)))
    if with_fc:
        net.sd["fc.weight"], net.sd["fc.bias"] = torch.zeros(1008, 2048, dtype=torch.float64), torch.zeros(1008, dtype=torch.float64)
        net.sd["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1, dtype=torch.float64)
    return net.sd


def prepare(images) -> torch.Tensor:
    """uint8 [N, H, W, 3] -> fp64 [N, 3, 299, 299] in [-1, 1]: bilinear resize (align_corners=False, no antialiasing), then x / 255 * 2 - 1."""
    x = images.permute(0, 3, 1, 2).to(torch.float64)
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    return x / 255.0 * 2.0 - 1.0


@torch.no_grad()
def features(sd, images, operand_dtype=None) -> torch.Tensor:
    """fp64 [N, 2048] pool features of uint8 [N, H, W, 3] images.  ``operand_dtype``: round every convolution's activation and
    folded weight to that 16-bit format first (an emulation of the kernels' operand rounding; the sums stay fp64)."""
    return _Net(sd, operand_dtype=operand_dtype).forward(prepare(images))
