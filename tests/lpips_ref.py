"""A torch restatement of upstream LPIPS-VGG (lpips 0.1.x: lpips/lpips.py, lpips/pretrained_networks.py) in any dtype, and a seeded state dict under
upstream's key names.  The float64 evaluation is the answer of tests/test_gpu_lpips.py, the float32 one gives d32 (tests/test_gpu_vggt_heads.py's
convention).  Key names and structure are restated, not imported: neither lpips nor torchvision is a dependency."""
import functools

import torch
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))       # torchvision vgg16().features indices of the convolutions, per slice
CHNS = (64, 128, 256, 512, 512)
NET_CASES = ((3, 3, 16, 16), (2, 3, 35, 29), (2, 3, 70, 61))


def rel_err(got, want):
    """max-abs error over max-abs of the float64 answer"""
    want = want.double()
    return float((got.double().cpu() - want.cpu()).abs().max() / want.abs().max())


def make_state_dict(seed=0):
    """The full module form: net.slice{k}.{i}.weight|bias, lin{k}.model.1.weight [1,C,1,1] and its duplicate lins.{k}..., scaling_layer.shift|scale.
    He-scaled convolutions, biases 0.1 N(0,1), lin weights uniform in [0, 0.01)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    cin = 3
    for k, (idx, cout) in enumerate(zip(SLICES, CHNS)):
        for i in idx:
            sd[f"net.slice{k + 1}.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            sd[f"net.slice{k + 1}.{i}.bias"] = 0.1 * torch.randn(cout, generator=g)
            cin = cout
    for k, c in enumerate(CHNS):
        sd[f"lin{k}.model.1.weight"] = 0.01 * torch.rand(1, c, 1, 1, generator=g)
        sd[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    sd["scaling_layer.shift"] = torch.tensor([-.030, -.088, -.188])[None, :, None, None]
    sd["scaling_layer.scale"] = torch.tensor([.458, .448, .450])[None, :, None, None]
    return sd


def two_files(sd, seed=1):
    """The same weights as upstream ships them: (the lin-only file `weights/v0.1/vgg.pth`, torchvision's VGG16 state dict with `features.{i}.*` and
    `classifier.*`, the latter small stand-ins here)"""
    lin = {k: v for k, v in sd.items() if k.startswith("lin") and not k.startswith("lins.")}
    tv = {f"features.{k.split('.')[2]}.{k.split('.')[3]}": v for k, v in sd.items() if k.startswith("net.")}
    g = torch.Generator().manual_seed(seed)
    for i in (0, 3, 6):
        tv[f"classifier.{i}.weight"], tv[f"classifier.{i}.bias"] = torch.randn(4, 4, generator=g), torch.randn(4, generator=g)
    return lin, tv


def features(sd, x, dt):
    """the five taps BEFORE their ReLU (upstream taps relu1_2 ... relu5_3, i.e. F.relu of these), NCHW"""
    h = (x.to(dt) - sd["scaling_layer.shift"].to(dt)) / sd["scaling_layer.scale"].to(dt)
    taps = []
    for k, idx in enumerate(SLICES):
        if k:
            h = F.max_pool2d(F.relu(h), 2, 2)
        for j, i in enumerate(idx):
            h = F.conv2d(F.relu(h) if j else h, sd[f"net.slice{k + 1}.{i}.weight"].to(dt), sd[f"net.slice{k + 1}.{i}.bias"].to(dt), padding=1)
        taps.append(h)
    return taps


def normalize_tensor(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def layer(f0, f1, w):
    """one LPIPS layer of two feature maps [N,C,H,W] (after their ReLU) with the lin weight [1,C,1,1] -> [N]"""
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return F.conv2d(d, w.to(d.dtype)).mean(dim=(2, 3)).reshape(-1)


def lpips(sd, in0, in1, dt, normalize=False):
    """-> (total [N], per-layer [5][N]) in dtype dt"""
    if normalize:
        in0, in1 = 2 * in0.to(dt) - 1, 2 * in1.to(dt) - 1
    t0, t1 = features(sd, in0, dt), features(sd, in1, dt)
    per = [layer(F.relu(a), F.relu(b), sd[f"lin{k}.model.1.weight"]) for k, (a, b) in enumerate(zip(t0, t1))]
    val = per[0]
    for p in per[1:]:
        val = val + p
    return val, per


class Net:
    """the restatement as a callable perceptual network (what oracle.scorer.lpips_metric takes)"""

    def __init__(self, sd, dt):
        self.sd, self.dt = sd, dt

    def __call__(self, a, b):
        return lpips(self.sd, a, b, self.dt)[0].reshape(-1, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def state():
    return make_state_dict(0)


@functools.lru_cache(maxsize=None)
def net_case(shape):
    """inputs and both reference evaluations of one whole-network case, computed once per session: rep = clamp(gt + 0.3 N(0,1))"""
    g = torch.Generator().manual_seed(sum(shape))
    gt = torch.rand(shape, generator=g) * 2 - 1
    rep = (gt + 0.3 * torch.randn(shape, generator=g)).clamp(-1, 1)
    sd = state()
    with torch.no_grad():
        out = {"gt": gt, "rep": rep}
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            out["feat" + tag] = features(sd, gt, dt)
            out["val" + tag], out["per" + tag] = lpips(sd, gt, rep, dt)
    return out
