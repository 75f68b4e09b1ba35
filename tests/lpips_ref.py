"""A float64 torch restatement of LPIPS over VGG16 and of the kernels of csrc/lpips.hip, written from the arithmetic:
what tests/test_lpips_*.py compare against.  CPU, NCHW throughout; the GPU tests permute.

    scaled   s = (x - shift[c]) / scale[c]
    VGG16    conv3x3(pad 1) + ReLU thirteen times, MaxPool2d(2, 2) before convolutions 3, 5, 8 and 11; the taps are the ReLU
             outputs of convolutions 2, 4, 7, 10 and 13
    layer    n_i = sqrt(sum_c f_i^2), u_i = f_i / (n_i + 1e-10), s = sum_c w_c (u0_c - u1_c)^2, res[b] = mean over the pixels of s
    value    res of lin0 + ... + lin4, in that order"""
import torch
import torch.nn.functional as F

SLICES = ((("net.slice1.0", "net.slice1.2")), ("net.slice2.5", "net.slice2.7"), ("net.slice3.10", "net.slice3.12", "net.slice3.14"),
          ("net.slice4.17", "net.slice4.19", "net.slice4.21"), ("net.slice5.24", "net.slice5.26", "net.slice5.28"))
EPS = 1e-10


def lin_weights(sd):
    """the five 1x1 weights as (C,) float64, whichever of model.0 / model.1 the state dict uses"""
    out = []
    for k in range(5):
        key = [n for n in sd if n.startswith(f"lin{k}.model.") and n.endswith(".weight")]
        assert len(key) == 1, key
        out.append(sd[key[0]].double().reshape(-1))
    return out


def conv_in(x, w, b, shift, scale):
    """x (n,3,h,w) -> relu(conv(scaled x) + b), (n,64,h,w); the zero padding is of the scaled tensor"""
    s = (x.double() - shift.double().view(1, 3, 1, 1)) / scale.double().view(1, 3, 1, 1)
    return F.relu(F.conv2d(s, w.double(), b.double(), padding=1))


def conv_in_bwd(dy, y, w, scale):
    """dy, y (n,64,h,w): the gradient with respect to x of <dy, relu(conv(scaled x) + b)> where y > 0 is the ReLU mask"""
    g = torch.where(y.double() > 0, dy.double(), torch.zeros((), dtype=torch.float64))
    ds = F.conv_transpose2d(g, w.double(), padding=1)
    return ds / scale.double().view(1, 3, 1, 1)


def relu_maxpool2(x):
    """x (n,c,h,w) -> (pooled (n,c,h//2,w//2), relu(x))"""
    r = F.relu(x.double())
    return F.max_pool2d(r, 2, 2), r


def relu_maxpool2_bwd(x, dy):
    """The first maximum of relu(x) in row-major window order takes dy (strict > while scanning), then the ReLU mask x > 0;
    dropped odd rows and columns get 0.  Written as the scan itself."""
    x, dy = x.double(), dy.double()
    n, c, h, w = x.shape
    ph, pw = h // 2, w // 2
    r = F.relu(x)
    dx = torch.zeros_like(x)
    win = [r[:, :, dy_:2 * ph:2, dx_:2 * pw:2] for dy_ in (0, 1) for dx_ in (0, 1)]          # row-major window order
    best, arg = win[0].clone(), torch.zeros_like(win[0], dtype=torch.long)
    for j in (1, 2, 3):
        better = win[j] > best
        best = torch.where(better, win[j], best)
        arg = torch.where(better, torch.full_like(arg, j), arg)
    for j in range(4):
        oy, ox = j >> 1, j & 1
        xs = x[:, :, oy:2 * ph:2, ox:2 * pw:2]
        dx[:, :, oy:2 * ph:2, ox:2 * pw:2] = torch.where((arg == j) & (xs > 0), dy, torch.zeros_like(dy))
    return dx


def normalize(f):
    n = torch.sqrt((f ** 2).sum(dim=1, keepdim=True))
    return f / (n + EPS), n


def layer(f0, f1, w):
    """f0, f1 (n,C,h,w) float64, w (C,) -> res (n,)"""
    u0, _ = normalize(f0.double())
    u1, _ = normalize(f1.double())
    s = (w.double().view(1, -1, 1, 1) * (u0 - u1) ** 2).sum(dim=1)
    return s.mean(dim=(1, 2))


def layer_bwd(fa, fb, w, g):
    """The gradient of sum_b g[b] res[b] with respect to fa, the closed form; where |fa| = 0 the norm term is taken as 0
    (torch autograd has 0/0 there), so the result is r * a."""
    fa, fb, g = fa.double(), fb.double(), g.double()
    hw = fa.shape[2] * fa.shape[3]
    ua, na = normalize(fa)
    ub, _ = normalize(fb)
    a = 2.0 * w.double().view(1, -1, 1, 1) * (ua - ub) * g.view(-1, 1, 1, 1) / hw
    r = 1.0 / (na + EPS)
    dot = (a * fa).sum(dim=1, keepdim=True)
    q = torch.where(na > 0, dot / (torch.where(na > 0, na, torch.ones_like(na)) * (na + EPS) ** 2), torch.zeros_like(na))
    return r * a - fa * q


def features(x, sd):
    """the five taps of the scaled image x (n,3,h,w), float64"""
    h = (x.double() - sd["scaling_layer.shift"].double()) / sd["scaling_layer.scale"].double()
    taps = []
    for k, names in enumerate(SLICES):
        if k > 0:
            h = F.max_pool2d(h, 2, 2)
        for name in names:
            h = F.relu(F.conv2d(h, sd[name + ".weight"].double(), sd[name + ".bias"].double(), padding=1))
        taps.append(h)
    return taps


def lpips(x0, x1, sd):
    """-> val (n,1,1,1) float64; differentiable by torch autograd with respect to x0 and x1 (float64 leaves)"""
    f0, f1 = features(x0, sd), features(x1, sd)
    val = None
    for a, b, w in zip(f0, f1, lin_weights(sd)):
        r = layer(a, b, w)
        val = r if val is None else val + r
    return val.view(-1, 1, 1, 1)


def value_and_grads(x0, x1, sd, g=None):
    """-> (val (n,1,1,1), d/dx0, d/dx1) of sum_b g[b] val[b] (g None: ones), float64"""
    a, b = x0.double().clone().requires_grad_(True), x1.double().clone().requires_grad_(True)
    val = lpips(a, b, sd)
    gg = torch.ones_like(val) if g is None else g.double().view_as(val)
    ga, gb = torch.autograd.grad((val * gg).sum(), (a, b))
    return val.detach(), ga, gb
