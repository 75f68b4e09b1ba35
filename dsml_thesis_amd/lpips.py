"""LPIPS over VGG16 (taming/modules/losses/lpips.py, vendored in both reference trees) on HIP: the perceptual term of
`VQLPIPSWithDiscriminator` and `LPIPSWithDiscriminator`, value and image gradient, with no torch convolution in it.

    val[b] = sum_k mean_pixels sum_c lin_k[c] (u0 - u1)^2,   u = f / (|f|_2 + 1e-10),   f = the five taps relu1_2 ... relu5_3

Dataflow.  The image enters through ldmk_lpips_conv_in (ScalingLayer on load, conv1_1, ReLU, NCHW -> NHWC); the twelve
other convolutions are `ops.conv3x3` with bias at LDMK_COMPUTE_F32, their data gradients `train_ops.conv3x3_dgrad` on weights packed
once, both with a shared split-K scratch (below: faster at small row counts, and shorter fp32 summation chains); ReLU + MaxPool2d(2, 2) at the four pooling points is one kernel that also leaves the post-ReLU tap in place of the
pre-activations; the inner ReLUs are the in-place ldmk_relu / ldmk_relu_bwd with the post-ReLU map as the mask; one
ldmk_lpips_layer(+_bwd) per tap.  The network is frozen: there is no weight gradient.  The two branches run slice by slice, so
what stays alive is the five taps of each branch, plus the inner post-ReLU maps of a branch that needs a gradient.

The class is eval-only: the reference's loss classes call `LPIPS().eval()`, dropout is never applied here, and `train()` leaves
the module in eval mode.  Nothing is ever downloaded: weights come from `load_state_dict` or from two local files."""
import torch
import torch.nn as nn

from . import lib as L
from . import ops
from . import train_ops as T
from .train import _splitk_ws as _scratch
from .synth import LPIPS_CHNS, LPIPS_SCALE, LPIPS_SHIFT, LPIPS_VGG

# The GEMMs split K into the trainers' split-K scratch (train._splitk_ws: ONE buffer per device for the whole process, which the
# first-stage trainer's own GEMMs already use, so LPIPS inside a training step holds no second one).  With a scratch the planner
# splits K where the output has fewer tiles than the chip has CUs -- 4 to 16 ways at the deep slices -- and each partial sum is a
# shorter fp32 chain.  The reuse is stream-ordered: like the trainers, LPIPS assumes that one stream per device runs it at a time;
# two streams evaluating LPIPS (or LPIPS and a trainer) concurrently on one device would share the slabs and must not be used.
# torchvision vgg16 `features` index of a convolution -> its slice
_SLICE_OF = {i: k for k, convs in LPIPS_VGG for i, _, _ in convs}


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(LPIPS_SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(LPIPS_SCALE)[None, :, None, None])


class NetLinLayer(nn.Module):
    """The reference's 1x1 'lin' layer: `model.1.weight` behind a Dropout that eval mode never applies, `model.0.weight` without."""

    def __init__(self, chn_in, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers.append(nn.utils.skip_init(nn.Conv2d, chn_in, 1, 1, stride=1, padding=0, bias=False))
        self.model = nn.Sequential(*layers)


class _VGG16Slices(nn.Module):
    """The parameter holders of the thirteen convolutions under the reference's names, `slice{k}.{features index}`."""

    def __init__(self):
        super().__init__()
        for k, convs in LPIPS_VGG:
            s = nn.Sequential()
            for i, cin, cout in convs:
                s.add_module(str(i), nn.utils.skip_init(nn.Conv2d, cin, cout, 3, padding=1))
            setattr(self, f"slice{k}", s)


class _LPIPSFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, target, module, needs):
        val, saved = module._forward(input, target, needs)
        ctx.module, ctx.saved_state, ctx.needs = module, saved, needs
        return val.view(-1, 1, 1, 1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        g = grad_output.reshape(-1).contiguous().float()
        grads = [ctx.module._backward(ctx.saved_state, br, g) if ctx.needs[br] else None for br in (0, 1)]
        return grads[0], grads[1], None, None


class LPIPS(nn.Module):
    """Weights count as present only once they came through `load_state_dict` (or a parent module's load, or the two checkpoint
    arguments): that hook is what marks them loaded.  Values written into the parameters directly (`p.copy_(...)`) are picked up
    by the repack, but do not lift the refusal of a module that never had a load."""

    def __init__(self, use_dropout=True, vgg_ckpt=None, lpips_ckpt=None):
        """vgg_ckpt: a local file holding the torchvision vgg16 state dict (`features.N.*`) or `net.slice*` keys (a full LPIPS
        state dict serves for both arguments); lpips_ckpt: the lin-layer file (`lin{k}.model.{0|1}.weight`, either index).  With
        neither, the parameters are allocated but hold nothing, and `forward` refuses until `load_state_dict` has run."""
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = list(LPIPS_CHNS)
        self.net = _VGG16Slices()
        self._lin_index = 1 if use_dropout else 0
        for k, c in enumerate(self.chns):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        for p in self.parameters():
            p.requires_grad = False
        self._have = set()                       # which of "net", "lin" a load has filled
        self._packed, self._pack_sig = None, None
        if vgg_ckpt is not None:
            self._load_file(vgg_ckpt, "net")
        if lpips_ckpt is not None:
            self._load_file(lpips_ckpt, "lin")
        super().train(False)

    def train(self, mode=True):
        """Eval-only: dropout is never applied and nothing here is trainable, so the mode stays eval."""
        return super().train(False)

    # ------------------------------------------------------------------------------------------ weights
    def _vgg_keys(self):
        return [f"net.slice{k}.{i}.{s}" for k, convs in LPIPS_VGG for i, _, _ in convs for s in ("weight", "bias")]

    def _lin_keys(self):
        return [f"lin{k}.model.{self._lin_index}.weight" for k in range(5)]

    def _load_file(self, path, part):
        sd = torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
        mine = {}
        for key, v in sd.items():
            f = key.split(".")
            if part == "net" and f[0] == "features" and len(f) == 3 and f[1].isdigit() and int(f[1]) in _SLICE_OF:
                mine[f"net.slice{_SLICE_OF[int(f[1])]}.{f[1]}.{f[2]}"] = v
            elif part == "net" and key.startswith("net.slice"):
                mine[key] = v
            elif part == "lin" and len(f) == 4 and f[0].startswith("lin") and f[1] == "model" and f[3] == "weight":
                mine[f"{f[0]}.model.{self._lin_index}.weight"] = v
        want = self._vgg_keys() if part == "net" else self._lin_keys()
        missing = [k for k in want if k not in mine]
        if missing:
            raise KeyError(f"LPIPS: {path} lacks {len(missing)} of the {len(want)} {part} tensors, first {missing[0]!r} "
                           "(a torchvision vgg16 state dict, `features.N.*`, or `net.slice*` keys; `lin{k}.model.*.weight` for the lin file)")
        self.load_state_dict({k: mine[k] for k in want}, strict=False)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """The hook `load_state_dict` and a parent module's load both go through: note what arrived, repack before the next call."""
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if all(prefix + k in state_dict for k in self._vgg_keys()):
            self._have.add("net")
        if all(prefix + k in state_dict for k in self._lin_keys()):
            self._have.add("lin")
        self._packed, self._pack_sig = None, None

    def _signature(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    @torch.no_grad()
    def pack_weights(self):
        """Kernel-layout copies of the frozen weights: ops.pack_conv3x3 for the forward GEMMs, pack_dgrad3x3 for the data gradients."""
        sd = {k: v.detach().float().contiguous() for k, v in self.state_dict().items()}
        dev = sd["net.slice1.0.weight"].device
        if dev.type != "cuda":
            raise L.LdmkError("LPIPS: the weights are on the CPU; move the module to the GPU (.cuda()) -- there is no CPU path")
        L.init(dev.index if dev.index is not None else torch.cuda.current_device())
        # every entry is a copy of its own (the unpacked ones too): a tape that keeps P is untouched by a later in-place load
        P = dict(w0=sd["net.slice1.0.weight"].clone(), b0=sd["net.slice1.0.bias"].clone(),
                 shift=sd["scaling_layer.shift"].reshape(3).clone(), scale=sd["scaling_layer.scale"].reshape(3).clone(), slices=[],
                 lin=[sd[k].reshape(-1).clone() for k in self._lin_keys()])
        for k, convs in LPIPS_VGG:
            recs = []
            for i, cin, cout in convs:
                if i == 0:
                    continue
                wp = ops.pack_conv3x3(sd[f"net.slice{k}.{i}.weight"])
                recs.append(dict(wp=wp, wd=T.pack_dgrad3x3(wp, cin, cout), b=sd[f"net.slice{k}.{i}.bias"].clone(), cin=cin, cout=cout))
            P["slices"].append(recs)
        self._packed, self._pack_sig = P, self._signature()

    def _require_weights(self):
        lack = [p for p in ("net", "lin") if p not in self._have]
        if lack:
            raise RuntimeError("LPIPS: no weights loaded (" + " and ".join({"net": "the VGG16 convolutions", "lin": "the lin layers"}[p] for p in lack)
                               + " are uninitialised): pass vgg_ckpt= / lpips_ckpt= local files or call load_state_dict first; "
                               "nothing is downloaded")

    def _ensure_packed(self):
        if self._packed is None or self._pack_sig != self._signature():
            self.pack_weights()

    # ------------------------------------------------------------------------------------------ the network
    def _check(self, input, target):
        for name, t in (("input", input), ("target", target)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3
                    and t.shape[2] >= 16 and t.shape[3] >= 16):
                raise ValueError(f"LPIPS: {name} must be a float32 CUDA image batch (n, 3, H, W) with H, W >= 16, got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} "
                                 f"{getattr(t, 'dtype', '')} {getattr(t, 'device', '')}")
        if input.shape != target.shape:
            raise ValueError(f"LPIPS: input {tuple(input.shape)} against target {tuple(target.shape)}")

    @torch.no_grad()
    def _forward(self, input, target, keeps):
        """-> (val (n,), saved).  keeps[br]: branch br will be differentiated (its inner post-ReLU maps are kept)."""
        P = self._packed
        xs = (input.detach().contiguous(), target.detach().contiguous())
        ws = _scratch(xs[0].device)
        H, W_ = xs[0].shape[2:]
        taps, inner, cur, dims = ([], []), ([], []), [None, None], []
        res = None
        for k, recs in enumerate(P["slices"]):
            dims.append((H >> k, W_ >> k))
            for br in (0, 1):
                kept = []
                if k == 0:
                    a = T.lpips_conv_in(xs[br], P["w0"], P["b0"], P["shift"], P["scale"])
                    kept.append(a)
                else:
                    a = cur[br]
                for j, r in enumerate(recs):
                    a = ops.conv3x3(a, r["wp"], bias=r["b"], compute=L.COMPUTE_F32, splitk_ws=ws)
                    if j < len(recs) - 1:
                        kept.append(T.relu(a, out=a))
                if k < 4:
                    cur[br], a = T.relu_maxpool2(a, relu_out=a)
                else:
                    T.relu(a, out=a)
                taps[br].append(a)
                inner[br].append(kept if keeps[br] else None)
            res = T.lpips_layer(taps[0][k], taps[1][k], P["lin"][k], res=res, accumulate=k > 0)
            if not any(keeps):
                taps[0][k] = taps[1][k] = None
        # P travels with the tape: the backward differentiates with the packed weights this forward used, whatever is loaded since
        return res, dict(taps=taps, inner=inner, dims=dims, P=P) if any(keeps) else None

    @torch.no_grad()
    def _backward(self, saved, br, g):
        """The image gradient of sum_b g[b] val[b] with respect to branch br (0: input, 1: target): (n, 3, H, W) NCHW."""
        P = saved["P"]
        fa, fb, inner, dims = saved["taps"][br], saved["taps"][1 - br], saved["inner"][br], saved["dims"]
        ws = _scratch(g.device)
        d = None
        for k in (4, 3, 2, 1, 0):
            recs, kept = P["slices"][k], inner[k]
            if k == 4:
                d = T.lpips_layer_bwd(fa[k], fb[k], P["lin"][k], g, relu_mask=True)
            else:
                d = T.relu_maxpool2_bwd(fa[k], d)
                T.lpips_layer_bwd(fa[k], fb[k], P["lin"][k], g, df=d, relu_mask=True, accumulate=True)
            for j in range(len(recs) - 1, -1, -1):
                d = T.conv3x3_dgrad(d, recs[j]["wd"], dims[k], compute=L.COMPUTE_F32, splitk_ws=ws)
                if k > 0 and j > 0:
                    T.relu_bwd(kept[j - 1], d, out=d)
        return T.lpips_conv_in_bwd(d, inner[0][0], P["w0"], P["scale"])

    def forward(self, input, target):
        """(n, 3, H, W) x 2 -> (n, 1, 1, 1); differentiable with respect to either image (a torch.autograd.Function)."""
        self._require_weights()
        self._check(input, target)
        self._ensure_packed()
        needs = tuple(bool(torch.is_grad_enabled() and t.requires_grad) for t in (input, target))
        return _LPIPSFunction.apply(input, target, self, needs)

    def value_and_grad(self, input, target, g=None, wrt="target"):
        """Without autograd: -> (val (n,1,1,1), gradient of sum_b g[b] val[b] (g None: ones) with respect to `wrt`): "target",
        "input", or "both" -> (d input, d target).  The same launches as the autograd route, bit for bit."""
        if wrt not in ("target", "input", "both"):
            raise ValueError(f"LPIPS.value_and_grad: wrt={wrt!r}: 'target', 'input' or 'both'")
        self._require_weights()
        self._check(input, target)
        self._ensure_packed()
        n = input.shape[0]
        g = torch.ones(n, device=input.device) if g is None else g.detach().reshape(-1).contiguous().float()
        if g.numel() != n:
            raise ValueError(f"LPIPS.value_and_grad: g has {g.numel()} elements for n={n}")
        needs = (wrt in ("input", "both"), wrt in ("target", "both"))
        val, saved = self._forward(input, target, needs)
        grads = [self._backward(saved, br, g) if needs[br] else None for br in (0, 1)]
        return val.view(n, 1, 1, 1), (tuple(grads) if wrt == "both" else grads[1] if wrt == "target" else grads[0])
