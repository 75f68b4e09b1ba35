"""Patch-wise evaluation, the mode `model.split_input_params = {...}` switches on
  face_reenactment/ldm/models/diffusion/ddpm.py:565-652 (weighting, fold / unfold), :716-753 (decode), :828-859 (encode),
  :904-986 (apply_model)

The reference loops over the L overlapping crops in Python (L network calls + slice / stack / multiply / Fold / divide).  Here
the crops are BATCH ITEMS: `ldmk_patch_unfold` writes all L*B crops into the network's input buffer, one launch program runs
at batch L*B, `ldmk_patch_fold` blends the L*B outputs into the full-size result -- two plain stream launches around the
program, so a sampler step still captures into one hipGraph.

The blend weights depend on the geometry alone: they are computed once per geometry on the CPU with the reference's own
sequence of torch operations (bit for bit its `weighting` / `normalization`) and cached per device.
"""
from collections import namedtuple

import torch

from . import ops

# cond_stage_key values whose conditioning is an image-like tensor that the reference crops along with x (ddpm.py:919-929)
IMAGE_COND_KEYS = ("image", "LR_image", "segmentation", "bbox_img")

Geometry = namedtuple("Geometry", "ks stride ly lx fks fstride fsize weight norm")
_cpu_cache, _dev_cache = {}, {}


def reduce_ks_stride(shape, ks, stride):
    """ddpm.py:722-728: a kernel / stride larger than the input shrinks to it."""
    h, w = int(shape[0]), int(shape[1])
    ks, stride = (int(ks[0]), int(ks[1])), (int(stride[0]), int(stride[1]))
    if ks[0] > h or ks[1] > w:
        ks = (min(ks[0], h), min(ks[1], w))
    if stride[0] > h or stride[1] > w:
        stride = (min(stride[0], h), min(stride[1], w))
    return ks, stride


def delta_border(h, w):
    """ddpm.py:565-584, operation for operation: distance to the nearest border, 0 at the border, 0.5 at the centre."""
    y = torch.arange(0, h).view(h, 1, 1).repeat(1, w, 1)
    x = torch.arange(0, w).view(1, w, 1).repeat(h, 1, 1)
    arr = torch.cat([y, x], dim=-1) / torch.tensor([h - 1, w - 1]).view(1, 1, 2)
    dist_left_up = torch.min(arr, dim=-1, keepdims=True)[0]
    dist_right_down = torch.min(1 - arr, dim=-1, keepdims=True)[0]
    return torch.min(torch.cat([dist_left_up, dist_right_down], dim=-1), dim=-1)[0]


def params_key(params):
    """The entries of split_input_params the blend weights depend on, as a cache key."""
    tie = bool(params.get("tie_braker", False))
    key = (float(params["clip_min_weight"]), float(params["clip_max_weight"]), tie)
    return key + ((float(params["clip_min_tie_weight"]), float(params["clip_max_tie_weight"])) if tie else ())


def geometry(shape, ks, stride, uf=1, df=1, *, params, device=None):
    """Everything the two kernels need for an input of `shape` = (h, w): the (reduced) crop size and stride, the crop counts, and
    the fold side -- sizes multiplied by `uf` (decode) or divided by `df` (encode), weights [fkh][fkw][L], norm [fh][fw].
    ValueError where the reference gives NaN or a shape error instead of a result."""
    h, w = int(shape[0]), int(shape[1])
    uf, df = int(uf), int(df)
    ks, stride = reduce_ks_stride((h, w), ks, stride)
    key = (h, w, ks, stride, uf, df) + params_key(params)
    g = _cpu_cache.get(key)
    if g is None:
        if uf != 1 and df != 1:
            raise NotImplementedError("patch_geometry: uf and df together (ddpm.py:649-650 raises too)")
        if min(ks + stride) < 1 or uf < 1 or df < 1:
            raise ValueError(f"patch_geometry: ks={ks} stride={stride} uf={uf} df={df} must be positive")
        if (uf != 1 or df != 1) and ks[0] != ks[1]:
            raise ValueError(f"patch_geometry: non-square ks={ks} with vqf != 1: the reference scales BOTH sides of the fold "
                             "kernel from ks[0] (get_fold_unfold, ddpm.py:627,640) and fails with a shape error")
        if uf != 1:
            fks, fstride, fsize = (ks[0] * uf, ks[0] * uf), (stride[0] * uf, stride[1] * uf), (h * uf, w * uf)
        elif df != 1:
            fks, fstride, fsize = (ks[0] // df, ks[0] // df), (stride[0] // df, stride[1] // df), (h // df, w // df)
        else:
            fks, fstride, fsize = ks, stride, (h, w)
        if min(fks + fstride) < 1:
            raise ValueError(f"patch_geometry: ks={ks} stride={stride} divided by df={df} leaves an empty fold kernel or stride")
        ly, lx = (h - ks[0]) // stride[0] + 1, (w - ks[1]) // stride[1] + 1
        fly, flx = (fsize[0] - fks[0]) // fstride[0] + 1, (fsize[1] - fks[1]) // fstride[1] + 1
        if ((ly - 1) * stride[0] + ks[0] != h or (lx - 1) * stride[1] + ks[1] != w or (fly, flx) != (ly, lx)
                or (ly - 1) * fstride[0] + fks[0] != fsize[0] or (lx - 1) * fstride[1] + fks[1] != fsize[1]):
            raise ValueError(f"patch_geometry: {ks[0]}x{ks[1]} patches at stride {stride[0]}x{stride[1]} do not cover a {h}x{w} "
                             f"input exactly (fold side: {fks} / {fstride} on {fsize}): the reference leaves the uncovered "
                             "pixels at 0/0 = NaN, or fails in Fold with a shape error")
        if fks[0] == 1 or fks[1] == 1:
            raise ValueError(f"patch_geometry: a fold kernel of {fks[0]}x{fks[1]}: delta_border divides by (size - 1) = 0 "
                             "(ddpm.py:579-580) and every weight is NaN")
        tie = bool(params.get("tie_braker", False))
        if tie and (ly == 1 or lx == 1):
            raise ValueError(f"patch_geometry: tie_braker with {ly}x{lx} patches: delta_border(Ly, Lx) divides by (L - 1) = 0 "
                             "(ddpm.py:593) and every weight is NaN")
        L_ = ly * lx
        # get_weighting, ddpm.py:586-600
        wt = torch.clip(delta_border(fks[0], fks[1]), params["clip_min_weight"], params["clip_max_weight"])
        wt = wt.view(1, fks[0] * fks[1], 1).repeat(1, 1, L_)
        if tie:
            lw = torch.clip(delta_border(ly, lx), params["clip_min_tie_weight"], params["clip_max_tie_weight"])
            wt = wt * lw.view(1, 1, L_)
        wt = wt.to(torch.float32)
        fold = torch.nn.Fold(output_size=fsize, kernel_size=fks, dilation=1, padding=0, stride=fstride)
        norm = fold(wt).view(fsize[0], fsize[1]).contiguous()          # ddpm.py:620: "normalizes the overlap"
        if not bool((norm > 0).all()):
            raise ValueError("patch_geometry: the accumulated weight is not positive everywhere (clip_min_weight <= 0?): the "
                             "reference divides by it")
        g = Geometry(ks, stride, ly, lx, fks, fstride, fsize, wt.view(fks[0], fks[1], L_).contiguous(), norm)
        _cpu_cache[key] = g
    if device is None or torch.device(device).type == "cpu":
        return g
    dkey = key + (str(torch.device(device)),)
    gd = _dev_cache.get(dkey)
    if gd is None:
        gd = g._replace(weight=g.weight.to(device), norm=g.norm.to(device))
        _dev_cache[dkey] = gd
    return gd


def patch_geometry(shape, ks, stride, uf=1, df=1, *, params, device=None):
    """-> (ly, lx, weight [fkh][fkw][ly*lx], norm [fh][fw]) as float32 tensors for an input of `shape` = (h, w); see `geometry`."""
    g = geometry(shape, ks, stride, uf, df, params=params, device=device)
    return g.ly, g.lx, g.weight, g.norm


def first_stage_patched(fn, x, params, uf=1, df=1):
    """decode_first_stage / encode_first_stage with `patch_distributed_vq` (ddpm.py:716-753, :828-859): unfold -> `fn` on all
    L*B crops at once (each crop is quantised on its own, as in the reference) -> fold at the first stage's scale."""
    x = x.contiguous().float()
    n, _, h, w = x.shape
    g = geometry((h, w), params["ks"], params["stride"], uf, df, params=params, device=x.device)
    crops = ops.patch_unfold(x, g.ks[0], g.ks[1], g.stride[0], g.stride[1])
    o = fn(crops).contiguous()
    assert tuple(o.shape[2:]) == g.fks, f"the first stage maps a {g.ks} crop to {tuple(o.shape[2:])}, not {g.fks} (vqf?)"
    return ops.patch_fold(o, g.weight, g.norm, n, g.fstride[0], g.fstride[1])


class PatchedEval:
    """The UNet evaluated patch-wise on `nb` full-size items: owns the full-size `x` / `eps` buffers and the two launches around
    the launch program `pg` (batch L*nb at the crop size).  `apply_model` and both sampling loops share it; it lives on `pg`
    and dies with it.  `loops`: the samplers' per-run state, kept here so that it never meets the state of a plain run."""

    def __init__(self, pg, g, nb, chans):
        self.pg, self.g, self.nb, self.L = pg, g, int(nb), g.ly * g.lx
        xin, out = pg.inputs["x"], pg.outputs["eps"]
        assert xin.is_contiguous() and out.is_contiguous()
        assert tuple(xin.shape) == (self.L * nb, chans) + g.ks, (tuple(xin.shape), self.L, nb, chans, g.ks)
        h, w = g.fsize
        self.x = torch.zeros(nb, chans, h, w, device=xin.device)
        self.eps = torch.zeros(nb, out.shape[1], h, w, device=xin.device)
        self.loops = {}

    def set_cond(self, ctx=None, cat=None, y_emb=None):
        """Conditioning of the nb items, written once per run: context tokens (nb,Lc,D) / label-embedding rows (nb,E) repeated
        for every patch (`cond_list = [cond] * L`, ddpm.py:974); an image-like concat tensor (nb,C,h,w) cropped like x (:919-929)."""
        pg, g = self.pg, self.g
        if ctx is not None:
            pg.inputs["context"].copy_(ctx.reshape(self.nb, -1).repeat(self.L, 1).view_as(pg.inputs["context"]))
        if cat is not None:
            ops.patch_unfold(cat.contiguous().float(), g.ks[0], g.ks[1], g.stride[0], g.stride[1], out=pg.inputs["c_concat"])
        if y_emb is not None:
            pg.inputs["y_emb"].copy_(y_emb.repeat(self.L, 1))
        pg.ctx_program.run()

    def set_t(self, t):
        if "t_f32" in self.pg.inputs:                      # the float-time program: a real-valued time, embedded as it is
            self.pg.inputs["t_f32"].copy_(t.to(torch.float32).repeat(self.L))
        else:
            self.pg.inputs["t"].copy_(t.to(torch.int64).repeat(self.L))

    def run(self):
        """x -> eps: unfold, the program at batch L*nb, fold.  Stream launches only."""
        pg, g = self.pg, self.g
        ops.patch_unfold(self.x, g.ks[0], g.ks[1], g.stride[0], g.stride[1], out=pg.inputs["x"])
        pg.run()
        ops.patch_fold(pg.outputs["eps"], g.weight, g.norm, self.nb, g.stride[0], g.stride[1], out=self.eps)
