"""MI355X-native first stages: drop-ins for the three classes `ldm.models.autoencoder` offers LatentDiffusion.

`VQModelInterface` (autoencoder.py:264-282) as the samplers use it -- `decode` (VQ lookup -> post_quant_conv ->
Decoder, model.py:462-568) and `encode` (Encoder -> quant_conv, model.py:368-459).
`AutoencoderKL` (autoencoder.py:285-342): `encode` -> DiagonalGaussianDistribution over the moments the encoder's
double-width head produces (one kernel, ldmk_conv3x3_moments), `decode` = post_quant_conv -> Decoder.
`IdentityFirstStage` (autoencoder.py:426-443): pixels are the latents.
`VQModel`: the trainable sibling of `VQModelInterface` (training_step, optimisers, EMA; train_first_stage.py).
`AutoencoderKL` carries its training surface itself; what the two trainable classes share is `_Trainable`.

Parameter trees and state-dict keys equal the reference's (`encoder.*`, `decoder.*`, `quant_conv.*`,
`post_quant_conv.*`, and `quantize.embedding.weight` for the VQ model).  Forward passes are launch programs over
libldmk.so kernels (NHWC inside, NCHW at the boundary); no PyTorch fallback.  What the two autoencoders share --
weight packing, the block emitters, the decoder program, the encoder trunk and the program cache -- is `_FirstStage`.
"""
import math
from contextlib import contextmanager

import torch
import torch.nn as nn

from . import lib as L
from . import ops
from .distributions import DiagonalGaussianDistribution
from .engine import NetBuilder, Program
from .unet import _Params, _Slots, _conv_params, _norm_params


def _resnet(cin, cout):
    ch = dict(norm1=_norm_params(cin), conv1=_conv_params(cin, cout, 3), norm2=_norm_params(cout),
              conv2=_conv_params(cout, cout, 3))
    if cin != cout:
        ch["nin_shortcut"] = _conv_params(cin, cout, 1)
    m = _Slots(**ch)
    m.cin, m.cout = cin, cout
    return m


def _attn_block(c):
    m = _Slots(norm=_norm_params(c), q=_conv_params(c, c, 1), k=_conv_params(c, c, 1), v=_conv_params(c, c, 1),
               proj_out=_conv_params(c, c, 1))
    m.c = c
    return m


class _Level(nn.Module):
    pass


class Decoder(nn.Module):
    """Parameter tree of model.py:462-533."""

    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, give_pre_end=False, tanh_out=False,
                 use_linear_attn=False, attn_type="vanilla", **ignorekwargs):
        super().__init__()
        if use_linear_attn or attn_type != "vanilla" or give_pre_end or tanh_out or not resamp_with_conv:
            raise NotImplementedError("Decoder: only the vanilla-attention / conv-resample configuration is built")
        self.ch, self.num_resolutions, self.num_res_blocks = ch, len(ch_mult), num_res_blocks
        self.resolution, self.z_channels, self.out_ch = resolution, z_channels, out_ch
        self.attn_resolutions = list(attn_resolutions)
        self.ch_mult = list(ch_mult)
        block_in = ch * ch_mult[-1]
        curr = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, curr, curr)
        self.conv_in = _conv_params(z_channels, block_in, 3)
        self.mid = _Slots(block_1=_resnet(block_in, block_in), attn_1=_attn_block(block_in),
                          block_2=_resnet(block_in, block_in))
        ups = []
        for lvl in reversed(range(self.num_resolutions)):
            block_out = ch * ch_mult[lvl]
            up = _Level()
            up.block = nn.ModuleList()
            up.attn = nn.ModuleList()
            for _ in range(num_res_blocks + 1):
                up.block.append(_resnet(block_in, block_out))
                block_in = block_out
                if curr in self.attn_resolutions:
                    up.attn.append(_attn_block(block_in))
            if lvl != 0:
                up.upsample = _Slots(conv=_conv_params(block_in, block_in, 3))
                curr *= 2
            ups.insert(0, up)
        self.up = nn.ModuleList(ups)
        self.norm_out = _norm_params(block_in)
        self.conv_out = _conv_params(block_in, out_ch, 3)
        self._final_ch = block_in


class Encoder(nn.Module):
    """Parameter tree of model.py:368-432."""

    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, double_z=True, use_linear_attn=False,
                 attn_type="vanilla", **ignore_kwargs):
        super().__init__()
        if use_linear_attn or attn_type != "vanilla" or not resamp_with_conv:
            raise NotImplementedError("Encoder: only the vanilla-attention / conv-resample configuration is built")
        self.ch, self.num_resolutions, self.num_res_blocks = ch, len(ch_mult), num_res_blocks
        self.resolution, self.in_channels = resolution, in_channels
        self.attn_resolutions = list(attn_resolutions)
        self.conv_in = _conv_params(in_channels, ch, 3)
        curr = resolution
        in_mult = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        block_in = ch
        for lvl in range(self.num_resolutions):
            block_in = ch * in_mult[lvl]
            block_out = ch * ch_mult[lvl]
            down = _Level()
            down.block = nn.ModuleList()
            down.attn = nn.ModuleList()
            for _ in range(num_res_blocks):
                down.block.append(_resnet(block_in, block_out))
                block_in = block_out
                if curr in self.attn_resolutions:
                    down.attn.append(_attn_block(block_in))
            if lvl != self.num_resolutions - 1:
                down.downsample = _Slots(conv=_conv_params(block_in, block_in, 3))
                curr //= 2
            self.down.append(down)
        self.mid = _Slots(block_1=_resnet(block_in, block_in), attn_1=_attn_block(block_in),
                          block_2=_resnet(block_in, block_in))
        self.norm_out = _norm_params(block_in)
        self.z_out = 2 * z_channels if double_z else z_channels
        self.conv_out = _conv_params(block_in, self.z_out, 3)
        self._final_ch = block_in


class VectorQuantizer(nn.Module):
    """taming VectorQuantizer2 as used at sampling time (quantize.py:213-329): nearest-codebook lookup."""

    def __init__(self, n_e, e_dim, beta=0.25, remap=None, unknown_index="random", sane_index_shape=False, legacy=True):
        super().__init__()
        if remap is not None:
            raise NotImplementedError("VectorQuantizer: index remapping is not used by the shipped configs")
        self.n_e, self.e_dim, self.beta = n_e, e_dim, beta
        self.sane_index_shape = sane_index_shape
        self.embedding = _Params(weight=(n_e, e_dim))
        with torch.no_grad():
            self.embedding.weight.uniform_(-1.0 / n_e, 1.0 / n_e)

    @torch.no_grad()
    def forward(self, z, temp=None, rescale_logits=False, return_logits=False):
        """-> (z_q, loss=None, (None, None, indices)); the straight-through estimator is the identity at inference."""
        zq, idx = ops.vq_nearest(z.contiguous(), self.embedding.weight)
        idx = idx.long()
        if self.sane_index_shape:
            idx = idx.reshape(z.shape[0], z.shape[2], z.shape[3])
        return zq, None, (None, None, idx)

    @torch.no_grad()
    def get_codebook_entry(self, indices, shape):
        z_q = self.embedding.weight[indices.reshape(-1)]
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q


class _FirstStage(nn.Module):
    """What VQModelInterface and AutoencoderKL share: recipe-free initialisation, checkpoint loading, kernel-layout
    weight packing, the ResnetBlock / AttnBlock emitters, the decoder program, the encoder trunk up to norm_out, and
    the program cache.  A subclass registers its modules, then calls `_finish_init`."""

    NARROW_KEYS = ()          # 3x3 weights that take the [9][cin][cout] boundary layout whatever their width
    SKIP_INIT = ()            # parameters that keep their own initialisation

    def _finish_init(self, ckpt_path, ignore_keys):
        self._init_weights()
        self._packed, self._pack_sig, self._programs = None, None, {}
        self.policy_batch = None
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    @torch.no_grad()
    def _init_weights(self):
        params = dict(self.named_parameters())
        for name, p in params.items():
            if name in self.SKIP_INIT:
                continue
            if p.dim() >= 2:
                b = 1.0 / math.sqrt(p[0].numel())
                p.uniform_(-b, b)
            elif name.endswith(".bias"):
                w = params.get(name[:-4] + "weight")
                if w is not None and w.dim() >= 2:
                    b = 1.0 / math.sqrt(w[0].numel())
                    p.uniform_(-b, b)
                else:
                    p.zero_()
            else:
                p.fill_(1.0)

    def init_from_ckpt(self, path, ignore_keys=list()):
        sd = torch.load(path, map_location="cpu")["state_dict"]
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                del sd[k]
        missing, unexpected = self.load_state_dict(sd, strict=False)
        print(f"Restored from {path} with {len(missing)} missing and {len(unexpected)} unexpected keys")

    # ------------------------------------------------------------------------------------------
    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    @torch.no_grad()
    def pack_weights(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.LdmkError(f"{type(self).__name__}: parameters must live on a GPU; there is no CPU path")
        sd = {k: v.detach().float().contiguous() for k, v in self.named_parameters()}
        P = {}
        for k, v in sd.items():
            if k.endswith(".weight") and v.dim() == 4:
                if v.shape[2] == 3:
                    # conv_in / conv_out at the latent / image boundary (and the KL encoder's 6- or 8-channel moment head)
                    narrow = v.shape[1] % 32 != 0 or v.shape[0] <= 4 or k in self.NARROW_KEYS
                    P[k] = ops.pack_conv3x3_narrow(v) if narrow else ops.pack_conv3x3(v)
                    if not narrow and v.shape[1] >= NetBuilder.WINO_MIN_CIN and k.endswith(("conv1.weight", "conv2.weight")):
                        P[k + "#wg"] = ops.pack_winograd(v)     # ResnetBlock convs wide enough for the Winograd route
                    if not narrow and v.shape[1] >= NetBuilder.WINO_MIN_CIN and k.endswith("upsample.conv.weight"):
                        P[k + "#up"] = ops.pack_upconv(v)       # Upsample conv as four 2x2-tap phase convolutions
                elif k.startswith(("quant_conv", "post_quant_conv")):
                    P[k] = v.reshape(v.shape[0], v.shape[1]).contiguous()      # narrow NCHW 1x1: [cout][cin]
                else:
                    P[k] = ops.pack_linear(v)
        # bf16x3 images of the GEMM weights (LDMK_COMPUTE_BF16X3): used for the shapes the "bf16x3" section of igemm_plans.json lists
        from .engine import split_enabled
        if split_enabled():
            for k in list(P):
                w = P[k]
                if k.startswith(("quant_conv", "post_quant_conv")) or not k.split("#")[0].endswith(".weight"):
                    continue
                if k.endswith(("#wg", "#up")):
                    P[k + "#s"] = ops.pack_wsplit(w, batch=w.shape[0])
                elif w.dim() == 2 and w.shape[0] % 32 == 0 and w.shape[1] % 4 == 0 and w.shape[1] > 4:
                    P[k + "#s"] = ops.pack_wsplit(w)
        self._sd, self._packed, self._pack_sig, self._programs = sd, P, self._signature(), {}

    def _ensure(self):
        if self._packed is None or self._pack_sig != self._signature():
            self.pack_weights()

    # ---- shared block emitters -----------------------------------------------------------------------
    def _resnet_block(self, nb, prefix, m, x, h, w):
        pg, P, sd, n = nb.pg, self._packed, self._sd, nb.n
        # GroupNorm+SiLU then conv: one elementwise pass + implicit GEMM, or (wide blocks, large batches) the Winograd route
        h1 = nb.gn_conv(x, None, h, w, sd[prefix + "norm1.weight"], sd[prefix + "norm1.bias"], 1e-6, P[prefix + "conv1.weight"],
                        P.get(prefix + "conv1.weight#wg"), sd[prefix + "conv1.bias"], stats=True)
        g2, b2 = sd[prefix + "norm2.weight"], sd[prefix + "norm2.bias"]
        if m.cin != m.cout:
            sk = nb.lin(x.reshape(n * h * w, m.cin), P[prefix + "nin_shortcut.weight"], sd[prefix + "nin_shortcut.bias"],
                        h * w)
            out = nb.gn_conv(h1, None, h, w, g2, b2, 1e-6, P[prefix + "conv2.weight"], P.get(prefix + "conv2.weight#wg"),
                             sd[prefix + "conv2.bias"], residual=sk, out=sk.view(n, h, w, m.cout), stats=True)
        else:
            out = nb.gn_conv(h1, None, h, w, g2, b2, 1e-6, P[prefix + "conv2.weight"], P.get(prefix + "conv2.weight#wg"),
                             sd[prefix + "conv2.bias"], residual=x, stats=True)
        nb.release(h1)
        return out

    def _attn(self, nb, prefix, m, x, h, w):
        """AttnBlock, model.py:178-202: single head over h*w tokens, logits scaled by C^-0.5."""
        pg, P, sd, n = nb.pg, self._packed, self._sd, nb.n
        hw, c = h * w, m.c
        rows = n * hw
        xr = x.reshape(rows, c)
        coef = nb.gn(x, None, hw, sd[prefix + "norm.weight"], sd[prefix + "norm.bias"], 1e-6)
        q = nb.lin(xr, P[prefix + "q.weight"], sd[prefix + "q.bias"], hw, tf=L.TF_AFFINE, tf_coef=coef)
        k = nb.lin(xr, P[prefix + "k.weight"], sd[prefix + "k.bias"], hw, tf=L.TF_AFFINE, tf_coef=coef)
        v = nb.lin(xr, P[prefix + "v.weight"], sd[prefix + "v.bias"], hw, tf=L.TF_AFFINE, tf_coef=coef)
        nb.release(coef)
        s = pg.alloc(n, hw, hw)
        a = ops.make_igemm_args(hw, hw, c, q, c, k, s, hw, hw, b_trans=True, batch=n, a_bstride=hw * c,
                                w_bstride=hw * c, out_bstride=hw * hw)
        pg.igemm(a, nb.pin, per_sample=True)      # one problem per sample, planned as the job's batch of them
        pg.add("ldmk_softmax_rows", s.data_ptr(), n * hw, hw, float(int(c) ** (-0.5)))
        o = pg.alloc(rows, c)
        a = ops.make_igemm_args(hw, c, hw, s, hw, v, o, c, hw, batch=n, a_bstride=hw * hw, w_bstride=hw * c,
                                out_bstride=hw * c)
        pg.igemm(a, nb.pin, per_sample=True)      # one problem per sample, planned as the job's batch of them
        nb.release(s, q, k, v)
        out = nb.lin(o, P[prefix + "proj_out.weight"], sd[prefix + "proj_out.bias"], hw, residual=xr, stats=True)
        nb.release(o)
        return out.view(n, h, w, c)

    # ---- programs -----------------------------------------------------------------------------------------
    def _build_decode(self, n, h, w, quantize):
        d = self.decoder
        P, sd = self._packed, self._sd
        dev = next(self.parameters()).device
        pg = Program(dev)
        zc, ed = d.z_channels, self.embed_dim               # latents carry embed_dim channels, post_quant_conv -> z_channels
        z_in = pg.alloc(n, ed, h, w)
        pg.inputs = dict(z=z_in)
        idx = pg.alloc(n * h * w, dtype=torch.int32) if quantize else None      # (written by ldmk_vq_nearest only: no lookup, no indices)
        zcur = z_in
        if quantize:
            zq = pg.alloc(n, ed, h, w)
            pg.add("ldmk_vq_nearest", z_in.data_ptr(), sd["quantize.embedding.weight"].data_ptr(), zq.data_ptr(),
                   idx.data_ptr(), n, h * w, self.embed_dim, self.n_embed)
            zcur = zq
        pq = pg.alloc(n, zc, h, w)
        pg.add("ldmk_conv1x1_nchw", zcur.data_ptr(), P["post_quant_conv.weight"].data_ptr(),
               sd["post_quant_conv.bias"].data_ptr(), pq.data_ptr(), n, h * w, self.embed_dim, zc)
        top = d.ch * d.ch_mult[-1]
        hw_max = h * w * 4 ** (d.num_resolutions - 1)
        pin = None if self.policy_batch in (None, n) else (self.policy_batch, n)
        nb = NetBuilder(pg, n, pin)
        x = pg.alloc(n, h, w, top)
        pg.add("ldmk_conv3x3_in", pq.data_ptr(), zc, 0, 0, P["decoder.conv_in.weight"].data_ptr(),
               sd["decoder.conv_in.bias"].data_ptr(), x.data_ptr(), n, h, w, top)

        def step(fn, *a):
            nonlocal x
            y = fn(nb, *a[:2], x, *a[2:])
            nb.release(x)
            x = y

        step(self._resnet_block, "decoder.mid.block_1.", d.mid.block_1, h, w)
        step(self._attn, "decoder.mid.attn_1.", d.mid.attn_1, h, w)
        step(self._resnet_block, "decoder.mid.block_2.", d.mid.block_2, h, w)
        ch_, cw_ = h, w
        for lvl in reversed(range(d.num_resolutions)):
            up = d.up[lvl]
            for ib in range(d.num_res_blocks + 1):
                step(self._resnet_block, f"decoder.up.{lvl}.block.{ib}.", up.block[ib], ch_, cw_)
                if len(up.attn) > 0:
                    step(self._attn, f"decoder.up.{lvl}.attn.{ib}.", up.attn[ib], ch_, cw_)
            if lvl != 0:
                kw_ = f"decoder.up.{lvl}.upsample.conv.weight"
                y = nb.up_conv(x, ch_, cw_, P[kw_], P.get(kw_ + "#up"), sd[f"decoder.up.{lvl}.upsample.conv.bias"], stats=True)
                nb.release(x)
                x = y
                ch_, cw_ = 2 * ch_, 2 * cw_
        coef = nb.gn(x, None, ch_ * cw_, sd["decoder.norm_out.weight"], sd["decoder.norm_out.bias"], 1e-6)
        img = pg.alloc(n, d.out_ch, ch_, cw_)
        pg.add("ldmk_conv3x3_out", x.data_ptr(), coef.data_ptr(), P["decoder.conv_out.weight"].data_ptr(),
               sd["decoder.conv_out.bias"].data_ptr(), img.data_ptr(), n, ch_, cw_, d._final_ch, d.out_ch)
        pg.outputs = dict(image=img) if idx is None else dict(image=img, indices=idx)
        return pg

    def _encode_trunk(self, n, H, W_):
        """Encoder up to norm_out (model.py:434-456): -> (program, builder, NHWC features, GroupNorm coefficient planes,
        h, w).  The subclass appends its head and names the outputs."""
        e = self.encoder
        P, sd = self._packed, self._sd
        dev = next(self.parameters()).device
        pg = Program(dev)
        x_in = pg.alloc(n, e.in_channels, H, W_)
        pg.inputs = dict(x=x_in)
        pin = None if self.policy_batch in (None, n) else (self.policy_batch, n)
        nb = NetBuilder(pg, n, pin)
        x = pg.alloc(n, H, W_, e.ch)
        pg.add("ldmk_conv3x3_in", x_in.data_ptr(), e.in_channels, 0, 0, P["encoder.conv_in.weight"].data_ptr(),
               sd["encoder.conv_in.bias"].data_ptr(), x.data_ptr(), n, H, W_, e.ch)

        def step(fn, *a):
            nonlocal x
            y = fn(nb, *a[:2], x, *a[2:])
            nb.release(x)
            x = y

        ch_, cw_ = H, W_
        for lvl in range(e.num_resolutions):
            dn = e.down[lvl]
            for ib in range(e.num_res_blocks):
                step(self._resnet_block, f"encoder.down.{lvl}.block.{ib}.", dn.block[ib], ch_, cw_)
                if len(dn.attn) > 0:
                    step(self._attn, f"encoder.down.{lvl}.attn.{ib}.", dn.attn[ib], ch_, cw_)
            if lvl != e.num_resolutions - 1:
                y = nb.conv(x, None, P[f"encoder.down.{lvl}.downsample.conv.weight"],
                            sd[f"encoder.down.{lvl}.downsample.conv.bias"], ch_, cw_, stride=2, pad_lo=0, stats=True)
                nb.release(x)
                x = y
                ch_, cw_ = (ch_ + 1 - 3) // 2 + 1, (cw_ + 1 - 3) // 2 + 1
        step(self._resnet_block, "encoder.mid.block_1.", e.mid.block_1, ch_, cw_)
        step(self._attn, "encoder.mid.attn_1.", e.mid.attn_1, ch_, cw_)
        step(self._resnet_block, "encoder.mid.block_2.", e.mid.block_2, ch_, cw_)
        coef = nb.gn(x, None, ch_ * cw_, sd["encoder.norm_out.weight"], sd["encoder.norm_out.bias"], 1e-6)
        return pg, nb, x, coef, ch_, cw_

    def _program(self, kind, *key):
        self._ensure()
        k = (kind,) + key + (self.policy_batch,)
        pg = self._programs.get(k)
        if pg is None:
            pg = self._build_decode(*key) if kind == "dec" else self._build_encode(*key)
            self._programs[k] = pg
        return pg


class _VQFirstStage(_FirstStage):
    """What VQModelInterface and VQModel share: the module tree, the encode program and the two program runners."""
    SKIP_INIT = ("quantize.embedding.weight",)

    def __init__(self, embed_dim, ddconfig=None, lossconfig=None, n_embed=None, ckpt_path=None, ignore_keys=[],
                 image_key="image", colorize_nlabels=None, monitor=None, batch_resize_range=None,
                 scheduler_config=None, lr_g_factor=1.0, remap=None, sane_index_shape=False, use_ema=False, **kw):
        super().__init__()
        ddconfig = dict(ddconfig)
        self.embed_dim, self.n_embed, self.image_key = embed_dim, n_embed, image_key
        self.ddconfig = ddconfig
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.quantize = VectorQuantizer(n_embed, embed_dim, beta=0.25, remap=remap, sane_index_shape=sane_index_shape)
        self.quant_conv = _conv_params(ddconfig["z_channels"], embed_dim, 1)
        self.post_quant_conv = _conv_params(embed_dim, ddconfig["z_channels"], 1)
        if monitor is not None:
            self.monitor = monitor
        self._finish_init(ckpt_path, ignore_keys)

    def _build_encode(self, n, H, W_):
        e, P, sd = self.encoder, self._packed, self._sd
        pg, nb, x, coef, ch_, cw_ = self._encode_trunk(n, H, W_)
        hz = pg.alloc(n, e.z_out, ch_, cw_)
        pg.add("ldmk_conv3x3_out", x.data_ptr(), coef.data_ptr(), P["encoder.conv_out.weight"].data_ptr(),
               sd["encoder.conv_out.bias"].data_ptr(), hz.data_ptr(), n, ch_, cw_, e._final_ch, e.z_out)
        z = pg.alloc(n, self.embed_dim, ch_, cw_)
        pg.add("ldmk_conv1x1_nchw", hz.data_ptr(), P["quant_conv.weight"].data_ptr(), sd["quant_conv.bias"].data_ptr(),
               z.data_ptr(), n, ch_ * cw_, e.z_out, self.embed_dim)
        pg.outputs = dict(z=z)
        return pg

    @torch.no_grad()
    def _run_encode(self, x):
        """Encoder -> quant_conv: the latent before quantisation."""
        if not x.is_cuda:
            raise L.LdmkError(f"{type(self).__name__}.encode: CUDA tensors only (no CPU fallback)")
        n, _, H, W_ = x.shape
        pg = self._program("enc", n, H, W_)
        pg.inputs["x"].copy_(x)
        pg.run()
        return pg.outputs["z"].clone()

    @torch.no_grad()
    def _run_decode(self, h, quantize, return_indices=False):
        """(VQ lookup ->) post_quant_conv -> Decoder."""
        if not h.is_cuda:
            raise L.LdmkError(f"{type(self).__name__}.decode: CUDA tensors only (no CPU fallback)")
        n, _, hh, ww = h.shape
        if return_indices and not quantize:
            raise L.LdmkError(f"{type(self).__name__}.decode: return_indices needs the codebook lookup (force_not_quantize skips it)")
        pg = self._program("dec", n, hh, ww, quantize)
        pg.inputs["z"].copy_(h)
        pg.run()
        img = pg.outputs["image"].clone()
        return (img, pg.outputs["indices"].clone()) if return_indices else img


class VQModelInterface(_VQFirstStage):
    # ---- public surface (autoencoder.py:269-282) ------------------------------------------------------------
    def encode(self, x):
        return self._run_encode(x)

    def decode(self, h, force_not_quantize=False, return_indices=False):
        return self._run_decode(h, not force_not_quantize, return_indices)

    def forward(self, x):
        return self.decode(self.encode(x))


class _AdamOfTrainer:
    """What configure_optimizers hands out for the autoencoder: the step is ldmk_adamw over the trainer's arena."""

    def __init__(self, model, lr, betas=(0.5, 0.9)):
        self.model, self.betas = model, betas
        self.param_groups = [dict(lr=lr, betas=betas)]

    def step(self):
        self.model.trainer().adam_step(self.param_groups[0]["lr"], betas=self.betas)
        self.model._dirty = True

    def zero_grad(self, set_to_none=False):
        self.model.trainer().P.grad.zero_()


class _Trainable:
    """What the trainable first stages (VQModel, AutoencoderKL) share, mixed in ahead of their `_FirstStage` base: the loss
    module kept out of the module tree but carried in the state dict under `loss.`, the lazily built
    `train_first_stage.FirstStageTrainer` whose arena runs ahead of the nn.Parameters (`_dirty`) and is written back by
    `_ensure` before any inference method, state-dict read or EMA scope, the logging stand-ins for Lightning's, the two
    optimizers, and `train_batch`, the loop body Lightning would run.  A subclass supplies `training_step`."""

    def _init_training(self, lossconfig, lr_g_factor=1.0, use_ema=False):
        from .util import instantiate_from_config
        loss = lossconfig if isinstance(lossconfig, nn.Module) or lossconfig is None else instantiate_from_config(lossconfig)
        object.__setattr__(self, "_loss", loss)            # kept out of the module tree (the first-stage machinery walks parameters())
        self.lr_g_factor, self.use_ema = lr_g_factor, use_ema
        self.learning_rate, self.global_step = 4.5e-6, 0
        self.logged = {}
        self._tr, self._dirty, self._shadow, self._ema_updates, self._opts = None, False, None, 0, None

    @property
    def loss(self):
        return self._loss

    def _apply(self, fn, *a, **kw):
        if isinstance(self._loss, nn.Module):
            self._loss._apply(fn)
        return super()._apply(fn, *a, **kw)

    def trainer(self):
        if self._tr is None:
            from .train_first_stage import FirstStageTrainer
            self._tr = FirstStageTrainer(self)
            if self.use_ema:
                self._shadow = self._tr.P.flat.clone()
        return self._tr

    def _ensure(self):
        if self._dirty:                          # the arena is ahead of the nn.Parameters
            self._dirty = False
            self._tr.sync_to_module()
        super()._ensure()

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """nn.Module.state_dict with the loss module's entries under `<prefix>loss.`, top level or nested in a parent."""
        if args:                                 # the legacy positional form (destination, prefix, keep_vars)
            destination, prefix, keep_vars = (list(args) + [prefix, keep_vars][len(args) - 1:])[:3]
        if self._dirty:
            self._ensure()
        sd = super().state_dict(destination=destination, prefix=prefix, keep_vars=keep_vars)
        if isinstance(self._loss, nn.Module):
            self._loss.state_dict(destination=sd, prefix=prefix + "loss.", keep_vars=keep_vars)
        return sd

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """The hook both `load_state_dict` and a parent module's load go through: the `<prefix>loss.` entries go to the loss
        module (which is no registered child), and the arena restarts from the loaded weights."""
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        lp = prefix + "loss."
        unexpected_keys[:] = [k for k in unexpected_keys if not k.startswith(lp)]
        mine = {k[len(lp):]: v for k, v in state_dict.items() if k.startswith(lp)}
        if isinstance(self._loss, nn.Module) and (mine or strict):
            res = self._loss.load_state_dict(mine, strict=False)
            missing_keys.extend(lp + k for k in res.missing_keys)
            unexpected_keys.extend(lp + k for k in res.unexpected_keys)
        self._tr, self._dirty, self._shadow, self._opts = None, False, None, None

    def log_dict(self, d, **kw):
        self.logged.update({k: (v.detach() if torch.is_tensor(v) else v) for k, v in d.items()})

    def log(self, k, v, **kw):
        self.log_dict({k: v})

    def get_input(self, batch, k):
        x = batch[k]
        if len(x.shape) == 3:
            x = x[..., None]
        return x.permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format).float()

    def get_last_layer(self):
        return self.decoder.conv_out.weight

    def configure_optimizers(self):
        lr_d, lr_g = self.learning_rate, self.lr_g_factor * self.learning_rate
        self._opts = [_AdamOfTrainer(self, lr_g), torch.optim.Adam(self.loss.discriminator.parameters(), lr=lr_d, betas=(0.5, 0.9))]
        return self._opts, []

    def train_batch(self, batch, batch_idx=0):
        """One iteration of the two-optimizer loop: -> (aeloss, discloss)."""
        opt_ae, opt_disc = self._opts if self._opts is not None else self.configure_optimizers()[0]
        aeloss = self.training_step(batch, batch_idx, 0)
        opt_ae.step()
        opt_disc.zero_grad(set_to_none=True)
        with torch.enable_grad():
            discloss = self.training_step(batch, batch_idx, 1)
            discloss.backward()
        opt_disc.step()
        self.on_train_batch_end()
        self.global_step += 1
        return aeloss, discloss.detach()

    def on_train_batch_end(self, *args, **kwargs):
        if self.use_ema:                           # LitEma.forward, ema.py:25-44: decay warms up with the update count
            self._ema_updates += 1
            decay = min(0.9999, (1 + self._ema_updates) / (10 + self._ema_updates))
            self.trainer().ema_update(self._shadow, decay)

    @contextmanager
    def ema_scope(self, context=None):
        if self.use_ema:
            self.trainer().sync_to_module(self._shadow)
            self._dirty = False
        try:
            yield None
        finally:
            if self.use_ema:
                self._tr.sync_to_module()


class VQModel(_Trainable, _VQFirstStage):
    """ldm.models.autoencoder.VQModel (autoencoder.py:14-262) and taming.models.vqgan.VQModel as a trainable drop-in, without
    Lightning: `training_step(batch, batch_idx, optimizer_idx)` runs the whole autoencoder step on the HIP kernels
    (train_first_stage.FirstStageTrainer) and returns the loss; `configure_optimizers()` hands out the two optimizers, and
    `train_batch(batch)` is the loop body Lightning would run (autoencoder step, discriminator step, EMA).  The trained
    weights live in the trainer's arena and are written back into the nn.Parameters whenever an inference method, the state
    dict or the EMA scope needs them.  The loss module is not a registered submodule (the first-stage machinery walks
    `parameters()`); `state_dict()` / `load_state_dict()` carry it under the reference's `loss.` prefix all the same.
    With use_ema the shadow is a flat copy of the arena (not part of the state dict)."""

    def __init__(self, ddconfig, lossconfig, n_embed, embed_dim, ckpt_path=None, ignore_keys=[], image_key="image",
                 colorize_nlabels=None, monitor=None, batch_resize_range=None, scheduler_config=None, lr_g_factor=1.0,
                 remap=None, sane_index_shape=False, use_ema=False):
        for name, v in (("batch_resize_range", batch_resize_range), ("remap", remap), ("colorize_nlabels", colorize_nlabels),
                        ("scheduler_config", scheduler_config)):
            if v is not None:
                raise NotImplementedError(f"VQModel: {name} is not built")
        super().__init__(embed_dim, ddconfig=ddconfig, n_embed=n_embed, image_key=image_key, monitor=monitor,
                         sane_index_shape=sane_index_shape)
        self._init_training(lossconfig, lr_g_factor, use_ema)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    # ---- the reference's surface -----------------------------------------------------------------------------------
    def encode(self, x):
        from . import train_ops as T
        h = self._run_encode(x)
        quant, idx = ops.vq_nearest(h, self.quantize.embedding.weight.detach())
        emb_loss, _ = T.vq_loss_bwd(h, self.quantize.embedding.weight.detach(), idx.reshape(-1), beta=self.quantize.beta,
                                    want_dz=False)
        ind = idx.long().reshape(x.shape[0], h.shape[2], h.shape[3]) if self.quantize.sane_index_shape else idx.long().reshape(-1)
        return quant, emb_loss, (None, None, ind)

    def encode_to_prequant(self, x):
        return self._run_encode(x)

    def decode(self, quant):
        return self._run_decode(quant, False)

    def decode_code(self, code_b):
        b, h, w = code_b.shape
        return self.decode(self.quantize.get_codebook_entry(code_b, (b, h, w, self.embed_dim)))

    def forward(self, input, return_pred_indices=False):
        quant, diff, (_, _, ind) = self.encode(input)
        dec = self.decode(quant)
        return (dec, diff, ind) if return_pred_indices else (dec, diff)

    def training_step(self, batch, batch_idx, optimizer_idx):
        """optimizer_idx 0: forward, loss, ONE backward through the autoencoder (gradients in trainer().P.grad), -> aeloss.
        optimizer_idx 1: forward again (the autoencoder may have stepped, as under Lightning), -> the discriminator loss with
        autograd attached to the discriminator."""
        from .losses import perplexity_from_counts
        x = self.get_input(batch, self.image_key).to(next(self.parameters()).device)
        tr, loss = self.trainer(), self.loss
        loss.discriminator.train()
        xrec = tr.forward(x)
        if optimizer_idx == 0:
            aeloss, log = loss(tr.qloss, x, xrec, 0, self.global_step, last_layer=tr.last_layer_grad, split="train")
            tr.backward(loss.d_image, codebook_weight=loss.codebook_weight)
            log["train/perplexity"], log["train/cluster_usage"] = perplexity_from_counts(tr.counts)
            self.log_dict(log)
            return aeloss
        tr.tape = []
        discloss, log = loss(tr.qloss, x, xrec, 1, self.global_step, split="train")
        self.log_dict(log)
        return discloss

    @torch.no_grad()
    def _validation_step(self, batch, batch_idx, suffix=""):
        x = self.get_input(batch, self.image_key).to(next(self.parameters()).device)
        xrec, qloss, ind = self(x, return_pred_indices=True)
        self.loss.discriminator.eval()
        aeloss, log_ae = self.loss(qloss, x, xrec, 0, self.global_step, last_layer=None, split="val" + suffix, predicted_indices=ind)
        _, log_disc = self.loss(qloss, x, xrec, 1, self.global_step, split="val" + suffix)
        log_ae[f"val{suffix}/aeloss"] = aeloss
        self.log_dict(log_ae)
        self.log_dict(log_disc)
        return dict(log_ae, **log_disc)

    def validation_step(self, batch, batch_idx):
        log = self._validation_step(batch, batch_idx)
        if self.use_ema:
            with self.ema_scope():
                log.update(self._validation_step(batch, batch_idx, suffix="_ema"))
        return log

    @torch.no_grad()
    def log_images(self, batch, only_inputs=False, plot_ema=False, **kwargs):
        x = self.get_input(batch, self.image_key).to(next(self.parameters()).device)
        log = dict(inputs=x)
        if only_inputs:
            return log
        log["reconstructions"] = self(x)[0]
        if plot_ema:
            with self.ema_scope():
                log["reconstructions_ema"] = self(x)[0]
        return log


class AutoencoderKL(_Trainable, _FirstStage):
    """autoencoder.py:285-423.  The encoder ends in a 3x3 convolution to 2*z_channels moment channels and a 1x1 `quant_conv`
    to 2*embed_dim: at inference both run in one kernel (ldmk_conv3x3_moments), which is built for up to 8 channels on either
    side -- z_channels, embed_dim <= 4, i.e. the KL-f4 and KL-f8 autoencoders.
    Training, without Lightning as for VQModel: under a `losses.LPIPSWithDiscriminator` lossconfig,
    `training_step(batch, batch_idx, optimizer_idx)` runs the autoencoder step on the HIP kernels
    (train_first_stage.FirstStageTrainer, KL bottleneck) and `train_batch(batch)` is the two-optimizer loop body.  Each
    `training_step` call draws the posterior once, from `sample_noise`.  With `lossconfig = torch.nn.Identity` (every
    LatentDiffusion config) nothing of that is built and `training_step` raises.  `use_ema` is this project's addition (the
    reference's AutoencoderKL has none): a flat shadow of the arena, as VQModel's."""

    NARROW_KEYS = ("encoder.conv_out.weight",)
    MAX_Z = 4

    def __init__(self, ddconfig, lossconfig, embed_dim, ckpt_path=None, ignore_keys=[], image_key="image",
                 colorize_nlabels=None, monitor=None, use_ema=False):
        super().__init__()
        ddconfig = dict(ddconfig)
        assert ddconfig["double_z"]
        zc = ddconfig["z_channels"]
        if zc > self.MAX_Z or embed_dim > self.MAX_Z:
            raise NotImplementedError(f"AutoencoderKL: z_channels={zc}, embed_dim={embed_dim}: the moment head "
                                      f"(ldmk_conv3x3_moments) is built for z_channels <= {self.MAX_Z} and embed_dim <= "
                                      f"{self.MAX_Z} (KL-f4 / KL-f8); wider heads (KL-f16 / KL-f32) are not built")
        self.embed_dim, self.image_key, self.ddconfig = embed_dim, image_key, ddconfig
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.quant_conv = _conv_params(2 * zc, 2 * embed_dim, 1)
        self.post_quant_conv = _conv_params(embed_dim, zc, 1)
        if colorize_nlabels is not None:
            assert type(colorize_nlabels) == int
            self.register_buffer("colorize", torch.randn(3, colorize_nlabels, 1, 1))
        if monitor is not None:
            self.monitor = monitor
        self._finish_init(None, ignore_keys)
        self._init_training(lossconfig, use_ema=use_ema)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    def _build_encode(self, n, H, W_):
        e, P, sd = self.encoder, self._packed, self._sd
        pg, nb, x, coef, ch_, cw_ = self._encode_trunk(n, H, W_)
        moments = pg.alloc(n, 2 * self.embed_dim, ch_, cw_)
        pg.add("ldmk_conv3x3_moments", x.data_ptr(), coef.data_ptr(), P["encoder.conv_out.weight"].data_ptr(),
               sd["encoder.conv_out.bias"].data_ptr(), P["quant_conv.weight"].data_ptr(), sd["quant_conv.bias"].data_ptr(),
               moments.data_ptr(), n, ch_, cw_, e._final_ch, e.z_out, 2 * self.embed_dim)
        pg.outputs = dict(moments=moments)
        return pg

    # ---- public surface (autoencoder.py:324-342) ------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x):
        if not x.is_cuda:
            raise L.LdmkError("AutoencoderKL.encode: CUDA tensors only (no CPU fallback)")
        n, _, H, W_ = x.shape
        pg = self._program("enc", n, H, W_)
        pg.inputs["x"].copy_(x)
        pg.run()
        return DiagonalGaussianDistribution(pg.outputs["moments"].clone())

    @torch.no_grad()
    def decode(self, z):
        if not z.is_cuda:
            raise L.LdmkError("AutoencoderKL.decode: CUDA tensors only (no CPU fallback)")
        n, _, hh, ww = z.shape
        pg = self._program("dec", n, hh, ww, False)
        pg.inputs["z"].copy_(z)
        pg.run()
        return pg.outputs["image"].clone()

    def sample_noise(self, shape):
        """The one source of every normal draw of this class (posterior samples of `forward` and of the training forward, the
        latents of `log_images`); tests and fixtures override it."""
        return torch.randn(tuple(shape), device=next(self.parameters()).device, dtype=torch.float32)

    def forward(self, input, sample_posterior=True):
        posterior = self.encode(input)
        z = posterior.sample(noise=self.sample_noise(posterior.mean.shape)) if sample_posterior else posterior.mode()
        return self.decode(z), posterior

    # ---- the training surface (autoencoder.py:344-415) --------------------------------------------------------------
    def _training_loss(self):
        loss = self.loss
        if not (isinstance(loss, nn.Module) and hasattr(loss, "discriminator") and hasattr(loss, "kl_weight")):
            raise L.LdmkError(f"AutoencoderKL.training_step: lossconfig gave {type(loss).__name__}, which is no training loss; "
                              "construct the model with ldm.modules.losses.LPIPSWithDiscriminator to train it")
        return loss

    def training_step(self, batch, batch_idx, optimizer_idx):
        """optimizer_idx 0: forward (one posterior draw), loss, ONE backward through the autoencoder (gradients in
        trainer().P.grad), -> aeloss.  optimizer_idx 1: forward again with a draw of its own (the autoencoder may have stepped,
        as under Lightning), -> the discriminator loss with autograd attached to the discriminator."""
        loss = self._training_loss()
        x = self.get_input(batch, self.image_key).to(next(self.parameters()).device)
        tr = self.trainer()
        loss.discriminator.train()
        xrec = tr.forward(x)
        if optimizer_idx == 0:
            aeloss, log = loss(x, xrec, tr.kl, 0, self.global_step, last_layer=tr.last_layer_grad, split="train")
            tr.backward(loss.d_image, kl_weight=loss.kl_weight)
            self.log("aeloss", aeloss)
            self.log_dict(log)
            return aeloss
        tr.tape = []
        discloss, log = loss(x, xrec, tr.kl, 1, self.global_step, split="train")
        self.log("discloss", discloss)
        self.log_dict(log)
        return discloss

    @torch.no_grad()
    def validation_step(self, batch, batch_idx):
        loss = self._training_loss()
        x = self.get_input(batch, self.image_key).to(next(self.parameters()).device)
        xrec, posterior = self(x)
        loss.discriminator.eval()
        _, log_ae = loss(x, xrec, posterior, 0, self.global_step, last_layer=None, split="val")
        _, log_disc = loss(x, xrec, posterior, 1, self.global_step, split="val")
        self.log_dict(log_ae)
        self.log_dict(log_disc)
        return dict(log_ae, **log_disc)

    @torch.no_grad()
    def log_images(self, batch, only_inputs=False, **kwargs):
        x = self.get_input(batch, self.image_key).to(next(self.parameters()).device)
        if x.shape[1] > 3:
            raise NotImplementedError("AutoencoderKL.log_images: the random colorize projection of segmentation inputs is not built")
        log = dict(inputs=x)
        if not only_inputs:
            xrec, posterior = self(x)
            log["samples"] = self.decode(self.sample_noise(posterior.mean.shape))
            log["reconstructions"] = xrec
        return log


class IdentityFirstStage(nn.Module):
    """autoencoder.py:426-443: pixel-space diffusion, the first stage passes everything through.  No parameters, no launches."""

    def __init__(self, *args, vq_interface=False, **kwargs):
        super().__init__()
        self.vq_interface = vq_interface

    def encode(self, x, *args, **kwargs):
        return x

    def decode(self, x, *args, **kwargs):
        return x

    def quantize(self, x, *args, **kwargs):
        return (x, None, [None, None, None]) if self.vq_interface else x

    def forward(self, x, *args, **kwargs):
        return x
