"""EncoderUNetModel: the half UNet with a pooled classification head (openaimodel.py:745-961), the network
`NoisyLatentImageClassifier` trains (classifier.py).

Same constructor kwargs (extra ones are swallowed: `load_classifier` hands over a deep copy of the diffusion UNet's params,
`use_spatial_transformer`, `context_dim`, ... included; the encoder always uses `AttentionBlock`), same parameter tree and
state-dict keys.  The torso is described with UNetModel's block descriptors, so the trainer's ResBlock / AttentionBlock /
Downsample code runs on it unchanged (train.EncoderUNetTrainer).  There is no compiled launch program for this network:
`forward` runs the trainer's forward and drops the tape, the way `forward_only` does for the diffusion objective.
"""
import math

import torch
import torch.nn as nn

from . import lib as L
from . import ops
from .unet import _Params, _Slots, _attention_block, _conv_params, _lin_params, _norm_params, _res_block, _seq, pack_attention_block

POOLS = ("adaptive", "attention", "spatial", "spatial_v2")
SPATIAL_HIDDEN = 2048


class EncoderUNetModel(nn.Module):
    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, use_checkpoint=False, use_fp16=False, num_heads=1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, pool="adaptive", *args, **kwargs):
        super().__init__()
        if dims != 2:
            raise NotImplementedError("EncoderUNetModel: only dims=2")
        if not conv_resample:
            raise NotImplementedError("EncoderUNetModel: conv_resample=False")
        if use_fp16:
            raise NotImplementedError("EncoderUNetModel: fp32 only (reference precision)")
        if pool not in POOLS:
            raise NotImplementedError(f"Unexpected {pool} pooling")                    # openaimodel.py:922
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        attention_resolutions = list(attention_resolutions)
        channel_mult = list(channel_mult)
        self.image_size, self.in_channels, self.model_channels = image_size, in_channels, model_channels
        self.out_channels, self.num_res_blocks = out_channels, num_res_blocks
        self.attention_resolutions, self.channel_mult = attention_resolutions, channel_mult
        self.dropout, self.conv_resample, self.use_checkpoint, self.dtype = dropout, conv_resample, use_checkpoint, torch.float32
        self.num_heads, self.num_head_channels, self.num_heads_upsample = num_heads, num_head_channels, num_heads_upsample
        self.use_scale_shift_norm, self.use_new_attention_order = bool(use_scale_shift_norm), bool(use_new_attention_order)
        self.resblock_updown = bool(resblock_updown)
        # what the trainer's torso code asks a UNetModel for
        self.num_classes, self.use_spatial_transformer, self.context_dim = None, False, None
        mc = model_channels
        emb_ch = 4 * mc
        self.time_embed = _Slots(_0=_lin_params(mc, emb_ch), _2=_lin_params(emb_ch, emb_ch))

        def attn(ch):
            n = num_heads if num_head_channels == -1 else ch // num_head_channels     # AttentionBlock, openaimodel.py:296-303
            if n * (ch // n) != ch or (ch // n) % 4:
                raise NotImplementedError(f"EncoderUNetModel: {ch} channels do not split into {n} heads of a width that is a multiple of 4")
            return _attention_block(ch, n, use_new_attention_order)

        # ---- same walk as openaimodel.py:801-889
        first = _conv_params(in_channels, mc, 3)
        first.kind = "conv_in"
        self.input_blocks = nn.ModuleList([_seq(first)])
        self._feature_size = mc
        self.feature_widths = [mc]            # channels of every input block's output, then the middle block's: the spatial pools' columns
        ch, ds = mc, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [_res_block(ch, mult * mc, emb_ch, use_scale_shift_norm)]
                ch = mult * mc
                if ds in attention_resolutions:
                    layers.append(attn(ch))
                self.input_blocks.append(_seq(*layers))
                self._feature_size += ch
                self.feature_widths.append(ch)
            if level != len(channel_mult) - 1:
                if resblock_updown:
                    down = _res_block(ch, ch, emb_ch, use_scale_shift_norm, updown="down")
                else:
                    down = _Slots(op=_conv_params(ch, ch, 3))
                    down.kind, down.ch = "down", ch
                self.input_blocks.append(_seq(down))
                ds *= 2
                self._feature_size += ch
                self.feature_widths.append(ch)
        self.middle_block = _seq(_res_block(ch, ch, emb_ch, use_scale_shift_norm), attn(ch), _res_block(ch, ch, emb_ch, use_scale_shift_norm))
        self._feature_size += ch
        self.feature_widths.append(ch)
        self.pool = pool
        self._final_ch, self._final_ds = ch, ds
        K = out_channels
        if pool == "adaptive":
            self.out = _Slots(_0=_norm_params(ch), _3=_conv_params(ch, K, 1))
        elif pool == "attention":
            assert num_head_channels != -1                                            # openaimodel.py:900
            if ch % num_head_channels or num_head_channels % 4:
                raise NotImplementedError(f"EncoderUNetModel: AttentionPool2d heads of {num_head_channels} channels over {ch}")
            self.pool_grid = image_size // ds
            self.pool_heads, self.pool_d_head = ch // num_head_channels, num_head_channels
            ap = _Slots(qkv_proj=_Params(weight=(3 * ch, ch, 1), bias=(3 * ch,)), c_proj=_Params(weight=(K, ch, 1), bias=(K,)))
            ap.register_parameter("positional_embedding", nn.Parameter(torch.empty(ch, self.pool_grid ** 2 + 1), requires_grad=False))
            self.out = _Slots(_0=_norm_params(ch), _2=ap)
        elif pool == "spatial":
            self.out = _Slots(_0=_lin_params(self._feature_size, SPATIAL_HIDDEN), _2=_lin_params(SPATIAL_HIDDEN, K))
        else:
            self.out = _Slots(_0=_lin_params(self._feature_size, SPATIAL_HIDDEN), _1=_norm_params(SPATIAL_HIDDEN),
                              _3=_lin_params(SPATIAL_HIDDEN, K))
        self.reset_parameters()
        self._packed = None
        self._trainer = None

    # ---- initialisation: PyTorch layer defaults + the reference's zero_module sites ----------------
    @torch.no_grad()
    def reset_parameters(self):
        params = dict(self.named_parameters())
        for name, p in params.items():
            if ".out_layers.3." in name or ".proj_out." in name or (self.pool == "adaptive" and name.startswith("out.3.")):
                p.zero_()                                   # openaimodel.py:229-231,313,896
            elif name.endswith("positional_embedding"):
                p.normal_().div_(p.shape[0] ** 0.5)         # openaimodel.py:45
            elif p.dim() >= 2:
                fan_in = p[0].numel()
                p.uniform_(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in))
            elif name.endswith(".bias"):
                owner = params.get(name[:-4] + "weight")
                if owner is not None and owner.dim() >= 2:
                    fan_in = owner[0].numel()
                    p.uniform_(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in))
                else:
                    p.zero_()       # norm bias
            else:
                p.fill_(1.0)        # norm weight

    def _walk(self):
        for i, blk in enumerate(self.input_blocks):
            for j, m in enumerate(blk.layers):
                yield f"input_blocks.{i}.{j}.", m
        for j, m in enumerate(self.middle_block.layers):
            yield f"middle_block.{j}.", m

    # ---- weight packing: torch layouts -> the layouts the training GEMMs read ---------------------------
    @torch.no_grad()
    def pack_weights(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.LdmkError("EncoderUNetModel: parameters must live on a GPU (model.cuda()); there is no CPU path")
        P = {}
        sd = {k: v.detach().float().contiguous() for k, v in self.named_parameters()}
        emb_w, emb_b = [], []
        self._emb_off = {}
        off = 0
        for prefix, m in self._walk():
            if m.kind == "res":
                P[prefix + "c1"] = ops.pack_conv3x3(sd[prefix + "in_layers.2.weight"])
                P[prefix + "c2"] = ops.pack_conv3x3(sd[prefix + "out_layers.3.weight"])
                if m.cin != m.cout:
                    P[prefix + "skip"] = ops.pack_linear(sd[prefix + "skip_connection.weight"])
                emb_w.append(sd[prefix + "emb_layers.1.weight"])
                emb_b.append(sd[prefix + "emb_layers.1.bias"])
                self._emb_off[prefix] = off
                off += 2 * m.cout if m.scale_shift else m.cout
            elif m.kind == "attn":
                pack_attention_block(P, sd, prefix, m)
            elif m.kind == "down":
                P[prefix + "w"] = ops.pack_conv3x3(sd[prefix + "op.weight"])
        P["emb_all"] = ops.pack_linear(torch.cat(emb_w, 0).contiguous())
        P["emb_all_b"] = torch.cat(emb_b, 0).contiguous()
        self._emb_total = off
        P["te0"] = ops.pack_linear(sd["time_embed.0.weight"])
        P["te2"] = ops.pack_linear(sd["time_embed.2.weight"])
        P["freqs"] = ops.timestep_freqs(self.model_channels, device=dev)
        self._sd = sd
        self._packed = P
        self._trainer = None

    def convert_to_fp16(self):
        """openaimodel.py:924-929 casts the torso to float16; this path is fp32 (use_fp16 is refused the same way)."""
        raise NotImplementedError("EncoderUNetModel.convert_to_fp16: fp32 only (reference precision; use_fp16 is refused the same way)")

    def convert_to_fp32(self):
        return None

    @torch.no_grad()
    def forward(self, x, timesteps):
        """x (N, C, H, W) fp32 NCHW, timesteps (N,) -> logits (N, K): the trainer's forward with the tape dropped."""
        from .train import EncoderUNetTrainer
        sig = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._trainer is None or self._trainer[0] != sig:
            self.pack_weights()
            self._trainer = (sig, EncoderUNetTrainer(self))
        return self._trainer[1].forward(x, timesteps, keep_tape=False)
