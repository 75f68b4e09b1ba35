"""Training the VQGAN and KL first stages (ldm/models/autoencoder.py:14-262 VQModel, :285-423 AutoencoderKL).

`FirstStageTrainer(model)`: encoder -> quant_conv -> bottleneck -> post_quant_conv -> decoder as one tape with parameter
gradients.  The bottleneck is one of two kinds: the quantiser of a VQ model (`bottleneck == "vq"`), or the diagonal-Gaussian
posterior of an `AutoencoderKL` with its KL term (`"kl"`, csrc/kl_train.hip); everything else is shared.
Parameters, gradients and Adam moments live in one `FlatParams` arena in the kernels' packed layouts, in forward order, like `UNetTrainer`.  The ResnetBlock / AttnBlock tapes below are a SECOND COPY of `DecoderGrad`'s (train_decoder.py),
written over arena views and with the weight gradients emitted instead of dropped (T.wgrad_conv3x3 / T.wgrad_linear, T.gn_bwd
with dgamma / dbeta): `DecoderGrad` reads a frozen module's tensors and caches its data-gradient weights, which a trainer
whose weights move every step cannot share, so the two are kept in step by hand.  The quantiser and the two narrow 1x1
convolutions around it are csrc/vq_train.hip.  The four boundary convolutions (3 or z_channels wide on one side) are
channel-padded to 32; the padding holds zeros, receives zero gradients and therefore stays zero under Adam.

fp32 parity arithmetic only; no dropout (refused at construction); `all_reduce_grads` is one blocking all-reduce over the
arena, not the bucketed overlap `UNetTrainer.backward` has.  No PyTorch fallback."""
import torch
import torch.nn.functional as F

from . import lib as L
from . import ops
from . import train_ops as T
from .train import FlatParams, gemm

EPS = 1e-6        # GroupNorm eps of model.py:38-39


def _unconv(wp, cin, cout):                    # [cin/32][9][32][cout] -> [cout][cin][3][3]
    return wp.view(cin // 32, 9, 32, cout).permute(3, 0, 2, 1).reshape(cout, cin, 3, 3).contiguous()


class FirstStageTrainer:
    def __init__(self, vq):
        if float(getattr(vq, "ddconfig", {}).get("dropout", 0.0) or 0.0) != 0.0:
            raise NotImplementedError("FirstStageTrainer: ddconfig dropout > 0 is not built (the tape has no dropout)")
        vq._ensure()
        self.vq, self.sd = vq, vq._sd
        self.dev = next(vq.parameters()).device
        e, d = vq.encoder, vq.decoder
        from .autoencoder import AutoencoderKL
        self.bottleneck = "vq" if hasattr(vq, "quantize") else ("kl" if isinstance(vq, AutoencoderKL) else None)
        if max(e.in_channels, e.z_out, d.z_channels, d.out_ch) > 32 or e.ch % 32 or self.bottleneck is None:
            raise NotImplementedError("FirstStageTrainer: a VQ or KL autoencoder with ch % 32 == 0 and boundary widths <= 32")
        if self.bottleneck == "vq":
            self.beta, self.legacy = float(vq.quantize.beta), bool(getattr(vq.quantize, "legacy", True))
        self.P = FlatParams()
        self.kind = {}          # arena name (= state-dict key) -> how its packed layout maps to the reference's
        self._collect()
        self.P.finalize(self.dev)
        self.tape = []
        self.acc_params = False

    # ---- parameters -------------------------------------------------------------------------------------------
    def _add(self, key, kind):
        w = self.sd[key]
        if kind == "conv":
            t = ops.pack_conv3x3(w)
        elif kind == "conv_padin":
            t = ops.pack_conv3x3(F.pad(w, (0, 0, 0, 0, 0, 32 - w.shape[1])).contiguous())
        elif kind == "conv_padout":
            t = ops.pack_conv3x3(F.pad(w, (0, 0, 0, 0, 0, 0, 0, 32 - w.shape[0])).contiguous())
        elif kind == "bias_pad":
            t = F.pad(w, (0, 32 - w.shape[0]))
        elif kind == "lin":
            t = ops.pack_linear(w)
        elif kind == "c11":
            t = w.reshape(w.shape[0], w.shape[1]).contiguous()
        else:
            t = w
        self.kind[key] = kind
        self.P.add(key, t)

    def _add_conv(self, p, kind="conv"):
        self._add(p + ".weight", kind)
        self._add(p + ".bias", "bias_pad" if kind == "conv_padout" else "raw")

    def _add_norm(self, p):
        self._add(p + ".weight", "raw")
        self._add(p + ".bias", "raw")

    def _add_resnet(self, p, m):
        self._add_norm(p + "norm1")
        self._add_conv(p + "conv1")
        self._add_norm(p + "norm2")
        self._add_conv(p + "conv2")
        if m.cin != m.cout:
            self._add_conv(p + "nin_shortcut", "lin")

    def _add_attn(self, p):
        self._add_norm(p + "norm")
        for k in ("q", "k", "v", "proj_out"):
            self._add_conv(p + k, "lin")

    def _collect(self):
        """Forward order, so that the backward finishes gradients from the end of the arena towards its start."""
        e, d = self.vq.encoder, self.vq.decoder
        self._add_conv("encoder.conv_in", "conv_padin")
        for lvl in range(e.num_resolutions):
            dn = e.down[lvl]
            for ib in range(e.num_res_blocks):
                self._add_resnet(f"encoder.down.{lvl}.block.{ib}.", dn.block[ib])
                if len(dn.attn) > 0:
                    self._add_attn(f"encoder.down.{lvl}.attn.{ib}.")
            if lvl != e.num_resolutions - 1:
                self._add_conv(f"encoder.down.{lvl}.downsample.conv")
        self._add_resnet("encoder.mid.block_1.", e.mid.block_1)
        self._add_attn("encoder.mid.attn_1.")
        self._add_resnet("encoder.mid.block_2.", e.mid.block_2)
        self._add_norm("encoder.norm_out")
        self._add_conv("encoder.conv_out", "conv_padout")
        self._add_conv("quant_conv", "c11")
        if self.bottleneck == "vq":
            self._add("quantize.embedding.weight", "raw")
        self._add_conv("post_quant_conv", "c11")
        self._add_conv("decoder.conv_in", "conv_padin")
        self._add_resnet("decoder.mid.block_1.", d.mid.block_1)
        self._add_attn("decoder.mid.attn_1.")
        self._add_resnet("decoder.mid.block_2.", d.mid.block_2)
        for lvl in reversed(range(d.num_resolutions)):
            up = d.up[lvl]
            for ib in range(d.num_res_blocks + 1):
                self._add_resnet(f"decoder.up.{lvl}.block.{ib}.", up.block[ib])
                if len(up.attn) > 0:
                    self._add_attn(f"decoder.up.{lvl}.attn.{ib}.")
            if lvl != 0:
                self._add_conv(f"decoder.up.{lvl}.upsample.conv")
        self._add_norm("decoder.norm_out")
        self._add_conv("decoder.conv_out", "conv_padout")
        missing = set(self.sd) - set(self.kind)
        assert not missing, f"parameters outside the arena: {sorted(missing)}"

    def _to_reference(self, name, t):
        kind, like = self.kind[name], self.sd[name]
        if kind == "conv":
            return _unconv(t, like.shape[1], like.shape[0])
        if kind == "conv_padin":
            return _unconv(t, 32, like.shape[0])[:, :like.shape[1]].contiguous()
        if kind == "conv_padout":
            return _unconv(t, like.shape[1], 32)[:like.shape[0]].contiguous()
        if kind == "bias_pad":
            return t[:like.shape[0]].clone()
        if kind == "lin":
            return t.t().contiguous().view(like.shape)
        return t.reshape(like.shape).clone()

    def state_dict_reference(self, flat=None):
        """The arena (or an EMA shadow of it) under the reference's state-dict keys and shapes."""
        src = self.P.flat if flat is None else flat
        return {name: self._to_reference(name, src[off:off + n].view(shape)) for name, shape, off, n in self.P.specs}

    def grads_reference(self):
        """The gradients of the last backward() under the reference's keys and shapes."""
        return self.state_dict_reference(self.P.grad)

    def sync_to_module(self, flat=None):
        sd = self.state_dict_reference(flat)
        with torch.no_grad():
            for k, prm in self.vq.named_parameters():
                prm.copy_(sd[k])
        self.vq.pack_weights()
        self.sd = self.vq._sd

    # ---- primitives (forward; each pushes its backward: gradient of the output -> gradient of the input) ---------------
    def _conv(self, x4, p, stride=1, pad_lo=1, upsample=False, residual=None, need_dx=True):
        n, h, w_, c = x4.shape
        wn, bn = p + ".weight", p + ".bias"
        wp = self.P.p[wn]
        cout = wp.shape[1]
        if upsample:
            oh, ow = 2 * h, 2 * w_
        else:
            oh, ow = (h + 2 * pad_lo - 3) // stride + 1 if pad_lo else (h + 1 - 3) // stride + 1, \
                     (w_ + 2 * pad_lo - 3) // stride + 1 if pad_lo else (w_ + 1 - 3) // stride + 1
        out = torch.empty(n, oh, ow, cout, device=self.dev)
        a = ops.make_igemm_args(n * oh * ow, cout, 9 * c, x4, c, wp, out, cout, oh * ow,
                                conv=(h, w_, oh, ow, stride, pad_lo, 1 if upsample else 0), bias=self.P.p[bn], residual=residual)
        gemm(a, self.dev)

        def bwd(dy):
            dy4 = dy.view(n, oh, ow, cout)
            T.wgrad_conv3x3(x4, dy4, stride=stride, pad_lo=pad_lo, upsample=upsample, dw=self.P.g[wn], dbias=self.P.g[bn],
                            accumulate=self.acc_params)
            if not need_dx:
                return None
            wd = T.pack_dgrad3x3(wp, c, cout)
            if upsample:
                return T.sumpool2(T.conv3x3_dgrad(dy4, wd, (2 * h, 2 * w_)))
            return T.conv3x3_dgrad(dy4, wd, (h, w_), stride=stride, pad_lo=pad_lo)
        return out, bwd

    def _lin(self, x2d, p, rows_per_sample, residual=None):
        wn, bn = p + ".weight", p + ".bias"
        wp = self.P.p[wn]
        M, K = x2d.shape
        N = wp.shape[1]
        out = torch.empty(M, N, device=self.dev)
        gemm(ops.make_igemm_args(M, N, K, x2d, K, wp, out, N, rows_per_sample, bias=self.P.p[bn], residual=residual), self.dev)

        def bwd(dy, dx_out=None, acc=False):
            T.wgrad_linear(x2d, dy, dw=self.P.g[wn], dbias=self.P.g[bn], accumulate=self.acc_params)
            dx = torch.empty(M, K, device=self.dev) if dx_out is None else dx_out
            gemm(ops.make_igemm_args(M, K, N, dy, N, wp, dx, K, M, b_trans=True, ldb=wp.stride(0), residual=dx if acc else None),
                 self.dev)
            return dx
        return out, bwd

    def _gn(self, x4, p, silu):
        n, h, w_, c = x4.shape
        hw = h * w_
        wn, bn = p + ".weight", p + ".bias"
        partial = torch.empty(n * L.load().ldmk_gn_chunks(hw) * c * 3, device=self.dev)
        coef = torch.empty(n, 2, c, device=self.dev)
        ops.gn_coef(x4, None, n, hw, self.P.p[wn], self.P.p[bn], EPS, partial=partial, coef=coef)
        mr = T.gn_group_stats(partial, c, None, 0, n, hw, 32, EPS)
        y = ops.gn_apply(x4, None, coef, n, hw, silu=silu)

        def bwd(dy2d):
            dx = torch.empty_like(x4)
            T.gn_bwd(x4, None, dy2d, coef, mr, self.P.p[wn], n, hw, silu=silu, dx0=dx, dgamma=self.P.g[wn], dbeta=self.P.g[bn],
                     acc_params=self.acc_params)
            return dx
        return y, bwd

    # ---- blocks (model.py:95-141 ResnetBlock, :157-202 AttnBlock) -----------------------------------------------
    def _resnet(self, p, m, x):
        n, h, w_, _ = x.shape
        rows = n * h * w_
        y1, b_n1 = self._gn(x, p + "norm1", True)
        h1, b_c1 = self._conv(y1.view(n, h, w_, m.cin), p + "conv1")
        y2, b_n2 = self._gn(h1, p + "norm2", True)
        b_sk = None
        if m.cin != m.cout:
            sk, b_sk = self._lin(x.view(rows, m.cin), p + "nin_shortcut", h * w_)
            out, b_c2 = self._conv(y2.view(n, h, w_, m.cout), p + "conv2", residual=sk)
        else:
            out, b_c2 = self._conv(y2.view(n, h, w_, m.cout), p + "conv2", residual=x)

        def bwd(dout):
            dx = b_n1(b_c1(b_n2(b_c2(dout).view(rows, -1))).view(rows, -1))
            if b_sk is not None:
                b_sk(dout.view(rows, -1), dx_out=dx.view(rows, -1), acc=True)
            else:
                T.axpy_(dx, dout, 1.0)
            return dx
        self.tape.append(bwd)
        return out

    def _attn(self, p, x):
        n, h, w_, c = x.shape
        hw, rows = h * w_, n * h * w_
        scale = float(int(c) ** (-0.5))
        xn, b_n = self._gn(x, p + "norm", False)
        q, b_q = self._lin(xn, p + "q", hw)
        k, b_k = self._lin(xn, p + "k", hw)
        v, b_v = self._lin(xn, p + "v", hw)
        pr = ops.bmm(q.view(n, hw, c), k.view(n, hw, c), True)
        ops.softmax_rows_(pr.view(rows, hw), scale)
        o = ops.bmm(pr, v.view(n, hw, c), False).view(rows, c)
        out, b_o = self._lin(o, p + "proj_out", hw, residual=x.view(rows, c))

        def bwd(dout):
            do = b_o(dout.view(rows, c)).view(n, hw, c)
            dv = torch.empty(n, hw, c, device=self.dev)
            T._wgrad_batched(pr, do, dv, n, hw, hw, c)                        # dV = P^T dO
            dp = ops.bmm(do, v.view(n, hw, c), True)                          # dP = dO V^T
            T.softmax_bwd_rows_(pr.view(rows, hw), dp.view(rows, hw), scale)
            dq = ops.bmm(dp, k.view(n, hw, c), False)                         # dQ = dS K
            dk = torch.empty(n, hw, c, device=self.dev)
            T._wgrad_batched(dp, q.view(n, hw, c), dk, n, hw, hw, c)          # dK = dS^T Q
            dxn = b_q(dq.view(rows, c))
            b_k(dk.view(rows, c), dx_out=dxn, acc=True)
            b_v(dv.view(rows, c), dx_out=dxn, acc=True)
            dx = b_n(dxn)
            T.axpy_(dx, dout.view_as(dx), 1.0)
            return dx
        self.tape.append(bwd)
        return out.view(n, h, w_, c)

    def _plain(self, pair):
        out, bwd = pair
        self.tape.append(bwd)
        return out

    # ---- the autoencoder -------------------------------------------------------------------------------------------
    def _pad_nhwc(self, x_nchw):
        n, c, h, w_ = x_nchw.shape
        out = torch.zeros(n, h, w_, 32, device=self.dev)
        out[..., :c] = x_nchw.permute(0, 2, 3, 1)
        return out

    def _quantise(self, hz):
        """quant_conv -> nearest code (straight-through) -> post_quant_conv; pushes the backward of the three."""
        p, d = self.P.p, self.vq.decoder
        z = ops.conv1x1_nchw(hz, p["quant_conv.weight"], p["quant_conv.bias"])
        cb = p["quantize.embedding.weight"]
        zq, idx = ops.vq_nearest(z, cb)
        idx = idx.reshape(-1)
        self.qloss, _ = T.vq_loss_bwd(z, cb, idx, beta=self.beta, legacy=self.legacy, want_dz=False)
        pq = ops.conv1x1_nchw(zq, p["post_quant_conv.weight"], p["post_quant_conv.bias"])
        self.z, self.zq, self.idx = z, zq, idx

        def bwd_quant(dpq_pad):
            g = self.P.g
            dpq = dpq_pad[..., :d.z_channels].permute(0, 3, 1, 2).contiguous()
            dzq, _, _ = T.conv1x1_nchw_bwd(zq, dpq, p["post_quant_conv.weight"], dw=g["post_quant_conv.weight"],
                                           db=g["post_quant_conv.bias"], accumulate=self.acc_params)
            cw = self._codebook_weight
            _, dz = T.vq_loss_bwd(z, cb, idx, dzq=dzq, beta=self.beta, legacy=self.legacy, w=cw)
            if self.acc_params:
                dE, self.counts = T.vq_codebook_grad(z, cb, idx, beta=self.beta, legacy=self.legacy, w=cw)
                T.axpy_(g["quantize.embedding.weight"], dE, 1.0)
            else:
                _, self.counts = T.vq_codebook_grad(z, cb, idx, beta=self.beta, legacy=self.legacy, w=cw,
                                                    dE=g["quantize.embedding.weight"])
            dhz, _, _ = T.conv1x1_nchw_bwd(hz, dz, p["quant_conv.weight"], dw=g["quant_conv.weight"], db=g["quant_conv.bias"],
                                           accumulate=self.acc_params)
            return self._pad_nhwc(dhz)
        self.tape.append(bwd_quant)
        return pq

    def _gaussian(self, hz, noise, sample_posterior):
        """quant_conv -> moments -> z = mean + std * noise (or the mean) and the per-sample KL -> post_quant_conv; pushes
        the backward of the three (AutoencoderKL.encode / forward / decode, autoencoder.py:324-342)."""
        p, d = self.P.p, self.vq.decoder
        moments = ops.conv1x1_nchw(hz, p["quant_conv.weight"], p["quant_conv.bias"])
        if sample_posterior:
            shape = (moments.shape[0], moments.shape[1] // 2) + tuple(moments.shape[2:])
            noise = self.vq.sample_noise(shape) if noise is None else noise
            noise = noise.to(self.dev, torch.float32).contiguous()
        else:
            noise = None
        z, kl = T.gauss_kl_fwd(moments, noise)
        pq = ops.conv1x1_nchw(z, p["post_quant_conv.weight"], p["post_quant_conv.bias"])
        self.moments, self.z, self.kl, self.noise = moments, z, kl, noise

        def bwd_gauss(dpq_pad):
            g = self.P.g
            dpq = dpq_pad[..., :d.z_channels].permute(0, 3, 1, 2).contiguous()
            dz, _, _ = T.conv1x1_nchw_bwd(z, dpq, p["post_quant_conv.weight"], dw=g["post_quant_conv.weight"],
                                          db=g["post_quant_conv.bias"], accumulate=self.acc_params)
            dmom = T.gauss_kl_bwd(moments, noise, dz, self._kl_weight / moments.shape[0])
            dhz, _, _ = T.conv1x1_nchw_bwd(hz, dmom, p["quant_conv.weight"], dw=g["quant_conv.weight"], db=g["quant_conv.bias"],
                                           accumulate=self.acc_params)
            return self._pad_nhwc(dhz)
        self.tape.append(bwd_gauss)
        return pq

    def forward(self, x, noise=None, sample_posterior=True):
        """x (n,in_channels,H,W) -> xrec (n,out_ch,H,W).  VQ (VQModel.forward, autoencoder.py:76-89,104-110): keeps z
        (pre-quantisation latent), zq, idx (int32) and qloss (the unweighted codebook loss, a device scalar).  KL
        (AutoencoderKL.forward, autoencoder.py:335-342): keeps moments, z (the draw from `noise`, default
        `model.sample_noise`; the mean without sample_posterior) and kl (n,); `noise` / `sample_posterior` are KL's alone."""
        if not x.is_cuda:
            raise L.LdmkError("FirstStageTrainer.forward: CUDA tensors only (no CPU fallback)")
        T.set_compute("f32")
        vq, e, d, p = self.vq, self.vq.encoder, self.vq.decoder, self.P.p
        self.tape = []
        n = x.shape[0]
        h = self._plain(self._conv(self._pad_nhwc(x.float()), "encoder.conv_in", need_dx=False))
        for lvl in range(e.num_resolutions):
            dn = e.down[lvl]
            for ib in range(e.num_res_blocks):
                h = self._resnet(f"encoder.down.{lvl}.block.{ib}.", dn.block[ib], h)
                if len(dn.attn) > 0:
                    h = self._attn(f"encoder.down.{lvl}.attn.{ib}.", h)
            if lvl != e.num_resolutions - 1:
                h = self._plain(self._conv(h, f"encoder.down.{lvl}.downsample.conv", stride=2, pad_lo=0))
        h = self._resnet("encoder.mid.block_1.", e.mid.block_1, h)
        h = self._attn("encoder.mid.attn_1.", h)
        h = self._resnet("encoder.mid.block_2.", e.mid.block_2, h)
        _, lh, lw, cf = h.shape
        y, b_no = self._gn(h, "encoder.norm_out", True)
        hz_pad, b_co = self._conv(y.view(n, lh, lw, cf), "encoder.conv_out")
        self.tape.append(lambda g: b_no(b_co(g).view(n * lh * lw, -1)))
        hz = hz_pad[..., :e.z_out].permute(0, 3, 1, 2).contiguous()
        pq = self._quantise(hz) if self.bottleneck == "vq" else self._gaussian(hz, noise, sample_posterior)
        h = self._plain(self._conv(self._pad_nhwc(pq), "decoder.conv_in"))
        h = self._resnet("decoder.mid.block_1.", d.mid.block_1, h)
        h = self._attn("decoder.mid.attn_1.", h)
        h = self._resnet("decoder.mid.block_2.", d.mid.block_2, h)
        for lvl in reversed(range(d.num_resolutions)):
            up = d.up[lvl]
            for ib in range(d.num_res_blocks + 1):
                h = self._resnet(f"decoder.up.{lvl}.block.{ib}.", up.block[ib], h)
                if len(up.attn) > 0:
                    h = self._attn(f"decoder.up.{lvl}.attn.{ib}.", h)
            if lvl != 0:
                h = self._plain(self._conv(h, f"decoder.up.{lvl}.upsample.conv", upsample=True))
        nf, hf, wf, cf = h.shape
        y, b_no2 = self._gn(h, "decoder.norm_out", True)
        self._last_in = y.view(nf, hf, wf, cf)
        img_pad, b_co2 = self._conv(self._last_in, "decoder.conv_out")
        self.tape.append(lambda g: b_no2(b_co2(g).view(nf * hf * wf, -1)))
        return img_pad[..., :d.out_ch].permute(0, 3, 1, 2).contiguous()

    def backward(self, d_image, codebook_weight=1.0, kl_weight=1.0):
        """d_image (n,out_ch,H,W): gradient of the image-space loss terms.  VQ: the codebook loss enters with
        `codebook_weight`, and `counts` holds the hits per code afterwards.  KL: kl_weight * mean_b kl[b] enters at the
        bottleneck.  Fills (with acc_params: adds to) P.grad."""
        T.set_compute("f32")
        self._codebook_weight, self._kl_weight = float(codebook_weight), float(kl_weight)
        g = self._pad_nhwc(d_image.float())
        for fn in reversed(self.tape):
            g = fn(g)
        self.tape = []

    def last_layer_grad(self, d_image):
        """The weight gradient of decoder.conv_out alone, in the reference's (out_ch, C, 3, 3) layout: what the adaptive
        discriminator weight needs (vqperceptual.py:63-75).  Uses the saved input of the last forward; touches no P.grad."""
        T.set_compute("f32")
        dw = T.wgrad_conv3x3(self._last_in, self._pad_nhwc(d_image.float()))
        return self._to_reference("decoder.conv_out.weight", dw)

    # ---- optimiser -----------------------------------------------------------------------------------------------
    def adam_step(self, lr, betas=(0.5, 0.9), eps=1e-8):
        """torch.optim.Adam as VQModel.configure_optimizers sets it up (autoencoder.py:160-163): ldmk_adamw, no decay."""
        P = self.P
        if P.m is None:
            P.m, P.v = torch.zeros_like(P.flat), torch.zeros_like(P.flat)
        P.step += 1
        T.adamw_(P.flat, P.grad, P.m, P.v, lr, betas, eps, 0.0, P.step)

    def ema_update(self, shadow_flat, decay):
        T.ema_(shadow_flat, self.P.flat, 1.0 - decay)

    def all_reduce_grads(self, world_size):
        import torch.distributed as dist
        dist.all_reduce(self.P.grad)
        self.P.grad.mul_(1.0 / world_size)
