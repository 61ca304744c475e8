"""The VGGT teacher's dense-prediction heads (vggt/heads/dpt_head.py DPTHead: depth_head, point_head, track_head.feature_extractor) on the HIP
kernels instead of the user's PyTorch module.

Every map lives channel-last on the separator-column layout of gd_stack3_rows, [gh * (gw + 1), C], so that each 3x3 convolution is ONE gemm_nt on
the overlapping-row view of a 3-row stacked operand (ops.stack3_rows / ops.conv_view), with bias, ReLU and the residual unit's skip in the GEMM
epilogue.  Around the GEMMs run the kernels of csrc/dpt.hip: gd_deconv_scatter (the pixel shuffle of the kernel = stride transposed convolutions),
gd_grid_resample (bilinear align_corners resampling with the fusion block's `output + res` and the position embedding added on the way, written
either as a grid or directly as the next convolution's stacked operand) and gd_dpt_head_out (1x1 convolution, split, activate_head).

Two rearrangements, both exact up to rounding:
  * a fusion block's 1x1 `out_conv` runs BEFORE its upsampling, on the small grid (bilinear weights sum to one, so the two commute, bias included);
    the upsampling is then the next block's gd_grid_resample, which adds that block's residual-unit output in the same pass;
  * the map resampled to image size plus position embedding is written once, as the operand of `output_conv2[0]`, never as a plain map.

A residual unit whose activation is ReLU(inplace=True) — the teacher's — rectifies its input before the skip reads it: skip = relu(x).  The unit's
`activation.inplace` flag is honoured: in place, the producer of x rectifies (GEMM epilogue / resample flag); out of place, the operand producer does
(gd_grid_resample at identity size with the ReLU flag) and the skip stays x.

The module stays the user's: this class reads its parameters (duck-typed on the attribute names, as teacher_blocks._BlockParams does), packs them
once into the operand layout, and refuses, naming the attribute, anything the kernels do not serve.  Off by default
(teacher_runner.VGGTTeacherRunner(fused_heads=True))."""
import functools

import torch

from . import ops
from ._lib import GdHipError


def _sincos(coords, channels):
    half = channels // 2
    omega = 1.0 / 100.0 ** (torch.arange(half, dtype=torch.float64) / half)
    ang = coords.reshape(-1, 1) * omega                    # float32 coordinates, fp64 frequencies and angles
    return torch.cat([ang.sin(), ang.cos()], dim=1).float()


@functools.lru_cache(maxsize=64)
def pos_tables(gw, gh, channels, aspect, ratio=0.1):
    """The head's position embedding (`_apply_pos_embed`) of a gh x gw map of `channels` channels is separable: the first half of the channels
    depends on x only, the second on y only, each [sin | cos] of coord * 100^(-j / (C/4)) in fp64, cast to float, times `ratio`.  The coordinates are
    the float32 linspace of +-span * (n - 1) / n, span_x = a / sqrt(a^2 + 1), span_y = 1 / sqrt(a^2 + 1), a = W / H of the IMAGE.
    -> (px [gw, C/2], py [gh, C/2]) float32 on the host, cached per (grid, C, aspect)."""
    diag = (aspect ** 2 + 1.0) ** 0.5
    sx, sy = aspect / diag, 1.0 / diag
    xs = torch.linspace(-sx * (gw - 1) / gw, sx * (gw - 1) / gw, steps=gw, dtype=torch.float32)
    ys = torch.linspace(-sy * (gh - 1) / gh, sy * (gh - 1) / gh, steps=gh, dtype=torch.float32)
    return _sincos(xs, channels // 2) * ratio, _sincos(ys, channels // 2) * ratio


class _Unit:
    """One residual unit: the two packed 3x3 weights, their biases, and whether its ReLU works in place."""


class FusedDPTHead:
    """FusedDPTHead(head, dtype=torch.float32).forward(aggregated_tokens_list, images, patch_start_idx, frames_chunk_size=None): what the module
    returns — (preds [B, S, H, W, output_dim - 1], conf [B, S, H, W]) fp32, or features [B, S, C, H', W'] when `feature_only`.

    dtype: the operand type of the matrix products.  torch.float32: exact operands, the faithful mode (the teacher runs its heads in fp32).
    torch.bfloat16: bf16 operands, fp32 accumulation, fp32 for everything that is added (skips, addends, embeddings): narrower, faster."""

    def __init__(self, head, dtype=torch.float32, name="head"):
        if dtype not in (torch.float32, torch.bfloat16):
            raise GdHipError("FusedDPTHead: dtype must be torch.float32 or torch.bfloat16")
        self.dtype, self.name = dtype, name

        def fail(attr, why):
            raise GdHipError(f"FusedDPTHead: {name}.{attr}: {why}")

        def need(obj, attr, where):
            if not hasattr(obj, attr):
                fail(f"{where}.{attr}" if where else attr, "missing")
            return getattr(obj, attr)
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        op = lambda t: t.detach().to(dtype).contiguous()
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)

        def chan(c, attr):
            if c % 8:
                fail(attr, f"{c} channels: the kernels move 16-byte chunks of either operand type, channel counts must be multiples of 8")

        def conv(m, attr, k, stride=1):
            """-> (packed weight [n, (kx, ky, c)] in the operand dtype, bias fp32 or None) of a k x k Conv2d with padding k // 2."""
            if not isinstance(m, torch.nn.Conv2d):
                fail(attr, f"is {type(m).__name__}, not a Conv2d")
            if m.groups != 1:
                fail(attr, f"groups = {m.groups}: served is groups = 1")
            if pair(m.kernel_size) != (k, k) or pair(m.stride) != (stride, stride) or pair(m.padding) != (k // 2, k // 2) or pair(m.dilation) != (1, 1):
                fail(attr, f"kernel {pair(m.kernel_size)} stride {pair(m.stride)} padding {m.padding} dilation {pair(m.dilation)}: served here is "
                           f"kernel {k}, stride {stride}, padding {k // 2}")
            chan(m.in_channels, attr)
            if attr != "scratch.output_conv2[2]":
                chan(m.out_channels, attr)
            return op(m.weight.permute(0, 3, 2, 1).reshape(m.out_channels, k * k * m.in_channels)), f32(m.bias)

        self.patch = int(need(head, "patch_size", ""))
        self.layer_idx = [int(i) for i in need(head, "intermediate_layer_idx", "")]
        self.pos_embed, self.feature_only = bool(need(head, "pos_embed", "")), bool(need(head, "feature_only", ""))
        self.down_ratio = need(head, "down_ratio", "")
        if len(self.layer_idx) != 4:
            fail("intermediate_layer_idx", f"{len(self.layer_idx)} entries: the head fuses four levels")
        if not self.feature_only:
            self.activation, self.conf_activation = need(head, "activation", ""), need(head, "conf_activation", "")
            if self.activation not in ops.DPT_ACT:
                fail("activation", f"{self.activation!r}: gd_dpt_head_out serves {sorted(ops.DPT_ACT)}")
            if self.conf_activation not in ops.DPT_CONF_ACT or self.conf_activation == "linear":
                fail("conf_activation", f"{self.conf_activation!r}: gd_dpt_head_out serves ['expp0', 'expp1', 'sigmoid']")
        norm = need(head, "norm", "")
        if not (isinstance(norm, torch.nn.LayerNorm) and norm.elementwise_affine and len(norm.normalized_shape) == 1):
            fail("norm", "is not an affine LayerNorm over the token width")
        self.norm = (f32(norm.weight), f32(norm.bias), float(norm.eps))
        dim_in = norm.normalized_shape[0]
        chan(dim_in, "norm")
        projects, resize, scratch = need(head, "projects", ""), need(head, "resize_layers", ""), need(head, "scratch", "")
        if len(projects) != 4 or len(resize) != 4:
            fail("projects", f"{len(projects)} projections / {len(resize)} resize layers: the head fuses four levels")
        self.proj, self.resize = [], []
        for i in range(4):
            w, b = conv(projects[i], f"projects[{i}]", 1)
            if projects[i].in_channels != dim_in:
                fail(f"projects[{i}]", f"takes {projects[i].in_channels} channels, the tokens have {dim_in}")
            self.proj.append((w, b))
            m, attr, c = resize[i], f"resize_layers[{i}]", projects[i].out_channels
            if isinstance(m, torch.nn.Identity):
                self.resize.append(("identity", c))
            elif isinstance(m, torch.nn.ConvTranspose2d):
                k = pair(m.kernel_size)[0]
                if (m.groups != 1 or pair(m.kernel_size) != (k, k) or pair(m.stride) != (k, k) or pair(m.padding) != (0, 0) or pair(m.output_padding) != (0, 0)
                        or pair(m.dilation) != (1, 1) or k > 8 or m.in_channels != c):
                    fail(attr, "served is a ConvTranspose2d with kernel = stride <= 8, no padding, groups = 1")
                chan(m.out_channels, attr)
                bias = f32(m.bias) if m.bias is not None else torch.zeros(m.out_channels, dtype=torch.float32, device=m.weight.device)
                # weight [c, n, ky, kx] -> [(ky, kx, n), c]: the GEMM's columns in the order gd_deconv_scatter reads them
                self.resize.append(("deconv", m.out_channels, k, op(m.weight.permute(2, 3, 1, 0).reshape(k * k * m.out_channels, c)), bias))
            elif isinstance(m, torch.nn.Conv2d):
                if m.in_channels != c:
                    fail(attr, f"takes {m.in_channels} channels, projects[{i}] gives {c}")
                self.resize.append(("conv_s2", m.out_channels) + conv(m, attr, 3, stride=2))
            else:
                fail(attr, f"is {type(m).__name__}: served are ConvTranspose2d (kernel = stride), Identity and Conv2d(kernel 3, stride 2, padding 1)")
        self.rn = []
        for i in range(4):
            m = need(scratch, f"layer{i + 1}_rn", "scratch")
            w, b = conv(m, f"scratch.layer{i + 1}_rn", 3)
            if m.in_channels != self.resize[i][1]:
                fail(f"scratch.layer{i + 1}_rn", f"takes {m.in_channels} channels, resize_layers[{i}] gives {self.resize[i][1]}")
            self.rn.append((w, b))
        self.features = features = scratch.layer1_rn.out_channels

        def unit(u, attr):
            if getattr(u, "bn", False) or getattr(u, "norm1", None) is not None or getattr(u, "norm2", None) is not None:
                fail(f"{attr}.bn", "a batch-norm inside a residual unit is not served")
            if getattr(u, "groups", 1) != 1:
                fail(f"{attr}.groups", f"{u.groups}: served is groups = 1")
            act = getattr(u, "activation", None)
            if not isinstance(act, torch.nn.ReLU):
                fail(f"{attr}.activation", f"is {type(act).__name__}: served is ReLU")
            p = _Unit()
            p.inplace = bool(act.inplace)
            (p.w1, p.b1), (p.w2, p.b2) = conv(need(u, "conv1", attr), f"{attr}.conv1", 3), conv(need(u, "conv2", attr), f"{attr}.conv2", 3)
            if not (u.conv1.in_channels == u.conv1.out_channels == u.conv2.in_channels == u.conv2.out_channels == features):
                fail(attr, f"its convolutions are not {features} -> {features}")
            return p
        self.fusion = []
        for i in range(4):
            attr = f"scratch.refinenet{i + 1}"
            blk = need(scratch, f"refinenet{i + 1}", "scratch")
            for flag in ("deconv", "expand"):
                if getattr(blk, flag, False):
                    fail(f"{attr}.{flag}", "True: not served")
            if getattr(blk, "align_corners", True) is not True:
                fail(f"{attr}.align_corners", f"{blk.align_corners}: gd_grid_resample resamples with align_corners=True")
            if getattr(blk, "groups", 1) != 1:
                fail(f"{attr}.groups", f"{blk.groups}: served is groups = 1")
            if getattr(blk, "size", None) is not None:
                fail(f"{attr}.size", "a fixed output size is not served")
            has_res = bool(getattr(blk, "has_residual", hasattr(blk, "resConfUnit1")))
            if has_res != (i != 3):
                fail(f"{attr}.has_residual", f"{has_res}: the first three blocks take a skip input, the fourth does not")
            oc = conv(need(blk, "out_conv", attr), f"{attr}.out_conv", 1)
            if blk.out_conv.in_channels != features or blk.out_conv.out_channels != features:
                fail(f"{attr}.out_conv", f"is not {features} -> {features}")
            self.fusion.append((unit(blk.resConfUnit1, f"{attr}.resConfUnit1") if has_res else None, unit(blk.resConfUnit2, f"{attr}.resConfUnit2"), oc))
        oc1 = need(scratch, "output_conv1", "scratch")
        self.out1 = conv(oc1, "scratch.output_conv1", 3)
        if oc1.in_channels != features:
            fail("scratch.output_conv1", f"takes {oc1.in_channels} channels, the fusion blocks give {features}")
        self.c_out1 = oc1.out_channels
        if not self.feature_only:
            oc2 = need(scratch, "output_conv2", "scratch")
            if not (isinstance(oc2, torch.nn.Sequential) and len(oc2) == 3 and isinstance(oc2[1], torch.nn.ReLU)):
                fail("scratch.output_conv2", "served is Sequential(Conv2d 3x3, ReLU, Conv2d 1x1)")
            self.out2 = conv(oc2[0], "scratch.output_conv2[0]", 3)
            conv(oc2[2], "scratch.output_conv2[2]", 1)
            if oc2[0].in_channels != self.c_out1 or oc2[2].in_channels != oc2[0].out_channels:
                fail("scratch.output_conv2", "channel counts do not chain")
            self.output_dim = oc2[2].out_channels
            if not 2 <= self.output_dim <= 8:
                fail("scratch.output_conv2[2]", f"output_dim {self.output_dim}: gd_dpt_head_out serves 2 .. 8")
            self.w_last = f32(oc2[2].weight.reshape(self.output_dim, -1))
            self.b_last = f32(oc2[2].bias) if oc2[2].bias is not None else torch.zeros(self.output_dim, dtype=torch.float32, device=oc2[2].weight.device)
        self._tables = {}

    # ------------------------------------------------------------------------------------------------------------------------------
    def _pos(self, gw, gh, C, aspect, dev):
        """(px, py, their sum laid out as token rows [gh*gw, C]) on the device."""
        key = (gw, gh, C, aspect, str(dev))
        if key not in self._tables:
            px, py = (t.to(dev) for t in pos_tables(gw, gh, C, aspect))
            rows = torch.cat([px[None].expand(gh, gw, C // 2), py[:, None].expand(gh, gw, C // 2)], dim=-1).reshape(gh * gw, C).contiguous()
            self._tables[key] = (px.contiguous(), py.contiguous(), rows)
        return self._tables[key]

    def _op(self, x):
        return x if self.dtype == torch.float32 else ops.cast(x, self.dtype)

    def _conv3(self, buf, gh, gw, C, wb, act=0, residual=None):
        """3x3 convolution of a stacked operand: -> the pitched fp32 grid [gh*(gw+1), n] (separator rows hold finite values nobody reads)."""
        return ops.gemm_nt(ops.conv_view(buf, gh * (gw + 1), C), wb[0], out_dtype=torch.float32, bias=wb[1], act=act, residual=residual)

    def _stack(self, grid, gh, gw, C):
        return ops.stack3_rows(grid, 1, gh, gw, C, gh * (gw + 1) * C, 0, gw + 1, self.dtype)

    def _unit(self, p, x, gh, gw):
        """x: the pitched fp32 grid — ALREADY rectified by its producer when p.inplace.  -> skip + conv2(relu(conv1(relu(x))))."""
        C = self.features
        buf = self._stack(x, gh, gw, C) if p.inplace else ops.grid_resample(x, 1, gh, gw, gh, gw, C, relu=True, stacked=self.dtype)
        h = self._conv3(buf, gh, gw, C, (p.w1, p.b1), act=2)
        return self._conv3(self._stack(h, gh, gw, C), gh, gw, C, (p.w2, p.b2), residual=x)

    def _frame(self, toks, gh, gw, img_hw, taps):
        """One frame: toks the four [gh*gw, dim_in] token-row views -> (preds [1, H, W, od-1], conf [1, H, W]) or features [C, H', W']."""
        dt, C, dev = self.dtype, self.features, toks[0].device
        aspect = img_hw[1] / img_hw[0]
        sizes, skips = [], []
        for i in range(4):
            x = toks[i] if toks[i].dtype in (torch.float32, torch.bfloat16) else toks[i].float()
            y, _, _ = ops.layernorm_fwd(x, *self.norm, save_stats=False, out_dtype=dt)
            w, b = self.proj[i]
            res = self._pos(gw, gh, w.shape[0], aspect, dev)[2] if self.pos_embed else None
            p = ops.gemm_nt(y, w, out_dtype=torch.float32, bias=b, residual=res)                     # token rows [gh*gw, oc]
            kind, c = self.resize[i][:2]
            first = self.fusion[i][0] or self.fusion[i][1]        # the unit that reads layer{i+1}_rn's output
            if kind == "deconv":
                _, _, k, wd, bd = self.resize[i]
                grid = ops.deconv_scatter(ops.gemm_nt(self._op(p), wd, out_dtype=torch.float32), bd, 1, gh, gw, gw, k, c)
                h, wd_ = gh * k, gw * k
                buf = ops.stack3_rows(grid, 1, h, wd_, c, h * (wd_ + 1) * c, 0, wd_ + 1, dt)
            elif kind == "identity":
                h, wd_ = gh, gw
                buf = ops.stack3_rows(p, 1, gh, gw, c, gh * gw * c, 0, gw, dt)
            else:       # kernel 3, stride 2, padding 1: the full-resolution convolution, then every second row and column
                cin = w.shape[0]
                full = self._conv3(ops.stack3_rows(p, 1, gh, gw, cin, gh * gw * cin, 0, gw, dt), gh, gw, cin, self.resize[i][2:])
                h, wd_ = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
                buf = ops.grid_resample(full, 1, gh, gw, h, wd_, c, step=2, stacked=dt)
            sizes.append((h, wd_))
            skips.append(self._conv3(buf, h, wd_, c, self.rn[i], act=2 if first.inplace else 0))
        o, prev = None, None
        for i in (3, 2, 1, 0):
            (h, w_), (u1, u2, oc) = sizes[i], self.fusion[i]
            if u1 is None:
                x = skips[i]
            else:
                x = ops.grid_resample(o, 1, prev[0], prev[1], h, w_, C, addend=self._unit(u1, skips[i], h, w_), relu=u2.inplace)
            y = self._unit(u2, x, h, w_)
            o = ops.gemm_nt(self._op(y), oc[0], out_dtype=torch.float32, bias=oc[1])          # out_conv on the small grid: it commutes with the upsampling
            prev = (h, w_)
        h, w_ = int(prev[0] * 2), int(prev[1] * 2)              # refinenet1 upsamples by scale_factor = 2
        fused = self._conv3(ops.grid_resample(o, 1, prev[0], prev[1], h, w_, C, stacked=dt), h, w_, C, self.out1)
        th, tw = int(gh * self.patch / self.down_ratio), int(gw * self.patch / self.down_ratio)
        C1 = self.c_out1
        px, py = self._pos(tw, th, C1, aspect, dev)[:2] if self.pos_embed else (None, None)
        if self.feature_only:
            if taps is not None:
                taps.setdefault("pre", []).append(fused.view(h, w_ + 1, C1)[:, :w_].permute(2, 0, 1))
            return ops.grid_resample(fused, 1, h, w_, th, tw, C1, px=px, py=py).view(th, tw + 1, C1)[:, :tw].permute(2, 0, 1)
        hid = self._conv3(ops.grid_resample(fused, 1, h, w_, th, tw, C1, px=px, py=py, stacked=dt), th, tw, C1, self.out2, act=2)
        if taps is not None:
            v, c = ops.dpt_head_out(hid, self.w_last, self.b_last, 1, th, tw, "linear", "linear")
            taps.setdefault("pre", []).append(torch.cat([v, c[..., None]], dim=-1)[0].permute(2, 0, 1))
        return ops.dpt_head_out(hid, self.w_last, self.b_last, 1, th, tw, self.activation, self.conf_activation)

    @torch.no_grad()
    def forward(self, aggregated_tokens_list, images, patch_start_idx, frames_chunk_size=None, taps=None):
        """Same signature and result as the module's forward.  Frames are independent and always run one at a time (at the teacher's size the fp32
        operand of the last convolution is ~410 MB per frame), so `frames_chunk_size` changes neither the result nor the peak memory.
        taps: a dict that receives "pre" — the map before the activations [B*S, output_dim, H, W], or with feature_only the fused map before the
        last resampling (what the tests compare with the reference's)."""
        B, S, _, H, W = images.shape
        gh, gw = H // self.patch, W // self.patch
        outs = []
        for b in range(B):
            for s in range(S):
                toks = []
                for li in self.layer_idx:
                    t = aggregated_tokens_list[li]
                    if not t.is_cuda or t.dim() != 4 or t.shape[2] - patch_start_idx != gh * gw or t.stride(-1) != 1:
                        raise GdHipError(f"FusedDPTHead: {self.name}: aggregated_tokens_list[{li}] {tuple(t.shape)} on {t.device} does not hold a "
                                         f"{gh} x {gw} patch grid after {patch_start_idx} prefix tokens on the GPU")
                    toks.append(t[b, s, patch_start_idx:])
                outs.append(self._frame(toks, gh, gw, (H, W), taps))
        if taps is not None:
            taps["pre"] = torch.stack(taps["pre"])
        if self.feature_only:
            f = torch.stack(outs)
            return f.view(B, S, *f.shape[1:])
        preds, conf = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        return preds.view(B, S, *preds.shape[1:]), conf.view(B, S, *conf.shape[1:])

    __call__ = forward
