"""The teachers' dense-prediction heads on the HIP kernels instead of the user's PyTorch modules: FusedDPTHead for the VGGT teacher
(vggt/heads/dpt_head.py DPTHead: depth_head, point_head, track_head.feature_extractor) and FusedMASt3RHead for the MASt3R teacher
(mast3r/catmlp_dpt_head.py Cat_MLP_LocalFeatures_DPT_Pts3d: downstream_head1 / downstream_head2).

Every map lives channel-last on the separator-column layout of gd_stack3_rows, [gh * (gw + 1), C], so that each 3x3 convolution is ONE gemm_nt on
the overlapping-row view of a 3-row stacked operand (ops.stack3_rows / ops.conv_view), with bias, ReLU and the residual unit's skip in the GEMM
epilogue.  Around the GEMMs run the kernels of csrc/dpt.hip: gd_deconv_scatter (the pixel shuffle of the kernel = stride transposed convolutions),
gd_grid_resample (bilinear align_corners resampling with the fusion block's `output + res` and the position embedding added on the way, written
either as a grid or directly as the next convolution's stacked operand), gd_dpt_head_out (1x1 convolution, split, activate_head) and
gd_mast3r_head_out (1x1 convolution, the local-feature MLP's pixel shuffle, and the MASt3R postprocess).

Two rearrangements, both exact up to rounding:
  * a fusion block's 1x1 `out_conv` runs BEFORE its upsampling, on the small grid (bilinear weights sum to one, so the two commute, bias included);
    the upsampling is then the next block's gd_grid_resample, which adds that block's residual-unit output in the same pass;
  * a map resampled to its last size (plus position embedding) is written once, as the operand of the convolution that reads it, never as a plain map.

A residual unit whose activation is ReLU(inplace=True) — the VGGT teacher's — rectifies its input before the skip reads it: skip = relu(x).  The unit's
`activation.inplace` flag is honoured: in place, the producer of x rectifies (GEMM epilogue / resample flag); out of place — the MASt3R teacher's —
the operand producer does (gd_grid_resample at identity size with the ReLU flag) and the skip stays x.

The modules stay the user's: these classes read their parameters (duck-typed on the attribute names, through teacher_read.Reader as teacher_blocks._ViTBlock does), pack them
once into the operand layout, and refuse, naming the attribute, anything the kernels do not serve.  Off by default
(teacher_runner.VGGTTeacherRunner(fused_heads=True), teacher_runner.MASt3RTeacherRunner(fused_heads=True)).

_FusedHead holds what the two share: the weight packers, the per-level resize + `layer_rn`, the residual unit and the fusion loop.

FusedCameraHead, at the end of the file, is the VGGT teacher's camera head (vggt/heads/camera_head.py) on the few-row kernels of csrc/rows.hip
(teacher_runner.VGGTTeacherRunner(fused_camera_head=True), off by default): no maps, M = B * S <= 8 token rows and a weight stream."""
import functools

import torch

from . import ops
from ._lib import GdHipError
from .teacher_read import Reader, f32, to_device


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


def pack_pixel_shuffle(t, patch):
    """Rows of a Linear's weight [n * patch^2, K] (or its bias [n * patch^2]) whose outputs F.pixel_shuffle(., patch) reads in the order (c, i, j)
    -> the order (i, j, c): a pixel's n values become contiguous columns of the GEMM's output (what gd_mast3r_head_out addresses)."""
    n = t.shape[0] // (patch * patch)
    return t.reshape(n, patch * patch, *t.shape[1:]).transpose(0, 1).reshape(t.shape).contiguous()


_pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class _Unit:
    """One residual unit: the two packed 3x3 weights, their biases, and whether its ReLU works in place."""


class _FusedHead:
    """What FusedDPTHead and FusedMASt3RHead share.  Reading: `_fail` / `_need` (the teacher_read.Reader's), `_chan` and the packers `_pack_conv`, `_pack_resize`,
    `_pack_unit`, `_pack_fusion` (a refusal reads '<class>: <name>.<attribute>: <why>').  Running: `_op`, `_stack`, `_conv3`, `_unit`, `_level`, `_fuse`
    on `frames` pitched grids at once.  A subclass fills self.resize, self.rn, self.fusion (four entries each) and self.features."""

    def __init__(self, dtype, name):
        if dtype not in (torch.float32, torch.bfloat16):
            raise GdHipError(f"{type(self).__name__}: dtype must be torch.float32 or torch.bfloat16")
        self.dtype, self.name = dtype, name
        r = self._r = Reader(type(self).__name__, name)
        # a head's attribute that is present and None is the module's own value (pos_embed, feature_only, conf_mode, ...): only an absent one is missing
        self._fail, self._need = r.fail, functools.partial(r.need, none_ok=True)

    # ---- reading the module -------------------------------------------------------------------------------------------------------
    def _to_op(self, t):
        return t.detach().to(self.dtype).contiguous()

    def _chan(self, c, attr):
        if c % 8:
            self._fail(attr, f"{c} channels: the kernels move 16-byte chunks of either operand type, channel counts must be multiples of 8")

    def _pack_conv(self, m, attr, k, stride=1, any_out=False):
        """-> (packed weight [n, (kx, ky, c)] in the operand dtype, bias fp32 or None) of a k x k Conv2d with padding k // 2."""
        if not isinstance(m, torch.nn.Conv2d):
            self._fail(attr, f"is {type(m).__name__}, not a Conv2d")
        if m.groups != 1:
            self._fail(attr, f"groups = {m.groups}: served is groups = 1")
        if _pair(m.kernel_size) != (k, k) or _pair(m.stride) != (stride, stride) or _pair(m.padding) != (k // 2, k // 2) or _pair(m.dilation) != (1, 1):
            self._fail(attr, f"kernel {_pair(m.kernel_size)} stride {_pair(m.stride)} padding {m.padding} dilation {_pair(m.dilation)}: served here is "
                             f"kernel {k}, stride {stride}, padding {k // 2}")
        self._chan(m.in_channels, attr)
        if not any_out:
            self._chan(m.out_channels, attr)
        return self._to_op(m.weight.permute(0, 3, 2, 1).reshape(m.out_channels, k * k * m.in_channels)), f32(m.bias)

    def _pack_resize(self, m, attr, c, src):
        """A level's resize module after its 1x1 projection of c channels (`src` names the projection in a refusal) -> the self.resize entry."""
        if isinstance(m, torch.nn.Identity):
            return ("identity", c)
        if isinstance(m, torch.nn.ConvTranspose2d):
            k = _pair(m.kernel_size)[0]
            if (m.groups != 1 or _pair(m.kernel_size) != (k, k) or _pair(m.stride) != (k, k) or _pair(m.padding) != (0, 0) or _pair(m.output_padding) != (0, 0)
                    or _pair(m.dilation) != (1, 1) or k > 8 or m.in_channels != c):
                self._fail(attr, "served is a ConvTranspose2d with kernel = stride <= 8, no padding, groups = 1")
            self._chan(m.out_channels, attr)
            bias = f32(m.bias) if m.bias is not None else torch.zeros(m.out_channels, dtype=torch.float32, device=m.weight.device)
            # weight [c, n, ky, kx] -> [(ky, kx, n), c]: the GEMM's columns in the order gd_deconv_scatter reads them
            return ("deconv", m.out_channels, k, self._to_op(m.weight.permute(2, 3, 1, 0).reshape(k * k * m.out_channels, c)), bias)
        if isinstance(m, torch.nn.Conv2d):
            if m.in_channels != c:
                self._fail(attr, f"takes {m.in_channels} channels, {src} gives {c}")
            return ("conv_s2", m.out_channels) + self._pack_conv(m, attr, 3, stride=2)
        self._fail(attr, f"is {type(m).__name__}: served are ConvTranspose2d (kernel = stride), Identity and Conv2d(kernel 3, stride 2, padding 1)")

    def _pack_unit(self, u, attr):
        features = self.features
        if getattr(u, "bn", False) or getattr(u, "norm1", None) is not None or getattr(u, "norm2", None) is not None:
            self._fail(f"{attr}.bn", "a batch-norm inside a residual unit is not served")
        if getattr(u, "groups", 1) != 1:
            self._fail(f"{attr}.groups", f"{u.groups}: served is groups = 1")
        act = getattr(u, "activation", None)
        if not isinstance(act, torch.nn.ReLU):
            self._fail(f"{attr}.activation", f"is {type(act).__name__}: served is ReLU")
        p = _Unit()
        p.inplace = bool(act.inplace)
        (p.w1, p.b1), (p.w2, p.b2) = (self._pack_conv(self._need(u, "conv1", attr), f"{attr}.conv1", 3),
                                      self._pack_conv(self._need(u, "conv2", attr), f"{attr}.conv2", 3))
        if not (u.conv1.in_channels == u.conv1.out_channels == u.conv2.in_channels == u.conv2.out_channels == features):
            self._fail(attr, f"its convolutions are not {features} -> {features}")
        return p

    def _pack_fusion(self, blk, attr, has_res, expect_res=None):
        """-> (resConfUnit1 or None, resConfUnit2, out_conv) of one fusion block; has_res: whether resConfUnit1 is read (the block's forward gets a
        skip input); expect_res: what the block's own `has_residual` must say, where the module has such a flag."""
        features = self.features
        for flag in ("deconv", "expand"):
            if getattr(blk, flag, False):
                self._fail(f"{attr}.{flag}", "True: not served")
        if getattr(blk, "align_corners", True) is not True:
            self._fail(f"{attr}.align_corners", f"{blk.align_corners}: gd_grid_resample resamples with align_corners=True")
        if getattr(blk, "groups", 1) != 1:
            self._fail(f"{attr}.groups", f"{blk.groups}: served is groups = 1")
        if getattr(blk, "size", None) is not None:
            self._fail(f"{attr}.size", "a fixed output size is not served")
        if expect_res is not None and has_res != expect_res:
            self._fail(f"{attr}.has_residual", f"{has_res}: the first three blocks take a skip input, the fourth does not")
        oc = self._pack_conv(self._need(blk, "out_conv", attr), f"{attr}.out_conv", 1)
        if blk.out_conv.in_channels != features or blk.out_conv.out_channels != features:
            self._fail(f"{attr}.out_conv", f"is not {features} -> {features}")
        return (self._pack_unit(blk.resConfUnit1, f"{attr}.resConfUnit1") if has_res else None,
                self._pack_unit(self._need(blk, "resConfUnit2", attr), f"{attr}.resConfUnit2"), oc)

    # ---- running ------------------------------------------------------------------------------------------------------------------
    def _op(self, x):
        return x if x.dtype == self.dtype else ops.cast(x, self.dtype)

    def _conv3(self, buf, gh, gw, C, wb, act=0, residual=None, frames=1):
        """3x3 convolution of a stacked operand: -> the pitched fp32 grid [frames*gh*(gw+1), n] (separator rows hold finite values nobody reads)."""
        return ops.gemm_nt(ops.conv_view(buf, frames * gh * (gw + 1), C), wb[0], out_dtype=torch.float32, bias=wb[1], act=act, residual=residual)

    def _stack(self, grid, gh, gw, C, frames=1):
        return ops.stack3_rows(grid, frames, gh, gw, C, gh * (gw + 1) * C, 0, gw + 1, self.dtype)

    def _unit(self, p, x, gh, gw, frames=1):
        """x: the pitched fp32 grid — ALREADY rectified by its producer when p.inplace.  -> skip + conv2(relu(conv1(relu(x))))."""
        C = self.features
        buf = self._stack(x, gh, gw, C, frames) if p.inplace else ops.grid_resample(x, frames, gh, gw, gh, gw, C, relu=True, stacked=self.dtype)
        h = self._conv3(buf, gh, gw, C, (p.w1, p.b1), act=2, frames=frames)
        return self._conv3(self._stack(h, gh, gw, C, frames), gh, gw, C, (p.w2, p.b2), residual=x, frames=frames)

    def _level(self, i, p, gh, gw, frames=1):
        """Level i after its 1x1 projection: p the fp32 token rows [frames*gh*gw, c] -> resize, `layer{i+1}_rn` -> (the pitched grid, its (h, w))."""
        dt = self.dtype
        kind, c = self.resize[i][:2]
        first = self.fusion[i][0] or self.fusion[i][1]        # the unit that reads layer{i+1}_rn's output
        if kind == "deconv":
            _, _, k, wd, bd = self.resize[i]
            grid = ops.deconv_scatter(ops.gemm_nt(self._op(p), wd, out_dtype=torch.float32), bd, frames, gh, gw, gw, k, c)
            h, w = gh * k, gw * k
            buf = ops.stack3_rows(grid, frames, h, w, c, h * (w + 1) * c, 0, w + 1, dt)
        elif kind == "identity":
            h, w = gh, gw
            buf = ops.stack3_rows(p, frames, gh, gw, c, gh * gw * c, 0, gw, dt)
        else:       # kernel 3, stride 2, padding 1: the full-resolution convolution, then every second row and column
            cin = p.shape[1]
            full = self._conv3(ops.stack3_rows(p, frames, gh, gw, cin, gh * gw * cin, 0, gw, dt), gh, gw, cin, self.resize[i][2:], frames=frames)
            h, w = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
            buf = ops.grid_resample(full, frames, gh, gw, h, w, c, step=2, stacked=dt)
        return self._conv3(buf, h, w, c, self.rn[i], act=2 if first.inplace else 0, frames=frames), (h, w)

    def _fuse(self, skips, sizes, frames=1, double=False):
        """refinenet4 .. refinenet1 without the last upsampling: -> (refinenet1's out_conv output on level 0's grid, that grid's (h, w)).
        double=False: a block's output is resampled to the next level's size (the VGGT head passes `size`).  double=True: it is resampled to twice
        its own size and the first rows and columns are kept (the MASt3R adapter: scale_factor 2, then a crop to the next level) — the same single
        pass when the sizes agree; otherwise the doubled grid is written out, cropped, and the addend joins in an identity-size pass."""
        C = self.features
        o, prev = None, None
        for i in (3, 2, 1, 0):
            (h, w), (u1, u2, oc) = sizes[i], self.fusion[i]
            if prev is None:
                x = skips[i]
            else:
                add = self._unit(u1, skips[i], h, w, frames)
                if double and (2 * prev[0], 2 * prev[1]) != (h, w):
                    H2, W2 = 2 * prev[0], 2 * prev[1]
                    if h > H2 or w > W2:
                        raise GdHipError(f"{type(self).__name__}: {self.name}: level {i} is {h} x {w}, more than twice level {i + 1}'s {prev[0]} x {prev[1]}")
                    full = ops.grid_resample(o, frames, prev[0], prev[1], H2, W2, C).view(frames, H2, W2 + 1, C)
                    crop = torch.zeros(frames, h, w + 1, C, dtype=torch.float32, device=full.device)
                    crop[:, :, :w] = full[:, :h, :w]
                    x = ops.grid_resample(crop.view(-1, C), frames, h, w, h, w, C, addend=add, relu=u2.inplace)
                else:
                    x = ops.grid_resample(o, frames, prev[0], prev[1], h, w, C, addend=add, relu=u2.inplace)
            y = self._unit(u2, x, h, w, frames)
            o = ops.gemm_nt(self._op(y), oc[0], out_dtype=torch.float32, bias=oc[1])          # out_conv on the small grid: it commutes with the upsampling
            prev = (h, w)
        return o, prev


class FusedDPTHead(_FusedHead):
    """FusedDPTHead(head, dtype=torch.float32).forward(aggregated_tokens_list, images, patch_start_idx, frames_chunk_size=None): what the module
    returns — (preds [B, S, H, W, output_dim - 1], conf [B, S, H, W]) fp32, or features [B, S, C, H', W'] when `feature_only`.

    dtype: the operand type of the matrix products.  torch.float32: exact operands, the faithful mode (the teacher runs its heads in fp32).
    torch.bfloat16: bf16 operands, fp32 accumulation, fp32 for everything that is added (skips, addends, embeddings): narrower, faster."""

    def __init__(self, head, dtype=torch.float32, name="head"):
        super().__init__(dtype, name)
        fail, need, conv = self._fail, self._need, self._pack_conv
        self.patch = int(need(head, "patch_size"))
        self.layer_idx = [int(i) for i in need(head, "intermediate_layer_idx")]
        self.pos_embed, self.feature_only = bool(need(head, "pos_embed")), bool(need(head, "feature_only"))
        self.down_ratio = need(head, "down_ratio")
        if len(self.layer_idx) != 4:
            fail("intermediate_layer_idx", f"{len(self.layer_idx)} entries: the head fuses four levels")
        if not self.feature_only:
            self.activation, self.conf_activation = need(head, "activation"), need(head, "conf_activation")
            if self.activation not in ops.DPT_ACT:
                fail("activation", f"{self.activation!r}: gd_dpt_head_out serves {sorted(ops.DPT_ACT)}")
            if self.conf_activation not in ops.DPT_CONF_ACT or self.conf_activation == "linear":
                fail("conf_activation", f"{self.conf_activation!r}: gd_dpt_head_out serves ['expp0', 'expp1', 'sigmoid']")
        self.norm = self._r.ln(need(head, "norm"), "norm")
        dim_in = head.norm.normalized_shape[0]
        self._chan(dim_in, "norm")
        projects, resize, scratch = need(head, "projects"), need(head, "resize_layers"), need(head, "scratch")
        if len(projects) != 4 or len(resize) != 4:
            fail("projects", f"{len(projects)} projections / {len(resize)} resize layers: the head fuses four levels")
        self.proj, self.resize = [], []
        for i in range(4):
            w, b = conv(projects[i], f"projects[{i}]", 1)
            if projects[i].in_channels != dim_in:
                fail(f"projects[{i}]", f"takes {projects[i].in_channels} channels, the tokens have {dim_in}")
            self.proj.append((w, b))
            self.resize.append(self._pack_resize(resize[i], f"resize_layers[{i}]", projects[i].out_channels, f"projects[{i}]"))
        self.rn = []
        for i in range(4):
            m = need(scratch, f"layer{i + 1}_rn", "scratch")
            w, b = conv(m, f"scratch.layer{i + 1}_rn", 3)
            if m.in_channels != self.resize[i][1]:
                fail(f"scratch.layer{i + 1}_rn", f"takes {m.in_channels} channels, resize_layers[{i}] gives {self.resize[i][1]}")
            self.rn.append((w, b))
        self.features = features = scratch.layer1_rn.out_channels
        self.fusion = []
        for i in range(4):
            attr = f"scratch.refinenet{i + 1}"
            blk = need(scratch, f"refinenet{i + 1}", "scratch")
            has_res = bool(getattr(blk, "has_residual", hasattr(blk, "resConfUnit1")))
            self.fusion.append(self._pack_fusion(blk, attr, has_res, expect_res=i != 3))
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
            conv(oc2[2], "scratch.output_conv2[2]", 1, any_out=True)
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

    def _frame(self, toks, gh, gw, img_hw, taps, channel_last=False):
        """One frame: toks the four [gh*gw, dim_in] token-row views -> (preds [1, H, W, od-1], conf [1, H, W]) or features [C, H', W']
        (channel_last: the pitched grid itself, [H', W' + 1, C])."""
        dt, C, dev = self.dtype, self.features, toks[0].device
        aspect = img_hw[1] / img_hw[0]
        sizes, skips = [], []
        for i in range(4):
            x = toks[i] if toks[i].dtype in (torch.float32, torch.bfloat16) else toks[i].float()
            y, _, _ = ops.layernorm_fwd(x, *self.norm, save_stats=False, out_dtype=dt)
            w, b = self.proj[i]
            res = self._pos(gw, gh, w.shape[0], aspect, dev)[2] if self.pos_embed else None
            p = ops.gemm_nt(y, w, out_dtype=torch.float32, bias=b, residual=res)                     # token rows [gh*gw, oc]
            skip, size = self._level(i, p, gh, gw)
            skips.append(skip)
            sizes.append(size)
        o, prev = self._fuse(skips, sizes)
        h, w_ = int(prev[0] * 2), int(prev[1] * 2)              # refinenet1 upsamples by scale_factor = 2
        fused = self._conv3(ops.grid_resample(o, 1, prev[0], prev[1], h, w_, C, stacked=dt), h, w_, C, self.out1)
        th, tw = int(gh * self.patch / self.down_ratio), int(gw * self.patch / self.down_ratio)
        C1 = self.c_out1
        px, py = self._pos(tw, th, C1, aspect, dev)[:2] if self.pos_embed else (None, None)
        if self.feature_only:
            if taps is not None:
                taps.setdefault("pre", []).append(fused.view(h, w_ + 1, C1)[:, :w_].permute(2, 0, 1))
            grid = ops.grid_resample(fused, 1, h, w_, th, tw, C1, px=px, py=py).view(th, tw + 1, C1)
            return grid if channel_last else grid[:, :tw].permute(2, 0, 1)
        hid = self._conv3(ops.grid_resample(fused, 1, h, w_, th, tw, C1, px=px, py=py, stacked=dt), th, tw, C1, self.out2, act=2)
        if taps is not None:
            v, c = ops.dpt_head_out(hid, self.w_last, self.b_last, 1, th, tw, "linear", "linear")
            taps.setdefault("pre", []).append(torch.cat([v, c[..., None]], dim=-1)[0].permute(2, 0, 1))
        return ops.dpt_head_out(hid, self.w_last, self.b_last, 1, th, tw, self.activation, self.conf_activation)

    @torch.no_grad()
    def forward(self, aggregated_tokens_list, images, patch_start_idx, frames_chunk_size=None, taps=None, channel_last=False):
        """Same signature and result as the module's forward.  Frames are independent and always run one at a time (at the teacher's size the fp32
        operand of the last convolution is ~410 MB per frame), so `frames_chunk_size` changes neither the result nor the peak memory.
        taps: a dict that receives "pre" — the map before the activations [B*S, output_dim, H, W], or with feature_only the fused map before the
        last resampling (what the tests compare with the reference's).
        channel_last (feature_only heads): -> (features [B, S, H', W', C], pitch): the data columns of the pitched grids [B, S, H', pitch = W' + 1, C]
        the head works on, without the permutation to [B, S, C, H', W'] (what teacher_tracker.FusedTracker takes as `fmaps_cl`)."""
        if channel_last and not self.feature_only:
            raise GdHipError(f"FusedDPTHead: {self.name}: channel_last is served for feature_only heads")
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
                outs.append(self._frame(toks, gh, gw, (H, W), taps, channel_last))
        if taps is not None:
            taps["pre"] = torch.stack(taps["pre"])
        if self.feature_only:
            f = torch.stack(outs)
            if channel_last:
                return f.view(B, S, *f.shape[1:])[:, :, :, :-1], f.shape[2]
            return f.view(B, S, *f.shape[1:])
        preds, conf = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        return preds.view(B, S, *preds.shape[1:]), conf.view(B, S, *conf.shape[1:])

    __call__ = forward


class FusedMASt3RHead(_FusedHead):
    """FusedMASt3RHead(head, dtype=torch.float32)(decout, img_shape): what the user's Cat_MLP_LocalFeatures_DPT_Pts3d returns — the dict pts3d
    [B, H, W, 3], conf [B, H, W] (with has_conf), desc [B, H, W, D], desc_conf [B, H, W], fp32.  decout: the list of encoder / decoder outputs
    [B, gh*gw, C]; the adapter reads decout[hooks[i]], the local-feature MLP cat(decout[0], decout[-1]).  All B frames run together.

    Against the VGGT head: no LayerNorm and no position embedding; `act_postprocess[i]` is a 1x1 convolution followed by the level's resize;
    the residual units rectify out of place; `refinenet4.resConfUnit1` exists but is never used; every fusion block upsamples by scale_factor 2,
    and refinenet4's output is then cropped to the token grid (odd grids: _FusedHead._fuse); the output stage upsamples once more between its two
    3x3 convolutions; the final 1x1 convolution, the MLP's pixel shuffle and the postprocess are gd_mast3r_head_out.

    dtype: as FusedDPTHead's — torch.bfloat16 runs every matrix product, the MLP's included, on bf16 operands with fp32 accumulation."""

    def __init__(self, head, dtype=torch.float32, name="head"):
        super().__init__(dtype, name)
        fail, need, conv = self._fail, self._need, self._pack_conv
        # ---- the postprocess: MASt3R's, recognised by the attributes it reads
        if not need(head, "postprocess"):
            fail("postprocess", "missing: the fused head returns the postprocessed dict (pts3d, conf, desc, desc_conf), not the raw map")
        self.patch, self.D = int(need(head, "patch_size")), int(need(head, "local_feat_dim"))
        self.two_confs = bool(need(head, "two_confs"))
        depth_mode, desc_mode = need(head, "depth_mode"), need(head, "desc_mode")
        conf_mode, desc_conf_mode = need(head, "conf_mode"), need(head, "desc_conf_mode")      # None: no confidence / as conf_mode
        if not (isinstance(depth_mode, (tuple, list)) and len(depth_mode) == 3 and depth_mode[0] in ops.MH_PTS):
            fail("depth_mode", f"{depth_mode!r}: served are (mode, -inf, inf) with mode in {sorted(ops.MH_PTS)}")
        if depth_mode[1] != -float("inf") or depth_mode[2] != float("inf"):
            fail("depth_mode", f"{tuple(depth_mode)!r}: bounded ranges are not served (the module itself asserts there are none)")
        self.pts_mode = depth_mode[0]

        def conf(mode, attr):
            if not (isinstance(mode, (tuple, list)) and len(mode) == 3 and mode[0] in ("exp", "sigmoid")):
                fail(attr, f"{mode!r}: served are ('exp' | 'sigmoid', vmin, vmax)")
            return (mode[0], float(mode[1]), float(mode[2]))
        self.conf_mode = None if conf_mode is None else conf(conf_mode, "conf_mode")
        if not (isinstance(desc_mode, (str, tuple, list)) and "norm" in desc_mode):
            fail("desc_mode", f"{desc_mode!r}: served is 'norm'")
        if not 1 <= self.D <= 32:
            fail("local_feat_dim", f"{self.D}: gd_mast3r_head_out serves 1 .. 32")
        if self.two_confs:
            self.desc_conf_mode = self.conf_mode if desc_conf_mode is None else conf(desc_conf_mode, "desc_conf_mode")
            if self.desc_conf_mode is None:
                fail("desc_conf_mode", "None with conf_mode None: the second confidence has no mode")
        elif self.conf_mode is None:
            fail("two_confs", "False without conf_mode: desc_conf would copy a confidence the head does not have")
        else:
            self.desc_conf_mode = self.conf_mode
        # ---- the DPT adapter
        dpt = need(head, "dpt")
        if getattr(dpt, "head_type", "regression") != "regression":
            fail("dpt.head_type", f"{dpt.head_type!r}: served is 'regression'")
        self.hooks = [int(i) for i in need(dpt, "hooks", "dpt")]
        if len(self.hooks) != 4:
            fail("dpt.hooks", f"{len(self.hooks)} entries: the adapter fuses four levels")
        stride = int(getattr(dpt, "stride_level", 1)) * int(getattr(dpt, "P_H", self.patch))
        if stride != self.patch or int(getattr(dpt, "stride_level", 1)) * int(getattr(dpt, "P_W", self.patch)) != self.patch:
            fail("dpt.P_H", f"the adapter's token stride {stride} is not the head's patch_size {self.patch}")
        post, scratch = need(dpt, "act_postprocess", "dpt"), need(dpt, "scratch", "dpt")
        if len(post) != 4:
            fail("dpt.act_postprocess", f"{len(post)} entries: the adapter fuses four levels")
        self.proj, self.resize = [], []
        for i in range(4):
            attr, seq = f"dpt.act_postprocess[{i}]", post[i]
            if not (isinstance(seq, torch.nn.Sequential) and 1 <= len(seq) <= 2):
                fail(attr, "served is Sequential(Conv2d 1x1[, ConvTranspose2d kernel = stride | Conv2d kernel 3, stride 2, padding 1])")
            self.proj.append(conv(seq[0], f"{attr}[0]", 1))
            self.resize.append(self._pack_resize(seq[1] if len(seq) == 2 else torch.nn.Identity(), f"{attr}[1]", seq[0].out_channels, f"{attr}[0]"))
        self.rn = []
        for i in range(4):
            attr = f"dpt.scratch.layer{i + 1}_rn"
            m = need(scratch, f"layer{i + 1}_rn", "dpt.scratch")
            w, b = conv(m, attr, 3)
            if m.in_channels != self.resize[i][1]:
                fail(attr, f"takes {m.in_channels} channels, dpt.act_postprocess[{i}] gives {self.resize[i][1]}")
            self.rn.append((w, b))
        self.features = features = scratch.layer1_rn.out_channels
        self.fusion = []
        for i in range(4):
            attr = f"dpt.scratch.refinenet{i + 1}"
            blk = need(scratch, f"refinenet{i + 1}", "dpt.scratch")
            if getattr(blk, "width_ratio", 1) != 1:
                fail(f"{attr}.width_ratio", f"{blk.width_ratio}: served is 1")
            # refinenet4 gets one input: its resConfUnit1 exists in the module and is never run
            self.fusion.append(self._pack_fusion(blk, attr, has_res=i != 3))
        seq = need(dpt, "head", "dpt")
        if not (isinstance(seq, torch.nn.Sequential) and len(seq) == 5 and isinstance(seq[3], torch.nn.ReLU) and not isinstance(seq[1], torch.nn.Conv2d)
                and getattr(seq[1], "scale_factor", None) == 2 and getattr(seq[1], "mode", None) == "bilinear" and getattr(seq[1], "align_corners", None) is True):
            fail("dpt.head", "served is Sequential(Conv2d 3x3, Interpolate(scale_factor=2, bilinear, align_corners=True), Conv2d 3x3, ReLU, Conv2d 1x1)")
        self.out1, self.out2 = conv(seq[0], "dpt.head[0]", 3), conv(seq[2], "dpt.head[2]", 3)
        conv(seq[4], "dpt.head[4]", 1, any_out=True)
        if seq[0].in_channels != features or seq[2].in_channels != seq[0].out_channels or seq[4].in_channels != seq[2].out_channels:
            fail("dpt.head", "channel counts do not chain")
        self.c_out1, self.od = seq[0].out_channels, seq[4].out_channels
        if self.od != 3 + (self.conf_mode is not None):
            fail("dpt.head[4]", f"{self.od} output channels with conf_mode {conf_mode!r}: served are 3 (pts3d) without, 4 (pts3d + confidence) with a conf_mode")
        self.w_last = f32(seq[4].weight.reshape(self.od, -1))
        self.b_last = f32(seq[4].bias) if seq[4].bias is not None else torch.zeros(self.od, dtype=torch.float32, device=seq[4].weight.device)
        # ---- the local-feature MLP: fc1 + GELU, fc2 with its rows in the kernel's (i, j, c) order
        mlp = need(head, "head_local_features")
        fc1, fc2, act = need(mlp, "fc1", "head_local_features"), need(mlp, "fc2", "head_local_features"), need(mlp, "act", "head_local_features")
        self._r.exact_gelu(act, "head_local_features.act")
        for m, attr in ((fc1, "head_local_features.fc1"), (fc2, "head_local_features.fc2")):
            if not isinstance(m, torch.nn.Linear):
                fail(attr, f"is {type(m).__name__}, not a Linear")
            self._chan(m.in_features, attr)
        n = self.D + self.two_confs
        if fc2.in_features != fc1.out_features or fc2.out_features != n * self.patch ** 2:
            fail("head_local_features.fc2", f"is {fc2.in_features} -> {fc2.out_features}: expected {fc1.out_features} -> "
                                            f"(local_feat_dim + two_confs) * patch_size^2 = {n * self.patch ** 2}")
        if not 1 <= self.patch <= 16:
            fail("patch_size", f"{self.patch}: gd_mast3r_head_out serves 1 .. 16")
        zeros = lambda m: torch.zeros(m.out_features, dtype=torch.float32, device=m.weight.device)
        self.fc1 = (self._to_op(fc1.weight), f32(fc1.bias) if fc1.bias is not None else zeros(fc1))
        self.fc2 = (self._to_op(pack_pixel_shuffle(fc2.weight.detach(), self.patch)),
                    pack_pixel_shuffle(f32(fc2.bias) if fc2.bias is not None else zeros(fc2), self.patch))

    def _rows(self, t, B, n, what):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.shape[0] == B and t.shape[1] == n):
            raise GdHipError(f"FusedMASt3RHead: {self.name}: {what} {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} does not hold {B} x {n} "
                             f"token rows on the GPU")
        t = t if t.dtype in (torch.float32, torch.bfloat16) else t.float()
        return t.reshape(B * n, t.shape[-1]).contiguous()

    @torch.no_grad()
    def forward(self, decout, img_shape, taps=None):
        """taps: a dict that receives "pre" — the map before the activations [B, od + D + two_confs, H, W] (what the module's `out` is before its
        postprocess)."""
        H, W = int(img_shape[0]), int(img_shape[1])
        gh, gw = H // self.patch, W // self.patch
        B, dt, C = decout[0].shape[0], self.dtype, self.features
        skips, sizes = [], []
        for i in range(4):
            x = self._rows(decout[self.hooks[i]], B, gh * gw, f"decout[{self.hooks[i]}]")
            w, b = self.proj[i]
            skip, size = self._level(i, ops.gemm_nt(self._op(x), w, out_dtype=torch.float32, bias=b), gh, gw, B)
            skips.append(skip)
            sizes.append(size)
        o, (h, w_) = self._fuse(skips, sizes, B, double=True)
        # refinenet1's upsampling, head[0], head[1]'s upsampling, head[2] + ReLU: both upsampled maps leave as stacked operands only
        mid = self._conv3(ops.grid_resample(o, B, h, w_, 2 * h, 2 * w_, C, stacked=dt), 2 * h, 2 * w_, C, self.out1, frames=B)
        th, tw = 4 * h, 4 * w_
        if (th, tw) != (gh * self.patch, gw * self.patch):
            raise GdHipError(f"FusedMASt3RHead: {self.name}: the adapter ends at {th} x {tw}, the patch grid asks for {gh * self.patch} x {gw * self.patch}")
        hid = self._conv3(ops.grid_resample(mid, B, 2 * h, 2 * w_, th, tw, self.c_out1, stacked=dt), th, tw, self.c_out1, self.out2, act=2, frames=B)
        # the local-feature MLP on cat(encoder output, last decoder output), all frames in one GEMM
        cat = torch.cat([self._rows(decout[0], B, gh * gw, "decout[0]").float(), self._rows(decout[-1], B, gh * gw, "decout[-1]").float()], dim=-1)
        hidden = ops.gemm_nt(self._op(cat), self.fc1[0], out_dtype=dt, bias=self.fc1[1], act=1)
        lf = ops.gemm_nt(hidden, self.fc2[0], out_dtype=torch.float32, bias=self.fc2[1])
        kw = dict(patch=self.patch, desc_dim=self.D, two_confs=self.two_confs)
        if taps is not None:
            p, c, d, dc = ops.mast3r_head_out(hid, self.w_last, self.b_last, lf, B, th, tw, desc_mode="raw", **kw)
            parts = [p] + ([c[..., None]] if c is not None else []) + [d] + ([dc[..., None]] if self.two_confs else [])
            taps["pre"] = torch.cat(parts, dim=-1).permute(0, 3, 1, 2)
        p, c, d, dc = ops.mast3r_head_out(hid, self.w_last, self.b_last, lf, B, th, tw, pts_mode=self.pts_mode, conf_mode=self.conf_mode or ("raw", 0.0, 0.0),
                                          desc_mode="norm", desc_conf_mode=self.desc_conf_mode, **kw)
        res = dict(pts3d=p)
        if c is not None:
            res["conf"] = c
        res["desc"], res["desc_conf"] = d, dc
        return res

    __call__ = forward


# ----------------------------------------------------------------------------------------------------------------------------------
# The camera head
# ----------------------------------------------------------------------------------------------------------------------------------
class FusedCameraHead:
    """FusedCameraHead(camera_head)(tokens_list) -> the module's list of [B, S, 9] encodings (vggt/heads/camera_head.py:83-154 CameraHead), on the
    few-row kernels of csrc/rows.hip and gd_layernorm_fwd; `poses(tokens_list, image_hw)` also returns the decoded cameras
    (vggt/utils/pose_enc.py:108-126), written by the last gd_pose_update.

    The head refines M = B * S <= 8 token rows; one call streams every weight `num_iterations` times and is bandwidth-bound.  One iteration is
        rows_linear (embed_pose, K = 9 padded to 12) -> rows_linear (SiLU prologue, poseLN_modulation) -> adaln_modulate
        per trunk block: layernorm -> rows_linear (qkv) -> rows_attention -> rows_linear (proj, gamma, in-place residual)
                         -> layernorm -> rows_linear (fc1, GELU) -> rows_linear (fc2, gamma, in-place residual)
        layernorm (trunk_norm) -> rows_linear (pose_branch.fc1, GELU) -> rows_linear (pose_branch.fc2) -> pose_update
    7 + 7 * depth launches, after one layernorm (token_norm) per call that reads the camera rows tokens[:, :, 0] in place through its row stride.

    dtype: the weight type of the trunk and modulation linears.  torch.float32 is the faithful mode (the reference runs this head in fp32, outside
    autocast); torch.bfloat16 halves the weight stream and is narrower than the reference.  embed_pose and pose_branch stay fp32 in both.

    The module stays the user's: its parameters are read once (duck-typed on the attribute names) and what the kernels do not serve is refused here,
    naming the attribute.  Off by default (teacher_runner.VGGTTeacherRunner(fused_camera_head=True))."""

    def __init__(self, camera_head, dtype=torch.float32, name="camera_head"):
        if dtype not in (torch.float32, torch.bfloat16):
            raise GdHipError(f"FusedCameraHead: dtype {dtype}: torch.float32 or torch.bfloat16")
        self.name, self.dtype, m = name, dtype, camera_head
        r = Reader("FusedCameraHead", name)
        fail, need, ln, linear, no_dropout = r.fail, r.need, r.ln, r.linear, r.no_dropout
        wt = lambda t: t.detach().to(dtype).contiguous()

        def scale(mod, attr, width):
            if isinstance(mod, torch.nn.Identity):
                return None
            g = getattr(mod, "gamma", None)
            if g is None or tuple(g.shape) != (width,):
                fail(attr, f"neither Identity nor a LayerScale with gamma [{width}]")
            return f32(g)

        if int(getattr(m, "target_dim", -1)) != 9:
            fail("target_dim", f"{getattr(m, 'target_dim', None)}: the pose kernel serves the 9-value absT_quaR_FoV encoding")
        self.acts = []
        for a in ("trans_act", "quat_act", "fl_act"):
            v = getattr(m, a, None)
            if v not in ops.POSE_ACTS:
                fail(a, f"{v!r}: known activations are {sorted(ops.POSE_ACTS)}")
            self.acts.append(v)
        embed = need(m, "embed_pose")
        if not isinstance(embed, torch.nn.Linear) or embed.in_features != 9:
            fail("embed_pose", "not a Linear(9 -> dim)")
        D = self.D = embed.out_features
        if D % 8 or D > 2048:
            fail("embed_pose", f"width {D}: a multiple of 8 up to 2048 is served (gd_layernorm_fwd's row limit)")
        # embed_pose's K = 9 padded to 12 with zero columns; the raw encoding is kept as [M, 12] rows with columns 9..11 at 0
        w12 = torch.zeros(D, 12, dtype=torch.float32, device=embed.weight.device)
        w12[:, :9] = embed.weight.detach().float()
        self.embed = (w12, f32(embed.bias))
        ept = need(m, "empty_pose_tokens")
        if ept.numel() != 9:
            fail("empty_pose_tokens", f"{tuple(ept.shape)}: not 9 values")
        self.empty = torch.zeros(1, 12, dtype=torch.float32, device=ept.device)
        self.empty[0, :9] = ept.detach().float().reshape(9)
        mod = need(m, "poseLN_modulation")
        if not (isinstance(mod, torch.nn.Sequential) and len(mod) == 2 and isinstance(mod[0], torch.nn.SiLU)):
            fail("poseLN_modulation", "not Sequential(SiLU, Linear)")
        self.modulation = linear(mod[1], "poseLN_modulation[1]", D, 3 * D, wt)
        an = need(m, "adaln_norm")
        if not isinstance(an, torch.nn.LayerNorm) or an.elementwise_affine or tuple(an.normalized_shape) != (D,):
            fail("adaln_norm", f"not a LayerNorm({D}) without affine parameters")
        self.adaln_eps = float(an.eps)
        self.token_norm = ln(need(m, "token_norm"), "token_norm", D)
        self.trunk_norm = ln(need(m, "trunk_norm"), "trunk_norm", D)
        self.blocks = []
        for i, blk in enumerate(need(m, "trunk")):
            w, wa, wm = f"trunk[{i}]", f"trunk[{i}].attn", f"trunk[{i}].mlp"
            at = need(blk, "attn", w)
            if getattr(at, "rope", None) is not None:
                fail(f"{wa}.rope", "set: gd_rows_attention has no rotary embedding")
            for nm in ("q_norm", "k_norm"):
                if not isinstance(getattr(at, nm, None), torch.nn.Identity):
                    fail(f"{wa}.{nm}", f"{type(getattr(at, nm, None)).__name__}: not Identity (qk_norm is not served)")
            H = int(need(at, "num_heads", wa))
            hd = D // H if H >= 1 and D % H == 0 else 0
            if hd % 4 or not 4 <= hd <= 256:
                fail(f"{wa}.num_heads", f"{H}: head dimension {D / H if H else None}; gd_rows_attention serves multiples of 4 from 4 to 256")
            no_dropout(getattr(at, "attn_drop", None), f"{wa}.attn_drop")
            no_dropout(getattr(at, "proj_drop", None), f"{wa}.proj_drop")
            mlp = need(blk, "mlp", w)
            r.exact_gelu(getattr(mlp, "act", None), f"{wm}.act")
            no_dropout(getattr(mlp, "drop", None), f"{wm}.drop")
            fc1 = linear(need(mlp, "fc1", wm), f"{wm}.fc1", D, None, wt)
            hidden = fc1[0].shape[0]
            if hidden % 8:
                fail(f"{wm}.fc1", f"hidden width {hidden}: a multiple of 8 is served")
            self.blocks.append(dict(H=H, scale=float(getattr(at, "scale", hd ** -0.5)), norm1=ln(need(blk, "norm1", w), f"{w}.norm1", D),
                                    norm2=ln(need(blk, "norm2", w), f"{w}.norm2", D), qkv=linear(need(at, "qkv", wa), f"{wa}.qkv", D, 3 * D, wt),
                                    proj=linear(need(at, "proj", wa), f"{wa}.proj", D, D, wt), fc1=fc1,
                                    fc2=linear(need(mlp, "fc2", wm), f"{wm}.fc2", hidden, D, wt),
                                    ls1=scale(need(blk, "ls1", w), f"{w}.ls1", D), ls2=scale(need(blk, "ls2", w), f"{w}.ls2", D)))
        if not self.blocks:
            fail("trunk", "empty")
        self.hidden = max(b["fc1"][0].shape[0] for b in self.blocks)
        pb = need(m, "pose_branch")
        r.exact_gelu(getattr(pb, "act", None), "pose_branch.act")
        no_dropout(getattr(pb, "drop", None), "pose_branch.drop")
        self.pb1 = linear(need(pb, "fc1", "pose_branch"), "pose_branch.fc1", D)
        self.pbh = self.pb1[0].shape[0]
        if self.pbh % 4:
            fail("pose_branch.fc1", f"hidden width {self.pbh}: a multiple of 4 is served")
        self.pb2 = linear(need(pb, "fc2", "pose_branch"), "pose_branch.fc2", self.pbh, 9)
        self.weight_bytes = sum(t.numel() * t.element_size() for t in self._weights())        # streamed once per iteration
        self._ws, self.launches = {}, 0

    def _weights(self):
        yield from (self.embed[0], self.modulation[0], self.pb1[0], self.pb2[0])
        for b in self.blocks:
            yield from (b["qkv"][0], b["proj"][0], b["fc1"][0], b["fc2"][0])

    def _to(self, device):
        if self.empty.device == device:
            return
        for n in ("embed", "empty", "modulation", "token_norm", "trunk_norm", "pb1", "pb2", "blocks"):
            setattr(self, n, to_device(getattr(self, n), device))
        self._ws = {}

    def _workspace(self, M, device):
        """Allocated once per M and reused: the token stream, the operands between the launches, the raw encoding."""
        ws = self._ws.get(M)
        if ws is None:
            D, e = self.D, lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
            ws = dict(tok=e(M, D), emb=e(M, D), mod=e(M, 3 * D), h=e(M, D), n=e(M, D), qkv=e(M, 3 * D), att=e(M, D), f=e(M, self.hidden), p=e(M, self.pbh),
                      delta=e(M, 12), raw=torch.zeros(M, 12, dtype=torch.float32, device=device), raw0=self.empty.expand(M, 12).contiguous(), plans={})
            self._ws[M] = ws
        return ws

    def _plan(self, ws, B, S, stream):
        """The launches of one iteration between embed_pose and the pose update as (entry point, arguments, name), built once per (B, S, stream): the
        head is ~35 short launches per iteration, and the argument checks of the ops wrappers would cost more host time than the kernels run.  The
        C entry points check every argument again."""
        key = (B, S, stream)
        plan = ws["plans"].get(key)
        if plan is not None:
            return plan
        L, ptr, M, D, F32 = ops.lib(), ops.ptr, B * S, self.D, ops._lib.F32
        tok, emb, mod, h, n, qkv, att, f, p, delta = (ws[k] for k in ("tok", "emb", "mod", "h", "n", "qkv", "att", "f", "p", "delta"))

        def lin(x, wb, y, ldy, res=None, gamma=None, silu=0, gelu=0):
            w, bias = wb
            N, K = w.shape
            return (L.gd_rows_linear, (ptr(x), ptr(w), ops.dtype_code(w), ptr(y), M, N, K, x.stride(0), K, ldy, ptr(bias), ptr(res), ldy if res is not None else 0,
                                       ptr(gamma), silu, gelu, stream), "gd_rows_linear")

        def ln(x, params, y):
            g, b, eps = params
            return (L.gd_layernorm_fwd, (ptr(x), ptr(g), ptr(b), ptr(y), None, None, M, D, D, D, eps, F32, F32, stream), "gd_layernorm_fwd")
        body = [lin(emb, self.modulation, mod, 3 * D, silu=1),
                (L.gd_adaln_modulate, (ptr(tok), ptr(mod), ptr(h), M, D, D, 3 * D, D, self.adaln_eps, stream), "gd_adaln_modulate")]
        for b in self.blocks:
            body += [ln(h, b["norm1"], n), lin(n, b["qkv"], qkv, 3 * D),
                     (L.gd_rows_attention, (ptr(qkv), ptr(att), B, S, b["H"], D // b["H"], 3 * D, D, b["scale"], stream), "gd_rows_attention"),
                     lin(att, b["proj"], h, D, res=h, gamma=b["ls1"]), ln(h, b["norm2"], n), lin(n, b["fc1"], f, self.hidden, gelu=1),
                     lin(f, b["fc2"], h, D, res=h, gamma=b["ls2"])]
        body += [ln(h, self.trunk_norm, n), lin(n, self.pb1, p, self.pbh, gelu=1), lin(p, self.pb2, delta, 12)]
        plan = ws["plans"][key] = dict(first=lin(ws["raw0"], self.embed, emb, D), later=lin(ws["raw"], self.embed, emb, D), body=body)
        return plan

    @torch.no_grad()
    def _run(self, tokens_list, num_iterations, image_hw):
        tokens = tokens_list[-1]
        if not (torch.is_tensor(tokens) and tokens.is_cuda and tokens.dim() == 4 and tokens.shape[-1] == self.D and tokens.dtype in (torch.float32, torch.bfloat16)):
            raise GdHipError(f"FusedCameraHead: {self.name}: tokens_list[-1] must be a CUDA fp32 | bf16 tensor [B, S, P, {self.D}], got "
                             f"{tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens).__name__} {getattr(tokens, 'dtype', None)} on {getattr(tokens, 'device', None)}")
        B, S = tokens.shape[:2]
        M, iters = B * S, int(num_iterations)
        if M > ops.ROWS_MAX_M:
            raise GdHipError(f"FusedCameraHead: {self.name}: B * S = {B} * {S} = {M} camera rows; gd_rows_linear serves up to {ops.ROWS_MAX_M}")
        if M * self.hidden > ops.ROWS_LDS_FLOATS:
            raise GdHipError(f"FusedCameraHead: {self.name}: B * S = {M} rows of the MLP's {self.hidden} hidden columns exceed the {ops.ROWS_LDS_FLOATS} floats "
                             "gd_rows_linear stages")
        if S > 8 or iters < 1:
            raise GdHipError(f"FusedCameraHead: {self.name}: S = {S}, num_iterations = {num_iterations}")
        # the camera rows tokens[:, :, 0], read where they lie: row (b, s) sits b * stride(0) + s * stride(1) in; one row stride must address them all
        ld = tokens.stride(1) if S > 1 else tokens.stride(0)
        if tokens.stride(3) != 1 or (B > 1 and S > 1 and tokens.stride(0) != S * tokens.stride(1)) or ld % 4 or \
                tokens.data_ptr() % 16:
            raise GdHipError(f"FusedCameraHead: {self.name}: tokens_list[-1] with strides {tuple(tokens.stride())}: the camera rows need a contiguous last dim, one "
                             "row stride (a multiple of 4) over (b, s) and a 16-byte aligned start")
        self._to(tokens.device)
        ws, D, stream, L, check = self._workspace(M, tokens.device), self.D, ops.stream(), ops.lib(), ops.check
        plan = self._plan(ws, B, S, stream)
        g, b, eps = self.token_norm
        check(L.gd_layernorm_fwd(tokens.data_ptr(), g.data_ptr(), b.data_ptr(), ws["tok"].data_ptr(), None, None, M, D, ld if M > 1 else D, D, eps,
                                 ops.dtype_code(tokens), ops._lib.F32, stream), "gd_layernorm_fwd")
        self.launches += 1 + iters * (len(plan["body"]) + 2)
        encs, E, K = [], None, None
        for it in range(iters):
            for fn, args, what in (plan["first"] if it == 0 else plan["later"],) + tuple(plan["body"]):
                rc = fn(*args)
                if rc:
                    check(rc, what)
            last = it == iters - 1
            r = ops.pose_update(ws["delta"][:, :9], ws["raw"], it == 0, self.acts, image_hw if last else None)
            if last and image_hw is not None:
                r, E, K = r
                E, K = E.view(B, S, 3, 4), K.view(B, S, 3, 3)
            encs.append(r.view(B, S, 9))
        return encs, E, K

    def forward(self, tokens_list, num_iterations=4):
        return self._run(tokens_list, num_iterations, None)[0]

    def poses(self, tokens_list, image_hw, num_iterations=4):
        """-> (the list of [B, S, 9] encodings, extrinsic [B, S, 3, 4], intrinsic [B, S, 3, 3]) of the last iteration, for an image of (H, W) pixels."""
        return self._run(tokens_list, num_iterations, (int(image_hw[0]), int(image_hw[1])))

    __call__ = forward
