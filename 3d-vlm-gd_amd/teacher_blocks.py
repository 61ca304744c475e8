"""The two frozen teachers' transformer stacks on the HIP kernels instead of the user's PyTorch modules: the VGGT aggregator
(FusedAggregatorBlocks, below), the DINOv2 patch embedder inside it (FusedDinoEmbed, after it) and the MASt3R / CroCo encoder and two-sided
decoder (FusedCroCoBlocks, at the end).

The VGGT teacher's alternating-attention stack (vggt/models/aggregator.py:246-275: `aa_block_size` frame blocks on [B*S, P], then
`aa_block_size` global blocks on [B, S*P], `depth / aa_block_size` times) on the HIP kernels instead of the user's PyTorch modules.

One block (vggt/layers/block.py:81-134 eval path, vggt/layers/attention.py:51-71) runs as
    layernorm_fwd -> gemm_nt(+bias) -> qk_norm_rope -> attention_fwd -> gemm_nt(+bias, +residual) ->
    layernorm_fwd -> gemm_nt(+bias, GELU) -> gemm_nt(+bias, +residual)
and the frame and global kinds differ only in the (B, N) handed to qk_norm_rope / attention_fwd: the token buffer is the same.  The
cross-view distillation target is accumulated by gd_cross_view_attn from the q / k that qk_norm_rope hands out for the last global block of
each selected iteration: no hooks, no [2B, H, n, n] maps, no placeholder.

The modules stay the user's: this class reads their parameters (duck-typed on the attribute names, as teacher_runner.QKCapture does) and
refuses, with the block's name, anything the kernels do not serve.  Off by default (teacher_runner.VGGTTeacherRunner(fused_blocks=True))."""
import torch

from . import ops
from . import teacher_glue as tg
from ._lib import GdHipError


def fold_layer_scale(linear, ls):
    """LayerScale after a frozen Linear, ls(linear(x)) = gamma * (W x + b), as one Linear: W' = diag(gamma) W, b' = gamma * b.
    `ls`: a module with a `gamma` vector (vggt/layers/layer_scale.py) or nn.Identity / None.  -> (W', b' or None), detached; the
    module's own tensors when there is nothing to fold."""
    W = linear.weight.detach()
    b = linear.bias.detach() if linear.bias is not None else None
    gamma = getattr(ls, "gamma", None)
    if gamma is None:
        return W, b
    g = gamma.detach().to(W.dtype)
    return g[:, None] * W, (g * b if b is not None else None)


class _BlockParams:
    """One block's tensors in the form the kernels take: matrices in the operand dtype, vectors in fp32."""

    def __init__(self, blk, name, dtype, who="FusedAggregatorBlocks", rotary=True):
        """rotary=False (the DINOv2 embedder's blocks): no q/k norm and no RoPE between the QKV GEMM and attention, so both must be absent."""
        def need(obj, attr, where):
            if not hasattr(obj, attr):
                raise GdHipError(f"{who}: {name}: {where} has no `{attr}`")
            return getattr(obj, attr)
        attn, mlp = need(blk, "attn", "the block"), need(blk, "mlp", "the block")
        H = int(need(attn, "num_heads", "attn"))
        C = need(attn, "qkv", "attn").weight.shape[1]
        if C % H or C // H != 64:
            raise GdHipError(f"{who}: {name}: head dim {C / H:g} (width {C}, {H} heads): the attention kernels serve head dim 64")
        scale = float(getattr(attn, "scale", 64 ** -0.5))
        if abs(scale - 64 ** -0.5) > 1e-9:
            raise GdHipError(f"{who}: {name}: attn.scale {scale} is not 64^-0.5")
        qn, kn = need(attn, "q_norm", "attn"), need(attn, "k_norm", "attn")
        ln = [isinstance(m, torch.nn.LayerNorm) and m.elementwise_affine and tuple(m.normalized_shape) == (64,) for m in (qn, kn)]
        ident = [isinstance(m, torch.nn.Identity) for m in (qn, kn)]
        if not rotary and not all(ident):
            raise GdHipError(f"{who}: {name}: attn.q_norm / attn.k_norm are {type(qn).__name__} / {type(kn).__name__}: served is Identity on both")
        if not (all(ln) or all(ident)):
            raise GdHipError(f"{who}: {name}: q_norm / k_norm are {type(qn).__name__} / {type(kn).__name__}: served are "
                             "LayerNorm(64) with affine on both, or Identity on both")
        if all(ln) and qn.eps != kn.eps:
            raise GdHipError(f"{who}: {name}: q_norm and k_norm differ in eps")
        rope = getattr(attn, "rope", None)
        if rotary and rope is None:
            raise GdHipError(f"{who}: {name}: attn.rope is None: the fused q/k step always rotates")
        if not rotary and rope is not None:
            raise GdHipError(f"{who}: {name}: attn.rope is {type(rope).__name__}: these blocks run without a rotary step")
        act = getattr(mlp, "act", None)           # vggt/layers/mlp.py: act_layer(); a layout without the attribute calls F.gelu itself
        if act is not None and not (isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"):
            raise GdHipError(f"{who}: {name}: mlp.act is {act}: the GEMM epilogue serves exact (erf) GELU")
        for nm in ("norm1", "norm2"):
            m = need(blk, nm, "the block")
            if not (isinstance(m, torch.nn.LayerNorm) and m.elementwise_affine and tuple(m.normalized_shape) == (C,)):
                raise GdHipError(f"{who}: {name}: {nm} is not an affine LayerNorm({C})")
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        op = lambda t: t.detach().to(dtype).contiguous()
        self.H, self.C = H, C
        self.base = float(getattr(rope, "base_frequency", getattr(rope, "base", 100.0)))
        self.n1 = (f32(blk.norm1.weight), f32(blk.norm1.bias), float(blk.norm1.eps))
        self.n2 = (f32(blk.norm2.weight), f32(blk.norm2.bias), float(blk.norm2.eps))
        self.wqkv, self.bqkv = op(attn.qkv.weight), f32(attn.qkv.bias)
        self.qk = (f32(qn.weight), f32(qn.bias), f32(kn.weight), f32(kn.bias)) if all(ln) else (None, None, None, None)
        self.qk_eps = float(qn.eps) if all(ln) else 0.0
        wp, bp = fold_layer_scale(need(attn, "proj", "attn"), getattr(blk, "ls1", None))
        self.wproj, self.bproj = op(wp), f32(bp)
        self.w1, self.b1 = op(need(mlp, "fc1", "mlp").weight), f32(mlp.fc1.bias)
        w2, b2 = fold_layer_scale(need(mlp, "fc2", "mlp"), getattr(blk, "ls2", None))
        self.w2, self.b2 = op(w2), f32(b2)


class FusedAggregatorBlocks:
    """FusedAggregatorBlocks(aggregator, dtype=torch.bfloat16).forward(tokens, pos, B, S) -> (outputs, maps).

    dtype: the operand type of the matrix products and of attention.  torch.bfloat16: bf16 operands, fp32 accumulation, and the residual
    stream kept in fp32 (as autocast keeps it): LayerNorm reads fp32 and writes the bf16 operand, the proj / fc2 GEMMs add the fp32
    residual and write fp32.  torch.float32: everything exact fp32, the parity mode."""

    def __init__(self, aggregator, dtype=torch.bfloat16):
        if dtype not in (torch.float32, torch.bfloat16):
            raise GdHipError("FusedAggregatorBlocks: dtype must be torch.float32 or torch.bfloat16")
        for a in ("frame_blocks", "global_blocks", "patch_start_idx"):
            if not hasattr(aggregator, a):
                raise GdHipError(f"FusedAggregatorBlocks: the aggregator has no `{a}`")
        order = list(getattr(aggregator, "aa_order", ["frame", "global"]))
        if order != ["frame", "global"]:
            raise GdHipError(f"FusedAggregatorBlocks: aa_order {order}: served is ['frame', 'global']")
        self.dtype = dtype
        self.per = int(getattr(aggregator, "aa_block_size", 1))
        depth = len(aggregator.frame_blocks)
        if len(aggregator.global_blocks) != depth or depth % self.per:
            raise GdHipError(f"FusedAggregatorBlocks: {depth} frame / {len(aggregator.global_blocks)} global blocks do not pair up in groups of {self.per}")
        # aggregator.py:255-260 keeps the map of iteration i `if i in self.attn_indices`: an index past the last iteration never matches
        self.attn_indices = sorted({int(i) for i in (getattr(aggregator, "attn_indices", None) or []) if 0 <= int(i) < depth // self.per})
        self.temperature = float(getattr(aggregator, "temperature", 1.0))
        self.prefix = int(aggregator.patch_start_idx)
        self.frame = [_BlockParams(b, f"frame_blocks[{i}]", dtype) for i, b in enumerate(aggregator.frame_blocks)]
        self.glob = [_BlockParams(b, f"global_blocks[{i}]", dtype) for i, b in enumerate(aggregator.global_blocks)]

    def _block(self, p, x, pos, B, N, want_qk=False):
        """x [B*N, C] fp32 residual stream -> (x after the block, (q, k) or None)."""
        dt = self.dtype
        y, _, _ = ops.layernorm_fwd(x, p.n1[0], p.n1[1], p.n1[2], save_stats=False, out_dtype=dt)
        qkv = ops.gemm_nt(y, p.wqkv, bias=p.bqkv)
        qk = ops.qk_norm_rope(qkv, B, N, p.H, pos, *p.qk, p.qk_eps, p.base, want_qk=want_qk)
        o, _ = ops.attention_fwd(qkv, B, N, p.H)
        x = ops.gemm_nt(o, p.wproj, out_dtype=torch.float32, bias=p.bproj, residual=x)
        y, _, _ = ops.layernorm_fwd(x, p.n2[0], p.n2[1], p.n2[2], save_stats=False, out_dtype=dt)
        h = ops.gemm_nt(y, p.w1, bias=p.b1, act=1)
        return ops.gemm_nt(h, p.w2, out_dtype=torch.float32, bias=p.b2, residual=x), qk

    @torch.no_grad()
    def forward(self, tokens, pos, B, S):
        """tokens [B*S, P, C], pos [B*S, P, 2] (y, x; the prefix tokens at 0) -> (outputs, maps): `outputs` the reference's list of
        [B, S, P, 2C] fp32 tensors (frame | global, one per block pair), `maps` [2B, n, n] fp32 the head- and block-averaged cross-view
        target (None when the aggregator selects no block)."""
        BS, P, C = tokens.shape
        if BS != B * S or tuple(pos.shape) != (BS, P, 2) or C != self.frame[0].C:
            raise GdHipError(f"FusedAggregatorBlocks: tokens {tuple(tokens.shape)} / pos {tuple(pos.shape)} do not fit B={B}, S={S}, width {self.frame[0].C}")
        sel = {i * self.per + self.per - 1 for i in self.attn_indices}       # the LAST global block of a selected iteration (aggregator.py:255-260)
        if sel and (S * P) % 2:
            raise GdHipError(f"FusedAggregatorBlocks: global_blocks[{min(sel)}]: odd global token count {S * P}: the cross-view maps need two views of equal length")
        x = tokens.detach().reshape(BS * P, C).float().contiguous()
        pos = pos.to(x.device).reshape(BS * P, 2).long().contiguous()
        outputs, maps, nsel = [], None, 0
        for it in range(len(self.frame) // self.per):
            inter = []
            for j in range(it * self.per, (it + 1) * self.per):
                x, _ = self._block(self.frame[j], x, pos, BS, P)
                inter.append(x)
            for k, j in enumerate(range(it * self.per, (it + 1) * self.per)):
                x, qk = self._block(self.glob[j], x, pos, B, S * P, want_qk=j in sel)
                if qk is not None:
                    maps = tg.cross_view_attention_maps(qk[0], qk[1], 64 ** -0.5, self.temperature, self.prefix, out=maps,
                                                        weight=1.0 / (self.glob[j].H * len(sel)), accumulate=nsel > 0)
                    nsel += 1
                outputs.append(torch.cat([inter[k].view(B, S, P, C), x.view(B, S, P, C)], dim=-1))
        return outputs, maps


# ----------------------------------------------------------------------------------------------------------------------------------
# The VGGT aggregator's DINOv2 patch embedder (vggt/layers/vision_transformer.py; vggt/models/aggregator.py:151-186, 206-242)
# ----------------------------------------------------------------------------------------------------------------------------------
class FusedDinoEmbed:
    """FusedDinoEmbed(embedder, dtype=torch.bfloat16, name="aggregator.patch_embed"): the aggregator's `patch_embed` when it is a DINOv2 ViT
    (`dinov2_vitl14_reg`: 24 blocks of width 1024 on 1 + 4 + gh * gw tokens per frame) on the HIP kernels.  The module stays the user's: its
    parameters are read once, here (duck-typed on the reference's attribute names), and anything the kernels do not serve is refused naming
    the attribute.

    One block runs as layernorm_fwd -> gemm_nt(+bias) -> attention_fwd -> gemm_nt(+bias, +residual) -> layernorm_fwd -> gemm_nt(+bias, GELU) ->
    gemm_nt(+bias, +residual): no q/k norm and no rotary step, LayerScale folded into proj / fc2, the residual stream in fp32.  The ends are
    gd_patch_im2col (normalisation fused) + the patch GEMM + gd_dino_assemble_tokens, and the final norm (gd_layernorm_fwd for `forward`, fused
    with the aggregator's token and position assembly in gd_vggt_tokens_from_dino for `aggregator_tokens`).

    dtype as FusedAggregatorBlocks: torch.bfloat16 = bf16 operands, fp32 accumulation; torch.float32 = exact fp32, the parity mode.

    The position table at the table's own square grid is `pos_embed`; for any other (H, W) the module's own `interpolate_pos_encoding` runs
    once on a shape-only stand-in and its fp32 result is cached per (H, W) (as vit.GDViT does for a foreign resampler): the bicubic /
    antialias / offset arithmetic stays the user's, exactly."""

    WHO = "FusedDinoEmbed"

    def __init__(self, embedder, dtype=torch.bfloat16, name="aggregator.patch_embed"):
        who = self.WHO
        if dtype not in (torch.float32, torch.bfloat16):
            raise GdHipError(f"{who}: dtype must be torch.float32 or torch.bfloat16")

        def need(obj, attr, where):
            if not hasattr(obj, attr):
                raise GdHipError(f"{who}: {where} has no `{attr}`")
            return getattr(obj, attr)
        blocks = getattr(embedder, "blocks", None)
        if blocks is None:
            raise GdHipError(f"{who}: {name} has no `blocks` (the 'conv' patch embedder is one convolution: leave fused_patch_embed off)")
        if getattr(embedder, "chunked_blocks", False):
            raise GdHipError(f"{who}: {name}.chunked_blocks is true: served is a flat block list (block_chunks=0)")
        pos_embed = need(embedder, "pos_embed", name)
        D = int(pos_embed.shape[-1])
        if D % 8 or D > 2048:
            raise GdHipError(f"{who}: {name}.pos_embed has width {D}: served is a multiple of 8 up to 2048")
        P = need(embedder, "patch_size", name)
        P = int(P[0] if isinstance(P, (tuple, list)) else P)
        proj = need(need(embedder, "patch_embed", name), "proj", f"{name}.patch_embed")
        if not (isinstance(proj, torch.nn.Conv2d) and tuple(proj.kernel_size) == (P, P) and tuple(proj.stride) == (P, P) and
                tuple(proj.padding) == (0, 0) and tuple(proj.dilation) == (1, 1) and proj.groups == 1 and proj.in_channels == 3 and
                proj.out_channels == D):
            raise GdHipError(f"{who}: {name}.patch_embed.proj is {proj}: served is Conv2d(3, {D}, kernel_size={P}, stride={P})")
        if not isinstance(getattr(embedder.patch_embed, "norm", None), (torch.nn.Identity, type(None))):
            raise GdHipError(f"{who}: {name}.patch_embed.norm is {type(embedder.patch_embed.norm).__name__}: served is Identity")
        R = int(need(embedder, "num_register_tokens", name))
        reg = getattr(embedder, "register_tokens", None)
        if (0 if reg is None else int(reg.shape[-2])) != R or (reg is not None and int(reg.shape[-1]) != D):
            raise GdHipError(f"{who}: {name}.register_tokens {None if reg is None else tuple(reg.shape)} disagrees with num_register_tokens = {R} at width {D}")
        cls = need(embedder, "cls_token", name)
        if cls.numel() != D:
            raise GdHipError(f"{who}: {name}.cls_token {tuple(cls.shape)} is not one token of width {D}")
        if not callable(getattr(embedder, "interpolate_pos_encoding", None)):
            raise GdHipError(f"{who}: {name} has no `interpolate_pos_encoding`")
        norm = need(embedder, "norm", name)
        if not (isinstance(norm, torch.nn.LayerNorm) and norm.elementwise_affine and tuple(norm.normalized_shape) == (D,)):
            raise GdHipError(f"{who}: {name}.norm is not an affine LayerNorm({D})")
        self.blocks = [_BlockParams(b, f"{name}.blocks[{i}]", dtype, who=who, rotary=False) for i, b in enumerate(blocks)]
        for i, p in enumerate(self.blocks):
            if p.C != D:
                raise GdHipError(f"{who}: {name}.blocks[{i}]: width {p.C} is not the embedder's {D}")
        f32 = lambda t: t.detach().float().contiguous()
        self.embedder, self.name, self.dtype, self.D, self.P, self.R = embedder, name, dtype, D, P, R
        K = 3 * P * P
        self.Kp = (K + 63) // 64 * 64                                 # the patch convolution as a [D, Kp] matrix (vit.GDViT._patch_plan)
        wp = torch.zeros(D, self.Kp, dtype=torch.float32, device=proj.weight.device)
        wp[:, :K] = proj.weight.detach().float().reshape(D, K)
        self.wpe, self.bpe = wp.to(dtype).contiguous(), None if proj.bias is None else f32(proj.bias)
        self.cls = f32(cls).reshape(D)
        self.reg = None if reg is None else f32(reg).reshape(R, D)
        self.norm = (f32(norm.weight), f32(norm.bias), float(norm.eps))
        self._pos_cache, self._agg_norm = {}, None

    # -- pieces ---------------------------------------------------------------------------------------------------------------------
    def _pos(self, H, W, gh, gw):
        """fp32 [1 + gh * gw, D]: `pos_embed` at its own square grid, else the module's own resampling (called as the module calls it: (tokens, w, h)
        with w the image's FIRST spatial extent), once per (H, W)."""
        key = (H, W)
        if key not in self._pos_cache:
            pe = self.embedder.pos_embed
            if not (gh * gw == pe.shape[1] - 1 and H == W):
                with torch.no_grad():
                    pe = self.embedder.interpolate_pos_encoding(torch.empty(1, 1 + gh * gw, self.D, device=pe.device, dtype=torch.float32), H, W)
            if tuple(pe.shape) != (1, 1 + gh * gw, self.D):
                raise GdHipError(f"{self.WHO}: {self.name}.interpolate_pos_encoding returned {tuple(pe.shape)}, expected {(1, 1 + gh * gw, self.D)}")
            self._pos_cache[key] = pe.detach().float()[0].contiguous()
        return self._pos_cache[key]

    def _block(self, p, x, B, N):
        """x [B*N, D] fp32 residual stream -> the same after one block (attention_fwd reads the packed qkv as the GEMM wrote it)."""
        dt = self.dtype
        y, _, _ = ops.layernorm_fwd(x, p.n1[0], p.n1[1], p.n1[2], save_stats=False, out_dtype=dt)
        qkv = ops.gemm_nt(y, p.wqkv, bias=p.bqkv)
        o, _ = ops.attention_fwd(qkv, B, N, p.H)
        x = ops.gemm_nt(o, p.wproj, out_dtype=torch.float32, bias=p.bproj, residual=x)
        y, _, _ = ops.layernorm_fwd(x, p.n2[0], p.n2[1], p.n2[2], save_stats=False, out_dtype=dt)
        h = ops.gemm_nt(y, p.w1, bias=p.b1, act=1)
        return ops.gemm_nt(h, p.w2, out_dtype=torch.float32, bias=p.b2, residual=x)

    def _grid(self, H, W):
        if H % self.P or W % self.P or H < self.P or W < self.P:
            raise GdHipError(f"{self.WHO}: {self.name}: image {H} x {W} is not a multiple of patch_size = {self.P}")
        return H // self.P, W // self.P

    # -- entry points -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def features(self, img, mean=None, std=None):
        """img [BS, 3, H, W] fp32 -> the residual stream after the last block, fp32 [BS, 1 + R + Np, D] (`x_prenorm`).  With `mean` and `std`
        (three floats each) the image is in [0, 1] and is normalised inside gd_patch_im2col; without them it is already normalised."""
        if img.dim() != 4 or img.shape[1] != 3:
            raise GdHipError(f"{self.WHO}: {self.name}: images {tuple(img.shape)}, expected [BS, 3, H, W]")
        if (mean is None) != (std is None):
            raise GdHipError(f"{self.WHO}: {self.name}: pass both mean and std or neither")
        BS, _, H, W = img.shape
        gh, gw = self._grid(H, W)
        Np, Nt = gh * gw, 1 + self.R + gh * gw
        col = ops.patch_im2col(img, H, W, self.P, self.Kp, (0.0, 0.0, 0.0) if mean is None else mean, (1.0, 1.0, 1.0) if std is None else std, self.dtype)
        tok = ops.gemm_nt(col, self.wpe, bias=self.bpe)
        x = ops.dino_assemble_tokens(tok, self.cls, self.reg, self._pos(H, W, gh, gw), BS, Np).view(BS * Nt, self.D)
        for p in self.blocks:
            x = self._block(p, x, BS, Nt)
        return x.view(BS, Nt, self.D)

    @torch.no_grad()
    def forward(self, img, masks=None):
        """The module's `forward` (forward_features, vision_transformer.py:262-281) on an already normalised image: its dict, for shadowing."""
        if masks is not None:
            raise GdHipError(f"{self.WHO}: {self.name}: masks are not served")
        x = self.features(img)
        BS, Nt, D = x.shape
        xn = ops.layernorm_fwd(x.view(BS * Nt, D), *self.norm, save_stats=False, out_dtype=torch.float32)[0].view(BS, Nt, D)
        return {"x_norm_clstoken": xn[:, 0], "x_norm_regtokens": xn[:, 1:self.R + 1], "x_norm_patchtokens": xn[:, self.R + 1:], "x_prenorm": x,
                "masks": None}

    def check_aggregator(self, aggregator):
        """-> (camera [2, D], regs [2, Rg, D] or None, prefix) of an aggregator this embedder can feed; refuses, naming the attribute, otherwise."""
        who = self.WHO
        for a in ("camera_token", "register_token", "patch_start_idx", "_resnet_mean", "_resnet_std"):
            if not hasattr(aggregator, a):
                raise GdHipError(f"{who}: the aggregator has no `{a}`")
        prefix = int(aggregator.patch_start_idx)
        if prefix < 1:
            raise GdHipError(f"{who}: aggregator.patch_start_idx = {prefix}: served is a camera token (and registers) in front of the patches")
        cam, reg = aggregator.camera_token, aggregator.register_token
        if cam.shape[-1] != self.D or tuple(cam.shape[:3]) != (1, 2, 1):
            raise GdHipError(f"{who}: aggregator.camera_token {tuple(cam.shape)}: the embedder's width is {self.D} (expected [1, 2, 1, {self.D}])")
        if tuple(reg.shape) != (1, 2, prefix - 1, self.D):
            raise GdHipError(f"{who}: aggregator.register_token {tuple(reg.shape)} does not fit patch_start_idx = {prefix} at width {self.D}")
        f32 = lambda t: t.detach().float().contiguous()
        return f32(cam).reshape(2, self.D), (f32(reg).reshape(2, prefix - 1, self.D) if prefix > 1 else None), prefix

    @torch.no_grad()
    def aggregator_tokens(self, images, aggregator):
        """images [B, S, 3, H, W] in [0, 1] -> (tokens fp32 [B*S, P, D], pos int64 [B*S, P, 2]): what the aggregator hands its first frame block
        (aggregator.py:206-242: normalisation, the embedder, its final norm on the patch rows, camera / register tokens, the position grid),
        without the module."""
        camera, regs, _ = self.check_aggregator(aggregator)
        if images.dim() != 5 or images.shape[2] != 3:
            raise GdHipError(f"{self.WHO}: images {tuple(images.shape)}, expected [B, S, 3, H, W]")
        B, S, _, H, W = images.shape
        gh, gw = self._grid(H, W)
        if self._agg_norm is None or self._agg_norm[0] is not aggregator:
            self._agg_norm = (aggregator, [float(v) for v in aggregator._resnet_mean.flatten().tolist()],
                              [float(v) for v in aggregator._resnet_std.flatten().tolist()])
        x = self.features(images.reshape(B * S, 3, H, W), self._agg_norm[1], self._agg_norm[2])
        return ops.vggt_tokens_from_dino(x, *self.norm, camera, regs, B, S, gh, gw, self.R)


# ----------------------------------------------------------------------------------------------------------------------------------
# MASt3R / CroCo: encoder blocks (dust3r/croco/models/blocks.py:115-131) and decoder blocks with cross-attention (blocks.py:133-195)
# ----------------------------------------------------------------------------------------------------------------------------------
_WHO = "FusedCroCoBlocks"


def _need(obj, attr, name, where):
    if not hasattr(obj, attr):
        raise GdHipError(f"{_WHO}: {name}: {where} has no `{attr}`")
    return getattr(obj, attr)


def _affine_ln(m, C, name, nm):
    if not (isinstance(m, torch.nn.LayerNorm) and m.elementwise_affine and tuple(m.normalized_shape) == (C,)):
        raise GdHipError(f"{_WHO}: {name}: {nm} is not an affine LayerNorm({C})")
    return m.weight.detach().float().contiguous(), m.bias.detach().float().contiguous(), float(m.eps)


def _heads_scale_rope(attn, C, name, what):
    """-> (H, rope base) of an attention module the kernels serve: head dim 64, scale 64^-0.5, a RoPE module."""
    H = int(_need(attn, "num_heads", name, what))
    if C % H or C // H != 64:
        raise GdHipError(f"{_WHO}: {name}: {what}: head dim {C / H:g} (width {C}, {H} heads): the attention kernels serve head dim 64")
    scale = float(getattr(attn, "scale", 64 ** -0.5))
    if abs(scale - 64 ** -0.5) > 1e-9:
        raise GdHipError(f"{_WHO}: {name}: {what}.scale {scale} is not 64^-0.5")
    rope = getattr(attn, "rope", None)
    if rope is None:
        raise GdHipError(f"{_WHO}: {name}: {what}.rope is None: the fused q / k step always rotates")
    return H, float(getattr(rope, "base_frequency", getattr(rope, "base", 100.0)))


class _CroCoBlockParams:
    """One CroCo block's tensors in the form the kernels take (matrices in the operand dtype, vectors in fp32).  `decoder`: the block also
    has `cross_attn` (projq / projk / projv / proj), `norm_y` (LayerNorm, or Identity with norm_mem=False) and `norm3`."""

    def __init__(self, blk, name, dtype, decoder):
        attn, mlp = _need(blk, "attn", name, "the block"), _need(blk, "mlp", name, "the block")
        C = _need(attn, "qkv", name, "attn").weight.shape[1]
        self.C = C
        self.H, self.base = _heads_scale_rope(attn, C, name, "attn")
        act = getattr(mlp, "act", None)
        if act is not None and not (isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"):
            raise GdHipError(f"{_WHO}: {name}: mlp.act is {act}: the GEMM epilogue serves exact (erf) GELU")
        f32 = lambda t: None if t is None else t.detach().float().contiguous()
        op = lambda t: t.detach().to(dtype).contiguous()
        self.n1 = _affine_ln(_need(blk, "norm1", name, "the block"), C, name, "norm1")
        self.nmlp = _affine_ln(_need(blk, "norm3" if decoder else "norm2", name, "the block"), C, name, "norm3" if decoder else "norm2")
        self.wqkv, self.bqkv = op(attn.qkv.weight), f32(attn.qkv.bias)
        proj = _need(attn, "proj", name, "attn")
        self.wproj, self.bproj = op(proj.weight), f32(proj.bias)
        self.w1, self.b1 = op(_need(mlp, "fc1", name, "mlp").weight), f32(mlp.fc1.bias)
        self.w2, self.b2 = op(_need(mlp, "fc2", name, "mlp").weight), f32(mlp.fc2.bias)
        if not decoder:
            return
        ca = _need(blk, "cross_attn", name, "the block")
        pq, pk, pv, po = (_need(ca, a, name, "cross_attn") for a in ("projq", "projk", "projv", "proj"))
        Hc, base_c = _heads_scale_rope(ca, C, name, "cross_attn")
        if (Hc, base_c) != (self.H, self.base):
            raise GdHipError(f"{_WHO}: {name}: attn and cross_attn differ in heads / RoPE base ({self.H}, {self.base:g} against {Hc}, {base_c:g})")
        if (pk.bias is None) != (pv.bias is None):
            raise GdHipError(f"{_WHO}: {name}: cross_attn.projk and projv differ in having a bias")
        self.n2 = _affine_ln(_need(blk, "norm2", name, "the block"), C, name, "norm2")
        ny = _need(blk, "norm_y", name, "the block")
        self.ny = None if isinstance(ny, torch.nn.Identity) else _affine_ln(ny, C, name, "norm_y")
        self.wq, self.bq = op(pq.weight), f32(pq.bias)
        # k and v projections of the other view's tokens as ONE GEMM: kv [M, 2C] = [projk | projv], the layout gd_cross_attention_fwd reads
        self.wkv = op(torch.cat([pk.weight.detach(), pv.weight.detach()], dim=0))
        self.bkv = None if pk.bias is None else f32(torch.cat([pk.bias.detach(), pv.bias.detach()]))
        self.wcproj, self.bcproj = op(po.weight), f32(po.bias)


class FusedCroCoBlocks:
    """FusedCroCoBlocks(matcher, dtype=torch.float32): the MASt3R teacher's 24 encoder blocks and 12 + 12 decoder blocks (AsymmetricCroCo3DStereo:
    `enc_blocks`, `decoder_embed`, `dec_blocks`, `dec_blocks2`, `dec_norm`) on the HIP kernels.  The modules stay the user's: their parameters
    are read once, here (duck-typed on the attribute names), and anything the kernels do not serve is refused with the block's name.

    dtype: torch.float32 — everything exact fp32, the parity mode and the faithful one (the reference runs this teacher in fp32 with TF32
    matmuls, dust3r/croco/models/croco.py:12); torch.bfloat16 — bf16 operands, fp32 accumulation, fp32 residual stream: narrower, faster.

    `encode(x, pos)` runs all encoder blocks; `decode(f1, pos1, f2, pos2)` is `_decoder` (dust3r/dust3r/model.py:297-322) with ONE
    difference in what it returns: the per-layer cross-attention score maps leave as one-head HEAD MEANS [B, 1, Nq, Nk] fp32,
    (scale / H) * Q K^T over the concatenated heads, taken by one batched GEMM straight off the rotated q and k buffers — never as
    [B, H, Nq, Nk] per-head tensors.  Both consumers reduce the maps with .mean(dim=1) first (model.py:347-356, both `reciprocity`
    branches; teacher_glue.mast3r_recip_logits), which leaves a one-head tensor unchanged, so the user's `forward` and the runner's
    keep_logits path work on them as they are."""

    def __init__(self, matcher, dtype=torch.float32):
        if dtype not in (torch.float32, torch.bfloat16):
            raise GdHipError(f"{_WHO}: dtype must be torch.float32 or torch.bfloat16")
        for a in ("enc_blocks", "decoder_embed", "dec_blocks", "dec_blocks2", "dec_norm"):
            if not hasattr(matcher, a):
                raise GdHipError(f"{_WHO}: the matcher has no `{a}`")
        if len(matcher.dec_blocks) != len(matcher.dec_blocks2):
            raise GdHipError(f"{_WHO}: dec_blocks ({len(matcher.dec_blocks)}) and dec_blocks2 ({len(matcher.dec_blocks2)}) differ in length")
        if len(matcher.dec_blocks) == 0:
            raise GdHipError(f"{_WHO}: dec_blocks is empty")
        self.dtype = dtype
        self.enc = [_CroCoBlockParams(b, f"enc_blocks[{i}]", dtype, False) for i, b in enumerate(matcher.enc_blocks)]
        self.dec1 = [_CroCoBlockParams(b, f"dec_blocks[{i}]", dtype, True) for i, b in enumerate(matcher.dec_blocks)]
        self.dec2 = [_CroCoBlockParams(b, f"dec_blocks2[{i}]", dtype, True) for i, b in enumerate(matcher.dec_blocks2)]
        de = matcher.decoder_embed
        if not isinstance(de, torch.nn.Linear):
            raise GdHipError(f"{_WHO}: decoder_embed is {type(de).__name__}, not a Linear")
        self.wde = de.weight.detach().to(dtype).contiguous()
        self.bde = None if de.bias is None else de.bias.detach().float().contiguous()
        Cd = de.weight.shape[0]
        for p, nm in [(p, f"dec_blocks[{i}]") for i, p in enumerate(self.dec1)] + [(p, f"dec_blocks2[{i}]") for i, p in enumerate(self.dec2)]:
            if p.C != Cd:
                raise GdHipError(f"{_WHO}: {nm}: width {p.C} is not decoder_embed's {Cd}")
        self.dnorm = _affine_ln(matcher.dec_norm, Cd, "dec_norm", "dec_norm")

    # -- pieces ---------------------------------------------------------------------------------------------------------------------
    def _self_attn(self, p, x, pos, B, N):
        y, _, _ = ops.layernorm_fwd(x, *p.n1, save_stats=False, out_dtype=self.dtype)
        qkv = ops.gemm_nt(y, p.wqkv, bias=p.bqkv)
        ops.qk_norm_rope(qkv, B, N, p.H, pos, None, None, None, None, 0.0, p.base)      # null gamma / beta: plain RoPE of q and k
        o, _ = ops.attention_fwd(qkv, B, N, p.H)
        return ops.gemm_nt(o, p.wproj, out_dtype=torch.float32, bias=p.bproj, residual=x)

    def _mlp(self, p, x):
        y, _, _ = ops.layernorm_fwd(x, *p.nmlp, save_stats=False, out_dtype=self.dtype)
        h = ops.gemm_nt(y, p.w1, bias=p.b1, act=1)
        return ops.gemm_nt(h, p.w2, out_dtype=torch.float32, bias=p.b2, residual=x)

    def _enc_block(self, p, x, pos, B, N):
        """x [B*N, C] fp32 residual stream -> the same after one encoder block."""
        return self._mlp(p, self._self_attn(p, x, pos, B, N))

    def _dec_block(self, p, x, y, xpos, ypos, B, Nx, Ny):
        """x [B*Nx, C], y [B*Ny, C] fp32 (this view's tokens, the other view's: read only) -> (x after the block, camap [B, 1, Nx, Ny] fp32:
        the head mean of the raw scaled scores)."""
        from .rope import rope_2d
        dt, C, H = self.dtype, p.C, p.H
        x = self._self_attn(p, x, xpos, B, Nx)
        xn, _, _ = ops.layernorm_fwd(x, *p.n2, save_stats=False, out_dtype=dt)
        q = ops.gemm_nt(xn, p.wq, bias=p.bq)
        if p.ny is not None:
            yn, _, _ = ops.layernorm_fwd(y, *p.ny, save_stats=False, out_dtype=dt)
        else:
            yn = y if dt == torch.float32 else ops.cast(y, dt)                            # norm_mem=False: cast only
        kv = ops.gemm_nt(yn, p.wkv, bias=p.bkv)
        rope_2d(q.view(B, Nx, H, 64), xpos.view(B, Nx, 2), p.base, 1.0)                   # in place: ld_tok = C
        rope_2d(kv.view(B, Ny, 2 * H, 64)[:, :, :H], ypos.view(B, Ny, 2), p.base, 1.0)    # the k half: ld_tok = 2C
        camap = ops.gemm_nt(q.view(B, Nx, C), kv.view(B, Ny, 2 * C)[:, :, :C], out_dtype=torch.float32, alpha=64 ** -0.5 / H)
        o, _ = ops.cross_attention_fwd(q, kv, B, Nx, Ny, H)
        x = ops.gemm_nt(o, p.wcproj, out_dtype=torch.float32, bias=p.bcproj, residual=x)
        return self._mlp(p, x), camap.unsqueeze(1)

    @staticmethod
    def _flat(x, pos, C, what):
        if x.dim() != 3 or x.shape[2] != C or tuple(pos.shape) != (x.shape[0], x.shape[1], 2):
            raise GdHipError(f"{_WHO}: {what}: tokens {tuple(x.shape)} / pos {tuple(pos.shape)} do not fit width {C}")
        B, N, _ = x.shape
        return x.detach().reshape(B * N, C).float().contiguous(), pos.to(x.device).reshape(B * N, 2).long().contiguous(), B, N

    # -- the two entry points ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, x, pos):
        """x [B, N, C] (after the patch embedding), pos [B, N, 2] (y, x) -> [B, N, C] fp32 after all `enc_blocks` (`enc_norm` stays the user's)."""
        t, p2, B, N = self._flat(x, pos, self.enc[0].C if self.enc else x.shape[-1], "encode")
        for p in self.enc:
            t = self._enc_block(p, t, p2, B, N)
        return t.view(B, N, -1)

    @torch.no_grad()
    def decode(self, f1, pos1, f2, pos2):
        """-> (list(zip(*final_output)), camaps1, camaps2), the contract of `_decoder` (model.py:297-322): final_output = [(f1, f2), every
        layer's pair ...] as fp32 [B, N, C] tensors, the last pair through `dec_norm`; camaps1[l] [B, 1, N1, N2], camaps2[l] [B, 1, N2, N1]:
        one-head head means (see the class docstring).  Both sides of layer l read the PREVIOUS layer's pair."""
        Ce = self.wde.shape[1]
        t1, p1, B, N1 = self._flat(f1, pos1, Ce, "decode view 1")
        t2, p2, B2, N2 = self._flat(f2, pos2, Ce, "decode view 2")
        if B2 != B:
            raise GdHipError(f"{_WHO}: decode: the two views differ in batch size ({B}, {B2})")
        final = [(t1.view(B, N1, Ce), t2.view(B, N2, Ce))]
        embed = lambda t: ops.gemm_nt(t if self.dtype == torch.float32 else ops.cast(t, self.dtype), self.wde, out_dtype=torch.float32, bias=self.bde)
        x1, x2 = embed(t1), embed(t2)
        camaps1, camaps2 = [], []
        for pa, pb in zip(self.dec1, self.dec2):
            n1, c1 = self._dec_block(pa, x1, x2, p1, p2, B, N1, N2)
            n2, c2 = self._dec_block(pb, x2, x1, p2, p1, B, N2, N1)        # (x1 is still the previous layer's: nothing is updated in place)
            x1, x2 = n1, n2
            final.append((x1.view(B, N1, -1), x2.view(B, N2, -1)))
            camaps1.append(c1)
            camaps2.append(c2)
        last = tuple(ops.layernorm_fwd(t, *self.dnorm, save_stats=False, out_dtype=torch.float32)[0] for t in (x1, x2))
        final[-1] = (last[0].view(B, N1, -1), last[1].view(B, N2, -1))
        return list(zip(*final)), camaps1, camaps2
